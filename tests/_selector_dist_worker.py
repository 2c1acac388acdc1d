"""Worker of tests/test_region_selectors.py: one rank of the sharded "edcd" / "topk" selection against ONE process over the union of the clouds.
SSDR_TEST_BACKEND=gloo: the CPU logic build, SSDR_TEST_SHARDS clouds per rank (e.g. "3,2,1"), SSDR_TEST_NOTOP_RANK = a rank whose regions all
rank last (no top region); nccl: world 1 on the GPU through RCCL.  The clouds come with fabricated network outputs (HotPath.from_clouds)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "ssdr-al_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))


def rank_last(cl, nc=13):
    """regions that rank last: a confident majority (class 1) and an uncertain minority (class 2) — WetSU counts the minority against the region"""
    probs = np.empty((len(cl["xyz"]), nc), np.float32)
    off, pts = cl["offsets"], cl["points"]
    for s in range(len(off) - 1):
        ids = pts[off[s]:off[s + 1]]
        k = len(ids) // 2 + 1
        p = np.full(nc, (0.02 - 1e-5 * s) / (nc - 1), np.float32); p[1] = 0.98 + 1e-5 * s
        q = np.full(nc, 0.92 / (nc - 1), np.float32); q[2] = 0.08
        probs[ids[:k]], probs[ids[k:]] = p, q
    return dict(cl, probs=probs)


def main():
    import torch.distributed as dist
    backend = os.environ.get("SSDR_TEST_BACKEND", "gloo")
    if backend == "nccl":
        import torch
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from _fabricate import make_clouds
    from ssdr_al import _lib, pipeline
    from ssdr_al.distributed import Comm
    from ssdr_al.helper_tool import ConfigS3DIS
    if backend == "gloo":
        _lib.use(os.path.join(ROOT, "tests", "hipemu", "libssdr_al_emu.so"))
    else:
        _lib.check(_lib.lib().ssdr_init(0))
    shards = [int(x) for x in os.environ.get("SSDR_TEST_SHARDS", "4").split(",")]
    assert len(shards) == world
    notop = int(os.environ.get("SSDR_TEST_NOTOP_RANK", "-1"))
    first = [sum(shards[:r]) for r in range(world + 1)]
    clouds, labelled, sel_list = make_clouds(78, first[-1], (30, 50), 6, 30, labelled_per_cloud=5)
    if notop >= 0:
        for b in range(first[notop], first[notop + 1]):
            clouds[b] = rank_last(clouds[b])
    mine = list(range(first[rank], first[rank + 1]))
    comm = Comm(dist, "cuda" if backend == "nccl" else "cpu")
    res = {"rank": rank, "rooms": mine}
    kw = dict(sampler_args=("sb", "WetSU", "clsbal", "edcd"), min_size=8, round_num=3, label_seed=31, batch_size=40)
    for selector in ("edcd", "topk"):
        hp = pipeline.HotPath.from_clouds([clouds[i] for i in mine], [labelled[i] for i in mine], sel_list, ConfigS3DIS, room_ids=mine, selector=selector, **kw)
        hp.step_selection(comm)
        res[selector], res[selector + "_path"] = hp.selected, hp.rule_path
        os.environ["SSDR_SELECT_HOST_RULE"] = "1"
        hp.step_selection(comm)
        res[selector + "_host_equal"] = hp.selected == res[selector] and hp.rule_path == "host"
        del os.environ["SSDR_SELECT_HOST_RULE"]
        if rank == 0:
            one = pipeline.HotPath.from_clouds(clouds, labelled, sel_list, ConfigS3DIS, selector=selector, **kw)
            one.step_selection()
            res[selector + "_single"] = one.selected
    with open(os.path.join(os.environ["SSDR_TEST_OUT"], "rank%d.json" % rank), "w") as f:
        json.dump(res, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
