"""Worker of tests/test_sharded_round.py: one rank of a sharded AL round — selection, the oracle over all ranks' picks, the next selection — against
ONE process over the union of the clouds.  SSDR_TEST_BACKEND=gloo: the CPU logic build, SSDR_TEST_SHARDS clouds per rank (e.g. "3,2,1"),
SSDR_TEST_NOTOP_RANK = a rank whose regions all rank last; nccl: world 1 on the GPU through RCCL.  SSDR_TEST_PART: "select" (HotPath.from_clouds over
fabricated network outputs, every selector) or "alround" (pipeline.ALRound).  Every rank writes rank<r>.npz; rank 0 adds the single-process run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "ssdr-al_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))

FPS_ARGS = ("sb", "WetSU", "clsbal", "gcn_fps")
EDCD_ARGS = ("sb", "WetSU", "clsbal", "edcd")
LABEL = dict(mode="NAIL", threshold=0.75, min_size=3)      # (sub-regions of more than 3 points: some regions split)


def pairs(x):
    return np.asarray([tuple(p) for p in x], np.int64).reshape(-1, 2)


def put_label(res, key, hp, r, global_cloud):
    """what a labelling left behind: used (+ walk positions), counters, budget, class list, the pseudo labels per (global) cloud"""
    res[key + "used"], res[key + "walk_pos"] = pairs(r.used), np.asarray(r.walk_pos, np.int64)
    res[key + "counters"] = np.asarray([r.counters[k] for k in sorted(r.counters)] + [r.budget_left, r.forms["wave"], r.forms["block"]], np.int64)
    res[key + "class_list"] = hp.selected_class_list.to_host()
    res[key + "entries"] = np.asarray(r.class_entries, np.int64)
    for b in range(hp.B):
        res[key + "pseudo%d" % global_cloud[b]] = r.to_host(b)
    res[key + "labeled"] = pairs(sorted((global_cloud[b], int(s) - hp.sp_base[b]) for b in range(hp.B) for s in hp.labeled[b]))


def oracle_facts(one, picks, budget, skip_before, order_before, edcd):
    """from the NumPy oracle over the single-process picks: picks left unused, regions split, and which clouds had a pick processed"""
    import _labeling_oracle as O
    from test_oracle_labeling import _oracle_clouds
    oc = _oracle_clouds(one)
    cloud_order = None
    if edcd:
        ranked = order_before[~skip_before[order_before]]
        cloud_order = list(dict.fromkeys(one.sp_cloud_h[ranked].tolist()))
    exp = O.label_round([tuple(p) for p in picks], oc, [np.zeros((2, len(c["gt"])), np.float32) for c in oc], LABEL["mode"], LABEL["threshold"], budget, LABEL["min_size"], [], cloud_order)
    return exp, np.asarray([len(picks) - len(exp["used"]), exp["counters"]["split_sp_num"]], np.int64)


def part_select(comm, rank, world, backend, res):
    from _fabricate import make_clouds
    from ssdr_al import pipeline
    from ssdr_al.helper_tool import ConfigS3DIS
    shards = [int(x) for x in os.environ.get("SSDR_TEST_SHARDS", "6").split(",")]
    assert len(shards) == world
    notop = int(os.environ.get("SSDR_TEST_NOTOP_RANK", "-1"))
    first = [sum(shards[:r]) for r in range(world + 1)]
    clouds, labelled, sel_list = make_clouds(78, first[-1], (30, 50), 6, 30, labelled_per_cloud=5)
    if notop >= 0:
        from _selector_dist_worker import rank_last
        for b in range(first[notop], first[notop + 1]):
            clouds[b] = rank_last(clouds[b])
    mine = list(range(first[rank], first[rank + 1]))
    res["rooms"] = np.asarray(mine, np.int64)
    batch, budget = 40, 33
    for selector in ("fps", "kcenter", "edcd", "topk"):
        kw = dict(sampler_args=EDCD_ARGS if selector == "edcd" else FPS_ARGS, min_size=8, round_num=3, label_seed=31, batch_size=batch, selector=selector)
        for rule in ("device", "host"):
            key = "%s_%s_" % (selector, rule)
            if rule == "host":
                os.environ["SSDR_SELECT_HOST_RULE"] = "1"
            try:
                hp = pipeline.HotPath.from_clouds([clouds[i] for i in mine], [labelled[i] for i in mine], sel_list, ConfigS3DIS, room_ids=mine, **kw)
                hp.step_selection(comm)
                res[key + "path"] = np.asarray([{"host": 0, "sharded-device": 1}[hp.rule_path]])
                res[key + "selected"] = pairs(hp.selected)
                try:
                    hp.label_selected(budget=budget, **LABEL)
                    res[key + "refused"] = np.asarray([0])
                except ValueError as e:
                    res[key + "refused"] = np.asarray([int("communicator" in str(e))])
                put_label(res, key, hp, hp.label_selected(budget=budget, comm=comm, **LABEL), mine)
                hp.step_selection(comm)
                res[key + "selected2"] = pairs(hp.selected)
            finally:
                os.environ.pop("SSDR_SELECT_HOST_RULE", None)
        if rank == 0:
            key = "%s_single_" % selector
            one = pipeline.HotPath.from_clouds(clouds, labelled, sel_list, ConfigS3DIS, **kw)
            one.step_selection()
            res[key + "selected"] = pairs(one.selected)
            skip_before, order_before = one.skip_mask.copy(), one.sorted_inds.to_host().astype(np.int64)
            exp, facts = oracle_facts(one, one.selected, budget, skip_before, order_before, selector == "edcd")
            put_label(res, key, one, one.label_selected(budget=budget, **LABEL), list(range(len(clouds))))
            assert [tuple(p) for p in res[key + "used"].tolist()] == exp["used"]           # (the single-process labelling is the oracle's)
            res[key + "facts"] = facts
            res[key + "used_clouds"] = np.asarray(sorted({c for c, _ in exp["used"]}), np.int64)
            one.step_selection()
            res[key + "selected2"] = pairs(one.selected)


def part_alround(comm, rank, world, backend, res):
    from oracle import randla_np as R
    from ssdr_al import pipeline, synthetic
    from ssdr_al.helper_tool import ConfigS3DIS
    gpu = backend == "nccl"

    class Cfg(ConfigS3DIS):
        num_points = 8192 if gpu else 512
    rooms = [synthetic.make_room(8100 + i, density=800.0 if gpu else 70.0) for i in range(2)]
    W = R.init_weights(0)
    kw = dict(batch_size=24, round_num=2, labeled_per_tile=3, precision="f32")
    try:
        pipeline.ALRound(W, rooms, world - 1, Cfg, comm=comm, **kw)
        res["refused"] = np.asarray([0])
    except ValueError:
        res["refused"] = np.asarray([1])
    ar = pipeline.ALRound(W, rooms, 3, Cfg, comm=comm, **kw)
    res["batches"] = np.asarray(ar.batch_ids, np.int64)

    def rounds(a, key, ids):
        a.run()
        res[key + "selected"] = pairs(a.sel.selected)
        res[key + "path"] = np.asarray([{"host": 0, "device": 2, "sharded-device": 1}[a.sel.rule_path]])
        put_label(res, key, a.sel, a.label(mode="NAIL", threshold=0.7), ids)
        if not gpu:
            a.run()
            res[key + "selected2"] = pairs(a.sel.selected)
    rounds(ar, "sharded_", ar.sel.room_ids)
    if rank == 0:
        one = pipeline.ALRound(W, rooms, 3, Cfg, **kw)
        rounds(one, "single_", list(range(6)))


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
    from ssdr_al import _lib
    from ssdr_al.distributed import Comm
    if backend == "gloo":
        _lib.use(os.path.join(ROOT, "tests", "hipemu", "libssdr_al_emu.so"))
    else:
        _lib.check(_lib.lib().ssdr_init(0))
    comm = Comm(dist, "cuda" if backend == "nccl" else "cpu")
    res = {}
    {"select": part_select, "alround": part_alround}[os.environ.get("SSDR_TEST_PART", "select")](comm, rank, world, backend, res)
    np.savez(os.path.join(os.environ["SSDR_TEST_OUT"], "rank%d.npz" % rank), **res)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
