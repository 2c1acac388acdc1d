"""Worker of tests/test_sharded_samplers.py: one rank of the sharded seed, random and label-all rounds — HotPath.seed_round(comm=),
step_selection(comm) + label_selected(comm=comm) of "random" / "all", pipeline.ALRound(selector="random", comm=) — beside ONE process over the union of the
clouds and the NumPy oracle (tests/_sampler_oracle.py) over it.  SSDR_TEST_BACKEND=gloo: the CPU logic build, SSDR_TEST_SHARDS clouds per rank (e.g.
"3,2,1"); nccl: world 1 on the GPU through RCCL.  SSDR_TEST_PART: "cases" (HotPath.from_clouds over the pool of test_region_samplers.py), "alround", "reload"
(one HotPath that gets load_rooms() twice, with other rooms, under the same communicator) or "all".  Every rank writes rank<r>.npz; rank 0 adds the single-process runs and the oracle's results."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "ssdr-al_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))

REGIONS = [40, 7, 25, 30, 3, 50]
SEED, RND = 5, 2
# name -> what runs: a random / label-all round of `budget` clicks, or a seed round of `seed` regions; pre: clouds labelled throughout beforehand
CASES = dict(rand60=dict(budget=60, min_size=8), nail60=dict(budget=60, min_size=8, mode="NAIL"), pre34=dict(budget=60, min_size=8, pre=(3, 4)),
             all155=dict(budget=155, min_size=1), maxiter=dict(budget=150, min_size=45), labelall=dict(budget=100, min_size=7, selector="all"),
             seed60=dict(seed=60), seed150=dict(seed=150), seed155=dict(seed=155), seedpre34=dict(seed=60, pre=(3, 4)))


def cat(parts, dtype=np.int64):
    parts = [np.asarray(p, dtype).reshape(-1) for p in parts]
    return (np.concatenate(parts) if parts else np.zeros(0, dtype)), np.asarray([len(p) for p in parts], np.int64)


def put(out, key, hp, r):
    """what a round left behind; regions as (room id, region in room) pairs: the test turns them into ids of the union"""
    out[key + "head"] = np.asarray([r.iterations, r.status, r.budget_left], np.int64)
    out[key + "counters"] = np.asarray([r.counters[k] for k in sorted(r.counters)], np.int64)
    out[key + "entries"], out[key + "class_list"] = np.asarray(r.class_entries, np.int64), np.asarray(hp._class_list_h, np.int64)
    drawn, out[key + "drawn_n"] = cat(r.drawn)
    out[key + "drawn"] = np.stack(hp._room_sp(drawn), axis=1)
    out[key + "pos"], _ = cat(r.item_pos if r.item_pos is not None else [np.arange(len(d)) for d in r.drawn])
    out[key + "info"] = np.asarray([[i["k"], i["live"], i["remain"], i["items"]] for i in r.draw_info], np.int64).reshape(-1, 4)
    out[key + "each"], out[key + "each_n"] = cat([i["each"] for i in r.draw_info])
    out[key + "used"] = np.asarray(r.used, np.int64).reshape(-1, 2)
    if r.walk_pos is not None:
        out[key + "walk_pos"], out[key + "walk_n"] = cat(r.walk_pos)
    out[key + "pseudo"], out[key + "labeled"] = r.to_host(), hp.labeled_mask.copy()


def put_oracle(out, key, e, pseudo, lab):
    """the oracle's round over the union, in the same words (regions as ids of the union)"""
    seed = "sp_num" in e
    out[key + "head"] = np.asarray([e["iterations"], 256 if e.get("stopped") else 0, e["remain"] if seed else e["budget_left"]], np.int64)
    c = dict(sp_num=e["sp_num"], p_num=e["p_num"], sub_num=0, sub_p_num=0, split_sp_num=0, ignore_sp_num=0) if seed else e["counters"]
    out[key + "counters"] = np.asarray([c[k] for k in sorted(c)], np.int64)
    out[key + "entries"] = np.asarray([] if seed else e["class_entries"], np.int64)
    out[key + "drawn"], out[key + "drawn_n"] = cat([d["items"] for d in e["iters"]])
    if "k" in e["iters"][0]:
        out[key + "info"] = np.asarray([[d["k"], len(d["live"]), d["remain"], len(d["items"])] for d in e["iters"]], np.int64)
        out[key + "each"], out[key + "each_n"] = cat([d["each"] for d in e["iters"]])
        out[key + "live"], _ = cat([d["live"] for d in e["iters"]])
    out[key + "used"] = np.asarray(e["used"], np.int64)
    out[key + "pseudo"], out[key + "labeled"] = np.concatenate(pseudo, axis=1), lab.copy()


def refusals(comm, clouds, mine, out):
    """draws="host" and "coregcn" with a communicator: raised before any exchange (every rank gets here, and on to the next collective)"""
    from test_region_samplers import _hot_path
    got = []
    sub = [clouds[i] for i in mine]
    for what in ("select", "seed"):
        hp = _hot_path(sub, None, "random", draws="host", batch_size=10, room_ids=mine)
        try:
            hp.step_selection(comm) if what == "select" else hp.seed_round(5, comm=comm)
            got.append(0)
        except ValueError as e:
            got.append(int('draws="host"' in str(e)))
    try:
        _hot_path(sub, None, "coregcn", batch_size=10, room_ids=mine).step_selection(comm)
        got.append(0)
    except ValueError as e:
        got.append(int("coregcn" in str(e) and "communicator" in str(e)))
    hp = _hot_path(sub, None, "random", batch_size=10, room_ids=mine)
    hp.step_selection(comm)
    try:
        hp.label_selected(mode="dominant")                           # (drawn with a communicator, labelled without: refused before any exchange)
        got.append(0)
    except ValueError as e:
        got.append(int("communicator" in str(e)))
    hp.label_selected(mode="dominant", comm=comm)
    out["refusals"] = np.asarray(got, np.int64)


def part_cases(comm, rank, world, out):
    import _sampler_oracle as SO
    from test_region_samplers import _hot_path, _pool
    shards = [int(x) for x in os.environ.get("SSDR_TEST_SHARDS", "6").split(",")]
    assert len(shards) == world and sum(shards) == len(REGIONS)
    first = np.concatenate([[0], np.cumsum(shards)])
    mine = list(range(first[rank], first[rank + 1]))
    gbase = np.concatenate([[0], np.cumsum(REGIONS)]).astype(np.int64)
    out["rooms"], out["gbase"] = np.asarray(mine, np.int64), gbase
    clouds = _pool(11, REGIONS, big=0.1)
    assert [len(c["components"]) for c in clouds] == REGIONS

    def run(case, ids, cm):
        c = CASES[case]
        labeled = [set(range(REGIONS[i])) if i in c.get("pre", ()) else set() for i in ids]
        kw = dict(draw_seed=SEED, round_num=RND, room_ids=ids)
        if "seed" in c:
            hp = _hot_path([clouds[i] for i in ids], labeled, "random", **kw)
            return hp, hp.seed_round(c["seed"], 0, comm=cm)
        mode = c.get("mode", "dominant")
        hp = _hot_path([clouds[i] for i in ids], labeled, c.get("selector", "random"), nail=mode == "NAIL", batch_size=c["budget"], min_size=c["min_size"], **kw)
        sel, unl = hp.step_selection(cm)
        assert np.array_equal(sel, np.arange(len(sel))) and len(unl.b) == len(sel)
        return hp, hp.label_selected(mode=mode, comm=cm)
    for case, c in CASES.items():
        put(out, case + "_sharded_", *run(case, mine, comm))
        if rank == 0:
            put(out, case + "_single_", *run(case, list(range(len(REGIONS))), None))
            lab = np.zeros(int(gbase[-1]), bool)
            for i in c.get("pre", ()):
                lab[gbase[i]:gbase[i + 1]] = True
            pseudo = [np.zeros((2, len(x["gt"])), np.float32) for x in clouds]
            if "seed" in c:
                e = SO.seed_round(SEED, 0, clouds, lab, gbase, pseudo, c["seed"])
            elif c.get("selector") == "all":
                e = SO.all_round(clouds, lab, gbase, pseudo, c["budget"])
            else:
                e = SO.random_round(SEED, RND, clouds, lab, gbase, pseudo, c["budget"], c["min_size"], c.get("mode", "dominant"))
            put_oracle(out, case + "_oracle_", e, pseudo, lab)
    refusals(comm, clouds, mine, out)


def part_alround(comm, rank, world, backend, out):
    """ALRound: seed, then two random rounds with run() + label(), 3 batches of 2 tiles over the ranks"""
    import _sampler_oracle as SO
    from oracle import randla_np as R
    from ssdr_al import pipeline, synthetic
    from ssdr_al.helper_tool import ConfigS3DIS
    gpu = backend == "nccl"

    class Cfg(ConfigS3DIS):
        num_points = 4096 if gpu else 512
    rooms = [synthetic.make_room(8300 + i, density=600.0 if gpu else 70.0) for i in range(2)]
    kw = dict(batch_size=14, round_num=3, labeled_per_tile=0, selector="random", draw_seed=21, min_size=4)

    def rounds(ar, key):
        ar.sel.record_shares = True
        put(out, key + "seed_", ar.sel, ar.seed(11))
        for i in (1, 2):
            sel, unl = ar.run()
            assert len(sel) == len(unl.b)
            put(out, key + "round%d_" % i, ar.sel, ar.label(mode="dominant"))
    ar = pipeline.ALRound(R.init_weights(0), rooms, 3, Cfg, comm=comm, **kw)
    out["al_batches"], out["al_rooms"] = np.asarray(ar.batch_ids, np.int64), np.asarray(ar.sel.room_ids, np.int64)
    rounds(ar, "al_sharded_")
    if rank == 0:
        one = pipeline.ALRound(R.init_weights(0), rooms, 3, Cfg, **kw)
        S, N = one.sel, Cfg.num_points
        gt = one.tile_l.to_host()
        base = np.concatenate([np.asarray(S.sp_base, np.int64), [S.S]])
        out["al_gbase"] = base
        clouds = []
        for t in range(S.B):
            off = S.sp_off_h[base[t]: base[t + 1] + 1].astype(np.int64)
            clouds.append(dict(components=[S.sp_pts_h[off[s]:off[s + 1]].astype(np.int64) - t * N for s in range(len(off) - 1)], gt=gt[t * N:(t + 1) * N]))
        rounds(one, "al_single_")
        lab = np.zeros(S.S, bool)
        pseudo = [np.zeros((2, N), np.float32) for _ in clouds]
        put_oracle(out, "al_oracle_seed_", SO.seed_round(21, 0, clouds, lab, base, pseudo, 11), pseudo, lab)
        for i in (1, 2):
            put_oracle(out, "al_oracle_round%d_" % i, SO.random_round(21, 3, clouds, lab, base, pseudo, 14, 4), pseudo, lab)


def part_reload(comm, rank, world, backend, out):
    """ONE HotPath per rank, load_rooms() with a share of the rooms, a seed and a random round, then load_rooms() again with OTHER shares (more rooms and more
    regions than any rank held before on rank 0) under the same communicator: nothing of the first pool's tables may survive"""
    import _sampler_oracle as SO
    from ssdr_al import pipeline, synthetic
    from ssdr_al.helper_tool import ConfigS3DIS
    gpu = backend == "nccl"

    class Cfg(ConfigS3DIS):
        num_points = 4096 if gpu else 512
    N = Cfg.num_points
    kw = dict(selector="random", batch_size=20, min_size=3, draw_seed=33, round_num=1, labeled_per_tile=2)
    shares = {1: ([3], [4]), 2: ([1, 2], [3, 1]), 3: ([1, 2, 1], [3, 1, 2])}[world]
    hp = pipeline.HotPath(None, Cfg, **kw)
    one = pipeline.HotPath(None, Cfg, **kw) if rank == 0 else None

    def rounds(h, key, cm):
        h.record_shares = True
        h.set_pseudo_gt(np.zeros((2, h.n_pts), np.float32))
        put(out, key + "seed_", h, h.seed_round(9, 0, comm=cm))
        h.step_selection(cm)
        put(out, key + "random_", h, h.label_selected(mode="dominant", comm=cm))
    for load, share in enumerate(shares):
        first = np.concatenate([[0], np.cumsum(share)])
        rooms = [synthetic.make_room(8500 + 10 * load + i, density=600.0 if gpu else 70.0) for i in range(int(first[-1]))]
        mine = list(range(int(first[rank]), int(first[rank + 1])))
        hp.load_rooms([rooms[i] for i in mine], mine)
        key = "reload%d_" % load
        out[key + "rooms"], out[key + "S"] = np.asarray(mine, np.int64), np.asarray([hp.S, hp.B], np.int64)
        rounds(hp, key + "sharded_", comm)
        if rank == 0:
            one.load_rooms(rooms)
            base = np.concatenate([np.asarray(one.sp_base, np.int64), [one.S]])
            out[key + "gbase"] = base
            gt = one.tile_l.to_host()
            clouds = []
            for t in range(one.B):
                off = one.sp_off_h[base[t]: base[t + 1] + 1].astype(np.int64)
                clouds.append(dict(components=[one.sp_pts_h[off[s]:off[s + 1]].astype(np.int64) - t * N for s in range(len(off) - 1)], gt=gt[t * N:(t + 1) * N]))
            lab = one.labeled_mask.copy()
            assert lab.sum() == 2 * one.B
            rounds(one, key + "single_", None)
            pseudo = [np.zeros((2, N), np.float32) for _ in clouds]
            put_oracle(out, key + "oracle_seed_", SO.seed_round(33, 0, clouds, lab, base, pseudo, 9), pseudo, lab)
            put_oracle(out, key + "oracle_random_", SO.random_round(33, 1, clouds, lab, base, pseudo, 20, 3), pseudo, lab)


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
    out = {}
    part = os.environ.get("SSDR_TEST_PART", "cases")
    if part in ("cases", "all"):
        part_cases(comm, rank, world, out)
    if part in ("alround", "all"):
        part_alround(comm, rank, world, backend, out)
    if part in ("reload", "all"):
        part_reload(comm, rank, world, backend, out)
    np.savez(os.path.join(os.environ["SSDR_TEST_OUT"], "rank%d.npz" % rank), **out)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
