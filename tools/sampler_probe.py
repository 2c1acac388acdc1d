"""What one random round costs on the device and in NumPy.

A fabricated pool at the reference's scale (272 clouds, about 100 000 regions, 10 000 clicks, "dominant", min_size 5) goes through
HotPath(selector="random", draws="device"): step_selection() + label_selected(), all iterations, the host's reads included — against the in-memory
NumPy restatement of the same rule (tests/_sampler_oracle.py: no pickles, no PLY files, which is where the reference's own loop spends its time).
Both start from the same labelled mask every time; the two results are compared once.  Median of --repeats after a warm-up, ms.  The launches per
iteration are counted from the code (csrc/select_random.hip, csrc/select_label.hip, RadixSorter::sort_segments) for the pool's sizes.

--comm: the same round through the SHARDED form at world 1 (RCCL: ssdr_region_draw_count_dev -> all-gather -> ssdr_region_draw_sharded_dev, the walk in
its verdict / all-gather / walk halves) against the plain path, in one call, alternating, median of --repeats after a warm-up; also written to
profiles/sampler_probe_comm.json.  No multi-GPU figure: what it shows is what the two exchanges and the split chains cost where nothing is exchanged.

Prints one JSON line.  GPU only.  Usage: python tools/sampler_probe.py [--clouds 272] [--regions 100000] [--clicks 10000] [--repeats 3] [--comm]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ssdr-al_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_pool(rng, n_clouds, n_regions, num_labels=13):
    """clouds of uneven region counts, regions of 1 .. 60 points (a few up to 700), 90 % of a region's points carry its label"""
    share = rng.random(n_clouds) + 0.2
    counts = np.maximum(1, np.round(share / share.sum() * n_regions)).astype(np.int64)
    clouds = []
    for n in counts:
        sizes = np.where(rng.random(n) < 0.03, rng.integers(257, 701, n), rng.integers(1, 61, n))
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        npts = int(off[-1])
        base = np.repeat(rng.integers(0, num_labels, n), sizes)
        gt = np.where(rng.random(npts) < 0.9, base, rng.integers(0, num_labels, npts)).astype(np.int32)
        pts = np.arange(npts, dtype=np.int32)
        clouds.append(dict(components=[pts[off[s]:off[s + 1]] for s in range(n)], gt=gt, pred=np.zeros(npts, np.int32), offsets=off, points=pts))
    return clouds


def sort_launches(key_bits, n, wide_high):
    """RadixSorter::sort_segments: the AND/OR pre-pass and its fold, three launches per wide pass, the one-workgroup kernel for the rest, the finish"""
    allp = (max(key_bits, 1) + 7) // 8
    wide = wide_high and key_bits > 32 and n >= 16384
    return 2 + 3 * (allp if wide else min(4, allp)) + (1 if key_bits > 32 and not wide else 0) + 1


def comm_probe(a, hp, device_round, sort_launches):
    """the plain round and the sharded round at world 1, alternating"""
    import torch.distributed as dist
    from ssdr_al.distributed import Comm
    comm = Comm(dist, "cuda")
    device_round(); device_round(comm)                       # warm-up: scratch, code objects, the communicator's first collective
    t_plain, t_comm = [], []
    for _ in range(a.repeats):
        ms, plain = device_round(); t_plain.append(ms)
        ms, shard = device_round(comm); t_comm.append(ms)
    same = (plain.iterations == shard.iterations and all(np.array_equal(x, y) for x, y in zip(plain.drawn, shard.drawn)) and plain.used == shard.used
            and plain.counters == shard.counters and plain.budget_left == shard.budget_left and np.array_equal(plain.to_host(), shard.to_host()))
    rank_bits = 1
    while (1 << rank_bits) <= hp.B:
        rank_bits += 1
    # draw: count half (fill, count), the all-gather, sharded half (fill, live, keys, sort, share, take, pick keys, sort, emit); walk: the keys' upload, verdict half
    # (two fills, ident, two verdict forms, pack), the all-gather, walk half (three fills, record keys, the 64-bit sort, scan, two apply forms)
    draw = 2 + 7 + sort_launches(32, hp.S, False) + sort_launches(32 + rank_bits, hp.S, True)
    walk = 6 + 6 + sort_launches(64, a.clicks, True)
    med = lambda v: round(float(np.median(v)), 2)
    out = dict(probe="sampler_comm", world=1, backend="rccl", clouds=hp.B, regions=hp.S, clicks=a.clicks, iterations=shard.iterations,
               items_per_iteration=[len(x) for x in shard.drawn], plain_round_ms=dict(median=med(t_plain), best=round(min(t_plain), 2), all=[round(x, 2) for x in t_plain]),
               sharded_round_ms=dict(median=med(t_comm), best=round(min(t_comm), 2), all=[round(x, 2) for x in t_comm]),
               launches_per_iteration=dict(draw=draw, walk=walk, collectives=2, host_uploads=1), sharded_equals_plain=bool(same))
    with open(os.path.join(ROOT, "profiles", "sampler_probe_comm.json"), "w") as f:
        json.dump(out, f, indent=1); f.write("\n")
    print(json.dumps(out))
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=272)
    ap.add_argument("--regions", type=int, default=100000)
    ap.add_argument("--clicks", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--comm", action="store_true", help="time the sharded form at world 1 (RCCL) against the plain path")
    a = ap.parse_args()
    if a.comm:                                               # the framework takes the device first: one HIP runtime per process
        import torch
        import torch.distributed as dist
        for k, v in (("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29593"), ("RANK", "0"), ("WORLD_SIZE", "1")):
            os.environ.setdefault(k, v)
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    import _sampler_oracle as SO
    from ssdr_al import _lib, pipeline
    from ssdr_al.helper_tool import ConfigS3DIS
    _lib.check(_lib.lib().ssdr_init(0))
    rng = np.random.default_rng(29)
    clouds = make_pool(rng, a.clouds, a.regions)
    cl = [dict(xyz=np.zeros((len(c["gt"]), 3), np.float32), gt=c["gt"], probs=np.zeros((len(c["gt"]), 13), np.float32), feat=np.zeros((len(c["gt"]), 32), np.float32),
               offsets=c["offsets"], points=c["points"]) for c in clouds]
    seed, rnd, min_size = 7, 2, 5
    hp = pipeline.HotPath.from_clouds(cl, [set() for _ in clouds], [], ConfigS3DIS, selector="random", batch_size=a.clicks, min_size=min_size, draw_seed=seed, round_num=rnd)
    base = np.concatenate([np.asarray(hp.sp_base, np.int64), [hp.S]])
    n_pts = hp.n_pts

    def device_round(comm=None):
        hp.set_labeled({b: set() for b in range(hp.B)})
        hp.set_pseudo_gt(np.zeros((2, n_pts), np.float32))
        _lib.sync()
        c0 = time.perf_counter()
        hp.step_selection(comm)
        res = hp.label_selected(mode="dominant", comm=comm)
        return 1e3 * (time.perf_counter() - c0), res

    def numpy_round():
        lab = np.zeros(hp.S, bool)
        pseudo = [np.zeros((2, len(c["gt"])), np.float32) for c in clouds]
        c0 = time.perf_counter()
        exp = SO.random_round(seed, rnd, clouds, lab, base, pseudo, a.clicks, min_size)
        return 1e3 * (time.perf_counter() - c0), exp, pseudo

    if a.comm:
        return comm_probe(a, hp, device_round, sort_launches)
    device_round()                                           # warm-up: scratch, code objects
    t_dev, t_np = [], []
    for _ in range(a.repeats):
        ms, res = device_round(); t_dev.append(ms)
        ms, exp, pseudo = numpy_round(); t_np.append(ms)
    same = (res.iterations == exp["iterations"] and all(np.array_equal(x, e["items"]) for x, e in zip(res.drawn, exp["iters"]))
            and np.array_equal(res.to_host(), np.concatenate(pseudo, axis=1)) and res.counters == exp["counters"] and res.budget_left == exp["budget_left"])
    rank_bits = 1
    while (1 << rank_bits) <= hp.B:
        rank_bits += 1
    # ssdr_region_draw_dev: two fills, count, live, keys, sort, share, take, pick keys, sort, emit; ssdr_oracle_label_dev: three fills, first, keys, sort, two verdict
    # forms, scan, two apply forms
    draw = 2 + 5 + sort_launches(32, hp.S, False) + sort_launches(32 + rank_bits, hp.S, True) + 2
    walk = 3 + 2 + sort_launches(31, a.clicks, False) + 2 + 1 + 2
    med = lambda v: round(float(np.median(v)), 2)
    print(json.dumps(dict(probe="sampler", clouds=hp.B, regions=hp.S, points=n_pts, clicks=a.clicks, min_size=min_size, mode="dominant", iterations=res.iterations,
                          items_per_iteration=[len(x) for x in res.drawn], used=len(res.used), budget_left=res.budget_left,
                          device_round_ms=dict(median=med(t_dev), best=round(min(t_dev), 2)), numpy_round_ms=dict(median=med(t_np), best=round(min(t_np), 2)),
                          launches_per_iteration=dict(draw=draw, walk=walk), device_equals_numpy=bool(same))))


if __name__ == "__main__":
    main()
