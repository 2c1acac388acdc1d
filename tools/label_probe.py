"""The labelling tail of one AL round at the reference's scale: 272 clouds, 40 800 regions of 20-60 points plus a handful of slabs of 5 000-40 000
points (the floors and walls a real partition hands over), 10 000 picks, NAIL at 0.9, ground truth noisy enough that a fair share of the regions
split.  Times, on one stream, ssdr_oracle_label_dev (host clock around the enqueue and the wait for the stream; pseudo labels, labelled mask and
budget are restored outside the timed window) against the restated reference loop a caller has today (tests/_labeling_oracle.py: _help's order +
oracle_labeling, per-point work in NumPy) over the same picks, and compares every output.  Prints one JSON line.
LABEL_PROBE_SHARDED=1 (needs torch.distributed with RCCL; world 1): the same workload through the sharded round's two halves in the same session —
verdict half, all-gather of the records on the stream, walk half ("sharded_ms") and the two halves without the all-gather ("halves_ms": at world 1 the
walk may read the verdict half's buffer directly), outputs compared with the one-call chain's."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "ssdr-al_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import _labeling_oracle as O
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    comm = None
    if os.environ.get("LABEL_PROBE_SHARDED"):         # (the framework initialises the GPU first, as in the sharded runs)
        import torch
        import torch.distributed as dist
        from ssdr_al.distributed import Comm
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29591")
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        comm = Comm(dist, "cuda")
    L = _lib.lib()
    _lib.check(L.ssdr_init(0))
    reps = int(os.environ.get("LABEL_PROBE_REPS", "10"))
    ncl = int(os.environ.get("LABEL_PROBE_CLOUDS", "272"))               # (fewer: a rehearsal on the CPU logic build)
    batch = 10000 * ncl // 272
    rng = np.random.default_rng(12)
    slabs = {int(c): int(n) for c, n in zip(rng.choice(ncl, min(6, ncl), replace=False), (5000, 9000, 14000, 22000, 31000, 40000))}
    clouds = []
    for c in range(ncl):
        sizes = rng.integers(20, 61, 150).tolist() + ([slabs[c]] if c in slabs else [])
        clouds.append(O.noisy_cloud(rng, sizes, purity=0.95, split=0.3))
    gt, pred, off, pts, cloud, base, p0 = O.concat_clouds(clouds)
    n, S = len(gt), len(off) - 1
    slab_ids = [int(base[c]) + 150 for c in slabs]
    rest = np.setdiff1d(np.arange(S), slab_ids)
    items = np.concatenate([slab_ids, rng.choice(rest, batch - len(slab_ids), replace=False)])
    items = items[rng.permutation(len(items))].astype(np.int32)
    M = len(items)
    cap = batch + 33
    d_gt, d_pred, d_off, d_pts, d_cloud = (DevArray.from_host(a) for a in (gt, pred, off, pts, cloud))
    d_items, d_n = DevArray.from_host(items), DevArray.from_host(np.array([M], np.int32))
    d_mask, d_label, d_labeled = DevArray((n,), np.float32), DevArray((n,), np.float32), DevArray((S,), np.uint8)
    d_budget, d_used, d_cls, d_proc, d_out = DevArray((1,), np.int64), DevArray((M,), np.uint8), DevArray((cap,), np.int32), DevArray((M,), np.int32), DevArray((12,), np.int64)
    zero_p, zero_s, b0 = np.zeros(n, np.float32), np.zeros(S, np.uint8), np.array([batch], np.int64)

    def restore():
        for d, a in ((d_mask, zero_p), (d_label, zero_p), (d_labeled, zero_s), (d_budget, b0)):
            _lib.check(L.ssdr_memcpy_h2d(d.ptr, _lib.ptr(a), a.nbytes))
        _lib.sync()

    def device():
        _lib.check(L.ssdr_oracle_label_dev(d_gt.ptr, d_pred.ptr, n, d_off.ptr, d_pts.ptr, S, d_cloud.ptr, ncl, d_items.ptr, d_n.ptr, M, None, int(np.diff(off).max()),
                                           13, 13, 1, 0.9, 1, d_budget.ptr, d_mask.ptr, d_label.ptr, d_used.ptr, d_labeled.ptr, d_cls.ptr, cap, d_proc.ptr, d_out.ptr, None))
        _lib.sync()
    ts = []
    for r in range(reps + 2):                 # two warm-ups: code objects, scratch buffers
        restore()
        t0 = time.perf_counter()
        device()
        if r >= 2:
            ts.append((time.perf_counter() - t0) * 1e3)
    out = d_out.to_host()
    picks = [(int(cloud[s]), int(s - base[cloud[s]])) for s in items]
    pseudo = [np.zeros((2, len(c["gt"])), np.float32) for c in clouds]
    t0 = time.perf_counter()
    exp = O.label_round(picks, clouds, pseudo, "NAIL", 0.9, batch, 1, [])
    host_ms = (time.perf_counter() - t0) * 1e3
    used, proc = d_used.to_host(), d_proc.to_host()
    same = (np.array_equal(np.stack([d_mask.to_host(), d_label.to_host()]), np.concatenate(exp["pseudo"], axis=1))
            and [picks[i] for i in proc if used[i]] == exp["used"] and d_cls.to_host()[: int(out[6])].tolist() == exp["class_list"]
            and [int(x) for x in out[:6]] == [exp["counters"][k] for k in O.COUNTERS] and int(out[7]) == exp["budget_left"] and int(out[8]) == 0)
    extra = {}
    if comm is not None:
        first = np.full(ncl, 1 << 30, np.int64)
        np.minimum.at(first, cloud[items], np.arange(M))
        d_keys = DevArray.from_host(((first[cloud[items]] << 32) | np.arange(M)).astype(np.uint64))
        RB = _lib.LABEL_RECORD_BYTES
        d_send, d_gath, d_pos = DevArray((M * RB,), np.uint8), DevArray((1, M * RB), np.uint8), DevArray((M,), np.int32)
        ref = [a.to_host() for a in (d_mask, d_label, d_labeled, d_used, d_out)] + [d_cls.to_host()[: int(out[6])], proc]

        def halves(gather):
            _lib.check(L.ssdr_oracle_label_verdict_dev(d_gt.ptr, d_pred.ptr, n, d_off.ptr, d_pts.ptr, S, d_items.ptr, d_n.ptr, M, d_keys.ptr, int(np.diff(off).max()), 13, 13, 1,
                                                       0.9, 1, d_send.ptr, None))
            if gather:
                comm.allgather_(d_send, d_gath, None)
            _lib.check(L.ssdr_oracle_label_walk_dev((d_gath if gather else d_send).ptr, 0, 1, d_pred.ptr, n, d_off.ptr, d_pts.ptr, S, d_items.ptr, d_n.ptr, M,
                                                    int(np.diff(off).max()), 13, d_budget.ptr, d_mask.ptr, d_label.ptr, d_used.ptr, d_labeled.ptr, d_cls.ptr, cap, d_pos.ptr,
                                                    d_out.ptr, None))
            _lib.sync()
        for name, gather in (("sharded_ms", True), ("halves_ms", False)):
            tt = []
            for r in range(reps + 2):
                restore()
                t0 = time.perf_counter()
                halves(gather)
                if r >= 2:
                    tt.append((time.perf_counter() - t0) * 1e3)
            extra[name] = [round(float(np.median(tt)), 3), round(float(min(tt)), 3)]
            got = [a.to_host() for a in (d_mask, d_label, d_labeled, d_used, d_out)] + [d_cls.to_host()[: int(out[6])]]
            pos = d_pos.to_host()
            extra[name.replace("_ms", "_identical")] = bool(all(np.array_equal(a, b) for a, b in zip(got, ref)) and np.array_equal(ref[6][pos[pos >= 0]], np.flatnonzero(pos >= 0)))
        ts2 = []
        for r in range(reps + 2):             # the plain path once more, behind the sharded runs: its own run-to-run spread in this session
            restore()
            t0 = time.perf_counter()
            device()
            if r >= 2:
                ts2.append((time.perf_counter() - t0) * 1e3)
        extra["device_ms_again"] = [round(float(np.median(ts2)), 3), round(float(min(ts2)), 3)]
        dist.destroy_process_group()
    print(json.dumps({"probe": "label", **extra, "clouds": ncl, "regions": S, "points": n, "picks": M, "slabs": sorted(slabs.values()), "reps": reps,
                      "device_ms": [round(float(np.median(ts)), 3), round(float(min(ts)), 3)], "host_loop_ms": round(host_ms, 1),
                      "counters": exp["counters"], "budget_left": exp["budget_left"], "class_entries": int(out[6]),
                      "wave_regions": int(out[10]), "workgroup_regions": int(out[11]), "identical": bool(same)}))


if __name__ == "__main__":
    main()
