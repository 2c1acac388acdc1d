"""The selection half of one AL round at the reference's scale (272 clouds, batch_size 10 000: make_clouds(3, 272, 150, 20, 60,
labelled_per_cloud=15), the shape of tests/test_al_round.py) for the "fps", "edcd" and "topk" selectors, host clock around _select_issue +
_select_collect (the scoring has run; the collect waits for the device).  Also the edcd loop a caller had before the batched chain:
ssdr_cloud_graph_dev + ssdr_fps_superpoint_dev per cloud on the same stream (buffers and uploads prepared outside the timed window), and whether
its picks are those of the one call.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "ssdr-al_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from _fabricate import make_clouds
    from ssdr_al import _lib, pipeline
    from ssdr_al._lib import DevArray
    from ssdr_al.helper_tool import ConfigS3DIS
    L = _lib.lib()
    _lib.check(L.ssdr_init(0))
    reps = int(os.environ.get("SELECTOR_PROBE_REPS", "10"))
    nc = int(os.environ.get("SELECTOR_PROBE_CLOUDS", "272"))           # (fewer: a rehearsal on the CPU logic build)
    batch = 10000 * nc // 272
    clouds, labelled, sel_list = make_clouds(3, nc, 150, 20, 60, labelled_per_cloud=15)
    out = {"probe": "selector", "clouds": len(clouds), "batch_size": batch, "reps": reps}
    kw = dict(sampler_args=("sb", "WetSU", "clsbal", "edcd"), round_num=5, label_seed=9, batch_size=batch)
    res = {}
    for sel in ("fps", "edcd", "topk"):
        hp = pipeline.HotPath.from_clouds(clouds, labelled, sel_list, ConfigS3DIS, selector=sel, **kw)
        hp._score_async(None)
        for _ in range(2):                    # warm-up: code objects, scratch buffers
            hp._select_issue(None); hp._select_collect()
        ts = []
        for _ in range(reps):
            _lib.sync()
            t0 = time.perf_counter()
            hp._select_issue(None)
            r = hp._select_collect()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[sel + "_ms"] = [round(float(np.median(ts)), 3), round(float(min(ts)), 3)]
        res[sel] = (hp, r)
    hp, (sel, unl) = res["edcd"]
    out["picks"], out["candidates"] = len(sel), len(unl)
    out["candidates_equal_fps"] = bool(unl == res["fps"][1][1])
    # the per-cloud loop over the same candidates and pick counts
    cc, cand, si = np.asarray(unl.a), np.asarray(unl.b), np.asarray(sel, np.int64)
    ntop = np.bincount(cc[si], minlength=hp.B)
    first = np.concatenate([[0], np.cumsum(np.bincount(cc, minlength=hp.B))])
    jobs = []
    for b in np.flatnonzero(ntop > 0):
        c = cand[first[b]:first[b + 1]].astype(np.int32)
        n, k = len(c), int(ntop[b])
        msp = int((hp.sp_off_h[c + 1] - hp.sp_off_h[c]).max())
        jobs.append((b, n, k, msp, DevArray.from_host(c), DevArray((n, 3), np.float64), DevArray((n * n,), np.float64), DevArray((n * n,), np.float64),
                     DevArray((k,), np.int32)))
    _lib.check(L.ssdr_select_set_chamfer_mode(0))

    def loop():
        for b, n, k, msp, d_s, d_c, d_d, d_a, d_o in jobs:
            _lib.check(L.ssdr_cloud_graph_dev(hp.xyz.ptr, hp.sp_off.ptr, hp.sp_pts.ptr, d_s.ptr, n, msp, 0, d_c.ptr, d_d.ptr, d_a.ptr, None))
            _lib.check(L.ssdr_fps_superpoint_dev(d_c.ptr, d_d.ptr, n, 0, k, d_o.ptr, None))
        _lib.sync()
    loop()
    ts = []
    for _ in range(reps):
        _lib.sync()
        t0 = time.perf_counter()
        loop()
        ts.append((time.perf_counter() - t0) * 1e3)
    out["edcd_loop_ms"] = [round(float(np.median(ts)), 3), round(float(min(ts)), 3)]
    out["edcd_loop_clouds"] = len(jobs)
    same = True
    for b, n, k, msp, d_s, d_c, d_d, d_a, d_o in jobs:
        same &= si[cc[si] == b].tolist() == (d_o.to_host().astype(np.int64) + first[b]).tolist()
    out["loop_picks_identical"] = bool(same)
    out["speedup_vs_loop"] = round(out["edcd_loop_ms"][0] / out["edcd_ms"][0], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
