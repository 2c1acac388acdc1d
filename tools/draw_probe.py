"""What the generators' per-row draws cost on the host and on the device.

(a) Per batch shape (20 x 40 960: a VoteTester batch; 6 x 40 960: TrainFeeder S3DIS; 4 x 65 536 with noise: TrainFeeder Semantic3D; 16 x 65 536
    with noise: a Semantic3D test-shaped batch): the host's draw (B permutations, and B x N x 3 float64 normals where the shape has noise), the
    upload of those arrays on a stream of its own, and the device fill (ssdr_draw_perm_dev, ssdr_draw_normal_dev) between HIP events
    (ssdr_prof_enable / ssdr_prof_report).  Median of --repeats after a warm-up, ms.
(b) One VoteTester epoch over tools/vote_probe.py's rooms in three readings: host draws inside the clock (what an evaluation runs), host draws
    made before the clock starts (section 16's reading), device draws.  The three are alternated after a warm-up of each, --repeats times, in
    one process; median and best, ms.

Prints one JSON line.  GPU only.  Usage: python tools/draw_probe.py [--rooms 68] [--steps 100] [--repeats 3] [--density 2000] [--skip-epoch]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ssdr-al_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [("vote_20x40960", 20, 40960, False), ("feed_s3dis_6x40960", 6, 40960, False), ("feed_sem3d_4x65536_noise", 4, 65536, True),
          ("sem3d_test_16x65536_noise", 16, 65536, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=68)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--density", type=float, default=2000.0)
    ap.add_argument("--skip-epoch", action="store_true", help="part (a) only")
    a = ap.parse_args()
    from ssdr_al import _lib, draws
    from ssdr_al._lib import DevArray
    L = _lib.lib()
    _lib.check(L.ssdr_init(0))
    med = lambda v: round(float(np.median(v)), 3)
    st = C.c_void_p(); _lib.check(L.ssdr_stream_create(C.byref(st))); s = st.value

    def prof_ms():
        return sum(float(line.split()[2]) for line in L.ssdr_prof_report().decode().splitlines() if line.startswith("draw_"))

    shapes = {}
    for name, B, N, noisy in SHAPES:
        d_perm = DevArray((B, N), np.int32)
        d_noise = DevArray((B, N, 3), np.float64) if noisy else None
        t_host, t_up, t_dev = [], [], []
        for rep in range(a.repeats + 1):
            rng = np.random.default_rng([0, 0, rep])
            c0 = time.perf_counter()
            perm = np.stack([rng.permutation(N) for _ in range(B)]).astype(np.int32)
            noise = rng.normal(scale=0.001, size=(B, N, 3)) if noisy else None
            c1 = time.perf_counter()
            _lib.check(L.ssdr_memcpy_h2d_on(d_perm.ptr, _lib.ptr(perm), perm.nbytes, s))
            if noisy:
                _lib.check(L.ssdr_memcpy_h2d_on(d_noise.ptr, _lib.ptr(noise), noise.nbytes, s))
            c2 = time.perf_counter()
            L.ssdr_prof_report(); L.ssdr_prof_enable(1)
            draws.perm(0, 0, rep, B, N, out=d_perm, stream=s)
            if noisy:
                draws.normal(0, 0, rep, draws.AUG_NOISE, B * N * 3, scale=0.001, out=d_noise, stream=s)
            _lib.sync(s)
            L.ssdr_prof_enable(0)
            dev = prof_ms()
            if rep:                                          # the first round warms up (scratch, code objects)
                t_host.append(1e3 * (c1 - c0)); t_up.append(1e3 * (c2 - c1)); t_dev.append(dev)
        shapes[name] = dict(host_draw_ms=med(t_host), upload_ms=med(t_up), device_fill_ms=med(t_dev),
                            upload_mb=round((B * N * 4 + (B * N * 24 if noisy else 0)) / 1e6, 2))
    out = dict(probe="draw", shapes=shapes)

    if not a.skip_epoch:
        from oracle import randla_np as R
        from ssdr_al import evaluate, subsampling, synthetic
        from ssdr_al.helper_tool import ConfigS3DIS

        class cfg(ConfigS3DIS):
            val_steps = a.steps
        clouds = []
        for i in range(a.rooms):
            xyz, rgb, lab = synthetic.make_room(30000 + i, density=a.density)
            sp, sc, sl = subsampling.compute(xyz, features=rgb.astype(np.float32), classes=lab.astype(np.int32), sampleDl=0.04)
            clouds.append(dict(xyz=sp, rgb=sc, labels=sl.reshape(-1).astype(np.int32)))
        sizes = [len(c["xyz"]) for c in clouds]
        W = R.init_weights(0)
        poss0 = [np.random.default_rng([0, c]).random(n) * 1e-3 for c, n in enumerate(sizes)]
        t0 = evaluate.VoteTester(W, clouds, config=cfg, possibility=poss0)
        made = [t0.draw(0, k) for k in range(a.steps)]
        t0.close()

        def epoch(mode):
            t = evaluate.VoteTester(W, clouds, config=cfg, possibility=poss0, draws="device" if mode == "device" else "host")
            _lib.sync(t.s_gen)
            c0 = time.perf_counter()
            t._epoch((lambda e, k: made[k]) if mode == "host_premade" else None)
            _lib.sync(t.s_net)
            ms = 1e3 * (time.perf_counter() - c0)
            t.close()
            return ms

        modes = ("host_inside", "host_premade", "device")
        for m in modes:
            epoch(m)                                         # warm-up
        times = {m: [] for m in modes}
        for _ in range(a.repeats):
            for m in modes:
                times[m].append(epoch(m))
        out.update(rooms=len(clouds), points=int(sum(sizes)), tiles=a.steps * cfg.val_batch_size, pads=bool(min(sizes) < cfg.num_points),
                   epoch_ms={m: dict(median=round(float(np.median(v)), 2), best=round(min(v), 2)) for m, v in times.items()})
        out["device_below_host_inside"] = bool(np.median(times["device"]) < np.median(times["host_inside"]))
    print(json.dumps(out))
    _lib.check(L.ssdr_stream_destroy(s))


if __name__ == "__main__":
    main()
