"""Training-batch epochs (ssdr_al.training.TrainFeeder) at the two workloads' own sizes, against the loop a caller had before, on the same box,
the same clouds and the same draws:

  S3DIS       batches of 6 x 40 960 over synthetic S3DIS-like rooms (synthetic.make_room, sub-sampled at 0.04 m), one DataLoader pass.
              Before: per tile ssdr_tile_select_batch_dev around a centre formed on the host, the tile's rows read back, the activation / pseudo
              channels gathered on the host and uploaded, then the pyramid.
  Semantic3D  batches of 4 x 65 536 over larger clouds, train_steps batches.  Before: per tile ssdr_tile_select_possibility_dev with its minimum /
              arg-min read back (unweighted and centred on three axes: the entry has no other rule), rows and xyz read back, the channels gathered
              and the augment computed in NumPy, features uploaded, then the pyramid.

Both sides end with the pyramid (pool outputs included) finished on the device.  Alternated after a warm-up; prints one JSON line with the
median and best epoch times in ms.  GPU only.
Usage: python tools/feed_probe.py [--rooms 24] [--clouds 4] [--cloud-points 400000] [--steps 8] [--repeats 3]"""
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


def _pyramid(L, _lib, cfg, xyz, B, bufs, s):
    arr = C.c_void_p * cfg.num_layers
    r = np.asarray(cfg.sub_sampling_ratio, np.int32)
    _lib.check(L.ssdr_knn_pyramid_dev(xyz.ptr, B, cfg.num_points, cfg.num_layers, _lib.ptr(r), cfg.k_n, arr(*[a.ptr for a in bufs["neigh"]]),
                                      arr(*[a.ptr for a in bufs["pool"]]), arr(*[a.ptr for a in bufs["up"]]), s))


def _numpy_augment(xyz, rot, scale, noise):
    out = np.empty(xyz.shape, np.float64)
    for t in range(len(xyz)):
        c, s = rot[t]
        R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
        out[t] = np.matmul(xyz[t], R) * scale[t][None, :] + noise[t]
    return out.astype(np.float32)


def probe(dataset, clouds, cfg, repeats):
    from ssdr_al import _lib, training
    from ssdr_al._lib import DevArray
    L = _lib.lib()
    N, B, K, NL = cfg.num_points, cfg.batch_size, cfg.k_n, cfg.num_layers
    sizes = [len(c["xyz"]) for c in clouds]
    r = np.random.default_rng(1)
    pg = [np.stack([(r.random(n) < 0.3), r.integers(0, cfg.num_classes, n)]).astype(np.float32) for n in sizes]
    act_h, pse_h = np.concatenate([p[0] for p in pg]), np.concatenate([p[1] for p in pg])
    poss0 = [np.random.default_rng([0, c]).random(n) * 1e-3 for c, n in enumerate(sizes)]
    mk = lambda: training.TrainFeeder(clouds, pg, config=cfg, dataset=dataset, possibility=poss0 if dataset == "Semantic3D" else None, color_scale=1.0 / 255.0)
    f0 = mk()
    steps = f0.steps_per_epoch
    all_draws = [f0.draw(0, s) for s in range(steps)]
    off = f0.off
    f0.close()
    draws = lambda epoch, step: all_draws[step]

    def device_epoch():
        f = mk()
        _lib.sync(f.s_gen)
        c0 = time.perf_counter()
        for batch in f.epoch_batches(None, draws):
            pass                                                          # the consumer would enqueue its step here; release() follows
        _lib.sync(f.s_gen)
        ms = 1e3 * (time.perf_counter() - c0)
        f.check()
        f.close()
        return ms

    st = C.c_void_p(); _lib.check(L.ssdr_stream_create(C.byref(st))); s = st.value
    d_p = DevArray.from_host(np.concatenate([c["xyz"] for c in clouds])); d_c = DevArray.from_host(np.concatenate([c["rgb"] for c in clouds]).astype(np.float32))
    d_l = DevArray.from_host(np.concatenate([c["labels"] for c in clouds]).astype(np.int32))
    d_m = [DevArray.from_host(np.array([n, 0], np.int64)) for n in sizes]
    lv = [N]
    for q in cfg.sub_sampling_ratio:
        lv.append(lv[-1] // q)
    xyz, feat, idx, lab = DevArray((B, N, 3), np.float32), DevArray((B, N, 6), np.float32), DevArray((B, N), np.int32), DevArray((B, N), np.int32)
    d_act, d_pse = DevArray((B, N), np.float32), DevArray((B, N), np.float32)
    bufs = dict(neigh=[DevArray((B, lv[i], K), np.int32) for i in range(NL)], pool=[DevArray((B, lv[i + 1], K), np.int32) for i in range(NL)],
                up=[DevArray((B, lv[i], 1), np.int32) for i in range(NL)])
    d_perm, d_dup = DevArray((B, N), np.int32), DevArray.from_host(np.zeros((B, N), np.float32))
    d_min, d_arg = DevArray((1,), np.float64), DevArray((1,), np.int32)

    def loop_epoch():
        d_poss = DevArray.from_host(np.concatenate(poss0))
        mins = np.array([p.min() for p in poss0]); args = [int(np.argmin(p)) for p in poss0]
        _lib.sync(); _lib.sync(s)
        c0 = time.perf_counter()
        for k in range(steps):
            d = all_draws[k]
            b = len(d["noise"])
            _lib.check(L.ssdr_memcpy_h2d_on(d_perm.ptr, _lib.ptr(d["perm"]), d["perm"].nbytes, s))
            if d["dup"] is not None:
                _lib.check(L.ssdr_memcpy_h2d_on(d_dup.ptr, _lib.ptr(d["dup"]), d["dup"].nbytes, s))
            which = []
            for j in range(b):
                if dataset == "S3DIS":
                    c = int(d["cloud"][j]); o = int(off[c])
                    pick = (clouds[c]["xyz"][d["point"][j]] + d["noise"][j]).astype(np.float32)
                    off1 = np.array([0, sizes[c]], np.int64)
                    _lib.check(L.ssdr_tile_select_batch_dev(d_p.ptr + 12 * o, d_c.ptr + 12 * o, 3, d_m[c].ptr, _lib.ptr(off1), 1, _lib.ptr(pick), N, d_perm.ptr + 4 * j * N,
                                                            d_dup.ptr + 4 * j * N, 1.0 / 255.0, xyz.ptr + 12 * j * N, feat.ptr + 24 * j * N, idx.ptr + 4 * j * N,
                                                            d_l.ptr + 4 * o, lab.ptr + 4 * j * N, s))
                else:
                    c = int(np.argmin(mins)); o = int(off[c])
                    pick = (clouds[c]["xyz"][args[c]] + d["noise"][j]).astype(np.float32)
                    _lib.check(L.ssdr_tile_select_possibility_dev(d_p.ptr + 12 * o, d_c.ptr + 12 * o, 3, d_m[c].ptr, sizes[c], _lib.ptr(pick), N, d_perm.ptr + 4 * j * N,
                                                                  d_dup.ptr + 4 * j * N, 1.0 / 255.0, xyz.ptr + 12 * j * N, feat.ptr + 24 * j * N, idx.ptr + 4 * j * N,
                                                                  d_poss.ptr + 8 * o, d_min.ptr, d_arg.ptr, s))
                    mins[c] = d_min.to_host(s)[0]; args[c] = int(d_arg.to_host(s)[0])
                which.append(int(off[c]))
            rows = idx.to_host(s)[:b] + np.asarray(which)[:, None]
            a_h, p_h = np.ascontiguousarray(act_h[rows]), np.ascontiguousarray(pse_h[rows])
            _lib.check(L.ssdr_memcpy_h2d_on(d_act.ptr, _lib.ptr(a_h), a_h.nbytes, s)); _lib.check(L.ssdr_memcpy_h2d_on(d_pse.ptr, _lib.ptr(p_h), p_h.nbytes, s))
            if dataset == "Semantic3D":
                f_h = feat.to_host(s)
                f_h[:b, :, :3] = _numpy_augment(f_h[:b, :, :3], d["rot"], d["scale"], d["aug_noise"])
                _lib.check(L.ssdr_memcpy_h2d_on(feat.ptr, _lib.ptr(f_h), f_h.nbytes, s))
            _pyramid(L, _lib, cfg, xyz, b, bufs, s)
        _lib.check(L.ssdr_knn_status(s, None))
        return 1e3 * (time.perf_counter() - c0)

    device_epoch(); loop_epoch()
    t_dev, t_loop = [], []
    for _ in range(repeats):
        t_dev.append(device_epoch()); t_loop.append(loop_epoch())
    _lib.check(L.ssdr_stream_destroy(s))
    med = lambda v: round(float(np.median(v)), 2)
    return dict(dataset=dataset, clouds=len(clouds), points=int(sum(sizes)), min_points=int(min(sizes)), max_points=int(max(sizes)), batches=steps, batch=B, tile=N,
                feeder_ms=dict(median=med(t_dev), best=round(min(t_dev), 2)), loop_ms=dict(median=med(t_loop), best=round(min(t_loop), 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=24)
    ap.add_argument("--clouds", type=int, default=4)
    ap.add_argument("--cloud-points", type=int, default=400000)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--density", type=float, default=2000.0)
    a = ap.parse_args()
    from ssdr_al import _lib, subsampling, synthetic
    from ssdr_al.helper_tool import ConfigS3DIS, ConfigSemantic3D
    _lib.check(_lib.lib().ssdr_init(0))
    rooms = []
    for i in range(a.rooms):
        xyz, rgb, lab = synthetic.make_room(30000 + i, density=a.density)
        sp, sc, sl = subsampling.compute(xyz, features=rgb.astype(np.float32), classes=lab.astype(np.int32), sampleDl=0.04)
        rooms.append(dict(xyz=sp, rgb=sc, labels=sl.reshape(-1).astype(np.int32)))
    out = [probe("S3DIS", rooms, ConfigS3DIS, a.repeats)]
    r = np.random.default_rng(4)
    big = []
    for i in range(a.clouds):
        n = a.cloud_points + 1000 * i
        big.append(dict(xyz=(r.random((n, 3), dtype=np.float32) * np.array([60, 50, 8], np.float32)).astype(np.float32),
                        rgb=r.integers(0, 256, (n, 3)).astype(np.float32), labels=r.integers(0, 8, n).astype(np.int32)))

    class Sem(ConfigSemantic3D):
        train_steps = a.steps
    out.append(probe("Semantic3D", big, Sem, a.repeats))
    print(json.dumps(dict(probe="feed", depth=2, workloads=out)))


if __name__ == "__main__":
    main()
