"""Test-time voting epoch (ssdr_al.evaluate.VoteTester) over 68 synthetic S3DIS-like rooms (synthetic.make_room, sub-sampled by the product's
front end at 0.04 m): one epoch of val_steps x val_batch_size = 100 x 20 tiles of 40 960 points, against the per-tile loop a caller had
before (ssdr_tile_select_possibility_dev with its minimum / arg-min read back per tile, then per batch the pyramid, the network, and
ssdr_vote_smooth_dev per tile) on the same draws, the same initial map and the same network, in the same process.  The two are alternated
after a warm-up, 3 repeats each; the generator chain alone (ssdr_vote_tiles_dev on its stream, no network) is timed the same way.
Prints one JSON line: generator_us_per_tile, epoch_ms, loop_ms (median and best), launches_per_tile, identical (possibility map and
test_probs of the two paths, bit for bit).  The draws are made before the clock starts (the host draws 20 permutations of 40 960 per batch,
about 10 ms, for either path).  GPU only.  Usage: python tools/vote_probe.py [--rooms 68] [--steps 100] [--repeats 3] [--density 2000] [--points 40960] [--batch 20]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=68)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--density", type=float, default=2000.0)
    ap.add_argument("--points", type=int, default=0, help="tile size (default: the configuration's 40 960)")
    ap.add_argument("--batch", type=int, default=0, help="tiles per batch (default: the configuration's 20)")
    a = ap.parse_args()
    from oracle import randla_np as R
    from ssdr_al import _lib, evaluate, randlanet, subsampling, synthetic
    from ssdr_al._lib import DevArray
    from ssdr_al.helper_tool import ConfigS3DIS
    L = _lib.lib()
    _lib.check(L.ssdr_init(0))

    class cfg(ConfigS3DIS):
        val_steps = a.steps
        num_points = a.points or ConfigS3DIS.num_points
        val_batch_size = a.batch or ConfigS3DIS.val_batch_size
    clouds = []
    for i in range(a.rooms):
        xyz, rgb, lab = synthetic.make_room(30000 + i, density=a.density)
        sp, sc, sl = subsampling.compute(xyz, features=rgb.astype(np.float32), classes=lab.astype(np.int32), sampleDl=0.04)
        clouds.append(dict(xyz=sp, rgb=sc, labels=sl.reshape(-1).astype(np.int32)))
    sizes = [len(c["xyz"]) for c in clouds]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    W = R.init_weights(0)
    N, B, Cn, K, NL = cfg.num_points, cfg.val_batch_size, cfg.num_classes, cfg.k_n, cfg.num_layers
    poss0 = [np.random.default_rng([0, c]).random(n) * 1e-3 for c, n in enumerate(sizes)]
    t0 = evaluate.VoteTester(W, clouds, config=cfg, possibility=poss0)
    all_draws = [t0.draw(0, s) for s in range(a.steps)]
    for d in all_draws:
        if d["dup"] is None:
            d["dup"] = np.zeros((B, N), np.float32)
    t0.close()
    draws = lambda epoch, step: all_draws[step]

    def device_epoch():
        t = evaluate.VoteTester(W, clouds, config=cfg, possibility=poss0)
        _lib.sync(t.s_gen)
        c0 = time.perf_counter()
        t._epoch(draws)
        _lib.sync(t.s_net)
        ms = 1e3 * (time.perf_counter() - c0)
        out = (np.concatenate(t.possibility()), t.probs_host())
        t.close()
        return ms, out

    def generator_alone():
        t = evaluate.VoteTester(W, clouds, config=cfg, possibility=poss0)
        _lib.sync(t.s_gen)
        c0 = time.perf_counter()
        for s in range(a.steps):
            t._generate(all_draws[s])
        _lib.sync(t.s_gen)
        us = 1e6 * (time.perf_counter() - c0) / (a.steps * B)
        t._issued = t._done = 0
        t.close()
        return us

    # the loop a caller had before: one stream, the centre formed on the host from the minimum / arg-min read back after every tile
    st = C.c_void_p(); _lib.check(L.ssdr_stream_create(C.byref(st))); s = st.value
    net = randlanet.Network(cfg).load(W)
    d_p = DevArray.from_host(np.concatenate([c["xyz"] for c in clouds])); d_c = DevArray.from_host(np.concatenate([c["rgb"] for c in clouds]).astype(np.float32))
    d_m = [DevArray.from_host(np.array([n, 0], np.int64)) for n in sizes]
    xyz, feat, idx = DevArray((B, N, 3), np.float32), DevArray((B, N, 6), np.float32), DevArray((B, N), np.int32)
    lv = [N]
    for r in cfg.sub_sampling_ratio:
        lv.append(lv[-1] // r)
    neigh = [DevArray((B, lv[i], K), np.int32) for i in range(NL)]; interp = [DevArray((B, lv[i], 1), np.int32) for i in range(NL)]
    probs, f32 = DevArray((B * N, Cn), np.float32), DevArray((B * N, 32), np.float32)
    d_min, d_arg = DevArray((1,), np.float64), DevArray((1,), np.int32)
    d_draw = [dict(perm=DevArray((B, N), np.int32), dup=DevArray((B, N), np.float32)) for _ in range(2)]
    ratios = np.asarray(cfg.sub_sampling_ratio, np.int32)
    arr = C.c_void_p * NL

    def loop_epoch():
        d_poss = DevArray.from_host(np.concatenate(poss0))
        test_probs = DevArray.from_host(np.zeros((int(off[-1]), Cn), np.float32)); owner = DevArray.from_host(np.full(int(off[-1]), -1, np.int32))
        mins = np.array([p.min() for p in poss0]); args = [int(np.argmin(p)) for p in poss0]
        _lib.sync(); _lib.sync(s)
        c0 = time.perf_counter()
        for k in range(a.steps):
            d = all_draws[k]; dd = d_draw[k % 2]
            _lib.check(L.ssdr_memcpy_h2d_on(dd["perm"].ptr, _lib.ptr(d["perm"]), d["perm"].nbytes, s))
            _lib.check(L.ssdr_memcpy_h2d_on(dd["dup"].ptr, _lib.ptr(d["dup"]), d["dup"].nbytes, s))
            which = []
            for j in range(B):
                c = int(np.argmin(mins))
                pick = (clouds[c]["xyz"][args[c]] + d["noise"][j]).astype(np.float32)
                o = int(off[c])
                _lib.check(L.ssdr_tile_select_possibility_dev(d_p.ptr + 12 * o, d_c.ptr + 12 * o, 3, d_m[c].ptr, sizes[c], _lib.ptr(pick), N, dd["perm"].ptr + 4 * j * N,
                                                              dd["dup"].ptr + 4 * j * N, 1.0 / 255.0, xyz.ptr + 12 * j * N, feat.ptr + 24 * j * N, idx.ptr + 4 * j * N,
                                                              d_poss.ptr + 8 * o, d_min.ptr, d_arg.ptr, s))
                mins[c] = d_min.to_host(s)[0]; args[c] = int(d_arg.to_host(s)[0])
                which.append(c)
            _lib.check(L.ssdr_knn_pyramid_dev(xyz.ptr, B, N, NL, _lib.ptr(ratios), K, arr(*[x.ptr for x in neigh]), None, arr(*[x.ptr for x in interp]), s))
            net.infer_dev(B, N, feat.ptr, xyz.ptr, [x.ptr for x in neigh], [x.ptr for x in interp], probs.ptr, f32.ptr, s)
            for j, c in enumerate(which):
                o = int(off[c])
                _lib.check(L.ssdr_vote_smooth_dev(test_probs.ptr + 4 * o * Cn, idx.ptr + 4 * j * N, probs.ptr + 4 * j * N * Cn, N, Cn, 0.95, owner.ptr + 4 * o, s))
        _lib.check(L.ssdr_knn_status(s, None))
        ms = 1e3 * (time.perf_counter() - c0)
        return ms, (d_poss.to_host(s), test_probs.to_host(s))

    device_epoch(); loop_epoch(); generator_alone()          # warm-up (workspaces, code objects)
    t_dev, t_loop, t_gen = [], [], []
    for _ in range(a.repeats):
        ms, dev_out = device_epoch(); t_dev.append(ms)
        ms, loop_out = loop_epoch(); t_loop.append(ms)
        t_gen.append(generator_alone())
    identical = bool(np.array_equal(dev_out[0], loop_out[0]) and np.array_equal(dev_out[1].view(np.uint32), loop_out[1].view(np.uint32)))
    med = lambda v: round(float(np.median(v)), 2)
    print(json.dumps(dict(probe="vote", rooms=len(clouds), points=int(sum(sizes)), min_points=int(min(sizes)), max_points=int(max(sizes)), tiles=a.steps * B,
                          generator_us_per_tile=dict(median=med(t_gen), best=round(min(t_gen), 2)),
                          epoch_ms=dict(median=med(t_dev), best=round(min(t_dev), 2)), loop_ms=dict(median=med(t_loop), best=round(min(t_loop), 2)),
                          launches_per_tile=int(L.ssdr_vote_tile_launches()), depth=evaluate.VoteTester.DEPTH, identical=identical)))
    _lib.check(L.ssdr_stream_destroy(s))


if __name__ == "__main__":
    main()
