"""The two network-side passes of a Semantic3D round that are not training, on synthetic scans, each against the loop a caller had before.
Prints one JSON line (kept as profiles/sem3d_round_probe.json).  GPU only.

(a) The prediction pass: WholeCloudPredictor(dataset="Semantic3D", draws="device", keep_chunks=False) over --scans scans of --points points
    (uniform in a 60 x 60 x 8 m box, so split3 cuts each into quadrants of about a quarter), against the per-part loop over the public calls:
    the same tiles and parts read back to the host, then per part a host gather, Network.infer with B = 1 (its own pyramid) and a host scatter.
    Both in one process, alternating after a warm-up; the host's clock around each with a synchronise at the end (the pass waits for the
    device once per split, so the host's clock is the time a caller sees).
(b) One evaluation epoch: VoteTester(dataset="Semantic3D") with the real configuration (--steps batches of val_batch_size tiles of 65 536
    points) against the per-tile loop: the chain called for one tile at a time with a wait after each (a caller who forms every tile on its
    own), the augmentation per tile, then per batch the pyramid, the network and the votes, on the same draws.

Usage: python tools/sem3d_round_probe.py [--scans 4] [--points 3000000] [--steps 100] [--repeats 3] [--clouds 6] [--cloud-points 400000]
       [--tile-points 65536] [--batch 16]"""
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
    ap.add_argument("--scans", type=int, default=4)
    ap.add_argument("--points", type=int, default=3000000)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--clouds", type=int, default=6)
    ap.add_argument("--cloud-points", type=int, default=400000)
    ap.add_argument("--tile-points", type=int, default=0, help="tile size of (b) (default: the configuration's 65 536)")
    ap.add_argument("--batch", type=int, default=0, help="tiles per batch of (b) (default: the configuration's 16)")
    a = ap.parse_args()
    from oracle import randla_np as R
    from ssdr_al import _lib, evaluate, randlanet
    from ssdr_al.helper_tool import ConfigSemantic3D as cfg
    from ssdr_al.prediction import WholeCloudPredictor
    L = _lib.lib()
    _lib.check(L.ssdr_init(0))
    W = R.init_weights(0, num_classes=cfg.num_classes)
    med = lambda v: round(float(np.median(v)), 2)
    say = lambda *x: print(*x, file=sys.stderr, flush=True)

    def scan(seed, n, box):
        rng = np.random.default_rng(seed)
        return dict(xyz=(rng.random((n, 3), dtype=np.float32) * np.asarray(box, np.float32)).astype(np.float32),
                    rgb=rng.random((n, 3), dtype=np.float32), labels=rng.integers(0, cfg.num_classes, n).astype(np.int32))

    # ---- (a) the prediction pass ----------------------------------------------------------------------------------------------------------
    scans = [scan(100 + i, a.points, (60, 60, 8)) for i in range(a.scans)]
    pred = WholeCloudPredictor(W, config=cfg, dataset="Semantic3D", draws="device", keep_chunks=False)
    net = randlanet.Network(cfg).load(W)
    Cn = cfg.num_classes

    def device_pass():
        c0 = time.perf_counter()
        out = pred.run(scans, seed=1)
        _lib.sync(out.stream)
        return 1e3 * (time.perf_counter() - c0), out

    def loop_pass(out):
        """the per-part loop over the same tiles and parts: host gather, Network.infer with B = 1, host scatter"""
        t_xyz, t_feat, t_idx, order = (out.inputs[k].to_host() for k in ("t_xyz", "t_feat", "t_idx", "order"))
        n = int(out.offsets[-1])
        probs, feat = np.empty((n, Cn), np.float32), np.empty((n, 32), np.float32)
        c0 = time.perf_counter()
        parts = 0
        for c, off in enumerate(out.part_offsets):
            o = int(out.offsets[c])
            for k in range(len(off) - 1):
                rows = o + order[o + off[k]:o + off[k + 1]]
                p, f = net.infer(t_feat[rows][None], t_xyz[rows][None])
                src = o + t_idx[rows]
                probs[src], feat[src] = p, f
                parts += 1
        return 1e3 * (time.perf_counter() - c0), parts, probs, feat

    ms, out = device_pass()                          # warm-up (workspaces, code objects)
    loop_pass(out)
    say("prediction: warm-up done")
    t_dev, t_loop = [], []
    for _ in range(a.repeats):
        ms, out = device_pass(); t_dev.append(ms)
        ms, parts, lp, lf = loop_pass(out); t_loop.append(ms)
        say("prediction: pass %.0f ms, per-part loop %.0f ms" % (t_dev[-1], t_loop[-1]))
    dp, df = out.probs.to_host(), out.feat32.to_host()
    res_a = dict(scans=a.scans, points=int(out.offsets[-1]), parts=parts, chunks=len(out.chunks),
                 pass_ms=dict(median=med(t_dev), best=round(min(t_dev), 2)), loop_ms=dict(median=med(t_loop), best=round(min(t_loop), 2)),
                 max_abs_diff=dict(probs=float(np.abs(dp - lp).max()), feat32=float(np.abs(df - lf).max())))
    del out, scans

    # ---- (b) one evaluation epoch ---------------------------------------------------------------------------------------------------------
    class vcfg(cfg):
        val_steps = a.steps
        num_points = a.tile_points or cfg.num_points
        val_batch_size = a.batch or cfg.val_batch_size
    clouds = [scan(200 + i, a.cloud_points, (40, 40, 8)) for i in range(a.clouds)]
    sizes = [len(c["xyz"]) for c in clouds]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N, B, K, NL = vcfg.num_points, vcfg.val_batch_size, vcfg.k_n, vcfg.num_layers
    poss0 = [np.random.default_rng([0, c]).random(n) * 1e-3 for c, n in enumerate(sizes)]
    t0 = evaluate.VoteTester(W, clouds, config=vcfg, dataset="Semantic3D", possibility=poss0)
    all_draws = [t0.draw(0, s) for s in range(a.steps)]
    t0.close()
    draws = lambda epoch, step: all_draws[step]

    def device_epoch():
        t = evaluate.VoteTester(W, clouds, config=vcfg, dataset="Semantic3D", possibility=poss0)
        _lib.sync(t.s_gen)
        c0 = time.perf_counter()
        t._epoch(draws)
        _lib.sync(t.s_net)
        ms = 1e3 * (time.perf_counter() - c0)
        res = (np.concatenate(t.possibility()), t.probs_host())
        t.close()
        return ms, res

    st = C.c_void_p(); _lib.check(L.ssdr_stream_create(C.byref(st))); s = st.value
    from ssdr_al._lib import DevArray
    d_p = DevArray.from_host(np.concatenate([c["xyz"] for c in clouds])); d_c = DevArray.from_host(np.concatenate([c["rgb"] for c in clouds]))
    xyz, feat, idx = DevArray((B, N, 3), np.float32), DevArray((B, N, 6), np.float32), DevArray((B, N), np.int32)
    cloud, center = DevArray((B,), np.int32), DevArray((B, 3), np.float32)
    lv = [N]
    for r in vcfg.sub_sampling_ratio:
        lv.append(lv[-1] // r)
    neigh = [DevArray((B, lv[i], K), np.int32) for i in range(NL)]; interp = [DevArray((B, lv[i], 1), np.int32) for i in range(NL)]
    probs, f32 = DevArray((B * N, Cn), np.float32), DevArray((B * N, 32), np.float32)
    dd = dict(noise=DevArray((B, 3), np.float32), perm=DevArray((B, N), np.int32), dup=DevArray.from_host(np.zeros((B, N), np.float32)),
              rot=DevArray((B, 2), np.float64), scale=DevArray((B, 3), np.float64), aug_noise=DevArray((B, N, 3), np.float64))
    ratios = np.asarray(vcfg.sub_sampling_ratio, np.int32)
    arr = C.c_void_p * NL

    def loop_epoch():
        d_poss = DevArray.from_host(np.concatenate(poss0))
        d_min, d_arg = DevArray((len(sizes),), np.float64), DevArray((len(sizes),), np.int32)
        _lib.check(L.ssdr_vote_init_dev(d_poss.ptr, _lib.ptr(off), len(sizes), d_min.ptr, d_arg.ptr, s))
        test_probs = DevArray.from_host(np.zeros((int(off[-1]), Cn), np.float32)); owner = DevArray.from_host(np.full(int(off[-1]), -1, np.int32))
        _lib.sync(); _lib.sync(s)
        c0 = time.perf_counter()
        for k in range(a.steps):
            d = all_draws[k]
            for key in ("noise", "perm", "rot", "scale", "aug_noise"):
                h = np.ascontiguousarray(d[key], dd[key].dtype)
                _lib.check(L.ssdr_memcpy_h2d_on(dd[key].ptr, _lib.ptr(h), h.nbytes, s))
            for j in range(B):
                _lib.check(L.ssdr_feed_chain_dev(d_p.ptr, d_c.ptr, 3, None, d_poss.ptr, d_min.ptr, d_arg.ptr, _lib.ptr(off), len(sizes), 1, N,
                                                 dd["noise"].ptr + 12 * j, dd["perm"].ptr + 4 * j * N, dd["dup"].ptr + 4 * j * N, 1.0, xyz.ptr + 12 * j * N,
                                                 feat.ptr + 24 * j * N, idx.ptr + 4 * j * N, None, cloud.ptr + 4 * j, center.ptr + 12 * j, 1 | 2, None, 0,
                                                 None, None, None, None, s))
                _lib.check(L.ssdr_feed_augment_dev(xyz.ptr + 12 * j * N, 1, N, dd["rot"].ptr + 16 * j, dd["scale"].ptr + 24 * j, dd["aug_noise"].ptr + 24 * j * N, 3,
                                                   feat.ptr + 24 * j * N, s))
                _lib.sync(s)
            _lib.check(L.ssdr_knn_pyramid_dev(xyz.ptr, B, N, NL, _lib.ptr(ratios), K, arr(*[x.ptr for x in neigh]), None, arr(*[x.ptr for x in interp]), s))
            net.infer_dev(B, N, feat.ptr, xyz.ptr, [x.ptr for x in neigh], [x.ptr for x in interp], probs.ptr, f32.ptr, s)
            for j in range(B):
                _lib.check(L.ssdr_vote_smooth_dev(test_probs.ptr, idx.ptr + 4 * j * N, probs.ptr + 4 * j * N * Cn, N, Cn, 0.98, owner.ptr, s))
        _lib.check(L.ssdr_knn_status(s, None))
        ms = 1e3 * (time.perf_counter() - c0)
        return ms, (d_poss.to_host(s), test_probs.to_host(s))

    device_epoch(); loop_epoch()
    e_dev, e_loop = [], []
    for _ in range(a.repeats):
        ms, dev_out = device_epoch(); e_dev.append(ms)
        ms, loop_out = loop_epoch(); e_loop.append(ms)
        say("evaluation: epoch %.0f ms, per-tile loop %.0f ms" % (e_dev[-1], e_loop[-1]))
    identical = bool(np.array_equal(dev_out[0], loop_out[0]) and np.array_equal(dev_out[1].view(np.uint32), loop_out[1].view(np.uint32)))
    res_b = dict(clouds=len(sizes), points=int(sum(sizes)), tiles=a.steps * B, tile_points=N,
                 epoch_ms=dict(median=med(e_dev), best=round(min(e_dev), 2)), loop_ms=dict(median=med(e_loop), best=round(min(e_loop), 2)), identical=identical)
    print(json.dumps(dict(probe="sem3d_round", prediction=res_a, evaluation=res_b)))
    _lib.check(L.ssdr_stream_destroy(s))


if __name__ == "__main__":
    main()
