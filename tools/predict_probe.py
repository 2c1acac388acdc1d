"""Whole-cloud prediction pass (ssdr_al.prediction.WholeCloudPredictor) over a pool of 204 synthetic rooms (synthetic.make_room, sub-sampled
by the product's front end at 0.04 m, densities varied so that sizes spread), against a per-room loop of the existing B = 1 calls
(ssdr_knn_pyramid_dev + ssdr_randla_infer_dev, device-resident, same stream) on the same tiles.  The two are alternated, 3 repeats each.
Prints one JSON line: rows, chunks, ms and Mpoints/s of run() at the default max_rows, the loop's ms, and the max |difference| of the outputs.
GPU only.  Usage: python tools/predict_probe.py [--rooms 204] [--repeats 3]"""
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
    ap.add_argument("--rooms", type=int, default=204)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    from oracle import randla_np as R
    from ssdr_al import _lib, randlanet, subsampling, synthetic
    from ssdr_al.helper_tool import ConfigS3DIS as cfg
    from ssdr_al.prediction import WholeCloudPredictor, level_sizes, packed_positions
    _lib.check(_lib.lib().ssdr_init(0))
    rng = np.random.default_rng(2024)
    clouds = []
    for i in range(a.rooms):
        xyz, rgb, lab = synthetic.make_room(20000 + i, density=float(np.exp(rng.uniform(np.log(40.0), np.log(1500.0)))))
        sp, sc, sl = subsampling.compute(xyz, features=rgb.astype(np.float32), classes=lab.astype(np.int32), sampleDl=0.04)
        clouds.append(dict(xyz=sp, rgb=sc, labels=sl.reshape(-1).astype(np.int32)))
    sizes = [len(c["xyz"]) for c in clouds]
    W = R.init_weights(0)
    pred = WholeCloudPredictor(W)
    s = C.c_void_p()
    _lib.check(_lib.lib().ssdr_stream_create(C.byref(s)))
    stream = s.value
    draws = [pred.draw(c["xyz"], i, 0) for i, c in enumerate(clouds)]

    # the per-room loop's inputs: every room's cloud-major tile (from one run of the predictor, untimed) and its own buffers
    out = pred.run(clouds, draws=draws, stream=stream)
    out.check()
    L, K, Cn = cfg.num_layers, cfg.k_n, cfg.num_classes
    ratios = np.asarray(cfg.sub_sampling_ratio, np.int32)
    net = randlanet.Network(cfg).load(W)
    rooms = []
    for ch in out.chunks:
        cm_xyz, pk_feat, pk_p, pk_f = ch["cm_xyz"].to_host(), ch["pk_feat"].to_host(), ch["pk_probs"].to_host(), ch["pk_f32"].to_host()
        pos = packed_positions(ch["T"], cfg.sub_sampling_ratio)
        r0 = np.concatenate([[0], np.cumsum(ch["T"])])
        for c, T in enumerate(ch["T"]):
            N = level_sizes(T, cfg.sub_sampling_ratio)
            rooms.append(dict(T=T, xyz=_lib.DevArray.from_host(cm_xyz[r0[c]:r0[c + 1]]), feat=_lib.DevArray.from_host(pk_feat[pos[c]]),
                              neigh=[_lib.DevArray((N[l], K), np.int32) for l in range(L)], interp=[_lib.DevArray((N[l], 1), np.int32) for l in range(L)],
                              probs=_lib.DevArray((T, Cn), np.float32), f32=_lib.DevArray((T, 32), np.float32), want=(pk_p[pos[c]], pk_f[pos[c]])))
    arr = C.c_void_p * L

    def loop():
        for rm in rooms:
            _lib.check(_lib.lib().ssdr_knn_pyramid_dev(rm["xyz"].ptr, 1, rm["T"], L, _lib.ptr(ratios), K, arr(*[x.ptr for x in rm["neigh"]]), None,
                                                       arr(*[x.ptr for x in rm["interp"]]), stream))
            net.infer_dev(1, rm["T"], rm["feat"].ptr, rm["xyz"].ptr, [x.ptr for x in rm["neigh"]], [x.ptr for x in rm["interp"]], rm["probs"].ptr,
                          rm["f32"].ptr, stream)
        _lib.check(_lib.lib().ssdr_knn_status(stream, None))

    def packed():
        o = pred.run(clouds, draws=draws, stream=stream)
        o.check()
        return o

    t_run, t_loop = [], []
    packed(); loop()                         # warm-up (workspaces, code objects)
    for _ in range(a.repeats):
        _lib.sync(stream); t0 = time.perf_counter(); o = packed(); t_run.append(1e3 * (time.perf_counter() - t0))
        _lib.sync(stream); t0 = time.perf_counter(); loop(); t_loop.append(1e3 * (time.perf_counter() - t0))
    diff = 0.0
    for rm in rooms:
        diff = max(diff, float(np.abs(rm["probs"].to_host() - rm["want"][0]).max()), float(np.abs(rm["f32"].to_host() - rm["want"][1]).max()))
    rows = int(sum(max(n, cfg.num_points) for n in sizes))
    ms = min(t_run)
    print(json.dumps(dict(probe="predict", rooms=len(clouds), points=int(sum(sizes)), min_points=int(min(sizes)), max_points=int(max(sizes)),
                          rows=rows, chunks=len(o.chunks), max_rows=pred.max_rows, run_ms=[round(x, 2) for x in t_run], loop_ms=[round(x, 2) for x in t_loop],
                          run_mpoints_s=round(sum(sizes) / ms / 1e3, 2), loop_mpoints_s=round(sum(sizes) / min(t_loop) / 1e3, 2),
                          speedup=round(min(t_loop) / ms, 3), max_abs_diff=diff)))
    _lib.check(_lib.lib().ssdr_stream_destroy(stream))


if __name__ == "__main__":
    main()
