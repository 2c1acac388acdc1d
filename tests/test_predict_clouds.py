"""Whole-cloud inference over ragged batches (ssdr_al.prediction.WholeCloudPredictor): the network pass of the reference's AL round
(TSampler.prediction / compute_features, S3/sampler2.py:580-642, :313-342) with every room whole, many rooms per call.

CPU part (the CPU logic build and the GPU build alike, through the `backend` fixture): a small configuration (num_points 1024, two levels)
over clouds of 300 (padded), 1024, 1029, 1500 and 2117 points, one holding a duplicated block (tie rows).  Each stage against a NumPy
restatement or the C oracle: the whole-cloud tile and its packing, the ragged pyramid, the packed network, the read-back, chunking and the
refusals.  GPU part: the S3DIS configuration at whole-room sizes, a pool of synthetic rooms, and the composition with HotPath.from_device."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal

SIZES = [300, 1024, 1029, 1500, 2117]


def _cfg():
    from ssdr_al.helper_tool import ConfigS3DIS

    class Small(ConfigS3DIS):
        num_points = 1024
        num_layers = 2
        d_out = [16, 64]
        sub_sampling_ratio = [4, 4]
        num_classes = 13
    return Small


def _clouds(sizes, seed=7, dup_block=2):
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(sizes):
        xyz = (rng.random((n, 3), dtype=np.float32) * np.array([3, 2.5, 2], np.float32)).astype(np.float32)
        if i == dup_block:
            xyz[-120:] = xyz[:120]                 # exact duplicates: equal distances (tile ties) and equal KNN distances
        out.append(dict(xyz=xyz, rgb=rng.integers(0, 256, (n, 3)).astype(np.uint8), labels=rng.integers(0, 13, n).astype(np.int32)))
    return out


def _np_tile(cloud, d, num_points):
    """tile.hip's rule with num_points = T = max(n, num_points) (the pattern of oracle/pipeline_np.front_end after its sub-sampling)"""
    xyz, rgb = cloud["xyz"], cloud["rgb"].astype(np.float32)
    n = len(xyz); T = max(n, num_points)
    c = np.asarray(d["center"], np.float32)
    dd = xyz - c[None]
    dist = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
    order = np.argsort(dist, kind="stable")
    perm, dup = np.asarray(d["perm"]), np.asarray(d["dup"], np.float32)
    if n == T:
        pos = perm
    else:
        shuffled = perm[perm < n]
        want = np.where(np.arange(T) < n, np.arange(T), np.minimum((dup * np.float32(n)).astype(np.int64), n - 1))
        pos = shuffled[want]
    ids = order[pos]
    txyz = (xyz[ids] - c[None]).astype(np.float32)
    return txyz, np.concatenate([txyz, rgb[ids] * np.float32(1.0 / 255.0)], 1).astype(np.float32), ids.astype(np.int32)


def _oracle_knn():
    import oracle
    r = oracle.ref()
    if r is not None:
        return lambda s, q, k: r.knn(s, q, k, omp=True)
    o = oracle.c()
    return lambda s, q, k: o.knn_batch(s[None], q[None], k, threads=1)[0]


def _chunk_views(pred, out, ch):
    """host copies of one chunk's intermediates, per cloud (cloud-major tile, KNN tables cloud-local, packed rows)"""
    from ssdr_al.prediction import level_sizes, packed_positions
    cfg = pred.cfg
    L = cfg.num_layers
    T, R = ch["T"], ch["R"]
    cm_xyz, cm_idx = ch["cm_xyz"].to_host(), ch["cm_idx"].to_host()
    cm_n, cm_i = ch["cm_neigh"].to_host(), ch["cm_interp"].to_host()
    pk_n, pk_i = ch["pk_neigh"].to_host(), ch["pk_interp"].to_host()
    pos = packed_positions(T, cfg.sub_sampling_ratio)
    row0 = np.concatenate([[0], np.cumsum(T)])
    clouds = []
    for c in range(len(T)):
        N = level_sizes(T[c], cfg.sub_sampling_ratio)
        neigh, interp, pneigh, pinterp = [], [], [], []
        for l in range(L):
            cmo = int(R[l]) + sum(level_sizes(T[k], cfg.sub_sampling_ratio)[l] for k in range(c))
            neigh.append(cm_n[cmo:cmo + N[l]]); interp.append(cm_i[cmo:cmo + N[l]])
            rows = int(R[l]) + pos[c][:N[l]]
            pneigh.append(pk_n[rows]); pinterp.append(pk_i[rows])
        clouds.append(dict(xyz=cm_xyz[row0[c]:row0[c + 1]], idx=cm_idx[row0[c]:row0[c + 1]], N=N, pos=pos[c],
                           neigh=neigh, interp=interp, pk_neigh=pneigh, pk_interp=pinterp))
    return clouds


@pytest.fixture(scope="module")
def weights_small():
    from oracle import randla_np as R
    return R.init_weights(0, d_out=(16, 64))


def _run(backend, W, sizes=SIZES, max_rows=1 << 22, readback="reference", seed=3, precision="f32"):
    from ssdr_al import _lib
    from ssdr_al.prediction import WholeCloudPredictor
    _lib.check(_lib.lib().ssdr_init(0))
    clouds = _clouds(sizes)
    pred = WholeCloudPredictor(W, config=_cfg(), precision=precision, max_rows=max_rows)
    out = pred.run(clouds, seed=seed, readback=readback)
    out.check()
    return pred, clouds, out


def test_whole_cloud_tile_and_packing(backend, weights_small):
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    pred, clouds, out = _run(backend, weights_small)
    cfg = pred.cfg
    assert len(out.chunks) == 1
    ch = out.chunks[0]
    views = _chunk_views(pred, out, ch)
    pk_xyz, pk_feat, pk_src, pk_lab = ch["pk_xyz"].to_host(), ch["pk_feat"].to_host(), ch["pk_src"].to_host(), ch["pk_lab"].to_host()
    draws = [pred.draw(c["xyz"], i, 3) for i, c in enumerate(clouds)]
    P = ch["P"]
    for c, (cl, v, d) in enumerate(zip(clouds, views, draws)):
        txyz, feat, ids = _np_tile(cl, d, cfg.num_points)
        assert_bits_equal(v["xyz"], txyz, "cloud %d cloud-major xyz" % c)
        assert np.array_equal(v["idx"], ids), "cloud %d source rows" % c
        assert_bits_equal(pk_xyz[v["pos"]], txyz, "cloud %d packed xyz" % c)
        assert_bits_equal(pk_feat[v["pos"]], feat, "cloud %d packed features" % c)
        assert np.array_equal(pk_src[v["pos"]], ids) and np.array_equal(pk_lab[v["pos"]], cl["labels"][ids])
        for l in range(cfg.num_layers + 1):            # level l of every cloud = the first P_l packed rows
            assert (v["pos"][:v["N"][l]] < P[l]).all() and (v["pos"][v["N"][l]:] >= P[l]).all()
    assert P[0] == sum(max(n, cfg.num_points) for n in SIZES)
    assert sorted(np.concatenate([v["pos"] for v in views]).tolist()) == list(range(int(P[0])))
    # n_c <= num_points: the fixed-size batch tile, bit for bit
    small = [c for c, n in enumerate(SIZES) if n <= cfg.num_points]
    N = cfg.num_points
    pts = np.concatenate([clouds[c]["xyz"] for c in small]); col = np.concatenate([clouds[c]["rgb"] for c in small]).astype(np.float32)
    off = np.concatenate([[0], np.cumsum([SIZES[c] for c in small])]).astype(np.int64)
    d_p, d_c, d_m = DevArray.from_host(pts), DevArray.from_host(col), DevArray.from_host(np.array([SIZES[c] for c in small] + [0], np.int64))
    d_perm = DevArray.from_host(np.stack([draws[c]["perm"] for c in small])); d_dup = DevArray.from_host(np.stack([draws[c]["dup"] for c in small]))
    d_xyz, d_feat, d_idx = DevArray((len(small), N, 3), np.float32), DevArray((len(small), N, 6), np.float32), DevArray((len(small), N), np.int32)
    centers = np.ascontiguousarray(np.stack([draws[c]["center"] for c in small]), np.float32)
    _lib.check(_lib.lib().ssdr_tile_select_batch_dev(d_p.ptr, d_c.ptr, 3, d_m.ptr, _lib.ptr(off), len(small), _lib.ptr(centers), N, d_perm.ptr,
                                                    d_dup.ptr, 1.0 / 255.0, d_xyz.ptr, d_feat.ptr, d_idx.ptr, None, None, None))
    _lib.sync()
    for k, c in enumerate(small):
        assert_bits_equal(views[c]["xyz"], d_xyz.to_host()[k], "cloud %d vs batch tile" % c)
        assert_bits_equal(pk_feat[views[c]["pos"]], d_feat.to_host()[k], "cloud %d features vs batch tile" % c)
        assert np.array_equal(views[c]["idx"], d_idx.to_host()[k])


def test_ragged_pyramid_matches_oracle_per_cloud(backend, weights_small):
    pred, clouds, out = _run(backend, weights_small)
    knn = _oracle_knn()
    for c, v in enumerate(_chunk_views(pred, out, out.chunks[0])):
        cur = v["xyz"]
        for l, r in enumerate(pred.cfg.sub_sampling_ratio):
            nxt = cur[: len(cur) // r]
            assert_bits_equal(v["neigh"][l], knn(cur, cur, 16).astype(np.int32), "cloud %d level %d neigh" % (c, l))
            assert_bits_equal(v["interp"][l][:, None], knn(nxt, cur, 1).astype(np.int32), "cloud %d level %d interp" % (c, l))
            # the translated tables: the same neighbours, as packed rows
            assert np.array_equal(v["pk_neigh"][l], v["pos"][v["neigh"][l]])
            assert np.array_equal(v["pk_interp"][l], v["pos"][v["interp"][l]])
            cur = nxt


def test_packed_network_against_oracle_and_per_cloud_calls(backend, weights_small):
    from oracle import randla_np as R
    from ssdr_al import _lib, randlanet
    pred, clouds, out = _run(backend, weights_small)
    cfg = pred.cfg
    ch = out.chunks[0]
    pp, pf = ch["pk_probs"].to_host(), ch["pk_f32"].to_host()
    pk_feat = ch["pk_feat"].to_host()
    net = randlanet.Network(cfg).load(weights_small)
    for c, v in enumerate(_chunk_views(pred, out, ch)):
        T = len(v["xyz"])
        gp, gf = pp[v["pos"]], pf[v["pos"]]
        feat = pk_feat[v["pos"]][None]
        xyz = [v["xyz"][None, :n] for n in v["N"][:-1]]
        sub = [v["neigh"][l][None, :v["N"][l + 1]] for l in range(cfg.num_layers)]
        p64, f64 = R.forward(weights_small, feat, xyz, [a[None] for a in v["neigh"]], sub, [a[None, :, None] for a in v["interp"]], dtype=np.float64)
        assert np.abs(gp - p64).max() < 3e-5 and np.abs(gf - f64).max() < 1.1e-4, (c, np.abs(gp - p64).max(), np.abs(gf - f64).max())
        # the same tile through the existing B = 1 entry point with the cloud's own pyramid
        d_feat, d_xyz = _lib.DevArray.from_host(feat), _lib.DevArray.from_host(v["xyz"][None])
        nb = [_lib.DevArray.from_host(a[None]) for a in v["neigh"]]; ip = [_lib.DevArray.from_host(a[None, :, None]) for a in v["interp"]]
        d_p, d_f = _lib.DevArray((T, cfg.num_classes), np.float32), _lib.DevArray((T, 32), np.float32)
        net.infer_dev(1, T, d_feat.ptr, d_xyz.ptr, [a.ptr for a in nb], [a.ptr for a in ip], d_p.ptr, d_f.ptr)
        _lib.sync()
        assert np.abs(gp - d_p.to_host()).max() < 1e-4 and np.abs(gf - d_f.to_host()).max() < 1e-4


def test_result_keeps_every_buffer_the_stream_reads(backend, weights_small):
    """run() returns before the stream has run its kernels: every input it uploaded (points, colours, labels, draws) must stay owned by
    the result.  A dropped DevArray goes back to the pool at once, and the next allocation of its size class would get (and overwrite)
    it while the tile kernel may still read it."""
    from ssdr_al._lib import DevArray
    pred, clouds, out = _run(backend, weights_small)
    held = {out.inputs[k].ptr for k in ("xyz", "rgb", "labels", "perm", "dup")}
    assert len(held) == 5
    n = sum(SIZES)
    fresh = [DevArray((n, 3), np.float32), DevArray((n,), np.int32), DevArray((sum(max(x, 1024) for x in SIZES),), np.float32)]
    assert not held & {f.ptr for f in fresh}


def test_readback_modes_on_synthetic_packed_arrays(backend):
    """packed outputs coded by row, read back in both modes: the padded cloud's reference order (stable argsort of point_idx) exactly"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    from ssdr_al.prediction import packed_positions
    _lib.check(_lib.lib().ssdr_init(0))
    rng = np.random.default_rng(5)
    cfg = _cfg()
    T = [max(n, cfg.num_points) for n in SIZES]
    keys = []
    for n, t in zip(SIZES, T):
        k = rng.permutation(n)
        if t > n:
            k = np.concatenate([k, rng.integers(0, n, t - n)])         # the tile's shape: rows [0, n) shuffle the points, duplicates behind
        keys.append(k.astype(np.int32))
    pos = packed_positions(T, cfg.sub_sampling_ratio)
    rows = sum(T); Cn = cfg.num_classes
    pk_p = (np.arange(rows * Cn, dtype=np.float32) / 7).reshape(rows, Cn); pk_f = -(np.arange(rows * 32, dtype=np.float32) / 3).reshape(rows, 32)
    d_idx, d_pp, d_pf = DevArray.from_host(np.concatenate(keys)), DevArray.from_host(pk_p), DevArray.from_host(pk_f)
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    r = np.asarray(cfg.sub_sampling_ratio, np.int32)
    for mode in (0, 1):
        d_p, d_f = DevArray((int(off[-1]), Cn), np.float32), DevArray((int(off[-1]), 32), np.float32)
        _lib.check(_lib.lib().ssdr_predict_readback_dev(_lib.ptr(off), len(SIZES), cfg.num_points, cfg.num_layers, _lib.ptr(r), d_idx.ptr, d_pp.ptr, Cn,
                                                       d_pf.ptr, mode, d_p.ptr, d_f.ptr, None))
        _lib.sync()
        gp, gf = d_p.to_host(), d_f.to_host()
        for c, (n, k) in enumerate(zip(SIZES, keys)):
            order = np.argsort(k, kind="stable")
            if mode == 0:
                src = order[:n]                                              # out[p] = tile_out[argsort(point_idx)[p]]
            else:
                first = np.full(n, -1); first[k[::-1]] = np.arange(len(k))[::-1]       # each point's first row
                src = first
            assert np.array_equal(gp[off[c]:off[c + 1]], pk_p[pos[c][src]]), (mode, c)
            assert np.array_equal(gf[off[c]:off[c + 1]], pk_f[pos[c][src]]), (mode, c)
            if n >= cfg.num_points:
                assert np.array_equal(order[:n], np.argsort(k)[:n])         # unpadded: a permutation, both modes agree


def test_chunking_keeps_tables_and_outputs(backend, weights_small):
    cfg = _cfg()
    pred1, clouds, out1 = _run(backend, weights_small)
    pred3, _, out3 = _run(backend, weights_small, max_rows=2600)
    assert [(c["lo"], c["hi"]) for c in out3.chunks] == [(0, 2), (2, 4), (4, 5)]
    one = _chunk_views(pred1, out1, out1.chunks[0])
    three = [v for ch in out3.chunks for v in _chunk_views(pred3, out3, ch)]
    for a, b in zip(one, three):
        assert_bits_equal(a["xyz"], b["xyz"])
        for l in range(cfg.num_layers):
            assert np.array_equal(a["neigh"][l], b["neigh"][l]) and np.array_equal(a["interp"][l], b["interp"][l])
    h1, h3 = out1.to_host(), out3.to_host()
    for a, b in zip(h1, h3):
        assert np.abs(a["probs"] - b["probs"]).max() < 1e-4 and np.abs(a["feat32"] - b["feat32"]).max() < 1e-4
        assert np.array_equal(a["labels"], b["labels"])


def test_refusals(backend, weights_small):
    from ssdr_al import _lib
    from ssdr_al.prediction import WholeCloudPredictor
    L = _lib.lib()
    _lib.check(L.ssdr_init(0))
    cfg = _cfg()
    r = np.asarray(cfg.sub_sampling_ratio, np.int32)
    off = np.array([0, 500, 500, 900], np.int64)                     # cloud 1 is empty
    assert L.ssdr_predict_layout(_lib.ptr(off), 3, cfg.num_points, 2, _lib.ptr(r), None) == 1
    assert b"cloud 1 is empty" in L.ssdr_last_error()
    big = np.array([0, (1 << 23) + 1], np.int64)
    assert L.ssdr_predict_layout(_lib.ptr(big), 1, cfg.num_points, 2, _lib.ptr(r), None) == 5
    assert b"2^23" in L.ssdr_last_error()
    with pytest.raises(_lib.SsdrError) as e:
        WholeCloudPredictor(weights_small, config=cfg, max_rows=(1 << 23) + 1)
    assert e.value.status == 5 and "2^23" in str(e.value)
    pred = WholeCloudPredictor(weights_small, config=cfg)
    with pytest.raises(_lib.SsdrError) as e:
        pred.run(_clouds([300, 0, 500]))
    assert e.value.status == 1 and "cloud 1 is empty" in str(e.value)
    arr = C.c_void_p * 2
    dummy = _lib.DevArray((4096, 16), np.float32)
    for bad in ([1024, 2048, 64], [1024, 256, 0]):                    # increasing, empty level
        lv = (C.c_size_t * 3)(*bad)
        assert L.ssdr_randla_infer_rows_dev(pred.net._h, lv, dummy.ptr, dummy.ptr, arr(dummy.ptr, dummy.ptr), arr(dummy.ptr, dummy.ptr),
                                            dummy.ptr, dummy.ptr, None) == 1
        assert b"non-increasing" in L.ssdr_last_error()
    many = np.arange(4098, dtype=np.int64) * 2000                     # 4097 clouds
    assert L.ssdr_knn_pyramid_ragged_dev(dummy.ptr, _lib.ptr(many), 4097, cfg.num_points, 2, _lib.ptr(r), 16, dummy.ptr, dummy.ptr, None) == 5
    assert b"at most 4096" in L.ssdr_last_error()
    lv = (C.c_size_t * 3)((1 << 23) + 4, 1 << 21, 1 << 19)
    assert L.ssdr_randla_infer_rows_dev(pred.net._h, lv, dummy.ptr, dummy.ptr, arr(dummy.ptr, dummy.ptr), arr(dummy.ptr, dummy.ptr),
                                        dummy.ptr, dummy.ptr, None) == 5
    assert b"2^23" in L.ssdr_last_error()


# ---- GPU: the S3DIS configuration at whole-room sizes ----------------------------------------------------------------------------------

def _gpu():
    from conftest import GPU_LIB, _have_gpu
    if not _have_gpu():
        pytest.skip("no GPU")
    from ssdr_al import _lib
    _lib.use(GPU_LIB)
    _lib.check(_lib.lib().ssdr_init(0))


def _room_pool(n_rooms, seed0=9300):
    """synthetic rooms through the product's front end (grid sub-sampling at 0.04 m), densities varied so that sizes spread"""
    from ssdr_al import subsampling, synthetic
    rng = np.random.default_rng(seed0)
    out = []
    for i in range(n_rooms):
        xyz, rgb, lab = synthetic.make_room(seed0 + i, density=float(rng.uniform(60.0, 900.0)))
        sp, sc, sl = subsampling.compute(xyz, features=rgb.astype(np.float32), classes=lab.astype(np.int32), sampleDl=0.04)
        out.append(dict(xyz=sp, rgb=sc, labels=sl.reshape(-1).astype(np.int32)))
    return out


@pytest.mark.gpu
def test_gpu_whole_rooms_against_oracle():
    """clouds of 7 013 (padded), 40 960, 40 961, 97 531 and 151 003 points in one run(): pyramid bit-exact per cloud, probs / feat32 within
    1e-3 of the fp32 NumPy oracle in f32 and bf16x3, f32 within 1e-4 of per-cloud B = 1 product calls"""
    from oracle import randla_np as R
    from ssdr_al import _lib, randlanet
    from ssdr_al.helper_tool import ConfigS3DIS
    from ssdr_al.prediction import WholeCloudPredictor
    _gpu()
    try:
        sizes = [7013, 40960, 40961, 97531, 151003]
        rng = np.random.default_rng(11)
        clouds = []
        for i, n in enumerate(sizes):
            xyz = (rng.random((n, 3), dtype=np.float32) * np.array([9, 7, 3], np.float32)).astype(np.float32)
            xyz[-3000:] = xyz[:3000]
            clouds.append(dict(xyz=xyz, rgb=rng.integers(0, 256, (n, 3)).astype(np.uint8), labels=rng.integers(0, 13, n).astype(np.int32)))
        W = R.init_weights(0)
        knn = _oracle_knn()
        net = randlanet.Network(ConfigS3DIS).load(W)
        ref = None
        for prec in ("f32", "bf16x3"):
            pred = WholeCloudPredictor(W, precision=prec)
            out = pred.run(clouds, seed=4)
            assert out.check()[2] == 0
            ch = out.chunks[0]
            views = _chunk_views(pred, out, ch)
            pp, pf, pk_feat = ch["pk_probs"].to_host(), ch["pk_f32"].to_host(), ch["pk_feat"].to_host()
            if ref is None:
                ref = []
                for c, v in enumerate(views):
                    cur = v["xyz"]
                    for l, r in enumerate(ConfigS3DIS.sub_sampling_ratio):
                        nxt = cur[: len(cur) // r]
                        assert_bits_equal(v["neigh"][l], knn(cur, cur, 16).astype(np.int32), "cloud %d level %d neigh" % (c, l))
                        assert_bits_equal(v["interp"][l][:, None], knn(nxt, cur, 1).astype(np.int32), "cloud %d level %d interp" % (c, l))
                        cur = nxt
                    feat = pk_feat[v["pos"]][None]
                    xyz = [v["xyz"][None, :n] for n in v["N"][:-1]]
                    sub = [v["neigh"][l][None, :v["N"][l + 1]] for l in range(ConfigS3DIS.num_layers)]
                    ref.append(R.forward(W, feat, xyz, [a[None] for a in v["neigh"]], sub, [a[None, :, None] for a in v["interp"]], dtype=np.float32))
            for c, v in enumerate(views):
                gp, gf = pp[v["pos"]], pf[v["pos"]]
                ep, ef = np.abs(gp - ref[c][0]).max(), np.abs(gf - ref[c][1]).max()
                print("\n%s cloud %d (%d points): max |probs - oracle| %.3g, |feat32 - oracle| %.3g" % (prec, c, sizes[c], ep, ef))
                assert ep < 1e-3 and ef < 1e-3, (prec, c, ep, ef)
                if prec == "f32":
                    T = len(v["xyz"])
                    d_feat, d_xyz = _lib.DevArray.from_host(pk_feat[v["pos"]][None]), _lib.DevArray.from_host(v["xyz"][None])
                    nb = [_lib.DevArray.from_host(a[None]) for a in v["neigh"]]; ip = [_lib.DevArray.from_host(a[None, :, None]) for a in v["interp"]]
                    d_p, d_f = _lib.DevArray((T, 13), np.float32), _lib.DevArray((T, 32), np.float32)
                    net.infer_dev(1, T, d_feat.ptr, d_xyz.ptr, [a.ptr for a in nb], [a.ptr for a in ip], d_p.ptr, d_f.ptr)
                    _lib.sync()
                    assert np.abs(gp - d_p.to_host()).max() < 1e-4 and np.abs(gf - d_f.to_host()).max() < 1e-4
    finally:
        _lib.use(None)


@pytest.mark.gpu
def test_gpu_room_pool_chunked():
    """40 synthetic rooms through the front end, default and 4-chunk max_rows: status clean, equal cloud-local neighbour tables, outputs
    within 1e-4 (f32)"""
    from oracle import randla_np as R
    from ssdr_al import _lib
    from ssdr_al.prediction import WholeCloudPredictor
    _gpu()
    try:
        clouds = _room_pool(40)
        W = R.init_weights(0)
        rows = sum(max(len(c["xyz"]), 40960) for c in clouds)
        res = []
        for max_rows in (1 << 22, rows // 4 + 160000):
            pred = WholeCloudPredictor(W, max_rows=max_rows)
            out = pred.run(clouds, seed=2)
            assert out.check()[2] == 0
            views = [v for ch in out.chunks for v in _chunk_views(pred, out, ch)]
            res.append((len(out.chunks), views, out.to_host()))
        print("\n40 rooms, %d rows: %d and %d chunks" % (rows, res[0][0], res[1][0]))
        assert res[1][0] >= 4 and res[1][0] > res[0][0]
        for a, b in zip(res[0][1], res[1][1]):
            assert_bits_equal(a["xyz"], b["xyz"])
            for l in range(5):
                assert np.array_equal(a["neigh"][l], b["neigh"][l]) and np.array_equal(a["interp"][l], b["interp"][l])
        for a, b in zip(res[0][2], res[1][2]):
            assert np.abs(a["probs"] - b["probs"]).max() < 1e-4 and np.abs(a["feat32"] - b["feat32"]).max() < 1e-4
    finally:
        _lib.use(None)


@pytest.mark.gpu
def test_gpu_prediction_feeds_selection():
    """the predictor's resident outputs through HotPath.from_device (superpoints: synthetic.superpoints_from_tile) select what
    oracle/pipeline_np.selection_round selects from host copies of the same probabilities and features"""
    from oracle import pipeline_np as P
    from oracle import randla_np as R
    from ssdr_al import _lib, pipeline, synthetic
    from ssdr_al.helper_tool import ConfigS3DIS
    from ssdr_al.prediction import WholeCloudPredictor
    _gpu()
    try:
        clouds = _room_pool(6, seed0=9500)
        W = R.init_weights(0)
        out = WholeCloudPredictor(W).run(clouds, seed=1)
        out.check()
        host = out.to_host()
        args, batch_size, round_num, seed = ("sb", "WetSU", "clsbal", "gcn_fps"), 40, 2, 3
        hc, labelled, offs, pts, sp_cloud, lab_g, s0 = [], [], [np.zeros(1, np.int64)], [], [], {}, 0
        for b, h in enumerate(host):
            o, p = synthetic.superpoints_from_tile(h["xyz"])
            o = np.asarray(o, np.int64)
            hc.append(dict(xyz=h["xyz"], gt=h["labels"], probs=h["probs"], feat=h["feat32"], offsets=o, points=np.asarray(p, np.int64)))
            labelled.append(set(range(0, len(o) - 1, 7)))
            offs.append(o[1:] + offs[-1][-1]); pts.append(np.asarray(p, np.int64) + out.offsets[b]); sp_cloud.append(np.full(len(o) - 1, b, np.int32))
            lab_g[b] = set(s + s0 for s in labelled[-1]); s0 += len(o) - 1
        sel_list = np.random.default_rng(5).integers(0, 13, 300)
        kw = dict(sampler_args=args, gcn_number=1, gcn_top=0, min_size=1, round_num=round_num, label_seed=seed, batch_size=batch_size)
        hp = pipeline.HotPath.from_device(out.xyz, out.probs, out.feat32, out.labels, np.concatenate(offs), np.concatenate(pts), np.concatenate(sp_cloud),
                                          lab_g, sel_list, ConfigS3DIS, **kw)
        sel, unl = hp.step_selection()
        r = P.selection_round(hc, labelled, sel_list, 13, list(args), 1, round_num, batch_size, 1, 0, 0, np.random.RandomState(seed))
        base = np.asarray(hp.sp_base)
        assert [(b, s - int(base[b])) for b, s in unl] == r["unl"]
        assert len(sel) == batch_size and np.array_equal(sel, r["seq"])
    finally:
        _lib.use(None)
