"""The Semantic3D flavour of the whole-cloud prediction pass (ssdr_al.prediction.WholeCloudPredictor(dataset="Semantic3D")):
Semantic3D_Dataset_Sampling in mode "sampling" with TSampler.prediction() / compute_features() of the reference's SSRD_AL_semantic3d: every
point of a scan, shuffled, centred on all three axes, features augmented, split3 + merge into parts, one pyramid and one set of network rows
per part, total[point_idx[0]] = out.

CPU part (the CPU logic build and the gfx950 build alike, through the `backend` fixture): two levels, split_max 700 / split_recurse_max 500 /
merge_max 40 over five scans, each built for one path of the split (see SCANS); every stage against a NumPy restatement or the C oracle.
GPU part: the real ConfigSemantic3D over one scan of 60 000 points."""
import numpy as np
import pytest

from conftest import assert_bits_equal

SPLIT = dict(split_max=700, split_recurse_max=500, merge_max=40)
SEED = 3

# quadrant populations, in split3's order (x low / y low, x low / y high, x high / y low, x high / y high); a list in place of a count is a
# quadrant that is itself laid out by quadrants
SCANS = dict(
    A=[530, 529, 529, 529],                                  # 2 117: four parts, no recursion, no merge
    B=[500, [600, 1400, 900, 600], 500, 500],                # 5 000: 70 % in one quadrant, split again; its 600-point children are held against 500
    C=[500, 500, 475, 25],                                   # 1 500: the last quadrant joins the part before it
    D=[20, 500, 490, 490],                                   # 1 500: the FIRST quadrant stays a part of 20 rows (levels 20 / 5 / 1)
    E=[300, 300, 300, 300],                                  # 1 200 with 120 exact duplicates
)
TOO_SMALL = [10, 500, 500, 490]                              # first quadrant: levels 10 / 2 / 0


def _cfg():
    from ssdr_al.helper_tool import ConfigSemantic3D

    class Small(ConfigSemantic3D):
        num_layers = 2
        sub_sampling_ratio = [4, 4]
        d_out = [16, 64]
        num_classes = 8
    return Small


def _fill(rng, box, spec, out):
    """points of `spec` inside box = (x0, y0, x1, y1): a count is that many uniform points, two of them on opposite corners (they pin the
    bounding box split3 halves); a list is four quadrants, kept 5 % of the box away from the mid-lines so that no comparison is close"""
    x0, y0, x1, y1 = box
    if isinstance(spec, int):
        p = rng.random((spec, 2)) * [x1 - x0, y1 - y0] + [x0, y0]
        p[0], p[1] = (x0, y0), (x1, y1)
        out.append(p)
        return
    mx, my, gx, gy = 0.5 * (x0 + x1), 0.5 * (y0 + y1), 0.05 * (x1 - x0), 0.05 * (y1 - y0)
    for q, (xa, xb) in enumerate([(x0, mx - gx), (mx + gx, x1)]):
        for r, (ya, yb) in enumerate([(y0, my - gy), (my + gy, y1)]):
            _fill(rng, (xa, ya, xb, yb), spec[2 * q + r], out)


def _scan(name, spec, seed):
    rng = np.random.default_rng(seed)
    out = []
    _fill(rng, (0.0, 0.0, 4.0, 4.0), spec, out)
    xy = np.concatenate(out)
    xyz = np.concatenate([xy, rng.random((len(xy), 1)) * 2.0], 1).astype(np.float32)
    if name == "E":
        xyz[-120:] = xyz[:120]                 # exact duplicates: equal distances (tile ties) and equal KNN distances
    n = len(xyz)
    # colours as the Semantic3D loader holds them: the sub-sampled scans store rgb / 255 (utils/data_prepare_semantic3d.py:45, :70)
    return dict(xyz=xyz, rgb=(rng.integers(0, 256, (n, 3)) / 255.0).astype(np.float32), labels=rng.integers(0, 8, n).astype(np.int32))


def _scans(names="ABCDE"):
    return [_scan(k, SCANS[k], 40 + i) for i, k in enumerate(names)]


def _np_tile(cloud, d, color_scale):
    """tile.hip's rule with num_points = n (test_predict_clouds._np_tile with n == T): all rows by ascending float32 squared distance, ties by
    index, through the shuffle, minus the centre"""
    xyz, rgb = cloud["xyz"], cloud["rgb"].astype(np.float32)
    c = np.asarray(d["center"], np.float32)
    dd = xyz - c[None]
    dist = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
    ids = np.argsort(dist, kind="stable")[np.asarray(d["perm"])]
    return (xyz[ids] - c[None]).astype(np.float32), (rgb[ids] * np.float32(color_scale)).astype(np.float32), ids.astype(np.int32)


def _np_parts(t_xyz):
    from oracle import split3_np
    pl = []
    split3_np.split3(t_xyz, np.arange(len(t_xyz)), pl, SPLIT["split_max"], SPLIT["split_recurse_max"])
    return pl, split3_np.combine(pl, SPLIT["merge_max"])


def _oracle_knn():
    import oracle
    r = oracle.ref()
    if r is not None:
        return lambda s, q, k: r.knn(s, q, k, omp=True)
    o = oracle.c()
    return lambda s, q, k: o.knn_batch(s[None], q[None], k, threads=1)[0]


@pytest.fixture(scope="module")
def weights_small():
    from oracle import randla_np as R
    return R.init_weights(0, d_out=(16, 64), num_classes=8)


class Host:
    """host copies of everything one run left: the tiles, the split's order, and per part (over all scans, in order) its rows and tables"""

    def __init__(self, pred, clouds, out, draws):
        from ssdr_al.prediction import level_sizes, packed_positions
        cfg = pred.cfg
        L, ratios = cfg.num_layers, cfg.sub_sampling_ratio
        self.offsets = out.offsets
        self.draws = draws
        self.perm = out.inputs["perm"].to_host()
        self.noise = out.inputs["aug_noise"].to_host() if out.inputs["aug_noise"] is not None else None
        self.t_xyz, self.t_feat, self.t_idx = (out.inputs[k].to_host() for k in ("t_xyz", "t_feat", "t_idx"))
        self.order = out.inputs["order"].to_host()
        self.part_offsets = out.part_offsets
        self.scan_parts = out.parts
        self.probs, self.feat32 = out.probs.to_host(), out.feat32.to_host()
        self.chunks = [dict(lo=ch["lo"], hi=ch["hi"], parts=ch["parts"], P=ch["P"]) for ch in out.chunks]
        self.parts = []
        for ch in out.chunks:
            T, R, P = ch["T"], ch["R"], ch["P"]
            pos = packed_positions(T, ratios)
            cm_xyz, cm_n, cm_i = ch["cm_xyz"].to_host(), ch["cm_neigh"].to_host(), ch["cm_interp"].to_host()
            pk_n, pk_i = ch["pk_neigh"].to_host(), ch["pk_interp"].to_host()
            pk = {k: ch[k].to_host() for k in ("pk_xyz", "pk_feat", "pk_src", "pk_lab", "pk_probs", "pk_f32")}
            row0 = np.concatenate([[0], np.cumsum(T)])
            for k in range(len(T)):
                N = level_sizes(T[k], ratios)
                neigh, interp, pneigh, pinterp = [], [], [], []
                for l in range(L):
                    cmo = int(R[l]) + sum(level_sizes(T[j], ratios)[l] for j in range(k))
                    neigh.append(cm_n[cmo:cmo + N[l]]); interp.append(cm_i[cmo:cmo + N[l]])
                    rows = int(R[l]) + pos[k][:N[l]]
                    pneigh.append(pk_n[rows]); pinterp.append(pk_i[rows])
                scan, part = ch["parts"][k]
                a = int(ch["part_off"][k]), int(ch["part_off"][k + 1])
                p = dict(scan=scan, part=part, rows=self.order[a[0]:a[1]], base=int(ch["part_base"][k]), N=N, pos=pos[k], P=P,
                         xyz=cm_xyz[row0[k]:row0[k + 1]], neigh=neigh, interp=interp, pk_neigh=pneigh, pk_interp=pinterp)
                p.update({key: v[pos[k]] for key, v in pk.items()})
                self.parts.append(p)


_CACHE = {}


def _run(backend, W, names="ABCDE", max_rows=1 << 22, draws="host", poison=None, precision="f32", handed=None):
    """one run per (build, arguments), shared by the cases that read it (nothing below changes what it returns)"""
    key = (backend, names, max_rows, draws, poison, precision, handed is not None)
    if key not in _CACHE:
        from ssdr_al import _lib
        from ssdr_al.prediction import WholeCloudPredictor
        _lib.check(_lib.lib().ssdr_init(0))
        clouds = _scans(names)
        pred = WholeCloudPredictor(W, config=_cfg(), dataset="Semantic3D", precision=precision, max_rows=max_rows, draws=draws, **SPLIT)
        pred.poison = poison
        used = handed if handed is not None else [pred.draw_scan(c["xyz"], i, SEED) for i, c in enumerate(clouds)]
        out = pred.run(clouds, seed=SEED, draws=handed)
        out.check()
        _CACHE[key] = (pred, clouds, Host(pred, clouds, out, used))
    return _CACHE[key]


def _full_draws(h):
    """the draws of a run with the per-row entries the device holds"""
    out = []
    for c, d in enumerate(h.draws):
        o, e = int(h.offsets[c]), int(h.offsets[c + 1])
        out.append(dict(d, perm=h.perm[o:e], aug_noise=None if h.noise is None else h.noise[o:e]))
    return out


# ---- 1. tile and features ------------------------------------------------------------------------------------------------------------------

def _check_tile_and_features(pred, clouds, h):
    import _feed_oracle
    for c, (cl, d) in enumerate(zip(clouds, _full_draws(h))):
        o, e = int(h.offsets[c]), int(h.offsets[c + 1])
        assert sorted(d["perm"].tolist()) == list(range(e - o))
        txyz, col, ids = _np_tile(cl, d, pred.color_scale)
        assert_bits_equal(h.t_xyz[o:e], txyz, "scan %d tile xyz" % c)
        assert np.array_equal(h.t_idx[o:e], ids), "scan %d queried_idx" % c
        assert d["aug_noise"] is not None and d["aug_noise"].shape == (e - o, 3)
        aug = _feed_oracle.augment(txyz[None], np.asarray(d["rot"])[None], np.asarray(d["scale"])[None], d["aug_noise"][None])[0]
        assert_bits_equal(h.t_feat[o:e, :3], aug, "scan %d augmented xyz" % c)
        assert_bits_equal(h.t_feat[o:e, 3:], col, "scan %d colours" % c)
        assert np.abs(aug - txyz).max() > 1e-3                         # the augmentation did something


def test_tile_and_features(backend, weights_small):
    pred, clouds, h = _run(backend, weights_small)
    e = clouds[4]["xyz"]
    assert np.array_equal(e[-120:], e[:120])                           # scan E: tie rows in the tile
    _check_tile_and_features(pred, clouds, h)


# ---- 2. parts ------------------------------------------------------------------------------------------------------------------------------

def _check_parts(h):
    at = 0
    for c in range(len(h.offsets) - 1):
        o, e = int(h.offsets[c]), int(h.offsets[c + 1])
        leaves, exp = _np_parts(h.t_xyz[o:e])
        off = h.part_offsets[c]
        assert len(off) - 1 == len(exp), "scan %d: %d parts, the restatement has %d" % (c, len(off) - 1, len(exp))
        got = [h.order[o + off[k]:o + off[k + 1]] for k in range(len(exp))]
        for k, (g, x) in enumerate(zip(got, exp)):
            assert np.array_equal(g, x), "scan %d part %d" % (c, k)                    # leaf by leaf, ascending inside a leaf
            p = h.parts[at + k]
            assert (p["scan"], p["part"], p["base"]) == (c, k, o) and np.array_equal(p["rows"], g)
        for leaf in leaves:
            assert (np.diff(leaf) > 0).all()
        assert sorted(np.concatenate(got).tolist()) == list(range(e - o))              # a permutation of the tile rows
        assert np.array_equal(h.scan_parts[c]["offsets"], off) and all(np.array_equal(a, b) for a, b in zip(h.scan_parts[c]["rows"], got))
        at += len(exp)
    assert at == len(h.parts)


def _sizes(h, c):
    return np.diff(h.part_offsets[c]).tolist()


def test_parts(backend, weights_small):
    from oracle import split3_np
    pred, clouds, h = _run(backend, weights_small)
    _check_parts(h)
    # A: four quadrants, no recursion, no merge
    a = _sizes(h, 0)
    assert len(a) == 4 and max(a) <= 700 and min(a) > 40 and sum(a) == 2117
    # B: the dense quadrant is above 700 and is split again; a child between 500 and 700 is split as well (the recursion's own bound)
    o, e = int(h.offsets[1]), int(h.offsets[2])
    tx = h.t_xyz[o:e]
    top = []
    split3_np.split3(tx, np.arange(e - o), top, 1 << 30, 1 << 30)
    assert max(len(p) for p in top) == 3500 and e - o == 5000
    same, own = [], []
    split3_np.split3(tx, np.arange(e - o), same, 700, 700)
    split3_np.split3(tx, np.arange(e - o), own, 700, 500)
    kept = [len(p) for p in same if 500 < len(p) <= 700]
    assert kept and max(len(p) for p in own) <= 500 and len(own) > len(same)
    assert max(_sizes(h, 1)) <= 500
    # C: the last quadrant (25 points) joined the part before it
    leaves, exp = _np_parts(h.t_xyz[int(h.offsets[2]):int(h.offsets[3])])
    nz = [len(p) for p in leaves if len(p)]
    assert nz[-1] == 25 and _sizes(h, 2) == nz[:-2] + [nz[-2] + 25] and len(_sizes(h, 2)) == 3
    # D: the first quadrant (20 points) stays a part of its own
    assert _sizes(h, 3)[0] == 20 and len(_sizes(h, 3)) == 4


# ---- 3. packing ----------------------------------------------------------------------------------------------------------------------------

def _check_packing(clouds, h):
    labels = np.concatenate([c["labels"] for c in clouds])
    for p in h.parts:
        rows = p["base"] + p["rows"]
        what = "scan %d part %d" % (p["scan"], p["part"])
        assert_bits_equal(p["xyz"], h.t_xyz[rows], what + " part-major xyz")
        assert_bits_equal(p["pk_xyz"], h.t_xyz[rows], what + " packed xyz")
        assert_bits_equal(p["pk_feat"], h.t_feat[rows], what + " packed features")
        assert np.array_equal(p["pk_src"], p["base"] + h.t_idx[rows]), what
        assert np.array_equal(p["pk_lab"], labels[p["pk_src"]]), what
        for l in range(len(p["N"])):                                    # level l of every part = the first P_l packed rows
            assert (p["pos"][:p["N"][l]] < p["P"][l]).all() and (p["pos"][p["N"][l]:] >= p["P"][l]).all()
    for ch in h.chunks:
        pos = np.concatenate([p["pos"] for p in h.parts[ch["lo"]:ch["hi"]]])
        assert sorted(pos.tolist()) == list(range(int(ch["P"][0])))


def test_packing(backend, weights_small):
    pred, clouds, h = _run(backend, weights_small)
    assert len(h.chunks) == 1 and len(h.parts) > 20
    _check_packing(clouds, h)


# ---- 4. pyramid ----------------------------------------------------------------------------------------------------------------------------

def _check_pyramid(pred, h):
    knn = _oracle_knn()
    for p in h.parts:
        cur = p["xyz"]
        for l, r in enumerate(pred.cfg.sub_sampling_ratio):
            what = "scan %d part %d level %d" % (p["scan"], p["part"], l)
            nxt = cur[: len(cur) // r]
            assert_bits_equal(p["neigh"][l], knn(cur, cur, 16).astype(np.int32), what + " neigh")
            assert_bits_equal(p["interp"][l][:, None], knn(nxt, cur, 1).astype(np.int32), what + " interp")
            assert np.array_equal(p["pk_neigh"][l], p["pos"][p["neigh"][l]]), what
            assert np.array_equal(p["pk_interp"][l], p["pos"][p["interp"][l]]), what
            cur = nxt


def test_pyramid(backend, weights_small):
    """every part against the oracle KNN, scan D's 20-row part (levels 20 and 5, both below k_n) among them: what ssdr_knn_pyramid_dev with
    B = 1 gives for that part alone"""
    from ssdr_al import knn as K
    pred, clouds, h = _run(backend, weights_small)
    small = [p for p in h.parts if p["scan"] == 3 and p["part"] == 0]
    assert len(small) == 1 and small[0]["N"] == [20, 5, 1] and pred.cfg.k_n == 16
    _check_pyramid(pred, h)
    neigh, sub, interp = K.knn_pyramid(small[0]["xyz"][None], pred.cfg.sub_sampling_ratio, 16)
    for l in range(2):
        assert np.array_equal(neigh[l][0], small[0]["neigh"][l]) and np.array_equal(interp[l][0].reshape(-1), small[0]["interp"][l])


# ---- 5. network ----------------------------------------------------------------------------------------------------------------------------

def _check_network(pred, W, h):
    from oracle import randla_np as R
    from ssdr_al import _lib, randlanet
    cfg = pred.cfg
    net = randlanet.Network(cfg).load(W)
    for p in h.parts:
        T = len(p["xyz"])
        gp, gf = p["pk_probs"], p["pk_f32"]
        feat = p["pk_feat"][None]
        xyz = [p["xyz"][None, :n] for n in p["N"][:-1]]
        sub = [p["neigh"][l][None, :p["N"][l + 1]] for l in range(cfg.num_layers)]
        p64, f64 = R.forward(W, feat, xyz, [a[None] for a in p["neigh"]], sub, [a[None, :, None] for a in p["interp"]], dtype=np.float64)
        ep, ef = np.abs(gp - p64).max(), np.abs(gf - f64).max()
        assert ep < 3e-5 and ef < 1.1e-4, (p["scan"], p["part"], ep, ef)
        # the same part through the existing B = 1 entry point with its own pyramid
        d_feat, d_xyz = _lib.DevArray.from_host(feat), _lib.DevArray.from_host(p["xyz"][None])
        nb = [_lib.DevArray.from_host(a[None]) for a in p["neigh"]]; ip = [_lib.DevArray.from_host(a[None, :, None]) for a in p["interp"]]
        d_p, d_f = _lib.DevArray((T, cfg.num_classes), np.float32), _lib.DevArray((T, 32), np.float32)
        net.infer_dev(1, T, d_feat.ptr, d_xyz.ptr, [a.ptr for a in nb], [a.ptr for a in ip], d_p.ptr, d_f.ptr)
        _lib.sync()
        assert np.abs(gp - d_p.to_host()).max() < 1e-4 and np.abs(gf - d_f.to_host()).max() < 1e-4, (p["scan"], p["part"])


def test_network(backend, weights_small):
    pred, clouds, h = _run(backend, weights_small)
    _check_network(pred, weights_small, h)


# ---- 6. read-back --------------------------------------------------------------------------------------------------------------------------

def _check_readback(h):
    n = int(h.offsets[-1])
    written = np.zeros(n, np.int64)
    for p in h.parts:
        assert_bits_equal(h.probs[p["pk_src"]], p["pk_probs"], "scan %d part %d probs" % (p["scan"], p["part"]))
        assert_bits_equal(h.feat32[p["pk_src"]], p["pk_f32"], "scan %d part %d feat32" % (p["scan"], p["part"]))
        np.add.at(written, p["pk_src"], 1)
    assert (written == 1).all()                                         # every point in exactly one part
    assert np.isfinite(h.probs).all() and np.isfinite(h.feat32).all()   # ... and written: nothing of the poison is left


def test_readback(backend, weights_small):
    pred, clouds, h = _run(backend, weights_small, poison=float("nan"))
    assert np.isnan(pred.poison)
    _check_readback(h)
    _, _, plain = _run(backend, weights_small)
    assert_bits_equal(h.probs, plain.probs); assert_bits_equal(h.feat32, plain.feat32)


# ---- 7. chunking ---------------------------------------------------------------------------------------------------------------------------

def test_chunking(backend, weights_small):
    pred1, clouds, one = _run(backend, weights_small)
    pred2, _, many = _run(backend, weights_small, max_rows=2048)
    assert len(one.chunks) == 1 and len(many.chunks) > 3
    for ch in many.chunks:
        assert sum(len(p["rows"]) for p in many.parts[ch["lo"]:ch["hi"]]) <= 2048
    scans = [sorted({s for s, _ in ch["parts"]}) for ch in many.chunks]
    assert any(len(s) > 1 for s in scans)                                               # two scans share a chunk
    assert any(scans[i][-1] == scans[i + 1][0] for i in range(len(scans) - 1))          # a scan's parts span chunks
    assert len(one.parts) == len(many.parts)
    for a, b in zip(one.parts, many.parts):
        assert (a["scan"], a["part"]) == (b["scan"], b["part"]) and np.array_equal(a["rows"], b["rows"])
        assert_bits_equal(a["xyz"], b["xyz"]); assert_bits_equal(a["pk_feat"], b["pk_feat"])
        assert np.array_equal(a["pk_src"], b["pk_src"])
        for l in range(2):
            assert np.array_equal(a["neigh"][l], b["neigh"][l]) and np.array_equal(a["interp"][l], b["interp"][l])
    assert np.abs(one.probs - many.probs).max() < 1e-4 and np.abs(one.feat32 - many.feat32).max() < 1e-4
    _check_readback(many)


# ---- 8. draws="device" ---------------------------------------------------------------------------------------------------------------------

def test_device_draws(backend, weights_small):
    import _draw_oracle as O
    pred, clouds, h = _run(backend, weights_small, draws="device")
    assert pred.draws == "device"
    scale = pred.cfg.augment_noise
    assert scale > 0
    for c, d in enumerate(h.draws):
        assert set(d) == {"center", "rot", "scale"}                     # nothing per row comes from the host
        o, e = int(h.offsets[c]), int(h.offsets[c + 1])
        ds = pred.device_seed(SEED, c)
        assert np.array_equal(h.perm[o:e], O.perm(ds, 0, 0, 1, e - o)[0]), "scan %d perm" % c
        ref = O.normal(ds, 0, 0, O.AUG_NOISE, 3 * (e - o), scale=scale).reshape(e - o, 3)
        assert np.abs(h.noise[o:e] - ref).max() <= 1e-12 * scale, "scan %d noise" % c   # tests/test_draws.py's bar for this comparison
    # the rest of the pass with those draws: the checks of cases 1-6
    _check_tile_and_features(pred, clouds, h)
    _check_parts(h)
    _check_packing(clouds, h)
    _check_pyramid(pred, h)
    _check_network(pred, weights_small, h)
    _check_readback(h)
    # ... and handed in from the host they give the same pass
    _, _, again = _run(backend, weights_small, handed=_full_draws(h))
    assert_bits_equal(again.t_feat, h.t_feat); assert np.array_equal(again.order, h.order)
    assert np.abs(again.probs - h.probs).max() < 1e-4


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals(backend, weights_small):
    from ssdr_al import _lib
    from ssdr_al.prediction import WholeCloudPredictor, level_sizes
    _lib.check(_lib.lib().ssdr_init(0))
    cfg = _cfg()
    pred = WholeCloudPredictor(weights_small, config=cfg, dataset="Semantic3D", **SPLIT)
    good = _scan("A", SCANS["A"], 40)
    bad = _scan("X", TOO_SMALL, 77)
    d = pred.draw_scan(bad["xyz"], 1, SEED)
    txyz, _, _ = _np_tile(bad, d, 1.0)
    leaves, exp = _np_parts(txyz)
    assert len(exp[0]) == 10 and level_sizes(10, cfg.sub_sampling_ratio) == [10, 2, 0]
    with pytest.raises(_lib.SsdrError) as e:
        pred.run([good, bad], seed=SEED)
    assert e.value.status == 1 and "scan 1, part 0 (10 rows) is too small for the pyramid" in str(e.value)
    empty = dict(xyz=np.zeros((0, 3), np.float32), rgb=np.zeros((0, 3), np.float32), labels=np.zeros(0, np.int32))
    with pytest.raises(_lib.SsdrError) as e:
        pred.run([good, empty], seed=SEED)
    assert e.value.status == 1 and "scan 1 is empty" in str(e.value)
    with pytest.raises(ValueError) as e:
        pred.run([good], seed=SEED, readback="point")
    assert "readback" in str(e.value)
    with pytest.raises(ValueError):
        WholeCloudPredictor(weights_small, config=cfg, dataset="KITTI")
    with pytest.raises(_lib.SsdrError) as e:
        WholeCloudPredictor(weights_small, config=cfg, dataset="Semantic3D", max_rows=(1 << 23) + 1)
    assert e.value.status == 5 and "2^23" in str(e.value)
    with pytest.raises(ValueError):
        WholeCloudPredictor(weights_small, config=cfg, dataset="Semantic3D", max_rows=0)
    # the entries themselves
    L = _lib.lib()
    r = np.asarray(cfg.sub_sampling_ratio, np.int32)
    x = _lib.DevArray((64, 8), np.float32)
    off, base = np.array([0, 10, 40], np.int64), np.zeros(2, np.int64)
    assert L.ssdr_predict_parts_dev(x.ptr, x.ptr, x.ptr, None, x.ptr, _lib.ptr(off), _lib.ptr(base), 2, 2, _lib.ptr(r), x.ptr, x.ptr, x.ptr, x.ptr, None, None) == 1
    assert b"cloud 0 (10 rows) is too small for the pyramid" in L.ssdr_last_error()
    assert L.ssdr_predict_scan_tile_dev(x.ptr, x.ptr, 0, _lib.ptr(np.zeros(3, np.float32)), x.ptr, 1.0, x.ptr, x.ptr, x.ptr, None) == 1
    assert b"empty" in L.ssdr_last_error()
    assert L.ssdr_predict_scatter_dev(x.ptr, (1 << 23) + 1, x.ptr, 8, x.ptr, 64, x.ptr, x.ptr, None) == 5
    assert L.ssdr_predict_scatter_dev(x.ptr, 4, x.ptr, 0, x.ptr, 64, x.ptr, x.ptr, None) == 1


def test_scatter_skips_sources_outside_the_output(backend):
    """ssdr_predict_scatter_dev on coded rows: every row lands at its source, a source outside [0, num_out) writes nothing"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    _lib.check(_lib.lib().ssdr_init(0))
    rows, n, Cn = 1000, 1200, 13
    rng = np.random.default_rng(2)
    src = rng.permutation(n)[:rows].astype(np.int32)
    src[5], src[77] = -1, n
    pp = rng.random((rows, Cn), dtype=np.float32); pf = rng.random((rows, 32), dtype=np.float32)
    probs = DevArray.from_host(np.full((n, Cn), -7, np.float32)); feat = DevArray.from_host(np.full((n, 32), -7, np.float32))
    d_src, d_pp, d_pf = DevArray.from_host(src), DevArray.from_host(pp), DevArray.from_host(pf)
    _lib.check(_lib.lib().ssdr_predict_scatter_dev(d_src.ptr, rows, d_pp.ptr, Cn, d_pf.ptr, n, probs.ptr, feat.ptr, None))
    _lib.sync()
    ep, ef = np.full((n, Cn), -7, np.float32), np.full((n, 32), -7, np.float32)
    ok = (src >= 0) & (src < n)
    ep[src[ok]], ef[src[ok]] = pp[ok], pf[ok]
    assert_bits_equal(probs.to_host(), ep); assert_bits_equal(feat.to_host(), ef)


# ---- 10. selection composes ----------------------------------------------------------------------------------------------------------------

def test_selection_composes(backend, weights_small):
    """HotPath.from_device over the pass's resident result selects the regions it selects from the same arrays handed in from the host"""
    from ssdr_al import _lib, pipeline, synthetic
    from ssdr_al._lib import DevArray
    from ssdr_al.prediction import WholeCloudPredictor
    _lib.check(_lib.lib().ssdr_init(0))
    cfg = _cfg()
    clouds = _scans("AC")
    out = WholeCloudPredictor(weights_small, config=cfg, dataset="Semantic3D", **SPLIT).run(clouds, seed=SEED)
    out.check()
    host = out.to_host()
    offs, pts, sp_cloud, lab_g, s0 = [np.zeros(1, np.int64)], [], [], {}, 0
    for b, h in enumerate(host):
        o, p = synthetic.superpoints_from_tile(h["xyz"])
        o = np.asarray(o, np.int64)
        offs.append(o[1:] + offs[-1][-1]); pts.append(np.asarray(p, np.int64) + out.offsets[b]); sp_cloud.append(np.full(len(o) - 1, b, np.int32))
        lab_g[b] = set(s + s0 for s in range(0, len(o) - 1, 7)); s0 += len(o) - 1
    sel_list = np.random.default_rng(5).integers(0, 8, 100)
    kw = dict(sampler_args=("sb", "WetSU", "clsbal", "gcn_fps"), selector="fps", gcn_number=1, gcn_top=0, min_size=1, round_num=2, label_seed=3, batch_size=12,
              max_size=1000, chamfer_mode="f32_cuda")
    args = (np.concatenate(offs), np.concatenate(pts), np.concatenate(sp_cloud), lab_g, sel_list, cfg)
    got = pipeline.HotPath.from_device(out.xyz, out.probs, out.feat32, out.labels, *args, **kw).step_selection()
    cat = lambda k: np.concatenate([h[k] for h in host])
    again = pipeline.HotPath.from_device(DevArray.from_host(cat("xyz")), DevArray.from_host(cat("probs")), DevArray.from_host(cat("feat32")),
                                         DevArray.from_host(cat("labels")), *args, **kw).step_selection()
    assert len(got[0]) == 12 and np.array_equal(got[0], again[0]) and list(got[1]) == list(again[1])


# ---- GPU: the real configuration -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_real_configuration_against_oracle():
    """ConfigSemantic3D (five levels, ratios 4 4 4 4 2), one scan of 60 000 points with a dense quadrant, split_max 20 000, merge_max 2 000:
    pyramids bit for bit per part, probs / feat32 within 1e-3 of the float32 NumPy oracle in f32 and bf16x3, f32 within 1e-4 of per-part B = 1
    product calls (the bars of test_predict_clouds.test_gpu_whole_rooms_against_oracle)"""
    from conftest import GPU_LIB, _have_gpu
    if not _have_gpu():
        pytest.skip("no GPU")
    from oracle import randla_np as R
    from ssdr_al import _lib, randlanet
    from ssdr_al.helper_tool import ConfigSemantic3D
    from ssdr_al.prediction import WholeCloudPredictor
    _lib.use(GPU_LIB)
    _lib.check(_lib.lib().ssdr_init(0))
    try:
        cfg = ConfigSemantic3D
        rng = np.random.default_rng(11)
        out = []
        _fill(rng, (0.0, 0.0, 9.0, 7.0), [7000, [9000, 8000, 10001, 7999], 9000, 9000], out)
        xy = np.concatenate(out)
        n = len(xy)
        assert n == 60000
        xyz = np.concatenate([xy, rng.random((n, 1)) * 3.0], 1).astype(np.float32)
        xyz[-3000:] = xyz[:3000]
        clouds = [dict(xyz=xyz, rgb=(rng.integers(0, 256, (n, 3)) / 255.0).astype(np.float32), labels=rng.integers(0, 8, n).astype(np.int32))]
        W = R.init_weights(0, num_classes=8)
        knn = _oracle_knn()
        net = randlanet.Network(cfg).load(W)
        ref = None
        for prec in ("f32", "bf16x3"):
            pred = WholeCloudPredictor(W, config=cfg, dataset="Semantic3D", precision=prec, split_max=20000, split_recurse_max=20000, merge_max=2000)
            res = pred.run(clouds, seed=4)
            assert res.check()[2] == 0
            h = Host(pred, clouds, res, None)
            sizes = [len(p["rows"]) for p in h.parts]
            assert len(sizes) >= 6 and any(s % 512 for s in sizes) and max(sizes) <= 20000 and sum(sizes) == n
            if ref is None:
                ref = []
                for p in h.parts:
                    cur = p["xyz"]
                    for l, r in enumerate(cfg.sub_sampling_ratio):
                        nxt = cur[: len(cur) // r]
                        assert_bits_equal(p["neigh"][l], knn(cur, cur, 16).astype(np.int32), "part %d level %d neigh" % (p["part"], l))
                        assert_bits_equal(p["interp"][l][:, None], knn(nxt, cur, 1).astype(np.int32), "part %d level %d interp" % (p["part"], l))
                        cur = nxt
                    xs = [p["xyz"][None, :m] for m in p["N"][:-1]]
                    sub = [p["neigh"][l][None, :p["N"][l + 1]] for l in range(cfg.num_layers)]
                    ref.append(R.forward(W, p["pk_feat"][None], xs, [a[None] for a in p["neigh"]], sub, [a[None, :, None] for a in p["interp"]], dtype=np.float32))
            for k, p in enumerate(h.parts):
                gp, gf = p["pk_probs"], p["pk_f32"]
                ep, ef = np.abs(gp - ref[k][0]).max(), np.abs(gf - ref[k][1]).max()
                print("\n%s part %d (%d rows): max |probs - oracle| %.3g, |feat32 - oracle| %.3g" % (prec, k, sizes[k], ep, ef))
                assert ep < 1e-3 and ef < 1e-3, (prec, k, ep, ef)
                if prec == "f32":
                    T = sizes[k]
                    d_feat, d_xyz = _lib.DevArray.from_host(p["pk_feat"][None]), _lib.DevArray.from_host(p["xyz"][None])
                    nb = [_lib.DevArray.from_host(a[None]) for a in p["neigh"]]; ip = [_lib.DevArray.from_host(a[None, :, None]) for a in p["interp"]]
                    d_p, d_f = _lib.DevArray((T, 8), np.float32), _lib.DevArray((T, 32), np.float32)
                    net.infer_dev(1, T, d_feat.ptr, d_xyz.ptr, [a.ptr for a in nb], [a.ptr for a in ip], d_p.ptr, d_f.ptr)
                    _lib.sync()
                    assert np.abs(gp - d_p.to_host()).max() < 1e-4 and np.abs(gf - d_f.to_host()).max() < 1e-4
            _check_readback(h)
    finally:
        _lib.use(None)
