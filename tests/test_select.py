"""Selection-stage parity: HIP kernels through the C ABI / the reference-named mirror against the golden vectors
made by the reference's own Python, and against oracle/select_np.py on fresh inputs.  Index sequences and integer
outputs must be identical; float64 quantities within 1e-12 relative (summation order of BLAS / exp differ)."""
import numpy as np
import pytest

from oracle import select_np as O


def test_point_uncertainty_golden(backend, golden):
    from ssdr_al import sampler
    g = golden("select_golden.npz")
    for mode in ("lc", "sb"):
        u, c = sampler.compute_point_uncertainty(g["u/prob"], [mode], return_class=True)
        assert np.array_equal(u, g["u/pu_" + mode]), mode            # bit-exact float32
        assert np.array_equal(c, np.argmax(g["u/prob"], -1))
    u = sampler.compute_point_uncertainty(g["u/prob"], ["entropy"])
    assert np.allclose(u, g["u/pu_entropy"], rtol=2e-6, atol=1e-7)   # log2f differs in the last ulp


def test_region_stats_golden(backend, golden):
    from ssdr_al import sampler
    g = golden("select_golden.npz")
    cls = np.argmax(g["u/prob"], -1).astype(np.int32)
    for mode in ("mean", "sum_weight", "WetSU"):
        ru, dom, cnt = sampler.compute_region_stats(g["u/pu_sb"], cls, g["u/offsets"], g["u/points"], 13, [mode])
        assert np.allclose(ru, g["u/ru_" + mode], rtol=1e-12, atol=0), mode
        assert np.array_equal(dom, g["u/dom"])
    ru, dom, cnt = sampler.compute_region_stats(g["u/pu_sb"], cls, g["u/offsets"], g["u/points"], 13, ["WetSU"])
    assert np.array_equal(ru, g["u/ru_WetSU"])                        # NumPy's pairwise order reproduced exactly
    lab, pur = sampler.dominant_labels(cls, g["u/offsets"], g["u/points"], 13)
    assert np.array_equal(lab, g["u/dom"]) and np.allclose(pur, g["u/purity"], rtol=1e-15)
    cb = sampler.add_clsbal(13, g["u/dom"], g["u/ru_WetSU"], {"selected_class_list": list(g["u/selected_class_list"])})
    assert np.allclose(cb, g["u/clsbal"], rtol=1e-13)
    order = sampler.rank_regions(cb)
    assert np.array_equal(order, O.rank_regions(cb))


def test_chamfer_adjacency_gcnfps_golden(backend, golden):
    from ssdr_al import sampler
    g = golden("select_golden.npz")
    clouds = {}
    for name in ("cloudA", "cloudB"):
        xyz, off, pts = g["f/%s/xyz" % name], g["f/%s/offsets" % name], g["f/%s/points" % name]
        clouds[name] = (xyz, off, pts)
        cd = sampler.create_cd(xyz, off, pts, np.arange(len(off) - 1))
        assert np.allclose(cd, g["f/%s/cd" % name], rtol=1e-13, atol=1e-15)
    names = ["cloudA", "cloudB"]
    unl = [{"cloud_name": names[c], "sp_idx": int(s)} for c, s in zip(g["f/unl_cloud"], g["f/unl_sp"])]
    lab = [{"cloud_name": names[c], "sp_idx": int(s)} for c, s in zip(g["f/lab_cloud"], g["f/lab_sp"])]
    # the reference's global adjacency, block by block
    refs = unl + lab
    for c, name in enumerate(names):
        rows = [i for i, r in enumerate(refs) if r["cloud_name"] == name]
        sel = [refs[i]["sp_idx"] for i in rows]
        _, _, adj = sampler.cloud_graph(*clouds[name], sel)
        assert np.allclose(adj, g["f/adj"][np.ix_(rows, rows)], rtol=1e-12, atol=1e-15)
    for gn in (1, 2, 3):
        fl = sampler.GCN_FPS_sampling(list(g["f/lab_feat"]), lab, list(g["f/unl_feat"]), unl, clouds, 5, gn, 0, int(g["f/gcnfps_start_%d" % gn]))
        assert fl.get("cloudA", []) == list(g["f/gcnfps_A_%d" % gn]) and fl.get("cloudB", []) == list(g["f/gcnfps_B_%d" % gn])
    # gcn_top > 0 (fps_gcn_cpu.py:153-160; the reference's scripts run --gcn_top 100): masked adjacency and selections
    for gt in (2, 3, 5, 13):
        for c, name in enumerate(names):
            rows = [i for i, r in enumerate(refs) if r["cloud_name"] == name]
            _, _, adj = sampler.cloud_graph(*clouds[name], [refs[i]["sp_idx"] for i in rows], gcn_top=gt)
            assert np.allclose(adj, g["f/adj_top%d" % gt][np.ix_(rows, rows)], rtol=1e-12, atol=1e-15), (gt, name)
        for gn in (1, 2):
            fl = sampler.GCN_FPS_sampling(list(g["f/lab_feat"]), lab, list(g["f/unl_feat"]), unl, clouds, 5, gn, gt, int(g["f/gcnfps_start_%d" % gn]))
            assert fl.get("cloudA", []) == list(g["f/gcnfps_top%d_A_%d" % (gt, gn)]) and fl.get("cloudB", []) == list(g["f/gcnfps_top%d_B_%d" % (gt, gn)]), (gt, gn)
    with pytest.raises(IndexError):          # the reference's mask assignment cannot broadcast when gcn_top exceeds the matrix size (:159)
        sampler.GCN_FPS_sampling(list(g["f/lab_feat"]), lab, list(g["f/unl_feat"]), unl, clouds, 5, 1, 14, 0)


def test_gcn_top_100_golden(backend, golden):
    """fps_gcn_cpu.GCN_FPS_sampling with the reference scripts' own --gcn_top 100 (and 5) on 70 + 60 superpoints: the masked adjacency
    (:153-160) and the selections, gcn_number 1 and 2."""
    from ssdr_al import sampler
    g = golden("select_golden.npz")
    names = ["cloudC", "cloudD"]
    clouds = {n: (g["g/%s/xyz" % n], g["g/%s/offsets" % n], g["g/%s/points" % n]) for n in names}
    unl = [{"cloud_name": names[c], "sp_idx": int(s)} for c, s in zip(g["g/unl_cloud"], g["g/unl_sp"])]
    lab = [{"cloud_name": names[c], "sp_idx": int(s)} for c, s in zip(g["g/lab_cloud"], g["g/lab_sp"])]
    refs = unl + lab
    for gt in (5, 100):
        for name in names:
            rows = [i for i, r in enumerate(refs) if r["cloud_name"] == name]
            _, _, adj = sampler.cloud_graph(*clouds[name], [refs[i]["sp_idx"] for i in rows], gcn_top=gt)
            want = g["g/adj_top%d" % gt][np.ix_(rows, rows)]                   # stored as float32
            assert np.allclose(adj, want, rtol=2e-7, atol=1e-12), (gt, name)
            assert np.array_equal(adj != 0, want != 0), (gt, name)             # the same entries survive the mask
        for gn in (1, 2):
            fl = sampler.GCN_FPS_sampling(list(g["g/lab_feat"]), lab, list(g["g/unl_feat"]), unl, clouds, 20, gn, gt, int(g["g/start"]))
            assert fl.get("cloudC", []) == list(g["g/gcnfps_top%d_C_%d" % (gt, gn)]), (gt, gn)
            assert fl.get("cloudD", []) == list(g["g/gcnfps_top%d_D_%d" % (gt, gn)]), (gt, gn)


def test_chamfer_mixed_superpoint_sizes(backend):
    """create_cd over superpoints of 1 ... 1700 points: several small ones share a wave (256-slot items), those above 256 points go pair
    by pair in passes, the one above 1536 points is streamed as a target; a subset in a shuffled order as `sel`."""
    from ssdr_al import sampler
    rng = np.random.default_rng(31)
    sizes = [1, 2, 3, 17, 40, 24, 64, 63, 2, 65, 130, 128, 127, 129, 100, 30, 256, 257, 16, 16, 17, 300, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 9, 700, 31, 33, 1700, 12, 64, 1]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(off[-1])
    xyz = (rng.random((n, 3)) * np.array([4, 3, 2])).astype(np.float32)
    for s_, (a, b) in enumerate(zip(off[:-1], off[1:])):             # compact blobs around random seats
        xyz[a:b] = (rng.random(3) * np.array([4, 3, 2]) + rng.normal(0, 0.08, (b - a, 3))).astype(np.float32)
    pts = rng.permutation(n).astype(np.int32)
    xyz = xyz[np.argsort(pts)]                                        # superpoint s = the points listed in pts[off[s]:off[s+1]]
    cent = O.bbox_centres(xyz, off, pts)
    want = O.create_cd(xyz, off, pts, cent)
    got = sampler.create_cd(xyz, off, pts, np.arange(len(sizes)))
    assert np.allclose(got, want, rtol=1e-12, atol=1e-14)
    sel = rng.permutation(len(sizes))[:20]
    got = sampler.create_cd(xyz, off, pts, sel)
    assert np.allclose(got, want[np.ix_(sel, sel)], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("kind", ["blobs", "duplicates", "lattice"])
def test_chamfer_matrix_screening_equals_float64(backend, kind, monkeypatch):
    """The float32 screening on the matrix cores (select_chamfer.hip) against the float64 kernel it replaced (SSDR_CHAMFER_F64=1), the same call twice:
    the same bits where the nearest target point is unique (random blobs; duplicated points tie at EQUAL coordinates, so the distance is the same
    whichever copy is named), within the last ulps on a lattice (equally near targets at different offsets).  Sizes on both sides of every path:
    items shared by several superpoints, passes of 256 over larger ones, targets of one to twenty tiles of 32 and one beyond the staging limit."""
    from ssdr_al import sampler
    rng = np.random.default_rng({"blobs": 51, "duplicates": 52, "lattice": 53}[kind])
    sizes = [1, 2, 5, 31, 32, 33, 64, 90, 100, 127, 128, 160, 200, 255, 256, 257, 300, 420, 511, 640, 641, 700, 9, 17, 40, 75]
    # targets beyond the staging limit are walked chunk by chunk, the workgroup's waves in lockstep (CH_TILE = 640 points per chunk in either build): one,
    # two and several chunks, as target and as source
    sizes += [1000] if backend == "emu" else [961, 1300, 2049, 3001]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(off[-1])
    xyz = np.empty((n, 3), np.float32)
    for a, b in zip(off[:-1], off[1:]):
        seat = rng.random(3) * np.array([6, 5, 2.5]) + 20.0
        if kind == "lattice": blob = seat.round(1) + rng.integers(-4, 5, (b - a, 3)) * 0.25          # many exactly equal distances
        else: blob = seat + rng.normal(0, 0.12, (b - a, 3)) * np.array([1.5, 1.0, 0.4])
        if kind == "duplicates" and b - a > 4: blob[(b - a) // 2:] = blob[: (b - a) - (b - a) // 2]   # every point twice: the runs tie exactly
        xyz[a:b] = blob.astype(np.float32)
    pts = rng.permutation(n).astype(np.int32)
    xyz = xyz[np.argsort(pts)]
    sel = np.arange(len(sizes))
    got = sampler.create_cd(xyz, off, pts, sel)
    monkeypatch.setenv("SSDR_CHAMFER_F64", "1")
    ref = sampler.create_cd(xyz, off, pts, sel)
    monkeypatch.delenv("SSDR_CHAMFER_F64")
    if kind == "lattice": assert np.allclose(got, ref, rtol=4e-16, atol=0)
    else: assert np.array_equal(got, ref)
    cent = O.bbox_centres(xyz, off, pts)
    assert np.allclose(got, O.create_cd(xyz, off, pts, cent), rtol=1e-12, atol=1e-14)


def test_chamfer_empty_superpoint_both_forms_agree(backend, monkeypatch):
    """an EMPTY superpoint among the targets (the reference's partition never makes one; the header documents it as supported): the screening on the matrix
    cores, the float64 kernel behind SSDR_CHAMFER_F64 and the streamed form for targets beyond the staging limit give the same matrix — the 1e300 sentinel's
    root where nothing can be nearest, never a stale LDS value (the advisor's round-5 finding)"""
    from ssdr_al import sampler
    rng = np.random.default_rng(77)
    sizes = [5, 0, 40, 130, 0, 700, 12]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(off[-1])
    xyz = (rng.random((n, 3)) * 3.0 + 10.0).astype(np.float32)
    pts = rng.permutation(n).astype(np.int32)
    sel = np.arange(len(sizes))
    got = sampler.create_cd(xyz, off, pts, sel)
    monkeypatch.setenv("SSDR_CHAMFER_F64", "1")
    ref = sampler.create_cd(xyz, off, pts, sel)
    monkeypatch.delenv("SSDR_CHAMFER_F64")
    assert np.array_equal(got, ref, equal_nan=True)
    live = np.array([s > 0 for s in sizes])
    assert np.isfinite(got[np.ix_(live, live)]).all()
    # a non-empty source against an empty target: every point's "nearest" distance is the sentinel's root
    assert np.all(got[np.ix_(live, ~live)] >= 1e149)


@pytest.mark.parametrize("scale", [1e-3, 1.0, 50.0, 80.0, 250.0])
def test_chamfer_matrix_screening_at_other_scales(backend, scale, monkeypatch):
    """The screening's error bound has absolute terms (half-precision subnormals) and a range limit (|p|^2 <= 1000 m^2 after centring): superpoints a
    few tenths of a millimetre across are mostly left to the float64 sweep, superpoints tens of metres across take the float64 kernel's path inside
    the screening kernel — the values must not change."""
    from ssdr_al import sampler
    rng = np.random.default_rng(61)
    sizes = [5, 40, 130, 257, 300, 64, 33]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(off[-1])
    xyz = np.empty((n, 3), np.float32)
    for a, b in zip(off[:-1], off[1:]):
        xyz[a:b] = ((rng.random(3) * np.array([6, 5, 2.5]) + rng.normal(0, 0.12, (b - a, 3))) * scale).astype(np.float32)
    pts = np.arange(n, dtype=np.int32)
    sel = np.arange(len(sizes))
    got = sampler.create_cd(xyz, off, pts, sel)
    monkeypatch.setenv("SSDR_CHAMFER_F64", "1")
    ref = sampler.create_cd(xyz, off, pts, sel)
    monkeypatch.delenv("SSDR_CHAMFER_F64")
    assert np.array_equal(got, ref)
    cent = O.bbox_centres(xyz, off, pts)
    assert np.allclose(got, O.create_cd(xyz, off, pts, cent), rtol=1e-12, atol=1e-14 * scale)


@pytest.mark.gpu
def test_chamfer_f32_cuda_flavour(backend):
    """Semantic3D's create_cd_cuda (SSRD_AL_semantic3d/fps_gcn_cuda.py:13-30): float32 CUDA-kernel chamfer values in the graph — ssdr_select_set_chamfer_mode(1)
    against the NumPy float32 restatement (parity unpinned: the CUDA op cannot run here; 1e-6 relative = the freedom of a float32 mean's order), and the
    adjacency built from them; the float64 default is a different matrix (1e-7 .. 1e-6 apart) and comes back with mode 0"""
    from oracle import select_np as S
    from ssdr_al import sampler
    rng = np.random.default_rng(23)
    sizes = np.array([1, 3, 17, 64, 65, 130, 300, 700, 40, 2, 90, 513])      # below / above a wave, above the staging slab
    n = int(sizes.sum())
    cen = rng.random((len(sizes), 3)) * 5.0
    xyz = (np.repeat(cen, sizes, axis=0) + rng.normal(0, 0.2, (n, 3))).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32); points = rng.permutation(n).astype(np.int32)
    xyz_s = np.empty_like(xyz); xyz_s[points] = xyz            # region s holds the points points[offsets[s]:offsets[s+1]]
    sel = np.arange(len(sizes), dtype=np.int32)
    c64, cd64, _ = sampler.cloud_graph(xyz_s, offsets, points, sel)
    sampler.set_chamfer_mode("f32_cuda")
    try:
        c, cd, adj = sampler.cloud_graph(xyz_s, offsets, points, sel)
    finally:
        sampler.set_chamfer_mode("f64")
    exp = S.create_cd_cuda(xyz_s, offsets, points, S.bbox_centres(xyz_s, offsets, points))
    assert np.array_equal(c, c64)
    assert np.allclose(cd, exp, rtol=2e-6, atol=0) and np.array_equal(np.diag(cd), np.zeros(len(sizes)))
    assert np.allclose(adj, S.block_adjacency(c, exp), rtol=1e-5, atol=1e-12)
    assert not np.array_equal(cd, cd64) and np.allclose(cd, cd64, rtol=1e-5)
    assert np.array_equal(sampler.cloud_graph(xyz_s, offsets, points, sel)[1], cd64)


def test_chamfer_more_superpoints_than_the_packer_lays_out():
    """4300 superpoints in one cloud (> PACK_MAX = 4096): the packer hands every superpoint to the pair-by-pair path.  The summation
    rule depends on a superpoint's size alone, so any sub-block must equal the packed computation over just those superpoints, bit for bit."""
    from conftest import GPU_LIB, _have_gpu
    if not _have_gpu():
        pytest.skip("no GPU")
    from ssdr_al import _lib, sampler
    _lib.use(GPU_LIB)
    try:
        rng = np.random.default_rng(41)
        sizes = rng.integers(1, 40, 4300); sizes[:5] = (130, 300, 16, 17, 1)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        n = int(off[-1])
        seats = rng.random((4300, 3)) * np.array([20, 15, 3])
        xyz = np.concatenate([c + rng.normal(0, 0.1, (s_, 3)) for c, s_ in zip(seats, sizes)]).astype(np.float32)
        pts = np.arange(n, dtype=np.int32)
        full = sampler.create_cd(xyz, off, pts, np.arange(4300))
        sub = np.concatenate([np.arange(8), rng.choice(4300, 60, replace=False)])
        part = sampler.create_cd(xyz, off, pts, sub)
        assert np.array_equal(full[np.ix_(sub, sub)], part)
        cent = O.bbox_centres(xyz, off[: 9], pts[: off[8]])
        assert np.allclose(part[:8, :8], O.create_cd(xyz, off[: 9], pts[: off[8]], cent), rtol=1e-12, atol=1e-14)
    finally:
        _lib.use(None)


def test_fps_and_kcenter_golden(backend, golden):
    from ssdr_al import sampler
    g = golden("select_golden.npz")
    assert np.array_equal(sampler.farthest_features_sample(g["fps/feat"], 50, int(g["fps/start"])), g["fps/seq"])
    kc = sampler.kCenterGreedy(g["kc/feat"])
    assert kc.select_batch_(g["kc/already"], 30) == list(g["kc/seq"])


@pytest.mark.parametrize("n,count", [(1537, 300), (4736, 600)])
def test_fps_mid_sizes_against_the_oracle(backend, n, count):
    """Candidate sets between the register-resident single workgroup (n <= 1536) and 16384 rows — the sharded run's replicated global FPS
    (2 / 4 / 8 ranks: 2368 / 4736 / 9472 candidates) — take the cooperative multi-workgroup kernel on the GPU (the single-workgroup sweep
    on the CPU logic build): the sequence is the oracle's, index for index."""
    from ssdr_al import sampler
    if backend == "emu":
        n, count = min(n, 1800), min(count, 40)
    f = np.random.default_rng(n).normal(size=(n, 32))
    f[n // 3] = f[n // 5]                                   # an exact duplicate: a tie the arg-max settles by index
    assert np.array_equal(sampler.farthest_features_sample(f, count, 7), O.farthest_features_sample(f, count, 7))


@pytest.mark.parametrize("n,count", [(300, 120), (700, 200), (1184, 400), (2368, 300)])
def test_fps_ties_take_the_first_index(backend, n, count):
    """Every row twice, at shuffled positions: at every pick the farthest candidate has a twin at the same distance, in the same wave or in another
    one (or another workgroup of the cooperative kernel), and np.argmax takes the lower index (fps_gcn_cpu.py:141).  The wave arg-max finds the maximum
    value first and then the smallest index among its holders: this is the case that tells the two apart."""
    from ssdr_al import sampler
    if backend == "emu":
        count = min(count, 40)
    rng = np.random.default_rng(n)
    half = rng.normal(size=(n // 2, 32))
    f = np.concatenate([half, half])[rng.permutation(n)]
    assert np.array_equal(sampler.farthest_features_sample(f, count, 3), O.farthest_features_sample(f, count, 3))


def test_compute_features_mean_golden(backend, golden):
    """np.mean(last_second_features[dominant_point_ids], axis=0) (sampler2.py:333, :339) with the reference's own _dominant_2 ids."""
    from ssdr_al import sampler
    g = golden("select_golden.npz")
    cls = np.argmax(g["u/prob"], -1).astype(np.int32)
    mf = sampler.segment_mean_features(g["u/feat32"], cls, g["u/dom"], g["u/offsets"], g["u/points"])
    assert np.array_equal(mf, g["u/segmean"])                           # bit-exact float32 (row-sequential sums, one division)
    assert np.array_equal(O.segment_mean_features(g["u/feat32"], g["u/offsets"], g["u/points"], cls, g["u/dom"]), g["u/segmean"])


def test_kcenter_larger_golden_and_at_scale(backend, golden):
    """kCenterGreedy.select_batch_ (kcenterGreedy.py:60-128) with the labelled rows as already_selected (gcn.py:247): 1000 x 129
    against the reference's own sequence; on the GPU also 20000 x 129 against the oracle."""
    from ssdr_al import sampler
    g = golden("select_golden.npz")
    kc = sampler.kCenterGreedy(g["kc2/feat"])
    assert kc.select_batch_(g["kc2/already"], 80) == list(g["kc2/seq"])
    assert np.array_equal(O.kcenter_greedy(g["kc2/feat"].astype(np.float64), g["kc2/already"], 80), g["kc2/seq"])
    if backend == "gpu":
        rng = np.random.default_rng(5)
        f = rng.normal(0, 1, (20000, 129)).astype(np.float32)
        already = np.arange(17000, 20000)
        got = sampler.kCenterGreedy(f).select_batch_(already, 300)
        assert got == list(O.kcenter_greedy(f.astype(np.float64), already, 300))
        assert len(set(got)) == 300 and not set(got) & set(already.tolist())


def test_kcenter_seeding_at_the_rounds_scale(backend):
    """the seeding of kCenterGreedy (min distance to every already-selected row, kcenterGreedy.py:72-82) for many rows x many seeds on 32-d features — the
    shape of the reference's own round (24 000 rows, 4 000 seeds) takes the tiled kernel (rows in registers, seeds through LDS, seed slices met by an atomic
    minimum): the picks are the oracle's, index for index, duplicates among the seeds and a seed that is also the farthest row's twin included"""
    from ssdr_al import sampler
    n, na, count = (3000, 1400, 30) if backend == "emu" else (24000, 4000, 400)
    rng = np.random.default_rng(12)
    f = rng.normal(0, 1, (n, 32)).astype(np.float32)
    already = rng.choice(n, na, replace=False)
    f[already[3]] = f[already[5]]                      # two equal seeds
    f[(already[7] + 1) % n] = f[already[7]]            # a row at distance 0 from a seed
    got = sampler.kCenterGreedy(f).select_batch_(already, count)
    assert got == list(O.kcenter_greedy(f.astype(np.float64), already, count))
    assert len(set(got)) == count and not set(got) & set(already.tolist())


def test_edcd_farthest_superpoint_sample_golden(backend, golden):
    from ssdr_al import sampler
    g = golden("select_golden.npz")
    xyz, off, pts = g["f/cloudA/xyz"], g["f/cloudA/offsets"], g["f/cloudA/points"]
    seq = sampler.farthest_superpoint_sample(xyz, off, pts, np.arange(len(off) - 1), 5, 0)
    assert np.array_equal(seq, g["f6/seq"])
    rng = np.random.default_rng(8)
    sel = rng.permutation(len(off) - 1)[:6]
    assert np.array_equal(sampler.farthest_superpoint_sample(xyz, off, pts, sel, 4, 2), O.farthest_superpoint_sample(xyz, off, pts, sel, 4, 2))


def test_selection_fresh_inputs_against_oracle(backend):
    from ssdr_al import sampler
    rng = np.random.default_rng(21)
    n, C = (18000, 13) if backend == "emu" else (300000, 13)
    prob = rng.dirichlet(np.ones(C) * 0.5, n).astype(np.float32)
    feat = rng.normal(0, 1, (n, 32)).astype(np.float32)
    # above / at the wave routine's staging capacity (larger ones are staged node by node of the recursion), several blocks of the pairwise sum, one block; and
    # above 8192 members — NumPy's reduction works through its 8192-element buffer: pairwise(first 8192) + pairwise(next 8192) + ..., not one recursion
    sizes = [8193, 2500, 1300, 1025, 1024, 700, 129, 128]
    if backend != "emu":
        sizes = [40003, 20011, 16385, 16384, 12000, 8200, 8192, 4099] + sizes          # floors and walls of a real partition
    while sum(sizes) < n:
        sizes.append(int(rng.integers(5, 400)))
    sizes[-1] -= sum(sizes) - n
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pts = rng.permutation(n).astype(np.int32)
    u, cls = sampler.compute_point_uncertainty(prob, ["sb"], return_class=True)
    assert np.array_equal(u, O.point_uncertainty(prob, "sb"))
    ru, dom, cnt = sampler.compute_region_stats(u, cls, off, pts, C, ["WetSU"])
    eru, edom, ecnt = O.region_stats(u, cls, off, pts, C, "WetSU")
    b64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)          # on the bits: np.array_equal cannot see the sign of a zero
    assert np.array_equal(b64(ru), b64(eru)) and np.array_equal(dom, edom) and np.array_equal(cnt, ecnt)
    for mode in ("mean", "sum_weight"):                     # NumPy's pairwise order in every mode, for every size class
        assert np.array_equal(b64(sampler.compute_region_stats(u, cls, off, pts, C, [mode])[0]), b64(O.region_stats(u, cls, off, pts, C, mode)[0])), mode
    sel = O.rank_regions(ru)[:40].astype(np.int32)
    mf = sampler.segment_mean_features(feat, cls, dom, off, pts, sel)
    sub_off = np.concatenate([[0], np.cumsum(off[sel + 1] - off[sel])]).astype(np.int32)
    sub_pts = np.concatenate([pts[off[s]:off[s + 1]] for s in sel])
    assert np.array_equal(mf, O.segment_mean_features(feat, sub_off, sub_pts, cls, dom[sel]))   # bit-exact float32
    m = 2000 if backend == "emu" else 20000
    f = rng.normal(0, 1, (m, 32))
    k = 60 if backend == "emu" else 600
    assert np.array_equal(sampler.farthest_features_sample(f, k, 17), O.farthest_features_sample(f, k, 17))


def test_create_adj_of_the_gcn_branch(backend, golden):
    """gcn.create_adj (gcn.py:116-191), torch float32 in the reference: golden from the reference's own function on the 70 + 60 superpoint
    fixture (tests/golden/make_golden_gcn.py).  Float32 dot products / column sums in another order than torch's: 2e-4 relative to max(|entry|, 1)."""
    from ssdr_al import sampler
    g = golden("select_golden.npz"); G = golden("gcn_golden.npz")
    names = ["cloudC", "cloudD"]
    clouds = {n: (g["g/%s/xyz" % n], g["g/%s/offsets" % n], g["g/%s/points" % n]) for n in names}
    unl = [{"cloud_name": names[c], "sp_idx": int(s)} for c, s in zip(g["g/unl_cloud"], g["g/unl_sp"])]
    lab = [{"cloud_name": names[c], "sp_idx": int(s)} for c, s in zip(g["g/lab_cloud"], g["g/lab_sp"])]
    V, adj = sampler.create_adj(np.concatenate([g["g/unl_feat"], g["g/lab_feat"]]), lab, unl, clouds)
    assert V.dtype == np.float32 and adj.dtype == np.float32 and adj.shape == (130, 130)
    assert np.abs(V - G["featuresV"]).max() < 1e-6
    # the columns are scaled by 1 / (their float32 sum), and a sum of ~130 entries of both signs can come close to 0: its rounding (which
    # depends on the order torch adds in) is what remains — relative to the entry, not absolute
    err = (np.abs(adj - G["adj"]) / np.maximum(np.abs(G["adj"]), 1.0)).max()
    print("\ncreate_adj on %s: max |adj - reference| / max(|reference|, 1) = %.3g (tolerance 2e-4), |adj| max %.3g" % (backend, err, np.abs(G["adj"]).max()))
    assert err < 2e-4
    cross = adj[:55, 55:100]                       # candidates of cloud C against candidates of cloud D: exactly 0
    assert np.all(cross == 0)


@pytest.mark.gpu
def test_cooperative_fps_reports_a_launch_that_is_not_co_resident():
    """fps_coop / fps_coop_reg are G workgroups that meet at a counter per pick: they need all G resident together.  The grid is now taken
    from the occupancy query (and refused otherwise), a workgroup that waits too long raises an abort flag every workgroup tests at every pick,
    and the stream's selection status carries it to the host (ssdr_select_status -> SSDR_ERR_INTERNAL).  SSDR_FPS_COOP_G forces a grid above
    residency (4096 workgroups of 256 threads on 256 CUs x 8): the call must report the failure, with the picks behind the abort reading -1 —
    and the same problem without the override must give the reference's sequence."""
    from conftest import GPU_LIB, _have_gpu
    if not _have_gpu():
        pytest.skip("no GPU")
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    worker = os.path.join(root, "tests", "_fps_coop_worker.py")
    env = dict(os.environ); env.pop("SSDR_FPS_COOP_G", None)
    ok = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert ok.returncode == 0, ok.stderr[-2000:]
    assert "RC 0 STATUS 0 MINUS 0" in ok.stdout and "MATCH 1" in ok.stdout, ok.stdout
    env["SSDR_FPS_COOP_G"] = "4096"
    bad = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert bad.returncode == 0, bad.stderr[-2000:]
    line = [l for l in bad.stdout.splitlines() if l.startswith("RC")][0].split()
    assert int(line[1]) != 0 and int(line[3]) & 1 and int(line[5]) > 0, bad.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("budget", ["", "40"])
def test_cooperative_chains_in_flight_on_several_streams(budget):
    """Three cooperative chains on three streams enqueued back to back (`--select-lag 2` keeps three global chains in flight): every launch is
    sized against the co-resident workgroups, so their SUM must fit as well — the library keeps an account of the cooperative grids in
    flight and makes a launch's stream wait for the oldest ones when it would not (select_fps.hip: CoopGuard).  With the default budget and with a
    budget of one chain's grid (full serialisation, SSDR_FPS_COOP_BUDGET) all three give the reference's sequences and no stream reports an abort."""
    from conftest import GPU_LIB, _have_gpu
    if not _have_gpu():
        pytest.skip("no GPU")
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ); env.pop("SSDR_FPS_COOP_BUDGET", None); env.pop("SSDR_FPS_COOP_G", None)
    if budget:
        env["SSDR_FPS_COOP_BUDGET"] = budget
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_fps_coop_multi_worker.py")], capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ALL 1" in r.stdout, r.stdout
