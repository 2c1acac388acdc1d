"""RandLA-Net inference, dispatch branch by dispatch branch, against the float64 oracle (oracle/randla_np.py).

test_randla.py checks the reference's one configuration (d_out 16..512, in_dim 6, C 13) end to end through infer(), at
a 1e-3 bar against the fp32 oracle.  Here the network is fed directly (Network.infer_dev) with index tables the test
uploads itself, so network parity is separate from KNN parity, and the sweep reaches the launcher branches that
configuration never takes: one attention width per level, d = 16 at a deep level, the unfused fc1 / fc2 / head for
C not in {8, 13} or a last width other than 32, in_dim 3 and 7 (scalar-load and non-row forms of the thin layers),
both sides of the row-count thresholds (1024: the one-row-per-lane forms; 16384: 32- or 128-row tiles), odd level
sizes (the point-pair tail of lfa32_l0_kernel), a deepest level of one row per batch, tile extents from 0.1 m to
50 m and a tile whose 16 neighbours all coincide with the point (|d| = 0).

Every case names the profiler scopes (ssdr_prof_report) its dispatch must reach, per arithmetic family ("f32"; the
bf16 modes with the 32 x 32-tile formulation, "t32"; with the 16 x 16-tile kernels, "t16"), and the ones it must
not reach ("!name"); test_cases_cover_every_randla_profiler_scope checks that the union covers every ProfScope name
of randla_*.hip.

Bars: max |x - fp64 oracle| over probabilities (p) and last_second_features (f); for plain bf16 also the relative RMS of
feat32 (rrms) and the share of points whose argmax class agrees with the oracle.  Worst case over the matrix, tiles of
0.1 .. 4 m (|feat32| <= 18):

    precision   CPU logic build (emu subset)                 MI355X (whole matrix)
    f32         p 3.3e-06  f 2.0e-05                         p 7.6e-06  f 2.7e-05
    bf16x3      p 1.3e-04  f 3.8e-04                         p 1.1e-04  f 3.4e-04
    bf16        p 0.055  f 0.16  rrms 0.0099  agree 0.978    p 0.055  f 0.16  rrms 0.0099  agree 0.978

Tiles of ~50 m (extent_50, knn_semantic3d: |feat32| up to 141): every absolute error grows with the features, so feat32
is held relative to its largest magnitude there (frel = max |f - f64| / max |f64|):

    f32         p 1.6e-05  f 2.8e-04  frel 2.0e-06           p 2.0e-05  f 3.7e-04  frel 2.7e-06
    bf16x3      p 6.7e-04  f 8.4e-03  frel 5.9e-05           p 5.6e-04  f 9.1e-03  frel 6.5e-05
    bf16        p 0.375  f 3.3  frel 0.024  rrms 0.010  agree 0.992 (both)

Bars: 4 x the worst of both columns, and no f32 / bf16x3 bar above 1e-3; argmax floors 1 - 2 x the worst disagreement.
Plain bf16 keeps test_randla.py's 0.08 / 0.8 on the few-metre tiles.  Split bf16 therefore holds 1e-3 only while the
features stay small: at 50 m its feat32 is 9e-3 off in absolute terms (6.5e-5 relative), plain bf16's probabilities 0.375.
"""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BARS = {"f32": dict(p=3e-5, f=1.1e-4), "bf16x3": dict(p=5.2e-4, f=1e-3), "bf16": dict(p=0.08, f=0.8, rrms=0.04, agree=0.957)}
# tiles of ~50 m: probabilities keep a max-abs bar (none for plain bf16), feat32 is held relative to its largest magnitude
BARS_WIDE = {"f32": dict(p=8.2e-5, frel=1.1e-5), "bf16x3": dict(p=1e-3, frel=2.6e-4), "bf16": dict(frel=0.095, rrms=0.041, agree=0.984)}

# (precision, tiles32): f32 has one formulation (set_formulation only switches the bf16 modes)
MODES = [("f32", True), ("bf16x3", True), ("bf16x3", False), ("bf16", True), ("bf16", False)]


def _family(prec, tiles32):
    return "f32" if prec == "f32" else ("t32" if tiles32 else "t16")


class Case:
    def __init__(self, name, d_out, ratios, N, B=1, C=13, in_dim=6, tables="synth", extent=4.0, emu=True, reach=None, why=""):
        self.name, self.d_out, self.ratios, self.N, self.B, self.C, self.in_dim = name, list(d_out), list(ratios), N, B, C, in_dim
        self.tables, self.extent, self.emu, self.reach, self.why = tables, extent, emu, reach or {}, why

    def sizes(self):
        s = [self.N]
        for r in self.ratios:
            s.append(s[-1] // r)
        return s


# reach: family -> profiler scopes the run must report ("!name": must NOT report).  "dense_kernel" is the vector-load f32 tile
# (dense_small_kernel up to 16384 rows, dense_kernel<true> above), "dense_kernel<false>" the scalar-load one.
CASES = [
    Case("w16", [16], [4], 1024, why="d = 16 alone; 1024 rows: fc0 + mlp1 in one row pass; C 13 + last width 32: fused tails",
         reach={"f32": ["dense_rows_kernel", "lfa_att_kernel", "dense_kernel", "gather_max_kernel", "tail_kernel", "!head_kernel"],
                "t32": ["dense_rows_kernel", "lfa32_l0_kernel", "dense_chain_kernel<16>", "dense_bf16_kernel<32,64>", "tail_kernel", "!lfa_att_kernel"],
                "t16": ["dense_rows_kernel", "lfa_att_kernel", "dense_chain_kernel<16>", "tail_kernel", "!lfa32_l0_kernel"]}),
    Case("w16_1023_rows", [16], [4], 1023, why="1023 rows (< 1024): fc0 6 -> 8 on the scalar-load tile, mlp1 + the coordinate fill on the vector tile; "
                                                "odd N: the last point pair of lfa32_l0 is half empty",
         reach={"f32": ["dense_kernel<false>", "dense_kernel", "!dense_rows_kernel"], "t32": ["dense_kernel<false>", "dense_kernel", "lfa32_l0_kernel", "!dense_rows_kernel"],
                "t16": ["dense_kernel<false>", "!dense_rows_kernel"]}),
    Case("w64", [64], [4], 1024, why="d = 64 at level 0: lfa32_res<64> at level 0, mlp1 8 -> 32 (no fused row pass), last width 128: unfused fc1 / fc2 / head",
         reach={"f32": ["dense_rows_kernel", "dense_kernel", "lfa_att_kernel", "head_kernel", "!tail_kernel"],
                "t32": ["lfa32_res_kernel<64>", "dense_chain_kernel<64>", "dense_bf16_kernel<32,64>", "head_kernel", "!tail_kernel"],
                "t16": ["lfa_att_kernel", "dense_chain_kernel<64>", "head_kernel", "!lfa32_res_kernel<64>"]}),
    Case("w128", [128], [4], 512, reach={"f32": ["lfa_att_kernel", "head_kernel"], "t32": ["lfa32_kernel<128>", "head_kernel"], "t16": ["lfa_att_kernel", "!lfa32_kernel<128>"]}),
    Case("w256", [256], [4], 256, reach={"f32": ["lfa_att_kernel"], "t32": ["lfa32_kernel<256>"], "t16": ["lfa_att_kernel", "!lfa32_kernel<256>"]}),
    Case("w512", [512], [2], 128, reach={"f32": ["lfa_att_kernel"], "t32": ["lfa32_kernel<512>"], "t16": ["lfa_att_kernel", "!lfa32_kernel<512>"]}),
    Case("mix_64_16", [64, 16], [4, 4], 1030, B=3, C=20,
         why="d = 16 at level 1 (257 rows, odd): the gather table and lfa32_l0 away from level 0; its 128-wide shortcut: no dense_chain<16>; C 20: head",
         reach={"f32": ["head_kernel"], "t32": ["lfa32_res_kernel<64>", "lfa32_l0_kernel", "dense_chain_kernel<64>", "!dense_chain_kernel<16>", "head_kernel"],
                "t16": ["dense_chain_kernel<64>", "!dense_chain_kernel<16>", "head_kernel"]}),
    Case("mix_512_64", [512, 64], [2, 4], 130, why="d = 512 at level 0, d = 64 deep with a 1024-wide shortcut: no dense_chain<64>",
         reach={"t32": ["lfa32_kernel<512>", "lfa32_res_kernel<64>", "!dense_chain_kernel<64>"], "t16": ["!dense_chain_kernel<64>"]}),
    Case("c1", [16, 64], [4, 4], 1024, C=1, reach={"f32": ["head_kernel", "!tail_kernel"], "t32": ["head_kernel", "!tail_kernel"], "t16": ["head_kernel"]}),
    Case("c8", [16, 64], [4, 4], 1024, C=8, reach={"f32": ["tail_kernel", "!head_kernel"], "t32": ["tail_kernel", "!head_kernel"], "t16": ["tail_kernel"]}),
    Case("c32", [16, 64], [4, 4], 1024, C=32, reach={"f32": ["head_kernel", "dense_kernel"], "t32": ["head_kernel", "dense_bf16_kernel<32,64>"], "t16": ["head_kernel"]}),
    Case("in3", [16, 64], [4, 4], 1024, in_dim=3, why="fc0 3 -> 8: no row form; mlp1 8 -> 8 alone on the row form",
         reach={"f32": ["dense_kernel<false>", "dense_rows_kernel"], "t32": ["dense_kernel<false>", "dense_rows_kernel"], "t16": ["dense_kernel<false>"]}),
    Case("in7", [16, 64], [4, 4], 1024, in_dim=7, reach={"f32": ["dense_kernel<false>", "dense_rows_kernel"], "t32": ["dense_kernel<false>", "dense_rows_kernel"]}),
    Case("odd_levels", [16, 64], [3, 3], 1017, B=2, why="odd N at every level (1017, 339, 113)"),
    Case("deep_1row", [16, 64, 128], [4, 4, 65], 1040, B=3, why="the deepest level has one row per batch element (1040, 260, 65, 1)",
         reach={"t32": ["lfa32_l0_kernel", "lfa32_res_kernel<64>", "lfa32_kernel<128>"]}),
    Case("rows_16384", [16], [4], 16384, C=20, emu=False, why="16384 rows: the last size on 32-row bf16 tiles", reach={"t32": ["dense_bf16_kernel<32,64>", "!dense_bf16_kernel<128,32>"]}),
    Case("rows_16385", [16], [4], 16385, C=20, why="16385 rows: 128-row tiles (bf16 and f32)", reach={"t32": ["dense_bf16_kernel<128,32>"], "t16": ["dense_bf16_kernel<128,32>"]}),
    Case("extent_0.1", [16, 64], [4, 4], 1024, extent=0.1),
    Case("extent_50", [16, 64], [4, 4], 1024, extent=50.0),
    Case("coincident", [16, 64], [4, 4], 1024, tables="self", why="every neighbour is the point itself: |d| = 0 in every LocSE row"),
    Case("knn_reference", [16, 64, 128, 256, 512], [4, 4, 4, 4, 2], 1024, tables="knn", why="the reference's network on KNN-built tables"),
    Case("knn_semantic3d", [16, 64, 128, 256, 512], [4, 4, 4, 4, 2], 65536, tables="knn", extent=50.0, emu=False,
         why="a Semantic3D-sized tile (65 536 points, ~50 m): LocSE rounding grows with |p|",
         reach={"f32": ["dense_rows_kernel", "tail_kernel"], "t32": ["lfa32_l0_kernel", "tail_kernel", "!dense_bf16_kernel<128,32>"]}),
]
# plain-emu subset: the bf16 modes of the wide single-level cases cost seconds each on the CPU build
EMU_MODES = {"w512": [("f32", True), ("bf16x3", True)], "mix_512_64": [("bf16x3", True), ("bf16", False)], "rows_16385": [("f32", True), ("bf16x3", True)],
             "knn_reference": [("f32", True), ("bf16x3", True), ("bf16", True)]}


def _cfg(d_out, C, ratios):
    return type("Cfg", (), dict(num_layers=len(d_out), d_out=list(d_out), k_n=16, num_classes=C, sub_sampling_ratio=list(ratios)))


def _tables(kind, xyz, sizes, rng):
    """neigh[i] [B, N_i, 16] into level i (its first N_i points), interp[i] [B, N_i, 1] into level i + 1; sub_idx[i] is neigh[i]'s prefix."""
    B = xyz.shape[0]
    if kind == "knn":
        import oracle
        from oracle import randla_np as R
        o = oracle.c()
        ratios = [sizes[i] // sizes[i + 1] for i in range(len(sizes) - 1)]
        _, neigh, _, interp = R.build_pyramid(xyz, ratios, lambda s, q, k: o.knn_batch(s, q, k, threads=8))
        return neigh, interp
    neigh, interp = [], []
    for i in range(len(sizes) - 1):
        n, m = sizes[i], sizes[i + 1]
        if kind == "self":
            nb = np.repeat(np.arange(n, dtype=np.int32)[None, :, None], B, 0).repeat(16, 2)
        else:
            nb = rng.integers(0, n, (B, n, 16)).astype(np.int32)
            nb[:, :, 0] = np.arange(n)                          # the point itself first, as KNN gives it
            nb[:, ::7, 5] = n - 1                               # the last point of the level
            nb[:, n - 1, :] = n - 1
            nb[:, 1::11, :] = nb[:, 1::11, 3:4]                 # all 16 neighbours the same point
            nb[:, 2::13, :] = np.arange(n)[2::13, None]         # all 16 the point itself
        it = rng.integers(0, m, (B, n, 1)).astype(np.int32)
        it[:, ::5] = m - 1                                      # the last point of the next level
        it[:, -1] = m - 1
        neigh.append(np.ascontiguousarray(nb))
        interp.append(it)
    return neigh, interp


def _inputs(case, seed=0):
    rng = np.random.default_rng(seed)
    B, N = case.B, case.N
    xyz = ((rng.random((B, N, 3)) - 0.5) * case.extent * np.array([1.0, 0.8, 0.3])).astype(np.float32)
    xyz[:, : N // 4, 2] = xyz[:, : N // 4, 2].min()              # a floor
    feat = np.concatenate([xyz - xyz.mean(1, keepdims=True), rng.random((B, N, 3))], -1)[:, :, : case.in_dim]
    if case.in_dim > feat.shape[2]:
        feat = np.concatenate([feat, rng.normal(size=(B, N, case.in_dim - feat.shape[2]))], -1)
    neigh, interp = _tables(case.tables, xyz, case.sizes(), rng)
    return xyz, np.ascontiguousarray(feat, np.float32), neigh, interp


def _oracle(W, case, xyz, feat, neigh, interp):
    from oracle import randla_np as R
    sz = case.sizes()
    sub = [neigh[i][:, : sz[i + 1]] for i in range(len(case.ratios))]
    return R.forward(W, feat, [xyz[:, :s] for s in sz[:-1]], neigh, sub, interp, dtype=np.float64)


def _run(case, W, xyz, feat, neigh, interp, prec, tiles32, B=None, prof=False):
    """infer_dev on tables uploaded here -> (probs [B*N, C], feat32 [B*N, 32], profiler scope names or None)"""
    from ssdr_al import _lib, randlanet
    B = B or xyz.shape[0]
    net = randlanet.Network(_cfg(case.d_out, case.C, case.ratios), in_dim=case.in_dim).load(W).set_precision(prec).set_formulation(tiles32)
    dx, df = _lib.DevArray.from_host(xyz), _lib.DevArray.from_host(feat)
    dn, di = [_lib.DevArray.from_host(a) for a in neigh], [_lib.DevArray.from_host(a) for a in interp]
    probs, f32 = _lib.DevArray((B * case.N, case.C), np.float32), _lib.DevArray((B * case.N, 32), np.float32)
    L = _lib.lib()
    names = None
    if prof:
        L.ssdr_prof_report()                                   # drop anything recorded before
        L.ssdr_prof_enable(1)
    try:
        net.infer_dev(B, case.N, df.ptr, dx.ptr, [a.ptr for a in dn], [a.ptr for a in di], probs.ptr, f32.ptr)
        _lib.sync()
    finally:
        if prof:
            names = {ln.rsplit(" ", 4)[0] for ln in L.ssdr_prof_report().decode().splitlines() if ln.strip()}
            L.ssdr_prof_enable(0)
    return probs.to_host(), f32.to_host(), names


def _errors(gp, gf, p64, f64):
    ep, ef = float(np.abs(gp - p64).max()), float(np.abs(gf - f64).max())
    rrms = float(np.sqrt(np.mean((gf - f64) ** 2) / max(np.mean(f64 ** 2), 1e-30)))
    agree = float(np.mean(gp.argmax(1) == p64.argmax(1)))
    return ep, ef, rrms, agree


_PREPARED = {}


def _prepared(case):
    """weights, inputs and the fp64 oracle's outputs of a case (shared by its five precision / formulation runs)"""
    if case.name not in _PREPARED:
        from oracle import randla_np as R
        W = R.init_weights(7, tuple(case.d_out), case.C, case.in_dim)
        xyz, feat, neigh, interp = _inputs(case)
        _PREPARED.clear()
        _PREPARED[case.name] = (W, xyz, feat, neigh, interp) + tuple(_oracle(W, case, xyz, feat, neigh, interp))
    return _PREPARED[case.name]


def _check_case(case, prec, tiles32, backend):
    W, xyz, feat, neigh, interp, p64, f64 = _prepared(case)
    gp, gf, names = _run(case, W, xyz, feat, neigh, interp, prec, tiles32, prof=True)
    assert gp.shape == p64.shape and gf.shape == f64.shape
    assert np.isfinite(gp).all() and np.isfinite(gf).all()
    ep, ef, rrms, agree = _errors(gp, gf, p64, f64)
    print("\nMEASURED %s %s %s %s: p %.3g f %.3g frel %.3g rrms %.3g agree %.4f |f| max %.3g" % (backend, case.name, prec, "t32" if tiles32 else "t16", ep, ef, ef / np.abs(f64).max(), rrms, agree, np.abs(f64).max()))
    fam = _family(prec, tiles32)
    for nm in case.reach.get(fam, []):
        if nm.startswith("!"):
            assert nm[1:] not in names, "%s / %s: dispatch reached %s (%s)" % (case.name, fam, nm[1:], sorted(names))
        else:
            assert nm in names, "%s / %s: dispatch did not reach %s (%s)" % (case.name, fam, nm, sorted(names))
    assert np.abs(gp.sum(1) - 1).max() < 1e-5
    if case.extent >= 20:
        bar, frel = BARS_WIDE[prec], ef / np.abs(f64).max()
        assert ep < bar.get("p", 1.0) and frel < bar["frel"], (case.name, prec, tiles32, ep, frel)
    else:
        bar = BARS[prec]
        assert ep < bar["p"] and ef < bar["f"], (case.name, prec, tiles32, ep, ef)
    if prec == "bf16":
        assert rrms < bar["rrms"] and agree >= bar["agree"], (case.name, tiles32, rrms, agree)


def _params(gpu):
    out = []
    for c in CASES:
        for prec, t32 in MODES:
            pid = "%s-%s-%s" % (c.name, prec, "t32" if t32 else "t16")
            if gpu:
                out.append(pytest.param(c, prec, t32, id=pid))
            elif c.emu and (prec, t32) in EMU_MODES.get(c.name, MODES):
                out.append(pytest.param(c, prec, t32, id=pid))
    return out


@pytest.mark.parametrize("case,prec,tiles32", _params(False))
def test_path_against_fp64_oracle_emu(emu_lib, case, prec, tiles32):
    from ssdr_al import _lib
    _lib.use(emu_lib)
    try:
        _check_case(case, prec, tiles32, "emu")
    finally:
        _lib.use(None)


@pytest.mark.gpu
@pytest.mark.parametrize("case,prec,tiles32", _params(True))
def test_path_against_fp64_oracle_gpu(case, prec, tiles32):
    from conftest import GPU_LIB, _have_gpu
    if not _have_gpu():
        pytest.skip("no GPU")
    from ssdr_al import _lib
    _lib.use(GPU_LIB)
    try:
        _check_case(case, prec, tiles32, "gpu")
    finally:
        _lib.use(None)


def _scopes_in_sources():
    names = set()
    for fn in glob.glob(os.path.join(ROOT, "ssdr-al_amd", "csrc", "randla_*.hip")):
        src = open(fn).read()
        for m in re.finditer(r"ProfScope\s+\w+\((.*?),\s*s\s*,", src):
            names.update(re.findall(r'"([^"]+)"', m.group(1)))
    return names


def test_cases_cover_every_randla_profiler_scope():
    """The union of what the cases must reach (each GPU case checks its own list against ssdr_prof_report) covers every profiler
    scope of the RandLA-Net launchers: a launcher added or renamed without a case fails here; each case's list, at run time."""
    src = _scopes_in_sources()
    assert len(src) >= 15, sorted(src)
    reached = {nm for c in CASES for lst in c.reach.values() for nm in lst if not nm.startswith("!")}
    assert src - reached == set(), "scopes no case reaches: %s" % sorted(src - reached)
    assert reached - src == set(), "cases name scopes the sources do not have: %s" % sorted(reached - src)
    emu_reached = {nm for c in CASES if c.emu for fam, lst in c.reach.items() for nm in lst if not nm.startswith("!")
                   and any(_family(*m) == fam for m in EMU_MODES.get(c.name, MODES))}
    assert src - emu_reached == set(), "scopes the emu subset does not reach: %s" % sorted(src - emu_reached)


def test_profiler_reports_names_on_emu(emu_lib):
    """the coverage checks rely on ssdr_prof_report naming the launches in the CPU logic build too"""
    case = CASES[0]
    from oracle import randla_np as R
    from ssdr_al import _lib
    _lib.use(emu_lib)
    try:
        W = R.init_weights(7, tuple(case.d_out), case.C, case.in_dim)
        _, _, names = _run(case, W, *_inputs(case), "f32", True, prof=True)
    finally:
        _lib.use(None)
    assert {"dense_rows_kernel", "lfa_att_kernel", "gather_max_kernel", "tail_kernel"} <= names, names


# ---- batch independence: B = 3 distinct tiles, every slot bit-identical to that tile alone ------------------------------------
# (row counts chosen so that B = 1 and B = 3 take the same kernels at every level: 2048 / 6144 rows on the one-row-per-lane
# and 32-row-tile sides of both thresholds)
BATCH_CASES = [Case("batch_16_64", [16, 64], [4, 4], 2048, B=3), Case("batch_64_16", [64, 16], [2, 4], 4800, B=3, C=20)]


def _check_batch(case, prec, tiles32):
    from oracle import randla_np as R
    W = R.init_weights(11, tuple(case.d_out), case.C, case.in_dim)
    xyz, feat, neigh, interp = _inputs(case, seed=5)
    assert not np.array_equal(xyz[0], xyz[1]) and not np.array_equal(neigh[0][0], neigh[0][1])
    gp, gf, _ = _run(case, W, xyz, feat, neigh, interp, prec, tiles32)
    N = case.N
    for b in range(case.B):
        sp, sf, _ = _run(case, W, xyz[b:b + 1], feat[b:b + 1], [a[b:b + 1] for a in neigh], [a[b:b + 1] for a in interp], prec, tiles32, B=1)
        assert np.array_equal(gp[b * N:(b + 1) * N].view(np.uint32), sp.view(np.uint32)), (case.name, prec, tiles32, b, "probs")
        assert np.array_equal(gf[b * N:(b + 1) * N].view(np.uint32), sf.view(np.uint32)), (case.name, prec, tiles32, b, "feat32")


# (plain emu: the second case in two modes only, for time)
@pytest.mark.parametrize("case,prec,tiles32", [pytest.param(c, p, t, id="%s-%s-%s" % (c.name, p, "t32" if t else "t16")) for c in BATCH_CASES for p, t in MODES
                                               if c is BATCH_CASES[0] or (p, t) in (("f32", True), ("bf16x3", True))])
def test_batch_slots_independent_emu(emu_lib, case, prec, tiles32):
    from ssdr_al import _lib
    _lib.use(emu_lib)
    try:
        _check_batch(case, prec, tiles32)
    finally:
        _lib.use(None)


@pytest.mark.gpu
@pytest.mark.parametrize("prec,tiles32", MODES)
@pytest.mark.parametrize("case", BATCH_CASES, ids=lambda c: c.name)
def test_batch_slots_independent_gpu(case, prec, tiles32):
    from conftest import GPU_LIB, _have_gpu
    if not _have_gpu():
        pytest.skip("no GPU")
    from ssdr_al import _lib
    _lib.use(GPU_LIB)
    try:
        _check_batch(case, prec, tiles32)
    finally:
        _lib.use(None)


# ---- what the ABI refuses --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,what", [((1, [16], 16, 13, 0), "in_dim"), ((1, [16], 16, 13, -2), "in_dim"), ((1, [32], 16, 13, 6), "d_out"),
                                       ((1, [16], 16, 33, 6), "num_classes"), ((1, [16], 16, 0, 6), "num_classes"), ((1, [16], 8, 13, 6), "k_n")])
def test_create_refuses_unsupported_configurations(emu_lib, args, what):
    from ssdr_al import _lib
    _lib.use(emu_lib)
    try:
        L, d, k, C, ind = args
        h = ctypes.c_void_p()
        dd = np.asarray(d, np.int32)
        rc = _lib.lib().ssdr_randla_create(L, _lib.ptr(dd), k, C, ind, ctypes.byref(h))
        assert rc == 5 and not h.value, (rc, what)            # SSDR_ERR_UNSUPPORTED, no handle
        assert what in _lib.lib().ssdr_last_error().decode()
    finally:
        _lib.use(None)
