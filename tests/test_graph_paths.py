"""The selection graph branch by branch: ssdr_cloud_graph_dev / ssdr_cloud_graph_batch_dev / ssdr_propagate_dev / ssdr_propagate_batch_dev (csrc/select.hip,
csrc/select_chamfer.hip) against plain NumPy in float64.  DESIGN.md section 19 lists every branch with the case that reaches it.  What the older tests
(test_select.py, test_select_oracle.py, test_region_selectors.py) leave open and this file closes:

  * every value check is on the DIRECTED matrix dir[i][j] (mean over the points of i of the distance to the nearest point of j), never on dir + dir.T: a
    writer that stores to dir[j][i] is caught;
  * the pruned two-pass walk over targets beyond CH_TILE points runs with pass 0 empty (hollow shapes), with pass 0 settling the sources (a floor), with the
    nearest point in pass 1 although pass 0 was not empty, and with an empty first chunk in the compaction;
  * the batched launches are compared with the per-cloud calls bit for bit, large targets, empty superpoints, gcn_top and the float32 flavour included, above
    PACK_MAX superpoints and above the batched grid's 1024 workgroups, and under SSDR_CHAMFER_SLICES = 1 and 32;
  * the keep-top mask on exact ties and beyond TOPK_ROW columns, the propagation around its unroll by eight.

Every case runs on the CPU logic build and on the gfx950 build with the same inputs, and asserts its input condition with tests/_graph_paths.py: plan (a NumPy
restatement of the packer and of the kernels' branch conditions) BEFORE the library is called.  The tolerances are those of tests/test_select.py: the float64
oracle at rtol 1e-12 / atol 1e-14 (times the coordinate scale), the screening against SSDR_CHAMFER_F64=1 bit for bit, the float32 flavour at rtol 2e-6, a batched
block against the per-cloud call bit for bit, centres against select_np.bbox_centres bit for bit.

The CPU logic build emulates the matrix instruction, the lane swap and the ballots; the inline assembly (v_mul_u32_u24, v_min_f64, v_and_or_b32), the real
v_mfma_f32_32x32x16_f16 / v_permlane32_swap and the concurrency of workgroups exist on the gfx950 leg alone.  Two cases run there only, because the CPU build
needs minutes for them: the batch above PACK_MAX superpoints and the keep-top rows beyond TOPK_ROW columns.

Measured on one MI355X: `pytest -m gpu tests/test_graph_paths.py` = 20 tests in 3.2 - 4.2 s, slowest the two child processes (0.4 - 0.8 s each) and the five-cloud batch (0.4 s).
The CPU logic build's leg (`-m "not gpu"`, 19 tests and one skip): 19 s.
"""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bits_equal
from oracle import select_np as O
import _graph_paths as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = G.constants()
RTOL, ATOL = 1e-12, 1e-14


def _both_forms(monkeypatch, call):
    """call() under the screening on the matrix cores and under SSDR_CHAMFER_F64=1 (read per launch)"""
    monkeypatch.delenv("SSDR_CHAMFER_F64", raising=False)
    screened = call()
    monkeypatch.setenv("SSDR_CHAMFER_F64", "1")
    try:
        plain = call()
    finally:
        monkeypatch.delenv("SSDR_CHAMFER_F64")
    return screened, plain


def _close(got, want, what, scale=1.0):
    bad = ~np.isclose(got, want, rtol=RTOL, atol=ATOL * scale)
    assert not bad.any(), "%s: %d entries off the oracle, first at %s: %r vs %r" % (what, bad.sum(), np.argwhere(bad)[0], got[bad][0], want[bad][0])


def _described(cloud):
    """-> centres (oracle), centred points, plan, (dir oracle, nearest indices)"""
    xyz, off, pts = cloud
    cen = G.bbox_centres(xyz, off, pts)
    al = G.centred(xyz, off, pts, cen)
    return cen, al, G.plan(np.diff(off), al), G.dir_oracle(xyz, off, pts, cen)


def _check_forms(monkeypatch, cloud, cen, want, what, scale=1.0, exact=True):
    (c0, d0, _), (c1, d1, _) = _both_forms(monkeypatch, lambda: G.graph_single(cloud))
    assert_bits_equal(c0, cen, what + ": centres"); assert_bits_equal(c1, cen, what + ": centres, float64 form")
    _close(d0, want, what + ", screening form", scale); _close(d1, want, what + ", float64 form", scale)
    if exact: assert_bits_equal(d0, d1, what + ": screening against SSDR_CHAMFER_F64=1")
    else: assert np.allclose(d0, d1, rtol=4e-16, atol=0), what
    return d0


# ---- 1. small sizes -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _small_sizes():
    rng = np.random.default_rng(101)
    sizes = [1, 2, 3, 5, K.SEQ_MAX, K.SEQ_MAX + 1, 29, 31, 32, 33, 63, 64, 65, K.ITEM - 1, K.ITEM, K.ITEM + 1, 2 * K.ITEM, 2 * K.ITEM + 1, K.CH_TILE, 5, 29, K.ITEM + 1]
    cloud = G.make_cloud(rng, [G.blob(rng, s, rng.random(3) * np.array([6, 5, 2.5]) + 20.0, 0.1) for s in sizes])
    return sizes, cloud, _described(cloud)


def test_directed_matrix_small_sizes(backend, monkeypatch):
    """Targets of 1 .. CH_TILE points on both sides of a tile of 32, of SEQ_MAX (one lane's sum | the wave's), of ITEM (an item | passes of ITEM, the last one
    partly live), the full set and a shuffled subset as `sel`, both forms.  The winning run of a target of 5 or 29 points whose LAST point is nearest holds
    that point alone: the rest of the run is clipped to nj - 1."""
    sizes, cloud, (cen, al, P, (want, nn)) = _small_sizes()
    n = len(sizes)
    assert all((P.item_of[i] < 0) == (sizes[i] > K.ITEM) for i in range(n)) and max(len(m) for m in P.items) > 3
    assert all(P.branch(i, j) == "mf" for i in range(n) for j in range(n) if i != j)
    for j in (sizes.index(5), sizes.index(29)):
        assert (sizes[j] - 1) % 4 == 0 and any((nn[i, j] == sizes[j] - 1).any() for i in range(n) if i != j), "no source has the last point of target %d nearest" % j
    full = _check_forms(monkeypatch, cloud, cen, want, "all superpoints")
    sel = np.random.default_rng(102).permutation(n)[:13]
    (c0, d0, _), (c1, d1, _) = _both_forms(monkeypatch, lambda: G.graph_single(cloud, sel))
    assert_bits_equal(c0, cen[sel], "centres of sel")
    assert_bits_equal(d0, full[np.ix_(sel, sel)], "sel against the block of the full matrix"); assert_bits_equal(d1, d0, "sel, float64 form")


# ---- 2. targets beyond the staging limit: the two-pass walk ---------------------------------------------------------------------------------------------
def _walk_case(shape):
    """-> [(cloud, large targets, check(P, al, nn, sizes))]"""
    rng = np.random.default_rng({"hollow": 201, "core_late": 202, "outer_wins": 203, "slab": 204, "both_large": 205}[shape])
    T = K.CH_TILE
    if shape == "hollow":
        def check(P, al, nn, sizes, j):
            assert P.pass0_surely_empty(j) and P.pass0_surely_empty(j, large=True)
        return [(G.make_cloud(rng, [G.ring(rng, m, (9, 9, 1), 2.5)] + G.small_sources(rng)), [0], check) for m in (T + 1, 2 * T + 1)]
    if shape == "core_late":
        def check(P, al, nn, sizes, j):
            out = (1 + 1e-9) * (P.Rs + G.PASS_MARGIN)
            assert (P.norm[j][:T] > out).all() and (P.norm[j][T:] <= 0.2).any() and P.chunks(j) == 3       # pass 0: nothing in the first chunk, something later
            items = [m for m in P.items if j not in m]
            settled = [all(P.surely_settled(i, j, nn) for i in m) for m in items]
            unsettled = [P.surely_unsettled(m, j, nn) for m in items]
            assert any(settled) and any(unsettled)
            for m, s in zip(items, settled):          # ... and whoever goes on to pass 1 still has its nearest point in the core
                assert s or all((P.norm[j][nn[i, j]] <= G.PASS_MARGIN).all() for i in m)
        return [(G.make_cloud(rng, [G.ring_with_core(rng, 1400, (9, 9, 1), 2.5, 60, T + 10)] + G.small_sources(rng, flat=0.1)), [0], check)]
    if shape == "outer_wins":
        def check(P, al, nn, sizes, j):
            i = len(sizes) - 1                         # the pole: its tips are 1 m from the ring and 1.5 m from the core
            assert sizes[i] <= K.ITEM and P.nearest_in_pass1(i, j, nn) and (P.norm[j][nn[i, j]] <= G.PASS_MARGIN).any()
        return [(G.make_cloud(rng, [G.ring_with_core(rng, T + 60, (9, 9, 1), 2.5, 20, 50)] + G.small_sources(rng) + [G.pole(rng, 60, (4, 4, 1), 3.0)]), [0], check)]
    if shape == "slab":
        def check(P, al, nn, sizes, j):
            assert P.chunks(j) == 4 and sizes[j] - 3 * T == 1
            assert all(P.surely_settled(i, j, nn) for i in range(len(sizes)) if 0 < sizes[i] <= K.ITEM)
        return [(G.make_cloud(rng, G.small_sources(rng, flat=0.1)[:5] + [G.slab(rng, 3 * T + 1, (9, 9, 0), 6.0, 5.0)] + G.small_sources(rng, flat=0.1)[5:]), [5], check)]
    if shape == "both_large":
        def check(P, al, nn, sizes, j):
            big = [i for i in range(len(sizes)) if sizes[i] > K.ITEM]
            assert len(big) == 5 and sum(sizes[i] > T for i in big) == 2       # two rounds of four waves: the target itself (i == j) in the first, three idle waves in the second
        src = G.small_sources(rng)
        return [(G.make_cloud(rng, [G.ring(rng, T + 60, (9, 9, 1), 2.5)] + src[:9] + [G.slab(rng, 2 * T + 20, (15, 3, 0), 4.0, 3.0)] + src[9:] + [G.blob(rng, K.ITEM + 1, (1, 1, 1))]), [0, 10], check)]
    raise ValueError(shape)


@functools.lru_cache(None)
def _walk_inputs(shape):
    return [(cloud, targets, check, _described(cloud)) for cloud, targets, check in _walk_case(shape)]


@pytest.mark.parametrize("shape", ["hollow", "core_late", "outer_wins", "slab", "both_large"])
def test_large_targets_two_pass_walk(backend, monkeypatch, shape):
    """chamfer_big_targets: pass 0 takes the target's points within R1 = (largest |a| of the workgroup's sources) + 0.25 m, pass 1 the others, only for waves the
    first pass did not settle.  hollow: pass 0 stages nothing, every distance comes from pass 1.  core_late: the first chunk of pass 0 is empty, a later
    one is not (the compaction restarts per chunk); some waves are settled, the others find their nearest point in the core all the same.  outer_wins: pass 0 is
    not empty and yet the nearest point lies in pass 1.  slab: four chunks, the last of ONE point, every small source settled (pass 1 never runs).
    both_large: two large targets, each a large source of the other (the lockstep loop: a wave whose source is the target itself, idle waves)."""
    for cloud, targets, check, (cen, al, P, (want, nn)) in _walk_inputs(shape):
        sizes = [int(s) for s in np.diff(cloud[1])]
        for j in targets:
            assert sizes[j] > K.CH_TILE and all(P.branch(i, j) == "big" for i in range(len(sizes)) if i != j)
            check(P, al, nn, sizes, j)
        assert sum(s > K.ITEM for s in sizes) >= 2 + len(targets) and min(sizes) == 1 and P.Rs <= 1.5 + 1e-6
        G.prime_pack(len(sizes))
        _check_forms(monkeypatch, cloud, cen, want, shape)


# ---- 3. screening ranges mixed in one cloud ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _range_mix():
    rng = np.random.default_rng(301)
    seat = lambda: rng.random(3) * np.array([6, 5, 2.5]) + 10.0
    shapes = [G.blob(rng, 5, seat()), G.blob(rng, 40, seat()), G.blob(rng, 130, seat()), G.blob(rng, 64, seat()),
              G.pole(rng, 5, seat(), 70.0, axis=1),              # 4: out of range, shares item 0 with the four in front
              G.pole(rng, 100, seat(), 62.0),                    # 5: |p|^2 = 961: just inside
              (np.array([3.0, 2.0, 1.0]) + rng.normal(0, 0.12, (40, 3))) * 1e-3,      # 6: a few tenths of a millimetre across
              G.pole(rng, K.ITEM + 44, seat(), 70.0, axis=2),    # 7: out of range, pair by pair
              G.blob(rng, K.ITEM + 1, seat(), 0.1), G.blob(rng, 33, seat())]
    cloud = G.make_cloud(rng, shapes)
    return cloud, _described(cloud)


def test_screening_range_mixes(backend, monkeypatch):
    """MF_R2_MAX decides per (item | pair-by-pair source, target): in-range sources against an out-of-range target and the reverse stream the target from global
    memory inside the screening kernel; an item whose r2item one 5-point member raises out of range takes its in-range members along; 961 m^2 is screened with
    a wide threshold; the millimetre-scale superpoint's pieces are half-precision subnormals.  The values do not depend on any of it."""
    cloud, (cen, al, P, (want, nn)) = _range_mix()
    R = K.MF_R2_MAX
    assert P.item_of[4] == P.item_of[0] == P.item_of[3] and P.r2sp[4] > R and P.r2item[P.item_of[4]] > R and all(P.r2sp[i] <= R for i in (0, 1, 2, 3))
    assert 900.0 < P.r2sp[5] <= R and P.item_of[5] != P.item_of[4] and P.r2item[P.item_of[5]] <= R and P.r2sp[7] > R and P.item_of[7] < 0 and P.radius[6] < 1e-3
    assert P.item_of[9] not in (P.item_of[4], -1) and P.item_of[6] != P.item_of[4]
    want_branch = {(9, 7): "stream", (9, 4): "stream", (7, 9): "stream", (0, 9): "stream", (3, 1): "stream", (4, 9): "stream", (7, 4): "stream",
                   (9, 5): "mf", (5, 9): "mf", (5, 6): "mf", (6, 5): "mf", (8, 5): "mf", (8, 7): "stream", (9, 8): "mf", (6, 9): "mf"}
    for (i, j), b in want_branch.items():
        assert P.branch(i, j) == b, (i, j, P.branch(i, j))
    _check_forms(monkeypatch, cloud, cen, want, "mixed ranges", scale=70.0)


# ---- 4. sources the screening cannot decide ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _swept():
    rng = np.random.default_rng(401)
    seat = lambda: rng.random(3) * np.array([6, 5, 2.5]) + 5.0
    shapes = [G.twice(G.blob(rng, 20, seat())), G.twice(G.blob(rng, 150, seat(), 0.15)), G.twice(G.blob(rng, K.CH_TILE // 2, seat(), 0.2)),
              G.blob(rng, 5, seat()), G.blob(rng, 40, seat()), G.blob(rng, 100, seat()), G.blob(rng, K.ITEM + 44, seat(), 0.15)]
    cloud = G.make_cloud(rng, shapes)
    return cloud, _described(cloud)


@functools.lru_cache(None)
def _lattices():
    rng = np.random.default_rng(402)
    cloud = G.make_cloud(rng, [G.lattice(rng, s, rng.random(3) * np.array([6, 5, 2.5]) + 5.0) for s in (40, 130, 300, 33, K.CH_TILE)])
    return cloud, _described(cloud)


def test_undecided_sources_are_swept(backend, monkeypatch):
    """Targets of 40, 300 and CH_TILE points that list every point twice, the copies in different runs of four: the two runs' minima tie exactly, no source is
    decided, every one is swept over the whole target in float64 — item sources and the passes of a pair-by-pair source (the last pass partly live)."""
    cloud, (cen, al, P, (want, nn)) = _swept()
    sizes = P.sizes
    assert sizes[:3] == [40, 300, K.CH_TILE] and all(P.surely_swept(j) for j in range(3)) and not any(P.surely_swept(j) for j in range(3, 7))
    assert all(P.branch(i, j) == "mf" for j in range(3) for i in range(7) if i != j)
    assert [P.item_of[i] >= 0 for i in range(7)] == [True, False, False, True, True, True, False] and sizes[6] % K.ITEM != 0
    _check_forms(monkeypatch, cloud, cen, want, "duplicated targets")
    # a lattice: equally near target points at DIFFERENT offsets, so the two forms may name different ones and agree within the last ulps only
    cloud, (cen, al, P, (want, nn)) = _lattices()
    d = al[1][:, None, :] - al[2][None, :, :]
    d2 = (d * d).sum(-1)
    assert ((d2 == d2.min(1, keepdims=True)).sum(1) > 1).any() and all(P.branch(i, j) == "mf" for i in range(P.n) for j in range(P.n) if i != j)
    _check_forms(monkeypatch, cloud, cen, want, "lattices", exact=False)


# ---- 5. the batched launches ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _batch_oracles(mode):
    out = []
    for (xyz, off, pts), sel in G.batch_clouds():
        so, sp = (off, pts) if sel is None else G.sub_csr(off, pts, sel)
        cen = G.bbox_centres(xyz, so, sp)
        out.append((cen, G.dir_oracle(xyz, so, sp, cen)[0] if mode == "f64" else G.dir_oracle_f32(xyz, so, sp, cen)))
    return out


def _assert_batch_inputs(clouds):
    sizes = [np.diff(c[1]) if sel is None else np.diff(c[1])[sel] for c, sel in clouds]
    assert [len(s) for s in sizes[1:4]] == [1, 2, 74] and (sizes[0] == 0).sum() == 2 and (sizes[0] > K.CH_TILE).sum() == 3 and (sizes[4] > K.ITEM).any()
    assert (sizes[0] > K.C32_SLAB).any() and set(sizes[4]) <= set(sizes[0]) and len(sizes[4]) < len(sizes[0])
    plans = []
    for s, ((xyz, off, pts), sel) in zip(sizes, clouds):
        so, sp = (off, pts) if sel is None else G.sub_csr(off, pts, sel)
        plans.append(G.plan(s, G.centred(xyz, so, sp, G.bbox_centres(xyz, so, sp))))
    # item 0 of the first cloud lies beyond the screening's range (its members take the float64 loop over global memory), item 0 of every other cloud inside it
    assert plans[0].r2item[0] > K.MF_R2_MAX and all(len(p.r2item) and p.r2item[0] <= K.MF_R2_MAX for p in plans[1:]) and len(plans[3].r2item) > len(plans[0].r2item)


@pytest.mark.parametrize("f64_env", ["screened", "env_f64"])
@pytest.mark.parametrize("mode", ["f64", "f32_cuda"])
def test_batch_equals_single_and_oracle(backend, monkeypatch, mode, f64_env):
    """Five clouds in ONE ssdr_cloud_graph_batch_dev call with gcn_top = 3 (hollow and both-large targets with empty superpoints | one superpoint | two | 74 of
    mixed sizes | superpoints of the first cloud again in another order): every block's centres, dir and adj equal ssdr_cloud_graph_dev on that cloud alone
    bit for bit (pack_at's offsets, coff / boff, blockIdx.z), and dir equals the oracle of the mode."""
    clouds = G.batch_clouds()
    _assert_batch_inputs(clouds)
    if f64_env == "env_f64": monkeypatch.setenv("SSDR_CHAMFER_F64", "1")
    else: monkeypatch.delenv("SSDR_CHAMFER_F64", raising=False)
    G.set_chamfer_mode(mode)
    try:
        got = G.graph_batch(clouds, gcn_top=3)
        alone = [G.graph_single(c, sel, gcn_top=3) for c, sel in clouds]
    finally:
        G.set_chamfer_mode("f64")
    for b, ((cen, want), g, a) in enumerate(zip(_batch_oracles(mode), got, alone)):
        for k, what in enumerate(("centres", "dir", "adj")):
            assert_bits_equal(g[k], a[k], "cloud %d: batched %s against the per-cloud call" % (b, what))
        assert_bits_equal(g[0], cen, "cloud %d: centres" % b)
        if mode == "f64": _close(g[1], want, "cloud %d" % b)
        else: assert np.allclose(g[1], want, rtol=2e-6, atol=0), "cloud %d: float32 flavour" % b
        assert np.isfinite(g[2]).all()
    assert got[1][2].tolist() == [[1.0]]            # one superpoint: rowsum = 0, 1 / 0 = inf becomes 0, plus I


# ---- 6. a batch above the packer's and the grid's caps (gfx950 leg only) ------------------------------------------------------------------------------------
def test_batch_above_the_caps(backend, monkeypatch):
    """4097 superpoints of one to three points in a batched call (above PACK_MAX: every superpoint pair by pair; above the batched grid's 1024 workgroups: four or
    five targets per workgroup) and a small cloud behind it (pack_at offsets of 4097 rows): a 70-superpoint sub-block equals the packed per-cloud computation
    over those superpoints bit for bit and the oracle; the small cloud equals its own call."""
    if backend == "emu":
        pytest.skip("the CPU logic build needs minutes for 4097 x 4097 pairs of superpoints: gfx950 leg only")
    monkeypatch.delenv("SSDR_CHAMFER_F64", raising=False)
    rng = np.random.default_rng(601)
    n = K.PACK_MAX + 1
    assert n > 4 * 1024
    sizes = rng.integers(1, 4, n)
    big = G.make_cloud(rng, [G.blob(rng, s, rng.random(3) * np.array([20, 15, 3]), 0.1) for s in sizes])
    small = G.make_cloud(rng, [G.blob(rng, s, rng.random(3) * 3.0) for s in (5, K.ITEM + 1, 40, 17, 1)])
    assert G.plan(sizes, [np.zeros((s, 3)) for s in sizes]).big == list(range(n))
    got = G.graph_batch([(big, None), (small, None)])
    sub = np.sort(rng.choice(n, 70, replace=False))
    c, d, _ = G.graph_single(big, sub)
    assert_bits_equal(got[0][0][sub], c, "centres of the sub-block"); assert_bits_equal(got[0][1][np.ix_(sub, sub)], d, "sub-block against the packed computation")
    so, sp = G.sub_csr(big[1], big[2], sub)
    cen = G.bbox_centres(big[0], so, sp)
    assert_bits_equal(c, cen, "centres")
    _close(d, G.dir_oracle(big[0], so, sp, cen)[0], "sub-block")
    alone = G.graph_single(small)
    for k in range(3):
        assert_bits_equal(got[1][k], alone[k], "the small cloud behind, array %d" % k)
    _close(alone[1], G.dir_oracle(*small, G.bbox_centres(*small))[0], "small cloud")


# ---- 7. SSDR_CHAMFER_SLICES, a child process per value ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slices", ["1", "32"])
def test_slices_switch(backend, monkeypatch, slices):
    """SSDR_CHAMFER_SLICES (read once per process) sets gridDim.y of the batched launch: which items a workgroup's waves take changes, no value may.  The batch
    of test_batch_equals_single_and_oracle in a child process per value, one at a time; its digest of dir equals this process's."""
    from ssdr_al import _lib
    monkeypatch.delenv("SSDR_CHAMFER_F64", raising=False)
    G.set_chamfer_mode("f64")
    here = hashlib.sha256(b"".join(np.ascontiguousarray(g[1]).tobytes() for g in G.graph_batch(G.batch_clouds(), gcn_top=3))).hexdigest()
    env = {k: v for k, v in os.environ.items() if k not in ("SSDR_CHAMFER_SLICES", "SSDR_CHAMFER_F64")}
    env["SSDR_CHAMFER_SLICES"] = slices
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_graph_forms_worker.py"), _lib.lib_path()], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith(("CASE ", "DIGEST "))]
    assert lines == [["DIGEST", "batch", here], ["CASE", "batch", "ok"]], (here, r.stdout)


# ---- 8. the keep-top mask ---------------------------------------------------------------------------------------------------------------------------------
def _topk_cloud(n):
    rng = np.random.default_rng(800 + n)
    return G.make_cloud(rng, [G.blob(rng, int(s), rng.random(3) * np.array([4, 3, 2])) for s in rng.integers(1, 20, n)])


def _tie_cloud():
    """27 copies of one 8-point shape on a 3 x 3 x 3 lattice of seats, every coordinate a multiple of 1/8: equal centre distances and equal chamfer terms"""
    rng = np.random.default_rng(827)
    shape = rng.integers(-2, 3, (8, 3)) / 8.0
    seats = np.stack(np.meshgrid(*[np.arange(3.0)] * 3, indexing="ij"), -1).reshape(-1, 3) + 4.0
    return G.make_cloud(rng, [s + shape for s in seats])


def _masked_equals_keep_top(cloud, tops, what):
    plain = G.graph_single(cloud)[2]
    for top in tops:
        masked = G.graph_single(cloud, gcn_top=top)[2]
        assert_bits_equal(masked, O.keep_top(plain, top), "%s, gcn_top %d" % (what, top))
        assert (masked >= 0).all()
    return plain


def test_topk_mask(backend, monkeypatch):
    """adj under gcn_top = 1, 2, n - 1, n, n + 5 equals select_np.keep_top of the device's OWN unmasked adj bit for bit (so no float noise enters), on random
    clouds of 2, 9 and 130 superpoints and on a lattice of identical superpoints whose rows hold exactly equal entries ACROSS the cut (the higher column is
    kept).  gfx950 leg only (the CPU build needs minutes): TOPK_ROW + 1 columns, ranked in place in global memory, single and batched; no -v - 4 marker stays."""
    monkeypatch.delenv("SSDR_CHAMFER_F64", raising=False)
    for n in (2, 9, 130):
        _masked_equals_keep_top(_topk_cloud(n), (1, 2, n - 1, n, n + 5), "%d superpoints" % n)
    tie, tops = _tie_cloud(), (1, 2, 3, 6, 13, 26)
    plain = G.graph_single(tie)[2]
    srt = np.sort(plain, axis=1)
    cut_ties = sum(int((srt[:, -t] == srt[:, -t - 1]).sum()) for t in tops)
    assert cut_ties > 0, "no row of the lattice cloud has equal entries on both sides of a cut"
    _masked_equals_keep_top(tie, tops, "lattice of identical superpoints")
    if backend == "emu":
        return
    n = K.TOPK_ROW + 1
    rng = np.random.default_rng(803)
    wide = G.make_cloud(rng, list((rng.random((n, 3)) * np.array([3, 3, 1]))[:, None, :]))
    plain = _masked_equals_keep_top(wide, (100,), "%d one-point superpoints" % n)
    want = O.keep_top(plain, 100)
    small = _topk_cloud(130)
    got = G.graph_batch([(small, None), (wide, None)], gcn_top=100)
    assert_bits_equal(got[1][2], want, "batched, %d columns" % n); assert (got[1][2] >= 0).all()
    assert_bits_equal(got[0][2], O.keep_top(G.graph_single(small)[2], 100), "batched, the small cloud in front")


# ---- 9. propagation ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gcn_number", [1, 3])
@pytest.mark.parametrize("D", [1, 32])
def test_propagation(backend, D, gcn_number):
    """comb = sum_h A^h V hop by hop through ssdr_propagate_dev and ssdr_propagate_batch_dev against select_np.propagate: blocks of 1, 7, 8, 9 and 74 rows (the
    loop over j is unrolled by eight, its tail guarded), D = 1 and 32, rows scattered over a larger table whose other rows must come back untouched."""
    rng = np.random.default_rng(900 + D)
    ns = [1, 7, 8, 9, 74]
    T = sum(ns) + 13
    perm = rng.permutation(T)
    rows, o = [], 0
    for n in ns:
        rows.append(perm[o:o + n]); o += n
    outside = perm[o:]
    adjs = [rng.random((n, n)) * (2.0 / n) for n in ns]
    V = rng.random((T, D)) + 0.5
    want = O.propagate(adjs, rows, V, gcn_number)
    res = {}
    for batched in (False, True):
        comb, last = G.propagate_hops(adjs, rows, V, gcn_number, batched)
        assert np.allclose(comb, want, rtol=1e-12, atol=0), "batched" if batched else "single"
        assert_bits_equal(comb[outside], V[outside], "comb rows outside the clouds")
        assert (last[outside] == -7.5).all(), "a hop wrote a row outside the clouds"
        res[batched] = (comb, last)
    assert_bits_equal(res[True][0], res[False][0], "comb: batched against single"); assert_bits_equal(res[True][1], res[False][1], "last hop: batched against single")
