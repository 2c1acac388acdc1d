"""ssdr_grid_subsample_batch_dev branch by branch against the per-cloud oracle (oracle.c().grid_subsampling(..., order="key")), bit for bit: points, features,
classes and the row count m.  The bucket partition (csrc/frontend.hip) and the batch half of the segmented sort (csrc/subsample.hip) each have branches that
the common input — 3 features, 1 label column, labels in [0,13), a workgroup per bucket, the library's stream — never takes; DESIGN.md section 18 lists them
with the case that reaches each.  Every case runs the same call under SSDR_SUBSAMPLE_AUTO and under SSDR_SUBSAMPLE_SORT, on the CPU logic build and on the
gfx950 build with the same inputs, and asserts its input condition with tests/_fe_paths.py: geometry (a float32 NumPy restatement of fe_params / fe_voxel
and of the greedy slicer) BEFORE the library is called: a case cannot pass without having reached the branch it names.

A status word other than 0 is part of what some cases expect: bit 2 = a grid the batch flavour cannot take (more than 65535 voxels along x, an origin that
rounds above the minimum, a NaN: partition path; a wrapped key: sort path), bit 4 = a bucket the partition path cannot reduce (a voxel above 1024 members, more
than 62 slices).  The other clouds of such a call must still equal the oracle.

The NaN case: what (long long) makes of a NaN is the platform's (x86: 2^63; gfx950: 0), so the reference's key of that point is too.  The case puts the NaN
in x and gives the point a (y, z) row of its own behind every other row: its key is then the largest under either conversion (and with the CPU build's 2^63
shifted out of the composite sort word), the row is the oracle's last row, and no other voxel depends on the conversion.  The status word of the sort path is
not asserted there (the CPU build reports the key that does not fit beside the index, the gfx950 build has nothing to report).

Labels drawn uniformly from [0,13) leave every label of a 600- or 900-member voxel far below 256 members, and the fast vote's byte counters would be right
without the exact vote; the crowded voxels of the [0,13) cases therefore give one label exactly 260 members (its byte shows 4: _fe_paths.wrapping_labels).

Measured on one MI355X: `pytest -m gpu tests/test_subsample_paths.py` = 26 tests in 1.3 s (2.6 s wall with the interpreter's start), slowest the child
process at 0.5 s. The CPU logic build's leg (`-m "not gpu"`, 26 tests): 87 s on 8 threads.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bits_equal
import _fe_paths as FP
from _fe_paths import AUTO, SORT, F32, FE_CAP, FE_CH, FE_SLICES, geometry, oracle_rows, run_batch, run_single

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, exp, what):
    assert len(got) == len(exp), what
    assert len(got[0]) == len(exp[0]), "%s: m = %d, oracle %d" % (what, len(got[0]), len(exp[0]))
    for k, (a, b) in enumerate(zip(got, exp)):
        assert_bits_equal(a, b, "%s array %d" % (what, k))


def _check(orc, clouds, dl, auto=0, auto_match=None, sort=0, sort_match=None, exp=None, stream=None):
    """the call under both methods -> the oracle's rows.  auto / sort: the status word the method must report (None: not asserted);
    *_match: the clouds whose rows must equal the oracle (default: all)"""
    exp = exp or [oracle_rows(orc, c, dl) for c in clouds]
    every = tuple(range(len(clouds)))
    for method, tag, want, which in ((AUTO, "auto", auto, auto_match), (SORT, "sort", sort, sort_match)):
        rc, st, rows = run_batch(clouds, dl, method, stream=stream)
        if want is not None:
            assert st == want and (rc != 0) == (want != 0), "%s: status %d (rc %d), expected %d" % (tag, st, rc, want)
        for r in (every if which is None else which):
            _same(rows[r], exp[r], "%s cloud %d" % (tag, r))
    return exp


# ---- 1. row layouts ---------------------------------------------------------------------------------------------------------------------------
LAYOUTS = [(3, 1),                                                      # the partition path's kernels for the hot path's rows: fe_scatter / fe_reduce / fe_move <3, 1>
           (0, 0), (1, 0), (0, 1), (4, 0), (0, 4), (1, 3), (2, 2),      # its generic kernels: <-1, -1>
           (3, 2),                                                      # 8 words: the packed reduction of the sort at its full width
           (6, 2), (0, 6)]                                              # above 8 words: gs_reduce_b (+ gs_reduce_labels_b), features NULL in the second


@pytest.mark.parametrize("fdim,ldim", LAYOUTS, ids=["f%d_l%d" % x for x in LAYOUTS])
def test_row_layouts(backend, orc, fdim, ldim):
    """Every row layout, NULL features / classes included, two clouds per call (one at negative coordinates)."""
    clouds, dl = FP.layout_clouds(fdim, ldim)
    _check(orc, clouds, dl)


# ---- 2. labels outside the fast vote, one-pass buckets ------------------------------------------------------------------------------------------
OUTSIDE = [(3, 1, (-5, 35)), (1, 3, (-5, 35)), (3, 1, (11, 17))]


@pytest.mark.parametrize("fdim,ldim,lab", OUTSIDE, ids=["f%d_l%d_lab%d_%d" % (f, l, a[0], a[1]) for f, l, a in OUTSIDE])
def test_labels_outside_fast_vote(backend, orc, fdim, ldim, lab):
    """Labels outside [0,13) in buckets read in one pass: L.slow is filled and fe_label_exact decides (the unordered_map emulation, its rehash at the 14th
    distinct label included); [11,17) mixes labels the byte counters hold with labels they do not."""
    clouds, dl = FP.outside_fast_vote_clouds(fdim, ldim, lab)
    _check(orc, clouds, dl)


# ---- 3. crowded voxels --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lab", [(0, 13), (-3, 20)], ids=["lab0_13", "lab-3_20"])
@pytest.mark.parametrize("shape", ["one_pass", "sliced"])
def test_crowded_voxels(backend, orc, shape, lab):
    """Voxels of 256 .. 1024 members (the packed byte counters wrap): in a bucket read in one pass, and in the later slices of a bucket cut into slices,
    where L.slow shares its storage with L.fill and nslow is reset per slice."""
    clouds, dl = FP.crowded_one_pass_clouds(lab) if shape == "one_pass" else FP.crowded_sliced_clouds(lab)
    _check(orc, clouds, dl)


# ---- 4. slice limit -----------------------------------------------------------------------------------------------------------------------------
def test_slice_limit(backend, orc):
    """One bucket of 512 voxels on either side of FE_SLICES = 62 slices, no voxel above FE_CAP: below, the oracle's rows; above, status bit 4, the other
    cloud of the call untouched, the sort the oracle's rows for both."""
    below, need, dl = FP.slice_limit_cloud(50000)
    assert need <= FE_SLICES, need
    _check(orc, [below], dl)
    above, need, dl = FP.slice_limit_cloud(60000)
    assert need > FE_SLICES, need
    other = FP.ordinary(np.random.default_rng(41))
    _check(orc, [above, other], dl, auto=4, auto_match=(1,))


# ---- 5. geometry edges ----------------------------------------------------------------------------------------------------------------------------
def _stretched(nx):
    """4000 points along x, the last voxel along x = nx - 1, 25 voxels along y: the 16-voxel-wide buckets (sx = 4)"""
    rng = np.random.default_rng(5000)
    p = rng.random((4000, 3)) * np.array([(nx - 1) * 0.04, 1.0, 0.3])
    p[0] = 0.0
    p[1] = ((nx - 1) * 0.04 + 0.02, 0.99, 0.29)
    p[2:600, 0] = (nx - 1) * 0.04 - rng.random(598) * 3.0            # (some rows with several voxels close to the far end)
    return FP.attach(rng, p.astype(F32))


def test_geometry_edge_widest_grid(backend, orc):
    """nx in [64000, 65535]: the widest grid the 16-bit row prefixes of `pre` take; status 0 on both paths."""
    rng = np.random.default_rng(51)
    edge, dl = _stretched(65535), 0.04
    g = geometry(edge[0], dl)
    assert g.fits and 64000 <= g.nx <= 65535 and g.inside.all(), g.nx
    _check(orc, [edge, FP.ordinary(rng)], dl)


def test_geometry_edge_grid_too_wide(backend, orc):
    """nx >= 65536 (the first such size: exactly 65536): the partition path reports bit 2 for that cloud, the sort takes it."""
    rng = np.random.default_rng(52)
    edge, dl = _stretched(65536), 0.04
    g = geometry(edge[0], dl)
    assert g.nx == 65536 and not g.fits, g.nx
    _check(orc, [edge, FP.ordinary(rng)], dl, auto=2, auto_match=(1,))


def test_geometry_edge_origin_above_minimum(backend, orc):
    """floor(min * (1 / dl)) * dl rounds above the minimum: the reference's size_t voxel index of that point wraps.  Both batch paths report bit 2 (the wrapped
    key does not fit beside the index in the sort word); ssdr_grid_subsample_dev, the documented way out, gives the oracle's rows in both orders."""
    rng = np.random.default_rng(53)
    dl = F32(0.06)
    edge = FP.make_cloud(rng, 800, (0.9, 0.9, 0.9), 0.1)
    edge[0][7] = (np.nextafter(F32(0.06), F32(0)), edge[0][:, 1].min(), edge[0][:, 2].min())
    g = geometry(edge[0], dl)
    assert g.min_vox[0] < 0 and not g.fits, g.min_vox
    # that point's voxel is (-1, 0, 0): its key is 2^64 - 1, which leaves no room for the index in the sort word
    assert (np.floor((edge[0][7] - g.org) / g.dl) == (-1, 0, 0)).all()
    clouds = [edge, FP.ordinary(rng)]
    _check(orc, clouds, dl, auto=2, auto_match=(1,), sort=2, sort_match=(1,))
    for order in ("reference", "key"):
        rc, st, got = run_single(edge, dl, order)
        assert rc == 0 and st == 0, (order, rc, st)
        _same(got, orc.grid_subsampling(edge[0], edge[1], edge[2], dl, order=order), "ssdr_grid_subsample_dev order %s" % order)
    # the same point in a higher (y, z) row: -1 + nx (iy + ny iz) wraps back to the key of the voxel at the END of the row in front, in the reference as in
    # the sort, which then has nothing to report and must give the oracle's rows; the partition path still refuses the cloud
    back = (edge[0].copy(), edge[1], edge[2])
    back[0][7, 1:] = (0.5, 0.5)
    g = geometry(back[0], dl)
    vox = np.floor((back[0][7] - g.org) / g.dl)
    assert g.min_vox[0] < 0 and not g.fits and vox[0] == -1 and vox[1] > 0 and vox[2] > 0
    _check(orc, [back, clouds[1]], dl, auto=2, auto_match=(1,))


def test_geometry_edge_nan(backend, orc):
    """One NaN coordinate: the partition path reports bit 2 (the point lies in no voxel), the sort keeps the point as a row of its own, as the oracle does."""
    rng = np.random.default_rng(54)
    dl = 0.04
    edge = FP.make_cloud(rng, 800, (1.0, 1.0, 1.0))
    edge[0][400] = (np.nan, 1.5, 1.5)
    g = geometry(edge[0], dl)
    assert g.fits and not g.inside[400] and g.inside.sum() == 799
    # input condition (module docstring): the NaN point's (y, z) row is the last one and holds no other point
    yz = np.floor((edge[0][:, 1:] - g.org[1:]) / g.dl)
    assert (yz[400] == (g.ny - 1, g.nz - 1)).all() and not (np.delete(yz, 400, axis=0) == yz[400]).all(axis=1).any()
    exp = _check(orc, [edge, FP.ordinary(rng)], dl, auto=2, auto_match=(1,), sort=None)
    assert np.isnan(exp[0][0][-1, 0]) and len(exp[0][0]) == len(g.vox_key) + 1          # the oracle keeps the NaN row


# ---- 6. state reuse and the caller's stream -------------------------------------------------------------------------------------------------------
def _calls():
    rng = np.random.default_rng(60)
    a = [FP.make_cloud(rng, 40000, (6.0, 5.0, 3.0)), FP.make_cloud(rng, 3000, (2.0, 2.0, 1.0), -1.0)]
    b = [FP.make_cloud(rng, 200, (0.5, 0.5, 0.5), fdim=1, ldim=1)]
    bad = [FP.make_cloud(rng, 1100, (0.01, 0.01, 0.01), 0.5), FP.make_cloud(rng, 300, (1.0, 1.0, 1.0))]
    assert len(a[0][0]) > FE_CH                                             # two count chunks: cntm's stride (chunks_max) differs between the calls
    assert geometry(bad[0][0], 0.04).vox_members.max() > FE_CAP
    return a, b, bad


def _sequence(orc, stream, with_bad):
    a, b, bad = _calls()
    dl = 0.04
    exp_a, exp_b = [oracle_rows(orc, c, dl) for c in a], [oracle_rows(orc, c, dl) for c in b]
    for method in (AUTO, SORT):
        rc, st, first = run_batch(a, dl, method, stream=stream)
        assert (rc, st) == (0, 0)
        rc, st, got_b = run_batch(b, dl, method, stream=stream)
        assert (rc, st) == (0, 0)
        if with_bad:
            rc, st, _ = run_batch(bad, dl, AUTO, stream=stream)
            assert rc != 0 and st == 4
        rc, st, second = run_batch(a, dl, method, stream=stream)
        assert (rc, st) == (0, 0), "the status of an earlier call is still reported"
        for r in range(len(a)):
            _same(first[r], exp_a[r], "call A, cloud %d" % r)
            _same(second[r], exp_a[r], "call A again, cloud %d" % r)
            _same(second[r], first[r], "call A against its repetition, cloud %d" % r)
        _same(got_b[0], exp_b[0], "call B")


def test_state_reuse_on_the_library_stream(backend, orc):
    """Calls of different shape on one stream: A (two count chunks, layout (3, 1)), B (200 points, layout (1, 1)), a call that reports status 4, A again —
    the per-stream tables (cntm by chunks_max, lrc / nocc / trow) carry nothing from one call into the next."""
    _sequence(orc, None, True)


def test_state_reuse_on_a_callers_stream(backend, orc):
    """A -> B -> A on a stream of the caller's: copies, call and status all ordered on that stream alone."""
    from ssdr_al import _lib
    L = _lib.lib()
    s = C.c_void_p()
    _lib.check(L.ssdr_stream_create(C.byref(s)))
    try:
        _sequence(orc, s.value, False)
    finally:
        _lib.check(L.ssdr_stream_destroy(s.value))


# ---- 7. the environment-selected forms, one child process per environment ---------------------------------------------------------------------------
FORM_ENVS = [("one_wg_per_cu", {"SSDR_FE_WGS": "1", "SSDR_FE_MOVE_WGS": "1"}, "many")]


@pytest.mark.parametrize("name,env_add,group", FORM_ENVS, ids=[e[0] for e in FORM_ENVS])
def test_environment_selected_forms(backend, name, env_add, group):
    """SSDR_FE_WGS=1 SSDR_FE_MOVE_WGS=1: one workgroup per CU, so every workgroup of fe_reduce takes more than ten items one after another (and every wave of fe_move
    several): the LDS state is reset between items, also behind an item that set L.bad.  The switches are read once per process: a child process each, never two at
    a time, no retry; every printed line is asserted."""
    from ssdr_al import _lib
    env = {k: v for k, v in os.environ.items() if k not in FP.FORM_ENV_NAMES}
    env.update(env_add)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_fe_forms_worker.py"), _lib.lib_path(), group], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    want = FP.form_names(group)
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("CASE ")]
    assert [ln[1] for ln in lines] == list(want), r.stdout
    for _, case, rc, st, match in lines:
        assert int(st) == want[case] and (int(rc) != 0) == (want[case] != 0), "%s %s: rc %s status %s, expected status %d\n%s" % (name, case, rc, st, want[case], r.stdout)
        assert int(match) == 1, "%s %s: the rows differ from the oracle\n%s" % (name, case, r.stdout)
