"""Room plans that hold the rooms' records (csrc/frontend.hip: FePlan::rec; include/ssdr_al.h: ssdr_rooms_plan_info).  Such a plan runs the every-bucket scatter once,
at build; a planned call launches no scatter, its voxel reduction reads the plan's records and writes its rows to the per-stream rows region.  The planned call must
still be ssdr_tile_from_rooms_batch_dev on the same inputs BIT FOR BIT: the tiles, the sub-sampled rows and their counts, the status word and both stats calls —
`scattered` included, which for such a call is "records the stages were given" and is counted by fe_tile_order / fe_tile_plan<2> instead of by a scatter.  The
unplanned call is the reference (tests/test_frontend_room_plan.py: _Set, _same).  Every case asserts its input condition with tests/_fe_paths.py: geometry before the
library is called, runs on the CPU logic build and on the gfx950 build, and looks at the profiler's sites: no "fe_scatter" where the records are the plan's.

Rooms are 5 k to 60 k raw points (the rooms of test_frontend_room_plan.test_stage_two_and_stage_three_with_padding, which case 2 takes over, hold up to 200 k), tiles
1024 rows, dl 0.04."""
import ctypes as C

import numpy as np
import pytest

import _fe_paths as FP
from _fe_paths import F32, FE_CAP, geometry
from test_frontend_room_plan import KEYS, N, _Set, _few_voxels_many_points, _room_g, _same, _three_rooms
from test_frontend_tile_prune import DL, FE_TO_NMAX, _box, _room, _short_estimate_room

CEN3 = [(2.0, 1.5, 1.25), (11.5, -2.7, 2.0), (-4.0, 0.7, 0.5)]          # inside each of _three_rooms


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    """the switches are read at every plan creation: every case starts from the defaults"""
    for k in ("SSDR_FE_PLAN_RECORDS", "SSDR_FE_PLAN_RECORDS_MAX_MB"):
        monkeypatch.delenv(k, raising=False)


def _info(S, plan):
    """ssdr_rooms_plan_info -> (record_bytes, sorted)"""
    from ssdr_al import _lib
    rb, so = C.c_int64(-1), C.c_int32(-1)
    _lib.check(S.L.ssdr_rooms_plan_info(plan, C.byref(rb), C.byref(so)))
    return rb.value, so.value


def _with_sites(S, fn):
    """fn() under ssdr_prof_enable -> (its result, the names of the profiler sites it passed)"""
    L = S.L
    L.ssdr_prof_report()
    L.ssdr_prof_enable(1)
    try:
        out = fn()
        names = {ln.rsplit(" ", 4)[0] for ln in L.ssdr_prof_report().decode().splitlines() if ln.strip()}
    finally:
        L.ssdr_prof_enable(0)
    return out, names


def _pair(S, cen, plan, what, records=True, stream=None):
    """planned call and unplanned call over the same centres, compared on every key; the planned call scatters exactly when the plan holds no records"""
    got, s_got = _with_sites(S, lambda: S.call(cen, plan, stream))
    ref, s_ref = _with_sites(S, lambda: S.call(cen, None, stream))
    assert "fe_reduce" in s_got and "fe_reduce" in s_ref and "fe_scatter" in s_ref, (s_got, s_ref)
    assert ("fe_scatter" in s_got) == (not records), "%s: sites of the planned call %s" % (what, sorted(s_got))
    _same(got, ref, what)
    return got, ref


def _ordinary(rooms):
    """input condition of a room that takes the common route: a grid the partition takes, every point inside it, several non-empty buckets, no crowded voxel"""
    for p, _, _ in rooms:
        g = geometry(p, DL)
        assert g.fits and g.inside.all() and 1 < np.count_nonzero(g.records) <= FE_TO_NMAX and g.vox_members.max() <= 255
        assert 5000 <= len(p) <= 60000


# ---- 1. stage 1 --------------------------------------------------------------------------------------------------------------------------------------
def test_stage_one_three_sets_of_centres(backend):
    """three rooms, three sets of centres from one plan: every key equals the unplanned call's (`scattered` < `points` among them: the order counted what stage 1 was
    given), the plan reports 32 bytes per raw point, and the planned call passes no scatter site"""
    rng = np.random.default_rng(201)
    rooms = _three_rooms(rng)
    _ordinary(rooms)
    for p, _, _ in rooms[:2]:          # about one point per occupied voxel: stage 1's 6 x 1024 points hold more than 1024 rows, in a part of the buckets
        g = geometry(p, DL)
        assert len(p) / len(g.vox_key) < 2.0 and len(p) > 3 * 6 * N
    S = _Set(rooms, 202)
    try:
        plan = S.plan()
        assert _info(S, plan) == (32 * S.nt, 0)
        sets = [CEN3, [(0.01, 0.02, 0.01), (12.99, -1.51, 2.99), (-5.0, 1.5, 0.0)], [(4.9, -0.6, 3.1), (9.2, -4.5, 0.4), (-2.5, 0.7, 1.6)]]
        outs = []
        for i, cen in enumerate(sets):
            got, ref = _pair(S, cen, plan, "centres %d" % i)
            assert list(got["stage"]) == [1, 1, 1] and got["reduced"][0] < got["buckets"][0]
            assert 0 < got["scattered"][0] < got["points"][0] and 0 < got["scattered"][1] < got["points"][1]
            assert list(got["points"]) == [len(r[0]) for r in rooms]
            outs.append(got)
        assert not np.array_equal(outs[0]["xyz"], outs[1]["xyz"]) and not np.array_equal(outs[1]["xyz"], outs[2]["xyz"])
        assert not np.array_equal(outs[0]["scattered"], outs[1]["scattered"])
    finally:
        S.close()


# ---- 2. the later stages: no second scatter -------------------------------------------------------------------------------------------------------------
def test_stages_two_and_three(backend):
    """the rooms of test_frontend_room_plan.test_stage_two_and_stage_three_with_padding: stages 2, 3, 3.  A room that goes on was given all of its records
    (scattered == points, counted by fe_tile_plan<2>), and every output is the unplanned call's although no second scatter ran"""
    rng = np.random.default_rng(111)
    nv = np.array([60, 60, 50])
    cells = np.stack(np.unravel_index(rng.choice(int(nv.prod()), 12500, replace=False), nv), 1)
    dense = ((np.repeat(cells, 16, 0) + 0.1 + 0.8 * np.repeat(rng.random((len(cells), 3)), 16, 0)) * DL).astype(F32)
    few, c_few, nvox = _few_voxels_many_points(rng)
    short, c_short, n_in, n_out = _short_estimate_room(rng)
    gd = geometry(dense, DL)
    assert gd.fits and gd.inside.all() and (gd.vox_members == 16).all() and len(gd.vox_key) == 12500          # stage 1's 6 x 1024 points are 384 rows
    assert nvox < N and len(few) > 6 * N and n_in < N < n_in + n_out
    for p in (few, short):
        g = geometry(p, DL)
        assert g.fits and g.inside.all() and np.count_nonzero(g.records) <= FE_TO_NMAX
    S = _Set([_room(rng, dense), _room(rng, few), _room(rng, short)], 112)
    try:
        plan = S.plan()
        assert _info(S, plan) == (32 * S.nt, 0)
        got, ref = _pair(S, [(1.2, 1.3, 1.0), c_few, c_short], plan, "stages")
        print("stage %s, reduced %s of %s, given %s of %s" % (got["stage"], got["reduced"], got["buckets"], got["scattered"], got["points"]))
        assert list(got["stage"]) == [2, 3, 3]
        assert list(got["scattered"][1:]) == list(got["points"][1:]) and got["scattered"][0] == got["points"][0]
        assert got["m"][1] == nvox and got["m"][2] == n_in + n_out and got["reduced"][0] < got["buckets"][0]
    finally:
        S.close()


# ---- 3. large buckets, refused rooms, a room without an order ----------------------------------------------------------------------------------------------
def _sliced_room(rng):
    """24 x 16 x 8 voxels, every one holding 16 points: six buckets of 8192 records, each cut into slices of consecutive voxels, and no voxel above FE_CAP"""
    nv = np.array([24, 16, 8])
    cells = np.stack(np.meshgrid(*[np.arange(k) for k in nv], indexing="ij"), -1).reshape(-1, 3)
    return ((np.repeat(cells, 16, 0) + 0.1 + 0.8 * rng.random((16 * len(cells), 3))) * DL).astype(F32)


def test_large_buckets_refused_and_unordered_rooms(backend):
    """One call over: a room whose buckets hold more than FE_CAP records at 16 points per voxel (the reduction's slice path, over records it did not see written); a
    voxel of more than FE_CAP points (status bit 4, as from the unplanned call); a grid the partition refuses (bit 2: no record in the plan, the tile untouched); a slab
    of more than FE_TO_NMAX non-empty buckets (stage 0: given whole); a normal room."""
    rng = np.random.default_rng(221)
    sliced = _sliced_room(rng)
    gs = geometry(sliced, DL)
    assert gs.fits and gs.inside.all() and gs.nb == 6 and (gs.vox_members == 16).all()
    for b in range(gs.nb):
        hist = FP.bucket_hist(gs, b)
        bounds, taken = FP.slices(hist)
        assert hist.sum() > FE_CAP and hist.max() <= FE_CAP and taken and len(bounds) - 1 >= 2
    crowd = np.concatenate([_box(rng, 30000, (3.0, 3.0, 2.0)), np.tile(np.array([[1.5, 1.5, 1.0]], F32) + F32(0.003), (FE_CAP + 80, 1))])
    assert geometry(crowd, DL).vox_members.max() > FE_CAP
    huge = _box(rng, 5000, (100.0, 100.0, 3.0))
    assert not geometry(huge, DL).fits
    sparse = _box(rng, 40000, (52.0, 34.0, 0.3))
    gp = geometry(sparse, DL)
    assert gp.fits and gp.inside.all() and np.count_nonzero(gp.records) > FE_TO_NMAX
    normal = _three_rooms(rng)[1]
    _ordinary([normal])
    S = _Set([_room(rng, sliced), _room(rng, crowd), _room(rng, huge), _room(rng, sparse), normal], 222)
    try:
        plan = S.plan()
        assert _info(S, plan) == (32 * S.nt, 0)
        cen = [(0.5, 0.3, 0.16), (1.52, 1.49, 1.02), (50.0, 50.0, 1.5), (21.0, 13.0, 0.15), (11.5, -2.7, 2.0)]
        got, ref = _pair(S, cen, plan, "large buckets")
        assert got["status"][0] == ref["status"][0] and got["status"][0] & 4 and got["status"][0] & 2
        assert list(got["stage"])[1:] == [1, 0, 0, 1] and got["m"][0] >= N and got["m"][2] == 0 and got["reduced"][3] == got["buckets"][3] > FE_TO_NMAX
        assert got["scattered"][2] == 0 and got["scattered"][3] == got["points"][3] and 0 < got["scattered"][4] < got["points"][4]
        assert (got["xyz"][2] == F32(-77.25)).all() and (got["xyz"][0] != F32(-77.25)).all()
    finally:
        S.close()


# ---- 4. the exact label vote -----------------------------------------------------------------------------------------------------------------------------
def test_labels_that_take_the_exact_vote(backend):
    """labels of 13 and more, and a voxel of 300 duplicates whose winning label's byte counter wraps: both are settled by fe_label_exact from the members themselves,
    read from the plan's records.  All rows (points, features and labels together) are shuffled, so a voxel's members arrive in another order than their indices'."""
    rng = np.random.default_rng(231)
    cv = np.array([30, 25, 20])                                                        # the crowded voxel
    p = np.concatenate([_box(rng, 20000, (3.0, 2.5, 2.0)), ((cv + 0.25 + 0.5 * rng.random((300, 3))) * float(F32(DL))).astype(F32)])
    lab = np.concatenate([rng.integers(0, 20, (20000, 1)), FP.wrapping_labels(rng, 300)]).astype(np.int32)
    perm = rng.permutation(len(p))
    p, lab = np.ascontiguousarray(p[perm]), np.ascontiguousarray(lab[perm])
    room = (p, rng.integers(0, 256, (len(p), 3)).astype(F32), lab)
    g = geometry(p, DL)
    assert g.fits and g.inside.all() and (lab >= 13).any()
    k = g.vox_key[np.argmax(g.vox_members)]
    members = np.flatnonzero(g.key == k)
    assert 255 < len(members) <= FE_CAP and FP.byte_counter_wraps(lab[members[lab[members, 0] < 13], 0]) and (np.diff(members) > 1).any()
    assert FP.max_distinct_labels(g, lab) <= FP.LAB_CAP
    small = _three_rooms(rng)[2]
    _ordinary([small])
    S = _Set([room, small], 232)
    try:
        plan = S.plan()
        centre = tuple(float(x) for x in (cv + 0.5) * DL)                              # the crowded voxel's bucket is the first of the order
        got, ref = _pair(S, [centre, (-4.0, 0.7, 0.5)], plan, "exact vote")
        assert got["stage"][0] == 1 and got["status"][0] == 0
        rows = got["sub_p"][:got["m"][0]]
        assert (np.floor((rows - g.org) / g.dl) == cv).all(1).any(), "the crowded voxel's row was not produced"
    finally:
        S.close()


# ---- 5. the generic row layouts --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fdim,ldim", [(2, 2), (0, 1)])
def test_generic_row_layouts(backend, fdim, ldim):
    """rows that are not 3 features + 1 label: the plan's records come from fe_scatter<-1, -1, 0>, the rows from fe_reduce<-1, -1, false> / fe_move<-1, -1>"""
    rng = np.random.default_rng(241)
    rooms = [_room_g(rng, _box(rng, 40000, (4.0, 3.0, 2.5)), fdim, ldim), _room_g(rng, _box(rng, 9000, (2.0, 1.5, 1.0), (7.0, 0.0, 0.0)), fdim, ldim),
             _room_g(rng, _box(rng, 20000, (3.0, 2.0, 2.0), (0.0, 9.0, 0.0)), fdim, ldim)]
    _ordinary(rooms)
    S = _Set(rooms, 242, fdim, ldim)
    try:
        plan = S.plan()
        assert _info(S, plan) == (32 * S.nt, 0)
        for cen in ([(2.0, 1.5, 1.2), (8.0, 0.7, 0.5), (1.5, 10.0, 1.0)], [(0.0, 0.0, 0.0), (9.1, 1.6, 1.1), (3.0, 9.0, 2.0)]):
            got, ref = _pair(S, cen, plan, "layout %d + %d" % (fdim, ldim))
            assert got["reduced"][0] < got["buckets"][0] and 0 < got["scattered"][0] < got["points"][0]
    finally:
        S.close()


# ---- 6. streams, and other calls in between -----------------------------------------------------------------------------------------------------------------
def test_streams_and_an_unplanned_call_in_between(backend):
    """The records are written on stream a; the first call that reads them runs on stream b (behind the plan's event), then the library's stream, then a.  An unplanned
    call over OTHER, larger rooms on the same stream between two planned calls rewrites the whole per-stream record buffer, whose layout a planned call shares (its
    rows region starts where that call's records do): both planned calls still equal their references."""
    from ssdr_al import _lib
    L = _lib.lib()
    rng = np.random.default_rng(251)
    rooms_a = _three_rooms(rng)
    rooms_b = [_room(rng, _box(rng, 50000, (6.0, 2.0, 2.0), (3.0, 3.0, 3.0))), _room(rng, _box(rng, 60000, (5.0, 5.0, 2.5))),
               _room(rng, _box(rng, 12000, (1.0, 4.0, 2.0), (-9.0, 0.0, 0.0))), _room(rng, _box(rng, 6000, (1.0, 1.0, 1.0)))]
    _ordinary(rooms_a + rooms_b)
    A, B = _Set(rooms_a, 252), _Set(rooms_b, 253)
    assert B.nt > A.nt
    a, b = C.c_void_p(), C.c_void_p()
    _lib.check(L.ssdr_stream_create(C.byref(a))); _lib.check(L.ssdr_stream_create(C.byref(b)))
    try:
        c1, c2 = CEN3, [(3.5, 0.4, 2.2), (10.2, -3.9, 1.2), (-3.3, 1.2, 0.2)]
        plan = A.plan(a.value)
        got_b = A.call(c1, plan, b.value)
        r1, r2 = A.call(c1), A.call(c2)
        _same(got_b, r1, "stream b")
        _same(A.call(c1, plan), r1, "library stream")
        _same(A.call(c1, plan, a.value), r1, "stream a")
        other = B.call([(6.0, 4.0, 4.0), (2.5, 2.5, 1.2), (-8.5, 2.0, 1.0), (0.5, 0.5, 0.5)], None, b.value)
        _same(A.call(c2, plan, b.value), r2, "stream b, after an unplanned call on it")
        assert len(other["m"]) == 4 and (other["m"] > 0).all()
        assert _info(A, plan) == (32 * A.nt, 0)
    finally:
        A.close(); B.close()
        _lib.check(L.ssdr_stream_destroy(a)); _lib.check(L.ssdr_stream_destroy(b))


# ---- 7. the switches ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,value", [("SSDR_FE_PLAN_RECORDS", "0"), ("SSDR_FE_PLAN_RECORDS_MAX_MB", "1")])
def test_switches_give_a_plan_without_records(backend, monkeypatch, name, value):
    """read at the plan's creation: the A/B switch, and a cap (1 MB) below the 3.1 MB of these rooms' records.  Such a plan's calls scatter per call and equal the
    reference; a plan created after the switch is gone holds records again"""
    rng = np.random.default_rng(261)
    rooms = _three_rooms(rng)
    _ordinary(rooms)
    S = _Set(rooms, 262)
    assert 32 * S.nt > 1 << 20
    try:
        monkeypatch.setenv(name, value)
        plain = S.plan()
        assert _info(S, plain) == (0, 0)
        monkeypatch.delenv(name)
        full = S.plan()
        assert _info(S, full) == (32 * S.nt, 0) and _info(S, plain) == (0, 0)
        got, ref = _pair(S, CEN3, plain, "without records", records=False)
        assert 0 < got["scattered"][0] < got["points"][0]
        _pair(S, CEN3, full, "with records")
    finally:
        S.close()


# ---- 8. new points, new plan ---------------------------------------------------------------------------------------------------------------------------------
def test_rebuilt_plan_holds_the_new_points(backend):
    """destroy, rewrite the points in place (the same device pointers and offsets), create: the records are the new points'"""
    from ssdr_al import _lib
    rng = np.random.default_rng(271)
    rooms = _three_rooms(rng)
    _ordinary(rooms)
    S = _Set(rooms, 272)
    try:
        plan = S.plan()
        old, _ = _pair(S, CEN3, plan, "old points")
        S.destroy(plan)
        new_p = np.concatenate([_box(rng, 60000, (3.0, 4.0, 2.0), (0.5, -0.5, 0.2)), _box(rng, 30000, (2.0, 3.0, 2.5), (10.5, -4.0, 0.5)), _box(rng, 8000, (1.5, 2.0, 1.2), (-4.5, 0.0, 0.0))])
        assert new_p.shape == S.d_p.shape
        for lo, hi in zip(S.off[:-1], S.off[1:]):
            g = geometry(new_p[lo:hi], DL)
            assert g.fits and g.inside.all()
        _lib.check(S.L.ssdr_memcpy_h2d(S.d_p.ptr, _lib.ptr(new_p), new_p.nbytes))
        plan = S.plan()
        assert _info(S, plan) == (32 * S.nt, 0)
        new, _ = _pair(S, CEN3, plan, "new points")
        assert not np.array_equal(new["xyz"], old["xyz"]) and not np.array_equal(new["buckets"], old["buckets"]) and not np.array_equal(new["scattered"], old["scattered"])
    finally:
        S.close()
