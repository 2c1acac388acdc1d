"""ssdr_tile_from_rooms_batch_dev (csrc/frontend.hip: the staged reduction; csrc/subsample.hip: the entry point) against the two calls it stands for,
ssdr_grid_subsample_batch_dev followed by ssdr_tile_select_batch_dev over all rows: xyz, feat and the tile's labels bit for bit, on the CPU logic build and on
the gfx950 build, and the stage ssdr_tile_from_rooms_stats reports for every room (1: the first stage's buckets, 6 num_points points and their shell, sufficed or were the whole room, 2: the
set estimated from the first stage's points per voxel sufficed, 3: the rest of the room was needed, 0: reduced whole without an order, -1: the sort).  The two calls are the reference: their own tests
(test_subsample_paths.py, test_tile_paths.py) hold them to the oracles.  Every case states its input condition (which stage, which grid, which bucket) and
asserts it: with tests/_fe_paths.py: geometry before the call where the geometry decides, with the stats after it where the device's counts do.

Rooms are 5 k to 200 k raw points, tiles 1024 or 4096 rows, dl 0.04 (0.0625 where exact ties need binary fractions)."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal
import _fe_paths as FP
from _fe_paths import AUTO, SORT, F32, FE_CAP, geometry

DL = 0.04
SCALE = 1.0 / 255.0
FE_TO_NMAX = 8192              # csrc/frontend.hip: non-empty buckets of a room the order is sorted for


def _room(rng, p):
    """raw rows of a room: colours 0..255, one label column in [0,13), the rows shuffled"""
    p = np.ascontiguousarray(p, F32)[rng.permutation(len(p))]
    return p, rng.integers(0, 256, (len(p), 3)).astype(F32), rng.integers(0, 13, (len(p), 1)).astype(np.int32)


def _box(rng, n, box, shift=(0, 0, 0)):
    return (rng.random((n, 3), dtype=F32) * np.asarray(box, F32) + np.asarray(shift, F32)).astype(F32)


def _run(rooms, centres, N, seed, method=AUTO, fused=True, dl=DL):
    """one call of the fused entry point (or of the two calls) -> dict(xyz [R, N, 3], feat [R, N, 6], lab [R, N], m [R], status, stage, reduced, buckets)"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    L = _lib.lib()
    rng = np.random.default_rng(seed)
    R = len(rooms)
    off = np.concatenate([[0], np.cumsum([len(r[0]) for r in rooms])]).astype(np.int64)
    nt = int(off[-1])
    perm = np.stack([rng.permutation(N) for _ in range(R)]).astype(np.int32)
    dup = rng.random((R, N)).astype(F32)
    dup[:, -1] = 1.0
    d_p, d_f, d_l = (DevArray.from_host(np.concatenate([r[k] for r in rooms])) for k in range(3))
    s_p, s_f, s_l = DevArray((nt, 3), np.float32), DevArray((nt, 3), np.float32), DevArray((nt, 1), np.int32)
    s_m = DevArray.from_host(np.zeros(R + 1, np.int64))
    d_perm, d_dup = DevArray.from_host(perm), DevArray.from_host(dup)
    o_xyz, o_feat = DevArray.from_host(np.full((R, N, 3), -77.25, F32)), DevArray.from_host(np.full((R, N, 6), -77.25, F32))
    o_lab = DevArray.from_host(np.full((R, N), -77, np.int32))
    cen = np.ascontiguousarray(np.asarray(centres, F32).reshape(R, 3))
    _lib.check(L.ssdr_grid_subsample_set_method(method))
    try:
        if fused:
            _lib.check(L.ssdr_tile_from_rooms_batch_dev(d_p.ptr, d_f.ptr, 3, d_l.ptr, 1, _lib.ptr(off), R, dl, s_p.ptr, s_f.ptr, s_l.ptr, s_m.ptr, _lib.ptr(cen), N,
                                                        d_perm.ptr, d_dup.ptr, SCALE, o_xyz.ptr, o_feat.ptr, None, o_lab.ptr, None))
        else:
            _lib.check(L.ssdr_grid_subsample_batch_dev(d_p.ptr, d_f.ptr, 3, d_l.ptr, 1, _lib.ptr(off), R, dl, s_p.ptr, s_f.ptr, s_l.ptr, s_m.ptr, None))
            _lib.check(L.ssdr_tile_select_batch_dev(s_p.ptr, s_f.ptr, 3, s_m.ptr, _lib.ptr(off), R, _lib.ptr(cen), N, d_perm.ptr, d_dup.ptr, SCALE,
                                                    o_xyz.ptr, o_feat.ptr, None, s_l.ptr, o_lab.ptr, None))
        st = C.c_int32()
        L.ssdr_grid_subsample_status(None, C.byref(st))
        out = dict(xyz=o_xyz.to_host(), feat=o_feat.to_host(), lab=o_lab.to_host(), m=s_m.to_host()[:R], status=st.value)
        if fused:
            stats = [np.zeros(R, np.int32) for _ in range(3)]
            _lib.check(L.ssdr_tile_from_rooms_stats(None, *[_lib.ptr(a) for a in stats], R))
            out.update(stage=stats[0], reduced=stats[1], buckets=stats[2])
    finally:
        _lib.check(L.ssdr_grid_subsample_set_method(AUTO))
    return out


def _compare(rooms, centres, N, seed, stages, method=AUTO, ref_method=None, status=0, dl=DL):
    """fused call == the two calls, bit for bit; `stages`: the stage every room must report -> (fused, two calls)"""
    ref = _run(rooms, centres, N, seed, ref_method if ref_method is not None else method, fused=False, dl=dl)
    got = _run(rooms, centres, N, seed, method, fused=True, dl=dl)
    print("stage %s, buckets reduced %s of %s, rows %s of %s" % (got["stage"], got["reduced"], got["buckets"], got["m"], ref["m"]))
    assert ref["status"] == (status if ref_method is None else 0) and got["status"] == status
    for r in range(len(rooms)):
        assert_bits_equal(got["xyz"][r], ref["xyz"][r], "room %d xyz" % r)
        assert_bits_equal(got["feat"][r], ref["feat"][r], "room %d feat" % r)
        assert np.array_equal(got["lab"][r], ref["lab"][r]), "room %d labels" % r
    assert (ref["xyz"] != F32(-77.25)).any()
    assert list(got["stage"]) == list(stages), "stages %s, expected %s" % (got["stage"], stages)
    return got, ref


# ---- 1. where the centre lies --------------------------------------------------------------------------------------------------------------------
CENTRES = {"middle": (2.0, 1.5, 1.25), "corner": (0.01, 0.02, 0.01), "outside": (4.9, -0.6, 3.1)}


@pytest.mark.parametrize("where", list(CENTRES))
def test_centre_positions(backend, where):
    """A room of uniform density, about one point per occupied voxel (60 k points in 4 x 3 x 2.5 m, 1040 buckets): stage 1's 6 x 1024 points hold more than 1024
    rows, so it suffices wherever the centre lies: in the middle, in a corner (the ball is cut by three walls: the cumulative counts are of real points), outside the
    box (the pick plus its noise)."""
    rng = np.random.default_rng(11)
    room = _room(rng, _box(rng, 60000, (4.0, 3.0, 2.5)))
    got, ref = _compare([room], [CENTRES[where]], 1024, 12, [1])
    assert 0 < got["reduced"][0] < got["buckets"][0] and got["m"][0] < ref["m"][0]


def test_stage_one_reduces_a_fraction(backend):
    """200 k points, a 4096-row tile: stage 1 ends it with well under half of the buckets reduced, and sub_m counts the reduced rows"""
    rng = np.random.default_rng(21)
    room = _room(rng, _box(rng, 200000, (8.0, 6.0, 3.0)))
    got, ref = _compare([room], [(3.1, 2.2, 1.4)], 4096, 22, [1])
    assert 4096 <= got["m"][0] < ref["m"][0] // 2 and got["reduced"][0] < got["buckets"][0] // 2


def test_stage_two(backend):
    """16 points in every occupied voxel (12 500 voxels, 200 k points): stage 1's 6 x 1024 points are 384 rows and cannot suffice; it measures 16 points per voxel, and
    stage 2's 1.15 x 16 x 1024 points hold the tile with a part of the room's buckets"""
    rng = np.random.default_rng(25)
    nv = np.array([60, 60, 50])
    cells = np.stack(np.unravel_index(rng.choice(int(nv.prod()), 12500, replace=False), nv), 1)
    p = ((np.repeat(cells, 16, 0) + 0.1 + 0.8 * np.repeat(rng.random((len(cells), 3)), 16, 0)) * DL).astype(F32)
    got, ref = _compare([_room(rng, p)], [(1.2, 1.3, 1.0)], 1024, 26, [2])
    assert got["reduced"][0] < got["buckets"][0] and 1024 <= got["m"][0] < ref["m"][0] == 12500


# ---- 2. the estimate falls short ------------------------------------------------------------------------------------------------------------------
def _short_estimate_room(rng):
    """Around the centre (radius 10 voxels) 10 % of the voxels hold 8 duplicates of a point: about 400 occupied voxels, fewer than the 1024 of the tile, at 8 points
    per voxel.  Everywhere else (6.4 x 6.4 x 2.56 m) 0.1 % of the voxels hold 100 duplicates: the points that stage 1 (6 x 1024) and stage 2 (1.15 x the measured points per voxel x 1024)
    ask for are reached after a few hundred voxels more.  The rows with a greatest distance below the frontier stay short of 1024 both times: stage 3."""
    nv = np.array([160, 160, 64])
    c = (nv // 2).astype(np.float64)
    ijk = np.stack(np.meshgrid(*[np.arange(k) for k in nv], indexing="ij"), -1).reshape(-1, 3)
    inner = ((ijk + 0.5 - c) ** 2).sum(1) < 100.0
    u = rng.random(len(ijk))
    a, b = ijk[inner & (u < 0.10)], ijk[~inner & (u < 0.001)]
    cells = np.concatenate([np.repeat(a, 8, 0), np.repeat(b, 100, 0)])
    jitter = np.repeat(rng.random((len(a) + len(b), 3)), np.concatenate([np.full(len(a), 8), np.full(len(b), 100)]), 0)
    return ((cells + 0.1 + 0.8 * jitter) * DL).astype(F32), (c * DL).astype(F32), len(a), len(b)


def test_stage_three(backend):
    """the estimate from stage 1's points per voxel falls short: the check fails and the rest of the room is reduced"""
    rng = np.random.default_rng(31)
    p, centre, n_in, n_out = _short_estimate_room(rng)
    assert 5000 <= len(p) <= 200000 and n_in < 1024 < n_in + n_out
    got, ref = _compare([_room(rng, p)], [centre], 1024, 32, [3])
    assert got["reduced"][0] == got["buckets"][0] and got["m"][0] == ref["m"][0] == n_in + n_out


# ---- 3. a room smaller than the tile ----------------------------------------------------------------------------------------------------------------
def test_room_smaller_than_tile(backend):
    """5000 points in fewer than 1024 voxels: fewer points than stage 1 asks for, its ranks are all the room's, and the tile is padded with the duplicate draws"""
    rng = np.random.default_rng(41)
    p = _box(rng, 5000, (0.52, 0.36, 0.16), (1.0, 2.0, 0.5))
    assert len(geometry(p, DL).vox_key) < 1024
    got, ref = _compare([_room(rng, p)], [(1.2, 2.1, 0.55)], 1024, 42, [1])
    assert got["reduced"][0] == got["buckets"][0] and got["m"][0] == ref["m"][0] < 1024


# ---- 4. exact ties at the cut -----------------------------------------------------------------------------------------------------------------------
def test_ties_at_the_cut(backend):
    """One point per voxel on a lattice of binary fractions (dl = 1/16), the centre on a lattice node: every distance is exact and whole shells tie.  The 1024th and
    the 1025th nearest barycentres are equidistant: the row index decides, and the rows of the reduced buckets keep the order of all rows."""
    rng = np.random.default_rng(51)
    dl = 0.0625
    ijk = np.stack(np.meshgrid(*[np.arange(40)] * 3, indexing="ij"), -1).reshape(-1, 3)
    p = ((ijk + 0.5) * dl).astype(F32)
    centre = ((np.array([17, 22, 19]) + 0.5) * dl).astype(F32)
    d = np.sort(((p - centre) ** 2).sum(1).astype(F32))
    assert d[1023] == d[1024] and d[1023] > d[0]
    _compare([_room(rng, p)], [centre], 1024, 52, [1], dl=dl)


# ---- 5. grids and buckets off the common path, rooms of very different sizes in one call ------------------------------------------------------------------
def test_mixed_batch(backend):
    """One call over: a thin slab whose grid takes 16 x 8 x 8 buckets (sx = 4) with a dense room in it; a room with a bucket of more than FE_CAP records at the
    centre (slices); a room of 5 k points, fewer than stage 1 asks for: it takes the room whole; a room of 200 k points; and a slab with more than FE_TO_NMAX non-empty buckets, which is reduced whole (stage 0)."""
    rng = np.random.default_rng(61)
    wide = np.concatenate([_box(rng, 30000, (4.0, 3.0, 0.3), (20.0, 10.0, 0.0)), _box(rng, 400, (52.0, 34.0, 0.3))])
    g = geometry(wide, DL)
    assert g.fits and g.sx == 4
    blob_at = np.array([1.6, 1.6, 1.28], F32)          # a bucket corner + half a bucket: the blob stays inside one bucket
    crowded = np.concatenate([_box(rng, 40000, (3.2, 3.2, 2.56)), _box(rng, 3000, (0.3, 0.3, 0.3), blob_at + 0.01)])
    gc = geometry(crowded, DL)
    assert gc.records.max() > FE_CAP and gc.vox_members.max() <= FE_CAP
    small = _box(rng, 5000, (1.5, 1.2, 1.0), (-3.0, -2.0, 0.0))
    big = _box(rng, 200000, (8.0, 6.0, 3.0))
    sparse = _box(rng, 40000, (52.0, 34.0, 0.3))
    gs = geometry(sparse, DL)
    assert gs.fits and np.count_nonzero(gs.records) > FE_TO_NMAX
    rooms = [_room(rng, x) for x in (wide, crowded, small, big, sparse)]
    centres = [(22.0, 11.5, 0.15), blob_at + 0.16, (-2.2, -1.4, 0.5), (4.0, 3.0, 1.5), (21.0, 13.0, 0.15)]
    got, ref = _compare(rooms, centres, 4096, 62, [1, 1, 1, 1, 0])
    assert got["reduced"][4] == got["buckets"][4] == np.count_nonzero(gs.records)
    assert got["reduced"][0] < got["buckets"][0] and got["reduced"][3] < got["buckets"][3]


# ---- 6. a cloud the partition refuses ---------------------------------------------------------------------------------------------------------------
def test_refused_cloud_takes_the_sort(backend):
    """A voxel of more than FE_CAP points beside the centre: the partition reports bit 4 from the fused call as from the two calls, and the fused call under the sort
    gives the sort route's tiles (no stage: -1)."""
    rng = np.random.default_rng(71)
    p = np.concatenate([_box(rng, 30000, (3.0, 3.0, 2.0)), np.tile(np.array([[1.5, 1.5, 1.0]], F32) + F32(0.003), (FE_CAP + 80, 1))])
    assert geometry(p, DL).vox_members.max() > FE_CAP
    rooms, centre = [_room(rng, p)], [(1.52, 1.49, 1.02)]
    refused = _run(rooms, centre, 1024, 72, AUTO, fused=True)
    assert refused["status"] & 4
    _compare(rooms, centre, 1024, 72, [-1], method=SORT)
