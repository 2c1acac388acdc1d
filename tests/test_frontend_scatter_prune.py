"""The pruned scatter of ssdr_tile_from_rooms_batch_dev (csrc/frontend.hip): the order of a room's buckets is taken BEFORE the records are written, the scatter
writes only the records of the buckets stage 1 reduces, and a room that goes on to stage 2 gets the rest of its records from a second pass.  Every case compares the
fused call with the two calls it stands for (ssdr_grid_subsample_batch_dev + ssdr_tile_select_batch_dev) bit for bit, on the CPU logic build and on the gfx950 build, and
asserts its own input condition from the stats: the stage of every room (ssdr_tile_from_rooms_stats) and the records written against the room's points
(ssdr_tile_from_rooms_scatter_stats).

The fused call always runs BEFORE its reference here: the record buffer of the stream then holds what an earlier call left (another room's records, or nothing), never
the full set of records of the room under test, so a bucket that is read without having been written shows.

Rooms are 5 k to 200 k raw points, tiles 1024 rows, dl 0.04."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from _fe_paths import F32, geometry
from test_frontend_tile_prune import DL, FE_TO_NMAX, _box, _room, _run, _short_estimate_room

FE_CH = 32768                  # csrc/frontend.hip: points per chunk of the count / scatter kernels
FE_STEP = 1024 * 12            # FE_SNT * FE_PPT: points a scatter workgroup takes per step


def _scatter_stats(R):
    """(records written, points) per room of the last fused call on the default stream"""
    from ssdr_al import _lib
    sc, pts = np.zeros(R, np.int64), np.zeros(R, np.int64)
    _lib.check(_lib.lib().ssdr_tile_from_rooms_scatter_stats(None, _lib.ptr(sc), _lib.ptr(pts), R))
    return sc, pts


def _fused(rooms, centres, N, seed):
    got = _run(rooms, centres, N, seed, fused=True)
    got["scattered"], got["points"] = _scatter_stats(len(rooms))
    assert list(got["points"]) == [len(r[0]) for r in rooms]
    return got


def _same(got, rooms, centres, N, seed, stages):
    """the fused call's tiles against the two calls', bit for bit; the stage every room must report"""
    ref = _run(rooms, centres, N, seed, fused=False)
    print("stage %s, buckets reduced %s of %s, records %s of %s points" % (got["stage"], got["reduced"], got["buckets"], got["scattered"], got["points"]))
    assert ref["status"] == 0 and got["status"] == 0
    for r in range(len(rooms)):
        assert_bits_equal(got["xyz"][r], ref["xyz"][r], "room %d xyz" % r)
        assert_bits_equal(got["feat"][r], ref["feat"][r], "room %d feat" % r)
        assert np.array_equal(got["lab"][r], ref["lab"][r]), "room %d labels" % r
    assert (ref["xyz"] != F32(-77.25)).any()
    assert list(got["stage"]) == list(stages), "stages %s, expected %s" % (got["stage"], stages)
    return ref


def _check(rooms, centres, N, seed, stages):
    got = _fused(rooms, centres, N, seed)
    _same(got, rooms, centres, N, seed, stages)
    return got


def _stage_two_room(rng):
    """16 points in every occupied voxel (12 500 voxels, 200 k points): stage 1 measures 16 points per voxel, stage 2 holds the tile (test_frontend_tile_prune.test_stage_two)"""
    nv = np.array([60, 60, 50])
    cells = np.stack(np.unravel_index(rng.choice(int(nv.prod()), 12500, replace=False), nv), 1)
    return ((np.repeat(cells, 16, 0) + 0.1 + 0.8 * np.repeat(rng.random((len(cells), 3)), 16, 0)) * DL).astype(F32)


# ---- 1. every record range holds another room's records -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", [1, 2])
def test_stale_records(backend, stage):
    """A call over a DIFFERENT room of the same point count first: every record range then holds plausible records of that room.  The stage-1 room leaves the ranges of its
    unflagged buckets as they are (and nobody reads them); the stage-2 room fills them in the second pass before the reduction sees them."""
    rng = np.random.default_rng(100 + stage)
    if stage == 1:
        room, centre = _room(rng, _box(rng, 200000, (8.0, 6.0, 3.0))), (3.1, 2.2, 1.4)
        other = _room(rng, _box(rng, 200000, (7.0, 6.5, 3.2), (0.3, -0.2, 0.1)))
    else:
        room, centre = _room(rng, _stage_two_room(rng)), (1.2, 1.3, 1.0)
        other = _room(rng, _stage_two_room(rng))
    assert len(other[0]) == len(room[0])
    _run([other], [centre], 1024, 110 + stage, fused=True)
    got = _check([room], [centre], 1024, 120 + stage, [stage])
    if stage == 1:
        assert 0 < got["scattered"][0] < got["points"][0]
    else:
        assert got["scattered"][0] == got["points"][0]


# ---- 2. every stage in one call ------------------------------------------------------------------------------------------------------------------
def test_every_stage_in_one_call(backend):
    """One call over rooms that end in stage 1 (200 k uniform points: seven chunks), 2, 3 and 0 (more than FE_TO_NMAX non-empty buckets: no order, every bucket in the first
    scatter), plus a room smaller than the tile (5 k points, less than a chunk: stage 1 takes it whole).  The second pass runs for the rooms of stages 2 and 3 and returns
    for the others; whoever is reduced whole has had every point written exactly once."""
    rng = np.random.default_rng(201)
    uniform = _box(rng, 200000, (8.0, 6.0, 3.0))
    two = _stage_two_room(rng)
    three, c3, n_in, n_out = _short_estimate_room(rng)
    sparse = _box(rng, 40000, (52.0, 34.0, 0.3))
    gs = geometry(sparse, DL)
    assert gs.fits and np.count_nonzero(gs.records) > FE_TO_NMAX
    small = _box(rng, 5000, (0.52, 0.36, 0.16), (1.0, 2.0, 0.5))
    assert len(geometry(small, DL).vox_key) < 1024 and len(small) < FE_CH < len(uniform)
    rooms = [_room(rng, x) for x in (uniform, two, three, sparse, small)]
    centres = [(3.1, 2.2, 1.4), (1.2, 1.3, 1.0), c3, (21.0, 13.0, 0.15), (1.2, 2.1, 0.55)]
    got = _check(rooms, centres, 1024, 202, [1, 2, 3, 0, 1])
    sc, pts = got["scattered"], got["points"]
    assert sc[0] < pts[0] // 2
    assert sc[1] == pts[1] and got["reduced"][1] < got["buckets"][1]          # stage 1's records plus the second pass's
    assert sc[2] == pts[2] and sc[3] == pts[3]
    assert sc[4] == pts[4] and got["reduced"][4] == got["buckets"][4]


# ---- 3. the scatter's loop edges with skipped points ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [FE_CH, FE_CH + 1, FE_STEP - 1, FE_STEP, FE_STEP + 1, 20001])
def test_loop_edges(backend, n):
    """Point counts at the ends of the scatter's loops: a whole chunk and one point more (a second workgroup with a single point), a whole step of a workgroup, one point
    less and one more, and an odd count (the last lane pair is half empty).  A long room with the centre at one end: stage 1's 6 x 1024 points are the near part of it, and
    the rows are shuffled, so every step (the last one too, where it holds more than a point) carries points of flagged and of unflagged buckets."""
    rng = np.random.default_rng(300 + n % 97)
    room = _room(rng, _box(rng, n, (12.0, 1.5, 1.0)))
    got = _check([room], [(0.4, 0.7, 0.5)], 1024, 301, [1])
    assert got["reduced"][0] < got["buckets"][0] and 0 < got["scattered"][0] < got["points"][0] == n


# ---- 4. every lane pair mixed ---------------------------------------------------------------------------------------------------------------------
def test_pairs_of_a_kept_and_a_skipped_point(backend):
    """Two blobs 10 m apart, their points interleaved (even rows: the blob that holds the centre, odd rows: the other one), NOT shuffled: in every even / odd lane pair of the
    scatter one record is written and its partner's is not, so each lane stores one half of one record."""
    rng = np.random.default_rng(401)
    a, b = _box(rng, 20000, (2.0, 2.0, 2.0)), _box(rng, 20000, (2.0, 2.0, 2.0), (12.0, 0.0, 0.0))
    p = np.empty((40000, 3), F32)
    p[0::2], p[1::2] = a, b
    room = (p, rng.integers(0, 256, (len(p), 3)).astype(F32), rng.integers(0, 13, (len(p), 1)).astype(np.int32))
    got = _check([room], [(1.0, 1.0, 1.0)], 1024, 402, [1])
    assert 0 < got["scattered"][0] <= got["points"][0] // 2


# ---- 5. nothing is kept between calls -------------------------------------------------------------------------------------------------------------
def test_two_centres_one_room(backend):
    """Two consecutive calls on one stream over the same room with centres at opposite ends: the buckets flagged for the first call mean nothing to the second"""
    rng = np.random.default_rng(501)
    room = _room(rng, _box(rng, 100000, (10.0, 4.0, 2.5)))
    c1, c2 = (1.0, 1.0, 1.2), (9.2, 3.1, 1.0)
    got1 = _fused([room], [c1], 1024, 502)
    got2 = _fused([room], [c2], 1024, 503)
    _same(got1, [room], [c1], 1024, 502, [1])
    _same(got2, [room], [c2], 1024, 503, [1])
    for g in (got1, got2):
        assert 0 < g["scattered"][0] < g["points"][0] // 2
    assert not np.array_equal(got1["xyz"], got2["xyz"])
