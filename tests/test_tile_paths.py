"""The tile generator (csrc/tile.hip, csrc/tile_body.hpp; the single flavour's sort: csrc/radix_sort.hip) branch by branch against the stable-sort oracle:
source rows index for index, xyz / features / labels bit for bit.  DESIGN.md section 20 lists the branches with the case that reaches each.  Every case runs
on the CPU logic build and on the gfx950 build with the same inputs, and asserts its input condition with tests/_tile_paths.py: plan() (a NumPy restatement of
tile_hist_b / tile_thresh_b: threshold bin, candidates, sort ranges) or varying_bytes() (the executed digit passes) BEFORE the library is called: a case
cannot pass without having reached the branch it names.

The oracle is the project's float32 convention (key (dx*dx + dy*dy) + dz*dz in float32, stable argsort, ties by index); test_nearest_in_float64 ties it to
float64 distances.

The room that reaches tile_compact_bins_b: the launcher takes that kernel for rstride = (maxn + 1023) / 1024 + 1 > TS_RMAX = 2048, i.e. from maxn = 2047 * 1024
+ 1 = 2 096 129 rows on.  A room of 2 095 105 rows (2046 * 1024 + 1) gives rstride = 2048 and is the LAST size on tile_compact_b, with every one of its 2048 LDS
counters in the table; both sizes are cases (test_large_room).

Measured on one MI355X: `pytest -m gpu tests/test_tile_paths.py` = 44 tests in 1.1 s, the two large rooms at 0.2 s each (inputs and oracle built once per
size and shared with the state tests); every case agrees with the CPU logic build, whose leg (`-m "not gpu"`, 44 tests) takes 4 s.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal
import _tile_paths as TP
from _tile_paths import F32, check_batch, constants, make_call, plan, rstride, run_batch, run_single, same_results, same_tile, untouched

ORIGIN = np.zeros(3, F32)


def _one_bin_call(seed, n, N):
    rng = np.random.default_rng(seed)
    return make_call(rng, [TP.one_bin_room(rng, n)], [ORIGIN], N)


# ---- 1. tile_binsort_b: the four networks and their edges ---------------------------------------------------------------------------------------------
BINSORT = [(1, "none"), (2, "lds"), (8, "lds"),                                               # generic network in LDS, N < 16
           (9, "registers"), (16, "registers"), (17, "registers"), (1024, "registers"), (1025, "registers"), (2048, "registers"),
           (2049, "lds"), (4096, "lds"),                                                         # generic network in LDS, N = 4096
           (4097, "global"), (9000, "global")]                                                   # in place in global memory


@pytest.mark.parametrize("n,path", BINSORT, ids=["n%d_%s" % x for x in BINSORT])
def test_binsort_network(backend, n, path):
    """A room of n rows in ONE distance bin (exact ties in pairs) is one sort range of n words, whatever the tile size: num_points = n and n // 2."""
    for N in sorted({n, max(1, n // 2)}):
        call = _one_bin_call(100 + n, n, N)
        p = plan(call.rooms[0], ORIGIN, N, n)
        assert p.ranges == [n] and p.paths == [path] and p.cand == n and p.holes == list(range(1, p.nk)), (p.ranges, p.paths, p.holes)
        check_batch(call, run_batch(call), what="n %d, num_points %d, room" % (n, N))


def test_binsort_hole_in_range_table(backend):
    """Two crowded bins: 2500 rows at r^2 in [4, 4.0625) and 3000 at 2.25 times that: the second bin starts at 2500 (range 2); entries 1, 3, 4, 5 of the range
    table stay 0xffffffff, and the two ranges are cut at the bin boundary."""
    rng = np.random.default_rng(120)
    room = np.concatenate([TP.one_bin_room(rng, 2500), TP.one_bin_room(rng, 3000, 1.5)])[rng.permutation(5500)]
    call = make_call(rng, [room], [ORIGIN], 5000)
    p = plan(room, ORIGIN, 5000, 5500)
    assert p.ranges == [2500, 3000] and p.paths == ["lds", "lds"] and p.nk == 6 and p.holes == [1, 3, 4, 5] and len(p.bins) == 2, vars(p)
    check_batch(call, run_batch(call))


# ---- 2. the large room: tile_compact_bins_b, the range loop's second trip --------------------------------------------------------------------------------
_LARGE = {}


def _large_call(n):
    """a room of n uniform rows in a 40 x 30 x 3 box, num_points = 70 000, and a 3000-row room in the same call; built once, with its oracle"""
    if n not in _LARGE:
        rng = np.random.default_rng(2000)
        big = (rng.random((n, 3), dtype=F32) * np.array([40, 30, 3], F32)).astype(F32)
        small, c_small = TP.box_room(rng, 3000)
        call = make_call(rng, [big, small], [np.array([20.1, 14.9, 1.4], F32), c_small], 70000, colors=False)
        _LARGE[n] = (call, TP.expected(call), plan(big, call.centres[0], 70000, n))
    return _LARGE[n]


LARGE = [(2046 * 1024 + 1, False), (2047 * 1024 + 1, True)]


@pytest.mark.parametrize("n,bins", LARGE, ids=["rows%d_%s" % (n, "compact_bins" if b else "compact_last") for n, b in LARGE])
def test_large_room(backend, n, bins):
    """More than 64 sort ranges in one room (tile_binsort_b's workgroups take a second trip of `q += gridDim.x`), at the two sizes around rstride = TS_RMAX:
    the last room tile_compact_b takes (all TS_RMAX counters of a workgroup in the table) and the first that goes to tile_compact_bins_b, where the 3000-row
    room of the same call goes with it (a room smaller than the tile: the padding map beside the per-bin cursors)."""
    k = constants()
    call, exp, p = _large_call(n)
    assert (rstride(call.sizes) > k.TS_RMAX) == bins and rstride(call.sizes) == k.TS_RMAX + (1 if bins else 0), rstride(call.sizes)
    assert p.nk > 64 and len(p.ranges) > 64 and p.cand > 65536 and set(p.paths) == {"registers"}, (p.nk, len(p.ranges), p.cand)
    check_batch(call, run_batch(call), exp)


# ---- 3. many rooms: xcd_tile_map on and off, device counts below the host's bound ------------------------------------------------------------------------
SIZES8 = (5000, 300, 1000, 999, 1001, 7000, 2500, 1)
COUNTS8 = (4000, 300, 500, 998, 1001, 7000, 1000, 1)


def _rooms(seed, sizes, counts=None):
    """uniform rooms; with counts: the rows from counts[r] on lie ON the centre, closer than any valid row"""
    rng = np.random.default_rng(seed)
    rooms, centres = [], []
    for r, n in enumerate(sizes):
        p, c = TP.box_room(rng, n)
        if counts is not None:
            p[counts[r]:] = c
            assert TP.keys(p[:counts[r]], c).min() > 0 and (TP.keys(p[counts[r]:], c) == 0).all()
        rooms.append(p); centres.append(c)
    return rng, rooms, centres


MANY = [(8, 1000), (7, 1000), (16, 7), (64, 300), (8, 100), (7, 100)]


@pytest.mark.parametrize("R,N", MANY, ids=["R%d_N%d" % x for x in MANY])
def test_many_rooms(backend, R, N):
    """Room counts that are multiples of 8 (tile_gather_b deals a room's workgroups to one XCD; N = 7: a gather grid one block wide; N = 1000: four blocks)
    and R = 7 on the same rooms (the identity); rooms larger than, equal to and smaller than the tile, one of a single row; num_points that is no multiple of
    256 and below 256 (tile_padmap_body's stretches); dup_u = 0 and 1.0 in the last rows of every room."""
    sizes = (SIZES8 * 8)[:R]
    rng, rooms, centres = _rooms(300, sizes)
    call = make_call(rng, rooms, centres, N)
    assert ((R & 7) == 0) == (R != 7) and call.dup[0, -1] == 1.0 and call.dup[0, -2] == 0.0
    check_batch(call, run_batch(call))


@pytest.mark.parametrize("N", [1000, 100])
def test_device_counts_below_host_bound(backend, N):
    """d_m[r] < the host's row bound, in both directions across num_points; the rows beyond d_m[r] lie on the centre: a kernel that read one would put it first."""
    rng, rooms, centres = _rooms(310, SIZES8, COUNTS8)
    call = make_call(rng, rooms, centres, N, m=COUNTS8)
    assert all(m <= n for m, n in zip(COUNTS8, SIZES8)) and sum(m < n for m, n in zip(COUNTS8, SIZES8)) == 4
    # a bound at or above the tile with a count below it, and a count that stays above the tile
    assert N != 1000 or (any(n >= N > m for m, n in zip(COUNTS8, SIZES8)) and any(n > m > N for m, n in zip(COUNTS8, SIZES8)))
    check_batch(call, run_batch(call))


def test_nearest_in_float64(backend):
    """The float32 oracle against float64 distances, on the R = 8 rooms: for every full tile (m > N), the largest float64 squared distance of the tile's rows
    <= the smallest of the room's other rows * (1 + g) / (1 - g), g = 6 * 2^-24.

    Derivation: a float32 key is ((dx^2 + dy^2) + dz^2) with dx = fl(x - cx): the rounding of the difference enters its square twice, the square rounds once,
    and the two additions round once each: every term, all of them non-negative, carries at most five factors (1 + e), |e| <= 2^-24, so key = d (1 + t) with
    |t| <= (1 + 2^-24)^5 - 1 < 6 * 2^-24 = g for the exact squared distance d.  A row i inside the tile and a row j outside have key_i <= key_j, hence
    d_i (1 - g) <= key_i <= key_j <= d_j (1 + g).  (Measured on the CPU over 20 rooms of 200 000 points: the float32 keys deviate by at most 4.7 * 2^-24.)"""
    N, g = 1000, 6.0 * 2.0 ** -24
    rng, rooms, centres = _rooms(300, SIZES8)
    call = make_call(rng, rooms, centres, N)
    got = run_batch(call)
    full = [r for r in range(8) if call.m[r] > N]
    assert len(full) == 4
    for r in full:
        d = ((rooms[r].astype(np.float64) - centres[r].astype(np.float64)[None]) ** 2).sum(1)
        rows = got["idx"][r]
        assert len(set(rows.tolist())) == N and rows.min() >= 0 and rows.max() < call.m[r]
        rest = np.setdiff1d(np.arange(call.m[r]), rows)
        far, near = d[rows].max(), d[rest].min()
        print("room %d: tile max %.9g, rest min %.9g, ratio - 1 = %.3g (bound %.3g)" % (r, far, near, far / near - 1, (1 + g) / (1 - g) - 1))
        assert far <= near * (1 + g) / (1 - g), "room %d" % r


# ---- 4. ties, +inf, identical rows ---------------------------------------------------------------------------------------------------------------------
def test_ties_inf_and_identical_rows(backend):
    """A 17^3 lattice around its centre (exact ties across every bin's range; also cut to 2000 rows by d_m: a small room with ties), 3000 lattice rows + 50 at
    coordinates 1e20 (the square overflows: +inf keys, 40 of them inside the tile, by index), 5000 identical rows with the centre on them (bin 0) and off them
    (one far bin): one range of 5000 words either way."""
    rng = np.random.default_rng(400)
    lat = TP.lattice(rng, 17, 0.25)
    call = make_call(rng, [lat, lat], [ORIGIN, ORIGIN], 4000, m=[len(lat), 2000])
    assert len(lat) == 4913 and len(np.unique(TP.keys(lat, ORIGIN))) < 400
    check_batch(call, run_batch(call), what="lattice")

    room = np.concatenate([lat[:3000], np.full((50, 3), 1e20, F32)])[rng.permutation(3050)]
    key = TP.keys(room, ORIGIN)
    assert np.isinf(key).sum() == 50 and not np.isnan(key).any()
    call = make_call(rng, [room], [ORIGIN], 3040)
    got = run_batch(call)
    check_batch(call, got, what="lattice and +inf")
    assert np.isinf(key[got["idx"][0]]).sum() == 40

    same = np.tile(np.array([[1.5, -2.25, 0.75]], F32), (5000, 1))
    call = make_call(rng, [same, same], [same[0], np.array([9.0, 4.0, -3.0], F32)], 1000)
    p0, p1 = plan(same, call.centres[0], 1000, 5000), plan(same, call.centres[1], 1000, 5000)
    assert p0.bins == [0] and p0.ranges == [5000] and len(p1.bins) == 1 and p1.bins[0] > 8000 and p1.paths == ["global"], (vars(p0), vars(p1))
    check_batch(call, run_batch(call), what="identical rows")


# ---- 5. per-stream state ----------------------------------------------------------------------------------------------------------------------------------
def _sequence(stream):
    rng = np.random.default_rng(500)
    a = make_call(rng, [TP.one_bin_room(rng, 9000)], [ORIGIN], 6000)
    rng, rooms, centres = _rooms(510, SIZES8)
    b = make_call(rng, rooms, centres, 100)
    big, exp_big, p = _large_call(LARGE[1][0])
    k = constants()
    assert plan(a.rooms[0], ORIGIN, 6000, 9000).paths == ["global"] and rstride(a.sizes) != rstride(b.sizes) and rstride(big.sizes) > k.TS_RMAX
    first = run_batch(a, stream=stream)
    got_b = run_batch(b, stream=stream)
    got_big = run_batch(big, stream=stream)
    second = run_batch(a, stream=stream)
    exp_a = check_batch(a, first, what="call A, room")
    check_batch(b, got_b, what="call B, room")
    check_batch(big, got_big, exp_big, what="the large-room call, room")
    check_batch(a, second, exp_a, what="call A again, room")
    same_results(first, second, "call A against its repetition")


def test_state_reuse_on_the_library_stream(backend):
    """Calls of different shape on one stream: A (9000 rows in one bin, num_points 6000), B (eight rooms, num_points 100), the large room (tile_compact_bins_b
    leaves the histogram as cursors), A again: the histogram is clear for every call, rstart / rcur are rebuilt over another rstride, the padding map is
    shared: every result equals the oracle, A's second bit for bit its first."""
    _sequence(None)


def test_state_reuse_on_a_callers_stream(backend):
    """The same on a stream of the caller's: copies and calls ordered on that stream alone."""
    from ssdr_al import _lib
    L = _lib.lib()
    s = C.c_void_p()
    _lib.check(L.ssdr_stream_create(C.byref(s)))
    try:
        _sequence(s.value)
    finally:
        _lib.check(L.ssdr_stream_destroy(s.value))


# ---- 6. optional arguments, refused arguments, the empty room ------------------------------------------------------------------------------------------------
def _small_call(seed=600, N=300, **kw):
    rng, rooms, centres = _rooms(seed, (1000, 200, 300))
    return make_call(rng, rooms, centres, N, **kw)


def test_null_outputs(backend):
    """out_feat, out_idx, out_labels NULL one at a time, and the colours NULL with color_dim 0 (features = the centred xyz): what remains equals the full call."""
    call = _small_call()
    full = run_batch(call)
    exp = check_batch(call, full)
    for off_name in ("feat", "idx", "lab"):
        got = run_batch(call, **{off_name: False})
        assert got[off_name] is None
        check_batch(call, got, exp, what="without %s, room" % off_name)
        for name in got:
            if name != off_name:
                assert_bits_equal(got[name], full[name], "without %s: %s" % (off_name, name))
    got = run_batch(call, colors=False)
    assert got["feat"].shape[-1] == 3
    check_batch(call, got, exp, what="without colours, room")
    assert_bits_equal(got["feat"], full["feat"][..., :3], "without colours: features")
    assert_bits_equal(got["feat"], got["xyz"], "without colours: features are the centred xyz")


def test_refused_arguments(backend):
    """SSDR_ERR_INVALID and nothing launched (the prefilled outputs untouched): 65 rooms, out_labels without labels, out_feat with color_dim > 0 and no colours,
    an offset that does not increase, num_points 0."""
    call = _small_call()
    rng = np.random.default_rng(610)
    many = make_call(rng, [rng.random((10, 3), dtype=F32) for _ in range(TP.MAX_ROOMS + 1)], np.zeros((TP.MAX_ROOMS + 1, 3), F32), 8)
    flat = call.off.copy()
    flat[2] = flat[1]
    for what, c, kw in (("65 rooms", many, {}), ("labels missing", call, dict(labels_in=False, lab=True)), ("colours missing", call, dict(colors=False, cdim=3)),
                        ("flat offsets", call, dict(off=flat)), ("num_points 0", call, dict(N=0))):
        got = run_batch(c, expect=TP.ERR_INVALID, **kw)
        for r in range(len(c.rooms)):
            untouched(got, r, what)
    check_batch(call, run_batch(call), what="after the refused calls, room")


def test_empty_room(backend):
    """d_m = (0, 500, 0): the empty rooms' output rows stay as they were (no sort word, point, colour or label of theirs is read), room 1 equals the oracle;
    the single flavour with d_m = 0 likewise, its possibility map untouched."""
    rng, rooms, centres = _rooms(620, (400, 500, 1))
    call = make_call(rng, rooms, centres, 300, m=[0, 500, 0])
    exp = TP.expected(call)
    assert exp[0] is None and exp[2] is None and plan(rooms[0], centres[0], 300, 0).cand == 0
    check_batch(call, run_batch(call), exp)
    call = make_call(rng, rooms, centres, 700, m=[0, 500, 0])           # ... and with room 1 smaller than the tile
    check_batch(call, run_batch(call))
    poss = rng.random(400)
    for plain in (False, True):
        got = run_single(rooms[0], call.col[:400], centres[0], 300, 0, call.perm[0, :300].copy(), call.dup[0, :300].copy(), None if plain else poss, plain=plain)
        untouched(got, None, "single flavour, d_m = 0")
        assert plain or np.array_equal(got["poss"], poss)


# ---- 7. the single flavour: executed digit passes, sort-tile edges, the possibility map -------------------------------------------------------------------------
def _single(rng, pts, centre, N, m=None, what=""):
    m = len(pts) if m is None else m
    col = rng.integers(0, 256, (len(pts), 3)).astype(F32)
    perm, dup = rng.permutation(N).astype(np.int32), rng.random(N).astype(F32)
    dup[-1] = 1.0
    got = run_single(pts, col, centre, N, m, perm, dup)
    same_tile(got, TP.oracle_tile(pts, col, None, centre, N, m, perm, dup), "%s num_points %d" % (what, N))


def _digit_room(rng, name):
    if name == "identical":
        return np.tile(np.array([[3.0, 4.0, 12.0]], F32), (3000, 1)), set()
    if name == "byte2":
        return TP.integer_room(rng, 128, 256), {2}
    if name == "bytes12":
        return TP.integer_room(rng, 32768, 65536, unit=8), {1, 2}
    if name == "bytes012":
        return TP.integer_room(rng, 65536, 131072, stride=11), {0, 1, 2}
    p = (rng.random((3000, 3), dtype=F32) * F32(8) - F32(4)).astype(F32)
    p[0] = (0.001, 0.0, 0.0)
    return p, {0, 1, 2, 3}


@pytest.mark.parametrize("name", ["identical", "byte2", "bytes12", "bytes012", "random"])
def test_single_digit_passes(backend, name):
    """0, 1, 2, 3 and 4 executed digit passes of the radix sort (rs_andor skips a pass whose byte is the same in every key; rs_finish copies the result home
    after an odd number): rows with integer coordinates whose squared distances are exact integers of one binade, a third of them duplicated (ties by index);
    num_points below, at and above the row count."""
    rng = np.random.default_rng(700)
    pts, want = _digit_room(rng, name)
    assert TP.varying_bytes(pts, ORIGIN) == want, TP.varying_bytes(pts, ORIGIN)
    n = len(pts)
    for N in (64, n, n + 77):
        _single(rng, pts, ORIGIN, N, what=name)


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 4096])
def test_single_sort_tile_edges(backend, n):
    """Row counts around the 2048-pair sort tile, num_points = n and n // 3."""
    rng = np.random.default_rng(710 + n)
    pts, c = TP.box_room(rng, n)
    for N in sorted({n, max(1, n // 3)}):
        _single(rng, pts, c, N, what="n %d" % n)


POSS_M = [20000, 12345, 3000]


@pytest.mark.parametrize("m", POSS_M)
def test_possibility_map_and_minimum(backend, m):
    """20 000 rows, num_points 4096, the map's minimum -1.0 at rows 5, 1029 and 7000 (rows 5 and 1029 fall to the same thread of possibility_min's 1024, row 7000
    to another), all three far from the centre and mirror images of one another (equal keys): d_m = 20 000 and 12 345 leave them outside the tile, d_m = 3000
    (smaller than the tile: avail = m, dmax = the farthest row) raises rows 5 and 1029 by the SAME amount: the minimum stays tied, the arg-min is the first.
    Map, minimum and arg-min bit for bit; ssdr_tile_select_dev gives the same tile with no map."""
    rng = np.random.default_rng(720)
    n, N = 20000, 4096
    pts = (rng.random((n, 3), dtype=F32) * np.array([8, 6, 3], F32) - np.array([4, 0, 0], F32)).astype(F32)
    centre = np.array([0.0, 3.1, 1.4], F32)
    pts[5] = (-3.96875, 0.5, 0.25)
    pts[1029] = pts[7000] = (3.96875, 0.5, 0.25)
    poss = rng.random(n) * 1e-3
    poss[[5, 1029, 7000]] = -1.0
    key = TP.keys(pts, centre)
    assert key[5] == key[1029] == key[7000]
    col = rng.integers(0, 256, (n, 3)).astype(F32)
    perm, dup = rng.permutation(N).astype(np.int32), rng.random(N).astype(F32)
    exp = TP.oracle_tile(pts, col, None, centre, N, m, perm, dup)
    exp_map, exp_min, exp_arg = TP.oracle_possibility(pts, centre, N, m, poss)
    in_tile = {5, 1029, 7000} & set(exp["idx"].tolist())
    assert in_tile == ({5, 1029} if m == 3000 else set()) and exp_arg == 5 and exp_map[5] == exp_map[1029] == exp_min
    assert (exp_min == -1.0) == (m != 3000)
    got = run_single(pts, col, centre, N, m, perm, dup, poss)
    same_tile(got, exp, "d_m %d" % m)
    assert np.array_equal(got["poss"], exp_map), "possibility map"
    assert got["min"] == exp_min and got["arg"] == exp_arg, (got["min"], got["arg"], exp_min, exp_arg)
    plain = run_single(pts, col, centre, N, m, perm, dup, plain=True)
    for name in ("xyz", "feat", "idx"):
        assert_bits_equal(plain[name], got[name], "ssdr_tile_select_dev %s" % name)
