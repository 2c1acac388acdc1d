"""The vote / feed generator (csrc/vote.hip; entries ssdr_vote_init_dev, ssdr_vote_tiles_dev, ssdr_feed_chain_dev, ssdr_feed_tiles_dev, ssdr_feed_status) branch by
branch against the stable-sort oracle (tests/_vote_oracle.py, tests/_feed_oracle.py: float32 key (dx*dx + dy*dy) + dz*dz, argsort(kind="stable"), a float64 map,
np.argmin's first minimum).  vote.hip has its own histogram / threshold / compaction / sort chain and kernels that exist nowhere else (vote_pick, vote_min_part,
vote_min_fin, vote_place, the weighted update of vote_gather); DESIGN.md section 23 lists the branches with the case that reaches each.

Every case runs on the CPU logic build and on the gfx950 build with the same inputs, and asserts its input condition with the predictors of tests/_vote_paths.py
(and _tile_paths.plan, which describes vote_thresh too) BEFORE the library is called: a case that no longer reaches its branch fails.  Everything is compared bit
for bit: cloud ids, centres, row numbers, xyz, features, labels, channels, the float64 map, and cloud_min / cloud_arg after every call.  No case has a tolerance.
Every chain tile has a finite, positive largest key (dmax = 0 or inf makes the reference's own update NaN: out of scope, and asserted away).

The sizes: vote_compact_bins starts at rstride = (maxn + 1023) / 1024 + 1 > TS_RMAX, i.e. at a largest cloud of 2047 * 1024 + 1 rows; vote_min_part's chunk stride
starts above VM_MAXPART * VM_CHUNK rows in the chain and above 64 * VM_CHUNK rows in ssdr_vote_init_dev.

Measured: CPU leg (`-m "not gpu"`) 30 tests in 5.6 s, the three two-million-row cases 1.4 - 1.6 s each (inputs and oracle included, built once per size and
shared with the state tests); on one MI355X `pytest -m gpu tests/test_vote_paths.py` = 29 tests in 2.6 s, those three at 0.45 - 0.7 s; every case agrees with
the CPU logic build.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import _tile_paths as TP
import _vote_paths as VP
from _tile_paths import F32
from _vote_paths import GLOBAL_ROWS, XY_ONLY, Table, chain_oracle, chain_reference, compare, compare_state, constants, make_draws, make_table, tile_plans

ORIGIN = np.zeros(3, F32)


def _flat_map(rng, table, base=0.0):
    """init_possibility's map: random * 1e-3 (+ base)"""
    return [base + rng.random(n) * 1e-3 for n in table.sizes]


def _chain(table, poss, N, batches, rng, check=None, centre=None, flags=GLOBAL_ROWS, weights=None, oracle_weights=None, entry="feed", noise_scale=0.35, stream=None,
           what="", **kw):
    """a table and a map through `batches` calls of the chain (B tiles each): the oracle steps first, the case's condition (`check(call, plans, ref, state)`) is
    asserted on the oracle's tiles, then the library runs the same draws; outputs, map, cloud_min and cloud_arg after every call.  -> [(got, ref, state)]"""
    channels = kw.get("channels", True) and entry != "vote"
    gen = chain_oracle(table, poss, N, flags, weights if oracle_weights is None else oracle_weights, channels)
    dev = Table(table, poss, stream=stream)
    compare_state(dev, VP.oracle_state(gen), what + " after ssdr_vote_init_dev:")
    out = []
    for k, B in enumerate(batches):
        draws = make_draws(rng, B, N, noise_scale)
        ref, state = chain_reference(gen, table, draws, centre)
        plans = tile_plans(table, ref, N)
        VP.assert_update_defined(plans)
        if check is not None:
            check(k, plans, ref, state)
        got = dev.chain(draws, N, flags, weights, entry=entry, **kw)
        compare(got, ref, "%s call %d:" % (what, k))
        compare_state(dev, state, "%s call %d:" % (what, k))
        out.append((got, ref, state))
    return out


def _indep(table, N, tile_cloud, tile_point, rng, check=None, centre=None, stream=None, what="tiles"):
    """independent tiles: the oracle, the case's condition on its tiles, the library"""
    draws = make_draws(rng, len(tile_cloud), N)
    if centre is not None:
        for t, (c, p) in enumerate(zip(tile_cloud, tile_point)):
            draws["noise"][t] = VP.towards(table, c, p, centre)
    ref = VP.indep_reference(table, tile_cloud, tile_point, draws, N)
    if check is not None:
        check(0, tile_plans(table, ref, N), ref, None)
    got = Table(table, stream=stream).tiles(tile_cloud, tile_point, draws, N)
    compare(got, ref, what + ":")
    return got, ref


# ---- 0. the predictors themselves -------------------------------------------------------------------------------------------------------------------------
def test_constants_and_predictors():
    k = constants()
    assert (k.TS_RCAP, k.TS_RSTEP) == (TP.constants().TS_RCAP, TP.constants().TS_RSTEP)
    assert [VP.sort_path(n) for n in (0, 1, 2, k.TS_RCAP, k.TS_RCAP + 1)] == ["none", "none", "lds", "lds", "global"]
    assert VP.rstride(1) == 2 and VP.rstride(k.TS_RSTEP) == 2 and VP.rstride(k.TS_RSTEP + 1) == 3
    assert VP.vm_grid(1) == 1 and VP.vm_grid(k.VM_CHUNK + 1) == 2 and VP.vm_grid(k.VM_MAXPART * k.VM_CHUNK + 1) == k.VM_MAXPART
    assert VP.init_grid(VP.INIT_GRID_CAP * k.VM_CHUNK) == VP.INIT_GRID_CAP == VP.init_grid(10 ** 7)
    assert VP.compact_passes(VP.COMPACT_GRID_CAP * VP.BLOCK * k.TS_CPT) == 1 and VP.compact_passes(VP.COMPACT_GRID_CAP * VP.BLOCK * k.TS_CPT + 1) == 2


# ---- 1. vote_sort: none, the LDS network at its ends, in place in global memory ---------------------------------------------------------------------------
SORT = [(1, "none"), (2, "lds"), (3, "lds"), (17, "lds"), (1025, "lds"), (4096, "lds"), (4097, "global"), (9000, "global")]


@pytest.mark.parametrize("n,path", SORT, ids=["n%d_%s" % x for x in SORT])
def test_sort_network(backend, n, path):
    """A cloud of n rows in ONE distance bin around the origin (exact ties in pairs), every tile's centre put on the origin by its noise: one sort range of n
    words whatever the tile size; num_points = n and n // 2, a chain tile (ssdr_vote_tiles_dev) and an independent tile each."""
    rng = np.random.default_rng(100 + n)
    table = make_table(rng, [TP.one_bin_room(rng, n)])
    poss = _flat_map(rng, table)

    def check(k, plans, ref, state):
        for p, c in zip(plans, ref["center"]):
            assert not c.any() and p.ranges == [n] and p.cand == n and VP.sort_path(p.ranges[0]) == path and p.holes == list(range(1, p.nk)), vars(p)

    for N in sorted({n, max(1, n // 2)}):
        _chain(table, poss, N, [1], rng, check, centre=ORIGIN, entry="vote", what="n %d, num_points %d" % (n, N))
        _indep(table, N, [0], [int(rng.integers(n))], rng, check, centre=ORIGIN, what="n %d, num_points %d, independent" % (n, N))


def test_sort_identical_rows(backend):
    """5000 identical rows and a non-zero noise: every key equal (one far bin, one range of 5000 words: in place in global memory, ties by row alone), every
    quotient d / dmax = 1: the update adds 0 to every row, and the second tile starts from the same row as the first."""
    rng = np.random.default_rng(130)
    table = make_table(rng, [np.tile(np.array([[1.5, -2.25, 0.75]], F32), (5000, 1))])
    poss = _flat_map(rng, table)

    def check(k, plans, ref, state):
        for p in plans:
            assert len(p.bins) == 1 and p.bins[0] > 0 and p.ranges == [5000] and VP.sort_path(5000) == "global" and p.dmax > 0, vars(p)
        assert np.array_equal(state[0], np.concatenate(poss))

    _chain(table, poss, 1000, [2], rng, check, what="identical rows")


# ---- 2. a hole in the range table ---------------------------------------------------------------------------------------------------------------------------
def _hole_table(rng):
    """two crowded bins, as in test_tile_paths.test_binsort_hole_in_range_table: 2500 rows at r^2 in [4, 4.0625) and 3000 at 2.25 times that"""
    return make_table(rng, [np.concatenate([TP.one_bin_room(rng, 2500), TP.one_bin_room(rng, 3000, 1.5)])[rng.permutation(5500)]])


def _hole_check(k, plans, ref, state):
    for p in plans:
        assert p.ranges == [2500, 3000] and p.nk == 6 and p.holes == [1, 3, 4, 5] and len(p.holes) > 0 and len(p.bins) == 2, vars(p)


def test_hole_in_range_table(backend):
    """The second bin starts at 2500 (range 2): entries 1, 3, 4, 5 of rstart stay 0xffffffff; vote_sort skips them and scans for the next live entry."""
    rng = np.random.default_rng(120)
    table = _hole_table(rng)
    _chain(table, _flat_map(rng, table), 5000, [2], rng, _hole_check, centre=ORIGIN, entry="vote", what="hole")
    _indep(table, 5000, [0, 0], [17, 4000], rng, _hole_check, centre=ORIGIN, what="hole, independent")


# ---- 3. the range loop's second trip (a production path: a Semantic3D tile of 65 536 points) -----------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["s3dis", "semantic3d"])
def test_sort_range_loop_second_trip(backend, flavour):
    """num_points 66 000 from a uniform cloud of 100 000 rows: more than 64 entries in the range table, so vote_sort's 64 workgroups take a second trip of
    `q += gridDim.x`; 100 000 rows are also more than vote_hist's 64 workgroups cover in one pass.  S3DIS: ssdr_vote_tiles_dev; Semantic3D: x / y centred only,
    the weighted update, both channels, cloud-local rows."""
    rng = np.random.default_rng(140)
    table = make_table(rng, [(rng.random((100000, 3), dtype=F32) * np.array([40, 30, 3], F32)).astype(F32)])
    weights = rng.random(8) + 0.1

    def check(k, plans, ref, state):
        for p in plans:
            assert p.nk > VP.SORT_GRID_CAP and len(p.ranges) > VP.SORT_GRID_CAP and p.cand >= 66000, (p.nk, len(p.ranges), p.cand)
        assert table.maxn > VP.HIST_GRID_CAP * VP.BLOCK and VP.rstride(table.maxn) <= constants().TS_RMAX

    if flavour == "s3dis":
        _chain(table, _flat_map(rng, table), 66000, [2], rng, check, entry="vote", what=flavour)
    else:
        _chain(table, _flat_map(rng, table), 66000, [2], rng, check, flags=XY_ONLY, weights=weights, what=flavour)


# ---- 4. the large clouds: vote_compact's last size and its second pass, vote_compact_bins, vote_min_part under VM_MAXPART -----------------------------------
LARGE_N = 4096
_LARGE = {}


def _large(n):
    """a cloud of n uniform rows in a 40 x 30 x 3 box and a 3000-row cloud (smaller than the tile) in one table, num_points 4096: the map sends the first chain
    tile to the large cloud and the second to the small one; two independent tiles, one per cloud.  Built once, with its oracle."""
    if n not in _LARGE:
        rng = np.random.default_rng(2000)
        big = (rng.random((n, 3), dtype=F32) * np.array([40, 30, 3], F32)).astype(F32)
        small, _ = TP.box_room(rng, 3000)
        table = make_table(rng, [big, small])
        poss = _flat_map(rng, table, 1e-3)
        poss[0][n // 3] = 0.0
        poss[1][77] = 0.5e-3
        gen = chain_oracle(table, poss, LARGE_N, GLOBAL_ROWS, None, False)
        draws = make_draws(rng, 2, LARGE_N)
        ref, state = chain_reference(gen, table, draws)
        tc, tp = [0, 1], [int(rng.integers(n)), int(rng.integers(3000))]
        idraws = make_draws(rng, 2, LARGE_N)
        _LARGE[n] = SimpleNamespace(table=table, poss=poss, draws=draws, ref=ref, state=state, plans=tile_plans(table, ref, LARGE_N), tc=tc, tp=tp, idraws=idraws,
                                    iref=VP.indep_reference(table, tc, tp, idraws, LARGE_N))
    return _LARGE[n]


LARGE = [(2046 * 1024 + 1, False), (2047 * 1024 + 1, True)]


@pytest.mark.parametrize("n,bins", LARGE, ids=["rows%d_%s" % (n, "compact_bins" if b else "compact_last") for n, b in LARGE])
def test_large_cloud(backend, n, bins):
    """The two sizes around rstride = TS_RMAX: the last table vote_compact takes (all TS_RMAX LDS counters in use; its 256 workgroups take a second pass) and the
    first that goes to vote_compact_bins, where the 3000-row cloud's tile goes with it (the branch follows the table's largest cloud)."""
    k = constants()
    L = _large(n)
    assert VP.rstride(L.table.maxn) == k.TS_RMAX + (1 if bins else 0) and (VP.rstride(L.table.maxn) > k.TS_RMAX) == bins
    assert VP.compact_passes(L.table.maxn) >= 2
    assert L.ref["cloud"].tolist() == [0, 1] and L.table.sizes[1] < LARGE_N
    VP.assert_update_defined(L.plans)
    dev = Table(L.table, L.poss)
    got = dev.chain(L.draws, LARGE_N, GLOBAL_ROWS, channels=False)
    compare(got, L.ref, "chain:")
    compare_state(dev, L.state, "chain:")
    compare(dev.tiles(L.tc, L.tp, L.idraws, LARGE_N), L.iref, "independent:")


def test_min_part_stride_under_vm_maxpart(backend):
    """A cloud of VM_MAXPART x VM_CHUNK + 1 rows: vote_min_part's workgroup 0 takes chunk VM_MAXPART, which holds the last row alone, on its second trip.
    Tile 1 starts from row P (0.0 in a map of values >= 1); after it the minimum 0.5 sits in row E (chunk 3) and in the last row L: the first must win.  Tile 2
    therefore starts from E, after it the last row alone holds the minimum.  Tile 3 starts from L, after it an earlier row (0.75) holds it."""
    k = constants()
    n = k.VM_MAXPART * k.VM_CHUNK + 1
    rng = np.random.default_rng(150)
    pts = (rng.random((n, 3), dtype=F32) * np.array([40, 30, 3], F32)).astype(F32)
    P, E, E2, Lr = n // 2 + 11, 3 * k.VM_CHUNK + 7, 500 * k.VM_CHUNK + 300, n - 1
    pts[P], pts[E], pts[E2], pts[Lr] = (5, 5, 1.5), (35, 25, 1.5), (35, 5, 1.5), (5, 25, 1.5)
    table = make_table(rng, [pts])
    poss = _flat_map(rng, table, 1.0)
    poss[0][P], poss[0][E], poss[0][Lr], poss[0][E2] = 0.0, 0.5, 0.5, 0.75
    assert VP.chunks(n) == k.VM_MAXPART + 1 and VP.vm_grid(n) == k.VM_MAXPART and Lr // k.VM_CHUNK == k.VM_MAXPART
    starts, after = [P, E, Lr], [(0.5, E), (0.5, Lr), (0.75, E2)]

    def check(c, plans, ref, state):
        assert (state[1][0], int(state[2][0])) == after[c], (c, state[1], state[2])
        touched = set((ref["idx"][0]).tolist())
        assert starts[c] in touched and not touched & (set(starts[c + 1:]) | {E2}), c
        if c == 0:
            assert state[0][E] == state[0][Lr] == 0.5

    _chain(table, poss, 4096, [1, 1, 1], rng, check, entry="vote", noise_scale=0.05, what="VM_MAXPART")


# ---- 5. ssdr_vote_init_dev under its cap of 64 workgroups per cloud -------------------------------------------------------------------------------------------
def test_init_min_under_grid_cap(backend):
    """Clouds of 64 x VM_CHUNK + 1, 1, 2049 and 5000 rows: gx = 64, so the largest cloud's workgroup 0 takes chunk 64 (the last row alone) on a second trip, and
    cloud y's partials lie at y * gx + x.  Minima in last rows; equal minima across a workgroup's trips, across workgroups, across threads of a chunk, and inside
    one thread (rows 256 apart): cloud_min and cloud_arg are np.min and np.argmin's first minimum."""
    k = constants()
    sizes = [VP.INIT_GRID_CAP * k.VM_CHUNK + 1, 1, 2049, 5000]
    assert VP.init_grid(max(sizes)) == VP.INIT_GRID_CAP < VP.vm_grid(max(sizes)) == VP.chunks(sizes[0]) and VP.chunks(2049) == 2 and VP.chunks(5000) == 3
    rng = np.random.default_rng(160)
    table = make_table(rng, [rng.random((n, 3), dtype=F32) for n in sizes])
    last, C = sizes[0] - 1, k.VM_CHUNK
    variants = [
        ("minima in last rows", {0: [([last], -1.0)], 2: [([2048], -2.0)], 3: [([4999], -3.0)]}),
        ("one thread, two trips; two workgroups; two threads of a chunk", {0: [([256, last], -1.0)], 2: [([100, 2048], -1.0)], 3: [([4100, 4999], -1.0)]}),
        ("two workgroups, a larger value before them; one thread, one chunk", {0: [([3 * C + 7, 40 * C + 9], -1.0), ([5], -0.5)], 3: [([5, 261], -1.0)]}),
        ("two trips, two threads; the last row below an earlier pair", {0: [([17, last], -1.0)], 2: [([3, 700], -1.0), ([2048], -1.5)]}),
        ("the last row below an earlier row", {0: [([C + 1], -1.0), ([last], -1.25)], 3: [([4096], -1.0), ([4999], -1.0)]}),
    ]
    dev = None
    for what, spec in variants:
        poss = _flat_map(rng, table, 1.0)
        for c, groups in spec.items():
            for rows, v in groups:
                poss[c][rows] = v
        exp_min, exp_arg = np.array([p.min() for p in poss]), np.array([int(np.argmin(p)) for p in poss], np.int32)
        if dev is None:
            dev = Table(table, poss)
            got_min, got_arg = dev.state()[1:]
        else:
            got_min, got_arg = dev.set_map(poss)
        assert np.array_equal(got_min.view(np.uint64), exp_min.view(np.uint64)) and np.array_equal(got_arg, exp_arg), (what, got_min, got_arg, exp_min, exp_arg)


# ---- 6. more than 256 clouds ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [257, VP.MAX_CLOUDS])
def test_pick_over_many_clouds(backend, nc):
    """Tables of 257 and 4096 clouds of 8 to 40 rows, num_points 16, 40 tiles in one call: vote_pick's threads take clouds tid, tid + 256, ...  The lowest cloud
    minimum -1.0 sits in two clouds a thread meets on different trips (3 and 259; 0 and 256 in the table of 257), the next, -0.5, in the neighbours 70 and 71,
    and twice in cloud 70 (two clusters 17 apart): after its first tile cloud 70 still ties with 71 and is visited again, its minimum read from LDS."""
    rng = np.random.default_rng(170 + nc)
    sizes = rng.integers(8, 41, nc)
    xyzs = [(rng.random((n, 3), dtype=F32) * np.array([3, 2.5, 2], F32)).astype(F32) for n in sizes]
    xyzs[70] = np.concatenate([rng.random((20, 3), dtype=F32) * F32(0.5), rng.random((20, 3), dtype=F32) * F32(0.5) + F32(10)]).astype(F32)
    table = make_table(rng, xyzs)
    poss = _flat_map(rng, table)
    a, b = (3, 259) if nc > 259 else (0, 256)
    poss[a][2] = poss[b][5] = -1.0
    poss[70][0] = poss[70][39] = poss[71][2] = -0.5
    assert nc > VP.BLOCK and a % VP.BLOCK == b % VP.BLOCK

    def check(k, plans, ref, state):
        order = ref["cloud"].tolist()
        assert order[:5] == [a, b, 70, 70, 71], order
        assert max(order) >= VP.BLOCK and any(x == y for x, y in zip(order, order[1:]))

    _chain(table, poss, 16, [40], rng, check, entry="vote" if nc == 257 else "feed", flags=GLOBAL_ROWS, what="%d clouds" % nc)


# ---- 7. vote_thresh: the threshold bin at the edges of a thread's stretch, a cumulative count equal to num_points ---------------------------------------------
def _shell(rng, n, lo, hi):
    """n rows with r^2 in (lo, hi) around the origin"""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = (d * np.sqrt(lo + (hi - lo) * (0.05 + 0.9 * rng.random((n, 1))))).astype(F32)
    key = TP.keys(p, ORIGIN)
    assert (key > lo).all() and (key < hi).all()
    return p


THRESH = [("first_bin_of_stretch", (4.0, 4.0625), 500, 0, False), ("last_bin_of_stretch", (7.875, 8.0), 500, 63, False), ("count_equals_num_points", (7.875, 8.0), 300, 63, True)]


@pytest.mark.parametrize("name,shell,rows,edge,exact", THRESH, ids=[x[0] for x in THRESH])
def test_threshold_bin_edges(backend, name, shell, rows, edge, exact):
    """300 rows with r^2 in (1, 3), `rows` in one bin, 200 beyond, num_points 600: the cumulative count reaches 600 inside the crowded bin, which is the first
    (T % 64 = 0) or the last (T % 64 = 63) of the 64 bins one thread of vote_thresh walks; with 300 rows in it the count equals num_points exactly at T."""
    rng = np.random.default_rng(180)
    PER = (1 << constants().TS_BITS) // VP.BLOCK                       # the bins one thread of vote_thresh walks
    cloud = np.concatenate([_shell(rng, 300, 1.0, 3.0), _shell(rng, rows, *shell), _shell(rng, 200, 9.0, 20.0)])[rng.permutation(500 + rows)]
    table = make_table(rng, [cloud])

    def check(k, plans, ref, state):
        for p in plans:
            assert PER == 64 and p.T % PER == edge and (p.cand == 600) == exact and p.cand == 300 + rows, vars(p)

    _chain(table, _flat_map(rng, table), 600, [2], rng, check, centre=ORIGIN, what=name)
    _indep(table, 600, [0], [int(rng.integers(len(cloud)))], rng, check, centre=ORIGIN, what=name + ", independent")


# ---- 8. equal keys across the cut and across a range boundary ---------------------------------------------------------------------------------------------------
def test_equal_keys_across_cut_and_range_boundary(backend):
    """A 17^3 lattice around the origin: the rows at positions num_points - 1 and num_points of the stable order have equal keys (the cut goes through a run of
    ties: the lower rows stay), and a run of equal keys lies across position k x TS_RSTEP of the candidates for every k."""
    k = constants()
    rng = np.random.default_rng(190)
    lat = TP.lattice(rng, 17, 0.25)
    ks = np.sort(TP.keys(lat, ORIGIN))
    N = next(n for n in range(3000, 3400) if ks[n - 1] == ks[n])
    table = make_table(rng, [lat])

    def check(c, plans, ref, state):
        for p in plans:
            edges = [q * k.TS_RSTEP for q in range(1, p.nk) if q * k.TS_RSTEP < p.cand]
            assert ks[N - 1] == ks[N] and p.cand > N and len(edges) >= 2 and all(ks[e - 1] == ks[e] for e in edges), (N, p.cand, edges)

    _chain(table, _flat_map(rng, table), N, [2], rng, check, centre=ORIGIN, entry="vote", what="lattice")
    _indep(table, N, [0], [1234], rng, check, centre=ORIGIN, what="lattice, independent")


# ---- 9. padding -------------------------------------------------------------------------------------------------------------------------------------------------
PAD_SIZES = (1, 100, 999, 1000, 1001)


@pytest.mark.parametrize("N", [1000, 100])
def test_padding(backend, N):
    """Clouds of 1, 100, 999, 1000 and 1001 rows at num_points 1000 and 100 (below 256; neither a multiple of 256): m < N, m == N, m > N, m == 1; every tile's
    last two rows carry dup_u = 0 and 1.0.  The map sends the chain through clouds 1, 2, 3, 4 and then 0 (a cloud of one row gains 0 and would be visited for
    ever); independent tiles, one per cloud."""
    rng = np.random.default_rng(200 + N)
    table = make_table(rng, [TP.box_room(rng, n)[0] for n in PAD_SIZES])
    poss = _flat_map(rng, table, 10.0)
    order = [1, 2, 3, 4, 0]
    for k, c in enumerate(order):
        poss[c][int(rng.integers(PAD_SIZES[c]))] = 0.01 * k
    ms = [PAD_SIZES[c] for c in order]
    assert any(m < N for m in ms) and any(m == N for m in ms) and any(m > N for m in ms) and 1 in ms and N % VP.BLOCK != 0

    def check(k, plans, ref, state):
        assert ref["cloud"].tolist() == order, ref["cloud"]

    _chain(table, poss, N, [5], rng, check, flags=XY_ONLY, noise_scale=0.1, what="padding")
    _indep(table, N, order, [int(rng.integers(PAD_SIZES[c])) for c in order], rng, what="padding, independent")


# ---- 10. more than 256 independent tiles, refused tiles among good ones ----------------------------------------------------------------------------------------
def test_many_tiles_and_refused_tiles(backend):
    """300 tiles of 64 points over clouds of 40, 64, 65 and 700 rows (vote_place's second workgroup; every cloud used many times).  Tiles 7, 255, 256 and 299 carry
    a cloud id of -1 or nc, or a point id of m: zero tiles and status bits 2 and 4, which ssdr_feed_status reports once; every other tile equals the oracle, and
    the next call is clean."""
    rng = np.random.default_rng(210)
    sizes, N, B = (40, 64, 65, 700), 64, 300
    table = make_table(rng, [TP.box_room(rng, n)[0] for n in sizes])
    tc = rng.integers(0, 4, B).astype(np.int32)
    tp = np.array([rng.integers(sizes[c]) for c in tc], np.int32)
    assert B > VP.BLOCK and np.bincount(tc, minlength=4).min() > 10
    draws = make_draws(rng, B, N)
    ref = VP.indep_reference(table, tc, tp, draws, N)
    bad_c, bad_p = tc.copy(), tp.copy()
    bad_c[7], bad_c[255] = -1, len(sizes)
    bad_p[256], bad_p[299] = sizes[tc[256]], sizes[tc[299]]
    bad = [7, 255, 256, 299]
    good = np.setdiff1d(np.arange(B), bad)
    VP.feed_status()
    dev = Table(table)
    got = dev.tiles(bad_c, bad_p, draws, N)
    assert VP.feed_status() == (VP.ERR_INVALID, VP.ST_CLOUD | VP.ST_POINT)
    assert VP.feed_status() == (0, 0)
    for t in bad:
        VP.zero_tile(got, t, "refused")
    compare(got, ref, "good tiles among refused ones:", tiles=good)
    got = dev.tiles(tc, tp, draws, N)
    compare(got, ref, "the next call:")
    assert VP.feed_status() == (0, 0)


# ---- 11. options on the hard paths -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hole", "global_sort"])
def test_options_on_hard_paths(backend, case):
    """On the two-bin table (a hole in the range table) and on 9000 rows in one bin (sorted in place in global memory): the weighted update with labels outside
    the weights (weight 0, status bit 1, the map equal to the oracle's with that weight), and out_feat / out_labels NULL, the colours NULL."""
    rng = np.random.default_rng(220)
    if case == "hole":
        table, N, check = _hole_table(rng), 5000, _hole_check
    else:
        table, N = make_table(rng, [TP.one_bin_room(rng, 9000)]), 6000

        def check(k, plans, ref, state):
            for p in plans:
                assert p.ranges == [9000] and VP.sort_path(9000) == "global", vars(p)
    poss = _flat_map(rng, table)
    w4 = rng.random(4) + 0.5
    assert (table.clouds[0]["labels"] >= 4).any() and (table.clouds[0]["labels"] < 4).any()
    VP.feed_status()
    (_, _, weighted), = _chain(table, poss, N, [2], rng, check, centre=ORIGIN, flags=XY_ONLY, weights=w4, oracle_weights=np.concatenate([w4, np.zeros(4)]), what=case + ", weighted")
    assert VP.feed_status() == (VP.ERR_INVALID, VP.ST_LABEL)
    assert VP.feed_status() == (0, 0)
    (full, _, plain), = _chain(table, poss, N, [2], np.random.default_rng(221), check, centre=ORIGIN, what=case)
    assert not np.array_equal(weighted[0], plain[0])                      # the weights decide the map
    (got, _, _), = _chain(table, poss, N, [2], np.random.default_rng(221), check, centre=ORIGIN, feat=False, labels=False, what=case + ", no features, no labels")
    assert "feat" not in got and "labels" not in got and np.array_equal(got["idx"], full["idx"])
    (got, _, _), = _chain(table, poss, N, [2], np.random.default_rng(221), check, centre=ORIGIN, colors=False, what=case + ", no colours")
    assert got["feat"].shape[-1] == 3 and np.array_equal(got["feat"].view(np.uint32), full["xyz"].view(np.uint32))
    assert VP.feed_status() == (0, 0)


# ---- 12. VoteState across calls of another shape -----------------------------------------------------------------------------------------------------------------
def _sequence(stream):
    """A (a small weighted chain over five clouds, num_points 100), A again from the same map (the same offset table: its upload is skipped), B (the
    vote_compact_bins table as independent tiles: another rstride, the histograms left as cursors and cleared, two rows of scratch), C (independent tiles of a
    third table, one refused), A a third time: the three results of A equal the oracle, hence each other, bit for bit"""
    k = constants()
    rng = np.random.default_rng(230)
    ta = make_table(rng, [TP.box_room(rng, n)[0] for n in (5000, 300, 1000, 999, 2500)])
    pa = _flat_map(rng, ta)
    weights = rng.random(8) + 0.1
    big = _large(LARGE[1][0])
    tcl = make_table(rng, [TP.box_room(rng, n)[0] for n in (40, 64, 65, 1500)])
    assert len({VP.rstride(ta.maxn), VP.rstride(big.table.maxn), VP.rstride(tcl.maxn)}) == 3 and VP.rstride(big.table.maxn) > k.TS_RMAX

    def run_a(what):
        (got, ref, state), = _chain(ta, pa, 100, [6], np.random.default_rng(231), flags=XY_ONLY, weights=weights, stream=stream, what=what)
        assert len(set(ref["cloud"].tolist())) > 1
        return got

    VP.feed_status(stream)
    first = run_a("A")
    second = run_a("A again")
    compare(Table(big.table, stream=stream).tiles(big.tc, big.tp, big.idraws, LARGE_N), big.iref, "B:")
    draws = make_draws(rng, 4, 64)
    tc, tp = [3, 0, 1, 2], [700, 5, 64, 9]                              # tile 2: point id m
    ref = VP.indep_reference(tcl, tc, [700, 5, 63, 9], draws, 64)
    got = Table(tcl, stream=stream).tiles(tc, tp, draws, 64)
    assert VP.feed_status(stream) == (VP.ERR_INVALID, VP.ST_POINT)
    VP.zero_tile(got, 2, "C")
    compare(got, ref, "C:", tiles=[0, 1, 3])
    third = run_a("A after B and C")
    for name in first:
        assert np.array_equal(first[name].view(np.uint32), second[name].view(np.uint32)) and np.array_equal(first[name].view(np.uint32), third[name].view(np.uint32)), name
    assert VP.feed_status(stream) == (0, 0)


def test_state_reuse_on_the_library_stream(backend):
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
