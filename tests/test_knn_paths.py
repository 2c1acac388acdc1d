"""The KNN grid, its retry pass and the hand-over to the tree walk, branch by branch (csrc/knn_grid.hip, kdtree.hip, api_knn.hip).

Results alone cannot see what this family most easily gets wrong: the tree walk is exact for every row, so a grid that hands over every row, never
settles one or stops answering the fused K = 1 job still matches the oracle bit for bit.  Every case therefore asserts three things:
  1. from the plan (tests/_knn_paths.py, on the device's own grid descriptor), BEFORE the call under test, that it is on the branch it names;
  2. the hand-over counters [0] / [1] (ssdr_knn_counters) against the rule: equal to hard_rows when no row left the grid unsettled ([3] == 0),
     otherwise [0] - [3] <= hard_rows <= [0], and inside the plan's |hard_rows U unsettled| bounds;
  3. the retry ([4] / [5]), unsettled ([3]) and fused (nq - [5]) counts inside the plan's bounds;
and the indices bit for bit against the oracle (int64, int32, and a pyramid where noted).  Each case prints its borderline share (at most 2 % of the rows)
and the certain rows of every branch."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _knn_paths as P
from conftest import GPU_LIB, PKG, ROOT, _have_gpu, assert_bits_equal

B, N = 2, 2048
BRANCHES = ("first_final", "long_row", "too_few_marks", "settled_5", "settled_7", "unsettled")


def _probe(sup):
    """the device's descriptors of the support sets sup [B, n, 3]: a one-query call builds the same grids (they depend on the support alone)"""
    from ssdr_al import knn
    knn.knn_batch(sup, np.ascontiguousarray(sup[:, :1]), 16)
    out = []
    for b in range(len(sup)):
        c, d = knn.knn_counters(set=b)
        assert d is not None and d["n"] == sup.shape[1]
        out.append(d)
    return out


class Tally:
    """sums over the jobs of a call"""

    def __init__(self):
        self.rows = self.border = 0
        self.hard = {16: 0, 1: 0}
        self.hand = {16: [0, 0], 1: [0, 0]}
        self.retry = {16: [0, 0], 1: [0, 0]}
        self.uns = [0, 0]
        self.fused = [0, 0]
        self.certain = dict.fromkeys(BRANCHES, 0)

    def add(self, K, p, hard, live_lo=None, live_hi=None):
        """live_*: rows of the job that reach the second pass at all (a fused K = 1 job: those the K = 16 scan did not answer)"""
        retry_lo, retry_hi = (p.retry_lo, p.retry_hi) if live_lo is None else (live_lo, live_hi)
        uns_lo, uns_hi = p.unsettled_lo & retry_lo, p.unsettled_hi & retry_hi
        self.rows += p.nq
        self.border += int(p.borderline.sum())
        self.hard[K] += int(hard.sum())
        self.hand[K][0] += int((hard | uns_lo).sum()); self.hand[K][1] += int((hard | uns_hi).sum())
        self.retry[K][0] += int(retry_lo.sum()); self.retry[K][1] += int(retry_hi.sum())
        self.uns[0] += int(uns_lo.sum()); self.uns[1] += int(uns_hi.sum())
        if live_lo is None:
            for nm, v in zip(BRANCHES, (p.first_final, p.long_row, p.too_few_marks, p.settled_at[1], p.settled_at[2], p.unsettled_lo)):
                self.certain[nm] += int(v.sum())

    def show(self, name):
        print("%s: rows %d, borderline %d (%.2f %%); certain rows %s; hard rows K=16 %d, K=1 %d; bounds: hand-over %s %s, retry %s %s, unsettled %s, "
              "fused %s" % (name, self.rows, self.border, 100.0 * self.border / max(self.rows, 1), self.certain, self.hard[16], self.hard[1], self.hand[16],
                            self.hand[1], self.retry[16], self.retry[1], self.uns, self.fused))
        assert self.border <= P.BORDERLINE_CAP * self.rows, "%s: %d borderline rows of %d" % (name, self.border, self.rows)

    def expect(self, name, least):
        for nm, m in least.items():
            assert self.certain[nm] >= m, "%s is not on the branch %s: %d certain rows, at least %d wanted" % (name, nm, self.certain[nm], m)

    def check(self, name, c, status=0, nq1=None):
        c = [int(v) for v in c]
        print("%s: counters %s" % (name, c[:13]))
        assert c[2] == status and c[11] == 0, "%s: status words %d, %d" % (name, c[2], c[11])
        for K, w in ((16, 0), (1, 1)):
            assert self.hand[K][0] <= c[w] <= self.hand[K][1], "%s: %d rows handed over (K = %d), plan %s" % (name, c[w], K, self.hand[K])
            assert self.retry[K][0] <= c[4 + w] <= self.retry[K][1], "%s: %d rows in the second pass (K = %d), plan %s" % (name, c[4 + w], K, self.retry[K])
        assert self.uns[0] <= c[3] <= self.uns[1], "%s: %d unsettled rows, plan %s" % (name, c[3], self.uns)
        hard = self.hard[16] + self.hard[1]
        if c[3] == 0:
            assert c[0] == self.hard[16] and c[1] == self.hard[1], "%s: handed over %d + %d, the rule gives %d + %d" % (name, c[0], c[1], self.hard[16], self.hard[1])
        else:
            assert c[0] + c[1] - c[3] <= hard <= c[0] + c[1], "%s: handed over %d + %d, %d unsettled, the rule gives %d" % (name, c[0], c[1], c[3], hard)
            assert self.hard[16] <= c[0] and self.hard[1] <= c[1]
        assert c[6] == c[0] + c[1], "%s: %d balls for %d handed-over rows" % (name, c[6], c[0] + c[1])
        if nq1 is not None:
            assert self.fused[0] <= nq1 - c[5] <= self.fused[1], "%s: %d rows of the K = 1 jobs answered inside the K = 16 scan, plan %s" % (name, nq1 - c[5], self.fused)


def _launch_checks(name, backend, t, total_q, max_n, want):
    K = 16 if t.hand[16][1] >= t.hand[1][1] else 1
    L = P.launches(backend, total_q, max_n, t.hand[K], t.retry[K])
    print("%s: work_cap %d, work-list grid %d -> %s rows per wave, retry grid %d -> second trip %s, build %s, rebuild %s" %
          (name, L.work_cap, L.wl_grid, L.rows_per_wave, L.retry_grid, L.retry_second_trip, L.build, L.rebuild))
    for key, v in want.items():
        assert getattr(L, key) == v, "%s: %s is %s, the case names %s" % (name, key, getattr(L, key), v)
    return L


def run_batch(backend, orc, name, sup, qry=None, K=16, least=None, launch=None, status=0):
    """one knn_batch call (int64, then int32) of queries `qry` (None: the support itself, taken in cell order) against sup [B, n, 3]"""
    from ssdr_al import knn
    Q = sup if qry is None else qry
    descs = _probe(sup)
    t = Tally()
    for b in range(len(sup)):
        d2 = P.nearest_d2(orc, sup[b], Q[b], K)
        t.add(K, P.plan(descs[b], sup[b], Q[b], K, d2), P.hard_rows(d2, K))
    t.show(name)
    t.expect(name, least or {})
    t.launches = _launch_checks(name, backend, t, Q.shape[0] * Q.shape[1], sup.shape[1], launch or {})
    ref = orc.knn_batch(sup, Q, K, threads=4)
    got = knn.knn_batch(sup, Q, K)
    c = knn.knn_counters()
    for b in range(len(sup)):
        d = knn.knn_counters(set=b)[1]
        assert all(np.array_equal(d[f], descs[b][f]) for f in d), "%s: the grid of set %d changed between two calls" % (name, b)
    assert_bits_equal(got, ref, name + " int64")
    t.check(name, c, status)
    assert c[1 if K == 16 else 0] == 0 and c[5 if K == 16 else 4] == 0
    got = knn.knn_batch_i32(sup, Q, K)
    c32 = knn.knn_counters()
    assert_bits_equal(got, ref.astype(np.int32), name + " int32")
    assert np.array_equal(c32[:10], c[:10]), "%s: int32 counters %s, int64 %s" % (name, list(c32[:10]), list(c[:10]))
    assert knn.knn_status()[:3] == (c[0], c[1], 0)          # the accessor folded and cleared nothing
    return t, c


def run_pyramid(backend, orc, name, xyz, ratios, least=None, launch=None, fused_least=0):
    from ssdr_al import knn
    nb = len(xyz)
    sizes = [xyz.shape[1]]
    for r in ratios:
        sizes.append(sizes[-1] // r)
    descs = [_probe(np.ascontiguousarray(xyz[:, :n])) for n in sizes]
    t = Tally()
    ref_n, ref_i = [], []
    for l in range(len(ratios)):
        cur, n1 = xyz[:, :sizes[l]], sizes[l + 1]
        ref_n.append(orc.knn_batch(cur, cur, 16, threads=4).astype(np.int32))
        ref_i.append(orc.knn_batch(cur[:, :n1], cur, 1, threads=4).astype(np.int32))
        for b in range(nb):
            d2 = P.nearest_d2(orc, cur[b], cur[b], 16)
            e2 = P.nearest_d2(orc, cur[b, :n1], cur[b], 1)
            p16 = P.plan(descs[l][b], cur[b], cur[b], 16, d2, n1, e2)
            t.add(16, p16, P.hard_rows(d2, 16))
            p1 = P.plan(descs[l + 1][b], cur[b, :n1], cur[b], 1, e2)
            p1.borderline = p1.borderline & ~p16.fused_lo          # only the rows its own grid may see
            t.add(1, p1, P.hard_rows(e2, 1), ~p16.fused_hi, ~p16.fused_lo)
            t.fused[0] += int(p16.fused_lo.sum()); t.fused[1] += int(p16.fused_hi.sum())
    t.show(name)
    t.expect(name, least or {})
    assert t.fused[0] >= fused_least, "%s: %d rows certainly answered inside the K = 16 scan, at least %d wanted" % (name, t.fused[0], fused_least)
    nq1 = nb * sum(sizes[:-1])
    _launch_checks(name, backend, t, 2 * nq1, sizes[0], launch or {})
    neigh, sub, interp = knn.knn_pyramid(xyz, ratios, 16)
    c = knn.knn_counters()
    for l in range(len(sizes)):                              # the pyramid's own grids: set (l, b) is the prefix of sizes[l] points of tile b
        for b in range(nb):
            d = knn.knn_counters(set=l * nb + b)[1]
            assert d is not None and all(np.array_equal(d[f], descs[l][b][f]) for f in d), "%s: the grid of level %d, tile %d is not the planned one" % (name, l, b)
    assert knn.knn_counters(set=len(sizes) * nb)[1] is None
    for l in range(len(ratios)):
        assert_bits_equal(neigh[l], ref_n[l], "%s level %d neigh" % (name, l))
        assert_bits_equal(sub[l], ref_n[l][:, :sizes[l + 1]], "%s level %d sub" % (name, l))
        assert_bits_equal(interp[l], ref_i[l], "%s level %d interp" % (name, l))
    t.check(name, c, nq1=nq1)
    return t, c


def _stack(fn, seeds, **kw):
    return np.stack([fn(s, **kw) for s in seeds])


def test_new_symbols_in_both_libraries(emu_lib):
    import ctypes
    for path in (emu_lib, GPU_LIB):
        assert hasattr(ctypes.CDLL(path), "ssdr_knn_counters"), path


def test_counters_accessor_reads_only(backend, orc):
    """ssdr_knn_counters folds and clears nothing: a failing call's ticket is still reported by ssdr_knn_status_poll afterwards, once; without a grid the
    ten grid words are zero and there is no descriptor; a set the call did not have leaves the descriptor untouched"""
    from ssdr_al import _lib, knn
    from ssdr_al._lib import DevArray
    x = np.repeat((2.0 ** -np.arange(110)).astype(np.float32), 2)          # a tree deeper than the level limit, with duplicates (test_knn.py)
    p = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)[None]
    d_p = DevArray.from_host(p); d_o = DevArray((1, p.shape[1], 16), np.int32)
    _lib.check(_lib.lib().ssdr_knn_batch_dev(d_p.ptr, 1, p.shape[1], 3, d_p.ptr, p.shape[1], 16, d_o.ptr, None))
    a, b = knn.knn_counters(), knn.knn_counters()
    assert np.array_equal(a, b) and a[0] > 0 and a[11] == 4 and not a[13:].any(), list(a)
    c, d = knn.knn_counters(set=0)
    assert d["n"] == p.shape[1] and knn.knn_counters(set=1)[1] is None
    with pytest.raises(_lib.SsdrError):
        knn.knn_status(wait=False)                                         # the call's ticket is still there to be folded
    assert knn.knn_status(wait=False)[2] == 0                              # reported once, then clear
    q = np.random.default_rng(0).random((1, 500, 3), dtype=np.float32)
    assert_bits_equal(knn.knn_batch(q, q, 5), orc.knn_batch(q, q, 5), "K = 5")       # no grid in this call
    c, d = knn.knn_counters(set=0)
    assert not c[:10].any() and d is None and c[12] > 0, list(c)
    with pytest.raises(_lib.SsdrError):
        _lib.check(_lib.lib().ssdr_knn_counters(None, None, 0, None))


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------------------
def test_uniform_first_pass_final(backend, orc):
    p = _stack(P.uniform, (11, 12))
    t, c = run_batch(backend, orc, "uniform", p, least={"first_final": int(0.9 * B * N)})
    assert c[0] == t.hard[16]
    t, c = run_pyramid(backend, orc, "uniform pyramid", p, [4, 4], fused_least=int(0.9 * B * (N + N // 4)))


def test_padded_lattice_ties_and_long_work_list(backend, orc):
    p = _stack(P.padded_lattice, (21, 22))
    t, c = run_batch(backend, orc, "padded", p, launch={"rows_per_wave": 64})
    assert t.hard[16] > 600
    t, c = run_pyramid(backend, orc, "padded pyramid", p, [4, 4, 2])
    assert c[3] == 0 and c[0] == t.hard[16] and c[1] == t.hard[1] and t.hard[1] > 100


def test_few_duplicates_short_work_list(backend, orc):
    p = _stack(P.few_duplicates, (31, 32))
    t, c = run_batch(backend, orc, "few duplicates", p, launch={"rows_per_wave": 4})
    assert 1 <= c[0] <= 4 * 64


def test_near_tie_rule_is_exact(backend, orc):
    k = P.constants()
    clouds = [P.near_tie(s) for s in (41, 42)]
    p = np.stack([c[0] for c in clouds])
    ng, gs = clouds[0][1], clouds[0][2]
    inside = outside = 0
    for b in range(B):
        q = p[b, :ng * gs:gs]                                  # the groups' query points
        d2 = P.nearest_d2(orc, p[b], q, 16)
        ratio = d2[:, 16].astype(np.float64) / d2[:, 15]
        assert np.array_equal(P.hard_rows(d2, 16), np.arange(ng) < ng // 2)      # the first half is handed over, the second is not
        inside += int(((ratio > 1) & (d2[:, 16] <= d2[:, 15] * k.NEAR_TIE)).sum())
        outside += int(((d2[:, 16] > d2[:, 15] * k.NEAR_TIE) & (ratio <= 1 + 4 * 2.0 ** -17)).sum())
    print("near-tie: %d rows with d[K] / d[K-1] in (1, NEAR_TIE], %d in (NEAR_TIE, 1 + 4 * 2^-17]" % (inside, outside))
    assert inside >= 50 and outside >= 50
    t, c = run_batch(backend, orc, "near-tie", p)
    assert c[3] == 0 and c[0] == t.hard[16] and t.hard[16] >= inside


def test_dense_clump_long_rows_and_second_trip(backend, orc):
    p = _stack(P.dense_clump, (51, 52))
    run_batch(backend, orc, "dense clump", p, least={"long_row": 2 * 300}, launch={"retry_second_trip": True})


def test_corner_groups_larger_blocks_and_unsettled(backend, orc):
    p = _stack(P.corner_groups, (61, 62))
    t, c = run_batch(backend, orc, "corner groups", p, least={"too_few_marks": 40, "settled_5": 10, "settled_7": 10, "unsettled": 10})
    assert c[3] >= 10


@pytest.mark.parametrize("K", [16, 1])
def test_foreign_queries_outside_the_box(backend, orc, K):
    rng = np.random.default_rng(71)
    sup = (P.BOX / 3 + rng.random((B, 512, 3)) * P.BOX / 3).astype(np.float32)
    q = (rng.random((B, 2048, 3)) * P.BOX).astype(np.float32)
    t, c = run_batch(backend, orc, "foreign queries K=%d" % K, sup, q, K, least={"unsettled": 20})
    assert c[3] > 0


def test_cloud_far_from_the_origin(backend, orc):
    p = _stack(P.uniform, (11, 12)) + np.float32(1e5)
    t, c = run_batch(backend, orc, "cloud at +1e5", p)
    assert t.retry[16][0] > B * N // 2 and c[3] == 0 and c[0] == t.hard[16]


def test_safety_net_one_cell_grid(backend, orc):
    k = P.constants()
    p = P.places_copies(81)[None]
    d = _probe(p)[0]
    print("safety net: descriptor %dx%dx%d, c = %g, extent %g" % (d["nx"], d["ny"], d["nz"], d["c"], (d["hi"] - d["lo"]).max()))
    assert (d["nx"], d["ny"], d["nz"]) == (1, 1, 1) and d["c"] == np.float32(2) * (d["hi"] - d["lo"]).max() + np.float32(1)
    t, c = run_batch(backend, orc, "safety net", p)
    assert c[0] == p.shape[1] > k.GRID_BALL_CAP and c[8] == 0


def test_two_clumps_cell_cap_growth(backend, orc):
    p = _stack(P.two_clumps, (91, 92))
    descs = _probe(p)
    for d in descs:
        cells = d["nx"] * d["ny"] * d["nz"]
        print("two clumps: %dx%dx%d = %d cells of %g for %d points" % (d["nx"], d["ny"], d["nz"], cells, d["c"], d["n"]))
        assert cells <= 8 * d["n"] + 64 and d["c"] > 1.0          # the measured radius of 22 points among 1024 in the 4 x 3 x 2 box is far below 1
    t, c = run_batch(backend, orc, "two clumps", p)
    assert c[3] == 0 and c[0] == t.hard[16]


@pytest.mark.parametrize("n", [89, 88, 17, 16, 1])
def test_small_sets(backend, orc, n):
    k = P.constants()
    assert 4 * k.GRID_TARGET_PTS == 88
    rng = np.random.default_rng(100 + n)
    p = (rng.random((B, n, 3)) * P.BOX).astype(np.float32)
    for d in _probe(p):
        ext = (d["hi"] - d["lo"]).max()
        print("n = %d: %dx%dx%d cells of %g, extent %g" % (n, d["nx"], d["ny"], d["nz"], d["c"], ext))
        if 1 < n <= 88:
            assert d["c"] == ext                                # no measured radius at or below 4 * GRID_TARGET_PTS points
    from ssdr_al import knn
    t, c = run_batch(backend, orc, "n = %d" % n, p)
    if n < 17:
        assert c[0] == c[3] == B * n
        assert (knn.knn_batch(p, p, 16)[:, :, n:] == 0).all()   # unwritten slots stay 0
    run_batch(backend, orc, "n = %d K = 1" % n, p, None, 1)


@pytest.mark.parametrize("target", ["1", "300"])
def test_target_pts_switch(backend, orc, monkeypatch, target):
    p0, p1 = _stack(P.uniform, (11, 12)), _stack(P.layered, (111, 112))
    base = [_probe(p)[0]["c"] for p in (p0, p1)]
    monkeypatch.setenv("SSDR_KNN_TARGET_PTS", target)
    for nm, p, c0 in (("uniform", p0, base[0]), ("layered", p1, base[1])):
        c = _probe(p)[0]["c"]
        print("%s: cell %g at TARGET_PTS = %s, %g by default" % (nm, c, target, c0))
        assert c < c0 if target == "1" else c > c0
        run_batch(backend, orc, "%s, TARGET_PTS = %s" % (nm, target), p)
        run_pyramid(backend, orc, "%s pyramid, TARGET_PTS = %s" % (nm, target), p, [4, 4])


def _dups_for(orc, lo, hi):
    """a uniform cloud of 4096 points (one of 2048 cannot hand over more rows than the ball list holds) with the number of duplicated points tuned so
    that hard_rows lies in [lo, hi]"""
    for dup in range(20, 400, 2):
        p = P.few_duplicates(121, 2 * N, dup)
        d2 = P.nearest_d2(orc, p, p, 16)
        h = int(P.hard_rows(d2, 16).sum())
        if lo <= h <= hi:
            return p[None], h
    raise AssertionError("no duplicate count gives %d..%d hard rows" % (lo, hi))


@pytest.mark.parametrize("side", ["below", "above"])
def test_ball_cap_either_side(backend, orc, monkeypatch, side):
    k = P.constants()
    assert k.GRID_BALL_CAP == 2048
    p, h = _dups_for(orc, 2049, 2200)
    # the queries: the cloud's own points without some of the rows the rule hands over, so that exactly GRID_BALL_CAP (the last count the ball list
    # holds) or one more remain
    hard = P.hard_rows(P.nearest_d2(orc, p[0], p[0], 16), 16)
    h = k.GRID_BALL_CAP + (side == "above")
    keep = np.sort(np.concatenate([np.flatnonzero(~hard), np.flatnonzero(hard)[:h]]))
    q = np.ascontiguousarray(p[:, keep])
    monkeypatch.setenv("SSDR_KNN_BALL_SCALE", "1e-9")
    t, c = run_batch(backend, orc, "ball cap, %s (%d hard rows)" % (side, h), p, q, launch={"rebuild": "one workgroup per tree"})
    assert c[3] == 0 and c[0] == h
    if side == "below":
        assert c[8] > 0
    else:
        assert c[8] == 0


def test_rebuild_above_one_workgroup_size(backend, orc, monkeypatch):
    k = P.constants()
    n = 65600
    assert n > 64 * (k.TREE_Q // 4)
    p = P.few_duplicates(131, n, 30)
    p = (p * np.float32(4)).astype(np.float32)[None]
    monkeypatch.setenv("SSDR_KNN_BALL_SCALE", "1e-9")
    t, c = run_batch(backend, orc, "rebuild above one workgroup's size", p, launch={"rebuild": "level-wide"})
    build = t.launches.build
    assert "kd_split_kernel<512>" in build and "kd_split_kernel<256>" in build and build[-1] == "kd_rest_kernel", build
    assert 0 < t.hard[16] <= k.GRID_BALL_CAP and c[0] == t.hard[16] and c[3] == 0
    assert c[8] > 0                                         # rows again on the complete tree: the rebuild ran


def test_tree_only(backend, orc, monkeypatch):
    from ssdr_al import knn
    monkeypatch.setenv("SSDR_KNN_TREE_ONLY", "1")
    rng = np.random.default_rng(141)
    lattice = (np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(8), indexing="ij"), -1).reshape(-1, 3) * 0.05).astype(np.float32)
    for nm, p in (("uniform", _stack(P.uniform, (11, 12))), ("padded", _stack(P.padded_lattice, (21, 22))),
                  ("lattice", np.stack([lattice[rng.permutation(N)] for _ in range(B)]))):
        q = (rng.random((B, 300, 3)) * P.BOX).astype(np.float32)
        for K in (16, 1):
            for qq, what in ((p, "self"), (q, "foreign")):      # self: qorder (the queries in the tree's point order); foreign: natural order
                ref = orc.knn_batch(p, qq, K, threads=4)
                assert_bits_equal(knn.knn_batch(p, qq, K), ref, "tree only %s %s K=%d int64" % (nm, what, K))
                c = knn.knn_counters()
                assert not c[:10].any() and c[11] == 0 and c[12] > 0, list(c)
                assert_bits_equal(knn.knn_batch_i32(p, qq, K), ref.astype(np.int32), "tree only %s %s K=%d int32" % (nm, what, K))
                assert not knn.knn_counters()[:10].any()
        ref = orc.knn_batch(p, q, 5, threads=4)                 # any other K: the generic kernel, both index types
        assert_bits_equal(knn.knn_batch(p, q, 5), ref, "tree only %s K=5 int64" % nm)
        assert_bits_equal(knn.knn_batch_i32(p, q, 5), ref.astype(np.int32), "tree only %s K=5 int32" % nm)
        neigh, sub, interp = knn.knn_pyramid(p, [4, 4], 16)
        assert not knn.knn_counters()[:10].any()
        cur = p
        for l in range(2):
            nxt = cur[:, :cur.shape[1] // 4]
            assert_bits_equal(neigh[l], orc.knn_batch(cur, cur, 16, threads=4).astype(np.int32), "tree only %s pyramid neigh %d" % (nm, l))
            assert_bits_equal(interp[l], orc.knn_batch(nxt, cur, 1, threads=4).astype(np.int32), "tree only %s pyramid interp %d" % (nm, l))
            cur = nxt


# ---- the static switches: a fresh process per setting ------------------------------------------------------------------------------------------------------
def _worker(lib, mode, env):
    e = dict(os.environ, **env)
    for name in ("SSDR_KNN_LDS", "SSDR_KD_LEVELS", "SSDR_KNN_BALL_SCALE", "SSDR_KNN_TREE_ONLY", "SSDR_KNN_TARGET_PTS"):
        if name not in env:
            e.pop(name, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_knn_forms_worker.py"), lib, mode], env=e, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("CASE")]
    assert r.returncode == 0 and lines and "failed" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return lines


def test_lds_form_of_the_first_pass(backend, orc):
    """SSDR_KNN_LDS=1 (grid_search_lds_kernel): the six clouds of test_knn_grid_select.py and the padded pyramid; the results must be the oracle's and the
    hand-over, retry and unsettled counts those of the default form"""
    import test_knn_grid_select as G
    from ssdr_al import _lib
    lib = _lib.lib_path()
    dflt, lds = _worker(lib, "clouds", {}), _worker(lib, "clouds", {"SSDR_KNN_LDS": "1"})
    print("\n".join(lds))
    assert dflt == lds and len(lds) == len(G.CASES) + 1
    for ln in lds:
        w = ln.split()
        if w[1] in G.CASES:
            ref = G._case(w[1], orc)
            h = hashlib.sha256(ref["self16"].tobytes() + ref["up1"].tobytes() + b"".join(a.tobytes() for a in ref["neigh"] + ref["interp"])).hexdigest()
            assert w[2] == h, ln
        else:
            assert w[1] == "padded_pyramid"
            cur, ref = np.stack([P.padded_lattice(sd) for sd in (21, 22)]), {"neigh": [], "interp": []}
            for r in (4, 4, 2):
                nxt = cur[:, :cur.shape[1] // r]
                ref["neigh"].append(orc.knn_batch(cur, cur, 16, threads=4).astype(np.int32))
                ref["interp"].append(orc.knn_batch(nxt, cur, 1, threads=4).astype(np.int32))
                cur = nxt
            assert w[2] == hashlib.sha256(b"".join(a.tobytes() for a in ref["neigh"] + ref["interp"])).hexdigest(), ln


@pytest.mark.gpu
def test_rebuild_levels_switch():
    """SSDR_KD_LEVELS=0 (the complete rebuild by kd_tree_kernel alone at every size) against the default (kd_levels_kernel above ONE_WG_MAX points): the input of
    test_knn.py::test_complete_rebuild_of_several_large_trees_in_one_launch at B = 1, SSDR_KNN_BALL_SCALE=1e-9; the same pyramid, rows again on complete trees"""
    if not _have_gpu():
        pytest.skip("no GPU")
    plain = _worker(GPU_LIB, "rebuild", {})
    dflt = _worker(GPU_LIB, "rebuild", {"SSDR_KNN_BALL_SCALE": "1e-9"})
    off = _worker(GPU_LIB, "rebuild", {"SSDR_KNN_BALL_SCALE": "1e-9", "SSDR_KD_LEVELS": "0"})
    print(plain, dflt, off)
    assert dflt == off and plain[0].split()[2] == dflt[0].split()[2]
    assert int(dflt[0].split()[3]) > 0 and int(plain[0].split()[3]) == 0       # [8]: rows again on complete trees


# ---- every launch is claimed -----------------------------------------------------------------------------------------------------------------------------------
CLAIMS = {
    "grid_search_kernel<16, int64_t>": "test_uniform_first_pass_final", "grid_search_kernel<16, int32_t>": "test_uniform_first_pass_final",
    "grid_search_kernel<1, int64_t>": "test_foreign_queries_outside_the_box", "grid_search_kernel<1, int32_t>": "test_foreign_queries_outside_the_box",
    "grid_search_lds_kernel<16, int64_t>": "test_lds_form_of_the_first_pass", "grid_search_lds_kernel<16, int32_t>": "test_lds_form_of_the_first_pass",
    "grid_retry_kernel<16, int64_t>": "test_dense_clump_long_rows_and_second_trip", "grid_retry_kernel<16, int32_t>": "test_dense_clump_long_rows_and_second_trip",
    "grid_retry_kernel<1, int64_t>": "test_foreign_queries_outside_the_box", "grid_retry_kernel<1, int32_t>": "test_foreign_queries_outside_the_box",
    "kd_search_kernel<16, int64_t>": "test_tree_only", "kd_search_kernel<16, int32_t>": "test_tree_only",
    "kd_search_kernel<1, int64_t>": "test_tree_only", "kd_search_kernel<1, int32_t>": "test_tree_only",
    "kd_search_any_kernel<int64_t>": "test_tree_only", "kd_search_any_kernel<int32_t>": "test_tree_only",
    "kd_search_worklist_kernel<16, int64_t>": "test_padded_lattice_ties_and_long_work_list", "kd_search_worklist_kernel<16, int32_t>": "test_padded_lattice_ties_and_long_work_list",
    "kd_search_worklist_kernel<1, int64_t>": "test_foreign_queries_outside_the_box", "kd_search_worklist_kernel<1, int32_t>": "test_foreign_queries_outside_the_box",
    "kd_tree_kernel": "test_ball_cap_either_side", "kd_levels_kernel": "test_rebuild_levels_switch", "kd_small_subtree_kernel": "test_ball_cap_either_side",
    "kd_init_kernel": "test_rebuild_above_one_workgroup_size", "kd_rest_kernel": "test_rebuild_above_one_workgroup_size",
    "kd_split_kernel<512>": "test_rebuild_above_one_workgroup_size", "kd_split_kernel<256>": "test_rebuild_above_one_workgroup_size",
}
ROWS = {      # the rows of the issue's table -> the test that proves the branch reached
    "uniform box": "test_uniform_first_pass_final", "padded + lattice slice": "test_padded_lattice_ties_and_long_work_list",
    "a handful of duplicates": "test_few_duplicates_short_work_list", "near-tie": "test_near_tie_rule_is_exact",
    "dense clump": "test_dense_clump_long_rows_and_second_trip", "isolated corner groups": "test_corner_groups_larger_blocks_and_unsettled",
    "queries outside the support's box": "test_foreign_queries_outside_the_box", "cloud at +1e5": "test_cloud_far_from_the_origin",
    "100 places x 30 copies": "test_safety_net_one_cell_grid", "two clumps 5 km apart": "test_two_clumps_cell_cap_growth",
    "n = 88, 89, 17, 16, 1": "test_small_sets", "SSDR_KNN_TARGET_PTS": "test_target_pts_switch", "GRID_BALL_CAP either side": "test_ball_cap_either_side",
    "rebuild above 64 * (TREE_Q / 4)": "test_rebuild_above_one_workgroup_size", "SSDR_KNN_TREE_ONLY": "test_tree_only",
    "SSDR_KNN_LDS": "test_lds_form_of_the_first_pass", "SSDR_KD_LEVELS": "test_rebuild_levels_switch",
}


def _function_body(text, head):
    i = text.index(head)
    j = text.index("\n}\n", i)
    return text[i:j]


def test_every_launch_is_claimed_by_a_case():
    grid = open(os.path.join(PKG, "csrc", "knn_grid.hip")).read()
    kd = open(os.path.join(PKG, "csrc", "kdtree.hip")).read()
    found = set()
    for text, head in ((grid, "int grid_search("), (kd, "int kd_search("), (kd, "int kd_search_worklist("), (kd, "static int launch_build(")):
        body = _function_body(text, head)
        names = re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_0-9]+(?:<[^>]*>)?)\s*\)?\s*,", body)
        assert names, head
        found |= {re.sub(r"\s+", " ", n) for n in names}
    here = globals()
    for inst in sorted(found):
        assert inst in CLAIMS, "%s is launched by the KNN family and claimed by no case" % inst
    for what, test in list(CLAIMS.items()) + list(ROWS.items()):
        assert callable(here.get(test)), "%s: no test %s" % (what, test)
    assert set(CLAIMS) == found, "claims of launches that no longer exist: %s" % sorted(set(CLAIMS) - found)
