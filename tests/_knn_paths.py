"""Helpers of tests/test_knn_paths.py: the constants of the KNN grid, retry and hand-over read from the sources, `hard_rows` (the hand-over rule, from
the oracle's K + 1 nearest), `plan` (what a query does on the DEVICE'S OWN grid descriptor: its cell, the populations of the rows of cells around it, the
radius each block guarantees, the block at which it settles), the bounds on the device counters that follow, and `launches` (the host arithmetic of
grid_search, kd_search_worklist and launch_build restated).

Every comparison of a distance with a guaranteed radius is three-valued: within BAND relative of the threshold a row is borderline, counts in upper
bounds only, and is never a "certain" row of a branch.  Cell indices, populations and the radii themselves are float32 / integer arithmetic that NumPy
reproduces exactly (knn_grid.hip is compiled without FMA contraction)."""
import os
import re
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ssdr-al_amd", "csrc")
F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
BAND = 1e-3
BORDERLINE_CAP = 0.02
NUM_CU = {"emu": 8, "gpu": 256}          # tests/hipemu/hip/hip_runtime.h: hipDeviceGetAttribute; MI355X: 256 CUs

_K = None


def _one(pattern, text, what):
    m = set(re.findall(pattern, text))
    assert len(m) == 1, "%s: %d different definitions (%s)" % (what, len(m), sorted(m))
    return m.pop()


def constants():
    global _K
    if _K is None:
        grid = open(os.path.join(CSRC, "knn_grid.hip")).read()
        api = open(os.path.join(CSRC, "api_knn.hip")).read()
        hdr = open(os.path.join(CSRC, "ssdr_internal.hpp")).read()
        kd = open(os.path.join(CSRC, "kdtree.hip")).read()
        k = {}
        k["NEAR_TIE"] = F32(_one(r"constexpr float NEAR_TIE\s*=\s*([0-9.]+)f\s*;", grid, "NEAR_TIE"))
        k["GS_RMAX"] = int(_one(r"constexpr int GS_RMAX\s*=\s*([0-9]+)\s*;", grid, "GS_RMAX"))
        k["GRID_TARGET_PTS"] = int(_one(r"constexpr int GRID_TARGET_PTS\s*=\s*([0-9]+)\s*;", api, "GRID_TARGET_PTS"))
        k["GRID_BALL_CAP"] = int(_one(r"constexpr int GRID_BALL_CAP\s*=\s*([0-9]+)\s*;", hdr, "GRID_BALL_CAP"))
        rl = re.findall(r"constexpr int RL\s*=\s*([0-9]+)\s*,\s*RCB\s*=\s*([0-9]+)\s*;", grid)
        assert len(rl) == 1, "RL, RCB"
        k["RL"], k["RCB"] = int(rl[0][0]), int(rl[0][1])
        k["GM_NT"] = int(_one(r"constexpr int GM_NT\s*=\s*([0-9]+)\s*;", grid, "GM_NT"))
        k["SMALL_MAX"] = int(_one(r"constexpr int SMALL_MAX\s*=\s*([0-9]+)\s*;", kd, "SMALL_MAX"))
        k["LEAF_MAX"] = int(_one(r"constexpr int LEAF_MAX\s*=\s*([0-9]+)\s*;", kd, "LEAF_MAX"))
        k["TREE_Q"] = int(_one(r"constexpr int TREE_NT\s*=\s*[0-9]+\s*,\s*TREE_Q\s*=\s*([0-9]+)\s*;", kd, "TREE_Q"))
        k["ONE_WG_MAX"] = int(_one(r"constexpr int ONE_WG_MAX\s*=\s*([0-9]+)\s*;", kd, "ONE_WG_MAX"))
        k["BIG_LEVELS"] = int(_one(r"constexpr int BIG_LEVELS\s*=\s*([0-9]+)\s*;", kd, "BIG_LEVELS"))
        k["MASK"] = int(_one(r"if \(e - s > ([0-9]+)\) \{ long_row = true;", grid, "mask width"))
        k["SHRINK"] = F32(_one(r"g \* ([0-9.]+)f - d\.slack", grid, "shrink"))
        assert k["NEAR_TIE"] == F32(1 + 2.0 ** -17) and k["GS_RMAX"] == 3 and k["MASK"] == 64
        _K = SimpleNamespace(**k)
    return _K


# ---- distances and the hand-over rule -------------------------------------------------------------------------------------------------------------------
def nearest_d2(orc, sup, q, K):
    """the K + 1 smallest float32 distances ((dx*dx + dy*dy) + dz*dz, no FMA) of every query, ascending, from the oracle's K + 1 nearest; a support of
    fewer than K + 1 points gives +inf in the missing places.  sup [n, 3], q [nq, 3] -> float32 [nq, K + 1]"""
    n = len(sup)
    m = min(n, K + 1)
    out = np.full((len(q), K + 1), np.inf, np.float32)
    if m > 0:
        idx = orc.knn_batch(sup[None], q[None], m, threads=4)[0]
        d = q[:, None, :] - sup[idx]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert d2.dtype == np.float32
        out[:, :m] = np.sort(d2, axis=1)
    return out


def hard_rows(d2, K):
    """grid_finish's rule on the K + 1 smallest distances: two equal values among them, or d[K] <= d[K-1] * NEAR_TIE; too few points -> every row"""
    k = constants()
    if not np.isfinite(d2[:, K]).all():
        return np.ones(len(d2), bool)
    return (np.diff(d2, axis=1) == 0).any(1) | (d2[:, K] <= d2[:, K - 1] * k.NEAR_TIE)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------------------------
def cell_of(v, o, inv_c, n):
    f = (v - F32(o)) * F32(inv_c)
    assert f.dtype == np.float32
    c = np.where(f > 0, np.minimum(f, F32(1.0e9)), F32(0)).astype(np.int64)
    return np.minimum(c, n - 1)


def _cells(desc, p):
    inv_c = F32(1) / F32(desc["c"])
    return [cell_of(p[:, k], desc["lo"][k], inv_c, desc[nm]) for k, nm in enumerate(("nx", "ny", "nz"))]


def _tau(desc, q, cc, R):
    """grid_mark_rows / grid_settled: squared radius the (2R+1)^3 block guarantees; +inf: the block is the whole grid; -1: no positive radius"""
    k = constants()
    c = F32(desc["c"])
    g = np.full(len(q), FLT_MAX, np.float32)
    for a, nm in enumerate(("nx", "ny", "nz")):
        nn, lo, qa = desc[nm], F32(desc["lo"][a]), q[:, a]
        a0, a1 = np.maximum(cc[a] - R, 0), np.minimum(cc[a] + R, nn - 1)
        g = np.where(a0 > 0, np.minimum(g, qa - (lo + a0.astype(np.float32) * c)), g)
        g = np.where(a1 < nn - 1, np.minimum(g, (lo + (a1 + 1).astype(np.float32) * c) - qa), g)
    assert g.dtype == np.float32
    gs = g * k.SHRINK - F32(desc["slack"])
    with np.errstate(over="ignore"):
        t = (gs * gs).astype(np.float64)
    return np.where(g == FLT_MAX, np.inf, np.where((g > 0) & (gs > 0), t, -1.0))


def _below(d, tau):
    """d < tau, three-valued: (certainly, possibly)"""
    d = d.astype(np.float64)
    return d < tau * (1 - BAND), d < tau * (1 + BAND)


def plan(desc, sup, q, K, d2, n1=0, e2=None):
    """One job: queries q against the support set sup on the grid `desc` (the device's).  d2 = nearest_d2(sup, q, K).  n1 > 0: the fused K = 1 job over the
    first n1 support points, e2 = nearest_d2(sup[:n1], q, 1).  Per-query boolean arrays; *_lo are certain, *_hi possible."""
    k = constants()
    assert desc["n"] == len(sup)
    nq = len(q)
    cc = _cells(desc, q)
    sc = _cells(desc, sup)
    nx, ny, nz = desc["nx"], desc["ny"], desc["nz"]
    cum = np.concatenate([[0], np.cumsum(np.bincount((sc[2] * ny + sc[1]) * nx + sc[0], minlength=nx * ny * nz))])
    # rows of cells of the 3^3 block: populations -> long rows (exact)
    x0, x1 = np.maximum(cc[0] - 1, 0), np.minimum(cc[0] + 1, nx - 1)
    long_row = np.zeros(nq, bool)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            z, y = cc[2] + dz, cc[1] + dy
            ok = (z >= 0) & (z < nz) & (y >= 0) & (y < ny)
            row = (np.clip(z, 0, nz - 1) * ny + np.clip(y, 0, ny - 1)) * nx
            long_row |= ok & (cum[row + x1 + 1] - cum[row + x0] > k.MASK)
    tau = [_tau(desc, q, cc, R) for R in range(1, k.GS_RMAX + 1)]
    few = len(sup) < K + 1
    dK = d2[:, K]
    st2 = long_row | (tau[0] < 0)
    in1_lo, in1_hi = _below(dK, tau[0])
    p = SimpleNamespace(nq=nq, cells=cc, long_row=long_row, st2=st2, tau=tau)
    p.first_final = ~st2 & in1_lo                       # certain rows of "first pass final"
    p.retry_lo, p.retry_hi = st2 | ~in1_hi, st2 | ~in1_lo
    p.too_few_marks = ~st2 & ~in1_hi                    # certain rows the 3^3 block leaves with fewer than K + 1 marks
    s_lo, s_hi = [], []
    for R in range(k.GS_RMAX):
        lo, hi = _below(dK, tau[R])
        whole = np.isinf(tau[R])
        s_lo.append((lo | whole) & (not few)); s_hi.append((hi | whole) & (not few))
    p.settled_at = [s_lo[0], ~s_hi[0] & s_lo[1], ~s_hi[0] & ~s_hi[1] & s_lo[2]]      # certain rows settled at 3^3, 5^3, 7^3
    p.unsettled_lo = ~(s_hi[0] | s_hi[1] | s_hi[2])
    p.unsettled_hi = ~(s_lo[0] | s_lo[1] | s_lo[2])
    border = np.zeros(nq, bool)
    for R in range(k.GS_RMAX):
        border |= s_lo[R] != s_hi[R]
    if n1 > 0:
        e0, e1 = e2[:, 0], e2[:, 1]
        clear = e0 * k.NEAR_TIE < e1                    # float32, as the device multiplies
        a_lo, a_hi = _below(e0, tau[0])
        b_lo, b_hi = _below(e0 * k.NEAR_TIE, tau[0])
        p.fused_lo, p.fused_hi = ~st2 & clear & a_lo & b_lo, ~st2 & clear & a_hi & b_hi
        border |= p.fused_lo != p.fused_hi
    p.borderline = border
    return p


def work_cap(total_queries):
    """grid_set_jobs: every list holds one entry per query of every job at least, so status 8 (list overflow) cannot happen"""
    cap = min(max(total_queries, 1024), 0x3fffffff)
    assert cap >= total_queries
    return cap


def launches(backend, total_queries, max_n, handed, retried):
    """host arithmetic of kd_search_worklist (rows per wave), grid_search's retry launch (a second trip of its stride loop) and launch_build (which
    kernels split the big nodes; which form a complete rebuild takes).  handed / retried: (lower, upper) bounds of the list lengths."""
    k = constants()
    cu = NUM_CU[backend]
    cap = work_cap(total_queries)
    wl_grid = max(1, min(cap // 64 + 1, cu * 8))
    r_grid = max(1, min(cap // 64 + 1, cu * 16))
    L = SimpleNamespace(work_cap=cap, wl_grid=wl_grid, retry_grid=r_grid)
    L.rows_per_wave = 4 if handed[1] <= wl_grid * 4 else 64 if handed[0] > wl_grid * 4 else None
    L.retry_second_trip = True if retried[0] > r_grid * (64 // k.RL) else False if retried[1] <= r_grid * (64 // k.RL) else None
    build, balanced = [], 0
    while (max_n >> balanced) > k.SMALL_MAX:
        balanced += 1
    for level in range(k.BIG_LEVELS):
        if max_n <= k.SMALL_MAX:
            break
        if level >= balanced + 2:
            build.append("kd_rest_kernel"); break
        build.append("kd_split_kernel<512>" if (max_n >> level) > 1024 else "kd_split_kernel<256>")
    L.build = build
    one_wg = max_n <= 64 * (k.TREE_Q // 4)
    L.rebuild = "one workgroup per tree" if one_wg else "level-wide"
    L.rebuild_levels = backend == "gpu" and one_wg and max_n > k.ONE_WG_MAX      # kd_levels_kernel beside kd_tree_kernel (product build only)
    return L


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------------
BOX = np.array([4.0, 3.0, 2.0])


def uniform(seed, n=2048):
    return (np.random.default_rng(seed).random((n, 3)) * BOX).astype(np.float32)


def padded_lattice(seed, n=2048, dup=300, lat=100):
    """a tile padded by duplication (the last `dup` points repeat the first) with `lat` points rounded to 1/8, shuffled: a pyramid's levels are prefixes"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * BOX
    p[dup:dup + lat] = np.round(p[dup:dup + lat] * 8) / 8
    p[n - dup:] = p[:dup]
    return p[rng.permutation(n)].astype(np.float32)


def few_duplicates(seed, n=2048, dup=6):
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * BOX
    p[n - dup:] = p[:dup]
    return p[rng.permutation(n)].astype(np.float32)


def near_tie(seed, n=2048, groups=55):
    """2 * `groups` isolated groups of 17 points; the first point of a group is its query: fourteen neighbours inside 0.8 r, the 16th at (r, 0, 0)
    (r = 1/8 and seats on multiples of 1/4: exact in float32, squared distance 2^-6) and the 17th on the other side of the x axis, at the float32
    coordinate, found by stepping through the neighbouring floats, whose float32 squared distance lies in (1, NEAR_TIE] times the 16th's (the first
    `groups` groups) or in (NEAR_TIE, 1 + 4 * 2^-17] times it (the others).  The rest of the cloud is uniform in a layer the groups' balls do not reach.
    Returns the cloud, the number of groups and their size (the queries are the points 0, 17, 34, ...)."""
    rng = np.random.default_rng(seed)
    k = constants()
    r = F32(0.125)
    d16 = r * r
    pts = []
    for gi in range(2 * groups):
        o = np.array([0.25 + 0.5 * (gi % 8), 0.25 + 0.5 * ((gi // 8) % 6), 0.25 + 0.5 * (gi // 48)], np.float32)
        xs = [o[0] - r]
        for _ in range(96):
            xs.append(np.nextafter(xs[-1], F32(-1e9), dtype=np.float32))
        xs = np.array(xs, np.float32)
        dx = o[0] - xs
        d17 = dx * dx
        assert d17.dtype == np.float32
        near = (d17 > d16) & (d17 <= d16 * k.NEAR_TIE)
        hit = near if gi < groups else (d17 > d16 * k.NEAR_TIE) & (d17.astype(np.float64) <= float(d16) * (1 + 4 * 2.0 ** -17))
        assert hit.any(), "no float32 coordinate gives the wanted ratio at x = %g" % o[0]
        grp = [o.copy()]
        for i in range(14):
            v = rng.normal(size=3); v *= (0.2 + 0.6 * (i + 1) / 16.0) * float(r) / np.linalg.norm(v)
            grp.append((o.astype(np.float64) + v).astype(np.float32))
        grp.append(o + np.array([r, 0, 0], np.float32))
        grp.append(np.array([rng.choice(xs[hit]), o[1], o[2]], np.float32))
        pts.append(np.stack(grp))
    g = np.concatenate(pts)
    rest = rng.random((n - len(g), 3)) * BOX * [1, 1, 0.1] + [0, 0, 1.8]
    return np.concatenate([g, rest.astype(np.float32)]).astype(np.float32), 2 * groups, 17


def dense_clump(seed, n=2048, m=300):
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * BOX
    p[:m] = BOX * 0.5 + 1e-3 * rng.random((m, 3))
    return p[rng.permutation(n)].astype(np.float32)


def corner_groups(seed, n=2048):
    """a dense core in the middle of the box (its cells are a few: the table's size, not the measured radius, decides the cell), groups of 5 points at
    the eight corners (fewer than K + 1 anywhere near: unsettled) and 24 isolated pairs of 9-point groups whose distance grows from 0.1 to 0.675 in
    steps of 0.025: a row of such a group finds its 17th neighbour in the other group, so whatever cell between 0.08 and 0.2 the device chooses some
    pairs settle in the 5^3 block, some in the 7^3 block and some not at all"""
    rng = np.random.default_rng(seed)
    p = BOX * 0.5 + 0.15 * rng.random((n, 3))
    corners = np.array([[i, j, kk] for i in (0, 1) for j in (0, 1) for kk in (0, 1)], np.float64) * BOX
    p[:40] = np.repeat(corners, 5, 0) + 0.05 * rng.random((40, 3))
    for i in range(24):
        seat = np.array([0.45 + 0.9 * (i % 4), 0.5 + 0.9 * ((i // 4) % 3), 0.15 if i < 12 else 1.85])
        at = 40 + 18 * i
        p[at: at + 9] = seat + 0.01 * rng.random((9, 3))
        p[at + 9: at + 18] = seat + [0.1 + 0.025 * i, 0, 0] + 0.01 * rng.random((9, 3))
    return p[rng.permutation(n)].astype(np.float32)


def places_copies(seed, places=100, copies=30, extent=1000.0):
    rng = np.random.default_rng(seed)
    p = np.repeat(rng.random((places, 3)) * extent, copies, 0)
    return p[rng.permutation(len(p))].astype(np.float32)


def two_clumps(seed, n=2048, far=5000.0):
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * BOX
    p[n // 2:, 0] += far
    return p[rng.permutation(n)].astype(np.float32)


def layered(seed, n=2048):
    rng = np.random.default_rng(seed)
    sizes = [1500, 450, n - 1950]
    p = np.concatenate([np.concatenate([rng.random((m, 2)) * BOX[:2], z + 0.01 * rng.random((m, 1))], 1) for m, z in zip(sizes, (0.0, 0.35, 0.9))])
    return p[rng.permutation(n)].astype(np.float32)
