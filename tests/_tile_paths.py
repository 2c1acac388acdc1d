"""Helpers of tests/test_tile_paths.py: the constants of the tile generator read from csrc/tile.hip, the float32 oracle of a tile (the NumPy restatement of
tests/test_tile.py: stable argsort of the float32 keys, ties by index), a NumPy restatement of what tile_hist_b / tile_thresh_b make of a room (`plan`: the
threshold bin, the candidates, the sort ranges and their sizes, hence the branch of tile_binsort_b each range takes; the cases assert their input conditions
with it BEFORE the library is called), the varying key bytes that decide the executed digit passes of the single flavour's radix sort, the builders of the
rooms the cases are made of, and the callers of ssdr_tile_select_batch_dev / ssdr_tile_select_possibility_dev / ssdr_tile_select_dev.  Nothing here touches a
device except the callers.

A call (`make_call`) is a SimpleNamespace: rooms (float32 [n_r, 3] each; n_r is the host's row bound), centres float32 [R, 3], N (num_points), m (the
device row counts d_m, default n_r), perm int32 [R, N], dup float32 [R, N], col float32 [sum n_r, 3], lab int32 [sum n_r]."""
import os
import re
from types import SimpleNamespace

import numpy as np

from conftest import assert_bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ssdr-al_amd", "csrc")
F32 = np.float32
SCALE = 1.0 / 255.0
SENTINEL_F, SENTINEL_I = F32(-77.25), -77
ERR_INVALID = 1                                   # SSDR_ERR_INVALID (include/ssdr_al.h)
MAX_ROOMS = 64                                    # RADIX_MAX_SEG (csrc/ssdr_internal.hpp)


# ---- constants, from the source -------------------------------------------------------------------------------------------------------------------
_CONSTANTS = None


def constants():
    """TS_BITS, TS_RSTEP, TS_RCAP, TS_RMAX (csrc/tile.hip) and what follows from them: a changed constant moves the shapes of the cases with it, a definition the
    pattern no longer finds fails here"""
    global _CONSTANTS
    if _CONSTANTS is None:
        path = os.path.join(CSRC, "tile.hip")
        with open(path) as f:
            text = f.read()
        out = {}
        for nm in ("TS_BITS", "TS_RSTEP", "TS_RCAP", "TS_RMAX"):
            m = re.findall(r"\b%s\s*=\s*([0-9]+)\s*[,;]" % nm, text)
            assert len(m) == 1, "%s: expected one definition of %s, found %d" % (path, nm, len(m))
            out[nm] = int(m[0])
        out["TS_BINS"] = 1 << out["TS_BITS"]
        out["TS_SHIFT"] = 31 - out["TS_BITS"]
        _CONSTANTS = SimpleNamespace(**out)
    return _CONSTANTS


# ---- keys, oracle -----------------------------------------------------------------------------------------------------------------------------------
def keys(points, centre):
    """the float32 sort keys: (dx*dx + dy*dy) + dz*dz, every operation rounded to float32 (an overflow to +inf is a value like any other)"""
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.asarray(points, F32) - np.asarray(centre, F32)[None]
        return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F32)


def oracle_rows(points, centre, N, m, perm, dup):
    """the source rows of a tile, index for index: the min(m, N) nearest of the first m rows (stable: ties by index) through the shuffle; a room smaller
    than the tile is its rows through the entries of perm below m, then duplicates of that list"""
    order = np.argsort(keys(points[:m], centre), kind="stable")[:min(m, N)]
    if m >= N:
        return order[perm]
    shuffled = order[perm[perm < m]]
    pick = np.minimum((dup[m:] * F32(m)).astype(np.int64), m - 1)
    return np.concatenate([shuffled, shuffled[pick]])


def oracle_tile(points, colors, labels, centre, N, m, perm, dup):
    """-> dict(idx, xyz, feat, lab) of one room; colors / labels may be None"""
    rows = oracle_rows(points, centre, N, m, perm, dup)
    with np.errstate(over="ignore", invalid="ignore"):
        xyz = (points[rows] - np.asarray(centre, F32)[None]).astype(F32)
    out = dict(idx=rows.astype(np.int32), xyz=xyz)
    out["feat"] = xyz if colors is None else np.concatenate([xyz, (colors[rows] * F32(SCALE)).astype(F32)], 1)
    out["lab"] = None if labels is None else labels[rows]
    return out


def oracle_possibility(points, centre, N, m, possibility):
    """the map after the update of tile_possibility: the avail = min(m, N) nearest rows gain (1 - d / dmax)^2, d and the quotient in float32, dmax = the key
    of the farthest of them; -> (map, min over the first m rows, its first arg-min)"""
    key = keys(points[:m], centre)
    rows = np.argsort(key, kind="stable")[:min(m, N)]
    d = key[rows]
    q = (F32(1) - d / d[-1]).astype(F32)
    out = possibility.copy()
    out[rows] += (q * q).astype(F32).astype(np.float64)
    return out, out[:m].min(), int(np.argmin(out[:m]))


# ---- plan: what tile_hist_b / tile_thresh_b make of a room ---------------------------------------------------------------------------------------------
def sort_path(n):
    """the branch of tile_binsort_b a range of n words takes"""
    k = constants()
    if n <= 1:
        return "none"
    N = 2
    while N < n:
        N <<= 1
    if 16 <= N <= 2048:
        return "registers"
    return "lds" if n <= k.TS_RCAP else "global"


def rstride(sizes):
    """the range-table stride of a call over rooms of these host row bounds"""
    k = constants()
    return (max(sizes) + k.TS_RSTEP - 1) // k.TS_RSTEP + 1


def plan(points, centre, N, m):
    """-> T (the first bin whose cumulative count reaches min(N, m)), cand (the rows of the bins <= T), ranges (the sizes n of the sort ranges, in order: range
    k = the bins that START in [k TS_RSTEP, (k + 1) TS_RSTEP) of the candidates), paths (sort_path of each), nk (the range table's live entries), holes (the
    entries < nk where no bin starts: RS[q] == 0xffffffff), bins (the occupied bins <= T)"""
    k = constants()
    bits = keys(points[:m], centre).view(np.uint32) & np.uint32(0x7fffffff)
    cnt = np.bincount((bits >> np.uint32(k.TS_SHIFT)).astype(np.int64), minlength=k.TS_BINS)
    want = min(N, m)
    cum = np.cumsum(cnt)
    T = int(np.searchsorted(cum, want)) if want > 0 else 0
    cand = int(cum[T])
    occupied = np.flatnonzero(cnt[:T + 1])
    start = (cum - cnt)[occupied]
    rid = start // k.TS_RSTEP
    first = np.array(sorted({int(r): int(s) for r, s in zip(rid[::-1], start[::-1])}.items()), np.int64).reshape(-1, 2)      # range id -> its lowest bin start
    edges = np.concatenate([first[:, 1], [cand]])
    ranges = [int(x) for x in np.diff(edges)]
    nk = (cand + k.TS_RSTEP - 1) // k.TS_RSTEP
    holes = sorted(set(range(nk)) - set(int(r) for r in first[:, 0]))
    return SimpleNamespace(T=T, cand=cand, ranges=ranges, paths=[sort_path(n) for n in ranges], nk=nk, holes=holes, bins=[int(b) for b in occupied])


def varying_bytes(points, centre, m=None):
    """the bytes of the float32 key patterns that differ between rows: the digit passes the single flavour's radix sort executes (rs_andor)"""
    bits = keys(points[:m], centre).view(np.uint32)
    diff = int(np.bitwise_and.reduce(bits)) ^ int(np.bitwise_or.reduce(bits))
    return {b for b in range(4) if (diff >> (8 * b)) & 0xff}


# ---- builders ------------------------------------------------------------------------------------------------------------------------------------------
def one_bin_room(rng, n, scale=1.0):
    """n rows around the origin with r^2 in [4, 4.0625) * scale^2: one distance bin (8256 at scale 1), hence one sort range of exactly n words; the second half
    mirrors the first in x: exact ties in pairs"""
    h = (n + 1) // 2
    d = rng.normal(size=(h, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = (d * (2.001 + rng.random((h, 1)) * 0.012)).astype(F32)
    q = p[:n - h].copy()
    q[:, 0] = -q[:, 0]
    out = np.concatenate([p, q])[rng.permutation(n)]
    return (out * F32(scale)).astype(F32)


def box_room(rng, n, box=(8.0, 6.0, 3.0)):
    """n uniform rows in a box, the centre near one of them -> (points, centre)"""
    p = (rng.random((n, 3), dtype=F32) * np.array(box, F32)).astype(F32)
    c = (p[int(rng.integers(n))] + rng.normal(0, 0.35, 3)).astype(F32)
    return p, c


def lattice(rng, side, step):
    """side^3 lattice points around the origin, shuffled: many exactly equal distances"""
    h = side // 2
    g = np.stack(np.meshgrid(*[np.arange(-h, side - h)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(F32) * F32(step)
    return g[rng.permutation(len(g))]


def _three_squares(vals):
    """integer (a, b, c) with a^2 + b^2 + c^2 = v for every v (none of the form 4^a (8 b + 7))"""
    vals = np.asarray(vals, np.int64)
    top = int(np.sqrt(vals.max())) + 1
    b, c = np.meshgrid(np.arange(top + 1), np.arange(top + 1), indexing="ij")
    s = (b * b + c * c).ravel()
    two = np.full(int(s.max()) + 1, -1, np.int64)
    two[s] = np.arange(len(s))                      # any representation as two squares
    a = np.floor(np.sqrt(vals.astype(np.float64))).astype(np.int64)
    a[a * a > vals] -= 1
    todo = two[vals - a * a] < 0
    while todo.any():
        a[todo] -= 1
        assert (a >= 0).all()
        todo = two[vals - a * a] < 0
    rep = two[vals - a * a]
    return np.stack([a, rep // (top + 1), rep % (top + 1)], 1)


def _is_three_squares(v):
    v = np.asarray(v, np.int64).copy()
    assert (v > 0).all()
    while (v % 4 == 0).any():
        v[v % 4 == 0] //= 4
    return v % 8 != 7


def integer_room(rng, lo, hi, unit=1, stride=1):
    """rows with integer coordinates (multiples of `unit`) whose squared distances from the origin are the values unit^2 * k, k = lo/unit^2 ... hi/unit^2 - 1 in
    steps of `stride` (those that are sums of three squares), exact in float32; a third of the rows duplicated, signs and order shuffled"""
    u2 = unit * unit
    k = np.arange(lo // u2, hi // u2, stride, dtype=np.int64)
    k = np.unique(np.concatenate([k, [lo // u2 + 1, hi // u2 - 1]]))
    k = k[_is_three_squares(k)]
    p = _three_squares(k) * unit
    p = np.concatenate([p, p[rng.integers(0, len(p), len(p) // 3)]])
    p = p * rng.choice([-1, 1], p.shape)
    p = np.take_along_axis(p, np.argsort(rng.random(p.shape), axis=1), 1)
    out = p[rng.permutation(len(p))].astype(F32)
    d2 = (out.astype(np.float64) ** 2).sum(1)
    assert d2.min() >= lo and d2.max() < hi and (keys(out, np.zeros(3, F32)) == d2).all()
    return out


# ---- calls ---------------------------------------------------------------------------------------------------------------------------------------------
def make_call(rng, rooms, centres, N, m=None, colors=True, labels=True):
    """draws the shuffles, the duplicate choices (dup_u = 0 in the row before the last and 1.0 in the last: the only value that reaches the clamp to m - 1), the
    colours and the labels"""
    R, sizes = len(rooms), [len(p) for p in rooms]
    tot = sum(sizes)
    dup = rng.random((R, N)).astype(F32)
    dup[:, -1] = 1.0
    if N > 1:
        dup[:, -2] = 0.0
    return SimpleNamespace(rooms=[np.ascontiguousarray(p, F32) for p in rooms], centres=np.ascontiguousarray(np.asarray(centres, F32).reshape(R, 3)), N=int(N),
                           m=[int(x) for x in (sizes if m is None else m)], sizes=sizes, off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                           perm=np.stack([rng.permutation(N) for _ in range(R)]).astype(np.int32), dup=dup,
                           col=rng.integers(0, 256, (tot, 3)).astype(F32) if colors else None, lab=rng.integers(0, 13, tot).astype(np.int32) if labels else None)


def expected(call):
    out = []
    for r, p in enumerate(call.rooms):
        if call.m[r] == 0:
            out.append(None)
            continue
        o = int(call.off[r])
        out.append(oracle_tile(p, None if call.col is None else call.col[o:o + len(p)], None if call.lab is None else call.lab[o:o + len(p)],
                               call.centres[r], call.N, call.m[r], call.perm[r], call.dup[r]))
    return out


def run_batch(call, stream=None, feat=True, idx=True, lab=None, colors=True, labels_in=True, cdim=None, off=None, num_clouds=None, N=None, expect=0):
    """ssdr_tile_select_batch_dev; the outputs are prefilled with a sentinel; feat / idx / lab False: that output NULL; colors False: the colours NULL and
    color_dim 0 (or `cdim`); labels_in False: the labels NULL; off / num_clouds / N: what the call is told in place of the call's own.
    -> dict(xyz [R, N, 3], feat [R, N, 3 + cdim] | None, idx [R, N] | None, lab [R, N] | None); expect: the status the call must return"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    L = _lib.lib()
    R, n = len(call.rooms), call.N
    colors = colors and call.col is not None
    labels_in = labels_in and call.lab is not None
    lab = labels_in if lab is None else lab
    cdim = (3 if colors else 0) if cdim is None else cdim
    up = lambda a: DevArray.from_host(a, stream=stream)
    d_p = up(np.concatenate(call.rooms))
    d_c = up(call.col) if colors else None
    d_l = up(call.lab) if labels_in else None
    d_m = up(np.array(call.m + [0], np.int64))
    d_perm, d_dup = up(call.perm), up(call.dup)
    o_xyz = up(np.full((R, n, 3), SENTINEL_F, F32))
    o_feat = up(np.full((R, n, 3 + cdim), SENTINEL_F, F32)) if feat else None
    o_idx = up(np.full((R, n), SENTINEL_I, np.int32)) if idx else None
    o_lab = up(np.full((R, n), SENTINEL_I, np.int32)) if lab else None
    dp = lambda d: None if d is None else d.ptr
    offsets = np.ascontiguousarray(call.off if off is None else off, np.int64)
    rc = L.ssdr_tile_select_batch_dev(d_p.ptr, dp(d_c), cdim, d_m.ptr, _lib.ptr(offsets), R if num_clouds is None else num_clouds, _lib.ptr(call.centres),
                                      n if N is None else N, d_perm.ptr, d_dup.ptr, SCALE, o_xyz.ptr, dp(o_feat), dp(o_idx), dp(d_l), dp(o_lab), stream)
    assert rc == expect, "status %d, expected %d: %s" % (rc, expect, L.ssdr_last_error().decode())
    down = lambda d: None if d is None else d.to_host(stream=stream)
    return dict(xyz=down(o_xyz), feat=down(o_feat), idx=down(o_idx), lab=down(o_lab))


def run_single(points, colors, centre, N, m, perm, dup, possibility=None, with_min=True, feat=True, idx=True, plain=False):
    """ssdr_tile_select_possibility_dev (plain: ssdr_tile_select_dev) of one cloud -> dict(xyz, feat, idx, poss, min, arg)"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    L = _lib.lib()
    n = len(points)
    cdim = 0 if colors is None else 3
    d_p, d_c = DevArray.from_host(points), (None if colors is None else DevArray.from_host(colors))
    d_m = DevArray.from_host(np.array([m, 0], np.int64))
    d_perm, d_dup = DevArray.from_host(perm), DevArray.from_host(dup)
    o_xyz = DevArray.from_host(np.full((N, 3), SENTINEL_F, F32))
    o_feat = DevArray.from_host(np.full((N, 3 + cdim), SENTINEL_F, F32)) if feat else None
    o_idx = DevArray.from_host(np.full((N,), SENTINEL_I, np.int32)) if idx else None
    d_poss = None if possibility is None else DevArray.from_host(possibility)
    d_min, d_arg = DevArray.from_host(np.array([7.5], np.float64)), DevArray.from_host(np.array([SENTINEL_I], np.int32))
    dp = lambda d: None if d is None else d.ptr
    centre = np.ascontiguousarray(centre, F32)
    if plain:
        _lib.check(L.ssdr_tile_select_dev(d_p.ptr, dp(d_c), cdim, d_m.ptr, n, _lib.ptr(centre), N, d_perm.ptr, d_dup.ptr, SCALE, o_xyz.ptr, dp(o_feat), dp(o_idx), None))
    else:
        use_min = with_min and d_poss is not None
        _lib.check(L.ssdr_tile_select_possibility_dev(d_p.ptr, dp(d_c), cdim, d_m.ptr, n, _lib.ptr(centre), N, d_perm.ptr, d_dup.ptr, SCALE, o_xyz.ptr, dp(o_feat), dp(o_idx),
                                                      dp(d_poss), d_min.ptr if use_min else None, d_arg.ptr if use_min else None, None))
    _lib.sync()
    down = lambda d: None if d is None else d.to_host()
    return dict(xyz=down(o_xyz), feat=down(o_feat), idx=down(o_idx), poss=down(d_poss), min=d_min.to_host()[0], arg=int(d_arg.to_host()[0]))


def same_tile(got, exp, what, r=None):
    """every present output of room r of a batch result (r None: a single-cloud result) against the oracle's tile: indices one for one, the rest bit for bit"""
    pick = (lambda a: a) if r is None else (lambda a: a[r])
    if got["idx"] is not None:
        bad = np.flatnonzero(pick(got["idx"]) != exp["idx"])
        assert len(bad) == 0, "%s: %d of %d source rows differ, first at row %d (%d, oracle %d)" % (
            what, len(bad), len(exp["idx"]), bad[0], pick(got["idx"])[bad[0]], exp["idx"][bad[0]])
    assert_bits_equal(pick(got["xyz"]), exp["xyz"], what + " xyz")
    if got["feat"] is not None:
        assert_bits_equal(pick(got["feat"]), exp["feat"][:, :pick(got["feat"]).shape[1]], what + " features")
    if got.get("lab") is not None:
        assert np.array_equal(pick(got["lab"]), exp["lab"]), what + " labels"


def check_batch(call, got, exp=None, what="room"):
    exp = expected(call) if exp is None else exp
    for r in range(len(call.rooms)):
        if exp[r] is None:
            untouched(got, r, "%s %d (empty)" % (what, r))
        else:
            same_tile(got, exp[r], "%s %d" % (what, r), r)
    return exp


def untouched(got, r, what):
    """room r of a batch result (r None: a single-cloud result) still holds the sentinel in every present output"""
    for name, val in got.items():
        if val is None or name in ("poss", "min", "arg"):
            continue
        a = val if r is None else val[r]
        assert (a == (SENTINEL_F if a.dtype == F32 else SENTINEL_I)).all(), "%s: %s was written" % (what, name)


def same_results(a, b, what):
    for name in a:
        assert (a[name] is None) == (b[name] is None), what
        if a[name] is not None:
            assert_bits_equal(a[name], b[name], "%s %s" % (what, name))
