"""Helpers of tests/test_score_paths.py: the constants of the scoring and ranking kernels read from the sources, a NumPy restatement of which branch of
csrc/select.hip a case takes (`plan_*`: the cases assert their input conditions with them BEFORE the library is called), the comparison of floats on their
bits (float32 as uint32, float64 as uint64: a signed zero or a NaN's payload is a difference), and the callers of the entry points.  Nothing here touches a
device except the callers.

Superpoints are a CSR pair (off int32 [S + 1], pts int32 [T]): region s holds the points pts[off[s]:off[s + 1]], in that order (the order matters: the sums
follow NumPy's pairwise order over the members as listed)."""
import os
import re
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ssdr-al_amd", "csrc")
NEG_INF_BITS = np.uint64(0xfff0000000000000)


# ---- constants, from the sources ----------------------------------------------------------------------------------------------------------------
def _one(pattern, text, path):
    m = re.findall(pattern, text)
    assert len(m) == 1, "%s: expected one match of %r, found %d" % (path, pattern, len(m))
    return int(m[0])


def _read(*parts):
    path = os.path.join(*parts)
    with open(path) as f:
        return f.read(), path


_CONSTANTS = None


def constants():
    """RS_CAP, NP_BUFSIZE, RANK_SMALL (select.hip), RADIX_WIDE (radix_sort.hip: from this many keys on the high passes run one by one), GRID_CAP (grid_for's
    default cap, select_fps.hpp), CU_GPU / CU_EMU (the CU count the launchers size their grids by: the MI355X's, which is also ssdr_internal.hpp's default, and
    what the CPU logic build's hipDeviceGetAttribute answers).  A changed constant moves the shapes with it, a definition the pattern misses fails here."""
    global _CONSTANTS
    if _CONSTANTS is None:
        out = {}
        text, path = _read(CSRC, "select.hip")
        for nm in ("RS_CAP", "NP_BUFSIZE", "RANK_SMALL"):
            out[nm] = _one(r"\b%s\s*=\s*(\d+)\s*[,;]" % nm, text, path)
        out["WAVE_GRID"] = _one(r"sel_region_stats_w, dim3\(\(unsigned\)std::min<size_t>\(\(S \+ 3\) / 4, \(size_t\)ctx\(\)\.num_cu \* (\d+)\)\)", text, path)
        out["DOM_GRID"] = _one(r"sel_dominant_label, dim3\(\(unsigned\)std::min<size_t>\(\(S \+ 3\) / 4, \(size_t\)ctx\(\)\.num_cu \* (\d+)\)\)", text, path)
        text, path = _read(CSRC, "radix_sort.hip")
        out["RADIX_WIDE"] = _one(r"key_bits > 32 && maxn >= (\d+);", text, path)
        text, path = _read(CSRC, "select_fps.hpp")
        out["GRID_CAP"] = _one(r"inline int grid_for\(long n, int cap = (\d+)\)", text, path)
        text, path = _read(CSRC, "ssdr_internal.hpp")
        out["CU_GPU"] = _one(r"int num_cu = (\d+);", text, path)
        text, path = _read(ROOT, "tests", "hipemu", "hip", "hip_runtime.h")
        out["CU_EMU"] = _one(r"hipDeviceGetAttribute\(int\* v, int, int\) \{ \*v = (\d+);", text, path)
        _CONSTANTS = SimpleNamespace(**out)
    return _CONSTANTS


def num_cu(backend):
    K = constants()
    return K.CU_EMU if backend == "emu" else K.CU_GPU


# ---- bits -----------------------------------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s vs %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = bits(got) != bits(want)
    if bad.any():
        k = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements differ on their bits, first at %s: %r vs %r" % (what, bad.sum(), bad.size, k, got[k], want[k]))


# ---- which branch a case takes ----------------------------------------------------------------------------------------------------------------------
def plan_point(n, C):
    """sel_point_unc: the rows staged in LDS (C <= 32) or read in place; the grid and how often a workgroup comes round; rows of the last block"""
    K = constants()
    blocks = -(-n // 256)
    grid = max(1, min(blocks, K.GRID_CAP))
    return SimpleNamespace(staged=C <= 32, grid=grid, trips=-(-blocks // grid), tail=n - 256 * (blocks - 1))


def plan_region(sizes, cu):
    """sel_region_stats_w, region by region: "empty" | "lane" (fewer than 8 members: lane 0's plain loop) | "w8" (staged, the eight accumulators on eight
    lanes; `blocks` > 1: the pairwise recursion splits) | "chunked" (above RS_CAP: nodes of at most RS_CAP staged one after the other; `buffers`: NumPy's
    pieces of NP_BUFSIZE); trips: how often a wave comes round"""
    K = constants()
    sizes = np.asarray(sizes, np.int64)
    S = len(sizes)
    branch = np.where(sizes <= 0, "empty", np.where(sizes < 8, "lane", np.where(sizes <= K.RS_CAP, "w8", "chunked")))
    grid = max(1, min((S + 3) // 4, cu * K.WAVE_GRID))
    return SimpleNamespace(branch=branch, blocks=np.where(sizes > 128, 2, 1), buffers=-(-sizes // K.NP_BUFSIZE), grid=grid, trips=-(-((S + 3) // 4) // grid),
                           tail_waves=S % 4)


def plan_dominant(sizes, cu):
    """sel_dominant_label: a lane's trips over the members (four members, 64 apart, per trip), and the wave loop's"""
    K = constants()
    sizes = np.asarray(sizes, np.int64)
    S = len(sizes)
    grid = max(1, min((S + 3) // 4, cu * K.DOM_GRID))
    return SimpleNamespace(member_trips=-(-sizes // 256), grid=grid, trips=-(-((S + 3) // 4) // grid))


def plan_clsbal(S, n_selected, skip):
    """sel_class_hist / sel_clsbal: the regions that enter the histogram; len(list_class) given by the host (no mask) or summed from the histogram (a mask)"""
    K = constants()
    counted = S - (0 if skip is None else int(np.count_nonzero(skip))) + n_selected
    return SimpleNamespace(total_from_hist=skip is not None, counted=counted, hist_grid=max(1, min(-(-(S + n_selected) // 256), K.GRID_CAP)))


def plan_mask(S, S_padded):
    """sel_mask_regions: rows behind S are padding; the last block's live lanes"""
    return SimpleNamespace(pad=S_padded - S, tail=(S_padded - 1) % 256 + 1)


def plan_segment(sizes):
    """sel_segment_mean: a thread's trips of 32 members; clipped: the last trip's loads are clamped to the region's last member"""
    sizes = np.asarray(sizes, np.int64)
    return SimpleNamespace(trips=-(-sizes // 32), clipped=sizes % 32 != 0)


def plan_rank(S):
    """ssdr_rank_regions_dev: "count" (sel_rank_count) up to RANK_SMALL, the radix sorter above: "radix" with the high passes in one kernel below RADIX_WIDE
    keys, "radix_wide" with every pass a launch from there on"""
    K = constants()
    return "count" if S <= K.RANK_SMALL else "radix" if S < K.RADIX_WIDE else "radix_wide"


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------
def csr(rng, sizes, n_points=None, permute=True):
    """regions of the given sizes over disjoint points -> (off, pts, n)"""
    sizes = np.asarray(sizes, np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(off[-1]) if n_points is None else n_points
    pts = (rng.permutation(n)[:off[-1]] if permute else np.arange(off[-1])).astype(np.int32)
    return off, pts, n


# ---- callers ----------------------------------------------------------------------------------------------------------------------------------------
def _L():
    from ssdr_al import _lib
    return _lib, _lib.lib(), _lib.DevArray


def point_uncertainty(probs, mode):
    """-> (unc float32 [n], cls int32 [n]); mode "lc" | "entropy" | "sb" """
    _lib, L, D = _L()
    n, C = probs.shape
    d_p, d_u, d_c = D.from_host(np.ascontiguousarray(probs, np.float32)), D((n,), np.float32), D((n,), np.int32)
    _lib.check(L.ssdr_point_uncertainty_dev(d_p.ptr, n, C, {"lc": 0, "entropy": 1, "sb": 2}[mode], d_u.ptr, d_c.ptr, None))
    _lib.sync()
    return d_u.to_host(), d_c.to_host()


def region_stats(unc, cls, off, pts, C, mode):
    """-> (region_unc float64 [S], dom int32 [S], dom_cnt int32 [S]); mode "mean" | "sum_weight" | "WetSU" """
    _lib, L, D = _L()
    S = len(off) - 1
    d = [D.from_host(np.ascontiguousarray(a, t)) for a, t in ((unc, np.float32), (cls, np.int32), (off, np.int32), (pts if len(pts) else np.zeros(1), np.int32))]
    d_r, d_d, d_n = D.from_host(np.full(S, 7.5)), D.from_host(np.full(S, -3, np.int32)), D.from_host(np.full(S, -3, np.int32))
    _lib.check(L.ssdr_region_stats_dev(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, S, C, {"mean": 0, "sum_weight": 1, "WetSU": 2}[mode], d_r.ptr, d_d.ptr, d_n.ptr, None))
    _lib.sync()
    return d_r.to_host(), d_d.to_host(), d_n.to_host()


def dominant_label(labels, off, pts, num_labels):
    _lib, L, D = _L()
    S = len(off) - 1
    d_l, d_o, d_p = D.from_host(np.ascontiguousarray(labels, np.int32)), D.from_host(np.ascontiguousarray(off, np.int32)), D.from_host(np.ascontiguousarray(pts, np.int32))
    d_lab, d_pur = D.from_host(np.full(S, -3, np.int32)), D.from_host(np.full(S, 7.5))
    _lib.check(L.ssdr_dominant_label_dev(d_l.ptr, d_o.ptr, d_p.ptr, S, num_labels, d_lab.ptr, d_pur.ptr, None))
    _lib.sync()
    return d_lab.to_host(), d_pur.to_host()


def clsbal(region_class, skip, selected, region_unc):
    """ssdr_clsbal_dev in one call -> region_unc (every region is scaled, the skipped ones included: they are masked later)"""
    _lib, L, D = _L()
    S = len(region_class)
    d_c, d_u = D.from_host(np.ascontiguousarray(region_class, np.int32)), D.from_host(np.ascontiguousarray(region_unc, np.float64))
    d_k = None if skip is None else D.from_host(np.ascontiguousarray(skip, np.uint8))
    d_s = None if not len(selected) else D.from_host(np.ascontiguousarray(selected, np.int32))
    _lib.check(L.ssdr_clsbal_dev(d_c.ptr, S, d_k.ptr if d_k else None, d_s.ptr if d_s else None, len(selected), d_u.ptr, None))
    _lib.sync()
    return d_u.to_host()


def clsbal_hist(region_class, skip, selected, region_unc):
    """the supplied-histogram flavour: ssdr_class_hist_dev, then ssdr_clsbal_hist_dev with the histogram's total -> (region_unc, hist int32 [64])"""
    _lib, L, D = _L()
    S = len(region_class)
    d_c, d_u = D.from_host(np.ascontiguousarray(region_class, np.int32)), D.from_host(np.ascontiguousarray(region_unc, np.float64))
    d_k = None if skip is None else D.from_host(np.ascontiguousarray(skip, np.uint8))
    d_s = None if not len(selected) else D.from_host(np.ascontiguousarray(selected, np.int32))
    d_h = D.from_host(np.full(64, -1, np.int32))
    _lib.check(L.ssdr_class_hist_dev(d_c.ptr, S, d_k.ptr if d_k else None, d_s.ptr if d_s else None, len(selected), d_h.ptr, None))
    _lib.sync()
    hist = d_h.to_host()
    _lib.check(L.ssdr_clsbal_hist_dev(d_c.ptr, S, d_h.ptr, int(hist.sum()), d_u.ptr, None))
    _lib.sync()
    return d_u.to_host(), hist


def mask_regions(u, labelled, S_padded):
    _lib, L, D = _L()
    d_u, d_l, d_o = D.from_host(np.ascontiguousarray(u, np.float64)), D.from_host(np.ascontiguousarray(labelled, np.uint8)), D.from_host(np.full(S_padded + 3, 7.5))
    _lib.check(L.ssdr_mask_regions_dev(d_u.ptr, d_l.ptr, len(u), S_padded, d_o.ptr, None))
    _lib.sync()
    return d_o.to_host()          # three words past the end: they must come back as they went in


def segment_mean(feat, cls, dom, off, pts, sel):
    """sel: region ids (int32) or None (the first len(off) - 1 regions) -> float32 [nsel, D]"""
    _lib, L, D = _L()
    nsel = len(off) - 1 if sel is None else len(sel)
    d = [D.from_host(np.ascontiguousarray(a, t)) for a, t in ((feat, np.float32), (cls, np.int32), (dom, np.int32), (off, np.int32), (pts, np.int32))]
    d_s = None if sel is None else D.from_host(np.ascontiguousarray(sel, np.int32))
    d_o = D.from_host(np.full((nsel, feat.shape[1]), 7.5, np.float32))
    _lib.check(L.ssdr_segment_mean_features_dev(d[0].ptr, feat.shape[1], d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d_s.ptr if d_s else None, nsel, d_o.ptr, None))
    _lib.sync()
    return d_o.to_host()


def rank_regions(u):
    _lib, L, D = _L()
    d_u, d_o = D.from_host(np.ascontiguousarray(u, np.float64)), D.from_host(np.full(len(u), -1, np.int32))
    _lib.check(L.ssdr_rank_regions_dev(d_u.ptr, len(u), d_o.ptr, None))
    _lib.sync()
    return d_o.to_host()
