"""Helpers of tests/test_cand_paths.py: the constants of the candidate rule and of the top-k kernel read from the sources, the ORACLE of the rule written as the
reference's plain loops (the `top` and `allr` dicts of sampler2.py:533-552 and allr[b][:2 * len(top[b])] of :745-753, as oracle/pipeline_np.py:
selection_round has them — not HotPath._candidates, the project's own vectorised restatement), a NumPy restatement of which branch of the cand_* kernels,
edcd_plan and topk_regions a case takes (`plan`, `plan_topk`: the cases assert their input conditions with them BEFORE the library is called), and the callers.
Nothing here touches a device except the callers.

A case of the rule is (order int32 [S]: the ranking of ALL regions; labelled uint8 [S]; base int32 [B + 1]: cloud c owns the regions base[c] .. base[c + 1] - 1;
batch_size).  Every region is ONE point, so that the graph behind the rule (bbox centres, chamfer means: all 0) costs nothing."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ssdr-al_amd", "csrc")
HEADER = 8                       # words of counts in front of the picks
SENTINEL = -777


# ---- constants, from the sources ----------------------------------------------------------------------------------------------------------------
_CONSTANTS = None


def constants():
    """CR_NT, CC_TILE (select.hip), TK_NT (select_region.hip), SLICE_DIV / SLICE_CAP (cand_slices: min(SLICE_CAP, max(1, (S / B) / SLICE_DIV)): the whole
    expression is matched, so a changed rule fails here rather than pass unseen), SCAN_NT (the 256 pieces of the one-workgroup prefix sums)"""
    global _CONSTANTS
    if _CONSTANTS is None:
        out = {}

        def one(pattern, text, path):
            m = re.findall(pattern, text)
            assert len(m) == 1, "%s: expected one match of %r, found %d" % (path, pattern, len(m))
            return m[0]
        path = os.path.join(CSRC, "select.hip")
        with open(path) as f:
            text = f.read()
        out["CR_NT"] = int(one(r"constexpr int CR_NT = (\d+);", text, path))
        out["CC_TILE"] = int(one(r"constexpr int CC_TILE = (\d+);", text, path))
        cap, div = one(r"cand_slices\(size_t S, size_t B\) \{ const size_t avg = S / std::max<size_t>\(B, 1\); "
                       r"return \(unsigned\)std::min<size_t>\((\d+), std::max<size_t>\(1, avg / (\d+)\)\); \}", text, path)
        out["SLICE_CAP"], out["SLICE_DIV"] = int(cap), int(div)
        path = os.path.join(CSRC, "select_region.hip")
        with open(path) as f:
            text = f.read()
        out["TK_NT"] = int(one(r"constexpr int TK_NT = (\d+);", text, path))
        out["SCAN_NT"] = 256
        _CONSTANTS = SimpleNamespace(**out)
    return _CONSTANTS


# ---- the oracle: the reference's loops ------------------------------------------------------------------------------------------------------------
def cloud_of(base, S):
    """the cloud of every region (empty clouds own nothing)"""
    return (np.searchsorted(np.asarray(base, np.int64), np.arange(S), side="right") - 1).astype(np.int64)


def rule_oracle(order, labelled, base, batch_size):
    """-> unl (the candidate list: cloud ascending, descending uncertainty inside a cloud), ntop [B], ncand [B], sampling_batch"""
    S, B = len(order), len(base) - 1
    cl = cloud_of(base, S)
    ref = [int(sp) for sp in order if not labelled[sp]]           # prediction(): only unlabelled regions are ranked
    batch_size = min(int(batch_size), len(ref))
    top, allr = {}, {}
    for i, sp in enumerate(ref):
        b = int(cl[sp])
        if i < batch_size:
            top.setdefault(b, []).append(sp)
        allr.setdefault(b, []).append(sp)
    unl, ntop, ncand = [], np.zeros(B, np.int64), np.zeros(B, np.int64)
    for b in sorted(top):
        take = allr[b][:2 * len(top[b])]
        unl += take
        ntop[b], ncand[b] = len(top[b]), len(take)
    return np.asarray(unl, np.int32), ntop, ncand, int(sum(len(v) for v in top.values()))


# ---- which branch a case takes ------------------------------------------------------------------------------------------------------------------------
def plan(order, labelled, base, batch_size):
    """cand_rank / cand_chunkscan / cand_cloud / cand_layout / edcd_plan, restated:
      nchunks, scan_per            chunks of CR_NT ranks; chunks per thread of the one-workgroup prefix sum (> 1 above 256 * CR_NT regions)
      dead_chunks, dead_waves      chunks / 64-rank waves of the ranking whose regions are all labelled
      slices                       cand_slices(S, B); early[c]: cloud c's upper slices return at once (slices > 1 and at most 256 * y regions for some y >= 1)
      n, tiles, padded             regions per cloud, its tiles of CC_TILE, whether its last tile is padded to a multiple of four
      nv, nt, take, capped         unlabelled regions, tops, candidates of a cloud; capped: 2 * nt > nv
      layout_per                   clouds per thread of cand_layout / edcd_plan (> 1 above 256 clouds)"""
    K = constants()
    S, B = len(order), len(base) - 1
    order, labelled, base = np.asarray(order, np.int64), np.asarray(labelled) != 0, np.asarray(base, np.int64)
    unl_rank = ~labelled[order]
    nchunks = -(-S // K.CR_NT)
    pad = np.concatenate([unl_rank, np.zeros(nchunks * K.CR_NT - S, bool)])
    dead_chunks = np.flatnonzero(~pad.reshape(nchunks, K.CR_NT).any(1) & (np.arange(nchunks) * K.CR_NT + K.CR_NT <= S))
    dead_waves = np.flatnonzero(~pad.reshape(-1, 64).any(1) & (np.arange(len(pad) // 64) * 64 + 64 <= S))
    pos = np.cumsum(unl_rank) - 1                                                       # place among the unlabelled, by rank
    lim = min(int(batch_size), S)
    is_top = np.zeros(S, bool); is_top[order[unl_rank & (pos < lim)]] = True
    cl = cloud_of(base, S)
    n = np.diff(base)
    nv = np.bincount(cl[~labelled], minlength=B)[:B]
    nt = np.bincount(cl[is_top], minlength=B)[:B]
    slices = int(min(K.SLICE_CAP, max(1, (S // max(B, 1)) // K.SLICE_DIV)))
    return SimpleNamespace(S=S, B=B, nchunks=nchunks, scan_per=-(-nchunks // K.SCAN_NT), dead_chunks=dead_chunks, dead_waves=dead_waves, slices=slices,
                           early=(n <= 256) & (slices > 1), n=n, tiles=-(-n // K.CC_TILE), padded=(n % K.CC_TILE) % 4 != 0, nv=nv, nt=nt,
                           take=np.minimum(2 * nt, nv), capped=2 * nt > nv, layout_per=-(-B // K.SCAN_NT))


def plan_topk(order, skip, batch_size):
    """topk_regions: chunks of TK_NT walked until the top is complete; dead_first: the first chunk holds skipped regions only; end_rank: the rank of the top's
    last entry (-1: an empty top), on_boundary: it is the last rank of a chunk"""
    K = constants()
    order, skip = np.asarray(order, np.int64), np.asarray(skip) != 0
    n = len(order)
    live = ~skip[order] if n else np.zeros(0, bool)
    pop = int(live.sum())
    top = min(int(batch_size), pop)
    end_rank = int(np.flatnonzero(live)[top - 1]) if top else -1
    run = np.concatenate([[0], np.cumsum(live.astype(np.int64))])
    walked = 0
    for base in range(0, n, K.TK_NT):
        if run[base] >= min(int(batch_size), 0x7fffffff):
            break
        walked += 1
    return SimpleNamespace(chunks=-(-n // K.TK_NT), walked=walked, dead_first=n >= K.TK_NT and not live[:K.TK_NT].any(), top=top, end_rank=end_rank,
                           on_boundary=end_rank >= 0 and (end_rank + 1) % K.TK_NT == 0, pop=pop)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------
def one_point_regions(rng, S):
    """-> xyz float32 [S, 3], sp_off, sp_pts: region s is the point s"""
    return rng.random((S, 3), dtype=np.float32) * np.float32(10), np.arange(S + 1, dtype=np.int32), np.arange(S, dtype=np.int32)


def base_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def shard(rng, per_rank, Smax, Bmax, lab_p=0.3):
    """per_rank: the cloud sizes of every rank -> the global arrays of the sharded entry points: glabelled [W * Smax] (padding counts as labelled), gbase
    [W * Bmax + 1] (a rank's missing clouds are empty, behind its regions), gorder (a ranking of all W * Smax ids)"""
    W = len(per_rank)
    glab = np.ones(W * Smax, np.uint8)
    gbase = []
    for r, sizes in enumerate(per_rank):
        S_r = int(np.sum(sizes))
        assert S_r <= Smax and len(sizes) <= Bmax
        glab[r * Smax:r * Smax + S_r] = rng.random(S_r) < lab_p
        b = np.concatenate([base_of(sizes)[:-1], np.full(Bmax - len(sizes), S_r)])
        gbase.append(b + r * Smax)
    gbase = np.concatenate(gbase + [[W * Smax]]).astype(np.int32)
    return glab, gbase, rng.permutation(W * Smax).astype(np.int32)


# ---- callers ----------------------------------------------------------------------------------------------------------------------------------------
def _L():
    from ssdr_al import _lib
    return _lib, _lib.lib(), _lib.DevArray


def _unpack(res, max_select, cap_rows):
    return SimpleNamespace(counts=res[:HEADER], picks=res[HEADER:HEADER + max_select], cand=res[HEADER + max_select:HEADER + max_select + cap_rows],
                           tail=res[HEADER + max_select + cap_rows:], raw=res)


def edcd(xyz, sp_off, sp_pts, order, labelled, base, batch_size, cap_rows, cap_nmax, cap_sq, max_select, guard=64):
    """ssdr_edcd_sampling_dev; the result buffer is filled with SENTINEL and `guard` words longer than the call may write"""
    _lib, L, D = _L()
    d = [D.from_host(np.ascontiguousarray(a, t)) for a, t in ((xyz, np.float32), (sp_off, np.int32), (sp_pts, np.int32), (order, np.int32), (labelled, np.uint8), (base, np.int32))]
    d_r = D.from_host(np.full(HEADER + max_select + cap_rows + guard, SENTINEL, np.int32))
    _lib.check(L.ssdr_edcd_sampling_dev(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, len(order), d[4].ptr, d[5].ptr, len(base) - 1, int(batch_size), int(cap_rows), int(cap_nmax),
                                        int(cap_sq), int(max_select), d_r.ptr, None))
    _lib.sync()
    return _unpack(d_r.to_host(), max_select, cap_rows)


def edcd_sharded(xyz, sp_off, sp_pts, num_clouds, gorder, glab, gbase, rank, world, Smax, Bmax, batch_size, cap_rows, cap_nmax, cap_sq, max_select, guard=64):
    _lib, L, D = _L()
    d = [D.from_host(np.ascontiguousarray(a, t)) for a, t in ((xyz, np.float32), (sp_off, np.int32), (sp_pts, np.int32), (gorder, np.int32), (glab, np.uint8), (gbase, np.int32))]
    d_r = D.from_host(np.full(HEADER + max_select + cap_rows + guard, SENTINEL, np.int32))
    _lib.check(L.ssdr_edcd_sampling_sharded_dev(d[0].ptr, d[1].ptr, d[2].ptr, int(num_clouds), d[3].ptr, len(gorder), d[4].ptr, d[5].ptr, int(rank), int(world), int(Smax), int(Bmax),
                                                int(batch_size), int(cap_rows), int(cap_nmax), int(cap_sq), int(max_select), d_r.ptr, None))
    _lib.sync()
    return _unpack(d_r.to_host(), max_select, cap_rows)


def gcn_fps(feat, cls, dom, lab_cls, lab_dom, xyz, sp_off, sp_pts, order, labelled, base, lab_off, lab_sp, batch_size, selector, cap_rows, cap_nmax, cap_sq, cap_unl,
            max_select, guard=64):
    """ssdr_gcn_fps_sampling_dev with gcn_number = 0, gcn_top = 0, start = 0 -> (result, the rows of ssdr_gcn_fps_sampling_rows float64 [cap_rows, 32])"""
    _lib, L, D = _L()
    i32, f32 = np.int32, np.float32
    d = [D.from_host(np.ascontiguousarray(a, t)) for a, t in ((feat, f32), (cls, i32), (dom, i32), (lab_cls, i32), (lab_dom, i32), (xyz, f32), (sp_off, i32), (sp_pts, i32),
                                                              (order, i32), (labelled, np.uint8), (base, i32), (lab_off, i32), (lab_sp, i32))]
    d_r = D.from_host(np.full(HEADER + max_select + cap_rows + guard, SENTINEL, np.int32))
    _lib.check(L.ssdr_gcn_fps_sampling_dev(d[0].ptr, 32, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr, d[7].ptr, d[8].ptr, len(order), d[9].ptr, d[10].ptr, len(base) - 1,
                                           d[11].ptr, d[12].ptr, len(lab_sp), int(batch_size), 0, 0, int(selector), 0, int(cap_rows), int(cap_nmax), int(cap_sq), int(cap_unl),
                                           int(max_select), d_r.ptr, None))
    _lib.sync()
    p, cap = C.c_void_p(), C.c_size_t()
    _lib.check(L.ssdr_gcn_fps_sampling_rows(None, C.byref(p), C.byref(cap)))
    assert cap.value == cap_rows
    rows = np.empty((cap_rows, 32), np.float64)
    _lib.check(L.ssdr_memcpy_d2h(_lib.ptr(rows), p, rows.nbytes))
    return _unpack(d_r.to_host(), max_select, cap_rows), rows


def gcn_fps_sharded_local(feat, xyz, sp_off, sp_pts, num_clouds, gorder, glab, gbase, rank, world, Smax, Bmax, batch_size, cap_rows, cap_nmax, cap_sq, nu_max, guard=64):
    """ssdr_gcn_fps_sharded_local_dev without labelled rows (n_lab = 0, nl_max = 0), every point of class 0, gcn_number = 0 -> (plan int32 with `guard` words
    behind it, comb_out float64 [nu_max + 1, 32]: one sentinel row behind what the call may write)"""
    _lib, L, D = _L()
    n, B = len(feat), int(num_clouds)
    d = [D.from_host(np.ascontiguousarray(a, t)) for a, t in ((feat, np.float32), (np.zeros(n), np.int32), (np.zeros(len(sp_off) - 1), np.int32), (xyz, np.float32), (sp_off, np.int32),
                                                              (sp_pts, np.int32), (np.zeros(B + 1), np.int32), (gorder, np.int32), (glab, np.uint8), (gbase, np.int32))]
    words = 16 + world + 2 * world * nu_max
    d_plan = D.from_host(np.full(words + guard, SENTINEL, np.int32))
    d_comb = D.from_host(np.full((nu_max + 1, 32), -7.5))
    _lib.check(L.ssdr_gcn_fps_sharded_local_dev(d[0].ptr, 32, d[1].ptr, d[2].ptr, None, None, d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr, None, 0, B, d[7].ptr, len(gorder), d[8].ptr,
                                                d[9].ptr, int(rank), int(world), int(Smax), int(Bmax), int(batch_size), 0, 0, int(cap_rows), int(cap_nmax), int(cap_sq), int(nu_max), 0,
                                                d_comb.ptr, d_plan.ptr, None))
    _lib.sync()
    return d_plan.to_host(), d_comb.to_host()


def topk(order, skip, batch_size, lo, hi, cap_out, guard=16):
    """ssdr_topk_regions_dev -> (res int32 [2], out int32 [cap_out + guard], SENTINEL where nothing was written)"""
    _lib, L, D = _L()
    d_o = D.from_host(np.ascontiguousarray(order if len(order) else np.zeros(1), np.int32)); d_s = D.from_host(np.ascontiguousarray(skip if len(skip) else np.zeros(1), np.uint8))
    d_res, d_out = D.from_host(np.full(2, SENTINEL, np.int32)), D.from_host(np.full(cap_out + guard, SENTINEL, np.int32))
    _lib.check(L.ssdr_topk_regions_dev(d_o.ptr, len(order), d_s.ptr, int(batch_size), int(lo), int(hi), d_res.ptr, d_out.ptr, None))
    _lib.sync()
    return d_res.to_host(), d_out.to_host()
