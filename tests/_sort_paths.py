"""Helpers of tests/test_sort_paths.py: the constants of csrc/radix_sort.hip read from the sources, the oracle (NumPy's stable argsort per segment), a restatement
of the host logic of RadixSorter::sort_segments (`plan`: which kernels are launched with which grids, which passes execute, where the result ends up, which
loops come round), the key builder, and the caller of ssdr_radix_sort_dev / ssdr_radix_sort_info.  Nothing here touches a device except `call`.

A case is a `Case`: the segment table, the buffers as the caller hands them over (dead slots and the words behind the last slot hold canaries) and the
parameters of the call.  `plan(case, cu)` is computed from those alone; `run(backend, case)` compares it with the library's record field by field."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np

import _score_paths as SP

ROOT = SP.ROOT
CSRC = SP.CSRC
U64 = np.uint64
ALL1 = U64(0xffffffffffffffff)
FILL_K, FILL_V = U64(0xa5a5a5a5a5a5a5a5), np.uint32(0xa5a5a5a5)          # what ssdr_radix_sort_dev leaves in the caller's buffers under INPUT_IN_ALT
CAN_K, CAN_V = U64(0xdeadbeefcafef00d), np.uint32(0xc0ffee11)            # canaries: dead slots and the words behind the buffers
TAIL = 64                                                                  # canary words behind the last slot
WIDE_HIGH, INPUT_IN_ALT = 1, 2
SSDR_ERR_INVALID = 1
RECORD = ("npass", "wide", "high", "g", "gao", "gseg", "nb", "nblocks_max")

_CONSTANTS = None


def constants():
    """RS_BS, RS_ITEMS, TILE (their product, equal to RADIX_TILE), RS_ANDOR_G, MAX_SEG, WIDE (the 16384 threshold, _score_paths' RADIX_WIDE), and the factors of
    the CU count in the grids: G_CU (rs_hist / rs_scatter), GSEG_CU and GSEG_ITEMS (the segment grid), GAO_CU (the pre-pass), FINISH_CAP (rs_finish)."""
    global _CONSTANTS
    if _CONSTANTS is None:
        out = {}
        text, path = SP._read(CSRC, "radix_sort.hip")
        out["RS_BS"] = SP._one(r"\bRS_BS = (\d+),", text, path)
        out["RS_ITEMS"] = SP._one(r"\bRS_ITEMS = (\d+),", text, path)
        out["RS_ANDOR_G"] = SP._one(r"\bRS_ANDOR_G = (\d+);", text, path)
        out["G_CU"] = SP._one(r"std::min\(nb, ctx\(\)\.num_cu \* (\d+)\)", text, path)
        out["GSEG_ITEMS"] = SP._one(r"\(maxn \+ RS_BS \* (\d+) - 1\)", text, path)
        out["GSEG_CU"] = SP._one(r"\(RS_BS \* \d+\), ctx\(\)\.num_cu \* (\d+)\)", text, path)
        out["GAO_CU"] = SP._one(r"ctx\(\)\.num_cu \* (\d+) / nseg", text, path)
        out["FINISH_CAP"] = SP._one(r"std::max\(1, (\d+) / nseg\)", text, path)
        out["WIDE"] = SP.constants().RADIX_WIDE
        text, path = SP._read(CSRC, "ssdr_internal.hpp")
        out["TILE"] = SP._one(r"\bRADIX_TILE = (\d+);", text, path)
        out["MAX_SEG"] = SP._one(r"\bRADIX_MAX_SEG = (\d+);", text, path)
        assert out["TILE"] == out["RS_BS"] * out["RS_ITEMS"]
        _CONSTANTS = SimpleNamespace(**out)
    return _CONSTANTS


# ---- a case ---------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """off int [nseg + 1], n_host int [nseg], keys uint64 [off[nseg]] (every slot: the live pairs first, canaries behind), vals uint32 [off[nseg]] or None,
    d_cnt int [nseg] or None, andor uint64 [nseg, 2] or None"""

    def __init__(self, off, n_host, keys, vals=None, d_cnt=None, key_bits=64, shift=0, andor=None, wide=False, in_alt=False):
        self.off, self.n_host = np.asarray(off, np.int32), np.asarray(n_host, np.int32)
        self.nseg = len(self.n_host)
        self.keys, self.vals = np.ascontiguousarray(keys, U64), None if vals is None else np.ascontiguousarray(vals, np.uint32)
        self.d_cnt = None if d_cnt is None else np.asarray(d_cnt, np.int32)
        self.key_bits, self.shift = int(key_bits), int(shift)
        self.andor = None if andor is None else np.ascontiguousarray(andor, U64).reshape(self.nseg, 2)
        self.wide, self.in_alt = bool(wide), bool(in_alt)
        assert len(self.off) == self.nseg + 1 and len(self.keys) == self.off[-1] and (self.vals is None or len(self.vals) == len(self.keys))

    @property
    def flags(self):
        return (WIDE_HIGH if self.wide else 0) | (INPUT_IN_ALT if self.in_alt else 0)

    def counts(self):
        c = self.n_host if self.d_cnt is None else np.minimum(self.d_cnt, self.n_host)
        return np.maximum(c, 0).astype(np.int64)


def layout(counts, slack_tiles=0):
    """tile-aligned offsets for segments that hold `counts` slots, `slack_tiles` (an int or one per segment) whole tiles more each"""
    T = constants().TILE
    slack = np.broadcast_to(np.asarray(slack_tiles, np.int64), (len(counts),))
    off = [0]
    for c, s in zip(counts, slack):
        off.append(off[-1] + (-(-int(c) // T) + int(s)) * T)
    return np.asarray(off, np.int32)


def field_keys(rng, n, varying, const, key_bits=64, shift=0, payload=None):
    """n words whose key field (bits [shift, shift + key_bits)) varies in exactly the digit bytes `varying` (0 = the lowest byte of the FIELD) and holds the bytes
    of `const` everywhere else; bits at and above shift + key_bits are zero.  With n >= 2 every varying digit does vary (the first two words differ in its
    lowest bit).  payload (below `shift`): given words, or random ones."""
    vmask = 0
    for p in varying:
        assert 8 * p < key_bits, "digit %d lies above the %d key bits" % (p, key_bits)
        vmask |= 0xff << (8 * p)
    fmask = (1 << key_bits) - 1
    vmask &= fmask
    f = rng.integers(0, 1 << 63, n, dtype=np.int64).astype(U64) * U64(2) + rng.integers(0, 2, n).astype(U64)
    f = (f & U64(vmask)) | U64(int(const) & fmask & ~vmask)
    if n >= 2:
        for p in varying:
            bit = U64(1 << (8 * p))
            f[0] &= ~bit
            f[1] |= bit
    if shift == 0:
        return f
    if payload is None:
        payload = rng.integers(0, 1 << min(shift, 62), n, dtype=np.int64).astype(U64)
    return (f << U64(shift)) | (np.asarray(payload, U64) & U64((1 << shift) - 1))


def assemble(off, live_keys, live_vals=None):
    """the buffers of a case: segment s's live words at off[s], canaries in every other slot"""
    keys = np.full(int(off[-1]), CAN_K, U64)
    vals = None if live_vals is None else np.full(int(off[-1]), CAN_V, np.uint32)
    for s, k in enumerate(live_keys):
        keys[off[s]:off[s] + len(k)] = k
        if vals is not None:
            vals[off[s]:off[s] + len(k)] = live_vals[s]
    return keys, vals


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------------------------
def words(case):
    """AND and OR of every segment's live words -> uint64 [nseg, 2]; an empty segment gives (~0, 0)"""
    out = np.empty((case.nseg, 2), U64)
    for s, c in enumerate(case.counts()):
        k = case.keys[case.off[s]:case.off[s] + c]
        out[s] = (np.bitwise_and.reduce(k), np.bitwise_or.reduce(k)) if c else (ALL1, U64(0))
    return out


def oracle(case):
    """-> (keys, vals) as the caller's buffers must read after the call, every slot"""
    keys = np.full_like(case.keys, FILL_K) if case.in_alt else case.keys.copy()
    vals = None if case.vals is None else (np.full_like(case.vals, FILL_V) if case.in_alt else case.vals.copy())
    for s, c in enumerate(case.counts()):
        a = int(case.off[s])
        k = case.keys[a:a + c]
        order = np.argsort(k >> U64(case.shift), kind="stable")
        keys[a:a + c] = k[order]
        if vals is not None:
            vals[a:a + c] = case.vals[a:a + c][order]
    return keys, vals


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------------------
def plan(case, cu):
    """RadixSorter::sort_segments restated.  Fields of the record (RECORD) and:
    words [nseg, 2] the kernels go by; varying: the digits (0..7) on which AND and OR disagree in some non-empty segment; executed: those of them a launched
    kernel covers; parity: which of the two buffers (0 = where the input was) holds the result before rs_finish; home; copies: rs_finish moves data;
    chunks [nseg]: trips of rs_scan's loop; tile_trips: tiles the busiest block of rs_hist / rs_scatter takes; branches: the names the closing test counts"""
    K = constants()
    nseg = case.nseg
    slots, maxn = int(case.off[-1]), int(case.n_host.max())
    all_ = (max(case.key_bits, 1) + 7) // 8
    wide = case.wide and case.key_bits > 32 and maxn >= K.WIDE
    npass = all_ if wide else min(4, all_)
    high = case.key_bits > 32 and not wide
    nb = -(-slots // K.TILE)
    g = max(1, min(nb, cu * K.G_CU))
    gseg = max(1, min(-(-maxn // (K.RS_BS * K.GSEG_ITEMS)), cu * K.GSEG_CU))
    gao = max(1, min(min(gseg, K.RS_ANDOR_G), max(1, cu * K.GAO_CU // nseg)))
    w = words(case) if case.andor is None else case.andor
    diff = 0
    for a, o in w:
        if not (a == ALL1 and o == 0):
            diff |= int(a) ^ int(o)
    diff >>= case.shift
    varying = [p for p in range(8) if (diff >> (8 * p)) & 0xff]
    executed = [p for p in varying if p < npass or (high and p >= 4)]
    parity, home = len(varying) & 1, int(case.in_alt)
    counts = case.counts()
    P = SimpleNamespace(all=all_, npass=npass, wide=int(wide), high=int(high), g=g, gao=gao, gseg=gseg, nb=nb, nblocks_max=nb + 1, words=w, varying=varying,
                        executed=executed, parity=parity, home=home, copies=parity != home, finish_grid=min(gseg, max(1, K.FINISH_CAP // nseg)),
                        chunks=-(-(-(-counts // K.TILE)) // K.RS_BS), tile_trips=-(-nb // g), andor_stride=gao * K.RS_BS)
    low, hi = [p for p in executed if p < npass], [p for p in executed if p >= npass]
    br = {"rs_andor:" + ("given" if case.andor is not None else "launched"), "rs_scatter:" + ("kv" if case.vals is not None else "keys"),
          "rs_high_passes:" + ("launched" if high else "not launched"), "high:" + ("wide" if wide else "single" if high else "none"),
          "parity%d:home%d" % (parity, home), "rs_finish:" + ("copies" if P.copies else "stays"), "wide passes executed:%d" % min(len(low), 2)}
    if hi:
        br.add("rs_high_passes:executes")
        if nseg > 1 and np.count_nonzero(counts) > 1: br.add("rs_high_passes:segments")
        if case.vals is None: br.add("rs_high_passes:keys only")
    if (P.chunks > 1).any() and low: br.add("scan chunks>1")
    if P.tile_trips > 1 and low: br.add("tile loop>1")
    if gao > 1 and case.andor is None: br.add("gao>1")
    if case.d_cnt is not None: br.add("d_cnt")
    if case.andor is not None: br.add("d_andor")
    if case.vals is None: br.add("keys only")
    P.branches = br
    return P


ALL_BRANCHES = ({"rs_andor:given", "rs_andor:launched", "rs_scatter:kv", "rs_scatter:keys", "rs_high_passes:launched", "rs_high_passes:not launched", "high:wide",
                 "high:single", "high:none", "rs_finish:copies", "rs_finish:stays", "wide passes executed:0", "wide passes executed:1", "wide passes executed:2",
                 "rs_high_passes:executes", "rs_high_passes:segments", "rs_high_passes:keys only", "scan chunks>1", "tile loop>1", "gao>1", "d_cnt", "d_andor",
                 "keys only"} | {"parity%d:home%d" % (p, h) for p in (0, 1) for h in (0, 1)})
RAN = {"emu": set(), "gpu": set()}          # the branches of the cases that ran and passed, per backend (the closing test)


# ---- the caller -----------------------------------------------------------------------------------------------------------------------------------------
def _L():
    from ssdr_al import _lib
    return _lib, _lib.lib(), _lib.DevArray


def info(stream=None, nseg=0):
    """ssdr_radix_sort_info -> (record dict, words uint64 [nseg, 2] prefilled with the canary)"""
    _lib, L, D = _L()
    out = np.full(8, -1, np.int32)
    w = np.full((nseg, 2), CAN_K, U64)
    _lib.check(L.ssdr_radix_sort_info(stream, _lib.ptr(out), _lib.ptr(w) if nseg else None))
    return dict(zip(RECORD, (int(x) for x in out))), w


def call(case, stream=None, raw=None):
    """the call as it is -> (status, keys [slots + TAIL], vals or None): the whole buffers, canary tails included.  raw: (nseg, off, n_host) to hand over
    in place of the case's (the refusals: the buffers are still the case's)"""
    _lib, L, D = _L()
    tail_k, tail_v = np.full(TAIL, CAN_K, U64), np.full(TAIL, CAN_V, np.uint32)
    d_k = D.from_host(np.concatenate([case.keys, tail_k]))
    d_v = None if case.vals is None else D.from_host(np.concatenate([case.vals, tail_v]))
    d_c = None if case.d_cnt is None else D.from_host(case.d_cnt)
    d_w = None if case.andor is None else D.from_host(case.andor)
    nseg, off, n_host = (case.nseg, case.off, case.n_host) if raw is None else raw
    off, n_host = np.ascontiguousarray(off, np.int32), np.ascontiguousarray(n_host, np.int32)
    _lib.sync()
    status = L.ssdr_radix_sort_dev(d_k.ptr, d_v.ptr if d_v else None, int(nseg), _lib.ptr(off), _lib.ptr(n_host), d_c.ptr if d_c else None, case.key_bits,
                                   case.shift, d_w.ptr if d_w else None, case.flags, stream)
    _lib.sync(stream)
    return status, d_k.to_host(), None if d_v is None else d_v.to_host()


def assert_same(got, want, what):
    bad = got != want
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError("%s: %d of %d words differ, first at %d: %#x, expected %#x" % (what, bad.sum(), bad.size, i, int(got[i]), int(want[i])))


def run(backend, case, expect=None, stream=None):
    """expect: {plan field: value or predicate}, asserted on the plan BEFORE the call.  Then: the call, every word of both buffers against the oracle (live
    pairs, dead slots, tails), the record and the AND / OR words against the plan.  -> the plan"""
    P = plan(case, SP.num_cu(backend))
    for name, v in (expect or {}).items():
        have = getattr(P, name)
        assert v(have) if callable(v) else np.array_equal(have, v), "the case does not reach its branch: %s is %r" % (name, have)
    assert all(p < P.npass or (P.high and p >= 4) for p in P.varying), "keys vary in a digit no launched pass covers: %s" % P.varying
    status, keys, vals = call(case, stream)
    assert status == 0, _L()[0].lib().ssdr_last_error().decode()
    want_k, want_v = oracle(case)
    n = len(case.keys)
    assert_same(keys[n:], np.full(TAIL, CAN_K, U64), "words behind the keys")
    assert_same(keys[:n], want_k, "keys")
    if vals is not None:
        assert_same(vals[n:], np.full(TAIL, CAN_V, np.uint32), "words behind the values")
        assert_same(vals[:n], want_v, "values")
    rec, w = info(stream, case.nseg)
    for name in RECORD:
        assert rec[name] == getattr(P, name), "record %s: the library says %d, the plan %d" % (name, rec[name], getattr(P, name))
    assert_same(w.ravel(), np.asarray(P.words, U64).ravel(), "AND / OR words")
    RAN[backend] |= P.branches
    return P
