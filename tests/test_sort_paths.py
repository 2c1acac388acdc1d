"""csrc/radix_sort.hip alone, through ssdr_radix_sort_dev: every pass, segment and buffer path against NumPy's stable argsort, bit for bit, on the CPU logic
build and on gfx950.

Every case (tests/_sort_paths.py)
  1. asserts from the plan — a restatement of the host logic of RadixSorter::sort_segments — that its input reaches the branch it is named after, BEFORE the
     library is called;
  2. compares every word of the caller's buffers with the oracle: the live pairs, the dead slots [cnt, off[s + 1]) of every segment and the words behind the
     last slot (canaries: unchanged, or the 0xA5 fill under INPUT_IN_ALT);
  3. compares the plan with the record of ssdr_radix_sort_info field by field, and the AND / OR words the kernels went by with the oracle's, exactly.
The last test asserts that every branch the plan can name was reached by a case that ran and passed on that backend."""
import ctypes

import numpy as np
import pytest

import _score_paths as SP
import _sort_paths as S

U64 = np.uint64
K = S.constants()


def _rng(*seed):
    return np.random.default_rng([20261020, *seed])


def _const(rng):
    return int(rng.integers(0, 1 << 62)) * 4 + int(rng.integers(0, 4))


def one_segment(rng, n, varying, key_bits=64, shift=0, with_vals=True, payload=None, **kw):
    """one segment of n pairs whose key field varies in exactly the digits `varying`; values are the input index"""
    off = S.layout([n])
    k = S.field_keys(rng, n, varying, _const(rng), key_bits, shift, payload)
    keys, vals = S.assemble(off, [k], [np.arange(n, dtype=np.uint32)] if with_vals else None)
    return S.Case(off, [n], keys, vals, key_bits=key_bits, shift=shift, **kw)


def segments(rng, counts, varying, key_bits=64, shift=0, with_vals=True, slack=0, n_host=None, consts=None, **kw):
    """segment s: counts[s] slots filled with keys varying in varying[s] (a list per segment, or one list for all), its own constant elsewhere"""
    n_host = list(counts) if n_host is None else n_host
    off = S.layout(counts, slack)
    per = varying if varying and isinstance(varying[0], (list, tuple)) else [varying] * len(counts)
    consts = [_const(rng) for _ in counts] if consts is None else consts
    ks = [S.field_keys(rng, c, v, cst, key_bits, shift) for c, v, cst in zip(counts, per, consts)]
    start = np.concatenate([[0], np.cumsum(counts)])
    keys, vals = S.assemble(off, ks, [np.arange(a, a + c, dtype=np.uint32) for a, c in zip(start, counts)] if with_vals else None)
    return S.Case(off, n_host, keys, vals, key_bits=key_bits, shift=shift, **kw)


# ---- parity: 0 to 8 executed passes, both homes, with and without values ------------------------------------------------------------------------------------
PARITY_SETS = {"0": [], "1-low": [2], "1-byte7": [7], "2": [0, 5], "3": [1, 2, 6], "4": [0, 1, 2, 3], "5": [0, 2, 4, 5, 7], "6": [0, 1, 3, 4, 6, 7],
               "7": [0, 1, 2, 3, 4, 5, 6], "8": [0, 1, 2, 3, 4, 5, 6, 7]}


@pytest.mark.parametrize("with_vals", [True, False], ids=["kv", "keys"])
@pytest.mark.parametrize("in_alt", [False, True], ids=["home0", "home1"])
@pytest.mark.parametrize("name", list(PARITY_SETS))
def test_parity_of_executed_passes(backend, name, in_alt, with_vals):
    """n = 3000: one full tile and a partial one.  All-equal keys ("0"): no pass runs; under INPUT_IN_ALT rs_finish alone moves the pairs home."""
    v = PARITY_SETS[name]
    c = one_segment(_rng(1, len(name), sum(v)), 3000, v, with_vals=with_vals, in_alt=in_alt)
    S.run(backend, c, dict(executed=v, parity=len(v) & 1, home=int(in_alt), copies=(len(v) & 1) != int(in_alt), npass=4, high=1, wide=0, nb=2))


# ---- the passes above bit 32 -----------------------------------------------------------------------------------------------------------------------------
HIGH_SETS = [(33, [4]), (33, [0, 4]), (40, [1, 4]), (40, [4]), (64, [4, 5, 6, 7]), (64, [2, 5, 7])]


@pytest.mark.parametrize("key_bits,varying", HIGH_SETS, ids=["%d-%s" % (b, "".join(map(str, v))) for b, v in HIGH_SETS])
@pytest.mark.parametrize("n,wide", [(20000, False), (16383, True), (16384, True)], ids=["20000-single", "16383-flag", "16384-wide"])
def test_high_passes_single_or_wide(backend, n, wide, key_bits, varying):
    want_wide = wide and n >= K.WIDE
    c = one_segment(_rng(2, n, key_bits, len(varying)), n, varying, key_bits=key_bits, wide=wide)
    S.run(backend, c, dict(executed=varying, wide=int(want_wide), high=int(not want_wide), npass=(key_bits + 7) // 8 if want_wide else 4))


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_high_passes_rounds_of_the_one_workgroup(backend, n):
    """rs_high_passes takes 1024 pairs a round: one partial round, one less than a round, a whole one, one more, two and one pair"""
    c = one_segment(_rng(3, n), n, [4, 6], in_alt=bool(n & 1))
    S.run(backend, c, dict(executed=[4, 6] if n > 1 else [], high=1))


@pytest.mark.parametrize("with_vals", [True, False], ids=["kv", "keys"])
def test_high_passes_over_segments(backend, with_vals):
    """three segments: the kernel offsets its key and value pointers per segment (keys only: there is no value array to offset)"""
    c = segments(_rng(4, with_vals), [1025, 2049, 700], [[4, 5], [5], [1, 7]], with_vals=with_vals, slack=[1, 0, 2])
    P = S.run(backend, c, dict(executed=[1, 4, 5, 7], high=1))
    assert "rs_high_passes:segments" in P.branches


def test_high_passes_keys_only_single_segment(backend):
    c = one_segment(_rng(5), 2500, [5, 6], with_vals=False)
    assert "rs_high_passes:keys only" in S.run(backend, c, dict(executed=[5, 6])).branches


# ---- the AND / OR pre-pass -----------------------------------------------------------------------------------------------------------------------------
def _odd_one_out(n, at, setbit, in_alt=False, extra=()):
    """all keys equal but the one at `at`, which has one bit set (bit 13) or cleared (bit 21) that the others have not; extra: further segments' counts,
    all their keys equal"""
    base = 0x0123456789abcdef
    bit = 1 << 13 if setbit else 1 << 21
    base = base & ~bit if setbit else base | bit
    k = np.full(n, base, U64)
    k[at] = U64(base ^ bit)
    counts = [n, *extra]
    off = S.layout(counts)
    start = np.concatenate([[0], np.cumsum(counts)])
    keys, vals = S.assemble(off, [k] + [np.full(c, base, U64) for c in extra], [np.arange(a, a + c, dtype=np.uint32) for a, c in zip(start, counts)])
    return S.Case(off, counts, keys, vals, in_alt=in_alt), (base & (base ^ bit), base | (base ^ bit))


@pytest.mark.parametrize("n", [1, 7, 255, 256, 257, 768, 769, 1023, 1024, 1025, 2047, 2048, 2049])
def test_andor_prepass_unrolled_loop_and_tail(backend, n):
    """one block of 256 threads per 2048 keys: up to 2048 keys the stride is 256 (a thread's 4x-unrolled trip needs i + 768 < n, the tail takes the rest); at
    2049 the plan says two blocks, stride 512.  The one key that differs sits where a lane's first, unrolled and tail loads fall."""
    cu = SP.num_cu(backend)
    for setbit in (True, False):
        probe, _ = _odd_one_out(n, 0, setbit)
        stride = S.plan(probe, cu).andor_stride
        for at in sorted({0, n - 1, 255, 256, 3 * 256, 4 * 256 - 1, stride - 1, stride, 3 * stride, 4 * stride - 1, 4 * stride}):
            if not 0 <= at < n:
                continue
            c, (a, o) = _odd_one_out(n, at, setbit)
            P = S.run(backend, c, dict(gseg=1 if n <= 2048 else 2, gao=1 if n <= 2048 else 2, andor_stride=256 if n <= 2048 else 512,
                                       executed=[] if n == 1 else [1 if setbit else 2]))
            assert (int(P.words[0, 0]), int(P.words[0, 1])) == ((a, o) if n > 1 else (int(c.keys[0]), int(c.keys[0])))


@pytest.mark.parametrize("setbit", [True, False], ids=["set", "cleared"])
def test_andor_prepass_several_blocks(backend, setbit):
    n = 5 * K.TILE + 77
    stride = S.plan(_odd_one_out(n, 0, setbit)[0], SP.num_cu(backend)).andor_stride
    for at in (0, n - 1, stride - 1, stride, 3 * stride, 4 * stride - 1, 4 * stride, 4 * stride + 255):
        c, (a, o) = _odd_one_out(n, at, setbit)
        P = S.run(backend, c, dict(gao=6, andor_stride=6 * 256))
        assert (int(P.words[0, 0]), int(P.words[0, 1])) == (a, o)
        assert "gao>1" in P.branches


def test_andor_prepass_64_segments_limit_of_the_grid(backend):
    """64 segments: the pre-pass's grid.x is limited to num_cu * 16 / nseg, below what the largest segment would take"""
    cu = SP.num_cu(backend)
    n = 65 * K.TILE + 5
    for at in (0, n - 1, (cu * K.GAO_CU // 64) * 256 * 4 + 17):
        c, (a, o) = _odd_one_out(n, at, True, extra=[3] * 63)
        P = S.run(backend, c, dict(gao=cu * K.GAO_CU // 64, gseg=lambda g: g > cu * K.GAO_CU // 64))
        assert (int(P.words[0, 0]), int(P.words[0, 1])) == (a, o) and P.words[1, 0] == P.words[1, 1]


# ---- d_andor given -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_alt", [False, True], ids=["home0", "home1"])
@pytest.mark.parametrize("shift,key_bits", [(0, 64), (0, 24), (17, 40)])
def test_given_words_exact_and_loosest(backend, shift, key_bits, in_alt):
    """the exact words, then the loosest legal ones (AND' = 0, OR' = every bit of the key field): the same result, but every pass of the field runs, and the
    parity and the final copy follow the GIVEN words.  The middle segment is empty: (~0, 0)."""
    varying = [0, 2] if key_bits <= 32 else [1, 4]
    c = segments(_rng(6, shift, key_bits), [2500, 0, 5000], varying, key_bits=key_bits, shift=shift, slack=[0, 1, 0], in_alt=in_alt)
    exact = S.words(c)
    assert exact[1, 0] == S.ALL1 and exact[1, 1] == 0
    c.andor = exact
    P = S.run(backend, c, dict(executed=varying, parity=0))
    assert {"d_andor", "rs_andor:given"} <= P.branches
    loose = exact.copy()
    loose[[0, 2]] = (0, ((1 << key_bits) - 1) << shift)
    c.andor = loose
    nd = (key_bits + 7) // 8
    S.run(backend, c, dict(executed=list(range(nd)), parity=nd & 1, copies=(nd & 1) != int(in_alt)))


# ---- shift -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_vals", [False, True], ids=["keys", "kv"])
@pytest.mark.parametrize("shift,key_bits", [(1, 63), (1, 9), (17, 47), (17, 12), (32, 32), (32, 20), (40, 24), (40, 7)])
def test_shift_payload_travels_with_its_key(backend, shift, key_bits, with_vals):
    """(key << shift) | index words as the subsampling builds them: the index below `shift` is no part of the sort key and stays with its word"""
    n = 5000
    varying = list(range((key_bits + 7) // 8))
    c = one_segment(_rng(7, shift, key_bits), n, varying, key_bits=key_bits, shift=shift, with_vals=with_vals, payload=np.arange(n), in_alt=with_vals)
    P = S.run(backend, c, dict(executed=varying))
    assert with_vals or "keys only" in P.branches


# ---- segments ----------------------------------------------------------------------------------------------------------------------------------------------
MIX = [0, 1, 2047, 2048, 2049, 5000]


@pytest.mark.parametrize("nseg", [1, 2, 3, 64])
def test_segments_of_mixed_counts(backend, nseg):
    """counts 0, 1, one short of a tile, a tile, one more, several tiles, with whole slack tiles between the segments; the pass of digit 2 varies in one segment
    only, and byte 3 — constant inside every segment, another constant in each — stays skipped"""
    rng = _rng(8, nseg)
    counts = [5000] if nseg == 1 else [MIX[(i + 2) % len(MIX)] for i in range(nseg)]
    only = min(nseg - 1, 2)                       # a segment of at least 2047 keys
    varying = [[0, 2] if i == only else [0] for i in range(nseg)]
    consts = [(_const(rng) & ~(0xff << 24)) | ((i * 37 + 5) & 0xff) << 24 for i in range(nseg)]
    c = segments(rng, counts, varying, key_bits=32, slack=[i % 3 for i in range(nseg)], consts=consts, in_alt=nseg == 3)
    S.run(backend, c, dict(executed=[0, 2], high=0, npass=4))


# ---- device counts -----------------------------------------------------------------------------------------------------------------------------------------
HOST = [5000, 2049, 4096 + 5, 3000]
COUNTS = {"below": [100, 2048, 2049, 1], "first-empty": [0, 2049, 4000, 3000], "middle-empty": [5000, 0, 0, 2999], "last-empty": [4097, 1, 4101, 0],
          "equal": HOST, "above": [5001, 1 << 30, 4102, 3000], "all-empty": [0, 0, 0, 0]}


@pytest.mark.parametrize("in_alt", [False, True], ids=["home0", "home1"])
@pytest.mark.parametrize("name", list(COUNTS))
def test_device_counts(backend, name, in_alt):
    """cnt = min(d_cnt, n_host): the pairs behind it are dead slots, whole tiles of them included (5000 slots, 100 live); a count above n_host is clamped"""
    c = segments(_rng(9, len(name)), HOST, [0, 3, 4], d_cnt=COUNTS[name], slack=[0, 1, 0, 0], in_alt=in_alt)
    live = np.minimum(COUNTS[name], HOST)
    P = S.run(backend, c, dict(executed=lambda e: e == ([0, 3, 4] if (live >= 2).any() else [])))
    assert "d_cnt" in P.branches


# ---- stability ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["1", "2", "3", "256", "runs"])
def test_ties_keep_their_input_order(backend, kind):
    """10000 pairs, values are the input index: any reordering of equal keys shows.  "runs": one digit over more than a wave's 512 pairs and over more than a tile"""
    rng, n = _rng(10, len(kind)), 10000
    pool = rng.integers(0, 1 << 32, 256).astype(U64)
    if kind == "runs":
        k = np.concatenate([np.repeat(pool[:4], 600), np.repeat(pool[4:6], 2500), pool[rng.integers(0, 8, n - 7400)]])
    else:
        k = pool[rng.integers(0, int(kind), n)]
    off = S.layout([n])
    keys, vals = S.assemble(off, [k], [np.arange(n, dtype=np.uint32)])
    c = S.Case(off, [n], keys, vals, key_bits=32)
    S.run(backend, c, dict(executed=lambda e: (len(e) == 0) == (kind == "1")))


# ---- rs_scan's carry ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", [256, 257])
def test_scan_carry_across_chunks(backend, tiles):
    """a segment of 256 tiles (one trip of rs_scan's loop) and of 257 (256 * 2048 + 1 pairs: two trips, the second takes the carry), between two small
    segments: its histogram rows start at a tile b0 > 0, and so do those of the segment behind it.  One executed pass."""
    n = 256 * K.TILE + (1 if tiles == 257 else 0)
    c = segments(_rng(11, tiles), [3000, n, 2500], [1], key_bits=32, slack=[1, 0, 0])
    P = S.run(backend, c, dict(executed=[1], chunks=[1, 2 if tiles == 257 else 1, 1]))
    assert (tiles == 257) == ("scan chunks>1" in P.branches)


# ---- the grid-stride loops of rs_hist / rs_scatter ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("varying", [[0], [1, 3]], ids=["1pass", "2passes"])
def test_blocks_take_a_second_tile(backend, varying):
    """one tile more than the grid has blocks (8 per CU), the last one partial: block 0 comes round a second time, with its counters cleared in between"""
    nb = K.G_CU * SP.num_cu(backend) + 1
    c = one_segment(_rng(12, len(varying)), (nb - 1) * K.TILE + 777, varying, key_bits=32)
    P = S.run(backend, c, dict(executed=varying, nb=nb, g=nb - 1, tile_trips=2))
    assert "tile loop>1" in P.branches


# ---- one sorter, call after call ------------------------------------------------------------------------------------------------------------------------------
def test_reuse_on_one_stream(backend):
    """small, larger (the histogram rows grow, the totals behind them move), small again; wide passes on and off: every call correct, the record follows each.
    A new stream starts from nothing."""
    from ssdr_al import _lib
    L = _lib.lib()
    st, st2 = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(L.ssdr_stream_create(ctypes.byref(st)))
    _lib.check(L.ssdr_stream_create(ctypes.byref(st2)))
    try:
        rec, _ = S.info(st)
        assert not any(rec.values())
        small = lambda i: one_segment(_rng(13, i), 3000, [0, 1], key_bits=32)
        seen = []
        for i, c in enumerate([small(0), segments(_rng(13, 9), [40000, 2049], [0, 2, 3], key_bits=32, in_alt=True), small(1),
                               one_segment(_rng(13, 2), 20000, [0, 4, 5], wide=True), one_segment(_rng(13, 3), 20000, [0, 4, 5], wide=False),
                               one_segment(_rng(13, 4), 20000, [4], wide=True, with_vals=False), small(2)]):
            P = S.run(backend, c, stream=st)
            seen.append((P.nblocks_max, P.wide))
        assert seen == [(3, 0), (23, 0), (3, 0), (11, 1), (11, 0), (11, 1), (3, 0)]
        rec, _ = S.info(st2)
        assert not any(rec.values())               # the other stream's sorter has not been used
        S.run(backend, small(3), stream=st2)
        assert S.info(st)[0]["nb"] == 2                # ... and left the first one's record alone
    finally:
        _lib.check(L.ssdr_stream_destroy(st))
        _lib.check(L.ssdr_stream_destroy(st2))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_alt", [False, True], ids=["home0", "home1"])
def test_refusals_touch_nothing(backend, in_alt):
    c = segments(_rng(14), [3000, 100], [0, 1], slack=[0, 1], in_alt=in_alt)
    T = K.TILE

    def untouched(want, raw=None, **change):
        saved = {k: getattr(c, k) for k in change}
        for k, v in change.items():
            setattr(c, k, v)
        try:
            st, keys, vals = S.call(c, raw=raw)
        finally:
            for k, v in saved.items():
                setattr(c, k, v)
        assert st == want, (st, raw, change)
        S.assert_same(keys, np.concatenate([c.keys, np.full(S.TAIL, S.CAN_K, U64)]), "keys after a refused call")
        S.assert_same(vals, np.concatenate([c.vals, np.full(S.TAIL, S.CAN_V, np.uint32)]), "values after a refused call")
        rec, w = S.info(None, 2)
        assert not any(rec.values()) and (w == S.CAN_K).all()

    INV = S.SSDR_ERR_INVALID
    untouched(INV, raw=(K.MAX_SEG + 1, np.arange(K.MAX_SEG + 2) * T, np.ones(K.MAX_SEG + 1)))
    untouched(INV, raw=(2, [0, 2 * T - 1, 4 * T], [3000, 100]))          # an unaligned start
    untouched(INV, raw=(2, [0, 2 * T, 4 * T - 1], [3000, 100]))          # an unaligned end: the kernels would leave the partial tile unsorted
    untouched(INV, raw=(2, [0, T, 4 * T], [3000, 100]))                  # a segment that does not hold its pairs
    untouched(INV, raw=(2, [0, 2 * T, 4 * T], [3000, 2 * T + 1]))
    untouched(INV, shift=-1)
    untouched(INV, shift=1, key_bits=64)
    untouched(INV, shift=40, key_bits=25)
    untouched(0, raw=(0, [0], [0]))
    untouched(0, raw=(-3, [0], [0]))
    untouched(0, raw=(2, [0, 0, 0], [0, 0]))
    from ssdr_al import _lib
    L = _lib.lib()
    off, nh = np.asarray(c.off), np.asarray(c.n_host)
    assert L.ssdr_radix_sort_dev(None, None, 2, _lib.ptr(off), _lib.ptr(nh), None, 64, 0, None, c.flags, None) == INV
    assert L.ssdr_radix_sort_dev(None, None, 2, _lib.ptr(off), _lib.ptr(nh), None, 64, 0, None, 4, None) == INV          # an unknown flag
    assert L.ssdr_radix_sort_info(None, None, None) == INV
    S.run(backend, c)                                                         # and the sorter still works


# ---- every branch was reached ----------------------------------------------------------------------------------------------------------------------------
def test_every_branch_was_reached(backend):
    """the branches the plan can name, against those of the cases above that ran and passed on this backend (run the whole file: a selection of its cases
    leaves branches open)"""
    missing = S.ALL_BRANCHES - S.RAN[backend]
    assert not missing, "no case that passed on %s reached: %s" % (backend, sorted(missing))
    assert S.RAN[backend] <= S.ALL_BRANCHES, "branches the closing test does not know: %s" % sorted(S.RAN[backend] - S.ALL_BRANCHES)
