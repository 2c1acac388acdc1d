"""The scoring half of a selection round and its ranking, branch by branch: ssdr_point_uncertainty_dev, ssdr_region_stats_dev, ssdr_dominant_label_dev,
ssdr_clsbal_dev, ssdr_class_hist_dev + ssdr_clsbal_hist_dev, ssdr_mask_regions_dev, ssdr_segment_mean_features_dev and ssdr_rank_regions_dev (csrc/select.hip)
against oracle/select_np.py on the same inputs.  DESIGN.md section 25 lists every branch with the case that reaches it.  What the older tests
(test_select.py, test_select_oracle.py, test_properties.py) leave open and this file closes:

  * floats are compared on their BITS (float32 as uint32, float64 as uint64): the sign of a zero is a difference, where np.array_equal sees none;
  * region sums of -0.0 members alone (the entropy of one-hot rows) at every size class of the wave kernel: NumPy returns +0.0;
  * the ranking with +0.0 / -0.0 interleaved (equal: by index) and with NaN of both signs (last, by index), on the counting kernel and both radix forms;
  * every size at which a kernel takes another path: the LDS staging of C <= 32, a second grid pass, fewer than 8 members, the eight-lane blocks, RS_CAP,
    NP_BUFSIZE, the wave loop's second trip, RANK_SMALL, the radix sorter's wide passes.

Every case runs on the CPU logic build and on the gfx950 build with the same inputs and asserts its input condition with tests/_score_paths.py: plan_* BEFORE
the library is called.  Two tolerances are not zero, and both are measured here from the oracle's own error, never from the device: the float32 entropy of
generic rows (log2f's last bit) and the class-balance factor (exp's last place); see _entropy_bound and _clsbal_bound.
"""
import functools

import numpy as np
import pytest

from oracle import select_np as O
import _score_paths as P

K = P.constants()
MODES = ("mean", "sum_weight", "WetSU")


# ---- A1. point uncertainty -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _probs(n, C, seed=11):
    """softmax-like float32 rows; every seventh row has its maximum twice (the first index wins, sb is exactly 1), every fifth its maximum in the last column,
    every eleventh exact zeros, every thirteenth is one-hot, every seventeenth holds subnormals"""
    rng = np.random.default_rng(seed + 1000 * C + n)
    p = rng.random((n, C), dtype=np.float32) ** 4 + np.float32(1e-6)
    r = np.arange(n)
    top = p.max(1) * np.float32(1.25)
    k = r % 5 == 0; p[k, C - 1] = top[k]
    k = r % 7 == 0; a = rng.integers(0, C - 1, n); p[k, a[k]] = top[k] * 2; p[k, (a[k] + 1 + rng.integers(0, C - 1, n)[k]) % C] = top[k] * 2
    p = (p / p.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)
    k = r % 11 == 0; z = rng.random((n, C)) < 0.4; z[:, 0] = False; p[k] = np.where(z[k], np.float32(0), p[k])
    k = r % 17 == 1; p[k, 1 % C] = np.float32(1e-41)
    k = r % 13 == 0; hot = rng.integers(0, C, n); p[k] = 0; p[k, hot[k]] = 1
    p.setflags(write=False)
    return p


@functools.lru_cache(None)
def _entropy_bound():
    """The oracle's own float32 entropy against a float64 entropy of the same rows, over all C of the cases: the largest absolute error E.  The device may
    be 2 E off the float64 value (its log2f and NumPy's round differently in the last bit).  -> (E, rows)"""
    worst, rows = 0.0, 0
    for C in (2, 13, 32, 33, 128):
        p = _probs(257, C)
        p64 = p.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            h64 = -np.sum(np.where(p64 > 0, p64 * np.log2(p64), 0.0), axis=-1)
        worst = max(worst, float(np.abs(O.point_uncertainty(p, "entropy").astype(np.float64) - h64).max())); rows += len(p)
    return worst, rows


def _entropy64(p):
    p64 = p.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.sum(np.where(p64 > 0, p64 * np.log2(p64), 0.0), axis=-1)


@pytest.mark.parametrize("C", [2, 13, 32, 33, 128])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_point_uncertainty(backend, n, C):
    """lc and sb on bits, the class against np.argmax, the entropy within twice the oracle's own error; one-hot rows give the bits of -0.0"""
    p = _probs(n, C)
    pl = P.plan_point(n, C)
    assert pl.staged == (C <= 32) and pl.trips == 1 and pl.tail == (n - 1) % 256 + 1
    if n >= 255:
        top = p.max(1)
        assert ((p == top[:, None]).sum(1) == 2).any() and (p.argmax(1) == C - 1).any() and (p == 0).any() and ((p == 1).sum(1) == 1).any() and ((p > 0) & (p < 1e-38)).any()
    want_cls = np.argmax(p, axis=-1).astype(np.int32)
    for mode in ("lc", "sb"):
        unc, cls = P.point_uncertainty(p, mode)
        P.assert_bits(unc, O.point_uncertainty(p, mode).astype(np.float32), "%s n=%d C=%d" % (mode, n, C))
        assert np.array_equal(cls, want_cls), mode
    twice = (p == p.max(1)[:, None]).sum(1) >= 2
    assert (P.point_uncertainty(p, "sb")[0][twice] == 1).all()
    unc, cls = P.point_uncertainty(p, "entropy")
    assert np.array_equal(cls, want_cls)
    E, _ = _entropy_bound()
    err = np.abs(unc.astype(np.float64) - _entropy64(p))
    print("entropy n=%d C=%d: device error %.3e, oracle's own error (bound / 2) %.3e" % (n, C, err.max(), E))
    assert err.max() <= 2 * E, "entropy: %.3e off the float64 value, the oracle itself %.3e" % (err.max(), E)
    hot = (p == 1).sum(1) == 1
    P.assert_bits(unc[hot], np.full(hot.sum(), -0.0, np.float32), "entropy of one-hot rows")
    P.assert_bits(unc[hot], O.point_uncertainty(p, "entropy")[hot], "entropy of one-hot rows against the oracle")


def test_point_uncertainty_second_grid_pass(backend):
    """one row more than a single pass of the capped grid covers: workgroup 0 comes round for it, with one live lane"""
    n, C = K.GRID_CAP * 256 + 1, 13
    pl = P.plan_point(n, C)
    assert pl.grid == K.GRID_CAP and pl.trips == 2 and pl.tail == 1 and pl.staged
    p = _probs(n, C)
    want_cls = np.argmax(p, axis=-1).astype(np.int32)
    for mode in ("lc", "sb"):
        unc, cls = P.point_uncertainty(p, mode)
        P.assert_bits(unc, O.point_uncertainty(p, mode).astype(np.float32), mode)
        assert np.array_equal(cls, want_cls)
    unc, _ = P.point_uncertainty(p, "entropy")
    assert np.abs(unc.astype(np.float64) - _entropy64(p)).max() <= 2 * _entropy_bound()[0]


# ---- A2. region statistics ---------------------------------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 7, 8, 9, 127, 128, 129, K.RS_CAP, K.RS_CAP + 1, K.NP_BUFSIZE, K.NP_BUFSIZE + 1)


@functools.lru_cache(None)
def _region_case(extra):
    """the twelve size classes twice (random classes of 32, class 31 among them | two or three classes with EQUAL counts), `extra` regions of 1-3 points
    behind them (S = 24 + extra); uncertainties of both signs.  -> inputs and the oracle's three results"""
    rng = np.random.default_rng(31 + extra)
    sizes = list(SIZES) + [6 if m == 7 else m for m in SIZES] + [1 + (i % 3) for i in range(extra)]          # (6: a tie below 8 members)
    off, pts, n = P.csr(rng, sizes)
    unc = (rng.random(n, dtype=np.float32) - np.float32(0.25)).astype(np.float32)
    cls = rng.integers(0, 32, n).astype(np.int32)
    cls[rng.random(n) < 0.1] = 31
    tied = {}
    for s in range(len(SIZES), 2 * len(SIZES)):          # equal counts: classes 5, 9 (and 2 when the size is a multiple of three), dealt round-robin from a shuffled start
        m = sizes[s]
        group = (9, 5, 2) if m % 3 == 0 else (9, 5)
        if m >= len(group) and m % len(group) == 0:
            cls[pts[off[s]:off[s + 1]]] = np.resize(group, m)
            tied[s] = min(group)
    want = {mode: O.region_stats(unc, cls, off, pts, 32, mode) for mode in MODES}
    return sizes, off, pts, unc, cls, want, tied


@pytest.mark.parametrize("extra", [1, 2, 3])
def test_region_stats_sizes(backend, extra):
    """every size class of sel_region_stats_w at S = 1, 2, 3 (mod 4), three modes, on bits; the lowest class wins equal counts"""
    sizes, off, pts, unc, cls, want, tied = _region_case(extra)
    pl = P.plan_region(sizes, P.num_cu(backend))
    assert len(sizes) % 4 == (24 + extra) % 4 == extra % 4 and pl.tail_waves == extra % 4 and pl.trips == 1
    assert set(pl.branch) == {"empty", "lane", "w8", "chunked"} and pl.buffers.max() == 2 and (pl.blocks[pl.branch == "w8"] == 2).any()
    for s, m in enumerate(SIZES):
        assert pl.branch[s] == ("empty" if m == 0 else "lane" if m < 8 else "w8" if m <= K.RS_CAP else "chunked")
    top2 = lambda s: np.sort(np.bincount(cls[pts[off[s]:off[s + 1]]]))[-2:]
    assert len(tied) >= 4 and all(top2(s)[0] == top2(s)[1] for s in tied) and {"lane", "w8", "chunked"} <= {pl.branch[s] for s in tied} and (cls == 31).any()
    for mode in MODES:
        ru, dom, cnt = P.region_stats(unc, cls, off, pts, 32, mode)
        w_ru, w_dom, w_cnt = want[mode]
        assert np.array_equal(dom, w_dom) and np.array_equal(cnt, w_cnt), mode
        assert all(dom[s] == c and cnt[s] == top2(s)[1] for s, c in tied.items()), "equal counts: the lowest class wins"
        P.assert_bits(ru, w_ru, "region_unc, mode %s" % mode)


@functools.lru_cache(None)
def _zero_case():
    """per size class three regions: members of -0.0 only, of +0.0 only, zeros of both signs among positive values"""
    rng = np.random.default_rng(41)
    sizes = [m for m in SIZES if m for _ in range(3)]
    off, pts, n = P.csr(rng, sizes)
    unc = np.empty(n, np.float32)
    for s, m in enumerate(sizes):
        ids = pts[off[s]:off[s + 1]]
        unc[ids] = [np.full(m, -0.0), np.full(m, 0.0), np.where(np.arange(m) % 3 == 0, rng.random(m), np.where(np.arange(m) % 3 == 1, -0.0, 0.0))][s % 3]
    cls = rng.integers(0, 13, n).astype(np.int32)
    return sizes, off, pts, unc, cls, {mode: O.region_stats(unc, cls, off, pts, 13, mode) for mode in MODES}


@pytest.mark.parametrize("mode", MODES)
def test_region_stats_signed_zero(backend, mode):
    """NumPy's reduction is identity + pairwise(...): a sum of -0.0 members is +0.0, at every size.  (Before the fix the eight accumulators, started from the
    first terms, returned -0.0 from 8 members on in `mean` and `sum_weight`.)"""
    sizes, off, pts, unc, cls, want = _zero_case()
    pl = P.plan_region(sizes, P.num_cu(backend))
    assert {"lane", "w8", "chunked"} <= set(pl.branch)
    neg = [s for s in range(len(sizes)) if s % 3 == 0]
    assert all(np.signbit(unc[pts[off[s]:off[s + 1]]]).all() and (unc[pts[off[s]:off[s + 1]]] == 0).all() for s in neg)
    ru, dom, cnt = P.region_stats(unc, cls, off, pts, 13, mode)
    assert np.array_equal(dom, want[mode][1]) and np.array_equal(cnt, want[mode][2])
    P.assert_bits(ru, want[mode][0], "region_unc of signed zeros, mode %s" % mode)
    if mode != "WetSU":
        P.assert_bits(ru[neg], np.zeros(len(neg)), "a sum of -0.0 members")


def test_region_stats_onehot_entropy_chain(backend):
    """the issue's six regions of 3, 8, 20, 5, 9 and 130 one-hot points: entropy -0.0 per point, region mean +0.0, ranking [0 1 2 3 4 5]"""
    rng = np.random.default_rng(43)
    sizes = [3, 8, 20, 5, 9, 130]
    off, pts, n = P.csr(rng, sizes)
    p = np.zeros((n, 13), np.float32); p[np.arange(n), rng.integers(0, 13, n)] = 1
    unc, cls = P.point_uncertainty(p, "entropy")
    P.assert_bits(unc, np.full(n, -0.0, np.float32), "entropy of one-hot rows")
    for mode in ("mean", "sum_weight"):
        ru, _, _ = P.region_stats(unc, cls, off, pts, 13, mode)
        P.assert_bits(ru, O.region_stats(unc, cls, off, pts, 13, mode)[0], mode)
        P.assert_bits(ru, np.zeros(6), mode)
        assert np.array_equal(P.rank_regions(ru), np.arange(6))


@functools.lru_cache(None)
def _many_regions():
    S = max(K.CU_GPU, K.CU_EMU) * K.WAVE_GRID * 4 + 5
    rng = np.random.default_rng(47)
    sizes = rng.integers(1, 4, S)
    off, pts, n = P.csr(rng, sizes)
    unc = rng.random(n, dtype=np.float32); cls = rng.integers(0, 13, n).astype(np.int32)
    return sizes, off, pts, unc, cls, O.region_stats(unc, cls, off, pts, 13, "mean"), O.dominant_labels(cls, off, pts)


def test_region_stats_second_trip(backend):
    """more regions of 1-3 points than the capped grid has waves: the wave loop's second trip (sel_region_stats_w and sel_dominant_label)"""
    sizes, off, pts, unc, cls, want, want_dom = _many_regions()
    cu = P.num_cu(backend)
    assert P.plan_region(sizes, cu).trips >= 2 and P.plan_region(sizes, cu).grid == cu * K.WAVE_GRID and P.plan_dominant(sizes, cu).trips >= 2
    ru, dom, cnt = P.region_stats(unc, cls, off, pts, 13, "mean")
    assert np.array_equal(dom, want[1]) and np.array_equal(cnt, want[2])
    P.assert_bits(ru, want[0], "region_unc")
    lab, pur = P.dominant_label(cls, off, pts, 13)
    assert np.array_equal(lab, want_dom[0])
    P.assert_bits(pur, want_dom[1], "purity")


# ---- A3. dominant label ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_labels", [1, 13, 64])
def test_dominant_label(backend, num_labels):
    """sizes around a lane's trip of 256 members, empty regions (purity 0), ties (the lowest label), purity on bits"""
    rng = np.random.default_rng(51 + num_labels)
    sizes = [0, 1, 255, 256, 257, 1025, 0, 2, 256, 1024, 6]
    off, pts, n = P.csr(rng, sizes)
    labels = rng.integers(0, num_labels, n).astype(np.int32)
    tied = [7, 8, 9, 10] if num_labels > 1 else []
    for s in tied:          # the top label of the region's range and a lower one, half each
        hi = num_labels - 1
        labels[pts[off[s]:off[s + 1]]] = np.resize([hi, hi // 2], sizes[s])
    pl = P.plan_dominant(sizes, P.num_cu(backend))
    assert set(pl.member_trips) == {0, 1, 2, 4, 5} and pl.trips == 1
    want_lab, want_pur = O.dominant_labels(labels, off, pts)
    assert all(want_lab[s] == (num_labels - 1) // 2 and want_pur[s] == 0.5 for s in tied) and want_pur[0] == 0
    lab, pur = P.dominant_label(labels, off, pts, num_labels)
    assert np.array_equal(lab, want_lab)
    P.assert_bits(pur, want_pur, "purity")


# ---- A4. class balance, mask ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _clsbal_inputs():
    rng = np.random.default_rng(61)
    S = 1031
    rclass = rng.integers(0, 13, S).astype(np.int32)
    ru = rng.random(S) * 2 - 0.5                                   # WetSU's negative values among them
    ru[::50] = 0.0; ru[7::50] = -0.0
    skip = (rng.random(S) < 0.3).astype(np.uint8)
    selected = rng.integers(0, 13, 77).astype(np.int32)
    return S, rclass, ru, skip, selected


def _clsbal_ld(rclass, ru, selected):
    """the formula of add_clsbal with the weight as NumPy has it (float64) and exp and the product in numpy.longdouble"""
    lst = list(rclass) + list(selected)
    h = np.bincount(np.asarray(lst, np.int64), minlength=13) / len(lst)
    w = h[np.asarray(rclass, np.int64)]
    return np.asarray(ru, np.longdouble) * np.exp(-np.asarray(w, np.longdouble))


@functools.lru_cache(None)
def _clsbal_bound():
    """O.add_clsbal (float64) against the same formula in numpy.longdouble: the largest relative error E over the four flavours of the case.  The device may
    be 2 E off (its exp and NumPy's differ in the last place)."""
    S, rclass, ru, skip, selected = _clsbal_inputs()
    worst = 0.0
    for use_skip in (False, True):
        for sel in ((), tuple(selected)):
            keep = skip == 0 if use_skip else np.ones(S, bool)
            ld = _clsbal_ld(rclass[keep], ru[keep], sel)
            got = O.add_clsbal(13, rclass[keep], ru[keep], sel)
            nz = ld != 0
            worst = max(worst, float((np.abs(got[nz] - ld[nz]) / np.abs(ld[nz])).max()))
    return worst


@pytest.mark.parametrize("use_sel", [False, True], ids=["noselected", "selected"])
@pytest.mark.parametrize("use_skip", [False, True], ids=["noskip", "skip"])
def test_clsbal(backend, use_skip, use_sel):
    S, rclass, ru, skip, selected = _clsbal_inputs()
    assert np.finfo(np.longdouble).nmant > 52, "numpy.longdouble is no wider than float64 here"
    sel = selected if use_sel else np.zeros(0, np.int32)
    keep = skip == 0 if use_skip else np.ones(S, bool)
    assert (ru < 0).any() and (P.bits(ru) == P.bits(np.array([-0.0]))[0]).any() and (P.bits(ru) == 0).any()
    pl = P.plan_clsbal(S, len(sel), skip if use_skip else None)
    assert pl.total_from_hist == use_skip and pl.counted == int(keep.sum()) + len(sel) and pl.hist_grid > 1
    got = P.clsbal(rclass, skip if use_skip else None, sel, ru)
    got_h, hist = P.clsbal_hist(rclass, skip if use_skip else None, sel, ru)
    assert np.array_equal(hist[:13], np.bincount(np.concatenate([rclass[keep], sel]), minlength=13)) and not hist[13:].any()
    P.assert_bits(got_h, got, "supplied-histogram flavour against the one-call flavour")
    ld = _clsbal_ld(rclass[keep], ru[keep], sel)
    E = _clsbal_bound()
    nz = ld != 0
    err = np.abs(got[keep][nz].astype(np.longdouble) - ld[nz]) / np.abs(ld[nz])
    print("clsbal skip=%s selected=%s: device relative error %.3e, oracle's own (bound / 2) %.3e" % (use_skip, use_sel, float(err.max()), E))
    assert float(err.max()) <= 2 * E
    want = O.add_clsbal(13, rclass[keep], ru[keep], sel)
    zero = ru[keep] == 0
    P.assert_bits(got[keep][zero], want[zero], "zeros keep their sign")
    assert np.array_equal(np.signbit(got[keep]), np.signbit(want))


@pytest.mark.parametrize("pad", [0, 5])
def test_mask_regions(backend, pad):
    rng = np.random.default_rng(71)
    S = 1000
    u = rng.random(S) - 0.5; u[3] = -0.0; u[4] = np.inf
    lab = (rng.random(S) < 0.4).astype(np.uint8)
    pl = P.plan_mask(S, S + pad)
    assert pl.pad == pad and pl.tail == (S + pad) % 256 and lab.any() and not lab.all()
    out = P.mask_regions(u, lab, S + pad)
    want = np.where(lab != 0, -np.inf, u)
    P.assert_bits(out[:S], want, "masked")
    assert (P.bits(out[:S])[lab != 0] == P.NEG_INF_BITS).all() and (P.bits(out[S:S + pad]) == P.NEG_INF_BITS).all()
    P.assert_bits(out[S + pad:], np.full(3, 7.5), "behind S_padded")


# ---- A5. segment mean -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_sel", [False, True], ids=["all", "sel"])
def test_segment_mean(backend, with_sel):
    """regions around the 32-member unroll; the dominant class on the first member only, on the last only, on random members"""
    rng = np.random.default_rng(81)
    sizes = [m for m in (31, 32, 33, 65) for _ in range(3)] + [1, 64]
    off, pts, n = P.csr(rng, sizes)
    feat = rng.normal(0, 1, (n, 32)).astype(np.float32)
    cls = rng.integers(0, 5, n).astype(np.int32)
    dom = rng.integers(0, 5, len(sizes)).astype(np.int32)
    for s in range(12):
        ids = pts[off[s]:off[s + 1]]
        if s % 3 == 0: cls[ids] = (dom[s] + 1) % 5; cls[ids[0]] = dom[s]
        elif s % 3 == 1: cls[ids] = (dom[s] + 1) % 5; cls[ids[-1]] = dom[s]
        else: cls[ids[0]] = dom[s]
    for s in (12, 13):
        cls[pts[off[s]:off[s + 1]]] = dom[s]
    assert all((cls[pts[off[s]:off[s + 1]]] == dom[s]).sum() == 1 for s in range(12) if s % 3 != 2)
    pl = P.plan_segment(sizes)
    assert sorted(set(pl.trips)) == [1, 2, 3] and pl.clipped[:3].all() and not pl.clipped[3:6].any() and pl.clipped[6:12].all()
    want = O.segment_mean_features(feat, off, pts, cls, dom)
    sel = rng.permutation(len(sizes)).astype(np.int32)[:9] if with_sel else None
    got = P.segment_mean(feat, cls, dom, off, pts, sel)
    P.assert_bits(got, want if sel is None else want[sel], "segment means")


# ---- B. ranking ---------------------------------------------------------------------------------------------------------------------------------------------
RANK_S = (1, 2, 31, 32, 33, K.RANK_SMALL - 1, K.RANK_SMALL, K.RANK_SMALL + 1, K.RADIX_WIDE - 1, K.RADIX_WIDE)
SUB = 5e-324


def _rank_values(S, kind):
    rng = np.random.default_rng(91 + S)
    r = np.arange(S)
    if kind == "ties":          # heavy exact ties, +-inf (many -inf, as ssdr_mask_regions_dev leaves them), subnormals of both signs
        u = rng.integers(0, 7, S).astype(np.float64) / 4 - 0.5
        u[rng.random(S) < 0.3] = -np.inf
        u[r % 11 == 3] = np.inf; u[r % 13 == 4] = SUB; u[r % 13 == 5] = -SUB; u[r % 17 == 6] = 3 * SUB
    elif kind == "zeros":       # +0.0 and -0.0 interleaved between values of both signs
        u = np.where(r % 2 == 0, 0.0, -0.0)
        u[r % 5 == 2] = 1.5; u[r % 7 == 3] = -1.5; u[r % 9 == 4] = SUB; u[r % 9 == 5] = -SUB
    else:                       # NaN of both signs, several of them, among everything else
        u = rng.integers(0, 5, S).astype(np.float64) - 2
        u[r % 6 == 1] = -np.inf; u[r % 10 == 7] = np.inf; u[r % 8 == 0] = -0.0
        nan_pos = np.array([0x7ff8000000000000, 0x7ff0000000000001], np.uint64).view(np.float64)          # quiet, signalling
        nan_neg = np.array([0xfff8000000000001, 0xffffffffffffffff], np.uint64).view(np.float64)          # the second one is -u's all-ones pattern
        u[r % 4 == 2] = np.resize(nan_pos, (r % 4 == 2).sum()); u[r % 5 == 3] = np.resize(nan_neg, (r % 5 == 3).sum())
    return u


@pytest.mark.parametrize("kind", ["ties", "zeros", "nan"])
@pytest.mark.parametrize("S", RANK_S)
def test_rank_regions(backend, S, kind):
    """index for index np.argsort(-u, kind="stable"): +0.0 and -0.0 are equal, every NaN ranks last, equal keys by ascending index"""
    u = _rank_values(S, kind)
    assert P.plan_rank(S) == ("count" if S <= K.RANK_SMALL else "radix" if S < K.RADIX_WIDE else "radix_wide")
    if S >= 31:
        if kind == "ties": assert np.isneginf(u).sum() > S // 5 and np.isposinf(u).any() and (np.abs(u) == SUB).any() and len(np.unique(u)) < 16
        if kind == "zeros": assert ((u == 0) & np.signbit(u)).sum() > S // 5 and ((u == 0) & ~np.signbit(u)).sum() > S // 5
        if kind == "nan": assert (np.isnan(u) & np.signbit(u)).sum() > 3 and (np.isnan(u) & ~np.signbit(u)).sum() > 3
    want = np.argsort(-u, kind="stable").astype(np.int32)
    if kind == "nan" and S >= 31:
        nn = int(np.isnan(u).sum())
        assert np.array_equal(want[S - nn:], np.flatnonzero(np.isnan(u))), "NumPy ranks NaN last, by ascending index"
    got = P.rank_regions(u)
    assert np.array_equal(got, want), "first difference at rank %d" % np.flatnonzero(got != want)[0]
