"""The training step's launchers (csrc/randla_train.hip: launch_gemm, launch_dw, launch_reduce_chunks / launch_combine, the loss's grid), branch by
branch, against float64 on the same float32 inputs.  Every case runs on the CPU logic build and, marked gpu, on the gfx950 build (the ``backend``
fixture), and first asserts from tests/_train_paths.plan that it is on the branch it names.  The pieces call the launch functions the tape calls, so
the split and chunk rules under test are the step's own.  Bars: tests/_train_paths.py's docstring (derived, not measured); every case prints its
largest error / bar.  DESIGN.md "The training step's launchers, branch by branch" has the table."""
import itertools
import re

import numpy as np
import pytest

import _train_cases as TC
import _train_oracle as O
import _train_paths as TP
from test_randla_train import MIN_VAR, _dev_mask, _logits_bar, _near_ties, _trainer

F32, U = np.float32, TP.U

# ---- the shapes ----------------------------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = {"16x16": [(1, 1, 1), (10, 8, 33), (16, 16, 16)],
               "256x16": [(256, 16, 32), (257, 13, 6), (300, 3, 17), (1000, 16, 10)],
               "16x256": [(8, 32, 40), (16, 257, 16), (3, 1024, 33)],
               "64x64": [(17, 17, 1), (64, 64, 16), (65, 65, 17), (130, 100, 50)]}
GEMM_CASES = [(t, s) for t, ss in GEMM_SHAPES.items() for s in ss]

# (in, out, M, transposed output, what plan must say)
DW_CASES = [(6, 8, 100, False, dict(nz=1, k_tail=4, tile="16x16")),
            (8, 32, 511, False, dict(nz=1, k_tail=15, tile="16x256")),
            (64, 64, 1024, False, dict(nz=2, kchunk=512, ragged=False, k_tail=0, tile="64x64")),
            (10, 8, 1039, False, dict(nz=2, kchunk=528, last=511, k_tail=15, tile="16x16")),
            (128, 256, 3840, False, dict(nz=7, kchunk=560, last=480, ragged=True, tile="64x64")),
            (13, 32, 12800, False, dict(nz=25, kchunk=512, tile="16x256")),
            (64, 64, 1024, True, dict(nz=2, kchunk=512, tile="64x64")),
            (512, 512, 16400, False, dict(nz=32, want=32, cap_bound=False, tile="64x64")),
            (512, 512, 17280, False, dict(nz=32, want=33, split=32, cap_bound=True, kchunk=544, tile="64x64")),
            (300, 10, 530, False, dict(nz=1, k_tail=2, tile="256x16"))]

# (M, C, what plan must say)
REDUCE_CASES = [(1, 8, dict(nchunks=1, few_rows=True)),
                (31, 8, dict(nchunks=1, few_rows=True, nsub=32)),
                (1023, 8, dict(nchunks=1)),
                (1024, 13, dict(nchunks=1, ct=16, below_ct=True)),
                (2049, 8, dict(nchunks=2, chunk=1025, last=1024, ragged=True)),
                (12800, 64, dict(nchunks=12, chunk=1067, last=1063, ragged=True)),
                (3000, 100, dict(nchunks=2, ct=64, cblocks=2, partial_cblock=True)),
                (23040, 16, dict(nchunks=22, chunk=1048, last=1032, ragged=True)),
                (80, 1024, dict(nchunks=1, cblocks=16))]


def _says(p, want, what):
    for k, v in want.items():
        got = getattr(p, k)
        got = TP.tile_name(got) if k == "tile" else got
        assert got == v, "%s: plan says %s = %s, the case needs %s" % (what, k, got, v)


# ---- GEMM ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,shape", GEMM_CASES, ids=["%s-%dx%dx%d" % ((t,) + s) for t, s in GEMM_CASES])
def test_gemm_piece(backend, tile, shape):
    """C (+)= A B (+ bias): A and B row-major and transposed, once with leading dimensions above the width and views that start at an odd column, once
    with C transposed; bias on and off; accumulate off over NaN (everything inside is overwritten) and on over random values; C's padding columns and the
    rows behind M keep their sentinel bit for bit."""
    M, N, K = shape
    p = TP.gemm_plan(M, N, K)
    assert TP.tile_name(p.tile) == tile and p.nz == 1 and p.chain == K, "not the %s tile" % tile
    rng = np.random.default_rng([M, N, K])
    worst = 0.0
    layouts = [(ta, tb, 0, 0, False) for ta in (False, True) for tb in (False, True)] + [(False, True, 5, 3, False), (True, False, 7, 1, False), (False, False, 0, 0, True)]
    for ta, tb, pad, off, tc in layouts:
        A = TP.strided(rng, M, K, ta, pad, off)
        B = TP.strided(rng, K, N, tb, pad, off)
        a64, b64 = A[4].astype(np.float64), B[4].astype(np.float64)
        prod, mag = a64 @ b64, np.abs(a64) @ np.abs(b64)
        bias = rng.standard_normal(N).astype(F32)
        for use_bias, acc in itertools.product((False, True), (False, True)):
            # C [M + 2 rows, N + 6 columns], the view starts at column 3 (row 3 when transposed)
            old = rng.standard_normal((M, N)).astype(F32) if acc else np.full((M, N), np.nan, F32)
            cb, c_off, crs, ccs, cv = TP.strided(rng, M + 2, N, tc, 6, 3, fill=TP.SENT)
            cv[:M] = old
            before = cb.copy()
            got = TP.run_gemm(A, B, cb, c_off, crs, ccs, M, N, K, bias if use_bias else None, acc)
            gv = (got[:, 3:3 + M + 2].T if tc else got[:, 3:3 + N])[:M]
            ref = prod + (bias.astype(np.float64) if use_bias else 0) + (old.astype(np.float64) if acc else 0)
            bar = (K + 2) * U * (mag + (np.abs(bias) if use_bias else 0) + (np.abs(old) if acc else 0))
            what = "gemm %s A%s B%s C%s pad %d bias %d accumulate %d" % (shape, "T" if ta else "", "T" if tb else "", "T" if tc else "", pad, use_bias, acc)
            assert np.isfinite(gv).all(), what + ": not every element inside was written"
            err = np.abs(gv - ref)
            assert (err <= bar).all(), "%s: error / bar %.3g at %s" % (what, (err / bar).max(), np.unravel_index(np.argmax(err / bar), err.shape))
            worst = max(worst, float((err / bar).max()))
            outside = np.ones(cb.shape, bool)
            (outside[:, 3:3 + M + 2].T if tc else outside[:, 3:3 + N])[:M] = False
            assert np.array_equal(got.view(np.uint32)[outside], before.view(np.uint32)[outside]), what + ": wrote outside C"
    print("gemm %s %s: largest error / bar %.3g" % (tile, shape, worst))


def test_gemm_piece_refusals(backend):
    L = TP.bound()
    a, b, c = (TP._up(np.zeros(4, F32)) for _ in range(3))
    ok = [a.ptr, 2, 1, b.ptr, 2, 1, c.ptr, 2, 1, 2, 2, 2, None, 0, None]
    assert L.ssdr_randla_train_gemm_dev(*ok) == 0
    for hole, val in ((0, None), (3, None), (6, None), (9, 0), (10, 0), (11, 0), (9, -1)):
        bad = list(ok); bad[hole] = val
        assert L.ssdr_randla_train_gemm_dev(*bad) == TP.ERR_INVALID and L.ssdr_last_error(), (hole, val)
    okw = [a.ptr, 2, b.ptr, 2, 2, 1, c.ptr, 1, 1, None]
    assert L.ssdr_randla_train_dw_dev(*okw) == 0
    for hole, val in ((0, None), (2, None), (6, None), (3, 0), (4, 0), (5, 0), (1, 1), (4, 1 << 20)):
        bad = list(okw); bad[hole] = val
        if hole == 4 and val > 2:
            bad[1], bad[5] = val, 16
        assert L.ssdr_randla_train_dw_dev(*bad) == TP.ERR_INVALID and L.ssdr_last_error(), (hole, val)
    okr = [0, a.ptr, 2, None, None, 0, 0, None, None, 2, 2, b.ptr, c.ptr, None, None, 0, None]
    assert L.ssdr_randla_train_reduce_dev(*okr) == 0
    for hole, val in ((0, 3), (0, -1), (1, None), (11, None), (12, None), (9, 0), (10, 0), (2, 1), (13, a.ptr), (0, 1)):
        bad = list(okr); bad[hole] = val
        assert L.ssdr_randla_train_reduce_dev(*bad) == TP.ERR_INVALID and L.ssdr_last_error(), (hole, val)
    from ssdr_al import _lib
    _lib.sync()


# ---- dW --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,M,transposed,want", DW_CASES, ids=["%dx%d-M%d%s" % (c[0], c[1], c[2], "-T" if c[3] else "") for c in DW_CASES])
def test_dw_piece(backend, cin, cout, M, transposed, want):
    """dW = x^T dz through the launcher's own split / kchunk / nz; x a view with a leading dimension above its width that starts at an odd column"""
    p = TP.dw_plan(M, cin, cout)
    _says(p, want, "dW (%d, %d, %d)" % (cin, cout, M))
    rng = np.random.default_rng([cin, cout, M])
    xb, x_off, ldx, _, xv = TP.strided(rng, M, cin, False, 3, 1)
    dz = rng.standard_normal((M, cout)).astype(F32)
    out = np.full(cin * cout + 5, TP.SENT, F32)
    rs, cs = (1, cin) if transposed else (cout, 1)
    got = TP.run_dw(xb, x_off, ldx, dz, M, cin, cout, out, rs, cs)
    gv = got[:cin * cout].reshape(cout, cin).T if transposed else got[:cin * cout].reshape(cin, cout)
    x64, d64 = xv.astype(np.float64), dz.astype(np.float64)
    ref, mag = x64.T @ d64, np.abs(x64).T @ np.abs(d64)
    bar = (p.n + 2) * U * mag
    err = np.abs(gv - ref)
    print("dW (%d, %d, %d)%s: kchunk %d, nz %d, last %d; largest error / bar %.3g" % (cin, cout, M, " transposed" if transposed else "", p.kchunk, p.nz, p.last, (err / bar).max()))
    assert np.isfinite(gv).all() and (err <= bar).all(), "error / bar %.3g" % (err / bar).max()
    assert (got[cin * cout:] == TP.SENT).all(), "wrote behind dW"


# ---- reductions --------------------------------------------------------------------------------------------------------------------------------------------
def _z(rng, M, Cn, mean=0.0):
    """z [M, C] as a view of a [M, C + 3] buffer from column 1"""
    buf = (rng.standard_normal((M, Cn + 3)) + mean).astype(F32)
    return buf, 1, Cn + 3, buf[:, 1:1 + Cn]


@pytest.mark.parametrize("M,Cn,want", REDUCE_CASES, ids=["%dx%d" % c[:2] for c in REDUCE_CASES])
def test_reduce_stats_piece(backend, M, Cn, want):
    """mode 0: mean and 1 / sqrt(var + eps), and the moving statistics with unbiased 0 and 1; once on data with mean 1000 and deviation 1, where the
    naive float32 E[x^2] - E[x]^2 misses the bar (asserted first): Chan's merge, not the naive rule"""
    p = TP.reduce_plan(M, Cn)
    _says(p, want, "reduce (%d, %d)" % (M, Cn))
    rng = np.random.default_rng([M, Cn, 0])
    worst = 0.0
    for mean in (0.0, 1000.0):
        zb, off, ld, zv = _z(rng, M, Cn, mean)
        o = TP.stats_oracle(zv, p)
        if mean and M > 1:
            naive = (zv * zv).mean(0, dtype=F32) - zv.mean(0, dtype=F32) ** 2
            assert (np.abs(naive - o.var) > o.bar_var).any(), "the offset data does not separate Chan's merge from the naive rule"
        for unbiased in (0, 1):
            m0, v0 = rng.standard_normal(Cn).astype(F32), (rng.random(Cn) + 0.5).astype(F32)
            g0, g1, mm, mv = TP.run_reduce(0, zb, off, ld, M, Cn, mov=(m0, v0), unbiased=unbiased)
            assert g0[Cn] == TP.SENT and g1[Cn] == TP.SENT
            e_mu, e_inv = np.abs(g0[:Cn] - o.mu) / o.bar_mu, np.abs(g1[:Cn] - o.inv) / o.bar_inv
            assert (e_mu <= 1).all() and (e_inv <= 1).all(), "mean %g: mean error / bar %.3g, invstd error / bar %.3g" % (mean, e_mu.max(), e_inv.max())
            fac = M / (M - 1.0) if unbiased and M > 1 else 1.0
            ref_m = m0 - (m0.astype(np.float64) - o.mu) * 0.01
            ref_v = v0 - (v0.astype(np.float64) - o.var * fac) * 0.01
            bar_m = 0.01 * o.bar_mu + 4 * U * np.maximum(np.abs(m0), np.abs(o.mu))           # three roundings of numbers no larger than max(|m|, |x|), 0.01f's own
            bar_v = 0.01 * fac * (o.bar_var + 2 * U * o.var) + 4 * U * np.maximum(np.abs(v0), o.var * fac)
            e_m, e_v = np.abs(mm - ref_m) / bar_m, np.abs(mv - ref_v) / bar_v
            assert (e_m <= 1).all() and (e_v <= 1).all(), "moving statistics (unbiased %d): %.3g, %.3g" % (unbiased, e_m.max(), e_v.max())
            worst = max(worst, e_mu.max(), e_inv.max(), e_m.max(), e_v.max())
        g0, g1, _, _ = TP.run_reduce(0, zb, off, ld, M, Cn)                                    # without the moving statistics: the same values
        assert (np.abs(g0[:Cn] - o.mu) <= o.bar_mu).all() and (np.abs(g1[:Cn] - o.inv) <= o.bar_inv).all()
    print("reduce mode 0 (%d, %d): %d chunks of %d, last %d; largest error / bar %.3g" % (M, Cn, p.nchunks, p.chunk, p.last, worst))


@pytest.mark.parametrize("M,Cn,want", REDUCE_CASES, ids=["%dx%d" % c[:2] for c in REDUCE_CASES])
def test_reduce_bnbwd_piece(backend, M, Cn, want):
    """mode 1: sum dY and sum dY xhat, act off and on; with act some av are exactly 0 and -0, both on the 0.2 side"""
    p = TP.reduce_plan(M, Cn)
    _says(p, want, "reduce (%d, %d)" % (M, Cn))
    rng = np.random.default_rng([M, Cn, 1])
    zb, off, ld, zv = _z(rng, M, Cn, 0.5)
    lda = Cn + 4
    da, av = rng.standard_normal((M, lda)).astype(F32), rng.standard_normal((M, lda)).astype(F32)
    flat = av[:, 3:3 + Cn]
    pick = rng.random(flat.shape)
    flat[pick < 0.1] = 0.0
    flat[pick > 0.9] = -0.0
    if M * Cn >= 40:
        assert np.signbit(flat[flat == 0]).any() and not np.signbit(flat[flat == 0]).all(), "the case needs av of exactly 0 and exactly -0"
    mean, invstd = rng.standard_normal(Cn).astype(F32), (rng.random(Cn) + 0.5).astype(F32)
    worst = 0.0
    for act in (0, 1):
        g0, g1, _, _ = TP.run_reduce(1, zb, off, ld, M, Cn, da=da, av=av, a_off=3, lda=lda, act=act, mean=mean, invstd=invstd)
        assert g0[Cn] == TP.SENT and g1[Cn] == TP.SENT
        dy = da[:, 3:3 + Cn].astype(np.float64)
        if act:
            dy = np.where(flat > 0, dy, dy * float(F32(0.2)))
        xh = (zv.astype(np.float64) - mean) * invstd
        e0 = np.abs(g0[:Cn] - dy.sum(0)) / ((p.n + 1) * U * np.abs(dy).sum(0))
        e1 = np.abs(g1[:Cn] - (dy * xh).sum(0)) / ((p.n + 4) * U * np.abs(dy * xh).sum(0))
        assert (e0 <= 1).all() and (e1 <= 1).all(), "act %d: sum dY error / bar %.3g, sum dY xhat error / bar %.3g" % (act, e0.max(), e1.max())
        worst = max(worst, e0.max(), e1.max())
        if act and M * Cn >= 40:                                                               # a zero on the 1.0 side would move the sum by more than the bar
            wrong = np.where(flat >= 0, da[:, 3:3 + Cn].astype(np.float64), dy)
            assert (np.abs(wrong.sum(0) - dy.sum(0)) > (p.n + 1) * U * np.abs(dy).sum(0)).any()
    print("reduce mode 1 (%d, %d): largest error / bar %.3g" % (M, Cn, worst))


@pytest.mark.parametrize("M,Cn,want", REDUCE_CASES, ids=["%dx%d" % c[:2] for c in REDUCE_CASES])
def test_reduce_sum_piece(backend, M, Cn, want):
    """mode 2: the bias gradient's column sums"""
    p = TP.reduce_plan(M, Cn)
    _says(p, want, "reduce (%d, %d)" % (M, Cn))
    rng = np.random.default_rng([M, Cn, 2])
    zb, off, ld, zv = _z(rng, M, Cn, 0.25)
    g0, g1, _, _ = TP.run_reduce(2, zb, off, ld, M, Cn)
    assert g0[Cn] == TP.SENT and (g1 == TP.SENT).all(), "mode 2 wrote out1 or behind out0"
    z64 = zv.astype(np.float64)
    e = np.abs(g0[:Cn] - z64.sum(0)) / (p.n * U * np.abs(z64).sum(0))
    print("reduce mode 2 (%d, %d): largest error / bar %.3g" % (M, Cn, e.max()))
    assert (e <= 1).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------
K_TAILS = ["dW: k tail in the %s tile" % t for t in ("16x16", "256x16", "16x256", "64x64")]
RAGGED_REDUCE = ["reduce mode %d: last row chunk shorter than chunk" % m for m in range(3)]
# what plan must say of a case before it runs: the branches it is there for, and one launch that shows the numbers the table quotes
E2E = {"b3n360": (K_TAILS + ["dW: last k-chunk shorter than kchunk", "forward: partial M tile of the 256x16 kernel", "loss: a row count that is no multiple of 256"],
                  ("Encoder_layer_0LFAmlp1", "dW", dict(K=17280, kchunk=528, nz=33, last=384))),
       "odd": (K_TAILS + ["reduce mode 0: C below ct", "reduce mode 1: C below ct", "gemm_kernel<64x64> as forward / dx"], ("fc", "forward", dict(M=1080, N=19, tile=(64, 64)))),
       "b5n400": (RAGGED_REDUCE, ("Encoder_layer_0LFAmlp1", "reduce0", dict(M=32000, nchunks=31, chunk=1033, last=1010))),
       "b3n480": (RAGGED_REDUCE, ("Encoder_layer_0LFAmlp1", "reduce0", dict(M=23040, nchunks=22, chunk=1048, last=1032))),
       "five_r": (RAGGED_REDUCE + ["dW: last k-chunk shorter than kchunk"], ("Encoder_layer_1LFAmlp1", "reduce1", dict(M=23040, C=32, nchunks=22, last=1032))),
       "loss257": (["loss: more than 256 row blocks into the combining block", "loss: a row count that is no multiple of 256"] + RAGGED_REDUCE,
                   ("fc", "dW", dict(K=65824, nz=125, last=352)))}


def _on_its_branches(case, cfg, B):
    pl = TP.plan(cfg, B)
    want, (unit, role, fields) = E2E[case]
    missing = [b for b in want if b not in pl.branches]
    assert not missing, "%s is not on %s" % (case, missing)
    hit = [l for l in pl.launches if l.unit == unit and l.role == role]
    assert len(hit) == 1
    for k, v in fields.items():
        assert getattr(hit[0].p, k) == v, "%s %s %s: plan says %s = %s, the case needs %s" % (case, unit, role, k, getattr(hit[0].p, k), v)
    return pl


def _radix_tile():
    with open(TP.SRC.replace("randla_train.hip", "ssdr_internal.hpp")) as f:
        m = re.findall(r"constexpr int RADIX_TILE\s*=\s*([0-9]+)\s*;", f.read())
    assert len(m) == 1
    return int(m[0])


def _forward_and_loss(tr, case, dev, dm, moving, forward=True):
    """the bars of test_randla_train.py::test_training_forward_loss_and_moving_statistics: logits, features, then (one step, or one gradient call) loss,
    accuracy, moving statistics"""
    from ssdr_al import _lib
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case(case)
    lab = batch["labels"].reshape(-1)
    bar = _logits_bar(r64, r32)
    if forward:
        logits, f32 = tr.forward_arrays(dev, is_training=True, mask=dm)
        _lib.sync()
        err = np.abs(logits.to_host() - r64["logits"]).max()
        print("%s: logits %.3g (float32 torch %.3g, bar %.3g)" % (case, err, np.abs(r32["logits"] - r64["logits"]).max(), bar))
        assert err <= bar
        assert np.abs(f32.to_host() - r64["feat32"]).max() <= max(8 * np.abs(r32["feat32"] - r64["feat32"]).max(), 64 * U * np.abs(r64["feat32"]).max())
    if moving:
        tr.step_arrays(dev, mask=dm)
    else:
        tr.grads_arrays(dev, mask=dm)
    loss, acc = tr.loss(), tr.accuracy()
    print("%s: loss %.8g (float64 %.8g), accuracy %.6g (%.6g)" % (case, loss, r64["loss"], acc, r64["acc"]))
    assert abs(loss - r64["loss"]) <= 2 * float(np.max(cw)) * bar
    assert abs(acc - r64["acc"]) * r64["valid"] <= _near_ties(r64["logits"], lab, ign, cfg.num_classes, 2 * bar) + 1e-3
    assert tr.status() == 0
    if moving:
        mv, after, worst = O.moving_update(W, r64["stats"]), tr.weights(), 0.0
        for name, (mu, var) in mv.items():
            for got, ref, old in ((after[name]["bn"][2], mu, W[name]["bn"][2]), (after[name]["bn"][3], var, W[name]["bn"][3])):
                s = np.maximum(1.0, np.maximum(np.abs(ref), np.abs(old)))
                worst = max(worst, float((np.abs(got - ref) / s).max()))
        print("%s: moving statistics, worst error / scale %.3g" % (case, worst))
        assert worst <= 4e-7


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("case", ["b3n360", "odd", "b5n400", "b3n480", "five_r"])
def test_step_on_shapes_that_are_no_power_of_two(backend, case, det):
    """A whole training step at row counts that divide nothing: every gradient tensor under test_gradients' metric and bar (tests/_train_cases.check_gradients),
    loss and accuracy under the forward test's bars; in deterministic mode two calls agree in every bit.  The input conditions come from the two oracle
    runs alone: they agree on every sign and arg-max set, no degenerate batch norm, and every leaky-ReLU input and pooling gap is further from the
    decision than float32 moves it (TC.margins).  five_r has no seed in 1 .. 64 that meets them (a million leaky-ReLU inputs put one within 1e-9 of
    zero): forward, loss, accuracy and moving statistics only, as the existing 'five' case; forward values are continuous in a flipped sign."""
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case(case)
    B, N = batch["labels"].shape
    _on_its_branches(case, cfg, B)
    mg = TC.margins(r64, r32)
    print("%s: %s" % (case, TC.describe_margins(mg)))
    grad = case not in TC.NO_GRAD_CASES
    signs, ties, min_var = TC.conditions(r64, r32)
    assert min_var >= MIN_VAR, "a degenerate batch norm (variance %.3g)" % min_var
    if grad:
        assert signs and ties, "the float32 and float64 oracle runs disagree on a sign or an arg-max set: pick another seed"
        assert mg["ok"], "a leaky-ReLU input or a pooling gap within float32's reach of the decision: pick another seed"
    if det and case in ("b3n360", "odd", "b3n480"):
        assert B * N * 16 in (17280, 23040) and B * N * 16 % _radix_tile() != 0, "the key lists must not be whole sort tiles"
    tr = _trainer(cfg, W, cw, ign, deterministic=det)
    dev, dm = TC.to_device(batch), _dev_mask(mask)
    if not grad:
        _forward_and_loss(tr, case, dev, dm, moving=True)
        return
    tr.grads_arrays(dev, mask=dm)
    G = tr.grads()
    assert tr.step_count() == 0 and tr.status() == 0
    rows, bad, worst = TC.check_gradients(G, cfg, B, r64, r32)
    print("%s %s: %d tensors, largest metric / bar %.2f" % (case, "deterministic" if det else "default", len(rows), worst))
    assert not bad, "\n".join(bad)
    assert abs(tr.loss() - r64["loss"]) <= 2 * float(np.max(cw)) * _logits_bar(r64, r32)
    if det:
        tr.grads_arrays(dev, mask=dm)
        G2 = tr.grads()
        diff = [k for k in G if not np.array_equal(G[k].view(np.uint32), G2[k].view(np.uint32))]
        assert not diff, "two deterministic calls differ in %s" % diff


def test_margins_reject_the_seed_whose_sign_float32_flips(backend):
    """B = 3, N = 480 at make_batch seed 1: conditions() can hold (the two oracle runs agree wherever float32 torch happens to round as float64), yet the level-0 residual has a leaky-ReLU input at 5.1e-8 of
    its layer's largest, below 2^-24: a device that sums in another order takes the other sign there and 21 gradient tensors miss the bar by up to 44 x.
    margins() must say so from the oracle runs alone."""
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case("b3n480@1")
    signs, ties, min_var = TC.conditions(r64, r32)
    mg = TC.margins(r64, r32)
    print("b3n480 seed 1: conditions() says signs %s, arg-max sets %s, smallest variance %.3g; %s" % (signs, ties, min_var, TC.describe_margins(mg)))
    m, t = min(mg["lrelu"])
    assert not mg["ok"] and 4e-8 < m < 6e-8 and m < 2.0 ** -24 and m < t


@pytest.mark.parametrize("case", ["s3dis", "sem3d", "ties", "five", "five_b4"])
def test_margins_of_the_existing_cases_are_printed(backend, case):
    """what margins() says of the five cases of test_randla_train.py (recorded in DESIGN.md); no assertion on them: their seeds were chosen under conditions() alone"""
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case(case)
    mg = TC.margins(r64, r32)
    print("%s: %s" % (case, TC.describe_margins(mg)))
    assert len(mg["lrelu"]) == len(r64["signs"]) and len(mg["pool"]) == cfg.num_layers


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
def test_loss_over_more_than_256_row_blocks(backend, det):
    """B = 1, N = 65 824: 258 blocks of loss rows, the last one partial, so loss_final_kernel's combining block takes a second trip and loss_grad_kernel
    has rows beyond 65 536.  Loss, accuracy and logits under the forward test's bars; the gradients of fc's W and b, which are sums over loss_grad_kernel's
    rows times forward values (no leaky ReLU or pooling lies behind them, so no margin is asked: margins() is printed); then every row ignored.
    The forward values do not depend on the mode: the deterministic leg leaves the logits and the all-ignored call to the default leg (a call at this
    size takes seconds on the CPU logic build)."""
    case = "loss257"
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case(case)
    B, N = batch["labels"].shape
    pl = _on_its_branches(case, cfg, B)
    assert (pl.loss.blocks, pl.loss.trips, pl.loss.rows % 256) == (258, 2, 32)
    valid = ~np.isin(batch["labels"].reshape(-1), ign) & (batch["act"].reshape(-1) > 0)
    assert valid[65536:].sum() > 50 and valid[65792:].any(), "the rows beyond 65 536 and the partial block must carry loss"
    # a combining block that stops after its first trip loses the valid rows of blocks 256 and 257: fc's gradients (1 / valid rows) would be off by that
    # share, which must be far above their bar 8 u sqrt(2 n)
    counted = ~np.isin(batch["labels"].reshape(-1), ign)
    share = counted[65536:].sum() / counted.sum()
    assert share > 10 * 8 * U * np.sqrt(2.0 * N), "the rows behind the first 256 blocks do not show in the gradients"
    print("%s: %s" % (case, TC.describe_margins(TC.margins(r64, r32))))
    tr = _trainer(cfg, W, cw, ign, deterministic=det)
    dev, dm = TC.to_device(batch), _dev_mask(mask)
    _forward_and_loss(tr, case, dev, dm, moving=False, forward=not det)
    G = tr.grads()
    rows, bad, worst = TC.check_gradients(G, cfg, B, r64, r32, only={("fc", "W"), ("fc", "b")})
    print("\n".join(rows))
    assert len(rows) == 2 and not bad, "\n".join(bad)
    if det:
        return
    # every row ignored: status bit 0 and zeros
    gone = dict(batch, labels=np.zeros_like(batch["labels"]))
    tr.grads_arrays(TC.to_device(gone), mask=dm)
    assert tr.loss() == 0.0 and tr.accuracy() == 0.0
    assert tr.status() & 1 and tr.status() == 0
    assert all(np.isfinite(g).all() and not g.any() for g in tr.grads().values())


# ---- closing: every branch of the table is reached ---------------------------------------------------------------------------------------------------------
def test_every_tile_and_branch_is_reached():
    """the branches the parametrisations above reach, from plan alone: a gemm_kernel instantiation or a row of the table that no case reaches fails here.
    (The PART_FLOATS cap is not in the table: create() limits d_out to 512, so C <= 1024, the cap PART_FLOATS / 2C >= 1024 = the largest chunk count asked.)"""
    reached = {}
    def add(branches, who):
        for b in branches:
            reached.setdefault(b, []).append(who)
    for tile, (M, N, K) in GEMM_CASES:
        add(TP.launch_branches("forward", TP.gemm_plan(M, N, K)), "gemm piece %s" % ((M, N, K),))
    for cin, cout, M, tr_, _ in DW_CASES:
        add(TP.launch_branches("dW", TP.dw_plan(M, cin, cout)), "dW piece %s" % ((cin, cout, M),))
    for M, Cn, _ in REDUCE_CASES:
        for mode in range(3):
            add(TP.launch_branches("reduce%d" % mode, TP.reduce_plan(M, Cn)), "reduce piece %s" % ((M, Cn),))
    for case in E2E:
        cfg = TC.PATH_CASES[case][0]
        add(TP.plan(cfg, cfg.batch_size).branches, case)
    table = TP.branches()
    for b in table:
        print("%-62s %s" % (b, ", ".join(reached.get(b, [])[:6]) + (" ..." if len(reached.get(b, [])) > 6 else "")))
    missing = [b for b in table if b not in reached]
    assert not missing, "reached by no case: %s" % missing
    assert not set(reached) - set(table), "plan names a branch the table does not have: %s" % (set(reached) - set(table))
    k = TP.constants()
    assert 1024 <= k.PART_FLOATS // (2 * 1024), "the PART_FLOATS cap can bind at C = 1024: it needs a case"
