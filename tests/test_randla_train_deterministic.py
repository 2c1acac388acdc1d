"""Trainer(deterministic=True): the atomic-free backward scatters (csrc/scatter_det.hip, DESIGN section 21 "Deterministic mode").  Every test runs on
the CPU logic build and, marked gpu, on the gfx950 build (the ``backend`` fixture).

1. the two exported pieces against tests/_scatter_np.py, the NumPy float32 restatement of the fixed summation order: np.array_equal, bit for bit;
2. gradients in deterministic mode against float64: metric, bar and input conditions of tests/test_randla_train.py::test_gradients, restated here
   (per tensor max|g - g64| / max|g64| <= max(8 x the float32-torch metric, 8 u sqrt(2 n)), n = TC.reduction_rows);
3. the same bits every time: repeated calls, a second trainer on a caller's stream, three steps on two fresh trainers, a TrainFeeder batch;
4. the switch: on / off / on, new contents in the same buffers, the workspace's size, the refusals of the exported pieces.

Measured, deterministic mode, `worst tensor's metric (largest metric / bar)` per case — CPU logic build: s3dis 5.4e-06 (0.19), sem3d 7.0e-06 (0.22),
ties 4.7e-06 (0.18), five_b4 2.2e-05 (0.32); one MI355X: s3dis 7.1e-06 (0.23), sem3d 7.0e-06 (0.24), ties 6.0e-06 (0.21), five_b4 1.9e-05 (0.30)."""
import ctypes as C

import numpy as np
import pytest

import _scatter_np as S
import _train_cases as TC

U = 2.0 ** -24
MIN_VAR = 1e-3            # as tests/test_randla_train.py: below it 1 / sqrt(var + eps) multiplies every rounding of xhat by more than 30
SSDR_ERR_INVALID = 1      # include/ssdr_al.h
SORT_TILE = 2048          # RADIX_TILE (csrc/ssdr_internal.hpp): the pairs one workgroup of the list builder's radix sort stages at once;
                          # the reductions stage nothing (one work-item walks its row's list from memory)


def _bind():
    from ssdr_al import _lib
    L = _lib.lib()
    vp, i32 = C.c_void_p, C.c_int
    L.ssdr_scatter_add_rows_dev.argtypes = [vp, i32, i32, i32, vp, i32, i32, vp, i32, vp]
    L.ssdr_pool_grad_rows_dev.argtypes = [vp, vp, i32, i32, vp, i32, i32, i32, vp, vp, i32, vp]
    return L


def _dev(a):
    from ssdr_al._lib import DevArray
    return DevArray.from_host(np.ascontiguousarray(a))


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. the pieces, bit for bit ------------------------------------------------------------------------------------------------------------
def _rows_case(name):
    """(idx [B, rows_per_b], src_rows, C, ldo, o_col, lds, s_col) and the case's input condition, asserted here"""
    rng = np.random.default_rng([41, sum(map(ord, name))])
    if name == "single_hub":                         # every position lands in one list
        idx, src_rows, C = rng.integers(0, 1, (1, 37)), 1, 3
        assert np.bincount(S.row_keys(idx, src_rows), minlength=1).tolist() == [37]
        return idx, src_rows, C, C, 0, C, 0
    if name == "strided_view":                       # columns 5 .. 12 of an lds = 24 buffer, dout in columns 2 .. 9 of an ldo = 11 buffer
        return rng.integers(0, 40, (3, 160)), 40, 8, 11, 2, 24, 5
    if name == "unreferenced_rows":                  # even rows only
        idx, src_rows = 2 * rng.integers(0, 25, (2, 300)), 50
        assert not (S.row_keys(idx, src_rows) % 2).any()
        return idx, src_rows, 6, 6, 0, 6, 0
    if name == "out_of_range":                       # -1 and src_rows + 5 among the indices: clamped to the first and the last row
        idx, src_rows = rng.integers(0, 30, (2, 90)), 30
        idx[:, ::7] = -1; idx[:, 3::11] = src_rows + 5
        assert (idx < 0).any() and (idx >= src_rows).any()
        return idx, src_rows, 4, 4, 0, 4, 0
    if name == "interp_k1":                          # nearest_interpolation's shape: 512 positions per tile (K = 1) into 128 rows
        return rng.integers(0, 128, (2, 512)), 128, 32, 64, 0, 64, 32
    if name == "wide_and_short":
        return rng.integers(0, 8, (1, 128)), 8, 1024, 1024, 0, 1024, 0
    if name == "skewed":                             # 9 600 positions on 600 rows, half of them on three rows
        idx = rng.integers(0, 600, (1, 9600))
        heavy = rng.permutation(9600)[:4800]
        idx[0, heavy[:2600]] = 17; idx[0, heavy[2600:4000]] = 311; idx[0, heavy[4000:]] = 599
        counts = np.bincount(S.row_keys(idx, 600), minlength=600)
        assert counts[[17, 311, 599]].sum() >= 4800 and counts.max() > SORT_TILE, "the longest list must exceed one sort tile"
        return idx, 600, 5, 5, 0, 5, 0
    raise KeyError(name)


@pytest.mark.parametrize("name", ["single_hub", "strided_view", "unreferenced_rows", "out_of_range", "interp_k1", "wide_and_short", "skewed"])
def test_scatter_add_rows_piece(backend, name):
    from ssdr_al import _lib
    L = _bind()
    idx, src_rows, Cn, ldo, o_col, lds, s_col = _rows_case(name)
    idx = np.ascontiguousarray(idx, np.int32)
    B, rows_per_b = idx.shape
    rng = np.random.default_rng(7)
    dout = rng.normal(0, 1, (B * rows_per_b, ldo)).astype(np.float32) * (10.0 ** rng.integers(-3, 3, (B * rows_per_b, 1))).astype(np.float32)
    dsrc = rng.normal(0, 1, (B * src_rows, lds)).astype(np.float32)
    dsrc[::3, s_col] = -0.0                           # a row that is not written keeps even the sign of a zero
    d_idx, d_dout, d_dsrc = _dev(idx), _dev(dout), _dev(dsrc)
    _lib.check(L.ssdr_scatter_add_rows_dev(d_idx.ptr, B, rows_per_b, src_rows, d_dout.ptr + 4 * o_col, ldo, Cn, d_dsrc.ptr + 4 * s_col, lds, None))
    _lib.sync()
    got = d_dsrc.to_host()
    want = dsrc.copy()
    want[:, s_col:s_col + Cn] = S.scatter_add_rows(idx, src_rows, dout[:, o_col:o_col + Cn], dsrc[:, s_col:s_col + Cn])
    assert not _bits_equal(want, dsrc)
    assert _bits_equal(got, want), "%d elements differ" % int((got.view(np.uint32) != want.view(np.uint32)).sum())
    if name == "strided_view":                        # (covered by the comparison above; spelled out because the issue names it)
        keep = np.ones(lds, bool); keep[s_col:s_col + Cn] = False
        assert _bits_equal(got[:, keep], dsrc[:, keep])
    if name == "unreferenced_rows":
        assert _bits_equal(got[1::2], dsrc[1::2]) and not _bits_equal(got[0::2], dsrc[0::2])


def _pool_case(name):
    """(src [B src_rows, C], idx [B, m_per_b, 16], src_rows) with the case's input condition asserted"""
    rng = np.random.default_rng([43, sum(map(ord, name))])
    if name == "copies":                              # rows 32 + m are exact copies of the rows m that win point m: two tied rows per (m, c)
        B, src_rows, m_per_b, Cn = 1, 64, 20, 5
        src = rng.random((src_rows, Cn), dtype=np.float32)
        src[:20] += 2.0
        src[32:52] = src[:20]
        idx = rng.integers(20, 32, (B, m_per_b, 16))
        idx[0, :, 0] = np.arange(20); idx[0, :, 9] = 32 + np.arange(20)
        ties = S.pool_ties(src, idx, src_rows, S.pool_forward(src, idx, src_rows))[1]
        assert (ties == 2).all(), "every (point, channel) must have exactly two tied rows"
    elif name == "same_maximum":                      # two different rows share the maximum of ONE channel
        B, src_rows, m_per_b, Cn = 1, 40, 12, 6
        src = rng.random((src_rows, Cn), dtype=np.float32)
        src[3, 2] = src[29, 2] = 5.0
        idx = np.stack([rng.permutation(np.r_[4:29])[:16] for _ in range(m_per_b)])[None]
        idx[0, :, 1] = 3; idx[0, :, 14] = 29
        ties = S.pool_ties(src, idx, src_rows, S.pool_forward(src, idx, src_rows))[1]
        assert (ties[:, 2] == 2).all() and (np.delete(ties, 2, axis=1) == 1).all()
    elif name == "repeated_index":                    # the winning row twice among a point's 16: counted twice, and its row adds the share twice
        B, src_rows, m_per_b, Cn = 1, 48, 10, 4
        src = rng.random((src_rows, Cn), dtype=np.float32)
        src[40:] += 3.0
        idx = np.stack([rng.permutation(40)[:16] for _ in range(m_per_b)])[None]
        idx[0, :, 3] = 40 + np.arange(m_per_b) % 8; idx[0, :, 7] = idx[0, :, 3]
        ties = S.pool_ties(src, idx, src_rows, S.pool_forward(src, idx, src_rows))[1]
        assert (ties == 2).all() and all(len(set(r)) == 15 for r in idx[0].tolist())
    elif name == "unpooled_rows":                     # nothing pools from the odd rows
        B, src_rows, m_per_b, Cn = 1, 60, 15, 7
        src = rng.random((src_rows, Cn), dtype=np.float32)
        idx = 2 * rng.integers(0, 30, (B, m_per_b, 16))
        assert not (S.row_keys(idx, src_rows) % 2).any()
    elif name == "two_tiles":                         # the second batch element's rows start at src_rows, its points at m_per_b
        B, src_rows, m_per_b, Cn = 2, 33, 9, 5
        src = rng.random((B * src_rows, Cn), dtype=np.float32)
        idx = rng.integers(-2, src_rows + 2, (B, m_per_b, 16))
        assert not np.array_equal(idx[0], idx[1]) and (idx < 0).any() and (idx >= src_rows).any()
    else:
        raise KeyError(name)
    return src, np.ascontiguousarray(idx, np.int32), src_rows


@pytest.mark.parametrize("name", ["copies", "same_maximum", "repeated_index", "unpooled_rows", "two_tiles"])
def test_pool_grad_rows_piece(backend, name):
    from ssdr_al import _lib
    L = _bind()
    src, idx, src_rows = _pool_case(name)
    B, m_per_b, Cn = idx.shape[0], idx.shape[1], src.shape[1]
    lds, s_col, ldo, o_col = (Cn + 3, 2, Cn + 2, 1) if name == "two_tiles" else (Cn, 0, Cn, 0)         # views with leading dimensions once
    rng = np.random.default_rng(11)
    src_buf = rng.random((B * src_rows, lds), dtype=np.float32); src_buf[:, s_col:s_col + Cn] = src
    dsrc_buf = rng.normal(0, 1, (B * src_rows, lds)).astype(np.float32); dsrc_buf[::3, s_col] = -0.0
    out = S.pool_forward(src, idx, src_rows)
    out_buf = rng.random((B * m_per_b, ldo), dtype=np.float32); out_buf[:, o_col:o_col + Cn] = out
    dout_buf = rng.normal(0, 1, (B * m_per_b, ldo)).astype(np.float32)
    d_src, d_dsrc, d_idx, d_out, d_dout = _dev(src_buf), _dev(dsrc_buf), _dev(idx), _dev(out_buf), _dev(dout_buf)
    _lib.check(L.ssdr_pool_grad_rows_dev(d_src.ptr + 4 * s_col, d_dsrc.ptr + 4 * s_col, lds, src_rows, d_idx.ptr, B, m_per_b, Cn, d_out.ptr + 4 * o_col,
                                         d_dout.ptr + 4 * o_col, ldo, None))
    _lib.sync()
    got = d_dsrc.to_host()
    want = dsrc_buf.copy()
    want[:, s_col:s_col + Cn] = S.pool_grad_rows(src, idx, src_rows, out, dout_buf[:, o_col:o_col + Cn], dsrc_buf[:, s_col:s_col + Cn])
    assert not _bits_equal(want, dsrc_buf)
    assert _bits_equal(got, want), "%d elements differ" % int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert _bits_equal(d_src.to_host(), src_buf)
    if name == "unpooled_rows":
        assert _bits_equal(got[1::2], dsrc_buf[1::2])
    if name == "repeated_index":                      # the whole gradient arrives: the two shares of a point land in the same row
        total = (got - dsrc_buf).sum(0)
        assert np.abs(total - dout_buf.sum(0)).max() < 1e-4


# ---- 2. gradients against float64 ---------------------------------------------------------------------------------------------------------------
def _trainer(cfg, W, cw=None, ign=(), **kw):
    from ssdr_al.trainer import Trainer
    return Trainer(cfg, class_weights=cw, ignored_labels=ign, **kw).load(W)


def _dev_mask(mask):
    return _dev(np.ascontiguousarray(mask, np.uint8).reshape(-1))


def _conditions(case):
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case(case)
    signs, ties, min_var = TC.conditions(r64, r32)
    assert signs and ties, "the float32 and float64 oracle runs disagree on a sign or an arg-max set: pick another seed"
    assert min_var >= MIN_VAR, "a degenerate batch norm (variance %.3g)" % min_var
    if case == "ties":
        assert int((r64["ties"][0].sum(2) > 1).sum()) > 0, "no tied maximum at level 0"
    if case == "five_b4":                             # the edges of the lists, from the batch itself
        neigh, pool0, pool4 = batch["neigh"][4], batch["pool"][0], batch["pool"][4]
        n4 = neigh.shape[1]
        assert np.bincount(S.row_keys(neigh.reshape(neigh.shape[0], -1), n4)).max() == 72, "the deepest level's longest list"
        assert sum(len(set(r)) < 16 for r in neigh.reshape(-1, 16).tolist()) == 32, "points with a repeated neighbour"
        assert sum(len(set(r)) < 16 for r in pool4.reshape(-1, 16).tolist()) == 16, "pooled rows with a repeated index"
        n0 = batch["neigh"][0].shape[1]
        hit = np.bincount(S.row_keys(pool0.reshape(pool0.shape[0], -1), n0), minlength=pool0.shape[0] * n0)
        assert int((hit == 0).sum()) == 115, "source rows pool[0] does not reference"


def _check_gradients(G, case, what):
    """the bars of test_randla_train.py::test_gradients on a grads() dict; returns the worst (metric, metric / bar)"""
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case(case)
    B = batch["labels"].shape[0]
    bad, rows, worst, worst_ratio = [], [], 0.0, 0.0
    for (name, key), g in G.items():
        g64, g32 = r64["grads"][(name, key)], r32["grads"][(name, key)]
        assert g.shape == g64.shape and np.isfinite(g).all(), (name, key)
        scale = np.abs(g64).max()
        if key == "b" and (name, "gamma") in r64["grads"]:
            scale = np.abs(r64["grads"][(name, "W")]).max()
        m_dev, m_32 = np.abs(g - g64).max() / scale, np.abs(g32 - g64).max() / scale
        bar = max(8 * m_32, 8 * U * np.sqrt(2.0 * TC.reduction_rows(cfg, B, name)))
        rows.append("%-36s %-5s device %.2e float32-torch %.2e bar %.2e" % (name, key, m_dev, m_32, bar))
        worst, worst_ratio = max(worst, m_dev), max(worst_ratio, m_dev / bar)
        if not m_dev <= bar:
            bad.append(rows[-1])
    print("%s %s: %d tensors, worst metric %.2e, largest metric / bar %.2f" % (what, case, len(G), worst, worst_ratio))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", ["s3dis", "sem3d", "ties", "five_b4"])
def test_gradients_deterministic(backend, case):
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case(case)
    _conditions(case)
    tr = _trainer(cfg, W, cw, ign, deterministic=True)
    assert tr.deterministic
    tr.grads_arrays(TC.to_device(batch), mask=_dev_mask(mask))
    _check_gradients(tr.grads(), case, "deterministic")
    assert tr.step_count() == 0 and tr.status() == 0


# ---- 3. the same bits every time ------------------------------------------------------------------------------------------------------------------
def _same(A, B):
    return [k for k in A if not _bits_equal(A[k], B[k])]


def _full_state(tr):
    """weights, the moving statistics and Adam's moments, flat"""
    st, out = tr.state(), {}
    for name, ent in st["weights"].items():
        out[(name, "W")] = ent["W"]
        if ent["b"] is not None:
            out[(name, "b")] = ent["b"]
        if ent["bn"] is not None:
            for k, a in zip(("gamma", "beta", "mean", "var"), ent["bn"]):
                out[(name, k)] = a
    for key, (m, v) in st["adam"].items():
        out[key + ("m",)], out[key + ("v",)] = m, v
    return out


def test_repeated_calls_and_streams_give_the_same_bits(backend):
    from ssdr_al import _lib
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case("ties")
    dev, dm = TC.to_device(batch), _dev_mask(mask)
    tr = _trainer(cfg, W, cw, ign, deterministic=True)
    runs = []
    for _ in range(3):
        tr.grads_arrays(dev, mask=dm)
        runs.append(tr.grads())
    assert any(g.any() for g in runs[0].values())
    assert not _same(runs[0], runs[1]) and not _same(runs[0], runs[2])
    L = _lib.lib()
    s1 = C.c_void_p()
    _lib.check(L.ssdr_stream_create(C.byref(s1)))
    other = _trainer(cfg, W, cw, ign, deterministic=True)
    other.grads_arrays(dev, stream=s1.value, mask=dm)
    _lib.sync(s1.value)
    assert not _same(runs[0], other.grads())
    L.ssdr_stream_destroy(s1.value)


def test_three_steps_on_two_trainers_give_the_same_state(backend):
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case("s3dis")
    dev = TC.to_device(batch)
    masks = [_dev_mask(TC.make_mask(batch, 100 + t)) for t in range(3)]
    states = []
    for _ in range(2):
        tr = _trainer(cfg, W, cw, ign, deterministic=True)
        for t in range(3):
            tr.step_arrays(dev, mask=masks[t])
        assert tr.step_count() == 3 and np.isfinite(tr.loss()) and tr.status() == 0
        states.append(_full_state(tr))
    moved = [k for k in states[0] if k[-1] == "W" and not np.array_equal(states[0][k], np.asarray(W[k[0]]["W"], np.float32))]
    assert len(moved) > 10, "the steps must have moved the weights"
    assert not _same(states[0], states[1])


def _feeder(seed=2):
    from ssdr_al import training
    from ssdr_al.helper_tool import ConfigS3DIS

    class Small(ConfigS3DIS):
        num_points = 512
        num_layers = 3
        sub_sampling_ratio = [4, 4, 2]
        d_out = [16, 64, 128]
        batch_size = 2
        train_steps = 2
        num_classes = 13
    rng = np.random.default_rng(seed)
    clouds, pg = [], []
    for n in (300, 800, 1300):
        lab = rng.integers(0, 13, n).astype(np.int32)
        clouds.append(dict(xyz=(rng.random((n, 3)) * [4, 4, 2]).astype(np.float32), rgb=rng.random((n, 3)).astype(np.float32), labels=lab))
        pg.append(np.stack([(rng.random(n) < 0.5).astype(np.float32), lab.astype(np.float32)]))
    return training.TrainFeeder(clouds, pg, config=Small, dataset="S3DIS", seed=seed), Small


def test_step_on_a_feeder_batch_gives_the_same_state(backend):
    """Trainer.step(batch) on a TrainFeeder batch and step_arrays on a copy of it, two steps each (the generated dropout masks of one seed):
    identical weights, moments and moving statistics"""
    from ssdr_al._lib import DevArray
    feeder, cfg = _feeder()
    W = TC.weights_for(cfg, 6)
    a, b = _trainer(cfg, W, seed=3, deterministic=True), _trainer(cfg, W, seed=3, deterministic=True)
    for _ in range(2):
        batch = feeder.next_batch(None)
        host = batch.to_host()
        a.step(batch)
        assert batch.released
        b.step_arrays([DevArray.from_host(h) for h in host])
    assert a.status() == 0 and np.isfinite(a.loss()) and a.step_count() == 2
    sa, sb = _full_state(a), _full_state(b)
    assert not np.array_equal(sa[("fc", "W")], np.asarray(W["fc"]["W"], np.float32))
    assert not _same(sa, sb)
    feeder.close()


# ---- 4. the switch ------------------------------------------------------------------------------------------------------------------------------
def test_switching_the_mode(backend):
    """on -> off -> on on one trainer: every call meets the bars, and the mode's bits do not depend on what ran before (no stale list, no stale plan);
    the same device buffers refilled with another batch: the lists follow the contents, not the pointers"""
    from ssdr_al import _lib
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case("s3dis")
    _conditions("s3dis")
    _conditions("ties")
    dev, dm = TC.to_device(batch), _dev_mask(mask)
    tr = _trainer(cfg, W, cw, ign)
    assert not tr.deterministic and tr.workspace_bytes() == 0
    tr.grads_arrays(dev, mask=dm)                                    # off (the default): the bars hold as before
    _check_gradients(tr.grads(), "s3dis", "off")
    ws_off = tr.workspace_bytes()
    tr.set_deterministic(True)
    ws_on = tr.workspace_bytes()                                     # known before the first deterministic call
    assert tr.deterministic and ws_on > ws_off > 0
    tr.grads_arrays(dev, mask=dm)
    on1 = tr.grads()
    _check_gradients(on1, "s3dis", "on after off")
    assert tr.workspace_bytes() == ws_on
    tr.set_deterministic(False)
    assert not tr.deterministic and tr.workspace_bytes() == ws_off
    tr.grads_arrays(dev, mask=dm)
    _check_gradients(tr.grads(), "s3dis", "off after on")
    tr.set_deterministic(True)
    tr.grads_arrays(dev, mask=dm)
    assert not _same(on1, tr.grads())
    fresh = _trainer(cfg, W, cw, ign, deterministic=True)
    fresh.grads_arrays(dev, mask=dm)
    assert not _same(on1, fresh.grads())
    # the 'ties' batch has the same shapes: copy it into the SAME device buffers
    cfg2, W2, batch2, mask2, cw2, ign2, _, _ = TC.oracle_case("ties")
    L = _lib.lib()
    for d, h in zip(dev, TC.input_list(batch2)):
        h = np.ascontiguousarray(h)
        assert h.shape == d.shape and h.dtype == d.dtype
        _lib.check(L.ssdr_memcpy_h2d(d.ptr, _lib.ptr(h), d.nbytes))
    tr.load(W2)
    tr.grads_arrays(dev, mask=_dev_mask(mask2))
    _check_gradients(tr.grads(), "ties", "refilled buffers")


def test_pieces_refuse_bad_arguments(backend):
    from ssdr_al import _lib
    L = _bind()
    idx = _dev(np.zeros((2, 8), np.int32))
    a, b = _dev(np.ones((16, 4), np.float32)), _dev(np.ones((6, 4), np.float32))
    ok = [idx.ptr, 2, 8, 3, a.ptr, 4, 4, b.ptr, 4, None]
    before = b.to_host()
    for hole, val in ((0, None), (4, None), (7, None), (6, 0), (6, -1), (5, 3), (8, 3)):
        bad = list(ok); bad[hole] = val
        assert L.ssdr_scatter_add_rows_dev(*bad) == SSDR_ERR_INVALID and L.ssdr_last_error(), (hole, val)
    empty = list(ok); empty[1] = 0
    assert L.ssdr_scatter_add_rows_dev(*empty) == 0
    empty = list(ok); empty[2] = 0
    assert L.ssdr_scatter_add_rows_dev(*empty) == 0
    _lib.sync()
    assert np.array_equal(b.to_host(), before)                       # nothing was launched
    pidx = _dev(np.zeros((1, 2, 16), np.int32))
    src, dsrc, out, dout = (_dev(np.ones((n, 4), np.float32)) for n in (5, 5, 2, 2))
    okp = [src.ptr, dsrc.ptr, 4, 5, pidx.ptr, 1, 2, 4, out.ptr, dout.ptr, 4, None]
    for hole, val in ((0, None), (1, None), (4, None), (8, None), (9, None), (7, 0), (2, 3), (10, 3)):
        bad = list(okp); bad[hole] = val
        assert L.ssdr_pool_grad_rows_dev(*bad) == SSDR_ERR_INVALID and L.ssdr_last_error(), (hole, val)
    empty = list(okp); empty[6] = 0
    assert L.ssdr_pool_grad_rows_dev(*empty) == 0
    assert L.ssdr_pool_grad_rows_dev(*okp) == 0 and L.ssdr_scatter_add_rows_dev(*ok) == 0
    _lib.sync()
    assert np.array_equal(b.to_host()[:, 0], [9, 1, 1, 9, 1, 1])      # 8 ones into row 0 of either tile: the valid calls run
