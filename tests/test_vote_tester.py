"""Test-time voting evaluation on the device (ssdr_vote_init_dev / ssdr_vote_tiles_dev, ssdr_al.evaluate.VoteTester) against the NumPy
restatement of the reference's loop (tests/_vote_oracle.py: S3/s3dis_dataset_test.py:85-151, S3/RandLANet.py:290-424).

Shapes: num_points 1024 over clouds of 300 (padded: every row taken), 1024, 1029, 2117 and 5000 points; the initial map random * 1e-3 with two
equal cloud minima and two equal minima inside cloud 0, so the first arg-min rules decide from the first tile on.  The noise comes from the
stream that made the clouds, tile after tile, which fixes the visit order the cases below rely on (asserted from the restatement before
anything is compared).  Every comparison is index for index and bit for bit; IoUs at the 1e-12 relative bar of tests/test_evaluate.py."""
import ctypes as C

import numpy as np
import pytest

import _vote_oracle as VO
from conftest import assert_bits_equal

SIZES = [300, 1024, 1029, 2117, 5000]
N = 1024
SSDR_ERR_INVALID, SSDR_ERR_UNSUPPORTED = 1, 5


def _cfg(batch, steps):
    from ssdr_al.helper_tool import ConfigS3DIS

    class Small(ConfigS3DIS):
        num_points = N
        num_layers = 2
        d_out = [16, 64]
        sub_sampling_ratio = [4, 4]
        num_classes = 13
        val_batch_size = batch
        val_steps = steps
        noise_init = 3.5
    return Small


@pytest.fixture(scope="module")
def weights_small():
    from oracle import randla_np as R
    return R.init_weights(0, d_out=(16, 64))


class _Chain:
    """the generator's state on the device and one call of the chain through the C ABI"""

    def __init__(self, clouds, poss, num_points, labels=True):
        from ssdr_al import _lib
        from ssdr_al._lib import DevArray
        _lib.check(_lib.lib().ssdr_init(0))
        self.N, self.nc = num_points, len(clouds)
        self.off = np.concatenate([[0], np.cumsum([len(c["xyz"]) for c in clouds])]).astype(np.int64)
        self.d_p = DevArray.from_host(np.concatenate([c["xyz"] for c in clouds]))
        self.d_c = DevArray.from_host(np.concatenate([c["rgb"] for c in clouds]).astype(np.float32))
        self.d_l = DevArray.from_host(np.concatenate([c["labels"] for c in clouds])) if labels else None
        self.d_poss = DevArray.from_host(np.concatenate(poss))
        self.d_min, self.d_arg = DevArray((self.nc,), np.float64), DevArray((self.nc,), np.int32)
        _lib.check(_lib.lib().ssdr_vote_init_dev(self.d_poss.ptr, _lib.ptr(self.off), self.nc, self.d_min.ptr, self.d_arg.ptr, None))

    def tiles(self, draws):
        from ssdr_al import _lib
        from ssdr_al._lib import DevArray
        B, N = len(draws["noise"]), self.N
        d_n, d_perm, d_dup = DevArray.from_host(draws["noise"]), DevArray.from_host(draws["perm"]), DevArray.from_host(draws["dup"])
        o = dict(xyz=DevArray((B, N, 3), np.float32), feat=DevArray((B, N, 6), np.float32), idx=DevArray((B, N), np.int32),
                 labels=DevArray((B, N), np.int32), cloud=DevArray((B,), np.int32), center=DevArray((B, 3), np.float32))
        _lib.check(_lib.lib().ssdr_vote_tiles_dev(self.d_p.ptr, self.d_c.ptr, 3, self.d_l.ptr if self.d_l else None, self.d_poss.ptr, self.d_min.ptr, self.d_arg.ptr,
                                                  _lib.ptr(self.off), self.nc, B, N, d_n.ptr, d_perm.ptr, d_dup.ptr, 1.0 / 255.0, o["xyz"].ptr, o["feat"].ptr,
                                                  o["idx"].ptr, o["labels"].ptr if self.d_l else None, o["cloud"].ptr, o["center"].ptr, None))
        _lib.sync()
        return {k: v.to_host() for k, v in o.items()}

    def state(self):
        return self.d_poss.to_host(), self.d_min.to_host(), self.d_arg.to_host()


def _compare_batch(got, ref, what):
    assert np.array_equal(got["cloud"], ref["cloud"]), what + " cloud ids"
    assert_bits_equal(got["center"], ref["center"], what + " centres")
    assert np.array_equal(got["idx"], ref["idx"]), what + " global rows"
    assert_bits_equal(got["xyz"], ref["xyz"], what + " xyz")
    assert_bits_equal(got["feat"], ref["feat"], what + " features")
    assert np.array_equal(got["labels"], ref["labels"]), what + " labels"


def _compare_state(state, gen, what):
    poss, cmin, carg = state
    assert np.array_equal(poss, np.concatenate(gen.possibility)), what + " possibility map (float64, bit for bit)"
    assert np.array_equal(cmin, np.asarray(gen.min_possibility)), what + " cloud minima"
    assert np.array_equal(carg, gen.cloud_arg()), what + " cloud arg-minima (first minimum)"


@pytest.fixture(scope="module")
def chain_reference():
    """Case 1's restatement, computed once: three batches of 20 tiles; (clouds, initial map, draws, per batch: tiles and the state after it)"""
    clouds, poss, rng = VO.make_case(SIZES)
    poss = VO.add_ties(poss)
    rng_perm = np.random.default_rng(99)
    gen = VO.Generator(clouds, poss, N)
    draws, batches, states = [], [], []
    for _ in range(3):
        d = VO.draw_batch(rng, rng_perm, 20, N)
        draws.append(d); batches.append(gen.batch(d))
        states.append((np.concatenate(gen.possibility).copy(), np.asarray(gen.min_possibility).copy(), gen.cloud_arg()))
    return clouds, poss, draws, batches, states


def test_chain_matches_restatement(backend, chain_reference):
    clouds, poss, draws, batches, states = chain_reference
    # what the restatement alone says about these 60 tiles: the paths they take
    order = np.concatenate([b["cloud"] for b in batches])
    assert order[:6].tolist() == [0, 2, 4, 3, 4, 1]                     # ties between clouds 0 and 2, and inside cloud 0: first minimum
    assert set(order.tolist()) == set(range(5))
    assert ((order[1:] == 4) & (order[:-1] == 4)).any()                 # a cloud visited in consecutive tiles: tile t + 1 reads tile t's minimum
    assert (order == 0).sum() == 4                                      # the 300-point cloud: padding path, every row taken
    assert abs(states[-1][1].min() - 0.81) < 0.01                       # every point covered: the regime after full coverage
    ch = _Chain(clouds, poss, N)
    p0, m0, a0 = ch.state()
    assert np.array_equal(m0, [p.min() for p in poss]) and np.array_equal(a0, [int(np.argmin(p)) for p in poss])      # init_possibility; cloud 0: row 5, not 9
    assert a0[0] == 5 and a0[2] == 17
    for k in range(3):
        _compare_batch(ch.tiles(draws[k]), batches[k], "batch %d" % k)
        poss_k, min_k, arg_k = states[k]
        got = ch.state()
        assert np.array_equal(got[0], poss_k), "batch %d possibility map (float64, bit for bit)" % k
        assert np.array_equal(got[1], min_k) and np.array_equal(got[2], arg_k), "batch %d cloud minima" % k


def test_chain_equals_the_per_tile_loop(backend, chain_reference):
    """the loop a caller had before: ssdr_tile_select_possibility_dev per tile, its minimum and arg-min read back, the next centre formed on the host"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    clouds, poss, draws, _, _ = chain_reference
    ch = _Chain(clouds, poss, N)
    got = [ch.tiles(d) for d in draws]
    got_state = ch.state()
    off = ch.off
    d_p, d_c = DevArray.from_host(np.concatenate([c["xyz"] for c in clouds])), DevArray.from_host(np.concatenate([c["rgb"] for c in clouds]).astype(np.float32))
    d_poss = DevArray.from_host(np.concatenate(poss))
    d_m = [DevArray.from_host(np.array([len(c["xyz"]), 0], np.int64)) for c in clouds]
    mins = [float(p.min()) for p in poss]; args = [int(np.argmin(p)) for p in poss]
    d_xyz, d_feat, d_idx = DevArray((N, 3), np.float32), DevArray((N, 6), np.float32), DevArray((N,), np.int32)
    d_min, d_arg = DevArray((1,), np.float64), DevArray((1,), np.int32)
    for k, d in enumerate(draws):
        d_perm, d_dup = DevArray.from_host(d["perm"]), DevArray.from_host(d["dup"])
        for t in range(len(d["noise"])):
            c = int(np.argmin(np.asarray(mins)))
            pick = (clouds[c]["xyz"][args[c]] + d["noise"][t]).astype(np.float32)
            o = int(off[c])
            _lib.check(_lib.lib().ssdr_tile_select_possibility_dev(d_p.ptr + 12 * o, d_c.ptr + 12 * o, 3, d_m[c].ptr, len(clouds[c]["xyz"]), _lib.ptr(pick), N,
                                                                  d_perm.ptr + 4 * t * N, d_dup.ptr + 4 * t * N, 1.0 / 255.0, d_xyz.ptr, d_feat.ptr, d_idx.ptr,
                                                                  d_poss.ptr + 8 * o, d_min.ptr, d_arg.ptr, None))
            _lib.sync()
            mins[c], args[c] = float(d_min.to_host()[0]), int(d_arg.to_host()[0])
            what = "batch %d tile %d" % (k, t)
            assert got[k]["cloud"][t] == c, what
            assert_bits_equal(got[k]["center"][t], pick, what + " centre")
            assert np.array_equal(got[k]["idx"][t], o + d_idx.to_host()), what + " rows"
            assert_bits_equal(got[k]["xyz"][t], d_xyz.to_host(), what + " xyz")
            assert_bits_equal(got[k]["feat"][t], d_feat.to_host(), what + " features")
    assert np.array_equal(got_state[0], d_poss.to_host())
    assert np.array_equal(got_state[1], mins) and np.array_equal(got_state[2], args)


def _tester(weights, batch, steps, **kw):
    from ssdr_al import evaluate
    clouds, poss, rng = VO.make_case(SIZES)
    poss = VO.add_ties(poss)
    return evaluate.VoteTester(weights, clouds, config=_cfg(batch, steps), possibility=poss, **kw), clouds, poss, rng


def test_votes_tile_by_tile(backend, weights_small):
    """test_probs after two batches = RandLANet.py:334 applied tile by tile to the device's own network outputs"""
    t, clouds, poss, rng = _tester(weights_small, 8, 1)
    rng_perm = np.random.default_rng(99)
    gen = VO.Generator(clouds, poss, N)
    ref = np.zeros((sum(SIZES), 13), np.float32)
    twice = 0
    for k in range(2):
        d = VO.draw_batch(rng, rng_perm, 8, N)
        out = t.run_batch(d)
        exp = gen.batch(d)
        assert np.array_equal(out["idx"].to_host(), exp["idx"]) and np.array_equal(out["cloud"].to_host(), exp["cloud"])
        probs = out["probs"].to_host()
        assert probs.shape == (8 * N, 13) and np.isfinite(probs).all()
        VO.vote(ref, exp["idx"], probs)
        tiles_of = np.zeros(sum(SIZES), np.int32)
        for j in range(8):
            tiles_of[np.unique(exp["idx"][j])] += 1
        twice += int((tiles_of >= 2).sum())
    assert twice > 0                                                   # points in two tiles of one batch: smoothed twice
    assert_bits_equal(t.probs_host(), ref, "test_probs")
    assert t.tiles == 16
    t.close()


def test_evaluate_end_to_end(backend, weights_small):
    t, clouds, poss, rng = _tester(weights_small, 8, 1)
    rng_perm = np.random.default_rng(99)
    all_draws = [VO.draw_batch(rng, rng_perm, 8, N) for _ in range(8)]
    draws = lambda epoch, step: all_draws[epoch]
    # the restatement of the loop (:305-424); the network's outputs come from a second tester that runs the same batches one by one
    t2, _, _, _ = _tester(weights_small, 8, 1)
    gen = VO.Generator(clouds, poss, N)
    ref = np.zeros((sum(SIZES), 13), np.float32)
    last_min, epochs, hist, stopped = -0.5, 0, [], False
    while last_min < 100 and epochs < 8:
        exp = gen.batch(all_draws[epochs])
        out = t2.run_batch(all_draws[epochs])
        assert np.array_equal(out["idx"].to_host(), exp["idx"])
        VO.vote(ref, exp["idx"], out["probs"].to_host())
        epochs += 1
        new_min = np.min(gen.min_possibility)                           # :339
        hist.append(float(new_min))
        if last_min + 1 < new_min:                                      # :342
            stopped = True
            break
    assert stopped and epochs == 7                                      # what the restatement alone gives: minima 1.4e-6 ... 0.49, 0.655
    assert abs(hist[0] - 1.3946853358485223e-06) < 1e-12 and abs(hist[-2] - 0.4923) < 1e-3 and abs(hist[-1] - 0.6551) < 1e-3
    m = VO.final_metrics(clouds, ref, gen.off, 13)
    m_iou, oa = t.evaluate(draws=draws)
    assert t.epochs == 7 and t.tiles == 56
    assert t.min_history == hist
    assert_bits_equal(t.probs_host(), ref, "test_probs")
    assert np.array_equal(t.sub_confusion, m["sub_confusion"]) and np.array_equal(t.confusion, m["confusion"])
    assert oa == m["oa"]
    assert np.allclose(t.ious, m["ious"], rtol=1e-12, atol=0) and np.allclose(t.sub_ious, m["sub_ious"], rtol=1e-12, atol=0)
    assert np.isclose(m_iou, m["m_iou"], rtol=1e-12, atol=0)
    preds = t.predictions()
    for c, cl in enumerate(clouds):
        assert np.array_equal(preds[c], np.argmax(ref[gen.off[c]:gen.off[c + 1]][cl["proj_idx"]], axis=1))
    # without proj_idx the full cloud is the sub-cloud
    sub_only = [dict(xyz=c["xyz"], rgb=c["rgb"], labels=c["labels"]) for c in clouds]
    from ssdr_al import evaluate
    t3 = evaluate.VoteTester(weights_small, sub_only, config=_cfg(8, 1), possibility=poss)
    m_iou3, oa3 = t3.evaluate(draws=draws)
    m3 = VO.final_metrics([dict(c, proj_idx=np.arange(len(c["xyz"])), raw_labels=c["labels"]) for c in sub_only], ref, gen.off, 13)
    assert t3.epochs == 7 and np.array_equal(t3.confusion, m3["confusion"]) and np.array_equal(t3.confusion, t3.sub_confusion)
    assert oa3 == m3["oa"] and np.isclose(m_iou3, m3["m_iou"], rtol=1e-12, atol=0) and np.allclose(t3.sub_ious, m3["sub_ious"], rtol=1e-12, atol=0)
    # max_epochs: whole epochs, and the reference's 0, 0 when the loop is cut short
    t4, _, _, _ = _tester(weights_small, 8, 1)
    assert t4.evaluate(max_epochs=2, draws=draws) == (0, 0)
    assert t4.epochs == 2 and t4.tiles == 16 and t4.min_history == hist[:2]
    for x in (t, t2, t3, t4):
        x.close()


def test_refusals(backend, weights_small):
    from ssdr_al import _lib, evaluate
    from ssdr_al._lib import DevArray
    L = _lib.lib()
    _lib.check(L.ssdr_init(0))
    clouds, poss, rng = VO.make_case([300, 1024])
    ch = _Chain(clouds, poss, N)
    before = ch.state()
    B = 2
    d = VO.draw_batch(rng, np.random.default_rng(1), B, N)
    d_n, d_perm, d_dup = DevArray.from_host(d["noise"]), DevArray.from_host(d["perm"]), DevArray.from_host(d["dup"])
    o = dict(xyz=DevArray((B, N, 3), np.float32), feat=DevArray((B, N, 6), np.float32), idx=DevArray((B, N), np.int32),
             labels=DevArray((B, N), np.int32), cloud=DevArray((B,), np.int32), center=DevArray((B, 3), np.float32))

    def call(off, nc, tiles=B, points=N, labels=True, out_labels=True):
        off = np.ascontiguousarray(off, np.int64)
        return L.ssdr_vote_tiles_dev(ch.d_p.ptr, ch.d_c.ptr, 3, ch.d_l.ptr if labels else None, ch.d_poss.ptr, ch.d_min.ptr, ch.d_arg.ptr, _lib.ptr(off), nc, tiles, points,
                                     d_n.ptr, d_perm.ptr, d_dup.ptr, 1.0 / 255.0, o["xyz"].ptr, o["feat"].ptr, o["idx"].ptr, o["labels"].ptr if out_labels else None,
                                     o["cloud"].ptr, o["center"].ptr, None)

    def init(off, nc):
        off = np.ascontiguousarray(off, np.int64)
        return L.ssdr_vote_init_dev(ch.d_poss.ptr, _lib.ptr(off), nc, ch.d_min.ptr, ch.d_arg.ptr, None)

    many = np.arange(4098, dtype=np.int64)
    assert call(ch.off, 0) == SSDR_ERR_INVALID and init(ch.off, 0) == SSDR_ERR_INVALID                       # no clouds
    assert call([0, 300, 300], 2) == SSDR_ERR_INVALID and init([0, 300, 300], 2) == SSDR_ERR_INVALID         # an empty cloud
    assert call(many, 4097) == SSDR_ERR_UNSUPPORTED and init(many, 4097) == SSDR_ERR_UNSUPPORTED             # 4 097 clouds
    assert call([0, 300, 0x40000000], 2) == SSDR_ERR_UNSUPPORTED                                             # more rows than the index arithmetic covers
    assert call(ch.off, 2, tiles=0) == SSDR_ERR_INVALID
    assert call(ch.off, 2, points=0) == SSDR_ERR_INVALID
    assert call(ch.off, 2, labels=False) == SSDR_ERR_INVALID                                                 # labels wanted but missing
    _lib.sync()
    after = ch.state()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))                                          # nothing was launched
    assert call(ch.off, 2, labels=False, out_labels=False) == 0                                              # ... and without labels the chain runs
    _lib.sync()
    # the class: evaluate() needs labels, predictions() does not (Semantic3D's test set)
    nolab = [dict(xyz=c["xyz"], rgb=c["rgb"], labels=None) for c in clouds]
    t = evaluate.VoteTester(weights_small, nolab, config=_cfg(2, 1))
    with pytest.raises(ValueError):
        t.evaluate()
    t.run_batch()
    preds = t.predictions()
    probs = t.probs_host()
    assert [len(p) for p in preds] == [300, 1024]
    assert np.array_equal(np.concatenate(preds), np.argmax(probs, axis=1))
    t.close()
    with pytest.raises(ValueError):
        evaluate.VoteTester(weights_small, [], config=_cfg(2, 1)).evaluate()


@pytest.mark.gpu
def test_chain_at_the_workload_tile_size():
    """num_points 40 960 over clouds of 90 000, 30 000 (smaller than a tile) and 150 000 points: one batch of 20 tiles"""
    from conftest import GPU_LIB, _have_gpu
    from ssdr_al import _lib
    if not _have_gpu():
        pytest.skip("no GPU")
    _lib.use(GPU_LIB)
    try:
        clouds, poss, rng = VO.make_case([90000, 30000, 150000])
        poss = VO.add_ties(poss)
        d = VO.draw_batch(rng, np.random.default_rng(99), 20, 40960)
        gen = VO.Generator(clouds, poss, 40960)
        exp = gen.batch(d)
        assert exp["cloud"][:6].tolist() == [0, 2, 2, 0, 1, 2]
        ch = _Chain(clouds, poss, 40960)
        _compare_batch(ch.tiles(d), exp, "batch")
        _compare_state(ch.state(), gen, "after the batch")
    finally:
        _lib.use(None)
