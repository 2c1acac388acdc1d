"""The Semantic3D flavour of the test-time voting evaluation (ssdr_al.evaluate.VoteTester(dataset="Semantic3D")): the reference's
Network.evaluate_test_semantic3d (SSRD_AL_semantic3d/RandLANet.py:339-485) over Semantic3D_Dataset_Test.get_batch
(semantic3d_dataset_test3.py:129-259), against the NumPy restatements of tests/_feed_oracle.py (the chain with x / y centring and global
rows, tf_augment_input) and tests/_vote_oracle.py (the votes), and a restatement of :394-479 below.

Shapes: num_points 256, batches of 4 tiles, 6 batches per epoch, over clouds of 300, 700 and 1 029 points (none smaller than a tile: the
reference's tree query raises there)."""
import numpy as np
import pytest

import _draw_oracle as DO
import _feed_oracle as FO
import _vote_oracle as VO
from conftest import assert_bits_equal

SIZES = [300, 700, 1029]
N, B, STEPS, NCLS = 256, 4, 6, 8


def _cfg(ignored=None):
    from ssdr_al.helper_tool import ConfigSemantic3D

    class Small(ConfigSemantic3D):
        num_layers = 2
        sub_sampling_ratio = [4, 4]
        d_out = [16, 64]
        num_classes = NCLS
        num_points = N
        val_batch_size = B
        val_steps = STEPS
    if ignored is not None:
        Small.ignored_label_inds = ignored
    return Small


def _case(seed=7, num_labels=NCLS):
    """clouds (colours in 0 .. 1, as the Semantic3D loaders hold them), the initial map = random * 1e-3 (init_possibility, test3.py:129-138), a raw
    cloud per sub-cloud (proj_idx, raw_labels)"""
    rng = np.random.default_rng(seed)
    clouds, poss = [], []
    for n in SIZES:
        clouds.append(dict(xyz=(rng.random((n, 3), dtype=np.float32) * np.array([3, 2.5, 2], np.float32)).astype(np.float32),
                           rgb=(rng.integers(0, 256, (n, 3)) / 255.0).astype(np.float32), labels=rng.integers(0, num_labels, n).astype(np.int32),
                           proj_idx=rng.integers(0, n, 2 * n + 7).astype(np.int32), raw_labels=rng.integers(0, num_labels, 2 * n + 7).astype(np.int32)))
        poss.append(rng.random(n) * 1e-3)
    return clouds, poss


@pytest.fixture(scope="module")
def weights_small():
    from oracle import randla_np as R
    return R.init_weights(0, d_out=(16, 64), num_classes=NCLS)


def _tester(weights, clouds, poss, **kw):
    from ssdr_al import evaluate
    kw.setdefault("config", _cfg())
    return evaluate.VoteTester(weights, clouds, dataset="Semantic3D", possibility=poss, seed=5, **kw)


def _generator(clouds, poss):
    return FO.ChainGenerator(clouds, poss, N, color_scale=np.float32(1.0), xy_only=True, global_rows=True, class_weight=None)


def _oracle_draws(d):
    """the restatement indexes the padding draws of every tile; no cloud here is padded"""
    return dict(d, dup=np.zeros((B, N), np.float32)) if d.get("dup") is None else d


def _compare_chain(t, out, exp, d, noise, clouds, what):
    xyz, feat, idx = out["xyz"].to_host(), out["feat"].to_host(), out["idx"].to_host()
    assert np.array_equal(out["cloud"].to_host(), exp["cloud"]), what + " cloud ids"
    assert_bits_equal(out["center"].to_host(), exp["center"], what + " centres")
    assert np.array_equal(idx, exp["idx"]), what + " global rows"
    assert_bits_equal(xyz, exp["xyz"], what + " xyz")
    assert_bits_equal(feat[..., :3], FO.augment(exp["xyz"], d["rot"], d["scale"], noise), what + " augmented xyz")
    assert_bits_equal(feat[..., 3:], exp["feat"][..., 3:], what + " colours")
    # z is not centred, x / y are (test3.py:173)
    pts = np.concatenate([c["xyz"] for c in clouds])[idx]
    assert_bits_equal(xyz[..., 2], pts[..., 2], what + " z as stored")
    assert_bits_equal(xyz[..., :2], pts[..., :2] - exp["center"][:, None, :2], what + " x / y centred")
    assert np.abs(exp["center"][:, 2]).min() > 1e-3


def _compare_state(t, gen, what):
    assert np.array_equal(np.concatenate(t.possibility()), np.concatenate(gen.possibility)), what + " possibility map (float64, bit for bit)"
    cmin, carg = t.cloud_state()
    assert np.array_equal(cmin, np.asarray(gen.min_possibility)) and np.array_equal(carg, gen.cloud_arg()), what + " cloud minima / arg-minima"


# ---- 1. chain ------------------------------------------------------------------------------------------------------------------------------

def test_chain(backend, weights_small):
    clouds, poss = _case()
    t = _tester(weights_small, clouds, poss)
    assert t.test_smooth == 0.98 and t.vote_gap == 4 and t.draws == "host" and not t.pads
    gen = _generator(clouds, poss)
    for k in range(3):
        d = t.draw(0, k)
        assert set(d) == {"noise", "perm", "dup", "rot", "scale", "aug_noise"} and d["aug_noise"].shape == (B, N, 3) and d["aug_noise"].dtype == np.float64
        out = t.run_batch(d)
        exp = gen.batch(_oracle_draws(d))
        _compare_chain(t, out, exp, d, d["aug_noise"], clouds, "batch %d" % k)
        _compare_state(t, gen, "after batch %d" % k)
    t.close()


# ---- 2. votes ------------------------------------------------------------------------------------------------------------------------------

def test_votes_tile_by_tile(backend, weights_small):
    clouds, poss = _case()
    t = _tester(weights_small, clouds, poss)
    gen = _generator(clouds, poss)
    ref = np.zeros((sum(SIZES), NCLS), np.float32)
    twice = 0
    for k in range(3):
        d = t.draw(0, k)
        out = t.run_batch(d)
        exp = gen.batch(_oracle_draws(d))
        assert np.array_equal(out["idx"].to_host(), exp["idx"])
        probs = out["probs"].to_host()
        assert probs.shape == (B * N, NCLS) and np.isfinite(probs).all()
        VO.vote(ref, exp["idx"], probs, test_smooth=0.98)
        tiles_of = np.zeros(sum(SIZES), np.int32)
        for j in range(B):
            tiles_of[np.unique(exp["idx"][j])] += 1
        twice += int((tiles_of >= 2).sum())
    assert twice > 0                                                   # a point in two tiles of one batch: smoothed twice
    assert_bits_equal(t.probs_host(), ref, "test_probs")
    z = np.zeros_like(ref)                                             # ... and 0.95, the S3DIS rate, gives other votes
    assert not np.array_equal(VO.vote(z.copy(), exp["idx"], probs, test_smooth=0.95), VO.vote(z.copy(), exp["idx"], probs, test_smooth=0.98))
    t.close()


# ---- 3. evaluate() -------------------------------------------------------------------------------------------------------------------------

def _confusion(labels, preds, C):
    m = np.zeros((C, C), np.int64)
    ok = (labels >= 0) & (labels < C)
    np.add.at(m, (labels[ok], preds[ok]), 1)
    return m


def _metrics(clouds, test_probs, off, C, ignored):
    """RandLANet.py:344-349 and :394-479 from the voted probabilities (label_values[k] = k)"""
    val_proportions = np.zeros(C, np.float32)
    values = [v for v in range(C + len(ignored)) if v not in ignored]
    for i, v in enumerate(values):
        val_proportions[i] = np.sum([np.sum(c["raw_labels"] == v) for c in clouds])

    def valid(labels, preds):
        if not ignored:
            return labels, preds
        invalid_idx = np.where(labels == ignored)[0]                                    # :408, :455
        return np.delete(labels, invalid_idx) - 1, np.delete(preds, invalid_idx)

    sub, full, correct, seen = [], [], 0, 0
    for c, cl in enumerate(clouds):
        probs = test_probs[off[c]:off[c + 1]]
        lv, pv = valid(cl["labels"], np.argmax(probs, axis=1).astype(np.int32))         # :399-411
        sub.append(_confusion(lv, pv, C))
        lv, pv = valid(cl["raw_labels"], np.argmax(probs[cl["proj_idx"], :], axis=1))   # :438-458
        correct += int(np.sum(pv == lv)); seen += len(lv)                               # :462-464
        full.append(_confusion(lv, pv, C))
    Cm = np.sum(np.stack(sub), axis=0).astype(np.float32)                               # :418
    Cm *= np.expand_dims(val_proportions / (np.sum(Cm, axis=1) + 1e-6), 1)              # :421
    conf = np.sum(np.stack(full), axis=0)                                               # :470
    ious = VO.iou_from_confusions(conf)
    return dict(sub_confusion=np.sum(np.stack(sub), axis=0), sub_ious=VO.iou_from_confusions(Cm), confusion=conf, ious=ious,
                m_iou=float(np.mean(ious)), oa=correct / float(seen), seen=seen)


def _restated_loop(t, clouds, poss, gap, limit=60):
    """the generator alone through the loop of :355-393: (min_history, stopped)"""
    gen = _generator(clouds, poss)
    hist, last_min = [], -0.5
    for epoch in range(limit):
        for step in range(STEPS):
            gen.batch(_oracle_draws(t.draw(epoch, step)))
        hist.append(float(np.min(gen.min_possibility)))
        if last_min + gap < hist[-1]:
            return hist, True
    return hist, False


def _check_metrics(t, res, m):
    m_iou, oa = res
    assert np.array_equal(t.sub_confusion, m["sub_confusion"]) and np.array_equal(t.confusion, m["confusion"])
    assert oa == m["oa"]
    assert np.allclose(t.ious, m["ious"], rtol=1e-12, atol=0) and np.allclose(t.sub_ious, m["sub_ious"], rtol=1e-12, atol=0)
    assert np.isclose(m_iou, m["m_iou"], rtol=1e-12, atol=0)


def test_evaluate(backend, weights_small):
    clouds, poss = _case()
    t = _tester(weights_small, clouds, poss)
    hist, stopped = _restated_loop(t, clouds, poss, 4)
    assert stopped and hist[-1] > 3.5 and max(hist[:-1]) <= 3.5
    assert any(h > 0.5 for h in hist[:-1])                             # the S3DIS rule (one vote) would have stopped earlier
    res = t.evaluate()
    assert t.epochs == len(hist) and t.tiles == len(hist) * STEPS * B
    assert t.min_history == hist
    m = _metrics(clouds, t.probs_host(), t.off, NCLS, [])
    assert m["seen"] == t.n_raw
    _check_metrics(t, res, m)
    assert 0 < res[0] <= 1 and 0 < res[1] <= 1
    t.close()
    # num_votes too small for the loop to start, and max_epochs ending it first: (m_IoU, 0), nothing evaluated
    t2 = _tester(weights_small, clouds, poss, num_votes=-1)
    assert t2.evaluate() == (0, 0) and t2.epochs == 0 and t2.confusion is None
    assert t2.evaluate(max_epochs=1) == (0, 0) and t2.epochs == 0
    t2.num_votes = 100
    assert t2.evaluate(max_epochs=2) == (0, 0) and t2.epochs == 2 and t2.min_history == hist[:2] and t2.confusion is None
    t2.close()


# ---- 4. ignored labels ---------------------------------------------------------------------------------------------------------------------

def test_ignored_labels(backend, weights_small):
    """ignored_label_inds = [0] over labels 0 .. 8: rows labelled 0 leave both confusions and OA's count, the others shift down by one.
    vote_gap 1 ends the loop early (the gap itself is test_evaluate's)"""
    clouds, poss = _case(num_labels=NCLS + 1)
    assert all((c["labels"] == 0).any() and (c["raw_labels"] == 0).any() and c["labels"].max() == NCLS for c in clouds)
    cfg = _cfg(ignored=[0])
    t = _tester(weights_small, clouds, poss, config=cfg, vote_gap=1)
    hist, stopped = _restated_loop(t, clouds, poss, 1)
    assert stopped and 1 < len(hist) < 30 and hist[-1] > 0.5
    res = t.evaluate()
    assert t.min_history == hist
    m = _metrics(clouds, t.probs_host(), t.off, NCLS, [0])
    assert m["seen"] == sum(int((c["raw_labels"] != 0).sum()) for c in clouds) < t.n_raw
    _check_metrics(t, res, m)
    plain = _metrics(clouds, t.probs_host(), t.off, NCLS, [])
    assert not np.array_equal(plain["confusion"], m["confusion"])
    t.close()
    from ssdr_al import evaluate
    with pytest.raises(ValueError):
        evaluate.VoteTester(weights_small, clouds, config=_cfg(ignored=[0, 1]), dataset="Semantic3D")


# ---- 5. draws="device" ---------------------------------------------------------------------------------------------------------------------

def test_device_draws(backend, weights_small):
    clouds, poss = _case()
    t = _tester(weights_small, clouds, poss, draws="device")
    gen = _generator(clouds, poss)
    scale = t.cfg.augment_noise
    assert scale > 0
    for k in range(2):
        d = t.draw(0, k)
        assert set(d) == {"noise", "rot", "scale"}                      # nothing per row comes from the host
        out = t.run_batch()
        st = t.sets[k % t.DEPTH]
        perm, noise = st["perm"].to_host(), st["aug_noise"].to_host()
        assert np.array_equal(perm, DO.perm(t.seed, 0, k, B, N)), "batch %d perm" % k
        ref = DO.normal(t.seed, 0, k, DO.AUG_NOISE, B * N * 3, scale=scale).reshape(B, N, 3)
        assert np.abs(noise - ref).max() <= 1e-12 * scale                # tests/test_draws.py's bar for this comparison
        exp = gen.batch(dict(d, perm=perm, dup=np.zeros((B, N), np.float32)))
        _compare_chain(t, out, exp, d, noise, clouds, "batch %d" % k)
        _compare_state(t, gen, "after batch %d" % k)
    t.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals(backend, weights_small):
    from ssdr_al import evaluate
    rng = np.random.default_rng(1)
    small = [dict(xyz=rng.random((n, 3), dtype=np.float32), rgb=rng.random((n, 3), dtype=np.float32), labels=rng.integers(0, NCLS, n).astype(np.int32))
             for n in (300, 200)]
    with pytest.raises(ValueError) as e:
        evaluate.VoteTester(weights_small, small, config=_cfg(), dataset="Semantic3D")
    assert "200 points is smaller than num_points = 256" in str(e.value)
    with pytest.raises(ValueError):
        evaluate.VoteTester(weights_small, small[:1], config=_cfg(), dataset="KITTI")
