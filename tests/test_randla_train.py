"""RandLA-Net training on the device (csrc/randla_train.hip, ssdr_al/trainer.py) against tests/_train_oracle.py, the float64 torch restatement
of the reference's training graph.  Every test runs on the CPU logic build and, marked gpu, on the gfx950 build (the ``backend`` fixture).

Shapes: num_layers 3, d_out [16, 64, 128], ratios [4, 4, 2], N = 512 (levels 512 / 128 / 32 / 16), B = 2, 13 classes; the Semantic3D-shaped case
(8 classes, label 0 ignored, labels 0 .. 8); the five-level configuration at N = 2048 (d = 256 / 512, the 1024-wide decoder_0).

Bars.  Where the issue fixes one it is quoted at the assertion.  The others compare the device's error against float64 with the error of the SAME
oracle run in float32 torch (``r32``): the device may be within 8 x of it (it sums in other orders), with a floor from float32's unit roundoff
u = 2^-24 where float32 torch happens to land closer than rounding explains:
  gradients   per tensor, metric max|g - g64| / max|g64|; floor 8 u sqrt(2 n), n = the rows summed into that tensor's gradient (B N_l K inside the
              local feature aggregation, B N_l elsewhere): n products and n additions, each rounded once, add up like a random walk of 2 n steps
              of size u relative to the largest term, and the same factor 8 as above covers the terms that cancel.
  logits      max|z - z64| <= max(8 max|z32 - z64|, 64 u max|z64|)   (about fifty layers, each a few roundings)
  loss        the loss is a mean of terms whose derivative in the logits is at most 2 w_max in the 1-norm: 2 w_max x the logits bar
  moving statistics   m - (m - x) 0.01 is three roundings of numbers no larger than s = max(1, |m|, |x|), the batch statistic's own error enters
              with a factor 0.01: 4e-7 s.  (The biased / unbiased rule moves a 32-row layer's variance by 3e-4 of it.)"""
import ctypes as C

import numpy as np
import pytest

import _train_cases as TC
import _train_oracle as O

U = 2.0 ** -24
MIN_VAR = 1e-3            # 1000 x eps: below it 1 / sqrt(var + eps) multiplies every rounding of xhat by more than 30

NEW_EXPORTS = """ssdr_randla_train_create ssdr_randla_train_destroy ssdr_randla_train_num_params ssdr_randla_train_param_shape
ssdr_randla_train_set_param ssdr_randla_train_get_param ssdr_randla_train_get_grad ssdr_randla_train_set_grad ssdr_randla_train_apply_dev
ssdr_randla_train_set_loss ssdr_randla_train_set_lr ssdr_randla_train_set_step_count ssdr_randla_train_step_count
ssdr_randla_train_workspace_bytes ssdr_randla_train_last_ms ssdr_randla_train_dropout_mask_dev ssdr_randla_train_step_dev ssdr_randla_train_grads_dev
ssdr_randla_train_forward_dev ssdr_randla_train_export ssdr_randla_train_status""".split()


def _trainer(cfg, W, cw=None, ign=(), **kw):
    from ssdr_al.trainer import Trainer
    return Trainer(cfg, class_weights=cw, ignored_labels=ign, **kw).load(W)


def _dev_mask(mask):
    from ssdr_al._lib import DevArray
    return DevArray.from_host(np.ascontiguousarray(mask, np.uint8).reshape(-1))


def _softmax(z):
    z = z - z.max(1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(1, keepdims=True)


def _logits_bar(r64, r32):
    return max(8 * np.abs(r32["logits"] - r64["logits"]).max(), 64 * U * np.abs(r64["logits"]).max())


# ---- 9 (part). the new exports and the import -----------------------------------------------------------------------------------------
def test_exports_present(backend):
    from ssdr_al import _lib
    L = _lib.lib()
    missing = [s for s in NEW_EXPORTS if not hasattr(L, s)]
    assert not missing, missing


def test_trainer_imports_and_enumerates_the_tensors(backend):
    from ssdr_al.trainer import Trainer
    tr = Trainer(TC.Cfg3)
    specs = tr.specs
    want = sum(1 + bool(s[3]) + 4 * bool(s[4]) for s in specs)             # W, b, (gamma, beta, mean, var)
    assert len(tr.shapes) == want
    for u, (name, cin, cout, bias, bn, act, tr_k) in enumerate(specs):
        assert tr.shapes[tr.index[(u, "W")]] == ((cout, cin) if tr_k else (cin, cout)), name       # conv2d_transpose kernels stay [out, in]


# ---- 1. inference-mode forward == the product's inference --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["s3dis", "sem3d", "five"])
def test_eval_forward_equals_inference(backend, case):
    """forward_dev(is_training = 0) and the exported network against Network.load(same weights).infer in "f32": 1e-3 absolute"""
    from ssdr_al import _lib
    from ssdr_al.randlanet import Network
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case(case)
    assert all(np.abs(e["bn"][2]).max() > 0.01 and np.abs(e["bn"][3] - 1).max() > 0.01 for e in W.values() if e["bn"] is not None), "trivial moving statistics"
    tr = _trainer(cfg, W, cw, ign)
    logits, f32 = tr.forward_arrays(TC.to_device(batch), is_training=False)
    _lib.sync()
    probs, feat = Network(cfg).load(W).infer(batch["feat"], batch["xyz"][0])
    got_p, got_f = _softmax(logits.to_host()), f32.to_host()
    print("eval forward %s: probs %.3g, features %.3g" % (case, np.abs(got_p - probs).max(), np.abs(got_f - feat).max()))
    assert np.abs(got_p - probs).max() < 1e-3 and np.abs(got_f - feat).max() < 1e-3
    p2, f2 = tr.export_to().infer(batch["feat"], batch["xyz"][0])
    assert np.abs(got_p - p2).max() < 1e-3 and np.abs(got_f - f2).max() < 1e-3
    # the exported table is the same fold that Network.load makes of the same raw weights
    assert np.abs(p2 - probs).max() < 1e-5 and np.abs(f2 - feat).max() < 1e-4


# ---- 2. training-mode forward, loss, accuracy, moving statistics ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["s3dis", "sem3d", "five"])
def test_training_forward_loss_and_moving_statistics(backend, case):
    from ssdr_al import _lib
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case(case)
    lab, pse = batch["labels"].reshape(-1), batch["pse"].reshape(-1).astype(np.int64)
    assert (lab != pse).any() and (batch["act"] == 0).any() and (batch["act"] == 1).any(), "pseudo labels and activation must matter"
    if ign:
        assert np.isin(lab, ign).any() and r64["valid"] < lab.size
    tr = _trainer(cfg, W, cw, ign)
    dev, dm = TC.to_device(batch), _dev_mask(mask)
    logits, f32 = tr.forward_arrays(dev, is_training=True, mask=dm)
    _lib.sync()
    bar = _logits_bar(r64, r32)
    err = np.abs(logits.to_host() - r64["logits"]).max()
    print("training forward %s: logits %.3g (float32 torch %.3g, bar %.3g)" % (case, err, np.abs(r32["logits"] - r64["logits"]).max(), bar))
    assert err <= bar
    assert np.abs(f32.to_host() - r64["feat32"]).max() <= max(8 * np.abs(r32["feat32"] - r64["feat32"]).max(), 64 * U * np.abs(r64["feat32"]).max())
    before = tr.weights()
    for name, ent in before.items():                       # a forward alone leaves the moving statistics alone
        if ent["bn"] is not None:
            assert np.array_equal(ent["bn"][2], np.asarray(W[name]["bn"][2], np.float32)) and np.array_equal(ent["bn"][3], np.asarray(W[name]["bn"][3], np.float32))
    tr.step_arrays(dev, mask=dm)
    loss, acc = tr.loss(), tr.accuracy()
    print("loss %.8g (float64 %.8g, float32 torch %.8g), accuracy %.6g (%.6g)" % (loss, r64["loss"], r32["loss"], acc, r64["acc"]))
    assert abs(loss - r64["loss"]) <= 2 * float(np.max(cw)) * bar
    # accuracy counts rows: the device may differ from float64 only in rows whose label logit ties with the best other one within the logits bar
    z = r64["logits"]
    assert abs(acc - r64["acc"]) * r64["valid"] <= _near_ties(z, lab, ign, cfg.num_classes, 2 * bar) + 1e-3
    assert tr.step_count() == 1 and tr.status() == 0
    mv = O.moving_update(W, r64["stats"])
    after = tr.weights()
    worst = 0.0
    for name, (mu, var) in mv.items():
        got_mu, got_var = after[name]["bn"][2], after[name]["bn"][3]
        for got, ref, old in ((got_mu, mu, W[name]["bn"][2]), (got_var, var, W[name]["bn"][3])):
            s = np.maximum(1.0, np.maximum(np.abs(ref), np.abs(old)))
            worst = max(worst, float((np.abs(got - ref) / s).max()))
    print("moving statistics: worst error / scale %.3g" % worst)
    assert worst <= 4e-7
    # the rule itself: a rank-4 layer of few rows takes the unbiased variance (the biased one would sit 0.01 var / (n - 1) away), fc0 the biased one
    # (the two rules differ by 0.01 var / (n - 1): the bar above must be able to tell them apart, on the rank-4 layers and on fc0)
    apart = {name: float((0.01 * var.numpy() / (n - 1)).max()) for name, (_, var, n) in r64["stats"].items()}
    print("rules apart: rank-4 layers %.3g, fc0 %.3g" % (max(v for k, v in apart.items() if k != "fc0"), apart["fc0"]))
    assert max(v for k, v in apart.items() if k != "fc0") > 10 * 4e-7 and apart["fc0"] > 2 * 4e-7, "the test cannot tell the two variance rules apart"


def _near_ties(z, lab, ign, C, tol):
    """rows (not ignored) whose label logit is within tol of the best other logit"""
    red = list(range(C))
    for i in ign:
        red = red[:i] + [0] + red[i:]
    red = np.asarray(red)
    keep = ~np.isin(lab, ign) if len(ign) else np.ones(lab.shape, bool)
    zz, ll = z[keep], red[lab[keep]]
    own = zz[np.arange(len(ll)), ll]
    other = zz.copy(); other[np.arange(len(ll)), ll] = -np.inf
    return int((np.abs(own - other.max(1)) <= tol).sum())


# ---- 3 / 4. gradients of every parameter tensor -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["s3dis", "sem3d", "ties", "five_b4"])
def test_gradients(backend, case):
    """Every parameter tensor's gradient against float64: metric max|g - g64| / max|g64|, bar max(8 x the float32-torch metric, 8 u sqrt(2 n)) (module
    docstring).  A bias in front of a batch norm has a mathematically zero gradient and is judged on the scale of its layer's weight gradient.
    No element is excluded.

    Input conditions: the float64 and float32 oracle runs agree on every leaky-ReLU sign and every pooling arg-max set, and no batch norm sees a
    batch variance below 1000 eps.  The last one is why the five-level configuration is checked here at B = 4, not B = 1: with N = 2048 its
    deepest level has 8 points, every pooled row is the maximum over all of them, so at B = 1 the rows decoder_0 normalises are identical, its
    batch variance is 0 and every gradient of level 4 is mathematically zero (float64 leaves 1e-14, float32 torch 1e-6: a relative error
    means nothing there).  B = 1 stays the shape of the forward, loss and inference cases above.
    'ties' (case 4): 480 distinct rows plus 32 repeats per tile; tied maxima exist at level 0 and the gradient is shared among them.
    Dividing by the number of tied rows matters: giving every tied row the WHOLE gradient would double it (the one-winner restatement of the
    oracle, ``one_winner=True``, is there for comparison by hand; on exact copies it gives the same parameter gradients as the even split)."""
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case(case)
    signs, ties, min_var = TC.conditions(r64, r32)
    assert signs and ties, "the float32 and float64 oracle runs disagree on a sign or an arg-max set: pick another seed"
    assert min_var >= MIN_VAR, "a degenerate batch norm (variance %.3g)" % min_var
    if case == "ties":
        n_tied = int((r64["ties"][0].sum(2) > 1).sum())
        assert n_tied > 0, "no tied maximum at level 0"
        # (tied rows are exact copies, their forward states are identical and the backward is linear in the incoming gradient, so a PARAMETER
        # gradient sees only the sum over a tie's rows: what this case pins is that a tie neither loses nor doubles its gradient)
    tr = _trainer(cfg, W, cw, ign)
    tr.grads_arrays(TC.to_device(batch), mask=_dev_mask(mask))
    G = tr.grads()
    assert tr.step_count() == 0
    B = batch["labels"].shape[0]
    rows, bad, _ = TC.check_gradients(G, cfg, B, r64, r32)      # the loop, shared with tests/test_train_paths.py
    print("\n".join(rows))
    assert not bad, "\n".join(bad)
    after = tr.weights()
    for name, ent in after.items():                     # grads_dev changes neither the weights nor the moving statistics
        assert np.array_equal(ent["W"], np.asarray(W[name]["W"], np.float32))
        if ent["bn"] is not None:
            assert np.array_equal(ent["bn"][3], np.asarray(W[name]["bn"][3], np.float32))


# ---- 5. loss edges ----------------------------------------------------------------------------------------------------------------------------
def test_loss_edges(backend):
    import torch
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case("s3dis")
    dm = _dev_mask(mask)
    bar = _logits_bar(r64, r32)
    # activation all 0: loss 0, every gradient 0, the weights move only by Adam's zero update (not at all)
    b0 = dict(batch, act=np.zeros_like(batch["act"]))
    tr = _trainer(cfg, W, cw)
    tr.step_arrays(TC.to_device(b0), mask=dm)
    assert tr.loss() == 0.0 and tr.status() == 0
    assert all(not g.any() for g in tr.grads().values())
    after = tr.weights()
    for name, ent in after.items():
        assert np.array_equal(ent["W"], np.asarray(W[name]["W"], np.float32)), name
        if ent["bn"] is not None:
            assert np.array_equal(ent["bn"][0], np.asarray(W[name]["bn"][0], np.float32)) and not np.array_equal(ent["bn"][2], np.asarray(W[name]["bn"][2], np.float32))
    # a class weight of 0: against the oracle with the same weights
    cw0 = cw.copy(); cw0[3] = 0.0
    assert (batch["pse"] == 3).any()
    ref = O.run(W, batch, mask, cw0, (), torch.float64, want_grad=False)
    tr = _trainer(cfg, W, cw0)
    tr.grads_arrays(TC.to_device(batch), mask=dm)
    assert abs(tr.loss() - ref["loss"]) <= 2 * float(cw0.max()) * bar and abs(ref["loss"] - r64["loss"]) > 100 * bar
    # pseudo != label: the loss follows the pseudo labels, the accuracy the labels (swap them and both numbers move)
    swapped = dict(batch, labels=batch["pse"].astype(np.int32), pse=batch["labels"].astype(np.float32))
    ref_s = O.run(W, swapped, mask, cw, (), torch.float64, want_grad=False)
    assert abs(ref_s["loss"] - r64["loss"]) > 100 * bar
    tr = _trainer(cfg, W, cw)
    tr.grads_arrays(TC.to_device(swapped), mask=dm)
    assert abs(tr.loss() - ref_s["loss"]) <= 2 * float(cw.max()) * bar
    assert abs(tr.accuracy() - ref_s["acc"]) * ref_s["valid"] <= _near_ties(ref_s["logits"], swapped["labels"].reshape(-1), (), cfg.num_classes, 2 * bar) + 1e-3
    # every row ignored: the status bit, zeros, nothing infinite
    cfg8, W8, batch8, mask8, cw8, ign8, _, _ = TC.oracle_case("sem3d")
    gone = dict(batch8, labels=np.zeros_like(batch8["labels"]))
    tr = _trainer(cfg8, W8, cw8, ign8)
    tr.step_arrays(TC.to_device(gone), mask=_dev_mask(mask8))
    assert tr.loss() == 0.0 and tr.accuracy() == 0.0
    assert tr.status() & 1
    assert tr.status() == 0                                  # reading clears
    assert all(np.isfinite(g).all() and not g.any() for g in tr.grads().values())
    assert all(np.isfinite(e["W"]).all() for e in tr.weights().values())


# ---- 6. Adam ------------------------------------------------------------------------------------------------------------------------------------
def test_adam_three_steps(backend):
    """fixed gradients through the test hook, against tf.train.AdamOptimizer's rule restated in float32 NumPy: 1e-6 of the tensor's largest update
    (about eight float32 roundings per element); the step count and lr_t at t = 1, 2, 3; set_lr and decay take effect at the next step"""
    from ssdr_al import _lib
    cfg = TC.Cfg3
    W = TC.weights_for(cfg, 1)
    tr = _trainer(cfg, W, lr=0.01)
    rng = np.random.default_rng(9)
    names = [(n, k, i) for n, k, i in tr._tensors() if k not in ("mean", "var")]
    state = {}
    for n, k, i in names:
        p = tr._get(i, 0)
        state[i] = (p, np.zeros_like(p), np.zeros_like(p))
    lrs = [0.01, 0.003, 0.003 * cfg.lr_decays[1]]
    for t in (1, 2, 3):
        if t == 2:
            tr.set_lr(0.003)
        if t == 3:
            tr.decay(1)
        assert abs(tr.lr - lrs[t - 1]) < 1e-12
        upd = {}
        for n, k, i in names:
            g = (rng.normal(0, 1, tr.shapes[i]) * 10.0 ** rng.integers(-6, 1)).astype(np.float32)
            _lib.check(tr._lib.ssdr_randla_train_set_grad(tr._h, i, _lib.ptr(g)))
            p, m, v = state[i]
            p2, m, v, lr_t = O.adam_np(p, g, m, v, t, np.float32(lrs[t - 1]))
            upd[i] = np.abs(p2 - p).max()
            state[i] = (p2, m, v)
        assert abs(float(lr_t) - lrs[t - 1] * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)) < 1e-9
        _lib.check(tr._lib.ssdr_randla_train_apply_dev(tr._h, None))
        _lib.sync()
        assert tr.step_count() == t
        for n, k, i in names:
            p, m, v = state[i]
            assert np.abs(tr._get(i, 0) - p).max() <= 1e-6 * max(upd[i], 1e-30), (n, k, t)
            assert np.allclose(tr._get(i, 1), m, rtol=1e-5, atol=1e-12) and np.allclose(tr._get(i, 2), v, rtol=1e-5, atol=1e-20), (n, k, t)


# ---- 7. dropout -------------------------------------------------------------------------------------------------------------------------------
def test_dropout(backend):
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case("s3dis")
    B, N = batch["labels"].shape
    tr = _trainer(cfg, W, cw, seed=4)
    dev = TC.to_device(batch)
    bias = np.asarray(W["fc"]["b"], np.float32)
    m1 = mask.copy(); m1[5] = 0; m1[700] = 0
    z1 = tr.forward_arrays(dev, True, mask=_dev_mask(m1))[0].to_host()
    assert np.array_equal(z1[5], bias) and np.array_equal(z1[700], bias)           # a row with nothing kept: the bias, bit for bit
    m2 = m1.copy(); m2[9, 3] ^= 1
    z2, f2 = (a.to_host() for a in tr.forward_arrays(dev, True, mask=_dev_mask(m2)))
    rows = np.flatnonzero((z1 != z2).any(1))
    assert rows.tolist() == [9]                                                      # one bit of the mask: that row alone
    f1 = tr.forward_arrays(dev, True, mask=_dev_mask(m1))[1].to_host()
    assert np.array_equal(f1, f2)                                                    # last_second_features are pre-dropout
    kept = tr.forward_arrays(dev, True, mask=_dev_mask(np.ones_like(mask)))[0].to_host()
    assert np.abs(kept - (2 * f1) @ np.asarray(W["fc"]["W"], np.float32) - bias).max() < 1e-4      # kept values are scaled by 1 / keep
    # the generated mask: a pure function of (seed, step), fair
    n = B * N * 32
    assert n == 2 * 512 * 32
    a = tr.make_mask(B, N, step=0).to_host().copy()
    b = tr.make_mask(B, N, step=0).to_host().copy()
    c = tr.make_mask(B, N, step=1).to_host().copy()
    assert np.array_equal(a, b) and not np.array_equal(a, c) and set(np.unique(a)) == {0, 1}
    other = _trainer(cfg, W, cw, seed=5).make_mask(B, N, step=0).to_host()
    assert not np.array_equal(a, other)
    for m in (a, c, other):
        assert abs(int(m.sum()) - n / 2) <= 5 * np.sqrt(n) / 2
    # inference mode ignores the mask
    e0 = tr.forward_arrays(dev, False)[0].to_host()
    e1 = tr.forward_arrays(dev, False, mask=_dev_mask(np.zeros_like(mask)))[0].to_host()
    assert np.array_equal(e0, e1) and not np.array_equal(e0, z1)


# ---- 8. it learns --------------------------------------------------------------------------------------------------------------------------------
def test_it_learns(backend):
    """40 steps at the test shape on tiles whose label is a function of the colour: the loss ends below half its first value and the exported
    network's accuracy is above chance.  Both hold for the float64 oracle's run of the same steps (conditions, asserted first)."""
    from ssdr_al.randlanet import Network
    losses64, acc64 = TC.learn_oracle()
    rec = {"losses": losses64, "acc": acc64}
    chance = 1.0 / 13
    assert rec["losses"][-1] < 0.5 * rec["losses"][0] and float(rec["acc"]) > chance, "the oracle's own run does not learn: the case is no test"
    cfg, W, batches, masks, ev = TC.learn_case()
    tr = _trainer(cfg, W, lr=TC.LEARN_LR)
    devs = {}
    first = last = None
    for t, (b, m) in enumerate(zip(batches, masks)):
        if id(b) not in devs:
            devs[id(b)] = TC.to_device(b)
        tr.step_arrays(devs[id(b)], mask=_dev_mask(m))
        if t == 0:
            first = tr.loss()
    last = tr.loss()
    probs, _ = tr.export_to(Network(cfg)).infer(ev["feat"], ev["xyz"][0])
    acc = float((probs.argmax(1) == ev["labels"].reshape(-1)).mean())
    print("loss %.4f -> %.4f (float64 oracle %.4f -> %.4f), accuracy %.3f (oracle %.3f)" % (first, last, rec["losses"][0], rec["losses"][-1], acc, float(rec["acc"])))
    assert abs(first - rec["losses"][0]) < 1e-3
    assert last < 0.5 * first and acc > chance


# ---- 9. plumbing -------------------------------------------------------------------------------------------------------------------------------
def _feeder(dataset, seed=2):
    from ssdr_al import training
    from ssdr_al.helper_tool import ConfigS3DIS, ConfigSemantic3D
    sem = dataset == "Semantic3D"

    class Small(ConfigSemantic3D if sem else ConfigS3DIS):
        num_points = 512
        num_layers = 3
        sub_sampling_ratio = [4, 4, 2]
        d_out = [16, 64, 128]
        batch_size = 2
        train_steps = 2
        num_classes = 8 if sem else 13
    rng = np.random.default_rng(seed)
    clouds, pg = [], []
    for n in ((700, 900, 1500) if sem else (300, 800, 1300)):
        xyz = (rng.random((n, 3)) * [4, 4, 2]).astype(np.float32)
        lab = rng.integers(0, 9 if sem else 13, n).astype(np.int32)
        clouds.append(dict(xyz=xyz, rgb=rng.random((n, 3)).astype(np.float32), labels=lab))
        pse = lab.copy(); flip = rng.random(n) < 0.2; pse[flip] = rng.integers(1 if sem else 0, 9 if sem else 13, int(flip.sum()))
        pg.append(np.stack([(rng.random(n) < 0.5).astype(np.float32), pse.astype(np.float32)]))
    return training.TrainFeeder(clouds, pg, config=Small, dataset=dataset, seed=seed), Small


@pytest.mark.parametrize("dataset", ["S3DIS", "Semantic3D"])
def test_step_on_a_feeder_batch(backend, dataset):
    """Trainer.step(batch) on a real TrainFeeder batch equals step_arrays on batch.to_host(): the forward values (loss, accuracy) bit for bit.  The
    weights afterwards carry the scatter atomics' run-dependent low bits and are held to a loose relative bound here; test_gradients holds the gradients."""
    from ssdr_al._lib import DevArray
    feeder, cfg = _feeder(dataset)
    ign = (0,) if dataset == "Semantic3D" else ()
    W = TC.weights_for(cfg, 6)
    a, b = _trainer(cfg, W, None, ign, seed=3), _trainer(cfg, W, None, ign, seed=3)
    batch = feeder.next_batch(None)
    assert len(batch) == 4 * 3 + 6 and batch[4 * 3 + 2].dtype == np.float32 and batch[4 * 3 + 3].dtype == np.float32
    host = batch.to_host()
    a.step(batch)
    assert batch.released
    la, aa = a.loss(), a.accuracy()
    b.step_arrays([DevArray.from_host(h) for h in host])
    assert np.float32(la).tobytes() == np.float32(b.loss()).tobytes() and np.float32(aa).tobytes() == np.float32(b.accuracy()).tobytes()
    assert a.status() == 0 and np.isfinite(la) and la > 0
    wa, wb = a.weights(), b.weights()
    for name in wa:
        assert np.abs(wa[name]["W"] - wb[name]["W"]).max() <= 1e-3 * max(np.abs(wb[name]["W"]).max(), 1e-3), name      # |update| <= lr = 1e-2 per element
        if wa[name]["bn"] is not None:
            assert np.array_equal(wa[name]["bn"][2], wb[name]["bn"][2]) and np.array_equal(wa[name]["bn"][3], wb[name]["bn"][3]), name   # forward values
    feeder.close()


def test_train_round_runs_the_epochs(backend):
    """train_round without a tester: every batch of every epoch is one step (the last S3DIS batch is partial), the rate decays per epoch"""
    feeder, cfg = _feeder("S3DIS")
    tr = _trainer(cfg, TC.weights_for(cfg, 6))
    assert feeder.steps_per_epoch == 2
    assert tr.train_round(feeder, 2) == (0, 0)
    assert tr.step_count() == 4 and np.isfinite(tr.loss()) and tr.status() == 0
    assert abs(tr.lr - cfg.learning_rate * cfg.lr_decays[1] * cfg.lr_decays[2]) < 1e-12
    feeder.close()


def test_train_round_with_a_tester(backend):
    """train_round through a VoteTester: from int(0.4 epochs) on every epoch ends with the voting evaluation of the exported network; the best
    (m_IoU, OA) comes back and the state that gave it is kept"""
    from ssdr_al import evaluate
    feeder, cfg = _feeder("S3DIS")

    class Val(cfg):
        val_batch_size = 2
        val_steps = 2
    rng = np.random.default_rng(4)
    clouds = [dict(xyz=(rng.random((n, 3)) * [4, 4, 2]).astype(np.float32), rgb=rng.random((n, 3)).astype(np.float32),
                   labels=rng.integers(0, 13, n).astype(np.int32)) for n in (700, 900)]
    W = TC.weights_for(cfg, 6)
    tester = evaluate.VoteTester(W, clouds, config=Val, num_votes=2)
    tr = _trainer(cfg, W)
    seen = []
    run = tester.evaluate
    tester.evaluate = lambda *a, **k: (seen.append(tr.step_count()), run(*a, **k))[1]
    m_iou, oa = tr.train_round(feeder, 3, tester)
    assert seen == [2, 4, 6]                                   # int(0.4 * 3) = 1: after every epoch
    assert 0 < m_iou <= 1 and 0 < oa <= 1 and tr.best_state is not None and tr.best_state["step"] in seen
    assert tr.step_count() == 6 and tr.status() == 0
    tester.close(); feeder.close()


def test_state_round_trip_and_streams(backend):
    """state() / load_state() reproduce the next step's loss; a caller's stream; two trainers on two streams"""
    from ssdr_al import _lib
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case("s3dis")
    L = _lib.lib()
    mk = lambda: (lambda p: (_lib.check(L.ssdr_stream_create(C.byref(p))), p.value)[1])(C.c_void_p())
    s1, s2 = mk(), mk()
    dev, dm = TC.to_device(batch), _dev_mask(mask)
    a = _trainer(cfg, W, cw)
    a.step_arrays(dev, stream=s1, mask=dm)
    first = a.loss()
    st = a.state()
    assert st["step"] == 1 and isinstance(st["adam"][("fc", "W")][0], np.ndarray) and st["adam"][("fc", "W")][0].any()
    a.step_arrays(dev, stream=s1, mask=dm)
    second = a.loss()
    assert second != first
    b = _trainer(cfg, TC.weights_for(cfg, 99), cw).load_state(st)
    c = _trainer(cfg, TC.weights_for(cfg, 98), cw).load_state(st)
    b.step_arrays(dev, stream=s1, mask=dm)            # two trainers, two streams, enqueued back to back
    c.step_arrays(dev, stream=s2, mask=dm)
    assert np.float32(b.loss()).tobytes() == np.float32(second).tobytes() and np.float32(c.loss()).tobytes() == np.float32(second).tobytes()
    assert b.step_count() == 2
    assert abs(first - r64["loss"]) <= 2 * float(cw.max()) * _logits_bar(r64, r32)
    _lib.sync(s1); _lib.sync(s2)
    L.ssdr_stream_destroy(s1); L.ssdr_stream_destroy(s2)


def test_refused_arguments(backend):
    from ssdr_al import _lib
    from ssdr_al.trainer import Trainer, _bind
    cfg, W, batch, mask, cw, ign, r64, r32 = TC.oracle_case("s3dis")
    L = _bind(_lib.lib())
    h = C.c_void_p()
    d = np.asarray(cfg.d_out, np.int32)
    assert L.ssdr_randla_train_create(3, _lib.ptr(d), 8, 13, 6, C.byref(h)) != 0 and b"k_n" in L.ssdr_last_error()
    assert L.ssdr_randla_train_create(3, None, 16, 13, 6, C.byref(h)) != 0
    assert L.ssdr_randla_train_create(3, _lib.ptr(d), 16, 13, 6, None) != 0
    tr = _trainer(cfg, W, cw)
    dev, dm = TC.to_device(batch), _dev_mask(mask)
    before = tr.weights()

    class Odd(cfg):
        sub_sampling_ratio = [4, 4, 3]           # 32 rows at level 2 are not divisible by 3
    tr.config = Odd
    with pytest.raises(_lib.SsdrError) as e:
        tr.step_arrays(dev, mask=dm)
    assert "divisible" in str(e.value)
    tr.config = cfg
    B, N, r, ptrs, feat, labels, act, pse = tr._pyramid(dev)
    args = [tr._h, B, N, feat.ptr, ptrs[0], _lib.ptr(r), ptrs[1], ptrs[2], ptrs[3], labels.ptr, act.ptr, pse.ptr, dm.ptr, None, None, None]
    for hole in (0, 3, 4, 6, 7, 8, 9, 10, 11, 12):
        bad = list(args); bad[hole] = None
        assert L.ssdr_randla_train_step_dev(*bad) != 0 and L.ssdr_last_error(), hole
    fresh = Trainer(cfg)                          # no weights yet
    with pytest.raises(_lib.SsdrError):
        fresh.step_arrays(dev, mask=dm)
    _lib.sync()
    assert tr.step_count() == 0 and tr.status() == 0
    after = tr.weights()                          # nothing was launched
    assert all(np.array_equal(after[n]["W"], before[n]["W"]) for n in before)
