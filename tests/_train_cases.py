"""TEST INFRASTRUCTURE ONLY — the batches, configurations and cached oracle runs that tests/test_randla_train.py shares between its cases and
between the two backends (the pyramid comes from the exact C oracle, so both backends and the torch oracle see the same indices)."""
import functools

import numpy as np

RATIOS3, RATIOS5 = [4, 4, 2], [4, 4, 4, 4, 2]


class Cfg3:                                 # the smallest configuration at which every kind of layer exists twice
    k_n = 16
    num_layers = 3
    num_points = 512
    num_classes = 13
    batch_size = 2
    sub_sampling_ratio = RATIOS3
    d_out = [16, 64, 128]
    learning_rate = 1e-2
    lr_decays = {i: 0.95 for i in range(0, 500)}


class Cfg3Sem(Cfg3):                        # Semantic3D-shaped: 8 classes, label 0 ignored, labels 0 .. 8
    num_classes = 8


class Cfg5:                                 # the full five levels: d = 256 / 512 and the 1024-wide decoder_0
    k_n = 16
    num_layers = 5
    num_points = 2048
    num_classes = 13
    batch_size = 1
    sub_sampling_ratio = RATIOS5
    d_out = [16, 64, 128, 256, 512]
    learning_rate = 1e-2
    lr_decays = {i: 0.95 for i in range(0, 500)}


def _cfg(base, name, **kw):
    return type(name, (base,), kw)


# the shapes of tests/test_train_paths.py: no power of two among the rows (DESIGN "The training step's launchers, branch by branch")
CfgB3N360 = _cfg(Cfg3, "CfgB3N360", num_points=360, batch_size=3, sub_sampling_ratio=[4, 3, 2])
CfgOdd = _cfg(CfgB3N360, "CfgOdd", d_out=[6, 20, 44], num_classes=19)
CfgB5N400 = _cfg(Cfg3, "CfgB5N400", num_points=400, batch_size=5, sub_sampling_ratio=[4, 4, 5])
CfgB3N480 = _cfg(Cfg3, "CfgB3N480", num_points=480, batch_size=3)
CfgFiveR = _cfg(Cfg5, "CfgFiveR", num_points=1920, batch_size=3, sub_sampling_ratio=[4, 4, 3, 2, 2])
CfgLoss257 = _cfg(Cfg3Sem, "CfgLoss257", num_points=65824, batch_size=1, d_out=[8, 8, 8])
PATH_CASES = {"b3n360": (CfgB3N360, {}, None, ()), "odd": (CfgOdd, dict(n_labels=20), None, (0,)), "b5n400": (CfgB5N400, {}, None, ()),
              "b3n480": (CfgB3N480, {}, None, ()), "five_r": (CfgFiveR, {}, None, ()), "loss257": (CfgLoss257, dict(n_labels=9), None, (0,))}


def make_batch(cfg, seed, B=None, n_labels=None, repeats=0, colour_labels=False):
    """a host batch dict: xyz [L], neigh, pool, up, feat [B,N,6], labels i32 [B,N], act f32, pse f32.  repeats: the last `repeats` rows of every
    tile are copies of earlier rows (DP.data_aug's padding) — xyz, colours and labels alike.  colour_labels: label = a function of the colour."""
    import oracle
    from oracle import randla_np as R
    B = cfg.batch_size if B is None else B
    N, C = cfg.num_points, cfg.num_classes
    n_labels = C if n_labels is None else n_labels
    rng = np.random.default_rng([seed, 17])
    xyz0 = (rng.random((B, N, 3), dtype=np.float32) * np.array([3.0, 3.0, 1.5], np.float32)).astype(np.float32)
    rgb = rng.random((B, N, 3), dtype=np.float32)
    if colour_labels:
        labels = np.minimum((rgb[..., 0] * n_labels).astype(np.int32), n_labels - 1)
    else:
        labels = rng.integers(0, n_labels, (B, N)).astype(np.int32)
    if repeats:
        src = rng.integers(0, N - repeats, (B, repeats))
        for b in range(B):
            xyz0[b, N - repeats:] = xyz0[b, src[b]]; rgb[b, N - repeats:] = rgb[b, src[b]]; labels[b, N - repeats:] = labels[b, src[b]]
    xyz, neigh, pool, up = R.build_pyramid(xyz0, cfg.sub_sampling_ratio, oracle.c().knn_batch, cfg.k_n)
    pse = labels.copy()
    flip = rng.random((B, N)) < 0.25                         # a quarter of the rows carry a pseudo label that differs from the label
    pse[flip] = (pse[flip] + 1 + rng.integers(0, n_labels - 1, int(flip.sum()))) % n_labels
    return dict(xyz=[np.ascontiguousarray(a, np.float32) for a in xyz], neigh=[np.ascontiguousarray(a, np.int32) for a in neigh],
                pool=[np.ascontiguousarray(a, np.int32) for a in pool], up=[np.ascontiguousarray(a, np.int32) for a in up],
                feat=np.concatenate([xyz0, rgb], -1).astype(np.float32), labels=labels,
                act=(rng.random((B, N)) < 0.6).astype(np.float32), pse=pse.astype(np.float32))


def input_list(batch):
    """the reference's input_list order (s3dis_dataset.py:180-181), host arrays"""
    return batch["xyz"] + batch["neigh"] + batch["pool"] + batch["up"] + [batch["feat"], batch["labels"], batch["act"], batch["pse"]]


def to_device(batch):
    from ssdr_al._lib import DevArray
    return [DevArray.from_host(a) for a in input_list(batch)]


def make_mask(batch, seed):
    B, N = batch["labels"].shape
    return (np.random.default_rng([seed, 23]).random((B * N, 32)) < 0.5).astype(np.uint8)


def weights_for(cfg, seed=0):
    from oracle import randla_np as R
    return R.init_weights(seed, tuple(cfg.d_out), cfg.num_classes, 6)


CLASS_W13 = np.linspace(0.5, 2.0, 13).astype(np.float32)


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """(cfg, weights, batch, mask, class weights, ignored, float64 run, float32 run) of a named case — computed once per process"""
    import torch
    import _train_oracle as O
    if name == "s3dis":
        cfg, kw, cw, ign = Cfg3, {}, CLASS_W13, ()
    elif name == "ties":
        cfg, kw, cw, ign = Cfg3, dict(repeats=32), CLASS_W13, ()
    elif name == "sem3d":
        cfg, kw, cw, ign = Cfg3Sem, dict(n_labels=9), np.linspace(0.6, 1.8, 8).astype(np.float32), (0,)
    elif name == "five":                     # forward only: see test_gradients' docstring
        cfg, kw, cw, ign = Cfg5, {}, CLASS_W13, ()
    elif name == "five_b4":
        cfg, kw, cw, ign = Cfg5, dict(B=4), CLASS_W13, ()
    elif name.split("@")[0] in PATH_CASES:    # "b3n480@1": the case at another seed than SEEDS' (the seed search, the seed-1 finding)
        cfg, kw, cw, ign = PATH_CASES[name.split("@")[0]]
        cw = (CLASS_W13 if cfg.num_classes == 13 else np.linspace(0.6, 1.8, cfg.num_classes).astype(np.float32)) if cw is None else cw
    else:
        raise KeyError(name)
    seed = int(name.split("@")[1]) if "@" in name else SEEDS[name]
    W = weights_for(cfg, seed)
    batch = make_batch(cfg, seed, **kw)
    mask = make_mask(batch, seed)
    grad = name != "five" and not name.startswith(NO_GRAD_CASES)
    r64 = O.run(W, batch, mask, cw, ign, torch.float64, want_grad=grad)
    # the cases that assert margins() ask how far float32 moves a value: one thread, so that the float32 run's order of summation, and with it the answer,
    # does not depend on how many threads the machine gives torch
    threads = torch.get_num_threads()
    if name.split("@")[0] in MARGIN_CASES:
        torch.set_num_threads(1)
    try:
        r32 = O.run(W, batch, mask, cw, ign, torch.float32, want_grad=grad)
    finally:
        torch.set_num_threads(threads)
    return cfg, W, batch, mask, cw, ign, r64, r32


# seeds for which the input conditions of the gradient test hold on the CPU (conditions() below; tests assert them again)
SEEDS = {"s3dis": 3, "ties": 5, "sem3d": 7, "five": 12, "five_b4": 12,
         # tests/test_train_paths.py: of the seeds 1 .. 64 for which conditions() AND margins() hold, the one with the widest margin over its threshold
         # (searched on the CPU; the tests assert both again)
         # (five_r: none of 1 .. 64 meets them, see NO_GRAD_CASES; loss257 compares no gradient that passes a leaky ReLU or a pooling)
         "b3n360": 27, "odd": 62, "b5n400": 32, "b3n480": 44, "five_r": 1, "loss257": 1}


MARGIN_CASES = ("b3n360", "odd", "b5n400", "b3n480")     # the path cases that compare every gradient, hence assert margins()
NO_GRAD_CASES = ("five_r",)     # the path cases for which no seed in 1 .. 64 meets the conditions: forward, loss and moving statistics only


def conditions(r64, r32):
    """what the float64 and float32 oracle runs say about a case: do they agree on every leaky-ReLU sign and every pooling arg-max set, the
    smallest batch variance any batch norm saw, and the smallest gap between the label's logit and the best other one"""
    signs = all(bool((a == b).all()) for a, b in zip(r64["signs"], r32["signs"]))
    ties = all(bool((a == b).all()) for a, b in zip(r64["ties"], r32["ties"]))
    min_var = min(float(v.min()) for _, v, _ in r64["stats"].values())
    return signs, ties, min_var


NEAR = 1e-3


def margins(r64, r32):
    """How far the case is from a decision that float32 may take the other way, from the two oracle runs alone.  Per leaky ReLU: the smallest
    |y64| / max|y64| (margin) and twice the largest |y32 - y64| / max|y64| among the elements the float64 run puts within NEAR of zero (threshold: what
    float32 arithmetic moves such an element by, with a factor 2 for a device that sums in another order).  Per pooling, on the scale max|rows|: the
    smallest gap between the maximum and the largest row below it, and twice the largest change of such a gap between the runs among the gaps
    within NEAR.  The case is fit for a gradient comparison when every margin is above its threshold: then no rounding at float32's level flips a
    sign or an arg-max.  -> dict(ok, lrelu=[(margin, threshold)], pool=[(margin, threshold)], worst=(margin / threshold smallest, kind, index))"""
    out = dict(lrelu=[], pool=[])
    for y64, y32 in zip(r64["pre"], r32["pre"]):
        y64, y32 = y64.numpy(), y32.numpy().astype(np.float64)
        scale = np.abs(y64).max()
        a = np.abs(y64) / scale
        near = a < NEAR
        out["lrelu"].append((float(a.min()), 2.0 * float((np.abs(y32 - y64)[near]).max() / scale) if near.any() else 0.0))
    for p64, p32 in zip(r64["pooled"], r32["pooled"]):
        p64, p32 = p64.numpy(), p32.numpy().astype(np.float64)
        scale = np.abs(p64).max()
        top = p64.max(2, keepdims=True)
        below = np.where(p64 < top, p64, -np.inf)
        k_top, k_run = p64.argmax(2)[:, :, None, :], below.argmax(2)[:, :, None, :]
        run = np.take_along_axis(p64, k_run, 2)
        has = np.isfinite(below.max(2, keepdims=True))
        gap = np.where(has, (top - run) / scale, np.inf)
        gap32 = (np.take_along_axis(p32, k_top, 2) - np.take_along_axis(p32, k_run, 2)) / scale
        near = gap < NEAR
        out["pool"].append((float(gap.min()), 2.0 * float(np.abs(gap32 - gap)[near].max()) if near.any() else 0.0))
    ratios = [(m / t if t > 0 else np.inf, kind, i) for kind in ("lrelu", "pool") for i, (m, t) in enumerate(out[kind])]
    out["worst"] = min(ratios)
    out["ok"] = all(m > t for kind in ("lrelu", "pool") for m, t in out[kind])
    return out


def describe_margins(mg):
    return "smallest leaky-ReLU margin %.3g (threshold there %.3g), smallest pooling gap %.3g (threshold %.3g), smallest margin / threshold %.3g (%s %d): %s" % (
        min(mg["lrelu"])[0], min(mg["lrelu"])[1], min(mg["pool"])[0], min(mg["pool"])[1], mg["worst"][0], mg["worst"][1], mg["worst"][2], "ok" if mg["ok"] else "REJECTED")


def check_gradients(G, cfg, B, r64, r32, only=None):
    """test_gradients' metric and bar on a grads() dict: per tensor max|g - g64| / max|g64| against max(8 x the float32-torch metric, 8 u sqrt(2 n)); a bias
    in front of a batch norm is judged on the scale of its layer's weight gradient.  -> (the report's rows, the rows over the bar, largest metric / bar)"""
    u = 2.0 ** -24
    bad, rows, worst = [], [], 0.0
    for (name, key), g in G.items():
        if only is not None and (name, key) not in only:
            continue
        g64, g32 = r64["grads"][(name, key)], r32["grads"][(name, key)]
        assert g.shape == g64.shape and np.isfinite(g).all(), (name, key)
        scale = np.abs(g64).max()
        if key == "b" and (name, "gamma") in r64["grads"]:
            scale = np.abs(r64["grads"][(name, "W")]).max()
        m_dev, m_32 = np.abs(g - g64).max() / scale, np.abs(g32 - g64).max() / scale
        bar = max(8 * m_32, 8 * u * np.sqrt(2.0 * reduction_rows(cfg, B, name)))
        rows.append("%-36s %-5s device %.2e float32-torch %.2e bar %.2e" % (name, key, m_dev, m_32, bar))
        worst = max(worst, m_dev / bar)
        if not m_dev <= bar:
            bad.append(rows[-1])
    return rows, bad, worst


LEARN_STEPS, LEARN_LR, LEARN_SEED = 40, 1e-2, 21


def learn_case():
    """'It learns': four tiles' worth of batches whose label is a function of the colour (one bit per channel: 8 of the 13 classes), every row active,
    pseudo = label; 40 steps cycle through them.  Returns (cfg, fresh weights, batches [40], masks [40], evaluation batch)."""
    from oracle import randla_np as R
    cfg = Cfg3
    W = R.init_weights(LEARN_SEED, tuple(cfg.d_out), cfg.num_classes, 6, trained_like=False)
    base = []
    for k in range(5):
        b = make_batch(cfg, LEARN_SEED + k)
        rgb = b["feat"][..., 3:]
        lab = ((rgb[..., 0] > 0.5) * 1 + (rgb[..., 1] > 0.5) * 2 + (rgb[..., 2] > 0.5) * 4).astype(np.int32)
        b["labels"], b["pse"], b["act"] = lab, lab.astype(np.float32), np.ones(lab.shape, np.float32)
        base.append(b)
    batches = [base[t % 4] for t in range(LEARN_STEPS)]
    masks = [make_mask(base[0], 1000 + t) for t in range(LEARN_STEPS)]
    return cfg, W, batches, masks, base[4]


@functools.lru_cache(maxsize=None)
def learn_oracle():
    """the float64 oracle's run of the same 40 steps: (losses [40], accuracy of the final weights on the evaluation batch in inference mode)"""
    import torch
    import _train_oracle as O
    cfg, W, batches, masks, ev = learn_case()
    losses, Wf = O.train_steps(W, batches, masks, LEARN_LR)
    r = O.run(Wf, ev, None, training=False, want_grad=False)
    return losses, r["acc"]


def reduction_rows(cfg, B, scope):
    """rows summed into a gradient of this unit: B N_l K for the layers inside the local feature aggregation, B N_l for the per-point ones"""
    N = [cfg.num_points]
    for r in cfg.sub_sampling_ratio:
        N.append(N[-1] // r)
    L = cfg.num_layers
    if scope.startswith("Encoder_layer_"):
        lvl = int(scope[len("Encoder_layer_")])
        per_neighbour = scope.endswith(("LFAmlp1", "LFAmlp2", "LFAatt_pooling_1fc", "LFAatt_pooling_2fc"))
        return B * N[lvl] * (cfg.k_n if per_neighbour else 1)
    if scope == "decoder_0":
        return B * N[L]
    if scope.startswith("Decoder_layer_"):
        return B * N[L - 1 - int(scope[len("Decoder_layer_"):])]
    return B * N[0]
