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
    else:
        raise KeyError(name)
    seed = SEEDS[name]
    W = weights_for(cfg, seed)
    batch = make_batch(cfg, seed, **kw)
    mask = make_mask(batch, seed)
    grad = name != "five"
    r64 = O.run(W, batch, mask, cw, ign, torch.float64, want_grad=grad)
    r32 = O.run(W, batch, mask, cw, ign, torch.float32, want_grad=grad)
    return cfg, W, batch, mask, cw, ign, r64, r32


# seeds for which the input conditions of the gradient test hold on the CPU (conditions() below; tests assert them again)
SEEDS = {"s3dis": 3, "ties": 5, "sem3d": 7, "five": 12, "five_b4": 12}


def conditions(r64, r32):
    """what the float64 and float32 oracle runs say about a case: do they agree on every leaky-ReLU sign and every pooling arg-max set, the
    smallest batch variance any batch norm saw, and the smallest gap between the label's logit and the best other one"""
    signs = all(bool((a == b).all()) for a, b in zip(r64["signs"], r32["signs"]))
    ties = all(bool((a == b).all()) for a, b in zip(r64["ties"], r32["ties"]))
    min_var = min(float(v.min()) for _, v, _ in r64["stats"].values())
    return signs, ties, min_var


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
