"""TEST INFRASTRUCTURE ONLY — torch (CPU) restatement of the reference's TRAINING graph with autograd, float64 by default.

Written from the reference's Python: SSDR_AL_s3dis/RandLANet.py:36-84 (graph, loss, optimiser), :140-180 (inference), :486-503 (get_loss),
:505-585 (the blocks), helper_tf_util.py:111-246 (conv2d / conv2d_transpose: bias, batch norm eps 1e-6 momentum 0.99, leaky ReLU 0.2).
PARITY UNPINNED, as oracle/randla_np.py: TensorFlow is not available, so the batch-norm moving-variance rule (fused rank-4 path: batch variance
times n / (n - 1); fc0's rank-3 path: the biased one) and tf.train.AdamOptimizer's formula are restated here, not measured.

Conventions: batch norm is written out by hand (batch mean, biased variance over all rows); ``amax`` does the pooling and splits a tied
maximum's gradient evenly, as TF's reduce_max gradient does; the loss and Adam are written out (torch.optim.Adam puts epsilon elsewhere)."""
import numpy as np
import torch

BN_EPS, LRELU, MOMENTUM = 1e-6, 0.2, 0.99


def params_of(weights, dtype=torch.float64):
    """reference-named dict -> {(scope, key): leaf tensor}; the moving statistics are plain tensors"""
    P = {}
    for name, ent in weights.items():
        P[(name, "W")] = torch.tensor(np.asarray(ent["W"], np.float64), dtype=dtype, requires_grad=True)
        if ent.get("b") is not None:
            P[(name, "b")] = torch.tensor(np.asarray(ent["b"], np.float64), dtype=dtype, requires_grad=True)
        if ent.get("bn") is not None:
            g, beta, mu, var = ent["bn"]
            P[(name, "gamma")] = torch.tensor(np.asarray(g, np.float64), dtype=dtype, requires_grad=True)
            P[(name, "beta")] = torch.tensor(np.asarray(beta, np.float64), dtype=dtype, requires_grad=True)
            P[(name, "mean")] = torch.tensor(np.asarray(mu, np.float64), dtype=dtype)
            P[(name, "var")] = torch.tensor(np.asarray(var, np.float64), dtype=dtype)
    return P


class Graph:
    def __init__(self, weights, P, training, dtype, one_winner=False):
        self.meta, self.P, self.training, self.dtype, self.one_winner = weights, P, training, dtype, one_winner
        self.stats = {}        # scope -> (batch mean, biased batch variance, rows)
        self.signs = []        # pre-activation > 0 of every leaky ReLU
        self.ties = []         # per pooling: which of the 16 rows equal the maximum
        self.pre = []          # the pre-activation of every leaky ReLU (for _train_cases.margins)
        self.pooled = []       # per pooling: the 16 rows it takes the maximum of

    def lrelu(self, y):
        self.signs.append((y > 0).detach())
        self.pre.append(y.detach())
        return torch.where(y > 0, y, y * LRELU)

    def linear(self, x, name):
        """conv2d / conv2d_transpose / dense on the channel axis, up to and including the batch norm (helper_tf_util.py:111-166, :169-246)"""
        ent = self.meta[name]
        w = self.P[(name, "W")]
        y = x @ (w.T if ent.get("transposed") else w)
        if (name, "b") in self.P:
            y = y + self.P[(name, "b")]
        if (name, "gamma") in self.P:
            if self.training:
                flat = y.reshape(-1, y.shape[-1])
                mu = flat.mean(0)
                var = ((flat - mu) ** 2).mean(0)                       # biased: what the batch is normalised with
                self.stats[name] = (mu.detach(), var.detach(), flat.shape[0])
            else:
                mu, var = self.P[(name, "mean")], self.P[(name, "var")]
            y = (y - mu) / torch.sqrt(var + BN_EPS) * self.P[(name, "gamma")] + self.P[(name, "beta")]
        return y

    def conv(self, x, name):
        y = self.linear(x, name)
        return self.lrelu(y) if self.meta[name]["act"] else y


def _gather(pc, idx):
    """gather_neighbour (RandLANet.py:561-570): pc [B,N,d], idx [B,M,K] -> [B,M,K,d]"""
    B, M, K = idx.shape
    flat = idx.reshape(B, M * K, 1).expand(-1, -1, pc.shape[-1])
    return torch.gather(pc, 1, flat).reshape(B, M, K, pc.shape[-1])


def _att_pooling(g, fset, name):
    """RandLANet.py:572-585"""
    act = fset @ g.P[(name + "fc", "W")]
    scores = torch.softmax(act, dim=2)
    return g.conv((fset * scores).sum(2), name + "mlp")


def forward(g, batch, mask):
    """inference() (RandLANet.py:140-180) -> logits [B N, C], last_second_features [B N, 32]"""
    dt = g.dtype
    L = len(batch["neigh"])
    idx = lambda a: torch.as_tensor(np.asarray(a, np.int64))
    f = g.conv(torch.as_tensor(batch["feat"], dtype=dt), "fc0")
    enc = []
    for i in range(L):
        p = "Encoder_layer_%d" % i
        x = torch.as_tensor(batch["xyz"][i], dtype=dt)
        nb = idx(batch["neigh"][i])
        f_pc = g.conv(f, p + "mlp1")                                    # dilated_res_block :506
        nxyz = _gather(x, nb)                                           # relative_pos_encoding :529-535
        tile = x[:, :, None, :].expand_as(nxyz)
        rel = tile - nxyz
        dis = torch.sqrt((rel * rel).sum(-1, keepdim=True))
        f_xyz = g.conv(torch.cat([dis, rel, tile, nxyz], -1), p + "LFAmlp1")
        agg = _att_pooling(g, torch.cat([_gather(f_pc, nb), f_xyz], -1), p + "LFAatt_pooling_1")
        f_xyz = g.conv(f_xyz, p + "LFAmlp2")
        agg = _att_pooling(g, torch.cat([_gather(agg, nb), f_xyz], -1), p + "LFAatt_pooling_2")
        out = g.lrelu(g.linear(agg, p + "mlp2") + g.linear(f, p + "shortcut"))        # :508-512
        pooled = _gather(out, idx(batch["pool"][i]))                    # random_sample :537-548
        # one_winner: torch.max(dim) sends a tied maximum's whole gradient to one row — what TF does NOT do; only there to show that the tests' bars notice
        samp = pooled.max(dim=2).values if g.one_winner else pooled.amax(dim=2)
        g.ties.append((pooled == samp[:, :, None, :]).detach())
        g.pooled.append(pooled.detach())
        if i == 0:
            enc.append(out)
        enc.append(samp)
        f = samp
    f = g.conv(enc[-1], "decoder_0")
    for j in range(L):
        up = idx(batch["up"][-j - 1])                                   # nearest_interpolation :550-559
        interp = _gather(f, up)[:, :, 0, :]
        f = g.conv(torch.cat([enc[-j - 2], interp], -1), "Decoder_layer_%d" % j)
    f1 = g.conv(f, "fc1")
    f2 = g.conv(f1, "fc2")
    h = f2
    if g.training:                                                      # dropout keep_prob 0.5 (:176-177)
        m = torch.as_tensor(np.asarray(mask, np.float64).reshape(f2.shape), dtype=dt)
        h = f2 * m * 2.0
    logits = g.conv(h, "fc")
    return logits.reshape(-1, logits.shape[-1]), f2.reshape(-1, 32)


def loss_and_accuracy(logits, labels, activation, pseudo, class_weights, ignored, num_classes):
    """RandLANet.py:43-84 and get_loss :486-503.  Returns (loss, accuracy, valid rows); no valid row: zeros."""
    dt = logits.dtype
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    pseudo = np.asarray(pseudo).reshape(-1).astype(np.int64)
    ignored_bool = np.zeros(labels.shape, bool)
    for ign in ignored:
        ignored_bool |= labels == ign
    valid = np.flatnonzero(~ignored_bool)
    reducing = list(range(num_classes))
    for ign in ignored:
        reducing = reducing[:ign] + [0] + reducing[ign:]
    reducing = np.asarray(reducing, np.int64)
    if len(valid) == 0:
        z = logits.sum() * 0
        return z, z.detach(), 0
    vl = logits[torch.as_tensor(valid)]
    v_lab = torch.as_tensor(reducing[labels[valid]])
    v_pse = torch.as_tensor(reducing[pseudo[valid]])
    v_act = torch.as_tensor(np.asarray(activation, np.float64).reshape(-1)[valid], dtype=dt)
    cw = torch.as_tensor(np.asarray(class_weights, np.float64), dtype=dt)
    ce = torch.logsumexp(vl, 1) - vl.gather(1, v_pse[:, None])[:, 0]
    loss = (ce * cw[v_pse] * v_act).mean()
    target = vl.gather(1, v_lab[:, None])                               # in_top_k(k = 1): nothing strictly above the label's logit
    acc = ((vl > target).sum(1) == 0).to(dt).mean()
    return loss, acc.detach(), len(valid)


def run(weights, batch, mask, class_weights=None, ignored=(), dtype=torch.float64, training=True, want_grad=True, one_winner=False):
    """One forward (+ backward).  Returns dict(logits, feat32, loss, acc, grads {(scope, key)}, stats, signs, ties)."""
    P = params_of(weights, dtype)
    g = Graph(weights, P, training, dtype, one_winner)
    logits, f2 = forward(g, batch, mask)
    C = logits.shape[1]
    cw = np.ones(C) if class_weights is None else class_weights
    out = {"logits": logits.detach().numpy(), "feat32": f2.detach().numpy(), "stats": g.stats, "signs": g.signs, "ties": g.ties, "pre": g.pre, "pooled": g.pooled, "P": P}
    if "labels" in batch:
        loss, acc, n = loss_and_accuracy(logits, batch["labels"], batch["act"], batch["pse"], cw, ignored, C)
        out.update(loss=float(loss.detach()), acc=float(acc), valid=n)
        if want_grad:
            loss.backward()
            out["grads"] = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in P.items() if v.requires_grad}
    return out


def moving_update(weights, stats):
    """the UPDATE_OPS of one training step: moving -= (moving - batch) * (1 - 0.99); the variance the fused (rank-4) path feeds is the batch
    variance times n / (n - 1), fc0 (tf.layers.dense output, rank 3: not fused) feeds the biased one.  Returns {scope: (mean, var)} float64."""
    out = {}
    for name, (mu, var, n) in stats.items():
        m0, v0 = (np.asarray(a, np.float64) for a in weights[name]["bn"][2:])
        v = var.numpy().astype(np.float64) * (1.0 if name == "fc0" or n < 2 else n / (n - 1.0))
        out[name] = (m0 - (m0 - mu.numpy().astype(np.float64)) * (1 - MOMENTUM), v0 - (v0 - v) * (1 - MOMENTUM))
    return out


def adam_np(p, g, m, v, t, lr, dtype=np.float32):
    """tf.train.AdamOptimizer at step t (1-based), in `dtype`: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); m, v as TF's assign ops;
    p -= lr_t m / (sqrt(v) + 1e-8).  Returns (p, m, v, lr_t)."""
    f = dtype
    lr_t = f(float(lr) * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t))
    m = (m + (g - m) * f(1 - 0.9)).astype(f)
    v = (v + (g * g - v) * f(1 - 0.999)).astype(f)
    p = (p - lr_t * m / (np.sqrt(v) + f(1e-8))).astype(f)
    return p, m, v, lr_t


def train_steps(weights, batches, masks, lr, class_weights=None, ignored=(), dtype=torch.float64):
    """plain training loop of the oracle (Adam from zero moments): returns (losses, final weights dict in float64 NumPy)"""
    import copy
    W = copy.deepcopy(weights)
    mom = {}
    losses = []
    for t, (batch, mask) in enumerate(zip(batches, masks), 1):
        r = run(W, batch, mask, class_weights, ignored, dtype)
        losses.append(r["loss"])
        mv = moving_update(W, r["stats"])
        for (name, key), g in r["grads"].items():
            ent = W[name]
            cur = np.asarray(ent[key] if key in ("W", "b") else ent["bn"][("gamma", "beta").index(key)], np.float64)
            m, v = mom.get((name, key), (np.zeros_like(cur), np.zeros_like(cur)))
            cur, m, v, _ = adam_np(cur, np.asarray(g, np.float64), m, v, t, lr, np.float64)
            mom[(name, key)] = (m, v)
            if key in ("W", "b"):
                ent[key] = cur
            else:
                bn = list(ent["bn"]); bn[("gamma", "beta").index(key)] = cur; ent["bn"] = tuple(bn)
        for name, (mu, var) in mv.items():
            bn = list(W[name]["bn"]); bn[2], bn[3] = mu, var; W[name]["bn"] = tuple(bn)
    return losses, W
