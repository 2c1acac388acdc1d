"""Golden vectors for the trained-GCN branch's training loop, produced by the reference's OWN gcn.GCN, BCEAdjLoss and torch.optim.Adam imported from
/root/reference (build container only):  python tests/golden/make_golden_gcn_train.py

Graph: gcn_golden.npz (the reference's create_adj on the 70 + 60 superpoint fixture: 100 candidates + 30 labelled rows).  As in make_golden_gcn.py
`.cuda(...)` is made the identity on tensors and modules (no CUDA device in the build container): the arithmetic is torch float32 on the CPU.  The one
replacement is F.dropout, by the explicit-mask form x * mask * (1 / (1 - p)) with the library's counter-based mask (tests/_gcn_oracle.dropout_keep), so
that the device can be given the same masks.  Recorded: the initial parameters, the parameters after 1 / 10 / 100 steps for p = 0 and p = 0.3 and the
evaluation rows (gcn.py:230-232, before the NaN / inf substitution) after 100.

The initial weights: on this graph (|adj| up to 16: float32 column sums near 0) every one of 1 000 draws of W3 and b3 from reset_parameters' +-1 saturates
a float32 sigmoid to exactly 1 on an unlabelled row, log(1 - s) is -inf and the reference's autograd multiplies it by 0: every parameter is NaN after
the first step.  Such a run says nothing about the arithmetic, so W3 and b3 are drawn from +-W3_SCALE instead (W1 and b1 as reset_parameters draws
them), and the generator takes the first seed from SEED0 upwards whose run stays finite for both dropout rates, and records it."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/SSDR_AL_s3dis"
SEED0, STEPS, W3_SCALE = 20240229, (1, 10, 100), 0.1


def main():
    import torch
    np.float = float
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    sys.path.insert(0, REF); sys.path.insert(0, os.path.join(REF, "utils")); sys.path.insert(0, os.path.dirname(HERE))
    cwd = os.getcwd(); os.chdir(REF)
    try:
        import gcn
    finally:
        os.chdir(cwd)
    import _gcn_oracle as O
    G = np.load(os.path.join(HERE, "gcn_golden.npz")); S = np.load(os.path.join(HERE, "select_golden.npz"))
    V, adj = torch.tensor(G["featuresV"]), torch.tensor(G["adj"])
    n_unl, N = len(S["g/unl_feat"]), len(G["featuresV"])
    for seed in range(SEED0, SEED0 + 1000):
        out = run(gcn, torch, O, V, adj, n_unl, N, seed)
        if all(np.isfinite(v).all() for v in out.values()):
            break
        print("seed", seed, "not finite in the reference")
    else:
        raise SystemExit("no seed with a finite reference run")
    path = os.path.join(HERE, "gcn_train_golden.npz")
    np.savez_compressed(path, **out)
    print("gcn_train_golden.npz", os.path.getsize(path) // 1024, "KiB, seed", seed)


def run(gcn, torch, O, V, adj, n_unl, N, SEED):
    rng = np.random.RandomState(SEED)
    s = 1.0 / np.sqrt(128.0)
    init = np.concatenate([rng.uniform(-s, s, 32 * 128), rng.uniform(-s, s, 128), rng.uniform(-W3_SCALE, W3_SCALE, 128), rng.uniform(-W3_SCALE, W3_SCALE, 1)]).astype(np.float32)
    out = {"init": init, "seed": np.int64(SEED), "n_unl": np.int64(n_unl)}
    state = {"step": 0, "p": 0.0}

    def dropout(x, p, training=True):
        if not training or p <= 0:
            return x
        keep = O.dropout_keep(SEED, state["step"], np.arange(N), p)
        return x * torch.tensor(keep.astype(np.float32)) * torch.tensor(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    gcn.F.dropout = dropout
    for p in (0.0, 0.3):
        m = gcn.GCN(nfeat=32, nhid=128, nclass=1, dropout=p, gcn_gpu=0)
        W1, b1, W3, b3 = O.split(init)
        with torch.no_grad():
            m.gc1.weight.copy_(torch.tensor(W1)); m.gc1.bias.copy_(torch.tensor(b1)); m.gc3.weight.copy_(torch.tensor(W3)); m.gc3.bias.copy_(torch.tensor(b3))
        opt = gcn.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-4)
        lbl = np.arange(n_unl, N); nlbl = np.arange(0, n_unl)
        for bb in range(max(STEPS)):
            state["step"] = bb
            opt.zero_grad()
            outputs, _, _ = m(V, adj)
            loss = gcn.BCEAdjLoss(outputs, lbl, nlbl, 1.2, gcn_gpu=0)
            loss.backward()
            opt.step()
            if bb + 1 in STEPS:
                out["p%02d/w%d" % (int(p * 10), bb + 1)] = np.concatenate([t.detach().numpy().reshape(-1) for t in (m.gc1.weight, m.gc1.bias, m.gc3.weight, m.gc3.bias)])
        m.eval()
        with torch.no_grad():
            _, _, feat = m(V, adj)
        out["p%02d/eval100" % int(p * 10)] = feat.numpy()
    return out


if __name__ == "__main__":
    main()
