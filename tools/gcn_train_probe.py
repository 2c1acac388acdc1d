#!/usr/bin/env python3
"""The trained-GCN selector at the round's scale: 272 clouds, 20 000 candidates + 4 000 labelled rows, 20 000 Adam steps — train +
evaluate + k-center in both forms, against the reference's dense formulation in torch on the same GPU (100 steps on the [N,N] matrix, scaled to the
step count and labelled as scaled).  Prints one JSON line.  (tools/gcn_probe.py is the older probe of the gcn_fps graph variants.)"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "ssdr-al_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--clouds", type=int, default=272); ap.add_argument("--unl", type=int, default=20000); ap.add_argument("--lab", type=int, default=4000)
ap.add_argument("--steps", type=int, default=20000); ap.add_argument("--picks", type=int, default=10000); ap.add_argument("--dense-steps", type=int, default=100)
ap.add_argument("--lib", default=None); ap.add_argument("--no-dense", action="store_true")
a = ap.parse_args()
from ssdr_al import _lib, sampler
if a.lib:
    _lib.use(a.lib)
rng = np.random.default_rng(0)
N = a.unl + a.lab
cuts = np.sort(rng.choice(np.arange(1, N // 2), a.clouds - 1, replace=False)) * 2          # every cloud at least two rows
counts = np.diff(np.concatenate([[0], cuts, [N]]))
blocks = [(np.eye(n) + (rng.random((n, n)) - 0.4) * (0.8 / np.sqrt(n))).astype(np.float32) for n in counts]
rows = rng.permutation(N).astype(np.int32)
V = rng.standard_normal((N, 32)).astype(np.float32); V /= np.linalg.norm(V, axis=1, keepdims=True)
G = sampler.GcnGraph.from_blocks(V, blocks, rows, a.unl)
init = sampler.gcn_init_params(0); init[4224:] *= 0.1
out = dict(clouds=a.clouds, rows=N, n_max=int(counts.max()), steps=a.steps, picks=a.picks)
for form in ("general", "fused"):
    if form == "fused" and counts.max() > sampler.GCN_FUSED_CAP:
        continue
    G.train(init, 10, form=form)                                                                  # warm the scratch
    t0 = time.perf_counter(); par, loss, info = G.train(init, a.steps, form=form); t1 = time.perf_counter()
    feat, _ = G.evaluate(par); t2 = time.perf_counter()
    picks = sampler.kCenterGreedy(feat[:N]).select_batch_(np.arange(a.unl, N), a.picks); t3 = time.perf_counter()
    out[form] = dict(train_s=round(t1 - t0, 4), us_per_step=round((t1 - t0) / max(a.steps, 1) * 1e6, 2), eval_s=round(t2 - t1, 4), kcenter_s=round(t3 - t2, 4),
                     loss=[float(x) for x in loss])
if not a.no_dense:
    import torch
    import _gcn_oracle as O
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    A = torch.tensor(O.dense_adj(blocks, rows, N, np.float32), device=dev); Vt = torch.tensor(V, device=dev)
    W1, b1, W3, b3 = [torch.tensor(np.array(x), device=dev, requires_grad=True) for x in O.split(init)]
    opt = torch.optim.Adam([W1, b1, W3, b3], lr=1e-3, weight_decay=5e-4)
    lbl = torch.arange(a.unl, N, device=dev); nlbl = torch.arange(0, a.unl, device=dev)

    def step():
        opt.zero_grad()
        h = torch.nn.functional.dropout(torch.relu(torch.mm(A, torch.mm(Vt, W1)) + b1), 0.3)
        s = torch.sigmoid(torch.mm(A, torch.mm(h, W3)) + b3)
        (-torch.mean(torch.log(s[lbl])) - 1.2 * torch.mean(torch.log(1 - s[nlbl]))).backward()
        opt.step()
    for _ in range(3):
        step()
    if dev == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.dense_steps):
        step()
    if dev == "cuda":
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out["dense_torch"] = dict(device=dev, steps_timed=a.dense_steps, us_per_step=round(dt / a.dense_steps * 1e6, 1), train_s_scaled_to_steps=round(dt / a.dense_steps * a.steps, 2), scaled=True)
print(json.dumps(out))
