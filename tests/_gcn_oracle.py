"""Float64 oracle of the trained-GCN selector's middle (gcn.py:60-86, :207-245): a torch autograd restatement with explicit initial weights and
explicit dropout masks, and the NumPy restatement of the library's counter-based dropout function (include/ssdr_al.h)."""
import numpy as np

NHID, NFEAT, NPARAM = 128, 32, 4353
M64 = (1 << 64) - 1


def dropout_keep(seed, step, rows, p):
    """keep[r, k] for the rows `rows` (indices in the [unlabelled | labelled] order) at step `step` (0-based): include/ssdr_al.h's function"""
    rows = np.asarray(rows, np.uint64).reshape(-1, 1)
    k = np.arange(NHID, dtype=np.uint64).reshape(1, -1)
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & M64) + np.uint64(0x9E3779B97F4A7C15) * np.uint64(step + 1) + np.uint64(0xD6E8FEB86659FD93) * (rows * np.uint64(128) + k + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u >= np.float32(p)


def split(params):
    p = np.asarray(params)
    return p[:4096].reshape(NFEAT, NHID), p[4096:4224], p[4224:4352].reshape(NHID, 1), p[4352:4353]


def dense_adj(blocks, rows, N, dtype=np.float64):
    """the [N,N] matrix of the blocks: rows[g] = the row of grouped position g"""
    A = np.zeros((N, N), dtype)
    g = 0
    for b in blocks:
        n = len(b)
        r = np.asarray(rows[g:g + n])
        A[np.ix_(r, r)] = b
        g += n
    return A


def train(V, A, n_unl, init, steps, p, seed, lr=1e-3, weight_decay=5e-4, lamda=1.2, dtype="float64", record=()):
    """The reference's loop statement for statement in `dtype`, with F.dropout replaced by the explicit mask dropout_keep gives.
    Returns ({step count: parameters}, loss at step 0, the final parameters)."""
    import torch
    dt = getattr(torch, dtype)
    V = torch.tensor(np.asarray(V), dtype=dt); A = torch.tensor(np.asarray(A), dtype=dt)
    N = V.shape[0]
    W1, b1, W3, b3 = [torch.tensor(np.array(x), dtype=dt, requires_grad=True) for x in split(np.asarray(init, np.float64))]
    opt = torch.optim.Adam([W1, b1, W3, b3], lr=lr, weight_decay=weight_decay)
    lbl = np.arange(n_unl, N); nlbl = np.arange(0, n_unl)
    out, loss0 = {}, None
    for t in range(steps):
        opt.zero_grad()
        h = torch.relu(torch.mm(A, torch.mm(V, W1)) + b1)
        if p > 0:
            h = h * torch.tensor(dropout_keep(seed, t, np.arange(N), p).astype(np.float64) / (1.0 - np.float64(np.float32(p))), dtype=dt)
        x = torch.mm(A, torch.mm(h, W3)) + b3
        s = torch.sigmoid(x)
        loss = -torch.mean(torch.log(s[lbl])) - lamda * (torch.mean(torch.log(1 - s[nlbl])) if n_unl else 0.0)
        if t == 0:
            loss0 = float(loss.detach())
        loss.backward()
        opt.step()
        if t + 1 in record:
            out[t + 1] = np.concatenate([x.detach().numpy().reshape(-1) for x in (W1, b1, W3, b3)])
    return out, loss0, np.concatenate([x.detach().numpy().reshape(-1) for x in (W1, b1, W3, b3)])


def evaluate(V, A, params, dtype=np.float64):
    """cat(relu(A (V W1) + b1), A (feat W3) + b3) without dropout, and the loss terms' x"""
    W1, b1, W3, b3 = [np.asarray(x, dtype) for x in split(params)]
    V = np.asarray(V, dtype); A = np.asarray(A, dtype)
    feat = np.maximum(A @ (V @ W1) + b1, 0)
    x = A @ (feat @ W3) + b3
    return np.concatenate([feat, x], axis=1)


def loss_of(rows129, n_unl, lamda=1.2):
    x = rows129[:, 128]
    s = 1.0 / (1.0 + np.exp(-x))
    return float(-np.mean(np.log(s[n_unl:])) - (lamda * np.mean(np.log(1 - s[:n_unl])) if n_unl else 0.0))
