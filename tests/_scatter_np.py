"""TEST INFRASTRUCTURE ONLY — NumPy float32 restatement of the deterministic backward scatters (csrc/scatter_det.hip), bit for bit: a stable
argsort of (b, clamp(idx)) gives every source row its positions in ascending order, then ONE sequential pass adds the rows in float32
(s = +0; s = s + term; finally dsrc = dsrc + s for the rows that have a list).  No pairwise or blocked summation anywhere: np.add on float32
scalars / rows rounds once per addition, like the kernels."""
import numpy as np


def row_keys(idx, src_rows):
    """idx [B, rows_per_b] -> q = b * src_rows + clamp(idx) per position, flat"""
    idx = np.asarray(idx)
    B = idx.shape[0]
    j = np.clip(idx.reshape(B, -1).astype(np.int64), 0, src_rows - 1)
    return (np.arange(B, dtype=np.int64)[:, None] * src_rows + j).reshape(-1)


def inverse_lists(idx, src_rows):
    """(off [B src_rows + 1], order): order[off[q]:off[q + 1]] are the flat positions of row q, ascending"""
    q = row_keys(idx, src_rows)
    order = np.argsort(q, kind="stable")
    off = np.searchsorted(q[order], np.arange(np.asarray(idx).shape[0] * src_rows + 1))
    return off, order


def scatter_add_rows(idx, src_rows, dout, dsrc):
    """dout [B rows_per_b, C], dsrc [B src_rows, C] float32 -> the new dsrc"""
    dout, out = np.asarray(dout, np.float32), np.array(dsrc, np.float32, copy=True)
    q = row_keys(idx, src_rows)
    s = np.zeros_like(out)
    for p in np.argsort(q, kind="stable"):               # ascending q, inside a row ascending position
        s[q[p]] = s[q[p]] + dout[p]
    hit = np.unique(q)
    out[hit] = out[hit] + s[hit]
    return out


def pool_ties(src, idx, src_rows, out):
    """tied [B m_per_b * 16, C]: the position's source value equals the pooled maximum; ties [B m_per_b, C]: their count per point"""
    q = row_keys(idx, src_rows)
    tied = np.asarray(src, np.float32)[q] == np.repeat(np.asarray(out, np.float32), 16, axis=0)
    return tied, tied.reshape(-1, 16, tied.shape[1]).sum(1)


def pool_forward(src, idx, src_rows):
    q = row_keys(idx, src_rows)
    return np.asarray(src, np.float32)[q].reshape(-1, 16, np.asarray(src).shape[1]).max(1)


def pool_grad_rows(src, idx, src_rows, out, dout, dsrc):
    """src / dsrc [B src_rows, C], idx [B, m_per_b, 16], out / dout [B m_per_b, C] -> the new dsrc"""
    res = np.array(dsrc, np.float32, copy=True)
    q = row_keys(idx, src_rows)
    tied, ties = pool_ties(src, idx, src_rows, out)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.asarray(dout, np.float32) / ties.astype(np.float32)          # one correctly rounded float32 division
    s = np.zeros_like(res)
    for p in np.argsort(q, kind="stable"):
        t = tied[p]
        s[q[p]][t] = s[q[p]][t] + share[p // 16][t]
    hit = np.unique(q)
    res[hit] = res[hit] + s[hit]
    return res
