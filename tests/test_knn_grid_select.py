"""The grid first pass's selection (grid_mark_select, csrc/knn_grid.hip): one loop over a lane's marks across all rows of cells,
records fetched ahead of the sorted insertion.  Every case is compared with the oracle bit for bit: K = 16 on the cloud itself, K = 1
from a prefix of the cloud (the fused prefix job of a pyramid asks the same question) and a two-level pyramid."""
import numpy as np
import pytest

from conftest import assert_bits_equal

B, N = 2, 2048
RATIOS = [4, 4]
CASES = ["uniform", "layered", "dense_clump", "isolated", "lattice", "too_few"]


def _cloud(case, b):
    rng = np.random.default_rng(1000 * CASES.index(case) + b)
    box = np.array([4.0, 3.0, 2.0])
    if case == "uniform":                  # marks spread over all nine rows of cells
        p = rng.random((N, 3)) * box
    elif case == "layered":                # lanes of one wave whose marks sit in different rows: three thin z-layers, very different density
        sizes = [1500, 450, N - 1950]
        p = np.concatenate([np.concatenate([rng.random((m, 2)) * box[:2], z + 0.01 * rng.random((m, 1))], 1)
                            for m, z in zip(sizes, (0.0, 0.35, 0.9))])
    elif case == "dense_clump":            # the masks cannot hold a row of more than 64 candidates (streaming retry): 300 points in a cube of 1e-3,
                                           # far below any cell size a 2 048-point cloud in this box gets, share one cell, so one row of three cells
        p = rng.random((N, 3)) * box
        p[:300] = box * 0.5 + 1e-3 * rng.random((300, 3))
    elif case == "isolated":               # fewer than K + 1 marks in the 3^3 block (5^3 / 7^3 shells, the prefix job answered from a few marks): the
                                           # groups of 5 points at the corners are fewer than 17 and the core is far more than a cell away
        p = box * 0.5 + 0.15 * rng.random((N, 3))
        corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float64) * box
        p[:40] = np.repeat(corners, 5, 0) + 0.05 * rng.random((40, 3))
    elif case == "lattice":                # equal distances: the rows go to the tree
        g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
        p = g * 0.05
    elif case == "too_few":                # fewer support points than K + 1
        p = rng.random((12, 3)) * box
    return p[rng.permutation(len(p))].astype(np.float32)      # a pyramid's levels are prefixes of the cloud


_cache = {}


def _case(case, orc):
    """input and oracle answers of a case, computed once for both backends"""
    if case not in _cache:
        p = np.stack([_cloud(case, b) for b in range(B)])
        n = p.shape[1]
        ref = {"p": p, "self16": orc.knn_batch(p, p, 16, threads=4), "up1": orc.knn_batch(p[:, : n // 4], p, 1, threads=4),
               "neigh": [], "interp": []}
        cur = p
        for r in RATIOS:
            nxt = cur[:, : cur.shape[1] // r]
            ref["neigh"].append(orc.knn_batch(cur, cur, 16, threads=4).astype(np.int32))
            ref["interp"].append(orc.knn_batch(nxt, cur, 1, threads=4).astype(np.int32))
            cur = nxt
        _cache[case] = ref
    return _cache[case]


def _grid_share(p, idx17):
    """share of rows that cannot go to the tree hand-over by rule: their 17 nearest float32 distances are pairwise distinct and the
    16th and 17th differ by more than 2^-19 relative (the reference's arithmetic: (dx*dx + dy*dy) + dz*dz, no FMA)"""
    ok = 0
    for b in range(p.shape[0]):
        d = p[b][:, None, :] - p[b][idx17[b]]
        d2 = np.sort((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], axis=1)
        assert d2.dtype == np.float32
        ok += int(((np.diff(d2, axis=1) > 0).all(1) & (d2[:, 16] > d2[:, 15] * np.float32(1 + 2.0 ** -19))).sum())
    return ok / float(p.shape[0] * p.shape[1])


@pytest.mark.parametrize("case", CASES)
def test_grid_selection_matches_oracle(backend, orc, case):
    from ssdr_al import knn
    ref = _case(case, orc)
    p = ref["p"]
    n = p.shape[1]
    if case in ("uniform", "layered"):     # the case must not pass by sending everything to the tree
        share = _grid_share(p, orc.knn_batch(p, p, 17, threads=4))
        print("%s: share of rows the grid must answer %.3f" % (case, share))
        assert share >= 0.9
    assert_bits_equal(knn.knn_batch(p, p, 16), ref["self16"], case + " K=16")
    assert_bits_equal(knn.knn_batch(p[:, : n // 4], p, 1), ref["up1"], case + " K=1 from the prefix")
    neigh, sub, interp = knn.knn_pyramid(p, RATIOS, 16)
    for i in range(len(RATIOS)):
        assert_bits_equal(neigh[i], ref["neigh"][i], "%s pyramid level %d neigh" % (case, i))
        assert_bits_equal(sub[i], ref["neigh"][i][:, : sub[i].shape[1]], "%s pyramid level %d sub" % (case, i))
        assert_bits_equal(interp[i], ref["interp"][i], "%s pyramid level %d interp" % (case, i))
