"""Worker of tests/test_knn_paths.py for the switches that are static and read once per process (SSDR_KNN_LDS in csrc/knn_grid.hip: grid_search,
SSDR_KD_LEVELS in csrc/kdtree.hip: launch_build).  Arguments: the library to bind (the gfx950 build or the CPU logic build) and the mode.
  clouds   the six clouds of test_knn_grid_select.py (K = 16 on the cloud, K = 1 from its first quarter, the pyramid [4, 4]) and the padded pyramid
           [4, 4, 2] of _knn_paths.py
  rebuild  the first tile of test_knn.py::test_complete_rebuild_of_several_large_trees_in_one_launch, pyramid [4, 4, 4, 4, 2]
One line per case, "CASE name sha256-of-the-results counters...", the counters being [8] for `rebuild` and [0], [1], [3], [4], [5] of every call for
`clouds`; the process stops at the first call that fails."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ssdr-al_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from ssdr_al import _lib, knn  # noqa: E402
import _knn_paths as P  # noqa: E402

_lib.use(sys.argv[1])


def words(c):
    return [int(c[i]) for i in (0, 1, 3, 4, 5)]


def clouds():
    import test_knn_grid_select as G
    for case in G.CASES:
        p = np.stack([G._cloud(case, b) for b in range(G.B)])
        n = p.shape[1]
        ctr = []
        a = knn.knn_batch(p, p, 16); ctr += words(knn.knn_counters())
        b = knn.knn_batch(p[:, : n // 4], p, 1); ctr += words(knn.knn_counters())
        neigh, sub, interp = knn.knn_pyramid(p, G.RATIOS, 16); ctr += words(knn.knn_counters())
        yield case, a.tobytes() + b.tobytes() + b"".join(x.tobytes() for x in neigh + interp), ctr
    p = np.stack([P.padded_lattice(s) for s in (21, 22)])
    neigh, sub, interp = knn.knn_pyramid(p, [4, 4, 2], 16)
    yield "padded_pyramid", b"".join(x.tobytes() for x in neigh + interp), words(knn.knn_counters())


def rebuild():
    rng = np.random.default_rng(77)
    B, N = 4, 40960
    xyz = (rng.random((B, N, 3), dtype=np.float32) * np.array([9, 7, 3], np.float32)).astype(np.float32)
    for b in range(B):
        xyz[b, -6 - 2 * b:] = xyz[b, : 6 + 2 * b]
        xyz[b] = xyz[b][rng.permutation(N)]
    neigh, sub, interp = knn.knn_pyramid(xyz[:1], [4, 4, 4, 4, 2], 16)
    yield "rebuild", b"".join(x.tobytes() for x in neigh + interp), [int(knn.knn_counters()[8])]


it = {"clouds": clouds, "rebuild": rebuild}[sys.argv[2]]()
while True:
    try:
        name, data, ctr = next(it)
    except StopIteration:
        break
    except Exception as e:          # a call that reported a failure: nothing more on the device from this process
        print("CASE failed:", e, flush=True)
        sys.exit(0)
    print("CASE", name, hashlib.sha256(data).hexdigest(), *ctr, flush=True)
