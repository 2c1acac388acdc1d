"""Golden vectors for the oracle labelling, produced by the reference's OWN sampler2.oracle_labeling imported from /root/reference
(build container only):  python tests/golden/make_golden_labeling.py

Modules the image lacks and the reference's compiled ops are replaced by empty stand-in modules ONLY so that `import sampler2` succeeds (the
stand-ins of make_golden_select.py); oracle_labeling touches none of them.  Every case stores its inputs (superpoints as CSR, ground truth,
predicted classes, the picks, pseudo_gt before) and every output (pseudo_gt after, used list, appended class list, counters, final budget)."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/SSDR_AL_s3dis"
sys.path.insert(0, os.path.dirname(HERE))
COUNTERS = ("sp_num", "p_num", "sub_num", "sub_p_num", "split_sp_num", "ignore_sp_num")


def _stub(name):
    m = types.ModuleType(name)
    sys.modules[name] = m
    return m


def main():
    np.float = float
    for n in ("open3d", "open3d.linux", "torchvision", "torchvision.transforms", "PIL", "PIL.Image", "cpp_wrappers", "cpp_wrappers.cpp_subsampling",
              "cpp_wrappers.cpp_subsampling.grid_subsampling", "nearest_neighbors", "nearest_neighbors.lib",
              "nearest_neighbors.lib.python", "nearest_neighbors.lib.python.nearest_neighbors"):
        _stub(n)
    sys.modules["open3d"].linux = sys.modules["open3d.linux"]
    sys.modules["torchvision.transforms"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["PIL"].Image = sys.modules["PIL.Image"]
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "utils"))
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        import sampler2
    finally:
        os.chdir(cwd)
    from _labeling_oracle import noisy_cloud
    rng = np.random.default_rng(2024)
    g = {}
    # (mode, regions, size range, picks, budget, min_size, threshold)
    cases = [("dominant", 60, (1, 70), 40, 25, 5, 0.9), ("dominant", 30, (3, 40), 30, 100, 1, 0.9),
             ("NAIL", 80, (1, 90), 60, 45, 5, 0.9), ("NAIL", 50, (10, 300), 50, 200, 8, 0.8),
             ("NAIL", 40, (2, 60), 40, 7, 3, 0.95), ("NAIL", 25, (20, 700), 25, 12, 10, 0.9)]
    for k, (mode, nsp, (lo, hi), npick, budget, min_size, thr) in enumerate(cases):
        cl = noisy_cloud(rng, rng.integers(lo, hi + 1, nsp))
        comps = np.empty(nsp, dtype=object)
        for s in range(nsp):
            comps[s] = list(cl["components"][s])
        n = len(cl["gt"])
        inds = rng.choice(nsp, npick, replace=npick > nsp).tolist()
        inds[3] = inds[0]                                   # a region picked twice
        pseudo = np.zeros((2, n), np.float32)
        pseudo[:, rng.random(n) < 0.1] = np.array([[1.0], [7.0]], np.float32)      # labels of earlier rounds
        w = dict.fromkeys(COUNTERS, 0)
        b = {"click": budget}
        total = {"selected_class_list": [3, 1]}
        p = "c%d/" % k
        g[p + "offsets"], g[p + "points"], g[p + "gt"], g[p + "pred"] = cl["offsets"], cl["points"], cl["gt"], cl["pred"]
        g[p + "inds"], g[p + "pseudo_in"] = np.asarray(inds, np.int32), pseudo.copy()
        g[p + "params"] = np.array([0 if mode == "dominant" else 1, budget, min_size], np.int64); g[p + "threshold"] = np.float64(thr)
        out, used = sampler2.oracle_labeling(superpoint_inds=inds, components=comps, input_gt=cl["gt"], pseudo_gt=pseudo, cloud_name="c", w=w,
                                             sampler_args=[mode], prob_class=cl["pred"], threshold=thr, budget=b, min_size=min_size, total_obj=total)
        g[p + "pseudo_out"] = np.asarray(out, np.float32)
        g[p + "used"] = np.asarray(used, np.int32)
        g[p + "class_list"] = np.asarray(total["selected_class_list"], np.int32)
        g[p + "counters"] = np.array([w[c] for c in COUNTERS], np.int64)
        g[p + "budget_left"] = np.int64(b["click"])
        print(mode, "used", len(used), "counters", [w[c] for c in COUNTERS], "left", b["click"])
    g["n_cases"] = np.int64(len(cases))
    path = os.path.join(HERE, "labeling_golden.npz")
    np.savez_compressed(path, **g)
    print("labeling_golden.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
