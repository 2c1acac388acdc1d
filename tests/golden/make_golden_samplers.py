"""Golden vectors for the seed, random and label-all rounds, produced by the reference's OWN sampler2.SeedSampler / RandomSampler / AllSampler imported
from /root/reference (build container only):  python tests/golden/make_golden_samplers.py

The stand-in modules are make_golden_labeling.py's (only so that `import sampler2` succeeds).  Every case lays a temporary directory out as the reference
expects it (io_formats: <data>/superpoint/{cloud}.superpoint, {cloud}.gt, total.pkl; <input>/{cloud}.ply) and runs three stages on it, each after its
own np.random.seed: SeedSampler._iteration, RandomSampler._iteration on what the seed left, AllSampler.sampling on what the random round left.  Stored per
stage: pseudo_gt of every cloud, every cloud's final `unlabeled` list (in the reference's order), selected_class_list, w and the final budget."""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/SSDR_AL_s3dis"
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "ssdr-al_amd"))
COUNTERS = ("sp_num", "p_num", "sub_num", "sub_p_num", "split_sp_num", "ignore_sp_num")

# (regions per cloud, region sizes, seeds to place, random clicks, min_size, mode, threshold, label-all clicks, np.random seeds of the three stages)
CASES = [([12, 1, 60, 3, 35], (1, 40), 40, 30, 5, "dominant", 0.9, 12, (11, 12, 13)),
         ([30, 2, 45, 1, 8, 20], (1, 25), 36, 40, 4, "dominant", 0.9, 1000, (21, 22, 23)),
         ([9, 1, 50, 25], (2, 60), 20, 25, 6, "NAIL", 0.0, 9, (31, 32, 33)),
         ([4, 57, 1, 16, 2], (1, 30), 12, 50, 3, "dominant", 0.9, 5, (41, 42, 43))]


def _stub(name):
    m = types.ModuleType(name)
    sys.modules[name] = m
    return m


def _import_reference():
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
    return sampler2


def _state(g, p, names, cur, total, w, budget):
    """what a stage left on disk and in total_obj / w"""
    from ssdr_al import io_formats
    g[p + "pseudo"] = np.concatenate([io_formats.load_gt(os.path.join(cur, n + ".gt")) for n in names], axis=1).astype(np.float32)
    lists = [np.asarray(total["unlabeled"].get(n, []), np.int32).reshape(-1) for n in names]
    g[p + "unl"] = np.concatenate(lists) if lists else np.zeros(0, np.int32)
    g[p + "unl_off"] = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    g[p + "unl_live"] = np.array([n in total["unlabeled"] for n in names], np.uint8)
    g[p + "class_list"] = np.asarray(total.get("selected_class_list", []), np.int32)
    g[p + "w"] = np.array([w[c] for c in COUNTERS], np.int64)
    g[p + "budget"] = np.int64(budget)


def main():
    sampler2 = _import_reference()
    from _labeling_oracle import noisy_cloud
    from ssdr_al import io_formats
    rng = np.random.default_rng(2025)
    g = {}
    for k, (regions, (lo, hi), number, clicks, min_size, mode, thr, all_clicks, seeds) in enumerate(CASES):
        p = "c%d/" % k
        clouds = [noisy_cloud(rng, rng.integers(lo, hi + 1, n)) for n in regions]
        names = ["cloud_%d" % i for i in range(len(clouds))]
        total_num = int(sum(regions))
        with tempfile.TemporaryDirectory() as tmp:
            data, inp = os.path.join(tmp, "data"), os.path.join(tmp, "input")
            cur = os.path.join(data, "superpoint")
            os.makedirs(cur); os.makedirs(inp)
            for n, c in zip(names, clouds):
                npts = len(c["gt"])
                in_comp = np.zeros(npts, np.int32)
                for s, ids in enumerate(c["components"]):
                    in_comp[ids] = s
                io_formats.save_superpoint(os.path.join(cur, n + ".superpoint"), c["components"], in_comp)
                io_formats.save_gt(os.path.join(cur, n + ".gt"), np.zeros((2, npts), np.float32))
                xyz = rng.random((npts, 3)).astype(np.float32)
                io_formats.write_ply(os.path.join(inp, n + ".ply"), [xyz, np.zeros((npts, 3), np.uint8), c["gt"].astype(np.int32)], ["x", "y", "z", "red", "green", "blue", "class"])
            total = io_formats.new_total({n: c["components"] for n, c in zip(names, clouds)})
            io_formats.save_total(os.path.join(cur, "total.pkl"), total)
            g[p + "regions"] = np.asarray(regions, np.int32)
            g[p + "offsets"] = np.concatenate([c["offsets"] for c in clouds]).astype(np.int32)      # every cloud's own CSR, one after the other
            g[p + "points"] = np.concatenate([c["points"] for c in clouds]).astype(np.int32)
            g[p + "gt"] = np.concatenate([c["gt"] for c in clouds]).astype(np.int32)
            g[p + "pred"] = np.concatenate([c["pred"] for c in clouds]).astype(np.int32)
            g[p + "params"] = np.array([number, clicks, min_size, 0 if mode == "dominant" else 1, all_clicks, total_num] + list(seeds), np.int64)
            g[p + "threshold"] = np.float64(thr)
            # stage 1: the seed
            w = dict.fromkeys(COUNTERS, 0)
            np.random.seed(seeds[0])
            sampler2.SeedSampler(inp, data, total_num, [mode])._iteration(current_path=cur, total_obj=total, number=number, w=w)
            _state(g, p + "seed/", names, cur, total, w, 0)
            print("case", k, "seed: sp_num", w["sp_num"], "left", sum(len(v) for v in total["unlabeled"].values()))
            # stage 2: the random round on what the seed left
            w = dict.fromkeys(COUNTERS, 0)
            total["selected_class_list"] = []
            budget = {"click": clicks}
            np.random.seed(seeds[1])
            sampler2.RandomSampler(inp, data, total_num, [mode], min_size)._iteration(current_path=cur, total_obj=total, w=w, threshold=thr, budget=budget)
            _state(g, p + "random/", names, cur, total, w, budget["click"])
            print("case", k, "random:", [w[c] for c in COUNTERS], "budget", budget["click"], "left", sum(len(v) for v in total["unlabeled"].values()))
            # stage 3: label-all on what the random round left (sampling() copies <data>/superpoint to round_2 and reads total.pkl there)
            w = dict.fromkeys(COUNTERS, 0)
            np.random.seed(seeds[2])
            sampler2.AllSampler(inp, data, total_num, [mode]).sampling(None, all_clicks, 1, w, thr)
            nxt = os.path.join(data, "sampling", sampler2.get_sampler_args_str([mode]), "round_2")
            total = io_formats.load_total(os.path.join(nxt, "total.pkl"))
            assert w["sub_num"] == w["split_sp_num"] == w["ignore_sp_num"] == 0      # (sampling() keeps its budget to itself: every click here is one sp_num)
            left = all_clicks - w["sp_num"]
            _state(g, p + "all/", names, nxt, total, w, left)
            print("case", k, "all:", [w[c] for c in COUNTERS], "left", sum(len(v) for v in total["unlabeled"].values()))
    g["n_cases"] = np.int64(len(CASES))
    path = os.path.join(HERE, "samplers_golden.npz")
    np.savez_compressed(path, **g)
    print("samplers_golden.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
