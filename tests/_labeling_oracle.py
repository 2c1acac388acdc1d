"""TEST INFRASTRUCTURE ONLY — a NumPy restatement of oracle_labeling (sampler2.py:124-192) and of the order sampling() calls _help() in
(:676-684, :796-806, fps_gcn_cpu.py:172-178), pinned against the reference's own function by tests/golden/labeling_golden.npz
(test_oracle_labeling.py::test_numpy_oracle_equals_reference_golden).  The device tests compare against this."""
import numpy as np

COUNTERS = ("sp_num", "p_num", "sub_num", "sub_p_num", "split_sp_num", "ignore_sp_num")


def dominant_label(ary):
    """_dominant_label (:102-106): first maximum of the histogram, rate in float64"""
    h = np.bincount(np.asarray(ary, np.int64))
    return int(np.argmax(h)), np.amax(h) / len(ary)


def oracle_labeling(superpoint_inds, components, input_gt, pseudo_gt, w, mode, prob_class, threshold, budget, min_size, class_list):
    """the reference's walk, statement by statement; mutates pseudo_gt, w, budget, class_list; returns the used list"""
    used = []
    if mode not in ("dominant", "NAIL"):
        raise ZeroDivisionError("not find oracle_mode")
    for sp in superpoint_inds:
        if budget["click"] <= 0:
            break
        ids = np.asarray(components[sp], np.int64)
        if len(ids) < min_size:
            continue
        used.append(int(sp))
        budget["click"] -= 1
        do_label, do_rate = dominant_label(input_gt[ids])
        if mode == "dominant" or do_rate >= threshold:
            pseudo_gt[0][ids] = 1.0
            pseudo_gt[1][ids] = do_label * 1.0
            class_list.append(do_label)
            w["sp_num"] += 1
            w["p_num"] += len(ids)
            continue
        ignore = True
        cls = np.asarray(prob_class)[ids]
        for c in range(int(cls.max()) + 1):
            sub = ids[cls == c]
            if len(sub) > min_size:
                l, r = dominant_label(input_gt[sub])
                if r >= threshold:
                    budget["click"] -= 1
                    pseudo_gt[0][sub] = 1.0
                    pseudo_gt[1][sub] = l * 1.0
                    class_list.append(l)
                    w["sub_num"] += 1
                    w["sub_p_num"] += len(sub)
                    ignore = False
        if ignore:
            w["ignore_sp_num"] += 1
        else:
            w["split_sp_num"] += 1
    return used


def help_order(picks, cloud_order=None):
    """picks [(cloud, sp)] in pick order -> [(cloud, [sp, ...])] as sampling() walks them: grouped by cloud, clouds by first appearance among
    the picks (or in `cloud_order`, the edcd round's file_list_top order), a cloud's picks in pick order"""
    groups = {}
    for c, s in picks:
        groups.setdefault(int(c), []).append(int(s))
    order = list(groups) if cloud_order is None else [c for c in cloud_order if c in groups]
    assert len(order) == len(groups)
    return [(c, groups[c]) for c in order]


def label_round(picks, clouds, pseudo, mode, threshold, budget, min_size, class_list, cloud_order=None):
    """the tail of sampling(): clouds[c] = dict(components, gt, pred); pseudo[c] = [2, n_c] (mutated).  -> dict(used [(cloud, sp)], counters,
    budget_left, class_list (the whole list), pseudo)"""
    w = dict.fromkeys(COUNTERS, 0)
    b = {"click": int(budget)}
    cl = list(class_list)
    used = []
    for c, sps in help_order(picks, cloud_order):
        u = oracle_labeling(sps, clouds[c]["components"], np.asarray(clouds[c]["gt"]), pseudo[c], w, mode, clouds[c].get("pred"), threshold, b, min_size, cl)
        used += [(c, s) for s in u]
    return dict(used=used, counters=w, budget_left=b["click"], class_list=cl, pseudo=pseudo)


# ---- fabricated inputs --------------------------------------------------------------------------------------------------------------------------
def region(n, parts):
    """(gt, pred) of one region of n points: parts = [(fraction or count, gt label, predicted class)], the last part takes the rest"""
    gt, pr, left = [], [], n
    for i, (k, g, c) in enumerate(parts):
        k = left if i == len(parts) - 1 else min(left, int(round(k * n)) if isinstance(k, float) else int(k))
        gt += [g] * k; pr += [c] * k; left -= k
    return np.array(gt, np.int32), np.array(pr, np.int32)


def cloud_from_regions(regions, rng=None):
    """regions = [(gt, pred)] -> dict(components, gt, pred, offsets, points) with the regions' points scattered over the cloud"""
    sizes = np.array([len(g) for g, _ in regions], np.int64)
    n = int(sizes.sum())
    perm = np.arange(n) if rng is None else rng.permutation(n)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    gt = np.empty(n, np.int32); pred = np.empty(n, np.int32)
    gt[perm] = np.concatenate([g for g, _ in regions]) if n else []
    pred[perm] = np.concatenate([p for _, p in regions]) if n else []
    comps = [perm[off[s]:off[s + 1]].astype(np.int32) for s in range(len(sizes))]
    return dict(components=comps, gt=gt, pred=pred, offsets=off, points=perm.astype(np.int32))


def noisy_cloud(rng, sizes, num_labels=13, num_classes=13, purity=0.93, split=0.35):
    """regions of the given sizes: most carry one label with `purity`; a share `split` is two or three stretches of different labels whose
    predicted classes mostly follow the stretches (so NAIL splits them, sometimes in vain)"""
    regs = []
    for n in sizes:
        n = int(n)
        if rng.random() < split and n >= 4:
            k = int(rng.integers(2, 4))
            cuts = np.sort(rng.choice(np.arange(1, n), k - 1, replace=False))
            seg = np.diff(np.concatenate([[0], cuts, [n]]))
            labs = rng.choice(num_labels, k, replace=False); cls = rng.choice(num_classes, k, replace=False)
            gt = np.repeat(labs, seg); pr = np.repeat(cls, seg)
            flip = rng.random(n) < 0.04
            pr = np.where(flip, rng.integers(0, num_classes, n), pr)
            gt = np.where(rng.random(n) < 0.03, rng.integers(0, num_labels, n), gt)
        else:
            base = int(rng.integers(0, num_labels))
            gt = np.where(rng.random(n) < purity, base, rng.integers(0, num_labels, n))
            pr = np.where(rng.random(n) < 0.8, int(rng.integers(0, num_classes)), rng.integers(0, num_classes, n))
        regs.append((gt.astype(np.int32), pr.astype(np.int32)))
    return cloud_from_regions(regs, rng)


def concat_clouds(clouds):
    """-> gt, pred, sp_off, sp_pts, sp_cloud, base (first global region of every cloud), p0 (first point)"""
    p0 = np.concatenate([[0], np.cumsum([len(c["gt"]) for c in clouds])]).astype(np.int64)
    base = np.concatenate([[0], np.cumsum([len(c["components"]) for c in clouds])]).astype(np.int64)
    offs, pts, cloud = [np.zeros(1, np.int64)], [], []
    for b, c in enumerate(clouds):
        o = np.asarray(c["offsets"], np.int64)
        offs.append(o[1:] + offs[-1][-1]); pts.append(np.asarray(c["points"], np.int64) + p0[b]); cloud.append(np.full(len(o) - 1, b, np.int32))
    return (np.concatenate([c["gt"] for c in clouds]).astype(np.int32), np.concatenate([c["pred"] for c in clouds]).astype(np.int32),
            np.concatenate(offs).astype(np.int32), np.concatenate(pts).astype(np.int32), np.concatenate(cloud).astype(np.int32), base, p0)
