"""TEST INFRASTRUCTURE ONLY — the seed, random and label-all rounds with draws="device" restated in NumPy: the key rule of include/ssdr_al.h
("the seed, random and label-all samplers") with _draw_oracle's words, the walk with _labeling_oracle.label_round.  Nothing here calls the
library.  Regions are GLOBAL ids throughout (cloud c owns [base[c], base[c + 1])); `labeled` is the bool mask over them and is mutated."""
import numpy as np

import _draw_oracle as D
import _labeling_oracle as LO

REGION_COUNT, REGION_PICK = 3, 4


def _keys(seed, rnd, it, kind, e, key_bits):
    return D.word(seed, rnd, it, kind, np.asarray(e, np.uint64), 0) >> np.uint64(32 - key_bits)


def drawn_elements(seed, rnd, it, T, k, key_bits=32):
    """the k smallest of range(T) by (key, element)"""
    if k > T:
        raise ValueError("Cannot take a larger sample than population when 'replace=False'")
    return np.argsort(_keys(seed, rnd, it, REGION_COUNT, np.arange(T), key_bits), kind="stable")[:k]


def pick_order(seed, rnd, it, regions, key_bits=32, first_region=0):
    """`regions` (ascending global ids) in draw order: ascending (key, id)"""
    regions = np.asarray(regions, np.int64)
    return regions[np.argsort(_keys(seed, rnd, it, REGION_PICK, first_region + regions, key_bits), kind="stable")]


def iteration(seed, rnd, it, T, click, labeled, base, key_bits=32):
    """one _iteration's draws -> dict(live [clouds], k, each, picks [(cloud, [global ids])], items, remain)"""
    B = len(base) - 1
    unl = {c: np.flatnonzero(~labeled[base[c]:base[c + 1]]) + base[c] for c in range(B)}
    live = [c for c in range(B) if len(unl[c])]
    L = len(live)
    each = np.bincount(drawn_elements(seed, rnd, it, T, click, key_bits) % L, minlength=L) if L else np.zeros(0, np.int64)
    picks, remain = [], 0
    for d, c in enumerate(live):
        cnt, u = int(each[d]), unl[c]
        if cnt == 0:
            continue
        if len(u) >= cnt:
            sel = pick_order(seed, rnd, it, u, key_bits)[:cnt]
        else:
            sel, remain = u, remain + cnt - len(u)
        picks.append((c, [int(s) for s in sel]))
    return dict(live=live, k=int(click), each=each.astype(np.int64), picks=picks, items=np.array([s for _, sps in picks for s in sps], np.int64), remain=remain)


def _walk(picks, clouds, base, pseudo, mode, threshold, budget, min_size):
    """the existing walk over one item list -> (label_round's result with global used ids)"""
    r = LO.label_round([(c, s - int(base[c])) for c, sps in picks for s in sps], clouds, pseudo, mode, threshold, budget, min_size, [])
    r["used"] = [int(base[c]) + s for c, s in r["used"]]
    return r


def random_round(seed, rnd, clouds, labeled, base, pseudo, budget, min_size, mode="dominant", threshold=0.9, T=None, key_bits=32, max_iter=32):
    """RandomSampler.sampling: -> dict(iters [iteration dicts], used, counters, budget_left, class_entries, iterations, stopped (max_iter hit))"""
    T = len(labeled) if T is None else T
    w, iters, used, entries, stopped = dict.fromkeys(LO.COUNTERS, 0), [], [], [], False
    it = 0
    while True:
        d = iteration(seed, rnd, it, T, budget, labeled, base, key_bits)
        r = _walk(d["picks"], clouds, base, pseudo, mode, threshold, budget, min_size)
        iters.append(d); used += r["used"]; entries += r["class_list"]
        for k in LO.COUNTERS:
            w[k] += r["counters"][k]
        labeled[r["used"]] = True
        budget = r["budget_left"]
        it += 1
        if budget <= 0 or labeled.all():
            break
        if it >= max_iter:
            stopped = True
            break
    return dict(iters=iters, used=used, counters=w, budget_left=budget, class_entries=entries, iterations=it, stopped=stopped)


def all_round(clouds, labeled, base, pseudo, budget, mode="dominant", threshold=0.9):
    """AllSampler.sampling: one walk over every unlabelled region in ascending order, min_size = 1"""
    B = len(base) - 1
    picks = [(c, [int(s) for s in np.flatnonzero(~labeled[base[c]:base[c + 1]]) + base[c]]) for c in range(B)]
    picks = [p for p in picks if p[1]]
    r = _walk(picks, clouds, base, pseudo, mode, threshold, budget, 1)
    labeled[r["used"]] = True
    return dict(iters=[dict(items=np.array([s for _, sps in picks for s in sps], np.int64))], used=r["used"], counters=r["counters"], budget_left=r["budget_left"],
                class_entries=r["class_list"], iterations=1, stopped=False)


def seed_round(seed, rnd, clouds, labeled, base, pseudo, number, T=None, key_bits=32, max_iter=32):
    """SeedSampler.sampling: every item labelled precisely; -> dict(iters, used, sp_num, p_num, remain, iterations)"""
    T = len(labeled) if T is None else T
    iters, used, sp_num, p_num, remain, it = [], [], 0, 0, int(number), 0
    while remain > 0 and not labeled.all() and it < max_iter:
        d = iteration(seed, rnd, it, T, remain, labeled, base, key_bits)
        for c, sps in d["picks"]:
            for s in sps:
                ids = np.asarray(clouds[c]["components"][s - int(base[c])], np.int64)
                pseudo[c][0][ids] = 1.0
                pseudo[c][1][ids] = np.asarray(clouds[c]["gt"])[ids]
                sp_num += 1; p_num += len(ids)
        labeled[d["items"]] = True
        iters.append(d); used += d["items"].tolist()
        remain = d["remain"]
        it += 1
    return dict(iters=iters, used=used, sp_num=sp_num, p_num=p_num, remain=remain, iterations=it)
