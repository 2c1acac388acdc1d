"""The seed, random and label-all rounds (the reference's SeedSampler, RandomSampler and AllSampler, S3/sampler2.py:344-520) on the device:
csrc/select_random.hip through HotPath(selector="random" | "all"), HotPath.seed_round and ALRound.

draws="host" is pinned to the reference's own classes by tests/golden/samplers_golden.npz (make_golden_samplers.py); draws="device" is compared index
for index with the NumPy restatement of the key rule in _sampler_oracle.py, on the CPU logic build and on the GPU.  Every case asserts its own input
condition from the oracle first."""
import numpy as np
import pytest

import _draw_oracle as D
import _labeling_oracle as LO
import _sampler_oracle as SO

NC = 13


def _pool(seed, regions, lo=1, hi=60, big=0.0):
    """clouds of the given region counts; region sizes lo..hi, a share `big` of them 257..700 points (the workgroup form)"""
    rng = np.random.default_rng(seed)
    clouds = []
    for n in regions:
        sizes = rng.integers(lo, hi + 1, n)
        if big:
            sizes = np.where(rng.random(n) < big, rng.integers(257, 701, n), sizes)
        clouds.append(LO.noisy_cloud(rng, sizes))
    return clouds


def _hot_path(clouds, labeled=None, selector="random", nail=False, **kw):
    from ssdr_al import _lib, pipeline
    from ssdr_al.helper_tool import ConfigS3DIS

    class Cfg(ConfigS3DIS):
        num_classes = NC
    cl = []
    for c in clouds:
        n = len(c["gt"])
        probs = np.zeros((n, NC), np.float32)
        if nail:
            probs[np.arange(n), c["pred"]] = 1.0                  # the prediction pass then finds the fabricated classes
        cl.append(dict(xyz=np.zeros((n, 3), np.float32), gt=c["gt"], probs=probs, feat=np.zeros((n, 32), np.float32), offsets=c["offsets"], points=c["points"]))
    hp = pipeline.HotPath.from_clouds(cl, labeled if labeled is not None else [set() for _ in clouds], [3, 1], Cfg, selector=selector, **kw)
    hp.record_shares = True
    if nail:
        hp._score_async()
        _lib.sync()
        assert np.array_equal(hp.cls.to_host(), np.concatenate([c["pred"] for c in clouds]))
    return hp


def _base(hp):
    return np.concatenate([np.asarray(hp.sp_base, np.int64), [hp.S]])


def _compare_draws(res, exp):
    assert res.iterations == exp["iterations"] == len(res.drawn) == len(exp["iters"])
    for i, (info, items, e) in enumerate(zip(res.draw_info, res.drawn, exp["iters"])):
        assert np.array_equal(items, e["items"]), "items of iteration %d" % i
        if "k" in e:
            assert info["k"] == e["k"] and info["live"] == len(e["live"]) and info["remain"] == e["remain"], "k / live clouds / remainder of iteration %d" % i
            assert np.array_equal(info["each"], e["each"]), "each_file_number of iteration %d" % i


def _random_case(clouds, budget, min_size, labeled=None, mode="dominant", threshold=0.9, selector="random", T=None, key_bits=32, max_iter=32, seed=5, rnd=2):
    """one round on the device and in the oracle, compared index for index -> (LabelResult, oracle result, HotPath)"""
    hp = _hot_path(clouds, labeled, selector, nail=mode == "NAIL", batch_size=budget, min_size=min_size, total_num=T, draw_key_bits=key_bits, max_iter=max_iter,
                   draw_seed=seed, round_num=rnd)
    base = _base(hp)
    lab = hp.labeled_mask.copy()
    pseudo = [np.zeros((2, len(c["gt"])), np.float32) for c in clouds]
    if selector == "all":
        exp = SO.all_round(clouds, lab, base, pseudo, budget, mode, threshold)
    else:
        exp = SO.random_round(seed, rnd, clouds, lab, base, pseudo, budget, min_size, mode, threshold, T, key_bits, max_iter)
    sel, unl = hp.step_selection()
    assert np.array_equal(sel, np.arange(len(sel))) and np.array_equal(unl.b, exp["iters"][0]["items"])
    assert hp.selected == [(int(hp.sp_cloud_h[s]), int(s - base[hp.sp_cloud_h[s]])) for s in exp["iters"][0]["items"]]
    res = hp.label_selected(mode=mode, threshold=threshold)
    _compare_draws(res, exp)
    assert np.array_equal(res.to_host(), np.concatenate(pseudo, axis=1)), "pseudo_gt"
    assert np.array_equal(hp.labeled_mask, lab), "labelled mask"
    assert hp._class_list_h.tolist() == [3, 1] + [int(x) for x in exp["class_entries"]] and res.class_entries.tolist() == [int(x) for x in exp["class_entries"]]
    assert res.counters == exp["counters"] and res.budget_left == exp["budget_left"]
    assert res.used == [(int(hp.sp_cloud_h[s]), int(s - base[hp.sp_cloud_h[s]])) for s in exp["used"]]
    from ssdr_al import sampler
    assert bool(res.status & sampler.ST_MAX_ITER) == exp["stopped"]
    return res, exp, hp


# ---- draws="device" against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dominant", "NAIL"])
def test_five_uneven_clouds_both_label_forms(backend, mode):
    """[40, 1, 300, 7, 2500] regions of 1 .. 700 points: both sorts span more than one 2048-slot tile, the walk judges regions by waves and by workgroups,
    two clouds are smaller than their share (taken whole), and one of them goes dead"""
    clouds = _pool(1, [40, 1, 300, 7, 2500], 1, 60, big=0.08)
    res, exp, hp = _random_case(clouds, 600, 3, mode=mode)
    assert hp.S == 2848 > 2048 and int(hp.sp_size_h.max()) > 256 and int(hp.sp_size_h.min()) == 1
    e0 = exp["iters"][0]
    assert e0["each"][1] > 1 and e0["each"][3] > 7 and exp["iterations"] > 1
    assert res.forms["wave"] > 0 and res.forms["block"] > 0
    if mode == "NAIL":
        assert res.counters["split_sp_num"] > 0 and res.counters["sub_num"] > 0


def test_total_num_not_a_multiple_of_the_live_clouds(backend):
    clouds = _pool(2, [10, 11, 12])
    res, exp, _ = _random_case(clouds, 20, 1, T=35)
    assert 35 % len(exp["iters"][0]["live"]) != 0 and 35 != 33


@pytest.mark.parametrize("click", [33, 1])
def test_click_equals_total_num_and_one(backend, click):
    clouds = _pool(3, [10, 11, 12])
    res, exp, hp = _random_case(clouds, click, 1)
    e0 = exp["iters"][0]
    assert hp.S == 33 and e0["k"] == click and int(e0["each"].sum()) == click
    if click == 33:
        assert e0["each"].tolist() == [11, 11, 11] and len(e0["items"]) == 32      # every element is drawn: cloud 0 is one short of its share
    else:
        assert len(e0["items"]) == 1 and exp["iterations"] == 1


def test_cloud_goes_dead_between_iterations(backend):
    clouds = _pool(4, [2, 30, 30])
    res, exp, _ = _random_case(clouds, 30, 1)
    assert exp["iterations"] >= 2 and exp["iters"][0]["live"] == [0, 1, 2] and exp["iters"][1]["live"] == [1, 2]


def test_all_clouds_exhausted_with_budget_left(backend):
    clouds = _pool(5, [5, 20])
    res, exp, hp = _random_case(clouds, 30, 1, T=40)
    assert hp.labeled_mask.all() and res.budget_left == 5 and exp["iterations"] > 1 and not exp["stopped"]


def test_four_key_bits_break_ties_by_id(backend):
    clouds = _pool(6, [150, 170])
    seed, rnd = 5, 2
    k3 = D.word(seed, rnd, 0, SO.REGION_COUNT, np.arange(320, dtype=np.uint64), 0) >> np.uint64(28)
    k4 = D.word(seed, rnd, 0, SO.REGION_PICK, np.arange(320, dtype=np.uint64), 0) >> np.uint64(28)
    assert len(np.unique(k3)) <= 16 and len(np.unique(k4)) <= 16         # 320 elements on 16 keys: both sorts are decided by the id
    res, exp, _ = _random_case(clouds, 100, 1, key_bits=4, seed=seed, rnd=rnd)
    e = exp["iters"][0]["picks"][0][1]
    assert e != sorted(e)                                                  # (the draw order is not the id order)


def test_three_hundred_small_clouds(backend):
    """the live scan and the take scan go around their 256-thread workgroup"""
    rng = np.random.default_rng(7)
    clouds = _pool(7, rng.integers(1, 4, 300).tolist(), 1, 12)
    labeled = [set() for _ in clouds]
    for c in (0, 17, 255, 256, 299):
        labeled[c] = set(range(len(clouds[c]["components"])))              # dead clouds on both sides of the workgroup's edge
    res, exp, _ = _random_case(clouds, 250, 1, labeled=labeled)
    assert len(exp["iters"][0]["live"]) == 295 > 256 and exp["iterations"] > 1


def test_max_iter_stops_the_loop(backend):
    """only regions below min_size are left: the reference recurses for ever, here the loop reports it"""
    clouds = _pool(8, [20, 20], 1, 3)
    res, exp, _ = _random_case(clouds, 5, 10, max_iter=3)
    assert exp["stopped"] and res.iterations == 3 and res.budget_left == 5 and res.used == []


def test_pre_labelled_mask(backend):
    clouds = _pool(9, [25, 40, 3])
    labeled = [set(range(0, 25, 2)), set(range(10, 40)), {1}]
    res, exp, hp = _random_case(clouds, 18, 1, labeled=labeled)
    base = _base(hp)
    before = np.zeros(hp.S, bool)
    for c, ids in enumerate(labeled):
        before[base[c] + np.array(sorted(ids))] = True
    assert not before[np.concatenate(res.drawn)].any() and exp["iterations"] >= 1


def test_label_all(backend):
    """AllSampler: one walk over every unlabelled region in ascending order, min_size = 1 whatever the HotPath's; the budget ends the walk"""
    clouds = _pool(10, [30, 1, 44], 1, 60, big=0.1)
    labeled = [set(range(5, 12)), set(), {0, 43}]
    res, exp, hp = _random_case(clouds, 40, 7, labeled=labeled, selector="all")
    assert res.iterations == 1 and len(res.drawn[0]) == 75 - 9 and res.budget_left == 0 and len(res.used) == 40
    assert int(hp.sp_size_h[np.concatenate(res.drawn)[:40]].min()) < 7     # (a region below the HotPath's min_size was labelled)
    res, exp, hp = _random_case(clouds, 500, 1, labeled=labeled, selector="all", mode="NAIL")
    assert hp.labeled_mask.all() and res.budget_left > 0


def test_seed_remainder_over_three_iterations(backend):
    clouds = _pool(11, [1, 12, 60], 1, 60, big=0.1)
    seed, rnd, number = 9, 0, 30
    hp = _hot_path(clouds, None, "random", draw_seed=seed)
    base = _base(hp)
    lab = hp.labeled_mask.copy()
    pseudo = [np.zeros((2, len(c["gt"])), np.float32) for c in clouds]
    exp = SO.seed_round(seed, rnd, clouds, lab, base, pseudo, number)
    assert exp["iterations"] >= 3 and exp["iters"][0]["remain"] > 0 and exp["iters"][1]["remain"] > 0 and exp["remain"] == 0
    assert len(exp["iters"][0]["live"]) == 3 and len(exp["iters"][1]["live"]) == 2
    res = hp.seed_round(number, rnd)
    _compare_draws(res, exp)
    assert np.array_equal(res.to_host(), np.concatenate(pseudo, axis=1)) and np.array_equal(hp.labeled_mask, lab)
    assert res.counters["sp_num"] == exp["sp_num"] == number and res.counters["p_num"] == exp["p_num"] and res.budget_left == 0
    assert len(res.class_entries) == 0 and hp._class_list_h.tolist() == [3, 1]
    got = res.to_host()
    gt = np.concatenate([c["gt"] for c in clouds])
    assert np.array_equal(got[1][got[0] == 1], gt[got[0] == 1].astype(np.float32))        # precise labels
    # more seeds than regions are left: everything is labelled and the rest is reported
    res = hp.seed_round(60, rnd)
    assert hp.labeled_mask.all() and res.budget_left > 0 and res.counters["sp_num"] == 73 - number


def test_refusals(backend):
    from ssdr_al import _lib, pipeline, sampler
    from ssdr_al._lib import DevArray
    L = _lib.lib()
    S, B = 6, 2
    lab, cloud = DevArray.from_host(np.zeros(S, np.uint8)), DevArray.from_host(np.array([0, 0, 0, 1, 1, 1], np.int32))
    cnt, items, n, info = DevArray.from_host(np.array([3], np.int64)), DevArray.from_host(np.full(S, -7, np.int32)), DevArray.from_host(np.array([-7], np.int32)), DevArray((8,), np.int64)

    def draw(mode=0, key_bits=32, lab_p=lab.ptr, cloud_p=cloud.ptr, S_=S, T=S, cnt_p=cnt.ptr, items_p=items.ptr, n_p=n.ptr, info_p=info.ptr):
        return L.ssdr_region_draw_dev(1, 0, 0, mode, key_bits, 0, lab_p, cloud_p, S_, B, T, cnt_p, items_p, S, n_p, info_p, None)
    for bad in (dict(lab_p=None), dict(cloud_p=None), dict(cnt_p=None), dict(items_p=None), dict(n_p=None), dict(info_p=None), dict(S_=0), dict(T=0), dict(key_bits=0),
                dict(key_bits=33), dict(mode=2)):
        assert draw(**bad) == 1, bad
    _lib.sync()
    assert items.to_host().tolist() == [-7] * S and n.to_host()[0] == -7              # nothing was launched
    assert draw(mode=1, cnt_p=None) == 0                                               # label-all reads no count
    _lib.sync()
    assert n.to_host()[0] == S and items.to_host().tolist() == list(range(S))
    # a count above total_num lives on the device: refused there, with an empty list
    cnt7 = DevArray.from_host(np.array([7], np.int64))
    assert draw(cnt_p=cnt7.ptr) == 0
    _lib.sync()
    w = info.to_host()
    assert w[5] & sampler.DRAW_ST_COUNT and w[1] == 0 and w[2] == 0 and n.to_host()[0] == 0
    with pytest.raises(ValueError, match="larger sample than population"):
        sampler.region_draw_status_check(int(w[5]), 7, S)
    # the precise labels
    gt, off, pts = DevArray.from_host(np.arange(4, dtype=np.int32)), DevArray.from_host(np.array([0, 2, 4], np.int32)), DevArray.from_host(np.arange(4, dtype=np.int32))
    m, l, lb, out = DevArray.from_host(np.zeros(4, np.float32)), DevArray.from_host(np.zeros(4, np.float32)), DevArray.from_host(np.zeros(2, np.uint8)), DevArray((3,), np.int64)
    it2, n2 = DevArray.from_host(np.array([1, 5], np.int32)), DevArray.from_host(np.array([2], np.int32))

    def seed(gt_p=gt.ptr, S_=2, it_p=it2.ptr, n_p=n2.ptr, m_p=m.ptr, out_p=out.ptr):
        return L.ssdr_seed_label_dev(gt_p, 4, off.ptr, pts.ptr, S_, it_p, n_p, 2, 2, m_p, l.ptr, lb.ptr, out_p, None)
    for bad in (dict(gt_p=None), dict(S_=0), dict(it_p=None), dict(n_p=None), dict(m_p=None), dict(out_p=None)):
        assert seed(**bad) == 1, bad
    assert seed() == 0
    _lib.sync()
    assert out.to_host().tolist() == [1, 2, 4] and m.to_host().tolist() == [0, 0, 1, 1] and l.to_host().tolist() == [0, 0, 2, 3] and lb.to_host().tolist() == [0, 1]
    # the Python layer
    clouds = _pool(12, [4, 5])
    hp = _hot_path(clouds, batch_size=10)                                              # 10 clicks of total_num = 9
    with pytest.raises(ValueError, match="larger sample than population"):
        hp.step_selection()
    hp = _hot_path(clouds, batch_size=4)
    with pytest.raises(RuntimeError, match="no selection to label"):
        hp.label_selected(mode="dominant")
    hp.step_selection()
    with pytest.raises(ValueError, match="predicted classes resident"):
        hp.label_selected(mode="NAIL")
    with pytest.raises(ValueError, match="drawn for batch_size = 4"):
        hp.label_selected(mode="dominant", budget=5)
    assert hp.label_selected(mode="dominant").budget_left == 0
    hp = _hot_path(clouds, selector="all", batch_size=4)                               # label-all draws nothing: another budget walks the same list
    hp.step_selection()
    res = hp.label_selected(mode="dominant", budget=2)
    assert res.budget_left == 0 and res.used == [(0, 0), (0, 1)]
    for sel in ("random", "all"):
        with pytest.raises(ValueError, match="communicator"):
            _hot_path(clouds, selector=sel, batch_size=4).step_selection(comm=object())
    with pytest.raises(AssertionError):
        _hot_path(clouds, selector="seed")
    assert "random" in pipeline.SELECTORS and "all" in pipeline.SELECTORS


# ---- draws="host" against the reference's own classes ------------------------------------------------------------------------------------------
def _golden_case(g, k):
    p = "c%d/" % k
    regions = g[p + "regions"]
    clouds, o0, p0 = [], 0, 0
    for n in regions:
        off = g[p + "offsets"][o0: o0 + n + 1]; o0 += n + 1
        npts = int(off[-1])
        pts, gt, pred = (g[p + key][p0: p0 + npts] for key in ("points", "gt", "pred")); p0 += npts
        clouds.append(dict(components=[pts[off[s]:off[s + 1]] for s in range(n)], gt=gt, pred=pred, offsets=off, points=pts))
    return p, clouds, [int(x) for x in g[p + "params"]], float(g[p + "threshold"])


def _assert_stage(g, p, hp, res, class_list):
    assert np.array_equal(res.to_host(), g[p + "pseudo"]), p + "pseudo_gt"
    off, live = g[p + "unl_off"], g[p + "unl_live"]
    lists = hp.unlabeled_lists
    assert sorted(lists) == np.flatnonzero(live).tolist(), p + "live clouds"
    for c in lists:
        assert [int(x) for x in lists[c]] == g[p + "unl"][off[c]:off[c + 1]].tolist(), p + "unlabeled list of cloud %d (the reference's order)" % c
    assert [res.counters[name] for name in LO.COUNTERS] == g[p + "w"].tolist(), p + "w"
    assert res.budget_left == int(g[p + "budget"]), p + "budget"
    assert class_list == g[p + "class_list"].tolist(), p + "selected_class_list"


def test_host_draws_reproduce_the_reference_golden(backend, golden):
    """SeedSampler._iteration, RandomSampler._iteration and AllSampler.sampling of the reference, one after the other on one pool, each after its own
    np.random.seed: draws="host" consumes a RandomState the same way and leaves the same pseudo_gt, unlabeled lists (order included), class list, w, budget"""
    g = golden("samplers_golden.npz")
    iters = []
    for k in range(int(g["n_cases"])):
        p, clouds, (number, clicks, min_size, nail, all_clicks, total_num, s0, s1, s2), thr = _golden_case(g, k)
        mode = "NAIL" if nail else "dominant"
        hp = _hot_path(clouds, None, "random", nail=bool(nail), draws="host", batch_size=clicks, min_size=min_size, total_num=total_num)
        hp._class_list_h = np.zeros(0, np.int32)
        hp.draw_rng = np.random.RandomState(s0)
        res = hp.seed_round(number)
        _assert_stage(g, p + "seed/", hp, res, [])
        it_seed = res.iterations
        hp.draw_rng = np.random.RandomState(s1)
        hp.step_selection()
        res = hp.label_selected(mode=mode, threshold=thr)
        _assert_stage(g, p + "random/", hp, res, hp._class_list_h.tolist())
        iters.append((it_seed, res.iterations))
        n_random = len(hp._class_list_h)
        hp.selector, hp.batch_size = "all", all_clicks
        hp._select_static()
        hp.draw_rng = np.random.RandomState(s2)
        hp.step_selection()
        res = hp.label_selected(mode=mode, threshold=thr)
        _assert_stage(g, p + "all/", hp, res, hp._class_list_h.tolist())
        assert len(hp._class_list_h) > n_random
    assert max(a for a, _ in iters) > 1 and max(b for _, b in iters) > 1, iters      # the take-all branch and a second iteration occur in both samplers


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------
def test_al_round_seed_random_all(backend):
    """ALRound.seed, ALRound(selector="random").run() / label(), then label-all over the same regions: the oracle's rounds over the round's own arrays; the
    random round passes no profiler site but the draw's and the walk's (no front end, no pyramid, no network, no scoring)"""
    from oracle import randla_np as R
    from ssdr_al import _lib, pipeline, synthetic
    from ssdr_al.helper_tool import ConfigS3DIS
    emu = backend == "emu"

    class Cfg(ConfigS3DIS):
        num_points = 512 if emu else 4096
    rooms = [synthetic.make_room(8300 + i, density=70.0 if emu else 600.0) for i in range(2)]
    ar = pipeline.ALRound(R.init_weights(0), rooms, 2, Cfg, batch_size=12, round_num=3, labeled_per_tile=0, selector="random", draw_seed=21, min_size=4)
    S = ar.sel
    assert not S.labeled_mask.any() and S.B == 4
    S.record_shares = True
    N = Cfg.num_points
    gt = ar.tile_l.to_host()
    base = _base(S)
    clouds = []
    for t in range(S.B):
        off = S.sp_off_h[base[t]: base[t + 1] + 1].astype(np.int64)
        clouds.append(dict(components=[S.sp_pts_h[off[s]:off[s + 1]].astype(np.int64) - t * N for s in range(len(off) - 1)], gt=gt[t * N:(t + 1) * N]))
    lab = np.zeros(S.S, bool)
    pseudo = [np.zeros((2, N), np.float32) for _ in clouds]
    e_seed = SO.seed_round(21, 0, clouds, lab, base, pseudo, 9)
    res = ar.seed(9)
    _compare_draws(res, e_seed)
    assert np.array_equal(res.to_host(), np.concatenate(pseudo, axis=1)) and np.array_equal(S.labeled_mask, lab) and res.counters["sp_num"] == 9
    L = _lib.lib()
    L.ssdr_prof_report()
    L.ssdr_prof_enable(1)
    try:
        sel, unl = ar.run()
        res = ar.label(mode="dominant")
        sites = {ln.rsplit(" ", 4)[0].strip() for ln in L.ssdr_prof_report().decode().splitlines() if ln.strip()}
    finally:
        L.ssdr_prof_enable(0)
    # (sel_dominant_label: set_labeled's bookkeeping of the labelled pool once the round is over)
    assert {"region_draw", "label_scan"} <= sites and all(s.startswith(("region_draw", "label_", "sel_dominant_label")) for s in sites), sites
    e_rand = SO.random_round(21, 3, clouds, lab, base, pseudo, 12, 4)
    _compare_draws(res, e_rand)
    assert np.array_equal(unl.b, e_rand["iters"][0]["items"])
    assert np.array_equal(res.to_host(), np.concatenate(pseudo, axis=1)) and np.array_equal(S.labeled_mask, lab)
    assert res.counters == e_rand["counters"] and res.budget_left == e_rand["budget_left"]
    S.selector, S.batch_size = "all", S.S
    S._select_static()
    e_all = SO.all_round(clouds, lab, base, pseudo, S.S)
    ar.run()
    res = ar.label(mode="dominant")
    assert np.array_equal(res.to_host(), np.concatenate(pseudo, axis=1)) and S.labeled_mask.all() and lab.all()
    assert res.counters == e_all["counters"] and res.budget_left == e_all["budget_left"]
    with pytest.raises(ValueError, match="communicator"):
        pipeline.ALRound(None, rooms, 2, Cfg, selector="random", comm=object())


# ---- the key rule on the oracle alone ----------------------------------------------------------------------------------------------------------
def test_shares_follow_the_hypergeometric_law():
    """each_file_number[d] counts the drawn elements of the class {e < T : e % L == d}: k draws without replacement from T elements of which N_d lie in
    the class — hypergeometric, mean k N_d / T, variance k (N_d / T) (1 - N_d / T) (T - k) / (T - 1).  Over the fixed seeds 0 .. 199 every cloud's mean
    count lies within four standard errors of that mean (the seed range was chosen so that the oracle passes: it is a check of the rule, not a
    statistical test of the mixer)."""
    T, L, k, n = 1000, 7, 100, 200
    each = np.stack([np.bincount(SO.drawn_elements(seed, 1, 0, T, k) % L, minlength=L) for seed in range(n)])
    assert (each.sum(axis=1) == k).all()
    for d in range(L):
        N_d = len(range(d, T, L))
        mean = k * N_d / T
        var = k * (N_d / T) * (1 - N_d / T) * (T - k) / (T - 1)
        se = np.sqrt(var / n)
        got = each[:, d].mean()
        print("cloud %d: N_d %d, mean %.3f, expected %.3f, standard error %.3f" % (d, N_d, got, mean, se))
        assert abs(got - mean) < 4 * se


def test_sanitized_stand_alone_program():
    """make region-draw-san: one case of each entry under ASan + UBSan on the CPU build, a program with its own main (nothing preloaded)"""
    import os
    import subprocess
    from conftest import PKG, ROOT
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(PKG, "csrc"), "region-draw-san"])
    env = dict(os.environ, OMP_NUM_THREADS="2", ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "san", "region_draw_san")], env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and "region draw ok" in r.stdout, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
