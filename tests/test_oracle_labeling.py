"""oracle_labeling / _help of TSampler.sampling() (S3/sampler2.py:124-216) on the device: ssdr_oracle_label_dev, sampler.oracle_labeling,
HotPath.label_selected and ALRound.label against the NumPy restatement in _labeling_oracle.py, which a golden file made with the reference's
own function pins.  Everything is integers and exact 0 / 1 / label values: compared for equality."""
import ctypes as C

import numpy as np
import pytest

import _labeling_oracle as O
from _fabricate import make_clouds

N_GOLDEN = 6


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------------
def _abi(clouds, picks, mode, thr, budget, min_size, nl=13, nc=13, pseudo=None, cloud_key=None, max_region=None, class_cap=None, labeled=None, profile=False):
    """ssdr_oracle_label_dev over the concatenated clouds; picks = [(cloud, region in cloud)] in pick order"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    gt, pred, off, pts, cloud, base, p0 = O.concat_clouds(clouds)
    n, S, M = len(gt), len(off) - 1, len(picks)
    items = np.array([base[c] + s for c, s in picks] + [0], np.int32)
    pseudo = np.zeros((2, n), np.float32) if pseudo is None else np.asarray(pseudo, np.float32)
    cap = max(1, M * 32) if class_cap is None else class_cap
    d = dict(gt=DevArray.from_host(gt), pred=DevArray.from_host(pred), off=DevArray.from_host(off), pts=DevArray.from_host(pts), cloud=DevArray.from_host(cloud),
             items=DevArray.from_host(items), n=DevArray.from_host(np.array([M], np.int32)), budget=DevArray.from_host(np.array([budget], np.int64)),
             mask=DevArray.from_host(np.ascontiguousarray(pseudo[0])), label=DevArray.from_host(np.ascontiguousarray(pseudo[1])),
             used=DevArray.from_host(np.full(max(M, 1), 7, np.uint8)), labeled=DevArray.from_host(np.zeros(S, np.uint8) if labeled is None else labeled.astype(np.uint8)),
             cls=DevArray.from_host(np.full(cap + 1, -5, np.int32)), proc=DevArray((max(M, 1),), np.int32), out=DevArray((12,), np.int64))
    d_key = None if cloud_key is None else DevArray.from_host(np.asarray(cloud_key, np.int32))
    L = _lib.lib()
    if max_region is None:
        max_region = int(np.diff(off).max())
    if profile:
        L.ssdr_prof_report(); L.ssdr_prof_enable(1)
    try:
        rc = L.ssdr_oracle_label_dev(d["gt"].ptr, d["pred"].ptr, n, d["off"].ptr, d["pts"].ptr, S, d["cloud"].ptr, len(clouds), d["items"].ptr, d["n"].ptr, M,
                                     None if d_key is None else d_key.ptr, max_region, nl, nc, {"dominant": 0, "NAIL": 1}.get(mode, 9), thr, min_size,
                                     d["budget"].ptr, d["mask"].ptr, d["label"].ptr, d["used"].ptr, d["labeled"].ptr, d["cls"].ptr, cap, d["proc"].ptr, d["out"].ptr, None)
        names = {ln.rsplit(" ", 4)[0] for ln in L.ssdr_prof_report().decode().splitlines() if ln.strip()} if profile else None
    finally:
        if profile:
            L.ssdr_prof_enable(0)
    if rc:
        return dict(rc=rc)
    _lib.sync()
    out = d["out"].to_host()
    cls = d["cls"].to_host()
    assert cls[cap] == -5                                                 # nothing behind the class list's capacity
    used = d["used"].to_host()[:M]
    proc = d["proc"].to_host()[:M]
    return dict(rc=0, out=out, pseudo=np.stack([d["mask"].to_host(), d["label"].to_host()]), used_flags=used,
                used=[picks[i] for i in proc if used[i]], proc=proc, labeled=d["labeled"].to_host() != 0, classes=cls[: int(out[6])].tolist(),
                budget=int(d["budget"].to_host()[0]), names=names, p0=p0, base=base)


def _expect(clouds, picks, mode, thr, budget, min_size, pseudo=None, cloud_order=None, class_list=()):
    n_of = [len(c["gt"]) for c in clouds]
    p0 = np.concatenate([[0], np.cumsum(n_of)])
    ps = [np.zeros((2, n), np.float32) if pseudo is None else np.array(pseudo[:, p0[b]:p0[b + 1]], np.float32) for b, n in enumerate(n_of)]
    return O.label_round(picks, clouds, ps, mode, thr, budget, min_size, list(class_list), cloud_order)


def _same(got, exp, clouds, labeled_before=None):
    assert got["rc"] == 0 and int(got["out"][8]) == 0
    assert got["used"] == exp["used"]
    assert [int(x) for x in got["out"][:6]] == [exp["counters"][k] for k in O.COUNTERS]
    assert int(got["out"][7]) == exp["budget_left"] == got["budget"]
    assert got["classes"] == exp["class_list"] and int(got["out"][9]) == len(exp["used"])
    assert np.array_equal(got["pseudo"], np.concatenate(exp["pseudo"], axis=1))
    lab = np.zeros(len(got["labeled"]), bool) if labeled_before is None else labeled_before.copy()
    for c, s in exp["used"]:
        lab[got["base"][c] + s] = True
    assert np.array_equal(got["labeled"], lab)


def _run(clouds, picks, mode, thr, budget, min_size, **kw):
    got = _abi(clouds, picks, mode, thr, budget, min_size, **kw)
    exp = _expect(clouds, picks, mode, thr, budget, min_size, pseudo=kw.get("pseudo"))
    _same(got, exp, clouds)
    return got, exp


def _golden_case(g, k):
    p = "c%d/" % k
    off, pts = g[p + "offsets"], g[p + "points"]
    comps = [pts[off[s]:off[s + 1]] for s in range(len(off) - 1)]
    mode, budget, min_size = [int(x) for x in g[p + "params"]]
    return dict(components=comps, gt=g[p + "gt"], pred=g[p + "pred"], offsets=off, points=pts), ["dominant", "NAIL"][mode], budget, min_size, float(g[p + "threshold"]), p


# ---- the oracle itself -------------------------------------------------------------------------------------------------------------------------
def test_numpy_oracle_equals_reference_golden(golden):
    g = golden("labeling_golden.npz")
    assert int(g["n_cases"]) == N_GOLDEN
    modes = set()
    for k in range(N_GOLDEN):
        cl, mode, budget, min_size, thr, p = _golden_case(g, k)
        modes.add(mode)
        pseudo = g[p + "pseudo_in"].copy()
        w, b, lst = dict.fromkeys(O.COUNTERS, 0), {"click": budget}, [3, 1]
        used = O.oracle_labeling(g[p + "inds"].tolist(), cl["components"], cl["gt"], pseudo, w, mode, cl["pred"], thr, b, min_size, lst)
        assert used == g[p + "used"].tolist() and lst == g[p + "class_list"].tolist()
        assert [w[c] for c in O.COUNTERS] == g[p + "counters"].tolist() and b["click"] == int(g[p + "budget_left"])
        assert np.array_equal(pseudo, g[p + "pseudo_out"])
    assert modes == {"dominant", "NAIL"}


# ---- golden cases through the C ABI and through sampler.oracle_labeling ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(N_GOLDEN))
def test_golden_through_the_c_abi(backend, golden, k):
    g = golden("labeling_golden.npz")
    cl, mode, budget, min_size, thr, p = _golden_case(g, k)
    picks = [(0, int(s)) for s in g[p + "inds"]]
    got = _abi([cl], picks, mode, thr, budget, min_size, pseudo=g[p + "pseudo_in"])
    assert got["rc"] == 0 and int(got["out"][8]) == 0
    assert [s for _, s in got["used"]] == g[p + "used"].tolist()
    assert [3, 1] + got["classes"] == g[p + "class_list"].tolist()
    assert got["out"][:6].tolist() == g[p + "counters"].tolist() and got["budget"] == int(g[p + "budget_left"]) == int(got["out"][7])
    assert np.array_equal(got["pseudo"], g[p + "pseudo_out"])


@pytest.mark.parametrize("k", range(N_GOLDEN))
def test_golden_through_sampler_oracle_labeling(backend, golden, k):
    from ssdr_al import sampler
    g = golden("labeling_golden.npz")
    cl, mode, budget, min_size, thr, p = _golden_case(g, k)
    comps = np.empty(len(cl["components"]), dtype=object)
    for s, c in enumerate(cl["components"]):
        comps[s] = list(c)
    pseudo = g[p + "pseudo_in"].copy()
    w, b, total = dict.fromkeys(O.COUNTERS, 0), {"click": budget}, {"selected_class_list": [3, 1]}
    out, used = sampler.oracle_labeling(superpoint_inds=g[p + "inds"].tolist(), components=comps, input_gt=cl["gt"], pseudo_gt=pseudo, cloud_name="c", w=w,
                                        sampler_args=[mode], prob_class=cl["pred"], threshold=thr, budget=b, min_size=min_size, total_obj=total)
    assert out is pseudo and np.array_equal(pseudo, g[p + "pseudo_out"])
    assert list(used) == g[p + "used"].tolist() and total["selected_class_list"] == g[p + "class_list"].tolist()
    assert [w[c] for c in O.COUNTERS] == g[p + "counters"].tolist() and b["click"] == int(g[p + "budget_left"])


# ---- region sizes: the wave edge, the workgroup edge, the switch between the two forms -------------------------------------------------------------------
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1025, 5000]


def _sized_cloud(rng, sizes):
    """every size three times: one label (passes), two stretches that split cleanly, noise that is ignored"""
    regs = []
    for n in sizes:
        regs.append(O.region(n, [(n, 4, 2)]))
        regs.append(O.region(n, [(0.5, 3, 1), (n, 9, 6)]))
        regs.append((rng.integers(0, 13, n).astype(np.int32), rng.integers(0, 13, n).astype(np.int32)))
    return O.cloud_from_regions(regs, rng)


@pytest.mark.parametrize("mode", ["dominant", "NAIL"])
def test_region_sizes_and_kernel_forms(backend, mode):
    rng = np.random.default_rng(3)
    cl = _sized_cloud(rng, SIZES)
    picks = [(0, int(s)) for s in rng.permutation(3 * len(SIZES))]
    got, exp = _run([cl], picks, mode, 0.9, 1000, 1, profile=True)
    assert {"label_form:wave", "label_form:block", "label_order", "label_scan", "label_apply"} <= got["names"]
    assert int(got["out"][10]) == 3 * sum(n <= 256 for n in SIZES) and int(got["out"][11]) == 3 * sum(n > 256 for n in SIZES)
    if mode == "NAIL":
        assert exp["counters"]["split_sp_num"] >= 7 and exp["counters"]["ignore_sp_num"] >= 7 and exp["counters"]["sp_num"] >= 10
    # regions of at most 256 points, and the caller says so: the workgroup form is not launched
    small = _sized_cloud(rng, [s for s in SIZES if s <= 256])
    picks = [(0, s) for s in range(len(small["components"]))]
    got, _ = _run([small], picks, mode, 0.9, 1000, 1, profile=True)
    assert "label_form:wave" in got["names"] and "label_form:block" not in got["names"]
    assert int(got["out"][10]) == len(picks) and int(got["out"][11]) == 0
    # without a bound both forms are launched; the workgroup form finds nothing to do
    got, _ = _run([small], picks, mode, 0.9, 1000, 1, profile=True, max_region=0)
    assert "label_form:block" in got["names"] and int(got["out"][11]) == 0


# ---- rule edges --------------------------------------------------------------------------------------------------------------------------------
def test_rule_edges(backend):
    R = O.region
    regs = [
        R(5, [(5, 2, 0)]),                                   # 0: len == min_size: used
        R(4, [(4, 2, 0)]),                                   # 1: min_size - 1: skipped, free
        R(10, [(9, 6, 1), (1, 7, 1)]),                       # 2: 9 of 10 at 0.9: passes
        R(100, [(89, 6, 1), (11, 7, 1)]),                    # 3: 89 of 100: does not; one class: the sub-region fails too -> ignored
        R(12, [(6, 8, 3), (6, 5, 4)]),                       # 4: two labels tied (lowest wins in dominant mode); sub-regions of 6 > 5: split
        R(10, [(5, 8, 3), (5, 5, 4)]),                       # 5: sub-regions of exactly min_size points: too small -> ignored
        R(12, [(4, 9, 0), (4, 3, 0), (4, 11, 0)]),           # 6: three labels tied
        R(40, [(14, 1, 2), (14, 2, 7), (12, 3, 12)]),        # 7: predicted classes with gaps, the highest class id of 13
        R(30, [(30, 12, 12)]),                               # 8: one class, one label, the highest ids
        R(14, [(6, 0, 0), (8, 1, 5)]),                       # 9: one sub-region of min_size + 1 passes, the other (6 > 5) too
        R(20, [(11, 4, 1), (9, 6, 1)]),                      # 10: all one predicted class, impure: ignored
    ]
    cl = O.cloud_from_regions(regs, np.random.default_rng(0))
    picks = [(0, s) for s in range(len(regs))]
    for mode in ("dominant", "NAIL"):
        got, exp = _run([cl], picks, mode, 0.9, 100, 5)
        assert got["used_flags"].tolist() == [1, 0] + [1] * 9
    assert exp["counters"] == dict(sp_num=3, p_num=45, sub_num=7, sub_p_num=66, split_sp_num=3, ignore_sp_num=4)
    assert exp["class_list"] == [2, 6, 8, 5, 1, 2, 3, 12, 0, 1] and exp["budget_left"] == 100 - 10 - 7
    dom = _expect([cl], picks, "dominant", 0.9, 100, 5)
    assert dom["class_list"] == [2, 6, 6, 5, 5, 3, 1, 12, 1, 4]      # ties: the lowest label
    # the bounds of the id ranges: label 63, class 31
    hi = O.cloud_from_regions([R(20, [(10, 63, 31), (10, 62, 30)]), R(9, [(9, 63, 31)])])
    got, exp = _run([hi], [(0, 0), (0, 1)], "NAIL", 0.9, 10, 3, nl=64, nc=32)
    assert exp["class_list"] == [62, 63, 63]


# ---- budget -------------------------------------------------------------------------------------------------------------------------------------
def test_budget(backend):
    R = O.region
    whole, small = R(10, [(10, 2, 1)]), R(2, [(2, 2, 1)])
    split3 = R(30, [(10, 1, 0), (10, 2, 1), (10, 3, 2)])                 # costs 1 + 3
    cl = O.cloud_from_regions([whole, small, split3, R(8, [(8, 5, 5)]), R(12, [(12, 6, 6)])], np.random.default_rng(1))
    picks = [(0, 1), (0, 0), (0, 1), (0, 3), (0, 0), (0, 2), (0, 1), (0, 4), (0, 3)]      # zero-cost items everywhere, region 0 twice
    for budget in (0, -3, 1, 2, 3, 4, 5, 100):
        got, exp = _run([cl], picks, "NAIL", 0.9, budget, 5)
    assert exp["budget_left"] == 100 - 9 and exp["used"] == [(0, 0), (0, 3), (0, 0), (0, 2), (0, 4), (0, 3)]
    got, exp = _run([cl], picks, "NAIL", 0.9, 0, 5)
    assert exp["used"] == [] and got["budget"] == 0 and not got["pseudo"].any()
    # the split region is reached with one click left and pays four: the items behind it are untouched
    got, exp = _run([cl], picks, "NAIL", 0.9, 4, 5)
    assert exp["budget_left"] == -3 and exp["used"][-1] == (0, 2) and not got["used_flags"][6:].any()
    assert not got["pseudo"][0][cl["components"][4]].any()
    got, exp = _run([cl], [(0, 0), (0, 2), (0, 4)], "NAIL", 0.9, 3, 5)
    assert exp["budget_left"] == -2 == got["budget"] and not got["used_flags"][2] and exp["used"] == [(0, 0), (0, 2)] and got["classes"] == [2, 1, 2, 3]
    # the same region twice pays twice
    got, exp = _run([cl], [(0, 0), (0, 0), (0, 0)], "dominant", 0.9, 2, 5)
    assert exp["used"] == [(0, 0), (0, 0)] and exp["counters"]["sp_num"] == 2 and got["classes"] == [2, 2]
    # no items at all
    got, exp = _run([cl], [], "NAIL", 0.9, 7, 5)
    assert got["budget"] == 7 and got["classes"] == []


# ---- order ---------------------------------------------------------------------------------------------------------------------------------------
def test_interleaved_clouds_are_grouped_by_first_appearance(backend):
    rng = np.random.default_rng(8)
    clouds = [O.noisy_cloud(rng, rng.integers(4, 50, 12)) for _ in range(3)]
    picks = [(2, 5), (0, 1), (2, 0), (1, 7), (0, 3), (1, 2), (2, 9), (0, 0), (1, 1), (2, 5)]
    for budget in (4, 8, 100):
        got, exp = _run(clouds, picks, "NAIL", 0.8, budget, 4)
        assert got["proc"].tolist() == [0, 2, 6, 9, 1, 4, 7, 3, 5, 8]    # cloud 2, 0, 1: neither the pick order nor the cloud ids
    # a caller's cloud key (the edcd round's file_list_top order): 1, 2, 0
    got = _abi(clouds, picks, "NAIL", 0.8, 6, 4, cloud_key=[40, 3, 17])
    exp = _expect(clouds, picks, "NAIL", 0.8, 6, 4, cloud_order=[1, 2, 0])
    _same(got, exp, clouds)
    assert got["proc"].tolist() == [3, 5, 8, 0, 2, 6, 9, 1, 4, 7]


# ---- rounds: every selector, then the labelling, then the next round ------------------------------------------------------------------------------------
FPS_ARGS = ("sb", "WetSU", "clsbal", "gcn_fps")
EDCD_ARGS = ("sb", "WetSU", "clsbal", "edcd")


def _cfg(nc=13):
    from ssdr_al.helper_tool import ConfigS3DIS

    class Cfg(ConfigS3DIS):
        num_classes = nc
    return Cfg


def _oracle_picks(clouds, labelled, class_list, selector, batch, min_size):
    """the round's picks [(cloud, region)] in the order sampling() meets them, and the edcd round's cloud order"""
    from oracle import pipeline_np as P
    if selector in ("fps", "kcenter"):
        r = P.selection_round(clouds, labelled, class_list, 13, list(FPS_ARGS), min_size, 2, batch, 1, 0, 0, np.random.RandomState(0), selector=selector)
        return r["selected"], None
    if selector == "topk":
        r = P.selection_round(clouds, labelled, class_list, 13, list(FPS_ARGS), min_size, 2, batch, 1, 0, 0, np.random.RandomState(0), graph_clouds=set())
        return [r["region"][i] for i in r["sorted_inds"][: min(batch, len(r["region"]))]], None
    from test_region_selectors import _oracle
    r, ntop, exp = _oracle(clouds, labelled, class_list, EDCD_ARGS, batch, min_size=min_size)
    top = [r["region"][i][0] for i in r["sorted_inds"][: min(batch, len(r["region"]))]]
    return [r["unl"][i] for _, seq in exp for i in seq], list(dict.fromkeys(top))


def _oracle_clouds(hp):
    """what _help() reads per cloud, from the HotPath's arrays: components, ground truth, predicted classes"""
    gt, pred = hp.tile_l.to_host().reshape(-1), hp.cls.to_host()
    out = []
    for b in range(hp.B):
        lo, hi = hp.sp_base[b], (hp.sp_base[b + 1] if b + 1 < hp.B else hp.S)
        p0, p1 = int(hp.pt_off[b]), int(hp.pt_off[b + 1])
        comps = [hp.sp_pts_h[hp.sp_off_h[s]:hp.sp_off_h[s + 1]].astype(np.int64) - p0 for s in range(lo, hi)]
        out.append(dict(components=comps, gt=gt[p0:p1], pred=pred[p0:p1]))
    return out


def _check_label(hp, res, exp, labelled_before):
    assert res.used == exp["used"]
    assert res.counters == exp["counters"] and res.budget_left == exp["budget_left"]
    assert hp.selected_class_list.to_host().tolist() == exp["class_list"]
    for b in range(hp.B):
        assert np.array_equal(res.to_host(b), exp["pseudo"][b]) and res.to_host(b).dtype == np.float32
    labelled = [set(l) | {s for c, s in exp["used"] if c == b} for b, l in enumerate(labelled_before)]
    base = hp.sp_base
    assert [sorted(int(s) - base[b] for s in hp.labeled[b]) for b in range(hp.B)] == [sorted(l) for l in labelled]
    mask = np.zeros(hp.S, bool)
    for b, l in enumerate(labelled):
        mask[[base[b] + s for s in l]] = True
    assert np.array_equal(hp.labeled_mask, mask) and np.array_equal(hp.skip_mask, mask | (hp.sp_size_h < hp.min_size))
    return labelled


@pytest.mark.parametrize("selector,host_rule", [("fps", False), ("kcenter", False), ("edcd", False), ("topk", False),
                                                ("fps", True), ("kcenter", True), ("edcd", True), ("topk", True)])
def test_round_label_and_next_round(backend, selector, host_rule, monkeypatch):
    """the picks of each selector (device rule: from the chain's result buffer; host rule: uploaded), labelled, and the next round on the updated state:
    it selects what the oracle does and what a fresh HotPath over the labelled sets and the class list the first round ended with does"""
    from ssdr_al import pipeline
    if host_rule:
        monkeypatch.setenv("SSDR_SELECT_HOST_RULE", "1")
    clouds, labelled, sel_list = make_clouds(31, 4, 36, 3, 40, labelled_per_cloud=6)
    batch, min_size = 24, 5
    kw = dict(sampler_args=EDCD_ARGS if selector == "edcd" else FPS_ARGS, selector=selector, min_size=min_size, batch_size=batch, round_num=2, label_seed=0)
    hp = pipeline.HotPath.from_clouds(clouds, labelled, sel_list, _cfg(), **kw)
    class_list = sel_list.tolist()
    for rnd in range(2):
        sel, unl = hp.step_selection()
        assert hp.rule_path == ("host" if host_rule else "device")
        picks, cloud_order = _oracle_picks(clouds, labelled, np.asarray(class_list), selector, batch, min_size)
        assert hp.selected == picks                          # (round 2: the hand-over — labelled set, skip mask, class list — is the oracle's)
        if rnd == 1:          # nothing of the first selection is left on the object
            fresh = pipeline.HotPath.from_clouds(clouds, labelled, np.asarray(class_list), _cfg(), **kw)
            fsel, funl = fresh.step_selection()
            assert np.array_equal(fsel, sel) and funl == unl and fresh.selected == hp.selected
            break
        oc = _oracle_clouds(hp)
        exp = O.label_round(picks, oc, [np.zeros((2, len(c["gt"])), np.float32) for c in oc], "NAIL", 0.6, batch - 5, min_size, class_list, cloud_order)
        res = hp.label_selected(mode="NAIL", threshold=0.6, budget=batch - 5)
        assert exp["counters"]["sp_num"] > 0 and len(exp["used"]) < len(picks)
        labelled = _check_label(hp, res, exp, labelled)
        class_list = exp["class_list"]
        with pytest.raises(RuntimeError):
            hp.label_selected()                              # these picks are spent


def test_label_selected_defaults_and_persistent_pseudo_labels(backend):
    """budget defaults to the round's batch_size, min_size to the HotPath's; the pseudo labels persist from round to round and may be given"""
    from ssdr_al import pipeline
    clouds, labelled, sel_list = make_clouds(5, 3, 30, 3, 40, labelled_per_cloud=4)
    hp = pipeline.HotPath.from_clouds(clouds, labelled, sel_list, _cfg(), sampler_args=FPS_ARGS, selector="topk", min_size=4, batch_size=10, round_num=2)
    n = hp.n_pts
    init = np.zeros((2, n), np.float32); init[:, ::7] = np.array([[1.0], [11.0]], np.float32)
    hp.set_pseudo_gt(init)
    class_list, pseudo = sel_list.tolist(), None
    for rnd in range(2):
        hp.step_selection()
        picks = [(hp.room_ids.index(r), s) for r, s in hp.selected]
        oc = _oracle_clouds(hp)
        if pseudo is None:
            pseudo = [init[:, int(hp.pt_off[b]): int(hp.pt_off[b + 1])].copy() for b in range(hp.B)]
        exp = O.label_round(picks, oc, pseudo, "dominant", 0.9, 10, 4, class_list)
        res = hp.label_selected(mode="dominant")
        labelled = _check_label(hp, res, exp, labelled)
        class_list, pseudo = exp["class_list"], exp["pseudo"]
        assert res.budget_left == 0 and len(res.used) == 10 and np.array_equal(res.to_host(), np.concatenate(pseudo, axis=1))


def test_al_round_label(emu_lib):
    """ALRound.label() over the round's arrays, the small configuration of test_al_round.py on the CPU logic build"""
    from oracle import randla_np as R
    from ssdr_al import _lib, pipeline, synthetic
    from ssdr_al.helper_tool import ConfigS3DIS
    _lib.use(emu_lib)
    try:
        class Cfg(ConfigS3DIS):
            num_points = 512
        rooms = [synthetic.make_room(8100 + i, density=70.0) for i in range(2)]
        ar = pipeline.ALRound(R.init_weights(0), rooms, 2, Cfg, batch_size=24, round_num=2, labeled_per_tile=3, precision="f32")
        ar.run()
        S = ar.sel
        picks = list(S.selected)
        labelled = [set(int(x) - S.sp_base[t] for x in S.labeled[t]) for t in range(S.B)]
        oc = _oracle_clouds(S)
        exp = O.label_round(picks, oc, [np.zeros((2, 512), np.float32) for _ in oc], "NAIL", 0.7, 24, 1, S.selected_class_list.to_host().tolist())
        res = ar.label(mode="NAIL", threshold=0.7)
        _check_label(S, res, exp, labelled)
        assert len(exp["used"]) > 0
        sel2, _ = ar.run()                                   # the next round runs on the updated state
        assert len(sel2) == 24 and not set(S.selected) & set(exp["used"])
    finally:
        _lib.use(None)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(backend):
    from ssdr_al import _lib, pipeline, sampler
    cl = O.cloud_from_regions([O.region(10, [(10, 2, 1)]), O.region(12, [(6, 14, 1), (6, 2, 20)])])
    assert _abi([cl], [(0, 0)], "part_do", 0.9, 5, 1)["rc"] == 1          # SSDR_ERR_INVALID
    with pytest.raises(_lib.SsdrError) as e:
        sampler.oracle_labeling([0], cl["components"], cl["gt"], np.zeros((2, 22), np.float32), "c", {}, ["domi_prec"], cl["pred"], 0.9, {"click": 3}, 1, {})
    assert e.value.status == 1
    got = _abi([cl], [(0, 0), (0, 1)], "NAIL", 0.9, 5, 1)                 # label 14 of 13, class 20 of 13: status bits, nothing indexed
    assert got["rc"] == 0 and int(got["out"][8]) == 3
    with pytest.raises(ValueError):
        sampler.oracle_labeling([0, 1], cl["components"], cl["gt"], np.zeros((2, 22), np.float32), "c", {}, ["NAIL"], cl["pred"], 0.9, {"click": 3}, 1, {},
                                num_labels=13, num_classes=13)
    assert _abi([cl], [(0, 0), (0, 1)], "NAIL", 0.9, 5, 1, nl=15, nc=21)["out"][8] == 0
    assert _abi([cl], [(0, 0)], "NAIL", 0.9, 5, 1, nl=65)["rc"] == 1 and _abi([cl], [(0, 0)], "NAIL", 0.9, 5, 1, nc=33)["rc"] == 1
    # a class list that is too short: status 8, nothing written behind it
    got = _abi([cl], [(0, 0), (0, 0), (0, 0)], "dominant", 0.9, 5, 1, class_cap=2)
    assert int(got["out"][8]) == 8 and int(got["out"][6]) == 3
    # a selection made with a communicator is refused
    clouds, labelled, sel_list = make_clouds(2, 2, 12, 3, 20, labelled_per_cloud=2)
    hp = pipeline.HotPath.from_clouds(clouds, labelled, sel_list, _cfg(), selector="topk", batch_size=4)
    hp.step_selection()
    hp._collected.comm = object()
    with pytest.raises(ValueError, match="communicator"):
        hp.label_selected()


def test_new_symbols_in_both_libraries(emu_lib):
    from conftest import GPU_LIB
    for path in (emu_lib, GPU_LIB):
        lib = C.CDLL(path)
        assert hasattr(lib, "ssdr_oracle_label_dev") and hasattr(lib, "ssdr_oracle_label_items_dev")
