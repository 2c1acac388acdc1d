"""The labelling chain in two halves (the sharded AL round's oracle): ssdr_oracle_label_verdict_dev + ssdr_oracle_label_walk_dev with the ranks emulated
in one process == ssdr_oracle_label_dev over the union of the clouds == the NumPy oracle.  Everything is integers and exact 0 / 1 / label values:
compared for equality.  `backend` runs every case on the CPU logic build and (-m gpu) on the gfx950 build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _labeling_oracle as O
import _sharded_label_case as H

SPECIAL = (1, 255, 256, 257, 5000)            # below min_size, the wave form's last two sizes, the workgroup form's first, a large region
MAX_ITEMS = {1: 2400, 2: 1200, 3: 1000}       # per rank; world 3: the 1 024-record chunks of the scan end inside rank 1's and rank 2's records, dead slots between
MIN_SIZE, THR = 4, 0.8
_case = {}


def _big_case():
    """12 clouds of ~190 small regions, the special sizes in three of them (one per rank at world 3), ~2 200 picks: all special regions, one of them and a
    few small ones twice, the rest at random — the clouds of all ranks interleave in the walk"""
    if "big" not in _case:
        rng = np.random.default_rng(20)
        clouds = []
        for c in range(12):
            sizes = rng.integers(3, 40, 190).tolist() + (list(SPECIAL) if c in (1, 6, 10) else [])
            clouds.append(O.noisy_cloud(rng, sizes))
        picks = [(c, 190 + k) for c in (1, 6, 10) for k in range(len(SPECIAL))]
        allr = [(c, s) for c in range(12) for s in range(190)]
        picks += [allr[i] for i in rng.choice(len(allr), 2175, replace=False)]
        picks += [(6, 190 + 4), picks[40], picks[41], picks[900]]                # a region picked twice (the 5 000-point one among them)
        picks = [picks[i] for i in rng.permutation(len(picks))]
        _case["big"] = (clouds, picks, rng.permutation(12) * 7 + 3)
    return _case["big"]


def _budgets(clouds, picks, mode, cloud_order, owner):
    """0, 1, above the total cost and — from the oracle's costs — one that ends inside a split region owned by another rank than the previous item's"""
    order, cost = H.walk_costs(clouds, picks, mode, THR, MIN_SIZE, cloud_order)
    before = np.concatenate([[0], np.cumsum(cost)])
    out = [0, 1, int(cost.sum()) + 5, int(before[1100]) + 1]
    cut = None
    if mode == "NAIL":
        one = len(set(owner.values())) == 1                  # (world 1: any split region)
        hits = [j for j in range(1, len(order)) if cost[j] >= 3 and (one or owner[order[j][0]] != owner[order[j - 1][0]])]
        assert hits, "the case has no split region at a change of ranks"
        cut = int(before[hits[len(hits) // 2]]) + 1
        out.append(cut)
    return out, cut, len(order)


@pytest.mark.parametrize("keys", ["first", "rank"])
@pytest.mark.parametrize("mode", ["dominant", "NAIL"])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_two_halves_equal_the_one_call_chain(backend, world, mode, keys):
    clouds, picks, ckey = _big_case()
    assert 2150 <= len(picks) <= 2250
    shares = H.split_clouds(len(clouds), world)
    cloud_key = ckey if keys == "rank" else None
    cloud_order = None if cloud_key is None else [int(c) for c in np.argsort(cloud_key)]
    sh = H.Sharded(clouds, shares, picks, MAX_ITEMS[world], cloud_key)
    assert all(R["n_items"] <= MAX_ITEMS[world] for R in sh.ranks) and (world < 3 or all(R["n_items"] < 1000 for R in sh.ranks))
    # the clouds of different ranks interleave in the walk
    if world > 1:
        seq = [sh.owner[c] for c, _ in O.help_order(picks, cloud_order)]
        assert sum(a != b for a, b in zip(seq, seq[1:])) >= 2          # (A, B, A at least)
    assert sh.verdicts(mode, THR, MIN_SIZE) == [0] * world
    rec = sh.records()
    for r, R in enumerate(sh.ranks):
        k = R["n_items"]
        assert (rec[r]["key"][k:] == H.DEAD).all() and not rec[r]["cost"][k:].any() and not rec[r]["kind"][k:].any()      # dead slots
        assert np.array_equal(rec[r]["key"][:k], sh.keys[r][1]) and np.array_equal(rec[r]["pos"], np.arange(sh.M))
        assert not rec[r]["status"].any()
    budgets, cut, n_walk = _budgets(clouds, picks, mode, cloud_order, sh.owner)
    for budget in budgets:
        ref = H.one_call(clouds, picks, mode, THR, budget, MIN_SIZE, cloud_key=cloud_key)
        res = sh.walk(budget)
        m = H.assert_halves_equal_one_call(sh, res, ref)
        if budget in (0, cut, budgets[2]):                   # ... and the one-call chain against the NumPy oracle
            exp = O.label_round(picks, clouds, [np.zeros((2, len(c["gt"])), np.float32) for c in clouds], mode, THR, budget, MIN_SIZE, [], cloud_order)
            assert [picks[i] for i in ref["proc"] if ref["used"][i]] == exp["used"] and ref["classes"] == exp["class_list"]
            assert ref["budget"] == exp["budget_left"] and np.array_equal(ref["pseudo"], np.concatenate(exp["pseudo"], axis=1))
            if budget == 0:
                assert not exp["used"] and (m["walk_pos"] == -1).all()
            elif budget == cut:
                assert exp["budget_left"] < 0                # ends inside a split region, owned by another rank than the item before it
            else:
                assert exp["budget_left"] == 5 and (m["walk_pos"] >= 0).all() and len(exp["used"]) < n_walk      # (the 1-point regions are skipped)
    # both forms ran: regions of 1 (skipped), 255, 256 (wave), 257, 5 000 (workgroup) points
    assert int(ref["out"][11]) == 7 and 2000 < int(ref["out"][10]) <= len(picks) - 7 - 3


def test_a_rank_without_items_and_tiny_worlds(backend):
    """world 3 with no pick on rank 1 (its slice is dead records only, between the live records of ranks 0 and 2); no item at all; max_items == 1"""
    rng = np.random.default_rng(4)
    clouds = [O.noisy_cloud(rng, rng.integers(3, 300, 25)) for _ in range(6)]
    picks = [(int(c), int(s)) for c, s in zip(rng.choice([0, 1, 4, 5], 60), rng.integers(0, 25, 60))]
    for mode in ("dominant", "NAIL"):
        sh = H.Sharded(clouds, H.split_clouds(6, 3), picks, 40)
        assert sh.ranks[1]["n_items"] == 0 and sh.verdicts(mode, THR, MIN_SIZE) == [0, 0, 0]
        assert (sh.records()[1]["key"] == H.DEAD).all()
        for budget in (0, 7, 31, 1000):
            H.assert_halves_equal_one_call(sh, sh.walk(budget), H.one_call(clouds, picks, mode, THR, budget, MIN_SIZE))
    sh = H.Sharded(clouds, H.split_clouds(6, 2), [], 5)
    assert sh.verdicts("NAIL", THR, MIN_SIZE) == [0, 0]
    H.assert_halves_equal_one_call(sh, sh.walk(9), H.one_call(clouds, [], "NAIL", THR, 9, MIN_SIZE))
    sh = H.Sharded(clouds, H.split_clouds(6, 2), [], 0)                        # no slot at all: nothing is launched but the scan
    assert sh.verdicts("NAIL", THR, MIN_SIZE) == [0, 0]
    res = sh.walk(9)
    assert all(x["rc"] == 0 and x["budget"] == 9 and x["out"].tolist() == [0] * 7 + [9, 0, 0, 0, 0] for x in res)
    sh = H.Sharded(clouds, H.split_clouds(6, 3), [(5, 3), (0, 2), (3, 1)], 1)
    assert sh.verdicts("NAIL", THR, MIN_SIZE) == [0, 0, 0]
    H.assert_halves_equal_one_call(sh, sh.walk(2), H.one_call(clouds, [(5, 3), (0, 2), (3, 1)], "NAIL", THR, 2, MIN_SIZE))


def test_more_than_16384_records_take_the_wide_sort_passes(backend):
    """world 2 x 8 200 slots: from 16 384 records on the sort of the 64-bit walk keys runs its high digits as wide passes too (the cloud keys vary up
    there); few live items, so the case stays small"""
    rng = np.random.default_rng(9)
    clouds = [O.noisy_cloud(rng, rng.integers(3, 80, 40)) for _ in range(6)]
    picks = [(int(c), int(s)) for c, s in zip(rng.integers(0, 6, 300), rng.integers(0, 40, 300))]
    ckey = rng.permutation(6) * 100003 + 70000                                  # cloud keys beyond 16 bits: several high digits differ
    for cloud_key in (None, ckey):
        sh = H.Sharded(clouds, H.split_clouds(6, 2), picks, 8200, cloud_key)
        assert sh.W * sh.M >= 16384 and sh.verdicts("NAIL", THR, MIN_SIZE) == [0, 0]
        for budget in (150, 10 ** 6):
            H.assert_halves_equal_one_call(sh, sh.walk(budget, class_cap=4000), H.one_call(clouds, picks, "NAIL", THR, budget, MIN_SIZE, cloud_key=cloud_key, class_cap=4000))


def test_pseudo_labels_and_labelled_mask_are_updated_in_place(backend):
    rng = np.random.default_rng(11)
    clouds = [O.noisy_cloud(rng, rng.integers(3, 60, 20)) for _ in range(4)]
    picks = [(int(c), int(s)) for c, s in zip(rng.integers(0, 4, 30), rng.integers(0, 20, 30))]
    n, S = sum(len(c["gt"]) for c in clouds), 80
    pseudo = np.zeros((2, n), np.float32); pseudo[:, ::5] = np.array([[1.0], [12.0]], np.float32)
    labeled = rng.random(S) < 0.3
    sh = H.Sharded(clouds, H.split_clouds(4, 2), picks, 32, labeled=labeled, pseudo=pseudo)
    assert sh.verdicts("NAIL", THR, MIN_SIZE) == [0, 0]
    ref = H.one_call(clouds, picks, "NAIL", THR, 14, MIN_SIZE, labeled=labeled, pseudo=pseudo)
    m = H.assert_halves_equal_one_call(sh, sh.walk(14), ref)
    assert m["labeled"][labeled].all() and m["labeled"].sum() > labeled.sum()


def test_class_cap_one_too_small_and_out_of_range_ids(backend):
    R = O.region
    a = O.cloud_from_regions([R(10, [(10, 2, 1)]), R(30, [(10, 1, 0), (10, 2, 1), (10, 3, 2)]), R(8, [(8, 5, 5)])], np.random.default_rng(1))
    b = O.cloud_from_regions([R(12, [(12, 6, 6)]), R(20, [(10, 4, 3), (10, 7, 8)])], np.random.default_rng(2))
    picks = [(0, 0), (1, 1), (0, 1), (1, 0), (0, 2)]
    sh = H.Sharded([a, b], [[0], [1]], picks, 4)
    assert sh.verdicts("NAIL", 0.9, 5) == [0, 0]
    full = H.one_call([a, b], picks, "NAIL", 0.9, 100, 5)
    n_ent = int(full["out"][6])
    assert n_ent == 8 and int(full["out"][8]) == 0
    ref = H.one_call([a, b], picks, "NAIL", 0.9, 100, 5, class_cap=n_ent - 1)
    res = sh.walk(100, class_cap=n_ent - 1)
    assert int(ref["out"][8]) == 8 and all(int(x["out"][8]) == 8 and int(x["out"][6]) == n_ent for x in res)      # status 8 on every rank, nothing behind the capacity
    H.assert_halves_equal_one_call(sh, res, ref)
    # label 14 of 13 (rank 0), class 20 of 13 (rank 1): the status bits of both ranks on every rank, nothing indexed
    c0 = O.cloud_from_regions([R(10, [(10, 2, 1)]), R(12, [(6, 14, 1), (6, 2, 3)])])
    c1 = O.cloud_from_regions([R(12, [(6, 3, 20), (6, 2, 1)]), R(9, [(9, 1, 1)])])
    picks = [(0, 0), (1, 0), (0, 1), (1, 1)]
    sh = H.Sharded([c0, c1], [[0], [1]], picks, 3)
    assert sh.verdicts("NAIL", 0.9, 1) == [0, 0]
    rec = sh.records()
    assert (rec[0]["status"] == 1).all() and (rec[1]["status"] == 2).all()
    ref = H.one_call([c0, c1], picks, "NAIL", 0.9, 5, 1)
    res = sh.walk(5)
    assert int(ref["out"][8]) == 3 and all(int(x["out"][8]) == 3 for x in res)
    H.assert_halves_equal_one_call(sh, res, ref)
    # an item outside the regions, a point id outside the points: bit 4, nothing indexed
    sh = H.Sharded([c0, c1], [[0], [1]], picks, 3)
    from ssdr_al._lib import DevArray
    sh.ranks[1]["items"] = DevArray.from_host(np.array([0, 77, 0], np.int32))
    assert sh.verdicts("NAIL", 0.9, 1) == [0, 0]
    rec = sh.records()
    assert (rec[1]["status"] & 4).all() and rec[1]["kind"][1] == 0 and rec[1]["cost"][1] == 0 and not (rec[0]["status"] & 4).any()
    res = sh.walk(5)
    assert all(int(x["out"][8]) & 4 for x in res) and res[1]["used"].tolist()[:2] == [1, 0]
    sh = H.Sharded([c0, c1], [[0], [1]], picks, 3)
    pts = sh.ranks[0]["pts"].to_host(); pts[3] = 10 ** 6; pts[7] = -2
    sh.ranks[0]["pts"] = DevArray.from_host(pts)
    assert sh.verdicts("NAIL", 0.9, 1) == [0, 0] and (sh.records()[0]["status"] & 4).all()
    assert all(x["rc"] == 0 and int(x["out"][8]) & 4 for x in sh.walk(5))


def test_refusals_of_the_two_halves(backend):
    """bad arguments: SSDR_ERR_INVALID, nothing launched (the record buffer and the outputs keep their fill)"""
    from ssdr_al import _lib
    L = _lib.lib()
    cl = O.cloud_from_regions([O.region(10, [(10, 2, 1)]), O.region(12, [(6, 4, 1), (6, 2, 3)])])
    sh = H.Sharded([cl], [[0]], [(0, 0), (0, 1)], 2)
    before = sh.rec.to_host().copy()
    assert sh.verdicts("part_do", 0.9, 1) == [1] and sh.verdicts("NAIL", 0.9, 1, nl=65) == [1] and sh.verdicts("NAIL", 0.9, 1, nc=33) == [1]
    assert sh.verdicts("NAIL", float("nan"), 1) == [1]
    R = sh.ranks[0]
    assert L.ssdr_oracle_label_verdict_dev(R["gt"].ptr, None, R["n"], R["off"].ptr, R["pts"].ptr, R["S"], R["items"].ptr, R["cnt"].ptr, 2, R["keys"].ptr, 0, 13, 13, 1, 0.9,
                                           1, sh.rec.ptr, None) == 1           # NAIL without predicted classes
    assert L.ssdr_oracle_label_verdict_dev(R["gt"].ptr, R["pred"].ptr, R["n"], R["off"].ptr, R["pts"].ptr, R["S"], R["items"].ptr, R["cnt"].ptr, 2, None, 0, 13, 13, 1, 0.9,
                                           1, sh.rec.ptr, None) == 1           # no keys
    assert np.array_equal(sh.rec.to_host(), before)
    assert sh.verdicts("NAIL", 0.9, 1) == [0]
    good = sh.walk(5)[0]
    assert good["rc"] == 0 and good["used"].tolist() == [1, 1]
    from ssdr_al._lib import DevArray
    for rank, world in ((1, 1), (-1, 1), (0, 0), (3, 2)):
        out = DevArray.from_host(np.full(12, -9, np.int64)); bud = DevArray.from_host(np.array([5], np.int64))
        z = DevArray.from_host(np.zeros(64, np.float32)); u8 = DevArray.from_host(np.full(64, 7, np.uint8)); i4 = DevArray.from_host(np.full(64, -5, np.int32))
        rc = L.ssdr_oracle_label_walk_dev(sh.rec.ptr, rank, world, R["pred"].ptr, R["n"], R["off"].ptr, R["pts"].ptr, R["S"], R["items"].ptr, R["cnt"].ptr, 2, 0, 13,
                                          bud.ptr, z.ptr, z.ptr, u8.ptr, u8.ptr, i4.ptr, 60, i4.ptr, out.ptr, None)
        _lib.sync()
        assert rc == 1 and (out.to_host() == -9).all() and (u8.to_host() == 7).all() and (i4.to_host() == -5).all() and not z.to_host().any()
    assert sh.walk(5, nc=33)[0]["rc"] == 1 and sh.walk(5, nc=0)[0]["rc"] == 1


def test_keys_entry_against_the_host_keys(backend):
    """ssdr_oracle_label_keys_dev: the picks of a replicated global selection -> this rank's items in pick order with (first appearance << 32 | pick position);
    a rank's own picks -> (cloud key << 32 | position); more picks than one 1 024 sweep of the ordered compaction"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    L = _lib.lib()
    rng = np.random.default_rng(6)
    W, Smax, Bmax = 3, 900, 5
    S_r = [900, 640, 777]
    gcloud = np.full(W * Smax, -1, np.int32)
    for r in range(W):
        gcloud[r * Smax: r * Smax + S_r[r]] = r * Bmax + np.sort(rng.integers(0, Bmax - (r == 1), S_r[r]))
    live = np.flatnonzero(gcloud >= 0)
    cand = rng.permutation(live)[:1800].astype(np.int32)
    picks = rng.permutation(1800)[:1500].astype(np.int32)
    picks[7], picks[1030] = -1, 1800                                            # an unset pick, a pick beyond the list: neither is anybody's item
    d_gc, d_cand, d_picks, d_ng = DevArray.from_host(gcloud), DevArray.from_host(cand), DevArray.from_host(picks), DevArray.from_host(np.array([1800], np.int32))
    ok = (picks >= 0) & (picks < 1800)
    gid = np.where(ok, cand[np.clip(picks, 0, 1799)], -1)
    first = {}
    for i, g in enumerate(gid):
        if g >= 0:
            first.setdefault(int(gcloud[g]), i)
    for r in range(W):
        mine = np.flatnonzero((gid >= 0) & (gid // Smax == r))
        M = len(mine) + 3
        d_items, d_n, d_keys = DevArray.from_host(np.full(M, -3, np.int32)), DevArray.from_host(np.array([-1], np.int32)), DevArray.from_host(np.zeros(M, np.uint64))
        assert L.ssdr_oracle_label_keys_dev(d_picks.ptr, 1500, d_ng.ptr, d_cand.ptr, 1800, d_gc.ptr, Smax, W * Bmax, r, W, None, d_items.ptr, d_n.ptr, M, d_keys.ptr, None) == 0
        _lib.sync()
        assert int(d_n.to_host()[0]) == len(mine) > 300
        assert np.array_equal(d_items.to_host()[: len(mine)], gid[mine] - r * Smax) and (d_items.to_host()[len(mine):] == -3).all()
        exp = np.array([(first[int(gcloud[gid[i]])] << 32) | int(i) for i in mine], np.uint64)
        assert np.array_equal(d_keys.to_host()[: len(mine)], exp)
        # the capacity bounds what is written
        d_items2, d_keys2 = DevArray.from_host(np.full(10, -3, np.int32)), DevArray.from_host(np.zeros(10, np.uint64))
        assert L.ssdr_oracle_label_keys_dev(d_picks.ptr, 1500, d_ng.ptr, d_cand.ptr, 1800, d_gc.ptr, Smax, W * Bmax, r, W, None, d_items2.ptr, d_n.ptr, 8, d_keys2.ptr, None) == 0
        _lib.sync()
        assert int(d_n.to_host()[0]) == 8 and (d_items2.to_host()[8:] == -3).all() and np.array_equal(d_keys2.to_host()[:8], exp[:8])
        # a rank's own picks with a key per global cloud
        ckey = (rng.permutation(W * Bmax) * 11 + 2).astype(np.int32)
        own = np.concatenate([rng.integers(0, S_r[r], 40), [Smax + 5, -1]]).astype(np.int32)
        d_own, d_cnt, d_ck, d_k = DevArray.from_host(own), DevArray.from_host(np.array([42], np.int32)), DevArray.from_host(ckey), DevArray.from_host(np.zeros(42, np.uint64))
        assert L.ssdr_oracle_label_keys_dev(None, 0, None, None, 0, d_gc.ptr, Smax, W * Bmax, r, W, d_ck.ptr, d_own.ptr, d_cnt.ptr, 42, d_k.ptr, None) == 0
        _lib.sync()
        hi = [int(ckey[gcloud[r * Smax + s]]) if 0 <= s < Smax and gcloud[r * Smax + s] >= 0 else 0x7fffffff for s in own]
        assert d_k.to_host().tolist() == [(h << 32) | i for i, h in enumerate(hi)]
    assert L.ssdr_oracle_label_keys_dev(None, 0, None, None, 0, d_gc.ptr, Smax, W * Bmax, 0, W, None, d_own.ptr, d_cnt.ptr, 42, d_k.ptr, None) == 1
    assert L.ssdr_oracle_label_keys_dev(d_picks.ptr, 1500, None, d_cand.ptr, 1800, d_gc.ptr, Smax, W * Bmax, 3, W, None, d_own.ptr, d_cnt.ptr, 42, d_k.ptr, None) == 1


def test_new_symbols_in_both_libraries(emu_lib):
    from conftest import GPU_LIB
    for path in (emu_lib, GPU_LIB):
        lib = C.CDLL(path)
        for name in ("ssdr_oracle_label_verdict_dev", "ssdr_oracle_label_walk_dev", "ssdr_oracle_label_keys_dev"):
            assert hasattr(lib, name), (path, name)


def test_two_halves_under_asan_ubsan():
    """a stand-alone program (tests/hipemu/label_halves_main.cpp) linked with the sanitized objects of the CPU logic build: the two halves at world 3 ==
    the one-call chain, no report"""
    from conftest import PKG, ROOT
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(PKG, "csrc"), "label-halves-san"])
    env = dict(os.environ, OMP_NUM_THREADS="4", ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "hipemu", "label_halves_san")], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
    assert "label halves ok" in r.stdout
