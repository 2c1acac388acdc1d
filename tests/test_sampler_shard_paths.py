"""The sharded draw of the seed, random and label-all samplers, half by half: ssdr_region_draw_count_dev and ssdr_region_draw_sharded_dev of
csrc/select_random.hip with the ranks emulated in ONE process (every input is an argument; a device copy of the ranks' count tables stands in for the
all-gather).  Merged by d_item_pos, the ranks' items, k, L, the remainder, the unlabelled count and each_file_number are those of
_sampler_oracle.iteration over the union of the ranks' clouds.  Every case asserts its input condition from the oracle first; everything is integers and
every comparison is exact.  CPU logic build and -m gpu."""
import numpy as np
import pytest

import _sampler_oracle as SO

RANDOM, ALL = 0, 1
ST_COUNT, ST_ITEMS, ST_CLOUD = 1, 2, 4
UNSUPPORTED = 5            # SSDR_ERR_UNSUPPORTED


class _Rank:
    """one rank's share: region counts of its clouds, the labelled mask over its regions"""
    def __init__(self, regions, labeled):
        self.regions = [int(n) for n in regions]
        self.B, self.S = len(self.regions), int(sum(self.regions))
        self.cloud = np.repeat(np.arange(self.B), self.regions).astype(np.int32)
        self.labeled = np.asarray(labeled, bool).copy()
        assert len(self.labeled) == self.S


def _ranks(seed, shares, lab_p=0.3):
    rng = np.random.default_rng(seed)
    return [_Rank(r, rng.random(int(sum(r))) < lab_p) for r in shares]


def _union(ranks):
    """-> (labelled mask over the union, base of every global cloud, first region of every rank)"""
    lab = np.concatenate([r.labeled for r in ranks])
    base = np.concatenate([[0], np.cumsum([n for r in ranks for n in r.regions])]).astype(np.int64)
    first = np.concatenate([[0], np.cumsum([r.S for r in ranks])]).astype(np.int64)
    return lab, base, first


def _run(ranks, T, click, mode=RANDOM, key_bits=32, seed=5, rnd=2, it=1, max_items=None, clouds=None):
    """both halves for every rank -> per rank dict(items (global ids), pos, n, info, each); clouds: per rank cloud arrays in place of the ranks' own"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    L = _lib.lib()
    W, CS = len(ranks), max(r.B for r in ranks)
    _, _, first = _union(ranks)
    dev, tables = [], []
    for i, r in enumerate(ranks):
        d = dict(lab=DevArray.from_host(r.labeled.astype(np.uint8)), cloud=DevArray.from_host(r.cloud if clouds is None else clouds[i]),
                 u=DevArray.from_host(np.full(CS + 1, -9, np.int32)))
        assert L.ssdr_region_draw_count_dev(d["lab"].ptr, d["cloud"].ptr, r.S, r.B, d["u"].ptr, CS, None) == 0
        _lib.sync()
        tables.append(d["u"].to_host())
        assert (tables[-1][r.B:CS] == 0).all()                   # the slots behind the rank's clouds
        dev.append(d)
    u_all = DevArray.from_host(np.stack(tables))                 # (what the all-gather leaves on every rank)
    cnt = DevArray.from_host(np.array([click], np.int64))
    out = []
    for i, r in enumerate(ranks):
        M = r.S if max_items is None else max_items
        items, pos, n, info = (DevArray.from_host(np.full(max(M, 1), -7, np.int32)), DevArray.from_host(np.full(max(M, 1), -7, np.int32)),
                               DevArray.from_host(np.array([-7], np.int32)), DevArray((8,), np.int64))
        d = dev[i]
        assert L.ssdr_region_draw_sharded_dev(seed, rnd, it, mode, key_bits, int(first[i]), i, W, u_all.ptr, CS, d["lab"].ptr, d["cloud"].ptr, r.S, r.B, T,
                                              cnt.ptr if mode == RANDOM else None, items.ptr, pos.ptr, M, n.ptr, info.ptr, None) == 0
        _lib.sync()
        w = info.to_host()
        each = np.zeros(int(w[0]), np.int32)
        assert L.ssdr_region_draw_shares(None, _lib.ptr(each), len(each)) == 0
        k = int(n.to_host()[0])
        got_items, got_pos = items.to_host(), pos.to_host()
        assert (got_items[k:] == -7).all() and (got_pos[k:] == -7).all()      # nothing behind the live items
        out.append(dict(items=got_items[:k].astype(np.int64) + first[i], pos=got_pos[:k].astype(np.int64), n=k, info=w, each=each, tables=tables))
    return out


def _expected(ranks, T, click, mode, key_bits=32, seed=5, rnd=2, it=1, lab=None):
    lab_u, base, _ = _union(ranks)
    lab = lab_u if lab is None else lab
    if mode == ALL:
        u = np.array([int((~lab[base[c]:base[c + 1]]).sum()) for c in range(len(base) - 1)])
        live = np.flatnonzero(u).tolist()
        return dict(live=live, k=int(u.sum()), each=u[live].astype(np.int64), items=np.flatnonzero(~lab).astype(np.int64), remain=0), lab
    return SO.iteration(seed, rnd, it, T, click, lab, base, key_bits), lab


def _compare(out, exp, lab, ranks):
    _, _, first = _union(ranks)
    merged = sorted((int(p), int(s)) for o in out for p, s in zip(o["pos"], o["items"]))
    assert [p for p, _ in merged] == list(range(len(exp["items"]))), "every position of the union's list once"
    assert [s for _, s in merged] == exp["items"].tolist(), "the ranks' items merged by position"
    for i, o in enumerate(out):
        w = o["info"]
        assert (w[0], w[1], w[2], w[3]) == (len(exp["live"]), exp["k"], len(exp["items"]), exp["remain"]), "L, k, items, remainder on rank %d" % i
        assert w[4] == int((~lab).sum()) - len(exp["items"]) and w[6] == o["n"] and w[7] == 0
        assert np.array_equal(o["each"], exp["each"]), "each_file_number on rank %d" % i
        assert (np.diff(o["pos"]) > 0).all() and ((o["items"] >= first[i]) & (o["items"] < first[i + 1])).all()


def _case(ranks, T, click, mode=RANDOM, key_bits=32, **kw):
    exp, lab = _expected(ranks, T, click, mode, key_bits, **kw)
    out = _run(ranks, T, click, mode, key_bits, **kw)
    _compare(out, exp, lab, ranks)
    assert all(o["info"][5] == 0 for o in out)
    return out, exp


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_first_region_no_multiple_of_the_wave(backend):
    """(a) 70 + 61 regions in 3 + 2 clouds: rank 1's regions hash first_region = 70 + s, its clouds sit behind one padding-free and one short table"""
    ranks = _ranks(1, [[30, 25, 15], [40, 21]])
    assert [r.S for r in ranks] == [70, 61] and 70 % 64 != 0
    out, exp = _case(ranks, 131, 50)
    assert len(exp["live"]) == 5 and all(o["n"] > 0 for o in out)
    # the pick order is the hash of the GLOBAL id: hashing rank 1's local ids gives another list
    lab, base, first = _union(ranks)
    c3 = [s for c, sps in exp["picks"] if c == 3 for s in sps]
    u3 = np.flatnonzero(~lab[base[3]:base[4]]) + base[3]
    assert 1 < len(c3) < len(u3) and c3 != (SO.pick_order(5, 2, 1, u3 - first[1], 32)[: len(c3)] + first[1]).tolist()


def test_middle_rank_fully_labelled(backend):
    """(b) the middle of three ranks holds no live cloud: it emits nothing, the live ranks of the others run on across it"""
    ranks = _ranks(2, [[10, 12], [8, 9], [11]])
    ranks[1].labeled[:] = True
    out, exp = _case(ranks, 50, 20)
    assert exp["live"] == [0, 1, 4] and out[1]["n"] == 0 and out[0]["n"] > 0 and out[2]["n"] > 0


def test_257_clouds_second_trip_of_the_scans(backend):
    """(c) 130 + 127 clouds of 2 and 3 regions: 260 cloud slots, the live scan's second trip begins inside rank 1, whose table ends in padding slots; more than
    256 live clouds take the take scan around as well"""
    rng = np.random.default_rng(3)
    sizes = rng.integers(2, 4, 257).tolist()
    ranks = _ranks(3, [sizes[:130], sizes[130:]], lab_p=0.05)
    T = sum(sizes)
    out, exp = _case(ranks, T, 400)
    assert len(exp["live"]) > 256 and ranks[1].B == 127 < 130 and exp["remain"] > 0
    assert out[1]["n"] > 0 and (out[0]["tables"][1][127:130] == 0).all()


def test_click_equals_total_num(backend):
    """(d) every element is drawn: small clouds are taken whole and the shortfall is the global remainder"""
    ranks = _ranks(4, [[3, 2], [1, 2, 3]], lab_p=0.0)
    out, exp = _case(ranks, 11, 11)
    assert exp["each"].tolist() == [3, 2, 2, 2, 2] and exp["remain"] == 1 and len(exp["items"]) == 10


def test_four_key_bits(backend):
    """(e) 320 elements on 16 keys: both sorts are decided by the (global) id"""
    ranks = _ranks(6, [[150], [170]], lab_p=0.1)
    out, exp = _case(ranks, 320, 100, key_bits=4)
    picks1 = exp["picks"][1][1]
    assert picks1 != sorted(picks1)


def test_label_all(backend):
    """(f) SSDR_REGION_ALL: every unlabelled region of every rank in ascending order, no count read"""
    ranks = _ranks(7, [[30, 1], [44], [5, 6]])
    ranks[0].labeled[30] = True                                   # a dead cloud
    out, exp = _case(ranks, 1, 0, mode=ALL)
    assert len(exp["live"]) == 4 and sum(o["n"] for o in out) == exp["k"]


def test_more_clicks_than_elements(backend):
    """(g) k > total_num: status bit 1 and empty lists on every rank"""
    ranks = _ranks(8, [[5, 6], [7]])
    out = _run(ranks, 18, 19)
    for o in out:
        assert o["info"][5] == ST_COUNT and o["info"][1] == 0 and o["info"][2] == 0 and o["n"] == 0 and o["info"][6] == 0


def test_cloud_outside_the_table_is_seen_by_every_rank(backend):
    """(h) one region of rank 1 names a cloud beyond its table: it takes no part, and bit 4 appears in every rank's d_info"""
    ranks = _ranks(9, [[9, 8], [7, 6], [5]], lab_p=0.0)
    clouds = [r.cloud.copy() for r in ranks]
    clouds[1][12] = 2                                             # rank 1 has clouds 0 and 1
    lab, base, first = _union(ranks)
    lab[first[1] + 12] = True                                     # (takes no part: as if labelled)
    exp, _ = _expected(ranks, 35, 12, RANDOM, lab=lab)
    out = _run(ranks, 35, 12, clouds=clouds)
    assert all(o["info"][5] == ST_CLOUD for o in out)
    assert out[0]["tables"][1][-1] == ST_CLOUD and out[0]["tables"][0][-1] == 0 and out[0]["tables"][2][-1] == 0
    _compare(out, exp, lab, ranks)


@pytest.mark.parametrize("mode", [RANDOM, ALL])
def test_world_one_equals_the_one_call_draw(backend, mode):
    """(i) the two halves at world 1 against ssdr_region_draw_dev, output for output"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    L = _lib.lib()
    ranks = _ranks(10, [[40, 1, 300, 7, 2500]], lab_p=0.2)
    r = ranks[0]
    out = _run(ranks, r.S, 600, mode)[0]
    lab, cloud, cnt = DevArray.from_host(r.labeled.astype(np.uint8)), DevArray.from_host(r.cloud), DevArray.from_host(np.array([600], np.int64))
    items, n, info = DevArray.from_host(np.full(r.S, -7, np.int32)), DevArray((1,), np.int32), DevArray((8,), np.int64)
    assert L.ssdr_region_draw_dev(5, 2, 1, mode, 32, 0, lab.ptr, cloud.ptr, r.S, r.B, r.S, cnt.ptr, items.ptr, r.S, n.ptr, info.ptr, None) == 0
    _lib.sync()
    w = info.to_host()
    each = np.zeros(int(w[0]), np.int32)
    assert L.ssdr_region_draw_shares(None, _lib.ptr(each), len(each)) == 0
    k = int(n.to_host()[0])
    assert k == out["n"] > 0 and np.array_equal(items.to_host()[:k], out["items"]) and np.array_equal(out["pos"], np.arange(k))
    assert np.array_equal(w[:6], out["info"][:6]) and w[6] == 0 and out["info"][6] == k and np.array_equal(each, out["each"])
    if mode == RANDOM:
        assert w[3] > 0                                            # (clouds smaller than their share)


def test_item_list_too_short_is_this_ranks_own_bit(backend):
    ranks = _ranks(11, [[20], [30]], lab_p=0.0)
    exp, _ = _expected(ranks, 50, 30, RANDOM)
    n1 = len(exp["picks"][1][1])
    assert n1 > 4 and len(exp["picks"][0][1]) <= 20
    out = _run(ranks, 50, 30, max_items=n1 - 1)
    assert out[0]["info"][5] == 0 or len(exp["picks"][0][1]) > n1 - 1
    assert out[1]["info"][5] == ST_ITEMS and out[1]["n"] == n1 - 1 and out[1]["info"][6] == n1
    assert out[1]["items"].tolist() == exp["picks"][1][1][: n1 - 1]


def test_refusals(backend):
    """(j) refused before anything is launched"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    L = _lib.lib()
    S, B = 6, 2
    lab, cloud = DevArray.from_host(np.zeros(S, np.uint8)), DevArray.from_host(np.array([0, 0, 0, 1, 1, 1], np.int32))
    u, u_all = DevArray.from_host(np.full(4, -9, np.int32)), DevArray.from_host(np.array([[3, 3, 0, 0], [3, 3, 0, 0]], np.int32))
    cnt, items, pos, n, info = (DevArray.from_host(np.array([3], np.int64)), DevArray.from_host(np.full(S, -7, np.int32)), DevArray.from_host(np.full(S, -7, np.int32)),
                                DevArray.from_host(np.array([-7], np.int32)), DevArray((8,), np.int64))

    def count(lab_p=lab.ptr, cloud_p=cloud.ptr, S_=S, B_=B, u_p=u.ptr, slots=3):
        return L.ssdr_region_draw_count_dev(lab_p, cloud_p, S_, B_, u_p, slots, None)
    for bad in (dict(lab_p=None), dict(cloud_p=None), dict(u_p=None), dict(S_=0), dict(B_=0), dict(slots=1)):
        assert count(**bad) == 1, bad
    assert count(S_=0x40000000) == UNSUPPORTED and count(slots=0x40000000) == UNSUPPORTED
    _lib.sync()
    assert u.to_host().tolist() == [-9] * 4

    def draw(mode=0, key_bits=32, first=0, rank=0, world=2, u_p=u_all.ptr, slots=3, lab_p=lab.ptr, cloud_p=cloud.ptr, S_=S, B_=B, T=12, cnt_p=cnt.ptr, items_p=items.ptr,
             pos_p=pos.ptr, n_p=n.ptr, info_p=info.ptr):
        return L.ssdr_region_draw_sharded_dev(1, 0, 0, mode, key_bits, first, rank, world, u_p, slots, lab_p, cloud_p, S_, B_, T, cnt_p, items_p, pos_p, S, n_p, info_p, None)
    for bad in (dict(lab_p=None), dict(cloud_p=None), dict(cnt_p=None), dict(items_p=None), dict(pos_p=None), dict(n_p=None), dict(info_p=None), dict(u_p=None),
                dict(S_=0), dict(T=0), dict(B_=0), dict(key_bits=0), dict(key_bits=33), dict(mode=2), dict(world=0), dict(rank=2), dict(rank=-1), dict(slots=1)):
        assert draw(**bad) == 1, bad
    for big in (dict(first=0x3fffffff), dict(first=0x3fffffff - 5), dict(world=2, slots=0x20000000), dict(T=0x40000000), dict(slots=0x40000000)):
        assert draw(**big) == UNSUPPORTED, big
    _lib.sync()
    assert items.to_host().tolist() == [-7] * S and pos.to_host().tolist() == [-7] * S and n.to_host()[0] == -7      # nothing was launched
    assert draw(first=0x3fffffff - 6, rank=1) == 0                 # the largest global id the draw takes
    assert draw(mode=1, cnt_p=None, rank=1, first=6) == 0          # label-all reads no count
    _lib.sync()
    assert n.to_host()[0] == S and items.to_host().tolist() == list(range(S)) and pos.to_host().tolist() == list(range(6, 12))


def test_sanitized_stand_alone_program():
    """make region-draw-sharded-san: two emulated ranks of cases (a) and (d) under ASan + UBSan on the CPU build, a program with its own main (nothing preloaded)"""
    import os
    import subprocess
    from conftest import PKG, ROOT
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(PKG, "csrc"), "region-draw-sharded-san"])
    env = dict(os.environ, OMP_NUM_THREADS="2", ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "san", "region_draw_sharded_san")], env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and "region draw sharded ok" in r.stdout, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
