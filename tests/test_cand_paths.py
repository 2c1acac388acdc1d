"""The candidate rule and the top-k head, branch by branch: the cand_* kernels of csrc/select.hip behind ssdr_edcd_sampling_dev, ssdr_gcn_fps_sampling_dev and the
sharded entry points ssdr_edcd_sampling_sharded_dev / ssdr_gcn_fps_sharded_local_dev, edcd_plan and topk_regions of csrc/select_region.hip.  DESIGN.md
section 25 lists every branch with the case that reaches it.  What the older tests (test_pipeline.py: test_candidate_rule_on_device_equals_host_rule,
test_region_selectors.py) leave open and this file closes:

  * the oracle is the reference's plain loops over the ranking (tests/_cand_paths.py: rule_oracle), not HotPath._candidates;
  * the kernels' constants: chunks of CR_NT ranks (one, one and a region, three, a whole labelled chunk, more than 256 of them), tiles of CC_TILE regions of a
    cloud (one short of a tile, one over, two and three over: the padded quads), the slices of cand_slices with a small cloud beside a large one, more than 256
    clouds, chunks of TK_NT ranks of the top-k walk;
  * the capacities one below what the rule produces: the status, zero counts and not a word written behind the buffers;
  * the sharded entry points in ONE process (every ranking input is an argument): worlds of 2 and 3 ranks against the single-process oracle's slices.

Every case is thousands of one-point regions (the graph behind the rule then costs nothing), runs on the CPU logic build and on the gfx950 build with the
same inputs and asserts its input condition with tests/_cand_paths.py: plan BEFORE the library is called.  Everything here is integers: every comparison is exact.
"""
import functools

import numpy as np
import pytest

from oracle import select_np as O
import _cand_paths as G
from _score_paths import assert_bits

K = G.constants()


# ---- the cases of the rule ------------------------------------------------------------------------------------------------------------------------------
def _case(name):
    """-> order, labelled, base, batch_size"""
    rng = np.random.default_rng(sum(map(ord, name)))
    T, R = K.CC_TILE, K.CR_NT

    def make(sizes, batch, lab_p=0.3):
        S = int(np.sum(sizes))
        return rng.permutation(S).astype(np.int32), (rng.random(S) < lab_p).astype(np.uint8), G.base_of(sizes), batch
    if name in ("one", "one_batch0"):
        order, lab, base, batch = make([1], 1 if name == "one" else 0, 0.0)
    elif name == "below_chunk":          # S = CR_NT - 1: clouds of 0, 1, 255, 256, 257 regions, one cloud labelled throughout
        order, lab, base, batch = make([0, 1, 255, 256, 257, R - 1 - 769 - 100, 100], 100)
        lab[base[6]:base[7]] = 1
    elif name == "chunk":                # S = CR_NT, a whole 64-rank wave of labelled regions, batch >= S: every cloud offers all it has
        order, lab, base, batch = make([255, 256, 257, R - 768], R + 5)
        lab[order[64:128]] = 1
    elif name == "chunk_plus_one":       # S = CR_NT + 1 in one cloud, one pick
        order, lab, base, batch = make([R + 1], 1)
    elif name == "three_chunks":         # S = 3 CR_NT, the middle chunk of the ranking labelled throughout; a cloud one short of a tile
        order, lab, base, batch = make([T - 1, 3 * R - (T - 1)], 300)
        lab[order[R:2 * R]] = 1
    elif name == "tiles":                # clouds of CC_TILE + 1 and 2 CC_TILE + 3 regions beside small ones: two slices, the upper one returns at once for the small clouds
        order, lab, base, batch = make([T + 1, 2 * T + 3, 100, 0, 1, 2 * T + 2], 200, 0.2)
    elif name == "tiles_capped":         # the same clouds, a batch that takes most of them: 2 * ntop exceeds what the clouds have
        order, lab, base, batch = make([T + 1, 40, 0, T + 2], 1500, 0.5)
    elif name == "all_labelled":
        order, lab, base, batch = make([100, 200, 3], 50, 2.0)
    elif name in ("clouds257", "clouds600"):
        B = 257 if name == "clouds257" else 600
        order, lab, base, batch = make(rng.integers(0, 11, B), 500)
    elif name == "many_chunks":          # more than 256 chunks of CR_NT regions over 300 clouds, none of them large
        B, S = 300, 256 * R + R // 2 + 1
        sizes = np.full(B, S // B); sizes[:S % B] += 1
        order, lab, base, batch = make(sizes, 300)
    else:
        raise KeyError(name)
    return order, lab, base, batch


@functools.lru_cache(None)
def _described(name):
    order, lab, base, batch = _case(name)
    for a in (order, lab, base):
        a.setflags(write=False)
    return order, lab, base, batch, G.plan(order, lab, base, batch), G.rule_oracle(order, lab, base, batch)


def _caps(ncand, ntop):
    return dict(cap_rows=max(1, int(ncand.sum())), cap_nmax=max(1, int(ncand.max())), cap_sq=max(1, int((ncand.astype(np.int64) ** 2).sum())), max_select=max(1, int(ntop.sum())))


def _check_rule(r, unl, ntop, ncand, batch_eff, what):
    """counts[0], [3], [4], [5], the candidate list element for element, the picks per cloud; nothing written behind the lists"""
    n_unl = len(unl)
    assert r.counts[5] == 0, "%s: status %d" % (what, r.counts[5])
    assert (r.counts[0], r.counts[3], r.counts[4]) == (n_unl, int(ncand.max()), batch_eff), "%s: counts %s" % (what, r.counts)
    assert np.array_equal(r.cand[:n_unl], unl), "%s: candidate list, first difference at %s" % (what, np.flatnonzero(r.cand[:n_unl] != unl)[:1])
    assert (r.cand[n_unl:] == G.SENTINEL).all() and (r.tail == G.SENTINEL).all(), "%s: written behind the candidate list" % what
    picks = r.picks[:batch_eff]
    assert (r.picks[batch_eff:] == G.SENTINEL).all(), "%s: written behind the picks" % what
    coff = np.concatenate([[0], np.cumsum(ncand)])
    per_cloud = np.bincount(np.searchsorted(coff, picks, side="right") - 1, minlength=len(ncand))[:len(ncand)] if batch_eff else np.zeros(len(ncand), np.int64)
    assert (picks >= 0).all() and (picks < max(n_unl, 1)).all() and len(np.unique(picks)) == batch_eff and np.array_equal(per_cloud, ntop), "%s: picks per cloud" % what
    assert np.array_equal(picks[np.concatenate([[0], np.cumsum(ntop)[:-1]])[ntop > 0].astype(np.int64)], coff[:-1][ntop > 0]), "%s: a cloud's first pick is its first candidate" % what


def _run(name):
    order, lab, base, batch, pl, (unl, ntop, ncand, batch_eff) = _described(name)
    assert np.array_equal(pl.take, ncand) and np.array_equal(pl.nt, ntop), "the restated kernels and the reference's loops disagree on the case itself"
    rng = np.random.default_rng(5)
    xyz, so, sp = G.one_point_regions(rng, len(order))
    r = G.edcd(xyz, so, sp, order, lab, base, batch, **_caps(ncand, ntop))
    _check_rule(r, unl, ntop, ncand, batch_eff, name)
    return pl


def test_rule_single_region(backend):
    for name in ("one", "one_batch0"):
        pl = _described(name)[4]
        assert pl.S == 1 and pl.nchunks == 1 and pl.nt.sum() == (name == "one")
        _run(name)


def test_rule_below_one_chunk(backend):
    pl = _described("below_chunk")[4]
    assert pl.S == K.CR_NT - 1 and pl.nchunks == 1 and {0, 1, 255, 256, 257} <= set(pl.n) and pl.slices == 1
    assert (pl.nv[6] == 0) and pl.n[6] > 0 and (pl.nt > 0).sum() >= 4 and not pl.capped[pl.nt > 0].all()
    _run("below_chunk")


def test_rule_one_chunk_labelled_wave_and_full_batch(backend):
    order, lab, base, batch, pl, _ = _described("chunk")
    assert pl.S == K.CR_NT and pl.nchunks == 1 and 1 in pl.dead_waves and batch >= pl.S and pl.capped.all() and np.array_equal(pl.take, pl.nv)
    _run("chunk")


def test_rule_chunk_and_one_region(backend):
    pl = _described("chunk_plus_one")[4]
    assert pl.S == K.CR_NT + 1 and pl.nchunks == 2 and pl.nt.sum() == 1 and pl.take.sum() == 2
    _run("chunk_plus_one")


def test_rule_three_chunks_labelled_chunk(backend):
    pl = _described("three_chunks")[4]
    assert pl.S == 3 * K.CR_NT and pl.nchunks == 3 and list(pl.dead_chunks) == [1] and pl.n[0] == K.CC_TILE - 1 and pl.padded[0] and pl.tiles[0] == 1 and pl.tiles[1] == 1
    _run("three_chunks")


def test_rule_tiles_and_slices(backend):
    pl = _described("tiles")[4]
    T = K.CC_TILE
    assert list(pl.n[:2]) == [T + 1, 2 * T + 3] and list(pl.tiles[:2]) == [2, 3] and pl.padded[0] and pl.padded[1] and pl.tiles[5] == 3 and pl.padded[5]
    assert pl.slices > 1 and list(np.flatnonzero(pl.early)) == [2, 3, 4] and pl.nt[2] > 0 and pl.n[3] == 0
    _run("tiles")


def test_rule_tiles_batch_beyond_the_clouds(backend):
    pl = _described("tiles_capped")[4]
    assert pl.slices > 1 and pl.capped[[0, 1, 3]].all() and (pl.tiles[[0, 3]] == 2).all() and pl.early[1]
    _run("tiles_capped")


def test_rule_everything_labelled(backend):
    order, lab, base, batch, pl, (unl, ntop, ncand, batch_eff) = _described("all_labelled")
    assert lab.all() and pl.nv.sum() == 0 and len(unl) == 0 and batch_eff == 0
    _run("all_labelled")


@pytest.mark.parametrize("name", ["clouds257", "clouds600"])
def test_rule_many_clouds(backend, name):
    pl = _described(name)[4]
    assert pl.layout_per == (2 if name == "clouds257" else 3) and (pl.n == 0).any() and (pl.nt > 0).sum() > 150
    _run(name)


def test_rule_more_than_256_chunks(backend):
    """cand_chunkscan's threads own two chunks each"""
    pl = _described("many_chunks")[4]
    assert pl.nchunks > K.SCAN_NT and pl.scan_per == 2 and pl.B >= 300 and pl.n.max() < K.CC_TILE and pl.slices == 1 and pl.layout_per == 2
    _run("many_chunks")


@pytest.mark.parametrize("short", ["rows", "sq"])
def test_rule_capacity_one_short(backend, short):
    """cap_rows / cap_sq one below what the rule produces: status 1 / 2, zero counts, no list, no picks, nothing behind the buffers"""
    order, lab, base, batch, pl, (unl, ntop, ncand, batch_eff) = _described("below_chunk")
    caps = _caps(ncand, ntop)
    caps["cap_rows" if short == "rows" else "cap_sq"] -= 1
    assert caps["cap_rows"] == pl.take.sum() - (short == "rows") >= 1 and caps["cap_sq"] == (pl.take ** 2).sum() - (short == "sq") >= 1
    xyz, so, sp = G.one_point_regions(np.random.default_rng(5), len(order))
    r = G.edcd(xyz, so, sp, order, lab, base, batch, **caps)
    assert r.counts[5] == (1 if short == "rows" else 2) and r.counts[0] == 0 and r.counts[2] == 0 and r.counts[4] == batch_eff
    assert (r.raw[G.HEADER:] == G.SENTINEL).all(), "over capacity: something was written behind the counts"


# ---- ssdr_gcn_fps_sampling_dev: the list with labelled rows, the rows, k-center --------------------------------------------------------------------------
@functools.lru_cache(None)
def _gcn_case():
    rng = np.random.default_rng(301)
    sizes = rng.integers(1, 4, 60)                       # points per region
    cl_sizes = [20, 0, 25, 15]                           # regions per cloud
    S = 60
    off = G.base_of(sizes); n = int(off[-1]); pts = rng.permutation(n).astype(np.int32)
    xyz = rng.random((n, 3), dtype=np.float32) * np.float32(4)
    feat = rng.normal(0, 1, (n, 32)).astype(np.float32)
    cls = rng.integers(0, 3, n).astype(np.int32); gt = rng.integers(0, 3, n).astype(np.int32)
    dom = np.array([np.bincount(cls[pts[off[s]:off[s + 1]]]).argmax() for s in range(S)], np.int32)
    gdom = np.array([np.bincount(gt[pts[off[s]:off[s + 1]]]).argmax() for s in range(S)], np.int32)
    base = G.base_of(cl_sizes)
    lab = (rng.random(S) < 0.3).astype(np.uint8)
    order = rng.permutation(S).astype(np.int32)
    lab_sp = np.flatnonzero(lab).astype(np.int32)                                     # cloud ascending, region ascending
    lab_off = np.searchsorted(lab_sp, base).astype(np.int32)
    return dict(off=off, pts=pts, xyz=xyz, feat=feat, cls=cls, gt=gt, dom=dom, gdom=gdom, base=base, lab=lab, order=order, lab_sp=lab_sp, lab_off=lab_off)


@pytest.mark.parametrize("selector", [0, 1], ids=["list_and_rows", "kcenter"])
def test_gcn_fps_list_rows_and_kcenter(backend, selector):
    """labelled rows, gcn_number = 0: the list is the candidates followed by the labelled regions; the rows are the widened segment means, predicted classes
    for the candidates and ground-truth classes for the labelled rows; selector 1 picks by k-center seeded with the labelled rows (`already` points at them)"""
    c = _gcn_case()
    batch = 12
    unl, ntop, ncand, batch_eff = G.rule_oracle(c["order"], c["lab"], c["base"], batch)
    n_lab = len(c["lab_sp"])
    per = ncand + np.diff(c["lab_off"])
    rows = len(unl) + n_lab
    pl = G.plan(c["order"], c["lab"], c["base"], batch)
    assert np.array_equal(pl.take, ncand) and np.array_equal(pl.nt, ntop) and pl.n[1] == 0 and pl.nchunks == 1 and (np.diff(c["lab_off"]) > 0).sum() == 3
    assert n_lab >= 8 and len(unl) >= 12 and (c["cls"] != c["gt"]).any() and (c["dom"][c["lab_sp"]] != c["gdom"][c["lab_sp"]]).any()
    picks = 5 if selector else 0
    r, got_rows = G.gcn_fps(c["feat"], c["cls"], c["dom"], c["gt"], c["gdom"], c["xyz"], c["off"], c["pts"], c["order"], c["lab"], c["base"], c["lab_off"], c["lab_sp"], batch, selector,
                            cap_rows=rows, cap_nmax=int(per.max()), cap_sq=int((per ** 2).sum()), cap_unl=len(unl), max_select=picks)
    assert r.counts[5] == 0 and (r.counts[0], r.counts[1], r.counts[2], r.counts[3], r.counts[4]) == (len(unl), n_lab, rows, int(per.max()), batch_eff)
    want_list = np.concatenate([unl, c["lab_sp"]])
    assert np.array_equal(r.cand, want_list) and (r.tail == G.SENTINEL).all()
    pred = O.segment_mean_features(c["feat"], c["off"], c["pts"], c["cls"], c["dom"])
    truth = O.segment_mean_features(c["feat"], c["off"], c["pts"], c["gt"], c["gdom"])
    want_rows = np.concatenate([pred[unl], truth[c["lab_sp"]]]).astype(np.float64)
    assert_bits(got_rows, want_rows, "the rows of ssdr_gcn_fps_sampling_rows")
    if selector:
        want = O.kcenter_greedy(want_rows, np.arange(len(unl), rows), picks)
        assert np.array_equal(r.picks, want) and (want < len(unl)).all()


# ---- the sharded entry points, in one process ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _shard_case(world):
    rng = np.random.default_rng(400 + world)
    per_rank = [[30, 0, 45, 20], [60, 25], [10, 10, 10]][:world]
    Smax, Bmax = 100, 4
    glab, gbase, gorder = G.shard(rng, per_rank, Smax, Bmax)
    batch = 40
    unl, ntop, ncand, batch_eff = G.rule_oracle(gorder, glab, gbase, batch)          # the single-process rule over the global arrays
    return per_rank, Smax, Bmax, glab, gbase, gorder, batch, unl, ntop, ncand, batch_eff


def _rank_inputs(per_rank, r):
    S_r = int(np.sum(per_rank[r]))
    rng = np.random.default_rng(450 + r)
    xyz, so, sp = G.one_point_regions(rng, S_r)
    return S_r, xyz, so, sp, rng.normal(0, 1, (S_r, 32)).astype(np.float32)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_entry_points_equal_single_process_slices(backend, world):
    """every rank's call of both sharded entry points in one process: its list and counts are the single-process oracle's slice for its clouds"""
    per_rank, Smax, Bmax, glab, gbase, gorder, batch, unl, ntop, ncand, batch_eff = _shard_case(world)
    assert len({len(p) for p in per_rank}) > 1 and any(len(p) < Bmax for p in per_rank) and any(int(np.sum(p)) < Smax for p in per_rank)
    for r, p in enumerate(per_rank):
        assert glab[r * Smax + int(np.sum(p)):(r + 1) * Smax].all(), "padded regions count as labelled"
    pl = G.plan(gorder, glab, gbase, batch)
    assert pl.B == world * Bmax and pl.S == world * Smax and (pl.n == 0).sum() >= 2 and np.array_equal(pl.take, ncand) and np.array_equal(pl.nt, ntop)
    per_rank_cand = ncand.reshape(world, Bmax).sum(1)
    nu_max = int(per_rank_cand.max())
    assert (per_rank_cand > 0).all() and batch_eff == batch
    uoff = np.concatenate([[0], np.cumsum(ncand)])
    for r in range(world):
        S_r, xyz, so, sp, feat = _rank_inputs(per_rank, r)
        B_r = len(per_rank[r])
        mine = unl[uoff[r * Bmax]:uoff[(r + 1) * Bmax]] - r * Smax
        nc_r, nt_r = ncand[r * Bmax:r * Bmax + B_r], ntop[r * Bmax:r * Bmax + B_r]
        assert nc_r.sum() == len(mine) and (mine >= 0).all() and (mine < S_r).all()
        e = G.edcd_sharded(xyz, so, sp, B_r, gorder, glab, gbase, r, world, Smax, Bmax, batch, **_caps(nc_r, nt_r))
        _check_rule(e, mine.astype(np.int32), nt_r, nc_r, int(nt_r.sum()), "edcd, rank %d of %d" % (r, world))
        caps = _caps(nc_r, nt_r); caps.pop("max_select")
        plan, comb = G.gcn_fps_sharded_local(feat, xyz, so, sp, B_r, gorder, glab, gbase, r, world, Smax, Bmax, batch, nu_max=nu_max, **caps)
        words = 16 + world + 2 * world * nu_max
        assert (plan[words:] == G.SENTINEL).all(), "written behind the plan"
        assert plan[5] == 0 and plan[9] == 0 and (plan[0], plan[4], plan[8]) == (len(mine), batch_eff, len(unl)), "rank %d: plan %s" % (r, plan[:16])
        assert np.array_equal(plan[16:16 + world], per_rank_cand)
        glist = plan[16 + world + world * nu_max:][:len(unl)]
        assert np.array_equal(glist, unl), "the global candidate list"
        src = plan[16 + world:][:len(unl)]
        want_src = np.concatenate([q * nu_max + np.arange(per_rank_cand[q]) for q in range(world)])
        assert np.array_equal(src, want_src), "the rows of the gathered array"
        assert_bits(comb[:len(mine)], feat[mine].astype(np.float64), "rank %d: its candidates' rows, in candidate order" % r)
        assert_bits(comb[nu_max:], np.full((1, 32), -7.5), "behind the rows")


def test_sharded_rank_above_nu_max(backend):
    """a rank offers nu_max + 1 candidates: plan[9] is set and neither the row table nor the global list is written"""
    world = 2
    per_rank, Smax, Bmax, glab, gbase, gorder, batch, unl, ntop, ncand, batch_eff = _shard_case(world)
    per_rank_cand = ncand.reshape(world, Bmax).sum(1)
    nu_max = int(per_rank_cand.max()) - 1
    r = int(per_rank_cand.argmin())
    assert per_rank_cand.max() == nu_max + 1 and per_rank_cand[r] <= nu_max and np.array_equal(G.plan(gorder, glab, gbase, batch).take, ncand)
    S_r, xyz, so, sp, feat = _rank_inputs(per_rank, r)
    B_r = len(per_rank[r])
    nc_r, nt_r = ncand[r * Bmax:r * Bmax + B_r], ntop[r * Bmax:r * Bmax + B_r]
    caps = _caps(nc_r, nt_r); caps.pop("max_select")
    plan, comb = G.gcn_fps_sharded_local(feat, xyz, so, sp, B_r, gorder, glab, gbase, r, world, Smax, Bmax, batch, nu_max=nu_max, **caps)
    assert plan[9] != 0 and plan[8] == 0 and np.array_equal(plan[16:16 + world], per_rank_cand)
    assert (plan[16 + world:] == G.SENTINEL).all(), "over nu_max: the tables behind the plan were written"


# ---- ssdr_topk_regions_dev ----------------------------------------------------------------------------------------------------------------------------------
def _topk_want(order, skip, batch, lo, hi):
    top = [int(i) for i in order if not skip[i]][:min(batch, len(order))]
    return np.asarray([i - lo for i in top if lo <= i < hi], np.int32), len(top)


TOPK_N = (0, 1, K.TK_NT - 1, K.TK_NT, K.TK_NT + 1, 3 * K.TK_NT + 5)


@pytest.mark.parametrize("n", TOPK_N)
def test_topk_sizes_batches_windows(backend, n):
    """batch 0, 1, the population, above it; windows empty, whole, a middle third; both result words; nothing behind the entries written"""
    rng = np.random.default_rng(500 + n)
    order = rng.permutation(n).astype(np.int32)
    skip = (rng.random(n) < 0.35).astype(np.uint8)
    pop = int((skip == 0).sum())
    for batch in (0, 1, pop, pop + 7):
        pl = G.plan_topk(order, skip, batch)
        assert pl.chunks == -(-n // K.TK_NT) and pl.top == min(batch, pop)
        for lo, hi in ((n // 2, n // 2), (0, n), (n // 3, 2 * n // 3)):
            want, top = _topk_want(order, skip, batch, lo, hi)
            res, out = G.topk(order, skip, batch, lo, hi, max(1, min(batch, hi - lo)))
            assert (res[0], res[1]) == (len(want), top), "n=%d batch=%d [%d, %d): res %s" % (n, batch, lo, hi, res)
            assert np.array_equal(out[:len(want)], want) and (out[len(want):] == G.SENTINEL).all(), "n=%d batch=%d [%d, %d)" % (n, batch, lo, hi)


def test_topk_skipped_first_chunk_and_top_on_a_boundary(backend):
    """the first chunk of the ranking holds skipped regions only; the top's last entry is the last rank of the second chunk: the walk stops there"""
    rng = np.random.default_rng(77)
    n = 3 * K.TK_NT + 5
    order = rng.permutation(n).astype(np.int32)
    skip = (rng.random(n) < 0.35).astype(np.uint8)
    skip[order[:K.TK_NT]] = 1
    skip[order[2 * K.TK_NT - 1]] = 0
    batch = int((skip[order[:2 * K.TK_NT]] == 0).sum())
    pl = G.plan_topk(order, skip, batch)
    assert pl.dead_first and pl.on_boundary and pl.end_rank == 2 * K.TK_NT - 1 and pl.walked == 2 and pl.chunks == 4 and pl.top == batch < pl.pop
    for b in (batch, batch + 1):          # one more: the third chunk is walked for one entry
        assert G.plan_topk(order, skip, b).walked == (2 if b == batch else 3)
        want, top = _topk_want(order, skip, b, 0, n)
        res, out = G.topk(order, skip, b, 0, n, b)
        assert (res[0], res[1]) == (b, top) and np.array_equal(out[:b], want) and (out[b:] == G.SENTINEL).all()
