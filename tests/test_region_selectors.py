"""The "edcd" and uncertainty-only branches of TSampler.sampling() (S3/sampler2.py:670-685, :783-806) as HotPath selectors.

edcd: per cloud, farthest_superpoint_sample (:49-80) over the cloud's candidates with |centre_i - centre_c|^2 + CD(i, c), every cloud in ONE launch
(ssdr_edcd_fps_batch_dev) behind the device candidate rule (ssdr_edcd_sampling_dev and its sharded twin); topk: the first batch_size regions of the
ranking (ssdr_topk_regions_dev).  The oracle is composed of existing pieces: oracle.pipeline_np.selection_round(graph_clouds=set()) for the
population, ranking, candidate list and budget, oracle.select_np.farthest_superpoint_sample for each cloud's sequence (float64 chamfer)."""
import json
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

from _fabricate import make_clouds
from conftest import ROOT

S3 = ("sb", "WetSU", "clsbal", "edcd")


def _cfg(nc=13):
    from ssdr_al.helper_tool import ConfigS3DIS

    class Cfg(ConfigS3DIS):
        num_classes = nc
    return Cfg


def _oracle(clouds, labelled, sel_list, args, batch, min_size=1, max_size=None, nc=13, seq_clouds=None):
    """selection_round's population / ranking / candidates + every cloud's farthest_superpoint_sample: (round, selected_num per cloud,
    [(cloud, expected picks as indices into the candidate list)])"""
    from oracle import pipeline_np as P
    from oracle import select_np as S
    r = P.selection_round(clouds, labelled, sel_list, nc, list(args), min_size, 2, batch, 1, 0, 0, np.random.RandomState(0), max_size=max_size,
                          graph_clouds=set())
    bs = min(batch, len(r["region"]))
    ntop = Counter(r["region"][i][0] for i in r["sorted_inds"][:bs])
    unl = r["unl"]
    exp, first = [], 0
    for b in sorted(ntop):
        cands = [s for c, s in unl if c == b]
        assert unl[first: first + len(cands)] == [(b, s) for s in cands]
        if seq_clouds is None or b in seq_clouds:
            cl = clouds[b]
            seq = S.farthest_superpoint_sample(np.asarray(cl["xyz"], np.float32), np.asarray(cl["offsets"]), np.asarray(cl["points"]), cands, ntop[b], 0)
            exp.append((b, [first + int(q) for q in seq]))
        first += len(cands)
    return r, ntop, exp


def _check_edcd(hp, sel, unl, r, ntop, exp):
    base = np.asarray(hp.sp_base)
    assert [(b, s - int(base[b])) for b, s in unl] == r["unl"]
    assert len(sel) == r["sampling_batch"] == sum(ntop.values())
    cloud_of = np.array([c for c, _ in r["unl"]], np.int64)
    si = np.asarray(sel, np.int64)
    assert Counter(cloud_of[si].tolist()) == ntop                     # selected_num per cloud
    for b, seq in exp:
        assert si[cloud_of[si] == b].tolist() == seq, "cloud %d" % b
    assert hp.selected == [r["unl"][i] for i in si]


def _relabel(cl, region_probs, nc=13):
    """every point of region s gets the class vector region_probs[s]: the region's uncertainty is fixed by it"""
    probs = np.empty((len(cl["xyz"]), nc), np.float32)
    off, pts = cl["offsets"], cl["points"]
    for s in range(len(off) - 1):
        probs[pts[off[s]:off[s + 1]]] = region_probs[s]
    return dict(cl, probs=probs)


def _peaked(m, nc=13):
    v = np.full(nc, (1.0 - m) / (nc - 1), np.float32); v[1] = m
    return v


def _last(cl, nc=13):
    """regions that rank last: a confident majority (class 1) and an uncertain minority (class 2) — WetSU counts the minority against the region"""
    probs = np.empty((len(cl["xyz"]), nc), np.float32)
    off, pts = cl["offsets"], cl["points"]
    for s in range(len(off) - 1):
        ids = pts[off[s]:off[s + 1]]
        k = len(ids) // 2 + 1
        probs[ids[:k]] = _peaked(0.98 + 1e-5 * s, nc)
        minority = _peaked(0.08, nc); minority[[1, 2]] = minority[[2, 1]]
        probs[ids[k:]] = minority
    return dict(cl, probs=probs)


# ---- 1. the batched kernel ---------------------------------------------------------------------------------------------------------------------------
def _np_fps(cen, cd, k):
    """sampler2.py:66-79 over given centres / chamfer matrix (cd = dir + dir^T)"""
    out = [0]
    d = np.ones(len(cen)) * 1e10
    for _ in range(k - 1):
        dist = np.sum((cen - cen[out[-1]]) ** 2, axis=-1) + cd[out[-1]]
        m = dist < d
        d[m] = dist[m]
        out.append(int(np.argmax(d)))
    return out


def _batch_kernel(cens, dirs, ntop, n_max=None, max_select=None):
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    n_c = np.array([len(c) for c in cens], np.int64)
    coff = np.concatenate([[0], np.cumsum(n_c)]).astype(np.int32)
    boff = np.concatenate([[0], np.cumsum(n_c * n_c)]).astype(np.int64)
    d_cen = DevArray.from_host(np.concatenate(cens).astype(np.float64))
    d_dir = DevArray.from_host(np.concatenate([d.reshape(-1) for d in dirs]).astype(np.float64))
    d_coff, d_boff, d_ntop = DevArray.from_host(coff), DevArray.from_host(boff), DevArray.from_host(np.asarray(ntop, np.int32))
    tot = int(np.sum(ntop))
    d_out = DevArray((max(tot, 1),), np.int32); d_st = DevArray((1,), np.int32)
    rc = _lib.lib().ssdr_edcd_fps_batch_dev(d_cen.ptr, d_dir.ptr, d_coff.ptr, d_boff.ptr, d_ntop.ptr, len(cens), int(n_c.max()) if n_max is None else n_max,
                                            tot if max_select is None else max_select, d_out.ptr, d_st.ptr, None)
    if rc:
        return rc, None, None, None
    _lib.sync()
    return 0, d_out.to_host()[:tot], int(d_st.to_host()[0]), d_dir.to_host()


def test_edcd_batch_kernel_matches_single_cloud_entry_and_numpy(backend):
    """clouds of 1, 2, 74 and ~1 500 rows, a cloud without picks and a cloud of coincident centres (ties) in ONE launch == per-cloud
    ssdr_fps_superpoint_dev == the NumPy loop, index for index; the blocks come back symmetrised; the status word refuses what does not fit"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    rng = np.random.default_rng(5)
    sizes = [1, 2, 74, 3, 1500 if backend == "gpu" else 600, 9]
    ntop = [1, 1, 37, 0, 700 if backend == "gpu" else 240, 5]
    cens = [rng.random((n, 3)) * np.array([6.0, 5.0, 2.5]) for n in sizes]
    dirs = [rng.random((n, n)) * 0.3 for n in sizes]
    cens[-1][:] = 1.5; dirs[-1][:] = 0.25                                      # ties everywhere: the lowest index wins (np.argmax)
    for d in dirs:
        np.fill_diagonal(d, 0.0)
    rc, got, st, dsym = _batch_kernel(cens, dirs, ntop)
    assert rc == 0 and st == 0 and len(got) == sum(ntop)
    coff = np.concatenate([[0], np.cumsum(sizes)])
    L = _lib.lib()
    o = 0
    for b, (cen, d, k) in enumerate(zip(cens, dirs, ntop)):
        mine = got[o:o + k] - coff[b]
        o += k
        if k == 0:
            continue
        exp = _np_fps(cen, d + d.T, k)
        assert mine.tolist() == exp, "cloud %d" % b
        d_c, d_d, d_o = DevArray.from_host(cen), DevArray.from_host(np.ascontiguousarray(d)), DevArray((k,), np.int32)
        _lib.check(L.ssdr_fps_superpoint_dev(d_c.ptr, d_d.ptr, len(cen), 0, k, d_o.ptr, None))
        _lib.sync()
        assert d_o.to_host().tolist() == exp
    assert got[-5:].tolist() == [int(coff[-2]) + i for i in range(5)]
    # the blocks are symmetrised in place, exactly
    bo = 0
    for d in dirs:
        n = len(d)
        assert np.array_equal(dsym[bo:bo + n * n].reshape(n, n), d + d.T)
        bo += n * n
    # the status word: more picks than rows (8), more picks than the output holds (16), a cloud above n_max (4); n_max above 8192 is refused
    assert _batch_kernel(cens[:3], dirs[:3], [1, 3, 4])[:3:2] == (0, 8)
    assert _batch_kernel(cens[:3], dirs[:3], [1, 2, 4], max_select=5)[:3:2] == (0, 16)
    assert _batch_kernel(cens[:3], dirs[:3], [1, 2, 4], n_max=8)[:3:2] == (0, 4)
    assert _batch_kernel(cens[:3], dirs[:3], [1, 2, 4], n_max=8193)[0] != 0


def test_edcd_batch_kernel_on_real_clouds_equals_oracle(backend):
    """clouds of 1, 2 and 74 superpoints through ssdr_cloud_graph_batch_dev + the batched kernel == select_np.farthest_superpoint_sample"""
    from oracle import select_np as S
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    clouds, _, _ = make_clouds(21, 3, 74, 4, 30)
    sizes, ntop = [1, 2, 74], [1, 2, 37]
    xyz = np.concatenate([c["xyz"] for c in clouds]).astype(np.float32)
    p0 = np.concatenate([[0], np.cumsum([len(c["xyz"]) for c in clouds])])
    offs, pts = [np.zeros(1, np.int64)], []
    for b, c in enumerate(clouds):
        offs.append(np.asarray(c["offsets"][1:], np.int64) + offs[-1][-1]); pts.append(np.asarray(c["points"], np.int64) + p0[b])
    off, pts = np.concatenate(offs).astype(np.int32), np.concatenate(pts).astype(np.int32)
    base = np.concatenate([[0], np.cumsum([len(c["offsets"]) - 1 for c in clouds])])
    sel = np.concatenate([base[b] + np.arange(n) for b, n in enumerate(sizes)]).astype(np.int32)
    n_c = np.array(sizes, np.int64)
    coff = np.concatenate([[0], np.cumsum(n_c)]).astype(np.int32); boff = np.concatenate([[0], np.cumsum(n_c * n_c)]).astype(np.int64)
    L = _lib.lib()
    _lib.check(L.ssdr_select_set_chamfer_mode(0))
    d_x, d_o, d_p, d_s = DevArray.from_host(xyz), DevArray.from_host(off), DevArray.from_host(pts), DevArray.from_host(sel)
    d_coff, d_boff, d_n = DevArray.from_host(coff), DevArray.from_host(boff), DevArray.from_host(np.asarray(ntop, np.int32))
    d_cen = DevArray((len(sel), 3), np.float64); d_dir = DevArray((int(boff[-1]),), np.float64); d_adj = DevArray((int(boff[-1]),), np.float64)
    _lib.check(L.ssdr_cloud_graph_batch_dev(d_x.ptr, d_o.ptr, d_p.ptr, d_s.ptr, d_coff.ptr, d_boff.ptr, 3, len(sel), 74, 0, d_cen.ptr, d_dir.ptr, d_adj.ptr, None))
    d_out = DevArray((sum(ntop),), np.int32)
    _lib.check(L.ssdr_edcd_fps_batch_dev(d_cen.ptr, d_dir.ptr, d_coff.ptr, d_boff.ptr, d_n.ptr, 3, 74, sum(ntop), d_out.ptr, None, None))
    _lib.sync()
    got = d_out.to_host()
    o = 0
    for b, (n, k) in enumerate(zip(sizes, ntop)):
        c = clouds[b]
        exp = S.farthest_superpoint_sample(c["xyz"], np.asarray(c["offsets"]), np.asarray(c["points"]), list(range(n)), k, 0)
        assert (got[o:o + k] - coff[b]).tolist() == np.asarray(exp).tolist()
        o += k


# ---- 2. the edcd round, S3DIS flavour --------------------------------------------------------------------------------------------------------------------
def _s3dis_clouds():
    """seven clouds: ordinary ones, one whose regions all rank last (no top region at a small batch), one of four very uncertain regions (its
    ranked list is shorter than 2 x its selected_num)"""
    clouds, labelled, sel_list = make_clouds(41, 7, (24, 40), 3, 25, labelled_per_cloud=5)
    clouds[2] = _last(clouds[2])
    small, _, _ = make_clouds(42, 1, 4, 10, 20, labelled_per_cloud=0)
    clouds[4], labelled[4] = _relabel(small[0], [_peaked(0.078 + 0.0005 * s) for s in range(4)]), set()
    return clouds, labelled, sel_list


@pytest.mark.parametrize("batch", [30, 10 ** 6, 0])
def test_edcd_round_equals_composed_oracle(backend, batch, monkeypatch):
    """HotPath(selector="edcd") over fabricated clouds (clsbal, min_size): candidate list, selected_num per cloud and every cloud's pick sequence ==
    the composed oracle; batch_size above the population is clamped, zero picks give nothing; labelled regions are never candidates; the device rule
    == the host rule"""
    from ssdr_al import pipeline
    clouds, labelled, sel_list = _s3dis_clouds()
    hp = pipeline.HotPath.from_clouds(clouds, labelled, sel_list, _cfg(), sampler_args=S3, selector="edcd", min_size=5, batch_size=batch, round_num=2)
    sel, unl = hp.step_selection()
    assert hp.rule_path == "device"
    r, ntop, exp = _oracle(clouds, labelled, sel_list, S3, batch, min_size=5)
    _check_edcd(hp, sel, unl, r, ntop, exp)
    base = np.asarray(hp.sp_base)
    assert not any(s - int(base[b]) in labelled[b] for b, s in unl)
    if batch == 30:
        assert 2 not in ntop and ntop[4] == 4 and sum(1 for b, _ in unl if b == 4) == 4          # no top region; fewer than 2 x selected_num ranked
    if batch == 10 ** 6:
        assert len(sel) == len(r["region"]) and len(sel) > 100
    if batch == 0:
        assert len(sel) == 0 and len(unl) == 0 and hp.selected == []
    monkeypatch.setenv("SSDR_SELECT_HOST_RULE", "1")
    sel_h, unl_h = hp.step_selection()
    assert hp.rule_path == "host" and unl_h == unl and np.array_equal(sel_h, sel)


# ---- 3. Semantic3D flavour: max_size; the float32 chamfer for gcn_fps, float64 for edcd --------------------------------------------------------------
def _tie_cloud(nc=13):
    """three two-point regions A, C, B (in rank order).  B and C sit at the same distance from A's centre; CD(A, C) is 1.4e-8 below CD(A, B): float64
    picks B after A, float32 chamfer values tie (0.25 - 1e-8 rounds to 0.25) and would pick C"""
    xyz = np.array([[0, 0.25, 0], [0, -0.25, 0],               # A
                    [-1.75, 1e-8, 0], [-2.25, -1e-8, 0],       # C: centre (-2, 0, 0), a segment turned by 4e-8 rad
                    [2.25, 0, 0], [1.75, 0, 0]], np.float32)   # B: centre (2, 0, 0)
    cl = dict(xyz=xyz, gt=np.ones(6, np.int32), feat=np.zeros((6, 32), np.float32), offsets=np.array([0, 2, 4, 6], np.int32), points=np.arange(6, dtype=np.int32))
    return _relabel(cl, [_peaked(m, nc) for m in (0.078, 0.079, 0.080)], nc)      # lc uncertainty 0.922 > 0.921 > 0.920: the most uncertain regions


def test_edcd_semantic3d_flavour_uses_float64_chamfer(backend):
    """max_size=1000 and chamfer_mode="f32_cuda" (the Semantic3D code): the edcd picks are the FLOAT64 oracle's — including a cloud where float32
    chamfer values would pick differently"""
    from oracle import select_np as S
    from ssdr_al import pipeline
    args = ("lc", "mean", "edcd")
    tie = _tie_cloud()
    # the construction: float32 chamfer values (create_cd_cuda) pick C, float64 (create_cd) picks B
    off6, pts6 = tie["offsets"], np.arange(6)
    cen = S.bbox_centres(tie["xyz"], off6, pts6)
    assert _np_fps(cen, S.create_cd_cuda(tie["xyz"], off6, pts6, cen), 2) == [0, 1]
    assert _np_fps(cen, S.create_cd(tie["xyz"], off6, pts6, cen), 2) == [0, 2]
    rest, labelled, sel_list = make_clouds(43, 3, (10, 16), 3, 20, labelled_per_cloud=3)
    big, _, _ = make_clouds(44, 1, 5, 950, 1060, labelled_per_cloud=0)          # regions of more than 1000 points drop out
    sz = np.diff(big[0]["offsets"])
    assert (sz > 1000).any() and (sz <= 1000).any()
    clouds = [tie] + rest + big
    labelled = [set()] + labelled + [set()]
    kw = dict(sampler_args=args, selector="edcd", max_size=1000, chamfer_mode="f32_cuda")
    hp = pipeline.HotPath.from_clouds(clouds, labelled, sel_list, _cfg(), batch_size=2, **kw)
    sel, unl = hp.step_selection()
    r, ntop, exp = _oracle(clouds, labelled, sel_list, args, 2, max_size=1000)
    assert dict(ntop) == {0: 2} and exp == [(0, [0, 2])]
    _check_edcd(hp, sel, unl, r, ntop, exp)
    assert hp.selected == [(0, 0), (0, 2)]
    # a wider round of the same flavour
    hp = pipeline.HotPath.from_clouds(clouds, labelled, sel_list, _cfg(), batch_size=25, **kw)
    sel, unl = hp.step_selection()
    r, ntop, exp = _oracle(clouds, labelled, sel_list, args, 25, max_size=1000)
    _check_edcd(hp, sel, unl, r, ntop, exp)
    over = set(np.flatnonzero(sz > 1000).tolist())
    assert not any(s - int(hp.sp_base[b]) in over for b, s in unl if b == len(clouds) - 1)


# ---- 4. topk -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [37, 10 ** 6])
def test_topk_round_is_the_ranking_head(backend, batch, monkeypatch):
    """selector="topk": hp.selected == the oracle ranking's first batch_size regions as (room id, superpoint); unl = those regions in rank order, sel = arange"""
    from oracle import pipeline_np as P
    from ssdr_al import pipeline
    args = ("sb", "WetSU", "clsbal")
    clouds, labelled, sel_list = _s3dis_clouds()
    hp = pipeline.HotPath.from_clouds(clouds, labelled, sel_list, _cfg(), sampler_args=args, selector="topk", min_size=5, batch_size=batch)
    sel, unl = hp.step_selection()
    assert hp.rule_path == "device"
    r = P.selection_round(clouds, labelled, sel_list, 13, list(args), 5, 2, batch, 1, 0, 0, np.random.RandomState(0), graph_clouds=set())
    exp = [r["region"][i] for i in r["sorted_inds"][:batch]]
    assert hp.selected == exp and len(exp) == min(batch, len(r["region"]))
    assert np.array_equal(sel, np.arange(len(exp)))
    base = np.asarray(hp.sp_base)
    assert [(b, s - int(base[b])) for b, s in unl] == exp
    monkeypatch.setenv("SSDR_SELECT_HOST_RULE", "1")
    sel_h, unl_h = hp.step_selection()
    assert hp.rule_path == "host" and unl_h == unl and np.array_equal(sel_h, sel) and hp.selected == exp


# ---- 4b. the host route of fps / k-center: what the device routes hand over -----------------------------------------------------------------------------
@pytest.mark.parametrize("selector", ["fps", "kcenter"])
def test_round_without_picks_selects_nothing(backend, selector):
    """batch_size 0: the device rule hands the round to the host route, which returns an empty selection and an empty candidate list"""
    from ssdr_al import pipeline
    clouds, labelled, sel_list = _s3dis_clouds()
    hp = pipeline.HotPath.from_clouds(clouds, labelled, sel_list, _cfg(), selector=selector, batch_size=0)
    sel, unl = hp.step_selection()
    assert hp.rule_path == "host"
    assert len(sel) == 0 and unl == [] and hp.selected == []


def test_kcenter_without_a_labelled_region_is_refused(backend):
    """k-center seeds its chain with the labelled rows: with none in any cloud the host route's kCenterGreedy call refuses the round"""
    from ssdr_al import _lib, pipeline
    clouds, labelled, sel_list = _s3dis_clouds()
    hp = pipeline.HotPath.from_clouds(clouds, [set() for _ in clouds], sel_list, _cfg(), selector="kcenter", batch_size=30)
    with pytest.raises(_lib.SsdrError, match="already_selected"):
        hp.step_selection()


def test_selector_for_follows_the_reference_branch_order():
    from ssdr_al import pipeline
    assert pipeline.selector_for(["sb", "WetSU", "clsbal", "edcd"]) == "edcd"
    assert pipeline.selector_for(["sb", "WetSU", "clsbal", "gcn_fps"]) == "fps"
    assert pipeline.selector_for(["lc", "mean"]) == "topk"
    assert pipeline.selector_for(["edcd", "gcn"]) == "edcd"               # the reference tests "edcd" first
    with pytest.raises(ValueError, match="kcenter"):
        pipeline.selector_for(["sb", "WetSU", "gcn"])
    with pytest.raises(AssertionError):
        pipeline.HotPath(None, selector="gcn")


# ---- 5. sharded (CPU logic build, gloo) -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards,notop,port", [("3,3", -1, 29561), ("3,2,1", 2, 29563)])
def test_sharded_region_selectors_equal_single_process(tmp_path, emu_lib, shards, notop, port):
    """world 2 and world 3 (3 + 2 + 1 clouds, one rank without a top region): every rank's edcd picks / top regions == the single-process run over
    the union of the rooms restricted to that rank's rooms, index for index; together they are the single-process result; device rule == host rule"""
    world = len(shards.split(","))
    env = dict(os.environ, SSDR_TEST_OUT=str(tmp_path), OMP_NUM_THREADS="2", SSDR_TEST_SHARDS=shards, SSDR_TEST_NOTOP_RANK=str(notop), SSDR_TEST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "_selector_dist_worker.py")]
    subprocess.run(cmd, check=True, env=env, timeout=1800, cwd=ROOT)
    r = [json.load(open(tmp_path / ("rank%d.json" % i))) for i in range(world)]
    for sel in ("edcd", "topk"):
        single = [tuple(x) for x in r[0][sel + "_single"]]
        assert len(single) == 40
        for x in r:
            mine = set(x["rooms"])
            assert [tuple(y) for y in x[sel]] == [y for y in single if y[0] in mine]
            assert x[sel + "_path"] == "sharded-device" and x[sel + "_host_equal"]
        assert sorted(tuple(y) for x in r for y in x[sel]) == sorted(single)
        if sel == "edcd":
            assert [tuple(y) for x in r for y in x[sel]] == single          # contiguous shards: rank order is cloud order
    if notop >= 0:
        assert r[notop]["edcd"] == [] and r[notop]["topk"] == []


# ---- 6. GPU ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_edcd_round_at_reference_scale(backend):
    """272 clouds, batch_size 10 000 through the device chain: the candidate list == the fps chain's; the picks sum to sampling_batch and a sample of
    clouds' sequences == the composed oracle"""
    if backend != "gpu":
        pytest.skip("the reference's scale runs on the GPU only")
    from ssdr_al import pipeline
    clouds, labelled, sel_list = make_clouds(3, 272, 150, 20, 60, labelled_per_cloud=15)
    kw = dict(sampler_args=S3, gcn_number=1, gcn_top=0, min_size=1, round_num=5, label_seed=9, batch_size=10000)
    hp = pipeline.HotPath.from_clouds(clouds, labelled, sel_list, _cfg(), selector="edcd", **kw)
    sel, unl = hp.step_selection()
    assert hp.rule_path == "device" and len(sel) == 10000
    fp = pipeline.HotPath.from_clouds(clouds, labelled, sel_list, _cfg(), selector="fps", **kw)
    _, unl_f = fp.step_selection()
    assert unl == unl_f and len(unl) == 20000
    r, ntop, exp = _oracle(clouds, labelled, sel_list, S3, 10000, seq_clouds={0, 100, 271})
    assert [b for b, _ in exp] == [0, 100, 271]
    _check_edcd(hp, sel, unl, r, ntop, exp)


@pytest.mark.gpu
def test_rccl_world_one_equals_plain_path_for_region_selectors(tmp_path):
    """the sharded code path through RCCL (world 1) == the plain path, both new selectors"""
    from conftest import _have_gpu
    if not _have_gpu():
        pytest.skip("no GPU")
    env = dict(os.environ, SSDR_TEST_OUT=str(tmp_path), SSDR_TEST_BACKEND="nccl", MASTER_ADDR="127.0.0.1", MASTER_PORT="29565", RANK="0", LOCAL_RANK="0",
               WORLD_SIZE="1")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_selector_dist_worker.py")], check=True, env=env, timeout=600, cwd=ROOT)
    r = json.load(open(tmp_path / "rank0.json"))
    for sel in ("edcd", "topk"):
        assert len(r[sel]) == 40 and r[sel] == r[sel + "_single"] and r[sel + "_path"] == "sharded-device" and r[sel + "_host_equal"]


@pytest.mark.gpu
@pytest.mark.parametrize("selector", ["edcd", "topk"])
def test_hot_path_step_with_region_selector(backend, selector):
    """one HotPath.step() per batch (front end -> network -> scoring -> the new selector) == the selection half over host copies of its arrays"""
    if backend != "gpu":
        pytest.skip("the per-batch hot path at its size runs on the GPU")
    from oracle import randla_np as R
    from ssdr_al import pipeline, synthetic
    from ssdr_al.helper_tool import ConfigS3DIS

    class Cfg(ConfigS3DIS):
        num_points = 8192
    W = R.init_weights(0)
    rooms = [synthetic.make_room(7300 + i, density=600.0) for i in range(3)]
    hp = pipeline.HotPath(W, Cfg, select_per_tile=9, labeled_per_tile=4, selector=selector).load_rooms(rooms)
    sel, unl = hp.step()
    assert len(sel) == 27
    N = Cfg.num_points
    xyz, probs, f32, lab = hp.xyz.to_host().reshape(-1, 3), hp.probs.to_host(), hp.f32.to_host(), hp.tile_l.to_host()
    clouds, labelled = [], []
    for t in range(hp.B):
        s0, s1 = hp.sp_base[t], (hp.sp_base[t + 1] if t + 1 < hp.B else hp.S)
        off = hp.sp_off_h[s0:s1 + 1].astype(np.int64)
        clouds.append(dict(xyz=xyz[t * N:(t + 1) * N], gt=lab[t * N:(t + 1) * N], probs=probs[t * N:(t + 1) * N], feat=f32[t * N:(t + 1) * N],
                           offsets=off - off[0], points=hp.sp_pts_h[off[0]:off[-1]].astype(np.int64) - t * N))
        labelled.append(set(int(x) - s0 for x in hp.labeled[t]))
    ref = pipeline.HotPath.from_clouds(clouds, labelled, hp.selected_class_list.to_host(), Cfg, batch_size=27, selector=selector)
    rsel, runl = ref.step_selection()
    assert runl == unl and np.array_equal(rsel, sel) and ref.selected == hp.selected


@pytest.mark.gpu
def test_edcd_refuses_a_cloud_above_8192_candidates(backend):
    """a cloud of 8 300 one- or two-point regions, all of them top: the chain's status refuses it and no picks come back"""
    if backend != "gpu":
        pytest.skip("an 8 300 x 8 300 chamfer block: GPU only")
    from ssdr_al import pipeline
    clouds, labelled, sel_list = make_clouds(45, 1, 8300, 1, 2, labelled_per_cloud=0)
    hp = pipeline.HotPath.from_clouds(clouds, labelled, sel_list, _cfg(), sampler_args=S3, selector="edcd", batch_size=8300)
    with pytest.raises(RuntimeError, match="8192"):
        hp.step_selection()
    assert hp.__dict__.get("_selected") is None


# ---- 7. ALRound -------------------------------------------------------------------------------------------------------------------------------------------
def test_al_round_edcd_equals_per_batch_selection(backend):
    """ALRound(selector="edcd"): the round's one selection == HotPath.from_clouds over host copies of the round's arrays"""
    from oracle import randla_np as R
    from ssdr_al import pipeline, synthetic
    from ssdr_al.helper_tool import ConfigS3DIS
    emu = backend == "emu"

    class Cfg(ConfigS3DIS):
        num_points = 512 if emu else 40960
    W = R.init_weights(0)
    rooms = [synthetic.make_room(8100 + i, density=70.0 if emu else 2500.0) for i in range(2)]
    nb = 2 if emu else 6
    ar = pipeline.ALRound(W, rooms, nb, Cfg, batch_size=24, round_num=2, labeled_per_tile=3, precision="f32", selector="edcd")
    sel, unl = ar.run()
    assert len(sel) == 24 and ar.sel.rule_path == "device"
    N, B = Cfg.num_points, len(rooms)
    xyz, probs, f32, lab = ar.xyz.to_host(), ar.probs.to_host(), ar.f32.to_host(), ar.tile_l.to_host()
    S = ar.sel
    clouds, labelled = [], []
    for t in range(nb * B):
        s0, s1 = S.sp_base[t], (S.sp_base[t + 1] if t + 1 < nb * B else S.S)
        off = S.sp_off_h[s0:s1 + 1].astype(np.int64)
        clouds.append(dict(xyz=xyz[t * N:(t + 1) * N], gt=lab[t * N:(t + 1) * N], probs=probs[t * N:(t + 1) * N], feat=f32[t * N:(t + 1) * N],
                           offsets=off - off[0], points=S.sp_pts_h[off[0]:off[-1]].astype(np.int64) - t * N))
        labelled.append(set(int(x) - s0 for x in S.labeled[t]))
    ref = pipeline.HotPath.from_clouds(clouds, labelled, S.selected_class_list.to_host(), Cfg, batch_size=24, round_num=2, selector="edcd")
    rsel, runl = ref.step_selection()
    assert runl == unl and np.array_equal(rsel, sel) and ref.selected == S.selected
