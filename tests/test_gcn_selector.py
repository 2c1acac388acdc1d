"""The trained-GCN selector (the reference's "gcn" branch, sampler2.py:687-734 -> gcn.py:193-263): block adjacency, the Adam training loop in both
forms, the evaluation rows, the one-call chain and its Python callers — against the reference's own run (tests/golden/make_golden_gcn_train.py) and
the float64 oracle (tests/_gcn_oracle.py).

The bar of the training tests: e_ref = max |golden float32 weights - float64 oracle| (the reference's own rounding on this graph, computed here);
the device must stay within 4 x e_ref of the float64 oracle.  Measured: the device sits at 0.3 - 1.7 x e_ref on the CPU logic
build."""
import functools
import os
import re

import numpy as np
import pytest

import _gcn_oracle as O
from conftest import ROOT

NAMES = ["cloudC", "cloudD"]


def _refs(g):
    unl = [{"cloud_name": NAMES[c], "sp_idx": int(s)} for c, s in zip(g["g/unl_cloud"], g["g/unl_sp"])]
    lab = [{"cloud_name": NAMES[c], "sp_idx": int(s)} for c, s in zip(g["g/lab_cloud"], g["g/lab_sp"])]
    clouds = {n: (g["g/%s/xyz" % n], g["g/%s/offsets" % n], g["g/%s/points" % n]) for n in NAMES}
    return unl, lab, clouds


def _fixture_graph(golden, cap_rows=None, from_golden_adj=True):
    """the 100 + 30 row graph of gcn_golden.npz: the device's own blocks, or the reference's adjacency cut into blocks (the training tests: same input
    as the golden run)"""
    from ssdr_al import sampler
    g, G = golden("select_golden.npz"), golden("gcn_golden.npz")
    unl, lab, clouds = _refs(g)
    Gr = sampler.GcnGraph.from_clouds(np.concatenate([g["g/unl_feat"], g["g/lab_feat"]]), lab, unl, clouds, cap_rows=cap_rows)
    if not from_golden_adj:
        return Gr
    blocks, g0 = [], 0
    for n in Gr.counts:
        r = Gr.rows_h[g0:g0 + n]; blocks.append(G["adj"][np.ix_(r, r)]); g0 += int(n)
    return sampler.GcnGraph.from_blocks(G["featuresV"], blocks, Gr.rows_h, len(unl), cap_rows=cap_rows)


@functools.lru_cache(maxsize=None)
def _oracle_run(p):
    """float64 oracle on the golden graph from the golden's initial weights: {steps: parameters} — computed once, shared"""
    G = np.load(os.path.join(ROOT, "tests", "golden", "gcn_golden.npz")); T = np.load(os.path.join(ROOT, "tests", "golden", "gcn_train_golden.npz"))
    out, loss0, _ = O.train(G["featuresV"].astype(np.float64), G["adj"].astype(np.float64), int(T["n_unl"]), T["init"], 100, p, int(T["seed"]), record=(1, 10, 100))
    return out, loss0


def test_dropout_function_is_the_documented_one():
    """the NumPy restatement against hand-computed values of the header's formula (Python integers), and the keep rate"""
    seed, step, row, k = 12345, 7, 33, 101
    z = (seed + 0x9E3779B97F4A7C15 * (step + 1) + 0xD6E8FEB86659FD93 * (128 * row + k + 1)) & O.M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & O.M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & O.M64
    z ^= z >> 31
    u = np.float32(z >> 40) * np.float32(2.0 ** -24)
    for p in (0.1, 0.3, 0.9):
        assert bool(O.dropout_keep(seed, step, [row], p)[0, k]) == bool(u >= np.float32(p))
    rate = O.dropout_keep(5, 0, np.arange(4000), 0.3).mean()
    assert abs(rate - 0.7) < 0.01, rate


def test_block_adjacency_matches_the_reference_inside_every_block(backend, golden):
    """the bar of test_select.py::test_create_adj_of_the_gcn_branch (2e-4 relative to max(|entry|, 1)); the transpose is exact; V as there"""
    G = golden("gcn_golden.npz")
    Gr = _fixture_graph(golden, cap_rows=137, from_golden_adj=False)
    assert list(Gr.info()[:3]) == [0, 0x7fffffff, 0]
    assert np.abs(Gr.normalised() - G["featuresV"]).max() < 1e-6
    g0 = 0
    for b, bt in zip(Gr.blocks(), Gr.blocks(transposed=True)):
        r = Gr.rows_h[g0:g0 + len(b)]; g0 += len(b)
        ref = G["adj"][np.ix_(r, r)]
        err = (np.abs(b - ref) / np.maximum(np.abs(ref), 1.0)).max()
        print("\nblock of %d rows on %s: max relative error %.3g" % (len(b), backend, err))
        assert err < 2e-4
        assert np.array_equal(bt.view(np.uint32), np.ascontiguousarray(b.T).view(np.uint32))
    assert g0 == 130


@pytest.mark.parametrize("form", ["general", "fused"])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_training_tracks_the_float64_oracle_as_closely_as_the_reference(backend, golden, form, p):
    T = golden("gcn_train_golden.npz")
    Gr = _fixture_graph(golden, cap_rows=133)
    ref64, loss0 = _oracle_run(p)
    key = "p%02d" % int(p * 10)
    for steps in (1, 10, 100):
        e_ref = np.abs(T["%s/w%d" % (key, steps)].astype(np.float64) - ref64[steps]).max()
        par, loss, info = Gr.train(T["init"], steps, p=p, seed=int(T["seed"]), form=form)
        e_dev = np.abs(par.astype(np.float64) - ref64[steps]).max()
        print("\n%s p=%.1f steps=%d on %s: device %.3g, reference %.3g (x %.2f)" % (form, p, steps, backend, e_dev, e_ref, e_dev / e_ref))
        assert info[3] == {"general": 1, "fused": 2}[form]
        assert e_dev <= 4 * e_ref
        assert abs(loss[0] - loss0) < 1e-5 * max(1.0, abs(loss0))
    if p == 0.0:
        assert loss[1] < loss[0]            # 100 steps lower the loss
    # evaluation rows after 100 steps, same bar
    ev, info = Gr.evaluate(par)
    G = golden("gcn_golden.npz")
    e64 = O.evaluate(G["featuresV"].astype(np.float64), G["adj"].astype(np.float64), ref64[100])
    e_ref = np.abs(T[key + "/eval100"].astype(np.float64) - e64).max()
    e_dev = np.abs(ev[:130] - e64).max()
    print("evaluation rows: device %.3g, reference %.3g" % (e_dev, e_ref))
    assert e_dev <= 4 * e_ref and info[2] == 0
    assert np.all(ev[130:] == -7.0)           # rows beyond the live count are not written
    assert abs(loss[1] - O.loss_of(e64, 100)) < 1e-4


@pytest.mark.parametrize("form", ["general", "fused"])
def test_same_call_twice_gives_the_same_bits(backend, golden, form):
    T = golden("gcn_train_golden.npz")
    Gr = _fixture_graph(golden)
    a = Gr.train(T["init"], 10, p=0.3, seed=3, form=form)
    b = Gr.train(T["init"], 10, p=0.3, seed=3, form=form)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    c = Gr.train(T["init"], 10, p=0.3, seed=4, form=form)
    assert not np.array_equal(a[0], c[0])       # the seed reaches the masks


def _random_graph(counts, n_unl, seed, labelled_only=None):
    """synthetic blocks of the given sizes (I plus non-symmetric entries of both signs: the training kernels do not care where a block comes from, and
    column sums near 0 as create_adj can produce saturate the sigmoid of the float64 oracle's autograd into NaN), rows scattered over the
    [unlabelled | labelled] order; labelled_only: a cloud whose rows are all labelled"""
    rng = np.random.default_rng(seed)
    N = int(sum(counts))
    blocks = []
    for n in counts:
        blocks.append((np.eye(n) + (rng.random((n, n)) - 0.4) * (0.8 / np.sqrt(n))).astype(np.float32))
    rows = rng.permutation(N).astype(np.int32)
    if labelled_only is not None:               # that cloud takes the last rows of the order
        g0 = int(sum(counts[:labelled_only])); n = counts[labelled_only]
        rest = np.concatenate([rows[:g0], rows[g0 + n:]])
        rest = np.argsort(np.argsort(rest)).astype(np.int32)      # the other rows, renumbered 0 .. N - n - 1
        rows = np.concatenate([rest[:g0], np.arange(N - n, N, dtype=np.int32), rest[g0:]])
    V = rng.standard_normal((N, 32)).astype(np.float32); V /= np.linalg.norm(V, axis=1, keepdims=True)
    return blocks, rows, V, n_unl


SHAPES = {
    "two_rows": dict(counts=[2, 2, 5], n_unl=6),
    "wave_edges": dict(counts=[63, 64, 65], n_unl=150),
    "labelled_only_cloud": dict(counts=[7, 9, 6], n_unl=13, labelled_only=1),
    "one_labelled_row": dict(counts=[5, 8], n_unl=12),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("form", ["general", "fused"])
def test_shapes_where_it_can_go_wrong(backend, shape, form):
    """float32 against the float64 oracle over 5 steps with dropout: 2e-5 absolute on parameters of magnitude <= 1 that move by <= 5e-3 (Adam steps of
    1e-3 whose direction m / sqrt(v) carries the gradient's float32 rounding, ~1e-6 relative, five times); NaN rows beyond the live count change nothing"""
    from ssdr_al import sampler
    kw = dict(SHAPES[shape]); counts = kw.pop("counts")
    blocks, rows, V, n_unl = _random_graph(counts, kw["n_unl"], 7, kw.get("labelled_only"))
    N = len(V)
    if "labelled_only" in kw:
        g0 = sum(counts[:kw["labelled_only"]])
        assert np.all(rows[g0:g0 + counts[kw["labelled_only"]]] >= n_unl)
    Gr = sampler.GcnGraph.from_blocks(V, blocks, rows, n_unl, cap_rows=N + 3)      # (the spare rows of V are NaN)
    init = sampler.gcn_init_params(5)
    init[4224:] *= 0.1
    A = O.dense_adj(blocks, rows, N)
    ref, loss0, _ = O.train(V.astype(np.float64), A, n_unl, init, 5, 0.3, seed=9, record=(5,))
    par, loss, info = Gr.train(init, 5, p=0.3, seed=9, form=form)
    assert np.isfinite(par).all() and np.abs(par - ref[5]).max() < 2e-5, np.abs(par - ref[5]).max()
    assert abs(loss[0] - loss0) < 1e-5 * max(1.0, abs(loss0))
    ev, info = Gr.evaluate(par)
    assert np.abs(ev[:N] - O.evaluate(V, A, par.astype(np.float64))).max() < 1e-4 and info[2] == 0


def test_fused_cap_and_the_form_auto_names(backend):
    """a cloud of exactly SSDR_GCN_FUSED_CAP rows runs fused under auto, one row more runs general; asking for fused there is SSDR_ERR_INVALID"""
    from ssdr_al import _lib, sampler
    cap = sampler.GCN_FUSED_CAP
    init = sampler.gcn_init_params(1); init[4224:] *= 0.1
    outs = {}
    for n in (cap, cap + 1):
        blocks, rows, V, n_unl = _random_graph([n, 3], n - 100, 11)
        Gr = sampler.GcnGraph.from_blocks(V, blocks, rows, n_unl)
        par, loss, info = Gr.train(init, 1, p=0.3, seed=2, form="auto")
        assert info[3] == (2 if n == cap else 1)
        gen, _, _ = Gr.train(init, 1, p=0.3, seed=2, form="general")
        assert np.abs(par - gen).max() < 1e-6           # one Adam step of 1e-3: the forms agree to float32 rounding
        outs[n] = Gr
    with pytest.raises(_lib.SsdrError) as e:
        outs[cap + 1].train(init, 1, form="fused")
    assert e.value.status == 1


def test_refusals_singleton_cloud_and_no_labelled_row(backend, golden):
    from ssdr_al import sampler
    g = golden("select_golden.npz")
    unl, lab, clouds = _refs(g)
    F = np.concatenate([g["g/unl_feat"], g["g/lab_feat"]])
    # cloud D contributes a single row
    keep_u = [i for i, r in enumerate(unl) if r["cloud_name"] == "cloudC"] + [next(i for i, r in enumerate(unl) if r["cloud_name"] == "cloudD")]
    keep_l = [i for i, r in enumerate(lab) if r["cloud_name"] == "cloudC"]
    Fs = np.concatenate([g["g/unl_feat"][keep_u], g["g/lab_feat"][keep_l]])
    Gr = sampler.GcnGraph.from_clouds(Fs, [lab[i] for i in keep_l], [unl[i] for i in keep_u], clouds)
    info = Gr.info()
    assert info[0] & sampler.GCN_ST_SINGLETON and Gr.cloud_names[info[1]] == "cloudD"
    init = sampler.gcn_init_params(0)
    with pytest.raises(ValueError, match="cloudD"):
        Gr.train(init, 3)
    par, _, _ = Gr.train(init, 3, check=False)
    assert np.array_equal(par, init)                    # nothing was trained, nothing is NaN
    with pytest.raises(ValueError, match="cloudD"):
        sampler.GCN_sampling(g["g/lab_feat"][keep_l], [lab[i] for i in keep_l], g["g/unl_feat"][keep_u], [unl[i] for i in keep_u], clouds, 5, steps=2)
    # no labelled row
    Gn = sampler.GcnGraph.from_clouds(g["g/unl_feat"], [], unl, clouds)
    with pytest.raises(ValueError, match="no labelled row"):
        Gn.train(init, 3)
    assert Gn.info()[0] & sampler.GCN_ST_NO_LABELLED
    with pytest.raises(ValueError, match="no labelled row"):
        sampler.GCN_sampling(np.zeros((0, 32), np.float32), [], g["g/unl_feat"], unl, clouds, 5, steps=2)
    assert len(F) == 130


def test_substitution_of_nan_and_inf(backend, golden):
    """an inf injected through the initial weights: b1[5] = +inf makes unit 5 of every row +inf (-> 1e10) and W3[5] = 0 turns the product into NaN in
    x (-> 1e-10); the count and the values must match gcn.py:241-245 applied to the oracle's rows"""
    T = golden("gcn_train_golden.npz"); G = golden("gcn_golden.npz")
    Gr = _fixture_graph(golden)
    par = T["init"].copy(); par[4096 + 5] = np.inf; par[4224 + 5] = 0.0
    ev, info = Gr.evaluate(par)
    with np.errstate(all="ignore"):
        e = O.evaluate(G["featuresV"], G["adj"], par.astype(np.float64))
    bad = np.isnan(e) | np.isinf(e)
    assert bad.sum() == 260 and info[2] == bad.sum() and info[0] & 128
    assert np.all(ev[np.isnan(e)] == 1e-10) and np.all(ev[np.isinf(e)] == 1e10)
    assert np.abs(ev[~bad] - e[~bad]).max() < 1e-4


def _selection_clouds():
    from _fabricate import make_clouds
    return make_clouds(41, 5, (24, 40), 3, 25, labelled_per_cloud=5)


def test_chain_and_python_callers(backend, golden):
    """from_clouds(selector="coregcn"): the candidate list of selector="fps" on the same ranking; the picks are oracle/select_np's k-center over the
    device's own 129-d rows; label_selected() runs after it; a communicator is refused"""
    from oracle import select_np as S
    from ssdr_al import pipeline
    import inspect
    clouds, labeled, sel_list = _selection_clouds()
    kw = dict(batch_size=30, round_num=2, seed=1)
    hp = pipeline.HotPath.from_clouds(clouds, labeled, sel_list, selector="coregcn", gcn_steps=50, gcn_seed=4, **kw)
    sel, unl = hp.step_selection()
    hf = pipeline.HotPath.from_clouds(clouds, labeled, sel_list, selector="fps", **kw)
    _, unl_f = hf.step_selection()
    assert list(unl) == list(unl_f)
    rows, par, loss, info = hp.gcn_rows()
    n_unl, n_lab = len(unl), hp._sel_static["n_lab"]
    assert info[0] == 0 and info[3] in (1, 2) and np.isfinite(loss).all() and np.isfinite(rows[:n_unl + n_lab]).all()
    exp = S.kcenter_greedy(rows[:n_unl + n_lab], np.arange(n_unl, n_unl + n_lab), len(sel))
    assert np.array_equal(np.asarray(sel), np.asarray(exp))
    assert len(set(sel.tolist())) == len(sel) and sel.min() >= 0 and sel.max() < n_unl
    res = hp.label_selected()
    assert len(res.used) > 0
    with pytest.raises(ValueError, match="communicator"):
        hp.step_selection(comm=object())
    assert "coregcn" in pipeline.SELECTORS
    assert pipeline.selector_for(["sb", "gcn"], trained_gcn=True) == "coregcn"
    assert pipeline.selector_for(["sb", "edcd", "gcn"], trained_gcn=True) == "edcd"
    assert pipeline.selector_for(["sb", "gcn", "gcn_fps"], trained_gcn=True) == "coregcn"
    assert pipeline.selector_for(["sb", "gcn_fps"], trained_gcn=True) == "fps"
    assert "trained_gcn" in inspect.signature(pipeline.selector_for).parameters


def test_al_round_with_the_trained_gcn_selector(backend):
    """ALRound(selector="coregcn") at the configuration of test_region_selectors.py's ALRound test: the round's one selection == HotPath.from_clouds
    over host copies of the round's arrays; ALRound.label() runs after it"""
    from oracle import randla_np as R
    from ssdr_al import pipeline, synthetic
    from ssdr_al.helper_tool import ConfigS3DIS
    emu = backend == "emu"

    class Cfg(ConfigS3DIS):
        num_points = 512 if emu else 40960
    W = R.init_weights(0)
    rooms = [synthetic.make_room(8100 + i, density=70.0 if emu else 2500.0) for i in range(2)]
    nb = 2 if emu else 6
    gk = dict(selector="coregcn", gcn_steps=20, gcn_seed=2)
    ar = pipeline.ALRound(W, rooms, nb, Cfg, batch_size=24, round_num=2, labeled_per_tile=3, precision="f32", **gk)
    sel, unl = ar.run()
    assert len(sel) == 24 and ar.sel.rule_path == "device" and len(set(sel.tolist())) == 24
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
    ref = pipeline.HotPath.from_clouds(clouds, labelled, S.selected_class_list.to_host(), Cfg, batch_size=24, round_num=2, **gk)
    rsel, runl = ref.step_selection()
    assert runl == unl and np.array_equal(rsel, sel) and ref.selected == S.selected
    assert len(ar.label().used) > 0


def test_reference_signature_wrapper(backend, golden):
    from ssdr_al import sampler
    g = golden("select_golden.npz")
    unl, lab, clouds = _refs(g)
    fl = sampler.GCN_sampling(g["g/lab_feat"], lab, g["g/unl_feat"], unl, clouds, 12, gcn_gpu=1, steps=20, seed=6)
    picks = [(n, s) for n in fl for s in fl[n]]
    assert len(picks) == 12 and len(set(picks)) == 12
    assert set(picks) <= set((r["cloud_name"], r["sp_idx"]) for r in unl)
    with pytest.raises(NotImplementedError):
        sampler.GCN_sampling(g["g/lab_feat"], lab, g["g/unl_feat"], unl, clouds, 12, coreGCN=False)


def test_every_gcn_form_name_is_reached(backend, golden):
    from ssdr_al import _lib
    src = open(os.path.join(ROOT, "ssdr-al_amd", "csrc", "select_gcn.hip")).read()
    names = sorted(set(re.findall(r'"(gcn_form:\w+)"', src)))
    assert names == ["gcn_form:fused", "gcn_form:general"]
    T = golden("gcn_train_golden.npz")
    Gr = _fixture_graph(golden)
    L = _lib.lib()
    _lib.check(L.ssdr_prof_enable(1))
    try:
        for form in ("general", "fused"):
            Gr.train(T["init"], 2, form=form)
        rep = L.ssdr_prof_report().decode()
    finally:
        _lib.check(L.ssdr_prof_enable(0))
    for n in names:
        assert re.search(r"^%s\s" % re.escape(n), rep, re.M), rep
