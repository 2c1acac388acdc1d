"""The sharded AL round: step_selection(comm) -> label_selected(comm=comm) -> step_selection(comm), and pipeline.ALRound(comm=), against ONE process over
the union of the clouds, index for index.  gloo with the CPU logic build at worlds 2 and 3; RCCL at world 1 on the GPU (-m gpu).  The worker is
tests/_label_dist_worker.py; every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

WORKER = os.path.join(ROOT, "tests", "_label_dist_worker.py")
SELECTORS = ("fps", "kcenter", "edcd", "topk")


def _gloo(tmp_path, world, port, **env):
    env = dict(os.environ, SSDR_TEST_OUT=str(tmp_path), OMP_NUM_THREADS="2", SSDR_TEST_BACKEND="gloo", **env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1", "--master-port", str(port), WORKER]
    subprocess.run(cmd, check=True, env=env, timeout=1800, cwd=ROOT)
    return [dict(np.load(tmp_path / ("rank%d.npz" % i))) for i in range(world)]


def _rccl_world_one(tmp_path, port, **env):
    """one child process per GPU step, each under its own time limit"""
    env = dict(os.environ, SSDR_TEST_OUT=str(tmp_path), SSDR_TEST_BACKEND="nccl", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", **env)
    subprocess.run([sys.executable, WORKER], check=True, env=env, timeout=300, cwd=ROOT)
    return [dict(np.load(tmp_path / "rank0.npz"))]


def _tuples(a):
    return [tuple(int(v) for v in p) for p in a]


def _check_labelling(r, key, skey, rooms_of):
    """ranks r under `key` against rank 0's single-process run under `skey`"""
    single = r[0]
    s_used = _tuples(single[skey + "used"])
    merged = sorted((int(w), p) for x in r for w, p in zip(x[key + "walk_pos"], _tuples(x[key + "used"])))
    assert [p for _, p in merged] == s_used                               # the ranks' used picks merged by their walk positions
    assert len({w for w, _ in merged}) == len(merged)
    for i, x in enumerate(r):
        assert all(p[0] in rooms_of[i] for p in _tuples(x[key + "used"]))
        assert np.array_equal(x[key + "counters"], single[skey + "counters"])          # the six counters, budget_left, regions per form: global on every rank
        assert np.array_equal(x[key + "class_list"], single[skey + "class_list"]) and np.array_equal(x[key + "entries"], single[skey + "entries"])
        for b in rooms_of[i]:
            assert np.array_equal(x[key + "pseudo%d" % b], single[skey + "pseudo%d" % b]) and x[key + "pseudo%d" % b].dtype == np.float32
        assert _tuples(x[key + "labeled"]) == [p for p in _tuples(single[skey + "labeled"]) if p[0] in rooms_of[i]]


def _check_select_part(r, world):
    rooms_of = [set(x["rooms"].tolist()) for x in r]
    for sel in SELECTORS:
        skey = sel + "_single_"
        single, single2 = _tuples(r[0][skey + "selected"]), _tuples(r[0][skey + "selected2"])
        assert len(single) == 40 and len(single2) == 40 and not set(single2) & set(_tuples(r[0][skey + "used"]))
        # from the oracle: some pick stays unused, some region is split, at least two ranks have processed items
        unused, split = r[0][skey + "facts"].tolist()
        assert unused > 0 and split > 0
        if world > 1:
            assert sum(bool(rooms & set(r[0][skey + "used_clouds"].tolist())) for rooms in rooms_of) >= 2
        for rule in ("device", "host"):
            key = "%s_%s_" % (sel, rule)
            for i, x in enumerate(r):
                assert int(x[key + "path"][0]) == (rule == "device") and int(x[key + "refused"][0]) == 1
                for which, ref in (("selected", single), ("selected2", single2)):      # fps / k-center: the global picks on every rank; edcd / topk: a rank's own
                    assert _tuples(x[key + which]) == (ref if sel in ("fps", "kcenter") else [p for p in ref if p[0] in rooms_of[i]])
            _check_labelling(r, key, skey, rooms_of)


@pytest.mark.parametrize("shards,notop,port", [("3,3", -1, 29571), ("3,2,1", 2, 29573)])
def test_sharded_selection_labelling_and_next_round_equal_single_process(tmp_path, emu_lib, shards, notop, port):
    world = len(shards.split(","))
    r = _gloo(tmp_path, world, port, SSDR_TEST_SHARDS=shards, SSDR_TEST_NOTOP_RANK=str(notop), SSDR_TEST_PART="select")
    _check_select_part(r, world)


def _check_alround(r, second):
    single = r[0]
    assert sorted(b for x in r for b in x["batches"].tolist()) == [0, 1, 2] and all(len(x["batches"]) for x in r)
    rooms_of = [{2 * b + i for b in x["batches"].tolist() for i in range(2)} for x in r]
    picks = _tuples(single["single_selected"])
    assert len(picks) == 24 and int(single["single_path"][0]) == 2
    for x in r:
        assert int(x["refused"][0]) == 1 and int(x["sharded_path"][0]) == 1
        assert _tuples(x["sharded_selected"]) == picks                      # the fps round: the global picks, on every rank
        if second:
            assert _tuples(x["sharded_selected2"]) == _tuples(single["single_selected2"]) and len(x["sharded_selected2"]) == 24
    assert len(single["single_used"]) > 0
    _check_labelling(r, "sharded_", "single_", rooms_of)


@pytest.mark.parametrize("world,port", [(2, 29575), (3, 29577)])
def test_sharded_al_round_equals_single_process(tmp_path, emu_lib, world, port):
    """ALRound(comm=) with 3 batches over 2 (2 + 1 batches) and 3 ranks: run(), label(), run() == the single-process ALRound; a world above n_batches is refused"""
    _check_alround(_gloo(tmp_path, world, port, SSDR_TEST_PART="alround"), second=True)


@pytest.mark.gpu
def test_rccl_world_one_label_selected_equals_plain_path(tmp_path):
    from conftest import _have_gpu
    if not _have_gpu():
        pytest.skip("no GPU")
    _check_select_part(_rccl_world_one(tmp_path, 29579, SSDR_TEST_SHARDS="6", SSDR_TEST_PART="select"), 1)


@pytest.mark.gpu
def test_rccl_world_one_al_round_equals_plain_al_round(tmp_path):
    from conftest import _have_gpu
    if not _have_gpu():
        pytest.skip("no GPU")
    _check_alround(_rccl_world_one(tmp_path, 29581, SSDR_TEST_PART="alround"), second=False)
