"""The sharded seed, random and label-all rounds: HotPath.seed_round(comm=), step_selection(comm) + label_selected(comm=comm) of "random" / "all" and
pipeline.ALRound(selector="random", comm=) with ALRound.seed, against the NumPy oracle (tests/_sampler_oracle.py) over the union of the ranks' clouds and
against ONE process over it, index for index.  gloo with the CPU logic build at worlds 2 (clouds 3 + 3) and 3 (3 + 2 + 1); RCCL at world 1 on the GPU
(-m gpu).  The worker is tests/_sampler_dist_worker.py; every comparison is exact, and every case asserts its input condition from the oracle first."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

WORKER = os.path.join(ROOT, "tests", "_sampler_dist_worker.py")
ST_MAX_ITER = 256


def _gloo(tmp_path, world, port, **env):
    env = dict(os.environ, SSDR_TEST_OUT=str(tmp_path), OMP_NUM_THREADS="2", SSDR_TEST_BACKEND="gloo", **env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1", "--master-port", str(port), WORKER]
    subprocess.run(cmd, check=True, env=env, timeout=1800, cwd=ROOT)
    return [dict(np.load(tmp_path / ("rank%d.npz" % i))) for i in range(world)]


def _rccl_world_one(tmp_path, port, **env):
    env = dict(os.environ, SSDR_TEST_OUT=str(tmp_path), SSDR_TEST_BACKEND="nccl", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", **env)
    subprocess.run([sys.executable, WORKER], check=True, env=env, timeout=300, cwd=ROOT)
    return [dict(np.load(tmp_path / "rank0.npz"))]


def _split(a, n):
    return np.split(a, np.cumsum(n)[:-1]) if len(n) else []


def _ids(pairs, gbase, rooms):
    """(room id, region in room) -> region ids of the union; `rooms`: the global cloud of every room id"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    return gbase[[rooms[int(r)] for r in pairs[:, 0]]] + pairs[:, 1] if len(pairs) else np.zeros(0, np.int64)


def _check_round(r, key, okey, skey, gbase, room_cloud, rooms_of):
    """the ranks' results under `key` merged into the union's order against the oracle's under `okey` and rank 0's single-process run under `skey`"""
    o = {k[len(okey):]: v for k, v in r[0].items() if k.startswith(okey)}
    s = {k[len(skey):]: v for k, v in r[0].items() if k.startswith(skey)}
    its = int(o["head"][0])
    # the single process is the oracle's round (so a rank's share of it is what the next lines compare)
    assert np.array_equal(s["head"], o["head"]) and np.array_equal(s["counters"], o["counters"]) and np.array_equal(s["entries"], o["entries"])
    assert np.array_equal(_ids(s["drawn"], gbase, room_cloud), o["drawn"]) and np.array_equal(s["drawn_n"], o["drawn_n"])
    assert np.array_equal(_ids(s["used"], gbase, room_cloud), o["used"]) and np.array_equal(s["pseudo"], o["pseudo"]) and np.array_equal(s["labeled"], o["labeled"])
    ranks = [{k[len(key):]: v for k, v in x.items() if k.startswith(key)} for x in r]
    for i, x in enumerate(ranks):
        # global and identical on every rank: iterations, status, budget_left, the counters, the class entries and list, k / live clouds / remainder / items
        assert np.array_equal(x["head"], o["head"]) and np.array_equal(x["counters"], o["counters"]) and np.array_equal(x["entries"], o["entries"]), "rank %d" % i
        assert np.array_equal(x["class_list"], s["class_list"])
        assert len(x["drawn_n"]) == its
        if "info" in o:
            assert np.array_equal(x["info"], o["info"]) and np.array_equal(x["each"], o["each"]) and np.array_equal(x["each_n"], o["each_n"]), "rank %d" % i
        assert all(int(room) in rooms_of[i] for room in x["drawn"][:, 0])
    # every iteration's items, merged by their positions in the union's list
    drawn = [_split(_ids(x["drawn"], gbase, room_cloud), x["drawn_n"]) for x in ranks]
    pos = [_split(x["pos"], x["drawn_n"]) for x in ranks]
    exp = _split(o["drawn"], o["drawn_n"])
    for it in range(its):
        merged = sorted((int(p), int(g)) for d, q in zip(drawn, pos) for p, g in zip(q[it], d[it]))
        assert [p for p, _ in merged] == list(range(len(exp[it]))) and [g for _, g in merged] == exp[it].tolist(), "items of iteration %d" % it
    # the used regions, merged by iteration and walk position (a seed round uses every item: by iteration and item position)
    if "walk_pos" in ranks[0]:
        used = [_split(_ids(x["used"], gbase, room_cloud), x["walk_n"]) for x in ranks]
        wpos = [_split(x["walk_pos"], x["walk_n"]) for x in ranks]
        merged = sorted((it, int(p), int(g)) for u, q in zip(used, wpos) for it in range(its) for p, g in zip(q[it], u[it]))
        assert len({(it, p) for it, p, _ in merged}) == len(merged)
    else:
        merged = sorted((it, int(p), int(g)) for d, q in zip(drawn, pos) for it in range(its) for p, g in zip(q[it], d[it]))
    assert [g for _, _, g in merged] == o["used"].tolist(), "the used regions"
    assert np.array_equal(np.concatenate([x["pseudo"] for x in ranks], axis=1), o["pseudo"]) and ranks[0]["pseudo"].dtype == np.float32, "pseudo labels"
    assert np.array_equal(np.concatenate([x["labeled"] for x in ranks]), o["labeled"]), "labelled mask"
    return o, ranks


def _check_cases(r, world):
    gbase = r[0]["gbase"]
    rooms_of = [set(x["rooms"].tolist()) for x in r]
    room_cloud = {c: c for c in range(len(gbase) - 1)}
    first = [int(gbase[min(rooms)]) for rooms in rooms_of] + [int(gbase[-1])]
    res = {}
    for case in ("rand60", "nail60", "pre34", "all155", "maxiter", "labelall", "seed60", "seed150", "seed155", "seedpre34"):
        res[case] = _check_round(r, case + "_sharded_", case + "_oracle_", case + "_single_", gbase, room_cloud, rooms_of)

    def used_per_rank(o):
        return [int(((o["used"] >= first[i]) & (o["used"] < first[i + 1])).sum()) for i in range(world)]
    # the input conditions, from the oracle
    o, _ = res["rand60"]
    live = _split(o["live"], o["info"][:, 1])
    assert o["drawn_n"].tolist() == [55, 6, 2, 2, 1] and live[0].tolist() == [0, 1, 2, 3, 4, 5] and live[-1].tolist() == [0, 2, 3, 4, 5]      # a cloud goes dead
    assert world == 1 or sum(n > 0 for n in used_per_rank(o)) >= 2
    o, _ = res["nail60"]
    names = ["ignore_sp_num", "p_num", "sp_num", "split_sp_num", "sub_num", "sub_p_num"]
    c = dict(zip(names, o["counters"].tolist()))
    assert c["split_sp_num"] > 0 and c["ignore_sp_num"] > 0 and c["sub_num"] > 0 and o["head"][2] <= 0
    if world == 3:
        assert used_per_rank(o) == [30, 9, 0] and len(res["nail60"][1][2]["drawn"]) > 0      # the budget ends before the last rank's items
    o, ranks = res["pre34"]
    assert o["head"][0] == 3 and not set(np.concatenate(_split(o["live"], o["info"][:, 1])).tolist()) & {3, 4}
    if world == 3:
        assert len(ranks[1]["drawn"]) == 0 and ranks[1]["labeled"].all()                       # the middle rank owns no live cloud
    o, _ = res["all155"]
    assert o["drawn_n"].tolist() == [112, 27, 16] and o["info"][:, 2].tolist() == [43, 16, 0]
    o, ranks = res["maxiter"]
    assert o["head"][0] == 32 and o["head"][1] == ST_MAX_ITER and all(x["head"][1] == ST_MAX_ITER for x in ranks)
    o, _ = res["labelall"]
    assert o["head"][0] == 1 and o["head"][2] == 0 and len(o["used"]) == 100 < len(o["drawn"]) == 155
    assert [int(res[c][0]["head"][0]) for c in ("seed60", "seed150", "seed155")] == [2, 3, 3]
    assert res["seed155"][0]["labeled"].all() and not res["seed150"][0]["labeled"].all() and res["seed155"][0]["counters"][2] == 155
    o, ranks = res["seedpre34"]
    assert o["head"][0] >= 1 and o["counters"][2] == 60
    if world == 3:
        assert len(ranks[1]["drawn"]) == 0 and len(ranks[0]["drawn"]) > 0 and len(ranks[2]["drawn"]) > 0      # a rank that labels nothing before the all-reduce
    for x in r:
        assert x["refusals"].tolist() == [1, 1, 1, 1]              # draws="host" (selection, seed round), "coregcn", labelling without the communicator


def _check_alround(r, world):
    gbase = r[0]["al_gbase"]
    assert sorted(b for x in r for b in x["al_batches"].tolist()) == [0, 1, 2] and all(len(x["al_batches"]) for x in r)
    assert [len(x["al_batches"]) for x in r] == {1: [3], 2: [2, 1], 3: [1, 1, 1]}[world]
    rooms_of = [set(x["al_rooms"].tolist()) for x in r]
    room_cloud = {t: t for t in range(6)}
    o, _ = _check_round(r, "al_sharded_seed_", "al_oracle_seed_", "al_single_seed_", gbase, room_cloud, rooms_of)
    assert o["counters"][2] == 11                                   # sp_num
    for i in (1, 2):
        o, _ = _check_round(r, "al_sharded_round%d_" % i, "al_oracle_round%d_" % i, "al_single_round%d_" % i, gbase, room_cloud, rooms_of)
        assert len(o["used"]) > 0 and o["head"][0] >= 1


@pytest.mark.parametrize("shards,port", [("3,3", 29583), ("3,2,1", 29585)])
def test_sharded_seed_random_and_label_all_rounds_equal_the_oracle_over_the_union(tmp_path, emu_lib, shards, port):
    world = len(shards.split(","))
    _check_cases(_gloo(tmp_path, world, port, SSDR_TEST_SHARDS=shards, SSDR_TEST_PART="cases"), world)


@pytest.mark.parametrize("world,port", [(2, 29587), (3, 29589)])
def test_sharded_al_round_seed_then_two_random_rounds(tmp_path, emu_lib, world, port):
    """ALRound(selector="random", comm=) with 3 batches as 2 + 1 and 1 + 1 + 1: seed(), then run() + label() twice"""
    _check_alround(_gloo(tmp_path, world, port, SSDR_TEST_PART="alround"), world)


def _check_reload(r, world):
    """the second load gives rank 0 more clouds and more regions than any rank held in the first: tables kept from the first pool would be too small"""
    S = [np.stack([x["reload%d_S" % k] for x in r]) for k in (0, 1)]
    assert S[1][0, 0] > S[0][:, 0].max() and S[1][0, 1] > S[0][:, 1].max()
    for k in (0, 1):
        key = "reload%d_" % k
        gbase = r[0][key + "gbase"]
        rooms_of = [set(x[key + "rooms"].tolist()) for x in r]
        room_cloud = {t: t for t in range(len(gbase) - 1)}
        o, _ = _check_round(r, key + "sharded_seed_", key + "oracle_seed_", key + "single_seed_", gbase, room_cloud, rooms_of)
        assert o["counters"][2] == 9
        o, _ = _check_round(r, key + "sharded_random_", key + "oracle_random_", key + "single_random_", gbase, room_cloud, rooms_of)
        assert len(o["used"]) > 0


@pytest.mark.parametrize("world,port", [(2, 29593), (3, 29595)])
def test_reloaded_rooms_under_the_same_communicator(tmp_path, emu_lib, world, port):
    """load_rooms() again with other shares of other rooms: every table of the sharded rounds belongs to the round, none to the communicator"""
    _check_reload(_gloo(tmp_path, world, port, SSDR_TEST_PART="reload"), world)


@pytest.mark.gpu
def test_rccl_world_one_equals_the_plain_calls(tmp_path):
    """every case and the ALRound through RCCL at world 1: bit for bit the same calls without a communicator (and the oracle's round)"""
    from conftest import _have_gpu
    if not _have_gpu():
        pytest.skip("no GPU")
    r = _rccl_world_one(tmp_path, 29591, SSDR_TEST_SHARDS="6", SSDR_TEST_PART="all")
    _check_cases(r, 1)
    _check_alround(r, 1)
    _check_reload(r, 1)
    for k in [k for k in r[0] if "_sharded_" in k]:
        if k.replace("_sharded_", "_single_") in r[0] and not k.endswith(("walk_pos", "walk_n")):
            assert np.array_equal(r[0][k], r[0][k.replace("_sharded_", "_single_")]), k
