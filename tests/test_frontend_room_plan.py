"""Room plans (include/ssdr_al.h: ssdr_rooms_plan_create_dev / ssdr_tile_from_rooms_planned_batch_dev / ssdr_rooms_plan_destroy; csrc/frontend.hip: FePlan).
A plan keeps what the bucket partition derives from the rooms' points and dl alone; a planned call must be ssdr_tile_from_rooms_batch_dev on the same inputs BIT FOR
BIT: the tiles (xyz, feat, labels), the sub-sampled rows and their counts, the status word, and both stats calls.  The unplanned call is the reference: its own tests
(test_frontend_tile_prune.py, test_frontend_scatter_prune.py) hold it to the two calls it stands for.  Every case runs on the CPU logic build and on the gfx950 build.

Rooms are 5 k to 200 k raw points, tiles 1024 rows, dl 0.04."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal
from _fe_paths import F32, FE_CAP, geometry
from test_frontend_tile_prune import DL, FE_TO_NMAX, SCALE, _box, _room, _short_estimate_room

N = 1024
ERR_INVALID = 1
KEYS = ("xyz", "feat", "lab", "sub_p", "sub_f", "sub_l", "m", "status", "stage", "reduced", "buckets", "scattered", "points")


def _room_g(rng, p, fdim, ldim):
    """raw rows of a room with any row layout: fdim feature columns 0..255, ldim label columns in [0,13), the rows shuffled"""
    p = np.ascontiguousarray(p, F32)[rng.permutation(len(p))]
    return p, rng.integers(0, 256, (len(p), fdim)).astype(F32), rng.integers(0, 13, (len(p), ldim)).astype(np.int32)


class _Set:
    """an uploaded set of rooms with the tiles' randomness; call() = one front-end call over it (planned or not) -> every output, the status and the stats"""

    def __init__(self, rooms, seed, fdim=3, ldim=1):
        from ssdr_al import _lib
        from ssdr_al._lib import DevArray
        self.L = _lib.lib()
        rng = np.random.default_rng(seed)
        self.R, self.fdim, self.ldim = len(rooms), fdim, ldim
        self.off = np.concatenate([[0], np.cumsum([len(r[0]) for r in rooms])]).astype(np.int64)
        self.nt = int(self.off[-1])
        self.perm = DevArray.from_host(np.stack([rng.permutation(N) for _ in range(self.R)]).astype(np.int32))
        dup = rng.random((self.R, N)).astype(F32)
        dup[:, -1] = 1.0
        self.dup = DevArray.from_host(dup)
        self.d_p = DevArray.from_host(np.concatenate([r[0] for r in rooms]))
        self.d_f = DevArray.from_host(np.concatenate([r[1] for r in rooms])) if fdim else None
        self.d_l = DevArray.from_host(np.concatenate([r[2] for r in rooms])) if ldim else None
        self.plans = []

    def _in(self, off=None, R=None, dl=DL):
        from ssdr_al import _lib
        return (self.d_p.ptr, self.d_f.ptr if self.fdim else None, self.fdim, self.d_l.ptr if self.ldim else None, self.ldim,
                _lib.ptr(self.off if off is None else off), self.R if R is None else R, dl)

    def plan(self, stream=None):
        from ssdr_al import _lib
        p = C.c_void_p()
        _lib.check(self.L.ssdr_rooms_plan_create_dev(*self._in(), stream, C.byref(p)))
        assert p.value
        self.plans.append(p.value)
        return p.value

    def destroy(self, plan):
        from ssdr_al import _lib
        self.plans.remove(plan)
        _lib.check(self.L.ssdr_rooms_plan_destroy(plan))

    def close(self):
        for p in list(self.plans):
            self.destroy(p)

    def raw_call(self, centres, plan, stream=None, **kw):
        """the status code of the call alone (outputs allocated and dropped)"""
        return self._call(centres, plan, stream, **kw)[0]

    def _call(self, centres, plan, stream, **kw):
        from ssdr_al import _lib
        from ssdr_al._lib import DevArray
        R, nt, fd, ld = self.R, self.nt, self.fdim, self.ldim
        # every output starts from a sentinel: what a call does not write compares equal only if the other call did not write it either
        o = dict(sub_p=DevArray.from_host(np.full((nt, 3), -77.25, F32)), sub_f=DevArray.from_host(np.full((nt, max(fd, 1)), -77.25, F32)),
                 sub_l=DevArray.from_host(np.full((nt, max(ld, 1)), -77, np.int32)), m=DevArray.from_host(np.full(R + 1, -77, np.int64)),
                 xyz=DevArray.from_host(np.full((R, N, 3), -77.25, F32)), feat=DevArray.from_host(np.full((R, N, 3 + fd), -77.25, F32)),
                 lab=DevArray.from_host(np.full((R, N), -77, np.int32)))
        cen = np.ascontiguousarray(np.asarray(centres, F32).reshape(-1, 3))
        args = self._in(**kw) + (o["sub_p"].ptr, o["sub_f"].ptr if fd else None, o["sub_l"].ptr if ld else None, o["m"].ptr, _lib.ptr(cen), N, self.perm.ptr, self.dup.ptr,
                                 SCALE, o["xyz"].ptr, o["feat"].ptr, None, o["lab"].ptr if ld == 1 else None, stream)
        rc = self.L.ssdr_tile_from_rooms_planned_batch_dev(plan, *args) if plan is not None else self.L.ssdr_tile_from_rooms_batch_dev(*args)
        return rc, o

    def call(self, centres, plan=None, stream=None):
        from ssdr_al import _lib
        L, R = self.L, self.R
        rc, o = self._call(centres, plan, stream)
        _lib.check(rc)
        st = C.c_int32(-1)
        L.ssdr_grid_subsample_status(stream, C.byref(st))          # (waits for the stream; non-zero return = a non-zero status word, which the cases compare)
        out = {k: v.to_host() for k, v in o.items()}
        out["status"] = np.array([st.value])
        stats = [np.full(R, -5, np.int32) for _ in range(3)]
        _lib.check(L.ssdr_tile_from_rooms_stats(stream, *[_lib.ptr(a) for a in stats], R))
        sc, pts = np.full(R, -5, np.int64), np.full(R, -5, np.int64)
        _lib.check(L.ssdr_tile_from_rooms_scatter_stats(stream, _lib.ptr(sc), _lib.ptr(pts), R))
        out.update(stage=stats[0], reduced=stats[1], buckets=stats[2], scattered=sc, points=pts)
        out["m"] = out["m"][:R]
        return out


def _same(got, ref, what):
    for k in KEYS:
        assert_bits_equal(got[k], ref[k], "%s: %s" % (what, k))
    assert (ref["xyz"] != F32(-77.25)).any() and (ref["m"] > 0).any()


def _three_rooms(rng):
    """60 k, 30 k and 8 k points at about one point per occupied voxel: stage 1 suffices with a part of the first two rooms' buckets"""
    return [_room(rng, _box(rng, 60000, (4.0, 3.0, 2.5))), _room(rng, _box(rng, 30000, (3.0, 2.5, 2.0), (10.0, -4.0, 1.0))), _room(rng, _box(rng, 8000, (2.0, 1.5, 1.0), (-5.0, 0.0, 0.0)))]


# ---- 1. one plan, many centres ---------------------------------------------------------------------------------------------------------------------
def test_one_plan_three_sets_of_centres(backend):
    """The plan is built once; three calls with different centres (in the middle of the rooms; at a corner of every room; outside every box) each equal the
    unplanned call with those centres, and differ from one another: nothing of a call's centres stays in the plan."""
    rng = np.random.default_rng(101)
    S = _Set(_three_rooms(rng), 102)
    try:
        plan = S.plan()
        sets = [[(2.0, 1.5, 1.25), (11.5, -2.7, 2.0), (-4.0, 0.7, 0.5)],
                [(0.01, 0.02, 0.01), (12.99, -1.51, 2.99), (-5.0, 1.5, 0.0)],
                [(4.9, -0.6, 3.1), (9.2, -4.5, 0.4), (-2.5, 0.7, 1.6)]]
        outs = []
        for i, cen in enumerate(sets):
            got, ref = S.call(cen, plan), S.call(cen)
            _same(got, ref, "centres %d" % i)
            assert list(got["stage"]) == [1, 1, 1] and got["reduced"][0] < got["buckets"][0] and 0 < got["scattered"][0] < got["points"][0]
            outs.append(got)
        assert not np.array_equal(outs[0]["xyz"], outs[1]["xyz"]) and not np.array_equal(outs[1]["xyz"], outs[2]["xyz"])
    finally:
        S.close()


# ---- 2. the later stages ---------------------------------------------------------------------------------------------------------------------------
def _few_voxels_many_points(rng):
    """test_frontend_tile_prune._short_estimate_room with fewer voxels than the tile has rows: about 400 voxels of 8 duplicates around the centre and about 500 of 100
    duplicates in the rest of 6.4 x 6.4 x 2.56 m.  Stage 1's 6 x 1024 points and stage 2's estimate both end short of 1024 rows: stage 3 reduces the rest of the room,
    and the tile is padded with the duplicate draws."""
    nv = np.array([160, 160, 64])
    c = (nv // 2).astype(np.float64)
    ijk = np.stack(np.meshgrid(*[np.arange(k) for k in nv], indexing="ij"), -1).reshape(-1, 3)
    inner = ((ijk + 0.5 - c) ** 2).sum(1) < 100.0
    u = rng.random(len(ijk))
    a, b = ijk[inner & (u < 0.10)], ijk[~inner & (u < 0.0003)]
    cells = np.concatenate([np.repeat(a, 8, 0), np.repeat(b, 100, 0)])
    jitter = np.repeat(rng.random((len(a) + len(b), 3)), np.concatenate([np.full(len(a), 8), np.full(len(b), 100)]), 0)
    return ((cells + 0.1 + 0.8 * jitter) * DL).astype(F32), (c * DL).astype(F32), len(a) + len(b)


def test_stage_two_and_stage_three_with_padding(backend):
    """One call over: a room of 16 points per occupied voxel (stage 2 holds the tile: test_frontend_tile_prune.test_stage_two); a room of fewer voxels than the tile
    whose points are many (stage 3, then the padding branch); the room whose estimate falls short (stage 3, rows to spare).  The stages are read from the stats of the
    planned call."""
    rng = np.random.default_rng(111)
    nv = np.array([60, 60, 50])
    cells = np.stack(np.unravel_index(rng.choice(int(nv.prod()), 12500, replace=False), nv), 1)
    dense = ((np.repeat(cells, 16, 0) + 0.1 + 0.8 * np.repeat(rng.random((len(cells), 3)), 16, 0)) * DL).astype(F32)
    few, c_few, nvox = _few_voxels_many_points(rng)
    assert nvox < N and len(few) > 6 * N
    short, c_short, n_in, n_out = _short_estimate_room(rng)
    S = _Set([_room(rng, dense), _room(rng, few), _room(rng, short)], 112)
    try:
        plan = S.plan()
        cen = [(1.2, 1.3, 1.0), c_few, c_short]
        got, ref = S.call(cen, plan), S.call(cen)
        print("stage %s, reduced %s of %s, rows %s" % (got["stage"], got["reduced"], got["buckets"], got["m"]))
        _same(got, ref, "stages")
        assert list(got["stage"]) == [2, 3, 3]
        assert got["m"][1] == nvox < N and got["m"][2] == n_in + n_out > N and got["reduced"][0] < got["buckets"][0]
        assert list(got["scattered"][1:]) == list(got["points"][1:])          # a room that goes on is scattered whole
    finally:
        S.close()


# ---- 3. rooms that leave the common route ----------------------------------------------------------------------------------------------------------------
def test_refused_and_unordered_rooms_beside_normal_ones(backend):
    """A voxel of more than FE_CAP points (status bit 4), a grid of more than 16384 buckets (bit 2: no row, its tile stays as it was) and a slab of more than FE_TO_NMAX
    non-empty buckets (reduced whole: stage 0) beside two normal rooms: status bits, stats and every output as from the unplanned call."""
    rng = np.random.default_rng(121)
    crowd = np.concatenate([_box(rng, 30000, (3.0, 3.0, 2.0)), np.tile(np.array([[1.5, 1.5, 1.0]], F32) + F32(0.003), (FE_CAP + 80, 1))])
    assert geometry(crowd, DL).vox_members.max() > FE_CAP
    huge = _box(rng, 5000, (100.0, 100.0, 3.0))
    assert not geometry(huge, DL).fits
    sparse = _box(rng, 40000, (52.0, 34.0, 0.3))
    gs = geometry(sparse, DL)
    assert gs.fits and np.count_nonzero(gs.records) > FE_TO_NMAX
    normal = _three_rooms(rng)
    S = _Set([normal[1], _room(rng, crowd), _room(rng, huge), _room(rng, sparse), normal[2]], 122)
    try:
        plan = S.plan()
        cen = [(11.5, -2.7, 2.0), (1.52, 1.49, 1.02), (50.0, 50.0, 1.5), (21.0, 13.0, 0.15), (-4.0, 0.7, 0.5)]
        got, ref = S.call(cen, plan), S.call(cen)
        _same(got, ref, "refused")
        assert got["status"][0] & 4 and got["status"][0] & 2
        assert list(got["stage"]) == [1, 1, 0, 0, 1] and got["m"][2] == 0 and got["reduced"][3] == got["buckets"][3] > FE_TO_NMAX
        assert (got["xyz"][2] == F32(-77.25)).all()
    finally:
        S.close()


# ---- 4. the generic row layout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fdim,ldim", [(2, 2), (0, 1)])
def test_generic_row_layout(backend, fdim, ldim):
    """rows that are not 3 features + 1 label take fe_scatter<-1, -1, *> / fe_reduce<-1, -1, *> / fe_move<-1, -1>, through the plan as without it"""
    rng = np.random.default_rng(131)
    rooms = [_room_g(rng, _box(rng, 40000, (4.0, 3.0, 2.5)), fdim, ldim), _room_g(rng, _box(rng, 9000, (2.0, 1.5, 1.0), (7.0, 0.0, 0.0)), fdim, ldim),
             _room_g(rng, _box(rng, 20000, (3.0, 2.0, 2.0), (0.0, 9.0, 0.0)), fdim, ldim)]
    S = _Set(rooms, 132, fdim, ldim)
    try:
        plan = S.plan()
        for cen in ([(2.0, 1.5, 1.2), (8.0, 0.7, 0.5), (1.5, 10.0, 1.0)], [(0.0, 0.0, 0.0), (9.1, 1.6, 1.1), (3.0, 9.0, 2.0)]):
            got, ref = S.call(cen, plan), S.call(cen)
            _same(got, ref, "layout %d + %d" % (fdim, ldim))
            assert got["reduced"][0] < got["buckets"][0]
    finally:
        S.close()


# ---- 5. the plan does not live in the per-stream scratch ------------------------------------------------------------------------------------------------------
def test_unplanned_call_on_other_rooms_between_planned_calls(backend):
    """planned call, an unplanned call over OTHER rooms on the same stream (it rewrites every per-stream table of the partition), planned call again: both planned
    calls equal the references taken before"""
    rng = np.random.default_rng(141)
    A, B = _Set(_three_rooms(rng), 142), _Set([_room(rng, _box(rng, 50000, (6.0, 2.0, 2.0), (3.0, 3.0, 3.0))), _room(rng, _box(rng, 70000, (5.0, 5.0, 2.5))),
                                               _room(rng, _box(rng, 12000, (1.0, 4.0, 2.0), (-9.0, 0.0, 0.0))), _room(rng, _box(rng, 6000, (1.0, 1.0, 1.0)))], 143)
    try:
        c1, c2 = [(2.0, 1.5, 1.25), (11.5, -2.7, 2.0), (-4.0, 0.7, 0.5)], [(3.5, 0.4, 2.2), (10.2, -3.9, 1.2), (-3.3, 1.2, 0.2)]
        r1, r2 = A.call(c1), A.call(c2)
        plan = A.plan()
        g1 = A.call(c1, plan)
        other = B.call([(6.0, 4.0, 4.0), (2.5, 2.5, 1.2), (-8.5, 2.0, 1.0), (0.5, 0.5, 0.5)])
        g2 = A.call(c2, plan)
        _same(g1, r1, "before")
        _same(g2, r2, "after")
        assert len(other["m"]) == 4 and (other["m"] > 0).all()
    finally:
        A.close(); B.close()


# ---- 6. streams ------------------------------------------------------------------------------------------------------------------------------------
def test_plan_built_on_one_stream_used_on_another(backend):
    """built on stream a; the first use is on stream b (ordered behind the build by the plan's event), then on the library's stream and on a again; the stats are
    those of the stream of the call"""
    from ssdr_al import _lib
    L = _lib.lib()
    rng = np.random.default_rng(151)
    S = _Set(_three_rooms(rng), 152)
    a, b = C.c_void_p(), C.c_void_p()
    _lib.check(L.ssdr_stream_create(C.byref(a))); _lib.check(L.ssdr_stream_create(C.byref(b)))
    try:
        cen = [(2.0, 1.5, 1.25), (11.5, -2.7, 2.0), (-4.0, 0.7, 0.5)]
        plan = S.plan(a.value)
        got_b = S.call(cen, plan, b.value)
        ref = S.call(cen)
        _same(got_b, ref, "stream b")
        _same(S.call(cen, plan), ref, "library stream")
        _same(S.call(cen, plan, a.value), ref, "stream a")
        _same(S.call(cen, plan, b.value), ref, "stream b again")
    finally:
        S.close()
        _lib.check(L.ssdr_stream_destroy(a)); _lib.check(L.ssdr_stream_destroy(b))


# ---- 7. a plan answers for its own inputs only ----------------------------------------------------------------------------------------------------------------
def test_mismatch_is_refused(backend):
    from ssdr_al import _lib
    rng = np.random.default_rng(161)
    S = _Set(_three_rooms(rng), 162)
    try:
        plan = S.plan()
        cen = [(2.0, 1.5, 1.25), (11.5, -2.7, 2.0), (-4.0, 0.7, 0.5)]
        moved = S.off.copy(); moved[1] += 7
        for what, kw in (("dl", dict(dl=0.05)), ("room_off", dict(off=moved)), ("one room fewer", dict(R=2))):
            assert S.raw_call(cen, plan, **kw) == ERR_INVALID, what
            assert b"plan" in S.L.ssdr_last_error(), what
        _same(S.call(cen, plan), S.call(cen), "after the refusals")
    finally:
        S.close()


# ---- 8. new points, new plan -------------------------------------------------------------------------------------------------------------------------------
def test_rebuilt_plan_follows_the_new_points(backend):
    """destroy, rewrite the points in place (the same device pointers and offsets), create: the planned call is the unplanned call over the new points"""
    from ssdr_al import _lib
    rng = np.random.default_rng(171)
    rooms = _three_rooms(rng)
    S = _Set(rooms, 172)
    try:
        cen = [(2.0, 1.5, 1.25), (11.5, -2.7, 2.0), (-4.0, 0.7, 0.5)]
        plan = S.plan()
        old = S.call(cen, plan)
        _same(old, S.call(cen), "old points")
        S.destroy(plan)
        # other boxes: the grids' origins, dimensions and every bucket count change
        new_p = np.concatenate([_box(rng, 60000, (3.0, 4.0, 2.0), (0.5, -0.5, 0.2)), _box(rng, 30000, (2.0, 3.0, 2.5), (10.5, -4.0, 0.5)), _box(rng, 8000, (1.5, 2.0, 1.2), (-4.5, 0.0, 0.0))])
        assert new_p.shape == S.d_p.shape
        _lib.check(S.L.ssdr_memcpy_h2d(S.d_p.ptr, _lib.ptr(new_p), new_p.nbytes))
        plan = S.plan()
        new = S.call(cen, plan)
        _same(new, S.call(cen), "new points")
        assert not np.array_equal(new["xyz"], old["xyz"]) and not np.array_equal(new["buckets"], old["buckets"])
    finally:
        S.close()


# ---- 9. the hot path ---------------------------------------------------------------------------------------------------------------------------------
def test_hot_path_switch(backend, monkeypatch):
    """HotPath.load_rooms builds the plan; two steps with it and two under SSDR_FE_ROOM_PLAN=0 (the unplanned call, same build) give the same tiles, network
    outputs and selection.  The workload of bench.py --emu (tests/test_bench_launch.py): two rooms at density 80, tiles of 1024 rows."""
    from oracle import randla_np as R
    from ssdr_al import pipeline, synthetic
    from ssdr_al.helper_tool import ConfigS3DIS

    class Cfg(ConfigS3DIS):
        num_points = 1024
    monkeypatch.delenv("SSDR_FE_ROOM_PLAN", raising=False)
    monkeypatch.delenv("SSDR_FE_TILE_PRUNE", raising=False)
    rooms = [synthetic.make_room(5000 + i, density=80.0) for i in range(2)]
    hp = pipeline.HotPath(R.init_weights(0), Cfg, select_per_tile=5, labeled_per_tile=2).load_rooms(rooms)
    try:
        assert hp._room_plan is not None and hp.subsample_method == 0
        runs = []
        for switch in (None, None, "0", "0"):
            if switch is not None:
                monkeypatch.setenv("SSDR_FE_ROOM_PLAN", switch)
            for a in (hp.xyz, hp.feat, hp.tile_l, hp.sub_m):          # the step must write them anew
                hp_fill = np.zeros(a.shape, a.dtype)
                from ssdr_al import _lib
                _lib.check(_lib.lib().ssdr_memcpy_h2d(a.ptr, _lib.ptr(hp_fill), hp_fill.nbytes))
            sel, unl = hp.step()
            runs.append(dict(sel=np.asarray(sel), unl=np.asarray(unl), xyz=hp.xyz.to_host(), feat=hp.feat.to_host(), lab=hp.tile_l.to_host(), m=hp.sub_m.to_host()[:hp.B],
                             probs=hp.probs.to_host(), f32=hp.f32.to_host()))
        for i in (1, 2, 3):
            for k, v in runs[0].items():
                assert_bits_equal(runs[i][k], v, "step %d: %s" % (i, k))
        assert (runs[0]["m"] > 0).all() and len(runs[0]["sel"]) > 0
    finally:
        hp.close()
    assert hp._room_plan is None
    # a HotPath loaded with the switch off keeps no plan
    hp2 = pipeline.HotPath(R.init_weights(0), Cfg, select_per_tile=5, labeled_per_tile=2).load_rooms(rooms)
    assert hp2._room_plan is None
    assert_bits_equal(hp2.xyz.to_host(), runs[0]["xyz"], "loaded without a plan: xyz")


# ---- 10. the plan's lifetime under the sanitizers -------------------------------------------------------------------------------------------------------
def test_plan_lifetime_under_asan_ubsan():
    """a stand-alone program (tests/san/room_plan_main.cpp) linked with the sanitized objects of the CPU logic build: create on one stream, the first planned call
    on another, the three mismatches, destroy, create again over new points, and the arguments no plan is built from, over exactly sized arrays; no report"""
    import os
    import subprocess
    from conftest import PKG, ROOT
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(PKG, "csrc"), "room-plan-san"])
    env = dict(os.environ, OMP_NUM_THREADS="4", ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "san", "room_plan_san")], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
    assert "room plan ok" in r.stdout
