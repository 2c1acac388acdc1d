"""Farthest-point sampling and k-center greedy, launcher branch by launcher branch, against the float64 oracle (oracle/select_np.py).

fps_like() (csrc/select_fps.hip) picks one of eight kernels and one of three seedings from (D, n, seeded, environment); a wrong pick still returns
`count` plausible indices.  It names what it took in two zero-work profiler scopes inside "fps_chain" ("fps_form:*", "fps_seed:*").  Every case here
runs through the C ABI (ssdr_fps_dev: squared distances; ssdr_kcenter_dev: their square roots, seeded by kc_init / kc_init_tiled), must equal
oracle.select_np.farthest_features_sample / kcenter_greedy INDEX FOR INDEX, must leave ssdr_select_status at 0 with no pick of -1, and must report
the scopes its `reach` names (and none of the other forms).  Brackets are written for the MI355X's 256 CUs: on another CU count a case fails by name.

Input condition, not a tolerance: for every case without deliberate ties the smallest relative gap between the largest and the second-largest entry of
the oracle's `distance` over all picks is computed from the oracle alone and asserted >= 1e-9 before the library's answer is looked at (summation-order
differences are bounded by about D * 2^-52 <= 3e-14 relative for D <= 129; standard-normal inputs give 1e-7 .. 1e-4).  Tie cases use exact duplicates
("every row twice at shuffled positions") or small integers, whose distances are bit-identical under any order; there np.argmax's first index is the
expectation.

The CPU logic build has a smaller dispatch (no cooperative kernels): D = 32 and n <= 1536 -> block_reg<1/2/3>; n <= 16384 -> block<32> (D = 32) or
block<0>; above -> step (one launch per pick).  Its leg runs every case with n <= 20 000 at the case's own n (count clipped to 40 above 2000 rows) and
checks the form that build must take; "fps_form:block<32>" is reached there only (on the GPU it needs the occupancy query to refuse the cooperative
grid, which no test may force).

No environment switch selects a form.  The two that change what a form does (SSDR_KC_TILED = 0: kc_init at every size; SSDR_FPS_SLOT_SHIFT: the size of
a coop_split record's slot) are read once per process: tests/_fps_forms_worker.py runs them in one child process per environment, one after another.

The live row count below the capacity (`d_n`) is reached through ssdr_fps_gathered_dev / ssdr_kcenter_gathered_dev, whose compacted array the caller
owns: rows beyond the live count hold 1e30, which would win every arg-max if a kernel read them.

Measured on one MI355X: `pytest -m gpu tests/test_fps_paths.py` = 109 tests in 28 s wall, most of it the NumPy oracle.  Slowest: the three child
processes under 1 s to 3.9 s each (kc_tiled0 3.9 s), rest_coop_far 2.1 s, n262144 1.3 s, d129_n70001 1.2 s; the one-launch-per-pick cases: n2pow20 (2^20 + 7 rows
x 8 picks) 1.1 s, n262145 (30 picks) 1.0 s, ties_step 1.0 s, kc_step 0.8 s.  The CPU logic build's leg (`-m "not gpu"`, 88 tests): about 50 s on 16
threads.  Smallest arg-max gap met over all cases: 4.3e-7 (n5003).
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _fps_oracle import SENTINEL, make_features, make_seeds, run_abi, trace_fps, trace_kcenter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP_FLOOR = 1e-9
ORACLE_BYTES = 2.0e9          # oracle.select_np.kcenter_greedy materialises n x na x D float64


class Case:
    def __init__(self, name, n, D, count, start=7, na=0, data="normal", seeds="random", reach=(), why=""):
        self.name, self.n, self.D, self.count, self.start, self.na, self.data, self.seeds, self.reach, self.why = name, n, D, count, min(start, n - 1), na, data, seeds, list(reach), why
        assert any(r.startswith("fps_form:") for r in self.reach) and any(r.startswith("fps_seed:") for r in self.reach), name

    @property
    def emu(self):
        return self.n <= 20000

    def emu_count(self):
        return self.count if self.n <= 2000 else min(self.count, 40)


def _fps(name, n, form, count=60, D=32, **kw):
    return Case(name, n, D, count, reach=["fps_form:" + form, "fps_seed:fill"], **kw)


def _kc(name, n, na, form, seed="kc_init", count=60, D=32, **kw):
    return Case(name, n, D, count, na=na, reach=["fps_form:" + form, "fps_seed:" + seed], **kw)


R1, R2, R3, SP2, COOP, B0, STEP = "block_reg<1>", "block_reg<2>", "block_reg<3>", "coop_split<2>", "coop", "block<0>", "step"

CASES = [
    # ---- D = 32, unseeded: both sides of every bracket of the default dispatch (FR_ROWS = 512; split<2>: 256 rows per workgroup, at most 256 of them) ----
    _fps("n1", 1, R1, count=1, start=0, why="one row, one pick"),
    _fps("n2", 2, R1, count=2, start=1),
    _fps("n64", 64, R1, count=40, why="one full wave"), _fps("n65", 65, R1, count=40, why="one row in the second wave"),
    _fps("n512", 512, R1, count=100, why="last size with one row per thread"), _fps("n513", 513, R2, count=100),
    _fps("n1024", 1024, R2, count=100), _fps("n1025", 1025, R3, count=100),
    _fps("n1536", 1536, R3, count=150, why="last single-workgroup size"), _fps("n1537", 1537, SP2, count=150, why="first cooperative size: 7 workgroups, the last with one row"),
    _fps("n5003", 5003, SP2, count=100, why="odd tail of the last workgroup and of the two-lanes-per-row split"),
    _fps("n16384", 16384, SP2, count=100), _fps("n16385", 16385, SP2, count=100, why="G = 65: one row in the last workgroup"),
    _fps("n18176", 18176, SP2, count=100, why="G = 71: the shorter delay in front of the first polling pass"),
    _fps("n18432", 18432, SP2, count=100, why="G = 72: the longer delay"),
    _fps("n33333", 33333, SP2, why="n odd, not a multiple of 64 / 256 / 512"),
    _fps("n65280", 65280, SP2, why="G = 255"), _fps("n65536", 65536, SP2, why="G = 256: the last split size"),
    _fps("n65537", 65537, COOP, why="first size of fps_coop with D = 32"),
    _fps("n100001", 100001, COOP, count=40), _fps("n131073", 131073, COOP, count=40, why="G saturated at num_cu / 2: 1025 rows over two lanes of a workgroup"),
    _fps("n262144", 262144, COOP, count=40, why="the last cooperative size: FC_NT * FC_PPT rows in every workgroup"),
    _fps("n262145", 262145, STEP, count=30, why="first size of the one-launch-per-pick loop"),
    _fps("n2pow20", (1 << 20) + 7, STEP, count=8, why="about 2^20 rows (DESIGN: the chain works to 2^22): nb = 512 partials ping-ponged between p0 / p1"),
    _fps("start0", 3001, SP2, start=0), _fps("start_last", 3001, SP2, start=3000), _fps("start_last_reg", 1300, R3, start=1299),
    # ---- D != 32: fps_block<0> to 4096 rows, fps_coop above, fps_step beyond 262 144 ----
    *[_fps("d%d_n4096" % D, 4096, B0, D=D, why="last single-workgroup size for D != 32") for D in (1, 3, 16, 31, 33, 129)],
    *[_fps("d%d_n4097" % D, 4097, COOP, D=D, why="first cooperative size for D != 32: G = 9") for D in (1, 3, 16, 31, 33, 129)],
    _fps("d16_n65536", 65536, COOP, D=16, why="G reaches num_cu / 2"), _fps("d16_n262144", 262144, COOP, D=16, count=40),
    _fps("d16_n262145", 262145, STEP, D=16, count=30), _fps("d129_n70001", 70001, COOP, D=129, count=40),
    # ---- seeded (k-center; use_sqrt = 1): kc_init feeds `from_partials = 1` of every form ----
    _kc("kc_reg1", 400, 50, R1), _kc("kc_reg2", 900, 100, R2), _kc("kc_reg3", 1400, 200, R3),
    _kc("kc_na999", 4000, 999, SP2, why="n * na = 3 996 000: the last kc_init size"),
    _kc("kc_na1001", 4000, 1001, SP2, seed="kc_init_tiled", why="n * na = 4 004 000: the first tiled size"),
    _kc("kc_na1", 3000, 1, SP2, why="one seed"),
    _kc("kc_most_selected", 2000, 1970, SP2, count=30, why="na = n - count: almost everything already selected"),
    _kc("kc_dup_seeds", 2500, 300, SP2, seeds="dups", why="a quarter of the seed list repeats other seeds"),
    _kc("kc_dup_seeds_reg", 1000, 120, R2, seeds="dups"),
    _kc("kc_d129_n4096", 4096, 200, B0, D=129), _kc("kc_d129_n4097", 4097, 200, COOP, D=129),
    _kc("kc_coop32", 70000, 20, COOP, count=40, why="seeded fps_coop with D = 32"),
    _kc("kc_coop32_tiled", 70000, 60, COOP, seed="kc_init_tiled", count=40, why="n * na = 4.2e6: tiled seeding in front of fps_coop"),
    _kc("kc_step", 262145, 4, STEP, count=20, why="seeded one-launch-per-pick loop: the first launch reads kc_init's partials"),
    # ---- count = n (FPS) and count = n - na and beyond (k-center): integers in [-8, 8], exact under any summation order; one n per form ----
    *[_fps("all_" + nm, n, form, count=n, D=D, data="ints", why="count = n: the last picks are ties at distance 0") for nm, n, form, D in
      (("reg1", 300, R1, 32), ("reg2", 700, R2, 32), ("reg3", 1200, R3, 32), ("split2", 1700, SP2, 32), ("coop", 4100, COOP, 16), ("block0", 600, B0, 16))],
    *[_kc("rest_%s%s" % (nm, "_plus5" if extra else ""), n, na, form, count=n - na + extra, D=D, data="ints",
          why="count = n - na%s: every further pick is np.argmax of an all-zero distance, index 0" % (" + 5" if extra else "")) for nm, n, na, form, D in
      (("reg3", 1200, 200, R3, 32), ("split2", 1800, 300, SP2, 32), ("coop", 4100, 3000, COOP, 16), ("block0", 600, 100, B0, 16)) for extra in (0, 5)],
    *[_kc("rest_%s_far" % nm, n, na, form, count=2 * n, D=D, data="ints", why="count = 2 n, far above n - na: the entry accepts it, the outputs are written by pick "
          "number and every pick behind n - na is index 0") for nm, n, na, form, D in (("reg3", 1200, 200, R3, 32), ("split2", 1800, 300, SP2, 32), ("coop", 4100, 3000, COOP, 16))],
    # ---- ties: every row twice at shuffled positions, twins in other waves / workgroups ----
    *[_fps("ties_" + nm, n, form, count=c, D=D, data="ties") for nm, n, form, D, c in
      (("reg1", 400, R1, 32, 150), ("reg2", 900, R2, 32, 150), ("reg3", 1400, R3, 32, 150), ("split2", 5000, SP2, 32, 150), ("split2_g256", 65536, SP2, 32, 60),
       ("coop32", 70000, COOP, 32, 60), ("coop16", 6000, COOP, 16, 150), ("block0", 2000, B0, 16, 150), ("step", 262146, STEP, 32, 30))],
    _kc("kc_ties_split2", 5000, 100, SP2, count=150, data="ties"), _kc("kc_ties_coop16", 6000, 100, COOP, D=16, count=150, data="ties"),
    _kc("kc_ties_reg3", 1400, 100, R3, count=150, data="ties"),
]
assert len({c.name for c in CASES}) == len(CASES)


def _emu_form(n, D):
    """what the CPU logic build's dispatch takes"""
    if D == 32 and n <= 1536:
        return "fps_form:block_reg<%d>" % (1 if n <= 512 else 2 if n <= 1024 else 3)
    if n <= 16384:
        return "fps_form:block<32>" if D == 32 else "fps_form:block<0>"
    return "fps_form:step"


def _expected(case, f, already, count):
    """the oracle's sequence; the replay (which also yields the gap) must give the same one wherever the oracle itself is affordable"""
    from oracle import select_np as O
    if already is None:
        seq, gap = trace_fps(f, count, case.start)
        assert np.array_equal(seq, O.farthest_features_sample(f, count, case.start))
    else:
        seq, gap = trace_kcenter(f, already, count)
        assert case.n * case.na * case.D * 8.0 <= ORACLE_BYTES, "case above the oracle's memory bound"
        assert np.array_equal(seq, O.kcenter_greedy(f, already, count))
    if case.data == "normal":
        print("%s: smallest relative arg-max gap %.3e" % (case.name, gap))
        assert gap >= GAP_FLOOR, "input condition: a pick of %s hangs on rounding (gap %.3e): give the case another seed" % (case.name, gap)
    return seq


def _check(case, emu):
    count = case.emu_count() if emu else case.count
    f = make_features(case.data, case.n, case.D, case.n + case.D)
    already = make_seeds(case.seeds, case.n, case.na, case.n) if case.na else None
    exp = _expected(case, f, already, count)
    rc, got, src, st, names = run_abi(f, count, start=case.start, already=already)
    assert rc == 0 and src == 0 and st == 0, (case.name, rc, src, st)
    assert not (got < 0).any(), (case.name, "a pick of -1")
    forms = {nm for nm in names if nm.startswith("fps_form:")}
    seeds = {nm for nm in names if nm.startswith("fps_seed:")}
    assert "fps_chain" in names and len(forms) == 1 and len(seeds) == 1, (case.name, names)
    want = {_emu_form(case.n, case.D)} | {r for r in case.reach if r.startswith("fps_seed:")} if emu else set(case.reach)      # (the seeding rule is the same in both builds)
    assert forms | seeds == want, "%s took %s, the case is written for %s" % (case.name, sorted(forms | seeds), sorted(want))
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, "%s (%s): %d of %d picks differ from the oracle, first at pick %d: %d, oracle %d" % (
        case.name, sorted(forms), bad.size, count, bad[0], got[bad[0]], exp[bad[0]])


@pytest.mark.parametrize("case", [c for c in CASES if c.emu], ids=lambda c: c.name)
def test_fps_case_emu(emu_lib, case):
    from ssdr_al import _lib
    _lib.use(emu_lib)
    try:
        _check(case, True)
    finally:
        _lib.use(None)


def _gpu_lib():
    from conftest import GPU_LIB, _have_gpu
    if not _have_gpu():
        pytest.skip("no GPU")
    assert os.path.exists(GPU_LIB), "libssdr_al.so missing: run __graft_entry__.build()"
    return GPU_LIB


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_fps_case_gpu(case):
    from ssdr_al import _lib
    _lib.use(_gpu_lib())
    try:
        _check(case, False)
    finally:
        _lib.use(None)


# ---- count and start edges, what the entry refuses ------------------------------------------------------------------------------------
EDGE_SIZES = [(300, 32), (700, 32), (1200, 32), (1700, 32), (600, 16), (4100, 16)]       # one n per form of the default dispatch


def _edges(n, D):
    from oracle import select_np as O
    f = make_features("normal", n, D, 3 * n)
    for start in (0, n - 1):
        rc, got, src, st, names = run_abi(f, 0, start=start)
        assert (rc, src, st, len(got)) == (0, 0, 0, 0) and not names           # (run_abi checks that the buffer still holds its sentinel)
        for count in (1, 2):
            rc, got, src, st, names = run_abi(f, count, start=start)
            assert (rc, src, st) == (0, 0, 0) and np.array_equal(got, O.farthest_features_sample(f, count, start)), (n, D, start, count, got)
    for count, start in ((n + 1, 0), (1, n), (2, -1)):
        rc, got, src, st, names = run_abi(f, count, start=start)
        assert rc == 1 and not names and (got == SENTINEL).all(), (n, D, count, start, rc, names)      # SSDR_ERR_INVALID
    already = make_seeds("random", n, 5, n)
    rc, got, src, st, names = run_abi(f, 0, already=already)
    assert (rc, src, st) == (0, 0, 0) and not names
    for count in (1, 2):
        rc, got, src, st, names = run_abi(f, count, already=already)
        assert (rc, src, st) == (0, 0, 0) and np.array_equal(got, O.kcenter_greedy(f, already, count)), (n, D, count, got)


@pytest.mark.parametrize("n,D", EDGE_SIZES, ids=["%dx%d" % e for e in EDGE_SIZES])
def test_count_and_start_edges(backend, n, D):
    """count = 0 returns OK and leaves the output untouched, count = 1 is `start` alone, count = 2 one arg-max; start = 0 and n - 1; count = n + 1 or
    start = n is SSDR_ERR_INVALID and launches nothing (no profiler scope, output untouched).  k-center: count = 0, 1, 2 behind the seeding."""
    _edges(n, D)


@pytest.mark.gpu
@pytest.mark.parametrize("n,D", [(70000, 32), (262145, 32)], ids=["coop32", "step"])
def test_count_and_start_edges_large_gpu(n, D):
    """the same edges on fps_coop with D = 32 and on the one-launch-per-pick loop (count = 1: the only launch is the last one)"""
    from ssdr_al import _lib
    _lib.use(_gpu_lib())
    try:
        _edges(n, D)
    finally:
        _lib.use(None)


# ---- the live row count below the capacity ------------------------------------------------------------------------------------------------
def _gathered(selector, cap, live, n_lab, count, data):
    """ssdr_fps_gathered_dev / ssdr_kcenter_gathered_dev of one rank over `live` rows with capacity `cap`: the plan names the rows of the gathered array in
    candidate order (a permutation here); d_glob holds 1e30 everywhere before the call -> (picks, scope names, the live rows in the order the entry lays them out)"""
    import ctypes as C
    from ssdr_al import _lib
    L = _lib.lib()
    rng = np.random.default_rng(cap + live)
    kc = selector == "kcenter"
    n_unl = live - (n_lab if kc else 0)
    nu_max, nl_max = n_unl + 3, (n_lab + 2 if kc else 0)
    rows = make_features(data, nu_max + nl_max, 32, cap + 7 * live)
    rows[n_unl:nu_max] = 1e30                                         # the padding of the all-gather: never named by the plan
    rows[nu_max + n_lab:] = 1e30
    perm = rng.permutation(n_unl).astype(np.int32)
    plan = np.zeros(16 + 1 + 2 * nu_max, np.int32)
    plan[0], plan[8], plan[16] = n_unl, n_unl, n_unl
    plan[17:17 + n_unl] = perm
    d_g, d_p = _lib.DevArray.from_host(rows), _lib.DevArray.from_host(plan)
    d_glob = _lib.DevArray.from_host(np.full((cap, 32), 1e30))
    d_o = _lib.DevArray.from_host(np.full(count + 1, SENTINEL, np.int32))
    L.ssdr_prof_report(); L.ssdr_prof_enable(1)
    try:
        if kc:
            d_off, d_a = _lib.DevArray.from_host(np.array([0, n_lab], np.int32)), _lib.DevArray((n_lab,), np.int32)
            _lib.check(L.ssdr_kcenter_gathered_dev(d_g.ptr, d_p.ptr, 1, nu_max, nl_max, d_off.ptr, n_lab, cap, count, d_glob.ptr, d_a.ptr, d_o.ptr, None))
        else:
            _lib.check(L.ssdr_fps_gathered_dev(d_g.ptr, d_p.ptr, 1, nu_max, cap, 1, 5, count, d_glob.ptr, d_o.ptr, None))
        st = C.c_int(0)
        assert L.ssdr_select_status(None, C.byref(st)) == 0 and st.value == 0
        names = {ln.rsplit(" ", 4)[0] for ln in L.ssdr_prof_report().decode().splitlines() if ln.strip()}
    finally:
        L.ssdr_prof_enable(0)
    out = d_o.to_host()
    assert out[-1] == SENTINEL
    glob = d_glob.to_host()
    live_rows = np.concatenate([rows[perm], rows[nu_max:nu_max + n_lab]]) if kc else rows[perm]
    assert np.array_equal(glob[:live], live_rows) and (glob[live:] == 1e30).all()
    return out[:count], names, live_rows


# (capacity, live rows, labelled rows of the k-center leg, GPU form, CPU-build form)
LIVE = [(1500, 400, 60, R3, R3, "capacity in block_reg<3>'s bracket, fewer than 512 live rows: two of the three rows of a thread are beyond the count"),
        (1600, 1200, 150, SP2, "block<32>", "capacity just above 1536 with the live rows below it: 7 workgroups, two of them wholly empty"),
        (1600, 200, 40, SP2, "block<32>", "all but the first workgroup empty"),
        (20000, 1900, 300, SP2, "step", "capacity 20 000, under 2000 live: 79 workgroups, 71 empty"),
        (70000, 9000, 200, COOP, "step", "capacity above 65 536 (fps_coop with D = 32): 128 workgroups, the live rows in the first lanes of each"),
        (300000, 5000, 300, STEP, "step", "capacity in the one-launch-per-pick loop's range")]


@pytest.mark.parametrize("selector", ["fps", "kcenter"])
@pytest.mark.parametrize("cap,live,n_lab,form,emu_form,why", LIVE, ids=["cap%d_live%d" % (c[0], c[1]) for c in LIVE])
def test_live_count_below_capacity(backend, selector, cap, live, n_lab, form, emu_form, why):
    """d_n: the launch is shaped by the capacity, the rows are counted on the device.  Rows beyond the live count hold 1e30 (they would win every
    arg-max if read); the picks must be the oracle's over the live rows alone, for standard-normal rows and for every row twice."""
    from oracle import select_np as O
    count = 40
    for data in ("normal", "ties"):
        got, names, rows = _gathered(selector, cap, live, n_lab, count, data)
        want_form = "fps_form:" + (emu_form if backend == "emu" else form)
        seed = "fps_seed:fill" if selector == "fps" else ("fps_seed:kc_init_tiled" if cap * n_lab > 4.0e6 else "fps_seed:kc_init")
        assert {nm for nm in names if nm.startswith(("fps_form:", "fps_seed:"))} == {want_form, seed}, (names, want_form, seed)
        if selector == "kcenter":
            already = np.arange(live - n_lab, live)
            exp, gap = trace_kcenter(rows, already, count)
            assert np.array_equal(exp, O.kcenter_greedy(rows, already, count))
        else:
            exp, gap = trace_fps(rows, count, 5)
            assert np.array_equal(exp, O.farthest_features_sample(rows, count, 5))
        assert data == "ties" or gap >= GAP_FLOOR, gap
        assert (got < live).all() and (got >= 0).all(), "a pick beyond the live count: %s" % got
        assert np.array_equal(got, exp), (selector, cap, live, data, got, exp)


# ---- the environment switches, one child process per environment ----------------------------------------------------------------------------
# (id, environment, [(n, na of the seeded leg, form, seeding of the seeded leg)]); D = 32 throughout.
ENV_ROWS = [
    ("kc_tiled0", {"SSDR_KC_TILED": "0"}, [(24000, 4000, "coop_split<2>", "kc_init")]),
    ("slot_shift4", {"SSDR_FPS_SLOT_SHIFT": "4"}, [(4736, 100, "coop_split<2>", "kc_init")]),
    ("slot_shift7", {"SSDR_FPS_SLOT_SHIFT": "7"}, [(4736, 100, "coop_split<2>", "kc_init")]),
]
ENV_NAMES = ("SSDR_KC_TILED", "SSDR_FPS_SLOT_SHIFT", "SSDR_FPS_COOP_G", "SSDR_FPS_COOP_BUDGET", "SSDR_FPS_DELAY", "SSDR_FPS_DBG")


@pytest.mark.gpu
@pytest.mark.parametrize("name,env_add,sizes", ENV_ROWS, ids=[r[0] for r in ENV_ROWS])
def test_environment_selected_forms(name, env_add, sizes):
    """Every environment switch that changes what a chain does, in a child process of its own (the switches are read once per process; never two GPU
    children at a time): for every size FPS and k-center, each over standard-normal rows and over every row twice, index for index the oracle's sequence,
    status 0, and the form / seeding the dispatch must have taken under that environment."""
    _gpu_lib()
    env = {k: v for k, v in os.environ.items() if k not in ENV_NAMES}
    env.update(env_add)
    args = ["%d:%d" % (n, na) for n, na, _, _ in sizes]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_fps_forms_worker.py")] + args, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
    assert len(lines) == 4 * len(sizes), r.stdout
    want = {(n, leg): {"fps_form:" + form, "fps_seed:" + (seed if leg.startswith("kc") else "fill")} for n, _, form, seed in sizes for leg in ("fps", "fps_ties", "kc", "kc_ties")}
    for _, n, leg, rc, st, minus, match, gap_ok, forms in lines:
        assert (int(rc), int(st), int(minus)) == (0, 0, 0), (name, n, leg, r.stdout)
        assert set(forms.split(",")) == want[(int(n), leg)], "%s n=%s %s took %s, expected %s" % (name, n, leg, forms, sorted(want[(int(n), leg)]))
        assert int(gap_ok) == 1, (name, n, leg, "input condition")
        assert int(match) == 1, "%s n=%s %s (%s): the picks differ from the oracle\n%s" % (name, n, leg, forms, r.stdout)


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------------
def test_replay_equals_the_oracle():
    """the replay the big seeded leg of the worker relies on (24 000 x 4000 x 32 doubles do not fit the oracle's one tensor) is the oracle, bit for bit"""
    from oracle import select_np as O
    for kind, n, D, na in (("normal", 900, 32, 300), ("ties", 700, 16, 90), ("ints", 500, 129, 40)):
        f = make_features(kind, n, D, 1)
        a = make_seeds("dups", n, na, 2)
        assert np.array_equal(trace_kcenter(f, a, 120, chunk=37)[0], O.kcenter_greedy(f, a, 120))
        assert np.array_equal(trace_fps(f, 120, 3)[0], O.farthest_features_sample(f, 120, 3))


def test_cases_cover_every_form_and_seeding():
    """Every "fps_form:" / "fps_seed:" name of select_fps.hip is reached by a case that asserts it at run time (the default dispatch above, the environment
    rows, the live-count cases).  One exception: fps_block<32> runs on the GPU only when the occupancy query refuses the cooperative grid, which no test
    may force; it counts as covered by the CPU logic build's cases (every D = 32 case of 1537 .. 16 384 rows takes it there)."""
    src = open(os.path.join(ROOT, "ssdr-al_amd", "csrc", "select_fps.hip")).read()
    names = set(re.findall(r'"(fps_(?:form|seed):[^"]+)"', src))
    assert names == {"fps_form:block_reg<1>", "fps_form:block_reg<2>", "fps_form:block_reg<3>", "fps_form:block<0>", "fps_form:block<32>", "fps_form:step", "fps_form:coop",
                     "fps_form:coop_split<2>", "fps_seed:fill", "fps_seed:kc_init", "fps_seed:kc_init_tiled"}, sorted(names)
    gpu = {r for c in CASES for r in c.reach} | {"fps_form:" + form for _, _, sizes in ENV_ROWS for _, _, form, _ in sizes} | \
          {"fps_seed:" + seed for _, _, sizes in ENV_ROWS for _, _, _, seed in sizes}
    emu = {_emu_form(c.n, c.D) for c in CASES if c.emu}
    assert "fps_form:block<32>" in emu and "fps_form:block<32>" not in gpu
    assert names - (gpu | {"fps_form:block<32>"}) == set(), "forms no case reaches: %s" % sorted(names - gpu)
    assert (gpu | emu) - names == set(), "cases name forms the source does not have: %s" % sorted((gpu | emu) - names)
    assert {"fps_form:block_reg<1>", "fps_form:block_reg<2>", "fps_form:block_reg<3>", "fps_form:block<0>", "fps_form:block<32>", "fps_form:step"} <= emu


def test_profiler_reports_form_names_on_emu(emu_lib):
    """the checks above rely on ssdr_prof_report naming the form in the CPU logic build too, and on "fps_chain" keeping its name and its work figure"""
    from ssdr_al import _lib
    _lib.use(emu_lib)
    try:
        L = _lib.lib()
        f = make_features("normal", 700, 32, 1)
        d_f, d_o = _lib.DevArray.from_host(f), _lib.DevArray((50,), np.int32)
        L.ssdr_prof_report(); L.ssdr_prof_enable(1)
        try:
            _lib.check(L.ssdr_fps_dev(d_f.ptr, 700, 32, 0, 50, d_o.ptr, None))
            rep = {ln.rsplit(" ", 4)[0]: ln.rsplit(" ", 4)[1:] for ln in L.ssdr_prof_report().decode().splitlines() if ln.strip()}
        finally:
            L.ssdr_prof_enable(0)
        assert set(rep) == {"fps_chain", "fps_form:block_reg<2>", "fps_seed:fill"}, rep
        assert int(rep["fps_chain"][0]) == 1 and float(rep["fps_chain"][2]) == 50 * (700 * 32 * 8.0 + 16.0 * 700)
        assert float(rep["fps_form:block_reg<2>"][2]) == 0.0 and float(rep["fps_seed:fill"][2]) == 0.0
        L.ssdr_prof_report()
        _lib.check(L.ssdr_fps_dev(d_f.ptr, 700, 32, 0, 50, d_o.ptr, None))
        assert L.ssdr_prof_report().decode().strip() == ""                 # profiling off: nothing is recorded
    finally:
        _lib.use(None)
