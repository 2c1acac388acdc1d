"""Shared by tests/test_fps_paths.py and its worker tests/_fps_forms_worker.py: inputs of the FPS / k-center dispatch cases, the two entry points through
the C ABI with the profiler's form names, and a replay of oracle/select_np.py's two loops that also returns the smallest relative gap between the
largest and the second-largest entry of `distance` over all picks (the input condition of an index-for-index comparison).  Test infrastructure only:
the expected sequences are oracle.select_np's; the replay is checked against it wherever the oracle's n x na x D tensor fits in memory."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

SENTINEL = -7          # what the output buffer holds before a call


def make_features(kind, n, D, seed):
    """normal: standard normal float64; ties: every row twice at shuffled positions (n odd: one row once); ints: integers in [-8, 8] with
    a few duplicated rows (every squared distance exact in float64 under any summation order)"""
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.normal(size=(n, D))
    if kind == "ties":
        half = rng.normal(size=((n + 1) // 2, D))
        return np.concatenate([half, half])[:n][rng.permutation(n)]
    if kind == "ints":
        f = rng.integers(-8, 9, (n, D)).astype(np.float64)
        if n >= 8:
            dup = rng.choice(n, 2 * (n // 8), replace=False)
            f[dup[: n // 8]] = f[dup[n // 8:]]
        return f
    raise ValueError(kind)


def make_seeds(kind, n, na, seed):
    """random: na distinct rows; dups: na entries, a quarter of them repeats of other entries; tail: the last na rows (as the one-call chain lays them out)"""
    rng = np.random.default_rng(seed + 1)
    if kind == "tail":
        return np.arange(n - na, n).astype(np.int32)
    a = rng.choice(n, na, replace=False)
    if kind == "dups" and na >= 4:
        a[: na // 4] = a[na // 4: 2 * (na // 4)]
    return a.astype(np.int32)


def _gap(distance):
    if len(distance) < 2:
        return np.inf
    top = np.partition(distance, -2)[-2:]
    return (top[1] - top[0]) / top[1] if top[1] > 0 else 0.0


def trace_fps(f, count, start):
    """oracle.select_np.farthest_features_sample's loop, statement for statement, with the gap of every arg-max -> (sequence, smallest gap)"""
    f = np.asarray(f, np.float64)
    cent = np.zeros(count, np.int32)
    if count:
        cent[0] = start
    distance = np.ones(len(f)) * 1e10
    gap = np.inf
    for i in range(count - 1):
        dist = np.sum((f - f[cent[i]]) ** 2, axis=-1)
        mask = dist < distance
        distance[mask] = dist[mask]
        cent[i + 1] = np.argmax(distance)
        gap = min(gap, _gap(distance))
    return cent, gap


def trace_kcenter(f, already, count, chunk=256):
    """oracle.select_np.kcenter_greedy's loop with the seeding computed over `chunk` rows at a time (the same expression row by row, so the same bits:
    every row's sum runs over its own D contiguous terms) -> (sequence, smallest gap)"""
    f = np.asarray(f, np.float64)
    a = np.asarray(already)
    md = np.empty(len(f))

    def seed(lo):
        md[lo:lo + chunk] = np.sqrt(((f[lo:lo + chunk, None, :] - f[None, a, :]) ** 2).sum(-1)).min(1)
    with ThreadPoolExecutor(8) as pool:          # (NumPy releases the lock inside its loops)
        list(pool.map(seed, range(0, len(f), chunk)))
    out, gap = [], np.inf
    for _ in range(count):
        ind = int(np.argmax(md))
        gap = min(gap, _gap(md))
        d = np.sqrt(((f - f[ind]) ** 2).sum(-1))
        md = np.minimum(md, d)
        out.append(ind)
    return np.asarray(out, np.int32), gap


def run_abi(f, count, start=None, already=None, n=None):
    """ssdr_fps_dev (already is None) or ssdr_kcenter_dev on the library _lib.use() selected -> (rc, picks, status rc, status word, fps_* scope names)"""
    from ssdr_al import _lib
    L = _lib.lib()
    f = np.ascontiguousarray(f, np.float64)
    n = len(f) if n is None else n
    d_f = _lib.DevArray.from_host(f if f.size else np.zeros((1, 1)))
    d_o = _lib.DevArray.from_host(np.full(max(count, 1) + 1, SENTINEL, np.int32))
    L.ssdr_prof_report()                                   # drop anything recorded before
    L.ssdr_prof_enable(1)
    try:
        if already is None:
            rc = L.ssdr_fps_dev(d_f.ptr, n, f.shape[1], start, count, d_o.ptr, None)
        else:
            d_a = _lib.DevArray.from_host(np.ascontiguousarray(already, np.int32))
            rc = L.ssdr_kcenter_dev(d_f.ptr, n, f.shape[1], d_a.ptr, len(already), count, d_o.ptr, None)
        st = C.c_int(0)
        src = L.ssdr_select_status(None, C.byref(st))
        names = {ln.rsplit(" ", 4)[0] for ln in L.ssdr_prof_report().decode().splitlines() if ln.strip()}
    finally:
        L.ssdr_prof_enable(0)
    out = d_o.to_host()
    assert out[-1] == SENTINEL and (count > 0 or out[0] == SENTINEL), "the call wrote outside its %d outputs" % count
    return rc, out[:count], src, st.value, {nm for nm in names if nm.startswith("fps_")}
