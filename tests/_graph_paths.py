"""Helpers of tests/test_graph_paths.py and tests/_graph_forms_worker.py: the constants of the selection graph read from the sources, the directed float64
oracle of the chamfer matrix, a NumPy restatement of which branch of csrc/select_chamfer.hip every (source, target) pair of a cloud takes (`plan`: the cases
assert their input conditions with it BEFORE the library is called), the shapes the cases are made of, and the callers of ssdr_cloud_graph_dev /
ssdr_cloud_graph_batch_dev / ssdr_propagate_dev / ssdr_propagate_batch_dev, which return the DIRECTED matrix.  Nothing here touches a device except the
callers.

A cloud is (xyz float32 [N, 3], off int32 [S + 1], pts int32 [N]): superpoint s holds the points xyz[pts[off[s]:off[s + 1]]], in that order (the order
matters: the screening works on runs of four consecutive target points, the large-target walk on chunks of CH_TILE)."""
import os
import re
from types import SimpleNamespace

import numpy as np

from oracle import select_np as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ssdr-al_amd", "csrc")
EMPTY_ROOT = np.sqrt(1.0e300)                    # a non-empty source against an EMPTY target: the root of the float64 kernels' sentinel
EMPTY_ROOT_F32 = np.sqrt(np.float32(3.402823466e+38))      # ... and of the float32 flavour's
PASS_MARGIN = 0.25                               # chamfer_big_targets: R1 = (the workgroup's largest |a|) + 0.25 m


# ---- constants, from the sources ----------------------------------------------------------------------------------------------------------------
def _const(text, name, path):
    m = re.findall(r"constexpr\s+(?:int|float)\s+%s\s*=\s*([0-9.]+)f?\s*;" % name, text)
    assert len(m) == 1, "%s: expected one definition of %s, found %d" % (path, name, len(m))
    return float(m[0]) if "." in m[0] else int(m[0])


_CONSTANTS = None


def constants():
    """CH_TILE, PACK_MAX, ITEM, SEQ_MAX, MF_R2_MAX (select_chamfer.hpp), TOPK_ROW (select.hip), C32_SLAB (select_chamfer.hip): a changed constant moves
    the shapes of the cases with it, a definition the pattern no longer finds fails here"""
    global _CONSTANTS
    if _CONSTANTS is None:
        out = {}
        for fname, names in (("select_chamfer.hpp", ("CH_TILE", "PACK_MAX", "ITEM", "SEQ_MAX", "MF_R2_MAX")), ("select.hip", ("TOPK_ROW",)),
                             ("select_chamfer.hip", ("C32_SLAB",))):
            path = os.path.join(CSRC, fname)
            with open(path) as f:
                text = f.read()
            for nm in names:
                out[nm] = _const(text, nm, path)
        _CONSTANTS = SimpleNamespace(**out)
    return _CONSTANTS


# ---- shapes (float64 [n, 3] around a seat) and clouds ----------------------------------------------------------------------------------------------
def blob(rng, n, seat, sigma=0.08):
    return np.asarray(seat, np.float64) + rng.normal(0, sigma, (n, 3)) * np.array([1.0, 1.0, 0.5])


def _pinned(seat, p, pins):
    """the first rows of p replaced by the extreme points `pins`: the bounding box (hence its centre, the seat) does not depend on the random rest"""
    p[:len(pins)] = pins
    return np.asarray(seat, np.float64) + p


def ring(rng, n, seat, radius, thick=0.02):
    """n points on a flat ring around the seat, none outside `radius`, four pinned on the axes: the box centre is the ring's centre"""
    t = rng.random(n) * 2 * np.pi
    r = radius * (1.0 - thick * rng.random(n))
    p = np.stack([r * np.cos(t), r * np.sin(t), np.zeros(n)], 1)
    return _pinned(seat, p, [(radius, 0, 0), (-radius, 0, 0), (0, radius, 0), (0, -radius, 0)])


def slab(rng, n, seat, lx, ly):
    """a floor of lx x ly: a jittered grid in shuffled order (no hole wider than a cell and its jitter), the rest random, two opposite corners pinned"""
    nx = int(np.sqrt(n * lx / ly)); ny = n // nx
    gx, gy = np.meshgrid((np.arange(nx) + 0.5) / nx - 0.5, (np.arange(ny) + 0.5) / ny - 0.5, indexing="ij")
    g = np.stack([gx.ravel(), gy.ravel()], 1) + rng.uniform(-0.2, 0.2, (nx * ny, 2)) / np.array([nx, ny])
    g = np.concatenate([g, rng.random((n - nx * ny, 2)) - 0.5])[rng.permutation(n)]
    p = np.concatenate([g * np.array([lx, ly]), np.zeros((n, 1))], 1)
    return _pinned(seat, p, [(lx / 2, ly / 2, 0), (-lx / 2, -ly / 2, 0)])


def pole(rng, n, seat, length, axis=0):
    """n >= 2 points along one axis, both tips pinned"""
    p = np.zeros((n, 3)); p[:, axis] = (rng.random(n) - 0.5) * length
    tip = np.zeros(3); tip[axis] = length / 2
    return _pinned(seat, p, [tip, -tip])


def lattice(rng, n, seat, step=0.25, half=4):
    """n points of a small cubic lattice (repeats included), the seat moved onto the lattice so that every coordinate is exact in float32: the centred
    points are multiples of step / 2 and many distances are exactly equal"""
    return np.round(np.asarray(seat, np.float64) / step) * step + rng.integers(-half, half + 1, (n, 3)) * step


def ring_with_core(rng, n, seat, radius, ncore, first, sigma=0.03):
    """a ring of n - ncore points with a blob of ncore points at its centre, the core listed behind the first `first` ring points: the first chunk of
    the large-target walk holds no core point"""
    assert first + ncore <= n
    r = ring(rng, n - ncore, (0, 0, 0), radius)
    core = rng.normal(0, sigma, (ncore, 3)) * np.array([1.0, 1.0, 0.0])
    return np.asarray(seat, np.float64) + np.concatenate([r[:first], core, r[first:]])


def twice(p):
    """every point of p twice, the copy half the list away and (for more than four points) in another run of four"""
    return np.concatenate([p, p])


def make_cloud(rng, shapes, permute=True):
    """shapes: the superpoints' points in list order (an empty array: an empty superpoint) -> (xyz, off, pts)"""
    sizes = [len(s) for s in shapes]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(off[-1])
    flat = np.concatenate([np.asarray(s, np.float64).reshape(-1, 3) for s in shapes] + [np.zeros((0, 3))]).astype(np.float32)
    pts = (rng.permutation(n) if permute else np.arange(n)).astype(np.int32)
    xyz = np.empty((n, 3), np.float32)
    xyz[pts] = flat
    return xyz, off, pts


def sub_csr(off, pts, sel):
    """the CSR pair of the superpoints `sel`, in that order"""
    sel = np.asarray(sel)
    so = np.concatenate([[0], np.cumsum(off[sel + 1] - off[sel])]).astype(np.int32)
    sp = np.concatenate([pts[off[s]:off[s + 1]] for s in sel] + [np.zeros(0, np.int32)]).astype(np.int32)
    return so, sp


def bbox_centres(xyz, off, pts):
    """select_np.bbox_centres; an empty superpoint (which the reference never makes) sits at 0, as FLT_MAX + -FLT_MAX leaves it in the library"""
    live = np.flatnonzero(np.diff(off) > 0)
    c = np.zeros((len(off) - 1, 3))
    if len(live):
        so, sp = sub_csr(off, pts, live)
        c[live] = O.bbox_centres(xyz, so, sp)
    return c


def centred(xyz, off, pts, centres):
    return [xyz[pts[off[s]:off[s + 1]]].astype(np.float64) - centres[s] for s in range(len(off) - 1)]


# ---- the directed oracle --------------------------------------------------------------------------------------------------------------------------
def dir_oracle(xyz, off, pts, centres):
    """-> (dir float64 [S, S], nn): dir[i, j] = mean over the points a of i of min over the points b of j of |(a - c_i) - (b - c_j)|, the three squares
    added in the order of select_np.create_cd, 0 on the diagonal; nn[i, j] = per point of i the index (in j's list order) of its nearest point of j.
    An empty superpoint: its row is 0; its column holds EMPTY_ROOT, what the library writes today (the sentinel's root: nothing can be nearest)."""
    S = len(off) - 1
    al = centred(xyz, off, pts, centres)
    size = np.diff(off)
    A = np.concatenate(al + [np.zeros((0, 3))])
    dirm = np.zeros((S, S)); nn = {}
    for j in range(S):
        if size[j] == 0:
            dirm[size > 0, j] = EMPTY_ROOT
            dirm[j, j] = 0.0
            continue
        best = np.empty(len(A)); arg = np.empty(len(A), np.int64)
        step = max(1, 1500000 // int(size[j]))
        for r in range(0, len(A), step):
            d = A[r:r + step, None, :] - al[j][None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            arg[r:r + step] = d2.argmin(1)
            best[r:r + step] = np.sqrt(d2.min(1))
        for i in range(S):
            if i != j and size[i]:
                dirm[i, j] = np.mean(best[off[i]:off[i + 1]])
                nn[i, j] = arg[off[i]:off[i + 1]]
    return dirm, nn


def dir_oracle_f32(xyz, off, pts, centres):
    """select_np.create_cd_cuda, directed: the centred points rounded to float32, squared float32 distances with dx = b - a, root and mean in float32,
    widened.  Empty superpoints as the library has them: a zero row, the root of FLT_MAX in the column."""
    S = len(off) - 1
    al = [a.astype(np.float32) for a in centred(xyz, off, pts, centres)]
    dirm = np.zeros((S, S), np.float32)
    for i in range(S):
        for j in range(S):
            if i == j or not len(al[i]):
                continue
            if not len(al[j]):
                dirm[i, j] = EMPTY_ROOT_F32
                continue
            d = al[j][None, :, :] - al[i][:, None, :]
            dist = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            dirm[i, j] = np.mean(np.sqrt(dist.min(1)), dtype=np.float32)
    return dirm.astype(np.float64)


# ---- which branch a pair takes ----------------------------------------------------------------------------------------------------------------------
def plan(sizes, al):
    """sizes, centred points (centred()) of the superpoints of ONE call's cloud, in `sel` order -> the branches of csrc/select.hip: chamfer_plan_body /
    chamfer_fill_body and csrc/select_chamfer.hip: chamfer_dir_body / chamfer_big_targets, restated:
      start / item_of / items / big   the packer: an empty superpoint or one above ITEM points goes pair by pair (item_of -1), all of them when the cloud
                                      has more than PACK_MAX; the others fill 256-slot items, the first of the last FOUR opened items with room
      radius, r2sp, r2item            max |p| (float64); max |p|^2 * 1.000001 as float32 per superpoint / per item
      branch(i, j)                    "diag" | "big" (target above CH_TILE: chamfer_big_targets) | "mf" (screened on the matrix cores) | "stream" (the screening
                                      build's float64 loop over the target in global memory: item or target beyond MF_R2_MAX) — the screening build's view;
                                      SSDR_CHAMFER_F64=1 takes the staged float64 screening wherever this says "mf" or "stream"
      chunks(j)                       steps of CH_TILE points of a large target
    and the two-pass walk's conditions, which depend on the radii alone and not on which items share a workgroup (Rs: the largest radius over the
    superpoints of at most ITEM points; Rb(j): over the larger ones but j):
      pass0_surely_empty(j)           every |b| > R + 0.25 (R = Rs for the item sources, Rb(j) with large=True)
      surely_settled(i, j, nn)        a target point within 0.2 m of the origin (where padding slots sit, see prime_pack) and of every point of i
      surely_unsettled(m, j, nn)      some point of the item m is farther from the target than Rs + 0.25 - (the item's largest |a|): its wave takes pass 1
      nearest_in_pass1(i, j, nn)      a target point with |b| <= 0.25 exists (pass 0 is not empty) and some point of i has its nearest with |b| > R + 0.25
      surely_swept(j)                 every target point is listed twice, the copies in different runs of four: the two runs tie exactly"""
    K = constants()
    sizes = [int(s) for s in sizes]
    n = len(sizes)
    norm = [np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]) if len(a) else np.zeros(0) for a in al]
    radius = np.array([r.max() if len(r) else 0.0 for r in norm])
    r2sp = np.array([np.float32(((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]).max() * 1.000001) if len(a) else np.float32(0) for a in al], np.float32)
    start = np.full(n, -1, np.int64)
    if n <= K.PACK_MAX:
        base, used, items = [0, 0, 0, 0], [K.ITEM] * 4, 0
        for i, ni in enumerate(sizes):
            if ni == 0 or ni > K.ITEM:
                continue
            j = next((k for k in range(4) if used[k] + ni <= K.ITEM), -1)
            if j < 0:
                base, used = base[1:] + [items * K.ITEM], used[1:] + [0]
                items += 1
                j = 3
            start[i] = base[j] + used[j]
            used[j] += ni
    item_of = np.where(start >= 0, start // K.ITEM, -1)
    nitems = int(item_of.max()) + 1 if n else 0
    items = [[i for i in range(n) if item_of[i] == it] for it in range(nitems)]
    r2item = np.array([max(r2sp[i] for i in m) for m in items], np.float32)
    small = [i for i in range(n) if 0 < sizes[i] <= K.ITEM]
    P = SimpleNamespace(n=n, sizes=sizes, radius=radius, r2sp=r2sp, start=start, item_of=item_of, items=items, r2item=r2item, norm=norm,
                        big=[i for i in range(n) if start[i] < 0], Rs=max([radius[i] for i in small] + [0.0]))
    P.Rb = lambda j: max([radius[i] for i in range(n) if sizes[i] > K.ITEM and i != j] + [0.0])
    P.chunks = lambda j: -(-sizes[j] // K.CH_TILE)

    def branch(i, j):
        if i == j:
            return "diag"
        if sizes[j] > K.CH_TILE:
            return "big"
        r2src = r2item[item_of[i]] if item_of[i] >= 0 else r2sp[i]
        return "mf" if r2sp[j] <= K.MF_R2_MAX and r2src <= K.MF_R2_MAX else "stream"
    P.branch = branch
    outer = lambda j, large: (1.0 + 1e-9) * ((P.Rb(j) if large else P.Rs) + PASS_MARGIN)
    P.pass0_surely_empty = lambda j, large=False: sizes[j] > K.CH_TILE and bool((norm[j] > outer(j, large)).all())

    def surely_settled(i, j, nn):
        d = al[i] - al[j][nn[i, j]]
        near = np.sqrt((d * d).sum(1))
        return sizes[j] > K.CH_TILE and norm[j].min() <= 0.2 and near.max() <= 0.2
    P.surely_settled = surely_settled

    def surely_unsettled(members, j, nn):
        """the wave of the item `members` goes on to pass 1: some point's nearest target point is farther than R1 - |a| can be (R1 <= Rs + 0.25)"""
        far = max(np.sqrt(((al[i] - al[j][nn[i, j]]) ** 2).sum(1)).max() for i in members)
        return sizes[j] > K.CH_TILE and far > (1 + 1e-9) * (P.Rs + PASS_MARGIN - max(radius[i] for i in members)) + 1e-9
    P.surely_unsettled = surely_unsettled
    P.nearest_in_pass1 = lambda i, j, nn: sizes[j] > K.CH_TILE and norm[j].min() <= PASS_MARGIN * (1 - 1e-9) and bool((norm[j][nn[i, j]] > outer(j, sizes[i] > K.ITEM)).any())

    def surely_swept(j):
        b = al[j]
        if len(b) < 2 or len(b) % 2:
            return False
        h = len(b) // 2
        twin = np.concatenate([np.arange(h, 2 * h), np.arange(h)])
        return bool((b == b[twin]).all() and (np.arange(2 * h) // 4 != twin // 4).all())
    P.surely_swept = surely_swept
    return P


# ---- callers ----------------------------------------------------------------------------------------------------------------------------------------
def set_chamfer_mode(mode):
    from ssdr_al import _lib
    _lib.check(_lib.lib().ssdr_select_set_chamfer_mode({"f64": 0, "f32_cuda": 1}[mode]))


def graph_single(cloud, sel=None, gcn_top=0):
    """ssdr_cloud_graph_dev over the superpoints `sel` (default: all) of one cloud -> (centres [n, 3], dir [n, n] DIRECTED, adj [n, n])"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    xyz, off, pts = cloud
    sel = np.arange(len(off) - 1, dtype=np.int32) if sel is None else np.ascontiguousarray(sel, np.int32)
    n = len(sel)
    d_x, d_o, d_p, d_s = DevArray.from_host(xyz), DevArray.from_host(off), DevArray.from_host(pts), DevArray.from_host(sel)
    d_c, d_d, d_a = DevArray((n, 3), np.float64), DevArray((n, n), np.float64), DevArray((n, n), np.float64)
    _lib.check(_lib.lib().ssdr_cloud_graph_dev(d_x.ptr, d_o.ptr, d_p.ptr, d_s.ptr, n, max(int((off[sel + 1] - off[sel]).max()), 1), int(gcn_top), d_c.ptr, d_d.ptr, d_a.ptr, None))
    _lib.sync()
    return d_c.to_host(), d_d.to_host(), d_a.to_host()


def batch_layout(clouds):
    """[(cloud, sel | None)] -> the concatenated arrays of ssdr_cloud_graph_batch_dev: xyz, off, pts, sel (grouped by cloud), coff, boff"""
    xyzs, offs, ptss, sels, counts = [], [np.zeros(1, np.int64)], [], [], []
    pbase = sbase = 0
    for (xyz, off, pts), sel in clouds:
        sel = np.arange(len(off) - 1) if sel is None else np.asarray(sel)
        xyzs.append(xyz); ptss.append(pts.astype(np.int64) + pbase); offs.append(off[1:].astype(np.int64) + offs[-1][-1])
        sels.append(sel + sbase); counts.append(len(sel))
        pbase += len(xyz); sbase += len(off) - 1
    counts = np.asarray(counts, np.int64)
    coff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32); boff = np.concatenate([[0], np.cumsum(counts * counts)]).astype(np.int64)
    return (np.concatenate(xyzs).astype(np.float32), np.concatenate(offs).astype(np.int32), np.concatenate(ptss).astype(np.int32),
            np.concatenate(sels).astype(np.int32), coff, boff)


def graph_batch(clouds, gcn_top=0):
    """ssdr_cloud_graph_batch_dev over [(cloud, sel | None)] in ONE call -> per cloud (centres, dir DIRECTED, adj)"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    xyz, off, pts, sel, coff, boff = batch_layout(clouds)
    N, tot = len(sel), int(boff[-1])
    d_x, d_o, d_p, d_s = DevArray.from_host(xyz), DevArray.from_host(off), DevArray.from_host(pts), DevArray.from_host(sel)
    d_coff, d_boff = DevArray.from_host(coff), DevArray.from_host(boff)
    d_c, d_d, d_a = DevArray((N, 3), np.float64), DevArray((tot,), np.float64), DevArray((tot,), np.float64)
    _lib.check(_lib.lib().ssdr_cloud_graph_batch_dev(d_x.ptr, d_o.ptr, d_p.ptr, d_s.ptr, d_coff.ptr, d_boff.ptr, len(clouds), N, int(np.diff(coff).max()), int(gcn_top),
                                                     d_c.ptr, d_d.ptr, d_a.ptr, None))
    _lib.sync()
    cen, dirm, adj = d_c.to_host(), d_d.to_host(), d_a.to_host()
    out = []
    for c in range(len(clouds)):
        n = int(coff[c + 1] - coff[c])
        out.append((cen[coff[c]:coff[c + 1]], dirm[boff[c]:boff[c + 1]].reshape(n, n), adj[boff[c]:boff[c + 1]].reshape(n, n)))
    return out


def prime_pack(n, seed=0):
    """The packer's slot tables are scratch that one call leaves to the next, and a padding slot's coordinates are whatever the buffer held: they cannot change
    a value (padding is never summed) but they enter the large-target walk's R1.  A call over n superpoints of exactly ITEM points within 1 cm — the tables
    are laid out by the superpoint count — leaves every slot a later call over n superpoints can reach within 1 cm of the origin, so that the walk's passes
    follow from the case's own radii on either build."""
    K = constants()
    rng = np.random.default_rng(seed)
    graph_single(make_cloud(rng, [rng.uniform(-0.005, 0.005, (K.ITEM, 3)) for _ in range(n)], permute=False))


def propagate_hops(adjs, rows, V, gcn_number, batched):
    """comb = sum_{h = 0 .. gcn_number} A^h V over the table V [T, D] (float64), cloud c owning the table rows rows[c] with the block adjs[c]: hop by hop
    through ssdr_propagate_dev (a call per cloud) or ssdr_propagate_batch_dev (one call per hop) -> (comb, the last hop's table)"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    L = _lib.lib()
    T, D = V.shape
    counts = np.array([len(r) for r in rows], np.int64)
    coff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32); boff = np.concatenate([[0], np.cumsum(counts * counts)]).astype(np.int64)
    d_adj = DevArray.from_host(np.concatenate([np.asarray(a, np.float64).ravel() for a in adjs]))
    d_rows = DevArray.from_host(np.concatenate(rows).astype(np.int32))
    d_coff, d_boff = DevArray.from_host(coff), DevArray.from_host(boff)
    d_comb = DevArray.from_host(V)
    fill = np.full((T, D), -7.5)                       # rows outside the clouds must come back as they went in
    tabs = [DevArray.from_host(V), DevArray.from_host(fill), DevArray.from_host(fill)]
    src = tabs[0]
    for hop in range(gcn_number):
        dst = tabs[1 + (hop & 1)]
        if batched:
            _lib.check(L.ssdr_propagate_batch_dev(d_adj.ptr, d_coff.ptr, d_boff.ptr, len(rows), int(counts.max()), d_rows.ptr, src.ptr, D, dst.ptr, d_comb.ptr, None))
        else:
            for c in range(len(rows)):
                _lib.check(L.ssdr_propagate_dev(d_adj.ptr + 8 * int(boff[c]), int(counts[c]), d_rows.ptr + 4 * int(coff[c]), src.ptr, D, dst.ptr, d_comb.ptr, None))
        src = dst
    _lib.sync()
    return d_comb.to_host(), src.to_host()


# ---- inputs shared by the cases and the worker --------------------------------------------------------------------------------------------------------
def small_sources(rng, seat0=(3.0, 2.0, 1.0), flat=1.0):
    """sources of 1 to 256 points with radii from 0.02 to 0.5 m, and two above ITEM points (flat: their extent along z, as a fraction)"""
    K = constants()
    spec = [(1, 0.02), (3, 0.02), (K.SEQ_MAX, 0.05), (K.SEQ_MAX + 1, 0.05), (40, 0.1), (100, 0.2), (K.ITEM - 1, 0.1), (K.ITEM, 0.02), (70, 0.5), (K.ITEM + 44, 0.3), (2 * K.ITEM + 8, 0.45)]
    out = []
    for k, (n, rad) in enumerate(spec):
        p = rng.uniform(-1, 1, (n, 3)) * rad / np.sqrt(3.0) * np.array([1.0, 1.0, flat])
        out.append(np.asarray(seat0) + np.array([1.5 * k, 0.7 * k, 0.0]) + p)
    return out


def batch_clouds():
    """the five clouds of test_batch_equals_single_and_oracle / test_slices_switch -> [(cloud, sel | None)]"""
    K = constants()
    rng = np.random.default_rng(505)
    e = np.zeros((0, 3))
    first = [ring(rng, K.CH_TILE + 1, (5, 5, 1), 2.5), e] + small_sources(rng)[:6] + [slab(rng, K.CH_TILE + 60, (12, 3, 0), 3.0, 2.0), e, blob(rng, 300, (1, 8, 1), 0.1),
                                                                                       ring(rng, 2 * K.CH_TILE + 1, (20, 5, 1), 2.5), blob(rng, 9, (2, 2, 2)),
                                                                                       pole(rng, 5, (30, 40, 1), 70.0, axis=1)]      # the last one takes item 0 of this cloud beyond MF_R2_MAX
    a = make_cloud(rng, first)
    one = make_cloud(rng, [blob(rng, 37, (1, 1, 1))])
    two = make_cloud(rng, [blob(rng, 5, (1, 1, 1)), blob(rng, 300, (3, 1, 1), 0.2)])
    sizes = [int(s) for s in rng.integers(1, 120, 74)]
    sizes[:8] = [1, 2, K.SEQ_MAX, K.SEQ_MAX + 1, K.ITEM, K.ITEM + 1, 33, 64]
    many = make_cloud(rng, [blob(rng, s, rng.random(3) * np.array([8, 6, 2.5])) for s in sizes])
    again = np.array([12, 3, 0, 9, 11, 7, 10, 5])
    return [(a, None), (one, None), (two, None), (many, None), (a, again)]
