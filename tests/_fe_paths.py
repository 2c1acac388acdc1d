"""Helpers of tests/test_subsample_paths.py and tests/_fe_forms_worker.py: one general call of ssdr_grid_subsample_batch_dev (any row layout, NULL
features / classes, the caller's stream), a float32 NumPy restatement of the bucket geometry of csrc/frontend.hip (fe_params, fe_voxel, fe_bucket, fe_vid
and the greedy slicer of fe_reduce) that the cases assert their input conditions with, and the inputs both files share.  Nothing here touches a device
except run_batch / run_single."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

FE_NBMAX, FE_CAP, FE_SLICES, FE_CH, LAB_CAP = 16384, 1024, 62, 32768, 29      # csrc/frontend.hip, csrc/voxel_label.hpp
AUTO, SORT = 0, 1                                                              # SSDR_SUBSAMPLE_AUTO / SSDR_SUBSAMPLE_SORT
F32 = np.float32


# ---- the call -------------------------------------------------------------------------------------------------------------------------------
def run_batch(clouds, dl, method, stream=None):
    """clouds: [(points, features | None, classes | None)], the same layout in every cloud; fdim == 0 / ldim == 0 go in as NULL pointers.
    -> (return code of ssdr_grid_subsample_status, status word, [per cloud: the tuple of present arrays cut to the cloud's row count m])"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    L = _lib.lib()
    sizes = [len(c[0]) for c in clouds]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    has_f, has_l = clouds[0][1] is not None, clouds[0][2] is not None
    assert all((c[1] is not None) == has_f and (c[2] is not None) == has_l for c in clouds)
    P = np.ascontiguousarray(np.concatenate([c[0] for c in clouds]), F32)
    Fe = np.ascontiguousarray(np.concatenate([c[1] for c in clouds]), F32) if has_f else None
    Lb = np.ascontiguousarray(np.concatenate([c[2] for c in clouds]), np.int32) if has_l else None
    fdim, ldim = (Fe.shape[1] if has_f else 0), (Lb.shape[1] if has_l else 0)
    d_p = DevArray.from_host(P, stream=stream)
    d_f = DevArray.from_host(Fe, stream=stream) if has_f else None
    d_l = DevArray.from_host(Lb, stream=stream) if has_l else None
    o_p = DevArray(P.shape, F32)
    o_f = DevArray(Fe.shape, F32) if has_f else None
    o_l = DevArray(Lb.shape, np.int32) if has_l else None
    d_m = DevArray((len(sizes),), np.int64)
    dp = lambda d: None if d is None else d.ptr
    _lib.check(L.ssdr_grid_subsample_set_method(method))
    try:
        _lib.check(L.ssdr_grid_subsample_batch_dev(d_p.ptr, dp(d_f), fdim, dp(d_l), ldim, _lib.ptr(off), len(sizes), float(dl), o_p.ptr, dp(o_f), dp(o_l), d_m.ptr, stream))
        st = C.c_int32()
        rc = L.ssdr_grid_subsample_status(stream, C.byref(st))
    finally:
        _lib.check(L.ssdr_grid_subsample_set_method(AUTO))
    m = d_m.to_host(stream=stream)
    outs = [o.to_host(stream=stream) for o in (o_p, o_f, o_l) if o is not None]
    rows = []
    for r in range(len(sizes)):
        assert 0 <= m[r] <= sizes[r], "cloud %d: row count %d of %d points" % (r, m[r], sizes[r])
        rows.append(tuple(o[int(off[r]):int(off[r]) + int(m[r])] for o in outs))
    return rc, st.value, rows


def run_single(cloud, dl, order):
    """ssdr_grid_subsample_dev of one cloud (the (key, value) sort: any grid) -> (status return code, status word, the present arrays cut to m)"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    L = _lib.lib()
    p, f, l = cloud
    n = len(p)
    d_p, o_p = DevArray.from_host(np.ascontiguousarray(p, F32)), DevArray((n, 3), F32)
    d_f = DevArray.from_host(np.ascontiguousarray(f, F32)) if f is not None else None
    d_l = DevArray.from_host(np.ascontiguousarray(l, np.int32)) if l is not None else None
    o_f = DevArray(f.shape, F32) if f is not None else None
    o_l = DevArray(l.shape, np.int32) if l is not None else None
    d_m = DevArray((1,), np.int64)
    dp = lambda d: None if d is None else d.ptr
    _lib.check(L.ssdr_grid_subsample_dev(d_p.ptr, n, dp(d_f), f.shape[1] if f is not None else 0, dp(d_l), l.shape[1] if l is not None else 0, float(dl),
                                         {"reference": 0, "key": 1}[order], o_p.ptr, dp(o_f), dp(o_l), d_m.ptr, None))
    st = C.c_int32()
    rc = L.ssdr_grid_subsample_status(None, C.byref(st))
    m = int(d_m.to_host()[0])
    assert 0 <= m <= n
    return rc, st.value, tuple(o.to_host()[:m] for o in (o_p, o_f, o_l) if o is not None)


def oracle_rows(orc, cloud, dl):
    return orc.grid_subsampling(cloud[0], cloud[1], cloud[2], dl, order="key")


def rows_equal(got, exp):
    """bit for bit, the row count included"""
    if len(got) != len(exp):
        return False
    for a, b in zip(got, exp):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            return False
    return True


# ---- the geometry of frontend.hip in float32 NumPy ---------------------------------------------------------------------------------------
def geometry(points, dl):
    """fe_params and fe_voxel of one cloud (header comment of frontend.hip; every operation in float32, no contraction):
    origin = floor(min / dl) * dl with min / dl taken as min * (1 / dl); n = floor((max - origin) / dl) + 1 per axis; a bucket is 2^sx x 8 x 8 voxels, sx = 3, or 4
    when that leaves more than 16384 buckets; fits = what the partition path takes (nx < 65536, the minimum in voxel 0, at most 16384 buckets).  min / max skip NaNs
    (fminf / fmaxf).  Per point: inside (its voxel lies in the grid), bucket, vid (voxel inside the bucket: x fastest, then y, z), key (ix + nx (iy + ny iz));
    per bucket: records; per occupied voxel: members (`vox_key`, `vox_members`, ascending key)."""
    p = np.ascontiguousarray(points, F32)
    dl = F32(dl)
    with np.errstate(invalid="ignore"):
        mn, mx = np.fmin.reduce(p, axis=0), np.fmax.reduce(p, axis=0)
        inv = F32(1) / dl
        org = (np.floor(mn * inv) * dl).astype(F32)
        nd = np.floor((mx - org) / dl) + F32(1)
        min_vox = np.floor((mn - org) / dl)
        fits = bool((nd >= 1).all() and nd[0] < 65536 and nd[1] < 1.0e6 and nd[2] < 1.0e6 and (min_vox >= 0).all())
        g = SimpleNamespace(org=org, dl=dl, min_vox=min_vox, nx=int(nd[0]), ny=int(nd[1]), nz=int(nd[2]), sx=3, nb=0, fits=fits)
        if fits:
            nby, nbz = (g.ny + 7) >> 3, (g.nz + 7) >> 3
            nbx = (g.nx + 7) >> 3
            if nbx * nby * nbz > FE_NBMAX:
                g.sx, nbx = 4, (g.nx + 15) >> 4
            if nbx * nby * nbz > FE_NBMAX:
                g.fits = False
            else:
                g.nbx, g.nby, g.nbz, g.nb = nbx, nby, nbz, nbx * nby * nbz
        if not g.fits:
            return g
        fl = np.floor((p - org) / dl)
        g.inside = ((fl >= 0) & (fl < np.array([g.nx, g.ny, g.nz], F32))).all(axis=1)          # False for a NaN
        iv = np.where(g.inside[:, None], fl, 0).astype(np.int64)
    ix, iy, iz = iv[:, 0], iv[:, 1], iv[:, 2]
    g.ijk = iv
    g.bucket = np.where(g.inside, (ix >> g.sx) + g.nbx * ((iy >> 3) + g.nby * (iz >> 3)), -1)
    g.vid = (ix & ((1 << g.sx) - 1)) | (((iy & 7) | ((iz & 7) << 3)) << g.sx)
    g.key = np.where(g.inside, ix + g.nx * (iy + g.ny * iz), -1)
    g.records = np.bincount(g.bucket[g.inside], minlength=g.nb)
    g.vox_key, g.vox_members = np.unique(g.key[g.inside], return_counts=True)
    return g


def bucket_hist(g, b):
    """members of every voxel of bucket b, by voxel id inside the bucket (64 << sx entries)"""
    return np.bincount(g.vid[g.bucket == b], minlength=64 << g.sx)


def slices(hist):
    """the greedy rule of fe_reduce for a bucket of more than FE_CAP records: consecutive voxels while their records stay within FE_CAP, at most FE_SLICES
    slices -> (slice bounds in voxel ids, whether the bucket is taken: no voxel above FE_CAP and no more than FE_SLICES slices)"""
    V = len(hist)
    cs = np.concatenate([[0], np.cumsum(hist)])
    bounds, v = [0], 0
    while v < V and len(bounds) - 1 < FE_SLICES:
        w = v
        while w < V and cs[w + 1] - cs[v] <= FE_CAP:
            w += 1
        if w == v:
            return bounds, False
        v = w
        bounds.append(v)
    return bounds, v >= V


def slices_needed(hist):
    """slices the greedy rule would cut with no limit on their number (None: a voxel above FE_CAP)"""
    cs = np.concatenate([[0], np.cumsum(hist)])
    k, v, V = 0, 0, len(hist)
    while v < V:
        w = v
        while w < V and cs[w + 1] - cs[v] <= FE_CAP:
            w += 1
        if w == v:
            return None
        v, k = w, k + 1
    return k


def max_distinct_labels(g, labels):
    """largest number of distinct labels one voxel holds in one column"""
    best = 0
    for col in range(labels.shape[1]):
        pairs = np.unique(np.stack([g.key[g.inside], labels[g.inside, col].astype(np.int64)], axis=1), axis=0)
        best = max(best, int(np.bincount(np.unique(pairs[:, 0], return_inverse=True)[1]).max()))
    return best


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def make_cloud(rng, n, box, shift=0.0, fdim=3, ldim=1, lab=(0, 13)):
    p = (rng.random((n, 3), dtype=F32) * np.asarray(box, F32) + np.asarray(shift, F32)).astype(F32)
    return attach(rng, p, fdim, ldim, lab)


def attach(rng, p, fdim=3, ldim=1, lab=(0, 13)):
    """features from normal(0, 50), labels from [lab[0], lab[1]); a width of 0 gives None"""
    n = len(p)
    f = rng.normal(0, 50, (n, fdim)).astype(F32) if fdim else None
    l = rng.integers(lab[0], lab[1], (n, ldim)).astype(np.int32) if ldim else None
    return p, f, l


def wrapping_labels(rng, n, ldim=1):
    """labels in [0,13) for the n >= 300 members of one crowded voxel whose vote the packed byte counters get wrong: per column one label on exactly 260 members
    (its byte shows 4), the other twelve labels share the rest in input order at random"""
    out = np.empty((n, ldim), np.int64)
    for col in range(ldim):
        top = int(rng.integers(0, 13))
        rest = np.array([x for x in range(13) if x != top])
        out[:, col] = rest[rng.integers(0, 12, n)]
        out[rng.permutation(n)[:260], col] = top
    return out


def byte_counter_wraps(labels):
    """input condition on one voxel's labels (one column): the winning label has 256 .. 511 members and what its byte counter shows is below another label's count"""
    cnt = np.sort(np.bincount(labels, minlength=13))
    return len(cnt) == 13 and 256 <= cnt[-1] < 512 and cnt[-1] - 256 < cnt[-2] < 256


def ordinary(rng):
    """the 500-point cloud that shares a call with an edge cloud"""
    return make_cloud(rng, 500, (1.0, 1.0, 1.0))


def layout_clouds(fdim, ldim, seed=None):
    """case 1: about 5000 points in a 2 x 1.5 x 1 box and 700 points at negative coordinates, dl = 0.08"""
    rng = np.random.default_rng(1000 + 10 * fdim + ldim if seed is None else seed)
    clouds = [make_cloud(rng, 5003, (2.0, 1.5, 1.0), 0.0, fdim, ldim), make_cloud(rng, 700, (1.0, 0.8, 0.5), (-3.0, -2.0, -1.5), fdim, ldim)]
    dl = 0.08
    for p, _, _ in clouds:
        g = geometry(p, dl)
        assert g.fits and g.inside.all() and np.count_nonzero(g.records) > 1
    assert (clouds[1][0] < 0).all()
    return clouds, dl


def outside_fast_vote_clouds(fdim, ldim, lab):
    """case 2: slabs one voxel thick (a bucket then holds at most 64 occupied voxels: one pass), a mean of at least 4 members per voxel, labels from `lab`"""
    rng = np.random.default_rng(2000 + 100 * fdim + 10 * ldim + lab[1])
    clouds = [make_cloud(rng, 3000, (2.0, 1.5, 0.05), 0.0, fdim, ldim, lab), make_cloud(rng, 1200, (1.0, 1.0, 0.05), (-3.0, -2.0, -1.5), fdim, ldim, lab)]
    dl = 0.08
    for p, _, l in clouds:
        g = geometry(p, dl)
        assert g.fits and g.inside.all()
        assert len(p) / len(g.vox_key) >= 4.0, "mean members per voxel %.2f" % (len(p) / len(g.vox_key))
        assert g.records.max() <= FE_CAP, "a bucket of %d records is not reduced in one pass" % g.records.max()
        assert max_distinct_labels(g, l) <= LAB_CAP
        assert ((l < 0) | (l >= 13)).any()
    return clouds, dl


def crowded_one_pass_clouds(lab):
    """case 3a: 900 points in one voxel (the byte counters of the fast vote wrap at 256), its bucket still read in one pass; a second ordinary cloud"""
    rng = np.random.default_rng(3000 + lab[1])
    clouds = [make_cloud(rng, 900, (0.01, 0.01, 0.01), 0.5, lab=lab), make_cloud(rng, 1500, (1.0, 1.0, 1.0), lab=lab)]
    dl = 0.04
    if lab == (0, 13):          # a uniform draw leaves every label near 70 members: no byte counter would wrap
        clouds[0] = (clouds[0][0], clouds[0][1], wrapping_labels(rng, 900).astype(np.int32))
        assert byte_counter_wraps(clouds[0][2][:, 0])
    g = geometry(clouds[0][0], dl)
    assert g.fits and g.inside.all() and len(g.vox_key) == 1 and 256 <= g.vox_members[0] <= FE_CAP
    assert g.records.max() <= FE_CAP
    assert max_distinct_labels(g, clouds[0][2]) <= LAB_CAP
    return clouds, dl


CROWDED_VOXELS = [(1, 1, 0), (5, 3, 1), (2, 6, 2), (7, 0, 4), (3, 4, 5), (6, 7, 7)]


def crowded_sliced_cloud(rng, lab, corner=(0.0, 0.0, 0.0), dl=0.04, crowd=600, spread=2000):
    """one 8 x 8 x 8 bucket at `corner` (a multiple of 8 dl): six voxels of `crowd` points each, `spread` points over the whole bucket, input order shuffled.
    Labels from `lab`; with [0,13) the crowded voxels' labels are drawn so that a byte counter of the fast vote wraps (wrapping_labels)."""
    dl32 = float(F32(dl))
    parts = [rng.random((spread, 3)) * (8 * dl32 * 0.999)]
    labs = [rng.integers(lab[0], lab[1], (spread, 1))]
    for v in CROWDED_VOXELS:
        parts.append((np.asarray(v) + 0.25 + 0.5 * rng.random((crowd, 3))) * dl32)
        labs.append(wrapping_labels(rng, crowd) if lab == (0, 13) else rng.integers(lab[0], lab[1], (crowd, 1)))
    p, l = np.concatenate(parts), np.concatenate(labs)
    p[0] = 0.0                                                  # the bucket's corner is the cloud's minimum
    perm = rng.permutation(len(p))
    p = (p[perm] + np.asarray(corner)).astype(F32)
    return p, rng.normal(0, 50, (len(p), 3)).astype(F32), l[perm].astype(np.int32)


def check_sliced_bucket(g, b):
    """preconditions of case 3b on bucket b -> (slice bounds, crowded voxels by slice)"""
    hist = bucket_hist(g, b)
    assert hist.sum() > FE_CAP and hist.max() <= FE_CAP
    bounds, taken = slices(hist)
    assert taken
    filled = [s for s in range(len(bounds) - 1) if hist[bounds[s]:bounds[s + 1]].sum() > 0]
    assert len(filled) >= 2
    late = [s for s in filled[1:] if (hist[bounds[s]:bounds[s + 1]] > 255).any()]
    assert late, "no voxel above 255 members in a slice after the first"
    return bounds, late


def crowded_sliced_clouds(lab):
    """case 3b"""
    rng = np.random.default_rng(3500 + lab[1])
    clouds = [crowded_sliced_cloud(rng, lab)]
    dl = 0.04
    g = geometry(clouds[0][0], dl)
    assert g.fits and g.inside.all() and g.nb == 1 and (g.nx, g.ny, g.nz) == (8, 8, 8)
    bounds, late = check_sliced_bucket(g, 0)
    assert max_distinct_labels(g, clouds[0][2]) <= LAB_CAP
    if lab == (0, 13):          # a voxel whose byte counter wraps, in a slice after the first
        crowded = [v for v in np.flatnonzero(bucket_hist(g, 0) > 255) if v >= bounds[1]]
        assert crowded and all(byte_counter_wraps(clouds[0][2][g.vid == v, 0]) for v in crowded)
    return clouds, dl


def slice_limit_cloud(n, seed=4000):
    """case 4: one bucket of 512 voxels, n points spread uniformly -> (cloud, slices the greedy rule needs)"""
    rng = np.random.default_rng(seed + n)
    dl = 0.04
    p = rng.random((n, 3)) * (8 * float(F32(dl)) * 0.999)
    p[0] = 0.0
    cloud = attach(rng, p.astype(F32))
    g = geometry(cloud[0], dl)
    assert g.fits and g.inside.all() and g.nb == 1 and len(g.vox_key) == 512 and g.vox_members.max() <= FE_CAP
    return cloud, slices_needed(bucket_hist(g, 0)), dl


def many_items_clouds(crowded0, n1=60000, workgroups=2560):
    """case 7, SSDR_FE_WGS=1 SSDR_FE_MOVE_WGS=1: more non-empty buckets than ten times the workgroups (one per CU: 256 on the MI355X, the figure the library
    assumes where it cannot ask), so every workgroup takes item after item.  Cloud 0: a few buckets, with crowded0 one voxel of 1100 points in them (status 4).
    Cloud 1: n1 points in a 6 x 5 x 3 box; five buckets hold a voxel of 600 points (one pass, exact vote), three hold two such voxels (sliced); the crowded
    voxels' labels come from [-3, 20) and, in turn, from [0,13) with a byte counter of the fast vote wrapping."""
    rng = np.random.default_rng(7000)
    dl, dl32 = 0.04, float(F32(0.04))
    p0 = rng.random((900, 3)) * np.array([0.9, 0.6, 0.3])
    l0 = rng.integers(0, 13, (900, 1))
    if crowded0:
        p0 = np.concatenate([p0, (np.array([9, 3, 2]) + 0.25 + 0.5 * rng.random((1100, 3))) * dl32])
        l0 = np.concatenate([l0, rng.integers(0, 13, (1100, 1))])
    p0[0] = 0.0
    c0 = (p0.astype(F32), rng.normal(0, 50, (len(p0), 3)).astype(F32), l0.astype(np.int32))
    p1 = [rng.random((n1, 3)) * np.array([6.0, 5.0, 3.0])]
    l1 = [rng.integers(0, 13, (n1, 1))]
    crowded = [((17 + 11 * k, 9 + 13 * k, 5 + 7 * k), 1) for k in range(5)] + [((40 + 24 * k, 20 + 16 * k, 12 + 8 * k), 2) for k in range(3)]
    for (vx, vy, vz), nv in crowded:
        for j in range(nv):
            p1.append((np.array([vx + 3 * j, vy + 2 * j, vz + j]) + 0.25 + 0.5 * rng.random((600, 3))) * dl32)          # (same bucket: the offsets stay inside 8 x 8 x 8)
            l1.append(rng.integers(-3, 20, (600, 1)) if (len(l1) & 1) else wrapping_labels(rng, 600))
    p1, l1 = np.concatenate(p1), np.concatenate(l1)
    p1[0] = 0.0
    perm = rng.permutation(len(p1))
    c1 = (p1[perm].astype(F32), rng.normal(0, 50, (len(p1), 3)).astype(F32), l1[perm].astype(np.int32))
    g0, g1 = geometry(c0[0], dl), geometry(c1[0], dl)
    assert g0.fits and g1.fits and g0.inside.all() and g1.inside.all()
    assert 2 <= np.count_nonzero(g0.records) <= 64
    assert (g0.vox_members.max() > FE_CAP) == bool(crowded0)
    nonempty = np.count_nonzero(g0.records) + np.count_nonzero(g1.records)
    assert nonempty > workgroups, "%d non-empty buckets for %d workgroups x 10" % (nonempty, workgroups // 10)
    assert g1.vox_members.max() <= FE_CAP and np.count_nonzero(g1.vox_members > 255) == 11
    big = np.flatnonzero(g1.records > FE_CAP)
    assert len(big) == 3
    for b in big:
        hist = bucket_hist(g1, b)
        bounds, taken = slices(hist)
        assert taken and len(bounds) - 1 >= 2
    one_pass = {int(b) for b in g1.bucket[np.isin(g1.key, g1.vox_key[g1.vox_members > 255])]} - {int(b) for b in big}
    assert len(one_pass) == 5
    assert max_distinct_labels(g1, c1[2]) <= LAB_CAP
    wraps = sum(bool(byte_counter_wraps(c1[2][g1.key == k, 0])) for k in g1.vox_key[g1.vox_members > 255] if (c1[2][g1.key == k, 0] >= 0).all() and (c1[2][g1.key == k, 0] < 13).all())
    assert wraps >= 4
    return [c0, c1], dl


# ---- the environment-selected forms (tests/_fe_forms_worker.py runs a group, tests/test_subsample_paths.py asserts on every line) -----------
FORM_ENV_NAMES = ("SSDR_FE_WGS", "SSDR_FE_MOVE_WGS", "SSDR_SUBSAMPLE_METHOD")


def form_inputs(group):
    """-> [(name, clouds, dl, status AUTO must report, clouds whose rows AUTO must match)]; SORT must report 0 and match every cloud"""
    assert group == "many"
    flagged, dl = many_items_clouds(True)
    healthy, _ = many_items_clouds(False)
    return [("many_items_flagged", flagged, dl, 4, (1,)), ("many_items", healthy, dl, 0, (0, 1))]


def form_names(group):
    """the lines the worker prints for a group, without building the inputs: name -> (status, match) expected"""
    names = {"many": ["many_items_flagged", "many_items"]}[group]
    want = {}
    for nm in names:
        want[nm + "/auto"] = 4 if nm == "many_items_flagged" else 0
        want[nm + "/sort"] = 0
    return want
