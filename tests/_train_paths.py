"""Helpers of tests/test_train_paths.py: the constants of the training step's launchers read from csrc/randla_train.hip, `plan` (a Python restatement of
the launcher arithmetic of launch_gemm / dw_split / red_split and of the loss's grid: every launch of a step with its tile, partial tiles, k-chunks and row
chunks, so that a case can assert BEFORE the library is called that it is on the branch it names), the float64 NumPy oracles of the three exported pieces
(ssdr_randla_train_gemm_dev / _dw_dev / _reduce_dev) with their derived error bars, and the callers of those pieces.

Bars (u = 2^-24, float32's unit roundoff; all derived, none measured):
  GEMM, dW   elementwise |c - c64| <= (n + 2) u sum|a||b| (the bias and C's old value under `accumulate` count as terms), n = the longest chain of
             roundings an output passes through: K for the forward's one fmaf chain, kchunk + nz for dW (a slab's chain, then the slabs' sum).
  sums       (reduce modes 1 and 2) |s - s64| <= (n + e) u sum|term|, n = rows per lane + lanes + chunks (a lane's serial sum, the lanes' sum, the
             chunks' sum), e = the roundings that make a term (1 for dY = 0.2 dA, 3 more for dY * xhat).
  mean       Chan's merge adds four roundings per chunk: n = rows per lane + lanes + 4 chunks + 2, times u sum|x| / M.
  variance   relative to m2 (every term of m2 is positive): (n + 4 chunks + 4) u var64 for the roundings (a square is two roundings more than a sum's
             term, the division by M and Chan's four roundings per merged chunk),
             plus what the chunk means' own error E does: a chunk's squared deviations about a mean that is off by e grow by n_b e^2, and the between-chunk
             term n_b (mu_b - mu)^2 moves by at most n_b (4 E |mu_b - mu| + 4 E^2):  5 E^2 + 4 E s_between, s_between^2 = sum n_b (mu_b - mu)^2 / M in float64.
  invstd     through its derivative: |d invstd| <= bar_var / (2 (var64 - bar_var + eps)^1.5) + 4 u invstd (float32's eps, add, sqrt, divide)."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ssdr-al_amd", "csrc", "randla_train.hip")
F32 = np.float32
U = 2.0 ** -24
BN_EPS = 1e-6
ERR_INVALID = 1
SENT = F32(-77.25)

# ---- constants, from the source ----------------------------------------------------------------------------------------------------------------------
_K = None


def constants():
    """BK, PART_FLOATS, DWP_FLOATS and the four gemm_kernel tile shapes, in the launcher's order (M <= 16 and N <= 16 | N <= 16 | M <= 16 | else)"""
    global _K
    if _K is None:
        with open(SRC) as f:
            text = f.read()
        out = {}
        m = re.findall(r"constexpr int BK\s*=\s*([0-9]+)\s*;", text)
        assert len(m) == 1, "BK: %d definitions" % len(m)
        out["BK"] = int(m[0])
        for nm in ("PART_FLOATS", "DWP_FLOATS"):
            m = re.findall(r"\b%s\s*=\s*1\s*<<\s*([0-9]+)\s*[,;]" % nm, text)
            assert len(m) == 1, "%s: %d definitions" % (nm, len(m))
            out[nm] = 1 << int(m[0])
        body = text[text.index("int launch_gemm("):]
        body = body[:body.index("return SSDR_OK")]
        tiles = re.findall(r"gemm_kernel<\s*([0-9]+)\s*,\s*([0-9]+)\s*,\s*[0-9]+\s*,\s*[0-9]+\s*>", body)
        assert len(tiles) == 4 and len(set(tiles)) == 4, "launch_gemm: expected four distinct gemm_kernel instantiations, found %s" % (tiles,)
        assert set(re.findall(r"gemm_kernel<\s*([0-9]+)\s*,\s*([0-9]+)\s*,", text)) == set(tiles), "a gemm_kernel instantiation outside launch_gemm"
        out["TILES"] = [(int(a), int(b)) for a, b in tiles]
        conds = re.findall(r"if \((M <= 16 && N <= 16|N <= 16|M <= 16)\)", body)
        assert conds == ["M <= 16 && N <= 16", "N <= 16", "M <= 16"], "launch_gemm: the tile choice changed: %s" % (conds,)
        _K = SimpleNamespace(**out)
    return _K


def tile_name(t):
    return "%dx%d" % t


# ---- the launcher arithmetic -------------------------------------------------------------------------------------------------------------------------
def gemm_plan(M, N, K, split=1):
    """launch_gemm: the tile, its grid, the partial tiles, the k-chunks"""
    k = constants()
    t = k.TILES[0] if (M <= 16 and N <= 16) else k.TILES[1] if N <= 16 else k.TILES[2] if M <= 16 else k.TILES[3]
    kchunk = ((K + split - 1) // split + k.BK - 1) // k.BK * k.BK
    nz = (K + kchunk - 1) // kchunk
    last = K - (nz - 1) * kchunk
    return SimpleNamespace(M=M, N=N, K=K, tile=t, grid=((M + t[0] - 1) // t[0], (N + t[1] - 1) // t[1], nz), partial_m=M % t[0] != 0, partial_n=N % t[1] != 0,
                           kchunk=kchunk, nz=nz, last=last, ragged=nz > 1 and last != kchunk, k_tail=last % k.BK, chain=min(K, kchunk))


def dw_plan(M, cin, cout):
    """dw_split + launch_gemm of dW = x^T dz over M rows"""
    k = constants()
    want = max(1, min(M // 512, 1024))
    split = max(1, min(want, k.DWP_FLOATS // (cin * cout)))
    p = gemm_plan(cin, cout, M, split)
    kchunk = ((M + split - 1) // split + k.BK - 1) // k.BK * k.BK
    assert p.kchunk == kchunk and p.nz == (M + kchunk - 1) // kchunk
    p.split, p.want, p.cap_bound = split, want, split < want
    p.n = p.kchunk + p.nz                  # the bar's chain: a slab's fmaf chain, then sum_slabs_kernel
    return p


def reduce_plan(M, Cn):
    """red_split: channel lanes ct, row lanes nsub, the row chunks"""
    k = constants()
    ct = 8
    while ct < 64 and ct < Cn:
        ct *= 2
    want = max(1, min(M // 1024, 1024))
    capped = max(1, min(want, k.PART_FLOATS // (2 * Cn)))
    chunk = (M + capped - 1) // capped
    nchunks = (M + chunk - 1) // chunk
    last = M - (nchunks - 1) * chunk
    nsub = 256 // ct
    rpl = (chunk + nsub - 1) // nsub
    return SimpleNamespace(M=M, C=Cn, ct=ct, nsub=nsub, chunk=chunk, nchunks=nchunks, last=last, ragged=nchunks > 1 and last != chunk, below_ct=Cn < ct,
                           cblocks=(Cn + ct - 1) // ct, partial_cblock=Cn % ct != 0 and Cn > ct, few_rows=M < nsub, part_cap_bound=capped < want,
                           n=rpl + nsub + nchunks, n_mean=rpl + nsub + 4 * nchunks + 2, rpl=rpl)


def levels(cfg):
    N = [cfg.num_points]
    for r in cfg.sub_sampling_ratio:
        assert N[-1] % r == 0
        N.append(N[-1] // r)
    return N


def units(cfg, B):
    """(name, in, out, bias, bn, has dx, rows) of every unit, in graph order (build_units / Runner::forward)"""
    N, L, d_out = levels(cfg), cfg.num_layers, list(cfg.d_out)
    out = [("fc0", 6, 8, True, True, False, B * N[0])]
    width, skips = 8, []
    for i in range(L):
        d, rows, p = d_out[i], B * N[i], "Encoder_layer_%d" % i
        R = rows * 16
        out += [(p + "mlp1", width, d // 2, True, True, True, rows), (p + "LFAmlp1", 10, d // 2, True, True, False, R),
                (p + "LFAatt_pooling_1fc", d, d, False, False, True, R), (p + "LFAatt_pooling_1mlp", d, d // 2, True, True, True, rows),
                (p + "LFAmlp2", d // 2, d // 2, True, True, True, R), (p + "LFAatt_pooling_2fc", d, d, False, False, True, R),
                (p + "LFAatt_pooling_2mlp", d, d, True, True, True, rows), (p + "mlp2", d, 2 * d, True, True, True, rows),
                (p + "shortcut", width, 2 * d, True, True, True, rows)]
        if i == 0:
            skips.append(2 * d)
        width = 2 * d
        skips.append(width)
    out.append(("decoder_0", width, width, True, True, True, B * N[L]))
    for j in range(L):
        skip = skips[len(skips) - j - 2]
        out.append(("Decoder_layer_%d" % j, skip + width, skip, True, True, True, B * N[L - 1 - j]))
        width = skip
    out += [("fc1", width, 64, True, True, True, B * N[0]), ("fc2", 64, 32, True, True, True, B * N[0]), ("fc", 32, cfg.num_classes, True, False, True, B * N[0])]
    return out


def plan(cfg, B):
    """every launch of a training step that goes through the three launchers, and the loss's grid.
    -> SimpleNamespace(launches=[SimpleNamespace(unit, role, p)], loss=SimpleNamespace(rows, blocks, partial, trips), branches=set of BRANCHES names)"""
    launches = []
    for name, cin, cout, bias, bn, dx, rows in units(cfg, B):
        launches.append(SimpleNamespace(unit=name, role="forward", p=gemm_plan(rows, cout, cin)))
        if bn:
            launches.append(SimpleNamespace(unit=name, role="reduce0", p=reduce_plan(rows, cout)))
            launches.append(SimpleNamespace(unit=name, role="reduce1", p=reduce_plan(rows, cout)))
        if bias:
            launches.append(SimpleNamespace(unit=name, role="reduce2", p=reduce_plan(rows, cout)))
        launches.append(SimpleNamespace(unit=name, role="dW", p=dw_plan(rows, cin, cout)))
        if dx:
            launches.append(SimpleNamespace(unit=name, role="dx", p=gemm_plan(rows, cin, cout)))
    rows0 = B * cfg.num_points
    blocks = (rows0 + 255) // 256
    loss = SimpleNamespace(rows=rows0, blocks=blocks, partial=rows0 % 256 != 0, trips=(blocks + 255) // 256)
    br = set()
    for l in launches:
        br |= launch_branches(l.role, l.p)
    if loss.trips > 1:
        br.add("loss: more than 256 row blocks into the combining block")
    if loss.partial:
        br.add("loss: a row count that is no multiple of 256")
    return SimpleNamespace(launches=launches, loss=loss, branches=br)


def launch_branches(role, p):
    """the names of BRANCHES this launch is on"""
    br = set()
    if role in ("forward", "dx", "dW"):
        br.add("gemm_kernel<%s> as %s" % (tile_name(p.tile), "dW" if role == "dW" else "forward / dx"))
        if role == "dW":
            if p.ragged:
                br.add("dW: last k-chunk shorter than kchunk")
            if p.k_tail:
                br.add("dW: k tail in the %s tile" % tile_name(p.tile))
            if p.cap_bound:
                br.add("dW: split cut by the slab buffer")
            if p.nz > 1:
                br.add("dW: more than one slab")
        else:
            if p.k_tail:
                br.add("forward / dx: k tail (K % 16)")
            if p.partial_m and p.tile == constants().TILES[1]:
                br.add("forward: partial M tile of the 256x16 kernel")
    else:
        mode = role[-1]
        if p.ragged:
            br.add("reduce mode %s: last row chunk shorter than chunk" % mode)
        if p.below_ct and mode in "01":
            br.add("reduce mode %s: C below ct" % mode)
        if p.partial_cblock:
            br.add("reduce: a partial last channel block")
        if p.few_rows:
            br.add("reduce: fewer rows than row lanes")
        assert not p.part_cap_bound, "the PART_FLOATS cap binds: create() limits d_out to 512, so C <= 1024 and the cap is 1024 = the largest want"
    return br


def branches():
    """the table of DESIGN.md "The training step's launchers, branch by branch": every entry must be reached by a case (the closing test)"""
    k = constants()
    out = ["gemm_kernel<%s> as %s" % (tile_name(t), role) for t in k.TILES for role in ("forward / dx", "dW")]
    out += ["dW: k tail in the %s tile" % tile_name(t) for t in k.TILES]
    out += ["dW: last k-chunk shorter than kchunk", "dW: split cut by the slab buffer", "dW: more than one slab", "forward / dx: k tail (K % 16)",
            "forward: partial M tile of the 256x16 kernel"]
    out += ["reduce mode %d: last row chunk shorter than chunk" % m for m in range(3)]
    out += ["reduce mode %d: C below ct" % m for m in range(2)]
    out += ["reduce: a partial last channel block", "reduce: fewer rows than row lanes", "loss: more than 256 row blocks into the combining block",
            "loss: a row count that is no multiple of 256"]
    return out


# ---- the pieces' callers -----------------------------------------------------------------------------------------------------------------------------
def bound():
    from ssdr_al import _lib
    L = _lib.lib()
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.ssdr_randla_train_gemm_dev.argtypes = [vp, i64, i64, vp, i64, i64, vp, i64, i64, i32, i32, i32, vp, i32, vp]
    L.ssdr_randla_train_dw_dev.argtypes = [vp, i32, vp, i32, i32, i32, vp, i64, i64, vp]
    L.ssdr_randla_train_reduce_dev.argtypes = [i32, vp, i32, vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp]
    return L


def _up(a):
    from ssdr_al._lib import DevArray
    return DevArray.from_host(np.ascontiguousarray(a))


def _at(d, off):
    return d.ptr + 4 * int(off)


def strided(rng, rows, cols, transposed, pad, off, fill=None):
    """a float32 matrix of `rows` x `cols` inside a larger buffer -> (buffer, element offset, row stride, column stride, the values)"""
    r, c = (cols, rows) if transposed else (rows, cols)
    buf = rng.standard_normal((r, c + pad)).astype(F32) if fill is None else np.full((r, c + pad), fill, F32)
    view = buf[:, off:off + c]
    return buf, off, (1 if transposed else c + pad), (c + pad if transposed else 1), (view.T if transposed else view)


def run_gemm(A, B, Cbuf, c_off, crs, ccs, M, N, K, bias, accumulate):
    """A, B: (buffer, offset, rs, cs); Cbuf: the host buffer C lives in -> the buffer afterwards"""
    from ssdr_al import _lib
    L = bound()
    dA, dB, dC = _up(A[0]), _up(B[0]), _up(Cbuf)
    db = None if bias is None else _up(bias)
    _lib.check(L.ssdr_randla_train_gemm_dev(_at(dA, A[1]), A[2], A[3], _at(dB, B[1]), B[2], B[3], _at(dC, c_off), crs, ccs, M, N, K, None if db is None else db.ptr,
                                            int(accumulate), None))
    _lib.sync()
    return dC.to_host()


def run_dw(xbuf, x_off, ldx, dz, M, cin, cout, outbuf, rs, cs):
    from ssdr_al import _lib
    L = bound()
    dx, dd, do = _up(xbuf), _up(dz), _up(outbuf)
    _lib.check(L.ssdr_randla_train_dw_dev(_at(dx, x_off), ldx, dd.ptr, M, cin, cout, do.ptr, rs, cs, None))
    _lib.sync()
    return do.to_host()


def run_reduce(mode, zbuf, z_off, ldz, M, Cn, da=None, av=None, a_off=0, lda=0, act=0, mean=None, invstd=None, mov=None, unbiased=0):
    """-> (out0 [C + 1], out1 [C + 1] with a sentinel behind, moving mean, moving variance)"""
    from ssdr_al import _lib
    L = bound()
    dz = _up(zbuf)
    dda, dav = (None if da is None else _up(da)), (None if av is None else _up(av))
    dm, di = (None if mean is None else _up(mean)), (None if invstd is None else _up(invstd))
    o0, o1 = _up(np.full(Cn + 1, SENT, F32)), _up(np.full(Cn + 1, SENT, F32))
    mm, mv = (None, None) if mov is None else (_up(mov[0]), _up(mov[1]))
    p = lambda d, off=0: None if d is None else _at(d, off)
    _lib.check(L.ssdr_randla_train_reduce_dev(mode, _at(dz, z_off), ldz, p(dda, a_off), p(dav, a_off), lda, act, p(dm), p(di), M, Cn, o0.ptr, o1.ptr, p(mm), p(mv),
                                              unbiased, None))
    _lib.sync()
    return o0.to_host(), o1.to_host(), None if mm is None else mm.to_host(), None if mv is None else mv.to_host()


# ---- oracles and bars of the reductions ----------------------------------------------------------------------------------------------------------------
def stats_oracle(z, p):
    """float64 mean, biased variance, and the bars of mean / variance / invstd for a [M, C] float32 matrix under reduce_plan p"""
    z = np.asarray(z, np.float64)
    M = z.shape[0]
    mu = z.mean(0)
    var = ((z - mu) ** 2).mean(0)
    bar_mu = p.n_mean * U * np.abs(z).sum(0) / M
    edges = list(range(0, M, p.chunk)) + [M]
    E = np.zeros(z.shape[1]); between = np.zeros(z.shape[1])
    for a, b in zip(edges[:-1], edges[1:]):
        E = np.maximum(E, (p.rpl + p.nsub + 1) * U * np.abs(z[a:b]).sum(0) / (b - a))
        between += (b - a) * (z[a:b].mean(0) - mu) ** 2
    bar_var = (p.n + 4 * p.nchunks + 4) * U * var + 5 * E * E + 4 * E * np.sqrt(between / M)
    inv = 1.0 / np.sqrt(var + BN_EPS)
    bar_inv = bar_var / (2 * np.maximum(var - bar_var, 0.0) + 2 * BN_EPS) / np.sqrt(np.maximum(var - bar_var, 0.0) + BN_EPS) + 4 * U * inv
    return SimpleNamespace(mu=mu, var=var, inv=inv, bar_mu=bar_mu, bar_var=bar_var, bar_inv=bar_inv)
