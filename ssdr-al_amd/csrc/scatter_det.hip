// Atomic-free backward scatters for the training step ("Deterministic mode"): the backward of gather_neighbour,
// nearest_interpolation and random_sample as a REDUCTION over the source row's inverse list instead of a float atomicAdd per position.
//
// Lists.  For idx [B][rows_per_b] into src_rows rows per batch element, the positions are keyed with q = b * src_rows + clamp(idx) and sorted by
// that key with the stable radix sort (radix_sort.hip), values = the position r inside its batch element.  Positions enter in ascending r, the
// sort is stable, so every row's positions come out in ascending r: `pos` is the sorted value array, `off[q]` the first slot whose key is >= q
// (a binary search per row of the sorted keys).  No atomic, integer or float, and nothing that depends on which lane ran first.
//
// Reductions.  One work-item per (source row, channel), channels fastest: s = +0, s = s + term for the row's positions in list order, then
// dsrc = dsrc + s.  Additions only (the build has -ffp-contract=off), so tests/_scatter_np.py restates the result bit for bit.
#include "scatter_det.hpp"

namespace ssdr {
namespace {

inline unsigned det_blocks(long n, int per = 256) { return (unsigned)((n + per - 1) / per); }

__global__ void inv_keys_kernel(const int32_t* idx, int rows_per_b, int src_rows, long total, uint64_t* keys, uint32_t* pos) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const long b = e / rows_per_b;
    int j = idx[e]; j = min(max(j, 0), src_rows - 1);
    keys[e] = (uint64_t)(b * src_rows + j);
    pos[e] = (uint32_t)(e - b * rows_per_b);
}
// off[q] = the number of sorted keys below q, q = 0 .. Q
__global__ void inv_off_kernel(const uint64_t* keys, int n, long Q, int* off) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > Q) return;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (keys[mid] < (uint64_t)q) lo = mid + 1; else hi = mid;
    }
    off[q] = lo;
}

__global__ void rows_reduce_kernel(const int* off, const int* pos, int src_rows, int rows_per_b, long Q, int C, const float* dout, int ldo, float* dsrc, int lds) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= Q * C) return;
    const int c = (int)(e % C); const long q = e / C, b = q / src_rows;
    const int i0 = off[q], i1 = off[q + 1];
    if (i0 == i1) return;
    const float* d = dout + b * rows_per_b * ldo + c;
    float s = 0.f;
    for (int i = i0; i < i1; ++i) s = s + d[(long)pos[i] * ldo];
    dsrc[q * lds + c] = dsrc[q * lds + c] + s;
}

// share[m, c] = dout[m, c] / ties(m, c): the 16 pooled rows equal to the maximum are counted each, a repeated index as often as it occurs
__global__ void pool_share_kernel(const float* src, int lds, int src_rows, const int32_t* idx, int m_per_b, long total_m, int C, const float* out, const float* dout,
                                  int ldo, float* share) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total_m * C) return;
    const int c = (int)(e % C); const long r = e / C, b = r / m_per_b;
    const float mx = out[r * ldo + c];
    int ties = 0;
    for (int k = 0; k < 16; ++k) {
        int j = idx[r * 16 + k]; j = min(max(j, 0), src_rows - 1);
        if (src[(b * src_rows + j) * lds + c] == mx) ++ties;
    }
    share[e] = ties ? dout[r * ldo + c] / (float)ties : 0.f;
}
// position r = m * 16 + k of row q's list is tied when the row's own value equals out[m, c]
__global__ void pool_reduce_kernel(const int* off, const int* pos, int src_rows, int m_per_b, long Q, int C, const float* src, const float* out, int ldo,
                                   const float* share, float* dsrc, int lds) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= Q * C) return;
    const int c = (int)(e % C); const long q = e / C, b = q / src_rows;
    const int i0 = off[q], i1 = off[q + 1];
    if (i0 == i1) return;
    const float v = src[q * lds + c];
    float s = 0.f;
    for (int i = i0; i < i1; ++i) {
        const long m = b * m_per_b + pos[i] / 16;
        if (v == out[m * ldo + c]) s = s + share[m * C + c];
    }
    dsrc[q * lds + c] = dsrc[q * lds + c] + s;
}

int key_bits_for(long Q) { int bits = 1; while (bits < 63 && (1L << bits) < Q) ++bits; return bits; }

}  // namespace

int inv_list_build(const int32_t* idx, int B, int rows_per_b, int src_rows, uint64_t* keys, InvList l, RadixSorter& sorter, hipStream_t s) {
    const long n = (long)B * rows_per_b, Q = (long)B * src_rows;
    if (n > 0) {
        hipLaunchKernelGGL(inv_keys_kernel, dim3(det_blocks(n)), dim3(256), 0, s, idx, rows_per_b, src_rows, n, keys, reinterpret_cast<uint32_t*>(l.pos));
        SSDR_HIP(hipGetLastError());
        SSDR_TRY(sorter.sort(keys, reinterpret_cast<uint32_t*>(l.pos), (int)n, nullptr, s, key_bits_for(Q)));
    }
    hipLaunchKernelGGL(inv_off_kernel, dim3(det_blocks(Q + 1)), dim3(256), 0, s, keys, (int)n, Q, l.off);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int scatter_rows_det(InvList l, int B, int rows_per_b, int src_rows, const float* dout, int ldo, int C, float* dsrc, int lds, hipStream_t s) {
    const long Q = (long)B * src_rows;
    hipLaunchKernelGGL(rows_reduce_kernel, dim3(det_blocks(Q * C)), dim3(256), 0, s, l.off, l.pos, src_rows, rows_per_b, Q, C, dout, ldo, dsrc, lds);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int pool_grad_det(InvList l, const float* src, float* dsrc, int lds, int src_rows, const int32_t* idx, int B, int m_per_b, int C, const float* out,
                  const float* dout, int ldo, float* share, hipStream_t s) {
    const long total_m = (long)B * m_per_b, Q = (long)B * src_rows;
    hipLaunchKernelGGL(pool_share_kernel, dim3(det_blocks(total_m * C)), dim3(256), 0, s, src, lds, src_rows, idx, m_per_b, total_m, C, out, dout, ldo, share);
    hipLaunchKernelGGL(pool_reduce_kernel, dim3(det_blocks(Q * C)), dim3(256), 0, s, l.off, l.pos, src_rows, m_per_b, Q, C, src, out, ldo, share, dsrc, lds);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

namespace {

// scratch of the two exported pieces, per stream: [off | pos | keys | share]
struct ScatterScratch { DevBuf buf; RadixSorter sorter; };

struct PieceLayout { InvList l; uint64_t* keys; float* share; };

int piece_scratch(hipStream_t s, long B, long rows_per_b, long src_rows, long share_floats, ScatterScratch** out, PieceLayout* lay) {
    ScatterScratch& sc = per_stream<ScatterScratch>(s);
    const long n_off = inv_off_ints(B, src_rows), n_pos = inv_pos_ints(B, rows_per_b), n = B * rows_per_b;
    SSDR_TRY(sc.buf.reserve((size_t)(n_off + n_pos) * 4 + (size_t)n * 8 + (size_t)share_floats * 4 + 64));
    lay->l.off = sc.buf.as<int>(); lay->l.pos = lay->l.off + n_off;
    lay->keys = reinterpret_cast<uint64_t*>(lay->l.pos + n_pos);
    lay->share = reinterpret_cast<float*>(lay->keys + n);
    *out = &sc;
    return SSDR_OK;
}

int check_piece(const char* who, long B, long rows_per_b, long src_rows, int C, int ldo, int lds) {
    if (C <= 0) { set_error("%s: C = %d channels", who, C); return SSDR_ERR_INVALID; }
    if (ldo < C || lds < C) { set_error("%s: a leading dimension (ldo %d, lds %d) is below C = %d", who, ldo, lds, C); return SSDR_ERR_INVALID; }
    if (B < 0 || rows_per_b < 0 || src_rows < 0) { set_error("%s: a negative size", who); return SSDR_ERR_INVALID; }
    if (B * rows_per_b > 0 && src_rows == 0) { set_error("%s: indices into no source row", who); return SSDR_ERR_INVALID; }
    if (B * rows_per_b > (1L << 30) || B * src_rows > (1L << 30)) { set_error("%s: more than 2^30 rows", who); return SSDR_ERR_UNSUPPORTED; }
    return SSDR_OK;
}

}  // namespace
}  // namespace ssdr

using namespace ssdr;

extern "C" {

/* dsrc[(b, clamp(idx[b, r])), c] += dout[(b, r), c], every source row summing its positions in ascending r: no float atomic, the same bits every run */
int ssdr_scatter_add_rows_dev(const int32_t* d_idx, int B, int rows_per_b, int src_rows, const float* d_dout, int ldo, int C, float* d_dsrc, int lds, void* stream) {
    if (!d_idx || !d_dout || !d_dsrc) { set_error("scatter_add_rows: NULL pointer"); return SSDR_ERR_INVALID; }
    SSDR_TRY(check_piece("scatter_add_rows", B, rows_per_b, src_rows, C, ldo, lds));
    if ((long)B * rows_per_b == 0) return SSDR_OK;
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    ScatterScratch* sc = nullptr; PieceLayout lay;
    SSDR_TRY(piece_scratch(s, B, rows_per_b, src_rows, 0, &sc, &lay));
    SSDR_TRY(inv_list_build(d_idx, B, rows_per_b, src_rows, lay.keys, lay.l, sc->sorter, s));
    return scatter_rows_det(lay.l, B, rows_per_b, src_rows, d_dout, ldo, C, d_dsrc, lds, s);
}

/* random_sample backward: d_idx i32 [B, m_per_b, 16]; out / dout [B m_per_b, C] with leading dimension ldo, src / dsrc [B src_rows, C] with lds.
 * Position (m, k) is tied when src[(b, clamp(idx)), c] == out[m, c]; a tied position adds dout[m, c] / ties(m, c) to its source row, in ascending
 * position order per row. */
int ssdr_pool_grad_rows_dev(const float* d_src, float* d_dsrc, int lds, int src_rows, const int32_t* d_idx, int B, int m_per_b, int C, const float* d_out,
                            const float* d_dout, int ldo, void* stream) {
    if (!d_src || !d_dsrc || !d_idx || !d_out || !d_dout) { set_error("pool_grad_rows: NULL pointer"); return SSDR_ERR_INVALID; }
    SSDR_TRY(check_piece("pool_grad_rows", B, (long)m_per_b * 16, src_rows, C, ldo, lds));
    if ((long)B * m_per_b == 0) return SSDR_OK;
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    ScatterScratch* sc = nullptr; PieceLayout lay;
    SSDR_TRY(piece_scratch(s, B, (long)m_per_b * 16, src_rows, (long)B * m_per_b * C, &sc, &lay));
    SSDR_TRY(inv_list_build(d_idx, B, m_per_b * 16, src_rows, lay.keys, lay.l, sc->sorter, s));
    return pool_grad_det(lay.l, d_src, d_dsrc, lds, src_rows, d_idx, B, m_per_b, C, d_out, d_dout, ldo, lay.share, s);
}

}
