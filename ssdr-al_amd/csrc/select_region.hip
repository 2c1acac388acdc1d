// Region selectors of sampling() beside gcn_fps, for gfx950 (S3/sampler2.py:644-806, TSampler.sampling()'s branches):
//   "edcd" (:670-685): per cloud, farthest_superpoint_sample (:49-80) over its candidates with the distance |centre_i - centre_c|^2 + CD(i, c);
//   plain uncertainty (:783-806): the first batch_size regions of the ranking.
//
// edcd runs every cloud's chain in ONE launch, one workgroup per cloud: the counts come from the device (the candidate rule of select.hip, or the
// caller), so the host reads nothing between the ranking and the picks.  The arithmetic is fps_superpoint's (select_fps.hip) step for step — ed =
// (dx*dx + dy*dy) + dz*dz, dist = ed + cd, running minima from 1e10, trigger row 0, arg-max with the lowest index among equal values (np.argmax) —
// so the picks are index for index those of the single-cloud entry.  What differs is the layout: fps_superpoint reads cd(c, i) as dir[c][i] +
// dir[i][c], a strided column read (one cache line per row per pick); here each block is symmetrised once (IEEE addition commutes: the same
// sums) and a pick reads one contiguous row.  The running minima live in LDS (8 B per row: 64 KiB at the 8 192-row limit).
#include "ssdr_internal.hpp"
#include "select_fps.hpp"
#include "select_region.hpp"
#include <mutex>

namespace ssdr {
namespace {

// (value, index) arg-max over the wave, result in every lane (values are never NaN here)
__device__ __forceinline__ void wave_argmax_pair(double& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (better(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

// output offsets (exclusive prefix of ntop) and the limits; one workgroup.  A status already set (the candidate rule's capacities) stops everything
__global__ __launch_bounds__(256) void edcd_plan(const int* __restrict__ coff, const int* __restrict__ ntop, int B, int lim, long long max_select, int* ooff, int* status) {
    __shared__ long long s_part[257];
    __shared__ int s_flags;
    if (*status) return;
    const int tid = threadIdx.x, per = (B + 255) / 256, lo = min(B, tid * per), hi = min(B, lo + per);
    if (tid == 0) s_flags = 0;
    __syncthreads();
    long long sum = 0; int fl = 0;
    for (int b = lo; b < hi; ++b) {
        const int n = coff[b + 1] - coff[b], k = ntop[b];
        if (k > 0 && n > lim) fl |= EDCD_ST_TOO_BIG;
        if (k > n || k < 0) fl |= EDCD_ST_COUNT;
        sum += max(k, 0);
    }
    if (fl) atomicOr(&s_flags, fl);
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int t = 0; t < 256; ++t) { const long long v = s_part[t]; s_part[t] = run; run += v; }
        s_part[256] = run;
    }
    __syncthreads();
    long long run = s_part[tid];
    for (int b = lo; b < hi; ++b) { ooff[b] = (int)min(run, (long long)0x7fffffff); run += max(ntop[b], 0); }
    if (tid == 0) {
        ooff[B] = (int)min(s_part[256], (long long)0x7fffffff);
        int f = s_flags;
        if (s_part[256] > max_select) f |= EDCD_ST_CAP;
        if (f) *status = f;
    }
}

// cd = dir + dir^T inside every cloud's block, diagonal 0 (fps_superpoint's `i == c ? 0 : dir[c][i] + dir[i][c]`); blockIdx.y = cloud.  The thread
// of the pair (i < j) reads both entries and writes both: no other thread touches them
__global__ __launch_bounds__(256) void edcd_symmetrise(const int* __restrict__ coff, const long long* __restrict__ boff, const int* __restrict__ status, double* cd) {
    if (*status) return;
    const int b = blockIdx.y, n = coff[b + 1] - coff[b];
    double* d = cd + boff[b];
    const long long nn = (long long)n * n;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nn; e += (long long)gridDim.x * 256) {
        const int i = (int)(e / n), j = (int)(e % n);
        if (i < j) {
            const size_t t = (size_t)j * n + i;
            const double v = d[e] + d[t];
            d[e] = v; d[t] = v;
        } else if (i == j) {
            d[e] = 0.0;
        }
    }
}

// one workgroup per cloud: the whole pick chain of farthest_superpoint_sample.  A lane owns rows tid, tid + NT, ... for the whole chain, so its
// running minima need no barrier; the waves' arg-maxes meet in LDS
template <int NT>
__global__ __launch_bounds__(NT) void edcd_fps_batch(const double* __restrict__ centres, const double* __restrict__ cd, const int* __restrict__ coff,
                                                     const long long* __restrict__ boff, const int* __restrict__ ntop, const int* __restrict__ ooff,
                                                     const int* __restrict__ status, int* __restrict__ out) {
    constexpr int NW = NT / 64;
    __shared__ double s_v[NW];
    __shared__ int s_i[NW];
    SSDR_DYN_SHARED(double, mind);          // [n]
    if (*status) return;
    const int b = blockIdx.x, r0 = coff[b], n = coff[b + 1] - r0, count = ntop[b];
    if (count <= 0 || n <= 0) return;
    const double* cen = centres + 3 * (size_t)r0;
    const double* blk = cd + boff[b];
    int* o = out + ooff[b];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int i = tid; i < n; i += NT) mind[i] = 1.0e10;
    int c = 0;                               // trigger_idx 0: the cloud's most uncertain candidate
    for (int it = 0;; ++it) {
        if (tid == 0) o[it] = r0 + c;
        if (it + 1 == count) break;
        const double cx = cen[3 * c], cy = cen[3 * c + 1], cz = cen[3 * c + 2];
        const double* row = blk + (size_t)c * n;
        double bv = -1.0; int bi = 0x7fffffff;
        for (int i = tid; i < n; i += NT) {
            const double dx = cen[3 * i] - cx, dy = cen[3 * i + 1] - cy, dz = cen[3 * i + 2] - cz;
            const double ed = (dx * dx + dy * dy) + dz * dz;               // np.sum(.., axis=-1) over 3 terms
            const double dist = ed + row[i];
            double m = mind[i];
            if (dist < m) { m = dist; mind[i] = m; }
            if (better(m, i, bv, bi)) { bv = m; bi = i; }
        }
        wave_argmax_pair(bv, bi);
        if constexpr (NW == 1) {
            c = bi;
        } else {
            if (lane == 0) { s_v[w] = bv; s_i[w] = bi; }
            __syncthreads();
            double v = s_v[0]; int k = s_i[0];
#pragma unroll
            for (int q = 1; q < NW; ++q) if (better(s_v[q], s_i[q], v, k)) { v = s_v[q]; k = s_i[q]; }
            c = k;
            __syncthreads();                 // s_v / s_i are rewritten by the next pick
        }
    }
}

// The first min(batch, population) not-skipped entries of a ranking, in rank order; of those, the ones in [lo, hi) are written (minus lo).  One
// workgroup walks the ranking in chunks of 1024 and stops once the top is complete (skipped regions rank anywhere; the chunks before the top's
// end are all it reads).  res[0] = entries written, res[1] = size of the top
constexpr int TK_NT = 1024;
__global__ __launch_bounds__(TK_NT) void topk_regions(const int* __restrict__ order, int n, const unsigned char* __restrict__ skip, int lim, int lo, int hi,
                                                      int* res, int* out) {
    __shared__ int s_a[TK_NT / 64], s_b[TK_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int run = 0, krun = 0;
    for (int base = 0; base < n && run < lim; base += TK_NT) {          // (run is the same in every thread: the loop is uniform)
        const int r = base + tid;
        int id = -1; bool v = false;
        if (r < n) { id = order[r]; v = !skip[id]; }
        const unsigned long long mv = __ballot(v);
        if (lane == 0) s_a[w] = __popcll(mv);
        __syncthreads();
        int pre = 0, tot = 0;
        for (int q = 0; q < TK_NT / 64; ++q) { const int c = s_a[q]; if (q < w) pre += c; tot += c; }
        const int pos = run + pre + __popcll(mv & below);
        const bool k = v && pos < lim && id >= lo && id < hi;
        const unsigned long long mk = __ballot(k);
        if (lane == 0) s_b[w] = __popcll(mk);
        __syncthreads();
        int kpre = 0, ktot = 0;
        for (int q = 0; q < TK_NT / 64; ++q) { const int c = s_b[q]; if (q < w) kpre += c; ktot += c; }
        if (k) out[krun + kpre + __popcll(mk & below)] = id - lo;
        run += tot; krun += ktot;
        __syncthreads();
    }
    if (tid == 0) { res[0] = krun; res[1] = min(run, lim); }
}

struct RegionState { DevBuf ooff, status; };
RegionState& rst(hipStream_t s) { return per_stream<RegionState>(s); }

template <int NT>
int edcd_fps_kernel(unsigned B, int lds_rows, const double* d_centres, const double* d_cd_dir, const int* d_coff, const long long* d_boff, const int* d_ntop,
                    const int* d_ooff, const int* d_status, int* d_out, hipStream_t s) {
    static std::once_flag once;          // 8 B per row next to the static arrays: beyond the 64 KiB default at the 8 192-row limit
    static hipError_t attr = hipSuccess;
    std::call_once(once, [] { attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&edcd_fps_batch<NT>), hipFuncAttributeMaxDynamicSharedMemorySize, 8 * EDCD_MAX_ROWS); });
    SSDR_HIP(attr);
    hipLaunchKernelGGL(edcd_fps_batch<NT>, dim3(B), dim3(NT), 8 * (size_t)lds_rows, s, d_centres, d_cd_dir, d_coff, d_boff, d_ntop, d_ooff, d_status, d_out);
    return SSDR_OK;
}

}  // namespace

int edcd_fps_launch(const double* d_centres, double* d_cd_dir, const int* d_coff, const long long* d_boff, const int* d_ntop, int num_clouds, int n_max,
                    long long max_select, int* d_ooff, int* d_status, int* d_out, hipStream_t s) {
    if (num_clouds <= 0) return SSDR_OK;
    const int lim = std::max(1, std::min(n_max, EDCD_MAX_ROWS));
    const unsigned B = (unsigned)num_clouds;
    ProfScope prof("sel_edcd_fps", s, 0.0);
    hipLaunchKernelGGL(edcd_plan, dim3(1), dim3(256), 0, s, d_coff, d_ntop, num_clouds, lim, max_select, d_ooff, d_status);
    hipLaunchKernelGGL(edcd_symmetrise, dim3((unsigned)std::max<long>(1, std::min<long>(((long)lim * lim + 255) / 256, 256)), B), dim3(256), 0, s,
                       d_coff, d_boff, (const int*)d_status, d_cd_dir);
    // a wave per cloud while every cloud fits four rows per lane (the reference's ~74 candidates per cloud): no barrier in the chain
    if (lim <= 256) SSDR_TRY(edcd_fps_kernel<64>(B, lim, d_centres, d_cd_dir, d_coff, d_boff, d_ntop, d_ooff, d_status, d_out, s));
    else SSDR_TRY(edcd_fps_kernel<256>(B, lim, d_centres, d_cd_dir, d_coff, d_boff, d_ntop, d_ooff, d_status, d_out, s));
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

}  // namespace ssdr

using namespace ssdr;

extern "C" {

int ssdr_edcd_fps_batch_dev(const double* d_centres, double* d_cd_dir, const int32_t* d_coff, const int64_t* d_boff, const int32_t* d_ntop, size_t num_clouds,
                            size_t n_max, size_t max_select, int32_t* d_out, int32_t* d_status, void* stream) {
    if (!d_centres || !d_cd_dir || !d_coff || !d_boff || !d_ntop || !d_out || num_clouds == 0 || num_clouds > 0x7fffffff || n_max == 0 || n_max > (size_t)EDCD_MAX_ROWS) {
        set_error("edcd_fps_batch: bad arguments (1 <= n_max <= 8192, at least one cloud)"); return SSDR_ERR_INVALID;
    }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); RegionState& R = rst(s);
    SSDR_TRY(R.ooff.reserve(4 * (num_clouds + 1)));
    int* st = d_status;
    if (!st) { SSDR_TRY(R.status.reserve(16)); st = R.status.as<int>(); }
    SSDR_HIP(hipMemsetAsync(st, 0, 4, s));
    return edcd_fps_launch(d_centres, d_cd_dir, d_coff, (const long long*)d_boff, d_ntop, (int)num_clouds, (int)n_max, (long long)std::min<size_t>(max_select, (size_t)1 << 62),
                           R.ooff.as<int>(), st, d_out, s);
}

int ssdr_topk_regions_dev(const int32_t* d_order, size_t n, const uint8_t* d_skip, size_t batch_size, size_t lo, size_t hi, int32_t* d_res, int32_t* d_out, void* stream) {
    if (!d_order || !d_skip || !d_res || !d_out || n > 0x7ffffff0 || lo > hi || hi > 0x7ffffff0) { set_error("topk_regions: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    hipLaunchKernelGGL(topk_regions, dim3(1), dim3(TK_NT), 0, s, d_order, (int)n, d_skip, (int)std::min<size_t>(batch_size, 0x7fffffff), (int)lo, (int)hi, d_res, d_out);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

}
