// Data-parallel training: the kernels on either side of the four kinds of collectives of a step ("Data-parallel") and the
// stand-alone entries over them.  The library links no collective library: randla_train.hip calls the host's exchange callback between a pack and
// a merge, and the callback only enqueues on the same stream.
//
// All kernels are one work-item per channel (or per element), 64 per workgroup: C is at most 1024, the work is a few dozen loads per work-item, and
// what a step pays for them is launch latency, not bandwidth.  So there is exactly one launch in front of a collective and one behind it, and none
// touches the activations.  Every merge adds in rank order starting from 0 (0 + x and a Chan merge from n = 0 are exact: world 1 reproduces the
// plain step bit for bit).  No fused multiply-add is formed (-ffp-contract=off), so tests restate the merges in NumPy float32 exactly.
#include "train_exchange.hpp"

namespace ssdr {
namespace {

constexpr float BN_EPS = 1e-6f, BN_MOMENTUM = 0.99f;       // as randla_train.hip

inline unsigned groups_of(long n) { return (unsigned)((n + 63) / 64); }

__global__ void pack_stats_kernel(const float* part, int nchunks, int chunk, int M, int C, float* record) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float n = 0.f, mu = 0.f, m2 = 0.f;
    for (int k = 0; k < nchunks; ++k) {
        const float nb = (float)(min(M, (k + 1) * chunk) - k * chunk), mb = part[((long)k * 2) * C + c], m2b = part[((long)k * 2 + 1) * C + c];
        const float d = mb - mu, nn = n + nb;
        mu += d * (nb / nn); m2 += m2b + d * d * (n * nb / nn); n = nn;
    }
    if (c == 0) record[0] = (float)M;
    record[1 + c] = mu; record[1 + C + c] = m2;
}

__global__ void pack_sums_kernel(const float* part, int nchunks, int C, float* out, int swap) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float x0 = 0.f, x1 = 0.f;
    for (int k = 0; k < nchunks; ++k) { x0 += part[((long)k * 2) * C + c]; x1 += part[((long)k * 2 + 1) * C + c]; }
    out[(swap ? C : 0) + c] = x0; out[(swap ? 0 : C) + c] = x1;
}

__global__ void merge_stats_kernel(const float* records, int world, int C, float* mean, float* invstd, float* count, float* mov_mean, float* mov_var, int unbiased) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const long stride = 1 + 2L * C;
    float n = 0.f, mu = 0.f, m2 = 0.f;
    for (int r = 0; r < world; ++r) {
        const float* rec = records + r * stride;
        const float nb = rec[0];
        if (!(nb > 0.f)) continue;                            // a rank without a row of this unit adds nothing
        const float d = rec[1 + c] - mu, nn = n + nb;
        mu += d * (nb / nn); m2 += rec[1 + C + c] + d * d * (n * nb / nn); n = nn;
    }
    const float var = m2 / n;
    mean[c] = mu; invstd[c] = 1.f / sqrtf(var + BN_EPS);
    if (c == 0) count[0] = n;
    if (mov_mean) {
        const float vm = (unbiased && n > 1.f) ? var * (n / (n - 1.f)) : var;
        mov_mean[c] -= (mov_mean[c] - mu) * (1.f - BN_MOMENTUM);
        mov_var[c] -= (mov_var[c] - vm) * (1.f - BN_MOMENTUM);
    }
}

__global__ void merge_sums_kernel(const float* records, int world, int n, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x = 0.f;
    for (int r = 0; r < world; ++r) x += records[(long)r * n + i];
    out[i] = x;
}

// one workgroup per range
__global__ void zero_ranges_kernel(float* g, const long* table) {
    const long off = table[2 * blockIdx.x], len = table[2 * blockIdx.x + 1];
    for (long e = threadIdx.x; e < len; e += blockDim.x) g[off + e] = 0.f;
}

}  // namespace

int xchg_pack_stats(const float* part, int nchunks, int chunk, int M, int C, float* record, hipStream_t s) {
    hipLaunchKernelGGL(pack_stats_kernel, dim3(groups_of(C)), dim3(64), 0, s, part, nchunks, chunk, M, C, record);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}
int xchg_pack_sums(const float* part, int nchunks, int C, float* out, int swap, hipStream_t s) {
    hipLaunchKernelGGL(pack_sums_kernel, dim3(groups_of(C)), dim3(64), 0, s, part, nchunks, C, out, swap);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}
int xchg_merge_stats(const float* records, int world, int C, float* mean, float* invstd, float* count, float* mov_mean, float* mov_var, int unbiased, hipStream_t s) {
    hipLaunchKernelGGL(merge_stats_kernel, dim3(groups_of(C)), dim3(64), 0, s, records, world, C, mean, invstd, count, mov_mean, mov_var, unbiased);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}
int xchg_merge_sums(const float* records, int world, int n, float* out, hipStream_t s) {
    hipLaunchKernelGGL(merge_sums_kernel, dim3(groups_of(n)), dim3(64), 0, s, records, world, n, out);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}
int xchg_zero_ranges(float* g, const long* d_table, int n_ranges, hipStream_t s) {
    if (n_ranges <= 0) return SSDR_OK;
    hipLaunchKernelGGL(zero_ranges_kernel, dim3((unsigned)n_ranges), dim3(64), 0, s, g, d_table);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

}  // namespace ssdr

using namespace ssdr;

extern "C" {

int ssdr_bn_stats_merge_dev(const float* d_records, int world, int C, float* d_mean, float* d_invstd, float* d_count, float* d_mov_mean, float* d_mov_var,
                            int unbiased, void* stream) {
    if (!d_records || !d_mean || !d_invstd || !d_count || world < 1 || C < 1 || (d_mov_mean == nullptr) != (d_mov_var == nullptr)) {
        set_error("bn_stats_merge: bad arguments (NULL pointer, world < 1, C < 1, or one moving statistic without the other)"); return SSDR_ERR_INVALID;
    }
    SSDR_TRY(ensure_init());
    return xchg_merge_stats(d_records, world, C, d_mean, d_invstd, d_count, d_mov_mean, d_mov_var, unbiased, pick_stream(stream));
}

int ssdr_rank_sums_merge_dev(const float* d_records, int world, int n, float* d_out, void* stream) {
    if (!d_records || !d_out || world < 1 || n < 1) { set_error("rank_sums_merge: bad arguments (NULL pointer, world < 1 or n < 1)"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    return xchg_merge_sums(d_records, world, n, d_out, pick_stream(stream));
}

}
