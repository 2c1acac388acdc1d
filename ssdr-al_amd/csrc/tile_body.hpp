// Row-level helpers of the tile generator, shared by tile.hip (fixed-size tiles) and predict.hip (whole clouds, num_points = the
// cloud's own row count): the padding map of a small cloud, the gather through the shuffle, and the distance key.
#pragma once
#include "ssdr_internal.hpp"

namespace ssdr {
namespace {

// A cloud smaller than num_points (avail = m < num_points): the entries of perm below avail, in order, shuffle its points; `padmap` holds them compacted
// (padmap[k] = the k-th such entry) so that a row finds its source with one load.  One workgroup of 256 threads per cloud: every thread counts its
// stretch of perm, an exclusive scan of the 256 counts, every thread writes its stretch.  (Until round 6 every ROW scanned perm for its entry: num_points^2
// steps — 13.6 ms of a 22 ms step in the Semantic3D flavour with 65 536-point tiles over rooms of ~50 k points, tools/sem3d_probe.py; S3DIS rooms below
// 40 960 subsampled points take the same path.)
__device__ __forceinline__ void tile_padmap_body(int m, int num_points, const int* __restrict__ perm, int* __restrict__ padmap, unsigned* s_part) {
    const int avail = min(m, num_points), tid = threadIdx.x;
    if (avail == num_points) return;                       // (uniform)
    const int per = (num_points + 255) / 256, q0 = min(tid * per, num_points), q1 = min(q0 + per, num_points);
    unsigned cnt = 0;
    for (int q = q0; q < q1; ++q) cnt += perm[q] < avail ? 1u : 0u;
    __syncthreads();
    s_part[tid] = cnt;
    __syncthreads();
    unsigned incl = cnt;
    for (int o = 1; o < 256; o <<= 1) {
        const unsigned y = tid >= o ? s_part[tid - o] : 0u;
        __syncthreads();
        incl += y; s_part[tid] = incl;
        __syncthreads();
    }
    unsigned at = incl - cnt;
    for (int q = q0; q < q1; ++q) { const int v = perm[q]; if (v < avail) padmap[at++] = v; }
}

// out row r takes sorted position perm[r] when that position exists (< min(m, num_points)); a cloud smaller than
// num_points is padded: rows >= m duplicate point floor(dup_u[r] * m) of the *shuffled* list (data_aug).
__device__ __forceinline__ void tile_gather_body(const float* __restrict__ pts, const float* __restrict__ colors, int cdim,
                                                   const uint32_t* __restrict__ sorted, const int* __restrict__ d_count,
                                                   const int* __restrict__ perm, const float* __restrict__ dup_u, int num_points,
                                                   float cx, float cy, float cz, float color_scale,
                                                   float* out_xyz, float* out_feat, int* out_idx, const int* __restrict__ padmap, int stride = 1, int bx = -1,
                                                   const int* __restrict__ labels = nullptr, int* out_lab = nullptr) {
    const int m = *d_count;
    const int avail = min(m, num_points);
    if (avail <= 0) return;                                // an empty cloud has no row to take or to duplicate (`sorted` holds nothing of this call): its output rows stay as they were
    for (int r = (bx < 0 ? (int)blockIdx.x : bx) * 256 + threadIdx.x; r < num_points; r += gridDim.x * 256) {
        int pos;
        if (avail == num_points) pos = perm[r];
        else {
            // small cloud: perm is a permutation of [0,num_points); its entries < avail, in order, shuffle the avail points (padmap, above):
            // row r < avail takes the r-th of them; row r >= avail duplicates one
            int want = r < avail ? r : (int)(dup_u[r] * (float)avail);
            if (want >= avail) want = avail - 1;
            pos = want >= 0 ? padmap[want] : 0;
        }
        const uint32_t id = sorted[(size_t)pos * stride];        // stride 2: the low words of 64-bit sort words
        const float x = pts[3 * (size_t)id] - cx, y = pts[3 * (size_t)id + 1] - cy, z = pts[3 * (size_t)id + 2] - cz;
        out_xyz[3 * (size_t)r] = x; out_xyz[3 * (size_t)r + 1] = y; out_xyz[3 * (size_t)r + 2] = z;
        if (out_feat) {
            float* f = out_feat + (size_t)r * (3 + cdim);
            f[0] = x; f[1] = y; f[2] = z;
            for (int c = 0; c < cdim; ++c) f[3 + c] = colors[(size_t)id * cdim + c] * color_scale;
        }
        if (out_idx) out_idx[r] = (int)id;
        if (out_lab) out_lab[r] = labels[id];              // queried_pc_label = input_label[queried_idx] (s3dis_dataset.py:141)
    }
}

__device__ __forceinline__ float tile_dist(const float* __restrict__ pts, int i, float cx, float cy, float cz) {
    const float dx = pts[3 * (size_t)i] - cx, dy = pts[3 * (size_t)i + 1] - cy, dz = pts[3 * (size_t)i + 2] - cz;
    // the sign bit cleared: a sum of squares has none, but a NaN coordinate can carry one, and the bins below are indexed by the bit pattern
    // (0xFFC00000 >> 17 lies past the histogram; a positive NaN lands in the last bins like any far point)
    return __uint_as_float(__float_as_uint((dx * dx + dy * dy) + dz * dz) & 0x7fffffffu);
}

}  // namespace
}  // namespace ssdr
