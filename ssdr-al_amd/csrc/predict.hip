// Whole-cloud prediction pass for gfx950: the network pass of the reference's active-learning round over many sub-sampled rooms at once.
//
// Reference: TSampler.prediction() / compute_features() (S3/sampler2.py:580-642, :313-342) run every room WHOLE through the network:
// spatially_regular_gen in mode "sampling" queries k = len(points) (s3dis_dataset.py:129-131), shuffles (:137), pads a room smaller than
// num_points (:147-150), builds the KNN pyramid over the whole cloud (tf_map, :156-183), and reads the outputs back in the room's own point
// order (prob_logits[np.argsort(point_idx[0])], sampler2.py:599; last_second_features likewise, :327).
//
// Nested-prefix packing.  Cloud c has T_c = max(n_c, num_points) tile rows; level l is its first N_c^(l) rows (N^(0) = T_c, N^(l+1) =
// N^(l) // ratio[l], N^(L+1) = 0).  The packed row space holds segment s = L, L-1, .., 0 in that order; segment s holds, cloud by cloud,
// tile rows [N_c^(s+1), N_c^(s)).  The level-l rows of EVERY cloud are then the first P_l = sum_c N_c^(l) packed rows, which is all the
// B = 1 network needs (ssdr_randla_infer_rows_dev): it reads level l as a prefix and pools through the first P_(l+1) rows of neigh_idx[l].
// pos(c, j) = base[c][s] + j with s = max{l : j < N_c^(l)} and base[c][s] = seg_start[s] + (offset of c inside segment s) - N_c^(s+1).
//
// Kernels (all bandwidth-bound glue around the existing tile sort, grid KNN and network):
//   predict_keys         (cloud << 31 | distance bits) per point, the point's index as the value: one stable radix sort orders every cloud
//                        by (distance, index), tile.hip's order, clouds kept apart by the high bits
//   predict_padmap       tile.hip's padding map, per padded cloud
//   predict_gather       tile.hip's gather with num_points = T_c: cloud-major xyz / source index (the KNN's support sets, the read-back's
//                        keys), then the same rows at their packed positions (xyz, features [xyz, rgb * scale], source index, label)
//   predict_translate    cloud-major KNN tables -> packed rows, every index value mapped through pos(c, .): neigh [P_l][16], interp [P_l]
//   predict_rb_scatter   per output point: the packed row it reads.  Rows [0, n) of every tile hold each point once: a scatter through the
//                        source index gives "point" (each point's first row) everywhere and "reference" for unpadded clouds
//   predict_rb_keys      "reference" on padded clouds: (cloud << kb | source index) words, row as value; the stable radix sort orders them
//   predict_rb_sorted    ... and the p-th smallest key's row becomes point p's (argsort(point_idx)[p], stable)
//   predict_rb_gather    probs / feat32 rows -> cloud order
// The Semantic3D flavour (whole scans, never padded, cut into parts by split3; further down):
//   scan_keys            distance bits per point of one scan, the stable radix sort orders them by (distance, index)
//   scan_gather          tile.hip's gather without the padding branch: t_xyz, t_idx, t_feat = [xyz, rgb * scale] in tile-row order
//   parts_gather         the parts of a chunk as ragged clouds: part-major xyz, then xyz / features / source point / label at their packed positions
//   predict_scatter      total[point_idx] = out: packed probs / feat32 rows -> the points they belong to, one writer per row
#include "ssdr_internal.hpp"
#include "tile_body.hpp"
#include <cmath>
#include <cstring>
#include <vector>

namespace ssdr {
namespace {

// per-cloud table (int32, row width tab_w(L)): n, T, row offset (sum of T before), point offset (sum of n before), N^(0..L+1), base[0..L],
// cloud-major offset of the cloud inside each KNN level's block [0..L-1]
constexpr int PT_N = 0, PT_T = 1, PT_ROW = 2, PT_PT = 3, PT_LIM = 4;
__host__ __device__ inline int tab_w(int L) { return PT_LIM + (L + 2) + (L + 1) + L; }
__host__ __device__ inline int pt_base(int L) { return PT_LIM + L + 2; }
__host__ __device__ inline int pt_cmo(int L) { return PT_LIM + L + 2 + L + 1; }

__device__ __forceinline__ int packed_pos(const int* __restrict__ t, int L, int j) {
    int s = 0;
    while (s < L && j < t[PT_LIM + s + 1]) ++s;        // s = max{l : j < N^(l)} (j < N^(0) always; most rows stop at the first test)
    return t[pt_base(L) + s] + j;
}

struct Pack {
    int nc = 0, L = 0;
    std::vector<int> tab;           // [nc][tab_w(L)]
    std::vector<long> P;            // P_l, l = 0..L
    std::vector<long> R;            // first row of level l's block in the KNN / translation layout, l = 0..L (R_L = total rows)
    long rows = 0, points = 0;
    int max_t = 0, max_n = 0, padded = 0;
};

// validates the chunk and lays it out; the refusals every entry point of this file shares
int make_pack(const char* who, const int64_t* cloud_offsets, size_t num_clouds, size_t num_points, size_t num_layers, const int32_t* ratios, Pack& p) {
    if (!cloud_offsets || !ratios || num_clouds == 0 || num_points == 0 || num_layers == 0 || num_layers > 16) { set_error("%s: bad arguments", who); return SSDR_ERR_INVALID; }
    if (num_clouds > 4096) { set_error("%s: %zu clouds in one call (at most 4096)", who, num_clouds); return SSDR_ERR_UNSUPPORTED; }
    const int L = (int)num_layers, nc = (int)num_clouds, W = tab_w(L);
    for (int l = 0; l < L; ++l) if (ratios[l] <= 0) { set_error("%s: ratio must be positive", who); return SSDR_ERR_INVALID; }
    p.nc = nc; p.L = L; p.tab.assign((size_t)nc * W, 0); p.P.assign(L + 1, 0); p.R.assign(L + 1, 0);
    p.rows = 0; p.points = 0; p.max_t = 0; p.max_n = 0; p.padded = 0;
    std::vector<long> lim((size_t)nc * (L + 2));
    for (int c = 0; c < nc; ++c) {
        const long n = (long)(cloud_offsets[c + 1] - cloud_offsets[c]);
        if (n <= 0) { set_error("%s: cloud %d is empty (every cloud needs at least one point)", who, c); return SSDR_ERR_INVALID; }
        const long T = std::max(n, (long)num_points);
        if (p.rows + T > SSDR_PREDICT_MAX_ROWS) {
            set_error("%s: %ld level-0 rows in one call (cap %d = 2^23: the network's int32 element offsets)", who, p.rows + T, SSDR_PREDICT_MAX_ROWS);
            return SSDR_ERR_UNSUPPORTED;
        }
        int* t = &p.tab[(size_t)c * W];
        t[PT_N] = (int)n; t[PT_T] = (int)T; t[PT_ROW] = (int)p.rows; t[PT_PT] = (int)p.points;
        long* lc = &lim[(size_t)c * (L + 2)];
        lc[0] = T;
        for (int l = 0; l < L; ++l) lc[l + 1] = lc[l] / ratios[l];
        lc[L + 1] = 0;
        if (lc[L] <= 0) { set_error("%s: cloud %d (%ld rows) is too small for the pyramid", who, c, T); return SSDR_ERR_INVALID; }
        for (int l = 0; l <= L + 1; ++l) t[PT_LIM + l] = (int)lc[l];
        for (int l = 0; l <= L; ++l) p.P[l] += lc[l];
        p.rows += T; p.points += n; p.max_t = std::max(p.max_t, (int)T); p.max_n = std::max(p.max_n, (int)n); p.padded += T > n;
    }
    // segments deepest first: segment s holds rows [N^(s+1), N^(s)) of every cloud in turn
    long at = 0;
    for (int s = L; s >= 0; --s)
        for (int c = 0; c < nc; ++c) {
            const long* lc = &lim[(size_t)c * (L + 2)];
            p.tab[(size_t)c * W + pt_base(L) + s] = (int)(at - lc[s + 1]);
            at += lc[s] - lc[s + 1];
        }
    // the KNN levels' blocks: level l's rows of cloud 0, cloud 1, ... starting at R_l
    long r = 0;
    for (int l = 0; l < L; ++l) {
        p.R[l] = r;
        for (int c = 0; c < nc; ++c) { p.tab[(size_t)c * W + pt_cmo(L) + l] = (int)(r - p.R[l]); r += lim[(size_t)c * (L + 2) + l]; }
    }
    p.R[L] = r;
    return SSDR_OK;
}

// one staging ring per entry point: a ring slot is reused SLOTS calls later, after waiting for its copy to have executed, so with one ring
// per entry a caller can keep SLOTS chunks in flight on a stream before the host waits for the device
enum { STG_TILE, STG_TRANSLATE, STG_READBACK, STG_PARTS };
struct PredictState { DevBuf tab, keys, vals, padmap, rb_rows; RadixSorter sorter; StagingRing<int> staging[4]; };
PredictState& pst(hipStream_t s) { return per_stream<PredictState>(s); }

int upload_tab(PredictState& S, const Pack& p, hipStream_t s, int which) {
    SSDR_TRY(S.tab.reserve(4 * p.tab.size()));
    int* st = nullptr;
    StagingRing<int>& ring = S.staging[which];
    const int slot = ring.acquire(p.tab.size(), &st);
    if (slot < 0) { set_error("predict: pinned staging buffer"); return SSDR_ERR_HIP; }
    memcpy(st, p.tab.data(), 4 * p.tab.size());
    SSDR_HIP(hipMemcpyAsync(S.tab.p, st, 4 * p.tab.size(), hipMemcpyHostToDevice, s));
    if (ring.release(slot, s)) { set_error("predict: staging event"); return SSDR_ERR_HIP; }
    return SSDR_OK;
}

// ---- tile ---------------------------------------------------------------------------------------------------------------------------

// blockIdx.y = cloud: word (cloud << 31 | distance bits) at the point's slot, the point's index inside its cloud as the value
__global__ __launch_bounds__(256) void predict_keys(const int* __restrict__ tab, int W, const float* __restrict__ pts, const float* __restrict__ centers,
                                                    uint64_t* keys, uint32_t* vals) {
    const int c = blockIdx.y;
    const int* t = tab + (size_t)c * W;
    const int n = t[PT_N], o = t[PT_PT];
    const float cx = centers[3 * c], cy = centers[3 * c + 1], cz = centers[3 * c + 2];
    const float* P = pts + 3 * (size_t)o;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        keys[o + i] = ((uint64_t)c << 31) | (uint64_t)__float_as_uint(tile_dist(P, i, cx, cy, cz));
        vals[o + i] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(256) void predict_padmap(const int* __restrict__ tab, int W, const int* __restrict__ perm, int* padmap) {
    __shared__ unsigned s_part[256];
    const int* t = tab + (size_t)blockIdx.x * W;
    tile_padmap_body(t[PT_N], t[PT_T], perm + t[PT_ROW], padmap + t[PT_ROW], s_part);
}

__global__ __launch_bounds__(256) void predict_gather(const int* __restrict__ tab, int W, int L, const float* __restrict__ pts, const float* __restrict__ colors,
                                                      const int* __restrict__ labels, const uint32_t* __restrict__ sorted, const float* __restrict__ centers,
                                                      const int* __restrict__ perm, const float* __restrict__ dup_u, const int* __restrict__ padmap, float color_scale,
                                                      float* cm_xyz, int* cm_idx, float* pk_xyz, float* pk_feat, int* pk_src, int* pk_lab) {
    const int c = blockIdx.y;
    const int* t = tab + (size_t)c * W;
    const int T = t[PT_T], ro = t[PT_ROW], o = t[PT_PT];
    const float cx = centers[3 * c], cy = centers[3 * c + 1], cz = centers[3 * c + 2];
    // tile.hip's rule with num_points = T (t[PT_N] is the cloud's point count, the gather's d_count)
    tile_gather_body(pts + 3 * (size_t)o, nullptr, 0, sorted + o, t + PT_N, perm + ro, dup_u + ro, T, cx, cy, cz, 0.f,
                     cm_xyz + 3 * (size_t)ro, nullptr, cm_idx + ro, padmap + ro);
    // the same rows (this thread wrote them) once more at their packed positions
    for (int r = blockIdx.x * 256 + threadIdx.x; r < T; r += gridDim.x * 256) {
        const size_t q = (size_t)ro + r, p = (size_t)packed_pos(t, L, r);
        const int id = cm_idx[q];
        const float x = cm_xyz[3 * q], y = cm_xyz[3 * q + 1], z = cm_xyz[3 * q + 2];
        pk_xyz[3 * p] = x; pk_xyz[3 * p + 1] = y; pk_xyz[3 * p + 2] = z;
        float* f = pk_feat + 6 * p;
        const float* col = colors + 3 * ((size_t)o + id);
        f[0] = x; f[1] = y; f[2] = z; f[3] = col[0] * color_scale; f[4] = col[1] * color_scale; f[5] = col[2] * color_scale;
        if (pk_src) pk_src[p] = id;
        if (pk_lab) pk_lab[p] = labels[(size_t)o + id];
    }
}

// ---- index translation --------------------------------------------------------------------------------------------------------------

// Workgroups are dealt out to the (level, cloud) blocks of the KNN layout in proportion to their rows: block k (= level * nc + cloud) owns
// workgroups [wg[k], wg[k+1]), TR_ROWS rows each, and a workgroup finds its block by one binary search (uniform: scalar loads).  bs[k] is
// the block's first row.  16 lanes per row: one neighbour each (coalesced 64-byte rows in and out), lane 0 also the up-sampling index.
constexpr int TR_ROWS = 64;
__global__ __launch_bounds__(256) void predict_translate(const int* __restrict__ tab, int W, int L, int nc, const int* __restrict__ bs,
                                                         const int* __restrict__ wg, const int* __restrict__ cm_neigh, const int* __restrict__ cm_interp,
                                                         int* pk_neigh, int* pk_interp) {
    const int b = (int)blockIdx.x;
    int lo = 0, hi = nc * L - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (wg[mid] <= b) lo = mid; else hi = mid - 1; }
    const int l = lo / nc, c = lo - l * nc;
    const int* t = tab + (size_t)c * W;
    const int n = t[PT_LIM + l], j0 = (b - wg[lo]) * TR_ROWS, lane = threadIdx.x & 15;
    const size_t src0 = (size_t)bs[lo], dst0 = (size_t)bs[l * nc];      // bs[l * nc] = R_l, the level's first row
    for (int q = threadIdx.x >> 4; q < TR_ROWS; q += 16) {
        const int j = j0 + q;
        if (j >= n) break;
        const size_t src = src0 + j, dst = dst0 + packed_pos(t, L, j);
        pk_neigh[16 * dst + lane] = packed_pos(t, L, cm_neigh[16 * src + lane]);
        if (lane == 0) pk_interp[dst] = packed_pos(t, L, cm_interp[src]);
    }
}

// ---- read-back ------------------------------------------------------------------------------------------------------------------------

// rows[point] = the packed row whose outputs the point receives.  Rows [0, n) of a cloud's tile hold every point once (a padded cloud's
// duplicates come after them), so rows[key[j]] = pos(j) over j < n is "point" for every cloud and "reference" for an unpadded one.
// blockIdx.y = cloud.
__global__ __launch_bounds__(256) void predict_rb_scatter(const int* __restrict__ tab, int W, int L, const int* __restrict__ cm_idx, int* rows) {
    const int* t = tab + (size_t)blockIdx.y * W;
    const int n = t[PT_N], ro = t[PT_ROW], o = t[PT_PT];
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) rows[o + cm_idx[ro + j]] = packed_pos(t, L, j);
}
// "reference" on a padded cloud (T = num_points rows, duplicated keys): the stable order of its keys, by the radix sorter over all padded
// clouds at once.  blockIdx.y = padded cloud k: word (k << kb | key), value = row
__global__ __launch_bounds__(256) void predict_rb_keys(const int* __restrict__ tab, int W, const int* __restrict__ padded, const int* __restrict__ cm_idx,
                                                       int kb, uint64_t* keys, uint32_t* vals) {
    const int k = blockIdx.y;
    const int* t = tab + (size_t)padded[k] * W;
    const int T = t[PT_T], ro = t[PT_ROW];
    for (int j = blockIdx.x * 256 + threadIdx.x; j < T; j += gridDim.x * 256) {
        keys[(size_t)k * T + j] = ((uint64_t)k << kb) | (uint64_t)(uint32_t)cm_idx[ro + j];
        vals[(size_t)k * T + j] = (uint32_t)j;
    }
}
// out[p] = tile_out[argsort(point_idx)[p]] (sampler2.py:599): the p-th smallest key's row, p < n
__global__ __launch_bounds__(256) void predict_rb_sorted(const int* __restrict__ tab, int W, int L, const int* __restrict__ padded, const uint32_t* __restrict__ vals,
                                                         int* rows) {
    const int k = blockIdx.y;
    const int* t = tab + (size_t)padded[k] * W;
    const int n = t[PT_N], T = t[PT_T], o = t[PT_PT];
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) rows[o + p] = packed_pos(t, L, (int)vals[(size_t)k * T + p]);
}

// one thread per output element: probs [P][C] and feat32 [P][32] rows -> cloud order
__global__ __launch_bounds__(256) void predict_rb_gather(const int* __restrict__ rows, long npts, const float* __restrict__ pk_probs, int C,
                                                         const float* __restrict__ pk_feat, float* probs, float* feat) {
    const long w = C + 32, total = npts * w;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long p = e / w; const int ch = (int)(e - p * w);
        const size_t r = (size_t)rows[p];
        if (ch < C) probs[(size_t)p * C + ch] = pk_probs[r * C + ch];
        else feat[(size_t)p * 32 + (ch - C)] = pk_feat[r * 32 + (ch - C)];
    }
}

// ---- Semantic3D flavour: a whole scan, never padded, cut into parts that run as ragged clouds -------------------------------------------
// Reference: Semantic3D_Dataset_Sampling in mode "sampling" (semantic3d_dataset_sampling.py:114-155: query(k = len(points)), shuffle, centre on
// all three axes), tf_map's split3 + merge (:198-294: one pyramid and one network call per part) and total[point_idx[0]] = out
// (sampler2.py:344, :629).  The tile of a scan is tile.hip's rule with num_points = n and no padding; a part is a "cloud" of the packing
// above with num_points = 1 (T = its rows), so the pyramid, the translation and the network run as they do for whole rooms.

// word = the distance bits (31: tile_dist clears the sign), value = the point: the stable sort gives (distance, index) order
__global__ __launch_bounds__(256) void scan_keys(int n, const float* __restrict__ pts, float cx, float cy, float cz, uint64_t* keys, uint32_t* vals) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        keys[i] = (uint64_t)__float_as_uint(tile_dist(pts, i, cx, cy, cz));
        vals[i] = (uint32_t)i;
    }
}

// tile_gather_body's unpadded branch: row r takes sorted position perm[r]; features [xyz, rgb * scale] (ssdr_feed_augment_dev rewrites columns 0..2)
__global__ __launch_bounds__(256) void scan_gather(int n, const float* __restrict__ pts, const float* __restrict__ colors, const uint32_t* __restrict__ sorted,
                                                   const int* __restrict__ perm, float cx, float cy, float cz, float color_scale,
                                                   float* t_xyz, float* t_feat, int* t_idx) {
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
        const int pos = min(max(perm[r], 0), n - 1);                   // a permutation of [0, n) by contract: never read past the scan
        const size_t id = sorted[pos];
        const float x = pts[3 * id] - cx, y = pts[3 * id + 1] - cy, z = pts[3 * id + 2] - cz;
        t_xyz[3 * (size_t)r] = x; t_xyz[3 * (size_t)r + 1] = y; t_xyz[3 * (size_t)r + 2] = z;
        float2* f = reinterpret_cast<float2*>(t_feat + 6 * (size_t)r);          // 24-byte rows: three 8-byte stores
        f[0] = make_float2(x, y);
        f[1] = make_float2(z, colors[3 * id] * color_scale);
        f[2] = make_float2(colors[3 * id + 1] * color_scale, colors[3 * id + 2] * color_scale);
        t_idx[r] = (int)id;
    }
}

// blockIdx.y = part, one work-item per row.  order[ro + j] is the scan-local tile row of the part's j-th row (ascending inside a part: the
// reads walk forward through the scan's tile, the part-major writes are contiguous, the packed ones contiguous per segment).
__global__ __launch_bounds__(256) void parts_gather(const int* __restrict__ tab, int W, int L, const int* __restrict__ base, const float* __restrict__ t_xyz,
                                                    const float* __restrict__ t_feat, const int* __restrict__ t_idx, const int* __restrict__ labels,
                                                    const int* __restrict__ order, float* cm_xyz, float* pk_xyz, float* pk_feat, int* pk_src, int* pk_lab) {
    const int c = blockIdx.y;
    const int* t = tab + (size_t)c * W;
    const int n = t[PT_N], ro = t[PT_ROW], b = base[c];
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        const size_t q = (size_t)ro + j, row = (size_t)b + order[q], p = (size_t)packed_pos(t, L, j);
        const float x = t_xyz[3 * row], y = t_xyz[3 * row + 1], z = t_xyz[3 * row + 2];
        cm_xyz[3 * q] = x; cm_xyz[3 * q + 1] = y; cm_xyz[3 * q + 2] = z;
        pk_xyz[3 * p] = x; pk_xyz[3 * p + 1] = y; pk_xyz[3 * p + 2] = z;
        const float2* fi = reinterpret_cast<const float2*>(t_feat + 6 * row);
        float2* fo = reinterpret_cast<float2*>(pk_feat + 6 * p);
        fo[0] = fi[0]; fo[1] = fi[1]; fo[2] = fi[2];
        const int src = b + t_idx[row];
        pk_src[p] = src;
        if (pk_lab) pk_lab[p] = labels[src];
    }
}

// total[point_idx] = out: eight lanes per packed row, a 16-byte piece of the 128-byte feature row each and every eighth class of the
// probabilities.  Every point lies in exactly one part, so every output row has one writer.  A source outside [0, num_out) writes nothing.
__global__ __launch_bounds__(256) void predict_scatter(const int* __restrict__ src, long rows, long num_out, const float* __restrict__ pk_probs, int C,
                                                       const float* __restrict__ pk_feat, float* probs, float* feat) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < rows * 8; e += (long)gridDim.x * 256) {
        const long r = e >> 3; const int lane = (int)(e & 7);
        const long d = src[r];
        if (d < 0 || d >= num_out) continue;
        reinterpret_cast<float4*>(feat)[d * 8 + lane] = reinterpret_cast<const float4*>(pk_feat)[r * 8 + lane];
        for (int ch = lane; ch < C; ch += 8) probs[d * C + ch] = pk_probs[r * C + ch];
    }
}

}  // namespace
}  // namespace ssdr

using namespace ssdr;

extern "C" {

int ssdr_predict_layout(const int64_t* cloud_offsets, size_t num_clouds, size_t num_points, size_t num_layers, const int32_t* ratios,
                        int64_t* level_rows) {
    Pack p;
    SSDR_TRY(make_pack("predict_layout", cloud_offsets, num_clouds, num_points, num_layers, ratios, p));
    if (level_rows) for (size_t l = 0; l <= num_layers; ++l) level_rows[l] = p.P[l];
    return SSDR_OK;
}

int ssdr_predict_tile_dev(const float* d_points, const float* d_colors, const int32_t* d_labels, const int64_t* cloud_offsets, size_t num_clouds,
                          const float* centers, size_t num_points, size_t num_layers, const int32_t* ratios, const int32_t* d_perm, const float* d_dup_u,
                          float color_scale, float* d_cm_xyz, int32_t* d_cm_idx, float* d_pk_xyz, float* d_pk_feat, int32_t* d_pk_src,
                          int32_t* d_pk_labels, void* stream) {
    if (!d_points || !d_colors || !centers || !d_perm || !d_dup_u || !d_cm_xyz || !d_cm_idx || !d_pk_xyz || !d_pk_feat || (d_pk_labels && !d_labels)) {
        set_error("predict_tile: bad arguments"); return SSDR_ERR_INVALID;
    }
    Pack p;
    SSDR_TRY(make_pack("predict_tile", cloud_offsets, num_clouds, num_points, num_layers, ratios, p));
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); PredictState& S = pst(s);
    const int W = tab_w(p.L), nc = p.nc, L = p.L;
    // the centres ride behind the cloud table (float bits)
    for (int i = 0; i < 3 * nc; ++i) { int v; memcpy(&v, centers + i, 4); p.tab.push_back(v); }
    SSDR_TRY(upload_tab(S, p, s, STG_TILE));
    const size_t npts = (size_t)p.points;
    SSDR_TRY(S.keys.reserve(8 * npts + 16)); SSDR_TRY(S.vals.reserve(4 * npts + 16)); SSDR_TRY(S.padmap.reserve(4 * (size_t)p.rows + 16));
    int cb = 0; while ((1 << cb) < nc) ++cb;
    const int* tab = S.tab.as<int>();
    const float* cen = reinterpret_cast<const float*>(tab + (size_t)nc * W);
    {
        ProfScope prof("predict_tile_keys", s, 16.0 * (double)npts);
        hipLaunchKernelGGL(predict_keys, dim3(std::max(1, std::min((p.max_n + 255) / 256, 64)), nc), dim3(256), 0, s, tab, W, d_points, cen,
                           S.keys.as<uint64_t>(), S.vals.as<uint32_t>());
    }
    S.sorter.wide_high = true;
    // one segment: the cloud bits above the distance keep the clouds apart, the stable sort keeps (distance, index) order inside each
    const int off[2] = {0, (int)((npts + RADIX_TILE - 1) / RADIX_TILE * RADIX_TILE)}, nh = (int)npts;
    SSDR_TRY(S.sorter.sort_segments(S.keys.as<uint64_t>(), S.vals.as<uint32_t>(), 1, off, &nh, nullptr, s, 31 + cb));
    if (p.padded) hipLaunchKernelGGL(predict_padmap, dim3(nc), dim3(256), 0, s, tab, W, d_perm, S.padmap.as<int>());
    {
        ProfScope prof("predict_tile_gather", s, (double)p.rows * (4 + 4 + 4 + 12 + 12 + 12 + 4 + 12 + 12 + 24 + (d_pk_src ? 4 : 0) + (d_pk_labels ? 8 : 0)));
        hipLaunchKernelGGL(predict_gather, dim3(std::max(1, std::min((p.max_t + 255) / 256, 256)), nc), dim3(256), 0, s, tab, W, L, d_points, d_colors, d_labels,
                           S.vals.as<uint32_t>(), cen, d_perm, d_dup_u, S.padmap.as<int>(), color_scale, d_cm_xyz, d_cm_idx, d_pk_xyz, d_pk_feat, d_pk_src, d_pk_labels);
    }
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_predict_translate_dev(const int64_t* cloud_offsets, size_t num_clouds, size_t num_points, size_t num_layers, const int32_t* ratios, size_t K,
                               const int32_t* d_cm_neigh, const int32_t* d_cm_interp, int32_t* d_pk_neigh, int32_t* d_pk_interp, void* stream) {
    if (K != 16) { set_error("predict_translate: K = %zu (the pyramid's K = 16 only)", K); return SSDR_ERR_UNSUPPORTED; }
    if (!d_cm_neigh || !d_cm_interp || !d_pk_neigh || !d_pk_interp) { set_error("predict_translate: bad arguments"); return SSDR_ERR_INVALID; }
    Pack p;
    SSDR_TRY(make_pack("predict_translate", cloud_offsets, num_clouds, num_points, num_layers, ratios, p));
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); PredictState& S = pst(s);
    // behind the cloud table: the blocks' first rows, then their first workgroups (and the total)
    const int W = tab_w(p.L), nb = p.nc * p.L;
    for (int l = 0; l < p.L; ++l)
        for (int c = 0; c < p.nc; ++c) p.tab.push_back((int)p.R[l] + p.tab[(size_t)c * W + pt_cmo(p.L) + l]);
    int nwg = 0;
    for (int l = 0; l < p.L; ++l)
        for (int c = 0; c < p.nc; ++c) { p.tab.push_back(nwg); nwg += (p.tab[(size_t)c * W + PT_LIM + l] + TR_ROWS - 1) / TR_ROWS; }
    p.tab.push_back(nwg);
    SSDR_TRY(upload_tab(S, p, s, STG_TRANSLATE));
    const int* tab = S.tab.as<int>();
    ProfScope prof("predict_translate", s, 2.0 * 17.0 * 4.0 * (double)p.R[p.L]);
    hipLaunchKernelGGL(predict_translate, dim3(nwg), dim3(256), 0, s, tab, W, p.L, p.nc, tab + (size_t)p.nc * W, tab + (size_t)p.nc * W + nb,
                       d_cm_neigh, d_cm_interp, d_pk_neigh, d_pk_interp);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_predict_readback_dev(const int64_t* cloud_offsets, size_t num_clouds, size_t num_points, size_t num_layers, const int32_t* ratios,
                              const int32_t* d_cm_idx, const float* d_pk_probs, size_t num_classes, const float* d_pk_feat32, int mode,
                              float* d_probs, float* d_feat32, void* stream) {
    if (mode != 0 && mode != 1) { set_error("predict_readback: mode %d (0 = reference, 1 = point)", mode); return SSDR_ERR_INVALID; }
    if (!d_cm_idx || !d_pk_probs || !d_pk_feat32 || !d_probs || !d_feat32 || num_classes == 0 || num_classes > 1024) { set_error("predict_readback: bad arguments"); return SSDR_ERR_INVALID; }
    Pack p;
    SSDR_TRY(make_pack("predict_readback", cloud_offsets, num_clouds, num_points, num_layers, ratios, p));
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); PredictState& S = pst(s);
    // the padded clouds ride behind the cloud table
    std::vector<int> padded;
    for (int c = 0; c < p.nc; ++c) if (p.tab[(size_t)c * tab_w(p.L) + PT_T] > p.tab[(size_t)c * tab_w(p.L) + PT_N]) padded.push_back(c);
    const bool sorted = mode == 0 && !padded.empty();
    if (sorted) p.tab.insert(p.tab.end(), padded.begin(), padded.end());
    SSDR_TRY(upload_tab(S, p, s, STG_READBACK));
    SSDR_TRY(S.rb_rows.reserve(4 * (size_t)p.points + 16));
    const int W = tab_w(p.L);
    const int* tab = S.tab.as<int>();
    {
        ProfScope prof("predict_rb_scatter", s, 12.0 * (double)p.points);
        hipLaunchKernelGGL(predict_rb_scatter, dim3(std::max(1, std::min((p.max_n + 255) / 256, 256)), p.nc), dim3(256), 0, s, tab, W, p.L, d_cm_idx,
                           S.rb_rows.as<int>());
    }
    if (sorted) {
        const int np = (int)padded.size(), T = (int)num_points;
        const size_t slots = (size_t)np * T;
        int kb = 1; while ((1 << kb) < T) ++kb;
        int cb = 0; while ((1 << cb) < np) ++cb;
        SSDR_TRY(S.keys.reserve(8 * slots + 16)); SSDR_TRY(S.vals.reserve(4 * slots + 16));
        const int* pad = tab + (size_t)p.nc * W;
        const dim3 g(std::max(1, std::min((T + 255) / 256, 64)), np);
        hipLaunchKernelGGL(predict_rb_keys, g, dim3(256), 0, s, tab, W, pad, d_cm_idx, kb, S.keys.as<uint64_t>(), S.vals.as<uint32_t>());
        S.sorter.wide_high = true;
        const int off[2] = {0, (int)((slots + RADIX_TILE - 1) / RADIX_TILE * RADIX_TILE)}, nh = (int)slots;
        SSDR_TRY(S.sorter.sort_segments(S.keys.as<uint64_t>(), S.vals.as<uint32_t>(), 1, off, &nh, nullptr, s, kb + cb));
        hipLaunchKernelGGL(predict_rb_sorted, g, dim3(256), 0, s, tab, W, p.L, pad, S.vals.as<uint32_t>(), S.rb_rows.as<int>());
    }
    {
        const double el = (double)p.points * (double)(num_classes + 32);
        ProfScope prof("predict_rb_gather", s, 8.0 * el + 4.0 * (double)p.points);
        const int g = (int)std::max(1.0, std::min(std::ceil(el / 256.0), (double)ctx().num_cu * 16));
        hipLaunchKernelGGL(predict_rb_gather, dim3(g), dim3(256), 0, s, S.rb_rows.as<int>(), (long)p.points, d_pk_probs, (int)num_classes, d_pk_feat32, d_probs, d_feat32);
    }
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_predict_scan_tile_dev(const float* d_points, const float* d_colors, size_t n, const float* center, const int32_t* d_perm, float color_scale,
                               float* d_t_xyz, float* d_t_feat, int32_t* d_t_idx, void* stream) {
    if (!d_points || !d_colors || !center || !d_perm || !d_t_xyz || !d_t_feat || !d_t_idx || ((uintptr_t)d_t_feat & 7)) {
        set_error("predict_scan_tile: bad arguments"); return SSDR_ERR_INVALID;
    }
    if (n == 0) { set_error("predict_scan_tile: the scan is empty (every scan needs at least one point)"); return SSDR_ERR_INVALID; }
    if (n > 0x3fffffffull) { set_error("predict_scan_tile: %zu points in one scan (at most 0x3fffffff)", n); return SSDR_ERR_UNSUPPORTED; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); PredictState& S = pst(s);
    SSDR_TRY(S.keys.reserve(8 * n + 16)); SSDR_TRY(S.vals.reserve(4 * n + 16));
    const int g = (int)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, (size_t)ctx().num_cu * 16));
    {
        ProfScope prof("predict_scan_keys", s, 24.0 * (double)n);
        hipLaunchKernelGGL(scan_keys, dim3(g), dim3(256), 0, s, (int)n, d_points, center[0], center[1], center[2], S.keys.as<uint64_t>(), S.vals.as<uint32_t>());
    }
    S.sorter.wide_high = true;
    const int off[2] = {0, (int)((n + RADIX_TILE - 1) / RADIX_TILE * RADIX_TILE)}, nh = (int)n;
    SSDR_TRY(S.sorter.sort_segments(S.keys.as<uint64_t>(), S.vals.as<uint32_t>(), 1, off, &nh, nullptr, s, 31));
    {
        ProfScope prof("predict_scan_gather", s, (double)n * (4 + 4 + 12 + 12 + 12 + 24 + 4));
        hipLaunchKernelGGL(scan_gather, dim3(g), dim3(256), 0, s, (int)n, d_points, d_colors, S.vals.as<uint32_t>(), d_perm, center[0], center[1], center[2],
                           color_scale, d_t_xyz, d_t_feat, d_t_idx);
    }
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_predict_parts_dev(const float* d_t_xyz, const float* d_t_feat, const int32_t* d_t_idx, const int32_t* d_labels, const int32_t* d_order,
                           const int64_t* part_offsets, const int64_t* part_base, size_t num_parts, size_t num_layers, const int32_t* ratios,
                           float* d_cm_xyz, float* d_pk_xyz, float* d_pk_feat, int32_t* d_pk_src, int32_t* d_pk_labels, void* stream) {
    if (!d_t_xyz || !d_t_feat || !d_t_idx || !d_order || !part_base || !d_cm_xyz || !d_pk_xyz || !d_pk_feat || !d_pk_src || (d_pk_labels && !d_labels) ||
        ((uintptr_t)d_t_feat & 7) || ((uintptr_t)d_pk_feat & 7)) {
        set_error("predict_parts: bad arguments"); return SSDR_ERR_INVALID;
    }
    Pack p;
    SSDR_TRY(make_pack("predict_parts", part_offsets, num_parts, 1, num_layers, ratios, p));
    for (int c = 0; c < p.nc; ++c)
        if (part_base[c] < 0 || part_base[c] > 0x7fffffffLL - 0x40000000LL) { set_error("predict_parts: part %d: its scan starts at point %lld (int32 sources)", c, (long long)part_base[c]); return SSDR_ERR_UNSUPPORTED; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); PredictState& S = pst(s);
    const int W = tab_w(p.L), nc = p.nc;
    for (int c = 0; c < nc; ++c) p.tab.push_back((int)part_base[c]);        // the scans' first rows ride behind the part table
    SSDR_TRY(upload_tab(S, p, s, STG_PARTS));
    const int* tab = S.tab.as<int>();
    ProfScope prof("predict_parts_gather", s, (double)p.rows * (4 + 12 + 24 + 4 + 12 + 12 + 24 + 4 + (d_pk_labels ? 8 : 0)));
    hipLaunchKernelGGL(parts_gather, dim3(std::max(1, std::min((p.max_t + 255) / 256, 256)), nc), dim3(256), 0, s, tab, W, p.L, tab + (size_t)nc * W, d_t_xyz, d_t_feat,
                       d_t_idx, d_labels, d_order + part_offsets[0], d_cm_xyz, d_pk_xyz, d_pk_feat, d_pk_src, d_pk_labels);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_predict_scatter_dev(const int32_t* d_pk_src, size_t num_rows, const float* d_pk_probs, size_t num_classes, const float* d_pk_feat32,
                             size_t num_out, float* d_probs, float* d_feat32, void* stream) {
    if (!d_pk_src || !d_pk_probs || !d_pk_feat32 || !d_probs || !d_feat32 || num_rows == 0 || num_classes == 0 || num_classes > 1024 ||
        ((uintptr_t)d_pk_feat32 & 15) || ((uintptr_t)d_feat32 & 15)) {
        set_error("predict_scatter: bad arguments"); return SSDR_ERR_INVALID;
    }
    if (num_rows > SSDR_PREDICT_MAX_ROWS) { set_error("predict_scatter: %zu packed rows (cap %d = 2^23)", num_rows, SSDR_PREDICT_MAX_ROWS); return SSDR_ERR_UNSUPPORTED; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    ProfScope prof("predict_scatter", s, (double)num_rows * (4.0 + 8.0 * (double)(num_classes + 32)));
    const int g = (int)std::max<size_t>(1, std::min<size_t>((num_rows * 8 + 255) / 256, (size_t)ctx().num_cu * 16));
    hipLaunchKernelGGL(predict_scatter, dim3(g), dim3(256), 0, s, d_pk_src, (long)num_rows, (long)num_out, d_pk_probs, (int)num_classes, d_pk_feat32, d_probs, d_feat32);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

}
