// Test-time generator chain for gfx950: get_batch of the test datasets (S3/s3dis_dataset_test.py:97-151, the Semantic3D flavour's
// semantic3d_dataset_test3.py:129-193) with the cloud and the centre of every tile chosen on the device.
//
// Reference, per tile: the cloud with the smallest min_possibility (:106), its arg-min point (:108) plus noise as the centre (:112-115), the
// num_points nearest rows (:117-122), shuffled (:125), centred (:127-128), possibility[queried] += (1 - d / max d)^2 (:132-134), the cloud's
// new minimum (:135), data_aug padding for a small cloud (:137-141).  Tile t + 1 reads what tile t wrote, so the tiles of a batch are a chain;
// here the whole chain is enqueued at once and no value comes back to the host.
//
// Launches per tile (VOTE_LAUNCHES), all plain launches in stream order, grids sized by the LARGEST cloud (the chosen one is known on the
// device only; workgroups past its rows leave at once):
//   vote_pick      one workgroup: finishes the previous tile's minimum (stage 2 over the partials of vote_min_part), then first arg-min
//                  over cloud_min, the centre, and the record {cloud, base, m, centre} every later kernel reads
//   vote_hist      histogram of the top TS_BITS bits of the float32 distance pattern (LDS, then one global add per non-empty bin)
//   vote_thresh    one workgroup: the first bin whose cumulative count reaches min(num_points, m), the bins' write cursors, the sort ranges,
//                  the padding map of a cloud smaller than the tile
//   vote_compact   rows with bin <= threshold to their range's slots as (distance bits << 32 | row) words
//   vote_sort      one workgroup per range: bitonic sort in LDS (ascending distance, ties by row)
//   vote_gather    the tile's rows through the shuffle (tile_body.hpp), global row numbers, possibility += delta over the sorted prefix (every
//                  row once: plain float64 read-modify-write, no atomics, the same bits on every run), and the histogram cleared
//   vote_min_part  stage 1 of the cloud's new minimum: one partial (value, first row) per workgroup of VM_CHUNK rows
// ... and one vote_pick more per call that only finishes the last tile's minimum.
#include "ssdr_internal.hpp"
#include "tile_body.hpp"
#include <cstring>
#include <vector>

namespace ssdr {
namespace {

constexpr int VOTE_LAUNCHES = 7;
constexpr int VOTE_MAX_CLOUDS = 4096;                 // predict.hip's bound
constexpr int TS_BITS = 14, TS_BINS = 1 << TS_BITS, TS_SHIFT = 31 - TS_BITS;      // tile.hip's histogram: 8 exponent + 6 mantissa bits
constexpr int TS_RCAP = 4096, TS_RSTEP = 1024, TS_CPT = 12, TS_RMAX = 2048;
constexpr int VM_CHUNK = 2048, VM_MAXPART = 1024;     // rows per stage-1 workgroup pass; most partials per cloud

struct VoteRec { int c, base, m; float cx, cy, cz; int pad0, pad1; };
struct MinPart { double v; int i; int pad; };

// (value, row) pairs order by value, then row: their minimum is np.argmin's first minimum whatever the order of the reduction
__device__ __forceinline__ bool vm_less(double v, int i, double w, int j) { return v < w || (v == w && i < j); }

// block minimum of (v, i) over 256 threads; the result in s_v[0], s_i[0] (callers synchronise before reusing the arrays)
__device__ __forceinline__ void vm_block_min(double v, int i, double* s_v, int* s_i) {
    const int tid = threadIdx.x;
    s_v[tid] = v; s_i[tid] = i;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o && vm_less(s_v[tid + o], s_i[tid + o], s_v[tid], s_i[tid])) { s_v[tid] = s_v[tid + o]; s_i[tid] = s_i[tid + o]; }
        __syncthreads();
    }
}

// stage 1: rec != nullptr: the record's cloud (grid x = partials, sized by the largest cloud); else cloud blockIdx.y of the offset table.
// Workgroup x reduces chunks x, x + gridDim.x, ... of VM_CHUNK rows; one without a chunk leaves at once (stage 2 counts the live ones).
__global__ __launch_bounds__(256) void vote_min_part(const VoteRec* __restrict__ rec, const int* __restrict__ off, const double* __restrict__ possibility, MinPart* part) {
    __shared__ double s_v[256];
    __shared__ int s_i[256];
    int base, m;
    if (rec) { base = rec->base; m = rec->m; } else { base = off[blockIdx.y]; m = off[blockIdx.y + 1] - base; }
    if ((long long)blockIdx.x * VM_CHUNK >= m) return;
    const double* P = possibility + base;
    double bv = 1.0e300; int bi = 0x7fffffff;
    for (long long c0 = (long long)blockIdx.x * VM_CHUNK; c0 < m; c0 += (long long)gridDim.x * VM_CHUNK) {
        const int e = (int)min((long long)m, c0 + VM_CHUNK);
        for (int i = (int)c0 + threadIdx.x; i < e; i += 256) { const double v = P[i]; if (vm_less(v, i, bv, bi)) { bv = v; bi = i; } }
    }
    vm_block_min(bv, bi, s_v, s_i);
    if (threadIdx.x == 0) { MinPart o; o.v = s_v[0]; o.i = s_i[0]; o.pad = 0; part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = o; }
}
__device__ __forceinline__ int vm_live(int m, int gx) { return min(gx, (m + VM_CHUNK - 1) / VM_CHUNK); }

// stage 2 for ssdr_vote_init_dev: one workgroup per cloud
__global__ __launch_bounds__(256) void vote_min_fin(const int* __restrict__ off, const MinPart* __restrict__ part, int gx, double* cloud_min, int* cloud_arg) {
    __shared__ double s_v[256];
    __shared__ int s_i[256];
    const int c = blockIdx.x, live = vm_live(off[c + 1] - off[c], gx);
    double bv = 1.0e300; int bi = 0x7fffffff;
    for (int k = threadIdx.x; k < live; k += 256) { const MinPart p = part[(size_t)c * gx + k]; if (vm_less(p.v, p.i, bv, bi)) { bv = p.v; bi = p.i; } }
    vm_block_min(bv, bi, s_v, s_i);
    if (threadIdx.x == 0) { cloud_min[c] = s_v[0]; cloud_arg[c] = s_i[0]; }
}

// One workgroup.  has_prev: the record holds the tile before this one, whose stage-1 partials wait in `part`: its cloud's new minimum and
// first arg-min are written (:135).  do_pick: tile t's cloud (:106), point (:108), centre (:112-115) -> the record, d_out_cloud, d_out_center.
__global__ __launch_bounds__(256) void vote_pick(int has_prev, int do_pick, int t, int nc, int gx, VoteRec* rec, const MinPart* __restrict__ part, const int* __restrict__ off,
                                                 const float* __restrict__ pts, const float* __restrict__ noise, double* cloud_min, int* cloud_arg,
                                                 int* out_cloud, float* out_center) {
    __shared__ double s_v[256];
    __shared__ int s_i[256];
    __shared__ double s_pv;
    __shared__ int s_pi;
    const int tid = threadIdx.x;
    int pc = -1;
    if (has_prev) {
        pc = rec->c;
        const int live = vm_live(rec->m, gx);
        double bv = 1.0e300; int bi = 0x7fffffff;
        for (int k = tid; k < live; k += 256) { const MinPart p = part[k]; if (vm_less(p.v, p.i, bv, bi)) { bv = p.v; bi = p.i; } }
        vm_block_min(bv, bi, s_v, s_i);
        if (tid == 0) { s_pv = s_v[0]; s_pi = s_i[0]; cloud_min[pc] = s_v[0]; cloud_arg[pc] = s_i[0]; }
        __syncthreads();
    }
    if (!do_pick) return;
    // the previous tile's cloud is read from LDS, not back from the global array this workgroup has just written
    double bv = 1.0e300; int bi = 0x7fffffff;
    for (int c = tid; c < nc; c += 256) { const double v = c == pc ? s_pv : cloud_min[c]; if (vm_less(v, c, bv, bi)) { bv = v; bi = c; } }
    __syncthreads();
    vm_block_min(bv, bi, s_v, s_i);
    if (tid == 0) {
        const int c = min(s_i[0], nc - 1);                       // (a map of NaNs alone: stay inside the table)
        const int base = off[c], m = off[c + 1] - base;
        int p = c == pc ? s_pi : cloud_arg[c];
        p = min(max(p, 0), m - 1);
        VoteRec r;
        r.c = c; r.base = base; r.m = m; r.pad0 = 0; r.pad1 = 0;
        r.cx = pts[3 * ((size_t)base + p)] + noise[3 * (size_t)t];
        r.cy = pts[3 * ((size_t)base + p) + 1] + noise[3 * (size_t)t + 1];
        r.cz = pts[3 * ((size_t)base + p) + 2] + noise[3 * (size_t)t + 2];
        *rec = r;
        out_cloud[t] = c;
        out_center[3 * (size_t)t] = r.cx; out_center[3 * (size_t)t + 1] = r.cy; out_center[3 * (size_t)t + 2] = r.cz;
    }
}

__global__ __launch_bounds__(256) void vote_hist(const VoteRec* __restrict__ rec, const float* __restrict__ pts, unsigned* hist) {
    __shared__ unsigned s_h[TS_BINS];
    const int m = rec->m;
    if ((int)blockIdx.x * 256 >= m) return;
    const float cx = rec->cx, cy = rec->cy, cz = rec->cz;
    for (int b = threadIdx.x; b < TS_BINS; b += 256) s_h[b] = 0u;
    __syncthreads();
    const float* P = pts + 3 * (size_t)rec->base;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < m; i += gridDim.x * 256) atomicAdd(&s_h[__float_as_uint(tile_dist(P, i, cx, cy, cz)) >> TS_SHIFT], 1u);
    __syncthreads();
    for (int b = threadIdx.x; b < TS_BINS; b += 256) if (s_h[b]) atomicAdd(&hist[b], s_h[b]);
}

// tile.hip's threshold step for the record's cloud: T = the first bin whose cumulative count reaches want = min(num_points, m); the histogram
// becomes the start of every bin <= T among the candidates (bins beyond T: 0); rstart[k] = the first bin start in [k TS_RSTEP, (k + 1) TS_RSTEP)
__global__ __launch_bounds__(256) void vote_thresh(const VoteRec* __restrict__ rec, unsigned* hist, int num_points, unsigned* thr, int* d_cand, unsigned* rstart, unsigned* rcur, int rstride,
                                                   const int* __restrict__ perm, int* padmap) {
    __shared__ unsigned s_h[TS_BINS + TS_BINS / 32];          // one pad word per 32 bins: a thread's stretch starts in its own bank pair
    __shared__ unsigned s_part[256];
    __shared__ unsigned s_T;
    const int tid = threadIdx.x, m = rec->m;
    constexpr int PER = TS_BINS / 256;
    auto at = [](int b) { return b + (b >> 5); };
    const unsigned want = (unsigned)min(num_points, m);
    for (int b = tid; b < TS_BINS; b += 256) s_h[at(b)] = hist[b];
    for (int k = tid; k < rstride; k += 256) { rstart[k] = 0xffffffffu; rcur[k] = 0u; }
    __syncthreads();
    unsigned tot = 0;
    for (int k = 0; k < PER; ++k) tot += s_h[at(tid * PER + k)];
    s_part[tid] = tot;
    __syncthreads();
    unsigned incl = tot;
    for (int o = 1; o < 256; o <<= 1) {
        const unsigned y = tid >= o ? s_part[tid - o] : 0u;
        __syncthreads();
        incl += y; s_part[tid] = incl;
        __syncthreads();
    }
    const unsigned before = incl - tot;
    if (want > 0 && before < want && incl >= want) {          // the bin where the cumulative count reaches `want` lies in this thread's stretch
        unsigned run = before; int k = 0;
        while (k < PER - 1 && run + s_h[at(tid * PER + k)] < want) { run += s_h[at(tid * PER + k)]; ++k; }
        s_T = (unsigned)(tid * PER + k);
    }
    if (want == 0 && tid == 0) s_T = 0;
    __syncthreads();
    const unsigned T = s_T;
    unsigned pos = before, ncand = 0;
    for (int k = 0; k < PER; ++k) {
        const int b = tid * PER + k;
        const unsigned cb = s_h[at(b)];
        if ((unsigned)b <= T) {
            s_h[at(b)] = pos;
            if (cb) atomicMin(&rstart[pos / TS_RSTEP], pos);
            pos += cb; ncand = pos;
        } else s_h[at(b)] = 0u;
    }
    if ((unsigned)(tid * PER) <= T && (unsigned)(tid * PER + PER - 1) >= T) { *thr = T; *d_cand = (int)ncand; }
    __syncthreads();
    for (int b = tid; b < TS_BINS; b += 256) hist[b] = s_h[at(b)];
    tile_padmap_body(m, num_points, perm, padmap, s_part);
}

// candidates to their range's slots: counted per range in LDS, each range's share reserved with one global atomic per workgroup pass
__global__ __launch_bounds__(256) void vote_compact(const VoteRec* __restrict__ rec, const float* __restrict__ pts, const unsigned* __restrict__ thr, const unsigned* __restrict__ hist,
                                                    const unsigned* __restrict__ rstart, unsigned* rcur, int rstride, uint64_t* keys) {
    __shared__ unsigned s_cnt[TS_RMAX], s_base[TS_RMAX];
    const int m = rec->m, tid = threadIdx.x;
    if ((long long)blockIdx.x * 256 * TS_CPT >= m) return;
    const float cx = rec->cx, cy = rec->cy, cz = rec->cz;
    const float* P = pts + 3 * (size_t)rec->base;
    const unsigned T = *thr;
    const int nr = min(rstride, m / TS_RSTEP + 2);               // the ranges this cloud's candidates can reach
    for (int i0 = blockIdx.x * 256 * TS_CPT; i0 < m; i0 += gridDim.x * 256 * TS_CPT) {          // uniform over the workgroup
        for (int k = tid; k < nr; k += 256) s_cnt[k] = 0u;
        __syncthreads();
        unsigned bits[TS_CPT], loc[TS_CPT]; int rid[TS_CPT];
#pragma unroll
        for (int u = 0; u < TS_CPT; ++u) {
            const int i = i0 + u * 256 + tid;
            rid[u] = -1; bits[u] = 0u; loc[u] = 0u;
            if (i < m) {
                bits[u] = __float_as_uint(tile_dist(P, i, cx, cy, cz));
                const unsigned b = bits[u] >> TS_SHIFT;
                if (b <= T) { rid[u] = (int)(hist[b] / TS_RSTEP); loc[u] = atomicAdd(&s_cnt[rid[u]], 1u); }
            }
        }
        __syncthreads();
        for (int k = tid; k < nr; k += 256) { const unsigned c = s_cnt[k]; if (c) s_base[k] = rstart[k] + atomicAdd(&rcur[k], c); }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < TS_CPT; ++u)
            if (rid[u] >= 0) keys[s_base[rid[u]] + loc[u]] = ((uint64_t)bits[u] << 32) | (uint64_t)(uint32_t)(i0 + u * 256 + tid);
        __syncthreads();
    }
}
// the same with one global atomic per candidate on its bin's cursor (clouds of more than TS_RMAX ranges)
__global__ __launch_bounds__(256) void vote_compact_bins(const VoteRec* __restrict__ rec, const float* __restrict__ pts, const unsigned* __restrict__ thr, unsigned* hist, uint64_t* keys) {
    const int m = rec->m;
    const float cx = rec->cx, cy = rec->cy, cz = rec->cz;
    const float* P = pts + 3 * (size_t)rec->base;
    const unsigned T = *thr;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < m; i += gridDim.x * 256) {
        const unsigned bits = __float_as_uint(tile_dist(P, i, cx, cy, cz));
        const unsigned b = bits >> TS_SHIFT;
        if (b <= T) keys[atomicAdd(&hist[b], 1u)] = ((uint64_t)bits << 32) | (uint64_t)(uint32_t)i;
    }
}

// one workgroup per range: bitonic network with ascending comparators only (the first step of every merge pairs a word with its mirror
// image in the block), so slots >= n count as +infinity, are never touched, and n need not be a power of two.  Up to TS_RCAP words in LDS,
// a longer range (one bin of more than TS_RSTEP candidates) in place in global memory.
__global__ __launch_bounds__(256) void vote_sort(const unsigned* __restrict__ rstart, const int* __restrict__ d_cand, uint64_t* keys) {
    __shared__ uint64_t s_k[TS_RCAP];
    const int tid = threadIdx.x;
    const unsigned cand = (unsigned)*d_cand;
    const int nk = (int)((cand + TS_RSTEP - 1) / TS_RSTEP);
    for (int q = blockIdx.x; q < nk; q += gridDim.x) {
        const unsigned s0 = rstart[q];
        if (s0 == 0xffffffffu) continue;                         // no bin starts here (it lies inside the previous range's last bin)
        unsigned e0 = cand;
        for (int q2 = q + 1; q2 < nk; ++q2) if (rstart[q2] != 0xffffffffu) { e0 = rstart[q2]; break; }
        const unsigned n = e0 - s0;
        if (n <= 1) continue;
        unsigned N = 2; while (N < n) N <<= 1;
        const bool lds = n <= (unsigned)TS_RCAP;
        uint64_t* A = lds ? s_k : keys + s0;
        if (lds) { for (unsigned i = tid; i < n; i += 256) s_k[i] = keys[s0 + i]; __syncthreads(); }
        for (unsigned k = 2; k <= N; k <<= 1) {
            for (unsigned j = k >> 1; j > 0; j >>= 1) {
                for (unsigned i = tid; i < N / 2; i += 256) {
                    unsigned lo, hi;
                    if (j == (k >> 1)) { const unsigned blk = i / j, o = i % j; lo = blk * k + o; hi = blk * k + (k - 1 - o); }
                    else { lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)); hi = lo | j; }
                    if (hi < n) { const uint64_t a = A[lo], b = A[hi]; if (a > b) { A[lo] = b; A[hi] = a; } }
                }
                if (!lds) __threadfence_block();
                __syncthreads();
            }
        }
        if (lds) { for (unsigned i = tid; i < n; i += 256) keys[s0 + i] = s_k[i]; __syncthreads(); }
    }
}

// the tile's rows (tile_body.hpp: shuffle, padding, centring, colours), their global row numbers, the possibility update (:132-134) over the
// sorted prefix (its rows are distinct: one plain update each), and the histogram cleared for the next tile
__global__ __launch_bounds__(256) void vote_gather(const VoteRec* __restrict__ rec, const float* __restrict__ pts, const float* __restrict__ colors, int cdim, const int* __restrict__ labels,
                                                   const uint64_t* __restrict__ keys, const int* __restrict__ perm, const float* __restrict__ dup_u, int num_points, float color_scale,
                                                   float* out_xyz, float* out_feat, int* out_idx, int* out_lab, const int* __restrict__ padmap, double* possibility, unsigned* hist) {
    const int base = rec->base, m = rec->m;
    const size_t o = (size_t)base;
    tile_gather_body(pts + 3 * o, colors ? colors + o * cdim : nullptr, cdim, reinterpret_cast<const uint32_t*>(keys), &rec->m, perm, dup_u, num_points, rec->cx, rec->cy, rec->cz,
                     color_scale, out_xyz, out_feat, out_idx, padmap, 2, -1, labels ? labels + o : nullptr, out_lab);
    for (int r = blockIdx.x * 256 + threadIdx.x; r < num_points; r += gridDim.x * 256) out_idx[r] += base;      // (this thread wrote the row)
    const int avail = min(m, num_points);
    if (avail > 0) {
        const float dmax = __uint_as_float((unsigned)(keys[avail - 1] >> 32));
        double* P = possibility + o;
        for (int r = blockIdx.x * 256 + threadIdx.x; r < avail; r += gridDim.x * 256) {
            const uint64_t w = keys[r];
            const float q = 1 - __uint_as_float((unsigned)(w >> 32)) / dmax;
            P[(uint32_t)w] += (double)(q * q);
        }
    }
    for (int b = blockIdx.x * 256 + threadIdx.x; b < TS_BINS; b += gridDim.x * 256) hist[b] = 0u;
}

struct VoteState {
    DevBuf rec, part, off, keys, hist, thr, rstart, rcur, padmap;
    StagingRing<int> staging;
    std::vector<int> off_host;          // the table the device holds: uploaded again only when a call brings another one
    bool hist_clear = false;
};
VoteState& vst(hipStream_t s) { return per_stream<VoteState>(s); }

// validates the offsets: the refusals both entries share, made before anything is initialised or launched
int vote_offsets(const char* who, const int64_t* cloud_offsets, size_t num_clouds, std::vector<int>& off, int& maxn) {
    if (!cloud_offsets || num_clouds == 0) { set_error("%s: no clouds", who); return SSDR_ERR_INVALID; }
    if (num_clouds > (size_t)VOTE_MAX_CLOUDS) { set_error("%s: %zu clouds (at most %d)", who, num_clouds, VOTE_MAX_CLOUDS); return SSDR_ERR_UNSUPPORTED; }
    if (cloud_offsets[0] != 0) { set_error("%s: cloud_offsets[0] must be 0", who); return SSDR_ERR_INVALID; }
    off.resize(num_clouds + 1);
    maxn = 0;
    for (size_t c = 0; c < num_clouds; ++c) {
        const int64_t n = cloud_offsets[c + 1] - cloud_offsets[c];
        if (n <= 0) { set_error("%s: cloud %zu is empty (every cloud needs at least one point)", who, c); return SSDR_ERR_INVALID; }
        if (cloud_offsets[c + 1] > 0x3fffffff) { set_error("%s: more than 0x3fffffff points in all", who); return SSDR_ERR_UNSUPPORTED; }
        off[c] = (int)cloud_offsets[c]; maxn = std::max(maxn, (int)n);
    }
    off[num_clouds] = (int)cloud_offsets[num_clouds];
    return SSDR_OK;
}
// leaves the int32 table on the device.  It travels through a pinned ring slot and only when it differs from the one the stream's state
// already holds: the calls of an evaluation all bring the same table, so none of them waits for the stream
int vote_upload(const char* who, VoteState& V, std::vector<int>& off, hipStream_t s) {
    if (off == V.off_host) return SSDR_OK;
    SSDR_TRY(V.off.reserve(4 * off.size()));
    int* st = nullptr;
    const int slot = V.staging.acquire(off.size(), &st);
    if (slot < 0) { set_error("%s: pinned staging buffer", who); return SSDR_ERR_HIP; }
    memcpy(st, off.data(), 4 * off.size());
    SSDR_HIP(hipMemcpyAsync(V.off.p, st, 4 * off.size(), hipMemcpyHostToDevice, s));
    if (V.staging.release(slot, s)) { set_error("%s: staging event", who); return SSDR_ERR_HIP; }
    V.off_host.swap(off);
    return SSDR_OK;
}
inline int vm_grid(int maxn) { return std::max(1, std::min((maxn + VM_CHUNK - 1) / VM_CHUNK, VM_MAXPART)); }

}  // namespace
}  // namespace ssdr

using namespace ssdr;

extern "C" int ssdr_vote_tile_launches(void) { return VOTE_LAUNCHES; }

extern "C" int ssdr_vote_init_dev(const double* d_possibility, const int64_t* cloud_offsets, size_t num_clouds, double* d_cloud_min, int32_t* d_cloud_arg, void* stream) {
    int maxn = 0;
    if (!d_possibility || !d_cloud_min || !d_cloud_arg) { set_error("vote_init: bad arguments"); return SSDR_ERR_INVALID; }
    std::vector<int> off;
    SSDR_TRY(vote_offsets("vote_init", cloud_offsets, num_clouds, off, maxn));
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); VoteState& V = vst(s);
    SSDR_TRY(vote_upload("vote_init", V, off, s));
    const int gx = std::min(vm_grid(maxn), 64);
    SSDR_TRY(V.part.reserve(sizeof(MinPart) * std::max((size_t)gx * num_clouds, (size_t)VM_MAXPART)));
    hipLaunchKernelGGL(vote_min_part, dim3(gx, (unsigned)num_clouds), dim3(256), 0, s, (const VoteRec*)nullptr, V.off.as<int>(), d_possibility, V.part.as<MinPart>());
    hipLaunchKernelGGL(vote_min_fin, dim3((unsigned)num_clouds), dim3(256), 0, s, V.off.as<int>(), V.part.as<MinPart>(), gx, d_cloud_min, d_cloud_arg);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

extern "C" int ssdr_vote_tiles_dev(const float* d_points, const float* d_colors, int color_dim, const int32_t* d_labels, double* d_possibility,
                                   double* d_cloud_min, int32_t* d_cloud_arg, const int64_t* cloud_offsets, size_t num_clouds,
                                   size_t num_tiles, size_t num_points, const float* d_noise, const int32_t* d_perm, const float* d_dup_u, float color_scale,
                                   float* d_out_xyz, float* d_out_feat, int32_t* d_out_idx, int32_t* d_out_labels, int32_t* d_out_cloud, float* d_out_center, void* stream) {
    if (!d_points || !d_possibility || !d_cloud_min || !d_cloud_arg || !d_noise || !d_perm || !d_dup_u || !d_out_xyz || !d_out_idx || !d_out_cloud || !d_out_center) {
        set_error("vote_tiles: bad arguments"); return SSDR_ERR_INVALID;
    }
    if (num_tiles == 0 || num_points == 0) { set_error("vote_tiles: num_tiles and num_points must be positive"); return SSDR_ERR_INVALID; }
    if (num_points > 0x3fffffff / num_tiles) { set_error("vote_tiles: num_tiles x num_points above 0x3fffffff rows"); return SSDR_ERR_UNSUPPORTED; }
    if (d_out_labels && !d_labels) { set_error("vote_tiles: labels missing"); return SSDR_ERR_INVALID; }
    if (d_out_feat && color_dim > 0 && !d_colors) { set_error("vote_tiles: colors missing"); return SSDR_ERR_INVALID; }
    if (color_dim < 0) { set_error("vote_tiles: color_dim"); return SSDR_ERR_INVALID; }
    int maxn = 0;
    std::vector<int> offh;
    SSDR_TRY(vote_offsets("vote_tiles", cloud_offsets, num_clouds, offh, maxn));
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); VoteState& V = vst(s);
    SSDR_TRY(vote_upload("vote_tiles", V, offh, s));
    const int N = (int)num_points, nc = (int)num_clouds, cdim = d_colors ? color_dim : 0;
    const int rstride = (maxn + TS_RSTEP - 1) / TS_RSTEP + 1;
    const int gx = vm_grid(maxn);
    SSDR_TRY(V.rec.reserve(sizeof(VoteRec))); SSDR_TRY(V.part.reserve(sizeof(MinPart) * VM_MAXPART));
    SSDR_TRY(V.keys.reserve(8 * (size_t)maxn + 16)); SSDR_TRY(V.hist.reserve(4 * (size_t)TS_BINS)); SSDR_TRY(V.thr.reserve(16));
    SSDR_TRY(V.rstart.reserve(4 * (size_t)rstride)); SSDR_TRY(V.rcur.reserve(4 * (size_t)rstride)); SSDR_TRY(V.padmap.reserve(4 * num_points));
    if (!V.hist_clear) { SSDR_HIP(hipMemsetAsync(V.hist.p, 0, 4 * (size_t)TS_BINS, s)); V.hist_clear = true; }      // vote_gather leaves it clear
    VoteRec* rec = V.rec.as<VoteRec>(); MinPart* part = V.part.as<MinPart>();
    const int* off = V.off.as<int>();
    unsigned* hist = V.hist.as<unsigned>(); unsigned* thr = V.thr.as<unsigned>(); int* cand = reinterpret_cast<int*>(V.thr.as<unsigned>() + 1);
    unsigned* rstart = V.rstart.as<unsigned>(); unsigned* rcur = V.rcur.as<unsigned>();
    uint64_t* keys = V.keys.as<uint64_t>(); int* padmap = V.padmap.as<int>();
    const int g_hist = std::max(1, std::min((maxn + 255) / 256, 64));
    const int g_comp = std::max(1, std::min((maxn + 256 * TS_CPT - 1) / (256 * TS_CPT), 256));
    const int g_gath = std::max(1, std::min((N + 255) / 256, 256));
    const int fdim = 3 + cdim;
    for (size_t t = 0; t < num_tiles; ++t) {
        const size_t q = t * num_points;
        hipLaunchKernelGGL(vote_pick, dim3(1), dim3(256), 0, s, t > 0 ? 1 : 0, 1, (int)t, nc, gx, rec, (const MinPart*)part, off, d_points, d_noise, d_cloud_min, d_cloud_arg,
                           d_out_cloud, d_out_center);
        hipLaunchKernelGGL(vote_hist, dim3(g_hist), dim3(256), 0, s, (const VoteRec*)rec, d_points, hist);
        hipLaunchKernelGGL(vote_thresh, dim3(1), dim3(256), 0, s, (const VoteRec*)rec, hist, N, thr, cand, rstart, rcur, rstride, d_perm + q, padmap);
        if (rstride <= TS_RMAX)
            hipLaunchKernelGGL(vote_compact, dim3(g_comp), dim3(256), 0, s, (const VoteRec*)rec, d_points, (const unsigned*)thr, (const unsigned*)hist, (const unsigned*)rstart, rcur, rstride, keys);
        else hipLaunchKernelGGL(vote_compact_bins, dim3(g_hist), dim3(256), 0, s, (const VoteRec*)rec, d_points, (const unsigned*)thr, hist, keys);
        hipLaunchKernelGGL(vote_sort, dim3(std::min(rstride, 64)), dim3(256), 0, s, (const unsigned*)rstart, (const int*)cand, keys);
        hipLaunchKernelGGL(vote_gather, dim3(g_gath), dim3(256), 0, s, (const VoteRec*)rec, d_points, d_colors, cdim, d_labels, (const uint64_t*)keys, d_perm + q, d_dup_u + q, N,
                           color_scale, d_out_xyz + 3 * q, d_out_feat ? d_out_feat + q * fdim : nullptr, d_out_idx + q, d_out_labels ? d_out_labels + q : nullptr,
                           (const int*)padmap, d_possibility, hist);
        hipLaunchKernelGGL(vote_min_part, dim3(gx), dim3(256), 0, s, (const VoteRec*)rec, off, (const double*)d_possibility, part);
    }
    hipLaunchKernelGGL(vote_pick, dim3(1), dim3(256), 0, s, 1, 0, 0, nc, gx, rec, (const MinPart*)part, off, d_points, d_noise, d_cloud_min, d_cloud_arg, d_out_cloud, d_out_center);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}
