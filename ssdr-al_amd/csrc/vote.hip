// Generator chain for gfx950: get_batch of the test datasets (S3/s3dis_dataset_test.py:97-151) with the cloud and the centre of every tile chosen
// on the device.  ssdr_vote_tiles_dev is that loop as S3DIS writes it: all three axes centred, every row's update unweighted, global rows out.
// The Semantic3D flavours differ in rules this file takes as options of the same launches (ChainArgs, vote_chain.hpp; entry ssdr_feed_chain_dev
// in feed.hip): x and y centred only, the update weighted by the row's class (semantic3d_dataset_train.py:182, :193-198), cloud-local rows, the
// activation / pseudo-label channels.  vote_indep_launch runs the same kernels over tiles that do not depend on each other (tile = blockIdx.y,
// S3DIS_Dataset.spatially_regular_gen): no map, every tile's cloud and point given.
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
//
// Every kernel from vote_hist to vote_gather works on record, histogram, cursors, sort words, draws and output rows number blockIdx.y: the chain
// launches them with one row of workgroups per tile; independent tiles (vote_place writes all their records at once, nothing else before
// vote_hist, nothing after vote_gather) with one row per tile of the batch.
#include "ssdr_internal.hpp"
#include "tile_body.hpp"
#include "vote_chain.hpp"
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
    rec += blockIdx.y; hist += (size_t)blockIdx.y * TS_BINS;
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
    {
        const size_t y = blockIdx.y;
        rec += y; hist += y * TS_BINS; thr += 2 * y; d_cand += 2 * y; rstart += y * rstride; rcur += y * rstride; perm += y * num_points; padmap += y * num_points;
    }
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
                                                    const unsigned* __restrict__ rstart, unsigned* rcur, int rstride, uint64_t* keys, size_t kstride) {
    __shared__ unsigned s_cnt[TS_RMAX], s_base[TS_RMAX];
    {
        const size_t y = blockIdx.y;
        rec += y; thr += 2 * y; hist += y * TS_BINS; rstart += y * rstride; rcur += y * rstride; keys += y * kstride;
    }
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
__global__ __launch_bounds__(256) void vote_compact_bins(const VoteRec* __restrict__ rec, const float* __restrict__ pts, const unsigned* __restrict__ thr, unsigned* hist, uint64_t* keys, size_t kstride) {
    {
        const size_t y = blockIdx.y;
        rec += y; thr += 2 * y; hist += y * TS_BINS; keys += y * kstride;
    }
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
__global__ __launch_bounds__(256) void vote_sort(const unsigned* __restrict__ rstart, int rstride, const int* __restrict__ d_cand, uint64_t* keys, size_t kstride) {
    __shared__ uint64_t s_k[TS_RCAP];
    rstart += (size_t)blockIdx.y * rstride; d_cand += 2 * (size_t)blockIdx.y; keys += (size_t)blockIdx.y * kstride;
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

// the records of independent tiles, all at once (thread t = tile t): cloud tile_cloud[t], centre = its point tile_point[t] + noise[t] (float32,
// s3dis_dataset.py:119-126).  An id outside its range: a record without rows (the gather writes a zero tile) and a status bit.
__global__ __launch_bounds__(256) void vote_place(int num_tiles, int nc, const int* __restrict__ off, const float* __restrict__ pts, const int* __restrict__ tile_cloud,
                                                  const int* __restrict__ tile_point, const float* __restrict__ noise, VoteRec* rec, int* out_cloud, float* out_center, int* status) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= num_tiles) return;
    VoteRec r;
    r.c = -1; r.base = 0; r.m = 0; r.cx = r.cy = r.cz = 0.f; r.pad0 = 0; r.pad1 = 0;
    const int c = tile_cloud[t];
    if (c < 0 || c >= nc) atomicOr(status, FEED_ST_CLOUD);
    else {
        const int base = off[c], m = off[c + 1] - base, p = tile_point[t];
        if (p < 0 || p >= m) atomicOr(status, FEED_ST_POINT);
        else {
            r.c = c; r.base = base; r.m = m;
            r.cx = pts[3 * ((size_t)base + p)] + noise[3 * (size_t)t];
            r.cy = pts[3 * ((size_t)base + p) + 1] + noise[3 * (size_t)t + 1];
            r.cz = pts[3 * ((size_t)base + p) + 2] + noise[3 * (size_t)t + 2];
        }
    }
    rec[t] = r;
    if (out_cloud) out_cloud[t] = r.c < 0 ? 0 : r.c;           // (a refused tile: zeros throughout)
    if (out_center) { out_center[3 * (size_t)t] = r.cx; out_center[3 * (size_t)t + 1] = r.cy; out_center[3 * (size_t)t + 2] = r.cz; }
}

// what vote_gather reads and writes beyond the tile itself (all optional but hist)
struct GatherExtra {
    const float* act; const float* pse; float* out_act; float* out_pse;      // the channels: rows as out_lab's
    double* possibility; const double* cw; int num_labels; int* status;       // the map (chain only), the class weights of its update
    int flags;
};

// the tile's rows (tile_body.hpp: shuffle, padding, centring, colours), the channels and the row numbers in their final form, the possibility
// update (:132-134; weighted: semantic3d_dataset_train.py:193-198) over the sorted prefix (its rows are distinct: one plain update each), and the
// histogram cleared for the next tile
__global__ __launch_bounds__(256) void vote_gather(const VoteRec* __restrict__ rec, const float* __restrict__ pts, const float* __restrict__ colors, int cdim, const int* __restrict__ labels,
                                                   const uint64_t* __restrict__ keys, size_t kstride, const int* __restrict__ perm, const float* __restrict__ dup_u, int num_points, float color_scale,
                                                   float* out_xyz, float* out_feat, int* out_idx, int* out_lab, const int* __restrict__ padmap, unsigned* hist, GatherExtra e) {
    {
        const size_t y = blockIdx.y, q = y * num_points;
        rec += y; keys += y * kstride; perm += q; dup_u += q; padmap += q; hist += y * TS_BINS;
        out_xyz += 3 * q; out_idx += q;
        if (out_feat) out_feat += q * (3 + cdim);
        if (out_lab) out_lab += q;
        if (e.out_act) e.out_act += q;
        if (e.out_pse) e.out_pse += q;
    }
    const int base = rec->base, m = rec->m;
    const size_t o = (size_t)base;
    if (m <= 0) {                                              // (uniform) a refused tile: zeros; nothing was counted in its histogram
        for (int r = blockIdx.x * 256 + threadIdx.x; r < num_points; r += gridDim.x * 256) {
            out_xyz[3 * (size_t)r] = 0.f; out_xyz[3 * (size_t)r + 1] = 0.f; out_xyz[3 * (size_t)r + 2] = 0.f;
            if (out_feat) for (int c = 0; c < 3 + cdim; ++c) out_feat[(size_t)r * (3 + cdim) + c] = 0.f;
            out_idx[r] = 0;
            if (out_lab) out_lab[r] = 0;
            if (e.out_act) e.out_act[r] = 0.f;
            if (e.out_pse) e.out_pse[r] = 0.f;
        }
        return;
    }
    // x - 0 = x for every x: with SSDR_FEED_XY_ONLY z goes through as it is
    tile_gather_body(pts + 3 * o, colors ? colors + o * cdim : nullptr, cdim, reinterpret_cast<const uint32_t*>(keys), &rec->m, perm, dup_u, num_points, rec->cx, rec->cy,
                     (e.flags & SSDR_FEED_XY_ONLY) ? 0.f : rec->cz, color_scale, out_xyz, out_feat, out_idx, padmap, 2, -1, labels ? labels + o : nullptr, out_lab);
    const bool global_rows = (e.flags & SSDR_FEED_GLOBAL_ROWS) != 0;
    if (global_rows || e.out_act || e.out_pse)
        for (int r = blockIdx.x * 256 + threadIdx.x; r < num_points; r += gridDim.x * 256) {      // (this thread wrote the row)
            const int id = out_idx[r];
            if (e.out_act) e.out_act[r] = e.act[o + id];
            if (e.out_pse) e.out_pse[r] = e.pse[o + id];
            if (global_rows) out_idx[r] = id + base;
        }
    const int avail = min(m, num_points);
    if (e.possibility) {
        const float dmax = __uint_as_float((unsigned)(keys[avail - 1] >> 32));
        double* P = e.possibility + o;
        for (int r = blockIdx.x * 256 + threadIdx.x; r < avail; r += gridDim.x * 256) {
            const uint64_t w = keys[r];
            const float q = 1 - __uint_as_float((unsigned)(w >> 32)) / dmax;
            double d = (double)(q * q);
            if (e.cw) {                                        // the float32 square widened, then times the float64 weight of the row's class
                const int l = labels[o + (uint32_t)w];
                double wt = 0.0;
                if (l >= 0 && l < e.num_labels) wt = e.cw[l]; else atomicOr(e.status, FEED_ST_LABEL);
                d = d * wt;
            }
            P[(uint32_t)w] += d;
        }
    }
    for (int b = blockIdx.x * 256 + threadIdx.x; b < TS_BINS; b += gridDim.x * 256) hist[b] = 0u;
}

struct VoteState {
    DevBuf rec, part, off, keys, hist, thr, rstart, rcur, padmap, stat;
    StagingRing<int> staging;
    std::vector<int> off_host;          // the table the device holds: uploaded again only when a call brings another one
    size_t hist_clear = 0;              // bytes of the histogram known to be clear (vote_gather leaves it so)
    bool stat_clear = false;
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


// what both launchers refuse, and the scratch both need for `rows` rows of workgroups
int chain_check(const char* who, const ChainArgs& a) {
    if (!a.points || !a.noise || !a.perm || !a.dup_u || !a.out_xyz || !a.out_idx) { set_error("%s: bad arguments", who); return SSDR_ERR_INVALID; }
    if (a.num_tiles == 0 || a.num_points == 0) { set_error("%s: num_tiles and num_points must be positive", who); return SSDR_ERR_INVALID; }
    if (a.num_points > 0x3fffffff / a.num_tiles) { set_error("%s: num_tiles x num_points above 0x3fffffff rows", who); return SSDR_ERR_UNSUPPORTED; }
    if (a.out_labels && !a.labels) { set_error("%s: labels missing", who); return SSDR_ERR_INVALID; }
    if (a.out_feat && a.color_dim > 0 && !a.colors) { set_error("%s: colors missing", who); return SSDR_ERR_INVALID; }
    if (a.color_dim < 0) { set_error("%s: color_dim", who); return SSDR_ERR_INVALID; }
    if ((a.out_activation && !a.activation) || (a.out_pseudo && !a.pseudo)) { set_error("%s: a channel output without its input", who); return SSDR_ERR_INVALID; }
    if (a.class_weight && (!a.labels || a.num_labels <= 0)) { set_error("%s: class weights need labels and num_labels > 0", who); return SSDR_ERR_INVALID; }
    return SSDR_OK;
}
int chain_scratch(VoteState& V, size_t rows, int maxn, int rstride, size_t kstride, size_t num_points, hipStream_t s) {
    SSDR_TRY(V.rec.reserve(sizeof(VoteRec) * rows)); SSDR_TRY(V.part.reserve(sizeof(MinPart) * VM_MAXPART));
    SSDR_TRY(V.keys.reserve(8 * kstride * rows + 16)); SSDR_TRY(V.thr.reserve(8 * rows + 16));
    SSDR_TRY(V.rstart.reserve(4 * (size_t)rstride * rows)); SSDR_TRY(V.rcur.reserve(4 * (size_t)rstride * rows)); SSDR_TRY(V.padmap.reserve(4 * num_points * rows));
    const size_t hb = 4 * (size_t)TS_BINS * rows;
    if (V.hist.cap < hb) V.hist_clear = 0;                   // (a new buffer)
    SSDR_TRY(V.hist.reserve(hb));
    if (V.hist_clear < hb) { SSDR_HIP(hipMemsetAsync(V.hist.p, 0, hb, s)); V.hist_clear = hb; }      // vote_gather leaves it clear
    SSDR_TRY(V.stat.reserve(16));
    if (!V.stat_clear) { SSDR_HIP(hipMemsetAsync(V.stat.p, 0, 16, s)); V.stat_clear = true; }
    return SSDR_OK;
}
GatherExtra gather_extra(const ChainArgs& a, VoteState& V) {
    GatherExtra e;
    e.act = a.out_activation ? a.activation : nullptr; e.pse = a.out_pseudo ? a.pseudo : nullptr; e.out_act = a.out_activation; e.out_pse = a.out_pseudo;
    e.possibility = a.possibility; e.cw = a.class_weight; e.num_labels = a.num_labels; e.status = V.stat.as<int>(); e.flags = a.flags;
    return e;
}

}  // namespace

int vote_chain_launch(const char* who, const ChainArgs& a, void* stream) {
    // (every NULL check before any size check, as ssdr_vote_tiles_dev has always ordered them)
    if (!a.possibility || !a.cloud_min || !a.cloud_arg || !a.out_cloud || !a.out_center) { set_error("%s: bad arguments", who); return SSDR_ERR_INVALID; }
    SSDR_TRY(chain_check(who, a));
    int maxn = 0;
    std::vector<int> offh;
    SSDR_TRY(vote_offsets(who, a.cloud_offsets, a.num_clouds, offh, maxn));
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); VoteState& V = vst(s);
    SSDR_TRY(vote_upload(who, V, offh, s));
    const int N = (int)a.num_points, nc = (int)a.num_clouds, cdim = a.colors ? a.color_dim : 0;
    const int rstride = (maxn + TS_RSTEP - 1) / TS_RSTEP + 1;
    const int gx = vm_grid(maxn);
    const size_t kstride = (size_t)maxn;
    SSDR_TRY(chain_scratch(V, 1, maxn, rstride, kstride, a.num_points, s));
    VoteRec* rec = V.rec.as<VoteRec>(); MinPart* part = V.part.as<MinPart>();
    const int* off = V.off.as<int>();
    unsigned* hist = V.hist.as<unsigned>(); unsigned* thr = V.thr.as<unsigned>(); int* cand = reinterpret_cast<int*>(V.thr.as<unsigned>() + 1);
    unsigned* rstart = V.rstart.as<unsigned>(); unsigned* rcur = V.rcur.as<unsigned>();
    uint64_t* keys = V.keys.as<uint64_t>(); int* padmap = V.padmap.as<int>();
    const int g_hist = std::max(1, std::min((maxn + 255) / 256, 64));
    const int g_comp = std::max(1, std::min((maxn + 256 * TS_CPT - 1) / (256 * TS_CPT), 256));
    const int g_gath = std::max(1, std::min((N + 255) / 256, 256));
    const int fdim = 3 + cdim;
    const GatherExtra e0 = gather_extra(a, V);
    for (size_t t = 0; t < a.num_tiles; ++t) {
        const size_t q = t * a.num_points;
        hipLaunchKernelGGL(vote_pick, dim3(1), dim3(256), 0, s, t > 0 ? 1 : 0, 1, (int)t, nc, gx, rec, (const MinPart*)part, off, a.points, a.noise, a.cloud_min, a.cloud_arg,
                           a.out_cloud, a.out_center);
        hipLaunchKernelGGL(vote_hist, dim3(g_hist), dim3(256), 0, s, (const VoteRec*)rec, a.points, hist);
        hipLaunchKernelGGL(vote_thresh, dim3(1), dim3(256), 0, s, (const VoteRec*)rec, hist, N, thr, cand, rstart, rcur, rstride, a.perm + q, padmap);
        if (rstride <= TS_RMAX)
            hipLaunchKernelGGL(vote_compact, dim3(g_comp), dim3(256), 0, s, (const VoteRec*)rec, a.points, (const unsigned*)thr, (const unsigned*)hist, (const unsigned*)rstart, rcur, rstride, keys, kstride);
        else hipLaunchKernelGGL(vote_compact_bins, dim3(g_hist), dim3(256), 0, s, (const VoteRec*)rec, a.points, (const unsigned*)thr, hist, keys, kstride);
        hipLaunchKernelGGL(vote_sort, dim3(std::min(rstride, 64)), dim3(256), 0, s, (const unsigned*)rstart, rstride, (const int*)cand, keys, kstride);
        GatherExtra e = e0;
        if (e.out_act) e.out_act += q;
        if (e.out_pse) e.out_pse += q;
        hipLaunchKernelGGL(vote_gather, dim3(g_gath), dim3(256), 0, s, (const VoteRec*)rec, a.points, a.colors, cdim, a.labels, (const uint64_t*)keys, kstride, a.perm + q, a.dup_u + q, N,
                           a.color_scale, a.out_xyz + 3 * q, a.out_feat ? a.out_feat + q * fdim : nullptr, a.out_idx + q, a.out_labels ? a.out_labels + q : nullptr,
                           (const int*)padmap, hist, e);
        hipLaunchKernelGGL(vote_min_part, dim3(gx), dim3(256), 0, s, (const VoteRec*)rec, off, (const double*)a.possibility, part);
    }
    hipLaunchKernelGGL(vote_pick, dim3(1), dim3(256), 0, s, 1, 0, 0, nc, gx, rec, (const MinPart*)part, off, a.points, a.noise, a.cloud_min, a.cloud_arg, a.out_cloud, a.out_center);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int vote_indep_launch(const char* who, const ChainArgs& a, void* stream) {
    if (!a.tile_cloud || !a.tile_point) { set_error("%s: bad arguments", who); return SSDR_ERR_INVALID; }
    SSDR_TRY(chain_check(who, a));
    if (a.num_tiles > 65535) { set_error("%s: %zu tiles (at most 65535 in one call)", who, a.num_tiles); return SSDR_ERR_UNSUPPORTED; }
    int maxn = 0;
    std::vector<int> offh;
    SSDR_TRY(vote_offsets(who, a.cloud_offsets, a.num_clouds, offh, maxn));
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); VoteState& V = vst(s);
    SSDR_TRY(vote_upload(who, V, offh, s));
    const int N = (int)a.num_points, nc = (int)a.num_clouds, cdim = a.colors ? a.color_dim : 0, T = (int)a.num_tiles;
    const int rstride = (maxn + TS_RSTEP - 1) / TS_RSTEP + 1;
    const size_t kstride = (size_t)maxn;                     // the tiles' clouds are known on the device only: room for the largest, per tile
    SSDR_TRY(chain_scratch(V, a.num_tiles, maxn, rstride, kstride, a.num_points, s));
    VoteRec* rec = V.rec.as<VoteRec>();
    unsigned* hist = V.hist.as<unsigned>(); unsigned* thr = V.thr.as<unsigned>(); int* cand = reinterpret_cast<int*>(V.thr.as<unsigned>() + 1);
    unsigned* rstart = V.rstart.as<unsigned>(); unsigned* rcur = V.rcur.as<unsigned>();
    uint64_t* keys = V.keys.as<uint64_t>(); int* padmap = V.padmap.as<int>();
    const unsigned Y = (unsigned)T;
    const int g_hist = std::max(1, std::min((maxn + 255) / 256, 64));
    const int g_comp = std::max(1, std::min((maxn + 256 * TS_CPT - 1) / (256 * TS_CPT), 256));
    const int g_gath = std::max(1, std::min((N + 255) / 256, 256));
    GatherExtra e = gather_extra(a, V);
    e.possibility = nullptr; e.cw = nullptr; e.flags &= ~SSDR_FEED_GLOBAL_ROWS;
    hipLaunchKernelGGL(vote_place, dim3((T + 255) / 256), dim3(256), 0, s, T, nc, V.off.as<int>(), a.points, a.tile_cloud, a.tile_point, a.noise, rec, a.out_cloud, a.out_center, V.stat.as<int>());
    hipLaunchKernelGGL(vote_hist, dim3(g_hist, Y), dim3(256), 0, s, (const VoteRec*)rec, a.points, hist);
    hipLaunchKernelGGL(vote_thresh, dim3(1, Y), dim3(256), 0, s, (const VoteRec*)rec, hist, N, thr, cand, rstart, rcur, rstride, a.perm, padmap);
    if (rstride <= TS_RMAX)
        hipLaunchKernelGGL(vote_compact, dim3(g_comp, Y), dim3(256), 0, s, (const VoteRec*)rec, a.points, (const unsigned*)thr, (const unsigned*)hist, (const unsigned*)rstart, rcur, rstride, keys, kstride);
    else hipLaunchKernelGGL(vote_compact_bins, dim3(g_hist, Y), dim3(256), 0, s, (const VoteRec*)rec, a.points, (const unsigned*)thr, hist, keys, kstride);
    hipLaunchKernelGGL(vote_sort, dim3(std::min(rstride, 64), Y), dim3(256), 0, s, (const unsigned*)rstart, rstride, (const int*)cand, keys, kstride);
    hipLaunchKernelGGL(vote_gather, dim3(g_gath, Y), dim3(256), 0, s, (const VoteRec*)rec, a.points, a.colors, cdim, a.labels, (const uint64_t*)keys, kstride, a.perm, a.dup_u, N,
                       a.color_scale, a.out_xyz, a.out_feat, a.out_idx, a.out_labels, (const int*)padmap, hist, e);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int vote_status(void* stream, int32_t* out_status) {
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); VoteState& V = vst(s);
    int st = 0;
    SSDR_HIP(hipStreamSynchronize(s));
    if (V.stat.p && V.stat_clear) {
        SSDR_HIP(hipMemcpy(&st, V.stat.p, 4, hipMemcpyDeviceToHost));
        if (st) {                                              // cleared in stream order: the stream's next call finds it clear, whatever kind of stream it is
            SSDR_HIP(hipMemsetAsync(V.stat.p, 0, 4, s));
            SSDR_HIP(hipStreamSynchronize(s));
        }
    }
    if (out_status) *out_status = st;
    if (st) { set_error("feed: device status 0x%x (1 = a label outside the class weights, 2 = a tile's cloud id, 4 = a tile's point id out of range)", st); return SSDR_ERR_INVALID; }
    return SSDR_OK;
}

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
    ChainArgs a = {};
    a.points = d_points; a.colors = d_colors; a.color_dim = color_dim; a.labels = d_labels; a.possibility = d_possibility; a.cloud_min = d_cloud_min; a.cloud_arg = d_cloud_arg;
    a.cloud_offsets = cloud_offsets; a.num_clouds = num_clouds; a.num_tiles = num_tiles; a.num_points = num_points; a.noise = d_noise; a.perm = d_perm; a.dup_u = d_dup_u;
    a.color_scale = color_scale; a.out_xyz = d_out_xyz; a.out_feat = d_out_feat; a.out_idx = d_out_idx; a.out_labels = d_out_labels; a.out_cloud = d_out_cloud;
    a.out_center = d_out_center; a.flags = SSDR_FEED_GLOBAL_ROWS;
    return vote_chain_launch("vote_tiles", a, stream);
}
