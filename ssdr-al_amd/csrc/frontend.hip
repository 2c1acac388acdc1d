// Grid subsampling of a batch of room-scale clouds without a global sort: one partition pass into spatial buckets, then one
// workgroup per bucket that orders and reduces its voxels in LDS.
//
// Reference: S3/utils/cpp_wrappers/cpp_subsampling/grid_subsampling/grid_subsampling.cpp:5-106.  Same contract as subsample.hip
// (fp32 voxel arithmetic :27-31/:53-56, per-voxel sums in INPUT order :59-70, `sum * (float)(1.0/count)` for positions and
// `sum / (float)count` for features :87-95, majority label with the reference's tie rule :97-101); rows come out by ascending voxel key.
//
// The sort-based formulation (subsample.hip) moved ~5.4 GB through HBM for 0.48 GB of algorithmic bytes (three digit passes over
// 13.4 M sort words plus a random 32-byte gather per point).  Here a point travels twice:
//
//   minmax / params   bounding box -> grid origin and dimensions (the reference's :27-31), bucket geometry: a bucket is a block of
//                     2^sx x 8 x 8 voxels (sx = 3, or 4 when that leaves more than FE_NBMAX buckets)
//   count             every chunk of FE_CH points histograms its points over the cloud's buckets in LDS -> one row of a
//                     [chunk][bucket] table
//   colscan / bscan   column prefix over the chunks and prefix over the buckets -> where each chunk's points of each bucket go; one
//                     work item per non-empty bucket
//   scatter           second read of the points: 32-byte records (xyz, index in the cloud | features, labels) written behind LDS cursors,
//                     a bucket's records contiguous (order inside a bucket is whatever the LDS atomics give: the index travels)
//   reduce            one workgroup per bucket: LDS histogram over the bucket's <= 1024 voxels from the first half of every record, every voxel's members
//                     ranked by their index (input order), then the records read in place in that order (the workgroup has just streamed them: L2) for the
//                     sequential sums and the label vote; the bucket's rows (32 bytes: row + voxel id) go to the rows region, with its occupancy per local row (y, z)
//   rowpre / rowscan  number of occupied voxels in front of every (row, bucket) in key order (key = ix + nx (iy + ny iz): rows of x)
//   move              every bucket's rows to their final position
//
// HBM traffic: 12 N (minmax) + 12 N (count) + 28 N + 32 N (scatter) + 32 N + 32 M (reduce: every record once from HBM, its second reading from the L2; the rows) + 32 M + 28 M
// (move) bytes for N points and M voxels, against 28 (N + M) algorithmic.  The staged reduction of ssdr_tile_from_rooms_batch_dev (below) orders a room's buckets BEFORE the scatter and writes and
// reduces only the share p of the points that lies in stage 1's buckets: 12 N + 12 N + 28 N + 32 p N (scatter) + 32 p N + 32 p M (reduce) + (32 + 28) p M (move);
// p = 0.42 on the bench's rooms.  A room that goes on to stage 2 pays 28 N more (a second read of its points) for the other 32 (1 - p) N of records.  A call with a room
// plan (FePlan) starts at the order: the 12 N + 12 N of minmax and count were paid once, when the plan was built — and so were the scatter's 28 N + 32 N when the plan holds the
// rooms' records (the default): such a call moves 32 p N + 32 p M (reduce, its records read from the plan) + (32 + 28) p M (move), and a room that goes on to stage 2 pays no second read.  Clouds whose grid does not fit (more than FE_NBMAX buckets of 1024 voxels) or that
// hold a voxel of more than FE_CAP points are flagged (ssdr_grid_subsample_status) and belong to the sort-based entry point.
#include "ssdr_internal.hpp"
#include "block_prims.hpp"
#include "voxel_label.hpp"
#include "subsample_types.hpp"
#include "frontend.hpp"
#include <memory>

namespace ssdr {
namespace {

constexpr int FE_NBMAX = 16384;      // buckets per cloud: the count / scatter kernels keep one LDS word per bucket (64 KiB)
constexpr int FE_CH = 32768;         // points per chunk of the count / scatter kernels
constexpr int FE_NT = 1024;          // their workgroup size
constexpr int FE_PPT = 12, FE_SNT = 1024;      // points per thread and step of the scatter, its workgroup size: 12288 points per step leave ~12 records = three
                                              // whole lines in a bucket at a time, and one workgroup per CU halves the lines the L2 has open (PPT 4: 0.51 ms, 8: 0.44, 12: 0.36;
                                              // 512 threads x 24 the same, x 32 = the whole chunk in one step spills: 0.37)
constexpr int FE_LR = 64;            // local rows (y, z) of a bucket: 8 x 8
constexpr int FE_VMAX = 1024;        // voxels per bucket (sx <= 4)
constexpr int FE_RNT = 128;          // workgroup size of the reduction: 128 threads with eight records each (two waves per barrier; 256 threads: front end 1.154-1.161 against
                                     // 1.106-1.110 ms on one box; 512 threads were 13 % slower in round 4; 64 threads leave two waves per SIMD by LDS)
constexpr int FE_WAVES = 4;          // waves per SIMD asked of the reduction: what its registers give (5 / 6 spill 24 / 36 dwords: 0.45-0.51 against 0.45-0.46 ms)
constexpr int FE_WALK = 4;           // members of a voxel whose gathers the ordered walk keeps in flight
constexpr int FE_CAP = 1024;         // records of a bucket (or of a slice of it) the reduction orders in LDS at a time
constexpr int FE_RPT = FE_CAP / FE_RNT;
constexpr int FE_SLICES = 62;        // slices of a bucket with more than FE_CAP records
constexpr int FE_ROWCAP = FE_LR * FE_NBMAX;      // padded rows (y, z) per cloud: at most 64 per bucket column

struct FeGeom {
    float org[3]; float dl;
    int nx, ny, nz, sx;
    int nbx, nby, nbz, nb;
    int ok, n, pad0, pad1;
};
// one non-empty bucket: everything its workgroup needs in one 32-byte load
struct FeItem { unsigned base, n, rb, sx; float org[3]; float dl; };       // base: first record (absolute); rb = cloud << 16 | bucket

struct FeTab { int nr; int chunks_max; int ovf_cap; int n_total; int off[RADIX_MAX_SEG + 1]; };
struct FeTileInfo { int n, k1, k2, stage, reduced, pad0, pad1, pad2; };      // staged reduction, per room; stage: 0 = reduced whole without an order, 1..3 = the stage that was the last
// per-room count of the records the pruned scatter wrote (64-bit words behind the 64 int counters; zeroed by fe_params)
__host__ __device__ __forceinline__ unsigned long long* fe_scatter_counters(int* counters) { return reinterpret_cast<unsigned long long*>(counters + 64); }

// voxel coordinates of a point (grid_subsampling.cpp:53-56: floor((p - origin) / dl), the same fp32 operations); false when the point
// falls outside the grid the bounding box gives (a wrapped size_t in the reference: only NaNs and overflowing coordinates get here)
__device__ __forceinline__ bool fe_voxel(const FeGeom& g, float x, float y, float z, int& ix, int& iy, int& iz) {
    const float fx = floorf((x - g.org[0]) / g.dl), fy = floorf((y - g.org[1]) / g.dl), fz = floorf((z - g.org[2]) / g.dl);
    const bool ok = fx >= 0.f && fx < (float)g.nx && fy >= 0.f && fy < (float)g.ny && fz >= 0.f && fz < (float)g.nz;
    ix = (int)fx; iy = (int)fy; iz = (int)fz;
    return ok;
}
__device__ __forceinline__ int fe_bucket(const FeGeom& g, int ix, int iy, int iz) { return (ix >> g.sx) + g.nbx * ((iy >> 3) + g.nby * (iz >> 3)); }
// voxel of a record inside its bucket: x fastest, then the local row (y, z)
__device__ __forceinline__ int fe_vid(const FeItem& it, float x, float y, float z) {
    const int ix = (int)floorf((x - it.org[0]) / it.dl), iy = (int)floorf((y - it.org[1]) / it.dl), iz = (int)floorf((z - it.org[2]) / it.dl);
    return (ix & ((1 << it.sx) - 1)) | (((iy & 7) | ((iz & 7) << 3)) << it.sx);
}

__global__ __launch_bounds__(BS) void fe_minmax_partial(FeTab t, const float* __restrict__ P, float* partial) {
    const int r = blockIdx.y;
    gs_minmax_partial_body(P + 3 * (size_t)t.off[r], t.off[r + 1] - t.off[r], partial + (size_t)r * PB * 6);
}

// (float)(1.0 / (double)k), the factor the reference multiplies a voxel's position sums with (cloud.h:120), k <= FE_CAP: once per state
__global__ void fe_rcp_init(float* rcp) { const int k = blockIdx.x * blockDim.x + threadIdx.x; if (k <= FE_CAP) rcp[k] = k ? (float)(1.0 / (double)k) : 0.f; }

// one workgroup per cloud: grid origin / dimensions exactly as the reference derives them, bucket geometry, per-call counters
__global__ __launch_bounds__(BS) void fe_params(FeTab t, const float* partial, float dl, GsParams* prm, FeGeom* geom, int* counters) {
    __shared__ float s_mm[(BS / 64) * 6];
    const int r = blockIdx.x;
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = threadIdx.x; i < PB; i += BS) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { mn[d] = fminf(mn[d], partial[((size_t)r * PB + i) * 6 + d]); mx[d] = fmaxf(mx[d], partial[((size_t)r * PB + i) * 6 + 3 + d]); }
    }
    block_minmax3(mn, mx, s_mm);
    if (threadIdx.x == 0) {
        if (r == 0) { for (int i = 0; i < 64; ++i) counters[i] = 0; }         // [0] work items, [3] overflow rows; [32..56) the same per stage of the staged reduction
        fe_scatter_counters(counters)[r] = 0ull;
        GsParams p; FeGeom g;
        const float inv = 1 / dl;               // grid_subsampling.cpp:27-31
        float nd[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) { g.org[d] = floorf(mn[d] * inv) * dl; p.org[d] = g.org[d]; nd[d] = floorf((mx[d] - g.org[d]) / dl) + 1.f; }
        g.dl = dl; p.dl = dl;
        bool ok = nd[0] >= 1.f && nd[1] >= 1.f && nd[2] >= 1.f && nd[0] < 65536.f && nd[1] < 1.0e6f && nd[2] < 1.0e6f;      // false for NaNs too (x: 16-bit row prefixes)
        // the smallest coordinate must land in voxel 0 (floor(min * inv) * dl can round above min: the reference's size_t index then wraps)
#pragma unroll
        for (int d = 0; d < 3; ++d) ok = ok && floorf((mn[d] - g.org[d]) / dl) >= 0.f;
        g.nx = ok ? (int)nd[0] : 1; g.ny = ok ? (int)nd[1] : 1; g.nz = ok ? (int)nd[2] : 1;
        p.nx = (unsigned long long)g.nx; p.ny = (unsigned long long)g.ny; p.m = 0; p.status = 0; p.key_and = 0ull; p.key_or = ~0ull;
        g.nby = (g.ny + 7) >> 3; g.nbz = (g.nz + 7) >> 3;
        g.sx = 3; g.nbx = (g.nx + 7) >> 3;
        if ((long long)g.nbx * g.nby * g.nbz > FE_NBMAX) { g.sx = 4; g.nbx = (g.nx + 15) >> 4; }
        if ((long long)g.nbx * g.nby * g.nbz > FE_NBMAX) ok = false;
        g.nb = ok ? g.nbx * g.nby * g.nbz : 0;
        g.ok = ok ? 1 : 0; g.n = t.off[r + 1] - t.off[r]; g.pad0 = g.pad1 = 0;
        if (!ok) p.status = 2;
        prm[r] = p; geom[r] = g;
    }
}

// [chunk][bucket] point counts of one cloud; chunk c = points [c FE_CH, (c + 1) FE_CH)
__global__ __launch_bounds__(FE_NT) void fe_count(FeTab t, const float* __restrict__ P, const FeGeom* __restrict__ geom, GsParams* prm, unsigned* cntm) {
    __shared__ unsigned s_h[FE_NBMAX];
    const int r = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    const FeGeom g = geom[r];
    if (!g.ok || c * FE_CH >= g.n) return;
    for (int b = tid; b < g.nb; b += FE_NT) s_h[b] = 0u;
    __syncthreads();
    const float* Pr = P + 3 * (size_t)t.off[r];
    const int hi = min(g.n, (c + 1) * FE_CH);
    bool bad = false;
    for (int i = c * FE_CH + tid; i < hi; i += FE_NT) {
        int ix, iy, iz;
        if (fe_voxel(g, Pr[3 * (size_t)i], Pr[3 * (size_t)i + 1], Pr[3 * (size_t)i + 2], ix, iy, iz)) atomicAdd(&s_h[fe_bucket(g, ix, iy, iz)], 1u);
        else bad = true;
    }
    if (bad) atomicOr(&prm[r].status, 2);
    __syncthreads();
    unsigned* row = cntm + ((size_t)r * t.chunks_max + c) * FE_NBMAX;
    for (int b = tid; b < g.nb; b += FE_NT) row[b] = s_h[b];
}

// exclusive scan over the workgroup; returns the exclusive prefix and the total
__device__ __forceinline__ unsigned long long fe_block_scan(unsigned long long v, unsigned long long* s_w, int nt, unsigned long long& total) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    unsigned long long incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long y = __shfl_up(incl, o); if (lane >= o) incl += y; }
    if (lane == 63) s_w[wid] = incl;
    __syncthreads();
    unsigned long long wbase = 0, tot = 0;
    for (int w = 0; w < nt / 64; ++w) { const unsigned long long cw = s_w[w]; if (w < wid) wbase += cw; tot += cw; }
    __syncthreads();
    total = tot;
    return wbase + incl - v;
}

// one thread per bucket: cntm[c][b] becomes the number of points of bucket b in the chunks before c; the bucket's total
__global__ __launch_bounds__(BS) void fe_colscan(FeTab t, const FeGeom* __restrict__ geom, unsigned* cntm, unsigned* tot) {
    const int r = blockIdx.y, b = blockIdx.x * BS + threadIdx.x;
    const FeGeom g = geom[r];
    if (!g.ok || b >= g.nb) return;
    const int nchunk = (g.n + FE_CH - 1) / FE_CH;
    unsigned* cm = cntm + (size_t)r * t.chunks_max * FE_NBMAX + b;
    unsigned run = 0;
    for (int c0 = 0; c0 < nchunk; c0 += 8) {
        unsigned v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = c0 + u < nchunk ? cm[(size_t)(c0 + u) * FE_NBMAX] : 0u;
#pragma unroll
        for (int u = 0; u < 8; ++u) if (c0 + u < nchunk) { cm[(size_t)(c0 + u) * FE_NBMAX] = run; run += v[u]; }
    }
    tot[(size_t)r * FE_NBMAX + b] = run;
}

// one workgroup per cloud: boff[b] = where bucket b starts among the cloud's records; one work item per non-empty bucket
__global__ __launch_bounds__(FE_NT) void fe_bscan(FeTab t, const FeGeom* __restrict__ geom, const unsigned* __restrict__ tot, unsigned* boff, FeItem* items, int* counters) {
    __shared__ unsigned long long s_w[FE_NT / 64];
    __shared__ unsigned s_base;
    const int r = blockIdx.x, tid = threadIdx.x;
    const FeGeom g = geom[r];
    unsigned* bo = boff + (size_t)r * (FE_NBMAX + 1);
    if (!g.ok) { if (tid == 0) bo[0] = 0u; return; }
    unsigned long long carry = 0;          // records << 20 | non-empty buckets of the step
    for (int b0 = 0; b0 < g.nb; b0 += FE_NT) {
        const int b = b0 + tid;
        const unsigned n = b < g.nb ? tot[(size_t)r * FE_NBMAX + b] : 0u;
        unsigned long long total;
        const unsigned long long ex = fe_block_scan(((unsigned long long)n << 20) | (n ? 1ull : 0ull), s_w, FE_NT, total);
        const unsigned start = (unsigned)((carry + ex) >> 20);
        if (b < g.nb) bo[b] = start;
        const unsigned nne = (unsigned)(total & 0xfffffull);
        if (tid == 0) s_base = nne ? (unsigned)atomicAdd(&counters[0], (int)nne) : 0u;
        __syncthreads();
        if (n) {
            FeItem it; it.base = (unsigned)t.off[r] + start; it.n = n; it.rb = ((unsigned)r << 16) | (unsigned)b; it.sx = (unsigned)g.sx;
            it.org[0] = g.org[0]; it.org[1] = g.org[1]; it.org[2] = g.org[2]; it.dl = g.dl;
            items[s_base + (unsigned)(ex & 0xfffffull)] = it;
        }
        carry += total & ~0xfffffull;
        __syncthreads();
    }
    if (tid == 0) bo[g.nb] = (unsigned)(carry >> 20);
}

// A call with a room plan: what fe_params and fe_bscan leave per call, from the plan (one workgroup per cloud).  The per-call counters start as fe_params
// starts them, with the whole-room item count fe_bscan reached, and the caller's prm as fe_params / fe_count left it (m = 0, the status bits, the grid).
__global__ __launch_bounds__(64) void fe_plan_begin(const GsParams* __restrict__ plan_prm, const int* __restrict__ plan_counters, GsParams* prm, int* counters) {
    const int r = blockIdx.x, tid = threadIdx.x;
    if (r == 0) counters[tid] = tid == 0 ? plan_counters[0] : 0;
    if (tid == 0) { fe_scatter_counters(counters)[r] = 0ull; prm[r] = plan_prm[r]; }
}

// second read of the points: packed records behind the LDS cursors of this chunk, FE_PPT points per thread and step (their loads issued
// together).  The kernel runs at the rate the memory system takes scattered 32-byte writes: what helps is more records per bucket and step (lines
// complete before the L2 drops them); issuing a step's loads ahead of the previous step's stores changed nothing.  FD / LD >= 0: row layout known at compile time (straight-line loads).
struct FePoint { float x, y, z; uint32_t w[4]; };
// the value of lane ^ 1: a DPP move (quad_perm [1,0,3,2]) instead of a trip through the LDS crossbar, which the cursors' atomics already use
__device__ __forceinline__ uint32_t fe_swap1(uint32_t v) {
#ifndef HIPEMU
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
#else
    return (uint32_t)__shfl_xor((int)v, 1);
#endif
}
template <int FD, int LD>
__device__ __forceinline__ FePoint fe_load_point(const float* __restrict__ Pr, const float* __restrict__ Fr, const int* __restrict__ Cr, int fdim, int ldim, int i) {
    FePoint pt;
    pt.x = Pr[3 * (size_t)i]; pt.y = Pr[3 * (size_t)i + 1]; pt.z = Pr[3 * (size_t)i + 2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t v = 0;
        if (FD >= 0) { if (q < FD) v = __float_as_uint(Fr[(size_t)i * FD + q]); else if (q - FD < LD) v = (uint32_t)Cr[(size_t)i * LD + (q - FD)]; }
        else { if (q < fdim) v = __float_as_uint(Fr[(size_t)i * fdim + q]); else if (q - fdim < ldim) v = (uint32_t)Cr[(size_t)i * ldim + (q - fdim)]; }
        pt.w[q] = v;
    }
    return pt;
}
constexpr unsigned FE_NOSLOT = 0xffffffffu;      // no record for this point; as a cursor: a bucket this pass does not write (offsets stay <= 0x3fffffff)
// one record to its slot
__device__ __forceinline__ void fe_store_record(uint4* R, const FePoint& pt, int i, unsigned slot, int tid) {
    // (non-temporal stores here: 2.6x slower — the L2 merges the two halves of a record, and little else: a chunk adds ~4 records to a bucket)
    // the two 16-byte halves of a record leave from ADJACENT lanes, so a store instruction carries 32 runs of 32 bytes instead of 64 of 16: lanes
    // 2j and 2j + 1 swap a half each (the even lane hands over its second half and takes the odd lane's first)
    const bool odd = tid & 1;
    const uint32_t a0 = __float_as_uint(pt.x), a1 = __float_as_uint(pt.y), a2 = __float_as_uint(pt.z), a3 = (uint32_t)i;
    const uint32_t b0 = pt.w[0], b1 = pt.w[1], b2 = pt.w[2], b3 = pt.w[3];
    const uint32_t g0 = fe_swap1(odd ? a0 : b0), g1 = fe_swap1(odd ? a1 : b1), g2 = fe_swap1(odd ? a2 : b2), g3 = fe_swap1(odd ? a3 : b3);
    const unsigned pslot = fe_swap1(slot);
    const unsigned se = odd ? pslot : slot, so = odd ? slot : pslot;          // the even lane's record, the odd lane's record
    if (se != FE_NOSLOT) R[2 * (size_t)se + (odd ? 1 : 0)] = odd ? make_uint4(g0, g1, g2, g3) : make_uint4(a0, a1, a2, a3);
    if (so != FE_NOSLOT) R[2 * (size_t)so + (odd ? 1 : 0)] = odd ? make_uint4(b0, b1, b2, b3) : make_uint4(g0, g1, g2, g3);
}
// MODE 0: every bucket (ssdr_grid_subsample_batch_dev, and the records of a room plan).  The staged reduction knows stage 1's buckets before
// a record is written (fe_tile_order runs first and leaves one flag per bucket), so MODE 1 writes the records of the flagged buckets only: the cursor of every
// other bucket is FE_NOSLOT from the start, and a point that finds it gets no slot and no store (a lane pair with one such point stores one record's two halves).  The layout
// (boff, cntm) is that of MODE 0: an unflagged bucket's range is simply not written, and nobody reads it — unless its room goes on to stage 2: MODE 2, launched behind
// fe_tile_plan<2>, then writes exactly the points of the UNflagged buckets of such rooms (a second read of the room's points) and leaves at once for every other room.
// Both count the records they wrote per room (one atomic per workgroup: ssdr_tile_from_rooms_scatter_stats).  All twelve points' loads still leave together, features
// and labels of skipped points included: loading those only for points with a slot (a second round of loads behind the cursors) read 0.018 ms per step slower in
// every one of five interleaved runs (profiles/r09_frontend_scatter_prune.md): the rooms' rows are shuffled, so hardly a 32-byte sector is spared.
template <int FD, int LD, int MODE>
__global__ __launch_bounds__(FE_SNT) void fe_scatter(FeTab t, const float* __restrict__ P, const float* __restrict__ F, int fdim, const int* __restrict__ cls, int ldim,
                                                    const FeGeom* __restrict__ geom, const unsigned* __restrict__ cntm, const unsigned* __restrict__ boff, uint4* rec,
                                                    const unsigned char* __restrict__ flag, const FeTileInfo* __restrict__ info, unsigned long long* nscat) {
    __shared__ unsigned s_cur[FE_NBMAX];
    const int r = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    const FeGeom g = geom[r];
    if (!g.ok || c * FE_CH >= g.n) return;
    if (MODE == 2 && info[r].stage < 2) return;          // stage 1 sufficed (or took the room whole)
    const unsigned* row = cntm + ((size_t)r * t.chunks_max + c) * FE_NBMAX;
    const unsigned* bo = boff + (size_t)r * (FE_NBMAX + 1);
    if (MODE == 0) { for (int b = tid; b < g.nb; b += FE_SNT) s_cur[b] = bo[b] + row[b]; }
    else {
        const unsigned char* fl = flag + (size_t)r * FE_NBMAX;
        for (int b = tid; b < g.nb; b += FE_SNT) s_cur[b] = (fl[b] != 0) == (MODE == 1) ? bo[b] + row[b] : FE_NOSLOT;
    }
    __syncthreads();
    const size_t o = (size_t)t.off[r];
    const float* Pr = P + 3 * o;
    const float* Fr = F ? F + o * fdim : nullptr;
    const int* Cr = cls ? cls + o * ldim : nullptr;
    uint4* R = rec + 2 * o;
    const int lo = c * FE_CH, hi = min(g.n, (c + 1) * FE_CH);
    unsigned kept = 0;
    for (int i0 = lo; i0 < hi; i0 += FE_SNT * FE_PPT) {
        FePoint cur[FE_PPT];
#pragma unroll
        for (int k = 0; k < FE_PPT; ++k) cur[k] = fe_load_point<FD, LD>(Pr, Fr, Cr, fdim, ldim, min(i0 + k * FE_SNT + tid, hi - 1));
#pragma unroll
        for (int k = 0; k < FE_PPT; ++k) {
            const int i = i0 + k * FE_SNT + tid;
            int ix, iy, iz;
            unsigned slot = FE_NOSLOT;
            if (i < hi && fe_voxel(g, cur[k].x, cur[k].y, cur[k].z, ix, iy, iz)) {
                unsigned* cp = &s_cur[fe_bucket(g, ix, iy, iz)];
                if (MODE == 0 || *cp != FE_NOSLOT) slot = atomicAdd(cp, 1u);
            }
            if (MODE != 0) kept += slot != FE_NOSLOT ? 1u : 0u;
            fe_store_record(R, cur[k], i, slot, tid);
        }
    }
    if (MODE != 0) {          // the workgroup's records: the cursors are done with, their first words carry the waves' sums
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) kept += __shfl_xor(kept, m);
        __syncthreads();
        if ((tid & 63) == 0) s_cur[tid >> 6] = kept;
        __syncthreads();
        if (tid == 0) {
            unsigned long long sum = 0;
            for (int w = 0; w < FE_SNT / 64; ++w) sum += s_cur[w];
            if (sum) atomicAdd(&nscat[r], sum);
        }
    }
}

// ---- reduction: one workgroup per bucket ------------------------------------------------------------------------------------
struct FeRedArgs {
    FeTab t; const FeItem* items; GsParams* prm; int* counters; const float* rcp;
    const uint4* rec; uint4* rows; unsigned* nocc; unsigned* trow; unsigned char* lrc; int fdim, ldim;
};
// rec: the records, read only — the call's own scatter left them in the per-stream buffer, or a room plan holds them (FePlan::rec).  rows: where the rows region
// starts (ovf_cap = n_total rows: at most one per point): behind the n_total records of the per-stream buffer, or that whole buffer when the records are the plan's.

// The ordered walk reads the records where the scatter left them (the workgroup has just streamed them: L2) and every bucket's rows go to the rows region: 19 KB of
// LDS per workgroup, the occupancy is the registers'.  (A variant that also kept the bucket's records in LDS and wrote its rows over them — 51 KB per workgroup, three
// workgroups per CU — measured on one box: fe_reduce 0.51-0.56 against 0.45-0.46 ms, front end 1.23-1.26 against 1.16-1.18 ms, 178.2-178.7 against 180.9-181.8 Mpoints/s.)
struct FeRedLds {
    unsigned midx[FE_CAP];                 // per voxel segment: the members' indices, in arrival order
    unsigned short perm[FE_CAP];           // per voxel segment: the members' positions among the bucket's records, by ascending index (input order)
    unsigned cnt[FE_VMAX + 1];             // histogram, then start of every voxel's segment
    union {
        unsigned fill[FE_VMAX];            // slices: members of a voxel seen so far (while a slice's records arrive)
        unsigned short slow[2 * FE_VMAX];  // row halves with a label column to settle from the members: row | half << 10 | columns << 11 (while the voxels are walked)
    };
    unsigned short ovid[FE_VMAX];          // the occupied voxels, ascending
    unsigned short orank[FE_VMAX + 2];     // occupied voxels in front of a voxel
    unsigned short slice[FE_SLICES + 2];
    unsigned long long sw[FE_RNT / 64];
    int nslice, bad, nslow; unsigned ovf;
};

// A label column's vote from the members themselves (labels outside [0,13), more than 255 members): rare, kept out of line so that its
// tables do not weigh on the reduction's registers
__device__ __attribute__((noinline)) int fe_label_exact(const uint32_t* W, const unsigned short* perm, int word, int s, int e, int* status) {
    auto getl = [&](int j) { return (int)W[(size_t)perm[j] * 8 + word]; };
    int best = voxel_label_fast_t(getl, s, e);
    if (best < 0) best = voxel_label_t(getl, s, e, status);
    return best;
}

// Rows o_begin .. o_end - 1 of the bucket.  TWO lanes per occupied voxel walk its members in input order (L.perm), 16 bytes per member and
// lane: the even lane owns words 0..3 of the row (x, y, z and the voxel id in place of the record's index), the odd lane words 4..7 (features, labels).  Sums are taken
// sequentially in that order (what makes them the reference's, grid_subsampling.cpp:59-70); a label word is voted on with packed byte
// counters (labels 0..15; pk0: 0..7, pk1: 8..15) and the step at which a label is first seen kept the same way (fp0 / fp1): the
// reference's vote takes the first maximum in the iteration order of its unordered_map<int,int>, which for labels in [0,13) is "first
// seen last" (voxel_label.hpp).  Labels outside [0,13) or more than 255 members: noted in L.slow, settled by a second pass.
// s0 = start of the slice's first segment.  FD / LD >= 0: row layout known at compile time.
template <int FD, int LD>
__device__ __forceinline__ void fe_reduce_voxels(FeRedLds& L, const FeRedArgs& a, int* status, int o_begin, int o_end, unsigned s0, uint4* rows, const uint4* __restrict__ Rg) {
    const int fdim = FD >= 0 ? FD : a.fdim, ldim = LD >= 0 ? LD : a.ldim;
    const int half = (int)threadIdx.x & 1;
    for (int o = o_begin + ((int)threadIdx.x >> 1); o < o_end; o += FE_RNT / 2) {
        const int v = L.ovid[o];
        const int s = (int)(L.cnt[v] - s0), e = (int)(L.cnt[v + 1] - s0), count = e - s;
        const float rc = a.rcp[count];                       // (float)(1.0 / (double)count): cloud.h:120 via grid_subsampling.cpp:87 (the load travels during the walk)
        float f[4] = {0.f, 0.f, 0.f, 0.f};
        unsigned long long pk0[4] = {0ull, 0ull, 0ull, 0ull}, pk1[4] = {0ull, 0ull, 0ull, 0ull}, fp0[4] = {0ull, 0ull, 0ull, 0ull}, fp1[4] = {0ull, 0ull, 0ull, 0ull};
        bool big = false;
        for (int j = s; j < e; j += FE_WALK) {               // FE_WALK members' positions, then their halves, in flight together
            int p[FE_WALK]; uint4 w[FE_WALK];
#pragma unroll
            for (int h = 0; h < FE_WALK; ++h) p[h] = L.perm[min(j + h, e - 1)];
#pragma unroll
            for (int h = 0; h < FE_WALK; ++h) w[h] = Rg[2 * (size_t)p[h] + half];
#pragma unroll
            for (int h = 0; h < FE_WALK; ++h) {
                if (j + h < e) {
                    const uint32_t ww[4] = {w[h].x, w[h].y, w[h].z, w[h].w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        // record word half * 4 + q: words 0..2 positions, word 3 the index (no sum); words 4.. the fdim features, then the ldim labels
                        const bool is_sum = half == 0 ? q < 3 : q < fdim, is_lab = half == 1 && q >= fdim && q < fdim + ldim;
                        if (is_sum) f[q] += __uint_as_float(ww[q]);
                        else if (is_lab) {
                            const unsigned Lb = ww[q], sh = (Lb & 7u) * 8u;
                            big |= Lb >= 13u;
                            const bool lo = Lb < 8u, hi = Lb >= 8u && Lb < 16u;
                            const unsigned long long cur = lo ? pk0[q] : pk1[q];
                            const unsigned long long first = ((cur >> sh) & 0xffull) ? 0ull : ((unsigned long long)((j + h - s) & 0xff) << sh);
                            const unsigned long long inc = 1ull << sh;
                            pk0[q] += lo ? inc : 0ull; pk1[q] += hi ? inc : 0ull;
                            fp0[q] |= lo ? first : 0ull; fp1[q] |= hi ? first : 0ull;
                        }
                    }
                }
            }
        }
        uint32_t out[4] = {0u, 0u, 0u, 0u};
        unsigned slow = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (half == 0) out[q] = q < 3 ? __float_as_uint(f[q] * rc) : (uint32_t)v;          // the row: (x, y, z, voxel id | features, labels)
            else if (q < fdim) out[q] = __float_as_uint(f[q] / (float)count);          // :90-94
            else if (q < fdim + ldim) {
                int best = 0, bestc = -1, bestf = -1;          // largest count; among equals the label first seen last
#pragma unroll
                for (int l = 0; l < 13; ++l) {
                    const int ck = (int)(((l < 8 ? pk0[q] : pk1[q]) >> ((l & 7) * 8)) & 0xffull);
                    const int fk = (int)(((l < 8 ? fp0[q] : fp1[q]) >> ((l & 7) * 8)) & 0xffull);
                    if (ck > bestc || (ck == bestc && fk > bestf)) { bestc = ck; bestf = fk; best = l; }
                }
                if (big || count > 255) slow |= 1u << q;          // labels outside [0,13) or byte counters too small: the exact routines
                out[q] = (uint32_t)best;
            }
        }
        if (slow) L.slow[atomicAdd(&L.nslow, 1)] = (unsigned short)((o - o_begin) | (half << 10) | (slow << 11));
        rows[2 * (size_t)o + half] = make_uint4(out[0], out[1], out[2], out[3]);
    }
    __syncthreads();
    if (L.nslow) {
        const uint32_t* W = reinterpret_cast<const uint32_t*>(Rg);
        for (int t = (int)threadIdx.x; t < L.nslow; t += FE_RNT) {
            const int o = o_begin + (L.slow[t] & 1023), hf = (L.slow[t] >> 10) & 1;
            const unsigned mask = L.slow[t] >> 11;
            const int v = L.ovid[o];
            const int s = (int)(L.cnt[v] - s0), e = (int)(L.cnt[v + 1] - s0);
            for (int q = 0; q < 4; ++q) if ((mask >> q) & 1u)
                reinterpret_cast<uint32_t*>(rows)[(size_t)o * 8 + hf * 4 + q] = (uint32_t)fe_label_exact(W, L.perm, hf * 4 + q, s, e, status);
        }
    }
}

// segment starts, the occupied voxels and their ranks from the histogram in L.cnt (V = 512 or 1024 voxels)
__device__ __forceinline__ void fe_segments(FeRedLds& L, int V) {
    constexpr int EM = FE_VMAX / FE_RNT;
    const int tid = threadIdx.x, E = V / FE_RNT;           // 2 or 4 voxels per thread (256 threads)
    unsigned c4[EM]; unsigned tot = 0, occ = 0;
#pragma unroll
    for (int k = 0; k < EM; ++k) { c4[k] = k < E ? L.cnt[tid * E + k] : 0u; tot += c4[k]; occ += c4[k] ? 1u : 0u; if (c4[k] > (unsigned)FE_CAP) L.bad = 1; }
    unsigned long long total;
    const unsigned long long ex = fe_block_scan(((unsigned long long)tot << 20) | occ, L.sw, FE_RNT, total);
    unsigned st = (unsigned)(ex >> 20), orr = (unsigned)(ex & 0xfffffull);
#pragma unroll
    for (int k = 0; k < EM; ++k) if (k < E) {
        const int v = tid * E + k;
        L.cnt[v] = st; L.orank[v] = (unsigned short)orr;
        if (c4[k]) { L.ovid[orr] = (unsigned short)v; ++orr; }
        st += c4[k];
    }
    if (tid == FE_RNT - 1) { L.cnt[V] = st; L.orank[V] = (unsigned short)orr; }
    __syncthreads();
}

// One workgroup per bucket (work items dealt round robin).  A bucket of at most FE_CAP records has the first halves of its records read once, the voxel
// histogram's returning atomics handing every record its arrival slot inside its voxel.  A larger bucket is cut into slices of consecutive voxels (at most
// FE_CAP records each) after a histogram pass, and its first halves are read again once per slice.  (Where the time goes, by clock stamps around the phases: load +
// histogram 27 %, segments 6 %, rank 15 %, ordered walk 44 %, tail 7 %.)
template <int FD, int LD>
__global__ __launch_bounds__(FE_RNT) SSDR_WAVES_PER_EU(FE_WAVES) void fe_reduce(FeRedArgs a) {
    __shared__ FeRedLds L;
    const int tid = threadIdx.x;
    const int nitems = a.counters[0];
    for (int i = blockIdx.x; i < nitems; i += (int)gridDim.x) {
        const FeItem it = a.items[i];
        const int r = (int)(it.rb >> 16), b = (int)(it.rb & 0xffffu);
        GsParams* prm = a.prm + r;
        const int n = (int)it.n, V = FE_LR << it.sx;
        const bool fast = n <= FE_CAP;
        const uint4* R = a.rec + 2 * (size_t)it.base;
        for (int v = tid; v <= V; v += FE_RNT) L.cnt[v] = 0;
        if (tid == 0) { L.bad = 0; L.nslow = 0; }
        __syncthreads();
        // histogram over the bucket's voxels; FE_RPT records per thread, their loads issued together.  The fast path keeps every record's
        // voxel and arrival slot inside the voxel (what the returning atomic hands out) in registers until the segments are known
        int vv[FE_RPT]; unsigned uu[FE_RPT], ix[FE_RPT];
#pragma unroll
        for (int k = 0; k < FE_RPT; ++k) { vv[k] = 0; uu[k] = 0u; ix[k] = 0u; }
        if (fast) {
            // (x, y, z, index) is the FIRST half of a record: this pass reads 16 of its 32 bytes
            uint4 r0[FE_RPT];
#pragma unroll
            for (int k = 0; k < FE_RPT; ++k) r0[k] = R[2 * (size_t)min(tid + k * FE_RNT, n - 1)];
#pragma unroll
            for (int k = 0; k < FE_RPT; ++k) {
                vv[k] = fe_vid(it, __uint_as_float(r0[k].x), __uint_as_float(r0[k].y), __uint_as_float(r0[k].z));
                ix[k] = r0[k].w;
                if (tid + k * FE_RNT < n) uu[k] = atomicAdd(&L.cnt[vv[k]], 1u);
            }
        } else {
            for (int p0 = 0; p0 < n; p0 += FE_CAP) {
                uint4 r0[FE_RPT];
#pragma unroll
                for (int k = 0; k < FE_RPT; ++k) r0[k] = R[2 * (size_t)min(p0 + tid + k * FE_RNT, n - 1)];
#pragma unroll
                for (int k = 0; k < FE_RPT; ++k)
                    if (p0 + tid + k * FE_RNT < n) atomicAdd(&L.cnt[fe_vid(it, __uint_as_float(r0[k].x), __uint_as_float(r0[k].y), __uint_as_float(r0[k].z))], 1u);
            }
        }
        __syncthreads();
        fe_segments(L, V);
        const int nocc = L.orank[V];
        unsigned sg[FE_RPT], eg[FE_RPT];
#pragma unroll
        for (int k = 0; k < FE_RPT; ++k) { sg[k] = 0u; eg[k] = 0u; }
        if (fast) {          // every voxel's member indices, in arrival order
#pragma unroll
            for (int k = 0; k < FE_RPT; ++k) {
                sg[k] = L.cnt[vv[k]]; eg[k] = L.cnt[vv[k] + 1];
                if (tid + k * FE_RNT < n) L.midx[sg[k] + uu[k]] = ix[k];
            }
        }
        if (tid == 0) {
            if (fast) { L.nslice = 1; L.slice[0] = 0; L.slice[1] = (unsigned short)V; }
            // the bucket's place in the rows region
            const unsigned at = (unsigned)atomicAdd(&a.counters[3], nocc);
            L.ovf = at + (unsigned)nocc <= (unsigned)a.t.ovf_cap ? at : 0xffffffffu;
            if (L.ovf == 0xffffffffu) L.bad = 1;
            if (!fast) {
                int ns = 0, v = 0; L.slice[0] = 0;
                while (v < V && ns < FE_SLICES) {
                    const unsigned s0 = L.cnt[v]; int w = v;
                    while (w < V && L.cnt[w + 1] - s0 <= (unsigned)FE_CAP) ++w;
                    if (w == v) { L.bad = 1; break; }
                    v = w; L.slice[++ns] = (unsigned short)v;
                }
                if (v < V) L.bad = 1;
                L.nslice = ns;
            }
        }
        __syncthreads();
        if (fast) {          // every member's rank by index inside its voxel = its place in the order the reference adds the members in
#pragma unroll
            for (int k = 0; k < FE_RPT; ++k) {
                if (tid + k * FE_RNT < n) {
                    unsigned rank = 0;
                    for (unsigned j0 = sg[k]; j0 < eg[k]; j0 += 8) {          // eight list entries in flight
                        unsigned m8[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) m8[u] = L.midx[min(j0 + u, eg[k] - 1)];
#pragma unroll
                        for (int u = 0; u < 8; ++u) rank += (j0 + u < eg[k] && m8[u] < ix[k]) ? 1u : 0u;
                    }
                    L.perm[sg[k] + rank] = (unsigned short)(tid + k * FE_RNT);
                }
            }
            __syncthreads();
        }
        const size_t tb = (size_t)r * FE_NBMAX + b;
        if (L.bad) {           // a voxel of more than FE_CAP points (or more slices / overflow rows than there is room for): not this entry point's case
            if (tid == 0) { atomicOr(&prm->status, 4); a.nocc[tb] = 0u; a.trow[tb] = 0u; }          // (no rows: what makes fe_move skip the bucket)
            for (int l = tid; l < FE_LR; l += FE_RNT) a.lrc[tb * FE_LR + l] = 0;
        } else {
            uint4* rows = a.rows + 2 * (size_t)L.ovf;
            for (int si = 0; si < L.nslice; ++si) {
                const int v0 = L.slice[si], v1 = L.slice[si + 1];
                const unsigned s0 = L.cnt[v0];
                const int ns = (int)(L.cnt[v1] - s0);
                if (ns > 0 && !fast) {          // the slice's records, read again; then L.midx / L.perm as the fast path leaves them
                    __syncthreads();
                    for (int v = v0 + tid; v < v1; v += FE_RNT) L.fill[v] = 0u;
                    __syncthreads();
                    for (int p0 = 0; p0 < n; p0 += FE_CAP) {
                        uint4 q0[FE_RPT];
#pragma unroll
                        for (int k = 0; k < FE_RPT; ++k) q0[k] = R[2 * (size_t)min(p0 + tid + k * FE_RNT, n - 1)];
#pragma unroll
                        for (int k = 0; k < FE_RPT; ++k) {
                            const int v = fe_vid(it, __uint_as_float(q0[k].x), __uint_as_float(q0[k].y), __uint_as_float(q0[k].z));
                            if (p0 + tid + k * FE_RNT < n && v >= v0 && v < v1) {
                                const int q = p0 + tid + k * FE_RNT;          // the record's place among the bucket's own (<= FE_SLICES * FE_CAP < 65536)
                                // (index, position) pairs of a voxel, in arrival order: midx holds the indices, perm the positions until the ranks are known
                                const unsigned at = L.cnt[v] - s0 + atomicAdd(&L.fill[v], 1u);
                                L.midx[at] = q0[k].w; L.perm[at] = (unsigned short)q;
                            }
                        }
                    }
                    __syncthreads();
                    // ranks inside every voxel: one thread per voxel orders its (short) list by insertion
                    for (int v = v0 + tid; v < v1; v += FE_RNT) {
                        const int sb = (int)(L.cnt[v] - s0), eb = (int)(L.cnt[v + 1] - s0);
                        for (int x = sb + 1; x < eb; ++x) {
                            const unsigned ki = L.midx[x]; const unsigned short pi = L.perm[x];
                            int y = x - 1;
                            while (y >= sb && L.midx[y] > ki) { L.midx[y + 1] = L.midx[y]; L.perm[y + 1] = L.perm[y]; --y; }
                            L.midx[y + 1] = ki; L.perm[y + 1] = pi;
                        }
                    }
                    __syncthreads();
                    if (tid == 0) L.nslow = 0;      // (L.slow shares its storage with L.fill)
                    __syncthreads();
                }
                if (ns > 0) fe_reduce_voxels<FD, LD>(L, a, &prm->status, L.orank[v0], L.orank[v1], s0, rows, R);
            }
            // what the move needs: number of rows, where they are, occupied voxels per local row (y, z)
            if (tid == 0) { a.nocc[tb] = (unsigned)nocc; a.trow[tb] = L.ovf; }
            for (int l = tid; l < FE_LR; l += FE_RNT) a.lrc[tb * FE_LR + l] = (unsigned char)(L.orank[(l + 1) << it.sx] - L.orank[l << it.sx]);
        }
        __syncthreads();
    }
}

// occupied voxels of every padded row (iy, iz) of a cloud, and in front of every bucket inside its row (keys grow along x first)
__global__ __launch_bounds__(BS) void fe_rowpre(const FeGeom* __restrict__ geom, const unsigned* __restrict__ boff, const unsigned char* __restrict__ lrc,
                                                unsigned short* pre, unsigned* rowcnt) {
    const int r = blockIdx.y;
    const FeGeom g = geom[r];
    if (!g.ok) return;
    const int ry = g.nby * 8, prows = ry * g.nbz * 8;
    const unsigned* bo = boff + (size_t)r * (FE_NBMAX + 1);
    for (int pr = blockIdx.x * BS + threadIdx.x; pr < prows; pr += gridDim.x * BS) {
        const int iy = pr % ry, iz = pr / ry;
        const int l = (iy & 7) | ((iz & 7) << 3);
        const int b0 = g.nbx * ((iy >> 3) + g.nby * (iz >> 3));
        unsigned run = 0;
        for (int bx = 0; bx < g.nbx; ++bx) {
            const int b = b0 + bx;
            if (bo[b + 1] != bo[b]) {
                const size_t at = ((size_t)r * FE_NBMAX + b) * FE_LR + l;
                pre[at] = (unsigned short)run;
                run += lrc[at];
            }
        }
        rowcnt[(size_t)r * FE_ROWCAP + pr] = run;
    }
}

// one workgroup per cloud: rows in front of every padded row; the cloud's voxel count
__global__ __launch_bounds__(FE_NT) void fe_rowscan(const FeGeom* __restrict__ geom, unsigned* rowcnt, GsParams* prm, long long* out_m) {
    __shared__ unsigned long long s_w[FE_NT / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    const FeGeom g = geom[r];
    if (!g.ok) { if (tid == 0) { prm[r].m = 0; if (out_m) out_m[r] = 0; } return; }
    const int prows = g.nby * 8 * g.nbz * 8;
    unsigned* rc = rowcnt + (size_t)r * FE_ROWCAP;
    unsigned long long carry = 0;
    for (int p0 = 0; p0 < prows; p0 += FE_NT) {
        const int p = p0 + tid;
        const unsigned v = p < prows ? rc[p] : 0u;
        unsigned long long total;
        const unsigned long long ex = fe_block_scan((unsigned long long)v, s_w, FE_NT, total);
        if (p < prows) rc[p] = (unsigned)(carry + ex);
        carry += total;
    }
    if (tid == 0) { prm[r].m = (int)carry; if (out_m) out_m[r] = (long long)carry; }
}

// one wave per bucket: its rows to their final places
struct FeMoveArgs {
    FeTab t; const FeGeom* geom; const FeItem* items; const int* counters; const uint4* rows; const unsigned* nocc; const unsigned* trow;          // rows: FeRedArgs' rows; trow: a bucket's first row in it
    const unsigned char* lrc; const unsigned short* pre; const unsigned* rowbase; int fdim, ldim; float* out_p; float* out_f; int* out_c;
};
// FD / LD >= 0: row layout known at compile time (the hot path's 3 features + 1 label: one 12-byte store each for the position and the features instead of
// seven guarded 4-byte stores)
template <int FD, int LD>
__global__ __launch_bounds__(BS) void fe_move(FeMoveArgs a) {
    const int fdim = FD >= 0 ? FD : a.fdim, ldim = LD >= 0 ? LD : a.ldim;
    const int lane = threadIdx.x & 63;
    const int nw = a.counters[0], nwaves = (int)gridDim.x * (BS / 64);
    for (int tk = (int)blockIdx.x * (BS / 64) + (int)(threadIdx.x >> 6); tk < nw; tk += nwaves) {
        const unsigned we = a.items[tk].rb;
        const int r = (int)(we >> 16), b = (int)(we & 0xffffu);
        const FeGeom g = a.geom[r];
        const size_t tb = (size_t)r * FE_NBMAX + b;
        const int nocc = (int)a.nocc[tb];
        const uint4* rows = a.rows + 2 * (size_t)a.trow[tb];
        const int by = (b / g.nbx) % g.nby, bz = b / (g.nbx * g.nby);
        // occupied voxels of the bucket in front of every local row
        const unsigned mine = a.lrc[tb * FE_LR + lane];
        unsigned incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned y = __shfl_up(incl, o); if (lane >= o) incl += y; }
        const unsigned lpre = incl - mine;
        const unsigned short* pre = a.pre + tb * FE_LR;
        const unsigned* rb = a.rowbase + (size_t)r * FE_ROWCAP;
        const size_t o = (size_t)a.t.off[r];
        // a lane PAIR takes a row: the even lane its first half (x, y, z, voxel) and the position, the odd lane the second (features, labels) — a load
        // instruction then reads 32 whole rows as one contiguous kilobyte instead of 64 half rows at a stride of 32 bytes
        const int half = lane & 1, pl = lane >> 1;
        for (int j0 = 0; j0 < nocc; j0 += 64) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int j = j0 + 32 * h + pl;
                const bool on = j < nocc;
                uint4 rr = make_uint4(0, 0, 0, 0);
                if (on) rr = rows[2 * (size_t)j + half];
                const unsigned other = fe_swap1(rr.w);                      // (unconditional: a DPP move reads its partner lane only while that lane is active)
                const unsigned vw = half ? other : rr.w;                    // the voxel word lives in the first half
                const int l = on ? (int)(vw >> g.sx) : 0;
                const unsigned lp = __shfl(lpre, l);
                if (on) {
                    const int iy = by * 8 + (l & 7), iz = bz * 8 + (l >> 3);
                    const size_t fin = o + rb[iy + g.nby * 8 * iz] + pre[l] + ((unsigned)j - lp);
                    if (!half) { a.out_p[3 * fin] = __uint_as_float(rr.x); a.out_p[3 * fin + 1] = __uint_as_float(rr.y); a.out_p[3 * fin + 2] = __uint_as_float(rr.z); }
                    else {
                        const uint32_t w[4] = {rr.x, rr.y, rr.z, rr.w};
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            if (k < fdim) a.out_f[fin * fdim + k] = __uint_as_float(w[k]);
                            else if (k - fdim < ldim) a.out_c[fin * ldim + (k - fdim)] = (int)w[k];
                        }
                    }
                }
            }
        }
    }
}

// ---- reduction of the buckets a tile can need only ------------------------------------------------------------------------------
// The hot path keeps num_points rows of a room: the barycentres nearest to a picked centre (tile.hip).  A barycentre lies in its voxel, so the
// least and greatest distance from the centre to a bucket's box bound every row the bucket can give BEFORE its records are read.  The room's
// non-empty buckets are ordered by that least distance, and fe_reduce (the same kernel: it only sees shorter work lists) runs in stages:
//   1  ranks [0, K1): K1 = the first rank at which the cumulative POINTS reach 6 num_points, widened to every rank whose least distance does not
//      exceed the greatest distance of a rank below it.  Enough for rooms of up to ~5 raw points per occupied voxel (S3DIS-like rooms at a 4 cm
//      grid hold 4 to 5), and it measures rho = points per occupied voxel around the centre exactly
//   check (after every stage): D = least distance of the first unreduced rank; the buckets whose greatest distance is below D hold exact row counts by
//      now.  At least num_points of them: every row of an unreduced bucket is strictly farther than num_points reduced rows and can neither enter
//      the tile nor tie with its last row: done.  Otherwise
//   2  ranks [K1, K2): K2 = the first rank at which the cumulative points reach 1.15 rho num_points, widened in the same way; if the check fails again
//   3  ranks [K2, n): the rest of the room (also what a room of fewer than num_points voxels ends with: the tile's padding branch).
// Unreduced buckets read as empty (nocc, lrc = 0) to fe_rowpre / fe_move: the rows that exist keep their key order, so the tile's tie rule
// (distance, then row) is the same relation on them.  The set of reduced buckets is a function of the inputs.  A call without a room plan keeps nothing
// between calls.  A room plan (FePlan, below) keeps what minmax / params / count / colscan / bscan leave — geom, cntm, tot, boff, the whole-room items and
// their count, every room's status and grid parameters — which is a function of the rooms' points and dl alone: a call with a plan reads those tables and
// writes none of them; everything that depends on the centres (the order, the flags, the records, nocc / lrc / trow, the rows) stays per call.
constexpr int FE_TO_NMAX = 8192;     // non-empty buckets of a room the order is sorted for (one LDS word each); a room with more is reduced whole
constexpr int FE_K1_MULT = 6;        // stage 1's size in tile sizes.  A stage costs the latency of a bucket's reduction (~100 us) however few buckets it holds, so the first stage should
                                     // usually be the last; a smaller one saves scattered writes, and a miss costs a second read of the room.  One box, step of 16 rooms: 2, not widened
                                     // (a probe for rho alone): 3.053-3.065 ms; 6: 2.962-2.971; 7 the same as 6; with the pruned scatter 4: 3.148-3.169
constexpr int FE_TO_KBITS = 14;     // low bits of a sort word: the bucket (FE_NBMAX = 2^14); above them 18 bits of the least distance's pattern
static_assert(FE_NBMAX == 1 << FE_TO_KBITS, "bucket bits of the order's sort words");
struct FeCentres { float c[3 * RADIX_MAX_SEG]; };
struct FeTileArgs {
    FeTab t; FeCentres cen; const FeGeom* geom; const unsigned* tot; const unsigned* boff; unsigned* nocc; unsigned char* lrc; unsigned char* flag;
    unsigned* okey; float* odmax; unsigned* ocum; FeItem* work; int* counters; FeTileInfo* info; int num_points;
    unsigned long long* given;          // fe_scatter_counters when the records are a room plan's and no scatter runs to count them (else NULL): per room, the records the stages were given
};
// per stage s = 1..3 a block of 8 counters behind the whole-room ones: [0] items of the stage's work list, [3] the overflow rows' cursor
__host__ __device__ __forceinline__ int* fe_stage_counters(int* counters, int stage) { return counters + 32 + 8 * (stage - 1); }

// Least and greatest squared distance from c to any barycentre of bucket b, safe against rounding on both sides:
//  - the box: voxels [i0, i1) per axis (clipped to the grid), org + i dl, taken in double (its own rounding is 2^-53 of a coordinate);
//  - a barycentre's distance from its voxel: the voxel test is floorf((p - org) / dl) in fp32 (two roundings, each <= u |p| with u = 2^-24), and a position sum is a
//    sequential fp32 sum of k <= FE_CAP terms times the rounded (float)(1 / k): |computed - mean| <= (k + 1) u max|p| to first order.  The margin takes
//    (FE_CAP + 8) 2 u A with A = the grid's largest |coordinate| (twice the first-order bound), and no less than dl / 4;
//  - tile_dist: (dx dx + dy dy) + dz dz in fp32 is five roundings deep per term (the difference, the square, two sums: all terms >= 0), so the
//    computed value lies within (1 +- u)^5 of the exact one: the bounds are scaled by 1 -+ 2^-20 = 16 u (the conversion to float costs one more u).
//    A least distance below 1e-30 counts as 0 (squares that underflow).
__device__ __forceinline__ void fe_bucket_bounds(const FeGeom& g, int b, const float* c, float& dmin2, float& dmax2) {
    const int bx = b % g.nbx, by = (b / g.nbx) % g.nby, bz = b / (g.nbx * g.nby);
    const int nd[3] = {g.nx, g.ny, g.nz};
    const int i0[3] = {bx << g.sx, by << 3, bz << 3};
    const int i1[3] = {min((bx + 1) << g.sx, g.nx), min((by + 1) << 3, g.ny), min((bz + 1) << 3, g.nz)};
    const double dl = (double)g.dl;
    double amax = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) amax = fmax(amax, fmax(fabs((double)g.org[d]), fabs((double)g.org[d] + (double)(nd[d] + 1) * dl)));
    const double margin = fmax(0.25 * dl, (double)(FE_CAP + 8) * (1.0 / 8388608.0) * amax);
    double lo2 = 0.0, hi2 = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double lo = (double)g.org[d] + (double)i0[d] * dl - margin, hi = (double)g.org[d] + (double)i1[d] * dl + margin, cd = (double)c[d];
        const double nearest = fmax(fmax(lo - cd, cd - hi), 0.0), farthest = fmax(fabs(cd - lo), fabs(hi - cd));
        lo2 += nearest * nearest; hi2 += farthest * farthest;
    }
    dmin2 = lo2 < 1.0e-30 ? 0.f : (float)(lo2 * (1.0 - 1.0 / 1048576.0));
    dmax2 = (float)(hi2 * (1.0 + 1.0 / 1048576.0));
}
__device__ __forceinline__ FeItem fe_tile_item(const FeTileArgs& a, const FeGeom& g, int r, int b) {
    FeItem it; it.base = (unsigned)a.t.off[r] + a.boff[(size_t)r * (FE_NBMAX + 1) + b]; it.n = a.tot[(size_t)r * FE_NBMAX + b];
    it.rb = ((unsigned)r << 16) | (unsigned)b; it.sx = (unsigned)g.sx;
    it.org[0] = g.org[0]; it.org[1] = g.org[1]; it.org[2] = g.org[2]; it.dl = g.dl;
    return it;
}

// One workgroup per room, after fe_bscan: every non-empty bucket reads as empty to the row kernels until a stage reduces it; the room's buckets by
// ascending least distance (sort word = 18 bits of the distance's pattern, rounded DOWN: still a lower bound | bucket: no two words are equal, the
// order is the inputs'), their greatest distances and running point counts in that order; stage 1's work items.  It needs geom, tot, boff and the centres, no
// record: it runs in front of the scatter and leaves it one flag per non-empty bucket, "stage 1 reduces this bucket" (every bucket of a room without an order).
__global__ __launch_bounds__(FE_NT) void fe_tile_order(FeTileArgs a) {
    __shared__ unsigned s_k[FE_TO_NMAX];
    __shared__ unsigned s_m;
    __shared__ unsigned long long s_w[FE_NT / 64];
    __shared__ int s_n, s_k1, s_base;
    const int r = blockIdx.x, tid = threadIdx.x;
    const FeGeom g = a.geom[r];
    int* cb = fe_stage_counters(a.counters, 1);
    FeTileInfo ti; ti.n = 0; ti.k1 = 0; ti.k2 = 0; ti.stage = 0; ti.reduced = 0; ti.pad0 = ti.pad1 = ti.pad2 = 0;
    if (!g.ok) { if (tid == 0) a.info[r] = ti; return; }          // (given[r] stays 0: such a room has no record)
    const float* c = a.cen.c + 3 * r;
    const unsigned* tot = a.tot + (size_t)r * FE_NBMAX;
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int b = tid; b < g.nb; b += FE_NT) {
        if (!tot[b]) continue;
        const size_t tb = (size_t)r * FE_NBMAX + b;
        a.nocc[tb] = 0u;
        uint4* z = reinterpret_cast<uint4*>(a.lrc + tb * FE_LR);
#pragma unroll
        for (int q = 0; q < FE_LR / 16; ++q) z[q] = make_uint4(0u, 0u, 0u, 0u);
        float dmin2, dmax2;
        fe_bucket_bounds(g, b, c, dmin2, dmax2);
        const int at = atomicAdd(&s_n, 1);
        if (at < FE_TO_NMAX) s_k[at] = (((__float_as_uint(dmin2) & 0x7fffffffu) >> 13) << FE_TO_KBITS) | (unsigned)b;
    }
    __syncthreads();
    const int n = s_n;
    __syncthreads();
    ti.n = n; ti.k1 = n; ti.k2 = n; ti.reduced = n;
    if (n > FE_TO_NMAX) {          // no order: the whole room in stage 1
        if (tid == 0) { s_base = atomicAdd(&cb[0], n); s_n = 0; }
        __syncthreads();
        for (int b = tid; b < g.nb; b += FE_NT) if (tot[b]) {
            a.work[(size_t)s_base + atomicAdd(&s_n, 1)] = fe_tile_item(a, g, r, b);
            if (a.flag) a.flag[(size_t)r * FE_NBMAX + b] = 1;
        }
        if (tid == 0) { a.info[r] = ti; if (a.given) a.given[r] = a.boff[(size_t)r * (FE_NBMAX + 1) + g.nb]; }          // every bucket is flagged: all of the room's records
        return;
    }
    // bitonic network over the next power of two (the padding sorts last); a rank-by-counting pass was tried: n^2 comparisons on ONE compute unit, 347 us
    // against this network's 50 us for the ~1500 buckets of a room
    int N2 = 2; while (N2 < n) N2 <<= 1;
    for (int i = n + tid; i < N2; i += FE_NT) s_k[i] = 0xffffffffu;
    if (tid == 0) s_k1 = n;
    __syncthreads();
    for (int k = 2; k <= N2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N2 / 2; i += FE_NT) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const unsigned x = s_k[lo], y = s_k[hi];
                if ((x > y) == !(lo & k)) { s_k[lo] = y; s_k[hi] = x; }
            }
            __syncthreads();
        }
    }
    const unsigned long long want = (unsigned long long)FE_K1_MULT * (unsigned long long)a.num_points;
    unsigned long long carry = 0;
    for (int i0 = 0; i0 < n; i0 += FE_NT) {
        const int i = i0 + tid;
        const int b = i < n ? (int)(s_k[i] & (FE_NBMAX - 1)) : 0;
        const unsigned long long pts = i < n ? tot[b] : 0u;
        unsigned long long total;
        const unsigned long long incl = carry + fe_block_scan(pts, s_w, FE_NT, total) + pts;
        if (i < n) {
            float dmin2, dmax2;
            fe_bucket_bounds(g, b, c, dmin2, dmax2);
            a.okey[(size_t)r * FE_NBMAX + i] = s_k[i]; a.odmax[(size_t)r * FE_NBMAX + i] = dmax2; a.ocum[(size_t)r * FE_NBMAX + i] = (unsigned)incl;
            if (incl - pts < want && incl >= want) s_k1 = i + 1;
        }
        carry += total;
    }
    __syncthreads();
    int k1 = s_k1;
    if (k1 < n) {         // every rank whose least distance does not exceed the greatest distance of a rank below k1: stage 1 can then pass the check itself
        if (tid == 0) s_m = 0u;
        __syncthreads();
        for (int i = tid; i < k1; i += FE_NT) {
            float dmin2, dmax2;
            fe_bucket_bounds(g, (int)(s_k[i] & (FE_NBMAX - 1)), c, dmin2, dmax2);
            atomicMax(&s_m, __float_as_uint(dmax2));
        }
        __syncthreads();
        const unsigned mq = s_m >> 13;
        unsigned long long v = 0, total;
        for (int i = tid; i < n; i += FE_NT) v += (s_k[i] >> FE_TO_KBITS) <= mq ? 1u : 0u;
        fe_block_scan(v, s_w, FE_NT, total);
        k1 = min(n, max((int)total, k1));
    }
    if (tid == 0) s_base = k1 ? atomicAdd(&cb[0], k1) : 0;
    __syncthreads();
    for (int i = tid; i < k1; i += FE_NT) a.work[(size_t)s_base + i] = fe_tile_item(a, g, r, (int)(s_k[i] & (FE_NBMAX - 1)));
    // what the pruned scatter goes by: every non-empty bucket's flag, written anew by every call (an empty bucket's is never looked at: no point finds its cursor)
    if (a.flag) for (int i = tid; i < n; i += FE_NT) a.flag[(size_t)r * FE_NBMAX + (s_k[i] & (FE_NBMAX - 1))] = i < k1 ? 1 : 0;
    ti.k1 = k1; ti.k2 = k1; ti.reduced = k1; ti.stage = 1;
    // what MODE 1 of the scatter would have counted: the points of the flagged buckets = of ranks [0, k1) (ocum: written above, in front of a barrier)
    if (tid == 0) { a.info[r] = ti; if (a.given) a.given[r] = k1 ? a.ocum[(size_t)r * FE_NBMAX + k1 - 1] : 0u; }
}

// One workgroup per room between two stages: what the stage before left (exact row counts in nocc) decides the next stage's ranks.
template <int STAGE>
__global__ __launch_bounds__(FE_NT) void fe_tile_plan(FeTileArgs a) {
    __shared__ unsigned long long s_w[FE_NT / 64];
    __shared__ unsigned s_u[2];
    __shared__ int s_base;
    const int r = blockIdx.x, tid = threadIdx.x;
    int* cb = fe_stage_counters(a.counters, STAGE);
    if (r == 0 && tid == 0) cb[3] = fe_stage_counters(a.counters, STAGE - 1)[3];          // the overflow rows go on where the stage before stopped
    const FeTileInfo ti = a.info[r];
    const int n = ti.n, k1 = ti.k1;
    if (k1 >= n) return;           // the room was reduced whole by stage 1 (or has no bucket)
    const unsigned* key = a.okey + (size_t)r * FE_NBMAX;
    const float* dmax = a.odmax + (size_t)r * FE_NBMAX;
    const unsigned* cum = a.ocum + (size_t)r * FE_NBMAX;
    const unsigned* nocc = a.nocc + (size_t)r * FE_NBMAX;
    int lo, hi;
    unsigned long long total;
    if (STAGE == 2) {
        // stage 1's ranks suffice when the room holds few enough points per voxel
        const float D1 = __uint_as_float((key[k1] >> FE_TO_KBITS) << 13);
        unsigned long long v = 0;
        for (int i = tid; i < k1; i += FE_NT) if (dmax[i] < D1) v += nocc[key[i] & (FE_NBMAX - 1)];
        fe_block_scan(v, s_w, FE_NT, total);
        if (total >= (unsigned long long)a.num_points) return;
        v = 0;
        for (int i = tid; i < k1; i += FE_NT) v += nocc[key[i] & (FE_NBMAX - 1)];
        fe_block_scan(v, s_w, FE_NT, total);
        // points of the ranks that are expected to hold 1.15 num_points occupied voxels at stage 1's points per voxel
        const double target = total ? 1.15 * (double)cum[k1 - 1] / (double)total * (double)a.num_points : 4.0e9;
        const unsigned tgt = target >= 4.0e9 ? 0xffffffffu : (unsigned)target + 1u;
        if (tid == 0) { s_u[0] = (unsigned)n; s_u[1] = 0u; }
        __syncthreads();
        for (int i = tid; i < n; i += FE_NT) if ((i ? cum[i - 1] : 0u) < tgt && cum[i] >= tgt) s_u[0] = (unsigned)(i + 1);
        __syncthreads();
        const int k2a = max((int)s_u[0], k1);
        for (int i = tid; i < k2a; i += FE_NT) atomicMax(&s_u[1], __float_as_uint(dmax[i]));          // (patterns of non-negative floats; a NaN's is above all: everything)
        __syncthreads();
        const unsigned mq = s_u[1] >> 13;
        v = 0;
        for (int i = tid; i < n; i += FE_NT) v += (key[i] >> FE_TO_KBITS) <= mq ? 1u : 0u;         // ranks whose least distance does not exceed that greatest one (a prefix: the order)
        fe_block_scan(v, s_w, FE_NT, total);
        lo = k1; hi = min(n, max((int)total, k2a));
        if (tid == 0) {
            a.info[r].k2 = hi; a.info[r].reduced = hi; a.info[r].stage = 2;
            if (a.given) a.given[r] += cum[n - 1] - (k1 ? cum[k1 - 1] : 0u);          // what MODE 2 would have counted: the points of the room's unflagged buckets, ranks [k1, n)
        }
    } else {
        const int k2 = ti.k2;
        if (k2 >= n) return;
        const float D = __uint_as_float((key[k2] >> FE_TO_KBITS) << 13);
        unsigned long long v = 0;
        for (int i = tid; i < k2; i += FE_NT) if (dmax[i] < D) v += nocc[key[i] & (FE_NBMAX - 1)];
        fe_block_scan(v, s_w, FE_NT, total);
        if (total >= (unsigned long long)a.num_points) return;
        lo = k2; hi = n;
        if (tid == 0) { a.info[r].reduced = n; a.info[r].stage = 3; }
    }
    if (tid == 0) s_base = hi > lo ? atomicAdd(&cb[0], hi - lo) : 0;
    __syncthreads();
    const FeGeom g = a.geom[r];
    for (int i = lo + tid; i < hi; i += FE_NT) a.work[(size_t)s_base + (i - lo)] = fe_tile_item(a, g, r, (int)(key[i] & (FE_NBMAX - 1)));
}

// ---- the launcher: environment, plan, launch ------------------------------------------------------------------------------------------------------
struct FeState {
    DevBuf partial, geom, cntm, tot, boff, items, counters, rec, nocc, trow, lrc, pre, rowcnt, rcp; bool rcp_ready = false;
    DevBuf okey, odmax, ocum, work, tinfo; int tile_clouds = 0;          // the staged reduction's tables; rooms of the last call if it was staged
    DevBuf flag; std::vector<long long> room_n;                          // [room][FE_NBMAX] bytes: stage 1 reduces this bucket; the last staged call's rooms' points
};

// the room table of a call, as every kernel takes it
int fe_room_table(const int64_t* room_off, size_t nr, FeTab& t) {
    t.nr = (int)nr;
    int maxn = 0;
    for (size_t r = 0; r < nr; ++r) {
        const long n = (long)(room_off[r + 1] - room_off[r]);
        if (n <= 0 || room_off[r + 1] > 0x3fffffff) { set_error("grid_subsample_batch: every cloud needs >= 1 point"); return n <= 0 ? SSDR_ERR_EMPTY : SSDR_ERR_INVALID; }
        t.off[r] = (int)room_off[r]; maxn = std::max(maxn, (int)n);
    }
    t.off[nr] = (int)room_off[nr];
    t.n_total = (int)room_off[nr];
    t.chunks_max = (maxn + FE_CH - 1) / FE_CH;
    t.ovf_cap = t.n_total;          // the rows region: every bucket's rows go there, at most one row per point
    return SSDR_OK;
}

// what depends on the rooms' points and dl alone (none of it on a centre): bounding box, grid and bucket geometry, the [chunk][bucket] counts and their scans, one
// work item per non-empty bucket; prm: every room's status and grid parameters; counters: zeroed as a call starts them, [0] = the items
struct FeTables { float* partial; FeGeom* geom; unsigned* cntm; unsigned* tot; unsigned* boff; FeItem* items; };
void fe_launch_tables(const FeTab& t, const float* d_p, float dl, GsParams* prm, const FeTables& T, int* counters, hipStream_t s) {
    const unsigned R = (unsigned)t.nr;
    hipLaunchKernelGGL(fe_minmax_partial, dim3(PB, R), dim3(BS), 0, s, t, d_p, T.partial);
    hipLaunchKernelGGL(fe_params, dim3(R), dim3(BS), 0, s, t, T.partial, dl, prm, T.geom, counters);
    hipLaunchKernelGGL(fe_count, dim3(t.chunks_max, R), dim3(FE_NT), 0, s, t, d_p, T.geom, prm, T.cntm);
    hipLaunchKernelGGL(fe_colscan, dim3(FE_NBMAX / BS, R), dim3(BS), 0, s, t, T.geom, T.cntm, T.tot);
    hipLaunchKernelGGL(fe_bscan, dim3(R), dim3(FE_NT), 0, s, t, T.geom, T.tot, T.boff, T.items, counters);
}

// The one scatter launcher: the input rows into `rec` by the tables' layout.  mode 0: every record (flag / info / nscat unused: NULL); 1: the records of the flagged
// buckets; 2: those of the unflagged buckets of the rooms info sends on to stage 2; 1 and 2 count what they wrote per room into nscat.
struct FeInputs { const float* p; const float* f; int fdim; const int* c; int ldim; };
void fe_launch_scatter(int mode, const FeTab& t, const FeInputs& in, const FeTables& T, uint4* rec, const unsigned char* flag, const FeTileInfo* info, unsigned long long* nscat,
                       hipStream_t s) {
    using Kernel = decltype(&fe_scatter<3, 1, 0>);          // [the hot path's rows (3 features + 1 label) or any][mode]
    static const Kernel kernel[2][3] = {{fe_scatter<-1, -1, 0>, fe_scatter<-1, -1, 1>, fe_scatter<-1, -1, 2>}, {fe_scatter<3, 1, 0>, fe_scatter<3, 1, 1>, fe_scatter<3, 1, 2>}};
    hipLaunchKernelGGL(kernel[in.fdim == 3 && in.ldim == 1][mode], dim3(t.chunks_max, (unsigned)t.nr), dim3(FE_SNT), 0, s, t, in.p, in.f, in.fdim, in.c, in.ldim, T.geom, T.cntm,
                       T.boff, rec, flag, info, nscat);
}
void fe_launch_reduce(int grid, const FeRedArgs& ra, hipStream_t s) {
    hipLaunchKernelGGL((ra.fdim == 3 && ra.ldim == 1 ? fe_reduce<3, 1> : fe_reduce<-1, -1>), dim3(grid), dim3(FE_RNT), 0, s, ra);
}

// The process-wide switches, read once (tests/test_subsample_paths.py gives a setting a child process of its own).  The two switches of a plan's creation,
// SSDR_FE_PLAN_RECORDS and SSDR_FE_PLAN_RECORDS_MAX_MB, are read at every frontend_plan_build instead: the tests set them in-process.
struct FeEnv {
    int wgs;             // SSDR_FE_WGS: workgroups per CU of the unstaged reduction, not capped by the points (unset: 0 = the default below)
    int move_wgs;        // SSDR_FE_MOVE_WGS: workgroups per CU of fe_move (unset: 32)
};
const FeEnv& fe_env() {
    static const FeEnv env = [] {
        auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
        return FeEnv{num("SSDR_FE_WGS", 0), num("SSDR_FE_MOVE_WGS", 32)};
    }();
    return env;
}
long fe_env_long(const char* name, long dflt) { const char* e = getenv(name); return e && e[0] ? atol(e) : dflt; }

}  // namespace

// A room plan: the tables of fe_launch_tables in buffers of its own (not the per-stream scratch: calls on any stream read them, a call without a plan on the same
// stream does not touch them), and the identity of what they were built from.  Read-only once built.
// It also holds the rooms' records: where a record lands follows from the rooms' points and dl alone (boff, cntm), and a record is the input row itself, so the
// every-bucket scatter (MODE 0) runs once, at build, and a call with such a plan launches no scatter and reads none of points / features / labels: fe_reduce reads
// the plan's records in place (it never writes them: its rows go to the per-stream rows region).  The plan holds the inputs rearranged and counts of them, never a
// sum or a vote.  Switches, read when a plan is created: SSDR_FE_PLAN_RECORDS=0 builds a plan without records (calls scatter per step as without them: A/B runs);
// SSDR_FE_PLAN_RECORDS_MAX_MB (default 4096): a plan whose records would be larger is built without them.
struct FePlan {
    DevBuf partial, geom, cntm, tot, boff, items, counters, prm;
    DevBuf rec; size_t record_bytes = 0;          // the rooms' records, every bucket's where (boff, cntm) put them: 32 B x n_total, or none (record_bytes 0: calls scatter per step)
    const float* d_p = nullptr; const float* d_f = nullptr; const int32_t* d_c = nullptr; size_t fdim = 0, ldim = 0, nr = 0; float dl = 0.f;
    std::vector<int64_t> room_off; FeTab t;
    hipStream_t stream = nullptr; hipEvent_t built = nullptr;          // the stream the tables were built on; recorded behind the last of their launches
    mutable std::mutex mu; mutable std::vector<hipStream_t> waited;      // the other streams that have waited for `built`
    FeTables tables() const { FeTables T; T.partial = partial.as<float>(); T.geom = geom.as<FeGeom>(); T.cntm = cntm.as<unsigned>(); T.tot = tot.as<unsigned>();
                              T.boff = boff.as<unsigned>(); T.items = items.as<FeItem>(); return T; }
    ~FePlan() { if (built) (void)hipEventDestroy(built); }
};

namespace {

// What one call enqueues.  Four kinds:
//
//   call                                              tables                         order                                scatter                              reduction
//   unstaged (no centres; a plan never arrives here)  own five launches              none                                 MODE 0                               one launch over all items
//   staged, no plan                                   own five launches              fe_tile_order before the scatter     MODE 1, then MODE 2 before stage 2   three stage launches
//   staged, plan without records                      plan's tables + fe_plan_begin  the same                             the same                             the same
//   staged, plan with records                         plan's tables + fe_plan_begin  the same, and it counts `given`      none                                 three stages reading plan->rec
//
// The order counts `given` (per room, the records the stages were given: FeTileArgs::given) exactly when no scatter runs to count them.
enum FeKind { FE_UNSTAGED, FE_STAGED, FE_STAGED_PLAN, FE_STAGED_PLAN_REC };
struct FeCall {
    FeKind kind = FE_UNSTAGED;
    bool staged() const { return kind != FE_UNSTAGED; }
    bool planned() const { return kind == FE_STAGED_PLAN || kind == FE_STAGED_PLAN_REC; }
    bool scatters() const { return kind != FE_STAGED_PLAN_REC; }
    const uint4* rec = nullptr;          // the records where a plan holds them; NULL: the call's scatter leaves them at the start of the per-stream buffer
    size_t rows_at = 0;                  // first row of the rows region (t.ovf_cap rows) in the per-stream buffer: behind the call's own records, or 0
    size_t buf_bytes = 0;                // that buffer
    int g_whole = 0, g_stage = 0, g_last = 0, g_move = 0;          // grids: the unstaged reduction; stages 1 and 2, stage 3; fe_move
};

// Launches nothing and reserves nothing.
FeCall fe_call_plan(const FeTab& t, bool centres, const FePlan* plan, int num_cu, const FeEnv& env) {
    FeCall c;
    c.kind = !centres ? FE_UNSTAGED : !plan ? FE_STAGED : !plan->record_bytes ? FE_STAGED_PLAN : FE_STAGED_PLAN_REC;
    if (!c.scatters()) c.rec = plan->rec.as<uint4>();
    c.rows_at = c.scatters() ? (size_t)t.n_total : 0;
    c.buf_bytes = 32 * (c.rows_at + (size_t)t.ovf_cap) + 64;
    // The items (buckets) differ in size and are dealt to the workgroups round robin: with twice the resident workgroups (16 per CU: rounds 4-5) the
    // kernel ended with its unluckiest workgroup; with ~ one workgroup per item the hardware's dispatcher does the balancing.  Same box, workgroups
    // per CU (SSDR_FE_WGS): 16: 0.43 ms, 32: 0.39, 64: 0.35, **128: 0.338**, 256: 0.337, 512: 0.343, 4096: slower than 16 (front end 1.08 -> 1.00 ms,
    // 198 -> 201 Mpoints/s).  Capped by the points (a bucket holds ~10^3 of them; workgroups beyond the item count exit at once).
    const long cap = std::max<long>((long)num_cu * 16, (long)t.n_total / 64);
    c.g_stage = (int)std::min<long>((long)num_cu * 128, cap);
    c.g_whole = env.wgs > 0 ? (int)std::min<long>((long)num_cu * env.wgs, 1L << 30) : c.g_stage;
    c.g_last = std::max(1, c.g_stage / 8);          // stage 3 is the exception: its workgroups take several items each
    // a wave per item, round robin: 8 workgroups per CU give every wave two items of different sizes, 32 one (0.100 -> 0.094 ms; SSDR_FE_MOVE_WGS)
    c.g_move = num_cu * env.move_wgs;
    return c;
}

}  // namespace

bool frontend_fits(size_t fdim, size_t ldim) { return 3 + fdim + ldim <= 7; }

// the five launches of fe_launch_tables into a new plan's buffers, on `s`, and the every-bucket scatter into its records; the event lets a call on another stream wait for them
int frontend_plan_build(const float* d_p, const float* d_f, size_t fdim, const int32_t* d_c, size_t ldim, const int64_t* room_off, size_t nr, float dl, hipStream_t s,
                        FePlan** out) {
    std::unique_ptr<FePlan> P(new FePlan);
    SSDR_TRY(fe_room_table(room_off, nr, P->t));
    P->d_p = d_p; P->d_f = d_f; P->d_c = d_c; P->fdim = fdim; P->ldim = ldim; P->nr = nr; P->dl = dl; P->room_off.assign(room_off, room_off + nr + 1); P->stream = s;
    const FeTab& t = P->t;
    SSDR_TRY(P->partial.reserve(24 * (size_t)PB * nr)); SSDR_TRY(P->geom.reserve(sizeof(FeGeom) * nr)); SSDR_TRY(P->counters.reserve(256 + 8 * RADIX_MAX_SEG));
    SSDR_TRY(P->cntm.reserve(4 * (size_t)FE_NBMAX * t.chunks_max * nr)); SSDR_TRY(P->tot.reserve(4 * (size_t)FE_NBMAX * nr)); SSDR_TRY(P->boff.reserve(4 * (size_t)(FE_NBMAX + 1) * nr));
    SSDR_TRY(P->items.reserve(sizeof(FeItem) * (size_t)FE_NBMAX * nr)); SSDR_TRY(P->prm.reserve(sizeof(GsParams) * nr));
    SSDR_HIP(hipEventCreateWithFlags(&P->built, hipEventDisableTiming));
    const size_t rec_bytes = 32 * (size_t)t.n_total;
    const long max_mb = fe_env_long("SSDR_FE_PLAN_RECORDS_MAX_MB", 4096);
    const bool records = fe_env_long("SSDR_FE_PLAN_RECORDS", 1) != 0 && max_mb > 0 && rec_bytes <= (size_t)max_mb << 20;
    if (records) SSDR_TRY(P->rec.reserve(rec_bytes));
    fe_launch_tables(t, d_p, dl, P->prm.as<GsParams>(), P->tables(), P->counters.as<int>(), s);
    if (records) {
        // every record of every room with a grid (a room without one writes nothing), behind fe_bscan: the layout a call's own scatter would give
        fe_launch_scatter(0, t, FeInputs{d_p, d_f, (int)fdim, (const int*)d_c, (int)ldim}, P->tables(), P->rec.as<uint4>(), nullptr, nullptr, nullptr, s);
        P->record_bytes = rec_bytes;
    }
    SSDR_HIP(hipGetLastError());
    SSDR_HIP(hipEventRecord(P->built, s));
    *out = P.release();
    return SSDR_OK;
}

// waits for the device: a call that reads the plan may still be in flight on any stream
int frontend_plan_destroy(FePlan* P) {
    if (!P) return SSDR_OK;
    const hipError_t e = hipDeviceSynchronize();
    delete P;
    if (e != hipSuccess) { set_error("rooms_plan_destroy: hipDeviceSynchronize failed: %s", hipGetErrorString(e)); return SSDR_ERR_HIP; }
    return SSDR_OK;
}

// what a plan holds beside its tables: the bytes of its records (0: none), and whether they are ordered inside a bucket (never, so far)
void frontend_plan_info(const FePlan* P, int64_t* record_bytes, int32_t* sorted) {
    if (record_bytes) *record_bytes = (int64_t)P->record_bytes;
    if (sorted) *sorted = 0;
}

// the plan answers for exactly the inputs it was built from
int frontend_plan_check(const FePlan* P, const float* d_p, const float* d_f, size_t fdim, const int32_t* d_c, size_t ldim, const int64_t* room_off, size_t nr, float dl) {
    const char* what = nullptr;
    if (P->d_p != d_p || P->d_f != d_f || P->d_c != d_c) what = "input pointers";
    else if (P->fdim != fdim || P->ldim != ldim) what = "fdim / ldim";
    else if (P->nr != nr) what = "num_clouds";
    else if (!std::equal(room_off, room_off + nr + 1, P->room_off.begin())) what = "cloud_offsets";
    else if (!(P->dl == dl)) what = "sampleDl";
    if (what) { set_error("tile_from_rooms_planned_batch: the plan was built from other %s (rebuild it: ssdr_rooms_plan_create_dev)", what); return SSDR_ERR_INVALID; }
    return SSDR_OK;
}

// All clouds of a batch in the same launches; prm: the caller's per-cloud GsParams (status / voxel count as the sort-based path leaves them).
// centres (host [nr, 3]) / num_points: reduce only the buckets the num_points rows nearest to every room's centre can lie in (the staged reduction above);
// the outputs then hold those buckets' rows, in key order, and d_om their count.  centres NULL: every bucket.
int frontend_batch_device(const float* d_p, const float* d_f, size_t fdim, const int32_t* d_c, size_t ldim, const int64_t* room_off, size_t nr, float dl,
                          float* d_op, float* d_of, int32_t* d_oc, int64_t* d_om, GsParams* prm, hipStream_t s, const float* centres, size_t num_points, const FePlan* plan) {
    FeState& S = per_stream<FeState>(s);
    S.tile_clouds = 0;
    // 1. the room table
    FeTab t;
    SSDR_TRY(fe_room_table(room_off, nr, t));
    // 2. what this call enqueues
    if (plan && !centres) { set_error("grid_subsample_batch: a room plan goes with centres"); return SSDR_ERR_INTERNAL; }
    const FeCall call = fe_call_plan(t, centres != nullptr, plan, ctx().num_cu, fe_env());
    // 3. the per-stream scratch
    SSDR_TRY(S.counters.reserve(256 + 8 * RADIX_MAX_SEG)); SSDR_TRY(S.rcp.reserve(4 * (FE_CAP + 1)));
    if (!call.planned()) {
        SSDR_TRY(S.partial.reserve(24 * (size_t)PB * nr)); SSDR_TRY(S.geom.reserve(sizeof(FeGeom) * nr));
        SSDR_TRY(S.cntm.reserve(4 * (size_t)FE_NBMAX * t.chunks_max * nr)); SSDR_TRY(S.tot.reserve(4 * (size_t)FE_NBMAX * nr)); SSDR_TRY(S.boff.reserve(4 * (size_t)(FE_NBMAX + 1) * nr));
        SSDR_TRY(S.items.reserve(sizeof(FeItem) * (size_t)FE_NBMAX * nr));
    }
    SSDR_TRY(S.nocc.reserve(4 * (size_t)FE_NBMAX * nr)); SSDR_TRY(S.trow.reserve(4 * (size_t)FE_NBMAX * nr));
    SSDR_TRY(S.lrc.reserve((size_t)FE_NBMAX * FE_LR * nr)); SSDR_TRY(S.pre.reserve(2 * (size_t)FE_NBMAX * FE_LR * nr));
    SSDR_TRY(S.rowcnt.reserve(4 * (size_t)FE_ROWCAP * nr));
    SSDR_TRY(S.rec.reserve(call.buf_bytes));
    if (call.staged()) {
        SSDR_TRY(S.okey.reserve(4 * (size_t)FE_NBMAX * nr)); SSDR_TRY(S.odmax.reserve(4 * (size_t)FE_NBMAX * nr)); SSDR_TRY(S.ocum.reserve(4 * (size_t)FE_NBMAX * nr));
        SSDR_TRY(S.work.reserve(sizeof(FeItem) * (size_t)FE_NBMAX * nr)); SSDR_TRY(S.tinfo.reserve(sizeof(FeTileInfo) * RADIX_MAX_SEG));
        SSDR_TRY(S.flag.reserve((size_t)FE_NBMAX * nr));
    }
    // 4. the launches, in stream order.  The centre-independent tables are this call's own (the per-stream scratch) or the plan's (read-only here; the only list the
    // stages write is S.work)
    const unsigned R = (unsigned)nr;
    FeTables own; own.partial = S.partial.as<float>(); own.geom = S.geom.as<FeGeom>(); own.cntm = S.cntm.as<unsigned>(); own.tot = S.tot.as<unsigned>();
    own.boff = S.boff.as<unsigned>(); own.items = S.items.as<FeItem>();
    const FeTables T = call.planned() ? plan->tables() : own;
    int* counters = S.counters.as<int>();
    const FeInputs in{d_p, d_f, (int)fdim, (const int*)d_c, (int)ldim};
    FeRedArgs ra; ra.t = t; ra.items = T.items; ra.prm = prm; ra.counters = counters; ra.rcp = S.rcp.as<float>();
    ra.rec = call.rec ? call.rec : S.rec.as<uint4>(); ra.rows = S.rec.as<uint4>() + 2 * call.rows_at;
    ra.nocc = S.nocc.as<unsigned>(); ra.trow = S.trow.as<unsigned>(); ra.lrc = S.lrc.as<unsigned char>(); ra.fdim = (int)fdim; ra.ldim = (int)ldim;
    // the staged reduction (centres given).  Stage 1's buckets follow from the buckets' point counts, their boxes and the centres: all there after fe_bscan, so the
    // order comes first and the scatter writes the records of those buckets only
    FeTileArgs ta;
    if (call.staged()) {
        ta.t = t; ta.geom = T.geom; ta.tot = T.tot; ta.boff = T.boff; ta.nocc = ra.nocc; ta.lrc = ra.lrc; ta.flag = S.flag.as<unsigned char>();
        for (size_t i = 0; i < 3 * nr; ++i) ta.cen.c[i] = centres[i];
        ta.okey = S.okey.as<unsigned>(); ta.odmax = S.odmax.as<float>(); ta.ocum = S.ocum.as<unsigned>(); ta.work = S.work.as<FeItem>(); ta.counters = counters;
        ta.info = S.tinfo.as<FeTileInfo>(); ta.num_points = (int)std::min<size_t>(num_points, 0x3fffffff);
        // no scatter counts its records when they are the plan's: the order and the stage plan count what the stages are given, into the same words
        ta.given = call.scatters() ? nullptr : fe_scatter_counters(counters);
    }
    const unsigned char* flag = S.flag.as<unsigned char>(); const FeTileInfo* tinfo = S.tinfo.as<FeTileInfo>(); unsigned long long* nscat = fe_scatter_counters(counters);
    if (!S.rcp_ready) {
        hipLaunchKernelGGL(fe_rcp_init, dim3((FE_CAP + 256) / 256), dim3(256), 0, s, S.rcp.as<float>());
        S.rcp_ready = true;
    }
    // profiler sites (ssdr_prof_enable; bench.py's roofline leg): `work` = the algorithmic bytes a site is charged with — the one read of the inputs
    // (28 B per point) goes to the scatter, the one write of the rows (28 B per voxel: the count is the device's, bench.py adds it) to the reduction
    {
    ProfScope prof("fe_bbox_count_scan", s, 0.0);
    if (call.planned()) {
        // the plan's launches ran on its own stream: the first call on every other stream is ordered behind them
        if (s != plan->stream) {
            std::lock_guard<std::mutex> lk(plan->mu);
            if (std::find(plan->waited.begin(), plan->waited.end(), s) == plan->waited.end()) { SSDR_HIP(hipStreamWaitEvent(s, plan->built, 0)); plan->waited.push_back(s); }
        }
        hipLaunchKernelGGL(fe_plan_begin, dim3(R), dim3(64), 0, s, plan->prm.as<GsParams>(), plan->counters.as<int>(), prm, counters);
    } else fe_launch_tables(t, d_p, dl, prm, own, counters, s);
    if (call.staged()) hipLaunchKernelGGL(fe_tile_order, dim3(R), dim3(FE_NT), 0, s, ta);
    }
    if (call.scatters()) {
    ProfScope prof("fe_scatter", s, (double)(12 + 4 * (fdim + ldim)) * (double)t.n_total);
    fe_launch_scatter(call.staged() ? 1 : 0, t, in, T, S.rec.as<uint4>(), flag, tinfo, nscat, s);
    }
    {
    ProfScope prof("fe_reduce", s, 0.0);
    if (call.staged()) {
        // the same kernel per stage, over the stage's work list; the lists' lengths are the device's (workgroups beyond them exit at once)
        ra.items = S.work.as<FeItem>();
        for (int stage = 1; stage <= 3; ++stage) {
            if (stage == 2) {
                hipLaunchKernelGGL((fe_tile_plan<2>), dim3(R), dim3(FE_NT), 0, s, ta);
                // the records stage 1 did not need, for the rooms that go on (a second read of their points); every other room's workgroups leave at once
                if (call.scatters()) fe_launch_scatter(2, t, in, T, S.rec.as<uint4>(), flag, tinfo, nscat, s);
            } else if (stage == 3) hipLaunchKernelGGL((fe_tile_plan<3>), dim3(R), dim3(FE_NT), 0, s, ta);
            ra.counters = fe_stage_counters(counters, stage);
            fe_launch_reduce(stage < 3 ? call.g_stage : call.g_last, ra, s);
        }
        S.tile_clouds = (int)nr;
        S.room_n.assign(nr, 0);
        for (size_t r = 0; r < nr; ++r) S.room_n[r] = (long long)(room_off[r + 1] - room_off[r]);
    } else fe_launch_reduce(call.g_whole, ra, s);
    }
    ProfScope prof_move("fe_rows_move", s, 0.0);
    hipLaunchKernelGGL(fe_rowpre, dim3(256, R), dim3(BS), 0, s, T.geom, T.boff, S.lrc.as<unsigned char>(), S.pre.as<unsigned short>(), S.rowcnt.as<unsigned>());
    hipLaunchKernelGGL(fe_rowscan, dim3(R), dim3(FE_NT), 0, s, T.geom, S.rowcnt.as<unsigned>(), prm, (long long*)d_om);
    FeMoveArgs ma; ma.t = t; ma.geom = T.geom; ma.items = T.items; ma.counters = counters; ma.rows = ra.rows; ma.nocc = S.nocc.as<unsigned>();
    ma.trow = S.trow.as<unsigned>(); ma.lrc = S.lrc.as<unsigned char>(); ma.pre = S.pre.as<unsigned short>(); ma.rowbase = S.rowcnt.as<unsigned>(); ma.fdim = (int)fdim; ma.ldim = (int)ldim;
    ma.out_p = d_op; ma.out_f = d_of; ma.out_c = d_oc;
    hipLaunchKernelGGL((fdim == 3 && ldim == 1 ? fe_move<3, 1> : fe_move<-1, -1>), dim3(call.g_move), dim3(BS), 0, s, ma);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

void frontend_tile_forget(hipStream_t s) { per_stream<FeState>(s).tile_clouds = 0; }

// what the staged reduction of the last call on `s` did, per room (waits for the stream): the stage it ended in (0 = reduced whole without an order: more than
// FE_TO_NMAX non-empty buckets, or a grid the partition refuses; -1 = the call was not staged), the buckets it reduced and the room's non-empty buckets
int frontend_tile_stats(hipStream_t s, int32_t* stage, int32_t* reduced, int32_t* buckets, size_t nr) {
    FeState& S = per_stream<FeState>(s);
    SSDR_HIP(hipStreamSynchronize(s));
    std::vector<FeTileInfo> h(nr);
    const bool staged = S.tile_clouds > 0 && (size_t)S.tile_clouds == nr;
    if (staged) SSDR_HIP(hipMemcpy(h.data(), S.tinfo.p, sizeof(FeTileInfo) * nr, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < nr; ++r) {
        if (stage) stage[r] = staged ? h[r].stage : -1;
        if (reduced) reduced[r] = staged ? h[r].reduced : -1;
        if (buckets) buckets[r] = staged ? h[r].n : -1;
    }
    return SSDR_OK;
}

// what the stages of the last staged call on `s` were given, per room (waits for the stream): the records the scatter wrote (stage 1's pass plus the second pass of a
// room that went on) — or, when a plan holds the records, the records of the same buckets, counted by the order — and the room's points; -1 / -1 when the call was not staged
int frontend_scatter_stats(hipStream_t s, int64_t* scattered, int64_t* points, size_t nr) {
    FeState& S = per_stream<FeState>(s);
    SSDR_HIP(hipStreamSynchronize(s));
    std::vector<unsigned long long> h(nr);
    const bool staged = S.tile_clouds > 0 && (size_t)S.tile_clouds == nr;
    if (staged) SSDR_HIP(hipMemcpy(h.data(), fe_scatter_counters(S.counters.as<int>()), sizeof(unsigned long long) * nr, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < nr; ++r) {
        if (scattered) scattered[r] = staged ? (int64_t)h[r] : -1;
        if (points) points[r] = staged ? (int64_t)S.room_n[r] : -1;
    }
    return SSDR_OK;
}

}  // namespace ssdr
