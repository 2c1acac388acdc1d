// The reference's other three samplers (S3/sampler2.py): one iteration of RandomSampler._iteration (:463-493) / SeedSampler._iteration (:354-386) and
// AllSampler.sampling's list (:442-449) as an item list on the device, and _help_seed's precise labelling (:218-245), for gfx950.
//
// ssdr_region_draw_dev, one iteration (include/ssdr_al.h states the rule):
//   1. count    every cloud's unlabelled regions: an integer atomic per run of one cloud inside a wave (the clouds ascend with the region id).
//   2. live     one workgroup scans the clouds in ascending order: the live rank d of every cloud with an unlabelled region, L of them, and the
//               first slot of every live cloud among the unlabelled regions in (live rank, ...) order.  It also reads the click count k.
//   3. share    the k drawn elements of range(total_num) are the k smallest by (hashed key, element): a stable radix sort of the total_num
//               keys whose values start ascending, then each_file_number[d] = #{drawn e : e % L == d} by integer atomics.
//   4. take     one workgroup: take[d] = min(each_file_number[d], u[d]), its exclusive prefix (a cloud's first item), the seed remainder, d_info.
//   5. picks    ONE stable sort of the words (live rank << 32 | pick key) over all S regions, region id as payload: the pick key is the hashed key
//               of the region, or 0 for a cloud that is taken whole / takes no part (ascending id by stability); labelled regions sort behind
//               every live cloud.  Slot j of cloud d is its (j - first slot)-th pick: emitted when that is below take[d].
// SSDR_REGION_ALL skips 3 (each_file_number = u) and hashes nothing: the list is every unlabelled region in ascending order.
//
// Sharded (the clouds of the pool lie on `world` ranks, contiguous shares in rank order): step 1 alone is ssdr_region_draw_count_dev, into a table of
// cloud_slots + 1 words (the last one: the rank's status bits); the caller all-gathers the tables; ssdr_region_draw_sharded_dev runs 2 - 5 over them.
// Steps 2 - 4 see ALL ranks' clouds (slot rank * cloud_slots + cloud, padding slots count no region) and are replicated: the same L, k,
// each_file_number, take and first items on every rank.  Step 5 sorts this rank's regions alone, under their cloud's GLOBAL live rank and the hash of
// their GLOBAL id, and emits them at (global position - the items of the ranks before).  ssdr_region_draw_dev is the same chain at world 1 over its
// own table.
// Plain launches, nothing waits on the host, the scratch is per stream, every count is an integer atomic or a scan: results are bit-stable.
//
// ssdr_seed_label_dev: every item is labelled with its points' own ground truth; regions of up to 256 points by a wave each, larger ones by a
// workgroup each (the boundary of select_label.hip).
#include "ssdr_internal.hpp"
#include "block_prims.hpp"
#include "draw_word.hpp"

namespace ssdr {
namespace {

constexpr int RD_BS = 256;
constexpr int SD_WAVE_MAX = 256;            // largest region of the wave form
constexpr size_t RD_MAX = 0x3fffffff;       // regions / elements: what one sort buffer holds
enum { RD_ST_COUNT = 1, RD_ST_ITEMS = 2, RD_ST_CLOUD = 4 };
enum { SD_ST_ITEM = 4 };

struct DrawArgs {
    const unsigned char* labeled; const int* sp_cloud; int S, B; long long T; int all;
    int* u;                                                     // this rank's table: [B] unlabelled regions per cloud ... [CS] its status bits
    const int* uall; int W, CS, me;                             // every rank's table [W][CS + 1]; this rank
    int *rank, *ustart, *ulive, *cnt, *take, *istart;           // per cloud slot of all ranks (rank) / per live rank
    // [0] L, [1] k, [2] unlabelled regions, [3] status; of this rank: [4] the unlabelled regions before its own, [5] its own, [6] its first live rank,
    // [7] one past its last
    long long* head;
};

inline unsigned rd_blocks(size_t n) { return (unsigned)std::max<size_t>(1, std::min<size_t>((n + RD_BS - 1) / RD_BS, (size_t)ctx().num_cu * 8)); }

__device__ __forceinline__ int region_cloud(const DrawArgs& a, int s) {
    const int c = a.sp_cloud[s];
    return c >= 0 && c < a.B ? c : -1;
}

// ---- 1. count ----------------------------------------------------------------------------------------------------------------------------------
// The clouds ascend with the region id, so a wave's 64 regions lie in a few runs of one cloud each: the first lane of a run adds the run's unlabelled
// regions in one atomic (any order of clouds is counted correctly, in more runs).  Every lane of a block takes the same number of trips.
__global__ __launch_bounds__(RD_BS) void rd_count(DrawArgs a) {
    const int lane = threadIdx.x & 63;
    for (int base = blockIdx.x * RD_BS; base < a.S; base += gridDim.x * RD_BS) {
        const int s = base + threadIdx.x;
        const bool in = s < a.S;
        const int c = in ? region_cloud(a, s) : -2;
        const bool unl = in && !a.labeled[s];
        if (unl && c < 0) atomicOr(&a.u[a.CS], (int)RD_ST_CLOUD);
        const int before = __shfl_up(c, 1u);
        const bool first = lane == 0 || c != before;
        const unsigned long long fm = __ballot(first), um = __ballot(unl && c >= 0);
        if (first && c >= 0) {
            const unsigned long long above = lane == 63 ? 0ull : fm >> (lane + 1);
            const int len = above ? __ffsll(above) : 64 - lane;                       // up to the next run's first lane
            const unsigned long long run = (len == 64 ? ~0ull : (1ull << len) - 1ull) << lane;
            const int n = __popcll(um & run);
            if (n) atomicAdd(&a.u[c], n);
        }
    }
}

// two inclusive sums over the workgroup's 256 threads at once; returns the totals, x / y become the EXCLUSIVE prefixes
__device__ __forceinline__ void block_scan2(int& x, int& y, int& tx, int& ty, int (*s_w)[2]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int ix = x, iy = y;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int ax = __shfl_up(ix, (unsigned)o), ay = __shfl_up(iy, (unsigned)o);
        if (lane >= o) { ix += ax; iy += ay; }
    }
    if (lane == 63) { s_w[w][0] = ix; s_w[w][1] = iy; }
    __syncthreads();
    int px = 0, py = 0; tx = 0; ty = 0;
    for (int q = 0; q < RD_BS / 64; ++q) { if (q < w) { px += s_w[q][0]; py += s_w[q][1]; } tx += s_w[q][0]; ty += s_w[q][1]; }
    x = px + ix - x; y = py + iy - y;
    __syncthreads();
}

// ---- 2. live -----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RD_BS) void rd_live(DrawArgs a, const long long* __restrict__ d_count) {
    __shared__ int s_w[RD_BS / 64][2];
    const int tid = threadIdx.x, G = a.W * a.CS, lo = a.me * a.CS, hi = lo + a.CS;      // [lo, hi): this rank's slots
    int runl = 0, runu = 0;
    for (int base = 0; base < G; base += RD_BS) {
        const int g = base + tid;
        const int uu = g < G ? max(a.uall[(size_t)(g / a.CS) * (a.CS + 1) + g % a.CS], 0) : 0, lv = uu > 0 ? 1 : 0;
        int xl = lv, xu = uu, tl, tu;
        block_scan2(xl, xu, tl, tu, s_w);
        if (g < G) a.rank[g] = lv ? runl + xl : -1;
        if (lv) { const int d = runl + xl; a.ustart[d] = runu + xu; a.ulive[d] = uu; a.cnt[d] = a.all ? uu : 0; }
        if (g == lo) { a.head[4] = runu + xu; a.head[6] = runl + xl; }
        if (g == hi) { a.head[5] = runu + xu; a.head[7] = runl + xl; }                   // ([5]: less [4], below)
        runl += tl; runu += tu;
    }
    __syncthreads();
    if (tid == 0) {
        long long st = 0;
        for (int w = 0; w < a.W; ++w) st |= a.uall[(size_t)w * (a.CS + 1) + a.CS] & RD_ST_CLOUD;      // a region outside its rank's table: seen by every rank
        long long k = a.all ? (long long)runu : *d_count;
        if (k < 0) k = 0;
        if (!a.all && k > a.T) { st |= RD_ST_COUNT; k = 0; }      // np.random.choice raises
        if (runl == 0) k = 0;
        a.head[0] = runl; a.head[1] = k; a.head[2] = runu; a.head[3] = st;
        if (hi == G) { a.head[5] = runu; a.head[7] = runl; }
        a.head[5] -= a.head[4];
    }
}

// ---- 3. share ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RD_BS) void rd_count_keys(DrawBase b, long long T, int key_bits, unsigned long long* keys, unsigned* vals) {
    const long long stride = (long long)gridDim.x * RD_BS;
    for (long long e = (long long)blockIdx.x * RD_BS + threadIdx.x; e < T; e += stride) {
        keys[e] = (unsigned long long)(draw_word(b, (uint64_t)e, 0u) >> (32 - key_bits));
        vals[e] = (unsigned)e;
    }
}
__global__ __launch_bounds__(RD_BS) void rd_share(DrawArgs a, const unsigned* __restrict__ vals) {
    const long long k = a.head[1], L = a.head[0], stride = (long long)gridDim.x * RD_BS;
    for (long long i = (long long)blockIdx.x * RD_BS + threadIdx.x; i < k; i += stride) atomicAdd(&a.cnt[(long long)vals[i] % L], 1);
}

// ---- 4. take -----------------------------------------------------------------------------------------------------------------------------------
// sharded: this rank's items are those of the live ranks [head[6], head[7]); info[6] counts them, n_items is their number after the clamp
__global__ __launch_bounds__(RD_BS) void rd_take(DrawArgs a, int max_items, int* n_items, long long* info, int sharded) {
    __shared__ int s_w[RD_BS / 64][2];
    __shared__ int s_own[2];
    const int tid = threadIdx.x, L = (int)a.head[0], dlo = (int)a.head[6], dhi = (int)a.head[7];
    int runi = 0, runr = 0;
    if (tid == 0) { s_own[0] = -1; s_own[1] = -1; }
    __syncthreads();
    for (int base = 0; base < L; base += RD_BS) {
        const int d = base + tid;
        const int c = d < L ? a.cnt[d] : 0, uu = d < L ? a.ulive[d] : 0;
        const int tk = min(c, uu);
        int xi = tk, xr = c - tk, ti, tr;
        block_scan2(xi, xr, ti, tr, s_w);
        if (d < L) { a.take[d] = tk; a.istart[d] = runi + xi; }
        if (d < L && d == dlo) s_own[0] = runi + xi;
        if (d < L && d == dhi) s_own[1] = runi + xi;
        runi += ti; runr += tr;
    }
    __syncthreads();
    if (tid == 0) {
        const int ilo = s_own[0] < 0 ? runi : s_own[0], own = (s_own[1] < 0 ? runi : s_own[1]) - ilo;      // (no live cloud at or behind: the end of the list)
        long long st = a.head[3];
        if (own > max_items) st |= RD_ST_ITEMS;
        *n_items = min(own, max_items);
        a.head[6] = ilo;                                                                                      // rd_emit: the items of the ranks before
        info[0] = L; info[1] = a.head[1]; info[2] = runi; info[3] = runr; info[4] = a.head[2] - runi; info[5] = st; info[6] = sharded ? own : 0; info[7] = 0;
    }
}

// ---- 5. picks ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RD_BS) void rd_pick_keys(DrawArgs a, DrawBase b, unsigned long long first_region, int key_bits, unsigned long long* keys, unsigned* vals) {
    for (int s = blockIdx.x * RD_BS + threadIdx.x; s < a.S; s += gridDim.x * RD_BS) {
        const int c = a.labeled[s] ? -1 : region_cloud(a, s);
        unsigned long long key = (unsigned long long)(unsigned)(a.W * a.CS) << 32;      // behind every live cloud
        const int d = c >= 0 ? a.rank[a.me * a.CS + c] : -1;      // (-1 too where the tables count no unlabelled region of c: they belong to another mask)
        if (d >= 0) {
            const int cn = a.cnt[d];
            const bool drawn = !a.all && cn > 0 && cn <= a.ulive[d];          // otherwise list order: ascending id
            key = ((unsigned long long)(unsigned)d << 32) | (drawn ? (unsigned long long)(draw_word(b, first_region + (uint64_t)s, 0u) >> (32 - key_bits)) : 0ull);
        }
        keys[s] = key; vals[s] = (unsigned)s;
    }
}
__global__ __launch_bounds__(RD_BS) void rd_emit(DrawArgs a, const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals, int* items, int* item_pos,
                                                 int max_items) {
    const int L = (int)a.head[0], ubefore = (int)a.head[4], nu = (int)a.head[5], ibefore = (int)a.head[6];
    for (int j = blockIdx.x * RD_BS + threadIdx.x; j < nu; j += gridDim.x * RD_BS) {      // this rank's unlabelled regions fill the first slots
        const int d = (int)(keys[j] >> 32);
        if (d >= L) continue;
        const int r = ubefore + j - a.ustart[d];
        if (r < 0 || r >= a.take[d]) continue;
        const int pos = a.istart[d] + r, at = pos - ibefore;                              // the item's place in the union's list / in this rank's
        if (at < 0 || at >= max_items) continue;
        items[at] = (int)vals[j];
        if (item_pos) item_pos[at] = pos;
    }
}

// ---- the precise labels of the seed round ------------------------------------------------------------------------------------------------------
struct SeedArgs {
    const int* gt; long long n; const int* sp_off; const int* sp_pts; int S; const int* items; const int* n_items; int max_items;
    float* mask; float* label; unsigned char* labeled; unsigned long long* out; int* big; int* nbig;
};
__device__ __forceinline__ void seed_points(const SeedArgs& a, int lo, int n, int t, int nt) {
    bool bad = false;
    for (int i = t; i < n; i += nt) {
        const int p = a.sp_pts[lo + i];
        if (p < 0 || p >= a.n) { bad = true; continue; }
        a.mask[p] = 1.0f; a.label[p] = (float)a.gt[p];
    }
    if (bad) atomicOr(&a.out[2], (unsigned long long)SD_ST_ITEM);
}
__global__ __launch_bounds__(RD_BS) void seed_label_wave(SeedArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int M = max(0, min(*a.n_items, a.max_items));
    for (int j = blockIdx.x * 4 + w; j < M; j += gridDim.x * 4) {
        const int sp = a.items[j];
        if (sp < 0 || sp >= a.S) { if (lane == 0) atomicOr(&a.out[2], (unsigned long long)SD_ST_ITEM); continue; }
        const int lo = a.sp_off[sp], n = max(a.sp_off[sp + 1] - lo, 0);
        if (lane == 0) { a.labeled[sp] = 1; atomicAdd(&a.out[0], 1ull); atomicAdd(&a.out[1], (unsigned long long)n); }
        if (n > SD_WAVE_MAX) { if (lane == 0) a.big[atomicAdd(a.nbig, 1)] = j; continue; }
        seed_points(a, lo, n, lane, 64);
    }
}
__global__ __launch_bounds__(RD_BS) void seed_label_block(SeedArgs a) {
    const int nb = min(*a.nbig, a.max_items);
    for (int b = blockIdx.x; b < nb; b += gridDim.x) {
        const int sp = a.items[a.big[b]];
        const int lo = a.sp_off[sp];
        seed_points(a, lo, a.sp_off[sp + 1] - lo, threadIdx.x, RD_BS);
    }
}

struct RegionDrawState { RadixSorter sorter; DevBuf keys, vals, tab, head, big; size_t B = 0; };      // B: the cloud slots of the newest draw (ssdr_region_draw_shares)
RegionDrawState& rds(hipStream_t s) { return per_stream<RegionDrawState>(s); }

int draw_refusals(const char* who, int mode, int key_bits, const void* d_labeled, const void* d_sp_cloud, size_t S, size_t num_clouds, size_t total_num, const void* d_count,
                  const void* d_items, size_t max_items, const void* d_n_items, const void* d_info, uint64_t first_region) {
    if (mode != SSDR_REGION_RANDOM && mode != SSDR_REGION_ALL) { set_error("%s: unknown mode %d (0: random, 1: all)", who, mode); return SSDR_ERR_INVALID; }
    if (!d_labeled || !d_sp_cloud || !d_n_items || !d_info || (max_items && !d_items) || (mode == SSDR_REGION_RANDOM && !d_count)) { set_error("%s: NULL pointer", who); return SSDR_ERR_INVALID; }
    if (S == 0 || total_num == 0 || num_clouds == 0) { set_error("%s: %zu regions of %zu clouds, total_num = %zu", who, S, num_clouds, total_num); return SSDR_ERR_INVALID; }
    if (key_bits < 1 || key_bits > 32) { set_error("%s: key_bits = %d is outside 1 .. 32", who, key_bits); return SSDR_ERR_INVALID; }
    if (S > RD_MAX || total_num > RD_MAX || num_clouds > RD_MAX || max_items > RD_MAX || first_region > 0xffffffffffffffffull - S) {
        set_error("%s: more than 0x3fffffff regions, clouds, elements or items", who); return SSDR_ERR_UNSUPPORTED;
    }
    return SSDR_OK;
}

// Steps 2 - 5 over the count tables `uall` [W][CS + 1] (nullptr: world 1, this call's own table, which step 1 fills here).  d_item_pos: the sharded form.
int draw_chain(uint64_t seed, uint32_t round, uint32_t iteration, int mode, int key_bits, uint64_t first_region, int me, int W, const int* uall, size_t CS,
               const uint8_t* d_labeled, const int32_t* d_sp_cloud, size_t S, size_t B, size_t total_num, const int64_t* d_count, int32_t* d_items, int32_t* d_item_pos,
               size_t max_items, int32_t* d_n_items, int64_t* d_info, hipStream_t s) {
    RegionDrawState& Q = rds(s);
    const size_t G = (size_t)W * CS, slots = std::max(S, mode == SSDR_REGION_RANDOM ? total_num : (size_t)1);
    SSDR_TRY(Q.keys.reserve(8 * slots)); SSDR_TRY(Q.vals.reserve(4 * slots)); SSDR_TRY(Q.tab.reserve(4 * (6 * G + CS + 1))); SSDR_TRY(Q.head.reserve(64));
    int* t = Q.tab.as<int>();
    Q.B = G;
    DrawArgs a{d_labeled, d_sp_cloud, (int)S, (int)B, (long long)total_num, mode == SSDR_REGION_ALL ? 1 : 0, t + 6 * G, uall ? uall : t + 6 * G, W, (int)CS, me,
               t, t + G, t + 2 * G, t + 3 * G, t + 4 * G, t + 5 * G, Q.head.as<long long>()};
    unsigned long long* keys = Q.keys.as<unsigned long long>(); unsigned* vals = Q.vals.as<unsigned>();
    ProfScope prof("region_draw", s, 12.0 * (double)slots);
    SSDR_HIP(hipMemsetAsync(Q.head.p, 0, 64, s));
    if (!uall) {
        SSDR_HIP(hipMemsetAsync(a.u, 0, 4 * (CS + 1), s));
        hipLaunchKernelGGL(rd_count, dim3(rd_blocks(S)), dim3(RD_BS), 0, s, a);
    }
    hipLaunchKernelGGL(rd_live, dim3(1), dim3(RD_BS), 0, s, a, (const long long*)d_count);
    if (mode == SSDR_REGION_RANDOM) {
        hipLaunchKernelGGL(rd_count_keys, dim3(rd_blocks(total_num)), dim3(RD_BS), 0, s, draw_base(seed, round, iteration, SSDR_DRAW_REGION_COUNT), (long long)total_num, key_bits,
                           keys, vals);
        SSDR_HIP(hipGetLastError());
        SSDR_TRY(Q.sorter.sort((uint64_t*)keys, vals, (int)total_num, nullptr, s, key_bits));
        hipLaunchKernelGGL(rd_share, dim3(rd_blocks(total_num)), dim3(RD_BS), 0, s, a, (const unsigned*)vals);
    }
    hipLaunchKernelGGL(rd_take, dim3(1), dim3(RD_BS), 0, s, a, (int)max_items, d_n_items, (long long*)d_info, d_item_pos ? 1 : 0);
    hipLaunchKernelGGL(rd_pick_keys, dim3(rd_blocks(S)), dim3(RD_BS), 0, s, a, draw_base(seed, round, iteration, SSDR_DRAW_REGION_PICK), (unsigned long long)first_region,
                       key_bits, keys, vals);
    SSDR_HIP(hipGetLastError());
    int rank_bits = 1;
    while (((size_t)1 << rank_bits) <= G) ++rank_bits;          // the live ranks and G itself (the labelled regions' word)
    Q.sorter.wide_high = true;                                  // the live rank varies above bit 32
    SSDR_TRY(Q.sorter.sort((uint64_t*)keys, vals, (int)S, nullptr, s, 32 + rank_bits));
    hipLaunchKernelGGL(rd_emit, dim3(rd_blocks(S)), dim3(RD_BS), 0, s, a, (const unsigned long long*)keys, (const unsigned*)vals, d_items, d_item_pos, (int)max_items);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

}  // namespace
}  // namespace ssdr

using namespace ssdr;

extern "C" {

int ssdr_region_draw_dev(uint64_t seed, uint32_t round, uint32_t iteration, int mode, int key_bits, uint64_t first_region, const uint8_t* d_labeled,
                         const int32_t* d_sp_cloud, size_t S, size_t num_clouds, size_t total_num, const int64_t* d_count, int32_t* d_items, size_t max_items,
                         int32_t* d_n_items, int64_t* d_info, void* stream) {
    SSDR_TRY(draw_refusals("region_draw", mode, key_bits, d_labeled, d_sp_cloud, S, num_clouds, total_num, d_count, d_items, max_items, d_n_items, d_info, first_region));
    SSDR_TRY(ensure_init());
    return draw_chain(seed, round, iteration, mode, key_bits, first_region, 0, 1, nullptr, num_clouds, d_labeled, d_sp_cloud, S, num_clouds, total_num, d_count, d_items, nullptr,
                      max_items, d_n_items, d_info, pick_stream(stream));
}

int ssdr_region_draw_count_dev(const uint8_t* d_labeled, const int32_t* d_sp_cloud, size_t S, size_t num_clouds, int32_t* d_u, size_t cloud_slots, void* stream) {
    if (!d_labeled || !d_sp_cloud || !d_u) { set_error("region_draw_count: NULL pointer"); return SSDR_ERR_INVALID; }
    if (S == 0 || num_clouds == 0 || cloud_slots < num_clouds) { set_error("region_draw_count: %zu regions of %zu clouds in %zu cloud slots", S, num_clouds, cloud_slots); return SSDR_ERR_INVALID; }
    if (S > RD_MAX || cloud_slots > RD_MAX) { set_error("region_draw_count: more than 0x3fffffff regions or cloud slots"); return SSDR_ERR_UNSUPPORTED; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    DrawArgs a{}; a.labeled = d_labeled; a.sp_cloud = d_sp_cloud; a.S = (int)S; a.B = (int)num_clouds; a.u = d_u; a.CS = (int)cloud_slots;
    ProfScope prof("region_draw_count", s, 5.0 * (double)S);
    SSDR_HIP(hipMemsetAsync(d_u, 0, 4 * (cloud_slots + 1), s));
    hipLaunchKernelGGL(rd_count, dim3(rd_blocks(S)), dim3(RD_BS), 0, s, a);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_region_draw_sharded_dev(uint64_t seed, uint32_t round, uint32_t iteration, int mode, int key_bits, uint64_t first_region, int rank, int world,
                                 const int32_t* d_u_all, size_t cloud_slots, const uint8_t* d_labeled, const int32_t* d_sp_cloud, size_t S, size_t num_clouds,
                                 size_t total_num, const int64_t* d_count, int32_t* d_items, int32_t* d_item_pos, size_t max_items, int32_t* d_n_items, int64_t* d_info,
                                 void* stream) {
    SSDR_TRY(draw_refusals("region_draw_sharded", mode, key_bits, d_labeled, d_sp_cloud, S, num_clouds, total_num, d_count, d_items, max_items, d_n_items, d_info, first_region));
    if (!d_u_all || (max_items && !d_item_pos)) { set_error("region_draw_sharded: NULL pointer"); return SSDR_ERR_INVALID; }
    if (world <= 0 || rank < 0 || rank >= world || cloud_slots < num_clouds) {
        set_error("region_draw_sharded: rank %d of %d, %zu clouds in %zu cloud slots", rank, world, num_clouds, cloud_slots); return SSDR_ERR_INVALID;
    }
    if (cloud_slots > RD_MAX || (size_t)world * cloud_slots > RD_MAX || first_region > RD_MAX || first_region + S > RD_MAX) {
        set_error("region_draw_sharded: more than 0x3fffffff cloud slots or regions over all ranks"); return SSDR_ERR_UNSUPPORTED;
    }
    SSDR_TRY(ensure_init());
    return draw_chain(seed, round, iteration, mode, key_bits, first_region, rank, world, d_u_all, cloud_slots, d_labeled, d_sp_cloud, S, num_clouds, total_num, d_count, d_items,
                      d_item_pos, max_items, d_n_items, d_info, pick_stream(stream));
}

int ssdr_region_draw_shares(void* stream, int32_t* out, size_t n) {
    if (!out && n) { set_error("region_draw_shares: NULL pointer"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); RegionDrawState& Q = rds(s);
    if (n > Q.B) { set_error("region_draw_shares: %zu entries asked, the newest draw on this stream had %zu clouds", n, Q.B); return SSDR_ERR_INVALID; }
    if (n) SSDR_HIP(hipMemcpyAsync(out, Q.tab.as<int>() + 3 * Q.B, 4 * n, hipMemcpyDeviceToHost, s));
    SSDR_HIP(hipStreamSynchronize(s));
    return SSDR_OK;
}

int ssdr_seed_label_dev(const int32_t* d_gt, size_t n, const int32_t* d_sp_off, const int32_t* d_sp_pts, size_t S, const int32_t* d_items, const int32_t* d_n_items,
                        size_t max_items, size_t max_region, float* d_mask, float* d_label, uint8_t* d_labeled, int64_t* d_out, void* stream) {
    if (!d_gt || !d_sp_off || !d_sp_pts || !d_n_items || !d_mask || !d_label || !d_labeled || !d_out || (max_items && !d_items)) { set_error("seed_label: NULL pointer"); return SSDR_ERR_INVALID; }
    if (S == 0) { set_error("seed_label: no regions"); return SSDR_ERR_INVALID; }
    if (S > 0x7ffffff0 || n > 0x7ffffff0 || max_items > RD_MAX) { set_error("seed_label: more than 0x7ffffff0 regions or points, or 0x3fffffff items"); return SSDR_ERR_UNSUPPORTED; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); RegionDrawState& Q = rds(s);
    const size_t M = max_items;
    SSDR_TRY(Q.big.reserve(4 * (M + 1)));
    SeedArgs a{d_gt, (long long)n, d_sp_off, d_sp_pts, (int)S, d_items, d_n_items, (int)M, d_mask, d_label, d_labeled, reinterpret_cast<unsigned long long*>(d_out),
               Q.big.as<int>() + 1, Q.big.as<int>()};
    ProfScope prof("seed_label", s, 0.0);
    SSDR_HIP(hipMemsetAsync(d_out, 0, 24, s));
    SSDR_HIP(hipMemsetAsync(Q.big.p, 0, 4, s));
    if (M) {
        const unsigned cap = (unsigned)ctx().num_cu;
        hipLaunchKernelGGL(seed_label_wave, dim3((unsigned)std::max<size_t>(1, std::min<size_t>((M + 3) / 4, (size_t)cap * 16))), dim3(RD_BS), 0, s, a);
        if (max_region == 0 || max_region > (size_t)SD_WAVE_MAX)
            hipLaunchKernelGGL(seed_label_block, dim3((unsigned)std::max<size_t>(1, std::min<size_t>(M, (size_t)cap * 4))), dim3(RD_BS), 0, s, a);
    }
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

}
