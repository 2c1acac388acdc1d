// Farthest-point and k-center sampling of the selection stage for gfx950 (F4 farthest_features_sample, S3/fps_gcn_cpu.py:119-147; F5 kCenterGreedy,
// S3/kcenterGreedy.py:60-128; farthest_superpoint_sample, S3/sampler2.py:49-80): the wave arg-max, the chain kernels, the seeding kernels, the account
// of cooperative grids in flight, and the launcher fps_like() behind ssdr_fps_dev, ssdr_kcenter_dev, the one-call chain of select.hip and the sharded
// ssdr_*_gathered_dev entries.
//
// A chain is `count` dependent picks: per pick every row's running minimum distance to the centres picked so far is updated and the row with the
// largest one (the lowest index among equal values, np.argmax) becomes the next centre.  Distances are float64 sums in NumPy's pairwise order
// (np_sum.hpp), so identical inputs give the reference's index sequence.  A pick is microseconds of work, so the chain is shaped by what stands between
// two picks.  Up to 1536 rows of 32 features one workgroup holds everything in registers (fps_block_reg) and a pick costs two barriers; a few thousand
// rows of any length one workgroup sweeps from L2 (fps_block).  Above, G co-resident workgroups run the whole chain in ONE launch and hand their partial
// maxima to each other once per pick, with no cache write-back / invalidate on either side: fps_coop_split (32 features, rows in registers) publishes
// self-validating records (data and pick number in one granule) with write-through (sc1) stores that the readers poll with sc1 loads; fps_coop (any
// length, features from L2) drains its stores and counts arrivals.  Both wait a bounded time that ends in an abort word and the stream's status word
// (ssdr_select_status), never in a wrong selection.  Beyond what can be co-resident there is one launch per pick (fps_step).
//
// The launcher is a plan and a launch: fps_env() reads the environment switches once per process, fps_plan() decides seeding, form, grid and the form's
// parameters from (n, D, seeded, na, num_cu, env) and launches nothing, fps_like() seeds and switches on the plan's form.  DESIGN.md section 13 is the
// decision as a table; tests/test_fps_paths.py holds every row of it.
#include <cstdlib>
#include <cstring>
#include "ssdr_internal.hpp"
#include "np_sum.hpp"
#include "select_fps.hpp"

namespace ssdr {
namespace {

// ---- F4: farthest_features_sample (fps_gcn_cpu.py:119-147) / F5: kCenterGreedy (kcenterGreedy.py:84-128) --------
struct Part { double v; int i; int pad; };

// Wavefront arg-max of (value, index) pairs, result in every lane.  The picks of FPS / k-center form a serial chain of
// ~600 such reductions: inside a row of 16 lanes the partners come through DPP (quad permutes, half-row and row mirrors),
// across rows through gfx950's v_permlane16_swap / v_permlane32_swap — no LDS crossbar round trips (ds_bpermute) at all.
// Two passes (round 4): the maximum of the VALUES alone (two moves and one v_max_f64 per step), then the smallest index among the lanes
// that hold it (one v_min_i32 per step) — 30 dependent instructions instead of 65 for the (value, index) pairs compared step by step,
// on a chain where a float64 instruction of a lone wave takes 12 cycles (tools/micro/valu_rate.hip).  Values are never NaN here.
#ifndef HIPEMU
__device__ __forceinline__ double max_f64(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
template <int CTRL> __device__ __forceinline__ unsigned dpp_u32(unsigned x) { return (unsigned)__builtin_amdgcn_update_dpp((int)x, (int)x, CTRL, 0xf, 0xf, true); }
template <int CTRL> __device__ __forceinline__ double dpp_max_f64(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = dpp_u32<CTRL>((unsigned)b), hi = dpp_u32<CTRL>((unsigned)(b >> 32));
    return max_f64(v, __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)));
}
template <int CTRL> __device__ __forceinline__ int dpp_min_i32(int t) { return min(t, (int)dpp_u32<CTRL>((unsigned)t)); }
// ... inside every row of 16 lanes (0xB1 quad_perm [1,0,3,2], 0x4E quad_perm [2,3,0,1], 0x141 row_half_mirror, 0x140 row_mirror)
__device__ __forceinline__ double row_max_f64(double v) { v = dpp_max_f64<0xB1>(v); v = dpp_max_f64<0x4E>(v); v = dpp_max_f64<0x141>(v); return dpp_max_f64<0x140>(v); }
__device__ __forceinline__ int row_min_i32(int t) { t = dpp_min_i32<0xB1>(t); t = dpp_min_i32<0x4E>(t); t = dpp_min_i32<0x141>(t); return dpp_min_i32<0x140>(t); }
#endif
__device__ __forceinline__ void wave_argmax(double& v, int& i) {
#ifndef HIPEMU
    double m = row_max_f64(v);
    // rows 0<->1, 2<->3, then the halves: after swap(a, a) the two results hold the even / odd row (half) of each pair
    {
        const long long b = __double_as_longlong(m);
        auto lo = __builtin_amdgcn_permlane16_swap((unsigned)b, (unsigned)b, false, false), hi = __builtin_amdgcn_permlane16_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
        m = max_f64(__longlong_as_double((long long)(((unsigned long long)hi[0] << 32) | lo[0])), __longlong_as_double((long long)(((unsigned long long)hi[1] << 32) | lo[1])));
    }
    {
        const long long b = __double_as_longlong(m);
        auto lo = __builtin_amdgcn_permlane32_swap((unsigned)b, (unsigned)b, false, false), hi = __builtin_amdgcn_permlane32_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
        m = max_f64(__longlong_as_double((long long)(((unsigned long long)hi[0] << 32) | lo[0])), __longlong_as_double((long long)(((unsigned long long)hi[1] << 32) | lo[1])));
    }
    int t = row_min_i32(v == m ? i : 0x7fffffff);
    { auto r = __builtin_amdgcn_permlane16_swap((unsigned)t, (unsigned)t, false, false); t = min((int)r[0], (int)r[1]); }
    { auto r = __builtin_amdgcn_permlane32_swap((unsigned)t, (unsigned)t, false, false); t = min((int)r[0], (int)r[1]); }
    v = m; i = t;
#else
    for (int o = 32; o > 0; o >>= 1) {
        const long long b = __double_as_longlong(v);
        const unsigned lo = __shfl_xor((unsigned)b, o), hi = __shfl_xor((unsigned)(b >> 32), o);
        const double ov = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
        const int oi = __shfl_xor(i, o);
        if (better(ov, oi, v, i)) { v = ov; i = oi; }
    }
#endif
}
// the index of the best of NW <= 16 (value, index) pairs in LDS, in every lane of the calling wave: lanes 0..NW-1 take one pair each and reduce
// inside their row of 16 (the other rows reduce padding)
template <int NW> __device__ __forceinline__ int pairs_argmax_index(const double* sv, const int* si, int lane) {
    static_assert(NW <= 16, "one row of lanes");
#ifndef HIPEMU
    const double v = lane < NW ? sv[lane] : -2.0;
    const int i = lane < NW ? si[lane] : 0x7fffffff;
    const double m = row_max_f64(v);
    return __builtin_amdgcn_readfirstlane(row_min_i32(v == m ? i : 0x7fffffff));
#else
    (void)lane;
    double bv = sv[0]; int bi = si[0];
    for (int w = 1; w < NW; ++w) if (better(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
    return bi;
#endif
}

// One step: (1) every block reduces the previous step's partial maxima to learn the current centre,
// (2) updates the running min-distance of its points, (3) publishes its own partial maximum.
__global__ __launch_bounds__(256) void fps_step(const double* __restrict__ f, int n, int D, int from_partials, int start, int use_sqrt,
                                                const Part* __restrict__ pin, int npart, Part* pout, double* mind, int* out, const int* __restrict__ dn = nullptr) {
    __shared__ Part s_p[256];
    if (dn) n = min(n, *dn);
    __shared__ int s_c;
    const int tid = threadIdx.x;
    if (!from_partials) { if (tid == 0) s_c = start; }
    else {
        Part b; b.v = -1.0; b.i = 0x7fffffff;
        for (int k = tid; k < npart; k += 256) if (better(pin[k].v, pin[k].i, b.v, b.i)) b = pin[k];
        s_p[tid] = b;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if (tid < o && better(s_p[tid + o].v, s_p[tid + o].i, s_p[tid].v, s_p[tid].i)) s_p[tid] = s_p[tid + o]; __syncthreads(); }
        if (tid == 0) s_c = s_p[0].i;
    }
    __syncthreads();
    const int c = s_c;
    if (blockIdx.x == 0 && tid == 0 && out) *out = c;
    __syncthreads();
    if (!pout) return;
    const double* fc = f + (size_t)c * D;
    Part b; b.v = -1.0; b.i = 0x7fffffff;
    for (int i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) {
        const double* fi = f + (size_t)i * D;
        double dist = np_pairwise<double>([&](int k) { const double d = fi[k] - fc[k]; return d * d; }, D);
        if (use_sqrt) dist = sqrt(dist);
        double m = mind[i];
        if (dist < m) { m = dist; mind[i] = m; }
        if (better(m, i, b.v, b.i)) { b.v = m; b.i = i; }
    }
    s_p[tid] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o && better(s_p[tid + o].v, s_p[tid + o].i, s_p[tid].v, s_p[tid].i)) s_p[tid] = s_p[tid + o]; __syncthreads(); }
    if (tid == 0) pout[blockIdx.x] = s_p[0];
}

// Whole FPS / k-center chain in ONE workgroup (no launch per iteration) for candidate sets that one CU can sweep
// per step.  DF > 0: feature length known at compile time; the first two points of every thread stay in registers
// (n <= 2048 -> no global feature traffic inside the loop).  mind[] lives in global memory; the arg-max is a wave
// shuffle + LDS reduction.
template <int DF>
__global__ __launch_bounds__(1024) void fps_block(const double* __restrict__ f, int n, int D, int from_partials, int start, int use_sqrt,
                                                  const Part* __restrict__ pin, int npart, double* mind, int count, int* out, const int* __restrict__ dn = nullptr) {
    if (dn) n = min(n, *dn);
    __shared__ double s_v[16];
    __shared__ int s_i[16];
    __shared__ int s_c;
    __shared__ double s_fc[DF > 0 ? DF : 1];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    auto block_argmax = [&](double v, int i) {
        wave_argmax(v, i);
        if (lane == 0) { s_v[wid] = v; s_i[wid] = i; }
        __syncthreads();
        if (tid == 0) {
            double bv = s_v[0]; int bi = s_i[0];
            for (int w = 1; w < 16; ++w) if (better(s_v[w], s_i[w], bv, bi)) { bv = s_v[w]; bi = s_i[w]; }
            s_c = bi;
        }
        __syncthreads();
    };
    constexpr int NR = 0;   // points per thread kept in registers: none (64 doubles per point spill at 1024 threads); L2 serves them
    double reg[NR > 0 ? NR : 1][DF > 0 ? DF : 1];
    double rmin[NR > 0 ? NR : 1];
    if (DF > 0) {
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            const int i = tid + q * 1024;
            rmin[q] = i < n ? mind[i] : -1.0;
#pragma unroll
            for (int k = 0; k < (DF > 0 ? DF : 1); ++k) reg[q][k] = i < n ? f[(size_t)i * D + k] : 0.0;
        }
    }
    if (!from_partials) { if (tid == 0) s_c = start; __syncthreads(); }
    else {
        double v = -1.0; int i = 0x7fffffff;
        for (int k = tid; k < npart; k += 1024) if (better(pin[k].v, pin[k].i, v, i)) { v = pin[k].v; i = pin[k].i; }
        block_argmax(v, i);
    }
    for (int it = 0; it < count; ++it) {
        const int c = s_c;
        if (tid == 0) out[it] = c;
        if (it + 1 == count) break;
        const double* fc = f + (size_t)c * D;
        if (DF > 0) { if (tid < DF) s_fc[tid] = fc[tid]; __syncthreads(); }
        double bv = -1.0; int bi = 0x7fffffff;
        if (DF > 0) {
#pragma unroll
            for (int q = 0; q < NR; ++q) {
                const int i = tid + q * 1024;
                if (i < n) {
                    double dist = np_pairwise_fixed<(DF > 0 ? DF : 8)>([&](int k) { const double d = reg[q][k] - s_fc[k]; return d * d; });
                    if (use_sqrt) dist = sqrt(dist);
                    if (dist < rmin[q]) rmin[q] = dist;
                    if (better(rmin[q], i, bv, bi)) { bv = rmin[q]; bi = i; }
                }
            }
        }
        for (int i = tid + NR * 1024; i < n; i += 1024) {
            const double* fi = f + (size_t)i * D;
            double dist;
            if (DF > 0) dist = np_pairwise_fixed<(DF > 0 ? DF : 8)>([&](int k) { const double d = fi[k] - s_fc[k]; return d * d; });
            else dist = np_pairwise<double>([&](int k) { const double d = fi[k] - fc[k]; return d * d; }, D);
            if (use_sqrt) dist = sqrt(dist);
            double m = mind[i];
            if (dist < m) { m = dist; mind[i] = m; }
            if (better(m, i, bv, bi)) { bv = m; bi = i; }
        }
        __syncthreads();          // everyone has read s_c / s_fc
        block_argmax(bv, bi);
    }
}

// Register-resident variant for small candidate sets (n <= 512 * PPT): every thread owns PPT points whose features
// and running min-distance never leave its registers; the current centre's features are published through LDS by
// the owning thread, so the loop touches global memory only to store the selected index.
template <int DF, int PPT, int NT>
__global__ __launch_bounds__(NT) void fps_block_reg(const double* __restrict__ f, int n, int from_partials, int start, int use_sqrt,
                                                    const Part* __restrict__ pin, int npart, const double* __restrict__ mind, int count, int* out,
                                                    const int* __restrict__ dn = nullptr) {
    if (dn) n = min(n, *dn);
    constexpr int NW = NT / 64;
    __shared__ double s_v[2][NW];
    __shared__ int s_i[2][NW];
    __shared__ double s_fc[2][DF];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    double reg[PPT][DF], rmin[PPT];
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const int i = tid + q * NT;
        rmin[q] = i < n ? mind[i] : -1.0;
#pragma unroll
        for (int k = 0; k < DF; ++k) reg[q][k] = i < n ? f[(size_t)i * DF + k] : 0.0;
    }
    // publishes this wave's best into s_v/s_i[par]; after the barrier every wave reduces the NW wave results itself
    auto block_argmax = [&](double v, int i, int par) -> int {
        wave_argmax(v, i);
        if (lane == 0) { s_v[par][wid] = v; s_i[par][wid] = i; }
        __syncthreads();
        return pairs_argmax_index<NW>(s_v[par], s_i[par], lane);
    };
    int c;
    if (!from_partials) c = start;
    else {
        double v = -1.0; int i = 0x7fffffff;
        for (int k = tid; k < npart; k += NT) if (better(pin[k].v, pin[k].i, v, i)) { v = pin[k].v; i = pin[k].i; }
        c = block_argmax(v, i, 1);
    }
    for (int it = 0; it < count; ++it) {
        const int par = it & 1;
        if (tid == 0) out[it] = c;
        if (it + 1 == count) break;
#pragma unroll
        for (int q = 0; q < PPT; ++q) if (c == tid + q * NT) {
#pragma unroll
            for (int k = 0; k < DF; ++k) s_fc[par][k] = reg[q][k];
        }
        __syncthreads();
        double bv = -1.0; int bi = 0x7fffffff;
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const int i = tid + q * NT;
            if (i < n) {
                double dist = np_pairwise_fixed<DF>([&](int k) { const double d = reg[q][k] - s_fc[par][k]; return d * d; });
                if (use_sqrt) dist = sqrt(dist);
                if (dist < rmin[q]) rmin[q] = dist;
                if (better(rmin[q], i, bv, bi)) { bv = rmin[q]; bi = i; }
            }
        }
        c = block_argmax(bv, bi, par);       // two barriers per iteration; parity double-buffering covers the reuse
    }
}

// FPS / k-center over more candidates than one workgroup sweeps per pick, for any feature length (every D != 32 above 4096 rows, D = 32 above the rows
// fps_coop_split below holds in registers): ONE launch of G co-resident workgroups instead of a launch per pick (the reference's AL rounds pick 10 000 of
// ~2 x 10^4 regions, ssdr_main_S3DIS2.py:134: 10^4 dependent launches).  The features stay in the table; every workgroup keeps the running min-distance
// of its FC_NT * FC_PPT points in registers.  Per pick it publishes its partial arg-max with write-through (sc1) stores, drains them, adds to a counter;
// all workgroups poll that counter and read the G partials with sc1 loads (the fence-free hand-off of MI355X_MICROARCH.md, "Valid forms": 9.3 us per pick
// with __threadfence on both sides, measured), and each reduces them itself.  Partials and counters alternate between two sets by the parity of the pick,
// so a workgroup that runs ahead never overwrites what a slower one still reads.
constexpr int FC_NT = 256, FC_PPT = 8;
struct FpsCoopArgs { const double* f; int n, D, from_partials, start, use_sqrt; const Part* pin; int npart; const double* mind; int count; int* out; Part* part; int* sync; int G; int* status; const int* dn; };
constexpr long FPS_COOP_SPINS = 1L << 22;      // ~0.3 s of polling: a pick among co-resident workgroups takes microseconds
// sync[0], sync[1]: arrival counters by pick parity; sync[2]: abort — a workgroup waited FPS_COOP_SPINS polls for one that never arrived (the launch was
// not co-resident).  It is checked at every pick by every workgroup, which then leaves (the picks from there on read -1), and the stream's selection
// status word takes bit 0: ssdr_select_status turns it into an error, so a launch that is not co-resident never ends in a wrong selection.
// fps_coop_split has no counters: its records carry the pick number, and it shares the abort word and the bound.
#ifndef HIPEMU
__global__ __launch_bounds__(FC_NT) void fps_coop(FpsCoopArgs a) {
    if (a.dn) a.n = min(a.n, *a.dn);
    __shared__ double s_v[FC_NT / 64]; __shared__ int s_i[FC_NT / 64]; __shared__ double s_fc[128];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = blockIdx.x, G = a.G;
    auto block_argmax = [&](double v, int i, double& ov, int& oi) {
        wave_argmax(v, i);
        if (lane == 0) { s_v[wid] = v; s_i[wid] = i; }
        __syncthreads();
        ov = s_v[0]; oi = s_i[0];
#pragma unroll
        for (int w = 1; w < FC_NT / 64; ++w) if (better(s_v[w], s_i[w], ov, oi)) { ov = s_v[w]; oi = s_i[w]; }
        __syncthreads();
    };
    // this workgroup's points: i = (k * G + g) * FC_NT + tid
    double rmin[FC_PPT];
#pragma unroll
    for (int k = 0; k < FC_PPT; ++k) { const long i = ((long)k * G + g) * FC_NT + tid; rmin[k] = i < a.n ? a.mind[i] : -1.0; }
    int c;
    if (!a.from_partials) c = a.start;
    else {
        double v = -1.0; int i = 0x7fffffff;
        for (int k = tid; k < a.npart; k += FC_NT) if (better(a.pin[k].v, a.pin[k].i, v, i)) { v = a.pin[k].v; i = a.pin[k].i; }
        double ov; block_argmax(v, i, ov, c);
    }
    __shared__ int s_abort;
    for (int it = 0; it < a.count; ++it) {
        if (tid == 0) s_abort = __hip_atomic_load(&a.sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (s_abort) { if (g == 0) for (int k = it + tid; k < a.count; k += FC_NT) a.out[k] = -1; return; }
        if (g == 0 && tid == 0) a.out[it] = c;
        if (it + 1 == a.count) break;
        const double* fc = a.f + (size_t)c * a.D;
        if (a.D <= 128) { if (tid < a.D) s_fc[tid] = fc[tid]; __syncthreads(); }
        double bv = -1.0; int bi = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < FC_PPT; ++k) {
            const long i = ((long)k * G + g) * FC_NT + tid;
            if (i < a.n) {
                const double* fi = a.f + (size_t)i * a.D;
                double dist;
                if (a.D == 32) dist = np_pairwise_fixed<32>([&](int q) { const double d = fi[q] - s_fc[q]; return d * d; });
                else if (a.D <= 128) dist = np_pairwise<double>([&](int q) { const double d = fi[q] - s_fc[q]; return d * d; }, a.D);
                else dist = np_pairwise<double>([&](int q) { const double d = fi[q] - fc[q]; return d * d; }, a.D);
                if (a.use_sqrt) dist = sqrt(dist);
                if (dist < rmin[k]) rmin[k] = dist;
                if (better(rmin[k], (int)i, bv, bi)) { bv = rmin[k]; bi = (int)i; }
            }
        }
        double wv; int wi;
        block_argmax(bv, bi, wv, wi);
        const int par = it & 1;
        Part* P = a.part + (size_t)par * G;
        if (tid == 0) {
            // write-through (sc1) stores of the partial, drained, then the arrival: no cache write-back / invalidate on either side
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(&P[g].v), (unsigned long long)__double_as_longlong(wv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&P[g].i, wi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_fetch_add(&a.sync[par], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int want = G * (it / 2 + 1);
            long spins = 0;
            while (__hip_atomic_load(&a.sync[par], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > FPS_COOP_SPINS || __hip_atomic_load(&a.sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { atomicOr(&a.sync[2], 1); atomicOr(a.status, 1); break; }
            }
        }
        __syncthreads();
        double v = -1.0; int i = 0x7fffffff;
        for (int k = tid; k < G; k += FC_NT) {
            const double pv = __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long*>(&P[k].v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const int pi = __hip_atomic_load(&P[k].i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (better(pv, pi, v, i)) { v = pv; i = pi; }
        }
        double ov; block_argmax(v, i, ov, c);
    }
}
#endif

#ifndef HIPEMU
// The chain for 32-d features, the reference's own scale included (10 000 picks over 20 000 candidates, ssdr_main_S3DIS2.py:134): every workgroup keeps its
// rows IN REGISTERS for the whole chain, 256 rows on 512 threads.  A pick at that scale is nearly all latency: the dependent float64 instructions of one
// row's distance, the arg-max, and the all-to-all of the G partials through the fabric.  The kernel is shaped against each of them:
//  * a ROW IS SPLIT OVER TWO LANES: NumPy's eight pairwise accumulators are dealt to the lanes (lane q owns accumulators 4 q .. 4 q + 3, i.e. features
//    8 k + 4 q + e), each lane adds its accumulators in the reference's order and the tree ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) closes through one quad
//    exchange (a + b == b + a bit for bit): 50 dependent instructions instead of the 95 of a whole row in one lane;
//  * a RECORD IS ONE 16-BYTE SLOT: two self-validating 8-byte granules {value half, 16-bit tag | index half}, the tag being the pick number — one lane
//    publishes it with ONE write-through store, ONE wave sweeps all G slots with every load in flight and re-reads only the slots whose tag is not there
//    yet: no drain, no counter, no second round trip.  Slots alternate between two sets by the parity of the pick (a workgroup is at most one pick ahead
//    of the slowest).  The winner's ROW is read from the feature table itself (immutable during the chain: plain, cacheable loads, every lane straight into
//    its registers) and does not travel in the records;
//  * the wait is bounded like fps_coop's: a sweep that gives up sets the abort word and the stream's status word, and every workgroup leaves.
// G = ceil(n / 256) workgroups, 79 at 20 000 rows; a sweeping lane takes up to four slots, so G <= 256.
template <int CTRL> __device__ __forceinline__ double dpp_f64(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = dpp_u32<CTRL>((unsigned)b), hi = dpp_u32<CTRL>((unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
typedef unsigned fs_u4 __attribute__((ext_vector_type(4)));
constexpr int FQ_NT = 512, FQ_LPR = 2, FQ_ROWS = FQ_NT / FQ_LPR, FQ_MAXG = 256;      // threads, lanes per row, rows per workgroup, slots one sweeping wave takes
constexpr int FR_ROWS = 512;         // the form's bracket: up to this many rows for each of half the CUs, i.e. at most one workgroup per CU (fps_plan)
// TIMED (development, SSDR_FPS_DBG=1): wave 0 of every workgroup accumulates its clock between the phases of a pick into dbg[g][8]
template <bool TIMED>
__global__ __launch_bounds__(FQ_NT) void fps_coop_split(FpsCoopArgs a, int slot_shift, int delay, long long* dbg) {
    constexpr int LPR = FQ_LPR, A = 8 / LPR, F = 32 / LPR, ROWS = FQ_ROWS, NW = FQ_NT / 64, P = FQ_MAXG / 64;      // 64 P >= G slots per sweeping lane
    static_assert(A == 4, "four of the eight pairwise accumulators per lane, one quad exchange");
    if (a.dn) a.n = min(a.n, *a.dn);
    long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = 0;
    auto mark = [&](int k) { if (TIMED) { const long long t = (long long)__builtin_readcyclecounter(); tacc[k] += t - tprev; tprev = t; } };
    __shared__ double s_v[2][NW]; __shared__ int s_i[2][NW]; __shared__ int s_c[2], s_gave;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = blockIdx.x, G = a.G, q = tid & (LPR - 1);
    if (tid == 0) s_gave = 0;
    const int row = g * ROWS + tid / LPR;
    // this lane's share of its row: x[k * A + e] = f[row][8 k + A q + e]
    double x[F], rmin = row < a.n ? a.mind[row] : -1.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < A; ++e) x[k * A + e] = row < a.n ? a.f[(size_t)row * 32 + 8 * k + A * q + e] : 0.0;
    int c;
    if (!a.from_partials) c = a.start;
    else {
        double v = -1.0; int i = 0x7fffffff;
        for (int k = tid; k < a.npart; k += FQ_NT) if (better(a.pin[k].v, a.pin[k].i, v, i)) { v = a.pin[k].v; i = a.pin[k].i; }
        wave_argmax(v, i);
        if (lane == 0) { s_v[0][wid] = v; s_i[0][wid] = i; }
        __syncthreads();
        v = s_v[0][0]; c = s_i[0][0];
        for (int w = 1; w < NW; ++w) if (better(s_v[0][w], s_i[0][w], v, c)) { v = s_v[0][w]; c = s_i[0][w]; }
    }
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.part, 0, (2 * G) << slot_shift, 0x00020000);
    // The first polling pass WAITS `delay` units of 64 cycles: a pass that finds a record missing costs another round trip through the fabric (~2300 cycles), and right
    // behind the workgroup's own store the other workgroups' records are still on their way (1.6 passes per pick at 20 000 rows, 1.1 with 16 units).  Fixed delays
    // measured at seven row counts (SSDR_FPS_DELAY, profiles/r06_fps_poll_delay.txt): the best is 16 units up to ~70 workgroups and 20 above (20 000 rows 2.78
    // -> 2.60 us per pick, 9 472 rows 2.65 -> 2.37, 65 000 rows 3.29 -> 2.92); 24 is already slower everywhere.  A per-workgroup controller on the miss rate (two units
    // more after a missed pass, one less after sixteen clean picks) was built and drifts upwards — a few per cent of the picks have a straggler whatever the delay.
    const int dly = delay;
    for (int it = 0; it < a.count; ++it) {
        if (g == 0 && tid == 0) a.out[it] = c;
        if (it + 1 == a.count) break;
        const int par = it & 1;
        if (TIMED) tprev = (long long)__builtin_readcyclecounter();
        // the centre's row, this lane's share of it, from the table
        double fc[F];
        {
            const double* src = a.f + (size_t)c * 32 + A * q;
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int e = 0; e < A; ++e) fc[k * A + e] = src[8 * k + e];
        }
        mark(0);
        double wv = -1.0; int wi = 0x7fffffff;
        {
            double r[A];
#pragma unroll
            for (int e = 0; e < A; ++e) { const double d = x[e] - fc[e]; r[e] = d * d; }
#pragma unroll
            for (int k = 1; k < 4; ++k)
#pragma unroll
                for (int e = 0; e < A; ++e) { const double d = x[k * A + e] - fc[k * A + e]; r[e] += d * d; }
            double p = (r[0] + r[1]) + (r[2] + r[3]);
            p = p + dpp_f64<0xB1>(p);          // the neighbouring lane's half of the tree
            if (a.use_sqrt) p = sqrt(p);
            if (row < a.n) { if (p < rmin) rmin = p; wv = rmin; wi = row; }
        }
        mark(1);
        wave_argmax(wv, wi);
        if (lane == 0) { s_v[par][wid] = wv; s_i[par][wid] = wi; }
        mark(2);
        __syncthreads();                                   // (1)
        mark(3);
        if (wid == 0) {
            // the eight waves' pairs: one per lane, reduced inside the row of 16 lanes (two DPP passes instead of a chain of eight dependent compares)
            const double pv0 = lane < NW ? s_v[par][lane] : -2.0;
            const int pi0 = lane < NW ? s_i[par][lane] : 0x7fffffff;
            const double bv = row_max_f64(pv0);
            const int bi = row_min_i32(pv0 == bv ? pi0 : 0x7fffffff);
            const unsigned tag = ((unsigned)it % 0xffffu + 1u) << 16;
            const unsigned base = (unsigned)(par * G) << slot_shift;
            if (lane == 0) {
                const unsigned long long b = (unsigned long long)__double_as_longlong(bv);
                fs_u4 v; v.x = (unsigned)b; v.y = tag | ((unsigned)bi >> 16); v.z = (unsigned)(b >> 32); v.w = tag | ((unsigned)bi & 0xffffu);
                __builtin_amdgcn_raw_buffer_store_b128(v, rs, base + ((unsigned)g << slot_shift), 0, 16);      // sc1: write-through
            }
            mark(4);
            // every record of the pick: all of a lane's slots in flight, the missing ones again
            double v = -1.0; int i = 0x7fffffff; bool gave_up = false; int passes = 0;
            for (int k0 = lane; k0 < G && !gave_up; k0 += P * 64) {
                unsigned pend = 0;
#pragma unroll
                for (int j = 0; j < P; ++j) if (k0 + j * 64 < G) pend |= 1u << j;
                long spins = 0;
                for (int z = 0; z < dly; ++z) __builtin_amdgcn_s_sleep(1);
                while (pend) {
                    fs_u4 u[P];
                    if (TIMED) ++passes;
#pragma unroll
                    for (int j = 0; j < P; ++j) if ((pend >> j) & 1u) u[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, base + ((unsigned)(k0 + j * 64) << slot_shift), 0, 16);
#pragma unroll
                    for (int j = 0; j < P; ++j)
                        if (((pend >> j) & 1u) && (u[j].y & 0xffff0000u) == tag && (u[j].w & 0xffff0000u) == tag) {
                            const double pv = __longlong_as_double((long long)(((unsigned long long)u[j].z << 32) | u[j].x));
                            const int pi = (int)(((u[j].y & 0xffffu) << 16) | (u[j].w & 0xffffu));
                            if (better(pv, pi, v, i)) { v = pv; i = pi; }
                            pend &= ~(1u << j);
                        }
                    if (pend && (++spins > FPS_COOP_SPINS / 16 || (spins % 1024 == 0 && __hip_atomic_load(&a.sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))) { gave_up = true; break; }
                }
            }
            if (gave_up) { atomicOr(&a.sync[2], 1); atomicOr(a.status, 1); s_gave = 1; }
            mark(5);
            if (TIMED) tacc[7] += passes;
            wave_argmax(v, i);
            if (lane == 0) s_c[par] = i;
        }
        __syncthreads();                                   // (2)
        mark(6);
        if (s_gave) { if (g == 0) for (int k = it + 1 + tid; k < a.count; k += FQ_NT) a.out[k] = -1; return; }
        c = s_c[par];
    }
    if (TIMED && tid == 0) for (int k = 0; k < 8; ++k) dbg[(size_t)g * 8 + k] = tacc[k];
}
#endif

// farthest_superpoint_sample (sampler2.py:49-80, the "edcd" branch): FPS over one cloud's superpoints with the
// distance |centre_i - centre_c|^2 + CD(i, c), CD = dir + dir^T from sel_chamfer_dir.  One workgroup, n <= a few thousand.
__global__ __launch_bounds__(256) void fps_superpoint(const double* __restrict__ centres, const double* __restrict__ dir, int n, int start, int count, int* out) {
    __shared__ double s_v[256];
    __shared__ int s_i[256];
    SSDR_DYN_SHARED(double, mind);          // [n]
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += 256) mind[i] = 1.0e10;
    int c = start;
    __syncthreads();
    for (int it = 0; it < count; ++it) {
        if (tid == 0) out[it] = c;
        if (it + 1 == count) break;
        double bv = -1.0; int bi = 0x7fffffff;
        for (int i = tid; i < n; i += 256) {
            const double dx = centres[3 * i] - centres[3 * c], dy = centres[3 * i + 1] - centres[3 * c + 1], dz = centres[3 * i + 2] - centres[3 * c + 2];
            const double ed = (dx * dx + dy * dy) + dz * dz;                                  // np.sum(.., axis=-1) over 3 terms
            const double cd = (i == c) ? 0.0 : dir[(size_t)c * n + i] + dir[(size_t)i * n + c];   // chamfer_distance(..)[i]: av_dist1 + av_dist2
            const double dist = ed + cd;
            double m = mind[i];
            if (dist < m) { m = dist; mind[i] = m; }
            if (better(m, i, bv, bi)) { bv = m; bi = i; }
        }
        s_v[tid] = bv; s_i[tid] = bi;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if (tid < o && better(s_v[tid + o], s_i[tid + o], s_v[tid], s_i[tid])) { s_v[tid] = s_v[tid + o]; s_i[tid] = s_i[tid + o]; } __syncthreads(); }
        c = s_i[0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void fill_double(double* p, int n, double v) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) p[i] = v;
}

// min_distances against the already-selected centres (kcenterGreedy.py:72-82); also the first partial maxima.  One wave per row, one lane
// per centre (each distance is summed in NumPy's pairwise order by its lane, the minimum over the centres is order-free): a thread per
// row walked the centres one after the other, 0.59 ms for 1400 rows x 240 centres.
__global__ __launch_bounds__(256) void kc_init(const double* __restrict__ f, int n, int D, const int* __restrict__ already, int na, double* mind, Part* pout,
                                               const int* __restrict__ dn = nullptr) {
    __shared__ Part s_p[4];
    if (dn) n = min(n, *dn);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    Part b; b.v = -1.0; b.i = 0x7fffffff;
    for (int i = blockIdx.x * 4 + wid; i < n; i += gridDim.x * 4) {
        const double* fi = f + (size_t)i * D;
        double m = 1.0e300;
        for (int a = lane; a < na; a += 64) {
            const double* fc = f + (size_t)already[a] * D;
            double dist = np_pairwise<double>([&](int k) { const double d = fi[k] - fc[k]; return d * d; }, D);
            m = fmin(m, sqrt(dist));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const long long bits = __double_as_longlong(m);
            const unsigned lo = __shfl_xor((unsigned)bits, o), hi = __shfl_xor((unsigned)(bits >> 32), o);
            m = fmin(m, __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)));
        }
        if (lane == 0) mind[i] = m;
        if (better(m, i, b.v, b.i)) { b.v = m; b.i = i; }
    }
    if (lane == 0) s_p[wid] = b;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) if (better(s_p[w].v, s_p[w].i, b.v, b.i)) b = s_p[w];
        pout[blockIdx.x] = b;
    }
}

// The same for the reference's own round (kcenterGreedy over 20 000 candidates + 4 000 labelled rows seeded with the 4 000: 96 M pairs): kc_init above reads the
// seed's row from L2 for every (row, seed) pair — 24.6 GB through the vector-memory path, ~10 ms.  Here a thread keeps ITS row in registers, the seeds of a slice
// pass through LDS in tiles of 32 (every lane reads the same address: a broadcast), and the slices of the seeds are spread over blockIdx.y and meet in an atomic
// minimum on the bit pattern (non-negative doubles order like their bits).  min over the seeds of sqrt(d) == sqrt(min d), bit for bit (sqrt is monotone and
// correctly rounded), so one root per row is taken afterwards (kc_finish, which also leaves the partial maxima the chain starts from).
constexpr int KT_SEEDS = 32;
__global__ __launch_bounds__(256) void kc_init_tiled(const double* __restrict__ f, int n, const int* __restrict__ already, int na, unsigned long long* mind2, const int* __restrict__ dn) {
    __shared__ double s_seed[KT_SEEDS][32];
    if (dn) n = min(n, *dn);
    const int tid = threadIdx.x, row = blockIdx.x * 256 + tid;
    const int per = (na + (int)gridDim.y - 1) / (int)gridDim.y, a0 = blockIdx.y * per, a1 = min(na, a0 + per);
    double reg[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) reg[k] = row < n ? f[(size_t)row * 32 + k] : 0.0;
    double m = 1.0e300;
    for (int t0 = a0; t0 < a1; t0 += KT_SEEDS) {
        const int cnt = min(KT_SEEDS, a1 - t0);
        __syncthreads();
        for (int e = tid; e < cnt * 32; e += 256) s_seed[e >> 5][e & 31] = f[(size_t)already[t0 + (e >> 5)] * 32 + (e & 31)];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const double dist = np_pairwise_fixed<32>([&](int k) { const double d = reg[k] - s_seed[j][k]; return d * d; });
            m = fmin(m, dist);
        }
    }
    if (row < n && a1 > a0) atomicMin(&mind2[row], (unsigned long long)__double_as_longlong(m));
}
__global__ __launch_bounds__(256) void kc_finish(unsigned long long* mind2, int n, Part* pout, const int* __restrict__ dn) {
    __shared__ Part s_p[4];
    if (dn) n = min(n, *dn);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    double* mind = reinterpret_cast<double*>(mind2);
    double v = -1.0; int i = 0x7fffffff;
    for (int r = blockIdx.x * 256 + tid; r < n; r += gridDim.x * 256) {
        const double mm = sqrt(__longlong_as_double((long long)mind2[r]));
        mind[r] = mm;
        if (better(mm, r, v, i)) { v = mm; i = r; }
    }
    wave_argmax(v, i);
    if (lane == 0) { s_p[wid].v = v; s_p[wid].i = i; }
    __syncthreads();
    if (tid == 0) {
        Part b = s_p[0];
        for (int w = 1; w < 4; ++w) if (better(s_p[w].v, s_p[w].i, b.v, b.i)) b = s_p[w];
        pout[blockIdx.x] = b;
    }
}

#ifndef HIPEMU
// Co-operative chains of DIFFERENT streams share the chip: each is sized against the workgroups that can be resident together, so the sum of the
// grids in flight must stay inside that number too (three selection streams with `--select-lag 2` each launched "half the resident grid": not
// co-resident -> 0.3 s of polling -> abort).  Every cooperative launch leaves an event; a new one first drops the finished ones from the account
// and, while the sum would pass the budget, makes its stream wait for the oldest (device-side: the host never blocks).
struct CoopFlight { hipEvent_t ev; int g; };
static std::mutex g_coop_mu;
static std::vector<CoopFlight> g_coop_flights;
static std::vector<hipEvent_t> g_coop_pool;
// One admission: holds the account's lock from the admit to the recorded event of the launch it admitted (two threads can no longer both pass
// on the same sum), and never takes a chain out of the account before its event reports it finished: a chain that stream A was made to wait for
// still runs, and a stream C admitted right afterwards must see it in the sum (and waits for it as well) — the polling-abort case the account exists for.
struct CoopGuard {
    std::unique_lock<std::mutex> lk;
    int admit(hipStream_t s, int g, int budget) {
        lk = std::unique_lock<std::mutex>(g_coop_mu);
        size_t keep = 0; int sum = 0;
        for (size_t i = 0; i < g_coop_flights.size(); ++i) {
            if (hipEventQuery(g_coop_flights[i].ev) == hipSuccess) { g_coop_pool.push_back(g_coop_flights[i].ev); continue; }      // finished: its event may be re-recorded
            g_coop_flights[keep++] = g_coop_flights[i]; sum += g_coop_flights[i].g;
        }
        g_coop_flights.resize(keep);
        (void)hipGetLastError();          // (hipErrorNotReady of the queries is not an error)
        for (size_t k = 0; k < g_coop_flights.size() && sum + g > budget; ++k) {      // oldest first; the flights stay in the account
            SSDR_HIP(hipStreamWaitEvent(s, g_coop_flights[k].ev, 0));
            sum -= g_coop_flights[k].g;
        }
        return SSDR_OK;
    }
    int launched(hipStream_t s, int g) {
        if (!lk.owns_lock()) lk = std::unique_lock<std::mutex>(g_coop_mu);
        hipEvent_t ev;
        if (!g_coop_pool.empty()) { ev = g_coop_pool.back(); g_coop_pool.pop_back(); }
        else SSDR_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        SSDR_HIP(hipEventRecord(ev, s));
        g_coop_flights.push_back({ev, g});
        lk.unlock();
        return SSDR_OK;
    }
};
#endif

// ---- the launcher: environment, plan, launch -------------------------------------------------------------------------------------------------
// one scratch set per stream: calls on different streams may run concurrently (include/ssdr_al.h).  status: the word the cooperative chains' abort sets
// bit 0 of (ssdr_select_status)
struct FpsState { DevBuf part, mind, vtmp, status; bool status_init = false; };
FpsState& fst(hipStream_t s) { return per_stream<FpsState>(s); }

// The environment switches, read once per process (tests/test_fps_paths.py gives every setting a child process of its own)
struct FpsEnv {
    int force_g;        // SSDR_FPS_COOP_G (tests): fps_coop's grid, launched without the occupancy query: a grid above residency must be reported, not believed
    int budget;         // SSDR_FPS_COOP_BUDGET (tests): a budget of resident workgroups that forces the serialisation of chains on different streams
    int slot_shift;     // SSDR_FPS_SLOT_SHIFT: a coop_split record's slot: 16 bytes, or a line / several of its own (unset: 6)
    int delay;          // SSDR_FPS_DELAY (development): s_sleep units in front of coop_split's first polling pass (unset: -1, chosen by G)
    bool dbg;           // SSDR_FPS_DBG (development): the TIMED coop_split kernel, its phase clocks printed (fps_dbg_report)
    bool kc_tiled;      // SSDR_KC_TILED: 0 keeps kc_init at every size (A/B)
};
const FpsEnv& fps_env() {
    static const FpsEnv env = [] {
        auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
        const char* t = getenv("SSDR_KC_TILED");
        return FpsEnv{num("SSDR_FPS_COOP_G", 0), num("SSDR_FPS_COOP_BUDGET", 0), num("SSDR_FPS_SLOT_SHIFT", 6), num("SSDR_FPS_DELAY", -1), getenv("SSDR_FPS_DBG") != nullptr,
                      !t || t[0] != '0'};
    }();
    return env;
}

// The seedings and the forms, and the names of the zero-work profiler scopes that say which ones a call took (inside "fps_chain";
// tests/test_fps_paths.py reads them; nothing when profiling is off): the tables follow the enums
enum FpsSeed { SEED_FILL, SEED_KC_INIT, SEED_KC_INIT_TILED };
enum FpsForm { FORM_BLOCK_REG1, FORM_BLOCK_REG2, FORM_BLOCK_REG3, FORM_BLOCK0, FORM_BLOCK32, FORM_STEP, FORM_COOP, FORM_COOP_SPLIT2 };
constexpr const char* FPS_SEED_NAME[] = {"fps_seed:fill", "fps_seed:kc_init", "fps_seed:kc_init_tiled"};
constexpr const char* FPS_FORM_NAME[] = {"fps_form:block_reg<1>", "fps_form:block_reg<2>", "fps_form:block_reg<3>", "fps_form:block<0>", "fps_form:block<32>", "fps_form:step",
                                         "fps_form:coop", "fps_form:coop_split<2>"};

struct FpsPlan {
    FpsSeed seed = SEED_FILL; FpsForm form = FORM_STEP;
    int nb = 1;                                  // partial maxima the seeding leaves (kc_init's / kc_finish's grid) and fps_step's grid
    int G = 0, budget = 0;                       // a cooperative form's grid (0: the other forms), admitted by the account against this many resident workgroups
    int slot_shift = 0, delay = 0;               // coop_split: log2 of a record's slot in bytes, s_sleep units in front of the first polling pass
};

// Which seeding and which form a chain over n rows of D features takes (seeded: k-center behind `na` already selected rows).  Launches nothing: its only
// HIP call is the occupancy query that accepts or refuses a cooperative grid.  The CPU logic build has the rows without cooperative kernels.
FpsPlan fps_plan(size_t n, int D, bool seeded, size_t na, int num_cu, const FpsEnv& env) {
    FpsPlan P;
    P.nb = grid_for((long)n, num_cu * 2);
    // seeded single-workgroup paths: kc_init takes a wave per row and its partial maxima are read once — as many workgroups as give every
    // wave a few rows (6 workgroups for 1400 rows left the kernel latency-bound at 0.57 ms)
    if (seeded && n <= 16384) P.nb = std::max(P.nb, (int)std::min<size_t>((n + 15) / 16, 2048));
    // tiled: the reference's own round (rows in registers, seeds through LDS, seed slices over blockIdx.y)
    P.seed = !seeded ? SEED_FILL : (env.kc_tiled && D == 32 && (double)n * (double)na > 4.0e6) ? SEED_KC_INIT_TILED : SEED_KC_INIT;
    auto take = [&P](FpsForm form, int G = 0) { P.form = form; P.G = G; return P; };
    if (D == 32 && n <= 1536) return take(n <= 512 ? FORM_BLOCK_REG1 : n <= 1024 ? FORM_BLOCK_REG2 : FORM_BLOCK_REG3);      // register-resident single workgroup
#ifndef HIPEMU
    // cooperative kernels (G co-resident workgroups that hand their partial maxima to each other once per pick): only above the sizes one workgroup sweeps
    // well (the 160 x 129 / 1000 x 129 k-center shapes keep the 1024-thread fps_block), and only with G workgroups the occupancy query says are resident
    // together — checked, not assumed.  Two forms:
    //  * coop_split<2> for D = 32 while the rows fit the registers of half the CUs at FR_ROWS each (so G = ceil(n / 256) <= num_cu) and one wave sweeps the
    //    G records (G <= 256): 2.47 / 2.49 / 2.56 / 2.61 / 2.73 us per pick at 2368 / 4736 / 9472 / 20000 / 24000 rows (profiles/r06_fps_*.txt);
    //  * coop for every other D and for D = 32 above that, up to FC_NT * FC_PPT rows for each of half the CUs.
    // Up to 256 CUs the first condition of the split form implies the second (512 * 128 = 256 * 256 rows).  On a part with more CUs there are sizes whose
    // rows fit the registers while the records pass one wave's sweep: they take coop like every other size above the split form.
    const size_t half = (size_t)(num_cu / 2);
    const size_t gs = (n + FQ_ROWS - 1) / FQ_ROWS;
    const bool split = D == 32 && n <= (size_t)FR_ROWS * half && gs <= (size_t)FQ_MAXG;       // (n > 1536 here)
    int g = split ? (int)gs : (n > 4096 && n <= (size_t)FC_NT * FC_PPT * half) ? (int)std::min<size_t>(half, (n + 2 * FC_NT - 1) / (2 * FC_NT)) : 0;
    int resident = 0;
    if (g && env.force_g > 0 && !split) g = env.force_g;
    else if (g) {
        int per_cu = 0;
        const hipError_t oe = split ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fps_coop_split<false>, FQ_NT, 0)
                                    : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fps_coop, FC_NT, 0);
        // half of what the query admits: the query is known to answer one block per CU high at some register counts (MI355X_MICROARCH.md), and
        // other chains / stage kernels share the CUs
        resident = (int)((long)per_cu * num_cu / 2);
        if (oe != hipSuccess || resident < g) g = 0;
    }
    if (g) {
        P.budget = env.budget > 0 ? std::max(env.budget, g) : std::max(resident, g);
        if (!split) return take(FORM_COOP, g);
        P.slot_shift = env.slot_shift; P.delay = env.delay >= 0 ? env.delay : (g >= 72 ? 20 : 16);
        return take(FORM_COOP_SPLIT2, g);
    }
#endif
    if (n <= 16384) return take(D == 32 ? FORM_BLOCK32 : FORM_BLOCK0);     // one CU sweeps the candidates faster than a launch per iteration costs
    return take(FORM_STEP);
}

#ifndef HIPEMU
// SSDR_FPS_DBG (development): where a pick's time goes, per workgroup (wave 0's clock).  The TIMED kernel accumulates eight phases into dbg[g][8];
// the chain is waited for and every phase printed per pick
int fps_dbg_begin(hipStream_t s, long long** dbg) {
    static DevBuf buf;
    SSDR_TRY(buf.reserve(8 * 8 * 512)); SSDR_HIP(hipMemsetAsync(buf.p, 0, 8 * 8 * 512, s));
    *dbg = buf.as<long long>();
    return SSDR_OK;
}
int fps_dbg_report(const char* kernel, const char* const (&phase)[8], int G, size_t count, const long long* dbg, hipStream_t s) {
    const int ng = std::min(G, 512);
    SSDR_HIP(hipStreamSynchronize(s));
    std::vector<long long> h(8 * (size_t)ng); SSDR_HIP(hipMemcpy(h.data(), dbg, 8 * h.size(), hipMemcpyDeviceToHost));
    int width = 0;
    for (int k = 0; k < 8; ++k) width = std::max(width, (int)strlen(phase[k]) + 1);
    for (int k = 0; k < 8; ++k) {
        long long mn = 1LL << 62, mx = 0, sum = 0;
        for (int g = 0; g < ng; ++g) { const long long v = h[(size_t)g * 8 + k]; mn = std::min(mn, v); mx = std::max(mx, v); sum += v; }
        fprintf(stderr, "%s G=%d %-*s per pick: mean %.1f min %.1f max %.1f\n", kernel, G, width, phase[k], (double)sum / ng / count, (double)mn / count, (double)mx / count);
    }
    return SSDR_OK;
}
#endif

}  // namespace

int fps_like(const double* d_feat, size_t n, int D, const int32_t* d_already, size_t na, int start, size_t count, int use_sqrt, int32_t* d_out, hipStream_t s, const int* d_n) {
    FpsState& Q = fst(s);
    // SURVEY 8d (F4 / F5): per pick n * D * 8 bytes of features + n * 8 of distances read and written (n = the capacity here: the count is the device's)
    ProfScope prof("fps_chain", s, (double)count * ((double)n * D * 8.0 + 16.0 * (double)n));
    auto took = [s](const char* name) { ProfScope mark(name, s, 0.0); };
    const FpsEnv& env = fps_env();
    const bool seeded = d_already && na;
    const FpsPlan P = fps_plan(n, D, seeded, na, ctx().num_cu, env);
    const int nb = P.nb, fp = seeded ? 1 : 0, G = P.G;
    SSDR_TRY(Q.part.reserve(sizeof(Part) * 2 * (size_t)nb)); SSDR_TRY(Q.mind.reserve(8 * n));
    Part* p0 = Q.part.as<Part>(); Part* p1 = p0 + nb;
    double* mind = Q.mind.as<double>();

    took(FPS_SEED_NAME[P.seed]);
    switch (P.seed) {
    case SEED_KC_INIT_TILED: {
        const int rb = (int)((n + 255) / 256), ys = (int)std::max<size_t>(1, std::min<size_t>((na + KT_SEEDS - 1) / KT_SEEDS, (size_t)std::max(1, 2 * ctx().num_cu / rb)));
        SSDR_HIP(hipMemsetAsync(Q.mind.p, 0x7f, 8 * n, s));                    // 0x7f7f...: a positive double above every squared distance
        hipLaunchKernelGGL(kc_init_tiled, dim3(rb, ys), dim3(256), 0, s, d_feat, (int)n, d_already, (int)na, Q.mind.as<unsigned long long>(), d_n);
        hipLaunchKernelGGL(kc_finish, dim3(nb), dim3(256), 0, s, Q.mind.as<unsigned long long>(), (int)n, p1, d_n);
        SSDR_HIP(hipGetLastError());
        break;
    }
    case SEED_KC_INIT: hipLaunchKernelGGL(kc_init, dim3(nb), dim3(256), 0, s, d_feat, (int)n, D, d_already, (int)na, mind, p1, d_n); break;
    case SEED_FILL: hipLaunchKernelGGL(fill_double, dim3(grid_for((long)n)), dim3(256), 0, s, mind, (int)n, 1.0e10); break;   // fps_gcn_cpu.py:135
    }

#ifndef HIPEMU
    CoopGuard coop;
    if (G) {
        SSDR_TRY(coop.admit(s, G, P.budget));
        if (!Q.status_init) { SSDR_TRY(Q.status.reserve(64)); SSDR_HIP(hipMemsetAsync(Q.status.p, 0, 64, s)); Q.status_init = true; }
    }
    FpsCoopArgs a{d_feat, (int)n, D, fp, start, use_sqrt, p1, nb, mind, (int)count, d_out, nullptr, nullptr, G, Q.status.as<int>(), d_n};
    // a cooperative form's records (recb bytes) with its sync words behind them: the whole of it cleared (tags start at 0: no pick has that number; abort
    // word), or the arrival counters and the abort word alone
    auto scratch = [&](size_t recb, bool whole) -> int {
        SSDR_TRY(Q.vtmp.reserve(recb + 64));
        a.part = Q.vtmp.as<Part>(); a.sync = reinterpret_cast<int*>(Q.vtmp.as<char>() + recb);
        if (whole) SSDR_HIP(hipMemsetAsync(Q.vtmp.p, 0, recb + 64, s));
        else SSDR_HIP(hipMemsetAsync(a.sync, 0, 16, s));
        return SSDR_OK;
    };
    long long* dbg = nullptr;
#endif

    took(FPS_FORM_NAME[P.form]);
    switch (P.form) {
    // (1024 threads — four waves per SIMD issue a float64 instruction every 5.5 cycles, the two of this form every 6.5, tools/micro/valu_rate.hip — with row tid in
    // registers and rows 1024.. in LDS was built and measured: 2.42 against 2.39 ms for the selection stage; the barrier over sixteen waves takes the gain back)
    case FORM_BLOCK_REG1: hipLaunchKernelGGL((fps_block_reg<32, 1, 512>), dim3(1), dim3(512), 0, s, d_feat, (int)n, fp, start, use_sqrt, p1, nb, mind, (int)count, d_out, d_n); break;
    case FORM_BLOCK_REG2: hipLaunchKernelGGL((fps_block_reg<32, 2, 512>), dim3(1), dim3(512), 0, s, d_feat, (int)n, fp, start, use_sqrt, p1, nb, mind, (int)count, d_out, d_n); break;
    case FORM_BLOCK_REG3: hipLaunchKernelGGL((fps_block_reg<32, 3, 512>), dim3(1), dim3(512), 0, s, d_feat, (int)n, fp, start, use_sqrt, p1, nb, mind, (int)count, d_out, d_n); break;
    case FORM_BLOCK32: hipLaunchKernelGGL((fps_block<32>), dim3(1), dim3(1024), 0, s, d_feat, (int)n, D, fp, start, use_sqrt, p1, nb, mind, (int)count, d_out, d_n); break;
    case FORM_BLOCK0: hipLaunchKernelGGL((fps_block<0>), dim3(1), dim3(1024), 0, s, d_feat, (int)n, D, fp, start, use_sqrt, p1, nb, mind, (int)count, d_out, d_n); break;
    case FORM_STEP:
        for (size_t it = 0; it < count; ++it) {
            Part* pin = (it & 1) ? p0 : p1; Part* pout = (it & 1) ? p1 : p0;
            const bool last = it + 1 == count;
            // k-center starts from the arg-max of the seeded distances; FPS from `start`
            hipLaunchKernelGGL(fps_step, dim3(last ? 1 : nb), dim3(256), 0, s, d_feat, (int)n, D, (seeded || it > 0) ? 1 : 0, start, use_sqrt, pin, nb,
                               last ? (Part*)nullptr : pout, mind, d_out + it, d_n);
        }
        break;
#ifndef HIPEMU
    case FORM_COOP:
        SSDR_TRY(scratch(sizeof(Part) * 2 * (size_t)G, false));
        hipLaunchKernelGGL(fps_coop, dim3(G), dim3(FC_NT), 0, s, a);
        break;
    case FORM_COOP_SPLIT2:
        SSDR_TRY(scratch(((size_t)2 * G) << P.slot_shift, true));
        if (env.dbg) SSDR_TRY(fps_dbg_begin(s, &dbg));
        if (dbg) hipLaunchKernelGGL(fps_coop_split<true>, dim3(G), dim3(FQ_NT), 0, s, a, P.slot_shift, P.delay, dbg);
        else hipLaunchKernelGGL(fps_coop_split<false>, dim3(G), dim3(FQ_NT), 0, s, a, P.slot_shift, P.delay, dbg);
        if (dbg) SSDR_TRY(fps_dbg_report("fps_coop_split<2>", {"row fetch", "dist", "wave_argmax", "barrier1", "combine+store", "sweep", "argmax+barrier2", "passes"}, G, count, dbg, s));
        break;
#else
    default: set_error("fps: %s is not in the CPU logic build", FPS_FORM_NAME[P.form]); return SSDR_ERR_INTERNAL;
#endif
    }
    SSDR_HIP(hipGetLastError());
#ifndef HIPEMU
    if (G) return coop.launched(s, G);
#endif
    return SSDR_OK;
}

}  // namespace ssdr

using namespace ssdr;

extern "C" {

/* What the enqueue-only selection calls on `stream` found and could not return: bit 0 = a cooperative FPS / k-center launch was not co-resident (a
 * workgroup waited for one that never arrived): its picks are invalid (-1 from the abort on).  Waits for the stream, clears the word. */
int ssdr_select_status(void* stream, int32_t* out_status) {
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); FpsState& Q = fst(s);
    int st = 0;
    if (Q.status_init) {
        SSDR_HIP(hipMemcpyAsync(&st, Q.status.p, 4, hipMemcpyDeviceToHost, s));
        SSDR_HIP(hipStreamSynchronize(s));
        if (st) SSDR_HIP(hipMemsetAsync(Q.status.p, 0, 4, s));
    } else SSDR_HIP(hipStreamSynchronize(s));
    if (out_status) *out_status = st;
    if (st & 1) { set_error("selection: a cooperative FPS / k-center launch was not co-resident (a workgroup never arrived); its picks are invalid"); return SSDR_ERR_INTERNAL; }
    return SSDR_OK;
}

int ssdr_fps_superpoint_dev(const double* d_centres, const double* d_cd_dir, size_t n, int start, size_t count, int32_t* d_out, void* stream) {
    if (!d_centres || !d_cd_dir || !d_out || start < 0 || (size_t)start >= n || count > n || n > 8192) { set_error("fps_superpoint: bad arguments (n <= 8192)"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (count == 0) return SSDR_OK;
    static bool attr_done = false;       // 8 n bytes of dynamic LDS next to the static arrays: beyond the 64 KiB default from n ~ 7800 on
    if (!attr_done) { SSDR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fps_superpoint), hipFuncAttributeMaxDynamicSharedMemorySize, 8 * 8192)); attr_done = true; }
    hipLaunchKernelGGL(fps_superpoint, dim3(1), dim3(256), 8 * n, pick_stream(stream), d_centres, d_cd_dir, (int)n, start, (int)count, d_out);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_fps_dev(const double* d_feat, size_t n, int feat_dim, int start, size_t count, int32_t* d_out, void* stream) {
    if (!d_feat || !d_out || feat_dim < 1 || start < 0 || (size_t)start >= n || count > n) { set_error("fps: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (count == 0) return SSDR_OK;
    return fps_like(d_feat, n, feat_dim, nullptr, 0, start, count, 0, d_out, pick_stream(stream));
}

int ssdr_kcenter_dev(const double* d_feat, size_t n, int feat_dim, const int32_t* d_already_selected, size_t n_already, size_t count, int32_t* d_out, void* stream) {
    if (!d_feat || !d_out || feat_dim < 1 || !d_already_selected || n_already == 0) { set_error("kcenter: bad arguments (needs a non-empty already_selected)"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (count == 0) return SSDR_OK;
    return fps_like(d_feat, n, feat_dim, d_already_selected, n_already, 0, count, 1, d_out, pick_stream(stream));
}

}
