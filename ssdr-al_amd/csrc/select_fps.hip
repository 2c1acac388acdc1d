// Farthest-point and k-center sampling of the selection stage for gfx950 (F4 farthest_features_sample, S3/fps_gcn_cpu.py:119-147; F5 kCenterGreedy,
// S3/kcenterGreedy.py:60-128; farthest_superpoint_sample, S3/sampler2.py:49-80): the wave arg-max, the chain kernels, the seeding kernels, the account
// of cooperative grids in flight, and the launcher fps_like() behind ssdr_fps_dev, ssdr_kcenter_dev, the one-call chain of select.hip and the sharded
// ssdr_*_gathered_dev entries.
//
// A chain is `count` dependent picks: per pick every row's running minimum distance to the centres picked so far is updated and the row with the
// largest one (the lowest index among equal values, np.argmax) becomes the next centre.  Distances are float64 sums in NumPy's pairwise order
// (np_sum.hpp), so identical inputs give the reference's index sequence.  Up to 1536 rows of 32 features one workgroup holds everything in registers;
// above, G co-resident workgroups run the whole chain in ONE launch and hand their partial maxima to each other once per pick: write-through (sc1)
// stores of self-validating records (data and pick number in one granule), polled with sc1 loads by the readers, no cache write-back / invalidate on
// either side, a bounded wait that ends in an abort word and the stream's status word (ssdr_select_status), never in a wrong selection.  Beyond what
// can be co-resident there is one launch per pick.
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

// FPS / k-center over more candidates than one workgroup sweeps per pick (n > 16384): ONE launch of G co-resident workgroups instead of a
// launch per pick (the reference's AL rounds pick 10 000 of ~2 x 10^4 regions, ssdr_main_S3DIS2.py:134: 10^4 dependent launches).  Every
// workgroup keeps the running min-distance of its points in registers; per pick it publishes its partial arg-max with write-through (sc1)
// stores, drains them, adds to a counter; all workgroups poll that counter and read the G partials with sc1 loads (the fence-free hand-off
// of MI355X_MICROARCH.md, "Valid forms": 9.3 us per pick with __threadfence on both sides, measured), and each reduces them itself.  Partials and counters alternate between two
// sets by the parity of the pick, so a workgroup that runs ahead never overwrites what a slower one still reads.
constexpr int FC_NT = 256, FC_PPT = 8;
struct FpsCoopArgs { const double* f; int n, D, from_partials, start, use_sqrt; const Part* pin; int npart; const double* mind; int count; int* out; Part* part; int* sync; int G; int* status; const int* dn; };
constexpr long FPS_COOP_SPINS = 1L << 22;      // ~0.3 s of polling: a pick among co-resident workgroups takes microseconds
// sync[0], sync[1]: arrival counters by pick parity; sync[2]: abort — a workgroup waited FPS_COOP_SPINS polls for one that never arrived (the launch was
// not co-resident).  It is checked at every pick by every workgroup, which then leaves (the picks from there on read -1), and the stream's selection
// status word takes bit 0: ssdr_select_status turns it into an error.  Without it a non-resident launch returned a wrong selection silently.
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

// The same chain for 32-d features with every workgroup's rows IN REGISTERS (512 per workgroup: one row per thread on eight waves since round 4 — two waves
// per SIMD issue a float64 instruction every 6.5 cycles, the lone wave of the 256-thread form with two rows per thread every 12: 3.21 / 3.64 / 4.51 -> 2.84 / 3.17 /
// 3.46 us per pick at 2368 / 4736 / 9472 rows on an idle GPU; 1024 rows per workgroup on 512 threads: 3.54 / 3.65 / 3.91) and partials that carry the candidate's
// features: a pick costs one publish (the owner's row through LDS, one 272-byte write-through store by 34 lanes, drained, counter) and ONE round of loads
// (every workgroup reads all G partials, features included, into LDS and finds the winner there) instead of three dependent rounds (partials, the winner's
// row from the feature table, every row's features from L2).  This is the replicated global FPS of the sharded run (2 / 4 / 8 ranks: 2368 / 4736 / 9472 rows).
#ifndef HIPEMU
constexpr int FR_NT = 512, FR_RPT = 1, FR_ROWS = FR_NT * FR_RPT, FR_REC = 34;        // record: v, (i, pad), f[32] as 34 doubles
__global__ __launch_bounds__(FR_NT) void fps_coop_reg(FpsCoopArgs a) {
    if (a.dn) a.n = min(a.n, *a.dn);
    extern __shared__ double s_all[];                      // [G][FR_REC]: the partials of a pick, as read
    __shared__ double s_v[FR_NT / 64]; __shared__ int s_i[FR_NT / 64]; __shared__ double s_fc[32]; __shared__ double s_pub[FR_REC];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = blockIdx.x, G = a.G;
    double reg[FR_RPT][32], rmin[FR_RPT];
#pragma unroll
    for (int q = 0; q < FR_RPT; ++q) {
        const long i = (long)g * FR_ROWS + q * FR_NT + tid;
        rmin[q] = i < a.n ? a.mind[i] : -1.0;
#pragma unroll
        for (int k = 0; k < 32; ++k) reg[q][k] = i < a.n ? a.f[(size_t)i * 32 + k] : 0.0;
    }
    auto block_argmax = [&](double v, int i, double& ov, int& oi) {
        wave_argmax(v, i);
        if (lane == 0) { s_v[wid] = v; s_i[wid] = i; }
        __syncthreads();
        ov = s_v[0]; oi = s_i[0];
#pragma unroll
        for (int w = 1; w < FR_NT / 64; ++w) if (better(s_v[w], s_i[w], ov, oi)) { ov = s_v[w]; oi = s_i[w]; }
        __syncthreads();
    };
    int c;
    if (!a.from_partials) c = a.start;
    else {
        double v = -1.0; int i = 0x7fffffff;
        for (int k = tid; k < a.npart; k += FR_NT) if (better(a.pin[k].v, a.pin[k].i, v, i)) { v = a.pin[k].v; i = a.pin[k].i; }
        double ov; block_argmax(v, i, ov, c);
    }
    if (tid < 32) s_fc[tid] = a.f[(size_t)c * 32 + tid];    // the first centre's row comes from the table
    __syncthreads();
    double* recs = reinterpret_cast<double*>(a.part);      // [2][G][FR_REC]
    __shared__ int s_abort;
    for (int it = 0; it < a.count; ++it) {
        if (tid == 0) s_abort = __hip_atomic_load(&a.sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (s_abort) { if (g == 0) for (int k = it + tid; k < a.count; k += FR_NT) a.out[k] = -1; return; }
        if (g == 0 && tid == 0) a.out[it] = c;
        if (it + 1 == a.count) break;
        double bv = -1.0; int bi = 0x7fffffff, bq = 0;
#pragma unroll
        for (int q = 0; q < FR_RPT; ++q) {
            const int i = g * FR_ROWS + q * FR_NT + tid;
            if (i < a.n) {
                double dist = np_pairwise_fixed<32>([&](int k) { const double d = reg[q][k] - s_fc[k]; return d * d; });
                if (a.use_sqrt) dist = sqrt(dist);
                if (dist < rmin[q]) rmin[q] = dist;
                if (better(rmin[q], i, bv, bi)) { bv = rmin[q]; bi = i; bq = q; }
            }
        }
        double wv; int wi;
        block_argmax(bv, bi, wv, wi);
        // the owner of the workgroup's best row lays the record out in LDS ...
        if (wi == bi && bi != 0x7fffffff) {
            s_pub[0] = wv; s_pub[1] = __longlong_as_double((long long)(unsigned)wi);
#pragma unroll
            for (int k = 0; k < 32; ++k) s_pub[2 + k] = bq == 0 ? reg[0][k] : reg[FR_RPT - 1][k];
        } else if (wi == 0x7fffffff && tid == 0) { s_pub[0] = -1.0; s_pub[1] = __longlong_as_double(0x7fffffffll); }      // a workgroup of padding rows only
        __syncthreads();
        const int par = it & 1;
        double* mine = recs + ((size_t)par * G + g) * FR_REC;
        if (tid < 64) {
            // ... and one wave writes it through (sc1), drains, then arrives: no cache write-back / invalidate on either side
            if (tid < FR_REC) __hip_atomic_store(reinterpret_cast<unsigned long long*>(mine + tid), (unsigned long long)__double_as_longlong(s_pub[tid]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (tid == 0) {
                __hip_atomic_fetch_add(&a.sync[par], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int want = G * (it / 2 + 1);
                long spins = 0;
                while (__hip_atomic_load(&a.sync[par], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > FPS_COOP_SPINS || __hip_atomic_load(&a.sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { atomicOr(&a.sync[2], 1); atomicOr(a.status, 1); break; }
                }
            }
        }
        __syncthreads();
        // every partial, features included, in ONE round of loads
        const double* all = recs + (size_t)par * G * FR_REC;
        for (int k = tid; k < G * FR_REC; k += FR_NT)
            s_all[k] = __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(all + k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        __syncthreads();
        double v = -1.0; int i = 0x7fffffff;
        for (int k = tid; k < G; k += FR_NT) {
            const double pv = s_all[(size_t)k * FR_REC]; const int pi = (int)(unsigned)__double_as_longlong(s_all[(size_t)k * FR_REC + 1]);
            if (better(pv, pi, v, i)) { v = pv; i = pi; }
        }
        double ov; block_argmax(v, i, ov, c);
        // the winner's row: the record of the workgroup that owns row c
        const int wg = c / FR_ROWS;
        if (tid < 32) s_fc[tid] = s_all[(size_t)wg * FR_REC + 2 + tid];
        __syncthreads();
    }
}

// The same chain with the hand-off in self-validating granules (MI355X_MICROARCH.md, price list: handoff-1to1 against handoff-flag): a record travels as 68
// 8-byte words {32 bits of data, pick number}, each written by ONE write-through store and polled directly by its reader — no drain, no counter, no second
// round trip.  Records alternate between two sets by the parity of the pick (a workgroup is at most one pick ahead of the slowest), the winner is found by
// every wave for itself out of the LDS copy (no barrier), and the distance loop reads the winner's features straight from that copy.  Four barriers per pick.
constexpr int FT_WORDS = 2 * FR_REC;         // 68 granules per record
__global__ __launch_bounds__(FR_NT) void fps_coop_tag(FpsCoopArgs a) {
    if (a.dn) a.n = min(a.n, *a.dn);
    extern __shared__ unsigned s_rec[];                    // [2][G][FT_WORDS]: the records of a pick, as read (data words)
    __shared__ double s_v[2][FR_NT / 64]; __shared__ int s_i[2][FR_NT / 64]; __shared__ unsigned s_pub[FT_WORDS]; __shared__ int s_abort, s_gave; __shared__ double s_f0[32];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = blockIdx.x, G = a.G;
    if (tid == 0) s_gave = 0;                              // (ordered before its first reader by the barrier behind s_f0 below)
    double reg[FR_RPT][32], rmin[FR_RPT];
#pragma unroll
    for (int q = 0; q < FR_RPT; ++q) {
        const long i = (long)g * FR_ROWS + q * FR_NT + tid;
        rmin[q] = i < a.n ? a.mind[i] : -1.0;
#pragma unroll
        for (int k = 0; k < 32; ++k) reg[q][k] = i < a.n ? a.f[(size_t)i * 32 + k] : 0.0;
    }
    int c;
    if (!a.from_partials) c = a.start;
    else {
        double v = -1.0; int i = 0x7fffffff;
        for (int k = tid; k < a.npart; k += FR_NT) if (better(a.pin[k].v, a.pin[k].i, v, i)) { v = a.pin[k].v; i = a.pin[k].i; }
        wave_argmax(v, i);
        if (lane == 0) { s_v[0][wid] = v; s_i[0][wid] = i; }
        __syncthreads();
        v = s_v[0][0]; c = s_i[0][0];
        for (int w = 1; w < FR_NT / 64; ++w) if (better(s_v[0][w], s_i[0][w], v, c)) { v = s_v[0][w]; c = s_i[0][w]; }
        __syncthreads();
    }
    if (tid < 32) s_f0[tid] = a.f[(size_t)c * 32 + tid];    // the first centre's row comes from the table
    __syncthreads();
    const double* fc = s_f0;
    unsigned long long* recs = reinterpret_cast<unsigned long long*>(a.part);      // [2][G][FT_WORDS]
    for (int it = 0; it < a.count; ++it) {
        if (g == 0 && tid == 0) a.out[it] = c;
        if (it + 1 == a.count) break;
        const int par = it & 1;
        double bv = -1.0; int bi = 0x7fffffff, bq = 0;
#pragma unroll
        for (int q = 0; q < FR_RPT; ++q) {
            const int i = g * FR_ROWS + q * FR_NT + tid;
            if (i < a.n) {
                double dist = np_pairwise_fixed<32>([&](int k) { const double d = reg[q][k] - fc[k]; return d * d; });
                if (a.use_sqrt) dist = sqrt(dist);
                if (dist < rmin[q]) rmin[q] = dist;
                if (better(rmin[q], i, bv, bi)) { bv = rmin[q]; bi = i; bq = q; }
            }
        }
        double wv = bv; int wi = bi;
        wave_argmax(wv, wi);
        if (lane == 0) { s_v[par][wid] = wv; s_i[par][wid] = wi; }
        if (tid == 0) s_abort = __hip_atomic_load(&a.sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();                                   // (1)
        if (s_abort) { if (g == 0) for (int k = it + 1 + tid; k < a.count; k += FR_NT) a.out[k] = -1; return; }
        wv = s_v[par][0]; wi = s_i[par][0];
#pragma unroll
        for (int w = 1; w < FR_NT / 64; ++w) if (better(s_v[par][w], s_i[par][w], wv, wi)) { wv = s_v[par][w]; wi = s_i[par][w]; }
        // the owner of the workgroup's best row lays the record out in LDS ...
        if (wi == bi && bi != 0x7fffffff) {
            double* pub = reinterpret_cast<double*>(s_pub);
            pub[0] = wv; pub[1] = __longlong_as_double((long long)(unsigned)wi);
#pragma unroll
            for (int k = 0; k < 32; ++k) pub[2 + k] = bq == 0 ? reg[0][k] : reg[FR_RPT - 1][k];
        } else if (wi == 0x7fffffff && tid == 0) { double* pub = reinterpret_cast<double*>(s_pub); pub[0] = -1.0; pub[1] = __longlong_as_double(0x7fffffffll); }      // padding rows only
        __syncthreads();                                   // (2)
        // ... and 68 lanes write it through, one self-validating granule each
        const unsigned tag = (unsigned)it + 1u;
        if (tid < FT_WORDS) __hip_atomic_store(recs + ((size_t)par * G + g) * FT_WORDS + tid, ((unsigned long long)tag << 32) | s_pub[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // every record of the pick, polled granule by granule
        unsigned* mine = s_rec + (size_t)par * G * FT_WORDS;
        const unsigned long long* all = recs + (size_t)par * G * FT_WORDS;
        bool gave_up = false;
        for (int k = tid; k < G * FT_WORDS; k += FR_NT) {
            unsigned long long v; long spins = 0;
            while (((v = __hip_atomic_load(all + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 32) != tag) {
                if (++spins > FPS_COOP_SPINS / 16 || (spins % 4096 == 0 && __hip_atomic_load(&a.sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) { gave_up = true; break; }
            }
            if (gave_up) break;                            // (a stale granule is never stored, the remaining records are not waited for)
            mine[k] = (unsigned)v;
        }
        if (gave_up) { atomicOr(&a.sync[2], 1); atomicOr(a.status, 1); s_gave = 1; }      // the others see sync[2] in their own polls / at their next pick
        __syncthreads();                                   // (3)
        if (s_gave) { if (g == 0) for (int k = it + 1 + tid; k < a.count; k += FR_NT) a.out[k] = -1; return; }      // before the winner (an LDS pointer) is formed from garbage
        // the winner: every wave finds it for itself (G <= 128 records, two per lane)
        double v = -1.0; int i = 0x7fffffff;
        for (int k = lane; k < G; k += 64) {
            const double* r = reinterpret_cast<const double*>(mine + (size_t)k * FT_WORDS);
            const double pv = r[0]; const int pi = (int)(unsigned)__double_as_longlong(r[1]);
            if (better(pv, pi, v, i)) { v = pv; i = pi; }
        }
        wave_argmax(v, i);
        c = i;
        fc = reinterpret_cast<const double*>(mine + (size_t)(c / FR_ROWS) * FT_WORDS) + 2;      // the winner's row: the record of the workgroup that owns row c
    }
}

// Round 6: the chain at the reference's own scale (10 000 picks over 20 000 candidates, ssdr_main_S3DIS2.py:134) is all hand-off: 0.5 us of float64
// arithmetic per pick, the rest the all-to-all of the G partials.  Two changes against fps_coop_tag:
//  (1) the SWEEP: a record is 34 slots of 16 bytes, each slot two self-validating 8-byte granules {data, tag}; every thread issues ALL its slot loads
//      (16-byte `sc1` loads) before it looks at a tag and re-reads only the slots that were not there yet — one memory round trip per pass instead of one
//      per granule (the polled form walked ceil(68 G / 512) dependent round trips per pick: 6.3 us at G = 40).  The owner's features go to the record
//      straight from a per-wave LDS image written beside the wave arg-max: two barriers per pick instead of four.
//  (2) the TEAM (team = 1): only workgroups that find themselves on ONE XCD take part — HW_REG_XCC_ID is read, not assumed: the first workgroup to
//      arrive names the XCD, the others of that XCD take tickets for the G row blocks, everybody else leaves at once — so that the records travel
//      through that XCD's own L2 (plain stores keep the line there; `sc1` loads by-pass the reading CU's L1 only) instead of the fabric.  Launched with
//      8 (G + 2) workgroups: placement is the dispatcher's (round-robin over the XCDs as observed, promised nowhere); too few workgroups on the XCD is
//      the same bounded wait -> abort -> status as a launch that was not co-resident, never a wrong selection.
constexpr int FS_SLOTS = FR_REC;             // 16-byte slots per record: words (v lo, v hi), (i, 0), 32 x (f lo, f hi)
constexpr int FS_XCC_ID = ((4 - 1) << 11) | 20;      // s_getreg_b32 hwreg(HW_REG_XCC_ID, 0, 4)
typedef unsigned fs_u4 __attribute__((ext_vector_type(4)));
// TIMED (development, SSDR_FPS_DBG=1): wave 0 of every workgroup accumulates s_memtime between the phases of a pick into dbg[g][8]
template <bool TIMED>
__global__ __launch_bounds__(FR_NT, 4) void fps_coop_sweep(FpsCoopArgs a, int team, int plain_store, long long* dbg) {
    long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = 0;
    auto mark = [&](int k) { if (TIMED) { const long long t = (long long)__builtin_readcyclecounter(); tacc[k] += t - tprev; tprev = t; } };
    if (a.dn) a.n = min(a.n, *a.dn);
    extern __shared__ __attribute__((aligned(16))) unsigned s_rec[];      // [2][G][FT_WORDS] data words of the records of a pick
    __shared__ double s_v[2][FR_NT / 64]; __shared__ int s_i[2][FR_NT / 64]; __shared__ __attribute__((aligned(16))) unsigned s_pubw[FR_NT / 64][FT_WORDS];
    __shared__ int s_g, s_gave; __shared__ double s_f0[32];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, G = a.G;
    if (tid == 0) {
        s_gave = 0;
        int g = blockIdx.x;
        if (team) {
            const int xcc = (int)(__builtin_amdgcn_s_getreg(FS_XCC_ID) & 0xf);
            const int seen = atomicCAS(&a.sync[4], 0, xcc + 1);
            g = (seen == 0 || seen == xcc + 1) ? atomicAdd(&a.sync[5], 1) : G;
        }
        s_g = g;
    }
    __syncthreads();
    const int g = s_g;
    if (g >= G) return;                                     // another XCD's workgroup, or a spare of the team's
    const int row = g * FR_ROWS + tid;
    double reg[32], rmin = row < a.n ? a.mind[row] : -1.0;
#pragma unroll
    for (int k = 0; k < 32; ++k) reg[k] = row < a.n ? a.f[(size_t)row * 32 + k] : 0.0;
    int c;
    if (!a.from_partials) c = a.start;
    else {
        double v = -1.0; int i = 0x7fffffff;
        for (int k = tid; k < a.npart; k += FR_NT) if (better(a.pin[k].v, a.pin[k].i, v, i)) { v = a.pin[k].v; i = a.pin[k].i; }
        wave_argmax(v, i);
        if (lane == 0) { s_v[0][wid] = v; s_i[0][wid] = i; }
        __syncthreads();
        v = s_v[0][0]; c = s_i[0][0];
        for (int w = 1; w < FR_NT / 64; ++w) if (better(s_v[0][w], s_i[0][w], v, c)) { v = s_v[0][w]; c = s_i[0][w]; }
        __syncthreads();
    }
    if (tid < 32) s_f0[tid] = a.f[(size_t)c * 32 + tid];    // the first centre's row comes from the table
    __syncthreads();
    const double* fc = s_f0;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.part, 0, 2 * G * FS_SLOTS * 16, 0x00020000);
    const int total = G * FS_SLOTS;
    for (int it = 0; it < a.count; ++it) {
        if (g == 0 && tid == 0) a.out[it] = c;
        if (it + 1 == a.count) break;
        const int par = it & 1;
        if (TIMED) tprev = (long long)__builtin_readcyclecounter();
        double wv = -1.0; int wi = 0x7fffffff;
        if (row < a.n) {
            double dist = np_pairwise_fixed<32>([&](int k) { const double d = reg[k] - fc[k]; return d * d; });
            if (a.use_sqrt) dist = sqrt(dist);
            if (dist < rmin) rmin = dist;
            wv = rmin; wi = row;
        }
        mark(0);
        wave_argmax(wv, wi);
        mark(1);
        // the wave's best row lays its record out (the workgroup's winner is read from the winning wave's image)
        if (wi == row) {
            double* pub = reinterpret_cast<double*>(s_pubw[wid]);
            pub[0] = wv; pub[1] = __longlong_as_double((long long)(unsigned)wi);
#pragma unroll
            for (int k = 0; k < 32; ++k) pub[2 + k] = reg[k];
        }
        if (lane == 0) { s_v[par][wid] = wv; s_i[par][wid] = wi; }
        mark(2);
        __syncthreads();                                   // (1)
        mark(3);
        const unsigned tag = (unsigned)it + 1u;
        const unsigned base = (unsigned)(par * G) * FS_SLOTS * 16u;
        if (tid < FS_SLOTS) {
            double bv = s_v[par][0]; int bi = s_i[par][0], bw = 0;
#pragma unroll
            for (int w = 1; w < FR_NT / 64; ++w) if (better(s_v[par][w], s_i[par][w], bv, bi)) { bv = s_v[par][w]; bi = s_i[par][w]; bw = w; }
            fs_u4 v;
            if (bi != 0x7fffffff) { v.x = s_pubw[bw][2 * tid]; v.z = s_pubw[bw][2 * tid + 1]; }
            else {          // padding rows only
                const unsigned long long neg1 = (unsigned long long)__double_as_longlong(-1.0);
                v.x = tid == 0 ? (unsigned)neg1 : tid == 1 ? 0x7fffffffu : 0u; v.z = tid == 0 ? (unsigned)(neg1 >> 32) : 0u;
            }
            v.y = tag; v.w = tag;
            const unsigned off = base + (unsigned)(g * FS_SLOTS + tid) * 16u;
            if (plain_store) __builtin_amdgcn_raw_buffer_store_b128(v, rs, off, 0, 0);
            else __builtin_amdgcn_raw_buffer_store_b128(v, rs, off, 0, 16);                          // sc1: write-through
        }
        mark(4);
        // every record of the pick: all of a thread's slots in flight, the missing ones again
        unsigned* mine = s_rec + (size_t)par * G * FT_WORDS;
        bool gave_up = false; int passes = 0;
        for (int k0 = tid; k0 < total && !gave_up; k0 += 4 * FR_NT) {
            unsigned pend = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) if (k0 + j * FR_NT < total) pend |= 1u << j;
            long spins = 0;
            while (pend) {
                fs_u4 v[4];
                if (TIMED) ++passes;
#pragma unroll
                for (int j = 0; j < 4; ++j) if ((pend >> j) & 1u) v[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, base + (unsigned)(k0 + j * FR_NT) * 16u, 0, 16);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (((pend >> j) & 1u) && v[j].y == tag && v[j].w == tag) {
                        *reinterpret_cast<uint2*>(mine + 2 * (size_t)(k0 + j * FR_NT)) = make_uint2(v[j].x, v[j].z);
                        pend &= ~(1u << j);
                    }
                if (pend && (++spins > FPS_COOP_SPINS / 16 || (spins % 1024 == 0 && __hip_atomic_load(&a.sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))) { gave_up = true; break; }
            }
        }
        if (gave_up) { atomicOr(&a.sync[2], 1); atomicOr(a.status, 1); s_gave = 1; }
        mark(5);
        if (TIMED) tacc[7] += passes;
        __syncthreads();                                   // (2)
        mark(6);
        if (s_gave) { if (g == 0) for (int k = it + 1 + tid; k < a.count; k += FR_NT) a.out[k] = -1; return; }
        // the winner: every wave finds it for itself (G <= 64 records, one per lane)
        double v = -1.0; int i = 0x7fffffff;
        if (lane < G) {
            const double* r = reinterpret_cast<const double*>(mine + (size_t)lane * FT_WORDS);
            v = r[0]; i = (int)(unsigned)__double_as_longlong(r[1]);
        }
        wave_argmax(v, i);
        c = i;
        fc = reinterpret_cast<const double*>(mine + (size_t)(c / FR_ROWS) * FT_WORDS) + 2;
        if (TIMED) { const long long t = (long long)__builtin_readcyclecounter(); tacc[6] += t - tprev; tprev = t; }      // (the last arg-max joins slot 6)
    }
    if (TIMED && tid == 0) for (int k = 0; k < 8; ++k) dbg[(size_t)g * 8 + k] = tacc[k];
}
#endif

#ifndef HIPEMU
// Round 6, second form (the phase clocks of fps_coop_sweep, tools/gpu_fps6_dbg.sh: of 4.3 us per pick at 20 000 rows 2.7 are INSIDE the workgroup — 0.73 the
// 95 dependent float64 instructions of a row's distance on a wave that issues one every ~12 cycles, 0.56 the wave arg-max and the owner's 272-byte LDS
// image, 0.43 the skew of two waves per SIMD at the barrier, 0.48 + 0.5 the two combines — and 1.5 the sweep of 40 x 544 bytes):
//  * a ROW IS SPLIT OVER LPR = 2 or 4 LANES: NumPy's eight pairwise accumulators are dealt to the lanes (lane q owns accumulators A q .. A q + A - 1, A = 8 / LPR,
//    i.e. features 8 k + A q + e), each lane adds its accumulators in the reference's order and the tree ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) closes through one
//    or two quad exchanges (a + b == b + a bit for bit): 29 / 50 dependent instructions instead of 95;
//  * a RECORD IS ONE 16-BYTE SLOT: two self-validating 8-byte granules {value half, 16-bit tag | index half} — one lane publishes, ONE wave sweeps all G
//    slots with every load in flight; the winner's ROW is then read from the feature table itself (it is immutable during the chain: plain, cacheable loads,
//    every lane straight into its registers) instead of travelling in every record.  G = n / (512 / LPR) workgroups: 79 / 157 at 20 000 rows.
template <int CTRL> __device__ __forceinline__ double dpp_f64(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = dpp_u32<CTRL>((unsigned)b), hi = dpp_u32<CTRL>((unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
constexpr int FQ_NT = 512;
template <int LPR, bool TIMED>
__global__ __launch_bounds__(FQ_NT) void fps_coop_split(FpsCoopArgs a, int slot_shift, int delay, long long* dbg) {
    static_assert(LPR == 2 || LPR == 4, "lanes per row");
    constexpr int A = 8 / LPR, F = 32 / LPR, ROWS = FQ_NT / LPR, NW = FQ_NT / 64, P = 4;      // 64 P >= G slots per sweeping lane
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
    // measured at seven row counts (tools/gpu_fps_delay.sh, profiles/r06_fps_poll_delay.txt): the best is 16 units up to ~70 workgroups and 20 above (20 000 rows 2.78
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
            double p;
            if (LPR == 4) { p = r[0] + r[1]; p = p + dpp_f64<0xB1>(p); p = p + dpp_f64<0x4E>(p); }
            else { p = (r[0] + r[1]) + (r[A > 2 ? 2 : 0] + r[A > 2 ? 3 : 1]); p = p + dpp_f64<0xB1>(p); }
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

#ifndef HIPEMU
// Third form (round 6; the phase clocks of fps_coop_split: of 3.05 us per pick 0.27 are the barrier in front of the workgroup's combine and 0.47 the combine
// itself — eight (value, index) pairs through LDS and a chain of dependent float64 compares by one wave): EVERY WAVE PUBLISHES ITS OWN 16-byte record, the
// eight records of a workgroup side by side in one 128-byte line, and ONE wave per workgroup sweeps all 8 G of them with every load in flight — the
// workgroup-level combine and its barrier are gone (a sweeper reads the same G lines as before); what is left per pick is the row fetch, 50 dependent
// float64 instructions, one wave arg-max, the hand-off (a write-through store becoming visible + ~1.2 loads' round trip through the fabric, ~1.5 us), one
// wave arg-max over the records and one barrier that hands the winner to the other seven waves.
constexpr int FW_NT = 512, FW_LPR = 2, FW_ROWS = FW_NT / FW_LPR, FW_NW = FW_NT / 64, FW_MAXP = 16;      // at most 64 * 16 / 8 = 128 workgroups = 32768 rows
template <bool TIMED>
__global__ __launch_bounds__(FW_NT) void fps_coop_wave(FpsCoopArgs a, long long* dbg) {
    constexpr int A = 8 / FW_LPR, F = 32 / FW_LPR;
    if (a.dn) a.n = min(a.n, *a.dn);
    long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = 0;
    auto mark = [&](int k) { if (TIMED) { const long long t = (long long)__builtin_readcyclecounter(); tacc[k] += t - tprev; tprev = t; } };
    __shared__ double s_v[FW_NW]; __shared__ int s_i[FW_NW]; __shared__ int s_c[2], s_gave;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = blockIdx.x, G = a.G, q = tid & (FW_LPR - 1);
    const int row = g * FW_ROWS + tid / FW_LPR;
    if (tid == 0) s_gave = 0;
    double x[F], rmin = row < a.n ? a.mind[row] : -1.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < A; ++e) x[k * A + e] = row < a.n ? a.f[(size_t)row * 32 + 8 * k + A * q + e] : 0.0;
    int c;
    if (!a.from_partials) c = a.start;
    else {
        double v = -1.0; int i = 0x7fffffff;
        for (int k = tid; k < a.npart; k += FW_NT) if (better(a.pin[k].v, a.pin[k].i, v, i)) { v = a.pin[k].v; i = a.pin[k].i; }
        wave_argmax(v, i);
        if (lane == 0) { s_v[wid] = v; s_i[wid] = i; }
        __syncthreads();
        v = s_v[0]; c = s_i[0];
        for (int w = 1; w < FW_NW; ++w) if (better(s_v[w], s_i[w], v, c)) { v = s_v[w]; c = s_i[w]; }
    }
    __syncthreads();
    const int total = G * FW_NW;                            // records of a pick: [g][wave], 16 bytes each
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.part, 0, 2 * total * 16, 0x00020000);
    for (int it = 0; it < a.count; ++it) {
        if (g == 0 && tid == 0) a.out[it] = c;
        if (it + 1 == a.count) break;
        const int par = it & 1;
        if (TIMED) tprev = (long long)__builtin_readcyclecounter();
        double fc[F];
        {
            const double* src = a.f + (size_t)c * 32 + A * q;
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int e = 0; e < A; ++e) fc[k * A + e] = src[8 * k + e];
        }
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
            p = p + dpp_f64<0xB1>(p);
            if (a.use_sqrt) p = sqrt(p);
            if (row < a.n) { if (p < rmin) rmin = p; wv = rmin; wi = row; }
        }
        wave_argmax(wv, wi);
        const unsigned tag = ((unsigned)it % 0xffffu + 1u) << 16;
        const unsigned base = (unsigned)(par * total) * 16u;
        if (lane == 0) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(wv);
            fs_u4 v; v.x = (unsigned)b; v.y = tag | ((unsigned)wi >> 16); v.z = (unsigned)(b >> 32); v.w = tag | ((unsigned)wi & 0xffffu);
            __builtin_amdgcn_raw_buffer_store_b128(v, rs, base + (unsigned)(g * FW_NW + wid) * 16u, 0, 16);      // sc1: write-through
        }
        mark(0);
        if (wid == 0) {
            // every record of the pick: all of a lane's slots in flight, the missing ones again
            double v = -1.0; int i = 0x7fffffff; bool gave_up = false; int passes = 0;
            unsigned pend = 0;
#pragma unroll
            for (int j = 0; j < FW_MAXP; ++j) if (lane + j * 64 < total) pend |= 1u << j;
            long spins = 0;
            while (pend) {
                fs_u4 u[FW_MAXP];
                if (TIMED) ++passes;
#pragma unroll
                for (int j = 0; j < FW_MAXP; ++j) if ((pend >> j) & 1u) u[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, base + (unsigned)(lane + j * 64) * 16u, 0, 16);
#pragma unroll
                for (int j = 0; j < FW_MAXP; ++j)
                    if (((pend >> j) & 1u) && (u[j].y & 0xffff0000u) == tag && (u[j].w & 0xffff0000u) == tag) {
                        const double pv = __longlong_as_double((long long)(((unsigned long long)u[j].z << 32) | u[j].x));
                        const int pi = (int)(((u[j].y & 0xffffu) << 16) | (u[j].w & 0xffffu));
                        if (better(pv, pi, v, i)) { v = pv; i = pi; }
                        pend &= ~(1u << j);
                    }
                if (pend && (++spins > FPS_COOP_SPINS / 16 || (spins % 1024 == 0 && __hip_atomic_load(&a.sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))) { gave_up = true; break; }
            }
            if (gave_up) { atomicOr(&a.sync[2], 1); atomicOr(a.status, 1); s_gave = 1; }
            mark(1);
            if (TIMED) tacc[7] += passes;
            wave_argmax(v, i);
            if (lane == 0) s_c[par] = i;
            mark(2);
        }
        __syncthreads();
        mark(3);
        if (s_gave) { if (g == 0) for (int k = it + 1 + tid; k < a.count; k += FW_NT) a.out[k] = -1; return; }
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
    int sweep;          // SSDR_FPS_COOP_SWEEP: the form of the 32-d cooperative chain for A/B runs (unset: -1, the default form; the values are fps_plan's)
    int force_g;        // SSDR_FPS_COOP_G (tests): a grid above residency must be reported, not believed
    int counter;        // SSDR_FPS_COOP_COUNTER: 1 / 0 forces the counter / the granule form of the rounds 3-5 chain (unset: -1, chosen by G)
    int budget;         // SSDR_FPS_COOP_BUDGET (tests): a budget of resident workgroups that forces the serialisation of chains on different streams
    int slot_shift;     // SSDR_FPS_SLOT_SHIFT: a coop_split record's slot: 16 bytes, or a line / several of its own (unset: 6)
    int delay;          // SSDR_FPS_DELAY (development): s_sleep units in front of coop_split's first polling pass (unset: -1, chosen by G)
    bool dbg;           // SSDR_FPS_DBG (development): the TIMED kernels, their phase clocks printed (fps_dbg_report)
    bool kc_tiled;      // SSDR_KC_TILED: 0 keeps kc_init at every size (A/B)
};
const FpsEnv& fps_env() {
    static const FpsEnv env = [] {
        auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
        const char* c = getenv("SSDR_FPS_COOP_COUNTER"); const char* t = getenv("SSDR_KC_TILED");
        return FpsEnv{num("SSDR_FPS_COOP_SWEEP", -1), num("SSDR_FPS_COOP_G", 0), c ? (c[0] == '1' ? 1 : 0) : -1, num("SSDR_FPS_COOP_BUDGET", 0),
                      num("SSDR_FPS_SLOT_SHIFT", 6), num("SSDR_FPS_DELAY", -1), getenv("SSDR_FPS_DBG") != nullptr, !t || t[0] != '0'};
    }();
    return env;
}

// The seedings and the forms, and the names of the zero-work profiler scopes that say which ones a call took (inside "fps_chain";
// tests/test_fps_paths.py reads them; nothing when profiling is off): the tables follow the enums
enum FpsSeed { SEED_FILL, SEED_KC_INIT, SEED_KC_INIT_TILED };
enum FpsForm { FORM_BLOCK_REG1, FORM_BLOCK_REG2, FORM_BLOCK_REG3, FORM_BLOCK0, FORM_BLOCK32, FORM_STEP, FORM_COOP, FORM_COOP_SPLIT2, FORM_COOP_SPLIT4,
               FORM_COOP_WAVE, FORM_COOP_SWEEP_M1, FORM_COOP_SWEEP_M2, FORM_COOP_SWEEP_M3, FORM_COOP_TAG, FORM_COOP_REG };
constexpr const char* FPS_SEED_NAME[] = {"fps_seed:fill", "fps_seed:kc_init", "fps_seed:kc_init_tiled"};
constexpr const char* FPS_FORM_NAME[] = {"fps_form:block_reg<1>", "fps_form:block_reg<2>", "fps_form:block_reg<3>", "fps_form:block<0>", "fps_form:block<32>", "fps_form:step",
                                         "fps_form:coop", "fps_form:coop_split<2>", "fps_form:coop_split<4>", "fps_form:coop_wave", "fps_form:coop_sweep_m1",
                                         "fps_form:coop_sweep_m2", "fps_form:coop_sweep_m3", "fps_form:coop_tag", "fps_form:coop_reg"};

struct FpsPlan {
    FpsSeed seed = SEED_FILL; FpsForm form = FORM_STEP;
    int nb = 1;                                  // partial maxima the seeding leaves (kc_init's / kc_finish's grid) and fps_step's grid
    int G = 0;                                   // workgroups of a cooperative form's launch
    int coop_g = 0, budget = 0;                  // the grid the occupancy query was asked for and the account admits, against this many resident workgroups
                                                 // (coop_g == G but for coop_wave, whose workgroups take 256 rows where the query's kernel takes 512)
    int lpr = 0, slot_shift = 0, delay = 0;      // coop_split: lanes per row, log2 of a record's slot in bytes, s_sleep units in front of the first polling pass
    int team = 0, plain_store = 0;               // coop_sweep: only one XCD's workgroups take part; plain instead of write-through stores
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
    // cooperative kernels (G workgroups that meet at a counter per pick): only above the sizes one workgroup sweeps well (the 160 x 129 / 1000 x 129
    // k-center shapes keep the 1024-thread fps_block), and only with G workgroups the occupancy query says are resident together — checked, not assumed
    // The form of the 32-d chain (round 6; us per pick at 2368 / 4736 / 9472 / 20000 / 24000 rows on one box, profiles/r06_fps_*.txt): rounds 3-5 (polled granules up to 24
    // workgroups, drained record + counter above) 2.85 / 3.21 / 3.68 / 5.22 / 5.36; rows split over two lanes with 16-byte records (fps_coop_split<2>) 2.47 / 2.49 / 2.56 /
    // 2.61 / 2.73 — the default.  SSDR_FPS_COOP_SWEEP selects the others for A/B runs: 0 rounds 3-5, 1 swept 544-byte records, 2 / 3 the same among one XCD's workgroups
    // (plain / write-through stores), 5 rows over four lanes, 6 a record per wave.
    const int sweep = env.sweep >= 0 ? env.sweep : 4;
    const int lpr = sweep == 4 ? 2 : sweep == 5 ? 4 : 0;
    const size_t half = (size_t)(num_cu / 2);
    const bool reg = D == 32 && n <= (size_t)FR_ROWS * half;       // rows in registers (n > 1536 here)
    const bool split = reg && lpr && (n + FQ_NT / lpr - 1) / (FQ_NT / lpr) <= 256;      // (a sweeping lane takes four slots)
    int g = split ? (int)((n + FQ_NT / lpr - 1) / (FQ_NT / lpr)) : reg ? (int)((n + FR_ROWS - 1) / FR_ROWS)
          : (n > 4096 && n <= (size_t)FC_NT * FC_PPT * half) ? (int)std::min<size_t>(half, (n + 2 * FC_NT - 1) / (2 * FC_NT)) : 0;
    int resident = 0;
    if (g && env.force_g > 0 && !split) g = env.force_g;
    else if (g) {
        int per_cu = 0;
        const hipError_t oe = split ? (lpr == 2 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fps_coop_split<2, false>, FQ_NT, 0)
                                                : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fps_coop_split<4, false>, FQ_NT, 0))
                            : reg ? (g > 24 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fps_coop_reg, FR_NT, 8 * (size_t)g * FR_REC)
                                            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fps_coop_tag, FR_NT, 4 * 2 * (size_t)g * FT_WORDS))
                                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fps_coop, FC_NT, 0);
        // half of what the query admits: the query is known to answer one block per CU high at some register counts (MI355X_MICROARCH.md), and
        // other chains / stage kernels share the CUs
        resident = (int)((long)per_cu * num_cu / 2);
        if (oe != hipSuccess || resident < g) g = 0;
    }
    if (g) {
        P.coop_g = g;
        P.budget = env.budget > 0 ? std::max(env.budget, g) : std::max(resident, g);
        if (!reg) return take(FORM_COOP, g);          // one launch: co-resident workgroups meeting at a counter per pick
        if (sweep == 6 && (n + FW_ROWS - 1) / FW_ROWS <= 64 * FW_MAXP / FW_NW) return take(FORM_COOP_WAVE, (int)((n + FW_ROWS - 1) / FW_ROWS));      // a record per wave
        if (split) {          // rows split over 2 / 4 lanes, 16-byte records, the winner's row from the table
            P.lpr = lpr; P.slot_shift = env.slot_shift; P.delay = env.delay >= 0 ? env.delay : (g >= 72 ? 20 : 16);
            return take(lpr == 2 ? FORM_COOP_SPLIT2 : FORM_COOP_SPLIT4, g);
        }
        if (sweep >= 1 && sweep <= 3 && g <= 64) {          // the swept 544-byte records (A/B runs)
            P.team = sweep >= 2; P.plain_store = sweep == 2;
            return take(sweep == 1 ? FORM_COOP_SWEEP_M1 : sweep == 2 ? FORM_COOP_SWEEP_M2 : FORM_COOP_SWEEP_M3, g);
        }
        // rows in registers, partials that carry the candidate's features
        // two hand-off forms, measured (tools/gpu_fps.sh, us per pick at 2368 / 4736 / 9472 / 20000 rows): self-validating granules 3.46 / 3.92 / 4.71 / 6.30,
        // drained record + counter 3.90 / 4.14 / 4.77 / 5.74 — the granule form polls 68 words per record and loses from ~24 workgroups on
        return take((env.counter >= 0 ? env.counter == 1 : g > 24) ? FORM_COOP_REG : FORM_COOP_TAG, g);
    }
#endif
    if (n <= 16384) return take(D == 32 ? FORM_BLOCK32 : FORM_BLOCK0);     // one CU sweeps the candidates faster than a launch per iteration costs
    return take(FORM_STEP);
}

#ifndef HIPEMU
// SSDR_FPS_DBG (development): where a pick's time goes, per workgroup (wave 0's clock).  The TIMED kernels accumulate eight phases into dbg[g][8];
// the chain is waited for and every phase printed per pick (`ticks`: the unit, named by fps_coop_sweep's lines only)
int fps_dbg_begin(hipStream_t s, long long** dbg) {
    static DevBuf buf;
    SSDR_TRY(buf.reserve(8 * 8 * 512)); SSDR_HIP(hipMemsetAsync(buf.p, 0, 8 * 8 * 512, s));
    *dbg = buf.as<long long>();
    return SSDR_OK;
}
int fps_dbg_report(const char* kernel, const char* const (&phase)[8], int G, size_t count, const char* ticks, const long long* dbg, hipStream_t s) {
    const int ng = std::min(G, 512);
    SSDR_HIP(hipStreamSynchronize(s));
    std::vector<long long> h(8 * (size_t)ng); SSDR_HIP(hipMemcpy(h.data(), dbg, 8 * h.size(), hipMemcpyDeviceToHost));
    int width = 0;
    for (int k = 0; k < 8; ++k) width = std::max(width, (int)strlen(phase[k]) + 1);
    for (int k = 0; k < 8; ++k) {
        long long mn = 1LL << 62, mx = 0, sum = 0;
        for (int g = 0; g < ng; ++g) { const long long v = h[(size_t)g * 8 + k]; mn = std::min(mn, v); mx = std::max(mx, v); sum += v; }
        char unit[32] = "";
        if (ticks) snprintf(unit, sizeof(unit), " (%s)", k == 7 ? "passes" : ticks);
        fprintf(stderr, "%s G=%d %-*s per pick: mean %.1f min %.1f max %.1f%s\n", kernel, G, width, phase[k], (double)sum / ng / count, (double)mn / count, (double)mx / count, unit);
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
    if (P.coop_g) {
        SSDR_TRY(coop.admit(s, P.coop_g, P.budget));
        if (!Q.status_init) { SSDR_TRY(Q.status.reserve(64)); SSDR_HIP(hipMemsetAsync(Q.status.p, 0, 64, s)); Q.status_init = true; }
        // fps_coop_reg / fps_coop_tag keep the G records of a pick in a table of 128 in LDS (every form decided behind them is refused with them)
        if (P.form >= FORM_COOP_WAVE && P.form <= FORM_COOP_REG && P.coop_g > 128) { set_error("fps: %d cooperative workgroups exceed the record table of the kernel (128)", P.coop_g); return SSDR_ERR_INVALID; }
    }
    FpsCoopArgs a{d_feat, (int)n, D, fp, start, use_sqrt, p1, nb, mind, (int)count, d_out, nullptr, nullptr, G, Q.status.as<int>(), d_n};
    // a cooperative form's records (recb bytes) with its sync words behind them: the whole of it cleared (tags start at 0: no pick has that number; abort
    // word, team words), or the arrival counters and the abort word alone
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
    case FORM_COOP_SPLIT2: case FORM_COOP_SPLIT4: {
        SSDR_TRY(scratch(((size_t)2 * G) << P.slot_shift, true));
        if (env.dbg) SSDR_TRY(fps_dbg_begin(s, &dbg));
        if (P.lpr == 2 && dbg) hipLaunchKernelGGL((fps_coop_split<2, true>), dim3(G), dim3(FQ_NT), 0, s, a, P.slot_shift, P.delay, dbg);
        else if (P.lpr == 2) hipLaunchKernelGGL((fps_coop_split<2, false>), dim3(G), dim3(FQ_NT), 0, s, a, P.slot_shift, P.delay, dbg);
        else if (dbg) hipLaunchKernelGGL((fps_coop_split<4, true>), dim3(G), dim3(FQ_NT), 0, s, a, P.slot_shift, P.delay, dbg);
        else hipLaunchKernelGGL((fps_coop_split<4, false>), dim3(G), dim3(FQ_NT), 0, s, a, P.slot_shift, P.delay, dbg);
        if (dbg) SSDR_TRY(fps_dbg_report(P.lpr == 2 ? "fps_coop_split<2>" : "fps_coop_split<4>", {"row fetch", "dist", "wave_argmax", "barrier1", "combine+store", "sweep", "argmax+barrier2", "passes"},
                                         G, count, nullptr, dbg, s));
        break;
    }
    case FORM_COOP_WAVE:          // one sweeping wave per workgroup
        SSDR_TRY(scratch((size_t)2 * G * FW_NW * 16, true));
        if (env.dbg) SSDR_TRY(fps_dbg_begin(s, &dbg));
        if (dbg) hipLaunchKernelGGL(fps_coop_wave<true>, dim3(G), dim3(FW_NT), 0, s, a, dbg);
        else hipLaunchKernelGGL(fps_coop_wave<false>, dim3(G), dim3(FW_NT), 0, s, a, dbg);
        if (dbg) SSDR_TRY(fps_dbg_report("fps_coop_wave", {"fetch+dist+argmax+store", "sweep", "argmax", "barrier", "-", "-", "-", "passes"}, G, count, nullptr, dbg, s));
        break;
    case FORM_COOP_SWEEP_M1: case FORM_COOP_SWEEP_M2: case FORM_COOP_SWEEP_M3: {
        SSDR_TRY(scratch(16 * 2 * (size_t)G * FS_SLOTS, true));
        static std::once_flag once;
        std::call_once(once, [] {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fps_coop_sweep<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 2 * FT_WORDS * 64);
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fps_coop_sweep<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 2 * FT_WORDS * 64); });
        const dim3 grid(P.team ? 8 * (G + 2) : G);
        if (env.dbg) SSDR_TRY(fps_dbg_begin(s, &dbg));
        if (dbg) hipLaunchKernelGGL(fps_coop_sweep<true>, grid, dim3(FR_NT), 4 * 2 * (size_t)G * FT_WORDS, s, a, P.team, P.plain_store, dbg);
        else hipLaunchKernelGGL(fps_coop_sweep<false>, grid, dim3(FR_NT), 4 * 2 * (size_t)G * FT_WORDS, s, a, P.team, P.plain_store, dbg);
        if (dbg) SSDR_TRY(fps_dbg_report("fps_coop_sweep", {"dist", "wave_argmax", "pub", "barrier1", "store", "sweep", "barrier2+argmax", "passes"}, G, count, "s_memtime ticks", dbg, s));
        break;
    }
    case FORM_COOP_TAG: {          // (the granule form: 68 words of 8 bytes per record)
        const size_t recb = 8 * 2 * (size_t)G * FR_REC * 2;
        SSDR_TRY(scratch(recb, false));
        SSDR_HIP(hipMemsetAsync(a.part, 0, recb, s));      // tags start at 0: no pick has that number
        static std::once_flag once;
        std::call_once(once, [] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fps_coop_tag), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 2 * FT_WORDS * 128); });
        hipLaunchKernelGGL(fps_coop_tag, dim3(G), dim3(FR_NT), 4 * 2 * (size_t)G * FT_WORDS, s, a);
        break;
    }
    case FORM_COOP_REG: {
        SSDR_TRY(scratch(8 * 2 * (size_t)G * FR_REC * 2, false));
        static std::once_flag once;
        std::call_once(once, [] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fps_coop_reg), hipFuncAttributeMaxDynamicSharedMemorySize, 8 * FR_REC * 128); });
        hipLaunchKernelGGL(fps_coop_reg, dim3(G), dim3(FR_NT), 8 * (size_t)G * FR_REC, s, a);
        break;
    }
#else
    default: set_error("fps: %s is not in the CPU logic build", FPS_FORM_NAME[P.form]); return SSDR_ERR_INTERNAL;
#endif
    }
    SSDR_HIP(hipGetLastError());
#ifndef HIPEMU
    if (P.coop_g) return coop.launched(s, G);
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
