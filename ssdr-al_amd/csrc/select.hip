// Selection stage of one active-learning round for gfx950: per-point uncertainty, per-superpoint statistics,
// candidate features, chamfer / adjacency / feature propagation per cloud, the candidate rule and the one-call chains.  The chamfer distance kernels
// are select_chamfer.hip, the farthest-point / k-center chains the one-call chains end in select_fps.hip, the other region selectors select_region.hip.
//
// Reference (S3 = /root/reference/SSDR_AL_s3dis/): S3/sampler2.py:12-47,102-115,262-266,313-342,612-640;
// S3/fps_gcn_cpu.py:12-178; S3/kcenterGreedy.py:60-128.  The reference does all of this in NumPy / sklearn on
// the host, in float64 for everything after the network.  The kernels keep float64 there and, where a NumPy
// reduction decides a discrete outcome (the arg-max chain of FPS), reproduce NumPy's pairwise summation order
// (np_pairwise, np_sum.hpp) so that identical inputs give the identical index sequence.
//
// Superpoints are CSR: sp_off[S+1] into sp_pts[T] (point ids), the same information as the reference's
// pickled `components` object array (S3/partition/compute_superpoint.py:63-68).
#include <optional>
#include "ssdr_internal.hpp"
#include <map>
#include "block_prims.hpp"
#include "np_sum.hpp"
#include "select_chamfer.hpp"
#include "select_fps.hpp"
#include "select_region.hpp"
#include "select_gcn.hpp"

namespace ssdr {
namespace {

// ---- U1: compute_point_uncertainty (sampler2.py:28-47) + argmax class (:602) ------------------------------
// (round 4: a workgroup's 256 rows of C <= 32 probabilities are one contiguous run: loaded coalesced into LDS, read back one row per lane — a lane reading its
// own 52-byte row straight from memory made every load instruction touch 64 lines)
__global__ __launch_bounds__(256) void sel_point_unc(const float* __restrict__ prob, int n, int C, int mode, float* unc, int* cls) {
    __shared__ float s_p[256 * 32];
    for (int i0 = blockIdx.x * 256; i0 < n; i0 += gridDim.x * 256) {          // uniform over the workgroup
        const int rows = min(256, n - i0);
        const bool staged = C <= 32;
        if (staged) {
            __syncthreads();
            const float* src = prob + (size_t)i0 * C;
            for (int e = threadIdx.x; e < rows * C; e += 256) s_p[e] = src[e];
            __syncthreads();
        }
        const int i = i0 + (int)threadIdx.x;
        if (i >= n) continue;
        const float* p = staged ? s_p + (size_t)threadIdx.x * C : prob + (size_t)i * C;
        float best = p[0], second = -1.f; int bi = 0;
        for (int c = 1; c < C; ++c) {
            const float v = p[c];
            if (v > best) { second = best; best = v; bi = c; }
            else if (v > second) second = v;
        }
        float u;
        if (mode == 0) u = 1.0f - best;                              // lc
        else if (mode == 2) u = second / best;                       // sb: sorted[-2] / sorted[-1]
        else {                                                       // entropy, float32 like np.sum over 13 classes
            u = -1.f * np_pairwise<float>([&](int c) { const float v = p[c]; const float k = log2f(v); return v * (__builtin_isinf(k) ? 0.f : k); }, C);
        }
        unc[i] = u; cls[i] = bi;
    }
}

// ---- U2: per-superpoint loop of TSampler.prediction (sampler2.py:612-626) ---------------------------------
// mode 0 mean, 1 sum_weight, 2 WetSU.  One lane per superpoint (sums must follow NumPy's order).
__global__ __launch_bounds__(256) void sel_region_stats(const float* __restrict__ unc, const int* __restrict__ cls,
                                                        const int* __restrict__ sp_off, const int* __restrict__ sp_pts, int S, int C, int mode,
                                                        double* region_unc, int* dom, int* dom_cnt) {
    for (int s = blockIdx.x * 256 + threadIdx.x; s < S; s += gridDim.x * 256) {
        const int lo = sp_off[s], n = sp_off[s + 1] - lo;
        if (n <= 0) { region_unc[s] = 0.0; dom[s] = 0; dom_cnt[s] = 0; continue; }
        int h[32];
        for (int c = 0; c < 32; ++c) h[c] = 0;
        for (int j = 0; j < n; ++j) { const int c = cls[sp_pts[lo + j]]; if (c >= 0 && c < 32) h[c]++; }
        int d = 0;
        for (int c = 1; c < C; ++c) if (h[c] > h[d]) d = c;           // np.argmax: first maximum
        dom[s] = d; dom_cnt[s] = h[d];
        double r;
        if (mode == 0) {
            const float sum = np_pairwise<float>([&](int j) { return unc[sp_pts[lo + j]]; }, n);
            r = (double)(float)((double)(sum + 0.f) / (double)n);          // identity + pairwise: see sel_region_stats_w
        } else if (mode == 1) {                                      // weights_percentage (:92-100) * uncertainty
            r = np_pairwise<double>([&](int j) { const int p = sp_pts[lo + j]; return ((double)h[cls[p]] / (double)n) * (double)unc[p]; }, n);
            r = r + 0.0;
        } else {                                                     // WetSU (:19-26)
            const double a = np_pairwise<double>([&](int j) { const int p = sp_pts[lo + j]; return (double)unc[p] * (cls[p] == d ? 1.0 : 0.0); }, n);
            const double b = np_pairwise<double>([&](int j) { const int p = sp_pts[lo + j]; return (double)unc[p] * (1.0 - (cls[p] == d ? 1.0 : 0.0)); }, n);
            r = (a + 0.0) - (b + 0.0);
        }
        region_unc[s] = r;
    }
}

// Wave-per-superpoint form of the same loop.  The one-lane form chased sp_pts -> (class, uncertainty) three times per member with 8 k lanes
// on the whole chip (0.37 ms at 1 % of the HBM rate).  Here the 64 lanes of a wave fetch the members' classes and uncertainties together
// into LDS (RS_CAP members per wave; a larger superpoint takes the one-lane routine), count the class histogram there, and lane 0 then runs
// the SAME summation routines (NumPy's pairwise order) over the staged values: same operations in the same order, same result.
constexpr int RS_CAP = 1024, NP_BUFSIZE = 8192;
__global__ __launch_bounds__(256) void sel_region_stats_w(const float* __restrict__ unc, const int* __restrict__ cls,
                                                          const int* __restrict__ sp_off, const int* __restrict__ sp_pts, int S, int C, int mode,
                                                          double* region_unc, int* dom, int* dom_cnt) {
    __shared__ float s_u[4][RS_CAP];
    __shared__ int s_c[4][RS_CAP];
    __shared__ int s_h[4][32];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int s = blockIdx.x * 4 + w; s < S; s += gridDim.x * 4) {
        const int lo = sp_off[s], n = sp_off[s + 1] - lo;
        if (n <= 0) { if (lane == 0) { region_unc[s] = 0.0; dom[s] = 0; dom_cnt[s] = 0; } continue; }
        if (lane < 32) s_h[w][lane] = 0;
        wave_sync();
        const bool staged = n <= RS_CAP;
        // (a wave runs in lockstep on the hardware; the block-level barrier is not available here because waves take different trip counts)
        for (int j = lane; j < n; j += 64) {
            const int p = sp_pts[lo + j];
            const int c = cls[p];
            if (staged) { s_c[w][j] = c; s_u[w][j] = unc[p]; }
            if (c >= 0 && c < 32) atomicAdd(&s_h[w][c], 1);
        }
        wave_sync();
        const int* h = s_h[w];
        int d = 0;
        for (int c = 1; c < C; ++c) if (h[c] > h[d]) d = c;           // np.argmax: first maximum (every lane: uniform)
        if (lane == 0) { dom[s] = d; dom_cnt[s] = h[d]; }
        auto U = [&](int j) { return staged ? s_u[w][j] : unc[sp_pts[lo + j]]; };
        auto K = [&](int j) { return staged ? s_c[w][j] : cls[sp_pts[lo + j]]; };
        const bool w8 = staged && n >= 8;                             // the blocks of NumPy's pairwise sum with their eight accumulators on eight lanes
        double r = 0.0;
        if (!staged) {
            // more members than the wave stages at once (a floor or a wall of a real partition: thousands of points; until round 6 lane 0 chased them one
            // dependent load at a time — 1.8 ms for a 3 600-point region, tools/sp_probe.py): the recursion's nodes of at most RS_CAP terms are staged one
            // after the other by all lanes and summed as above
            // ... and NumPy's reduction hands its inner loop at most NP_BUFSIZE = 8192 elements at a time (the ufunc buffer, whatever the dtype): a sum over more
            // terms is pairwise(first 8192) + pairwise(next 8192) + ..., accumulated left to right — not one recursion over everything (measured against np.sum
            // for 4 099 .. 40 000 terms: the chunked order 20 / 20, the single recursion 11-17 / 20; found when this path met a 8 193-point region)
            int base = 0;
            auto stage = [&](int l0, int cnt) {
                wave_sync();                                      // the previous node's reads are done
                for (int j = lane; j < cnt; j += 64) { const int p = sp_pts[lo + base + l0 + j]; s_c[w][j] = cls[p]; s_u[w][j] = unc[p]; }
                wave_sync();
            };
            float fa = 0.f; double da = 0.0, db = 0.0;
            for (; base < n; base += NP_BUFSIZE) {
                const int cn = min(NP_BUFSIZE, n - base);
                if (mode == 0) {
                    float sa = 0.f, sb = 0.f;
                    np_pairwise_wave_chunked2<float>(stage, [&](int j) { return s_u[w][j]; }, [&](int j) { return s_u[w][j]; }, false, cn, lane, RS_CAP, sa, sb);
                    fa = base == 0 ? sa : fa + sa;
                } else if (mode == 1) {
                    double sa = 0.0, sb = 0.0;
                    auto term = [&](int j) { return ((double)h[s_c[w][j]] / (double)n) * (double)s_u[w][j]; };
                    np_pairwise_wave_chunked2<double>(stage, term, term, false, cn, lane, RS_CAP, sa, sb);
                    da = base == 0 ? sa : da + sa;
                } else {
                    double sa = 0.0, sb = 0.0;
                    np_pairwise_wave_chunked2<double>(stage, [&](int j) { return (double)s_u[w][j] * (s_c[w][j] == d ? 1.0 : 0.0); },
                                                      [&](int j) { return (double)s_u[w][j] * (1.0 - (s_c[w][j] == d ? 1.0 : 0.0)); }, true, cn, lane, RS_CAP, sa, sb);
                    da = base == 0 ? sa : da + sa; db = base == 0 ? sb : db + sb;
                }
            }
            r = mode == 0 ? (double)(float)((double)(fa + 0.f) / (double)n) : mode == 1 ? da + 0.0 : (da + 0.0) - (db + 0.0);      // + 0: see below
        } else if (mode == 0) {
            // np.sum / np.mean are identity + pairwise(...): the finished sum plus T(0).  It changes one value, a sum of -0.0 terms alone (the entropy of one-hot
            // rows), which the eight accumulators started from the first terms leave at -0.0 and NumPy returns as +0.0
            float sum = 0.f;
            if (w8) sum = np_pairwise_wave<float>([&](int j) { return U(j); }, n, lane);
            else if (lane == 0) sum = np_pairwise<float>([&](int j) { return U(j); }, n);
            r = (double)(float)((double)(sum + 0.f) / (double)n);
        } else if (mode == 1) {                                      // weights_percentage (:92-100) * uncertainty
            auto term = [&](int j) { return ((double)h[K(j)] / (double)n) * (double)U(j); };
            if (w8) r = np_pairwise_wave<double>(term, n, lane);
            else if (lane == 0) r = np_pairwise<double>(term, n);
            r = r + 0.0;
        } else {                                                     // WetSU (:19-26)
            auto ta = [&](int j) { return (double)U(j) * (K(j) == d ? 1.0 : 0.0); };
            auto tb = [&](int j) { return (double)U(j) * (1.0 - (K(j) == d ? 1.0 : 0.0)); };
            double a = 0.0, b = 0.0;
            if (w8) { a = np_pairwise_wave<double>(ta, n, lane); b = np_pairwise_wave<double>(tb, n, lane); }
            else if (lane == 0) { a = np_pairwise<double>(ta, n); b = np_pairwise<double>(tb, n); }
            r = (a + 0.0) - (b + 0.0);
        }
        if (lane == 0) region_unc[s] = r;
        wave_sync();
    }
}

// ---- D1: dominant ground-truth label + purity (sampler2.py:102-106 via oracle_labeling :127-144) ------------
// One WAVE per superpoint (a lane per superpoint walked its ~185 members one dependent load at a time with a 64-entry private histogram: 0.18 ms
// for the bench's 7000 regions, more than the whole scoring stage): members dealt to the lanes, histogram in LDS, first maximum like np.argmax.
__global__ __launch_bounds__(256) void sel_dominant_label(const int* __restrict__ labels, const int* __restrict__ sp_off, const int* __restrict__ sp_pts,
                                                          int S, int num_labels, int* out_label, double* out_purity, int* status) {
    __shared__ int s_h[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nl = min(num_labels, 64);
    for (int s = blockIdx.x * 4 + w; s < S; s += gridDim.x * 4) {
        const int lo = sp_off[s], n = sp_off[s + 1] - lo;
        s_h[w][lane] = 0;
        wave_sync();
        bool bad = false;
        for (int j0 = lane; j0 < n; j0 += 256) {          // four members' dependent loads (member, label) in flight per lane
            int p[4], c[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) p[u] = sp_pts[lo + min(j0 + 64 * u, n - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u) c[u] = labels[p[u]];
#pragma unroll
            for (int u = 0; u < 4; ++u) if (j0 + 64 * u < n) { if (c[u] >= 0 && c[u] < nl) atomicAdd(&s_h[w][c[u]], 1); else bad = true; }
        }
        if (bad) atomicOr(status, 1);
        wave_sync();
        // (count, lowest class first) as one key: the wave's maximum is np.argmax's first maximum
        int key = lane < nl ? (s_h[w][lane] << 6) | (63 - lane) : -1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o));
        if (lane == 0) { const int d = 63 - (key & 63); out_label[s] = d; out_purity[s] = n > 0 ? (double)(key >> 6) / (double)n : 0.0; }
        wave_sync();
    }
}

// ---- clsbal (sampler2.py:262-266): u *= exp(-freq(dominant class among candidates + already selected)) -------
// `skip` != 0: the region is not in the population (labelled, or below min_size): prediction() appends only unlabelled regions to region_class
// (sampler2.py:612-627), so only those enter list_class
__global__ __launch_bounds__(256) void sel_class_hist(const int* __restrict__ region_class, int S, const unsigned char* __restrict__ skip, const int* __restrict__ extra, int n_extra, int* hist) {
    __shared__ int s_h[64];          // thousands of regions on a dozen classes: count in LDS, one global add per class and workgroup
    if (threadIdx.x < 64) s_h[threadIdx.x] = 0;
    __syncthreads();
    for (int i = blockIdx.x * 256 + threadIdx.x; i < S + n_extra; i += gridDim.x * 256) {
        if (i < S && skip && skip[i]) continue;
        const int c = i < S ? region_class[i] : extra[i - S];
        if (c >= 0 && c < 64) atomicAdd(&s_h[c], 1);
    }
    __syncthreads();
    if (threadIdx.x < 64 && s_h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_h[threadIdx.x]);
}
__global__ __launch_bounds__(256) void sel_clsbal(const int* __restrict__ region_class, int S, int total, const int* __restrict__ hist, double* region_unc) {
    if (total < 0) {                 // len(list_class) = what the histogram counted (a population behind a mask: the count is the device's)
        total = 0;
        for (int c = 0; c < 64; ++c) total += hist[c];
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < S; i += gridDim.x * 256) {
        const double w = (double)hist[region_class[i]] / (double)total;
        region_unc[i] = region_unc[i] * exp(-w);
    }
}

// ---- ranking: argsort(-u) (sampler2.py:640), ties by ascending index --------------------------------------------
// The order-preserving map of -u to u64, with NumPy's two rules for what IEEE bits alone order differently: +0.0 and -0.0 are EQUAL (0.0 - u is +0.0 for
// both, where -u keeps two bit patterns one key apart), and every NaN, whatever its sign bit, ranks LAST (one key above -u = +inf's 0xfff0...0; not all
// ones: sel_rank_count adds 1 to a key).  Equal keys go by ascending index in both rankers.
__device__ __forceinline__ unsigned long long rank_key(double u) {
    if (u != u) return 0xfffffffffffffffeull;
    const unsigned long long b = (unsigned long long)__double_as_longlong(0.0 - u);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__global__ __launch_bounds__(256) void sel_rank_keys(const double* __restrict__ u, int S, uint64_t* keys, uint32_t* vals) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < S; i += gridDim.x * 256) { keys[i] = rank_key(u[i]); vals[i] = (uint32_t)i; }
}

// Ranking of up to RANK_SMALL regions by COUNTING, spread over the chip: the rank of region i is the number of regions whose (key, index) pair is
// smaller — descending uncertainty, equal values by ascending index: the order the stable radix sort of (key, index) pairs gives.  Every workgroup
// stages all keys in LDS and ranks 32 regions, eight lanes per region (S^2 / 8 comparisons per lane group: 51 M in all for the bench's 7149 regions).
// The segmented radix sorter takes ~14 launch-bound launches for a few thousand keys (0.17 ms in front of every selection), a bitonic network in one
// workgroup 0.1 ms (one CU's vector rate); this is one launch of ~10 us.
constexpr int RANK_SMALL = 8192;
__global__ __launch_bounds__(256) void sel_rank_count(const double* __restrict__ u, int S, int* __restrict__ sorted_inds) {
    __shared__ unsigned long long s_k[RANK_SMALL];
    const int tid = threadIdx.x;
    for (int i = tid; i < S; i += 256) s_k[i] = rank_key(u[i]);
    __syncthreads();
    const int i = blockIdx.x * 32 + (tid >> 3), part = tid & 7;
    const bool live = i < S;
    const unsigned long long ki = s_k[live ? i : 0];
    int cnt = 0;
    if (live) {
        // (kj, j) < (ki, i)  <=>  kj < ki + (j < i): one 64-bit add and compare per pair (ki + 1 does not wrap: the largest key, a NaN's, is all ones minus one); eight
        // LDS reads in flight
        int j = part;
        for (; j + 56 < S; j += 64) {
            unsigned long long kj[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) kj[t] = s_k[j + 8 * t];
#pragma unroll
            for (int t = 0; t < 8; ++t) cnt += kj[t] < ki + (unsigned long long)(j + 8 * t < i);
        }
        for (; j < S; j += 8) cnt += s_k[j] < ki + (unsigned long long)(j < i);
    }
    cnt += __shfl_xor(cnt, 1); cnt += __shfl_xor(cnt, 2); cnt += __shfl_xor(cnt, 4);
    if (live && part == 0) sorted_inds[cnt] = i;
}

// ---- U3: compute_features (sampler2.py:333,339): float32 row-sequential mean over the dominant-class members ----
__global__ __launch_bounds__(256) void sel_segment_mean(const float* __restrict__ feat, int D, const int* __restrict__ cls_pred, const int* __restrict__ dom,
                                                        const int* __restrict__ sp_off, const int* __restrict__ sp_pts,
                                                        const int* __restrict__ sel, int nsel, float* out, const int* __restrict__ dn = nullptr,
                                                        double* y0 = nullptr, double* y1 = nullptr, const int* __restrict__ cls_lab = nullptr,
                                                        const int* __restrict__ dom_lab = nullptr, const int* __restrict__ d_nfirst = nullptr) {
    if (dn) nsel = min(nsel, *dn);               // the row count is the device's (candidate rule on the device)
    // rows >= *d_nfirst are the labelled regions: their dominant_point_ids come from the GROUND-TRUTH classes (sampler2.py:288-291), the candidates'
    // from the predicted ones (:625-626)
    const int nfirst = (cls_lab && d_nfirst) ? *d_nfirst : nsel;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < nsel * D; e += gridDim.x * 256) {
        const int q = e / D, c = e % D, s = sel ? sel[q] : q;
        const int* __restrict__ cls = q < nfirst ? cls_pred : cls_lab;
        const int lo = sp_off[s], hi = sp_off[s + 1], d = (q < nfirst ? dom : dom_lab)[s];
        float sum = 0.f; int cnt = 0;
        // thirty-two members at a time: their three dependent loads (member, class, feature) are in flight together; the additions stay in
        // member order (sixteen: 40 us for the bench's 1184 regions of ~185 points — a chain of round trips, not bandwidth)
        for (int j0 = lo; j0 < hi; j0 += 32) {
            int p[32], k[32]; float v[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) p[u] = sp_pts[min(j0 + u, hi - 1)];
#pragma unroll
            for (int u = 0; u < 32; ++u) { k[u] = cls[p[u]]; v[u] = feat[(size_t)p[u] * D + c]; }
#pragma unroll
            for (int u = 0; u < 32; ++u) if (j0 + u < hi && k[u] == d) { sum = sum + v[u]; ++cnt; }
        }
        const float mean = cnt ? sum / (float)cnt : 0.f;
        if (out) out[(size_t)q * D + c] = mean;
        if (y0) { y0[(size_t)q * D + c] = (double)mean; y1[(size_t)q * D + c] = (double)mean; }      // float32 -> float64 as np.concatenate / np.matmul promote it
    }
}

// ---- F1/F2: bbox centres, chamfer, adjacency, propagation for the superpoints `sel` of ONE cloud ----------------
// The lay-out of one cloud (one workgroup): slots of the cloud start at ITEM * (its first row), the per-superpoint tables at its first row.
__device__ void chamfer_plan_body(const int* __restrict__ sp_off, const int* __restrict__ sel, int n, ChamferPack P, int* counts, int* s_n) {
    const int tid = threadIdx.x;
    if (n > PACK_MAX) {
        for (int i = tid; i < n; i += 256) { P.big[i] = i; P.start[i] = -1; }
        if (tid == 0) { counts[0] = 0; counts[1] = n; }
        return;
    }
    for (int i = tid; i < n; i += 256) { const int sp = sel[i]; s_n[i] = sp_off[sp + 1] - sp_off[sp]; }
    __syncthreads();
    // The lay-out: whole superpoints into 256-slot items, in order.  Rounds 2-4 filled ONE item at a time (next fit: ~70 % full — and every padding slot is a
    // lane that runs the whole distance loop for nothing); round 5 keeps the last FOUR opened items open and takes the first of them with room (the fullest-
    // effort rule, first fit over ALL items by one wave with the free slots in registers, packed 3 % tighter and cost 0.1 ms more per step than it saved:
    // a lone wave spends ~1 us per superpoint on the ballot / readlane chain).  Which item a superpoint lands in changes nothing but the padding: its
    // roots are summed in an order that depends on its size alone.  One lane, the recurrence carried in scalars.
    __shared__ int s_start[PACK_MAX];
    if (tid == 0) {
        int base[4] = {0, 0, 0, 0}, used[4] = {ITEM, ITEM, ITEM, ITEM}, items = 0;
        for (int i = 0; i < n; ++i) {
            const int ni = s_n[i];
            if (ni == 0 || ni > ITEM) { s_start[i] = -1; continue; }
            int j = -1;
#pragma unroll
            for (int k = 0; k < 4; ++k) if (j < 0 && used[k] + ni <= ITEM) j = k;
            if (j < 0) {          // nothing open takes it: the oldest open item is closed, a new one opened
#pragma unroll
                for (int k = 0; k < 3; ++k) { base[k] = base[k + 1]; used[k] = used[k + 1]; }
                j = 3; base[3] = items++ * ITEM; used[3] = 0;
            }
            int st = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k == j) { st = base[k] + used[k]; used[k] += ni; }
            s_start[i] = st;
        }
    }
    __syncthreads();
    // ranks of the item openers and of the pair-by-pair superpoints: counted per thread over a contiguous piece, then offset by the pieces before
    const int per = (n + 255) / 256, lo = min(n, tid * per), hi = min(n, lo + per);
    int ci = 0, cb = 0;
    for (int i = lo; i < hi; ++i) { const int st = s_start[i]; if (st < 0) ++cb; else if ((st & (ITEM - 1)) == 0) ++ci; }
    // exclusive prefix over the 256 pieces: inside a wave by shuffles, across the four waves through LDS (a serial pass by one lane took ~10 us)
    {
        const int lane = tid & 63, w = tid >> 6;
        int pi = ci, pb = cb;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int ui = __shfl_up(pi, o), ub = __shfl_up(pb, o); if (lane >= o) { pi += ui; pb += ub; } }
        __shared__ int s_wi[4], s_wb[4];
        if (lane == 63) { s_wi[w] = pi; s_wb[w] = pb; }
        __syncthreads();
        int oi = 0, ob = 0;
        for (int k = 0; k < w; ++k) { oi += s_wi[k]; ob += s_wb[k]; }
        if (tid == 255) { counts[0] = oi + pi; counts[1] = ob + pb; }
        ci = oi + pi - ci; cb = ob + pb - cb;          // exclusive
    }
    for (int i = lo; i < hi; ++i) {
        const int st = s_start[i];
        P.start[i] = st;
        if (st < 0) P.big[cb++] = i;
        else if ((st & (ITEM - 1)) == 0) P.item_slot[ci++] = st;
    }
}
// ... and its slots: one wave per superpoint (seg / cnt / r2item of the padding slots and unused items were preset by the launcher: -1 / 0 / 0).
// r2sp / r2item: the largest |p|^2 of the superpoint / of the item's superpoints, rounded up — what bounds the float32 screening's error (select_chamfer.hip)
__device__ void chamfer_fill_body(const float* __restrict__ xyz, const int* __restrict__ sp_off, const int* __restrict__ sp_pts, const int* __restrict__ sel, int n,
                                  double* __restrict__ centres, ChamferPack P) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
        const int st = P.start[i];
        const int sp = sel[i], lo = sp_off[sp], ni = sp_off[sp + 1] - lo;
        // the superpoint's bounding-box centre (sel_centres' arithmetic; its launch is saved: the wave reads the points twice, the second time from L2)
        float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        for (int a = lane; a < ni; a += 64) {
            const size_t q = sp_pts[lo + a];
#pragma unroll
            for (int d = 0; d < 3; ++d) { const float v = xyz[3 * q + d]; mn[d] = fminf(mn[d], v); mx[d] = fmaxf(mx[d], v); }
        }
        double cen[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) cen[d] = (double)(wave_min(mn[d]) + wave_max(mx[d])) / 2.0;      // float32 add, exact halving (fps_gcn_cpu.py:86-88)
        if (lane < 3) centres[3 * (size_t)i + lane] = lane == 0 ? cen[0] : lane == 1 ? cen[1] : cen[2];
        const double cx = cen[0], cy = cen[1], cz = cen[2];
        double r2 = 0.0;
        for (int a = lane; a < ni; a += 64) {
            const size_t q = sp_pts[lo + a];
            const double x = (double)xyz[3 * q] - cx, y = (double)xyz[3 * q + 1] - cy, z = (double)xyz[3 * q + 2] - cz;
            r2 = fmax(r2, (x * x + y * y) + z * z);
            if (st >= 0) {
                const int k = st + a;
                P.x[k] = x; P.y[k] = y; P.z[k] = z;
                P.seg[k] = i; P.cnt[k] = a == 0 ? ni : 0;
                P.src0[k] = source_operand(x, y, 0);
                const uint4 up = source_operand(z, 0.0, 1);
                P.src1[k] = (unsigned long long)up.x | ((unsigned long long)up.y << 32);
            }
        }
        const float r = wave_max((float)(r2 * 1.000001));
        if (lane == 0) {
            P.r2sp[i] = r;
            if (st >= 0) atomicMax((unsigned*)&P.r2item[st / ITEM], __float_as_uint(r));      // non-negative floats order like their bit patterns
        }
    }
}

__global__ __launch_bounds__(256) void sel_chamfer_plan(const int* __restrict__ sp_off, const int* __restrict__ sel, const int* __restrict__ coff, int nsingle, ChamferPack P) {
    __shared__ int s_n[PACK_MAX];
    const int c = blockIdx.x, lo = coff ? coff[c] : 0, n = coff ? coff[c + 1] - lo : nsingle;
    chamfer_plan_body(sp_off, sel + lo, n, pack_at(P, lo), P.counts + 2 * c, s_n);
}
__global__ __launch_bounds__(256) void sel_chamfer_fill(const float* __restrict__ xyz, const int* __restrict__ sp_off, const int* __restrict__ sp_pts,
                                                        const int* __restrict__ sel, const int* __restrict__ coff, int nsingle, double* __restrict__ centres, ChamferPack P) {
    const int c = blockIdx.y, lo = coff ? coff[c] : 0, n = coff ? coff[c + 1] - lo : nsingle;
    chamfer_fill_body(xyz, sp_off, sp_pts, sel + lo, n, centres + 3 * (size_t)lo, pack_at(P, lo));
}

// adj = exp(-(ED + CD)) - I (fps_gcn_cpu.py:102-104); rowsum (:106)
__device__ void adj_build_body(const double* __restrict__ centres, const double* __restrict__ dir, int n, double* adj, double* rowsum, double* part) {
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        double acc = 0.0;
        for (int j = threadIdx.x; j < n; j += 256) {
            const double dx = centres[3 * i] - centres[3 * j], dy = centres[3 * i + 1] - centres[3 * j + 1], dz = centres[3 * i + 2] - centres[3 * j + 2];
            const double ed = sqrt((dx * dx + dy * dy) + dz * dz);
            const double cd = dir[(size_t)i * n + j] + dir[(size_t)j * n + i];
            double v = exp(-(ed + cd));
            if (i == j) v = v - 1.0;
            adj[(size_t)i * n + j] = v; acc += v;
        }
        part[threadIdx.x] = acc;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o]; __syncthreads(); }
        if (threadIdx.x == 0) rowsum[i] = part[0];
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void sel_adj_build(const double* __restrict__ centres, const double* __restrict__ dir, int n, double* adj, double* rowsum) {
    __shared__ double part[256];
    adj_build_body(centres, dir, n, adj, rowsum, part);
}
__global__ __launch_bounds__(256) void sel_adj_build_batch(const double* __restrict__ centres, const double* __restrict__ dir, const int* __restrict__ coff,
                                                           const long long* __restrict__ boff, double* adj, double* rowsum) {
    __shared__ double part[256];
    const int c = blockIdx.z, lo = coff[c];
    adj_build_body(centres + 3 * (size_t)lo, dir + boff[c], coff[c + 1] - lo, adj + boff[c], rowsum + lo, part);
}
// adj = adj * diag(1/rowsum) + I (:108-115): column j scaled by 1/rowsum[j], inf -> 0
__device__ void adj_norm_body(const double* __restrict__ rowsum, int n, double* adj) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < (size_t)n * n; e += (size_t)gridDim.x * 256) {
        const int i = (int)(e / n), j = (int)(e % n);
        double dinv = 1.0 / rowsum[j];
        if (__builtin_isinf(dinv)) dinv = 0.0;
        adj[e] = adj[e] * dinv + (i == j ? 1.0 : 0.0);
    }
}
__global__ __launch_bounds__(256) void sel_adj_norm(const double* __restrict__ rowsum, int n, double* adj) { adj_norm_body(rowsum, n, adj); }
__global__ __launch_bounds__(256) void sel_adj_norm_batch(const double* __restrict__ rowsum, const int* __restrict__ coff, const long long* __restrict__ boff, double* adj) {
    const int c = blockIdx.z, lo = coff[c];
    adj_norm_body(rowsum + lo, coff[c + 1] - lo, adj + boff[c]);
}
// keep the gcn_top largest entries of every row (fps_gcn_cpu.py:153-160: mask[row, argsort(row)[-top:]] = 1); among equal entries the
// higher column index is kept (NumPy's quicksort leaves such ties unspecified).  One wave per row: the row is copied to LDS, every
// lane ranks its columns against the whole row (n^2 / 64 comparisons per lane) and zeroes the ones ranked >= top.
constexpr int TOPK_ROW = 2048;       // columns a wave keeps in LDS (4 waves x 16 KiB); longer rows rank against global memory
__device__ void adj_topk_body(double* adj, int n, int top, double* s_row /* [4][TOPK_ROW] */) {
    if (top <= 0 || top >= n) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    double* mine = s_row + (size_t)wid * TOPK_ROW;
    const bool in_lds = n <= TOPK_ROW;
    for (int i0 = blockIdx.x * 4; i0 < n; i0 += gridDim.x * 4) {          // uniform over the workgroup: barriers inside
        const int i = i0 + wid;
        const bool live = i < n;
        double* row = adj + (size_t)(live ? i : 0) * n;
        if (live && in_lds) for (int k = lane; k < n; k += 64) mine[k] = row[k];
        __syncthreads();
        for (int base = 0; base < n; base += 64 * 64) {
            unsigned long long zero = 0ull;   // this lane's columns j = base + lane + 64 u to clear
            if (live)
                for (int u = 0; u < 64; ++u) {
                    const int j = base + lane + 64 * u;
                    if (j >= n) break;
                    // rows longer than the LDS copy are ranked in place: a column already decided is stored as -v - 4 (entries lie in
                    // [0, 2]) and decoded here, and is cleared after the whole row has been ranked
                    auto val = [&](int k) { const double v = in_lds ? mine[k] : row[k]; return v < -1.0 ? -(v + 4.0) : v; };
                    const double vj = val(j);
                    int larger = 0;
                    for (int k = 0; k < n; ++k) { const double vk = val(k); larger += (vk > vj) || (vk == vj && k > j); }
                    if (larger >= top) zero |= 1ull << u;
                }
            if (!in_lds) __syncthreads();     // every lane has read this pass's columns before anyone marks one
            for (int u = 0; u < 64; ++u) if ((zero >> u) & 1ull) row[base + lane + 64 * u] = in_lds ? 0.0 : -row[base + lane + 64 * u] - 4.0;
            if (!in_lds) __syncthreads();
        }
        if (live && !in_lds) for (int k = lane; k < n; k += 64) if (row[k] < -1.0) row[k] = 0.0;
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void sel_adj_topk(double* adj, int n, int top) {
    __shared__ double s_row[4 * TOPK_ROW];
    adj_topk_body(adj, n, top, s_row);
}
__global__ __launch_bounds__(256) void sel_adj_topk_batch(double* adj, const int* __restrict__ coff, const long long* __restrict__ boff, int top) {
    __shared__ double s_row[4 * TOPK_ROW];
    const int c = blockIdx.z;
    adj_topk_body(adj + boff[c], coff[c + 1] - coff[c], top, s_row);
}
// Vout[rows[i]] = sum_j adj[i][j] * Vin[rows[j]]  (one hop of fps_gcn_cpu.py:164-165), comb[rows[i]] += Vout
__device__ void propagate_body(const double* __restrict__ adj, int n, const int* __restrict__ rows, const double* __restrict__ vin, int D,
                               double* vout, double* comb) {
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n * D; e += gridDim.x * 256) {
        const int i = e / D, c = e % D;
        double acc = 0.0;
        // eight terms' dependent loads (row index, then the feature) in flight; the additions stay in column order (np.matmul's row-times-column sum
        // is compared at 1e-12, and the selection downstream must not depend on the unrolling)
        for (int j0 = 0; j0 < n; j0 += 8) {
            int rj[8]; double a[8], v[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) rj[t] = rows[min(j0 + t, n - 1)];
#pragma unroll
            for (int t = 0; t < 8; ++t) { a[t] = adj[(size_t)i * n + min(j0 + t, n - 1)]; v[t] = vin[(size_t)rj[t] * D + c]; }
#pragma unroll
            for (int t = 0; t < 8; ++t) if (j0 + t < n) acc += a[t] * v[t];
        }
        vout[(size_t)rows[i] * D + c] = acc;
        comb[(size_t)rows[i] * D + c] += acc;
    }
}
__global__ __launch_bounds__(256) void sel_propagate(const double* __restrict__ adj, int n, const int* __restrict__ rows, const double* __restrict__ vin, int D,
                                                     double* vout, double* comb) { propagate_body(adj, n, rows, vin, D, vout, comb); }
__global__ __launch_bounds__(256) void sel_propagate_batch(const double* __restrict__ adj, const int* __restrict__ coff, const long long* __restrict__ boff,
                                                           const int* __restrict__ rows, const double* __restrict__ vin, int D, double* vout, double* comb) {
    const int c = blockIdx.z, lo = coff[c];
    propagate_body(adj + boff[c], coff[c + 1] - lo, rows + lo, vin, D, vout, comb);
}

__global__ __launch_bounds__(256) void widen_f32_f64(const float* __restrict__ x, size_t n, double* y0, double* y1) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) { const double v = (double)x[i]; y0[i] = v; if (y1) y1[i] = v; }
}

// ---- gcn.create_adj (gcn.py:116-191): the adjacency of the trained-GCN branch, torch float32 in the reference ---------------------------
// rows of V: features / max(|features|_2, 1e-12) (torch.nn.functional.normalize)
__global__ __launch_bounds__(256) void ca_normalize(const float* __restrict__ f, int n, int F, float* V) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
        float ss = 0.f;
        for (int k = lane; k < F; k += 64) { const float v = f[(size_t)i * F + k]; ss += v * v; }
        for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
        const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
        for (int k = lane; k < F; k += 64) V[(size_t)i * F + k] = f[(size_t)i * F + k] * inv;
    }
}
// one cloud's block: adj[rows[i]][rows[j]] = <V_i, V_j> * exp(-((float)ED + (float)CD)), minus 1 on the diagonal.  Entries between clouds are
// <V_i, V_j> * exp(-2e10) = +-0 in the reference: the matrix is cleared beforehand.
__global__ __launch_bounds__(256) void ca_block(const float* __restrict__ V, int F, const double* __restrict__ centres, const double* __restrict__ dir,
                                                const int* __restrict__ coff, const long long* __restrict__ boff, const int* __restrict__ rows, int N, float* adj) {
    const int c = blockIdx.z, r0 = coff[c], nc = coff[c + 1] - r0;
    const double* D = dir + boff[c];
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < (long)nc * nc; e += (long)gridDim.x * 256) {
        const int i = (int)(e / nc), j = (int)(e % nc);
        const int gi = rows[r0 + i], gj = rows[r0 + j];
        const double dx = centres[3 * (size_t)(r0 + i)] - centres[3 * (size_t)(r0 + j)], dy = centres[3 * (size_t)(r0 + i) + 1] - centres[3 * (size_t)(r0 + j) + 1],
                     dz = centres[3 * (size_t)(r0 + i) + 2] - centres[3 * (size_t)(r0 + j) + 2];
        const double ed = sqrt((dx * dx + dy * dy) + dz * dz);
        const double cd = i == j ? 0.0 : D[(size_t)i * nc + j] + D[(size_t)j * nc + i];
        float lat = 0.f;
        for (int k = 0; k < F; ++k) lat += V[(size_t)gi * F + k] * V[(size_t)gj * F + k];
        adj[(size_t)gi * N + gj] = lat * expf(-((float)ed + (float)cd)) - (gi == gj ? 1.0f : 0.0f);
    }
}
// column sums (torch.sum(adj, dim=0)), then adj[:, j] *= 1 / sum_j, plus I
__global__ __launch_bounds__(256) void ca_colsum(const float* __restrict__ adj, int N, float* colsum) {
    for (int j = blockIdx.x * 256 + threadIdx.x; j < N; j += gridDim.x * 256) {
        float s = 0.f;
        for (int i = 0; i < N; ++i) s += adj[(size_t)i * N + j];
        colsum[j] = s;
    }
}
__global__ __launch_bounds__(256) void ca_scale(float* adj, int N, const float* __restrict__ colsum) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < (long)N * N; e += (long)gridDim.x * 256) {
        const int i = (int)(e / N), j = (int)(e % N);
        adj[e] = adj[e] * (1.0f / colsum[j]) + (i == j ? 1.0f : 0.0f);
    }
}

// ---- the candidate rule on the device (sampler2.py:533-552 create_file_top_and_all, :745-753 GCN_FPS_sampling's caller) -----------------------
// order[] ranks the regions by descending uncertainty.  cand = the unlabelled ones in that order; the first min(batch, S) of them are "top";
// a cloud offers its first 2 x (its number of top regions) candidates.  The superpoints of cloud c are sp_base[c] .. sp_base[c+1]-1.
// Results: the candidates cloud by cloud (descending uncertainty inside a cloud) followed by the labelled regions (refs), the same rows grouped
// cloud by cloud (candidates then labelled of the cloud: the block structure of the graph), and the counts downstream kernels read instead of
// host-side sizes.  counts[]: 0 n_unl, 1 n_lab, 2 ntot, 3 nmax, 4 sampling_batch, 5 status (1: more rows, 2: more block elements than the
// caller's capacity), 6-7 the block elements as int64.
constexpr int CR_NT = 1024;
__global__ __launch_bounds__(CR_NT) void cand_rank(const int* __restrict__ order, int S, const unsigned char* __restrict__ labelled, int* rankpos, int* cploc, int* chunkcnt) {
    __shared__ int s_w[CR_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r = blockIdx.x * CR_NT + tid;
    int sp = -1, v = 0;
    if (r < S) { sp = order[r]; v = labelled[sp] ? 0 : 1; }
    const unsigned long long m = __ballot(v);
    if (lane == 0) s_w[wid] = __popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < CR_NT / 64; ++w) { const int c = s_w[w]; if (w < wid) base += c; tot += c; }
    if (sp >= 0) { rankpos[sp] = r; cploc[sp] = base + __popcll(m & ((1ull << lane) - 1ull)); }
    if (tid == 0) chunkcnt[blockIdx.x] = tot;
}
// exclusive prefix of n ints in place by one workgroup of 256: every thread owns a contiguous piece
__device__ void block_exscan_inplace(int* a, int n, int* s_part /* [257] */) {
    const int tid = threadIdx.x, per = (n + 255) / 256, lo = min(n, tid * per), hi = min(n, lo + per);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += a[i];
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) { int run = 0; for (int t = 0; t < 256; ++t) { const int v = s_part[t]; s_part[t] = run; run += v; } s_part[256] = run; }
    __syncthreads();
    int run = s_part[tid];
    for (int i = lo; i < hi; ++i) { const int v = a[i]; a[i] = run; run += v; }
    __syncthreads();
}
__global__ __launch_bounds__(256) void cand_chunkscan(int* chunkcnt, int nchunks) {
    __shared__ int s_part[257];
    block_exscan_inplace(chunkcnt, nchunks, s_part);
}
constexpr int CC_TILE = 2048;
__global__ __launch_bounds__(256) void cand_cloud(const int* __restrict__ rankpos, const int* __restrict__ cploc, const int* __restrict__ chunkoff,
                                                  const unsigned char* __restrict__ labelled, const int* __restrict__ sp_base, int S, int batch_size,
                                                  int* stage, int* ncand, int* ntop) {
    __shared__ __attribute__((aligned(16))) int s_tile[CC_TILE];
    __shared__ int s_red[8];
    const int tid = threadIdx.x, c = blockIdx.x, lo = sp_base[c], n = sp_base[c + 1] - lo;
    const int lim = min(batch_size, S);
    // blockIdx.y: a slice of the cloud's regions (every 256 * gridDim.y-th block of 256).  A region's place inside its cloud is found by counting, n^2 per cloud:
    // nothing at the ~450 regions of the stand-in's tiles, 5 ms on one workgroup at 8 300 (a partition of many small regions, tools/variety_probe.py)
    if ((int)blockIdx.y * 256 >= n && blockIdx.y > 0) return;
    int nv = 0, nt = 0;
    for (int j = tid; j < n; j += 256)
        if (!labelled[lo + j]) { ++nv; const int r = rankpos[lo + j]; nt += (chunkoff[r / CR_NT] + cploc[lo + j]) < lim; }
    block_sum2<256>(nv, nt, s_red);
    const int take = min(2 * nt, nv);
    if (tid == 0 && blockIdx.y == 0) { ncand[c] = take; ntop[c] = nt; }
    for (int j0 = (int)blockIdx.y * 256; j0 < n; j0 += 256 * (int)gridDim.y) {
        const int j = j0 + tid;
        const bool live = j < n && !labelled[lo + j];
        const int rj = live ? rankpos[lo + j] : 0x7fffffff;
        int pos = 0;
        for (int t0 = 0; t0 < n; t0 += CC_TILE) {
            const int m = min(CC_TILE, n - t0);
            __syncthreads();
            for (int k = tid; k < ((m + 3) & ~3); k += 256) s_tile[k] = (k >= m || labelled[lo + t0 + k]) ? 0x7fffffff : rankpos[lo + t0 + k];
            __syncthreads();
            if (live) {          // four rank positions per LDS read (the tile is padded with +infinity to a multiple of four)
                const int4* t4 = reinterpret_cast<const int4*>(s_tile);
                for (int k = 0; k < (m + 3) / 4; ++k) { const int4 v = t4[k]; pos += (v.x < rj) + (v.y < rj) + (v.z < rj) + (v.w < rj); }
            }
        }
        if (live && pos < take) stage[lo + pos] = lo + j;
    }
}
// slices of a cloud's regions for cand_cloud: one below ~1000 regions per cloud on average, up to 32 above (the host knows the totals, not a cloud's own count)
static unsigned cand_slices(size_t S, size_t B) { const size_t avg = S / std::max<size_t>(B, 1); return (unsigned)std::min<size_t>(32, std::max<size_t>(1, avg / 512)); }
__global__ __launch_bounds__(256) void cand_layout(const int* __restrict__ ncand, const int* __restrict__ ntop, const int* __restrict__ lab_off, int B,
                                                   long long cap_rows, long long cap_sq, int* uoff, int* coff, long long* boff, int* counts) {
    __shared__ long long s_p[3][257];
    __shared__ int s_mx[256];
    const int tid = threadIdx.x, per = (B + 255) / 256, lo = min(B, tid * per), hi = min(B, lo + per);
    long long su = 0, sc = 0, sb = 0; int mx = 0, st = 0;
    for (int c = lo; c < hi; ++c) { const long long a = ncand[c] + (lab_off[c + 1] - lab_off[c]); su += ncand[c]; sc += a; sb += a * a; mx = max(mx, (int)a); st += ntop[c]; }
    s_p[0][tid] = su; s_p[1][tid] = sc; s_p[2][tid] = sb; s_mx[tid] = mx;
    __syncthreads();
    // sampling_batch: the tops of all clouds
    __shared__ int s_st[256];
    s_st[tid] = st;
    __syncthreads();
    if (tid == 0) {
        long long r0 = 0, r1 = 0, r2 = 0; int m = 0, t = 0;
        for (int k = 0; k < 256; ++k) { const long long a = s_p[0][k], b = s_p[1][k], q = s_p[2][k]; s_p[0][k] = r0; s_p[1][k] = r1; s_p[2][k] = r2; r0 += a; r1 += b; r2 += q; m = max(m, s_mx[k]); t += s_st[k]; }
        int status = 0;
        if (r1 > cap_rows) status |= 1;
        if (r2 > cap_sq) status |= 2;
        counts[0] = status ? 0 : (int)r0; counts[1] = lab_off[B]; counts[2] = status ? 0 : (int)r1; counts[3] = m; counts[4] = t; counts[5] = status;
        counts[6] = (int)(r2 & 0xffffffffll); counts[7] = (int)(r2 >> 32);
        s_p[0][256] = status;
    }
    __syncthreads();
    const bool bad = s_p[0][256] != 0;           // over capacity: every block is empty, nothing downstream runs; the caller reads the status
    long long u = s_p[0][tid], k = s_p[1][tid], q = s_p[2][tid];
    for (int c = lo; c < hi; ++c) {
        const long long a = ncand[c] + (lab_off[c + 1] - lab_off[c]);
        uoff[c] = (int)u; coff[c] = bad ? 0 : (int)k; boff[c] = bad ? 0 : q;
        u += ncand[c]; k += a; q += a * a;
    }
    if (hi == B && lo < B) { uoff[B] = (int)u; coff[B] = bad ? 0 : (int)k; boff[B] = bad ? 0 : q; }
    if (B == 0 && tid == 0) { uoff[0] = 0; coff[0] = 0; boff[0] = 0; }
}
__global__ __launch_bounds__(256) void cand_fill(const int* __restrict__ stage, const int* __restrict__ sp_base, const int* __restrict__ ncand, const int* __restrict__ uoff,
                                                 const int* __restrict__ coff, const int* __restrict__ lab_off, const int* __restrict__ lab_sp, const int* __restrict__ counts,
                                                 int* sel, int* gsel, int* rows, int* already) {
    if (counts[5]) return;
    const int c = blockIdx.x, nc = ncand[c], u0 = uoff[c], g0 = coff[c], l0 = lab_off[c], nl = lab_off[c + 1] - l0, n_unl = counts[0], lo = sp_base[c];
    for (int k = threadIdx.x; k < nc; k += 256) { const int sp = stage[lo + k]; sel[u0 + k] = sp; gsel[g0 + k] = sp; rows[g0 + k] = u0 + k; }
    for (int k = threadIdx.x; k < nl; k += 256) { const int sp = lab_sp[l0 + k]; sel[n_unl + l0 + k] = sp; gsel[g0 + nc + k] = sp; rows[g0 + nc + k] = n_unl + l0 + k; already[l0 + k] = n_unl + l0 + k; }
}


// ---- the candidate rule of the SHARDED run on the device ------------------------------------------------------------------------------------------------
// Every rank holds the global ranking (regions of all ranks, global id = rank * Smax + local id, padding counted as labelled) and runs the rule over all
// clouds of all ranks (cloud rank * Bmax + b): what it keeps for its own graph are its own clouds; what it needs of the others are their candidate COUNTS
// (where each rank's rows sit in the padded all-gather of the propagated features) and, for the read-back, the global candidate list.
// plan[]: 0 n_unl (this rank), 1 n_lab, 2 rows, 3 largest block, 4 sampling_batch (all ranks), 5 status, 6-7 block elements, 8 n_unl of all ranks,
// 9 bit 0: a rank offers more than nu_max candidates; [16 .. 16 + W) candidates per rank; then [W * nu_max] the rows of the gathered array in
// candidate order, then [W * nu_max] the global candidate list (global region ids).
__global__ __launch_bounds__(256) void cand_global(const int* __restrict__ ncand, const int* __restrict__ ntop, int W, int Bmax, int nu_max, int* guoff, int* plan) {
    __shared__ int s_cnt[64], s_off[65], s_top[256], s_bad;
    const int tid = threadIdx.x, Bg = W * Bmax;
    int t = 0;
    for (int c = tid; c < Bg; c += 256) t += ntop[c];
    s_top[tid] = t;
    if (tid < W) { int n = 0; for (int b = 0; b < Bmax; ++b) n += ncand[tid * Bmax + b]; s_cnt[tid] = n; }
    __syncthreads();
    if (tid == 0) {
        int run = 0, bad = 0, tot = 0;
        for (int r = 0; r < W; ++r) { s_off[r] = run; run += s_cnt[r]; bad |= s_cnt[r] > nu_max; plan[16 + r] = s_cnt[r]; }
        s_off[W] = run;
        for (int k = 0; k < 256; ++k) tot += s_top[k];
        plan[4] = tot; plan[8] = bad ? 0 : run; plan[9] = bad; s_bad = bad;
    }
    __syncthreads();
    // candidate offsets of the global clouds, rank-major (a rank's clouds are consecutive)
    if (tid < W) { int run = s_off[tid]; for (int b = 0; b < Bmax; ++b) { guoff[tid * Bmax + b] = run; run += ncand[tid * Bmax + b]; } }
    if (tid == 0) guoff[Bg] = s_off[W];
    if (s_bad) return;          // a rank offers more than nu_max: the prefix sums run past the 2 * W * nu_max words behind the plan (plan[9] says so)
    int* src = plan + 16 + W;
    for (int r = 0; r < W; ++r) for (int p = tid; p < min(s_cnt[r], nu_max); p += 256) src[s_off[r] + p] = r * nu_max + p;
}
__global__ __launch_bounds__(256) void cand_fill_global(const int* __restrict__ stage, const int* __restrict__ gbase, const int* __restrict__ ncand, const int* __restrict__ guoff,
                                                        const int* __restrict__ plan, int* glist) {
    if (plan[9]) return;
    const int c = blockIdx.x, nc = ncand[c], u0 = guoff[c], lo = gbase[c];
    for (int k = threadIdx.x; k < nc; k += 256) glist[u0 + k] = stage[lo + k];
}
// cand_fill for one rank's clouds: stage holds global region ids, the local tables want local ones
__global__ __launch_bounds__(256) void cand_fill_local(const int* __restrict__ stage, const int* __restrict__ gbase, const int* __restrict__ ncand, const int* __restrict__ uoff,
                                                       const int* __restrict__ coff, const int* __restrict__ lab_off, const int* __restrict__ lab_sp, const int* __restrict__ counts,
                                                       int sub, int* sel, int* gsel, int* rows) {
    if (counts[5]) return;
    const int c = blockIdx.x, nc = ncand[c], u0 = uoff[c], g0 = coff[c], l0 = lab_off[c], nl = lab_off[c + 1] - l0, n_unl = counts[0], lo = gbase[c];
    for (int k = threadIdx.x; k < nc; k += 256) { const int sp = stage[lo + k] - sub; sel[u0 + k] = sp; gsel[g0 + k] = sp; rows[g0 + k] = u0 + k; }
    for (int k = threadIdx.x; k < nl; k += 256) { const int sp = lab_sp[l0 + k]; sel[n_unl + l0 + k] = sp; gsel[g0 + nc + k] = sp; rows[g0 + nc + k] = n_unl + l0 + k; }
}
// rows [0, n) of src -> dst, n on the device
// rows idx[k % n] of in -> row k of out for k < repeat * n (n on the device); nrep receives repeat * n
__global__ __launch_bounds__(256) void sel_gather_rows_rep(const uint32_t* __restrict__ in, const int* __restrict__ idx, int cap, int row_words, uint32_t* __restrict__ out,
                                                           const int* __restrict__ dn, int repeat, int* nrep) {
    const int n = *dn, tot = min(cap, n * repeat);
    if (blockIdx.x == 0 && threadIdx.x == 0) *nrep = tot;
    const long total = (long)tot * row_words;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int r = (int)(e / row_words), c = (int)(e % row_words);
        out[e] = in[(size_t)idx[r % n] * row_words + c];
    }
}
__global__ __launch_bounds__(256) void copy_rows_dn(const double* __restrict__ src, double* __restrict__ dst, int row_len, int cap, const int* __restrict__ dn) {
    const long total = (long)min(cap, *dn) * row_len;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) dst[e] = src[e];
}

// rows [*off, *off + n) of src -> rows [0, n) of dst (the labelled regions' propagated rows sit behind the candidates, whose count is the device's)
__global__ __launch_bounds__(256) void copy_rows_from(const double* __restrict__ src, double* __restrict__ dst, int row_len, int n, const int* __restrict__ off) {
    const long total = (long)n * row_len, o = (long)*off * row_len;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) dst[e] = src[o + e];
}
// The global array of the sharded k-center: [every rank's candidates, in candidate order | every rank's labelled regions, rank by rank] out of the all-gather
// of `per` = nu_max + nl_max rows per rank (candidates padded to nu_max, then the labelled ones); already[] = the labelled rows, *nrows = rows in all
__global__ __launch_bounds__(256) void sel_gather_kc(const uint32_t* __restrict__ in, const int* __restrict__ plan, int W, int nu_max, int per, const int* __restrict__ nlab_off,
                                                     int cap, int row_words, uint32_t* __restrict__ out, int* __restrict__ already, int* nrows) {
    const int n_unl = plan[9] ? 0 : plan[8], n_lab = nlab_off[W], tot = min(cap, n_unl + n_lab);
    const int* idx = plan + 16 + W;
    if (blockIdx.x == 0 && threadIdx.x == 0) *nrows = tot;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n_lab; j += gridDim.x * 256) already[j] = n_unl + j;
    const long total = (long)tot * row_words;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int r = (int)(e / row_words), c = (int)(e % row_words);
        int srow;
        if (r < n_unl) { const int g = idx[r]; srow = (g / nu_max) * per + g % nu_max; }
        else { const int j = r - n_unl; int q = 0; while (q + 1 < W && nlab_off[q + 1] <= j) ++q; srow = q * per + nu_max + (j - nlab_off[q]); }
        out[e] = in[(size_t)srow * row_words + c];
    }
}

struct SelState { RadixSorter sorter; DevBuf keys, vals, hist, mins, dir, rowsum, pack_xyz, pack_int, cand_i, cand_f;
                  const double* last_comb = nullptr; size_t last_cap = 0; };

// scratch of the chamfer packer for nrows superpoints in nclouds clouds
int chamfer_pack_buffers(SelState& Q, size_t nrows, size_t nclouds, ChamferPack& P) {
    const size_t slots = (size_t)ITEM * nrows;
    SSDR_TRY(Q.pack_xyz.reserve((3 * 8 + 16 + 8) * slots + 64)); SSDR_TRY(Q.pack_int.reserve(4 * (2 * slots + 5 * nrows + 2 * nclouds) + 64));
    P.x = Q.pack_xyz.as<double>(); P.y = P.x + slots; P.z = P.y + slots; P.src1 = (unsigned long long*)(P.z + slots); P.src0 = (uint4*)(P.src1 + slots);
    P.seg = Q.pack_int.as<int>(); P.cnt = P.seg + slots; P.r2item = (float*)(P.cnt + slots); P.r2sp = P.r2item + nrows;
    P.item_slot = (int*)(P.r2sp + nrows); P.big = P.item_slot + nrows; P.start = P.big + nrows; P.counts = P.start + nrows;
    return SSDR_OK;
}
// plan + fill of the packer for nclouds clouds (coff == nullptr: one cloud of nsingle superpoints); the fill also writes the superpoints' bounding-box
// centres (d_centres [nrows, 3]: what the adjacency kernels read) — rows the device-side count leaves unused are not touched
int chamfer_pack_launch(const ChamferPack& P, const float* d_xyz, const int* d_sp_off, const int* d_sp_pts, const int* d_sel, const int* d_coff, int nsingle,
                        size_t nrows, int n_max, unsigned nclouds, double* d_centres, hipStream_t s) {
    const size_t slots = (size_t)ITEM * nrows;
    SSDR_HIP(hipMemsetAsync(P.seg, 0xff, 4 * slots, s));          // padding slots: no superpoint ...
    SSDR_HIP(hipMemsetAsync(P.cnt, 0, 4 * (slots + nrows), s));   // ... and nothing to sum; r2item (behind cnt) = 0
    hipLaunchKernelGGL(sel_chamfer_plan, dim3(nclouds), dim3(256), 0, s, d_sp_off, d_sel, d_coff, nsingle, P);
    hipLaunchKernelGGL(sel_chamfer_fill, dim3(std::max(1, std::min((n_max + 3) / 4, 1024)), nclouds), dim3(256), 0, s, d_xyz, d_sp_off, d_sp_pts, d_sel, d_coff, nsingle, d_centres, P);
    return SSDR_OK;
}
// one scratch set per stream: calls on different streams may run concurrently (include/ssdr_al.h)
SelState& sst(hipStream_t st = nullptr) { return per_stream<SelState>(st); }

}  // namespace
}  // namespace ssdr

using namespace ssdr;

extern "C" {

int ssdr_point_uncertainty_dev(const float* d_probs, size_t n, int num_classes, int mode, float* d_unc, int32_t* d_cls, void* stream) {
    if (!d_probs || !d_unc || !d_cls || num_classes < 2 || num_classes > 128 || mode < 0 || mode > 2) { set_error("point_uncertainty: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (n == 0) return SSDR_OK;
    ProfScope prof("sel_point_unc", pick_stream(stream), (4.0 * num_classes + 8.0) * (double)n);
    hipLaunchKernelGGL(sel_point_unc, dim3(grid_for((long)n)), dim3(256), 0, pick_stream(stream), d_probs, (int)n, num_classes, mode, d_unc, d_cls);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_region_stats_dev(const float* d_unc, const int32_t* d_cls, const int32_t* d_sp_off, const int32_t* d_sp_pts, size_t S, int num_classes,
                          int mode, double* d_region_unc, int32_t* d_dom, int32_t* d_dom_cnt, void* stream) {
    if (!d_unc || !d_cls || !d_sp_off || !d_sp_pts || !d_region_unc || !d_dom || !d_dom_cnt || num_classes > 32 || mode < 0 || mode > 2) { set_error("region_stats: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (S == 0) return SSDR_OK;
    ProfScope prof("sel_region_stats", pick_stream(stream), 0.0);
    hipLaunchKernelGGL(sel_region_stats_w, dim3((unsigned)std::min<size_t>((S + 3) / 4, (size_t)ctx().num_cu * 16)), dim3(256), 0, pick_stream(stream), d_unc, d_cls, d_sp_off, d_sp_pts,
                       (int)S, num_classes, mode, d_region_unc, d_dom, d_dom_cnt);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_dominant_label_dev(const int32_t* d_labels, const int32_t* d_sp_off, const int32_t* d_sp_pts, size_t S, int num_labels,
                            int32_t* d_label, double* d_purity, void* stream) {
    if (!d_labels || !d_sp_off || !d_sp_pts || !d_label || !d_purity || num_labels < 1 || num_labels > 64) { set_error("dominant_label: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (S == 0) return SSDR_OK;
    hipStream_t s = pick_stream(stream); SelState& Q = sst(s);
    SSDR_TRY(Q.hist.reserve(4 * 64)); SSDR_HIP(hipMemsetAsync(Q.hist.p, 0, 4, s));
    ProfScope prof("sel_dominant_label", s, 0.0);
    hipLaunchKernelGGL(sel_dominant_label, dim3((unsigned)std::min<size_t>((S + 3) / 4, (size_t)ctx().num_cu * 16)), dim3(256), 0, s, d_labels, d_sp_off, d_sp_pts, (int)S, num_labels, d_label, d_purity, Q.hist.as<int>());
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_clsbal_dev(const int32_t* d_region_class, size_t S, const uint8_t* d_skip, const int32_t* d_selected_class_list, size_t n_selected, double* d_region_unc, void* stream) {
    if (!d_region_class || !d_region_unc || (n_selected && !d_selected_class_list)) { set_error("clsbal: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (S == 0) return SSDR_OK;
    hipStream_t s = pick_stream(stream); SelState& Q = sst(s);
    SSDR_TRY(Q.hist.reserve(4 * 64)); SSDR_HIP(hipMemsetAsync(Q.hist.p, 0, 4 * 64, s));
    ProfScope prof("sel_clsbal", s, 0.0);
    hipLaunchKernelGGL(sel_class_hist, dim3(grid_for((long)(S + n_selected))), dim3(256), 0, s, d_region_class, (int)S, d_skip, d_selected_class_list, (int)n_selected, Q.hist.as<int>());
    hipLaunchKernelGGL(sel_clsbal, dim3(grid_for((long)S)), dim3(256), 0, s, d_region_class, (int)S, d_skip ? -1 : (int)(S + n_selected), Q.hist.as<int>(), d_region_unc);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

/* multi-GPU flavour of add_clsbal: the class histogram is supplied (all-reduced by the caller) */
int ssdr_class_hist_dev(const int32_t* d_region_class, size_t S, const uint8_t* d_skip, const int32_t* d_selected_class_list, size_t n_selected, int32_t* d_hist64, void* stream) {
    if (!d_region_class || !d_hist64 || (n_selected && !d_selected_class_list)) { set_error("class_hist: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    SSDR_HIP(hipMemsetAsync(d_hist64, 0, 4 * 64, s));
    if (S + n_selected == 0) return SSDR_OK;
    hipLaunchKernelGGL(sel_class_hist, dim3(grid_for((long)(S + n_selected))), dim3(256), 0, s, d_region_class, (int)S, d_skip, d_selected_class_list, (int)n_selected, d_hist64);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}
int ssdr_clsbal_hist_dev(const int32_t* d_region_class, size_t S, const int32_t* d_hist64, size_t total, double* d_region_unc, void* stream) {
    if (!d_region_class || !d_hist64 || !d_region_unc || total == 0) { set_error("clsbal_hist: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (S == 0) return SSDR_OK;
    hipLaunchKernelGGL(sel_clsbal, dim3(grid_for((long)S)), dim3(256), 0, pick_stream(stream), d_region_class, (int)S, (int)total, d_hist64, d_region_unc);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_rank_regions_dev(const double* d_region_unc, size_t S, int32_t* d_sorted_inds, void* stream) {
    if (!d_region_unc || !d_sorted_inds) { set_error("rank_regions: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (S == 0) return SSDR_OK;
    hipStream_t s = pick_stream(stream); SelState& Q = sst(s);
    ProfScope prof("sel_rank", s, 0.0);
    if (S <= (size_t)RANK_SMALL) {
        hipLaunchKernelGGL(sel_rank_count, dim3((unsigned)((S + 31) / 32)), dim3(256), 0, s, d_region_unc, (int)S, d_sorted_inds);
        SSDR_HIP(hipGetLastError());
        return SSDR_OK;
    }
    SSDR_TRY(Q.keys.reserve(8 * S)); SSDR_TRY(Q.vals.reserve(4 * S));
    hipLaunchKernelGGL(sel_rank_keys, dim3(grid_for((long)S)), dim3(256), 0, s, d_region_unc, (int)S, Q.keys.as<uint64_t>(), Q.vals.as<uint32_t>());
    Q.sorter.wide_high = true;       // the keys' high words are the uncertainties' float bits: every pass up there runs
    SSDR_TRY(Q.sorter.sort(Q.keys.as<uint64_t>(), Q.vals.as<uint32_t>(), (int)S, nullptr, s));
    SSDR_HIP(hipMemcpyAsync(d_sorted_inds, Q.vals.p, 4 * S, hipMemcpyDeviceToDevice, s));
    return SSDR_OK;
}

int ssdr_segment_mean_features_dev(const float* d_feat, int feat_dim, const int32_t* d_cls, const int32_t* d_dom, const int32_t* d_sp_off,
                                   const int32_t* d_sp_pts, const int32_t* d_sel, size_t nsel, float* d_out, void* stream) {
    if (!d_feat || !d_cls || !d_dom || !d_sp_off || !d_sp_pts || !d_out || feat_dim < 1) { set_error("segment_mean_features: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (nsel == 0) return SSDR_OK;
    hipLaunchKernelGGL(sel_segment_mean, dim3(grid_for((long)nsel * feat_dim)), dim3(256), 0, pick_stream(stream), d_feat, feat_dim, d_cls, d_dom, d_sp_off, d_sp_pts, d_sel,
                       (int)nsel, d_out);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

// ---- sharded selection: device-side pieces of the exchanges (ssdr_al/distributed.py) -----------------------------------
__global__ __launch_bounds__(256) void sel_mask_regions(const double* __restrict__ u, const unsigned char* __restrict__ labelled, int S, int Spad, double* out) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < Spad; i += gridDim.x * 256)
        out[i] = (i < S && !labelled[i]) ? u[i] : __longlong_as_double((long long)0xfff0000000000000ULL);      // -inf: labelled regions and padding sort last
}
__global__ __launch_bounds__(256) void sel_gather_rows(const uint32_t* __restrict__ in, const int* __restrict__ idx, int n, int row_words, uint32_t* __restrict__ out,
                                                       const int* __restrict__ dn = nullptr) {
    if (dn) n = min(n, *dn);
    const long total = (long)n * row_words;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int r = (int)(e / row_words), c = (int)(e % row_words);
        out[e] = in[(size_t)idx[r] * row_words + c];
    }
}

int ssdr_mask_regions_dev(const double* d_region_unc, const uint8_t* d_labelled, size_t S, size_t S_padded, double* d_out, void* stream) {
    if (!d_region_unc || !d_labelled || !d_out || S_padded < S) { set_error("mask_regions: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (S_padded == 0) return SSDR_OK;
    hipLaunchKernelGGL(sel_mask_regions, dim3(grid_for((long)S_padded)), dim3(256), 0, pick_stream(stream), d_region_unc, d_labelled, (int)S, (int)S_padded, d_out);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_gather_rows_dev(const void* d_in, const int32_t* d_idx, size_t n, size_t row_bytes, void* d_out, void* stream) {
    if (!d_in || !d_idx || !d_out || row_bytes % 4) { set_error("gather_rows: bad arguments (row_bytes must be a multiple of 4)"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (n == 0) return SSDR_OK;
    hipLaunchKernelGGL(sel_gather_rows, dim3(grid_for((long)n * (long)(row_bytes / 4))), dim3(256), 0, pick_stream(stream), (const uint32_t*)d_in, d_idx, (int)n,
                       (int)(row_bytes / 4), (uint32_t*)d_out);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_widen_f32_f64_dev(const float* d_x, size_t n, double* d_y0, double* d_y1, void* stream) {
    if (!d_x || !d_y0) { set_error("widen_f32_f64: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (n == 0) return SSDR_OK;
    hipLaunchKernelGGL(widen_f32_f64, dim3(grid_for((long)n)), dim3(256), 0, pick_stream(stream), d_x, n, d_y0, d_y1);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_cloud_graph_dev(const float* d_xyz, const int32_t* d_sp_off, const int32_t* d_sp_pts, const int32_t* d_sel, size_t nsel, size_t max_sp_size,
                         int gcn_top, double* d_centres, double* d_cd_dir, double* d_adj, void* stream) {
    if (!d_xyz || !d_sp_off || !d_sp_pts || !d_sel || !d_centres || !d_cd_dir || !d_adj || max_sp_size == 0) { set_error("cloud_graph: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (nsel == 0) return SSDR_OK;
    hipStream_t s = pick_stream(stream); SelState& Q = sst(s);
    const int n = (int)nsel;
    SSDR_TRY(Q.rowsum.reserve(8 * nsel));
    ChamferPack P; SSDR_TRY(chamfer_pack_buffers(Q, nsel, 1, P));
    SSDR_TRY(chamfer_pack_launch(P, d_xyz, d_sp_off, d_sp_pts, d_sel, nullptr, n, nsel, n, 1, d_centres, s));
    SSDR_TRY(chamfer_dir_launch(d_xyz, d_sp_off, d_sp_pts, d_sel, n, d_centres, d_cd_dir, P, s));
    hipLaunchKernelGGL(sel_adj_build, dim3(std::min(n, 2048)), dim3(256), 0, s, d_centres, d_cd_dir, n, d_adj, Q.rowsum.as<double>());
    hipLaunchKernelGGL(sel_adj_norm, dim3(grid_for((long)n * n)), dim3(256), 0, s, Q.rowsum.as<double>(), n, d_adj);
    if (gcn_top > 0) hipLaunchKernelGGL(sel_adj_topk, dim3(std::max(1, std::min((n + 3) / 4, 2048))), dim3(256), 0, s, d_adj, n, gcn_top);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_cloud_graph_batch_dev(const float* d_xyz, const int32_t* d_sp_off, const int32_t* d_sp_pts, const int32_t* d_sel, const int32_t* d_coff,
                               const int64_t* d_boff, size_t num_clouds, size_t n_total, size_t n_max, int gcn_top,
                               double* d_centres, double* d_cd_dir, double* d_adj, void* stream) {
    if (!d_xyz || !d_sp_off || !d_sp_pts || !d_sel || !d_coff || !d_boff || !d_centres || !d_cd_dir || !d_adj || num_clouds > 65535) { set_error("cloud_graph_batch: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (num_clouds == 0 || n_total == 0 || n_max == 0) return SSDR_OK;
    hipStream_t s = pick_stream(stream); SelState& Q = sst(s);
    const int nm = (int)n_max; const unsigned nc = (unsigned)num_clouds;
    SSDR_TRY(Q.rowsum.reserve(8 * n_total));
    ChamferPack P; SSDR_TRY(chamfer_pack_buffers(Q, n_total, num_clouds, P));
    SSDR_TRY(chamfer_pack_launch(P, d_xyz, d_sp_off, d_sp_pts, d_sel, d_coff, 0, n_total, nm, nc, d_centres, s));
    SSDR_TRY(chamfer_dir_batch_launch(d_xyz, d_sp_off, d_sp_pts, d_sel, d_coff, (const long long*)d_boff, nm, nc, d_centres, d_cd_dir, P, s));
    hipLaunchKernelGGL(sel_adj_build_batch, dim3(std::min(nm, 1024), 1, nc), dim3(256), 0, s, d_centres, d_cd_dir, d_coff, (const long long*)d_boff, d_adj, Q.rowsum.as<double>());
    hipLaunchKernelGGL(sel_adj_norm_batch, dim3(grid_for((long)nm * nm, 256), 1, nc), dim3(256), 0, s, Q.rowsum.as<double>(), d_coff, (const long long*)d_boff, d_adj);
    if (gcn_top > 0) hipLaunchKernelGGL(sel_adj_topk_batch, dim3(std::max(1, std::min((nm + 3) / 4, 1024)), 1, nc), dim3(256), 0, s, d_adj, d_coff, (const long long*)d_boff, gcn_top);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_propagate_batch_dev(const double* d_adj, const int32_t* d_coff, const int64_t* d_boff, size_t num_clouds, size_t n_max, const int32_t* d_rows,
                             const double* d_vin, int feat_dim, double* d_vout, double* d_comb, void* stream) {
    if (!d_adj || !d_coff || !d_boff || !d_rows || !d_vin || !d_vout || !d_comb || feat_dim < 1 || num_clouds > 65535) { set_error("propagate_batch: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (num_clouds == 0 || n_max == 0) return SSDR_OK;
    hipLaunchKernelGGL(sel_propagate_batch, dim3(grid_for((long)n_max * feat_dim, 256), 1, (unsigned)num_clouds), dim3(256), 0, pick_stream(stream), d_adj, d_coff,
                       (const long long*)d_boff, d_rows, d_vin, feat_dim, d_vout, d_comb);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_propagate_dev(const double* d_adj, size_t n, const int32_t* d_rows, const double* d_vin, int feat_dim, double* d_vout, double* d_comb, void* stream) {
    if (!d_adj || !d_rows || !d_vin || !d_vout || !d_comb || feat_dim < 1) { set_error("propagate: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (n == 0) return SSDR_OK;
    hipLaunchKernelGGL(sel_propagate, dim3(grid_for((long)n * feat_dim)), dim3(256), 0, pick_stream(stream), d_adj, (int)n, d_rows, d_vin, feat_dim, d_vout, d_comb);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

/* gcn.create_adj (gcn.py:116-191): the adjacency the trained-GCN branch feeds its graph convolutions and the k-center step, torch float32 in the
 * reference.  d_feat [N,F] float32 = concatenate(unlabelled candidates, labelled regions) (gcn.py:199); the clouds' bbox centres and directed
 * chamfer means come from ssdr_cloud_graph_batch_dev (same d_coff / d_boff), d_rows [N] gives, cloud by cloud, the row of every member in the
 * result.  Outputs: d_out_v [N,F] (the normalised features the function returns) and d_out_adj [N,N] = (cos * exp(-(ED + CD)) - I) D^-1 + I. */
int ssdr_create_adj_dev(const float* d_feat, size_t N, int F, const double* d_centres, const double* d_cd_dir, const int32_t* d_coff, const int64_t* d_boff,
                        size_t num_clouds, size_t n_max, const int32_t* d_rows, float* d_out_v, float* d_out_adj, void* stream) {
    if (!d_feat || !d_centres || !d_cd_dir || !d_coff || !d_boff || !d_rows || !d_out_v || !d_out_adj || N == 0 || F < 1 || num_clouds == 0 || N > 0x7fff) { set_error("create_adj: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); SelState& Q = sst(s);
    SSDR_TRY(Q.rowsum.reserve(8 * N));
    SSDR_HIP(hipMemsetAsync(d_out_adj, 0, 4 * N * N, s));
    hipLaunchKernelGGL(ca_normalize, dim3(grid_for((long)N * 64)), dim3(256), 0, s, d_feat, (int)N, F, d_out_v);
    hipLaunchKernelGGL(ca_block, dim3(grid_for((long)n_max * n_max, 256), 1, (unsigned)num_clouds), dim3(256), 0, s, d_out_v, F, d_centres, d_cd_dir, d_coff, (const long long*)d_boff, d_rows, (int)N, d_out_adj);
    hipLaunchKernelGGL(ca_colsum, dim3(grid_for((long)N)), dim3(256), 0, s, d_out_adj, (int)N, Q.rowsum.as<float>());
    hipLaunchKernelGGL(ca_scale, dim3(grid_for((long)N * N)), dim3(256), 0, s, d_out_adj, (int)N, Q.rowsum.as<float>());
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

}  // extern "C"

// What ssdr_gcn_fps_sampling_dev and ssdr_gcn_sampling_dev share: the candidate rule (four small kernels, cand_*), compute_features of the candidates and
// the labelled regions, the chamfer packer with the bbox centres, and the directed chamfer means — everything up to the adjacency, which differs.
struct SamplingFront { int* counts; int* out; int* sel; int* coff; long long* boff; int* gsel; int* rows; int* already;
                       double* V; double* comb; double* tmp0; double* tmp1; double* cen; double* dir; double* adj; int nm; unsigned nc; };
// feat32 (optional, [cap_rows, 32]): the float32 rows of compute_features next to their widened copies
static int sampling_front(SelState& Q, hipStream_t s, const float* d_feat, int D, const int32_t* d_cls, const int32_t* d_dom, const int32_t* d_lab_cls, const int32_t* d_lab_dom,
                          const float* d_xyz, const int32_t* d_sp_off, const int32_t* d_sp_pts, const int32_t* d_order, size_t S, const uint8_t* d_labelled, const int32_t* d_sp_base,
                          size_t num_clouds, const int32_t* d_lab_off, const int32_t* d_lab_sp, size_t n_lab, size_t batch_size, size_t cap_rows, size_t cap_nmax, size_t cap_sq,
                          size_t max_select, int32_t* d_result, float* feat32, std::optional<ProfScope>& prof, SamplingFront& R) {
    const int B = (int)num_clouds, nchunks = (int)((S + CR_NT - 1) / CR_NT);
    // ints: rankpos S, cploc S, stage S, chunk nchunks, ncand B, ntop B, uoff B+1, coff B+1, gsel cap, rows cap | int64: boff B+1
    const size_t ni = 3 * S + (size_t)nchunks + 4 * (size_t)B + 2 + 2 * cap_rows + n_lab + 16;
    SSDR_TRY(Q.cand_i.reserve(4 * ni + 8 * ((size_t)B + 2)));
    int* rankpos = Q.cand_i.as<int>(); int* cploc = rankpos + S; int* stage = cploc + S; int* chunk = stage + S; int* ncand = chunk + nchunks; int* ntop = ncand + B;
    int* uoff = ntop + B; int* coff = uoff + B + 1; int* gsel = coff + B + 1; int* rows = gsel + cap_rows; int* already = rows + cap_rows;
    long long* boff = reinterpret_cast<long long*>(Q.cand_i.as<char>() + ((4 * ni + 7) & ~(size_t)7));
    // doubles: V, comb, tmp0, tmp1 [cap_rows, D]; centres [cap_rows, 3]; dir, adj [cap_sq]
    SSDR_TRY(Q.cand_f.reserve(8 * (4 * cap_rows * D + 3 * cap_rows + 2 * cap_sq)));
    double* V = Q.cand_f.as<double>(); double* comb = V + cap_rows * D; double* tmp0 = comb + cap_rows * D; double* tmp1 = tmp0 + cap_rows * D;
    double* cen = tmp1 + cap_rows * D; double* dir = cen + 3 * cap_rows; double* adj = dir + cap_sq;
    int* counts = d_result; int* out = d_result + 8; int* sel = out + max_select;
    prof.emplace("sel_candidate_rule", s, 0.0);
    hipLaunchKernelGGL(cand_rank, dim3(nchunks), dim3(CR_NT), 0, s, d_order, (int)S, d_labelled, rankpos, cploc, chunk);
    hipLaunchKernelGGL(cand_chunkscan, dim3(1), dim3(256), 0, s, chunk, nchunks);
    hipLaunchKernelGGL(cand_cloud, dim3(B, cand_slices((size_t)S, (size_t)B)), dim3(256), 0, s, rankpos, cploc, chunk, d_labelled, d_sp_base, (int)S, (int)std::min<size_t>(batch_size, 0x7fffffff), stage, ncand, ntop);
    hipLaunchKernelGGL(cand_layout, dim3(1), dim3(256), 0, s, ncand, ntop, d_lab_off, B, (long long)cap_rows, (long long)cap_sq, uoff, coff, boff, counts);
    hipLaunchKernelGGL(cand_fill, dim3(B), dim3(256), 0, s, stage, d_sp_base, ncand, uoff, coff, d_lab_off, d_lab_sp, counts, sel, gsel, rows, already);
    const int nt = (int)cap_rows, nm = (int)cap_nmax; const unsigned nc = (unsigned)B;
    prof.emplace("sel_features_pack", s, 0.0);
    // compute_features (sampler2.py:333,339) of the refs, widened; bbox centres of the grouped rows
    hipLaunchKernelGGL(sel_segment_mean, dim3(grid_for((long)nt * D)), dim3(256), 0, s, d_feat, D, d_cls, d_dom, d_sp_off, d_sp_pts, sel, nt, feat32, counts + 2, V, comb,
                       d_lab_cls, d_lab_dom, counts);
    SSDR_TRY(Q.rowsum.reserve(8 * cap_rows));
    ChamferPack P; SSDR_TRY(chamfer_pack_buffers(Q, cap_rows, num_clouds, P));
    SSDR_TRY(chamfer_pack_launch(P, d_xyz, d_sp_off, d_sp_pts, gsel, coff, 0, cap_rows, nm, nc, cen, s));
    prof.emplace("sel_chamfer", s, 0.0);          // (pairs of points: the counts are the device's; bench.py derives the FLOPs from the result)
    SSDR_TRY(chamfer_dir_batch_launch(d_xyz, d_sp_off, d_sp_pts, gsel, coff, boff, nm, nc, cen, dir, P, s));
    R = SamplingFront{counts, out, sel, coff, boff, gsel, rows, already, V, comb, tmp0, tmp1, cen, dir, adj, nm, nc};
    return SSDR_OK;
}

extern "C" {
/* GCN_FPS_sampling (sampler2.py:313-342, :736-781) behind the candidate rule of its caller (sampler2.py:533-552, :745-753), with no host decision in
 * between: ranking in, selected candidates out.  The candidate rule runs as four small kernels (cand_*); the row counts it finds stay on the device and
 * every kernel behind it (features, bbox centres, chamfer packer, chamfer, adjacency, keep-top mask, propagation hops, FPS) reads them there, its launch
 * shape chosen by the caller's capacities.  d_result: [0..7] counts (n_unl, n_lab, ntot, nmax, sampling_batch, status, block elements as int64),
 * [8 .. 8+max_select) the selected candidates (indices into the candidate list), [8+max_select .. +cap_rows) the candidate list followed by the labelled
 * regions (superpoint ids; the first n_unl are the candidates, cloud by cloud, descending uncertainty inside a cloud). */
int ssdr_gcn_fps_sampling_dev(const float* d_feat, int feat_dim, const int32_t* d_cls, const int32_t* d_dom, const int32_t* d_lab_cls, const int32_t* d_lab_dom,
                              const float* d_xyz, const int32_t* d_sp_off, const int32_t* d_sp_pts, const int32_t* d_order, size_t S, const uint8_t* d_labelled, const int32_t* d_sp_base, size_t num_clouds,
                              const int32_t* d_lab_off, const int32_t* d_lab_sp, size_t n_lab, size_t batch_size, int gcn_number, int gcn_top, int selector, int start,
                              size_t cap_rows, size_t cap_nmax, size_t cap_sq, size_t cap_unl, size_t max_select, int32_t* d_result, void* stream) {
    if (!d_feat || !d_cls || !d_dom || (!d_lab_cls != !d_lab_dom) || !d_xyz || !d_sp_off || !d_sp_pts || !d_order || !d_labelled || !d_sp_base || !d_lab_off || !d_result || feat_dim != 32 ||
        num_clouds == 0 || num_clouds > 65535 || S == 0 || S > 0x7ffffff0 || cap_rows == 0 || cap_nmax == 0 || cap_sq == 0 || cap_unl == 0 || cap_rows > (1u << 22) || gcn_number < 0 || start < 0 || selector < 0 || selector > 1 || (selector == 1 && n_lab == 0) || (n_lab && !d_lab_sp)) {
        set_error("gcn_fps_sampling: bad arguments (feat_dim == 32, at most 2^22 candidate + labelled rows, at most 65535 clouds, k-center needs labelled regions)"); return SSDR_ERR_INVALID;
    }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); SelState& Q = sst(s);
    const int D = feat_dim;
    std::optional<ProfScope> prof; SamplingFront R;
    SSDR_TRY(sampling_front(Q, s, d_feat, D, d_cls, d_dom, d_lab_cls, d_lab_dom, d_xyz, d_sp_off, d_sp_pts, d_order, S, d_labelled, d_sp_base, num_clouds, d_lab_off, d_lab_sp, n_lab,
                            batch_size, cap_rows, cap_nmax, cap_sq, max_select, d_result, nullptr, prof, R));
    Q.last_comb = R.comb; Q.last_cap = cap_rows;
    const int nm = R.nm; const unsigned nc = R.nc;
    prof.emplace("sel_adjacency_propagate", s, 0.0);
    hipLaunchKernelGGL(sel_adj_build_batch, dim3(std::min(nm, 1024), 1, nc), dim3(256), 0, s, R.cen, R.dir, R.coff, R.boff, R.adj, Q.rowsum.as<double>());
    hipLaunchKernelGGL(sel_adj_norm_batch, dim3(grid_for((long)nm * nm, 256), 1, nc), dim3(256), 0, s, Q.rowsum.as<double>(), R.coff, R.boff, R.adj);
    if (gcn_top > 0) hipLaunchKernelGGL(sel_adj_topk_batch, dim3(std::max(1, std::min((nm + 3) / 4, 1024)), 1, nc), dim3(256), 0, s, R.adj, R.coff, R.boff, gcn_top);
    const double* src = R.V;
    for (int hop = 0; hop < gcn_number; ++hop) {
        double* dst = (hop & 1) ? R.tmp1 : R.tmp0;
        hipLaunchKernelGGL(sel_propagate_batch, dim3(grid_for((long)nm * D, 256), 1, nc), dim3(256), 0, s, R.adj, R.coff, R.boff, R.rows, src, D, dst, R.comb);
        src = dst;
    }
    SSDR_HIP(hipGetLastError());
    prof.reset();
    if (max_select == 0) return SSDR_OK;
    // selector 1: kCenterGreedy over candidates + labelled rows, seeded with the labelled ones (kcenterGreedy.py:84-128; sampler2.py's "kcenter" branch)
    if (selector == 1) return fps_like(R.comb, cap_rows, D, R.already, n_lab, 0, max_select, 1, R.out, s, R.counts + 2);
    return fps_like(R.comb, cap_unl, D, nullptr, 0, start, max_select, 0, R.out, s, R.counts);
}

/* sampling()'s "gcn" branch (sampler2.py:687-734 -> gcn.py:193-263) behind the same candidate rule, features, bbox centres and chamfer means: block
 * adjacency -> Adam training of the two-layer GCN -> evaluation -> kCenterGreedy over the 129-d rows, seeded with the labelled ones (select_gcn.hip). */
int ssdr_gcn_sampling_dev(const float* d_feat, int feat_dim, const int32_t* d_cls, const int32_t* d_dom, const int32_t* d_lab_cls, const int32_t* d_lab_dom,
                          const float* d_xyz, const int32_t* d_sp_off, const int32_t* d_sp_pts, const int32_t* d_order, size_t S, const uint8_t* d_labelled, const int32_t* d_sp_base, size_t num_clouds,
                          const int32_t* d_lab_off, const int32_t* d_lab_sp, size_t n_lab, size_t batch_size, const float* d_init, int steps, float p, float lr, float weight_decay,
                          float lamda, uint64_t seed, int form, size_t cap_rows, size_t cap_nmax, size_t cap_sq, size_t cap_unl, size_t max_select, int32_t* d_result, void* stream) {
    if (!d_feat || !d_cls || !d_dom || (!d_lab_cls != !d_lab_dom) || !d_xyz || !d_sp_off || !d_sp_pts || !d_order || !d_labelled || !d_sp_base || !d_lab_off || !d_result || !d_init || feat_dim != 32 ||
        num_clouds == 0 || num_clouds > 65535 || S == 0 || S > 0x7ffffff0 || cap_rows == 0 || cap_nmax == 0 || cap_sq == 0 || cap_unl == 0 || cap_rows > (1u << 22) || steps < 0 || (n_lab && !d_lab_sp)) {
        set_error("gcn_sampling: bad arguments (feat_dim == 32, at most 2^22 candidate + labelled rows, at most 65535 clouds)"); return SSDR_ERR_INVALID;
    }
    if (form == SSDR_GCN_FORM_FUSED && cap_nmax > (size_t)SSDR_GCN_FUSED_CAP) { set_error("gcn_sampling: the fused form holds blocks of at most %d rows (cap_nmax = %zu)", SSDR_GCN_FUSED_CAP, cap_nmax); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); SelState& Q = sst(s);
    GcnChainBufs G; SSDR_TRY(gcn_chain_buffers(s, cap_rows, cap_sq, G));
    std::optional<ProfScope> prof; SamplingFront R;
    SSDR_TRY(sampling_front(Q, s, d_feat, feat_dim, d_cls, d_dom, d_lab_cls, d_lab_dom, d_xyz, d_sp_off, d_sp_pts, d_order, S, d_labelled, d_sp_base, num_clouds, d_lab_off, d_lab_sp, n_lab,
                            batch_size, cap_rows, cap_nmax, cap_sq, max_select, d_result, G.feat, prof, R));
    prof.emplace("sel_gcn_train", s, 0.0);
    int* rowcloud = G.info + 8;
    SSDR_TRY(ssdr_gcn_block_adj_dev(G.feat, cap_rows, 32, R.cen, R.dir, R.coff, (const int64_t*)R.boff, num_clouds, cap_nmax, R.rows, R.counts, G.v, G.adj, G.adjT, rowcloud, G.info, s));
    SSDR_TRY(ssdr_gcn_train_dev(G.v, G.adj, G.adjT, R.coff, (const int64_t*)R.boff, num_clouds, cap_nmax, R.rows, rowcloud, R.counts, cap_rows, d_init, G.params, steps, p, lr, weight_decay,
                                lamda, seed, form, G.loss, G.info, s));
    SSDR_TRY(ssdr_gcn_eval_dev(G.v, G.adj, G.adjT, R.coff, (const int64_t*)R.boff, num_clouds, cap_nmax, R.rows, rowcloud, R.counts, cap_rows, G.params, G.rows129, G.info, s));
    SSDR_TRY(gcn_merge_status(G.info, R.counts, s));
    prof.reset();
    if (max_select == 0 || n_lab == 0) return SSDR_OK;
    return fps_like(G.rows129, cap_rows, 129, R.already, n_lab, 0, max_select, 1, R.out, s, R.counts + 2);
}

/* The propagated rows of the last ssdr_gcn_fps_sampling_dev call on `stream` (device pointer, [cap_rows][32] float64: the candidates first, then the labelled
 * regions — sum_i A^i V of fps_gcn_cpu.py:162-167, what its FPS / k-center ran over).  Valid until the next selection call on that stream. */
int ssdr_gcn_fps_sampling_rows(void* stream, const double** d_rows, size_t* cap_rows) {
    if (!d_rows) { set_error("gcn_fps_sampling_rows: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    SelState& Q = sst(pick_stream(stream));
    if (!Q.last_comb) { set_error("gcn_fps_sampling_rows: no ssdr_gcn_fps_sampling_dev call on this stream yet"); return SSDR_ERR_INVALID; }
    *d_rows = Q.last_comb; if (cap_rows) *cap_rows = Q.last_cap;
    return SSDR_OK;
}

/* The sharded run's selection without a host decision: two enqueue-only calls around the all-gather of the candidates' propagated features (exchange 3).
 * ssdr_gcn_fps_sharded_local_dev: the candidate rule over the GLOBAL ranking (d_gorder over Sg = world * Smax padded region ids, d_glabelled != 0 for
 * labelled regions and padding, global cloud c = rank * Bmax + b spans d_gbase[c] .. d_gbase[c+1]-1), then this rank's share of GCN_FPS_sampling (features,
 * chamfer graph, adjacency, propagation) for its own clouds.  d_comb_out [nu_max, 32]: its candidates' propagated features in candidate order (what the
 * all-gather sends); d_plan (int32, 16 + world + 2 * world * nu_max words): counts, candidates per rank, the rows of the gathered array in global candidate
 * order, the global candidate list.  ssdr_fps_gathered_dev: compacts the gathered array by the plan and runs the replicated global FPS from candidate `start`. */
int ssdr_gcn_fps_sharded_local_dev(const float* d_feat, int feat_dim, const int32_t* d_cls, const int32_t* d_dom, const int32_t* d_lab_cls, const int32_t* d_lab_dom,
                                   const float* d_xyz, const int32_t* d_sp_off, const int32_t* d_sp_pts, const int32_t* d_lab_off, const int32_t* d_lab_sp, size_t n_lab, size_t num_clouds,
                                   const int32_t* d_gorder, size_t Sg, const uint8_t* d_glabelled, const int32_t* d_gbase, int rank, int world, size_t Smax, size_t Bmax,
                                   size_t batch_size, int gcn_number, int gcn_top, size_t cap_rows, size_t cap_nmax, size_t cap_sq, size_t nu_max, size_t nl_max,
                                   double* d_comb_out, int32_t* d_plan, void* stream) {
    if (!d_feat || !d_cls || !d_dom || (!d_lab_cls != !d_lab_dom) || !d_xyz || !d_sp_off || !d_sp_pts || !d_lab_off || !d_gorder || !d_glabelled || !d_gbase || !d_comb_out || !d_plan || feat_dim != 32 ||
        world < 1 || world > 64 || rank < 0 || rank >= world || num_clouds == 0 || num_clouds > Bmax || Bmax * (size_t)world > 65535 || Sg != Smax * (size_t)world || Sg > 0x7ffffff0 ||
        cap_rows == 0 || cap_nmax == 0 || cap_sq == 0 || nu_max == 0 || gcn_number < 0 || (n_lab && !d_lab_sp) || (nl_max && n_lab > nl_max)) {
        set_error("gcn_fps_sharded_local: bad arguments (feat_dim == 32, world <= 64, Sg == world * Smax, n_lab <= nl_max)"); return SSDR_ERR_INVALID;
    }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); SelState& Q = sst(s);
    const int W = world, Bg = (int)(Bmax * (size_t)world), B = (int)num_clouds, nchunks = (int)((Sg + CR_NT - 1) / CR_NT), D = feat_dim;
    const size_t ni = 3 * Sg + (size_t)nchunks + 3 * (size_t)Bg + 2 * (size_t)B + 8 + 3 * cap_rows + 16;
    SSDR_TRY(Q.cand_i.reserve(4 * ni + 8 * ((size_t)B + 2)));
    int* rankpos = Q.cand_i.as<int>(); int* cploc = rankpos + Sg; int* stage = cploc + Sg; int* chunk = stage + Sg; int* ncand = chunk + nchunks; int* ntop = ncand + Bg;
    int* guoff = ntop + Bg; int* uoff = guoff + Bg + 1; int* coff = uoff + B + 1; int* gsel = coff + B + 1; int* rows = gsel + cap_rows; int* sel = rows + cap_rows;
    long long* boff = reinterpret_cast<long long*>(Q.cand_i.as<char>() + ((4 * ni + 7) & ~(size_t)7));
    SSDR_TRY(Q.cand_f.reserve(8 * (4 * cap_rows * D + 3 * cap_rows + 2 * cap_sq)));
    double* V = Q.cand_f.as<double>(); double* comb = V + cap_rows * D; double* tmp0 = comb + cap_rows * D; double* tmp1 = tmp0 + cap_rows * D;
    double* cen = tmp1 + cap_rows * D; double* dir = cen + 3 * cap_rows; double* adj = dir + cap_sq;
    int* plan = d_plan;
    std::optional<ProfScope> prof; prof.emplace("sel_candidate_rule", s, 0.0);
    hipLaunchKernelGGL(cand_rank, dim3(nchunks), dim3(CR_NT), 0, s, d_gorder, (int)Sg, d_glabelled, rankpos, cploc, chunk);
    hipLaunchKernelGGL(cand_chunkscan, dim3(1), dim3(256), 0, s, chunk, nchunks);
    hipLaunchKernelGGL(cand_cloud, dim3(Bg, cand_slices((size_t)Sg, (size_t)Bg)), dim3(256), 0, s, rankpos, cploc, chunk, d_glabelled, d_gbase, (int)Sg, (int)std::min<size_t>(batch_size, 0x7fffffff), stage, ncand, ntop);
    // this rank's clouds: the layout every kernel below reads (counts in plan[0..7]); then what the other ranks contribute
    hipLaunchKernelGGL(cand_layout, dim3(1), dim3(256), 0, s, ncand + (size_t)rank * Bmax, ntop + (size_t)rank * Bmax, d_lab_off, B, (long long)cap_rows, (long long)cap_sq, uoff, coff, boff, plan);
    hipLaunchKernelGGL(cand_global, dim3(1), dim3(256), 0, s, ncand, ntop, W, (int)Bmax, (int)nu_max, guoff, plan);
    hipLaunchKernelGGL(cand_fill_global, dim3(Bg), dim3(256), 0, s, stage, d_gbase, ncand, guoff, plan, plan + 16 + W + (size_t)W * nu_max);
    hipLaunchKernelGGL(cand_fill_local, dim3(B), dim3(256), 0, s, stage, d_gbase + (size_t)rank * Bmax, ncand + (size_t)rank * Bmax, uoff, coff, d_lab_off, d_lab_sp, plan,
                       (int)((size_t)rank * Smax), sel, gsel, rows);
    const int nt = (int)cap_rows, nm = (int)cap_nmax; const unsigned nc = (unsigned)B;
    prof.emplace("sel_features_pack", s, 0.0);
    hipLaunchKernelGGL(sel_segment_mean, dim3(grid_for((long)nt * D)), dim3(256), 0, s, d_feat, D, d_cls, d_dom, d_sp_off, d_sp_pts, sel, nt, (float*)nullptr, plan + 2, V, comb,
                       d_lab_cls, d_lab_dom, plan);
    SSDR_TRY(Q.rowsum.reserve(8 * cap_rows));
    ChamferPack P; SSDR_TRY(chamfer_pack_buffers(Q, cap_rows, num_clouds, P));
    SSDR_TRY(chamfer_pack_launch(P, d_xyz, d_sp_off, d_sp_pts, gsel, coff, 0, cap_rows, nm, nc, cen, s));
    prof.emplace("sel_chamfer", s, 0.0);          // (pairs of points: the counts are the device's; bench.py derives the FLOPs from the result)
    SSDR_TRY(chamfer_dir_batch_launch(d_xyz, d_sp_off, d_sp_pts, gsel, coff, boff, nm, nc, cen, dir, P, s));
    prof.emplace("sel_adjacency_propagate", s, 0.0);
    hipLaunchKernelGGL(sel_adj_build_batch, dim3(std::min(nm, 1024), 1, nc), dim3(256), 0, s, cen, dir, coff, boff, adj, Q.rowsum.as<double>());
    hipLaunchKernelGGL(sel_adj_norm_batch, dim3(grid_for((long)nm * nm, 256), 1, nc), dim3(256), 0, s, Q.rowsum.as<double>(), coff, boff, adj);
    if (gcn_top > 0) hipLaunchKernelGGL(sel_adj_topk_batch, dim3(std::max(1, std::min((nm + 3) / 4, 1024)), 1, nc), dim3(256), 0, s, adj, coff, boff, gcn_top);
    const double* src = V;
    for (int hop = 0; hop < gcn_number; ++hop) {
        double* dst = (hop & 1) ? tmp1 : tmp0;
        hipLaunchKernelGGL(sel_propagate_batch, dim3(grid_for((long)nm * D, 256), 1, nc), dim3(256), 0, s, adj, coff, boff, rows, src, D, dst, comb);
        src = dst;
    }
    prof.reset();
    // the candidates' rows (the first n_unl of comb) are what the exchange sends
    hipLaunchKernelGGL(copy_rows_dn, dim3(grid_for((long)nu_max * D)), dim3(256), 0, s, comb, d_comb_out, D, (int)nu_max, plan);
    // ... and, for the global k-center (nl_max > 0), this rank's labelled regions' rows behind them
    if (nl_max && n_lab) hipLaunchKernelGGL(copy_rows_from, dim3(grid_for((long)n_lab * D)), dim3(256), 0, s, comb, d_comb_out + nu_max * (size_t)D, D, (int)n_lab, plan);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

/* The replicated global k-center of the sharded run (BASELINE configuration 4; kcenterGreedy.py:84-128 over [candidates | labelled regions of ALL ranks], the labelled
 * ones already selected): d_gathered = the all-gather of every rank's nu_max + nl_max rows (ssdr_gcn_fps_sharded_local_dev with nl_max > 0), d_nlab_off[world + 1] =
 * prefix of the ranks' labelled counts (static: the host knows it), d_glob [cap_rows][32] and d_already [n_lab_total] scratch.  Nothing is read back. */
int ssdr_kcenter_gathered_dev(const double* d_gathered, const int32_t* d_plan, int world, size_t nu_max, size_t nl_max, const int32_t* d_nlab_off, size_t n_lab_total,
                              size_t cap_rows, size_t max_select, double* d_glob, int32_t* d_already, int32_t* d_out, void* stream) {
    if (!d_gathered || !d_plan || !d_glob || !d_out || !d_already || !d_nlab_off || world < 1 || world > 64 || nu_max == 0 || nl_max == 0 || n_lab_total == 0 || cap_rows <= n_lab_total ||
        n_lab_total > (size_t)world * nl_max) { set_error("kcenter_gathered: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (max_select == 0) return SSDR_OK;
    hipStream_t s = pick_stream(stream); SelState& Q = sst(s);
    SSDR_TRY(Q.hist.reserve(64));
    int* nrows = Q.hist.as<int>();
    hipLaunchKernelGGL(sel_gather_kc, dim3(grid_for((long)cap_rows * 64)), dim3(256), 0, s, (const uint32_t*)d_gathered, d_plan, world, (int)nu_max, (int)(nu_max + nl_max), d_nlab_off,
                       (int)cap_rows, 64, (uint32_t*)d_glob, d_already, nrows);
    SSDR_HIP(hipGetLastError());
    return fps_like(d_glob, cap_rows, 32, d_already, n_lab_total, 0, max_select, 1, d_out, s, nrows);
}

int ssdr_fps_gathered_dev(const double* d_gathered, const int32_t* d_plan, int world, size_t nu_max, size_t cap_rows, int repeat, int start, size_t max_select, double* d_glob,
                          int32_t* d_out, void* stream) {
    if (!d_gathered || !d_plan || !d_glob || !d_out || world < 1 || nu_max == 0 || cap_rows == 0 || repeat < 1 || start < 0) { set_error("fps_gathered: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    if (max_select == 0) return SSDR_OK;
    hipStream_t s = pick_stream(stream); SelState& Q = sst(s);
    SSDR_TRY(Q.hist.reserve(64));
    int* nrep = Q.hist.as<int>();
    hipLaunchKernelGGL(sel_gather_rows_rep, dim3(grid_for((long)cap_rows * 64)), dim3(256), 0, s, (const uint32_t*)d_gathered, d_plan + 16 + world, (int)cap_rows, 64, (uint32_t*)d_glob,
                       d_plan + 8, repeat, nrep);
    SSDR_HIP(hipGetLastError());
    return fps_like(d_glob, cap_rows, 32, nullptr, 0, start, max_select, 0, d_out, s, nrep);
}

/* sampling()'s "edcd" branch (sampler2.py:670-685) behind the candidate rule, as one enqueue-only chain: the same candidate rule as the gcn_fps chain with no
 * labelled rows (the branch draws none), the candidates' bbox centres and directed chamfer means, always in float64 (the Semantic3D code's edcd branch
 * uses gcn.chamfer_distance, a float64 KDTree, SSRD_AL_semantic3d/sampler2.py:51-80, whatever its GCN_FPS_sampling uses), then every cloud's
 * farthest_superpoint_sample in one launch (select_region.hip).  The two entry points below differ in their candidate rule only. */
static int edcd_graph_fps(SelState& Q, const float* d_xyz, const int32_t* d_sp_off, const int32_t* d_sp_pts, const int* gsel, const int* coff, const long long* boff,
                          const int* ntop, int B, size_t cap_rows, size_t cap_nmax, size_t max_select, int* ooff, double* cen, double* dir, int32_t* d_result, hipStream_t s) {
    const int nm = (int)cap_nmax; const unsigned nc = (unsigned)B;
    std::optional<ProfScope> prof; prof.emplace("sel_features_pack", s, 0.0);
    ChamferPack P; SSDR_TRY(chamfer_pack_buffers(Q, cap_rows, (size_t)B, P));
    SSDR_TRY(chamfer_pack_launch(P, d_xyz, d_sp_off, d_sp_pts, gsel, coff, 0, cap_rows, nm, nc, cen, s));
    prof.emplace("sel_chamfer", s, 0.0);
    SSDR_TRY(chamfer_dir_batch_launch(d_xyz, d_sp_off, d_sp_pts, gsel, coff, boff, nm, nc, cen, dir, P, s, 0));
    prof.reset();
    SSDR_HIP(hipGetLastError());
    return edcd_fps_launch(cen, dir, coff, boff, ntop, B, nm, (long long)max_select, ooff, d_result + 5, d_result + 8, s);
}

int ssdr_edcd_sampling_dev(const float* d_xyz, const int32_t* d_sp_off, const int32_t* d_sp_pts, const int32_t* d_order, size_t S, const uint8_t* d_labelled,
                           const int32_t* d_sp_base, size_t num_clouds, size_t batch_size, size_t cap_rows, size_t cap_nmax, size_t cap_sq, size_t max_select,
                           int32_t* d_result, void* stream) {
    if (!d_xyz || !d_sp_off || !d_sp_pts || !d_order || !d_labelled || !d_sp_base || !d_result || num_clouds == 0 || num_clouds > 65535 || S == 0 || S > 0x7ffffff0 ||
        cap_rows == 0 || cap_nmax == 0 || cap_sq == 0 || cap_rows > (1u << 22) || max_select > 0x7fffffff) {
        set_error("edcd_sampling: bad arguments (at most 2^22 candidates, at most 65535 clouds)"); return SSDR_ERR_INVALID;
    }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); SelState& Q = sst(s);
    const int B = (int)num_clouds, nchunks = (int)((S + CR_NT - 1) / CR_NT);
    // ints: rankpos S, cploc S, stage S, chunk nchunks, ncand B, ntop B, uoff / coff / lab_off / ooff B+1 each, gsel cap, rows cap | int64: boff B+1
    const size_t ni = 3 * S + (size_t)nchunks + 6 * (size_t)B + 4 + 2 * cap_rows + 16;
    SSDR_TRY(Q.cand_i.reserve(4 * ni + 8 * ((size_t)B + 2)));
    int* rankpos = Q.cand_i.as<int>(); int* cploc = rankpos + S; int* stage = cploc + S; int* chunk = stage + S; int* ncand = chunk + nchunks; int* ntop = ncand + B;
    int* uoff = ntop + B; int* coff = uoff + B + 1; int* lab_off = coff + B + 1; int* ooff = lab_off + B + 1; int* gsel = ooff + B + 1; int* rows = gsel + cap_rows;
    long long* boff = reinterpret_cast<long long*>(Q.cand_i.as<char>() + ((4 * ni + 7) & ~(size_t)7));
    SSDR_TRY(Q.cand_f.reserve(8 * (3 * cap_rows + cap_sq)));
    double* cen = Q.cand_f.as<double>(); double* dir = cen + 3 * cap_rows;
    int* counts = d_result; int* sel = d_result + 8 + max_select;
    SSDR_HIP(hipMemsetAsync(lab_off, 0, 4 * ((size_t)B + 1), s));
    std::optional<ProfScope> prof; prof.emplace("sel_candidate_rule", s, 0.0);
    hipLaunchKernelGGL(cand_rank, dim3(nchunks), dim3(CR_NT), 0, s, d_order, (int)S, d_labelled, rankpos, cploc, chunk);
    hipLaunchKernelGGL(cand_chunkscan, dim3(1), dim3(256), 0, s, chunk, nchunks);
    hipLaunchKernelGGL(cand_cloud, dim3(B, cand_slices(S, (size_t)B)), dim3(256), 0, s, rankpos, cploc, chunk, d_labelled, d_sp_base, (int)S, (int)std::min<size_t>(batch_size, 0x7fffffff), stage, ncand, ntop);
    hipLaunchKernelGGL(cand_layout, dim3(1), dim3(256), 0, s, ncand, ntop, lab_off, B, (long long)cap_rows, (long long)cap_sq, uoff, coff, boff, counts);
    hipLaunchKernelGGL(cand_fill, dim3(B), dim3(256), 0, s, stage, d_sp_base, ncand, uoff, coff, lab_off, (const int*)nullptr, counts, sel, gsel, rows, (int*)nullptr);
    SSDR_HIP(hipGetLastError());
    prof.reset();
    return edcd_graph_fps(Q, d_xyz, d_sp_off, d_sp_pts, gsel, coff, boff, ntop, B, cap_rows, cap_nmax, max_select, ooff, cen, dir, d_result, s);
}

int ssdr_edcd_sampling_sharded_dev(const float* d_xyz, const int32_t* d_sp_off, const int32_t* d_sp_pts, size_t num_clouds, const int32_t* d_gorder, size_t Sg,
                                   const uint8_t* d_glabelled, const int32_t* d_gbase, int rank, int world, size_t Smax, size_t Bmax, size_t batch_size,
                                   size_t cap_rows, size_t cap_nmax, size_t cap_sq, size_t max_select, int32_t* d_result, void* stream) {
    if (!d_xyz || !d_sp_off || !d_sp_pts || !d_gorder || !d_glabelled || !d_gbase || !d_result || world < 1 || world > 64 || rank < 0 || rank >= world || num_clouds == 0 ||
        num_clouds > Bmax || Bmax * (size_t)world > 65535 || Sg != Smax * (size_t)world || Sg > 0x7ffffff0 || cap_rows == 0 || cap_nmax == 0 || cap_sq == 0 ||
        cap_rows > (1u << 22) || max_select > 0x7fffffff) {
        set_error("edcd_sampling_sharded: bad arguments (world <= 64, Sg == world * Smax, at most 2^22 candidates)"); return SSDR_ERR_INVALID;
    }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream); SelState& Q = sst(s);
    const int Bg = (int)(Bmax * (size_t)world), B = (int)num_clouds, nchunks = (int)((Sg + CR_NT - 1) / CR_NT);
    const size_t ni = 3 * Sg + (size_t)nchunks + 2 * (size_t)Bg + 4 * (size_t)B + 4 + 2 * cap_rows + 16;
    SSDR_TRY(Q.cand_i.reserve(4 * ni + 8 * ((size_t)B + 2)));
    int* rankpos = Q.cand_i.as<int>(); int* cploc = rankpos + Sg; int* stage = cploc + Sg; int* chunk = stage + Sg; int* ncand = chunk + nchunks; int* ntop = ncand + Bg;
    int* uoff = ntop + Bg; int* coff = uoff + B + 1; int* lab_off = coff + B + 1; int* ooff = lab_off + B + 1; int* gsel = ooff + B + 1; int* rows = gsel + cap_rows;
    long long* boff = reinterpret_cast<long long*>(Q.cand_i.as<char>() + ((4 * ni + 7) & ~(size_t)7));
    SSDR_TRY(Q.cand_f.reserve(8 * (3 * cap_rows + cap_sq)));
    double* cen = Q.cand_f.as<double>(); double* dir = cen + 3 * cap_rows;
    int* counts = d_result; int* sel = d_result + 8 + max_select;
    const size_t rb = (size_t)rank * Bmax;
    SSDR_HIP(hipMemsetAsync(lab_off, 0, 4 * ((size_t)B + 1), s));
    std::optional<ProfScope> prof; prof.emplace("sel_candidate_rule", s, 0.0);
    hipLaunchKernelGGL(cand_rank, dim3(nchunks), dim3(CR_NT), 0, s, d_gorder, (int)Sg, d_glabelled, rankpos, cploc, chunk);
    hipLaunchKernelGGL(cand_chunkscan, dim3(1), dim3(256), 0, s, chunk, nchunks);
    hipLaunchKernelGGL(cand_cloud, dim3(Bg, cand_slices(Sg, (size_t)Bg)), dim3(256), 0, s, rankpos, cploc, chunk, d_glabelled, d_gbase, (int)Sg, (int)std::min<size_t>(batch_size, 0x7fffffff), stage, ncand, ntop);
    // this rank's clouds: counts[4] = its picks; edcd is per cloud, so nothing of the other ranks is needed
    hipLaunchKernelGGL(cand_layout, dim3(1), dim3(256), 0, s, ncand + rb, ntop + rb, lab_off, B, (long long)cap_rows, (long long)cap_sq, uoff, coff, boff, counts);
    hipLaunchKernelGGL(cand_fill_local, dim3(B), dim3(256), 0, s, stage, d_gbase + rb, ncand + rb, uoff, coff, lab_off, (const int*)nullptr, counts, (int)((size_t)rank * Smax), sel, gsel, rows);
    SSDR_HIP(hipGetLastError());
    prof.reset();
    return edcd_graph_fps(Q, d_xyz, d_sp_off, d_sp_pts, gsel, coff, boff, ntop + rb, B, cap_rows, cap_nmax, max_select, ooff, cen, dir, d_result, s);
}

}
