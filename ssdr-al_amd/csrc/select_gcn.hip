// The trained-GCN selector of one active-learning round for gfx950: gcn.GCN_sampling (S3/gcn.py:193-263) between create_adj and kCenterGreedy —
// block adjacency, the Adam training loop of the two-layer GCN, and the evaluation that writes the 129-d rows the k-center step runs over.
//
// The adjacency is block-diagonal per cloud (entries between clouds are cos * exp(-2e10) = 0), so nothing here forms the [N,N] matrix:
//   P = A V once (A (V W1) = (A V) W1: layer 1 is a row-wise dense layer on P, dW1 = P^T dh);
//   per step, two block mat-vecs on one scalar per row (t = feat W3: x = A t + b3 forward, u = A^T g backward);
//   dL/dx in closed form: -(1 - s) / n_lab on labelled rows, lamda * s / n_unl on unlabelled ones (finite where float32 autograd meets 0 * inf).
// Rows are kept in GROUPED order (cloud by cloud: position g of d_rows names the row in the [unlabelled | labelled] order).  The 4 353 gradient sums
// are float64, per-workgroup partials in a fixed row order and one reduction in workgroup order: no floating-point atomics, same call same bits.
//
// Two forms (ProfScope "gcn_form:<name>"):
//   general  four launches per step: gcn_fwd (rows) -> gcn_mid (rows) -> gcn_bwd (rows, partials) -> gcn_adam (reduction + Adam, the step's last launch)
//   fused    two launches per step: gcn_step_fused (a workgroup owns whole clouds: forward, both mat-vecs, backward, partials) -> gcn_adam.
//            A cloud's t and g vectors live in LDS (2 x 4 bytes a row; 64 KiB would hold 8 192 rows) and the hidden activations are recomputed in
//            the backward pass instead of being stored (32 FMAs a value), so neither LDS nor registers (32 weights + 16 float64 sums a lane,
//            whatever the block) bound the block; what does is the serial work: one workgroup's two mat-vecs over an n x n block are 2 n^2 / 256
//            FMAs a lane, 8 192 at n = 1024 — about the two launch gaps the form saves.  SSDR_GCN_FUSED_CAP = 1024 rows.
// No kernel here waits for another workgroup.
#include "ssdr_internal.hpp"
#include "select_fps.hpp"
#include "select_gcn.hpp"

namespace ssdr {
namespace {

constexpr int GF = 32, GH = SSDR_GCN_NHID, NPARAM = SSDR_GCN_NPARAM, OFF_B1 = GF * GH, OFF_W3 = OFF_B1 + GH, OFF_B3 = OFF_W3 + GH;
constexpr int FUSED_CAP = SSDR_GCN_FUSED_CAP;
constexpr int ST_REFUSED = SSDR_GCN_ST_SINGLETON | SSDR_GCN_ST_NO_LABELLED;

// the dropout decision (include/ssdr_al.h): a function of (seed, step, row in the [unlabelled | labelled] order, hidden unit) alone
__device__ __forceinline__ bool gcn_keep(unsigned long long seed, unsigned step, unsigned row, unsigned k, float p) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)step + 1ull) + 0xD6E8FEB86659FD93ull * ((unsigned long long)row * 128ull + k + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(z >> 40) * (1.0f / 16777216.0f) >= p;
}

__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- block adjacency (gcn.py:177-189 inside every cloud's block; the arithmetic of select.hip's ca_* kernels) ---------------------------------
__global__ __launch_bounds__(256) void gcn_normalize(const float* __restrict__ f, int cap, const int* __restrict__ counts, float* V) {
    const int lane = threadIdx.x & 63, n = min(cap, counts[2]);
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
        float ss = 0.f;
        for (int k = lane; k < GF; k += 64) { const float v = f[(size_t)i * GF + k]; ss += v * v; }
        for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
        const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
        for (int k = lane; k < GF; k += 64) V[(size_t)i * GF + k] = f[(size_t)i * GF + k] * inv;
    }
}
// block[i][j] = <V_i, V_j> * exp(-((float)ED + (float)CD)) - (i == j)
__global__ __launch_bounds__(256) void gcn_adj_block(const float* __restrict__ V, const double* __restrict__ centres, const double* __restrict__ dir,
                                                     const int* __restrict__ coff, const long long* __restrict__ boff, const int* __restrict__ rows, float* adj) {
    const int c = blockIdx.z, r0 = coff[c], nc = coff[c + 1] - r0;
    const double* D = dir + boff[c];
    float* A = adj + boff[c];
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < (long)nc * nc; e += (long)gridDim.x * 256) {
        const int i = (int)(e / nc), j = (int)(e % nc);
        const int gi = rows[r0 + i], gj = rows[r0 + j];
        const double dx = centres[3 * (size_t)(r0 + i)] - centres[3 * (size_t)(r0 + j)], dy = centres[3 * (size_t)(r0 + i) + 1] - centres[3 * (size_t)(r0 + j) + 1],
                     dz = centres[3 * (size_t)(r0 + i) + 2] - centres[3 * (size_t)(r0 + j) + 2];
        const double ed = sqrt((dx * dx + dy * dy) + dz * dz);
        const double cd = i == j ? 0.0 : D[(size_t)i * nc + j] + D[(size_t)j * nc + i];
        float lat = 0.f;
        for (int k = 0; k < GF; ++k) lat += V[(size_t)gi * GF + k] * V[(size_t)gj * GF + k];
        A[e] = lat * expf(-((float)ed + (float)cd)) - (i == j ? 1.0f : 0.0f);
    }
}
// column sums inside the block (rows ascend in the [unlabelled | labelled] order: the order ca_colsum adds the non-zero entries in), columns scaled by
// 1 / sum, plus I; the transpose next to it.  A block of one row has the column sum 0: flagged, left as the identity.
__global__ __launch_bounds__(256) void gcn_adj_scale(const int* __restrict__ coff, const long long* __restrict__ boff, float* adj, float* adjT, int* rowcloud, int* info) {
    const int c = blockIdx.z, r0 = coff[c], nc = coff[c + 1] - r0;
    float* A = adj + boff[c]; float* T = adjT + boff[c];
    if (nc == 1 && blockIdx.x == 0 && threadIdx.x == 0) { atomicOr(&info[0], (int)SSDR_GCN_ST_SINGLETON); atomicMin(&info[1], c); A[0] = 1.0f; T[0] = 1.0f; rowcloud[r0] = c; }
    if (nc <= 1) return;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < nc; j += gridDim.x * 256) {
        float s = 0.f;
        for (int i = 0; i < nc; ++i) s += A[(size_t)i * nc + j];
        const float inv = 1.0f / s;
        for (int i = 0; i < nc; ++i) {
            const float a = A[(size_t)i * nc + j] * inv + (i == j ? 1.0f : 0.0f);
            A[(size_t)i * nc + j] = a; T[(size_t)j * nc + i] = a;
        }
        rowcloud[r0 + j] = c;
    }
}
__global__ void gcn_info_reset(int* info) { if (threadIdx.x < 8) info[threadIdx.x] = threadIdx.x == 1 ? 0x7fffffff : 0; }

// ---- P = A V, once and in float64 (the products of float32 values are exact there: what is left of the reassociation (A V) W1 = A (V W1) is the
// rounding of h itself — a float32 P moved h by ~1e-7 and with it the step at which a ReLU unit of a row switches on, which Adam turns into a
// different trajectory): a wave per row, lanes = 2 column slices x 32 features -----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gcn_prep(const float* __restrict__ V, const float* __restrict__ adj, const int* __restrict__ coff, const long long* __restrict__ boff,
                                                const int* __restrict__ rows, const int* __restrict__ counts, const int* __restrict__ info, double* P, int* flag) {
    const int c = blockIdx.z, r0 = coff[c], nc = coff[c + 1] - r0, lane = threadIdx.x & 63, f = lane & 31, half = lane >> 5;
    if (c == 0 && blockIdx.x == 0 && threadIdx.x == 0 && counts[1] == 0) atomicOr(flag, (int)SSDR_GCN_ST_NO_LABELLED);
    if (info[0] & SSDR_GCN_ST_SINGLETON) return;
    const float* A = adj + boff[c];
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < nc; i += gridDim.x * 4) {
        double acc = 0.0;
        for (int j = half; j < nc; j += 2) acc = fma((double)A[(size_t)i * nc + j], (double)V[(size_t)rows[r0 + j] * GF + f], acc);
        acc += __shfl_xor(acc, 32);
        if (half == 0) P[(size_t)(r0 + i) * GF + f] = acc;
    }
}

// ---- the three row phases, shared by both forms -------------------------------------------------------------------------------------------------
struct GcnArgs {
    const double* P; const float* adj; const float* adjT; const int* coff; const long long* boff; const int* rows; const int* rowcloud; const int* counts; const int* info;
    const float* params; float* feat; float* t; float* x; float* g; double* part;
    float p, scale, lamda; unsigned long long seed; int step, train, cap;
};

// hidden activation of row g, unit k: dropout(relu(P_g W1[:,k] + b1_k))
__device__ __forceinline__ float gcn_hidden(const double* __restrict__ Pg, const float (&w)[GF], float b1k, const GcnArgs& a, int row, int k) {
    double acc = 0.0;
#pragma unroll
    for (int f = 0; f < GF; ++f) acc = fma(Pg[f], (double)w[f], acc);
    const float r = fmaxf((float)(acc + (double)b1k), 0.f);
    if (!a.train || a.p <= 0.f) return r;
    return gcn_keep(a.seed, (unsigned)a.step, (unsigned)row, (unsigned)k, a.p) ? r * a.scale : 0.f;
}

// forward dense layer of the grouped rows [g0, g0 + n): t[l] = sum_k feat[l][k] W3[k] (t indexed from g0), two rows at a time (threads = 2 x 128 units)
__device__ void gcn_fwd_rows(const GcnArgs& a, int g0, int n, const float (&w)[GF], float b1k, float w3k, float* t, float* s_red) {
    const int k = threadIdx.x & 127, half = threadIdx.x >> 7, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int l0 = 0; l0 < n; l0 += 2) {
        const int l = l0 + half; const bool live = l < n;
        float v = 0.f;
        if (live) {
            v = gcn_hidden(a.P + (size_t)(g0 + l) * GF, w, b1k, a, a.rows[g0 + l], k);
            if (a.feat) a.feat[(size_t)(g0 + l) * GH + k] = v;
            v *= w3k;
        }
        v = wave_sum(v);
        if (lane == 0) s_red[wv] = v;
        __syncthreads();
        if (k == 0 && live) t[l] = s_red[2 * half] + s_red[2 * half + 1];
        __syncthreads();
    }
}
// rows l = w, w + nw, .. of one cloud's block: x = A t + b3, s = sigmoid(x), g = dL/dx (t, g indexed inside the block)
__device__ void gcn_mid_rows(const GcnArgs& a, int c, int w, int nw, const float* t, float* g) {
    const int r0 = a.coff[c], nc = a.coff[c + 1] - r0, lane = threadIdx.x & 63, n_unl = a.counts[0], n_lab = a.counts[1];
    const float* A = a.adj + a.boff[c];
    const float b3 = a.params[OFF_B3];
    for (int l = w; l < nc; l += nw) {
        float acc = 0.f;
        for (int j = lane; j < nc; j += 64) acc = fmaf(A[(size_t)l * nc + j], t[j], acc);
        acc = wave_sum(acc);
        if (lane == 0) {
            const float x = acc + b3, s = 1.0f / (1.0f + expf(-x));
            a.x[r0 + l] = x;
            g[l] = a.rows[r0 + l] >= n_unl ? -(1.0f - s) / (float)n_lab : a.lamda * s / (float)n_unl;
        }
    }
}
// backward of the grouped rows [ga, gb): u = A^T g per row (a wave each), dh, and the float64 sums of this workgroup; RECOMP: the hidden
// activations are computed again instead of read (g_lds != nullptr: the block's g vector in LDS, all rows of one cloud)
struct GcnAcc { double w1[16]; double b1, w3, b3; };
template <bool RECOMP>
__device__ void gcn_bwd_rows(const GcnArgs& a, int ga, int gb, const float (&w)[GF], float b1k, float w3k, const float* g_lds, GcnAcc& acc,
                             double (*s_P)[GF], float* s_u, int* s_row) {
    const int k = threadIdx.x & 127, half = threadIdx.x >> 7, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int q0 = ga; q0 < gb; q0 += 4) {
        const int gi = q0 + wv;
        float u = 0.f, gv = 0.f;
        if (gi < gb) {
            const int c = a.rowcloud[gi], r0 = a.coff[c], nc = a.coff[c + 1] - r0, l = gi - r0;
            const float* T = a.adjT + a.boff[c];
            const float* gvec = g_lds ? g_lds : a.g + r0;
            for (int j = lane; j < nc; j += 64) u = fmaf(T[(size_t)l * nc + j], gvec[j], u);
            u = wave_sum(u);
            gv = gvec[l];
            if (lane < GF) s_P[wv][lane] = a.P[(size_t)gi * GF + lane];
        }
        if (lane == 0) { s_u[wv] = u; s_row[wv] = gi < gb ? gi : -1; if (gi < gb && wv >= 0) s_u[4 + wv] = gv; }
        __syncthreads();
        for (int r = 0; r < 4; ++r) {
            const int row = s_row[r];
            if (row < 0) continue;
            const float ur = s_u[r];
            const float fv = RECOMP ? gcn_hidden(s_P[r], w, b1k, a, a.rows[row], k) : a.feat[(size_t)row * GH + k];
            float dh = 0.f;
            if (fv > 0.f) { dh = ur * w3k; if (a.train && a.p > 0.f) dh *= a.scale; }
#pragma unroll
            for (int ff = 0; ff < 16; ++ff) acc.w1[ff] = fma(s_P[r][half * 16 + ff], (double)dh, acc.w1[ff]);
            if (half == 0) { acc.b1 += (double)dh; acc.w3 += (double)ur * (double)fv; }
            if (threadIdx.x == 0) acc.b3 += (double)s_u[4 + r];
        }
        __syncthreads();
    }
}
__device__ void gcn_write_partials(const GcnAcc& acc, double* part) {
    const int k = threadIdx.x & 127, half = threadIdx.x >> 7;
#pragma unroll
    for (int ff = 0; ff < 16; ++ff) part[(half * 16 + ff) * GH + k] = acc.w1[ff];
    if (half == 0) { part[OFF_B1 + k] = acc.b1; part[OFF_W3 + k] = acc.w3; }
    if (threadIdx.x == 0) part[OFF_B3] = acc.b3;
}
__device__ __forceinline__ void gcn_load_unit(const float* __restrict__ params, int k, float (&w)[GF], float& b1k, float& w3k) {
#pragma unroll
    for (int f = 0; f < GF; ++f) w[f] = params[f * GH + k];
    b1k = params[OFF_B1 + k]; w3k = params[OFF_W3 + k];
}

// general form ------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gcn_fwd(GcnArgs a, int chunk) {
    __shared__ float s_red[4];
    if (a.info[0] & ST_REFUSED) return;
    const int n = min(a.cap, a.counts[2]), g0 = blockIdx.x * chunk;
    if (g0 >= n) return;
    float w[GF], b1k, w3k;
    gcn_load_unit(a.params, threadIdx.x & 127, w, b1k, w3k);
    gcn_fwd_rows(a, g0, min(chunk, n - g0), w, b1k, w3k, a.t + g0, s_red);
}
__global__ __launch_bounds__(256) void gcn_mid(GcnArgs a) {
    if (a.info[0] & ST_REFUSED) return;
    const int n = min(a.cap, a.counts[2]);
    for (int gi = blockIdx.x * 4 + (threadIdx.x >> 6); gi < n; gi += gridDim.x * 4) {
        const int c = a.rowcloud[gi], r0 = a.coff[c];
        gcn_mid_rows(a, c, gi - r0, 0x7fffffff - (gi - r0), a.t + r0, a.g + r0);      // this row alone
    }
}
__global__ __launch_bounds__(256) void gcn_bwd(GcnArgs a, int chunk) {
    __shared__ double s_P[4][GF]; __shared__ float s_u[8]; __shared__ int s_row[4];
    if (a.info[0] & ST_REFUSED) return;
    const int n = min(a.cap, a.counts[2]), g0 = min(n, (int)blockIdx.x * chunk);
    float w[GF], b1k, w3k;
    gcn_load_unit(a.params, threadIdx.x & 127, w, b1k, w3k);
    GcnAcc acc; for (int i = 0; i < 16; ++i) acc.w1[i] = 0.0; acc.b1 = acc.w3 = acc.b3 = 0.0;
    gcn_bwd_rows<false>(a, g0, min(n, g0 + chunk), w, b1k, w3k, nullptr, acc, s_P, s_u, s_row);
    gcn_write_partials(acc, a.part + (size_t)blockIdx.x * NPARAM);
}
// fused form: a workgroup owns whole clouds --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gcn_step_fused(GcnArgs a, int B, int* flag) {
    __shared__ float s_t[FUSED_CAP]; __shared__ float s_g[FUSED_CAP];
    __shared__ float s_red[4]; __shared__ double s_P[4][GF]; __shared__ float s_u[8]; __shared__ int s_row[4];
    if (a.info[0] & ST_REFUSED) return;
    float w[GF], b1k, w3k;
    gcn_load_unit(a.params, threadIdx.x & 127, w, b1k, w3k);
    GcnAcc acc; for (int i = 0; i < 16; ++i) acc.w1[i] = 0.0; acc.b1 = acc.w3 = acc.b3 = 0.0;
    for (int c = blockIdx.x; c < B; c += gridDim.x) {
        const int r0 = a.coff[c], nc = a.coff[c + 1] - r0;
        if (nc <= 0) continue;
        if (nc > FUSED_CAP || r0 + nc > a.cap) { if (threadIdx.x == 0) atomicOr(flag, (int)SSDR_GCN_ST_OVERSIZE); continue; }      // (refused on the host from n_max; never indexed)
        gcn_fwd_rows(a, r0, nc, w, b1k, w3k, s_t, s_red);
        gcn_mid_rows(a, c, threadIdx.x >> 6, 4, s_t, s_g);
        __syncthreads();
        if (a.part) gcn_bwd_rows<true>(a, r0, r0 + nc, w, b1k, w3k, s_g, acc, s_P, s_u, s_row);
        __syncthreads();
    }
    if (a.part) gcn_write_partials(acc, a.part + (size_t)blockIdx.x * NPARAM);
}

// ---- the step's last launch: gradient = the partials in workgroup order; torch.optim.Adam (decay added to the gradient) ------------------------
__global__ __launch_bounds__(64) void gcn_adam(const double* __restrict__ part, int nwg, float* params, float* m, float* v, const int* __restrict__ info,
                                               float wd, float omb1, float beta2, float omb2, float eps, float step_size, float bc2_sqrt) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= NPARAM || (info[0] & ST_REFUSED)) return;
    double s = 0.0;
    for (int w = 0; w < nwg; ++w) s += part[(size_t)w * NPARAM + i];
    const float p = params[i];
    const float g = (float)s + wd * p;
    const float mi = m[i] + omb1 * (g - m[i]);
    const float vi = v[i] * beta2 + (omb2 * g) * g;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    params[i] = p + (-step_size) * (mi / denom);
}

// loss = -mean(log s[labelled]) - lamda * mean(log(1 - s[unlabelled])) from the stored x, float64 sums in a fixed order (one workgroup)
__global__ __launch_bounds__(256) void gcn_loss(GcnArgs a, float* out) {
    __shared__ double s_l[256], s_u[256];
    if (a.info[0] & ST_REFUSED) { if (threadIdx.x == 0) *out = 0.f; return; }
    const int n = min(a.cap, a.counts[2]), n_unl = a.counts[0], n_lab = a.counts[1];
    double sl = 0.0, su = 0.0;
    for (int gi = threadIdx.x; gi < n; gi += 256) {
        const float s = 1.0f / (1.0f + expf(-a.x[gi]));
        if (a.rows[gi] >= n_unl) sl += log((double)s); else su += log((double)(1.0f - s));
    }
    s_l[threadIdx.x] = sl; s_u[threadIdx.x] = su;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) { s_l[threadIdx.x] += s_l[threadIdx.x + o]; s_u[threadIdx.x] += s_u[threadIdx.x + o]; } __syncthreads(); }
    if (threadIdx.x == 0) *out = (float)(-(s_l[0] / (double)n_lab) - (n_unl ? (double)a.lamda * (s_u[0] / (double)n_unl) : 0.0));
}

// evaluation rows: cat(relu(P W1 + b1), x) as float64 at the row's place in the [unlabelled | labelled] order; NaN -> 1e-10, +-inf -> 1e10 (gcn.py:241-245)
__global__ __launch_bounds__(256) void gcn_eval_rows(GcnArgs a, double* out, int* info) {
    const int n = min(a.cap, a.counts[2]);
    const bool refused = (a.info[0] & ST_REFUSED) != 0;
    int subst = 0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < (long)n * 129; e += (long)gridDim.x * 256) {
        const int gi = (int)(e / 129), k = (int)(e % 129);
        float v = 0.f;
        if (!refused) {
            if (k == GH) v = a.x[gi];
            else {
                double acc = 0.0;
                for (int f = 0; f < GF; ++f) acc = fma(a.P[(size_t)gi * GF + f], (double)a.params[f * GH + k], acc);
                const float h = (float)(acc + (double)a.params[OFF_B1 + k]);
                v = fmaxf(h, 0.f);
                if (__builtin_isnan(h)) v = h;          // (fmaxf drops a NaN operand; torch's relu keeps it)
            }
        }
        double d = (double)v;
        if (__builtin_isnan(v)) { d = 1.0e-10; ++subst; } else if (__builtin_isinf(v)) { d = 1.0e10; ++subst; }
        out[(size_t)a.rows[gi] * 129 + k] = d;
    }
    if (subst) { atomicAdd(&info[2], subst); atomicOr(&info[0], (int)SSDR_GCN_ST_SUBSTITUTED); }
}
__global__ void gcn_merge(const int* info, int* counts) { if (threadIdx.x == 0) counts[5] |= info[0] & ST_REFUSED; }
__global__ void gcn_set_form(int* info, int form) { if (threadIdx.x == 0) info[3] = form; }

struct GcnState { DevBuf f, d, i, chain_f, chain_d, chain_i; GcnChainBufs last; bool have_last = false; };
GcnState& gst(hipStream_t st) { return per_stream<GcnState>(st); }

constexpr const char* GCN_FORM_NAME[] = {"", "gcn_form:general", "gcn_form:fused"};

struct GcnPlan { GcnArgs a; float* m; float* v; int* flag; int nwg_b, chunk_b, nwg_f, chunk_f, nwg_fused; };

// scratch + P = A V for a graph of at most cap_rows rows; d_info is the caller's status words (the NO_LABELLED flag is raised there)
int gcn_prepare(hipStream_t s, const float* d_v, const float* d_adj, const float* d_adjT, const int32_t* d_coff, const int64_t* d_boff, size_t B, size_t n_max,
                const int32_t* d_rows, const int32_t* d_rowcloud, const int32_t* d_counts, size_t cap, int32_t* d_info, GcnPlan& pl) {
    GcnState& Q = gst(s);
    const int nwg_b = (int)std::max<size_t>(1, std::min<size_t>(256, (cap + 15) / 16)), chunk_b = (int)(((cap + nwg_b - 1) / nwg_b + 3) & ~(size_t)3);
    const int nwg_f = (int)std::max<size_t>(1, std::min<size_t>(1024, (cap + 7) / 8)), chunk_f = (int)(((cap + nwg_f - 1) / nwg_f + 1) & ~(size_t)1);
    const int nwg_fused = (int)std::max<size_t>(1, std::min<size_t>(256, B));
    // P [cap,32] float64, then floats: feat [cap,128], t, x, g [cap], m, v [NPARAM]
    SSDR_TRY(Q.f.reserve(4 * (cap * (2 * GF + GH + 3) + 2 * (size_t)NPARAM + 64)));
    SSDR_TRY(Q.d.reserve(8 * (size_t)NPARAM * (size_t)std::max(nwg_b, nwg_fused)));
    double* P = Q.f.as<double>(); float* feat = reinterpret_cast<float*>(P + cap * GF); float* t = feat + cap * GH; float* x = t + cap; float* g = x + cap; float* m = g + cap; float* v = m + NPARAM;
    pl.a = GcnArgs{P, d_adj, d_adjT, d_coff, (const long long*)d_boff, d_rows, d_rowcloud, d_counts, d_info, nullptr, feat, t, x, g, Q.d.as<double>(),
                   0.f, 1.f, 1.2f, 0ull, 0, 0, (int)cap};
    pl.m = m; pl.v = v; pl.flag = d_info; pl.nwg_b = nwg_b; pl.chunk_b = chunk_b; pl.nwg_f = nwg_f; pl.chunk_f = chunk_f; pl.nwg_fused = nwg_fused;
    hipLaunchKernelGGL(gcn_prep, dim3((unsigned)std::max<size_t>(1, std::min<size_t>((n_max + 3) / 4, 1024)), 1, (unsigned)B), dim3(256), 0, s, d_v, d_adj, d_coff,
                       (const long long*)d_boff, d_rows, d_counts, d_info, P, d_info);
    return SSDR_OK;
}
// forward without dropout with `params`: x for every live row (the loss after the last step, the evaluation)
void gcn_forward_eval(hipStream_t s, GcnPlan& pl, const float* params) {
    GcnArgs a = pl.a; a.params = params; a.train = 0; a.p = 0.f; a.scale = 1.f; a.part = nullptr;
    hipLaunchKernelGGL(gcn_fwd, dim3(pl.nwg_f), dim3(256), 0, s, a, pl.chunk_f);
    hipLaunchKernelGGL(gcn_mid, dim3((unsigned)std::max(1, std::min((a.cap + 3) / 4, 4096))), dim3(256), 0, s, a);
}

bool bad_graph(const void* a, const void* b, const void* c, const void* d, const void* e, const void* f, size_t B, size_t n_max, size_t cap) {
    return !a || !b || !c || !d || !e || !f || B == 0 || B > 65535 || n_max == 0 || cap == 0 || cap > (1u << 22);
}

}  // namespace

int gcn_chain_buffers(hipStream_t s, size_t cap_rows, size_t cap_sq, GcnChainBufs& B) {
    GcnState& Q = gst(s);
    SSDR_TRY(Q.chain_f.reserve(4 * (2 * cap_rows * GF + 2 * cap_sq + NPARAM + 8)));
    SSDR_TRY(Q.chain_d.reserve(8 * cap_rows * 129));
    SSDR_TRY(Q.chain_i.reserve(4 * (cap_rows + 16)));
    B.feat = Q.chain_f.as<float>(); B.v = B.feat + cap_rows * GF; B.adj = B.v + cap_rows * GF; B.adjT = B.adj + cap_sq; B.params = B.adjT + cap_sq; B.loss = B.params + NPARAM;
    B.rows129 = Q.chain_d.as<double>(); B.info = Q.chain_i.as<int32_t>(); B.cap_rows = cap_rows;
    Q.last = B; Q.have_last = true;
    return SSDR_OK;
}
const GcnChainBufs* gcn_chain_last(hipStream_t s) { GcnState& Q = gst(s); return Q.have_last ? &Q.last : nullptr; }
int gcn_merge_status(const int32_t* d_info, int32_t* d_counts, hipStream_t s) {
    hipLaunchKernelGGL(gcn_merge, dim3(1), dim3(64), 0, s, d_info, d_counts);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

}  // namespace ssdr

using namespace ssdr;

extern "C" {

int ssdr_gcn_block_adj_dev(const float* d_feat, size_t cap_rows, int F, const double* d_centres, const double* d_cd_dir, const int32_t* d_coff, const int64_t* d_boff,
                           size_t num_clouds, size_t n_max, const int32_t* d_rows, const int32_t* d_counts, float* d_out_v, float* d_out_adj, float* d_out_adjT,
                           int32_t* d_rowcloud, int32_t* d_info, void* stream) {
    if (bad_graph(d_feat, d_centres, d_cd_dir, d_coff, d_boff, d_rows, num_clouds, n_max, cap_rows) || !d_counts || !d_out_v || !d_out_adj || !d_out_adjT || !d_rowcloud || !d_info || F != GF) {
        set_error("gcn_block_adj: bad arguments (F == 32, at most 2^22 rows, at most 65535 clouds)"); return SSDR_ERR_INVALID;
    }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    const unsigned B = (unsigned)num_clouds;
    hipLaunchKernelGGL(gcn_info_reset, dim3(1), dim3(64), 0, s, d_info);
    hipLaunchKernelGGL(gcn_normalize, dim3(grid_for((long)cap_rows * 64)), dim3(256), 0, s, d_feat, (int)cap_rows, d_counts, d_out_v);
    hipLaunchKernelGGL(gcn_adj_block, dim3(grid_for((long)n_max * n_max, 256), 1, B), dim3(256), 0, s, d_out_v, d_centres, d_cd_dir, d_coff, (const long long*)d_boff, d_rows, d_out_adj);
    hipLaunchKernelGGL(gcn_adj_scale, dim3(grid_for((long)n_max, 64), 1, B), dim3(256), 0, s, d_coff, (const long long*)d_boff, d_out_adj, d_out_adjT, d_rowcloud, d_info);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_gcn_train_dev(const float* d_v, const float* d_adj, const float* d_adjT, const int32_t* d_coff, const int64_t* d_boff, size_t num_clouds, size_t n_max,
                       const int32_t* d_rows, const int32_t* d_rowcloud, const int32_t* d_counts, size_t cap_rows, const float* d_init, float* d_trained, int steps,
                       float p, float lr, float weight_decay, float lamda, uint64_t seed, int form, float* d_loss, int32_t* d_info, void* stream) {
    if (bad_graph(d_v, d_adj, d_adjT, d_coff, d_boff, d_rows, num_clouds, n_max, cap_rows) || !d_rowcloud || !d_counts || !d_init || !d_trained || !d_loss || !d_info || steps < 0 ||
        !(p >= 0.f && p < 1.f) || form < SSDR_GCN_FORM_AUTO || form > SSDR_GCN_FORM_FUSED) {
        set_error("gcn_train: bad arguments (0 <= p < 1, form 0..2, at most 2^22 rows)"); return SSDR_ERR_INVALID;
    }
    if (form == SSDR_GCN_FORM_FUSED && n_max > (size_t)FUSED_CAP) { set_error("gcn_train: the fused form holds blocks of at most %d rows (n_max = %zu)", FUSED_CAP, n_max); return SSDR_ERR_INVALID; }
    if (form == SSDR_GCN_FORM_AUTO) form = n_max <= (size_t)FUSED_CAP ? SSDR_GCN_FORM_FUSED : SSDR_GCN_FORM_GENERAL;
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    GcnPlan pl;
    SSDR_TRY(gcn_prepare(s, d_v, d_adj, d_adjT, d_coff, d_boff, num_clouds, n_max, d_rows, d_rowcloud, d_counts, cap_rows, d_info, pl));
    hipLaunchKernelGGL(gcn_set_form, dim3(1), dim3(64), 0, s, d_info, form);
    if (d_trained != d_init) SSDR_HIP(hipMemcpyAsync(d_trained, d_init, 4 * NPARAM, hipMemcpyDeviceToDevice, s));
    SSDR_HIP(hipMemsetAsync(pl.m, 0, 4 * 2 * NPARAM, s));
    {
        ProfScope prof(GCN_FORM_NAME[form], s, 0.0);
        GcnArgs a = pl.a; a.params = d_trained; a.train = 1; a.p = p; a.scale = 1.0f / (1.0f - p); a.lamda = lamda; a.seed = seed;
        const float omb1 = (float)(1.0 - 0.9), beta2 = 0.999f, omb2 = (float)(1.0 - 0.999), eps = 1e-8f;      // (1 - beta in float64 first, as torch passes them)
        const bool fused = form == SSDR_GCN_FORM_FUSED;
        const int nwg = fused ? pl.nwg_fused : pl.nwg_b;
        for (int step = 0; step < steps; ++step) {
            a.step = step;
            if (fused) hipLaunchKernelGGL(gcn_step_fused, dim3(nwg), dim3(256), 0, s, a, (int)num_clouds, d_info);
            else {
                hipLaunchKernelGGL(gcn_fwd, dim3(pl.nwg_f), dim3(256), 0, s, a, pl.chunk_f);
                hipLaunchKernelGGL(gcn_mid, dim3((unsigned)std::max(1, std::min((a.cap + 3) / 4, 4096))), dim3(256), 0, s, a);
                hipLaunchKernelGGL(gcn_bwd, dim3(nwg), dim3(256), 0, s, a, pl.chunk_b);
            }
            if (step == 0) hipLaunchKernelGGL(gcn_loss, dim3(1), dim3(256), 0, s, a, d_loss);
            const double bc1 = 1.0 - std::pow(0.9, step + 1), bc2 = 1.0 - std::pow(0.999, step + 1);
            hipLaunchKernelGGL(gcn_adam, dim3((NPARAM + 63) / 64), dim3(64), 0, s, a.part, nwg, d_trained, pl.m, pl.v, d_info, weight_decay, omb1, beta2, omb2, eps,
                               (float)((double)lr / bc1), (float)std::sqrt(bc2));
        }
        SSDR_HIP(hipGetLastError());
    }
    gcn_forward_eval(s, pl, d_trained);
    GcnArgs a = pl.a; a.lamda = lamda;
    hipLaunchKernelGGL(gcn_loss, dim3(1), dim3(256), 0, s, a, d_loss + 1);
    if (steps == 0) SSDR_HIP(hipMemcpyAsync(d_loss, d_loss + 1, 4, hipMemcpyDeviceToDevice, s));
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_gcn_eval_dev(const float* d_v, const float* d_adj, const float* d_adjT, const int32_t* d_coff, const int64_t* d_boff, size_t num_clouds, size_t n_max,
                      const int32_t* d_rows, const int32_t* d_rowcloud, const int32_t* d_counts, size_t cap_rows, const float* d_params, double* d_out, int32_t* d_info,
                      void* stream) {
    if (bad_graph(d_v, d_adj, d_adjT, d_coff, d_boff, d_rows, num_clouds, n_max, cap_rows) || !d_rowcloud || !d_counts || !d_params || !d_out || !d_info) {
        set_error("gcn_eval: bad arguments"); return SSDR_ERR_INVALID;
    }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    GcnPlan pl;
    SSDR_TRY(gcn_prepare(s, d_v, d_adj, d_adjT, d_coff, d_boff, num_clouds, n_max, d_rows, d_rowcloud, d_counts, cap_rows, d_info, pl));
    gcn_forward_eval(s, pl, d_params);
    GcnArgs a = pl.a; a.params = d_params;
    hipLaunchKernelGGL(gcn_eval_rows, dim3(grid_for((long)cap_rows * 129)), dim3(256), 0, s, a, d_out, d_info);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_gcn_sampling_rows(void* stream, const double** d_rows, size_t* cap_rows, const float** d_params, const float** d_loss, const int32_t** d_info) {
    if (!d_rows) { set_error("gcn_sampling_rows: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    const GcnChainBufs* B = gcn_chain_last(pick_stream(stream));
    if (!B) { set_error("gcn_sampling_rows: no ssdr_gcn_sampling_dev call on this stream yet"); return SSDR_ERR_INVALID; }
    *d_rows = B->rows129; if (cap_rows) *cap_rows = B->cap_rows; if (d_params) *d_params = B->params; if (d_loss) *d_loss = B->loss; if (d_info) *d_info = B->info;
    return SSDR_OK;
}

}  // extern "C"
