// RandLA-Net training step + C ABI (include/ssdr_al.h, "RandLA-Net training" section): forward in training or inference mode, the loss of
// RandLANet.py:43-84 / get_loss (:486-503), the backward pass and TF's Adam, all float32 with float32 accumulation.
//
// A small set of generic kernels (strided GEMM, per-channel reductions, batch norm, gathers, attention pooling, max pooling, loss, Adam) is driven
// from a host-side tape: every forward helper launches its kernel and pushes the closure that runs its backward; the backward pass zeroes the
// gradient workspace once and replays the tape in reverse, every closure ACCUMULATING into its inputs' gradients.
//
// Units (graph order; the order of oracle/randla_np.layer_specs):
//   fc0 | per encoder level i: mlp1, LFAmlp1, LFAatt_pooling_1fc, LFAatt_pooling_1mlp, LFAmlp2, LFAatt_pooling_2fc, LFAatt_pooling_2mlp, mlp2,
//   shortcut | decoder_0 | Decoder_layer_0 .. L-1 | fc1, fc2, fc
// Parameter tensors (ssdr_randla_train_param_shape): for each unit in that order  W, b (when the unit has a bias), gamma, beta, moving mean,
// moving variance (when it has a batch norm) — raw and unfolded.  W is [in, out]; the Decoder_layer_j kernels (conv2d_transpose) are [out, in].
// Inference layer `l` of csrc/randla_model.hip is unit l for fc0, units 1 + 9 i + (0..6) for 1 + 8 i + (0..6), units 1 + 9 i + 7 and + 8 stacked
// for 1 + 8 i + 7, and unit l + L from decoder_0 on.
//
// The scatter-adds behind gather_neighbour, nearest_interpolation and random_sample use float atomicAdd by default: the low bits of the gradients (and
// of the weights after a step) depend on the run.  Forward values do not.  ssdr_randla_train_set_deterministic(handle, 1) replaces the three scatters
// with reductions over inverse lists (scatter_det.hip) that add in a fixed order: then the gradients and the weights are the same bits every run.
#include "ssdr_internal.hpp"
#include "scatter_det.hpp"
#include "train_exchange.hpp"
#include "mix32.hpp"
#include <cmath>
#include <cstring>
#include <functional>

namespace ssdr {
namespace {

constexpr float BN_EPS = 1e-6f, LRELU = 0.2f, BN_MOMENTUM = 0.99f;
constexpr int BK = 16;

// ---- strided GEMM: C[i,j] (+)= sum_k A(i,k) B(k,j) (+ bias[j]) over k in this block's chunk; blockIdx.z selects the chunk and the output slab ----
struct GemmArgs {
    const float* A; long ars, acs; const float* B; long brs, bcs; float* C; long crs, ccs, czs;
    int M, N, K, kchunk; const float* bias; int accumulate;
};

template <int BM, int BN, int TM, int TN>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs a) {
    __shared__ float As[BK][BM + 1];
    __shared__ float Bs[BK][BN + 1];
    const int t = threadIdx.x, i0 = blockIdx.x * BM, j0 = blockIdx.y * BN;
    const int k_lo = blockIdx.z * a.kchunk, k_hi = min(a.K, k_lo + a.kchunk);
    constexpr int TX = BN / TN;
    const int ty = t / TX, tx = t % TX;
    float acc[TM][TN];
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int n = 0; n < TN; ++n) acc[m][n] = 0.f;
    for (int k0 = k_lo; k0 < k_hi; k0 += BK) {
        for (int e = t; e < BM * BK; e += 256) {
            int i, k;
            if (a.acs == 1) { k = e % BK; i = e / BK; } else { i = e % BM; k = e / BM; }
            const int gi = i0 + i, gk = k0 + k;
            As[k][i] = (gi < a.M && gk < k_hi) ? a.A[(long)gi * a.ars + (long)gk * a.acs] : 0.f;
        }
        for (int e = t; e < BN * BK; e += 256) {
            int j, k;
            if (a.bcs == 1) { j = e % BN; k = e / BN; } else { k = e % BK; j = e / BK; }
            const int gj = j0 + j, gk = k0 + k;
            Bs[k][j] = (gj < a.N && gk < k_hi) ? a.B[(long)gk * a.brs + (long)gj * a.bcs] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < BK; ++kk) {
            float av[TM], bv[TN];
#pragma unroll
            for (int m = 0; m < TM; ++m) av[m] = As[kk][ty * TM + m];
#pragma unroll
            for (int n = 0; n < TN; ++n) bv[n] = Bs[kk][tx * TN + n];
#pragma unroll
            for (int m = 0; m < TM; ++m)
#pragma unroll
                for (int n = 0; n < TN; ++n) acc[m][n] = fmaf(av[m], bv[n], acc[m][n]);
        }
        __syncthreads();
    }
    float* C = a.C + (long)blockIdx.z * a.czs;
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int n = 0; n < TN; ++n) {
            const int gi = i0 + ty * TM + m, gj = j0 + tx * TN + n;
            if (gi < a.M && gj < a.N) {
                float v = acc[m][n];
                if (a.bias && blockIdx.z == 0) v += a.bias[gj];
                float* c = C + (long)gi * a.crs + (long)gj * a.ccs;
                *c = a.accumulate ? *c + v : v;
            }
        }
}

// out[i * rs + j * cs] = sum_z part[z][i][j]   (the combine of a split reduction: dW)
__global__ void sum_slabs_kernel(const float* part, int nz, int rows, int cols, float* out, long rs, long cs) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x, n = (long)rows * cols;
    if (e >= n) return;
    float s = 0.f;
    for (int z = 0; z < nz; ++z) s += part[(long)z * n + e];
    out[(e / cols) * rs + (e % cols) * cs] = s;
}

// ---- per-channel reductions over rows: a grid of row chunks, two partial values per (chunk, channel), then a combine ----
// RED_STATS: chunk mean and sum of squared deviations from it of z.   RED_BNBWD: sum dY and sum dY * xhat, dY = dA * lrelu'(A).   RED_SUM: sum z.
enum { RED_STATS = 0, RED_BNBWD = 1, RED_SUM = 2 };
struct RedArgs {
    const float* z; int ldz; const float* da; const float* av; int lda; int act;     // da / av: gradient and value of the layer's output
    const float* mean; const float* invstd; int M, C, ct, chunk; float* part;          // part [nchunks][2][C]
};

template <int MODE>
__global__ __launch_bounds__(256) void reduce_kernel(RedArgs a) {
    __shared__ float s0[256];
    __shared__ float s1[256];
    const int t = threadIdx.x, ct = a.ct, nsub = 256 / ct, cl = t % ct, sub = t / ct;
    const int c = blockIdx.y * ct + cl;
    const int r0 = blockIdx.x * a.chunk, r1 = min(a.M, r0 + a.chunk);
    const bool on = c < a.C;
    float v0 = 0.f, v1 = 0.f;
    if (MODE == RED_STATS) {
        if (on) for (int r = r0 + sub; r < r1; r += nsub) v0 += a.z[(long)r * a.ldz + c];
        s0[t] = v0; __syncthreads();
        float sum = 0.f;
        for (int s = 0; s < nsub; ++s) sum += s0[s * ct + cl];
        const float mu = sum / (float)(r1 - r0);
        if (on) for (int r = r0 + sub; r < r1; r += nsub) { const float d = a.z[(long)r * a.ldz + c] - mu; v1 = fmaf(d, d, v1); }
        s1[t] = v1; __syncthreads();
        if (sub == 0 && on) {
            float m2 = 0.f;
            for (int s = 0; s < nsub; ++s) m2 += s1[s * ct + cl];
            a.part[((long)blockIdx.x * 2 + 0) * a.C + c] = mu;
            a.part[((long)blockIdx.x * 2 + 1) * a.C + c] = m2;
        }
        return;
    }
    if (on) {
        if (MODE == RED_BNBWD) {
            const float mu = a.mean[c], is = a.invstd[c];
            for (int r = r0 + sub; r < r1; r += nsub) {
                float dy = a.da[(long)r * a.lda + c];
                if (a.act && !(a.av[(long)r * a.lda + c] > 0.f)) dy *= LRELU;
                v0 += dy; v1 = fmaf(dy, (a.z[(long)r * a.ldz + c] - mu) * is, v1);
            }
        } else {
            for (int r = r0 + sub; r < r1; r += nsub) v0 += a.z[(long)r * a.ldz + c];
        }
    }
    s0[t] = v0; s1[t] = v1; __syncthreads();
    if (sub == 0 && on) {
        float x0 = 0.f, x1 = 0.f;
        for (int s = 0; s < nsub; ++s) { x0 += s0[s * ct + cl]; x1 += s1[s * ct + cl]; }
        a.part[((long)blockIdx.x * 2 + 0) * a.C + c] = x0;
        a.part[((long)blockIdx.x * 2 + 1) * a.C + c] = x1;
    }
}

// RED_STATS: Chan's pairwise merge of the chunks -> batch mean, 1 / sqrt(biased var + eps); optionally the moving averages (momentum 0.99):
// the moving variance takes var * n / (n - 1) on the fused (rank-4) path and the biased one for fc0.
// RED_BNBWD: out0 = dbeta, out1 = dgamma.   RED_SUM: out0 = the sum.
template <int MODE>
__global__ void combine_kernel(const float* part, int nchunks, int chunk, int M, int C, float* out0, float* out1, float* mov_mean, float* mov_var, int unbiased) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    if (MODE == RED_STATS) {
        float n = 0.f, mu = 0.f, m2 = 0.f;
        for (int k = 0; k < nchunks; ++k) {
            const float nb = (float)(min(M, (k + 1) * chunk) - k * chunk), mb = part[((long)k * 2) * C + c], m2b = part[((long)k * 2 + 1) * C + c];
            const float d = mb - mu, nn = n + nb;
            mu += d * (nb / nn); m2 += m2b + d * d * (n * nb / nn); n = nn;
        }
        const float var = m2 / (float)M;
        out0[c] = mu; out1[c] = 1.f / sqrtf(var + BN_EPS);
        if (mov_mean) {
            const float vm = (unbiased && M > 1) ? var * ((float)M / (float)(M - 1)) : var;
            mov_mean[c] -= (mov_mean[c] - mu) * (1.f - BN_MOMENTUM);
            mov_var[c] -= (mov_var[c] - vm) * (1.f - BN_MOMENTUM);
        }
        return;
    }
    float x0 = 0.f, x1 = 0.f;
    for (int k = 0; k < nchunks; ++k) { x0 += part[((long)k * 2) * C + c]; x1 += part[((long)k * 2 + 1) * C + c]; }
    out0[c] = x0;
    if (MODE == RED_BNBWD) out1[c] = x1;
}

// inference mode: the moving statistics take the batch statistics' place
__global__ void bn_eval_prep_kernel(const float* mov_mean, const float* mov_var, int C, float* mean, float* invstd) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) { mean[c] = mov_mean[c]; invstd[c] = 1.f / sqrtf(mov_var[c] + BN_EPS); }
}

// out = act(bn(z) [+ bn2(z2)])
struct BnArgs {
    const float* z; const float* mean; const float* invstd; const float* gamma; const float* beta;
    const float* z2; const float* mean2; const float* invstd2; const float* gamma2; const float* beta2;
    float* out; int ldo; int M, C, act;
};
__global__ void bn_apply_kernel(BnArgs a) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)a.M * a.C) return;
    const int c = (int)(e % a.C); const long r = e / a.C;
    float y = (a.z[e] - a.mean[c]) * a.invstd[c] * a.gamma[c] + a.beta[c];
    if (a.z2) y += (a.z2[e] - a.mean2[c]) * a.invstd2[c] * a.gamma2[c] + a.beta2[c];
    if (a.act) y = y > 0.f ? y : y * LRELU;
    a.out[r * a.ldo + c] = y;
}

// dz (in place of z) = gamma * invstd * (dY - dbeta / M - xhat * dgamma / M).  GLOBAL: dbeta and dgamma are sums over all ranks' rows and the row count
// is the global one, read from the device (count[0], left by the forward pass's merge)
template <bool GLOBAL>
__global__ void bn_bwd_kernel(float* z, const float* da, const float* av, int lda, int act, const float* mean, const float* invstd, const float* gamma,
                              const float* dbeta, const float* dgamma, int M, int C, const float* count) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)M * C) return;
    const int c = (int)(e % C); const long r = e / C;
    float dy = da[r * lda + c];
    if (act && !(av[r * lda + c] > 0.f)) dy *= LRELU;
    const float xh = (z[e] - mean[c]) * invstd[c], inv_m = 1.f / (GLOBAL ? count[0] : (float)M);
    z[e] = gamma[c] * invstd[c] * (dy - dbeta[c] * inv_m - xh * dgamma[c] * inv_m);
}

// dz = dY for a unit without batch norm (copy out of the strided gradient view, activation applied)
__global__ void copy_grad_kernel(float* z, const float* da, const float* av, int lda, int act, int M, int C) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)M * C) return;
    const int c = (int)(e % C); const long r = e / C;
    float dy = da[r * lda + c];
    if (act && !(av[r * lda + c] > 0.f)) dy *= LRELU;
    z[e] = dy;
}

// ---- gathers ----
// out[(b, r), 0..C) = src[(b, idx[b, r]), 0..C): gather_neighbour (r = n * K + k) and nearest_interpolation (K = 1)
__global__ void gather_rows_kernel(const float* src, int lds, int src_rows, const int32_t* idx, int rows_per_b, long total_rows, int C, float* out, int ldo) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total_rows * C) return;
    const int c = (int)(e % C); const long r = e / C; const long b = r / rows_per_b;
    int j = idx[r]; j = min(max(j, 0), src_rows - 1);
    out[r * ldo + c] = src[(b * src_rows + j) * lds + c];
}
__global__ void scatter_rows_kernel(float* dsrc, int lds, int src_rows, const int32_t* idx, int rows_per_b, long total_rows, int C, const float* dout, int ldo) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total_rows * C) return;
    const int c = (int)(e % C); const long r = e / C; const long b = r / rows_per_b;
    int j = idx[r]; j = min(max(j, 0), src_rows - 1);
    atomicAdd(&dsrc[(b * src_rows + j) * lds + c], dout[r * ldo + c]);
}

// relative_pos_encoding (RandLANet.py:529-535): [|p - q|, p - q, p, q] for every neighbour q of p
__global__ void relpos_kernel(const float* xyz, const int32_t* neigh, int n, long total, float* out) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;      // (b, p, k)
    if (e >= total) return;
    const long bp = e / 16, b = bp / n;
    int j = neigh[e]; j = min(max(j, 0), n - 1);
    const float* p = xyz + bp * 3; const float* q = xyz + (b * n + j) * 3;
    const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    float* o = out + e * 10;
    o[0] = sqrtf(dx * dx + dy * dy + dz * dz); o[1] = dx; o[2] = dy; o[3] = dz; o[4] = p[0]; o[5] = p[1]; o[6] = p[2]; o[7] = q[0]; o[8] = q[1]; o[9] = q[2];
}

// ---- attention pooling (RandLANet.py:572-585): softmax over the 16 neighbours per channel of s = f W_fc, then the weighted sum ----
__global__ void att_fwd_kernel(const float* f, const float* s, long points, int d, float* agg) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= points * d) return;
    const int c = (int)(e % d); const long p = e / d;
    const float* fp = f + p * 16 * d + c; const float* sp = s + p * 16 * d + c;
    float mx = sp[0];
    for (int k = 1; k < 16; ++k) mx = fmaxf(mx, sp[(long)k * d]);
    float den = 0.f, num = 0.f;
    for (int k = 0; k < 16; ++k) { const float w = expf(sp[(long)k * d] - mx); den += w; num = fmaf(w, fp[(long)k * d], num); }
    agg[e] = num / den;
}
// df += dagg * att;  ds (in place of s) = att * (dagg * f - sum_j att_j dagg f_j)
__global__ void att_bwd_kernel(const float* f, float* s, const float* dagg, long points, int d, float* df) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= points * d) return;
    const int c = (int)(e % d); const long p = e / d;
    const float* fp = f + p * 16 * d + c; float* sp = s + p * 16 * d + c; float* dfp = df + p * 16 * d + c;
    float mx = sp[0];
    for (int k = 1; k < 16; ++k) mx = fmaxf(mx, sp[(long)k * d]);
    float w[16], den = 0.f;
    for (int k = 0; k < 16; ++k) { w[k] = expf(sp[(long)k * d] - mx); den += w[k]; }
    const float g = dagg[e], inv = 1.f / den;
    float dot = 0.f;
    for (int k = 0; k < 16; ++k) { w[k] *= inv; dot = fmaf(w[k], g * fp[(long)k * d], dot); }
    for (int k = 0; k < 16; ++k) {
        dfp[(long)k * d] += g * w[k];
        sp[(long)k * d] = w[k] * (g * fp[(long)k * d] - dot);
    }
}

// ---- random_sample (RandLANet.py:537-548): max over the 16 pooled rows; the gradient is shared evenly among the rows equal to the maximum ----
__global__ void pool_fwd_kernel(const float* src, int lds, int src_rows, const int32_t* idx, int m_per_b, long total_m, int C, float* out, int ldo) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total_m * C) return;
    const int c = (int)(e % C); const long r = e / C, b = r / m_per_b;
    float mx = 0.f;
    for (int k = 0; k < 16; ++k) {
        int j = idx[r * 16 + k]; j = min(max(j, 0), src_rows - 1);
        const float v = src[(b * src_rows + j) * lds + c];
        mx = k == 0 ? v : fmaxf(mx, v);
    }
    out[r * ldo + c] = mx;
}
__global__ void pool_bwd_kernel(const float* src, float* dsrc, int lds, int src_rows, const int32_t* idx, int m_per_b, long total_m, int C, const float* out,
                                const float* dout, int ldo) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total_m * C) return;
    const int c = (int)(e % C); const long r = e / C, b = r / m_per_b;
    const float mx = out[r * ldo + c];
    int ties = 0; unsigned mask = 0;
    for (int k = 0; k < 16; ++k) {
        int j = idx[r * 16 + k]; j = min(max(j, 0), src_rows - 1);
        if (src[(b * src_rows + j) * lds + c] == mx) { ++ties; mask |= 1u << k; }
    }
    if (!ties) return;
    const float g = dout[r * ldo + c] / (float)ties;
    for (int k = 0; k < 16; ++k)
        if (mask >> k & 1) {
            int j = idx[r * 16 + k]; j = min(max(j, 0), src_rows - 1);
            atomicAdd(&dsrc[(b * src_rows + j) * lds + c], g);
        }
}

// ---- dropout (keep_prob 0.5 after fc2, RandLANet.py:176-177); mix32: mix32.hpp ----
// mask[i] = the bit of element first + i
__global__ void dropout_mask_kernel(uint64_t seed, uint64_t step, uint64_t first, long n, uint8_t* mask) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t e = first + (uint64_t)i;
    uint32_t h = mix32((uint32_t)seed ^ 0x9e3779b9u);
    h = mix32(h ^ (uint32_t)(seed >> 32)); h = mix32(h ^ (uint32_t)step); h = mix32(h ^ (uint32_t)(step >> 32));
    h = mix32(h ^ (uint32_t)e); h = mix32(h + (uint32_t)(e >> 32));
    mask[i] = (uint8_t)(h >> 31);
}
__global__ void dropout_fwd_kernel(const float* x, const uint8_t* mask, long n, float* y) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) y[e] = mask[e] ? x[e] * 2.f : 0.f;
}
__global__ void dropout_bwd_kernel(const float* dy, const uint8_t* mask, long n, float* dx) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n && mask[e]) dx[e] += dy[e] * 2.f;
}

// ---- loss (RandLANet.py:43-84, :486-503) ----
struct LossTables { int32_t remap[64]; uint8_t ignored[64]; float cw[32]; int nlab; };
// per row: validity, the weighted cross entropy on the pseudo label, correctness on the label; per block: their sums
__global__ __launch_bounds__(256) void loss_rows_kernel(const float* logits, int C, const int32_t* labels, const float* activation, const float* pseudo, long M,
                                                         LossTables tb, float* row_w, int32_t* row_cls, float* part, int* status) {
    __shared__ float sh[3][256];
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    float loss = 0.f, valid = 0.f, correct = 0.f;
    if (r < M) {
        const int lab = labels[r];
        float w = 0.f; int cls = -1;
        if (lab < 0 || lab >= tb.nlab) atomicOr(status, 2);
        else if (!tb.ignored[lab]) {
            const int ps = (int)pseudo[r];
            if (ps < 0 || ps >= tb.nlab) atomicOr(status, 2);
            else {
                cls = tb.remap[ps]; const int lc = tb.remap[lab];
                const float* z = logits + r * C;
                float mx = z[0];
                for (int c = 1; c < C; ++c) mx = fmaxf(mx, z[c]);
                float den = 0.f;
                for (int c = 0; c < C; ++c) den += expf(z[c] - mx);
                w = tb.cw[cls] * activation[r];
                loss = (logf(den) - (z[cls] - mx)) * w;
                int above = 0;
                for (int c = 0; c < C; ++c) above += z[c] > z[lc];
                correct = above == 0 ? 1.f : 0.f; valid = 1.f;
            }
        }
        row_w[r] = w; row_cls[r] = cls;
    }
    sh[0][threadIdx.x] = loss; sh[1][threadIdx.x] = valid; sh[2][threadIdx.x] = correct;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) for (int q = 0; q < 3; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) for (int q = 0; q < 3; ++q) part[(long)blockIdx.x * 3 + q] = sh[q][0];
}
// out[0] = loss, out[1] = accuracy, out[2] = valid rows; no valid row: zeros and status bit 0.  PACK: out[0 .. 2] = this rank's three sums (loss, valid,
// correct) for the gather; loss_merge_kernel finishes
template <bool PACK>
__global__ __launch_bounds__(256) void loss_final_kernel(const float* part, int nblocks, float* out, float* d_loss, float* d_acc, int* status) {
    __shared__ float sh[3][256];
    float v[3] = {0.f, 0.f, 0.f};
    for (int b = threadIdx.x; b < nblocks; b += 256) for (int q = 0; q < 3; ++q) v[q] += part[(long)b * 3 + q];
    for (int q = 0; q < 3; ++q) sh[q][threadIdx.x] = v[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) for (int q = 0; q < 3; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (PACK) { for (int q = 0; q < 3; ++q) out[q] = sh[q][0]; return; }
        const float n = sh[1][0];
        const float loss = n > 0.f ? sh[0][0] / n : 0.f, acc = n > 0.f ? sh[2][0] / n : 0.f;
        out[0] = loss; out[1] = acc; out[2] = n;
        if (d_loss) *d_loss = loss;
        if (d_acc) *d_acc = acc;
        if (!(n > 0.f)) atomicOr(status, 1);
    }
}
// records [world][3] = every rank's (loss, valid, correct) sums, added in rank order from 0: the same out / d_loss / d_acc on every rank, status bit 0
// only when no rank has a valid row
__global__ void loss_merge_kernel(const float* records, int world, float* out, float* d_loss, float* d_acc, int* status) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float v[3] = {0.f, 0.f, 0.f};
    for (int r = 0; r < world; ++r) for (int q = 0; q < 3; ++q) v[q] += records[r * 3 + q];
    const float n = v[1];
    const float loss = n > 0.f ? v[0] / n : 0.f, acc = n > 0.f ? v[2] / n : 0.f;
    out[0] = loss; out[1] = acc; out[2] = n;
    if (d_loss) *d_loss = loss;
    if (d_acc) *d_acc = acc;
    if (!(n > 0.f)) atomicOr(status, 1);
}
// dlogits = (softmax - onehot(pseudo)) * weight * activation / valid rows (of all ranks, when an exchange is set: fin[2] is global then)
__global__ void loss_grad_kernel(const float* logits, int C, long M, const float* row_w, const int32_t* row_cls, const float* fin, float* dlogits) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    const float n = fin[2]; const int cls = row_cls[r];
    const float* z = logits + r * C; float* d = dlogits + r * C;
    if (cls < 0 || !(n > 0.f)) { for (int c = 0; c < C; ++c) d[c] = 0.f; return; }
    const float w = row_w[r] / n;
    float mx = z[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, z[c]);
    float den = 0.f;
    for (int c = 0; c < C; ++c) den += expf(z[c] - mx);
    for (int c = 0; c < C; ++c) d[c] = (expf(z[c] - mx) / den - (c == cls ? 1.f : 0.f)) * w;
}

// ---- Adam as tf.train.AdamOptimizer applies it: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) comes from the host's step count ----
__global__ void adam_kernel(float* p, const float* g, float* m, float* v, long n, float lr_t) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const float gi = g[e];
    const float mi = m[e] + (gi - m[e]) * 0.1f;             // 1 - beta1, 1 - beta2 rounded once (1.f - 0.9f is not 0.1f)
    const float vi = v[e] + (gi * gi - v[e]) * 0.001f;
    m[e] = mi; v[e] = vi;
    p[e] -= lr_t * mi / (sqrtf(vi) + 1e-8f);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
struct Unit { int in, out; bool bias, bn, act, transposed, rank3; long oW = -1, ob = -1, og = -1, obeta = -1, omean = -1, ovar = -1, obs = -1; };
struct Tensor { int unit, kind, rows, cols; long off; };     // kind: 0 W, 1 b, 2 gamma, 3 beta (parameter arena); 4 moving mean, 5 moving variance (statistics arena)
struct View { float* v = nullptr; float* g = nullptr; int ld = 0, w = 0; };
View cols(const View& a, int c0, int w) { View r = a; r.v += c0; if (r.g) r.g += c0; r.w = w; return r; }

struct TrainStatus { DevBuf word; };
struct TrainPieces { DevBuf part, dwp; };      // scratch of the stand-alone launcher pieces, per stream

struct Train {
    int L = 5, K = 16, C = 13, in_dim = 6;
    int d_out[8] = {0};
    std::vector<Unit> units; std::vector<Tensor> tensors;
    long n_par = 0, n_stat = 0, n_bs = 0;
    DevBuf P, G, M, V, S, BS;           // parameters, gradients, Adam moments, moving statistics, per-step batch mean / invstd
    DevBuf act, grad, part, dwp, fin;   // activation and gradient workspaces (one (B, N) layout), reduction partials, dW slabs, loss result [3]
    DevBuf lpart;
    long act_floats = 0, grad_floats = 0; size_t planned_B = 0, planned_N = 0;
    LossTables tb{};
    float lr = 0.01f; long step = 0;
    bool params_set = false;
    // data-parallel mode (train_exchange.hpp): the callback, the collectives' send [1 + 2 cmax] and receive [world][1 + 2 cmax] buffers, and the table
    // of the (offset, length) ranges of G that hold gamma / beta gradients (global before the gradient sum: ranks other than 0 zero them)
    Exchange xg; DevBuf xsend, xrecv, gb_table; std::vector<long> gb_ranges; int cmax = 1;
    long xchg_floats() const { return xg.world > 0 ? (1L + xg.world) * xchg_record_floats(cmax) : 0; }
    // deterministic mode: the inverse lists of neigh / pool / interp of every level (list 3 i + 0 / 1 / 2), laid out by det_layout
    struct DetList { long off_at, pos_at; int src_rows, rows_per_b; };
    bool det = false, planned_det = false;
    std::vector<DetList> dl; std::vector<int> levels;      // levels: N_0 .. N_L of the last shape planned
    long list_ints = 0, key_slots = 0, share_floats = 0;
    DevBuf lists; RadixSorter sorter;                       // lists: [off and pos of every list | sort keys u64 [key_slots] | pooling shares f32 [share_floats]]
    InvList list(int i) const { return InvList{lists.as<int>() + dl[i].off_at, lists.as<int>() + dl[i].pos_at}; }
    uint64_t* sort_keys() const { return reinterpret_cast<uint64_t*>(lists.as<int>() + list_ints); }
    float* shares() const { return reinterpret_cast<float*>(sort_keys() + key_slots); }
    size_t det_bytes() const { return (size_t)list_ints * 4 + (size_t)key_slots * 8 + (size_t)share_floats * 4 + RadixSorter::scratch_bytes(sort_slots()); }
    size_t sort_slots() const { return ((size_t)key_slots + RADIX_TILE - 1) / RADIX_TILE * RADIX_TILE; }       // RadixSorter::sort rounds up to whole tiles
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};     // start, forward done, backward done, update done of the last call (ssdr_randla_train_last_ms)
    bool ev_valid = false;
    ~Train() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    float* par(long o) const { return P.as<float>() + o; }
    float* grd(long o) const { return G.as<float>() + o; }
};

constexpr long PART_FLOATS = 1 << 21, DWP_FLOATS = 1 << 23;

void build_units(Train& m) {
    auto add = [&](int in, int out, bool bn = true, bool act = true, bool bias = true, bool tr = false, bool r3 = false) {
        Unit u{}; u.in = in; u.out = out; u.bias = bias; u.bn = bn; u.act = act; u.transposed = tr; u.rank3 = r3; m.units.push_back(u);
    };
    add(m.in_dim, 8, true, true, true, false, true);
    int width = 8; std::vector<int> skips;
    for (int i = 0; i < m.L; ++i) {
        const int d = m.d_out[i];
        add(width, d / 2); add(10, d / 2); add(d, d, false, false, false); add(d, d / 2); add(d / 2, d / 2); add(d, d, false, false, false); add(d, d);
        add(d, 2 * d, true, false); add(width, 2 * d, true, false);
        if (i == 0) skips.push_back(2 * d);
        width = 2 * d; skips.push_back(width);
    }
    add(width, width);
    for (int j = 0; j < m.L; ++j) { const int skip = skips[skips.size() - j - 2]; add(skip + width, skip, true, true, true, true); width = skip; }
    add(width, 64); add(64, 32); add(32, m.C, false, false);
    for (size_t i = 0; i < m.units.size(); ++i) {
        Unit& u = m.units[i];
        u.oW = m.n_par; m.tensors.push_back({(int)i, 0, u.transposed ? u.out : u.in, u.transposed ? u.in : u.out, u.oW}); m.n_par += (long)u.in * u.out;
        if (u.bias) { u.ob = m.n_par; m.tensors.push_back({(int)i, 1, 1, u.out, u.ob}); m.n_par += u.out; }
        if (u.bn) {
            u.og = m.n_par; m.tensors.push_back({(int)i, 2, 1, u.out, u.og}); m.n_par += u.out;
            u.obeta = m.n_par; m.tensors.push_back({(int)i, 3, 1, u.out, u.obeta}); m.n_par += u.out;
            u.omean = m.n_stat; m.tensors.push_back({(int)i, 4, 1, u.out, u.omean}); m.n_stat += u.out;
            u.ovar = m.n_stat; m.tensors.push_back({(int)i, 5, 1, u.out, u.ovar}); m.n_stat += u.out;
            u.obs = m.n_bs; m.n_bs += 2 * u.out + 1;            // mean, 1 / std, and the global row count (one float; data-parallel mode)
            m.gb_ranges.push_back(u.og); m.gb_ranges.push_back(2L * u.out);      // gamma and beta lie side by side
            m.cmax = std::max(m.cmax, u.out);
        }
    }
}

inline unsigned blocks_for(long n, int per = 256) { return (unsigned)((n + per - 1) / per); }

// ---- the launchers: the tape (Runner) and the stand-alone pieces ssdr_randla_train_{gemm, dw, reduce}_dev both go through these, so a piece runs
// the step's own tile choice, split and chunk rules ----
int launch_gemm(hipStream_t s, const float* A, long ars, long acs, const float* B, long brs, long bcs, float* Cp, long crs, long ccs, int M, int N, int K,
                const float* bias, bool accumulate, int split = 1, long czs = 0) {
    GemmArgs a{A, ars, acs, B, brs, bcs, Cp, crs, ccs, czs, M, N, K, 0, bias, accumulate ? 1 : 0};
    a.kchunk = ((K + split - 1) / split + BK - 1) / BK * BK;
    const unsigned z = (unsigned)((K + a.kchunk - 1) / a.kchunk);
    if (M <= 16 && N <= 16) hipLaunchKernelGGL((gemm_kernel<16, 16, 1, 1>), dim3(1, 1, z), dim3(256), 0, s, a);
    else if (N <= 16) hipLaunchKernelGGL((gemm_kernel<256, 16, 4, 4>), dim3(blocks_for(M, 256), 1, z), dim3(256), 0, s, a);
    else if (M <= 16) hipLaunchKernelGGL((gemm_kernel<16, 256, 4, 4>), dim3(1, blocks_for(N, 256), z), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((gemm_kernel<64, 64, 4, 4>), dim3(blocks_for(M, 64), blocks_for(N, 64), z), dim3(256), 0, s, a);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

// the split of dW = x^T dz over its M rows: at most one slab per 512 rows, 1024 slabs, and what the slab buffer [split][in][out] holds
struct DwSplit { long split; int kchunk, nz; };
DwSplit dw_split(int M, int in, int out) {
    long split = std::max<long>(1, std::min<long>(M / 512, 1024));
    split = std::max<long>(1, std::min<long>(split, DWP_FLOATS / ((long)in * out)));
    const int kchunk = (int)(((M + split - 1) / split + BK - 1) / BK * BK);
    return DwSplit{split, kchunk, (M + kchunk - 1) / kchunk};
}
// dW[i * rs + j * cs] = sum over the M rows of x[r, i] dz[r, j]: slabs [nz][in][out] into dwp, then the combine.  dz is dense [M, out]
int launch_dw(hipStream_t s, const float* x, int ldx, const float* dz, int M, int in, int out, float* dwp, float* dW, long rs, long cs) {
    const DwSplit d = dw_split(M, in, out);
    SSDR_TRY(launch_gemm(s, x, 1, ldx, dz, out, 1, dwp, out, 1, in, out, M, nullptr, false, (int)d.split, (long)in * out));
    hipLaunchKernelGGL(sum_slabs_kernel, dim3(blocks_for((long)in * out)), dim3(256), 0, s, dwp, d.nz, in, out, dW, rs, cs);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

// the row chunks of a per-channel reduction: about one per 1024 rows, at most 1024, and what the partial buffer [nchunks][2][C] holds
struct RedSplit { int ct, chunk, nchunks; };
RedSplit red_split(int M, int C) {
    int ct = 8; while (ct < 64 && ct < C) ct *= 2;
    long want = std::max<long>(1, std::min<long>(M / 1024, 1024));
    want = std::max<long>(1, std::min<long>(want, PART_FLOATS / (2L * C)));
    const int chunk = (int)((M + want - 1) / want);
    return RedSplit{ct, chunk, (M + chunk - 1) / chunk};
}
// fills a.ct, a.chunk and a.part, launches the chunks; the number of chunks comes back
template <int MODE> int launch_reduce_chunks(hipStream_t s, RedArgs& a, float* part) {
    const RedSplit r = red_split(a.M, a.C);
    a.ct = r.ct; a.chunk = r.chunk; a.part = part;
    hipLaunchKernelGGL((reduce_kernel<MODE>), dim3(r.nchunks, blocks_for(a.C, r.ct)), dim3(256), 0, s, a);
    return r.nchunks;
}
template <int MODE> int launch_combine(hipStream_t s, const RedArgs& a, int nchunks, float* out0, float* out1, float* mm, float* mv, int unbiased) {
    hipLaunchKernelGGL((combine_kernel<MODE>), dim3(blocks_for(a.C, 64)), dim3(64), 0, s, a.part, nchunks, a.chunk, a.M, a.C, out0, out1, mm, mv, unbiased);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

// One pass over the graph.  dry: only the workspace layout is computed (no launch).
struct Runner {
    Train& m; hipStream_t s; bool dry; bool training; bool update_stats; bool want_grad;
    long a_off = 0, g_off = 0;
    std::vector<std::function<int()>> tape;
    int rc = SSDR_OK;

    View alloc(long rows, int w, bool with_grad, int ld = 0) {
        if (!ld) ld = w;
        View r; r.ld = ld; r.w = w;
        const long n = (rows * ld + 63) / 64 * 64;
        r.v = m.act.as<float>() + a_off; a_off += n;
        if (with_grad) { r.g = m.grad.as<float>() + g_off; g_off += n; }
        return r;
    }
    void push(std::function<int()> f) { if (!dry && want_grad) tape.push_back(std::move(f)); }

    int gemm(const float* A, long ars, long acs, const float* B, long brs, long bcs, float* Cp, long crs, long ccs, int M, int N, int K, const float* bias,
             bool accumulate) {
        if (dry) return SSDR_OK;
        return launch_gemm(s, A, ars, acs, B, brs, bcs, Cp, crs, ccs, M, N, K, bias, accumulate);
    }
    // W(k, n) of a unit: [in, out], or [out, in] for the transposed kernels
    static long w_rs(const Unit& u) { return u.transposed ? 1 : u.out; }
    static long w_cs(const Unit& u) { return u.transposed ? u.in : 1; }

    // data-parallel mode: this pass meets the other ranks
    bool meets() const { return m.xg.world > 0 && training; }
    int exchange(int op, const float* send, float* recv, size_t count) {
        if (m.xg.fn(m.xg.user, op, send, recv, count, (void*)s) != 0) { set_error("randla_train: exchange failed"); return SSDR_ERR_INVALID; }
        return SSDR_OK;
    }
    // RED_STATS: out0 = mean, out1 = 1 / std, and the row count behind them.  RED_BNBWD: out0 = dbeta, out1 = dgamma with out1 + C == out0.
    template <int MODE> int reduce(RedArgs a, float* out0, float* out1, float* mm, float* mv, int unbiased) {
        if (dry) return SSDR_OK;
        const int nchunks = launch_reduce_chunks<MODE>(s, a, m.part.as<float>());
        if (MODE != RED_SUM && meets()) {
            // one launch in front of the collective (the chunks' combine, into the send buffer), one behind it (the ranks' merge)
            float* send = m.xsend.as<float>(); float* recv = m.xrecv.as<float>();
            SSDR_HIP(hipGetLastError());
            if (MODE == RED_STATS) {
                SSDR_TRY(xchg_pack_stats(a.part, nchunks, a.chunk, a.M, a.C, send, s));
                SSDR_TRY(exchange(SSDR_XCHG_GATHER, send, recv, (size_t)xchg_record_floats(a.C)));
                return xchg_merge_stats(recv, m.xg.world, a.C, out0, out1, out1 + a.C, mm, mv, unbiased, s);
            }
            SSDR_TRY(xchg_pack_sums(a.part, nchunks, a.C, send, 1, s));
            SSDR_TRY(exchange(SSDR_XCHG_GATHER, send, recv, (size_t)2 * a.C));
            return xchg_merge_sums(recv, m.xg.world, 2 * a.C, out1, s);
        }
        return launch_combine<MODE>(s, a, nchunks, out0, out1, mm, mv, unbiased);
    }

    // z [M, out] = x W + b; with a batch norm its statistics land in BS (batch, or moving in inference mode)
    int linear(int ui, const View& x, int M, float** z_out) {
        const Unit& u = m.units[ui];
        if (x.w != u.in) { set_error("randla_train: unit %d takes %d channels, got %d", ui, u.in, x.w); return SSDR_ERR_INTERNAL; }
        View z = alloc(M, u.out, false); *z_out = z.v;
        SSDR_TRY(gemm(x.v, x.ld, 1, m.par(u.oW), w_rs(u), w_cs(u), z.v, u.out, 1, M, u.out, u.in, u.bias ? m.par(u.ob) : nullptr, false));
        if (u.bn && !dry) {
            float* mean = m.BS.as<float>() + u.obs; float* invstd = mean + u.out;
            if (training) {
                RedArgs r{}; r.z = z.v; r.ldz = u.out; r.M = M; r.C = u.out;
                SSDR_TRY(reduce<RED_STATS>(r, mean, invstd, update_stats ? m.S.as<float>() + u.omean : nullptr, update_stats ? m.S.as<float>() + u.ovar : nullptr, u.rank3 ? 0 : 1));
            } else {
                hipLaunchKernelGGL(bn_eval_prep_kernel, dim3(blocks_for(u.out, 64)), dim3(64), 0, s, m.S.as<float>() + u.omean, m.S.as<float>() + u.ovar, u.out, mean, invstd);
            }
        }
        return SSDR_OK;
    }
    // backward of linear: dz [M, out] is ready in z
    int linear_bwd(int ui, const View& x, int M, float* dz) {
        const Unit& u = m.units[ui];
        if (u.bias) { RedArgs r{}; r.z = dz; r.ldz = u.out; r.M = M; r.C = u.out; SSDR_TRY(reduce<RED_SUM>(r, m.grd(u.ob), nullptr, nullptr, nullptr, 0)); }
        SSDR_TRY(launch_dw(s, x.v, x.ld, dz, M, u.in, u.out, m.dwp.as<float>(), m.grd(u.oW), w_rs(u), w_cs(u)));
        if (x.g) SSDR_TRY(gemm(dz, u.out, 1, m.par(u.oW), w_cs(u), w_rs(u), x.g, x.ld, 1, M, u.in, u.out, nullptr, true));       // dx += dz W^T
        SSDR_HIP(hipGetLastError());
        return SSDR_OK;
    }
    BnArgs bn_args(int ui, const float* z) {
        const Unit& u = m.units[ui]; BnArgs b{};
        b.z = z; b.mean = m.BS.as<float>() + u.obs; b.invstd = b.mean + u.out; b.gamma = m.par(u.og); b.beta = m.par(u.obeta);
        return b;
    }
    // dz of a batch-normed unit whose output view y received its gradient (activation `act` applied after the norm)
    int bn_bwd(int ui, float* z, const View& y, int M, int act) {
        const Unit& u = m.units[ui];
        const float* mean = m.BS.as<float>() + u.obs; const float* invstd = mean + u.out;
        RedArgs r{}; r.z = z; r.ldz = u.out; r.da = y.g; r.av = y.v; r.lda = y.ld; r.act = act; r.mean = mean; r.invstd = invstd; r.M = M; r.C = u.out;
        SSDR_TRY(reduce<RED_BNBWD>(r, m.grd(u.obeta), m.grd(u.og), nullptr, nullptr, 0));
        if (meets()) hipLaunchKernelGGL(bn_bwd_kernel<true>, dim3(blocks_for((long)M * u.out)), dim3(256), 0, s, z, y.g, y.v, y.ld, act, mean, invstd, m.par(u.og), m.grd(u.obeta), m.grd(u.og), M, u.out, invstd + u.out);
        else hipLaunchKernelGGL(bn_bwd_kernel<false>, dim3(blocks_for((long)M * u.out)), dim3(256), 0, s, z, y.g, y.v, y.ld, act, mean, invstd, m.par(u.og), m.grd(u.obeta), m.grd(u.og), M, u.out, (const float*)nullptr);
        return SSDR_OK;
    }

    // conv + BN + leaky ReLU (helper_tf_util.conv2d / conv2d_transpose / dense) into y (a column range of some buffer)
    int conv(int ui, const View& x, int M, const View& y) {
        const Unit& u = m.units[ui]; float* z = nullptr;
        SSDR_TRY(linear(ui, x, M, &z));
        if (!dry) {
            if (u.bn) {
                BnArgs b = bn_args(ui, z); b.out = y.v; b.ldo = y.ld; b.M = M; b.C = u.out; b.act = u.act;
                hipLaunchKernelGGL(bn_apply_kernel, dim3(blocks_for((long)M * u.out)), dim3(256), 0, s, b);
            } else {
                SSDR_HIP(hipMemcpy2DAsync(y.v, sizeof(float) * y.ld, z, sizeof(float) * u.out, sizeof(float) * u.out, M, hipMemcpyDeviceToDevice, s));
            }
            SSDR_HIP(hipGetLastError());
        }
        push([=]() -> int {
            const Unit& uu = m.units[ui];
            if (uu.bn) SSDR_TRY(bn_bwd(ui, z, y, M, uu.act));
            else hipLaunchKernelGGL(copy_grad_kernel, dim3(blocks_for((long)M * uu.out)), dim3(256), 0, s, z, y.g, y.v, y.ld, 0, M, uu.out);
            return linear_bwd(ui, x, M, z);
        });
        return SSDR_OK;
    }
    // y = lrelu(bn(x1 W1 + b1) + bn(x2 W2 + b2))   (RandLANet.py:508-512)
    int residual(int u1, const View& x1, int u2, const View& x2, int M, const View& y) {
        float *z1 = nullptr, *z2 = nullptr;
        SSDR_TRY(linear(u1, x1, M, &z1)); SSDR_TRY(linear(u2, x2, M, &z2));
        if (!dry) {
            BnArgs b = bn_args(u1, z1); const BnArgs b2 = bn_args(u2, z2);
            b.z2 = b2.z; b.mean2 = b2.mean; b.invstd2 = b2.invstd; b.gamma2 = b2.gamma; b.beta2 = b2.beta;
            b.out = y.v; b.ldo = y.ld; b.M = M; b.C = m.units[u1].out; b.act = 1;
            hipLaunchKernelGGL(bn_apply_kernel, dim3(blocks_for((long)M * b.C)), dim3(256), 0, s, b);
            SSDR_HIP(hipGetLastError());
        }
        push([=]() -> int {
            SSDR_TRY(bn_bwd(u1, z1, y, M, 1)); SSDR_TRY(linear_bwd(u1, x1, M, z1));
            SSDR_TRY(bn_bwd(u2, z2, y, M, 1)); return linear_bwd(u2, x2, M, z2);
        });
        return SSDR_OK;
    }
    // y[(b, r), :] = src[(b, idx[b, r]), :]
    // list: which of the handle's inverse lists belongs to idx (deterministic mode)
    int gather(const View& src, int src_rows, const int32_t* idx, int rows_per_b, int B, const View& y, int list) {
        const long total = (long)B * rows_per_b; const int Cw = src.w; const bool det = m.det;
        if (!dry) { hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks_for(total * Cw)), dim3(256), 0, s, src.v, src.ld, src_rows, idx, rows_per_b, total, Cw, y.v, y.ld); SSDR_HIP(hipGetLastError()); }
        push([=]() -> int {
            if (det) return scatter_rows_det(m.list(list), B, rows_per_b, src_rows, y.g, y.ld, Cw, src.g, src.ld, s);
            hipLaunchKernelGGL(scatter_rows_kernel, dim3(blocks_for(total * Cw)), dim3(256), 0, s, src.g, src.ld, src_rows, idx, rows_per_b, total, Cw, y.g, y.ld);
            SSDR_HIP(hipGetLastError()); return SSDR_OK;
        });
        return SSDR_OK;
    }
    // att_pooling up to the weighted sum: fcat [P * 16, d] (dense) -> agg [P, d]
    int attention(int ufc, const View& fcat, long points, const View& agg) {
        const int d = fcat.w; float* sc = nullptr;
        SSDR_TRY(linear(ufc, fcat, (int)(points * 16), &sc));
        if (!dry) { hipLaunchKernelGGL(att_fwd_kernel, dim3(blocks_for(points * d)), dim3(256), 0, s, fcat.v, sc, points, d, agg.v); SSDR_HIP(hipGetLastError()); }
        push([=]() -> int {
            hipLaunchKernelGGL(att_bwd_kernel, dim3(blocks_for(points * d)), dim3(256), 0, s, fcat.v, sc, agg.g, points, d, fcat.g);
            return linear_bwd(ufc, fcat, (int)(points * 16), sc);
        });
        return SSDR_OK;
    }
    int pool(const View& src, int src_rows, const int32_t* idx, int m_per_b, int B, const View& y, int list) {
        const long total = (long)B * m_per_b; const int Cw = src.w; const bool det = m.det;
        if (!dry) { hipLaunchKernelGGL(pool_fwd_kernel, dim3(blocks_for(total * Cw)), dim3(256), 0, s, src.v, src.ld, src_rows, idx, m_per_b, total, Cw, y.v, y.ld); SSDR_HIP(hipGetLastError()); }
        push([=]() -> int {
            if (det) return pool_grad_det(m.list(list), src.v, src.g, src.ld, src_rows, idx, B, m_per_b, Cw, y.v, y.g, y.ld, m.shares(), s);
            hipLaunchKernelGGL(pool_bwd_kernel, dim3(blocks_for(total * Cw)), dim3(256), 0, s, src.v, src.g, src.ld, src_rows, idx, m_per_b, total, Cw, y.v, y.g, y.ld);
            SSDR_HIP(hipGetLastError()); return SSDR_OK;
        });
        return SSDR_OK;
    }

    // inference() (RandLANet.py:140-180).  logits [B N, C] and fc2's output (pre-dropout) come back as views.
    int forward(int B, const std::vector<int>& N, const float* d_features, const float* const* d_xyz, const int32_t* const* d_neigh, const int32_t* const* d_pool,
                const int32_t* const* d_interp, const uint8_t* d_mask, View* logits, View* feat32) {
        const int L = m.L; const int rows0 = B * N[0];
        View xin; xin.v = const_cast<float*>(d_features); xin.g = nullptr; xin.ld = m.in_dim; xin.w = m.in_dim;
        View f = alloc(rows0, 8, true);
        SSDR_TRY(conv(0, xin, rows0, f));
        std::vector<View> enc;
        for (int i = 0; i < L; ++i) {
            const int d = m.d_out[i], h = d / 2, n = N[i], rows = B * n, base = 1 + 9 * i; const long R = (long)rows * 16;
            View f_pc = alloc(rows, h, true); SSDR_TRY(conv(base + 0, f, rows, f_pc));
            View rel = alloc(R, 10, false);
            if (!dry) { hipLaunchKernelGGL(relpos_kernel, dim3(blocks_for(R)), dim3(256), 0, s, d_xyz[i], d_neigh[i], n, R, rel.v); SSDR_HIP(hipGetLastError()); }
            View fcat1 = alloc(R, d, true);
            SSDR_TRY(gather(f_pc, n, d_neigh[i], n * 16, B, cols(fcat1, 0, h), 3 * i));
            SSDR_TRY(conv(base + 1, rel, (int)R, cols(fcat1, h, h)));
            View agg1 = alloc(rows, d, true); SSDR_TRY(attention(base + 2, fcat1, rows, agg1));
            View a1 = alloc(rows, h, true); SSDR_TRY(conv(base + 3, agg1, rows, a1));
            View fcat2 = alloc(R, d, true);
            SSDR_TRY(gather(a1, n, d_neigh[i], n * 16, B, cols(fcat2, 0, h), 3 * i));
            SSDR_TRY(conv(base + 4, cols(fcat1, h, h), (int)R, cols(fcat2, h, h)));
            View agg2 = alloc(rows, d, true); SSDR_TRY(attention(base + 5, fcat2, rows, agg2));
            View a2 = alloc(rows, d, true); SSDR_TRY(conv(base + 6, agg2, rows, a2));
            // the encoder outputs that a decoder layer reads as its skip input are the left columns of that layer's [skip | interp] buffer
            View out = i == 0 ? cols(alloc(rows, 4 * d, true), 0, 2 * d) : alloc(rows, 2 * d, true);
            if (i == 0) out.ld = 4 * d;
            SSDR_TRY(residual(base + 7, a2, base + 8, f, rows, out));
            const int rows_next = B * N[i + 1];
            View samp;
            if (i <= L - 2) { samp = cols(alloc(rows_next, 2 * d + 2 * m.d_out[i + 1], true), 0, 2 * d); }
            else samp = alloc(rows_next, 2 * d, true);
            SSDR_TRY(pool(out, n, d_pool[i], N[i + 1], B, samp, 3 * i + 1));
            if (i == 0) enc.push_back(out);
            enc.push_back(samp);
            f = samp;
        }
        int ui = 1 + 9 * L;
        View dec = alloc(B * N[L], f.w, true); SSDR_TRY(conv(ui++, f, B * N[L], dec));
        View feat = dec; int feat_n = N[L];
        std::vector<int> enc_n; enc_n.push_back(N[0]); for (int i = 0; i < L; ++i) enc_n.push_back(N[i + 1]);
        for (int j = 0; j < L; ++j) {
            const int e = (int)enc.size() - j - 2; const View skip = enc[e]; const int n = enc_n[e];
            if (skip.ld != skip.w + feat.w) { set_error("randla_train: decoder %d: skip buffer laid out for %d interpolated channels, got %d", j, skip.ld - skip.w, feat.w); return SSDR_ERR_INTERNAL; }
            View cat = skip; cat.w = skip.ld;
            SSDR_TRY(gather(feat, feat_n, d_interp[L - 1 - j], n, B, cols(cat, skip.w, feat.w), 3 * (L - 1 - j) + 2));       // nearest_interpolation :550-559
            View y = alloc(B * n, skip.w, true); SSDR_TRY(conv(ui++, cat, B * n, y));
            feat = y; feat_n = n;
        }
        View f1 = alloc(rows0, 64, true); SSDR_TRY(conv(ui++, feat, rows0, f1));
        View f2 = alloc(rows0, 32, true); SSDR_TRY(conv(ui++, f1, rows0, f2));
        View head_in = f2;
        if (training) {
            View dr = alloc(rows0, 32, true);
            const long n = (long)rows0 * 32;
            if (!dry) { hipLaunchKernelGGL(dropout_fwd_kernel, dim3(blocks_for(n)), dim3(256), 0, s, f2.v, d_mask, n, dr.v); SSDR_HIP(hipGetLastError()); }
            push([=]() -> int { hipLaunchKernelGGL(dropout_bwd_kernel, dim3(blocks_for(n)), dim3(256), 0, s, dr.g, d_mask, n, f2.g); SSDR_HIP(hipGetLastError()); return SSDR_OK; });
            head_in = dr;
        }
        View lg = alloc(rows0, m.C, true); SSDR_TRY(conv(ui++, head_in, rows0, lg));
        *logits = lg; *feat32 = f2;
        return SSDR_OK;
    }
};

int* status_word(hipStream_t s) {
    TrainStatus& st = per_stream<TrainStatus>(s);
    if (!st.word.p) { if (st.word.reserve(64) != SSDR_OK) return nullptr; if (hipMemset(st.word.p, 0, 64) != hipSuccess) return nullptr; }
    return st.word.as<int>();
}

struct StepIn {
    size_t B, N; const float* d_features; const float* const* d_xyz; const int32_t* ratios; const int32_t* const* d_neigh; const int32_t* const* d_pool;
    const int32_t* const* d_interp; const int32_t* d_labels; const float* d_activation; const float* d_pseudo; const uint8_t* d_mask;
};

int check_common(Train* m, const StepIn& in, std::vector<int>& N, const char* who) {
    if (!m || !in.d_features || !in.d_xyz || !in.ratios || !in.d_neigh || !in.d_pool || !in.d_interp || in.B == 0 || in.N == 0) { set_error("%s: bad arguments (NULL pointer or empty batch)", who); return SSDR_ERR_INVALID; }
    if (!m->params_set) { set_error("%s: not every parameter tensor has been set", who); return SSDR_ERR_INVALID; }
    N.assign(m->L + 1, 0); N[0] = (int)in.N;
    for (int i = 0; i < m->L; ++i) {
        if (!in.d_xyz[i] || !in.d_neigh[i] || !in.d_pool[i] || !in.d_interp[i]) { set_error("%s: level %d: NULL pyramid array", who, i); return SSDR_ERR_INVALID; }
        if (in.ratios[i] <= 0 || N[i] % in.ratios[i] != 0) { set_error("%s: level %d has %d rows, not divisible by its sub-sampling ratio %d", who, i, N[i], in.ratios[i]); return SSDR_ERR_INVALID; }
        N[i + 1] = N[i] / in.ratios[i];
    }
    if (in.B * in.N * 16 > 0x7fffffffull / 2) { set_error("%s: more than 2^30 neighbour rows", who); return SSDR_ERR_UNSUPPORTED; }
    return SSDR_OK;
}

// Deterministic mode's share of the workspace for B tiles of N[0] points: list 3 i is neigh_i (the level's two gathers share it), 3 i + 1 pool_i,
// 3 i + 2 interp_i; one key buffer for the largest list and one share buffer for the largest pooling follow.  Sizes only, nothing is allocated.
void det_layout(Train* m, long B, const std::vector<int>& N) {
    m->dl.clear(); m->list_ints = m->key_slots = m->share_floats = 0;
    auto add = [&](int src_rows, long rows_per_b) {
        Train::DetList d{m->list_ints, m->list_ints + inv_off_ints(B, src_rows), src_rows, (int)rows_per_b};
        m->list_ints = d.pos_at + inv_pos_ints(B, rows_per_b);
        m->key_slots = std::max(m->key_slots, B * rows_per_b);
        m->dl.push_back(d);
    };
    for (int i = 0; i < m->L; ++i) {
        add(N[i], (long)N[i] * 16); add(N[i], (long)N[i + 1] * 16); add(N[i + 1], N[i]);
        m->share_floats = std::max(m->share_floats, B * N[i + 1] * 2L * m->d_out[i]);
    }
}

int plan(Train* m, const StepIn& in, const std::vector<int>& N, hipStream_t s) {
    if (m->planned_B == in.B && m->planned_N == in.N && m->planned_det == m->det && m->levels == N) return SSDR_OK;
    if (m->det) {
        det_layout(m, (long)in.B, N);
        SSDR_TRY(m->lists.reserve((size_t)m->list_ints * 4 + (size_t)m->key_slots * 8 + (size_t)m->share_floats * 4));
        SSDR_TRY(m->sorter.reserve(m->sort_slots()));
    }
    Runner dryrun{*m, s, true, true, false, true};
    View a, b;
    SSDR_TRY(dryrun.forward((int)in.B, N, in.d_features, in.d_xyz, in.d_neigh, in.d_pool, in.d_interp, nullptr, &a, &b));
    // a smaller layout fits the buffers of a larger one; nothing else may be enqueued on them while they move
    if ((size_t)dryrun.a_off * 4 > m->act.cap || (size_t)dryrun.g_off * 4 > m->grad.cap) SSDR_HIP(hipDeviceSynchronize());
    SSDR_TRY(m->act.reserve((size_t)dryrun.a_off * 4)); SSDR_TRY(m->grad.reserve((size_t)dryrun.g_off * 4));
    const long rows0 = (long)in.B * in.N;
    SSDR_TRY(m->lpart.reserve((size_t)(rows0 * 8 + (rows0 / 256 + 2) * 12 + 64)));
    m->act_floats = dryrun.a_off; m->grad_floats = dryrun.g_off; m->planned_B = in.B; m->planned_N = in.N;
    m->planned_det = m->det; m->levels = N;
    return SSDR_OK;
}

// mode bits: 1 loss + backward, 2 Adam update (and the moving statistics)
int run(Train* m, const StepIn& in, int is_training, int mode, float* d_logits, float* d_feat32, float* d_loss, float* d_acc, void* stream, const char* who) {
    std::vector<int> N;
    SSDR_TRY(check_common(m, in, N, who));
    if (is_training && !in.d_mask) { set_error("%s: training mode needs a dropout mask", who); return SSDR_ERR_INVALID; }
    if ((mode & 1) && (!in.d_labels || !in.d_activation || !in.d_pseudo)) { set_error("%s: NULL labels / activation / pseudo", who); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    int* status = status_word(s);
    if (!status) { set_error("%s: no status word", who); return SSDR_ERR_HIP; }
    SSDR_TRY(plan(m, in, N, s));
    Runner r{*m, s, false, is_training != 0, (mode & 2) != 0, (mode & 1) != 0};
    View logits, feat32;
    m->ev_valid = false;
    SSDR_HIP(hipEventRecord(m->ev[0], s));
    SSDR_TRY(r.forward((int)in.B, N, in.d_features, in.d_xyz, in.d_neigh, in.d_pool, in.d_interp, in.d_mask, &logits, &feat32));
    const long rows0 = (long)in.B * in.N;
    if (d_logits) SSDR_HIP(hipMemcpyAsync(d_logits, logits.v, sizeof(float) * rows0 * m->C, hipMemcpyDeviceToDevice, s));
    if (d_feat32) SSDR_HIP(hipMemcpyAsync(d_feat32, feat32.v, sizeof(float) * rows0 * 32, hipMemcpyDeviceToDevice, s));
    SSDR_HIP(hipEventRecord(m->ev[1], s));
    if (!(mode & 1)) { SSDR_HIP(hipEventRecord(m->ev[2], s)); SSDR_HIP(hipEventRecord(m->ev[3], s)); m->ev_valid = true; return SSDR_OK; }
    SSDR_HIP(hipMemsetAsync(m->grad.p, 0, (size_t)m->grad_floats * 4, s));
    float* row_w = m->lpart.as<float>(); int32_t* row_cls = reinterpret_cast<int32_t*>(row_w + rows0); float* lp = row_w + 2 * rows0;
    const int nb = (int)blocks_for(rows0);
    hipLaunchKernelGGL(loss_rows_kernel, dim3(nb), dim3(256), 0, s, logits.v, m->C, in.d_labels, in.d_activation, in.d_pseudo, rows0, m->tb, row_w, row_cls, lp, status);
    if (r.meets()) {
        hipLaunchKernelGGL(loss_final_kernel<true>, dim3(1), dim3(256), 0, s, lp, nb, m->xsend.as<float>(), (float*)nullptr, (float*)nullptr, status);
        SSDR_HIP(hipGetLastError());
        SSDR_TRY(r.exchange(SSDR_XCHG_GATHER, m->xsend.as<float>(), m->xrecv.as<float>(), 3));
        hipLaunchKernelGGL(loss_merge_kernel, dim3(1), dim3(64), 0, s, m->xrecv.as<float>(), m->xg.world, m->fin.as<float>(), d_loss, d_acc, status);
    } else {
        hipLaunchKernelGGL(loss_final_kernel<false>, dim3(1), dim3(256), 0, s, lp, nb, m->fin.as<float>(), d_loss, d_acc, status);
    }
    hipLaunchKernelGGL(loss_grad_kernel, dim3(blocks_for(rows0)), dim3(256), 0, s, logits.v, m->C, rows0, row_w, row_cls, m->fin.as<float>(), logits.g);
    SSDR_HIP(hipGetLastError());
    // the lists are built from the index arrays of THIS call, every call: a feeder hands out the same buffers with new contents
    if (m->det) {
        for (int i = 0; i < m->L; ++i) {
            const int32_t* const idx[3] = {in.d_neigh[i], in.d_pool[i], in.d_interp[i]};
            for (int k = 0; k < 3; ++k) {
                const Train::DetList& d = m->dl[3 * i + k];
                SSDR_TRY(inv_list_build(idx[k], (int)in.B, d.rows_per_b, d.src_rows, m->sort_keys(), m->list(3 * i + k), m->sorter, s));
            }
        }
    }
    for (size_t i = r.tape.size(); i-- > 0;) SSDR_TRY(r.tape[i]());
    if (r.meets()) {
        // ONE sum over the whole arena.  gamma / beta gradients are global already: every rank but 0 zeroes them (adding 0 is exact)
        if (m->xg.rank != 0) SSDR_TRY(xchg_zero_ranges(m->G.as<float>(), m->gb_table.as<long>(), (int)(m->gb_ranges.size() / 2), s));
        SSDR_TRY(r.exchange(SSDR_XCHG_SUM, m->G.as<float>(), m->G.as<float>(), (size_t)m->n_par));
    }
    SSDR_HIP(hipEventRecord(m->ev[2], s));
    if (mode & 2) {
        m->step += 1;
        const double t = (double)m->step;
        const float lr_t = (float)((double)m->lr * std::sqrt(1.0 - std::pow(0.999, t)) / (1.0 - std::pow(0.9, t)));
        hipLaunchKernelGGL(adam_kernel, dim3(blocks_for(m->n_par)), dim3(256), 0, s, m->P.as<float>(), m->G.as<float>(), m->M.as<float>(), m->V.as<float>(), m->n_par, lr_t);
        SSDR_HIP(hipGetLastError());
    }
    SSDR_HIP(hipEventRecord(m->ev[3], s));
    m->ev_valid = true;
    return SSDR_OK;
}

}  // namespace
}  // namespace ssdr

using namespace ssdr;

extern "C" {

int ssdr_randla_train_create(int num_layers, const int32_t* d_out, int k_n, int num_classes, int in_dim, void** handle) {
    if (!handle || !d_out || num_layers < 1 || num_layers > 8) { set_error("randla_train_create: bad arguments"); return SSDR_ERR_INVALID; }
    if (k_n != 16) { set_error("randla_train: k_n=%d is not supported (16)", k_n); return SSDR_ERR_UNSUPPORTED; }
    if (num_classes < 1 || num_classes > 32) { set_error("randla_train: num_classes must be in [1,32]"); return SSDR_ERR_UNSUPPORTED; }
    if (in_dim < 1) { set_error("randla_train: in_dim=%d: the input features need at least one channel", in_dim); return SSDR_ERR_UNSUPPORTED; }
    for (int i = 0; i < num_layers; ++i)
        if (d_out[i] < 2 || d_out[i] > 512 || d_out[i] % 2) { set_error("randla_train: d_out[%d]=%d is not supported (even, 2 .. 512)", i, d_out[i]); return SSDR_ERR_UNSUPPORTED; }
    SSDR_TRY(ensure_init());
    Train* m = new Train();
    m->L = num_layers; m->K = k_n; m->C = num_classes; m->in_dim = in_dim;
    for (int i = 0; i < num_layers; ++i) m->d_out[i] = d_out[i];
    build_units(*m);
    auto fail = [&](int rc) { delete m; return rc; };
    const size_t pb = sizeof(float) * (size_t)m->n_par, sb = sizeof(float) * (size_t)std::max<long>(m->n_stat, 1);
    for (DevBuf* b : {&m->P, &m->G, &m->M, &m->V}) { if (b->reserve(pb) != SSDR_OK) return fail(SSDR_ERR_HIP); if (hipMemset(b->p, 0, pb) != hipSuccess) return fail(SSDR_ERR_HIP); }
    if (m->S.reserve(sb) != SSDR_OK || m->BS.reserve(sizeof(float) * (size_t)std::max<long>(m->n_bs, 1)) != SSDR_OK || m->part.reserve(sizeof(float) * PART_FLOATS) != SSDR_OK ||
        m->dwp.reserve(sizeof(float) * DWP_FLOATS) != SSDR_OK || m->fin.reserve(64) != SSDR_OK) return fail(SSDR_ERR_HIP);
    if (hipMemset(m->S.p, 0, sb) != hipSuccess || hipMemset(m->fin.p, 0, 64) != hipSuccess) return fail(SSDR_ERR_HIP);
    // get_loss with no weights and nothing ignored until ssdr_randla_train_set_loss says otherwise
    m->tb.nlab = num_classes;
    for (int c = 0; c < 64; ++c) { m->tb.remap[c] = c < num_classes ? c : 0; m->tb.ignored[c] = 0; }
    for (int c = 0; c < 32; ++c) m->tb.cw[c] = 1.f;
    for (hipEvent_t& e : m->ev) if (hipEventCreate(&e) != hipSuccess) return fail(SSDR_ERR_HIP);
    if (!m->gb_ranges.empty()) {
        const size_t tb = sizeof(long) * m->gb_ranges.size();
        if (m->gb_table.reserve(tb) != SSDR_OK || hipMemcpy(m->gb_table.p, m->gb_ranges.data(), tb, hipMemcpyHostToDevice) != hipSuccess) return fail(SSDR_ERR_HIP);
    }
    *handle = m;
    return SSDR_OK;
}

void ssdr_randla_train_destroy(void* handle) { delete static_cast<Train*>(handle); }

int ssdr_randla_train_num_params(void* handle) { return handle ? (int)static_cast<Train*>(handle)->tensors.size() : 0; }

int ssdr_randla_train_param_shape(void* handle, int i, int* unit, int* kind, int* rows, int* cols) {
    Train* m = static_cast<Train*>(handle);
    if (!m || i < 0 || i >= (int)m->tensors.size()) { set_error("randla_train_param_shape: bad tensor index"); return SSDR_ERR_INVALID; }
    const Tensor& t = m->tensors[i];
    if (unit) *unit = t.unit;
    if (kind) *kind = t.kind;
    if (rows) *rows = t.rows;
    if (cols) *cols = t.cols;
    return SSDR_OK;
}

static int param_ptr(Train* m, int i, int which, float** p, size_t* bytes, const char* who) {
    if (!m || i < 0 || i >= (int)m->tensors.size() || which < 0 || which > 2) { set_error("%s: bad tensor index or slot", who); return SSDR_ERR_INVALID; }
    const Tensor& t = m->tensors[i];
    if (t.kind >= 4 && which != 0) { set_error("%s: the moving statistics have no Adam moments", who); return SSDR_ERR_INVALID; }
    float* base = t.kind >= 4 ? m->S.as<float>() : which == 0 ? m->P.as<float>() : which == 1 ? m->M.as<float>() : m->V.as<float>();
    *p = base + t.off; *bytes = sizeof(float) * (size_t)t.rows * t.cols;
    return SSDR_OK;
}

/* which: 0 the tensor, 1 Adam's m, 2 Adam's v.  Host pointers; synchronous. */
int ssdr_randla_train_set_param(void* handle, int i, int which, const float* host) {
    Train* m = static_cast<Train*>(handle); float* p; size_t n;
    if (!host) { set_error("randla_train_set_param: NULL"); return SSDR_ERR_INVALID; }
    SSDR_TRY(param_ptr(m, i, which, &p, &n, "randla_train_set_param"));
    SSDR_HIP(hipDeviceSynchronize());
    SSDR_HIP(hipMemcpy(p, host, n, hipMemcpyHostToDevice));
    m->params_set = true;
    return SSDR_OK;
}
int ssdr_randla_train_get_param(void* handle, int i, int which, float* host) {
    Train* m = static_cast<Train*>(handle); float* p; size_t n;
    if (!host) { set_error("randla_train_get_param: NULL"); return SSDR_ERR_INVALID; }
    SSDR_TRY(param_ptr(m, i, which, &p, &n, "randla_train_get_param"));
    SSDR_HIP(hipDeviceSynchronize());
    SSDR_HIP(hipMemcpy(host, p, n, hipMemcpyDeviceToHost));
    return SSDR_OK;
}
int ssdr_randla_train_get_grad(void* handle, int i, float* host) {
    Train* m = static_cast<Train*>(handle);
    if (!m || !host || i < 0 || i >= (int)m->tensors.size() || m->tensors[i].kind >= 4) { set_error("randla_train_get_grad: bad tensor index (the moving statistics have no gradient)"); return SSDR_ERR_INVALID; }
    const Tensor& t = m->tensors[i];
    SSDR_HIP(hipDeviceSynchronize());
    SSDR_HIP(hipMemcpy(host, m->G.as<float>() + t.off, sizeof(float) * (size_t)t.rows * t.cols, hipMemcpyDeviceToHost));
    return SSDR_OK;
}
/* test hook: overwrite a gradient, for ssdr_randla_train_apply_dev */
int ssdr_randla_train_set_grad(void* handle, int i, const float* host) {
    Train* m = static_cast<Train*>(handle);
    if (!m || !host || i < 0 || i >= (int)m->tensors.size() || m->tensors[i].kind >= 4) { set_error("randla_train_set_grad: bad tensor index"); return SSDR_ERR_INVALID; }
    const Tensor& t = m->tensors[i];
    SSDR_HIP(hipDeviceSynchronize());
    SSDR_HIP(hipMemcpy(m->G.as<float>() + t.off, host, sizeof(float) * (size_t)t.rows * t.cols, hipMemcpyHostToDevice));
    return SSDR_OK;
}
/* one Adam update from the gradients as they stand */
int ssdr_randla_train_apply_dev(void* handle, void* stream) {
    Train* m = static_cast<Train*>(handle);
    if (!m) { set_error("randla_train_apply: bad handle"); return SSDR_ERR_INVALID; }
    hipStream_t s = pick_stream(stream);
    m->step += 1;
    const double t = (double)m->step;
    const float lr_t = (float)((double)m->lr * std::sqrt(1.0 - std::pow(0.999, t)) / (1.0 - std::pow(0.9, t)));
    hipLaunchKernelGGL(adam_kernel, dim3(blocks_for(m->n_par)), dim3(256), 0, s, m->P.as<float>(), m->G.as<float>(), m->M.as<float>(), m->V.as<float>(), m->n_par, lr_t);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

int ssdr_randla_train_set_loss(void* handle, const float* class_weights, const int32_t* ignored_labels, int n_ignored) {
    Train* m = static_cast<Train*>(handle);
    if (!m || n_ignored < 0 || (n_ignored > 0 && !ignored_labels) || m->C + n_ignored > 64) { set_error("randla_train_set_loss: bad arguments"); return SSDR_ERR_INVALID; }
    // reducing_list (RandLANet.py:66-69): range(C) with a 0 inserted at every ignored label, in the order given
    std::vector<int> list(m->C);
    for (int c = 0; c < m->C; ++c) list[c] = c;
    for (int k = 0; k < n_ignored; ++k) {
        const int ign = ignored_labels[k];
        if (ign < 0 || ign > (int)list.size()) { set_error("randla_train_set_loss: ignored label %d outside 0 .. %d", ign, (int)list.size()); return SSDR_ERR_INVALID; }
        list.insert(list.begin() + ign, 0);
    }
    m->tb.nlab = (int)list.size();
    for (int c = 0; c < 64; ++c) { m->tb.remap[c] = c < (int)list.size() ? list[c] : 0; m->tb.ignored[c] = 0; }
    for (int k = 0; k < n_ignored; ++k) m->tb.ignored[ignored_labels[k]] = 1;
    for (int c = 0; c < 32; ++c) m->tb.cw[c] = (class_weights && c < m->C) ? class_weights[c] : 1.f;
    return SSDR_OK;
}

int ssdr_randla_train_set_lr(void* handle, float lr) {
    Train* m = static_cast<Train*>(handle);
    if (!m || !(lr >= 0.f)) { set_error("randla_train_set_lr: bad arguments"); return SSDR_ERR_INVALID; }
    m->lr = lr;
    return SSDR_OK;
}
int ssdr_randla_train_set_step_count(void* handle, int64_t t) {
    Train* m = static_cast<Train*>(handle);
    if (!m || t < 0) { set_error("randla_train_set_step_count: bad arguments"); return SSDR_ERR_INVALID; }
    m->step = (long)t;
    return SSDR_OK;
}
int64_t ssdr_randla_train_step_count(void* handle) { return handle ? (int64_t)static_cast<Train*>(handle)->step : -1; }
/* bytes of the activation + gradient workspaces laid out by the last call */
size_t ssdr_randla_train_workspace_bytes(void* handle) {
    Train* m = static_cast<Train*>(handle);
    return m ? (size_t)(m->act_floats + m->grad_floats) * 4 + (m->det && !m->dl.empty() ? m->det_bytes() : 0) + (m->act_floats ? (size_t)m->xchg_floats() * 4 : 0) : 0;
}

/* on != 0: the three backward scatters become reductions over inverse lists (scatter_det.hip), the same bits every run.  Off (the default) launches
 * the atomic kernels.  The workspace is planned again at the next call; when a shape has been planned already its new size is reported at once. */
int ssdr_randla_train_set_deterministic(void* handle, int on) {
    Train* m = static_cast<Train*>(handle);
    if (!m) { set_error("randla_train_set_deterministic: bad handle"); return SSDR_ERR_INVALID; }
    m->det = on != 0;
    if (m->det && !m->levels.empty()) det_layout(m, (long)m->planned_B, m->levels);
    return SSDR_OK;
}
int ssdr_randla_train_deterministic(void* handle) { return handle ? (static_cast<Train*>(handle)->det ? 1 : 0) : 0; }

/* Waits for the last forward / grads / step call of this handle; out3 = milliseconds of its forward, loss + backward and update parts (HIP events). */
int ssdr_randla_train_last_ms(void* handle, float* out3) {
    Train* m = static_cast<Train*>(handle);
    if (!m || !out3 || !m->ev_valid) { set_error("randla_train_last_ms: no finished call to report"); return SSDR_ERR_INVALID; }
    SSDR_HIP(hipEventSynchronize(m->ev[3]));
    for (int i = 0; i < 3; ++i) SSDR_HIP(hipEventElapsedTime(&out3[i], m->ev[i], m->ev[i + 1]));
    return SSDR_OK;
}

/* elements first .. first + n - 1 of the mask of (seed, step): a rank's slice of the union's mask */
int ssdr_randla_train_dropout_mask_range_dev(uint64_t seed, uint64_t step, uint64_t first, size_t n, uint8_t* d_mask, void* stream) {
    if (!d_mask || n == 0) { set_error("randla_train_dropout_mask: bad arguments"); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(blocks_for((long)n)), dim3(256), 0, pick_stream(stream), seed, step, first, (long)n, d_mask);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}
int ssdr_randla_train_dropout_mask_dev(uint64_t seed, uint64_t step, size_t n, uint8_t* d_mask, void* stream) {
    return ssdr_randla_train_dropout_mask_range_dev(seed, step, 0, n, d_mask, stream);
}

/* Data-parallel mode (include/ssdr_al.h): fn is called, on the calling thread, wherever the ranks must meet, and only enqueues on the call's stream.
 * fn NULL with world 1: back to one process. */
int ssdr_randla_train_set_exchange(void* handle, ssdr_exchange_fn fn, void* user, int rank, int world) {
    Train* m = static_cast<Train*>(handle);
    if (!m) { set_error("randla_train_set_exchange: bad handle"); return SSDR_ERR_INVALID; }
    if (world < 1 || rank < 0 || rank >= world) { set_error("randla_train_set_exchange: rank %d of world %d", rank, world); return SSDR_ERR_INVALID; }
    if (!fn && world > 1) { set_error("randla_train_set_exchange: world %d needs a callback", world); return SSDR_ERR_INVALID; }
    if (!fn) { m->xg = Exchange{}; return SSDR_OK; }
    // nothing that was enqueued may still use the buffers when they move
    SSDR_HIP(hipDeviceSynchronize());
    SSDR_TRY(m->xsend.reserve(sizeof(float) * (size_t)xchg_record_floats(m->cmax)));
    SSDR_TRY(m->xrecv.reserve(sizeof(float) * (size_t)world * (size_t)xchg_record_floats(m->cmax)));
    m->xg = Exchange{fn, user, rank, world};
    return SSDR_OK;
}
int ssdr_randla_train_exchange(void* handle, int* rank, int* world) {
    Train* m = static_cast<Train*>(handle);
    if (!m) { set_error("randla_train_exchange: bad handle"); return SSDR_ERR_INVALID; }
    if (rank) *rank = m->xg.rank;
    if (world) *world = m->xg.world;
    return SSDR_OK;
}

/* Forward, loss, backward, the moving statistics and one Adam update; enqueue only.  By default the scatter-adds are float atomics and the weights' low
 * bits depend on the run; not so after ssdr_randla_train_set_deterministic(handle, 1). */
int ssdr_randla_train_step_dev(void* handle, size_t B, size_t N, const float* d_features, const float* const* d_xyz, const int32_t* ratios,
                               const int32_t* const* d_neigh, const int32_t* const* d_pool, const int32_t* const* d_interp, const int32_t* d_labels,
                               const float* d_activation, const float* d_pseudo, const uint8_t* d_drop_mask, float* d_loss, float* d_accuracy, void* stream) {
    StepIn in{B, N, d_features, d_xyz, ratios, d_neigh, d_pool, d_interp, d_labels, d_activation, d_pseudo, d_drop_mask};
    return run(static_cast<Train*>(handle), in, 1, 3, nullptr, nullptr, d_loss, d_accuracy, stream, "randla_train_step");
}
/* Forward and backward without the update (neither the weights nor the moving statistics change): gradients through ssdr_randla_train_get_grad. */
int ssdr_randla_train_grads_dev(void* handle, size_t B, size_t N, const float* d_features, const float* const* d_xyz, const int32_t* ratios,
                                const int32_t* const* d_neigh, const int32_t* const* d_pool, const int32_t* const* d_interp, const int32_t* d_labels,
                                const float* d_activation, const float* d_pseudo, const uint8_t* d_drop_mask, float* d_loss, float* d_accuracy, void* stream) {
    StepIn in{B, N, d_features, d_xyz, ratios, d_neigh, d_pool, d_interp, d_labels, d_activation, d_pseudo, d_drop_mask};
    return run(static_cast<Train*>(handle), in, 1, 1, nullptr, nullptr, d_loss, d_accuracy, stream, "randla_train_grads");
}
/* The network alone: is_training = 1 batch statistics and dropout (the moving statistics stay), 0 moving statistics and no dropout. */
int ssdr_randla_train_forward_dev(void* handle, size_t B, size_t N, const float* d_features, const float* const* d_xyz, const int32_t* ratios,
                                  const int32_t* const* d_neigh, const int32_t* const* d_pool, const int32_t* const* d_interp, const uint8_t* d_drop_mask,
                                  int is_training, float* d_logits, float* d_feat32, void* stream) {
    if (!d_logits || !d_feat32) { set_error("randla_train_forward: NULL output"); return SSDR_ERR_INVALID; }
    StepIn in{B, N, d_features, d_xyz, ratios, d_neigh, d_pool, d_interp, nullptr, nullptr, nullptr, d_drop_mask};
    return run(static_cast<Train*>(handle), in, is_training, 0, d_logits, d_feat32, nullptr, nullptr, stream, "randla_train_forward");
}

/* Folds every batch norm with its moving statistics (float64 on the host) and loads the inference handle through ssdr_randla_set_layer. */
int ssdr_randla_train_export(void* handle, void* net) {
    Train* m = static_cast<Train*>(handle);
    if (!m || !net) { set_error("randla_train_export: bad arguments"); return SSDR_ERR_INVALID; }
    if (ssdr_randla_num_layers(net) != 1 + 8 * m->L + 1 + m->L + 3) { set_error("randla_train_export: the inference handle has another number of levels"); return SSDR_ERR_INVALID; }
    SSDR_HIP(hipDeviceSynchronize());
    std::vector<float> P((size_t)m->n_par), S((size_t)std::max<long>(m->n_stat, 1));
    SSDR_HIP(hipMemcpy(P.data(), m->P.p, sizeof(float) * P.size(), hipMemcpyDeviceToHost));
    if (m->n_stat) SSDR_HIP(hipMemcpy(S.data(), m->S.p, sizeof(float) * (size_t)m->n_stat, hipMemcpyDeviceToHost));
    auto fold = [&](int ui, std::vector<double>& W, std::vector<double>& b) {
        const Unit& u = m->units[ui];
        W.assign((size_t)u.in * u.out, 0.0); b.assign(u.out, 0.0);
        for (int k = 0; k < u.in; ++k) for (int c = 0; c < u.out; ++c) W[(size_t)k * u.out + c] = P[u.oW + (u.transposed ? (long)c * u.in + k : (long)k * u.out + c)];
        if (u.bias) for (int c = 0; c < u.out; ++c) b[c] = P[u.ob + c];
        if (u.bn) for (int c = 0; c < u.out; ++c) {
            const double sc = (double)P[u.og + c] / std::sqrt((double)S[u.ovar + c] + 1e-6);
            for (int k = 0; k < u.in; ++k) W[(size_t)k * u.out + c] *= sc;
            b[c] = (b[c] - (double)S[u.omean + c]) * sc + (double)P[u.obeta + c];
        }
    };
    auto put = [&](int layer, const std::vector<double>& W, const std::vector<double>& b, bool has_b) -> int {
        int in = 0, out = 0, hb = 0;
        SSDR_TRY(ssdr_randla_layer_shape(net, layer, &in, &out, &hb));
        if ((size_t)in * out != W.size() || (hb != 0) != has_b) { set_error("randla_train_export: layer %d of the inference handle has another shape", layer); return SSDR_ERR_INVALID; }
        std::vector<float> w32(W.begin(), W.end()), b32(b.begin(), b.end());
        return ssdr_randla_set_layer(net, layer, w32.data(), has_b ? b32.data() : nullptr);
    };
    std::vector<double> W, b, W2, b2;
    fold(0, W, b); SSDR_TRY(put(0, W, b, true));
    for (int i = 0; i < m->L; ++i) {
        for (int r = 0; r < 7; ++r) { fold(1 + 9 * i + r, W, b); SSDR_TRY(put(1 + 8 * i + r, W, b, m->units[1 + 9 * i + r].bias)); }
        fold(1 + 9 * i + 7, W, b); fold(1 + 9 * i + 8, W2, b2);
        W.insert(W.end(), W2.begin(), W2.end());
        for (size_t c = 0; c < b.size(); ++c) b[c] += b2[c];
        SSDR_TRY(put(1 + 8 * i + 7, W, b, true));
    }
    for (int l = 1 + 8 * m->L; l < 1 + 8 * m->L + 1 + m->L + 3; ++l) { fold(l + m->L, W, b); SSDR_TRY(put(l, W, b, true)); }
    return SSDR_OK;
}

/* ---- the launchers as stand-alone pieces (include/ssdr_al.h): the tile choice, the dW split and the reduction chunks are the step's own ---- */
int ssdr_randla_train_gemm_dev(const float* d_A, int64_t ars, int64_t acs, const float* d_B, int64_t brs, int64_t bcs, float* d_C, int64_t crs, int64_t ccs,
                               int M, int N, int K, const float* d_bias, int accumulate, void* stream) {
    if (!d_A || !d_B || !d_C) { set_error("randla_train_gemm: NULL pointer"); return SSDR_ERR_INVALID; }
    if (M <= 0 || N <= 0 || K <= 0) { set_error("randla_train_gemm: M = %d, N = %d, K = %d must be positive", M, N, K); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    return launch_gemm(pick_stream(stream), d_A, (long)ars, (long)acs, d_B, (long)brs, (long)bcs, d_C, (long)crs, (long)ccs, M, N, K, d_bias, accumulate != 0);
}

int ssdr_randla_train_dw_dev(const float* d_x, int ldx, const float* d_dz, int M, int in, int out, float* d_dW, int64_t rs, int64_t cs, void* stream) {
    if (!d_x || !d_dz || !d_dW) { set_error("randla_train_dw: NULL pointer"); return SSDR_ERR_INVALID; }
    if (M <= 0 || in <= 0 || out <= 0) { set_error("randla_train_dw: M = %d, in = %d, out = %d must be positive", M, in, out); return SSDR_ERR_INVALID; }
    if (ldx < in) { set_error("randla_train_dw: the leading dimension %d is below in = %d", ldx, in); return SSDR_ERR_INVALID; }
    if ((long)in * out > DWP_FLOATS) { set_error("randla_train_dw: in * out = %ld is more than one slab holds", (long)in * out); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    TrainPieces& sc = per_stream<TrainPieces>(s);
    SSDR_TRY(sc.dwp.reserve(sizeof(float) * (size_t)dw_split(M, in, out).nz * (size_t)in * (size_t)out));
    return launch_dw(s, d_x, ldx, d_dz, M, in, out, sc.dwp.as<float>(), d_dW, (long)rs, (long)cs);
}

/* mode 0: d_out0 = mean, d_out1 = 1 / sqrt(biased variance + 1e-6) of z's columns, and the moving averages when both are given.
 * mode 1: d_out0 = sum dY, d_out1 = sum dY xhat with dY = da (x 0.2 where act and not av > 0), xhat = (z - mean) invstd.   mode 2: d_out0 = sum z. */
int ssdr_randla_train_reduce_dev(int mode, const float* d_z, int ldz, const float* d_da, const float* d_av, int lda, int act, const float* d_mean,
                                 const float* d_invstd, int M, int C, float* d_out0, float* d_out1, float* d_mov_mean, float* d_mov_var, int unbiased,
                                 void* stream) {
    if (mode < RED_STATS || mode > RED_SUM) { set_error("randla_train_reduce: mode %d (0 statistics, 1 batch-norm backward, 2 sum)", mode); return SSDR_ERR_INVALID; }
    if (!d_z || !d_out0 || (mode != RED_SUM && !d_out1)) { set_error("randla_train_reduce: NULL pointer"); return SSDR_ERR_INVALID; }
    if (mode == RED_BNBWD && (!d_da || !d_mean || !d_invstd || (act && !d_av))) { set_error("randla_train_reduce: mode 1 needs da, mean, invstd (and av with act)"); return SSDR_ERR_INVALID; }
    if ((d_mov_mean == nullptr) != (d_mov_var == nullptr)) { set_error("randla_train_reduce: the moving mean and variance come together"); return SSDR_ERR_INVALID; }
    if (M <= 0 || C <= 0) { set_error("randla_train_reduce: M = %d, C = %d must be positive", M, C); return SSDR_ERR_INVALID; }
    if (ldz < C || (mode == RED_BNBWD && lda < C)) { set_error("randla_train_reduce: a leading dimension is below C = %d", C); return SSDR_ERR_INVALID; }
    if (2L * C > PART_FLOATS) { set_error("randla_train_reduce: C = %d is more than the partial buffer holds", C); return SSDR_ERR_INVALID; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    TrainPieces& sc = per_stream<TrainPieces>(s);
    SSDR_TRY(sc.part.reserve(sizeof(float) * 2 * (size_t)C * (size_t)red_split(M, C).nchunks));
    RedArgs a{}; a.z = d_z; a.ldz = ldz; a.da = d_da; a.av = d_av; a.lda = lda; a.act = act; a.mean = d_mean; a.invstd = d_invstd; a.M = M; a.C = C;
    if (mode == RED_STATS) { const int n = launch_reduce_chunks<RED_STATS>(s, a, sc.part.as<float>()); return launch_combine<RED_STATS>(s, a, n, d_out0, d_out1, d_mov_mean, d_mov_var, unbiased); }
    if (mode == RED_BNBWD) { const int n = launch_reduce_chunks<RED_BNBWD>(s, a, sc.part.as<float>()); return launch_combine<RED_BNBWD>(s, a, n, d_out0, d_out1, nullptr, nullptr, 0); }
    const int n = launch_reduce_chunks<RED_SUM>(s, a, sc.part.as<float>());
    return launch_combine<RED_SUM>(s, a, n, d_out0, nullptr, nullptr, nullptr, 0);
}

/* Waits for `stream`; the bits the training calls on it raised since the last call (bit 0: no valid row, loss and gradient are 0; bit 1: a label or pseudo
 * label outside the table) and clears them.  SSDR_ERR_INVALID when any is set. */
int ssdr_randla_train_status(void* stream, int32_t* out_status) {
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    int* w = status_word(s);
    if (!w) { set_error("randla_train_status: no status word"); return SSDR_ERR_HIP; }
    int v = 0;
    SSDR_HIP(hipMemcpyAsync(&v, w, sizeof(int), hipMemcpyDeviceToHost, s));
    SSDR_HIP(hipMemsetAsync(w, 0, sizeof(int), s));
    SSDR_HIP(hipStreamSynchronize(s));
    if (out_status) *out_status = v;
    if (v) { set_error("randla_train: status bits 0x%x (1: no valid row, 2: label outside the table)", v); return SSDR_ERR_INVALID; }
    return SSDR_OK;
}

}
