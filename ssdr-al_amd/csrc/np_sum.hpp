// NumPy's summation orders on the device.  Where a NumPy reduction of the reference decides a discrete outcome (the arg-max chain of FPS, the ranking of the
// regions) the kernels of select.hip and select_fps.hip add in the same order, so that identical inputs give the identical result.
#pragma once
#include <hip/hip_runtime.h>

namespace ssdr {

// NumPy's pairwise summation (numpy/_core/src/umath/loops_utils.h.src, @TYPE@_pairwise_sum) over get(i), i in [0,n)
template <class T, class Get>
__device__ T np_pairwise(Get get, int n) {
    // iterative version of the recursion: blocks are produced left to right; partial sums are combined exactly
    // like the call tree sum(a[:n2]) + sum(a[n2:]) with n2 = n/2 - (n/2)%8.
    struct Fr { int lo, n; int state; T left; };
    Fr st[24]; int sp = 0; T ret = T(0);
    st[0] = Fr{0, n, 0, T(0)};
    while (sp >= 0) {
        Fr& f = st[sp];
        if (f.n <= 128) {
            T res;
            if (f.n < 8) { res = T(0); for (int i = 0; i < f.n; ++i) res += get(f.lo + i); }
            else {
                T r[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) r[j] = get(f.lo + j);
                int i = 8;
                for (; i < f.n - (f.n % 8); i += 8) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) r[j] += get(f.lo + i + j);
                }
                res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                for (; i < f.n; ++i) res += get(f.lo + i);
            }
            ret = res; --sp;
        } else if (f.state == 0) {
            int n2 = f.n / 2; n2 -= n2 % 8;
            f.state = 1; st[sp + 1] = Fr{f.lo, n2, 0, T(0)}; ++sp;
        } else if (f.state == 1) {
            int n2 = f.n / 2; n2 -= n2 % 8;
            f.left = ret; f.state = 2; st[sp + 1] = Fr{f.lo + n2, f.n - n2, 0, T(0)}; ++sp;
        } else { ret = f.left + ret; --sp; }
    }
    return ret;
}

// Same summation order for a compile-time length 8 <= D <= 128 that is a multiple of 8 (fully unrolled: the 32-d
// feature distance of farthest_features_sample).
template <int D, class Get>
__device__ __forceinline__ double np_pairwise_fixed(Get get) {
    static_assert(D >= 8 && D <= 128 && D % 8 == 0, "np_pairwise_fixed");
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = get(j);
#pragma unroll
    for (int i = 8; i < D; i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += get(i + j);
    }
    return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
}

// The same order for one block of 8 <= n <= 128 terms with the eight accumulators on eight lanes of a wave (every lane of the wave calls it with uniform
// n; result on lane 0): lane k sums the terms k, k + 8, ... of the multiple-of-eight part, the accumulators are combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7))
// through lane exchanges (fp addition is commutative, so lane 0's a + b is the reference's), the leftover terms are added by lane 0 in order.
template <class T, class Get>
__device__ __forceinline__ T np_pairwise_w8(Get get, int n, int lane) {
    const int n8 = n - (n % 8);
    T r = T(0);
    if (lane < 8) { r = get(lane); for (int i = 8; i < n8; i += 8) r += get(i + lane); }
    auto xchg = [&](T v, int m) -> T {
        if constexpr (sizeof(T) == 8) {
            const long long b = __double_as_longlong((double)v);
            const unsigned lo = __shfl_xor((unsigned)b, m), hi = __shfl_xor((unsigned)(b >> 32), m);
            return (T)__longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
        } else return (T)__shfl_xor((float)v, m);
    };
    r = r + xchg(r, 1); r = r + xchg(r, 2); r = r + xchg(r, 4);
    if (lane == 0) for (int i = n8; i < n; ++i) r += get(i);
    return r;
}

// The whole recursion with every block of at most 128 terms summed by np_pairwise_w8 (uniform n over the wave; result on lane 0): the call tree
// sum(a[:n2]) + sum(a[n2:]) is walked by all lanes alike, only its leaves use the eight lanes.  A superpoint of 185 points is two such blocks of ~12 dependent
// additions per lane instead of 185 on one lane.
template <class T, class Get>
__device__ T np_pairwise_wave(Get get, int n, int lane) {
    struct Fr { int lo, n; int state; T left; };
    Fr st[24]; int sp = 0; T ret = T(0);
    st[0] = Fr{0, n, 0, T(0)};
    while (sp >= 0) {
        Fr& f = st[sp];
        if (f.n <= 128) {
            T res = T(0);
            const int lo = f.lo;
            if (f.n < 8) { if (lane == 0) for (int i = 0; i < f.n; ++i) res += get(lo + i); }
            else res = np_pairwise_w8<T>([&](int i) { return get(lo + i); }, f.n, lane);
            ret = res; --sp;
        } else if (f.state == 0) {
            int n2 = f.n / 2; n2 -= n2 % 8;
            f.state = 1; st[sp + 1] = Fr{f.lo, n2, 0, T(0)}; ++sp;
        } else if (f.state == 1) {
            int n2 = f.n / 2; n2 -= n2 % 8;
            f.left = ret; f.state = 2; st[sp + 1] = Fr{f.lo + n2, f.n - n2, 0, T(0)}; ++sp;
        } else { ret = f.left + ret; --sp; }
    }
    return ret;
}

// The same recursion for MORE terms than a wave can stage at once: the call tree is walked down to nodes of at most `cap` terms; such a node's terms are staged
// by all lanes (stage(lo, n): terms lo .. lo + n - 1 into slots 0 .. n - 1) and summed by np_pairwise_wave over the staged values — exactly the sub-call
// sum(a[lo:lo+n]) of the reference's recursion.  Two sums over the same members (WetSU's) share the walk and the staging.  Results on lane 0.
template <class T, class Stage, class GetA, class GetB>
__device__ void np_pairwise_wave_chunked2(Stage stage, GetA get_a, GetB get_b, bool two, int n, int lane, int cap, T& out_a, T& out_b) {
    struct Fr { int lo, n; int state; T left_a, left_b; };
    Fr st[24]; int sp = 0; T ra = T(0), rb = T(0);
    st[0] = Fr{0, n, 0, T(0), T(0)};
    while (sp >= 0) {
        Fr& f = st[sp];
        if (f.n <= cap) {
            stage(f.lo, f.n);
            if (f.n >= 8) { ra = np_pairwise_wave<T>(get_a, f.n, lane); if (two) rb = np_pairwise_wave<T>(get_b, f.n, lane); }
            else { ra = np_pairwise<T>(get_a, f.n); if (two) rb = np_pairwise<T>(get_b, f.n); }
            --sp;
        } else if (f.state == 0) {
            int n2 = f.n / 2; n2 -= n2 % 8;
            f.state = 1; st[sp + 1] = Fr{f.lo, n2, 0, T(0), T(0)}; ++sp;
        } else if (f.state == 1) {
            int n2 = f.n / 2; n2 -= n2 % 8;
            f.left_a = ra; f.left_b = rb; f.state = 2; st[sp + 1] = Fr{f.lo + n2, f.n - n2, 0, T(0), T(0)}; ++sp;
        } else { ra = f.left_a + ra; rb = f.left_b + rb; --sp; }
    }
    out_a = ra; out_b = rb;
}

}  // namespace ssdr
