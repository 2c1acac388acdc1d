// The farthest-point / k-center family (select_fps.hip): what select.hip's one-call chains and select_region.hip need of it.
#pragma once
#include "ssdr_internal.hpp"

namespace ssdr {

// the arg-max rule of every selection chain
__device__ __forceinline__ bool better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }   // np.argmax: first maximum

inline int grid_for(long n, int cap = 2048) { return (int)std::max<long>(1, std::min<long>((n + 255) / 256, cap)); }

// farthest_features_sample (fps_gcn_cpu.py:119-147; d_already == nullptr: `count` picks from row `start`, squared distances) / kCenterGreedy
// (kcenterGreedy.py:84-128; seeded with the `na` rows of d_already, use_sqrt = 1) over d_feat [n, D], enqueued on s.  d_n (optional): the row count on
// the device; n is then the bound the launch shapes are chosen by.  A cooperative form that was not co-resident reports through ssdr_select_status.
int fps_like(const double* d_feat, size_t n, int D, const int32_t* d_already, size_t na, int start, size_t count, int use_sqrt, int32_t* d_out, hipStream_t s,
             const int* d_n = nullptr);

}  // namespace ssdr
