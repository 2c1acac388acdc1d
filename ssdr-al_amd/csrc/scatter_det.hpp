// Atomic-free backward scatters (scatter_det.hip): inverse lists of an index array and the two reductions that walk them in a fixed order.
// What randla_train.hip's deterministic mode and the two exported pieces (ssdr_scatter_add_rows_dev, ssdr_pool_grad_rows_dev) share.
#pragma once
#include "ssdr_internal.hpp"

namespace ssdr {

// Inverse lists of idx [B][rows_per_b] into src_rows rows per batch element: pos[off[q] .. off[q + 1]) are the positions r (ascending) whose
// clamped index is row q = b * src_rows + j.  off has B * src_rows + 1 entries, pos B * rows_per_b.
struct InvList { int* off = nullptr; int* pos = nullptr; };

inline long inv_pad(long n) { return (n + 63) / 64 * 64; }
inline long inv_off_ints(long B, long src_rows) { return inv_pad(B * src_rows + 1); }
inline long inv_pos_ints(long B, long rows_per_b) { return inv_pad(B * rows_per_b); }

// Builds the lists on s.  keys: scratch for B * rows_per_b u64 words (free again when the call's launches have run); the sorter's own scratch grows
// to the same number of slots.  The contents are a function of idx alone: a stable radix sort of (q, r), no atomic anywhere.
int inv_list_build(const int32_t* idx, int B, int rows_per_b, int src_rows, uint64_t* keys, InvList l, RadixSorter& sorter, hipStream_t s);

// dsrc[q, c] += sum over the row's list, ascending, of dout[(b, r), c]; one work-item per (q, c), a row with an empty list keeps its value
int scatter_rows_det(InvList l, int B, int rows_per_b, int src_rows, const float* dout, int ldo, int C, float* dsrc, int lds, hipStream_t s);

// random_sample backward: share [B m_per_b, C] (scratch) takes dout / ties per (m, c), then the same walk adds the shares of the tied positions
int pool_grad_det(InvList l, const float* src, float* dsrc, int lds, int src_rows, const int32_t* idx, int B, int m_per_b, int C, const float* out,
                  const float* dout, int ldo, float* share, hipStream_t s);

}  // namespace ssdr
