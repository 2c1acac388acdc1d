// The trained-GCN selector (select_gcn.hip): what select.hip's one-call chain needs of it.
#pragma once
#include "ssdr_internal.hpp"

namespace ssdr {

// Scratch of the one-call chain (ssdr_gcn_sampling_dev) per stream: what the accessor hands out afterwards.
struct GcnChainBufs {
    float* feat = nullptr;      // [cap_rows, 32] compute_features rows (candidates, then labelled regions)
    float* v = nullptr;         // [cap_rows, 32] normalised
    float* adj = nullptr;       // [cap_sq] blocks
    float* adjT = nullptr;      // [cap_sq] their transposes
    float* params = nullptr;    // [SSDR_GCN_NPARAM] trained
    float* loss = nullptr;      // [2]
    double* rows129 = nullptr;  // [cap_rows, 129]
    int32_t* info = nullptr;    // [8]
    size_t cap_rows = 0;
};
int gcn_chain_buffers(hipStream_t s, size_t cap_rows, size_t cap_sq, GcnChainBufs& B);
const GcnChainBufs* gcn_chain_last(hipStream_t s);

// d_info[0] |= bits 32 / 64 into counts[5] of a chain's result (128, values substituted, is no failure and stays in d_info)
int gcn_merge_status(const int32_t* d_info, int32_t* d_counts, hipStream_t s);

}  // namespace ssdr
