// Data-parallel training (train_exchange.hip): what randla_train.hip enqueues on either side of a collective when an exchange callback is set, and the
// three exported pieces (ssdr_bn_stats_merge_dev, ssdr_rank_sums_merge_dev, the range-table zeroing behind the gradient sum).
// Every merge walks the ranks' records in rank order from 0, one work-item per channel: the same bits on every rank, and a NumPy restatement is exact.
#pragma once
#include "ssdr_internal.hpp"

namespace ssdr {

struct Exchange { ssdr_exchange_fn fn = nullptr; void* user = nullptr; int rank = 0, world = 0; };      // world 0: none set

// floats of one batch-norm record [n | mean[C] | M2[C]]
inline long xchg_record_floats(int C) { return 1 + 2L * C; }

// Chan's merge of this rank's row chunks (reduce_kernel<RED_STATS>'s partials [nchunks][2][C], the operations of combine_kernel<RED_STATS>) into the
// record [(float)M | mean[C] | M2[C]]
int xchg_pack_stats(const float* part, int nchunks, int chunk, int M, int C, float* record, hipStream_t s);
// sums of the chunks' two partial values per channel into out [first[C] | second[C]] when swap == 0, [second[C] | first[C]] when swap != 0
int xchg_pack_sums(const float* part, int nchunks, int C, float* out, int swap, hipStream_t s);
// records [world][1 + 2C] -> mean, 1 / sqrt(biased var + eps), the global row count (one float) and, when mov_mean is not NULL, the moving statistics
int xchg_merge_stats(const float* records, int world, int C, float* mean, float* invstd, float* count, float* mov_mean, float* mov_var, int unbiased, hipStream_t s);
// out[i] = ((0 + r0[i]) + r1[i]) + ...   records [world][n]
int xchg_merge_sums(const float* records, int world, int n, float* out, hipStream_t s);
// g[off .. off + len) = 0 for every (off, len) pair of table [n_ranges][2]
int xchg_zero_ranges(float* g, const long* d_table, int n_ranges, hipStream_t s);

}  // namespace ssdr
