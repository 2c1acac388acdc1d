// The bucket partition + per-bucket LDS reduction (frontend.hip: rows of at most 7 words, grids of at most 16384 buckets of 1024 voxels): what subsample.hip's
// entry points need of it.
#pragma once
#include "ssdr_internal.hpp"
#include "subsample_types.hpp"

namespace ssdr {

bool frontend_fits(size_t fdim, size_t ldim);

// All clouds of a batch in the same launches on s; prm: the caller's per-cloud GsParams.  centres (host [nr, 3]) / num_points: the staged reduction, which leaves
// out the buckets that cannot hold one of the num_points rows nearest to a room's centre; NULL: every bucket.  plan (optional, with centres only): see below
struct FePlan;          // a room plan: what the partition derives from the rooms' points and dl alone, kept between calls
int frontend_batch_device(const float* d_p, const float* d_f, size_t fdim, const int32_t* d_c, size_t ldim, const int64_t* room_off, size_t nr, float dl,
                          float* d_op, float* d_of, int32_t* d_oc, int64_t* d_om, GsParams* prm, hipStream_t s, const float* centres, size_t num_points, const FePlan* plan);

int frontend_plan_build(const float* d_p, const float* d_f, size_t fdim, const int32_t* d_c, size_t ldim, const int64_t* room_off, size_t nr, float dl, hipStream_t s,
                        FePlan** out);
int frontend_plan_destroy(FePlan* plan);
void frontend_plan_info(const FePlan* plan, int64_t* record_bytes, int32_t* sorted);
int frontend_plan_check(const FePlan* plan, const float* d_p, const float* d_f, size_t fdim, const int32_t* d_c, size_t ldim, const int64_t* room_off, size_t nr, float dl);

// the last staged call on s, per room (both wait for the stream); a call that was not staged: -1 everywhere.  forget: the last call on s no longer counts as staged
int frontend_tile_stats(hipStream_t s, int32_t* stage, int32_t* reduced, int32_t* buckets, size_t nr);
int frontend_scatter_stats(hipStream_t s, int64_t* scattered, int64_t* points, size_t nr);
void frontend_tile_forget(hipStream_t s);

}  // namespace ssdr
