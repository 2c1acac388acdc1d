// The generator chain's launchers (vote.hip), shared by the test-time entry (ssdr_vote_tiles_dev) and the training-time entries (feed.hip).
#pragma once
#include "ssdr_internal.hpp"

namespace ssdr {

struct ChainArgs {
    const float* points; const float* colors; int color_dim; const int32_t* labels;
    const int64_t* cloud_offsets; size_t num_clouds, num_tiles, num_points;
    const float* noise; const int32_t* perm; const float* dup_u; float color_scale;
    float* out_xyz; float* out_feat; int32_t* out_idx; int32_t* out_labels; float* out_center;
    const float* activation; const float* pseudo; float* out_activation; float* out_pseudo;
    int flags;                                                       // SSDR_FEED_*
    // the chain alone: the map and its per-cloud state, the class weights
    double* possibility; double* cloud_min; int32_t* cloud_arg; int32_t* out_cloud; const double* class_weight; int num_labels;
    // independent tiles alone: every tile's cloud and point
    const int32_t* tile_cloud; const int32_t* tile_point;
};

// status bits of a stream's chain / feed calls (ssdr_feed_status)
constexpr int FEED_ST_LABEL = 1, FEED_ST_CLOUD = 2, FEED_ST_POINT = 4;

int vote_chain_launch(const char* who, const ChainArgs& a, void* stream);      // tiles in order, tile t + 1 reading what tile t left
int vote_indep_launch(const char* who, const ChainArgs& a, void* stream);      // all tiles in one set of launches, tile = blockIdx.y
int vote_status(void* stream, int32_t* out_status);

}  // namespace ssdr
