// Training-time generators for gfx950: what Network.train() reads, formed on the device from the resident clouds and the resident pseudo_gt.
//
//   ssdr_feed_chain_dev    Semantic3D_Dataset_Train.get_batch (SSRD_AL_semantic3d/semantic3d_dataset_train.py:151-210): the possibility chain of
//                          vote.hip with the options that loop needs (x / y centring, class-weighted update, local rows, the two channels)
//   ssdr_feed_tiles_dev    S3DIS_Dataset.spatially_regular_gen, mode "training" (SSDR_AL_s3dis/s3dis_dataset.py:115-154): tiles that do not depend on
//                          each other, any cloud per tile, the centre formed on the device; vote.hip's kernels with the tile on blockIdx.y
//   ssdr_feed_augment_dev  tf_augment_input (semantic3d_dataset_train.py:237-276): rotation about z, scale, symmetry, noise, in float64
//   ssdr_feed_prefix_dev   the sub-sampled xyz levels of tf_map (:221): per-element prefixes, copied out
//
// The launchers of the first two live with their kernels in vote.hip (vote_chain.hpp); this file holds the entry points and the two streaming
// kernels.
#include "ssdr_internal.hpp"
#include "vote_chain.hpp"

namespace ssdr {
namespace {

constexpr int AUG_PER = 4;      // points per thread: a workgroup covers 1024 points of ONE tile, whose five parameters it reads once

// (x . R) with R = [[c, -s, 0], [s, c, 0], [0, 0, 1]] as np.matmul's plain dot product orders it, (x R0j + y R1j) + z R2j, the products with R's
// zeros and its one included (they are exact; -0 and non-finite inputs come out as the reference's).  No contraction: the build sets -ffp-contract=off.
__global__ __launch_bounds__(256) void feed_augment(const float* __restrict__ xyz, int num_points, const double* __restrict__ rot, const double* __restrict__ scale,
                                                    const double* __restrict__ noise, int fdim, float* feat) {
    const size_t t = blockIdx.y;
    const double c = rot[2 * t], s = rot[2 * t + 1], ns = -s;
    const double s0 = scale[3 * t], s1 = scale[3 * t + 1], s2 = scale[3 * t + 2];
    const float* X = xyz + 3 * t * num_points;
    const double* Z = noise ? noise + 3 * t * num_points : nullptr;
    float* F = feat + t * num_points * fdim;
#pragma unroll
    for (int u = 0; u < AUG_PER; ++u) {
        const int i = (blockIdx.x * AUG_PER + u) * 256 + threadIdx.x;
        if (i >= num_points) break;
        const double x = (double)X[3 * (size_t)i], y = (double)X[3 * (size_t)i + 1], z = (double)X[3 * (size_t)i + 2];
        double r0 = ((x * c + y * s) + z * 0.0) * s0;
        double r1 = ((x * ns + y * c) + z * 0.0) * s1;
        double r2 = ((x * 0.0 + y * 0.0) + z * 1.0) * s2;
        if (Z) { r0 = r0 + Z[3 * (size_t)i]; r1 = r1 + Z[3 * (size_t)i + 1]; r2 = r2 + Z[3 * (size_t)i + 2]; }
        float* f = F + (size_t)i * fdim;
        f[0] = (float)r0; f[1] = (float)r1; f[2] = (float)r2;
    }
}

// out[t, :num_sub] = xyz[t, :num_sub]: 3 num_sub floats per tile, consecutive on both sides
__global__ __launch_bounds__(256) void feed_prefix(const float* __restrict__ xyz, size_t in_stride, int n_out, float* out) {
    const float* X = xyz + blockIdx.y * in_stride;
    float* O = out + (size_t)blockIdx.y * n_out;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_out; i += gridDim.x * 256) O[i] = X[i];
}

}  // namespace
}  // namespace ssdr

using namespace ssdr;

extern "C" int ssdr_feed_chain_dev(const float* d_points, const float* d_colors, int color_dim, const int32_t* d_labels, double* d_possibility,
                                   double* d_cloud_min, int32_t* d_cloud_arg, const int64_t* cloud_offsets, size_t num_clouds,
                                   size_t num_tiles, size_t num_points, const float* d_noise, const int32_t* d_perm, const float* d_dup_u, float color_scale,
                                   float* d_out_xyz, float* d_out_feat, int32_t* d_out_idx, int32_t* d_out_labels, int32_t* d_out_cloud, float* d_out_center,
                                   int flags, const double* d_class_weight, int num_labels, const float* d_activation, const float* d_pseudo,
                                   float* d_out_activation, float* d_out_pseudo, void* stream) {
    if (flags & ~(SSDR_FEED_XY_ONLY | SSDR_FEED_GLOBAL_ROWS)) { set_error("feed_chain: unknown flags 0x%x", flags); return SSDR_ERR_INVALID; }
    ChainArgs a = {};
    a.points = d_points; a.colors = d_colors; a.color_dim = color_dim; a.labels = d_labels; a.possibility = d_possibility; a.cloud_min = d_cloud_min; a.cloud_arg = d_cloud_arg;
    a.cloud_offsets = cloud_offsets; a.num_clouds = num_clouds; a.num_tiles = num_tiles; a.num_points = num_points; a.noise = d_noise; a.perm = d_perm; a.dup_u = d_dup_u;
    a.color_scale = color_scale; a.out_xyz = d_out_xyz; a.out_feat = d_out_feat; a.out_idx = d_out_idx; a.out_labels = d_out_labels; a.out_cloud = d_out_cloud;
    a.out_center = d_out_center; a.flags = flags; a.class_weight = d_class_weight; a.num_labels = num_labels;
    a.activation = d_activation; a.pseudo = d_pseudo; a.out_activation = d_out_activation; a.out_pseudo = d_out_pseudo;
    return vote_chain_launch("feed_chain", a, stream);
}

extern "C" int ssdr_feed_tiles_dev(const float* d_points, const float* d_colors, int color_dim, const int32_t* d_labels, const float* d_activation,
                                   const float* d_pseudo, const int64_t* cloud_offsets, size_t num_clouds, size_t num_tiles, size_t num_points,
                                   const int32_t* d_tile_cloud, const int32_t* d_tile_point, const float* d_noise, const int32_t* d_perm, const float* d_dup_u,
                                   float color_scale, float* d_out_xyz, float* d_out_feat, int32_t* d_out_idx, int32_t* d_out_labels, float* d_out_activation,
                                   float* d_out_pseudo, int32_t* d_out_cloud, float* d_out_center, void* stream) {
    ChainArgs a = {};
    a.points = d_points; a.colors = d_colors; a.color_dim = color_dim; a.labels = d_labels; a.cloud_offsets = cloud_offsets; a.num_clouds = num_clouds;
    a.num_tiles = num_tiles; a.num_points = num_points; a.noise = d_noise; a.perm = d_perm; a.dup_u = d_dup_u; a.color_scale = color_scale;
    a.out_xyz = d_out_xyz; a.out_feat = d_out_feat; a.out_idx = d_out_idx; a.out_labels = d_out_labels; a.out_center = d_out_center; a.out_cloud = d_out_cloud;
    a.activation = d_activation; a.pseudo = d_pseudo; a.out_activation = d_out_activation; a.out_pseudo = d_out_pseudo;
    a.tile_cloud = d_tile_cloud; a.tile_point = d_tile_point;
    return vote_indep_launch("feed_tiles", a, stream);
}

extern "C" int ssdr_feed_augment_dev(const float* d_xyz, size_t num_tiles, size_t num_points, const double* d_rot, const double* d_scale, const double* d_noise,
                                     int color_dim, float* d_feat, void* stream) {
    if (!d_xyz || !d_rot || !d_scale || !d_feat || color_dim < 0) { set_error("feed_augment: bad arguments"); return SSDR_ERR_INVALID; }
    if (num_tiles == 0 || num_points == 0) { set_error("feed_augment: num_tiles and num_points must be positive"); return SSDR_ERR_INVALID; }
    if (num_tiles > 65535 || num_points > 0x3fffffff / num_tiles) { set_error("feed_augment: more than 65535 tiles or 0x3fffffff rows"); return SSDR_ERR_UNSUPPORTED; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    const unsigned gx = (unsigned)((num_points + 256 * AUG_PER - 1) / (256 * AUG_PER));
    ProfScope prof("feed_augment", s, (double)num_tiles * (double)num_points * (24.0 + (d_noise ? 24.0 : 0.0)));
    hipLaunchKernelGGL(feed_augment, dim3(gx, (unsigned)num_tiles), dim3(256), 0, s, d_xyz, (int)num_points, d_rot, d_scale, d_noise, 3 + color_dim, d_feat);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

extern "C" int ssdr_feed_prefix_dev(const float* d_xyz, size_t num_tiles, size_t num_points, size_t num_sub, float* d_out, void* stream) {
    if (!d_xyz || !d_out) { set_error("feed_prefix: bad arguments"); return SSDR_ERR_INVALID; }
    if (num_tiles == 0 || num_sub == 0 || num_sub > num_points) { set_error("feed_prefix: 0 < num_sub <= num_points, num_tiles > 0"); return SSDR_ERR_INVALID; }
    if (num_tiles > 65535 || num_points > 0x3fffffff / num_tiles) { set_error("feed_prefix: more than 65535 tiles or 0x3fffffff rows"); return SSDR_ERR_UNSUPPORTED; }
    SSDR_TRY(ensure_init());
    hipStream_t s = pick_stream(stream);
    const int n_out = (int)(3 * num_sub);
    hipLaunchKernelGGL(feed_prefix, dim3((unsigned)std::max(1, std::min((n_out + 255) / 256, 64)), (unsigned)num_tiles), dim3(256), 0, s, d_xyz, 3 * num_points, n_out, d_out);
    SSDR_HIP(hipGetLastError());
    return SSDR_OK;
}

extern "C" int ssdr_feed_status(void* stream, int32_t* out_status) { return vote_status(stream, out_status); }
