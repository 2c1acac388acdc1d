/* ssdr_al.h — C ABI of libssdr_al.so, the MI355X (gfx950) implementation of the SSDR-AL hot path
 *
 *     grid-subsample -> KNN pyramid -> RandLA-Net inference -> FPS-GCN / k-center selection
 *
 * Plain pointers and sizes only; no C++ or torch types.  Every entry point returns an int status
 * (SSDR_OK == 0); ssdr_last_error() gives the message for the calling thread's last failure.
 *
 * Two flavours of each op:
 *   host entry points   take host pointers, are synchronous, and are the drop-in replacements for the
 *                       reference's native modules (they copy in, run the HIP kernels, copy out);
 *   *_dev entry points  take device pointers + a HIP stream handle (void*, NULL = the library's own
 *                       stream), enqueue only, and let a caller keep tiles resident in HBM between
 *                       stages.  Outputs are valid after the stream is synchronised
 *                       (ssdr_stream_sync).
 *
 * There is no CPU fallback: without a HIP device every compute entry point fails with
 * SSDR_ERR_NO_DEVICE.
 *
 * Reference interfaces are cited relative to /root/reference/SSDR_AL_s3dis/ ("S3/").
 */
#ifndef SSDR_AL_H
#define SSDR_AL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSDR_OK               0
#define SSDR_ERR_INVALID      1   /* bad argument (shape, NULL, unsupported dim/K) */
#define SSDR_ERR_NO_DEVICE    2   /* no HIP device / HIP runtime failure at init */
#define SSDR_ERR_HIP          3   /* a HIP call failed */
#define SSDR_ERR_EMPTY        4   /* empty result (reference: RuntimeError("Error"), wrapper.cpp:225-229) */
#define SSDR_ERR_UNSUPPORTED  5   /* valid for the reference but outside what the kernels cover */
#define SSDR_ERR_INTERNAL     6   /* device-side consistency flag raised (e.g. kd-tree deeper than the search stack) */

/* ---- library / device ---------------------------------------------------------------------- */
const char* ssdr_version(void);
const char* ssdr_last_error(void);
int  ssdr_init(int device);              /* idempotent; selects the HIP device, creates stream + workspace */
void ssdr_shutdown(void);
int  ssdr_stream_sync(void* stream);     /* NULL = library stream */
/* Extra streams for callers that overlap independent work (e.g. the per-room front end); every *_dev entry point
 * keeps its workspaces per stream, so calls on different streams may run concurrently. */
int  ssdr_stream_create(void** out_stream);
/* priority > 0: the device's highest stream priority, < 0: its lowest, 0: the default (hipStreamCreateWithPriority, non-blocking).  Streams of
 * another priority live on hardware queues of their own: short dependent launches are not held behind the other streams' chip-filling kernels. */
int  ssdr_stream_create_priority(void** out_stream, int priority);
int  ssdr_stream_destroy(void* stream);
int  ssdr_main_stream(void** out_stream);            /* the library's own stream (what stream == NULL means) */
int  ssdr_stream_wait(void* waiter, void* waited);   /* waiter continues after what is enqueued on waited so far */
/* events: ssdr_event_record marks a point in a stream's work; ssdr_stream_wait_event makes a stream wait for that point (issued any time later) */
int  ssdr_event_create(void** ev);
int  ssdr_event_record(void* ev, void* stream);
int  ssdr_stream_wait_event(void* stream, void* ev);
int  ssdr_event_destroy(void* ev);
/* Optional per-launch timing (HIP events on the launch stream) of the instrumented kernels; used by bench.py for
 * the roofline line.  ssdr_prof_report() synchronises and returns "name calls total_ms total_work total_work2\n" lines, where
 * total_work is the summed algorithmic FLOPs (MFMA kernels) or bytes (HBM kernels) of those launches and total_work2 the FLOPs
 * their MFMA instructions execute (0 for the other kernels). */
int ssdr_prof_enable(int on);
const char* ssdr_prof_report(void);
/* Milliseconds spent in the GPU part of the last host-flavour call (HIP events on the library stream). */
float ssdr_last_gpu_ms(void);

/* ---- KNN (replaces S3/utils/nearest_neighbors: knn_.h:4-26, knn_.cxx:22-135, knn.pyx:33-109) --
 * Exact K nearest neighbours of every query among `npts` support points, ascending squared
 * distance, with nanoflann v1.2.3's tie order (kd-tree traversal order, leaf size 10), i.e. the
 * int64 indices equal the reference's cpp_knn* output bit for bit.  dim must be 3; the host entry points also take dim 1 and 2 (answered exactly as the
 * 3-D problem with the missing coordinates at zero); dim > 3: SSDR_ERR_UNSUPPORTED.
 * If K > npts the slots >= npts hold 0 (what the reference's zero-initialised buffers leave there).
 * ssdr_knn           <-> cpp_knn / cpp_knn_omp              (knn_.cxx:22-69)
 * ssdr_knn_batch     <-> cpp_knn_batch / cpp_knn_batch_omp  (knn_.cxx:72-135)
 */
int ssdr_knn(const float* points, size_t npts, size_t dim,
             const float* queries, size_t nqueries, size_t K, int64_t* indices);
int ssdr_knn_batch(const float* batch_data, size_t batch_size, size_t npts, size_t dim,
                   const float* queries, size_t nqueries, size_t K, int64_t* batch_indices);
/* Same, but int32 output: the dtype DataProcessing.knn_search hands on (S3/helper_tool.py:173-183). */
int ssdr_knn_batch_i32(const float* batch_data, size_t batch_size, size_t npts, size_t dim,
                       const float* queries, size_t nqueries, size_t K, int32_t* batch_indices);
/* Device flavour: d_* are device pointers; out is int32 [B,nq,K]. */
int ssdr_knn_batch_dev(const float* d_batch_data, size_t batch_size, size_t npts, size_t dim,
                       const float* d_queries, size_t nqueries, size_t K, int32_t* d_indices, void* stream);
/* The device flavours (ssdr_knn_batch_dev, ssdr_knn_pyramid_dev) only enqueue work, so they cannot report what the kernels
 * found.  ssdr_knn_status waits for `stream` and returns SSDR_ERR_INTERNAL if the last KNN call issued on it overflowed one of
 * its device-side capacities (kd queue / node table / level limit, hand-over list); the host flavours check this themselves.
 * out4 (optional, host): rows handed from the grid search to the exact tree walk for K = 16 and K = 1 (tie rows, see
 * csrc/knn_grid.hip), the status bits, and the depth of the deepest tree built. */
int ssdr_knn_status(void* stream, int32_t* out4);
/* The same check without waiting: every device-flavour KNN call leaves a ticket (its counters copied to pinned memory behind its
 * kernels); this folds the tickets of the calls that HAVE finished and returns SSDR_ERR_INTERNAL if one of them overflowed.  For
 * callers that keep several batches in flight on `stream` and must not wait for the newest one (ssdr_al/pipeline.py). */
int ssdr_knn_status_poll(void* stream, int32_t* out4);
/* Read-only view of what the newest KNN call on `stream` counted on the device (waits for the stream; folds and clears nothing, so
 * ssdr_knn_status / _poll report afterwards as if it had not been called).  out16 (host): [0], [1] rows handed to the tree walk (K = 16, K = 1),
 * [2] grid status bits, [3] rows that left the grid unsettled, [4], [5] rows of the second pass, [6] balls, [7] unused, [8], [9] rows answered
 * again on complete trees, [10..12] the forest's words (-, status, deepest tree), [13..15] zero.  After a call without a grid [0..9] are zero.
 * desc_out (optional, host float[12]): n, c, nx, ny, nz, lo[3], hi[3], slack of support set `set` of that call's grid, as the device
 * computed them; left untouched when the call had no such set.  The integers n, nx, ny, nz travel as float: exact up to 2^24, rounded above. */
int ssdr_knn_counters(void* stream, int32_t* out16, size_t set, float* desc_out);

/* ---- KNN pyramid (replaces the loop of tf_map, S3/s3dis_dataset.py:156-183) ------------------
 * For level i in [0,num_layers): N_0 = npts, N_{i+1} = N_i / ratio[i] (integer division);
 *   neigh_idx[i]  int32 [B,N_i,K]       = knn(xyz[:, :N_i], xyz[:, :N_i], K)
 *   sub_idx[i]    int32 [B,N_{i+1},K]   = neigh_idx[i][:, :N_{i+1}]        (a prefix: not materialised
 *                                         separately unless d_sub_idx != NULL)
 *   interp_idx[i] int32 [B,N_i,1]       = knn(xyz[:, :N_{i+1}], xyz[:, :N_i], 1)
 * d_neigh_idx / d_sub_idx / d_interp_idx are host arrays of num_layers device pointers. */
int ssdr_knn_pyramid_dev(const float* d_xyz, size_t batch_size, size_t npts,
                         size_t num_layers, const int32_t* ratios, size_t K,
                         int32_t* const* d_neigh_idx, int32_t* const* d_sub_idx,
                         int32_t* const* d_interp_idx, void* stream);
/* Host flavour (host pointers everywhere, synchronous). */
int ssdr_knn_pyramid(const float* xyz, size_t batch_size, size_t npts,
                     size_t num_layers, const int32_t* ratios, size_t K,
                     int32_t* const* neigh_idx, int32_t* const* sub_idx, int32_t* const* interp_idx);

/* ---- grid subsampling (replaces S3/utils/cpp_wrappers/cpp_subsampling: grid_subsampling.cpp:5-106,
 *      called through wrapper.cpp:58-276) -------------------------------------------------------
 * Voxel-grid barycentres: per occupied voxel the mean position, mean feature vector (fp32, summed in
 * input order) and the majority label per label column (ties and row order as in the reference, see
 * `order`).  features / classes may be NULL (then fdim / ldim are ignored).
 * order: SSDR_ORDER_REFERENCE  rows in the reference's order (iteration order of its
 *                              std::unordered_map<size_t,...>, GCC libstdc++)  — bit-identical output
 *        SSDR_ORDER_KEY        rows by ascending voxel key (cheaper)
 * Two-step host protocol: ssdr_grid_subsample computes and keeps the result on the device and
 * returns M in *out_m; ssdr_grid_subsample_fetch copies it into caller-owned arrays of M rows. */
#define SSDR_ORDER_REFERENCE 0
#define SSDR_ORDER_KEY       1
int ssdr_grid_subsample(const float* points, size_t n,
                        const float* features, size_t fdim,
                        const int32_t* classes, size_t ldim,
                        float sampleDl, int order, size_t* out_m);
int ssdr_grid_subsample_fetch(float* out_points, float* out_features, int32_t* out_classes);
/* Device flavour: outputs must have room for n rows; *d_out_m (device int64) receives M. */
int ssdr_grid_subsample_dev(const float* d_points, size_t n,
                            const float* d_features, size_t fdim,
                            const int32_t* d_classes, size_t ldim,
                            float sampleDl, int order,
                            float* d_out_points, float* d_out_features, int32_t* d_out_classes,
                            int64_t* d_out_m, void* stream);

/* All clouds of a batch in one call (the per-cloud chain is ~45 small launches; batching divides that by the batch).
 * The clouds are concatenated: cloud r owns rows [cloud_offsets[r], cloud_offsets[r+1]) (host int64 [num_clouds+1]) of
 * d_points / d_features / d_classes; its M_r output rows are written from row cloud_offsets[r] of the output arrays and
 * M_r to d_out_m[r].  Rows by ascending voxel key (SSDR_ORDER_KEY).  At most 64 clouds per call. */
int ssdr_grid_subsample_batch_dev(const float* d_points, const float* d_features, size_t fdim, const int32_t* d_classes, size_t ldim,
                                  const int64_t* cloud_offsets, size_t num_clouds, float sampleDl,
                                  float* d_out_points, float* d_out_features, int32_t* d_out_classes, int64_t* d_out_m, void* stream);
/* The device flavours only enqueue work: what their kernels found is read here (waits for `stream`).  bit 0 = a voxel with more labels in one
 * column than the per-voxel table holds (the host flavour returns SSDR_ERR_UNSUPPORTED for the same). */
/* Which implementation ssdr_grid_subsample_batch_dev uses (process-wide).
 *   SSDR_SUBSAMPLE_AUTO (default)  rows of at most 7 words (3 + fdim + ldim <= 7): one partition pass into spatial buckets of 8 x 8 x 8 (or
 *                                  16 x 8 x 8) voxels and one workgroup per bucket that orders and reduces its voxels in LDS; clouds whose grid
 *                                  needs more than 16384 such buckets, or that hold a voxel of more than 1024 points, are reported by
 *                                  ssdr_grid_subsample_status (bits 2 / 4) and must be repeated with SSDR_SUBSAMPLE_SORT.  Other rows: the sort.
 *   SSDR_SUBSAMPLE_SORT            segmented radix sort of (voxel key, index) words: any grid, any voxel population.
 * Both give the reference's rows bit for bit (grid_subsampling.cpp:5-106), by ascending voxel key. */
#define SSDR_SUBSAMPLE_AUTO 0
#define SSDR_SUBSAMPLE_SORT 1
int ssdr_grid_subsample_set_method(int method);
int ssdr_grid_subsample_status(void* stream, int32_t* out_status);

/* ---- Semantic3D sampling loader: the cut of a whole scan into network inputs ---------------------------------------
 * split3 (SSRD_AL_semantic3d/semantic3d_dataset_sampling.py:198-236) + the merge rule of tf_map (:243-255): the cloud is halved along x and y at
 * the middle of its bounding box (float32 comparisons against float64 mid-points, as NumPy evaluates them; the z test of :224 holds for every
 * point and is reproduced), a part of more than max_size points is split again (the parts of THAT split against recurse_max_size: the
 * reference's recursive call passes the literal 800000 whatever its caller's max_size was, :233), and a part of at most merge_max points joins
 * the one before it.  d_xyz [n,3].  Outputs: d_order [n] = the points grouped by combined part (ascending index inside a leaf, leaves in the order split3
 * appends them; the reference's order inside a part is CPython's set iteration order), part_offsets (host, max_parts + 1 entries) and
 * *num_parts; d_part [n] (may be NULL) = the combined part of every point.  Synchronous (the recursion tree is decided on the host).
 * SSDR_ERR_UNSUPPORTED: a part above max_size that does not split (coincident points: the reference recurses without end). */
int ssdr_split3_dev(const float* d_xyz, size_t n, size_t max_size, size_t recurse_max_size, size_t merge_max, int32_t* d_part, int32_t* d_order, int64_t* part_offsets,
                    size_t max_parts, size_t* num_parts, void* stream);

/* ---- tile generator (spatially_regular_gen, S3/s3dis_dataset.py:115-154; data_aug, S3/helper_tool.py:185-199) --
 * From a (sub-sampled) cloud resident on the device — d_points [*,3], d_colors [*,color_dim], live row count
 * *d_m (device int64, as written by ssdr_grid_subsample_dev; n_max bounds it) — take the num_points points nearest
 * to center[3] (host), order them by the caller's shuffle d_perm (a permutation of [0,num_points)), subtract the
 * centre, and emit d_out_xyz [num_points,3], d_out_feat [num_points,3+color_dim] = [xyz_centred, colors*scale]
 * (may be NULL) and d_out_idx [num_points] = source row (may be NULL).  A cloud with fewer than num_points rows
 * is padded by duplicating row floor(d_dup_u[r] * m) of the shuffled list (d_dup_u: uniform [0,1) floats).
 * An empty cloud (*d_m <= 0) has no row to take or to duplicate: the call reads none of its points or colours and
 * leaves d_out_xyz / d_out_feat / d_out_idx as they were. */
int ssdr_tile_select_dev(const float* d_points, const float* d_colors, int color_dim, const int64_t* d_m, size_t n_max,
                         const float* center, size_t num_points, const int32_t* d_perm, const float* d_dup_u, float color_scale,
                         float* d_out_xyz, float* d_out_feat, int32_t* d_out_idx, void* stream);

/* Batch form: cloud r = rows [cloud_offsets[r], cloud_offsets[r+1]) with live count d_m[r]; centers host [num_clouds,3];
 * d_perm / d_dup_u [num_clouds, num_points]; outputs [num_clouds, num_points, ...].  d_out_idx = source row inside its cloud.
 * d_labels (int32, one per row, may be NULL) -> d_out_labels [num_clouds, num_points] = queried_pc_label (s3dis_dataset.py:141).
 * An empty cloud (d_m[r] <= 0: what ssdr_grid_subsample_batch_dev hands on for a cloud it refused, status bit 2) has no row to take or to
 * duplicate: none of its points, colours or labels is read, and its rows of every output stay as they were; the other clouds are not affected. */
int ssdr_tile_select_batch_dev(const float* d_points, const float* d_colors, int color_dim, const int64_t* d_m, const int64_t* cloud_offsets,
                               size_t num_clouds, const float* centers, size_t num_points, const int32_t* d_perm, const float* d_dup_u,
                               float color_scale, float* d_out_xyz, float* d_out_feat, int32_t* d_out_idx, const int32_t* d_labels,
                               int32_t* d_out_labels, void* stream);
/* ssdr_grid_subsample_batch_dev + ssdr_tile_select_batch_dev in one call, for a caller that keeps nothing of the sub-sampled clouds but the tiles: the tiles
 * (d_out_xyz / d_out_feat / d_out_labels) are those of the two calls bit for bit, with d_colors = the sub-sampled features and d_labels = the sub-sampled
 * classes (ldim 1).  The partition path (SSDR_SUBSAMPLE_AUTO) reduces only the spatial buckets that can hold one of the num_points rows nearest to a cloud's
 * centre: the bounds follow from the buckets' boxes, the sufficiency check from exact row counts, all on the stream and from this call's inputs alone.  d_sub_*
 * then receive the rows of those buckets (ascending voxel key), d_sub_m[r] their count, and d_out_idx counts among them.  ssdr_grid_subsample_status reports
 * as for the two calls (a refused cloud: repeat with SSDR_SUBSAMPLE_SORT, which produces every row). */
int ssdr_tile_from_rooms_batch_dev(const float* d_points, const float* d_features, size_t fdim, const int32_t* d_classes, size_t ldim,
                                   const int64_t* cloud_offsets, size_t num_clouds, float sampleDl,
                                   float* d_sub_points, float* d_sub_features, int32_t* d_sub_classes, int64_t* d_sub_m,
                                   const float* centers, size_t num_points, const int32_t* d_perm, const float* d_dup_u, float color_scale,
                                   float* d_out_xyz, float* d_out_feat, int32_t* d_out_idx, int32_t* d_out_labels, void* stream);
/* Per cloud of the last ssdr_tile_from_rooms_batch_dev on `stream` (waits for it; int32 [num_clouds] each, may be NULL): the stage the reduction ended in
 * (1: the first stage's buckets sufficed or were the whole cloud, 2: the set estimated from the first stage's points per voxel sufficed, 3: the rest of the
 * cloud was needed, 0: reduced whole without an order, -1: the sort), the buckets reduced, the cloud's non-empty buckets. */
int ssdr_tile_from_rooms_stats(void* stream, int32_t* out_stage, int32_t* out_reduced, int32_t* out_buckets, size_t num_clouds);
/* Per cloud of the last ssdr_tile_from_rooms_batch_dev on `stream` (waits for it; int64 [num_clouds] each, may be NULL): the 32-byte records its partition wrote
 * and the cloud's points.  The partition writes only the records of the buckets a stage reduces: records < points for a cloud whose first stage sufficed with a
 * part of its buckets, records == points for a cloud that went on to a later stage or was reduced whole.  -1 / -1 when the call took the sort.  A planned call whose plan holds the records (below) writes
 * none: for it the first number is "records the stages were given", not "records written" — the points of the buckets the first stage was handed, plus, for a
 * cloud that went on, the points of all its other buckets — which is the number the unplanned call reports for the same inputs. */
int ssdr_tile_from_rooms_scatter_stats(void* stream, int64_t* out_scattered, int64_t* out_points, size_t num_clouds);
/* Room plans: a caller that uploads a set of rooms once and draws many tiles from it (every tile has its own centres) builds a plan behind the upload and
 * hands it to every call.  The plan keeps what the partition path derives from the points and sampleDl alone — every cloud's grid and bucket geometry, its status
 * bits, the per-chunk and per-bucket point counts with their prefix sums, one work item per non-empty bucket — in device buffers of its own; a planned call reads
 * them and starts at the order of the buckets around the centres (two of the three reads of all coordinates and five launches fewer per call).
 *   ssdr_rooms_plan_create_dev   builds the plan on `stream` (asynchronous; the inputs as for ssdr_tile_from_rooms_batch_dev).  Rows of more than 7 words
 *                                (3 + fdim + ldim) take the sort, which keeps nothing: SSDR_ERR_UNSUPPORTED.
 *   ssdr_tile_from_rooms_planned_batch_dev   ssdr_tile_from_rooms_batch_dev with the plan: the same outputs, ssdr_grid_subsample_status and
 *                                ssdr_tile_from_rooms_*stats bit for bit, refused clouds (status bits 2, 4) and clouds reduced whole included.  It may run on any
 *                                stream: the first call on a stream other than the plan's is ordered behind the build by an event the plan keeps.  SSDR_ERR_INVALID
 *                                when d_points, d_features, d_classes, fdim, ldim, cloud_offsets, num_clouds or sampleDl differ from the plan's.  Under
 *                                SSDR_SUBSAMPLE_SORT the plan is checked and not used.
 *   ssdr_rooms_plan_destroy      waits for the device, then frees the plan (NULL is accepted).
 *   ssdr_rooms_plan_info         read-only: *out_record_bytes = the bytes of the records the plan holds (0: none), *out_sorted = 1 when they are ordered inside a
 *                                bucket (0 in this version); either pointer may be NULL.
 * The plan also OWNS A COPY OF THE CLOUDS' ROWS: every point as a 32-byte record (xyz, its index in the cloud, features, classes) in the spatial bucket the tables
 * assign it to — the inputs rearranged, no sum and no vote.  A planned call with such a plan runs no partition pass and does NOT READ d_points, d_features or
 * d_classes (their pointers are still compared); its voxel reduction reads the plan's records.  Environment, read at every ssdr_rooms_plan_create_dev:
 * SSDR_FE_PLAN_RECORDS=0 builds a plan without records (calls then write their records per call, as without this copy); SSDR_FE_PLAN_RECORDS_MAX_MB (default
 * 4096): a plan whose records would be larger is built without them, silently (ssdr_rooms_plan_info tells).
 * CONTRACT: a plan is valid while the bytes behind d_points, d_features, d_classes and cloud_offsets are unchanged.  The library compares pointers and offsets, not
 * the bytes: a caller that rewrites any of them in place destroys the plan and creates it again (with records a stale plan would go on answering for the OLD rows).
 * A plan is read-only once built: any number of planned calls, on any streams, may share it.
 * Memory: the per-chunk counts are sized for the worst case, 16384 buckets x ceil(largest cloud / 32768) chunks x num_clouds words — about 39 MB for 16 clouds
 * of up to 1.2 M points — plus 0.7 MB per cloud of bucket tables, per plan; the records add 32 bytes per raw point (431 MB for 13.46 M points), up to the cap.  A
 * stream that only makes planned calls with records keeps 32 bytes per raw point less of scratch (its record buffer holds the rows region alone). */
int ssdr_rooms_plan_create_dev(const float* d_points, const float* d_features, size_t fdim, const int32_t* d_classes, size_t ldim,
                               const int64_t* cloud_offsets, size_t num_clouds, float sampleDl, void* stream, void** out_plan);
int ssdr_rooms_plan_destroy(void* plan);
int ssdr_rooms_plan_info(void* plan, int64_t* out_record_bytes, int32_t* out_sorted);
int ssdr_tile_from_rooms_planned_batch_dev(const void* plan, const float* d_points, const float* d_features, size_t fdim, const int32_t* d_classes, size_t ldim,
                                           const int64_t* cloud_offsets, size_t num_clouds, float sampleDl,
                                           float* d_sub_points, float* d_sub_features, int32_t* d_sub_classes, int64_t* d_sub_m,
                                           const float* centers, size_t num_points, const int32_t* d_perm, const float* d_dup_u, float color_scale,
                                           float* d_out_xyz, float* d_out_feat, int32_t* d_out_idx, int32_t* d_out_labels, void* stream);
/* Test-time variant (S3/s3dis_dataset_test.py:105-143): the same tile, plus the possibility-map update
 * possibility[idx] += (1 - dists/max(dists))^2 over the tile's (un-padded) points (float64 map, float32 dists) and,
 * optionally, min / argmin of the updated map (the next pick: :106-108).  An empty cloud (*d_m <= 0): the tile outputs and the
 * map stay as they were; the minimum over no rows comes out as 1e300 with arg-min 0x7fffffff. */
int ssdr_tile_select_possibility_dev(const float* d_points, const float* d_colors, int color_dim, const int64_t* d_m, size_t n_max,
                                     const float* center, size_t num_points, const int32_t* d_perm, const float* d_dup_u, float color_scale,
                                     float* d_out_xyz, float* d_out_feat, int32_t* d_out_idx,
                                     double* d_possibility, double* d_out_min_possibility, int32_t* d_out_argmin, void* stream);

/* ---- prune: the voxel grid of the superpoint partition (replaces libply_c.prune, S3/partition/ply_c/ply_c.cpp:289-383, called from
 *      partition/partition.py:126-144) ---------------------------------------------------------------------------------------
 * bin = floor((p - bbox_min) / voxel_size); per voxel: float32 position sum / count, uint32 colour sum / count truncated to uint8,
 * histogram of labels [n_labels + 1] and of objects [n_objects + 1] (uint32), rows in the order in which the voxels are first met
 * in the input.  d_rgb / d_out_rgb may be NULL; labels / objects are skipped when n_labels / n_objects is 0.  Outputs are sized
 * for n rows; *d_out_m (device int64) receives the number of voxels.  ssdr_prune_status waits for the stream and reports a
 * grid with more than 2^21 bins along an axis or an id above its declared maximum (the reference's .at() would throw). */
int ssdr_prune_dev(const float* d_xyz, size_t n, float voxel_size, const uint8_t* d_rgb, const uint8_t* d_labels, int n_labels,
                   const uint32_t* d_objects, int n_objects, float* d_out_xyz, uint8_t* d_out_rgb, uint32_t* d_out_labels,
                   uint32_t* d_out_objects, int64_t* d_out_m, void* stream);
int ssdr_prune_status(void* stream, int32_t* out_status);

/* ---- RandLA-Net inference (replaces the TF1 graph of S3/RandLANet.py:140-180, 505-585 run by
 *      model.sess.run([prob_logits, last_second_features, ...]) in S3/sampler2.py:598 / :327) ----------
 * Activations, accumulation and every non-matrix operation are fp32.  The matrix products run in one of three arithmetic
 * modes (ssdr_randla_set_precision): SSDR_PREC_F32 (default) exact f32-input MFMA; SSDR_PREC_BF16X3 both operands carried as
 * two bf16 pieces, hi*hi + lo*hi + hi*lo on the bf16 MFMA with fp32 accumulation (within the 1e-3 feature tolerance of
 * the fp32 path); SSDR_PREC_BF16 operands rounded to bf16 once (BASELINE configuration 3; tolerance reported separately).
 * Weights are handed over per layer with batch-norm already folded
 * (W [in,out] row-major, b [out]); the layer table is documented in csrc/randla_model.hip and built from the
 * reference's variable scopes by ssdr_al/randlanet.py.  Inputs are device pointers:
 *   d_features [B,N0,in_dim]   d_xyz [B,N0,3] (level i uses the first N_i points, tf_map's prefix sub-sampling)
 *   d_neigh_idx[i] int32 [B,N_i,16]  (sub_idx[i] is its prefix)   d_interp_idx[i] int32 [B,N_i,1]
 * Outputs: d_probs [B*N0,C] = softmax(logits) (RandLANet.py:84), d_feat32 [B*N0,32] = last_second_features
 * (RandLANet.py:45,175). */
int  ssdr_randla_create(int num_layers, const int32_t* d_out, int k_n, int num_classes, int in_dim, void** handle);
int  ssdr_randla_num_layers(void* handle);
int  ssdr_randla_layer_shape(void* handle, int layer, int* in, int* out, int* has_bias);
int  ssdr_randla_set_layer(void* handle, int layer, const float* W, const float* b);   /* host pointers */
#define SSDR_PREC_F32 0
#define SSDR_PREC_BF16X3 1
#define SSDR_PREC_BF16 2
int  ssdr_randla_set_precision(void* handle, int mode);
/* formulation of the K-expanded building_block halves in the two bf16 modes: 1 (default) = 32 x 32 MFMA tiles with the softmax over the
 * neighbours inside the lane (csrc/randla_lfa32.hip, every level), 0 = the 16 x 16-tile kernels of rounds 1-3 (csrc/randla_bf16.hip; their level 0
 * runs on the exact-f32 kernel).  Same results within the tolerance above; kept selectable for A/B timing and as a second check of either. */
int  ssdr_randla_set_formulation(void* handle, int tiles32);
void ssdr_randla_destroy(void* handle);
int  ssdr_randla_infer_dev(void* handle, size_t batch_size, size_t npts, const float* d_features, const float* d_xyz,
                           const int32_t* ratios, int32_t* const* d_neigh_idx, int32_t* const* d_interp_idx,
                           float* d_probs, float* d_feat32, void* stream);
/* B = 1 with explicit level sizes: level l is the first level_rows[l] rows (level_rows host [num_layers + 1], positive, non-increasing, or
 * SSDR_ERR_INVALID; more than SSDR_PREDICT_MAX_ROWS level-0 rows: SSDR_ERR_UNSUPPORTED).  neigh_idx[l] [level_rows[l], K] indexes level l,
 * interp_idx[l] [level_rows[l], 1] level l + 1; rows need not come from one cloud (the packed whole-cloud batch of the prediction pass,
 * ssdr_predict_*).  ssdr_randla_infer_dev is this call with level_rows[l + 1] = level_rows[l] / ratios[l] and B tiles. */
int  ssdr_randla_infer_rows_dev(void* handle, const size_t* level_rows, const float* d_features, const float* d_xyz,
                                int32_t* const* d_neigh_idx, int32_t* const* d_interp_idx, float* d_probs, float* d_feat32, void* stream);

/* ---- whole-cloud prediction pass (TSampler.prediction / compute_features, S3/sampler2.py:580-642, :313-342; csrc/predict.hip) -------
 * Every cloud goes through the network WHOLE (spatially_regular_gen in mode "sampling", s3dis_dataset.py:129-150): cloud c (n_c points,
 * rows [cloud_offsets[c], cloud_offsets[c+1]) of the concatenated clouds; cloud_offsets host int64 [num_clouds + 1]) has
 * T_c = max(n_c, num_points) tile rows; its level l is its first N_c^(l) rows (N^(0) = T_c, N^(l+1) = N^(l) / ratios[l]).
 * Packed layout: segment s = L .. 0 (deepest first) holds rows [N_c^(s+1), N_c^(s)) of every cloud in turn, so the level-l rows of all
 * clouds are the first P_l = sum_c N_c^(l) packed rows (the network's prefix levels, ssdr_randla_infer_rows_dev).
 * Cloud-major layout: cloud c's T_c rows start at row sum_{c' < c} T_c'.  KNN block layout: level l's block starts at row
 * R_l = sum_{l' < l} P_l', cloud c's N_c^(l) rows follow the clouds before it.
 * Refused by every entry below: an empty cloud or one too small for the pyramid (SSDR_ERR_INVALID), more than SSDR_PREDICT_MAX_ROWS
 * level-0 rows or more than 4096 clouds in one call (SSDR_ERR_UNSUPPORTED). */
#define SSDR_PREDICT_MAX_ROWS (1 << 23)
/* P_0 .. P_L of a chunk (level_rows host int64 [num_layers + 1], may be NULL: validation only). */
int ssdr_predict_layout(const int64_t* cloud_offsets, size_t num_clouds, size_t num_points, size_t num_layers, const int32_t* ratios,
                        int64_t* level_rows);
/* The whole-cloud tile: tile.hip's rule (ascending float32 squared distance to centers[c], ties by index; row r takes sorted position
 * d_perm[r] or, for a padded cloud, DP.data_aug's duplicate floor(d_dup_u[r] * n_c) of the shuffled list; coordinates minus the centre)
 * with num_points = T_c.  d_perm / d_dup_u: [sum T_c], cloud c's T_c draws at its cloud-major offset.  Outputs: cloud-major d_cm_xyz
 * [sum T_c, 3] and d_cm_idx [sum T_c] (source point inside its cloud = the reference's point_idx); packed d_pk_xyz [P_0, 3], d_pk_feat
 * [P_0, 6] = [xyz, rgb * color_scale], d_pk_src [P_0] (may be NULL), d_pk_labels [P_0] (may be NULL; needs d_labels [sum n_c]). */
int ssdr_predict_tile_dev(const float* d_points, const float* d_colors, const int32_t* d_labels, const int64_t* cloud_offsets, size_t num_clouds,
                          const float* centers, size_t num_points, size_t num_layers, const int32_t* ratios, const int32_t* d_perm, const float* d_dup_u,
                          float color_scale, float* d_cm_xyz, int32_t* d_cm_idx, float* d_pk_xyz, float* d_pk_feat, int32_t* d_pk_src,
                          int32_t* d_pk_labels, void* stream);
/* KNN pyramid of every cloud over its cloud-major rows (ssdr_knn_pyramid_dev per cloud, bit for bit; K = 16 only): d_cm_neigh
 * [R_L, 16] and d_cm_interp [R_L] in the KNN block layout, values cloud-local rows.  Status through ssdr_knn_status on the stream. */
int ssdr_knn_pyramid_ragged_dev(const float* d_cm_xyz, const int64_t* cloud_offsets, size_t num_clouds, size_t num_points, size_t num_layers,
                                const int32_t* ratios, size_t K, int32_t* d_cm_neigh, int32_t* d_cm_interp, void* stream);
/* Cloud-local KNN tables -> packed: row j of cloud c in level l's block moves to R_l + pos(c, j), every value v to pos(c, v).  Level l of
 * d_pk_neigh [R_L, 16] / d_pk_interp [R_L] starts at row R_l and is the network's neigh_idx[l] / interp_idx[l]. */
int ssdr_predict_translate_dev(const int64_t* cloud_offsets, size_t num_clouds, size_t num_points, size_t num_layers, const int32_t* ratios, size_t K,
                               const int32_t* d_cm_neigh, const int32_t* d_cm_interp, int32_t* d_pk_neigh, int32_t* d_pk_interp, void* stream);
/* Packed network outputs -> each cloud's own point order: d_probs [sum n_c, num_classes], d_feat32 [sum n_c, 32].
 * mode SSDR_READBACK_REFERENCE: out[p] = tile_out[argsort(point_idx)[p]] (sampler2.py:599, :327) with a STABLE argsort — on a padded cloud
 *   point_idx holds duplicates and row p is the p-th smallest key's row, not always point p's (NumPy's default argsort is not stable:
 *   it may pick another row of the same point, which differs only in rounding);
 * mode SSDR_READBACK_POINT: point p gets the output of its own first tile row.  Identical for an unpadded cloud.
 * d_cm_idx is ssdr_predict_tile_dev's: rows [0, n_c) of every cloud hold each of its points once, a padded cloud's duplicates follow. */
#define SSDR_READBACK_REFERENCE 0
#define SSDR_READBACK_POINT 1
int ssdr_predict_readback_dev(const int64_t* cloud_offsets, size_t num_clouds, size_t num_points, size_t num_layers, const int32_t* ratios,
                              const int32_t* d_cm_idx, const float* d_pk_probs, size_t num_classes, const float* d_pk_feat32, int mode,
                              float* d_probs, float* d_feat32, void* stream);
/* The Semantic3D flavour (Semantic3D_Dataset_Sampling in mode "sampling", SSRD_AL_semantic3d/semantic3d_dataset_sampling.py:114-294;
 * total[point_idx[0]] = out, sampler2.py:344, :629): a scan is never padded, ssdr_split3_dev cuts its tile into parts, and every combined part
 * is one cloud of the layout above with num_points = 1 (T = the part's rows): ssdr_predict_layout, ssdr_knn_pyramid_ragged_dev,
 * ssdr_predict_translate_dev and ssdr_randla_infer_rows_dev take the part offsets as cloud_offsets and num_points = 1.
 * ssdr_predict_scan_tile_dev: the tile of ONE scan of n points (at most 0x3fffffff), tile.hip's rule with num_points = n: all rows by ascending
 *   float32 squared distance to center[3] (host), ties by index, row r = sorted position d_perm[r] (a permutation of [0, n)), minus the centre
 *   on all three axes.  d_t_xyz [n,3], d_t_idx [n] (the reference's queried_idx), d_t_feat [n,6] = [xyz, rgb * color_scale] (8-byte aligned;
 *   ssdr_feed_augment_dev with one tile of n rows then rewrites columns 0..2).
 * ssdr_predict_parts_dev: the parts of one chunk as ragged clouds.  d_t_xyz / d_t_feat / d_t_idx: the tiles of all scans, concatenated in scan
 *   order (scan c's rows start at its first point, T_c = n_c); d_order: ssdr_split3_dev's output of every scan at the same offsets (values are
 *   scan-local tile rows); part_offsets host int64 [num_parts + 1]: the chunk's parts as ranges of d_order (absolute, the first need not be 0);
 *   part_base host int64 [num_parts]: the first point of each part's scan; d_labels i32 [sum n_c] in point order (may be NULL).  With
 *   row = part_base[k] + d_order[part_offsets[k] + j]: d_cm_xyz [rows,3] part-major (ssdr_knn_pyramid_ragged_dev's input), and at packed position
 *   pos(k, j): d_pk_xyz = d_t_xyz[row], d_pk_feat = d_t_feat[row], d_pk_src = part_base[k] + d_t_idx[row] (the point, over all scans; the sum
 *   of all n_c must stay below 2^30), d_pk_labels = d_labels[d_pk_src] (may be NULL).  Refusals: as ssdr_predict_layout, with "cloud" = part.
 * ssdr_predict_scatter_dev: d_probs[d_pk_src[r]] = d_pk_probs[r] and d_feat32 likewise for r < num_rows (d_probs [num_out, num_classes],
 *   d_feat32 [num_out, 32], both feature arrays 16-byte aligned).  Every point lies in exactly one part: one writer per output row, no atomic,
 *   no order dependence.  A source outside [0, num_out) writes nothing.  All three only enqueue. */
int ssdr_predict_scan_tile_dev(const float* d_points, const float* d_colors, size_t n, const float* center, const int32_t* d_perm, float color_scale,
                               float* d_t_xyz, float* d_t_feat, int32_t* d_t_idx, void* stream);
int ssdr_predict_parts_dev(const float* d_t_xyz, const float* d_t_feat, const int32_t* d_t_idx, const int32_t* d_labels, const int32_t* d_order,
                           const int64_t* part_offsets, const int64_t* part_base, size_t num_parts, size_t num_layers, const int32_t* ratios,
                           float* d_cm_xyz, float* d_pk_xyz, float* d_pk_feat, int32_t* d_pk_src, int32_t* d_pk_labels, void* stream);
int ssdr_predict_scatter_dev(const int32_t* d_pk_src, size_t num_rows, const float* d_pk_probs, size_t num_classes, const float* d_pk_feat32,
                             size_t num_out, float* d_probs, float* d_feat32, void* stream);

/* ---- selection stage (replaces the NumPy / sklearn host code of S3/sampler2.py:12-47,102-115,262-266,313-342,
 *      612-640, S3/fps_gcn_cpu.py:12-178 and S3/kcenterGreedy.py:60-128) ---------------------------------------
 * Superpoints are CSR: sp_off int32 [S+1] into sp_pts int32 [T] (point ids) == the reference's `components`.
 * All pointers are device pointers; float64 where the reference computes in float64. */
#define SSDR_UNC_LC 0       /* 1 - max p                          (sampler2.py:29-34) */
#define SSDR_UNC_ENTROPY 1  /* -sum p log2 p                      (:35-40, :247-255)  */
#define SSDR_UNC_SB 2       /* second best / best                 (:41-44)            */
#define SSDR_REGION_MEAN 0        /* sampler2.py:13-14 */
#define SSDR_REGION_SUM_WEIGHT 1  /* :15-18 */
#define SSDR_REGION_WETSU 2       /* :19-26 */
/* compute_point_uncertainty + argmax class (sampler2.py:28-47, :602) */
int ssdr_point_uncertainty_dev(const float* d_probs, size_t n, int num_classes, int mode, float* d_unc, int32_t* d_cls, void* stream);
/* per-superpoint region uncertainty (float64), dominant predicted class and its member count (sampler2.py:612-626) */
int ssdr_region_stats_dev(const float* d_unc, const int32_t* d_cls, const int32_t* d_sp_off, const int32_t* d_sp_pts, size_t S,
                          int num_classes, int mode, double* d_region_unc, int32_t* d_dom, int32_t* d_dom_cnt, void* stream);
/* ssdr_max_dominant: per-superpoint dominant ground-truth label + purity (sampler2.py:102-106, :127-144) */
int ssdr_dominant_label_dev(const int32_t* d_labels, const int32_t* d_sp_off, const int32_t* d_sp_pts, size_t S, int num_labels,
                            int32_t* d_label, double* d_purity, void* stream);
/* add_clsbal (sampler2.py:262-266), in place on d_region_unc; n_selected == 0 is add_classbal (:256-260).  d_skip [S] (may be NULL) != 0: the
 * region is not part of the population — prediction() collects region_class over the UNLABELLED regions of at least min_size points only
 * (sampler2.py:612-627), so labelled / too small regions enter neither the histogram nor its length (their own values are scaled and never used) */
int ssdr_clsbal_dev(const int32_t* d_region_class, size_t S, const uint8_t* d_skip, const int32_t* d_selected_class_list, size_t n_selected,
                    double* d_region_unc, void* stream);
/* the same in two steps for sharded runs: local class histogram (int32[64]), then — after the caller has summed the
 * histograms of all ranks — the scaling with the global histogram / global count */
int ssdr_class_hist_dev(const int32_t* d_region_class, size_t S, const uint8_t* d_skip, const int32_t* d_selected_class_list, size_t n_selected,
                        int32_t* d_hist64, void* stream);
int ssdr_clsbal_hist_dev(const int32_t* d_region_class, size_t S, const int32_t* d_hist64, size_t total, double* d_region_unc, void* stream);
/* sorted_inds = argsort(-u) (sampler2.py:640); equal values keep ascending index */
int ssdr_rank_regions_dev(const double* d_region_unc, size_t S, int32_t* d_sorted_inds, void* stream);
/* compute_features (sampler2.py:333,339): float32 mean of feat rows over the dominant-class members of the
 * superpoints d_sel[0..nsel) (d_sel == NULL: superpoints 0..nsel-1) */
int ssdr_segment_mean_features_dev(const float* d_feat, int feat_dim, const int32_t* d_cls, const int32_t* d_dom,
                                   const int32_t* d_sp_off, const int32_t* d_sp_pts, const int32_t* d_sel, size_t nsel,
                                   float* d_out, void* stream);
/* Device-side pieces of the sharded selection's exchanges (ssdr_al/distributed.py runs the RCCL collectives
 * directly on these buffers, on the caller's stream):
 * ssdr_mask_regions_dev: out[i] = labelled[i] ? -inf : region_unc[i] for i < S, -inf for S <= i < S_padded (what every rank
 * contributes to the all-gather before the global ranking; labelled regions and padding sort last);
 * ssdr_gather_rows_dev: out[r] = in[idx[r]] for rows of row_bytes bytes (compacts the padded all-gather of candidate features). */
int ssdr_mask_regions_dev(const double* d_region_unc, const uint8_t* d_labelled, size_t S, size_t S_padded, double* d_out, void* stream);
int ssdr_gather_rows_dev(const void* d_in, const int32_t* d_idx, size_t n, size_t row_bytes, void* d_out, void* stream);
/* y0[i] = (y1[i] =) (double)x[i]: what np.concatenate / np.matmul do to the float32 features when they meet the float64
 * adjacency (sampler2.py:760-770, fps_gcn_cpu.py:162-166); y1 may be NULL. */
int ssdr_widen_f32_f64_dev(const float* d_x, size_t n, double* d_y0, double* d_y1, void* stream);
/* One cloud's block of fps_adj_all (fps_gcn_cpu.py:40-117) for its superpoints d_sel[0..nsel): bbox centres
 * [nsel,3], directed chamfer means [nsel,nsel] (cd = dir + dir^T, create_cd :12-38) and the normalised adjacency
 * (S-I)D^-1 + I [nsel,nsel]; gcn_top > 0 keeps the top entries per row (:153-160).  max_sp_size >= largest
 * superpoint in d_sel. */
int ssdr_cloud_graph_dev(const float* d_xyz, const int32_t* d_sp_off, const int32_t* d_sp_pts, const int32_t* d_sel, size_t nsel,
                         size_t max_sp_size, int gcn_top, double* d_centres, double* d_cd_dir, double* d_adj, void* stream);
/* All clouds of a batch in one call: d_sel [n_total] lists the superpoints cloud by cloud, d_coff int32 [num_clouds+1]
 * gives each cloud's row range in d_sel / d_centres, d_boff int64 [num_clouds+1] the start of its n_c x n_c block in
 * d_cd_dir / d_adj (both of sum n_c^2 elements); n_max = largest n_c.  Same results as the per-cloud call. */
int ssdr_cloud_graph_batch_dev(const float* d_xyz, const int32_t* d_sp_off, const int32_t* d_sp_pts, const int32_t* d_sel,
                               const int32_t* d_coff, const int64_t* d_boff, size_t num_clouds, size_t n_total, size_t n_max,
                               int gcn_top, double* d_centres, double* d_cd_dir, double* d_adj, void* stream);
/* Arithmetic of the chamfer term in every selection-graph entry point: 0 = float64 (S3DIS: fps_gcn_cpu.py:12-38, the default), 1 = the Semantic3D code's
 * float32 CUDA-kernel values (SSRD_AL_semantic3d/fps_gcn_cuda.py:13-30: centred coordinates rounded to float32, chamfer3D.cu's squared distances,
 * sqrt and the two means in float32, widened).  Process-wide, read at every call. */
int ssdr_select_set_chamfer_mode(int mode);
int ssdr_propagate_batch_dev(const double* d_adj, const int32_t* d_coff, const int64_t* d_boff, size_t num_clouds, size_t n_max,
                             const int32_t* d_rows, const double* d_vin, int feat_dim, double* d_vout, double* d_comb, void* stream);
/* One hop of sum_i A^i V on a block (fps_gcn_cpu.py:162-167): vout[rows] = adj * vin[rows]; comb[rows] += vout[rows] */
int ssdr_propagate_dev(const double* d_adj, size_t n, const int32_t* d_rows, const double* d_vin, int feat_dim, double* d_vout,
                       double* d_comb, void* stream);
/* gcn.create_adj (S3/gcn.py:116-191): the adjacency of the trained-GCN branch (what GCN_sampling feeds its graph convolutions, gcn.py:193-263),
 * torch float32 in the reference: rows of d_feat [N,F] L2-normalised (eps 1e-12) -> d_out_v, cosine matrix times exp(-(ED + CD)) inside a
 * cloud's block and 0 between clouds, minus I, columns scaled by the inverse column sums, plus I -> d_out_adj [N,N].  The clouds' bbox centres
 * and directed chamfer means are those of ssdr_cloud_graph_batch_dev (same d_coff / d_boff); d_rows [N] gives, cloud by cloud, the row of
 * every member in the result (the reference's ref_idx: unlabelled candidates first, then the labelled regions).  N <= 32767. */
int ssdr_create_adj_dev(const float* d_feat, size_t N, int F, const double* d_centres, const double* d_cd_dir, const int32_t* d_coff, const int64_t* d_boff,
                        size_t num_clouds, size_t n_max, const int32_t* d_rows, float* d_out_v, float* d_out_adj, void* stream);
/* ---- the trained-GCN selector: gcn.GCN_sampling (S3/gcn.py:193-263; sampler2.py's "gcn" branch, :687-734), csrc/select_gcn.hip ----------------
 * The graph is the one of ssdr_cloud_graph_batch_dev: cloud c owns the grouped positions d_coff[c] .. d_coff[c+1]-1 and the n_c x n_c block at d_boff[c];
 * d_rows [rows] names, cloud by cloud, the row of every member in the reference's [unlabelled | labelled] order (ref_idx).  d_counts (device int32,
 * the first words of a one-call chain's d_result): [0] unlabelled rows, [1] labelled rows, [2] rows in all — the LIVE counts every kernel reads;
 * cap_rows / n_max (>= rows / >= the largest block) only shape the launches, rows beyond the live count are never read.
 * d_info (device int32 [8]): [0] status bits below, [1] the first cloud with a single row (0x7fffffff: none), [2] values substituted by the
 * evaluation, [3] the training form that ran.  ssdr_gcn_block_adj_dev resets it; the others add to it.
 *
 * ssdr_gcn_block_adj_dev: gcn.create_adj (gcn.py:177-189) stored as per-cloud blocks and never as the [N,N] matrix: d_feat [rows,32] ->
 * d_out_v (rows L2-normalised, eps 1e-12); block[i][j] = <v_i, v_j> * exp(-((float)ED + (float)CD)) - (i == j), columns scaled by the inverse of their
 * float32 sums, plus I -> d_out_adj; d_out_adjT holds every block transposed (bit for bit); d_rowcloud [cap_rows] the cloud of every grouped position.
 * Inside a block the values are ssdr_create_adj_dev's.  A cloud that contributes ONE row has the column sum 0 (the reference divides by it and trains on
 * NaN): SSDR_GCN_ST_SINGLETON is raised, the block is left as the identity, and training / evaluation do nothing.
 *
 * ssdr_gcn_train_dev: `steps` Adam steps of the reference's GCN (gcn.py:60-86, :207-226; nfeat 32, nhid 128; gc2 and linear never receive a gradient and
 * are not represented):  h = A (V W1) + b1;  feat = dropout_p(relu(h)) (kept values times 1 / (1 - p));  x = A (feat W3) + b3;  s = sigmoid(x);
 * loss = -mean(log s[labelled]) - lamda * mean(log(1 - s[unlabelled]));  torch.optim.Adam(lr, betas (0.9, 0.999), eps 1e-8, weight_decay): the decay is
 * added to the gradient, denom = sqrt(v) / sqrt(1 - beta2^t) + eps, step size lr / (1 - beta1^t).  Parameters are one float32 array of
 * SSDR_GCN_NPARAM values: W1 [32,128] row-major, b1 [128], W3 [128], b3.  d_init -> d_trained (may be the same array); d_loss [2] = the loss of step 0's
 * forward pass (with its dropout) and the loss after the last step (forward pass without dropout).  No labelled row (d_counts[1] == 0; the loss is a
 * mean over an empty set): SSDR_GCN_ST_NO_LABELLED, nothing is trained.  Without unlabelled rows the second term is 0.
 * Dropout: unit k of the row r (its index in the [unlabelled | labelled] order) is KEPT at step t (0-based) iff
 *     z = seed + 0x9E3779B97F4A7C15 * (t + 1) + 0xD6E8FEB86659FD93 * (128 r + k + 1)                      (all mod 2^64)
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31
 *     (float)(z >> 40) * 2^-24 >= p                                                                       (float32 comparison)
 * — a function of (seed, step, row, unit) alone, whatever the launch geometry.
 * form: SSDR_GCN_FORM_GENERAL (row-parallel launches, any block size), SSDR_GCN_FORM_FUSED (a workgroup owns whole clouds; n_max <=
 * SSDR_GCN_FUSED_CAP or SSDR_ERR_INVALID), SSDR_GCN_FORM_AUTO (fused when n_max allows it).  The gradient sums are float64 in a fixed order: the same
 * call twice gives the same bits.  The two forms agree to float32 rounding, not bit for bit.
 *
 * ssdr_gcn_eval_dev: the evaluation pass (gcn.py:230-245) -> d_out [cap_rows,129] float64, row r = cat(relu(h_r), x_r) without dropout, NaN replaced
 * by 1e-10 and +-inf by 1e10 (d_info[2] counts them, SSDR_GCN_ST_SUBSTITUTED).  After a refusal the live rows are zeros. */
#define SSDR_GCN_NHID 128
#define SSDR_GCN_NPARAM 4353
#define SSDR_GCN_FUSED_CAP 1024
#define SSDR_GCN_FORM_AUTO 0
#define SSDR_GCN_FORM_GENERAL 1
#define SSDR_GCN_FORM_FUSED 2
#define SSDR_GCN_ST_SINGLETON 32
#define SSDR_GCN_ST_NO_LABELLED 64
#define SSDR_GCN_ST_SUBSTITUTED 128
#define SSDR_GCN_ST_OVERSIZE 256   /* a block above the fused form's cap met on the device (n_max understated): that cloud took no part */
int ssdr_gcn_block_adj_dev(const float* d_feat, size_t cap_rows, int F, const double* d_centres, const double* d_cd_dir, const int32_t* d_coff, const int64_t* d_boff,
                           size_t num_clouds, size_t n_max, const int32_t* d_rows, const int32_t* d_counts, float* d_out_v, float* d_out_adj, float* d_out_adjT,
                           int32_t* d_rowcloud, int32_t* d_info, void* stream);
int ssdr_gcn_train_dev(const float* d_v, const float* d_adj, const float* d_adjT, const int32_t* d_coff, const int64_t* d_boff, size_t num_clouds, size_t n_max,
                       const int32_t* d_rows, const int32_t* d_rowcloud, const int32_t* d_counts, size_t cap_rows, const float* d_init, float* d_trained, int steps,
                       float p, float lr, float weight_decay, float lamda, uint64_t seed, int form, float* d_loss, int32_t* d_info, void* stream);
int ssdr_gcn_eval_dev(const float* d_v, const float* d_adj, const float* d_adjT, const int32_t* d_coff, const int64_t* d_boff, size_t num_clouds, size_t n_max,
                      const int32_t* d_rows, const int32_t* d_rowcloud, const int32_t* d_counts, size_t cap_rows, const float* d_params, double* d_out, int32_t* d_info,
                      void* stream);
/* sampling()'s "gcn" branch as ONE enqueue-only call: the candidate rule, compute_features, bbox centres and chamfer means of ssdr_gcn_fps_sampling_dev
 * (same arguments, same d_result layout: counts, picks at word 8, the candidate list followed by the labelled regions), then block adjacency -> training
 * from d_init -> evaluation -> kCenterGreedy over candidates + labelled rows seeded with the labelled ones (kcenterGreedy.py:84-128) over the 129-d rows.
 * d_result[5] also carries SSDR_GCN_ST_SINGLETON / SSDR_GCN_ST_NO_LABELLED (the picks mean nothing then); substitutions are no failure and are reported
 * by the accessor's d_info alone.  coreGCN = False (gcn.py:251-255) has no call site in the reference and is not offered. */
int ssdr_gcn_sampling_dev(const float* d_feat, int feat_dim, const int32_t* d_cls, const int32_t* d_dom, const int32_t* d_lab_cls, const int32_t* d_lab_dom,
                          const float* d_xyz, const int32_t* d_sp_off, const int32_t* d_sp_pts, const int32_t* d_order, size_t S, const uint8_t* d_labelled, const int32_t* d_sp_base, size_t num_clouds,
                          const int32_t* d_lab_off, const int32_t* d_lab_sp, size_t n_lab, size_t batch_size, const float* d_init, int steps, float p, float lr, float weight_decay,
                          float lamda, uint64_t seed, int form, size_t cap_rows, size_t cap_nmax, size_t cap_sq, size_t cap_unl, size_t max_select, int32_t* d_result, void* stream);
/* What the last ssdr_gcn_sampling_dev call on `stream` left on the device: the evaluation rows [cap_rows][129] float64 (candidates first, then the
 * labelled regions), the trained parameters, d_loss [2] and d_info [8] as above (each may be NULL).  Valid until the next such call on that stream. */
int ssdr_gcn_sampling_rows(void* stream, const double** d_rows, size_t* cap_rows, const float** d_params, const float** d_loss, const int32_t** d_info);
/* The candidate rule of sampling() + GCN_FPS_sampling as ONE enqueue-only call (S3/sampler2.py:533-552 create_file_top_and_all, :745-753 the
 * "first 2 x selected_num regions of a cloud" rule, :313-342 / :736-781 GCN_FPS_sampling; fps_gcn_cpu.py:60-178): the ranking goes in, the selected
 * candidates come out, and no host decision sits in between — the row counts the rule finds stay on the device and every kernel behind it reads them
 * there.  d_order [S] = the regions by descending uncertainty (ssdr_rank_regions_dev); d_labelled [S] != 0: the region is labelled and never competes;
 * the superpoints of cloud c are d_sp_base[c] .. d_sp_base[c+1]-1; d_lab_off [num_clouds+1] / d_lab_sp: the labelled regions cloud by cloud
 * (ascending superpoint id), n_lab of them in all.  batch_size = sampling_batch.  selector 0: farthest_features_sample from candidate `start`
 * (fps_gcn_cpu.py:119-147); 1: kCenterGreedy over candidates + labelled rows seeded with the labelled ones (kcenterGreedy.py:84-128).  Capacities the caller sizes the run by (upper bounds, computable from the static tables):
 * cap_rows >= candidates + labelled regions, cap_nmax >= the largest cloud's share of them, cap_sq >= the sum over clouds of its share squared,
 * cap_unl >= candidates (cap_rows <= 2^22: the reference's own round, 20 000 candidates + 4 000 labelled rows of 272 clouds, is one call), max_select = min(batch_size, unlabelled regions) = the number of picks.
 * d_result (int32): [0..7] n_unl, n_lab, rows, largest block, picks, status (bit 0: rows > cap_rows, bit 1: blocks > cap_sq: nothing was selected),
 * block elements (int64 in two words); [8 .. 8+max_select) the picks (indices into the candidate list); then [cap_rows] the candidate list
 * (superpoint ids, cloud by cloud, descending uncertainty inside a cloud) followed by the labelled regions.  feat_dim = 32.
 * d_cls / d_dom: predicted class per point / dominant predicted class per region — the candidates' dominant_point_ids (sampler2.py:625-626);
 * d_lab_cls / d_lab_dom (both or neither; NULL = the predicted pair): GROUND-TRUTH class per point / dominant ground-truth class per region
 * (ssdr_dominant_label_dev) — the labelled regions' dominant_point_ids (get_labeled_selection_cloudname_spidx_pointidx, sampler2.py:288-291). */
int ssdr_gcn_fps_sampling_dev(const float* d_feat, int feat_dim, const int32_t* d_cls, const int32_t* d_dom, const int32_t* d_lab_cls, const int32_t* d_lab_dom,
                              const float* d_xyz, const int32_t* d_sp_off, const int32_t* d_sp_pts, const int32_t* d_order, size_t S, const uint8_t* d_labelled, const int32_t* d_sp_base, size_t num_clouds,
                              const int32_t* d_lab_off, const int32_t* d_lab_sp, size_t n_lab, size_t batch_size, int gcn_number, int gcn_top, int selector, int start,
                              size_t cap_rows, size_t cap_nmax, size_t cap_sq, size_t cap_unl, size_t max_select, int32_t* d_result, void* stream);
/* The propagated rows of the last ssdr_gcn_fps_sampling_dev call on `stream`: device pointer to [cap_rows][32] float64, the candidates first, then the
 * labelled regions (sum_i A^i V, fps_gcn_cpu.py:162-167 — what GCN_FPS_sampling hands to farthest_features_sample, :169-170).  Valid until the
 * next selection call on that stream. */
int ssdr_gcn_fps_sampling_rows(void* stream, const double** d_rows, size_t* cap_rows);
/* The same for the SHARDED run (one process per GPU), again without a host decision: two enqueue-only calls around the all-gather of the
 * candidates' propagated features.  Global region id = rank * Smax + local id (padding counts as labelled), global cloud = rank * Bmax + local cloud.
 * ssdr_gcn_fps_sharded_local_dev: the candidate rule over the global ranking d_gorder [Sg = world * Smax] (ssdr_rank_regions_dev over the all-gathered masked
 * uncertainties) for the clouds of ALL ranks — d_gbase [world * Bmax + 1]: global cloud c spans d_gbase[c] .. d_gbase[c+1]-1 — then this rank's share of
 * GCN_FPS_sampling for its own clouds.  d_comb_out [nu_max (+ nl_max), 32] float64: its candidates' propagated features in candidate order (what the all-gather
 * sends; nu_max >= the candidates of any rank; nl_max = 0 for the FPS selector).  d_plan (int32, 16 + world + 2 * world * nu_max words): [0..7] as d_result above for this rank, [4] the picks
 * of all ranks, [8] the candidates of all ranks, [9] != 0: a rank offers more than nu_max; [16 .. 16 + world) candidates per rank; then the rows of the gathered
 * array in global candidate order; then the global candidate list (global region ids, rank by rank, cloud by cloud, descending uncertainty inside a cloud).
 * ssdr_fps_gathered_dev: d_gathered [world, nu_max, 32] -> the candidates' rows in order (d_glob [cap_rows, 32], cap_rows >= repeat x the candidates of all
 * ranks, which never exceed 2 x the picks) -> farthest_features_sample from candidate `start` (the replicated global FPS, fps_gcn_cpu.py:169-170); max_select
 * picks (indices into the global candidate list).  repeat > 1 (measurement only): the rows are taken `repeat` times — the chain's load at `repeat` x the ranks. */
int ssdr_gcn_fps_sharded_local_dev(const float* d_feat, int feat_dim, const int32_t* d_cls, const int32_t* d_dom, const int32_t* d_lab_cls, const int32_t* d_lab_dom,
                                   const float* d_xyz, const int32_t* d_sp_off, const int32_t* d_sp_pts, const int32_t* d_lab_off, const int32_t* d_lab_sp, size_t n_lab, size_t num_clouds,
                                   const int32_t* d_gorder, size_t Sg, const uint8_t* d_glabelled, const int32_t* d_gbase, int rank, int world, size_t Smax, size_t Bmax,
                                   size_t batch_size, int gcn_number, int gcn_top, size_t cap_rows, size_t cap_nmax, size_t cap_sq, size_t nu_max, size_t nl_max,
                                   double* d_comb_out, int32_t* d_plan, void* stream);
int ssdr_fps_gathered_dev(const double* d_gathered, const int32_t* d_plan, int world, size_t nu_max, size_t cap_rows, int repeat, int start, size_t max_select, double* d_glob,
                          int32_t* d_out, void* stream);
/* The k-center selector of the sharded run (BASELINE configuration 4: "a single all-gather of per-superpoint features before the global k-center step"; sampler2.py's
 * "kcenter" branch, kcenterGreedy.py:84-128): ssdr_gcn_fps_sharded_local_dev with nl_max > 0 (>= the labelled regions of any rank) also writes this rank's labelled
 * regions' propagated rows behind its candidates (d_comb_out [nu_max + nl_max, 32]); after the all-gather of those rows, ssdr_kcenter_gathered_dev builds
 * [every rank's candidates | every rank's labelled regions] in d_glob [cap_rows, 32] (cap_rows > n_lab_total + the candidates of all ranks), marks the labelled rows as
 * already selected (d_already [n_lab_total], scratch) and runs kCenterGreedy for max_select picks (indices into the global candidate list) — nothing is read back.
 * d_nlab_off [world + 1]: prefix of the ranks' labelled counts (static). */
int ssdr_kcenter_gathered_dev(const double* d_gathered, const int32_t* d_plan, int world, size_t nu_max, size_t nl_max, const int32_t* d_nlab_off, size_t n_lab_total,
                              size_t cap_rows, size_t max_select, double* d_glob, int32_t* d_already, int32_t* d_out, void* stream);
/* What the enqueue-only selection calls issued on `stream` found and could not return (bit 0: a cooperative multi-workgroup FPS / k-center
 * launch — ssdr_fps_dev / ssdr_kcenter_dev above 1536 / 4096 rows — was not co-resident: a workgroup waited for one that never arrived, the chain
 * stopped and its remaining picks read -1).  Waits for the stream; SSDR_ERR_INTERNAL when a bit is set; clears the word. */
int ssdr_select_status(void* stream, int32_t* out_status);
/* farthest_features_sample (fps_gcn_cpu.py:119-147); `start` is the reference's np.random.randint draw */
int ssdr_fps_dev(const double* d_feat, size_t n, int feat_dim, int start, size_t count, int32_t* d_out, void* stream);
/* farthest_superpoint_sample (sampler2.py:49-80, "edcd" branch) over one cloud's superpoints, from the centres and
 * directed chamfer means ssdr_cloud_graph_dev produced: distance = |centre_i - centre_c|^2 + CD(i,c); n <= 8192 */
int ssdr_fps_superpoint_dev(const double* d_centres, const double* d_cd_dir, size_t n, int start, size_t count, int32_t* d_out, void* stream);
/* farthest_superpoint_sample of MANY clouds in one launch (one workgroup per cloud; the "edcd" branch, sampler2.py:49-80, :670-685): cloud b's rows are
 * d_coff[b] .. d_coff[b+1]-1 of d_centres [rows, 3] (ssdr_cloud_graph_batch_dev), its directed chamfer means the n_b x n_b block at d_boff[b] of d_cd_dir,
 * which the call OVERWRITES with dir + dir^T (diagonal 0).  Cloud b picks d_ntop[b] <= n_b rows from its first one, with ssdr_fps_superpoint_dev's arithmetic;
 * the picks (row indices) are written cloud by cloud at the exclusive prefix of d_ntop, FPS order inside a cloud, max_select >= their sum.  n_max >= every
 * n_b with picks, n_max <= 8192.  d_status (optional, device int32): set to 0 or to what the device found (4: a cloud above n_max rows, 8: more picks than
 * rows, 16: more than max_select picks in all); nothing is picked then. */
int ssdr_edcd_fps_batch_dev(const double* d_centres, double* d_cd_dir, const int32_t* d_coff, const int64_t* d_boff, const int32_t* d_ntop, size_t num_clouds,
                            size_t n_max, size_t max_select, int32_t* d_out, int32_t* d_status, void* stream);
/* sampling()'s "edcd" branch behind the candidate rule, ONE enqueue-only call: the arguments and the candidate rule of ssdr_gcn_fps_sampling_dev without
 * features, labelled rows or GCN (the branch draws no labelled rows), the candidates' bbox centres and directed chamfer means — float64 whatever
 * ssdr_select_set_chamfer_mode says (the Semantic3D edcd branch uses gcn.chamfer_distance, a float64 KDTree) — and ssdr_edcd_fps_batch_dev over every
 * cloud.  cap_rows >= the candidates, cap_nmax >= the largest cloud's, cap_sq >= the sum of their squares, max_select = min(batch_size, unlabelled regions).
 * d_result [8 + max_select + cap_rows] as ssdr_gcn_fps_sampling_dev's: [0..7] counts (n_unl, 0, rows, largest block, picks, status, block elements),
 * the picks (indices into the candidate list, cloud ascending, FPS order inside a cloud), the candidate list.  Status bits 0-1 as there; 4: a cloud has
 * more than 8192 candidates (or more than cap_nmax); 8, 16 as above: nothing was selected. */
int ssdr_edcd_sampling_dev(const float* d_xyz, const int32_t* d_sp_off, const int32_t* d_sp_pts, const int32_t* d_order, size_t S, const uint8_t* d_labelled,
                           const int32_t* d_sp_base, size_t num_clouds, size_t batch_size, size_t cap_rows, size_t cap_nmax, size_t cap_sq, size_t max_select,
                           int32_t* d_result, void* stream);
/* The same for the sharded run: the candidate rule over the GLOBAL ranking as ssdr_gcn_fps_sharded_local_dev takes it (d_gorder [Sg = world * Smax],
 * d_glabelled, d_gbase [world * Bmax + 1]), then this rank's clouds' graphs and picks.  edcd is per cloud: no exchange follows.  d_result as above for
 * this rank alone: its candidates (local region ids), its picks (indices into them; counts[4] = its share of sampling_batch). */
int ssdr_edcd_sampling_sharded_dev(const float* d_xyz, const int32_t* d_sp_off, const int32_t* d_sp_pts, size_t num_clouds, const int32_t* d_gorder, size_t Sg,
                                   const uint8_t* d_glabelled, const int32_t* d_gbase, int rank, int world, size_t Smax, size_t Bmax, size_t batch_size,
                                   size_t cap_rows, size_t cap_nmax, size_t cap_sq, size_t max_select, int32_t* d_result, void* stream);
/* sampling()'s last branch, uncertainty alone (sampler2.py:783-806): the first min(batch_size, population) entries of the ranking d_order [n] whose
 * d_skip[id] == 0, in rank order; of them, the ids in [lo, hi) are written to d_out as id - lo (a sharded rank keeps its own: lo = rank * Smax).
 * d_res[0] = entries written, d_res[1] = the size of the whole top.  d_out holds min(batch_size, hi - lo). */
int ssdr_topk_regions_dev(const int32_t* d_order, size_t n, const uint8_t* d_skip, size_t batch_size, size_t lo, size_t hi, int32_t* d_res, int32_t* d_out, void* stream);
/* ---- oracle_labeling (sampler2.py:124-192) over the picks of one round, in the order sampling() calls _help() (:676-684, :796-806) ---------------
 * Enqueue-only.  d_items [max_items]: the picked regions as global superpoint ids in pick order, *d_n_items (device) of them are live; items are grouped by
 * cloud (d_sp_cloud [S], values below num_clouds), the clouds ordered by d_cloud_key [num_clouds] (NULL: first appearance among the items), a cloud's
 * picks in pick order.  The walk over that list is the reference's: stop at click <= 0, skip regions of fewer than min_size points at no cost, otherwise
 * pay one click and label the region with its dominant ground-truth label d_gt (lowest label among equals) — SSDR_LABEL_DOMINANT always, SSDR_LABEL_NAIL
 * when count / len >= threshold (float64); else the points split by predicted class d_pred_class, every sub-region of MORE than min_size points whose own
 * rate reaches the threshold pays one more click and is labelled (the budget may end below zero).  num_labels <= 64, num_classes <= 32; labels / classes /
 * ids outside their range are not counted and raise a status bit.  max_region: an upper bound of a region's size when the caller knows one (0: unknown) —
 * regions of up to 256 points are judged by a wave each, larger ones by a workgroup, and the workgroup kernels are not launched when none can occur.
 * In place: d_mask / d_label [n] float32 (the two rows of pseudo_gt), d_labeled [S] uint8, *d_budget (int64, the clicks left).  Written: d_used
 * [max_items] uint8 per item (pick order), d_class_out [class_cap] the appended selected_class_list entries in the reference's order, d_proc_order
 * (optional, [max_items]) the item processed at every position of the walk, d_out int64 [12]: sp_num, p_num, sub_num, sub_p_num, split_sp_num,
 * ignore_sp_num, class entries, budget left, status (1: label, 2: class out of range, 4: item / point id out of range, 8: more entries than class_cap:
 * the class list is incomplete), items used, regions judged by the wave form, by the workgroup form. */
#define SSDR_LABEL_DOMINANT 0
#define SSDR_LABEL_NAIL     1
int ssdr_oracle_label_dev(const int32_t* d_gt, const int32_t* d_pred_class, size_t n, const int32_t* d_sp_off, const int32_t* d_sp_pts, size_t S,
                          const int32_t* d_sp_cloud, size_t num_clouds, const int32_t* d_items, const int32_t* d_n_items, size_t max_items,
                          const int32_t* d_cloud_key, size_t max_region, int num_labels, int num_classes, int mode, double threshold, int64_t min_size,
                          int64_t* d_budget, float* d_mask, float* d_label, uint8_t* d_used, uint8_t* d_labeled, int32_t* d_class_out, size_t class_cap,
                          int32_t* d_proc_order, int64_t* d_out, void* stream);
/* The picks of a one-call selection as the item list above, on the device: d_result of ssdr_gcn_fps_sampling_dev / ssdr_edcd_sampling_dev (layout 0:
 * picks at word 8 index the candidate list at word 8 + max_select, counts in words 0 and 4, nothing when the status word 5 is set) or of
 * ssdr_topk_regions_dev (layout 1: d_res with d_out = d_res + 8; max_select = max_items).  d_result NULL: the items are the caller's.  d_cloud_key
 * (optional, [num_clouds]): every cloud's first place in the ranking d_order [S] among the regions with d_skip == 0 — the edcd round's cloud order
 * (file_list_top, sampler2.py:533-552). */
int ssdr_oracle_label_items_dev(const int32_t* d_result, int layout, size_t max_select, const int32_t* d_order, size_t S, const uint8_t* d_skip,
                                const int32_t* d_sp_cloud, size_t num_clouds, int32_t* d_items, size_t max_items, int32_t* d_n_items, int32_t* d_cloud_key,
                                void* stream);
/* ---- the same chain in two halves, for a round whose clouds are sharded over `world` ranks -------------------------------------------------------------
 * The walk is a prefix sum over costs that depend on the item alone, so: every rank judges its own items (verdict half), the fixed-size verdict records
 * are all-gathered, and every rank sorts all records by their 64-bit walk key, runs the same scan over them and applies its own (walk half).  Both
 * entries are enqueue-only with per-stream scratch.  A record (SSDR_LABEL_RECORD_BYTES = 80, a multiple of 16 so that gathered slices stay aligned):
 *    0 uint64 key        the walk key (live keys are unique over all ranks; all ones: a dead slot beyond the rank's live count, cost 0, sorts last)
 *    8 int32  pos        the slot among the rank's items
 *   12 int32  kind       0 skipped (fewer than min_size points / no such region), 1 whole region, 2 split, 3 ignored
 *   16 int32  lab, 20 cost (clicks), 24 nent (class-list entries), 28 subp (points of the labelled sub-regions), 32 len (points of the region)
 *   36 uint32 smask      the predicted classes whose sub-region is labelled
 *   40 uint8  sublab[32] their labels (0 where the mask is clear)
 *   72 int32  status     the bits (1, 2, 4 above) the rank's verdict half raised; 76: zero
 * ssdr_oracle_label_verdict_dev: d_items [max_items] are LOCAL superpoint ids, *d_n_items of them live, d_keys [max_items] their walk keys (cloud key in
 * the high half, position in pick order in the low half); same wave / workgroup forms, 256-point boundary and max_region shortcut as above; writes
 * d_records [max_items].
 * ssdr_oracle_label_walk_dev: d_records [world * max_items] rank-major (what the all-gather of the verdict halves' buffers gives); the other arrays are
 * this rank's.  Writes the WHOLE class list in walk order (identical on every rank), d_out [12] with the meaning above (counters, entries, budget left and
 * the status over all ranks; words 10 and 11 count all ranks' regions per form) and *d_budget; applies only the records of `rank`: d_mask / d_label,
 * d_used [max_items], d_labeled [S]; d_walk_pos [max_items]: every own item's position in the global walk, -1 when the walk does not reach it.
 * With world = 1 and the keys (first appearance or cloud key) << 32 | position every output equals ssdr_oracle_label_dev's (d_walk_pos inverts d_proc_order). */
#define SSDR_LABEL_RECORD_BYTES 80
int ssdr_oracle_label_verdict_dev(const int32_t* d_gt, const int32_t* d_pred_class, size_t n, const int32_t* d_sp_off, const int32_t* d_sp_pts, size_t S,
                                  const int32_t* d_items, const int32_t* d_n_items, size_t max_items, const uint64_t* d_keys, size_t max_region, int num_labels,
                                  int num_classes, int mode, double threshold, int64_t min_size, void* d_records, void* stream);
int ssdr_oracle_label_walk_dev(const void* d_records, int rank, int world, const int32_t* d_pred_class, size_t n, const int32_t* d_sp_off, const int32_t* d_sp_pts, size_t S,
                               const int32_t* d_items, const int32_t* d_n_items, size_t max_items, size_t max_region, int num_classes, int64_t* d_budget, float* d_mask,
                               float* d_label, uint8_t* d_used, uint8_t* d_labeled, int32_t* d_class_out, size_t class_cap, int32_t* d_walk_pos, int64_t* d_out,
                               void* stream);
/* The walk keys of a sharded round, on the device.  Global superpoint id = rank * Smax + local id; d_gcloud [world * Smax] = every global region's global
 * cloud (below num_gclouds; -1: padding).  d_picks given (fps / k-center: the picks [n_picks] index the replicated global candidate list d_cand
 * [*d_n_cand <= cand_cap]): a cloud's key is its first appearance among ALL picks; the picks whose region lives on `rank` become d_items (local ids, pick
 * order) / *d_n_items with the global pick position as the low half.  d_picks NULL (edcd / topk: d_items / *d_n_items are the rank's own picks): the key
 * is d_cloud_key [num_gclouds] of the item's cloud (ssdr_oracle_label_items_dev over the global ranking), the low half the position among the items. */
int ssdr_oracle_label_keys_dev(const int32_t* d_picks, size_t n_picks, const int32_t* d_n_cand, const int32_t* d_cand, size_t cand_cap, const int32_t* d_gcloud, size_t Smax,
                               size_t num_gclouds, int rank, int world, const int32_t* d_cloud_key, int32_t* d_items, int32_t* d_n_items, size_t max_items, uint64_t* d_keys,
                               void* stream);
/* kCenterGreedy.select_batch_ (kcenterGreedy.py:84-128) with direct float64 Euclidean distances */
int ssdr_kcenter_dev(const double* d_feat, size_t n, int feat_dim, const int32_t* d_already_selected, size_t n_already, size_t count,
                     int32_t* d_out, void* stream);

/* ---- chamfer_3D.forward (Semantic3D variant: SSRD_AL_semantic3d/chamfer3D/chamfer3D.cu:12-152, chamfer_cuda.cpp:30-33,
 *      dist_chamfer_3D.py:29-81).  xyz1 [b,n,3], xyz2 [b,m,3] -> squared distances dist1 [b,n], dist2 [b,m] and
 *      nearest indices idx1 [b,n] (into xyz2), idx2 [b,m] (into xyz1); fp32; lowest index on exact ties. */
int ssdr_chamfer3d_forward_dev(const float* d_xyz1, const float* d_xyz2, size_t batch, size_t n, size_t m,
                               float* d_dist1, float* d_dist2, int32_t* d_idx1, int32_t* d_idx2, void* stream);

/* ---- evaluation tail ("next" row N2: S3/RandLANet.py:326-334, 353-411; S3/helper_tool.py:237-262) ------------------
 * ssdr_vote_smooth_dev: test_probs[point_idx] = smooth*test_probs[point_idx] + (1-smooth)*probs with NumPy's rule for
 *   repeated indices (old row on the right-hand side, last occurrence wins).  d_owner_scratch: int32, one entry per
 *   row of test_probs, initialised to -1 by the caller once (the call restores it).
 * ssdr_confusion_dev: preds = argmax(probs[proj_idx[i]]) (proj_idx may be NULL: row i), confusion[label][pred] += 1
 *   accumulated into d_confusion uint64 [C,C] (caller zeroes it), optional d_pred int32 [n] and d_iou float64 [C] =
 *   DP.IoU_from_confusions of the accumulated matrix.  Re-projection to the raw cloud is proj_idx = ssdr_knn(sub_xyz,
 *   raw_xyz, K=1) (utils/data_prepare_s3dis.py:69). */
int ssdr_vote_smooth_dev(float* d_test_probs, const int32_t* d_point_idx, const float* d_probs, size_t n, int num_classes, double smooth,
                         int32_t* d_owner_scratch, void* stream);
int ssdr_confusion_dev(const float* d_probs, int num_classes, const int32_t* d_proj_idx, const int32_t* d_labels, size_t n, int32_t* d_pred,
                       uint64_t* d_confusion, double* d_iou, void* stream);

/* ---- test-time generator chain (S3/s3dis_dataset_test.py:85-151, get_batch; csrc/vote.hip) ---------------------------
 * State, owned by the caller, over ALL evaluation clouds concatenated (cloud c = rows [cloud_offsets[c], cloud_offsets[c+1]), host int64
 * [num_clouds + 1], cloud_offsets[0] = 0): d_points f32 [n,3], d_colors f32 [n,color_dim], d_labels i32 [n] (optional), d_possibility f64 [n],
 * d_cloud_min f64 [num_clouds] (min_possibility) and d_cloud_arg i32 [num_clouds] (the LOCAL row of each cloud's first minimum).
 * ssdr_vote_init_dev: every cloud's minimum and first arg-min of the map as it stands (init_possibility, :85-92).
 * ssdr_vote_tiles_dev: num_tiles tiles of get_batch's generator loop (:104-147), in order, tile t + 1 reading what tile t left: the cloud
 *   = first arg-min of d_cloud_min, the centre = its arg-min point + d_noise[t] (float32), the tile = what ssdr_tile_select_possibility_dev
 *   gives for that cloud, centre, d_perm[t] and d_dup_u[t] (d_noise f32 [num_tiles,3], d_perm i32 [num_tiles,num_points], d_dup_u f32
 *   [num_tiles,num_points]), then the possibility update and the cloud's new minimum / arg-min.  Outputs: d_out_xyz [num_tiles,num_points,3],
 *   d_out_feat [num_tiles,num_points,3+color_dim] (optional), d_out_idx [num_tiles,num_points] = GLOBAL rows (cloud_offsets[c] + queried_idx),
 *   d_out_labels [num_tiles,num_points] (optional; needs d_labels), d_out_cloud i32 [num_tiles], d_out_center f32 [num_tiles,3].
 *   Enqueue only: no device value is read by the host, and a call does not wait for the stream (the offset table is uploaded only when it
 *   differs from the last call's on that stream).  The map comes out bit for bit the same on every run.
 * Refused before anything is launched: no clouds, an empty cloud, num_tiles or num_points 0, d_out_labels without d_labels
 * (SSDR_ERR_INVALID); more than 4096 clouds, more than 0x3fffffff points or tile rows in all (SSDR_ERR_UNSUPPORTED).
 * ssdr_vote_tile_launches: kernel launches ssdr_vote_tiles_dev makes per tile (plus one per call).
 * The Semantic3D flavour (Semantic3D_Dataset_Test.get_batch, semantic3d_dataset_test3.py:143-192) is ssdr_feed_chain_dev with flags =
 * SSDR_FEED_XY_ONLY | SSDR_FEED_GLOBAL_ROWS, no class weights and no channels, followed by ssdr_feed_augment_dev over the batch. */
int ssdr_vote_init_dev(const double* d_possibility, const int64_t* cloud_offsets, size_t num_clouds, double* d_cloud_min, int32_t* d_cloud_arg,
                       void* stream);
int ssdr_vote_tiles_dev(const float* d_points, const float* d_colors, int color_dim, const int32_t* d_labels, double* d_possibility,
                        double* d_cloud_min, int32_t* d_cloud_arg, const int64_t* cloud_offsets, size_t num_clouds,
                        size_t num_tiles, size_t num_points, const float* d_noise, const int32_t* d_perm, const float* d_dup_u, float color_scale,
                        float* d_out_xyz, float* d_out_feat, int32_t* d_out_idx, int32_t* d_out_labels, int32_t* d_out_cloud, float* d_out_center,
                        void* stream);
int ssdr_vote_tile_launches(void);

/* ---- training-time generators (csrc/feed.hip; SSDR_AL_s3dis/s3dis_dataset.py:115-154, SSRD_AL_semantic3d/semantic3d_dataset_train.py:151-276) ----
 * ssdr_feed_chain_dev: the general form of the chain above (ssdr_vote_tiles_dev = flags SSDR_FEED_GLOBAL_ROWS, no weights, no channels; the same
 *   launches per tile).  Semantic3D_Dataset_Train.get_batch is flags = SSDR_FEED_XY_ONLY with d_class_weight and both channels.
 *   flags: SSDR_FEED_XY_ONLY    x and y of the tile's rows are centred, z is left as it is (:182); the distance key and the possibility update
 *                               use all three axes (:196)
 *          SSDR_FEED_GLOBAL_ROWS d_out_idx = cloud_offsets[c] + queried_idx; clear: queried_idx itself, rows local to the tile's cloud c
 *                               (d_out_cloud[t]), the reference's batch_pc_idx
 *   d_class_weight f64 [num_labels] (may be NULL; needs d_labels): possibility[row] += (double)(q * q) * d_class_weight[d_labels[row]], q = 1 - d / dmax
 *     in float32 (:196-198).  A label outside [0, num_labels) counts with weight 0 and raises bit 1 of ssdr_feed_status.
 *   d_activation, d_pseudo f32 [n] (each may be NULL) -> d_out_activation, d_out_pseudo f32 [num_tiles,num_points], row for row what d_out_labels takes
 *     from d_labels (the duplicates of a padded cloud included, DP.data_aug).
 *   Refused before anything is launched: what ssdr_vote_tiles_dev refuses; d_class_weight without d_labels or with num_labels <= 0; a channel
 *   output without its input (SSDR_ERR_INVALID).
 * ssdr_feed_tiles_dev: num_tiles INDEPENDENT tiles (S3DIS_Dataset.spatially_regular_gen, mode "training"): tile t is cut from cloud d_tile_cloud[t]
 *   around its point d_tile_point[t] (a cloud-local row); both are device int32 [num_tiles].  The centre = that point + d_noise[t] (device f32
 *   [num_tiles,3]) is formed on the device in float32.  The tile is the num_points nearest rows (ascending float32 squared distance, ties by
 *   row), through d_perm[t], padded through d_dup_u[t] when the cloud is smaller, centred on all three axes.  Outputs as above; d_out_idx holds
 *   rows local to the tile's cloud; d_out_cloud i32 [num_tiles] (may be NULL) receives a copy of the tiles' cloud ids written in stream order,
 *   d_out_center f32 [num_tiles,3] (may be NULL) the centres.  The same cloud may serve several tiles; all tiles go through one set of launches.
 *   A cloud or point id out of range gives an all-zero tile (cloud id and centre included) and raises bit 2 (cloud) or bit 4 (point) of
 *   ssdr_feed_status.  Refusals as above, and more than 65535 tiles (SSDR_ERR_UNSUPPORTED).
 * ssdr_feed_augment_dev: tf_augment_input (:237-276) for a whole batch in one launch: columns 0..2 of d_feat [num_tiles,num_points,3+color_dim]
 *   = float32(((x . R) * s) + noise) in float64, x = d_xyz f32 [num_tiles,num_points,3], R = [[c,-s,0],[s,c,0],[0,0,1]] with (c, s) = d_rot f64
 *   [num_tiles,2], (x . R)_j = (x * R0j + y * R1j) + z * R2j, s = d_scale f64 [num_tiles,3] (scale times symmetry sign), noise = d_noise f64
 *   [num_tiles,num_points,3] (may be NULL: none).  The colour columns are not touched.
 * ssdr_feed_prefix_dev: d_out f32 [num_tiles,num_sub,3] = d_xyz[:, :num_sub] (the sub-sampled xyz levels of tf_map are per-element prefixes).
 * ssdr_feed_status: waits for `stream`, returns the status bits the feed / chain calls on it have raised since the last call (and clears them);
 *   SSDR_ERR_INVALID when any is set.  All other entries only enqueue. */
#define SSDR_FEED_XY_ONLY 1
#define SSDR_FEED_GLOBAL_ROWS 2
int ssdr_feed_chain_dev(const float* d_points, const float* d_colors, int color_dim, const int32_t* d_labels, double* d_possibility,
                        double* d_cloud_min, int32_t* d_cloud_arg, const int64_t* cloud_offsets, size_t num_clouds,
                        size_t num_tiles, size_t num_points, const float* d_noise, const int32_t* d_perm, const float* d_dup_u, float color_scale,
                        float* d_out_xyz, float* d_out_feat, int32_t* d_out_idx, int32_t* d_out_labels, int32_t* d_out_cloud, float* d_out_center,
                        int flags, const double* d_class_weight, int num_labels, const float* d_activation, const float* d_pseudo,
                        float* d_out_activation, float* d_out_pseudo, void* stream);
int ssdr_feed_tiles_dev(const float* d_points, const float* d_colors, int color_dim, const int32_t* d_labels, const float* d_activation,
                        const float* d_pseudo, const int64_t* cloud_offsets, size_t num_clouds, size_t num_tiles, size_t num_points,
                        const int32_t* d_tile_cloud, const int32_t* d_tile_point, const float* d_noise, const int32_t* d_perm, const float* d_dup_u,
                        float color_scale, float* d_out_xyz, float* d_out_feat, int32_t* d_out_idx, int32_t* d_out_labels, float* d_out_activation,
                        float* d_out_pseudo, int32_t* d_out_cloud, float* d_out_center, void* stream);
int ssdr_feed_augment_dev(const float* d_xyz, size_t num_tiles, size_t num_points, const double* d_rot, const double* d_scale, const double* d_noise,
                          int color_dim, float* d_feat, void* stream);
int ssdr_feed_prefix_dev(const float* d_xyz, size_t num_tiles, size_t num_points, size_t num_sub, float* d_out, void* stream);
int ssdr_feed_status(void* stream, int32_t* out_status);

/* ---- RandLA-Net training (csrc/randla_train.hip; SSDR_AL_s3dis/RandLANet.py:36-84, :140-180, :486-585, helper_tf_util.py:111-246) ----
 * One handle holds the raw, unfolded network: per unit W, b, gamma, beta, the moving mean and variance, Adam's m and v.  float32 throughout.
 * Units in graph order: fc0 | per encoder level mlp1, LFAmlp1, LFAatt_pooling_1fc, LFAatt_pooling_1mlp, LFAmlp2, LFAatt_pooling_2fc,
 * LFAatt_pooling_2mlp, mlp2, shortcut | decoder_0 | Decoder_layer_0 .. L-1 | fc1, fc2, fc.
 * Parameter tensors, for each unit in that order: W, b (if the unit has a bias), gamma, beta, moving mean, moving variance (if it has a batch norm).
 *   ssdr_randla_train_param_shape: unit, kind (0 W, 1 b, 2 gamma, 3 beta, 4 moving mean, 5 moving variance), rows x cols as stored: W is
 *   [in, out], the Decoder_layer_j kernels (conv2d_transpose) [out, in]; vectors are [1, out].
 *   ssdr_randla_train_set_param / _get_param: host pointers, synchronous.  which = 0 the tensor, 1 Adam's m, 2 Adam's v (kinds 0..3 only).
 *   ssdr_randla_train_get_grad: the gradient the last step / grads call left (kinds 0..3).  _set_grad and _apply_dev (one Adam update from the
 *   gradients as they stand) exist for tests of the optimiser.
 * ssdr_randla_train_set_loss: class_weights f32 [num_classes] (NULL: ones); ignored_labels: labels dropped from the loss, the remaining labels
 *   shifted down as reducing_list does (:66-71), so labels run over 0 .. num_classes + n_ignored - 1.
 * The *_dev calls only enqueue on `stream`; the host reads no device value.  d_xyz / d_neigh / d_pool / d_interp: host arrays of num_layers
 *   device pointers: xyz_l f32 [B, N_l, 3], neigh_l i32 [B, N_l, 16], pool_l i32 [B, N_l+1, 16], interp_l i32 [B, N_l, 1] (tf_map's input_list);
 *   d_features f32 [B, N, in_dim], d_labels i32 [B N], d_activation / d_pseudo f32 [B N], d_drop_mask u8 [B N, 32] (1 = kept, scaled by 2).
 *   d_loss / d_accuracy (device f32, may be NULL) receive get_loss's mean over the valid rows and mean(argmax == label).
 *   _step_dev: forward (batch statistics, dropout), loss, backward, the moving statistics (momentum 0.99) and Adam as tf.train.AdamOptimizer
 *     (lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), p -= lr_t m / (sqrt(v) + 1e-8)).
 *   _grads_dev: forward and backward only: weights, moving statistics and the step count stay.
 *   _forward_dev: d_logits f32 [B N, num_classes] and d_feat32 f32 [B N, 32] (fc2's output before the dropout).  is_training = 0 normalises with the
 *     moving statistics and ignores the mask (may be NULL).
 *   By default the backward pass scatters with float atomicAdd: gradients and updated weights differ in their low bits from run to run; forward
 *   values do not.
 * ssdr_randla_train_set_deterministic(handle, on): on != 0 replaces the three backward scatters (gather_neighbour, nearest_interpolation,
 *   random_sample) with reductions over inverse lists built from the call's own index arrays (csrc/scatter_det.hip): every source row adds its
 *   positions in ascending order, no float atomic, so gradients and weights are the same bits every run.  Off is the default and launches the
 *   atomic kernels.  Changing it plans the workspace again at the next call; ssdr_randla_train_deterministic reads the switch back.
 * ssdr_randla_train_export: folds the batch norms with the moving statistics and loads an inference handle of the same configuration
 *   (ssdr_randla_set_layer's table, mlp2 and shortcut stacked).  Synchronous.
 * ssdr_randla_train_workspace_bytes: activation + gradient workspace of the last (B, N) laid out, in deterministic mode plus the lists, their
 *   sort scratch and the pooling shares.  ssdr_randla_train_last_ms: waits for the handle's
 *   last call; milliseconds of its forward, loss + backward and update parts (HIP events on its stream).
 * ssdr_randla_train_dropout_mask_dev: d_mask u8 [n] from a counter-based hash of (seed, step, index).
 * ssdr_randla_train_status: waits for `stream`; bit 0 = a loss without a valid row (loss and gradients are 0), bit 1 = a label or pseudo label outside
 *   the table (its row is dropped).  Clears the bits; SSDR_ERR_INVALID when one was set.
 * Refused before anything is launched: k_n != 16 (SSDR_ERR_UNSUPPORTED); NULL arguments, unset parameters, a level whose rows are not divisible by
 *   its ratio (SSDR_ERR_INVALID). */
int ssdr_randla_train_create(int num_layers, const int32_t* d_out, int k_n, int num_classes, int in_dim, void** handle);
void ssdr_randla_train_destroy(void* handle);
int ssdr_randla_train_num_params(void* handle);
int ssdr_randla_train_param_shape(void* handle, int i, int* unit, int* kind, int* rows, int* cols);
int ssdr_randla_train_set_param(void* handle, int i, int which, const float* host);
int ssdr_randla_train_get_param(void* handle, int i, int which, float* host);
int ssdr_randla_train_get_grad(void* handle, int i, float* host);
int ssdr_randla_train_set_grad(void* handle, int i, const float* host);
int ssdr_randla_train_apply_dev(void* handle, void* stream);
int ssdr_randla_train_set_loss(void* handle, const float* class_weights, const int32_t* ignored_labels, int n_ignored);
int ssdr_randla_train_set_lr(void* handle, float lr);
int ssdr_randla_train_set_step_count(void* handle, int64_t t);
int64_t ssdr_randla_train_step_count(void* handle);
size_t ssdr_randla_train_workspace_bytes(void* handle);
int ssdr_randla_train_last_ms(void* handle, float* out3);
int ssdr_randla_train_dropout_mask_dev(uint64_t seed, uint64_t step, size_t n, uint8_t* d_mask, void* stream);
int ssdr_randla_train_step_dev(void* handle, size_t B, size_t N, const float* d_features, const float* const* d_xyz, const int32_t* ratios,
                               const int32_t* const* d_neigh, const int32_t* const* d_pool, const int32_t* const* d_interp, const int32_t* d_labels,
                               const float* d_activation, const float* d_pseudo, const uint8_t* d_drop_mask, float* d_loss, float* d_accuracy, void* stream);
int ssdr_randla_train_grads_dev(void* handle, size_t B, size_t N, const float* d_features, const float* const* d_xyz, const int32_t* ratios,
                                const int32_t* const* d_neigh, const int32_t* const* d_pool, const int32_t* const* d_interp, const int32_t* d_labels,
                                const float* d_activation, const float* d_pseudo, const uint8_t* d_drop_mask, float* d_loss, float* d_accuracy, void* stream);
int ssdr_randla_train_forward_dev(void* handle, size_t B, size_t N, const float* d_features, const float* const* d_xyz, const int32_t* ratios,
                                  const int32_t* const* d_neigh, const int32_t* const* d_pool, const int32_t* const* d_interp, const uint8_t* d_drop_mask,
                                  int is_training, float* d_logits, float* d_feat32, void* stream);
int ssdr_randla_train_export(void* handle, void* net);
int ssdr_randla_train_status(void* stream, int32_t* out_status);
int ssdr_randla_train_set_deterministic(void* handle, int on);
int ssdr_randla_train_deterministic(void* handle);

/* The two atomic-free reductions of the deterministic mode as stand-alone pieces (csrc/scatter_det.hip); scratch per stream, enqueue only.
 * ssdr_scatter_add_rows_dev: d_idx i32 [B, rows_per_b] into src_rows rows per batch element, clamped to [0, src_rows - 1];
 *   dsrc[(b, idx[b, r]), c] += dout[(b, r), c] for c < C, where every source row first sums its positions in ascending r from +0 in float32 and
 *   then adds that sum to its old value; a row no position points at is not written.  ldo / lds: leading dimensions of dout / dsrc.
 * ssdr_pool_grad_rows_dev: the backward of the max over 16 pooled rows.  d_idx i32 [B, m_per_b, 16]; src / dsrc [B src_rows, C] (lds), out / dout
 *   [B m_per_b, C] (ldo).  Position r = m * 16 + k is tied when src[(b, idx[b, m, k]), c] == out[m, c]; a tied position contributes
 *   dout[m, c] / (float)ties(m, c), summed per source row in ascending r as above.
 * Refused (SSDR_ERR_INVALID): NULL pointers, C <= 0, a leading dimension below C.  B * rows_per_b == 0 is a no-op. */
int ssdr_scatter_add_rows_dev(const int32_t* d_idx, int B, int rows_per_b, int src_rows, const float* d_dout, int ldo, int C, float* d_dsrc, int lds,
                              void* stream);
int ssdr_pool_grad_rows_dev(const float* d_src, float* d_dsrc, int lds, int src_rows, const int32_t* d_idx, int B, int m_per_b, int C,
                            const float* d_out, const float* d_dout, int ldo, void* stream);

/* The training step's three launchers as stand-alone pieces (csrc/randla_train.hip); scratch per stream, enqueue only.  The tape of a step and
 * these pieces call the same launch functions: the tile choice (16x16, 256x16, 16x256, 64x64 by M and N), the dW split over rows and the reductions'
 * row chunks are the step's own.  All float32 with float32 accumulation.
 * ssdr_randla_train_gemm_dev: C[i crs + j ccs] (+)= sum_k A[i ars + k acs] B[k brs + j bcs] (+ bias[j]) for i < M, j < N, k < K, one fmaf chain
 *   over k from +0; `accumulate` != 0 adds to C's old value, otherwise C is overwritten.  Nothing outside those M x N elements is written.
 * ssdr_randla_train_dw_dev: dW[i rs + j cs] = sum_r x[r ldx + i] dz[r out + j] for i < in, j < out over r < M (dz dense [M, out]); the rows are
 *   split into slabs of a multiple of 16 rows (one per 512 rows, at most 1024, at most what 2^23 floats of [in][out] slabs hold), one fmaf chain
 *   per slab, the slabs added in order from +0.
 * ssdr_randla_train_reduce_dev: per channel c < C over the M rows of z (leading dimension ldz), in row chunks merged in order:
 *   mode 0: out0 = mean, out1 = 1 / sqrt(biased variance + 1e-6) (chunk means and squared deviations, Chan's merge); with d_mov_mean / d_mov_var
 *     (both or neither): moving -= (moving - x) * 0.01, x the mean and the variance (times M / (M - 1) when unbiased != 0 and M > 1).
 *   mode 1: out0 = sum dY, out1 = sum dY (z - mean[c]) invstd[c], dY = da[r lda + c], times 0.2 where act != 0 and not av[r lda + c] > 0.
 *   mode 2: out0 = sum z (out1 unused).
 * Refused (SSDR_ERR_INVALID): NULL pointers, sizes <= 0, a leading dimension below its width, in * out > 2^23. */
int ssdr_randla_train_gemm_dev(const float* d_A, int64_t ars, int64_t acs, const float* d_B, int64_t brs, int64_t bcs, float* d_C, int64_t crs, int64_t ccs,
                               int M, int N, int K, const float* d_bias, int accumulate, void* stream);
int ssdr_randla_train_dw_dev(const float* d_x, int ldx, const float* d_dz, int M, int in, int out, float* d_dW, int64_t rs, int64_t cs, void* stream);
int ssdr_randla_train_reduce_dev(int mode, const float* d_z, int ldz, const float* d_da, const float* d_av, int lda, int act, const float* d_mean,
                                 const float* d_invstd, int M, int C, float* d_out0, float* d_out1, float* d_mov_mean, float* d_mov_var, int unbiased,
                                 void* stream);

/* ---- data-parallel training: one process per GPU, every rank a replica (csrc/train_exchange.hip, DESIGN section 21 "Data-parallel") ----
 * The library links no collective library.  With an exchange set, _step_dev, _grads_dev and _forward_dev(is_training = 1) call `fn` where the ranks
 * must meet; `fn` only ENQUEUES the collective on `stream` (the call's stream) and returns 0, the host reads no device value.  The step is then the
 * step of ONE process over the union of all ranks' tiles: batch norm over all ranks' rows (forward and backward), the loss over the global number
 * of valid rows, one gradient sum.  Ranks may hold different B; every rank must make the same calls in the same order.
 *   SSDR_XCHG_GATHER: d_recv [world][count] <- every rank's d_send [count], in rank order.
 *   SSDR_XCHG_SUM:    d_recv [count] (may equal d_send) <- the element-wise sum over the ranks, the same bits on every rank.
 * Meeting points: per batch-normed unit one GATHER of [n_r | mean[C] | M2[C]] in the forward pass (merged by Chan's formula in rank order from
 *   n = 0; the moving statistics take the global values, the unbiased factor n / (n - 1) the global count) and one GATHER of [dgamma[C] | dbeta[C]]
 *   in the backward pass (summed in rank order; the norm's backward divides by the global count); one GATHER of the loss's three sums (d_loss,
 *   d_accuracy are global and identical on every rank; status bit 0 only when NO rank has a valid row); ONE SUM over the whole gradient arena
 *   before Adam (ranks other than 0 zero their gamma / beta gradients first: those are global already).  After it every rank holds the union's
 *   gradient with the same bits, so replicas that start identical stay identical; weights are never broadcast.
 *   _forward_dev(is_training = 0) and _apply_dev do not meet.
 * ssdr_randla_train_set_exchange: fn NULL (with world <= 1): back to one process.  Refused (SSDR_ERR_INVALID) before anything changes: world < 1,
 *   rank outside [0, world), fn NULL with world > 1.  ssdr_randla_train_exchange reads rank and world back (world 0: none set).
 *   A callback that returns non-zero fails the call with SSDR_ERR_INVALID, "exchange failed".  The send [1 + 2 Cmax] and receive
 *   [world][1 + 2 Cmax] buffers are part of ssdr_randla_train_workspace_bytes.  Without an exchange every call launches what it launched before.
 * The merges as stand-alone pieces, enqueue only:
 * ssdr_bn_stats_merge_dev: d_records f32 [world][1 + 2C] -> d_mean [C], d_invstd [C] = 1 / sqrt(M2 / n + 1e-6), d_count [1] = n; when
 *   d_mov_mean / d_mov_var are not NULL (both or neither): moving -= (moving - x) * 0.01 with x the mean and the variance (times n / (n - 1) when
 *   unbiased != 0 and n > 1).  A record with n_r = 0 is skipped.
 * ssdr_rank_sums_merge_dev: d_records f32 [world][n] -> d_out[i] = ((0 + r0[i]) + r1[i]) + ...
 * ssdr_randla_train_dropout_mask_range_dev: elements first .. first + n - 1 of the mask of (seed, step): a rank's mask is the slice of the union's.
 *   first = 0 is ssdr_randla_train_dropout_mask_dev.
 * Refused (SSDR_ERR_INVALID): NULL pointers, world < 1, C < 1, n < 1. */
typedef int (*ssdr_exchange_fn)(void* user, int op, const float* d_send, float* d_recv, size_t count, void* stream);
#define SSDR_XCHG_GATHER 0
#define SSDR_XCHG_SUM    1
int ssdr_randla_train_set_exchange(void* handle, ssdr_exchange_fn fn, void* user, int rank, int world);
int ssdr_randla_train_exchange(void* handle, int* rank, int* world);
int ssdr_bn_stats_merge_dev(const float* d_records, int world, int C, float* d_mean, float* d_invstd, float* d_count, float* d_mov_mean, float* d_mov_var,
                            int unbiased, void* stream);
int ssdr_rank_sums_merge_dev(const float* d_records, int world, int n, float* d_out, void* stream);
int ssdr_randla_train_dropout_mask_range_dev(uint64_t seed, uint64_t step, uint64_t first, size_t n, uint8_t* d_mask, void* stream);

/* ---- per-row draws of the tile generators, made on the device (csrc/draw.hip) ----
 * Every value is a pure function of a counter (seed u64, epoch u32, step u32, kind u32, element u64, word u32); nothing depends on the launch.
 * All arithmetic is on uint32, modulo 2^32:
 *   mix32(x):   x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16          (the dropout mask's mixer)
 *   state(c):   s = mix32(lo32(seed) ^ c); s = mix32(s ^ hi32(seed)); s = mix32(s ^ epoch); s = mix32(s ^ step); s = mix32(s ^ kind)
 *   chain(c, e, j): a = mix32(state(c) ^ lo32(e)); a = mix32(a + hi32(e)); a = mix32(a ^ j)
 *   word(e, j): mix32(chain(0x9e3779b9, e, j) + chain(0x85ebca6b, e, j))
 * Two chains, because one alone is a bijection of lo32(e): a tile's keys would be one fixed bijection of an aligned block of integers.
 *   bits53(e, j): (word(e, j) >> 5) * 2^26 + (word(e, j + 1) >> 6), an integer in [0, 2^53)
 * ssdr_draw_perm_dev: d_perm i32 [num_tiles, num_points]; row t is the stable argsort over r < num_points of
 *   key(T, r) = word(T * 2^32 + r, 0) >> (32 - key_bits) with T = first_tile + t and kind = SSDR_DRAW_PERM: ascending key, equal keys by ascending r.
 *   key_bits = 32 is the generators' choice (smaller values force ties).  first_tile: tiles [first_tile, first_tile + num_tiles) of a larger
 *   call, row for row.  Refused before anything is launched: NULL, num_tiles or num_points 0, key_bits outside 1 .. 32, a tile id of 2^32 or
 *   more (SSDR_ERR_INVALID); more than 0x3fffffff pairs in the sort buffers, where every tile of more than 1024 rows owns its rows rounded up to a
 *   multiple of 2048 and smaller tiles are packed, up to 65536 together, and rounded up likewise (SSDR_ERR_UNSUPPORTED).
 * ssdr_draw_uniform_dev: d_out f32 [n], d_out[i] = (word(first + i, 0) >> 8) * 2^-24, in [0, 1 - 2^-24] (the rule of NumPy's float32 random).
 * ssdr_draw_normal_dev: d_out f64 [n], d_out[i] = scale * z(first + i) by Box-Muller in float64, every product and call rounded on its own:
 *   u1 = (bits53(e, 0) + 1) * 2^-53 in (0, 1], u2 = bits53(e, 2) * 2^-53 in [0, 1), z = sqrt(-2 * log(u1)) * cos(6.283185307179586 * u2).
 *   log and cos are the platform's: builds agree to a few units in the last place, not bit for bit.
 * first makes a rank's draws the slice of the union's, as ssdr_randla_train_dropout_mask_range_dev does.  Both refuse NULL and n = 0 (SSDR_ERR_INVALID).
 * The generators use element = tile * num_points + r for SSDR_DRAW_DUP and (tile * num_points + r) * 3 + axis for SSDR_DRAW_AUG_NOISE.
 * All three only enqueue; the host reads no device value; the permutation's sort scratch is kept per stream. */
#define SSDR_DRAW_PERM 0
#define SSDR_DRAW_DUP 1
#define SSDR_DRAW_AUG_NOISE 2
int ssdr_draw_perm_dev(uint64_t seed, uint32_t epoch, uint32_t step, uint64_t first_tile, size_t num_tiles, size_t num_points, int key_bits,
                       int32_t* d_perm, void* stream);
int ssdr_draw_uniform_dev(uint64_t seed, uint32_t epoch, uint32_t step, uint32_t kind, uint64_t first, size_t n, float* d_out, void* stream);
int ssdr_draw_normal_dev(uint64_t seed, uint32_t epoch, uint32_t step, uint32_t kind, uint64_t first, size_t n, double scale, double* d_out,
                         void* stream);

/* ---- the seed, random and label-all samplers (S3/sampler2.py:344-520; csrc/select_random.hip) ----
 * ssdr_region_draw_dev: ONE iteration of RandomSampler._iteration / SeedSampler._iteration as an item list, with the draws of the chain above
 * (epoch = round, step = iteration).  d_labeled uint8 [S] (non-zero: labelled), d_sp_cloud i32 [S] ascending, values below num_clouds.
 *   live clouds: those with an unlabelled region, in ascending order, L of them; u(d) = the unlabelled regions of live cloud d.
 *   k = *d_count (device int64: the clicks left, or the seeds still to place).  The k drawn elements of range(total_num) are the k smallest by
 *     (word(e, 0) >> (32 - key_bits), e) under kind SSDR_DRAW_REGION_COUNT;  each_file_number(d) = the number of drawn e with e % L == d.
 *   cloud d with 0 < each_file_number(d) <= u(d): its first each_file_number(d) unlabelled regions by ascending
 *     (word(g, 0) >> (32 - key_bits), g) under kind SSDR_DRAW_REGION_PICK, g = first_region + region id, in that order;
 *   cloud d with each_file_number(d) > u(d): all its unlabelled regions by ascending id; the shortfall adds to the seed remainder.
 *   d_items [max_items] / *d_n_items: the clouds in live order, each cloud's picks in pick order.
 * SSDR_REGION_ALL (AllSampler): every unlabelled region of every cloud in ascending order; d_count is not read.
 * d_info int64 [8]: [0] live clouds, [1] k, [2] items (before the clamp to max_items), [3] the seed remainder, [4] unlabelled regions left once every
 *   item is labelled, [5] status (1: k > total_num, nothing is drawn — np.random.choice raises; 2: more items than max_items; 4: a region's cloud is
 *   outside the table: the region takes no part), [6], [7] zero.
 * ssdr_seed_label_dev: _help_seed (:232-237) over the items: d_mask[p] = 1, d_label[p] = d_gt[p] for every point of every item, d_labeled[item] = 1;
 *   d_out int64 [3]: sp_num, p_num, status (4: an item or point id outside the arrays; it is skipped).  max_region: as for ssdr_oracle_label_dev.
 * Both only enqueue, with scratch per stream.  Refused before anything is launched: NULL pointers, S = 0, total_num = 0, key_bits outside 1 .. 32, an
 * unknown mode (SSDR_ERR_INVALID); more than 0x3fffffff regions, elements or items (SSDR_ERR_UNSUPPORTED).  *d_count lives on the device: a count above
 * total_num is refused there, by status bit 1 and an empty list. */
#define SSDR_DRAW_REGION_COUNT 3
#define SSDR_DRAW_REGION_PICK 4
#define SSDR_REGION_RANDOM 0
#define SSDR_REGION_ALL    1
int ssdr_region_draw_dev(uint64_t seed, uint32_t round, uint32_t iteration, int mode, int key_bits, uint64_t first_region, const uint8_t* d_labeled,
                         const int32_t* d_sp_cloud, size_t S, size_t num_clouds, size_t total_num, const int64_t* d_count, int32_t* d_items, size_t max_items,
                         int32_t* d_n_items, int64_t* d_info, void* stream);
/* Read-only view of the newest ssdr_region_draw_dev call on `stream` (waits for the stream): out (host) [n] = each_file_number of the first n live clouds,
 * n at most that call's num_clouds (SSDR_ERR_INVALID beyond, and before the first call). */
int ssdr_region_draw_shares(void* stream, int32_t* out, size_t n);
int ssdr_seed_label_dev(const int32_t* d_gt, size_t n, const int32_t* d_sp_off, const int32_t* d_sp_pts, size_t S, const int32_t* d_items, const int32_t* d_n_items,
                        size_t max_items, size_t max_region, float* d_mask, float* d_label, uint8_t* d_labeled, int64_t* d_out, void* stream);
/* The draw over a pool whose clouds lie on `world` ranks, contiguous shares in rank order: the union has a global cloud order and a global region id
 * (first_region = the regions of the ranks before, + the local id), and a rank's share of every result is, index for index, ssdr_region_draw_dev over
 * the union.  Two halves around ONE all-gather that the caller runs on the same stream:
 *   ssdr_region_draw_count_dev: d_u int32 [cloud_slots + 1] <- this rank's unlabelled regions per cloud, zero at and behind num_clouds; the last word:
 *     the rank's status bits (4: a region's cloud is outside the table).  cloud_slots: the largest cloud count of any rank, the same on all ranks.
 *   the all-gather of d_u into d_u_all [world][cloud_slots + 1], rank-major.
 *   ssdr_region_draw_sharded_dev: the live clouds, L, k, each_file_number, every cloud's take and first item over ALL ranks' clouds (global cloud =
 *     rank * cloud_slots + cloud; replicated: total_num keys on every rank, as in one process), then the picks of this rank's own regions under their
 *     cloud's global live rank and the word of g = first_region + region id.  d_items [max_items]: this rank's items as LOCAL ids, d_item_pos
 *     [max_items] their positions in the union's list, ascending; *d_n_items of both are live.
 *     d_info: [0] .. [4] the global values as above, [5] the OR of all ranks' status bits 1 and 4 and this rank's own bit 2, [6] this rank's items
 *     (before the clamp to max_items), [7] zero.  ssdr_region_draw_shares afterwards: the global each_file_number.
 * With world = 1 the two halves give ssdr_region_draw_dev's outputs.  Both only enqueue; refused before anything is launched, beyond the refusals above:
 * world = 0, rank outside [0, world), cloud_slots < num_clouds (SSDR_ERR_INVALID); world * cloud_slots or first_region + S above 0x3fffffff
 * (SSDR_ERR_UNSUPPORTED).  The scans sum the union's counts in 32 bits and a low rank cannot see the union's size: the caller, who sized the all-gather,
 * keeps the regions of ALL ranks at or below 0x3fffffff.  A region whose cloud d_u_all counts as dead (tables of another mask) is not emitted. */
int ssdr_region_draw_count_dev(const uint8_t* d_labeled, const int32_t* d_sp_cloud, size_t S, size_t num_clouds, int32_t* d_u, size_t cloud_slots, void* stream);
int ssdr_region_draw_sharded_dev(uint64_t seed, uint32_t round, uint32_t iteration, int mode, int key_bits, uint64_t first_region, int rank, int world,
                                 const int32_t* d_u_all, size_t cloud_slots, const uint8_t* d_labeled, const int32_t* d_sp_cloud, size_t S, size_t num_clouds,
                                 size_t total_num, const int64_t* d_count, int32_t* d_items, int32_t* d_item_pos, size_t max_items, int32_t* d_n_items, int64_t* d_info,
                                 void* stream);

/* ---- the radix sort under every stage, alone (csrc/radix_sort.hip) ----
 * Stable sort of (u64 word, u32 value) pairs by bits [shift, shift + key_bits) of the word, 8 bits per pass, over nseg <= 64 independent segments of
 * one buffer.  Every argument is handed to RadixSorter::sort_segments as it comes:
 *   d_keys   device u64 [off[nseg]]; segment i owns the slots [off[i], off[i + 1]), off[i] a multiple of 2048, its live pairs are the first
 *            cnt[i] = min(d_cnt[i], n_host[i]) of them (n_host[i] without d_cnt); the slots behind them are neither read nor written.  Bits at and above
 *            shift + key_bits must be zero; what sits below `shift` travels with its word
 *   d_vals   device u32 [off[nseg]], or NULL: keys only
 *   off      host int32 [nseg + 1];  n_host  host int32 [nseg];  d_cnt  device int32 [nseg], or NULL
 *   d_andor  device u64 [nseg][2], or NULL: AND and OR of every segment's words when the caller knows them (any subset of the AND's bits and superset of
 *            the OR's will do, an empty segment gives ~0, 0); NULL: a pre-pass reads the keys.  A pass whose digit AND and OR agree on in every
 *            segment is skipped on the device
 *   flags    SSDR_SORT_WIDE_HIGH: RadixSorter::wide_high for this call (from 16 384 pairs on the passes above bit 32 run as wide passes, not in the
 *            one-workgroup kernel).  SSDR_SORT_INPUT_IN_ALT: the sorter's input_in_alt protocol — the entry reserves, copies the off[nseg] slots of
 *            d_keys / d_vals into the sorter's own buffers, fills d_keys / d_vals with the byte 0xA5 and sorts from there: the result comes home to
 *            d_keys / d_vals, the slots no live pair lands in keep the fill.  Any other bit: SSDR_ERR_INVALID
 * nseg <= 0 or off[nseg] <= 0: SSDR_OK, nothing is touched.  nseg > 64, an off[i] that is no multiple of 2048, off[i + 1] < off[i] + n_host[i],
 * shift < 0 or shift + key_bits > 64: SSDR_ERR_INVALID, nothing is touched.  The sorter belongs to `stream` and to this entry alone: calls on one
 * stream reuse it (its buffers grow), a new stream starts from nothing. */
#define SSDR_SORT_WIDE_HIGH    1
#define SSDR_SORT_INPUT_IN_ALT 2
int ssdr_radix_sort_dev(uint64_t* d_keys, uint32_t* d_vals, int nseg, const int32_t* off, const int32_t* n_host, const int32_t* d_cnt, int key_bits,
                        int shift, const uint64_t* d_andor, int flags, void* stream);
/* Read-only view of the newest ssdr_radix_sort_dev call on `stream` (waits for the stream; changes nothing).  out8 (host): what the host decided when
 * it launched — [0] wide passes launched (npass), [1] 1 when the passes above bit 32 were chosen wide, [2] 1 when the one-workgroup kernel for them
 * (rs_high_passes) was launched, [3] grid of rs_hist / rs_scatter (g), [4] grid.x of the AND/OR pre-pass (gao; computed also when d_andor replaced the
 * pre-pass), [5] the segment grid rs_finish is sized by (gseg), [6] tiles of the buffer (nb), [7] the row length of the histogram table (nblocks_max).
 * All zero after a call that was refused or had nothing to sort, and before the first call.
 * words_out (optional, host u64 [2 * nseg] of that call): AND and OR per segment as the kernels used them (the pre-pass's result or the caller's
 * d_andor), copied back from the sorter; left untouched when out8 is all zero. */
int ssdr_radix_sort_info(void* stream, int32_t* out8, uint64_t* words_out);

/* ---- plain device memory for callers without their own allocator (tests, the ctypes mirror) ---------- */
int ssdr_dev_alloc(size_t bytes, void** d_ptr);
int ssdr_dev_free(void* d_ptr);
int ssdr_memcpy_h2d(void* d_dst, const void* src, size_t bytes);
int ssdr_memcpy_d2h(void* dst, const void* d_src, size_t bytes);
/* the same, ordered on `stream` (NULL = library stream) and waiting for that stream only: a selection that runs on its own stream
 * uploads its index tables and reads its result back without waiting for what the other streams hold */
int ssdr_memcpy_h2d_on(void* d_dst, const void* src, size_t bytes, void* stream);
int ssdr_memcpy_d2h_on(void* dst, const void* d_src, size_t bytes, void* stream);

/* cpp_knn_batch_distance_pick (knn_.h:21-23, knn_.cxx:136-203, knn.pyx:111-149): nqueries "least used first" query points
 * per batch element and their K neighbours.  The reference seeds std::mt19937 with time(0); here the seed is an argument
 * (the same seed gives the reference's result).  batch_queries [B][nqueries][dim], batch_indices [B][nqueries][K]. */
int ssdr_knn_batch_distance_pick(const float* batch_data, size_t batch_size, size_t npts, size_t dim, float* batch_queries,
                                 size_t nqueries, size_t K, int64_t* batch_indices, uint32_t seed);

/* ---- superpoint-graph inputs (the partition itself, cut-pursuit, stays out of scope) -----------------
 * compute_graph_nn_2 (partition/graphs.py:23-70, voronoi == 0): sklearn's exact float64 k-NN.  source/target/distances
 * [n*k_nn1] of the adjacency graph (neighbour j of point i at i*k_nn1 + j, the point itself dropped), target2 [n*k_nn2].
 * Equidistant neighbours (sklearn leaves their order open) come in the order the kd-tree walk meets them. */
int ssdr_knn_graph_dev(const float* d_xyz, size_t n, size_t k_nn1, size_t k_nn2, uint32_t* d_source, uint32_t* d_target,
                       float* d_distances, uint32_t* d_target2, void* stream);
/* libply_c.compute_geof (partition/ply_c/ply_c.cpp:385-455): [n,4] = linearity, planarity, scattering, verticality of
 * every point and its k_nn neighbours d_target[n*k_nn]. */
int ssdr_geof_dev(const float* d_xyz, size_t n, const uint32_t* d_target, size_t k_nn, float* d_geof, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSDR_AL_H */
