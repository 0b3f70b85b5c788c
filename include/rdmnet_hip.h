/* librdmnet_hip.so -- C-ABI of the MI355X (gfx950) implementation of RDMNet's dense-matching
 * inference path.  Plain pointers and sizes only; no torch types.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter name ends in `_host`;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises
 *     unless the function's comment says so;
 *   - `ws`/`ws_bytes` is caller-owned scratch (query the size with the matching *_workspace_bytes);
 *     the library never allocates or frees caller memory and keeps no global state (re-entrant) -- the diagnostic
 *     counters of the lock-step scheduler (rdm_lockstep_stats*, marked DIAGNOSTIC below) are the one exception;
 *   - return value: 0 = ok, <0 = error (see rdm_last_error(), thread-local);
 *   - data-dependent overflows on the device are reported through a caller-provided int32 `status`
 *     word (device memory, must be zero before the call; non-zero afterwards = RDM_ERR_CAPACITY).
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference
 * repository root).
 */
#ifndef RDMNET_HIP_H_
#define RDMNET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDM_ABI_VERSION 2   /* 2: rdm_engine_result / rdm_data_dict / rdm_kpconv_profile grew, three entry points left (round 3);
                               parameter sets are reference counted (round 4) */

int rdm_abi_version(void);
/* sizeof of the structs that cross this boundary, so that a binding can verify its own layout against the library it
 * loaded: which = 0 rdm_engine_config, 1 rdm_engine_result, 2 rdm_tensor_view, 3 rdm_kpconv_profile, 4 rdm_data_dict;
 * anything else returns 0.                                                                                        */
size_t rdm_abi_struct_size(int which);
const char* rdm_last_error(void);

/* libstdc++ std::unordered_map growth schedule used by rdm_grid_subsample to reproduce the
 * reference's output order: rehash to `buckets[j]` happens when the map already holds `at[j]`
 * elements.  Host-only helper (no GPU needed).  Returns the number of entries written. */
int rdm_rehash_schedule(int64_t max_elems, int64_t* at_host, int64_t* buckets_host, int cap);

/* ---- a1: voxel-grid subsampling ------------------------------------------------------------
 * Replaces rdmnet.ext.grid_subsampling
 *   (geotransformer/extensions/pybind.cpp:13-17,
 *    geotransformer/extensions/cpu/grid_subsampling/grid_subsampling.cpp:5-62,
 *    geotransformer/extensions/cpu/grid_subsampling/grid_subsampling_cpu.cpp:3-75).
 * points [n_points,3] f32 stacked clouds, lengths [batch] i64.  Writes the barycentres of the
 * occupied voxels of each cloud, stacked, in the reference's order (libstdc++ unordered_map
 * iteration order) into out_points (capacity n_points rows) and the per-cloud counts into
 * out_lengths [batch] i64.  No synchronisation: the caller reads out_lengths when it needs the
 * row count.                                                                                  */
size_t rdm_grid_subsample_workspace_bytes(int64_t n_points, int batch);
int rdm_grid_subsample(const float* points, int64_t n_points, const int64_t* lengths, int batch,
                       float voxel_size, float* out_points, int64_t* out_lengths, void* ws,
                       size_t ws_bytes, void* stream);
/* The same with the kernel form chosen by the caller: 0 = by size (what rdm_grid_subsample does: from 16 384 stacked points
 * the phases before the hash-map order replay run as separate launches over many workgroups), 1 = one workgroup per cloud
 * for every phase, 2 = the multi-launch form.  Identical output bit for bit (tests/test_native_gpu.py).                  */
int rdm_grid_subsample_form(const float* points, int64_t n_points, const int64_t* lengths, int batch, float voxel_size,
                            float* out_points, int64_t* out_lengths, void* ws, size_t ws_bytes, void* stream, int form);

/* ---- a2: radius neighbours -----------------------------------------------------------------
 * Replaces rdmnet.ext.radius_neighbors
 *   (geotransformer/extensions/pybind.cpp:8-12,
 *    geotransformer/extensions/cpu/radius_neighbors/radius_neighbors.cpp:5-68,
 *    geotransformer/extensions/cpu/radius_neighbors/radius_neighbors_cpu.cpp:3-91)
 * and the column truncation of geotransformer/modules/ops/radius_search.py:24-26.
 * For every query of cloud b: all support points of cloud b with fp32 d2 < radius*radius, ascending
 * by (d2, index), as GLOBAL support indices; unused slots hold n_s.
 *   out_idx    [n_q, width] i64 (row stride = width); may be NULL when width == 0 (count-only pass)
 *   out_counts [n_q] i32 untruncated neighbour counts (may be NULL)
 *   out_max    [1] i32, atomically max-ed with the largest count (may be NULL; zero it first)
 *   status     [1] i32, non-zero on an internal error (2: the grid was built for a smaller radius).  There is no
 *              neighbour-count limit: rows beyond the kernels' 1024-key buffer are produced in rounds of a radix
 *              select over the (d2, index) keys, like the reference (radius_neighbors_cpu.cpp:36-64) returns them all
 * The reference's output width is max(count); call once with width = 0 to obtain it, or pass the
 * neighbour limit directly (the first min(limit, max) columns are identical).                  */
size_t rdm_radius_neighbors_workspace_bytes(int64_t n_q, int64_t n_s, int batch);
int rdm_radius_neighbors(const float* q_points, int64_t n_q, const float* s_points, int64_t n_s,
                         const int64_t* q_lengths, const int64_t* s_lengths, int batch,
                         float radius, int width, int64_t* out_idx, int32_t* out_counts,
                         int32_t* out_max, int32_t* status, void* ws, size_t ws_bytes,
                         void* stream);

/* The same search in two steps, so that several query sets share one grid over a support cloud (the
 * collate searches every level three times with the same radius: self, from the coarser and from the
 * finer level).  `radius` of a query must not exceed the radius the grid was built with (status = 2). */
size_t rdm_radius_grid_workspace_bytes(int64_t n_s);
int rdm_radius_grid_build(const float* s_points, int64_t n_s, const int64_t* s_lengths, int batch, float radius,
                          void* grid_ws, size_t grid_ws_bytes, void* stream);
int rdm_radius_grid_query(void* grid_ws, size_t grid_ws_bytes, int64_t n_s, const float* q_points, int64_t n_q,
                          const int64_t* q_lengths, int batch, float radius, int width, int64_t* out_idx,
                          int32_t* out_counts, int32_t* out_max, int32_t* status, void* ws, size_t ws_bytes,
                          void* stream);

/* The grid's support records in cell order: n_s x {x, y, z, bit pattern of the int32 row index}.  Rows of
 * one cell are contiguous, which makes the 4th component a spatially coherent processing order. */
const float* rdm_radius_grid_records(void* grid_ws, size_t grid_ws_bytes, int64_t n_s);

/* Calibration of the neighbour limits (geotransformer/utils/data.py:195-220): hist[c] += #{i : counts[i] == c}
 * for c < hist_n, i.e. the reference's np.bincount(counts, minlength=hist_n)[:hist_n] accumulated over calls.
 * counts = out_counts of a width-0 (count-only) rdm_radius_neighbors call.  hist_n <= 1024. */
int rdm_neighbor_histogram(const int32_t* counts, int64_t n, int32_t* hist, int hist_n, void* stream);

/* ---- §8f rank 3: raw-scan preprocessing --------------------------------------------------------
 * Centroid voxel down-sampling of one raw scan: points[n, ld] f32 with `channels` >= 3 leading columns
 * (x, y, z, then e.g. intensity) -> out[m, ldo], m in *out_count (device int32).  Replaces
 * preporcess/downsample_pcd_kitti.py:21-36 (Open3D 0.11.2 voxel_down_sample(0.3) on points + colors):
 * index = floor((p - (min_bound - voxel/2)) / voxel) in float64, per-voxel means accumulated in float64.
 * Open3D is not part of the reference tree -> parity unpinned; voxels are emitted in first-occurrence
 * order (Open3D's hash-map order is unspecified).  status (device int32, caller zeroes): 1 = a point is
 * non-finite or more than 2^21 voxels from the minimum (point skipped).  n < 2^26.                    */
size_t rdm_voxel_downsample_workspace_bytes(int64_t n);
int rdm_voxel_downsample(const float* points, int64_t n, int64_t ld, int channels, double voxel, float* out,
                         int64_t ldo, int32_t* out_count, int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- §8f rank 4: RANSAC pose from correspondences ------------------------------------------------
 * The reference's second evaluation mode (experiments/infer.py:75-82, eval.py:179-186 ->
 * geotransformer/utils/open3d.py:173-203: Open3D registration_ransac_based_on_correspondence, point-to-point,
 * ransac_n 4, 50 000 iterations, 0.3 m).  src_corr/ref_corr: device f32 [n_corr, 3].  Every iteration draws
 * ransac_n correspondences with replacement (counter-based hash of (seed, iteration, draw)), fits a rigid
 * transform (float64 Kabsch), scores it on all correspondences (float64); the winner is the iteration with
 * most inliers, then lowest inlier RMSE, then lowest index; its transform is returned without refit.
 * Outputs (device): transform f32[16] row-major 4x4 (identity if nothing fits), stats int32[2] =
 * {winning iteration or -1, its inliers}, inlier_rmse f32[1], optional hyp_inliers int32[num_iterations].
 * Open3D is not part of the reference tree -> parity unpinned (checked against oracle/preprocess.py).   */
size_t rdm_ransac_workspace_bytes(int num_iterations);
int rdm_ransac_correspondences(const float* src_corr, const float* ref_corr, int64_t n_corr, float distance_threshold,
                               int ransac_n, int num_iterations, uint64_t seed, float* transform, int32_t* stats,
                               float* inlier_rmse, int32_t* hyp_inliers, void* ws, size_t ws_bytes, void* stream);

/* ---- §7 ICP / pair generation: point-to-point ICP --------------------------------------------------
 * The ground-truth refinement of preporcess/generate_kitti_pairs.py:157-172 (Open3D registration_icp,
 * TransformationEstimationPointToPoint without scaling, ICPConvergenceCriteria; 0.5 m, up to 5000 iterations, on
 * raw scans).  source [n_source, ld_source] / target [n_target, ld_target]: device f32, xyz in the first three
 * columns.  pcd = init . source (float64; untouched for the identity), transformation = init, evaluate; then up to
 * max_iteration times: update = Kabsch of the correspondences (identity without any), transformation = update .
 * transformation, pcd = update . pcd, evaluate; stop when |d fitness| < relative_fitness and |d rmse| <
 * relative_rmse.  Evaluate: nearest target with d2 < r2, r2 = (double)(float)(r*r), d2 = ((dx*dx)+(dy*dy))+(dz*dz) in
 * float64 on the float32 targets, ties to the lowest index; fitness = n_corr / n_source, rmse = sqrt(err2 / n_corr).
 * init_host: host f64[16] row-major (NULL = identity).  Outputs (device): transform f64[16], fitness_rmse f64[2] of
 * the last evaluation, stats int32[2] = {updates applied, n_corr}; history (optional, device) f64[(max_iteration+1)
 * x 15], record k = {fitness_k, rmse_k, n_corr_k, update_k (12, the update computed from evaluation k and applied
 * after it; the identity in the last record, after which no update follows)}.  The host reads one int32 per 32
 * iterations.  max_correspondence_distance <= 0 is an argument error; an empty source returns init with fitness 0;
 * a target point that is not finite (or beyond 2^30 cells of r from the origin) is an argument error.
 * n_source, n_target < 2^31.  Open3D is not part of the reference tree -> parity unpinned.                    */
size_t rdm_icp_workspace_bytes(int64_t n_source, int64_t n_target);
int rdm_icp_point_to_point(const float* source, int64_t n_source, int64_t ld_source, const float* target, int64_t n_target,
                           int64_t ld_target, double max_correspondence_distance, const double* init_host, int max_iteration,
                           double relative_fitness, double relative_rmse, double* transform, double* fitness_rmse,
                           int32_t* stats, double* history, void* ws, size_t ws_bytes, void* stream);
/* The evaluation step alone (preporcess/generate_kitti_pairs.py:157-172, inside Open3D's registration_icp; parity
 * unpinned) on a caller's float64 query cloud pcd [n, 3] (device): idx int32[n] = nearest target with d2 < r2
 * (lowest index among equal d2) or -1, d2 f64[n] = its squared distance (-1 where idx is -1).  Same semantics, bit for
 * bit, as the search inside rdm_icp_point_to_point; workspace rdm_icp_workspace_bytes(0, n_target).            */
int rdm_icp_correspondences(const double* pcd, int64_t n, const float* target, int64_t n_target, int64_t ld_target,
                            double max_correspondence_distance, int32_t* idx, double* d2, void* ws, size_t ws_bytes,
                            void* stream);

/* ---- ground-truth point correspondences and cloud overlap (ball_query.hip) -------------------
 * get_correspondences and compute_overlap (geotransformer/utils/registration.py:191-216) as one fixed-radius ball query
 * between two full clouds.  ref [n_ref, >=3] / src [n_src, >=3]: device f32, row strides ld_ref / ld_src (xyz first);
 * transform_host: row-major float64 4x4 on the HOST, src -> ref (null: src as it is).  Points are read as double,
 * x' = ((R00 x + R01 y) + R02 z) + t0, d2 = ((dx dx) + (dy dy)) + (dz dz) with d = ref - src', r2 = radius * radius in double,
 * nothing contracted.  (i, j) is a correspondence iff d2 <= r2 (closed, as cKDTree's ball); a row overlaps iff the smallest
 * d2 of its correspondences has sqrt(d2) < radius (strict, as compute_overlap).
 * rdm_ball_count builds the cell index of the moved src cloud, counts per ref row and leaves index, counts and int64 offsets
 * in the workspace.  Optional device outputs: ref_min_d2 f64 [n_ref] (the row's smallest d2, -1 without a correspondence),
 * ref_hit u8 [n_ref] / src_hit u8 [n_src rounded up to a multiple of 4 bytes, 4-byte aligned] (1 iff the row appears in a
 * correspondence).  totals_host (host int64[4], the call's one read-back, after which the stream is idle) = {C, overlapping
 * ref rows, overlapping src rows, status}.  A point that is not finite, or a moved src point beyond 2^30 cells of `radius`
 * from the origin, is RDM_ERR_ARG (status 2), not a fault.  radius <= 0 is an argument error.  n_ref, n_src < 2^31 - 64.
 * rdm_ball_fill, on the SAME workspace, ref and sizes, writes out int64 [C, 2] (capacity >= C rows) in ascending (i, j) --
 * cKDTree leaves the order inside a row open; this library defines it as ascending j.  No cap on the length of a row; no
 * float atomics: two calls give the same counts and order.  No synchronisation in rdm_ball_fill.                          */
size_t rdm_ball_workspace_bytes(int64_t n_ref, int64_t n_src);
int rdm_ball_count(const float* ref, int64_t n_ref, int64_t ld_ref, const float* src, int64_t n_src, int64_t ld_src,
                   const double* transform_host, double radius, double* ref_min_d2, uint8_t* ref_hit, uint8_t* src_hit,
                   int64_t* totals_host, void* ws, size_t ws_bytes, void* stream);
int rdm_ball_fill(const float* ref, int64_t n_ref, int64_t ld_ref, int64_t n_src, int64_t* out, int64_t capacity, void* ws,
                  size_t ws_bytes, void* stream);

/* ---- exact cloud-to-cloud nearest neighbours: chamfer, fitness, re-alignment error (nearest.hip) ---------
 * get_nearest_neighbor (geotransformer/utils/pointcloud.py:11-22, a cKDTree k = 1 query) and what registration.py builds on
 * it (compute_overlap :191-197, compute_modified_chamfer_distance :155-172).  q [n_q, >=3] / s [n_s, >=3]: device f32, row
 * strides ld_q / ld_s (xyz first); q_transform_host / s_transform_host: optional row-major float64 4x4 on the HOST, applied to
 * the respective cloud (null: the cloud as it is).  Points are read as double, x' = ((R00 x + R01 y) + R02 z) + t0,
 * d2 = ((dx dx) + (dy dy)) + (dz dz) with d = q' - s', nothing contracted.  Per query row: d2 f64 [n_q] (device, optional) =
 * the smallest d2 over ALL support rows, idx i32 [n_q] (device, optional) = the LOWEST support row that attains it (cKDTree
 * leaves equal distances open; this library defines the tie); the distance is sqrt(d2) in double.  n_s = 0: d2 = +inf and
 * idx = n_s, as cKDTree returns; n_q = 0 is valid and empty.  cell: the edge of the index's cells (<= 0: chosen on the device,
 * about 8 support points per cell); the result does not depend on it, nor on the path a row takes -- rows the cell search
 * cannot settle are swept against every support row with the same expression -- and two calls give the same bits (float64
 * sums in a fixed order, no float atomics).  totals_host (host double[5], the call's one read-back, after which the stream is
 * idle) = {sum of sqrt(d2), rows with sqrt(d2) < radius (strict, as compute_overlap; none with radius <= 0), the sum of d2
 * over those rows, rows that took the sweep, status}.  A point that is not finite, before or after moving, or a support point
 * beyond 2^30 cells of `cell` from the origin, is RDM_ERR_ARG (status 2), not a fault: nothing is indexed by such a point and
 * idx / d2 are left untouched.  n_q, n_s < 2^31 - 64.
 * rdm_realign_error: compute_registration_rmse (registration.py:136-152), *mean_host = the mean over the rows of pts [n, >=3]
 * of |gt p - est p| with the arithmetic above (NaN for n = 0); workspace rdm_nearest_workspace_bytes(0, 0).             */
size_t rdm_nearest_workspace_bytes(int64_t n_q, int64_t n_s);
int rdm_nearest(const float* q, int64_t n_q, int64_t ld_q, const float* s, int64_t n_s, int64_t ld_s,
                const double* q_transform_host, const double* s_transform_host, double cell, double radius, int32_t* idx,
                double* d2, double* totals_host, void* ws, size_t ws_bytes, void* stream);
int rdm_realign_error(const float* pts, int64_t n, int64_t ld, const double* gt_host, const double* est_host, double* mean_host,
                      void* ws, size_t ws_bytes, void* stream);

/* ---- pose information matrix of an aligned pair (nearest.hip) ---------------------------------------------------------
 * What Open3D's get_information_matrix_from_point_clouds(source, target, max_correspondence_distance, transformation) and
 * evaluate_registration compute (Open3D is not part of the reference tree -> parity unpinned; pinned to the float64
 * restatement tests/information_restatement.py).  q = source, s = target, transforms, reads and arithmetic exactly as
 * rdm_nearest (one run of its move / index / shell / sweep phases).  Source row i has a correspondence (i, j) iff its nearest
 * target row j (the lowest among equal distances) has sqrt(d2) < radius -- STRICT, the rows rdm_nearest counts in totals[1];
 * Open3D's own comparison is library-internal, this library defines it.  With p = (x, y, z) the MOVED TARGET point s'_j, the
 * matrix is the sum over the correspondences of g g^T for g = (0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1)
 * (rotation first, then translation, as Open3D), evaluated in closed form from C = sum 1 (an integer), sum p and sum p p^T:
 * rotation block tr(M) I - M, translation block C I, upper-right block [sum p]x and its transpose below.  Float64 sums in a
 * fixed order (per thread in row order, lanes by butterfly, wavefronts and block slabs in order; the launch geometry depends
 * on n_q only), no float atomics: two calls give the same bits, whatever `cell` and whatever path a row took.
 * out_host (host double[40], the call's one read-back, after which the stream is idle) = {the matrix row-major [36], C, the sum
 * of d2 over the correspondences, rows that took the sweep, status 0}.  corr_out (device, optional): int64 [C, 2] rows (i, j) in
 * ascending i -- evaluate_registration's correspondence_set --, compacted in order on the device (no atomic counter); at most
 * `capacity` rows are written, and C > capacity returns RDM_ERR_CAPACITY with out_host filled.  n_q = 0, n_s = 0 or no row
 * under the radius: the zero matrix and C = 0.  radius <= 0 is RDM_ERR_ARG; so is a point that is not finite, before or after
 * moving (or a target point beyond 2^30 cells of `cell`), with out_host and corr_out untouched.  n_q, n_s < 2^31 - 64.   */
size_t rdm_information_workspace_bytes(int64_t n_q, int64_t n_s);
int rdm_information_matrix(const float* q, int64_t n_q, int64_t ld_q, const float* s, int64_t n_s, int64_t ld_s,
                           const double* q_transform_host, const double* s_transform_host, double cell, double radius,
                           double* out_host, int64_t* corr_out, int64_t capacity, void* ws, size_t ws_bytes, void* stream);

/* ---- pose-graph optimisation (pose_graph.hip) ---------------------------------------------------------------------------
 * What Open3D's global_optimization does (Open3D is not part of the reference tree -> parity unpinned; the definition is DESIGN.md
 * section 7, pinned to the float64 restatement tests/pose_graph_restatement.py): damped Gauss-Newton on SE(3), information
 * matrices as weights, a line process for uncertain (loop-closure) edges.  A call takes n_graphs graphs, concatenated:
 * graph_node_offsets_host / graph_edge_offsets_host (host int64 [G + 1], from 0), nodes (device float64 [N, 16], row-major 4 x 4,
 * the pose of scan i in the frame of its graph's node 0, which stays fixed), edges_host (host int64 [E, 2], rows (s, t), node
 * numbers INSIDE the edge's graph), transforms (device float64 [E, 16], source-scan to target-scan coordinates: the model is
 * X_s = X_t T), informations (device float64 [E, 36], rotation first, as rdm_information_matrix), uncertain_host (host uint8 [E]
 * or null: no edge is uncertain).  line_process_weight mu <= 0: no line process (every weight is 1); else an uncertain edge's
 * weight is l = (mu / (mu + r^T L r))^2 at the current poses, and it is reported as pruned when l < edge_prune_threshold at the
 * final poses (edges are never removed).  Residual r = (Log of the rotation of E, translation of E), E = T^-1 X_t^-1 X_s; update
 * X <- X [Exp(dw) | dt]; exact Jacobians; (H + lambda blockdiag(H)) x = -b solved per graph by one workgroup with block-Jacobi
 * preconditioned conjugate gradients until sqrt(r^T M^-1 r) <= pcg_tolerance times its first value or pcg_max_iterations;
 * lambda starts at 1e-6, a step is accepted iff the new cost is <= the old one (lambda / 10, at least 1e-12), else rejected
 * (lambda * 10; above 1e12 the solve ends with stop reason 2).  Stops: 1 = the largest |entry| of the gradient of F (2 J^T L r) is
 * <= gradient_tolerance, 2 = the relative decrease of an accepted step is <= cost_tolerance, 3 = max_iterations (accepted and
 * rejected steps count), 4 = a graph without nodes or without edges (returned as given).  Float64, no float atomics, every sum
 * in an order the graph alone decides: a graph's outputs are the same bits alone, in any batch, at any position, in any run.
 * Outputs (device): nodes_out [N, 16] (may be `nodes`), weights_out [E] (optional: l at the final poses), pruned_out uint8 [E]
 * (optional); report_host (host double [G, 8], the call's one read-back of results): {initial cost, final cost, iterations, PCG
 * iterations in total, stop reason, status, final lambda, largest gradient entry at the last linearisation}.  RDM_ERR_ARG, with
 * every device output untouched: an edge that joins a node to itself or names a node outside its graph, a graph above 65 536
 * nodes or 1 048 576 edges, (status 1) an entry that is not finite, (2) an information matrix with |L_ij - L_ji| > 1e-12 max|L|,
 * (3) a residual rotation of the GIVEN poses with cos(angle) < -0.99 (during the solve such a candidate is a rejected step),
 * (4) a node block that is not positive definite (a node no edge reaches, an indefinite information matrix); the message names
 * the first graph whose status is not 0.  The host reads one word every 8 iterations.  The per-graph limits are nominal: the
 * block-Jacobi conjugate gradients need on the order of 10^4 iterations per step at 500 nodes (docs/EXPERIMENTS.md 5n), all inside one
 * launch of one workgroup; with block-Jacobi choose pcg_max_iterations accordingly for graphs beyond a few thousand nodes, or
 * select the chain preconditioner below (7 to 17 times fewer iterations on drives with loop closures, each about 4 times as
 * long at 500 nodes: 5o).
 * The _pc forms take `preconditioner`: 0 block-Jacobi (what the plain forms forward, bit for bit), 1 the odometry chain, anything
 * else RDM_ERR_ARG.  The chain preconditioner M is block tridiagonal over the free nodes 1 .. n - 1: diagonal blocks
 * (1 + lambda) D_i (D_i the node block from all incident edges), block (i, i + 1) the sum of l A^T L B over the edges that join
 * nodes i and i + 1 in ascending edge order (as is when the edge's source is i, transposed when it is i + 1); every other edge
 * contributes to the diagonal only, so a graph without such pairs gets block-Jacobi again.  M is factored once per linearisation
 * by a block Cholesky along the chain (a pivot that is not positive: status 4) and applied once per PCG iteration by two sweeps
 * of one wavefront; the determinism guarantee above holds.  Only preconditioner 1 enlarges the workspace (36 doubles per node).
 * Graphs whose system is far from its chain (a hub) gain nothing; the solution is the same within the tolerances.            */
size_t rdm_pose_graph_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int64_t n_edges);
size_t rdm_pose_graph_workspace_bytes_pc(int64_t n_graphs, int64_t n_nodes, int64_t n_edges, int preconditioner);
int rdm_pose_graph_optimize_pc(int64_t n_graphs, const int64_t* graph_node_offsets_host, const int64_t* graph_edge_offsets_host,
                               const double* nodes, const int64_t* edges_host, const double* transforms, const double* informations,
                               const uint8_t* uncertain_host, double line_process_weight, double edge_prune_threshold,
                               int max_iterations, double gradient_tolerance, double cost_tolerance, int pcg_max_iterations,
                               double pcg_tolerance, int preconditioner, double* nodes_out, double* weights_out,
                               uint8_t* pruned_out, double* report_host, void* ws, size_t ws_bytes, void* stream);
int rdm_pose_graph_optimize(int64_t n_graphs, const int64_t* graph_node_offsets_host, const int64_t* graph_edge_offsets_host,
                            const double* nodes, const int64_t* edges_host, const double* transforms, const double* informations,
                            const uint8_t* uncertain_host, double line_process_weight, double edge_prune_threshold,
                            int max_iterations, double gradient_tolerance, double cost_tolerance, int pcg_max_iterations,
                            double pcg_tolerance, double* nodes_out, double* weights_out, uint8_t* pruned_out, double* report_host,
                            void* ws, size_t ws_bytes, void* stream);
/* The kernels' per-edge arithmetic compiled for the host (all pointers host memory; no GPU needed), so that it can be held
 * against the restatement without a device: out (double[128]) = {l, cost term, r [6], l A^T L A [36], l A^T L B [36],
 * l B^T L B [36], l A^T L r [6], l B^T L r [6]} for one edge (A, B: the Jacobians of r with respect to the source's and the
 * target's perturbation); RDM_ERR_ARG beyond the angle limit (r is still written).  And X [Exp(dw) | dt] -> out (double[16]). */
int rdm_pose_graph_edge_terms_host(const double* source_pose, const double* target_pose, const double* transform,
                                   const double* information, double line_process_weight, int uncertain, double* out);
int rdm_pose_graph_retract_host(const double* pose, const double* delta, double* out);
/* The chain preconditioner's factor and apply functions, as the kernels run them, on the host (all pointers host memory): solves
 * M out = rhs for the block tridiagonal M with diagonal blocks diag [n, 36] (row-major 6 x 6, the lower triangle is read) and
 * blocks (i, i + 1) off [n - 1, 36]; rhs and out [n, 6].  RDM_ERR_ARG for a pivot that is not positive.                      */
int rdm_pose_graph_chain_host(int64_t n, const double* diag, const double* off, const double* rhs, double* out);
/* The _ls forms take `linear_solver` after `preconditioner`: 0 conjugate gradients with that preconditioner (what the _pc forms
 * forward, bit for bit), 1 the direct sparse solve (then `preconditioner`, pcg_max_iterations and pcg_tolerance are ignored and
 * report entry 3 is 0), anything else RDM_ERR_ARG.  The direct solve suits a chain with loop closures: an
 * edge is off-chain when both ends are free and more than one node apart (several between the same two nodes count once); the
 * separator S is a vertex cover of the off-chain pairs chosen by one rule -- repeatedly the node with the most uncovered pairs,
 * the lowest number among equals -- and kept ascending; the free nodes outside S fall into runs of consecutive numbers, block
 * tridiagonal and uncoupled.  With A_II = L L^T along the runs: Y = L^-1 A_IS (a column block is stored from its first coupling
 * position to its run's end), C = A_SS - Y^T Y = L_S L_S^T dense in 6 x 6 blocks, y = L^-1 r_I, x_S = C^-1 (r_S - Y^T y),
 * x_I = L^-T (y - Y x_S).  A pivot that is not positive, in a run or in C, is status 4.  Every sum runs in an order the graph
 * alone decides (ascending edge, node, separator index, block column), so the determinism guarantee holds.  A graph may have at
 * most rdm_pose_graph_direct_max_separator() (256) separator nodes; above it the call is RDM_ERR_ARG, the message names the
 * graph, the count and the limit, every output is untouched, and nothing falls back to conjugate gradients.  The direct solve's
 * workspace depends on the structure (the separator sizes squared and the stored part of Y), so
 * rdm_pose_graph_workspace_bytes_ls reads the edges and returns the exact size; 0 with rdm_last_error set for a graph above the
 * limit or bad arguments; with linear_solver 0 what rdm_pose_graph_workspace_bytes_pc returns.                                  */
size_t rdm_pose_graph_workspace_bytes_ls(int64_t n_graphs, const int64_t* graph_node_offsets_host,
                                         const int64_t* graph_edge_offsets_host, const int64_t* edges_host, int preconditioner,
                                         int linear_solver);
int rdm_pose_graph_optimize_ls(int64_t n_graphs, const int64_t* graph_node_offsets_host, const int64_t* graph_edge_offsets_host,
                               const double* nodes, const int64_t* edges_host, const double* transforms, const double* informations,
                               const uint8_t* uncertain_host, double line_process_weight, double edge_prune_threshold,
                               int max_iterations, double gradient_tolerance, double cost_tolerance, int pcg_max_iterations,
                               double pcg_tolerance, int preconditioner, int linear_solver, double* nodes_out, double* weights_out,
                               uint8_t* pruned_out, double* report_host, void* ws, size_t ws_bytes, void* stream);
int rdm_pose_graph_direct_max_separator(void);
/* |S| of one graph under the rule above (host only); the nodes go to out_nodes in ascending order, never past `capacity`
 * (out_nodes may be null with capacity 0).  -1 for an edge outside the graph or a self edge.                                  */
int64_t rdm_pose_graph_separator_host(int64_t n_nodes, int64_t n_edges, const int64_t* edges_host, int64_t* out_nodes,
                                      int64_t capacity);
/* The direct solve's factor, border, Schur and solve functions, as the kernels run them and in their order, on the host (all
 * pointers host memory): solves the system with diagonal block i = diag[i] ([n_nodes, 36], the lower triangle is read) and, per
 * edge e = (s, t), off[e] ([n_edges, 36]) added to block (s, t) with its rows belonging to s, its transpose to (t, s); rhs and
 * out [n_nodes, 6].  Row 0 and edges that touch node 0 are ignored and out[0] = 0.  RDM_ERR_ARG ("not positive") for a failed
 * pivot and for a separator above the limit.                                                                                   */
int rdm_pose_graph_direct_host(int64_t n_nodes, int64_t n_edges, const int64_t* edges_host, const double* diag, const double* off,
                               const double* rhs, double* out);
/* Marginal covariances of a batch of graphs in rdm_pose_graph_optimize's layout: per graph, with
 * H = sum_e w_e J_e^T L_e J_e over the free nodes 1 .. n - 1 -- the undamped Gauss-Newton matrix at `nodes` (normally the optimiser's
 * output), linearised as the optimiser linearises, `weights` (device [E], >= 0; null: all 1 -- the optimiser's weights_out fits) in
 * the line process's place -- covariances_out (device [N, 36], float64) row i is (H^-1)_ii: the covariance of node i's right
 * perturbation X_i [Exp(dw) | dt], rotation first, conditioned on node 0, whose row is zero.  The factor is H^-1, not (2 H)^-1: the
 * information matrices are inverse covariances of the residuals.  Every block is written exactly symmetric (an entry above the
 * diagonal is a copy of the one below).  The blocks come from the direct solve's factors at lambda = 0 by a selected inversion --
 * Sigma_SS = C^-1 on the separator and one backward recurrence per run -- so the separator limit above holds here too and nothing
 * dense of size N is formed; no float atomics and every sum in an order the graph alone decides: a graph's rows are the same bits
 * alone, anywhere in a batch and from run to run.  report_host [G, 2]: status (0, or 4: a pivot of a run or of the Schur complement
 * is not positive -- zero weights that cut a node off, an indefinite information matrix, a graph of several nodes without edges;
 * that graph's rows but row 0 are NaN, the call is still RDM_OK and the other graphs are unaffected) and the separator's size.
 * RDM_ERR_ARG with every output untouched for what rdm_pose_graph_optimize refuses (non-finite entries, asymmetric information, an
 * angle beyond the limit, a self edge, an edge outside its graph, the size limits), for a negative or non-finite weight and for a
 * graph above the separator limit (the message names the graph, the count and the limit).  The workspace size is exact and reads
 * the edges; 0 with rdm_last_error set for a graph above the limit or bad arguments.                                             */
size_t rdm_pose_graph_marginals_workspace_bytes(int64_t n_graphs, const int64_t* graph_node_offsets_host,
                                                const int64_t* graph_edge_offsets_host, const int64_t* edges_host);
int rdm_pose_graph_marginals(int64_t n_graphs, const int64_t* graph_node_offsets_host, const int64_t* graph_edge_offsets_host,
                             const double* nodes, const int64_t* edges_host, const double* transforms, const double* informations,
                             const double* weights, double* covariances_out, double* report_host, void* ws, size_t ws_bytes,
                             void* stream);
/* The same functions as the kernels run them and in their order, on the host, on a system given as rdm_pose_graph_direct_host
 * takes it (diag, off; all pointers host memory): out [n_nodes, 36], row 0 zero.  RDM_ERR_ARG ("not positive") for a failed pivot and
 * for a separator above the limit.                                                                                              */
int rdm_pose_graph_marginals_host(int64_t n_nodes, int64_t n_edges, const int64_t* edges_host, const double* diag, const double* off,
                                  double* out);
/* Cross covariances and the consistency of candidate (loop) edges with a graph (g2o's computeMarginals with
 * block pairs, GTSAM's jointMarginalCovariance): the marginals call above, with the same arguments and the same kernels in the same
 * order -- covariances_out is bit for bit what rdm_pose_graph_marginals writes --, and then, for a list of P pairs in the edges' layout
 * (pairs_host int64 [P, 2] rows (s, t) numbered inside their graph, graph_pair_offsets_host int64 [G + 1]; pair_transforms device
 * [P, 16] with an edge's convention X_s = X_t T; pair_informations device [P, 36] or null for the whole call), per pair:
 *   cross_out [P, 36]         Sigma_st = (H^-1)_st, rows belonging to s; zero when s or t is node 0
 *   residual_cov_out [P, 36]  M = A Sigma_ss A^T + A Sigma_st B^T + B Sigma_ts A^T + B Sigma_tt B^T with the Jacobians A, B of the
 *                             residual r of (X_s, X_t, T) as an edge's are formed: the covariance of that residual under the graph (at
 *                             T = X_t^-1 X_s: of the relative pose); exactly symmetric
 *   d2_out [P]                r^T (M + L^-1)^-1 r (without informations r^T M^-1 r) by a 6 x 6 Cholesky
 *   pair_status_out [P]       uint8: 0, or 1: L or M + L^-1 is not positive definite -- d2 is NaN, the blocks are written
 * Every output pointer may be null.  The six columns of H^-1 of a pair's column node t are solved for from the factors the marginals
 * leave (forwards along t's run, through Sigma_SS, backwards along s's run), a thread per scalar column, kColumnsInFlight = 128 column
 * nodes at a time on the stream; nothing of size N x N or N x P is formed, no float atomics, and every sum in an order the graph and
 * the pair decide: a pair's rows are the same bits alone, with any other pairs, anywhere in a batch and from run to run.  report_host
 * [G, 2] as above; a graph with status 4 has NaN in its pairs' rows (pair status 0).  RDM_ERR_ARG with every output untouched, the
 * message naming the first offender: whatever the marginals call refuses, a pair with s = t or outside its graph, a non-finite pair
 * transform or information, an asymmetric information (the edges' rule), a pair residual beyond the angle limit.  The workspace size
 * is exact and reads edges and pairs: the marginals' plus O(P) and 128 x (the longest forward pass + the largest separator) blocks;
 * 0 with rdm_last_error set for what the host can refuse.                                                                          */
size_t rdm_pose_graph_consistency_workspace_bytes(int64_t n_graphs, const int64_t* graph_node_offsets_host,
                                                  const int64_t* graph_edge_offsets_host, const int64_t* edges_host,
                                                  const int64_t* graph_pair_offsets_host, const int64_t* pairs_host);
int rdm_pose_graph_consistency(int64_t n_graphs, const int64_t* graph_node_offsets_host, const int64_t* graph_edge_offsets_host,
                               const double* nodes, const int64_t* edges_host, const double* transforms, const double* informations,
                               const double* weights, const int64_t* graph_pair_offsets_host, const int64_t* pairs_host,
                               const double* pair_transforms, const double* pair_informations, double* covariances_out,
                               double* cross_out, double* residual_cov_out, double* d2_out, uint8_t* pair_status_out,
                               double* report_host, void* ws, size_t ws_bytes, void* stream);
/* The pairs' work items as the kernels run them and in their order, on the host, on a system given as rdm_pose_graph_marginals_host
 * takes it: out [n_pairs, 36] is Sigma_st of pairs_host's rows (s, t).  RDM_ERR_ARG as there, and for a pair with s = t or outside
 * the graph.                                                                                                                      */
int rdm_pose_graph_pair_covariances_host(int64_t n_nodes, int64_t n_edges, const int64_t* edges_host, const double* diag,
                                         const double* off, int64_t n_pairs, const int64_t* pairs_host, double* out);
/* One pair as the pair kernel's thread computes it (host pointers): poses and transform [16], information [36] or null, Sigma_ss and
 * Sigma_tt (their lower triangles are read) and Sigma_st [36] -> out [44]: r [6], M [36], d2, status (0 or 1).  RDM_ERR_ARG beyond
 * the angle limit.                                                                                                                */
int rdm_pose_graph_pair_terms_host(const double* source_pose, const double* target_pose, const double* transform,
                                   const double* information, const double* cov_ss, const double* cov_tt, const double* cov_st,
                                   double* out);
/* Measurement hook (tools/pose_graph_bench.py --marginals): with a device buffer of 3 long long per run of the next calls of this
 * thread, the run sweep's lane 0 stores the 100 MHz clock ticks it spent in the columns' products, the butterflies and the nodes'
 * steps; null (the default) turns it off.                                                                                       */
int rdm_dbg_pose_graph_marginals_ticks(long long* device_ticks);

/* ---- dense contraction ---------------------------------------------------------------------
 * C[b] = act((A[b] (m x k) * op(B[b])) / rowdiv[row] + bias[col]) in fp32 on the f32 MFMA.
 * trans_b = 0: B is [k, n] row-major (pre-transposed nn.Linear weights, KPConv weights viewed
 * [15*C_in, C_out]); trans_b = 1: B is [n, k] row-major.  act: 0 none, 1 ReLU, 2 LeakyReLU(0.1).
 * Replaces torch.nn.Linear / torch.matmul / torch.einsum call sites of the path, e.g.
 * geotransformer/modules/kpconv/kpconv.py:107-110, modules/kpconv/modules.py:77,
 * experiments/model_infer.py:310-311.  k, lda, ldb must be multiples of 4 (zero padded), A and B
 * 16-byte aligned.  ws (rdm_gemm_workspace_bytes) enables deterministic split-K; may be NULL.   */
size_t rdm_gemm_workspace_bytes(int64_t m, int64_t n, int batches);
int rdm_gemm(const float* a, int64_t lda, int64_t stride_a, const float* b, int64_t ldb,
             int64_t stride_b, int trans_b, float* c, int64_t ldc, int64_t stride_c, int64_t m,
             int64_t n, int64_t k, int batches, const float* bias, const float* rowdiv, int act,
             void* ws, size_t ws_bytes, void* stream);
/* The tile and split-K factor the dispatch model chose for the calling thread's last rdm_gemm / fused Linear call:
 * out4_host = {tile rows, tile columns, k-tile depth, split-K factor} (diagnostic: profiles/r03_gemm_shapes.md).  */
int rdm_gemm_last_plan(int* out4_host);

/* ---- a4: KPConv neighbourhood aggregation ---------------------------------------------------
 * Replaces the gather half of KPConv.forward (geotransformer/modules/kpconv/kpconv.py:91-105,
 * 113-115): wf[m, k*c + ch] = sum_h max(0, 1 - |s[idx[m,h]] - q[m] - kp[k]| / sigma) * feats[idx[m,h], ch]
 * and nn[m] = max(1, #neighbours whose feature row sums to > 0) (as float).  Pad indices (>= n_s)
 * are the reference's shadow point/zero row.  s_positive[i] = (sum_c feats[i,c] > 0), see
 * rdm_row_positive / rdm_group_norm.  width (optional device int32) caps the row width like the
 * reference's `[:, :min(limit, max_count)]`.  c = 1 or any multiple of 32; any h (rows wider than the 128 slots a wavefront stages in LDS run in chunks).
 * The second half of the convolution is rdm_gemm(wf, W[15*c, c'], rowdiv = nn, bias).          */
int rdm_kpconv_gather(const float* q_points, int64_t m, const float* s_points, int64_t n_s,
                      const float* s_feats, int64_t c, int64_t ldf, const uint8_t* s_positive,
                      const int64_t* idx, int64_t h, int64_t ldi, const int32_t* width,
                      const float* kernel_points, float sigma, float* wf, int64_t ldw, float* nn,
                      void* stream);
/* rdm_kpconv_fused: the WHOLE KPConv.forward (kpconv.py:79-122) in one kernel for the fine levels -- c_in = 1 (c_out
 * 64), 32 -> 32, 64 -> 64: out[m, c'] = (sum_k sum_c wf[m, k, c] W[k, c, c']) / nn[m] + bias[c'] with wf and nn as in
 * rdm_kpconv_gather; the [m, 15*c] intermediate stays in LDS.  w_packed: W [15, c_in, c_out] reordered by
 * rdm_kpconv_pack_weights (host arrays; rdm_kpconv_packed_floats floats).  gn_partial (optional): fp64 column sums /
 * sums of squares of the output, one partial row per workgroup: [rdm_kpconv_fused_partial_rows(m, c_in)][2][c_out] -- the
 * input of the GroupNorm that follows every KPConv.  rdm_kpconv_fused_group_norm = that convolution +
 * act(GroupNorm(.)) (modules.py:141-145, 205-207), workspace rdm_kpconv_fused_workspace_bytes.
 * order_records (optional, round 4): m x float4 {x, y, z, query row} in the cell order of the query level's search grid
 * (rdm_radius_grid_records).  For h <= 128 and c_in = 32, or c_in = 64 with queries and support on the same level (2 m > n_s),
 * a workgroup then takes 16 queries that are neighbours in space, stages the union of their support rows (feature row,
 * point, positive flag) ONCE in LDS and aggregates from there ("LDS-staged neighbour tiles"); null = the queries in row order
 * (spatially random for a level of the pyramid: nothing to share, the lock-step kernel runs).  The convolution
 * output does not depend on the order; the GroupNorm partials group the rows by workgroup, i.e. by that order.      */
int rdm_kpconv_fused_enabled(void);   /* 1 iff RDM_FUSED_KPCONV is set: engine and per-op path then use the fused kernel */
int rdm_kpconv_fused_supported(int64_t c_in, int64_t c_out);
int64_t rdm_kpconv_fused_partial_rows(int64_t m, int64_t c_in);
size_t rdm_kpconv_packed_floats(int64_t c_in, int64_t c_out);
int rdm_kpconv_pack_weights(const float* w_host, int64_t c_in, int64_t c_out, float* packed_host);
int rdm_kpconv_fused(const float* q_points, int64_t m, const float* s_points, int64_t n_s, const float* s_feats,
                     int64_t c, int64_t ldf, const uint8_t* s_positive, const int64_t* idx, int64_t h, int64_t ldi,
                     const int32_t* width, const float* kernel_points, float sigma, const float* w_packed,
                     const float* bias, int64_t c_out, float* out, int64_t ldo, double* gn_partial,
                     const float* order_records, void* stream);
/* The same with the kernel chosen by the caller (tests and A/B runs): form 0 = the library's choice (rdm_kpconv_fused), 1 = the
 * lock-step kernel (every (query, neighbour) row fetched from L2), 2 = the LDS-tile kernel where it applies (c_in = 32 / 64,
 * h <= 128).  Both give the same convolution output bit for bit and one partial row per 16 queries (form 2 groups the
 * queries of a row by `order_records`).                                                                              */
int rdm_kpconv_fused_form(const float* q_points, int64_t m, const float* s_points, int64_t n_s, const float* s_feats,
                          int64_t c, int64_t ldf, const uint8_t* s_positive, const int64_t* idx, int64_t h, int64_t ldi,
                          const int32_t* width, const float* kernel_points, float sigma, const float* w_packed,
                          const float* bias, int64_t c_out, float* out, int64_t ldo, double* gn_partial,
                          const float* order_records, int form, void* stream);
size_t rdm_kpconv_fused_workspace_bytes(int64_t m, int64_t c_in, int64_t c_out);
int rdm_kpconv_fused_group_norm(const float* q_points, int64_t m, const float* s_points, int64_t n_s,
                                const float* s_feats, int64_t c, int64_t ldf, const uint8_t* s_positive,
                                const int64_t* idx, int64_t h, int64_t ldi, const int32_t* width,
                                const float* kernel_points, float sigma, const float* w_packed, const float* bias,
                                int64_t c_out, int groups, const float* gamma, const float* beta, float eps, int act,
                                float* conv_out, int64_t ld_conv, float* y, int64_t ldy, void* ws, size_t ws_bytes,
                                const float* order_records, void* stream);
/* Same as rdm_kpconv_gather, visiting the queries in the order given by `order_records` (m x float4 whose 4th component
 * holds the query row, e.g. rdm_radius_grid_records of the query level): neighbouring queries share
 * most of their neighbours, so the gathered lines are re-used from the CU's L1.  Results are identical. */
int rdm_kpconv_gather_ordered(const float* q_points, int64_t m, const float* s_points, int64_t n_s,
                              const float* s_feats, int64_t c, int64_t ldf, const uint8_t* s_positive,
                              const int64_t* idx, int64_t h, int64_t ldi, const int32_t* width,
                              const float* kernel_points, float sigma, float* wf, int64_t ldw, float* nn,
                              const float* order_records, void* stream);
/* The same with the kernel form chosen by the caller (tests and A/B runs): 0 = the library's choice, 1 = one wavefront per
 * (query, 64-channel slice) fetching every neighbour row, 2 = the support rows of 16 cell-ordered queries staged once in LDS
 * (needs order_records, c a multiple of 64 >= 128, h <= 128; else form 1).  Same WF and nn bits in every form.            */
int rdm_kpconv_gather_form(const float* q_points, int64_t m, const float* s_points, int64_t n_s,
                              const float* s_feats, int64_t c, int64_t ldf, const uint8_t* s_positive,
                              const int64_t* idx, int64_t h, int64_t ldi, const int32_t* width,
                              const float* kernel_points, float sigma, float* wf, int64_t ldw, float* nn,
                              const float* order_records, int form, void* stream);
int rdm_row_positive(const float* x, int64_t n, int64_t c, int64_t ld, uint8_t* out, void* stream);

/* ---- a5: block glue --------------------------------------------------------------------------
 * rdm_group_norm: y = act(GroupNorm(x) [+ residual]) with statistics over ALL n rows
 *   (geotransformer/modules/kpconv/modules.py:33-50, 53-83, 204-225); optionally also writes the
 *   positive-row flag of y.  rdm_layer_norm: y = act(LayerNorm(x [+ residual]))
 *   (torch.nn.LayerNorm call sites: modules/transformer/vanilla_transformer.py:79,101, output_layer.py:13,20, rdmnet/vote/vote.py:58-77).
 * rdm_gather_max: modules/kpconv/functional.py:54-67.  rdm_upsample_concat: functional.py:6-22 +
 *   the torch.cat of experiments/backbone.py:131-143; pad columns of y are zeroed.              */
size_t rdm_group_norm_workspace_bytes(int64_t n, int64_t c);
int rdm_group_norm(const float* x, int64_t n, int64_t c, int64_t ldx, int groups, const float* gamma,
                   const float* beta, float eps, const float* residual, int64_t ldr, int act, float* y,
                   int64_t ldy, uint8_t* positive, void* ws, size_t ws_bytes, void* stream);
/* The same with the launch structure chosen by the caller (tests, A/B runs): form 0 = the library's choice -- up to 4 096 rows with
 * whole 64-column slabs, finalize and apply are ONE launch (every workgroup recomputes the scale / shift of its slab from the few
 * dozen partial rows: one dependent launch less on a pair's critical path, same bits) --, form 1 = statistics, finalize and apply
 * as separate launches everywhere.  Applies to this call only.                                                                 */
int rdm_group_norm_form(const float* x, int64_t n, int64_t c, int64_t ldx, int groups, const float* gamma,
                        const float* beta, float eps, const float* residual, int64_t ldr, int act, float* y, int64_t ldy,
                        uint8_t* positive, void* ws, size_t ws_bytes, int form, void* stream);
/* rdm_linear_group_norm: y = act(GroupNorm(x W + bias [/ rowdiv]) [+ residual]) -- UnaryBlock / the
 * KPConv weight contraction + norm_conv (modules/kpconv/modules.py:53-83, 196-207): the GEMM epilogue
 * emits the GroupNorm statistics, saving a pass over the activations.  lin_out [m, n] is scratch for
 * the pre-norm activations.  Same operand rules as rdm_gemm (trans_b = 0).                       */
size_t rdm_linear_group_norm_workspace_bytes(int64_t m, int64_t n);
int rdm_linear_group_norm(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias,
                          const float* rowdiv, int64_t m, int64_t n, int64_t k, int groups, const float* gamma,
                          const float* beta, float eps, const float* residual, int64_t ldr, int act, float* lin_out,
                          int64_t ld_lin, float* y, int64_t ldy, uint8_t* positive, void* ws, size_t ws_bytes,
                          void* stream);
/* rdm_patch_scores: the patch score matrices of the fine matching (experiments/model_infer.py:291-311: index_select of the
 * patch features + einsum('bnd,bmd->bnm') / sqrt(d)): scores[b, i, j] = <ref_feats[ref_idx[b, i]], src_feats[src_idx[b, j]]>
 * / rowdiv[i], ref_idx / src_idx [batch, side] int64 with the reference's padded gather (an index outside the tensor selects a
 * zero row).  scores [batch, side, side] contiguous.  The gathered [batch, side, d] tensors are never materialised. */
int rdm_patch_scores(const float* ref_feats, int64_t ld_ref, int64_t n_ref, const int64_t* ref_idx, const float* src_feats,
                     int64_t ld_src, int64_t n_src, const int64_t* src_idx, int64_t batch, int64_t side, int64_t d,
                     const float* rowdiv, float* scores, void* stream);
/* rdm_decoder_stage: one stage of the decoder (experiments/backbone.py:118-151; nearest_upsample =
 * geotransformer/modules/kpconv/functional.py:6-22, UnaryBlock / LastUnaryBlock = modules.py:53-101):
 *   y = act(GroupNorm([coarse[idx[:, 0]] | skip] W + bias))        gamma != NULL (lin_out: scratch for the pre-norm rows)
 *   lin_out = [coarse[idx[:, 0]] | skip] W + bias                  gamma == NULL
 * idx [m, ldi] is the upsampling table (column 0 used; an index outside [0, n_coarse) gives a zero row); W [pad4(c1+c2), n pad]
 * as rdm_gemm's B.  Three routes, chosen from the sizes alone:
 *   - c1 no multiple of 32 (or c1 + c2 no multiple of 4): the rows are concatenated into the workspace, then the plain product;
 *   - else, when the product runs un-split (rdm_gemm_last_plan) and n_coarse < m: coarse W[0:c1] is formed once per COARSE row
 *     (into the same workspace region) and the product of skip with W[c1:] starts its accumulators from that row of it;
 *   - else the concatenated rows exist only inside the GEMM's operand tiles.
 * An output element is one fp32 fma chain over ascending k from +0 on every route, and after its first c1 steps that chain holds
 * coarse[idx[m]] W[0:c1, n] whichever fine row m runs it: for one tile shape and split-K factor the routes return the same bits. */
size_t rdm_decoder_stage_workspace_bytes(int64_t m, int64_t n, int64_t k);
int rdm_decoder_stage(const float* coarse, int64_t n_coarse, int64_t c1, int64_t ld1, const int64_t* idx, int64_t ldi,
                      const float* skip, int64_t c2, int64_t ld2, int64_t m, const float* w, int64_t ldw, const float* bias,
                      int64_t n, int groups, const float* gamma, const float* beta, float eps, int act, float* lin_out,
                      int64_t ld_lin, float* y, int64_t ldy, void* ws, size_t ws_bytes, void* stream);
int rdm_layer_norm(const float* x, int64_t n, int64_t c, int64_t ldx, const float* residual,
                   int64_t ldr, const float* gamma, const float* beta, float eps, int act, float* y,
                   int64_t ldy, void* stream);
/* rdm_linear_layer_norm: y = act(LayerNorm(x W + bias [+ residual])) in one launch for the transformer width
 * (n = 128, k % 16 == 0, W [128, k] = the nn.Linear weight as stored, row stride ldw >= k): the Linear + residual
 * LayerNorm pairs of the attention layers
 * (rdmnet/thdroformer/thdroformer.py:159-173, modules/transformer/vanilla_transformer.py:87-103, output_layer.py:13-21). */
int rdm_linear_layer_norm(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, int64_t m, int64_t n,
                          int64_t k, const float* residual, int64_t ldr, const float* gamma, const float* beta, float eps,
                          int act, float* y, int64_t ldy, void* stream);
/* rdm_attention_tail: everything of an attention layer after softmax(QK^T)V in one launch:
 *   y = LayerNorm(hidden Wo^T + bo + x); z = relu(y W1^T + b1); out = LayerNorm(z W2^T + b2 + y)
 * (rdmnet/thdroformer/thdroformer.py:142-173 RPEAttentionLayer / :159-173, geotransformer/modules/transformer/
 * vanilla_transformer.py:69-103, output_layer.py:6-21 AttentionOutput).  d = 128 with a 256-wide FFN; weights as
 * nn.Linear stores them: wo [128,128], w1 [256,128], w2 [128,256], row strides ld_* (multiples of 4), 16-byte aligned.
 * hidden, x, out: [m, 128] rows.  Other widths: rdm_linear_layer_norm / rdm_gemm + rdm_layer_norm.                  */
int rdm_attention_tail(const float* hidden, int64_t ld_hidden, const float* x, int64_t ldx, int64_t m, int64_t d,
                       const float* wo, int64_t ld_wo, const float* bo, const float* gamma1, const float* beta1,
                       const float* w1, int64_t ld_w1, const float* b1, const float* w2, int64_t ld_w2, const float* b2,
                       const float* gamma2, const float* beta2, float eps, float* out, int64_t ld_out, void* stream);
/* The same on weights stored once in OPERAND order (round 6): rdm_attention_tail_pack_weights writes wo | w1 | w2 as float4
 * [(wavefront, step), lane] into `packed` (rdm_attention_tail_packed_floats() floats, 16-byte aligned), so that every weight load
 * instruction of the kernel reads one contiguous KB instead of 16 rows x 64 B (28 k -> 19.5 k clocks per workgroup: the kernel
 * is bound by the CU's L2 fill path).  Same values in the same lanes: the bits of rdm_attention_tail.                        */
size_t rdm_attention_tail_packed_floats(void);
int rdm_attention_tail_pack_weights(const float* wo, int64_t ld_wo, const float* w1, int64_t ld_w1, const float* w2, int64_t ld_w2,
                                    float* packed, void* stream);
int rdm_attention_tail_packed(const float* hidden, int64_t ld_hidden, const float* x, int64_t ldx, int64_t m, int64_t d,
                              const float* packed, const float* bo, const float* gamma1, const float* beta1, const float* b1,
                              const float* b2, const float* gamma2, const float* beta2, float eps, float* out, int64_t ld_out,
                              void* stream);
int rdm_gather_max(const float* x, int64_t n_s, int64_t c, int64_t ldx, const int64_t* idx, int64_t m,
                   int64_t h, int64_t ldi, const int32_t* width, float* y, int64_t ldy, void* stream);
/* rdm_gather_rows: y[i,:] = x[idx[i],:] on raw 32-bit words, out-of-range index -> zero row (the
 * padded index_select of geotransformer/modules/ops/index_select.py:4-31 and boolean-mask selects). */
int rdm_gather_rows(const void* x, int64_t n_src, int64_t words, int64_t ldx, const int64_t* idx, int64_t m,
                    void* y, int64_t ldy, void* stream);
int rdm_upsample_concat(const float* coarse, int64_t n_coarse, int64_t c1, int64_t ld1,
                        const int64_t* idx, int64_t ldi, const float* skip, int64_t c2, int64_t ld2,
                        int64_t m, float* y, int64_t ldy, void* stream);

/* ---- a7: 3DRoFormer attention ------------------------------------------------------------------
 * rdm_rope: in-place learned rotary embedding of q (and k when non-NULL): pair p of row r is rotated
 *   by theta = 2*pi*sigmoid(emb[r, p]) (rdmnet/thdroformer/thdroformer.py:56-85; emb has d_model/2
 *   columns = heads x 16).
 * rdm_attention: out = softmax(q k^T / sqrt(head_dim)) v per head, heads packed along the columns
 *   (thdroformer.py:20-40 with k=None, :112-139; geotransformer/modules/transformer/
 *   vanilla_transformer.py:51-66).  head_dim must be 32.                                        */
int rdm_rope(float* q, int64_t ldq, float* k, int64_t ldk, const float* emb, int64_t lde, int64_t n,
             int64_t d_model, void* stream);
int rdm_attention(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                  float* out, int64_t ldo, int64_t n_q, int64_t n_k, int heads, int head_dim, void* stream);
/* Same with Q, K, V and the probabilities rounded to bf16 for the two contractions (bf16 MFMA); logits,
 * softmax and accumulation in fp32 (BASELINE.json configs[3]: "bf16 attention + fp32 SVD").  Tensors in HBM
 * stay fp32. */
int rdm_attention_bf16(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                  float* out, int64_t ldo, int64_t n_q, int64_t n_k, int heads, int head_dim, void* stream);
/* rdm_attention_self_pair: the self-attention of both stacked clouds in one launch -- rows [0, n0) attend to rows
 * [0, n0), rows [n0, n0 + n1) to rows [n0, n0 + n1) (rdmnet/thdroformer/thdroformer.py:225-236 applies the self layer to
 * ref and src separately); bf16 != 0 selects the bf16-operand variant.  Same results as two rdm_attention calls.   */
int rdm_attention_self_pair(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                            float* out, int64_t ldo, int64_t n0, int64_t n1, int heads, int head_dim, int bf16,
                            void* stream);
/* rdm_attention_topk: the top-k ("dynamic") attention of the second 3DRoFormer's self layers (cfg.thdroformer.k2;
 *   rdmnet/thdroformer/thdroformer.py:20-40 with k != None): each query row keeps its `keep` (0 <= keep <= n_k) largest scores
 *   q k^T / sqrt(head_dim) -- the same fp32 scores rdm_attention forms -- and out = softmax over the kept scores times their
 *   v rows; the other keys get probability 0.  keep = 0 gives zero rows.  Ties: among keys whose score equals the keep-th
 *   largest (-0 equal to +0), the lowest key indices are kept (torch.topk leaves the choice unspecified).  Any n_k (rows of
 *   up to 2048 keys keep their scores in LDS, longer rows form them again per pass); n_q = 0 and n_k = 0 are valid.
 *   Arguments as rdm_attention.
 * rdm_attention_self_pair_topk: both stacked clouds in one launch, as rdm_attention_self_pair, cloud 0 keeping keep0 of its
 *   n0 keys and cloud 1 keep1 of its n1; the bits of two rdm_attention_topk calls.
 * rdm_topk_count: the kept count int(n * frac) of the reference -- the IEEE double product truncated (int(100 * 0.57) is 56).
 *   Host only; the single definition the engine uses.                                                                      */
int rdm_attention_topk(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, float* out,
                       int64_t ldo, int64_t n_q, int64_t n_k, int64_t keep, int heads, int head_dim, void* stream);
int rdm_attention_self_pair_topk(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                 float* out, int64_t ldo, int64_t n0, int64_t n1, int64_t keep0, int64_t keep1, int heads,
                                 int head_dim, void* stream);
int64_t rdm_topk_count(int64_t n, double frac);

/* ---- a8/a9 helpers ------------------------------------------------------------------------------
 * rdm_vote_shift: xyz + clamp(offset[:, :3], +-limit) (rdmnet/vote/vote.py:98-108).
 * rdm_sigmoid_column: clamp(sigmoid(x[:, 0]), 0, 1) of a strided column (experiments/model_infer.py:161-162).
 * rdm_l2_normalize: F.normalize(x, p=2, dim=1) (experiments/model_infer.py:248-249).              */
int rdm_vote_shift(const float* xyz, const float* offsets, int64_t ldo, int64_t n, float lx, float ly,
                   float lz, float* out, void* stream);
int rdm_sigmoid_column(const float* x, int64_t ldx, int64_t n, float* out, void* stream);
int rdm_l2_normalize(const float* x, int64_t ldx, int64_t n, int64_t c, float* y, int64_t ldy, void* stream);

/* ---- a10: NMS -----------------------------------------------------------------------------------
 * keep[i] = 1 iff no lower-index neighbour of row i is kept: the greedy index-order sweep of
 * NMS.forward (rdmnet/vote/vote.py:33-40) given the radius-neighbour rows of the shifted nodes.
 * rdm_compact_indices: order-preserving list of kept rows in [begin, end) and their count (the
 * boolean-mask selects of experiments/model_infer.py:221-229).                                   */
int rdm_nms(const int64_t* idx, int64_t n, int64_t h, int64_t ldi, const int32_t* width, uint8_t* keep,
            void* stream);
int rdm_compact_indices(const uint8_t* keep, int64_t begin, int64_t end, int32_t* order, int32_t* count,
                        void* stream);

/* ---- a11: point-to-node grouping -----------------------------------------------------------------
 * Replaces point_to_node_partition (geotransformer/modules/ops/pointcloud_partition.py:60-107) for
 * one cloud: every point joins its nearest node (first minimum of the reference's fp32 distance
 * formula), every node keeps its k nearest OWN points ascending by (distance, index); unused slots
 * hold n_points / mask 0.  status != 0 if a node owns more than 4096 points.                     */
size_t rdm_point_to_node_workspace_bytes(int64_t n_points, int64_t n_nodes);
int rdm_point_to_node(const float* points, int64_t n_points, const float* nodes, int64_t n_nodes, int k,
                      int64_t* knn_idx, uint8_t* knn_mask, uint8_t* node_mask, int32_t* status, void* ws,
                      size_t ws_bytes, void* stream);
/* rdm_point_to_node_pair: the same grouping for the two clouds of a pair (a: ref, b: src) with one set of launches;
 * workspace: rdm_point_to_node_workspace_bytes(n_a, m_a) + rdm_point_to_node_workspace_bytes(n_b, m_b).         */
int rdm_point_to_node_pair(const float* points_a, int64_t n_a, const float* nodes_a, int64_t m_a, const float* points_b,
                           int64_t n_b, const float* nodes_b, int64_t m_b, int k, int64_t* knn_idx_a, uint8_t* knn_mask_a,
                           uint8_t* node_mask_a, int64_t* knn_idx_b, uint8_t* knn_mask_b, uint8_t* node_mask_b,
                           int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- a12: coarse matching -------------------------------------------------------------------------
 * Replaces SuperPointMatching.forward (geotransformer/modules/geotransformer/superpoint_matching.py:
 * 14-61).  scores holds f_ref . f_src^T on entry (rdm_gemm, trans_b) and the dual-normalised
 * matching scores on return; the k best (descending, ties by flat index) are written as node
 * indices + scores, *out_count = min(k, #non-empty pairs).                                        */
size_t rdm_coarse_matching_workspace_bytes(int64_t m, int64_t n);
int rdm_coarse_matching(float* scores, int64_t m, int64_t n, int64_t ld, const uint8_t* ref_mask,
                        const uint8_t* src_mask, int dual_normalization, int k, int64_t* ref_idx,
                        int64_t* src_idx, float* out_scores, int32_t* out_count, void* ws, size_t ws_bytes,
                        void* stream);

/* rdm_coarse_matching_features: the same stage from the L2-normalised superpoint features themselves
 * (superpoint_matching.py:14-61 with pairwise_distance(normalized=True), ops/pairwise_distance.py:4-31): dot
 * products, exp, row / column sums and the dual normalisation are evaluated in fp64 and rounded once to the
 * fp32 score that is ranked.  The reference's top-k order hangs on relative score gaps down to 4e-7
 * (tests/golden/coarse_order_analysis.json); this entry reproduces the reference's indices exactly when fed the
 * reference's features, which the fp32 pipeline above (GEMM, then rdm_coarse_matching) cannot promise.
 * ref_feats [m, d] (row stride ld_ref), src_feats [n, d]; d <= 448.                                         */
size_t rdm_coarse_matching_features_workspace_bytes(int64_t m, int64_t n);
int rdm_coarse_matching_features(const float* ref_feats, int64_t ld_ref, int64_t m, const float* src_feats,
                                 int64_t ld_src, int64_t n, int64_t d, const uint8_t* ref_mask,
                                 const uint8_t* src_mask, int dual_normalization, int k, int64_t* ref_idx,
                                 int64_t* src_idx, float* out_scores, int32_t* out_count, void* ws,
                                 size_t ws_bytes, void* stream);

/* ---- §7 descriptor matching: exact nearest-feature correspondences ----------------------------------------------------
 * Replaces get_nearest_neighbor (geotransformer/utils/pointcloud.py:11-22, a cKDTree over the feature rows) as
 * extract_corr_indices_from_feats / extract_correspondences_from_feats use it (geotransformer/utils/registration.py:222-277).
 * a [n, c] (row stride lda), b [m, c] (row stride ldb): device f32, finite, 1 <= c <= 1024; float4 loads when c, lda, ldb are
 * multiples of 4 and both pointers 16-byte aligned, scalar loads otherwise.  nn_ab [n] i64: for every row of a the row of b
 * with the smallest sum_c (a_ic - b_jc)^2 EVALUATED IN FLOAT64 on the fp32 inputs, the lowest index among exactly equal
 * distances (cKDTree leaves ties open); dist_ab [n] f32 (may be null): sqrt of that float64 sum, rounded to fp32.  With
 * both_sides also nn_ba [m] / dist_ba [m]: the nearest row of a for every row of b.  The fp32 MFMA tiles of |a|^2 + |b|^2 -
 * 2 a.b decide a line only where their two best candidates are further apart than twice the proven round-off bound
 * (c + 8) 2^-24 (|a_i|^2 + max_j |b_j|^2); every other line is evaluated in float64 against every row of the other side
 * (feature_match.hip).  No n x m matrix is written, no float atomics, results do not depend on scheduling.
 * phase2_lines (optional, device int32[2]): the lines of a / of b that took the float64 pass.  n = 0: nothing is written
 * (RDM_ERR_ARG with both_sides); m = 0: RDM_ERR_ARG.  n, m < 2^31 - 128, n <= 65535 * 128.  No synchronisation.
 * rdm_feature_match_select turns the two index vectors into extract_corr_indices_from_feats' output on the device:
 * mode 0 = (arange(n), nn_ab); 1 = mutual: the i with nn_ba[nn_ab[i]] == i, ascending, and their nn_ab; 2 = bilateral:
 * ([arange(n), nn_ba], [nn_ab, arange(m)]).  ref_idx / src_idx i64 and dist f32 (optional; the rows' dist_ab, then dist_ba)
 * with capacity n (n + m for mode 2); *count (device int32) = rows written.                                              */
size_t rdm_feature_match_workspace_bytes(int64_t n, int64_t m, int both_sides);
int rdm_feature_match(const float* a, int64_t lda, int64_t n, const float* b, int64_t ldb, int64_t m, int64_t c, int both_sides,
                      int64_t* nn_ab, float* dist_ab, int64_t* nn_ba, float* dist_ba, int32_t* phase2_lines, void* ws,
                      size_t ws_bytes, void* stream);
int rdm_feature_match_select(int mode, const int64_t* nn_ab, const float* dist_ab, const int64_t* nn_ba, const float* dist_ba,
                             int64_t n, int64_t m, int64_t* ref_idx, int64_t* src_idx, float* dist, int32_t* count, void* stream);

/* ---- evaluation: ground-truth superpoint correspondences ----------------------------------------------------
 * Replaces get_node_correspondences (geotransformer/modules/registration/matching.py:252-350) as test.py's evaluation
 * forward calls it (experiments/model.py:283-295, radius cfg.model.ground_truth_matching_radius = 0.6,
 * experiments/config.py:101).  ref/src nodes [m,3] / [n,3]; patches of k <= 128 slots: with ref_knn_idx / src_knn_idx
 * null, *_points are the gathered patch points [m*k, 3] / [n*k, 3] (the reference's knn points); otherwise *_points are
 * the clouds' points [*_n_points, 3] and *_knn_idx the int64 [m,k] / [n,k] slot indices into them, an index outside
 * [0, n_points) standing for the zero pad row (rdm_point_to_node's layout).  Masks (u8, 1 = valid) may be null = all
 * valid, as the reference's None.  transform: device f32 4x4 row-major, src -> ref; pos_radius in double as the Python
 * float it is (the sphere test uses (float)pos_radius, the point test (float)(pos_radius^2)).
 * Outputs: the candidates with overlap > 0 in row-major (ref, src) order (torch.nonzero's): out_indices int64 [C,2],
 * out_overlaps f32 [C], at most `capacity` rows written; counts (device int32[2]) = {C, B} (B = candidate pairs that pass
 * the sphere test); *status (device int32, caller zeroes) = 1 when C > capacity (-> RDM_ERR_CAPACITY for the caller).
 * Workspace: rdm_gt_node_correspondences_workspace_bytes(m, n) (about 4 B per node pair, the worst case B = m*n).
 * m * n <= 2^31.                                                                                                      */
size_t rdm_gt_node_correspondences_workspace_bytes(int64_t m, int64_t n);
int rdm_gt_node_correspondences(const float* ref_nodes, int64_t m, const float* src_nodes, int64_t n,
                                const float* ref_points, const int64_t* ref_knn_idx, int64_t ref_n_points,
                                const float* src_points, const int64_t* src_knn_idx, int64_t src_n_points, int k,
                                const uint8_t* ref_node_mask, const uint8_t* src_node_mask, const uint8_t* ref_knn_mask,
                                const uint8_t* src_knn_mask, const float* transform, double pos_radius,
                                int64_t* out_indices, float* out_overlaps, int64_t capacity, int32_t* counts,
                                int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- a14: Sinkhorn ---------------------------------------------------------------------------------
 * Replaces LearnableLogOptimalTransport.forward (geotransformer/modules/sinkhorn/
 * learnable_sinkhorn.py:13-66): scores [batch, m, n], masks [batch, m] / [batch, n] (1 = valid),
 * alpha = dustbin score (device scalar), out [batch, m+1, n+1].  m, n <= 128.  Masked entries are
 * fl(-1e12), except where a whole side of a patch is masked, which gives the reference's values:
 * after >= 1 iteration, no valid row -> the dustbin column is -inf (every row) and the valid entries of
 * the dustbin row are 0; no valid column -> the mirror image; neither -> NaN everywhere (-inf everywhere
 * with iters = 0).                                                                                 */
int rdm_sinkhorn(const float* scores, int64_t batch, int64_t m, int64_t n, const uint8_t* row_mask,
                 const uint8_t* col_mask, const float* alpha, int iters, float* out, void* stream);

/* ---- a15/a16: local-to-global registration ----------------------------------------------------------
 * Replaces LocalGlobalRegistration.forward (geotransformer/modules/geotransformer/
 * local_global_registration.py:204-243; k=1, dustbin, non-mutual) including weighted_procrustes
 * (geotransformer/modules/registration/procrustes.py:6-73) without the reference's host SVD.
 * Outputs have capacity batch*2*side rows; counts[0..2] = {n_correspondences, n_hypotheses, best}. */
size_t rdm_lgr_workspace_bytes(int64_t batch);
int rdm_lgr(const float* log_scores, const float* ref_knn_points, const float* src_knn_points,
            const uint8_t* ref_knn_masks, const uint8_t* src_knn_masks, int64_t batch, int64_t side,
            float acceptance_radius, int correspondence_threshold, int num_refinement_steps, float* ref_corr,
            float* src_corr, float* corr_scores, float* transform, int32_t* counts, void* ws, size_t ws_bytes,
            void* stream);

/* cfg.fine_matching beyond the three keys of rdm_lgr (experiments/config.py:152-161; passed to LocalGlobalRegistration at
 * experiments/model_infer.py:91-101).  The shipped values are {1, 0, 1, 0, 0.f, 0}.                                   */
typedef struct rdm_fine_matching_options {
  int32_t topk;                 /* k of both top-k selections, 1 .. side (side + 1 with use_dustbin)                    */
  int32_t mutual;               /* 1: a correspondence needs both sides (and), 0: either (or)                           */
  int32_t use_dustbin;          /* 1: test against the line's dustbin entry, 0: against confidence_threshold            */
  int32_t use_global_score;     /* 1: corr_scores are multiplied by the patch's superpoint-pair score                   */
  float confidence_threshold;   /* >= 0; read without use_dustbin only                                                  */
  int32_t correspondence_limit; /* 0: none; L >= 1: hypotheses are scored and the pose refined on the L best-scored    */
} rdm_fine_matching_options;

/* LocalGlobalRegistration.forward with every option (local_global_registration.py:49-91 compute_correspondence_matrix,
 * :145-202 local_to_global_registration, :229-243 forward).  (i, j) is a candidate of the ref side iff j is among the topk
 * largest of row i of S = exp(log_scores) -- the dustbin column included with use_dustbin -- and S[i,j] exceeds the row's dustbin
 * entry (use_dustbin) or confidence_threshold; the src side likewise over columns; `mutual` combines them; both knn masks
 * apply.  Among equal values at a k-th boundary the lowest index is kept (torch.topk leaves it open).  corr_scores =
 * S[i,j] (x global_scores[patch] with use_global_score, after the test).  correspondence_limit = L: if more than L
 * correspondences exist, the local hypotheses -- still fitted on every patch with >= correspondence_threshold of ALL its
 * correspondences -- are scored, and the pose is refined, on the L with the largest scores (lowest position among equal scores
 * at the boundary), kept in nonzero order; the outputs still list all C, counts[0] = C.
 * log_scores [batch, score_dim, score_dim]: score_dim = side + 1 (the Sinkhorn output; without use_dustbin only its
 * [side, side] block is read, model_infer.py:319-320) or, without use_dustbin, side.  global_scores [batch] (may be null
 * without use_global_score).  Outputs have capacity rdm_lgr_options_capacity = batch * min(2 topk side, side^2) rows (0 for
 * invalid arguments, as the workspace size).  With the shipped values the result equals rdm_lgr's bit for bit.
 * RDM_ERR_ARG for options outside the ranges above.                                                                         */
int64_t rdm_lgr_options_capacity(int64_t batch, int64_t side, const rdm_fine_matching_options* options);
size_t rdm_lgr_options_workspace_bytes(int64_t batch, int64_t side, const rdm_fine_matching_options* options);
int rdm_lgr_options(const float* log_scores, int64_t score_dim, const float* ref_knn_points, const float* src_knn_points,
                    const uint8_t* ref_knn_masks, const uint8_t* src_knn_masks, const float* global_scores, int64_t batch,
                    int64_t side, float acceptance_radius, int correspondence_threshold, int num_refinement_steps,
                    const rdm_fine_matching_options* options, float* ref_corr, float* src_corr, float* corr_scores,
                    float* transform, int32_t* counts, void* ws, size_t ws_bytes, void* stream);

/* ---- native orchestration: one call per scan pair ----------------------------------------------
 * rdm_engine_run = the collate of geotransformer/utils/data.py:13-77 + RDMNet.forward of
 * experiments/model_infer.py:109-354 as a fixed sequence of the kernels above on one stream, with
 * activations in an engine-owned device arena (the ~700 launches of a pair cost ~2 us each from
 * native code instead of ~15 us each from Python).  Parameters are handed over by their reference
 * state-dict names (weights/rdmnet.pth.tar -> state['model'], engine/base_tester.py:97-107).
 * An engine is bound to the device that is current when it is created and must be used by one host
 * thread at a time; create one engine per in-flight pair.                                        */
typedef struct rdm_engine rdm_engine;

typedef struct rdm_engine_config {
  int num_stages;             /* 5 */
  int kernel_size;            /* 15 */
  int group_norm;             /* 32 */
  float init_voxel_size;      /* 0.3 */
  float init_radius;          /* 4.25 * 0.3 */
  float init_sigma;           /* 2.0 * 0.3 */
  int neighbor_limits[5];
  int out_dim;                /* 256 */
  int num_heads;              /* 4 */
  int num_layers;             /* 4 (self,cross) pairs, transformer #1 */
  int num_layers2;            /* 4, transformer #2 */
  int vote_mlp_layers;        /* 2 */
  float vote_limit[3];        /* 3.0 m */
  float nms_radius;           /* 2.4 m */
  int points_in_patch;        /* 128 */
  int num_correspondences;    /* 256 */
  int dual_normalization;     /* 1 */
  int sinkhorn_iterations;    /* 100 */
  float acceptance_radius;    /* 0.6 m */
  int correspondence_threshold; /* 3 */
  int num_refinement_steps;   /* 5 */
  int use_vote;               /* 1; 0 = infer.py:119-120 (Mulran): superpoints = un-shifted coarse points with the
                                 first transformer's features (the reference leaves this case undefined) */
  int attention_bf16;         /* 0 = fp32 QK^T / PV; 1 = bf16 operands, fp32 softmax + accumulation */
  size_t arena_bytes;         /* 0 = default (3 GiB) */
} rdm_engine_config;

typedef struct rdm_engine_result {
  float transform[16];        /* estimated_transform, row-major 4x4, src -> ref (host copy) */
  int32_t n_correspondences, n_hypotheses, best_hypothesis;
  int64_t n_ref_nodes, n_src_nodes, n_node_correspondences;
  int64_t level_sizes[5];        /* stacked [ref; src] points per pyramid level */
  int64_t level_ref_sizes[5];    /* of which ref */
  const float* ref_corr_points;  /* device, [n_correspondences, 3]; valid until the next run */
  const float* src_corr_points;
  const float* corr_scores;
  const float* transform_dev;
  size_t arena_used;
  /* the same correspondences on the HOST (engine-owned pinned memory, written by the run's last kernel; valid until the
   * next call on this engine): what infer.py:70-101 reads after `.cpu()`.  n_host_correspondences == n_correspondences
   * (the buffer holds the path's upper bound, num_correspondences x 2 x points_in_patch).                             */
  const float* host_ref_corr_points;  /* [n, 3] */
  const float* host_src_corr_points;  /* [n, 3] */
  const float* host_corr_scores;      /* [n] */
  int32_t n_host_correspondences;
} rdm_engine_result;

typedef struct rdm_tensor_view {
  void* data;                 /* device pointer into the engine arena (valid until the next run) */
  int64_t rows, cols, ld;     /* ld in elements */
  int dtype;                  /* 0 = f32, 1 = i64, 2 = u8, 3 = i32 */
} rdm_tensor_view;

typedef struct rdm_kpconv_profile {   /* one KPConv layer of the last run (HIP events on the run's stream) */
  int64_t m, h, c_in, c_out, pooled_channels;
  float gather_ms;            /* the neighbourhood kernel alone: rdm_kpconv_gather, or rdm_kpconv_fused (gather + weight
                                 contraction in one kernel) when `fused` */
  float total_ms;             /* whole layer: + weight GEMM (two-kernel form) or + GroupNorm passes (fused form), + the
                                 shortcut max-pool of strided blocks */
  int32_t fused;              /* 1: the layer ran as ONE kernel (c_in = 1, 32, 64) */
  int32_t reserved;
} rdm_kpconv_profile;

int rdm_engine_create(const rdm_engine_config* cfg, rdm_engine** out);
void rdm_engine_destroy(rdm_engine* e);
int rdm_engine_set_param(rdm_engine* e, const char* name, const float* data_host, const int64_t* shape_host, int ndim);
int rdm_engine_finalize(rdm_engine* e);
/* Instead of set_param + finalize: `e` uses the prepared device parameters of `src` (finalized, SAME device, same model-shape
 * fields of the configuration -- else RDM_ERR_ARG) -- one copy of the weights for all the engines a process keeps in flight.
 * The parameter set is reference counted: the engines may be destroyed in any order (the device memory goes with the last
 * user), and rdm_engine_finalize of `src` afterwards gives `src` a fresh set while its sharers keep the one they have.   */
int rdm_engine_share_params(rdm_engine* e, const rdm_engine* src);
/* ref/src points: device f32 [n,3].  Synchronises `stream` (4 small read-backs of data-dependent sizes). */
int rdm_engine_run(rdm_engine* e, const float* ref_points, int64_t n_ref, const float* src_points, int64_t n_src,
                   rdm_engine_result* result_host, void* stream);

/* The reference's `data_dict` (experiments/model_infer.py:113-124, produced by registration_collate_fn_stack_mode,
 * geotransformer/utils/data.py:139-192) as device pointers: what RDMNet.forward(data_dict) reads.  Clouds are stacked
 * [ref; src]; index tables are int64 row-major with the stated row stride (the reference hands over `[:, :limit]`
 * views), pad index = number of support points.  `*_count` are optional device int32 scalars holding the effective
 * table width min(limit, max_count) when a table was allocated wider than that (this library's own collate without
 * the shape read-back); null = every column is valid, as in the reference's tensors.                              */
typedef struct rdm_data_dict {
  const float* features;  int64_t features_ld;       /* [n_points[0], 1] */
  const float* points[5];                            /* [n_points[i], 3] contiguous */
  const int64_t* lengths[5];                         /* device int64[2] per level */
  int64_t n_points[5], n_ref[5];                     /* host copies: stacked rows per level, of which ref */
  const int64_t* neighbors[5];   int64_t neighbors_width[5],   neighbors_ld[5];   const int32_t* neighbors_count[5];
  const int64_t* subsampling[4]; int64_t subsampling_width[4], subsampling_ld[4]; const int32_t* subsampling_count[4];
  const int64_t* upsampling[4];  int64_t upsampling_width[4],  upsampling_ld[4];  const int32_t* upsampling_count[4];
  /* optional: the {max count, status} words of the searches that built the tables (rdm_engine_collate's "search_flags",
   * device int32 [n_collate_status, 2]).  A non-zero status word makes rdm_engine_forward return RDM_ERR_CAPACITY at its
   * first read-back instead of computing on a broken table; null / 0 for tables from another collate.              */
  const int32_t* collate_status; int64_t n_collate_status;
} rdm_data_dict;

/* rdm_engine_collate = the collate alone (registration_collate_fn_stack_mode / precompute_data_stack_mode,
 * geotransformer/utils/data.py:13-77,139-192) as ONE native call: four subsamplings + 13 searches; the tables stay in the
 * engine's arena as stage tensors "points0..4", "lengths0..4" (i64 [1,2]), "neighbors0..4", "subsampling0..3",
 * "upsampling0..3" (i64 [n, limit]; effective widths in "search_flags", i32 [32,2] = {max count, status} per search in the
 * order self / sub / up per level) -- fetch them with rdm_engine_export.  result_host receives the level sizes.      */
int rdm_engine_collate(rdm_engine* e, const float* ref_points, int64_t n_ref, const float* src_points, int64_t n_src,
                       rdm_engine_result* result_host, void* stream);

/* rdm_engine_forward = RDMNet.forward(data_dict) alone (experiments/model_infer.py:109-354): the same native sequence
 * as rdm_engine_run after its collate, on tables the caller built -- with this library's collate
 * (rdmnet_amd.collate) or the reference's.  Same result structure, taps and waits as rdm_engine_run; bit-identical to
 * it when fed the tables rdm_engine_run builds itself.                                                              */
int rdm_engine_forward(rdm_engine* e, const rdm_data_dict* data, rdm_engine_result* result_host, void* stream);

/* Batched collate (round 5): the collates of `n_pairs` (1 .. 16) pairs -- precompute_data_stack_mode, data.py:13-77, once per
 * pair in the reference's DataLoader workers -- as ONE sequence of launches: every subsampling launch works on 2 * n_pairs
 * clouds, the search grids are built as (pair, level) items, the 12 searches a plain run needs per pair are flushed 16 per
 * launch, the level sizes of all pairs return in one read-back.  The pyramids stay in the engine's arena;
 * rdm_engine_forward_batched(e, k, ...) then runs RDMNet.forward (model_infer.py:109-354) of pair k on them: result structure,
 * waits and read-outs of rdm_engine_run, and the same bits (every pair's tables, points and query order are what its own
 * collate writes).  ref_points / src_points: host arrays of device pointers, float32 [n, 3] each; the clouds must stay valid
 * until the collate has run on `stream`.  Not with rdm_engine_keep_taps (a run that keeps its stage tensors builds the
 * reference's full tables).  Any other run on the engine discards the batch.                                          */
int rdm_engine_collate_batch(rdm_engine* e, int n_pairs, const float* const* ref_points, const int64_t* n_ref,
                             const float* const* src_points, const int64_t* n_src, void* stream);
int rdm_engine_forward_batched(rdm_engine* e, int k, rdm_engine_result* result_host, void* stream);

/* Lock step (round 5, experimental): rdm_engine_run of `n_pairs` (1 .. 8) pairs on as many engines -- one arena and one
 * result buffer each, the weights shared (rdm_engine_share_params) -- on ONE stream: the runs advance together on the calling
 * thread, the launches of the same kernel of all pairs go out as one grouped launch, the size read-backs of the pairs become
 * waits of the group.  What the reference does pair after pair (engine/single_tester.py:86-134) and this library otherwise does on
 * one stream per pair.  Every pair: the bits of rdm_engine_run on it alone.  collate_batched != 0: the collates of the group run
 * as one launch sequence on engines[0] (rdm_engine_collate_batch) before the forwards run in lock step (not when engines[0] keeps
 * its stage tensors).  A pair that exhausts its arena is run again on its own (the arena grows as in rdm_engine_run).        */
int rdm_engine_run_lockstep(rdm_engine* const* engines, int n_pairs, const float* const* ref_points, const int64_t* n_ref,
                            const float* const* src_points, const int64_t* n_src, rdm_engine_result* const* results,
                            int collate_batched, void* stream);
/* rdm_engine_forward of `n_pairs` (1 .. 8) callers' data_dicts on as many engines in lock step (round 6): the drop-in operator
 * API -- model(data_dict), experiments/model_infer.py:109-354 -- for several pairs on one stream; with rdm_engine_keep_taps every
 * engine holds the stage tensors of ITS pair afterwards (rdm_engine_export per engine).  Every pair: the bits of
 * rdm_engine_forward on it alone.                                                                                            */
int rdm_engine_forward_lockstep(rdm_engine* const* engines, int n_pairs, const rdm_data_dict* const* data,
                                rdm_engine_result* const* results, void* stream);
/* rdm_engine_collate of `n_pairs` (1 .. 8) pairs on as many engines in lock step: what the reference's DataLoader workers do pair
 * by pair (registration_collate_fn_stack_mode, geotransformer/utils/data.py:139-192); every engine then holds its pair's
 * pyramid and 13 tables as stage tensors, exactly as after rdm_engine_collate on the pair alone.                              */
int rdm_engine_collate_lockstep(rdm_engine* const* engines, int n_pairs, const float* const* ref_points, const int64_t* n_ref,
                                const float* const* src_points, const int64_t* n_src, rdm_engine_result* const* results, void* stream);
/* DIAGNOSTIC, process-global (not part of the stateless compute ABI): developer counters of the lock-step scheduler
 * (tools/lockstep_lab.py): out[0..5] = ns spent in lock-step runs, ns of them in
 * host waits, waits, grouped launches, records carried, runs (summed over threads; reset != 0 clears them).  In the lab build
 * (make lab), with RDM_LOCKSTEP_STATS in the environment, rdm_lockstep_stats_dump prints launches and records per kernel.    */
void rdm_lockstep_stats(long long* out, int reset);
/* DIAGNOSTIC: self-test of the lock-step scheduler on scripted stand-in launches (no GPU needed; tests/test_lockstep.py). */
int rdm_lockstep_selftest(int n_ctx, const int* script, int len, int* log, int cap, int* rcs);
/* DIAGNOSTIC: self-test of the grouped launch on the GPU (tests/test_lockstep_gpu.py).  `n_ctx` (1 .. 8) contexts of a real
 * lock-step group launch a probe kernel through the product path with scripted grids: script[(k * len + s) * 4 ..] = (gx, gy, gz,
 * dynamic LDS bytes) of context k's step s (host memory); gx < 0 = a host wait, a grid with a zero dimension = nothing.  Every
 * workgroup of every launch owns one slot of 10 int32 in `out` (device memory, zeroed by the caller, `cap_slots` slots):
 * {threads seen, visits, tag = k * len + s, blockIdx.x/y/z, gridDim.x/y/z, LDS round trip ok}, slots in the order (context, step,
 * linear workgroup id of the step's own grid).  threads = 64 | 256 selects one of the probe's two instantiations.  Waits for
 * `stream`.  Returns the number of slots written, or a negative error code (rdm_last_error).                                    */
int rdm_lockstep_selftest_gpu(int n_ctx, const int* script, int len, int threads, int32_t* out, int64_t cap_slots, void* stream);
void rdm_lockstep_stats_dump(void);
/* Stage intermediates by name (test/inspection aid): enable before a run, query after it. */
/* Per-KPConv-layer HIP-event timing of the last run; get_profile returns the number of layers. */
/* Re-allocates the engine's activation arena at `bytes`, growable (rdm_engine_config.arena_bytes != 0 fixes the size instead; the
 * default is 3 GiB, doubled and the pair re-run when a pair exhausts it).  For callers that know their largest pair or lock-step
 * group; the reference has no counterpart (torch's caching allocator).  Waits for the device; drops a collated batch.           */
int rdm_engine_reserve(rdm_engine* e, size_t bytes);
/* How rdm_engine_run waits for its stream at the size read-backs: sleep_us = 0 (default) uses hipStreamSynchronize,
 * which spins a host core per in-flight pair; sleep_us > 0 polls hipStreamQuery and sleeps that long in between (for
 * hosts whose CPU quota is smaller than ranks x pairs in flight). */
int rdm_engine_set_wait(rdm_engine* e, int sleep_us);
/* How many scan pairs the caller keeps in flight on this GPU (one engine and stream each; default 1).  A scheduling hint, results do
 * not depend on it: from 3 the tiled GEMM leaves half of a CU's registers and LDS to the other pairs' kernels (two workgroups
 * per CU instead of four: +3 % pairs/s at four in flight, -2 % with one pair alone, docs/EXPERIMENTS.md 5d).                            */
int rdm_engine_set_pairs_in_flight(rdm_engine* e, int n);
/* Latency mode.  With one pair in flight most of the GPU idles while chains of one-workgroup kernels run, so the engine runs the
 * wide, independent parts of a pair -- the first level's grid, neighbour search and encoder blocks beside the subsampling of the
 * deeper levels; the decoder beside the second transformer / grouping / coarse-matching chain -- on a side stream of its own
 * (created on first use) and joins them by host waits next to read-backs the run performs anyway.  Same kernels on the same
 * operands: results are bit-identical in every mode.  mode: 0 = never, 1 = when pairs_in_flight == 1 (default), 2 = always.
 * Not used when `stream` is the null stream; the first half only when `stream` is idle at the call.  The side stream must lie on
 * another hardware pipe than `stream` (two queues of one pipe are served in turns); the engine finds that out with a pair of 60 us
 * spin kernels the first time it sees a caller stream (a few hundred microseconds, once) and stays serial where no such stream exists.
 * The reference has no counterpart (its loop is synchronous: geotransformer/engine/single_tester.py:86-134).                    */
int rdm_engine_set_overlap(rdm_engine* e, int mode);
/* cfg.thdroformer.k2: self layer i (0 .. n_layers - 1) of transformer #2 runs rdm_attention_self_pair_topk with
 * keep = rdm_topk_count(n, fracs[i]) for each cloud's superpoint count n; fracs[i] < 0, layers past n_layers, transformer #1 and
 * every cross layer stay dense.  fracs[i] must be <= 1; not with attention_bf16.  n_layers = 0 clears the setting.  Valid
 * before or after finalize / share_params (the setting is the engine's own, not part of the shared parameters).            */
int rdm_engine_set_attention_topk(rdm_engine* e, int n_layers, const double* fracs);
/* cfg.fine_matching.{topk, mutual, use_dustbin, confidence_threshold, use_global_score, correspondence_limit}
 * (experiments/model_infer.py:91-101, :319-329): the engine's registration then runs rdm_lgr_options -- global_scores are the
 * superpoint-pair scores of coarse matching -- and its correspondence buffers, the mapped host buffer among them, hold
 * num_correspondences * min(2 topk K, K^2) rows.  NULL restores rdm_lgr.  Call it after rdm_engine_create and before the
 * engine's first run (it re-allocates the host buffer); the setting is the engine's own, not part of the shared parameters,
 * so the engines of a lock-step group may differ in it.                                                              */
int rdm_engine_set_fine_matching(rdm_engine* e, const rdm_fine_matching_options* options);
/* Per-KPConv-layer profile of the next runs: 0 = off, 1 = HIP events around every layer's neighbourhood kernel and around the
 * whole layer (rdm_engine_get_profile: sizes + milliseconds), 2 = the layers' sizes only, no events -- for the other pairs of a
 * lock-step group whose first engine records the events: the launches (and durations) are the group's.                     */
int rdm_engine_enable_profile(rdm_engine* e, int enable);
int rdm_engine_get_profile(rdm_engine* e, rdm_kpconv_profile* out, int cap);
int rdm_engine_keep_taps(rdm_engine* e, int enable);
int rdm_engine_get_tensor(rdm_engine* e, const char* name, rdm_tensor_view* out);
/* Copies n stage tensors of the last run into caller buffers (dst[i]: rows * ld * element size bytes of names[i]) with
 * one batched launch: how model(data_dict) fills the reference's output_dict (model_infer.py:133-334).           */
int rdm_engine_export(rdm_engine* e, int n, const char* const* names, void* const* dst, void* stream);
/* rdm_engine_get_tensor for n names at once (out[n]). */
int rdm_engine_describe(rdm_engine* e, int n, const char* const* names, rdm_tensor_view* out);
/* The same stage (rdm_gt_node_correspondences; experiments/model.py:283-295 -> matching.py:252-350) on the LAST run's
 * resident superpoints, patches and fine points (rdm_engine_run / _forward / _forward_batched / the lock-step entries, per
 * engine): no upload, no export.  transform: device f32 4x4 (src -> ref).  Writes at most `capacity` rows to out_indices
 * (int64 [C,2]) / out_overlaps (f32 [C]); count_host[0..1] = {C, B} (host int64[2]).  Scratch comes from the engine's
 * arena above the last run's tensors.  Synchronises `stream`; returns RDM_ERR_CAPACITY when C > capacity (nothing written
 * past capacity) and RDM_ERR_ARG when the engine has no completed forward run (e.g. after rdm_engine_collate alone).   */
int rdm_engine_gt_node_correspondences(rdm_engine* e, const float* transform, double pos_radius, int64_t* out_indices,
                                       float* out_overlaps, int64_t capacity, int64_t* count_host, void* stream);
/* Descriptor matching (rdm_feature_match + rdm_feature_match_select) on the LAST run's resident tensors, no upload, no export:
 * level 0 = fine (ref/src_points_f, ref/src_feats_f: the first level's points and the decoder's features), 1 = coarse
 * (ref/src_points_c, ref/src_feats_c: the superpoints and their normalised features); mode as rdm_feature_match_select.  All
 * four tensors stay in the arena after a plain run, so rdm_engine_keep_taps is not needed.  Per engine after its run, also for
 * the engines of a lock-step group (not a grouped launch).  Outputs (device, capacity rows: >= n_ref, n_ref + n_src for mode
 * 2, else RDM_ERR_CAPACITY): ref_idx / src_idx i64, ref_points / src_points f32 [.,3] (optional), dists f32 (optional).
 * count_host (host int64[3]) = {correspondences, lines of ref, lines of src that took the float64 pass}.  Scratch comes
 * from the arena above the last run; synchronises `stream`; RDM_ERR_ARG without a completed forward run.                */
int rdm_engine_feature_correspondences(rdm_engine* e, int level, int mode, int64_t* ref_idx, int64_t* src_idx, float* ref_points,
                                       float* src_points, float* dists, int64_t capacity, int64_t* count_host, void* stream);
/* Ground-truth point correspondences (rdm_ball_count + rdm_ball_fill) on the LAST run's resident points, no upload, no export:
 * level 0 = the full-resolution input clouds, 1 = the fine level (ref/src_points_f), 2 = the superpoints (ref/src_points_c);
 * transform_host float64 4x4 on the host, src -> ref (null: identity).  Per engine after its run, also for the engines of a
 * lock-step group.  The count call takes its workspace from the arena above the last run, fills totals_host (host int64[4],
 * as rdm_ball_count) and synchronises `stream`; the fill call writes out int64 [C, 2] (device, capacity >= C rows, else
 * RDM_ERR_CAPACITY), synchronises and releases the workspace (so does the next count call or run).  A forward that is not
 * followed by these calls launches nothing for them.  RDM_ERR_ARG without a completed forward run / a pending count call. */
int rdm_engine_gt_point_correspondences_count(rdm_engine* e, int level, const double* transform_host, double radius,
                                              int64_t* totals_host, void* stream);
int rdm_engine_gt_point_correspondences_fill(rdm_engine* e, int64_t* out, int64_t capacity, void* stream);
/* How well a pose aligns the LAST run's resident clouds, without ground truth (two rdm_nearest calls, no upload, no export):
 * levels as above; transform_host float64 4x4 on the host, src -> ref (null: the run's own estimated_transform).  Both sides
 * are measured in the ref frame: ref rows against the moved src cloud, moved src rows against the ref cloud.  out_host (host
 * double[8]) = {ref rows with a neighbour nearer than radius, their sum of d2, the sum of all ref rows' nearest distances, the
 * same three for the src rows, n_ref, n_src}.  Per engine after its run, also for the engines of a lock-step group; the
 * workspace lies in the arena above the last run and is released before the call returns (a pending count call's too);
 * synchronises `stream`.  A forward that is not followed by this call launches nothing for it.  radius <= 0 and an engine
 * without a completed forward run are RDM_ERR_ARG.                                                                      */
int rdm_engine_alignment_quality(rdm_engine* e, int level, const double* transform_host, double radius, double* out_host,
                                 void* stream);
/* rdm_information_matrix on the LAST run's resident clouds (no upload, no export): levels as above; source = the src cloud moved
 * by transform_host (float64 4x4 on the host, src -> ref; null: the run's own estimated_transform), target = the ref cloud;
 * out_host (host double[40]), corr_out (device int64 [C, 2], rows (src row, ref row); optional) and capacity as
 * rdm_information_matrix.  Per engine after its run, also for the engines of a lock-step group; the workspace lies in the arena
 * above the last run and is released before the call returns (a pending count call's too); synchronises `stream`.  A forward
 * that is not followed by this call launches nothing for it.  radius <= 0 and an engine without a completed forward run are
 * RDM_ERR_ARG; C > capacity is RDM_ERR_CAPACITY.                                                                          */
int rdm_engine_information_matrix(rdm_engine* e, int level, const double* transform_host, double radius, double* out_host,
                                  int64_t* corr_out, int64_t capacity, void* stream);
/* Plain device-to-device copy on `stream` (lets a host without a HIP binding read arena tensors). */
int rdm_copy_device(void* dst, const void* src, size_t bytes, void* stream);

/* ---- §7 offline evaluator: the meters of experiments/eval.py for a batch of saved pairs ------------------------------
 * What eval.py:100-239 computes per pair file, for P pairs per call, with a number of launches that does not depend on P
 * (method RANSAC adds the three launches of rdm_ransac_correspondences per pair) and no host synchronisation.
 * Packed ragged device inputs:
 *   corr_offsets i64[P+1]; ref_corr, src_corr f32[sum C, 3]; corr_scores f32[sum C]   (pair p: rows corr_offsets[p] ..)
 *   gt_transform f32[P,16]; est_transform f32[P,16]: input for RDM_EVAL_LGR, output for the two other methods
 *   node_offsets i64[P+1], ref_node_corr, src_node_corr i64[sum]: the predicted superpoint pairs
 *   gt_offsets i64[P+1], gt_node_corr i64[sum, 2]: the ground-truth superpoint pairs; node_dims i64[P,2] = {M, N}
 * corr_offsets_host is the host's copy of corr_offsets (grid sizes, and the per-pair calls of RANSAC).
 * Per pair: (1) options.num_corr = L > 0 and C > L: the L best-scored rows -- the first L in the order (score descending, row
 * ascending), kept in row order (eval.py:121-125; np.argsort leaves equal scores open, here the lowest rows stay);
 * (2) the transform: the stored one (LGR), the weighted Procrustes of the selected rows with weights s / (sum s + 1e-5) --
 * float64 sums in a fixed order, Horn's solver (SVD, procrustes.py:6-73) --, or rdm_ransac_correspondences of the selected
 * rows (RANSAC; every pair with options.ransac_seed); (3) registration.py:175-200,361-375 on the selected rows: src moved
 * by gt_transform in fp32 (x r0 + y r1 + z r2 as two fma, then + t), fp32 residuals sqrt((dx dx + dy dy) + dz dz), their
 * mean (float64 sum), the rows below acceptance_radius, 0.3 and 0.1, and `overlap`: the ref rows whose nearest moved src
 * row (exact search) is closer than acceptance_radius; (4) registration.py:378-402: precision = predicted cells that are
 * ground-truth cells / (predicted cells + 1e-12), cells counted once on both sides; (5) registration.py:17-108 in float64 on
 * the fp32 matrices.  No atomics; every sum has a fixed order, so a pair's record does not depend on its batch.
 * records: device f64 [P, RDM_EVAL_RECORD_WIDTH]: {num_corr, residual, inlier_ratio, inlier_ratio_0.3, inlier_ratio_0.1,
 * overlap, precision, rre (degrees), rte, |d roll|, |d pitch|, |d yaw|, inliers, inliers_0.3, inliers_0.1, overlapping rows,
 * hit cells, predicted cells, ground-truth cells, superpoint indices outside M x N (ignored; 0 for valid input)}.  A pair
 * without correspondences has NaN in fields 1-5.                                                                          */
#define RDM_EVAL_RECORD_WIDTH 20
enum { RDM_EVAL_LGR = 0, RDM_EVAL_SVD = 1, RDM_EVAL_RANSAC = 2 };
typedef struct rdm_eval_options {
  int32_t method;             /* RDM_EVAL_* */
  int32_t num_corr;           /* eval.py --num_corr; 0 = every correspondence */
  double acceptance_radius;   /* cfg.eval.acceptance_radius (0.6) */
  float ransac_distance_threshold;  /* cfg.ransac: 0.3 */
  int32_t ransac_n;                 /*             4   */
  int32_t ransac_iterations;        /*             50 000 */
  int32_t reserved;
  uint64_t ransac_seed;
} rdm_eval_options;
size_t rdm_eval_pairs_workspace_bytes(int64_t num_pairs, int64_t total_corr, int64_t max_corr, const rdm_eval_options* options);
int rdm_eval_pairs(int64_t num_pairs, const int64_t* corr_offsets, const int64_t* corr_offsets_host, const float* ref_corr,
                   const float* src_corr, const float* corr_scores, const float* gt_transform, float* est_transform,
                   const int64_t* node_offsets, const int64_t* ref_node_corr, const int64_t* src_node_corr,
                   const int64_t* gt_offsets, const int64_t* gt_node_corr, const int64_t* node_dims,
                   const rdm_eval_options* options, double* records, void* ws, size_t ws_bytes, void* stream);

/* ---- §7 robust pose from correspondences: maximum clique and truncated least squares (robust.hip) ---------------------
 * The estimator experiments/eval.py:198-219 names `teaser`.  The library it calls is not part of the reference tree ->
 * parity unpinned; this is the project's own definition after the published algorithm, pinned to the
 * float64 restatement tests/robust_restatement.py.  src_corr / ref_corr: device f32 [n_corr, 3], the pose moves src onto ref;
 * n_corr <= RDM_ROBUST_MAX_CORR, above it RDM_ERR_CAPACITY.  All arithmetic is float64 on the fp32 inputs, uncontracted, every
 * sum in a fixed order, no float atomics: two calls give the same bits.
 *   (1) graph: rows i != j are adjacent iff |sqrt((dx dx + dy dy) + dz dz)(src_j - src_i) - the same of ref| <= 2 noise_bound
 *       sqrt(cbar2); a row with a non-finite value is adjacent to nothing.  degree int32[n_corr].
 *   (2) core int32[n_corr]: the k-core numbers of the graph.
 *   (3) selection: RDM_ROBUST_CLIQUE -- of all maximum cliques the one whose ascending row list is lexicographically smallest;
 *       one depth-first subproblem per lowest row, each limited to max_clique_nodes search nodes (<= 0: the default,
 *       rdm_robust_default_clique_nodes()); when a subproblem runs out, the best clique found is returned with exact = 0 (still
 *       a deterministic result).  RDM_ROBUST_KCORE -- the rows of maximum core number.  RDM_ROBUST_NONE -- all rows.
 *   (4) rotation: GNC-TLS over the pairs p < q of the K selected rows, a = src_q - src_p, b = ref_q - ref_p, n2 = (2 noise_bound)^2
 *       cbar2, weights 1 at first; per iteration R = Horn's rotation of sum w a b^T, r2 = |b - R a|^2, first iteration mu = 1 /
 *       (2 max r2 / n2 - 1) (mu <= 0: stop), th1 = (mu+1)/mu n2, th2 = mu/(mu+1) n2, cost = sum w r2 (old weights), w = 0 for
 *       r2 >= th1, 1 for r2 <= th2, else sqrt(n2 mu (mu+1) / r2) - mu; stop when |cost - previous| < cost_threshold (not on the
 *       first iteration) or after max_iterations; mu *= gnc_factor.  The device decides; the host reads one int32 per 16
 *       iterations.
 *   (5) translation, per axis: x_k = (ref_k - R src_k)[axis], c = noise_bound sqrt(cbar2), h = the sorted 2K values x_k -+ c; for
 *       every midpoint m of consecutive h: S = {k : |x_k - m| <= c} (empty: skipped), est = mean of S, cost = sum_S (x_k - est)^2
 *       + (K - |S|) c^2; the est of least cost, the lowest midpoint among equals.
 * Outputs (device): transform f64[16] row-major with bottom row 0 0 0 1 (eval.py:217 writes 1 1 1 0 there; nothing reads it);
 * stats int32[RDM_ROBUST_STATS] = {K, valid, exact, GNC iterations, translation inliers (rows within c on all three axes),
 * graph edges}; selected int32[n_corr]: the K rows ascending, then -1; weights (optional) f64[weights_capacity]: the final
 * weight of pair (p, q) of the selected rows at p K - p (p + 1) / 2 + q - p - 1 (pairs beyond the capacity are not written);
 * degree, core (optional).  K < 3: valid = 0 and the identity.  n_corr = 0 launches nothing but the output fill.            */
#define RDM_ROBUST_MAX_CORR 16384
#define RDM_ROBUST_STATS 6
enum { RDM_ROBUST_CLIQUE = 0, RDM_ROBUST_KCORE = 1, RDM_ROBUST_NONE = 2 };
int64_t rdm_robust_default_clique_nodes(void);
size_t rdm_robust_registration_workspace_bytes(int64_t n_corr, int inlier_selection);
int rdm_robust_registration(const float* src_corr, const float* ref_corr, int64_t n_corr, double noise_bound, double cbar2,
                            double gnc_factor, int max_iterations, double cost_threshold, int inlier_selection,
                            int64_t max_clique_nodes, double* transform, int32_t* stats, int32_t* selected, double* weights,
                            int64_t weights_capacity, int32_t* degree, int32_t* core, void* ws, size_t ws_bytes, void* stream);

/* ---- §7 loop-closure detection: Scan Context descriptors and exhaustive search (scan_context.hip) ----------------------
 * Kim & Kim, "Scan Context", IROS 2018.  Not in the reference tree -> parity unpinned; the project's own definition (DESIGN.md
 * section 7), pinned to the float64 restatement tests/scan_context_restatement.py.  1 <= n_rings, n_sectors <=
 * RDM_SCAN_CONTEXT_MAX_DIM; outside that every function here returns RDM_ERR_ARG (the workspace functions 0).
 * Descriptor of a cloud: D f32 [n_rings, n_sectors].  Per point, in float64 on the fp32 coordinates: r = sqrt(x x + y y); the
 * point is skipped if x, y or z is not finite, r == 0 or r > max_range; ring = min(floor(r / max_range n_rings), n_rings - 1);
 * theta = atan2(y, x) (+ 2 pi if negative), sector = min(floor(theta / (2 pi) n_sectors), n_sectors - 1); value = the fp32 sum
 * z + (float)lidar_height.  A bin holds the maximum value of its points (negative values included), 0 without a point.
 * Integer atomic max on order-preserving keys: independent of the order of the points, two calls give the same bits.
 * rdm_scan_context: points device f32 [n_points, ld >= 3]; offsets device int64 [n_scans + 1], scan s is rows
 * offsets[s] .. offsets[s + 1] (clamped to [0, n_points]; empty scans allowed); n_scans <= 65535.  Outputs (device, desc or the
 * other two may be null): desc f32 [n_scans, n_rings, n_sectors]; desc_norm f32 [n_scans, n_rings, RDM_SCAN_CONTEXT_LD]: every
 * column divided by its 2-norm (float64 sum of squares, one rounding), 0 in columns of norm 0 and in the pad columns; valid
 * uint64 [n_scans]: bit j = column j has a norm > 0.
 * Distance of descriptors Q, C: for shift n in [0, n_sectors) query column j meets candidate column (j - n) mod n_sectors;
 * d_n = 1 - (sum of the cosines of the cnt_n column pairs valid on both sides) / cnt_n, 1 when cnt_n = 0; d = min_n d_n, shift
 * = the lowest n that attains it (a query that is the candidate rotated by +a about z has shift ~ a n_sectors / 360 deg).
 * fp32: per ring the 64 products of a row are summed in column order, the ring sums are added in ring order.
 * rdm_scan_context_distance: q_desc / c_desc device f32 raw descriptors [n_q | n_c, n_rings, n_sectors] (normalised into the
 * workspace; the same pointer and count on both sides: once); n_c <= 2^26 (RDM_ERR_CAPACITY above), n_q <= 65535 x 16.
 * Query i has the global index q_base + i, candidate j c_base + j; j is eligible for i iff (q_base + i) - (c_base + j) >=
 * exclude_recent (negative: every candidate is).  best_distance f32 / best_index int32 / best_shift int32 [n_q]: the eligible
 * candidate of lowest d, the lowest candidate among equals, and its shift; (+inf, -1, -1) without an eligible candidate.
 * dist f32 / shift int32 [n_q, n_c] (both or neither; for tests and small problems): every pair, eligible or not; the best
 * values are the same bits with and without them.  No float atomics: the per-query merge is a 64-bit integer atomic min.  */
#define RDM_SCAN_CONTEXT_MAX_DIM 64
#define RDM_SCAN_CONTEXT_LD 64
size_t rdm_scan_context_workspace_bytes(int64_t n_scans, int n_rings, int n_sectors);
int rdm_scan_context(const float* points, int64_t ld, int64_t n_points, const int64_t* offsets, int64_t n_scans, int n_rings,
                     int n_sectors, double max_range, double lidar_height, float* desc, float* desc_norm, uint64_t* valid, void* ws,
                     size_t ws_bytes, void* stream);
size_t rdm_scan_context_distance_workspace_bytes(int64_t n_q, int64_t n_c, int n_rings, int n_sectors);
int rdm_scan_context_distance(const float* q_desc, int64_t n_q, const float* c_desc, int64_t n_c, int n_rings, int n_sectors,
                              int64_t q_base, int64_t c_base, int64_t exclude_recent, float* best_distance, int32_t* best_index,
                              int32_t* best_shift, float* dist, int32_t* shift, void* ws, size_t ws_bytes, void* stream);

/* ---- §7 voxel map: the scans of a sequence fused under its trajectory (voxel_map.hip) -----------------------------------
 * Not in the reference tree -> parity unpinned; the project's own definition, pinned bit for bit to the
 * NumPy restatement tests/voxel_map_restatement.py.  A map has a voxel size `voxel` (> 0), C = `channels` (3 ... 8: xyz and C - 3
 * attributes) and F = RDM_VOXEL_MAP_FRAC_BITS fractional bits.  Per point p (fp32 row) of a scan with pose X (f64 [4, 4] row-major,
 * world = X p), everything in float64 without contraction:
 *   gate      r2 = (x x + y y) + z z in the sensor frame; a row with a non-finite value among its C is counted in
 *             skipped_nonfinite, else one without min_range^2 <= r2 <= max_range^2 in skipped_range;
 *   transform w_d = ((X[d][0] x + X[d][1] y) + X[d][2] z) + X[d][3];
 *   quantise  Q_d = (int64) floor(w_d / voxel 2^F), cell_d = Q_d >> F (cell c covers [c voxel, (c + 1) voxel), anchored at the
 *             world origin); A_k = llrint(v_k 2^F) for the attributes; a point with a cell outside [-2^20, 2^20) (a non-finite w_d
 *             included) or |v_k| >= 2^20 is counted in out_of_extent;
 *   add       into the voxel of key ((cell_x + 2^20) << 42) | ((cell_y + 2^20) << 21) | (cell_z + 2^20): a uint32 count and C
 *             int64 sums of Q_d / A_k, by integer atomic adds -- the map is a function of the SET of integrated points: the order
 *             of the scans, the batching, the schedule and the run do not change one bit.  (A count wraps at 2^32 points.)
 * The map lives in ONE caller-owned device block of rdm_voxel_map_bytes(capacity, channels) bytes (0 for a bad shape): capacity
 * a power of two in [64, 2^30]; six uint64 counters {occupied, integrated, skipped_nonfinite, skipped_range, out_of_extent,
 * dropped_full}, then keys uint64 [S] (all ones = empty), counts uint32 [S], sums int64 [C][S] (each 256-byte aligned): open
 * addressing, linear probing from the home slot fmix64(key) & (S - 1) (MurmurHash3's 64-bit finaliser), 12 + 8 C bytes a slot.  Every function takes (map, map_bytes, capacity, channels) and checks them.
 * rdm_voxel_map_reset empties the map (a fresh block must be reset).  rdm_voxel_map_integrate: one launch for a packed batch --
 * points device f32 [total, ld >= C], offsets device int64 [n_scans + 1] (scan s = rows offsets[s] .. offsets[s + 1], ascending,
 * clamped to [0, total]; empty scans and n_scans = 0 are valid), poses device f64 [n_scans, 16].  The probe is bounded: a point
 * that finds neither its key nor an empty slot in one full cycle is counted in dropped_full and changes nothing else, so a key
 * is stored with all of its points or not at all (slots only go from empty to a key, so a key that found the table full finds it
 * full ever after; callers keep capacity >= 2 (occupied + batch)).  rdm_voxel_map_rehash: resets new_map (another block,
 * new_capacity >= old_capacity) and moves every occupied slot and the counters into it.  rdm_voxel_map_stats: the six counters
 * to HOST memory; waits for the stream.  rdm_voxel_map_extract: the voxels with count >= min_points in ascending key order --
 * points f32 [max_rows, C]: (float)((double)sum / (double)count / 2^F voxel) for xyz, the same without voxel for the attributes;
 * counts int32 [max_rows]; cells int32 [max_rows, 3]; *n_rows (device int64) = the number of such voxels, of which the first
 * min(*n_rows, max_rows) are written.  No float atomics and no unbounded loop anywhere.                                        */
#define RDM_VOXEL_MAP_FRAC_BITS 20
#define RDM_VOXEL_MAP_MAX_CHANNELS 8
#define RDM_VOXEL_MAP_STATS 6
size_t rdm_voxel_map_bytes(int64_t capacity, int channels);
int rdm_voxel_map_reset(void* map, size_t map_bytes, int64_t capacity, int channels, void* stream);
int rdm_voxel_map_integrate(void* map, size_t map_bytes, int64_t capacity, int channels, double voxel, const float* points, int64_t ld,
                            int64_t total, const int64_t* offsets, const double* poses, int64_t n_scans, double min_range,
                            double max_range, void* stream);
int rdm_voxel_map_rehash(const void* old_map, size_t old_bytes, int64_t old_capacity, void* new_map, size_t new_bytes,
                         int64_t new_capacity, int channels, void* stream);
int rdm_voxel_map_stats(const void* map, size_t map_bytes, int64_t capacity, int channels, uint64_t* stats, void* stream);
size_t rdm_voxel_map_extract_workspace_bytes(int64_t capacity);
int rdm_voxel_map_extract(const void* map, size_t map_bytes, int64_t capacity, int channels, double voxel, int64_t min_points,
                          float* points, int32_t* counts, int32_t* cells, int64_t max_rows, int64_t* n_rows, void* ws, size_t ws_bytes,
                          void* stream);

/* ---- §7 voxel moments: per-voxel Gaussians of the voxel map (voxel_map.hip) ---------------------------------------------------
 * Not in the reference tree -> parity unpinned; the project's own definition, pinned to the NumPy restatement
 * tests/voxel_moments_restatement.py.  For a point that the map integrates, with Q_d and cell_d as above (the same gates,
 * transform and quantisation), the local coordinate is u_d = (Q_d - (cell_d << F)) >> RDM_VOXEL_MOMENTS_SHIFT, in [0, 4096): 12
 * bits, a resolution of voxel / 4096.  The point adds RDM_VOXEL_MOMENTS_PLANES non-negative integers to its voxel, in this order:
 * u_x, u_y, u_z, u_x u_x, u_x u_y, u_x u_z, u_y u_y, u_y u_z, u_z u_z.  The sums stay below 2^56 for any uint32 count, so the int64
 * integer atomic adds are exact and the moments, like the map, depend on the SET of integrated points only.
 * A moments block is a second caller-owned device block of rdm_voxel_moments_bytes(capacity) bytes (0 for a bad capacity) beside
 * the map block: nine int64 sums per slot, addressed by the map's slot index (a slot's nine sums are 72 consecutive bytes).
 * rdm_voxel_moments_reset zeroes it (a fresh block must be reset, together with its map).  rdm_voxel_map_integrate_moments is
 * rdm_voxel_map_integrate plus the block: ONE pass, the map's own adds and the nine moment adds go into the same slot; the
 * gates, the six counters and the treatment of a full table are those of rdm_voxel_map_integrate, and a dropped point adds
 * nothing anywhere.  A map must be integrated through one of the two functions throughout.  rdm_voxel_moments_rehash runs AFTER
 * rdm_voxel_map_rehash(old_map -> new_map) on the same stream: it zeroes new_moments and, for every occupied slot of old_map,
 * looks the key up in new_map (without claiming) and copies the nine sums.  rdm_voxel_map_extract_moments: selection, order,
 * min_points, max_rows, *n_rows and the workspace (rdm_voxel_map_extract_workspace_bytes) are those of rdm_voxel_map_extract,
 * so its rows are the rows of that call; per row, in float64 with this association and no contraction:
 *   n = (double)count, m_a = S_a / n, s = voxel / 4096.0, s2 = s s, cov_ab = (S_ab / n - m_a m_b) s2
 * -- the population covariance in m^2, no clamp.  Outputs: sums int64 [max_rows, 9] (may be null), cov f64 [max_rows, 6] (xx, xy,
 * xz, yy, yz, zz), eigenvalues f64 [max_rows, 3] ascending, normals f64 [max_rows, 3]: the unit eigenvector of the smallest
 * eigenvalue, signed so that its component of largest magnitude is positive (on a tie the lowest axis decides).  The solver is a
 * float64 cyclic Jacobi with a fixed number of sweeps, one voxel per thread (the trigonometric closed form loses the small
 * eigenvalue of a planar voxel).                                                                                               */
#define RDM_VOXEL_MOMENTS_PLANES 9
#define RDM_VOXEL_MOMENTS_SHIFT 8
size_t rdm_voxel_moments_bytes(int64_t capacity);
int rdm_voxel_moments_reset(void* moments, size_t moments_bytes, int64_t capacity, void* stream);
int rdm_voxel_map_integrate_moments(void* map, size_t map_bytes, int64_t capacity, int channels, double voxel, const float* points,
                                    int64_t ld, int64_t total, const int64_t* offsets, const double* poses, int64_t n_scans,
                                    double min_range, double max_range, void* moments, size_t moments_bytes, void* stream);
int rdm_voxel_moments_rehash(const void* old_map, size_t old_bytes, int64_t old_capacity, const void* old_moments,
                             size_t old_moments_bytes, const void* new_map, size_t new_bytes, int64_t new_capacity, void* new_moments,
                             size_t new_moments_bytes, int channels, void* stream);
int rdm_voxel_map_extract_moments(const void* map, size_t map_bytes, int64_t capacity, int channels, const void* moments,
                                  size_t moments_bytes, double voxel, int64_t min_points, int64_t* sums, double* cov,
                                  double* eigenvalues, double* normals, int64_t max_rows, int64_t* n_rows, void* ws, size_t ws_bytes,
                                  void* stream);

/* ---- §7 voxel map registration: scans against the per-voxel Gaussians (voxel_map.hip) ---------------------------------------------
 * Point-to-distribution registration (the NDT / voxelised-GICP family) of a packed batch of scans against a map with moments.  Not in
 * the reference tree -> parity unpinned; the project's own definition, pinned to the NumPy restatement
 * tests/voxel_register_restatement.py.  The map and the moments block are only read.  points / offsets / poses are those of
 * rdm_voxel_map_integrate (ld >= channels; poses: the initial pose X_s of every scan).  Parameters: sigma > 0 (metres: the isotropic
 * noise of a scan point), min_points >= 1, neighbors 1 or 7, max_iteration >= 0, rot_eps >= 0, trans_eps >= 0, min_range, max_range.
 * One evaluation of scan s at the pose X = (R, t), everything in float64 without contraction:
 *   gate      each row as rdm_voxel_map_integrate does (non-finite values, then range), w = X p with its association, Q_d and cell_d
 *             by its quantisation; a point the map would count in out_of_extent is dropped;
 *   visit     the voxels cell + o for o = (0,0,0), (-1,0,0), (+1,0,0), (0,-1,0), (0,+1,0), (0,0,-1), (0,0,+1) (neighbors = 1: the
 *             first only), passing over a cell outside [-2^20, 2^20); a voxel takes part if its key is in the table and its count
 *             n >= min_points;
 *   per pair  mu_d = ((double)sum_d / n) / 2^F voxel; Sigma = the covariance of rdm_voxel_map_extract_moments (its formula, from
 *             the nine sums) + sigma^2 on the diagonal; M = Sigma^-1 (here: cofactors over the determinant); r = w - mu, q = w - t,
 *             J = [-[q]x | I3] (3 x 6, rotation first);
 *   totals    H += J^T M J, g += J^T M r, cost += r^T M r, n_corr += 1.
 * Iteration: (1) evaluate at X and record the outputs; (2) if max_iteration updates are applied, stop with status 0; (3) solve
 * H delta = -g by a float64 Cholesky without pivoting; (4) if n_corr = 0 or a pivot is <= 0 or not finite, stop with status 2
 * (degenerate: the pose is the one just evaluated); (5) else with delta = (omega, v): R <- Exp(omega) R (Rodrigues), t <- t + v --
 * a perturbation about the sensor's position, so a map far from the origin is as well conditioned as one at it; (6) if |omega| <
 * rot_eps and |v| < trans_eps, evaluate once more at the new pose and stop with status 1; (7) else continue.  The outputs always
 * describe the returned pose; max_iteration = 0 is the evaluation alone.
 * Outputs per scan (device): transforms f64 [n, 16]; hessians f64 [n, 36] (H: the information of the pose in the (omega, v)
 * parametrisation, usable as a scan-to-map edge weight); gradients f64 [n, 6]; costs f64 [n]; stats int64 [n, 4] = {updates
 * applied, n_corr, points that passed the gates, status}.  n_scans = 0 (nothing is written) and empty scans (status 2, or 0 with
 * max_iteration = 0) are valid; n_scans <= 2^20.  A null or short moments block, sigma <= 0, neighbors not 1 or 7 and negative
 * tolerances or counts are RDM_ERR_ARG; a workspace below rdm_voxel_map_register_workspace_bytes(n_scans) is RDM_ERR_WORKSPACE.
 * An iteration is two launches: a fixed number of workgroups per scan, each thread striding over rows by their index within the
 * scan and the sums reduced in a fixed order, then one workgroup per scan that adds the slab rows in index order.  No float
 * atomics: two runs give the same bits, and a scan's result does not depend on the rest of the batch, on the capacity or on the
 * order in which the map was integrated.  The host reads one word per chunk of iterations and returns when every scan stopped. */
size_t rdm_voxel_map_register_workspace_bytes(int64_t n_scans);
int rdm_voxel_map_register(const void* map, size_t map_bytes, int64_t capacity, int channels, const void* moments, size_t moments_bytes,
                           double voxel, const float* points, int64_t ld, int64_t total, const int64_t* offsets, const double* poses,
                           int64_t n_scans, double min_range, double max_range, double sigma, int64_t min_points, int neighbors,
                           int max_iteration, double rot_eps, double trans_eps, double* transforms, double* hessians, double* gradients,
                           double* costs, int64_t* stats, void* ws, size_t ws_bytes, void* stream);

/* ---- §7 voxel map registration with robust weights (voxel_map.hip) -------------------------------------------------------------------
 * rdm_voxel_map_register with one weight per point-voxel pair: the Geman-McClure weight of the pose graph's line process,
 * l = (mu / (mu + d2))^2, mu = robust_scale in units of squared Mahalanobis distance (9, about the 97 % point of chi^2 with 3 degrees
 * of freedom, is a value to start from; there is no default but off).  Not in the reference tree -> parity unpinned; the project's own
 * definition, pinned to the NumPy restatement tests/voxel_register_robust_restatement.py.  Arguments: those of
 * rdm_voxel_map_register in its order, with robust_scale after trans_eps and weight_sums (f64 [n], may be null) after costs.  Gates,
 * visit, mu_d, Sigma, M, r, q and J are rdm_voxel_map_register's, word for word.  Per pair, in float64 without contraction:
 *   d2 = r^T M r (the value the plain form adds to the cost); s = mu / (mu + d2); l = s s;
 *   H += l (J^T M J): each of the pair's 21 upper-triangle terms is multiplied by l and then added;
 *   g += l (J^T M r): each of the 6 terms is multiplied by l and then added;
 *   cost += s d2 (= mu d2 / (mu + d2); its gradient with the associations held fixed is 2 g);
 *   weight_sum += l; n_corr += 1 (every pair counts, whatever its weight).
 * Iteration, update, convergence test, statuses and outputs are those of the plain form; H, now the weighted sum, discounts the
 * outliers as the information of a scan-to-map edge too.  weight_sums[s] is the sum of l over the pairs of the returned pose: how
 * many correspondences scan s has by weight.  robust_scale = 0 is rdm_voxel_map_register bit for bit (it runs the same kernels), and
 * weight_sums, if given, then takes n_corr; rdm_voxel_map_register is this function with 0 and null.  A negative, NaN or infinite
 * robust_scale is RDM_ERR_ARG; every other error is rdm_voxel_map_register's, under its name.  The workspace is
 * rdm_voxel_map_register_workspace_bytes(n_scans).  weight_sum is one more sum of the same fixed-order reduction: no float atomics,
 * and the bit-for-bit guarantees of the plain form hold. */
int rdm_voxel_map_register_robust(const void* map, size_t map_bytes, int64_t capacity, int channels, const void* moments,
                                  size_t moments_bytes, double voxel, const float* points, int64_t ld, int64_t total,
                                  const int64_t* offsets, const double* poses, int64_t n_scans, double min_range, double max_range,
                                  double sigma, int64_t min_points, int neighbors, int max_iteration, double rot_eps, double trans_eps,
                                  double robust_scale, double* transforms, double* hessians, double* gradients, double* costs,
                                  double* weight_sums, int64_t* stats, void* ws, size_t ws_bytes, void* stream);

/* ---- §7 voxel map alignment: one map's voxel Gaussians against another's (voxel_map.hip) --------------------------------------------
 * Distribution-to-distribution registration (voxelised GICP on both sides) of a packed batch of SETS of voxel records against a map
 * with moments: what says where a map of one origin sits in the frame of another.  Not in the reference tree -> parity unpinned; the
 * project's own definition, pinned to the NumPy restatement tests/voxel_align_restatement.py.  The target (map,
 * moments block, voxel: the head of rdm_voxel_map_register) is only read.  The source is records as rdm_voxel_map_export writes
 * them, on the device: counts u32 [total], sums i64 [total, sums_ld] (sums_ld >= 3; only the first three columns are read, so a
 * state's [M, C] array is passed as it is), moment_sums i64 [total, 9], and source_voxel > 0, the edge of the grid the records were
 * taken on, which may differ from the target's voxel.  Keys are no input: the sums are absolute fixed-point world coordinates, so a
 * record's mean needs no cell.  offsets i64 [n_sets + 1] and poses f64 [n_sets, 16] are those of register's scans: set s is the
 * rows offsets[s] .. offsets[s + 1], clamped to [0, total], and poses holds its initial pose X_s (target <- source).  Parameters:
 * sigma > 0, min_points >= 1 (of a target voxel), source_min_points >= 1 (of a record), neighbors 1 or 7, max_iteration >= 0,
 * rot_eps >= 0, trans_eps >= 0.  One evaluation of set s at X = (R, t), everything in float64 without contraction:
 *   gate      a record with count < source_min_points is passed over and counted nowhere;
 *   source    n = (double)count, mu_b,d = ((double)sum_d / n) / 2^F source_voxel; Sigma_b = the covariance of
 *             rdm_voxel_map_extract_moments (its formula, from the nine sums) with source_voxel;
 *   transform w_d = ((R[d][0] mu_x + R[d][1] mu_y) + R[d][2] mu_z) + t_d; Q_d = floor(w_d / voxel 2^F) and cell_d = Q_d >> F on the
 *             TARGET's grid; a record whose w rdm_voxel_map_integrate would count in out_of_extent (non-finite included) is
 *             dropped; the others are the records that passed;
 *   visit     the 1 or 7 cells of rdm_voxel_map_register, in its order and under its rule (key present, count >= min_points);
 *   per pair  mu_a and Sigma_a as register forms them; P = R Sigma_b, C = P R^T, every entry as ((x0 + x1) + x2) over the inner
 *             index, only the six upper entries of C; cov_k = Sigma_a,k + C_k; M = (cov + sigma^2 I)^-1 (cofactors over the
 *             determinant); r = w - mu_a, q = w - t, J = [-[q]x | I3];
 *   totals    H += J^T M J, g += J^T M r, cost += r^T M r, n_corr += 1: every pair has weight one.
 * M is held fixed in the linearisation -- its dependence on R through C is not differentiated (GICP's approximation).  Iteration,
 * outputs and statuses are those of rdm_voxel_map_register, word for word: evaluate, Cholesky without pivoting, R <- Exp(omega) R,
 * t <- t + v, the one more evaluation after convergence, statuses 0 / 1 / 2; transforms f64 [n, 16], hessians f64 [n, 36], gradients
 * f64 [n, 6], costs f64 [n], stats int64 [n, 4] = {updates applied, n_corr, records that passed the gates, status}.  n_sets = 0
 * (nothing is written) and empty sets are valid; n_sets <= 2^20.  Errors are register's: RDM_ERR_ARG, by name in rdm_last_error,
 * for a null or short moments block, null counts, sums or moment_sums with total > 0, sums_ld < 3, a voxel or sigma that is not
 * positive and finite, neighbors not 1 or 7 and negative tolerances or counts; a workspace below
 * rdm_voxel_map_align_workspace_bytes(n_sets) is RDM_ERR_WORKSPACE.  The launches are register's with one other accumulate kernel
 * (row j of a set goes to thread j mod (64 x 256) of the set's threads), so again no float atomics and no unbounded loop: two runs
 * give the same bits, and a set's result does not depend on the rest of the batch, on the target's capacity or on the order in
 * which either map was integrated.                                                                                                 */
size_t rdm_voxel_map_align_workspace_bytes(int64_t n_sets);
int rdm_voxel_map_align(const void* map, size_t map_bytes, int64_t capacity, int channels, const void* moments, size_t moments_bytes,
                        double voxel, const uint32_t* counts, const int64_t* sums, int64_t sums_ld, const int64_t* moment_sums,
                        double source_voxel, int64_t total, const int64_t* offsets, const double* poses, int64_t n_sets, double sigma,
                        int64_t min_points, int64_t source_min_points, int neighbors, int max_iteration, double rot_eps,
                        double trans_eps, double* transforms, double* hessians, double* gradients, double* costs, int64_t* stats,
                        void* ws, size_t ws_bytes, void* stream);

/* ---- §7 voxel observations: in how many scans a voxel was seen, and a map without the voxels seen too rarely (voxel_map.hip) ------
 * Not in the reference tree -> parity unpinned; the project's own definition, pinned to the NumPy restatement
 * tests/voxel_observations_restatement.py.  Every integrated scan has an integer id in [0, 2^31 - 1).  A voxel OBSERVES scan s when at
 * least one point of s is integrated into it -- the gates, the transform, the quantisation and the full-table rule are those of
 * rdm_voxel_map_integrate; a skipped or dropped point observes nothing.  Per voxel: scans = the number of distinct ids observed,
 * first = the smallest and last = the largest of them.  They are a function of the SET of (id, point) pairs under one condition: all
 * points of an id come in ONE call.
 * An observations block is a third caller-owned device block of rdm_voxel_observations_bytes(capacity) bytes (0 for a bad capacity)
 * beside the map block and the (optional) moments block, addressed by the map's slot index: per slot a 64-bit scratch mask (bit s =
 * scan s of the running call was seen) and three int32 {scans, first, last}.  rdm_voxel_observations_reset: no scan seen -- scans 0,
 * first 2^31 - 1, last -1 (a fresh block must be reset, together with its map).  rdm_voxel_map_integrate_observed takes the arguments
 * of rdm_voxel_map_integrate_moments plus the block and first_id: scan s of the batch has the id first_id + s.  `moments` may be null
 * (moments_bytes is then not looked at): the one entry point of a map with and without moments.  A call carries at most
 * RDM_VOXEL_OBSERVATIONS_MAX_SCANS scans; n_scans above that, first_id < 0 or first_id + n_scans > 2^31 - 1 are RDM_ERR_ARG, a short
 * block RDM_ERR_WORKSPACE.  One sweep zeroes the masks at the start of the call, then ONE pass: the point is integrated as always, the
 * slot's mask is loaded and, if the scan's bit is clear, set by an atomic or; the one thread that got the bit clear back adds 1 to
 * scans and takes an atomic min / max on first / last.  Bits only go from 0 to 1 inside a call, so in a dense voxel almost every point
 * costs one load and no atomic.  The six counters and the map are those of the other two integrates, bit for bit.  A map must be
 * integrated through this function throughout.  rdm_voxel_observations_rehash is the counterpart of rdm_voxel_moments_rehash: AFTER
 * the map's rehash (or prune) old_map -> new_map on the same stream it resets new_observations and, for every occupied slot of
 * old_map, looks the key up in new_map (without claiming) and copies {scans, first, last}; a key that new_map lacks is passed over,
 * and the masks are not copied.  rdm_voxel_moments_rehash passes over such a key in the same way, so both serve after a prune.
 * rdm_voxel_map_extract_observations: selection, order, min_points, max_rows, *n_rows and the workspace are those of
 * rdm_voxel_map_extract, so its rows are the rows of that call; outputs int32 [max_rows] each.  rdm_voxel_map_prune: resets new_map
 * (another block, new_capacity >= old_capacity) and moves into it every occupied slot of old_map with count >= min_points and scans >=
 * min_scans; occupied = the number kept, integrated = the sum of their counts, the other four counters are copied.  The moments and
 * the observations of the kept keys follow through the two *_rehash functions.  Integer atomics only; no unbounded loop.            */
#define RDM_VOXEL_OBSERVATIONS_MAX_SCANS 64
size_t rdm_voxel_observations_bytes(int64_t capacity);
int rdm_voxel_observations_reset(void* observations, size_t observations_bytes, int64_t capacity, void* stream);
int rdm_voxel_map_integrate_observed(void* map, size_t map_bytes, int64_t capacity, int channels, double voxel, const float* points,
                                     int64_t ld, int64_t total, const int64_t* offsets, const double* poses, int64_t n_scans,
                                     double min_range, double max_range, void* moments, size_t moments_bytes, void* observations,
                                     size_t observations_bytes, int64_t first_id, void* stream);
int rdm_voxel_observations_rehash(const void* old_map, size_t old_bytes, int64_t old_capacity, const void* old_observations,
                                  size_t old_observations_bytes, const void* new_map, size_t new_bytes, int64_t new_capacity,
                                  void* new_observations, size_t new_observations_bytes, int channels, void* stream);
int rdm_voxel_map_extract_observations(const void* map, size_t map_bytes, int64_t capacity, int channels, const void* observations,
                                       size_t observations_bytes, double voxel, int64_t min_points, int32_t* scans, int32_t* first,
                                       int32_t* last, int64_t max_rows, int64_t* n_rows, void* ws, size_t ws_bytes, void* stream);
int rdm_voxel_map_prune(const void* old_map, size_t old_bytes, int64_t old_capacity, const void* old_observations,
                        size_t old_observations_bytes, void* new_map, size_t new_bytes, int64_t new_capacity, int channels,
                        int64_t min_points, int64_t min_scans, void* stream);

/* ---- §7 voxel map queries: what the map says about every point of a scan (voxel_map.hip) ---------------------------------------
 * Not in the reference tree -> parity unpinned; the project's own definition, pinned to the NumPy restatement
 * tests/voxel_query_restatement.py.  The map, the moments block and the observations block are only read.  points / ld / total /
 * offsets / poses / n_scans / min_range / max_range are those of rdm_voxel_map_register, without its limit on n_scans.  Parameters:
 * sigma > 0, min_points >= 1, neighbors 1 or 7, min_scans >= 0, max_d2 >= 0 (+inf allowed, NaN is RDM_ERR_ARG).  `moments` may be null:
 * every voxel's covariance is then zero, Sigma = sigma^2 I and d2 = |r|^2 / sigma^2.  `observations` may be null: then min_scans > 1 or
 * a non-null `seen` is RDM_ERR_ARG.  Per row i of scan s at the pose X, everything in float64 without contraction:
 *   gate      as rdm_voxel_map_integrate does: the labels RDM_VOXEL_POINT_NONFINITE, _RANGE and _EXTENT, for the rows it counts in
 *             skipped_nonfinite, skipped_range and out_of_extent;
 *   visit     the voxels cell + o, o = 0 ... neighbors - 1, in rdm_voxel_map_register's order and under its rule: a voxel takes part
 *             if its key is in the table and its count >= min_points;
 *   per voxel d2_o = r^T M r with r, Sigma = cov + sigma^2 I and M exactly as rdm_voxel_map_register forms them;
 *   best      the voxel of the smallest d2_o, ties going to the smallest o;
 *   label     no voxel took part -> _UNMAPPED; else the best voxel's scans < min_scans -> _TRANSIENT (a voxel of the table was seen
 *             in at least one scan, so min_scans <= 1 never is and does not read the block); else d2 > max_d2 -> _OFF_SURFACE; else
 *             _STATIC.
 * Outputs, all on the device and indexed by row; ANY of them may be null and is then neither computed nor written: labels u8 [total];
 * best i8 [total] (the winning o, or -1); counts i32 [total] (the best voxel's count, or 0); seen i32 [total, 3] (its {scans, first,
 * last}, or the reset values {0, 2^31 - 1, -1}); d2 f64 [total] (the best, or +inf); d2_sum f64 [total] (the sum of d2_o in ascending o,
 * or 0: its sum over a scan's rows is rdm_voxel_map_register's cost); pairs u8 [total] (how many voxels took part); tallies i64
 * [n_scans, RDM_VOXEL_QUERY_TALLIES]: per scan the number of rows of each label 0 ... 6 and, in column 7, the sum of pairs -- the call
 * zeroes it and adds one integer atomic per workgroup, scan and field after a reduction in the workgroup.  Rows outside every
 * [offsets[s], offsets[s + 1]) are left untouched; n_scans = 0 (nothing is written) and empty scans are valid.  No workspace, no float
 * atomics: a row's outputs are a function of the row, its pose and the map's contents -- not of the capacity, the order of
 * integration, the row's place in the batch or the run.  With neighbors = 1, max_d2 = +inf and neither d2 nor d2_sum wanted no
 * distance is formed: the lookup alone.                                                                                          */
#define RDM_VOXEL_POINT_NONFINITE 0
#define RDM_VOXEL_POINT_RANGE 1
#define RDM_VOXEL_POINT_EXTENT 2
#define RDM_VOXEL_POINT_UNMAPPED 3
#define RDM_VOXEL_POINT_TRANSIENT 4
#define RDM_VOXEL_POINT_OFF_SURFACE 5
#define RDM_VOXEL_POINT_STATIC 6
#define RDM_VOXEL_QUERY_TALLIES 8
int rdm_voxel_map_query(const void* map, size_t map_bytes, int64_t capacity, int channels, const void* moments, size_t moments_bytes,
                        const void* observations, size_t observations_bytes, double voxel, const float* points, int64_t ld,
                        int64_t total, const int64_t* offsets, const double* poses, int64_t n_scans, double min_range, double max_range,
                        double sigma, int64_t min_points, int neighbors, int64_t min_scans, double max_d2, uint8_t* labels,
                        int8_t* best, int32_t* counts, int32_t* seen, double* d2, double* d2_sum, uint8_t* pairs, int64_t* tallies,
                        void* stream);

/* ---- §7 voxel map state: the raw sums of a map out of the table and into another one (voxel_map.hip) ---------------------------------
 * Not in the reference tree -> parity unpinned; the project's own definition, pinned to the NumPy restatement
 * tests/voxel_state_restatement.py.  The STATE of a voxel is what the integrates have added to it, as integers: its key, its uint32
 * count, its C int64 sums and, where the map has the blocks, its nine int64 moment sums and its {scans, first, last}.  A map is a
 * function of the SET of integrated points, and every one of these is a sum (a min, a max) over that set, so the states of two maps
 * of different scans add, key by key, to the state of the map of all the scans -- bit for bit, at any capacity.
 * rdm_voxel_map_export reads the state of the voxels with count >= min_points in ascending key order.  The map and the blocks are only
 * read.  Selection, order, min_points, max_rows, *n_rows and the workspace (rdm_voxel_map_extract_workspace_bytes) are those of
 * rdm_voxel_map_extract, so its rows are the rows of that call with the same min_points.  Outputs on the device, each of which may be
 * null: keys u64 [max_rows]; counts u32 [max_rows]; sums i64 [max_rows, C] row-major; moment_sums i64 [max_rows, 9]; seen i32
 * [max_rows, 3] = {scans, first, last}.  `moments` and `observations` may be null; moment_sums (seen) must then be null too, else
 * RDM_ERR_ARG.
 * rdm_voxel_map_import adds n_records records of that layout (device arrays) into a map.  moment_sums is required if and only if the
 * map has a moments block (`moments` not null) -- records that carry moments go into a map without the block with moment_sums null --
 * and seen if and only if it has an observations block; anything else is RDM_ERR_ARG, as are id_offset < 0 and a null n_rejected.
 * n_records = 0 is valid.  One launch, one thread per record:
 *   reject    a record whose key has bit 63 set (the empty marker included), whose count is 0 or, where seen is given, whose record
 *             is not 1 <= scans <= last - first + 1 with 0 <= first <= last <= 2^31 - 2 - id_offset, changes nothing and is counted
 *             in the device word *n_rejected (int64), which the call zeroes first;
 *   claim     the slot of the key by integrate's bounded probe; a record that finds neither its key nor an empty slot in one full
 *             cycle adds its count to dropped_full and nothing else -- a key is stored with all of its records or not at all, by
 *             integrate's argument --; a fresh claim adds 1 to occupied;
 *   add       count to the slot's count (it wraps at 2^32, as the map's counts do) and to integrated, the C sums, the nine moment
 *             sums, scans to scans, and first + id_offset / last + id_offset by an atomic min / max.  Integer atomics throughout: two
 *             records of one batch may hold the same key.  The observation masks are scratch of integrate and are not touched.
 * skipped_host (HOST memory, may be null): four uint64 that are added to skipped_nonfinite, skipped_range, out_of_extent and
 * dropped_full, so that the six counters of a merged map are those of the map built in one pass.
 * Condition: the records' scans are scans other than those already in the map -- after id_offset their ids are disjoint from the
 * map's; `scans` adds only then (count, the sums, first and last hold regardless).
 * Property: without drops, the contents of the table as rdm_voxel_map_export shows them are a function of the contents before and of
 * the multiset of records: not of their order, the batching, the capacity or the run.  No float anywhere, no unbounded loop and no
 * workspace.                                                                                                                        */
int rdm_voxel_map_export(const void* map, size_t map_bytes, int64_t capacity, int channels, const void* moments, size_t moments_bytes,
                         const void* observations, size_t observations_bytes, int64_t min_points, uint64_t* keys, uint32_t* counts,
                         int64_t* sums, int64_t* moment_sums, int32_t* seen, int64_t max_rows, int64_t* n_rows, void* ws, size_t ws_bytes,
                         void* stream);
int rdm_voxel_map_import(void* map, size_t map_bytes, int64_t capacity, int channels, void* moments, size_t moments_bytes,
                         void* observations, size_t observations_bytes, const uint64_t* keys, const uint32_t* counts, const int64_t* sums,
                         const int64_t* moment_sums, const int32_t* seen, int64_t n_records, int64_t id_offset,
                         const uint64_t* skipped_host, int64_t* n_rejected, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDMNET_HIP_H_ */
