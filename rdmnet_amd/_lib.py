"""ctypes loader for librdmnet_hip.so.  There is no CPU fallback: a missing library or a failing
call raises."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('RDM_LIB_PATH') or os.path.join(_HERE, 'librdmnet_hip.so')  # override: A/B builds

c_void = ctypes.c_void_p
c_i64 = ctypes.c_int64
c_int = ctypes.c_int
c_f32 = ctypes.c_float
c_size = ctypes.c_size_t

ABI_VERSION = 2  # = RDM_ABI_VERSION of include/rdmnet_hip.h this binding was written against


class FineMatchingOptions(ctypes.Structure):
    """rdm_fine_matching_options (include/rdmnet_hip.h); correspondence_limit 0 = none."""
    _fields_ = [('topk', ctypes.c_int32), ('mutual', ctypes.c_int32), ('use_dustbin', ctypes.c_int32),
                ('use_global_score', ctypes.c_int32), ('confidence_threshold', ctypes.c_float),
                ('correspondence_limit', ctypes.c_int32)]

    @classmethod
    def of(cls, topk=1, mutual=False, use_dustbin=True, confidence_threshold=0.0, use_global_score=False,
           correspondence_limit=None):
        return cls(int(topk), int(bool(mutual)), int(bool(use_dustbin)), int(bool(use_global_score)), float(confidence_threshold),
                   0 if correspondence_limit is None else int(correspondence_limit))


class EvalOptions(ctypes.Structure):
    """rdm_eval_options (include/rdmnet_hip.h); num_corr 0 = every correspondence."""
    METHODS = {'lgr': 0, 'svd': 1, 'ransac': 2}
    _fields_ = [('method', ctypes.c_int32), ('num_corr', ctypes.c_int32), ('acceptance_radius', ctypes.c_double),
                ('ransac_distance_threshold', ctypes.c_float), ('ransac_n', ctypes.c_int32),
                ('ransac_iterations', ctypes.c_int32), ('reserved', ctypes.c_int32), ('ransac_seed', ctypes.c_uint64)]

    @classmethod
    def of(cls, method='lgr', num_corr=None, acceptance_radius=0.6, distance_threshold=0.3, ransac_n=4, num_iterations=50000,
           seed=0):
        if method not in cls.METHODS:
            raise ValueError(f'Unsupported registration method: {method}.')
        return cls(cls.METHODS[method], 0 if num_corr is None else int(num_corr), float(acceptance_radius),
                   float(distance_threshold), int(ransac_n), int(num_iterations), 0, int(seed))


ROBUST_SELECTIONS = {'clique': 0, 'kcore': 1, 'none': 2}  # RDM_ROBUST_*
ROBUST_MAX_CORR = 16384  # = RDM_ROBUST_MAX_CORR
ROBUST_STATS = ('num_selected', 'valid', 'exact', 'iterations', 'translation_inliers', 'edges')  # rdm_robust_registration's stats

SCAN_CONTEXT_MAX_DIM = 64  # = RDM_SCAN_CONTEXT_MAX_DIM: n_rings, n_sectors <= this
SCAN_CONTEXT_LD = 64  # = RDM_SCAN_CONTEXT_LD: columns of a row of the normalised descriptors

VOXEL_MAP_FRAC_BITS = 20  # = RDM_VOXEL_MAP_FRAC_BITS
VOXEL_MAP_MAX_CHANNELS = 8  # = RDM_VOXEL_MAP_MAX_CHANNELS
# rdm_voxel_map_stats' counters, in order (RDM_VOXEL_MAP_STATS of them)
VOXEL_MAP_STATS = ('occupied', 'integrated', 'skipped_nonfinite', 'skipped_range', 'out_of_extent', 'dropped_full')
VOXEL_MOMENTS_PLANES = 9  # = RDM_VOXEL_MOMENTS_PLANES: u_x, u_y, u_z, then u_a u_b for ab = xx, xy, xz, yy, yz, zz
VOXEL_MOMENTS_SHIFT = 8  # = RDM_VOXEL_MOMENTS_SHIFT
VOXEL_OBSERVATIONS_MAX_SCANS = 64  # = RDM_VOXEL_OBSERVATIONS_MAX_SCANS: scans of one rdm_voxel_map_integrate_observed call
# rdm_voxel_map_query's labels, in the order of their codes RDM_VOXEL_POINT_*
VOXEL_POINT_LABELS = ('nonfinite', 'range', 'extent', 'unmapped', 'transient', 'off_surface', 'static')
VOXEL_QUERY_TALLIES = 8  # = RDM_VOXEL_QUERY_TALLIES: a scan's rows per label, then its pairs

EVAL_RECORD_WIDTH = 20 # = RDM_EVAL_RECORD_WIDTH
# the fields of one record of rdm_eval_pairs, in order
EVAL_FIELDS = ('num_corr', 'residual', 'inlier_ratio', 'inlier_ratio_0.3', 'inlier_ratio_0.1', 'overlap', 'precision', 'rre', 'rte',
               'rx', 'ry', 'rz', 'inliers', 'inliers_0.3', 'inliers_0.1', 'overlap_rows', 'hit_cells', 'pred_cells', 'gt_cells',
               'bad_indices')

# name -> (restype, argtypes); mirrors include/rdmnet_hip.h one to one
SIGNATURES = {
    'rdm_abi_version': (c_int, []),
    'rdm_abi_struct_size': (c_size, [c_int]),
    'rdm_last_error': (ctypes.c_char_p, []),
    'rdm_rehash_schedule': (c_int, [c_i64, c_void, c_void, c_int]),
    'rdm_grid_subsample_workspace_bytes': (c_size, [c_i64, c_int]),
    'rdm_grid_subsample': (c_int, [c_void, c_i64, c_void, c_int, c_f32, c_void, c_void, c_void, c_size,
                                   c_void]),
    'rdm_grid_subsample_form': (c_int, [c_void, c_i64, c_void, c_int, c_f32, c_void, c_void, c_void, c_size,
                                        c_void, c_int]),
    'rdm_radius_neighbors_workspace_bytes': (c_size, [c_i64, c_i64, c_int]),
    'rdm_radius_neighbors': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_void, c_int, c_f32, c_int,
                                     c_void, c_void, c_void, c_void, c_void, c_size, c_void]),
    'rdm_radius_grid_workspace_bytes': (c_size, [c_i64]),
    'rdm_radius_grid_build': (c_int, [c_void, c_i64, c_void, c_int, c_f32, c_void, c_size, c_void]),
    'rdm_radius_grid_query': (c_int, [c_void, c_size, c_i64, c_void, c_i64, c_void, c_int, c_f32, c_int, c_void, c_void,
                                      c_void, c_void, c_void, c_size, c_void]),
    'rdm_gemm_workspace_bytes': (c_size, [c_i64, c_i64, c_int]),
    'rdm_gemm': (c_int, [c_void, c_i64, c_i64, c_void, c_i64, c_i64, c_int, c_void, c_i64, c_i64, c_i64, c_i64,
                         c_i64, c_int, c_void, c_void, c_int, c_void, c_size, c_void]),
    'rdm_gemm_last_plan': (c_int, [c_void]),
    'rdm_kpconv_gather': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_i64, c_i64, c_void, c_void, c_i64,
                                  c_i64, c_void, c_void, c_f32, c_void, c_i64, c_void, c_void]),
    'rdm_kpconv_gather_ordered': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_i64, c_i64, c_void, c_void, c_i64,
                                          c_i64, c_void, c_void, c_f32, c_void, c_i64, c_void, c_void, c_void]),
    'rdm_kpconv_gather_form': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_i64, c_i64, c_void, c_void, c_i64,
                                       c_i64, c_void, c_void, c_f32, c_void, c_i64, c_void, c_void, c_int, c_void]),
    'rdm_kpconv_fused_enabled': (c_int, []),
    'rdm_kpconv_fused_supported': (c_int, [c_i64, c_i64]),
    'rdm_kpconv_fused_partial_rows': (c_i64, [c_i64, c_i64]),
    'rdm_kpconv_packed_floats': (c_size, [c_i64, c_i64]),
    'rdm_kpconv_pack_weights': (c_int, [c_void, c_i64, c_i64, c_void]),
    'rdm_kpconv_fused': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_i64, c_i64, c_void, c_void, c_i64, c_i64, c_void, c_void,
                                 c_f32, c_void, c_void, c_i64, c_void, c_i64, c_void, c_void, c_void]),
    'rdm_kpconv_fused_form': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_i64, c_i64, c_void, c_void, c_i64, c_i64, c_void, c_void,
                                      c_f32, c_void, c_void, c_i64, c_void, c_i64, c_void, c_void, c_int, c_void]),
    'rdm_kpconv_fused_workspace_bytes': (c_size, [c_i64, c_i64, c_i64]),
    'rdm_kpconv_fused_group_norm': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_i64, c_i64, c_void, c_void, c_i64, c_i64, c_void,
                                            c_void, c_f32, c_void, c_void, c_i64, c_int, c_void, c_void, c_f32, c_int, c_void, c_i64,
                                            c_void, c_i64, c_void, c_size, c_void, c_void]),
    'rdm_voxel_downsample_workspace_bytes': (c_size, [c_i64]),
    'rdm_voxel_downsample': (c_int, [c_void, c_i64, c_i64, c_int, ctypes.c_double, c_void, c_i64, c_void, c_void, c_void,
                                     c_size, c_void]),
    'rdm_ransac_workspace_bytes': (c_size, [c_int]),
    'rdm_ransac_correspondences': (c_int, [c_void, c_void, c_i64, c_f32, c_int, c_int, ctypes.c_uint64, c_void, c_void, c_void,
                                           c_void, c_void, c_size, c_void]),
    'rdm_icp_workspace_bytes': (c_size, [c_i64, c_i64]),
    'rdm_icp_point_to_point': (c_int, [c_void, c_i64, c_i64, c_void, c_i64, c_i64, ctypes.c_double, c_void, c_int, ctypes.c_double,
                                       ctypes.c_double, c_void, c_void, c_void, c_void, c_void, c_size, c_void]),
    'rdm_icp_correspondences': (c_int, [c_void, c_i64, c_void, c_i64, c_i64, ctypes.c_double, c_void, c_void, c_void, c_size,
                                        c_void]),
    'rdm_ball_workspace_bytes': (c_size, [c_i64, c_i64]),
    'rdm_ball_count': (c_int, [c_void, c_i64, c_i64, c_void, c_i64, c_i64, c_void, ctypes.c_double, c_void, c_void, c_void, c_void,
                               c_void, c_size, c_void]),
    'rdm_ball_fill': (c_int, [c_void, c_i64, c_i64, c_i64, c_void, c_i64, c_void, c_size, c_void]),
    'rdm_nearest_workspace_bytes': (c_size, [c_i64, c_i64]),
    'rdm_nearest': (c_int, [c_void, c_i64, c_i64, c_void, c_i64, c_i64, c_void, c_void, ctypes.c_double, ctypes.c_double, c_void,
                            c_void, c_void, c_void, c_size, c_void]),
    'rdm_realign_error': (c_int, [c_void, c_i64, c_i64, c_void, c_void, c_void, c_void, c_size, c_void]),
    'rdm_information_workspace_bytes': (c_size, [c_i64, c_i64]),
    'rdm_information_matrix': (c_int, [c_void, c_i64, c_i64, c_void, c_i64, c_i64, c_void, c_void, ctypes.c_double, ctypes.c_double,
                                       c_void, c_void, c_i64, c_void, c_size, c_void]),
    'rdm_pose_graph_workspace_bytes': (c_size, [c_i64, c_i64, c_i64]),
    'rdm_pose_graph_optimize': (c_int, [c_i64, c_void, c_void, c_void, c_void, c_void, c_void, c_void, ctypes.c_double, ctypes.c_double,
                                        c_int, ctypes.c_double, ctypes.c_double, c_int, ctypes.c_double, c_void, c_void, c_void, c_void,
                                        c_void, c_size, c_void]),
    'rdm_pose_graph_workspace_bytes_pc': (c_size, [c_i64, c_i64, c_i64, c_int]),
    'rdm_pose_graph_optimize_pc': (c_int, [c_i64, c_void, c_void, c_void, c_void, c_void, c_void, c_void, ctypes.c_double,
                                           ctypes.c_double, c_int, ctypes.c_double, ctypes.c_double, c_int, ctypes.c_double, c_int,
                                           c_void, c_void, c_void, c_void, c_void, c_size, c_void]),
    'rdm_pose_graph_chain_host': (c_int, [c_i64, c_void, c_void, c_void, c_void]),
    'rdm_pose_graph_workspace_bytes_ls': (c_size, [c_i64, c_void, c_void, c_void, c_int, c_int]),
    'rdm_pose_graph_optimize_ls': (c_int, [c_i64, c_void, c_void, c_void, c_void, c_void, c_void, c_void, ctypes.c_double,
                                           ctypes.c_double, c_int, ctypes.c_double, ctypes.c_double, c_int, ctypes.c_double, c_int, c_int,
                                           c_void, c_void, c_void, c_void, c_void, c_size, c_void]),
    'rdm_pose_graph_direct_max_separator': (c_int, []),
    'rdm_pose_graph_separator_host': (c_i64, [c_i64, c_i64, c_void, c_void, c_i64]),
    'rdm_pose_graph_direct_host': (c_int, [c_i64, c_i64, c_void, c_void, c_void, c_void, c_void]),
    'rdm_pose_graph_marginals_workspace_bytes': (c_size, [c_i64, c_void, c_void, c_void]),
    'rdm_pose_graph_marginals': (c_int, [c_i64, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_size,
                                         c_void]),
    'rdm_pose_graph_marginals_host': (c_int, [c_i64, c_i64, c_void, c_void, c_void, c_void]),
    'rdm_dbg_pose_graph_marginals_ticks': (c_int, [c_void]),
    'rdm_pose_graph_consistency_workspace_bytes': (c_size, [c_i64, c_void, c_void, c_void, c_void, c_void]),
    'rdm_pose_graph_consistency': (c_int, [c_i64, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void,
                                           c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_size, c_void]),
    'rdm_pose_graph_pair_covariances_host': (c_int, [c_i64, c_i64, c_void, c_void, c_void, c_i64, c_void, c_void]),
    'rdm_pose_graph_pair_terms_host': (c_int, [c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void]),
    'rdm_pose_graph_edge_terms_host': (c_int, [c_void, c_void, c_void, c_void, ctypes.c_double, c_int, c_void]),
    'rdm_pose_graph_retract_host': (c_int, [c_void, c_void, c_void]),
    'rdm_neighbor_histogram': (c_int, [c_void, c_i64, c_void, c_int, c_void]),
    'rdm_radius_grid_records': (c_void, [c_void, c_size, c_i64]),
    'rdm_row_positive': (c_int, [c_void, c_i64, c_i64, c_i64, c_void, c_void]),
    'rdm_group_norm_workspace_bytes': (c_size, [c_i64, c_i64]),
    'rdm_group_norm': (c_int, [c_void, c_i64, c_i64, c_i64, c_int, c_void, c_void, c_f32, c_void, c_i64, c_int,
                               c_void, c_i64, c_void, c_void, c_size, c_void]),
    'rdm_group_norm_form': (c_int, [c_void, c_i64, c_i64, c_i64, c_int, c_void, c_void, c_f32, c_void, c_i64, c_int,
                                    c_void, c_i64, c_void, c_void, c_size, c_int, c_void]),
    'rdm_linear_group_norm_workspace_bytes': (c_size, [c_i64, c_i64]),
    'rdm_linear_group_norm': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_void, c_i64, c_i64, c_i64, c_int, c_void, c_void,
                                      c_f32, c_void, c_i64, c_int, c_void, c_i64, c_void, c_i64, c_void, c_void, c_size, c_void]),
    'rdm_patch_scores': (c_int, [c_void, c_i64, c_i64, c_void, c_void, c_i64, c_i64, c_void, c_i64, c_i64, c_i64, c_void, c_void,
                                 c_void]),
    'rdm_decoder_stage_workspace_bytes': (c_size, [c_i64, c_i64, c_i64]),
    'rdm_decoder_stage': (c_int, [c_void, c_i64, c_i64, c_i64, c_void, c_i64, c_void, c_i64, c_i64, c_i64, c_void, c_i64, c_void,
                                  c_i64, c_int, c_void, c_void, c_f32, c_int, c_void, c_i64, c_void, c_i64, c_void, c_size, c_void]),
    'rdm_layer_norm': (c_int, [c_void, c_i64, c_i64, c_i64, c_void, c_i64, c_void, c_void, c_f32, c_int, c_void,
                               c_i64, c_void]),
    'rdm_linear_layer_norm': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_i64, c_i64, c_i64, c_void, c_i64, c_void, c_void,
                                      c_f32, c_int, c_void, c_i64, c_void]),
    'rdm_attention_tail': (c_int, [c_void, c_i64, c_void, c_i64, c_i64, c_i64, c_void, c_i64, c_void, c_void, c_void, c_void, c_i64,
                                   c_void, c_void, c_i64, c_void, c_void, c_void, c_f32, c_void, c_i64, c_void]),
    'rdm_attention_tail_packed_floats': (c_size, []),
    'rdm_attention_tail_pack_weights': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_i64, c_void, c_void]),
    'rdm_attention_tail_packed': (c_int, [c_void, c_i64, c_void, c_i64, c_i64, c_i64, c_void, c_void, c_void, c_void, c_void, c_void,
                                          c_void, c_void, c_f32, c_void, c_i64, c_void]),
    'rdm_gather_max': (c_int, [c_void, c_i64, c_i64, c_i64, c_void, c_i64, c_i64, c_i64, c_void, c_void, c_i64,
                               c_void]),
    'rdm_upsample_concat': (c_int, [c_void, c_i64, c_i64, c_i64, c_void, c_i64, c_void, c_i64, c_i64, c_i64,
                                    c_void, c_i64, c_void]),
    'rdm_gather_rows': (c_int, [c_void, c_i64, c_i64, c_i64, c_void, c_i64, c_void, c_i64, c_void]),
    'rdm_rope': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_i64, c_i64, c_i64, c_void]),
    'rdm_attention': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_i64, c_void, c_i64, c_i64, c_i64, c_int, c_int,
                              c_void]),
    'rdm_attention_bf16': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_i64, c_void, c_i64, c_i64, c_i64, c_int, c_int,
                              c_void]),
    'rdm_attention_self_pair': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_i64, c_void, c_i64, c_i64, c_i64, c_int, c_int,
                                        c_int, c_void]),
    'rdm_attention_topk': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_i64, c_void, c_i64, c_i64, c_i64, c_i64, c_int, c_int,
                                   c_void]),
    'rdm_attention_self_pair_topk': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_i64, c_void, c_i64, c_i64, c_i64, c_i64, c_i64,
                                             c_int, c_int, c_void]),
    'rdm_topk_count': (c_i64, [c_i64, ctypes.c_double]),
    'rdm_vote_shift': (c_int, [c_void, c_void, c_i64, c_i64, c_f32, c_f32, c_f32, c_void, c_void]),
    'rdm_sigmoid_column': (c_int, [c_void, c_i64, c_i64, c_void, c_void]),
    'rdm_l2_normalize': (c_int, [c_void, c_i64, c_i64, c_i64, c_void, c_i64, c_void]),
    'rdm_nms': (c_int, [c_void, c_i64, c_i64, c_i64, c_void, c_void, c_void]),
    'rdm_compact_indices': (c_int, [c_void, c_i64, c_i64, c_void, c_void, c_void]),
    'rdm_point_to_node_workspace_bytes': (c_size, [c_i64, c_i64]),
    'rdm_point_to_node': (c_int, [c_void, c_i64, c_void, c_i64, c_int, c_void, c_void, c_void, c_void, c_void,
                                  c_size, c_void]),
    'rdm_point_to_node_pair': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_i64, c_void, c_i64, c_int, c_void, c_void, c_void,
                                       c_void, c_void, c_void, c_void, c_void, c_size, c_void]),
    'rdm_coarse_matching_workspace_bytes': (c_size, [c_i64, c_i64]),
    'rdm_coarse_matching': (c_int, [c_void, c_i64, c_i64, c_i64, c_void, c_void, c_int, c_int, c_void, c_void, c_void,
                                    c_void, c_void, c_size, c_void]),
    'rdm_coarse_matching_features_workspace_bytes': (c_size, [c_i64, c_i64]),
    'rdm_coarse_matching_features': (c_int, [c_void, c_i64, c_i64, c_void, c_i64, c_i64, c_i64, c_void, c_void, c_int, c_int,
                                             c_void, c_void, c_void, c_void, c_void, c_size, c_void]),
    'rdm_gt_node_correspondences_workspace_bytes': (c_size, [c_i64, c_i64]),
    'rdm_gt_node_correspondences': (c_int, [c_void, c_i64, c_void, c_i64, c_void, c_void, c_i64, c_void, c_void, c_i64, c_int,
                                            c_void, c_void, c_void, c_void, c_void, ctypes.c_double, c_void, c_void, c_i64,
                                            c_void, c_void, c_void, c_size, c_void]),
    'rdm_sinkhorn': (c_int, [c_void, c_i64, c_i64, c_i64, c_void, c_void, c_void, c_int, c_void, c_void]),
    'rdm_lgr_workspace_bytes': (c_size, [c_i64]),
    'rdm_lgr': (c_int, [c_void, c_void, c_void, c_void, c_void, c_i64, c_i64, c_f32, c_int, c_int, c_void, c_void,
                        c_void, c_void, c_void, c_void, c_size, c_void]),
    'rdm_lgr_options_capacity': (c_i64, [c_i64, c_i64, c_void]),
    'rdm_lgr_options_workspace_bytes': (c_size, [c_i64, c_i64, c_void]),
    'rdm_lgr_options': (c_int, [c_void, c_i64, c_void, c_void, c_void, c_void, c_void, c_i64, c_i64, c_f32, c_int, c_int, c_void,
                                c_void, c_void, c_void, c_void, c_void, c_void, c_size, c_void]),
    'rdm_engine_create': (c_int, [c_void, c_void]),
    'rdm_engine_destroy': (None, [c_void]),
    'rdm_engine_set_param': (c_int, [c_void, ctypes.c_char_p, c_void, c_void, c_int]),
    'rdm_engine_finalize': (c_int, [c_void]),
    'rdm_engine_share_params': (c_int, [c_void, c_void]),
    'rdm_engine_run': (c_int, [c_void, c_void, c_i64, c_void, c_i64, c_void, c_void]),
    'rdm_engine_collate': (c_int, [c_void, c_void, c_i64, c_void, c_i64, c_void, c_void]),
    'rdm_engine_forward': (c_int, [c_void, c_void, c_void, c_void]),
    'rdm_engine_collate_batch': (c_int, [c_void, c_int, c_void, c_void, c_void, c_void, c_void]),
    'rdm_engine_forward_batched': (c_int, [c_void, c_int, c_void, c_void]),
    'rdm_engine_run_lockstep': (c_int, [c_void, c_int, c_void, c_void, c_void, c_void, c_void, c_int, c_void]),
    'rdm_engine_forward_lockstep': (c_int, [c_void, c_int, c_void, c_void, c_void]),
    'rdm_engine_collate_lockstep': (c_int, [c_void, c_int, c_void, c_void, c_void, c_void, c_void, c_void]),
    'rdm_lockstep_stats': (None, [c_void, c_int]),
    'rdm_lockstep_stats_dump': (None, []),
    'rdm_lockstep_selftest': (c_int, [c_int, c_void, c_int, c_void, c_int, c_void]),
    'rdm_lockstep_selftest_gpu': (c_int, [c_int, c_void, c_int, c_int, c_void, c_i64, c_void]),
    'rdm_engine_reserve': (c_int, [c_void, c_size]),
    'rdm_engine_set_wait': (c_int, [c_void, c_int]),
    'rdm_engine_set_pairs_in_flight': (c_int, [c_void, c_int]),
    'rdm_engine_set_overlap': (c_int, [c_void, c_int]),
    'rdm_engine_set_attention_topk': (c_int, [c_void, c_int, c_void]),
    'rdm_engine_set_fine_matching': (c_int, [c_void, c_void]),
    'rdm_engine_enable_profile': (c_int, [c_void, c_int]),
    'rdm_engine_get_profile': (c_int, [c_void, c_void, c_int]),
    'rdm_engine_keep_taps': (c_int, [c_void, c_int]),
    'rdm_engine_get_tensor': (c_int, [c_void, ctypes.c_char_p, c_void]),
    'rdm_engine_describe': (c_int, [c_void, c_int, c_void, c_void]),
    'rdm_engine_export': (c_int, [c_void, c_int, c_void, c_void, c_void]),
    'rdm_engine_gt_node_correspondences': (c_int, [c_void, c_void, ctypes.c_double, c_void, c_void, c_i64, c_void, c_void]),
    'rdm_feature_match_workspace_bytes': (c_size, [c_i64, c_i64, c_int]),
    'rdm_feature_match': (c_int, [c_void, c_i64, c_i64, c_void, c_i64, c_i64, c_i64, c_int, c_void, c_void, c_void, c_void, c_void,
                                  c_void, c_size, c_void]),
    'rdm_feature_match_select': (c_int, [c_int, c_void, c_void, c_void, c_void, c_i64, c_i64, c_void, c_void, c_void, c_void, c_void]),
    'rdm_engine_feature_correspondences': (c_int, [c_void, c_int, c_int, c_void, c_void, c_void, c_void, c_void, c_i64, c_void,
                                                   c_void]),
    'rdm_engine_gt_point_correspondences_count': (c_int, [c_void, c_int, c_void, ctypes.c_double, c_void, c_void]),
    'rdm_engine_gt_point_correspondences_fill': (c_int, [c_void, c_void, c_i64, c_void]),
    'rdm_engine_alignment_quality': (c_int, [c_void, c_int, c_void, ctypes.c_double, c_void, c_void]),
    'rdm_engine_information_matrix': (c_int, [c_void, c_int, c_void, ctypes.c_double, c_void, c_void, c_i64, c_void]),
    'rdm_copy_device': (c_int, [c_void, c_void, c_size, c_void]),
    'rdm_eval_pairs_workspace_bytes': (c_size, [c_i64, c_i64, c_i64, c_void]),
    'rdm_eval_pairs': (c_int, [c_i64, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void,
                               c_void, c_void, c_void, c_void, c_void, c_size, c_void]),
    'rdm_robust_default_clique_nodes': (c_i64, []),
    'rdm_robust_registration_workspace_bytes': (c_size, [c_i64, c_int]),
    'rdm_robust_registration': (c_int, [c_void, c_void, c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_int,
                                        ctypes.c_double, c_int, c_i64, c_void, c_void, c_void, c_void, c_i64, c_void, c_void,
                                        c_void, c_size, c_void]),
    'rdm_scan_context_workspace_bytes': (c_size, [c_i64, c_int, c_int]),
    'rdm_scan_context': (c_int, [c_void, c_i64, c_i64, c_void, c_i64, c_int, c_int, ctypes.c_double, ctypes.c_double, c_void, c_void,
                                 c_void, c_void, c_size, c_void]),
    'rdm_scan_context_distance_workspace_bytes': (c_size, [c_i64, c_i64, c_int, c_int]),
    'rdm_scan_context_distance': (c_int, [c_void, c_i64, c_void, c_i64, c_int, c_int, c_i64, c_i64, c_i64, c_void, c_void, c_void,
                                          c_void, c_void, c_void, c_size, c_void]),
    'rdm_voxel_map_bytes': (c_size, [c_i64, c_int]),
    'rdm_voxel_map_reset': (c_int, [c_void, c_size, c_i64, c_int, c_void]),
    'rdm_voxel_map_integrate': (c_int, [c_void, c_size, c_i64, c_int, ctypes.c_double, c_void, c_i64, c_i64, c_void, c_void, c_i64,
                                        ctypes.c_double, ctypes.c_double, c_void]),
    'rdm_voxel_map_rehash': (c_int, [c_void, c_size, c_i64, c_void, c_size, c_i64, c_int, c_void]),
    'rdm_voxel_map_stats': (c_int, [c_void, c_size, c_i64, c_int, c_void, c_void]),
    'rdm_voxel_map_extract_workspace_bytes': (c_size, [c_i64]),
    'rdm_voxel_map_extract': (c_int, [c_void, c_size, c_i64, c_int, ctypes.c_double, c_i64, c_void, c_void, c_void, c_i64, c_void,
                                      c_void, c_size, c_void]),
    'rdm_voxel_moments_bytes': (c_size, [c_i64]),
    'rdm_voxel_moments_reset': (c_int, [c_void, c_size, c_i64, c_void]),
    'rdm_voxel_map_integrate_moments': (c_int, [c_void, c_size, c_i64, c_int, ctypes.c_double, c_void, c_i64, c_i64, c_void, c_void,
                                                c_i64, ctypes.c_double, ctypes.c_double, c_void, c_size, c_void]),
    'rdm_voxel_moments_rehash': (c_int, [c_void, c_size, c_i64, c_void, c_size, c_void, c_size, c_i64, c_void, c_size, c_int, c_void]),
    'rdm_voxel_map_extract_moments': (c_int, [c_void, c_size, c_i64, c_int, c_void, c_size, ctypes.c_double, c_i64, c_void, c_void,
                                              c_void, c_void, c_i64, c_void, c_void, c_size, c_void]),
    'rdm_voxel_map_register_workspace_bytes': (c_size, [c_i64]),
    'rdm_voxel_map_register': (c_int, [c_void, c_size, c_i64, c_int, c_void, c_size, ctypes.c_double, c_void, c_i64, c_i64, c_void, c_void,
                                       c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_i64, c_int, c_int, ctypes.c_double,
                                       ctypes.c_double, c_void, c_void, c_void, c_void, c_void, c_void, c_size, c_void]),
    'rdm_voxel_map_register_robust': (c_int, [c_void, c_size, c_i64, c_int, c_void, c_size, ctypes.c_double, c_void, c_i64, c_i64, c_void,
                                              c_void, c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_i64, c_int, c_int,
                                              ctypes.c_double, ctypes.c_double, ctypes.c_double, c_void, c_void, c_void, c_void, c_void,
                                              c_void, c_void, c_size, c_void]),
    'rdm_voxel_map_align_workspace_bytes': (c_size, [c_i64]),
    'rdm_voxel_map_align': (c_int, [c_void, c_size, c_i64, c_int, c_void, c_size, ctypes.c_double, c_void, c_void, c_i64, c_void,
                                    ctypes.c_double, c_i64, c_void, c_void, c_i64, ctypes.c_double, c_i64, c_i64, c_int, c_int,
                                    ctypes.c_double, ctypes.c_double, c_void, c_void, c_void, c_void, c_void, c_void, c_size, c_void]),
    'rdm_voxel_observations_bytes': (c_size, [c_i64]),
    'rdm_voxel_observations_reset': (c_int, [c_void, c_size, c_i64, c_void]),
    'rdm_voxel_map_integrate_observed': (c_int, [c_void, c_size, c_i64, c_int, ctypes.c_double, c_void, c_i64, c_i64, c_void, c_void,
                                                 c_i64, ctypes.c_double, ctypes.c_double, c_void, c_size, c_void, c_size, c_i64, c_void]),
    'rdm_voxel_observations_rehash': (c_int, [c_void, c_size, c_i64, c_void, c_size, c_void, c_size, c_i64, c_void, c_size, c_int, c_void]),
    'rdm_voxel_map_extract_observations': (c_int, [c_void, c_size, c_i64, c_int, c_void, c_size, ctypes.c_double, c_i64, c_void, c_void,
                                                   c_void, c_i64, c_void, c_void, c_size, c_void]),
    'rdm_voxel_map_prune': (c_int, [c_void, c_size, c_i64, c_void, c_size, c_void, c_size, c_i64, c_int, c_i64, c_i64, c_void]),
    'rdm_voxel_map_query': (c_int, [c_void, c_size, c_i64, c_int, c_void, c_size, c_void, c_size, ctypes.c_double, c_void, c_i64, c_i64,
                                    c_void, c_void, c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_i64, c_int, c_i64,
                                    ctypes.c_double, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void]),
    'rdm_voxel_map_export': (c_int, [c_void, c_size, c_i64, c_int, c_void, c_size, c_void, c_size, c_i64, c_void, c_void, c_void, c_void,
                                     c_void, c_i64, c_void, c_void, c_size, c_void]),
    'rdm_voxel_map_import': (c_int, [c_void, c_size, c_i64, c_int, c_void, c_size, c_void, c_size, c_void, c_void, c_void, c_void, c_void,
                                     c_i64, c_i64, c_void, c_void, c_void]),
}



_lib = None


def build():
    """Compile the library in-tree (hipcc cross-compiles for gfx950 without a GPU)."""
    import subprocess
    subprocess.run(['make', '-C', os.path.join(_HERE, 'csrc'), '-j8'], check=True)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} is missing: build it with `make -C rdmnet_amd/csrc` '
                '(or __graft_entry__.build()); there is no CPU fallback')
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        got = handle.rdm_abi_version()
        if got != ABI_VERSION:  # a stale .so with other struct layouts would corrupt memory silently
            raise RuntimeError(f'{LIB_PATH} has ABI version {got}, this binding expects {ABI_VERSION}: rebuild it '
                               '(`make -C rdmnet_amd/csrc`)')
        _check_struct_sizes(handle)
        _lib = handle
    return _lib


def _check_struct_sizes(handle):
    """The ctypes mirrors of the structs that cross the C-ABI must have the library's sizes (the C side memsets and fills
    them through the pointers it is given)."""
    from . import engine as E  # (the mirrors live next to their user)
    for which, cls in enumerate((E.EngineConfig, E.EngineResult, E.TensorView, E.KpconvProfile, E.DataDict)):
        want, have = handle.rdm_abi_struct_size(which), ctypes.sizeof(cls)
        if want != have:
            raise RuntimeError(f'{LIB_PATH}: sizeof({cls.__name__}) is {want} in the library, {have} in rdmnet_amd/engine.py')


def check(code, what):
    if code != 0:
        msg = lib().rdm_last_error().decode('utf-8', 'replace')
        raise RuntimeError(f'{what} failed with code {code}: {msg}')


def ptr(t):
    """Device (or host) address of a torch tensor, 0 for None."""
    return 0 if t is None else t.data_ptr()


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream
