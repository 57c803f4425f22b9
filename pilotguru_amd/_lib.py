"""ctypes binding of libpgorb.so (the C ABI declared in include/pgorb.h).

The HIP library is the product: importing this module without a built
pilotguru_amd/libpgorb.so raises immediately -- there is no Python or CPU fallback.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PGORB_LIBRARY: a developer build of the same ABI (e.g. a timing build made with make EXTRA=...), for the scripts under tools/experiments
LIB_PATH = os.environ.get("PGORB_LIBRARY") or os.path.join(_HERE, "libpgorb.so")

PGORB_MAX_LEVELS = 16
PGORB_OK, PGORB_E_ARG, PGORB_E_TOOSMALL, PGORB_E_CAP = 0, -1, -2, -3
PGORB_E_NODEVICE, PGORB_E_HIP, PGORB_E_LIMIT, PGORB_E_OVERFLOW = -4, -5, -6, -7

# every symbol include/pgorb.h declares (tests check the .so exports all of them)
SYMBOLS = (
    "pgorb_create", "pgorb_destroy", "pgorb_last_error", "pgorb_levels", "pgorb_scale_tables",
    "pgorb_features_per_level", "pgorb_max_keypoints", "pgorb_extract", "pgorb_extract_batch",
    "pgorb_extract_batch_device", "pgorb_check_async", "pgorb_descriptor_distance",
    "pgorb_hamming_matrix", "pgorb_hamming_best2", "pgorb_match_batch_device",
    "pgorb_debug_level_size", "pgorb_debug_level_image", "pgorb_debug_level_candidates",
    "pgorb_debug_level_keypoints", "pgorb_debug_sincos_checksum", "pgorb_debug_arena", "pgorb_debug_host_graph", "pgorb_profile_begin", "pgorb_profile_read", "pgorb_profile_host",
    "pgorb_vocab_load_text", "pgorb_vocab_load_cached", "pgorb_vocab_from_blob", "pgorb_vocab_blob", "pgorb_vocab_info",
    "pgorb_vocab_free", "pgorb_vocab_upload", "pgorb_vocab_upload_device", "pgorb_bow_transform",
    "pgorb_bow_transform_device", "pgorb_bow_vectors", "pgorb_bow_score_l1",
    "pgorb_frame_grid", "pgorb_frame_grid_batch_device", "pgorb_search_for_initialization",
    "pgorb_search_for_initialization_batch_device", "pgorb_extract_batch_color_device",
    "pgorb_extract_batch_ingest_device",
    "pgorb_search_by_projection_points", "pgorb_search_by_projection_frame", "pgorb_search_by_bow",
    "pgorb_search_by_projection_points_batch_device", "pgorb_search_by_projection_frame_batch_device",
    "pgorb_feature_vectors_batch_device", "pgorb_search_by_bow_batch_device",
    "pgorb_search_for_triangulation", "pgorb_search_for_triangulation_batch_device",
    "pgorb_create_new_map_points", "pgorb_create_new_map_points_batch_device",
    "pgorb_fuse", "pgorb_fuse_batch_device",
    "pgorb_search_by_projection_sim3", "pgorb_search_by_projection_sim3_batch_device",
    "pgorb_fuse_sim3", "pgorb_fuse_sim3_batch_device",
    "pgorb_search_by_sim3", "pgorb_search_by_sim3_batch_device",
    "pgorb_search_by_bow_keyframes", "pgorb_search_by_bow_keyframes_batch_device",
    "pgorb_refresh_map_points", "pgorb_refresh_map_points_batch_device",
    "pgorb_update_connections", "pgorb_update_connections_batch_device", "pgorb_covisibility_views_device",
    "pgorb_update_local_map", "pgorb_update_local_map_batch_device",
    "pgorb_compact_observations_device", "pgorb_map_point_culling", "pgorb_map_point_culling_device",
    "pgorb_keyframe_culling", "pgorb_keyframe_culling_device",
    "pgorb_apply_map_edits", "pgorb_apply_map_edits_device", "pgorb_map_edits_from_keyframe_device",
    "pgorb_map_edits_from_fuse_device", "pgorb_map_edits_from_lba_erase_device", "pgorb_map_edits_from_loop_matches_device",
    "pgorb_observation_ids_device",
    "pgorb_correct_loop_poses", "pgorb_correct_loop_poses_device", "pgorb_global_ba_map_update", "pgorb_global_ba_map_update_device",
    "pgorb_track_predict", "pgorb_track_predict_batch_device", "pgorb_track_commit", "pgorb_track_commit_batch_device",
    "pgorb_keyframe_tcp", "pgorb_keyframe_tcp_device", "pgorb_get_trajectory", "pgorb_get_trajectory_device",
    "pgorb_check_replaced", "pgorb_check_replaced_batch_device", "pgorb_increase_visible", "pgorb_increase_visible_batch_device",
    "pgorb_query_seen_from_outliers", "pgorb_query_seen_from_outliers_batch_device", "pgorb_track_decide", "pgorb_track_decide_batch_device",
    "pgorb_track_finish", "pgorb_track_finish_batch_device", "pgorb_scene_median_depth", "pgorb_scene_median_depth_batch_device",
    "pgorb_scale_initial_map", "pgorb_scale_initial_map_device",
    "pgorb_bow_vectors_batch_device", "pgorb_bow_score_l1_batch_device",
    "pgorb_detect_relocalization_candidates", "pgorb_detect_relocalization_candidates_batch_device",
    "pgorb_detect_loop_candidates", "pgorb_detect_loop_candidates_batch_device",
    "pgorb_search_by_projection_keyframe", "pgorb_search_by_projection_keyframe_batch_device",
    "pgorb_log_f", "pgorb_log_scale_factor", "pgorb_predict_scale",
    "pgorb_search_local_points", "pgorb_search_local_points_batch_device",
    "pgorb_search_by_projection_last_frame", "pgorb_search_by_projection_last_frame_batch_device",
    "pgorb_search_by_projection_keyframe_pose", "pgorb_search_by_projection_keyframe_pose_batch_device",
    "pgorb_pose_optimization", "pgorb_pose_optimization_batch_device",
    "pgorb_slots_from_assignment", "pgorb_slots_from_assignment_batch_device",
    "pgorb_sim3_solver", "pgorb_sim3_solver_batch_device", "pgorb_sim3_max_iterations",
    "pgorb_optimize_sim3", "pgorb_optimize_sim3_batch_device",
    "pgorb_pnp_solver", "pgorb_pnp_solver_batch_device", "pgorb_pnp_ransac",
    "pgorb_initializer", "pgorb_initializer_batch_device",
    "pgorb_local_bundle_adjustment", "pgorb_local_bundle_adjustment_batch_device",
    "pgorb_optimize_essential_graph", "pgorb_optimize_essential_graph_device",
    "pgorb_global_bundle_adjustment", "pgorb_global_bundle_adjustment_device",
    "pgorb_undistort_keypoints", "pgorb_undistort_keypoints_batch_device", "pgorb_image_bounds",
    "pgorb_host_alloc", "pgorb_host_free", "pgorb_host_register", "pgorb_host_unregister", "pgorb_stream_create", "pgorb_stream_create_ingest", "pgorb_stream_create_device", "pgorb_stream_submit_device", "pgorb_stream_wait_device", "pgorb_stream_lanes", "pgorb_stream_destroy", "pgorb_stream_input", "pgorb_stream_reset", "pgorb_stream_submit",
    "pgorb_stream_wait", "pgorb_stream_frontend", "pgorb_stream_frontend_results", "pgorb_set_option", "pgorb_get_option", "pgorb_matcher_is_popcount",
    "pgorb_smooth_heading_directions", "pgorb_smooth_time_series", "pgorb_trajectory_pca",
    "pgorb_project_directions", "pgorb_project_translations", "pgorb_turn_angles",
    "pgorb_principal_rotation_axes", "pgorb_angular_velocities_around_axis",
    "pgorb_comm_library", "pgorb_comm_unique_id", "pgorb_comm_create_local", "pgorb_comm_create_rank", "pgorb_comm_ranks", "pgorb_vocab_broadcast", "pgorb_comm_destroy",
    "pgorb_kahan_sum", "pgorb_fit_num_windows", "pgorb_fit_velocity_windows", "pgorb_calibrator_eval", "pgorb_fit_motion_velocities",
)


# the records of the trajectory read-out (include/pgorb.h: pgorb_kf_pose, pgorb_track_state, pgorb_trajectory_record) and its constants
KF_POSE_DTYPE = np.dtype([("Tcw", "<f4", (12,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
                          ("invfx", "<f4"), ("invfy", "<f4")])
TRACK_STATE_DTYPE = np.dtype([("last", KF_POSE_DTYPE), ("velocity", "<f4", (12,)), ("last_ref_kf", "<i4"), ("has_last", "u1"),
                              ("has_velocity", "u1"), ("pad", "u1", (2,))])
TRAJECTORY_RECORD_DTYPE = np.dtype([("pose", "<f4", (12,)), ("ref_kf", "<i4"), ("has_pose", "u1"), ("lost", "u1"), ("pad", "u1", (2,)),
                                    ("frame_time", "<f8"), ("frame_id", "<i8")])
assert (KF_POSE_DTYPE.itemsize, TRACK_STATE_DTYPE.itemsize, TRAJECTORY_RECORD_DTYPE.itemsize) == (84, 140, 72)
PGORB_TRACK_MOTION_MODEL, PGORB_TRACK_REFERENCE_KF = 0, 1
PGORB_TRACK_NO_LAST, PGORB_TRACK_NO_VELOCITY, PGORB_TRACK_BAD_INDEX, PGORB_TRACK_FULL, PGORB_TRACK_MAX = 1, 2, 4, 8, 4096
PGORB_TRAJ_BROKEN, PGORB_TRAJ_BAD_TIME, PGORB_TRAJ_NO_ORIGIN, PGORB_TRAJ_INFO, PGORB_TRAJ_MAX_RECORDS = 1, 2, 4, 4, 1 << 22
PGORB_TCP_INFO = 4
# Tracking's decisions (include/pgorb.h: pgorb_track_counters and the PGORB_DECIDE_ / PGORB_DEPTH_ constants)
TRACK_COUNTERS_DTYPE = np.dtype([("frame_id", "<u8"), ("last_reloc_frame_id", "<u4"), ("last_kf_frame_id", "<u4"), ("max_frames", "<i4"),
                                 ("min_frames", "<i4"), ("nkfs", "<i4"), ("ref_kf", "<i4"), ("next_kf_id", "<u8"), ("stopped", "u1"),
                                 ("stop_requested", "u1"), ("accept_keyframes", "u1"), ("set_not_stop_ok", "u1"), ("pad", "u1", (4,))])
assert TRACK_COUNTERS_DTYPE.itemsize == 48
PGORB_DECIDE_MOTION_MODEL, PGORB_DECIDE_REFERENCE_KF, PGORB_DECIDE_LOCAL_MAP, PGORB_DECIDE_WRONG_INIT, PGORB_DECIDE_INFO = 0, 1, 2, 4, 4
PGORB_DEPTH_EMPTY, PGORB_DEPTH_NAN, PGORB_DEPTH_MAX_LIST = 1, 2, 262144


class PgorbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("max_width", C.c_int32),
                ("max_height", C.c_int32), ("max_batch", C.c_int32), ("device", C.c_int32),
                ("blur_tie_mode", C.c_int32)]


class PgorbError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("pgorb error %d: %s" % (code, text))
        self.code = code


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: build it with `make -C pilotguru_amd/csrc` "
                          "(hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 (+ HSA).  If
    # libpgorb.so pulled in /opt/rocm's copy first, torch would later load a SECOND runtime and
    # see no GPUs.  Importing torch first makes the loader satisfy our DT_NEEDED
    # libamdhip64.so.7 with the already-loaded copy (same SONAME).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32p, fp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float)
    L.pgorb_create.restype = C.c_int
    L.pgorb_create.argtypes = [C.POINTER(PgorbParams), C.POINTER(vp)]
    L.pgorb_destroy.restype = None
    L.pgorb_destroy.argtypes = [vp]
    L.pgorb_last_error.restype = C.c_char_p
    L.pgorb_last_error.argtypes = [vp]
    L.pgorb_levels.argtypes = [vp]
    L.pgorb_scale_tables.argtypes = [vp, fp, fp, fp, fp]
    L.pgorb_features_per_level.argtypes = [vp, i32p]
    L.pgorb_max_keypoints.argtypes = [vp, C.c_int, C.c_int]
    L.pgorb_extract.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, i32p]
    L.pgorb_extract_batch.argtypes = [vp, C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int,
                                      vp, vp, C.c_int, i32p]
    L.pgorb_extract_batch_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64,
                                             vp, vp, C.c_int, vp, vp]
    L.pgorb_check_async.argtypes = [vp, vp]
    L.pgorb_extract_batch_color_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int,
                                                   vp, vp, C.c_int, vp, vp]
    L.pgorb_extract_batch_ingest_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int,
                                                    C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp]
    L.pgorb_descriptor_distance.argtypes = [vp, vp]
    L.pgorb_hamming_matrix.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp]
    L.pgorb_hamming_best2.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, vp]
    L.pgorb_match_batch_device.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]
    L.pgorb_debug_level_size.argtypes = [vp, C.c_int, i32p, i32p]
    L.pgorb_debug_level_image.argtypes = [vp, C.c_int, C.c_int, vp]
    L.pgorb_debug_level_candidates.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int]
    L.pgorb_debug_level_keypoints.argtypes = [vp, C.c_int, C.c_int]
    L.pgorb_debug_arena.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_int64)]
    L.pgorb_debug_host_graph.argtypes = [vp, i32p, i32p]
    L.pgorb_stream_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.pgorb_stream_create_ingest.argtypes = [vp] + [C.c_int] * 9 + [C.POINTER(vp)]
    L.pgorb_stream_create_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.pgorb_stream_submit_device.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int64, vp]
    L.pgorb_stream_wait_device.argtypes = [vp, C.c_int, C.c_int, vp] + [C.POINTER(vp)] * 6 + [i32p]
    L.pgorb_stream_lanes.argtypes = [vp]
    L.pgorb_stream_destroy.restype = None
    L.pgorb_stream_destroy.argtypes = [vp]
    L.pgorb_stream_input.restype = vp
    L.pgorb_stream_input.argtypes = [vp, C.c_int]
    L.pgorb_stream_reset.argtypes = [vp]
    L.pgorb_stream_submit.argtypes = [vp, C.c_int, C.c_int]
    L.pgorb_stream_wait.argtypes = [vp, C.c_int] + [C.POINTER(vp)] * 6 + [i32p]
    L.pgorb_stream_frontend.argtypes = [vp] + [C.c_float] * 4 + [C.c_int, C.c_float, C.c_int, C.c_int]
    L.pgorb_stream_frontend_results.argtypes = [vp, C.c_int] + [C.POINTER(vp)] * 5
    L.pgorb_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    L.pgorb_get_option.argtypes = [vp, C.c_char_p]
    L.pgorb_matcher_is_popcount.argtypes = [vp, C.c_int]
    L.pgorb_profile_begin.argtypes = [vp, C.c_int]
    L.pgorb_profile_read.argtypes = [vp, C.POINTER(C.c_double)]
    L.pgorb_profile_host.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
    f4 = [C.c_float] * 4
    L.pgorb_frame_grid.argtypes = [vp, vp, C.c_int] + f4 + [vp, vp]
    L.pgorb_frame_grid_batch_device.argtypes = [vp, vp, vp, C.c_int, C.c_int] + f4 + [vp, vp, vp]
    L.pgorb_search_for_initialization.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int] + f4 + [vp, vp, C.c_int, C.c_float, C.c_int]
    L.pgorb_search_for_initialization_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int] + f4 + \
        [vp, vp, vp, C.c_int, C.c_float, C.c_int, vp]
    L.pgorb_search_by_projection_points.argtypes = [vp, vp, vp, C.c_int] + f4 + [vp, C.c_int] + [vp] * 7 + [C.c_float, C.c_float, vp]
    L.pgorb_search_by_projection_frame.argtypes = [vp, vp, vp, C.c_int] + f4 + [vp, C.c_int] + [vp] * 7 + [C.c_float, C.c_int, vp]
    L.pgorb_search_by_bow.argtypes = [vp] + [vp] * 3 + [C.c_int] + [vp] * 3 + [C.c_int] + [vp] * 2 + [C.c_int] + [vp] * 3 + \
        [C.c_int, C.c_float, C.c_int, vp]
    # (ctx, kps, desc, n, cap, grid_start, grid_idx, pair_frame, npairs, bounds x 4, kp_has_point, qcap, nq, 7 query arrays, th, ratio | check, assigned, nmatches, stream)
    L.pgorb_search_by_projection_points_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int] + f4 + [vp, C.c_int, vp] + [vp] * 7 + \
        [C.c_float, C.c_float, vp, vp, vp]
    L.pgorb_search_by_projection_frame_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int] + f4 + [vp, C.c_int, vp] + [vp] * 7 + \
        [C.c_float, C.c_int, vp, vp, vp]
    L.pgorb_search_by_projection_keyframe.argtypes = [vp, vp, vp, C.c_int] + f4 + [vp, C.c_int] + [vp] * 9 + [C.c_float, C.c_float, C.c_int, C.c_int, vp]
    L.pgorb_search_by_projection_keyframe_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int] + f4 + [vp, C.c_int, vp] + [vp] * 9 + \
        [C.c_float, C.c_float, C.c_int, C.c_int, vp, vp, vp]
    # the tracking thread's matchers with the projection on the device
    # (ctx, kps, desc, n, bounds x 4, pose, kp_point, npoints, points, point_desc, point_bad, point_has_obs, nq, queries, query_seen,
    #  viewing_cos_limit, th, nnratio, in_view, proj_x, proj_y, level, view_cos, kp_point_out, n_to_match, assigned)
    L.pgorb_search_local_points.argtypes = [vp, vp, vp, C.c_int] + f4 + [vp, vp, C.c_int] + [vp] * 4 + [C.c_int, vp, vp] + [C.c_float] * 3 + [vp] * 8
    # (ctx, kps, desc, n, bounds x 4, pose, kp_has_point, last_kps, nlast, last_point, last_outlier, npoints, points, point_desc,
    #  point_has_obs, th, check, valid, u, v, assigned)
    L.pgorb_search_by_projection_last_frame.argtypes = [vp, vp, vp, C.c_int] + f4 + [vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp,
                                                        C.c_float, C.c_int] + [vp] * 4
    # (..., kf_kps, nkf, kf_point, already_found, npoints, points, point_desc, point_bad, th, orb_dist, check, u, v, dist3d, assigned)
    L.pgorb_search_by_projection_keyframe_pose.argtypes = [vp, vp, vp, C.c_int] + f4 + [vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp,
                                                           C.c_float, C.c_int, C.c_int] + [vp] * 4
    # (ctx, kps, desc, n, cap, grid_start, grid_idx, pair_frame, npairs, bounds x 4, pose, kp_point, npoints, 4 table arrays, qcap, nq,
    #  queries, query_seen, viewing_cos_limit, th, nnratio, 5 query outputs, kp_point_out, n_to_match, assigned, nmatches, stream)
    L.pgorb_search_local_points_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int] + f4 + [vp, vp, C.c_int] + [vp] * 4 + \
        [C.c_int, vp, vp, vp] + [C.c_float] * 3 + [vp] * 10
    # (ctx, kps, desc, n, cap, grid_start, grid_idx, pair_frame, pair_last | pair_kf, npairs, bounds x 4, pose, kp_has_point, ...)
    L.pgorb_search_by_projection_last_frame_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int] + f4 + \
        [vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_float, C.c_int] + [vp] * 6
    L.pgorb_search_by_projection_keyframe_pose_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int] + f4 + \
        [vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_float, C.c_int, C.c_int] + [vp] * 6
    # (ctx, kps, n, pose, kp_point, npoints, points, point_has_obs, discard_outliers, pose_out, outlier, kp_point_out, nmatches_map, chi2, info)
    L.pgorb_pose_optimization.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int] + [vp] * 6
    # (ctx, kps, n, cap, pair_frame, npairs, pose, kp_point, npoints, points, point_has_obs, discard_outliers, pose_out, outlier,
    #  kp_point_out, nmatches_map, chi2, info, ninliers, stream)
    L.pgorb_pose_optimization_batch_device.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int] + [vp] * 8
    # (ctx, assigned, source, nsource | source_stride, kp_point, n | cap, [npairs, stream])
    L.pgorb_slots_from_assignment.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int]
    L.pgorb_slots_from_assignment_batch_device.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp]
    # (ctx, kps1, n1, pose1, kf_point1, kps2, n2, pose2, kf_point2, matches12, npoints, points, point_bad, params, draws, found, found_sim3,
    #  best, inlier, matches12_out, already1, already2, info)
    L.pgorb_sim3_solver.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int] + [vp] * 12
    # (ctx, kps, n, cap, pair_kf1, pair_kf2, npairs, pose, kf_point, matches12, npoints, points, point_bad, params, first_iteration,
    #  best_inliers_in, draws, found, found_sim3, best, inlier, matches12_out, already1, already2, info, ninliers, stream)
    L.pgorb_sim3_solver_batch_device.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_int] + [vp] * 16
    L.pgorb_sim3_max_iterations.argtypes = [C.c_float, C.c_int, C.c_int, C.c_int]
    # (ctx, kps, n, camera, kp_point, npoints, points, point_bad, params, draws, best_inlier_in, best_pose_in, pose_out, inlier, kp_point_out,
    #  best_inlier_out, best_pose_out, trace, info)
    L.pgorb_pnp_solver.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int] + [vp] * 13
    # (ctx, kps, n, cap, pair_frame, npairs, camera, kp_point, npoints, points, point_bad, params, first_iteration, best_inliers_in, draws,
    #  best_inlier, best_pose, pose_out, inlier, kp_point_out, trace, info, ninliers, stream)
    L.pgorb_pnp_solver_batch_device.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int] + [vp] * 15
    L.pgorb_pnp_ransac.argtypes = [C.c_float, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, i32p, i32p]
    # (ctx, kps1, n1, kps2, n2, camera, matches12, params, draws, pose_out, P3D, triangulated, matches12_out, points, kf_point1, kf_point2,
    #  obs_start, obs_frame, obs_idx, npoints, trace, info, finfo)
    L.pgorb_initializer.argtypes = [vp, vp, C.c_int, vp, C.c_int] + [vp] * 18
    # (ctx, kps, n, cap, pair_f1, pair_f2, npairs, camera, matches12, params, draws, pose_out, P3D, triangulated, matches12_out, points,
    #  kf_point1, kf_point2, obs_start, obs_frame, obs_idx, npoints, trace, info, finfo, stream)
    L.pgorb_initializer_batch_device.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int] + [vp] * 19
    # (ctx, kps1, n1, pose1, kf_point1, kps2, n2, pose2, kf_point2, matches12, new_matches12, npoints, points, point_bad, estimate, th2,
    #  fix_scale, estimate_out, matches12_out, chi2_12, chi2_21, scw_pose, info)
    L.pgorb_optimize_sim3.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_float, C.c_int] + [vp] * 6
    # (ctx, kps, n, cap, pair_kf1, pair_kf2, npairs, pose, kf_point, matches12, new_matches12, npoints, points, point_bad, estimate, th2,
    #  fix_scale, estimate_out, matches12_out, chi2_12, chi2_21, scw_pose, info, nin, stream)
    L.pgorb_optimize_sim3_batch_device.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_float, C.c_int] + \
        [vp] * 8
    # (ctx, nkf, kps[], n, pose, kf_bad, kf_point[], kf_fixed_id0, nlocal, local_kf, npoints, points, point_bad, obs_start, obs_frame,
    #  obs_idx, rounds, pose_out, erase, chi2, level, is_local, role, info)
    L.pgorb_local_bundle_adjustment.argtypes = [vp, C.c_int] + [vp] * 6 + [C.c_int, vp, C.c_int] + [vp] * 5 + [C.c_int] + [vp] * 7
    # (ctx, kps, n, nframes, cap, pose, kf_bad, kf_point, kf_fixed_id0, win_start, win_kf, nwin, nwin_kf, npoints, points, point_bad,
    #  obs_start, obs_frame, obs_idx, nobs, rounds, pose_out, erase, chi2, level, is_local, role, info, nerased, stream)
    L.pgorb_local_bundle_adjustment_batch_device.argtypes = [vp, vp, vp, C.c_int, C.c_int] + [vp] * 6 + [C.c_int, C.c_int, C.c_int] + [vp] * 5 + \
        [C.c_int, C.c_int] + [vp] * 9
    # (ctx, nkf, kf_id, pose, kf_bad, loop_kf, cur_kf, fix_scale, has_corrected, corrected, has_non_corrected, non_corrected, nloop_conn,
    #  loop_conn, parent, loop_edge_start, loop_edge, covis_start, covis, covis_weight, min_feat, iterations, npoints, points, point_bad,
    #  point_ref_kf, sim3_out, pose_out, edge_out, info)
    L.pgorb_optimize_essential_graph.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int] + [vp] * 4 + [C.c_int] + [vp] * 7 + \
        [C.c_int, C.c_int, C.c_int] + [vp] * 7
    # (... loop_edge, nloop_edges, covis_start, covis, covis_weight, ncovis, ... info, stream)
    L.pgorb_optimize_essential_graph_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int] + [vp] * 4 + [C.c_int] + [vp] * 4 + \
        [C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 8
    # (ctx, nkf, kps[], n, pose, kf_bad, kf_fixed_id0, npoints, points, point_bad, obs_start, obs_frame, obs_idx, iterations, robust,
    #  in_place, pose_out, pos_out, kf_done, point_done, chi2, info)
    L.pgorb_global_bundle_adjustment.argtypes = [vp, C.c_int] + [vp] * 5 + [C.c_int] + [vp] * 5 + [C.c_int, C.c_int, C.c_int] + [vp] * 6
    # (ctx, kps, n, nframes, cap, pose, kf_bad, kf_fixed_id0, npoints, points, point_bad, obs_start, obs_frame, obs_idx, nobs, iterations,
    #  robust, in_place, pose_out, pos_out, kf_done, point_done, chi2, info, stream)
    L.pgorb_global_bundle_adjustment_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int] + [vp] * 5 + \
        [C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 7
    L.pgorb_log_f.argtypes = [C.c_float]
    L.pgorb_log_scale_factor.argtypes = [vp]
    L.pgorb_predict_scale.argtypes = [vp, C.c_float, C.c_float]
    L.pgorb_feature_vectors_batch_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.pgorb_search_by_bow_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, C.c_float, C.c_int, vp, vp, vp]
    # (ctx, kps1, desc1, has_point1, n1, fv1 x 3, nfv1, kps2, desc2, has_point2, n2, fv2 x 3, nfv2, F12, ex, ey, check, matches12)
    L.pgorb_search_for_triangulation.argtypes = [vp] + ([vp] * 3 + [C.c_int] + [vp] * 3 + [C.c_int]) * 2 + [vp, C.c_float, C.c_float, C.c_int, vp]
    L.pgorb_search_for_triangulation_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int] + [vp] * 4 + \
        [C.c_int, vp, vp, vp]
    L.pgorb_create_new_map_points.argtypes = [vp] + [vp] * 3 + [C.c_int] + [vp] * 3 + [C.c_int, vp] + [C.c_int] + [vp] * 15
    L.pgorb_create_new_map_points_batch_device.argtypes = [vp, vp, vp, vp, C.c_int] + [vp] * 7 + [C.c_int, vp, vp, C.c_int] + [vp] * 8
    # (ctx, kps, desc, n, pose, kf_id, bounds x 4, kf_point, npoints, points, point_desc, point_bad, obs_start, obs_kf, nq, queries, th,
    #  action, best_idx, best_dist, kf_point_out)
    L.pgorb_fuse.argtypes = [vp, vp, vp, C.c_int, vp, C.c_uint64] + f4 + [vp, C.c_int] + [vp] * 5 + [C.c_int, vp, C.c_float] + [vp] * 4
    L.pgorb_fuse_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp] + f4 + [vp, C.c_int] + [vp] * 5 + \
        [C.c_int, vp, vp, C.c_float] + [vp] * 5 + [vp]
    # (ctx, kps, desc, n, scw_pose, bounds x 4, matched_in, npoints, points, point_desc, point_bad, nq, queries, th, assigned, matched_out)
    L.pgorb_search_by_projection_sim3.argtypes = [vp, vp, vp, C.c_int, vp] + f4 + [vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp]
    L.pgorb_search_by_projection_sim3_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp] + f4 + \
        [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.c_int] + [vp] * 4
    # (ctx, [desc, angle, point_valid, n, fv x 3, nfv] x 2, nnratio, check, matches12)
    L.pgorb_search_by_bow_keyframes.argtypes = [vp] + ([vp] * 3 + [C.c_int] + [vp] * 3 + [C.c_int]) * 2 + [C.c_float, C.c_int, vp]
    # (ctx, kps, desc, n, cap, fv x 3, nfv, pair_kf1, pair_kf2, npairs, point_valid1, point_valid2, nnratio, check, matches12, nmatches, stream)
    L.pgorb_search_by_bow_keyframes_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_float,
                                                             C.c_int, vp, vp, vp]
    # (ctx, [kps, desc, n, pose, kf_point, already] x 2, bounds x 4, npoints, points, point_desc, point_bad, sim3, th, match12)
    L.pgorb_search_by_sim3.argtypes = [vp] + [vp, vp, C.c_int, vp, vp, vp] * 2 + f4 + [C.c_int, vp, vp, vp, vp, C.c_float, vp]
    L.pgorb_search_by_sim3_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp] + f4 + \
        [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_float, vp, vp, vp]
    # (ctx, kps, desc, n, scw_pose, bounds x 4, kf_point, npoints, points, point_desc, point_bad, nq, queries, th, action, replace_point,
    #  best_idx, best_dist, kf_point_out)
    L.pgorb_fuse_sim3.argtypes = [vp, vp, vp, C.c_int, vp] + f4 + [vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_float] + [vp] * 5
    L.pgorb_fuse_sim3_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp] + f4 + \
        [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.c_float] + [vp] * 7
    # (ctx, nkf, kps[], desc[], n, pose, kf_bad, npoints, points, point_desc, point_bad, obs_start, obs_frame, obs_idx, ref_obs, nsel,
    #  select, what, best_obs, status)
    L.pgorb_refresh_map_points.argtypes = [vp, C.c_int] + [vp] * 5 + [C.c_int] + [vp] * 7 + [C.c_int, vp, C.c_int, vp, vp]
    # (ctx, kps, desc, n, nframes, cap, pose, kf_bad, npoints, points, point_desc, point_bad, obs_start, obs_frame, obs_idx, nobs,
    #  ref_obs, nsel, select, what, best_obs, status, stream)
    L.pgorb_refresh_map_points_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int] + [vp] * 6 + \
        [C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, vp]
    # (ctx, nkf, kf_point[], n, npoints, point_bad, obs_start, obs_frame, kf_order, kf_id0, nlist, list, th, conn_cap, conn_kf, conn_w, nconn,
    #  ord_kf, ord_w, nord, parent, first_connection, row_status, loop_conn_cap, loop_conn, info)
    L.pgorb_update_connections.argtypes = [vp, C.c_int, vp, vp, C.c_int] + [vp] * 5 + [C.c_int, vp, C.c_int, C.c_int] + [vp] * 9 + [C.c_int, vp, vp]
    # (ctx, kf_point, n, nframes, cap, npoints, point_bad, obs_start, obs_frame, nobs, kf_order, kf_id0, nlist, list, th, conn_cap, 6 row arrays,
    #  parent, first_connection, row_status, loop_conn_cap, loop_conn, info, stream)
    L.pgorb_update_connections_batch_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int,
                                                        C.c_int] + [vp] * 9 + [C.c_int, vp, vp, vp]
    # (ctx, nframes, conn_cap, ord_kf, ord_w, nord, nbest, best, ncovis_cap, covis_start, covis, covis_weight, w, by_weight, info, stream)
    L.pgorb_covisibility_views_device.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp]
    # (ctx, nkf, kf_point[], n, kf_bad, kp_point, nkp, npoints, point_bad, obs_start, obs_frame, conn_cap, ord_kf, nord, parent, kf_order, nbest,
    #  max_local, nprev, prev_local_kf, kp_point_out, lkf_cap, local_kf, nlocal_kf, ref_kf, qcap, queries, nq, status)
    L.pgorb_update_local_map.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int,
                                         C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp]
    # (ctx, kf_point, n, nframes, cap, kf_bad, pair_frame, npairs, kp_point, npoints, point_bad, obs_start, obs_frame, nobs, conn_cap, ord_kf,
    #  nord, parent, kf_order, nbest, max_local, lkf_cap, prev_local_kf, nprev, kp_point_out, local_kf, nlocal_kf, ref_kf, qcap, queries, nq,
    #  status, stream)
    L.pgorb_update_local_map_batch_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int,
                                                      vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
    # (ctx, npoints, obs_start, obs_frame, obs_idx, nobs, obs_live, ref_obs, obs_start_out, obs_frame_out, obs_idx_out, ref_obs_out, info, stream)
    L.pgorb_compact_observations_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int] + [vp] * 8
    # (ctx, nkf, kf_point[], n, npoints, point_bad, obs_start, obs_frame, obs_idx, obs_live, first_kf_id, visible, found, nrecent, recent,
    #  cur_kf_id, th_obs, action, recent_out, nrecent_out, info)
    L.pgorb_map_point_culling.argtypes = [vp, C.c_int, vp, vp, C.c_int] + [vp] * 8 + [C.c_int, vp, C.c_int, C.c_int] + [vp] * 4
    # (ctx, kf_point, n, nframes, cap, npoints, point_bad, obs_start, obs_frame, obs_idx, nobs, obs_live, first_kf_id, visible, found, nrecent,
    #  recent, cur_kf_id, th_obs, action, recent_out, nrecent_out, info, stream)
    L.pgorb_map_point_culling_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp,
                                                 C.c_int, C.c_int] + [vp] * 5
    # (ctx, nkf, kps[], kf_point[], n, npoints, point_bad, obs_start, obs_frame, obs_idx, obs_live, ref_obs, kf_order, kf_id0, kf_not_erase,
    #  kf_bad, kf_to_be_erased, cur_kf, conn_cap, 6 row arrays, parent, list_cap, record, row_status, info)
    L.pgorb_keyframe_culling.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int] + [vp] * 11 + [C.c_int, C.c_int] + [vp] * 7 + [C.c_int, vp, vp, vp]
    # (ctx, kps, kf_point, n, nframes, cap, npoints, point_bad, obs_start, obs_frame, obs_idx, nobs, obs_live, ref_obs, kf_order, kf_id0,
    #  kf_not_erase, kf_bad, kf_to_be_erased, cur_kf, conn_cap, 6 row arrays, parent, list_cap, record, row_status, info, stream)
    L.pgorb_keyframe_culling_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int] + [vp] * 7 + \
        [C.c_int, C.c_int] + [vp] * 7 + [C.c_int, vp, vp, vp, vp]
    # (ctx, edits, nedits, nkf, kf_point[], n, kf_order, npoints, point_bad, visible, found, replaced, obs_start, obs_frame, obs_idx, obs_live,
    #  ref_obs, obs_cap_out, obs_start_out, obs_frame_out, obs_idx_out, ref_obs_out, edit_status, touched, select_bits, sel_cap, select_out, info)
    L.pgorb_apply_map_edits.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int] + [vp] * 9 + [C.c_int] + [vp] * 6 + [C.c_int, C.c_int, vp, vp]
    # (ctx, edits, nedits, nedits_dev, kf_point, n, nframes, cap, kf_order, npoints, point_bad, visible, found, replaced, obs_start, obs_frame,
    #  obs_idx, nobs, obs_live, ref_obs, obs_cap_out, 4 CSR outputs, edit_status, touched, select_bits, sel_cap, select_out, info, stream)
    L.pgorb_apply_map_edits_device.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int] + [vp] * 7 + [C.c_int, vp, vp, C.c_int] + \
        [vp] * 6 + [C.c_int, C.c_int, vp, vp, vp]
    # (ctx, kf_point, n, nframes, cap, npoints, point_bad, obs_start, obs_frame, nobs, obs_live, kf, edits, slot_class, stream)
    L.pgorb_map_edits_from_keyframe_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp]
    # (ctx, kf_point, n, nframes, cap, npoints, kf, qcap, nq, queries, action, best_idx, replace_point, edits, stream)
    L.pgorb_map_edits_from_fuse_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 7
    # (ctx, npoints, obs_start, obs_frame, nobs, erase, edits, stream)
    L.pgorb_map_edits_from_lba_erase_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, vp]
    # (ctx, kf_point, n, nframes, cap, npoints, cur_kf, matched, edits, stream)
    L.pgorb_map_edits_from_loop_matches_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    # (ctx, npoints, obs_start, obs_frame, nobs, kf_id, nframes, obs_kf_out, stream)
    L.pgorb_observation_ids_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, vp]
    # (ctx, nkf, kps[], n, pose, cur_kf, scw, nlist, list, kf_order, kf_point[], npoints, points, point_bad, obs_start, obs_frame, obs_idx,
    #  ref_obs, ref_kf, has_corrected, corrected, has_non_corrected, non_corrected, pose_out, corrected_by, point_ref_kf, info)
    L.pgorb_correct_loop_poses.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int] + [vp] * 15
    # (ctx, kps, n, nframes, cap, pose, cur_kf, scw, nlist, list, list_count, kf_order, kf_point, npoints, points, point_bad, obs_start,
    #  obs_frame, obs_idx, nobs, ref_obs, ref_kf, has_corrected, corrected, has_non_corrected, non_corrected, pose_out, corrected_by,
    #  point_ref_kf, info, stream)
    L.pgorb_correct_loop_poses_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int] + [vp] * 5 + \
        [C.c_int] + [vp] * 11
    # (ctx, nkf, pose, pose_gba, kf_done, parent, kf_origin, kf_bad, npoints, points, pos_gba, point_done, point_bad, ref_kf, pose_out,
    #  kf_updated, point_updated, info[, stream])
    L.pgorb_global_ba_map_update.argtypes = [vp, C.c_int] + [vp] * 6 + [C.c_int] + [vp] * 9
    L.pgorb_global_ba_map_update_device.argtypes = [vp, C.c_int] + [vp] * 6 + [C.c_int] + [vp] * 10
    # (ctx, mode, state, last_record, nkf, kf_pose, pose_out)
    L.pgorb_track_predict.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp]
    # (ctx, ntrack, mode, modes, state, traj, traj_cap, ntrajectory, nkf, kf_pose, pose_out, status, stream)
    L.pgorb_track_predict_batch_device.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    # (ctx, state, pose, ok, ref_kf, frame_time, frame_id, nkf, kf_pose, traj, traj_cap, ntrajectory)
    L.pgorb_track_commit.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_double, C.c_int64, C.c_int, vp, vp, C.c_int, vp]
    # (ctx, ntrack, state, pose, ok, ref_kf, frame_time, frame_id, nkf, kf_pose, traj, traj_cap, ntrajectory, status, stream)
    L.pgorb_track_commit_batch_device.argtypes = [vp, C.c_int] + [vp] * 6 + [C.c_int, vp, vp, C.c_int, vp, vp, vp]
    # (ctx, nkf, pose, parent, nrecord | list_cap, record, [cull_info,] tcp, info_out[, stream])
    L.pgorb_keyframe_tcp.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, vp]
    L.pgorb_keyframe_tcp_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    # (ctx, nkf, pose, kf_bad, parent, kf_id, tcp, n, traj, [count,] quat_wxyz, translation, time_usec, frame_id, is_lost, status, info[, stream])
    L.pgorb_get_trajectory.argtypes = [vp, C.c_int] + [vp] * 5 + [C.c_int] + [vp] * 8
    L.pgorb_get_trajectory_device.argtypes = [vp, C.c_int] + [vp] * 5 + [C.c_int] + [vp] * 10
    # Tracking's decisions; the _batch_device / _device forms take the same arguments and a stream
    # (ctx, ntrack, n, nframes, cap, frame, last_point, npoints, replaced)
    td = [vp, C.c_int, vp, C.c_int, C.c_int, vp]
    L.pgorb_check_replaced.argtypes = td + [vp, C.c_int, vp]
    # (.., run, kp_point, qcap, nq, queries, in_view, npoints, visible)
    L.pgorb_increase_visible.argtypes = td + [vp, vp, C.c_int, vp, vp, vp, C.c_int, vp]
    # (.., kp_point, outlier, kp_point_opt, qcap, nq, queries, npoints, query_seen)
    L.pgorb_query_seen_from_outliers.argtypes = td + [vp, vp, vp, C.c_int, vp, vp, C.c_int, vp]
    # (ctx, ntrack, mode, modes, after_retry, n, nframes, cap, frame, run, nmatches, nmatches_map, pose_before, kp_point_before, pose_opt,
    #  kp_point_opt, outlier, npoints, point_has_obs, found, counters, ok, inliers, retry, pose_final, kp_point_final)
    L.pgorb_track_decide.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int] + [vp] * 9 + [C.c_int] + [vp] * 8
    # (.., ok, inliers, counters, pose_final, kp_point, outlier, npoints, point_bad, point_has_obs, obs_start, obs_frame, nobs, obs_live,
    #  kf_point, kf_pose, kf_id, kp_point_out, ref_kf_out, new_kf, interrupt_ba)
    L.pgorb_track_finish.argtypes = td + [vp] * 6 + [C.c_int, vp, vp, vp, vp, C.c_int] + [vp] * 8
    # (ctx, nlist, kf, q, kf_point, n, nframes, cap, pose, npoints, points, median_depth, status)
    L.pgorb_scene_median_depth.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp]
    # (ctx, kf_ini, kf_cur, kf_point, n, nframes, cap, pose, npoints, points, point_bad, obs_start, obs_frame, nobs, obs_live, info)
    L.pgorb_scale_initial_map.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp]
    for name in ("check_replaced", "increase_visible", "query_seen_from_outliers", "track_decide", "track_finish", "scene_median_depth"):
        getattr(L, "pgorb_%s_batch_device" % name).argtypes = getattr(L, "pgorb_" + name).argtypes + [vp]
    L.pgorb_scale_initial_map_device.argtypes = L.pgorb_scale_initial_map.argtypes + [vp]
    # (ctx, word, weight, n, nframes, cap, bow_id, bow_val, nbow, stream)
    L.pgorb_bow_vectors_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    # (ctx, bow_id, bow_val, nbow, nframes, cap, pair_a, pair_b, npairs, score, stream)
    L.pgorb_bow_score_l1_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp]
    # (ctx, bow_id, bow_val, nbow, nframes, cap, in_db, neigh, query, nq, [state | min_score, conn_start, conn, nconn], cand, ccap, ncand,
    #  common, score, stats, stream)
    L.pgorb_detect_relocalization_candidates_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.c_int] + [vp] * 5
    L.pgorb_detect_loop_candidates_batch_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int] + \
        [vp] * 5
    # (ctx, nkf, bow_start, bow_id, bow_val, in_db, neigh_start, neigh, query, ...)
    L.pgorb_detect_relocalization_candidates.argtypes = [vp, C.c_int] + [vp] * 6 + [C.c_int, vp, vp, C.c_int, vp, vp]
    L.pgorb_detect_loop_candidates.argtypes = [vp, C.c_int] + [vp] * 6 + [C.c_int, C.c_float, vp, C.c_int, vp, C.c_int, vp, vp, vp]
    L.pgorb_undistort_keypoints.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    L.pgorb_undistort_keypoints_batch_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.pgorb_image_bounds.argtypes = [C.c_int, C.c_int, vp, vp, vp]
    L.pgorb_smooth_heading_directions.argtypes = [vp, C.c_int, C.c_int]
    L.pgorb_smooth_time_series.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_double, vp]
    L.pgorb_trajectory_pca.argtypes = [vp, C.c_int, vp, vp, vp]
    L.pgorb_project_directions.argtypes = [vp, C.c_int, vp, vp]
    L.pgorb_project_translations.argtypes = [vp, C.c_int, vp]
    L.pgorb_turn_angles.argtypes = [vp, C.c_int, vp]
    series = [vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int]
    L.pgorb_principal_rotation_axes.argtypes = [vp, vp, C.c_int, C.c_int64, vp]
    L.pgorb_angular_velocities_around_axis.argtypes = [vp, C.c_int, vp, vp]
    L.pgorb_kahan_sum.argtypes = [vp, C.c_int, C.c_int, vp]
    L.pgorb_fit_num_windows.argtypes = [C.c_int, C.c_int]
    L.pgorb_fit_velocity_windows.argtypes = [vp] + series + [C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.pgorb_calibrator_eval.argtypes = [vp] + series + [vp, C.c_int, vp, vp]
    L.pgorb_fit_motion_velocities.argtypes = [vp] + series + [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                                              vp, vp, i32p, vp]
    L.pgorb_host_alloc.restype = vp
    L.pgorb_host_alloc.argtypes = [C.c_int64]
    L.pgorb_host_free.restype = None
    L.pgorb_host_free.argtypes = [vp]
    L.pgorb_host_register.argtypes = [vp, C.c_int64]
    L.pgorb_host_unregister.argtypes = [vp]
    L.pgorb_vocab_load_text.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.pgorb_vocab_load_cached.argtypes = [C.c_char_p, C.POINTER(vp), i32p]
    L.pgorb_vocab_from_blob.argtypes = [vp, C.c_int64, C.POINTER(vp)]
    L.pgorb_vocab_blob.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64)]
    L.pgorb_vocab_info.argtypes = [vp] + [i32p] * 6
    L.pgorb_vocab_free.restype = None
    L.pgorb_vocab_free.argtypes = [vp]
    L.pgorb_vocab_upload.argtypes = [vp, vp]
    L.pgorb_vocab_upload_device.argtypes = [vp, vp, C.c_int64, vp]
    L.pgorb_bow_transform.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.pgorb_bow_transform_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.pgorb_bow_vectors.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, i32p, vp, vp, vp, i32p]
    L.pgorb_comm_library.argtypes = [C.c_char_p, C.c_int, i32p]
    L.pgorb_comm_unique_id.argtypes = [vp]
    L.pgorb_comm_create_local.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp)]
    L.pgorb_comm_create_rank.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.pgorb_comm_ranks.argtypes = [vp]
    L.pgorb_vocab_broadcast.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_double)]
    L.pgorb_comm_destroy.restype = None
    L.pgorb_comm_destroy.argtypes = [vp]
    L.pgorb_bow_score_l1.restype = C.c_double
    L.pgorb_bow_score_l1.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int]
    for name in SYMBOLS:
        if name not in ("pgorb_destroy", "pgorb_last_error", "pgorb_vocab_free", "pgorb_bow_score_l1",
                        "pgorb_host_alloc", "pgorb_host_free", "pgorb_stream_destroy", "pgorb_stream_input", "pgorb_log_f", "pgorb_log_scale_factor",
                        "pgorb_comm_destroy"):
            getattr(L, name).restype = C.c_int
    L.pgorb_log_f.restype = C.c_float
    L.pgorb_log_scale_factor.restype = C.c_float
    _lib = L
    return L
