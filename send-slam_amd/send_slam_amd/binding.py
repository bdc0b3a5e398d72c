"""ctypes binding of libsendslam_orb.so (include/sendslam_orb.h).

This is plumbing over the C ABI: it owns no arithmetic.  There is no fallback of any kind:
if the shared library is missing or exports the wrong ABI, importing the symbols raises, and
without a HIP device `OrbContext()` raises `OrbError(SS_ERR_NO_DEVICE)`.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, "lib", "libsendslam_orb.so")
SS_MAX_LEVELS = 16
EXPANDED_ROW_BYTES = 128  # one FP4 value (+1 / -1) per descriptor bit
ABI_VERSION = 5
SS_TRACK_DESC_STAYS_VALID = 1
SS_GUIDED_MAX_ROWS = 16384
SS_MAX_RECTIFY_MAPS = 16
SS_VOCAB_MAX_K, SS_VOCAB_MAX_DEPTH, SS_VOCAB_MAX_NODES, SS_BOW_MAX_ROWS = 256, 32, 1 << 24, SS_GUIDED_MAX_ROWS

SS_OK = 0
SS_ERR_INVALID_ARG, SS_ERR_NO_DEVICE, SS_ERR_HIP, SS_ERR_TOO_SMALL = -1, -2, -3, -4
SS_ERR_OVERFLOW, SS_ERR_NOT_CALIBRATED, SS_ERR_BAD_FRAME, SS_ERR_NO_MEMORY, SS_ERR_STATE = -5, -6, -7, -8, -9
SS_ERR_BUSY = -10

EXPORTS = ["ss_abi_version", "ss_orb_params_default", "ss_create", "ss_destroy", "ss_last_error",
           "ss_set_calibration", "ss_extract", "ss_extract_batch_device", "ss_get_batch_view", "ss_fetch_frame", "ss_match",
           "ss_match_device", "ss_match_batch_device", "ss_track", "ss_track_reset", "ss_synchronize", "ss_get_stream",
           "ss_profile_enable", "ss_profile_reset", "ss_stats", "ss_debug_fetch", "ss_debug_sort",
           "ss_match_pairs_device", "ss_expand_descriptors_device", "ss_match_expanded_device",
           "ss_match_partial_expanded_device", "ss_track_features", "ss_track_features_matched", "ss_match_partial_device", "ss_match_fold_device", "ss_wait_stream",
           "ss_pipe_create", "ss_pipe_destroy", "ss_pipe_last_error", "ss_pipe_acquire", "ss_pipe_submit",
           "ss_pipe_submit_frames", "ss_pipe_wait", "ss_pipe_poll", "ss_pipe_release", "ss_pipe_in_flight",
           "ss_match_fold_strided_device", "ss_xchg_create", "ss_xchg_destroy", "ss_xchg_last_error", "ss_xchg_status",
           "ss_xchg_allgather", "ss_xchg_broadcast", "ss_pipe_debug_inject_failure", "ss_stereo_exchange_match",
           "ss_match_batch_sources_device", "ss_track_detach", "ss_pipe_match_sources", "ss_stereo_batch_device",
           "ss_extract_stereo", "ss_match_guided_pairs_device", "ss_match_guided_batch_device", "ss_match_guided",
           "ss_rectify_build_map", "ss_rectify_set_map", "ss_rectify_batch_device", "ss_extract_stereo_raw",
           "ss_vocab_load_text", "ss_vocab_from_arrays", "ss_vocab_info", "ss_vocab_copy_out", "ss_vocab_destroy",
           "ss_bow_set_vocabulary", "ss_bow_transform_device", "ss_bow_transform_batch_device", "ss_match_bow_pairs_device",
           "ss_match_bow_batch_device", "ss_bow_score_device", "ss_proj_view_init", "ss_proj_points_host",
           "ss_match_proj_pairs_device", "ss_match_proj_batch_device", "ss_match_proj", "ss_epi_pair_init", "ss_epi_check_host",
           "ss_triangulate_host", "ss_match_epi_pairs_device", "ss_match_epi_batch_device", "ss_triangulate_pairs_device",
           "ss_triangulate_batch_device", "ss_fuse_view_sim3", "ss_fuse_points_host", "ss_fuse_check_host",
           "ss_match_fuse_pairs_device", "ss_match_fuse_batch_device", "ss_match_fuse", "ss_sim3_model_host", "ss_sim3_check_host",
           "ss_sim3_to_view", "ss_sim3_pairs_device", "ss_sim3_batch_device", "ss_sim3", "ss_pose_opt_host", "ss_pose_opt_pairs_device",
           "ss_pose_opt_batch_device", "ss_pose_opt", "ss_sim3_opt_host", "ss_sim3_opt_pairs_device", "ss_sim3_opt_batch_device",
           "ss_sim3_opt", "ss_sim3_marks_pairs_device", "ss_sim3_mutual_pairs_device", "ss_sim3_marks_batch_device",
           "ss_sim3_mutual_batch_device", "ss_sim3_to_view21", "ss_local_ba_host", "ss_local_ba_pairs_device",
           "ss_local_ba_batch_device", "ss_local_ba", "ss_local_ba_points_to_block", "ss_pnp_host", "ss_pnp_model_host", "ss_pnp_check_host",
           "ss_pnp_pairs_device", "ss_pnp_batch_device", "ss_pnp", "ss_pose_graph_host", "ss_pose_graph_edge_host", "ss_graph_atan2_host",
           "ss_graph_ln_host", "ss_pose_graph_device", "ss_pose_graph", "ss_pose_graph_points_device", "ss_global_ba_host",
           "ss_global_ba_obs_from_idx_host", "ss_global_ba_device", "ss_global_ba", "ss_two_view_host", "ss_two_view_model_host",
           "ss_two_view_check_host", "ss_two_view_accept_host", "ss_two_view_beats_host", "ss_two_view_point_tests_host", "ss_two_view_pairs_device", "ss_two_view_batch_device", "ss_two_view",
           "ss_covis_params_default", "ss_covis_set_map", "ss_covis_kf_device", "ss_covis_frames_device", "ss_covis", "ss_covis_kf_host",
           "ss_covis_frames_host", "ss_covis_edges_host", "ss_covis_set_map_rows", "ss_global_ba_rows_from_idx_host", "ss_refresh_params_default",
           "ss_refresh_device", "ss_refresh", "ss_refresh_host", "ss_place_params_default", "ss_place_set_database", "ss_place_query_device",
           "ss_place", "ss_place_query_host", "ss_undistort_bounds_host", "ss_proj_view_set_bounds", "ss_undistort_host",
           "ss_undistort_pairs_device", "ss_undistort_batch_device", "ss_get_batch_raw_xy", "ss_depth_params_from_camera", "ss_depth_host",
           "ss_depth_pairs_device", "ss_depth_batch_device", "ss_unproject_view_init", "ss_unproject_host", "ss_unproject_pairs_device",
           "ss_unproject_batch_device", "ss_unproject", "ss_triangulate_stereo_host", "ss_triangulate_stereo_pairs_device",
           "ss_triangulate_stereo_batch_device"]


class OrbParams(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("scale_factor", C.c_float), ("n_levels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("lapping_x0", C.c_int32),
                ("lapping_x1", C.c_int32), ("max_batch", C.c_int32), ("steer_fma", C.c_int32)]


class Camera(C.Structure):
    _fields_ = [("type", C.c_char * 16), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double),
                ("p2", C.c_double), ("width", C.c_int32), ("height", C.c_int32), ("fps", C.c_double),
                ("rgb", C.c_int32), ("th_depth", C.c_double), ("baseline", C.c_double),
                ("depth_map_factor", C.c_double)]


class FrameResult(C.Structure):
    _fields_ = [("n_keypoints", C.c_int32), ("camera_id", C.c_int32), ("timestamp", C.c_double),
                ("keypoints", C.c_void_p), ("descriptors", C.c_void_p),
                ("level_counts", C.c_int32 * SS_MAX_LEVELS)]


class BatchView(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("kp_capacity", C.c_int32), ("keypoints", C.c_void_p),
                ("descriptors", C.c_void_p), ("n_keypoints", C.c_void_p), ("level_counts", C.c_void_p),
                ("frame_error", C.c_void_p)]


class StageStats(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_int64), ("total_ms", C.c_double),
                ("mean_ms", C.c_double), ("median_ms", C.c_double), ("algorithmic_bytes", C.c_int64)]


class Pose(C.Structure):
    _fields_ = [("tracking_state", C.c_int32), ("camera_id", C.c_int32), ("timestamp", C.c_double),
                ("position", C.c_double * 3), ("quaternion", C.c_double * 4), ("n_keypoints", C.c_int32),
                ("n_matches", C.c_int32), ("n_inliers", C.c_int32), ("n_map_points", C.c_int32)]


class PipeConfig(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32), ("batch", C.c_int32),
                ("depth", C.c_int32), ("match_mode", C.c_int32), ("match_th", C.c_int32), ("ratio_num", C.c_int32),
                ("ratio_den", C.c_int32), ("copy_threads", C.c_int32)]


class PipeSlot(C.Structure):
    _fields_ = [("slot", C.c_int32), ("pixels", C.c_void_p), ("row_stride", C.c_int64), ("frame_stride", C.c_int64)]


class PipeResult(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n_frames", C.c_int32), ("kp_capacity", C.c_int32), ("sequence", C.c_uint64),
                ("status", C.c_void_p), ("camera_id", C.c_void_p), ("timestamp", C.c_void_p),
                ("n_keypoints", C.c_void_p), ("level_counts", C.c_void_p), ("keypoints", C.c_void_p),
                ("descriptors", C.c_void_p), ("match_idx", C.c_void_p), ("match_d1", C.c_void_p),
                ("match_d2", C.c_void_p), ("d_descriptors", C.c_void_p)]


KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4")])


class StereoParams(C.Structure):
    _fields_ = [("fx", C.c_float), ("baseline", C.c_float), ("th_depth", C.c_float)]


class StereoSummary(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_left", C.c_int32), ("n_right", C.c_int32), ("n_matched", C.c_int32),
                ("n_refined", C.c_int32), ("n_depth", C.c_int32), ("n_close", C.c_int32), ("sad_median", C.c_int32)]


# ss_stereo_point: one per left keypoint row
STEREO_POINT_DTYPE = np.dtype([("u_right", "<f4"), ("depth", "<f4"), ("right_idx", "<i4"), ("orb_dist", "<u2"), ("sad", "<u2")])
STEREO_SUMMARY_DTYPE = np.dtype([(n, "<i4") for n, _ in StereoSummary._fields_])


class GuidedParams(C.Structure):
    _fields_ = [("th", C.c_int32), ("ratio_num", C.c_int32), ("ratio_den", C.c_int32), ("one_to_one", C.c_int32),
                ("orientation", C.c_int32), ("radius", C.c_float), ("radius_by_octave", C.c_int32), ("octave_span", C.c_int32),
                ("extent_w", C.c_int32), ("extent_h", C.c_int32)]


class GuidedSummary(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_query", C.c_int32), ("n_train", C.c_int32), ("n_candidates", C.c_int32),
                ("n_accepted", C.c_int32), ("n_unique", C.c_int32), ("n_final", C.c_int32), ("rot_bins", C.c_int32)]


# ss_guided_window: one per query row
GUIDED_WINDOW_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("radius", "<f4"), ("oct_lo", "<i2"), ("oct_hi", "<i2")])
GUIDED_SUMMARY_DTYPE = np.dtype([(n, "<i4") for n, _ in GuidedSummary._fields_])


def guided_params(th: int = 50, ratio_num: int = 9, ratio_den: int = 10, one_to_one: bool = False, orientation: int = 0,
                  radius: float = 0.0, radius_by_octave: bool = False, octave_span: int = 0, extent_w: int = 0,
                  extent_h: int = 0) -> GuidedParams:
    return GuidedParams(th=th, ratio_num=ratio_num, ratio_den=ratio_den, one_to_one=int(one_to_one), orientation=orientation,
                        radius=radius, radius_by_octave=int(radius_by_octave), octave_span=octave_span, extent_w=extent_w,
                        extent_h=extent_h)


class ProjView(C.Structure):
    """ss_proj_view: the pose and intrinsics a frame's map points are projected with, all float32"""
    _fields_ = [("rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float),
                ("min_y", C.c_float), ("max_y", C.c_float)]


class ProjParams(C.Structure):
    _fields_ = [("view_cos_limit", C.c_float), ("th", C.c_float), ("far_limit", C.c_float), ("th_high", C.c_int32),
                ("ratio_num", C.c_int32), ("ratio_den", C.c_int32), ("one_to_one", C.c_int32), ("check_right", C.c_int32),
                ("extent_w", C.c_int32), ("extent_h", C.c_int32)]


class ProjSummary(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_points", C.c_int32), ("n_train", C.c_int32), ("n_in_view", C.c_int32),
                ("n_candidates", C.c_int32), ("n_accepted", C.c_int32), ("n_unique", C.c_int32), ("reserved", C.c_int32)]


PROJ_VIEW_DTYPE = np.dtype([("rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("ow", "<f4", (3,))] +
                           [(n, "<f4") for n in ("fx", "fy", "cx", "cy", "bf", "min_x", "max_x", "min_y", "max_y")])
# ss_map_point: one per map point; ss_proj_point: one per point row of the outputs
MAP_POINT_DTYPE = np.dtype([(n, "<f4") for n in ("x", "y", "z", "nx", "ny", "nz", "min_dist", "max_dist")])
PROJ_POINT_DTYPE = np.dtype([(n, "<f4") for n in ("u", "v", "u_right", "view_cos", "dist", "radius")] + [("level", "<i4"), ("state", "<i4")])
PROJ_SUMMARY_DTYPE = np.dtype([(n, "<i4") for n, _ in ProjSummary._fields_])


def proj_params(view_cos_limit: float = 0.5, th: float = 1.0, far_limit: float = 0.0, th_high: int = 100, ratio_num: int = 8,
                ratio_den: int = 10, one_to_one: bool = False, check_right: bool = False, extent_w: int = 0,
                extent_h: int = 0) -> ProjParams:
    """upstream's SearchLocalPoints: view_cos_limit 0.5, TH_HIGH 100, ratio 8 / 10, th 1 (3 after a relocalisation)"""
    return ProjParams(view_cos_limit=view_cos_limit, th=th, far_limit=far_limit, th_high=th_high, ratio_num=ratio_num,
                      ratio_den=ratio_den, one_to_one=int(one_to_one), check_right=int(check_right), extent_w=extent_w,
                      extent_h=extent_h)


def proj_view(camera: Camera, rcw, tcw, bf: float = 0.0) -> ProjView:
    """ss_proj_view_init: the view of `camera` at pose (rcw 3 x 3 row-major, tcw); needs no device"""
    r = np.ascontiguousarray(rcw, np.float64).reshape(9)
    t = np.ascontiguousarray(tcw, np.float64).reshape(3)
    v = ProjView()
    rc = load().ss_proj_view_init(C.byref(camera), r.ctypes.data, t.ctypes.data, C.c_float(bf), C.byref(v))
    if rc != SS_OK:
        raise OrbError(rc, "ss_proj_view_init refused its arguments")
    return v


def _views_array(views):
    """one ProjView, a sequence of them or a PROJ_VIEW_DTYPE array -> a contiguous PROJ_VIEW_DTYPE array"""
    if isinstance(views, ProjView):
        views = [views]
    if isinstance(views, np.ndarray):
        return np.ascontiguousarray(views, PROJ_VIEW_DTYPE).reshape(-1)
    return np.frombuffer(b"".join(bytes(v) for v in views), PROJ_VIEW_DTYPE).copy()


def proj_points_host(view, params: ProjParams, scale, points: np.ndarray) -> np.ndarray:
    """ss_proj_points_host: frustum, level and window of every map point on the host (the text the kernel compiles) ->
    PROJ_POINT_DTYPE rows; needs no device"""
    v = _views_array(view)
    if len(v) != 1:
        raise ValueError("one view")
    sc = np.ascontiguousarray(scale, np.float32)
    pts = np.ascontiguousarray(points, MAP_POINT_DTYPE)
    out = np.empty(len(pts), PROJ_POINT_DTYPE)
    rc = load().ss_proj_points_host(v.ctypes.data, C.byref(params), sc.ctypes.data, len(sc), pts.ctypes.data if len(pts) else None, len(pts),
                                    out.ctypes.data if len(pts) else None)
    if rc != SS_OK:
        raise OrbError(rc, "ss_proj_points_host refused its arguments")
    return out


SS_FUSE_NONE, SS_FUSE_ADD, SS_FUSE_REPLACE, SS_FUSE_DUPLICATE = 0, 1, 2, 3


class FuseParams(C.Structure):
    _fields_ = [("view_cos_limit", C.c_float), ("th", C.c_float), ("chi2_mono", C.c_float), ("chi2_stereo", C.c_float),
                ("th_low", C.c_int32), ("check_right", C.c_int32), ("extent_w", C.c_int32), ("extent_h", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class FuseSummary(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_points", C.c_int32), ("n_train", C.c_int32), ("n_in_view", C.c_int32),
                ("n_candidates", C.c_int32), ("n_add", C.c_int32), ("n_replace", C.c_int32), ("n_duplicate", C.c_int32)]


# ss_fuse_point and ss_fuse_action: one per point row of the outputs
FUSE_POINT_DTYPE = np.dtype([(n, "<f4") for n in ("u", "v", "u_right", "dot", "dist", "radius")] + [("level", "<i4"), ("state", "<i4")])
FUSE_ACTION_DTYPE = np.dtype([("action", "<i4"), ("other", "<i4")])
FUSE_SUMMARY_DTYPE = np.dtype([(n, "<i4") for n, _ in FuseSummary._fields_])


def fuse_params(view_cos_limit: float = 0.5, th: float = 3.0, chi2_mono: float = 5.99, chi2_stereo: float = 7.8, th_low: int = 50,
                check_right: bool = False, extent_w: int = 0, extent_h: int = 0, reserved=(0, 0)) -> FuseParams:
    """upstream's Fuse in local mapping: 0.5, th 3, chi-square 5.99 / 7.8, TH_LOW 50.  The Sim3 forms: chi2_mono 0 (no chi-square
    test), th 4 (SearchAndFuse) or 8 (the candidate check), th_low 50 or 50 * ratioHamming"""
    return FuseParams(view_cos_limit=view_cos_limit, th=th, chi2_mono=chi2_mono, chi2_stereo=chi2_stereo, th_low=th_low,
                      check_right=int(check_right), extent_w=extent_w, extent_h=extent_h, reserved=(C.c_int32 * 2)(*reserved))


def fuse_view_sim3(camera: Camera, srcw, t, bf: float = 0.0) -> ProjView:
    """ss_fuse_view_sim3: the view of `camera` under upstream's Sim3 Scw = [s.R | t] (srcw 3 x 3 row-major); needs no device"""
    r = np.ascontiguousarray(srcw, np.float64).reshape(9)
    tt = np.ascontiguousarray(t, np.float64).reshape(3)
    v = ProjView()
    rc = load().ss_fuse_view_sim3(C.byref(camera), r.ctypes.data, tt.ctypes.data, C.c_float(bf), C.byref(v))
    if rc != SS_OK:
        raise OrbError(rc, "ss_fuse_view_sim3 refused its arguments")
    return v


def fuse_points_host(view, params: FuseParams, scale, points: np.ndarray, skip=None) -> np.ndarray:
    """ss_fuse_points_host: step 1 of every map point on the host (the text the kernel compiles) -> FUSE_POINT_DTYPE rows; needs no
    device"""
    v = _views_array(view)
    if len(v) != 1:
        raise ValueError("one view")
    sc = np.ascontiguousarray(scale, np.float32)
    pts = np.ascontiguousarray(points, MAP_POINT_DTYPE)
    sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
    if sk is not None and len(sk) != len(pts):
        raise ValueError("one skip flag per point")
    out = np.empty(len(pts), FUSE_POINT_DTYPE)
    rc = load().ss_fuse_points_host(v.ctypes.data, C.byref(params), sc.ctypes.data, len(sc), pts.ctypes.data if len(pts) else None,
                                    None if sk is None or not len(pts) else sk.ctypes.data, len(pts), out.ctypes.data if len(pts) else None)
    if rc != SS_OK:
        raise OrbError(rc, "ss_fuse_points_host refused its arguments")
    return out


def fuse_check_host(params: FuseParams, scale, points: np.ndarray, kp: np.ndarray, right=None, taken=None) -> np.ndarray:
    """ss_fuse_check_host: step 2 of the couples (points[k] FUSE_POINT_DTYPE, kp[k], right[k], taken[k]) on the host (the text the
    kernel compiles) -> uint8, 0 a candidate, else the number 1 .. 4 of the first failing test; needs no device"""
    sc = np.ascontiguousarray(scale, np.float32)
    pts = np.ascontiguousarray(points, FUSE_POINT_DTYPE)
    k = np.ascontiguousarray(kp, KP_DTYPE)
    n = len(pts)
    r = None if right is None else np.ascontiguousarray(right, np.float32)
    tk = None if taken is None else np.ascontiguousarray(taken, np.uint8)
    if len(k) != n or (r is not None and len(r) != n) or (tk is not None and len(tk) != n):
        raise ValueError("one keypoint, right coordinate and taken flag per couple")
    out = np.empty(n, np.uint8)
    rc = load().ss_fuse_check_host(C.byref(params), sc.ctypes.data, len(sc), pts.ctypes.data if n else None, k.ctypes.data if n else None,
                                   None if r is None or not n else r.ctypes.data, None if tk is None or not n else tk.ctypes.data, n,
                                   out.ctypes.data if n else None)
    if rc != SS_OK:
        raise OrbError(rc, "ss_fuse_check_host refused its arguments")
    return out


SS_SIM3_MAX_ITERATIONS = 1024


class Sim3Params(C.Structure):
    _fields_ = [("chi2", C.c_float), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("fix_scale", C.c_int32),
                ("seed", C.c_uint32), ("reserved", C.c_int32 * 3)]


class Sim3Result(C.Structure):
    _fields_ = [("sr12", C.c_float * 9), ("t12", C.c_float * 3), ("s12", C.c_float), ("sr21", C.c_float * 9), ("t21", C.c_float * 3),
                ("state", C.c_int32), ("n_corr", C.c_int32), ("n_inliers", C.c_int32), ("best_inliers", C.c_int32),
                ("iteration", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)]


# ss_sim3_result: one per pair
SIM3_RESULT_DTYPE = np.dtype([("sr12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4"), ("sr21", "<f4", (9,)), ("t21", "<f4", (3,))] +
                             [(n, "<i4") for n in ("state", "n_corr", "n_inliers", "best_inliers", "iteration", "status", "reserved")])


def sim3_params(chi2: float = 9.210, min_inliers: int = 20, max_iterations: int = 300, fix_scale: bool = False, seed: int = 0,
                reserved=(0, 0, 0)) -> Sim3Params:
    """upstream's Sim3Solver::SetRansacParameters(0.99, 20, 300) with th 9.210; fix_scale for stereo and RGB-D"""
    return Sim3Params(chi2=chi2, min_inliers=min_inliers, max_iterations=max_iterations, fix_scale=int(fix_scale), seed=seed & 0xFFFFFFFF,
                      reserved=(C.c_int32 * 3)(*reserved))


def sim3_model_host(params: Sim3Params, x1, x2) -> np.ndarray:
    """ss_sim3_model_host: step 3b for the triple x1[k], x2[k] (3 x 3 float32 camera coordinates, draw order) -> one SIM3_RESULT_DTYPE
    record holding the model; needs no device"""
    a = np.ascontiguousarray(x1, np.float32).reshape(9)
    b = np.ascontiguousarray(x2, np.float32).reshape(9)
    out = np.zeros(1, SIM3_RESULT_DTYPE)
    rc = load().ss_sim3_model_host(C.byref(params), a.ctypes.data, b.ctypes.data, out.ctypes.data)
    if rc != SS_OK:
        raise OrbError(rc, "ss_sim3_model_host refused its arguments")
    return out[0]


def sim3_check_host(params: Sim3Params, view1, view2, scale, points1, kp1, points2, kp2, model):
    """ss_sim3_check_host: steps 1 and 3c of the couples under `model` (a SIM3_RESULT_DTYPE record) -> (uint8 [n]: 0 inlier, 1 octave
    outside the table, 2 first test fails, 3 second; float32 [n][2]: e1, e2); needs no device"""
    v1, v2 = _views_array(view1), _views_array(view2)
    if len(v1) != 1 or len(v2) != 1:
        raise ValueError("one view each")
    sc = np.ascontiguousarray(scale, np.float32)
    p1, p2 = np.ascontiguousarray(points1, MAP_POINT_DTYPE), np.ascontiguousarray(points2, MAP_POINT_DTYPE)
    k1, k2 = np.ascontiguousarray(kp1, KP_DTYPE), np.ascontiguousarray(kp2, KP_DTYPE)
    n = len(p1)
    if len(p2) != n or len(k1) != n or len(k2) != n:
        raise ValueError("one map point and keypoint per side and couple")
    m = np.ascontiguousarray(np.asarray(model, SIM3_RESULT_DTYPE).reshape(1))
    out, err = np.empty(n, np.uint8), np.empty((n, 2), np.float32)
    ptr = lambda a: a.ctypes.data if n else None  # noqa: E731
    rc = load().ss_sim3_check_host(C.byref(params), v1.ctypes.data, v2.ctypes.data, sc.ctypes.data, len(sc), ptr(p1), ptr(k1), ptr(p2), ptr(k2), n,
                                   m.ctypes.data, ptr(out), ptr(err))
    if rc != SS_OK:
        raise OrbError(rc, "ss_sim3_check_host refused its arguments")
    return out, err


def sim3_to_view(camera: Camera, result, rcw2, tcw2, bf: float = 0.0):
    """ss_sim3_to_view: upstream's gScw = gScm * gSmw from a state-0 result and keyframe 2's pose -> (ProjView of keyframe 1's camera
    under it, srcw 3 x 3, t); needs no device"""
    m = np.ascontiguousarray(np.asarray(result, SIM3_RESULT_DTYPE).reshape(1))
    r = np.ascontiguousarray(rcw2, np.float64).reshape(9)
    t = np.ascontiguousarray(tcw2, np.float64).reshape(3)
    srcw, tt, v = np.empty(9, np.float64), np.empty(3, np.float64), ProjView()
    rc = load().ss_sim3_to_view(C.byref(camera), m.ctypes.data, r.ctypes.data, t.ctypes.data, C.c_float(bf), srcw.ctypes.data, tt.ctypes.data,
                                C.byref(v))
    if rc != SS_OK:
        raise OrbError(rc, "ss_sim3_to_view refused its arguments")
    return v, srcw.reshape(3, 3), tt


class Sim3OptParams(C.Structure):
    _fields_ = [("chi2", C.c_double), ("lambda_", C.c_double), ("step_eps", C.c_double), ("iterations0", C.c_int32),
                ("iterations_more", C.c_int32), ("iterations_same", C.c_int32), ("min_corr", C.c_int32), ("min_inliers", C.c_int32),
                ("fix_scale", C.c_int32), ("reserved", C.c_int32 * 4)]


# ss_sim3_opt_result: one per pair; ss_sim3_mutual_summary likewise
SIM3_OPT_RESULT_DTYPE = np.dtype([("r12", "<f8", (9,)), ("t12", "<f8", (3,)), ("s12", "<f8"), ("cost", "<f8")] +
                                 [(n, "<i4") for n in ("state", "status", "n_corr", "n_removed", "n_inliers")] +
                                 [("steps", "<i4", (2,)), ("reserved", "<i4"), ("model", SIM3_RESULT_DTYPE)])
SIM3_MUTUAL_DTYPE = np.dtype([("n_prior", "<i4"), ("n_new", "<i4")])


def sim3_opt_params(chi2: float = 10.0, lambda_: float = 1e-6, step_eps: float = 1e-10, iterations0: int = 5, iterations_more: int = 10,
                    iterations_same: int = 5, min_corr: int = 10, min_inliers: int = 10, fix_scale: bool = False,
                    reserved=(0, 0, 0, 0)) -> Sim3OptParams:
    """upstream's Optimizer::OptimizeSim3 as LoopClosing calls it: th2 10, 5 robust steps, then 10 or 5; lambda and step_eps are the pose
    rule's"""
    return Sim3OptParams(chi2=chi2, lambda_=lambda_, step_eps=step_eps, iterations0=iterations0, iterations_more=iterations_more,
                         iterations_same=iterations_same, min_corr=min_corr, min_inliers=min_inliers, fix_scale=int(fix_scale),
                         reserved=(C.c_int32 * 4)(*reserved))


def _sim3_pair_arrays(view1, q_xyz, q_kp, view2, t_xyz, t_kp, idx, start, q_skip, t_skip):
    """the host arrays of one pair, checked -> (v1, v2, qx, qk, tx, tk, ix, st, q_skip, t_skip, nq, nt)"""
    v1, v2 = _views_array(view1), _views_array(view2)
    qx, tx = np.ascontiguousarray(q_xyz, MAP_POINT_DTYPE), np.ascontiguousarray(t_xyz, MAP_POINT_DTYPE)
    qk, tk = np.ascontiguousarray(q_kp, KP_DTYPE), np.ascontiguousarray(t_kp, KP_DTYPE)
    ix = np.ascontiguousarray(idx, np.int32)
    st = np.ascontiguousarray(np.asarray(start, SIM3_RESULT_DTYPE).reshape(1))
    nq, nt = len(qx), len(tx)
    q_skip = None if q_skip is None else np.ascontiguousarray(q_skip, np.uint8)
    t_skip = None if t_skip is None else np.ascontiguousarray(t_skip, np.uint8)
    if len(v1) != 1 or len(v2) != 1 or len(qk) != nq or len(ix) != nq or len(tk) != nt or (q_skip is not None and len(q_skip) != nq) or \
            (t_skip is not None and len(t_skip) != nt):
        raise ValueError("views, map points, keypoints, flags and matches differ in length")
    return v1, v2, qx, qk, tx, tk, ix, st, q_skip, t_skip, nq, nt


def sim3_opt_host(view1, q_xyz, q_kp, view2, t_xyz, t_kp, idx, start, scale, params: Sim3OptParams, q_skip=None, t_skip=None):
    """ss_sim3_opt_host: the whole rule on the host for one pair -> (uint8 flag per query row: 0 inlier, 1 removed, 2 no correspondence;
    one SIM3_OPT_RESULT_DTYPE record); needs no device"""
    v1, v2, qx, qk, tx, tk, ix, st, q_skip, t_skip, nq, nt = _sim3_pair_arrays(view1, q_xyz, q_kp, view2, t_xyz, t_kp, idx, start, q_skip, t_skip)
    sc = np.ascontiguousarray(scale, np.float32)
    flags, res = np.empty(nq, np.uint8), np.zeros(1, SIM3_OPT_RESULT_DTYPE)
    ptr = lambda a, n: None if a is None or not n else a.ctypes.data  # noqa: E731
    rc = load().ss_sim3_opt_host(v1.ctypes.data, v2.ctypes.data, sc.ctypes.data, len(sc), ptr(qx, nq), ptr(qk, nq), ptr(q_skip, nq), nq, ptr(tx, nt),
                                 ptr(tk, nt), ptr(t_skip, nt), nt, ptr(ix, nq), st.ctypes.data, C.byref(params), ptr(flags, nq), res.ctypes.data)
    if rc != SS_OK:
        raise OrbError(rc, "ss_sim3_opt_host refused its arguments")
    return flags, res[0]


def sim3_to_view21(camera: Camera, result, rcw1, tcw1, bf: float = 0.0):
    """ss_sim3_to_view21: S21.T1w from a state-0 result and keyframe 1's pose -> (ProjView of keyframe 2's camera under it, srcw 3 x 3, t 3);
    needs no device"""
    m = np.ascontiguousarray(np.asarray(result, SIM3_RESULT_DTYPE).reshape(1))
    r, t = np.ascontiguousarray(rcw1, np.float64).reshape(9), np.ascontiguousarray(tcw1, np.float64).reshape(3)
    srcw, tt = np.zeros(9, np.float64), np.zeros(3, np.float64)
    v = ProjView()
    rc = load().ss_sim3_to_view21(C.byref(camera), m.ctypes.data, r.ctypes.data, t.ctypes.data, C.c_float(bf), srcw.ctypes.data, tt.ctypes.data,
                                  C.byref(v))
    if rc != SS_OK:
        raise OrbError(rc, "ss_sim3_to_view21 refused its arguments")
    return v, srcw.reshape(3, 3), tt


class PoseOptParams(C.Structure):
    _fields_ = [("chi2_mono", C.c_double), ("chi2_stereo", C.c_double), ("lambda_", C.c_double), ("step_eps", C.c_double),
                ("n_rounds", C.c_int32), ("iterations", C.c_int32), ("robust_rounds", C.c_int32), ("min_obs", C.c_int32),
                ("check_right", C.c_int32), ("idx_by_row", C.c_int32), ("reserved", C.c_int32 * 2)]


# ss_pose_result: one per frame
POSE_RESULT_DTYPE = np.dtype([("rcw", "<f8", (9,)), ("tcw", "<f8", (3,)), ("cost", "<f8")] +
                             [(n, "<i4") for n in ("state", "status", "n_obs", "n_stereo", "n_inliers")] + [("steps", "<i4", (8,)), ("reserved", "<i4")])


def pose_opt_params(chi2_mono: float = 5.991, chi2_stereo: float = 7.815, lambda_: float = 1e-6, step_eps: float = 1e-10, n_rounds: int = 4,
                    iterations: int = 10, robust_rounds: int = 2, min_obs: int = 3, check_right: bool = False, idx_by_row: bool = False,
                    reserved=(0, 0)) -> PoseOptParams:
    """upstream's Optimizer::PoseOptimization: 4 rounds of 10 steps, chi-square 5.991 / 7.815; lambda, step_eps and robust_rounds are
    the host step's (sst_pose_only)"""
    return PoseOptParams(chi2_mono=chi2_mono, chi2_stereo=chi2_stereo, lambda_=lambda_, step_eps=step_eps, n_rounds=n_rounds,
                         iterations=iterations, robust_rounds=robust_rounds, min_obs=min_obs, check_right=int(check_right),
                         idx_by_row=int(idx_by_row), reserved=(C.c_int32 * 2)(*reserved))


def _start_array(start, n):
    """n start poses, each twelve doubles (rcw row-major, then tcw) -> a contiguous float64 array [n][12]"""
    a = np.ascontiguousarray(start, np.float64).reshape(-1, 12)
    if len(a) != n:
        raise ValueError("one start pose of twelve doubles per frame")
    return a


def pose_opt_host(view, start, scale, points: np.ndarray, kp: np.ndarray, idx: np.ndarray, params: PoseOptParams, skip=None, right=None):
    """ss_pose_opt_host: the whole rule on the host for one frame -> (uint8 flag per slot: 0 inlier, 1 outlier, 2 no observation; one
    POSE_RESULT_DTYPE record); needs no device"""
    v = _views_array(view)
    if len(v) != 1:
        raise ValueError("one view")
    st = _start_array(start, 1)
    sc = np.ascontiguousarray(scale, np.float32)
    pts, k = np.ascontiguousarray(points, MAP_POINT_DTYPE), np.ascontiguousarray(kp, KP_DTYPE)
    ix = np.ascontiguousarray(idx, np.int32)
    n_p, n_k = len(pts), len(k)
    ns = n_k if params.idx_by_row else n_p
    skip = None if skip is None else np.ascontiguousarray(skip, np.uint8)
    right = None if right is None else np.ascontiguousarray(right, np.float32)
    if len(ix) != ns or (skip is not None and len(skip) != n_p) or (right is not None and len(right) != n_k):
        raise ValueError("map points, keypoints, flags and matches differ in length")
    flags, res = np.empty(ns, np.uint8), np.zeros(1, POSE_RESULT_DTYPE)
    ptr = lambda a, n: None if a is None or not n else a.ctypes.data  # noqa: E731
    rc = load().ss_pose_opt_host(v.ctypes.data, st.ctypes.data, sc.ctypes.data, len(sc), ptr(pts, n_p), ptr(skip, n_p), n_p, ptr(k, n_k),
                                 ptr(right, n_k), n_k, ptr(ix, ns), C.byref(params), ptr(flags, ns), res.ctypes.data)
    if rc != SS_OK:
        raise OrbError(rc, "ss_pose_opt_host refused its arguments")
    return flags, res[0]


# ---- PnP RANSAC (the rule: include/sendslam_orb.h) ----
SS_PNP_MAX_ITERATIONS, SS_PNP_MAX_REFINE = 1024, 16


class PnpParams(C.Structure):
    _fields_ = [("chi2", C.c_float), ("min_ratio", C.c_float), ("lambda_", C.c_double), ("min_inliers", C.c_int32),
                ("max_iterations", C.c_int32), ("refine_steps", C.c_int32), ("seed", C.c_uint32), ("reserved", C.c_int32 * 2)]


class PnpResult(C.Structure):
    _fields_ = [("rcw", C.c_double * 9), ("tcw", C.c_double * 3), ("state", C.c_int32), ("status", C.c_int32), ("n_corr", C.c_int32),
                ("n_inliers", C.c_int32), ("best_inliers", C.c_int32), ("iteration", C.c_int32), ("reserved", C.c_int32 * 2)]


# ss_pnp_result: one per problem
PNP_RESULT_DTYPE = np.dtype([("rcw", "<f8", (9,)), ("tcw", "<f8", (3,))] +
                            [(n, "<i4") for n in ("state", "status", "n_corr", "n_inliers", "best_inliers", "iteration")] + [("reserved", "<i4", (2,))])


def pnp_params(chi2: float = 5.991, min_ratio: float = 0.5, lambda_: float = 1e-6, min_inliers: int = 10, max_iterations: int = 300,
               refine_steps: int = 5, seed: int = 0, reserved=(0, 0)) -> PnpParams:
    """upstream's MLPnPsolver::SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991) as Tracking::Relocalization calls it; lambda is the
    pose rule's"""
    return PnpParams(chi2=chi2, min_ratio=min_ratio, lambda_=lambda_, min_inliers=min_inliers, max_iterations=max_iterations,
                     refine_steps=refine_steps, seed=seed & 0xFFFFFFFF, reserved=(C.c_int32 * 2)(*reserved))


def _pnp_arrays(view, points, kp, idx, skip):
    """the host arrays of one problem, checked -> (v, pts, k, ix, skip, n_p, n_k)"""
    v = _views_array(view)
    pts, k = np.ascontiguousarray(points, MAP_POINT_DTYPE), np.ascontiguousarray(kp, KP_DTYPE)
    ix = np.ascontiguousarray(idx, np.int32)
    n_p, n_k = len(pts), len(k)
    skip = None if skip is None else np.ascontiguousarray(skip, np.uint8)
    if len(v) != 1 or len(ix) != n_k or (skip is not None and len(skip) != n_p):
        raise ValueError("view, map points, keypoints, flags and matches differ in length")
    return v, pts, k, ix, skip, n_p, n_k


def pnp_host(view, scale, points: np.ndarray, kp: np.ndarray, idx: np.ndarray, params: PnpParams, skip=None, problem: int = 0):
    """ss_pnp_host: the whole rule on the host for one problem -> (uint8 inlier flag per keypoint row, one PNP_RESULT_DTYPE record); needs
    no device"""
    v, pts, k, ix, skip, n_p, n_k = _pnp_arrays(view, points, kp, idx, skip)
    sc = np.ascontiguousarray(scale, np.float32)
    inlier, res = np.empty(n_k, np.uint8), np.zeros(1, PNP_RESULT_DTYPE)
    ptr = lambda a, n: None if a is None or not n else a.ctypes.data  # noqa: E731
    rc = load().ss_pnp_host(v.ctypes.data, sc.ctypes.data, len(sc), ptr(pts, n_p), ptr(skip, n_p), n_p, ptr(k, n_k), n_k, ptr(ix, n_k),
                            C.byref(params), problem, ptr(inlier, n_k), res.ctypes.data)
    if rc != SS_OK:
        raise OrbError(rc, "ss_pnp_host refused its arguments")
    return inlier, res[0]


def pnp_model_host(params: PnpParams, view, xyz, uv, scale6, point_rows6) -> np.ndarray:
    """ss_pnp_model_host: steps 3b - 3d of one sextuple in draw order (xyz 6 x 3, uv 6 x 2, the six scales and point rows) -> one
    PNP_RESULT_DTYPE record holding the pose; needs no device"""
    v = _views_array(view)
    a = np.ascontiguousarray(xyz, np.float32).reshape(18)
    b = np.ascontiguousarray(uv, np.float32).reshape(12)
    s = np.ascontiguousarray(scale6, np.float32).reshape(6)
    r = np.ascontiguousarray(point_rows6, np.int32).reshape(6)
    out = np.zeros(1, PNP_RESULT_DTYPE)
    rc = load().ss_pnp_model_host(C.byref(params), v.ctypes.data, a.ctypes.data, b.ctypes.data, s.ctypes.data, r.ctypes.data, out.ctypes.data)
    if rc != SS_OK:
        raise OrbError(rc, "ss_pnp_model_host refused its arguments")
    return out[0]


def pnp_check_host(params: PnpParams, view, scale, points, kp, model):
    """ss_pnp_check_host: steps 1 and 3e of the couples under `model` (a PNP_RESULT_DTYPE record) -> (uint8 [n]: 0 inlier, 1 octave
    outside the table, 2 depth not > 0, 3 error not < max; float32 [n]: the squared error); needs no device"""
    v = _views_array(view)
    sc = np.ascontiguousarray(scale, np.float32)
    pts, k = np.ascontiguousarray(points, MAP_POINT_DTYPE), np.ascontiguousarray(kp, KP_DTYPE)
    n = len(pts)
    if len(v) != 1 or len(k) != n:
        raise ValueError("one view; one map point and keypoint per couple")
    m = np.ascontiguousarray(np.asarray(model, PNP_RESULT_DTYPE).reshape(1))
    out, err = np.empty(n, np.uint8), np.empty(n, np.float32)
    ptr = lambda a: a.ctypes.data if n else None  # noqa: E731
    rc = load().ss_pnp_check_host(C.byref(params), v.ctypes.data, sc.ctypes.data, len(sc), ptr(pts), ptr(k), n, m.ctypes.data, ptr(out), ptr(err))
    if rc != SS_OK:
        raise OrbError(rc, "ss_pnp_check_host refused its arguments")
    return out, err


# ---- two-view initialisation (the rule: include/sendslam_orb.h) ----
SS_TWO_VIEW_MAX_ITERATIONS = 1024
SS_TWO_VIEW_COS_1DEG = 0.9998476951563913


class TwoViewParams(C.Structure):
    _fields_ = [("chi2_h", C.c_double), ("chi2_f", C.c_double), ("chi2_score", C.c_double), ("rh_threshold", C.c_double),
                ("cos_min_parallax", C.c_double), ("min_triangulated", C.c_int32), ("max_iterations", C.c_int32), ("seed", C.c_uint32),
                ("reserved", C.c_int32 * 3)]


# ss_two_view_result: one per problem
TWO_VIEW_RESULT_DTYPE = np.dtype([("r21", "<f8", (9,)), ("t21", "<f8", (3,)), ("score_h", "<f8"), ("score_f", "<f8"), ("cos_parallax", "<f8")] +
                                 [(n, "<i4") for n in ("state", "reason", "status", "model", "iteration_h", "iteration_f", "n_corr", "n_inliers",
                                                       "n_good", "n_triangulated")] + [("reserved", "<i4", (8,))])


def two_view_params(chi2_h: float = 5.991, chi2_f: float = 3.841, chi2_score: float = 5.991, rh_threshold: float = 0.45,
                    cos_min_parallax: float = SS_TWO_VIEW_COS_1DEG, min_triangulated: int = 50, max_iterations: int = 200, seed: int = 0,
                    reserved=(0, 0, 0)) -> TwoViewParams:
    """upstream's TwoViewReconstruction(K, 1.0, 200) with its thresholds; rh_threshold is ss_track's 0.45 (upstream's source: 0.50)"""
    return TwoViewParams(chi2_h=chi2_h, chi2_f=chi2_f, chi2_score=chi2_score, rh_threshold=rh_threshold, cos_min_parallax=cos_min_parallax,
                         min_triangulated=min_triangulated, max_iterations=max_iterations, seed=seed & 0xFFFFFFFF,
                         reserved=(C.c_int32 * 3)(*reserved))


def _two_view_arrays(view, kp1, kp2, idx):
    """the host arrays of one problem, checked -> (v, k1, k2, ix, n1, n2)"""
    v = _views_array(view)
    k1, k2 = np.ascontiguousarray(kp1, KP_DTYPE), np.ascontiguousarray(kp2, KP_DTYPE)
    ix = np.ascontiguousarray(idx, np.int32)
    if len(v) != 1 or len(ix) != len(k1):
        raise ValueError("one view; one match per row of frame 1")
    return v, k1, k2, ix, len(k1), len(k2)


def _two_view_outputs(n1):
    return (np.empty(n1, np.uint8), np.zeros(n1, MAP_POINT_DTYPE), np.full((n1, 2), -1, np.int32), np.zeros(1, np.int32),
            np.zeros(1, TWO_VIEW_RESULT_DTYPE))


def two_view_host(view, scale, kp1: np.ndarray, kp2: np.ndarray, idx: np.ndarray, params: TwoViewParams, problem: int = 0):
    """ss_two_view_host: the whole rule on the host for one problem -> (uint8 flag per row of frame 1, the triangulated MAP_POINT_DTYPE
    points, their int32 rows (i, j), one TWO_VIEW_RESULT_DTYPE record); needs no device"""
    v, k1, k2, ix, n1, n2 = _two_view_arrays(view, kp1, kp2, idx)
    sc = np.ascontiguousarray(scale, np.float32)
    flag, pts, rows, n_pts, res = _two_view_outputs(n1)
    ptr = lambda a, n: a.ctypes.data if n else None  # noqa: E731
    rc = load().ss_two_view_host(v.ctypes.data, sc.ctypes.data, len(sc), ptr(k1, n1), n1, ptr(k2, n2), n2, ptr(ix, n1), C.byref(params), problem,
                                 ptr(flag, n1), ptr(pts, n1), ptr(rows, n1), n_pts.ctypes.data, res.ctypes.data)
    if rc != SS_OK:
        raise OrbError(rc, "ss_two_view_host refused its arguments")
    return flag, pts[:n_pts[0]], rows[:n_pts[0]], res[0]


def two_view_model_host(uv):
    """ss_two_view_model_host: steps 2 and 3 of one octuple (8 x 4 float32: u1 v1 u2 v2) normalised by itself -> (H21, H12, F21 as 3 x 3
    float64, (ok_h, ok_f)); needs no device"""
    a = np.ascontiguousarray(uv, np.float32).reshape(32)
    h21, h12, f21, ok = np.zeros(9), np.zeros(9), np.zeros(9), np.zeros(2, np.int32)
    rc = load().ss_two_view_model_host(a.ctypes.data, h21.ctypes.data, h12.ctypes.data, f21.ctypes.data, ok.ctypes.data)
    if rc != SS_OK:
        raise OrbError(rc, "ss_two_view_model_host refused its arguments")
    return h21.reshape(3, 3), h12.reshape(3, 3), f21.reshape(3, 3), (int(ok[0]), int(ok[1]))


def two_view_check_host(params: TwoViewParams, view, uv, h21=None, h12=None, f21=None, r21=None, t21=None) -> dict:
    """ss_two_view_check_host: steps 4 and 8 of n correspondences (n x 4 float32) under the models and the motion given -> a dict of
    chi_h / in_h / score_h, chi_f / in_f / score_f, good / cos / xyz for whichever were given; needs no device"""
    v = _views_array(view)
    a = np.ascontiguousarray(uv, np.float32).reshape(-1, 4)
    n = len(a)
    f8 = lambda m, k: None if m is None else np.ascontiguousarray(m, np.float64).reshape(k)  # noqa: E731
    h21, h12, f21, r21, t21 = f8(h21, 9), f8(h12, 9), f8(f21, 9), f8(r21, 9), f8(t21, 3)
    out = {"chi_h": np.zeros((n, 2)), "in_h": np.zeros(n, np.uint8), "score_h": np.zeros(1), "chi_f": np.zeros((n, 2)),
           "in_f": np.zeros(n, np.uint8), "score_f": np.zeros(1), "good": np.zeros(n, np.uint8), "cos": np.zeros(n), "xyz": np.zeros((n, 3))}
    ptr = lambda m: None if m is None else m.ctypes.data  # noqa: E731
    rc = load().ss_two_view_check_host(C.byref(params), v.ctypes.data, a.ctypes.data if n else None, n, ptr(h21), ptr(h12), ptr(f21), ptr(r21),
                                       ptr(t21), *[out[k].ctypes.data for k in ("chi_h", "in_h", "score_h", "chi_f", "in_f", "score_f", "good",
                                                                                 "cos", "xyz")])
    if rc != SS_OK:
        raise OrbError(rc, "ss_two_view_check_host refused its arguments")
    out["score_h"], out["score_f"] = float(out["score_h"][0]), float(out["score_f"][0])
    return out


def two_view_accept_host(params: TwoViewParams, model: int, good, n_in: int, cos_parallax: float):
    """ss_two_view_accept_host: steps 8 and 9 on the hypotheses' counts -> (reason, best hypothesis, its count, the second count)"""
    g = np.ascontiguousarray(good, np.int32)
    out = np.zeros(4, np.int32)
    rc = load().ss_two_view_accept_host(C.byref(params), model, g.ctypes.data, len(g), n_in, C.c_double(cos_parallax), out.ctypes.data)
    if rc != SS_OK:
        raise OrbError(rc, "ss_two_view_accept_host refused its arguments")
    return tuple(int(v) for v in out)


def two_view_beats_host(score: float, t: int, best: float, best_t: int) -> bool:
    """ss_two_view_beats_host: step 5's order"""
    return bool(load().ss_two_view_beats_host(C.c_double(score), t, C.c_double(best), best_t))


def two_view_point_tests_host(cos_parallax: float, err_sq: float):
    """ss_two_view_point_tests_host: step 8's tests on numbers -> (triangulated, exempt from the depth tests, within 4 sigma^2)"""
    out = np.zeros(3, np.int32)
    rc = load().ss_two_view_point_tests_host(C.c_double(cos_parallax), C.c_double(err_sq), out.ctypes.data)
    if rc != SS_OK:
        raise OrbError(rc, "ss_two_view_point_tests_host refused its arguments")
    return tuple(bool(v) for v in out)


# ---- local bundle adjustment (the rule: include/sendslam_orb.h) ----
SS_BA_MAX_KF, SS_BA_MAX_FREE, SS_BA_MAX_ROUNDS = 64, 32, 4


class BaParams(C.Structure):
    _fields_ = [("chi2_mono", C.c_double), ("chi2_stereo", C.c_double), ("lambda_", C.c_double), ("lambda_factor", C.c_double),
                ("lambda_min", C.c_double), ("step_eps", C.c_double), ("n_rounds", C.c_int32), ("iterations", C.c_int32 * 4),
                ("robust_rounds", C.c_int32), ("min_point_obs", C.c_int32), ("check_right", C.c_int32), ("reserved", C.c_int32 * 4)]


# ss_ba_problem: one per problem (a host table); ss_ba_result: one per problem
BA_PROBLEM_DTYPE = np.dtype([(n, "<i4") for n in ("first_frame", "n_kf", "n_free", "point_block")])
BA_RESULT_DTYPE = np.dtype([("lambda_", "<f8"), ("cost_before", "<f8"), ("cost_after", "<f8")] +
                           [(n, "<i4") for n in ("state", "status", "n_obs", "n_stereo", "n_inliers", "n_points_active", "n_frozen_max")] +
                           [("steps", "<i4", (4,)), ("accepted", "<i4", (4,)), ("reserved", "<i4")])


def ba_params(chi2_mono: float = 5.991, chi2_stereo: float = 7.815, lambda_: float = 1e-4, lambda_factor: float = 10.0, lambda_min: float = 1e-9,
              step_eps: float = 1e-10, n_rounds: int = 2, iterations=(5, 10, 0, 0), robust_rounds: int = 1, min_point_obs: int = 2,
              check_right: bool = False, reserved=(0, 0, 0, 0)) -> BaParams:
    """ORB-SLAM2's LocalBundleAdjustment schedule: 5 robust iterations, classification, 10 plain ones on the inliers; ORB-SLAM3's single
    robust round of 10 is n_rounds=1, iterations=(10,), robust_rounds=1"""
    its = tuple(iterations) + (0,) * (4 - len(tuple(iterations)))
    return BaParams(chi2_mono=chi2_mono, chi2_stereo=chi2_stereo, lambda_=lambda_, lambda_factor=lambda_factor, lambda_min=lambda_min,
                    step_eps=step_eps, n_rounds=n_rounds, iterations=(C.c_int32 * 4)(*its), robust_rounds=robust_rounds,
                    min_point_obs=min_point_obs, check_right=int(check_right), reserved=(C.c_int32 * 4)(*reserved))


def _ba_host_arrays(views, start, points, kp, idx, n_kp, skip, right):
    """the arrays of one problem, checked against each other: kp [n_kf][rows], idx [n_kf][n_points]"""
    v = _views_array(views)
    n_kf = len(v)
    st = _start_array(start, n_kf)
    pts, k = np.ascontiguousarray(points, MAP_POINT_DTYPE), np.ascontiguousarray(kp, KP_DTYPE)
    n_p = len(pts)
    if k.ndim != 2 or len(k) != n_kf or k.shape[1] < 1:
        raise ValueError("keypoints are [n_kf][rows_per_frame]")
    ix = np.ascontiguousarray(idx, np.int32).reshape(n_kf, n_p)
    nk = np.full(n_kf, k.shape[1], np.int32) if n_kp is None else np.ascontiguousarray(n_kp, np.int32)
    skip = None if skip is None else np.ascontiguousarray(skip, np.uint8)
    right = None if right is None else np.ascontiguousarray(right, np.float32)
    if len(nk) != n_kf or (skip is not None and len(skip) != n_p) or (right is not None and right.shape != k.shape):
        raise ValueError("views, map points, keypoints, counts and matches differ in length")
    return v, st, pts, k, ix, nk, skip, right


def local_ba_host(views, start, n_free: int, scale, points: np.ndarray, kp: np.ndarray, idx: np.ndarray, params: BaParams, n_kp=None, skip=None,
                  right=None):
    """ss_local_ba_host: the whole rule on the host for one problem -> (poses float64 [n_kf][12], xyz float64 [n_points][3], uint8 point
    flags, uint8 observation flags [n_kf][n_points], one BA_RESULT_DTYPE record); needs no device"""
    v, st, pts, k, ix, nk, skip, right = _ba_host_arrays(views, start, points, kp, idx, n_kp, skip, right)
    sc = np.ascontiguousarray(scale, np.float32)
    n_kf, n_p = len(v), len(pts)
    poses, xyz = np.empty((n_kf, 12), np.float64), np.empty((n_p, 3), np.float64)
    pf, of, res = np.empty(n_p, np.uint8), np.empty((n_kf, n_p), np.uint8), np.zeros(1, BA_RESULT_DTYPE)
    ptr = lambda a, n: None if a is None or not n else a.ctypes.data  # noqa: E731
    rc = load().ss_local_ba_host(v.ctypes.data, st.ctypes.data, n_kf, n_free, sc.ctypes.data, len(sc), ptr(pts, n_p), ptr(skip, n_p), n_p,
                                 k.ctypes.data, ptr(right, 1), nk.ctypes.data, k.shape[1], ptr(ix, n_p), C.byref(params), poses.ctypes.data,
                                 ptr(xyz, n_p), ptr(pf, n_p), ptr(of, n_p), res.ctypes.data)
    if rc != SS_OK:
        raise OrbError(rc, "ss_local_ba_host refused its arguments")
    return poses, xyz, pf, of, res[0]


# ---- essential-graph optimisation (the rule: include/sendslam_orb.h) ----
SS_GRAPH_MAX_KF, SS_GRAPH_MAX_EDGES = 16384, 131072


class GraphParams(C.Structure):
    _fields_ = [("lambda_", C.c_double), ("lambda_factor", C.c_double), ("lambda_min", C.c_double), ("pcg_tol", C.c_double),
                ("iterations", C.c_int32), ("pcg_iterations", C.c_int32), ("fix_scale", C.c_int32), ("reserved", C.c_int32)]


# ss_graph_problem: one per problem (a host table); ss_graph_result: one per problem
GRAPH_PROBLEM_DTYPE = np.dtype([(n, "<i4") for n in ("first_kf", "n_kf", "first_edge", "n_edges")])
GRAPH_RESULT_DTYPE = np.dtype([("lambda_", "<f8"), ("cost_before", "<f8"), ("cost_after", "<f8")] +
                              [(n, "<i4") for n in ("state", "n_edges", "n_free", "steps", "accepted", "pcg_iterations")])


def graph_params(lambda_: float = 1e-16, lambda_factor: float = 10.0, lambda_min: float = 0.0, pcg_tol: float = 1e-2, iterations: int = 20,
                 pcg_iterations: int = 128, fix_scale: bool = False, reserved: int = 0) -> GraphParams:
    """upstream's OptimizeEssentialGraph: 20 Levenberg-Marquardt iterations from lambda 1e-16; fix_scale is its bFixScale (stereo, RGB-D)"""
    return GraphParams(lambda_=lambda_, lambda_factor=lambda_factor, lambda_min=lambda_min, pcg_tol=pcg_tol, iterations=iterations,
                       pcg_iterations=pcg_iterations, fix_scale=int(fix_scale), reserved=reserved)


def _graph_host_arrays(nc, start, fixed, edges):
    """the arrays of one problem, checked against each other: nc, start [n_kf][13], fixed [n_kf], edges [n_edges][2]"""
    nc = np.ascontiguousarray(nc, np.float64).reshape(-1, 13)
    st = np.ascontiguousarray(start, np.float64).reshape(-1, 13)
    fx = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
    ed = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
    if len(st) != len(nc) or len(fx) != len(nc):
        raise ValueError("one non-corrected Sim3, one start and one fixed byte per keyframe")
    return nc, st, fx, ed


def pose_graph_host(nc, start, fixed, edges, params: GraphParams):
    """ss_pose_graph_host: the whole rule on the host for one problem -> (sim3 float64 [n_kf][13], poses float64 [n_kf][12], one
    GRAPH_RESULT_DTYPE record); needs no device"""
    nc, st, fx, ed = _graph_host_arrays(nc, start, fixed, edges)
    n_kf = len(nc)
    sim3, poses, res = np.empty((n_kf, 13), np.float64), np.empty((n_kf, 12), np.float64), np.zeros(1, GRAPH_RESULT_DTYPE)
    rc = load().ss_pose_graph_host(nc.ctypes.data, st.ctypes.data, fx.ctypes.data, n_kf, ed.ctypes.data if len(ed) else None, len(ed),
                                   C.byref(params), sim3.ctypes.data, poses.ctypes.data, res.ctypes.data)
    if rc != SS_OK:
        raise OrbError(rc, "ss_pose_graph_host refused its arguments")
    return sim3, poses, res[0]


def pose_graph_edge_host(nc_i, nc_j, s_i, s_j, fixed_i: bool = False, fixed_j: bool = False, fix_scale: bool = False):
    """ss_pose_graph_edge_host: one edge -> (e float64 [7], J float64 [14][7]: row c is column c of the 7 x 14 block)"""
    a = [np.ascontiguousarray(v, np.float64).reshape(13) for v in (nc_i, nc_j, s_i, s_j)]
    e, J = np.empty(7, np.float64), np.empty((14, 7), np.float64)
    rc = load().ss_pose_graph_edge_host(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, int(fixed_i), int(fixed_j),
                                        int(fix_scale), e.ctypes.data, J.ctypes.data)
    if rc != SS_OK:
        raise OrbError(rc, "ss_pose_graph_edge_host refused its arguments")
    return e, J


def graph_atan2_host(y, x) -> np.ndarray:
    """ss_graph_atan2_host: the library's series for atan2(y, x), y >= 0, elementwise"""
    y, x = np.ascontiguousarray(y, np.float64).reshape(-1), np.ascontiguousarray(x, np.float64).reshape(-1)
    if len(y) != len(x):
        raise ValueError("one x per y")
    out = np.empty(len(y), np.float64)
    rc = load().ss_graph_atan2_host(y.ctypes.data, x.ctypes.data, len(y), out.ctypes.data) if len(y) else SS_OK
    if rc != SS_OK:
        raise OrbError(rc, "ss_graph_atan2_host refused its arguments")
    return out


def graph_ln_host(x) -> np.ndarray:
    """ss_graph_ln_host: the library's series for ln(x), x > 0, elementwise"""
    x = np.ascontiguousarray(x, np.float64).reshape(-1)
    out = np.empty(len(x), np.float64)
    rc = load().ss_graph_ln_host(x.ctypes.data, len(x), out.ctypes.data) if len(x) else SS_OK
    if rc != SS_OK:
        raise OrbError(rc, "ss_graph_ln_host refused its arguments")
    return out


class EpiPair(C.Structure):
    """ss_epi_pair: a (keyframe 1 = query, keyframe 2 = train) pair; float32 for the search, double for the triangulation"""
    _fields_ = [("f12", C.c_float * 9), ("ex", C.c_float), ("ey", C.c_float), ("epipole_test", C.c_int32)] + \
               [(n + s, C.c_double * k) for s in ("1", "2") for n, k in (("rcw", 9), ("tcw", 3), ("ow", 3))] + \
               [(n + s, C.c_double) for s in ("1", "2") for n in ("fx", "fy", "cx", "cy", "invfx", "invfy")]


class EpiParams(C.Structure):
    _fields_ = [("th", C.c_int32), ("coarse", C.c_int32), ("one_to_one", C.c_int32), ("orientation", C.c_int32)]


class EpiSummary(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_query", C.c_int32), ("n_train", C.c_int32), ("n_candidates", C.c_int32),
                ("n_geometric", C.c_int32), ("n_near", C.c_int32), ("n_accepted", C.c_int32), ("n_unique", C.c_int32),
                ("n_final", C.c_int32), ("rot_bins", C.c_int32)]


class TriParams(C.Structure):
    _fields_ = [("cos_parallax_max", C.c_double), ("chi2", C.c_double), ("ratio_factor", C.c_double), ("far_limit", C.c_double)]


class TriSummary(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_query", C.c_int32), ("n_train", C.c_int32), ("n_matches", C.c_int32),
                ("n_points", C.c_int32), ("n_state", C.c_int32 * 11)]


EPI_PAIR_DTYPE = np.dtype([("f12", "<f4", (9,)), ("ex", "<f4"), ("ey", "<f4"), ("epipole_test", "<i4")] +
                          [(n + s, "<f8", (k,)) for s in ("1", "2") for n, k in (("rcw", 9), ("tcw", 3), ("ow", 3))] +
                          [(n + s, "<f8") for s in ("1", "2") for n in ("fx", "fy", "cx", "cy", "invfx", "invfy")])
EPI_SUMMARY_DTYPE = np.dtype([(n, "<i4") for n, _ in EpiSummary._fields_])
# ss_tri_info: one per query row; ss_tri_summary: one per pair
TRI_INFO_DTYPE = np.dtype([("state", "<i4"), ("cos_parallax", "<f4"), ("err1_sq", "<f4"), ("err2_sq", "<f4")])
TRI_SUMMARY_DTYPE = np.dtype([(n, "<i4") for n, _ in TriSummary._fields_[:5]] + [("n_state", "<i4", (11,))])


def epi_params(th: int = 50, coarse: bool = False, one_to_one: bool = False, orientation: int = 1) -> EpiParams:
    """upstream's SearchForTriangulation: TH_LOW 50, bCoarse false, the rotation histogram on"""
    return EpiParams(th=th, coarse=int(coarse), one_to_one=int(one_to_one), orientation=orientation)


def tri_params(cos_parallax_max: float = 0.9998, chi2: float = 5.991, ratio_factor: float = 1.5 * 1.2, far_limit: float = 0.0) -> TriParams:
    """upstream's CreateNewMapPoints: 0.9998, 5.991, ratio_factor = 1.5f * scale_factor, no far limit"""
    return TriParams(cos_parallax_max=cos_parallax_max, chi2=chi2, ratio_factor=ratio_factor, far_limit=far_limit)


def epi_pair(cam1: Camera, rcw1, tcw1, cam2: Camera, rcw2, tcw2) -> EpiPair:
    """ss_epi_pair_init: the pair of `cam1` at pose 1 (query side) and `cam2` at pose 2 (train side); needs no device"""
    r1, t1 = np.ascontiguousarray(rcw1, np.float64).reshape(9), np.ascontiguousarray(tcw1, np.float64).reshape(3)
    r2, t2 = np.ascontiguousarray(rcw2, np.float64).reshape(9), np.ascontiguousarray(tcw2, np.float64).reshape(3)
    w = EpiPair()
    rc = load().ss_epi_pair_init(C.byref(cam1), r1.ctypes.data, t1.ctypes.data, C.byref(cam2), r2.ctypes.data, t2.ctypes.data, C.byref(w))
    if rc != SS_OK:
        raise OrbError(rc, "ss_epi_pair_init refused its arguments")
    return w


def _pairs_array(pairs):
    """one EpiPair, a sequence of them or an EPI_PAIR_DTYPE array -> a contiguous EPI_PAIR_DTYPE array"""
    if isinstance(pairs, EpiPair):
        pairs = [pairs]
    if isinstance(pairs, np.ndarray):
        return np.ascontiguousarray(pairs, EPI_PAIR_DTYPE).reshape(-1)
    return np.frombuffer(b"".join(bytes(v) for v in pairs), EPI_PAIR_DTYPE).copy()


def _one_pair_couples(pair, scale, kp1, kp2):
    w = _pairs_array(pair)
    if len(w) != 1:
        raise ValueError("one pair")
    k1, k2 = np.ascontiguousarray(kp1, KP_DTYPE), np.ascontiguousarray(kp2, KP_DTYPE)
    if len(k1) != len(k2):
        raise ValueError("one keypoint of each side per couple")
    return w, np.ascontiguousarray(scale, np.float32), k1, k2


def epi_check_host(pair, params: EpiParams, scale, kp1: np.ndarray, kp2: np.ndarray) -> np.ndarray:
    """ss_epi_check_host: tests 1 - 3 of the couples (kp1[k], kp2[k]) on the host (the text the kernel compiles) -> uint8, 0 pass,
    1 octave, 2 epipole, 3 line; needs no device"""
    w, sc, k1, k2 = _one_pair_couples(pair, scale, kp1, kp2)
    n = len(k1)
    out = np.empty(n, np.uint8)
    rc = load().ss_epi_check_host(w.ctypes.data, C.byref(params), sc.ctypes.data, len(sc), k1.ctypes.data if n else None,
                                  k2.ctypes.data if n else None, n, out.ctypes.data if n else None)
    if rc != SS_OK:
        raise OrbError(rc, "ss_epi_check_host refused its arguments")
    return out


def triangulate_host(pair, params: TriParams, scale, kp1: np.ndarray, kp2: np.ndarray):
    """ss_triangulate_host: the triangulation of the couples (kp1[k], kp2[k]) on the host -> (MAP_POINT_DTYPE rows, TRI_INFO_DTYPE
    rows); needs no device"""
    w, sc, k1, k2 = _one_pair_couples(pair, scale, kp1, kp2)
    n = len(k1)
    pts, info = np.empty(n, MAP_POINT_DTYPE), np.empty(n, TRI_INFO_DTYPE)
    rc = load().ss_triangulate_host(w.ctypes.data, C.byref(params), sc.ctypes.data, len(sc), k1.ctypes.data if n else None,
                                    k2.ctypes.data if n else None, n, pts.ctypes.data if n else None, info.ctypes.data if n else None)
    if rc != SS_OK:
        raise OrbError(rc, "ss_triangulate_host refused its arguments")
    return pts, info


class TriStereoRig(C.Structure):
    """ss_tri_stereo_rig: b the baseline in metres (upstream's mb), bf = b * fx, of both sides of a pair"""
    _fields_ = [("bf1", C.c_double), ("b1", C.c_double), ("bf2", C.c_double), ("b2", C.c_double)]


class TriStereoParams(C.Structure):
    _fields_ = [("tri", TriParams), ("chi2_stereo", C.c_double)]


TRI_STEREO_RIG_DTYPE = np.dtype([(n, "<f8") for n in ("bf1", "b1", "bf2", "b2")])
TRI_STEREO_INFO_DTYPE = np.dtype([("state", "<i4"), ("mode", "<i4"), ("cos_rays", "<f4"), ("cs1", "<f4"), ("cs2", "<f4"), ("err1_sq", "<f4"),
                                  ("err2_sq", "<f4"), ("reserved", "<i4")])
TRI_STEREO_SUMMARY_DTYPE = np.dtype(TRI_SUMMARY_DTYPE.descr + [("n_mode", "<i4", (3,)), ("reserved", "<i4")])


def tri_stereo_params(chi2_stereo: float = 7.8, **tri) -> TriStereoParams:
    """upstream's CreateNewMapPoints: tri_params() and 7.8 for a stereo side"""
    return TriStereoParams(tri=tri_params(**tri), chi2_stereo=chi2_stereo)


def _rigs_array(rigs):
    """one TriStereoRig, a sequence of them or a TRI_STEREO_RIG_DTYPE array -> a contiguous TRI_STEREO_RIG_DTYPE array"""
    if isinstance(rigs, TriStereoRig):
        rigs = [rigs]
    if isinstance(rigs, np.ndarray):
        return np.ascontiguousarray(rigs, TRI_STEREO_RIG_DTYPE).reshape(-1)
    return np.frombuffer(b"".join(bytes(v) for v in rigs), TRI_STEREO_RIG_DTYPE).copy()


def triangulate_stereo_host(pair, rig: TriStereoRig, params: TriStereoParams, scale, kp1, kp2, depth1=None, right1=None, depth2=None, right2=None):
    """ss_triangulate_stereo_host: the couples (kp1[k], kp2[k]) with the depth and right coordinate of each side (float32 [n]; all None:
    every row mono) -> (MAP_POINT_DTYPE rows, TRI_STEREO_INFO_DTYPE rows); needs no device"""
    w, sc, k1, k2 = _one_pair_couples(pair, scale, kp1, kp2)
    n = len(k1)
    planes = [None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1) for a in (depth1, right1, depth2, right2)]
    if any(a is not None and len(a) != n for a in planes):
        raise ValueError("one depth and right coordinate per couple")
    pts, info = np.empty(n, MAP_POINT_DTYPE), np.empty(n, TRI_STEREO_INFO_DTYPE)
    ptr = lambda a: a.ctypes.data if a is not None and n else None  # noqa: E731
    rc = load().ss_triangulate_stereo_host(w.ctypes.data, C.byref(rig), C.byref(params), sc.ctypes.data, len(sc), ptr(k1), ptr(k2), *[ptr(a) for a in planes],
                                           n, ptr(pts), ptr(info))
    if rc != SS_OK:
        raise OrbError(rc, "ss_triangulate_stereo_host refused its arguments")
    return pts, info


class VocabShape(C.Structure):
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("n_nodes", C.c_int32), ("n_words", C.c_int32), ("max_depth", C.c_int32)]


class BowSummary(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_rows", C.c_int32), ("n_used", C.c_int32), ("n_words", C.c_int32),
                ("n_nodes", C.c_int32), ("reserved", C.c_int32), ("norm", C.c_double)]


BOW_SUMMARY_DTYPE = np.dtype([(n, "<i4") for n, _ in BowSummary._fields_[:6]] + [("norm", "<f8")])


class RectifyModel(C.Structure):
    """ss_rectify_model: raw intrinsics, distortion in OpenCV's order, the rectifying rotation (row-major), the new intrinsics"""
    _fields_ = [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")] + [("R", C.c_double * 9)] + \
               [(n, C.c_double) for n in ("fx_new", "fy_new", "cx_new", "cy_new")] + [("width", C.c_int32), ("height", C.c_int32)]


def rectify_model(fx, fy, cx, cy, k1, k2, p1, p2, k3, R, fx_new, fy_new, cx_new, cy_new, width, height) -> RectifyModel:
    m = RectifyModel(fx=fx, fy=fy, cx=cx, cy=cy, k1=k1, k2=k2, p1=p1, p2=p2, k3=k3, fx_new=fx_new, fy_new=fy_new, cx_new=cx_new,
                     cy_new=cy_new, width=int(width), height=int(height))
    m.R[:] = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
    return m


# ---- global bundle adjustment (the rule: include/sendslam_orb.h) ----
SS_GBA_MAX_KF, SS_GBA_MAX_POINTS, SS_GBA_MAX_OBS = 16384, 1048576, 4194304


class GbaParams(C.Structure):
    _fields_ = [("chi2_mono", C.c_double), ("chi2_stereo", C.c_double), ("lambda_", C.c_double), ("lambda_factor", C.c_double),
                ("lambda_min", C.c_double), ("step_eps", C.c_double), ("pcg_tol", C.c_double), ("n_rounds", C.c_int32),
                ("iterations", C.c_int32 * 4), ("robust_rounds", C.c_int32), ("min_point_obs", C.c_int32), ("check_right", C.c_int32),
                ("pcg_iterations", C.c_int32), ("reserved", C.c_int32 * 3)]


# ss_gba_obs: one per observation record; ss_gba_problem: one per problem (host tables); ss_gba_result: one per problem
GBA_OBS_DTYPE = np.dtype([("kf", "<i4"), ("point", "<i4"), ("u", "<f4"), ("v", "<f4"), ("right", "<f4"), ("octave", "<i4")])
GBA_PROBLEM_DTYPE = np.dtype([(n, "<i4") for n in ("first_kf", "n_kf", "first_block", "n_blocks", "first_obs", "n_obs")] + [("reserved", "<i4", (2,))])
GBA_RESULT_DTYPE = np.dtype([("lambda_", "<f8"), ("cost_before", "<f8"), ("cost_after", "<f8")] +
                            [(n, "<i4") for n in ("state", "status", "n_obs", "n_stereo", "n_inliers", "n_points_active", "n_frozen_max")] +
                            [("steps", "<i4", (4,)), ("accepted", "<i4", (4,))] + [(n, "<i4") for n in ("pcg_iterations", "n_free", "n_fixed")] +
                            [("reserved", "<i4", (2,))])


def gba_params(chi2_mono: float = 5.991, chi2_stereo: float = 7.815, lambda_: float = 1e-4, lambda_factor: float = 10.0, lambda_min: float = 1e-9,
               step_eps: float = 1e-10, pcg_tol: float = 1e-2, n_rounds: int = 1, iterations=(10, 0, 0, 0), robust_rounds: int = 1,
               min_point_obs: int = 2, check_right: bool = False, pcg_iterations: int = 64, reserved=(0, 0, 0)) -> GbaParams:
    """upstream's GlobalBundleAdjustemnt schedule: one robust round of 10 iterations"""
    its = tuple(iterations) + (0,) * (4 - len(tuple(iterations)))
    return GbaParams(chi2_mono=chi2_mono, chi2_stereo=chi2_stereo, lambda_=lambda_, lambda_factor=lambda_factor, lambda_min=lambda_min,
                     step_eps=step_eps, pcg_tol=pcg_tol, n_rounds=n_rounds, iterations=(C.c_int32 * 4)(*its), robust_rounds=robust_rounds,
                     min_point_obs=min_point_obs, check_right=int(check_right), pcg_iterations=pcg_iterations,
                     reserved=(C.c_int32 * 3)(*reserved))


def _gba_host_arrays(views, start, fixed, points, obs, skip):
    """the arrays of one problem, checked against each other"""
    v = _views_array(views)
    n_kf = len(v)
    st = _start_array(start, n_kf)
    fx = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
    pts = np.ascontiguousarray(points, MAP_POINT_DTYPE).reshape(-1)
    ob = np.ascontiguousarray(obs, GBA_OBS_DTYPE).reshape(-1)
    skip = None if skip is None else np.ascontiguousarray(skip, np.uint8)
    if len(fx) != n_kf or (skip is not None and len(skip) != len(pts)):
        raise ValueError("views, start poses, fixed bytes, map points and skip bytes differ in length")
    return v, st, fx, pts, ob, skip


def global_ba_host(views, start, fixed, scale, points: np.ndarray, obs: np.ndarray, params: GbaParams, skip=None):
    """ss_global_ba_host: the whole rule on the host for one problem -> (poses float64 [n_kf][12], xyz float64 [n_points][3], uint8 point
    flags, uint8 observation flags [n_obs] in the order of obs, one GBA_RESULT_DTYPE record); needs no device.  A refusal raises
    OrbError with the library's message"""
    v, st, fx, pts, ob, skip = _gba_host_arrays(views, start, fixed, points, obs, skip)
    sc = np.ascontiguousarray(scale, np.float32)
    n_kf, n_p, n_o = len(v), len(pts), len(ob)
    poses, xyz = np.empty((n_kf, 12), np.float64), np.empty((n_p, 3), np.float64)
    pf, of, res = np.empty(n_p, np.uint8), np.empty(n_o, np.uint8), np.zeros(1, GBA_RESULT_DTYPE)
    err = C.create_string_buffer(512)
    ptr = lambda a, n: None if a is None or not n else a.ctypes.data  # noqa: E731
    rc = load().ss_global_ba_host(ptr(v, n_kf), ptr(st, n_kf), ptr(fx, n_kf), n_kf, ptr(sc, len(sc)), len(sc), ptr(pts, n_p), ptr(skip, n_p), n_p,
                                  ptr(ob, n_o), n_o, C.byref(params), poses.ctypes.data, ptr(xyz, n_p), ptr(pf, n_p), ptr(of, n_o), res.ctypes.data,
                                  err, len(err))
    if rc != SS_OK:
        raise OrbError(rc, err.value.decode() or "ss_global_ba_host refused its arguments")
    return poses, xyz, pf, of, res[0]


def global_ba_obs_from_idx(kp: np.ndarray, idx: np.ndarray, n_kp=None, right=None) -> np.ndarray:
    """ss_global_ba_obs_from_idx_host: kp [n_kf][rows], idx int32 [n_kf][n_points] (a stack of projection-search outputs), right
    [n_kf][rows] or None -> the GBA_OBS_DTYPE records in ascending (point, kf) order"""
    k = np.ascontiguousarray(kp, KP_DTYPE)
    if k.ndim != 2 or k.shape[1] < 1:
        raise ValueError("keypoints are [n_kf][rows_per_frame]")
    n_kf = len(k)
    ix = np.ascontiguousarray(idx, np.int32).reshape(n_kf, -1)
    nk = np.full(n_kf, k.shape[1], np.int32) if n_kp is None else np.ascontiguousarray(n_kp, np.int32)
    right = None if right is None else np.ascontiguousarray(right, np.float32)
    if len(nk) != n_kf or (right is not None and right.shape != k.shape):
        raise ValueError("keypoints, counts and right coordinates differ in length")
    fn = load().ss_global_ba_obs_from_idx_host
    args = (k.ctypes.data, None if right is None else right.ctypes.data, nk.ctypes.data, n_kf, k.shape[1], ix.ctypes.data, ix.shape[1])
    n = fn(*args, None, 0)
    if n < 0:
        raise OrbError(n, "ss_global_ba_obs_from_idx_host refused its arguments")
    out = np.zeros(n, GBA_OBS_DTYPE)
    if n and fn(*args, out.ctypes.data, n) != n:
        raise OrbError(SS_ERR_STATE, "ss_global_ba_obs_from_idx_host: the count changed between two calls")
    return out


# ---- place recognition (the rule: include/sendslam_orb.h) ----
SS_PLACE_MAX_DB, SS_PLACE_MAX_QUERIES, SS_PLACE_MAX_CANDIDATES, SS_PLACE_MAX_NEIGHBOURS = 262144, 256, 256, 1024


class PlaceParams(C.Structure):
    _fields_ = [("min_score_mode", C.c_int32), ("min_score", C.c_float), ("n_best", C.c_int32), ("scope", C.c_int32),
                ("common_ratio", C.c_float), ("retain_ratio", C.c_float), ("reserved", C.c_int32 * 2)]


# ss_place_cand: one per candidate slot; ss_place_summary: one per query
PLACE_CAND_DTYPE = np.dtype([("kf", "<i4"), ("problem", "<i4"), ("words", "<i4"), ("class", "<i4"), ("score", "<f4"), ("acc", "<f4")])
PLACE_SUMMARY_DTYPE = np.dtype([("n_sharing", "<i4"), ("max_common", "<i4"), ("min_common", "<i4"), ("n_survivors", "<i4"), ("n_seeds", "<i4"),
                                ("min_score", "<f4"), ("best_acc", "<f4"), ("n_candidates", "<i4"), ("n_written", "<i4"), ("status", "<i4"),
                                ("reserved", "<i4", (2,))])


def place_params(min_score_mode: int = 1, min_score: float = 0.0, n_best: int = 0, scope: int = 1, common_ratio: float = 0.8,
                 retain_ratio: float = 0.75, reserved=(0, 0)) -> PlaceParams:
    """upstream's loop detection: the minimum score from the connected keyframes, the 0.75 cut, every map"""
    return PlaceParams(min_score_mode=min_score_mode, min_score=min_score, n_best=n_best, scope=scope, common_ratio=common_ratio,
                       retain_ratio=retain_ratio, reserved=(C.c_int32 * 2)(*reserved))


def _place_arrays(db_word, db_value, db_count, db_skip, problems, q_word, q_value, q_count, q_kf, q_problem, q_nb, q_row, nb):
    """the host arrays of a place call in their C types and the counts they imply"""
    dw = np.ascontiguousarray(db_word, np.int32)
    dv = np.ascontiguousarray(db_value, np.float64)
    dc = np.ascontiguousarray(db_count, np.int32).reshape(-1)
    if dw.ndim != 2 or dv.shape != dw.shape or len(dc) != dw.shape[0]:
        raise ValueError("db_word and db_value are [n_db][stride], db_count [n_db]")
    sk = None if db_skip is None else np.ascontiguousarray(db_skip, np.uint8).reshape(-1)
    if sk is not None and len(sk) != len(dc):
        raise ValueError("one skip byte per database row")
    pr = np.ascontiguousarray(problems, GBA_PROBLEM_DTYPE).reshape(-1)
    qw = np.ascontiguousarray(q_word, np.int32)
    qv = np.ascontiguousarray(q_value, np.float64)
    qc = np.ascontiguousarray(q_count, np.int32).reshape(-1)
    if qw.ndim != 2 or qv.shape != qw.shape or len(qc) != qw.shape[0]:
        raise ValueError("q_word and q_value are [n_q][q_stride], q_count [n_q]")
    n_q = len(qc)
    qk = np.ascontiguousarray(q_kf, np.int32).reshape(-1)
    qp = np.ascontiguousarray(q_problem, np.int32).reshape(-1)
    if len(qk) != n_q or len(qp) != n_q:
        raise ValueError("one q_kf and q_problem per query")
    qn = qr = None
    q_cap = 0
    if q_nb is not None:
        qn = np.ascontiguousarray(q_nb, np.int32)
        qr = np.ascontiguousarray(q_row, COVIS_ROW_DTYPE).reshape(-1)
        if qn.ndim != 3 or qn.shape[0] != n_q or qn.shape[2] != 2 or len(qr) != n_q:
            raise ValueError("q_nb is [n_q][q_cap][2], q_row [n_q]")
        q_cap = qn.shape[1]
    nbr = np.ascontiguousarray(nb, np.int32)
    if nbr.ndim != 3 or nbr.shape[0] != len(dc) or nbr.shape[2] != 2:
        raise ValueError("nb is [n_db][nb_cap][2]")
    return dw, dv, dc, sk, pr, qw, qv, qc, qk, qp, qn, qr, q_cap, nbr


def _place_outputs(n_q, n_db, cand_cap):
    cand = np.zeros((n_q, max(cand_cap, 1)), PLACE_CAND_DTYPE)
    cand.view(np.uint8)[...] = 0x5A
    summary = np.zeros(n_q, PLACE_SUMMARY_DTYPE)
    summary.view(np.uint8)[...] = 0x5A
    return cand, summary, np.full((n_q, n_db), 0x5A5A5A5A, np.int32), np.full((n_q, n_db), np.nan, np.float32)


def place_query_host(db_word, db_value, db_count, n_words: int, problems, q_word, q_value, q_count, q_kf, q_problem, nb, params: PlaceParams,
                     cand_cap: int, db_skip=None, q_nb=None, q_row=None):
    """ss_place_query_host: the whole rule on the host -> (cand PLACE_CAND_DTYPE [n_q][cand_cap], summary PLACE_SUMMARY_DTYPE [n_q], words
    int32 [n_q][n_db], score float32 [n_q][n_db])"""
    dw, dv, dc, sk, pr, qw, qv, qc, qk, qp, qn, qr, q_cap, nbr = _place_arrays(db_word, db_value, db_count, db_skip, problems, q_word, q_value, q_count,
                                                                               q_kf, q_problem, q_nb, q_row, nb)
    n_db, n_q = len(dc), len(qc)
    cand, summary, words, score = _place_outputs(n_q, n_db, cand_cap)
    err = C.create_string_buffer(512)
    ptr = lambda a: None if a is None or not a.size else a.ctypes.data  # noqa: E731
    rc = load().ss_place_query_host(ptr(dw), ptr(dv), ptr(dc), ptr(sk), n_db, dw.shape[1], n_words, ptr(pr), len(pr), ptr(qw), ptr(qv), ptr(qc), qw.shape[1], n_q,
                                    ptr(qk), ptr(qp), ptr(qn), ptr(qr), q_cap, ptr(nbr), nbr.shape[1], C.byref(params), cand_cap, ptr(cand), ptr(summary),
                                    ptr(words), ptr(score), err, len(err))
    if rc != SS_OK:
        raise OrbError(rc, err.value.decode() or "the place recognition host twin refused its arguments")
    return cand, summary, words, score


# ---- covisibility (the rule: include/sendslam_orb.h) ----
SS_COVIS_MAX_ROW_ITEMS, SS_COVIS_MAX_NEIGHBOURS, SS_COVIS_MAX_MAP_KF = 262143, 1024, 1048576


class CovisParams(C.Structure):
    _fields_ = [("min_weight", C.c_int32), ("fallback", C.c_int32), ("cull_obs", C.c_int32), ("cull_slack", C.c_int32),
                ("redundant_th", C.c_float), ("reserved", C.c_int32 * 3)]


# ss_covis_row: one per row
COVIS_ROW_DTYPE = np.dtype([(n, "<i4") for n in ("n_shared", "max_weight", "max_kf", "n_listed", "n_written", "n_mps", "n_redundant", "redundant")])


def covis_params(min_weight: int = 15, fallback: int = 1, cull_obs: int = 3, cull_slack: int = 1, redundant_th: float = 0.9,
                 reserved=(0, 0, 0)) -> CovisParams:
    """upstream's values: UpdateConnections' threshold of 15 (UpdateLocalKeyFrames: min_weight 1), KeyFrameCulling's thObs 3, one octave
    of slack and 0.9 of the points"""
    return CovisParams(min_weight=min_weight, fallback=int(fallback), cull_obs=cull_obs, cull_slack=cull_slack, redundant_th=redundant_th,
                       reserved=(C.c_int32 * 3)(*reserved))


def _covis_map_arrays(problems, obs, cull_skip):
    pr = np.ascontiguousarray(problems, GBA_PROBLEM_DTYPE).reshape(-1)
    ob = np.ascontiguousarray(obs, GBA_OBS_DTYPE).reshape(-1)
    sk = None if cull_skip is None else np.ascontiguousarray(cull_skip, np.uint8).reshape(-1)
    if sk is not None and len(sk) != len(ob):
        raise ValueError("one skip byte per observation record")
    return pr, ob, sk


def _covis_host(frames, problems, n_kf, n_blocks, point_rows, obs, n_levels, table, idx, n_points, n_rows, params, cap, cull_skip, check_right):
    pr, ob, sk = _covis_map_arrays(problems, obs, cull_skip)
    tb = None if table is None else np.ascontiguousarray(table, np.int32).reshape(-1)
    n_rows = len(tb) if tb is not None else n_rows
    nb, row = np.full((max(n_rows, 0), max(cap, 1), 2), 0x5A5A5A5A, np.int32), np.zeros(max(n_rows, 0), COVIS_ROW_DTYPE)
    err = C.create_string_buffer(512)
    ptr = lambda a: None if a is None or not len(a) else a.ctypes.data  # noqa: E731
    map_args = (ptr(pr), len(pr), n_kf, n_blocks, point_rows, ptr(ob), len(ob), ptr(sk), int(check_right), n_levels)
    if frames:
        ix = np.ascontiguousarray(idx, np.int32).reshape(n_rows, -1)
        npts = np.ascontiguousarray(n_points, np.int32).reshape(-1)
        if n_rows and ix.shape[1] != point_rows:
            raise ValueError("idx is [n_frames][point_rows]")
        rc = load().ss_covis_frames_host(*map_args, ptr(ix.reshape(-1)), ptr(npts), ptr(tb), n_rows, C.byref(params), cap, ptr(nb.reshape(-1)), ptr(row), err, len(err))
    else:
        rc = load().ss_covis_kf_host(*map_args, ptr(tb), n_rows, C.byref(params), cap, ptr(nb.reshape(-1)), ptr(row), err, len(err))
    if rc != SS_OK:
        raise OrbError(rc, err.value.decode() or "the covisibility host twin refused its arguments")
    return nb, row


def covis_kf_host(problems, n_kf: int, n_blocks: int, point_rows: int, obs, n_levels: int, params: CovisParams, cap: int, rows=None, cull_skip=None,
                  check_right: bool = False):
    """ss_covis_kf_host: the whole rule on the host -> (nb int32 [n_rows][cap][2], COVIS_ROW_DTYPE [n_rows]); rows None: every keyframe of
    the map.  A refusal raises OrbError with the library's message"""
    return _covis_host(False, problems, n_kf, n_blocks, point_rows, obs, n_levels, rows, None, None, n_kf, params, cap, cull_skip, check_right)


def covis_frames_host(problems, n_kf: int, n_blocks: int, point_rows: int, obs, n_levels: int, idx, n_points, point_src, params: CovisParams, cap: int,
                      cull_skip=None, check_right: bool = False):
    """ss_covis_frames_host: idx int32 [n_frames][point_rows], n_points int32 [n_blocks], point_src [n_frames] -> as covis_kf_host"""
    return _covis_host(True, problems, n_kf, n_blocks, point_rows, obs, n_levels, point_src, idx, n_points, 0, params, cap, cull_skip, check_right)


def covis_edges(nb: np.ndarray, row: np.ndarray, row_kf, min_weight: int) -> np.ndarray:
    """ss_covis_edges_host: the pairs (k, j), j > k, of weight >= min_weight in the downloaded rows -> int32 [n][2]"""
    nb = np.ascontiguousarray(nb, np.int32)
    rw = np.ascontiguousarray(row, COVIS_ROW_DTYPE).reshape(-1)
    rk = np.ascontiguousarray(row_kf, np.int32).reshape(-1)
    if nb.ndim != 3 or nb.shape[0] != len(rw) or len(rk) != len(rw) or nb.shape[2] != 2:
        raise ValueError("nb is [n_rows][cap][2], with one row record and one keyframe number per row")
    fn = load().ss_covis_edges_host
    ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    args = (ptr(nb), ptr(rw), ptr(rk), len(rw), max(nb.shape[1], 1), min_weight)
    n = fn(*args, None, 0)
    if n < 0:
        raise OrbError(n, "ss_covis_edges_host refused its arguments")
    out = np.zeros((n, 2), np.int32)
    if n and fn(*args, out.ctypes.data, n) != n:
        raise OrbError(SS_ERR_STATE, "ss_covis_edges_host: the count changed between two calls")
    return out


def global_ba_rows_from_idx(idx: np.ndarray, n_kp, rows_per_frame: int) -> np.ndarray:
    """ss_global_ba_rows_from_idx_host: the keypoint row of each record of global_ba_obs_from_idx(kp, idx, n_kp), kp being
    [n_kf][rows_per_frame] -> int32, parallel to its table"""
    nk = np.ascontiguousarray(n_kp, np.int32).reshape(-1)
    ix = np.ascontiguousarray(idx, np.int32).reshape(len(nk), -1)
    fn = load().ss_global_ba_rows_from_idx_host
    args = (nk.ctypes.data if len(nk) else None, len(nk), rows_per_frame, ix.ctypes.data if ix.size else None, ix.shape[1])
    n = fn(*args, None, 0)
    if n < 0:
        raise OrbError(n, "ss_global_ba_rows_from_idx_host refused its arguments")
    out = np.zeros(n, np.int32)
    if n and fn(*args, out.ctypes.data, n) != n:
        raise OrbError(SS_ERR_STATE, "ss_global_ba_rows_from_idx_host: the count changed between two calls")
    return out


# ---- map-point refresh (the rule: include/sendslam_orb.h) ----
class RefreshParams(C.Structure):
    _fields_ = [("geometry", C.c_int32), ("descriptor", C.c_int32), ("reserved", C.c_int32 * 6)]


# ss_refresh_info: one per point row; ss_refresh_summary: one per block
REFRESH_INFO_DTYPE = np.dtype([(n, "<i4") for n in ("state", "n_obs", "count", "ref_kf", "level", "best_kf", "best_median", "reserved")])
REFRESH_SUMMARY_DTYPE = np.dtype([(n, "<i4") for n in ("status", "n_rows", "n_selected", "n_refreshed", "n_no_obs", "n_degenerate", "max_obs", "reserved")])


def refresh_params(geometry: int = 1, descriptor: int = 1, reserved=(0, 0, 0, 0, 0, 0)) -> RefreshParams:
    """geometry: UpdateNormalAndDepth; descriptor: ComputeDistinctiveDescriptors; upstream calls the first alone after a bundle adjustment
    or a loop correction, both after a fusion and a creation"""
    return RefreshParams(geometry=int(geometry), descriptor=int(descriptor), reserved=(C.c_int32 * 6)(*reserved))


def _refresh_rows(desc, n_kf, rows_per_frame):
    if rows_per_frame is not None:
        return int(rows_per_frame)
    return 0 if desc is None else desc.reshape(max(n_kf, 1), -1, 32).shape[1]


def refresh_host(problems, n_kf: int, n_blocks: int, point_rows: int, obs, obs_row, scale, points, point_desc, n_points, desc, views,
                 params: RefreshParams, ref_kf=None, select=None, check_right: bool = False, rows_per_frame=None):
    """ss_refresh_host: the whole rule on the host.  points MAP_POINT_DTYPE [n_blocks][point_rows] and point_desc uint8
    [n_blocks][point_rows][32] are copied, refreshed and returned with REFRESH_INFO_DTYPE [n_blocks][point_rows] and REFRESH_SUMMARY_DTYPE
    [n_blocks]; desc uint8 [n_kf][rows_per_frame][32] or None; obs_row int32 [n_obs] or None.  A refusal raises OrbError with the
    library's message"""
    pr, ob, _ = _covis_map_arrays(problems, obs, None)
    rows = None if obs_row is None else np.ascontiguousarray(obs_row, np.int32).reshape(-1)
    if rows is not None and len(rows) != len(ob):
        raise ValueError("one keypoint row per observation record")
    sc = np.ascontiguousarray(scale, np.float32).reshape(-1)
    pts = np.array(points, MAP_POINT_DTYPE).reshape(max(n_blocks, 0), -1)
    pd = None if point_desc is None else np.array(point_desc, np.uint8).reshape(max(n_blocks, 0), -1, 32)
    npts = np.ascontiguousarray(n_points, np.int32).reshape(-1)
    rk = None if ref_kf is None else np.ascontiguousarray(ref_kf, np.int32).reshape(-1)
    sel = None if select is None else np.ascontiguousarray(select, np.uint8).reshape(-1)
    ds = None if desc is None else np.ascontiguousarray(desc, np.uint8)
    v = _views_array(views)
    if len(v) != n_kf or len(npts) != n_blocks:
        raise ValueError("one view per keyframe and one count per block")
    info, summary = np.zeros((max(n_blocks, 0), max(point_rows, 0)), REFRESH_INFO_DTYPE), np.zeros(max(n_blocks, 0), REFRESH_SUMMARY_DTYPE)
    err = C.create_string_buffer(512)
    ptr = lambda a: None if a is None or not a.size else a.ctypes.data  # noqa: E731
    rc = load().ss_refresh_host(ptr(pr), len(pr), n_kf, n_blocks, point_rows, ptr(ob), len(ob), int(check_right), ptr(rows), ptr(sc), len(sc), ptr(pts), ptr(pd),
                                ptr(npts), ptr(rk), ptr(sel), ptr(ds), _refresh_rows(ds, n_kf, rows_per_frame), ptr(v), C.byref(params),
                                ptr(info), ptr(summary), err, len(err))
    if rc != SS_OK:
        raise OrbError(rc, err.value.decode() or "the refresh host twin refused its arguments")
    return pts, pd, info, summary


class DepthParams(C.Structure):
    """ss_depth_params: depth_type 0 float32 samples, 1 uint16 samples"""
    _fields_ = [("bf", C.c_float), ("depth_map_factor", C.c_float), ("close_limit", C.c_float), ("depth_type", C.c_int32)]


DEPTH_SUMMARY_DTYPE = np.dtype([(n, "<i4") for n in ("status", "n_kp", "n_depth", "n_close")])


def depth_params(bf: float, depth_map_factor: float = 1.0, close_limit: float = 0.0, depth_type: int = 0) -> DepthParams:
    return DepthParams(bf=bf, depth_map_factor=depth_map_factor, close_limit=close_limit, depth_type=depth_type)


def depth_params_from_camera(camera: Camera, depth_type: int = 0) -> DepthParams:
    """ss_depth_params_from_camera: bf, depth_map_factor and close_limit (mThDepth) of a calibration; needs no device"""
    p = DepthParams()
    rc = load().ss_depth_params_from_camera(C.byref(camera), int(depth_type), C.byref(p))
    if rc != SS_OK:
        raise OrbError(rc, "ss_depth_params_from_camera refused its arguments")
    return p


def _cameras_array(cams):
    """one Camera or a sequence of them -> (a ctypes array, its length); None -> (None, 0)"""
    if cams is None:
        return None, 0
    if isinstance(cams, Camera):
        cams = [cams]
    return (Camera * len(cams))(*cams), len(cams)


def undistort_bounds_host(camera: Camera) -> np.ndarray:
    """ss_undistort_bounds_host: Frame::ComputeImageBounds -> float32 (min_x, max_x, min_y, max_y); needs no device"""
    out = np.empty(4, np.float32)
    rc = load().ss_undistort_bounds_host(C.byref(camera), out.ctypes.data)
    if rc != SS_OK:
        raise OrbError(rc, "ss_undistort_bounds_host refused its arguments")
    return out


def proj_view_set_bounds(view: ProjView, camera: Camera) -> ProjView:
    """ss_proj_view_set_bounds: overwrites the four bounds of `view` with those of `camera` and returns it; needs no device"""
    rc = load().ss_proj_view_set_bounds(C.byref(view), C.byref(camera))
    if rc != SS_OK:
        raise OrbError(rc, "ss_proj_view_set_bounds refused its arguments")
    return view


def undistort_host(camera: Camera, kp: np.ndarray, in_place: bool = False) -> np.ndarray:
    """ss_undistort_host: mvKeysUn of KP_DTYPE rows on the host (the text the kernel compiles); in_place: out aliases kp, which
    must then be a contiguous KP_DTYPE array.  Needs no device"""
    k = kp if in_place else np.ascontiguousarray(kp, KP_DTYPE).reshape(-1)
    if in_place and (k.dtype != KP_DTYPE or not k.flags.c_contiguous):
        raise ValueError("in_place needs a contiguous KP_DTYPE array")
    out = k if in_place else np.empty(len(k), KP_DTYPE)
    rc = load().ss_undistort_host(C.byref(camera), k.ctypes.data if len(k) else None, len(k), out.ctypes.data if len(k) else None)
    if rc != SS_OK:
        raise OrbError(rc, "ss_undistort_host refused its arguments")
    return out


def depth_host(params: DepthParams, depth: np.ndarray, kp_raw: np.ndarray, kp_un=None, width=None):
    """ss_depth_host: ComputeStereoFromRGBD of one frame on the host.  depth: a 2-D float32 or uint16 array whose rows may be
    longer than `width` samples (a pitch) -> (right float32 [n], depth float32 [n], summary DEPTH_SUMMARY_DTYPE scalar)"""
    if depth.ndim != 2 or depth.strides[1] != depth.itemsize:
        raise ValueError("depth: a 2-D array with contiguous rows")
    raw = np.ascontiguousarray(kp_raw, KP_DTYPE).reshape(-1)
    un = None if kp_un is None else np.ascontiguousarray(kp_un, KP_DTYPE).reshape(-1)
    n = len(raw)
    right, out = np.empty(n, np.float32), np.empty(n, np.float32)
    summary = np.zeros(1, DEPTH_SUMMARY_DTYPE)
    rc = load().ss_depth_host(C.byref(params), depth.ctypes.data, depth.shape[1] if width is None else int(width), depth.shape[0], depth.strides[0],
                              raw.ctypes.data if n else None, un.ctypes.data if un is not None and n else None, n, right.ctypes.data if n else None,
                              out.ctypes.data if n else None, summary.ctypes.data)
    if rc != SS_OK:
        raise OrbError(rc, "ss_depth_host refused its arguments")
    return right, out, summary[0]


# ---- map points from depth (the rule: include/sendslam_orb.h) ----
SS_UNPROJECT_ALL, SS_UNPROJECT_CLOSE = 0, 1
SS_UNPROJECT_CREATED, SS_UNPROJECT_KEPT, SS_UNPROJECT_FAR, SS_UNPROJECT_NO_DEPTH, SS_UNPROJECT_OCTAVE, SS_UNPROJECT_DEGENERATE = range(6)


class UnprojectView(C.Structure):
    """ss_unproject_view: the pose and camera of one frame, in double"""
    _fields_ = [("rcw", C.c_double * 9), ("tcw", C.c_double * 3)] + [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "invfx", "invfy")] + \
               [("ow", C.c_double * 3)]


class UnprojectParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("max_points", C.c_int32), ("close_limit", C.c_float), ("reserved", C.c_int32)]


UNPROJECT_VIEW_DTYPE = np.dtype([("rcw", "<f8", (9,)), ("tcw", "<f8", (3,))] + [(n, "<f8") for n in ("fx", "fy", "cx", "cy", "invfx", "invfy")] +
                                [("ow", "<f8", (3,))])
UNPROJECT_INFO_DTYPE = np.dtype([("state", "<i4")])
UNPROJECT_SUMMARY_DTYPE = np.dtype([(n, "<i4") for n in ("status", "n_kp", "n_depth", "n_close", "n_not_far", "n_processed", "n_created", "n_kept",
                                                         "n_tracked_close", "n_untracked_close")])


def unproject_params(mode: int = SS_UNPROJECT_CLOSE, max_points: int = 100, close_limit: float = 0.0) -> UnprojectParams:
    """upstream's CreateNewKeyFrame / UpdateLastFrame: the close rule with 100 points; close_limit is mThDepth"""
    return UnprojectParams(mode=mode, max_points=max_points, close_limit=close_limit, reserved=0)


def unproject_view(camera: Camera, rcw, tcw) -> UnprojectView:
    """ss_unproject_view_init: the view of `camera` at the pose (rcw, tcw); needs no device"""
    r, t = np.ascontiguousarray(rcw, np.float64).reshape(9), np.ascontiguousarray(tcw, np.float64).reshape(3)
    v = UnprojectView()
    rc = load().ss_unproject_view_init(C.byref(camera), r.ctypes.data, t.ctypes.data, C.byref(v))
    if rc != SS_OK:
        raise OrbError(rc, "ss_unproject_view_init refused its arguments")
    return v


def _unproject_views_array(views):
    """one UnprojectView, a sequence of them or an UNPROJECT_VIEW_DTYPE array -> a contiguous UNPROJECT_VIEW_DTYPE array"""
    if isinstance(views, UnprojectView):
        views = [views]
    if isinstance(views, np.ndarray):
        return np.ascontiguousarray(views, UNPROJECT_VIEW_DTYPE).reshape(-1)
    return np.frombuffer(b"".join(bytes(v) for v in views), UNPROJECT_VIEW_DTYPE).copy()


def _depth_plane(depth, rows):
    """a float32 array of `rows` depths, or an array of records with a float32 field "depth" (STEREO_POINT_DTYPE), read in place ->
    (the array kept alive, the address of row 0's depth, the byte stride)"""
    d = np.asarray(depth)
    if d.dtype.fields:
        d = np.ascontiguousarray(d).reshape(-1)
        if d.dtype.fields["depth"][0] != np.dtype("<f4"):
            raise ValueError("depth: the field must be float32")
        at, stride = d.ctypes.data + d.dtype.fields["depth"][1], d.dtype.itemsize
    else:
        d = np.ascontiguousarray(d, np.float32).reshape(-1)
        at, stride = d.ctypes.data, 4
    if len(d) != rows:
        raise ValueError("one depth per keypoint row")
    return d, at, stride


def _row_flags(flags, rows, name):
    if flags is None:
        return None
    f = np.ascontiguousarray(flags, np.uint8).reshape(-1)
    if len(f) != rows:
        raise ValueError(f"{name}: one byte per keypoint row")
    return f


def _unproject_one(call, what, kp, desc, depth, n, has_point, outlier):
    """the arrays of one frame for ss_unproject_host / ss_unproject -> (info, points, point_desc, point_rows, summary)"""
    k = np.ascontiguousarray(kp, KP_DTYPE).reshape(-1)
    rows = len(k)
    de = np.ascontiguousarray(desc, np.uint8).reshape(rows, 32)
    d, d_at, stride = _depth_plane(depth, rows)
    hp, ol = _row_flags(has_point, rows, "has_point"), _row_flags(outlier, rows, "outlier")
    info = np.empty(rows, UNPROJECT_INFO_DTYPE)
    pts, pd, pr = np.zeros(rows, MAP_POINT_DTYPE), np.zeros((rows, 32), np.uint8), np.zeros((rows, 2), np.int32)
    n_pts, summary = np.zeros(1, np.int32), np.zeros(1, UNPROJECT_SUMMARY_DTYPE)

    def ptr(a):
        return a.ctypes.data if a is not None and a.size else None
    rc = call(rows if n is None else int(n), rows, ptr(k), ptr(de), d_at if rows else None, stride, ptr(hp), ptr(ol), ptr(info), ptr(pts), ptr(pd), ptr(pr),
              n_pts.ctypes.data, summary.ctypes.data)
    if rc != SS_OK:
        raise OrbError(rc, what + " refused its arguments")
    m = int(n_pts[0])
    return info, pts[:m], pd[:m], pr[:m], summary[0]


def unproject_host(view: UnprojectView, params: UnprojectParams, scale, kp, desc, depth, n=None, has_point=None, outlier=None):
    """ss_unproject_host: the whole rule for one frame on the host (the text the kernel compiles).  depth: float32 [rows], or records
    with a "depth" field read in place; n: the told count (None: every row) -> (UNPROJECT_INFO_DTYPE [rows], MAP_POINT_DTYPE
    [n_points], uint8 [n_points][32], int32 [n_points][2], UNPROJECT_SUMMARY_DTYPE scalar); needs no device"""
    sc = np.ascontiguousarray(scale, np.float32)
    lib = load()

    def call(n_, rows, k, de, d_at, stride, hp, ol, info, pts, pd, pr, n_pts, summary):
        return lib.ss_unproject_host(C.byref(view), C.byref(params), sc.ctypes.data, len(sc), k, de, n_, rows, d_at, stride, hp, ol, info, pts, pd, pr,
                                     n_pts, summary)
    return _unproject_one(call, "ss_unproject_host", kp, desc, depth, n, has_point, outlier)


class OrbError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libsendslam_orb: {message} (status {code})")
        self.code = code
        self.message = message


_lib = None


def load():
    """Loads the shared library or raises; never substitutes anything for it."""
    global _lib, LIB_PATH
    if _lib is not None:
        return _lib
    if os.environ.get("SENDSLAM_LIB"):  # A/B builds of the same ABI (profiles/tools/*.sh); never a fallback
        LIB_PATH = os.environ["SENDSLAM_LIB"]
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C send-slam_amd` "
                          f"(or __graft_entry__.build()); there is no CPU fallback")
    # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64.so.7 and a
    # second copy (from /opt/rocm) cannot initialise the device after the first has.  Loading
    # torch first makes the dynamic loader resolve our NEEDED libamdhip64.so.7 to torch's copy,
    # so device pointers, streams and RCCL buffers are shared.  Without torch installed the
    # library simply uses /opt/rocm's runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise ImportError(f"{LIB_PATH} does not export {name}")
    lib.ss_last_error.restype = C.c_char_p
    lib.ss_last_error.argtypes = [C.c_void_p]
    lib.ss_create.argtypes = [C.c_int, C.POINTER(OrbParams), C.POINTER(C.c_void_p)]
    lib.ss_destroy.argtypes = [C.c_void_p]
    lib.ss_set_calibration.argtypes = [C.c_void_p, C.c_int, C.POINTER(Camera)]
    lib.ss_extract.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                               C.c_double, C.POINTER(FrameResult)]
    lib.ss_extract_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int64, C.c_int64]
    lib.ss_get_batch_view.argtypes = [C.c_void_p, C.POINTER(BatchView)]
    lib.ss_fetch_frame.argtypes = [C.c_void_p, C.c_int, C.POINTER(FrameResult)]
    lib.ss_match.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                             C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ss_match_device.argtypes = lib.ss_match.argtypes
    lib.ss_match_batch_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
    lib.ss_match_batch_sources_device.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                  C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ss_track.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                             C.POINTER(Pose)]
    lib.ss_track_reset.argtypes = [C.c_void_p]
    lib.ss_track_detach.argtypes = [C.c_void_p]
    lib.ss_pipe_match_sources.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.ss_synchronize.argtypes = [C.c_void_p]
    lib.ss_get_stream.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.ss_profile_enable.argtypes = [C.c_void_p, C.c_int]
    lib.ss_profile_reset.argtypes = [C.c_void_p]
    lib.ss_stats.argtypes = [C.c_void_p, C.POINTER(StageStats), C.c_int]
    lib.ss_debug_fetch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64]
    lib.ss_debug_sort.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.ss_match_pairs_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ss_expand_descriptors_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.ss_match_expanded_device.argtypes = lib.ss_match.argtypes
    lib.ss_match_partial_expanded_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
    lib.ss_track_features.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Pose)]
    lib.ss_track_features_matched.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                              C.POINTER(Pose)]
    lib.ss_match_partial_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
    lib.ss_match_fold_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ss_wait_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.ss_match_fold_strided_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ss_xchg_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.ss_xchg_destroy.argtypes = [C.c_void_p]
    lib.ss_xchg_last_error.restype = C.c_char_p
    lib.ss_xchg_last_error.argtypes = [C.c_void_p]
    lib.ss_xchg_status.argtypes = [C.c_void_p]
    lib.ss_xchg_allgather.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int,
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    lib.ss_xchg_broadcast.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    lib.ss_stereo_exchange_match.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.ss_stereo_batch_device.argtypes = [C.c_void_p, C.POINTER(StereoParams), C.c_void_p, C.c_void_p]
    lib.ss_extract_stereo.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                      C.POINTER(FrameResult), C.POINTER(FrameResult), C.POINTER(C.c_void_p), C.POINTER(StereoSummary)]
    lib.ss_match_guided_pairs_device.argtypes = [C.c_void_p] + [C.c_void_p] * 7 + [C.c_int, C.c_int, C.POINTER(GuidedParams)] + [C.c_void_p] * 4
    lib.ss_match_guided_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GuidedParams)] + [C.c_void_p] * 4
    lib.ss_match_guided.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                    C.POINTER(GuidedParams), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GuidedSummary)]
    lib.ss_rectify_build_map.argtypes = [C.POINTER(RectifyModel), C.c_void_p, C.c_void_p]
    lib.ss_rectify_set_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.ss_rectify_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                            C.POINTER(C.c_int32), C.c_void_p, C.c_int64, C.c_int64]
    lib.ss_extract_stereo_raw.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                          C.c_int, C.c_int, C.POINTER(StereoParams), C.POINTER(FrameResult), C.POINTER(FrameResult),
                                          C.POINTER(C.c_void_p), C.POINTER(StereoSummary)]
    lib.ss_vocab_load_text.argtypes = [C.c_char_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_int]
    lib.ss_vocab_from_arrays.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                         C.c_char_p, C.c_int]
    lib.ss_vocab_info.argtypes = [C.c_void_p, C.POINTER(VocabShape)]
    lib.ss_vocab_copy_out.argtypes = [C.c_void_p] * 6
    lib.ss_vocab_destroy.argtypes = [C.c_void_p]
    lib.ss_bow_set_vocabulary.argtypes = [C.c_void_p, C.c_void_p]
    lib.ss_bow_transform_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
    lib.ss_bow_transform_batch_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
    lib.ss_match_bow_pairs_device.argtypes = [C.c_void_p] + [C.c_void_p] * 8 + [C.c_int, C.c_int, C.POINTER(GuidedParams)] + [C.c_void_p] * 4
    lib.ss_match_bow_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(GuidedParams)] + [C.c_void_p] * 4
    lib.ss_bow_score_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_int, C.c_void_p]
    lib.ss_proj_view_init.argtypes = [C.POINTER(Camera), C.c_void_p, C.c_void_p, C.c_float, C.POINTER(ProjView)]
    lib.ss_proj_points_host.argtypes = [C.c_void_p, C.POINTER(ProjParams), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.ss_match_proj_pairs_device.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_int] + \
                                              [C.c_void_p, C.c_void_p, C.POINTER(ProjParams)] + [C.c_void_p] * 5
    lib.ss_match_proj_batch_device.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.POINTER(ProjParams)] + \
                                              [C.c_void_p] * 5
    lib.ss_match_proj.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                  C.c_void_p, C.POINTER(ProjParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ProjSummary)]
    lib.ss_epi_pair_init.argtypes = [C.POINTER(Camera), C.c_void_p, C.c_void_p, C.POINTER(Camera), C.c_void_p, C.c_void_p, C.POINTER(EpiPair)]
    lib.ss_epi_check_host.argtypes = [C.c_void_p, C.POINTER(EpiParams), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.ss_triangulate_host.argtypes = [C.c_void_p, C.POINTER(TriParams), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p]
    lib.ss_match_epi_pairs_device.argtypes = [C.c_void_p] + [C.c_void_p] * 10 + [C.c_int, C.c_int, C.c_void_p, C.POINTER(EpiParams)] + [C.c_void_p] * 3
    lib.ss_match_epi_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EpiParams)] + [C.c_void_p] * 3
    lib.ss_triangulate_pairs_device.argtypes = [C.c_void_p] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.POINTER(TriParams)] + [C.c_void_p] * 6
    lib.ss_triangulate_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TriParams)] + [C.c_void_p] * 6
    lib.ss_fuse_view_sim3.argtypes = [C.POINTER(Camera), C.c_void_p, C.c_void_p, C.c_float, C.POINTER(ProjView)]
    lib.ss_fuse_points_host.argtypes = [C.c_void_p, C.POINTER(FuseParams), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.ss_fuse_check_host.argtypes = [C.POINTER(FuseParams), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p]
    lib.ss_match_fuse_pairs_device.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_int] + \
                                              [C.c_void_p, C.c_void_p, C.POINTER(FuseParams)] + [C.c_void_p] * 5
    lib.ss_match_fuse_batch_device.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.POINTER(FuseParams)] + \
                                              [C.c_void_p] * 5
    lib.ss_match_fuse.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + \
                                 [C.POINTER(FuseParams)] + [C.c_void_p] * 4 + [C.POINTER(FuseSummary)]
    lib.ss_sim3_model_host.argtypes = [C.POINTER(Sim3Params), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ss_sim3_check_host.argtypes = [C.POINTER(Sim3Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + \
                                      [C.c_void_p] * 3
    lib.ss_sim3_to_view.argtypes = [C.POINTER(Camera), C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(ProjView)]
    lib.ss_sim3_pairs_device.argtypes = [C.c_void_p] + [C.c_void_p] * 9 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Sim3Params)] + \
                                        [C.c_void_p] * 2
    lib.ss_sim3_batch_device.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.POINTER(Sim3Params)] + [C.c_void_p] * 2
    lib.ss_sim3.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.POINTER(Sim3Params), C.c_void_p,
                                                                                            C.c_void_p]
    lib.ss_local_ba_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(BaParams)] + [C.c_void_p] * 5
    lib.ss_local_ba_pairs_device.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + \
                                            [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(BaParams)] + [C.c_void_p] * 5
    lib.ss_local_ba_batch_device.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + \
                                            [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(BaParams)] + [C.c_void_p] * 5
    lib.ss_local_ba.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_int, C.c_void_p, C.POINTER(BaParams)] + [C.c_void_p] * 5
    lib.ss_local_ba_points_to_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.ss_pose_graph_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(GraphParams)] + [C.c_void_p] * 3
    lib.ss_pose_graph_edge_host.argtypes = [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p] * 2
    lib.ss_graph_atan2_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.ss_graph_ln_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.ss_pose_graph_device.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(GraphParams)] + \
                                        [C.c_void_p] * 3
    lib.ss_pose_graph.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(GraphParams)] + [C.c_void_p] * 3
    lib.ss_pose_graph_points_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.ss_global_ba_host.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                         C.POINTER(GbaParams)] + [C.c_void_p] * 5 + [C.c_char_p, C.c_int]
    lib.ss_global_ba_obs_from_idx_host.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.ss_global_ba_device.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                                          C.c_void_p, C.c_int, C.c_void_p, C.POINTER(GbaParams)] + [C.c_void_p] * 5
    lib.ss_global_ba.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                                   C.POINTER(GbaParams)] + [C.c_void_p] * 5
    covis_map = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.ss_covis_params_default.argtypes = [C.POINTER(CovisParams)]
    lib.ss_covis_set_map.argtypes = [C.c_void_p] + covis_map
    lib.ss_covis_kf_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(CovisParams), C.c_int, C.c_void_p, C.c_void_p]
    lib.ss_covis_frames_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(CovisParams), C.c_int, C.c_void_p, C.c_void_p]
    lib.ss_covis.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(CovisParams), C.c_int, C.c_void_p, C.c_void_p]
    lib.ss_covis_kf_host.argtypes = covis_map + [C.c_int, C.c_void_p, C.c_int, C.POINTER(CovisParams), C.c_int, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    lib.ss_covis_frames_host.argtypes = covis_map + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(CovisParams), C.c_int, C.c_void_p,
                                                     C.c_void_p, C.c_char_p, C.c_int]
    lib.ss_covis_edges_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.ss_covis_set_map_rows.argtypes = [C.c_void_p] + covis_map + [C.c_void_p]
    lib.ss_global_ba_rows_from_idx_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.ss_refresh_params_default.argtypes = [C.POINTER(RefreshParams)]
    lib.ss_refresh_device.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.POINTER(RefreshParams), C.c_void_p, C.c_void_p]
    lib.ss_refresh.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                               C.c_void_p, C.c_int, C.POINTER(RefreshParams), C.c_void_p, C.c_void_p]
    lib.ss_refresh_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + \
                                   [C.c_int, C.c_void_p, C.POINTER(RefreshParams), C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    lib.ss_place_params_default.argtypes = [C.POINTER(PlaceParams)]
    lib.ss_place_set_database.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    place_query = [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_int, C.POINTER(PlaceParams), C.c_int] + [C.c_void_p] * 4
    place_db = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.ss_place_query_device.argtypes = [C.c_void_p] + place_query
    lib.ss_place.argtypes = [C.c_void_p] + place_db + place_query
    lib.ss_place_query_host.argtypes = place_db + place_query + [C.c_char_p, C.c_int]
    lib.ss_pnp_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                C.POINTER(PnpParams), C.c_int, C.c_void_p, C.c_void_p]
    lib.ss_pnp_model_host.argtypes = [C.POINTER(PnpParams)] + [C.c_void_p] * 6
    lib.ss_pnp_check_host.argtypes = [C.POINTER(PnpParams), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3
    lib.ss_pnp_pairs_device.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                                         C.c_int] + [C.c_void_p] * 3 + [C.POINTER(PnpParams)] + [C.c_void_p] * 2
    lib.ss_pnp_batch_device.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + \
                                       [C.POINTER(PnpParams)] + [C.c_void_p] * 2
    lib.ss_pnp.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(PnpParams), C.c_void_p, C.c_void_p]
    lib.ss_two_view_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                     C.POINTER(TwoViewParams), C.c_int] + [C.c_void_p] * 5
    lib.ss_two_view_model_host.argtypes = [C.c_void_p] * 5
    lib.ss_two_view_check_host.argtypes = [C.POINTER(TwoViewParams), C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 14
    lib.ss_two_view_accept_host.argtypes = [C.POINTER(TwoViewParams), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]
    lib.ss_two_view_point_tests_host.argtypes = [C.c_double, C.c_double, C.c_void_p]
    lib.ss_two_view_beats_host.argtypes = [C.c_double, C.c_int, C.c_double, C.c_int]
    lib.ss_two_view_pairs_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                             C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TwoViewParams)] + [C.c_void_p] * 5
    lib.ss_two_view_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(TwoViewParams)] + [C.c_void_p] * 5
    lib.ss_two_view.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(TwoViewParams)] + \
        [C.c_void_p] * 5
    lib.ss_pose_opt_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p, C.POINTER(PoseOptParams), C.c_void_p, C.c_void_p]
    lib.ss_pose_opt_pairs_device.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + \
                                            [C.c_void_p] * 4 + [C.POINTER(PoseOptParams)] + [C.c_void_p] * 2
    lib.ss_pose_opt_batch_device.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.POINTER(PoseOptParams)] + \
                                            [C.c_void_p] * 2
    lib.ss_pose_opt.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(PoseOptParams),
                                                                  C.c_void_p, C.c_void_p]
    lib.ss_sim3_opt_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3 + \
                                    [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Sim3OptParams), C.c_void_p, C.c_void_p]
    lib.ss_sim3_opt_pairs_device.argtypes = [C.c_void_p] + [C.c_void_p] * 9 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                                               C.POINTER(Sim3OptParams)] + [C.c_void_p] * 2
    lib.ss_sim3_opt_batch_device.argtypes = [C.c_void_p] + [C.c_void_p] * 6 + [C.POINTER(Sim3OptParams)] + [C.c_void_p] * 2
    lib.ss_sim3_opt.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p,
                                                                                                 C.POINTER(Sim3OptParams), C.c_void_p, C.c_void_p]
    lib.ss_sim3_marks_pairs_device.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int, C.c_int] + [C.c_void_p] * 2
    lib.ss_sim3_mutual_pairs_device.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int, C.c_int] + [C.c_void_p] * 2
    lib.ss_sim3_marks_batch_device.argtypes = [C.c_void_p] + [C.c_void_p] * 5
    lib.ss_sim3_mutual_batch_device.argtypes = [C.c_void_p] + [C.c_void_p] * 6
    lib.ss_sim3_to_view21.argtypes = [C.POINTER(Camera), C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(ProjView)]
    lib.ss_undistort_bounds_host.argtypes = [C.POINTER(Camera), C.c_void_p]
    lib.ss_proj_view_set_bounds.argtypes = [C.POINTER(ProjView), C.POINTER(Camera)]
    lib.ss_undistort_host.argtypes = [C.POINTER(Camera), C.c_void_p, C.c_int, C.c_void_p]
    lib.ss_undistort_pairs_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.ss_undistort_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.ss_get_batch_raw_xy.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.ss_depth_params_from_camera.argtypes = [C.POINTER(Camera), C.c_int, C.POINTER(DepthParams)]
    lib.ss_depth_host.argtypes = [C.POINTER(DepthParams), C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p]
    lib.ss_depth_pairs_device.argtypes = [C.c_void_p, C.POINTER(DepthParams), C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ss_depth_batch_device.argtypes = [C.c_void_p, C.POINTER(DepthParams), C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
    lib.ss_triangulate_stereo_host.argtypes = [C.c_void_p, C.POINTER(TriStereoRig), C.POINTER(TriStereoParams), C.c_void_p, C.c_int] + [C.c_void_p] * 6 + \
                                               [C.c_int, C.c_void_p, C.c_void_p]
    lib.ss_triangulate_stereo_pairs_device.argtypes = [C.c_void_p] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p] + \
                                                       [C.c_void_p, C.c_int64] * 4 + [C.POINTER(TriStereoParams)] + [C.c_void_p] * 6
    lib.ss_triangulate_stereo_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_void_p, C.c_int64] * 2 + \
                                                       [C.POINTER(TriStereoParams)] + [C.c_void_p] * 6
    lib.ss_unproject_view_init.argtypes = [C.POINTER(Camera), C.c_void_p, C.c_void_p, C.POINTER(UnprojectView)]
    lib.ss_unproject_host.argtypes = [C.POINTER(UnprojectView), C.POINTER(UnprojectParams), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_void_p, C.c_int64] + [C.c_void_p] * 8
    lib.ss_unproject_pairs_device.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                                                 C.POINTER(UnprojectParams)] + [C.c_void_p] * 6
    lib.ss_unproject_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(UnprojectParams)] + \
                                             [C.c_void_p] * 6
    lib.ss_unproject.argtypes = [C.c_void_p, C.POINTER(UnprojectView), C.POINTER(UnprojectParams), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_int64] + [C.c_void_p] * 8
    lib.ss_pipe_create.argtypes = [C.c_int, C.POINTER(OrbParams), C.POINTER(Camera), C.POINTER(PipeConfig),
                                   C.POINTER(C.c_void_p)]
    lib.ss_pipe_destroy.argtypes = [C.c_void_p]
    lib.ss_pipe_last_error.restype = C.c_char_p
    lib.ss_pipe_last_error.argtypes = [C.c_void_p]
    lib.ss_pipe_acquire.argtypes = [C.c_void_p, C.POINTER(PipeSlot)]
    lib.ss_pipe_submit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.ss_pipe_submit_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
    lib.ss_pipe_wait.argtypes = [C.c_void_p, C.POINTER(PipeResult)]
    lib.ss_pipe_poll.argtypes = [C.c_void_p, C.POINTER(PipeResult)]
    lib.ss_pipe_release.argtypes = [C.c_void_p, C.c_int]
    lib.ss_pipe_in_flight.argtypes = [C.c_void_p]
    lib.ss_pipe_debug_inject_failure.argtypes = [C.c_void_p, C.c_int]
    if lib.ss_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI {lib.ss_abi_version()} != {ABI_VERSION}")
    _lib = lib
    return lib


def rectify_build_map(model: RectifyModel):
    """ss_rectify_build_map: the float maps of a model -> (map_x, map_y) float32 [height][width].  Host code: needs no context and
    no device."""
    map_x = np.empty((model.height, model.width), np.float32)
    map_y = np.empty((model.height, model.width), np.float32)
    rc = load().ss_rectify_build_map(C.byref(model), map_x.ctypes.data, map_y.ctypes.data)
    if rc != SS_OK:
        raise OrbError(rc, "ss_rectify_build_map: bad size or a singular K' * R")
    return map_x, map_y


class Vocabulary:
    """ss_vocab: a DBoW2 vocabulary tree on the host (no device needed).  Node ids are the text file's (0 = the root), word ids
    count the leaves in file order."""

    def __init__(self, handle):
        self._lib = load()
        self._h = handle

    @staticmethod
    def _made(rc: int, h, err) -> "Vocabulary":
        if rc != SS_OK:
            raise OrbError(rc, err.value.decode(errors="replace"))
        return Vocabulary(h)

    @classmethod
    def load_text(cls, path: str) -> "Vocabulary":
        h, err = C.c_void_p(), C.create_string_buffer(256)
        return cls._made(load().ss_vocab_load_text(os.fsencode(path), C.byref(h), err, len(err)), h, err)

    @classmethod
    def from_arrays(cls, parent, is_leaf, desc, weight, k: int, L: int) -> "Vocabulary":
        parent = np.ascontiguousarray(parent, np.int32)
        is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        weight = np.ascontiguousarray(weight, np.float64)
        assert len(parent) == len(is_leaf) == len(desc) == len(weight)
        h, err = C.c_void_p(), C.create_string_buffer(256)
        return cls._made(load().ss_vocab_from_arrays(len(parent), parent.ctypes.data, is_leaf.ctypes.data, desc.ctypes.data, weight.ctypes.data,
                                                     int(k), int(L), C.byref(h), err, len(err)), h, err)

    def info(self) -> dict:
        s = VocabShape()
        rc = self._lib.ss_vocab_info(self._h, C.byref(s))
        if rc != SS_OK:
            raise OrbError(rc, "ss_vocab_info")
        return {n: int(getattr(s, n)) for n, _ in VocabShape._fields_}

    def copy_out(self) -> dict:
        """per node id (0 = the root): first_child (-1: a leaf), n_children, word (-1: an inner node), weight, depth"""
        n = self.info()["n_nodes"] + 1
        out = {"first_child": np.empty(n, np.int32), "n_children": np.empty(n, np.int32), "word": np.empty(n, np.int32),
               "weight": np.empty(n, np.float64), "depth": np.empty(n, np.int32)}
        rc = self._lib.ss_vocab_copy_out(self._h, *(out[k].ctypes.data for k in ("first_child", "n_children", "word", "weight", "depth")))
        if rc != SS_OK:
            raise OrbError(rc, "ss_vocab_copy_out")
        return out

    def close(self):
        if self._h:
            self._lib.ss_vocab_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_params(**kw) -> OrbParams:
    p = OrbParams()
    load().ss_orb_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class OrbContext:
    """One extraction context = one HIP stream on one device (ss_create / ss_destroy)."""

    def __init__(self, device: int = 0, **params):
        self._lib = load()
        self.params = default_params(**params)
        h = C.c_void_p()
        rc = self._lib.ss_create(int(device), C.byref(self.params), C.byref(h))
        if rc != SS_OK:
            raise OrbError(rc, (self._lib.ss_last_error(None) or b"").decode())
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ss_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int):
        if rc < 0:
            raise OrbError(rc, (self._lib.ss_last_error(self._h) or b"").decode())
        return rc

    def last_error(self) -> str:
        return (self._lib.ss_last_error(self._h) or b"").decode()

    # ---- calibration (the "calibration" message of the wire protocol) ----
    def set_calibration(self, camera_id: int, cam: Camera):
        self._check(self._lib.ss_set_calibration(self._h, int(camera_id), C.byref(cam)))

    # ---- host in / host out ----
    def extract(self, img: np.ndarray, camera_id: int = 1, timestamp: float = 0.0):
        """img: (H, W) or (H, W, C) uint8.  -> (keypoints KP_DTYPE[n], desc u8[n,32], level_counts)"""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w = img.shape[:2]
        ch = 1 if img.ndim == 2 else img.shape[2]
        res = FrameResult()
        self._check(self._lib.ss_extract(self._h, int(camera_id), img.ctypes.data, w, h, ch, w * ch,
                                         float(timestamp), C.byref(res)))
        n = res.n_keypoints
        kps = np.empty(n, KP_DTYPE)
        desc = np.empty((n, 32), np.uint8)
        if n:
            C.memmove(kps.ctypes.data, res.keypoints, n * KP_DTYPE.itemsize)
            C.memmove(desc.ctypes.data, res.descriptors, n * 32)
        return kps, desc, np.array(list(res.level_counts)[:self.params.n_levels])

    def match(self, q: np.ndarray, t: np.ndarray, th: int = 50, ratio_num: int = 9, ratio_den: int = 10,
              exclude_self: bool = False):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        nq, nt = len(q), len(t)
        idx = np.empty(nq, np.int32)
        d1 = np.empty(nq, np.uint16)
        d2 = np.empty(nq, np.uint16)
        self._check(self._lib.ss_match(self._h, q.ctypes.data, nq, t.ctypes.data if nt else None, nt, int(th),
                                       int(ratio_num), int(ratio_den), int(exclude_self), idx.ctypes.data,
                                       d1.ctypes.data, d2.ctypes.data))
        return idx, d1, d2

    # ---- pose (bounded monocular front-end; needs set_calibration) ----
    def track(self, img: np.ndarray, camera_id: int = 1, timestamp: float = 0.0) -> dict:
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w = img.shape[:2]
        ch = 1 if img.ndim == 2 else img.shape[2]
        po = Pose()
        self._check(self._lib.ss_track(self._h, int(camera_id), img.ctypes.data, w, h, ch, w * ch, float(timestamp),
                                       C.byref(po)))
        return {"state": po.tracking_state, "camera_id": po.camera_id, "timestamp": po.timestamp,
                "position": np.array(list(po.position)), "quaternion": np.array(list(po.quaternion)),
                "n_keypoints": po.n_keypoints, "n_matches": po.n_matches, "n_inliers": po.n_inliers,
                "n_map_points": po.n_map_points}

    def track_features(self, d_desc: int, kps: np.ndarray, camera_id: int = 1, timestamp: float = 0.0) -> dict:
        """Pose step alone: descriptors already on the device (n x 32 B at d_desc), keypoints KP_DTYPE[n] on the host."""
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        po = Pose()
        self._check(self._lib.ss_track_features(self._h, int(camera_id), float(timestamp), C.c_void_p(d_desc),
                                                kps.ctypes.data, len(kps), C.byref(po)))
        return {"state": po.tracking_state, "camera_id": po.camera_id, "timestamp": po.timestamp,
                "position": np.array(list(po.position)), "quaternion": np.array(list(po.quaternion)),
                "n_keypoints": po.n_keypoints, "n_matches": po.n_matches, "n_inliers": po.n_inliers,
                "n_map_points": po.n_map_points}

    def track_features_matched(self, d_desc: int, kps: np.ndarray, match_idx=None, match_d1=None, desc_stays_valid: bool = False,
                               camera_id: int = 1, timestamp: float = 0.0) -> dict:
        """track_features with this frame's matches against the previous call's frame handed in (int32[n], uint16[n] or None)."""
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        mi = None if match_idx is None else np.ascontiguousarray(match_idx, np.int32)
        md = None if match_d1 is None else np.ascontiguousarray(match_d1, np.uint16)
        if mi is not None and (len(mi) < len(kps) or md is None or len(md) < len(kps)):
            raise ValueError("match arrays shorter than the keypoints")
        po = Pose()
        self._check(self._lib.ss_track_features_matched(self._h, int(camera_id), float(timestamp), C.c_void_p(d_desc), kps.ctypes.data, len(kps),
                                                        None if mi is None else mi.ctypes.data, None if md is None else md.ctypes.data,
                                                        SS_TRACK_DESC_STAYS_VALID if desc_stays_valid else 0, C.byref(po)))
        return {"state": po.tracking_state, "camera_id": po.camera_id, "timestamp": po.timestamp,
                "position": np.array(list(po.position)), "quaternion": np.array(list(po.quaternion)),
                "n_keypoints": po.n_keypoints, "n_matches": po.n_matches, "n_inliers": po.n_inliers,
                "n_map_points": po.n_map_points}

    def track_reset(self):
        self._check(self._lib.ss_track_reset(self._h))

    def track_detach(self):
        """Copy the descriptor rows any camera's tracker still refers to (desc_stays_valid) into the context."""
        self._check(self._lib.ss_track_detach(self._h))

    # ---- device in / device out (pointers are raw device addresses, e.g. tensor.data_ptr()) ----
    def extract_batch_device(self, d_ptr: int, n_frames: int, width: int, height: int, channels: int = 1,
                             row_stride: Optional[int] = None, frame_stride: Optional[int] = None):
        row_stride = width * channels if row_stride is None else row_stride
        frame_stride = row_stride * height if frame_stride is None else frame_stride
        self._check(self._lib.ss_extract_batch_device(self._h, C.c_void_p(d_ptr), n_frames, width, height,
                                                      channels, row_stride, frame_stride))

    def batch_view(self) -> BatchView:
        v = BatchView()
        self._check(self._lib.ss_get_batch_view(self._h, C.byref(v)))
        return v

    def fetch_frame(self, frame: int):
        """Host copy of one frame of the last batch -> (keypoints, desc, level_counts)."""
        res = FrameResult()
        self._check(self._lib.ss_fetch_frame(self._h, int(frame), C.byref(res)))
        n = res.n_keypoints
        kps = np.empty(n, KP_DTYPE)
        desc = np.empty((n, 32), np.uint8)
        if n:
            C.memmove(kps.ctypes.data, res.keypoints, n * KP_DTYPE.itemsize)
            C.memmove(desc.ctypes.data, res.descriptors, n * 32)
        return kps, desc, np.array(list(res.level_counts)[:self.params.n_levels])

    def match_device(self, d_q: int, nq: int, d_t: int, nt: int, d_idx: int, d_d1: int, d_d2: int, th: int = 50,
                     ratio_num: int = 9, ratio_den: int = 10, exclude_self: bool = False):
        self._check(self._lib.ss_match_device(self._h, C.c_void_p(d_q), nq, C.c_void_p(d_t), nt, th, ratio_num,
                                              ratio_den, int(exclude_self), C.c_void_p(d_idx), C.c_void_p(d_d1),
                                              C.c_void_p(d_d2)))

    def match_batch_device(self, mode: int, d_idx: int, d_d1: int, d_d2: int, th: int = 50, ratio_num: int = 9,
                           ratio_den: int = 10):
        self._check(self._lib.ss_match_batch_device(self._h, mode, th, ratio_num, ratio_den, C.c_void_p(d_idx),
                                                    C.c_void_p(d_d1), C.c_void_p(d_d2)))

    def match_batch_sources_device(self, train_src, d_idx: int, d_d1: int, d_d2: int, d_carry: int = 0, d_carry_n: int = 0,
                                   n_carry: int = 0, th: int = 50, ratio_num: int = 9, ratio_den: int = 10):
        """Every frame of the last batch against the train frame train_src[b] names (host ints, one per frame): >= 0 a frame
        of the batch, -1 none, <= -2 carry frame -2 - t of d_carry ([n_carry][kp_capacity][32] packed, device) with
        d_carry_n (device int32 [n_carry]) rows.  Outputs as match_batch_device."""
        src = np.ascontiguousarray(train_src, dtype=np.int32)
        self._check(self._lib.ss_match_batch_sources_device(self._h, src.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(d_carry),
                                                            C.c_void_p(d_carry_n), int(n_carry), th, ratio_num, ratio_den,
                                                            C.c_void_p(d_idx), C.c_void_p(d_d1), C.c_void_p(d_d2)))

    def match_pairs_device(self, d_q: int, d_nq: int, d_t: int, d_nt: int, n_frames: int, rows_per_frame: int, d_idx: int,
                           d_d1: int, d_d2: int, th: int = 50, ratio_num: int = 9, ratio_den: int = 10):
        """n_frames independent (query frame, train frame) pairs: [n_frames][rows_per_frame][32] both sides."""
        self._check(self._lib.ss_match_pairs_device(self._h, C.c_void_p(d_q), C.c_void_p(d_nq), C.c_void_p(d_t), C.c_void_p(d_nt),
                                                    n_frames, rows_per_frame, th, ratio_num, ratio_den, C.c_void_p(d_idx),
                                                    C.c_void_p(d_d1), C.c_void_p(d_d2)))

    @staticmethod
    def expanded_bytes(n: int) -> int:
        """bytes of n descriptors in the matrix-core matcher's operand format (128 B per row, rows rounded up to 32)"""
        return ((n + 31) & ~31) * EXPANDED_ROW_BYTES

    def expand_descriptors_device(self, d_packed: int, n: int, d_expanded: int):
        self._check(self._lib.ss_expand_descriptors_device(self._h, C.c_void_p(d_packed), n, C.c_void_p(d_expanded)))

    def match_expanded_device(self, d_qx: int, nq: int, d_tx: int, nt: int, d_idx: int, d_d1: int, d_d2: int, th: int = 50,
                              ratio_num: int = 9, ratio_den: int = 10, exclude_self: bool = False):
        self._check(self._lib.ss_match_expanded_device(self._h, C.c_void_p(d_qx), nq, C.c_void_p(d_tx), nt, th, ratio_num,
                                                       ratio_den, int(exclude_self), C.c_void_p(d_idx), C.c_void_p(d_d1),
                                                       C.c_void_p(d_d2)))

    def match_partial_expanded_device(self, d_qx: int, nq: int, d_tx: int, nt: int, row_offset: int, d_part: int):
        self._check(self._lib.ss_match_partial_expanded_device(self._h, C.c_void_p(d_qx), nq, C.c_void_p(d_tx), nt,
                                                               int(row_offset), C.c_void_p(d_part)))

    def match_partial_device(self, d_q: int, nq: int, d_t: int, nt: int, row_offset: int, d_part: int):
        """Raw local match of a database shard -> nq 8-byte ss_match_part records (global rows) at d_part."""
        self._check(self._lib.ss_match_partial_device(self._h, C.c_void_p(d_q), nq, C.c_void_p(d_t), nt, int(row_offset),
                                                      C.c_void_p(d_part)))

    def match_fold_device(self, d_parts: int, n_parts: int, nq: int, d_idx: int, d_d1: int, d_d2: int, th: int = 50,
                          ratio_num: int = 9, ratio_den: int = 10):
        self._check(self._lib.ss_match_fold_device(self._h, C.c_void_p(d_parts), n_parts, nq, th, ratio_num, ratio_den,
                                                   C.c_void_p(d_idx), C.c_void_p(d_d1), C.c_void_p(d_d2)))

    def match_fold_strided_device(self, d_parts: int, n_parts: int, part_stride_bytes: int, nq: int, d_idx: int, d_d1: int,
                                  d_d2: int, th: int = 50, ratio_num: int = 9, ratio_den: int = 10):
        """the fold on parts part_stride_bytes apart: the layout Exchange.allgather leaves"""
        self._check(self._lib.ss_match_fold_strided_device(self._h, C.c_void_p(d_parts), n_parts, part_stride_bytes, nq, th, ratio_num,
                                                           ratio_den, C.c_void_p(d_idx), C.c_void_p(d_d1), C.c_void_p(d_d2)))

    # ---- stereo depth of rectified pairs (frames 2p = left, 2p + 1 = right) ----
    def stereo_batch_device(self, d_points: int, d_summary: int, fx: float, baseline: float, th_depth: float = 35.0):
        """ss_stereo_batch_device on the last batch: d_points [n_frames / 2][kp_capacity] STEREO_POINT_DTYPE rows and
        d_summary [n_frames / 2] STEREO_SUMMARY_DTYPE rows, both device memory; asynchronous."""
        sp = StereoParams(fx=fx, baseline=baseline, th_depth=th_depth)
        self._check(self._lib.ss_stereo_batch_device(self._h, C.byref(sp), C.c_void_p(d_points), C.c_void_p(d_summary)))

    def extract_stereo(self, left: np.ndarray, right: np.ndarray, camera_id: int = 1, timestamp: float = 0.0):
        """One rectified pair (same shape, (H, W) or (H, W, C) uint8) -> (kpsL, descL, kpsR, descR, points, summary):
        points is STEREO_POINT_DTYPE[len(kpsL)], summary a dict of the ss_stereo_summary fields.  Needs the calibration
        of camera_id (fx, baseline, th_depth) and a context created with max_batch >= 2."""
        left = np.ascontiguousarray(left, dtype=np.uint8)
        right = np.ascontiguousarray(right, dtype=np.uint8)
        if left.shape != right.shape:
            raise ValueError(f"the two eyes differ in shape: {left.shape} and {right.shape}")
        h, w = left.shape[:2]
        ch = 1 if left.ndim == 2 else left.shape[2]
        rl, rr, pts, summ = FrameResult(), FrameResult(), C.c_void_p(), StereoSummary()
        self._check(self._lib.ss_extract_stereo(self._h, int(camera_id), left.ctypes.data, right.ctypes.data, w, h, ch, w * ch,
                                                float(timestamp), C.byref(rl), C.byref(rr), C.byref(pts), C.byref(summ)))
        return self._pair_results(rl, rr, pts, summ)

    def _pair_results(self, rl, rr, pts, summ):
        out = []
        for res in (rl, rr):
            n = res.n_keypoints
            kps = np.empty(n, KP_DTYPE)
            desc = np.empty((n, 32), np.uint8)
            if n:
                C.memmove(kps.ctypes.data, res.keypoints, n * KP_DTYPE.itemsize)
                C.memmove(desc.ctypes.data, res.descriptors, n * 32)
            out += [kps, desc]
        points = np.empty(rl.n_keypoints, STEREO_POINT_DTYPE)
        if rl.n_keypoints:
            C.memmove(points.ctypes.data, pts.value, rl.n_keypoints * STEREO_POINT_DTYPE.itemsize)
        return out[0], out[1], out[2], out[3], points, {n: getattr(summ, n) for n, _ in StereoSummary._fields_}

    # ---- rectification of raw frames (the rule: include/sendslam_orb.h) ----
    def set_rectify_map(self, map_id: int, map_x: Optional[np.ndarray], map_y: Optional[np.ndarray]):
        """ss_rectify_set_map: any float32 map pair [height][width] becomes map map_id; None, None drops it.  Synchronises."""
        if map_x is None and map_y is None:
            self._check(self._lib.ss_rectify_set_map(self._h, int(map_id), None, None, 0, 0))
            return
        map_x, map_y = np.ascontiguousarray(map_x, np.float32), np.ascontiguousarray(map_y, np.float32)
        if map_x.ndim != 2 or map_x.shape != map_y.shape:
            raise ValueError(f"the two maps must be [height][width] arrays of one shape: {map_x.shape} and {map_y.shape}")
        h, w = map_x.shape
        self._check(self._lib.ss_rectify_set_map(self._h, int(map_id), map_x.ctypes.data, map_y.ctypes.data, w, h))

    def set_rectify_model(self, map_id: int, model: RectifyModel):
        """builds the maps of a model on the host and sets them as map map_id"""
        self.set_rectify_map(map_id, *rectify_build_map(model))

    def rectify_batch_device(self, d_src: int, n_frames: int, width: int, height: int, map_ids, d_dst: int, channels: int = 1,
                             row_stride: Optional[int] = None, frame_stride: Optional[int] = None,
                             dst_row_stride: Optional[int] = None, dst_frame_stride: Optional[int] = None):
        """ss_rectify_batch_device: frame b of d_src remapped with map map_ids[b] (host ints) into d_dst; asynchronous."""
        row_stride = width * channels if row_stride is None else row_stride
        frame_stride = row_stride * height if frame_stride is None else frame_stride
        dst_row_stride = width * channels if dst_row_stride is None else dst_row_stride
        dst_frame_stride = dst_row_stride * height if dst_frame_stride is None else dst_frame_stride
        ids = np.ascontiguousarray(map_ids, dtype=np.int32)
        if len(ids) != n_frames:
            raise ValueError(f"{len(ids)} map ids for {n_frames} frames")
        self._check(self._lib.ss_rectify_batch_device(self._h, C.c_void_p(d_src), n_frames, width, height, channels, row_stride,
                                                      frame_stride, ids.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(d_dst),
                                                      dst_row_stride, dst_frame_stride))

    def extract_stereo_raw(self, left: np.ndarray, right: np.ndarray, map_left: int, map_right: int, fx: float, baseline: float,
                           th_depth: float = 35.0, camera_id: int = 1, timestamp: float = 0.0):
        """extract_stereo on a RAW pair: both eyes are remapped on the device with maps map_left / map_right first.  fx, baseline
        and th_depth are those of the RECTIFIED pair (fx_new, the baseline of P2).  Returns what extract_stereo returns."""
        left = np.ascontiguousarray(left, dtype=np.uint8)
        right = np.ascontiguousarray(right, dtype=np.uint8)
        if left.shape != right.shape:
            raise ValueError(f"the two eyes differ in shape: {left.shape} and {right.shape}")
        h, w = left.shape[:2]
        ch = 1 if left.ndim == 2 else left.shape[2]
        sp = StereoParams(fx=fx, baseline=baseline, th_depth=th_depth)
        rl, rr, pts, summ = FrameResult(), FrameResult(), C.c_void_p(), StereoSummary()
        self._check(self._lib.ss_extract_stereo_raw(self._h, int(camera_id), left.ctypes.data, right.ctypes.data, w, h, ch, w * ch,
                                                    float(timestamp), int(map_left), int(map_right), C.byref(sp), C.byref(rl),
                                                    C.byref(rr), C.byref(pts), C.byref(summ)))
        return self._pair_results(rl, rr, pts, summ)

    # ---- guided matching: window search, conflicts, rotation histogram (the rule: include/sendslam_orb.h) ----
    def match_guided_pairs_device(self, d_q: int, d_q_kp: int, d_nq: int, d_t: int, d_t_kp: int, d_nt: int, d_windows: int,
                                  n_frames: int, rows_per_frame: int, params: GuidedParams, d_idx: int, d_d1: int, d_d2: int,
                                  d_summary: int):
        """n_frames independent (query, train) pairs on device arrays [n_frames][rows_per_frame] (descriptors, KP_DTYPE
        keypoints, GUIDED_WINDOW_DTYPE windows); d_summary [n_frames] GUIDED_SUMMARY_DTYPE rows; asynchronous."""
        self._check(self._lib.ss_match_guided_pairs_device(self._h, C.c_void_p(d_q), C.c_void_p(d_q_kp), C.c_void_p(d_nq), C.c_void_p(d_t),
                                                           C.c_void_p(d_t_kp), C.c_void_p(d_nt), C.c_void_p(d_windows), n_frames,
                                                           rows_per_frame, C.byref(params), C.c_void_p(d_idx), C.c_void_p(d_d1),
                                                           C.c_void_p(d_d2), C.c_void_p(d_summary)))

    def match_guided_batch_device(self, params: GuidedParams, d_idx: int, d_d1: int, d_d2: int, d_summary: int, train_src=None,
                                  d_windows: int = 0):
        """The frames of the last batch, frame b against train_src[b] (host ints; None: b - 1); d_windows [n_frames][kp_capacity]
        or 0: the windows follow from params (radius, radius_by_octave, octave_span); asynchronous."""
        src = None if train_src is None else np.ascontiguousarray(train_src, dtype=np.int32)
        self._check(self._lib.ss_match_guided_batch_device(self._h, None if src is None else src.ctypes.data, C.c_void_p(d_windows),
                                                           C.byref(params), C.c_void_p(d_idx), C.c_void_p(d_d1), C.c_void_p(d_d2),
                                                           C.c_void_p(d_summary)))

    def match_guided(self, q: np.ndarray, q_kp: np.ndarray, t: np.ndarray, t_kp: np.ndarray, windows: np.ndarray, params: GuidedParams):
        """One pair, host arrays in and out -> (idx, d1, d2, summary dict)."""
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        q_kp, t_kp = np.ascontiguousarray(q_kp, KP_DTYPE), np.ascontiguousarray(t_kp, KP_DTYPE)
        windows = np.ascontiguousarray(windows, GUIDED_WINDOW_DTYPE)
        nq, nt = len(q), len(t)
        if len(q_kp) != nq or len(windows) != nq or len(t_kp) != nt:
            raise ValueError("descriptors, keypoints and windows differ in length")
        idx, d1, d2, summ = np.empty(nq, np.int32), np.empty(nq, np.uint16), np.empty(nq, np.uint16), GuidedSummary()
        self._check(self._lib.ss_match_guided(self._h, q.ctypes.data if nq else None, q_kp.ctypes.data if nq else None, nq,
                                              t.ctypes.data if nt else None, t_kp.ctypes.data if nt else None, nt,
                                              windows.ctypes.data if nq else None, C.byref(params), idx.ctypes.data, d1.ctypes.data,
                                              d2.ctypes.data, C.byref(summ)))
        return idx, d1, d2, {n: getattr(summ, n) for n, _ in GuidedSummary._fields_}

    # ---- map-point projection search: frustum, level, window match (the rule: include/sendslam_orb.h) ----
    @staticmethod
    def _proj_tables(views, point_src, n_frames=None):
        v = _views_array(views)
        if n_frames is not None and len(v) != n_frames:
            raise ValueError("one view per frame")
        src = None if point_src is None else np.ascontiguousarray(point_src, np.int32)
        if src is not None and len(src) != len(v):
            raise ValueError("one point_src entry per frame")
        return v, src

    def match_proj_pairs_device(self, d_points: int, d_point_desc: int, d_n_points: int, n_blocks: int, point_rows: int, d_train: int,
                                d_train_kp: int, d_n_train: int, n_frames: int, rows_per_frame: int, views, params: ProjParams, d_idx: int,
                                d_d1: int, d_d2: int, d_proj: int, d_summary: int, point_src=None, d_train_right: int = 0,
                                d_train_taken: int = 0):
        """n_frames frames on device arrays: map points [n_blocks][point_rows] (MAP_POINT_DTYPE, descriptors, counts), train frames
        [n_frames][rows_per_frame]; views: n_frames ProjView (host); point_src: host ints, frame b searches block point_src[b]
        (None: block b); outputs [n_frames][point_rows], d_proj PROJ_POINT_DTYPE, d_summary PROJ_SUMMARY_DTYPE; asynchronous."""
        v, src = self._proj_tables(views, point_src, n_frames)
        self._check(self._lib.ss_match_proj_pairs_device(self._h, C.c_void_p(d_points), C.c_void_p(d_point_desc), C.c_void_p(d_n_points), n_blocks,
                                                         point_rows, C.c_void_p(d_train), C.c_void_p(d_train_kp), C.c_void_p(d_n_train),
                                                         C.c_void_p(d_train_right), C.c_void_p(d_train_taken), n_frames, rows_per_frame,
                                                         v.ctypes.data if len(v) else None, None if src is None else src.ctypes.data, C.byref(params),
                                                         C.c_void_p(d_idx), C.c_void_p(d_d1), C.c_void_p(d_d2), C.c_void_p(d_proj),
                                                         C.c_void_p(d_summary)))

    def match_proj_batch_device(self, d_points: int, d_point_desc: int, d_n_points: int, n_blocks: int, point_rows: int, views,
                                params: ProjParams, d_idx: int, d_d1: int, d_d2: int, d_proj: int, d_summary: int, point_src=None,
                                d_train_right: int = 0, d_train_taken: int = 0):
        """the same against the frames of the last batch (one view per frame of it; d_train_right / d_train_taken
        [n_frames][kp_capacity]); asynchronous."""
        v, src = self._proj_tables(views, point_src)
        self._check(self._lib.ss_match_proj_batch_device(self._h, C.c_void_p(d_points), C.c_void_p(d_point_desc), C.c_void_p(d_n_points), n_blocks,
                                                         point_rows, C.c_void_p(d_train_right), C.c_void_p(d_train_taken), v.ctypes.data,
                                                         None if src is None else src.ctypes.data, C.byref(params), C.c_void_p(d_idx),
                                                         C.c_void_p(d_d1), C.c_void_p(d_d2), C.c_void_p(d_proj), C.c_void_p(d_summary)))

    def match_proj(self, view: ProjView, points: np.ndarray, point_desc: np.ndarray, t: np.ndarray, t_kp: np.ndarray, params: ProjParams,
                   right=None, taken=None):
        """One frame, host arrays in and out -> (idx, d1, d2, PROJ_POINT_DTYPE rows, summary dict)."""
        v = _views_array(view)
        pts = np.ascontiguousarray(points, MAP_POINT_DTYPE)
        pd = np.ascontiguousarray(point_desc, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        t_kp = np.ascontiguousarray(t_kp, KP_DTYPE)
        n, nt = len(pts), len(t)
        right = None if right is None else np.ascontiguousarray(right, np.float32)
        taken = None if taken is None else np.ascontiguousarray(taken, np.uint8)
        if len(v) != 1 or len(pd) != n or len(t_kp) != nt or (right is not None and len(right) != nt) or (taken is not None and len(taken) != nt):
            raise ValueError("points, descriptors, keypoints, right coordinates and taken flags differ in length")
        idx, d1, d2 = np.empty(n, np.int32), np.empty(n, np.uint16), np.empty(n, np.uint16)
        proj, summ = np.empty(n, PROJ_POINT_DTYPE), ProjSummary()
        self._check(self._lib.ss_match_proj(self._h, v.ctypes.data, pts.ctypes.data if n else None, pd.ctypes.data if n else None, n,
                                            t.ctypes.data if nt else None, t_kp.ctypes.data if nt else None, nt,
                                            None if right is None else right.ctypes.data, None if taken is None else taken.ctypes.data,
                                            C.byref(params), idx.ctypes.data, d1.ctypes.data, d2.ctypes.data, proj.ctypes.data if n else None,
                                            C.byref(summ)))
        return idx, d1, d2, proj, {n_: getattr(summ, n_) for n_, _ in ProjSummary._fields_}

    # ---- map-point fusion: Fuse and the Sim3 projection search (the rule: include/sendslam_orb.h) ----
    def match_fuse_pairs_device(self, d_points: int, d_point_desc: int, d_n_points: int, n_blocks: int, point_rows: int, d_train: int,
                                d_train_kp: int, d_n_train: int, n_frames: int, rows_per_frame: int, views, params: FuseParams, d_idx: int,
                                d_d1: int, d_fuse: int, d_point: int, d_summary: int, point_src=None, d_point_skip: int = 0,
                                d_train_right: int = 0, d_train_taken: int = 0, d_train_point: int = 0):
        """n_frames frames on device arrays, laid out as for match_proj_pairs_device, plus d_point_skip (uint8 [n_frames][point_rows])
        and d_train_point (int32 [n_frames][rows_per_frame]); outputs [n_frames][point_rows]: d_idx, d_d1, d_fuse FUSE_ACTION_DTYPE,
        d_point FUSE_POINT_DTYPE; d_summary FUSE_SUMMARY_DTYPE; asynchronous."""
        v, src = self._proj_tables(views, point_src, n_frames)
        self._check(self._lib.ss_match_fuse_pairs_device(self._h, C.c_void_p(d_points), C.c_void_p(d_point_desc), C.c_void_p(d_n_points), n_blocks,
                                                         point_rows, C.c_void_p(d_point_skip), C.c_void_p(d_train), C.c_void_p(d_train_kp),
                                                         C.c_void_p(d_n_train), C.c_void_p(d_train_right), C.c_void_p(d_train_taken),
                                                         C.c_void_p(d_train_point), n_frames, rows_per_frame, v.ctypes.data if len(v) else None,
                                                         None if src is None else src.ctypes.data, C.byref(params), C.c_void_p(d_idx),
                                                         C.c_void_p(d_d1), C.c_void_p(d_fuse), C.c_void_p(d_point), C.c_void_p(d_summary)))

    def match_fuse_batch_device(self, d_points: int, d_point_desc: int, d_n_points: int, n_blocks: int, point_rows: int, views,
                                params: FuseParams, d_idx: int, d_d1: int, d_fuse: int, d_point: int, d_summary: int, point_src=None,
                                d_point_skip: int = 0, d_train_right: int = 0, d_train_taken: int = 0, d_train_point: int = 0):
        """the same against the frames of the last batch (one view per frame of it; the train-row arrays [n_frames][kp_capacity]);
        asynchronous."""
        v, src = self._proj_tables(views, point_src)
        self._check(self._lib.ss_match_fuse_batch_device(self._h, C.c_void_p(d_points), C.c_void_p(d_point_desc), C.c_void_p(d_n_points), n_blocks,
                                                         point_rows, C.c_void_p(d_point_skip), C.c_void_p(d_train_right), C.c_void_p(d_train_taken),
                                                         C.c_void_p(d_train_point), v.ctypes.data, None if src is None else src.ctypes.data,
                                                         C.byref(params), C.c_void_p(d_idx), C.c_void_p(d_d1), C.c_void_p(d_fuse),
                                                         C.c_void_p(d_point), C.c_void_p(d_summary)))

    def match_fuse(self, view: ProjView, points: np.ndarray, point_desc: np.ndarray, t: np.ndarray, t_kp: np.ndarray, params: FuseParams,
                   skip=None, right=None, taken=None, train_point=None):
        """One frame, host arrays in and out -> (idx, d1, FUSE_ACTION_DTYPE rows, FUSE_POINT_DTYPE rows, summary dict)."""
        v = _views_array(view)
        pts = np.ascontiguousarray(points, MAP_POINT_DTYPE)
        pd = np.ascontiguousarray(point_desc, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        t_kp = np.ascontiguousarray(t_kp, KP_DTYPE)
        n, nt = len(pts), len(t)
        skip = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        right = None if right is None else np.ascontiguousarray(right, np.float32)
        taken = None if taken is None else np.ascontiguousarray(taken, np.uint8)
        train_point = None if train_point is None else np.ascontiguousarray(train_point, np.int32)
        if len(v) != 1 or len(pd) != n or len(t_kp) != nt or (skip is not None and len(skip) != n) or \
                any(a is not None and len(a) != nt for a in (right, taken, train_point)):
            raise ValueError("points, descriptors, flags, keypoints, right coordinates and ids differ in length")
        idx, d1 = np.empty(n, np.int32), np.empty(n, np.uint16)
        fuse, point, summ = np.empty(n, FUSE_ACTION_DTYPE), np.empty(n, FUSE_POINT_DTYPE), FuseSummary()
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        self._check(self._lib.ss_match_fuse(self._h, v.ctypes.data, pts.ctypes.data if n else None, pd.ctypes.data if n else None, ptr(skip), n,
                                            t.ctypes.data if nt else None, t_kp.ctypes.data if nt else None, nt, ptr(right), ptr(taken),
                                            ptr(train_point), C.byref(params), idx.ctypes.data, d1.ctypes.data, fuse.ctypes.data,
                                            point.ctypes.data if n else None, C.byref(summ)))
        return idx, d1, fuse, point, {n_: getattr(summ, n_) for n_, _ in FuseSummary._fields_}

    # ---- bag of words: vocabulary transform, SearchByBoW, L1 score (the rule: include/sendslam_orb.h) ----
    def set_vocabulary(self, voc: Vocabulary):
        """uploads the vocabulary; the context keeps its own copy"""
        self._check(self._lib.ss_bow_set_vocabulary(self._h, voc._h))

    def bow_transform_device(self, d_desc: int, d_n_rows: int, n_frames: int, rows_per_frame: int, levelsup: int, d_word: int, d_node: int,
                             d_bow_word: int, d_bow_value: int, d_summary: int):
        """asynchronous; outputs [n_frames][rows_per_frame] int32 / int32 / int32 / float64 and [n_frames] BOW_SUMMARY_DTYPE"""
        self._check(self._lib.ss_bow_transform_device(self._h, C.c_void_p(d_desc), C.c_void_p(d_n_rows), n_frames, rows_per_frame, int(levelsup),
                                                      C.c_void_p(d_word), C.c_void_p(d_node), C.c_void_p(d_bow_word), C.c_void_p(d_bow_value),
                                                      C.c_void_p(d_summary)))

    def bow_transform_batch_device(self, levelsup: int, d_word: int, d_node: int, d_bow_word: int, d_bow_value: int, d_summary: int):
        """the frames of the last batch; outputs [n_frames][kp_capacity]"""
        self._check(self._lib.ss_bow_transform_batch_device(self._h, int(levelsup), C.c_void_p(d_word), C.c_void_p(d_node), C.c_void_p(d_bow_word),
                                                            C.c_void_p(d_bow_value), C.c_void_p(d_summary)))

    def match_bow_pairs_device(self, d_q: int, d_q_kp: int, d_q_node: int, d_nq: int, d_t: int, d_t_kp: int, d_t_node: int, d_nt: int,
                               n_frames: int, rows_per_frame: int, params: GuidedParams, d_idx: int, d_d1: int, d_d2: int, d_summary: int):
        self._check(self._lib.ss_match_bow_pairs_device(self._h, C.c_void_p(d_q), C.c_void_p(d_q_kp), C.c_void_p(d_q_node), C.c_void_p(d_nq),
                                                        C.c_void_p(d_t), C.c_void_p(d_t_kp), C.c_void_p(d_t_node), C.c_void_p(d_nt), n_frames,
                                                        rows_per_frame, C.byref(params), C.c_void_p(d_idx), C.c_void_p(d_d1), C.c_void_p(d_d2),
                                                        C.c_void_p(d_summary)))

    def match_bow_batch_device(self, params: GuidedParams, d_idx: int, d_d1: int, d_d2: int, d_summary: int, train_src=None):
        """the frames and nodes of the last bow_transform_batch_device; train_src as in match_guided_batch_device"""
        src = None if train_src is None else np.ascontiguousarray(train_src, np.int32)
        self._check(self._lib.ss_match_bow_batch_device(self._h, None if src is None else src.ctypes.data, C.byref(params), C.c_void_p(d_idx),
                                                        C.c_void_p(d_d1), C.c_void_p(d_d2), C.c_void_p(d_summary)))

    def bow_score_device(self, d_q_word: int, d_q_value: int, d_q_count: int, q_rows: int, d_db_word: int, d_db_value: int, d_db_count: int,
                         n_db: int, stride: int, d_score: int):
        """one query vector against n_db kept vectors [n_db][stride] -> float64 [n_db]; asynchronous"""
        self._check(self._lib.ss_bow_score_device(self._h, C.c_void_p(d_q_word), C.c_void_p(d_q_value), C.c_void_p(d_q_count), int(q_rows),
                                                  C.c_void_p(d_db_word), C.c_void_p(d_db_value), C.c_void_p(d_db_count), int(n_db), int(stride),
                                                  C.c_void_p(d_score)))

    # ---- epipolar search and triangulation: new map points from pairs (the rule: include/sendslam_orb.h) ----
    def match_epi_pairs_device(self, d_q: int, d_q_kp: int, d_q_node: int, d_nq: int, d_t: int, d_t_kp: int, d_t_node: int, d_nt: int,
                               n_frames: int, rows_per_frame: int, pairs, params: EpiParams, d_idx: int, d_d1: int, d_summary: int,
                               d_q_taken: int = 0, d_t_taken: int = 0):
        """n_frames pairs on device arrays [n_frames][rows_per_frame] (those of match_bow_pairs_device, uint8 taken flags or 0);
        pairs: n_frames EpiPair (host); outputs d_idx int32 / d_d1 uint16, d_summary EPI_SUMMARY_DTYPE; asynchronous."""
        w = _pairs_array(pairs)
        if len(w) != n_frames:
            raise ValueError("one pair per frame")
        self._check(self._lib.ss_match_epi_pairs_device(self._h, C.c_void_p(d_q), C.c_void_p(d_q_kp), C.c_void_p(d_q_node), C.c_void_p(d_q_taken),
                                                        C.c_void_p(d_nq), C.c_void_p(d_t), C.c_void_p(d_t_kp), C.c_void_p(d_t_node),
                                                        C.c_void_p(d_t_taken), C.c_void_p(d_nt), n_frames, rows_per_frame,
                                                        w.ctypes.data if len(w) else None, C.byref(params), C.c_void_p(d_idx), C.c_void_p(d_d1),
                                                        C.c_void_p(d_summary)))

    def match_epi_batch_device(self, pairs, params: EpiParams, d_idx: int, d_d1: int, d_summary: int, train_src=None, d_taken: int = 0):
        """the frames and nodes of the last bow_transform_batch_device, frame b against train_src[b] (None: b - 1) under pairs[b];
        d_taken uint8 [n_frames][kp_capacity] for both sides, or 0; asynchronous."""
        w = _pairs_array(pairs)
        src = None if train_src is None else np.ascontiguousarray(train_src, np.int32)
        self._check(self._lib.ss_match_epi_batch_device(self._h, None if src is None else src.ctypes.data, C.c_void_p(d_taken), w.ctypes.data,
                                                        C.byref(params), C.c_void_p(d_idx), C.c_void_p(d_d1), C.c_void_p(d_summary)))

    def triangulate_pairs_device(self, d_q: int, d_q_kp: int, d_nq: int, d_t_kp: int, d_nt: int, d_idx: int, n_frames: int,
                                 rows_per_frame: int, pairs, params: TriParams, d_info: int, d_points: int, d_point_desc: int,
                                 d_point_rows: int, d_n_points: int, d_summary: int):
        """triangulates the matches d_idx of n_frames pairs; d_info TRI_INFO_DTYPE [n_frames][rows_per_frame]; the compact
        d_points (MAP_POINT_DTYPE) / d_point_desc / d_point_rows (int32 pairs) and d_n_points are the blocks match_proj_pairs_device
        reads; d_summary TRI_SUMMARY_DTYPE; asynchronous."""
        w = _pairs_array(pairs)
        if len(w) != n_frames:
            raise ValueError("one pair per frame")
        self._check(self._lib.ss_triangulate_pairs_device(self._h, C.c_void_p(d_q), C.c_void_p(d_q_kp), C.c_void_p(d_nq), C.c_void_p(d_t_kp),
                                                          C.c_void_p(d_nt), C.c_void_p(d_idx), n_frames, rows_per_frame,
                                                          w.ctypes.data if len(w) else None, C.byref(params), C.c_void_p(d_info),
                                                          C.c_void_p(d_points), C.c_void_p(d_point_desc), C.c_void_p(d_point_rows),
                                                          C.c_void_p(d_n_points), C.c_void_p(d_summary)))

    def triangulate_batch_device(self, d_idx: int, pairs, params: TriParams, d_info: int, d_points: int, d_point_desc: int, d_point_rows: int,
                                 d_n_points: int, d_summary: int, train_src=None):
        """the same on the frames of the last batch, frame b against train_src[b] (None: b - 1); asynchronous."""
        w = _pairs_array(pairs)
        src = None if train_src is None else np.ascontiguousarray(train_src, np.int32)
        self._check(self._lib.ss_triangulate_batch_device(self._h, None if src is None else src.ctypes.data, C.c_void_p(d_idx), w.ctypes.data,
                                                          C.byref(params), C.c_void_p(d_info), C.c_void_p(d_points), C.c_void_p(d_point_desc),
                                                          C.c_void_p(d_point_rows), C.c_void_p(d_n_points), C.c_void_p(d_summary)))

    # ---- Sim3 from matched map points: Horn RANSAC per loop candidate (the rule: include/sendslam_orb.h) ----
    def sim3_pairs_device(self, d_query_xyz: int, d_query_kp: int, d_n_query: int, d_train_xyz: int, d_train_kp: int, d_n_train: int, d_idx: int,
                          n_pairs: int, rows: int, views1, views2, params: Sim3Params, d_inlier: int, d_result: int, d_query_skip: int = 0,
                          d_train_skip: int = 0):
        """n_pairs pairs on device arrays: MAP_POINT_DTYPE / KP_DTYPE [n_pairs][rows] of either side, optional skip bytes, counts, d_idx as
        match_bow_pairs_device wrote it; views1 / views2 host views, one per pair each; d_inlier uint8 [n_pairs][rows] by query row,
        d_result SIM3_RESULT_DTYPE [n_pairs]; asynchronous."""
        v1, v2 = _views_array(views1), _views_array(views2)
        if len(v1) != n_pairs or len(v2) != n_pairs:
            raise ValueError("one view of either keyframe per pair")
        self._check(self._lib.ss_sim3_pairs_device(self._h, C.c_void_p(d_query_xyz), C.c_void_p(d_query_kp), C.c_void_p(d_query_skip),
                                                   C.c_void_p(d_n_query), C.c_void_p(d_train_xyz), C.c_void_p(d_train_kp), C.c_void_p(d_train_skip),
                                                   C.c_void_p(d_n_train), C.c_void_p(d_idx), n_pairs, rows, v1.ctypes.data if n_pairs else None,
                                                   v2.ctypes.data if n_pairs else None, C.byref(params), C.c_void_p(d_inlier), C.c_void_p(d_result)))

    def sim3_batch_device(self, d_xyz: int, d_idx: int, views, params: Sim3Params, d_inlier: int, d_result: int, train_src=None, d_skip: int = 0):
        """the same on the frames of the last batch, frame b against train_src[b] (None: b - 1): d_xyz MAP_POINT_DTYPE
        [n_frames][kp_capacity], views one per frame; asynchronous."""
        v = _views_array(views)
        src = None if train_src is None else np.ascontiguousarray(train_src, np.int32)
        self._check(self._lib.ss_sim3_batch_device(self._h, None if src is None else src.ctypes.data, C.c_void_p(d_xyz), C.c_void_p(d_skip),
                                                   C.c_void_p(d_idx), v.ctypes.data, C.byref(params), C.c_void_p(d_inlier), C.c_void_p(d_result)))

    def sim3(self, view1, q_xyz: np.ndarray, q_kp: np.ndarray, view2, t_xyz: np.ndarray, t_kp: np.ndarray, idx: np.ndarray, params: Sim3Params,
             q_skip=None, t_skip=None):
        """One pair, host arrays in and out -> (uint8 inlier flag per query row, SIM3_RESULT_DTYPE record)."""
        v1, v2 = _views_array(view1), _views_array(view2)
        qx, tx = np.ascontiguousarray(q_xyz, MAP_POINT_DTYPE), np.ascontiguousarray(t_xyz, MAP_POINT_DTYPE)
        qk, tk = np.ascontiguousarray(q_kp, KP_DTYPE), np.ascontiguousarray(t_kp, KP_DTYPE)
        ix = np.ascontiguousarray(idx, np.int32)
        nq, nt = len(qx), len(tx)
        q_skip = None if q_skip is None else np.ascontiguousarray(q_skip, np.uint8)
        t_skip = None if t_skip is None else np.ascontiguousarray(t_skip, np.uint8)
        if len(v1) != 1 or len(v2) != 1 or len(qk) != nq or len(ix) != nq or len(tk) != nt or (q_skip is not None and len(q_skip) != nq) or \
                (t_skip is not None and len(t_skip) != nt):
            raise ValueError("views, map points, keypoints, flags and matches differ in length")
        inlier, res = np.empty(nq, np.uint8), np.zeros(1, SIM3_RESULT_DTYPE)
        ptr = lambda a, n: None if a is None or not n else a.ctypes.data  # noqa: E731
        self._check(self._lib.ss_sim3(self._h, v1.ctypes.data, ptr(qx, nq), ptr(qk, nq), ptr(q_skip, nq), nq, v2.ctypes.data, ptr(tx, nt), ptr(tk, nt),
                                      ptr(t_skip, nt), nt, ptr(ix, nq), C.byref(params), ptr(inlier, nq), res.ctypes.data))
        return inlier, res[0]

    # ---- pose-only optimisation: Gauss-Newton per frame of a batch (the rule: include/sendslam_orb.h) ----
    def pose_opt_pairs_device(self, d_points: int, d_n_points: int, n_blocks: int, point_rows: int, d_kp: int, d_n_kp: int, n_frames: int,
                              rows_per_frame: int, d_idx: int, views, start_poses, params: PoseOptParams, d_flags: int, d_result: int,
                              point_src=None, d_point_skip: int = 0, d_right: int = 0):
        """n_frames frames on device arrays: map points [n_blocks][point_rows] (MAP_POINT_DTYPE, optional skip bytes, counts), keypoints
        KP_DTYPE [n_frames][rows_per_frame] (optional right coordinates, counts), d_idx as match_proj_* (or, with idx_by_row, match_bow_*)
        wrote it; views and start_poses (twelve doubles each) host tables, one per frame; d_flags uint8 [n_frames][slots], d_result
        POSE_RESULT_DTYPE [n_frames]; asynchronous."""
        v, src = self._proj_tables(views, point_src, n_frames)
        st = _start_array(start_poses, n_frames)
        self._check(self._lib.ss_pose_opt_pairs_device(self._h, C.c_void_p(d_points), C.c_void_p(d_point_skip), C.c_void_p(d_n_points), n_blocks,
                                                       point_rows, C.c_void_p(d_kp), C.c_void_p(d_right), C.c_void_p(d_n_kp), n_frames,
                                                       rows_per_frame, C.c_void_p(d_idx), v.ctypes.data if n_frames else None,
                                                       st.ctypes.data if n_frames else None, None if src is None else src.ctypes.data,
                                                       C.byref(params), C.c_void_p(d_flags), C.c_void_p(d_result)))

    def pose_opt_batch_device(self, d_points: int, d_n_points: int, n_blocks: int, point_rows: int, d_idx: int, views, start_poses,
                              params: PoseOptParams, d_flags: int, d_result: int, point_src=None, d_point_skip: int = 0, d_right: int = 0):
        """the same, the keypoints being the frames of the last batch (rows_per_frame = kp_capacity); asynchronous."""
        v, src = self._proj_tables(views, point_src)
        st = _start_array(start_poses, len(v))
        self._check(self._lib.ss_pose_opt_batch_device(self._h, C.c_void_p(d_points), C.c_void_p(d_point_skip), C.c_void_p(d_n_points), n_blocks,
                                                       point_rows, C.c_void_p(d_right), C.c_void_p(d_idx), v.ctypes.data, st.ctypes.data,
                                                       None if src is None else src.ctypes.data, C.byref(params), C.c_void_p(d_flags),
                                                       C.c_void_p(d_result)))

    def pose_opt(self, view, start, points: np.ndarray, kp: np.ndarray, idx: np.ndarray, params: PoseOptParams, skip=None, right=None):
        """One frame, host arrays in and out -> (uint8 flag per slot, POSE_RESULT_DTYPE record)."""
        v = _views_array(view)
        st = _start_array(start, 1)
        pts, k = np.ascontiguousarray(points, MAP_POINT_DTYPE), np.ascontiguousarray(kp, KP_DTYPE)
        ix = np.ascontiguousarray(idx, np.int32)
        n_p, n_k = len(pts), len(k)
        ns = n_k if params.idx_by_row else n_p
        skip = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        right = None if right is None else np.ascontiguousarray(right, np.float32)
        if len(v) != 1 or len(ix) != ns or (skip is not None and len(skip) != n_p) or (right is not None and len(right) != n_k):
            raise ValueError("view, map points, keypoints, flags and matches differ in length")
        flags, res = np.empty(ns, np.uint8), np.zeros(1, POSE_RESULT_DTYPE)
        ptr = lambda a, n: None if a is None or not n else a.ctypes.data  # noqa: E731
        self._check(self._lib.ss_pose_opt(self._h, v.ctypes.data, st.ctypes.data, ptr(pts, n_p), ptr(skip, n_p), n_p, ptr(k, n_k), ptr(right, n_k),
                                          n_k, ptr(ix, ns), C.byref(params), ptr(flags, ns), res.ctypes.data))
        return flags, res[0]

    # ---- local bundle adjustment: Schur-reduced steps per local map (the rule: include/sendslam_orb.h) ----
    @staticmethod
    def _ba_tables(problems, views, start_poses, n_frames):
        pr = np.ascontiguousarray(problems, BA_PROBLEM_DTYPE).reshape(-1)
        v = _views_array(views)
        if n_frames is not None and len(v) != n_frames:
            raise ValueError("one view per frame")
        return pr, v, _start_array(start_poses, len(v))

    def local_ba_pairs_device(self, d_points: int, d_n_points: int, n_blocks: int, point_rows: int, d_kp: int, d_n_kp: int, n_frames: int,
                              rows_per_frame: int, d_idx: int, problems, views, start_poses, params: BaParams, d_poses: int, d_xyz: int,
                              d_point_flags: int, d_obs_flags: int, d_result: int, d_point_skip: int = 0, d_right: int = 0):
        """the problems (BA_PROBLEM_DTYPE, a host table) of one call on device arrays: map points and keypoints as for
        pose_opt_pairs_device, d_idx int32 [n_frames][point_rows]; views and start_poses host tables, one per frame; d_poses float64
        [n_frames][12], d_xyz float64 [n_problems][point_rows][3], d_point_flags uint8 [n_problems][point_rows], d_obs_flags uint8
        [n_frames][point_rows], d_result BA_RESULT_DTYPE [n_problems]; asynchronous."""
        pr, v, st = self._ba_tables(problems, views, start_poses, n_frames)
        self._check(self._lib.ss_local_ba_pairs_device(self._h, C.c_void_p(d_points), C.c_void_p(d_point_skip), C.c_void_p(d_n_points), n_blocks,
                                                       point_rows, C.c_void_p(d_kp), C.c_void_p(d_right), C.c_void_p(d_n_kp), n_frames,
                                                       rows_per_frame, C.c_void_p(d_idx), pr.ctypes.data if len(pr) else None, len(pr),
                                                       v.ctypes.data if n_frames else None, st.ctypes.data if n_frames else None,
                                                       C.byref(params), C.c_void_p(d_poses), C.c_void_p(d_xyz), C.c_void_p(d_point_flags),
                                                       C.c_void_p(d_obs_flags), C.c_void_p(d_result)))

    def local_ba_batch_device(self, d_points: int, d_n_points: int, n_blocks: int, point_rows: int, d_idx: int, problems, views, start_poses,
                              params: BaParams, d_poses: int, d_xyz: int, d_point_flags: int, d_obs_flags: int, d_result: int,
                              d_point_skip: int = 0, d_right: int = 0):
        """the same, the keyframes being the frames of the last batch (rows_per_frame = kp_capacity); asynchronous."""
        pr, v, st = self._ba_tables(problems, views, start_poses, None)
        self._check(self._lib.ss_local_ba_batch_device(self._h, C.c_void_p(d_points), C.c_void_p(d_point_skip), C.c_void_p(d_n_points), n_blocks,
                                                       point_rows, C.c_void_p(d_right), C.c_void_p(d_idx), pr.ctypes.data if len(pr) else None,
                                                       len(pr), v.ctypes.data, st.ctypes.data, C.byref(params), C.c_void_p(d_poses),
                                                       C.c_void_p(d_xyz), C.c_void_p(d_point_flags), C.c_void_p(d_obs_flags), C.c_void_p(d_result)))

    def local_ba(self, views, start, n_free: int, points: np.ndarray, kp: np.ndarray, idx: np.ndarray, params: BaParams, n_kp=None, skip=None,
                 right=None):
        """One problem, host arrays in and out -> what local_ba_host returns."""
        v, st, pts, k, ix, nk, skip, right = _ba_host_arrays(views, start, points, kp, idx, n_kp, skip, right)
        n_kf, n_p = len(v), len(pts)
        poses, xyz = np.empty((n_kf, 12), np.float64), np.empty((n_p, 3), np.float64)
        pf, of, res = np.empty(n_p, np.uint8), np.empty((n_kf, n_p), np.uint8), np.zeros(1, BA_RESULT_DTYPE)
        ptr = lambda a, n: None if a is None or not n else a.ctypes.data  # noqa: E731
        self._check(self._lib.ss_local_ba(self._h, v.ctypes.data, st.ctypes.data, n_kf, n_free, ptr(pts, n_p), ptr(skip, n_p), n_p, k.ctypes.data,
                                          ptr(right, 1), nk.ctypes.data, k.shape[1], ptr(ix, n_p), C.byref(params), poses.ctypes.data,
                                          ptr(xyz, n_p), ptr(pf, n_p), ptr(of, n_p), res.ctypes.data))
        return poses, xyz, pf, of, res[0]

    def local_ba_points_to_block(self, d_xyz: int, d_point_flags: int, n_problems: int, point_rows: int, d_points: int, n_blocks: int,
                                 block_of=None):
        """x, y, z of the points of n_problems problems rounded into their blocks of MAP_POINT_DTYPE (block_of: host ints, or problem q
        into block q); rows flagged 2 and the other fields stay; asynchronous."""
        bo = None if block_of is None else np.ascontiguousarray(block_of, np.int32)
        if bo is not None and len(bo) != n_problems:
            raise ValueError("one block number per problem")
        self._check(self._lib.ss_local_ba_points_to_block(self._h, C.c_void_p(d_xyz), C.c_void_p(d_point_flags), n_problems, point_rows,
                                                          None if bo is None else bo.ctypes.data, C.c_void_p(d_points), n_blocks))

    # ---- essential-graph optimisation: the Sim3 pose graph of a closed loop (the rule: include/sendslam_orb.h) ----
    def pose_graph_device(self, d_nc: int, d_start: int, d_fixed: int, n_kf: int, problems, edges, params: GraphParams, d_sim3: int, d_poses: int,
                          d_result: int):
        """the problems (GRAPH_PROBLEM_DTYPE, a host table) of one call on device arrays: d_nc and d_start float64 [n_kf][13], d_fixed uint8
        [n_kf]; edges a host table int32 [n_edges][2] of the call's keyframe numbers; d_sim3 float64 [n_kf][13], d_poses float64 [n_kf][12],
        d_result GRAPH_RESULT_DTYPE [n_problems]; asynchronous."""
        pr = np.ascontiguousarray(problems, GRAPH_PROBLEM_DTYPE).reshape(-1)
        ed = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
        self._check(self._lib.ss_pose_graph_device(self._h, C.c_void_p(d_nc), C.c_void_p(d_start), C.c_void_p(d_fixed), n_kf,
                                                   pr.ctypes.data if len(pr) else None, len(pr), ed.ctypes.data if len(ed) else None, len(ed),
                                                   C.byref(params), C.c_void_p(d_sim3), C.c_void_p(d_poses), C.c_void_p(d_result)))

    def pose_graph(self, nc, start, fixed, edges, params: GraphParams):
        """One problem, host arrays in and out -> what pose_graph_host returns."""
        nc, st, fx, ed = _graph_host_arrays(nc, start, fixed, edges)
        n_kf = len(nc)
        sim3, poses, res = np.empty((n_kf, 13), np.float64), np.empty((n_kf, 12), np.float64), np.zeros(1, GRAPH_RESULT_DTYPE)
        self._check(self._lib.ss_pose_graph(self._h, nc.ctypes.data, st.ctypes.data, fx.ctypes.data, n_kf, ed.ctypes.data if len(ed) else None,
                                            len(ed), C.byref(params), sim3.ctypes.data, poses.ctypes.data, res.ctypes.data))
        return sim3, poses, res[0]

    def pose_graph_points_device(self, d_points: int, d_ref: int, n_blocks: int, point_rows: int, d_nc: int, d_sim3: int, n_kf: int):
        """x, y, z of every row of the blocks of MAP_POINT_DTYPE whose d_ref entry (int32 [n_blocks][point_rows]) names a keyframe of the call
        move with that keyframe: x <- S^-1(N(x)); the other fields and the rows with another entry (-1) stay; asynchronous."""
        self._check(self._lib.ss_pose_graph_points_device(self._h, C.c_void_p(d_points), C.c_void_p(d_ref), n_blocks, point_rows, C.c_void_p(d_nc),
                                                          C.c_void_p(d_sim3), n_kf))

    # ---- global bundle adjustment: Schur PCG over a whole map (the rule: include/sendslam_orb.h) ----
    def global_ba_device(self, d_points: int, d_n_points: int, n_blocks: int, point_rows: int, d_start: int, d_fixed: int, n_kf: int, problems, obs,
                         views, params: GbaParams, d_poses: int, d_xyz: int, d_point_flags: int, d_obs_flags: int, d_result: int,
                         d_point_skip: int = 0):
        """the problems (GBA_PROBLEM_DTYPE), the observation records (GBA_OBS_DTYPE, any order) and the views (one per keyframe) are host
        tables; d_start float64 [n_kf][12] (pose_graph_device's d_poses feeds it), d_fixed uint8 [n_kf], map points as for
        local_ba_pairs_device; d_poses float64 [n_kf][12], d_xyz float64 [n_blocks][point_rows][3], d_point_flags uint8
        [n_blocks][point_rows], d_obs_flags uint8 [n_obs] in the order of obs, d_result GBA_RESULT_DTYPE [n_problems]; asynchronous."""
        pr = np.ascontiguousarray(problems, GBA_PROBLEM_DTYPE).reshape(-1)
        ob = np.ascontiguousarray(obs, GBA_OBS_DTYPE).reshape(-1)
        v = _views_array(views)
        if len(v) != n_kf:
            raise ValueError("one view per keyframe")
        self._check(self._lib.ss_global_ba_device(self._h, C.c_void_p(d_points), C.c_void_p(d_point_skip), C.c_void_p(d_n_points), n_blocks, point_rows,
                                                  C.c_void_p(d_start), C.c_void_p(d_fixed), n_kf, pr.ctypes.data if len(pr) else None, len(pr),
                                                  ob.ctypes.data if len(ob) else None, len(ob), v.ctypes.data if n_kf else None, C.byref(params),
                                                  C.c_void_p(d_poses), C.c_void_p(d_xyz), C.c_void_p(d_point_flags), C.c_void_p(d_obs_flags),
                                                  C.c_void_p(d_result)))

    def global_ba(self, views, start, fixed, points: np.ndarray, obs: np.ndarray, params: GbaParams, skip=None):
        """One problem, host arrays in and out -> what global_ba_host returns."""
        v, st, fx, pts, ob, skip = _gba_host_arrays(views, start, fixed, points, obs, skip)
        n_kf, n_p, n_o = len(v), len(pts), len(ob)
        poses, xyz = np.empty((n_kf, 12), np.float64), np.empty((n_p, 3), np.float64)
        pf, of, res = np.empty(n_p, np.uint8), np.empty(n_o, np.uint8), np.zeros(1, GBA_RESULT_DTYPE)
        ptr = lambda a, n: None if a is None or not n else a.ctypes.data  # noqa: E731
        self._check(self._lib.ss_global_ba(self._h, ptr(v, n_kf), ptr(st, n_kf), ptr(fx, n_kf), n_kf, ptr(pts, n_p), ptr(skip, n_p), n_p, ptr(ob, n_o), n_o,
                                           C.byref(params), poses.ctypes.data, ptr(xyz, n_p), ptr(pf, n_p), ptr(of, n_o), res.ctypes.data))
        return poses, xyz, pf, of, res[0]

    # ---- covisibility: neighbour lists and culling counts from the map's incidence lists (the rule: include/sendslam_orb.h) ----
    def covis_set_map(self, problems, n_kf: int, n_blocks: int, point_rows: int, obs, cull_skip=None, check_right: bool = False, obs_row=None):
        """the problems (GBA_PROBLEM_DTYPE) and the observation records (GBA_OBS_DTYPE, any order) global_ba_device takes, and optionally
        one skip byte per record; the context keeps the map until the next call.  No problem clears it.  obs_row (int32, one per record:
        its keypoint row in its keyframe) goes through ss_covis_set_map_rows: refresh_device needs it for the descriptors."""
        pr, ob, sk = _covis_map_arrays(problems, obs, cull_skip)
        args = (self._h, pr.ctypes.data if len(pr) else None, len(pr), n_kf, n_blocks, point_rows, ob.ctypes.data if len(ob) else None, len(ob),
                None if sk is None or not len(sk) else sk.ctypes.data, int(check_right))
        if obs_row is None:
            self._check(self._lib.ss_covis_set_map(*args))
            return
        rows = np.ascontiguousarray(obs_row, np.int32).reshape(-1)
        if len(rows) != len(ob):
            raise ValueError("one keypoint row per observation record")
        self._check(self._lib.ss_covis_set_map_rows(*args, rows.ctypes.data if len(rows) else np.zeros(1, np.int32).ctypes.data))

    def refresh_device(self, d_points: int, d_point_desc: int, d_n_points: int, d_desc: int, rows_per_frame: int, views, params: RefreshParams,
                       d_info: int, d_summary: int, d_ref_kf: int = 0, d_select: int = 0):
        """UpdateNormalAndDepth and ComputeDistinctiveDescriptors over the context's map (covis_set_map with obs_row): d_points MAP_POINT_DTYPE
        [n_blocks][point_rows] and d_point_desc uint8 [n_blocks][point_rows][32] are refreshed in place; d_desc uint8
        [n_kf][rows_per_frame][32]; views one per keyframe of the map (only ow is read); d_ref_kf int32 and d_select uint8
        [n_blocks][point_rows] or 0 (the d_point_flags of local_ba / global_ba serve as d_select); d_info REFRESH_INFO_DTYPE
        [n_blocks][point_rows], d_summary REFRESH_SUMMARY_DTYPE [n_blocks]; asynchronous."""
        v = _views_array(views)
        self._check(self._lib.ss_refresh_device(self._h, C.c_void_p(d_points), C.c_void_p(d_point_desc), C.c_void_p(d_n_points), C.c_void_p(d_ref_kf),
                                                C.c_void_p(d_select), C.c_void_p(d_desc), rows_per_frame, v.ctypes.data if len(v) else None, C.byref(params),
                                                C.c_void_p(d_info), C.c_void_p(d_summary)))

    def refresh(self, views, points, point_desc, obs, obs_row, desc, params: RefreshParams, ref_kf=None, select=None, check_right: bool = False):
        """One problem, host arrays in and out -> (points, point_desc, info, summary) as refresh_host returns them for one block of
        len(points) rows (more than 16384 points: blocks of 16384); the map of the context becomes this one."""
        v = _views_array(views)
        pts = np.array(points, MAP_POINT_DTYPE).reshape(-1)
        n = len(pts)
        pd = None if point_desc is None else np.array(point_desc, np.uint8).reshape(n, 32)
        _, ob, _ = _covis_map_arrays(np.zeros(0, GBA_PROBLEM_DTYPE), obs, None)
        rows = None if obs_row is None else np.ascontiguousarray(obs_row, np.int32).reshape(-1)
        rk = None if ref_kf is None else np.ascontiguousarray(ref_kf, np.int32).reshape(-1)
        sel = None if select is None else np.ascontiguousarray(select, np.uint8).reshape(-1)
        ds = None if desc is None else np.ascontiguousarray(desc, np.uint8)
        pr = min(max(n, 1), SS_GUIDED_MAX_ROWS)
        info, summary = np.zeros(n, REFRESH_INFO_DTYPE), np.zeros((n + pr - 1) // pr, REFRESH_SUMMARY_DTYPE)
        ptr = lambda a: None if a is None or not a.size else a.ctypes.data  # noqa: E731
        self._check(self._lib.ss_refresh(self._h, ptr(v), len(v), ptr(pts), ptr(pd), n, ptr(rk), ptr(sel), ptr(ob), ptr(rows), len(ob), int(check_right), ptr(ds),
                                         _refresh_rows(ds, len(v), None), C.byref(params), ptr(info), ptr(summary)))
        return pts, pd, info, summary


    def covis_kf_device(self, rows, n_rows: int, params: CovisParams, cap: int, d_nb: int, d_row: int):
        """rows: call keyframe numbers (any order, duplicates allowed) or None: every keyframe of the map; d_nb int32 [n_rows][cap][2],
        d_row COVIS_ROW_DTYPE [n_rows]; asynchronous."""
        rw = None if rows is None else np.ascontiguousarray(rows, np.int32).reshape(-1)
        if rw is not None and len(rw) != n_rows:
            raise ValueError("one keyframe number per row")
        self._check(self._lib.ss_covis_kf_device(self._h, None if rw is None or not n_rows else rw.ctypes.data, n_rows, C.byref(params), cap,
                                                 C.c_void_p(d_nb), C.c_void_p(d_row)))

    def covis_frames_device(self, d_idx: int, d_n_points: int, point_src, params: CovisParams, cap: int, d_nb: int, d_row: int):
        """d_idx int32 [n_frames][point_rows] as match_proj_batch_device wrote it, d_n_points int32 [n_blocks] of the map's blocks, point_src
        the block of each frame; outputs as covis_kf_device; asynchronous."""
        ps = np.ascontiguousarray(point_src, np.int32).reshape(-1)
        self._check(self._lib.ss_covis_frames_device(self._h, C.c_void_p(d_idx), C.c_void_p(d_n_points), ps.ctypes.data if len(ps) else None, len(ps),
                                                     C.byref(params), cap, C.c_void_p(d_nb), C.c_void_p(d_row)))

    def covis(self, n_kf: int, n_points: int, obs, params: CovisParams, cap: int, cull_skip=None, check_right: bool = False):
        """One problem, host arrays in and out -> what covis_kf_host returns for every keyframe; the map of the context becomes this one."""
        _, ob, sk = _covis_map_arrays(np.zeros(0, GBA_PROBLEM_DTYPE), obs, cull_skip)
        nb, row = np.full((max(n_kf, 0), max(cap, 1), 2), 0x5A5A5A5A, np.int32), np.zeros(max(n_kf, 0), COVIS_ROW_DTYPE)
        self._check(self._lib.ss_covis(self._h, n_kf, n_points, ob.ctypes.data if len(ob) else None, len(ob),
                                       None if sk is None or not len(sk) else sk.ctypes.data, int(check_right), C.byref(params), cap,
                                       nb.ctypes.data if nb.size else None, row.ctypes.data if len(row) else None))
        return nb, row

    # ---- place recognition: loop and relocalisation candidates from an inverted file (the rule: include/sendslam_orb.h) ----
    def place_set_database(self, d_db_word: int, d_db_value: int, d_db_count: int, n_db: int, stride: int, n_words: int, problems, d_db_skip: int = 0):
        """d_db_word int32 / d_db_value float64 [n_db][stride], d_db_count int32 [n_db], d_db_skip uint8 [n_db] or 0: the caller's device
        arrays, which the context reads again at every query; problems GBA_PROBLEM_DTYPE (only first_kf and n_kf are read).  Builds the
        inverted file on the device; asynchronous.  n_db 0 clears the database."""
        pr = np.ascontiguousarray(problems, GBA_PROBLEM_DTYPE).reshape(-1)
        self._check(self._lib.ss_place_set_database(self._h, C.c_void_p(d_db_word), C.c_void_p(d_db_value), C.c_void_p(d_db_count), C.c_void_p(d_db_skip), n_db,
                                                    stride, n_words, pr.ctypes.data if len(pr) else None, len(pr)))

    def place_query_device(self, d_q_word: int, d_q_value: int, d_q_count: int, q_stride: int, q_kf, q_problem, d_nb: int, nb_cap: int, params: PlaceParams,
                           cand_cap: int, d_cand: int, d_summary: int, d_words: int = 0, d_score: int = 0, d_q_nb: int = 0, d_q_row: int = 0, q_cap: int = 0):
        """len(q_kf) queries: d_q_word / d_q_value [n_q][q_stride], d_q_count [n_q]; q_kf, q_problem host tables; d_q_nb int32 [n_q][q_cap][2]
        and d_q_row COVIS_ROW_DTYPE [n_q] as covis_kf_device wrote them, or 0; d_nb int32 [n_db][nb_cap][2]; d_cand PLACE_CAND_DTYPE
        [n_q][cand_cap], d_summary PLACE_SUMMARY_DTYPE [n_q], d_words int32 / d_score float32 [n_q][n_db] or 0; asynchronous."""
        qk = np.ascontiguousarray(q_kf, np.int32).reshape(-1)
        qp = np.ascontiguousarray(q_problem, np.int32).reshape(-1)
        if len(qk) != len(qp):
            raise ValueError("one q_kf and q_problem per query")
        self._check(self._lib.ss_place_query_device(self._h, C.c_void_p(d_q_word), C.c_void_p(d_q_value), C.c_void_p(d_q_count), q_stride, len(qk),
                                                    qk.ctypes.data if len(qk) else None, qp.ctypes.data if len(qp) else None, C.c_void_p(d_q_nb),
                                                    C.c_void_p(d_q_row), q_cap, C.c_void_p(d_nb), nb_cap, C.byref(params), cand_cap, C.c_void_p(d_cand),
                                                    C.c_void_p(d_summary), C.c_void_p(d_words), C.c_void_p(d_score)))

    def place(self, db_word, db_value, db_count, n_words: int, problems, q_word, q_value, q_count, q_kf, q_problem, nb, params: PlaceParams, cand_cap: int,
              db_skip=None, q_nb=None, q_row=None):
        """One database and its queries, host arrays in and out -> what place_query_host returns; the context's database is left cleared."""
        dw, dv, dc, sk, pr, qw, qv, qc, qk, qp, qn, qr, q_cap, nbr = _place_arrays(db_word, db_value, db_count, db_skip, problems, q_word, q_value, q_count,
                                                                                   q_kf, q_problem, q_nb, q_row, nb)
        n_db, n_q = len(dc), len(qc)
        cand, summary, words, score = _place_outputs(n_q, n_db, cand_cap)
        ptr = lambda a: None if a is None or not a.size else a.ctypes.data  # noqa: E731
        self._check(self._lib.ss_place(self._h, ptr(dw), ptr(dv), ptr(dc), ptr(sk), n_db, dw.shape[1], n_words, ptr(pr), len(pr), ptr(qw), ptr(qv), ptr(qc),
                                       qw.shape[1], n_q, ptr(qk), ptr(qp), ptr(qn), ptr(qr), q_cap, ptr(nbr), nbr.shape[1], C.byref(params), cand_cap, ptr(cand),
                                       ptr(summary), ptr(words), ptr(score)))
        return cand, summary, words, score

    # ---- PnP RANSAC: a pose for every relocalisation candidate (the rule: include/sendslam_orb.h) ----
    # ---- undistorted keypoints and RGB-D depth ----
    def undistort_pairs_device(self, d_kp: int, d_n_kp: int, n_frames: int, rows_per_frame: int, cams, d_kp_out: int):
        """cams: one Camera (all frames) or n_frames of them; d_kp_out may equal d_kp"""
        arr, n = _cameras_array(cams)
        self._check(self._lib.ss_undistort_pairs_device(self._h, d_kp, d_n_kp, int(n_frames), int(rows_per_frame), arr, n, d_kp_out))

    def undistort_batch_device(self, cams=None, d_kp_out: int = 0):
        """cams None: the calibration set last; d_kp_out 0: in place (the raw pairs are saved first: batch_raw_xy)"""
        arr, n = _cameras_array(cams)
        self._check(self._lib.ss_undistort_batch_device(self._h, arr, n, d_kp_out or None))

    def batch_raw_xy(self) -> int:
        """the device address of the raw pairs the in-place undistortion saved, float32 [n_frames][kp_capacity][2]"""
        p = C.c_void_p()
        self._check(self._lib.ss_get_batch_raw_xy(self._h, C.byref(p)))
        return p.value

    def depth_pairs_device(self, params: DepthParams, d_depth: int, width: int, height: int, row_stride: int, frame_stride: int, d_kp_raw: int,
                           d_n_kp: int, n_frames: int, rows_per_frame: int, d_right: int, d_depth_out: int, d_summary: int, d_kp_un: int = 0):
        self._check(self._lib.ss_depth_pairs_device(self._h, C.byref(params), d_depth, int(width), int(height), int(row_stride), int(frame_stride), d_kp_raw,
                                                    d_kp_un or None, d_n_kp, int(n_frames), int(rows_per_frame), d_right, d_depth_out, d_summary))

    def depth_batch_device(self, params: DepthParams, d_depth: int, width: int, height: int, row_stride: int, frame_stride: int, d_right: int,
                           d_depth_out: int, d_summary: int):
        self._check(self._lib.ss_depth_batch_device(self._h, C.byref(params), d_depth, int(width), int(height), int(row_stride), int(frame_stride), d_right,
                                                    d_depth_out, d_summary))

    # ---- the stereo form of the triangulation ----
    def triangulate_stereo_pairs_device(self, d_q: int, d_q_kp: int, d_nq: int, d_t_kp: int, d_nt: int, d_idx: int, n_frames: int, rows_per_frame: int,
                                        pairs, rigs, planes, params: TriStereoParams, d_info: int, d_points: int, d_point_desc: int, d_point_rows: int,
                                        d_n_points: int, d_summary: int):
        """triangulate_pairs_device with planes = ((d_depth1, stride), (d_right1, stride), (d_depth2, stride), (d_right2, stride)) and
        rigs: n_frames TriStereoRig (host); d_info TRI_STEREO_INFO_DTYPE, d_summary TRI_STEREO_SUMMARY_DTYPE; asynchronous."""
        w, r = _pairs_array(pairs), _rigs_array(rigs)
        if len(w) != n_frames or len(r) != n_frames or len(planes) != 4:
            raise ValueError("one pair and one rig per pair of frames, four planes")
        flat = [int(v) for pl in planes for v in pl]
        self._check(self._lib.ss_triangulate_stereo_pairs_device(self._h, d_q, d_q_kp, d_nq, d_t_kp, d_nt, d_idx, int(n_frames), int(rows_per_frame),
                                                                 w.ctypes.data if n_frames else None, r.ctypes.data if n_frames else None, *flat,
                                                                 C.byref(params), d_info, d_points, d_point_desc, d_point_rows, d_n_points, d_summary))

    def triangulate_stereo_batch_device(self, d_idx: int, pairs, rigs, d_depth: int, depth_stride: int, d_right: int, right_stride: int,
                                        params: TriStereoParams, d_info: int, d_points: int, d_point_desc: int, d_point_rows: int, d_n_points: int,
                                        d_summary: int, train_src=None):
        """the same on the frames of the last batch, frame b against train_src[b] (None: b - 1); the planes are [n_frames][kp_capacity]"""
        w, r = _pairs_array(pairs), _rigs_array(rigs)
        n_frames = self.batch_view().n_frames
        if len(w) != n_frames or len(r) != n_frames:
            raise ValueError("one pair and one rig per frame of the batch")
        src = None if train_src is None else np.ascontiguousarray(train_src, np.int32)
        self._check(self._lib.ss_triangulate_stereo_batch_device(self._h, None if src is None else src.ctypes.data, d_idx, w.ctypes.data, r.ctypes.data,
                                                                 d_depth, int(depth_stride), d_right, int(right_stride), C.byref(params), d_info, d_points,
                                                                 d_point_desc, d_point_rows, d_n_points, d_summary))

    # ---- map points from depth: unprojection and the close-point rule (the rule: include/sendslam_orb.h) ----
    @staticmethod
    def _depth_blocks(depth_src, n_depth_blocks, n_frames):
        src = None if depth_src is None else np.ascontiguousarray(depth_src, np.int32).reshape(-1)
        if src is not None and len(src) != n_frames:
            raise ValueError("one depth_src entry per frame")
        if n_depth_blocks is None:
            n_depth_blocks = n_frames if src is None else max(int(src.max(initial=-1)) + 1, 1)
        return src, int(n_depth_blocks)

    def unproject_pairs_device(self, d_kp: int, d_desc: int, d_n_kp: int, d_depth: int, depth_stride: int, n_frames: int, rows_per_frame: int, views,
                               params: UnprojectParams, d_info: int, d_points: int, d_point_desc: int, d_point_rows: int, d_n_points: int,
                               d_summary: int, d_has_point: int = 0, d_outlier: int = 0, depth_src=None, n_depth_blocks=None):
        """views: n_frames UnprojectView (host).  d_depth: the depth of row 0 of block 0, depth_stride bytes to the next row (4: a
        float plane; 16 at &points[0].depth: STEREO_POINT_DTYPE in place); depth_src: host ints, frame b reads block depth_src[b] of
        n_depth_blocks (-1: the frame has no depth; None: block b).  d_info UNPROJECT_INFO_DTYPE [n_frames][rows_per_frame]; the
        compact d_points / d_point_desc / d_point_rows with d_n_points are the blocks match_proj_pairs_device reads; d_summary
        UNPROJECT_SUMMARY_DTYPE [n_frames]; asynchronous."""
        v = _unproject_views_array(views)
        if len(v) != n_frames:
            raise ValueError("one view per frame")
        src, blocks = self._depth_blocks(depth_src, n_depth_blocks, n_frames)
        self._check(self._lib.ss_unproject_pairs_device(self._h, d_kp, d_desc, d_n_kp, d_depth, int(depth_stride), blocks,
                                                        None if src is None else src.ctypes.data, d_has_point or None, d_outlier or None,
                                                        int(n_frames), int(rows_per_frame), v.ctypes.data if n_frames else None, C.byref(params), d_info,
                                                        d_points, d_point_desc, d_point_rows, d_n_points, d_summary))

    def unproject_batch_device(self, d_depth: int, depth_stride: int, views, params: UnprojectParams, d_info: int, d_points: int, d_point_desc: int,
                               d_point_rows: int, d_n_points: int, d_summary: int, d_has_point: int = 0, d_outlier: int = 0, depth_src=None,
                               n_depth_blocks=None):
        """the same on the frames of the last batch (rows_per_frame = kp_capacity); views: one per frame of the batch.  After
        stereo_batch_device: d_depth at the depth field of its points, depth_stride 16, depth_src [0, -1, 1, -1, ...]"""
        v = _unproject_views_array(views)
        n_frames = self.batch_view().n_frames  # OrbError SS_ERR_STATE without a batch
        if len(v) != n_frames:
            raise ValueError("one view per frame of the batch")
        src, blocks = self._depth_blocks(depth_src, n_depth_blocks, n_frames)
        self._check(self._lib.ss_unproject_batch_device(self._h, d_depth, int(depth_stride), blocks, None if src is None else src.ctypes.data,
                                                        d_has_point or None, d_outlier or None, v.ctypes.data,
                                                        C.byref(params), d_info, d_points, d_point_desc, d_point_rows, d_n_points, d_summary))

    def unproject(self, view: UnprojectView, params: UnprojectParams, kp, desc, depth, has_point=None, outlier=None):
        """ss_unproject: one frame in host memory, synchronous; the arguments and the result of unproject_host with n = the rows"""
        def call(n_, rows, k, de, d_at, stride, hp, ol, info, pts, pd, pr, n_pts, summary):
            rc = self._lib.ss_unproject(self._h, C.byref(view), C.byref(params), k, de, rows, d_at, stride, hp, ol, info, pts, pd, pr, n_pts, summary)
            self._check(rc)
            return rc
        return _unproject_one(call, "ss_unproject", kp, desc, depth, None, has_point, outlier)

    @staticmethod
    def _pnp_tables(views, kp_src, point_src, n_problems):
        v = _views_array(views)
        if len(v) != n_problems:
            raise ValueError("one view per problem")
        ks = None if kp_src is None else np.ascontiguousarray(kp_src, np.int32)
        ps = None if point_src is None else np.ascontiguousarray(point_src, np.int32)
        if (ks is not None and len(ks) != n_problems) or (ps is not None and len(ps) != n_problems):
            raise ValueError("one frame and block number per problem")
        return v, ks, ps

    def pnp_pairs_device(self, d_points: int, d_n_points: int, n_blocks: int, point_rows: int, d_kp: int, d_n_kp: int, n_kp_frames: int,
                         rows_per_frame: int, d_idx: int, n_problems: int, views, params: PnpParams, d_inlier: int, d_result: int, kp_src=None,
                         point_src=None, d_point_skip: int = 0):
        """n_problems problems on device arrays: map points [n_blocks][point_rows] (MAP_POINT_DTYPE, optional skip bytes, counts), keypoints
        KP_DTYPE [n_kp_frames][rows_per_frame] with counts, d_idx as match_bow_pairs_device wrote it; views one per problem, kp_src and
        point_src host tables or None (problem q reads frame q, block q); d_inlier uint8 [n_problems][rows_per_frame], d_result
        PNP_RESULT_DTYPE [n_problems]; asynchronous."""
        v, ks, ps = self._pnp_tables(views, kp_src, point_src, n_problems)
        self._check(self._lib.ss_pnp_pairs_device(self._h, C.c_void_p(d_points), C.c_void_p(d_point_skip), C.c_void_p(d_n_points), n_blocks,
                                                  point_rows, C.c_void_p(d_kp), C.c_void_p(d_n_kp), n_kp_frames, rows_per_frame, C.c_void_p(d_idx),
                                                  n_problems, v.ctypes.data if n_problems else None, None if ks is None else ks.ctypes.data,
                                                  None if ps is None else ps.ctypes.data, C.byref(params), C.c_void_p(d_inlier),
                                                  C.c_void_p(d_result)))

    def pnp_batch_device(self, d_points: int, d_n_points: int, n_blocks: int, point_rows: int, d_idx: int, n_problems: int, views,
                         params: PnpParams, d_inlier: int, d_result: int, kp_src=None, point_src=None, d_point_skip: int = 0):
        """the same, the keypoints being the frames of the last batch (rows_per_frame = kp_capacity); asynchronous."""
        v, ks, ps = self._pnp_tables(views, kp_src, point_src, n_problems)
        self._check(self._lib.ss_pnp_batch_device(self._h, C.c_void_p(d_points), C.c_void_p(d_point_skip), C.c_void_p(d_n_points), n_blocks,
                                                  point_rows, C.c_void_p(d_idx), n_problems, v.ctypes.data if n_problems else None,
                                                  None if ks is None else ks.ctypes.data, None if ps is None else ps.ctypes.data,
                                                  C.byref(params), C.c_void_p(d_inlier), C.c_void_p(d_result)))

    def pnp(self, view, points: np.ndarray, kp: np.ndarray, idx: np.ndarray, params: PnpParams, skip=None):
        """One problem, host arrays in and out -> (uint8 inlier flag per keypoint row, PNP_RESULT_DTYPE record)."""
        v, pts, k, ix, skip, n_p, n_k = _pnp_arrays(view, points, kp, idx, skip)
        inlier, res = np.empty(n_k, np.uint8), np.zeros(1, PNP_RESULT_DTYPE)
        ptr = lambda a, n: None if a is None or not n else a.ctypes.data  # noqa: E731
        self._check(self._lib.ss_pnp(self._h, v.ctypes.data, ptr(pts, n_p), ptr(skip, n_p), n_p, ptr(k, n_k), n_k, ptr(ix, n_k), C.byref(params),
                                     ptr(inlier, n_k), res.ctypes.data))
        return inlier, res[0]

    # ---- two-view initialisation: a pose and points from two frames' matches (the rule: include/sendslam_orb.h) ----
    def two_view_pairs_device(self, d_kp1: int, d_n_kp1: int, n_frames1: int, d_kp2: int, d_n_kp2: int, n_frames2: int, rows_per_frame: int,
                              d_idx: int, n_problems: int, views, params: TwoViewParams, d_flag: int, d_points: int, d_point_rows: int,
                              d_n_points: int, d_result: int, kp1_src=None, kp2_src=None):
        """n_problems problems on device arrays: keypoints KP_DTYPE [n_frames][rows_per_frame] with counts on both sides, d_idx as
        match_guided_pairs_device wrote it; views one per problem, kp1_src and kp2_src host tables or None (problem q reads frame q); d_flag
        uint8 [n_problems][rows_per_frame], d_points MAP_POINT_DTYPE and d_point_rows int32 x 2 of the same shape, d_n_points int32
        [n_problems], d_result TWO_VIEW_RESULT_DTYPE [n_problems]; asynchronous."""
        v = _views_array(views)
        s1 = None if kp1_src is None else np.ascontiguousarray(kp1_src, np.int32)
        s2 = None if kp2_src is None else np.ascontiguousarray(kp2_src, np.int32)
        if len(v) != n_problems or (s1 is not None and len(s1) != n_problems) or (s2 is not None and len(s2) != n_problems):
            raise ValueError("one view and one frame number of each side per problem")
        self._check(self._lib.ss_two_view_pairs_device(self._h, C.c_void_p(d_kp1), C.c_void_p(d_n_kp1), n_frames1, C.c_void_p(d_kp2),
                                                       C.c_void_p(d_n_kp2), n_frames2, rows_per_frame, C.c_void_p(d_idx), n_problems,
                                                       v.ctypes.data if n_problems else None, None if s1 is None else s1.ctypes.data,
                                                       None if s2 is None else s2.ctypes.data, C.byref(params), C.c_void_p(d_flag),
                                                       C.c_void_p(d_points), C.c_void_p(d_point_rows), C.c_void_p(d_n_points), C.c_void_p(d_result)))

    def two_view_batch_device(self, d_idx: int, n_problems: int, views, params: TwoViewParams, d_flag: int, d_points: int, d_point_rows: int,
                              d_n_points: int, d_result: int, train_src=None):
        """the same, frame q of the last batch against frame train_src[q] of it (None: q - 1; -1: none); asynchronous."""
        v = _views_array(views)
        ts = None if train_src is None else np.ascontiguousarray(train_src, np.int32)
        if len(v) != n_problems or (ts is not None and len(ts) != n_problems):
            raise ValueError("one view and one train frame per problem")
        self._check(self._lib.ss_two_view_batch_device(self._h, None if ts is None else ts.ctypes.data, C.c_void_p(d_idx), n_problems,
                                                       v.ctypes.data if n_problems else None, C.byref(params), C.c_void_p(d_flag),
                                                       C.c_void_p(d_points), C.c_void_p(d_point_rows), C.c_void_p(d_n_points), C.c_void_p(d_result)))

    def two_view(self, view, kp1: np.ndarray, kp2: np.ndarray, idx: np.ndarray, params: TwoViewParams):
        """One problem, host arrays in and out -> what two_view_host returns."""
        v, k1, k2, ix, n1, n2 = _two_view_arrays(view, kp1, kp2, idx)
        flag, pts, rows, n_pts, res = _two_view_outputs(n1)
        ptr = lambda a, n: a.ctypes.data if n else None  # noqa: E731
        self._check(self._lib.ss_two_view(self._h, v.ctypes.data, ptr(k1, n1), n1, ptr(k2, n2), n2, ptr(ix, n1), C.byref(params), ptr(flag, n1),
                                          ptr(pts, n1), ptr(rows, n1), n_pts.ctypes.data, res.ctypes.data))
        return flag, pts[:n_pts[0]], rows[:n_pts[0]], res[0]

    # ---- Sim3 refinement: SearchBySim3's bookkeeping and OptimizeSim3 per loop candidate (the rule: include/sendslam_orb.h) ----
    def sim3_opt_pairs_device(self, d_query_xyz: int, d_query_kp: int, d_n_query: int, d_train_xyz: int, d_train_kp: int, d_n_train: int,
                              d_idx: int, n_pairs: int, rows: int, views1, views2, d_start: int, params: Sim3OptParams, d_flags: int,
                              d_result: int, d_query_skip: int = 0, d_train_skip: int = 0):
        """n_pairs pairs on device arrays as for sim3_pairs_device; d_start SIM3_RESULT_DTYPE [n_pairs] on the device (sim3_pairs_device's
        d_result); d_flags uint8 [n_pairs][rows] by query row, d_result SIM3_OPT_RESULT_DTYPE [n_pairs]; asynchronous."""
        v1, v2 = _views_array(views1), _views_array(views2)
        if len(v1) != n_pairs or len(v2) != n_pairs:
            raise ValueError("one view of either keyframe per pair")
        self._check(self._lib.ss_sim3_opt_pairs_device(self._h, C.c_void_p(d_query_xyz), C.c_void_p(d_query_kp), C.c_void_p(d_query_skip),
                                                       C.c_void_p(d_n_query), C.c_void_p(d_train_xyz), C.c_void_p(d_train_kp),
                                                       C.c_void_p(d_train_skip), C.c_void_p(d_n_train), C.c_void_p(d_idx), n_pairs, rows,
                                                       v1.ctypes.data if n_pairs else None, v2.ctypes.data if n_pairs else None,
                                                       C.c_void_p(d_start), C.byref(params), C.c_void_p(d_flags), C.c_void_p(d_result)))

    def sim3_opt_batch_device(self, d_xyz: int, d_idx: int, views, d_start: int, params: Sim3OptParams, d_flags: int, d_result: int,
                              train_src=None, d_skip: int = 0):
        """the same on the frames of the last batch, frame b against train_src[b] (None: b - 1); asynchronous."""
        v = _views_array(views)
        src = None if train_src is None else np.ascontiguousarray(train_src, np.int32)
        self._check(self._lib.ss_sim3_opt_batch_device(self._h, None if src is None else src.ctypes.data, C.c_void_p(d_xyz), C.c_void_p(d_skip),
                                                       C.c_void_p(d_idx), v.ctypes.data, C.c_void_p(d_start), C.byref(params),
                                                       C.c_void_p(d_flags), C.c_void_p(d_result)))

    def sim3_opt(self, view1, q_xyz, q_kp, view2, t_xyz, t_kp, idx, start, params: Sim3OptParams, q_skip=None, t_skip=None):
        """One pair, host arrays in and out -> (uint8 flag per query row, SIM3_OPT_RESULT_DTYPE record)."""
        v1, v2, qx, qk, tx, tk, ix, st, q_skip, t_skip, nq, nt = _sim3_pair_arrays(view1, q_xyz, q_kp, view2, t_xyz, t_kp, idx, start, q_skip, t_skip)
        flags, res = np.empty(nq, np.uint8), np.zeros(1, SIM3_OPT_RESULT_DTYPE)
        ptr = lambda a, n: None if a is None or not n else a.ctypes.data  # noqa: E731
        self._check(self._lib.ss_sim3_opt(self._h, v1.ctypes.data, ptr(qx, nq), ptr(qk, nq), ptr(q_skip, nq), nq, v2.ctypes.data, ptr(tx, nt),
                                          ptr(tk, nt), ptr(t_skip, nt), nt, ptr(ix, nq), st.ctypes.data, C.byref(params), ptr(flags, nq),
                                          res.ctypes.data))
        return flags, res[0]

    def sim3_marks_pairs_device(self, d_idx: int, d_n_query: int, d_n_train: int, n_pairs: int, rows: int, d_skip1_out: int, d_skip2_out: int,
                                d_query_skip: int = 0, d_train_skip: int = 0):
        """the skip bytes of SearchBySim3's two searches, uint8 [n_pairs][rows] each; asynchronous."""
        self._check(self._lib.ss_sim3_marks_pairs_device(self._h, C.c_void_p(d_idx), C.c_void_p(d_query_skip), C.c_void_p(d_train_skip),
                                                         C.c_void_p(d_n_query), C.c_void_p(d_n_train), n_pairs, rows, C.c_void_p(d_skip1_out),
                                                         C.c_void_p(d_skip2_out)))

    def sim3_mutual_pairs_device(self, d_idx: int, d_idx12: int, d_idx21: int, d_n_query: int, d_n_train: int, n_pairs: int, rows: int,
                                 d_idx_out: int, d_summary: int):
        """the agreement test of the two searches: d_idx_out int32 [n_pairs][rows], d_summary SIM3_MUTUAL_DTYPE [n_pairs]; asynchronous."""
        self._check(self._lib.ss_sim3_mutual_pairs_device(self._h, C.c_void_p(d_idx), C.c_void_p(d_idx12), C.c_void_p(d_idx21), C.c_void_p(d_n_query),
                                                          C.c_void_p(d_n_train), n_pairs, rows, C.c_void_p(d_idx_out), C.c_void_p(d_summary)))

    def sim3_marks_batch_device(self, d_idx: int, d_skip1_out: int, d_skip2_out: int, train_src=None, d_skip: int = 0):
        """sim3_marks_pairs_device on the frames of the last batch; asynchronous."""
        src = None if train_src is None else np.ascontiguousarray(train_src, np.int32)
        self._check(self._lib.ss_sim3_marks_batch_device(self._h, None if src is None else src.ctypes.data, C.c_void_p(d_idx), C.c_void_p(d_skip),
                                                         C.c_void_p(d_skip1_out), C.c_void_p(d_skip2_out)))

    def sim3_mutual_batch_device(self, d_idx: int, d_idx12: int, d_idx21: int, d_idx_out: int, d_summary: int, train_src=None):
        """sim3_mutual_pairs_device on the frames of the last batch; asynchronous."""
        src = None if train_src is None else np.ascontiguousarray(train_src, np.int32)
        self._check(self._lib.ss_sim3_mutual_batch_device(self._h, None if src is None else src.ctypes.data, C.c_void_p(d_idx), C.c_void_p(d_idx12),
                                                          C.c_void_p(d_idx21), C.c_void_p(d_idx_out), C.c_void_p(d_summary)))

    def wait_stream(self, hip_stream: int):
        """Orders this context's stream after everything enqueued so far on another stream of the device."""
        self._check(self._lib.ss_wait_stream(self._h, C.c_void_p(hip_stream)))

    def synchronize(self):
        self._check(self._lib.ss_synchronize(self._h))

    def stream(self) -> int:
        s = C.c_void_p()
        self._check(self._lib.ss_get_stream(self._h, C.byref(s)))
        return s.value or 0

    def profile(self, on: bool):
        self._check(self._lib.ss_profile_enable(self._h, int(on)))

    def profile_reset(self):
        self._check(self._lib.ss_profile_reset(self._h))

    def stats(self):
        arr = (StageStats * 32)()
        n = self._check(self._lib.ss_stats(self._h, arr, 32))
        return [dict(name=arr[i].name.decode(), launches=arr[i].launches, total_ms=arr[i].total_ms,
                     mean_ms=arr[i].mean_ms, median_ms=arr[i].median_ms,
                     algorithmic_bytes=arr[i].algorithmic_bytes) for i in range(min(n, 32))]

    def debug_fetch(self, what: int, frame: int, level: int, shape, dtype=np.uint8) -> np.ndarray:
        out = np.empty(shape, dtype)
        n = self._check(self._lib.ss_debug_fetch(self._h, what, frame, level, out.ctypes.data, out.nbytes))
        return out.reshape(-1)[: n // out.itemsize]


class Exchange:
    """ss_xchg_*: the C ABI's own all-gather / broadcast between the ranks of one node (one process per GPU): every rank
    stores its block straight into every peer's IPC-mapped slab and raises a flag there.  Creation and destruction are
    collective; every rank issues the same sequence of messages; consumers of a gathered block are enqueued on the same
    context's stream."""

    def __init__(self, device: int, rank: int, world: int, max_bytes: int, rendezvous: str, timeout_ms: int = 0):
        self._lib = load()
        h = C.c_void_p()
        rc = self._lib.ss_xchg_create(int(device), int(rank), int(world), int(max_bytes), rendezvous.encode(), int(timeout_ms), C.byref(h))
        if rc != SS_OK:
            raise OrbError(rc, (self._lib.ss_xchg_last_error(None) or b"").decode())
        self._h = h
        self.rank, self.world = rank, world

    def _check(self, rc: int):
        if rc < 0:
            raise OrbError(rc, (self._lib.ss_xchg_last_error(self._h) or b"").decode())
        return rc

    def allgather(self, ctx: "OrbContext", segments):
        """segments: [(device pointer, bytes), ...] (<= 4), the same sizes on every rank.  Returns (base, stride): rank r's
        block is at base + r * stride in LOCAL device memory, the segments back to back (each padded to 16 bytes); valid
        until the second-next message."""
        n = len(segments)
        ptrs = (C.c_void_p * n)(*[C.c_void_p(p) for p, _ in segments])
        sizes = (C.c_int64 * n)(*[int(b) for _, b in segments])
        base, stride = C.c_void_p(), C.c_int64()
        self._check(self._lib.ss_xchg_allgather(self._h, ctx._h, ptrs, sizes, n, C.byref(base), C.byref(stride)))
        return base.value, stride.value

    def stereo_match(self, ctx: "OrbContext", peer: int, kp_capacity: int, th: int = 50, ratio_num: int = 9, ratio_den: int = 10):
        """ss_stereo_exchange_match: the frame ctx extracted last against the peer rank's -> (idx, d1, d2 over this eye's
        keypoints, peer's keypoint count)"""
        idx = np.empty(kp_capacity, np.int32)
        d1 = np.empty(kp_capacity, np.uint16)
        d2 = np.empty(kp_capacity, np.uint16)
        n_own, n_peer = C.c_int32(), C.c_int32()
        rc = self._lib.ss_stereo_exchange_match(ctx._h, self._h, int(peer), th, ratio_num, ratio_den, idx.ctypes.data, d1.ctypes.data,
                                                d2.ctypes.data, C.byref(n_own), C.byref(n_peer))
        if rc < 0:
            raise OrbError(rc, (self._lib.ss_last_error(ctx._h) or b"").decode())
        n = n_own.value
        return idx[:n], d1[:n], d2[:n], n_peer.value

    def broadcast(self, ctx: "OrbContext", root: int, d_buf: int, nbytes: int):
        self._check(self._lib.ss_xchg_broadcast(self._h, ctx._h, int(root), C.c_void_p(d_buf), int(nbytes)))

    def status(self):
        """raises if a peer's message did not arrive in time (valid once the stream has been synchronised)"""
        self._check(self._lib.ss_xchg_status(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ss_xchg_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Pipe:
    """ss_pipe_*: ring of pinned slots; host frames in, host keypoints / descriptors / matches out, copies and
    kernels of different batches overlapped.  Arrays of a result are views of the slot's pinned memory: valid until
    release(slot)."""

    def __init__(self, device: int, width: int, height: int, channels: int = 1, batch: int = 64, depth: int = 4,
                 match_mode: int = 0, copy_threads: int = 0, cam: Optional[Camera] = None, match_th: int = 0, ratio_num: int = 0,
                 ratio_den: int = 0, **params):
        self._lib = load()
        self.params = default_params(**params)
        self.cfg = PipeConfig(width=width, height=height, channels=channels, batch=batch, depth=depth,
                              match_mode=match_mode, match_th=match_th, ratio_num=ratio_num, ratio_den=ratio_den, copy_threads=copy_threads)
        h = C.c_void_p()
        rc = self._lib.ss_pipe_create(int(device), C.byref(self.params), C.byref(cam) if cam is not None else None,
                                      C.byref(self.cfg), C.byref(h))
        if rc != SS_OK:
            raise OrbError(rc, (self._lib.ss_pipe_last_error(None) or b"").decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ss_pipe_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int):
        if rc < 0:
            raise OrbError(rc, (self._lib.ss_pipe_last_error(self._h) or b"").decode())
        return rc

    def acquire(self):
        """-> (slot id, uint8 view [batch, height, row_stride] of the slot's pinned pixels) or None when busy"""
        sl = PipeSlot()
        rc = self._lib.ss_pipe_acquire(self._h, C.byref(sl))
        if rc == SS_ERR_BUSY:
            return None
        self._check(rc)
        n = self.cfg.batch * sl.frame_stride
        buf = (C.c_uint8 * n).from_address(sl.pixels)
        return sl.slot, np.frombuffer(buf, np.uint8).reshape(self.cfg.batch, self.cfg.height, sl.row_stride)

    def submit(self, slot: int, n_frames: int, camera_ids=None, timestamps=None):
        ci = None if camera_ids is None else np.ascontiguousarray(camera_ids, np.int32)
        ts = None if timestamps is None else np.ascontiguousarray(timestamps, np.float64)
        self._check(self._lib.ss_pipe_submit(self._h, slot, n_frames, None if ci is None else ci.ctypes.data,
                                             None if ts is None else ts.ctypes.data))

    def submit_frames(self, frames, camera_ids=None, timestamps=None, row_stride: Optional[int] = None) -> bool:
        """frames: sequence of uint8 arrays of the pipe's shape (None = a bad frame).  False when no slot is free."""
        keep = [None if f is None else np.ascontiguousarray(f, np.uint8) for f in frames]
        rs = self.cfg.width * self.cfg.channels if row_stride is None else row_stride
        need = (self.cfg.height - 1) * rs + self.cfg.width * self.cfg.channels  # what the library's copy threads read per frame
        for i, f in enumerate(keep):
            if f is not None and f.size < need:
                raise ValueError(f"frame {i}: {f.size} bytes, the pipe's shape needs {need} (height {self.cfg.height}, row stride {rs})")
        ptrs = (C.c_void_p * len(keep))(*[None if f is None else f.ctypes.data for f in keep])
        ci = None if camera_ids is None else np.ascontiguousarray(camera_ids, np.int32)
        ts = None if timestamps is None else np.ascontiguousarray(timestamps, np.float64)
        rc = self._lib.ss_pipe_submit_frames(self._h, ptrs, len(keep), rs, None if ci is None else ci.ctypes.data,
                                             None if ts is None else ts.ctypes.data)
        if rc == SS_ERR_BUSY:
            return False
        self._check(rc)
        return True

    def submit_batch_array(self, batch: np.ndarray, camera_ids=None, timestamps=None) -> bool:
        """batch: one contiguous uint8 array [n, height, width(, channels)]: frame pointers without per-frame Python work"""
        assert batch.dtype == np.uint8 and batch.flags.c_contiguous
        want = (self.cfg.height, self.cfg.width) if self.cfg.channels == 1 and batch.ndim == 3 else (self.cfg.height, self.cfg.width, self.cfg.channels)
        if tuple(batch.shape[1:]) != want:
            raise ValueError(f"batch frames have shape {tuple(batch.shape[1:])}, the pipe's shape is {want}")
        n = batch.shape[0]
        fs = batch.strides[0]
        base = batch.ctypes.data
        ptrs = (C.c_void_p * n)(*[base + i * fs for i in range(n)])
        ci = None if camera_ids is None else np.ascontiguousarray(camera_ids, np.int32)
        ts = None if timestamps is None else np.ascontiguousarray(timestamps, np.float64)
        rc = self._lib.ss_pipe_submit_frames(self._h, ptrs, n, self.cfg.width * self.cfg.channels,
                                             None if ci is None else ci.ctypes.data, None if ts is None else ts.ctypes.data)
        if rc == SS_ERR_BUSY:
            return False
        self._check(rc)
        return True

    def _result(self, r: PipeResult) -> dict:
        n, k = r.n_frames, r.kp_capacity

        def view(ptr, dtype, shape):
            if not ptr:
                return None
            nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
            return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype).reshape(shape)
        return {"slot": r.slot, "n_frames": n, "kp_capacity": k, "sequence": r.sequence,
                "status": view(r.status, np.int32, (n,)), "camera_id": view(r.camera_id, np.int32, (n,)),
                "timestamp": view(r.timestamp, np.float64, (n,)), "n_keypoints": view(r.n_keypoints, np.int32, (n,)),
                "level_counts": view(r.level_counts, np.int32, (n, SS_MAX_LEVELS)),
                "keypoints": view(r.keypoints, KP_DTYPE, (n, k)), "descriptors": view(r.descriptors, np.uint8, (n, k, 32)),
                "match_idx": view(r.match_idx, np.int32, (n, k)), "match_d1": view(r.match_d1, np.uint16, (n, k)),
                "match_d2": view(r.match_d2, np.uint16, (n, k)), "d_descriptors": r.d_descriptors, **self._sources(r)}

    def _sources(self, r: PipeResult) -> dict:
        """match_mode 2: which frame each frame was matched against, (sequence, index in its batch) or -1 -1"""
        if self.cfg.match_mode != 2:
            return {}
        seq, frame = np.empty(r.n_frames, np.int64), np.empty(r.n_frames, np.int32)
        self._check(self._lib.ss_pipe_match_sources(self._h, r.slot, seq.ctypes.data, frame.ctypes.data))
        return {"train_sequence": seq, "train_frame": frame}

    def wait(self) -> dict:
        r = PipeResult()
        self._check(self._lib.ss_pipe_wait(self._h, C.byref(r)))
        return self._result(r)

    def poll(self) -> Optional[dict]:
        r = PipeResult()
        rc = self._check(self._lib.ss_pipe_poll(self._h, C.byref(r)))
        return self._result(r) if rc == 1 else None

    def release(self, slot: int):
        self._check(self._lib.ss_pipe_release(self._h, slot))

    def debug_inject_failure(self, after_operations: int):
        """test hook: the next submission fails after that many of its enqueues"""
        self._check(self._lib.ss_pipe_debug_inject_failure(self._h, int(after_operations)))

    def in_flight(self) -> int:
        return self._check(self._lib.ss_pipe_in_flight(self._h))


def _debug_sort(self, size, ulx):
    """Permutation (ids) the device's std::sort restatement leaves for compareNodes keys."""
    n = len(size)
    items = (np.asarray(size, np.uint64) << np.uint64(32)) | (np.asarray(ulx, np.uint64) << np.uint64(20)) | np.arange(n, dtype=np.uint64)
    items = np.ascontiguousarray(items)
    self._check(self._lib.ss_debug_sort(self._h, items.ctypes.data, n))
    return (items & np.uint64(0xFFFFF)).astype(np.int32)


OrbContext.debug_sort = _debug_sort
