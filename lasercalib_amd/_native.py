"""ctypes binding of libsba_hip.so (C ABI declared in include/sba_hip.h).

There is NO CPU fallback: if the shared library is missing, or no gfx950 GPU is
visible, every compute entry point raises.  The library is built in-tree by
``__graft_entry__.build()`` / ``make -C lasercalib_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsba_hip.so")

SBA_F64, SBA_F32 = 0, 1
CAM_RADIAL, CAM_RADIAL_TANGENTIAL = 0, 1        # sba_cam_model: 11 / 13 parameters per camera
LOSS_LINEAR, LOSS_HUBER, LOSS_SOFT_L1, LOSS_CAUCHY = 0, 1, 2, 3      # sba_loss
MODE_FULL, MODE_POINTS_ONLY, MODE_SHARED_INTR, MODE_CAMS_ONLY_SQ, MODE_TRANSFORM_SQ = 0, 1, 2, 3, 4
NSCALARS = 8

# every symbol include/sba_hip.h declares (tests/test_cabi_symbols.py checks the .so exports all of them)
EXPORTED_SYMBOLS = (
    "sba_abi_version", "sba_device_count", "sba_last_error", "sba_rotate", "sba_project", "sba_project_model",
    "sba_create", "sba_upload", "sba_upload_ex", "sba_get_upload_report", "sba_get_layout", "sba_set_params", "sba_get_params", "sba_destroy",
    "sba_get_gradient", "sba_get_transform", "sba_lm_get_step", "sba_ipc_export", "sba_ipc_attach", "sba_residual", "sba_residual_jacobian", "sba_solve_lm",
    "sba_lm_exchange_size", "sba_lm_begin", "sba_lm_linearize", "sba_lm_form_reduced",
    "sba_lm_solve_trial", "sba_lm_decide", "sba_lm_decide_async", "sba_lm_poll", "sba_lm_run", "sba_lm_finish", "sba_lm_get_log", "sba_time_kernel", "sba_get_kernel_profile",
    "sba_comm_get_unique_id", "sba_comm_init", "sba_set_fixed_points", "sba_set_robust_loss", "sba_covariance",
    "sba_triangulate", "sba_align", "sba_apply_similarity", "sba_reproj_stats",
    "sba_unproject_rows", "sba_unproject", "sba_detect_dots", "sba_detect_blobs",
    "sba_undistort_frames", "sba_background_accumulate", "sba_background_suppress", "sba_convert_frames", "sba_resize_frames",
    "sba_frames_to_yuv", "sba_undistort_yuv", "sba_frame_histograms", "sba_warp_frames",
    "sba_refine_corners", "sba_adaptive_threshold",
)


class SbaError(RuntimeError):
    """A libsba_hip call returned a negative status."""


class ProblemDesc(C.Structure):
    _fields_ = [("n_cams", C.c_int32), ("n_points", C.c_int32), ("n_obs", C.c_int64),
                ("dtype", C.c_int32), ("device", C.c_int32), ("stream", C.c_void_p),
                ("use_stream", C.c_int32), ("cam_model", C.c_int32), ("reserved", C.c_int32 * 2)]


class LmOpts(C.Structure):
    _fields_ = [("ftol", C.c_double), ("xtol", C.c_double), ("gtol", C.c_double),
                ("max_nfev", C.c_int64), ("mode", C.c_int32), ("verbose", C.c_int32),
                ("max_iter", C.c_int32), ("always_relinearize", C.c_int32),
                ("lambda0", C.c_double), ("reserved", C.c_int32 * 4)]


class LmReport(C.Structure):
    _fields_ = [("cost", C.c_double), ("initial_cost", C.c_double), ("optimality", C.c_double),
                ("step_norm", C.c_double), ("lambda_", C.c_double), ("nfev", C.c_int64),
                ("njev", C.c_int64), ("iterations", C.c_int32), ("accepted", C.c_int32),
                ("status", C.c_int32), ("reserved", C.c_int32), ("seconds_total", C.c_double),
                ("seconds_device", C.c_double)]


class LmIterLog(C.Structure):
    _fields_ = [("iteration", C.c_int32), ("accepted", C.c_int32), ("nfev", C.c_int64),
                ("cost", C.c_double), ("cost_reduction", C.c_double), ("step_norm", C.c_double),
                ("optimality", C.c_double), ("lambda_", C.c_double), ("rho", C.c_double)]


class CovOpts(C.Structure):
    _fields_ = [("cams_fixed", C.c_int32), ("scale", C.c_int32), ("reserved", C.c_int32 * 6)]


class CovReport(C.Structure):
    _fields_ = [("sigma2", C.c_double), ("dof", C.c_int64), ("gauge_rank", C.c_int32), ("n_points_degenerate", C.c_int32),
                ("info", C.c_int32), ("n_points_anchored", C.c_int32), ("gauge_residual", C.c_double),
                ("seconds_device", C.c_double), ("seconds_form", C.c_double), ("seconds_inverse", C.c_double),
                ("seconds_points", C.c_double), ("seconds_total", C.c_double)]


class TriOpts(C.Structure):
    _fields_ = [("min_views", C.c_int32), ("max_drop", C.c_int32), ("trim_px", C.c_double), ("write_back", C.c_int32),
                ("reserved", C.c_int32 * 5)]


class TriReport(C.Structure):
    _fields_ = [("n_ok", C.c_int64), ("n_anchored", C.c_int64), ("n_too_few", C.c_int64), ("n_degenerate", C.c_int64),
                ("n_behind", C.c_int64), ("n_obs_unusable", C.c_int64), ("n_obs_trimmed", C.c_int64),
                ("n_points_trimmed", C.c_int64), ("seconds_device", C.c_double), ("seconds_linear", C.c_double),
                ("seconds_trim", C.c_double), ("seconds_total", C.c_double)]


TRI_OK, TRI_ANCHORED, TRI_TOO_FEW, TRI_DEGENERATE, TRI_BEHIND = 0, 1, 2, 3, 4       # sba_tri_status


class UnpOpts(C.Structure):
    _fields_ = [("use_ref_cam", C.c_int32), ("ref_cam", C.c_int32), ("min_views", C.c_int32), ("write_back", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class UnpReport(C.Structure):
    _fields_ = [("n_ok", C.c_int64), ("n_anchored", C.c_int64), ("n_no_view", C.c_int64), ("n_degenerate", C.c_int64),
                ("n_behind", C.c_int64), ("n_obs_unusable", C.c_int64), ("n_obs_used", C.c_int64),
                ("seconds_device", C.c_double), ("seconds_total", C.c_double)]


UNP_OK, UNP_ANCHORED, UNP_NO_VIEW, UNP_DEGENERATE, UNP_BEHIND = 0, 1, 2, 3, 4       # sba_unp_status
UNP_ROW_OK, UNP_ROW_UNUSABLE, UNP_ROW_PARALLEL, UNP_ROW_BEHIND = 0, 1, 2, 3        # sba_unp_row_status


class DotOpts(C.Structure):
    _fields_ = [("channel", C.c_int32), ("threshold", C.c_int32), ("frames_on_device", C.c_int32), ("min_area", C.c_int32),
                ("max_area", C.c_int32), ("max_extent", C.c_int32), ("roi_rect", C.c_int32 * 4), ("roi_circle", C.c_int32 * 3),
                ("chunk_frames", C.c_int32), ("reserved", C.c_int32 * 2)]


DOT_OK, DOT_NONE, DOT_TOO_SMALL, DOT_TOO_LARGE, DOT_SPREAD = 0, 1, 2, 3, 4       # sba_dot_status
DOT_MAX_DIM = 16384


class HistOpts(C.Structure):
    _fields_ = [("channel", C.c_int32), ("frames_on_device", C.c_int32), ("roi_rect", C.c_int32 * 4), ("roi_circle", C.c_int32 * 3),
                ("chunk_frames", C.c_int32), ("reserved", C.c_int32 * 4)]


class CornerOpts(C.Structure):                                            # sba_corner_opts
    _fields_ = [("eps", C.c_double), ("frames_on_device", C.c_int32), ("chunk_frames", C.c_int32), ("channel", C.c_int32),
                ("gray_w", C.c_int32 * 3), ("win_x", C.c_int32), ("win_y", C.c_int32), ("zero_x", C.c_int32), ("zero_y", C.c_int32),
                ("max_iter", C.c_int32), ("reserved", C.c_int32 * 5)]


class AdaptiveOpts(C.Structure):                                          # sba_adaptive_opts
    _fields_ = [("n_windows", C.c_int32), ("block", C.c_int32 * 4), ("delta", C.c_int32 * 4), ("invert", C.c_int32),
                ("max_value", C.c_int32), ("channel", C.c_int32), ("gray_w", C.c_int32 * 3), ("frames_on_device", C.c_int32),
                ("out_on_device", C.c_int32), ("chunk_frames", C.c_int32), ("reserved", C.c_int32 * 4)]


ADAPTIVE_MAX_WINDOWS, ADAPTIVE_MAX_BLOCK, ADAPTIVE_MAX_DELTA = 4, 127, 256
# the columns a wave reads in one step and the tile of a workgroup (csrc/sba_adaptive.hpp: AT_STEP, at_tile), for the tests that
# straddle them
ADAPTIVE_STEP = 256


def adaptive_tile(max_block):
    """(columns, rows, row segments) of the tile a workgroup takes when ``max_block`` is the largest window of the call."""
    R = int(max_block) // 2
    L = (R + 1 + 3) // 4 * 4
    if R <= 48:
        return (ADAPTIVE_STEP - L - R) // 4 * 4, 64 if R <= 32 else 32, 1
    tw = 128 if (32 + 2 * R) * ((128 + L + R + 3) // 4 * 4) <= 32768 else 64
    return tw, 32, 256 // tw


# sba_corner_status bits
CORNER_CONVERGED, CORNER_MAX_ITER, CORNER_SINGULAR, CORNER_LEFT_IMAGE, CORNER_RESTORED, CORNER_INVALID = 1, 2, 4, 8, 16, 32
CORNER_MAX_WIN, CORNER_MAX_ITERATIONS = 15, 10000


class BlobOpts(C.Structure):
    _fields_ = [("channel", C.c_int32), ("threshold", C.c_int32), ("frames_on_device", C.c_int32), ("dilate_radius", C.c_int32),
                ("close_radius", C.c_int32), ("max_blobs", C.c_int32), ("min_area", C.c_int32), ("max_area", C.c_int32),
                ("centre_x", C.c_int32), ("centre_y", C.c_int32), ("max_centre_dist", C.c_int32), ("roi_rect", C.c_int32 * 4),
                ("roi_circle", C.c_int32 * 3), ("chunk_frames", C.c_int32), ("reserved", C.c_int32 * 5)]


BLOB_OK, BLOB_NONE, BLOB_OVERFLOW, BLOB_REJECTED, BLOB_MULTIPLE = 0, 1, 2, 3, 4       # sba_blob_status
BLOB_NREC, BLOB_DEFAULT_BLOBS, BLOB_MAX_BLOBS, BLOB_MAX_RADIUS = 12, 8, 64, 8
# geometry of the kernels (csrc/sba_blobs.hpp), for the tests that straddle it: rows of a morphology band, rows of a labelling
# tile (a tile is one 64-pixel word wide), words of a morphology band
BLOB_MORPH_ROWS, BLOB_TILE_ROWS, BLOB_MORPH_WORDS = 32, 32, 8


class LensStruct(C.Structure):                                            # sba_lens
    _fields_ = [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]


class UndistortOpts(C.Structure):
    _fields_ = [("frames_on_device", C.c_int32), ("out_on_device", C.c_int32), ("interpolation", C.c_int32),
                ("border_value", C.c_int32), ("chunk_frames", C.c_int32), ("reserved", C.c_int32 * 7)]


UNDIST_OUTSIDE, UNDIST_FOLDED, UNDIST_RANGE = 1, 2, 4                       # sba_undistort_flag
WARP_BEHIND = 8                                                            # sba_undistort_flag, set by sba_warp_frames only
UNDIST_INTERPOLATION = {"linear": 0, "nearest": 1}                         # sba_undistort_opts.interpolation
# the tile of destination pixels one workgroup owns (csrc/sba_undistort.hpp), for the tests that straddle it
UNDIST_TILE_ROWS, UNDIST_TILE_COLS = 4, 256


class BgAccumulateOpts(C.Structure):                                      # sba_background_accumulate_opts
    _fields_ = [("channel", C.c_int32), ("threshold", C.c_int32), ("frames_on_device", C.c_int32), ("stats_on_device", C.c_int32),
                ("accumulate", C.c_int32), ("chunk_frames", C.c_int32), ("reserved", C.c_int32 * 6)]


class BgSuppressOpts(C.Structure):                                        # sba_background_suppress_opts
    _fields_ = [("channel", C.c_int32), ("frames_on_device", C.c_int32), ("model_on_device", C.c_int32), ("out_on_device", C.c_int32),
                ("mode", C.c_int32), ("chunk_frames", C.c_int32), ("reserved", C.c_int32 * 6)]


BG_MODES = {"gate": 0, "subtract": 1}                                      # sba_background_mode
BG_MAX_FRAMES = 1 << 24                                                    # frames one set of accumulators takes
# where the accumulate kernel splits the frames of a chunk over grid.y and merges with atomics (csrc/sba_background.hpp), for the
# tests that sit either side of it: a frame of fewer than BG_SPLIT_GROUPS 16-byte groups (height * ceil(width * channels / 16))
# in a chunk of more than BG_SPLIT_FRAMES frames
BG_SPLIT_GROUPS, BG_SPLIT_FRAMES = 65536, 16
BG_STAT_BYTES = {"sum": 4, "sumsq": 8, "hot": 4, "vmax": 1}               # bytes of a value of each accumulator


class YuvMatrix(C.Structure):                                             # sba_yuv_matrix
    _fields_ = [(n, C.c_int32) for n in ("y_offset", "cy", "cvr", "cug", "cvg", "cub")]


class ConvertOpts(C.Structure):                                           # sba_convert_opts
    _fields_ = [("frames_on_device", C.c_int32), ("out_on_device", C.c_int32), ("out_format", C.c_int32),
                ("chunk_frames", C.c_int32), ("reserved", C.c_int32 * 8)]


PIXEL_FORMATS = {"bgr": 0, "rgb": 1, "bgra": 2, "rgba": 3, "b": 4, "g": 5, "r": 6}      # sba_pixel_format
PIXEL_BYTES = {"bgr": 3, "rgb": 3, "bgra": 4, "rgba": 4, "b": 1, "g": 1, "r": 1}
YUV_FORMATS = ("nv12", "nv21", "i420", "yv12")
YUV_BT601 = (16, 1220542, 1673527, -409993, -852492, 2116026)             # OpenCV's table: what a NULL matrix means
# geometry of the kernel (csrc/sba_convert.hpp), for the tests that straddle it: the pixels of a row a lane owns, the pixels a
# wave spans, the rows of a workgroup's tile
CONVERT_RUN, CONVERT_WAVE_COLS, CONVERT_TILE_ROWS = 16, 512, 16


class ResizeOpts(C.Structure):                                            # sba_resize_opts
    _fields_ = [("frames_on_device", C.c_int32), ("out_on_device", C.c_int32), ("chunk_frames", C.c_int32), ("gray", C.c_int32),
                ("gray_w", C.c_int32 * 3), ("reserved", C.c_int32 * 5)]


RESIZE_MAX_FACTOR = 16
GRAY_BGR = (3735, 19235, 9798)                                            # OpenCV's weights of B, G, R: what all-zero gray_w means
GRAY_SHIFT = 15                                                           # the weights sum to 2^15
# the items (source bytes, or source pixels with gray) of a row that a wave takes in one step (csrc/sba_resize.hpp), for the
# tests that straddle a segment
RESIZE_ITEMS = 1024


class RgbMatrix(C.Structure):                                             # sba_rgb_matrix
    _fields_ = [(n, C.c_int32) for n in ("y_offset", "cry", "cgy", "cby", "cru", "cgu", "cbu", "crv", "cgv", "cbv")]


class ToYuvOpts(C.Structure):                                             # sba_to_yuv_opts
    _fields_ = [("frames_on_device", C.c_int32), ("out_on_device", C.c_int32), ("in_format", C.c_int32), ("chroma", C.c_int32),
                ("chunk_frames", C.c_int32), ("reserved", C.c_int32 * 7)]


RGB_BT601 = (16, 269484, 528482, 102760, -155188, -305135, 460324, 460324, -385875, -74448)   # OpenCV's table: a NULL matrix
CHROMA_MODES = {"nearest": 0, "average": 1}                               # sba_chroma_mode
IN_FORMATS = {"bgr": 3, "rgb": 3, "bgra": 4, "rgba": 4, "gray": 1}        # what frames_to_yuv reads: the channels of each


class YuvPlanes(C.Structure):                                             # sba_yuv_planes
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("y_row_pitch", C.c_int64), ("y_frame_pitch", C.c_int64),
                ("c_row_pitch", C.c_int64), ("c_frame_pitch", C.c_int64), ("c_step", C.c_int32), ("reserved", C.c_int32)]


class UndistortYuvOpts(C.Structure):                                      # sba_undistort_yuv_opts
    _fields_ = [("frames_on_device", C.c_int32), ("out_on_device", C.c_int32), ("interpolation", C.c_int32), ("border_y", C.c_int32),
                ("border_u", C.c_int32), ("border_v", C.c_int32), ("chunk_frames", C.c_int32), ("reserved", C.c_int32 * 5)]


# the tile of luma pixels one workgroup of k_undistort_yuv owns and the workgroups a launch aims at, above which a workgroup walks
# more than one frame of its chunk (csrc/sba_undistort_yuv.hpp), for the tests that straddle them
UNDIST_YUV_TILE_ROWS, UNDIST_YUV_TILE_COLS, UNDIST_YUV_GROUPS = 8, 128, 2048


def rgb_matrix_in_bound(m):
    """Whether the ten integers (y_offset, cry, cgy, cby, cru, cgu, cbu, crv, cgv, cbv) are a matrix sba_frames_to_yuv accepts:
    32-bit values, y_offset in 0..255 and 255 (|a| + |b| + |c|) < 2^28 for each of the three rows."""
    vals = [int(v) for v in m]
    if len(vals) != 10 or any(not -(1 << 31) <= v < (1 << 31) for v in vals[1:]) or not 0 <= vals[0] <= 255:
        return False
    return all(255 * sum(abs(c) for c in vals[i:i + 3]) < (1 << 28) for i in (1, 4, 7))


def yuv_matrix_in_bound(m):
    """Whether the six integers (y_offset, cy, cvr, cug, cvg, cub) are a matrix sba_convert_frames accepts: 32-bit values,
    y_offset in 0..255 and 255 |cy| + 128 (|a| + |b|) + 2^19 < 2^31 for each output row's chroma coefficients a, b."""
    y_offset, cy, cvr, cug, cvg, cub = (int(v) for v in m)
    if any(not -(1 << 31) <= v < (1 << 31) for v in (cy, cvr, cug, cvg, cub)) or not 0 <= y_offset <= 255:
        return False
    return all(255 * abs(cy) + 128 * ab + (1 << 19) < (1 << 31) for ab in (abs(cvr), abs(cug) + abs(cvg), abs(cub)))


class AlignOpts(C.Structure):
    _fields_ = [("with_scale", C.c_int32), ("apply", C.c_int32), ("reserved", C.c_int32 * 6)]


class AlignReport(C.Structure):
    _fields_ = [("scale", C.c_double), ("R", C.c_double * 9), ("t", C.c_double * 3), ("rms_before", C.c_double),
                ("rms_after", C.c_double), ("max_after", C.c_double), ("n_points_used", C.c_int64), ("n_cams_used", C.c_int32),
                ("reserved", C.c_int32), ("sv", C.c_double * 3), ("seconds_device", C.c_double), ("seconds_total", C.c_double)]


class ReprojOpts(C.Structure):
    _fields_ = [("select", C.c_int32), ("hist_bins", C.c_int32), ("hist_bin_px", C.c_double), ("grid_x", C.c_int32),
                ("grid_y", C.c_int32), ("radial_bins", C.c_int32), ("n_worst", C.c_int32), ("width", C.c_double),
                ("height", C.c_double), ("r_max_px", C.c_double), ("reserved", C.c_int32 * 6)]


class ReprojReport(C.Structure):
    _fields_ = [("n_selected", C.c_int64), ("n_unselected", C.c_int64), ("n_nonfinite", C.c_int64), ("n_overflow", C.c_int64),
                ("n_worst", C.c_int32), ("reserved", C.c_int32), ("mean_du", C.c_double), ("mean_dv", C.c_double),
                ("mean", C.c_double), ("rms", C.c_double), ("max", C.c_double), ("q50", C.c_double), ("q95", C.c_double),
                ("q99", C.c_double), ("seconds_device", C.c_double), ("seconds_total", C.c_double)]


REPROJ_SELECT = {"all": 0, "used": 1, "held_out": 2}                      # sba_reproj_opts.select
REPROJ_DEFAULT_BINS, REPROJ_DEFAULT_BIN_PX = 1024, 1.0 / 16


class UploadOpts(C.Structure):
    _fields_ = [("obs_on_device", C.c_int32), ("layout", C.c_int32), ("reserved", C.c_int32 * 6)]


class UploadReport(C.Structure):
    _fields_ = [("route", C.c_int32), ("decline_reason", C.c_int32), ("dense", C.c_int32), ("masked", C.c_int32),
                ("group_indexed", C.c_int32), ("identity_perm", C.c_int32), ("n_blocks", C.c_int32), ("n_chunks", C.c_int32),
                ("max_degree", C.c_int32), ("stream_syncs", C.c_int32), ("reserved", C.c_int32 * 2),
                ("seconds_total", C.c_double), ("seconds_h2d", C.c_double), ("seconds_device_layout", C.c_double),
                ("seconds_host_layout", C.c_double), ("seconds_tables", C.c_double)]


LAYOUT_ROUTES = {"auto": 0, "host": 1, "device": 2}                       # sba_layout_route
UPLOAD_ROUTE_NAMES = ("host", "device dense", "device general")            # sba_upload_route
DECLINE_NAMES = (None, "index out of range", "duplicate pair", "more than 256 observations of a point")   # sba_layout_decline


class Covariance:
    """Result of Problem.covariance: camera blocks (C, P, P), optionally the full camera matrix (n, n) and the point blocks
    (N, 3, 3), plus sigma2, dof, gauge_rank, n_points_degenerate, n_points_anchored, info, gauge_residual and the timings
    (seconds_device = seconds_form + seconds_inverse + seconds_points, kernels only; seconds_total, the whole call)."""

    def __init__(self, cameras, cameras_full, points, rep):
        self.cameras, self.cameras_full, self.points = cameras, cameras_full, points
        for name, _t in CovReport._fields_:
            setattr(self, name, getattr(rep, name))

    def camera_std(self):
        """(C, P) standard deviations of the camera parameters."""
        return np.sqrt(np.einsum("cii->ci", self.cameras))

    def point_std(self):
        """(N, 3) standard deviations of the point coordinates (NaN for points seen by fewer than two cameras)."""
        if self.points is None:
            raise ValueError("the point covariance was not computed (points=False)")
        return np.sqrt(np.einsum("nii->ni", self.points))


class Triangulation:
    """Result of Problem.triangulate (sba_triangulate, include/sba_hip.h): ``points`` (N, 3), ``status`` (N,) of TRI_*,
    ``n_views``, ``rms_px``, ``max_px``, ``spread`` (N,), ``inliers`` (M,) bool in the caller's observation order, the
    report's counts and seconds as attributes, and ``ok``: the mask of the points with status TRI_OK."""

    def __init__(self, points, status, n_views, rms_px, max_px, spread, inliers, rep):
        self.points, self.status, self.n_views = points, status, n_views
        self.rms_px, self.max_px, self.spread, self.inliers = rms_px, max_px, spread, inliers
        for name, _t in TriReport._fields_:
            setattr(self, name, getattr(rep, name))

    @property
    def ok(self):
        return self.status == TRI_OK


class Unprojection:
    """Result of Problem.unproject (sba_unproject, include/sba_hip.h): ``points`` (N, 3), ``status`` (N,) of UNP_*, ``n_views``,
    ``rms_px``, ``max_px`` (N,), ``used`` (M,) bool in the caller's observation order, the report's counts and seconds as
    attributes, and ``ok``: the mask of the points with status UNP_OK."""

    def __init__(self, points, status, n_views, rms_px, max_px, used, rep):
        self.points, self.status, self.n_views = points, status, n_views
        self.rms_px, self.max_px, self.used = rms_px, max_px, used
        for name, _t in UnpReport._fields_:
            setattr(self, name, getattr(rep, name))

    @property
    def ok(self):
        return self.status == UNP_OK


class LaserDots:
    """Result of detect_dots (sba_detect_dots, include/sba_hip.h), one row per frame: ``sums`` (B, 12) uint64 -- n, sum m x,
    sum m y, sum m x^2, sum m y^2, sum m x y, sum w, sum w x, sum w y, n_sat, 0, 0; ``box`` (B, 4) int32 -- xmin, ymin, xmax, ymax;
    ``centroid`` (B, 4) float64 -- binary x, y, then weighted x, y (columns first: x is the column, y the row); ``status`` (B,)
    int32 of DOT_*; ``n`` (B,) the number of pixels above the threshold; ``ok`` the mask of the frames with status DOT_OK."""

    def __init__(self, sums, box, centroid, status):
        self.sums, self.box, self.centroid, self.status = sums, box, centroid, status

    @property
    def n(self):
        return self.sums[:, 0]

    @property
    def ok(self):
        return self.status == DOT_OK

    @property
    def spread_px(self):
        """(B,) RMS distance of the pixels above the threshold from their binary centroid,
        sqrt(sum m x^2 / n - cx^2 + sum m y^2 / n - cy^2), computed on the host; NaN where n = 0."""
        n = self.sums[:, 0].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            var = (self.sums[:, 3] / n - self.centroid[:, 0] ** 2) + (self.sums[:, 4] / n - self.centroid[:, 1] ** 2)
            return np.sqrt(np.maximum(var, 0.0))


class LaserBlobs:
    """Result of detect_blobs (sba_detect_blobs, include/sba_hip.h), one row per frame: ``n_components`` (B,) int32, the true
    number of 8-connected components of the morphed mask; ``blobs`` (B, K, 12) uint64 -- of the first K = max_blobs components
    in label order n, sum x, sum y, n_raw, sum w, sum w x, sum w y, n_sat, xmin, ymin, xmax, ymax (zero rows beyond);
    ``accepted`` (B,) int32, the table index of the single accepted component or -1; ``centroid`` (B, 4) float64 -- binary x, y
    of it (over the morphed pixels), then weighted x, y (over the raw ones); ``status`` (B,) int32 of BLOB_*; ``mask`` (B, H, W)
    uint8 and ``labels`` (B, H, W) int32 when asked for, else None."""

    def __init__(self, n_components, blobs, accepted, centroid, status, mask=None, labels=None):
        self.n_components, self.blobs, self.accepted, self.centroid, self.status = n_components, blobs, accepted, centroid, status
        self.mask, self.labels = mask, labels

    @property
    def ok(self):
        return self.status == BLOB_OK


class Alignment:
    """Result of Problem.align (sba_align, include/sba_hip.h): the similarity dst ~ scale R src + t as ``scale``, ``R`` (3, 3),
    ``t`` (3,), the distances ``rms_before``, ``rms_after``, ``max_after``, the counts ``n_points_used``, ``n_cams_used``, the
    singular values ``sv`` (3,) of the correlation matrix and the report's seconds."""

    def __init__(self, rep):
        self.scale = rep.scale
        self.R = np.array(rep.R, dtype=np.float64).reshape(3, 3)
        self.t = np.array(rep.t, dtype=np.float64)
        self.sv = np.array(rep.sv, dtype=np.float64)
        for name in ("rms_before", "rms_after", "max_after", "n_points_used", "n_cams_used", "seconds_device", "seconds_total"):
            setattr(self, name, getattr(rep, name))

    def transform(self, X):
        """scale R X + t for an (..., 3) array of points."""
        return self.scale * (np.asarray(X, dtype=np.float64) @ self.R.T) + self.t


class ReprojStats:
    """Result of Problem.reproj_stats (sba_reproj_stats, include/sba_hip.h).  ``cam_stats`` (C, 9): n, mean du, mean dv, mean,
    rms, max, q50, q95, q99 per camera; ``cam_hist`` (C, B) int64 with the overflow bin last; ``cam_grid`` (C, gy, gx, 4): n,
    mean du, mean dv, rms per image cell, or None; ``cam_radial`` (C, nr, 4): n, mean radial, mean tangential, rms per radial
    bin, or None; ``pt_stats`` (N, 3): n, rms, max per point, or None; ``errors`` (M,) in the caller's order, or None;
    ``worst_idx`` / ``worst_err`` (n_worst,): the worst observations, largest first.  The report's fields (``n_selected``,
    ``n_unselected``, ``n_nonfinite``, ``n_overflow``, ``mean_du``, ``mean_dv``, ``mean``, ``rms``, ``max``, ``q50``, ``q95``,
    ``q99``, the seconds) are attributes; ``bin_edges`` (B + 1,) are the histogram's edges in pixels (the last bin is open:
    its upper edge is inf), ``total_hist`` (B,) the sum over the cameras, ``hist_bin_px``, ``r_max_px`` the resolved options."""

    def __init__(self, cam_stats, cam_hist, cam_grid, cam_radial, pt_stats, errors, worst_idx, worst_err, rep, hist_bin_px, r_max_px):
        self.cam_stats, self.cam_hist, self.cam_grid, self.cam_radial = cam_stats, cam_hist, cam_grid, cam_radial
        self.pt_stats, self.errors = pt_stats, errors
        self.worst_idx, self.worst_err = worst_idx[: rep.n_worst], worst_err[: rep.n_worst]
        for name, _t in ReprojReport._fields_:
            if name != "reserved":
                setattr(self, name, getattr(rep, name))
        self.hist_bin_px, self.r_max_px = hist_bin_px, r_max_px
        B = cam_hist.shape[1]
        self.bin_edges = np.append(np.arange(B) * hist_bin_px, np.inf)
        self.total_hist = cam_hist.sum(axis=0)

    @property
    def radial_edges(self):
        """(nr + 1,) edges of the radial bins in pixels (the last bin also takes every larger radius), or None."""
        if self.cam_radial is None:
            return None
        nr = self.cam_radial.shape[1]
        return np.arange(nr + 1) * (self.r_max_px / nr)


_lib = None


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME as /opt/rocm's);
    if this library pulled in the system copy first, a later ``import torch`` would bring up a second runtime that
    finds no GPU ("No HIP GPUs are available").  When torch is installed but not imported yet, its copy is loaded
    first so that both resolve to the same runtime; torch itself is not imported."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.isfile(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Load libsba_hip.so once; raise (never fall back) when it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SbaError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C lasercalib_amd/csrc`. lasercalib_amd has no CPU fallback.")
    _preload_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    H = C.c_void_p
    sig = {
        "sba_abi_version": (C.c_int, []),
        "sba_device_count": (C.c_int, []),
        "sba_last_error": (C.c_char_p, [H]),
        "sba_rotate": (C.c_int, [C.c_int, C.c_int, C.c_int64, dp, dp, dp]),
        "sba_project": (C.c_int, [C.c_int, C.c_int, C.c_int64, dp, dp, dp]),
        "sba_project_model": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int64, dp, dp, dp]),
        "sba_create": (C.c_int, [C.POINTER(ProblemDesc), C.POINTER(H)]),
        "sba_upload": (C.c_int, [H, dp, dp, dp, ip, ip, dp]),
        "sba_upload_ex": (C.c_int, [H, dp, dp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(UploadOpts)]),
        "sba_get_upload_report": (C.c_int, [H, C.POINTER(UploadReport)]),
        "sba_get_layout": (C.c_int, [H] + [C.c_void_p] * 11),
        "sba_set_params": (C.c_int, [H, dp]),
        "sba_get_params": (C.c_int, [H, dp, dp]),
        "sba_destroy": (C.c_int, [H]),
        "sba_get_gradient": (C.c_int, [H, dp, dp]),
        "sba_get_transform": (C.c_int, [H, dp]),
        "sba_lm_get_step": (C.c_int, [H, dp]),
        "sba_residual": (C.c_int, [H, dp, dp, dp]),
        "sba_residual_jacobian": (C.c_int, [H, dp, dp, dp, dp]),
        "sba_solve_lm": (C.c_int, [H, C.POINTER(LmOpts), dp, dp, C.POINTER(LmReport),
                                   C.POINTER(LmIterLog), C.c_int32, C.POINTER(C.c_int32)]),
        "sba_lm_exchange_size": (C.c_int64, [H]),
        "sba_lm_begin": (C.c_int, [H, C.POINTER(LmOpts)]),
        "sba_lm_linearize": (C.c_int, [H]),
        "sba_lm_form_reduced": (C.c_int, [H, C.c_void_p]),
        "sba_lm_solve_trial": (C.c_int, [H, C.c_void_p, C.c_void_p]),
        "sba_lm_decide": (C.c_int, [H, C.c_void_p, C.c_int32, C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int32), C.POINTER(LmIterLog)]),
        "sba_lm_decide_async": (C.c_int, [H, C.c_void_p, C.c_int32]),
        "sba_lm_poll": (C.c_int, [H, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "sba_lm_run": (C.c_int, [H, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "sba_lm_finish": (C.c_int, [H, dp, dp, C.POINTER(LmReport)]),
        "sba_lm_get_log": (C.c_int, [H, C.POINTER(LmIterLog), C.c_int32, C.POINTER(C.c_int32)]),
        "sba_time_kernel": (C.c_int, [H, C.c_char_p, C.c_int32, dp]),
        "sba_get_kernel_profile": (C.c_int, [H, dp, ip]),
        "sba_comm_get_unique_id": (C.c_int, [C.c_char_p]),
        "sba_comm_init": (C.c_int, [H, C.c_char_p, C.c_int32, C.c_int32]),
        "sba_ipc_export": (C.c_int, [H, C.c_int32, C.c_char_p]),
        "sba_ipc_attach": (C.c_int, [H, C.c_int32, C.c_int32, C.c_char_p]),
        "sba_set_fixed_points": (C.c_int, [H, C.c_void_p]),
        "sba_set_robust_loss": (C.c_int, [H, C.c_int32, C.c_double]),
        "sba_covariance": (C.c_int, [H, C.POINTER(CovOpts), dp, dp, dp, C.POINTER(CovReport)]),
        "sba_triangulate": (C.c_int, [H, C.POINTER(TriOpts), dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), dp, dp, dp,
                                      C.POINTER(C.c_uint8), C.POINTER(TriReport)]),
        "sba_unproject_rows": (C.c_int, [C.c_int, C.c_int, C.c_int64, dp, dp, dp, C.c_int64, dp, dp, dp, dp, dp, C.POINTER(C.c_int32)]),
        "sba_unproject": (C.c_int, [H, C.POINTER(UnpOpts), dp, C.c_int64, dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), dp, dp,
                                    C.POINTER(C.c_uint8), C.POINTER(UnpReport)]),
        "sba_detect_dots": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                      C.POINTER(DotOpts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "sba_detect_blobs": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                       C.POINTER(BlobOpts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
        "sba_undistort_frames": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                           C.POINTER(LensStruct), dp, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                           C.POINTER(UndistortOpts), C.c_void_p, C.c_void_p, C.c_void_p]),
        "sba_warp_frames": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                      C.POINTER(LensStruct), dp, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                      C.POINTER(UndistortOpts), C.c_void_p, C.c_void_p, C.c_void_p]),
        "sba_background_accumulate": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                                C.POINTER(BgAccumulateOpts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.c_uint64)]),
        "sba_background_suppress": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                              C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(BgSuppressOpts), C.c_void_p]),
        "sba_convert_frames": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                         C.c_int64, C.c_int64, C.c_int32, C.POINTER(YuvMatrix), C.c_int64, C.c_int64,
                                         C.POINTER(ConvertOpts), C.c_void_p]),
        "sba_frames_to_yuv": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                        C.POINTER(RgbMatrix), C.POINTER(ToYuvOpts)]),
        "sba_undistort_yuv": (C.c_int, [C.c_int, C.POINTER(YuvPlanes), C.c_int64, C.c_int32, C.c_int32, C.POINTER(LensStruct), dp, C.c_int32,
                                        C.c_int32, C.POINTER(YuvPlanes), C.POINTER(UndistortYuvOpts), C.c_void_p, C.c_void_p]),
        "sba_frame_histograms": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                           C.POINTER(HistOpts), C.c_void_p, C.c_void_p]),
        "sba_refine_corners": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, ip, dp,
                                         C.POINTER(CornerOpts), dp, dp, C.c_void_p, C.c_void_p, dp]),
        "sba_adaptive_threshold": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                             C.POINTER(AdaptiveOpts), C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
        "sba_resize_frames": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32,
                                        C.c_int32, C.c_int64, C.c_int64, C.POINTER(ResizeOpts), C.c_void_p]),
        "sba_align": (C.c_int, [H, C.POINTER(AlignOpts), dp, dp, dp, dp, C.POINTER(AlignReport)]),
        "sba_apply_similarity": (C.c_int, [H, C.c_double, dp, dp]),
        "sba_reproj_stats": (C.c_int, [H, C.POINTER(ReprojOpts), dp, ip, dp, dp, dp, dp, ip, dp, C.POINTER(ReprojReport)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.sba_abi_version() != 2:
        raise SbaError("libsba_hip.so ABI version mismatch")
    _lib = lib
    return lib


def _dptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _is_tensor(a):
    return type(a).__module__.split(".")[0] == "torch" and hasattr(a, "data_ptr")


def _device_tensor(name, t, dtype, device):
    """A torch tensor handed over as a device pointer: on the handle's device, float64 / int64, contiguous."""
    if not t.is_cuda or (t.device.index or 0) != device:
        raise ValueError(f"{name}: the tensor must live on the handle's device (cuda:{device})")
    if str(t.dtype) != "torch." + dtype:
        raise ValueError(f"{name}: the tensor must be {dtype}, not {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: the tensor must be contiguous")
    return t


def _check(rc, handle=None):
    if rc == 0:
        return
    msg = load().sba_last_error(handle)
    text = msg.decode() if msg else ""
    if rc == -4:
        # scipy raises ValueError here (scipy/optimize/_lsq/least_squares.py:844-845); keep the type.
        raise ValueError(text or "Residuals are not finite in the initial point.")
    raise SbaError(f"libsba_hip status {rc}: {text}")


def dtype_code(dtype):
    if dtype in (SBA_F64, "f64", "float64", np.float64):
        return SBA_F64
    if dtype in (SBA_F32, "f32", "float32", np.float32):
        return SBA_F32
    raise ValueError(f"unknown dtype {dtype!r}")


def device_count():
    return int(load().sba_device_count())


COMM_ID_BYTES = 128
IPC_HANDLE_BYTES = 64


def comm_unique_id():
    """Rank 0: a fresh 128-byte ncclUniqueId (bytes) to hand to every rank's Problem.comm_init."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(load().sba_comm_get_unique_id(buf))
    return buf.raw


def cam_model_of(n_cam_params):
    """11 columns = the reference's radial camera row (pySBA.py:31-35), 13 = radial + tangential (p1, p2 before cx, cy)."""
    if n_cam_params == 11:
        return CAM_RADIAL
    if n_cam_params == 13:
        return CAM_RADIAL_TANGENTIAL
    raise ValueError("camera rows must have 11 columns (radial model) or 13 (radial + tangential)")


def project_rows(points, cam_rows, dtype=SBA_F64, device=0):
    """PySBA.project on gathered rows (pySBA.py:76-89), computed on the GPU."""
    lib = load()
    p, c = _f64(points), _f64(cam_rows)
    if p.ndim != 2 or p.shape[1] != 3 or c.ndim != 2 or c.shape[1] not in (11, 13) or p.shape[0] != c.shape[0]:
        raise ValueError("project expects (M,3) points and (M,11) camera rows ((M,13) with tangential distortion)")
    out = np.empty((p.shape[0], 2))
    _check(lib.sba_project_model(device, dtype_code(dtype), cam_model_of(c.shape[1]), p.shape[0], _dptr(p), _dptr(c), _dptr(out)))
    return out


def rotate_rows(points, rot_vecs, dtype=SBA_F64, device=0):
    """PySBA.rotate on gathered rows (pySBA.py:61-73), computed on the GPU."""
    lib = load()
    p, r = _f64(points), _f64(rot_vecs)
    if p.ndim != 2 or p.shape[1] != 3 or r.shape != p.shape:
        raise ValueError("rotate expects (M,3) points and (M,3) rotation vectors")
    out = np.empty_like(p)
    _check(lib.sba_rotate(device, dtype_code(dtype), p.shape[0], _dptr(p), _dptr(r), _dptr(out)))
    return out


def _planes(planes, rows, what):
    """(1, 4) or (rows, 4) float64 plane rows (n_x, n_y, n_z, d) from a (4,), (1, 4) or (rows, 4) array."""
    pl = _f64(planes)
    if pl.ndim == 1:
        pl = pl.reshape(1, -1)
    if pl.ndim != 2 or pl.shape[1] != 4:
        raise ValueError(f"{what}: planes must be (4,) or (n, 4) rows of (n_x, n_y, n_z, d), got {pl.shape}")
    return np.ascontiguousarray(pl)


def z_planes(z, n_points):
    """(1, 4) or (n_points, 4) plane rows (0, 0, 1, z) from a scalar or an (n_points,) array of heights."""
    z = np.asarray(z, dtype=np.float64)
    if z.ndim > 1 or (z.ndim == 1 and z.shape[0] != n_points):
        raise ValueError(f"z must be a scalar or have one entry per 3-D point ({n_points}), got shape {z.shape}")
    pl = np.zeros((z.size, 4))
    pl[:, 2] = 1.0
    pl[:, 3] = z.reshape(-1)
    return pl


def unproject_rows(uv, cam_rows, planes=None, device=0):
    """The inverse of ``project_rows`` (sba_unproject_rows, include/sba_hip.h): pixels (M, 2) and gathered camera rows (M, 11) or
    (M, 13) become rays, and with ``planes`` -- (4,) for one plane n . X = d, or (M, 4) -- the points where the rays meet them.
    Returns a dict: ``xn`` (M, 2) undistorted normalised coordinates, ``origin``, ``dir`` (M, 3), ``status`` (M,) of UNP_ROW_*,
    and with planes ``points`` (M, 3) and ``depth`` (M,)."""
    lib = load()
    p, c = _f64(uv), _f64(cam_rows)
    if p.ndim != 2 or p.shape[1] != 2 or c.ndim != 2 or c.shape[1] not in (11, 13) or p.shape[0] != c.shape[0]:
        raise ValueError("unproject expects (M,2) pixels and (M,11) camera rows ((M,13) with tangential distortion)")
    n = p.shape[0]
    pl = None if planes is None else _planes(planes, n, "unproject_rows")
    out = dict(xn=np.empty((n, 2)), origin=np.empty((n, 3)), dir=np.empty((n, 3)), status=np.empty(n, np.int32))
    if pl is not None:
        out.update(points=np.empty((n, 3)), depth=np.empty(n))
    _check(lib.sba_unproject_rows(device, cam_model_of(c.shape[1]), n, _dptr(p), _dptr(c), _dptr(pl), 0 if pl is None else pl.shape[0],
                                  _dptr(out["xn"]), _dptr(out["origin"]), _dptr(out["dir"]), _dptr(out.get("points")),
                                  _dptr(out.get("depth")), out["status"].ctypes.data_as(C.POINTER(C.c_int32))))
    return out


def _frame_layout(frames, device):
    """(tensor?, B, H, W, C, row stride, frame stride) of a batch of uint8 frames, numpy or device tensor; ValueError when the
    layout is not one the detectors read in place."""
    tensor = _is_tensor(frames)
    if tensor:
        if not frames.is_cuda or (frames.device.index or 0) != device:
            raise ValueError(f"frames: the tensor must live on cuda:{device}")
        if str(frames.dtype) != "torch.uint8":
            raise ValueError(f"frames: the tensor must be uint8, not {frames.dtype}")
        shape, strides = tuple(frames.shape), tuple(frames.stride())
    else:
        frames = np.asarray(frames)
        if frames.dtype != np.uint8:
            raise ValueError(f"frames must be uint8, not {frames.dtype}")
        shape, strides = frames.shape, frames.strides
    if len(shape) == 3:
        shape, strides = shape + (1,), strides + (1,)
    if len(shape) != 4 or shape[3] not in (1, 3, 4):
        raise ValueError(f"frames must be (B, H, W, C) with C in (1, 3, 4) or (B, H, W), got {tuple(shape[:len(frames.shape)])}")
    B, H, W, Cn = (int(v) for v in shape)
    sf, sr, sp, sc = (int(v) for v in strides)
    # the strides of an axis of length 1, and all strides of an empty array, say nothing: take those of a packed array
    empty = B * H * W == 0
    sc = 1 if Cn == 1 or empty else sc
    sp = Cn if W == 1 or empty else sp
    sr = W * Cn if H == 1 or empty else sr
    sf = H * sr if B == 1 or empty else sf
    if (sc, sp) != (1, Cn) or sr < W * Cn or sf < H * sr:
        raise ValueError("frames: pixels must be contiguous (channel stride 1, pixel stride C), rows and frames in ascending order; "
                         f"got strides {tuple(strides)} for shape {tuple(shape)}")
    return tensor, frames, B, H, W, Cn, sr, sf


def _addr(a):
    return a.data_ptr() if _is_tensor(a) else a.ctypes.data


def _synced(device, a=None, also=False):
    """The address of ``a`` (a numpy array or a device tensor; None: None) for the C call.  When it is a tensor, or with ``also``
    (the call hands over other tensors), the current stream is synchronised first: what was queued on it is complete before
    the library touches the memory."""
    if also or _is_tensor(a):
        import torch
        torch.cuda.current_stream(device).synchronize()
    return None if a is None else _addr(a)


def _frames_out(out, shapes, on_device, device, like_frames=None):
    """The result of a call that turns frames into frames -> (out, is a tensor, address, row stride, frame stride).  ``out``
    None: a packed uint8 array of ``shapes[0]`` is allocated, a tensor on ``device`` with ``on_device``, else a numpy array.
    Otherwise the caller's array is checked -- of one of ``shapes`` (the expected one first; a None among them counts for
    nothing), pixels contiguous -- and its strides are the pitches.  ``like_frames`` True / False: ``out`` must be a tensor / a numpy array,
    as the frames are; None: it may lie on either side."""
    if out is None:
        if on_device:
            import torch
            out = torch.empty(shapes[0], dtype=torch.uint8, device=f"cuda:{device}")
        else:
            out = np.empty(shapes[0], np.uint8)
    else:
        on_device = _is_tensor(out)
        if like_frames is not None and on_device != like_frames:
            raise ValueError("out must be of the kind of frames: a numpy array for numpy frames, a device tensor for tensor frames")
        if not on_device and not (isinstance(out, np.ndarray) and out.flags.writeable):
            raise ValueError("out must be a writeable numpy array" + ("" if like_frames is not None else " or a tensor on the device"))
        if tuple(out.shape) not in shapes:
            raise ValueError(f"out has the shape {tuple(out.shape)}, expected {shapes[0]}")
    _t, _o, _B, _H, _W, _C, osr, osf = _frame_layout(out, device)
    return out, on_device, _addr(out), osr, osf


def _frame_args(frames, device, opts, channel, threshold, chunk_frames, roi_rect, roi_circle):
    """What detect_dots, detect_blobs and frame_histograms do alike with their frames: fills the fields their options structs
    share (``threshold`` None: the struct has none) and returns (B, H, W, leading arguments of the C call -- device, pointer,
    sizes, pitches, options --, the object that owns the pixels)."""
    tensor, frames, B, H, W, Cn, sr, sf = _frame_layout(frames, device)
    opts.channel, opts.frames_on_device, opts.chunk_frames = int(channel), 1 if tensor else 0, int(chunk_frames)
    if threshold is not None:
        opts.threshold = int(threshold)
    if roi_rect is not None:
        opts.roi_rect = (C.c_int32 * 4)(*(int(v) for v in roi_rect))
    if roi_circle is not None:
        opts.roi_circle = (C.c_int32 * 3)(*(int(v) for v in roi_circle))
    return B, H, W, (device, C.c_void_p(_synced(device, frames)), B, H, W, Cn, sr, sf, C.byref(opts)), frames


def detect_dots(frames, threshold=50, channel=1, min_area=0, max_area=0, max_extent=0, roi_rect=None, roi_circle=None,
                chunk_frames=0, device=0):
    """Thresholded image moments of a batch of frames (sba_detect_dots, include/sba_hip.h) -> LaserDots.

    ``frames``: uint8, (B, H, W, C) with C in (1, 3, 4) or (B, H, W).  A numpy array is read where it is, in any layout whose
    pixels are contiguous (channel stride 1, pixel stride C) and whose row and frame strides are large enough: the pitches are
    its strides, nothing is copied on the host.  A torch tensor on ``device`` is handed over as a device pointer and read in
    place.  ``channel`` is the thresholded byte of a pixel (the reference: 1, green of BGR), a pixel counts when its value is
    above ``threshold``; ``roi_rect`` = (x0, y0, x1, y1) half-open, ``roi_circle`` = (cx, cy, r); ``min_area``, ``max_area``,
    ``max_extent``: the status rules, 0 = no limit; ``chunk_frames``: host frames staged per copy, 0 = the library's default."""
    lib = load()
    opts = DotOpts()
    opts.min_area, opts.max_area, opts.max_extent = int(min_area), int(max_area), int(max_extent)
    B, H, W, args, _keep = _frame_args(frames, device, opts, channel, threshold, chunk_frames, roi_rect, roi_circle)
    sums, box = np.zeros((B, 12), np.uint64), np.zeros((B, 4), np.int32)
    centroid, status = np.full((B, 4), np.nan), np.full(B, DOT_NONE, np.int32)
    _check(lib.sba_detect_dots(*args, sums.ctypes.data, box.ctypes.data, centroid.ctypes.data, status.ctypes.data))
    return LaserDots(sums, box, centroid, status)


def frame_histograms(frames, channel=1, roi_rect=None, roi_circle=None, total=None, want_hist=True, chunk_frames=0, device=0):
    """256-bin histograms of byte ``channel`` of a batch of frames (sba_frame_histograms, include/sba_hip.h) -> (hist, total).

    ``frames``, ``roi_rect``, ``roi_circle`` and ``chunk_frames`` as for ``detect_dots``.  ``hist`` is (B, 256) uint32, one row
    per frame, or None with ``want_hist=False``; ``total`` is (256,) uint64: the sum of the rows added to the ``total`` handed
    in (None: zeros), which is not written -- a video streams through any number of calls by passing each result on."""
    lib = load()
    opts = HistOpts()
    B, _H, _W, args, _keep = _frame_args(frames, device, opts, channel, None, chunk_frames, roi_rect, roi_circle)
    hist = np.zeros((B, 256), np.uint32) if want_hist else None
    if total is None:
        total = np.zeros(256, np.uint64)
    else:
        total = np.array(total, dtype=np.uint64)
        if total.shape != (256,):
            raise ValueError(f"total must hold 256 counts, got the shape {total.shape}")
    _check(lib.sba_frame_histograms(*args, None if hist is None else hist.ctypes.data, total.ctypes.data))
    return hist, total


def detect_blobs(frames, threshold=70, channel=1, dilate_radius=1, close_radius=4, max_blobs=BLOB_DEFAULT_BLOBS, min_area=0,
                 max_area=0, centre=None, max_centre_dist=0, roi_rect=None, roi_circle=None, chunk_frames=0, device=0,
                 want_mask=False, want_labels=False):
    """Connected-component laser-dot detection of a batch of frames (sba_detect_blobs, include/sba_hip.h) -> LaserBlobs.

    ``frames`` as for ``detect_dots``: uint8, (B, H, W, C) with C in (1, 3, 4) or (B, H, W), a numpy array read where it is or a
    torch tensor on ``device`` read in place.  The raw mask (``channel`` above ``threshold`` inside ``roi_rect`` and
    ``roi_circle``) is dilated by disk(``dilate_radius``) and closed by disk(``close_radius``), its 8-connected components are
    numbered in raster order and the first ``max_blobs`` measured.  ``min_area``, ``max_area`` and ``max_centre_dist`` around
    ``centre`` = (x, y) accept or reject a component (0 = no limit); the status is BLOB_OK when exactly one is accepted.
    ``chunk_frames`` caps the frames per chunk, 0 = the library's choice; ``want_mask`` / ``want_labels`` return the morphed
    mask and measure.label's array."""
    lib = load()
    opts = BlobOpts()
    opts.dilate_radius, opts.close_radius, opts.max_blobs = int(dilate_radius), int(close_radius), int(max_blobs)
    opts.min_area, opts.max_area, opts.max_centre_dist = int(min_area), int(max_area), int(max_centre_dist)
    if centre is not None:
        opts.centre_x, opts.centre_y = int(centre[0]), int(centre[1])
    B, H, W, args, _keep = _frame_args(frames, device, opts, channel, threshold, chunk_frames, roi_rect, roi_circle)
    K = int(max_blobs) if 0 < int(max_blobs) <= BLOB_MAX_BLOBS else BLOB_DEFAULT_BLOBS
    ncomp, blobs = np.zeros(B, np.int32), np.zeros((B, K, BLOB_NREC), np.uint64)
    accepted, centroid, status = np.full(B, -1, np.int32), np.full((B, 4), np.nan), np.full(B, BLOB_NONE, np.int32)
    mask = np.zeros((B, H, W), np.uint8) if want_mask else None
    labels = np.zeros((B, H, W), np.int32) if want_labels else None
    _check(lib.sba_detect_blobs(*args, ncomp.ctypes.data, blobs.ctypes.data, accepted.ctypes.data, centroid.ctypes.data, status.ctypes.data,
                                None if mask is None else mask.ctypes.data, None if labels is None else labels.ctypes.data))
    return LaserBlobs(ncomp, blobs, accepted, centroid, status, mask, labels)


def _through_lens(symbol, model, frames, lens9, out_size, interpolation, border_value, out, want_flags, want_map, want_frames,
                  chunk_frames, device, out_on_device):
    """What undistort_frames and warp_frames share -- everything but the front end of the model: ``symbol`` is the entry point,
    ``model`` its float64 values (new_k or m)."""
    lib = load()
    if interpolation not in UNDIST_INTERPOLATION:
        raise ValueError(f"interpolation must be one of {sorted(UNDIST_INTERPOLATION)}, not {interpolation!r}")
    if int(border_value) != border_value or not 0 <= int(border_value) <= 255:
        raise ValueError(f"border_value must be an integer in 0..255, not {border_value!r}")
    tensor, frames, B, H, W, Cn, sr, sf = _frame_layout(frames, device)
    Ho, Wo = (int(v) for v in out_size)
    if not (0 <= Ho <= DOT_MAX_DIM and 0 <= Wo <= DOT_MAX_DIM):
        raise ValueError(f"out_size must be (height, width) within 0..{DOT_MAX_DIM}, got {(Ho, Wo)}")
    lens = LensStruct(*(float(v) for v in lens9))
    opts = UndistortOpts()
    opts.frames_on_device = 1 if tensor else 0
    opts.interpolation, opts.border_value, opts.chunk_frames = UNDIST_INTERPOLATION[interpolation], int(border_value), int(chunk_frames)
    shapes = ((B, Ho, Wo, Cn), (B, Ho, Wo) if Cn == 1 else None)            # a one-channel result may drop the last axis
    osr, osf, optr = Wo * Cn, Ho * Wo * Cn, None
    if not want_frames:
        if out is not None:
            raise ValueError("out was given but no frames are asked for")
        if not (want_flags or want_map):
            raise ValueError("nothing asked for: neither frames nor flags nor map")
    else:
        out, out_tensor, optr, osr, osf = _frames_out(out, shapes if len(frames.shape) == 4 else shapes[::-1],
                                                      tensor if out_on_device is None else bool(out_on_device), device,
                                                      like_frames=tensor if out_on_device is None else None)
        opts.out_on_device = 1 if out_tensor else 0
    flags = np.zeros((Ho, Wo), np.uint8) if want_flags else None
    qmap = np.zeros((Ho, Wo, 2), np.int32) if want_map else None
    _check(getattr(lib, symbol)(device, C.c_void_p(_synced(device, frames, also=bool(opts.out_on_device))), B, H, W, Cn, sr, sf, C.byref(lens), _dptr(model), Ho, Wo, osr, osf,
                                    C.byref(opts), C.c_void_p(optr), None if flags is None else flags.ctypes.data,
                                    None if qmap is None else qmap.ctypes.data))
    return out, flags, qmap


def undistort_frames(frames, lens9, new_k, out_size, interpolation="linear", border_value=0, out=None, want_flags=False,
                     want_map=False, want_frames=True, chunk_frames=0, device=0, out_on_device=None):
    """sba_undistort_frames (include/sba_hip.h): ``frames`` as for ``detect_dots`` (numpy, or a torch tensor on ``device`` read in
    place) resampled through the lens ``lens9`` = (fx, fy, cx, cy, k1, k2, p1, p2, k3) into the pinhole image of ``new_k`` = (fxn,
    fyn, cxn, cyn) of ``out_size`` = (height, width).  Returns (out, flags, map): ``out`` is a numpy array for numpy frames and a
    device tensor for tensor frames -- allocated here, or the caller's ``out``, which may be a strided view with contiguous
    pixels --, None with ``want_frames=False`` (then no frame is read); ``flags`` (height, width) uint8 and ``map`` (height, width, 2) int32 are numpy
    or None.  ``out_on_device`` True / False puts the result on that side whatever side the frames are on (an ``out`` may then be of
    either kind); None keeps it with the frames.  ``lasercalib_amd.imaging`` is the public face of this call."""
    nk = np.ascontiguousarray([float(v) for v in new_k], dtype=np.float64)
    return _through_lens("sba_undistort_frames", nk, frames, lens9, out_size, interpolation, border_value, out, want_flags, want_map,
                         want_frames, chunk_frames, device, out_on_device)


def warp_frames(frames, lens9, m, out_size, interpolation="linear", border_value=0, out=None, want_flags=False, want_map=False,
                want_frames=True, chunk_frames=0, device=0, out_on_device=None):
    """sba_warp_frames (include/sba_hip.h): as ``undistort_frames`` with the 3 x 3 matrix ``m`` (nine values, row-major) in place of
    ``new_k``: destination pixel (x, y) is the normalised camera position m (x, y, 1) taken through the lens ``lens9``.  ``flags``
    may also hold WARP_BEHIND.  ``lasercalib_amd.imaging`` is the public face of this call."""
    m = np.ascontiguousarray(m, dtype=np.float64).reshape(-1)
    if m.shape != (9,):
        raise ValueError(f"m must hold the nine values of a 3 x 3 matrix, got {m.shape[0]}")
    return _through_lens("sba_warp_frames", m, frames, lens9, out_size, interpolation, border_value, out, want_flags, want_map,
                         want_frames, chunk_frames, device, out_on_device)


def _plane(name, a, itemsize, H, W, device, writeable):
    """(is a tensor, pointer) of a packed (H, W) plane of ``itemsize``-byte integers, a numpy array or a tensor on ``device``."""
    if _is_tensor(a):
        if not a.is_cuda or (a.device.index or 0) != device:
            raise ValueError(f"{name}: the tensor must live on cuda:{device}")
        if tuple(a.shape) != (H, W) or a.element_size() != itemsize or a.is_floating_point() or not a.is_contiguous():
            raise ValueError(f"{name}: must be a contiguous ({H}, {W}) tensor of {itemsize}-byte integers, got {tuple(a.shape)} {a.dtype}")
        return True, a.data_ptr()
    if not isinstance(a, np.ndarray) or a.shape != (H, W) or a.dtype.kind not in "uib" or a.dtype.itemsize != itemsize or not a.flags.c_contiguous:
        raise ValueError(f"{name}: must be a C-contiguous ({H}, {W}) numpy array of {itemsize}-byte integers")
    if writeable and not a.flags.writeable:
        raise ValueError(f"{name}: must be writeable")
    return False, a.ctypes.data


def background_accumulate(frames, sum=None, sumsq=None, hot=None, vmax=None, n_used=0, use=None, threshold=50, channel=1,
                          accumulate=True, chunk_frames=0, device=0):
    """sba_background_accumulate (include/sba_hip.h): per-pixel statistics over time of byte ``channel`` of ``frames`` (as for
    ``detect_dots``: numpy, or a torch tensor on ``device`` read in place).  ``sum`` and ``hot`` (4-byte integers), ``sumsq``
    (8-byte) and ``vmax`` (uint8) are (H, W) planes, updated IN PLACE; each may be None; they are all numpy arrays or all
    tensors on ``device`` (torch.int32 / torch.int64 hold the unsigned values' bits).  ``use``: one flag per frame, None = all
    frames.  ``accumulate=False`` overwrites the planes instead of adding to them.  Returns the new frame count:
    ``n_used`` (taken as 0 with ``accumulate=False``) plus the frames that took part."""
    lib = load()
    tensor, frames, B, H, W, Cn, sr, sf = _frame_layout(frames, device)
    opts = BgAccumulateOpts()
    opts.channel, opts.threshold, opts.frames_on_device = int(channel), int(threshold), 1 if tensor else 0
    opts.accumulate, opts.chunk_frames = 1 if accumulate else 0, int(chunk_frames)
    ptrs, kinds = [], set()
    for name, a in (("sum", sum), ("sumsq", sumsq), ("hot", hot), ("vmax", vmax)):
        if a is None:
            ptrs.append(None)
            continue
        on_dev, ptr = _plane(name, a, BG_STAT_BYTES[name], H, W, device, True)
        kinds.add(on_dev)
        ptrs.append(C.c_void_p(ptr))
    if len(kinds) > 1:
        raise ValueError("sum, sumsq, hot and vmax must all be numpy arrays or all be device tensors")
    opts.stats_on_device = 1 if True in kinds else 0
    if use is not None:
        use = np.ascontiguousarray(np.asarray(use) != 0, dtype=np.uint8)
        if use.shape != (B,):
            raise ValueError(f"use must hold one flag per frame ({B}), got the shape {use.shape}")
    n = C.c_uint64(int(n_used))
    ptr = _synced(device, frames, also=bool(opts.stats_on_device))
    _check(lib.sba_background_accumulate(device, C.c_void_p(ptr), B, H, W, Cn, sr, sf, C.byref(opts),
                                         None if use is None else C.c_void_p(use.ctypes.data), *ptrs, C.byref(n)))
    return int(n.value)


def background_suppress(frames, level=None, mask=None, mode="gate", channel=1, out=None, chunk_frames=0, device=0):
    """sba_background_suppress (include/sba_hip.h): byte ``channel`` of ``frames`` (as for ``detect_dots``) with the static light
    taken out -> (B, H, W) uint8, a numpy array for numpy frames and a device tensor for tensor frames (allocated here, or the
    caller's ``out``, which may be a strided view with contiguous pixels).  ``level`` and ``mask`` are (H, W) planes of bytes or
    None, both numpy arrays or both tensors on ``device``.  ``mode`` "gate": 0 where the mask is set or the value is not above
    the level, else the value; "subtract": 0 where the mask is set, else max(value - level, 0)."""
    lib = load()
    if mode not in BG_MODES:
        raise ValueError(f"mode must be one of {sorted(BG_MODES)}, not {mode!r}")
    tensor, frames, B, H, W, Cn, sr, sf = _frame_layout(frames, device)
    opts = BgSuppressOpts()
    opts.channel, opts.frames_on_device, opts.out_on_device = int(channel), 1 if tensor else 0, 1 if tensor else 0
    opts.mode, opts.chunk_frames = BG_MODES[mode], int(chunk_frames)
    ptrs, kinds, keep = [], set(), []
    for name, a in (("level", level), ("mask", mask)):
        if a is None:
            ptrs.append(None)
            continue
        if not _is_tensor(a):
            a = np.ascontiguousarray(a)                  # uint8, or bool (a byte of 0 / 1)
        keep.append(a)
        on_dev, ptr = _plane(name, a, 1, H, W, device, False)
        kinds.add(on_dev)
        ptrs.append(C.c_void_p(ptr))
    if len(kinds) > 1:
        raise ValueError("level and mask must both be numpy arrays or both be device tensors")
    opts.model_on_device = 1 if True in kinds else 0
    if len(getattr(out, "shape", (B, H, W))) != 3:                         # not (B, H, W, 1): the result has no channel axis
        raise ValueError(f"out must be (B, H, W), got the shape {tuple(out.shape)}")
    out, _t, optr, osr, osf = _frames_out(out, ((B, H, W),), tensor, device, like_frames=tensor)
    ptr = _synced(device, frames, also=bool(opts.model_on_device))
    _check(lib.sba_background_suppress(device, C.c_void_p(ptr), B, H, W, Cn, sr, sf, *ptrs, osr, osf, C.byref(opts), C.c_void_p(optr)))
    return out


class YuvLayout:
    """What sba_convert_frames is told about a batch of YUV 4:2:0 frames: the addresses of the three planes, their pitches in
    bytes and the chroma step; ``keep`` holds the objects that own the memory."""

    __slots__ = ("tensor", "n_frames", "height", "width", "y", "u", "v", "y_row_pitch", "y_frame_pitch", "c_row_pitch",
                 "c_frame_pitch", "c_step", "keep")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def pitches(self):
        return self.y_row_pitch, self.y_frame_pitch, self.c_row_pitch, self.c_frame_pitch, self.c_step

    def planes_struct(self):
        """The sba_yuv_planes of sba_undistort_yuv."""
        return YuvPlanes(self.y, self.u, self.v, *self.pitches(), 0)

    def loose_args(self):
        """The same as the eight arguments of sba_convert_frames and sba_frames_to_yuv."""
        return (C.c_void_p(self.y), C.c_void_p(self.u), C.c_void_p(self.v), *self.pitches())


def _int32s(values, n, what):
    """The ``n`` 32-bit integers ``values`` as a list; anything else is a ValueError that opens with ``what``."""
    vals = [int(v) for v in values]
    if len(vals) != n or any(not -(1 << 31) <= v < (1 << 31) for v in vals):
        raise ValueError(f"{what}, got {values!r}")
    return vals


def _bytes_view(name, a, device):
    """(is a tensor, the object, base address, shape, strides in bytes) of a uint8 numpy array or tensor on ``device``."""
    if _is_tensor(a):
        if not a.is_cuda or (a.device.index or 0) != device:
            raise ValueError(f"{name}: the tensor must live on cuda:{device}")
        if str(a.dtype) != "torch.uint8":
            raise ValueError(f"{name}: the tensor must be uint8, not {a.dtype}")
        return True, a, a.data_ptr(), tuple(int(v) for v in a.shape), tuple(int(v) for v in a.stride())
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise ValueError(f"{name} must be uint8, not {a.dtype}")
    return False, a, a.ctypes.data, tuple(int(v) for v in a.shape), tuple(int(v) for v in a.strides)


def _plane_pitches(name, shape, strides, steps):
    """(frame pitch, row pitch, step) of a (B, rows, cols) plane whose samples lie ``step`` bytes apart, step in ``steps``.  The
    strides of an axis of length 1, and all strides of an empty plane, say nothing: those of a packed plane are taken."""
    B, R, Cl = shape
    sf, sr, sp = strides
    empty = B * R * Cl == 0
    sp = steps[0] if Cl == 1 or empty else sp
    if sp not in steps:
        raise ValueError(f"{name}: neighbouring samples of a row must lie {' or '.join(str(s) for s in steps)} byte(s) apart, got {sp}")
    row = sp * (Cl - 1) + 1 if Cl else 0
    sr = row if R == 1 or empty else sr
    sf = R * sr if B == 1 or empty else sf
    if sr < row or sf < R * sr:
        raise ValueError(f"{name}: rows and frames must be in ascending order and must not overlap; got strides {strides} for shape {shape}")
    return sf, sr, sp


def _yuv_layout(frames, pixel_format, device=0):
    """Reads the layout of a batch of 8-bit YUV 4:2:0 frames -> YuvLayout.  ``pixel_format``: "nv12", "nv21" (a luma plane and one
    plane of interleaved UV / VU pairs) or "i420", "yv12" (a luma plane and two chroma planes, U first / V first).  ``frames``:

    * a tuple of planes in the format's order -- ``(y, uv)``, or ``(y, u, v)`` (yv12: ``(y, v, u)``) -- with y (B, H, W), uv
      (B, ceil(H / 2), ceil(W / 2), 2) and u, v (B, ceil(H / 2), ceil(W / 2)); any row and frame strides; the samples of a planar
      chroma row 1 or 2 bytes apart (``uv[..., 0]`` is a plane), the two chroma planes with equal strides; H and W may be odd;
    * one stacked array (B, H + ceil(H / 2), W), as ffmpeg's rawvideo pipe delivers ``nv12`` and ``yuv420p`` frames: the luma
      rows, then the chroma.  nv12 / nv21 need an even W (a chroma row is 2 ceil(W / 2) bytes).  i420 / yv12 need even W and H and
      packed rows (row stride W): their chroma rows are half rows of one packed buffer."""
    fmt = str(pixel_format).lower()
    if fmt not in YUV_FORMATS:
        raise ValueError(f"pixel_format must be one of {YUV_FORMATS}, not {pixel_format!r}")
    semi, first_is_u = fmt in ("nv12", "nv21"), fmt in ("nv12", "i420")
    if isinstance(frames, (tuple, list)):
        if len(frames) != (2 if semi else 3):
            raise ValueError(f"{fmt}: expected a tuple of {'(y, uv)' if semi else '(y, u, v)'} planes, got {len(frames)} planes")
        views = [_bytes_view(n, a, device) for n, a in zip(("y", "chroma", "chroma 2"), frames)]
        if len({t for t, *_ in views}) != 1:
            raise ValueError("the planes must all be numpy arrays or all be tensors on the device")
        tensor, yobj, yptr, yshape, ystr = views[0]
        if len(yshape) != 3:
            raise ValueError(f"y must be (B, H, W), got the shape {yshape}")
        B, H, W = yshape
        ch, cw = (H + 1) // 2, (W + 1) // 2
        ysf, ysr, _one = _plane_pitches("y", yshape, ystr, (1,))
        if semi:
            _t, cobj, cptr, cshape, cstr = views[1]
            if cshape != (B, ch, cw, 2):
                raise ValueError(f"uv must be {(B, ch, cw, 2)} for y of {yshape}, got the shape {cshape}")
            if B * ch * cw and cstr[3] != 1:
                raise ValueError(f"uv: the two bytes of a pair must be neighbours, got strides {cstr}")
            csf, csr, step = _plane_pitches("uv", (B, ch, 2 * cw), (cstr[0], cstr[1], 1), (1,))
            step, first, second = 2, cptr, cptr + 1
            if B * ch * cw and cw > 1 and cstr[2] != 2:
                raise ValueError(f"uv: pairs must be contiguous (stride 2), got strides {cstr}")
        else:
            (_t1, c1, p1, s1, st1), (_t2, c2, p2, s2, st2) = views[1], views[2]
            if s1 != (B, ch, cw) or s2 != (B, ch, cw):
                raise ValueError(f"the chroma planes must be {(B, ch, cw)} for y of {yshape}, got the shapes {s1} and {s2}")
            csf, csr, step = _plane_pitches("chroma", s1, st1, (1, 2))
            if _plane_pitches("chroma 2", s2, st2, (step,)) != (csf, csr, step):
                raise ValueError(f"the two chroma planes must have the same strides, got {st1} and {st2}")
            first, second = p1, p2
        keep = tuple(v[1] for v in views)
    else:
        tensor, obj, ptr, shape, strides = _bytes_view("frames", frames, device)
        if len(shape) != 3:
            raise ValueError(f"frames must be a tuple of planes or one stacked (B, H + ceil(H / 2), W) array, got the shape {shape}")
        B, T, W = shape
        ysf, ysr, _one = _plane_pitches("frames", shape, strides, (1,))
        k, rem = divmod(T, 3)
        if rem == 1:
            raise ValueError(f"stacked frames have H + ceil(H / 2) rows; {T} rows fit no H")
        H = 2 * k + (1 if rem else 0)
        ch, cw = (H + 1) // 2, (W + 1) // 2
        if semi:
            if W % 2:
                raise ValueError(f"stacked {fmt} frames need an even width (a chroma row is 2 ceil(W / 2) bytes), got {W}; "
                                 "pass a tuple of planes instead")
            first, second, step, csr, csf = ptr + H * ysr, ptr + H * ysr + 1, 2, ysr, ysf
        else:
            if W % 2 or H % 2:
                raise ValueError(f"stacked {fmt} frames need an even width and height, got {W} x {H}; pass a tuple of planes instead")
            if ysr != W and B * T * W:
                raise ValueError(f"stacked {fmt} frames need packed rows (row stride {W}), got {ysr}; pass a tuple of planes instead")
            first, step, csr, csf = ptr + H * W, 1, W // 2, ysf
            second = first + ch * cw
        yptr, keep = ptr, (obj,)
    u, v = (first, second) if first_is_u else (second, first)
    return YuvLayout(tensor=tensor, n_frames=B, height=H, width=W, y=yptr, u=u, v=v, y_row_pitch=ysr, y_frame_pitch=ysf,
                     c_row_pitch=csr, c_frame_pitch=csf, c_step=step, keep=keep)


def yuv_frame_slice(frames, lo, hi):
    """The frames [lo, hi) of a batch given as a tuple of planes or as a stacked array."""
    return tuple(p[lo:hi] for p in frames) if isinstance(frames, (tuple, list)) else frames[lo:hi]


def convert_frames(frames, pixel_format, out_format="bgr", matrix=None, out=None, out_on_device=None, chunk_frames=0, device=0):
    """sba_convert_frames (include/sba_hip.h): 8-bit YUV 4:2:0 ``frames`` (see ``_yuv_layout``; numpy, or torch tensors on
    ``device`` read in place) -> (B, H, W, 3 | 4) frames of ``out_format`` "bgr", "rgb", "bgra", "rgba", or the (B, H, W) plane
    "b", "g", "r".  ``matrix``: the six integers (y_offset, cy, cvr, cug, cvg, cub) or None for OpenCV's BT.601 table.  The
    result is allocated on the side the source is on (``out_on_device`` True / False overrides that), or is the caller's
    ``out``: a writeable numpy array or a tensor on ``device`` of that shape, any row and frame strides, padding left untouched.
    ``lasercalib_amd.imaging.convert_frames`` is the public face of this call."""
    lib = load()
    L = _yuv_layout(frames, pixel_format, device)
    fmt = str(out_format).lower()
    if fmt not in PIXEL_FORMATS:
        raise ValueError(f"out_format must be one of {sorted(PIXEL_FORMATS)}, not {out_format!r}")
    Cn = PIXEL_BYTES[fmt]
    B, H, W = L.n_frames, L.height, L.width
    shape = (B, H, W) if Cn == 1 else (B, H, W, Cn)
    m = None if matrix is None else YuvMatrix(*_int32s(matrix, 6, "matrix must be six 32-bit integers (y_offset, cy, cvr, cug, cvg, cub)"))
    out, out_tensor, optr, osr, osf = _frames_out(out, (shape, (B, H, W, Cn)), L.tensor if out_on_device is None else bool(out_on_device), device)
    opts = ConvertOpts()
    opts.frames_on_device, opts.out_on_device = 1 if L.tensor else 0, 1 if out_tensor else 0
    opts.out_format, opts.chunk_frames = PIXEL_FORMATS[fmt], int(chunk_frames)
    _synced(device, also=L.tensor or out_tensor)             # the planes' addresses are in L
    y, u, v, *pitches = L.loose_args()
    _check(lib.sba_convert_frames(device, y, u, v, B, H, W, *pitches, None if m is None else C.byref(m), osr, osf, C.byref(opts),
                                  C.c_void_p(optr)))
    return out


def yuv_planes_alloc(pixel_format, B, H, W, on_device, device=0):
    """Uninitialised memory for ``B`` YUV 4:2:0 frames of ``W`` x ``H`` in ``pixel_format``, as ``_yuv_layout`` reads it: the stacked
    (B, H + H / 2, W) array of ffmpeg's rawvideo pipe when W and H are even, else the tuple of planes in the format's order
    -- ``(y, uv)``, or ``(y, u, v)`` (yv12: ``(y, v, u)``).  numpy, or torch on ``device`` with ``on_device``."""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    if W % 2 == 0 and H % 2 == 0:
        shapes = [(B, H + ch, W)]
    else:
        shapes = [(B, H, W), (B, ch, cw, 2)] if pixel_format in ("nv12", "nv21") else [(B, H, W), (B, ch, cw), (B, ch, cw)]
    if on_device:
        import torch
        planes = [torch.empty(s, dtype=torch.uint8, device=f"cuda:{device}") for s in shapes]
    else:
        planes = [np.empty(s, np.uint8) for s in shapes]
    return planes[0] if len(planes) == 1 else tuple(planes)


def _yuv_out(out, pixel_format, B, H, W, on_device, device, wanted):
    """(out, its YuvLayout) of a call that writes ``B`` YUV 4:2:0 frames of ``W`` x ``H``: the caller's ``out``, checked, or memory
    from ``yuv_planes_alloc``.  ``wanted`` ("the frames are", "the result is") words the second half of the size error."""
    if out is None:
        out = yuv_planes_alloc(pixel_format, B, H, W, on_device, device)
    L = _yuv_layout(out, pixel_format, device)
    if (L.n_frames, L.height, L.width) != (B, H, W):
        raise ValueError(f"out holds {L.n_frames} frames of {L.width} x {L.height}, {wanted} {B} of {W} x {H}")
    if not L.tensor and any(not (isinstance(a, np.ndarray) and a.flags.writeable) for a in L.keep):
        raise ValueError("out must be writeable numpy arrays or tensors on the device")
    return out, L


def frames_to_yuv(frames, pixel_format="nv12", in_format="bgr", matrix=None, chroma="nearest", out=None, out_on_device=None,
                  chunk_frames=0, device=0):
    """sba_frames_to_yuv (include/sba_hip.h): ``frames`` as for ``detect_dots`` (uint8, (B, H, W, C) with C in (1, 3, 4) or
    (B, H, W); numpy, or a torch tensor on ``device`` read in place) -> 8-bit YUV 4:2:0 in ``pixel_format`` "nv12", "nv21",
    "i420" or "yv12".  ``in_format``: "bgr", "rgb" (C = 3), "bgra", "rgba" (C = 4) or "gray" (C = 1); frames with one channel
    are grey whatever it says.  ``matrix``: the ten integers (y_offset, cry, cgy, cby, cru, cgu, cbu, crv, cgv, cbv) or None for
    OpenCV's BT.601 table; ``chroma``: "nearest" or "average".  The result is described as ``_yuv_layout`` reads a source: it
    is ``out`` -- a stacked array or a tuple of planes, numpy (writeable) or tensors on ``device``, any strides that layout
    allows, what lies between the samples left untouched -- or is allocated by ``yuv_planes_alloc`` on the side the frames are
    on (``out_on_device`` True / False overrides that).  ``lasercalib_amd.imaging.frames_to_yuv`` is the public face."""
    fmt, pix = str(in_format).lower(), str(pixel_format).lower()
    if fmt not in IN_FORMATS:
        raise ValueError(f"in_format must be one of {sorted(IN_FORMATS)}, not {in_format!r}")
    if pix not in YUV_FORMATS:
        raise ValueError(f"pixel_format must be one of {YUV_FORMATS}, not {pixel_format!r}")
    if chroma not in CHROMA_MODES:
        raise ValueError(f"chroma must be one of {sorted(CHROMA_MODES)}, not {chroma!r}")
    tensor, frames, B, H, W, Cn, sr, sf = _frame_layout(frames, device)
    if Cn != 1 and IN_FORMATS[fmt] != Cn:
        raise ValueError(f"in_format {fmt!r} has {IN_FORMATS[fmt]} byte(s) per pixel, the frames have {Cn}")
    m = None if matrix is None else RgbMatrix(*_int32s(
        matrix, 10, "matrix must be ten 32-bit integers (y_offset, cry, cgy, cby, cru, cgu, cbu, crv, cgv, cbv)"))
    out, L = _yuv_out(out, pix, B, H, W, tensor if out_on_device is None else bool(out_on_device), device, "the frames are")
    lib = load()
    opts = ToYuvOpts()
    opts.frames_on_device, opts.out_on_device = 1 if tensor else 0, 1 if L.tensor else 0
    opts.in_format = PIXEL_FORMATS.get(fmt, 0)                             # "gray": one channel, the format is not looked at
    opts.chroma, opts.chunk_frames = CHROMA_MODES[chroma], int(chunk_frames)
    ptr = _synced(device, frames, also=L.tensor)
    _check(lib.sba_frames_to_yuv(device, C.c_void_p(ptr), B, H, W, Cn, sr, sf, *L.loose_args(), None if m is None else C.byref(m),
                                 C.byref(opts)))
    return out


def undistort_yuv(frames, pixel_format, lens9, new_k, out_size, interpolation="linear", border=(16, 128, 128), out_pixel_format=None,
                  out=None, out_on_device=None, want_flags=False, want_map=False, want_frames=True, chunk_frames=0, device=0):
    """sba_undistort_yuv (include/sba_hip.h): 8-bit YUV 4:2:0 ``frames`` in ``pixel_format`` (see ``_yuv_layout``; numpy, or torch
    tensors on ``device`` read in place) resampled plane by plane through the lens ``lens9`` = (fx, fy, cx, cy, k1, k2, p1, p2, k3)
    into the pinhole image of ``new_k`` = (fxn, fyn, cxn, cyn) of ``out_size`` = (height, width), in ``out_pixel_format`` (None:
    that of the frames).  ``border`` = (Y, U, V), each 0..255, fills what lies outside the source.  Returns (out, flags, map):
    ``out`` is described as ``_yuv_layout`` reads a source -- the caller's ``out`` (a stacked array or a tuple of planes, numpy
    (writeable) or tensors on ``device``, what lies between the samples left untouched) or allocated by ``yuv_planes_alloc`` on
    the side the frames are on (``out_on_device`` True / False overrides that) --, None with ``want_frames=False`` (then no
    frame is read); ``flags`` (height, width) uint8 and ``map`` (height, width, 2) int32 are those of ``undistort_frames`` for
    the luma plane, numpy or None.  Every ValueError is raised before the library is loaded.
    ``lasercalib_amd.imaging.undistort_yuv`` is the public face of this call."""
    pix = str(pixel_format).lower()
    if pix not in YUV_FORMATS:
        raise ValueError(f"pixel_format must be one of {YUV_FORMATS}, not {pixel_format!r}")
    opix = pix if out_pixel_format is None else str(out_pixel_format).lower()
    if opix not in YUV_FORMATS:
        raise ValueError(f"out_pixel_format must be one of {YUV_FORMATS}, not {out_pixel_format!r}")
    if interpolation not in UNDIST_INTERPOLATION:
        raise ValueError(f"interpolation must be one of {sorted(UNDIST_INTERPOLATION)}, not {interpolation!r}")
    try:
        by, bu, bv = border
        if any(int(b) != b or not 0 <= int(b) <= 255 for b in (by, bu, bv)):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"border must be three integers (Y, U, V) in 0..255, not {border!r}") from None
    S = _yuv_layout(frames, pix, device)
    Ho, Wo = (int(v) for v in out_size)
    if not (0 <= Ho <= DOT_MAX_DIM and 0 <= Wo <= DOT_MAX_DIM):
        raise ValueError(f"out_size must be (height, width) within 0..{DOT_MAX_DIM}, got {(Ho, Wo)}")
    lens = LensStruct(*(float(v) for v in lens9))
    nk = np.ascontiguousarray([float(v) for v in new_k], dtype=np.float64)
    opts = UndistortYuvOpts()
    opts.frames_on_device = 1 if S.tensor else 0
    opts.interpolation, opts.chunk_frames = UNDIST_INTERPOLATION[interpolation], int(chunk_frames)
    opts.border_y, opts.border_u, opts.border_v = int(by), int(bu), int(bv)
    D = dst = None
    if not want_frames:
        if out is not None:
            raise ValueError("out was given but no frames are asked for")
        if not (want_flags or want_map):
            raise ValueError("nothing asked for: neither frames nor flags nor map")
    else:
        out, D = _yuv_out(out, opix, S.n_frames, Ho, Wo, S.tensor if out_on_device is None else bool(out_on_device), device, "the result is")
        opts.out_on_device = 1 if D.tensor else 0
        dst = D.planes_struct()
    lib = load()
    src = S.planes_struct()
    flags = np.zeros((Ho, Wo), np.uint8) if want_flags else None
    qmap = np.zeros((Ho, Wo, 2), np.int32) if want_map else None
    _synced(device, also=S.tensor or bool(opts.out_on_device))             # the planes' addresses are in S and D
    _check(lib.sba_undistort_yuv(device, C.byref(src), S.n_frames, S.height, S.width, C.byref(lens), _dptr(nk), Ho, Wo,
                                 None if dst is None else C.byref(dst), C.byref(opts), None if flags is None else flags.ctypes.data,
                                 None if qmap is None else qmap.ctypes.data))
    return out, flags, qmap


def resize_frames(frames, fx, fy, gray_w=None, out=None, out_on_device=None, chunk_frames=0, device=0):
    """sba_resize_frames (include/sba_hip.h): every pixel of the result is the average of a block of ``fx`` x ``fy`` pixels of
    ``frames`` (as for ``detect_dots``: numpy, or a torch tensor on ``device`` read in place) -> (B, H // fy, W // fx[, C]).
    ``gray_w``: None keeps the channels; three integer weights of the channels 0, 1, 2 (all zero: OpenCV's of B, G, R) give the
    (B, H // fy, W // fx) plane of grey values.  The result is allocated on the side the frames are on (``out_on_device`` True /
    False overrides that), or is the caller's ``out``: a writeable numpy array or a tensor on ``device`` of that shape, which
    may be a view into a larger array -- a tile of a canvas: its row and frame strides are the pitches, the pixels must be
    contiguous, and what lies between its rows is left untouched.  ``lasercalib_amd.imaging.resize_frames`` is the public
    face of this call."""
    lib = load()
    tensor, frames, B, H, W, Cn, sr, sf = _frame_layout(frames, device)
    fx, fy = int(fx), int(fy)
    if not (1 <= fx <= RESIZE_MAX_FACTOR and 1 <= fy <= RESIZE_MAX_FACTOR):
        raise ValueError(f"the factors must be in 1..{RESIZE_MAX_FACTOR}, got {(fx, fy)}")
    opts = ResizeOpts()
    if gray_w is not None:
        opts.gray, opts.gray_w = 1, (C.c_int32 * 3)(*_int32s(gray_w, 3, "gray_w must be three 32-bit integers"))
    Ho, Wo, Co = H // fy, W // fx, 1 if gray_w is not None else Cn
    shape = (B, Ho, Wo, Cn) if gray_w is None and len(frames.shape) == 4 else (B, Ho, Wo)
    shapes = (shape, (B, Ho, Wo, Co), (B, Ho, Wo) if Co == 1 else None)
    out, out_tensor, optr, osr, osf = _frames_out(out, shapes, tensor if out_on_device is None else bool(out_on_device), device)
    opts.frames_on_device, opts.out_on_device, opts.chunk_frames = 1 if tensor else 0, 1 if out_tensor else 0, int(chunk_frames)
    ptr = _synced(device, frames, also=out_tensor)
    _check(lib.sba_resize_frames(device, C.c_void_p(ptr), B, H, W, Cn, sr, sf, fx, fy, osr, osf, C.byref(opts), C.c_void_p(optr)))
    return out


def refine_corners(frames, corner_start, corners, win=(3, 3), zero_zone=(-1, -1), max_iter=200, eps=1e-5, channel=0, gray_w=None,
                   weights=None, chunk_frames=0, device=0):
    """sba_refine_corners (include/sba_hip.h) -> (refined (n, 2) float64, status (n,) int32, iterations (n,) int32, tensor (n, 3)).

    ``frames`` as for ``detect_dots``; ``corner_start`` (B + 1,) int64 and ``corners`` (n, 2) float64 as the header describes
    them; ``win`` = (win_x, win_y) and ``zero_zone`` = (zero_x, zero_y) half sizes; ``channel`` -1 is the grey value with
    ``gray_w`` (None: OpenCV's of B, G, R); ``weights`` None lets the library build OpenCV's window, else the
    (2 win_y + 1, 2 win_x + 1) float64 weights.  ``lasercalib_amd.imaging.refine_corners`` is the public face of this call."""
    lib = load()
    tensor, frames, B, H, W, Cn, sr, sf = _frame_layout(frames, device)
    start = np.ascontiguousarray(corner_start, dtype=np.int64)
    if start.shape != (B + 1,):
        raise ValueError(f"corner_start must hold {B + 1} offsets, got the shape {start.shape}")
    n = int(start[-1])
    xy = _f64(corners).reshape(-1, 2)
    if xy.shape[0] != n:
        raise ValueError(f"corners has {xy.shape[0]} rows, corner_start ends at {n}")
    opts = CornerOpts()
    opts.eps, opts.frames_on_device, opts.chunk_frames, opts.channel = float(eps), 1 if tensor else 0, int(chunk_frames), int(channel)
    if gray_w is not None:
        opts.gray_w = (C.c_int32 * 3)(*_int32s(gray_w, 3, "gray_w must be three 32-bit integers"))
    (opts.win_x, opts.win_y), (opts.zero_x, opts.zero_y), opts.max_iter = (int(v) for v in win), (int(v) for v in zero_zone), int(max_iter)
    if weights is not None:
        weights = _f64(weights)
        if weights.shape != (2 * opts.win_y + 1, 2 * opts.win_x + 1):
            raise ValueError(f"weights must have the shape {(2 * opts.win_y + 1, 2 * opts.win_x + 1)}, got {weights.shape}")
    refined, status = xy.copy(), np.full(n, CORNER_INVALID, np.int32)
    iterations, tens = np.zeros(n, np.int32), np.zeros((n, 3))
    _check(lib.sba_refine_corners(device, C.c_void_p(_synced(device, frames)), B, H, W, Cn, sr, sf, _iptr(start), _dptr(xy),
                                  C.byref(opts), _dptr(weights), _dptr(refined), status.ctypes.data, iterations.ctypes.data, _dptr(tens)))
    return refined, status, iterations, tens


def _windows_out(name, a, K, B, H, W, device):
    """A caller's (K, B, H, W) uint8 output of adaptive_threshold -> (is a tensor, address, window, frame and row stride)."""
    tensor = _is_tensor(a)
    if not tensor and not (isinstance(a, np.ndarray) and a.flags.writeable):
        raise ValueError(f"{name} must be a writeable numpy array or a tensor on the device")
    if tuple(a.shape) != (K, B, H, W):
        raise ValueError(f"{name} has the shape {tuple(a.shape)}, expected {(K, B, H, W)}")
    _t, _a, _n, _H, _W, _C, sr, sf = _frame_layout(a[0], device)           # checks dtype, device and the strides inside a window
    sw = int(a.stride(0) if tensor else a.strides[0])
    if K == 1 or B * H * W == 0:
        sw = max(sw, B * sf)
    if sw < B * sf:
        raise ValueError(f"{name}: the windows must lie in ascending order, a window's frames in front of the next window's")
    return tensor, _addr(a), sw, sf, sr


def adaptive_threshold(frames, blocks, deltas, invert=True, max_value=255, channel=-1, gray_w=None, out=None, mean_out=None,
                       out_on_device=None, chunk_frames=0, device=0):
    """sba_adaptive_threshold (include/sba_hip.h): the local-mean masks of ``frames`` (as for ``detect_dots``: numpy, or a torch
    tensor on ``device`` read in place) for the K <= 4 odd window sizes ``blocks`` and integer ``deltas`` -> (masks, means), each
    (K, B, H, W) uint8 or None.  ``channel`` -1 is the grey value with ``gray_w`` (None: OpenCV's of B, G, R).  ``out``: None
    allocates the masks, False leaves them out, else the caller's array; ``mean_out``: None leaves the means out, True allocates
    them, else the caller's array.  What is allocated lies on the side the frames are on (``out_on_device`` True / False
    overrides that).  A caller's array is a writeable numpy array or a tensor on ``device`` of the shape (K, B, H, W), which may
    be a view into a larger array: its strides are the pitches, pixels contiguous, and what lies between is left untouched; when
    both are the caller's they must lie on the same side with the same strides.  ``lasercalib_amd.imaging.adaptive_threshold``
    is the public face of this call."""
    lib = load()
    tensor, frames, B, H, W, Cn, sr, sf = _frame_layout(frames, device)
    blocks = list(blocks)
    K = len(blocks)
    blocks = _int32s(blocks, K, "blocks must be 32-bit integers")
    if not 1 <= K <= ADAPTIVE_MAX_WINDOWS:
        raise ValueError(f"blocks must hold 1..{ADAPTIVE_MAX_WINDOWS} window sizes, got {K}")
    deltas = _int32s(deltas, K, f"deltas must be {K} 32-bit integers, one per window")
    opts = AdaptiveOpts()
    opts.n_windows, opts.invert, opts.max_value, opts.channel = K, 1 if invert else 0, int(max_value), int(channel)
    opts.block[:K], opts.delta[:K] = blocks, deltas
    if gray_w is not None:
        opts.gray_w = (C.c_int32 * 3)(*_int32s(gray_w, 3, "gray_w must be three 32-bit integers"))
    if out is False and mean_out is None:
        raise ValueError("neither the masks nor the means are asked for")
    given = [(n, a) for n, a in (("out", out), ("mean_out", mean_out)) if a is not None and a is not False and a is not True]
    if out is True:
        out = None
    layouts = [_windows_out(n, a, K, B, H, W, device) for n, a in given]
    if len(layouts) == 2 and (layouts[0][0] != layouts[1][0] or layouts[0][2:] != layouts[1][2:]):
        raise ValueError("out and mean_out must lie on the same side and have the same strides: the call has one set of pitches")
    if layouts:
        out_tensor, _p, sw, osf, osr = layouts[0]
    else:
        out_tensor, sw, osf, osr = tensor if out_on_device is None else bool(out_on_device), B * H * W, H * W, W

    def fresh():
        if out_tensor:
            import torch
            return torch.empty((K, B, H, W), dtype=torch.uint8, device=f"cuda:{device}")
        return np.empty((K, B, H, W), np.uint8)

    if layouts and (out is None or mean_out is True):                      # allocated beside a caller's array: in its strides
        if (sw, osf, osr) != (B * H * W, H * W, W):
            raise ValueError("out and mean_out share the pitches: pass both, or neither, when one is a view with strides")
    out = None if out is False else fresh() if out is None else out
    mean_out = fresh() if mean_out is True else mean_out
    opts.frames_on_device, opts.out_on_device, opts.chunk_frames = 1 if tensor else 0, 1 if out_tensor else 0, int(chunk_frames)
    ptr = _synced(device, frames, also=out_tensor)
    _check(lib.sba_adaptive_threshold(device, C.c_void_p(ptr), B, H, W, Cn, sr, sf, C.byref(opts), osr, osf, sw,
                                      C.c_void_p(None if out is None else _addr(out)),
                                      C.c_void_p(None if mean_out is None else _addr(mean_out))))
    return out, mean_out


class Problem:
    """One device-resident bundle-adjustment problem (wraps an sba_handle)."""

    def __init__(self, cams, pts, uv, cam_idx, pt_idx, weights=None, dtype=SBA_F64, device=0, stream=None, layout="auto"):
        """uv, cam_idx, pt_idx and weights are numpy arrays (anything numpy converts), or torch tensors on the handle's
        device (float64 / int64, contiguous): those are handed to the library as device pointers.  layout: "auto" (by size),
        "host" (the host pass) or "device" (try the device pass at any size)."""
        lib = load()
        self._lib = lib
        if layout not in LAYOUT_ROUTES:
            raise ValueError("layout must be 'auto', 'host' or 'device'")
        self.cams0, self.pts0 = _f64(cams), _f64(pts)
        named = (("points_2d", uv, "float64"), ("camera_ind", cam_idx, "int64"), ("point_ind", pt_idx, "int64"),
                 ("weights", weights, "float64"))
        tensors = [_is_tensor(a) for _n, a, _d in named if a is not None]
        on_device = any(tensors)
        if on_device and not all(tensors):
            raise ValueError("points_2d, camera_ind, point_ind and weights must be all numpy arrays or all torch tensors")
        if on_device:
            uv, ci, pi, w = (None if a is None else _device_tensor(nm, a, dt, device) for nm, a, dt in named)
            ci, pi = ci.reshape(-1), pi.reshape(-1)
            w = None if w is None else w.reshape(-1)
        else:
            uv = _f64(uv)
            ci = np.ascontiguousarray(cam_idx, dtype=np.int64).reshape(-1)
            pi = np.ascontiguousarray(pt_idx, dtype=np.int64).reshape(-1)
            w = None if weights is None else _f64(weights).reshape(-1)
        self.C, self.N, self.M = self.cams0.shape[0], self.pts0.shape[0], int(ci.shape[0])
        if self.cams0.ndim != 2 or self.cams0.shape[1] not in (11, 13):
            raise ValueError("cameraArray must have shape (n_cameras, 11) (or (n_cameras, 13) with tangential distortion)")
        self.P = self.cams0.shape[1]
        if self.pts0.ndim != 2 or self.pts0.shape[1] != 3:
            raise ValueError("points3D must have shape (n_points, 3)")
        if tuple(uv.shape) != (self.M, 2) or pi.shape[0] != self.M:
            raise ValueError("points2D must be (n_observations, 2) and index arrays (n_observations,)")
        if w is not None and w.shape[0] != self.M:
            raise ValueError("pointWeights must have one entry per observation")
        self.dtype = dtype_code(dtype)
        # stream=None: private stream.  stream=<int handle>: run on it (0 = the legacy default stream).
        desc = ProblemDesc(self.C, self.N, self.M, self.dtype, device,
                           C.c_void_p(stream) if stream else None, 0 if stream is None else 1, cam_model_of(self.P),
                           (C.c_int32 * 2)())
        h = C.c_void_p()
        _check(lib.sba_create(C.byref(desc), C.byref(h)))
        self._h = h
        opts = UploadOpts(1 if on_device else 0, LAYOUT_ROUTES[layout], (C.c_int32 * 6)())
        if on_device:
            import torch
            torch.cuda.current_stream(device).synchronize()      # the tensors are complete before the library reads them
            ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
        else:
            ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)     # noqa: E731
        try:        # (uv, ci, pi, w stay referenced until the upload has returned)
            _check(lib.sba_upload_ex(h, _dptr(self.cams0), _dptr(self.pts0), ptr(uv), ptr(ci), ptr(pi), ptr(w), C.byref(opts)), h)
        except Exception:
            self.close()
            raise

    # -- what sba_upload did, and the layout it left on the device (include/sba_hip.h)
    def upload_report(self):
        """dict: route ('host' / 'device dense' / 'device general'), decline_reason (None or a text), the layout flags, counts,
        stream_syncs and the phase seconds of the upload."""
        rep = UploadReport()
        _check(self._lib.sba_get_upload_report(self._h, C.byref(rep)), self._h)
        out = {name: getattr(rep, name) for name, _t in UploadReport._fields_ if name != "reserved"}
        out["route"] = UPLOAD_ROUTE_NAMES[rep.route]
        out["decline_reason"] = DECLINE_NAMES[rep.decline_reason]
        for k in ("dense", "masked", "group_indexed", "identity_perm"):
            out[k] = bool(out[k])
        return out

    def layout(self):
        """The layout as it lies on the device (float data widened to float64): perm, pt_start, cam_pm, pt_pm, uv_pm, w_pm,
        pt_cm, uv_cm, w_cm, cam_start, vis_mask."""
        M, N = self.M, self.N
        out = dict(perm=np.empty(M, np.int64), pt_start=np.empty(N + 1, np.int32), cam_pm=np.empty(M, np.int32),
                   pt_pm=np.empty(M, np.int32), uv_pm=np.empty((M, 2)), w_pm=np.empty(M), pt_cm=np.empty(M, np.int32),
                   uv_cm=np.empty((M, 2)), w_cm=np.empty(M), cam_start=np.empty(self.C + 1, np.int32),
                   vis_mask=np.empty(N, np.uint16))
        _check(self._lib.sba_get_layout(self._h, *[C.c_void_p(a.ctypes.data) for a in out.values()]), self._h)
        return out

    # -- multi-GPU inside the library (RCCL): after this, solve_lm runs the sharded loop on all ranks together
    def comm_init(self, unique_id, rank, n_ranks):
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("unique_id must be the 128 bytes comm_unique_id() returned on rank 0")
        _check(self._lib.sba_comm_init(self._h, bytes(unique_id), int(rank), int(n_ranks)), self._h)
        self.comm_rank, self.comm_n = int(rank), int(n_ranks)

    # -- the same sharded loop over peer-mapped buffers instead of RCCL (sba_ipc_export / sba_ipc_attach, include/sba_hip.h)
    def ipc_export(self, n_ranks):
        """This rank's exchange area for a job of n_ranks: returns the 64-byte handle every peer needs."""
        buf = C.create_string_buffer(IPC_HANDLE_BYTES)
        _check(self._lib.sba_ipc_export(self._h, int(n_ranks), buf), self._h)
        return bytes(buf.raw)

    def ipc_attach(self, rank, handles):
        """handles: the n_ranks handles in rank order (this rank's own included); after this, solve_lm runs the sharded loop."""
        if any(len(h) != IPC_HANDLE_BYTES for h in handles):
            raise ValueError("every handle must be the 64 bytes ipc_export() returned on its rank")
        _check(self._lib.sba_ipc_attach(self._h, int(rank), len(handles), b"".join(bytes(h) for h in handles)), self._h)
        self.comm_rank, self.comm_n = int(rank), len(handles)

    # -- opt-in extensions (off by default: the reference ignores points3Dfixed and uses the linear loss)
    def set_fixed_points(self, mask):
        """mask: (N,) booleans / 0-1, True = the point is held at its uploaded coordinates (gauge anchor); None clears."""
        if mask is None:
            _check(self._lib.sba_set_fixed_points(self._h, None), self._h)
            return
        m = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
        if m.shape[0] != self.N:
            raise ValueError("fixed-point mask must have one entry per 3-D point")
        _check(self._lib.sba_set_fixed_points(self._h, m.ctypes.data_as(C.c_void_p)), self._h)

    def set_robust_loss(self, loss="huber", f_scale=1.0):
        """scipy.optimize.least_squares(loss=..., f_scale=...) semantics; loss in ('linear', 'huber', 'soft_l1', 'cauchy')."""
        code = {"linear": LOSS_LINEAR, "huber": LOSS_HUBER, "soft_l1": LOSS_SOFT_L1, "cauchy": LOSS_CAUCHY}.get(loss)
        if code is None:
            raise ValueError("loss must be 'linear', 'huber', 'soft_l1' or 'cauchy'")
        _check(self._lib.sba_set_robust_loss(self._h, code, float(f_scale)), self._h)

    # -- parameter covariance at the current parameters (sba_covariance, include/sba_hip.h)
    def covariance(self, scale=True, full=False, points=True, cams_fixed=False):
        """Gauss-Newton covariance of the cameras and points; returns a Covariance (see include/sba_hip.h for the gauge)."""
        n = self.P * self.C
        cams = np.empty((self.C, self.P, self.P))
        cfull = np.empty((n, n)) if full else None
        pts = np.empty((self.N, 6)) if points else None
        rep = CovReport()
        opts = CovOpts(1 if cams_fixed else 0, 1 if scale else 0, (C.c_int32 * 6)())
        _check(self._lib.sba_covariance(self._h, C.byref(opts), _dptr(cfull), _dptr(cams), _dptr(pts), C.byref(rep)), self._h)
        pcov = None
        if pts is not None:
            pcov = pts[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(self.N, 3, 3)
        return Covariance(cams, cfull, pcov, rep)

    # -- 3-D points from the current cameras and the pixels (sba_triangulate, include/sba_hip.h)
    def triangulate(self, min_views=2, trim_px=None, max_drop=1, write_back=False):
        """Least-squares intersection of the rays of every point at the handle's current cameras; trim_px: leave-one-out
        trimming while a point's largest pixel error exceeds it (at most max_drop observations per point); write_back: the
        estimates of the OK points become the handle's current points.  Returns a Triangulation."""
        pts = np.empty((self.N, 3))
        status, n_views = np.empty(self.N, np.int32), np.empty(self.N, np.int32)
        rms, mx, spread = np.empty(self.N), np.empty(self.N), np.empty(self.N)
        inl = np.empty(self.M, np.uint8)
        rep = TriReport()
        opts = TriOpts(int(min_views), int(max_drop), float(trim_px) if trim_px else 0.0, 1 if write_back else 0, (C.c_int32 * 5)())
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))      # noqa: E731
        _check(self._lib.sba_triangulate(self._h, C.byref(opts), _dptr(pts), i32(status), i32(n_views), _dptr(rms), _dptr(mx),
                                         _dptr(spread), inl.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(rep)), self._h)
        return Triangulation(pts, status, n_views, rms, mx, spread, inl != 0, rep)

    # -- 3-D points on known planes from the current cameras and the pixels (sba_unproject, include/sba_hip.h)
    def unproject(self, planes, ref_cam=None, min_views=1, write_back=False):
        """Per point the point of its plane closest to the rays of its observations at the handle's current cameras.  planes:
        (4,) for one plane n . X = d, or (N, 4); ref_cam: only the observations of that camera (the reference's 3-D init
        camera); write_back: the estimates of the OK points become the handle's current points.  Returns an Unprojection."""
        pl = _planes(planes, self.N, "unproject")
        pts = np.empty((self.N, 3))
        status, n_views = np.empty(self.N, np.int32), np.empty(self.N, np.int32)
        rms, mx = np.empty(self.N), np.empty(self.N)
        used = np.empty(self.M, np.uint8)
        rep = UnpReport()
        opts = UnpOpts(0 if ref_cam is None else 1, 0 if ref_cam is None else int(ref_cam), int(min_views), 1 if write_back else 0,
                       (C.c_int32 * 4)())
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))      # noqa: E731
        _check(self._lib.sba_unproject(self._h, C.byref(opts), _dptr(pl), pl.shape[0], _dptr(pts), i32(status), i32(n_views),
                                       _dptr(rms), _dptr(mx), used.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(rep)), self._h)
        return Unprojection(pts, status, n_views, rms, mx, used != 0, rep)

    # -- similarity registration of the handle's current solution (sba_align, include/sba_hip.h)
    def _targets(self, name, target, weights, rows):
        if target is None:
            return None, None
        tgt = _f64(target)
        if tgt.shape != (rows, 3):
            raise ValueError(f"{name}: expected shape ({rows}, 3), got {tgt.shape}")
        w = None if weights is None else _f64(weights)
        if w is not None and w.shape != (rows,):
            raise ValueError(f"{name}: expected ({rows},) weights, got {w.shape}")
        return tgt, w

    def align(self, target_points=None, point_weights=None, target_centres=None, centre_weights=None, with_scale=True, apply=True):
        """The similarity that brings the handle's current points onto ``target_points`` (N, 3) and its camera centres onto
        ``target_centres`` (C, 3), weighted (weight 0: not used); ``apply``: every camera and point of the handle is moved
        with it, which leaves every residual where it was.  Returns an Alignment."""
        tp, pw = self._targets("target_points", target_points, point_weights, self.N)
        tc, cw = self._targets("target_centres", target_centres, centre_weights, self.C)
        rep = AlignReport()
        opts = AlignOpts(1 if with_scale else 0, 1 if apply else 0, (C.c_int32 * 6)())
        _check(self._lib.sba_align(self._h, C.byref(opts), _dptr(tp), _dptr(pw), _dptr(tc), _dptr(cw), C.byref(rep)), self._h)
        return Alignment(rep)

    def apply_similarity(self, scale, R, t):
        """Moves every camera and point of the handle by X -> scale R X + t (R: (3, 3) rotation, t: (3,))."""
        R, t = _f64(R), _f64(t)
        if R.shape != (3, 3) or t.shape != (3,):
            raise ValueError("apply_similarity: R must be (3, 3) and t (3,)")
        _check(self._lib.sba_apply_similarity(self._h, float(scale), _dptr(R), _dptr(t)), self._h)

    # -- reprojection diagnostics at the current parameters (sba_reproj_stats, include/sba_hip.h)
    def reproj_stats(self, select="all", hist_bins=None, hist_bin_px=None, grid=None, image_size=None, radial_bins=0,
                     r_max_px=None, n_worst=0, points=True, errors=False):
        """Pixel-error statistics of the handle's current solution, computed on the device from the data it already holds.
        select: "all", "used" (weight > 0) or "held_out" (weight == 0); grid: (gx, gy) cells of a residual field over an image
        of image_size = (width, height); radial_bins: bins of the radial / tangential profile out to r_max_px (default: half
        the image diagonal); n_worst: length of the worst-observation list; points: the per-point table; errors: the
        per-observation errors in the caller's order.  Returns a ReprojStats."""
        if select not in REPROJ_SELECT:
            raise ValueError("select must be 'all', 'used' or 'held_out'")
        B = REPROJ_DEFAULT_BINS if not hist_bins else int(hist_bins)
        bin_px = REPROJ_DEFAULT_BIN_PX if not hist_bin_px else float(hist_bin_px)
        gx, gy = (0, 0) if grid is None else (int(grid[0]), int(grid[1]))
        width, height = (0.0, 0.0) if image_size is None else (float(image_size[0]), float(image_size[1]))
        nr, K = int(radial_bins), int(n_worst)
        opts = ReprojOpts(REPROJ_SELECT[select], int(hist_bins or 0), float(hist_bin_px or 0.0), gx, gy, nr, K, width, height,
                          float(r_max_px or 0.0), (C.c_int32 * 6)())
        alloc = lambda ok, shape, dt=np.float64: np.empty(shape, dt) if ok else None      # noqa: E731
        ok_dims = 2 <= B <= 4096 and 0 <= gx * gy <= 256 and gx >= 0 and gy >= 0 and 0 <= nr <= 64 and 0 <= K <= 4096
        if not ok_dims:        # the library owns the error text; give it nothing to write into
            _check(self._lib.sba_reproj_stats(self._h, C.byref(opts), None, None, None, None, None, None, None, None, None), self._h)
            raise ValueError("reproj_stats: an option is out of its range")
        cam_stats, cam_hist = np.empty((self.C, 9)), np.empty((self.C, B), np.int64)
        cam_grid = alloc(gx * gy > 0, (self.C, gy, gx, 4))
        cam_radial = alloc(nr > 0, (self.C, nr, 4))
        pt_stats = alloc(points, (self.N, 3))
        err = alloc(errors, (self.M,))
        worst_idx, worst_err = np.empty(K, np.int64), np.empty(K)
        rep = ReprojReport()
        ip = lambda a: None if a is None else _iptr(a)      # noqa: E731
        _check(self._lib.sba_reproj_stats(self._h, C.byref(opts), _dptr(cam_stats), ip(cam_hist), _dptr(cam_grid), _dptr(cam_radial),
                                          _dptr(pt_stats), _dptr(err), ip(worst_idx), _dptr(worst_err), C.byref(rep)), self._h)
        r_max = float(r_max_px) if r_max_px else 0.5 * float(np.hypot(width, height))
        return ReprojStats(cam_stats, cam_hist, cam_grid, cam_radial, pt_stats, err, worst_idx, worst_err, rep, bin_px, r_max)

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None):
            self._lib.sba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def n_params(self):
        return self.P * self.C + 3 * self.N

    # -- model evaluation
    def residual(self, x=None, want_r=True):
        r = np.empty(2 * self.M) if want_r else None
        cost = C.c_double()
        xx = None if x is None else _f64(x)
        _check(self._lib.sba_residual(self._h, _dptr(xx), _dptr(r), C.byref(cost)), self._h)
        return r, cost.value

    def residual_jacobian(self, x=None):
        r = np.empty(2 * self.M)
        Jc = np.empty((self.M, 2, self.P))
        Jp = np.empty((self.M, 2, 3))
        xx = None if x is None else _f64(x)
        _check(self._lib.sba_residual_jacobian(self._h, _dptr(xx), _dptr(r), _dptr(Jc), _dptr(Jp)), self._h)
        return r, Jc, Jp

    def set_params(self, x):
        _check(self._lib.sba_set_params(self._h, _dptr(_f64(x))), self._h)

    def get_params(self):
        cams = np.empty((self.C, self.P))
        pts = np.empty((self.N, 3))
        _check(self._lib.sba_get_params(self._h, _dptr(cams), _dptr(pts)), self._h)
        return cams, pts

    def get_gradient(self):
        gc = np.empty((self.C, self.P))
        gp = np.empty((self.N, 3))
        _check(self._lib.sba_get_gradient(self._h, _dptr(gc), _dptr(gp)), self._h)
        return gc, gp

    def get_transform(self):
        th = np.empty(12)
        _check(self._lib.sba_get_transform(self._h, _dptr(th)), self._h)
        return th

    # -- solver
    @staticmethod
    def make_opts(ftol=1e-8, xtol=1e-8, gtol=1e-8, max_nfev=0, mode=MODE_FULL, verbose=0, max_iter=0,
                  always_relinearize=False, lambda0=0.0, profile=False):
        return LmOpts(ftol, xtol, gtol, int(max_nfev or 0), mode, verbose, int(max_iter or 0),
                      1 if always_relinearize else 0, float(lambda0), (C.c_int32 * 4)(1 if profile else 0, 0, 0, 0))

    def solve_lm(self, opts, log_capacity=4096):
        cams = np.empty((self.C, self.P))
        pts = np.empty((self.N, 3))
        rep = LmReport()
        log = (LmIterLog * log_capacity)()
        rows = C.c_int32(0)
        _check(self._lib.sba_solve_lm(self._h, C.byref(opts), _dptr(cams), _dptr(pts), C.byref(rep), log,
                                      log_capacity, C.byref(rows)), self._h)
        return cams, pts, rep, [log[i] for i in range(min(rows.value, log_capacity))]

    # -- phase-level API (multi-GPU driver)
    def exchange_size(self):
        return int(self._lib.sba_lm_exchange_size(self._h))

    def lm_begin(self, opts):
        _check(self._lib.sba_lm_begin(self._h, C.byref(opts)), self._h)

    def lm_linearize(self):
        _check(self._lib.sba_lm_linearize(self._h), self._h)

    def lm_form_reduced(self, exchange_ptr):
        _check(self._lib.sba_lm_form_reduced(self._h, C.c_void_p(exchange_ptr)), self._h)

    def lm_solve_trial(self, exchange_ptr, scalars_ptr):
        _check(self._lib.sba_lm_solve_trial(self._h, C.c_void_p(exchange_ptr), C.c_void_p(scalars_ptr)), self._h)

    def lm_get_step(self):
        """delta_c of the last lm_solve_trial (test hook for the reduced-system factorisations)."""
        d = np.empty((self.C, self.P))
        _check(self._lib.sba_lm_get_step(self._h, _dptr(d)), self._h)
        return d

    def lm_decide(self, scalars_all_ptr, n_ranks):
        status, acc = C.c_int32(), C.c_int32()
        row = LmIterLog()
        _check(self._lib.sba_lm_decide(self._h, C.c_void_p(scalars_all_ptr), n_ranks, C.byref(status),
                                       C.byref(acc), C.byref(row)), self._h)
        return status.value, bool(acc.value), row

    def lm_decide_async(self, scalars_all_ptr, n_ranks):
        _check(self._lib.sba_lm_decide_async(self._h, C.c_void_p(scalars_all_ptr), n_ranks), self._h)

    def lm_poll(self):
        status, iters = C.c_int32(), C.c_int32()
        _check(self._lib.sba_lm_poll(self._h, C.byref(status), C.byref(iters)), self._h)
        return status.value, iters.value

    def lm_run(self):
        """The iteration loop of solve_lm alone (between lm_begin and lm_finish); returns (status, iterations)."""
        status, iters = C.c_int32(), C.c_int32()
        _check(self._lib.sba_lm_run(self._h, C.byref(status), C.byref(iters)), self._h)
        return status.value, iters.value

    def lm_finish(self):
        cams = np.empty((self.C, self.P))
        pts = np.empty((self.N, 3))
        rep = LmReport()
        _check(self._lib.sba_lm_finish(self._h, _dptr(cams), _dptr(pts), C.byref(rep)), self._h)
        return cams, pts, rep

    def iteration_log(self, capacity=4096):
        log = (LmIterLog * capacity)()
        rows = C.c_int32(0)
        _check(self._lib.sba_lm_get_log(self._h, log, capacity, C.byref(rows)), self._h)
        return [log[i] for i in range(min(rows.value, capacity))]

    # -- measurement
    PROFILE_SLOTS = ("linearize_points", "linearize_cams", "schur", "schur_reduce", "cholesky_solve", "backsub")

    def kernel_profile(self):
        """Mean in-loop duration (us) per kernel class of the last solve run with profile=True."""
        tot = np.zeros(len(self.PROFILE_SLOTS))
        cnt = np.zeros(len(self.PROFILE_SLOTS), dtype=np.int64)
        _check(self._lib.sba_get_kernel_profile(self._h, _dptr(tot), _iptr(cnt)), self._h)
        return {k: (tot[i] / cnt[i] if cnt[i] else 0.0) for i, k in enumerate(self.PROFILE_SLOTS)}

    def time_kernel(self, name, reps=20):
        us = C.c_double()
        _check(self._lib.sba_time_kernel(self._h, name.encode(), reps, C.byref(us)), self._h)
        return us.value
