"""ctypes binding of libcerebro_hip.so (include/cerebro_hip.h).

Plumbing only: every compute call goes through the C-ABI into the HIP kernels.  There is NO CPU
fallback -- if the shared library is missing or a call fails, a ChipError is raised.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
PRODUCT_LIB_PATH = _HERE / "lib" / "libcerebro_hip.so"
HOOKS_LIB_PATH = _HERE / "lib" / "hooks" / "libcerebro_hip.so"    # the TEST build (-DCHIP_TEST_HOOKS, `make testlibs`): fault injection; tests only


def _lib_path() -> Path:
    """CHIP_LIB=<path> loads another build of the library (same-box A/B runs, the degraded and the test builds) -- but only together with
    CHIP_ALLOW_LIB_OVERRIDE=1: a stray CHIP_LIB must not redirect a deployed process to some other .so."""
    override = os.environ.get("CHIP_LIB")
    if override:
        if os.environ.get("CHIP_ALLOW_LIB_OVERRIDE") == "1":
            return Path(override).resolve()
        sys.stderr.write(f"[cerebro_amd] CHIP_LIB={override} IGNORED: set CHIP_ALLOW_LIB_OVERRIDE=1 to load another build of the library\n")
    return PRODUCT_LIB_PATH


LIB_PATH = _lib_path()

CHIP_OK = 0
CHIP_ERR_INVALID_ARG = -1
CHIP_ERR_NO_DEVICE = -2
CHIP_ERR_HIP = -3
CHIP_ERR_OOM = -4
CHIP_ERR_NOT_F32 = -5
CHIP_ERR_NONFINITE = -6
CHIP_ERR_RANGE = -7
CHIP_ERR_UNSUPPORTED = -8
CHIP_ERR_TOO_FEW_POINTS = -9
CHIP_ERR_BUSY = -10
CHIP_ERR_COMM = -11
CHIP_ERR_SHARD_FAILED = -12
CHIP_ERR_GROUP_BROKEN = -13

CHIP_MAX_TOPK = 16
CHIP_MAX_NQ = 4
CHIP_DEFAULT_TOPK = 8
CHIP_RING_ROWS = 4096
CHIP_MAX_INFLIGHT = 64
CHIP_APPEND_ALLOW_ROUNDING = 1
CHIP_CREATE_STORE_F32 = 1
CHIP_CREATE_STORE_F64 = 2
CHIP_MULTI_EXCHANGE_COPY = 4
CHIP_COMM_ID_BYTES = 128
CHIP_EXCHANGE_NONE, CHIP_EXCHANGE_RCCL, CHIP_EXCHANGE_COPY = 0, 1, 2
CHIP_SCAN_FORM_ONE_ROW, CHIP_SCAN_FORM_ROWS = 1, 2
CHIP_SAMPLER_FRESH, CHIP_SAMPLER_THEIA_PERSISTENT = 0, 1
CHIP_RANSAC_LEG_PNP, CHIP_RANSAC_LEG_ICP = 0, 1
CHIP_SCAN_FAMILY_NONE, CHIP_SCAN_FAMILY_ONE_ROW, CHIP_SCAN_FAMILY_WIDE, CHIP_SCAN_FAMILY_ROWS, CHIP_SCAN_FAMILY_MULTI = 0, 1, 2, 3, 4
CHIP_SCAN_CALL_QUERY, CHIP_SCAN_CALL_TICK, CHIP_SCAN_CALL_TICK_SYNC = 0, 1, 2
SCAN_FAMILY_NAMES = {0: "none", 1: "one_row", 2: "wide", 3: "rows", 4: "multi", 5: "prefilter", 6: "halfq"}

CHIP_TICK_SKIPPED, CHIP_TICK_TOO_SHORT, CHIP_TICK_SCANNED = 0, 1, 2
CHIP_MATCH_MAX_KEYPOINTS = 16384
CHIP_MATCH_MAX_BATCH = 16
CHIP_MATCH_MAX_PAIRS = CHIP_MATCH_MAX_BATCH
CHIP_ICP_MAX_BATCH = 16
CHIP_ORB_DESC_BYTES = 32
CHIP_SET_AB, CHIP_SET_BA = 0, 1
CHIP_DISP_S16, CHIP_DISP_F32 = 0, 1
# chip_stereo_bm_params' defaults: cv::StereoBM::create(64, 21)
CHIP_STEREO_BM_NUM_DISPARITIES, CHIP_STEREO_BM_BLOCK_SIZE, CHIP_STEREO_BM_PREFILTER_CAP = 64, 21, 31
CHIP_STEREO_BM_TEXTURE_THRESHOLD, CHIP_STEREO_BM_UNIQUENESS_RATIO = 10, 15
# chip_orb_params' defaults: cv::ORB::create(5000) with setFastThreshold(0)
CHIP_ORB_MAX_LEVELS, CHIP_ORB_MAX_SIDE = 8, 4096
CHIP_ORB_BINS = 32
CHIP_ORB_N_FEATURES, CHIP_ORB_N_LEVELS, CHIP_ORB_FAST_THRESHOLD, CHIP_ORB_BORDER = 5000, 8, 0, 31
# rectification: map values are quantised to 1/32 pixel (5 fraction bits) inside [-2, 32768]; NaN gives -64
CHIP_RECTIFY_FRACTION_BITS, CHIP_RECTIFY_MAP_MIN, CHIP_RECTIFY_MAP_MAX, CHIP_RECTIFY_NAN_Q = 5, -2.0, 32768.0, -64
# descriptor projection: the matrix's element type; in_dim % 256 == 0, 256 <= in_dim <= CHIP_PROJ_MAX_IN_DIM
CHIP_PROJ_F32, CHIP_PROJ_F64, CHIP_PROJ_MAX_IN_DIM = 1, 2, 32768
# NetVLAD pooling: the layout of a feature map, the positions per aggregation block (part of the definition), the most positions
CHIP_VLAD_NHWC, CHIP_VLAD_NCHW, CHIP_VLAD_BLOCK, CHIP_VLAD_MAX_POSITIONS = 1, 2, 64, 16384


class ChipError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        super().__init__(f"{where}: status {status} ({_strerror(status)}){' -- ' + detail if detail else ''}")


class DotParams(C.Structure):
    _fields_ = [("locality", C.c_int32), ("lag", C.c_int32), ("min_new", C.c_int32), ("min_k", C.c_int32),
                ("thresh", C.c_double)]


class TickResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("found", C.c_int32), ("idx_curr", C.c_int64), ("idx_prev", C.c_int64),
                ("score", C.c_double), ("argmax", C.c_int64 * 3), ("maxv", C.c_double * 3)]

    def as_dict(self):
        return dict(status=self.status, found=self.found, idx_curr=self.idx_curr, idx_prev=self.idx_prev,
                    score=self.score, argmax=list(self.argmax), maxv=list(self.maxv))


class TopkEntry(C.Structure):
    _fields_ = [("score", C.c_double), ("idx", C.c_int64)]


class RansacParams(C.Structure):
    _fields_ = [("error_thresh", C.c_double), ("min_inlier_ratio", C.c_double), ("max_iterations", C.c_int32),
                ("min_iterations", C.c_int32), ("use_mle", C.c_int32), ("sample_size", C.c_int32),
                ("failure_probability", C.c_double), ("seed", C.c_uint64), ("n_hypotheses", C.c_int32),
                ("sampler", C.c_int32)]


class RansacSummary(C.Structure):
    _fields_ = [("n_iterations", C.c_int32), ("n_inliers", C.c_int32), ("best_hypothesis", C.c_int32),
                ("n_models", C.c_int32), ("best_cost", C.c_double)]


class StereoBmParams(C.Structure):
    _fields_ = [("num_disparities", C.c_int32), ("block_size", C.c_int32), ("prefilter_cap", C.c_int32),
                ("texture_threshold", C.c_int32), ("uniqueness_ratio", C.c_int32)]


class OrbParams(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("n_levels", C.c_int32), ("fast_threshold", C.c_int32), ("border", C.c_int32)]


class OrbKeypoint(C.Structure):
    _fields_ = [("response", C.c_int64), ("x", C.c_float), ("y", C.c_float), ("m10", C.c_int32), ("m01", C.c_int32),
                ("x_level", C.c_uint16), ("y_level", C.c_uint16), ("level", C.c_uint16), ("zero", C.c_uint16)]


class OrbLevel(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("quota", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32),
                ("x1", C.c_int32), ("y1", C.c_int32), ("scale", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# chip_orb_keypoint as a numpy record
ORB_KEYPOINT_DTYPE = np.dtype([("response", "<i8"), ("x", "<f4"), ("y", "<f4"), ("m10", "<i4"), ("m01", "<i4"), ("x_level", "<u2"),
                               ("y_level", "<u2"), ("level", "<u2"), ("zero", "<u2")])


class MatchFrame(C.Structure):
    _fields_ = [("desc", C.c_void_p), ("kp_xy", C.c_void_p), ("n", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("xyz", C.c_void_p)]


class MatchSummary(C.Structure):
    _fields_ = [("n_matches_all", C.c_int32), ("n_matches_gms", C.c_int32), ("n_3d2d_ab", C.c_int32), ("n_3d2d_ba", C.c_int32),
                ("n_3d3d", C.c_int32), ("n_out_of_image", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


CHIP_GMS_WITH_SCALE, CHIP_GMS_WITH_ROTATION = 1, 2


class GmsChoice(C.Structure):
    """chip_gms_choice: which (scale index, rotation type) GMS with scale / rotation kept, and the inlier count of every hypothesis"""
    _fields_ = [("scale", C.c_int32), ("rotation", C.c_int32), ("n_inliers", C.c_int32), ("counts", (C.c_int32 * 8) * 5)]

    def as_dict(self):
        return dict(scale=self.scale, rotation=self.rotation, n_inliers=self.n_inliers,
                    counts=np.array([list(row) for row in self.counts], dtype=np.int32))


class MatchSetsOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("uv", "uv_d", "X_ab", "uvn_ab", "X_ba", "uvn_ba", "A_3d3d", "B_3d3d",
                                          "match_query_idx", "match_train_idx")]


class ScanLaunch(C.Structure):
    """chip_debug_scan_launch: which kernel a top-k scan launch is (test aid)"""
    _fields_ = [(n, C.c_int32) for n in ("family", "elem", "nq", "K", "U", "NT", "FULL", "NG", "R", "NTL", "ticks", "q64", "claimed", "fused",
                                         "grid", "block", "wg_per_cu", "lds_bytes")] + [("n_rows", C.c_int64), ("launches", C.c_int64)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_}
        d["family"] = SCAN_FAMILY_NAMES[d["family"]]
        return d


class PassInfo(C.Structure):
    """chip_debug_pass_info: what the last prefilter pass was launched with (test aid)"""
    _fields_ = [(n, C.c_int32) for n in ("family", "ticks", "grid", "wpb", "K", "e")] + [("k", C.c_int64 * 5), ("E", C.c_double)]


class RansacShape(C.Structure):
    """chip_debug_ransac_shape: the launch a per-hypothesis record belongs to (test aid)"""
    _fields_ = [(n, C.c_int32) for n in ("P", "H", "N", "words", "S", "sampler")]


class Info(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("D", C.c_int32), ("device", C.c_int32), ("shard_rank", C.c_int32),
                ("shard_count", C.c_int32), ("n_cus", C.c_int32), ("rows_global", C.c_int64),
                ("rows_local", C.c_int64), ("capacity_local", C.c_int64), ("lossy_rows", C.c_int64),
                ("arch", C.c_char * 32), ("storage_bytes", C.c_int32), ("n_devices", C.c_int32), ("exchange", C.c_int32),
                ("comm_ranks", C.c_int32), ("comm_init_abandoned", C.c_int32), ("scan_forms", C.c_int32), ("test_hooks", C.c_int32),
                ("row_norm_max", C.c_double)]


# every symbol include/cerebro_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_SIGS = {
    "chip_strerror": (C.c_char_p, [C.c_int]),
    "chip_abi_version": (C.c_int, []),
    "chip_build_scan_forms": (C.c_int, []),
    "chip_build_test_hooks": (C.c_int, []),
    "chip_last_hip_error": (C.c_int, [_P, C.POINTER(C.c_char_p)]),
    "chip_last_comm_error": (C.c_int, [_P, C.POINTER(C.c_char_p)]),
    "chip_create": (C.c_int, [C.POINTER(_P), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "chip_create_ex": (C.c_int, [C.POINTER(_P), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_uint32]),
    "chip_create_multi": (C.c_int, [C.POINTER(_P), C.c_int32, C.c_int64, _P, C.c_int32, C.c_uint32]),
    "chip_comm_unique_id": (C.c_int, [_P]),
    "chip_comm_init_rank": (C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    "chip_destroy": (None, [_P]),
    "chip_set_stream": (C.c_int, [_P, _P]),
    "chip_reset_stream": (C.c_int, [_P]),
    "chip_synchronize": (C.c_int, [_P]),
    "chip_db_append_f64": (C.c_int, [_P, _P, C.c_int64, C.c_uint32, C.POINTER(C.c_int64)]),
    "chip_db_append_f32": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "chip_db_size": (C.c_int64, [_P]),
    "chip_db_read_rows_f32": (C.c_int, [_P, _P, C.c_int64, _P]),
    "chip_db_read_rows_f64": (C.c_int, [_P, _P, C.c_int64, _P]),
    "chip_db_append_synthetic": (C.c_int, [_P, C.c_int64, C.c_uint64, _P, _P, _P, C.c_int64]),
    "chip_db_append_synthetic_unit": (C.c_int, [_P, C.c_int64, C.c_uint64, _P, _P, _P, C.c_int64]),
    "chip_query_rows": (C.c_int, [_P, C.c_int64, _P, C.c_int32, C.c_int32, _P, _P]),
    "chip_query_vectors_f32": (C.c_int, [_P, C.c_int64, _P, C.c_int32, C.c_int32, _P, _P]),
    "chip_query_vectors_f64": (C.c_int, [_P, C.c_int64, _P, C.c_int32, C.c_int32, _P, _P]),
    "chip_query_scores": (C.c_int, [_P, C.c_int64, C.c_int64, _P]),
    "chip_query_batch_f32": (C.c_int, [_P, C.c_int64, _P, C.c_int32, C.c_int32, _P, _P]),
    "chip_query_batch_cast_f32": (C.c_int, [_P, C.c_int64, _P, C.c_int32, C.c_int32, _P, _P]),
    "chip_build_has_query_prefix": (C.c_int, []),
    "chip_query_batch_rows_f32": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    "chip_query_batch_rows_cast_f32": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    "chip_query_batch_prefix_f32": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    "chip_query_batch_prefix_cast_f32": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    "chip_query_prefix_plan": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "chip_debug_query_prefix_last": (C.c_int, [_P, _P]),
    "chip_build_has_bulk_ticks": (C.c_int, []),
    "chip_loop_ticks_bulk": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int64, C.c_int32, _P, _P, _P, _P]),
    "chip_bulk_ticks_plan": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.c_int64, _P, _P, _P]),
    "chip_debug_bulk_ticks_last": (C.c_int, [_P, _P]),
    "chip_dot_params_default": (None, [C.POINTER(DotParams)]),
    "chip_loop_tick": (C.c_int, [_P, C.c_int64, C.POINTER(DotParams), C.POINTER(TickResult)]),
    "chip_resident_pause": (C.c_int, [_P]),
    "chip_resident_resume": (C.c_int, [_P]),
    "chip_loop_tick_enqueue": (C.c_int, [_P, C.c_int64, C.POINTER(DotParams), C.c_int32]),
    "chip_loop_tick_collect": (C.c_int, [_P, C.c_int32, C.POINTER(TickResult)]),
    "chip_loop_last_l": (C.c_int64, [_P]),
    "chip_loop_reset": (None, [_P]),
    "chip_scan_local": (C.c_int, [_P, C.c_int64, C.POINTER(DotParams), C.c_int32, _P, C.POINTER(C.c_int32)]),
    "chip_merge_decide": (C.c_int, [_P, C.c_int64, C.POINTER(DotParams), _P, C.c_int32, C.c_int32, C.POINTER(TickResult)]),
    "chip_merge_decide_enqueue": (C.c_int, [_P, C.c_int64, C.POINTER(DotParams), _P, C.c_int32, C.c_int32, C.c_int32]),
    "chip_debug_merge_lists": (C.c_int, [_P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64, C.POINTER(DotParams),
                                         C.POINTER(TickResult)]),
    "chip_debug_last_pass": (C.c_int, [_P, C.POINTER(PassInfo), _P, _P, _P]),
    "chip_ransac_params_default": (None, [C.POINTER(RansacParams)]),
    "chip_pnp_ransac": (C.c_int, [_P, _P, _P, C.c_int32, C.POINTER(RansacParams), _P, C.POINTER(C.c_float), _P,
                                  C.POINTER(RansacSummary)]),
    "chip_pnp_ransac_batch": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.POINTER(RansacParams), _P, _P, _P, _P, _P]),
    "chip_icp_params_default": (None, [C.POINTER(RansacParams)]),
    "chip_icp_ransac": (C.c_int, [_P, _P, _P, C.c_int32, C.POINTER(RansacParams), _P, C.POINTER(C.c_float), _P,
                                  C.POINTER(RansacSummary)]),
    "chip_icp_ransac_enqueue": (C.c_int, [_P, _P, _P, C.c_int32, C.POINTER(RansacParams)]),
    "chip_icp_ransac_collect": (C.c_int, [_P, _P, C.POINTER(C.c_float), _P, C.POINTER(RansacSummary)]),
    "chip_build_has_icp_batch": (C.c_int, []),
    "chip_icp_ransac_batch": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.POINTER(RansacParams), _P, _P, _P, _P, _P]),
    "chip_debug_ransac_record": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(RansacShape), _P, _P, _P, _P, _P, _P, _P]),
    "chip_debug_pnp_stage": (C.c_int, [_P, C.c_int32, _P, _P, _P]),
    "chip_debug_pnp_keep_stage": (C.c_int, [_P, C.c_int32]),
    "chip_build_has_match": (C.c_int, []),
    "chip_build_has_tick_coalesce": (C.c_int, []),
    "chip_debug_coalesce_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "chip_debug_coalesce_force": (C.c_int, [_P, C.c_int32]),
    "chip_debug_coalesce_decide": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "chip_debug_last_scan": (C.c_int, [_P, C.POINTER(ScanLaunch)]),
    "chip_debug_scan_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(ScanLaunch)]),
    "chip_debug_multi_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(ScanLaunch)]),
    "chip_debug_prefilter_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(ScanLaunch)]),
    "chip_debug_halfq_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(ScanLaunch)]),
    "chip_debug_halfq_bound": (C.c_int, [C.c_int32, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "chip_debug_prefilter_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "chip_orb_match": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, _P]),
    "chip_gms_filter": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P,
                                  C.POINTER(C.c_int32)]),
    "chip_match_pair": (C.c_int, [_P, C.POINTER(MatchFrame), C.POINTER(MatchFrame), _P, C.POINTER(MatchSummary)]),
    "chip_match_read_sets": (C.c_int, [_P, C.POINTER(MatchSetsOut)]),
    "chip_pnp_ransac_matched": (C.c_int, [_P, C.c_int32, C.POINTER(RansacParams), _P, C.POINTER(C.c_float), _P, C.POINTER(RansacSummary)]),
    "chip_icp_ransac_matched": (C.c_int, [_P, C.POINTER(RansacParams), _P, C.POINTER(C.c_float), _P, C.POINTER(RansacSummary)]),
    "chip_build_has_gms_modes": (C.c_int, []),
    "chip_gms_filter_modes": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32,
                                        C.c_uint32, _P, C.POINTER(C.c_int32), C.POINTER(GmsChoice)]),
    "chip_match_batch_modes": (C.c_int, [_P, C.POINTER(MatchFrame), C.POINTER(MatchFrame), C.c_int32, _P, C.c_uint32, C.POINTER(MatchSummary),
                                         C.POINTER(GmsChoice)]),
    "chip_match_batch_stored_modes": (C.c_int, [_P, C.c_int64, _P, C.c_int32, _P, C.c_uint32, C.POINTER(MatchSummary), C.POINTER(GmsChoice)]),
    "chip_build_has_match_batch": (C.c_int, []),
    "chip_match_batch": (C.c_int, [_P, C.POINTER(MatchFrame), C.POINTER(MatchFrame), C.c_int32, _P, C.POINTER(MatchSummary)]),
    "chip_match_select": (C.c_int, [_P, C.c_int32]),
    "chip_match_batch_read_matches": (C.c_int, [_P, C.c_int32, _P, _P]),
    "chip_pnp_ransac_matched_batch": (C.c_int, [_P, C.c_int32, _P, _P, C.POINTER(RansacParams), _P, _P, _P, _P, _P, _P]),
    "chip_icp_ransac_matched_batch_enqueue": (C.c_int, [_P, C.c_int32, _P, C.POINTER(RansacParams), _P, _P]),
    "chip_icp_ransac_matched_batch_collect": (C.c_int, [_P, _P, _P, _P, _P]),
    "chip_icp_ransac_matched_batch": (C.c_int, [_P, C.c_int32, _P, C.POINTER(RansacParams), _P, _P, _P, _P, _P, _P]),
    "chip_build_has_frame_store": (C.c_int, []),
    "chip_frame_store_reserve": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "chip_frame_store_info": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "chip_frame_put": (C.c_int, [_P, C.c_int64, C.POINTER(MatchFrame)]),
    "chip_frame_drop": (C.c_int, [_P, C.c_int64]),
    "chip_frame_read": (C.c_int, [_P, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _P, _P]),
    "chip_match_batch_stored": (C.c_int, [_P, C.c_int64, _P, C.c_int32, _P, C.POINTER(MatchSummary)]),
    "chip_build_has_match_pairs": (C.c_int, []),
    "chip_match_pairs_stored": (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_uint32, C.POINTER(MatchSummary), C.POINTER(GmsChoice)]),
    "chip_build_has_disparity": (C.c_int, []),
    "chip_frame_put_disparity": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    "chip_disparity_to_xyz": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "chip_stereo_bm_params_default": (None, [C.POINTER(StereoBmParams)]),
    "chip_build_has_stereo_bm": (C.c_int, []),
    "chip_stereo_bm": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.POINTER(StereoBmParams), _P]),
    "chip_frame_put_stereo": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.POINTER(StereoBmParams), _P]),
    "chip_orb_params_default": (None, [C.POINTER(OrbParams)]),
    "chip_build_has_orb_detect": (C.c_int, []),
    "chip_orb_plan": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(OrbParams), C.POINTER(OrbLevel)]),
    "chip_orb_detect": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(OrbParams), _P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "chip_debug_orb_level": (C.c_int, [_P, C.c_int32, _P, _P]),
    "chip_build_has_orb_describe": (C.c_int, []),
    "chip_orb_bin": (C.c_int, [C.c_int32, C.c_int32]),
    "chip_orb_pattern": (C.c_int, [_P, _P]),
    "chip_orb_detect_describe": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(OrbParams), _P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                           _P]),
    "chip_debug_orb_blur": (C.c_int, [_P, C.c_int32, _P]),
    "chip_frame_put_orb_stereo": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, _P, C.POINTER(OrbParams), C.POINTER(StereoBmParams), _P,
                                            C.POINTER(C.c_int32)]),
    "chip_build_has_rectify": (C.c_int, []),
    "chip_rectify_quantize": (C.c_int, [_P, C.c_int64, _P]),
    "chip_remap": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "chip_rectify_set_maps": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "chip_rectify_pair": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    "chip_frame_put_raw_orb_stereo": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, _P, C.POINTER(OrbParams), C.POINTER(StereoBmParams), _P,
                                                C.POINTER(C.c_int32)]),
    "chip_build_has_frame_put_batch": (C.c_int, []),
    "chip_frame_put_plan": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(OrbParams), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "chip_frame_put_orb_stereo_batch": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.POINTER(OrbParams), C.POINTER(StereoBmParams), _P,
                                                  _P]),
    "chip_frame_put_raw_orb_stereo_batch": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.POINTER(OrbParams),
                                                      C.POINTER(StereoBmParams), _P, _P]),
    "chip_frame_put_records": (C.c_int, [_P, C.c_int64, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
    "chip_debug_frame_put_last": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "chip_build_has_project": (C.c_int, []),
    "chip_project_set": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P]),
    "chip_project_clear": (C.c_int, [_P]),
    "chip_project_info": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "chip_project": (C.c_int, [_P, _P, C.c_int64, _P]),
    "chip_db_append_projected_f32": (C.c_int, [_P, _P, C.c_int64, C.c_uint32, C.POINTER(C.c_int64)]),
    "chip_build_has_vlad": (C.c_int, []),
    "chip_vlad_set": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "chip_vlad_clear": (C.c_int, [_P]),
    "chip_vlad_info": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "chip_vlad": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    "chip_db_append_vlad_f32": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_int64)]),
    "chip_debug_vlad_stage": (C.c_int, [_P, _P, _P, _P]),
    "chip_project_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, _P]),
    "chip_debug_project_last": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "chip_vlad_batch": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "chip_db_append_vlad_batch_f32": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_int64)]),
    "chip_get_info": (C.c_int, [_P, C.POINTER(Info)]),
    "chip_profile_enable": (C.c_int, [_P, C.c_int32]),
    "chip_profile_reset": (C.c_int, [_P]),
    "chip_profile_scan": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}

_lib = None


def load_library(path: os.PathLike | None = None) -> C.CDLL:
    """Load libcerebro_hip.so and bind every declared symbol.  Raises if the library or a symbol is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else LIB_PATH
    # One HIP runtime per process.  The torch wheel bundles its own libamdhip64 (SONAME libamdhip64.so.7 but
    # NEEDED by file name), so a torch imported AFTER this library maps a second runtime that sees no GPUs.
    # When torch is installed, let it load its runtime first; this library then binds to the same one.
    if p.exists() and "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except Exception:  # torch absent: the system ROCm runtime is used
            pass
    if not p.exists():
        raise FileNotFoundError(
            f"{p} not found: the HIP extension is not built. Run `make lib` (or __graft_entry__.build()). "
            "cerebro_amd has no CPU fallback.")
    lib = C.CDLL(str(p))
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


class use_hooks_library:
    """Context manager for tests/: Chip objects created inside it run on the TEST build of the library (lib/hooks/, fault-injection hooks
    compiled in); outside it -- and in every product path -- the product build, which has none.  Both builds may be mapped in one process
    (RTLD_LOCAL; each registers its own code objects)."""

    def __enter__(self):
        global _lib
        self.saved = _lib
        lib = load_library(HOOKS_LIB_PATH)
        if lib.chip_build_test_hooks() != 1:
            raise RuntimeError(f"{HOOKS_LIB_PATH} is not a -DCHIP_TEST_HOOKS build")
        _lib = lib
        return lib

    def __exit__(self, *exc):
        global _lib
        _lib = self.saved
        return False


def declared_symbols():
    return sorted(_SIGS)


def _strerror(status: int) -> str:
    try:
        return load_library().chip_strerror(status).decode()
    except Exception:  # pragma: no cover
        return "?"


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def default_dot_params() -> DotParams:
    p = DotParams()
    load_library().chip_dot_params_default(C.byref(p))
    return p


def default_stereo_bm_params(**fields) -> StereoBmParams:
    """chip_stereo_bm_params_default, with the given fields replaced"""
    p = StereoBmParams()
    load_library().chip_stereo_bm_params_default(C.byref(p))
    for k, v in fields.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def default_orb_params(**fields) -> OrbParams:
    """chip_orb_params_default, with the given fields replaced"""
    p = OrbParams()
    load_library().chip_orb_params_default(C.byref(p))
    for k, v in fields.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _orb_params(params):
    """a parameter pointer or None from an OrbParams, a dict of its fields or None"""
    if isinstance(params, dict):
        params = default_orb_params(**params)
    return params, (None if params is None else C.byref(params))


def orb_bin(m10: int, m01: int) -> int:
    """chip_orb_bin: the orientation bin (0 .. 31) of a keypoint's moments; no ctx, no device"""
    return int(load_library().chip_orb_bin(m10, m01))


def orb_pattern():
    """chip_orb_pattern -> (the (256, 4) int8 pairs x1, y1, x2, y2, the (32, 256, 4) int8 steered table); no ctx, no device"""
    pattern, steered = np.zeros((256, 4), dtype=np.int8), np.zeros((CHIP_ORB_BINS, 256, 4), dtype=np.int8)
    rc = load_library().chip_orb_pattern(_ptr(pattern), _ptr(steered))
    if rc != CHIP_OK:
        raise ChipError(rc, "chip_orb_pattern")
    return pattern, steered


def rectify_quantize(map) -> np.ndarray:
    """chip_rectify_quantize: the float map values in 1/32 pixel -> an int32 array of the map's shape; no ctx, no device"""
    m = np.ascontiguousarray(map, dtype=np.float32)
    q = np.zeros(m.shape, dtype=np.int32)
    rc = load_library().chip_rectify_quantize(_ptr(m), m.size, _ptr(q))
    if rc != CHIP_OK:
        raise ChipError(rc, "chip_rectify_quantize")
    return q


def frame_put_plan(width: int, height: int, F: int, params=None, raw: bool = False) -> dict:
    """chip_frame_put_plan -> dict(group, n_groups): how a batched put of F pairs of this size is walked (no ctx, no device)"""
    _, o = _orb_params(params)
    g, n = C.c_int32(), C.c_int32()
    rc = load_library().chip_frame_put_plan(width, height, o, int(raw), F, C.byref(g), C.byref(n))
    if rc != CHIP_OK:
        raise ChipError(rc, "chip_frame_put_plan")
    return dict(group=g.value, n_groups=n.value)


def orb_plan(width: int, height: int, params=None) -> list:
    """chip_orb_plan -> the level table of a detect on a width x height image: n_levels dicts (width, height, quota, x0, y0, x1, y1,
    scale).  Needs no ctx and no device."""
    params, p = _orb_params(params)
    lv = (OrbLevel * CHIP_ORB_MAX_LEVELS)()
    rc = load_library().chip_orb_plan(width, height, p, lv)
    if rc != CHIP_OK:
        raise ChipError(rc, "chip_orb_plan")
    n = CHIP_ORB_N_LEVELS if params is None else params.n_levels
    return [lv[l].as_dict() for l in range(n)]


class ProjectPlan(C.Structure):
    """chip_project_plan_out"""
    _fields_ = [("width", C.c_int32), ("slab", C.c_int32), ("lds_bytes", C.c_int32), ("single_lds_bytes", C.c_int32), ("block", C.c_int32),
                ("reserved", C.c_int32), ("passes", C.c_int64), ("shared_passes", C.c_int64), ("single_launches", C.c_int64)]


def project_plan(in_dim: int, matrix_type: int, n: int) -> dict:
    """chip_project_plan -> what a projecting call over n descriptors launches: width, passes (= shared_passes + single_launches), slab,
    lds_bytes, single_lds_bytes, block.  Needs no ctx and no device."""
    out = ProjectPlan()
    rc = load_library().chip_project_plan(in_dim, matrix_type, n, C.byref(out))
    if rc != CHIP_OK:
        raise ChipError(rc, "chip_project_plan")
    return {name: getattr(out, name) for name, _ in ProjectPlan._fields_ if name != "reserved"}


CHIP_QUERY_PREFIX_GROUP = 4096


class QueryPrefixPlan(C.Structure):
    """chip_query_prefix_plan_out"""
    _fields_ = [("group_size", C.c_int32), ("groups", C.c_int32), ("tile_full", C.c_int32), ("tile_last", C.c_int32),
                ("qtiles", C.c_int64), ("units", C.c_int64), ("units_rect", C.c_int64)]


class QueryPrefixLast(C.Structure):
    """chip_query_prefix_last"""
    _fields_ = [("groups", C.c_int32), ("launches", C.c_int32), ("waits", C.c_int32), ("reserved", C.c_int32),
                ("units_claimed", C.c_int64), ("units_planned", C.c_int64)]


def query_prefix_plan(k, elem: int = 4, topk: int = 5) -> dict:
    """chip_query_prefix_plan -> the order and the work of a prefix call over the prefixes k: order (int32 [Q], the caller's position of
    the i-th query walked), group_size, groups, tile_full, tile_last, qtiles, units, units_rect.  Needs no ctx and no device."""
    k = np.ascontiguousarray(k, dtype=np.int64).reshape(-1)
    order = np.empty(k.shape[0], dtype=np.int32)
    out = QueryPrefixPlan()
    rc = load_library().chip_query_prefix_plan(_ptr(k), k.shape[0], elem, topk, _ptr(order), C.byref(out))
    if rc != CHIP_OK:
        raise ChipError(rc, "chip_query_prefix_plan")
    d = {name: getattr(out, name) for name, _ in QueryPrefixPlan._fields_}
    d["order"] = order
    return d


CHIP_BULK_TICKS_GROUP, CHIP_BULK_TICKS_MAX_TOPK = 1365, 8


class BulkTicksPlan(C.Structure):
    """chip_bulk_ticks_plan_out"""
    _fields_ = [("group_ticks", C.c_int32), ("groups", C.c_int32), ("tile_full", C.c_int32), ("tile_last", C.c_int32),
                ("ticks_scanned", C.c_int64), ("ticks_skipped", C.c_int64), ("ticks_too_short", C.c_int64),
                ("units", C.c_int64), ("units_rect", C.c_int64), ("last_l", C.c_int64)]


class BulkTicksLast(C.Structure):
    """chip_bulk_ticks_last"""
    _fields_ = [("groups", C.c_int32), ("launches", C.c_int32), ("waits", C.c_int32), ("list_len", C.c_int32),
                ("certified", C.c_int64), ("uncertified", C.c_int64), ("rescored_rows", C.c_int64),
                ("exact_reruns", C.c_int64), ("E", C.c_double)]


def bulk_ticks_plan(ls, n_rows: int, params: DotParams | None = None, last_l: int = 0) -> dict:
    """chip_bulk_ticks_plan -> status (int32 [T]) and k (int64 [T], 0 where the tick is not scanned) of the ticks at ls run one after the
    other from the loop state last_l on a DB of n_rows rows, and the grouping of a chip_loop_ticks_bulk call over them: group_ticks,
    groups, tile_full, tile_last, ticks_scanned / _skipped / _too_short, units, units_rect, last_l.  Needs no ctx and no device."""
    ls = np.ascontiguousarray(ls, dtype=np.int64).reshape(-1)
    T = ls.shape[0]
    status = np.empty(T, dtype=np.int32)
    k = np.empty(T, dtype=np.int64)
    out = BulkTicksPlan()
    rc = load_library().chip_bulk_ticks_plan(_ptr(ls) if T else None, T, C.byref(params) if params is not None else None, last_l, n_rows,
                                             _ptr(status), _ptr(k), C.byref(out))
    if rc != CHIP_OK:
        raise ChipError(rc, "chip_bulk_ticks_plan")
    d = {name: getattr(out, name) for name, _ in BulkTicksPlan._fields_}
    d["status"] = status
    d["k"] = k
    return d


def default_ransac_params() -> RansacParams:
    p = RansacParams()
    load_library().chip_ransac_params_default(C.byref(p))
    return p


def default_icp_params() -> RansacParams:
    p = RansacParams()
    load_library().chip_icp_params_default(C.byref(p))
    return p


def scan_plan(D: int, elem: int, nq: int, K: int, n_rows: int, call: int = CHIP_SCAN_CALL_QUERY, n_cus: int = 256, check: bool = True):
    """chip_debug_scan_plan: the kernel a plain single-GPU ctx created under the CURRENT environment would launch for this scan, as
    ScanLaunch.as_dict() -- no device needed.  check=False: (status, dict) instead of raising on a status other than CHIP_OK."""
    out = ScanLaunch()
    rc = load_library().chip_debug_scan_plan(D, elem, nq, K, n_rows, call, n_cus, C.byref(out))
    if not check:
        return rc, out.as_dict()
    if rc != CHIP_OK:
        raise ChipError(rc, "chip_debug_scan_plan")
    return out.as_dict()


def multi_plan(D: int, elem: int, n_ticks: int, K: int = CHIP_DEFAULT_TOPK, n_cus: int = 256, check: bool = True):
    """chip_debug_multi_plan: the pass that serves n_ticks pipelined ticks together on a plain single-GPU ctx, as ScanLaunch.as_dict() (q64 =
    queries staged as fp64, NG = queries read in place) -- no device needed.  check=False: (status, dict) instead of raising."""
    out = ScanLaunch()
    rc = load_library().chip_debug_multi_plan(D, elem, n_ticks, K, n_cus, C.byref(out))
    if not check:
        return rc, out.as_dict()
    if rc != CHIP_OK:
        raise ChipError(rc, "chip_debug_multi_plan")
    return out.as_dict()


def prefilter_plan(D: int, elem: int = 4, K: int = CHIP_DEFAULT_TOPK, n_cus: int = 256, check: bool = True):
    """chip_debug_prefilter_plan: the fp32 prefilter pass that serves four pipelined ticks together (float rows), as ScanLaunch.as_dict()
    (NG = queries read in place, the other 12 - NG staged in LDS) -- no device needed.  check=False: (status, dict) instead of raising."""
    out = ScanLaunch()
    rc = load_library().chip_debug_prefilter_plan(D, elem, K, n_cus, C.byref(out))
    if not check:
        return rc, out.as_dict()
    if rc != CHIP_OK:
        raise ChipError(rc, "chip_debug_prefilter_plan")
    return out.as_dict()


def halfq_plan(D: int, elem: int = 4, K: int = CHIP_DEFAULT_TOPK, n_cus: int = 256, check: bool = True):
    """chip_debug_halfq_plan: the pass that serves five pipelined ticks together (float rows, all 15 queries staged in LDS as fp16), as
    ScanLaunch.as_dict() -- no device needed.  check=False: (status, dict) instead of raising."""
    out = ScanLaunch()
    rc = load_library().chip_debug_halfq_plan(D, elem, K, n_cus, C.byref(out))
    if not check:
        return rc, out.as_dict()
    if rc != CHIP_OK:
        raise ChipError(rc, "chip_debug_halfq_plan")
    return out.as_dict()


def halfq_bound(D: int, row_norm_max: float) -> tuple[int, float]:
    """chip_debug_halfq_bound: (e, E_h) -- the exponent of the scale of the fp16-staged queries and the error bound of the five-tick pass"""
    e, E = C.c_int32(), C.c_double()
    rc = load_library().chip_debug_halfq_bound(D, row_norm_max, C.byref(e), C.byref(E))
    if rc != CHIP_OK:
        raise ChipError(rc, "chip_debug_halfq_bound")
    return e.value, E.value


def comm_unique_id() -> bytes:
    """chip_comm_unique_id: 128 bytes rank 0 hands to every rank (any transport) before chip_comm_init_rank"""
    buf = C.create_string_buffer(CHIP_COMM_ID_BYTES)
    st = load_library().chip_comm_unique_id(buf)
    if st != CHIP_OK:
        raise ChipError(st, "chip_comm_unique_id")
    return buf.raw


class Chip:
    """Thin RAII wrapper over a chip_ctx.  storage: None = decided by the data (chip_create), "f32" / "f64" = chip_create_ex.
    devices=[...] makes ONE ctx over several GPUs of this process (chip_create_multi); copy_exchange forces the device-copy
    exchange instead of RCCL (implied when a device is named twice)."""

    def __init__(self, D: int, capacity_hint: int = 0, device: int = 0, shard_rank: int = 0, shard_count: int = 1,
                 storage: str | None = None, devices=None, copy_exchange: bool = False):
        self.lib = load_library()
        self.D = int(D)
        self.shard_rank, self.shard_count = shard_rank, shard_count
        flags = {None: 0, "f32": CHIP_CREATE_STORE_F32, "f64": CHIP_CREATE_STORE_F64}[storage]
        h = C.c_void_p()
        if devices is not None:
            dev = np.ascontiguousarray(devices, dtype=np.int32)
            st = self.lib.chip_create_multi(C.byref(h), D, capacity_hint, _ptr(dev), dev.size,
                                            flags | (CHIP_MULTI_EXCHANGE_COPY if copy_exchange else 0))
            where = "chip_create_multi"
        elif flags:
            st = self.lib.chip_create_ex(C.byref(h), D, capacity_hint, device, shard_rank, shard_count, flags)
            where = "chip_create_ex"
        else:
            st = self.lib.chip_create(C.byref(h), D, capacity_hint, device, shard_rank, shard_count)
            where = "chip_create"
        if st != CHIP_OK:
            raise ChipError(st, where)
        self.h = h

    def comm_init_rank(self, unique_id: bytes, n_ranks: int, rank: int):
        """attach an RCCL communicator to this sharded ctx (one process per GPU); afterwards loop_tick* work on it"""
        assert len(unique_id) == CHIP_COMM_ID_BYTES
        self._chk(self.lib.chip_comm_init_rank(self.h, C.c_char_p(unique_id), n_ranks, rank), "chip_comm_init_rank")

    # -- lifecycle
    def close(self):
        if getattr(self, "h", None):
            self.lib.chip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, st: int, where: str):
        if st != CHIP_OK:
            txt = C.c_char_p()
            if st == CHIP_ERR_COMM:
                r = self.lib.chip_last_comm_error(self.h, C.byref(txt))
                raise ChipError(st, where, f"ncclResult {r}: {txt.value.decode() if txt.value else ''}")
            hip = self.lib.chip_last_hip_error(self.h, C.byref(txt)) if st in (CHIP_ERR_HIP, CHIP_ERR_OOM) else 0
            raise ChipError(st, where, f"hipError {hip}: {txt.value.decode() if txt.value else ''}" if hip else "")

    def last_comm_error(self) -> str:
        """chip_last_comm_error: "<code>: <text>" of the last RCCL failure (or abandoned bootstrap) this ctx has seen"""
        txt = C.c_char_p()
        r = self.lib.chip_last_comm_error(self.h, C.byref(txt))
        return f"{r}: {txt.value.decode() if txt.value else ''}"

    def set_stream(self, stream_ptr: int | None):
        """None -> back to the ctx's private stream; an int is a hipStream_t handle (0 = HIP's null stream)."""
        if stream_ptr is None:
            self._chk(self.lib.chip_reset_stream(self.h), "chip_reset_stream")
        else:
            self._chk(self.lib.chip_set_stream(self.h, C.c_void_p(stream_ptr)), "chip_set_stream")

    def synchronize(self):
        self._chk(self.lib.chip_synchronize(self.h), "chip_synchronize")

    # -- DB
    def append_f64(self, desc: np.ndarray, allow_rounding: bool = False) -> int:
        desc = np.ascontiguousarray(desc, dtype=np.float64).reshape(-1, self.D)
        first = C.c_int64()
        self._chk(self.lib.chip_db_append_f64(self.h, _ptr(desc), desc.shape[0],
                                              CHIP_APPEND_ALLOW_ROUNDING if allow_rounding else 0, C.byref(first)),
                  "chip_db_append_f64")
        return first.value

    def append_f32(self, desc: np.ndarray) -> int:
        desc = np.ascontiguousarray(desc, dtype=np.float32).reshape(-1, self.D)
        first = C.c_int64()
        self._chk(self.lib.chip_db_append_f32(self.h, _ptr(desc), desc.shape[0], C.byref(first)), "chip_db_append_f32")
        return first.value

    # -- descriptor projection: z = normalise(Mt x + b) made on the device (include/cerebro_hip.h "descriptor projection")
    def project_set(self, Mt: np.ndarray, bias=None):
        """chip_project_set: Mt is (D, in_dim), one row per OUTPUT component (np.ascontiguousarray(WPCA_M.T)), float32 or float64 --
        its dtype is the matrix type; bias: D doubles or None"""
        Mt = np.asarray(Mt)
        if Mt.dtype not in (np.float32, np.float64) or Mt.ndim != 2 or Mt.shape[0] != self.D:
            raise ValueError("project_set: Mt must be a (D, in_dim) float32 or float64 array")
        Mt = np.ascontiguousarray(Mt)
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float64).reshape(self.D)
        self._chk(self.lib.chip_project_set(self.h, Mt.shape[1], _ptr(Mt), CHIP_PROJ_F32 if Mt.dtype == np.float32 else CHIP_PROJ_F64,
                                            None if b is None else _ptr(b)), "chip_project_set")

    def project_clear(self):
        self._chk(self.lib.chip_project_clear(self.h), "chip_project_clear")

    def project_info(self) -> dict:
        """chip_project_info: in_dim 0 when no projection is set"""
        v = [C.c_int32(), C.c_int32(), C.c_int32()]
        self._chk(self.lib.chip_project_info(self.h, *(C.byref(x) for x in v)), "chip_project_info")
        return dict(in_dim=v[0].value, matrix_type=v[1].value, has_bias=bool(v[2].value))

    def _raw_descriptors(self, x, n):
        """(pointer, n, what keeps it alive) of raw descriptors: a numpy array of n x in_dim float32 values, or an integer device address
        (memory of the ctx's device that the caller has waited for) together with n"""
        if isinstance(x, (int, np.integer)):
            if n is None:
                raise ValueError("a device address needs n")
            return C.c_void_p(int(x)), int(n), None
        in_dim = self.project_info()["in_dim"]
        a = np.ascontiguousarray(x, dtype=np.float32)
        a = a.reshape(-1, in_dim) if in_dim else a.reshape(1, -1)      # (without a projection the call reports CHIP_ERR_BUSY itself)
        return _ptr(a), a.shape[0], a

    def project(self, x, n: int | None = None) -> np.ndarray:
        """chip_project -> (n, D) float64: the rows an append_projected of the same x would store in a double-row DB"""
        p, n, keep = self._raw_descriptors(x, n)
        z = np.empty((n, self.D), dtype=np.float64)
        self._chk(self.lib.chip_project(self.h, p, n, _ptr(z)), "chip_project")
        return z

    def append_projected(self, x, flags: int = 0, n: int | None = None) -> int:
        """chip_db_append_projected_f32 -> the index of the first row appended"""
        p, n, keep = self._raw_descriptors(x, n)
        first = C.c_int64()
        self._chk(self.lib.chip_db_append_projected_f32(self.h, p, n, flags, C.byref(first)), "chip_db_append_projected_f32")
        return first.value

    def debug_project_last(self) -> dict:
        """chip_debug_project_last: what the last projecting call launched -- shared passes and single launches, counted apart"""
        passes, descs, width = (C.c_int64 * 2)(), (C.c_int64 * 2)(), C.c_int32()
        self._chk(self.lib.chip_debug_project_last(self.h, passes, descs, C.byref(width)), "chip_debug_project_last")
        return dict(shared_passes=passes[0], single_launches=passes[1], shared_descriptors=descs[0], single_descriptors=descs[1],
                    width=width.value)

    # -- NetVLAD pooling: the trunk's feature map -> the pooled float32 vector on the device (include/cerebro_hip.h "NetVLAD pooling")
    def vlad_set(self, Wt, bias, centres):
        """chip_vlad_set: Wt (K+G, C), bias (K+G), centres (K, C), all float32; K = centres.shape[0], the other rows are ghosts"""
        Wt = np.ascontiguousarray(Wt, dtype=np.float32)
        centres = np.ascontiguousarray(centres, dtype=np.float32)
        bias = np.ascontiguousarray(bias, dtype=np.float32).reshape(-1)
        if Wt.ndim != 2 or centres.ndim != 2 or centres.shape[1] != Wt.shape[1] or bias.size != Wt.shape[0] or centres.shape[0] > Wt.shape[0]:
            raise ValueError("vlad_set: Wt (K+G, C), bias (K+G), centres (K, C)")
        K, G = centres.shape[0], Wt.shape[0] - centres.shape[0]
        self._chk(self.lib.chip_vlad_set(self.h, Wt.shape[1], K, G, _ptr(Wt), _ptr(bias), _ptr(centres)), "chip_vlad_set")

    def vlad_clear(self):
        self._chk(self.lib.chip_vlad_clear(self.h), "chip_vlad_clear")

    def vlad_info(self) -> dict:
        """chip_vlad_info: all 0 when no weights are set"""
        v = [C.c_int32(), C.c_int32(), C.c_int32()]
        self._chk(self.lib.chip_vlad_info(self.h, *(C.byref(x) for x in v)), "chip_vlad_info")
        return dict(channels=v[0].value, clusters=v[1].value, ghost=v[2].value)

    def _feature_map(self, fmap, positions, layout):
        """(pointer, positions, what keeps it alive): a numpy array -- (N, C) for CHIP_VLAD_NHWC, (C, N) for CHIP_VLAD_NCHW, leading axes
        of one flattened -- or an integer device address (memory of the ctx's device that the caller has waited for) with positions"""
        if isinstance(fmap, (int, np.integer)):
            if positions is None:
                raise ValueError("a device address needs positions")
            return C.c_void_p(int(fmap)), int(positions), None
        a = np.ascontiguousarray(fmap, dtype=np.float32)
        ch = self.vlad_info()["channels"]
        if positions is None:
            positions = a.size // ch if ch else a.size     # (without weights the call reports CHIP_ERR_BUSY itself)
        return _ptr(a), int(positions), a

    def vlad(self, fmap, layout: int = CHIP_VLAD_NHWC, positions: int | None = None) -> np.ndarray:
        """chip_vlad -> the pooled vector, (K * C,) float32"""
        p, n, keep = self._feature_map(fmap, positions, layout)
        i = self.vlad_info()
        v = np.empty(max(i["clusters"] * i["channels"], 1), dtype=np.float32)
        self._chk(self.lib.chip_vlad(self.h, p, n, layout, _ptr(v)), "chip_vlad")
        return v

    def append_vlad(self, fmap, layout: int = CHIP_VLAD_NHWC, flags: int = 0, positions: int | None = None) -> int:
        """chip_db_append_vlad_f32 -> the index of the row appended"""
        p, n, keep = self._feature_map(fmap, positions, layout)
        first = C.c_int64()
        self._chk(self.lib.chip_db_append_vlad_f32(self.h, p, n, layout, flags, C.byref(first)), "chip_db_append_vlad_f32")
        return first.value

    def _feature_maps(self, fmaps, n_maps, positions):
        """(pointer, n_maps, positions, what keeps it alive) of a batch: a numpy array whose first axis counts the maps -- (B, N, C) or
        (B, H, W, C) for CHIP_VLAD_NHWC, (B, C, N) or (B, C, H, W) for CHIP_VLAD_NCHW -- or an integer device address with both counts"""
        if isinstance(fmaps, (int, np.integer)):
            if positions is None or n_maps is None:
                raise ValueError("a device address needs n_maps and positions")
            return C.c_void_p(int(fmaps)), int(n_maps), int(positions), None
        a = np.ascontiguousarray(fmaps, dtype=np.float32)
        if n_maps is None:
            n_maps = a.shape[0]
        ch = self.vlad_info()["channels"]
        if positions is None:
            positions = a.size // (ch * n_maps) if ch and n_maps else 1
        return _ptr(a), int(n_maps), int(positions), a

    def vlad_batch(self, fmaps, layout: int = CHIP_VLAD_NHWC, n_maps: int | None = None, positions: int | None = None) -> np.ndarray:
        """chip_vlad_batch -> (n_maps, K * C) float32: row m is vlad(map m)"""
        p, b, n, keep = self._feature_maps(fmaps, n_maps, positions)
        i = self.vlad_info()
        v = np.empty((b, max(i["clusters"] * i["channels"], 1)), dtype=np.float32)
        self._chk(self.lib.chip_vlad_batch(self.h, p, b, n, layout, _ptr(v)), "chip_vlad_batch")
        return v

    def append_vlad_batch(self, fmaps, layout: int = CHIP_VLAD_NHWC, flags: int = 0, n_maps: int | None = None,
                          positions: int | None = None) -> int:
        """chip_db_append_vlad_batch_f32 -> the index of the first row appended"""
        p, b, n, keep = self._feature_maps(fmaps, n_maps, positions)
        first = C.c_int64()
        self._chk(self.lib.chip_db_append_vlad_batch_f32(self.h, p, b, n, layout, flags, C.byref(first)), "chip_db_append_vlad_batch_f32")
        return first.value

    def debug_vlad_stage(self, positions: int) -> dict:
        """chip_debug_vlad_stage after a pooling call over `positions` positions -> a (N, K+G), V (K, C), A (K,), float64"""
        i = self.vlad_info()
        a = np.empty((int(positions), i["clusters"] + i["ghost"]))
        V = np.empty((i["clusters"], i["channels"]))
        A = np.empty(i["clusters"])
        self._chk(self.lib.chip_debug_vlad_stage(self.h, _ptr(a), _ptr(V), _ptr(A)), "chip_debug_vlad_stage")
        return dict(a=a, V=V, A=A)

    def append_synthetic(self, n: int, seed: int, plants=(), unit: bool = False):
        """unit=True: the rows normalised to unit L2 norm (chip_db_append_synthetic_unit, SURVEY.md 8d's data)."""
        plants = sorted(plants)
        name = "chip_db_append_synthetic_unit" if unit else "chip_db_append_synthetic"
        fn = getattr(self.lib, name)
        if plants:
            dst = np.array([p[0] for p in plants], dtype=np.int64)
            src = np.array([p[1] for p in plants], dtype=np.int64)
            kind = np.array([p[2] for p in plants], dtype=np.int32)
            st = fn(self.h, n, seed, _ptr(dst), _ptr(src), _ptr(kind), len(plants))
        else:
            st = fn(self.h, n, seed, None, None, None, 0)
        self._chk(st, name)

    def size(self) -> int:
        return int(self.lib.chip_db_size(self.h))

    def read_rows(self, rows) -> np.ndarray:
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        out = np.empty((rows.size, self.D), dtype=np.float32)
        self._chk(self.lib.chip_db_read_rows_f32(self.h, _ptr(rows), rows.size, _ptr(out)), "chip_db_read_rows_f32")
        return out

    def read_rows_f64(self, rows) -> np.ndarray:
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        out = np.empty((rows.size, self.D), dtype=np.float64)
        self._chk(self.lib.chip_db_read_rows_f64(self.h, _ptr(rows), rows.size, _ptr(out)), "chip_db_read_rows_f64")
        return out

    # -- queries
    def query_scores(self, k: int, row: int) -> np.ndarray:
        """the whole score vector u = v^T M[:, :k] of one query row (Cerebro.cpp:1026)"""
        u = np.full(max(k, 1), np.nan, dtype=np.float64)
        self._chk(self.lib.chip_query_scores(self.h, k, row, _ptr(u)), "chip_query_scores")
        return u[:k]

    def query_vectors_f64(self, k: int, q: np.ndarray, topk: int = CHIP_DEFAULT_TOPK):
        q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, self.D)
        nq = q.shape[0]
        sc = np.empty((nq, topk), dtype=np.float64)
        ix = np.empty((nq, topk), dtype=np.int64)
        self._chk(self.lib.chip_query_vectors_f64(self.h, k, _ptr(q), nq, topk, _ptr(sc), _ptr(ix)), "chip_query_vectors_f64")
        return sc, ix

    def query_rows(self, k: int, rows, topk: int = CHIP_DEFAULT_TOPK):
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        nq = rows.size
        sc = np.empty((nq, topk), dtype=np.float64)
        ix = np.empty((nq, topk), dtype=np.int64)
        self._chk(self.lib.chip_query_rows(self.h, k, _ptr(rows), nq, topk, _ptr(sc), _ptr(ix)), "chip_query_rows")
        return sc, ix

    def query_vectors(self, k: int, q: np.ndarray, topk: int = CHIP_DEFAULT_TOPK):
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, self.D)
        nq = q.shape[0]
        sc = np.empty((nq, topk), dtype=np.float64)
        ix = np.empty((nq, topk), dtype=np.int64)
        self._chk(self.lib.chip_query_vectors_f32(self.h, k, _ptr(q), nq, topk, _ptr(sc), _ptr(ix)),
                  "chip_query_vectors_f32")
        return sc, ix

    def query_batch(self, k: int, q: np.ndarray, topk: int = CHIP_DEFAULT_TOPK, cast_rows: bool = False):
        """many-query fp32 MFMA mode: returns (scores float32 [Q, topk], idx int64 [Q, topk]).  cast_rows=True goes through
        chip_query_batch_cast_f32: a double-row DB is accepted, its rows narrowed to float (RNE) in the GEMM's loader."""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, self.D)
        Q = q.shape[0]
        sc = np.empty((Q, topk), dtype=np.float32)
        ix = np.empty((Q, topk), dtype=np.int64)
        name = "chip_query_batch_cast_f32" if cast_rows else "chip_query_batch_f32"
        self._chk(getattr(self.lib, name)(self.h, k, _ptr(q), Q, topk, _ptr(sc), _ptr(ix)), name)
        return sc, ix

    def query_batch_rows(self, rows, k, topk: int = CHIP_DEFAULT_TOPK, cast_rows: bool = False):
        """many-query mode with a prefix per query, the queries taken from DB rows on the device: query j is row rows[j] against rows
        [0, k[j]).  Returns (scores float32 [Q, topk], idx int64 [Q, topk]) in the caller's order; entry j is what
        query_batch(k[j], row rows[j], topk) gives.  cast_rows=True: chip_query_batch_rows_cast_f32 (double rows, narrowed RNE)."""
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        k = np.ascontiguousarray(k, dtype=np.int64).reshape(-1)
        if rows.shape != k.shape:
            raise ValueError("rows and k must have the same length")
        Q = rows.shape[0]
        sc = np.empty((Q, topk), dtype=np.float32)
        ix = np.empty((Q, topk), dtype=np.int64)
        name = "chip_query_batch_rows_cast_f32" if cast_rows else "chip_query_batch_rows_f32"
        self._chk(getattr(self.lib, name)(self.h, _ptr(rows), _ptr(k), Q, topk, _ptr(sc), _ptr(ix)), name)
        return sc, ix

    def query_batch_prefix(self, k, q: np.ndarray, topk: int = CHIP_DEFAULT_TOPK, cast_rows: bool = False):
        """many-query mode with a prefix per query, host vectors: query j is q[j] against rows [0, k[j]).  Returns as query_batch_rows."""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, self.D)
        k = np.ascontiguousarray(k, dtype=np.int64).reshape(-1)
        Q = q.shape[0]
        if k.shape[0] != Q:
            raise ValueError("k must have one entry per query")
        sc = np.empty((Q, topk), dtype=np.float32)
        ix = np.empty((Q, topk), dtype=np.int64)
        name = "chip_query_batch_prefix_cast_f32" if cast_rows else "chip_query_batch_prefix_f32"
        self._chk(getattr(self.lib, name)(self.h, _ptr(k), _ptr(q), Q, topk, _ptr(sc), _ptr(ix)), name)
        return sc, ix

    def self_join(self, first: int, count: int, lag: int, topk: int = CHIP_DEFAULT_TOPK, cast_rows: bool = False):
        """the causal self-join of rows [first, first + count): row first + j against rows [0, max(0, first + j - lag)) -- one
        query_batch_rows call."""
        rows = first + np.arange(count, dtype=np.int64)
        return self.query_batch_rows(rows, np.maximum(0, rows - lag), topk, cast_rows)

    def debug_query_prefix_last(self) -> dict:
        """chip_debug_query_prefix_last: groups, launches, host waits of the last prefix call, the DB tiles its kernels walked
        (units_claimed, from the kernels' own counters) and the tiles the host planned (units_planned)"""
        out = QueryPrefixLast()
        self._chk(self.lib.chip_debug_query_prefix_last(self.h, C.byref(out)), "chip_debug_query_prefix_last")
        return {name: getattr(out, name) for name, _ in QueryPrefixLast._fields_ if name != "reserved"}

    # -- tick
    def loop_tick(self, l: int, params: DotParams | None = None) -> TickResult:
        p = params or default_dot_params()
        r = TickResult()
        self._chk(self.lib.chip_loop_tick(self.h, l, C.byref(p), C.byref(r)), "chip_loop_tick")
        return r

    def loop_ticks_bulk(self, ls, params: DotParams | None = None, last_l: int = 0, topk: int = 1):
        """chip_loop_ticks_bulk: the records of loop_tick(ls[0]), loop_tick(ls[1]), ... started from the loop state last_l, from many-query
        passes -- the ctx's own loop state is neither read nor written.  Returns (records: list of TickResult, scores float64
        [T, 3, topk], idx int64 [T, 3, topk], last_l after the last tick); the lists of a scanned tick are query_rows(l - lag,
        [l-1, l-2, l-3], topk)'s, of every other tick -inf / -1."""
        ls = np.ascontiguousarray(ls, dtype=np.int64).reshape(-1)
        T = ls.shape[0]
        recs = (TickResult * max(T, 1))()
        sc = np.empty((T, 3, topk), dtype=np.float64)
        ix = np.empty((T, 3, topk), dtype=np.int64)
        last = C.c_int64(last_l)
        self._chk(self.lib.chip_loop_ticks_bulk(self.h, _ptr(ls) if T else None, T, C.byref(params) if params is not None else None, last_l, topk,
                                                C.byref(recs), _ptr(sc), _ptr(ix), C.byref(last)), "chip_loop_ticks_bulk")
        return [recs[t] for t in range(T)], sc, ix, last.value

    def debug_bulk_ticks_last(self) -> dict:
        """chip_debug_bulk_ticks_last: groups, launches and host waits of the last bulk call, list_len (KL), its certified / uncertified
        ticks, the rows its finishing launches scored exactly, the ticks it ran again through the exact scan, the error bound E"""
        out = BulkTicksLast()
        self._chk(self.lib.chip_debug_bulk_ticks_last(self.h, C.byref(out)), "chip_debug_bulk_ticks_last")
        return {name: getattr(out, name) for name, _ in BulkTicksLast._fields_}

    def resident_pause(self):
        self._chk(self.lib.chip_resident_pause(self.h), "chip_resident_pause")

    def resident_resume(self):
        self._chk(self.lib.chip_resident_resume(self.h), "chip_resident_resume")

    def loop_tick_enqueue(self, l: int, slot: int, params: DotParams | None = None):
        p = params or default_dot_params()
        self._chk(self.lib.chip_loop_tick_enqueue(self.h, l, C.byref(p), slot), "chip_loop_tick_enqueue")

    def loop_tick_collect(self, slot: int) -> TickResult:
        r = TickResult()
        self._chk(self.lib.chip_loop_tick_collect(self.h, slot, C.byref(r)), "chip_loop_tick_collect")
        return r

    def loop_reset(self):
        self.lib.chip_loop_reset(self.h)

    def last_l(self) -> int:
        return int(self.lib.chip_loop_last_l(self.h))

    def coalesce_stats(self) -> tuple[int, int]:
        """(passes that served more than one pipelined tick, ticks those passes served) -- chip_debug_coalesce_stats"""
        passes, ticks = C.c_int64(), C.c_int64()
        self._chk(self.lib.chip_debug_coalesce_stats(self.h, C.byref(passes), C.byref(ticks)), "chip_debug_coalesce_stats")
        return passes.value, ticks.value

    def prefilter_stats(self) -> tuple[int, int, int]:
        """(prefilter passes of four or five ticks, ticks they served, ticks among them run again alone because their certificate did not hold) --
        chip_debug_prefilter_stats"""
        passes, ticks, unc = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self.lib.chip_debug_prefilter_stats(self.h, C.byref(passes), C.byref(ticks), C.byref(unc)), "chip_debug_prefilter_stats")
        return passes.value, ticks.value, unc.value

    def coalesce_force(self, on: bool):
        """tests: while on, a pipelined tick that may share a pass parks even when no scan of the ctx is running"""
        self._chk(self.lib.chip_debug_coalesce_force(self.h, 1 if on else 0), "chip_debug_coalesce_force")

    def last_scan(self) -> dict:
        """which kernel the last top-k scan of this ctx ran (chip_debug_last_scan): ScanLaunch.as_dict()"""
        out = ScanLaunch()
        self._chk(self.lib.chip_debug_last_scan(self.h, C.byref(out)), "chip_debug_last_scan")
        return out.as_dict()

    def last_pass(self) -> dict:
        """chip_debug_last_pass: the ctx's last prefilter pass (four ticks or five) read back -- family, ticks, grid, wpb, K, k (list), E, e,
        cand_s float64 / cand_i int64 [T, grid, 3, K] (the pass's lists), exact_s / exact_i [T, 3, K] (tick_rescore's lists),
        cert uint32 [T, 3] (1 certified, 2 not)"""
        info = PassInfo()
        self._chk(self.lib.chip_debug_last_pass(self.h, C.byref(info), None, None, None), "chip_debug_last_pass")
        T, grid, K = info.ticks, info.grid, info.K
        cand = np.empty((T, grid, 3, K, 2), dtype=np.float64)
        exact = np.empty((T, 3, K, 2), dtype=np.float64)
        cert = np.zeros((T, 3), dtype=np.uint32)
        self._chk(self.lib.chip_debug_last_pass(self.h, C.byref(info), _ptr(cand), _ptr(exact), _ptr(cert)), "chip_debug_last_pass")
        return dict(family=SCAN_FAMILY_NAMES[info.family], ticks=T, grid=grid, wpb=int(info.wpb), K=K, k=[int(x) for x in info.k[:T]],
                    E=float(info.E), e=int(info.e), cand_s=cand[..., 0].copy(), cand_i=cand[..., 1].copy().view(np.int64),
                    exact_s=exact[..., 0].copy(), exact_i=exact[..., 1].copy().view(np.int64), cert=cert)

    def scan_local(self, l: int, dev_out_ptr: int, topk: int = CHIP_DEFAULT_TOPK, params: DotParams | None = None) -> int:
        p = params or default_dot_params()
        status = C.c_int32()
        self._chk(self.lib.chip_scan_local(self.h, l, C.byref(p), topk, C.c_void_p(dev_out_ptr), C.byref(status)),
                  "chip_scan_local")
        return status.value

    def merge_decide(self, l: int, dev_gathered_ptr: int, n_lists: int, topk: int = CHIP_DEFAULT_TOPK,
                     params: DotParams | None = None) -> TickResult:
        p = params or default_dot_params()
        r = TickResult()
        self._chk(self.lib.chip_merge_decide(self.h, l, C.byref(p), C.c_void_p(dev_gathered_ptr), n_lists, topk,
                                             C.byref(r)), "chip_merge_decide")
        return r

    def merge_decide_enqueue(self, l: int, dev_gathered_ptr: int, n_lists: int, slot: int, topk: int = CHIP_DEFAULT_TOPK,
                             params: DotParams | None = None):
        p = params or default_dot_params()
        self._chk(self.lib.chip_merge_decide_enqueue(self.h, l, C.byref(p), C.c_void_p(dev_gathered_ptr), n_lists, topk, slot),
                  "chip_merge_decide_enqueue")

    def debug_merge_lists(self, form: int, scores: np.ndarray, idx: np.ndarray, l: int = 0, params: DotParams | None = None,
                          record: bool = False):
        """chip_debug_merge_lists: scores float64 / idx int64 [n_lists, nq, K] through topk_merge<nq> (form 0) or topk_merge_batch
        (form 1) -> (scores [nq, K], idx [nq, K], TickResult or None), as the kernel wrote them (idx[0, 0] == -2: a failed list)."""
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        assert scores.ndim == 3 and scores.shape == idx.shape
        n_lists, nq, K = scores.shape
        lists = np.empty((n_lists, nq, K, 2), dtype=np.float64)
        lists[..., 0] = scores
        lists[..., 1] = idx.view(np.float64)
        out = np.empty((nq, K, 2), dtype=np.float64)
        r = TickResult() if record else None
        p = params or default_dot_params()
        self._chk(self.lib.chip_debug_merge_lists(self.h, form, _ptr(lists), n_lists, nq, K, _ptr(out), l, C.byref(p),
                                                  C.byref(r) if record else None), "chip_debug_merge_lists")
        return out[..., 0].copy(), out[..., 1].copy().view(np.int64), r

    # -- PnP
    def pnp_ransac(self, X: np.ndarray, uv: np.ndarray, params: RansacParams | None = None):
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
        uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
        N = X.shape[0]
        assert uv.shape[0] == N
        p = params or default_ransac_params()
        T = np.empty(16, dtype=np.float64)
        conf = C.c_float()
        mask = np.zeros(max(N, 1), dtype=np.uint8)
        summ = RansacSummary()
        st = self.lib.chip_pnp_ransac(self.h, _ptr(X), _ptr(uv), N, C.byref(p), _ptr(T), C.byref(conf), _ptr(mask),
                                      C.byref(summ))
        if st == CHIP_ERR_TOO_FEW_POINTS:
            return dict(status=st, confidence=-1.0, T=None, mask=None, summary=None)
        self._chk(st, "chip_pnp_ransac")
        return dict(status=st, confidence=float(conf.value), T=T.reshape(4, 4).T.copy(), mask=mask[:N].copy(),
                    summary=dict(n_iterations=summ.n_iterations, n_inliers=summ.n_inliers,
                                 best_hypothesis=summ.best_hypothesis, n_models=summ.n_models,
                                 best_cost=summ.best_cost))

    def pnp_ransac_batch(self, problems, params: RansacParams | None = None, seeds=None):
        """problems: list of (X (N_i,3), uv (N_i,2)).  One pair of launches for the whole list; entry i equals
        pnp_ransac(X_i, uv_i) run with seed seeds[i] (default: params.seed for all)."""
        P = len(problems)
        Xs = [np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3) for X, _ in problems]
        uvs = [np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2) for _, uv in problems]
        Ns = np.array([x.shape[0] for x in Xs], dtype=np.int32)
        p = params or default_ransac_params()
        T = np.empty((P, 16), dtype=np.float64)
        conf = np.zeros(P, dtype=np.float32)
        masks = [np.zeros(max(int(n), 1), dtype=np.uint8) for n in Ns]
        summ = (RansacSummary * max(P, 1))()
        Xp = (C.c_void_p * max(P, 1))(*[x.ctypes.data for x in Xs])
        uvp = (C.c_void_p * max(P, 1))(*[u.ctypes.data for u in uvs])
        mp = (C.c_void_p * max(P, 1))(*[m.ctypes.data for m in masks])
        sd = None if seeds is None else np.asarray(seeds, dtype=np.uint64)
        st = self.lib.chip_pnp_ransac_batch(self.h, P, Xp, uvp, _ptr(Ns), C.byref(p), None if sd is None else _ptr(sd),
                                            _ptr(T), _ptr(conf), mp, summ)
        self._chk(st, "chip_pnp_ransac_batch")
        return [dict(status=st, confidence=float(conf[i]), T=T[i].reshape(4, 4).T.copy(), mask=masks[i][:Ns[i]].copy(),
                     summary=dict(n_iterations=summ[i].n_iterations, n_inliers=summ[i].n_inliers,
                                  best_hypothesis=summ[i].best_hypothesis, n_models=summ[i].n_models,
                                  best_cost=summ[i].best_cost)) for i in range(P)]

    def icp_ransac_enqueue(self, A: np.ndarray, B: np.ndarray, params: RansacParams | None = None):
        """start an ICP estimation on the ctx's ICP stream (returns at once); fetch it with icp_ransac_collect(N)"""
        A = np.ascontiguousarray(A, dtype=np.float64).reshape(-1, 3)
        B = np.ascontiguousarray(B, dtype=np.float64).reshape(-1, 3)
        p = params or default_icp_params()
        self._chk(self.lib.chip_icp_ransac_enqueue(self.h, _ptr(A), _ptr(B), A.shape[0], C.byref(p)), "chip_icp_ransac_enqueue")
        return A.shape[0]

    def icp_ransac_collect(self, N: int):
        T = np.empty(16, dtype=np.float64)
        conf = C.c_float()
        mask = np.zeros(max(N, 1), dtype=np.uint8)
        summ = RansacSummary()
        self._chk(self.lib.chip_icp_ransac_collect(self.h, _ptr(T), C.byref(conf), _ptr(mask), C.byref(summ)), "chip_icp_ransac_collect")
        return dict(status=0, confidence=float(conf.value), T=T.reshape(4, 4).T.copy(), mask=mask[:N].copy(),
                    summary=dict(n_iterations=summ.n_iterations, n_inliers=summ.n_inliers, best_hypothesis=summ.best_hypothesis,
                                 n_models=summ.n_models, best_cost=summ.best_cost))

    def icp_ransac(self, A: np.ndarray, B: np.ndarray, params: RansacParams | None = None):
        A = np.ascontiguousarray(A, dtype=np.float64).reshape(-1, 3)
        B = np.ascontiguousarray(B, dtype=np.float64).reshape(-1, 3)
        N = A.shape[0]
        assert B.shape[0] == N
        p = params or default_icp_params()
        T = np.empty(16, dtype=np.float64)
        conf = C.c_float()
        mask = np.zeros(max(N, 1), dtype=np.uint8)
        summ = RansacSummary()
        st = self.lib.chip_icp_ransac(self.h, _ptr(A), _ptr(B), N, C.byref(p), _ptr(T), C.byref(conf), _ptr(mask), C.byref(summ))
        if st == CHIP_ERR_TOO_FEW_POINTS:
            return dict(status=st, confidence=-1.0, T=None, mask=None, summary=None)
        self._chk(st, "chip_icp_ransac")
        return dict(status=st, confidence=float(conf.value), T=T.reshape(4, 4).T.copy(), mask=mask[:N].copy(),
                    summary=dict(n_iterations=summ.n_iterations, n_inliers=summ.n_inliers,
                                 best_hypothesis=summ.best_hypothesis, n_models=summ.n_models, best_cost=summ.best_cost))

    def icp_ransac_batch(self, problems, params: RansacParams | None = None, seeds=None):
        """problems: list of (A (N_i,3), B (N_i,3)), at most CHIP_ICP_MAX_BATCH.  One pair of launches for the whole list; entry i equals
        icp_ransac(A_i, B_i) run with seed seeds[i] (default: params.seed for all)."""
        P = len(problems)
        As = [np.ascontiguousarray(A, dtype=np.float64).reshape(-1, 3) for A, _ in problems]
        Bs = [np.ascontiguousarray(B, dtype=np.float64).reshape(-1, 3) for _, B in problems]
        Ns = np.array([a.shape[0] for a in As], dtype=np.int32)
        p = params or default_icp_params()
        T = np.empty((max(P, 1), 16), dtype=np.float64)
        conf = np.zeros(max(P, 1), dtype=np.float32)
        masks = [np.zeros(max(int(n), 1), dtype=np.uint8) for n in Ns]
        summ = (RansacSummary * max(P, 1))()
        Ap = (C.c_void_p * max(P, 1))(*[a.ctypes.data for a in As])
        Bp = (C.c_void_p * max(P, 1))(*[b.ctypes.data for b in Bs])
        mp = (C.c_void_p * max(P, 1))(*[m.ctypes.data for m in masks])
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        st = self.lib.chip_icp_ransac_batch(self.h, P, Ap, Bp, _ptr(Ns), C.byref(p), None if sd is None else _ptr(sd), _ptr(T), _ptr(conf), mp, summ)
        self._chk(st, "chip_icp_ransac_batch")
        return [dict(status=st, confidence=float(conf[i]), T=T[i].reshape(4, 4).T.copy(), mask=masks[i][:Ns[i]].copy(),
                     summary=dict(n_iterations=summ[i].n_iterations, n_inliers=summ[i].n_inliers, best_hypothesis=summ[i].best_hypothesis,
                                  n_models=summ[i].n_models, best_cost=summ[i].best_cost)) for i in range(P)]

    # -- test aids: every hypothesis of the last estimation
    def ransac_record(self, leg: int = CHIP_RANSAC_LEG_PNP, problem: int = 0) -> dict:
        """chip_debug_ransac_record: the record of every hypothesis of problem `problem` of the last PnP launch or of the last collected
        ICP launch (a single call: problem 0 of 1; a matched batch: the problems that ran): P, H, N, words, S, sampler and valid[H], cost[H], nin[H], T[H, 16] (column-major), mask[H, words] (uint64);
        PnP also nsol[H] and sample[H, S].  Rejected hypotheses: T = NaN, mask row 0."""
        sh = self.ransac_record_shape(leg, problem)
        H, W, S = sh["H"], sh["words"], sh["S"]
        r = dict(valid=np.empty(H, np.int32), cost=np.empty(H, np.float64), nin=np.empty(H, np.int32), T=np.empty((H, 16), np.float64),
                 mask=np.empty((H, W), np.uint64))
        if leg == CHIP_RANSAC_LEG_PNP:
            r.update(nsol=np.empty(H, np.int32), sample=np.empty((H, S), np.int32))
        ptrs = [_ptr(r[k]) if k in r else None for k in ("valid", "cost", "nin", "T", "mask", "nsol", "sample")]
        self._chk(self.lib.chip_debug_ransac_record(self.h, leg, problem, None, *ptrs), "chip_debug_ransac_record")
        r.update(sh)
        return r

    def pnp_stage(self, problem: int = 0) -> dict:
        """chip_debug_pnp_stage: what pnp_build_solve handed to pnp_eig_score in the last PnP launch: ok[H], Tg[H, 27], Sg[H, 27, 27] (NaN
        where ok is 0; exactly what the first kernel wrote only for launches made under pnp_keep_stage(True))"""
        H = self.ransac_record_shape(CHIP_RANSAC_LEG_PNP, problem)["H"]
        r = dict(ok=np.empty(H, np.int32), Tg=np.empty((H, 27), np.float64), Sg=np.empty((H, 27, 27), np.float64))
        self._chk(self.lib.chip_debug_pnp_stage(self.h, problem, _ptr(r["ok"]), _ptr(r["Tg"]), _ptr(r["Sg"])), "chip_debug_pnp_stage")
        return r

    def ransac_record_shape(self, leg: int = CHIP_RANSAC_LEG_PNP, problem: int = 0) -> dict:
        sh = RansacShape()
        self._chk(self.lib.chip_debug_ransac_record(self.h, leg, problem, C.byref(sh), *([None] * 7)), "chip_debug_ransac_record")
        return {k: int(getattr(sh, k)) for k, _ in RansacShape._fields_}

    def pnp_keep_stage(self, on: bool = True):
        """while on, a PnP launch copies the action matrices aside between its two kernels (pnp_stage()'s Sg)"""
        self._chk(self.lib.chip_debug_pnp_keep_stage(self.h, 1 if on else 0), "chip_debug_pnp_keep_stage")

    # -- candidate verification front end (ORB matching, GMS, correspondence sets)
    def orb_match(self, d1: np.ndarray, d2: np.ndarray):
        """-> (train_idx, distance) int32 per query descriptor; ties -> the lowest train index; no train descriptors: -1 / -1"""
        d1 = np.ascontiguousarray(d1, dtype=np.uint8).reshape(-1, CHIP_ORB_DESC_BYTES)
        d2 = np.ascontiguousarray(d2, dtype=np.uint8).reshape(-1, CHIP_ORB_DESC_BYTES)
        n1, n2 = d1.shape[0], d2.shape[0]
        idx = np.full(max(n1, 1), -1, dtype=np.int32)
        dist = np.full(max(n1, 1), -1, dtype=np.int32)
        self._chk(self.lib.chip_orb_match(self.h, _ptr(d1), n1, _ptr(d2), n2, _ptr(idx), _ptr(dist)), "chip_orb_match")
        return idx[:n1].copy(), dist[:n1].copy()

    def gms_filter(self, kp1: np.ndarray, size1, kp2: np.ndarray, size2, query_idx, train_idx, modes=None):
        """size = (width, height) -> uint8 inlier mask in match order.  modes (CHIP_GMS_WITH_SCALE | CHIP_GMS_WITH_ROTATION, or 0):
        chip_gms_filter_modes -> (mask, choice dict(scale, rotation, n_inliers, counts (5, 8)))"""
        kp1 = np.ascontiguousarray(kp1, dtype=np.float32).reshape(-1, 2)
        kp2 = np.ascontiguousarray(kp2, dtype=np.float32).reshape(-1, 2)
        q = np.ascontiguousarray(query_idx, dtype=np.int32)
        t = np.ascontiguousarray(train_idx, dtype=np.int32)
        assert q.shape == t.shape
        n = q.shape[0]
        mask = np.zeros(max(n, 1), dtype=np.uint8)
        cnt = C.c_int32()
        if modes is not None:
            ch = GmsChoice()
            self._chk(self.lib.chip_gms_filter_modes(self.h, _ptr(kp1), kp1.shape[0], size1[0], size1[1], _ptr(kp2), kp2.shape[0], size2[0],
                                                     size2[1], _ptr(q), _ptr(t), n, modes, _ptr(mask), C.byref(cnt), C.byref(ch)),
                      "chip_gms_filter_modes")
            assert cnt.value == int(mask[:n].sum()) == ch.n_inliers
            return mask[:n].copy(), ch.as_dict()
        self._chk(self.lib.chip_gms_filter(self.h, _ptr(kp1), kp1.shape[0], size1[0], size1[1], _ptr(kp2), kp2.shape[0], size2[0], size2[1],
                                           _ptr(q), _ptr(t), n, _ptr(mask), C.byref(cnt)), "chip_gms_filter")
        assert cnt.value == int(mask[:n].sum())
        return mask[:n].copy()

    @staticmethod
    def _match_frame(f: dict):
        desc = np.ascontiguousarray(f["desc"], dtype=np.uint8).reshape(-1, CHIP_ORB_DESC_BYTES)
        kp = np.ascontiguousarray(f["kp"], dtype=np.float32).reshape(-1, 2)
        xyz = np.ascontiguousarray(f["xyz"], dtype=np.float32)
        assert xyz.ndim == 3 and xyz.shape[2] == 3 and desc.shape[0] == kp.shape[0]
        return MatchFrame(desc.ctypes.data, kp.ctypes.data, kp.shape[0], xyz.shape[1], xyz.shape[0], xyz.ctypes.data), (desc, kp, xyz)

    def match_pair(self, frame_a: dict, frame_b: dict, Kinv: np.ndarray, read_sets: bool = True) -> dict:
        """The whole stage for frames dict(desc (n, 32) uint8, kp (n, 2) float32, xyz (H, W, 3) float32).  The five sets stay on the
        device for pnp_matched / icp_matched; read_sets also copies them out (chip_match_read_sets)."""
        fa, keep_a = self._match_frame(frame_a)
        fb, keep_b = self._match_frame(frame_b)
        Ki = np.ascontiguousarray(Kinv, dtype=np.float64).reshape(9)
        sm = MatchSummary()
        self._chk(self.lib.chip_match_pair(self.h, C.byref(fa), C.byref(fb), _ptr(Ki), C.byref(sm)), "chip_match_pair")
        out = dict(summary=sm.as_dict())
        if read_sets:
            out.update(self.match_read_sets(sm))
        return out

    def match_read_sets(self, sm: MatchSummary) -> dict:
        g, ab, ba, dd = sm.n_matches_gms, sm.n_3d2d_ab, sm.n_3d2d_ba, sm.n_3d3d
        shapes = dict(uv=(g, 2), uv_d=(g, 2), X_ab=(ab, 3), uvn_ab=(ab, 2), X_ba=(ba, 3), uvn_ba=(ba, 2), A_3d3d=(dd, 3), B_3d3d=(dd, 3))
        arrs = {k: np.full(shp, np.nan, dtype=np.float64) for k, shp in shapes.items()}
        arrs["match_query_idx"] = np.full(g, -1, dtype=np.int32)
        arrs["match_train_idx"] = np.full(g, -1, dtype=np.int32)
        o = MatchSetsOut(**{k: (v.ctypes.data if v.size else None) for k, v in arrs.items()})
        self._chk(self.lib.chip_match_read_sets(self.h, C.byref(o)), "chip_match_read_sets")
        return arrs

    def _matched(self, st: int, where: str, N: int, T, conf, mask, summ):
        if st == CHIP_ERR_TOO_FEW_POINTS:
            return dict(status=st, confidence=-1.0, T=None, mask=None, summary=None)
        self._chk(st, where)
        return dict(status=st, confidence=float(conf.value), T=T.reshape(4, 4).T.copy(), mask=mask[:N].copy(),
                    summary=dict(n_iterations=summ.n_iterations, n_inliers=summ.n_inliers, best_hypothesis=summ.best_hypothesis,
                                 n_models=summ.n_models, best_cost=summ.best_cost))

    def pnp_matched(self, which: int, N: int, params: RansacParams | None = None):
        """chip_pnp_ransac on the device-resident set `which` (CHIP_SET_AB / CHIP_SET_BA) of the last match_pair; N = that set's count"""
        p = params or default_ransac_params()
        T = np.empty(16, dtype=np.float64)
        conf = C.c_float()
        mask = np.zeros(max(N, 1), dtype=np.uint8)
        summ = RansacSummary()
        st = self.lib.chip_pnp_ransac_matched(self.h, which, C.byref(p), _ptr(T), C.byref(conf), _ptr(mask), C.byref(summ))
        return self._matched(st, "chip_pnp_ransac_matched", N, T, conf, mask, summ)

    def icp_matched(self, N: int, params: RansacParams | None = None):
        """chip_icp_ransac on the device-resident 3d-3d set of the last match_pair; N = n_3d3d"""
        p = params or default_icp_params()
        T = np.empty(16, dtype=np.float64)
        conf = C.c_float()
        mask = np.zeros(max(N, 1), dtype=np.uint8)
        summ = RansacSummary()
        st = self.lib.chip_icp_ransac_matched(self.h, C.byref(p), _ptr(T), C.byref(conf), _ptr(mask), C.byref(summ))
        return self._matched(st, "chip_icp_ransac_matched", N, T, conf, mask, summ)

    # -- one query frame against several candidate frames
    def match_batch(self, frame_a: dict, frames_b, Kinv: np.ndarray, modes=None):
        """chip_match_batch: frame_a against every frame of frames_b (at most CHIP_MATCH_MAX_BATCH) -> the list of MatchSummary, one
        per candidate.  The sets of all candidates stay on the device; candidate 0 is selected (match_select).
        modes (CHIP_GMS_WITH_SCALE | CHIP_GMS_WITH_ROTATION, or 0): chip_match_batch_modes -> (summaries, list of choice dicts)"""
        fa, keep_a = self._match_frame(frame_a)
        made = [self._match_frame(f) for f in frames_b]
        B = len(made)
        fb = (MatchFrame * max(B, 1))(*[m[0] for m in made])
        Ki = np.ascontiguousarray(Kinv, dtype=np.float64).reshape(9)
        sm = (MatchSummary * max(B, 1))()
        if modes is not None:
            ch = (GmsChoice * max(B, 1))()
            self._chk(self.lib.chip_match_batch_modes(self.h, C.byref(fa), fb, B, _ptr(Ki), modes, sm, ch), "chip_match_batch_modes")
            self._match_batch_n1 = fa.n
            return [MatchSummary.from_buffer_copy(sm[j]) for j in range(B)], [ch[j].as_dict() for j in range(B)]
        self._chk(self.lib.chip_match_batch(self.h, C.byref(fa), fb, B, _ptr(Ki), sm), "chip_match_batch")
        self._match_batch_n1 = fa.n
        return [MatchSummary.from_buffer_copy(sm[j]) for j in range(B)]

    def match_select(self, j: int):
        """make candidate j of the last match_batch the one match_read_sets / pnp_matched / icp_matched work on"""
        self._chk(self.lib.chip_match_select(self.h, j), "chip_match_select")

    def match_batch_matches(self, j: int):
        """-> (train_idx, distance) int32 of candidate j of the last match_batch: the brute-force matches before GMS"""
        n1 = getattr(self, "_match_batch_n1", 0)
        if isinstance(n1, list):                  # after match_pairs_stored: every pair has a query frame of its own
            n1 = n1[j] if 0 <= j < len(n1) else 0
        idx = np.full(max(n1, 1), -1, dtype=np.int32)
        dist = np.full(max(n1, 1), -1, dtype=np.int32)
        self._chk(self.lib.chip_match_batch_read_matches(self.h, j, _ptr(idx), _ptr(dist)), "chip_match_batch_read_matches")
        return idx[:n1].copy(), dist[:n1].copy()

    def pnp_matched_batch(self, problems, params: RansacParams | None = None, seeds=None) -> list:
        """chip_pnp_ransac_matched_batch.  problems: list of (candidate, which, N) with N = that set's count (it sizes the mask).
        Entry i is what pnp_matched(which, N) returns after match_select(candidate) with seed seeds[i] (default: params.seed)."""
        P = len(problems)
        p = params or default_ransac_params()
        cand = np.array([q[0] for q in problems], dtype=np.int32).reshape(P)
        which = np.array([q[1] for q in problems], dtype=np.int32).reshape(P)
        Ns = [int(q[2]) for q in problems]
        T = np.empty((max(P, 1), 16), dtype=np.float64)
        conf = np.zeros(max(P, 1), dtype=np.float32)
        masks = [np.zeros(max(n, 1), dtype=np.uint8) for n in Ns]
        mp = (C.c_void_p * max(P, 1))(*[m.ctypes.data for m in masks])
        summ = (RansacSummary * max(P, 1))()
        status = np.zeros(max(P, 1), dtype=np.int32)
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        self._chk(self.lib.chip_pnp_ransac_matched_batch(self.h, P, _ptr(cand), _ptr(which), C.byref(p), None if sd is None else _ptr(sd), _ptr(T),
                                                         _ptr(conf), mp, summ, _ptr(status)), "chip_pnp_ransac_matched_batch")
        out = []
        for i in range(P):
            cf, s = C.c_float(float(conf[i])), RansacSummary.from_buffer_copy(summ[i])
            out.append(self._matched(int(status[i]), "chip_pnp_ransac_matched_batch", Ns[i], T[i], cf, masks[i], s))
        return out

    def _icp_batch_out(self, Ns, status, T, conf, masks, summ) -> list:
        out = []
        for i in range(len(Ns)):
            cf, s = C.c_float(float(conf[i])), RansacSummary.from_buffer_copy(summ[i])
            r = self._matched(int(status[i]), "chip_icp_ransac_matched_batch", Ns[i], T[i], cf, masks[i], s)
            if status[i] != 0:
                r["raw"] = dict(T=T[i].copy(), confidence=float(conf[i]), mask=masks[i].copy(),
                                summary=dict(n_iterations=s.n_iterations, n_inliers=s.n_inliers, best_hypothesis=s.best_hypothesis,
                                             n_models=s.n_models, best_cost=s.best_cost))
            out.append(r)
        return out

    def icp_matched_batch_enqueue(self, problems, params: RansacParams | None = None, seeds=None):
        """chip_icp_ransac_matched_batch_enqueue.  problems: list of (candidate, N) with N = that candidate's n_3d3d (it sizes the mask).
        Returns at once with the ticket icp_matched_batch_collect takes."""
        P = len(problems)
        p = params or default_icp_params()
        cand = np.array([q[0] for q in problems], dtype=np.int32).reshape(P)
        status = np.zeros(max(P, 1), dtype=np.int32)
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        self._chk(self.lib.chip_icp_ransac_matched_batch_enqueue(self.h, P, _ptr(cand), C.byref(p), None if sd is None else _ptr(sd), _ptr(status)),
                  "chip_icp_ransac_matched_batch_enqueue")
        return dict(Ns=[int(q[1]) for q in problems], status=status)

    def icp_matched_batch_collect(self, ticket) -> list:
        """chip_icp_ransac_matched_batch_collect -> entry i is what icp_matched(N) returns after match_select(candidate) with that seed;
        a left-out problem (status CHIP_ERR_TOO_FEW_POINTS) additionally carries `raw`: the T, confidence, summary and mask as delivered"""
        Ns, status = ticket["Ns"], ticket["status"]
        P = len(Ns)
        T = np.zeros((max(P, 1), 16), dtype=np.float64)
        conf = np.zeros(max(P, 1), dtype=np.float32)
        masks = [np.full(max(n, 1), 0xAB, dtype=np.uint8) for n in Ns]
        mp = (C.c_void_p * max(P, 1))(*[m.ctypes.data for m in masks])
        summ = (RansacSummary * max(P, 1))()
        self._chk(self.lib.chip_icp_ransac_matched_batch_collect(self.h, _ptr(T), _ptr(conf), mp, summ), "chip_icp_ransac_matched_batch_collect")
        return self._icp_batch_out(Ns, status, T, conf, masks, summ)

    def icp_matched_batch(self, problems, params: RansacParams | None = None, seeds=None) -> list:
        """chip_icp_ransac_matched_batch (enqueue + collect in one call); see icp_matched_batch_enqueue / _collect"""
        P = len(problems)
        p = params or default_icp_params()
        cand = np.array([q[0] for q in problems], dtype=np.int32).reshape(P)
        Ns = [int(q[1]) for q in problems]
        T = np.zeros((max(P, 1), 16), dtype=np.float64)
        conf = np.zeros(max(P, 1), dtype=np.float32)
        masks = [np.full(max(n, 1), 0xAB, dtype=np.uint8) for n in Ns]
        mp = (C.c_void_p * max(P, 1))(*[m.ctypes.data for m in masks])
        summ = (RansacSummary * max(P, 1))()
        status = np.zeros(max(P, 1), dtype=np.int32)
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        self._chk(self.lib.chip_icp_ransac_matched_batch(self.h, P, _ptr(cand), C.byref(p), None if sd is None else _ptr(sd), _ptr(T), _ptr(conf), mp,
                                                         summ, _ptr(status)), "chip_icp_ransac_matched_batch")
        return self._icp_batch_out(Ns, status, T, conf, masks, summ)

    # -- frames kept on the device (the frame store)
    def frame_store_reserve(self, n_slots: int, slot_keypoints: int):
        """chip_frame_store_reserve: n_slots slots of slot_keypoints keypoints each, 56 bytes of device memory per keypoint"""
        self._chk(self.lib.chip_frame_store_reserve(self.h, n_slots, slot_keypoints), "chip_frame_store_reserve")

    def frame_store_info(self) -> dict:
        v = [C.c_int32() for _ in range(3)]
        self._chk(self.lib.chip_frame_store_info(self.h, *[C.byref(x) for x in v]), "chip_frame_store_info")
        return dict(n_slots=v[0].value, slot_keypoints=v[1].value, n_frames=v[2].value)

    def frame_put(self, id: int, frame: dict):
        """chip_frame_put: store (or replace) the frame dict(desc, kp, xyz) under id; the arrays are free again on return"""
        f, keep = self._match_frame(frame)
        self._chk(self.lib.chip_frame_put(self.h, id, C.byref(f)), "chip_frame_put")

    @staticmethod
    def _disparity(disparity):
        """-> (contiguous (H, W) int16 or float32 array, CHIP_DISP_*): int16 (CV_16SC1) stays, every other dtype goes as float32"""
        d = np.asarray(disparity)
        d = np.ascontiguousarray(d, dtype=np.int16 if d.dtype == np.int16 else np.float32)
        assert d.ndim == 2
        return d, CHIP_DISP_S16 if d.dtype == np.int16 else CHIP_DISP_F32

    def frame_put_disparity(self, id: int, frame: dict, disparity, Q: np.ndarray):
        """chip_frame_put_disparity: store (or replace) the frame dict(desc, kp) under id with the 3-D points of its keypoints computed
        on the device from the (H, W) disparity (int16: CV_16SC1 raw, otherwise float32 in the same units) and the 4 x 4 Q"""
        desc = np.ascontiguousarray(frame["desc"], dtype=np.uint8).reshape(-1, CHIP_ORB_DESC_BYTES)
        kp = np.ascontiguousarray(frame["kp"], dtype=np.float32).reshape(-1, 2)
        assert desc.shape[0] == kp.shape[0]
        d, kind = self._disparity(disparity)
        Qd = np.ascontiguousarray(Q, dtype=np.float64).reshape(16)
        self._chk(self.lib.chip_frame_put_disparity(self.h, id, _ptr(desc), _ptr(kp), kp.shape[0], d.shape[1], d.shape[0], _ptr(d), kind, _ptr(Qd)),
                  "chip_frame_put_disparity")

    def disparity_to_xyz(self, disparity, Q: np.ndarray) -> np.ndarray:
        """chip_disparity_to_xyz -> the (H, W, 3) float32 3-D image of the (H, W) disparity under the 4 x 4 Q"""
        d, kind = self._disparity(disparity)
        Qd = np.ascontiguousarray(Q, dtype=np.float64).reshape(16)
        xyz = np.zeros(d.shape + (3,), dtype=np.float32)
        self._chk(self.lib.chip_disparity_to_xyz(self.h, _ptr(d), kind, d.shape[1], d.shape[0], _ptr(Qd), _ptr(xyz)), "chip_disparity_to_xyz")
        return xyz

    @staticmethod
    def _stereo_pair(left, right, params):
        """-> (contiguous (H, W) uint8 left, right, the parameter pointer or None): params a StereoBmParams, a dict of its fields or None"""
        l, r = np.ascontiguousarray(left, dtype=np.uint8), np.ascontiguousarray(right, dtype=np.uint8)
        assert l.ndim == 2 and l.shape == r.shape
        if isinstance(params, dict):
            params = default_stereo_bm_params(**params)
        return l, r, None if params is None else C.byref(params)

    def stereo_bm(self, left, right, params=None) -> np.ndarray:
        """chip_stereo_bm -> the (H, W) int16 disparity (sixteenths of a pixel, -16: none) of the rectified (H, W) uint8 pair"""
        l, r, p = self._stereo_pair(left, right, params)
        disp = np.zeros(l.shape, dtype=np.int16)
        self._chk(self.lib.chip_stereo_bm(self.h, _ptr(l), _ptr(r), l.shape[1], l.shape[0], p, _ptr(disp)), "chip_stereo_bm")
        return disp

    def frame_put_stereo(self, id: int, frame: dict, left, right, Q: np.ndarray, params=None):
        """chip_frame_put_stereo: store (or replace) the frame dict(desc, kp) under id with the 3-D points of its keypoints computed on
        the device from the rectified (H, W) uint8 pair (block matcher at the keypoints) and the 4 x 4 Q"""
        desc = np.ascontiguousarray(frame["desc"], dtype=np.uint8).reshape(-1, CHIP_ORB_DESC_BYTES)
        kp = np.ascontiguousarray(frame["kp"], dtype=np.float32).reshape(-1, 2)
        assert desc.shape[0] == kp.shape[0]
        l, r, p = self._stereo_pair(left, right, params)
        Qd = np.ascontiguousarray(Q, dtype=np.float64).reshape(16)
        self._chk(self.lib.chip_frame_put_stereo(self.h, id, _ptr(desc), _ptr(kp), kp.shape[0], l.shape[1], l.shape[0], _ptr(l), _ptr(r), p, _ptr(Qd)),
                  "chip_frame_put_stereo")

    def orb_detect(self, image, params=None):
        """chip_orb_detect on the (H, W) uint8 image -> (the records as an ORB_KEYPOINT_DTYPE array, level_counts[8]); params an
        OrbParams, a dict of its fields or None"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        assert img.ndim == 2
        params, p = _orb_params(params)
        cap = CHIP_ORB_N_FEATURES if params is None else max(int(params.n_features), 1)
        kp = np.zeros(cap, dtype=ORB_KEYPOINT_DTYPE)
        n = C.c_int32()
        counts = (C.c_int32 * CHIP_ORB_MAX_LEVELS)()
        self._chk(self.lib.chip_orb_detect(self.h, _ptr(img), img.shape[1], img.shape[0], p, _ptr(kp), cap, C.byref(n), counts), "chip_orb_detect")
        return kp[:n.value].copy(), list(counts)

    def orb_level(self, level: int, width: int, height: int):
        """chip_debug_orb_level -> (the (height, width) uint8 pyramid level, the (height, width) int16 FAST score plane, -256 where the
        score is not defined) the last orb_detect left behind; width and height are that level's (orb_plan)"""
        img = np.zeros((height, width), dtype=np.uint8)
        score = np.zeros((height, width), dtype=np.int16)
        self._chk(self.lib.chip_debug_orb_level(self.h, level, _ptr(img) if img.size else None, _ptr(score) if score.size else None),
                  "chip_debug_orb_level")
        return img, score

    def orb_detect_describe(self, image, params=None):
        """chip_orb_detect_describe on the (H, W) uint8 image -> (the records of orb_detect, level_counts[8], the (n, 32) uint8
        descriptors, row i that of record i)"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        assert img.ndim == 2
        params, p = _orb_params(params)
        cap = CHIP_ORB_N_FEATURES if params is None else max(int(params.n_features), 1)
        kp = np.zeros(cap, dtype=ORB_KEYPOINT_DTYPE)
        desc = np.zeros((cap, CHIP_ORB_DESC_BYTES), dtype=np.uint8)
        n = C.c_int32()
        counts = (C.c_int32 * CHIP_ORB_MAX_LEVELS)()
        self._chk(self.lib.chip_orb_detect_describe(self.h, _ptr(img), img.shape[1], img.shape[0], p, _ptr(kp), cap, C.byref(n), counts, _ptr(desc)),
                  "chip_orb_detect_describe")
        return kp[:n.value].copy(), list(counts), desc[:n.value].copy()

    def orb_blur(self, level: int, width: int, height: int) -> np.ndarray:
        """chip_debug_orb_blur -> the (height, width) uint8 blurred plane of a level the last orb_detect_describe or
        frame_put_orb_stereo left behind; width and height are that level's (orb_plan)"""
        out = np.zeros((height, width), dtype=np.uint8)
        self._chk(self.lib.chip_debug_orb_blur(self.h, level, _ptr(out) if out.size else None), "chip_debug_orb_blur")
        return out

    def frame_put_orb_stereo(self, id: int, left, right, Q: np.ndarray, orb=None, bm=None) -> int:
        """chip_frame_put_orb_stereo: store (or replace) under id the frame the detector and the descriptor make of the rectified (H, W)
        uint8 left image, with the 3-D points the block matcher makes at its keypoints -> the number of keypoints kept"""
        l, r, b = self._stereo_pair(left, right, bm)
        _, o = _orb_params(orb)
        Qd = np.ascontiguousarray(Q, dtype=np.float64).reshape(16)
        n = C.c_int32()
        self._chk(self.lib.chip_frame_put_orb_stereo(self.h, id, l.shape[1], l.shape[0], _ptr(l), _ptr(r), o, b, _ptr(Qd), C.byref(n)),
                  "chip_frame_put_orb_stereo")
        return n.value

    def remap(self, image, map_x, map_y) -> np.ndarray:
        """chip_remap -> the (H, W) uint8 image sampled through the (H, W) float32 maps: one stage of the rectification's definition"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        mx, my = np.ascontiguousarray(map_x, dtype=np.float32), np.ascontiguousarray(map_y, dtype=np.float32)
        assert img.ndim == 2 and mx.shape == img.shape and my.shape == img.shape
        out = np.zeros(img.shape, dtype=np.uint8)
        self._chk(self.lib.chip_remap(self.h, _ptr(img), img.shape[1], img.shape[0], _ptr(mx), _ptr(my), _ptr(out)), "chip_remap")
        return out

    def rectify_set_maps(self, left, right):
        """chip_rectify_set_maps: left and right are (x1, y1) for one stage or (x1, y1, x2, y2) for two, (H, W) float32 maps each (the
        reference's map_x, map_y, map1_x, map1_y and map_x, map_y, map2_x, map2_y); they replace the maps the ctx had"""
        if len(left) != len(right) or len(left) not in (2, 4):
            raise ValueError("rectify_set_maps: two or four maps per eye, as many left as right")
        maps = [np.ascontiguousarray(m, dtype=np.float32) for m in tuple(left) + tuple(right)]
        assert maps[0].ndim == 2 and all(m.shape == maps[0].shape for m in maps)
        k = len(left)
        p = [_ptr(m) for m in maps[:k]] + [None] * (4 - k) + [_ptr(m) for m in maps[k:]] + [None] * (4 - k)
        self._chk(self.lib.chip_rectify_set_maps(self.h, maps[0].shape[1], maps[0].shape[0], *p), "chip_rectify_set_maps")

    def rectify_pair(self, left_raw, right_raw):
        """chip_rectify_pair -> (left, right): the (H, W) uint8 raw pair through the ctx's maps"""
        l, r, _ = self._stereo_pair(left_raw, right_raw, None)
        lo, ro = np.zeros(l.shape, dtype=np.uint8), np.zeros(l.shape, dtype=np.uint8)
        self._chk(self.lib.chip_rectify_pair(self.h, _ptr(l), _ptr(r), l.shape[1], l.shape[0], _ptr(lo), _ptr(ro)), "chip_rectify_pair")
        return lo, ro

    def frame_put_raw_orb_stereo(self, id: int, left_raw, right_raw, Q: np.ndarray, orb=None, bm=None) -> int:
        """chip_frame_put_raw_orb_stereo: frame_put_orb_stereo with the cameras' raw (H, W) uint8 pair, rectified on the device through
        the ctx's maps -> the number of keypoints kept"""
        l, r, b = self._stereo_pair(left_raw, right_raw, bm)
        _, o = _orb_params(orb)
        Qd = np.ascontiguousarray(Q, dtype=np.float64).reshape(16)
        n = C.c_int32()
        self._chk(self.lib.chip_frame_put_raw_orb_stereo(self.h, id, l.shape[1], l.shape[0], _ptr(l), _ptr(r), o, b, _ptr(Qd), C.byref(n)),
                  "chip_frame_put_raw_orb_stereo")
        return n.value

    def _frame_put_batch(self, fn, name: str, ids, lefts, rights, Q, orb, bm) -> list:
        idv = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        F = len(idv)
        if len(lefts) != F or len(rights) != F:
            raise ValueError(f"{name}: as many left and right images as ids")
        ls = [np.ascontiguousarray(a, dtype=np.uint8) for a in lefts]
        rs = [np.ascontiguousarray(a, dtype=np.uint8) for a in rights]
        shape = ls[0].shape if F else (0, 0)
        assert all(a.ndim == 2 and a.shape == shape for a in ls + rs), "every image of a call has one (H, W)"
        _, o = _orb_params(orb)
        if isinstance(bm, dict):
            bm = default_stereo_bm_params(**bm)
        lp = (C.c_void_p * max(F, 1))(*[a.ctypes.data for a in ls])
        rp = (C.c_void_p * max(F, 1))(*[a.ctypes.data for a in rs])
        Qd = np.ascontiguousarray(Q, dtype=np.float64).reshape(16)
        n = np.full(max(F, 1), -2, dtype=np.int32)
        self._chk(fn(self.h, _ptr(idv) if F else None, F, shape[1], shape[0], lp, rp, o, None if bm is None else C.byref(bm), _ptr(Qd), _ptr(n)), name)
        return [int(v) for v in n[:F]]

    def frame_put_orb_stereo_batch(self, ids, lefts, rights, Q: np.ndarray, orb=None, bm=None) -> list:
        """chip_frame_put_orb_stereo_batch: frame_put_orb_stereo for F rectified pairs of one rig in one call -- every stage one launch
        per group of frames, one host wait per group -> the F kept counts.  The stored rows equal the single call's byte for byte"""
        return self._frame_put_batch(self.lib.chip_frame_put_orb_stereo_batch, "chip_frame_put_orb_stereo_batch", ids, lefts, rights, Q, orb, bm)

    def frame_put_raw_orb_stereo_batch(self, ids, lefts_raw, rights_raw, Q: np.ndarray, orb=None, bm=None) -> list:
        """chip_frame_put_raw_orb_stereo_batch: the same with the cameras' raw pairs, rectified on the device through the ctx's maps"""
        return self._frame_put_batch(self.lib.chip_frame_put_raw_orb_stereo_batch, "chip_frame_put_raw_orb_stereo_batch", ids, lefts_raw, rights_raw,
                                     Q, orb, bm)

    def frame_put_records(self, id: int, frame: dict):
        """chip_frame_put_records: what frame_read gave -- dict(desc, kp, pts, width, height) -- back into the store under id: three
        uploads, no kernel.  The fourth float of every record must be 0.0 or 1.0"""
        desc = np.ascontiguousarray(frame["desc"], dtype=np.uint8).reshape(-1, CHIP_ORB_DESC_BYTES)
        kp = np.ascontiguousarray(frame["kp"], dtype=np.float32).reshape(-1, 2)
        pts = np.ascontiguousarray(frame["pts"], dtype=np.float32).reshape(-1, 4)
        assert desc.shape[0] == kp.shape[0] == pts.shape[0]
        keep = np.zeros(4, dtype=np.float32)                          # an empty frame still hands over three addresses
        a = [_ptr(x) if x.size else _ptr(keep) for x in (desc, kp, pts)]
        self._chk(self.lib.chip_frame_put_records(self.h, id, *a, kp.shape[0], int(frame["width"]), int(frame["height"])), "chip_frame_put_records")

    def frame_put_last(self) -> dict:
        """chip_debug_frame_put_last -> dict(groups, launches, waits) of the ctx's last batched put"""
        v = [C.c_int32() for _ in range(3)]
        self._chk(self.lib.chip_debug_frame_put_last(self.h, *[C.byref(x) for x in v]), "chip_debug_frame_put_last")
        return dict(groups=v[0].value, launches=v[1].value, waits=v[2].value)

    def frame_drop(self, id: int):
        self._chk(self.lib.chip_frame_drop(self.h, id), "chip_frame_drop")

    def frame_read(self, id: int) -> dict:
        """chip_frame_read -> dict(n, width, height, desc (n, 32) uint8, kp (n, 2) float32, pts (n, 4) float32: the point records)"""
        v = [C.c_int32() for _ in range(3)]
        self._chk(self.lib.chip_frame_read(self.h, id, *[C.byref(x) for x in v], None, None, None), "chip_frame_read")
        n = v[0].value
        desc = np.zeros((n, CHIP_ORB_DESC_BYTES), dtype=np.uint8)
        kp = np.zeros((n, 2), dtype=np.float32)
        pts = np.zeros((n, 4), dtype=np.float32)
        if n:
            self._chk(self.lib.chip_frame_read(self.h, id, None, None, None, _ptr(desc), _ptr(kp), _ptr(pts)), "chip_frame_read")
        return dict(n=n, width=v[1].value, height=v[2].value, desc=desc, kp=kp, pts=pts)

    def match_batch_stored(self, a_id: int, b_ids, Kinv: np.ndarray, modes=None):
        """chip_match_batch_stored: the stored frame a_id against the stored frames b_ids, nothing uploaded -> what match_batch returns
        on the host frames that were put under those ids; match_select / match_read_sets / match_batch_matches and the _matched
        solvers work on the result.  modes (or 0): chip_match_batch_stored_modes -> (summaries, list of choice dicts)"""
        ids = np.ascontiguousarray(b_ids, dtype=np.int64).reshape(-1)
        B = len(ids)
        Ki = np.ascontiguousarray(Kinv, dtype=np.float64).reshape(9)
        sm = (MatchSummary * max(B, 1))()
        self._match_batch_n1 = 0
        ch = (GmsChoice * max(B, 1))()
        if modes is not None:
            self._chk(self.lib.chip_match_batch_stored_modes(self.h, a_id, _ptr(ids) if B else None, B, _ptr(Ki), modes, sm, ch),
                      "chip_match_batch_stored_modes")
        else:
            self._chk(self.lib.chip_match_batch_stored(self.h, a_id, _ptr(ids) if B else None, B, _ptr(Ki), sm), "chip_match_batch_stored")
        n1 = C.c_int32()
        self._chk(self.lib.chip_frame_read(self.h, a_id, C.byref(n1), None, None, None, None, None), "chip_frame_read")
        self._match_batch_n1 = n1.value
        summaries = [MatchSummary.from_buffer_copy(sm[j]) for j in range(B)]
        return (summaries, [ch[j].as_dict() for j in range(B)]) if modes is not None else summaries

    def match_pairs_stored(self, a_ids, b_ids, Kinv: np.ndarray, modes=None):
        """chip_match_pairs_stored: the stored frames a_ids[j] against b_ids[j], pair by pair in the launches of one batch -> what
        match_batch_stored returns, with the pair index in the place of the candidate's (match_select / match_read_sets /
        match_batch_matches and the _matched solvers).  modes (or 0): -> (summaries, list of choice dicts)"""
        ia = np.ascontiguousarray(a_ids, dtype=np.int64).reshape(-1)
        ib = np.ascontiguousarray(b_ids, dtype=np.int64).reshape(-1)
        if len(ia) != len(ib):
            raise ValueError("match_pairs_stored: a_ids and b_ids differ in length")
        P = len(ia)
        Ki = np.ascontiguousarray(Kinv, dtype=np.float64).reshape(9)
        sm = (MatchSummary * max(P, 1))()
        ch = (GmsChoice * max(P, 1))()
        self._match_batch_n1 = 0
        self._chk(self.lib.chip_match_pairs_stored(self.h, _ptr(ia) if P else None, _ptr(ib) if P else None, P, _ptr(Ki), modes or 0, sm, ch),
                  "chip_match_pairs_stored")
        n1 = []
        for a in ia:
            n = C.c_int32()
            self._chk(self.lib.chip_frame_read(self.h, int(a), C.byref(n), None, None, None, None, None), "chip_frame_read")
            n1.append(n.value)
        self._match_batch_n1 = n1
        summaries = [MatchSummary.from_buffer_copy(sm[j]) for j in range(P)]
        return (summaries, [ch[j].as_dict() for j in range(P)]) if modes is not None else summaries

    # -- introspection / profiling
    def info(self) -> dict:
        i = Info()
        self._chk(self.lib.chip_get_info(self.h, C.byref(i)), "chip_get_info")
        return {k: (getattr(i, k).decode() if k == "arch" else getattr(i, k)) for k, _ in Info._fields_}

    def profile_enable(self, on: bool = True):
        self._chk(self.lib.chip_profile_enable(self.h, 1 if on else 0), "chip_profile_enable")

    def profile_reset(self):
        self._chk(self.lib.chip_profile_reset(self.h), "chip_profile_reset")

    def profile_scan(self):
        ms, n, b, span = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        self._chk(self.lib.chip_profile_scan(self.h, C.byref(ms), C.byref(n), C.byref(b), C.byref(span)), "chip_profile_scan")
        return ms.value, n.value, b.value, span.value
