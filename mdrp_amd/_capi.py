"""ctypes binding of libmdrp_hip.so (include/mdrp.h) — the only route from Python to the HIP kernels.

There is no CPU fallback: if the shared library is missing or no gfx950 device is usable, every entry point
raises.  Build with `python -c "import __graft_entry__ as g; g.build()"` (or mdrp_amd/build.py).
"""
import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MDRP_LIB") or os.path.join(_HERE, "libmdrp_hip.so")  # MDRP_LIB: experiment builds (tools/)

CALIB, SHARED_FOCAL, VARYING_FOCAL = 0, 1, 2
RELPOSE_5PT, SHARED_6PT, FUNDAMENTAL_7PT = 3, 4, 5  # non-monodepth baselines (d1 = d2 = None)
MEM_HOST, MEM_DEVICE = 0, 1
SOLVER_P3P, SOLVER_SHIFT, SOLVER_SHARED, SOLVER_VARYING = 0, 1, 2, 3

DENSE_COORDS = {"normalized": 0, "pixel": 1}  # mdrp_dense_matches.coords (include/mdrp_dense.h MDRP_DENSE_*)
DENSE_MAX_ROWS, DENSE_MAX_STAGE1, DENSE_MAX_N, DENSE_MAX_GRID = 1 << 22, 65536, 16384, 8  # include/mdrp_dense.h MDRP_DENSE_MAX_*
RECON_KEEP = {"not_inf": 0, "finite": 1}  # mdrp_reconstruct_opt.keep (include/mdrp_reconstruct.h MDRP_KEEP_*)
RECON_MAX_EXTENT, RECON_ALL = 65536, 0xFFFFFFFF  # include/mdrp_reconstruct.h MDRP_RECON_MAX_EXTENT, MDRP_RECON_ALL
FOCAL_NO_MODEL, FOCAL_F1_NOT_REAL, FOCAL_F2_NOT_REAL, FOCAL_NO_VOTERS = 1, 2, 4, 8  # include/mdrp_classic_focals.h MDRP_FOCAL_*: mdrp_focal_pose.status
# include/mdrp.h MDRP_RETIRE_*: flags of mdrp_retire_models
RETIRE_TWO_PHASE, RETIRE_BOUND, RETIRE_SWEEP_SCORE, RETIRE_SWEEP_SPLIT, RETIRE_SWEEP_WAVE = 1, 2, 0, 4, 8
STAGE_LO, STAGE_INLIERS = 1, 2  # include/mdrp.h MDRP_STAGE_*: the stages of mdrp_refine_batch
MAX_BUDGETS = 16  # include/mdrp.h MDRP_MAX_BUDGETS
F32, F64 = 0, 1  # mdrp_matches.kp_type / depth_type
FILTERS = {"both_inf": 0, "finite": 1}  # mdrp_matches.filter (include/mdrp.h MDRP_FILTER_*)


class Model(C.Structure):
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("scale", C.c_double), ("shift1", C.c_double),
                ("shift2", C.c_double), ("f1", C.c_double), ("f2", C.c_double)]


class RansacOpt(C.Structure):
    _fields_ = [("max_iterations", C.c_uint64), ("min_iterations", C.c_uint64), ("dyn_num_trials_mult", C.c_double),
                ("success_prob", C.c_double), ("max_reproj_error", C.c_double), ("max_epipolar_error", C.c_double),
                ("seed", C.c_uint64), ("monodepth_estimate_shift", C.c_int32), ("monodepth_weight_sampson", C.c_float),
                ("score_initial_model", C.c_int32), ("progressive_sampling", C.c_int32), ("max_prosac_iterations", C.c_uint64),
                ("real_focal_check", C.c_int32), ("reserved_", C.c_int32)]


class BundleOpt(C.Structure):
    _fields_ = [("max_iterations", C.c_uint64), ("loss_type", C.c_int32), ("loss_scale", C.c_double),
                ("gradient_tol", C.c_double), ("step_tol", C.c_double), ("initial_lambda", C.c_double),
                ("min_lambda", C.c_double), ("max_lambda", C.c_double)]


class Camera(C.Structure):
    _fields_ = [("model_id", C.c_int32), ("pad_", C.c_int32), ("params", C.c_double * 4)]


class Stats(C.Structure):
    _fields_ = [("count_ms", C.c_double), ("count_launches", C.c_int64), ("sweep_ms", C.c_double), ("sweep_launches", C.c_int64),
                ("evals_algorithmic", C.c_int64), ("evals_mfma", C.c_int64), ("evals_fp64", C.c_int64), ("evals_bound", C.c_int64),
                ("lo_ms", C.c_double), ("lo_launches", C.c_int64), ("final_ms", C.c_double), ("final_launches", C.c_int64),
                ("bound_ms", C.c_double), ("bound_launches", C.c_int64), ("solve_ms", C.c_double), ("solve_launches", C.c_int64),
                ("lm_cost_evals", C.c_int64), ("lm_accum_evals", C.c_int64), ("final_cost_evals", C.c_int64), ("final_accum_evals", C.c_int64),
                ("fuse_gate_timeouts", C.c_int64), ("fuse_wait_timeouts", C.c_int64),  # ABI 0.3 (mdrp_last_stats_sized)
                ("first_chunk", C.c_int64)]  # ABI 0.5


class Matches(C.Structure):
    """mdrp_matches (ABI 0.6): a matcher's output and two depth maps, every pointer in device memory"""
    _fields_ = [("kp1", C.c_void_p), ("kp2", C.c_void_p), ("kp_type", C.c_int32), ("k1", C.c_int32), ("k2", C.c_int32),
                ("matches", C.c_void_p), ("m_max", C.c_int32), ("depth1", C.c_void_p), ("depth2", C.c_void_p), ("depth_type", C.c_int32),
                ("h1", C.c_int32), ("w1", C.c_int32), ("h2", C.c_int32), ("w2", C.c_int32), ("center1", C.c_void_p), ("center2", C.c_void_p),
                ("filter", C.c_int32)]


class ImagePairs(C.Structure):
    """mdrp_image_pairs (within ABI 0.6): per-image keypoint tables and depth maps, pairs as image indices, every pointer in device memory"""
    _fields_ = [("kp", C.c_void_p), ("kp_type", C.c_int32), ("k_max", C.c_int32), ("kp_count", C.c_void_p), ("depth", C.c_void_p),
                ("depth_type", C.c_int32), ("h_max", C.c_int32), ("w_max", C.c_int32), ("size", C.c_void_p), ("center", C.c_void_p),
                ("n_images", C.c_int32), ("pairs", C.c_void_p), ("matches", C.c_void_p), ("m_max", C.c_int32), ("filter", C.c_int32)]


class PointMatches(C.Structure):
    """mdrp_point_matches (include/mdrp_classic_frontend.h): a matcher's output without depth maps, every pointer in device memory"""
    _fields_ = [("kp1", C.c_void_p), ("kp2", C.c_void_p), ("kp_type", C.c_int32), ("k1", C.c_int32), ("k2", C.c_int32),
                ("matches", C.c_void_p), ("m_max", C.c_int32), ("center1", C.c_void_p), ("center2", C.c_void_p)]


class PointImagePairs(C.Structure):
    """mdrp_point_image_pairs (include/mdrp_classic_frontend.h): per-image keypoint tables, pairs as image indices, every pointer in device memory"""
    _fields_ = [("kp", C.c_void_p), ("kp_type", C.c_int32), ("k_max", C.c_int32), ("kp_count", C.c_void_p), ("center", C.c_void_p),
                ("n_images", C.c_int32), ("pairs", C.c_void_p), ("matches", C.c_void_p), ("m_max", C.c_int32)]


class DenseMatches(C.Structure):
    """mdrp_dense_matches (include/mdrp_dense.h): a dense matcher's warp and certainty, two depth maps and the sampler's arguments; every pointer in
    device memory"""
    _fields_ = [("warp", C.c_void_p), ("warp_type", C.c_int32), ("rows", C.c_int32), ("certainty", C.c_void_p), ("certainty_type", C.c_int32),
                ("coords", C.c_int32), ("depth1", C.c_void_p), ("depth2", C.c_void_p), ("depth_type", C.c_int32), ("h1", C.c_int32), ("w1", C.c_int32),
                ("h2", C.c_int32), ("w2", C.c_int32), ("filter", C.c_int32), ("center1", C.c_void_p), ("center2", C.c_void_p), ("n", C.c_int32),
                ("balanced", C.c_int32), ("expansion", C.c_int32), ("grid", C.c_int32), ("min_count", C.c_int32), ("ranked", C.c_int32),
                ("seed", C.c_uint64), ("threshold", C.c_double), ("rows_out", C.c_void_p), ("score_out", C.c_void_p)]


class DepthPairs(C.Structure):
    """mdrp_depth_pairs (include/mdrp_reconstruct.h): two depth maps per pair, every pointer in device memory"""
    _fields_ = [("depth1", C.c_void_p), ("depth2", C.c_void_p), ("depth_type", C.c_int32), ("h1", C.c_int32), ("w1", C.c_int32), ("h2", C.c_int32),
                ("w2", C.c_int32), ("reserved_", C.c_int32), ("center1", C.c_void_p), ("center2", C.c_void_p)]


class DepthImagePairs(C.Structure):
    """mdrp_depth_image_pairs (include/mdrp_reconstruct.h): one depth map per image, pairs as image indices, every pointer in device memory"""
    _fields_ = [("depth", C.c_void_p), ("depth_type", C.c_int32), ("h_max", C.c_int32), ("w_max", C.c_int32), ("n_images", C.c_int32),
                ("size", C.c_void_p), ("center", C.c_void_p), ("pairs", C.c_void_p)]


class ReconstructOpt(C.Structure):
    """mdrp_reconstruct_opt (include/mdrp_reconstruct.h)"""
    _fields_ = [("keep", C.c_int32), ("thr", C.c_uint32), ("seed", C.c_uint64), ("p_max", C.c_int32), ("reserved_", C.c_int32)]


assert C.sizeof(DepthPairs) == 56 and C.sizeof(DepthImagePairs) == 48 and C.sizeof(ReconstructOpt) == 24


class SceneTransform(C.Structure):
    """mdrp_scene_transform (include/mdrp_scene.h): a point X of the image is (R X + t) * (1 / s) in the frame of `root`; depth -1 = absent or detached"""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("s", C.c_double), ("f", C.c_double), ("shift", C.c_double), ("root", C.c_int32),
                ("depth", C.c_int32)]


assert C.sizeof(SceneTransform) == 128
SCENE_ABSENT, SCENE_EDGE, SCENE_ROOT = 0, 1, 2  # include/mdrp_scene.h MDRP_SCENE_*: tree[i][1]


class CovisOpt(C.Structure):
    """mdrp_covis_opt (include/mdrp_covis.h): the subsample (R3's threshold and seed) and the band lo * zt .. hi * zt a consistent depth lies in"""
    _fields_ = [("thr", C.c_uint32), ("reserved_", C.c_int32), ("seed", C.c_uint64), ("lo", C.c_double), ("hi", C.c_double)]


assert C.sizeof(CovisOpt) == 32
COVIS_SLOTS = 8  # include/mdrp_covis.h MDRP_COVIS_SLOTS: counters per direction
COVIS_CLASSES = ("sampled", "front", "inside", "known", "consistent", "occluded", "violating")  # MDRP_COVIS_*: the slot of each class


class FuseOpt(C.Structure):
    """mdrp_fuse_opt (include/mdrp_fuse.h): the scene cloud's options, the number of view columns, C6's band and the gate"""
    _fields_ = [("keep", C.c_int32), ("thr", C.c_uint32), ("seed", C.c_uint64), ("p_max", C.c_int32), ("n_views", C.c_int32), ("lo", C.c_double),
                ("hi", C.c_double), ("min_consistent", C.c_int32), ("max_violating", C.c_int32)]


assert C.sizeof(FuseOpt) == 48
FUSE_MAX_VIEWS = 8  # include/mdrp_fuse.h MDRP_FUSE_MAX_VIEWS: columns of `views`


class Result(C.Structure):
    _fields_ = [("model", Model), ("refinements", C.c_uint64), ("iterations", C.c_uint64), ("num_inliers", C.c_uint64),
                ("inlier_ratio", C.c_double), ("model_score", C.c_double)]


MODEL_DTYPE = np.dtype([("q", "f8", 4), ("t", "f8", 3), ("scale", "f8"), ("shift1", "f8"), ("shift2", "f8"), ("f1", "f8"), ("f2", "f8")])
RESULT_DTYPE = np.dtype([("model", MODEL_DTYPE), ("refinements", "u8"), ("iterations", "u8"), ("num_inliers", "u8"),
                         ("inlier_ratio", "f8"), ("model_score", "f8")])
CAMERA_DTYPE = np.dtype([("model_id", "i4"), ("pad_", "i4"), ("params", "f8", 4)])
# mdrp_focal_pose (include/mdrp_classic_focals.h), 128 bytes
FOCAL_POSE_DTYPE = np.dtype([("model", MODEL_DTYPE), ("votes", "i4", 4), ("voters", "i4"), ("winner", "i4"), ("status", "i4"), ("pad_", "i4")])
assert MODEL_DTYPE.itemsize == C.sizeof(Model) and RESULT_DTYPE.itemsize == C.sizeof(Result) and CAMERA_DTYPE.itemsize == C.sizeof(Camera)

# mdrp_replay_state / mdrp_replay_trigger / mdrp_replay (include/mdrp.h): the bookkeeping train of one super-chunk on caller-given slot tables
REPLAY_STATE_DTYPE = np.dtype([("n", "i4"), ("active", "i4"), ("sq_thr", "f8"), ("best_min_cnt", "u8"), ("best_min_score", "f8"), ("dyn_max_iter", "u8"),
                               ("iterations", "u8"), ("refinements", "u8"), ("num_inliers", "u8"), ("inlier_ratio", "f8"), ("model_score", "f8"),
                               ("best", MODEL_DTYPE)])
REPLAY_TRIGGER_DTYPE = np.dtype([("iter", "u4"), ("k_ref", "i4"), ("k_min", "i4"), ("cnt_min", "i4"), ("score_min", "f8"), ("cnt_ref", "i4"), ("pad_", "i4")])


class Replay(C.Structure):
    _fields_ = [("mps", C.c_int32), ("sample_sz", C.c_int32), ("batch", C.c_int32), ("n_chunks", C.c_int32), ("chunk_start", C.c_uint64),
                ("chunk_lens", C.c_void_p), ("slot_score", C.c_void_p), ("slot_inl", C.c_void_p), ("models", C.c_void_p), ("lo_score", C.c_void_p),
                ("lo_cnt", C.c_void_p), ("lo_models", C.c_void_p), ("budgets", C.c_void_p), ("n_budgets", C.c_int32), ("pad_", C.c_int32),
                ("states", C.c_void_p), ("checkpoints", C.c_void_p), ("triggers", C.c_void_p), ("n_triggers", C.c_void_p), ("scan_cnt", C.c_void_p),
                ("scan_score", C.c_void_p), ("scan_inst", C.c_void_p), ("lo_plan", C.c_void_p), ("n_active", C.c_void_p), ("max_needed", C.c_void_p)]


assert REPLAY_STATE_DTYPE.itemsize == 176 and REPLAY_TRIGGER_DTYPE.itemsize == 32 and C.sizeof(Replay) == 176


class FrontTables(C.Structure):
    """mdrp_front_tables (include/mdrp.h): the first chunk's pick and filter on caller-given lists"""
    _fields_ = [("batch", C.c_int32), ("slots", C.c_int32), ("pick", C.c_int32), ("pad_", C.c_int32), ("n", C.c_void_p), ("active", C.c_void_p),
                ("sq_thr", C.c_void_p), ("count", C.c_void_p), ("tags", C.c_void_p), ("slot_score", C.c_void_p), ("slot_inl", C.c_void_p),
                ("tags_pick", C.c_void_p), ("tags_rest", C.c_void_p), ("tags_out", C.c_void_p), ("pick_count", C.c_void_p), ("rest_count", C.c_void_p),
                ("surv_count", C.c_void_p), ("evals", C.c_void_p)]


assert C.sizeof(FrontTables) == 128
FRONT_PICK_LIMIT = 64  # mdrp_schedule.h sched::FIRST_PICK_LIMIT

# mdrp_front_state / mdrp_front_run (include/mdrp.h): the scheduler's own stages in front of the sweeps, on a caller's chunk list
FRONT_STATE_DTYPE = np.dtype([("n", "i4"), ("table", "i4"), ("active", "i4"), ("n_triggers", "i4"), ("eps", "f8"), ("sq_thr", "f8"), ("scale_reproj", "f8"),
                              ("lo_loss_scale", "f8"), ("final_loss_scale", "f8"), ("norm", "f8"), ("box", "f8", 4), ("cen", "f8", 4), ("best_min_cnt", "u8"),
                              ("best_min_score", "f8"), ("dyn_max_iter", "u8"), ("iterations", "u8"), ("refinements", "u8"), ("num_inliers", "u8"),
                              ("inlier_ratio", "f8"), ("model_score", "f8"), ("best", MODEL_DTYPE)])
FRONT_FILL = 0xA5  # MDRP_FRONT_FILL: the byte every buffer of a front_stages run holds where no kernel wrote
FRONT_FILL_I32 = int(np.frombuffer(bytes([FRONT_FILL] * 4), dtype=np.int32)[0])
FRONT_FILL_U32 = int(np.frombuffer(bytes([FRONT_FILL] * 4), dtype=np.uint32)[0])
SAMPLE_SIZE = {0: 3, 1: 3, 2: 3, 3: 5, 4: 6, 5: 7}    # mdrp_schedule.h sched::sample_size
MODEL_SLOTS = {0: 4, 1: 4, 2: 4, 3: 12, 4: 16, 5: 4}  # mdrp_schedule.h sched::model_slots


class FrontRun(C.Structure):
    _fields_ = [("kind", C.c_int32), ("batch", C.c_int32), ("n_max", C.c_int32), ("n_chunks", C.c_int32), ("slot_iters", C.c_int32), ("pad_", C.c_int32),
                ("x1", C.c_void_p), ("x2", C.c_void_p), ("d1", C.c_void_p), ("d2", C.c_void_p), ("n_per_pair", C.c_void_p), ("cam1", C.c_void_p),
                ("cam2", C.c_void_p), ("chunk_lens", C.c_void_p), ("pts", C.c_void_p), ("dep", C.c_void_p), ("rfrag", C.c_void_p), ("states", C.c_void_p),
                ("table_of_pair", C.c_void_p), ("table_n", C.c_void_p), ("n_tables", C.c_void_p), ("samples", C.c_void_p), ("slot_inl", C.c_void_p),
                ("models", C.c_void_p), ("tags", C.c_void_p), ("model_count", C.c_void_p)]


assert FRONT_STATE_DTYPE.itemsize == 288 and C.sizeof(FrontRun) == 184

# ---- the prototypes: {header: {symbol: argtypes}}, what load_library() declares and what the EXPORTS* tuples below list.  A new entry point is a row
# here, a method of Handle on the staging helpers below, and a case in tests/binding_cases.py.
_i, _p, _u64, _f64 = C.c_int, C.c_void_p, C.c_uint64, C.c_double
_XD = [_p, _p, _p, _p]  # x1, x2, d1, d2
_TAB = [_i, _i, _p, _p, _p]  # batch, n_max, n_per_pair, cam1, cam2
_OPT = [C.POINTER(RansacOpt), C.POINTER(BundleOpt)]


def _gather_args(desc, outs, ranked):
    """a front end's gather: descriptor, (scores, score_type), batch, `outs` device buffers, the counts"""
    return [_p, C.POINTER(desc), *([_p, _i] if ranked else []), _i, *[_p] * outs, _p]


def _front_args(desc, ranked):
    """a front end + estimator: kind, descriptor, (scores, score_type), batch, cam1, cam2, options, mask, the counts"""
    return [_p, _i, C.POINTER(desc), *([_p, _i] if ranked else []), _i, _p, _p, *_OPT, _p, _p]


PROTOTYPES = {
    "mdrp.h": {
        "mdrp_create_": [_i, _p, C.POINTER(_p), _i, _i],
        "mdrp_create_on_stream_": [_i, _p, C.POINTER(_p), _i, _i],
        "mdrp_destroy": [_p],
        "mdrp_synchronize": [_p],
        "mdrp_estimate_batch": [_p, _i, _i, *_XD, *_TAB, *_OPT, _p, _p],
        "mdrp_estimate_batch_async": [_p, _i, *_XD, *_TAB, *_OPT, _p],
        "mdrp_fetch_results": [_p, _p, _i],
        "mdrp_copy_results_device": [_p, _p, _i],
        "mdrp_solver_batch": [_p, _i, *_XD, _i, _p, _p],
        "mdrp_score_models": [_p, _i, _i, _p, _i, _p, _p, _i, _f64, _p, _p],
        "mdrp_count_candidates": [_p, _i, _p, _i, _p, _p, _i, _f64, _p],
        "mdrp_bound_models": [_p, _i, _p, _i, _p, _p, _i, _f64, _p, _p],
        "mdrp_refine_models": [_p, _i, _p, _i, *_XD, _i, _f64, _f64, C.POINTER(BundleOpt), _i, _p],
        "mdrp_last_sweep_stats": [_p, C.POINTER(_f64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
        "mdrp_last_stats": [_p, C.POINTER(Stats)],
        "mdrp_last_stats_sized": [_p, C.POINTER(Stats), C.c_size_t],
        "mdrp_classic_solver_batch": [_p, _i, _p, _p, _i, _p, _p],
        "mdrp_solver_residency": [_i, _i, _i, _u64, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_i)],
        "mdrp_gather_matches": _gather_args(Matches, 5, False),
        "mdrp_estimate_matches_async": _front_args(Matches, False),
        "mdrp_estimate_batch_budgets": [_p, _i, _i, *_XD, *_TAB, *_OPT, _p, _i, _p, _p],
        "mdrp_estimate_batch_budgets_async": [_p, _i, *_XD, *_TAB, *_OPT, _p, _i, _p],
        "mdrp_fetch_budget_results": [_p, _p, _i, _i],
        "mdrp_copy_budget_results_device": [_p, _p, _i, _i],
        "mdrp_refine_batch": [_p, _i, _i, *_XD, *_TAB, *_OPT, _p, _i, _p, _p, _p, _p],
        "mdrp_refine_batch_async": [_p, _i, *_XD, *_TAB, *_OPT, _p, _i, _p, _p, _p],
        "mdrp_gather_image_pairs": _gather_args(ImagePairs, 5, False),
        "mdrp_estimate_image_pairs_async": _front_args(ImagePairs, False),
        "mdrp_estimate_batch_prior": [_p, _i, _i, *_XD, *_TAB, *_OPT, _p, _p, _p],
        "mdrp_estimate_batch_prior_async": [_p, _i, *_XD, *_TAB, *_OPT, _p, _p],
        "mdrp_retire_models": [_p, _i, _p, _i, _p, _p, _i, _f64, _u64, _f64, _p, _i, _p, _p, _p, _p, _p],
        "mdrp_replay_slots": [_p, C.POINTER(RansacOpt), C.POINTER(Replay)],
        "mdrp_front_lists": [_p, C.POINTER(FrontTables)],
        "mdrp_front_models": [_p, _i, _p, _i, _p, _p, _i, _f64, _u64, _f64, _i, _p, _p, _p, _p],
        "mdrp_front_stages": [_p, *_OPT, C.POINTER(FrontRun)],
        "mdrp_estimate_batch_ranked":[_p, _i, _i, *_XD, _p, *_TAB, *_OPT, _p, _p],
        "mdrp_estimate_batch_ranked_async": [_p, _i, *_XD, _p, *_TAB, *_OPT, _p],
        "mdrp_prosac_samples": [_p, _u64, _i, _u64, _p, _i, _p],
        "mdrp_rank_scores": [_p, _i, _p, _i, _i, _p, _p],
        "mdrp_gather_matches_ranked": _gather_args(Matches, 5, True),
        "mdrp_estimate_matches_ranked_async": _front_args(Matches, True),
        "mdrp_gather_image_pairs_ranked": _gather_args(ImagePairs, 5, True),
        "mdrp_estimate_image_pairs_ranked_async": _front_args(ImagePairs, True),
    },
    "mdrp_classic_ranked.h": {  # the 5- / 6- / 7-point baselines in match-score order
        "mdrp_estimate_classic_ranked": [_p, _i, _i, _p, _p, _p, *_TAB, *_OPT, _p, _p],
        "mdrp_estimate_classic_ranked_async": [_p, _i, _p, _p, _p, *_TAB, *_OPT, _p],
        "mdrp_prosac_samples_k": [_p, _u64, _i, _i, _u64, _p, _i, _p],
    },
    "mdrp_classic_models.h": {  # the baselines from a caller's model
        "mdrp_refine_classic": [_p, _i, _i, _p, _p, *_TAB, *_OPT, _p, _i, _p, _p, _p, _p],
        "mdrp_refine_classic_async": [_p, _i, _p, _p, *_TAB, *_OPT, _p, _i, _p, _p, _p],
        "mdrp_estimate_classic_prior": [_p, _i, _i, _p, _p, *_TAB, *_OPT, _p, _i, _p, _p],
        "mdrp_estimate_classic_prior_async": [_p, _i, _p, _p, *_TAB, *_OPT, _p, _i, _p],
    },
    "mdrp_classic_frontend.h": {  # the baselines' device front end (no depth maps)
        "mdrp_gather_point_matches": _gather_args(PointMatches, 3, False),
        "mdrp_gather_point_matches_ranked": _gather_args(PointMatches, 3, True),
        "mdrp_gather_point_image_pairs": _gather_args(PointImagePairs, 3, False),
        "mdrp_gather_point_image_pairs_ranked": _gather_args(PointImagePairs, 3, True),
        "mdrp_estimate_classic_matches_async": _front_args(PointMatches, False),
        "mdrp_estimate_classic_matches_ranked_async": _front_args(PointMatches, True),
        "mdrp_estimate_classic_image_pairs_async": _front_args(PointImagePairs, False),
        "mdrp_estimate_classic_image_pairs_ranked_async": _front_args(PointImagePairs, True),
    },
    "mdrp_classic_focals.h": {  # focals and pose from the 7-point estimator's F
        "mdrp_focals_from_fundamental": [_p, _i, _p, _p, _p, _i, _p],
        "mdrp_pose_from_fundamental": [_p, _i, _p, _p, _i, _i, _p, _p, _i, _p, _p, _p, _p],
        "mdrp_pose_from_fundamental_async": [_p, _p, _p, _i, _i, _p, _p, _i, _p, _p, _p, _p],
        "mdrp_estimate_fundamental_focals_async": [_p, _p, _p, _i, _i, _p, *_OPT, _p, _p, _p, _p],
    },
    "mdrp_dense.h": {  # the front end for dense matchers (a warp sampled by certainty)
        "mdrp_sample_dense": _gather_args(DenseMatches, 6, False),
        "mdrp_estimate_dense_async": _front_args(DenseMatches, False),
    },
    "mdrp_reconstruct.h": {  # the back end: fused two-view point clouds from models and depth maps
        "mdrp_reconstruct_pairs_async": [_p, _i, C.POINTER(DepthPairs), C.POINTER(ReconstructOpt), _i, _p, _i, _p, _p, _p, _p, _p],
        "mdrp_reconstruct_image_pairs_async": [_p, _i, C.POINTER(DepthImagePairs), C.POINTER(ReconstructOpt), _i, _p, _i, _p, _p, _p, _p, _p],
    },
    "mdrp_scene.h": {  # an image set: the pairs chained along a tree, one fused cloud per scene
        "mdrp_scene_transforms_async": [_p, _i, _i, _p, _i, _p, _i, _p, _p],
        "mdrp_reconstruct_scene_async": [_p, _i, C.POINTER(DepthImagePairs), C.POINTER(ReconstructOpt), _i, _p, _i, _p, _p, _p, _p, _p, _p],
    },
    "mdrp_covis.h": {  # co-visibility: dense depth-consistency counts per pair
        "mdrp_covisibility_pairs_async": [_p, _i, C.POINTER(DepthPairs), C.POINTER(CovisOpt), _i, _p, _i, _p, _p, _p],
        "mdrp_covisibility_image_pairs_async": [_p, _i, C.POINTER(DepthImagePairs), C.POINTER(CovisOpt), _i, _p, _i, _p, _p, _p],
    },
    "mdrp_fuse.h": {  # the consistency filter of a scene: only the points that other images' depth maps confirm
        "mdrp_fuse_scene_async": [_p, _i, C.POINTER(DepthImagePairs), C.POINTER(FuseOpt), _i, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p],
    },
}
# what each header declares: mdrp.h's own list (with the four symbols that only get a restype), then its extension headers'
EXPORTS = tuple(PROTOTYPES["mdrp.h"]) + ("mdrp_last_error", "mdrp_version", "mdrp_abi_version", "mdrp_hip_build_version")
EXPORTS_CLASSIC_RANKED = tuple(PROTOTYPES["mdrp_classic_ranked.h"])
EXPORTS_CLASSIC_MODELS = tuple(PROTOTYPES["mdrp_classic_models.h"])
EXPORTS_CLASSIC_FRONTEND = tuple(PROTOTYPES["mdrp_classic_frontend.h"])
EXPORTS_CLASSIC_FOCALS = tuple(PROTOTYPES["mdrp_classic_focals.h"])
EXPORTS_DENSE = tuple(PROTOTYPES["mdrp_dense.h"])
EXPORTS_RECONSTRUCT = tuple(PROTOTYPES["mdrp_reconstruct.h"])
EXPORTS_SCENE = tuple(PROTOTYPES["mdrp_scene.h"])
EXPORTS_COVIS = tuple(PROTOTYPES["mdrp_covis.h"])
EXPORTS_FUSE = tuple(PROTOTYPES["mdrp_fuse.h"])

_lib = None
_lib_lock = threading.Lock()


class MdrpError(RuntimeError):
    pass


def load_library():
    """dlopen libmdrp_hip.so and declare prototypes.  Raises MdrpError if it is not built."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise MdrpError(f"{LIB_PATH} is not built (run __graft_entry__.build()); mdrp_amd has no CPU fallback")
        _ensure_hip_runtime()  # the library binds its hip* symbols to the process's one runtime when it is loaded
        lib = C.CDLL(LIB_PATH)
        _check_hip_runtime_version(lib)
        lib.mdrp_last_error.restype = C.c_char_p
        lib.mdrp_version.restype = C.c_char_p
        abi = getattr(lib, "mdrp_abi_version", None)  # (a library from before ABI 0.4, e.g. through MDRP_LIB, has no such symbol)
        if abi is None or getattr(lib, "mdrp_create_", None) is None:
            raise MdrpError(f"{LIB_PATH} predates ABI {ABI_VERSION:#x} (no mdrp_abi_version / mdrp_create_): rebuild (mdrp_amd/build.py)")
        abi.restype = C.c_int
        if abi() != ABI_VERSION:
            raise MdrpError(f"{LIB_PATH} speaks ABI {abi():#x}, this binding {ABI_VERSION:#x}: rebuild (mdrp_amd/build.py)")
        lib.mdrp_destroy.restype = None
        for symbols in PROTOTYPES.values():
            for name, argtypes in symbols.items():
                if hasattr(lib, name):  # (an older ABI-0.6 library through MDRP_LIB lacks the later entry points: _fn raises where one is called)
                    getattr(lib, name).argtypes = argtypes
        _lib = lib
        return lib


ABI_VERSION = 0x00000006  # include/mdrp.h MDRP_ABI_VERSION
ERR_UNSUPPORTED = 4  # include/mdrp.h MDRP_ERR_UNSUPPORTED: a reference option that selects behaviour the library does not build


def _check(lib, rc):
    if rc == ERR_UNSUPPORTED:
        raise NotImplementedError(f"mdrp: {lib.mdrp_last_error().decode(errors='replace')} (DESIGN.md 9)")
    if rc != 0:
        raise MdrpError(f"mdrp error {rc}: {lib.mdrp_last_error().decode(errors='replace')}")


def _fn(lib, name):
    """the entry point `name` of the loaded library, or MdrpError where an older library (through MDRP_LIB) does not have it"""
    fn = getattr(lib, name, None)
    if fn is None:
        raise MdrpError(f"{LIB_PATH} has no {name}: rebuild (mdrp_amd/build.py)")
    return fn


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _dev(p):
    """an optional device pointer (an int; None or 0: absent) as the library takes it"""
    return C.c_void_p(p) if p else None


def _tables(n_per_pair, cam1, cam2):
    """the per-pair tables of an estimator call, each optional, as the host arrays the library reads: n_per_pair int32, cam1 / cam2 camera records"""
    return (None if n_per_pair is None else np.ascontiguousarray(n_per_pair, dtype=np.int32),
            None if cam1 is None else np.ascontiguousarray(cam1, dtype=CAMERA_DTYPE),
            None if cam2 is None else np.ascontiguousarray(cam2, dtype=CAMERA_DTYPE))


def _host_batch(x1, x2, d1=None, d2=None, depths="none"):
    """The correspondences of a host (numpy) batch as the library reads them: (x1, x2 (B, N, 2) float64, d1, d2 (B, N) float64 or None, B, N).
    depths: "required" (a monodepth estimator without them is refused here), "optional" (each may be None: the library decides) or "none" (a
    baseline: whatever was passed is dropped)."""
    x1 = np.ascontiguousarray(x1, dtype=np.float64)
    x2 = np.ascontiguousarray(x2, dtype=np.float64)
    if x1.ndim != 3 or x1.shape[2] != 2 or x2.shape != x1.shape:
        raise ValueError("expected x1,x2 (B,N,2)")
    if depths == "none":
        d1 = d2 = None
    else:
        d1 = None if d1 is None and depths == "optional" else np.ascontiguousarray(d1, dtype=np.float64)
        d2 = None if d2 is None and depths == "optional" else np.ascontiguousarray(d2, dtype=np.float64)
        if d1 is not None and d2 is not None and (d1.shape != x1.shape[:2] or d2.shape != d1.shape):
            raise ValueError("expected d1,d2 (B,N)")
    return x1, x2, d1, d2, x1.shape[0], x1.shape[1]


def _host_models(models, B, what):
    """one optional model record per pair of a host batch"""
    models = None if models is None else np.ascontiguousarray(models, dtype=MODEL_DTYPE).reshape(-1)
    if models is not None and len(models) != B:
        raise ValueError(f"expected {B} {what}, got {len(models)}")
    return models


def _host_scores(scores, B, N):
    """one optional score per correspondence of a host batch"""
    scores = None if scores is None else np.ascontiguousarray(scores, dtype=np.float64)
    if scores is not None and scores.shape != (B, N):
        raise ValueError(f"expected scores ({B},{N}), got {scores.shape}")
    return scores


def _results(B, N, want_mask, planes=()):
    """the records and the inlier masks a blocking call fills, `planes`: the leading axes (one per budget)"""
    return np.zeros((*planes, B), dtype=RESULT_DTYPE), np.zeros((*planes, B, N), dtype=np.uint8) if want_mask else None


def ransac_opt_from_dict(d=None):
    """RansacOptions from a poselib-style dict; defaults as the reference's pybind wrapper;
    unknown keys are ignored like the reference does.  progressive_sampling / max_prosac_iterations / real_focal_check travel to the
    library, which refuses what it does not build (MDRP_ERR_UNSUPPORTED -> NotImplementedError) instead of ignoring it."""
    d = d or {}
    return RansacOpt(int(d.get("max_iterations", 100000)), int(d.get("min_iterations", 1000)),
                     float(d.get("dyn_num_trials_mult", 3.0)), float(d.get("success_prob", 0.9999)),
                     float(d.get("max_reproj_error", 12.0)), float(d.get("max_epipolar_error", 1.0)),
                     int(d.get("seed", 0)), int(bool(d.get("monodepth_estimate_shift", False))),
                     float(d.get("monodepth_weight_sampson", 1.0)), int(bool(d.get("score_initial_model", False))),
                     int(bool(d.get("progressive_sampling", False))), int(d.get("max_prosac_iterations", 100000)),
                     int(bool(d.get("real_focal_check", False))), 0)


LOSS_TYPES = {"TRIVIAL": 0, "TRUNCATED": 1, "HUBER": 2, "CAUCHY": 3, "TRUNCATED_CAUCHY": 4, "TRUNCATED_LE_ZACH": 5}


def bundle_opt_from_dict(d=None):
    d = d or {}
    lt = d.get("loss_type", "CAUCHY")
    if isinstance(lt, str):
        if lt.upper() not in LOSS_TYPES:
            raise ValueError(f"unknown loss_type {lt!r}")
        lt = LOSS_TYPES[lt.upper()]
    return BundleOpt(int(d.get("max_iterations", 100)), int(lt), float(d.get("loss_scale", 1.0)),
                     float(d.get("gradient_tol", 1e-10)), float(d.get("step_tol", 1e-8)), float(d.get("initial_lambda", 1e-3)),
                     float(d.get("min_lambda", 1e-10)), float(d.get("max_lambda", 1e10)))


def budget_list(budgets, ransac_opt=None):
    """An iteration-budget list as the library takes it (mdrp_estimate_batch_budgets): integers >= 1, strictly increasing, at most MAX_BUDGETS.
    Returns (uint64 array, ransac option dict with max_iterations = the last budget).  ValueError for an invalid list, and where the dict
    already holds another max_iterations.  Needs no library."""
    try:
        ks = [int(k) for k in budgets]
        exact = all(k == b for k, b in zip(ks, budgets))
    except (TypeError, ValueError):
        raise ValueError("budgets must be a sequence of integers") from None
    if not ks:
        raise ValueError("budgets: an empty list")
    if not exact:
        raise ValueError("budgets must be integers")
    if len(ks) > MAX_BUDGETS:
        raise ValueError(f"budgets: more than {MAX_BUDGETS}")
    if ks[0] < 1 or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError("budgets must be >= 1 and strictly increasing")
    ro = dict(ransac_opt or {})
    if "max_iterations" in ro and int(ro["max_iterations"]) != ks[-1]:
        raise ValueError(f"ransac_opt['max_iterations'] = {ro['max_iterations']} differs from the last budget {ks[-1]}")
    ro["max_iterations"] = ks[-1]
    return np.asarray(ks, dtype=np.uint64), ro


def solver_residency(solver, resident_per_simd, keep_free_bytes=0, device=0):
    """(LDS bytes of a compute unit, dynamic LDS the scheduler's rule reserves per one-wavefront solver workgroup or 0, workgroups per compute unit
    the runtime's occupancy query reports for that reservation): mdrp_solver_residency — no kernel runs"""
    lib = load_library()
    lds, reserve, wgs = C.c_uint64(), C.c_uint64(), C.c_int()
    _check(lib, _fn(lib, "mdrp_solver_residency")(int(device), int(solver), int(resident_per_simd), int(keep_free_bytes), C.byref(lds), C.byref(reserve), C.byref(wgs)))
    return lds.value, reserve.value, wgs.value


def library_version():
    return load_library().mdrp_version().decode()


def library_source_hash():
    """the source hash the loaded library was built from (mdrp_version(); compare with build.source_hash())"""
    v = library_version()
    return v.split("MDRP_SRC_HASH=", 1)[1][:16] if "MDRP_SRC_HASH=" in v else None


_hip_runtime = None
hip_versions = None  # {"built": HIP_VERSION of the toolchain, "runtime": hipRuntimeGetVersion()} once the library is loaded


def _check_hip_runtime_version(lib):
    """The library binds to whatever HIP runtime the process holds (-no-hip-rt).  Compare that runtime's version
    (hipRuntimeGetVersion: major * 10^7 + minor * 10^5 + patch) with the HIP_VERSION hipcc compiled the library against
    (mdrp_hip_build_version()): a different MAJOR is refused (fat-binary registration and struct layouts may differ), a different
    minor is reported once."""
    import warnings
    try:
        lib.mdrp_hip_build_version.restype = C.c_int
        built = int(lib.mdrp_hip_build_version())
        v = C.c_int(0)
        rt = _hip_runtime.hipRuntimeGetVersion
        rt.argtypes = [C.POINTER(C.c_int)]
        if rt(C.byref(v)) != 0:
            return
    except (AttributeError, OSError):
        return
    have = int(v.value)
    if have // 10_000_000 != built // 10_000_000:
        raise MdrpError(f"libmdrp_hip.so was built against HIP {built // 10_000_000}.{built // 100_000 % 100} but the process's HIP runtime "
                        f"({getattr(_hip_runtime, '_name', '?')}) is {have // 10_000_000}.{have // 100_000 % 100}: set MDRP_HIP_RUNTIME to a "
                        "matching libamdhip64.so or rebuild (mdrp_amd/build.py)")
    global hip_versions
    hip_versions = {"built": built, "runtime": have}  # e.g. PyTorch-ROCm 2.10 wheels bundle HIP 7.0, this image's hipcc is 7.2: same major
    if have // 100_000 != built // 100_000 and os.environ.get("MDRP_DEBUG"):
        warnings.warn(f"mdrp: HIP runtime {have // 10_000_000}.{have // 100_000 % 100} in this process, library built against "
                      f"{built // 10_000_000}.{built // 100_000 % 100} (same major: continuing)", RuntimeWarning, stacklevel=3)


def _ensure_hip_runtime():
    """libmdrp_hip.so is linked WITHOUT a HIP runtime of its own (build.py: -no-hip-rt): its hip* symbols bind to whatever runtime
    the process has, so that there is exactly one — streams, events and device pointers of the host framework are then valid
    inside the library by construction.  PyTorch-ROCm wheels bundle a runtime (torch/lib/libamdhip64.so, no SONAME): if torch is
    imported or merely installed, THAT file is (re)opened with RTLD_GLOBAL (dlopen of an already loaded library only widens its
    scope); otherwise the system runtime is.  MDRP_HIP_RUNTIME=/path/to/libamdhip64.so overrides the choice."""
    global _hip_runtime
    if _hip_runtime is not None:
        return _hip_runtime
    import sys
    cands = []
    if os.environ.get("MDRP_HIP_RUNTIME"):
        cands.append(os.environ["MDRP_HIP_RUNTIME"])
    try:
        torch = sys.modules.get("torch")
        if torch is not None:
            tdir = os.path.dirname(torch.__file__)
        else:
            import importlib.util
            spec = importlib.util.find_spec("torch")
            tdir = list(spec.submodule_search_locations)[0] if spec is not None and spec.submodule_search_locations else None
        if tdir and os.path.exists(os.path.join(tdir, "lib", "libamdhip64.so")):
            cands.append(os.path.join(tdir, "lib", "libamdhip64.so"))
    except Exception:
        pass
    import glob
    # the SONAME major follows the ROCm release: whatever /opt/rocm (or ROCM_PATH) ships, newest first, then the linker's search
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    def _soname_version(path):
        tail = os.path.basename(path).split(".so.", 1)[-1]
        return tuple(int(x) for x in tail.split(".") if x.isdigit())
    cands += sorted(glob.glob(os.path.join(rocm, "lib", "libamdhip64.so.*")), key=_soname_version, reverse=True) + ["libamdhip64.so", os.path.join(rocm, "lib", "libamdhip64.so")]
    errs = []
    for c in cands:
        try:
            _hip_runtime = C.CDLL(c, mode=C.RTLD_GLOBAL)
            return _hip_runtime
        except OSError as e:
            errs.append(f"{c}: {e}")
    raise MdrpError("no HIP runtime (libamdhip64) could be loaded: " + "; ".join(errs))


class _ReconstructCalls:
    """The back end's two calls (include/mdrp_reconstruct.h), methods of Handle through this base: a DepthPairs / DepthImagePairs descriptor and a
    ReconstructOpt of device pointers and plain values.  Arguments go to the library as they are: the library checks them."""

    def reconstruct_pairs_device(self, kind, desc, opt, batch, models_ptr, model_stride, points_ptr, pixel_ptr, counts_ptr, cam1=None, cam2=None):
        """fused two-view point clouds on the handle's stream into the caller's device buffers: points [batch][p_max][3] float32, pixel
        [batch][p_max] int32, counts [batch][2] int32.  models_ptr: device records model_stride bytes apart (96: models, 136: what
        copy_results_device wrote); cam1 / cam2: per PAIR, the calibrated kind alone.  Nothing synchronises."""
        stem = "image_pairs" if isinstance(desc, DepthImagePairs) else "pairs"
        _, c1, c2 = _tables(None, cam1, cam2)
        _check(self._lib, _fn(self._lib, f"mdrp_reconstruct_{stem}_async")(self._h, int(kind), C.byref(desc), C.byref(opt), int(batch), _dev(models_ptr),
                                                                          int(model_stride), _ptr(c1), _ptr(c2), _dev(points_ptr), _dev(pixel_ptr),
                                                                          _dev(counts_ptr)))

    def reconstruct_image_pairs_device(self, kind, desc, opt, batch, models_ptr, model_stride, points_ptr, pixel_ptr, counts_ptr, cam1=None, cam2=None):
        """reconstruct_pairs_device for a DepthImagePairs descriptor"""
        if not isinstance(desc, DepthImagePairs):
            raise ValueError("reconstruct_image_pairs_device takes a DepthImagePairs descriptor")
        self.reconstruct_pairs_device(kind, desc, opt, batch, models_ptr, model_stride, points_ptr, pixel_ptr, counts_ptr, cam1, cam2)


class _SceneCalls:
    """The two calls of include/mdrp_scene.h, methods of Handle through this base.  Arguments go to the library as they are: the library checks them."""

    def scene_transforms_device(self, kind, batch, models_ptr, model_stride, pairs_ptr, n_images, tree_ptr, transforms_ptr):
        """the accumulated transform of every image of a tree on the handle's stream into the caller's device buffer, [n_images] SceneTransform
        records.  pairs_ptr: int32 [batch][2], tree_ptr: int32 [n_images][2] (pair, role), both on the device.  Nothing synchronises."""
        _check(self._lib, _fn(self._lib, "mdrp_scene_transforms_async")(self._h, int(kind), int(batch), _dev(models_ptr), int(model_stride), _dev(pairs_ptr),
                                                                        int(n_images), _dev(tree_ptr), _dev(transforms_ptr)))

    def reconstruct_scene_device(self, kind, desc, opt, batch, models_ptr, model_stride, tree_ptr, points_ptr, pixel_ptr, offsets_ptr, cams=None,
                                 transforms_ptr=None):
        """the fused cloud of an image set on the handle's stream into the caller's device buffers: points [p_max][3] float32, pixel [p_max] int32,
        offsets [n_images + 1] int64, and the [n_images] transform records where transforms_ptr is given.  desc: a DepthImagePairs; cams: per
        IMAGE, the calibrated kind alone.  Nothing synchronises."""
        if not isinstance(desc, DepthImagePairs):
            raise ValueError("reconstruct_scene_device takes a DepthImagePairs descriptor")
        _, c, _ = _tables(None, cams, None)
        _check(self._lib, _fn(self._lib, "mdrp_reconstruct_scene_async")(self._h, int(kind), C.byref(desc), C.byref(opt), int(batch), _dev(models_ptr),
                                                                         int(model_stride), _dev(tree_ptr), _ptr(c), _dev(transforms_ptr),
                                                                         _dev(points_ptr), _dev(pixel_ptr), _dev(offsets_ptr)))


class _CovisCalls:
    """The two calls of include/mdrp_covis.h, methods of Handle through this base.  Arguments go to the library as they are: the library checks them."""

    def covisibility_pairs_device(self, kind, desc, opt, batch, models_ptr, model_stride, counts_ptr, cam1=None, cam2=None):
        """the depth-consistency counts of a batch of pairs on the handle's stream into the caller's device buffer, counts [batch][2][8] int32.
        desc: a DepthPairs or a DepthImagePairs; opt: a CovisOpt; models_ptr, cam1 / cam2 as reconstruct_pairs_device.  Nothing synchronises."""
        stem = "image_pairs" if isinstance(desc, DepthImagePairs) else "pairs"
        _, c1, c2 = _tables(None, cam1, cam2)
        _check(self._lib, _fn(self._lib, f"mdrp_covisibility_{stem}_async")(self._h, int(kind), C.byref(desc), C.byref(opt), int(batch), _dev(models_ptr),
                                                                           int(model_stride), _ptr(c1), _ptr(c2), _dev(counts_ptr)))

    def covisibility_image_pairs_device(self, kind, desc, opt, batch, models_ptr, model_stride, counts_ptr, cam1=None, cam2=None):
        """covisibility_pairs_device for a DepthImagePairs descriptor"""
        if not isinstance(desc, DepthImagePairs):
            raise ValueError("covisibility_image_pairs_device takes a DepthImagePairs descriptor")
        self.covisibility_pairs_device(kind, desc, opt, batch, models_ptr, model_stride, counts_ptr, cam1, cam2)


class _FuseCalls:
    """The call of include/mdrp_fuse.h, a method of Handle through this base.  Arguments go to the library as they are: the library checks them."""

    def fuse_scene_device(self, kind, desc, opt, batch, models_ptr, model_stride, tree_ptr, views_ptr, points_ptr, pixel_ptr, support_ptr, offsets_ptr,
                          cams=None, transforms_ptr=None):
        """the consistency-filtered cloud of an image set on the handle's stream into the caller's device buffers: points [p_max][3] float32, pixel
        [p_max] int32, support [p_max][2] uint8, offsets [n_images + 1] int64, and the [n_images] transform records where transforms_ptr is given.
        desc: a DepthImagePairs; opt: a FuseOpt; views_ptr: int32 [n_images][opt.n_views] on the device; cams: per IMAGE, the calibrated kind
        alone.  Nothing synchronises."""
        if not isinstance(desc, DepthImagePairs):
            raise ValueError("fuse_scene_device takes a DepthImagePairs descriptor")
        _, c, _ = _tables(None, cams, None)
        _check(self._lib, _fn(self._lib, "mdrp_fuse_scene_async")(self._h, int(kind), C.byref(desc), C.byref(opt), int(batch), _dev(models_ptr),
                                                                  int(model_stride), _dev(tree_ptr), _dev(views_ptr), _ptr(c), _dev(transforms_ptr),
                                                                  _dev(points_ptr), _dev(pixel_ptr), _dev(support_ptr), _dev(offsets_ptr)))


class Handle(_ReconstructCalls, _SceneCalls, _CovisCalls, _FuseCalls):
    """One handle = one HIP device + one stream + its scratch buffers.  Calls on one handle are serialised inside the
    library; use one handle per host thread for concurrency (default_handle() does).

    stream=None: the handle creates its own stream.  stream=<int>: a hipStream_t of the caller, used as given —
    0 is the device's legacy default stream (torch.cuda.current_stream().cuda_stream is 0 on torch's default stream)."""

    def __init__(self, device=0, stream=None):
        self._lib = load_library()
        h = C.c_void_p()
        if stream is None:
            _check(self._lib, self._lib.mdrp_create_(int(device), None, C.byref(h), ABI_VERSION, C.sizeof(RansacOpt)))
        else:
            _check(self._lib, self._lib.mdrp_create_on_stream_(int(device), _dev(int(stream)), C.byref(h), ABI_VERSION, C.sizeof(RansacOpt)))
        self._h = h
        self.device = int(device)
        self.stream = stream

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mdrp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(self._lib, self._lib.mdrp_synchronize(self._h))

    # ---- batched estimators, host (numpy) buffers
    def estimate_batch(self, kind, x1, x2, d1, d2, ropt, bopt, n_per_pair=None, cam1=None, cam2=None, want_mask=True):
        x1, x2, d1, d2, B, N = _host_batch(x1, x2, d1, d2, "none" if kind >= RELPOSE_5PT else "required")  # the non-monodepth baselines take no depths
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        out, mask = _results(B, N, want_mask)
        _check(self._lib, self._lib.mdrp_estimate_batch(self._h, kind, MEM_HOST, _ptr(x1), _ptr(x2), _ptr(d1), _ptr(d2), B, N,
                                                        _ptr(npp), _ptr(c1), _ptr(c2), C.byref(ropt), C.byref(bopt),
                                                        _ptr(out), _ptr(mask)))
        return out, mask

    # ---- batched estimators, device pointers (ints), results fetched separately
    def estimate_batch_device(self, kind, x1_ptr, x2_ptr, d1_ptr, d2_ptr, batch, n_max, ropt, bopt, n_per_pair=None,
                              cam1=None, cam2=None, mask_ptr=None):
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        _check(self._lib, self._lib.mdrp_estimate_batch_async(self._h, kind, _dev(x1_ptr), _dev(x2_ptr), _dev(d1_ptr), _dev(d2_ptr), int(batch), int(n_max),
                                                              _ptr(npp), _ptr(c1), _ptr(c2), C.byref(ropt), C.byref(bopt), _dev(mask_ptr)))

    # ---- every budget of a list in one run (include/mdrp.h: iteration budgets).  The list goes to the library as it is: the library checks it.
    def estimate_batch_budgets(self, kind, x1, x2, d1, d2, ropt, bopt, budgets, n_per_pair=None, cam1=None, cam2=None, want_mask=True):
        """estimate_batch at every budget: records (C, B) and masks (C, B, N), C = len(budgets)"""
        x1, x2, d1, d2, B, N = _host_batch(x1, x2, d1, d2, "none" if kind >= RELPOSE_5PT else "required")
        ks = np.ascontiguousarray(budgets, dtype=np.uint64).reshape(-1)
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        out, mask = _results(B, N, want_mask, (len(ks),))
        _check(self._lib, _fn(self._lib, "mdrp_estimate_batch_budgets")(self._h, kind, MEM_HOST, _ptr(x1), _ptr(x2), _ptr(d1), _ptr(d2), B, N,
                                                                        _ptr(npp), _ptr(c1), _ptr(c2), C.byref(ropt), C.byref(bopt),
                                                                        _ptr(ks), len(ks), _ptr(out), _ptr(mask)))
        return out, mask

    def estimate_batch_budgets_device(self, kind, x1_ptr, x2_ptr, d1_ptr, d2_ptr, batch, n_max, ropt, bopt, budgets, n_per_pair=None,
                                      cam1=None, cam2=None, mask_ptr=None):
        """estimate_batch_device at every budget; mask_ptr: (C, batch, n_max) bytes on the device.  Records: fetch_budget_results."""
        ks = np.ascontiguousarray(budgets, dtype=np.uint64).reshape(-1)
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        _check(self._lib, _fn(self._lib, "mdrp_estimate_batch_budgets_async")(self._h, kind, _dev(x1_ptr), _dev(x2_ptr), _dev(d1_ptr), _dev(d2_ptr),
                                                                              int(batch), int(n_max), _ptr(npp), _ptr(c1), _ptr(c2), C.byref(ropt),
                                                                              C.byref(bopt), _ptr(ks), len(ks), _dev(mask_ptr)))

    def fetch_budget_results(self, n_budgets, batch):
        out = np.zeros((int(n_budgets), int(batch)), dtype=RESULT_DTYPE)
        _check(self._lib, _fn(self._lib, "mdrp_fetch_budget_results")(self._h, _ptr(out), int(n_budgets), int(batch)))
        return out

    def copy_budget_results_device(self, dst_ptr, n_budgets, batch):
        """the records of the last budgets call into device memory at dst_ptr (n_budgets x batch x 136 bytes)"""
        _check(self._lib, _fn(self._lib, "mdrp_copy_budget_results_device")(self._h, _dev(dst_ptr), int(n_budgets), int(batch)))

    # ---- refine and verify caller-supplied models (include/mdrp.h: mdrp_refine_batch).  Arguments go to the library as they are: the library checks them.
    def refine_batch(self, kind, x1, x2, d1, d2, models, ropt, bopt, stages=STAGE_LO | STAGE_INLIERS, n_per_pair=None, cam1=None, cam2=None, want_mask=True):
        """B models (MODEL_DTYPE) against B pairs, host (numpy) buffers: (records, masks (B, N) uint8 or None, initial score (B,) float64,
        initial inlier count (B,) int32)"""
        x1, x2, d1, d2, B, N = _host_batch(x1, x2, d1, d2, "required")
        models = _host_models(models, B, "models")
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        out, mask = _results(B, N, want_mask)
        score0, inl0 = np.zeros(B), np.zeros(B, dtype=np.int32)
        _check(self._lib, _fn(self._lib, "mdrp_refine_batch")(self._h, int(kind), MEM_HOST, _ptr(x1), _ptr(x2), _ptr(d1), _ptr(d2), B, N, _ptr(npp), _ptr(c1),
                                                              _ptr(c2), C.byref(ropt), C.byref(bopt), _ptr(models), int(stages), _ptr(out), _ptr(mask),
                                                              _ptr(score0), _ptr(inl0)))
        return out, mask, score0, inl0

    def refine_batch_device(self, kind, x1_ptr, x2_ptr, d1_ptr, d2_ptr, batch, n_max, models_ptr, ropt, bopt, stages=STAGE_LO | STAGE_INLIERS, n_per_pair=None,
                            cam1=None, cam2=None, mask_ptr=None, initial_score_ptr=None, initial_inliers_ptr=None):
        """the same on device pointers (ints), queued on the handle's stream; models_ptr: batch x 96 bytes; initial_score_ptr / initial_inliers_ptr:
        batch float64 / int32 on the device, or None.  Records: fetch_results / copy_results_device."""
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        _check(self._lib, _fn(self._lib, "mdrp_refine_batch_async")(self._h, int(kind), _dev(x1_ptr), _dev(x2_ptr), _dev(d1_ptr), _dev(d2_ptr), int(batch),
                                                                    int(n_max), _ptr(npp), _ptr(c1), _ptr(c2), C.byref(ropt), C.byref(bopt), _dev(models_ptr),
                                                                    int(stages), _dev(mask_ptr), _dev(initial_score_ptr), _dev(initial_inliers_ptr)))

    # ---- estimate with a prior (include/mdrp.h: mdrp_estimate_batch_prior).  Arguments go to the library as they are: the library checks them.
    def estimate_batch_prior(self, kind, x1, x2, d1, d2, priors, ropt, bopt, n_per_pair=None, cam1=None, cam2=None, want_mask=True):
        """estimate_batch with one prior (MODEL_DTYPE; a NaN q[0]: none) per pair, host (numpy) buffers: (records, masks (B, N) uint8 or None)"""
        x1, x2, d1, d2, B, N = _host_batch(x1, x2, d1, d2, "optional")
        priors = _host_models(priors, B, "priors")
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        out, mask = _results(B, N, want_mask)
        _check(self._lib, _fn(self._lib, "mdrp_estimate_batch_prior")(self._h, int(kind), MEM_HOST, _ptr(x1), _ptr(x2), _ptr(d1), _ptr(d2), B, N, _ptr(npp),
                                                                      _ptr(c1), _ptr(c2), C.byref(ropt), C.byref(bopt), _ptr(priors), _ptr(out), _ptr(mask)))
        return out, mask

    def estimate_batch_prior_device(self, kind, x1_ptr, x2_ptr, d1_ptr, d2_ptr, batch, n_max, priors_ptr, ropt, bopt, n_per_pair=None, cam1=None, cam2=None,
                                    mask_ptr=None):
        """the same on device pointers (ints), queued on the handle's stream; priors_ptr: batch x 96 bytes.  Records: fetch_results / copy_results_device."""
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        _check(self._lib, _fn(self._lib, "mdrp_estimate_batch_prior_async")(self._h, int(kind), _dev(x1_ptr), _dev(x2_ptr), _dev(d1_ptr), _dev(d2_ptr),
                                                                            int(batch), int(n_max), _ptr(npp), _ptr(c1), _ptr(c2), C.byref(ropt),
                                                                            C.byref(bopt), _dev(priors_ptr), _dev(mask_ptr)))

    # ---- estimate in match-score order (include/mdrp.h: mdrp_estimate_batch_ranked).  Arguments go to the library as they are: the library checks them.
    def estimate_batch_ranked(self, kind, x1, x2, d1, d2, scores, ropt, bopt, n_per_pair=None, cam1=None, cam2=None, want_mask=True):
        """estimate_batch in score order with the progressive sampler, host (numpy) buffers; scores (B, N), higher is better, or None: the records
        are in quality order already.  (records, masks (B, N) uint8 in the caller's order or None)"""
        x1, x2, d1, d2, B, N = _host_batch(x1, x2, d1, d2, "optional")
        scores = _host_scores(scores, B, N)
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        out, mask = _results(B, N, want_mask)
        _check(self._lib, _fn(self._lib, "mdrp_estimate_batch_ranked")(self._h, int(kind), MEM_HOST, _ptr(x1), _ptr(x2), _ptr(d1), _ptr(d2), _ptr(scores), B, N,
                                                                       _ptr(npp), _ptr(c1), _ptr(c2), C.byref(ropt), C.byref(bopt), _ptr(out), _ptr(mask)))
        return out, mask

    def estimate_batch_ranked_device(self, kind, x1_ptr, x2_ptr, d1_ptr, d2_ptr, scores_ptr, batch, n_max, ropt, bopt, n_per_pair=None, cam1=None, cam2=None,
                                     mask_ptr=None):
        """the same on device pointers (ints), queued on the handle's stream; scores_ptr: batch x n_max float64, or None / 0 for records in quality
        order.  Records: fetch_results / copy_results_device."""
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        _check(self._lib, _fn(self._lib, "mdrp_estimate_batch_ranked_async")(self._h, int(kind), _dev(x1_ptr), _dev(x2_ptr), _dev(d1_ptr), _dev(d2_ptr),
                                                                             _dev(scores_ptr), int(batch), int(n_max), _ptr(npp), _ptr(c1), _ptr(c2),
                                                                             C.byref(ropt), C.byref(bopt), _dev(mask_ptr)))

    def prosac_samples(self, seed, n, max_prosac_iterations, chunk_lens, fill=0):
        """the device's progressive sampler for one table of n records, drawn chunk by chunk: (sum(chunk_lens), 3) uint32 (`fill` where n < 3:
        nothing is written)"""
        lens = np.ascontiguousarray(chunk_lens, dtype=np.int32).reshape(-1)
        out = np.full((int(lens.sum()), 3), fill, dtype=np.uint32)
        _check(self._lib, _fn(self._lib, "mdrp_prosac_samples")(self._h, int(seed), int(n), int(max_prosac_iterations), _ptr(lens), len(lens), _ptr(out)))
        return out

    # ---- the 5- / 6- / 7-point baselines in match-score order (include/mdrp.h: mdrp_estimate_classic_ranked): no depths
    def estimate_classic_ranked(self, kind, x1, x2, scores, ropt, bopt, n_per_pair=None, cam1=None, cam2=None, want_mask=True):
        """estimate_batch of a baseline (kind 3, 4, 5) in score order with the progressive sampler, host (numpy) buffers; scores (B, N), higher is
        better, or None: the records are in quality order already.  (records, masks (B, N) uint8 in the caller's order or None)"""
        x1, x2, _, _, B, N = _host_batch(x1, x2)
        scores = _host_scores(scores, B, N)
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        out, mask = _results(B, N, want_mask)
        _check(self._lib, _fn(self._lib, "mdrp_estimate_classic_ranked")(self._h, int(kind), MEM_HOST, _ptr(x1), _ptr(x2), _ptr(scores), B, N, _ptr(npp),
                                                                         _ptr(c1), _ptr(c2), C.byref(ropt), C.byref(bopt), _ptr(out), _ptr(mask)))
        return out, mask

    def estimate_classic_ranked_device(self, kind, x1_ptr, x2_ptr, scores_ptr, batch, n_max, ropt, bopt, n_per_pair=None, cam1=None, cam2=None, mask_ptr=None):
        """the same on device pointers (ints), queued on the handle's stream; scores_ptr: batch x n_max float64, or None / 0 for records in quality
        order.  Records: fetch_results / copy_results_device."""
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        _check(self._lib, _fn(self._lib, "mdrp_estimate_classic_ranked_async")(self._h, int(kind), _dev(x1_ptr), _dev(x2_ptr), _dev(scores_ptr), int(batch),
                                                                               int(n_max), _ptr(npp), _ptr(c1), _ptr(c2), C.byref(ropt), C.byref(bopt),
                                                                               _dev(mask_ptr)))

    def prosac_samples_k(self, seed, n, sample_size, max_prosac_iterations, chunk_lens, fill=0):
        """prosac_samples for samples of sample_size records (3, 5, 6 or 7): (sum(chunk_lens), sample_size) uint32"""
        lens = np.ascontiguousarray(chunk_lens, dtype=np.int32).reshape(-1)
        out = np.full((int(lens.sum()), int(sample_size)), fill, dtype=np.uint32)
        _check(self._lib, _fn(self._lib, "mdrp_prosac_samples_k")(self._h, int(seed), int(n), int(sample_size), int(max_prosac_iterations), _ptr(lens),
                                                                  len(lens), _ptr(out)))
        return out

    # ---- the 5- / 6- / 7-point baselines from a caller's model (include/mdrp_classic_models.h).  Arguments go to the library as they are: the library checks them.
    def refine_classic(self, kind, x1, x2, models, ropt, bopt, stages=STAGE_LO | STAGE_INLIERS, n_per_pair=None, cam1=None, cam2=None, want_mask=True):
        """refine_batch for a baseline (kind 3, 4, 5): B models (MODEL_DTYPE, in the caller's units; a fundamental matrix in the first nine doubles)
        against B pairs, host (numpy) buffers: (records, masks (B, N) uint8 or None, initial score (B,) float64, initial inlier count (B,) int32)"""
        x1, x2, _, _, B, N = _host_batch(x1, x2)
        models = _host_models(models, B, "models")
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        out, mask = _results(B, N, want_mask)
        score0, inl0 = np.zeros(B), np.zeros(B, dtype=np.int32)
        _check(self._lib, _fn(self._lib, "mdrp_refine_classic")(self._h, int(kind), MEM_HOST, _ptr(x1), _ptr(x2), B, N, _ptr(npp), _ptr(c1), _ptr(c2),
                                                                C.byref(ropt), C.byref(bopt), _ptr(models), int(stages), _ptr(out), _ptr(mask),
                                                                _ptr(score0), _ptr(inl0)))
        return out, mask, score0, inl0

    def refine_classic_device(self, kind, x1_ptr, x2_ptr, batch, n_max, models_ptr, ropt, bopt, stages=STAGE_LO | STAGE_INLIERS, n_per_pair=None, cam1=None,
                              cam2=None, mask_ptr=None, initial_score_ptr=None, initial_inliers_ptr=None):
        """the same on device pointers (ints), queued on the handle's stream; models_ptr: batch x 96 bytes; initial_score_ptr / initial_inliers_ptr:
        batch float64 / int32 on the device, or None.  Records: fetch_results / copy_results_device."""
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        _check(self._lib, _fn(self._lib, "mdrp_refine_classic_async")(self._h, int(kind), _dev(x1_ptr), _dev(x2_ptr), int(batch), int(n_max), _ptr(npp), _ptr(c1),
                                                                      _ptr(c2), C.byref(ropt), C.byref(bopt), _dev(models_ptr), int(stages), _dev(mask_ptr),
                                                                      _dev(initial_score_ptr), _dev(initial_inliers_ptr)))

    def estimate_classic_prior(self, kind, x1, x2, priors, ropt, bopt, n_per_pair=None, cam1=None, cam2=None, want_mask=True, prior_space=0):
        """estimate_batch of a baseline (kind 3, 4, 5) with one prior (MODEL_DTYPE; a NaN first double: none) per pair, host (numpy) buffers;
        prior_space 0: the caller's units, 1: the estimator's normalised coordinates.  (records, masks (B, N) uint8 or None)"""
        x1, x2, _, _, B, N = _host_batch(x1, x2)
        priors = _host_models(priors, B, "priors")
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        out, mask = _results(B, N, want_mask)
        _check(self._lib, _fn(self._lib, "mdrp_estimate_classic_prior")(self._h, int(kind), MEM_HOST, _ptr(x1), _ptr(x2), B, N, _ptr(npp), _ptr(c1), _ptr(c2),
                                                                        C.byref(ropt), C.byref(bopt), _ptr(priors), int(prior_space), _ptr(out), _ptr(mask)))
        return out, mask

    def estimate_classic_prior_device(self, kind, x1_ptr, x2_ptr, batch, n_max, priors_ptr, ropt, bopt, n_per_pair=None, cam1=None, cam2=None, mask_ptr=None,
                                      prior_space=0):
        """the same on device pointers (ints), queued on the handle's stream; priors_ptr: batch x 96 bytes.  Records: fetch_results / copy_results_device."""
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        _check(self._lib, _fn(self._lib, "mdrp_estimate_classic_prior_async")(self._h, int(kind), _dev(x1_ptr), _dev(x2_ptr), int(batch), int(n_max), _ptr(npp),
                                                                              _ptr(c1), _ptr(c2), C.byref(ropt), C.byref(bopt), _dev(priors_ptr),
                                                                              int(prior_space), _dev(mask_ptr)))

    def rank_scores(self, scores, n_per_pair=None):
        """k_rank on host scores (B, N): order (B, N) int32, -1 at and past n"""
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        B, N = scores.shape
        npp = _tables(n_per_pair, None, None)[0]
        order = np.full((B, N), -2, dtype=np.int32)
        _check(self._lib, _fn(self._lib, "mdrp_rank_scores")(self._h, MEM_HOST, _ptr(scores), B, N, _ptr(npp), _ptr(order)))
        return order

    def rank_scores_device(self, scores_ptr, batch, n_max, order_ptr, n_per_pair=None):
        """k_rank on device pointers (ints): scores batch x n_max float64, order batch x n_max int32.  Synchronous."""
        npp = _tables(n_per_pair, None, None)[0]
        _check(self._lib, _fn(self._lib, "mdrp_rank_scores")(self._h, MEM_DEVICE, _dev(scores_ptr), int(batch), int(n_max), _ptr(npp), _dev(order_ptr)))

    # ---- the device front ends: a descriptor of device pointers (Matches, ImagePairs; PointMatches, PointImagePairs without depth maps).  scores_ptr
    # is a device pointer to batch x m_max scores of score_type (F32 | F64), or None / 0 for match rows that are in quality order already; a ranked call
    # is the entry point `stem`_ranked.  Arguments go to the library as they are: the library checks them.
    def _gather(self, stem, desc, batch, out_ptrs, scores_ptr=None, score_type=F64, ranked=False):
        """a front end's gather alone into the caller's device buffers `out_ptrs`: the kept rows per pair"""
        n = np.zeros(int(batch), dtype=np.int32)
        scored = (_dev(scores_ptr), int(score_type)) if ranked else ()
        _check(self._lib, _fn(self._lib, stem + "_ranked" if ranked else stem)(self._h, C.byref(desc), *scored, int(batch), *map(_dev, out_ptrs), _ptr(n)))
        return n

    def _estimate_front(self, stem, kind, desc, batch, ropt, bopt, cam1, cam2, mask_ptr, scores_ptr=None, score_type=F64, ranked=False):
        """a front end + estimator on the handle's stream: the kept rows per pair"""
        _, c1, c2 = _tables(None, cam1, cam2)
        n = np.zeros(int(batch), dtype=np.int32)
        scored = (_dev(scores_ptr), int(score_type)) if ranked else ()
        _check(self._lib, _fn(self._lib, stem + ("_ranked_async" if ranked else "_async"))(self._h, int(kind), C.byref(desc), *scored, int(batch), _ptr(c1), _ptr(c2),
                                                                                            C.byref(ropt), C.byref(bopt), _dev(mask_ptr), _ptr(n)))
        return n

    def gather_matches(self, mm, batch, x1_ptr, x2_ptr, d1_ptr, d2_ptr, slot_ptr):
        """k_gather alone into the caller's device buffers; returns the kept rows per pair (numpy int32).  Synchronises the stream once."""
        return self._gather("mdrp_gather_matches", mm, batch, (x1_ptr, x2_ptr, d1_ptr, d2_ptr, slot_ptr))

    def estimate_matches_device(self, kind, mm, batch, ropt, bopt, cam1=None, cam2=None, match_mask_ptr=None):
        """front end + estimator on the handle's stream; results stay on the device (fetch_results / copy_results_device).  Returns the kept rows
        per pair (numpy int32)."""
        return self._estimate_front("mdrp_estimate_matches", kind, mm, batch, ropt, bopt, cam1, cam2, match_mask_ptr)

    def gather_image_pairs(self, ip, batch, x1_ptr, x2_ptr, d1_ptr, d2_ptr, slot_ptr):
        """k_gather_images alone into the caller's device buffers; returns the kept rows per pair (numpy int32).  Synchronises the stream once."""
        return self._gather("mdrp_gather_image_pairs", ip, batch, (x1_ptr, x2_ptr, d1_ptr, d2_ptr, slot_ptr))

    def estimate_image_pairs_device(self, kind, ip, batch, ropt, bopt, cam1=None, cam2=None, match_mask_ptr=None):
        """front end on per-image tables + estimator on the handle's stream; cam1 / cam2 are per PAIR; results stay on the device (fetch_results /
        copy_results_device).  Returns the kept rows per pair (numpy int32)."""
        return self._estimate_front("mdrp_estimate_image_pairs", kind, ip, batch, ropt, bopt, cam1, cam2, match_mask_ptr)

    def gather_matches_ranked(self, mm, scores_ptr, score_type, batch, x1_ptr, x2_ptr, d1_ptr, d2_ptr, slot_ptr):
        """k_gather_ranked alone into the caller's device buffers: the kept rows at their ranks; returns the kept rows per pair (numpy int32).
        Synchronises the stream once."""
        return self._gather("mdrp_gather_matches", mm, batch, (x1_ptr, x2_ptr, d1_ptr, d2_ptr, slot_ptr), scores_ptr, score_type, True)

    def estimate_matches_ranked_device(self, kind, mm, scores_ptr, score_type, batch, ropt, bopt, cam1=None, cam2=None, match_mask_ptr=None):
        """ranked front end + estimator with the progressive sampler on the handle's stream; results stay on the device (fetch_results /
        copy_results_device).  Returns the kept rows per pair (numpy int32)."""
        return self._estimate_front("mdrp_estimate_matches", kind, mm, batch, ropt, bopt, cam1, cam2, match_mask_ptr, scores_ptr, score_type, True)

    def gather_image_pairs_ranked(self, ip, scores_ptr, score_type, batch, x1_ptr, x2_ptr, d1_ptr, d2_ptr, slot_ptr):
        """gather_matches_ranked on per-image tables (k_gather_images_ranked)"""
        return self._gather("mdrp_gather_image_pairs", ip, batch, (x1_ptr, x2_ptr, d1_ptr, d2_ptr, slot_ptr), scores_ptr, score_type, True)

    def estimate_image_pairs_ranked_device(self, kind, ip, scores_ptr, score_type, batch, ropt, bopt, cam1=None, cam2=None, match_mask_ptr=None):
        """estimate_matches_ranked_device on per-image tables; cam1 / cam2 are per PAIR"""
        return self._estimate_front("mdrp_estimate_image_pairs", kind, ip, batch, ropt, bopt, cam1, cam2, match_mask_ptr, scores_ptr, score_type, True)

    # ---- the baselines' front end (include/mdrp_classic_frontend.h): a PointMatches / PointImagePairs descriptor, no depths; ranked=False is the
    # unranked entry point
    def gather_points(self, desc, batch, x1_ptr, x2_ptr, slot_ptr, scores_ptr=None, score_type=F64, ranked=False):
        """k_gather_points* alone into the caller's device buffers (no depths); returns the kept rows per pair (numpy int32).  Synchronises the
        stream once."""
        stem = "image_pairs" if isinstance(desc, PointImagePairs) else "matches"
        return self._gather(f"mdrp_gather_point_{stem}", desc, batch, (x1_ptr, x2_ptr, slot_ptr), scores_ptr, score_type, ranked)

    def estimate_points_device(self, kind, desc, batch, ropt, bopt, cam1=None, cam2=None, match_mask_ptr=None, scores_ptr=None, score_type=F64, ranked=False):
        """front end without depths + a baseline (kind 3, 4, 5) on the handle's stream; cam1 / cam2 are per PAIR; results stay on the device
        (fetch_results / copy_results_device).  Returns the kept rows per pair (numpy int32)."""
        stem = "image_pairs" if isinstance(desc, PointImagePairs) else "matches"
        return self._estimate_front(f"mdrp_estimate_classic_{stem}", kind, desc, batch, ropt, bopt, cam1, cam2, match_mask_ptr, scores_ptr, score_type, ranked)

    def fetch_results(self, batch):
        out = np.zeros(batch, dtype=RESULT_DTYPE)
        _check(self._lib, self._lib.mdrp_fetch_results(self._h, _ptr(out), int(batch)))
        return out

    def copy_results_device(self, dst_ptr, batch):
        """the result records of the last device-resident estimate into device memory at dst_ptr (batch x 136 bytes)"""
        _check(self._lib, self._lib.mdrp_copy_results_device(self._h, _dev(dst_ptr), int(batch)))

    def last_sweep_stats(self):
        ms, launches, evals = C.c_double(0), C.c_int64(0), C.c_int64(0)
        _check(self._lib, self._lib.mdrp_last_sweep_stats(self._h, C.byref(ms), C.byref(launches), C.byref(evals)))
        return ms.value, launches.value, evals.value

    def last_stats(self):
        """dict: time and launches of k_count (MFMA) and k_score (fp64), and the evaluation counters of the last estimate call"""
        st = Stats()
        _check(self._lib, self._lib.mdrp_last_stats_sized(self._h, C.byref(st), C.sizeof(Stats)))
        d = {k: getattr(st, k) for k, _ in Stats._fields_}
        d["fuse_timeouts"] = d["fuse_gate_timeouts"] + d["fuse_wait_timeouts"]
        return d

    # ---- unit-parity entry points
    def solver_batch(self, solver, x1h, x2h, d1, d2):
        x1h = np.ascontiguousarray(x1h, dtype=np.float64).reshape(-1, 3, 3)
        x2h = np.ascontiguousarray(x2h, dtype=np.float64).reshape(-1, 3, 3)
        d1 = np.ascontiguousarray(d1, dtype=np.float64).reshape(-1, 3)
        d2 = np.ascontiguousarray(d2, dtype=np.float64).reshape(-1, 3)
        count = len(d1)
        out = np.zeros((count, 4), dtype=MODEL_DTYPE)
        n_out = np.zeros(count, dtype=np.int32)
        _check(self._lib, self._lib.mdrp_solver_batch(self._h, int(solver), _ptr(x1h), _ptr(x2h), _ptr(d1), _ptr(d2), count,
                                                      _ptr(out), _ptr(n_out)))
        return out, n_out

    def classic_solver_batch(self, kind, x1h, x2h):
        """relpose_5pt (kind 3: x1h, x2h (count, 5, 3) unit bearings -> up to 10 poses) / relpose_6pt_shared_focal (kind 4:
        (count, 6, 3) -> up to 15 poses with f1 = f2 = f, by ascending f) / relpose_7pt (kind 5: (count, 7, 3) -> up to 3
        fundamental matrices in the models' first nine doubles)"""
        K, M = {RELPOSE_5PT: (5, 10), SHARED_6PT: (6, 15), FUNDAMENTAL_7PT: (7, 3)}[kind]
        x1h = np.ascontiguousarray(x1h, dtype=np.float64).reshape(-1, K, 3)
        x2h = np.ascontiguousarray(x2h, dtype=np.float64).reshape(-1, K, 3)
        count = len(x1h)
        out = np.zeros((count, M), dtype=MODEL_DTYPE)
        n_out = np.zeros(count, dtype=np.int32)
        _check(self._lib, self._lib.mdrp_classic_solver_batch(self._h, int(kind), _ptr(x1h), _ptr(x2h), count, _ptr(out), _ptr(n_out)))
        return out, n_out

    def score_models(self, kind, models, x1, x2, sq_threshold):
        models = np.ascontiguousarray(models, dtype=MODEL_DTYPE).reshape(-1)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        x2 = np.ascontiguousarray(x2, dtype=np.float64)
        scores = np.zeros(len(models))
        counts = np.zeros(len(models), dtype=np.int32)
        _check(self._lib, self._lib.mdrp_score_models(self._h, int(kind), MEM_HOST, _ptr(models), len(models), _ptr(x1), _ptr(x2),
                                                      len(x1), float(sq_threshold), _ptr(scores), _ptr(counts)))
        return scores, counts

    def count_candidates(self, kind, models, x1, x2, sq_threshold):
        """k_count alone: per model an upper bound on its inlier count (MFMA pre-pass)"""
        models = np.ascontiguousarray(models, dtype=MODEL_DTYPE).reshape(-1)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        x2 = np.ascontiguousarray(x2, dtype=np.float64)
        cand = np.zeros(len(models), dtype=np.int32)
        _check(self._lib, self._lib.mdrp_count_candidates(self._h, int(kind), _ptr(models), len(models), _ptr(x1), _ptr(x2), len(x1),
                                                          float(sq_threshold), _ptr(cand)))
        return cand

    def bound_models(self, kind, models, x1, x2, sq_threshold):
        """k_bound alone: per model (lower bound of the MSAC score, upper bound of the inlier count) from the fp32 stage"""
        models = np.ascontiguousarray(models, dtype=MODEL_DTYPE).reshape(-1)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        x2 = np.ascontiguousarray(x2, dtype=np.float64)
        lb = np.zeros(len(models))
        ub = np.zeros(len(models), dtype=np.int32)
        _check(self._lib, self._lib.mdrp_bound_models(self._h, int(kind), _ptr(models), len(models), _ptr(x1), _ptr(x2), len(x1),
                                                      float(sq_threshold), _ptr(lb), _ptr(ub)))
        return lb, ub

    def retire_models(self, kind, models, x1, x2, sq_threshold, rec_cnt, rec_score, cand_stat=(0, 0), flags=0):
        """the armed retirement stages on one pair (mdrp_retire_models): k_count (RETIRE_TWO_PHASE: phase A + B) -> k_bound (RETIRE_BOUND) -> the
        exact sweep RETIRE_SWEEP_*, against the records (rec_cnt, rec_score); rec_score None or inf: no record.  Returns (scores, counts, left_at,
        info, cand_stat): the slots (count -2: retired), 1 / 2 / 3 = left at k_count / at k_bound / reached the sweep, info = (undecided after
        phase A, survivors of the count, survivors of the bound), and the pair's candidate statistics after the run"""
        fn = _fn(self._lib, "mdrp_retire_models")
        models = np.ascontiguousarray(models, dtype=MODEL_DTYPE).reshape(-1)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        x2 = np.ascontiguousarray(x2, dtype=np.float64)
        scores = np.zeros(len(models))
        counts = np.zeros(len(models), dtype=np.int32)
        left_at = np.zeros(len(models), dtype=np.int32)
        info = np.zeros(3, dtype=np.int32)
        cs_in = np.array([int(cand_stat[0]), int(cand_stat[1])], dtype=np.uint64)
        cs_out = np.zeros(2, dtype=np.uint64)
        score = np.finfo(np.float64).max if rec_score is None or not rec_score < np.finfo(np.float64).max else float(rec_score)
        _check(self._lib, fn(self._h, int(kind), _ptr(models), len(models), _ptr(x1), _ptr(x2), len(x1), float(sq_threshold),
                             int(rec_cnt), score, _ptr(cs_in), int(flags), _ptr(scores), _ptr(counts), _ptr(left_at), _ptr(info), _ptr(cs_out)))
        return scores, counts, left_at, info, cs_out

    def replay_slots(self, mps, sample_sz, chunk_start, chunk_lens, ropt, states, slot_score, slot_inl, models, lo_score, lo_cnt, lo_models, budgets=None,
                     checkpoints=None):
        """the bookkeeping train of one super-chunk on caller-given tables (mdrp_replay_slots): k_scan per chunk -> k_lo_plan -> k_walk (k_walk_ckpt
        with budgets), the LO results taken from the lo_* tables.  states: REPLAY_STATE_DTYPE [batch]; the six tables [batch][super_len * mps]
        (models: MODEL_DTYPE); checkpoints: REPLAY_STATE_DTYPE [n_budgets][batch] of the call before, or None.  Returns dict(states, triggers: one
        REPLAY_TRIGGER_DTYPE array per pair, n_triggers / scan_cnt / scan_score [n_chunks][batch] behind each scan, scan_inst [n_chunks], prefix,
        begin, end, total of the LO plan, n_active, max_needed, checkpoints)"""
        fn = _fn(self._lib, "mdrp_replay_slots")
        lens = np.ascontiguousarray(chunk_lens, dtype=np.int32).reshape(-1)
        states = np.array(states, dtype=REPLAY_STATE_DTYPE).reshape(-1)  # (a copy: in and out)
        batch, nc, slots = len(states), len(lens), int(lens.sum()) * int(mps)
        tabs = [np.ascontiguousarray(a, dtype=dt).reshape(batch, -1) for a, dt in ((slot_score, np.float64), (slot_inl, np.int32), (models, MODEL_DTYPE),
                                                                                  (lo_score, np.float64), (lo_cnt, np.int32), (lo_models, MODEL_DTYPE))]
        for a in tabs:
            if a.shape[1] != slots:
                raise ValueError(f"replay_slots: a table of {a.shape[1]} slots per pair, expected {slots}")
        bud = None if budgets is None else np.ascontiguousarray(budgets, dtype=np.uint64).reshape(-1)
        nb = 0 if bud is None else len(bud)
        ck = np.zeros((nb, batch), dtype=REPLAY_STATE_DTYPE) if checkpoints is None else np.array(checkpoints, dtype=REPLAY_STATE_DTYPE).reshape(nb, batch)
        trig = np.zeros((batch, int(lens.sum())), dtype=REPLAY_TRIGGER_DTYPE)
        ntr, scnt, ssc = np.zeros((nc, batch), np.int32), np.zeros((nc, batch), np.uint64), np.zeros((nc, batch), np.float64)
        inst, plan, nact, need = np.zeros(nc, np.int32), np.zeros(3 * batch + 2, np.int32), np.zeros(1, np.int32), np.zeros(1, np.uint64)
        io = Replay(int(mps), int(sample_sz), batch, nc, int(chunk_start), _ptr(lens), *[_ptr(a) for a in tabs], _ptr(bud), nb, 0, _ptr(states),
                    _ptr(ck) if nb else None, _ptr(trig), _ptr(ntr), _ptr(scnt), _ptr(ssc), _ptr(inst), _ptr(plan), _ptr(nact), _ptr(need))
        _check(self._lib, fn(self._h, C.byref(ropt), C.byref(io)))
        return dict(states=states, triggers=[trig[p, :ntr[-1, p]] for p in range(batch)], n_triggers=ntr, scan_cnt=scnt, scan_score=ssc, scan_inst=inst,
                    prefix=plan[:batch + 1], begin=plan[batch + 1:2 * batch + 1], end=plan[2 * batch + 1:3 * batch + 1], total=int(plan[3 * batch + 1]),
                    n_active=int(nact[0]), max_needed=int(need[0]), checkpoints=ck)

    def front_lists(self, n, sq_thr, active, lists, pick, slot_score, slot_inl, fill=None):
        """k_first_pick -> k_first_filter on caller-given lists (mdrp_front_lists), one pair per entry of `lists`: uint32 arrays of tags
        slot | key << 24.  slot_score, slot_inl: [batch][slots].  fill: dict of initial values of the outputs (tag lists: uint32, counters: int32),
        which an inactive pair keeps.  Returns dict(picked, rest, kept: one uint32 array per pair, in the kernels' order; pick_count, rest_count
        [2 batch], surv_count; evals; tags_pick, tags_rest, tags_out: the whole buffers)"""
        fn = _fn(self._lib, "mdrp_front_lists")
        slot_score = np.ascontiguousarray(slot_score, dtype=np.float64)
        slot_inl = np.ascontiguousarray(slot_inl, dtype=np.int32)
        batch, slots = slot_inl.shape
        if slot_score.shape != (batch, slots) or len(lists) != batch:
            raise ValueError("front_lists: one list per pair and two tables [batch][slots]")
        n = np.ascontiguousarray(n, dtype=np.int32).reshape(batch)
        thr = np.ascontiguousarray(sq_thr, dtype=np.float64).reshape(batch)
        act = np.ascontiguousarray(active, dtype=np.int32).reshape(batch)
        count = np.array([len(t) for t in lists], dtype=np.int32)
        if count.max(initial=0) > slots:
            raise MdrpError("front_lists: a list longer than the table")
        tags = np.zeros((batch, slots), dtype=np.uint32)
        for p, t in enumerate(lists):
            tags[p, :len(t)] = t
        fill = fill or {}
        bufs = {k: np.full((batch, slots), fill.get(k, 0xFFFFFFFF), dtype=np.uint32) for k in ("tags_pick", "tags_rest", "tags_out")}
        cnts = {k: np.full(batch * w, fill.get(k, -7), dtype=np.int32) for k, w in (("pick_count", 1), ("rest_count", 2), ("surv_count", 1))}
        evals = np.zeros(1, dtype=np.uint64)
        io = FrontTables(batch, slots, int(pick), 0, _ptr(n), _ptr(act), _ptr(thr), _ptr(count), _ptr(tags), _ptr(slot_score), _ptr(slot_inl),
                         _ptr(bufs["tags_pick"]), _ptr(bufs["tags_rest"]), _ptr(bufs["tags_out"]), _ptr(cnts["pick_count"]), _ptr(cnts["rest_count"]),
                         _ptr(cnts["surv_count"]), _ptr(evals))
        _check(self._lib, fn(self._h, C.byref(io)))

        def cut(buf, lens):
            return [buf[p, :max(0, min(int(lens[p]), slots))].copy() for p in range(batch)]
        return dict(picked=cut(bufs["tags_pick"], cnts["pick_count"]), rest=cut(bufs["tags_rest"], cnts["rest_count"][0::2]),
                    kept=cut(bufs["tags_out"], cnts["surv_count"]), evals=int(evals[0]), **bufs, **cnts)

    def front_models(self, kind, models, x1, x2, sq_threshold, pick, rec_cnt=0, rec_score=None):
        """the first chunk's train on one pair (mdrp_front_models): k_count (armed with (rec_cnt, rec_score) unless rec_score is None or inf) -> the
        prefix retirement -> k_score.  Returns (scores, counts, left_at, info): the slots (count -2: retired, -3: a NaN model), 0 / 1 / 4 / 5 / 3 =
        on no list / retired by k_count / picked / retired by k_first_filter / kept and scored, info = (survivors of the count, entries of P, of
        the rest list, of the kept list, hypotheses the filter reports as evaluated)"""
        fn = _fn(self._lib, "mdrp_front_models")
        models = np.ascontiguousarray(models, dtype=MODEL_DTYPE).reshape(-1)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        x2 = np.ascontiguousarray(x2, dtype=np.float64)
        scores = np.zeros(len(models))
        counts = np.zeros(len(models), dtype=np.int32)
        left_at = np.zeros(len(models), dtype=np.int32)
        info = np.zeros(5, dtype=np.int32)
        score = np.finfo(np.float64).max if rec_score is None or not rec_score < np.finfo(np.float64).max else float(rec_score)
        _check(self._lib, fn(self._h, int(kind), _ptr(models), len(models), _ptr(x1), _ptr(x2), len(x1), float(sq_threshold),
                             int(rec_cnt), score, int(pick), _ptr(scores), _ptr(counts), _ptr(left_at), _ptr(info)))
        return scores, counts, left_at, info

    def front_stages(self, kind, x1, x2, d1, d2, ropt, bopt, chunk_lens, n_per_pair=None, cam1=None, cam2=None, slot_iters=None):
        """the scheduler's own stages in front of the sweeps (mdrp_front_stages): plan, parameters, k_prep / kc_prep, then the sample tables and the
        minimal solver of every chunk of `chunk_lens`, in order.  slot_iters: iterations per pair the slot outputs hold (None: the chunks' sum).
        Returns dict(pts (B, N, 6), dep (B, N, 2) or None, rfrag (B, ceil(N / 16), 64, 4) uint32, states FRONT_STATE_DTYPE (B,), table_of_pair (B,),
        table_n (n_tables,), samples (n_tables, super_len, K), slot_inl (n_chunks, B, slot_iters, MPS), models (B, slot_iters, MPS),
        tags (n_chunks, B, slot_iters * MPS), model_count (n_chunks, B, 2), chunk_off (n_chunks,)); what no kernel wrote holds FRONT_FILL bytes"""
        fn = _fn(self._lib, "mdrp_front_stages")
        x1, x2, d1, d2, B, N = _host_batch(x1, x2, d1, d2, "none" if kind >= RELPOSE_5PT else "optional")
        npp, c1, c2 = _tables(n_per_pair, cam1, cam2)
        lens = np.ascontiguousarray(chunk_lens, dtype=np.int32).reshape(-1)
        K, mps, nc, total = SAMPLE_SIZE.get(kind, 3), MODEL_SLOTS.get(kind, 4), len(lens), int(lens.sum())
        iters = total if slot_iters is None else int(slot_iters)
        S = max(iters, 0) * mps

        def filled(shape, dtype):
            a = np.empty(shape, dtype=dtype)
            a.view(np.uint8).fill(FRONT_FILL)
            return a
        pts, dep = filled((B, N, 6), np.float64), filled((B, N, 2), np.float64) if kind < RELPOSE_5PT else None
        rfrag, states = filled((B, (N + 15) // 16, 64, 4), np.uint32), filled(B, FRONT_STATE_DTYPE)
        table_of, table_n, n_tables = filled(B, np.int32), filled(B, np.int32), np.zeros(1, dtype=np.int32)
        samples = filled((B, max(total, 0), K), np.uint32)
        slot_inl, models = filled((nc, B, S), np.int32), filled((B, S), MODEL_DTYPE)
        tags, model_count = filled((nc, B, S), np.uint32), filled((nc, B, 2), np.int32)
        io = FrontRun(int(kind), B, N, nc, iters, 0, _ptr(x1), _ptr(x2), _ptr(d1), _ptr(d2), _ptr(npp), _ptr(c1), _ptr(c2), _ptr(lens), _ptr(pts), _ptr(dep),
                      _ptr(rfrag), _ptr(states), _ptr(table_of), _ptr(table_n), _ptr(n_tables), _ptr(samples), _ptr(slot_inl), _ptr(models), _ptr(tags),
                      _ptr(model_count))
        _check(self._lib, fn(self._h, C.byref(ropt), C.byref(bopt), C.byref(io)))
        nt = int(n_tables[0])
        return dict(pts=pts, dep=dep, rfrag=rfrag, states=states, table_of_pair=table_of, table_n=table_n[:nt], samples=samples[:nt],
                    slot_inl=slot_inl.reshape(nc, B, iters, mps), models=models.reshape(B, iters, mps), tags=tags, model_count=model_count,
                    chunk_off=np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64))

    def score_models_device(self, kind, models_ptr, num_models, x1_ptr, x2_ptr, n, sq_threshold, scores_ptr, counts_ptr):
        _check(self._lib, self._lib.mdrp_score_models(self._h, int(kind), MEM_DEVICE, _dev(models_ptr), int(num_models), _dev(x1_ptr), _dev(x2_ptr), int(n),
                                                      float(sq_threshold), _dev(scores_ptr), _dev(counts_ptr)))

    def refine_models(self, kind, models, x1, x2, d1, d2, scale_reproj, weight_sampson, bopt, estimate_shift=False):
        models = np.ascontiguousarray(models, dtype=MODEL_DTYPE).reshape(-1).copy()
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        x2 = np.ascontiguousarray(x2, dtype=np.float64)
        d1 = None if d1 is None else np.ascontiguousarray(d1, dtype=np.float64)
        d2 = None if d2 is None else np.ascontiguousarray(d2, dtype=np.float64)
        cost = np.zeros(len(models))
        _check(self._lib, self._lib.mdrp_refine_models(self._h, int(kind), _ptr(models), len(models), _ptr(x1), _ptr(x2), _ptr(d1),
                                                       _ptr(d2), len(x1), float(scale_reproj), float(weight_sampson), C.byref(bopt),
                                                       int(bool(estimate_shift)), _ptr(cost)))
        return models, cost

    # ---- the varying-focal baseline's tail: focals and pose from F (include/mdrp_classic_focals.h)
    def focals_from_fundamental(self, F, pp1=None, pp2=None):
        """F (B, 3, 3) or (B, 9) row-major, pp1 / pp2 (B, 2) or None (the origin) -> (B, 2) focals, NaN where not real (mdrp_focals_from_fundamental)"""
        F = np.ascontiguousarray(F, dtype=np.float64).reshape(-1, 9)
        B = len(F)
        pp1 = None if pp1 is None else np.ascontiguousarray(pp1, dtype=np.float64).reshape(B, 2)
        pp2 = None if pp2 is None else np.ascontiguousarray(pp2, dtype=np.float64).reshape(B, 2)
        out = np.zeros((B, 2))
        _check(self._lib, _fn(self._lib, "mdrp_focals_from_fundamental")(self._h, MEM_HOST, _ptr(F), _ptr(pp1), _ptr(pp2), B, _ptr(out)))
        return out

    def focals_from_fundamental_device(self, F_ptr, pp1_ptr, pp2_ptr, batch, out_ptr):
        _check(self._lib, _fn(self._lib, "mdrp_focals_from_fundamental")(self._h, MEM_DEVICE, _dev(F_ptr), _dev(pp1_ptr), _dev(pp2_ptr), int(batch),
                                                                         _dev(out_ptr)))

    def pose_from_fundamental(self, x1, x2, models, n_per_pair=None, mask=None, pp1=None, pp2=None):
        """host buffers: x1, x2 (B, N, 2); models: (B,) MODEL_DTYPE or RESULT_DTYPE records holding F (the record size is the stride); mask (B, N)
        uint8 or None; pp1 / pp2 (B, 2) or None -> (B,) FOCAL_POSE_DTYPE (mdrp_pose_from_fundamental)"""
        x1, x2, _, _, B, N = _host_batch(x1, x2)
        models = np.ascontiguousarray(models).reshape(-1)
        if models.dtype not in (MODEL_DTYPE, RESULT_DTYPE) or len(models) != B:
            raise ValueError(f"models: {B} records of _capi.MODEL_DTYPE or _capi.RESULT_DTYPE")
        npp = _tables(n_per_pair, None, None)[0]
        mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(B, N)
        pp1 = None if pp1 is None else np.ascontiguousarray(pp1, dtype=np.float64).reshape(B, 2)
        pp2 = None if pp2 is None else np.ascontiguousarray(pp2, dtype=np.float64).reshape(B, 2)
        out = np.zeros(B, dtype=FOCAL_POSE_DTYPE)
        _check(self._lib, _fn(self._lib, "mdrp_pose_from_fundamental")(self._h, MEM_HOST, _ptr(x1), _ptr(x2), B, N, _ptr(npp), _ptr(models),
                                                                       models.dtype.itemsize, _ptr(mask), _ptr(pp1), _ptr(pp2), _ptr(out)))
        return out

    def pose_from_fundamental_device(self, x1_ptr, x2_ptr, batch, n_max, models_ptr, stride, out_ptr, n_per_pair=None, mask_ptr=None, pp1_ptr=None,
                                     pp2_ptr=None, blocking_out=None):
        """device pointers (ints).  blocking_out None: mdrp_pose_from_fundamental_async into out_ptr (device); a FOCAL_POSE_DTYPE array: the blocking
        call with mem_space = device, the records into that host array (out_ptr is not read)"""
        npp = _tables(n_per_pair, None, None)[0]
        args = (_dev(x1_ptr), _dev(x2_ptr), int(batch), int(n_max), _ptr(npp), _dev(models_ptr), int(stride), _dev(mask_ptr), _dev(pp1_ptr), _dev(pp2_ptr))
        if blocking_out is None:
            _check(self._lib, _fn(self._lib, "mdrp_pose_from_fundamental_async")(self._h, *args, _dev(out_ptr)))
        else:
            _check(self._lib, _fn(self._lib, "mdrp_pose_from_fundamental")(self._h, MEM_DEVICE, *args, _ptr(blocking_out)))

    def estimate_fundamental_focals_device(self, x1_ptr, x2_ptr, batch, n_max, ropt, bopt, out_ptr, n_per_pair=None, mask_ptr=None, pp1_ptr=None,
                                           pp2_ptr=None):
        """the 7-point estimate with the tail queued behind it (mdrp_estimate_fundamental_focals_async); the F records through fetch_results"""
        npp = _tables(n_per_pair, None, None)[0]
        _check(self._lib, _fn(self._lib, "mdrp_estimate_fundamental_focals_async")(self._h, _dev(x1_ptr), _dev(x2_ptr), int(batch), int(n_max), _ptr(npp),
                                                                                   C.byref(ropt), C.byref(bopt), _dev(mask_ptr), _dev(pp1_ptr), _dev(pp2_ptr),
                                                                                   _dev(out_ptr)))

    # ---- the front end for dense matchers (include/mdrp_dense.h): a DenseMatches descriptor of device pointers.  Arguments go to the library as they
    # are: the library checks them.
    def sample_dense(self, desc, batch, x1_ptr, x2_ptr, d1_ptr, d2_ptr, rows_ptr, score_ptr):
        """the sampler alone into the caller's device buffers ([batch][n]); returns the records per pair (numpy int32).  Synchronises the stream once."""
        return self._gather("mdrp_sample_dense", desc, batch, (x1_ptr, x2_ptr, d1_ptr, d2_ptr, rows_ptr, score_ptr))

    def estimate_dense_device(self, kind, desc, batch, ropt, bopt, cam1=None, cam2=None, record_mask_ptr=None):
        """sampler + estimator on the handle's stream; results stay on the device (fetch_results / copy_results_device); desc.rows_out / score_out
        receive the records' rows and certainties.  Returns the records per pair (numpy int32)."""
        return self._estimate_front("mdrp_estimate_dense", kind, desc, batch, ropt, bopt, cam1, cam2, record_mask_ptr)


_default_tls = threading.local()


def default_handle(device=0):
    """The calling THREAD's handle for `device` (created on first use): the drop-in entry points release the GIL inside
    the C call like the reference does, so two Python threads must not share scratch buffers — each gets its own handle
    and stream, and their batches run concurrently on the GPU."""
    handles = getattr(_default_tls, "handles", None)
    if handles is None:
        handles = _default_tls.handles = {}
    h = handles.get(device)
    if h is None:
        h = handles[device] = Handle(device)
    return h


def fundamental_to_model(F):
    """a 3 x 3 fundamental matrix as an MDRP_FUNDAMENTAL_7PT model record (row-major in the first nine doubles)"""
    m = np.zeros((), dtype=MODEL_DTYPE)
    flat = np.asarray(F, dtype=np.float64).reshape(9)
    m["q"] = flat[:4]; m["t"] = flat[4:7]; m["scale"] = flat[7]; m["shift1"] = flat[8]
    m["f1"] = m["f2"] = 1.0
    return m


def model_to_fundamental(m):
    return np.r_[m["q"], m["t"], m["scale"], m["shift1"]].reshape(3, 3).copy()


def model_to_array(m):
    """structured MODEL_DTYPE scalar -> flat (12,) float64 [q t scale shift1 shift2 f1 f2]"""
    return np.concatenate([m["q"], m["t"], [m["scale"], m["shift1"], m["shift2"], m["f1"], m["f2"]]]).astype(np.float64)


def array_to_models(a):
    a = np.asarray(a, dtype=np.float64).reshape(-1, 12)
    out = np.zeros(len(a), dtype=MODEL_DTYPE)
    out["q"] = a[:, :4]; out["t"] = a[:, 4:7]; out["scale"] = a[:, 7]; out["shift1"] = a[:, 8]; out["shift2"] = a[:, 9]
    out["f1"] = a[:, 10]; out["f2"] = a[:, 11]
    return out
