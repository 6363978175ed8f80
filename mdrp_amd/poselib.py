"""Drop-in for the monodepth part of the reference's `poselib` module, backed by the HIP kernels.

    import mdrp_amd.poselib as poselib
    geometry, info = poselib.estimate_monodepth_relative_pose(x1, x2, d1, d2, cam1, cam2, ransac_opt, bundle_opt)

Signatures, option dictionaries, result classes and the `info` dictionary follow the reference binding
(wheel poselib/_core.pyi:446-501, 134-204; callers /root/reference/make_pair.py:111, make_video.py:284,
README.md:86-96).  Each single-pair call is a batch of one; `*_batch` variants take B pairs at once, which is how
the GPU is meant to be fed (the reference parallelises over pairs with a process pool, eval.py:355-359).
The fork names used by the paper scripts (eval.py:153, eval_shared_f.py:177, eval_varying_f.py:168) are provided as
adapters at the bottom.
"""
import numpy as np

from . import _capi, pipeline

__version__ = "2.0.5+mdrp_amd"

CAMERA_MODELS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1}
CAMERA_MODEL_NAMES = {v: k for k, v in CAMERA_MODELS.items()}


def _quat_to_R(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


class CameraPose:
    """q = (w,x,y,z), x_cam = R X + t  (_core.pyi:134-156)"""

    def __init__(self, q=None, t=None):
        self.q = np.array([1.0, 0.0, 0.0, 0.0]) if q is None else np.asarray(q, dtype=np.float64).reshape(4)
        self.t = np.zeros(3) if t is None else np.asarray(t, dtype=np.float64).reshape(3)

    @property
    def R(self):
        return _quat_to_R(self.q)

    @property
    def Rt(self):
        return np.hstack([self.R, self.t.reshape(3, 1)])

    def center(self):
        return -self.R.T @ self.t

    def __repr__(self):
        return f"[q: {self.q}, t: {self.t}]"


class Camera:
    """COLMAP-style pinhole camera (_core.pyi:76-132).  Only the models the reference callers use."""

    def __init__(self, model="SIMPLE_PINHOLE", params=None, width=-1, height=-1):
        if isinstance(model, str):
            if model not in CAMERA_MODELS:
                raise NotImplementedError(f"camera model {model!r}: only SIMPLE_PINHOLE and PINHOLE are on the monodepth path")
            model = CAMERA_MODELS[model]
        self.model_id = int(model)
        self.params = [1.0, 0.0, 0.0] if params is None else [float(p) for p in params]
        self.width, self.height = int(width), int(height)

    @classmethod
    def from_any(cls, c):
        if isinstance(c, Camera):
            return c
        if isinstance(c, dict):
            return cls(c["model"], c["params"], c.get("width", -1), c.get("height", -1))
        raise TypeError("camera must be a Camera or a dict {'model','width','height','params'}")

    def model_name(self):
        return CAMERA_MODEL_NAMES[self.model_id]

    def focal_x(self):
        return self.params[0]

    def focal_y(self):
        return self.params[1] if self.model_id == 1 else self.params[0]

    def focal(self):
        return 0.5 * (self.focal_x() + self.focal_y())

    def principal_point(self):
        return np.array(self.params[2:4] if self.model_id == 1 else self.params[1:3])

    def unproject(self, x):
        x = np.asarray(x, dtype=np.float64)
        return (x - self.principal_point()) / np.array([self.focal_x(), self.focal_y()])

    def project(self, x):
        x = np.asarray(x, dtype=np.float64)
        return x * np.array([self.focal_x(), self.focal_y()]) + self.principal_point()

    def _record(self):
        r = np.zeros((), dtype=_capi.CAMERA_DTYPE)
        r["model_id"] = self.model_id
        p = np.zeros(4)
        p[: len(self.params)] = self.params
        r["params"] = p
        return r

    def __repr__(self):
        return f"Camera({self.model_name()}, params={self.params}, {self.width}x{self.height})"


class MonoDepthTwoViewGeometry:
    """R (d1+shift1) K1^-1 x1 + t = scale (d2+shift2) K2^-1 x2  (_core.pyi:178-204)"""

    def __init__(self, pose=None, scale=1.0, shift1=0.0, shift2=0.0):
        self.pose = pose if pose is not None else CameraPose()
        self.scale, self.shift1, self.shift2 = float(scale), float(shift1), float(shift2)

    def __repr__(self):
        return f"[pose: {self.pose}, scale: {self.scale}, shift1: {self.shift1}, shift2: {self.shift2}]"


class MonoDepthImagePair:
    """(_core.pyi:171-176); `.pose` is kept for the older wheel's naming used by eval_shared_f.py:84-96"""

    def __init__(self, geometry=None, camera1=None, camera2=None):
        self.geometry = geometry if geometry is not None else MonoDepthTwoViewGeometry()
        self.camera1 = camera1 if camera1 is not None else Camera()
        self.camera2 = camera2 if camera2 is not None else Camera()

    @property
    def pose(self):
        return self.geometry.pose

    def __repr__(self):
        return f"[geometry: {self.geometry}, camera1: {self.camera1}, camera2: {self.camera2}]"


def _geometry_from_model(m):
    return MonoDepthTwoViewGeometry(CameraPose(m["q"].copy(), m["t"].copy()), m["scale"], m["shift1"], m["shift2"])


def _pair_from_model(m):
    return MonoDepthImagePair(_geometry_from_model(m), Camera("SIMPLE_PINHOLE", [float(m["f1"]), 0.0, 0.0]),
                              Camera("SIMPLE_PINHOLE", [float(m["f2"]), 0.0, 0.0]))


def _info(res, mask_row, n):
    return {"refinements": int(res["refinements"]), "iterations": int(res["iterations"]), "num_inliers": int(res["num_inliers"]),
            "inlier_ratio": float(res["inlier_ratio"]), "model_score": float(res["model_score"]),
            "inliers": np.asarray(mask_row[:n]).astype(bool).tolist()}  # list[bool] like the reference, built at C speed


def _as_points(p):
    p = np.ascontiguousarray(p, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError("points must have shape (N, 2)")
    return p


def _with_initial(initial, ransac_opt):
    """The reference binding sets RansacOptions::score_initial_model whenever an initial pose / image pair is passed
    (_core.pyi:455; upstream pybind wrapper).  What the reference does with it, pinned in tests/golden/initial.npz from the
    binary: the POSE handed in is never read — ransac_*_relpose reset it to the identity — and the reset model (no inliers,
    score N eps^2) is scored and LO-refined first, to no effect except `refinements` + 1 and the records it sets."""
    ro = dict(ransac_opt or {})
    if initial is not None:
        ro["score_initial_model"] = True
    return ro


def _initial_fallback(initial, geometry):
    """When RANSAC adopts nothing the reference returns the caller's model with its pose reset: scale and shifts of the
    initial geometry survive (cameras of an initial image pair do not: they come back as the normalisation focal)."""
    if initial is None:
        return geometry
    g0 = getattr(initial, "geometry", initial)
    p = geometry.pose
    if tuple(p.q) == (1.0, 0.0, 0.0, 0.0) and not p.t.any() and geometry.scale == 1.0:
        geometry.scale, geometry.shift1, geometry.shift2 = float(g0.scale), float(g0.shift1), float(g0.shift2)
    return geometry


def _camera_records(c, B):
    """[B] mdrp_camera records: one Camera | dict for all pairs (one record, repeated — no per-pair Python objects), a list of B, or a
    ready CAMERA_DTYPE array"""
    if isinstance(c, np.ndarray) and c.dtype == _capi.CAMERA_DTYPE:
        if len(c) != B:
            raise ValueError(f"expected {B} camera records, got {len(c)}")
        return np.ascontiguousarray(c)
    if not isinstance(c, (list, tuple)):
        return np.repeat(np.asarray(Camera.from_any(c)._record()).reshape(1), B)
    if len(c) != B:
        raise ValueError(f"expected {B} cameras, got {len(c)}")
    return np.array([Camera.from_any(v)._record() for v in c], dtype=_capi.CAMERA_DTYPE)


# ------------------------------------------------------------------------------------------------ batch API
# budgets=[K_0 < ... < K_{C-1}] on a *_batch entry point: the result at every iteration budget from ONE run (include/mdrp.h), each bit
# for bit what the call with max_iterations = K_c returns.  ransac_opt['max_iterations'] is set to the last budget when absent and must equal it
# when present (ValueError, as for an invalid list: checked before anything else).  The return value gains a leading budget axis: the two lists
# become lists over the budgets of today's lists (geometries[c][i], infos[c][i]); as_arrays and the torch form return records (C, B) and masks
# (C, B, N).
def _budget_args(ransac_opt, budgets):
    """(ransac option dict, uint64 budgets or None)"""
    if budgets is None:
        return ransac_opt, None
    ks, ro = _capi.budget_list(budgets, ransac_opt)
    return ro, ks


def _per_budget(budgets, res, mask, build):
    """build(records (B,), masks (B, N)) -> (objects, infos): once, or per budget plane"""
    if budgets is None:
        return build(res, mask)
    parts = [build(res[c], mask[c]) for c in range(len(res))]
    return [p[0] for p in parts], [p[1] for p in parts]


# priors=[...] on a monodepth *_batch entry point (prior= on the single-pair forms): the search of each pair STARTS from the caller's model — scored
# and LO-refined first, as ransac<> treats an initial model under score_initial_model, and not reset to the identity (include/mdrp.h:
# mdrp_estimate_batch_prior).  Everything is still sampled, so a wrong prior costs one LM and cannot give a wrong answer.  An entry that
# is None (a NaN quaternion in a record array) is a pair without a prior.  Not with budgets.  initial_pose / initial_image_pair keep the
# reference's semantics (_with_initial): that model is reset, never read.
def _prior_records(priors, kind, B):
    """list of MonoDepthTwoViewGeometry / MonoDepthImagePair / None, or a MODEL_DTYPE array -> [B] MODEL_DTYPE records (None: a NaN record)"""
    if isinstance(priors, np.ndarray):
        if priors.dtype != _capi.MODEL_DTYPE:
            raise ValueError("priors: a numpy array must have dtype _capi.MODEL_DTYPE")
        rec = np.ascontiguousarray(priors).reshape(-1)
    else:
        priors = list(priors)
        rec = np.zeros(len(priors), dtype=_capi.MODEL_DTYPE)
        have = [i for i, p in enumerate(priors) if p is not None]
        rec["q"] = np.nan
        rec["scale"] = rec["f1"] = rec["f2"] = 1.0
        if have:
            rec[have] = _model_records([priors[i] for i in have], kind)
    if len(rec) != B:
        raise ValueError(f"priors: expected {B} models, got {len(rec)}")
    return rec


def _no_budgets_with_priors(priors, budgets):
    if priors is not None and budgets is not None:
        raise ValueError("priors and budgets do not combine: run the budgets without priors, or one call per budget")


# scores=... on a monodepth *_batch entry point, on the single-pair forms, on estimate_batch_torch and on the device front end (one score per MATCH
# ROW there: gather_matches_torch, estimate_matches_torch and the image-pairs forms rank inside the gather): the estimate in match-score order with the
# reference's progressive sampler (PROSAC; include/mdrp.h mdrp_estimate_batch_ranked).  One score per correspondence, higher is better
# (a matcher's confidence), or the string "presorted" for records that are in quality order already.  progressive_sampling in ransac_opt may be
# absent, False or True: scores= is what asks for the sampler; max_prosac_iterations is read.  Masks and info["inliers"] stay in the caller's order.
# Not with budgets or priors.
PRESORTED = "presorted"


def _no_scores_with(scores, budgets, priors):
    if scores is not None and (budgets is not None or priors is not None):
        raise ValueError("scores do not combine with budgets or priors: rank without them, or run them without scores")


def _score_rows(scores, ns, N):
    """scores of a host batch -> (B, N) float64 padded with -inf, or None for "presorted"; checked against the pairs' sizes"""
    if isinstance(scores, str):
        if scores != PRESORTED:
            raise ValueError(f'scores: the only string is "{PRESORTED}", not {scores!r}')
        return None
    B = len(ns)
    if isinstance(scores, np.ndarray) and scores.ndim == 2:
        rows = [scores[i] for i in range(scores.shape[0])]
    else:
        rows = [np.asarray(r).reshape(-1) for r in scores]
    if len(rows) != B:
        raise ValueError(f"scores: expected {B} rows, got {len(rows)}")
    out = np.full((B, N), -np.inf)
    for i, r in enumerate(rows):
        if len(r) != ns[i] and len(r) != N:
            raise ValueError(f"scores: pair {i} has {ns[i]} correspondences and {len(r)} scores")
        if np.asarray(r).dtype.kind not in "fiub":
            raise ValueError(f"scores: pair {i} has dtype {np.asarray(r).dtype}, not real numbers")
        out[i, :ns[i]] = np.asarray(r, dtype=np.float64)[:ns[i]]
    return out


def _ranked_host(kind, x1, x2, d1, d2, ns, scores, cams1, cams2, ransac_opt, bundle_opt, device):
    """(records, masks) of a host batch in score order: one blocking call on the device's default handle"""
    rows = _score_rows(scores, ns, x1.shape[1])  # (checked before anything touches the device)
    return _capi.default_handle(device).estimate_batch_ranked(kind, x1, x2, d1, d2, rows, _capi.ransac_opt_from_dict(ransac_opt),
                                                              _capi.bundle_opt_from_dict(bundle_opt), ns, cams1, cams2)


def _prior_host(kind, x1, x2, d1, d2, ns, priors, cams1, cams2, ransac_opt, bundle_opt, device):
    """(records, masks) of a host batch with priors: one blocking call on the device's default handle"""
    rec = _prior_records(priors, kind, len(ns))  # (checked before anything touches the device)
    return _capi.default_handle(device).estimate_batch_prior(kind, x1, x2, d1, d2, rec, _capi.ransac_opt_from_dict(ransac_opt),
                                                             _capi.bundle_opt_from_dict(bundle_opt), ns, cams1, cams2)


def _stack(points1, points2, depth1, depth2):
    """list of ragged pairs or already-stacked arrays -> padded (B,N,2),(B,N,2),(B,N),(B,N), n_per_pair"""
    if isinstance(points1, np.ndarray) and points1.ndim == 3:
        B, N = points1.shape[:2]
        return (np.ascontiguousarray(points1, np.float64), np.ascontiguousarray(points2, np.float64),
                np.ascontiguousarray(depth1, np.float64), np.ascontiguousarray(depth2, np.float64), np.full(B, N, np.int32))
    B = len(points1)
    ns = np.array([len(p) for p in points1], dtype=np.int32)
    N = int(ns.max()) if B else 0
    x1 = np.zeros((B, N, 2)); x2 = np.zeros((B, N, 2)); d1 = np.ones((B, N)); d2 = np.ones((B, N))
    for i in range(B):
        n = ns[i]
        x1[i, :n] = _as_points(points1[i]); x2[i, :n] = _as_points(points2[i])
        d1[i, :n] = np.asarray(depth1[i], np.float64).reshape(-1); d2[i, :n] = np.asarray(depth2[i], np.float64).reshape(-1)
    return x1, x2, d1, d2, ns


def estimate_monodepth_relative_pose_batch(points2D_1, points2D_2, depth_1, depth_2, cameras1, cameras2, ransac_opt=None,
                                           bundle_opt=None, device=0, as_arrays=False, budgets=None, priors=None, scores=None):
    """B calibrated pairs at once.  cameras1/2: one Camera|dict for all pairs, or a list of B.  Returns
    (list[MonoDepthTwoViewGeometry], list[info dict]) — or, with as_arrays=True, (records, inlier masks, n_per_pair) as numpy arrays
    (_capi.RESULT_DTYPE; (B, N) uint8): building B Python objects and B lists of N bools costs more than the estimate itself beyond
    a few thousand pairs.  A host batch is ONE call whatever its size: the C side copies the correspondences in 256-pair slices on a copy stream
    beside the first kernels of the slices before them (MDRP_PIPELINE_MIN=<pairs> brings back the chunked two-in-flight path of rounds 4-5,
    mdrp_amd.pipeline; results identical to sequential chunk calls).  budgets: see _budget_args above.  priors: a list of B
    MonoDepthTwoViewGeometry | None (or a MODEL_DTYPE array) each pair's search starts from, see _prior_records above.  scores: one score per
    correspondence (a (B, N) array or a list of B arrays) or "presorted": the estimate in score order with the progressive sampler, see PRESORTED above."""
    _no_scores_with(scores, budgets, priors)
    _no_budgets_with_priors(priors, budgets)
    ransac_opt, budgets = _budget_args(ransac_opt, budgets)
    x1, x2, d1, d2, ns = _stack(points2D_1, points2D_2, depth_1, depth_2)
    B = len(ns)

    def cams(c):
        return _camera_records(c, B)

    if scores is not None:
        res, mask = _ranked_host(_capi.CALIB, x1, x2, d1, d2, ns, scores, cams(cameras1), cams(cameras2), ransac_opt, bundle_opt, device)
    elif priors is not None:
        res, mask = _prior_host(_capi.CALIB, x1, x2, d1, d2, ns, priors, cams(cameras1), cams(cameras2), ransac_opt, bundle_opt, device)
    else:
        res, mask = pipeline.estimate_host(_capi.CALIB, x1, x2, d1, d2, _capi.ransac_opt_from_dict(ransac_opt),
                                           _capi.bundle_opt_from_dict(bundle_opt), ns, cams(cameras1), cams(cameras2), device, budgets=budgets)
    if as_arrays:
        return res, mask, ns
    return _per_budget(budgets, res, mask, lambda r, m: ([_geometry_from_model(q["model"]) for q in r], [_info(r[i], m[i], ns[i]) for i in range(B)]))


def _focal_batch(kind, points2D_1, points2D_2, depth_1, depth_2, ransac_opt, bundle_opt, device, as_arrays=False, budgets=None, priors=None, scores=None):
    _no_scores_with(scores, budgets, priors)
    _no_budgets_with_priors(priors, budgets)
    ransac_opt, budgets = _budget_args(ransac_opt, budgets)
    x1, x2, d1, d2, ns = _stack(points2D_1, points2D_2, depth_1, depth_2)
    if scores is not None:
        res, mask = _ranked_host(kind, x1, x2, d1, d2, ns, scores, None, None, ransac_opt, bundle_opt, device)
    elif priors is not None:
        res, mask = _prior_host(kind, x1, x2, d1, d2, ns, priors, None, None, ransac_opt, bundle_opt, device)
    else:
        res, mask = pipeline.estimate_host(kind, x1, x2, d1, d2, _capi.ransac_opt_from_dict(ransac_opt), _capi.bundle_opt_from_dict(bundle_opt), ns, None, None,
                                           device, budgets=budgets)
    if as_arrays:
        return res, mask, ns
    return _per_budget(budgets, res, mask, lambda r, m: ([_pair_from_model(q["model"]) for q in r], [_info(r[i], m[i], ns[i]) for i in range(len(ns))]))


def estimate_monodepth_shared_focal_relative_pose_batch(points2D_1, points2D_2, depth_1, depth_2, ransac_opt=None,
                                                        bundle_opt=None, device=0, as_arrays=False, budgets=None, priors=None, scores=None):
    """priors: a list of B MonoDepthImagePair | None (focals: camera1 / camera2 .focal(), in pixels), see _prior_records; scores: see PRESORTED"""
    return _focal_batch(_capi.SHARED_FOCAL, points2D_1, points2D_2, depth_1, depth_2, ransac_opt, bundle_opt, device, as_arrays, budgets, priors, scores)


def estimate_monodepth_varying_focal_relative_pose_batch(points2D_1, points2D_2, depth_1, depth_2, ransac_opt=None,
                                                         bundle_opt=None, device=0, as_arrays=False, budgets=None, priors=None, scores=None):
    return _focal_batch(_capi.VARYING_FOCAL, points2D_1, points2D_2, depth_1, depth_2, ransac_opt, bundle_opt, device, as_arrays, budgets, priors, scores)


# ------------------------------------------------------------------------------------------------ reference signatures
def _one_scores(scores):
    """scores= of a single-pair form (not in the reference): an array of one score per correspondence, or "presorted" -> the batch forms' argument"""
    return scores if scores is None or isinstance(scores, str) else [np.asarray(scores).reshape(-1)]


def estimate_monodepth_relative_pose(points2D_1, points2D_2, depth_1, depth_2, camera1, camera2, ransac_opt={},
                                     bundle_opt={}, initial_pose=None, prior=None, scores=None):
    """Pose estimation using depth estimates with non-linear refinement (_core.pyi:446-475).  prior (not in the reference): a
    MonoDepthTwoViewGeometry the search starts from (_prior_records); initial_pose keeps the reference's reset semantics."""
    g, i = estimate_monodepth_relative_pose_batch([_as_points(points2D_1)], [_as_points(points2D_2)], [depth_1], [depth_2],
                                                  camera1, camera2, _with_initial(initial_pose, ransac_opt), bundle_opt,
                                                  priors=None if prior is None else [prior], scores=_one_scores(scores))
    return _initial_fallback(initial_pose, g[0]), i[0]


def estimate_monodepth_shared_focal_relative_pose(points2D_1, points2D_2, depth_1, depth_2, ransac_opt={}, bundle_opt={},
                                                  initial_image_pair=None, prior=None, scores=None):
    """Unknown equal focal lengths; points principal-point-centred (_core.pyi:477-488, README.md:88-90).  prior: a MonoDepthImagePair the
    search starts from (_prior_records)."""
    p, i = estimate_monodepth_shared_focal_relative_pose_batch([_as_points(points2D_1)], [_as_points(points2D_2)], [depth_1],
                                                               [depth_2], _with_initial(initial_image_pair, ransac_opt), bundle_opt,
                                                               priors=None if prior is None else [prior], scores=_one_scores(scores))
    _initial_fallback(initial_image_pair, p[0].geometry)
    return p[0], i[0]


def estimate_monodepth_varying_focal_relative_pose(points2D_1, points2D_2, depth_1, depth_2, ransac_opt={}, bundle_opt={},
                                                   initial_image_pair=None, prior=None, scores=None):
    """Two unknown focal lengths (_core.pyi:490-501, README.md:94-96).  `monodepth_estimate_shift` is ignored here
    exactly like in the reference.  prior: a MonoDepthImagePair the search starts from (_prior_records)."""
    p, i = estimate_monodepth_varying_focal_relative_pose_batch([_as_points(points2D_1)], [_as_points(points2D_2)], [depth_1],
                                                                [depth_2], _with_initial(initial_image_pair, ransac_opt), bundle_opt,
                                                                priors=None if prior is None else [prior], scores=_one_scores(scores))
    _initial_fallback(initial_image_pair, p[0].geometry)
    return p[0], i[0]


# ------------------------------------------------------------------------------------------------ the older wheel's names
# demo/poselib_old-2.0.5-cp312-*.whl (poselib/_core.pyi:171-199, 441-497) ships the same three estimators as estimate_monodepth_pose,
# estimate_monodepth_shared_focal_pose and estimate_monodepth_varying_focal_pose; its result type is MonoDepthCameraPose — a CameraPose
# that carries scale, shift_1 and shift_2 itself — and its MonoDepthImagePair holds that as `.pose`.
class MonoDepthCameraPose(CameraPose):
    def __init__(self, q=None, t=None, scale=1.0, shift_1=0.0, shift_2=0.0):
        if isinstance(q, CameraPose):
            q, t = q.q, q.t
        super().__init__(q, t)
        self.scale, self.shift_1, self.shift_2 = float(scale), float(shift_1), float(shift_2)

    def __repr__(self):
        return f"[q: {self.q}, t: {self.t}, scale: {self.scale}, shift_1: {self.shift_1}, shift_2: {self.shift_2}]"


def _old_pose(g):
    return MonoDepthCameraPose(g.pose.q, g.pose.t, g.scale, g.shift1, g.shift2)


def _old_initial(initial):
    """a MonoDepthCameraPose / old-style image pair handed in as the initial value -> today's types (the pose itself is never read:
    the reference resets it, include/mdrp.h score_initial_model)"""
    if initial is None:
        return None
    if isinstance(initial, MonoDepthCameraPose):
        return MonoDepthTwoViewGeometry(CameraPose(initial.q, initial.t), initial.scale, initial.shift_1, initial.shift_2)
    if isinstance(getattr(initial, "pose", None), MonoDepthCameraPose):  # an old-style image pair
        return MonoDepthImagePair(_old_initial(initial.pose), getattr(initial, "camera1", None), getattr(initial, "camera2", None))
    return initial


def estimate_monodepth_pose(points2D_1, points2D_2, depth_1, depth_2, camera1, camera2, ransac_opt={}, bundle_opt={}, initial_pose=None):
    """older wheel's name of estimate_monodepth_relative_pose (poselib_old _core.pyi:441-470); returns (MonoDepthCameraPose, info)"""
    g, info = estimate_monodepth_relative_pose(points2D_1, points2D_2, depth_1, depth_2, camera1, camera2, ransac_opt, bundle_opt, _old_initial(initial_pose))
    return _old_pose(g), info


class _OldImagePair:
    """MonoDepthImagePair of the older wheel: camera1, camera2, pose (a MonoDepthCameraPose)"""

    def __init__(self, pair):
        self.camera1, self.camera2, self.pose = pair.camera1, pair.camera2, _old_pose(pair.geometry)

    def __repr__(self):
        return f"[pose: {self.pose}, camera1: {self.camera1}, camera2: {self.camera2}]"


def estimate_monodepth_shared_focal_pose(points2D_1, points2D_2, depth_1, depth_2, ransac_opt={}, bundle_opt={}, initial_image_pair=None):
    """older wheel's name of estimate_monodepth_shared_focal_relative_pose (poselib_old _core.pyi:472-483)"""
    p, info = estimate_monodepth_shared_focal_relative_pose(points2D_1, points2D_2, depth_1, depth_2, ransac_opt, bundle_opt,
                                                            _old_initial(initial_image_pair))
    return _OldImagePair(p), info


def estimate_monodepth_varying_focal_pose(points2D_1, points2D_2, depth_1, depth_2, ransac_opt={}, bundle_opt={}, initial_image_pair=None):
    """older wheel's name of estimate_monodepth_varying_focal_relative_pose (poselib_old _core.pyi:485-497)"""
    p, info = estimate_monodepth_varying_focal_relative_pose(points2D_1, points2D_2, depth_1, depth_2, ransac_opt, bundle_opt,
                                                             _old_initial(initial_image_pair))
    return _OldImagePair(p), info


# ------------------------------------------------------------------------------------------------ minimal solvers
def _solver(solver, x1, x2, d1, d2, wrap):
    x1 = np.asarray(x1, dtype=np.float64).reshape(3, 3)
    x2 = np.asarray(x2, dtype=np.float64).reshape(3, 3)
    out, n = _capi.default_handle().solver_batch(solver, x1[None], x2[None], np.asarray(d1, np.float64)[None], np.asarray(d2, np.float64)[None])
    return [wrap(out[0, k]) for k in range(int(n[0]))]


def monodepth_pose_3pt(x1, x2, d1, d2):
    """relpose_monodepth_3pt: scale + two shifts, <= 4 solutions (_core.pyi:614-619); x = homogeneous points with z = 1"""
    return _solver(_capi.SOLVER_SHIFT, x1, x2, d1, d2, _geometry_from_model)


def shared_focal_monodepth_pose_3pt(x1, x2, d1, d2):
    """relpose_monodepth_3pt_shared_focal (_core.pyi:871-876)"""
    return _solver(_capi.SOLVER_SHARED, x1, x2, d1, d2, _pair_from_model)


def varying_focal_monodepth_pose_4pt(x1, x2, d1, d2):
    """relpose_monodepth_3pt_varying_focal — the reference's Python name says 4pt (_core.pyi:914-919)"""
    return _solver(_capi.SOLVER_VARYING, x1, x2, d1, d2, _pair_from_model)


# ------------------------------------------------------------------------------------------------ fork-name adapters
# The paper scripts were written against kocurvik/PoseLib-mdrp@iccv-eval, whose RansacOptions carry experiment switches the
# released PR-152 binary (the wheel in /root/reference/demo, the only behaviour that can be pinned here) does not have.
# Every switch eval.py:93-127 / eval_shared_f.py:111-152 / eval_varying_f.py:105-150 can emit is listed: either it selects
# exactly what the PR-152 estimators do (-> mapped), or it selects a fork-only variant (-> NotImplementedError; parity
# unpinned).  Nothing is mapped "to the nearest behaviour" silently.
#   PR-152 calibrated estimator:  monodepth_estimate_shift=False: P3P on the depth of image 1, hybrid LM (Sampson + both
#       reprojections) of R, t, scale, Sampson scoring;  =True: 3-point scale + two shifts solver, the same LM also over both shifts.
#   PR-152 shared / varying focal estimators: 3-point scale + focal(s) solver without shifts, hybrid LM, Sampson scoring.
FORK_FLAG_TABLE = {
    # flag:               (values PR-152 behaviour corresponds to,                                   what any other value selects)
    "use_madpose":        ((False,), "MADPose solvers / optimisation (mad_poselib_*)"),
    "use_reldepth":       ((False,), "3p_reldepth relative-depth solver"),
    "use_4p4d":           ((False,), "4p4d solver (varying focal)"),
    "use_fundamental":    ((False,), "7-point fundamental-matrix baseline inside the monodepth estimator"),
    "use_eigen":          ((False,), "eigen-decomposition variant of the varying-focal solver"),
    "use_reproj":         ((False,), "reprojection-error scoring instead of Sampson (…_reproj)"),
    "optimize_symmetric": ((False,), "symmetric reprojection cost (…_sym_reproj, calibrated)"),
    "sym_repro":          ((False,), "symmetric reprojection cost (…_sym_reproj, focal)"),
    "no_normalization":   ((False,), "no scale normalisation of the pixel coordinates (NN)"),
    "graduated_steps":    ((0,), "graduated LO (GLO)"),
    "optimize_hybrid":    ((True,), "Sampson-only (or reprojection-only) LM instead of the hybrid cost"),
    "lo_iterations":      ((25,), "LO iteration count other than the binary's fixed 25 (nLO)"),
    "progressive_sampling": ((False,), "PROSAC sampling"),
}
_FORK_KEYS = tuple(FORK_FLAG_TABLE) + ("use_p3p", "use_ours", "solver_shift", "solver_scale", "optimize_shift", "all_permutations",
                                       "use_madpose_shift_optim", "weight_sampson")


def _map_fork_options(ransac_opt, kind=_capi.CALIB):
    """Option dict of the paper scripts -> option dict of the PR-152 estimators, or NotImplementedError naming the
    fork-only variant.  Plain PR-152 dicts (none of the fork keys) pass through unchanged."""
    ro = dict(ransac_opt or {})
    if not any(k in ro for k in _FORK_KEYS):
        return ro

    def fork_only(what):
        raise NotImplementedError(f"ransac options select a fork-only variant — {what} — whose behaviour cannot be pinned against "
                                  "the released PoseLib binary (SURVEY.md 8b; mdrp_amd.poselib.FORK_FLAG_TABLE)")

    for flag, (ok, what) in FORK_FLAG_TABLE.items():
        if flag in ro and ro[flag] not in ok and not (isinstance(ro[flag], bool) and int(ro[flag]) in [int(v) for v in ok if isinstance(v, bool)]):
            fork_only(f"{flag}={ro[flag]!r}: {what}")
    p3p, ours = bool(ro.get("use_p3p")), bool(ro.get("use_ours"))
    shift, scale, opt_shift = bool(ro.get("solver_shift")), bool(ro.get("solver_scale")), bool(ro.get("optimize_shift"))
    if kind == _capi.CALIB:
        if p3p and not ours and not shift and not opt_shift:
            ro["monodepth_estimate_shift"] = False          # p3p_hybrid*: P3P, LM without shifts
        elif ours and not p3p and shift and scale and opt_shift:
            ro["monodepth_estimate_shift"] = True           # 3p_ours_shift_scale_hybrid-s*: shift solver, LM over the shifts too
        elif p3p or ours or shift or scale or opt_shift:
            fork_only(f"use_p3p={p3p}, use_ours={ours}, solver_shift={shift}, solver_scale={scale}, optimize_shift={opt_shift}: the "
                      "released estimator ties the shift solver and the shift optimisation together (monodepth_estimate_shift) and "
                      "has no scale-only / shift-only 3-point solver")
        # all_permutations: the calibrated 3-point solvers are symmetric in the sample, permutations change nothing -> accepted
    else:
        if ours and not p3p and scale and not shift and not opt_shift:
            pass                                            # 3p_ours_scale_hybrid*: the PR-152 focal estimators
        elif p3p or ours or shift or scale or opt_shift:
            fork_only(f"use_p3p={p3p}, use_ours={ours}, solver_shift={shift}, solver_scale={scale}, optimize_shift={opt_shift}: the "
                      "released focal estimators are the 3-point scale + focal solvers without shifts")
        if ro.get("all_permutations"):
            fork_only("all_permutations=True: the shared-focal solver treats the third correspondence differently; the released "
                      "estimator runs the sample order as drawn")
    if "weight_sampson" in ro:
        ro["monodepth_weight_sampson"] = ro["weight_sampson"]
    return ro


def estimate_relative_pose_w_mono_depth(kp1, kp2, d, camera1, camera2, ransac_opt={}, bundle_opt={}):
    """eval.py:153 — d is (N,2) with the two depth columns; returns (pose-like with .R/.t, info)"""
    d = np.asarray(d, dtype=np.float64)
    g, info = estimate_monodepth_relative_pose(kp1, kp2, d[:, 0], d[:, 1], camera1, camera2, _map_fork_options(ransac_opt), bundle_opt)
    pose = g.pose
    pose.scale, pose.shift1, pose.shift2 = g.scale, g.shift1, g.shift2
    return pose, info


def estimate_shared_focal_monodepth_relative_pose(kp1, kp2, d, ransac_opt={}, bundle_opt={}):
    """eval_shared_f.py:177"""
    d = np.asarray(d, dtype=np.float64)
    return estimate_monodepth_shared_focal_relative_pose(kp1, kp2, d[:, 0], d[:, 1], _map_fork_options(ransac_opt, _capi.SHARED_FOCAL), bundle_opt)


def estimate_varying_focal_monodepth_relative_pose(kp1, kp2, d, ransac_opt={}, bundle_opt={}):
    """eval_varying_f.py:168"""
    d = np.asarray(d, dtype=np.float64)
    return estimate_monodepth_varying_focal_relative_pose(kp1, kp2, d[:, 0], d[:, 1], _map_fork_options(ransac_opt, _capi.VARYING_FOCAL), bundle_opt)


def _not_on_path(name, where):
    def stub(*args, **kwargs):
        raise NotImplementedError(f"poselib.{name} ({where}) is a non-monodepth baseline outside the accelerated hot path "
                                  "(SURVEY.md §8f-4 / DESIGN.md §8); use upstream PoseLib for it")
    stub.__name__ = name
    stub.__doc__ = f"{where}: not on the monodepth RANSAC path rebuilt here — raises NotImplementedError."
    return stub


# ------------------------------------------------------------------------------------------------ non-monodepth baselines
# the comparison rows of the paper tables run through the same kernels (sampler, MFMA candidate counts,
# fp32 bound, exact sweep, scan, walk) with the upstream estimators' solvers and Sampson-only LM (mdrp_classic.h).
def _stack2(points1, points2):
    if isinstance(points1, np.ndarray) and points1.ndim == 3:
        B, N = points1.shape[:2]
        return np.ascontiguousarray(points1, np.float64), np.ascontiguousarray(points2, np.float64), np.full(B, N, np.int32)
    B = len(points1)
    ns = np.array([len(p) for p in points1], dtype=np.int32)
    N = int(ns.max()) if B else 0
    x1 = np.zeros((B, N, 2)); x2 = np.zeros((B, N, 2))
    for i in range(B):
        x1[i, :ns[i]] = _as_points(points1[i]); x2[i, :ns[i]] = _as_points(points2[i])
    return x1, x2, ns


def _check_baseline_options(ransac_opt, scores=None):
    """options of upstream RansacOptions that change what the baseline estimators do and are not built here.  progressive_sampling needs the match
    scores: with scores= it may be absent, False or True (see PRESORTED), without them it is refused."""
    ro = ransac_opt or {}
    if ro.get("progressive_sampling") and scores is None:
        raise NotImplementedError("progressive_sampling (PROSAC) needs the match scores: pass scores= (DESIGN.md 7e)")
    if ro.get("real_focal_check"):
        raise NotImplementedError("real_focal_check (FundamentalEstimator drops models without real focal lengths) is not built")


# priors=[...] on a baseline's *_batch entry point (prior= on the single-pair forms): _prior_records' semantics for the 5-, 6- and 7-point estimators
# (include/mdrp_classic_models.h: mdrp_estimate_classic_prior).  A prior is what the estimator returns: a CameraPose (5-point), an
# ImagePair (6-point; the focal is camera1's, in pixels) or a 3 x 3 fundamental matrix for pixel coordinates (7-point); None is a pair without one.
def _baseline_model_records(models, kind, B, what):
    """list of CameraPose / ImagePair / 3 x 3 arrays (None: a NaN record), or a MODEL_DTYPE array -> [B] MODEL_DTYPE records in the caller's units"""
    if isinstance(models, np.ndarray) and models.dtype == _capi.MODEL_DTYPE:
        rec = np.ascontiguousarray(models).reshape(-1)
    else:
        if kind == _capi.FUNDAMENTAL_7PT and isinstance(models, np.ndarray) and models.ndim == 3:
            models = [models[i] for i in range(models.shape[0])]
        if isinstance(models, (np.ndarray, str)) or not hasattr(models, "__len__"):
            raise ValueError(f"{what}: a list with one model per pair, or a numpy array of _capi.MODEL_DTYPE")
        models = list(models)
        rec = np.zeros(len(models), dtype=_capi.MODEL_DTYPE)
        rec["q"] = np.nan
        rec["scale"] = rec["f1"] = rec["f2"] = 1.0
        for i, m in enumerate(models):
            if m is None:
                continue
            if kind == _capi.FUNDAMENTAL_7PT:
                if isinstance(m, (CameraPose, ImagePair)) or np.asarray(m).shape != (3, 3) or np.asarray(m).dtype.kind not in "fiu":
                    raise ValueError(f"{what}: pair {i} needs a 3 x 3 fundamental matrix, not {type(m).__name__}")
                rec[i] = _capi.fundamental_to_model(m)
            elif kind == _capi.SHARED_6PT:
                if not isinstance(m, ImagePair):
                    raise ValueError(f"{what}: pair {i} needs an ImagePair, not {type(m).__name__}")
                rec[i]["q"] = m.pose.q; rec[i]["t"] = m.pose.t
                rec[i]["f1"] = rec[i]["f2"] = m.camera1.focal()
            else:
                if not isinstance(m, CameraPose):
                    raise ValueError(f"{what}: pair {i} needs a CameraPose, not {type(m).__name__}")
                rec[i]["q"] = m.q; rec[i]["t"] = m.t
    if len(rec) != B:
        raise ValueError(f"{what}: expected {B} models, got {len(rec)}")
    return rec


def _baseline_host(kind, x1, x2, ns, scores, cams1, cams2, ransac_opt, bundle_opt, device, budgets, priors=None, prior_space=0):
    """(records, masks) of a baseline's host batch: pipeline.estimate_host, or with scores (see PRESORTED) one blocking ranked call on the device's
    default handle (include/mdrp.h mdrp_estimate_classic_ranked), or with priors one blocking call of mdrp_estimate_classic_prior"""
    if priors is not None:
        rec = _baseline_model_records(priors, kind, len(ns), "priors")  # (checked before anything touches the device)
        return _capi.default_handle(device).estimate_classic_prior(kind, x1, x2, rec, _capi.ransac_opt_from_dict(ransac_opt),
                                                                   _capi.bundle_opt_from_dict(bundle_opt), ns, cams1, cams2, prior_space=prior_space)
    if scores is None:
        return pipeline.estimate_host(kind, x1, x2, None, None, _capi.ransac_opt_from_dict(ransac_opt), _capi.bundle_opt_from_dict(bundle_opt), ns, cams1, cams2,
                                      device, budgets=budgets)
    rows = _score_rows(scores, ns, x1.shape[1])  # (checked before anything touches the device)
    return _capi.default_handle(device).estimate_classic_ranked(kind, x1, x2, rows, _capi.ransac_opt_from_dict(ransac_opt),
                                                                _capi.bundle_opt_from_dict(bundle_opt), ns, cams1, cams2)


def estimate_relative_pose_batch(points2D_1, points2D_2, cameras1, cameras2, ransac_opt=None, bundle_opt=None, device=0, budgets=None, scores=None,
                                 priors=None):
    """B calibrated pairs through the 5-point estimator.  Returns (list[CameraPose], list[info dict]).  budgets: see _budget_args; scores: see
    PRESORTED (not with budgets); priors: see _baseline_model_records (not with budgets or scores)."""
    _no_scores_with(scores, budgets, priors)
    _no_budgets_with_priors(priors, budgets)
    ransac_opt, budgets = _budget_args(ransac_opt, budgets)
    _check_baseline_options(ransac_opt, scores)
    x1, x2, ns = _stack2(points2D_1, points2D_2)
    B = len(ns)

    def cams(c):
        return _camera_records(c, B)

    res, mask = _baseline_host(_capi.RELPOSE_5PT, x1, x2, ns, scores, cams(cameras1), cams(cameras2), ransac_opt, bundle_opt, device, budgets, priors)
    return _per_budget(budgets, res, mask, lambda r, m: ([CameraPose(q["model"]["q"].copy(), q["model"]["t"].copy()) for q in r],
                                                         [_info(r[i], m[i], ns[i]) for i in range(B)]))


def estimate_fundamental_batch(points2D_1, points2D_2, ransac_opt=None, bundle_opt=None, device=0, budgets=None, scores=None, priors=None):
    """B pairs through the 7-point estimator.  Returns (list[3 x 3 ndarray], list[info dict]).  budgets: see _budget_args; scores: see PRESORTED
    (not with budgets); priors: see _baseline_model_records (not with budgets or scores)."""
    _no_scores_with(scores, budgets, priors)
    _no_budgets_with_priors(priors, budgets)
    ransac_opt, budgets = _budget_args(ransac_opt, budgets)
    _check_baseline_options(ransac_opt, scores)
    x1, x2, ns = _stack2(points2D_1, points2D_2)
    res, mask = _baseline_host(_capi.FUNDAMENTAL_7PT, x1, x2, ns, scores, None, None, ransac_opt, bundle_opt, device, budgets, priors)
    return _per_budget(budgets, res, mask, lambda r, m: ([_capi.model_to_fundamental(q["model"]) for q in r], [_info(r[i], m[i], ns[i]) for i in range(len(ns))]))


def estimate_relative_pose(points2D_1, points2D_2, camera1, camera2, ransac_opt={}, bundle_opt={}, initial_pose=None, scores=None, prior=None):
    """Relative pose estimation with non-linear refinement (_core.pyi:504-529; eval.py:136 — the 5-point baseline).  As in the
    monodepth estimators, an initial pose only sets score_initial_model: ransac_relpose resets the pose itself.  scores (not in the reference): see
    PRESORTED.  prior (not in the reference): a CameraPose the search STARTS from, see _baseline_model_records."""
    poses, infos = estimate_relative_pose_batch([_as_points(points2D_1)], [_as_points(points2D_2)], camera1, camera2,
                                                _with_initial(initial_pose, ransac_opt), bundle_opt, scores=_one_scores(scores),
                                                priors=None if prior is None else [prior])
    return poses[0], infos[0]


def estimate_fundamental(points2D_1, points2D_2, ransac_opt={}, bundle_opt={}, initial_F=None, scores=None, prior=None):
    """Fundamental matrix estimation with non-linear refinement (_core.pyi:309-323; the 7-point baseline).  scores (not in the reference): see PRESORTED.
    initial_F: as the reference reads it — scored and LO-refined first, not reset.  prior (not in the reference): the same under another name, a 3 x 3 F
    for pixel coordinates the search STARTS from, see _baseline_model_records."""
    if initial_F is not None:
        # unlike ransac_*relpose, which reset the model they are handed (an initial pose only sets score_initial_model), the reference's
        # ransac_fundamental scores the caller's F itself, converted into its normalised coordinates, once the binding has set score_initial_model:
        # the state a prior in the caller's units leaves (mdrp_estimate_classic_prior, prior_space = 0; DESIGN.md 9, pinned in
        # tests/golden/classic_initial_F_ref.npz from the binary)
        if prior is not None:
            raise ValueError("initial_F and prior both start the search from a matrix: pass one of them")
        prior = np.asarray(initial_F, dtype=np.float64)
    Fs, infos = estimate_fundamental_batch([_as_points(points2D_1)], [_as_points(points2D_2)], ransac_opt, bundle_opt, scores=_one_scores(scores),
                                           priors=None if prior is None else [prior])
    return Fs[0], infos[0]


def _bearings(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] != 3:
        raise ValueError("bearings must have shape (K, 3)")
    return x


def relpose_5pt(x1, x2):
    """_core.pyi:851-854: five unit bearings per view -> list[CameraPose] in the reference's order"""
    out, n = _capi.default_handle(0).classic_solver_batch(_capi.RELPOSE_5PT, _bearings(x1)[None], _bearings(x2)[None])
    return [CameraPose(m["q"].copy(), m["t"].copy()) for m in out[0][:n[0]]]


def relpose_7pt(x1, x2):
    """seven unit bearings per view -> list of 3 x 3 fundamental matrices (unit Frobenius norm) in the reference's order"""
    out, n = _capi.default_handle(0).classic_solver_batch(_capi.FUNDAMENTAL_7PT, _bearings(x1)[None], _bearings(x2)[None])
    return [_capi.model_to_fundamental(m) for m in out[0][:n[0]]]


class ImagePair:
    """(_core.pyi:164-169): pose and the two cameras of the 6-point shared-focal estimator"""

    def __init__(self, pose=None, camera1=None, camera2=None):
        self.pose = pose if pose is not None else CameraPose()
        self.camera1 = camera1 if camera1 is not None else Camera()
        self.camera2 = camera2 if camera2 is not None else Camera()

    def __repr__(self):
        return f"ImagePair(pose={self.pose!r}, f1={self.camera1.focal():.6g}, f2={self.camera2.focal():.6g})"


def _pp_records(pp, B):
    """principal point(s) as the camera records the C ABI carries them in (MDRP_SHARED_6PT: cam1[i].params[0..1])"""
    pp = np.zeros(2) if pp is None else np.asarray(pp, dtype=np.float64)
    pp = np.broadcast_to(pp.reshape(-1, 2) if pp.size != 2 else pp.reshape(1, 2), (B, 2))
    rec = np.zeros(B, dtype=_capi.CAMERA_DTYPE)
    rec["params"][:, 0] = pp[:, 0]; rec["params"][:, 1] = pp[:, 1]
    return rec, pp


def estimate_shared_focal_relative_pose_batch(points2D_1, points2D_2, pp=None, ransac_opt=None, bundle_opt=None, device=0, budgets=None, scores=None,
                                              priors=None):
    """B pairs through the 6-point shared-focal estimator.  pp: one principal point for all pairs or (B, 2).
    Returns (list[ImagePair], list[info dict]).  budgets: see _budget_args; scores: see PRESORTED (not with budgets); priors: see
    _baseline_model_records (not with budgets or scores)."""
    _no_scores_with(scores, budgets, priors)
    _no_budgets_with_priors(priors, budgets)
    ransac_opt, budgets = _budget_args(ransac_opt, budgets)
    _check_baseline_options(ransac_opt, scores)
    x1, x2, ns = _stack2(points2D_1, points2D_2)
    B = len(ns)
    rec, ppb = _pp_records(pp, B)
    res, mask = _baseline_host(_capi.SHARED_6PT, x1, x2, ns, scores, rec, rec, ransac_opt, bundle_opt, device, budgets, priors)

    def build(res, mask):
        out = []
        for i, r in enumerate(res):
            f = float(r["model"]["f1"])
            cam = Camera("SIMPLE_PINHOLE", [f, float(ppb[i, 0]), float(ppb[i, 1])])
            out.append(ImagePair(CameraPose(r["model"]["q"].copy(), r["model"]["t"].copy()), cam, Camera("SIMPLE_PINHOLE", [f, float(ppb[i, 0]), float(ppb[i, 1])])))
        return out, [_info(res[i], mask[i], ns[i]) for i in range(B)]
    return _per_budget(budgets, res, mask, build)


def estimate_shared_focal_relative_pose(points2D_1, points2D_2, pp=None, ransac_opt={}, bundle_opt={}, initial_image_pair=None, scores=None, prior=None):
    """Relative pose with one unknown focal length shared by both images, 6-point solver + non-linear refinement
    (_core.pyi:531-543; /root/reference/eval_shared_f.py:161, where the fork's signature has no `pp` and the points are
    already centred: a dict in the third position is taken as ransac_opt).  An initial image pair only sets
    score_initial_model, like the initial pose of the other estimators.  scores (not in the reference): see PRESORTED.  prior (not in the reference):
    an ImagePair the search STARTS from, see _baseline_model_records."""
    if isinstance(pp, dict):  # fork call shape: (kp1, kp2, ransac_dict, bundle_dict)
        pp, ransac_opt, bundle_opt = None, pp, (ransac_opt if ransac_opt else bundle_opt)
    pairs, infos = estimate_shared_focal_relative_pose_batch([_as_points(points2D_1)], [_as_points(points2D_2)], pp,
                                                             _with_initial(initial_image_pair, ransac_opt), bundle_opt, scores=_one_scores(scores),
                                                             priors=None if prior is None else [prior])
    return pairs[0], infos[0]


def relpose_6pt_shared_focal(x1, x2):
    """six homogeneous image points per view -> list[ImagePair], by ascending focal length (the reference's order is the
    order of its eigenvalue solver and is not reproduced)"""
    out, n = _capi.default_handle(0).classic_solver_batch(_capi.SHARED_6PT, _bearings(x1)[None], _bearings(x2)[None])
    return [ImagePair(CameraPose(m["q"].copy(), m["t"].copy()), Camera("SIMPLE_PINHOLE", [float(m["f1"]), 0.0, 0.0]),
                      Camera("SIMPLE_PINHOLE", [float(m["f2"]), 0.0, 0.0])) for m in out[0][:n[0]]]


# ------------------------------------------------------------------------------------------------ the varying-focal baseline (`7p`)
# The 7-point fundamental matrix, then focals and a pose from it (include/mdrp_classic_focals.h): what the reference's varying-focal
# tables compare the monodepth estimator with (/root/reference/eval_varying_f.py:134).
def _focal_pp(pp, B, what):
    """None, one principal point or one per pair -> (B, 2) float64, or None for the origin"""
    if pp is None:
        return None
    a = np.asarray(pp, dtype=np.float64)
    if a.size == 2:
        a = a.reshape(1, 2)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] not in (1, B) or not np.isfinite(a).all():
        raise ValueError(f"{what}: a finite principal point (2,) or one per pair ({B}, 2)")
    return np.broadcast_to(a, (B, 2)).copy()


def _focal_matrices(F):
    a = np.asarray(F)
    if a.dtype.kind not in "fiu" or a.ndim != 3 or a.shape[1:] != (3, 3):
        raise ValueError("F: fundamental matrices (B, 3, 3)")
    return np.ascontiguousarray(a, dtype=np.float64)


def focals_from_fundamental_batch(F, pp1=None, pp2=None, device=0):
    """B fundamental matrices (B, 3, 3) for pixel coordinates and the principal points of the two images (one for all pairs, (B, 2), or None: the
    origin) -> (list[Camera], list[Camera]) as focals_from_fundamental returns them."""
    F = _focal_matrices(F)
    B = len(F)
    a, b = _focal_pp(pp1, B, "pp1"), _focal_pp(pp2, B, "pp2")  # (checked before anything touches the device)
    f = _capi.default_handle(device).focals_from_fundamental(F, a, b)
    za = np.zeros((B, 2)) if a is None else a
    zb = np.zeros((B, 2)) if b is None else b
    return ([Camera("SIMPLE_PINHOLE", [float(f[i, 0]), float(za[i, 0]), float(za[i, 1])]) for i in range(B)],
            [Camera("SIMPLE_PINHOLE", [float(f[i, 1]), float(zb[i, 0]), float(zb[i, 1])]) for i in range(B)])


def focals_from_fundamental(F, pp1, pp2):
    """(_core.pyi: focals_from_fundamental(F, pp1, pp2) -> tuple[Camera, Camera]): the focal lengths of two cameras with known principal points from
    their fundamental matrix, closed form.  Two SIMPLE_PINHOLE cameras [f, ppx, ppy] with width = height = -1, as the wheel returns them; a focal
    whose square comes out negative is NaN."""
    a = np.asarray(F)
    if a.shape != (3, 3):
        raise ValueError("F: a 3 x 3 fundamental matrix")
    for name, pp in (("pp1", pp1), ("pp2", pp2)):
        if pp is None or np.asarray(pp).size != 2:
            raise ValueError(f"{name}: a principal point (2,)")
    c1, c2 = focals_from_fundamental_batch(a[None], np.asarray(pp1, dtype=np.float64).reshape(2), np.asarray(pp2, dtype=np.float64).reshape(2))
    return c1[0], c2[0]


def _focal_pose_pairs(rec, ppa, ppb):
    out = []
    for i, r in enumerate(rec):
        m = r["model"]
        out.append(ImagePair(CameraPose(m["q"].copy(), m["t"].copy()), Camera("SIMPLE_PINHOLE", [float(m["f1"]), float(ppa[i, 0]), float(ppa[i, 1])]),
                             Camera("SIMPLE_PINHOLE", [float(m["f2"]), float(ppb[i, 0]), float(ppb[i, 1])])))
    return out


def estimate_varying_focal_relative_pose_batch(points2D_1, points2D_2, pp1=None, pp2=None, ransac_opt=None, bundle_opt=None, device=0, scores=None,
                                               priors=None):
    """B pairs through the varying-focal baseline: the 7-point estimator (estimate_fundamental_batch, with its scores / priors), then the focals of
    the two cameras from its F and the pose the inliers vote for (include/mdrp_classic_focals.h).  pp1 / pp2: the principal point of each image in the
    points' coordinates, one for all pairs or (B, 2); None is the origin (centred points).  Returns (list[ImagePair], list[info dict]): the 7-point
    info plus "F" (3 x 3), "votes" (4 ints), "winner" and "status" (0: a pose chosen by the inliers; _capi.FOCAL_* bits otherwise — a focal that is
    not real is NaN and the pose is the identity)."""
    _no_scores_with(scores, None, priors)
    _check_baseline_options(ransac_opt, scores)
    x1, x2, ns = _stack2(points2D_1, points2D_2)
    B = len(ns)
    a, b = _focal_pp(pp1, B, "pp1"), _focal_pp(pp2, B, "pp2")  # (checked before anything touches the device)
    res, mask = _baseline_host(_capi.FUNDAMENTAL_7PT, x1, x2, ns, scores, None, None, ransac_opt, bundle_opt, device, None, priors)
    rec = _capi.default_handle(device).pose_from_fundamental(x1, x2, res, ns, mask, a, b)
    infos = []
    for i in range(B):
        info = _info(res[i], mask[i], ns[i])
        info.update(F=_capi.model_to_fundamental(res[i]["model"]), votes=[int(v) for v in rec[i]["votes"]], winner=int(rec[i]["winner"]),
                    status=int(rec[i]["status"]))
        infos.append(info)
    return _focal_pose_pairs(rec, np.zeros((B, 2)) if a is None else a, np.zeros((B, 2)) if b is None else b), infos


def estimate_varying_focal_relative_pose(points2D_1, points2D_2, pp1=None, pp2=None, ransac_opt={}, bundle_opt={}, scores=None, prior=None):
    """estimate_varying_focal_relative_pose_batch for one pair.  Returns (ImagePair, info)."""
    pairs, infos = estimate_varying_focal_relative_pose_batch([_as_points(points2D_1)], [_as_points(points2D_2)], pp1, pp2, ransac_opt, bundle_opt,
                                                              scores=_one_scores(scores), priors=None if prior is None else [prior])
    return pairs[0], infos[0]


# names the reference scripts also reach for: present so that a swapped import fails with a clear message at the call
estimate_relative_pose_w_relative_depth = _not_on_path("estimate_relative_pose_w_relative_depth", "fork-only variant, eval.py:140 (commented out upstream)")


# ------------------------------------------------------------------------------------------------ device-resident batches
_TORCH_HANDLE_CACHE = 4  # handles kept per thread (each owns its scratch buffers); least recently used is closed
_torch_tls = None


def _torch_handle(dev, stream_ptr):
    """the calling thread's handle bound to (device, stream), LRU-bounded; stream_ptr 0 = the legacy default stream"""
    global _torch_tls
    import collections
    import threading
    if _torch_tls is None:
        _torch_tls = threading.local()
    cache = getattr(_torch_tls, "cache", None)
    if cache is None:
        cache = _torch_tls.cache = collections.OrderedDict()
    key = (dev, stream_ptr)
    h = cache.pop(key, None)
    if h is None:
        h = _capi.Handle(dev, stream_ptr)
        while len(cache) >= _TORCH_HANDLE_CACHE:
            cache.popitem(last=False)[1].close()
    cache[key] = h
    return h


def _handle_on(dev):
    """the calling thread's handle on the current torch stream of the torch device `dev`"""
    import torch
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    return _torch_handle(index, int(torch.cuda.current_stream(dev).cuda_stream))


MONODEPTH_KINDS = {"calibrated": _capi.CALIB, "shared_focal": _capi.SHARED_FOCAL, "varying_focal": _capi.VARYING_FOCAL}


def _monodepth_kind(kind):
    """the kind of an entry point that reads depth maps: a name of MONODEPTH_KINDS or its id"""
    if isinstance(kind, str) and kind not in MONODEPTH_KINDS:
        raise ValueError(f"kind must be one of {tuple(MONODEPTH_KINDS)}, not {kind!r}")
    k = MONODEPTH_KINDS[kind] if isinstance(kind, str) else int(kind)
    if k not in MONODEPTH_KINDS.values():
        raise ValueError("only the monodepth estimators (calibrated, shared_focal, varying_focal) take depth maps")
    return k


def _check_resident_scores(scores, shape):
    """a score tensor of a resident batch, checked before anything touches the device: float32 / float64, one score per correspondence"""
    import torch
    if not (isinstance(scores, torch.Tensor) and scores.dtype in (torch.float32, torch.float64)):
        raise ValueError('scores must be a float32 / float64 tensor on the inputs\' device or "presorted"')
    if tuple(scores.shape) != tuple(shape):
        raise ValueError(f"scores must be {tuple(shape)}, one per correspondence, not {tuple(scores.shape)}")


def _resident_scores(scores, device):
    """the checked scores as the ranked entry points read them: None for "presorted", else a contiguous float64 tensor the caller keeps alive"""
    import torch
    if isinstance(scores, str):
        return None
    if not (scores.is_cuda and scores.device == device):
        raise ValueError("scores must live on the inputs' device")
    return scores.to(torch.float64).contiguous()  # (float32 -> float64 is exact: the order is the caller's)


def estimate_batch_torch(kind, points2D_1, points2D_2, depth_1, depth_2, cameras1=None, cameras2=None, ransac_opt=None,
                         bundle_opt=None, n_per_pair=None, budgets=None, priors=None, scores=None):
    """Batch that already lives on the GPU (e.g. matcher output): `points2D_*` (B, N, 2) and `depth_*` (B, N) float64 torch
    tensors on a ROCm device; the work is queued on that device's CURRENT torch stream — including torch's default
    (null) stream — so it is ordered after whatever produced the inputs there and before later consumers of the mask;
    nothing crosses PCIe except the 136-byte result records.  kind: "calibrated" | "shared_focal" | "varying_focal".
    Returns (records: numpy structured array with `model`, `refinements`, `iterations`, `num_inliers`, `inlier_ratio`,
    `model_score`; inlier mask: (B, N) uint8 tensor on the device).  Ragged batches: pad and pass `n_per_pair`
    (sequence, numpy array or tensor on any device).  budgets (see _budget_args): records (C, B) and a (C, B, N) mask tensor.
    priors (see _prior_records; not with budgets): one model per pair the search starts from — a device tensor holding B records of 96 bytes
    (uint8 (B, 96), or float64 (B, 12): q t scale shift1 shift2 f1 f2, a NaN q[0] for a pair without one), or a numpy array of _capi.MODEL_DTYPE,
    which is uploaded on the stream.  scores (see PRESORTED; not with budgets or priors): a (B, N) float32 / float64 tensor on the inputs' device, one
    score per correspondence, higher is better, or "presorted": the estimate in score order with the progressive sampler; the mask stays in the
    caller's order."""
    _no_scores_with(scores, budgets, priors)
    _no_budgets_with_priors(priors, budgets)
    ransac_opt, budgets = _budget_args(ransac_opt, budgets)
    import torch
    if priors is not None:  # (checked before anything touches the device)
        if isinstance(priors, np.ndarray):
            priors = _prior_records(priors, None, int(depth_1.shape[0]))
        elif not (isinstance(priors, torch.Tensor) and priors.dtype in (torch.uint8, torch.float64)):
            raise ValueError("priors must be a uint8 / float64 tensor on the inputs' device or a numpy array of _capi.MODEL_DTYPE")
        elif priors.numel() * priors.element_size() != int(depth_1.shape[0]) * _capi.MODEL_DTYPE.itemsize:
            raise ValueError(f"priors must hold {int(depth_1.shape[0])} records of {_capi.MODEL_DTYPE.itemsize} bytes")
    if scores is not None and not (isinstance(scores, str) and scores == PRESORTED):  # (checked before anything touches the device)
        _check_resident_scores(scores, depth_1.shape)
    k = MONODEPTH_KINDS[kind] if isinstance(kind, str) else int(kind)
    x1, x2, d1, d2 = (t.contiguous() for t in (points2D_1, points2D_2, depth_1, depth_2))
    for t in (x1, x2, d1, d2):
        if not (t.is_cuda and t.dtype == torch.float64):
            raise ValueError("estimate_batch_torch needs float64 tensors on the GPU")
        if t.device != x1.device:
            raise ValueError("all tensors must live on the same device")
    B, N = d1.shape
    if x1.shape != (B, N, 2) or x2.shape != (B, N, 2) or d2.shape != (B, N):
        raise ValueError("shapes must be (B, N, 2), (B, N, 2), (B, N), (B, N)")
    h = _handle_on(x1.device)
    if n_per_pair is not None and isinstance(n_per_pair, torch.Tensor):
        n_per_pair = n_per_pair.detach().cpu().numpy()
    cams1 = cams2 = None
    if k == _capi.CALIB:
        cams1, cams2 = _camera_records(cameras1, B), _camera_records(cameras2, B)
    with torch.cuda.device(x1.device):
        if budgets is not None:
            mask = torch.zeros((len(budgets), B, N), dtype=torch.uint8, device=x1.device)
            h.estimate_batch_budgets_device(k, x1.data_ptr(), x2.data_ptr(), d1.data_ptr(), d2.data_ptr(), B, N,
                                            _capi.ransac_opt_from_dict(ransac_opt), _capi.bundle_opt_from_dict(bundle_opt), budgets, n_per_pair, cams1, cams2,
                                            mask.data_ptr())
            return h.fetch_budget_results(len(budgets), B), mask
        mask = torch.zeros((B, N), dtype=torch.uint8, device=x1.device)
        if scores is not None:
            sc = _resident_scores(scores, x1.device)
            h.estimate_batch_ranked_device(k, x1.data_ptr(), x2.data_ptr(), d1.data_ptr(), d2.data_ptr(), None if sc is None else sc.data_ptr(), B, N,
                                           _capi.ransac_opt_from_dict(ransac_opt), _capi.bundle_opt_from_dict(bundle_opt), n_per_pair, cams1, cams2,
                                           mask.data_ptr())
        elif priors is not None:
            if isinstance(priors, np.ndarray):
                priors = torch.from_numpy(priors.view(np.uint8).copy()).to(x1.device)
            if not (priors.is_cuda and priors.device == x1.device):
                raise ValueError("priors must live on the inputs' device")
            priors = priors.contiguous()
            h.estimate_batch_prior_device(k, x1.data_ptr(), x2.data_ptr(), d1.data_ptr(), d2.data_ptr(), B, N, priors.data_ptr(),
                                          _capi.ransac_opt_from_dict(ransac_opt), _capi.bundle_opt_from_dict(bundle_opt), n_per_pair, cams1, cams2,
                                          mask.data_ptr())
        else:
            h.estimate_batch_device(k, x1.data_ptr(), x2.data_ptr(), d1.data_ptr(), d2.data_ptr(), B, N,
                                    _capi.ransac_opt_from_dict(ransac_opt), _capi.bundle_opt_from_dict(bundle_opt), n_per_pair, cams1, cams2,
                                    mask.data_ptr())
        res = h.fetch_results(B)
    return res, mask


BASELINE_KINDS = {"relpose_5pt": _capi.RELPOSE_5PT, "shared_focal_6pt": _capi.SHARED_6PT, "fundamental_7pt": _capi.FUNDAMENTAL_7PT}


def _baseline_kind(kind):
    if not (isinstance(kind, str) and kind in BASELINE_KINDS):
        raise ValueError(f"kind: one of {sorted(BASELINE_KINDS)}, not {kind!r}")
    return BASELINE_KINDS[kind]


def _model_tensor(models, B, device, what):
    """one model record per pair on `device`: a uint8 (B, 96) / float64 (B, 12) tensor there, or a numpy array of _capi.MODEL_DTYPE (uploaded on the
    current stream)"""
    import torch
    if isinstance(models, np.ndarray):
        if models.dtype != _capi.MODEL_DTYPE:
            raise ValueError(f"{what}: a numpy array must have dtype _capi.MODEL_DTYPE")
        models = torch.from_numpy(np.ascontiguousarray(models).reshape(-1).view(np.uint8).copy()).to(device)
    if not (isinstance(models, torch.Tensor) and models.is_cuda and models.device == device and models.dtype in (torch.uint8, torch.float64)):
        raise ValueError(f"{what} must be a uint8 / float64 tensor on the inputs' device or a numpy array of _capi.MODEL_DTYPE")
    models = models.contiguous()
    if models.numel() * models.element_size() != B * _capi.MODEL_DTYPE.itemsize:
        raise ValueError(f"{what} must hold {B} records of {_capi.MODEL_DTYPE.itemsize} bytes")
    return models


def _baseline_points_shape(who, points2D_1, points2D_2):
    """(B, N) of two (B, N, 2) tensors"""
    import torch
    if not (isinstance(points2D_1, torch.Tensor) and isinstance(points2D_2, torch.Tensor)):
        raise ValueError(f"{who} needs float64 tensors on the GPU")
    if points2D_1.ndim != 3 or points2D_1.shape[2] != 2 or points2D_2.shape != points2D_1.shape:
        raise ValueError("shapes must be (B, N, 2), (B, N, 2)")
    return int(points2D_1.shape[0]), int(points2D_1.shape[1])


def _baseline_torch_args(who, kind, points2D_1, points2D_2, cameras1, cameras2, pp, n_per_pair):
    """what the baselines' resident entry points check before anything touches the device: (kind id, x1, x2, B, N, n_per_pair, cams1, cams2)"""
    import torch
    k = _baseline_kind(kind)
    B, N = _baseline_points_shape(who, points2D_1, points2D_2)
    x1, x2 = points2D_1.contiguous(), points2D_2.contiguous()
    for t in (x1, x2):
        if not (t.is_cuda and t.dtype == torch.float64):
            raise ValueError(f"{who} needs float64 tensors on the GPU")
        if t.device != x1.device:
            raise ValueError("all tensors must live on the same device")
    if n_per_pair is not None and isinstance(n_per_pair, torch.Tensor):
        n_per_pair = n_per_pair.detach().cpu().numpy()
    cams1 = cams2 = None
    if k == _capi.RELPOSE_5PT:
        cams1, cams2 = _camera_records(cameras1, B), _camera_records(cameras2, B)
    elif k == _capi.SHARED_6PT:
        cams1 = cams2 = _pp_records(pp, B)[0]
    return k, x1, x2, B, N, n_per_pair, cams1, cams2


def refine_baseline_batch_torch(kind, points2D_1, points2D_2, models, cameras1=None, cameras2=None, pp=None, ransac_opt=None, bundle_opt=None,
                                n_per_pair=None, stages=("lo", "inliers")):
    """refine_batch_torch for the comparison rows (include/mdrp_classic_models.h: mdrp_refine_classic): one model per pair goes in and the baseline's
    own tail runs on it without a sample.  kind, points, cameras and pp as in estimate_baseline_batch_torch; models as in refine_batch_torch, in the
    caller's units (5-point: q, t; 6-point: q, t and f1 = f2 in pixels; 7-point: F for pixel coordinates in the first nine doubles; a NaN first double:
    no model).  Of ransac_opt only max_epipolar_error is read.  Returns (records, (B, N) uint8 mask tensor on the device, initial: {"score",
    "inliers"} numpy arrays of the models handed in)."""
    import torch
    k, x1, x2, B, N, n_per_pair, cams1, cams2 = _baseline_torch_args("refine_baseline_batch_torch", kind, points2D_1, points2D_2, cameras1, cameras2, pp,
                                                                     n_per_pair)
    flags = _stage_flags(stages)
    with torch.cuda.device(x1.device):
        h = _handle_on(x1.device)
        models = _model_tensor(models, B, x1.device, "models")
        mask = torch.zeros((B, N), dtype=torch.uint8, device=x1.device)
        score0 = torch.zeros(B, dtype=torch.float64, device=x1.device)
        inl0 = torch.zeros(B, dtype=torch.int32, device=x1.device)
        h.refine_classic_device(k, x1.data_ptr(), x2.data_ptr(), B, N, models.data_ptr(), _capi.ransac_opt_from_dict(ransac_opt),
                                _capi.bundle_opt_from_dict(bundle_opt), flags, n_per_pair, cams1, cams2, mask.data_ptr(), score0.data_ptr(), inl0.data_ptr())
        res = h.fetch_results(B)  # (waits for the stream: the two small tensors below are complete)
        initial = {"score": score0.cpu().numpy(), "inliers": inl0.cpu().numpy()}
    return res, mask, initial


# The names refine_relative_pose / refine_fundamental are NOT defined here: upstream gives them another meaning (a plain LM over all the points
# handed in, no threshold, no LO, no mask), and a function of that name with the estimator's tail would not be a drop-in.
def refine_baseline_batch(kind, points2D_1, points2D_2, models, cameras1=None, cameras2=None, pp=None, ransac_opt=None, bundle_opt=None, device=0,
                          stages=("lo", "inliers"), as_arrays=False):
    """B pairs, each with a model to start from, through the baseline's tail (refine_monodepth_*_batch for the comparison rows).  kind: see
    BASELINE_KINDS; models: list[CameraPose] (5-point), list[ImagePair] (6-point) or 3 x 3 arrays (7-point), or a MODEL_DTYPE array.  Returns
    (list of the same type, list[info dict] as _refine_info builds them); as_arrays=True: (records, masks, n_per_pair, initial scores, initial
    inlier counts)."""
    k = _baseline_kind(kind)
    flags = _stage_flags(stages)  # (everything is checked before anything touches the device)
    x1, x2, ns = _stack2(points2D_1, points2D_2)
    B = len(ns)
    rec = _baseline_model_records(models, k, B, "models")
    if np.isnan(rec["q"][:, 0]).any() and not (isinstance(models, np.ndarray) and models.dtype == _capi.MODEL_DTYPE):
        raise ValueError("models: every pair needs a model to start from (None is for priors)")
    cams1 = cams2 = None
    ppb = None
    if k == _capi.RELPOSE_5PT:
        cams1, cams2 = _camera_records(cameras1, B), _camera_records(cameras2, B)
    elif k == _capi.SHARED_6PT:
        cams1, ppb = _pp_records(pp, B)
        cams2 = cams1
    res, mask, score0, inl0 = _capi.default_handle(device).refine_classic(k, x1, x2, rec, _capi.ransac_opt_from_dict(ransac_opt),
                                                                          _capi.bundle_opt_from_dict(bundle_opt), flags, ns, cams1, cams2)
    if as_arrays:
        return res, mask, ns, score0, inl0
    if k == _capi.RELPOSE_5PT:
        out = [CameraPose(r["model"]["q"].copy(), r["model"]["t"].copy()) for r in res]
    elif k == _capi.FUNDAMENTAL_7PT:
        out = [_capi.model_to_fundamental(r["model"]) for r in res]
    else:
        out = []
        for i, r in enumerate(res):
            f = float(r["model"]["f1"])
            out.append(ImagePair(CameraPose(r["model"]["q"].copy(), r["model"]["t"].copy()), Camera("SIMPLE_PINHOLE", [f, float(ppb[i, 0]), float(ppb[i, 1])]),
                                 Camera("SIMPLE_PINHOLE", [f, float(ppb[i, 0]), float(ppb[i, 1])])))
    return out, [_refine_info(res[i], mask[i], ns[i], score0[i], inl0[i]) for i in range(B)]


def refine_baseline(kind, points2D_1, points2D_2, model, camera1=None, camera2=None, pp=None, ransac_opt={}, bundle_opt={}, stages=("lo", "inliers")):
    """refine_baseline_batch for one pair.  Returns (model, info)."""
    if model is None:
        raise ValueError("model is required: there is nothing to refine without a model to start from")
    m, i = refine_baseline_batch(kind, [_as_points(points2D_1)], [_as_points(points2D_2)], [model], camera1, camera2, pp, ransac_opt, bundle_opt, stages=stages)
    return m[0], i[0]


def estimate_baseline_batch_torch(kind, points2D_1, points2D_2, cameras1=None, cameras2=None, pp=None, ransac_opt=None, bundle_opt=None, n_per_pair=None,
                                  scores=None, priors=None, prior_space=0):
    """estimate_batch_torch for the comparison rows, which have no depths: `points2D_*` (B, N, 2) float64 torch tensors on a ROCm device, queued on
    that device's current torch stream.  kind: "relpose_5pt" (cameras1 / cameras2) | "shared_focal_6pt" (pp: one principal point or (B, 2); None is
    (0, 0)) | "fundamental_7pt".  Returns (records, (B, N) uint8 mask tensor on the device) as estimate_batch_torch does.  scores (see PRESORTED): a
    (B, N) float32 / float64 tensor on the inputs' device, one per correspondence, higher is better, or "presorted": the estimate in score order with
    the progressive sampler of the estimator's sample size; the mask stays in the caller's order.  Without scores it is the plain estimator.
    priors (not with scores): one model per pair as in refine_baseline_batch_torch, a NaN first double meaning none — the search of each pair starts
    from it (include/mdrp_classic_models.h: mdrp_estimate_classic_prior); prior_space 1: the records are in the estimator's normalised coordinates."""
    import torch
    k = _baseline_kind(kind)
    _no_scores_with(scores, None, priors)
    _check_baseline_options(ransac_opt, scores)
    # (everything down to the handle is checked before anything touches the device)
    B, N = _baseline_points_shape("estimate_baseline_batch_torch", points2D_1, points2D_2)
    if isinstance(scores, str):
        if scores != PRESORTED:
            raise ValueError(f'scores: the only string is "{PRESORTED}", not {scores!r}')
    elif scores is not None:
        _check_resident_scores(scores, (B, N))
    k, x1, x2, B, N, n_per_pair, cams1, cams2 = _baseline_torch_args("estimate_baseline_batch_torch", kind, points2D_1, points2D_2, cameras1, cameras2, pp,
                                                                     n_per_pair)
    h = _handle_on(x1.device)
    ro, bo = _capi.ransac_opt_from_dict(ransac_opt), _capi.bundle_opt_from_dict(bundle_opt)
    with torch.cuda.device(x1.device):
        mask = torch.zeros((B, N), dtype=torch.uint8, device=x1.device)
        if priors is not None:
            pr = _model_tensor(priors, B, x1.device, "priors")
            h.estimate_classic_prior_device(k, x1.data_ptr(), x2.data_ptr(), B, N, pr.data_ptr(), ro, bo, n_per_pair, cams1, cams2, mask.data_ptr(),
                                            prior_space=prior_space)
        elif scores is None:
            h.estimate_batch_device(k, x1.data_ptr(), x2.data_ptr(), None, None, B, N, ro, bo, n_per_pair, cams1, cams2, mask.data_ptr())
        else:
            sc = _resident_scores(scores, x1.device)
            h.estimate_classic_ranked_device(k, x1.data_ptr(), x2.data_ptr(), None if sc is None else sc.data_ptr(), B, N, ro, bo, n_per_pair, cams1, cams2,
                                             mask.data_ptr())
        res = h.fetch_results(B)
    return res, mask


def _focal_pp_tensor(pp, B, device, what):
    """a principal point for pose_from_fundamental_batch_torch: None (the origin), a float64 (B, 2) tensor on `device`, or what _focal_pp takes (uploaded)"""
    import torch
    if pp is None:
        return None
    if isinstance(pp, torch.Tensor):
        if not (pp.is_cuda and pp.device == device and pp.dtype == torch.float64 and tuple(pp.shape) == (B, 2)):
            raise ValueError(f"{what}: a float64 ({B}, 2) tensor on the inputs' device")
        return pp.contiguous()
    return torch.from_numpy(_focal_pp(pp, B, what)).to(device)


def pose_from_fundamental_batch_torch(points2D_1, points2D_2, models, n_per_pair=None, inlier_mask=None, pp1=None, pp2=None):
    """Focals and pose from a fundamental matrix per pair, on tensors that already live on the GPU (include/mdrp_classic_focals.h:
    mdrp_pose_from_fundamental_async) — the tail to put behind any 7-point call (estimate_baseline_batch_torch("fundamental_7pt", ...) with or without
    scores or priors, refine_baseline_batch_torch).  points2D_*: (B, N, 2) float64; models: B records holding F row-major in their first nine doubles —
    a uint8 (B, 96) / float64 (B, 12) tensor of model records, a uint8 (B, 136) / float64 (B, 17) tensor of result records, or a numpy array of
    _capi.MODEL_DTYPE / _capi.RESULT_DTYPE (uploaded on the current stream); inlier_mask: (B, N) uint8 tensor or None (every record votes);
    pp1 / pp2: see _focal_pp_tensor.  Queued on the device's current torch stream.  Returns B records of _capi.FOCAL_POSE_DTYPE (numpy)."""
    import torch
    B, N = _baseline_points_shape("pose_from_fundamental_batch_torch", points2D_1, points2D_2)
    x1, x2 = points2D_1.contiguous(), points2D_2.contiguous()
    for t in (x1, x2):
        if not (t.is_cuda and t.dtype == torch.float64 and t.device == x1.device):
            raise ValueError("pose_from_fundamental_batch_torch needs float64 tensors on one GPU")
    if isinstance(models, np.ndarray):
        if models.dtype not in (_capi.MODEL_DTYPE, _capi.RESULT_DTYPE):
            raise ValueError("models: a numpy array must have dtype _capi.MODEL_DTYPE or _capi.RESULT_DTYPE")
        models = torch.from_numpy(np.ascontiguousarray(models).reshape(-1).view(np.uint8).copy())
        upload = True
    else:
        upload = False
    if not (isinstance(models, torch.Tensor) and models.dtype in (torch.uint8, torch.float64)) or (not upload and not (models.is_cuda and models.device == x1.device)):
        raise ValueError("models must be a uint8 / float64 tensor on the inputs' device or a numpy array of _capi.MODEL_DTYPE / _capi.RESULT_DTYPE")
    nbytes = models.numel() * models.element_size()
    if B > 0 and (nbytes % B != 0 or nbytes // B not in (_capi.MODEL_DTYPE.itemsize, _capi.RESULT_DTYPE.itemsize)):
        raise ValueError(f"models must hold {B} records of {_capi.MODEL_DTYPE.itemsize} or {_capi.RESULT_DTYPE.itemsize} bytes")
    stride = nbytes // B if B > 0 else _capi.MODEL_DTYPE.itemsize
    if inlier_mask is not None and not (isinstance(inlier_mask, torch.Tensor) and inlier_mask.is_cuda and inlier_mask.device == x1.device
                                        and inlier_mask.dtype == torch.uint8 and tuple(inlier_mask.shape) == (B, N)):
        raise ValueError(f"inlier_mask: a uint8 ({B}, {N}) tensor on the inputs' device")
    if n_per_pair is not None and isinstance(n_per_pair, torch.Tensor):
        n_per_pair = n_per_pair.detach().cpu().numpy()
    with torch.cuda.device(x1.device):
        h = _handle_on(x1.device)
        a, b = _focal_pp_tensor(pp1, B, x1.device, "pp1"), _focal_pp_tensor(pp2, B, x1.device, "pp2")
        models = models.to(x1.device).contiguous()
        mk = None if inlier_mask is None else inlier_mask.contiguous()
        out = torch.zeros((B, _capi.FOCAL_POSE_DTYPE.itemsize), dtype=torch.uint8, device=x1.device)
        h.pose_from_fundamental_device(x1.data_ptr(), x2.data_ptr(), B, N, models.data_ptr(), stride, out.data_ptr(), n_per_pair,
                                       None if mk is None else mk.data_ptr(), None if a is None else a.data_ptr(), None if b is None else b.data_ptr())
        rec = out.cpu().numpy().reshape(-1).view(_capi.FOCAL_POSE_DTYPE).copy()  # (waits for the stream the kernel was queued on)
    return rec


def estimate_varying_focal_baseline_batch_torch(points2D_1, points2D_2, pp1=None, pp2=None, ransac_opt=None, bundle_opt=None, n_per_pair=None):
    """The varying-focal baseline on tensors that already live on the GPU, in ONE call of the library (mdrp_estimate_fundamental_focals_async): the
    7-point estimate of estimate_baseline_batch_torch("fundamental_7pt", ...) with pose_from_fundamental_batch_torch queued behind it on its result
    records and its mask, which never leave the device.  Returns (B records of _capi.FOCAL_POSE_DTYPE, the 7-point records, (B, N) uint8 mask tensor)."""
    import torch
    _check_baseline_options(ransac_opt, None)
    k, x1, x2, B, N, n_per_pair, _, _ = _baseline_torch_args("estimate_varying_focal_baseline_batch_torch", "fundamental_7pt", points2D_1, points2D_2,
                                                             None, None, None, n_per_pair)
    ro, bo = _capi.ransac_opt_from_dict(ransac_opt), _capi.bundle_opt_from_dict(bundle_opt)
    with torch.cuda.device(x1.device):
        h = _handle_on(x1.device)
        a, b = _focal_pp_tensor(pp1, B, x1.device, "pp1"), _focal_pp_tensor(pp2, B, x1.device, "pp2")
        mask = torch.zeros((B, N), dtype=torch.uint8, device=x1.device)
        out = torch.zeros((B, _capi.FOCAL_POSE_DTYPE.itemsize), dtype=torch.uint8, device=x1.device)
        h.estimate_fundamental_focals_device(x1.data_ptr(), x2.data_ptr(), B, N, ro, bo, out.data_ptr(), n_per_pair, mask.data_ptr(),
                                             None if a is None else a.data_ptr(), None if b is None else b.data_ptr())
        res = h.fetch_results(B)  # (waits for the stream: the tail's records are complete)
        rec = out.cpu().numpy().reshape(-1).view(_capi.FOCAL_POSE_DTYPE).copy()
    return rec, res, mask


# ------------------------------------------------------------------------------------------------ device front end
# What the reference's callers do in NumPy before the estimator (make_pair.py:96-106, make_video.py:265-275) — gather the matched
# keypoints, read their depths at the truncated pixel, drop the rows whose depths are both infinite — on the device, so that extractor,
# matcher and depth-network outputs go in as they are.  mdrp_amd/frontend.py states the semantics in NumPy (include/mdrp.h, ABI 0.6).
# The pieces the five descriptor builders below are made of.  Each builder calls them in its own order, which is the order its complaints come in: the
# builders with depth maps complain about placement first, the point builders about types and shapes first.
def _check_tensors(named):
    import torch
    for name, t in named.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor on the GPU")


def _check_on_gpu(named):
    """every named value is a torch tensor on the GPU, on the first one's device -> that device"""
    import torch
    for name, t in named.items():
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{name} must be a torch tensor on the GPU")
        if t.device != next(iter(named.values())).device:
            raise ValueError("all tensors must live on the same device")
    return next(iter(named.values())).device


def _float_types():
    import torch
    return {torch.float32: _capi.F32, torch.float64: _capi.F64}


def _check_float_pair(a, b, what):
    if a.dtype not in _float_types() or b.dtype != a.dtype:
        raise ValueError(f"{what} must both be float32 or both float64")


def _check_match_dtype(matches):
    import torch
    if matches.dtype not in (torch.int32, torch.int64):
        raise ValueError("matches must be int32 or int64")


def _check_keypoint_tables(kp1, kp2):
    if kp1.dim() != 3 or kp1.shape[2] != 2 or kp2.dim() != 3 or kp2.shape[2] != 2:
        raise ValueError("keypoints must have shape (B, K, 2) or (K, 2)")


def _check_match_rows(matches, B, whose, tables_agree=True):
    if not tables_agree or matches.dim() != 3 or matches.shape[0] != B or matches.shape[2] != 2:
        raise ValueError(f"matches must have shape (B, M, 2) with the {whose}' B")


def _narrow_matches(matches):
    import torch
    return matches.to(torch.int32) if matches.dtype == torch.int64 else matches  # narrowed on the device, on the current stream: no synchronisation


def _center(c, B, dev):
    """an optional principal point, (2,) or (B, 2) -> contiguous float64 (B, 2) tensor on `dev`"""
    import torch
    if c is None:
        return None
    c = torch.as_tensor(c, dtype=torch.float64).to(dev)
    if c.numel() == 2:
        c = c.reshape(1, 2).expand(B, 2)
    if c.shape != (B, 2):
        raise ValueError("centers must have shape (B, 2) or (2,)")
    return c.contiguous()


def _per_image(v, dtype, shape, what, dev):
    """an optional per-image table -> contiguous device tensor of that dtype and shape (uploaded on the current stream when it is on the host)"""
    import torch
    if v is None:
        return None
    v = (v if isinstance(v, torch.Tensor) else torch.tensor(np.asarray(v))).to(device=dev, dtype=dtype)
    if what == "centers" and v.numel() == 2:
        v = v.reshape(1, 2).expand(shape[0], 2)
    if tuple(v.shape) != shape:
        raise ValueError(f"{what} must have shape {shape}" + (" or (2,)" if what == "centers" else ""))
    return v.contiguous()


def _pairs_on_host(pairs, dev, need_host_pairs):
    """(pairs already lives on `dev`?, host pairs or None where they were not asked for and pairs is on the device: no copy back, B)"""
    import torch
    on_device = isinstance(pairs, torch.Tensor) and pairs.device == dev
    if on_device and (pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype.is_floating_point):
        raise ValueError("pairs must be (B, 2) integer image indices")
    host_pairs = _host_pairs(pairs) if need_host_pairs or not on_device else None
    return on_device, host_pairs, pairs.shape[0] if host_pairs is None else len(host_pairs)


def _pairs_on_device(pairs, on_device, host_pairs, dev):
    """the pair table as the descriptors carry it: int32 (B, 2) on `dev` (host_pairs is this call's own copy)"""
    import torch
    return pairs.clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous() if on_device else torch.from_numpy(host_pairs).to(dev)


def _data_ptr(t):
    return None if t is None else t.data_ptr()


def _matches_descriptor(keypoints1, keypoints2, matches, depth_map1, depth_map2, center1, center2, filter):
    """validated mdrp_matches descriptor of torch tensors on one ROCm device -> (descriptor, tensors it points into, B, M, device)"""
    if filter not in _capi.FILTERS:
        raise ValueError(f"filter must be one of {tuple(_capi.FILTERS)}, not {filter!r}")
    dev = _check_on_gpu({"keypoints1": keypoints1, "keypoints2": keypoints2, "matches": matches, "depth_map1": depth_map1, "depth_map2": depth_map2})
    kp1, kp2 = (t.unsqueeze(0) if t.dim() == 2 else t for t in (keypoints1, keypoints2))
    mt = matches.unsqueeze(0) if matches.dim() == 2 and kp1.shape[0] == 1 else matches
    dm1, dm2 = (t.unsqueeze(0) if t.dim() == 2 and kp1.shape[0] == 1 else t for t in (depth_map1, depth_map2))
    _check_float_pair(kp1, kp2, "keypoints")
    _check_float_pair(dm1, dm2, "depth maps")
    _check_match_dtype(mt)
    _check_keypoint_tables(kp1, kp2)
    B = kp1.shape[0]
    _check_match_rows(mt, B, "keypoints", kp2.shape[0] == B)
    if dm1.dim() != 3 or dm2.dim() != 3 or dm1.shape[0] != B or dm2.shape[0] != B:
        raise ValueError("depth maps must have shape (B, H, W) with the keypoints' B")
    kp1, kp2, mt, dm1, dm2 = (t.contiguous() for t in (kp1, kp2, _narrow_matches(mt), dm1, dm2))
    c1, c2 = _center(center1, B, dev), _center(center2, B, dev)
    ftypes = _float_types()
    mm = _capi.Matches(kp1.data_ptr(), kp2.data_ptr(), ftypes[kp1.dtype], kp1.shape[1], kp2.shape[1], mt.data_ptr(), mt.shape[1],
                       dm1.data_ptr(), dm2.data_ptr(), ftypes[dm1.dtype], dm1.shape[1], dm1.shape[2], dm2.shape[1], dm2.shape[2],
                       _data_ptr(c1), _data_ptr(c2), _capi.FILTERS[filter])
    return mm, (kp1, kp2, mt, dm1, dm2, c1, c2), B, int(mt.shape[1]), dev


def _front_end_scores(scores, matches):
    """scores= of a front-end entry point -> (ranked call?, score tensor shaped like matches' rows or None for rows in quality order already).
    Checked against `matches` as the caller passed it, before anything touches the device."""
    import torch
    if scores is None:
        return False, None
    if isinstance(scores, str):
        if scores != PRESORTED:
            raise ValueError(f'scores: the only string is "{PRESORTED}", not {scores!r}')
        return True, None
    if not (isinstance(scores, torch.Tensor) and scores.dtype in (torch.float32, torch.float64)):
        raise ValueError('scores must be a float32 / float64 tensor on the inputs\' device or "presorted"')
    if not (isinstance(matches, torch.Tensor) and matches.dim() in (2, 3)):
        raise ValueError("matches must have shape (B, M, 2)")
    if scores.device != matches.device:
        raise ValueError("scores must live on the inputs' device")
    rows = tuple(matches.shape[:-1])
    if tuple(scores.shape) != rows and not (len(rows) == 2 and rows[0] == 1 and tuple(scores.shape) == rows[1:]):
        raise ValueError(f"scores must be {rows}, one per match row, not {tuple(scores.shape)}")
    return True, scores


def _score_args(sc):
    """(device pointer or None, score_type, the tensor to keep alive) of a checked score tensor: float32 goes in as it is, nothing is widened"""
    import torch
    if sc is None:
        return None, _capi.F64, None
    sc = sc.contiguous()
    return sc.data_ptr(), _capi.F32 if sc.dtype == torch.float32 else _capi.F64, sc


def _gather_rows(stem, desc, B, M, dev, ranked, sc):
    """the gather alone of a Matches ("matches") or ImagePairs ("image_pairs") descriptor on the device's current torch stream: (x1, x2, d1, d2,
    n_per_pair, slot)"""
    import torch
    h = _handle_on(dev)
    with torch.cuda.device(dev):
        x1 = torch.empty((B, M, 2), dtype=torch.float64, device=dev)
        x2 = torch.empty((B, M, 2), dtype=torch.float64, device=dev)
        d1 = torch.empty((B, M), dtype=torch.float64, device=dev)
        d2 = torch.empty((B, M), dtype=torch.float64, device=dev)
        slot = torch.empty((B, M), dtype=torch.int32, device=dev)
        out = (x1.data_ptr(), x2.data_ptr(), d1.data_ptr(), d2.data_ptr(), slot.data_ptr())
        if ranked:
            sp, st, sc = _score_args(sc)
            n = getattr(h, f"gather_{stem}_ranked")(desc, sp, st, B, *out)
        else:
            n = getattr(h, f"gather_{stem}")(desc, B, *out)
    del sc
    return x1, x2, d1, d2, n, slot


def _estimate_rows(stem, k, desc, B, M, dev, ranked, sc, cams1, cams2, ransac_opt, bundle_opt):
    """front end + estimator of either descriptor with depth maps on the device's current torch stream: (records, match_mask, n_used)"""
    import torch
    ro, bo = _capi.ransac_opt_from_dict(ransac_opt), _capi.bundle_opt_from_dict(bundle_opt)
    h = _handle_on(dev)
    with torch.cuda.device(dev):
        match_mask = torch.zeros((B, M), dtype=torch.uint8, device=dev)
        if ranked:
            sp, st, sc = _score_args(sc)
            n_used = getattr(h, f"estimate_{stem}_ranked_device")(k, desc, sp, st, B, ro, bo, cams1, cams2, match_mask.data_ptr())
        else:
            n_used = getattr(h, f"estimate_{stem}_device")(k, desc, B, ro, bo, cams1, cams2, match_mask.data_ptr())
        res = h.fetch_results(B)
    del sc
    return res, match_mask, n_used


def gather_matches_torch(keypoints1, keypoints2, matches, depth_map1, depth_map2, center1=None, center2=None, filter="both_inf", scores=None):
    """The front end alone, on the device's current torch stream.  keypoints (B, K, 2) float32 | float64 (a (K, 2) tensor is B = 1), matches
    (B, M, 2) int32 | int64 with -1 rows as padding, depth maps (B, H, W) float32 | float64 (the two images may differ in size), all on one
    ROCm device; center1 / center2: optional (B, 2) or (2,) principal points, subtracted in float64; filter: "both_inf" (the reference
    scripts' rule) | "finite".  Returns (x1, x2 (B, M, 2), d1, d2 (B, M): float64 device tensors, kept rows first, in match order, the
    rest x = 0, d = 1; n_per_pair: numpy int32; slot (B, M): int32 device tensor, the position of every match row, -1 if dropped).
    One stream synchronisation (the counts).
    scores: a (B, M) float32 | float64 tensor on the inputs' device ((M,) for B = 1), one per match row, higher is better (a matcher's
    confidence) — the kept rows come in QUALITY order instead (mdrp_amd/frontend.py rule 6): slot is the rank of every match row,
    the buffers are what estimate_batch_torch(..., scores="presorted") takes.  A score never drops a row.  "presorted": the rows are in quality
    order already, which for the gather alone is no scores at all."""
    ranked, sc = _front_end_scores(scores, matches)
    mm, keep, B, M, dev = _matches_descriptor(keypoints1, keypoints2, matches, depth_map1, depth_map2, center1, center2, filter)
    out = _gather_rows("matches", mm, B, M, dev, ranked, sc)
    del keep
    return out


def estimate_matches_torch(kind, keypoints1, keypoints2, matches, depth_map1, depth_map2, cameras1=None, cameras2=None, ransac_opt=None,
                           bundle_opt=None, center1=None, center2=None, filter="both_inf", scores=None):
    """estimate_batch_torch straight from a matcher's output and two depth maps (inputs as gather_matches_torch): the correspondences are
    gathered on the device into buffers of the handle and handed to the same estimator — records identical to gathering with
    mdrp_amd.frontend.gather_matches_numpy and calling estimate_batch_torch with its n_per_pair.  kind: "calibrated" | "shared_focal" |
    "varying_focal" (pass center1 / center2 for the focal estimators: they take principal-point-centred pixels).  Queued on the device's
    current torch stream; the B kept-row counts cross to the host behind one stream synchronisation, then the 136-byte result records.
    Returns (records, match_mask: (B, M) uint8 device tensor — 1 where the row was kept and is an inlier —, n_used: numpy int32).
    scores (see PRESORTED and gather_matches_torch): one score per match row or "presorted" — the estimate in score order with the progressive
    sampler, bit for bit estimate_batch_torch(scores=the kept rows' scores) on the unranked gather; the gather itself ranks, each kept row is
    written once.  progressive_sampling in ransac_opt may be absent, False or True; without scores it is refused as before."""
    ranked, sc = _front_end_scores(scores, matches)
    k = _monodepth_kind(kind)
    mm, keep, B, M, dev = _matches_descriptor(keypoints1, keypoints2, matches, depth_map1, depth_map2, center1, center2, filter)
    cams1 = cams2 = None
    if k == _capi.CALIB:
        cams1, cams2 = _camera_records(cameras1, B), _camera_records(cameras2, B)
    out = _estimate_rows("matches", k, mm, B, M, dev, ranked, sc, cams1, cams2, ransac_opt, bundle_opt)
    del keep
    return out


# ---- the front end for DENSE matchers (include/mdrp_dense.h): a warp and its certainty instead of keypoints and index pairs.  What the
# reference's dense demo does between the matcher and the estimator (certainty-weighted sampling, a density-balanced re-sampling, pixel coordinates,
# depths at the truncated pixel, the depth filter) on the device; mdrp_amd/frontend.py sample_dense_numpy is the definition, equal as bytes.
def _dense_descriptor(warp, certainty, depth_map1, depth_map2, n, seed, coords, threshold, balanced, expansion, grid, min_count, filter, ranked,
                      center1, center2):
    """validated mdrp_dense_matches descriptor of torch tensors on one ROCm device -> (descriptor, tensors it points into, B, device)"""
    if filter not in _capi.FILTERS:
        raise ValueError(f"filter must be one of {tuple(_capi.FILTERS)}, not {filter!r}")
    if coords not in _capi.DENSE_COORDS:
        raise ValueError(f"coords must be one of {tuple(_capi.DENSE_COORDS)}, not {coords!r}")
    n, expansion, grid, min_count = (int(v) for v in (n, expansion, grid, min_count))
    if not 1 <= n <= _capi.DENSE_MAX_N:
        raise ValueError(f"n must be 1 .. {_capi.DENSE_MAX_N}, not {n}")
    if expansion < 1 or expansion * n > _capi.DENSE_MAX_STAGE1:
        raise ValueError(f"expansion must be at least 1 and expansion * n at most {_capi.DENSE_MAX_STAGE1}, not {expansion} * {n}")
    if not 1 <= grid <= _capi.DENSE_MAX_GRID:
        raise ValueError(f"grid must be 1 .. {_capi.DENSE_MAX_GRID}, not {grid}")
    if min_count < 1:
        raise ValueError(f"min_count must be at least 1, not {min_count}")
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit 64 bits (its low 32 bits are used)")
    threshold = float(threshold)
    dev = _check_on_gpu({"warp": warp, "certainty": certainty, "depth_map1": depth_map1, "depth_map2": depth_map2})
    ftypes = _float_types()
    if warp.dtype not in ftypes or certainty.dtype not in ftypes:
        raise ValueError("warp and certainty must be float32 or float64")
    _check_float_pair(depth_map1, depth_map2, "depth maps")
    if warp.dim() not in (3, 4) or warp.shape[-1] != 4:
        raise ValueError("warp must have shape (B, R, 4) or (B, Hc, Wc, 4)")
    B = int(warp.shape[0])
    R = int(warp[0].numel()) // 4 if B > 0 else 0
    if certainty.dim() not in (2, 3) or certainty.shape[0] != B or tuple(certainty.shape[1:]) != tuple(warp.shape[1:-1]):
        raise ValueError(f"certainty must have shape {tuple(warp.shape[:-1])}, one value per warp row, not {tuple(certainty.shape)}")
    if R > _capi.DENSE_MAX_ROWS:
        raise ValueError(f"a pair's warp has at most 2^22 rows, not {R}")
    if depth_map1.dim() != 3 or depth_map2.dim() != 3 or depth_map1.shape[0] != B or depth_map2.shape[0] != B:
        raise ValueError("depth maps must have shape (B, H, W) with the warp's B")
    wp, ct, dm1, dm2 = (t.contiguous() for t in (warp, certainty, depth_map1, depth_map2))
    c1, c2 = _center(center1, B, dev), _center(center2, B, dev)
    desc = _capi.DenseMatches(wp.data_ptr(), ftypes[wp.dtype], R, ct.data_ptr(), ftypes[ct.dtype], _capi.DENSE_COORDS[coords], dm1.data_ptr(), dm2.data_ptr(),
                              ftypes[dm1.dtype], dm1.shape[1], dm1.shape[2], dm2.shape[1], dm2.shape[2], _capi.FILTERS[filter],
                              _data_ptr(c1), _data_ptr(c2), n, 1 if balanced else 0, expansion, grid,
                              min_count, 1 if ranked else 0, seed, threshold, None, None)
    return desc, (wp, ct, dm1, dm2, c1, c2), B, dev


def sample_dense_torch(warp, certainty, depth_map1, depth_map2, n=5000, seed=0, coords="normalized", threshold=0.05, balanced=True, expansion=4, grid=8,
                       min_count=2, filter="both_inf", ranked=False, center1=None, center2=None):
    """A dense matcher's output to the estimators' records, on the device's current torch stream.  warp (B, R, 4) or (B, Hc, Wc, 4) float32 |
    float64 rows (xA, yA, xB, yB) - several layouts such as symmetric halves concatenate along the rows -, certainty with one value per row, depth
    maps (B, H, W) float32 | float64 of their images' sizes, all on one ROCm device.  coords: "normalized" ([-1, 1] over each image, as the matcher
    emits them) | "pixel".  n records per pair are drawn by certainty (certainties above `threshold` count alike), from `expansion` times as many
    when `balanced`, which then re-draws n of them with weights inverse to the number of draws in their cell of a grid^4 histogram over both images
    (cells of fewer than min_count draws get the smallest weight); mdrp_amd.frontend.sample_dense_numpy states every rule, and the result equals it
    as bytes.  threshold, expansion, grid and min_count are untuned defaults: their effect on pose accuracy has not been measured.  The result of a
    pair depends on the pair and the seed, not on its batch.
    Returns (x1, x2 (B, n, 2), d1, d2 (B, n): float64 device tensors, the records first - in ascending row order, or with ranked=True in descending
    certainty, the order estimate_batch_torch(scores="presorted") takes -, the rest x = 0, d = 1; n_per_pair: numpy int32; rows (B, n): int32 device
    tensor, the warp row of every record, -1 behind the count; score (B, n): float64 device tensor, its certainty).  One stream synchronisation."""
    import torch
    desc, keep, B, dev = _dense_descriptor(warp, certainty, depth_map1, depth_map2, n, seed, coords, threshold, balanced, expansion, grid, min_count,
                                           filter, ranked, center1, center2)
    n = desc.n
    h = _handle_on(dev)
    with torch.cuda.device(dev):
        x1 = torch.empty((B, n, 2), dtype=torch.float64, device=dev)
        x2 = torch.empty((B, n, 2), dtype=torch.float64, device=dev)
        d1 = torch.empty((B, n), dtype=torch.float64, device=dev)
        d2 = torch.empty((B, n), dtype=torch.float64, device=dev)
        rows = torch.empty((B, n), dtype=torch.int32, device=dev)
        score = torch.empty((B, n), dtype=torch.float64, device=dev)
        cnt = h.sample_dense(desc, B, x1.data_ptr(), x2.data_ptr(), d1.data_ptr(), d2.data_ptr(), rows.data_ptr(), score.data_ptr())
    del keep
    return x1, x2, d1, d2, cnt, rows, score


def estimate_dense_torch(kind, warp, certainty, depth_map1, depth_map2, cameras1=None, cameras2=None, ransac_opt=None, bundle_opt=None, n=5000, seed=0,
                         coords="normalized", threshold=0.05, balanced=True, expansion=4, grid=8, min_count=2, filter="both_inf", ranked=False,
                         center1=None, center2=None):
    """estimate_batch_torch straight from a dense matcher's output and two depth maps (inputs as sample_dense_torch): the records are sampled on the
    device into buffers of the handle and handed to the same estimator - byte for byte estimate_batch_torch on sample_dense_torch's output with its
    n_per_pair (ranked=True: with scores="presorted", the progressive sampler in descending certainty; progressive_sampling in ransac_opt may then
    be absent, False or True, and without ranked it is refused as before).  kind: "calibrated" | "shared_focal" | "varying_focal" (pass center1 /
    center2 for the focal estimators: they take principal-point-centred pixels).  Queued on the device's current torch stream; the B counts cross to
    the host behind one stream synchronisation, then the 136-byte result records.
    Returns (records, record_mask: (B, n) uint8 device tensor - 1 where the sampled record is an inlier -, n_used: numpy int32, rows: (B, n) int32
    device tensor, the warp row of every record, -1 behind the count)."""
    import torch
    k = _monodepth_kind(kind)
    desc, keep, B, dev = _dense_descriptor(warp, certainty, depth_map1, depth_map2, n, seed, coords, threshold, balanced, expansion, grid, min_count,
                                           filter, ranked, center1, center2)
    n = desc.n
    cams1 = cams2 = None
    if k == _capi.CALIB:
        cams1, cams2 = _camera_records(cameras1, B), _camera_records(cameras2, B)
    ro, bo = _capi.ransac_opt_from_dict(ransac_opt), _capi.bundle_opt_from_dict(bundle_opt)
    h = _handle_on(dev)
    with torch.cuda.device(dev):
        record_mask = torch.zeros((B, n), dtype=torch.uint8, device=dev)
        rows = torch.empty((B, n), dtype=torch.int32, device=dev)
        desc.rows_out = rows.data_ptr()
        n_used = h.estimate_dense_device(k, desc, B, ro, bo, cams1, cams2, record_mask.data_ptr())
        res = h.fetch_results(B)
    del keep
    return res, record_mask, n_used, rows


# ---- the same for a batch held per IMAGE (include/mdrp.h mdrp_image_pairs): keypoint tables and depth maps exist once per image
# and the pairs are index pairs into the image set — every frame of a video against one anchor, each image of an SfM set against many
# others — so nothing is copied once per pair.  mdrp_amd/frontend.py gather_image_pairs_numpy states the semantics.
def _host_pairs(pairs):
    """(B, 2) image indices as a contiguous host int32 array, from a sequence, a NumPy array or a tensor on any device"""
    if hasattr(pairs, "detach"):
        pairs = pairs.detach().cpu().numpy()
    pairs = np.asarray(pairs)
    if pairs.size == 0:
        return np.zeros((0, 2), dtype=np.int32)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in "iu":
        raise ValueError("pairs must be (B, 2) integer image indices")
    return np.ascontiguousarray(np.clip(pairs, -1, 2 ** 31 - 1).astype(np.int32))  # (an index past int32 stays out of range instead of wrapping into it)


def _image_pairs_descriptor(keypoints, depth_maps, pairs, matches, centers, sizes, kp_counts, filter, need_host_pairs):
    """validated mdrp_image_pairs descriptor of torch tensors on one ROCm device -> (descriptor, tensors it points into, host pairs, B, M, I, device);
    host pairs is None where they were not asked for and pairs already lives on the device (no copy back, no synchronisation)"""
    import torch
    if filter not in _capi.FILTERS:
        raise ValueError(f"filter must be one of {tuple(_capi.FILTERS)}, not {filter!r}")
    dev = _check_on_gpu({"keypoints": keypoints, "depth_maps": depth_maps, "matches": matches})
    ftypes = _float_types()
    if keypoints.dtype not in ftypes or depth_maps.dtype not in ftypes:
        raise ValueError("keypoints and depth maps must be float32 or float64")
    _check_match_dtype(matches)
    if keypoints.dim() != 3 or keypoints.shape[2] != 2:
        raise ValueError("keypoints must have shape (I, K, 2)")
    I = keypoints.shape[0]
    if depth_maps.dim() != 3 or depth_maps.shape[0] != I:
        raise ValueError("depth maps must have shape (I, H, W) with the keypoints' I")
    on_device, host_pairs, B = _pairs_on_host(pairs, dev, need_host_pairs)
    _check_match_rows(matches, B, "pairs")
    kp, dm, mt = keypoints.contiguous(), depth_maps.contiguous(), _narrow_matches(matches).contiguous()
    cs = _per_image(centers, torch.float64, (I, 2), "centers", dev)
    sz = _per_image(sizes, torch.int32, (I, 2), "sizes", dev)
    kc = _per_image(kp_counts, torch.int32, (I,), "kp_counts", dev)
    pr = _pairs_on_device(pairs, on_device, host_pairs, dev)
    ip = _capi.ImagePairs(kp.data_ptr(), ftypes[kp.dtype], kp.shape[1], _data_ptr(kc), dm.data_ptr(), ftypes[dm.dtype], dm.shape[1], dm.shape[2], _data_ptr(sz),
                          _data_ptr(cs), I, pr.data_ptr(), mt.data_ptr(), mt.shape[1], _capi.FILTERS[filter])
    return ip, (kp, dm, mt, cs, sz, kc, pr), host_pairs, B, int(mt.shape[1]), I, dev


def gather_image_pairs_torch(keypoints, depth_maps, pairs, matches, centers=None, sizes=None, kp_counts=None, filter="both_inf", scores=None):
    """gather_matches_torch for pairs given as image indices.  keypoints (I, K, 2) and depth_maps (I, H, W) float32 | float64, matches (B, M, 2)
    int32 | int64 with -1 rows as padding, all on one ROCm device; pairs (B, 2) image indices (a, c) as a sequence, NumPy array or tensor on any
    device (a pair with an index outside [0, I) is empty: n = 0, slots -1, filler).  sizes (I, 2) (h, w) and kp_counts (I,): the valid part of
    each image's map and table (clamped to H, W and K; None = all); centers (I, 2) or (2,), subtracted in float64.  Returns what
    gather_matches_torch returns, on the device's current torch stream, behind one stream synchronisation (the counts).  scores: as
    gather_matches_torch's, (B, M)."""
    ranked, sc = _front_end_scores(scores, matches)
    ip, keep, _, B, M, _, dev = _image_pairs_descriptor(keypoints, depth_maps, pairs, matches, centers, sizes, kp_counts, filter, False)
    out = _gather_rows("image_pairs", ip, B, M, dev, ranked, sc)
    del keep
    return out


def _pair_cameras(cameras, host_pairs, I):
    """per-image cameras (one for all | a list of I | a CAMERA_DTYPE array of I) -> two [B] per-pair record arrays.  A pair with an image index
    outside [0, I) gets record 0 (a zero record when I == 0): it has n = 0, no correspondence is read against its camera."""
    rec = _camera_records(cameras, I) if I > 0 else np.zeros(1, dtype=_capi.CAMERA_DTYPE)
    idx = np.where((host_pairs >= 0) & (host_pairs < I), host_pairs, 0)
    return np.ascontiguousarray(rec[idx[:, 0]]), np.ascontiguousarray(rec[idx[:, 1]])


def estimate_image_pairs_torch(kind, keypoints, depth_maps, pairs, matches, cameras=None, ransac_opt=None, bundle_opt=None, centers=None, sizes=None,
                               kp_counts=None, filter="both_inf", scores=None):
    """estimate_matches_torch for pairs given as image indices (inputs as gather_image_pairs_torch): records identical to gathering with
    mdrp_amd.frontend.gather_image_pairs_numpy and calling estimate_batch_torch with its n_per_pair and the per-pair cameras.  cameras
    (calibrated only) are per IMAGE — one Camera | dict for all, a list of I, or a CAMERA_DTYPE array of I records — and expanded to per-pair
    records by pairs on the host.  kind: "calibrated" | "shared_focal" | "varying_focal" (pass centers for the focal estimators).
    Returns (records, match_mask: (B, M) uint8 device tensor, n_used: numpy int32), stream behaviour as estimate_matches_torch.  scores: as
    estimate_matches_torch's, (B, M)."""
    ranked, sc = _front_end_scores(scores, matches)
    k = _monodepth_kind(kind)
    ip, keep, host_pairs, B, M, I, dev = _image_pairs_descriptor(keypoints, depth_maps, pairs, matches, centers, sizes, kp_counts, filter, True)
    cams1 = cams2 = None
    if k == _capi.CALIB:
        cams1, cams2 = _pair_cameras(cameras, host_pairs, I)
    out = _estimate_rows("image_pairs", k, ip, B, M, dev, ranked, sc, cams1, cams2, ransac_opt, bundle_opt)
    del keep
    return out


# ---- the same two front ends for the comparison rows, which have no depths (include/mdrp_classic_frontend.h): keypoint tables and index
# pairs go in, the 5- / 6- / 7-point baselines run on the gathered correspondences.  mdrp_amd/frontend.py gather_point_matches_numpy /
# gather_point_image_pairs_numpy state the semantics: a row is kept iff its indices address their tables and its four coordinates are finite.
def _point_matches_descriptor(keypoints1, keypoints2, matches, center1, center2):
    """_matches_descriptor without the depth maps: validated mdrp_point_matches descriptor -> (descriptor, tensors it points into, B, M, device)"""
    named = {"keypoints1": keypoints1, "keypoints2": keypoints2, "matches": matches}
    _check_tensors(named)
    kp1, kp2 = (t.unsqueeze(0) if t.dim() == 2 else t for t in (keypoints1, keypoints2))
    mt = matches.unsqueeze(0) if matches.dim() == 2 and kp1.shape[0] == 1 else matches
    _check_float_pair(kp1, kp2, "keypoints")
    _check_match_dtype(mt)
    _check_keypoint_tables(kp1, kp2)
    B = kp1.shape[0]
    _check_match_rows(mt, B, "keypoints", kp2.shape[0] == B)
    dev = _check_on_gpu(named)  # (types and shapes first: a caller who mixes both up hears about the tensors themselves)
    kp1, kp2, mt = (t.contiguous() for t in (kp1, kp2, _narrow_matches(mt)))
    c1, c2 = _center(center1, B, dev), _center(center2, B, dev)
    pm = _capi.PointMatches(kp1.data_ptr(), kp2.data_ptr(), _float_types()[kp1.dtype], kp1.shape[1], kp2.shape[1], mt.data_ptr(), mt.shape[1],
                            _data_ptr(c1), _data_ptr(c2))
    return pm, (kp1, kp2, mt, c1, c2), B, int(mt.shape[1]), dev


def _point_image_pairs_descriptor(keypoints, pairs, matches, centers, kp_counts, need_host_pairs):
    """_image_pairs_descriptor without the depth maps: validated mdrp_point_image_pairs descriptor -> (descriptor, tensors it points into, host
    pairs or None, B, M, I, device)"""
    import torch
    named = {"keypoints": keypoints, "matches": matches}
    _check_tensors(named)
    dev = keypoints.device
    if keypoints.dtype not in _float_types():
        raise ValueError("keypoints must be float32 or float64")
    _check_match_dtype(matches)
    if keypoints.dim() != 3 or keypoints.shape[2] != 2:
        raise ValueError("keypoints must have shape (I, K, 2)")
    I = keypoints.shape[0]
    on_device, host_pairs, B = _pairs_on_host(pairs, dev, need_host_pairs)
    _check_match_rows(matches, B, "pairs")
    _check_on_gpu(named)  # (types and shapes first, as _point_matches_descriptor)
    kp, mt = keypoints.contiguous(), _narrow_matches(matches).contiguous()
    cs = _per_image(centers, torch.float64, (I, 2), "centers", dev)
    kc = _per_image(kp_counts, torch.int32, (I,), "kp_counts", dev)
    pr = _pairs_on_device(pairs, on_device, host_pairs, dev)
    pp = _capi.PointImagePairs(kp.data_ptr(), _float_types()[kp.dtype], kp.shape[1], _data_ptr(kc), _data_ptr(cs), I, pr.data_ptr(), mt.data_ptr(), mt.shape[1])
    return pp, (kp, mt, cs, kc, pr), host_pairs, B, int(mt.shape[1]), I, dev


def _gather_points(desc, B, M, dev, ranked, sc):
    """the gather alone of either descriptor on the device's current torch stream: (x1, x2, n_per_pair, slot)"""
    import torch
    h = _handle_on(dev)
    with torch.cuda.device(dev):
        x1 = torch.empty((B, M, 2), dtype=torch.float64, device=dev)
        x2 = torch.empty((B, M, 2), dtype=torch.float64, device=dev)
        slot = torch.empty((B, M), dtype=torch.int32, device=dev)
        sp, st, sc = _score_args(sc)
        n = h.gather_points(desc, B, x1.data_ptr(), x2.data_ptr(), slot.data_ptr(), sp, st, ranked)
    del sc
    return x1, x2, n, slot


def _estimate_points(k, desc, B, M, dev, ranked, sc, cams1, cams2, ransac_opt, bundle_opt):
    """front end + baseline of either descriptor on the device's current torch stream: (records, match_mask, n_used)"""
    import torch
    ro, bo = _capi.ransac_opt_from_dict(ransac_opt), _capi.bundle_opt_from_dict(bundle_opt)
    h = _handle_on(dev)
    with torch.cuda.device(dev):
        match_mask = torch.zeros((B, M), dtype=torch.uint8, device=dev)
        sp, st, sc = _score_args(sc)
        n_used = h.estimate_points_device(k, desc, B, ro, bo, cams1, cams2, match_mask.data_ptr(), sp, st, ranked)
        res = h.fetch_results(B)
    del sc
    return res, match_mask, n_used


def gather_point_matches_torch(keypoints1, keypoints2, matches, center1=None, center2=None, scores=None):
    """gather_matches_torch without depth maps, for the 5- / 6- / 7-point baselines: keypoints (B, K, 2) float32 | float64 (a (K, 2) tensor is
    B = 1), matches (B, M, 2) int32 | int64 with -1 rows as padding, all on one ROCm device; center1 / center2: optional (B, 2) or (2,), subtracted in
    float64.  A row is kept iff its indices address their tables and its four coordinates are finite (mdrp_amd/frontend.py
    gather_point_matches_numpy).  Returns (x1, x2 (B, M, 2): float64 device tensors, kept rows first, the rest 0; n_per_pair: numpy int32; slot
    (B, M): int32 device tensor, -1 if dropped).  One stream synchronisation (the counts).  scores: as gather_matches_torch's — the kept rows in
    QUALITY order, what estimate_baseline_batch_torch(..., scores="presorted") takes."""
    ranked, sc = _front_end_scores(scores, matches)
    pm, keep, B, M, dev = _point_matches_descriptor(keypoints1, keypoints2, matches, center1, center2)
    out = _gather_points(pm, B, M, dev, ranked, sc)
    del keep
    return out


def estimate_baseline_matches_torch(kind, keypoints1, keypoints2, matches, cameras1=None, cameras2=None, pp=None, ransac_opt=None, bundle_opt=None,
                                    center1=None, center2=None, scores=None):
    """estimate_baseline_batch_torch straight from a matcher's output (inputs as gather_point_matches_torch): records identical to gathering with
    mdrp_amd.frontend.gather_point_matches_numpy and calling estimate_baseline_batch_torch with its n_per_pair.  kind: see BASELINE_KINDS
    ("relpose_5pt": cameras1 / cameras2 per pair; "shared_focal_6pt": pp and principal-point-centred keypoints through center1 / center2;
    "fundamental_7pt").  Returns (records, match_mask: (B, M) uint8 device tensor — 1 where the row was kept and is an inlier —, n_used: numpy
    int32).  scores: one per match row or "presorted" — the estimate in score order with the progressive sampler, bit for bit
    estimate_baseline_batch_torch(scores="presorted") on the ranked gather; progressive_sampling in ransac_opt may then be absent, False or True,
    without scores it is refused."""
    k = _baseline_kind(kind)
    ranked, sc = _front_end_scores(scores, matches)
    _check_baseline_options(ransac_opt, scores)
    pm, keep, B, M, dev = _point_matches_descriptor(keypoints1, keypoints2, matches, center1, center2)
    cams1 = cams2 = None
    if k == _capi.RELPOSE_5PT:
        cams1, cams2 = _camera_records(cameras1, B), _camera_records(cameras2, B)
    elif k == _capi.SHARED_6PT:
        cams1 = cams2 = _pp_records(pp, B)[0]
    out = _estimate_points(k, pm, B, M, dev, ranked, sc, cams1, cams2, ransac_opt, bundle_opt)
    del keep
    return out


def gather_point_image_pairs_torch(keypoints, pairs, matches, centers=None, kp_counts=None, scores=None):
    """gather_point_matches_torch for pairs given as image indices (gather_image_pairs_torch without depth maps): keypoints (I, K, 2), pairs
    (B, 2) image indices as a sequence, NumPy array or tensor on any device (an index outside [0, I): an empty pair), matches (B, M, 2); kp_counts
    (I,) clamped to K, centers (I, 2) or (2,).  Returns what gather_point_matches_torch returns.  scores: (B, M)."""
    ranked, sc = _front_end_scores(scores, matches)
    desc, keep, _, B, M, _, dev = _point_image_pairs_descriptor(keypoints, pairs, matches, centers, kp_counts, False)
    out = _gather_points(desc, B, M, dev, ranked, sc)
    del keep
    return out


def estimate_baseline_image_pairs_torch(kind, keypoints, pairs, matches, cameras=None, pp=None, ransac_opt=None, bundle_opt=None, centers=None,
                                        kp_counts=None, scores=None):
    """estimate_baseline_matches_torch for pairs given as image indices (inputs as gather_point_image_pairs_torch): records identical to
    gathering with mdrp_amd.frontend.gather_point_image_pairs_numpy and calling estimate_baseline_batch_torch with its n_per_pair and the per-pair
    cameras.  cameras ("relpose_5pt" only) are per IMAGE and expanded to per-pair records by pairs on the host; pp ("shared_focal_6pt") is one
    principal point or one per PAIR (B, 2).  Returns (records, match_mask, n_used)."""
    k = _baseline_kind(kind)
    ranked, sc = _front_end_scores(scores, matches)
    _check_baseline_options(ransac_opt, scores)
    desc, keep, host_pairs, B, M, I, dev = _point_image_pairs_descriptor(keypoints, pairs, matches, centers, kp_counts, k == _capi.RELPOSE_5PT)
    cams1 = cams2 = None
    if k == _capi.RELPOSE_5PT:
        cams1, cams2 = _pair_cameras(cameras, host_pairs, I)
    elif k == _capi.SHARED_6PT:
        cams1 = cams2 = _pp_records(pp, B)[0]
    out = _estimate_points(k, desc, B, M, dev, ranked, sc, cams1, cams2, ransac_opt, bundle_opt)
    del keep
    return out


# ------------------------------------------------------------------------------------------------ refine / verify caller-supplied models
# The counterpart of PoseLib's refine_relative_pose for the three monodepth estimators (include/mdrp.h mdrp_refine_batch): one model
# per pair goes in and the estimator's tail runs on it — score, LO, inlier mask, inlier-only refinement — without a single sample.  A pose from the
# previous video frame, an SfM database or a coarse first pass is refined for the price of the tail; stages=() only counts its inliers with the
# estimator's thresholds, normalisation and cheirality rule.  Of ransac_opt only max_epipolar_error, max_reproj_error, monodepth_weight_sampson and
# monodepth_estimate_shift are read; nothing is refused.
_STAGES = {"lo": _capi.STAGE_LO, "inliers": _capi.STAGE_INLIERS}


def _stage_flags(stages):
    """("lo", "inliers") | a subset | () | the integer flags themselves -> MDRP_STAGE_* flags"""
    if isinstance(stages, (int, np.integer)) and not isinstance(stages, bool):
        return int(stages)
    if isinstance(stages, str):
        stages = (stages,)
    flags = 0
    for s in stages:
        if s not in _STAGES:
            raise ValueError(f"stages must be drawn from {tuple(_STAGES)}, not {s!r}")
        flags |= _STAGES[s]
    return flags


def _model_records(initial, kind):
    """list of MonoDepthTwoViewGeometry (calibrated) / MonoDepthImagePair (focal kinds; focals from the two cameras), or a ready MODEL_DTYPE array"""
    if isinstance(initial, np.ndarray) and initial.dtype == _capi.MODEL_DTYPE:
        return np.ascontiguousarray(initial).reshape(-1)
    out = np.zeros(len(initial), dtype=_capi.MODEL_DTYPE)
    for i, obj in enumerate(initial):
        g = getattr(obj, "geometry", obj)
        out[i]["q"] = g.pose.q; out[i]["t"] = g.pose.t
        out[i]["scale"], out[i]["shift1"], out[i]["shift2"] = g.scale, g.shift1, g.shift2
        focal = kind != _capi.CALIB and hasattr(obj, "camera1")
        out[i]["f1"] = obj.camera1.focal() if focal else 1.0
        out[i]["f2"] = obj.camera2.focal() if focal else 1.0
    return out


def _refine_info(res, mask_row, n, score0, inl0):
    info = _info(res, mask_row, n)
    info["initial_score"], info["initial_inliers"] = float(score0), int(inl0)
    return info


def _refine_host(kind, points2D_1, points2D_2, depth_1, depth_2, initial, cameras1, cameras2, ransac_opt, bundle_opt, device, stages, as_arrays):
    x1, x2, d1, d2, ns = _stack(points2D_1, points2D_2, depth_1, depth_2)
    B = len(ns)
    models = _model_records(initial, kind)
    if len(models) != B:
        raise ValueError(f"expected {B} initial models, got {len(models)}")
    cams1 = cams2 = None
    if kind == _capi.CALIB:
        cams1, cams2 = _camera_records(cameras1, B), _camera_records(cameras2, B)
    res, mask, score0, inl0 = _capi.default_handle(device).refine_batch(kind, x1, x2, d1, d2, models, _capi.ransac_opt_from_dict(ransac_opt),
                                                                        _capi.bundle_opt_from_dict(bundle_opt), _stage_flags(stages), ns, cams1, cams2)
    if as_arrays:
        return res, mask, ns, score0, inl0
    wrap = _geometry_from_model if kind == _capi.CALIB else _pair_from_model
    return [wrap(r["model"]) for r in res], [_refine_info(res[i], mask[i], ns[i], score0[i], inl0[i]) for i in range(B)]


def refine_monodepth_relative_pose_batch(points2D_1, points2D_2, depth_1, depth_2, cameras1, cameras2, geometries, ransac_opt=None, bundle_opt=None,
                                         device=0, stages=("lo", "inliers"), as_arrays=False):
    """B calibrated pairs, each with a MonoDepthTwoViewGeometry to start from (or a MODEL_DTYPE array).  Returns (list[MonoDepthTwoViewGeometry],
    list[info dict]): the estimators' info keys describing the model that entered the inlier-only refinement, plus `initial_score` and
    `initial_inliers` of the model handed in.  as_arrays=True: (records, masks, n_per_pair, initial scores, initial inlier counts)."""
    return _refine_host(_capi.CALIB, points2D_1, points2D_2, depth_1, depth_2, geometries, cameras1, cameras2, ransac_opt, bundle_opt, device, stages, as_arrays)


def refine_monodepth_shared_focal_relative_pose_batch(points2D_1, points2D_2, depth_1, depth_2, image_pairs, ransac_opt=None, bundle_opt=None,
                                                      device=0, stages=("lo", "inliers"), as_arrays=False):
    """B pairs of principal-point-centred pixels, each with a MonoDepthImagePair to start from (focals: camera1 / camera2 .focal(), in pixels)"""
    return _refine_host(_capi.SHARED_FOCAL, points2D_1, points2D_2, depth_1, depth_2, image_pairs, None, None, ransac_opt, bundle_opt, device, stages, as_arrays)


def refine_monodepth_varying_focal_relative_pose_batch(points2D_1, points2D_2, depth_1, depth_2, image_pairs, ransac_opt=None, bundle_opt=None,
                                                       device=0, stages=("lo", "inliers"), as_arrays=False):
    return _refine_host(_capi.VARYING_FOCAL, points2D_1, points2D_2, depth_1, depth_2, image_pairs, None, None, ransac_opt, bundle_opt, device, stages, as_arrays)


def _need_initial(initial, what):
    if initial is None:
        raise ValueError(f"{what} is required: there is nothing to refine without a model to start from")
    return [initial]


def refine_monodepth_relative_pose(points2D_1, points2D_2, depth_1, depth_2, camera1, camera2, ransac_opt={}, bundle_opt={}, initial_pose=None,
                                   stages=("lo", "inliers")):
    """estimate_monodepth_relative_pose's arguments; initial_pose (a MonoDepthTwoViewGeometry) is READ here.  Returns (geometry, info)."""
    g, i = refine_monodepth_relative_pose_batch([_as_points(points2D_1)], [_as_points(points2D_2)], [depth_1], [depth_2], camera1, camera2,
                                                _need_initial(initial_pose, "initial_pose"), ransac_opt, bundle_opt, stages=stages)
    return g[0], i[0]


def refine_monodepth_shared_focal_relative_pose(points2D_1, points2D_2, depth_1, depth_2, ransac_opt={}, bundle_opt={}, initial_image_pair=None,
                                                stages=("lo", "inliers")):
    p, i = refine_monodepth_shared_focal_relative_pose_batch([_as_points(points2D_1)], [_as_points(points2D_2)], [depth_1], [depth_2],
                                                             _need_initial(initial_image_pair, "initial_image_pair"), ransac_opt, bundle_opt, stages=stages)
    return p[0], i[0]


def refine_monodepth_varying_focal_relative_pose(points2D_1, points2D_2, depth_1, depth_2, ransac_opt={}, bundle_opt={}, initial_image_pair=None,
                                                 stages=("lo", "inliers")):
    p, i = refine_monodepth_varying_focal_relative_pose_batch([_as_points(points2D_1)], [_as_points(points2D_2)], [depth_1], [depth_2],
                                                              _need_initial(initial_image_pair, "initial_image_pair"), ransac_opt, bundle_opt, stages=stages)
    return p[0], i[0]


def refine_batch_torch(kind, points2D_1, points2D_2, depth_1, depth_2, models, cameras1=None, cameras2=None, ransac_opt=None, bundle_opt=None,
                       n_per_pair=None, stages=("lo", "inliers")):
    """The same on a batch that already lives on the GPU (inputs as estimate_batch_torch), queued on the device's current torch stream.
    models: one per pair — a device tensor holding B records of 96 bytes (uint8 (B, 96), or float64 (B, 12): q t scale shift1 shift2 f1 f2; e.g.
    written by a torch op just before the call), or a numpy array of _capi.MODEL_DTYPE, which is uploaded on that stream.  Returns (records,
    inlier mask: (B, N) uint8 device tensor, initial: {"score": (B,) float64, "inliers": (B,) int32} numpy arrays of the models handed in)."""
    import torch
    k = MONODEPTH_KINDS[kind] if isinstance(kind, str) else int(kind)
    flags = _stage_flags(stages)
    x1, x2, d1, d2 = (t.contiguous() for t in (points2D_1, points2D_2, depth_1, depth_2))
    for t in (x1, x2, d1, d2):
        if not (t.is_cuda and t.dtype == torch.float64):
            raise ValueError("refine_batch_torch needs float64 tensors on the GPU")
        if t.device != x1.device:
            raise ValueError("all tensors must live on the same device")
    B, N = d1.shape
    if x1.shape != (B, N, 2) or x2.shape != (B, N, 2) or d2.shape != (B, N):
        raise ValueError("shapes must be (B, N, 2), (B, N, 2), (B, N), (B, N)")
    if n_per_pair is not None and isinstance(n_per_pair, torch.Tensor):
        n_per_pair = n_per_pair.detach().cpu().numpy()
    cams1 = cams2 = None
    if k == _capi.CALIB:
        cams1, cams2 = _camera_records(cameras1, B), _camera_records(cameras2, B)
    with torch.cuda.device(x1.device):
        h = _handle_on(x1.device)
        if isinstance(models, np.ndarray):
            models = torch.from_numpy(np.ascontiguousarray(models, dtype=_capi.MODEL_DTYPE).reshape(-1).view(np.uint8).copy()).to(x1.device)
        if not (isinstance(models, torch.Tensor) and models.is_cuda and models.device == x1.device and models.dtype in (torch.uint8, torch.float64)):
            raise ValueError("models must be a uint8 / float64 tensor on the inputs' device or a numpy array of _capi.MODEL_DTYPE")
        models = models.contiguous()
        if models.numel() * models.element_size() != B * _capi.MODEL_DTYPE.itemsize:
            raise ValueError(f"models must hold {B} records of {_capi.MODEL_DTYPE.itemsize} bytes")
        mask = torch.zeros((B, N), dtype=torch.uint8, device=x1.device)
        score0 = torch.zeros(B, dtype=torch.float64, device=x1.device)
        inl0 = torch.zeros(B, dtype=torch.int32, device=x1.device)
        h.refine_batch_device(k, x1.data_ptr(), x2.data_ptr(), d1.data_ptr(), d2.data_ptr(), B, N, models.data_ptr(), _capi.ransac_opt_from_dict(ransac_opt),
                              _capi.bundle_opt_from_dict(bundle_opt), flags, n_per_pair, cams1, cams2, mask.data_ptr(), score0.data_ptr(), inl0.data_ptr())
        res = h.fetch_results(B)  # (waits for the stream: the two small tensors below are complete)
        initial = {"score": score0.cpu().numpy(), "inliers": inl0.cpu().numpy()}
    return res, mask, initial


# ---- the back end (include/mdrp_reconstruct.h): fused two-view point clouds from models and depth maps.  mdrp_amd/reconstruct.py holds
# the three entry points; they are found here, beside the estimators whose records they take.
from .reconstruct import reconstruct_image_pairs_torch, reconstruct_pair, reconstruct_pairs_torch  # noqa: E402, F401


# ---- scenes (include/mdrp_scene.h): an image set's pairs chained along a tree, one fused cloud per scene.  mdrp_amd/scene.py holds the
# entry points; they are found here, beside the estimators whose records they take.
from .scene import reconstruct_scene, reconstruct_scene_torch, scene_transforms_torch, scene_tree, video_tree  # noqa: E402, F401


# ---- co-visibility (include/mdrp_covis.h): dense depth-consistency counts per pair.  mdrp_amd/covis.py holds the entry points; they are
# found here, beside the estimators whose records they take.
from .covis import covisibility_image_pairs_torch, covisibility_pair, covisibility_pairs_torch, covisibility_scores  # noqa: E402, F401

# ---- the consistency filter of a scene (include/mdrp_fuse.h): only the points that other images' depth maps confirm.  mdrp_amd/fuse.py
# holds the entry points; they are re-exported here.
from .fuse import fuse_scene, fuse_scene_torch, scene_views  # noqa: E402, F401
