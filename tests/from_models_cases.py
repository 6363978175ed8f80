"""Inputs of the mdrp_refine_batch tests (a helper, not a test): ragged batches with their start models, the yardstick's answers, and the margins that
make "masks identical" a fair demand.  Everything here runs on the CPU (tests/from_models_ref.py over the oracle)."""
import functools

import numpy as np

import from_models_ref as fm
import helpers
from mdrp_amd import synth
from oracle import pyorc as po

RAGGED_N = (0, 2, 3, 4, 8, 63, 64, 65, 257, 300, 600, 777)
# start model of each pair of the ragged batch: ground truth perturbed by about 2 deg / 5 % / 3 %, but for one exact ground truth, one identity model, one
# NaN quaternion and one hopeless model (fewer inliers than stage INLIERS asks for)
RAGGED_START = {63: "exact", 64: "identity", 65: "nan", 257: "hopeless"}
LOSSES = {"TRUNCATED_CAUCHY": 4, "HUBER": 2}
RO = dict(max_epipolar_error=2.0, max_reproj_error=16.0)
F1, F2, PP = 800.0, 700.0, (12.0, -7.0)  # calibrated kind: SIMPLE_PINHOLE for image 1, PINHOLE with fx != fy for image 2 (helpers.options_cameras)


def rotmat_to_quat(R):
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def cameras(kind):
    """((model_id, params), (model_id, params)) of the calibrated kind, None otherwise"""
    if kind != po.CALIB:
        return None
    return (0, [F1, PP[0], PP[1]]), (1, [F2 * 1.01, F2 * 0.99, PP[0], PP[1]])


def make_pair(name, index, n):
    kind, es, rf = helpers.OPTIONS_KINDS[name]
    kw = dict(f1=F1, f2=F2, pp=PP) if kind == po.CALIB else {}
    return synth.make_pair(index, n, noise_px=0.5, depth_noise=0.02, outlier_frac=0.3, random_focal=rf, shift1=0.2 if es else 0.0, shift2=-0.1 if es else 0.0, **kw)


def start_model(name, p, how, rng, amount=1.0):
    """12-wide start model (focals in pixels; 1 for the calibrated kind) of pair p"""
    kind = helpers.OPTIONS_KINDS[name][0]
    f = (1.0, 1.0) if kind == po.CALIB else (p["f1"], p["f2"])
    R, t, scale = p["R"], p["t"], p["scale"]
    if how == "identity":
        return np.r_[1.0, 0, 0, 0, 0, 0, 0, 1.0, 0, 0, f]
    if how == "hopeless":
        R, t, scale = synth.rodrigues(rng.normal(0.0, 1.5, 3)), rng.normal(0.0, 0.5, 3), 1.0
    elif how == "perturbed":
        w = rng.normal(0.0, 1.0, 3)
        R = synth.rodrigues(np.radians(2.0 * amount) * w / np.linalg.norm(w)) @ R
        t = t * (1.0 + 0.05 * amount * rng.uniform(-1.0, 1.0, 3))
        scale = scale * (1.0 + 0.03 * amount)
        f = (f[0] * (1.0 if kind == po.CALIB else 1.0 - 0.03 * amount), f[1] * (1.0 if kind == po.CALIB else 1.0 + 0.03 * amount))
    m = np.r_[rotmat_to_quat(R), t, scale, p["shift1"], p["shift2"], f]
    if how == "nan":
        m[:4] = np.nan
    return m


@functools.lru_cache(maxsize=None)
def batch(name, n_list=RAGGED_N, first=71000, start=tuple(RAGGED_START.items()), amount=1.0):
    """(amount: the size of the perturbation, 1 = about 2 deg / 5 % / 3 %) padded arrays x1, x2 (B, n_max, 2), d1, d2 (B, n_max), n (B,), models (B, 12), cams (or None) of a batch of the estimator `name`"""
    start = dict(start)
    B, n_max = len(n_list), max(max(n_list), 1)
    x1 = np.zeros((B, n_max, 2)); x2 = np.zeros((B, n_max, 2)); d1 = np.ones((B, n_max)); d2 = np.ones((B, n_max))
    models = np.zeros((B, 12))
    rng = np.random.default_rng(first)
    for i, n in enumerate(n_list):
        p = make_pair(name, first + i, max(n, 3))
        x1[i, :n], x2[i, :n], d1[i, :n], d2[i, :n] = p["x1"][:n], p["x2"][:n], p["d1"][:n], p["d2"][:n]
        models[i] = start_model(name, p, start.get(n, "perturbed"), rng, amount)
    return dict(x1=x1, x2=x2, d1=d1, d2=d2, n=np.array(n_list, dtype=np.int32), models=models, cams=cameras(helpers.OPTIONS_KINDS[name][0]))


def oracle_options(name, loss):
    es = helpers.OPTIONS_KINDS[name][1]
    return po.ransac_opt(estimate_shift=es, **RO), po.bundle_opt(max_iterations=100, loss_type=LOSSES[loss], loss_scale=1.0, gradient_tol=1e-10)


def library_options(name, loss, capi):
    es = helpers.OPTIONS_KINDS[name][1]
    return capi.ransac_opt_from_dict(dict(RO, monodepth_estimate_shift=es)), capi.bundle_opt_from_dict({"loss_type": loss})


def camera_records(b, capi):
    """(cam1, cam2) as [B] CAMERA_DTYPE arrays, or (None, None)"""
    if b["cams"] is None:
        return None, None
    out = []
    for mid, params in b["cams"]:
        rec = np.zeros(len(b["n"]), dtype=capi.CAMERA_DTYPE)
        rec["model_id"] = mid
        rec["params"][:, :len(params)] = params
        out.append(rec)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def yardstick(name, loss, stages, **kw):
    """the yardstick's answer for every pair of batch(name, **kw): a list of refine_from_model dicts"""
    kind = helpers.OPTIONS_KINDS[name][0]
    b = batch(name, **kw)
    ro, bo = oracle_options(name, loss)
    c1, c2 = (po.cam_flat(*b["cams"][0]), po.cam_flat(*b["cams"][1])) if b["cams"] else (None, None)
    return [fm.refine_from_model(kind, b["x1"][i, :n], b["x2"][i, :n], b["d1"][i, :n], b["d2"][i, :n], b["models"][i], ro, bo, stages, c1, c2)
            for i, n in enumerate(b["n"])]


def sampson_sq(kind, m, p):
    """squared Sampson residuals of the normalised model m over the prepared pair p (from_models_ref.prep)"""
    F = po.essential(m) if kind == po.CALIB else po.fundamental(m)
    h1, h2 = np.c_[p["a1"], np.ones(len(p["a1"]))], np.c_[p["a2"], np.ones(len(p["a2"]))]
    Fx1, Ftx2 = h1 @ F.T, h2 @ F
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sum(h2 * Fx1, axis=1) ** 2 / (Fx1[:, 0] ** 2 + Fx1[:, 1] ** 2 + Ftx2[:, 0] ** 2 + Ftx2[:, 1] ** 2)


def threshold_margin(kind, r):
    """smallest relative distance of a squared residual of the model that entered stage INLIERS from the squared threshold (inf: no pair, a NaN model)"""
    if r["entered"] is None or np.isnan(r["entered"][0]):
        return np.inf
    r2 = sampson_sq(kind, r["entered"], r["prep"])
    r2 = r2[np.isfinite(r2)]
    return float(np.min(np.abs(r2 / r["prep"]["sq_thr"] - 1.0))) if len(r2) else np.inf


def branches(name, loss, **kw):
    """which branches of the definition the yardstick takes over the batch: a set of names"""
    kind = helpers.OPTIONS_KINDS[name][0]
    b = batch(name, **kw)
    seen = set()
    full, lo_only = yardstick(name, loss, 3, **kw), yardstick(name, loss, fm.STAGE_LO, **kw)
    for i, n in enumerate(b["n"]):
        if n < 3:
            seen.add("n<3")
            continue
        if np.isnan(b["models"][i][0]):
            seen.add("nan")
            continue
        adopted = lo_only[i]["model_score"] < lo_only[i]["initial_score"]
        seen.add("lo_adopted" if adopted else "lo_not_adopted")
        if full[i]["num_inliers"] <= (7 if kind == po.VARYING else 3):
            seen.add("inliers_skipped")
            assert full[i]["refinements"] == 1
        else:
            seen.add("inliers_run")
    return seen


EXACT_N = 40  # records per pair of exact_inlier_batch


@functools.lru_cache(maxsize=None)
def exact_inlier_batch(name, counts, first=75000):
    """one noise-free pair per entry of `counts`: c records that the pair's ground truth counts as inliers (the yardstick's own get_inliers picks them), the
    others gross outliers (the second image's point and depth drawn anew until the yardstick counts none of them), and the start model is that ground
    truth — a model with exactly c inliers, all exact"""
    kind, es, rf = helpers.OPTIONS_KINDS[name]
    kw = dict(f1=F1, f2=F2, pp=PP) if kind == po.CALIB else {}
    B, N = len(counts), EXACT_N
    x1 = np.zeros((B, N, 2)); x2 = np.zeros((B, N, 2)); d1 = np.ones((B, N)); d2 = np.ones((B, N))
    models = np.zeros((B, 12))
    rng = np.random.default_rng(first)
    ro, bo = oracle_options(name, "HUBER")  # (stages = 0: the loss is not looked at)
    cams = cameras(kind)
    c1, c2 = (po.cam_flat(*cams[0]), po.cam_flat(*cams[1])) if cams else (None, None)
    for i, c in enumerate(counts):
        p = synth.make_pair(first + i, N, noise_px=0.0, depth_noise=0.0, outlier_frac=0.0, random_focal=rf, shift1=0.2 if es else 0.0, shift2=-0.1 if es else 0.0, **kw)
        m = start_model(name, p, "exact", rng)
        mask = lambda a2, e2: np.asarray(fm.refine_from_model(kind, p["x1"], a2, p["d1"], e2, m, ro, bo, 0, c1, c2)["mask"], dtype=bool)
        order = np.argsort(~mask(p["x2"], p["d2"]), kind="stable")  # the ground truth's inliers first
        a1, a2, e1, e2 = p["x1"][order], p["x2"][order].copy(), p["d1"][order], p["d2"][order].copy()
        p = dict(p, x1=a1, d1=e1)
        lo, hi = a2.min(axis=0), a2.max(axis=0)
        redo = np.arange(N) >= c
        for _ in range(50):
            a2[redo] = rng.uniform(lo, hi, (int(redo.sum()), 2))
            e2[redo] = rng.uniform(e2.min(), e2.max(), int(redo.sum()))
            redo = mask(a2, e2) & (np.arange(N) >= c)
            if not redo.any():
                break
        x1[i], x2[i], d1[i], d2[i], models[i] = a1, a2, e1, e2, m
    return dict(x1=x1, x2=x2, d1=d1, d2=d2, n=np.full(B, N, dtype=np.int32), models=models, cams=cams)


def exact_inlier_yardstick(name, loss, stages, counts):
    kind = helpers.OPTIONS_KINDS[name][0]
    b = exact_inlier_batch(name, counts)
    ro, bo = oracle_options(name, loss)
    c1, c2 = (po.cam_flat(*b["cams"][0]), po.cam_flat(*b["cams"][1])) if b["cams"] else (None, None)
    return [fm.refine_from_model(kind, b["x1"][i], b["x2"][i], b["d1"][i], b["d2"][i], b["models"][i], ro, bo, stages, c1, c2) for i in range(len(counts))]
