"""Inputs of the tests of the baselines from a caller's model (a helper, not a test): the ragged batch with its start models per kind, the yardstick's
answers (tests/classic_models_ref.py over the oracle, on the CPU), and the margins that make "masks identical" a fair demand."""
import functools

import numpy as np

import classic_models_ref as cm
from from_models_cases import LOSSES, rotmat_to_quat
from mdrp_amd import synth
from oracle import pyorc as po

KINDS = (cm.FIVE, cm.SIX, cm.SEVEN)
KIND_NAMES = {cm.FIVE: "relpose_5pt", cm.SIX: "shared_focal_6pt", cm.SEVEN: "fundamental_7pt"}
RAGGED_N = (0, 4, 5, 6, 7, 8, 63, 65, 255, 257, 500, 777)
# start model of each pair: the ground truth perturbed by about 1 deg / 3 %, but for one exact ground truth, one identity pose (5- and 6-point) or random
# rank-2 F (7-point), one NaN record and one hopeless model
RAGGED_START = {63: "exact", 65: "identity", 255: "nan", 257: "hopeless"}
F, PP = 800.0, (640.0, 480.0)
THR = 2.0
# first synthetic pair of the ragged batch, per kind: chosen so that the yardstick's answer on the pairs without redundancy is determined by the data and
# not by rounding (both conditions are asserted in tests/test_classic_models_host.py, from the yardstick alone):
#   - the 7-point kind's pair of exactly seven records has ONE minimal model (exact_fits).  Seven records in general position have three real fundamental matrices that fit
#     them exactly — the three real roots of the 7-point cubic; each scores the rounding of seven zero residuals (4e-32, 2e-31, 2e-31 on one such pair),
#     so which of them a run ends with is decided in the last bit, and in pixel coordinates they lie 1e-4 .. 1e-2 apart.  About one set of seven
#     records in twenty has a single real root; the 7-point kind's batch starts at such a set;
#     This is the score tie the prior-free estimators' tests already allow for, not a new exemption: DESIGN.md 5 class (v); tests/test_gpu_prior.py
#     EXEMPT / SCORE_TIE and test_exemptions_are_earned (N = 3 with a 3-point solver); the +-1 LO count below N = 100 of
#     tests/test_gpu_parity.py::test_batched_ragged_calls_under_random_options_vs_oracle.  Here nothing is exempted: the input avoids the tie;
#   - on the pairs of at most 8 records the answer does not move under a rounding-sized perturbation of the inputs (prior_sensitivity).
FIRST = {cm.FIVE: 83000, cm.SIX: 83000, cm.SEVEN: 84400}
ITERATIONS = {cm.FIVE: (200, 50), cm.SIX: (100, 50), cm.SEVEN: (200, 50)}  # (max, min) of the long prior run: the 6-point solver is slow


def cameras(kind):
    """((model_id, params), (model_id, params)) of the 5-point kind, None otherwise"""
    if kind != cm.FIVE:
        return None
    return (0, [F, PP[0], PP[1]]), (1, [F * 1.01, F * 0.99, PP[0], PP[1]])


def make_pair(index, n):
    return synth.make_pair(index, n, f1=F, f2=F, pp=PP, noise_px=0.5, outlier_frac=0.3)


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def singular_value_gap(Fm):
    """smallest relative gap between the two non-zero singular values of a start F (two equal ones have no unique factorisation)"""
    s = np.linalg.svd(np.asarray(Fm, float).reshape(3, 3), compute_uv=False)
    return float((s[0] - s[1]) / s[0])


def start_model(kind, p, how, rng, amount=1.0):
    """12-wide start model of pair p (synth.make_pair: its ground truth, focal and principal point) in the caller's units; amount: the size of the
    perturbation (1: about 1 deg / 3 %)"""
    R, t, f, pp = p["R"], p["t"], p["f1"], p["pp"]
    if how == "nan":
        m = np.zeros(12)
        m[0] = np.nan
        m[7] = m[10] = m[11] = 1.0
        return m
    if how == "identity" and kind != cm.SEVEN:
        return np.r_[1.0, 0, 0, 0, 0, 0, 0, 1.0, 0, 0, f if kind == cm.SIX else 1.0, f if kind == cm.SIX else 1.0]
    if how == "identity":  # a random rank-2 F
        U, _, Vt = np.linalg.svd(rng.normal(0.0, 1.0, (3, 3)))
        Fm = U @ np.diag([1.0, 0.6, 0.0]) @ Vt
        return np.r_[Fm.reshape(-1), 0.0, 1.0, 1.0]
    if how == "hopeless":
        R, t = synth.rodrigues(rng.normal(0.0, 1.5, 3)), rng.normal(0.0, 0.5, 3)
    elif how == "perturbed":
        w = rng.normal(0.0, 1.0, 3)
        R = synth.rodrigues(np.radians(1.0 * amount) * w / np.linalg.norm(w)) @ R
        t = t * (1.0 + 0.03 * amount * rng.uniform(-1.0, 1.0, 3))
        f = f * (1.0 - 0.03 * amount)
    if kind == cm.SEVEN:
        Kinv = np.array([[1.0 / f, 0.0, -pp[0] / f], [0.0, 1.0 / f, -pp[1] / f], [0.0, 0.0, 1.0]])
        Fm = Kinv.T @ skew(t) @ R @ Kinv
        return np.r_[(Fm / np.linalg.norm(Fm)).reshape(-1), 0.0, 1.0, 1.0]
    return np.r_[rotmat_to_quat(R), t, 1.0, 0.0, 0.0, f if kind == cm.SIX else 1.0, f if kind == cm.SIX else 1.0]


@functools.lru_cache(maxsize=None)
def batch(kind, n_list=RAGGED_N, first=None, start=tuple(RAGGED_START.items())):
    """padded arrays x1, x2 (B, n_max, 2), n (B,), models (B, 12), cams (or None), pp of a batch of the baseline `kind`"""
    start = dict(start)
    first = FIRST[kind] if first is None else first
    B, n_max = len(n_list), max(max(n_list), 1)
    x1 = np.zeros((B, n_max, 2)); x2 = np.zeros((B, n_max, 2))
    models = np.zeros((B, 12))
    rng = np.random.default_rng(first + kind)
    for i, n in enumerate(n_list):
        p = make_pair(first + i, max(n, 8))
        x1[i, :n], x2[i, :n] = p["x1"][:n], p["x2"][:n]
        models[i] = start_model(kind, p, start.get(n, "perturbed"), rng)
        if kind == cm.SEVEN and not np.isnan(models[i][0]):
            assert singular_value_gap(models[i][:9]) > 1e-3, (i, n)
    return dict(x1=x1, x2=x2, n=np.array(n_list, dtype=np.int32), models=models, cams=cameras(kind), pp=PP)


EXACT_N = 40  # records per pair of exact_inlier_batch


@functools.lru_cache(maxsize=None)
def exact_inlier_batch(kind, counts, first=88000):
    """from_models_cases.exact_inlier_batch for the baselines: one noise-free pair per entry of `counts` with c records that the pair's ground truth
    counts as inliers (the yardstick's own mask picks them), the others gross outliers (the second image's point drawn anew until the yardstick
    counts none of them — the 7-point kind's threshold moves with the points, so the mask is taken afresh each time), and the start model is that
    ground truth: a model with exactly c inliers, all exact.  The 5-point kind's second image is rescaled to its PINHOLE camera's two focals."""
    B, N = len(counts), EXACT_N
    x1 = np.zeros((B, N, 2)); x2 = np.zeros((B, N, 2))
    models = np.zeros((B, 12))
    rng = np.random.default_rng(first + kind)
    ro, bo = oracle_options("HUBER")  # (stages = 0: the loss is not looked at)
    cams = cameras(kind)
    c1, c2 = oracle_cams(dict(cams=cams))
    for i, c in enumerate(counts):
        p = synth.make_pair(first + i, N, f1=F, f2=F, pp=PP, noise_px=0.0, outlier_frac=0.0)
        m = start_model(kind, p, "exact", rng)
        a1, a2 = p["x1"], p["x2"].copy()
        if kind == cm.FIVE:
            a2 = (a2 - PP) / F * np.array(cams[1][1][:2]) + PP
        mask = lambda a2: np.asarray(cm.refine_from_model_classic(kind, a1, a2, m, ro, bo, 0, c1, c2, PP)["mask"], dtype=bool)
        assert mask(a2).all(), (kind, i)  # noise-free: every record fits the ground truth
        lo, hi = a2.min(axis=0), a2.max(axis=0)
        redo = np.arange(N) >= c
        for _ in range(50):
            a2[redo] = rng.uniform(lo, hi, (int(redo.sum()), 2))
            redo = mask(a2) & (np.arange(N) >= c)
            if not redo.any():
                break
        assert not redo.any() and mask(a2)[:c].all(), (kind, i)
        x1[i], x2[i], models[i] = a1, a2, m
    return dict(x1=x1, x2=x2, n=np.full(B, N, dtype=np.int32), models=models, cams=cams, pp=PP)


def exact_inlier_yardstick(kind, loss, stages, counts):
    b = exact_inlier_batch(kind, counts)
    ro, bo = oracle_options(loss)
    c1, c2 = oracle_cams(b)
    return [cm.refine_from_model_classic(kind, b["x1"][i], b["x2"][i], b["models"][i], ro, bo, stages, c1, c2, b["pp"]) for i in range(len(counts))]


def oracle_options(loss, max_iterations=0, min_iterations=0, score_initial=False, seed=3):
    return (po.ransac_opt(max_iterations=max_iterations, min_iterations=min_iterations, max_epipolar_error=THR, seed=seed, score_initial_model=score_initial),
            po.bundle_opt(max_iterations=100, loss_type=LOSSES[loss], loss_scale=1.0, gradient_tol=1e-10))


def library_options(loss, capi, max_iterations=0, min_iterations=0, score_initial=False, seed=3):
    return (capi.ransac_opt_from_dict(dict(max_epipolar_error=THR, max_iterations=max_iterations, min_iterations=min_iterations, seed=seed,
                                           score_initial_model=score_initial)), capi.bundle_opt_from_dict({"loss_type": loss}))


def oracle_cams(b):
    return (po.cam_flat(*b["cams"][0]), po.cam_flat(*b["cams"][1])) if b["cams"] else (None, None)


def camera_records(kind, b, capi, B=None):
    """(cam1, cam2) as [B] CAMERA_DTYPE arrays: the cameras (5-point), the principal point in params[0..1] (6-point), or (None, None)"""
    B = len(b["n"]) if B is None else B
    if kind == cm.SEVEN:
        return None, None
    if kind == cm.SIX:
        rec = np.zeros(B, dtype=capi.CAMERA_DTYPE)
        rec["params"][:, 0], rec["params"][:, 1] = b["pp"]
        return rec, rec
    out = []
    for mid, params in b["cams"]:
        rec = np.zeros(B, dtype=capi.CAMERA_DTYPE)
        rec["model_id"] = mid
        rec["params"][:, :len(params)] = params
        out.append(rec)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def yardstick(kind, loss, stages, **kw):
    """the yardstick's answer for every pair of batch(kind, **kw): a list of refine_from_model_classic dicts"""
    b = batch(kind, **kw)
    ro, bo = oracle_options(loss)
    c1, c2 = oracle_cams(b)
    return [cm.refine_from_model_classic(kind, b["x1"][i, :n], b["x2"][i, :n], b["models"][i], ro, bo, stages, c1, c2, b["pp"]) for i, n in enumerate(b["n"])]


@functools.lru_cache(maxsize=None)
def prior_yardstick(kind, loss, max_iterations, min_iterations, with_prior=True, score_initial=False, **kw):
    """estimate_from_prior_classic for every pair of batch(kind, **kw); with_prior=False: the prior-free run"""
    b = batch(kind, **kw)
    ro, bo = oracle_options(loss, max_iterations, min_iterations, score_initial)
    c1, c2 = oracle_cams(b)
    return [cm.estimate_from_prior_classic(kind, b["x1"][i, :n], b["x2"][i, :n], ro, bo, b["models"][i] if with_prior else None, c1, c2, b["pp"])
            for i, n in enumerate(b["n"])]


def prior_sensitivity(kind, loss, max_iterations, min_iterations, n_limit=8, rel=1e-13, trials=3):
    """how far the yardstick's own answer moves (model_diff) when the coordinates of a pair of at most n_limit records are perturbed by `rel`
    relative: {n: the largest move over `trials` perturbations}.  A model compared at 1e-6 has to stand still under it."""
    b = batch(kind)
    ro, bo = oracle_options(loss, max_iterations, min_iterations)
    c1, c2 = oracle_cams(b)
    rng = np.random.default_rng(1)
    out = {}
    for i, n in enumerate(b["n"]):
        if n < cm.K_OF[kind] or n > n_limit:
            continue
        x1, x2 = b["x1"][i, :n], b["x2"][i, :n]
        r0 = cm.estimate_from_prior_classic(kind, x1, x2, ro, bo, b["models"][i], c1, c2, b["pp"])
        out[int(n)] = max(model_diff(kind, cm.estimate_from_prior_classic(kind, x1 * (1.0 + rel * rng.uniform(-1, 1, x1.shape)), x2 * (1.0 + rel * rng.uniform(-1, 1, x2.shape)),
                                                                          ro, bo, b["models"][i], c1, c2, b["pp"])["model"], r0["model"]) for _ in range(trials))
    return out


def exact_fits(kind, loss):
    """{how many minimal models the solver returns per sample} over the first samples of the batch's pair of exactly K records (every sample is the
    same K records in another order): more than one model means several exact fits, whose order by score is the rounding of zero residuals"""
    b = batch(kind)
    K = cm.K_OF[kind]
    i = list(b["n"]).index(K)
    ro, bo = oracle_options(loss)
    c1, c2 = oracle_cams(b)
    p = cm.prep(kind, b["x1"][i, :K], b["x2"][i, :K], ro, bo, c1, c2, b["pp"])
    return {len(cm.generate_models(kind, p["a1"], p["a2"], s)) for s in cm.draw_samples_k(3, K, K, 8)}


def sampson_sq(kind, m, p):
    """squared Sampson residuals of the normalised model m over the prepared pair p (classic_models_ref.prep)"""
    Fm = cm.matrix(kind, m)
    h1, h2 = np.c_[p["a1"], np.ones(len(p["a1"]))], np.c_[p["a2"], np.ones(len(p["a2"]))]
    Fx1, Ftx2 = h1 @ Fm.T, h2 @ Fm
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sum(h2 * Fx1, axis=1) ** 2 / (Fx1[:, 0] ** 2 + Fx1[:, 1] ** 2 + Ftx2[:, 0] ** 2 + Ftx2[:, 1] ** 2)


def threshold_margin(kind, r):
    """from_models_cases.threshold_margin's rule: smallest relative distance of a squared residual of the model that entered the inlier-only
    refinement from the squared threshold (inf: no pair, no model)"""
    if r.get("entered") is None or np.isnan(r["entered"][0]):
        return np.inf
    r2 = sampson_sq(kind, r["entered"], r["prep"])
    r2 = r2[np.isfinite(r2)]
    return float(np.min(np.abs(r2 / r["prep"]["sq_thr"] - 1.0))) if len(r2) else np.inf


def branches(kind, loss, **kw):
    """which branches of mdrp_refine_classic's definition the yardstick takes over the batch: a set of names"""
    b = batch(kind, **kw)
    seen = set()
    full, lo_only = yardstick(kind, loss, 3, **kw), yardstick(kind, loss, cm.STAGE_LO, **kw)
    for i, n in enumerate(b["n"]):
        if n < cm.K_OF[kind]:
            seen.add("n<K")
            continue
        if np.isnan(b["models"][i][0]):
            seen.add("nan")
            continue
        adopted = lo_only[i]["model_score"] < lo_only[i]["initial_score"]
        seen.add("lo_adopted" if adopted else "lo_not_adopted")
        if not lo_only[i]["lo_ran"]:
            seen.add("lo_skipped")
        if full[i]["num_inliers"] <= cm.K_OF[kind]:
            seen.add("inliers_skipped")
            assert full[i]["refinements"] == 1
        else:
            seen.add("inliers_run")
    return seen


def model_diff(kind, a, b):
    """the existing classic tests' comparison: q up to sign and the DIRECTION of t (|t| is a gauge of the 5-parameter LM), the focal relative; F up to
    sign and scale"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    if kind == cm.SEVEN:
        x, y = a[:9] / np.linalg.norm(a[:9]), b[:9] / np.linalg.norm(b[:9])
        return float(min(np.abs(x - y).max(), np.abs(x + y).max()))
    dq = min(np.abs(a[:4] - b[:4]).max(), np.abs(a[:4] + b[:4]).max())
    na, nb = np.linalg.norm(a[4:7]), np.linalg.norm(b[4:7])
    if na == 0.0 or nb == 0.0:  # (the identity pose, where no LM moved it: there is no direction)
        d = dq + np.abs(a[4:7] - b[4:7]).max()
    else:
        d = dq + np.abs(a[4:7] / na - b[4:7] / nb).max()
    if kind == cm.SIX:
        d += abs(a[10] - b[10]) / abs(b[10])
    return float(d)
