"""Yardstick of mdrp_estimate_batch_prior (include/mdrp.h): the definition, in NumPy over the CPU oracle's pieces.  A helper, not a test.

ransac_from_prior restates the loop of orc_ransac (oracle/orc_ransac.c) with ONE difference: a prior is the initial model of the `pending_initial` pass
and is NOT reset to the identity.  Without a prior (None, or a NaN q[0]) it is orc_ransac, score_initial_model included.  estimate_from_prior puts
from_models_ref.prep in front and the mask, the inlier-only refinement and the focal un-normalisation behind it: the tail of orc_estimate.  Sampling,
solvers, scoring and the LM are the oracle's own functions."""
import ctypes as C
import sys

import numpy as np

import from_models_ref as fm
from oracle import pyorc as po

DBL_MAX = sys.float_info.max
T63 = 9223372036854775808.0


def f64_to_u64_x86(d):
    """(uint64_t) of a double as the reference's x86-64 build computes it (mdrp_oracle.h orc_f64_to_u64; mdrp_kernels.h f64_to_u64_x86)"""
    d = float(d)
    if d >= T63:
        e = d - T63
        return ((int(e) if e < T63 else 1 << 63) ^ (1 << 63)) & (2 ** 64 - 1)
    if d >= -T63:  # (NaN fails both comparisons)
        return int(d) & (2 ** 64 - 1)
    return 1 << 63


def dyn_max_iter(ratio, ropt, log_prob_missing):
    """ransac<>'s dynamic iteration bound from the inlier ratio (the power as x * x * x, as the library pins it against the reference binary)"""
    if ratio >= 0.9999:
        return int(ropt.min_iterations)
    if ratio <= 0.0001:
        return int(ropt.max_iterations)
    with np.errstate(all="ignore"):
        r = np.float64(ratio)
        prob_outlier = np.float64(1.0) - r * r * r
        return f64_to_u64_x86(np.ceil(log_prob_missing / np.log(prob_outlier) * np.float64(ropt.dyn_num_trials_mult)))


def _p3p_nan(x1h, x2h, d1):
    X = (x1h * d1[:, None]).copy()
    xb = (x2h / np.sqrt((x2h * x2h).sum(axis=1))[:, None]).copy()
    fn = po.lib().orc_p3p_reference_nan
    fn.restype = C.c_int
    return bool(fn(po._p(po.f64(xb.reshape(-1))), po._p(po.f64(X.reshape(-1)))))


def generate_models(kind, es, x1, x2, d1, d2, s):
    """the minimal models of sample s (three record indices): generate_models of orc_ransac.c"""
    x1h, x2h = np.c_[x1[s], np.ones(3)], np.c_[x2[s], np.ones(3)]
    a, b = d1[s].copy(), d2[s].copy()
    if kind == po.CALIB:
        if es:
            return po.solver_calib_shift(x1h.reshape(-1), x2h.reshape(-1), a, b)
        if _p3p_nan(x1h, x2h, a):  # the reference's P3P returns NaN poses there: one stands for the four
            m = np.zeros((1, po.MODEL_W))
            m[0, :8] = np.nan
            m[0, 10:12] = 1.0
            return m
        return po.solver_calib_p3p(x1h.reshape(-1), x2h.reshape(-1), a, b)
    if kind == po.SHARED:
        return po.solver_shared(x1h.reshape(-1), x2h.reshape(-1), a, b)
    return po.solver_varying(x1h.reshape(-1), x2h.reshape(-1), a, b)


def ransac_from_prior(kind, x1, x2, d1, d2, ropt, prior=None):
    """x1, x2 normalised, ropt in normalised units (as orc_estimate hands them to orc_ransac), prior a 12-wide model in normalised units or None.
    dict(model, refinements, iterations, num_inliers, inlier_ratio, model_score, mask, branch: 'n<3' | 'none' | 'nan' | 'lo_adopted' | 'lo_not_adopted' |
    'unscored', best_min: (count, score) before iteration 0)"""
    x1, x2, d1, d2 = po.f64(x1).reshape(-1, 2), po.f64(x2).reshape(-1, 2), po.f64(d1).reshape(-1), po.f64(d2).reshape(-1)
    n = len(x1)
    out = dict(model=po.new_model(), refinements=0, iterations=0, num_inliers=0, inlier_ratio=0.0, model_score=DBL_MAX, mask=np.zeros(n, np.uint8),
               branch="n<3", best_min=(0, DBL_MAX))
    if n < 3:
        return out
    es = kind == po.CALIB and bool(ropt.estimate_shift)
    eps = ropt.max_epipolar_error
    sq_thr = eps * eps
    p = dict(a1=x1, a2=x2, sq_thr=sq_thr)
    scale_reproj = sq_thr / (ropt.max_reproj_error * ropt.max_reproj_error) if ropt.max_reproj_error > 0.0 else 0.0
    lo = po.bundle_opt(max_iterations=25, loss_type=1, loss_scale=1.0 if kind == po.VARYING else eps, gradient_tol=1e-10, step_tol=1e-8,
                       initial_lambda=1e-3, min_lambda=1e-10, max_lambda=1e10)

    def refine_model(m):
        return po.refine(kind, x1, x2, d1, d2, m, scale_reproj, ropt.weight_sampson, lo, es)[0]

    have_prior = prior is not None and not np.isnan(po.f64(prior)[0])
    best = po.f64(prior).copy() if have_prior else po.new_model()  # (the reference resets the caller's model; a prior is not reset)
    pending = True if have_prior else bool(ropt.score_initial_model)  # a pair with a prior ignores score_initial_model
    out["branch"] = "none" if prior is None else ("nan" if not have_prior else "unscored")
    samples = po.draw_samples(int(ropt.seed), n, int(ropt.max_iterations)) if ropt.max_iterations else np.zeros((0, 3), np.int64)
    best_min_cnt, best_min_score = 0, DBL_MAX
    dyn = int(ropt.max_iterations)
    with np.errstate(all="ignore"):
        log_prob_missing = np.log(np.float64(1.0) - np.float64(ropt.success_prob))
    model_score, num_inliers, inlier_ratio, refinements, it = DBL_MAX, 0, 0.0, 0, 0
    while True:
        if not pending and it >= ropt.max_iterations:
            break
        models = [best.copy()] if pending else generate_models(kind, es, x1, x2, d1, d2, samples[it])
        best_ind = -1
        for i, m in enumerate(models):
            s, c = fm.score(kind, m, p)
            more, better = c > best_min_cnt, s < best_min_score
            if more or better:
                if more:
                    best_min_cnt = c
                if better:
                    best_min_score = s
                best_ind = i
                if s < model_score:
                    model_score, best, num_inliers = s, np.array(m, copy=True), c
        if best_ind >= 0:
            refined = refine_model(models[best_ind])
            refinements += 1
            s, c = fm.score(kind, refined, p)
            adopted = s < model_score
            if adopted:
                model_score, num_inliers, best = s, c, refined
            if pending and have_prior:
                out["branch"] = "lo_adopted" if adopted else "lo_not_adopted"
            inlier_ratio = num_inliers / n
            dyn = dyn_max_iter(inlier_ratio, ropt, log_prob_missing)
        if pending:
            pending = False  # not an iteration
            out["best_min"] = (best_min_cnt, best_min_score)
            continue
        it += 1
        if it >= ropt.max_iterations:
            break
        if it <= ropt.min_iterations:
            continue
        if it > dyn:
            break
    refined = refine_model(best)  # the closing LO: adopts the model and its count, not the score / ratio
    refinements += 1
    s, c = fm.score(kind, refined, p)
    if s < model_score:
        best, num_inliers = refined, c
    out.update(model=best, refinements=refinements, iterations=it, num_inliers=int(num_inliers), inlier_ratio=inlier_ratio, model_score=model_score,
               mask=fm.inliers(kind, best, p))
    return out


def estimate_from_prior(kind, x1, x2, d1, d2, ropt, bopt, prior=None, cam1=None, cam2=None):
    """the caller's units: pixels, the caller's thresholds, a prior with focals in pixels.  The dict of ransac_from_prior for the whole estimator."""
    x1, x2 = po.f64(x1).reshape(-1, 2), po.f64(x2).reshape(-1, 2)
    d1, d2 = po.f64(d1).reshape(-1), po.f64(d2).reshape(-1)
    n = len(x1)
    if n < 3:  # the estimators' record: identity model, zero stats; the prior is not read
        return ransac_from_prior(kind, x1, x2, d1, d2, ropt, None)
    p = fm.prep(kind, x1, x2, ropt, bopt, cam1, cam2)
    es = kind == po.CALIB and bool(ropt.estimate_shift)
    ro = po.ransac_opt(ropt.max_iterations, ropt.min_iterations, ropt.dyn_num_trials_mult, ropt.success_prob, p["rep"], p["eps"], ropt.seed, ropt.estimate_shift,
                       p["ws"], ropt.score_initial_model)
    m0 = None
    if prior is not None:
        m0 = po.f64(prior).copy()
        if kind != po.CALIB:
            m0[10:12] = m0[10:12] / p["norm"]
    r = ransac_from_prior(kind, p["a1"], p["a2"], d1, d2, ro, m0)
    m = r["model"]
    if r["num_inliers"] > (7 if kind == po.VARYING else 3):
        k = r["mask"].astype(bool)
        fo = po.bundle_opt(bopt.max_iterations, bopt.loss_type, p["final_loss_scale"], bopt.gradient_tol, bopt.step_tol, bopt.initial_lambda, bopt.min_lambda,
                           bopt.max_lambda)
        m, _ = po.refine(kind, p["a1"][k], p["a2"][k], d1[k], d2[k], m, p["scale_reproj"], p["ws"], fo, es)
    m = np.array(m, copy=True)
    if kind != po.CALIB:
        m[10:12] = m[10:12] * p["norm"]
    r["model"] = m
    r["prep"] = p
    return r
