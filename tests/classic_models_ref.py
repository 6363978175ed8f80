"""Yardstick of mdrp_refine_classic and mdrp_estimate_classic_prior (include/mdrp_classic_models.h): the definition, in NumPy over
the CPU oracle's pieces.  A helper, not a test.

prep restates orc_estimate_classic's normalisation (oracle/orc_classic.c); refine_model restates c_refine_model; ransac_from_prior_classic restates the
loop of orc_ransac_classic with ONE difference: a prior is the initial model of the `pending_initial` pass and is NOT reset.  Without a prior (None, or
a NaN first double) it is orc_ransac_classic, score_initial_model included.  Scoring, inlier selection, the minimal solvers, the sampler's draws and
the LM are the oracle's own functions."""
import ctypes as C
import math
import sys

import numpy as np

from oracle import pyorc as po
from prior_ref import f64_to_u64_x86

STAGE_LO, STAGE_INLIERS = 1, 2
DBL_MAX = sys.float_info.max
FIVE, SIX, SEVEN = 3, 4, 5
K_OF = {FIVE: 5, SIX: 6, SEVEN: 7}


def _focal(cam):
    return 0.5 * (cam[2] + cam[3]) if int(cam[0]) == 1 else cam[2]


def _unproject(cam, x):
    if int(cam[0]) == 1:
        return (x - cam[4:6]) / cam[2:4]
    return (x - cam[3:5]) / cam[2]


def prep(kind, x1, x2, ropt, bopt, cam1=None, cam2=None, pp=(0.0, 0.0)):
    """normalised coordinates and the estimator's thresholds: dict(a1, a2, norm, c1, c2, eps, sq_thr, final_loss_scale)"""
    x1, x2 = po.f64(x1).reshape(-1, 2), po.f64(x2).reshape(-1, 2)
    n = len(x1)
    norm, c1, c2 = 1.0, np.zeros(2), np.zeros(2)
    if kind == FIVE:
        k1, k2 = po.f64(cam1), po.f64(cam2)
        a1, a2 = _unproject(k1, x1), _unproject(k2, x2)
        k = 0.5 * (1.0 / _focal(k1) + 1.0 / _focal(k2))
        eps, final_ls = ropt.max_epipolar_error * k, bopt.loss_scale * k
    else:
        if kind == SEVEN:
            for i in range(n):  # (the oracle's summation order)
                c1 = c1 + x1[i]
                c2 = c2 + x2[i]
            if n > 0:
                c1, c2 = c1 / n, c2 / n
        else:
            c1 = c2 = po.f64(pp).copy()
        a1, a2 = x1 - c1, x2 - c2
        acc = 0.0
        for i in range(n):
            acc += np.sqrt(a1[i, 0] * a1[i, 0] + a1[i, 1] * a1[i, 1]) + np.sqrt(a2[i, 0] * a2[i, 0] + a2[i, 1] * a2[i, 1])
        norm = acc / (np.sqrt(2.0) * max(n, 1))
        a1, a2 = a1 / norm, a2 / norm
        eps, final_ls = ropt.max_epipolar_error / norm, bopt.loss_scale / norm
    return dict(a1=np.ascontiguousarray(a1), a2=np.ascontiguousarray(a2), norm=float(norm), c1=c1, c2=c2, eps=float(eps), sq_thr=float(eps) * float(eps),
                final_loss_scale=float(final_ls))


def matrix(kind, m):
    """the 3 x 3 matrix the Sampson error of model m is taken from (normalised coordinates)"""
    if kind == FIVE:
        return po.essential(m)
    if kind == SIX:
        return po.fundamental(m)
    return po.f64(m)[:9].reshape(3, 3).copy()


def score(kind, m, p, thr=None):
    thr = p["sq_thr"] if thr is None else thr
    if kind == FIVE:
        return po.msac_pose(m, p["a1"], p["a2"], thr)
    return po.msac_F(matrix(kind, m), p["a1"], p["a2"], thr)


def inliers(kind, m, p, thr=None):
    thr = p["sq_thr"] if thr is None else thr
    if kind == FIVE:
        return po.inliers_pose(m, p["a1"], p["a2"], thr)
    return po.inliers_F(matrix(kind, m), p["a1"], p["a2"], thr)


def refine_model(kind, m, p):
    """the estimator's LO step (c_refine_model): (model, whether its LM ran)"""
    lo = po.bundle_opt(max_iterations=25, loss_type=1, loss_scale=p["eps"], gradient_tol=1e-10, step_tol=1e-8, initial_lambda=1e-3, min_lambda=1e-10,
                       max_lambda=1e10)
    if kind == SEVEN:
        return po.refine_classic(kind, p["a1"], p["a2"], m, lo)[0], True
    k = inliers(kind, m, p, 5.0 * p["sq_thr"]).astype(bool)
    if int(k.sum()) > K_OF[kind]:
        return po.refine_classic(kind, p["a1"][k], p["a2"][k], m, lo)[0], True
    return po.f64(m).copy(), False


def final_refine(kind, m, mask, p, bopt):
    k = mask.astype(bool)
    fo = po.bundle_opt(bopt.max_iterations, bopt.loss_type, p["final_loss_scale"], bopt.gradient_tol, bopt.step_tol, bopt.initial_lambda, bopt.min_lambda,
                       bopt.max_lambda)
    return po.refine_classic(kind, p["a1"][k], p["a2"][k], m, fo)[0]


def _congruence(F, T1, T2):
    """T2' (F T1), both products accumulated over the inner index in ascending order (orc_estimate_classic's loops)"""
    M, O = np.zeros(9), np.zeros(9)
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s += F[3 * i + k] * T1[3 * k + j]
            M[3 * i + j] = s
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s += T2[3 * k + i] * M[3 * k + j]
            O[3 * i + j] = s
    return O


def to_estimator_units(kind, model, p, space=0):
    """the caller's model in the estimator's units (the header's conversion); space 1: as it stands"""
    m = po.f64(model).copy()
    if space == 0 and kind == SIX:
        m[10:12] = m[10:12] / p["norm"]
    if space == 0 and kind == SEVEN:
        s = p["norm"]
        T1 = [s, 0, p["c1"][0], 0, s, p["c1"][1], 0, 0, 1]
        T2 = [s, 0, p["c2"][0], 0, s, p["c2"][1], 0, 0, 1]
        m[:9] = _congruence(m[:9], T1, T2)
    return m


def to_caller_units(kind, model, p):
    """the estimator's way out: f * norm; F <- T2' F T1 with unit Frobenius norm"""
    m = po.f64(model).copy()
    if kind == SIX:
        m[10:12] = m[10:12] * p["norm"]
    if kind == SEVEN:
        s = p["norm"]
        T1 = [1 / s, 0, -p["c1"][0] / s, 0, 1 / s, -p["c1"][1] / s, 0, 0, 1]
        T2 = [1 / s, 0, -p["c2"][0] / s, 0, 1 / s, -p["c2"][1] / s, 0, 0, 1]
        O = _congruence(m[:9], T1, T2)
        nrm = 0.0
        for v in O:
            nrm += v * v
        m[:9] = O / np.sqrt(nrm)
    return m


def refine_from_model_classic(kind, x1, x2, model, ropt, bopt, stages, cam1=None, cam2=None, pp=(0.0, 0.0)):
    """dict(model, model_score, num_inliers, inlier_ratio, mask, refinements, initial_score, initial_inliers, entered: the normalised model that
    entered stage INLIERS, prep, lo_ran: whether stage LO's LM ran (None: no stage LO))"""
    m0 = po.f64(model).copy()
    n = len(po.f64(x1).reshape(-1, 2))
    K = K_OF[kind]
    if n < K:
        return dict(model=m0, model_score=DBL_MAX, num_inliers=0, inlier_ratio=0.0, mask=np.zeros(n, np.uint8), refinements=0, initial_score=DBL_MAX,
                    initial_inliers=0, entered=None, prep=None, lo_ran=None)
    p = prep(kind, x1, x2, ropt, bopt, cam1, cam2, pp)
    if np.isnan(m0[0]):  # no model: no inliers, n * threshold^2
        s0 = p["sq_thr"] * n
        return dict(model=m0, model_score=s0, num_inliers=0, inlier_ratio=0.0, mask=np.zeros(n, np.uint8), refinements=0, initial_score=s0,
                    initial_inliers=0, entered=None, prep=p, lo_ran=None)
    m = to_estimator_units(kind, m0, p)
    s, c = score(kind, m, p)
    s0, c0 = s, c
    refinements, lo_ran = 0, None
    if stages & STAGE_LO:
        m1, lo_ran = refine_model(kind, m, p)
        refinements += 1
        s1, c1 = score(kind, m1, p)
        if s1 < s:
            m, s, c = m1, s1, c1
    mask = inliers(kind, m, p)
    entered = m.copy()
    if (stages & STAGE_INLIERS) and c > K:
        m = final_refine(kind, m, mask, p, bopt)
        refinements += 1
    m = to_caller_units(kind, m, p) if refinements else m0.copy()  # no stage ran: the caller's record, bit for bit
    return dict(model=m, model_score=s, num_inliers=int(c), inlier_ratio=c / n, mask=mask, refinements=refinements, initial_score=s0, initial_inliers=int(c0),
                entered=entered, prep=p, lo_ran=lo_ran)


# ---------------------------------------------------------------------------------------------------------------- the search
def draw_samples_k(seed, n, K, count):
    """draw_sample_k of orc_classic.c over orc_random_int: (count, K) record indices"""
    fn = po.lib().orc_random_int
    fn.restype = C.c_int32
    st = C.c_uint64(int(seed))
    out = np.zeros((count, K), dtype=np.int64)
    for r in range(count):
        for i in range(K):
            while True:
                v = (int(fn(C.byref(st))) & (2 ** 64 - 1)) % n  # (uint64_t)(int64_t)r % n
                if all(out[r, j] != v for j in range(i)):
                    break
            out[r, i] = v
    return out


def generate_models(kind, x1, x2, s):
    """the minimal models of sample s (K record indices): c_generate_models"""
    a, b = x1[s], x2[s]
    n1, n2 = np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + 1.0), np.sqrt(b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1] + 1.0)
    x1h = np.c_[a[:, 0] / n1, a[:, 1] / n1, 1.0 / n1].reshape(-1)
    x2h = np.c_[b[:, 0] / n2, b[:, 1] / n2, 1.0 / n2].reshape(-1)
    if kind == FIVE:
        return po.relpose_5pt(x1h, x2h)
    if kind == SIX:
        return po.relpose_6pt(x1h, x2h)
    Fs = po.relpose_7pt(x1h, x2h).reshape(-1, 9)
    out = np.zeros((len(Fs), po.MODEL_W))
    out[:, :9] = Fs
    return out


def dyn_max_iter(ratio, K, ropt, log_prob_missing):
    if ratio >= 0.9999:
        return int(ropt.min_iterations)
    if ratio <= 0.0001:
        return int(ropt.max_iterations)
    prob_outlier = 1.0 - math.pow(ratio, float(K))  # (libm's pow and log, as the oracle calls them)
    with np.errstate(all="ignore"):  # log(1) = 0: -inf, which the conversion maps as the reference's x86-64 build does
        return f64_to_u64_x86(np.ceil(np.float64(log_prob_missing) / np.float64(math.log(prob_outlier)) * np.float64(ropt.dyn_num_trials_mult)))


def ransac_from_prior_classic(kind, x1, x2, ropt, prior=None):
    """x1, x2 normalised, ropt in normalised units (as orc_estimate_classic hands them to orc_ransac_classic), prior a 12-wide model in normalised
    units or None.  dict(model, refinements, iterations, num_inliers, inlier_ratio, model_score, mask, branch: 'n<K' | 'none' | 'nan' | 'lo_adopted' |
    'lo_not_adopted' | 'unscored', lo_ran: whether the prior's LM ran, best_min: (count, score) before iteration 0)"""
    x1, x2 = po.f64(x1).reshape(-1, 2), po.f64(x2).reshape(-1, 2)
    n, K = len(x1), K_OF[kind]
    out = dict(model=po.classic_blob(kind), refinements=0, iterations=0, num_inliers=0, inlier_ratio=0.0, model_score=DBL_MAX, mask=np.zeros(n, np.uint8),
               branch="n<K", lo_ran=None, best_min=(0, DBL_MAX))
    if n < K:
        return out
    eps = ropt.max_epipolar_error
    p = dict(a1=x1, a2=x2, eps=eps, sq_thr=eps * eps)
    have_prior = prior is not None and not np.isnan(po.f64(prior)[0])
    best = po.f64(prior).copy() if have_prior else po.classic_blob(kind)  # (the reference resets the caller's model; a prior is not reset)
    pending = True if have_prior else bool(ropt.score_initial_model)  # a pair with a prior ignores score_initial_model
    out["branch"] = "none" if prior is None else ("nan" if not have_prior else "unscored")
    samples = draw_samples_k(ropt.seed, n, K, int(ropt.max_iterations))
    best_min_cnt, best_min_score = 0, DBL_MAX
    dyn = int(ropt.max_iterations)
    log_prob_missing = math.log(1.0 - ropt.success_prob)
    model_score, num_inliers, inlier_ratio, refinements, it = DBL_MAX, 0, 0.0, 0, 0
    while True:
        if not pending and it >= ropt.max_iterations:
            break
        models = [best.copy()] if pending else generate_models(kind, x1, x2, samples[it])
        best_ind = -1
        for i, m in enumerate(models):
            s, c = score(kind, m, p)
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
            refined, ran = refine_model(kind, models[best_ind], p)
            refinements += 1
            s, c = score(kind, refined, p)
            adopted = s < model_score
            if adopted:
                model_score, num_inliers, best = s, c, refined
            if pending and have_prior:
                out["branch"] = "lo_adopted" if adopted else "lo_not_adopted"
                out["lo_ran"] = ran
            inlier_ratio = num_inliers / n
            dyn = dyn_max_iter(inlier_ratio, K, ropt, log_prob_missing)
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
    refined, _ = refine_model(kind, best, p)  # the closing LO: adopts the model and its count, not the score / ratio
    refinements += 1
    s, c = score(kind, refined, p)
    if s < model_score:
        best, num_inliers = refined, c
    out.update(model=best, refinements=refinements, iterations=it, num_inliers=int(num_inliers), inlier_ratio=inlier_ratio, model_score=model_score,
               mask=inliers(kind, best, p))
    return out


def normalised_options(ropt, p):
    return po.ransac_opt(ropt.max_iterations, ropt.min_iterations, ropt.dyn_num_trials_mult, ropt.success_prob, ropt.max_reproj_error, p["eps"], ropt.seed,
                         False, 1.0, ropt.score_initial_model)


def estimate_from_prior_classic(kind, x1, x2, ropt, bopt, prior=None, cam1=None, cam2=None, pp=(0.0, 0.0), prior_space=0):
    """the caller's units: pixels, the caller's thresholds, a prior as the estimator returns it.  The dict of ransac_from_prior_classic for the whole
    estimator (orc_estimate_classic's prep in front, its tail behind)."""
    x1, x2 = po.f64(x1).reshape(-1, 2), po.f64(x2).reshape(-1, 2)
    n, K = len(x1), K_OF[kind]
    if n < K:  # the estimators' record: identity model, zero stats; the prior is not read
        return ransac_from_prior_classic(kind, x1, x2, ropt, None)
    p = prep(kind, x1, x2, ropt, bopt, cam1, cam2, pp)
    m0 = None if prior is None else to_estimator_units(kind, prior, p, prior_space)
    r = ransac_from_prior_classic(kind, p["a1"], p["a2"], normalised_options(ropt, p), m0)
    m = r["model"]
    r["entered"] = np.array(m, copy=True)
    if r["num_inliers"] > K:
        m = final_refine(kind, m, r["mask"], p, bopt)
    r["model"] = to_caller_units(kind, m, p)
    r["prep"] = p
    return r
