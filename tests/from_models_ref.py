"""Yardstick of mdrp_refine_batch (include/mdrp.h): the definition, in NumPy over the CPU oracle's pieces.  A helper, not a test.

One pair, one caller-supplied model (12-wide: q t scale shift1 shift2 f1 f2, focals in pixels), the stage flags -> what the estimator does from the
moment RANSAC has picked its winner.  The prep restates orc_estimate (oracle/orc_ransac.c); scoring, inlier selection and the two LMs are the oracle's."""
import sys

import numpy as np

from oracle import pyorc as po

STAGE_LO, STAGE_INLIERS = 1, 2
DBL_MAX = sys.float_info.max


def _focal(cam):
    return 0.5 * (cam[2] + cam[3]) if int(cam[0]) == 1 else cam[2]


def _unproject(cam, x):
    if int(cam[0]) == 1:
        return (x - cam[4:6]) / cam[2:4]
    return (x - cam[3:5]) / cam[2]


def prep(kind, x1, x2, ropt, bopt, cam1=None, cam2=None):
    """normalised coordinates and the estimator's thresholds: dict(a1, a2, norm, eps, rep, sq_thr, scale_reproj, ws, lo_loss_scale, final_loss_scale)"""
    x1, x2 = po.f64(x1).reshape(-1, 2), po.f64(x2).reshape(-1, 2)
    n = len(x1)
    ws = float(np.float32(ropt.weight_sampson))
    ws = ws if ws > 0.0 else 0.0
    if kind == po.CALIB:
        c1, c2 = po.f64(cam1), po.f64(cam2)
        a1, a2, norm = _unproject(c1, x1), _unproject(c2, x2), 1.0
        k = 0.5 * (1.0 / _focal(c1) + 1.0 / _focal(c2))
        eps, rep = ropt.max_epipolar_error * k, ropt.max_reproj_error * k
        final_ls = (1.0 / _focal(c2) + 1.0 / _focal(c1)) * (ropt.max_epipolar_error * 0.25)
    else:
        acc = 0.0
        for i in range(n):  # (the oracle's summation order)
            acc += np.sqrt(x1[i, 0] * x1[i, 0] + x1[i, 1] * x1[i, 1]) + np.sqrt(x2[i, 0] * x2[i, 0] + x2[i, 1] * x2[i, 1])
        norm = acc / (np.sqrt(2.0) * max(n, 1))
        a1, a2 = x1 / norm, x2 / norm
        eps, rep = ropt.max_epipolar_error / norm, ropt.max_reproj_error / norm
        final_ls = bopt.loss_scale / norm
    return dict(a1=np.ascontiguousarray(a1), a2=np.ascontiguousarray(a2), norm=norm, eps=eps, rep=rep, sq_thr=eps * eps,
                scale_reproj=(eps * eps) / (rep * rep) if rep > 0.0 else 0.0, ws=ws, lo_loss_scale=1.0 if kind == po.VARYING else eps, final_loss_scale=final_ls)


def score(kind, m, p):
    if kind == po.CALIB:
        return po.msac_pose(m, p["a1"], p["a2"], p["sq_thr"])
    return po.msac_F(po.fundamental(m), p["a1"], p["a2"], p["sq_thr"])


def inliers(kind, m, p):
    if kind == po.CALIB:
        return po.inliers_pose(m, p["a1"], p["a2"], p["sq_thr"])
    return po.inliers_F(po.fundamental(m), p["a1"], p["a2"], p["sq_thr"])


def refine_from_model(kind, x1, x2, d1, d2, model, ropt, bopt, stages, cam1=None, cam2=None):
    """dict(model, model_score, num_inliers, inlier_ratio, mask, refinements, initial_score, initial_inliers, entered: the normalised model that
    entered stage INLIERS, prep)"""
    m0 = po.f64(model).copy()
    n = len(po.f64(x1).reshape(-1, 2))
    if n < 3:
        return dict(model=m0, model_score=DBL_MAX, num_inliers=0, inlier_ratio=0.0, mask=np.zeros(n, np.uint8), refinements=0, initial_score=DBL_MAX,
                    initial_inliers=0, entered=None, prep=None)
    d1, d2 = po.f64(d1), po.f64(d2)
    p = prep(kind, x1, x2, ropt, bopt, cam1, cam2)
    es = kind == po.CALIB and bool(ropt.estimate_shift)
    m = m0.copy()
    if kind != po.CALIB:
        m[10:12] = m[10:12] / p["norm"]
    s, c = score(kind, m, p)
    s0, c0 = s, c
    refinements = 0
    if (stages & STAGE_LO) and not np.isnan(m[0]):
        lo = po.bundle_opt(max_iterations=25, loss_type=1, loss_scale=p["lo_loss_scale"], gradient_tol=1e-10, step_tol=1e-8, initial_lambda=1e-3,
                           min_lambda=1e-10, max_lambda=1e10)
        m1, _ = po.refine(kind, p["a1"], p["a2"], d1, d2, m, p["scale_reproj"], p["ws"], lo, es)
        refinements += 1
        s1, c1 = score(kind, m1, p)
        if s1 < s:
            m, s, c = m1, s1, c1
    mask = inliers(kind, m, p)
    entered = m.copy()
    if (stages & STAGE_INLIERS) and c > (7 if kind == po.VARYING else 3):
        k = mask.astype(bool)
        fo = po.bundle_opt(bopt.max_iterations, bopt.loss_type, p["final_loss_scale"], bopt.gradient_tol, bopt.step_tol, bopt.initial_lambda, bopt.min_lambda,
                           bopt.max_lambda)
        m, _ = po.refine(kind, p["a1"][k], p["a2"][k], d1[k], d2[k], m, p["scale_reproj"], p["ws"], fo, es)
        refinements += 1
    if refinements == 0:
        m = m0.copy()  # no LM ran: the caller's model, bit for bit
    elif kind != po.CALIB:
        m[10:12] = m[10:12] * p["norm"]
    return dict(model=m, model_score=s, num_inliers=int(c), inlier_ratio=c / n, mask=mask, refinements=refinements, initial_score=s0, initial_inliers=int(c0),
                entered=entered, prep=p)
