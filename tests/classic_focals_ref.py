"""The varying-focal baseline's tail in NumPy (include/mdrp_classic_focals.h): the yardstick of tests/test_classic_focals_host.py and
tests/test_gpu_classic_focals.py.

    focals(F, pp1, pp2)            the closed form of poselib::focals_from_fundamental, NaN where f^2 < 0
    essential(F, f1, f2, pp1, pp2) E = K2' F K1, not rescaled
    candidates(E)                  the four poses of orc_motion_from_essential with npts = 0: (R1, t), (R1, -t), (R2, -t), (R2, t)
    focal_pose(...)                the 128-byte record: votes of the pair's kept records by check_cheirality at minimum depth 0 (restated here),
                                   winner, status — and the smallest |depth| any (candidate, record) test came to, which the vote cases must keep
                                   above MARGIN so that the integers do not depend on the last bits of the arithmetic
"""
import ctypes as C

import numpy as np

from oracle import pyorc as po

NO_MODEL, F1_NOT_REAL, F2_NOT_REAL, NO_VOTERS = 1, 2, 4, 8
MIN_RECORDS = 7
MARGIN = 1e-9
II = np.diag([1.0, 1.0, 0.0])


def null_cross(M):
    """null vector of a rank-2 3 x 3 matrix: the largest of the cross products of two of its rows (the first one on ties); not normalised"""
    c = [np.cross(M[0], M[1]), np.cross(M[0], M[2]), np.cross(M[1], M[2])]
    return c[int(np.argmax([v @ v for v in c]))]


def null_svd(M):
    return np.linalg.svd(M)[2][-1]


def _skew(e):
    return np.array([[0.0, -e[2], e[1]], [e[2], 0.0, -e[0]], [-e[1], e[0], 0.0]])


def focals_squared(F, pp1, pp2, null=null_cross):
    F = np.asarray(F, dtype=np.float64).reshape(3, 3)
    p1, p2 = np.r_[np.asarray(pp1, float), 1.0], np.r_[np.asarray(pp2, float), 1.0]
    e1, e2 = null(F), null(F.T)  # F e1 = 0, F' e2 = 0
    with np.errstate(all="ignore"):
        f1 = -(p2 @ _skew(e2) @ II @ F @ p1) * (p1 @ F.T @ p2) / (p2 @ _skew(e2) @ II @ F @ II @ F.T @ p2)
        f2 = -(p1 @ _skew(e1) @ II @ F.T @ p2) * (p2 @ F @ p1) / (p1 @ _skew(e1) @ II @ F.T @ II @ F @ p1)
    return f1, f2


def focals(F, pp1=(0.0, 0.0), pp2=(0.0, 0.0), null=null_cross):
    with np.errstate(all="ignore"):
        return tuple(np.sqrt(v) if v >= 0 else np.nan for v in focals_squared(F, pp1, pp2, null))


def essential(F, f1, f2, pp1, pp2):
    F = np.asarray(F, dtype=np.float64).reshape(3, 3)
    M = np.empty((3, 3))
    M[:, 0] = F[:, 0] * f1
    M[:, 1] = F[:, 1] * f1
    M[:, 2] = F[:, 0] * pp1[0] + F[:, 1] * pp1[1] + F[:, 2]
    E = np.empty((3, 3))
    E[0] = f2 * M[0]
    E[1] = f2 * M[1]
    E[2] = pp2[0] * M[0] + pp2[1] * M[1] + M[2]
    return E


def candidates(E):
    out = np.zeros((4, po.MODEL_W))
    Ef = po.f64(np.asarray(E).reshape(-1))
    n = po.lib().orc_motion_from_essential(po._p(Ef), None, None, C.c_int(0), po._p(out))
    assert n == 4
    return out


def depths(q, t, b1, b2):
    """check_cheirality's two depths for unit bearings b1, b2 [n][3]: the test is l1 > 0 and l2 > 0 at minimum depth 0"""
    u = b1 @ po.quat_to_rotmat(q).T
    a = -np.sum(u * b2, axis=1)
    c1 = -(u @ t)
    c2 = b2 @ t
    return c1 - a * c2, -a * c1 + c2


def identity_model(f1=np.nan, f2=np.nan):
    m = np.zeros(po.MODEL_W)
    m[0] = 1.0; m[7] = 1.0; m[10] = f1; m[11] = f2
    return m


def focal_pose(F, x1, x2, n, mask=None, pp1=(0.0, 0.0), pp2=(0.0, 0.0)):
    """dict(model [12], votes [4], voters, winner, status, cand [4][12] or None, margin)"""
    F = np.asarray(F, dtype=np.float64).reshape(-1)[:9]
    pp1, pp2 = np.asarray(pp1, float), np.asarray(pp2, float)
    rec = dict(model=identity_model(), votes=np.zeros(4, np.int32), voters=0, winner=-1, status=0, cand=None, margin=np.inf)
    if np.isnan(F[0]) or n < MIN_RECORDS:
        rec["status"] = NO_MODEL
        return rec
    f1, f2 = focals(F, pp1, pp2)
    rec["model"] = identity_model(f1, f2)
    rec["status"] = (F1_NOT_REAL if np.isnan(f1) else 0) | (F2_NOT_REAL if np.isnan(f2) else 0)
    if rec["status"]:
        return rec
    cand = candidates(essential(F, f1, f2, pp1, pp2))
    rec["cand"] = cand
    keep = np.ones(n, bool) if mask is None else np.asarray(mask[:n]) != 0
    a1, a2 = np.asarray(x1, float)[:n][keep], np.asarray(x2, float)[:n][keep]
    b1 = np.c_[(a1 - pp1) / f1, np.ones(len(a1))]
    b2 = np.c_[(a2 - pp2) / f2, np.ones(len(a2))]
    b1 /= np.linalg.norm(b1, axis=1, keepdims=True)
    b2 /= np.linalg.norm(b2, axis=1, keepdims=True)
    for c in range(4):
        l1, l2 = depths(cand[c, :4], cand[c, 4:7], b1, b2)
        rec["votes"][c] = int(np.sum((l1 > 0) & (l2 > 0)))
        if len(l1):
            rec["margin"] = min(rec["margin"], float(np.abs(l1).min()), float(np.abs(l2).min()))
    rec["voters"] = int(keep.sum())
    rec["winner"] = int(np.argmax(rec["votes"]))  # the largest count, the first one on ties
    if rec["voters"] == 0:
        rec["status"] = NO_VOTERS
    rec["model"][:7] = cand[rec["winner"], :7]
    return rec


# ---- the generator of the probe: random rank-2 matrices from two cameras with the principal point at the origin and a motion, noise
# entry by entry, the rank restored; the principal points handed to the formula are drawn on their own (an error of some twenty pixels, which is what
# makes f^2 negative for a few per cent of the draws)
def random_F(rng, pp_sigma=20.0):
    """(F [9] row-major with unit Frobenius norm, pp1, pp2)"""
    f1, f2 = rng.uniform(300.0, 2000.0, 2)
    rv = rng.normal(0.0, 0.3, 3)
    th = np.linalg.norm(rv)
    k = rv / th
    K = _skew(k)
    R = np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * K @ K
    t = rng.normal(0.0, 0.5, 3)
    K1, K2 = np.diag([f1, f1, 1.0]), np.diag([f2, f2, 1.0])
    F = np.linalg.inv(K2).T @ _skew(t) @ R @ np.linalg.inv(K1)
    F *= 1.0 + 10.0 ** rng.uniform(-7.0, -3.0) * rng.normal(0.0, 1.0, (3, 3))
    u, s, vt = np.linalg.svd(F)
    F = u @ np.diag([s[0], s[1], 0.0]) @ vt
    pp1, pp2 = rng.normal(0.0, pp_sigma, 2), rng.normal(0.0, pp_sigma, 2)
    return (F / np.linalg.norm(F)).reshape(-1), pp1, pp2
