"""Yardstick of tests/test_gpu_front_stages.py and tests/test_front_stages_host.py: what the stages in front of the sweeps are defined to leave behind,
stated in NumPy (extended precision where a bound is checked) over the CPU oracle's solvers.  A helper, not a test; no device code.

  prep       the comments above k_prep (mdrp_kernels.h) and kc_prep (mdrp_classic.h): unprojection, the sum-of-norms scale, centroids, thresholds
  fragments  bf16_bits / bf16_split (mdrp_math.h) and the lane layout above pack_bf16x8 (mdrp_kernels.h)
  sampler    prosac_ref._draw: K distinct indices by rejection, the uniform draw for any K
  solvers    the oracle's (oracle/pyorc.py) and the host build of the device's (tests/hostmath), on inputs formed from the device's own records
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import prosac_ref
from oracle import pyorc as po

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
SAMPLE_SIZE = {0: 3, 1: 3, 2: 3, 3: 5, 4: 6, 5: 7}
MODEL_SLOTS = {0: 4, 1: 4, 2: 4, 3: 12, 4: 16, 5: 4}
SQRT2 = np.sqrt(LD(2))
assert np.finfo(LD).nmant >= 63, "the bounds below are checked in x87 extended precision"


# ---------------------------------------------------------------------------------------------------------------- prep
def intrinsics(cam):
    """(fx, fy, cx, cy) of a camera record: SIMPLE_PINHOLE {f, cx, cy}, PINHOLE {fx, fy, cx, cy}"""
    p = [float(v) for v in cam["params"]]
    return (p[0], p[1], p[2], p[3]) if int(cam["model_id"]) == 1 else (p[0], p[0], p[1], p[2])


def fsum_ld(terms):
    """the exact sum of extended-precision terms, rounded once: math.fsum over their double heads and tails"""
    terms = np.asarray(terms, dtype=LD).reshape(-1)
    hi = terms.astype(np.float64)
    lo = (terms - hi.astype(LD)).astype(np.float64)
    return LD(math.fsum(hi.tolist())) + LD(math.fsum(lo.tolist()))


def scale_and_centre(kind, x1, x2, cam1):
    """of the scale-normalised kinds (1, 2, 4, 5), over the pair's n records: (centre[4], mean |x|[4]) in extended precision.  The centre is 0
    (kinds 1, 2), the caller's principal point (4) or the centroids (5: fsum / n; the mean magnitude of their terms is what their bound is relative to)"""
    n = len(x1)
    xs = np.concatenate([x1, x2], axis=1).astype(LD)
    cen, mean_abs = np.zeros(4, dtype=LD), np.zeros(4, dtype=LD)
    if kind == 5 and n:
        cen = np.array([fsum_ld(xs[:, q]) / LD(n) for q in range(4)], dtype=LD)
        mean_abs = np.array([fsum_ld(np.abs(xs[:, q])) / LD(n) for q in range(4)], dtype=LD)
    if kind == 4:
        cen = np.array([cam1["params"][0], cam1["params"][1]] * 2, dtype=LD)
    return cen, mean_abs


def norm_of(x1, x2, cen):
    """sum(|x1 - c1| + |x2 - c2|) / (sqrt2 n) in extended precision, about the centre given (the device's own, for the 7-point kind)"""
    n = len(x1)
    d = np.concatenate([x1, x2], axis=1).astype(LD) - np.asarray(cen, dtype=LD)
    terms = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + np.sqrt(d[:, 2] * d[:, 2] + d[:, 3] * d[:, 3])
    return fsum_ld(terms) / (SQRT2 * LD(max(n, 1)))


def sum_bound(n):
    """relative bound of the device's sums (norm, centroids) against the fsum value: a lane adds at most ceil(n / 256) terms, then six shuffle
    levels and three adds; each root carries half an ulp; the quotient by sqrt2 n and the rest stay inside the ten"""
    return (math.ceil(n / 256) + 10) * 2.0 ** -52


def points(kind, x1, x2, cam1, cam2, norm=None, cen=None):
    """pts[:, 0:4] in float64, bit for bit: one subtraction and one IEEE quotient.  Calibrated kinds (0, 3): (x - c) / f per axis; the others:
    (x - cen) / norm with the DEVICE's norm and centre (cen 0 for kinds 1 and 2, where the kernel divides x itself)"""
    xs = np.concatenate([x1, x2], axis=1).astype(np.float64)
    with np.errstate(all="ignore"):
        if kind in (0, 3):
            (fx1, fy1, cx1, cy1), (fx2, fy2, cx2, cy2) = intrinsics(cam1), intrinsics(cam2)
            return (xs - np.array([cx1, cy1, cx2, cy2])) / np.array([fx1, fy1, fx2, fy2])
        if kind in (1, 2):
            return xs / np.float64(norm)
        return (xs - np.asarray(cen, dtype=np.float64)) / np.float64(norm)


def inverse_lengths(p4):
    """pts[:, 4:6] = 1 / sqrt(a^2 + b^2 + 1) of the device's own coordinates, in extended precision"""
    p = np.asarray(p4, dtype=LD)
    return np.stack([1 / np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + 1), 1 / np.sqrt(p[:, 2] * p[:, 2] + p[:, 3] * p[:, 3] + 1)], axis=1)


def state_fields(kind, n, cam1, cam2, norm_dev, ro, bo):
    """{field: (value in extended precision, r)}: every threshold and scale of the pair state as its defining expression, with r the number of
    roundings the kernel's evaluation of it goes through (a factor used twice counts twice); the device must be within r 2^-53 relative.
    Calibrated kinds: k = ((1 / ((fx1 + fy1) / 2) + 1 / ((fx2 + fy2) / 2)) / 2   5 roundings (two sums, two quotients, one sum; halving is exact)
    the others:       k = 1 / norm of the device's own norm                        1 rounding"""
    me, mr, ls = LD(ro["max_epipolar_error"]), LD(ro.get("max_reproj_error", 12.0)), LD(bo.get("loss_scale", 1.0))
    if kind in (0, 3):
        (fx1, fy1, _, _), (fx2, fy2, _, _) = intrinsics(cam1), intrinsics(cam2)
        k, rk = (1 / ((LD(fx1) + LD(fy1)) / 2) + 1 / ((LD(fx2) + LD(fy2)) / 2)) / 2, 5
    else:
        k, rk = 1 / LD(norm_dev), 1
    eps, re_ = me * k, rk + 1                                     # eps = max_epi * k: one product more
    out = {"eps": (eps, re_), "sq_thr": (eps * eps, 2 * re_ + 1)}  # eps * eps: eps twice, one product
    if kind <= 2:
        rep = mr * k                                               # rep = max_reproj * k (re_ roundings); eps^2 / rep^2: (2 re_ + 1) twice, one quotient
        out["scale_reproj"] = (eps * eps / (rep * rep) if rep > 0 else LD(0), 2 * (2 * re_ + 1) + 1)
    else:
        out["scale_reproj"] = (LD(0), 0)
    out["lo_loss_scale"] = (LD(1), 0) if kind == 2 else (eps, re_)
    # calibrated monodepth: (1 / f2m + 1 / f1m) * (max_epi / 4): the five roundings of the sum, one product (the quarter is exact)
    out["final_loss_scale"] = (2 * k * (me / 4), rk + 1) if kind == 0 else (ls * k, rk + 1)
    out["norm"] = (LD(1), 0) if kind in (0, 3) else (LD(norm_dev), 0)
    return out


def exact_fields(kind, n, table, K, ro, sq_thr_dev):
    """the fields that are exact: n, active, table, the records, dyn_max_iter, the score_initial_model state (from the device's own sq_thr)"""
    ok = n >= K
    DBL_MAX = np.finfo(np.float64).max
    initial = bool(ro.get("score_initial_model")) and ok and kind != 5
    score = np.float64(sq_thr_dev) * np.float64(n) if initial else DBL_MAX
    best = np.zeros(12)
    best[0] = 1.0
    if kind == 5:
        best[[0, 4, 8]] = 1.0  # the identity as a fundamental matrix in the model's first nine doubles
        best[[10, 11]] = 1.0
    else:
        best[[7, 10, 11]] = 1.0
    return dict(n=n if ok else 0, table=table, active=int(ok), n_triggers=0, best_min_cnt=0, best_min_score=score, dyn_max_iter=int(ro["max_iterations"]),
                iterations=0, refinements=int(initial), num_inliers=0, inlier_ratio=0.0, model_score=score), best


# ---------------------------------------------------------------------------------------------------------------- fragments
def bf16_bits(x32):
    """float32 -> bf16 bit pattern, round to nearest even; NaN stays NaN"""
    u = np.asarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF) >> 16
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_value(b):
    return (np.asarray(b, dtype=np.uint32) << 16).view(np.float32)


def bf16_split(x):
    """x = h + l, each a bf16"""
    with np.errstate(all="ignore"):
        x = np.asarray(x, dtype=np.float64)
        h = bf16_bits(x.astype(np.float32))
        return h, bf16_bits((x - bf16_value(h).astype(np.float64)).astype(np.float32))


def monomials(p4):
    a, b, c, d = (np.asarray(p4, dtype=np.float64)[:, q] for q in range(4))
    with np.errstate(all="ignore"):
        return np.stack([a * c, b * c, c, a * d, b * d, d, a, b], axis=1)


def unusable_rows(p4):
    """records whose fragment row is all zero: a monomial that is not below 1e15 in magnitude (NaN dropped, as fmax does), or a non-finite sum"""
    m = monomials(p4)
    with np.errstate(all="ignore"):
        mag = np.fmax.reduce(np.abs(m), axis=1, initial=0.0)
        s = m[:, 0] + m[:, 1] + m[:, 3] + m[:, 4]
        return ~(mag < 1e15) | ~(s == s)


def fragments(p4, n, n_max):
    """the pair's block of MFMA A fragments [ceil(n_max / 16)][64][4] uint32: for record i, in group i >> 4 at row i & 15, lanes 0-15 hold the high
    bf16 halves of the eight monomials, 16-31 the low halves, 32-47 the high halves again, 48-63 (1, 1, 1, 0, ...); eight bf16 per lane, two to a
    word, the even one in the low half.  Rows of unusable records and rows from n to the end of n's group are zero; later groups are not written
    (None in the mask returned beside the block)."""
    G = (n_max + 15) // 16
    out = np.zeros((G, 64, 4), dtype=np.uint32)
    written = np.zeros((G, 64), dtype=bool)
    if n > 0:
        m = monomials(p4[:n])
        h, l = bf16_split(m)
        pack = lambda v: (v[:, 0::2].astype(np.uint32) | (v[:, 1::2].astype(np.uint32) << 16))  # noqa: E731
        hi, lo = pack(h), pack(l)
        ones = np.tile(np.array([0x3F803F80, 0x00003F80, 0, 0], dtype=np.uint32), (n, 1))
        bad = unusable_rows(p4[:n])
        for blk, val in ((0, hi), (16, lo), (32, hi), (48, ones)):
            val = np.where(bad[:, None], np.uint32(0), val)
            out[np.arange(n) >> 4, blk + (np.arange(n) & 15)] = val
    g_end = (n + 15) // 16 * 16
    for i in range(g_end):
        written[i >> 4, (i & 15)::16] = True
    return out, written


# ---------------------------------------------------------------------------------------------------------------- sampler
def draw_table(seed, n, K, count):
    """the first `count` samples of the sequence for (seed, n, K): [count][K]"""
    out, state = np.zeros((count, K), dtype=np.int64), int(seed) & prosac_ref.M64
    for j in range(count):
        out[j], state = prosac_ref._draw(K, n, state)
    return out


# ---------------------------------------------------------------------------------------------------------------- solvers
_HM = None


def hostmath():
    """the device arithmetic compiled for the host (tests/hostmath), built where it is missing or stale, as tests/test_hostmath.py builds it"""
    global _HM
    if _HM is None:
        src, so = os.path.join(HERE, "hostmath", "hostmath.cpp"), os.path.join(HERE, "hostmath", "libhostmath.so")
        hdrs = [os.path.join(HERE, "..", "mdrp_amd", "csrc", h) for h in ("mdrp_math.h", "mdrp_classic_math.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", src, "-o", so])
        _HM = C.CDLL(so)
    return _HM


_dp = C.POINTER(C.c_double)
_P = lambda a: a.ctypes.data_as(_dp)  # noqa: E731
HM_SOLVER = {"p3p": 0, "shift": 1, "shared": 2, "varying": 3}


def solver_name(kind, shift):
    return {0: "shift" if shift else "p3p", 1: "shared", 2: "varying", 3: "5pt", 4: "6pt", 5: "7pt"}[kind]


def solver_inputs(kind, pts_rows, dep_rows):
    """what the solver kernels form from a sample's records: monodepth kinds (a, b, 1) and the depths; baselines the bearings (a p4, b p4, p4)"""
    p = np.asarray(pts_rows, dtype=np.float64)
    if kind <= 2:
        one = np.ones((len(p), 1))
        return (np.ascontiguousarray(np.concatenate([p[:, 0:2], one], axis=1)), np.ascontiguousarray(np.concatenate([p[:, 2:4], one], axis=1)),
                np.ascontiguousarray(dep_rows[:, 0]), np.ascontiguousarray(dep_rows[:, 1]))
    x1h = np.stack([p[:, 0] * p[:, 4], p[:, 1] * p[:, 4], p[:, 4]], axis=1)
    x2h = np.stack([p[:, 2] * p[:, 5], p[:, 3] * p[:, 5], p[:, 5]], axis=1)
    return np.ascontiguousarray(x1h), np.ascontiguousarray(x2h), None, None


def p3p_nan(x1h, x2h, d1):
    """the reference's P3P returns NaN poses for this sample (orc_p3p_reference_nan)"""
    import prior_ref
    return prior_ref._p3p_nan(x1h, x2h, d1)


def oracle_solutions(name, x1h, x2h, d1, d2):
    """the oracle's solutions as rows comparable with device_rows(): monodepth solvers 12-wide models; 5-point (q, t); 6-point (q, t, f); 7-point F.
    P3P: none where the reference's P3P returns NaN poses (the NaN model is no solution: slot state -3 stands for it)"""
    if name == "p3p":
        return [] if p3p_nan(x1h, x2h, d1) else list(po.solver_calib_p3p(x1h.reshape(-1), x2h.reshape(-1), d1, d2))
    if name in ("shift", "shared", "varying"):
        fn = {"shift": po.solver_calib_shift, "shared": po.solver_shared, "varying": po.solver_varying}[name]
        return list(fn(x1h.reshape(-1), x2h.reshape(-1), d1, d2))
    if name == "5pt":
        return [m[:7].copy() for m in po.relpose_5pt(x1h, x2h)]
    if name == "6pt":
        return [np.r_[m[:7], m[10]] for m in po.relpose_6pt(x1h, x2h)]
    return [f.reshape(-1).copy() for f in po.relpose_7pt(x1h, x2h)]


def host_solutions(name, x1h, x2h, d1, d2):
    """the host build of the device solver on the same sample, or None where there is none (6-point)"""
    hm = hostmath()
    if name in HM_SOLVER:
        out = np.zeros((4, 12))
        n = hm.hm_solver(C.c_int(HM_SOLVER[name]), _P(x1h), _P(x2h), _P(d1), _P(d2), _P(out))
        return list(out[:n])
    if name == "6pt":
        return None
    out = np.zeros((10, 12))
    n = (hm.hm_relpose_5pt if name == "5pt" else hm.hm_relpose_7pt)(_P(x1h), _P(x2h), _P(out))
    return [r[:7].copy() if name == "5pt" else r[:9].copy() for r in out[:n]]


def device_rows(name, models):
    """model records (MODEL_DTYPE) as rows comparable with the oracle's"""
    m = np.ascontiguousarray(models).view(np.float64).reshape(-1, 12)
    if name == "5pt":
        return [r[:7] for r in m]
    if name == "6pt":
        return [np.r_[r[:7], r[10]] for r in m]
    if name == "7pt":
        return [r[:9] for r in m]
    return list(m)


def same_solutions(name, A, B, ordered=False):
    """two solution lists agree by the suite's tolerances: monodepth match_solution_sets(1e-7); 5-point pose_diff, 7-point fund_diff, 6-point
    _same_sixpt at 1e-6 (tests/test_gpu_classic.py).  ordered: element by element, else as sets (a greedy one-to-one matching)"""
    from helpers import match_solution_sets
    from test_oracle_classic import _same_sixpt, fund_diff, pose_diff
    if len(A) != len(B):
        return False
    if name in HM_SOLVER:
        return match_solution_sets(list(A), list(B), 1e-7)
    near = {"5pt": lambda u, v: pose_diff(u, v) < 1e-6, "6pt": lambda u, v: _same_sixpt(u, v, 1e-6), "7pt": lambda u, v: fund_diff(u, v) < 1e-6}[name]
    with np.errstate(all="ignore"):
        if ordered:
            return all(near(u, v) for u, v in zip(A, B))
        left = list(range(len(B)))
        for u in A:
            j = next((j for j in left if near(u, B[j])), None)
            if j is None:
                return False
            left.remove(j)
    return True
