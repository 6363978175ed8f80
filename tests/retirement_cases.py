"""Inputs of tests/test_gpu_retirement.py: pairs, the 1100 models of a pair, their oracle scores, and count_split_tiles restated.

Nothing here touches the GPU.  A pair's models follow the mix of test_count_candidates_is_conservative: every third one is a perturbation of the true pose
(0.0015 (k mod 7) in rotation, 0.0015 (k mod 5) in translation, the true focal lengths), the rest are random poses with focal lengths that fit nothing;
one NaN, one inf and one zero-quaternion model; and three slots — one in each k_count workgroup, the last one also in the ragged last k_bound
workgroup — that a test overwrites with exact duplicates of the model it plants its bar from."""
import functools
import math

import numpy as np

NS = (3, 64, 257, 513, 1000, 1024, 1025, 2000, 2049)
FRONT_NS = (40, 257, 600)  # tests/test_gpu_first_front.py (the sizes of tests/test_gpu_first_filter.py above one sample)
_SEED_NS = NS + tuple(n for n in FRONT_NS if n not in NS)
PAIRS = ((0.05, 1.0), (0.4, 1.0), (0.6, 1.0), (0.0, 0.5))  # (outlier fraction, noise in pixels)
NUM_MODELS = 1100  # three k_count workgroups of 512 (the last one ragged), five k_bound workgroups of 256
NAN_SLOT, INF_SLOT, ZEROQ_SLOT = 7, 8, 9
SPECIAL_SLOTS = (NAN_SLOT, INF_SLOT, ZEROQ_SLOT)
DUP_SLOTS = (1, 700, 1099)  # garbage slots (k mod 3 != 0)
THR = (2.0 / 800.0) ** 2
DBL_MAX = float(np.finfo(np.float64).max)
NEAR_TRUE = tuple(k for k in range(0, NUM_MODELS, 3) if k not in SPECIAL_SLOTS)
# garbage candidate rates a two-phase count is given besides the pair's own statistics, as (candidates, evaluations)
RATE_STATS = ((50_000, 1_000_000), (0, 1_000_000), (250_000, 1_000_000))
# split points (tiles of phase A, tiles of the pair) the cases must reach between them
REQUIRED_SPLITS = frozenset({(2, 4), (2, 5), (3, 5), (3, 8), (5, 8), (6, 8), (3, 9), (5, 9), (7, 9)})


def count_tiles(n):
    return (((n + 15) >> 4) + 15) // 16  # k_count: tiles of 16 groups of 16 records


def split_tiles(n, thr, rec_cnt, rec_score, cand, evals):
    """count_split_tiles (mdrp_kernels.h), operation for operation: the tiles of phase A, or all of them where the pair is not split"""
    n_tiles = count_tiles(n)
    if not rec_score < DBL_MAX or n_tiles < 4 or evals == 0:
        return n_tiles
    inflated = rec_score * (1.0 + 1e-12)
    bar = min(math.floor(float(n) - inflated / thr), int(rec_cnt))
    if bar <= 0:
        return n_tiles
    g = min(0.5, 1.1 * float(cand) / float(evals) + 0.005)
    ra = int(float(n - bar) / (1.0 - g)) + 32
    ta = (ra + 255) >> 8
    return n_tiles if ta + 2 > n_tiles else ta


@functools.lru_cache(maxsize=None)
def pair_case(n, pi):
    """correspondences (normalised by the focal length 800) and the pose models [NUM_MODELS][12] of pair pi at n correspondences"""
    from mdrp_amd import synth
    from oracle import pyorc as po
    frac, noise = PAIRS[pi]
    p = synth.make_pair(61000 + 4 * _SEED_NS.index(n) + pi, n, noise_px=noise, outlier_frac=frac)
    x1, x2 = np.ascontiguousarray(p["x1"] / 800.0), np.ascontiguousarray(p["x2"] / 800.0)
    rng = np.random.default_rng(7000 + 10 * n + pi)
    ms = np.zeros((NUM_MODELS, 12))
    for k in range(NUM_MODELS):
        m = po.new_model()
        if k % 3 == 0:
            R = p["R"] @ synth.rodrigues(rng.normal(0, 0.0015 * (k % 7), 3)); t = p["t"] + rng.normal(0, 0.0015 * (k % 5), 3)
        else:
            R = synth.rodrigues(rng.normal(0, 1.0, 3)); t = rng.normal(size=3) * 10.0 ** rng.integers(-3, 3)
            m[10] = 1.0 + 0.3 * (k % 5); m[11] = 0.8 + 0.1 * (k % 7)
        q = np.zeros(4); po.lib().orc_rotmat_to_quat(np.ascontiguousarray(R.reshape(-1)).ctypes.data_as(po._dp), q.ctypes.data_as(po._dp))
        m[:4] = q; m[4:7] = t
        ms[k] = m
    ms[NAN_SLOT][4] = np.nan; ms[INF_SLOT][5] = np.inf; ms[ZEROQ_SLOT][:4] = 0.0
    for a in (x1, x2, ms):
        a.setflags(write=False)
    return x1, x2, ms


@functools.lru_cache(maxsize=None)
def fundamentals(n, pi):
    """the same models as raw fundamental matrices [NUM_MODELS][9] (MDRP_FUNDAMENTAL_7PT): F = diag(1, 1, f2) E diag(1, 1, f1) of every finite pose;
    a NaN entry, an inf entry and the zero matrix in the special slots"""
    from oracle import pyorc as po
    _, _, ms = pair_case(n, pi)
    F = np.zeros((NUM_MODELS, 9))
    for k in range(NUM_MODELS):
        if k not in SPECIAL_SLOTS:
            F[k] = po.fundamental(ms[k]).reshape(-1)
    F[NAN_SLOT] = F[0]; F[NAN_SLOT][4] = np.nan
    F[INF_SLOT] = F[3]; F[INF_SLOT][5] = np.inf
    F.setflags(write=False)
    return F


@functools.lru_cache(maxsize=None)
def oracle_scores(n, pi, pose):
    """(score, count) of every model but the special ones by the oracle: msac_pose of the pose models (calibrated), msac_F of their fundamental
    matrices (the varying-focal estimator and the 7-point baseline score the same F)"""
    from oracle import pyorc as po
    x1, x2, ms = pair_case(n, pi)
    F = None if pose else fundamentals(n, pi)
    score, count = np.full(NUM_MODELS, np.nan), np.full(NUM_MODELS, -1, dtype=np.int64)
    for k in range(NUM_MODELS):
        if k in SPECIAL_SLOTS:
            continue
        score[k], count[k] = po.msac_pose(ms[k], x1, x2, THR) if pose else po.msac_F(F[k], x1, x2, THR)
    score.setflags(write=False); count.setflags(write=False)
    return score, count


def with_duplicates(rows, k):
    """rows with the duplicate slots overwritten by row k"""
    out = np.array(rows, copy=True)
    for d in DUP_SLOTS:
        out[d] = out[k]
    return out


def bar_models(order):
    """the models a test plants its bars from, given the near-true models in ascending order of (count, -score): median, 0.9-quantile, best"""
    picks = []
    for k in (order[len(order) // 2], order[int(0.9 * len(order))], order[-1]):
        if k not in picks:
            picks.append(k)
    return picks
