"""Yardstick of mdrp_estimate_batch_ranked (include/mdrp.h): the definition, in NumPy over the CPU oracle's pieces.  A helper, not a test.

order() is the ranking, growth() / subset_schedule() / samples() restate RandomSampler::initialize_prosac / generate_sample of the reference (pinned
to its binary through tests/golden/prosac_ref.npz), and estimate() is the loop of tests/prior_ref.py on the records in score order with the sample
source swapped: prior_ref asks the oracle for its sample table through po.draw_samples, and gets this module's table for the length of the call."""
import contextlib
import math

import numpy as np

import prior_ref as pr
from oracle import pyorc as po

K = 3
M64 = (1 << 64) - 1


def order(scores):
    """caller index of the record at every rank: descending score, NaN as -inf, -0.0 = +0.0, ties by ascending caller index"""
    key = np.array(scores, dtype=np.float64).reshape(-1)
    key[np.isnan(key)] = -np.inf
    key = key + 0.0  # (-0.0 + 0.0 = +0.0: the two zeros are one key; the stable sort would keep them tied anyway)
    return np.argsort(-key, kind="stable")


def growth(n, max_prosac_iterations):
    g = [1] * max(n, K)
    if n < K:
        return g
    T = float(max_prosac_iterations)
    for i in range(K):
        T = T * (float(K - i) / float(n - i))
    Tp = 1
    for i in range(K, n):
        Tn = T * (i + 1.0) / (i + 1.0 - K)
        Tp += math.ceil(Tn - T)
        g[i] = Tp
        T = Tn
    return g


def _splitmix_int(state):
    state = (state + 0x9E3779B97F4A7C15) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    v = (z ^ (z >> 31)) & 0xFFFFFFFF
    return state, (v - (1 << 32) if v >= (1 << 31) else v)


def _draw(k, n, state):
    """k distinct indices from [0, n): int32 draws taken modulo n as uint64, redrawn on a duplicate (draw_sample)"""
    out = []
    while len(out) < k:
        state, v = _splitmix_int(state)
        i = (v & M64) % n
        if i not in out:
            out.append(i)
    return out, state


def samples(n, seed, max_prosac_iterations, count):
    """(samples (count, 3) int64, subset size before each sample (count,) int64)"""
    out, subs = np.zeros((count, K), dtype=np.int64), np.zeros(count, dtype=np.int64)
    if n < K:
        return out, subs
    g = growth(n, max_prosac_iterations)
    state, k, sub = int(seed) & M64, 1, K
    for j in range(count):
        subs[j] = sub
        if k < max_prosac_iterations:
            s, state = _draw(K - 1, sub - 1, state)
            out[j] = s + [sub - 1]
            k += 1
            if k < max_prosac_iterations and k > g[sub - 1]:
                sub = min(sub + 1, n)
        else:
            out[j], state = _draw(K, n, state)
    return out, subs


@contextlib.contextmanager
def _sample_source(max_prosac_iterations):
    """po.draw_samples(seed, n, count) answers with the progressive table while the block runs"""
    uniform = po.draw_samples
    po.draw_samples = lambda seed, n, count: samples(int(n), int(seed), int(max_prosac_iterations), int(count))[0]
    try:
        yield
    finally:
        po.draw_samples = uniform


def estimate(kind, x1, x2, d1, d2, scores, ropt, bopt, max_prosac_iterations, cam1=None, cam2=None):
    """the ranked estimator in the caller's units: prior_ref.estimate_from_prior's dict, `mask` in the caller's order, plus `order` and `mask_ranked`.
    scores None: the records are in quality order already."""
    x1, x2 = po.f64(x1).reshape(-1, 2), po.f64(x2).reshape(-1, 2)
    d1, d2 = po.f64(d1).reshape(-1), po.f64(d2).reshape(-1)
    o = np.arange(len(x1)) if scores is None else order(scores)
    with _sample_source(max_prosac_iterations):
        r = pr.estimate_from_prior(kind, x1[o], x2[o], d1[o], d2[o], ropt, bopt, None, cam1, cam2)
    r["order"], r["mask_ranked"] = o, r["mask"]
    mask = np.zeros(len(x1), dtype=np.uint8)
    mask[o] = r["mask_ranked"]
    r["mask"] = mask
    return r
