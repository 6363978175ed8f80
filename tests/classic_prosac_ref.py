"""Yardstick of mdrp_estimate_classic_ranked's sampler (include/mdrp.h): tests/prosac_ref.py's definition with the sample size K turned
from the constant 3 into a parameter, and nothing else changed.  A helper, not a test.

growth() / samples() restate RandomSampler::initialize_prosac / generate_sample of the reference for sample_sz = K (pinned to its binary through
tests/golden/classic_prosac_ref.npz); the ranking is prosac_ref.order, unchanged."""
import math

import numpy as np

from prosac_ref import M64, _draw, order  # noqa: F401  (order: the ranking is the monodepth estimators')


def growth(n, max_prosac_iterations, K):
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


def samples(n, seed, max_prosac_iterations, count, K):
    """(samples (count, K) int64, subset size before each sample (count,) int64)"""
    out, subs = np.zeros((count, K), dtype=np.int64), np.zeros(count, dtype=np.int64)
    if n < K:
        return out, subs
    g = growth(n, max_prosac_iterations, K)
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
