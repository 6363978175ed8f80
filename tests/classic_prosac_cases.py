"""Inputs of the ranked baselines' (PROSAC on the 5- / 6- / 7-point estimators) tests, shared by tests/tools/gen_golden_classic_prosac.py,
tests/test_classic_prosac_host.py and tests/test_gpu_classic_prosac.py (a helper, not a test): the sampler rows and the estimator cases of
tests/golden/classic_prosac_ref.npz, and their options for the oracle and the library."""
import functools
import hashlib
import os

import numpy as np

from mdrp_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "classic_prosac_ref.npz")
KINDS = (3, 4, 5)
SAMPLE_SIZE = {3: 5, 4: 6, 5: 7}
KIND_NAMES = {3: "relpose_5pt", 4: "shared_focal_6pt", 5: "fundamental_7pt"}
FOCAL = 800.0
THRESHOLD = 2.0
CAMERA = {"model": "SIMPLE_PINHOLE", "width": 1600, "height": 1200, "params": [FOCAL, 0.0, 0.0]}
BUNDLE = {"max_iterations": 100, "loss_type": "TRUNCATED_CAUCHY", "loss_scale": 1.0, "gradient_tol": 1e-10}


def sampler_rows(K):
    """(n, seed, max_prosac_iterations, count) for sample size K"""
    return ((K, 0, 100000, 50), (K + 1, 1, 100000, 200), (20, 0, 50, 60), (64, 2, 150, 2500), (65, 2, 100000, 2500), (97, 2, 0, 600), (97, 2, 1, 600),
            (97, 2, 2, 600), (300, 3, 150, 2500), (2000, 0, 100000, 12000))


# (n, max_iterations, min_iterations, max_prosac_iterations, RANSAC seed, outlier fraction)
_CASES = ((300, 400, 400, 100000, 0, 0.5), (300, 400, 400, 150, 3, 0.5), (1000, 1000, 1000, 1000, 0, 0.7), (200, 500, 20, 60, 9, 0.2),
          (97, 300, 300, 1, 2, 0.3), (2000, 2000, 2000, 100000, 0, 0.5))


def cases(kind):
    """the kind's cases; the 6-point estimator (about 0.5 k pairs/s) runs half the iterations and not the n = 2000 case"""
    if kind != 4:
        return _CASES
    return tuple((n, mx // 2, max(mn // 2, 1), mp, seed, out) for n, mx, mn, mp, seed, out in _CASES[:5])


# The number that seeds a case's pair and its score noise: 100 * kind + index, moved on by 1000 per replacement where the CPU oracle's uniform run did
# not reproduce the reference's uniform record on the pair first tried (the admission rule of tests/tools/gen_golden_classic_prosac.py, which prints
# every replacement)
DATA_ID = {3: (300, 301, 302, 303, 304, 305), 4: (400, 401, 402, 403, 404), 5: (500, 501, 502, 503, 504, 505)}


@functools.lru_cache(maxsize=None)
def case(kind, index, data_id=None):
    """the pair in the caller's order, its scores (higher is better) and order (caller index of every rank), and the case's options"""
    n, max_it, min_it, max_prosac, seed, outliers = cases(kind)[index]
    did = DATA_ID[kind][index] if data_id is None else data_id
    p = synth.make_pair(did, n, outlier_frac=outliers, random_focal="shared" if kind == 4 else None)
    q = p["is_outlier"] + np.random.default_rng(did).normal(0.0, 0.6, n)
    scores = -q
    return dict(x1=p["x1"], x2=p["x2"], scores=scores, order=np.argsort(-scores, kind="stable"), n=n, max_it=max_it, min_it=min_it, max_prosac=max_prosac,
                seed=seed, data_id=did)


def digest(c):
    h = hashlib.sha256()
    for k in ("x1", "x2", "scores"):
        h.update(np.ascontiguousarray(c[k], dtype=np.float64).tobytes())
    return h.digest()


def ransac_dict(c, **more):
    """the case's RansacOptions as the Python entry points take them"""
    return dict(max_iterations=c["max_it"], min_iterations=c["min_it"], seed=c["seed"], max_epipolar_error=THRESHOLD, max_prosac_iterations=c["max_prosac"], **more)


def oracle_run(kind, c, x1, x2):
    """po.estimate_classic (uniform sampling) under the case's options: (model, stats, mask)"""
    from oracle import pyorc as po
    cam = po.cam_flat(0, [FOCAL, 0.0, 0.0]) if kind == 3 else None
    return po.estimate_classic(kind, x1, x2, po.ransac_opt(max_iterations=c["max_it"], min_iterations=c["min_it"], max_epipolar_error=THRESHOLD, seed=c["seed"]),
                               po.bundle_opt(max_iterations=100, loss_type=4, loss_scale=1.0, gradient_tol=1e-10), cam, cam, pp=(0.0, 0.0))


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


def golden_case(kind, index):
    """the reference's records on the pre-sorted pair: under progressive_sampling (model, stats, mask in RANK order) and uniform (u...)"""
    g, t = golden(), f"{kind}_{index}"
    n = cases(kind)[index][0]
    return dict(order=g["order_" + t].astype(np.int64), digest=g["digest_" + t].tobytes(), model=g["model_" + t], stats=g["stats_" + t],
                mask=np.unpackbits(g["mask_" + t])[:n], umodel=g["umodel_" + t], ustats=g["ustats_" + t], umask=np.unpackbits(g["umask_" + t])[:n])
