"""Inputs of the mdrp_estimate_batch_prior tests (a helper, not a test): the ragged batches of tests/from_models_cases.py with their start models as
priors, the options, and the yardstick's answers (tests/prior_ref.py over the oracle; computed once per process, on the CPU)."""
import functools

import numpy as np

import from_models_cases as fc
import helpers
import prior_ref as pr
from oracle import pyorc as po

LOSS = "TRUNCATED_CAUCHY"
ITER = dict(max_iterations=1000, min_iterations=100)


def oracle_options(name, score_initial=False, **iters):
    es = helpers.OPTIONS_KINDS[name][1]
    return (po.ransac_opt(estimate_shift=es, score_initial_model=score_initial, **fc.RO, **dict(ITER, **iters)),
            po.bundle_opt(max_iterations=100, loss_type=fc.LOSSES[LOSS], loss_scale=1.0, gradient_tol=1e-10))


def library_options(name, capi, score_initial=False, **more):
    es = helpers.OPTIONS_KINDS[name][1]
    return (capi.ransac_opt_from_dict(dict(fc.RO, monodepth_estimate_shift=es, score_initial_model=score_initial, **dict(ITER, **more))),
            capi.bundle_opt_from_dict({"loss_type": LOSS}))


def _cams(b):
    return (po.cam_flat(*b["cams"][0]), po.cam_flat(*b["cams"][1])) if b["cams"] else (None, None)


@functools.lru_cache(maxsize=None)
def yardstick(name, with_priors=True, max_iterations=1000, min_iterations=100):
    """the yardstick's answer for every pair of from_models_cases.batch(name), its start models as priors (or none): a list of dicts"""
    kind = helpers.OPTIONS_KINDS[name][0]
    b = fc.batch(name)
    ro, bo = oracle_options(name, max_iterations=max_iterations, min_iterations=min_iterations)
    c1, c2 = _cams(b)
    return [pr.estimate_from_prior(kind, b["x1"][i, :n], b["x2"][i, :n], b["d1"][i, :n], b["d2"][i, :n], ro, bo, b["models"][i] if with_priors else None, c1, c2)
            for i, n in enumerate(b["n"])]


@functools.lru_cache(maxsize=None)
def oracle_estimate(name):
    """po.estimate (no prior) for every pair of the batch with n >= 3, None below: [(model, stats, mask)]"""
    kind = helpers.OPTIONS_KINDS[name][0]
    b = fc.batch(name)
    ro, bo = oracle_options(name)
    c1, c2 = _cams(b)
    return [po.estimate(kind, b["x1"][i, :n], b["x2"][i, :n], b["d1"][i, :n], b["d2"][i, :n], ro, bo, c1, c2) if n >= 3 else None for i, n in enumerate(b["n"])]


def identity_priors(name, capi):
    """[B] records that are the identity pose in NORMALISED units (scale 1, shifts 0, focals 1): focals = the pair's normalisation scale in pixels"""
    kind = helpers.OPTIONS_KINDS[name][0]
    b = fc.batch(name)
    ro, bo = oracle_options(name)
    c1, c2 = _cams(b)
    out = np.zeros((len(b["n"]), 12))
    for i, n in enumerate(b["n"]):
        out[i] = po.new_model()
        if kind != po.CALIB and n >= 3:
            out[i, 10:12] = pr.fm.prep(kind, b["x1"][i, :n], b["x2"][i, :n], ro, bo, c1, c2)["norm"]
    return capi.array_to_models(out)
