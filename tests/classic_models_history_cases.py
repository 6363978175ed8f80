"""The calls of the history matrix for the entry points of include/mdrp_classic_models.h (a helper, not a test): tests/history_cases.py's table
enumerates the handle entry points of include/mdrp.h itself and tests/classic_history_cases.py those of mdrp_classic_ranked.h; the baselines' calls
from a caller's model are declared in their own extension header and have their calls here, built from the same classes, and
tests/test_gpu_classic_models_history.py runs them against that table in both directions."""
import functools
import os
import re

import numpy as np

import classic_models_cases as cc
import history_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def classic_start_models(e, d):
    """[B] model records in the caller's units from the pairs' ground truth through classic_models_cases.start_model; e.how: one word per pair"""
    rng = np.random.default_rng(e.seed + 977)
    return hc._capi().array_to_models(np.stack([cc.start_model(e.kind, p, e.how[i % len(e.how)], rng, e.amount) for i, p in enumerate(d["pairs"])]))


class ClassicPrior(hc.Prior):
    """mdrp_estimate_classic_prior / mdrp_estimate_classic_prior_async: a baseline (kind 3, 4, 5) with a prior per pair, one of them a NaN record, one
    hopeless; no depths"""

    def make(self):
        d = hc.Estimate.make(self)
        d["models"] = classic_start_models(self, d)
        return d

    def run(self, h):
        if self.device:
            return self.collect(h, self.issue(h))
        d = self.data()
        ro, bo = self.options()
        cam = self.cams()
        res, mask = h.estimate_classic_prior(self.kind, d["x1"], d["x2"], d["models"], ro, bo, d["n"], cam, cam)
        self.stats = h.last_stats()
        return res.tobytes(), mask.tobytes()

    def queue(self, h, x1, x2, d1, d2, ro, bo, cam, mask, state):
        h.estimate_classic_prior_device(self.kind, x1.data_ptr(), x2.data_ptr(), self.batch, self.n_max, state["models"].data_ptr(), ro, bo, self.data()["n"],
                                        cam, cam, mask.data_ptr())


class ClassicRefine(hc.Refine):
    """mdrp_refine_classic / mdrp_refine_classic_async: records, mask, and the start models' scores and inlier counts"""
    amount = 0.1  # (near enough for the start model itself to have inliers under the pose kinds' cheirality rule: it is all a refine call has)
    how = ("perturbed", "exact", "identity", "nan", "hopeless", "perturbed", "exact")

    def make(self):
        d = hc.Estimate.make(self)
        d["models"] = classic_start_models(self, d)
        return d

    def run(self, h):
        if self.device:
            return self.collect(h, self.issue(h))
        d = self.data()
        ro, bo = self.options()
        cam = self.cams()
        res, mask, score0, inl0 = h.refine_classic(self.kind, d["x1"], d["x2"], d["models"], ro, bo, self.stages, d["n"], cam, cam)
        self.stats = h.last_stats()
        return res.tobytes(), mask.tobytes(), score0.tobytes(), inl0.tobytes()

    def queue(self, h, x1, x2, d1, d2, ro, bo, cam, mask, state):
        h.refine_classic_device(self.kind, x1.data_ptr(), x2.data_ptr(), self.batch, self.n_max, state["models"].data_ptr(), ro, bo, self.stages,
                                self.data()["n"], cam, cam, mask.data_ptr(), state["score0"].data_ptr(), state["inl0"].data_ptr())


@functools.lru_cache(maxsize=None)
def probes():
    e = hc._estimate
    fetch = "mdrp_fetch_results"
    return (
        e("classic_refine_host", 3, (5, 130, 0, 0), 3700, cls=ClassicRefine, entry_points=["mdrp_refine_classic"]),
        e("classic_refine_device", 5, (24, 300, 0, 0), 3750, True, cls=ClassicRefine, entry_points=["mdrp_refine_classic_async", fetch]),
        e("classic_refine_device_count_only", 4, (5, 130, 0, 0), 3800, True, cls=ClassicRefine, entry_points=["mdrp_refine_classic_async", fetch], stages=0),
        e("classic_prior_host", 5, hc.S1, 3850, cls=ClassicPrior, entry_points=["mdrp_estimate_classic_prior"]),
        e("classic_prior_device", 3, hc.S5, 3900, True, cls=ClassicPrior, entry_points=["mdrp_estimate_classic_prior_async", fetch]),
        e("classic_prior_device_6pt", 4, hc.S7, 3950, True, cls=ClassicPrior, entry_points=["mdrp_estimate_classic_prior_async", fetch]),
    )


@functools.lru_cache(maxsize=None)
def back_to_back():
    """device-resident calls issued without a wait between them, as hc.back_to_back(): a call from models in front of and behind a plain one"""
    shape = (5, 130, 300, 300)
    a = dict(device=True, probe=False, focal=800.0)
    b = dict(device=True, probe=False, focal=640.0, ns=(113, 130, 0, 2, 97))
    e = hc._estimate
    prior, refine = ["mdrp_estimate_classic_prior_async"], ["mdrp_refine_classic_async"]
    return ((e("b2b_classic_prior", 3, shape, 8100, cls=ClassicPrior, entry_points=prior, **a), e("b2b_then_plain_7pt", 5, shape, 8200, **b)),
            (e("b2b_plain_5pt", 3, shape, 8300, **a), e("b2b_then_classic_prior", 5, shape, 8400, cls=ClassicPrior, entry_points=prior, **b)),
            (e("b2b_classic_refine", 5, (5, 130, 0, 0), 8500, cls=ClassicRefine, entry_points=refine, **a), e("b2b_then_plain_5pt_2", 3, shape, 8600, **b)),
            (e("b2b_mono_estimate", 0, shape, 8700, **a), e("b2b_then_classic_refine", 3, (5, 130, 0, 0), 8900, cls=ClassicRefine, entry_points=refine, **b)))


def extension_entry_points():
    """names of the functions declared in include/mdrp_classic_models.h with an `mdrp_handle *` parameter (tests/test_history_host.py's parse)"""
    src = open(os.path.join(ROOT, "include", "mdrp_classic_models.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = "\n".join(line for line in src.splitlines() if not line.lstrip().startswith("#"))
    decls = re.findall(r"\b(mdrp_\w+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S)
    return sorted({name for name, args in decls if re.search(r"\bmdrp_handle\s*\*\s*\w", args)})
