"""The calls of the history matrix for the entry points of include/mdrp_classic_ranked.h (a helper, not a test): tests/history_cases.py's table
enumerates the handle entry points of include/mdrp.h itself; the baselines' ranked entry points are declared in the extension header and have their
calls here, built from the same classes, and tests/test_gpu_classic_history.py runs them against that table in both directions."""
import functools
import os
import re

import numpy as np

import history_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ClassicRanked(hc.Ranked):
    """mdrp_estimate_classic_ranked / mdrp_estimate_classic_ranked_async: a baseline (kind 3, 4, 5) in match-score order, no depths"""

    def run(self, h):
        if self.device:
            return self.collect(h, self.issue(h))
        d = self.data()
        ro, bo = self.options()
        cam = self.cams()
        res, mask = h.estimate_classic_ranked(self.kind, d["x1"], d["x2"], None if self.presorted else d["scores"], ro, bo, d["n"], cam, cam)
        self.stats = h.last_stats()
        return res.tobytes(), mask.tobytes()

    def queue(self, h, x1, x2, d1, d2, ro, bo, cam, mask, state):
        sc = state["scores"]
        h.estimate_classic_ranked_device(self.kind, x1.data_ptr(), x2.data_ptr(), None if sc is None else sc.data_ptr(), self.batch, self.n_max, ro, bo,
                                         self.data()["n"], cam, cam, mask.data_ptr())


@functools.lru_cache(maxsize=None)
def probes():
    e = hc._estimate
    dev = ["mdrp_estimate_classic_ranked_async", "mdrp_fetch_results"]
    return (
        e("classic_ranked_host_150", 3, hc.S1, 3500, cls=ClassicRanked, entry_points=["mdrp_estimate_classic_ranked"]),
        e("classic_ranked_host_presorted", 4, hc.S7, 3550, cls=ClassicRanked, entry_points=["mdrp_estimate_classic_ranked"], presorted=True),
        e("classic_ranked_device_150", 5, hc.S2, 3600, True, cls=ClassicRanked, entry_points=dev),
        e("classic_ranked_device_6pt", 4, hc.S5, 3650, True, cls=ClassicRanked, entry_points=dev),
        hc.Unit("prosac_samples_k", ["mdrp_prosac_samples_k"], lambda: dict(row=np.array([300, 3, 150, 7], dtype=np.int64), lens=np.array([128, 372], dtype=np.int32)),
                lambda h, capi, d: (h.prosac_samples_k(int(d["row"][1]), int(d["row"][0]), int(d["row"][3]), int(d["row"][2]), d["lens"]),), ("samples",),
                lambda d: [d["row"], d["lens"]]),
    )


@functools.lru_cache(maxsize=None)
def back_to_back():
    """device-resident calls issued without a wait between them, as hc.back_to_back(): a ranked baseline call in front of and behind a plain one"""
    shape = (5, 130, 300, 300)
    a = dict(device=True, probe=False, focal=800.0)
    b = dict(device=True, probe=False, focal=640.0, ns=(113, 130, 0, 2, 97))
    e = hc._estimate
    dev = ["mdrp_estimate_classic_ranked_async"]
    return ((e("b2b_classic_ranked", 3, shape, 7300, cls=ClassicRanked, entry_points=dev, **a), e("b2b_then_plain_5pt", 3, shape, 7400, **b)),
            (e("b2b_plain_7pt", 5, shape, 7500, **a), e("b2b_then_classic_ranked", 5, shape, 7600, cls=ClassicRanked, entry_points=dev, **b)),
            (e("b2b_mono_ranked", 0, shape, 7700, cls=hc.Ranked, entry_points=["mdrp_estimate_batch_ranked_async"], **a),
             e("b2b_then_classic_ranked_5pt", 3, shape, 7800, cls=ClassicRanked, entry_points=dev, **b)))


def extension_entry_points():
    """names of the functions declared in include/mdrp_classic_ranked.h with an `mdrp_handle *` parameter (tests/test_history_host.py's parse)"""
    src = open(os.path.join(ROOT, "include", "mdrp_classic_ranked.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = "\n".join(line for line in src.splitlines() if not line.lstrip().startswith("#"))
    decls = re.findall(r"\b(mdrp_\w+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S)
    return sorted({name for name, args in decls if re.search(r"\bmdrp_handle\s*\*\s*\w", args)})
