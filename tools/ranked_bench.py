#!/usr/bin/env python3
"""What estimating in match-score order costs and buys at the headline shape (B = 1024 pairs, N = 2000 correspondences, calibrated estimator,
10^4 RANSAC iterations), correspondences and scores resident on the GPU, seeded from synth, at 50 % and at 85 % outliers; the scores are
-(outlier flag + N(0, 0.6)), a matcher's confidence of middling quality.

Three routes, warmed and alternated in one process, each timed with the host clock around a call that ends in the fetched result records:
  (r) poselib.estimate_batch_torch(scores = tensor): ranking, gather, progressive sampler, mask scatter;
  (s) poselib.estimate_batch_torch(scores = "presorted") on the pre-sorted records: the progressive sampler alone;
  (e) poselib.estimate_batch_torch on the pre-sorted records: today's uniform sampler.
(r) against (s) is the cost of ranking and permuting, (s) against (e) what the sampler itself changes.  Each under the fixed schedule (min_iterations
= max_iterations) and under the dynamic rule (min_iterations = 100), and once more one pair per call at N = 1000.  Reports the median of the
repetitions and their spread, and the mean inliers, iterations and LO counts each route ends with; writes profiles/ranked_bench.json.

    python tools/ranked_bench.py [--batch 1024] [--n 2000] [--iters 10000] [--reps 21] [--out profiles/ranked_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAM = {"model": "SIMPLE_PINHOLE", "width": 1600, "height": 1200, "params": [800.0, 0.0, 0.0]}
BO = {"loss_type": "TRUNCATED_CAUCHY"}


def inputs(batch, n, frac):
    """(caller-order arrays, scores, the same arrays pre-sorted by descending score)"""
    from mdrp_amd import synth
    b = synth.make_batch(0, batch, n, noise_px=0.5, depth_noise=0.02, outlier_frac=frac)
    rng = np.random.default_rng(9)
    scores = -(np.stack([g["is_outlier"] for g in b["gt"]]).astype(np.float64) + rng.normal(0.0, 0.6, (batch, n)))
    order = np.argsort(-scores, axis=1, kind="stable")
    srt = {k: np.ascontiguousarray(np.take_along_axis(b[k], order[..., None] if b[k].ndim == 3 else order, axis=1)) for k in ("x1", "x2", "d1", "d2")}
    return b, scores, srt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--dynamic-min", type=int, default=100)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--outliers", type=float, nargs="+", default=[0.5, 0.85])
    ap.add_argument("--single-n", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranked_bench.json"))
    a = ap.parse_args()
    import torch
    import mdrp_amd.poselib as poselib
    dev = torch.device("cuda", 0)
    doc = {"shape": {"batch": a.batch, "correspondences": a.n, "iterations": a.iters, "repetitions": a.reps, "estimator": "calibrated",
                     "scores": "-(outlier flag + N(0, 0.6))", "max_prosac_iterations": 100000},
           "routes": {"r": "estimate_batch_torch, scores = tensor", "s": 'estimate_batch_torch, scores = "presorted", pre-sorted records',
                      "e": "estimate_batch_torch, pre-sorted records, uniform sampler"},
           "runs": []}
    for batch, n in ((a.batch, a.n), (1, a.single_n)):
        for frac in a.outliers:
            b, scores, srt = inputs(batch, n, frac)
            t = [torch.from_numpy(b[k]).to(dev) for k in ("x1", "x2", "d1", "d2")]
            ts = [torch.from_numpy(srt[k]).to(dev) for k in ("x1", "x2", "d1", "d2")]
            sc = torch.from_numpy(scores).to(dev)
            for schedule, min_it in (("fixed", a.iters), ("dynamic", min(a.dynamic_min, a.iters))):
                ro = {"max_iterations": a.iters, "min_iterations": min_it, "max_epipolar_error": 2.0, "max_reproj_error": 16.0}
                routes = {"r": lambda: poselib.estimate_batch_torch("calibrated", *t, CAM, CAM, ro, BO, scores=sc),
                          "s": lambda: poselib.estimate_batch_torch("calibrated", *ts, CAM, CAM, ro, BO, scores="presorted"),
                          "e": lambda: poselib.estimate_batch_torch("calibrated", *ts, CAM, CAM, ro, BO)}
                times = {k: [] for k in routes}
                last = {}
                for rep in range(a.reps + 2):  # two warm-up rounds
                    for k, fn in routes.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        last[k] = fn()
                        torch.cuda.synchronize()
                        if rep >= 2:
                            times[k].append(time.perf_counter() - t0)
                assert last["r"][0].tobytes() == last["s"][0].tobytes(), "ranked and presorted records differ"
                run = {"batch": batch, "correspondences": n, "outlier_frac": frac, "schedule": schedule, "min_iterations": min_it}
                for k, v in times.items():
                    v, r = np.array(v), last[k][0]
                    run[k] = {"pairs_per_s_median": batch / float(np.median(v)), "ms_median": 1e3 * float(np.median(v)), "ms_min": 1e3 * float(v.min()),
                              "ms_max": 1e3 * float(v.max()), "spread_rel": float((v.max() - v.min()) / np.median(v)),
                              "inliers_mean": float(r["num_inliers"].mean()), "iterations_mean": float(r["iterations"].mean()),
                              "refinements_mean": float(r["refinements"].mean())}
                doc["runs"].append(run)
                print(json.dumps(run), flush=True)
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
