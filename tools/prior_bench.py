#!/usr/bin/env python3
"""What a prior buys the estimator at the headline shape (B = 1024 pairs, N = 2000 correspondences, calibrated estimator, 10^4 RANSAC iterations):
correspondences and priors resident on the GPU, seeded from synth, at 50 % and at 85 % outliers.

The priors are the estimator's own results on the same pairs, perturbed by 1 degree in the rotation and 2 % in the translation and the scale (the
previous video frame's pose, a pose from the pose graph or from a coarse first pass); the hopeless priors are random poses (what a wrong prior
costs: one LM per pair).  Three routes, warmed and alternated in one process, each timed with the host clock around a call that ends in the fetched
result records:
  (p) poselib.estimate_batch_torch(priors = perturbed results);
  (h) poselib.estimate_batch_torch(priors = random poses);
  (e) poselib.estimate_batch_torch without priors — the existing call the two are compared with.
Each under the fixed schedule (min_iterations = max_iterations: a prior can only retire hypotheses) and under the dynamic one (min_iterations =
1000: a prior also ends the search sooner).  Reports the median of the repetitions and their spread, and how many inliers and iterations each route
ends with; writes profiles/prior_bench.json.

    python tools/prior_bench.py [--batch 1024] [--n 2000] [--iters 10000] [--reps 21] [--out profiles/prior_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from from_models_bench import BO, CAM, perturb  # noqa: E402


def hopeless(models, rng):
    """random unit quaternions, translations and a scale of 1: models that fit nothing"""
    out = models.copy()
    q = rng.normal(0.0, 1.0, (len(out), 4))
    out["q"] = q / np.linalg.norm(q, axis=1, keepdims=True)
    out["t"] = rng.normal(0.0, 0.5, (len(out), 3))
    out["scale"] = 1.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--dynamic-min", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--outliers", type=float, nargs="+", default=[0.5, 0.85])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prior_bench.json"))
    a = ap.parse_args()
    import torch
    import mdrp_amd.poselib as poselib
    from mdrp_amd import synth
    dev = torch.device("cuda", 0)
    doc = {"shape": {"batch": a.batch, "correspondences": a.n, "iterations": a.iters, "repetitions": a.reps, "estimator": "calibrated",
                     "priors": "the estimator's results, rotated by 1 degree, t and scale off by up to 2 %", "hopeless": "random poses"},
           "routes": {"p": "estimate_batch_torch, perturbed priors", "h": "estimate_batch_torch, hopeless priors", "e": "estimate_batch_torch, no priors"},
           "runs": []}
    for frac in a.outliers:
        b = synth.make_batch(0, a.batch, a.n, noise_px=0.5, depth_noise=0.02, outlier_frac=frac)
        t = [torch.from_numpy(b[k]).to(dev) for k in ("x1", "x2", "d1", "d2")]
        for schedule, min_it in (("fixed", a.iters), ("dynamic", min(a.dynamic_min, a.iters))):
            ro = {"max_iterations": a.iters, "min_iterations": min_it, "max_epipolar_error": 2.0, "max_reproj_error": 16.0}
            est, _ = poselib.estimate_batch_torch("calibrated", *t, CAM, CAM, ro, BO)
            rng = np.random.default_rng(5)
            good, bad = (torch.from_numpy(m.view(np.uint8).reshape(a.batch, -1).copy()).to(dev) for m in (perturb(est["model"], rng), hopeless(est["model"], rng)))
            routes = {"p": lambda: poselib.estimate_batch_torch("calibrated", *t, CAM, CAM, ro, BO, priors=good),
                      "h": lambda: poselib.estimate_batch_torch("calibrated", *t, CAM, CAM, ro, BO, priors=bad),
                      "e": lambda: poselib.estimate_batch_torch("calibrated", *t, CAM, CAM, ro, BO)}
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
            run = {"outlier_frac": frac, "schedule": schedule, "min_iterations": min_it}
            for k, v in times.items():
                v, r = np.array(v), last[k][0]
                run[k] = {"pairs_per_s_median": a.batch / float(np.median(v)), "ms_median": 1e3 * float(np.median(v)), "ms_min": 1e3 * float(v.min()),
                          "ms_max": 1e3 * float(v.max()), "spread_rel": float((v.max() - v.min()) / np.median(v)),
                          "inliers_mean": float(r["num_inliers"].mean()), "iterations_mean": float(r["iterations"].mean()),
                          "refinements_mean": float(r["refinements"].mean())}
            doc["runs"].append(run)
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
