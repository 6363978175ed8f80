#!/usr/bin/env python3
"""What refining caller-supplied models costs beside estimating from nothing, at the headline shape (B = 1024 pairs, N = 2000 correspondences,
calibrated estimator, 10^4 RANSAC iterations for the estimator): correspondences and models resident on the GPU, seeded from synth.

The start models are the estimator's own results on the same pairs, perturbed by 1 degree in the rotation and 2 % in the translation and the
scale (a pose from the previous video frame, or from a coarse first pass).  Three routes, warmed and alternated in one process, each timed
with the host clock around a call that ends in the fetched result records:
  (a) poselib.refine_batch_torch, default stages (LO + inlier-only refinement);
  (b) poselib.refine_batch_torch, stages = 0 (verification: score and inlier mask only);
  (c) poselib.estimate_batch_torch — the existing call the two are compared with.
Reports the median of the repetitions and their spread, and how many inliers each route ends with; writes profiles/from_models_bench.json.

    python tools/from_models_bench.py [--batch 1024] [--n 2000] [--iters 10000] [--reps 21] [--out profiles/from_models_bench.json]
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


def quat_mul(a, b):
    w1, x1, y1, z1 = a.T
    w2, x2, y2, z2 = b.T
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], 1)


def perturb(models, rng, deg=1.0, frac=0.02):
    """the records' models rotated by `deg` degrees about a random axis, translation and scale off by up to `frac`"""
    out = models.copy()
    axis = rng.normal(0.0, 1.0, (len(out), 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    half = np.radians(deg) / 2.0
    out["q"] = quat_mul(np.c_[np.full(len(out), np.cos(half)), np.sin(half) * axis], models["q"])
    out["t"] = models["t"] * (1.0 + frac * rng.uniform(-1.0, 1.0, (len(out), 3)))
    out["scale"] = models["scale"] * (1.0 + frac * rng.uniform(-1.0, 1.0, len(out)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "from_models_bench.json"))
    a = ap.parse_args()
    import torch
    import mdrp_amd.poselib as poselib
    from mdrp_amd import synth
    dev = torch.device("cuda", 0)
    ro = {"max_iterations": a.iters, "min_iterations": a.iters, "max_epipolar_error": 2.0, "max_reproj_error": 16.0}
    b = synth.make_batch(0, a.batch, a.n, noise_px=0.5, depth_noise=0.02, outlier_frac=0.5)
    t = [torch.from_numpy(b[k]).to(dev) for k in ("x1", "x2", "d1", "d2")]
    est, _ = poselib.estimate_batch_torch("calibrated", *t, CAM, CAM, ro, BO)
    start = perturb(est["model"], np.random.default_rng(5))
    models = torch.from_numpy(start.view(np.uint8).reshape(a.batch, -1).copy()).to(dev)
    routes = {"a": lambda: poselib.refine_batch_torch("calibrated", *t, models, CAM, CAM, ro, BO),
              "b": lambda: poselib.refine_batch_torch("calibrated", *t, models, CAM, CAM, ro, BO, stages=0),
              "c": lambda: poselib.estimate_batch_torch("calibrated", *t, CAM, CAM, ro, BO)}
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
    doc = {"shape": {"batch": a.batch, "correspondences": a.n, "iterations": a.iters, "repetitions": a.reps, "estimator": "calibrated",
                     "start_models": "the estimator's results, rotated by 1 degree, t and scale off by up to 2 %"},
           "routes": {"a": "refine_batch_torch, stages = LO | INLIERS", "b": "refine_batch_torch, stages = 0", "c": "estimate_batch_torch"},
           "inliers_mean": {"start_models": float(last["b"][0]["num_inliers"].mean()), "a": float(last["a"][0]["num_inliers"].mean()),
                            "c": float(last["c"][0]["num_inliers"].mean())}}
    for k, v in times.items():
        v = np.array(v)
        doc[k] = {"pairs_per_s_median": a.batch / float(np.median(v)), "ms_median": 1e3 * float(np.median(v)), "ms_min": 1e3 * float(v.min()),
                  "ms_max": 1e3 * float(v.max()), "spread_rel": float((v.max() - v.min()) / np.median(v))}
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
