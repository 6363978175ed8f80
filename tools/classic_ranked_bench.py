#!/usr/bin/env python3
"""What match-score order (PROSAC) costs and buys on the comparison rows: the 5-point and 7-point estimators at B = 1024 pairs, N = 2000
correspondences, 10^4 RANSAC iterations, and the 6-point estimator at B = 256, 10^3 iterations; correspondences and scores resident on the GPU, seeded
from synth, at 50 % and at 85 % outliers; the scores are -(outlier flag + N(0, 0.6)), as in tools/ranked_bench.py.

Three routes, warmed and alternated in one process, each timed with the host clock around a call that ends in the fetched result records:
  (r) poselib.estimate_baseline_batch_torch(scores = tensor): ranking, gather, progressive sampler, mask scatter;
  (s) poselib.estimate_baseline_batch_torch(scores = "presorted") on the pre-sorted records: the progressive sampler alone;
  (e) poselib.estimate_baseline_batch_torch on the pre-sorted records: today's uniform sampler.
Each under the fixed schedule (min_iterations = max_iterations) and under the dynamic rule (min_iterations = 100).  Reports the median of the
repetitions and their spread, and the mean inliers, iterations and LO counts each route ends with.  Last, the sampler alone through
mdrp_prosac_samples_k for K = 7, n = 2000, 10^4 samples in one chunk: max_prosac_iterations = 100000 (every sample progressive) against 1 (every
sample the uniform draw kc_samples<7> makes, through the same kernel), host clock around the call, which includes the table upload and the copy of
the samples back.  Writes profiles/classic_ranked_bench.json.

    python tools/classic_ranked_bench.py [--reps 21] [--out profiles/classic_ranked_bench.json]
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
# kind -> (pairs, iterations)
SHAPES = {"relpose_5pt": (1024, 10000), "fundamental_7pt": (1024, 10000), "shared_focal_6pt": (256, 1000)}


def inputs(kind, batch, n, frac):
    """(caller-order arrays, scores, the same arrays pre-sorted by descending score)"""
    from mdrp_amd import synth
    b = synth.make_batch(0, batch, n, noise_px=0.5, depth_noise=0.02, outlier_frac=frac, random_focal="shared" if kind == "shared_focal_6pt" else None)
    rng = np.random.default_rng(9)
    scores = -(np.stack([g["is_outlier"] for g in b["gt"]]).astype(np.float64) + rng.normal(0.0, 0.6, (batch, n)))
    order = np.argsort(-scores, axis=1, kind="stable")
    srt = {k: np.ascontiguousarray(np.take_along_axis(b[k], order[..., None], axis=1)) for k in ("x1", "x2")}
    return b, scores, srt


def sampler_alone(reps):
    from mdrp_amd import _capi
    h = _capi.default_handle(0)
    out = {"sample_size": 7, "n": 2000, "samples": 10000}
    for name, mp in (("progressive_ms_median", 100000), ("uniform_ms_median", 1)):
        ts = []
        for rep in range(reps + 2):
            t0 = time.perf_counter()
            h.prosac_samples_k(0, 2000, 7, mp, [10000])
            if rep >= 2:
                ts.append(time.perf_counter() - t0)
        out[name] = 1e3 * float(np.median(ts))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--dynamic-min", type=int, default=100)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--outliers", type=float, nargs="+", default=[0.5, 0.85])
    ap.add_argument("--kinds", nargs="+", default=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classic_ranked_bench.json"))
    a = ap.parse_args()
    import torch
    import mdrp_amd.poselib as poselib
    dev = torch.device("cuda", 0)
    doc = {"shape": {"correspondences": a.n, "repetitions": a.reps, "pairs_and_iterations": {k: SHAPES[k] for k in a.kinds},
                     "scores": "-(outlier flag + N(0, 0.6))", "max_prosac_iterations": 100000},
           "routes": {"r": "estimate_baseline_batch_torch, scores = tensor", "s": 'estimate_baseline_batch_torch, scores = "presorted", pre-sorted records',
                      "e": "estimate_baseline_batch_torch, pre-sorted records, uniform sampler"},
           "runs": []}
    for kind in a.kinds:
        batch, iters = SHAPES[kind]
        for frac in a.outliers:
            b, scores, srt = inputs(kind, batch, a.n, frac)
            t = [torch.from_numpy(b[k]).to(dev) for k in ("x1", "x2")]
            ts = [torch.from_numpy(srt[k]).to(dev) for k in ("x1", "x2")]
            sc = torch.from_numpy(scores).to(dev)
            for schedule, min_it in (("fixed", iters), ("dynamic", min(a.dynamic_min, iters))):
                ro = {"max_iterations": iters, "min_iterations": min_it, "max_epipolar_error": 2.0}
                routes = {"r": lambda: poselib.estimate_baseline_batch_torch(kind, *t, CAM, CAM, (0.0, 0.0), ro, BO, scores=sc),
                          "s": lambda: poselib.estimate_baseline_batch_torch(kind, *ts, CAM, CAM, (0.0, 0.0), ro, BO, scores="presorted"),
                          "e": lambda: poselib.estimate_baseline_batch_torch(kind, *ts, CAM, CAM, (0.0, 0.0), ro, BO)}
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
                run = {"kind": kind, "batch": batch, "iterations": iters, "outlier_frac": frac, "schedule": schedule, "min_iterations": min_it}
                for k, v in times.items():
                    v, r = np.array(v), last[k][0]
                    run[k] = {"pairs_per_s_median": batch / float(np.median(v)), "ms_median": 1e3 * float(np.median(v)), "ms_min": 1e3 * float(v.min()),
                              "ms_max": 1e3 * float(v.max()), "spread_rel": float((v.max() - v.min()) / np.median(v)),
                              "inliers_mean": float(r["num_inliers"].mean()), "iterations_mean": float(r["iterations"].mean()),
                              "refinements_mean": float(r["refinements"].mean())}
                doc["runs"].append(run)
                print(json.dumps(run), flush=True)
    doc["sampler_alone"] = sampler_alone(a.reps)
    print(json.dumps(doc["sampler_alone"]), flush=True)
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
