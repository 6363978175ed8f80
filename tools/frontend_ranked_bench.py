#!/usr/bin/env python3
"""What ranking inside the gather costs and saves at B = 1024 pairs, M = 2048 match rows of which 1850 to 2000 are
kept (the matches form keeps fewer than the image-pairs form: the result file records the count), 10^4 RANSAC iterations, calibrated estimator, at 50 % and at 85 % outliers.  Inputs as tools/frontend_bench.py makes them (float32
keypoints and depth maps, int64 matches with a ragged tail of -1 rows, resident on the GPU); one float32 score per MATCH ROW, as
tools/ranked_bench.py makes its scores: -(outlier flag + N(0, 0.6)), a matcher's confidence of middling quality.

Three routes, every shape warmed, alternated inside one process, each timed with the host clock around a call that ends in the fetched result
records and the mask on the match rows:
  (a) poselib.estimate_matches_torch(scores = S): k_gather_ranked, the progressive sampler, k_match_mask;
  (b) the route without it, on the same inputs: gather_matches_torch (one more stream synchronisation), S pushed through slot with torch
      indexing, estimate_batch_torch(scores =) — k_rank, k_rank_gather into the ordered copies, the run, k_rank_scatter —, the mask mapped back
      through slot with torch indexing;
  (c) poselib.estimate_matches_torch without scores: the uniform sampler on the match-ordered rows.
(a) and (b) must return the same records and the same mask.  The same three on the per-image form (--images images, pairs as image indices:
estimate_image_pairs_torch, gather_image_pairs_torch).  Reports medians, the spread of the repetitions of every route and (a) - (b) beside
the spread of (b); writes profiles/frontend_ranked_bench.json.

    python tools/frontend_ranked_bench.py [--batch 1024] [--rows 2048] [--iters 10000] [--reps 21] [--out profiles/frontend_ranked_bench.json]

--baseline KIND (relpose_5pt | shared_focal_6pt | fundamental_7pt): the three routes for a comparison row, which has no depths, on the
matches form: (a) poselib.estimate_baseline_matches_torch(scores = S) — k_gather_points_ranked, the progressive sampler, k_match_mask; (b) what a
caller writes without it — tools/frontend_bench.torch_point_front_end (torch indexing, the ordered compaction, the count copied to the host), S
pushed through slot, estimate_baseline_batch_torch(scores =), the mask mapped back; (c) estimate_baseline_matches_torch without scores.  Writes
under the key "baseline_<KIND>" of profiles/classic_frontend_ranked_bench.json unless --out says otherwise.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import frontend_bench as fb  # noqa: E402


def two_call_route(poselib, gather, estimate, scores):
    """route (b): gather() -> (x1, x2, d1, d2, n, slot); the scores and the mask go through slot by hand"""
    import torch
    x1, x2, d1, d2, n, slot = gather()
    B, M = slot.shape
    kept = slot >= 0
    at = torch.where(kept, slot, M).long()  # dropped rows land in a spare column
    gathered = torch.zeros((B, M + 1), dtype=scores.dtype, device=scores.device)
    gathered.scatter_(1, at, scores)
    res, mask = estimate(x1, x2, d1, d2, n, gathered[:, :M].contiguous())
    match_mask = torch.where(kept, torch.gather(mask, 1, at.clamp(max=M - 1)), 0).to(torch.uint8)
    return res, match_mask


def measure(routes, reps):
    import torch
    times = {k: [] for k in routes}
    last = {}
    for rep in range(reps + 2):  # two warm-up rounds of every route
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = fn()
            torch.cuda.synchronize()
            if rep >= 2:
                times[k].append(time.perf_counter() - t0)
    return times, last


def summarise(times, last, batch):
    run = {}
    for k, v in times.items():
        v, r = np.array(v), last[k][0]
        q1, q3 = np.percentile(v, [25, 75])
        run[k] = {"pairs_per_s_median": batch / float(np.median(v)), "ms_median": 1e3 * float(np.median(v)), "ms_min": 1e3 * float(v.min()),
                  "ms_max": 1e3 * float(v.max()), "ms_iqr": 1e3 * float(q3 - q1), "spread_rel": float((v.max() - v.min()) / np.median(v)),
                  "inliers_mean": float(r["num_inliers"].mean()), "iterations_mean": float(r["iterations"].mean())}
    run["a_minus_b_ms"] = run["a"]["ms_median"] - run["b"]["ms_median"]
    run["b_spread_ms"] = run["b"]["ms_max"] - run["b"]["ms_min"]
    run["a_minus_c_ms"] = run["a"]["ms_median"] - run["c"]["ms_median"]
    return run


def run_baseline(a):
    import torch
    import mdrp_amd.poselib as poselib
    dev = torch.device("cuda", 0)
    kind = a.baseline
    cam1, cam2, pp, centre = fb.baseline_arguments(kind)
    ro = {"max_iterations": a.iters, "min_iterations": a.iters, "max_epipolar_error": 2.0 * fb.A, "max_reproj_error": 16.0 * fb.A}
    doc = {"shape": {"batch": a.batch, "match_rows": a.rows, "keypoints": fb.K, "iterations": a.iters, "repetitions": a.reps, "estimator": kind,
                     "scores": "float32, -(outlier flag + N(0, 0.6)) per match row", "max_prosac_iterations": 100000},
           "routes": {"a": "estimate_baseline_matches_torch, scores = tensor",
                      "b": "torch-op front end with a host count, scores through slot, estimate_baseline_batch_torch(scores = tensor), mask through slot",
                      "c": "estimate_baseline_matches_torch without scores"},
           "runs": []}
    for frac in a.outliers:
        flags = []
        rng = np.random.default_rng(9)
        t = fb.make_inputs(a.batch, a.rows, dev, frac, flags, depth_maps=False)
        scores = torch.from_numpy((-(flags[0].astype(np.float64) + rng.normal(0.0, 0.6, flags[0].shape))).astype(np.float32)).to(dev)
        direct = lambda **kw: poselib.estimate_baseline_matches_torch(kind, *t, cam1, cam2, pp, ro, fb.BO, center1=centre, center2=centre, **kw)  # noqa: E731

        def gather():
            x1, x2, n, slot, keep = fb.torch_point_front_end(*t, centre)
            return x1, x2, None, None, n.cpu().numpy(), torch.where(keep, slot, -1)

        estimate = lambda x1, x2, d1, d2, n, sc: poselib.estimate_baseline_batch_torch(kind, x1, x2, cam1, cam2, pp, ro, fb.BO, n_per_pair=n, scores=sc)  # noqa: E731
        routes = {"a": lambda: direct(scores=scores)[:2], "b": lambda: two_call_route(poselib, gather, estimate, scores), "c": lambda: direct()[:2]}
        times, last = measure(routes, a.reps)
        assert last["a"][0].tobytes() == last["b"][0].tobytes(), "the records of (a) and (b) differ"
        assert torch.equal(last["a"][1], last["b"][1]), "the masks of (a) and (b) differ"
        run = {"form": "matches", "outlier_frac": frac, "kept_rows_mean": float(direct()[2].mean())}
        run.update(summarise(times, last, a.batch))
        doc["runs"].append(run)
        print(json.dumps(run), flush=True)
        del routes, direct, scores, t
        torch.cuda.empty_cache()
    out = a.out or os.path.join(ROOT, "profiles", "classic_frontend_ranked_bench.json")
    if out != "/dev/null":
        whole = json.load(open(out)) if os.path.exists(out) else {}
        whole["baseline_" + kind] = doc
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(whole, open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--outliers", type=float, nargs="+", default=[0.5, 0.85])
    ap.add_argument("--images", type=int, default=46)
    ap.add_argument("--forms", nargs="+", choices=["matches", "image_pairs"], default=["matches", "image_pairs"])
    ap.add_argument("--baseline", choices=fb.BASELINES, default=None, help="the routes for a comparison row, without depth maps (see above)")
    ap.add_argument("--out", default=None, help="default: profiles/frontend_ranked_bench.json (--baseline: profiles/classic_frontend_ranked_bench.json)")
    a = ap.parse_args()
    if a.baseline:
        return run_baseline(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "frontend_ranked_bench.json")
    import torch
    import mdrp_amd.poselib as poselib
    dev = torch.device("cuda", 0)
    CAM, BO = fb.CAM, fb.BO
    ro = {"max_iterations": a.iters, "min_iterations": a.iters, "max_epipolar_error": 2.0 * fb.A, "max_reproj_error": 16.0 * fb.A}
    doc = {"shape": {"batch": a.batch, "match_rows": a.rows, "keypoints": fb.K, "depth_map": [fb.H, fb.W], "iterations": a.iters, "repetitions": a.reps,
                     "estimator": "calibrated", "scores": "float32, -(outlier flag + N(0, 0.6)) per match row", "max_prosac_iterations": 100000,
                     "images": a.images},
           "routes": {"a": "estimate_matches_torch / estimate_image_pairs_torch, scores = tensor",
                      "b": "gather_*_torch, scores through slot, estimate_batch_torch(scores = tensor), mask through slot",
                      "c": "estimate_matches_torch / estimate_image_pairs_torch without scores"},
           "runs": []}
    for form in a.forms:
        for frac in a.outliers:
            flags = []
            rng = np.random.default_rng(9)
            if form == "matches":
                t = fb.make_inputs(a.batch, a.rows, dev, frac, flags)
                is_out = flags[0]
                gather = lambda: poselib.gather_matches_torch(*t)  # noqa: E731
                direct = lambda **kw: poselib.estimate_matches_torch("calibrated", *t, CAM, CAM, ro, BO, **kw)  # noqa: E731
            else:
                kp, dm, pairs, matches = fb.make_image_inputs(a.images, a.batch, a.rows, dev, frac, flags)
                is_out = np.stack(flags)
                gather = lambda: poselib.gather_image_pairs_torch(kp, dm, pairs, matches)  # noqa: E731
                direct = lambda **kw: poselib.estimate_image_pairs_torch("calibrated", kp, dm, pairs, matches, CAM, ro, BO, **kw)  # noqa: E731
            scores = torch.from_numpy((-(is_out.astype(np.float64) + rng.normal(0.0, 0.6, is_out.shape))).astype(np.float32)).to(dev)
            estimate = lambda x1, x2, d1, d2, n, sc: poselib.estimate_batch_torch("calibrated", x1, x2, d1, d2, CAM, CAM, ro, BO, n_per_pair=n, scores=sc)  # noqa: E731
            routes = {"a": lambda: direct(scores=scores)[:2], "b": lambda: two_call_route(poselib, gather, estimate, scores), "c": lambda: direct()[:2]}
            times, last = measure(routes, a.reps)
            assert last["a"][0].tobytes() == last["b"][0].tobytes(), "the records of (a) and (b) differ"
            assert torch.equal(last["a"][1], last["b"][1]), "the masks of (a) and (b) differ"
            run = {"form": form, "outlier_frac": frac, "kept_rows_mean": float(direct()[2].mean())}
            run.update(summarise(times, last, a.batch))
            doc["runs"].append(run)
            print(json.dumps(run), flush=True)
            del routes, gather, direct, scores
            if form == "matches":
                del t
            else:
                del kp, dm, matches
            torch.cuda.empty_cache()
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
