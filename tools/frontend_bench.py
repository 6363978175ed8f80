#!/usr/bin/env python3
"""What the device front end costs and saves at the headline shape (B = 1024 pairs, M = 2000 match rows, 10^4 RANSAC iterations, calibrated
estimator): float32 keypoints (B, 2048, 2), float32 depth maps (B, 480, 640) and int64 matches, resident on the GPU, seeded from synth.

Three routes, warmed and alternated in one process, each timed with the host clock around a call that ends in the fetched result records:
  (a) torch_front_end + poselib.estimate_batch_torch — the route a user has without the front end, in torch ops: gathers, masks, an ordered
      compaction by cumulative sum + scatter, casts to float64, the count copied to the host, and the inlier mask mapped back onto the rows;
  (b) poselib.estimate_matches_torch;
  (c) poselib.estimate_batch_torch alone on input gathered beforehand — the floor.
Reports the median of the repetitions and their spread, checks that (a) and (b) return the same records, and writes profiles/frontend_bench.json.

    python tools/frontend_bench.py [--batch 1024] [--rows 2000] [--iters 10000] [--reps 21] [--out profiles/frontend_bench.json]
The front end's own kernel time comes from a separate run under the profiler, folded into the same file afterwards:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/frontend_bench.py --only b --reps 3 --out /dev/null
    python tools/frontend_bench.py --kernel-stats <dir>/**/*_kernel_stats.csv --out profiles/frontend_bench.json

--image-pairs: the same 1024-pair batch as its producer holds it — 46 images (1035 possible pairs), one keypoint table and one depth map per
image, the pairs as image indices — through poselib.estimate_image_pairs_torch (route "i"), against the unchanged estimate_matches_torch on the
per-pair expansion of the same data (route "e": every image's tables copied once per pair it takes part in, built before the clock starts).
Checks that both return the same records, records the bytes of input each route holds, and writes under the key "image_pairs" of the same file.

--baseline KIND (relpose_5pt | shared_focal_6pt | fundamental_7pt): the same three routes for a comparison row, which has no depths (DESIGN.md
7g) — (a) torch_point_front_end (torch indexing, the finite test, the ordered compaction, the count copied to the host) +
estimate_baseline_batch_torch, (b) poselib.estimate_baseline_matches_torch, (c) estimate_baseline_batch_torch on input gathered beforehand.  No
depth maps are made.  Writes under the key "baseline_<KIND>" of profiles/classic_frontend_bench.json unless --out says otherwise.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, K = 480, 640, 2048
A, C = 0.38, (320.0, 240.0)  # map pixel = A * synth pixel + C: a camera with focal A * 800 and principal point C
CAM = {"model": "SIMPLE_PINHOLE", "width": W, "height": H, "params": [A * 800.0, *C]}
BO = {"loss_type": "TRUNCATED_CAUCHY"}


def make_inputs(batch, rows, dev, outlier_frac=0.5, outlier_flags=None, depth_maps=True):
    """matcher-shaped inputs on the device: keypoint tables with the correspondences scattered through a permutation, their depths painted
    into the maps, a tail of -1 padding rows of a different length per pair (LightGlue pads ragged match lists that way).  outlier_flags: a
    list that receives the (batch, rows) outlier flags of the match rows (tools/frontend_ranked_bench.py makes its scores from them).
    depth_maps=False: keypoints and matches alone (the baselines' front end)."""
    import torch
    from mdrp_amd import synth
    rng = np.random.default_rng(5)
    b = synth.make_batch(0, batch, rows, noise_px=0.5, depth_noise=0.02, outlier_frac=outlier_frac)
    if outlier_flags is not None:
        outlier_flags.append(np.stack([g["is_outlier"] for g in b["gt"]]))
    kp1 = np.stack([rng.uniform(0, W, (batch, K)), rng.uniform(0, H, (batch, K))], 2)
    kp2 = kp1.copy()
    matches = np.full((batch, rows, 2), -1, dtype=np.int64)
    pt1 = A * b["x1"] + np.array(C)
    pt2 = A * b["x2"] + np.array(C)
    live = rows - rng.integers(0, rows // 20 + 1, batch)  # up to 5 % padding rows
    for k in range(batch):
        p1, p2 = rng.permutation(K)[:rows], rng.permutation(K)[:rows]
        kp1[k, p1] = pt1[k]; kp2[k, p2] = pt2[k]
        matches[k, :live[k], 0] = p1[:live[k]]; matches[k, :live[k], 1] = p2[:live[k]]
    if not depth_maps:
        return torch.from_numpy(kp1.astype(np.float32)).to(dev), torch.from_numpy(kp2.astype(np.float32)).to(dev), torch.from_numpy(matches).to(dev)
    g = torch.Generator(device=dev); g.manual_seed(5)
    dm1 = torch.rand((batch, H, W), device=dev, generator=g) * 5 + 1
    dm2 = torch.rand((batch, H, W), device=dev, generator=g) * 5 + 1
    for dm, pt, d in ((dm1, pt1, b["d1"]), (dm2, pt2, b["d2"])):
        inside = (pt[..., 0] > -1) & (pt[..., 0] < W) & (pt[..., 1] > -1) & (pt[..., 1] < H)
        bi, mi = np.nonzero(inside)
        dm[torch.from_numpy(bi).to(dev), torch.from_numpy(pt[bi, mi, 1].astype(np.int64)).to(dev),
           torch.from_numpy(pt[bi, mi, 0].astype(np.int64)).to(dev)] = torch.from_numpy(d[bi, mi].astype(np.float32)).to(dev)
    dm1[:, ::7, ::5] = float("inf")   # a depth network's invalid pixels, in both maps: some rows have both depths infinite
    dm2[:, ::3, ::5] = float("inf")
    return (torch.from_numpy(kp1.astype(np.float32)).to(dev), torch.from_numpy(kp2.astype(np.float32)).to(dev), torch.from_numpy(matches).to(dev), dm1, dm2)


def torch_front_end(kp1, kp2, matches, dm1, dm2):
    """the reference scripts' preparation (gather, depth at the truncated pixel, drop inf & inf) in batched torch ops, order preserved"""
    import torch
    B, M, _ = matches.shape
    i, j = matches[..., 0], matches[..., 1]
    valid = (i >= 0) & (j >= 0) & (i < kp1.shape[1]) & (j < kp2.shape[1])
    p1 = torch.gather(kp1, 1, i.clamp(0, kp1.shape[1] - 1).unsqueeze(-1).expand(-1, -1, 2))
    p2 = torch.gather(kp2, 1, j.clamp(0, kp2.shape[1] - 1).unsqueeze(-1).expand(-1, -1, 2))

    def depth(p, dm):
        h, w = dm.shape[1:]
        x, y = p[..., 0], p[..., 1]
        inside = (x > -1) & (x < w) & (y > -1) & (y < h)
        flat = torch.where(inside, y.long() * w + x.long(), 0)
        return inside, torch.gather(dm.reshape(B, -1), 1, flat)

    in1, d1 = depth(p1, dm1)
    in2, d2 = depth(p2, dm2)
    keep = valid & in1 & in2 & ~(torch.isinf(d1) & torch.isinf(d2))
    count = torch.cumsum(keep, dim=1)
    n = count[:, -1].to(torch.int32)
    slot = torch.where(keep, count - 1, M)  # dropped rows land in a spare column
    x1 = torch.zeros((B, M + 1, 2), dtype=torch.float64, device=kp1.device); x2 = torch.zeros_like(x1)
    e1 = torch.ones((B, M + 1), dtype=torch.float64, device=kp1.device); e2 = torch.ones_like(e1)
    s2 = slot.unsqueeze(-1).expand(-1, -1, 2)
    x1.scatter_(1, s2, p1.double()); x2.scatter_(1, s2, p2.double())
    e1.scatter_(1, slot, d1.double()); e2.scatter_(1, slot, d2.double())
    x1[:, M] = 0.0; x2[:, M] = 0.0  # (not read: n <= M)
    return x1[:, :M].contiguous(), x2[:, :M].contiguous(), e1[:, :M].contiguous(), e2[:, :M].contiguous(), n, slot, keep


def route_a(poselib, t, ro):
    import torch
    x1, x2, d1, d2, n, slot, keep = torch_front_end(*t)
    res, mask = poselib.estimate_batch_torch("calibrated", x1, x2, d1, d2, CAM, CAM, ro, BO, n_per_pair=n.cpu().numpy())
    match_mask = torch.where(keep, torch.gather(mask, 1, slot.clamp(max=mask.shape[1] - 1)), 0).to(torch.uint8)
    return res, match_mask


def route_b(poselib, t, ro):
    res, match_mask, _ = poselib.estimate_matches_torch("calibrated", *t, CAM, CAM, ro, BO)
    return res, match_mask


# ---- the comparison rows (5- / 6- / 7-point), which have no depths
BASELINES = ("relpose_5pt", "shared_focal_6pt", "fundamental_7pt")


def baseline_arguments(kind):
    """(cameras1, cameras2, pp, centre) of a baseline on make_inputs' keypoints: cameras for the 5-point kind, principal-point-centred pixels and
    pp = (0, 0) for the 6-point kind, nothing for the 7-point kind"""
    if kind == "relpose_5pt":
        return CAM, CAM, None, None
    return None, None, ((0.0, 0.0) if kind == "shared_focal_6pt" else None), (C if kind == "shared_focal_6pt" else None)


def torch_point_front_end(kp1, kp2, matches, centre=None):
    """the baselines' preparation in batched torch ops, order preserved: kp[matches], drop padding, bad indices and non-finite coordinates, compact"""
    import torch
    B, M, _ = matches.shape
    i, j = matches[..., 0], matches[..., 1]
    valid = (i >= 0) & (j >= 0) & (i < kp1.shape[1]) & (j < kp2.shape[1])
    p1 = torch.gather(kp1, 1, i.clamp(0, kp1.shape[1] - 1).unsqueeze(-1).expand(-1, -1, 2)).double()
    p2 = torch.gather(kp2, 1, j.clamp(0, kp2.shape[1] - 1).unsqueeze(-1).expand(-1, -1, 2)).double()
    keep = valid & torch.isfinite(p1).all(-1) & torch.isfinite(p2).all(-1)
    if centre is not None:
        c = torch.tensor(centre, dtype=torch.float64, device=kp1.device)
        p1, p2 = p1 - c, p2 - c
    count = torch.cumsum(keep, dim=1)
    n = count[:, -1].to(torch.int32)
    slot = torch.where(keep, count - 1, M)  # dropped rows land in a spare column
    x1 = torch.zeros((B, M + 1, 2), dtype=torch.float64, device=kp1.device); x2 = torch.zeros_like(x1)
    s2 = slot.unsqueeze(-1).expand(-1, -1, 2)
    x1.scatter_(1, s2, p1); x2.scatter_(1, s2, p2)
    x1[:, M] = 0.0; x2[:, M] = 0.0  # (not read: n <= M)
    return x1[:, :M].contiguous(), x2[:, :M].contiguous(), n, slot, keep


def time_routes(routes, reps):
    """every route warmed twice, then alternated: ({route: seconds of every repetition}, {route: its last result})"""
    import torch
    times = {k: [] for k in routes}
    last = {}
    for rep in range(reps + 2):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = fn()
            torch.cuda.synchronize()
            if rep >= 2:
                times[k].append(time.perf_counter() - t0)
    return times, last


def run_baseline(a):
    import torch
    import mdrp_amd.poselib as poselib
    from mdrp_amd import frontend
    dev = torch.device("cuda", 0)
    kind = a.baseline
    cam1, cam2, pp, centre = baseline_arguments(kind)
    ro = {"max_iterations": a.iters, "min_iterations": a.iters, "max_epipolar_error": 2.0 * A, "max_reproj_error": 16.0 * A}
    t = make_inputs(a.batch, a.rows, dev, depth_maps=False)
    gx1, gx2, gn, gslot = poselib.gather_point_matches_torch(*t, center1=centre, center2=centre)
    ta = torch_point_front_end(*t, centre)  # the two front ends agree, and both agree with the NumPy statement on the first pairs
    assert np.array_equal(ta[2].cpu().numpy(), gn) and torch.equal(ta[0], gx1) and torch.equal(ta[1], gx2)
    for k in range(2):
        ref = frontend.gather_point_matches_numpy(*(v[k].cpu().numpy() for v in t), centre, centre)
        assert len(ref[0]) == gn[k] and gx2[k, :gn[k]].cpu().numpy().tobytes() == ref[1].tobytes() and gslot[k].cpu().numpy().tobytes() == ref[2].tobytes()

    def route_a():
        x1, x2, n, slot, keep = torch_point_front_end(*t, centre)
        res, mask = poselib.estimate_baseline_batch_torch(kind, x1, x2, cam1, cam2, pp, ro, BO, n_per_pair=n.cpu().numpy())
        return res, torch.where(keep, torch.gather(mask, 1, slot.clamp(max=mask.shape[1] - 1)), 0).to(torch.uint8)

    routes = {"a": route_a, "b": lambda: poselib.estimate_baseline_matches_torch(kind, *t, cam1, cam2, pp, ro, BO, center1=centre, center2=centre)[:2],
              "c": lambda: poselib.estimate_baseline_batch_torch(kind, gx1, gx2, cam1, cam2, pp, ro, BO, n_per_pair=gn)}
    times, last = time_routes(routes, a.reps)
    assert last["a"][0].tobytes() == last["b"][0].tobytes() == last["c"][0].tobytes(), "the routes' records differ"
    assert torch.equal(last["a"][1], last["b"][1])
    doc = {"shape": {"batch": a.batch, "match_rows": a.rows, "keypoints": K, "iterations": a.iters, "repetitions": a.reps, "kept_rows_mean": float(gn.mean()),
                     "estimator": kind, "inliers_mean": float(last["b"][0]["num_inliers"].mean())},
           "routes": {"a": "torch-op front end + estimate_baseline_batch_torch", "b": "estimate_baseline_matches_torch",
                      "c": "estimate_baseline_batch_torch on gathered input"}}
    for k, v in times.items():
        v = np.array(v)
        doc[k] = {"pairs_per_s_median": a.batch / float(np.median(v)), "ms_median": 1e3 * float(np.median(v)), "ms_min": 1e3 * float(v.min()),
                  "ms_max": 1e3 * float(v.max()), "spread_rel": float((v.max() - v.min()) / np.median(v))}
    doc["front_end_ms"] = {"a_minus_c": doc["a"]["ms_median"] - doc["c"]["ms_median"], "b_minus_c": doc["b"]["ms_median"] - doc["c"]["ms_median"]}
    if a.out != "/dev/null":
        whole = json.load(open(a.out)) if os.path.exists(a.out) else {}
        whole["baseline_" + kind] = doc
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(whole, open(a.out, "w"), indent=1)
    print(json.dumps({"baseline_" + kind: doc}))


def make_image_inputs(n_images, batch, rows, dev, outlier_frac=0.5, outlier_flags=None):
    """one scene seen by n_images cameras: K world points projected into every image (each image's table in an order of its own), the depth
    of every visible point painted into that image's one map, and for the first `batch` of the image pairs a match list over `rows` of the
    points, half of the rows (outlier_frac) mismatched, with a tail of -1 padding rows; outlier_flags as in make_inputs.  Returns the device tensors (keypoints (I, K, 2) float32, depth maps
    (I, H, W) float32, pairs (B, 2) int32 on the host, matches (B, rows, 2) int64)."""
    import itertools
    import torch
    rng = np.random.default_rng(6)
    f = A * 800.0
    world = np.stack([rng.uniform(-2.2, 2.2, K), rng.uniform(-1.6, 1.6, K), rng.uniform(3.0, 8.0, K)], 1)
    kp = np.zeros((n_images, K, 2))
    order = np.zeros((n_images, K), dtype=np.int64)  # order[i][p]: where point p sits in image i's table
    g = torch.Generator(device=dev); g.manual_seed(6)
    dm = torch.rand((n_images, H, W), device=dev, generator=g) * 5 + 1
    for i in range(n_images):
        w = rng.normal(0, 0.05, 3)  # a small rotation (Rodrigues) and a small translation per camera
        th = np.linalg.norm(w)
        kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
        rot = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx
        cam = world @ rot.T + rng.normal(0, 0.3, 3)
        px = f * cam[:, :2] / cam[:, 2:] + np.array(C) + rng.normal(0, 0.5, (K, 2))
        order[i] = rng.permutation(K)
        kp[i, order[i]] = px
        inside = (px[:, 0] > -1) & (px[:, 0] < W) & (px[:, 1] > -1) & (px[:, 1] < H)
        dm[i, torch.from_numpy(px[inside, 1].astype(np.int64)).to(dev), torch.from_numpy(px[inside, 0].astype(np.int64)).to(dev)] = \
            torch.from_numpy((cam[inside, 2] * (1 + rng.normal(0, 0.02, int(inside.sum())))).astype(np.float32)).to(dev)
    dm[:, ::7, ::5] = float("inf")  # a depth network's invalid pixels
    pairs = np.array(list(itertools.combinations(range(n_images), 2))[:batch], dtype=np.int32)
    assert len(pairs) == batch, f"{n_images} images give {n_images * (n_images - 1) // 2} pairs, fewer than {batch}"
    matches = np.full((batch, rows, 2), -1, dtype=np.int64)
    live = rows - rng.integers(0, rows // 20 + 1, batch)  # up to 5 % padding rows
    for b, (i, j) in enumerate(pairs):
        pts = rng.permutation(K)[:rows]
        other = pts.copy()
        wrong = rng.random(rows) < outlier_frac
        if outlier_flags is not None:
            outlier_flags.append(wrong)
        other[wrong] = rng.permutation(pts[wrong])  # outliers: a point matched to another point's keypoint
        matches[b, :live[b], 0] = order[i][pts[:live[b]]]
        matches[b, :live[b], 1] = order[j][other[:live[b]]]
    return torch.from_numpy(kp.astype(np.float32)).to(dev), dm, pairs, torch.from_numpy(matches).to(dev)


def tensor_bytes(*tensors):
    return int(sum(t.numel() * t.element_size() for t in tensors))


def run_image_pairs(a):
    """route "i" (estimate_image_pairs_torch on the per-image tables) against route "e" (estimate_matches_torch on their per-pair expansion)"""
    import torch
    import mdrp_amd.poselib as poselib
    dev = torch.device("cuda", 0)
    ro = {"max_iterations": a.iters, "min_iterations": a.iters, "max_epipolar_error": 2.0 * A, "max_reproj_error": 16.0 * A}
    kp, dm, pairs, matches = make_image_inputs(a.images, a.batch, a.rows, dev)
    pairs_dev = torch.from_numpy(pairs).to(dev)
    ia, ic = pairs_dev[:, 0].long(), pairs_dev[:, 1].long()
    expanded = (kp[ia], kp[ic], matches, dm[ia], dm[ic])  # what a caller of estimate_matches_torch has to build and hold
    routes = {"i": lambda: poselib.estimate_image_pairs_torch("calibrated", kp, dm, pairs, matches, CAM, ro, BO),
              "e": lambda: poselib.estimate_matches_torch("calibrated", *expanded, CAM, CAM, ro, BO)}
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
    assert last["i"][0].tobytes() == last["e"][0].tobytes(), "the routes' records differ"
    assert torch.equal(last["i"][1], last["e"][1]) and np.array_equal(last["i"][2], last["e"][2])
    doc = {"shape": {"images": a.images, "batch": a.batch, "match_rows": a.rows, "keypoints": K, "depth_map": [H, W], "iterations": a.iters,
                     "repetitions": a.reps, "kept_rows_mean": float(last["i"][2].mean()), "inlier_ratio_mean": float(last["i"][0]["inlier_ratio"].mean()),
                     "estimator": "calibrated"},
           "routes": {"i": "estimate_image_pairs_torch on per-image tables", "e": "estimate_matches_torch on the per-pair expansion (built beforehand)"},
           "input_bytes": {"i": tensor_bytes(kp, dm, pairs_dev, matches), "e": tensor_bytes(*expanded)}}
    for k, v in times.items():
        v = np.array(v)
        doc[k] = {"pairs_per_s_median": a.batch / float(np.median(v)), "ms_median": 1e3 * float(np.median(v)), "ms_min": 1e3 * float(v.min()),
                  "ms_max": 1e3 * float(v.max()), "spread_rel": float((v.max() - v.min()) / np.median(v))}
    if a.out != "/dev/null":
        whole = json.load(open(a.out)) if os.path.exists(a.out) else {}
        whole["image_pairs"] = doc
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(whole, open(a.out, "w"), indent=1)
    print(json.dumps({"image_pairs": doc}))


def fold_kernel_stats(paths, out):
    """average duration of the front end's kernels from rocprofv3's kernel statistics into the result file"""
    rows = {}
    for p in paths:
        for r in csv.DictReader(open(p)):
            name = r.get("Name") or r.get("KernelName") or ""
            for key in ("k_gather", "k_match_mask"):
                if key in name:
                    rows[key] = {"name": name, "calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                                 "max_us": float(r["MaxNs"]) / 1e3}
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["front_end_kernels"] = rows
    json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None, help="run one route alone (profiler runs)")
    ap.add_argument("--image-pairs", action="store_true", help="the batch as pairs of image indices into --images images (see above)")
    ap.add_argument("--images", type=int, default=46)
    ap.add_argument("--baseline", choices=BASELINES, default=None, help="the routes for a comparison row, without depth maps (see above)")
    ap.add_argument("--out", default=None, help="default: profiles/frontend_bench.json (--baseline: profiles/classic_frontend_bench.json)")
    ap.add_argument("--kernel-stats", nargs="+", default=None, help="rocprofv3 *_kernel_stats.csv files (globs allowed) to fold into --out")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "classic_frontend_bench.json" if a.baseline else "frontend_bench.json")
    if a.kernel_stats:
        return fold_kernel_stats([p for g in a.kernel_stats for p in glob.glob(g, recursive=True)], a.out)
    if a.image_pairs:
        return run_image_pairs(a)
    if a.baseline:
        return run_baseline(a)
    import torch
    import mdrp_amd.poselib as poselib
    from mdrp_amd import frontend
    dev = torch.device("cuda", 0)
    ro = {"max_iterations": a.iters, "min_iterations": a.iters, "max_epipolar_error": 2.0 * A, "max_reproj_error": 16.0 * A}
    t = make_inputs(a.batch, a.rows, dev)
    gx1, gx2, gd1, gd2, gn, _ = poselib.gather_matches_torch(*t)
    routes = {"a": lambda: route_a(poselib, t, ro), "b": lambda: route_b(poselib, t, ro),
              "c": lambda: poselib.estimate_batch_torch("calibrated", gx1, gx2, gd1, gd2, CAM, CAM, ro, BO, n_per_pair=gn)}
    if a.only:
        routes = {a.only: routes[a.only]}
    else:  # the two front ends agree, and both agree with the NumPy statement on the first pairs
        ta = torch_front_end(*t)
        assert np.array_equal(ta[4].cpu().numpy(), gn) and torch.equal(ta[0], gx1) and torch.equal(ta[3], gd2)
        for k in range(2):
            ref = frontend.gather_matches_numpy(*(v[k].cpu().numpy() for v in t))
            assert len(ref[2]) == gn[k] and gx2[k, :gn[k]].cpu().numpy().tobytes() == ref[1].tobytes()
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
    if not a.only:
        assert last["a"][0].tobytes() == last["b"][0].tobytes() == last["c"][0].tobytes(), "the routes' records differ"
        assert torch.equal(last["a"][1], last["b"][1])
    doc = {"shape": {"batch": a.batch, "match_rows": a.rows, "keypoints": K, "depth_map": [H, W], "iterations": a.iters, "repetitions": a.reps,
                     "kept_rows_mean": float(gn.mean()), "estimator": "calibrated"},
           "routes": {"a": "torch-op front end + estimate_batch_torch", "b": "estimate_matches_torch", "c": "estimate_batch_torch on gathered input"}}
    for k, v in times.items():
        v = np.array(v)
        doc[k] = {"pairs_per_s_median": a.batch / float(np.median(v)), "ms_median": 1e3 * float(np.median(v)), "ms_min": 1e3 * float(v.min()),
                  "ms_max": 1e3 * float(v.max()), "spread_rel": float((v.max() - v.min()) / np.median(v))}
    if not a.only:
        doc["front_end_ms"] = {"a_minus_c": doc["a"]["ms_median"] - doc["c"]["ms_median"], "b_minus_c": doc["b"]["ms_median"] - doc["c"]["ms_median"]}
    if a.out != "/dev/null":
        old = json.load(open(a.out)) if os.path.exists(a.out) else {}
        if "front_end_kernels" in old:
            doc["front_end_kernels"] = old["front_end_kernels"]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
