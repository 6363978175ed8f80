#!/usr/bin/env python3
"""What the back end costs against the route a torch user has without it, on the same tensors: B pairs of 480 x 640 float32 depth maps
resident on the device, the varying-focal kind, one model per pair.  Three cases: 1 pair and 1024 pairs at rate 0.05 (the video loop and the batch), and
64 pairs at rate 1.  Two routes alternate within every repetition, each ending with the stream drained:
    reconstruct   poselib.reconstruct_pairs_torch: points, pixel and counts on the device
    torch         per image: broadcast unprojection of every pixel to a (B, H, W, 3) tensor, the mask (subsample & not infinite), torch.nonzero, index;
                  image 1's kept points rotated, translated and divided by the scale with the pair's R, t, scale gathered by the kept rows' pair
The torch route is handed the subsample's candidate mask ready-made (the hash of R3 evaluated once, outside the timed region: it depends on the shape
and the seed alone and a caller could keep it), so that both routes keep the SAME pixels, which is checked before anything is timed: the counts and the
kept pixels of every pair are equal, and the points agree to float32 rounding (the torch route computes in float32).
Medians of --reps repetitions (21 by default) after a warm-up of every route with their spreads, and the peak device memory of each route above the
resident inputs (torch's allocator's peak; the library's own scratch is outside that allocator and is added from its sizes), written to
profiles/recon_bench.json.
    python tools/recon_bench.py [--reps 21] [--out profiles/recon_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mdrp_amd import _capi, frontend, poselib, reconstruct  # noqa: E402

H, W, SEED = 480, 640, 7
CASES = (("1_pair_rate_0.05", 1, 0.05), ("1024_pairs_rate_0.05", 1024, 0.05), ("64_pairs_rate_1", 64, 1.0))


def make_inputs(B, dev):
    g = torch.Generator(device=dev).manual_seed(B)
    dm = []
    for _ in range(2):
        d = torch.rand((B, H, W), generator=g, device=dev) * 9.0 + 1.0
        d[torch.rand((B, H, W), generator=g, device=dev) < 0.03] = float("inf")
        dm.append(d)
    rng = np.random.default_rng(B)
    m = np.zeros(B, dtype=_capi.MODEL_DTYPE)
    q = rng.normal(size=(B, 4))
    m["q"], m["t"], m["scale"] = q / np.linalg.norm(q, axis=1, keepdims=True), rng.normal(size=(B, 3)), rng.uniform(0.5, 2.0, size=B)
    m["f1"], m["f2"] = rng.uniform(400.0, 700.0, size=B), rng.uniform(400.0, 700.0, size=B)
    models = torch.from_numpy(m.view(np.float64).reshape(B, 12).copy()).to(dev)
    centre = torch.tensor([W / 2.0, H / 2.0], dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    return dm, m, models, centre


def candidate_masks(rate, dev):
    thr = frontend.recon_threshold(rate)
    return [torch.from_numpy(frontend.recon_candidates(H, W, thr, SEED, stage)).to(dev) for stage in frontend.RECON_STAGES]


def torch_route(dm, m_dev, centre, masks):
    """(points1 (n1, 3), rows1 (n1, 3) = (pair, v, u), points2, rows2) in float32"""
    B = dm[0].shape[0]
    dev = dm[0].device
    q, t, scale = m_dev[:, :4].float(), m_dev[:, 4:7].float(), m_dev[:, 7].float()
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(B, 3, 3)
    us = (torch.arange(W, device=dev, dtype=torch.float32) - float(centre[0])).reshape(1, 1, W)
    vs = (torch.arange(H, device=dev, dtype=torch.float32) - float(centre[1])).reshape(1, H, 1)
    out = []
    for side in range(2):
        f = m_dev[:, 10 + side].float().reshape(B, 1, 1)
        d = dm[side] + m_dev[:, 8 + side].float().reshape(B, 1, 1)
        xyz = torch.stack([(us / f) * d, (vs / f) * d, d.expand(B, H, W)], -1)  # (B, H, W, 3)
        rows = torch.nonzero(masks[side].unsqueeze(0) & ~torch.isinf(dm[side]))
        pts = xyz[rows[:, 0], rows[:, 1], rows[:, 2]]
        if side == 0:
            b = rows[:, 0]
            pts = (torch.einsum("nij,nj->ni", R[b], pts) + t[b]) / scale[b].unsqueeze(1)
        out += [pts, rows]
    return out


def same_kept_set(ours, theirs, B):
    """the counts and the kept pixels of every pair are equal; the largest relative difference of the points"""
    points, pixel, counts = (t.cpu().numpy() for t in ours)
    worst = 0.0
    for side in range(2):
        pts, rows = theirs[2 * side].cpu().numpy(), theirs[2 * side + 1].cpu().numpy()
        n = np.bincount(rows[:, 0], minlength=B)
        if not (n == counts[:, side]).all():
            return False, None
        start = np.concatenate([[0], np.cumsum(n)])
        for b in range(min(B, 8)):  # (the first pairs: a per-pair loop over 1024 pairs of NumPy slices proves no more)
            at = counts[b, 0] if side else 0
            mine = pixel[b, at:at + n[b]]
            if not (mine == rows[start[b]:start[b + 1], 1] * W + rows[start[b]:start[b + 1], 2]).all():
                return False, None
            a, c = points[b, at:at + n[b]].astype(np.float64), pts[start[b]:start[b + 1]].astype(np.float64)
            worst = max(worst, float(np.abs(a - c).max() / np.abs(a).max()))
    return True, worst


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0), r


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    return int(peak)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    doc = {"shape": {"maps": [H, W], "dtype": "float32", "kind": "varying_focal", "seed": SEED}, "reps": a.reps, "library": _capi.library_version(),
           "unit": "ms per call of all pairs, host clock around a drained stream; bytes of peak device memory above the resident inputs",
           "favours_the_torch_route": "its subsample mask is handed over ready-made; it computes in float32, the library in float64", "case": {}}
    for name, B, rate in CASES:
        dm, m, models, centre = make_inputs(B, dev)
        masks = candidate_masks(rate, dev)
        thr = frontend.recon_threshold(rate)
        p_max = reconstruct.default_p_max(2 * H * W, thr)

        def ours():
            return poselib.reconstruct_pairs_torch("varying_focal", models, dm[0], dm[1], center1=centre, center2=centre, rate=rate, seed=SEED)

        def theirs():
            return torch_route(dm, models, centre, masks)

        same, worst = same_kept_set(ours(), theirs(), B)  # (also the warm-up of both routes)
        if not same:
            raise SystemExit(f"{name}: the two routes keep different pixels")
        routes = {"reconstruct": ours, "torch": theirs}
        ms = {k: [] for k in routes}
        for _ in range(a.reps):
            for k, fn in routes.items():
                ms[k].append(timed(fn)[0])
        peak = {k: peak_above_inputs(fn) for k, fn in routes.items()}
        tiles = 2 * ((H * W + 1023) // 1024)
        peak["reconstruct"] += B * (4 * tiles + 184 + 80)  # the library's own scratch: tile counts, the pairs' records, the camera tables
        kept = ours()[2].sum().item()
        doc["case"][name] = {"pairs": B, "rate": rate, "p_max": p_max, "kept_points": int(kept), "same_kept_set": True, "max_relative_point_difference": worst,
                             "routes": {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v),
                                            "peak_bytes": peak[k]} for k, v in ms.items()}}
        del dm, masks, models
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
