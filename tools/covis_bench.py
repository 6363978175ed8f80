#!/usr/bin/env python3
"""What the co-visibility counts cost against the route a user has without them, on the same tensors: 46 images of 480 x 640 float32
depth maps resident on the device, pairs over them as image indices with one varying-focal model per pair (near the identity, so that most of an
image lands inside the other).  Cases: 1 pair at rate 0.05, 1024 pairs at rate 0.05, 64 pairs at rate 1.  Two routes alternate within every
repetition, each ending with the stream drained:
    covis    poselib.covisibility_image_pairs_torch: the (B, 2, 8) counters on the device
    torch    per direction, on the SAME sampled pixels: the candidate pixels' index lists are handed over ready-made (C3's hash evaluated once, outside
             the timed region), then broadcast unprojection, the transform, round (px + 0.5, truncated), gather of the target depth, the comparisons
             and the sums, in float64 and in the definition's order of operations.
The two routes' counters are compared before anything is timed; the comparison's outcome stands in the result.  Medians of --reps repetitions (21 by
default) after a warm-up of every route, with min and max, and each route's peak device memory above the resident inputs, written to
profiles/covis_bench.json.
    python tools/covis_bench.py [--reps 21] [--out profiles/covis_bench.json]"""
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
from mdrp_amd import _capi, frontend, poselib  # noqa: E402

H, W, I, SEED, KIND, TOL = 480, 640, 46, 7, "varying_focal", 0.05
CASES = ((1, 0.05), (1024, 0.05), (64, 1.0))


def make_models(n, rng):
    m = np.zeros(n, dtype=_capi.MODEL_DTYPE)
    q = rng.normal(size=(n, 4)) * 0.03 + np.array([1.0, 0.0, 0.0, 0.0])
    m["q"], m["t"], m["scale"] = q / np.linalg.norm(q, axis=1, keepdims=True), rng.normal(size=(n, 3)) * 0.2, rng.uniform(0.9, 1.1, size=n)
    m["f1"], m["f2"] = rng.uniform(400.0, 700.0, size=n), rng.uniform(400.0, 700.0, size=n)
    return m


def make_maps(dev):
    g = torch.Generator(device=dev).manual_seed(I)
    dm = 5.0 + 0.1 * torch.randn((I, H, W), generator=g, device=dev)
    wild = torch.rand((I, H, W), generator=g, device=dev) < 0.2
    dm = torch.where(wild, torch.rand((I, H, W), generator=g, device=dev) * 9.0 + 1.0, dm)
    dm[torch.rand((I, H, W), generator=g, device=dev) < 0.03] = float("inf")
    torch.cuda.synchronize()
    return dm


def torch_route(dm, models, pairs, centre, cand, lo, hi):
    """(B, 2, 8) int64 counters; models (B, 12) float64, pairs (B, 2) int64 on the device, cand[dir] = (v, u) index tensors of the candidates"""
    w, x, y, z = models[:, 0], models[:, 1], models[:, 2], models[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    t, scale = models[:, 4:7], models[:, 7:8]
    out = []
    for direction in range(2):
        s, g = direction, 1 - direction
        v, u = cand[direction]
        d = dm[pairs[:, s, None], v[None, :], u[None, :]].double()
        shift_s, shift_t, f_s, f_t = models[:, 8 + s, None], models[:, 8 + g, None], models[:, 10 + s, None], models[:, 10 + g, None]
        zz = d + shift_s
        sampled = torch.isfinite(d) & (zz > 0)
        r = 1.0 / f_s
        X = [((u.double() - centre[0])[None, :] * r) * zz, ((v.double() - centre[1])[None, :] * r) * zz, zz]
        if direction == 0:
            inv = 1.0 / scale
            P = [inv * (((R[:, k, 0, None] * X[0] + R[:, k, 1, None] * X[1]) + R[:, k, 2, None] * X[2]) + t[:, k, None]) for k in range(3)]
        else:
            Y = [scale * X[k] - t[:, k, None] for k in range(3)]
            P = [(R[:, 0, k, None] * Y[0] + R[:, 1, k, None] * Y[1]) + R[:, 2, k, None] * Y[2] for k in range(3)]
        front = sampled & torch.isfinite(P[2]) & (P[2] > 0)
        a, b = ((P[0] / P[2]) * f_t + centre[0]) + 0.5, ((P[1] / P[2]) * f_t + centre[1]) + 0.5
        inside = front & (a >= 0) & (a < W) & (b >= 0) & (b < H)
        ut, vt = torch.where(inside, a, torch.zeros_like(a)).long(), torch.where(inside, b, torch.zeros_like(b)).long()
        dt = dm[pairs[:, g, None], vt, ut].double()
        zt = dt + shift_t
        known = inside & torch.isfinite(dt) & (zt > 0)
        low, high = lo * zt, hi * zt
        classes = (sampled, front, inside, known, known & (P[2] >= low) & (P[2] <= high), known & (P[2] > high), known & (P[2] < low))
        out.append(torch.stack([c.sum(1) for c in classes] + [torch.zeros(len(models), dtype=torch.int64, device=dm.device)], 1))
    return torch.stack(out, 1)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0), r


def peak_mib(fn):
    """peak device memory of one call above what is resident before it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    del r
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covis_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    dm = make_maps(dev)
    centre = torch.tensor([W / 2.0, H / 2.0], dtype=torch.float64, device=dev)
    lo, hi = frontend.covis_band(TOL)
    doc = {"shape": {"images": I, "maps": [H, W], "dtype": "float32", "kind": KIND, "tol": TOL, "seed": SEED}, "reps": a.reps, "library": _capi.library_version(),
           "unit": "ms per call of the whole batch, host clock around a drained stream; MiB of peak device memory above the resident inputs",
           "favours_the_torch_route": "its candidate pixels are handed over as ready-made index lists", "cases": []}
    for B, rate in CASES:
        rng = np.random.default_rng(B)
        pairs = np.stack([rng.integers(0, I, B), rng.integers(0, I, B)], axis=1).astype(np.int32)
        models = torch.from_numpy(make_models(B, rng).view(np.float64).reshape(B, 12).copy()).to(dev)
        pairs_dev = torch.from_numpy(pairs.astype(np.int64)).to(dev)
        thr = frontend.recon_threshold(rate)
        cand = [tuple(torch.from_numpy(ix).to(dev) for ix in np.nonzero(frontend.recon_candidates(H, W, thr, SEED, frontend.COVIS_STAGES[d]))) for d in range(2)]

        def ours():
            return poselib.covisibility_image_pairs_torch(KIND, models, dm, pairs_dev, centers=centre, rate=rate, seed=SEED, tol=TOL)

        def theirs():
            return torch_route(dm, models, pairs_dev, centre, cand, lo, hi)

        routes = {"covis": ours, "torch": theirs}
        got, want = ours().cpu().numpy().astype(np.int64), theirs().cpu().numpy()  # (also the warm-up of both routes)
        differing = int((got != want).sum())
        if differing:
            print(f"B {B} rate {rate}: {differing} of {got.size} counters differ between the routes, by at most {int(np.abs(got - want).max())}", file=sys.stderr)
        peaks = {k: peak_mib(fn) for k, fn in routes.items()}
        ms = {k: [] for k in routes}
        for _ in range(a.reps):
            for k, fn in routes.items():
                ms[k].append(timed(fn)[0])
        doc["cases"].append({"pairs": B, "rate": rate, "sampled_pixels": int(got[:, :, 0].sum()), "consistent_pixels": int(got[:, :, 4].sum()),
                             "routes_equal": differing == 0, "differing_counters": differing,
                             "routes": {k: {**stats(v), "peak_mib": peaks[k]} for k, v in ms.items()}})
        del cand, models, pairs_dev
        torch.cuda.empty_cache()
    doc["not_measured"] = "the kernels' own times (no profiler run), float64 maps, the calibrated kind, the per-pair form, run-to-run spread across calls"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
