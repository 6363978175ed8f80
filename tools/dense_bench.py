#!/usr/bin/env python3
"""What the dense front end costs, per call of B pairs at a dense matcher's shape: R = 560 x 1120 warp rows per pair (a symmetric warp
of two 560 x 560 images), n = 5000 records, float32 inputs resident on the device, calibrated estimator with 1000 iterations.  Four variants
alternate within every repetition, each ending with its results on the host:
    sample_dense           poselib.sample_dense_torch (records on the device, counts on the host)
    estimate_dense         poselib.estimate_dense_torch (sampler + estimator in one call)
    torch_sample           the same steps in torch: torch.multinomial over the thresholded certainty (expansion * n draws), a second torch.multinomial
                           down to n (uniform weights: the 40 000 x 40 000 kernel-density estimate of the procedure is NOT run, which favours this
                           route), pixel coordinates, truncation, depth lookup, the both-infinite filter, compaction to padded buffers and counts
    torch_estimate         torch_sample, then poselib.estimate_batch_torch with its n_per_pair
The two routes draw different rows (torch's random stream against the project's integer sampler): only their cost is compared.  Medians of --reps
repetitions (21 by default) with their spreads, written to profiles/dense_bench.json.
    python tools/dense_bench.py [--pairs 8] [--reps 21] [--out profiles/dense_bench.json]"""
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
from mdrp_amd import _capi, poselib  # noqa: E402

HC, WC, H, W, N, EXPANSION, THRESHOLD = 560, 1120, 560, 560, 5000, 4, 0.05
RO = {"max_iterations": 1000, "min_iterations": 1000, "max_epipolar_error": 2.0, "max_reproj_error": 16.0}
BO = {"loss_type": "TRUNCATED_CAUCHY"}
CAM = {"model": "SIMPLE_PINHOLE", "width": W, "height": H, "params": [500.0, W / 2.0, H / 2.0]}


def make_inputs(B, dev):
    """a smooth random warp (an affine map of the grid per pair plus noise), a certainty with about half the rows above the threshold, random depths
    with a few infinite pixels"""
    g = torch.Generator(device="cpu").manual_seed(0)
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, HC), torch.linspace(-1, 1, WC), indexing="ij")
    base = torch.stack([xs, ys], -1).reshape(1, -1, 2)
    A = torch.eye(2).reshape(1, 2, 2) + 0.1 * torch.randn((B, 2, 2), generator=g)
    other = base @ A.transpose(1, 2) + 0.05 * torch.randn((B, 1, 2), generator=g) + 0.002 * torch.randn((B, HC * WC, 2), generator=g)
    warp = torch.cat([base.expand(B, -1, -1), other], -1).reshape(B, HC, WC, 4).float()
    u = torch.rand((B, HC, WC), generator=g)
    cert = torch.where(u < 0.5, u * 0.1, u).float()
    dm = [torch.rand((B, H, W), generator=g) * 5.0 + 1.0 for _ in range(2)]
    for d in dm:
        d[torch.rand((B, H, W), generator=g) < 0.05] = float("inf")
    out = [t.to(dev).contiguous() for t in (warp, cert, dm[0], dm[1])]
    torch.cuda.synchronize()
    return out


def torch_sample(warp, cert, dm1, dm2):
    B = warp.shape[0]
    R = HC * WC
    wp, ct = warp.reshape(B, R, 4), cert.reshape(B, R)
    p = torch.where(ct > THRESHOLD, torch.ones_like(ct), ct.clamp(min=0.0))
    first = torch.multinomial(p, EXPANSION * N, replacement=False)
    second = torch.multinomial(torch.ones((B, EXPANSION * N), device=warp.device), N, replacement=False)
    rows = torch.gather(first, 1, second).sort(dim=1).values
    m = torch.gather(wp, 1, rows[..., None].expand(-1, -1, 4)).double()
    x1 = (m[..., :2] + 1.0) * torch.tensor([0.5 * W, 0.5 * H], dtype=torch.float64, device=warp.device)
    x2 = (m[..., 2:] + 1.0) * torch.tensor([0.5 * W, 0.5 * H], dtype=torch.float64, device=warp.device)
    inside = ((x1 > -1.0) & (x1 < torch.tensor([W, H], device=warp.device))).all(-1) & ((x2 > -1.0) & (x2 < torch.tensor([W, H], device=warp.device))).all(-1)
    i1, i2 = x1.clamp(0, W - 1).long(), x2.clamp(0, W - 1).long()
    bi = torch.arange(B, device=warp.device)[:, None]
    d1, d2 = dm1[bi, i1[..., 1], i1[..., 0]].double(), dm2[bi, i2[..., 1], i2[..., 0]].double()
    keep = inside & ~(torch.isinf(d1) & torch.isinf(d2))
    order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)  # kept rows first, in row order
    x1, x2 = (torch.gather(x, 1, order[..., None].expand(-1, -1, 2)).contiguous() for x in (x1, x2))
    d1, d2 = (torch.gather(d, 1, order).contiguous() for d in (d1, d2))
    return x1, x2, d1, d2, keep.sum(1).cpu().numpy().astype(np.int32)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return 1000.0 * (time.perf_counter() - t0), r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    t = make_inputs(a.pairs, dev)

    def sample_dense():
        return poselib.sample_dense_torch(*t, n=N, expansion=EXPANSION, threshold=THRESHOLD)[4]

    def estimate_dense():
        return poselib.estimate_dense_torch("calibrated", *t, CAM, CAM, RO, BO, n=N, expansion=EXPANSION, threshold=THRESHOLD)[0]

    def torch_only():
        return torch_sample(*t)[4]

    def torch_estimate():
        x1, x2, d1, d2, cnt = torch_sample(*t)
        return poselib.estimate_batch_torch("calibrated", x1, x2, d1, d2, CAM, CAM, RO, BO, n_per_pair=cnt)[0]

    variants = {"sample_dense": sample_dense, "estimate_dense": estimate_dense, "torch_sample": torch_only, "torch_estimate": torch_estimate}
    counts = {k: fn() for k, fn in variants.items()}  # warm-up
    ms = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, fn in variants.items():
            ms[k].append(timed(fn)[0])
    case = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v)} for k, v in ms.items()}
    doc = {"shape": {"pairs": a.pairs, "rows": HC * WC, "n": N, "expansion": EXPANSION, "maps": [H, W], "iterations": RO["max_iterations"], "dtype": "float32"},
           "reps": a.reps, "library": _capi.library_version(), "unit": "ms per call of all pairs, host clock, results on the host",
           "records_per_pair": {"sample_dense": [int(v) for v in counts["sample_dense"]], "torch_sample": [int(v) for v in counts["torch_sample"]]},
           "not_in_the_torch_route": "the kernel-density estimate of the balanced re-sampling (uniform weights instead)", "case": case}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
