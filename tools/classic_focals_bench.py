#!/usr/bin/env python3
"""What the varying-focal baseline's tail costs, at the headline shape: 1024 pairs, N = 2000, 10^4 iterations, 50 % outliers, resident
tensors.  Three variants alternate within every repetition, each ending in records on the host:
    seven_point_alone      mdrp_estimate_batch_async(MDRP_FUNDAMENTAL_7PT) + mdrp_fetch_results
    fused                  mdrp_estimate_fundamental_focals_async + mdrp_fetch_results + the 128-byte records copied back
    seven_point_host_tail  the first, then the mask copied back and the tail in NumPy on the host (focals, E, four candidates, cheirality votes)
Medians of --reps repetitions (21 by default) with their spreads, written to profiles/classic_focals_bench.json.  The fused call's focals and
sorted vote counts are compared with the NumPy tail's first.
    python tools/classic_focals_bench.py [--reps 21] [--out profiles/classic_focals_bench.json]"""
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
from mdrp_amd import _capi, synth  # noqa: E402

B, N, ITERS = 1024, 2000, 10000
RO = {"max_iterations": ITERS, "min_iterations": ITERS, "max_epipolar_error": 2.0}
BO = {"loss_type": "TRUNCATED_CAUCHY"}
II = np.diag([1.0, 1.0, 0.0])


def _skew(e):
    return np.array([[0.0, -e[2], e[1]], [e[2], 0.0, -e[0]], [-e[1], e[0], 0.0]])


def _null(M):
    c = [np.cross(M[0], M[1]), np.cross(M[0], M[2]), np.cross(M[1], M[2])]
    return c[int(np.argmax([v @ v for v in c]))]


def numpy_tail(x1, x2, F, mask):
    """(f1, f2, winner, votes) per pair with the principal points at the origin: the tail of include/mdrp_classic_focals.h, pair by pair in NumPy"""
    p = np.array([0.0, 0.0, 1.0])
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    out = np.zeros((len(F), 3))
    votes = np.zeros((len(F), 4), dtype=np.int64)
    for i in range(len(F)):
        Fi = F[i]
        e1, e2 = _null(Fi), _null(Fi.T)
        with np.errstate(all="ignore"):
            f1 = np.sqrt(-(p @ _skew(e2) @ II @ Fi @ p) * (p @ Fi.T @ p) / (p @ _skew(e2) @ II @ Fi @ II @ Fi.T @ p))
            f2 = np.sqrt(-(p @ _skew(e1) @ II @ Fi.T @ p) * (p @ Fi @ p) / (p @ _skew(e1) @ II @ Fi.T @ II @ Fi @ p))
        out[i] = f1, f2, -1
        if not (np.isfinite(f1) and np.isfinite(f2)):
            continue
        E = np.diag([f2, f2, 1.0]) @ Fi @ np.diag([f1, f1, 1.0])
        U, _, Vt = np.linalg.svd(E)
        U, Vt = U * np.sign(np.linalg.det(U)), Vt * np.sign(np.linalg.det(Vt))
        t = U[:, 2]
        keep = mask[i] != 0
        b1 = np.c_[x1[i][keep] / f1, np.ones(int(keep.sum()))]
        b2 = np.c_[x2[i][keep] / f2, np.ones(int(keep.sum()))]
        b1 /= np.linalg.norm(b1, axis=1, keepdims=True)
        b2 /= np.linalg.norm(b2, axis=1, keepdims=True)
        for c, (R, s) in enumerate(((U @ W @ Vt, 1.0), (U @ W @ Vt, -1.0), (U @ W.T @ Vt, -1.0), (U @ W.T @ Vt, 1.0))):
            u = b1 @ R.T
            a = -np.sum(u * b2, axis=1)
            c1, c2 = -(u @ (s * t)), b2 @ (s * t)
            votes[i, c] = int(np.sum((c1 - a * c2 > 0) & (-a * c1 + c2 > 0)))
        out[i, 2] = int(np.argmax(votes[i]))
    return out, votes


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return 1000.0 * (time.perf_counter() - t0), r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classic_focals_bench.json"))
    a = ap.parse_args()
    b = synth.make_batch(0, B, N, noise_px=0.5, outlier_frac=0.5, random_focal="varying")
    dev = torch.device("cuda", 0)
    x1, x2 = torch.from_numpy(b["x1"]).to(dev), torch.from_numpy(b["x2"]).to(dev)
    mask = torch.zeros((B, N), dtype=torch.uint8, device=dev)
    out = torch.zeros((B, 128), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    h = _capi.Handle(0)
    ro, bo = _capi.ransac_opt_from_dict(RO), _capi.bundle_opt_from_dict(BO)

    def alone():
        h.estimate_batch_device(_capi.FUNDAMENTAL_7PT, x1.data_ptr(), x2.data_ptr(), None, None, B, N, ro, bo, None, None, None, mask.data_ptr())
        return h.fetch_results(B)

    def fused():
        h.estimate_fundamental_focals_device(x1.data_ptr(), x2.data_ptr(), B, N, ro, bo, out.data_ptr(), None, mask.data_ptr())
        res = h.fetch_results(B)  # (waits for the handle's stream: the tail's records are complete)
        return res, out.cpu().numpy().reshape(-1).view(_capi.FOCAL_POSE_DTYPE).copy()

    def host_tail():
        res = alone()
        F = np.stack([_capi.model_to_fundamental(m) for m in res["model"]])
        return numpy_tail(b["x1"], b["x2"], F, mask.cpu().numpy())

    variants = {"seven_point_alone": alone, "fused": fused, "seven_point_host_tail": host_tail}
    (_, rec), (ref, votes) = fused(), host_tail()  # warm-up, and the check
    real = rec["status"] == 0
    # (the SVD's candidates are the same four poses in another order, and a vote within rounding of zero may fall either way: the sorted counts, to one)
    if not (np.array_equal(real, ref[:, 2] >= 0) and np.abs(np.sort(rec["votes"][real], axis=1) - np.sort(votes[real], axis=1)).max() <= 1
            and np.allclose(rec["model"]["f1"][real], ref[real, 0], rtol=1e-6) and np.allclose(rec["model"]["f2"][real], ref[real, 1], rtol=1e-6)):
        sys.exit("classic_focals_bench: the fused call and the NumPy tail disagree")
    alone()
    ms = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, fn in variants.items():
            ms[k].append(timed(fn)[0])
    case = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v)} for k, v in ms.items()}
    case["tail_on_device_ms"] = case["fused"]["median_ms"] - case["seven_point_alone"]["median_ms"]
    case["tail_on_host_ms"] = case["seven_point_host_tail"]["median_ms"] - case["seven_point_alone"]["median_ms"]
    doc = {"shape": {"pairs": B, "n": N, "iterations": ITERS, "outlier_fraction": 0.5}, "reps": a.reps, "library": _capi.library_version(),
           "unit": "ms per call, host clock, records on the host", "pairs_with_a_pose": int(real.sum()), "case": case}
    h.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
