#!/usr/bin/env python3
"""What the consistency filter of a scene costs, on the scene of tools/scene_bench.py: 46 images of 480 x 640 float32 depth maps resident
on the device (around one surface, as tools/covis_bench.py makes them, so that views agree and disagree), a batch of 1024 pairs over them with one
varying-focal model per pair, the maximum-weight spanning tree of that batch, and per image its V best partners as views (fuse.scene_views).
V in {0, 2, 8}, rates 0.05 and 1.  Three routes alternate within every repetition, each ending with the stream drained:
    scene    (a) poselib.reconstruct_scene_torch on the same scene: the parent's path.  fuse - scene is the filter's price.
    fuse     poselib.fuse_scene_torch; V = 0 runs under the open gate (0, 0) - the scene's own work - and V > 0 under the default gate (1, 0)
    torch    (b) the same survivors in torch, in float64 and in the definition's order of operations: every candidate of every image in one flat
             list, the point in the root's frame, then per view slot a gather of the view's record, the inverse transform, the projection, a gather
             of the view's depth, the comparisons; the gate, torch.nonzero, the rows.  It is handed the candidates' (image, v, u) index lists (S3's
             hash evaluated once), the transform records and the valid slots (F3) ready-made, outside the timed region: all three favour it.
Before anything is timed the torch route's kept pixels, support and per-image counts are checked EQUAL to fuse's, and fuse at V = 0 under the open
gate equal to the scene's cloud as bytes; a difference ends the run.  Medians of --reps repetitions (21 by default) after a warm-up of every route,
with min and max, and each route's peak device memory above the resident inputs, written to profiles/fuse_bench.json.
    python tools/fuse_bench.py [--reps 21] [--out profiles/fuse_bench.json]"""
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
from mdrp_amd import _capi, frontend, poselib, scene  # noqa: E402

H, W, I, B, SEED, KIND, TOL = 480, 640, 46, 1024, 7, "varying_focal", 0.05
VIEWS = (0, 2, 8)
RATES = (0.05, 1.0)


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


def torch_route(dm, centre, cand, rec, slots, lo, hi, gate):
    """(pixel (n,) int64 = v * W + u, image (n,), support (n, 2) int64, points (n, 3) float32) of the kept candidates, in the filter's order.
    cand = (image, v, u) index tensors; rec: R (I, 3, 3), t (I, 3), s, f, shift (I,) float64 and depth (I,); slots (I, V): the valid views, -1 elsewhere"""
    img, v, u = cand
    R, t, s, f, shift, depth = rec
    d = dm[img, v, u].double()
    z = d + shift[img]
    r = 1.0 / f[img]
    X = [((u.double() - centre[0]) * r) * z, ((v.double() - centre[1]) * r) * z, z]
    inv = 1.0 / s[img]
    root = depth[img] == 0
    Q = [torch.where(root, X[k], (((R[img, k, 0] * X[0] + R[img, k, 1] * X[1]) + R[img, k, 2] * X[2]) + t[img, k]) * inv) for k in range(3)]
    tested = torch.isfinite(d) & (z > 0)
    cons, viol = torch.zeros_like(img), torch.zeros_like(img)
    for k in range(slots.shape[1]):
        n = slots[img, k]
        valid = tested & (n >= 0)
        n = n.clamp(min=0)
        Y = [s[n] * Q[j] - t[n, j] for j in range(3)]
        P = [torch.where(depth[n] == 0, Q[j], (R[n, 0, j] * Y[0] + R[n, 1, j] * Y[1]) + R[n, 2, j] * Y[2]) for j in range(3)]
        front = valid & torch.isfinite(P[2]) & (P[2] > 0)
        a, b = ((P[0] / P[2]) * f[n] + centre[0]) + 0.5, ((P[1] / P[2]) * f[n] + centre[1]) + 0.5
        inside = front & (a >= 0) & (a < W) & (b >= 0) & (b < H)
        ut, vt = torch.where(inside, a, torch.zeros_like(a)).long(), torch.where(inside, b, torch.zeros_like(b)).long()
        dt = dm[n, vt, ut].double()
        zt = dt + shift[n]
        known = inside & torch.isfinite(dt) & (zt > 0)
        low, high = lo * zt, hi * zt
        cons += (known & (P[2] >= low) & (P[2] <= high)).long()
        viol += (known & (P[2] < low)).long()
    keep = torch.nonzero(~torch.isinf(d) & (cons >= gate[0]) & (viol <= gate[1])).reshape(-1)
    return v[keep] * W + u[keep], img[keep], torch.stack([cons[keep], viol[keep]], 1), torch.stack([q[keep] for q in Q], 1).float()


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    dm = make_maps(dev)
    rng = np.random.default_rng(I)
    pairs = np.stack([rng.integers(0, I, B), rng.integers(0, I, B)], axis=1).astype(np.int32)
    weights = rng.uniform(size=B)
    tree = scene.scene_tree(pairs, weights, I)
    m = make_models(B, rng)
    models = torch.from_numpy(m.view(np.float64).reshape(B, 12).copy()).to(dev)
    centre = torch.tensor([W / 2.0, H / 2.0], dtype=torch.float64, device=dev)
    lo, hi = frontend.covis_band(TOL)
    T = scene._records(poselib.scene_transforms_torch(KIND, models, pairs, tree, I))
    rec = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (T["R"].reshape(I, 3, 3), T["t"], T["s"], T["f"], T["shift"], T["depth"].astype(np.int64)))
    doc = {"shape": {"images": I, "maps": [H, W], "dtype": "float32", "kind": KIND, "pairs": B, "tol": TOL, "seed": SEED, "attached_images": int((T["depth"] >= 0).sum()),
                     "tree_depth": int(T["depth"].max())},
           "reps": a.reps, "library": _capi.library_version(),
           "unit": "ms per call of the whole scene, host clock around a drained stream; MiB of peak device memory above the resident inputs",
           "favours_the_torch_route": "its candidates' index lists, the transform records and the valid view slots are handed over ready-made",
           "cases": []}
    for rate in RATES:
        thr = frontend.recon_threshold(rate)
        lists = [np.nonzero(frontend.recon_candidates(H, W, thr, frontend.scene_seed(SEED, i), frontend.SCENE_STAGE)) if T[i]["depth"] >= 0 else (np.zeros(0, np.int64),) * 2
                 for i in range(I)]
        cand = tuple(torch.from_numpy(np.concatenate(x).astype(np.int64)).to(dev) for x in
                     ([np.full(len(l[0]), i) for i, l in enumerate(lists)], [l[0] for l in lists], [l[1] for l in lists]))
        del lists
        for V in VIEWS:
            views = poselib.scene_views(pairs, I, V, weights)
            slots = torch.from_numpy(np.array([frontend.fuse_valid_slots(T, views[i], i) for i in range(I)], dtype=np.int64).reshape(I, V)).to(dev)
            gate = (0, 0) if V == 0 else (1, 0)

            def plain():
                return poselib.reconstruct_scene_torch(KIND, models, dm, pairs, tree, None, centre, None, rate, SEED)

            def ours():
                return poselib.fuse_scene_torch(KIND, models, dm, pairs, tree, views, None, centre, None, rate, SEED, "not_inf", TOL, gate[0], gate[1])

            def theirs():
                return torch_route(dm, centre, cand, rec, slots, lo, hi, gate)

            routes = {"scene": plain, "fuse": ours, "torch": theirs}
            points, pixel, support, offsets = ours()  # (also the warm-up of the routes)
            n = int(offsets[-1])
            t_pixel, t_image, t_support, t_points = theirs()
            equal = (len(t_pixel) == n and bool((t_pixel == pixel[:n]).all()) and bool((t_support == support[:n]).all()) and bool((t_points == points[:n]).all())
                     and bool((torch.bincount(t_image, minlength=I) == offsets[1:] - offsets[:-1]).all()))
            if not equal:
                raise SystemExit(f"rate {rate} V {V}: the torch route's survivors or support differ from fuse_scene_torch's")
            if V == 0:
                s_points, s_pixel, s_offsets = plain()
                if not (torch.equal(s_points, points) and torch.equal(s_pixel, pixel) and torch.equal(s_offsets, offsets)):
                    raise SystemExit(f"rate {rate}: the open gate without views differs from the scene's cloud")
            candidates = int(plain()[2][-1])
            del points, pixel, support, t_pixel, t_image, t_support, t_points
            peaks = {k: peak_mib(fn) for k, fn in routes.items()}
            ms = {k: [] for k in routes}
            for _ in range(a.reps):
                for k, fn in routes.items():
                    ms[k].append(timed(fn)[0])
            doc["cases"].append({"rate": rate, "views": V, "valid_slots": int((slots >= 0).sum()), "gate": list(gate), "candidates": candidates, "kept": n,
                                 "torch_route_equal": True, "routes": {k: {**stats(v), "peak_mib": peaks[k]} for k, v in ms.items()}})
            del slots
            torch.cuda.empty_cache()
        del cand
    doc["not_measured"] = ("the kernels' own times (no profiler run), float64 maps, the calibrated kind, register-count variants of the kernels, "
                           "run-to-run spread across runs of this tool")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
