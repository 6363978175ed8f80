#!/usr/bin/env python3
"""What a fused scene costs against the two routes a user has without it, on the same tensors: 46 images of 480 x 640 float32 depth maps
resident on the device, a batch of 1024 pairs over them with one varying-focal model per pair, and the maximum-weight spanning tree of that batch
(scene.scene_tree, random weights).  Rates 0.05 and 1.  Three routes alternate within every repetition, each ending with the stream drained:
    scene    poselib.reconstruct_scene_torch: points, pixel and offsets of the whole image set on the device
    pairs    (a) poselib.reconstruct_image_pairs_torch on the tree's I - 1 pairs, then torch: the chains composed level by level of the tree (batched
             3 x 3 products in float64), every pair's rows carried to the root's frame by one batched product and masked to the image that hangs on the
             pair.  The rows stay padded per pair (no compaction) and the root's own points are not produced: both favour this route.
    torch    (b) per image: broadcast unprojection of every pixel to an (I, H, W, 3) tensor, the mask (subsample & not infinite), torch.nonzero, index,
             the same level-by-level composition, one batched product.  It is handed the scene's candidate masks ready-made (S3's hash evaluated once,
             outside the timed region), so that it keeps the SAME pixels, which is checked before anything is timed: offsets and kept pixels are equal
             and the points agree to float32 rounding (the route computes in float32).
Route (a) subsamples with the two-view stages, so its kept pixels are others at rate 0.05; at rate 1 every pixel is kept and its rows are checked
against the scene's.  The level lists of the tree (parents, directions, depths) are host data of the caller and are uploaded before the timed region.
Also timed: scene_transforms_torch alone on a 2000-frame video_tree chain (k_scene_chain: one lane per image, about I^2 / 2 edge steps).
Medians of --reps repetitions (21 by default) after a warm-up of every route, with min and max, written to profiles/scene_bench.json.
    python tools/scene_bench.py [--reps 21] [--out profiles/scene_bench.json]"""
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

H, W, I, B, SEED, KIND = 480, 640, 46, 1024, 7, "varying_focal"
RATES = (0.05, 1.0)
CHAIN = 2000


def make_models(n, rng):
    m = np.zeros(n, dtype=_capi.MODEL_DTYPE)
    q = rng.normal(size=(n, 4)) * 0.05 + np.array([1.0, 0.0, 0.0, 0.0])  # small rotations: a chain of 2000 stays in range
    m["q"], m["t"], m["scale"] = q / np.linalg.norm(q, axis=1, keepdims=True), rng.normal(size=(n, 3)) * 0.1, rng.uniform(0.9, 1.1, size=n)
    m["f1"], m["f2"] = rng.uniform(400.0, 700.0, size=n), rng.uniform(400.0, 700.0, size=n)
    return m


def make_inputs(dev):
    g = torch.Generator(device=dev).manual_seed(I)
    dm = torch.rand((I, H, W), generator=g, device=dev) * 9.0 + 1.0
    dm[torch.rand((I, H, W), generator=g, device=dev) < 0.03] = float("inf")
    rng = np.random.default_rng(I)
    pairs = np.stack([rng.integers(0, I, B), rng.integers(0, I, B)], axis=1).astype(np.int32)
    tree = scene.scene_tree(pairs, rng.uniform(size=B), I)
    m = make_models(B, rng)
    models = torch.from_numpy(m.view(np.float64).reshape(B, 12).copy()).to(dev)
    centre = torch.tensor([W / 2.0, H / 2.0], dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    return dm, pairs, tree, m, models, centre


def tree_levels(pairs, tree, dev):
    """host data of the tree for the torch composition: per image its pair, whether it is the pair's image 1, its parent and depth; per level the
    images and their parents as index tensors on the device"""
    n = len(tree)
    pair, first, parent, depth = tree[:, 0].astype(np.int64), np.zeros(n, bool), np.full(n, -1), np.full(n, -1)
    for i in range(n):
        if tree[i, 1] in (_capi.SCENE_EDGE, _capi.SCENE_ROOT) and pair[i] >= 0:
            a, c = pairs[pair[i]]
            first[i] = i == a
            parent[i] = -1 if tree[i, 1] == _capi.SCENE_ROOT else (c if i == a else a)
    for i in range(n):
        k, node = 0, i
        while parent[node] >= 0:
            node, k = parent[node], k + 1
        depth[i] = k
    levels = [(torch.from_numpy(np.nonzero(depth == d)[0]).to(dev), torch.from_numpy(parent[depth == d]).to(dev)) for d in range(1, int(depth.max()) + 1)]
    return {"pair": torch.from_numpy(pair).to(dev), "first": torch.from_numpy(first).to(dev), "parent": parent, "depth": depth, "levels": levels, "first_host": first}


def compose(models, lv):
    """the accumulated (R (I, 3, 3), t (I, 3), s (I,)) of every image in float64, level by level; and the images' own f and shift"""
    m = models[lv["pair"].clamp(min=0)]
    w, x, y, z = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    t, scale, fw = m[:, 4:7], m[:, 7], lv["first"]
    Re = torch.where(fw[:, None, None], R, R.transpose(1, 2))
    te = torch.where(fw[:, None], t, -torch.einsum("nji,nj->ni", R, t) / scale[:, None])
    se = torch.where(fw, scale, 1.0 / scale)
    f, shift = torch.where(fw, m[:, 10], m[:, 11]), torch.where(fw, m[:, 8], m[:, 9])
    n = len(m)
    aR, at, as_ = torch.eye(3, dtype=torch.float64, device=m.device).repeat(n, 1, 1), torch.zeros((n, 3), dtype=torch.float64, device=m.device), torch.ones(n, dtype=torch.float64, device=m.device)
    for idx, par in lv["levels"]:
        aR[idx] = aR[par] @ Re[idx]
        at[idx] = torch.einsum("nij,nj->ni", aR[par], te[idx]) + se[idx, None] * at[par]
        as_[idx] = se[idx] * as_[par]
    return aR, at, as_, f, shift


def pairs_route(dm, models, centre, sub, lv, rate):
    """(a): (points (I - 1, p_max, 3) in the roots' frames, mask (I - 1, p_max) of the rows of the image that hangs on the pair)"""
    points, pixel, counts = poselib.reconstruct_image_pairs_torch(KIND, models[sub["pair"]], dm, sub["pairs"], centers=centre, rate=rate, seed=SEED)
    aR, at, as_, _, _ = compose(models, lv)
    R, t, s = aR[sub["via"]].float(), at[sub["via"]].float(), as_[sub["via"]].float()
    out = (torch.einsum("bij,bpj->bpi", R, points) + t[:, None, :]) / s[:, None, None]
    r = torch.arange(points.shape[1], device=points.device)[None, :]
    n1, n2 = counts[:, 0:1], counts[:, 1:2]
    return out, torch.where(sub["first"][:, None], r < n1, (r >= n1) & (r < n1 + n2))


def torch_route(dm, models, centre, lv, masks):
    """(b): (points (n, 3) float32 in the roots' frames, rows (n, 3) = (image, v, u))"""
    aR, at, as_, f, shift = compose(models, lv)
    us = (torch.arange(W, device=dm.device, dtype=torch.float32) - float(centre[0])).reshape(1, 1, W)
    vs = (torch.arange(H, device=dm.device, dtype=torch.float32) - float(centre[1])).reshape(1, H, 1)
    f = f.float().reshape(-1, 1, 1)
    d = dm + shift.float().reshape(-1, 1, 1)
    xyz = torch.stack([(us / f) * d, (vs / f) * d, d], -1)  # (I, H, W, 3)
    rows = torch.nonzero(masks & ~torch.isinf(dm))
    pts, img = xyz[rows[:, 0], rows[:, 1], rows[:, 2]], rows[:, 0]
    return (torch.einsum("nij,nj->ni", aR.float()[img], pts) + at.float()[img]) / as_.float()[img].unsqueeze(1), rows


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0), r


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    dm, pairs, tree, m, models, centre = make_inputs(dev)
    lv = tree_levels(pairs, tree, dev)
    hang = np.nonzero(tree[:, 1] == _capi.SCENE_EDGE)[0]
    sub = {"pair": torch.from_numpy(tree[hang, 0].astype(np.int64)).to(dev), "pairs": pairs[tree[hang, 0]], "first": torch.from_numpy(lv["first_host"][hang]).to(dev),
           "via": torch.from_numpy(np.where(lv["first_host"][hang], lv["parent"][hang], hang)).to(dev)}
    doc = {"shape": {"images": I, "maps": [H, W], "dtype": "float32", "kind": KIND, "pairs": B, "tree_edges": int(len(hang)), "roots": int((tree[:, 1] == _capi.SCENE_ROOT).sum()),
                     "max_depth": int(lv["depth"].max()), "seed": SEED},
           "reps": a.reps, "library": _capi.library_version(), "unit": "ms per call of the whole scene, host clock around a drained stream",
           "favours_the_other_routes": "pairs: rows stay padded per pair, the roots' own points are not produced; torch: its subsample masks are handed over "
                                       "ready-made; both transform in float32, the library in float64", "rate": {}}
    for rate in RATES:
        thr = frontend.recon_threshold(rate)
        masks = torch.from_numpy(np.stack([frontend.recon_candidates(H, W, thr, frontend.scene_seed(SEED, i), frontend.SCENE_STAGE) for i in range(I)])).to(dev)

        def ours():
            return poselib.reconstruct_scene_torch(KIND, models, dm, pairs, tree, centers=centre, rate=rate, seed=SEED)

        def by_pairs():
            return pairs_route(dm, models, centre, sub, lv, rate)

        def theirs():
            return torch_route(dm, models, centre, lv, masks)

        routes = {"scene": ours, "pairs": by_pairs, "torch": theirs}
        points, pixel, offsets = (t.cpu().numpy() for t in ours())  # (also the warm-up of every route)
        pts, rows = (t.cpu().numpy() for t in theirs())
        n = np.bincount(rows[:, 0], minlength=I)
        if not ((np.diff(offsets) == n).all() and (pixel[:offsets[-1]] == rows[:, 1] * W + rows[:, 2]).all()):
            raise SystemExit(f"rate {rate}: the scene and the torch route keep different pixels")
        worst = float(np.abs(points[:offsets[-1]].astype(np.float64) - pts).max() / np.abs(pts).max())
        check_a = "not checked: the two-view stages keep other pixels at this rate"
        pa, ma = by_pairs()
        if rate >= 1.0:  # every pixel kept: pair b's masked rows are the rows of the image that hangs on it
            worst_a = 0.0
            for b in range(0, len(hang), 9):
                mine = points[offsets[hang[b]]:offsets[hang[b] + 1]].astype(np.float64)
                got = pa[b][ma[b]].cpu().numpy()
                if got.shape != mine.shape:
                    raise SystemExit(f"rate {rate}: the pairs route keeps other rows for image {hang[b]}")
                worst_a = max(worst_a, float(np.abs(got - mine).max() / np.abs(mine).max()))
            check_a = {"max_relative_point_difference": worst_a}
        del pa, ma
        ms = {k: [] for k in routes}
        for _ in range(a.reps):
            for k, fn in routes.items():
                ms[k].append(timed(fn)[0])
        doc["rate"][str(rate)] = {"kept_points": int(offsets[-1]), "rows_allocated": int(points.shape[0]), "same_kept_set_as_torch": True,
                                  "max_relative_point_difference_to_torch": worst, "pairs_route_check": check_a, "routes": {k: stats(v) for k, v in ms.items()}}
        del masks
        torch.cuda.empty_cache()
    vp, vt = scene.video_tree(CHAIN)
    vm = torch.from_numpy(make_models(CHAIN - 1, np.random.default_rng(CHAIN)).view(np.float64).reshape(CHAIN - 1, 12).copy()).to(dev)
    vp_d, vt_d = torch.from_numpy(vp).to(dev), torch.from_numpy(vt).to(dev)

    def chain():
        return poselib.scene_transforms_torch(KIND, vm, vp_d, vt_d, CHAIN)

    T = scene._records(chain())
    if not (T["depth"] == np.arange(CHAIN)).all():
        raise SystemExit("the chain's depths are not 0 .. n - 1")
    doc["video_chain"] = {"frames": CHAIN, "edge_steps": CHAIN * (CHAIN - 1) // 2, "what": "scene_transforms_torch alone (k_scene_chain and the call around it)",
                          **stats([timed(chain)[0] for _ in range(a.reps)])}
    doc["not_measured"] = "the kernels' own times (no profiler run), float64 maps, the calibrated kind, peak memory, run-to-run spread"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
