"""The consistency filter of a scene for the drop-in module: the fused cloud of an image set with only the points that other images' depth maps
confirm, on the GPU (include/mdrp_fuse.h).

`reconstruct_scene_torch` returns the raw union of the maps: depth-edge smear, floaters and every surface error of a monocular network, and overlaps
as contradicting sheets.  Every image of a scene has a transform to its root, so a point of one image can be tested against any other image of its
component: it is carried into that image's camera, projected to the nearest pixel and compared with the depth the map holds there.  A point stays
if at least `min_consistent` views see a surface at its depth and at most `max_violating` see through it.  The entry points are re-exported by
mdrp_amd.poselib; mdrp_amd/frontend.py fuse_scene_numpy states every rule (F1-F6), and the device result equals it as bytes.
"""
import numpy as np

from . import _capi, frontend

MAX_VIEWS = _capi.FUSE_MAX_VIEWS


def scene_views(pairs, n_images, max_views=MAX_VIEWS, weights=None):
    """Per image the images its points are tested against, as a `views` array (n_images, max_views) int32 padded with -1.  Runs on the HOST, in
    NumPy and plain Python (choosing views on the device is out of scope).  An image's views are its partners over the pairs, in both directions,
    ordered by descending weight, then ascending image index; each partner appears once (with its best weight), a pair with a weight <= 0 or NaN,
    with a == c or with an index outside [0, n_images) is left out, and the list is cut at max_views.  weights (B,): None = 1 for every pair;
    covisibility_scores(...)["weight"] is the natural choice.  A view NEED NOT be a partner: every image of a component has a transform to the
    root, so any row of image indices is a valid `views` - an image that is detached, hangs on another root, is the image itself or repeats
    is ignored by the filter."""
    I, V = int(n_images), int(max_views)
    if I < 0:
        raise ValueError("n_images must not be negative")
    if not 0 <= V <= MAX_VIEWS:
        raise ValueError(f"max_views must be 0 .. {MAX_VIEWS}, not {V}")
    pairs = np.asarray(pairs).astype(np.int64).reshape(-1, 2)
    w = np.ones(len(pairs)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if len(w) != len(pairs):
        raise ValueError("one weight per pair")
    best = [{} for _ in range(I)]
    for (a, c), x in zip(pairs.tolist(), w.tolist()):
        if a == c or not (0 <= a < I and 0 <= c < I) or not x > 0.0:
            continue
        best[a][c] = max(best[a].get(c, x), x)
        best[c][a] = max(best[c].get(a, x), x)
    views = np.full((I, V), -1, dtype=np.int32)
    for i, partners in enumerate(best):
        order = sorted(partners, key=lambda n: (-partners[n], n))[:V]
        views[i, :len(order)] = order
    return views


def _views_table(views, I, dev):
    """a sequence, NumPy array or tensor of integers (I, V), 0 <= V <= MAX_VIEWS -> (contiguous int32 tensor on `dev`, V)"""
    import torch
    if isinstance(views, torch.Tensor):
        if views.dim() != 2 or views.dtype.is_floating_point:
            raise ValueError("views must be (n_images, V) integers")
        t = views.to(dev).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).contiguous()
    else:
        a = np.asarray(views)
        if a.size == 0 and a.ndim < 2:
            a = a.reshape(I, 0).astype(np.int32)
        if a.ndim != 2 or a.dtype.kind not in "iu":
            raise ValueError("views must be (n_images, V) integers")
        t = torch.from_numpy(np.ascontiguousarray(np.clip(a, -2 ** 31, 2 ** 31 - 1).astype(np.int32))).to(dev)
    if t.shape[0] != I:
        raise ValueError(f"views must have one row per image: ({I}, V), not {tuple(t.shape)}")
    if t.shape[1] > MAX_VIEWS:
        raise ValueError(f"views has at most {MAX_VIEWS} columns, not {t.shape[1]}")
    return t, int(t.shape[1])


def _options(rate, seed, keep, p_max, pixels, n_views, tol, min_consistent, max_violating):
    o = reconstruct._options(rate, seed, keep, p_max, pixels)
    lo, hi = frontend.covis_band(tol)
    min_consistent, max_violating = int(min_consistent), int(max_violating)
    if min_consistent < 0:
        raise ValueError(f"min_consistent must not be negative, not {min_consistent}")
    if max_violating < 0:
        raise ValueError(f"max_violating must not be negative, not {max_violating}")
    return _capi.FuseOpt(o.keep, o.thr, o.seed, o.p_max, int(n_views), lo, hi, min(min_consistent, 2 ** 31 - 1), min(max_violating, 2 ** 31 - 1))


def fuse_scene_torch(kind, models, depth_maps, pairs, tree, views, cameras=None, centers=None, sizes=None, rate=1.0, seed=0, keep="not_inf", tol=0.05,
                     min_consistent=1, max_violating=0, p_max=None, return_transforms=False, return_image=False):
    """The consistency-filtered cloud of an image set on the current torch stream; nothing synchronises and nothing crosses to the host.
    kind, models ("last" included), depth_maps (I, H, W), pairs, tree, cameras, centers, sizes, rate, seed, keep: as reconstruct_scene_torch takes
    them - the candidates are the scene's own (the same hash), so a smaller rate tests a subset.  views (I, V) integers, 0 <= V <= 8: per image the
    images its points are tested against (scene_views builds one from the pairs; a view need not be a partner, and a slot that names the image
    itself, a detached image, an image of another component, an index outside [0, I) or an image named earlier in the row is ignored).
    tol: a depth is consistent within (1 - tol) .. (1 + tol) of the view's, 0 <= tol <= 1.  A point is kept iff at least min_consistent views are
    consistent with it and at most max_violating see through it (it floats in front of a surface the view saw).  The defaults tol = 0.05,
    min_consistent = 1, max_violating = 0 are UNTUNED: no dataset stands behind them.  min_consistent = 0 with max_violating >= V keeps every
    candidate: points, pixel and offsets are then reconstruct_scene_torch's, byte for byte, and support labels every point.
    p_max: rows of the whole scene; None = the scene's candidate bound, as reconstruct_scene_torch derives it.
    Returns (points (p_max, 3) float32 in the frame of each image's root, pixel (p_max,) int32 = v * W + u, -1 behind the last row, support
    (p_max, 2) uint8 = (consistent views, violating views) of every row, offsets (I + 1,) int64: the TRUE running sum of the kept points per image)
    as device tensors; with return_transforms the (I, 128) uint8 transform records next, with return_image the image index of every row (p_max,)
    int64 last.  Duplicates of one surface seen by several images are all kept."""
    import torch
    k = _pl._monodepth_kind(kind)
    dev, I, H, W = reconstruct._check_image_maps(depth_maps)
    vw, V = _views_table(views, I, dev)
    opt = _options(rate, seed, keep, p_max, I * H * W, V, tol, min_consistent, max_violating)
    cams = None
    if k == _capi.CALIB:
        cams = _pl._camera_records(cameras, I) if I > 0 else None
    elif cameras is not None:
        raise reconstruct._focal_kind_cameras("unprojects")
    pr = scene._int_table(pairs, 2, "pairs", dev)
    tr = scene._tree_table(tree, I, dev)
    B = int(pr.shape[0])
    desc, images = reconstruct._stage_images(depth_maps, centers, sizes, pr.data_ptr() if B else None)
    h = _pl._handle_on(dev)
    with torch.cuda.device(dev):
        rec, stride = reconstruct._models(models, B, dev, h)
        points = torch.empty((opt.p_max, 3), dtype=torch.float32, device=dev)
        pixel = torch.empty((opt.p_max,), dtype=torch.int32, device=dev)
        support = torch.empty((opt.p_max, 2), dtype=torch.uint8, device=dev)
        offsets = torch.empty((I + 1,), dtype=torch.int64, device=dev)
        T = torch.empty((I, scene.TRANSFORM_DTYPE.itemsize), dtype=torch.uint8, device=dev) if return_transforms else None
        h.fuse_scene_device(k, desc, opt, B, rec.data_ptr() if B else None, stride, tr.data_ptr() if I else None, vw.data_ptr() if I and V else None,
                            points.data_ptr(), pixel.data_ptr(), support.data_ptr(), offsets.data_ptr(), cams, T.data_ptr() if T is not None and I else None)
    del rec, images, pr, tr, vw  # (queued on the current stream, where torch's allocator orders the reuse of their memory behind the call)
    out = [points, pixel, support, offsets]
    if return_transforms:
        out.append(T)
    if return_image:
        rows = torch.arange(opt.p_max, device=dev)
        image = torch.searchsorted(offsets[1:].contiguous(), rows, right=True)
        out.append(torch.where(rows < offsets[-1], image, torch.full_like(image, -1)))
    return tuple(out)


def fuse_scene(kind, models, depth_maps, pairs, tree, views, cameras=None, centers=None, sizes=None, rate=1.0, seed=0, keep="not_inf", tol=0.05,
               min_consistent=1, max_violating=0, p_max=None, device=0):
    """fuse_scene_torch for NumPy users, over the same device call: depth_maps (I, H, W) float32 | float64 as a NumPy array, the rest as there.
    Returns (points (n, 3) float32, pixel (n,) int32, support (n, 2) uint8, offsets (I + 1,) int64, transforms (I,) scene.TRANSFORM_DTYPE, image
    (n,) int64) as NumPy arrays, n = the written rows."""
    import torch
    dev = torch.device("cuda", int(device))
    dm = torch.from_numpy(np.ascontiguousarray(frontend._table(depth_maps, "depth maps"))).to(dev)
    with torch.cuda.device(dev):
        points, pixel, support, offsets, T, image = fuse_scene_torch(kind, models, dm, pairs, tree, views, cameras, centers, sizes, rate, seed, keep, tol,
                                                                     min_consistent, max_violating, p_max, True, True)
    offsets = offsets.cpu().numpy()
    n = min(int(offsets[-1]), points.shape[0])
    return points[:n].cpu().numpy(), pixel[:n].cpu().numpy(), support[:n].cpu().numpy(), offsets, scene._records(T), image[:n].cpu().numpy()


from . import poselib as _pl  # noqa: E402  (at the end: poselib re-exports the entry points above, whichever of the modules is imported first)
from . import reconstruct, scene  # noqa: E402  (behind poselib, which loads them: their option, model, table and p_max helpers are shared)
