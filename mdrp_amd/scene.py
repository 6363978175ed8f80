"""Scenes for the drop-in module: an image set's pairs chained along a tree and ONE fused point cloud per scene, on the GPU (include/mdrp_scene.h,
DESIGN.md 7k).

`reconstruct_image_pairs_torch` gives a per-image batch one two-view cloud per pair, each in its own pair's camera-2 frame; the reference's video demo
(make_video.py) carries every frame to its first anchor's frame by R' = R_anchor R, t' = R_anchor t + scale t_anchor, s' = s_anchor scale, on the
host.  The entry points below take the pairs' models and a tree over the images - which pair an image hangs on - accumulate every image's transform to
its root on the device and unproject every image ONCE, into its root's frame.  They are re-exported by mdrp_amd.poselib; mdrp_amd/frontend.py
scene_transforms_numpy / reconstruct_scene_numpy state every rule (S1-S6), and the device result equals them as bytes.
"""
import numpy as np

from . import _capi, frontend

TRANSFORM_DTYPE = frontend.SCENE_TRANSFORM_DTYPE  # mdrp_scene_transform as a NumPy record: R (9,), t (3,), s, f, shift, root, depth


def video_tree(n):
    """The video demo's chain over n frames: (pairs (n - 1, 2), tree (n, 2)) with pairs[i - 1] = (i, i - 1) - frame i is image 1 of its pair with the
    frame before it - frame 0 the root (on pair 0's second side; a single frame: a root without a pair, which only the calibrated kind allows) and
    frame i hanging on pair i - 1."""
    n = int(n)
    if n < 1:
        raise ValueError("a video has at least one frame")
    i = np.arange(1, n, dtype=np.int32)
    pairs = np.stack([i, i - 1], axis=1).astype(np.int32).reshape(-1, 2)
    tree = np.zeros((n, 2), dtype=np.int32)
    tree[0] = (0 if n > 1 else -1, _capi.SCENE_ROOT)
    tree[1:, 0], tree[1:, 1] = i - 1, _capi.SCENE_EDGE
    return pairs, tree


def scene_tree(pairs, weights, n_images, roots=None):
    """The maximum-weight spanning forest of the images under the pairs, as a `tree` array (n_images, 2) int32 of (pair, role).  Runs on the HOST, in
    NumPy and plain Python (choosing the tree on the device is out of scope): fetch the weights first - num_inliers of the records, say, or better
    covisibility_scores(covisibility_image_pairs_torch(...))["weight"], the number of pixels on which the pair's two depth maps agree under its model
    (mdrp_amd/covis.py): 300 inliers on one poster no longer beat a pair whose maps agree over half the frame.
    pairs (B, 2) image indices, weights (B,): larger is better; a pair with a == c, an index outside [0, n_images) or a NaN weight is left out.
    Deterministic: Kruskal's algorithm over the pairs by descending weight, ties by the lower pair index.  roots: the image each component is rooted
    at - any number of images, at most one per component; a component without one is rooted at its lowest image.  A root takes the lowest-index
    tree pair that holds it (its shift and focal come from there); an image no pair reaches is a root on pair -1, which only the calibrated kind
    accepts (the focal kinds have no focal for it: it is detached there)."""
    I = int(n_images)
    pairs = np.asarray(pairs).astype(np.int64).reshape(-1, 2)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if len(w) != len(pairs):
        raise ValueError("one weight per pair")
    ok = (pairs[:, 0] != pairs[:, 1]) & (pairs >= 0).all(axis=1) & (pairs < I).all(axis=1) & ~np.isnan(w)
    order = [int(b) for b in np.lexsort((np.arange(len(w)), -w)) if ok[b]]  # descending weight, then ascending pair index
    parent = list(range(I))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    adjacent = [[] for _ in range(I)]
    for b in order:
        a, c = int(pairs[b, 0]), int(pairs[b, 1])
        ra, rc = find(a), find(c)
        if ra != rc:
            parent[max(ra, rc)] = min(ra, rc)
            adjacent[a].append((b, c)); adjacent[c].append((b, a))
    component = [find(i) for i in range(I)]  # (the lowest image of the component: unions keep the smaller representative)
    root_of = {}
    for r in ([] if roots is None else [int(v) for v in np.asarray(roots).reshape(-1)]):
        if not 0 <= r < I:
            raise ValueError(f"root {r} is outside [0, {I})")
        if root_of.setdefault(component[r], r) != r:
            raise ValueError(f"two roots in one component: {root_of[component[r]]} and {r}")
    tree = np.zeros((I, 2), dtype=np.int32)
    for comp in sorted(set(component)):
        root = root_of.get(comp, comp)
        tree[root] = (min((b for b, _ in adjacent[root]), default=-1), _capi.SCENE_ROOT)
        seen, queue = {root}, [root]
        while queue:  # breadth first, neighbours by ascending pair index
            node = queue.pop(0)
            for b, other in sorted(adjacent[node]):
                if other not in seen:
                    seen.add(other)
                    tree[other] = (b, _capi.SCENE_EDGE)
                    queue.append(other)
    return tree


def _device_of(*values):
    import torch
    for v in values:
        if isinstance(v, torch.Tensor) and v.is_cuda:
            return v.device
    return torch.device("cuda", torch.cuda.current_device())


def _int_table(v, cols, what, dev):
    """a sequence, NumPy array or tensor of integers -> contiguous int32 (n, cols) tensor on `dev`"""
    import torch
    if isinstance(v, torch.Tensor):
        if v.dim() != 2 or v.shape[1] != cols or v.dtype.is_floating_point:
            raise ValueError(f"{what} must be (n, {cols}) integers")
        return v.to(dev).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).contiguous()
    a = np.asarray(v)
    if a.size == 0:
        a = a.reshape(0, cols)
    if a.ndim != 2 or a.shape[1] != cols or a.dtype.kind not in "iu":
        raise ValueError(f"{what} must be (n, {cols}) integers")
    return torch.from_numpy(np.ascontiguousarray(np.clip(a, -2 ** 31, 2 ** 31 - 1).astype(np.int32))).to(dev)


def _tree_table(tree, I, dev):
    tr = _int_table(tree, 2, "tree", dev)
    if tr.shape[0] != I:
        raise ValueError(f"tree must have one (pair, role) row per image: ({I}, 2), not {tuple(tr.shape)}")
    return tr


def _records(t):
    """a (n, 128) uint8 tensor of transform records -> NumPy records"""
    return t.cpu().numpy().view(TRANSFORM_DTYPE).reshape(-1)


def scene_transforms_torch(kind, models, pairs, tree, n_images):
    """The accumulated transform of every image of a tree, on the current torch stream; nothing synchronises and nothing crosses to the host.
    models: what reconstruct_pairs_torch takes (a model tensor, model or result records, or "last"), one per pair; pairs (B, 2) image indices (a, c);
    tree (n_images, 2) of (pair, role): role 0 = the image is absent, 1 = it hangs on the other image of pairs[pair], 2 = a root (video_tree and
    scene_tree build one).  Returns a (n_images, 128) uint8 device tensor of mdrp_scene_transform records - `scene.TRANSFORM_DTYPE` views its NumPy copy:
    a point X of image i is (R X + t) / s in the frame of image `root`; depth = its edges to the root, -1 = absent or detached (a bad pair, an
    unusable model or a cycle on its way)."""
    import torch
    k = _pl._monodepth_kind(kind)
    I = int(n_images)
    if I < 0:
        raise ValueError("n_images must not be negative")
    dev = _device_of(models, pairs, tree)
    pr = _int_table(pairs, 2, "pairs", dev)
    tr = _tree_table(tree, I, dev)
    B = int(pr.shape[0])
    h = _pl._handle_on(dev)
    with torch.cuda.device(dev):
        rec, stride = reconstruct._models(models, B, dev, h)
        out = torch.empty((I, TRANSFORM_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        h.scene_transforms_device(k, B, rec.data_ptr() if B else None, stride, pr.data_ptr() if B else None, I, tr.data_ptr() if I else None,
                                  out.data_ptr() if I else None)
    del rec, pr, tr  # (queued on the current stream, where torch's allocator orders the reuse of their memory behind the call)
    return out


def reconstruct_scene_torch(kind, models, depth_maps, pairs, tree, cameras=None, centers=None, sizes=None, rate=0.05, seed=0, keep="not_inf", p_max=None,
                            return_transforms=False, return_image=False):
    """The fused point cloud of an image set on the current torch stream: every image unprojected ONCE, in the frame of its root; nothing synchronises
    and nothing crosses to the host.  depth_maps (I, H, W) float32 | float64 on one ROCm device; models, pairs, tree as scene_transforms_torch;
    cameras (calibrated only) per IMAGE - one for all, a list of I or a CAMERA_DTYPE array of I; centers (I, 2) or (2,); sizes (I, 2) (h, w), the
    valid region of each map.  rate, seed, keep as reconstruct_pairs_torch: the kept set of an image depends on (seed, image, v, u) alone and a smaller
    rate keeps a subset.  p_max: rows of the whole scene; None = reconstruct.default_p_max over the scene's I * H * W pixels.
    Returns (points (p_max, 3) float32: the images in ascending index, an image's kept pixels row-major; pixel (p_max,) int32: v * W + u in the
    row's own map, -1 behind the last row; offsets (I + 1,) int64: the TRUE running sum of the kept points per image - image i's rows are
    offsets[i] : offsets[i + 1], and offsets[I] > p_max says the scene was truncated) as device tensors; with return_image the image index of every
    row (p_max,) int64, -1 behind the last row, derived from offsets with torch; with return_transforms the (I, 128) uint8 transform records last.
    A forest is allowed: every component is in its own root's frame (`root` of the records)."""
    import torch
    k = _pl._monodepth_kind(kind)
    dev, I, H, W = reconstruct._check_image_maps(depth_maps)
    opt = reconstruct._options(rate, seed, keep, p_max, I * H * W)
    cams = None
    if k == _capi.CALIB:
        cams = _pl._camera_records(cameras, I) if I > 0 else None
    elif cameras is not None:
        raise reconstruct._focal_kind_cameras("unprojects")
    pr = _int_table(pairs, 2, "pairs", dev)
    tr = _tree_table(tree, I, dev)
    B = int(pr.shape[0])
    desc, images = reconstruct._stage_images(depth_maps, centers, sizes, pr.data_ptr() if B else None)
    h = _pl._handle_on(dev)
    with torch.cuda.device(dev):
        rec, stride = reconstruct._models(models, B, dev, h)
        points = torch.empty((opt.p_max, 3), dtype=torch.float32, device=dev)
        pixel = torch.empty((opt.p_max,), dtype=torch.int32, device=dev)
        offsets = torch.empty((I + 1,), dtype=torch.int64, device=dev)
        T = torch.empty((I, TRANSFORM_DTYPE.itemsize), dtype=torch.uint8, device=dev) if return_transforms else None
        h.reconstruct_scene_device(k, desc, opt, B, rec.data_ptr() if B else None, stride, tr.data_ptr() if I else None, points.data_ptr(),
                                   pixel.data_ptr(), offsets.data_ptr(), cams, T.data_ptr() if T is not None and I else None)
    del rec, images, pr, tr  # (queued on the current stream, where torch's allocator orders the reuse of their memory behind the call)
    out = [points, pixel, offsets]
    if return_image:
        rows = torch.arange(opt.p_max, device=dev)
        image = torch.searchsorted(offsets[1:].contiguous(), rows, right=True)
        out.append(torch.where(rows < offsets[-1], image, torch.full_like(image, -1)))
    if return_transforms:
        out.append(T)
    return tuple(out)


def reconstruct_scene(kind, models, depth_maps, pairs, tree, cameras=None, centers=None, sizes=None, rate=0.05, seed=0, keep="not_inf", p_max=None, device=0):
    """reconstruct_scene_torch for NumPy users, over the same device call: depth_maps (I, H, W) float32 | float64 as a NumPy array, the rest as there.
    Returns (points (n, 3) float32, pixel (n,) int32, offsets (I + 1,) int64, image (n,) int64, transforms (I,) scene.TRANSFORM_DTYPE) as NumPy
    arrays, n = the written rows."""
    import torch
    dev = torch.device("cuda", int(device))
    dm = torch.from_numpy(np.ascontiguousarray(frontend._table(depth_maps, "depth maps"))).to(dev)
    with torch.cuda.device(dev):
        points, pixel, offsets, image, T = reconstruct_scene_torch(kind, models, dm, pairs, tree, cameras, centers, sizes, rate, seed, keep, p_max, True, True)
    offsets = offsets.cpu().numpy()
    n = min(int(offsets[-1]), points.shape[0])
    return points[:n].cpu().numpy(), pixel[:n].cpu().numpy(), offsets, image[:n].cpu().numpy(), _records(T)


from . import poselib as _pl  # noqa: E402  (at the end: poselib re-exports the entry points above, whichever of the modules is imported first)
from . import reconstruct  # noqa: E402  (behind poselib, which loads it: its option, model and p_max helpers are shared)
