"""Co-visibility for the drop-in module: how far a pair's two depth maps agree under the pair's model, as 16 integer counts per pair, on the GPU
(include/mdrp_covis.h).

The sparse inlier count says how many of the matches a model was fitted to agree with it; it says nothing of the rest of the frame.  The entry points
below take a subsample of each image's pixels through the model into the other image and compare depths there: per direction the numbers of sampled
pixels, of those in front of the other camera, inside its map, on a known depth, and of these the consistent, the occluded and the violating ones.
They are re-exported by mdrp_amd.poselib; mdrp_amd/frontend.py covisibility_pair_numpy states every rule (C1-C7), and the device result equals it as
bytes.
"""
import numpy as np

from . import _capi, frontend

CLASSES = _capi.COVIS_CLASSES  # the slot of each class in counts[..., dir, :]


def _options(rate, seed, tol):
    thr = frontend.recon_threshold(rate)
    if thr < 1:
        raise ValueError(f"rate {rate!r} is below 2^-32: nothing would be sampled")
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit 64 bits (its low 32 bits are used)")
    lo, hi = frontend.covis_band(tol)
    return _capi.CovisOpt(thr, 0, seed, lo, hi)


def _counters(B, opt, dev):
    import torch
    return (torch.empty((B, 2, _capi.COVIS_SLOTS), dtype=torch.int32, device=dev),)


def _run(staged, models):
    return reconstruct._run(staged, models, _counters, lambda h: h.covisibility_pairs_device)[0]


def covisibility_pairs_torch(kind, models, depth_map1, depth_map2, cameras1=None, cameras2=None, center1=None, center2=None, rate=0.05, seed=0, tol=0.05):
    """The depth-consistency counts of B pairs on the device's current torch stream; nothing synchronises and nothing crosses to the host.
    kind, models ("last" included), depth maps, cameras and centres: as reconstruct_pairs_torch takes them.  rate, seed: the share of each image's
    pixels that is sampled, by a hash of (seed, direction, v, u) alone - a pair's counts do not depend on its batch, a smaller rate samples a subset,
    and the set is not the cloud's; rate >= 1 samples all.  tol: a depth is consistent within (1 - tol) .. (1 + tol) of the target's, 0 <= tol <= 1.
    Returns counts (B, 2, 8) int32 on the device: per direction (0: image 1's pixels into image 2, 1: the other way round) the numbers of
    sampled | front | inside | known | consistent | occluded | violating pixels and a 0 - each of the first four a subset of the one before it, the
    last three a partition of `known`.  `violating` points float in front of a surface the other camera saw: evidence against the model.  A pair
    whose model is not usable (a NaN pose, scale 0, a focal <= 0) has all counters 0.  covisibility_scores turns the counts into ratios and a weight."""
    staged = reconstruct._stage_pairs(kind, depth_map1, depth_map2, cameras1, cameras2, center1, center2, lambda pixels: _options(rate, seed, tol), "projects")
    return _run(staged, models)


def covisibility_image_pairs_torch(kind, models, depth_maps, pairs, cameras=None, centers=None, sizes=None, rate=0.05, seed=0, tol=0.05):
    """covisibility_pairs_torch for pairs given as image indices: depth_maps (I, H, W) exist once per image, pairs (B, 2) image indices (a, c) as a
    sequence, NumPy array or tensor on any device (a pair with an index outside [0, I) has all counters 0); sizes, centers and cameras per IMAGE, as
    reconstruct_image_pairs_torch takes them.  Returns counts (B, 2, 8) int32 on the device."""
    staged = reconstruct._stage_image_pairs(kind, depth_maps, pairs, cameras, centers, sizes, lambda pixels: _options(rate, seed, tol), "projects")
    return _run(staged, models)


def covisibility_pair(geometry_or_image_pair, depth_map1, depth_map2, camera1=None, camera2=None, center1=None, center2=None, rate=0.05, seed=0,
                      tol=0.05, device=0):
    """One pair for NumPy users, over the same device call: a MonoDepthTwoViewGeometry with its two cameras (the calibrated kind), or a
    MonoDepthImagePair (its cameras' focals; pass center1 / center2, the principal points), and two (H, W) float32 | float64 depth maps.
    Returns counts (2, 8) int32 as a NumPy array."""
    kind, rec, maps = reconstruct._single_pair(geometry_or_image_pair, depth_map1, depth_map2, camera1, camera2, device)
    return covisibility_pairs_torch(kind, rec, maps[0], maps[1], camera1, camera2, center1, center2, rate, seed, tol).cpu().numpy()[0]


def covisibility_scores(counts):
    """What the counts say, per direction, for counts (..., 2, 8) as a torch tensor (any device: a few elementwise torch operations, no kernel of
    this library and no synchronisation) or a NumPy array.  Returns a dict: overlap (..., 2) float64 = consistent / sampled - the share of a frame
    the two maps agree on; agreement (..., 2) float64 = consistent / (consistent + violating) - how far the pixels that can speak about the model
    speak for it (an occluded pixel says nothing); both 0 where the denominator is 0; weight (...,) int64 = consistent[dir 0] + consistent[dir 1],
    an integer meant for scene_tree(weights=...)."""
    S, C, V = (_capi.COVIS_CLASSES.index(n) for n in ("sampled", "consistent", "violating"))
    if isinstance(counts, np.ndarray) or not hasattr(counts, "dim"):
        c = np.asarray(counts)
        if c.ndim < 2 or c.shape[-2:] != (2, _capi.COVIS_SLOTS) or c.dtype.kind not in "iu":
            raise ValueError("counts must be integers of shape (..., 2, 8)")
        c = c.astype(np.int64)

        def ratio(n, d):
            return np.where(d > 0, n / np.maximum(d, 1), 0.0)
        return {"overlap": ratio(c[..., C], c[..., S]), "agreement": ratio(c[..., C], c[..., C] + c[..., V]), "weight": c[..., 0, C] + c[..., 1, C]}
    import torch
    if counts.dim() < 2 or tuple(counts.shape[-2:]) != (2, _capi.COVIS_SLOTS) or counts.dtype.is_floating_point:
        raise ValueError("counts must be integers of shape (..., 2, 8)")
    c = counts.to(torch.int64)

    def ratio(n, d):
        return torch.where(d > 0, n.double() / d.clamp(min=1).double(), torch.zeros_like(n, dtype=torch.float64))
    return {"overlap": ratio(c[..., C], c[..., S]), "agreement": ratio(c[..., C], c[..., C] + c[..., V]), "weight": c[..., 0, C] + c[..., 1, C]}


from . import poselib as _pl  # noqa: E402  (at the end: poselib re-exports the entry points above, whichever of the modules is imported first)
from . import reconstruct  # noqa: E402  (behind poselib, which loads it: its model and map helpers are shared)
