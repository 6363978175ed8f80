"""The back end of the drop-in module: fused two-view point clouds from models and depth maps, on the GPU (include/mdrp_reconstruct.h).

What the reference's callers do BEHIND the estimator (README: `xyz1_in_camera2_frame = (1/geometry.scale) * ((pose.R @ xyz1.T).T + pose.t)`;
make_pair.py, make_video.py): unproject both depth maps, drop the infinite points, subsample, and bring image 1's cloud into camera 2's frame.  The
three entry points below are re-exported by mdrp_amd.poselib, where their callers look for them; mdrp_amd/frontend.py reconstruct_pair_numpy states
every rule (R1-R7), and the device result equals it as bytes.
"""
import math

import numpy as np

from . import _capi, frontend

LAST = "last"  # models="last": the device records of the handle's last estimate, never copied to the host


def default_p_max(pixels, thr):
    """The documented bound on a pair's kept points, in integers.  At "all" every pixel: `pixels`.  Otherwise the kept number is at most binomial
    (pixels draws of probability thr / 2^32, before the depth filter, which only drops): its mean plus eight standard deviations plus 64, capped at
    `pixels`.  A pair above it is truncated and says so (n1 + n2 > p_max)."""
    pixels, thr = int(pixels), int(thr)
    if thr >= _capi.RECON_ALL:
        return pixels
    mean = -((-pixels * thr) >> 32)                               # ceil(pixels * p)
    sd = math.isqrt((pixels * thr * ((1 << 32) - thr)) >> 64) + 1  # above sqrt(pixels * p * (1 - p))
    return min(pixels, mean + 8 * sd + 64)


def _options(rate, seed, keep, p_max, pixels):
    if keep not in _capi.RECON_KEEP:
        raise ValueError(f"keep must be one of {tuple(_capi.RECON_KEEP)}, not {keep!r}")
    thr = frontend.recon_threshold(rate)
    if thr < 1:
        raise ValueError(f"rate {rate!r} is below 2^-32: nothing would be kept")
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit 64 bits (its low 32 bits are used)")
    p_max = default_p_max(pixels, thr) if p_max is None else int(p_max)
    if not 0 <= p_max < 1 << 31:
        raise ValueError(f"p_max must be 0 .. 2^31 - 1, not {p_max}")
    return _capi.ReconstructOpt(_capi.RECON_KEEP[keep], thr, seed, p_max, 0)


def _check_maps(h, w):
    if h > _capi.RECON_MAX_EXTENT or w > _capi.RECON_MAX_EXTENT:
        raise ValueError(f"a map extent is at most {_capi.RECON_MAX_EXTENT}, not {h} x {w}")
    if h * w >= 1 << 31:
        raise ValueError("a map has fewer than 2^31 pixels")


def _models(models, B, dev, h):
    """(tensor that holds the records, stride in bytes) of models= on `dev`"""
    import torch
    if isinstance(models, str):
        if models != LAST:
            raise ValueError(f'models: the only string is "{LAST}", not {models!r}')
        rec = torch.empty((B, _capi.RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        if B > 0:
            try:
                h.copy_results_device(rec.data_ptr(), B)
            except _capi.MdrpError:
                raise ValueError(f'models="last": the handle on this device and stream holds no {B} records (no estimate has run on it, or a smaller '
                                 "one)") from None
        return rec, _capi.RESULT_DTYPE.itemsize
    if isinstance(models, np.ndarray) and models.dtype == _capi.RESULT_DTYPE:
        models = np.ascontiguousarray(models.reshape(-1)["model"])
    return _pl._model_tensor(models, B, dev, "models"), _capi.MODEL_DTYPE.itemsize


def _focal_kind_cameras(verb):
    return ValueError(f"cameras are the calibrated kind's: a focal kind {verb} with the model's focals")


def _stage_pairs(kind, depth_map1, depth_map2, cameras1, cameras2, center1, center2, options, verb="unprojects"):
    """The per-pair form checked and staged: (k, desc, opt, B, dev, cams1, cams2, keep_alive).  options(pixels) -> the call's option record, made
    between the checks of the maps and of the cameras; verb: what a focal kind does with its focals, for the exception."""
    k = _pl._monodepth_kind(kind)
    dev = _pl._check_on_gpu({"depth_map1": depth_map1, "depth_map2": depth_map2})
    _pl._check_float_pair(depth_map1, depth_map2, "depth maps")
    if depth_map1.dim() != 3 or depth_map2.dim() != 3 or depth_map1.shape[0] != depth_map2.shape[0]:
        raise ValueError("depth maps must have shape (B, H, W) with one B")
    B = int(depth_map1.shape[0])
    (h1, w1), (h2, w2) = (int(v) for v in depth_map1.shape[1:]), (int(v) for v in depth_map2.shape[1:])
    _check_maps(h1, w1); _check_maps(h2, w2)
    opt = options(h1 * w1 + h2 * w2)
    cams1 = cams2 = None
    if k == _capi.CALIB:
        cams1, cams2 = _pl._camera_records(cameras1, B), _pl._camera_records(cameras2, B)
    elif cameras1 is not None or cameras2 is not None:
        raise _focal_kind_cameras(verb)
    dm1, dm2 = depth_map1.contiguous(), depth_map2.contiguous()
    c1, c2 = _pl._center(center1, B, dev), _pl._center(center2, B, dev)
    desc = _capi.DepthPairs(dm1.data_ptr(), dm2.data_ptr(), _pl._float_types()[dm1.dtype], h1, w1, h2, w2, 0, _pl._data_ptr(c1), _pl._data_ptr(c2))
    return k, desc, opt, B, dev, cams1, cams2, (dm1, dm2, c1, c2)


def _stage_images(depth_maps, centers, sizes, pairs_ptr):
    """The image part of the per-image form staged - the checked maps, the centres and the sizes - around the pairs' device pointer:
    (desc, keep_alive)"""
    import torch
    dev = depth_maps.device
    I, H, W = (int(v) for v in depth_maps.shape)
    dm = depth_maps.contiguous()
    cs = _pl._per_image(centers, torch.float64, (I, 2), "centers", dev)
    sz = _pl._per_image(sizes, torch.int32, (I, 2), "sizes", dev)
    desc = _capi.DepthImagePairs(dm.data_ptr(), _pl._float_types()[dm.dtype], H, W, I, _pl._data_ptr(sz), _pl._data_ptr(cs), pairs_ptr)
    return desc, (dm, cs, sz)


def _check_image_maps(depth_maps):
    """(dev, I, H, W) of the per-image form's maps"""
    dev = _pl._check_on_gpu({"depth_maps": depth_maps})
    if depth_maps.dtype not in _pl._float_types():
        raise ValueError("depth maps must be float32 or float64")
    if depth_maps.dim() != 3:
        raise ValueError("depth maps must have shape (I, H, W)")
    I, H, W = (int(v) for v in depth_maps.shape)
    _check_maps(H, W)
    return dev, I, H, W


def _stage_image_pairs(kind, depth_maps, pairs, cameras, centers, sizes, options, verb="unprojects"):
    """_stage_pairs for the per-image form: the cameras are per image and expanded to per-pair records by pairs on the host."""
    k = _pl._monodepth_kind(kind)
    dev, I, H, W = _check_image_maps(depth_maps)
    on_device, host_pairs, B = _pl._pairs_on_host(pairs, dev, k == _capi.CALIB)
    B = int(B)
    opt = options(2 * H * W)
    cams1 = cams2 = None
    if k == _capi.CALIB:
        cams1, cams2 = _pl._pair_cameras(cameras, host_pairs, I)
    elif cameras is not None:
        raise _focal_kind_cameras(verb)
    pr = _pl._pairs_on_device(pairs, on_device, host_pairs, dev)
    desc, keep_alive = _stage_images(depth_maps, centers, sizes, pr.data_ptr())
    return k, desc, opt, B, dev, cams1, cams2, keep_alive + (pr,)


def _run(staged, models, outputs, method):
    """One two-view device call on staged = what _stage_pairs returns.  outputs(B, opt, dev) -> the output tensors, allocated under the device;
    method(handle) -> the handle's entry point, called with the tensors' pointers between the model records and the cameras."""
    import torch
    k, desc, opt, B, dev, cams1, cams2, keep_alive = staged
    h = _pl._handle_on(dev)
    with torch.cuda.device(dev):
        rec, stride = _models(models, B, dev, h)
        out = outputs(B, opt, dev)
        method(h)(k, desc, opt, B, rec.data_ptr(), stride, *(t.data_ptr() for t in out), cams1, cams2)
    del rec, keep_alive, staged  # (queued on the current stream, where torch's allocator orders the reuse of their memory behind the call)
    return out


def _cloud(B, opt, dev):
    import torch
    return (torch.empty((B, opt.p_max, 3), dtype=torch.float32, device=dev), torch.empty((B, opt.p_max), dtype=torch.int32, device=dev),
            torch.empty((B, 2), dtype=torch.int32, device=dev))


def reconstruct_pairs_torch(kind, models, depth_map1, depth_map2, cameras1=None, cameras2=None, center1=None, center2=None, rate=0.05, seed=0,
                            keep="not_inf", p_max=None):
    """The fused two-view point cloud of B pairs on the device's current torch stream; nothing synchronises and nothing crosses to the host.
    kind: "calibrated" | "shared_focal" | "varying_focal".  depth maps (B, H, W) float32 | float64 on one ROCm device (the two images may differ in
    size); cameras1 / cameras2 (calibrated only): one Camera | dict for all pairs, a list of B or a CAMERA_DTYPE array; center1 / center2: optional
    (B, 2) or (2,), subtracted from the pixel in float64 (the focal kinds' principal points).
    models: what priors= takes (a float64 (B, 12) or uint8 (B, 96) tensor on the device, a numpy _capi.MODEL_DTYPE array), the numpy records an
    estimate_* call returned (their model field), or "last": the records of the last estimate on this device and stream, copied device to device.
    rate: the share of pixels kept before the depth filter, by a hash of (seed, image, v, u) alone - a pair's cloud does not depend on its batch,
    and a smaller rate keeps a subset; rate >= 1 keeps all.  keep: "not_inf" (the scripts' rule: a NaN depth stays) | "finite".
    p_max: rows per pair; None = default_p_max (every pixel at rate >= 1, else the binomial mean plus eight standard deviations plus 64).
    Returns (points (B, p_max, 3) float32: image 1's kept pixels in row-major order, in camera 2's frame, then image 2's; pixel (B, p_max) int32:
    v * W + u of every row in its own map, -1 behind the last row; counts (B, 2) int32: the TRUE kept numbers, n1 + n2 > p_max says truncated) as
    device tensors.  A pair whose model is not usable (a NaN pose, scale 0, a focal <= 0) is empty."""
    staged = _stage_pairs(kind, depth_map1, depth_map2, cameras1, cameras2, center1, center2, lambda pixels: _options(rate, seed, keep, p_max, pixels))
    return _run(staged, models, _cloud, lambda h: h.reconstruct_pairs_device)


def reconstruct_image_pairs_torch(kind, models, depth_maps, pairs, cameras=None, centers=None, sizes=None, rate=0.05, seed=0, keep="not_inf", p_max=None):
    """reconstruct_pairs_torch for pairs given as image indices: depth_maps (I, H, W) exist once per image, pairs (B, 2) image indices (a, c) as a
    sequence, NumPy array or tensor on any device (a pair with an index outside [0, I) is empty).  sizes (I, 2) (h, w): the valid region of each
    map, clamped to (H, W), None = all; centers (I, 2) or (2,); cameras (calibrated only) are per IMAGE - one for all, a list of I or a
    CAMERA_DTYPE array of I - and expanded to per-pair records by pairs on the host.  pixel is v * W + u with the ALLOCATED W, whatever the sizes.
    p_max None: default_p_max of 2 * H * W pixels.  Everything else, and what is returned, as reconstruct_pairs_torch."""
    staged = _stage_image_pairs(kind, depth_maps, pairs, cameras, centers, sizes, lambda pixels: _options(rate, seed, keep, p_max, pixels))
    return _run(staged, models, _cloud, lambda h: h.reconstruct_pairs_device)


def _single_pair(geometry_or_image_pair, depth_map1, depth_map2, camera1, camera2, device):
    """(kind, model records, the two maps as (1, H, W) device tensors) of one pair for NumPy users"""
    import torch
    g = geometry_or_image_pair
    focal = hasattr(g, "camera1") and hasattr(g, "geometry")
    if not focal and (camera1 is None or camera2 is None):
        raise ValueError("a MonoDepthTwoViewGeometry needs camera1 and camera2; a MonoDepthImagePair brings its focals")
    if focal and (camera1 is not None or camera2 is not None):
        raise ValueError("a MonoDepthImagePair brings its focals: pass no cameras")
    kind = _capi.VARYING_FOCAL if focal else _capi.CALIB
    rec = _pl._model_records([g], kind)
    dev = torch.device("cuda", int(device))
    maps = [torch.from_numpy(np.ascontiguousarray(frontend._table(d, "depth maps"))).to(dev).unsqueeze(0) for d in (depth_map1, depth_map2)]
    if maps[0].dim() != 3 or maps[1].dim() != 3:
        raise ValueError("expected depth maps (H, W)")
    return kind, rec, maps


def reconstruct_pair(geometry_or_image_pair, depth_map1, depth_map2, camera1=None, camera2=None, center1=None, center2=None, rate=0.05, seed=0,
                     keep="not_inf", p_max=None, device=0):
    """One pair for NumPy users, over the same device call: a MonoDepthTwoViewGeometry with its two cameras (the calibrated kind), or a
    MonoDepthImagePair (its cameras' focals; pass center1 / center2, the principal points), and two (H, W) float32 | float64 depth maps.
    Returns (points (n, 3) float32 in camera 2's frame, pixel (n,) int32, counts (2,) int32) as NumPy arrays, n = the written rows."""
    kind, rec, maps = _single_pair(geometry_or_image_pair, depth_map1, depth_map2, camera1, camera2, device)
    points, pixel, counts = reconstruct_pairs_torch(kind, rec, maps[0], maps[1], camera1, camera2, center1, center2, rate, seed, keep, p_max)
    counts = counts.cpu().numpy()[0]
    n = min(int(counts.astype(np.int64).sum()), points.shape[1])
    return points[0, :n].cpu().numpy(), pixel[0, :n].cpu().numpy(), counts


from . import poselib as _pl  # noqa: E402  (at the end: poselib re-exports the three entry points above, whichever of the two modules is imported first)
