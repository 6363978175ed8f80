"""Case builders for the back end's tests (include/mdrp_reconstruct.h): models with awkward normal-range values, depth maps with planted
+inf, -inf, NaN, 0 and negative depths, cameras of both models, and the reference as the NumPy definition states it (mdrp_amd/frontend.py), computed
once per pair and shared."""
import functools

import numpy as np

from mdrp_amd import _capi, frontend

KINDS = ("calibrated", "shared_focal", "varying_focal")
SIZES = (((1, 1), (1, 1)), ((3, 5), (2, 7)), ((37, 53), (41, 29)), ((64, 64), (64, 32)), ((130, 257), (67, 131)))  # ((h1, w1), (h2, w2))
BATCHES = (1, 3, 17)
RATES = (1.0, 0.5, 0.05, 1e-9)
KEEPS = ("not_inf", "finite")
B_MAX = max(BATCHES)
SEED = 0x1234ABCD5
EMPTY = {1: "nan_q", 5: "zero_scale", 9: "bad_focal", 13: "inf_t"}  # R1's empty pairs, mixed into every batch of more than one pair
# ---- the wide sizes (tests/test_gpu_backend_wide.py, tests/test_scan_runs_host.py): maps of more than 256 tiles, where k_recon_scan's threads hold runs
# of more than one tile (per = ceil(tiles / 256) > 1).  409 * 643 = 262 987 pixels are 257 tiles, the smallest count with per = 2, the last tile
# ragged; 723 * 727 = 525 621 pixels are 514 tiles, per = 3; 130 * 257 are 33 tiles, per = 1: s_run is rewritten between the sides with another run
# length, in both orders.  Only the wide tests take them: B = WIDE_B usable pairs each.
TILE = 1024                              # mdrp_reconstruct.h RECON_TILE
SCAN_THREADS = 256                       # mdrp_reconstruct.h RECON_THREADS
WIDE_SIZES = (((409, 643), (130, 257)), ((130, 257), (409, 643)), ((723, 727), (409, 643)))
WIDE_B = 2
WIDE_KINDS = ("varying_focal", "calibrated")
WIDE_RATES = (1.0, 0.05)


def tiles(h, w):
    return -(-(int(h) * int(w)) // TILE)


def scan_run(n, threads=SCAN_THREADS):
    """the run length of the chunked scans: a thread sums per = ceil(n / threads) consecutive values"""
    return -(-int(n) // threads)


def models(kind, n=B_MAX, seed=11):
    """n models whose every value has a full mantissa (a fused multiply-add would round differently somewhere); the pairs of EMPTY are not usable"""
    rng = np.random.default_rng(seed)
    m = np.zeros(n, dtype=_capi.MODEL_DTYPE)
    q = rng.normal(size=(n, 4))
    m["q"] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.97, 1.03, size=(n, 1))  # (nobody promised a unit quaternion)
    m["t"] = rng.normal(size=(n, 3)) * 1.7
    m["scale"] = rng.uniform(0.31, 2.9, size=n) * rng.choice([-1.0, 1.0], size=n, p=[0.2, 0.8])
    m["shift1"] = rng.normal(size=n) * 0.37
    m["shift2"] = rng.normal(size=n) * 0.41
    m["f1"] = rng.uniform(310.0, 910.0, size=n) if kind != "calibrated" else 1.0
    m["f2"] = m["f1"] if kind == "shared_focal" else (rng.uniform(310.0, 910.0, size=n) if kind == "varying_focal" else 1.0)
    for i, what in EMPTY.items():
        if i >= n:
            continue
        if what == "nan_q":
            m["q"][i, 0] = np.nan
        elif what == "zero_scale":
            m["scale"][i] = 0.0
        elif what == "bad_focal":
            if kind == "calibrated":
                m["shift2"][i] = np.inf
            else:
                m["f1"][i] = -1.0
        else:
            m["t"][i, 1] = -np.inf
    return m


def cameras(n=B_MAX, seed=12):
    """two [n] camera tables: SIMPLE_PINHOLE and PINHOLE with fx != fy alternate"""
    rng = np.random.default_rng(seed)
    out = np.zeros((2, n), dtype=_capi.CAMERA_DTYPE)
    for s in range(2):
        for i in range(n):
            if (i + s) % 2:
                out[s, i]["model_id"] = 1
                out[s, i]["params"] = [rng.uniform(400, 900), rng.uniform(400, 900), rng.uniform(10, 300) + 0.37, rng.uniform(10, 200) + 0.11]
            else:
                out[s, i]["params"] = [rng.uniform(400, 900), rng.uniform(10, 300) + 0.29, rng.uniform(10, 200) + 0.53, 0.0]
    return out[0], out[1]


def centres(n=B_MAX, seed=13):
    rng = np.random.default_rng(seed)
    return rng.uniform(-40.0, 160.0, size=(n, 2)), rng.uniform(-40.0, 160.0, size=(n, 2))


def depth_maps(h, w, dtype, n=B_MAX, seed=14, whole_inf=2):
    """(n, h, w) depths in float32's normal range with planted +inf, -inf, NaN, 0 and negatives; row 0 of every odd map is +inf where the map has
    more than one row; map `whole_inf` is all +inf"""
    rng = np.random.default_rng(seed + 1000 * h + w)
    d = rng.uniform(0.4, 23.0, size=(n, h, w))
    plant = rng.integers(0, 40, size=(n, h, w))
    d[plant == 0] = np.inf
    d[plant == 1] = -np.inf
    d[plant == 2] = np.nan
    d[plant == 3] = 0.0
    d[plant == 4] *= -1.0
    if h > 1:
        d[1::2, 0, :] = np.inf
    if n > whole_inf:
        d[whole_inf] = np.inf
    return d.astype(dtype)


@functools.lru_cache(maxsize=None)
def inputs(kind, dtype_name, size):
    """everything a call of the per-pair form takes, for B_MAX pairs; a batch of B is the first B of each.  A size of WIDE_SIZES: WIDE_B pairs, both
    usable (models 0 and 2), no map all inf"""
    (h1, w1), (h2, w2) = size
    dtype = np.dtype(dtype_name)
    n = WIDE_B if size in WIDE_SIZES else B_MAX
    cam1, cam2 = cameras(n) if kind == "calibrated" else (None, None)
    c1, c2 = centres(n)
    ms = models(kind, 3)[[0, 2]] if size in WIDE_SIZES else models(kind)
    return {"models": ms, "dm1": depth_maps(h1, w1, dtype, n, seed=14), "dm2": depth_maps(h2, w2, dtype, n, seed=15, whole_inf=4), "c1": c1, "c2": c2,
            "cam1": cam1, "cam2": cam2}


@functools.lru_cache(maxsize=None)
def rows(kind, dtype_name, size, keep, rate, b):
    """the definition's kept rows of pair b (R1-R6 and the rounding): computed once, shared by every batch and every p_max that holds the pair"""
    x = inputs(kind, dtype_name, size)
    return frontend.reconstruct_rows_numpy(x["models"][b], kind, x["dm1"][b], x["dm2"][b], x["c1"][b], x["c2"][b],
                                           None if x["cam1"] is None else x["cam1"][b], None if x["cam2"] is None else x["cam2"][b], keep,
                                           frontend.recon_threshold(rate), SEED)


def reference(kind, dtype_name, size, keep, rate, B, p_max):
    """(points (B, p_max, 3), pixel (B, p_max), counts (B, 2)) by the definition"""
    packed = [frontend.pack_rows(rows(kind, dtype_name, size, keep, rate, b), p_max) for b in range(B)]
    return tuple(np.stack([p[i] for p in packed]) for i in range(3))


def p_max_cases(kind, dtype_name, size, keep, rate):
    """R7's five cases, placed by pair 0's counts: 0, inside image 1, exactly n1, inside image 2, n1 + n2 (equal ones collapse)"""
    r = rows(kind, dtype_name, size, keep, rate, 0)
    n1, n2 = len(r[0][1]), len(r[1][1])
    return sorted({0, n1 // 2, n1, n1 + n2 // 2, n1 + n2})


def run(kind, dtype_name, size, keep, rate, B, p_max, device="cuda:0"):
    """poselib.reconstruct_pairs_torch on the first B pairs: (points, pixel, counts) as NumPy arrays"""
    import torch
    from mdrp_amd import poselib
    x = inputs(kind, dtype_name, size)
    dev = torch.device(device)
    out = poselib.reconstruct_pairs_torch(kind, x["models"][:B], torch.from_numpy(x["dm1"][:B]).to(dev), torch.from_numpy(x["dm2"][:B]).to(dev),
                                          None if x["cam1"] is None else x["cam1"][:B], None if x["cam2"] is None else x["cam2"][:B],
                                          torch.from_numpy(x["c1"][:B]).to(dev), torch.from_numpy(x["c2"][:B]).to(dev), rate, SEED, keep, p_max)
    return tuple(t.cpu().numpy() for t in out)


def wide_p_max_cases(kind, dtype_name, size, keep, rate):
    """p_max_cases' scheme (placed by pair 0's counts) at a size of WIDE_SIZES: a cut inside the last tile of the side with more tiles (tile 256 or
    513: half of that tile's kept pixels are written) | the true total"""
    r = rows(kind, dtype_name, size, keep, rate, 0)
    n1, n2 = len(r[0][1]), len(r[1][1])
    side = 0 if tiles(*size[0]) >= tiles(*size[1]) else 1
    last = int((r[side][1] // TILE == tiles(*size[side]) - 1).sum())  # (pixel = v * w + u: the tile walk's own index)
    return ((n1 if side else 0) + len(r[side][1]) - max(last // 2, 1), n1 + n2)


def run_image_form(kind, dtype_name, size, keep, rate, B, p_max, device="cuda:0"):
    """the first B pairs through poselib.reconstruct_image_pairs_torch: 2 B images in one allocation of the larger extents, image 2 b = pair b's map 1
    and image 2 b + 1 its map 2 as valid regions, a finite depth behind them.  pixel is re-based from the allocation's width to the map's own, so
    the result compares with `reference` as it stands."""
    import torch
    from mdrp_amd import poselib
    x = inputs(kind, dtype_name, size)
    (h1, w1), (h2, w2) = size
    H, W = max(h1, h2), max(w1, w2)
    dm = np.full((2 * B, H, W), 3.0, dtype=np.dtype(dtype_name))
    dm[0::2, :h1, :w1], dm[1::2, :h2, :w2] = x["dm1"][:B], x["dm2"][:B]
    sizes = np.tile(np.array([[h1, w1], [h2, w2]], dtype=np.int32), (B, 1))
    cs = np.stack([x["c1"][:B], x["c2"][:B]], axis=1).reshape(2 * B, 2)
    cams = None if x["cam1"] is None else np.stack([x["cam1"][:B], x["cam2"][:B]], axis=1).reshape(2 * B)
    out = poselib.reconstruct_image_pairs_torch(kind, x["models"][:B], torch.from_numpy(dm).to(torch.device(device)), np.arange(2 * B).reshape(B, 2), cams, cs, sizes,
                                                rate=rate, seed=SEED, keep=keep, p_max=p_max)
    points, pixel, counts = (t.cpu().numpy() for t in out)
    own = np.where(np.arange(p_max)[None, :] < counts[:, :1], w1, w2)  # a pair's rows below its true n1 are image 1's
    return points, np.where(pixel >= 0, pixel // W * own + pixel % W, pixel).astype(np.int32), counts


def same_bytes(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


# ---- straight through a handle (refusals, history): the descriptor of the first B pairs of `inputs`, the call, the three outputs as byte strings
def device_call(h, kind="varying_focal", dtype_name="float32", size=SIZES[2], B=3, rate=0.5, keep="not_inf", p_max=700, stride=96, change=None, image_form=False):
    """h.reconstruct_pairs_device on the inputs of (kind, dtype, size); change(args) may overwrite any entry of the argument dict before the call
    (desc, opt, kind, batch, models, stride, points, pixel, counts, cam1, cam2).  image_form: the same pairs through a DepthImagePairs descriptor
    whose image set is the B maps of image 1 (image 2 of pair b is image B - 1 - b)."""
    import torch
    from mdrp_amd import poselib
    x = inputs(kind, dtype_name, size)
    dev = torch.device("cuda:0")
    k = poselib.MONODEPTH_KINDS[kind]
    (h1, w1), (h2, w2) = size
    dm1, dm2 = torch.from_numpy(x["dm1"][:B]).to(dev), torch.from_numpy(x["dm2"][:B]).to(dev)
    c1, c2 = torch.from_numpy(x["c1"][:B]).to(dev), torch.from_numpy(x["c2"][:B]).to(dev)
    rec = np.zeros(B, dtype=_capi.RESULT_DTYPE if stride == 136 else _capi.MODEL_DTYPE)
    (rec["model"] if stride == 136 else rec)[...] = x["models"][:B]
    models = torch.from_numpy(rec.view(np.uint8).reshape(B, stride).copy()).to(dev)
    ftype = _capi.F32 if dtype_name == "float32" else _capi.F64
    if image_form:
        pairs = torch.tensor([[b, B - 1 - b] for b in range(B)], dtype=torch.int32, device=dev)
        desc = _capi.DepthImagePairs(dm1.data_ptr(), ftype, h1, w1, B, None, c1.data_ptr(), pairs.data_ptr())
    else:
        desc = _capi.DepthPairs(dm1.data_ptr(), dm2.data_ptr(), ftype, h1, w1, h2, w2, 0, c1.data_ptr(), c2.data_ptr())
    opt = _capi.ReconstructOpt(_capi.RECON_KEEP[keep], frontend.recon_threshold(rate), SEED, p_max, 0)
    points = torch.full((B, p_max, 3), 7.0, dtype=torch.float32, device=dev)
    pixel = torch.full((B, p_max), 7, dtype=torch.int32, device=dev)
    counts = torch.full((B, 2), 7, dtype=torch.int32, device=dev)
    a = {"kind": k, "desc": desc, "opt": opt, "batch": B, "models": models.data_ptr(), "stride": stride, "points": points.data_ptr(),
         "pixel": pixel.data_ptr(), "counts": counts.data_ptr(), "cam1": None if x["cam1"] is None else x["cam1"][:B],
         "cam2": None if x["cam2"] is None else x["cam2"][:B]}
    if change is not None:
        change(a)
    torch.cuda.synchronize()
    h.reconstruct_pairs_device(a["kind"], a["desc"], a["opt"], a["batch"], a["models"], a["stride"], a["points"], a["pixel"], a["counts"], a["cam1"], a["cam2"])
    h.synchronize()
    return points.cpu().numpy().tobytes(), pixel.cpu().numpy().tobytes(), counts.cpu().numpy().tobytes()
