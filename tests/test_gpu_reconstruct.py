"""The back end on a real MI355X (include/mdrp_reconstruct.h): poselib.reconstruct_pairs_torch and reconstruct_image_pairs_torch against
the NumPy definition (mdrp_amd/frontend.py, rules R1-R7) as BYTES, over kinds, depth types, map sizes around the wavefront and tile boundaries, batch
sizes, subsample rates, both depth filters and R7's five p_max cases; batch independence and a side stream; the per-image form against the per-pair
form; estimate -> reconstruct on one stream with the records left on the device; every refusal."""
import numpy as np
import pytest

import reconstruct_cases as rc
from mdrp_amd import frontend

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "float64")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def poselib():
    import mdrp_amd.poselib as poselib
    return poselib


@pytest.fixture(scope="module")
def capi():
    from mdrp_amd import _capi
    return _capi


# ---- bytes against the definition
@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}")
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("kind", rc.KINDS)
def test_bytes_equal_the_definition(kind, dtype_name, size):
    """the cross product B x rate x keep x p_max for one kind, depth type and pair of map sizes.  The inputs plant +inf, -inf, NaN, 0 and negative
    depths, a whole row and a whole map of inf, non-zero centres and shifts, SIMPLE_PINHOLE and PINHOLE with fx != fy, models with full mantissas and
    R1's empty pairs at batch positions 1, 5, 9 and 13 (reconstruct_cases.py).  The definition's rows of a pair are computed once."""
    cases = 0
    for keep in rc.KEEPS:
        for rate in rc.RATES:
            for p_max in rc.p_max_cases(kind, dtype_name, size, keep, rate):
                for B in rc.BATCHES:
                    got = rc.run(kind, dtype_name, size, keep, rate, B, p_max)
                    want = rc.reference(kind, dtype_name, size, keep, rate, B, p_max)
                    for name, g, w in zip(("points", "pixel", "counts"), got, want):
                        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
                        if g.tobytes() != w.tobytes():
                            bad = np.argwhere(g.view(np.uint32 if name == "points" else np.int32) != w.view(np.uint32 if name == "points" else np.int32))
                            raise AssertionError((name, keep, rate, p_max, B, len(bad), bad[:3].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))
                    cases += 1
    assert cases >= len(rc.BATCHES) * len(rc.KEEPS) * len(rc.RATES)
    if size[0][0] >= 37:  # the planted depths did what they are there for (a map of a few pixels may hold no NaN)
        n_inf = rc.reference(kind, dtype_name, size, "not_inf", 1.0, 3, 0)[2]
        n_fin = rc.reference(kind, dtype_name, size, "finite", 1.0, 3, 0)[2]
        assert (n_inf[0] > n_fin[0]).all() and n_inf[1].tolist() == [0, 0] and n_inf[2, 0] == 0 and n_inf[2, 1] > 0  # NaN kept | empty pair | a map of inf
        assert rc.reference(kind, dtype_name, size, "not_inf", 1e-9, 3, 4)[2].sum() == 0  # nothing kept


def test_default_p_max_and_options(torch, poselib):
    """p_max=None is the documented bound: every pixel at rate 1, the binomial bound otherwise, and the result is the definition's at that p_max"""
    from mdrp_amd import reconstruct
    kind, dt, size = "shared_focal", "float32", rc.SIZES[3]
    x = rc.inputs(kind, dt, size)
    pixels = 64 * 64 + 64 * 32
    for rate, p_max in ((1.0, pixels), (0.05, reconstruct.default_p_max(pixels, frontend.recon_threshold(0.05)))):
        got = poselib.reconstruct_pairs_torch(kind, torch.from_numpy(x["models"][:3].view(np.float64).reshape(3, 12)).cuda(), torch.from_numpy(x["dm1"][:3]).cuda(),
                                              torch.from_numpy(x["dm2"][:3]).cuda(), center1=x["c1"][:3], center2=x["c2"][:3], rate=rate, seed=rc.SEED)
        assert got[0].shape == (3, p_max, 3) and got[0].is_cuda and got[2].dtype == torch.int32
        assert rc.same_bytes([t.cpu().numpy() for t in got], rc.reference(kind, dt, size, "not_inf", rate, 3, p_max))
        assert (got[2].sum(1) <= p_max).all()  # not truncated


# ---- batch independence, a side stream
def test_a_pair_does_not_depend_on_its_batch(torch, poselib):
    """pairs 3 and 6 alone, as a batch of two in the other order, and inside the batch of 17: the same rows (R2: nothing depends on the position)"""
    kind, dt, size = "varying_focal", "float32", rc.SIZES[4]
    x = rc.inputs(kind, dt, size)
    n1, n2 = (len(r[1]) for r in rc.rows(kind, dt, size, "not_inf", 0.5, 3))
    p_max = n1 + n2 // 2  # pair 3 is truncated inside image 2

    def call(idx):
        out = poselib.reconstruct_pairs_torch(kind, x["models"][idx], torch.from_numpy(x["dm1"][idx]).cuda(), torch.from_numpy(x["dm2"][idx]).cuda(),
                                              center1=x["c1"][idx], center2=x["c2"][idx], rate=0.5, seed=rc.SEED, p_max=p_max)
        return [t.cpu().numpy() for t in out]
    full = call(list(range(rc.B_MAX)))
    two = call([6, 3])
    for pos, b in enumerate((6, 3)):
        alone = call([b])
        for a, t, f in zip(alone, two, full):
            assert a[0].tobytes() == t[pos].tobytes() == f[b].tobytes(), b
    assert full[2][3].tolist() == [n1, n2] and n1 > 64 and n2 > 64


def test_inputs_from_a_side_stream(torch, poselib):
    """the maps and the models are produced by kernels on a side stream and the call is made on that stream: it is ordered behind them"""
    kind, dt, size = "calibrated", "float64", rc.SIZES[4]
    x = rc.inputs(kind, dt, size)
    want = rc.reference(kind, dt, size, "finite", 0.5, 3, 5000)
    side = torch.cuda.Stream()
    host = [torch.from_numpy(x[k][:3].copy()).pin_memory() for k in ("dm1", "dm2")]
    models = torch.from_numpy(x["models"][:3].view(np.float64).reshape(3, 12).copy()).pin_memory()
    with torch.cuda.stream(side):
        big = torch.randn(4096, 4096, device="cuda")
        for _ in range(4):  # work in front of the copies, so that a call that did not wait would read unwritten maps
            big = big @ big * 1e-3
        dm1, dm2 = (t.to("cuda", non_blocking=True) * 1.0 for t in host)
        md = models.to("cuda", non_blocking=True) * 1.0
        got = poselib.reconstruct_pairs_torch(kind, md, dm1, dm2, x["cam1"][:3], x["cam2"][:3], x["c1"][:3], x["c2"][:3], rate=0.5, seed=rc.SEED, keep="finite",
                                              p_max=5000)
    side.synchronize()
    assert rc.same_bytes([t.cpu().numpy() for t in got], want)


# ---- the per-image form
@pytest.mark.parametrize("kind, dtype_name", [("calibrated", "float32"), ("varying_focal", "float64")])
def test_per_image_form(torch, poselib, capi, kind, dtype_name):
    """six images allocated 40 x 70 with smaller valid sizes, a repeated image, a == c, and two pairs with an index outside the set: bytes equal to the
    per-pair form on the expanded maps of pairs with equal valid sizes, and to the definition everywhere; pixel counts rows by w_max"""
    rng = np.random.default_rng(21)
    I, H, W = 6, 40, 70
    dm = rc.depth_maps(H, W, np.dtype(dtype_name), n=I, seed=33, whole_inf=99)
    sizes = np.array([[40, 70], [33, 50], [33, 50], [40, 64], [1, 70], [50, 80]], dtype=np.int32)  # (the last one is clamped to 40 x 70)
    pairs = np.array([[0, 5], [1, 2], [2, 2], [3, 0], [4, 1], [6, 0], [1, 2], [0, -1]], dtype=np.int64)
    B = len(pairs)
    ms = rc.models(kind, 11, seed=22)[[0, 2, 3, 4, 6, 7, 8, 10]]  # (the usable ones: the empty pairs here are the two bad indices)
    cs = rng.uniform(0.0, 40.0, size=(I, 2))
    cams = rc.cameras(I, seed=23)[0] if kind == "calibrated" else None
    p_max = 3000
    ok = (pairs >= 0).all(1) & (pairs < I).all(1)
    safe = np.where(ok[:, None], pairs, 0)
    want = frontend.reconstruct_image_pairs_numpy(ms, kind, dm, pairs, p_max, cs, sizes, None if cams is None else cams[safe[:, 0]],
                                                  None if cams is None else cams[safe[:, 1]], "not_inf", frontend.recon_threshold(0.5), rc.SEED)
    got = poselib.reconstruct_image_pairs_torch(kind, ms, torch.from_numpy(dm).cuda(), pairs, cams, cs, sizes, rate=0.5, seed=rc.SEED, p_max=p_max)
    got = [t.cpu().numpy() for t in got]
    assert rc.same_bytes(got, want)
    assert got[2][5].tolist() == got[2][7].tolist() == [0, 0] and (got[1][5] == -1).all() and not got[0][7].any()  # an index outside the set: empty
    assert got[2][1].sum() > 0 and got[2][1][0] + got[2][1][1] <= p_max
    n1 = got[2][1][0]
    assert set(np.unique(got[1][1][:n1] % W)) <= set(range(50)) and got[1][1][:n1].max() >= W  # v * w_max + u with u inside the valid width
    # the per-pair form on the expanded tables: pairs whose two images are full-size take the same maps as they are
    a, c = 0, 5
    one = poselib.reconstruct_pairs_torch(kind, ms[:1], torch.from_numpy(dm[a:a + 1]).cuda(), torch.from_numpy(dm[c:c + 1]).cuda(),
                                          None if cams is None else cams[a:a + 1], None if cams is None else cams[c:c + 1], cs[a], cs[c], rate=0.5,
                                          seed=rc.SEED, p_max=p_max)
    assert all(t.cpu().numpy()[0].tobytes() == g[0].tobytes() for t, g in zip(one, got))
    # ... and a cropped pair takes its valid regions, with pixel re-based to the cropped width
    crop = np.ascontiguousarray(dm[1:3, :33, :50])
    two = poselib.reconstruct_pairs_torch(kind, ms[1:2], torch.from_numpy(crop[0:1]).cuda(), torch.from_numpy(crop[1:2]).cuda(),
                                          None if cams is None else cams[1:2], None if cams is None else cams[2:3], cs[1], cs[2], rate=0.5, seed=rc.SEED,
                                          p_max=p_max)
    two = [t.cpu().numpy()[0] for t in two]
    assert two[0].tobytes() == got[0][1].tobytes() and two[2].tobytes() == got[2][1].tobytes()
    k = int(two[2].sum())
    assert ((two[1][:k] // 50) * W + two[1][:k] % 50 == got[1][1][:k]).all()


# ---- the chain on one stream
def _scene(kind, seed=31):
    """A noise-free pair as the front-end tests build theirs: n scene points, image 1's keypoints ON pixel centres (integer coordinates), image 2's where
    the points project; each map holds a point's depth at its keypoint's pixel.  Returns the tensors' NumPy sources and the ground truth."""
    from mdrp_amd import synth
    rng = np.random.default_rng(seed)
    H, W, n, f = 96, 128, 160, 110.0
    c = np.array([W / 2.0, H / 2.0])
    R, t, scale = synth.rodrigues(rng.normal(0.0, 0.2, 3)), rng.normal(0.0, 0.4, 3), 1.6
    f2 = f * 1.25 if kind == "varying_focal" else f
    dm = rng.uniform(2.0, 9.0, size=(2, H, W))
    kp = np.zeros((2, n, 2))
    used, k = set(), 0
    while k < n:
        u, v = int(rng.integers(4, W - 4)), int(rng.integers(4, H - 4))
        d1 = rng.uniform(3.0, 8.0)
        X2 = R @ (d1 * np.array([(u - c[0]) / f, (v - c[1]) / f, 1.0])) + t
        x2 = f2 * X2[:2] / X2[2] + c
        key1, key2 = (0, v, u), (1, int(x2[1]), int(x2[0]))
        if X2[2] < 0.5 or not (2 <= x2[0] < W - 2 and 2 <= x2[1] < H - 2) or key1 in used or key2 in used:
            continue
        used.update((key1, key2))
        dm[key1], dm[key2] = d1, X2[2] / scale
        kp[0, k], kp[1, k] = (u, v), x2
        k += 1
    return {"kp": kp, "dm": dm, "c": c, "f": (f, f2), "n": n, "H": H, "W": W, "scale": scale}


@pytest.mark.parametrize("kind", rc.KINDS)
def test_estimate_then_reconstruct_on_one_stream(torch, poselib, capi, kind):
    """estimate_image_pairs_torch, then reconstruct_image_pairs_torch(models="last"): byte for byte the call on the returned records, and geometrically
    right: at every inlier match image 1's transformed point meets image 2's point to 1e-5 relative (float32 output rounding 6e-8 plus the estimator's
    1e-6 on noise-free pairs).  Image 1's keypoints are pixel centres, image 2's are the sub-pixel projections, and a map has one depth per pixel: image
    2's point AT THE KEYPOINT is its pixel's depth along the keypoint's ray, z * ((x2 - c) / f2, (y2 - c) / f2, 1) with the row's own z; the row's x and y
    are checked against the pixel's ray in the same way."""
    s = _scene(kind)
    n, W = s["n"], s["W"]
    kp, dm = torch.from_numpy(s["kp"]).cuda(), torch.from_numpy(s["dm"]).cuda()
    matches = torch.arange(n, device="cuda").reshape(1, n, 1).expand(1, n, 2).contiguous()
    pairs = np.array([[0, 1]])
    cams = [{"model": "SIMPLE_PINHOLE", "width": W, "height": s["H"], "params": [s["f"][i], *s["c"]]} for i in range(2)] if kind == "calibrated" else None
    centers = None if kind == "calibrated" else s["c"]
    ro = {"max_iterations": 1000, "min_iterations": 1000, "max_epipolar_error": 0.5, "max_reproj_error": 2.0, "seed": 3}
    res, mask, n_used = poselib.estimate_image_pairs_torch(kind, kp, dm, pairs, matches, cams, ro, {"loss_type": "TRUNCATED_CAUCHY"}, centers)
    assert n_used[0] == n and res["num_inliers"][0] >= 0.95 * n
    last = poselib.reconstruct_image_pairs_torch(kind, "last", dm, pairs, cams, centers, rate=1.0)
    again = poselib.reconstruct_image_pairs_torch(kind, res, dm, pairs, cams, centers, rate=1.0)
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(last, again))
    points, pixel, counts = (t.cpu().numpy()[0] for t in last)
    n1 = s["H"] * W
    assert counts.tolist() == [n1, n1] and (pixel[:n1] == np.arange(n1)).all() and (pixel[n1:] == np.arange(n1)).all()
    inl = mask.cpu().numpy()[0].astype(bool)
    p1 = s["kp"][0].astype(np.int64)
    x2 = s["kp"][1]
    p2 = x2.astype(np.int64)
    P1 = points[p1[:, 1] * W + p1[:, 0]].astype(np.float64)
    row2 = points[n1 + p2[:, 1] * W + p2[:, 0]].astype(np.float64)
    m = res["model"][0]
    f2 = s["f"][1] if kind == "calibrated" else float(m["f2"])
    ray = lambda xy: np.concatenate([(xy - s["c"]) / f2, np.ones((n, 1))], axis=1)  # noqa: E731
    P2 = row2[:, 2:3] * ray(x2)
    err = np.abs(P1 - P2)[inl].max() / np.abs(P2[inl]).max()
    print(kind, "inliers", int(inl.sum()), "max relative distance at the inlier matches", err)
    assert err <= 1e-5
    assert np.abs(row2 - row2[:, 2:3] * ray(p2.astype(np.float64)))[inl].max() <= 1e-5 * np.abs(row2[inl]).max()
    assert abs(m["scale"] - s["scale"]) <= 1e-5 * s["scale"]


def test_last_needs_an_estimate_of_the_batch(torch, poselib):
    dm = torch.ones((2, 4, 4), device="cuda")
    side = torch.cuda.Stream()  # a stream no estimate ran on: its handle is fresh
    with torch.cuda.stream(side):
        with pytest.raises(ValueError, match="last"):
            poselib.reconstruct_pairs_torch("calibrated", "last", dm, dm, {"model": "SIMPLE_PINHOLE", "params": [50.0, 2.0, 2.0]},
                                            {"model": "SIMPLE_PINHOLE", "params": [50.0, 2.0, 2.0]})
    with pytest.raises(ValueError):
        poselib.reconstruct_pairs_torch("calibrated", "first", dm, dm, {"model": "SIMPLE_PINHOLE", "params": [50.0, 2.0, 2.0]},
                                        {"model": "SIMPLE_PINHOLE", "params": [50.0, 2.0, 2.0]})


# ---- refusals
def _set(**kw):
    def change(a):
        for k, v in kw.items():
            if "." in k:
                obj, field = k.split(".")
                setattr(a[obj], field, v)
            else:
                a[k] = v
    return change


REFUSALS = [
    ("null_depth", dict(change=_set(**{"desc.depth1": None})), "NULL depth map"),
    ("null_models", dict(change=_set(models=None)), "NULL models_dev or counts"),
    ("null_counts", dict(change=_set(counts=None)), "NULL models_dev or counts"),
    ("null_points", dict(change=_set(points=None)), "NULL points or pixel"),
    ("null_pixel", dict(change=_set(pixel=None)), "NULL points or pixel"),
    ("negative_batch", dict(change=_set(batch=-1)), "negative batch"),
    ("negative_size", dict(change=_set(**{"desc.h2": -1})), "negative size"),
    ("extent", dict(change=_set(**{"desc.w1": 65537})), "extent above MDRP_RECON_MAX_EXTENT (65536)"),
    ("pixels", dict(change=_set(**{"desc.w1": 65536, "desc.h1": 65536})), "a map of 2^31 pixels or more"),
    ("depth_type", dict(change=_set(**{"desc.depth_type": 2})), "depth_type must be MDRP_F32 or MDRP_F64"),
    ("keep", dict(change=_set(**{"opt.keep": 2})), "keep must be MDRP_KEEP_NOT_INF or MDRP_KEEP_FINITE"),
    ("thr", dict(change=_set(**{"opt.thr": 0})), "thr == 0 keeps nothing (1 .. MDRP_RECON_ALL)"),
    ("p_max", dict(change=_set(**{"opt.p_max": -1})), "negative p_max"),
    ("stride_small", dict(change=_set(stride=88)), "model_stride must be at least 96 and a multiple of 8"),
    ("stride_odd", dict(change=_set(stride=100)), "model_stride must be at least 96 and a multiple of 8"),
    ("kind_low", dict(change=_set(kind=-1)), "only the monodepth estimators' models (kind 0..2) have depths to unproject"),
    ("kind_high", dict(change=_set(kind=3)), "only the monodepth estimators' models (kind 0..2) have depths to unproject"),
    ("cameras_missing", dict(kind="calibrated", change=_set(cam2=None)), "MDRP_CALIB needs cam1_host and cam2_host, one record per pair"),
    ("cameras_given", dict(change=_set(cam1=rc.cameras(3)[0])), "cameras are MDRP_CALIB's: a focal kind unprojects with the model's focals (pass NULL)"),
    ("camera_model", dict(kind="calibrated", change=lambda a: a.update(cam1=np.array([(2, 0, [1, 1, 1, 1])] * 3, dtype=a["cam1"].dtype))),
     "only SIMPLE_PINHOLE (0) and PINHOLE (1) cameras unproject here"),
    ("image_null_pairs", dict(image_form=True, change=_set(**{"desc.pairs": None})), "NULL pairs"),
    ("image_negative_n", dict(image_form=True, change=_set(**{"desc.n_images": -1})), "negative size"),
    ("image_extent", dict(image_form=True, change=_set(**{"desc.h_max": 70000})), "extent above MDRP_RECON_MAX_EXTENT (65536)"),
]


@pytest.fixture(scope="module")
def fresh(capi):
    """the good calls' bytes on handles of their own"""
    out = {}
    for form in (False, True):
        h = capi.Handle(0)
        try:
            out[form] = rc.device_call(h, image_form=form)
        finally:
            h.close()
    return out


@pytest.mark.parametrize("name, args, message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_handle_usable(capi, fresh, name, args, message):
    """MDRP_ERR_INVALID with its message before any device work (the outputs keep their fill), then a good call returns a fresh handle's bytes"""
    form = args.get("image_form", False)
    who = "mdrp_reconstruct_image_pairs_async" if form else "mdrp_reconstruct_pairs_async"
    h = capi.Handle(0)
    try:
        with pytest.raises(capi.MdrpError) as e:
            rc.device_call(h, **args)
        assert str(e.value) == f"mdrp error 1: {who}: {message}", str(e.value)
        assert rc.device_call(h, image_form=form) == fresh[form]
    finally:
        h.close()


def test_null_descriptor_options_and_an_empty_batch(capi, fresh):
    import ctypes as C
    h = capi.Handle(0)
    try:
        lib = capi.load_library()
        opt, desc = capi.ReconstructOpt(0, 5, 0, 4, 0), capi.DepthPairs()
        for d, o in ((None, C.byref(opt)), (C.byref(desc), None)):
            assert lib.mdrp_reconstruct_pairs_async(h._h, 1, d, o, 1, None, 96, None, None, None, None, None) == 1
            assert lib.mdrp_last_error() == b"invalid argument"
        assert lib.mdrp_reconstruct_pairs_async(None, 1, C.byref(desc), C.byref(opt), 1, None, 96, None, None, None, None, None) == 1
        assert lib.mdrp_reconstruct_image_pairs_async(h._h, 1, None, C.byref(opt), 1, None, 96, None, None, None, None, None) == 1
        h.reconstruct_pairs_device(1, desc, opt, 0, None, 96, None, None, None)  # batch == 0 succeeds and does nothing
        h.reconstruct_pairs_device(1, capi.DepthImagePairs(), opt, 0, None, 96, None, None, None)
        assert rc.device_call(h) == fresh[False]
        assert rc.device_call(h, stride=136) == fresh[False]  # what mdrp_copy_results_device writes: the model at the front of 136 bytes
    finally:
        h.close()


def test_python_refusals(torch, poselib):
    dm = torch.ones((2, 4, 4), device="cuda")
    ms = rc.models("shared_focal", 2)
    for kw in (dict(rate=0.0), dict(rate=float("nan")), dict(rate=-1.0), dict(keep="both_inf"), dict(p_max=-1), dict(seed=-1),
               dict(cameras1={"model": "SIMPLE_PINHOLE", "params": [1.0, 0.0, 0.0]})):
        with pytest.raises(ValueError):
            poselib.reconstruct_pairs_torch("shared_focal", ms, dm, dm, **kw)
    with pytest.raises(ValueError):
        poselib.reconstruct_pairs_torch("shared_focal", ms[:1], dm, dm)  # one model for two pairs
    with pytest.raises(ValueError):
        poselib.reconstruct_pairs_torch("shared_focal", ms, dm, dm[:1])
    with pytest.raises(ValueError):
        poselib.reconstruct_pairs_torch("shared_focal", ms, dm, dm.double())
    with pytest.raises(ValueError):
        poselib.reconstruct_pairs_torch("relpose_5pt", ms, dm, dm)
    with pytest.raises(ValueError):
        poselib.reconstruct_pairs_torch("shared_focal", ms, dm.cpu(), dm.cpu())
    with pytest.raises(ValueError):
        poselib.reconstruct_image_pairs_torch("shared_focal", ms, dm, [[0, 1], [1, 0]], sizes=[[4, 4]])
    with pytest.raises(ValueError):
        poselib.reconstruct_pairs_torch("shared_focal", ms, torch.ones((2, 1, 65537), device="cuda"), dm)


def test_reconstruct_pair_for_numpy_users(poselib, capi):
    """the host convenience over the same device call: the definition's rows, trimmed to the written ones"""
    kind, dt, size = "calibrated", "float32", rc.SIZES[2]
    x = rc.inputs(kind, dt, size)
    m = x["models"][0]
    g = poselib.MonoDepthTwoViewGeometry(poselib.CameraPose(m["q"], m["t"]), m["scale"], m["shift1"], m["shift2"])
    cams = [poselib.Camera(int(x[k][0]["model_id"]), list(x[k][0]["params"][:4 if x[k][0]["model_id"] else 3])) for k in ("cam1", "cam2")]
    points, pixel, counts = poselib.reconstruct_pair(g, x["dm1"][0], x["dm2"][0], cams[0], cams[1], x["c1"][0], x["c2"][0], rate=0.5, seed=rc.SEED)
    want = rc.reference(kind, dt, size, "not_inf", 0.5, 1, sum(len(r[1]) for r in rc.rows(kind, dt, size, "not_inf", 0.5, 0)))
    assert points.tobytes() == want[0][0].tobytes() and pixel.tobytes() == want[1][0].tobytes() and counts.tolist() == want[2][0].tolist()
    pair = poselib.MonoDepthImagePair(g, poselib.Camera("SIMPLE_PINHOLE", [512.25, 0, 0]), poselib.Camera("SIMPLE_PINHOLE", [498.5, 0, 0]))
    p2, x2, c2 = poselib.reconstruct_pair(pair, x["dm1"][0], x["dm2"][0], center1=x["c1"][0], center2=x["c2"][0], rate=1.0)
    m2 = m.copy()
    m2["f1"], m2["f2"] = 512.25, 498.5
    w2 = frontend.reconstruct_pair_numpy(m2, "varying_focal", x["dm1"][0], x["dm2"][0], x["c1"][0], x["c2"][0])
    assert p2.tobytes() == w2[0].tobytes() and x2.tobytes() == w2[1].tobytes() and c2.tolist() == w2[2].tolist()
