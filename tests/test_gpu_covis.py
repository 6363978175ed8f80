"""Co-visibility on a real MI355X (include/mdrp_covis.h): poselib.covisibility_pairs_torch and covisibility_image_pairs_torch against the
NumPy definition (mdrp_amd/frontend.py, rules C1-C7) as BYTES, over kinds, depth types, map sizes around the lane and tile boundaries, batch sizes,
subsample rates and tolerances; the per-image form against the per-pair form; a side stream; the forms of models=; estimate -> covisibility on one
stream with the records left on the device; every refusal, each followed by a good call."""
import numpy as np
import pytest

import covis_cases as cc
from mdrp_amd import frontend

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "float64")
S, F, I, K, CO, OC, VI = range(7)


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
@pytest.mark.parametrize("size", cc.SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}")
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("kind", cc.KINDS)
def test_bytes_equal_the_definition(kind, dtype_name, size):
    """the cross product B x rate x tol for one kind, depth type and pair of map sizes.  The inputs plant +inf, -inf, NaN, 0 and negative depths, a
    whole row and a whole map of inf, non-zero centres and shifts, SIMPLE_PINHOLE and PINHOLE with fx != fy, models with full mantissas, C1's empty
    pairs at batch positions 1, 5, 9 and 13, a model that throws every point behind the target (6) and one that throws every point outside it (7)
    (covis_cases.py).  The definition's counters of a pair are computed once."""
    cases = 0
    for rate in cc.RATES:
        for tol in cc.TOLS:
            for B in cc.BATCHES:
                got = cc.run(kind, dtype_name, size, rate, tol, B)
                want = cc.reference(kind, dtype_name, size, rate, tol, B)
                assert got.dtype == want.dtype and got.shape == want.shape == (B, 2, 8), (got.dtype, got.shape)
                if got.tobytes() != want.tobytes():
                    bad = np.argwhere(got != want)
                    raise AssertionError((rate, tol, B, len(bad), bad[:3].tolist(), got[tuple(bad[0][:2])].tolist(), want[tuple(bad[0][:2])].tolist()))
                cases += 1
    assert cases == len(cc.BATCHES) * len(cc.RATES) * len(cc.TOLS)
    if size[0][0] >= 37:  # the cases did what they are there for
        c = cc.reference(kind, dtype_name, size, 1.0, 0.05, cc.B_MAX).astype(np.int64)
        assert (c[0, :, CO] > 0).all() and (c[0, :, OC] > 0).all() and (c[0, :, VI] > 0).all() and (c[0, :, I] > c[0, :, K]).all()
        assert (c[cc.BEHIND, :, S] > 0).all() and not c[cc.BEHIND, :, F].any() and (c[cc.OUTSIDE, :, F] > 0).all() and not c[cc.OUTSIDE, :, I].any()
        assert not c[list(cc.EMPTY)].any() and c[cc.INF_MAP[0], 0, S] == 0 and c[cc.INF_MAP[0], 1, K] == 0 and c[cc.INF_MAP[0], 1, I] > 0


def test_a_pair_does_not_depend_on_its_batch(torch, poselib):
    """pairs 3 and 8 alone, as a batch of two in the other order, and inside the batch of 17: the same counters (C2)"""
    kind, dt, size = "varying_focal", "float32", cc.SIZES[3]
    x = cc.inputs(kind, dt, size)

    def call(idx):
        return poselib.covisibility_pairs_torch(kind, x["models"][idx], torch.from_numpy(x["dm1"][idx]).cuda(), torch.from_numpy(x["dm2"][idx]).cuda(),
                                                center1=x["c1"][idx], center2=x["c2"][idx], rate=0.5, seed=cc.SEED).cpu().numpy()
    full, two = call(list(range(cc.B_MAX))), call([8, 3])
    for pos, b in enumerate((8, 3)):
        assert call([b])[0].tobytes() == two[pos].tobytes() == full[b].tobytes() == cc.pair_counts(kind, dt, size, 0.5, 0.05, b).tobytes(), b
    assert full[3, :, K].min() > 64


def test_inputs_from_a_side_stream(torch, poselib):
    """the maps and the models are produced by kernels on a side stream and the call is made on that stream: it is ordered behind them"""
    kind, dt, size = "calibrated", "float64", cc.SIZES[3]
    x = cc.inputs(kind, dt, size)
    want = cc.reference(kind, dt, size, 0.5, 0.05, 3)
    side = torch.cuda.Stream()
    host = [torch.from_numpy(x[k][:3].copy()).pin_memory() for k in ("dm1", "dm2")]
    models = torch.from_numpy(x["models"][:3].view(np.float64).reshape(3, 12).copy()).pin_memory()
    with torch.cuda.stream(side):
        big = torch.randn(4096, 4096, device="cuda")
        for _ in range(4):  # work in front of the copies, so that a call that did not wait would read unwritten maps
            big = big @ big * 1e-3
        dm1, dm2 = (t.to("cuda", non_blocking=True) * 1.0 for t in host)
        md = models.to("cuda", non_blocking=True) * 1.0
        got = poselib.covisibility_pairs_torch(kind, md, dm1, dm2, x["cam1"][:3], x["cam2"][:3], x["c1"][:3], x["c2"][:3], rate=0.5, seed=cc.SEED)
    side.synchronize()
    assert got.cpu().numpy().tobytes() == want.tobytes()


def test_the_forms_of_models(torch, poselib, capi):
    """a NumPy model array, the records an estimate returns, a float64 (B, 12) tensor and a uint8 (B, 96) tensor on the device: one result"""
    kind, dt, size = "shared_focal", "float32", cc.SIZES[2]
    x = cc.inputs(kind, dt, size)
    B = 5
    want = cc.reference(kind, dt, size, 1.0, 0.05, B)
    ms = x["models"][:B]
    rec = np.zeros(B, dtype=capi.RESULT_DTYPE)
    rec["model"] = ms
    flat = torch.from_numpy(ms.view(np.float64).reshape(B, 12).copy()).cuda()
    raw = torch.from_numpy(ms.view(np.uint8).reshape(B, 96).copy()).cuda()
    dm1, dm2 = torch.from_numpy(x["dm1"][:B]).cuda(), torch.from_numpy(x["dm2"][:B]).cuda()
    for form in (ms, rec, flat, raw):
        got = poselib.covisibility_pairs_torch(kind, form, dm1, dm2, center1=x["c1"][:B], center2=x["c2"][:B], rate=1.0, seed=cc.SEED)
        assert got.is_cuda and got.dtype == torch.int32 and got.cpu().numpy().tobytes() == want.tobytes()
    s = poselib.covisibility_scores(got)
    assert s["weight"].is_cuda and s["weight"].cpu().tolist() == (want[:, 0, CO].astype(np.int64) + want[:, 1, CO]).tolist()
    assert poselib.covisibility_pairs_torch(kind, ms[:0], dm1[:0], dm2[:0]).shape == (0, 2, 8)  # an empty batch


# ---- the per-image form
@pytest.mark.parametrize("kind, dtype_name", [("calibrated", "float32"), ("varying_focal", "float64")])
def test_per_image_form(torch, poselib, kind, dtype_name):
    """six images allocated 40 x 70 with smaller valid sizes, a repeated image, a == c, and two pairs with an index outside the set: bytes equal to
    the definition everywhere, and to the per-pair form on the expanded (and, for a smaller valid region, cropped) maps"""
    rng = np.random.default_rng(21)
    n_img, H, W = 6, 40, 70
    dm = cc.depth_maps(H, W, np.dtype(dtype_name), n=n_img, seed=33, whole_inf=99)
    sizes = np.array([[40, 70], [33, 50], [33, 50], [40, 64], [1, 70], [50, 80]], dtype=np.int32)  # (the last one is clamped to 40 x 70)
    pairs = np.array([[0, 5], [1, 2], [2, 2], [3, 0], [4, 1], [6, 0], [1, 2], [0, -1]], dtype=np.int64)
    ms = cc.models(kind, 11, seed=22)[[0, 2, 3, 4, 8, 10, 0, 2]]  # (usable ones: the empty pairs here are the two bad indices)
    cs = np.array([W / 2.0, H / 2.0]) * (kind != "calibrated") + rng.uniform(-1.5, 1.5, size=(n_img, 2))
    cams = cc.cameras(((H, W), (H, W)), n_img, seed=23)[0] if kind == "calibrated" else None
    ok = (pairs >= 0).all(1) & (pairs < n_img).all(1)
    safe = np.where(ok[:, None], pairs, 0)
    lo, hi = frontend.covis_band(0.05)
    want = frontend.covisibility_image_pairs_numpy(ms, kind, dm, pairs, cs, sizes, None if cams is None else cams[safe[:, 0]],
                                                   None if cams is None else cams[safe[:, 1]], frontend.recon_threshold(0.5), cc.SEED, lo, hi)
    got = poselib.covisibility_image_pairs_torch(kind, ms, torch.from_numpy(dm).cuda(), pairs, cams, cs, sizes, rate=0.5, seed=cc.SEED).cpu().numpy()
    assert got.shape == (8, 2, 8) and got.tobytes() == want.tobytes(), (got.tolist(), want.tolist())
    assert not got[5].any() and not got[7].any() and (got[[0, 1, 2, 3], :, K] > 0).all()  # an index outside the set: all counters zero
    assert got[2, 0, S] > 0 and got[4, 0, S] > 0  # a == c, and a one-row image
    # the per-pair form on the expanded tables: full-size images as they are, a cropped pair on its valid regions
    for b, crop in ((0, (slice(None), slice(None))), (1, (slice(0, 33), slice(0, 50)))):
        a, c = pairs[b]
        one = poselib.covisibility_pairs_torch(kind, ms[b:b + 1], torch.from_numpy(np.ascontiguousarray(dm[a][crop])[None]).cuda(),
                                               torch.from_numpy(np.ascontiguousarray(dm[c][crop])[None]).cuda(), None if cams is None else cams[a:a + 1],
                                               None if cams is None else cams[c:c + 1], cs[a], cs[c], rate=0.5, seed=cc.SEED)
        assert one.cpu().numpy()[0].tobytes() == got[b].tobytes(), b
    # pairs as a tensor on the device and sizes=None
    dev = poselib.covisibility_image_pairs_torch(kind, ms, torch.from_numpy(dm).cuda(), torch.from_numpy(pairs).cuda(), cams, cs, None, rate=0.5, seed=cc.SEED)
    full = frontend.covisibility_image_pairs_numpy(ms, kind, dm, pairs, cs, None, None if cams is None else cams[safe[:, 0]],
                                                   None if cams is None else cams[safe[:, 1]], frontend.recon_threshold(0.5), cc.SEED, lo, hi)
    assert dev.cpu().numpy().tobytes() == full.tobytes()


# ---- the chain on one stream
@pytest.mark.parametrize("kind", cc.KINDS)
def test_estimate_then_covisibility_on_one_stream(torch, poselib, kind):
    """estimate_image_pairs_torch, then covisibility_image_pairs_torch(models="last") on the synthetic pairs of the two-view back end's chain test:
    byte for byte the call on the returned records, and the estimated model agrees with the maps on strictly more pixels than the same model with
    its scale times 1.5, in both directions (every pixel sampled)."""
    import test_gpu_reconstruct as tgr
    s = tgr._scene(kind)
    n, W = s["n"], s["W"]
    kp, dm = torch.from_numpy(s["kp"]).cuda(), torch.from_numpy(s["dm"]).cuda()
    matches = torch.arange(n, device="cuda").reshape(1, n, 1).expand(1, n, 2).contiguous()
    pairs = np.array([[0, 1]])
    cams = [{"model": "SIMPLE_PINHOLE", "width": W, "height": s["H"], "params": [s["f"][i], *s["c"]]} for i in range(2)] if kind == "calibrated" else None
    centers = None if kind == "calibrated" else s["c"]
    ro = {"max_iterations": 1000, "min_iterations": 1000, "max_epipolar_error": 0.5, "max_reproj_error": 2.0, "seed": 3}
    res, mask, n_used = poselib.estimate_image_pairs_torch(kind, kp, dm, pairs, matches, cams, ro, {"loss_type": "TRUNCATED_CAUCHY"}, centers)
    assert n_used[0] == n and res["num_inliers"][0] >= 0.95 * n
    last = poselib.covisibility_image_pairs_torch(kind, "last", dm, pairs, cams, centers, rate=1.0)
    again = poselib.covisibility_image_pairs_torch(kind, res, dm, pairs, cams, centers, rate=1.0)
    assert last.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    wrong = res["model"].copy()
    wrong["scale"] *= 1.5
    worse = poselib.covisibility_image_pairs_torch(kind, wrong, dm, pairs, cams, centers, rate=1.0).cpu().numpy()[0]
    good = last.cpu().numpy()[0]
    print(kind, "estimated", good.tolist(), "scale x 1.5", worse.tolist())
    assert (good[:, S] == s["H"] * W).all() and (good[:, CO] > worse[:, CO]).all()
    cam_rec = None if cams is None else [{"model_id": 0, "params": [s["f"][i], *s["c"], 0.0]} for i in range(2)]
    want = frontend.covisibility_pair_numpy(res["model"][0], kind, s["dm"][0], s["dm"][1], centers, centers, None if cams is None else cam_rec[0],
                                            None if cams is None else cam_rec[1], frontend.RECON_ALL, 0, *frontend.covis_band(0.05))
    assert good.tobytes() == want.tobytes()


def test_last_needs_an_estimate_of_the_batch(torch, poselib):
    dm = torch.ones((2, 4, 4), device="cuda")
    cam = {"model": "SIMPLE_PINHOLE", "params": [50.0, 2.0, 2.0]}
    side = torch.cuda.Stream()  # a stream no estimate ran on: its handle is fresh
    with torch.cuda.stream(side):
        with pytest.raises(ValueError, match="last"):
            poselib.covisibility_pairs_torch("calibrated", "last", dm, dm, cam, cam)
    with pytest.raises(ValueError):
        poselib.covisibility_pairs_torch("calibrated", "first", dm, dm, cam, cam)


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


BAND = "lo and hi must be finite with 0 <= lo <= 1 <= hi"
REFUSALS = [
    ("null_depth", dict(change=_set(**{"desc.depth1": None})), "NULL depth map"),
    ("null_models", dict(change=_set(models=None)), "NULL models_dev or counts"),
    ("null_counts", dict(change=_set(counts=None)), "NULL models_dev or counts"),
    ("negative_batch", dict(change=_set(batch=-1)), "negative batch"),
    ("negative_size", dict(change=_set(**{"desc.h2": -1})), "negative size"),
    ("extent", dict(change=_set(**{"desc.w1": 65537})), "extent above MDRP_RECON_MAX_EXTENT (65536)"),
    ("pixels", dict(change=_set(**{"desc.w1": 65536, "desc.h1": 65536})), "a map of 2^31 pixels or more"),
    ("depth_type", dict(change=_set(**{"desc.depth_type": 2})), "depth_type must be MDRP_F32 or MDRP_F64"),
    ("thr", dict(change=_set(**{"opt.thr": 0})), "thr == 0 keeps nothing (1 .. MDRP_RECON_ALL)"),
    ("lo_negative", dict(change=_set(**{"opt.lo": -0.01})), BAND),
    ("lo_above_one", dict(change=_set(**{"opt.lo": 1.01, "opt.hi": 1.02})), BAND),
    ("hi_below_one", dict(change=_set(**{"opt.hi": 0.99})), BAND),
    ("lo_nan", dict(change=_set(**{"opt.lo": float("nan")})), BAND),
    ("hi_inf", dict(change=_set(**{"opt.hi": float("inf")})), BAND),
    ("hi_nan", dict(change=_set(**{"opt.hi": float("nan")})), BAND),
    ("stride_small", dict(change=_set(stride=88)), "model_stride must be at least 96 and a multiple of 8"),
    ("stride_odd", dict(change=_set(stride=100)), "model_stride must be at least 96 and a multiple of 8"),
    ("kind_low", dict(change=_set(kind=-1)), "only the monodepth estimators' models (kind 0..2) have depths to unproject"),
    ("kind_high", dict(change=_set(kind=3)), "only the monodepth estimators' models (kind 0..2) have depths to unproject"),
    ("cameras_missing", dict(kind="calibrated", change=_set(cam2=None)), "MDRP_CALIB needs cam1_host and cam2_host, one record per pair"),
    ("cameras_given", dict(change=_set(cam1=cc.cameras(cc.SIZES[2], 3)[0])), "cameras are MDRP_CALIB's: a focal kind unprojects with the model's focals (pass NULL)"),
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
            out[form] = cc.device_call(h, image_form=form)
        finally:
            h.close()
    return out


def test_fresh_calls_are_the_definition(fresh):
    assert fresh[False][0] == cc.reference("varying_focal", "float32", cc.SIZES[2], 0.5, 0.05, 3).tobytes()
    assert fresh[True][0] != fresh[False][0] and np.frombuffer(fresh[True][0], dtype=np.int32).reshape(3, 2, 8)[0, :, K].min() > 0


@pytest.mark.parametrize("name, args, message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_handle_usable(capi, fresh, name, args, message):
    """MDRP_ERR_INVALID with its message before any device work, then a good call returns a fresh handle's bytes"""
    form = args.get("image_form", False)
    who = "mdrp_covisibility_image_pairs_async" if form else "mdrp_covisibility_pairs_async"
    h = capi.Handle(0)
    try:
        with pytest.raises(capi.MdrpError) as e:
            cc.device_call(h, **args)
        assert str(e.value) == f"mdrp error 1: {who}: {message}", str(e.value)
        assert cc.device_call(h, image_form=form) == fresh[form]
    finally:
        h.close()


def test_null_descriptor_options_and_an_empty_batch(capi, fresh):
    import ctypes as C
    h = capi.Handle(0)
    try:
        lib = capi.load_library()
        opt, desc = capi.CovisOpt(5, 0, 0, 0.95, 1.05), capi.DepthPairs()
        for d, o in ((None, C.byref(opt)), (C.byref(desc), None)):
            assert lib.mdrp_covisibility_pairs_async(h._h, 1, d, o, 1, None, 96, None, None, None) == 1
            assert lib.mdrp_last_error() == b"invalid argument"
        assert lib.mdrp_covisibility_pairs_async(None, 1, C.byref(desc), C.byref(opt), 1, None, 96, None, None, None) == 1
        assert lib.mdrp_covisibility_image_pairs_async(h._h, 1, None, C.byref(opt), 1, None, 96, None, None, None) == 1
        h.covisibility_pairs_device(1, desc, opt, 0, None, 96, None)  # batch == 0 succeeds and does nothing
        h.covisibility_pairs_device(1, capi.DepthImagePairs(), opt, 0, None, 96, None)
        assert cc.device_call(h) == fresh[False]
        assert cc.device_call(h, stride=136) == fresh[False]  # what mdrp_copy_results_device writes: the model at the front of 136 bytes
        assert cc.device_call(h, tol=0.0) != fresh[False]
    finally:
        h.close()


def test_python_refusals(torch, poselib):
    dm = torch.ones((2, 4, 4), device="cuda")
    ms = cc.models("shared_focal", 2)
    for kw in (dict(rate=0.0), dict(rate=float("nan")), dict(rate=-1.0), dict(seed=-1), dict(tol=-0.1), dict(tol=1.5), dict(tol=float("nan")),
               dict(cameras1={"model": "SIMPLE_PINHOLE", "params": [1.0, 0.0, 0.0]})):
        with pytest.raises(ValueError):
            poselib.covisibility_pairs_torch("shared_focal", ms, dm, dm, **kw)
    with pytest.raises(ValueError):
        poselib.covisibility_pairs_torch("shared_focal", ms[:1], dm, dm)  # one model for two pairs
    with pytest.raises(ValueError):
        poselib.covisibility_pairs_torch("shared_focal", ms, dm, dm[:1])
    with pytest.raises(ValueError):
        poselib.covisibility_pairs_torch("shared_focal", ms, dm, dm.double())
    with pytest.raises(ValueError):
        poselib.covisibility_pairs_torch("relpose_5pt", ms, dm, dm)
    with pytest.raises(ValueError):
        poselib.covisibility_pairs_torch("shared_focal", ms, dm.cpu(), dm.cpu())
    with pytest.raises((TypeError, ValueError)):
        poselib.covisibility_pairs_torch("calibrated", ms, dm, dm)  # no cameras
    with pytest.raises(ValueError):
        poselib.covisibility_image_pairs_torch("shared_focal", ms, dm, [[0, 1], [1, 0]], sizes=[[4, 4]])
    with pytest.raises(ValueError):
        poselib.covisibility_image_pairs_torch("shared_focal", ms, dm, [[0, 1], [1, 0]], cameras={"model": "SIMPLE_PINHOLE", "params": [1.0, 0.0, 0.0]})
    with pytest.raises(ValueError):
        poselib.covisibility_pairs_torch("shared_focal", ms, torch.ones((2, 1, 65537), device="cuda"), dm)
    good = poselib.covisibility_pairs_torch("shared_focal", ms, dm, dm)  # and a good call behind them
    assert good.shape == (2, 2, 8)


def test_covisibility_pair_for_numpy_users(poselib):
    """the host convenience over the same device call: the definition's counters"""
    kind, dt, size = "calibrated", "float32", cc.SIZES[2]
    x = cc.inputs(kind, dt, size)
    m = x["models"][0]
    g = poselib.MonoDepthTwoViewGeometry(poselib.CameraPose(m["q"], m["t"]), m["scale"], m["shift1"], m["shift2"])
    cams = [poselib.Camera(int(x[k][0]["model_id"]), list(x[k][0]["params"][:4 if x[k][0]["model_id"] else 3])) for k in ("cam1", "cam2")]
    counts = poselib.covisibility_pair(g, x["dm1"][0], x["dm2"][0], cams[0], cams[1], x["c1"][0], x["c2"][0], rate=0.5, seed=cc.SEED)
    assert isinstance(counts, np.ndarray) and counts.tobytes() == cc.pair_counts(kind, dt, size, 0.5, 0.05, 0).tobytes()
