"""The consistency filter of a scene on a real MI355X (include/mdrp_fuse.h): poselib.fuse_scene_torch against the NumPy definition
(mdrp_amd/frontend.py fuse_scene_numpy, rules F1-F6) as BYTES - points, pixel, support, offsets and transforms - over kinds, depth types, map sizes
(1 x 1, 5 x 7, 37 x 53, unequal valid regions inside a larger allocation), the trees of tests/fuse_cases.py (1, 2, 3 and 5 images: chain, star, mixed
edge directions, two roots, a subtree detached by an unusable model that other images list as views), V in {0, 1, 3, 8} with every inert kind of
slot, rates, tolerances, the four gates and p_max below, at and above the kept count; the open gate against reconstruct_scene_torch; a side stream;
the forms of models; estimate -> fuse on one stream; every refusal followed by a good call."""
import ctypes as C
import itertools

import numpy as np
import pytest

import fuse_cases as fc
from mdrp_amd import frontend

pytestmark = pytest.mark.gpu


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


def _check(got, want, what):
    assert got[4].tobytes() == want[4].tobytes(), ("transforms",) + what
    assert got[3].dtype == np.int64 and got[3].tobytes() == want[3].tobytes(), ("offsets",) + what + (got[3], want[3])
    assert got[2].dtype == np.uint8 and got[2].shape == want[2].shape and got[2].tobytes() == want[2].tobytes(), ("support",) + what
    assert fc.same_bytes(got[:2], want[:2]), ("rows",) + what


# ---- bytes against the definition
@pytest.mark.parametrize("shape", sorted(fc.SHAPES))
@pytest.mark.parametrize("dtype_name", fc.DTYPES)
@pytest.mark.parametrize("kind", fc.KINDS)
def test_bytes_equal_the_definition(kind, dtype_name, shape):
    """every tree and V for one kind, depth type and map size; the six (rate, tol) pairs go round over the 28 (tree, V) cases, one step further per
    tree, so each of them meets every V; all four gates at a generous p_max, and the default gate at p_max 0, below and at the kept count.  The
    inputs plant +inf, -inf, NaN, 0 and negative depths, non-zero centres and shifts, SIMPLE_PINHOLE and PINHOLE with fx != fy, models with full
    mantissas."""
    settings = itertools.cycle(itertools.product(fc.RATES, fc.TOLS))
    kept_somewhere = dropped_somewhere = 0
    for tree in fc.TREES:
        for V in fc.VS:
            rate, tol = next(settings)
            case = (kind, dtype_name, shape, tree, V, rate, tol)
            everything = fc.kept_count(*case, (0, V))
            for gate in fc.gates(V):
                n = fc.kept_count(*case, gate)
                for p_max in sorted({n + 1500} | ({0, n // 2, n} if gate == (1, 0) else set())):
                    _check(fc.run(*case, gate, p_max), fc.reference(*case, gate, p_max), (tree, V, rate, tol, gate, p_max))
                assert n == 0 or gate[0] <= V
                kept_somewhere += n
                dropped_somewhere += everything - n
        next(settings)
    assert dropped_somewhere > 0 and (kept_somewhere > 0 or shape == "1x1")


@pytest.mark.parametrize("kind", fc.KINDS)
def test_the_open_gate_is_reconstruct_scene_torch(torch, poselib, kind):
    for tree, shape, V, rate, keep in (("chain", "37x53", 8, 0.5, "not_inf"), ("forest", "unequal", 3, 1.0, "finite"), ("broken", "37x53", 0, 1.0, "not_inf")):
        x = fc.inputs(kind, "float32", shape, tree)
        dm = torch.from_numpy(x["dm"]).cuda()
        for p_max in (None, 300):
            scene = poselib.reconstruct_scene_torch(kind, x["models"], dm, x["pairs"], x["tree"], x["cams"], x["centers"], x["sizes"], rate, fc.SEED, keep, p_max,
                                                    return_transforms=True, return_image=True)
            fused = poselib.fuse_scene_torch(kind, x["models"], dm, x["pairs"], x["tree"], fc.views(x["I"], V), x["cams"], x["centers"], x["sizes"], rate, fc.SEED, keep,
                                             0.05, 0, V, p_max, return_transforms=True, return_image=True)
            points, pixel, support, offsets, T, image = fused
            assert fc.same_bytes([t.cpu().numpy() for t in (points, pixel, offsets, image, T)], [t.cpu().numpy() for t in scene]), (tree, p_max)
            assert points.shape[0] == scene[0].shape[0]  # p_max None: the scene's candidate bound
            want = fc.reference(kind, "float32", shape, tree, V, rate, 0.05, (0, V), points.shape[0], keep)
            assert support.cpu().numpy().tobytes() == want[2].tobytes()


def test_a_side_stream_the_forms_of_models_and_the_numpy_call(torch, poselib, capi):
    kind, dt, shape, tree, V, rate, tol, gate = "varying_focal", "float32", "37x53", "star", 3, 0.5, 0.05, (1, 0)
    x = fc.inputs(kind, dt, shape, tree)
    want = fc.reference(kind, dt, shape, tree, V, rate, tol, gate, 4000)
    records = np.zeros(len(x["models"]), dtype=capi.RESULT_DTYPE)
    records["model"] = x["models"]
    as_f64 = torch.from_numpy(np.ascontiguousarray(x["models"]).view(np.float64).reshape(-1, 12)).cuda()
    as_u8 = torch.from_numpy(np.ascontiguousarray(x["models"]).view(np.uint8).reshape(-1, 96)).cuda()
    for models in (records, as_f64, as_u8):
        _check(fc.run(kind, dt, shape, tree, V, rate, tol, gate, 4000, models=models), want, ("models",))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = fc.run(kind, dt, shape, tree, V, rate, tol, gate, 4000)
    _check(got, want, ("side stream",))
    views_on_device = torch.from_numpy(fc.views(x["I"], V)).cuda().to(torch.int64)
    _check(fc.run(kind, dt, shape, tree, V, rate, tol, gate, 4000, view_table=views_on_device), want, ("views as a tensor",))
    points, pixel, support, offsets, T, image = poselib.fuse_scene(kind, x["models"], x["dm"], x["pairs"], x["tree"], fc.views(x["I"], V), None, x["centers"], x["sizes"],
                                                                   rate, fc.SEED, "not_inf", tol, *gate)
    n = int(want[3][-1])
    assert len(pixel) == n and points.tobytes() == want[0][:n].tobytes() and support.tobytes() == want[2][:n].tobytes() and T.tobytes() == want[4].tobytes()
    assert image.tolist() == np.repeat(np.arange(x["I"]), np.diff(want[3])).tolist() and offsets.tobytes() == want[3].tobytes()


@pytest.mark.parametrize("kind", fc.KINDS)
def test_estimate_then_fuse_on_one_stream(torch, poselib, kind):
    """estimate_image_pairs_torch, then fuse_scene_torch(models="last"): byte for byte the call on the fetched records and the definition on them"""
    import test_gpu_scene as tgs
    from mdrp_amd import scene
    s = tgs._image_set(kind)
    W = s["W"]
    kp, dm = torch.from_numpy(s["kp"]).cuda(), torch.from_numpy(s["dm"]).cuda()
    cams = [{"model": "SIMPLE_PINHOLE", "width": W, "height": s["H"], "params": [s["f"][i], *s["c"]]} for i in range(4)] if kind == "calibrated" else None
    centers = None if kind == "calibrated" else s["c"]
    ro = {"max_iterations": 1000, "min_iterations": 1000, "max_epipolar_error": 0.5, "max_reproj_error": 2.0, "seed": 3}
    res, mask, n_used = poselib.estimate_image_pairs_torch(kind, kp, dm, s["pairs"], torch.from_numpy(s["matches"]).cuda(), cams, ro,
                                                           {"loss_type": "TRUNCATED_CAUCHY"}, centers)
    views = poselib.scene_views(s["pairs"], 4, 3, res["num_inliers"])
    assert sorted(views[1].tolist()) == [0, 2, 3] and views[0].tolist() == [1, -1, -1]  # image 1 is in all three pairs
    args = (dm, s["pairs"], s["tree"], views, cams, centers)
    kw = dict(rate=0.25, tol=0.5, min_consistent=1, max_violating=1, return_transforms=True)
    last = poselib.fuse_scene_torch(kind, "last", *args, **kw)
    fetched = poselib.fuse_scene_torch(kind, res, *args, **kw)
    assert fc.same_bytes([t.cpu().numpy() for t in last], [t.cpu().numpy() for t in fetched])
    cam_rec = None if cams is None else poselib._camera_records(cams, 4)
    lo, hi = frontend.covis_band(0.5)
    want = frontend.fuse_scene_numpy(res["model"], kind, s["dm"], s["pairs"], s["tree"], views, last[0].shape[0], centers, None, cam_rec, "not_inf",
                                     frontend.recon_threshold(0.25), 0, lo, hi, 1, 1)
    got = [t.cpu().numpy() for t in last[:4]] + [scene._records(last[4])]
    _check(got, want, ("last",))
    assert 0 < want[3][-1] < 4 * s["H"] * W


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


FUSE = "mdrp_fuse_scene_async"
KIND_MSG = "only the monodepth estimators' models (kind 0..2) have depths to unproject"
STRIDE_MSG = "model_stride must be at least 96 and a multiple of 8"
BAND_MSG = "lo and hi must be finite with 0 <= lo <= 1 <= hi"
GATE_MSG = "negative min_consistent or max_violating"
REFUSALS = [
    # everything the scene cloud's entry point refuses
    ("null_depth", dict(change=_set(**{"desc.depth": None})), "NULL depth map"),
    ("null_models", dict(change=_set(models=None)), "NULL models_dev or pairs"),
    ("null_pairs", dict(change=_set(**{"desc.pairs": None})), "NULL models_dev or pairs"),
    ("null_tree", dict(change=_set(tree=None)), "NULL tree_dev"),
    ("null_offsets", dict(change=_set(offsets=None)), "NULL offsets"),
    ("null_points", dict(change=_set(points=None)), "NULL points or pixel"),
    ("null_pixel", dict(change=_set(pixel=None)), "NULL points or pixel"),
    ("negative_batch", dict(change=_set(batch=-1)), "negative batch"),
    ("negative_n_images", dict(change=_set(**{"desc.n_images": -1})), "negative n_images"),
    ("negative_size", dict(change=_set(**{"desc.h_max": -1})), "negative size"),
    ("extent", dict(change=_set(**{"desc.w_max": 65537})), "extent above MDRP_RECON_MAX_EXTENT (65536)"),
    ("pixels", dict(change=_set(**{"desc.w_max": 65536, "desc.h_max": 65536})), "a map of 2^31 pixels or more"),
    ("depth_type", dict(change=_set(**{"desc.depth_type": 2})), "depth_type must be MDRP_F32 or MDRP_F64"),
    ("keep", dict(change=_set(**{"opt.keep": 2})), "keep must be MDRP_KEEP_NOT_INF or MDRP_KEEP_FINITE"),
    ("thr", dict(change=_set(**{"opt.thr": 0})), "thr == 0 keeps nothing (1 .. MDRP_RECON_ALL)"),
    ("p_max", dict(change=_set(**{"opt.p_max": -1})), "negative p_max"),
    ("stride_small", dict(change=_set(stride=88)), STRIDE_MSG),
    ("stride_odd", dict(change=_set(stride=100)), STRIDE_MSG),
    ("kind_low", dict(change=_set(kind=-1)), KIND_MSG),
    ("kind_high", dict(change=_set(kind=3)), KIND_MSG),
    ("cameras_missing", dict(kind="calibrated", change=_set(cams=None)), "MDRP_CALIB needs cams_host, one record per image"),
    ("cameras_given", dict(change=_set(cams=fc.cc.cameras(((37, 53), (37, 53)), 5)[0])), "cameras are MDRP_CALIB's: a focal kind unprojects with the model's focals (pass NULL)"),
    ("camera_model", dict(kind="calibrated", change=lambda a: a.update(cams=np.array([(2, 0, [1, 1, 1, 1])] * 5, dtype=a["cams"].dtype))),
     "only SIMPLE_PINHOLE (0) and PINHOLE (1) cameras unproject here"),
    ("tiles", dict(change=_set(**{"desc.w_max": 32768, "desc.h_max": 32768, "desc.n_images": 2048})), "the scene's tiles above 2^31 - 1: split the scene"),
    # the filter's own
    ("views_negative", dict(change=_set(**{"opt.n_views": -1})), "n_views must be 0 .. MDRP_FUSE_MAX_VIEWS (8)"),
    ("views_nine", dict(change=_set(**{"opt.n_views": 9})), "n_views must be 0 .. MDRP_FUSE_MAX_VIEWS (8)"),
    ("null_views", dict(change=_set(views=None)), "NULL views_dev"),
    ("lo_negative", dict(change=_set(**{"opt.lo": -0.1})), BAND_MSG),
    ("lo_above_one", dict(change=_set(**{"opt.lo": 1.01})), BAND_MSG),
    ("hi_below_one", dict(change=_set(**{"opt.hi": 0.99})), BAND_MSG),
    ("hi_inf", dict(change=_set(**{"opt.hi": float("inf")})), BAND_MSG),
    ("lo_nan", dict(change=_set(**{"opt.lo": float("nan")})), BAND_MSG),
    ("min_consistent", dict(change=_set(**{"opt.min_consistent": -1})), GATE_MSG),
    ("max_violating", dict(change=_set(**{"opt.max_violating": -1})), GATE_MSG),
    ("null_support", dict(change=_set(support=None)), "NULL support"),
]


@pytest.fixture(scope="module")
def fresh(capi):
    """the good calls' bytes on handles of their own"""
    out = {}
    for key, args in (("fuse", {}), ("calibrated", dict(kind="calibrated"))):
        h = capi.Handle(0)
        try:
            out[key] = fc.device_call(h, **args)
        finally:
            h.close()
    return out


def test_fresh_calls_are_the_definition(fresh):
    for key, kind in (("fuse", "varying_focal"), ("calibrated", "calibrated")):
        want = fc.reference(kind, "float32", "37x53", "chain", 3, 0.5, 0.05, (1, 0), 6000)
        assert fresh[key] == tuple(w.tobytes() for w in want) and 0 < want[3][-1] < 6000


@pytest.mark.parametrize("name, args, message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_handle_usable(capi, fresh, name, args, message):
    """MDRP_ERR_INVALID with its message before any device work, then a good call returns a fresh handle's bytes"""
    h = capi.Handle(0)
    try:
        with pytest.raises(capi.MdrpError) as e:
            fc.device_call(h, **args)
        assert str(e.value) == f"mdrp error 1: {FUSE}: {message}", str(e.value)
        assert fc.device_call(h, **{k: v for k, v in args.items() if k != "change"}) == fresh["calibrated" if args.get("kind") == "calibrated" else "fuse"]
    finally:
        h.close()


def test_null_descriptor_options_empty_scenes_and_no_transforms(capi, fresh, torch):
    h = capi.Handle(0)
    try:
        lib = capi.load_library()
        opt, desc = capi.FuseOpt(0, 5, 0, 4, 8, 0.95, 1.05, 1, 0), capi.DepthImagePairs()
        nothing = (None,) * 8
        for d, o in ((None, C.byref(opt)), (C.byref(desc), None)):
            assert lib.mdrp_fuse_scene_async(h._h, 1, d, o, 0, None, 96, *nothing) == 1
            assert lib.mdrp_last_error() == b"invalid argument"
        assert lib.mdrp_fuse_scene_async(None, 1, C.byref(desc), C.byref(opt), 0, None, 96, *nothing) == 1
        points = torch.full((4, 3), 7.0, device="cuda")
        pixel = torch.full((4,), 7, dtype=torch.int32, device="cuda")
        support = torch.full((4, 2), 7, dtype=torch.uint8, device="cuda")
        offsets = torch.full((1,), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        h.fuse_scene_device(1, desc, opt, 0, None, 96, None, None, points.data_ptr(), pixel.data_ptr(), support.data_ptr(), offsets.data_ptr())  # no image, n_views 8, no views
        h.synchronize()
        assert offsets.cpu().tolist() == [0] and not points.cpu().numpy().any() and pixel.cpu().tolist() == [-1] * 4 and not support.cpu().numpy().any()
        assert fc.device_call(h) == fresh["fuse"]
        assert fc.device_call(h, stride=136) == fresh["fuse"]  # what mdrp_copy_results_device writes: the model at the front of 136 bytes
        assert fc.device_call(h, with_transforms=False)[:4] == fresh["fuse"][:4]  # the records in the handle's scratch
        assert fc.device_call(h, V=0, gate=(0, 0), change=_set(views=None))[3] == fc.reference("varying_focal", "float32", "37x53", "chain", 0, 0.5, 0.05, (0, 0), 6000)[3].tobytes()
    finally:
        h.close()


def test_python_refusals(torch, poselib):
    dm = torch.ones((3, 4, 4), device="cuda")
    ms = fc.cc.models("shared_focal", 3)[[0, 2]]
    pairs, tree = poselib.video_tree(3)
    views = poselib.scene_views(pairs, 3)
    good = poselib.fuse_scene_torch("shared_focal", ms, dm, pairs, tree, views)
    assert len(good) == 4 and good[2].shape == (48, 2) and good[2].dtype == torch.uint8
    for kw, word in ((dict(rate=0.0), "rate"), (dict(rate=float("nan")), "rate"), (dict(keep="both_inf"), "keep"), (dict(p_max=-1), "p_max"), (dict(seed=-1), "seed"),
                     (dict(tol=-0.1), "tol"), (dict(tol=1.5), "tol"), (dict(min_consistent=-1), "min_consistent"), (dict(max_violating=-2), "max_violating"),
                     (dict(cameras={"model": "SIMPLE_PINHOLE", "params": [1.0, 0.0, 0.0]}), "cameras"), (dict(sizes=[[4, 4]]), None)):
        with pytest.raises(ValueError, match=word):
            poselib.fuse_scene_torch("shared_focal", ms, dm, pairs, tree, views, **kw)
    for bad, word in ((np.zeros((3, 9), dtype=np.int32), "views"), (np.zeros((2, 2), dtype=np.int32), "views"), (np.zeros((3, 2)), "views")):
        with pytest.raises(ValueError, match=word):
            poselib.fuse_scene_torch("shared_focal", ms, dm, pairs, tree, bad)
    with pytest.raises(ValueError):
        poselib.fuse_scene_torch("shared_focal", ms[:1], dm, pairs, tree, views)  # one model for two pairs
    with pytest.raises(ValueError, match="tree"):
        poselib.fuse_scene_torch("shared_focal", ms, dm, pairs, tree[:2], views)
    with pytest.raises(ValueError):
        poselib.fuse_scene_torch("shared_focal", ms, dm.cpu(), pairs, tree, views)
    side = torch.cuda.Stream()  # a stream no estimate ran on: its handle is fresh
    with torch.cuda.stream(side):
        with pytest.raises(ValueError, match="last"):
            poselib.fuse_scene_torch("shared_focal", "last", dm, pairs, tree, views)
    again = poselib.fuse_scene_torch("shared_focal", ms, dm, pairs, tree, views)  # every refusal followed by a good call
    assert fc.same_bytes([t.cpu().numpy() for t in again], [t.cpu().numpy() for t in good])
