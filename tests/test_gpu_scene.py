"""Scenes on a real MI355X (include/mdrp_scene.h): poselib.reconstruct_scene_torch and scene_transforms_torch against the NumPy definition
(mdrp_amd/frontend.py, rules S1-S6) as BYTES over kinds, depth types, the tree cases of tests/scene_cases.py (1, 2, 5 and 9 images with valid regions
from 1 x 1 to 33 x 70; chain of depth 8, star, mixed directions, two roots, every detached case), subsample rates, both depth filters and S6's five
p_max cases; an image's rows against what else the scene holds, a side stream, the three forms of models; estimate -> scene on one stream; every
refusal."""
import numpy as np
import pytest

import scene_cases as sc
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
@pytest.mark.parametrize("name", sorted(sc.TREES))
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("kind", sc.KINDS)
def test_bytes_equal_the_definition(kind, dtype_name, name):
    """the cross product rate x keep x p_max for one kind, depth type and tree case: transforms, points, pixel and offsets.  The inputs plant +inf,
    -inf, NaN, 0 and negative depths, a whole row and a whole map of inf, non-zero centres and shifts, SIMPLE_PINHOLE and PINHOLE with fx != fy,
    models with full mantissas and negative scales."""
    for rate in sc.RATES:
        for keep in sc.KEEPS:
            for p_max in sc.p_max_cases(kind, dtype_name, name, keep, rate):
                got = sc.run(kind, dtype_name, name, keep, rate, p_max)
                want = sc.reference(kind, dtype_name, name, keep, rate, p_max)
                assert got[3].tobytes() == want[3].tobytes(), ("transforms", rate, keep, p_max)
                assert got[2].dtype == np.int64 and got[2].tobytes() == want[2].tobytes(), ("offsets", rate, keep, p_max, got[2], want[2])
                assert sc.same_bytes(got[:2], want[:2]), ("rows", rate, keep, p_max)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_scene_transforms_alone(torch, poselib, kind):
    from mdrp_amd import scene
    for name in sorted(sc.TREES):
        x = sc.inputs(kind, "float32", name)
        got = scene._records(poselib.scene_transforms_torch(kind, x["models"], x["pairs"], x["tree"], x["I"]))
        assert got.tobytes() == sc.transforms(kind, name).tobytes(), name
    x = sc.inputs(kind, "float32", "chain")
    on_device = poselib.scene_transforms_torch(kind, x["models"], torch.from_numpy(x["pairs"]).cuda().long(), torch.from_numpy(x["tree"]).cuda(), 9)
    assert scene._records(on_device).tobytes() == sc.transforms(kind, "chain").tobytes()
    assert poselib.scene_transforms_torch(kind, x["models"][:0], np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32), 0).shape == (0, 128)


def test_default_p_max_image_index_and_the_numpy_call(torch, poselib):
    from mdrp_amd import reconstruct
    kind, name = "calibrated", "forest"
    x = sc.inputs(kind, "float32", name)
    dm = torch.from_numpy(x["dm"]).cuda()
    points, pixel, offsets, image = poselib.reconstruct_scene_torch(kind, x["models"], dm, x["pairs"], x["tree"], x["cams"], x["centers"], x["sizes"], rate=0.5,
                                                                    seed=sc.SEED, return_image=True)
    p_max = reconstruct.default_p_max(5 * sc.H * sc.W, frontend.recon_threshold(0.5))
    want = sc.reference(kind, "float32", name, "not_inf", 0.5, p_max)
    assert points.shape == (p_max, 3) and sc.same_bytes([t.cpu().numpy() for t in (points, pixel, offsets)], want[:3])
    off = want[2]
    want_image = np.full(p_max, -1, dtype=np.int64)
    for i in range(5):
        want_image[off[i]:off[i + 1]] = i
    assert image.dtype == torch.int64 and (image.cpu().numpy() == want_image).all()
    p, px, o, im, T = poselib.reconstruct_scene(kind, x["models"], x["dm"], x["pairs"], x["tree"], x["cams"], x["centers"], x["sizes"], rate=0.5, seed=sc.SEED)
    n = int(off[-1])
    assert p.tobytes() == want[0][:n].tobytes() and px.tobytes() == want[1][:n].tobytes() and o.tobytes() == off.tobytes()
    assert (im == want_image[:n]).all() and T.tobytes() == want[3].tobytes()


# ---- independence
@pytest.mark.parametrize("kind", sc.KINDS)
def test_an_images_rows_do_not_depend_on_the_rest_of_the_scene(torch, poselib, capi, kind):
    """the star's images 0, 1 and 2: alone as a scene of three, in the scene of five, and with images 3 (absent) and 4 (a NaN pose) taken out; on a
    side stream; with models as result records, as a float64 (B, 12) tensor and as a uint8 (B, 96) tensor"""
    x = sc.inputs(kind, "float32", "star")
    dm = torch.from_numpy(x["dm"]).cuda()
    cams = x["cams"]
    args = dict(rate=0.5, seed=sc.SEED, p_max=7000)

    def rows_of(out, images):
        p, px, off = (t.cpu().numpy() for t in out[:3])
        return [(p[off[i]:off[i + 1]].tobytes(), px[off[i]:off[i + 1]].tobytes()) for i in images]

    full = poselib.reconstruct_scene_torch(kind, x["models"], dm, x["pairs"], x["tree"], cams, x["centers"], x["sizes"], **args)
    want = sc.reference(kind, "float32", "star", "not_inf", 0.5, 7000)
    assert sc.same_bytes([t.cpu().numpy() for t in full], want[:3])
    base = rows_of(full, (0, 1, 2))
    assert all(len(r[1]) > 0 for r in base[::2])
    three = poselib.reconstruct_scene_torch(kind, x["models"][:2], dm[:3], x["pairs"][:2], x["tree"][:3], None if cams is None else cams[:3], x["centers"][:3],
                                            x["sizes"][:3], **args)
    assert rows_of(three, (0, 1, 2)) == base
    tree, ms = x["tree"].copy(), x["models"].copy()
    tree[3, 1] = capi.SCENE_ABSENT
    ms[3] = sc.rc.models(kind)[1]
    fewer = poselib.reconstruct_scene_torch(kind, ms, dm, x["pairs"], tree, cams, x["centers"], x["sizes"], **args)
    assert rows_of(fewer, (0, 1, 2)) == base and fewer[2].cpu().numpy()[-1] == full[2].cpu().numpy()[3]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = poselib.reconstruct_scene_torch(kind, x["models"], dm, x["pairs"], x["tree"], cams, x["centers"], x["sizes"], **args)
    side.synchronize()
    assert sc.same_bytes([t.cpu().numpy() for t in on_side], want[:3])
    rec = np.zeros(len(x["models"]), dtype=capi.RESULT_DTYPE)
    rec["model"] = x["models"]
    as_f64 = torch.from_numpy(x["models"].view(np.float64).reshape(-1, 12).copy()).cuda()
    as_u8 = torch.from_numpy(x["models"].view(np.uint8).reshape(-1, 96).copy()).cuda()
    for models in (rec, as_f64, as_u8):
        out = poselib.reconstruct_scene_torch(kind, models, dm, x["pairs"], x["tree"], cams, x["centers"], x["sizes"], **args)
        assert sc.same_bytes([t.cpu().numpy() for t in out], want[:3])


# ---- estimate -> scene on one stream
def _image_set(kind, seed=41):
    """Four noise-free images with consistent geometry and three tree edges: pair 0 = (1, 0) and pair 2 = (3, 1) are forward edges, pair 1 = (1, 2) is
    an inverse one (image 2 hangs on image 1 as the pair's image 2).  As the front-end tests build theirs: image a's keypoints sit ON pixel centres,
    image c's where the points project, and each map holds a point's depth at its keypoint's pixel, in the image's own depth unit alpha_i."""
    from mdrp_amd import synth
    rng = np.random.default_rng(seed)
    H, W, n, f0 = 96, 128, 150, 110.0
    c = np.array([W / 2.0, H / 2.0])
    I, pairs, tree = 4, np.array([(1, 0), (1, 2), (3, 1)]), np.array([(0, 2), (0, 1), (1, 1), (2, 1)])
    Rw = [np.eye(3)] + [synth.rodrigues(rng.normal(0.0, 0.15, 3)) for _ in range(3)]  # X_i = Rw_i X_0 + tw_i, metric
    tw = [np.zeros(3)] + [rng.normal(0.0, 0.3, 3) for _ in range(3)]
    alpha = np.array([1.0, 1.6, 0.7, 1.25])
    f = np.full(I, f0) if kind != "varying_focal" else np.array([f0, f0 * 1.25, f0 * 0.9, f0 * 1.1])
    dm = rng.uniform(2.0, 9.0, size=(I, H, W))
    kp = np.zeros((I, 3 * n, 2))  # (image 1 is in all three pairs)
    n_kp, used = [0] * I, set()
    matches = np.full((3, n, 2), -1, dtype=np.int64)
    truth = {}  # (image, keypoint) -> the point in image 0's frame and unit
    for b, (a, cc) in enumerate(pairs):
        k = 0
        while k < n:
            u, v = int(rng.integers(4, W - 4)), int(rng.integers(4, H - 4))
            Za = rng.uniform(3.0, 8.0)
            Xa = Za * np.array([(u - c[0]) / f[a], (v - c[1]) / f[a], 1.0])
            X0 = Rw[a].T @ (Xa - tw[a])
            Xc = Rw[cc] @ X0 + tw[cc]
            x2 = f[cc] * Xc[:2] / Xc[2] + c
            key1, key2 = (a, v, u), (cc, int(x2[1]), int(x2[0]))
            if Xc[2] < 0.5 or not (2 <= x2[0] < W - 2 and 2 <= x2[1] < H - 2) or key1 in used or key2 in used:
                continue
            used.update((key1, key2))
            dm[key1], dm[key2] = Za / alpha[a], Xc[2] / alpha[cc]
            kp[a, n_kp[a]], kp[cc, n_kp[cc]] = (u, v), x2
            matches[b, k] = (n_kp[a], n_kp[cc])
            truth[(a, n_kp[a])] = truth[(cc, n_kp[cc])] = X0 / alpha[0]
            n_kp[a] += 1; n_kp[cc] += 1
            k += 1
    return {"kp": kp, "dm": dm, "c": c, "f": f, "n": n, "H": H, "W": W, "pairs": pairs, "tree": tree, "matches": matches, "truth": truth, "n_kp": n_kp}


@pytest.mark.parametrize("kind", sc.KINDS)
def test_estimate_then_scene_on_one_stream(torch, poselib, kind):
    """estimate_image_pairs_torch, then reconstruct_scene_torch(models="last"): byte for byte the definition on the fetched records, and geometrically
    right: at the inlier matches an image's points are the scene's points in the root's frame to 1e-5 relative PER EDGE of its depth (the two-view
    test's bound, tests/test_gpu_reconstruct.py, times the depth).  Images 1 (depth 1) and 3 (depth 2) hold their keypoints on pixel centres: their
    emitted rows are checked.  Image 2 (depth 2, an inverse edge) holds sub-pixel projections and one depth per pixel: its point AT THE KEYPOINT is its
    pixel's depth along the keypoint's ray, carried by its transform record."""
    from mdrp_amd import scene
    s = _image_set(kind)
    n, W = s["n"], s["W"]
    kp, dm = torch.from_numpy(s["kp"]).cuda(), torch.from_numpy(s["dm"]).cuda()
    cams = [{"model": "SIMPLE_PINHOLE", "width": W, "height": s["H"], "params": [s["f"][i], *s["c"]]} for i in range(4)] if kind == "calibrated" else None
    centers = None if kind == "calibrated" else s["c"]
    ro = {"max_iterations": 1000, "min_iterations": 1000, "max_epipolar_error": 0.5, "max_reproj_error": 2.0, "seed": 3}
    res, mask, n_used = poselib.estimate_image_pairs_torch(kind, kp, dm, s["pairs"], torch.from_numpy(s["matches"]).cuda(), cams, ro,
                                                           {"loss_type": "TRUNCATED_CAUCHY"}, centers)
    assert (n_used == n).all() and (res["num_inliers"] >= 0.95 * n).all()
    last = poselib.reconstruct_scene_torch(kind, "last", dm, s["pairs"], s["tree"], cams, centers, rate=1.0, return_transforms=True)
    cam_rec = None if cams is None else poselib._camera_records(cams, 4)
    want = frontend.reconstruct_scene_numpy(res["model"], kind, s["dm"], s["pairs"], s["tree"], last[0].shape[0], centers, None, cam_rec)
    T = scene._records(last[3])
    assert sc.same_bytes([t.cpu().numpy() for t in last[:3]], want[:3]) and T.tobytes() == want[3].tobytes()
    assert T["root"].tolist() == [0, 0, 0, 0] and T["depth"].tolist() == [0, 1, 2, 2]
    points, offsets = last[0].cpu().numpy().astype(np.float64), last[2].cpu().numpy()
    inl = mask.cpu().numpy().astype(bool)
    scale = max(np.abs(v).max() for v in s["truth"].values())
    for b, image, side in ((0, 1, 0), (2, 3, 0), (1, 2, 1)):
        ks = s["matches"][b][inl[b], side]
        want_pts = np.array([s["truth"][(image, k)] for k in ks])
        xy = s["kp"][image][ks]
        px = xy.astype(np.int64)
        if side == 0:   # keypoints on pixel centres: the emitted rows (rate 1: row = offsets[image] + v * W + u)
            got = points[offsets[image] + px[:, 1] * W + px[:, 0]]
        else:           # sub-pixel keypoints: the pixel's depth along the keypoint's ray, through the image's record
            cam = None if cam_rec is None else cam_rec[image]
            got = frontend.scene_transform_points(T[image], frontend.scene_unproject(T[image], kind, xy[:, 1], xy[:, 0], s["dm"][image][px[:, 1], px[:, 0]], centers, cam))
        err = np.abs(got - want_pts).max() / scale
        print(kind, "image", image, "depth", T["depth"][image], "inliers", len(ks), "max relative distance to the root's points", err)
        assert err <= 1e-5 * T["depth"][image]


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


SCENE = "mdrp_reconstruct_scene_async"
TRANSFORMS = "mdrp_scene_transforms_async"
KIND_MSG = "only the monodepth estimators' models (kind 0..2) have depths to unproject"
STRIDE_MSG = "model_stride must be at least 96 and a multiple of 8"
REFUSALS = [
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
    ("cameras_given", dict(change=_set(cams=sc.rc.cameras(9)[0])), "cameras are MDRP_CALIB's: a focal kind unprojects with the model's focals (pass NULL)"),
    ("camera_model", dict(kind="calibrated", change=lambda a: a.update(cams=np.array([(2, 0, [1, 1, 1, 1])] * 9, dtype=a["cams"].dtype))),
     "only SIMPLE_PINHOLE (0) and PINHOLE (1) cameras unproject here"),
    ("tiles", dict(change=_set(**{"desc.w_max": 32768, "desc.h_max": 32768, "desc.n_images": 2048})), "the scene's tiles above 2^31 - 1: split the scene"),
    ("transforms_null_tree", dict(transforms_only=True, change=_set(tree=None)), "NULL tree_dev"),
    ("transforms_null_out", dict(transforms_only=True, change=_set(transforms=None)), "NULL transforms_dev"),
    ("transforms_null_models", dict(transforms_only=True, change=_set(models=None)), "NULL models_dev or pairs"),
    ("transforms_null_pairs", dict(transforms_only=True, change=_set(pairs=None)), "NULL models_dev or pairs"),
    ("transforms_negative_batch", dict(transforms_only=True, change=_set(batch=-1)), "negative batch"),
    ("transforms_negative_n", dict(transforms_only=True, change=_set(n_images=-1)), "negative n_images"),
    ("transforms_kind", dict(transforms_only=True, change=_set(kind=3)), KIND_MSG),
    ("transforms_stride", dict(transforms_only=True, change=_set(stride=90)), STRIDE_MSG),
]


@pytest.fixture(scope="module")
def fresh(capi):
    """the good calls' bytes on handles of their own"""
    out = {}
    for key, args in (("scene", {}), ("calibrated", dict(kind="calibrated")), ("transforms", dict(transforms_only=True))):
        h = capi.Handle(0)
        try:
            out[key] = sc.device_call(h, **args)
        finally:
            h.close()
    return out


def test_fresh_calls_are_the_definition(fresh):
    want = sc.reference("varying_focal", "float32", "chain", "not_inf", 0.5, 6000)
    assert fresh["scene"] == tuple(w.tobytes() for w in want) and fresh["transforms"] == (want[3].tobytes(),)
    assert fresh["calibrated"] == tuple(w.tobytes() for w in sc.reference("calibrated", "float32", "chain", "not_inf", 0.5, 6000))


@pytest.mark.parametrize("name, args, message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_handle_usable(capi, fresh, name, args, message):
    """MDRP_ERR_INVALID with its message before any device work, then a good call returns a fresh handle's bytes"""
    only = args.get("transforms_only", False)
    h = capi.Handle(0)
    try:
        with pytest.raises(capi.MdrpError) as e:
            sc.device_call(h, **args)
        assert str(e.value) == f"mdrp error 1: {TRANSFORMS if only else SCENE}: {message}", str(e.value)
        key = "transforms" if only else ("calibrated" if args.get("kind") == "calibrated" else "scene")
        assert sc.device_call(h, **{k: v for k, v in args.items() if k != "change"}) == fresh[key]
    finally:
        h.close()


def test_null_descriptor_options_empty_scenes_and_no_transforms(capi, fresh, torch):
    import ctypes as C
    h = capi.Handle(0)
    try:
        lib = capi.load_library()
        opt, desc = capi.ReconstructOpt(0, 5, 0, 4, 0), capi.DepthImagePairs()
        for d, o in ((None, C.byref(opt)), (C.byref(desc), None)):
            assert lib.mdrp_reconstruct_scene_async(h._h, 1, d, o, 0, None, 96, None, None, None, None, None, None) == 1
            assert lib.mdrp_last_error() == b"invalid argument"
        assert lib.mdrp_reconstruct_scene_async(None, 1, C.byref(desc), C.byref(opt), 0, None, 96, None, None, None, None, None, None) == 1
        assert lib.mdrp_scene_transforms_async(None, 1, 0, None, 96, None, 0, None, None) == 1
        h.scene_transforms_device(1, 0, None, 96, None, 0, None, None)  # no image: succeeds and does nothing
        points = torch.full((4, 3), 7.0, device="cuda")
        pixel = torch.full((4,), 7, dtype=torch.int32, device="cuda")
        offsets = torch.full((1,), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        h.reconstruct_scene_device(1, desc, opt, 0, None, 96, None, points.data_ptr(), pixel.data_ptr(), offsets.data_ptr())  # no image: offsets[0] = 0 and the filler
        h.synchronize()
        assert offsets.cpu().tolist() == [0] and not points.cpu().numpy().any() and pixel.cpu().tolist() == [-1] * 4
        assert sc.device_call(h) == fresh["scene"]
        assert sc.device_call(h, stride=136) == fresh["scene"]  # what mdrp_copy_results_device writes: the model at the front of 136 bytes
        assert sc.device_call(h, with_transforms=False)[:3] == fresh["scene"][:3]  # the records in the handle's scratch
    finally:
        h.close()


def test_python_refusals(torch, poselib):
    dm = torch.ones((3, 4, 4), device="cuda")
    ms = sc.rc.models("shared_focal", 2)
    pairs, tree = poselib.video_tree(3)
    for kw in (dict(rate=0.0), dict(rate=float("nan")), dict(keep="both_inf"), dict(p_max=-1), dict(seed=-1),
               dict(cameras={"model": "SIMPLE_PINHOLE", "params": [1.0, 0.0, 0.0]}), dict(sizes=[[4, 4]])):
        with pytest.raises(ValueError):
            poselib.reconstruct_scene_torch("shared_focal", ms, dm, pairs, tree, **kw)
    with pytest.raises(ValueError):
        poselib.reconstruct_scene_torch("shared_focal", ms[:1], dm, pairs, tree)  # one model for two pairs
    with pytest.raises(ValueError):
        poselib.reconstruct_scene_torch("shared_focal", ms, dm, pairs, tree[:2])  # a tree row per image
    with pytest.raises(ValueError):
        poselib.reconstruct_scene_torch("shared_focal", ms, dm, pairs.astype(np.float64), tree)
    with pytest.raises(ValueError):
        poselib.reconstruct_scene_torch("shared_focal", ms, dm.cpu(), pairs, tree)
    with pytest.raises(ValueError):
        poselib.scene_transforms_torch("shared_focal", ms, pairs, tree, 4)
    side = torch.cuda.Stream()  # a stream no estimate ran on: its handle is fresh
    with torch.cuda.stream(side):
        with pytest.raises(ValueError, match="last"):
            poselib.reconstruct_scene_torch("shared_focal", "last", dm, pairs, tree)
