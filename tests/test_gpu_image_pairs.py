"""The front end on per-image tables on a real MI355X: poselib.gather_image_pairs_torch / estimate_image_pairs_torch against the NumPy statement
of the same definition (mdrp_amd/frontend.py gather_image_pairs_numpy) followed by the estimator the project already has.

The batch is tests/image_pairs_cases.py: five images of different valid sizes in 48 x 72 allocations, K = 700 keypoints of which two images
hold fewer, ten pairs that repeat images and pairs and hold two indices outside the set, row counts on the wavefront and tile boundaries of
the ordered compaction.  Everything is compared bitwise: the front end only moves and widens numbers, and the estimate is the same estimator
run twice on identical buffers."""
import numpy as np
import pytest

import image_pairs_cases as cases

pytestmark = pytest.mark.gpu

GOOD = [b for b in range(len(cases.PAIRS)) if b not in cases.BAD]
DBL_MAX = np.finfo(np.float64).max


def to_device(kp_dtype=np.float32, depth_dtype=np.float32, match_dtype=np.int64, pairs=None):
    """(keypoints, depth_maps, host pairs, matches) of the batch, the tables and the matches on the device"""
    import torch
    t = cases.batch()
    dev = torch.device("cuda", 0)
    sel = slice(None) if pairs is None else list(pairs)
    return (torch.from_numpy(t["keypoints"].astype(kp_dtype)).to(dev), torch.from_numpy(t["depth_maps"].astype(depth_dtype)).to(dev),
            t["pairs"][sel].copy(), torch.from_numpy(t["matches"][sel].astype(match_dtype)).to(dev))


def assert_gather_equal(got, ref, what):
    x1, x2, d1, d2, n, slot = got
    for name, mine, want in (("x1", x1, ref[0]), ("x2", x2, ref[1]), ("d1", d1, ref[2]), ("d2", d2, ref[3]), ("slot", slot, ref[5])):
        mine = mine.cpu().numpy()
        assert mine.dtype == want.dtype and mine.shape == want.shape, (what, name)
        assert mine.tobytes() == want.tobytes(), (what, name, np.flatnonzero((mine != want).reshape(len(mine), -1).any(axis=1)))
    assert isinstance(n, np.ndarray) and n.dtype == np.int32 and np.array_equal(n, ref[4]), (what, n, ref[4])


@pytest.mark.parametrize("kp_dtype,depth_dtype", [(np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64)])
def test_gather_equals_numpy_bitwise(kp_dtype, depth_dtype):
    import torch
    import mdrp_amd.poselib as poselib
    t = cases.batch()
    for match_dtype in (np.int32, np.int64):
        kp, dm, pairs, matches = to_device(kp_dtype, depth_dtype, match_dtype)
        sizes, counts = torch.tensor(t["sizes"]).to(kp.device), t["kp_counts"]  # a device tensor and a host array
        for filter in ("both_inf", "finite"):
            for centres in (False, True):
                got = poselib.gather_image_pairs_torch(kp, dm, pairs, matches, centers=t["centers"] if centres else None, sizes=sizes, kp_counts=counts,
                                                       filter=filter)
                ref = cases.twin(kp_dtype, depth_dtype, filter, centres)
                assert_gather_equal(got, ref, (match_dtype.__name__, filter, centres))
                x1, x2, d1, d2, n, slot = (v if isinstance(v, np.ndarray) else v.cpu().numpy() for v in got)
                for b in cases.BAD:  # an image index outside the set: no row, all slots -1, pure filler
                    assert n[b] == 0 and (slot[b] == -1).all() and not x1[b].any() and not x2[b].any() and (d1[b] == 1.0).all() and (d2[b] == 1.0).all()
                assert n[GOOD].min() >= 1 and n.sum() > 800


def test_pairs_as_list_array_and_tensors_give_the_same_bytes():
    import torch
    import mdrp_amd.poselib as poselib
    t = cases.batch()
    kp, dm, pairs, matches = to_device()
    ref = cases.twin(centres=True)
    forms = (pairs.tolist(), pairs.astype(np.int64), torch.from_numpy(pairs), torch.from_numpy(pairs).to(kp.device), torch.from_numpy(pairs.astype(np.int64)).to(kp.device))
    for k, form in enumerate(forms):
        got = poselib.gather_image_pairs_torch(kp, dm, form, matches, centers=torch.tensor(t["centers"]).to(kp.device), sizes=t["sizes"].tolist(),
                                               kp_counts=torch.tensor(t["kp_counts"]))
        assert_gather_equal(got, ref, k)
    one = poselib.gather_image_pairs_torch(kp, dm, pairs, matches, centers=t["centers"][3], sizes=t["sizes"], kp_counts=t["kp_counts"])  # one centre for all
    from mdrp_amd import frontend
    want = frontend.gather_image_pairs_numpy(t["keypoints"].astype(np.float32), t["depth_maps"].astype(np.float32), pairs, t["matches"], centers=t["centers"][3],
                                             sizes=t["sizes"], kp_counts=t["kp_counts"])
    assert_gather_equal(one, want, "one centre")


def test_without_extents_equals_gather_matches_on_the_expanded_tables():
    """sizes and kp_counts omitted, the two bad pairs removed: the per-pair front end on keypoints[pairs[:, 0]], ... gives the same bytes"""
    import torch
    import mdrp_amd.poselib as poselib
    t = cases.batch()
    kp, dm, pairs, matches = to_device(pairs=GOOD)
    centers = torch.tensor(t["centers"]).to(kp.device)
    a, c = (torch.from_numpy(pairs[:, k].astype(np.int64)).to(kp.device) for k in (0, 1))
    for filter in ("both_inf", "finite"):
        for centres in (False, True):
            got = poselib.gather_image_pairs_torch(kp, dm, pairs, matches, centers=centers if centres else None, filter=filter)
            want = poselib.gather_matches_torch(kp[a], kp[c], matches, dm[a], dm[c], center1=centers[a] if centres else None,
                                                center2=centers[c] if centres else None, filter=filter)
            for name, mine, ref in zip(("x1", "x2", "d1", "d2", "n", "slot"), got, want):
                mine, ref = (v if isinstance(v, np.ndarray) else v.cpu().numpy() for v in (mine, ref))
                assert mine.dtype == ref.dtype and mine.tobytes() == ref.tobytes(), (filter, centres, name)
            assert_gather_equal(got, cases.twin(filter=filter, centres=centres, extents=False, pairs=GOOD), (filter, centres))


def _pair_cameras():
    import mdrp_amd.poselib as poselib
    rec = poselib._camera_records(cases.CAMERAS, cases.I)
    idx = np.where((cases.PAIRS >= 0) & (cases.PAIRS < cases.I), cases.PAIRS, 0)
    return rec, rec[idx[:, 0]].copy(), rec[idx[:, 1]].copy()


_reference = {}


def reference(kind):
    """estimate_batch_torch on the NumPy-gathered buffers with their n_per_pair and the per-pair cameras: (records, mask, twin), computed once"""
    import torch
    import mdrp_amd.poselib as poselib
    if kind not in _reference:
        focal = kind != "calibrated"
        ref = cases.twin(centres=focal)
        dev = torch.device("cuda", 0)
        x1, x2, d1, d2 = (torch.tensor(a, device=dev) for a in ref[:4])
        _, cams1, cams2 = _pair_cameras()
        res, mask = poselib.estimate_batch_torch(kind, x1, x2, d1, d2, None if focal else cams1, None if focal else cams2, cases.RO, cases.BO, n_per_pair=ref[4])
        _reference[kind] = (res, mask.cpu().numpy(), ref)
    return _reference[kind]


def estimate(kind, tensors=None, cameras=None, **kw):
    import mdrp_amd.poselib as poselib
    t = cases.batch()
    focal = kind != "calibrated"
    kp, dm, pairs, matches = to_device() if tensors is None else tensors
    return poselib.estimate_image_pairs_torch(kind, kp, dm, pairs, matches, None if focal else (cases.CAMERAS if cameras is None else cameras), cases.RO, cases.BO,
                                              centers=t["centers"] if focal else None, sizes=t["sizes"], kp_counts=t["kp_counts"], **kw)


def assert_estimates_equal(got, want, what):
    (res, match_mask, n_used), (res_ref, mask_ref, ref) = got, want
    n, slot = ref[4], ref[5]
    assert isinstance(n_used, np.ndarray) and n_used.dtype == np.int32 and np.array_equal(n_used, n), what
    assert res.dtype == res_ref.dtype and res.tobytes() == res_ref.tobytes(), (what, [k for k in range(len(res)) if res[k].tobytes() != res_ref[k].tobytes()])
    expect = np.zeros(slot.shape, dtype=np.uint8)
    for b in range(len(n)):
        kept = slot[b] >= 0
        expect[b, kept] = mask_ref[b, slot[b, kept]]
    mm = match_mask.cpu().numpy()
    assert mm.dtype == np.uint8 and np.array_equal(mm, expect), what
    assert [int(mm[b].sum()) for b in range(len(n))] == [int(mask_ref[b, :n[b]].sum()) for b in range(len(n))], what


@pytest.mark.parametrize("kind", ["calibrated", "shared_focal", "varying_focal"])
def test_estimate_from_image_pairs_equals_estimate_on_gathered_input(kind):
    got, want = estimate(kind), reference(kind)
    assert_estimates_equal(got, want, kind)
    res, n = got[0], got[2]
    assert (res["iterations"][n >= 3] == 200).all() and int(res["num_inliers"].max()) >= 20
    for b in cases.BAD:  # what an n = 0 pair returns: zeroed stats, model_score = DBL_MAX, the identity model, no inlier
        r = res[b]
        assert n[b] == 0 and (int(r["iterations"]), int(r["refinements"]), int(r["num_inliers"]), float(r["inlier_ratio"])) == (0, 0, 0, 0.0)
        assert float(r["model_score"]) == DBL_MAX and r["model"]["q"].tolist() == [1.0, 0.0, 0.0, 0.0] and not r["model"]["t"].any()
        assert not got[1][b].any().item()


def test_camera_forms_give_the_same_records():
    """per-image cameras as a list of I and as a record array of I, and one camera for all images as a dict, as I copies and as I records"""
    rec, _, _ = _pair_cameras()
    as_list = estimate("calibrated")
    assert_estimates_equal(as_list, reference("calibrated"), "list")
    as_records = estimate("calibrated", cameras=rec)
    assert as_records[0].tobytes() == as_list[0].tobytes() and np.array_equal(as_records[1].cpu().numpy(), as_list[1].cpu().numpy())
    one = estimate("calibrated", cameras=cases.CAMERAS[2])
    assert one[0].tobytes() != as_list[0].tobytes()  # another camera for four of the images
    for same in ([cases.CAMERAS[2]] * cases.I, np.repeat(rec[2:3], cases.I)):
        got = estimate("calibrated", cameras=same)
        assert got[0].tobytes() == one[0].tobytes() and np.array_equal(got[1].cpu().numpy(), one[1].cpu().numpy())
    with pytest.raises(ValueError):
        estimate("calibrated", cameras=cases.CAMERAS[:3])


def test_inputs_produced_on_the_current_stream_just_before_the_call():
    """the inputs are written by asynchronous torch kernels queued on a non-default current stream behind a long chain of work: the call must be
    ordered after them (it runs on that stream, and uploads its pairs there), so the result equals the synchronous one"""
    import torch
    want = reference("calibrated")
    sync = estimate("calibrated")
    assert_estimates_equal(sync, want, "synchronous")
    dev = torch.device("cuda", 0)
    kp, dm, pairs, matches = to_device()
    big = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        assert torch.cuda.current_stream(dev).cuda_stream == stream.cuda_stream != 0
        late = [torch.full_like(v, -1) if v.dtype == torch.int64 else torch.full_like(v, float("nan")) for v in (kp, dm, matches)]  # the inputs do not exist yet
        junk = big
        for _ in range(40):
            junk = junk @ big
            junk = junk / junk.abs().max()
        bump = junk[0, 0] * 0.0  # data dependence on the long chain
        for v, o in zip((kp, dm, matches), late):
            torch.add(v, bump.to(v.dtype), out=o)  # asynchronous producers of the real inputs
        got = estimate("calibrated", tensors=(late[0], late[1], pairs, late[2]))
        after = got[1].sum(dim=1)  # a consumer on the same stream, no explicit synchronisation
        assert_estimates_equal(got, want, "stream")
        assert got[0].tobytes() == sync[0].tobytes()
        assert np.array_equal(after.cpu().numpy(), sync[1].sum(dim=1).cpu().numpy())
    torch.cuda.synchronize()


def test_refusals_leave_the_handle_usable():
    import torch
    import mdrp_amd.poselib as poselib
    from mdrp_amd import _capi
    t = cases.batch()
    tensors = to_device()
    kp, dm, pairs, matches = tensors
    for kind in (_capi.RELPOSE_5PT, _capi.SHARED_6PT, _capi.FUNDAMENTAL_7PT, -1, "fundamental"):
        with pytest.raises(ValueError):
            poselib.estimate_image_pairs_torch(kind, kp, dm, pairs, matches, cases.CAMERAS, cases.RO, cases.BO)
    for bad in ((kp.half(), dm, pairs, matches), (kp, dm.half(), pairs, matches), (kp, dm, pairs, matches.cpu()), (kp, dm, pairs, matches.to(torch.int16)),
                (kp, dm[:3], pairs, matches), (kp, dm, pairs[:4], matches), (kp, dm, pairs.astype(np.float64), matches), (kp, dm, pairs, matches[..., 0])):
        with pytest.raises(ValueError):
            poselib.estimate_image_pairs_torch("calibrated", *bad, cases.CAMERAS, cases.RO, cases.BO)
        with pytest.raises(ValueError):
            poselib.gather_image_pairs_torch(*bad)
    for kw in ({"filter": "nonsense"}, {"sizes": t["sizes"][:3]}, {"kp_counts": t["kp_counts"][:4]}, {"centers": t["centers"][:2]}):
        with pytest.raises(ValueError):
            poselib.gather_image_pairs_torch(kp, dm, pairs, matches, **kw)
        with pytest.raises(ValueError):
            poselib.estimate_image_pairs_torch("calibrated", kp, dm, pairs, matches, cases.CAMERAS, cases.RO, cases.BO, **kw)
    # the C ABI's own refusals, below the Python checks: another kind and a bad descriptor are MDRP_ERR_INVALID (1)
    h = poselib._torch_handle(0, int(torch.cuda.current_stream(kp.device).cuda_stream))
    ip, keep, host_pairs, B, M, I, _ = poselib._image_pairs_descriptor(kp, dm, pairs, matches, None, t["sizes"], t["kp_counts"], "both_inf", True)
    ro, bo = _capi.ransac_opt_from_dict(cases.RO), _capi.bundle_opt_from_dict(cases.BO)
    cams1, cams2 = poselib._pair_cameras(cases.CAMERAS, host_pairs, I)
    for kind in (3, 4, 5, -1):
        with pytest.raises(_capi.MdrpError, match="mdrp error 1"):
            h.estimate_image_pairs_device(kind, ip, B, ro, bo, cams1, cams2)
    for field, value in (("kp_type", 2), ("depth_type", -1), ("filter", 2), ("m_max", -1), ("k_max", -1), ("h_max", -1), ("w_max", -1), ("n_images", -1),
                         ("pairs", None), ("matches", None), ("kp", None), ("depth", None)):
        was = getattr(ip, field)
        setattr(ip, field, value)
        with pytest.raises(_capi.MdrpError, match="mdrp error 1"):
            h.estimate_image_pairs_device(_capi.CALIB, ip, B, ro, bo, cams1, cams2)
        with pytest.raises(_capi.MdrpError, match="mdrp error 1"):
            h.gather_image_pairs(ip, B, 0, 0, 0, 0, 0)
        setattr(ip, field, was)
    with pytest.raises(NotImplementedError):  # the option refusals are the estimator's own
        poselib.estimate_image_pairs_torch("calibrated", *tensors, cases.CAMERAS, dict(cases.RO, progressive_sampling=True), cases.BO, sizes=t["sizes"],
                                           kp_counts=t["kp_counts"])
    del keep
    assert_estimates_equal(estimate("calibrated", tensors=tensors), reference("calibrated"), "after the refusals")


def test_no_images_and_no_pairs():
    """I = 0: every pair is a bad pair and the cameras are zero records; B = 0: empty results"""
    import torch
    import mdrp_amd.poselib as poselib
    dev = torch.device("cuda", 0)
    kp, dm = torch.zeros((0, 4, 2), device=dev), torch.zeros((0, 3, 5), device=dev)
    matches = torch.zeros((2, 5, 2), dtype=torch.int64, device=dev)
    res, mask, n = poselib.estimate_image_pairs_torch("calibrated", kp, dm, [(0, 0), (1, -1)], matches, [], cases.RO, cases.BO)
    assert n.tolist() == [0, 0] and not mask.any().item() and res["iterations"].tolist() == [0, 0] and (res["model_score"] == DBL_MAX).all()
    kp, dm, _, matches = to_device()
    out = poselib.gather_image_pairs_torch(kp, dm, [], matches[:0])
    assert out[0].shape == (0, cases.M, 2) and out[4].shape == (0,) and out[5].shape == (0, cases.M)
    res, mask, n = poselib.estimate_image_pairs_torch("shared_focal", kp, dm, np.zeros((0, 2), dtype=np.int32), matches[:0], None, cases.RO, cases.BO)
    assert len(res) == 0 and mask.shape == (0, cases.M) and len(n) == 0
