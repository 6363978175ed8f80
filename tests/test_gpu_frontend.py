"""The device front end on a real MI355X: poselib.gather_matches_torch / estimate_matches_torch against the NumPy statement of the same
definition (mdrp_amd/frontend.py) followed by the estimator the project already has.

Inputs: synth.make_pair correspondences, scaled into a 48 x 64 map for image 1 and a 40 x 72 map for image 2 (non-square, different sizes:
a swapped x / y or a wrong stride fails), scattered into keypoint tables through random permutations (i != j != m), their depths painted
into the maps.  Row counts sit on the wavefront and tile boundaries of the ordered compaction.  Everything is compared bitwise: the front
end only moves and widens numbers, and the estimate is the same estimator run twice on identical buffers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H1, W1, H2, W2 = 48, 64, 40, 72
A1, C1 = 0.035, (32.0, 24.0)   # pixel = A * synth pixel + C: a camera with focal A * 800 and principal point C
A2, C2 = 0.03, (36.0, 20.0)
ROW_COUNTS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 600)
RO = {"max_iterations": 200, "min_iterations": 200, "max_epipolar_error": 0.1, "max_reproj_error": 0.8}
BO = {"loss_type": "TRUNCATED_CAUCHY"}
CAM1 = {"model": "SIMPLE_PINHOLE", "width": W1, "height": H1, "params": [A1 * 800.0, *C1]}
CAM2 = {"model": "SIMPLE_PINHOLE", "width": W2, "height": H2, "params": [A2 * 800.0, *C2]}
DBL_MAX = np.finfo(np.float64).max


def _inside(p, w, h):
    return (p[:, 0] >= 0) & (p[:, 0] < w - 1) & (p[:, 1] >= 0) & (p[:, 1] < h - 1)


def make_pair_inputs(seed, rows, special=None):
    """one pair in float64: keypoint tables, (rows, 2) int64 matches, the two depth maps.  special: None (planted cases where rows >= 64) |
    "none_kept" | 2 | 3 (exactly that many rows survive)"""
    from mdrp_amd import synth
    rng = np.random.default_rng(9000 + seed)
    p = synth.make_pair(7000 + seed, rows, noise_px=0.5, depth_noise=0.02, outlier_frac=0.2)
    pt1 = A1 * p["x1"] + np.array(C1)
    pt2 = A2 * p["x2"] + np.array(C2)
    K1, K2 = rows + 5, rows + 9
    perm1, perm2 = rng.permutation(K1), rng.permutation(K2)
    kp1 = np.stack([rng.uniform(0, W1 - 1, K1), rng.uniform(0, H1 - 1, K1)], 1)
    kp2 = np.stack([rng.uniform(0, W2 - 1, K2), rng.uniform(0, H2 - 1, K2)], 1)
    kp1[perm1[:rows]] = pt1
    kp2[perm2[:rows]] = pt2
    matches = np.stack([perm1[:rows], perm2[:rows]], 1).astype(np.int64)
    dm1 = rng.uniform(1.0, 6.0, (H1, W1))
    dm2 = rng.uniform(1.0, 6.0, (H2, W2))
    in1, in2 = _inside(pt1, W1, H1), _inside(pt2, W2, H2)
    for m in range(rows):  # paint (a later keypoint on the same pixel wins: the earlier one becomes an outlier)
        if in1[m]:
            dm1[int(pt1[m, 1]), int(pt1[m, 0])] = p["d1"][m]
        if in2[m]:
            dm2[int(pt2[m, 1]), int(pt2[m, 0])] = p["d2"][m]
    both = np.flatnonzero(in1 & in2)
    if special == "none_kept":
        dm1[:] = np.inf
        dm2[:] = -np.inf
        matches[rng.choice(rows, rows // 4, replace=False)] = -1
    elif special in (2, 3):
        keep = rng.choice(both, special, replace=False)
        gone = np.setdiff1d(np.arange(rows), keep)
        matches[gone[::2]] = -1
        matches[gone[1::2], 0] = -1
    elif rows >= 64:
        def px(dm, pt, m):
            return (int(pt[m, 1]), int(pt[m, 0]))
        planted, seen1, seen2 = [], set(), set()
        for m in rng.permutation(both):  # 24 rows inside both maps, no two on one pixel: a planted depth is not overwritten by the next
            if px(dm1, pt1, m) not in seen1 and px(dm2, pt2, m) not in seen2 and len(planted) < 24:
                planted.append(m); seen1.add(px(dm1, pt1, m)); seen2.add(px(dm2, pt2, m))
        assert len(planted) == 24
        r = iter(planted)
        m = next(r); dm1[px(dm1, pt1, m)] = np.inf; dm2[px(dm2, pt2, m)] = np.inf          # both infinite: dropped
        m = next(r); dm1[px(dm1, pt1, m)] = -np.inf; dm2[px(dm2, pt2, m)] = np.inf
        m = next(r); dm1[px(dm1, pt1, m)] = np.inf                                           # one-sided: kept by "both_inf", dropped by "finite"
        m = next(r); dm2[px(dm2, pt2, m)] = -np.inf
        m = next(r); dm1[px(dm1, pt1, m)] = np.nan                                           # NaN depth: likewise
        m = next(r); dm2[px(dm2, pt2, m)] = np.nan
        m = next(r); dm1[px(dm1, pt1, m)] = np.nan; dm2[px(dm2, pt2, m)] = np.inf
        for x in (-0.5, -1.0, W1 - 0.001, float(W1), np.nan, np.inf):                         # coordinates at the edges of image 1 (x) ...
            kp1[matches[next(r), 0], 0] = x
        for y in (-0.5, -1.0, H2 - 0.001, float(H2), np.nan, -np.inf):                        # ... and of image 2 (y)
            kp2[matches[next(r), 1], 1] = y
        matches[next(r), 0] = K1                                                              # index == K
        matches[next(r), 1] = K2
        matches[next(r), 1] = -1                                                              # one-sided -1
        matches[next(r), 0] = -7
        matches[rng.choice(np.setdiff1d(np.arange(rows), planted), 3, replace=False)] = -1    # padding rows in mid-list
    return kp1, kp2, matches, dm1, dm2


def make_batch_inputs(specs, first_seed):
    """pairs of different row counts stacked: matches padded to a common M with -1 rows, keypoint tables to a common K with unused entries"""
    pairs = [make_pair_inputs(first_seed + k, rows, special) for k, (rows, special) in enumerate(specs)]
    M = max(len(q[2]) for q in pairs) + 7
    K1, K2 = max(len(q[0]) for q in pairs), max(len(q[1]) for q in pairs)
    B = len(pairs)
    kp1 = np.full((B, K1, 2), 5.0); kp2 = np.full((B, K2, 2), 5.0)
    matches = np.full((B, M, 2), -1, dtype=np.int64)
    for b, q in enumerate(pairs):
        kp1[b, :len(q[0])] = q[0]; kp2[b, :len(q[1])] = q[1]; matches[b, :len(q[2])] = q[2]
    return {"kp1": kp1, "kp2": kp2, "matches": matches, "dm1": np.stack([q[3] for q in pairs]), "dm2": np.stack([q[4] for q in pairs]),
            "c1": np.tile(np.array(C1), (B, 1)) + np.arange(B)[:, None] * 0.125, "c2": np.tile(np.array(C2), (B, 1)), "specs": specs}


@pytest.fixture(scope="module")
def batches():
    a = make_batch_inputs([(1, None), (2, None), (3, None), (63, None), (64, None), (65, None), (600, None)], 0)
    b = make_batch_inputs([(255, None), (256, None), (257, None), (64, "none_kept"), (70, 2), (100, 3), (64, None)], 20)
    return a, b


_twin_cache = {}


def twin(batch, kp_dtype, depth_dtype, filter, centres):
    """the NumPy front end on the batch as the device sees it (tables cast to their dtypes): padded buffers of frontend.pad_pairs, computed once"""
    from mdrp_amd import frontend
    key = (id(batch), np.dtype(kp_dtype).name, np.dtype(depth_dtype).name, filter, centres)
    if key not in _twin_cache:
        kp1, kp2 = batch["kp1"].astype(kp_dtype), batch["kp2"].astype(kp_dtype)
        dm1, dm2 = batch["dm1"].astype(depth_dtype), batch["dm2"].astype(depth_dtype)
        B, M = batch["matches"].shape[:2]
        g = [frontend.gather_matches_numpy(kp1[b], kp2[b], batch["matches"][b], dm1[b], dm2[b], batch["c1"][b] if centres else None,
                                           batch["c2"][b] if centres else None, filter) for b in range(B)]
        out = frontend.pad_pairs(g, M)
        for a in out:
            a.setflags(write=False)
        _twin_cache[key] = out
    return _twin_cache[key]


def to_device(batch, kp_dtype, depth_dtype, match_dtype):
    import torch
    dev = torch.device("cuda", 0)
    return (torch.from_numpy(batch["kp1"].astype(kp_dtype)).to(dev), torch.from_numpy(batch["kp2"].astype(kp_dtype)).to(dev),
            torch.from_numpy(batch["matches"].astype(match_dtype)).to(dev),
            torch.from_numpy(batch["dm1"].astype(depth_dtype)).to(dev), torch.from_numpy(batch["dm2"].astype(depth_dtype)).to(dev))


def assert_gather_equal(got, ref, what):
    x1, x2, d1, d2, n, slot = got
    for name, mine, want in (("x1", x1, ref[0]), ("x2", x2, ref[1]), ("d1", d1, ref[2]), ("d2", d2, ref[3]), ("slot", slot, ref[5])):
        mine = mine.cpu().numpy()
        assert mine.dtype == want.dtype and mine.shape == want.shape, (what, name)
        assert mine.tobytes() == want.tobytes(), (what, name, np.flatnonzero((mine != want).reshape(len(mine), -1).any(axis=1)))
    assert isinstance(n, np.ndarray) and n.dtype == np.int32 and np.array_equal(n, ref[4]), (what, n, ref[4])


def test_the_inputs_hold_the_planted_cases(batches):
    a, b = batches
    for batch in (a, b):
        both, fin = twin(batch, np.float32, np.float32, "both_inf", False), twin(batch, np.float32, np.float32, "finite", False)
        for k, (rows, special) in enumerate(batch["specs"]):
            if special is None and rows >= 64:
                assert 3 <= fin[4][k] <= both[4][k] - 3 and both[4][k] < rows - 10, (rows, both[4][k], fin[4][k])  # one-sided inf / NaN rows differ
                d1, d2 = both[2][k, :both[4][k]], both[3][k, :both[4][k]]
                assert np.isnan(d1).any() and np.isnan(d2).any() and (np.isinf(d1) ^ np.isinf(d2)).any()
                assert (both[0][k, :both[4][k], 0] == -0.5).any() and (both[0][k, :both[4][k], 0] == np.float32(W1 - 0.001)).any()
                assert not np.isin(both[0][k, :, 0], [-1.0, float(W1)]).any()
    assert [int(v) for v in twin(b, np.float32, np.float32, "both_inf", False)[4][3:6]] == [0, 2, 3]
    assert [int(v) for v in twin(b, np.float64, np.float64, "finite", True)[4][3:6]] == [0, 2, 3]


@pytest.mark.parametrize("kp_dtype,depth_dtype", [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)])
def test_gather_equals_numpy_bitwise(batches, kp_dtype, depth_dtype):
    import torch
    import mdrp_amd.poselib as poselib
    for which, batch in enumerate(batches):
        for match_dtype in (np.int32, np.int64):
            t = to_device(batch, kp_dtype, depth_dtype, match_dtype)
            for filter in ("both_inf", "finite"):
                for centres in (False, True):
                    c = (torch.from_numpy(batch["c1"]).to(t[0].device), batch["c2"]) if centres else (None, None)  # a device tensor and a host array
                    got = poselib.gather_matches_torch(*t, center1=c[0], center2=c[1], filter=filter)
                    assert_gather_equal(got, twin(batch, kp_dtype, depth_dtype, filter, centres), (which, match_dtype.__name__, filter, centres))


@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_gather_at_every_row_count_without_padding(rows):
    """M itself on the boundaries: no padded tail behind the last row, one pair as a (K, 2) / (M, 2) / (H, W) call (B = 1), two as a batch"""
    import torch
    import mdrp_amd.poselib as poselib
    from mdrp_amd import frontend
    dev = torch.device("cuda", 0)
    pairs = [make_pair_inputs(40 + rows + k, rows) for k in range(2)]
    ref = [frontend.gather_matches_numpy(q[0].astype(np.float32), q[1].astype(np.float32), q[2], q[3].astype(np.float32), q[4].astype(np.float32)) for q in pairs]
    stacked = [torch.from_numpy(np.stack([q[k] for q in pairs]).astype(np.int64 if k == 2 else np.float32)).to(dev) for k in range(5)]
    assert stacked[2].shape == (2, rows, 2)
    assert_gather_equal(poselib.gather_matches_torch(*stacked), frontend.pad_pairs(ref, rows), rows)
    single = [t[1] for t in stacked]
    assert_gather_equal(poselib.gather_matches_torch(*single), frontend.pad_pairs(ref[1:], rows), rows)


def _estimate_both_ways(kind, batch, filter, t=None):
    """(front-end route, NumPy front end + estimate_batch_torch) on float32 tables and int64 matches, the shape a matcher leaves behind"""
    import torch
    import mdrp_amd.poselib as poselib
    focal = kind != "calibrated"
    cams = (None, None) if focal else (CAM1, CAM2)
    ref = twin(batch, np.float32, np.float32, filter, focal)
    dev = torch.device("cuda", 0)
    x1, x2, d1, d2 = (torch.tensor(a, device=dev) for a in ref[:4])
    res_ref, mask_ref = poselib.estimate_batch_torch(kind, x1, x2, d1, d2, *cams, RO, BO, n_per_pair=ref[4])
    if t is None:
        t = to_device(batch, np.float32, np.float32, np.int64)
    res, match_mask, n_used = poselib.estimate_matches_torch(kind, *t, *cams, RO, BO, center1=batch["c1"] if focal else None,
                                                             center2=batch["c2"] if focal else None, filter=filter)
    return (res, match_mask, n_used), (res_ref, mask_ref.cpu().numpy(), ref)


def _assert_estimates_equal(got, want, what):
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
def test_estimate_from_matches_equals_estimate_on_gathered_input(batches, kind):
    for which, batch in enumerate(batches):
        got, want = _estimate_both_ways(kind, batch, "both_inf")
        _assert_estimates_equal(got, want, (kind, which))
        res, n = got[0], got[2]
        assert (res["iterations"][n >= 3] == 200).all() and int(res["num_inliers"].max()) >= 20
        for b in np.flatnonzero(n < 3):  # "fewer than 3 correspondences": zeroed stats, model_score = DBL_MAX, the identity model
            r = res[b]
            assert (int(r["iterations"]), int(r["refinements"]), int(r["num_inliers"]), float(r["inlier_ratio"])) == (0, 0, 0, 0.0)
            assert float(r["model_score"]) == DBL_MAX and r["model"]["q"].tolist() == [1.0, 0.0, 0.0, 0.0] and not r["model"]["t"].any()
    assert [int(v) for v in got[2][3:6]] == [0, 2, 3] and int(got[0][3]["iterations"]) == 0 and int(got[0][4]["iterations"]) == 0


def test_estimate_from_matches_with_the_finite_filter(batches):
    got, want = _estimate_both_ways("calibrated", batches[0], "finite")
    _assert_estimates_equal(got, want, "finite")
    assert np.isfinite(want[2][2]).all() and np.isfinite(want[2][3]).all()


def test_inputs_produced_on_the_current_stream_just_before_the_call(batches):
    """the inputs are written by asynchronous torch kernels queued on a non-default current stream behind ~100 ms of work: the call must be
    ordered after them (it runs on that stream), so the result equals the synchronous one"""
    import torch
    batch = batches[1]
    want_sync, want_ref = _estimate_both_ways("calibrated", batch, "both_inf")
    _assert_estimates_equal(want_sync, want_ref, "synchronous")
    dev = torch.device("cuda", 0)
    src = to_device(batch, np.float32, np.float32, np.int64)
    big = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        assert torch.cuda.current_stream(dev).cuda_stream == stream.cuda_stream != 0
        t = [torch.full_like(v, -1) if v.dtype == torch.int64 else torch.full_like(v, float("nan")) for v in src]  # the inputs do not exist yet
        junk = big
        for _ in range(40):
            junk = junk @ big
            junk = junk / junk.abs().max()
        bump = junk[0, 0] * 0.0  # data dependence on the long chain
        for v, o in zip(src, t):
            torch.add(v, bump.to(v.dtype), out=o)  # asynchronous producers of the real inputs
        got, _ = _estimate_both_ways("calibrated", batch, "both_inf", t)
        after = got[1].sum(dim=1)  # a consumer on the same stream, no explicit synchronisation
        _assert_estimates_equal(got, want_ref, "stream")
        assert got[0].tobytes() == want_sync[0].tobytes()
        assert np.array_equal(after.cpu().numpy(), want_sync[1].sum(dim=1).cpu().numpy())
    torch.cuda.synchronize()


def test_refusals_leave_the_handle_usable(batches):
    import torch
    import mdrp_amd.poselib as poselib
    from mdrp_amd import _capi
    batch = batches[0]
    t = to_device(batch, np.float32, np.float32, np.int64)
    for kind in (_capi.RELPOSE_5PT, _capi.SHARED_6PT, _capi.FUNDAMENTAL_7PT, "fundamental"):
        with pytest.raises((ValueError, _capi.MdrpError)):
            poselib.estimate_matches_torch(kind, *t, CAM1, CAM2, RO, BO)
    half = (t[0].half(), t[1].half(), t[2], t[3], t[4])
    cpu = (t[0], t[1], t[2].cpu(), t[3], t[4])
    for bad in (half, cpu, (t[0], t[1], t[2], t[3].half(), t[4].half()), (t[0], t[1], t[2].to(torch.int16), t[3], t[4]),
                (t[0], t[1][:3], t[2], t[3], t[4]), (t[0], t[1], t[2][..., 0], t[3], t[4])):
        with pytest.raises(ValueError):
            poselib.estimate_matches_torch("calibrated", *bad, CAM1, CAM2, RO, BO)
        with pytest.raises(ValueError):
            poselib.gather_matches_torch(*bad)
    with pytest.raises(ValueError):
        poselib.gather_matches_torch(*t, filter="nonsense")
    # the C ABI's own refusals, below the Python checks: kind 3..5 and a bad descriptor are MDRP_ERR_INVALID (1)
    h = poselib._torch_handle(0, int(torch.cuda.current_stream(t[0].device).cuda_stream))
    mm, keep, B, M, _ = poselib._matches_descriptor(*t, None, None, "both_inf")
    ro, bo = _capi.ransac_opt_from_dict(RO), _capi.bundle_opt_from_dict(BO)
    cams = poselib._camera_records(CAM1, B)
    for kind in (3, 4, 5, -1):
        with pytest.raises(_capi.MdrpError, match="mdrp error 1"):
            h.estimate_matches_device(kind, mm, B, ro, bo, cams, cams)
    for field, value in (("kp_type", 2), ("depth_type", -1), ("filter", 2), ("m_max", -1), ("w1", -1)):
        was = getattr(mm, field)
        setattr(mm, field, value)
        with pytest.raises(_capi.MdrpError, match="mdrp error 1"):
            h.estimate_matches_device(_capi.CALIB, mm, B, ro, bo, cams, cams)
        setattr(mm, field, was)
    with pytest.raises(NotImplementedError):  # the option refusals are the estimator's own
        poselib.estimate_matches_torch("calibrated", *t, CAM1, CAM2, dict(RO, progressive_sampling=True), BO)
    got, want = _estimate_both_ways("calibrated", batch, "both_inf", t)
    _assert_estimates_equal(got, want, "after the refusals")
