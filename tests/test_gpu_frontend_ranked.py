"""The front end with match scores on a real MI355X: gather_matches_torch / estimate_matches_torch and the image-pairs forms with
scores= against the NumPy definition (mdrp_amd/frontend.py) and against the ranked estimator the project already has
(estimate_batch_torch(scores=)) on the unranked gather.

Inputs: the pairs of tests/test_gpu_frontend.py and tests/image_pairs_cases.py with the score patterns of tests/frontend_ranked_cases.py planted
across the pairs.  Everything is compared bitwise: the gather only moves and widens numbers, and both estimates run the same kernels on the same
ordered records."""
import numpy as np
import pytest

import frontend_ranked_cases as rc
import image_pairs_cases as ipc
import test_gpu_frontend as fe

pytestmark = pytest.mark.gpu

KEY_TILE = 2048  # RANK_TILE of mdrp_amd/csrc/mdrp_prosac.h: the key tile of k_gather_ranked's counting loop
ROW_COUNTS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 600, KEY_TILE - 1, KEY_TILE, KEY_TILE + 1)
KINDS = ("calibrated", "shared_focal", "varying_focal")
IP_PAIRS = [0, 2, 6, 7, 9, 5]  # of image_pairs_cases.PAIRS: (0, 1) twice, a == c, an image index outside the set, the 600-row pair, (4, 0)
IP_GOOD = [0, 2, 6, 9, 5]


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype)).to(_dev())  # (a copy: the cases' arrays are read-only)


def _np(v):
    return v if isinstance(v, np.ndarray) else v.cpu().numpy()


def test_the_key_tile_is_the_kernels():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mdrp_amd", "csrc", "mdrp_prosac.h")).read()
    assert int(re.search(r"RANK_TILE = (\d+)", src).group(1)) == KEY_TILE


# ---- 1. the gather against the NumPy definition
@pytest.mark.parametrize("score_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kp_dtype,depth_dtype", [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)])
def test_gather_equals_numpy_definition_bitwise(kp_dtype, depth_dtype, score_dtype):
    import mdrp_amd.poselib as poselib
    kept_counts = set()
    for which, batch in enumerate(rc.batches()):
        t = fe.to_device(batch, kp_dtype, depth_dtype, np.int64 if which else np.int32)
        kept = rc.kept_rows(batch)
        for offset in (0, 2, 4):  # over the three offsets every pair of six meets "special", "dropped_high" or "levels" at least once
            scores = rc.batch_scores(kept, offset, which).astype(score_dtype)
            filter, centres = ("both_inf", "finite")[(offset // 2) % 2], offset == 2
            got = poselib.gather_matches_torch(*t, center1=batch["c1"] if centres else None, center2=batch["c2"] if centres else None, filter=filter,
                                               scores=_t(scores))
            ref = rc.ranked_twin(batch, scores, kp_dtype, depth_dtype, filter, centres)
            fe.assert_gather_equal(got, ref, (which, offset))
            kept_counts |= {int(v) for v in ref[4]}
    assert {0, 1, 2, 3} <= kept_counts


@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_gather_at_every_row_count_without_padding(rows):
    """M itself on the boundaries of the gather's tiles, of the four-records-per-thread pass and of the key tile: three pairs as a batch, one as a
    (K, 2) / (M, 2) / (H, W) / (M,) call"""
    import mdrp_amd.poselib as poselib
    score_dtype = np.float32 if rows % 2 else np.float64
    batch = rc.make_batch([(rows, None)] * 3, 300 + rows, pad=0)
    assert batch["matches"].shape == (3, rows, 2)
    kept = rc.kept_rows(batch)
    scores = rc.batch_scores(kept, rows % 7, rows).astype(score_dtype)
    if rows >= 64:
        scores[2] = rc.pair_scores("dropped_high", kept[2], rows).astype(score_dtype)
        scores[1] = rc.pair_scores("levels", kept[1], rows).astype(score_dtype)
    t = fe.to_device(batch, np.float32, np.float32, np.int64)
    ref = rc.ranked_twin(batch, scores, np.float32, np.float32, "both_inf", False)
    fe.assert_gather_equal(poselib.gather_matches_torch(*t, scores=_t(scores)), ref, rows)
    single = [v[1] for v in t]
    fe.assert_gather_equal(poselib.gather_matches_torch(*single, scores=_t(scores[1])), tuple(a[1:2] for a in ref), (rows, "single"))


@pytest.mark.parametrize("score_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kp_dtype,depth_dtype", [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)])
def test_image_pairs_gather_equals_numpy_definition_bitwise(kp_dtype, depth_dtype, score_dtype):
    import mdrp_amd.poselib as poselib
    from mdrp_amd import frontend
    t = ipc.batch()
    kp, dm = t["keypoints"].astype(kp_dtype), t["depth_maps"].astype(depth_dtype)
    pairs, matches = t["pairs"][IP_PAIRS], t["matches"][IP_PAIRS]
    kept = ipc.twin(np.float32, np.float32)[5][IP_PAIRS] >= 0
    for offset, filter, centres in ((1, "both_inf", True), (3, "finite", False)):
        scores = rc.batch_scores(kept, offset, 5).astype(score_dtype)
        kw = dict(centers=t["centers"] if centres else None, sizes=t["sizes"], kp_counts=t["kp_counts"], filter=filter)
        ref = frontend.gather_image_pairs_numpy(kp, dm, pairs, matches, scores=scores, **kw)
        got = poselib.gather_image_pairs_torch(_t(kp), _t(dm), pairs, _t(matches), scores=_t(scores), **kw)
        fe.assert_gather_equal(got, ref, (offset, filter))
        bad = IP_PAIRS.index(7)  # an image index outside the set: no row, all slots -1, pure filler, whatever its scores
        x1, x2, d1, d2, n, slot = (_np(v) for v in got)
        assert n[bad] == 0 and (slot[bad] == -1).all() and not x1[bad].any() and not x2[bad].any() and (d1[bad] == 1.0).all() and (d2[bad] == 1.0).all()
        assert n[IP_PAIRS.index(9)] >= 64 and n[IP_PAIRS.index(2)] >= 1  # the 600-row pair and the a == c pair keep rows


# ---- 2. the estimate against the existing ranked route
def _estimate_batch():
    """six pairs, M = 600 without a padded tail: three full pairs and one of 257 rows, all planted with inliers (80 % of their rows), then a
    pair that keeps two rows and one that keeps none"""
    if not hasattr(_estimate_batch, "v"):
        batch = rc.make_batch([(600, None), (257, None), (600, None), (600, None), (70, 2), (64, "none_kept")], 60, pad=0)
        kept = rc.kept_rows(batch)
        scores = rc.batch_scores(kept, 0, 7)                                  # random, levels, special, dropped_high, ascending, descending
        scores[2] = rc.pair_scores("dropped_high", kept[2], 71)               # the second full pair
        scores[3] = rc.pair_scores("special", kept[3], 72)
        _estimate_batch.v = (batch, scores)
    return _estimate_batch.v


def _ro(max_prosac, **kw):
    return dict(fe.RO, max_prosac_iterations=max_prosac, **kw)


def _existing_route(kind, batch, scores, max_prosac):
    """gather_matches_numpy, the scores through its slot, estimate_batch_torch(scores=): (records, the mask on the match rows, n)"""
    import torch
    import mdrp_amd.poselib as poselib
    focal = kind != "calibrated"
    ref = fe.twin(batch, np.float32, np.float32, "both_inf", focal)
    n, slot = ref[4], ref[5]
    gathered = np.zeros(slot.shape)
    for b in range(len(n)):
        k = slot[b] >= 0
        gathered[b, slot[b, k]] = scores[b, k]
    x1, x2, d1, d2 = (torch.tensor(a, device=_dev()) for a in ref[:4])
    cams = (None, None) if focal else (fe.CAM1, fe.CAM2)
    res, mask = poselib.estimate_batch_torch(kind, x1, x2, d1, d2, *cams, _ro(max_prosac), fe.BO, n_per_pair=n, scores=_t(gathered))
    mask = mask.cpu().numpy()
    on_rows = np.zeros(slot.shape, dtype=np.uint8)
    for b in range(len(n)):
        k = slot[b] >= 0
        on_rows[b, k] = mask[b, slot[b, k]]
    return res, on_rows, n


def _front_end(kind, batch, scores, max_prosac, t=None, **ro):
    import mdrp_amd.poselib as poselib
    focal = kind != "calibrated"
    cams = (None, None) if focal else (fe.CAM1, fe.CAM2)
    if t is None:
        t = fe.to_device(batch, np.float32, np.float32, np.int64)
    return poselib.estimate_matches_torch(kind, *t, *cams, _ro(max_prosac, **ro), fe.BO, center1=batch["c1"] if focal else None,
                                          center2=batch["c2"] if focal else None, scores=scores)


def _assert_same_estimate(got, want, what):
    (res, mask, n_used), (res_ref, mask_ref, n) = got, want
    assert isinstance(n_used, np.ndarray) and n_used.dtype == np.int32 and np.array_equal(n_used, n), what
    assert res.dtype == res_ref.dtype and res.tobytes() == res_ref.tobytes(), (what, [k for k in range(len(res)) if res[k].tobytes() != res_ref[k].tobytes()])
    mask = _np(mask)
    assert mask.dtype == np.uint8 and mask.shape == mask_ref.shape and np.array_equal(mask, mask_ref), (what, np.flatnonzero((mask != mask_ref).any(axis=1)))


@pytest.mark.parametrize("max_prosac", [1, 50, 150, 100000])
@pytest.mark.parametrize("kind", KINDS)
def test_estimate_equals_the_ranked_estimator_on_the_unranked_gather(kind, max_prosac):
    """max_prosac_iterations: uniform from the first sample | the switch to uniform sampling inside the first chunk | inside a later chunk | never.
    The ordered copies of the existing route hold d = 0 behind n, the gather holds d = 1 there: no kernel reads past n, or the records differ."""
    batch, scores = _estimate_batch()
    score_dtype = np.float32 if kind != "shared_focal" else np.float64
    want = _existing_route(kind, batch, scores, max_prosac)
    got = _front_end(kind, batch, _t(scores, score_dtype), max_prosac)
    _assert_same_estimate(got, want, (kind, max_prosac))
    res_ref, mask_ref, n = want
    assert n.tolist() == [583, 200, 552, 325, 2, 0]
    # Pairs 0 to 3 are the pairs planted with inliers: on each of them the existing route finds a model, so the equality is not one of empty
    # results.  (Each keeps at least 200 rows: even with max_prosac_iterations = 100000 the 200 progressive samples reach past the first 26
    # records, 100000 * C(26, 3) / C(200, 3) = 198.)
    for b in (0, 1, 2, 3):
        assert int(res_ref[b]["iterations"]) == 200 and int(res_ref[b]["num_inliers"]) >= 3 and mask_ref[b].sum() >= 3, (b, res_ref[b])


# ---- 3. image pairs
@pytest.mark.parametrize("kind", KINDS)
def test_image_pairs_estimate_equals_estimate_matches_on_the_expanded_tables(kind):
    import mdrp_amd.poselib as poselib
    t = ipc.batch()
    focal = kind != "calibrated"
    pairs, matches = t["pairs"][IP_GOOD], _t(t["matches"][IP_GOOD])
    kp, dm, centers = _t(t["keypoints"], np.float32), _t(t["depth_maps"], np.float32), _t(t["centers"])
    kept = ipc.twin(extents=False, pairs=IP_GOOD)[5] >= 0
    scores = _t(rc.batch_scores(kept, 1, 11), np.float32)
    a, c = (_t(pairs[:, k].astype(np.int64)) for k in (0, 1))
    rec = poselib._camera_records(ipc.CAMERAS, ipc.I)
    ro = dict(ipc.RO, max_prosac_iterations=150)
    got = poselib.estimate_image_pairs_torch(kind, kp, dm, pairs, matches, None if focal else ipc.CAMERAS, ro, ipc.BO, centers=centers if focal else None,
                                             scores=scores)
    want = poselib.estimate_matches_torch(kind, kp[a], kp[c], matches, dm[a], dm[c], None if focal else rec[pairs[:, 0]], None if focal else rec[pairs[:, 1]],
                                          ro, ipc.BO, center1=centers[a] if focal else None, center2=centers[c] if focal else None, scores=scores)
    _assert_same_estimate(got, (want[0], _np(want[1]), want[2]), kind)
    assert int(want[0]["num_inliers"].max()) >= 20 and _np(want[1]).sum() >= 20


def test_image_pairs_estimate_with_extents_and_a_pair_outside_the_set():
    """sizes, kp_counts and the pair with an image index outside the set: the ranked estimator on the NumPy definition's ordered buffers"""
    import torch
    import mdrp_amd.poselib as poselib
    from mdrp_amd import frontend
    t = ipc.batch()
    pairs, matches = t["pairs"][IP_PAIRS], t["matches"][IP_PAIRS]
    kp, dm = t["keypoints"].astype(np.float32), t["depth_maps"].astype(np.float32)
    kept = ipc.twin()[5][IP_PAIRS] >= 0
    scores = rc.batch_scores(kept, 3, 12)
    ro = dict(ipc.RO, max_prosac_iterations=100000)
    ref = frontend.gather_image_pairs_numpy(kp, dm, pairs, matches, sizes=t["sizes"], kp_counts=t["kp_counts"], scores=scores)
    rec = poselib._camera_records(ipc.CAMERAS, ipc.I)
    idx = np.where((pairs >= 0) & (pairs < ipc.I), pairs, 0)
    x1, x2, d1, d2 = (torch.tensor(a, device=_dev()) for a in ref[:4])
    res, mask = poselib.estimate_batch_torch("calibrated", x1, x2, d1, d2, rec[idx[:, 0]].copy(), rec[idx[:, 1]].copy(), ro, ipc.BO, n_per_pair=ref[4], scores="presorted")
    mask, slot = mask.cpu().numpy(), ref[5]
    on_rows = np.zeros(slot.shape, dtype=np.uint8)
    for b in range(len(slot)):
        k = slot[b] >= 0
        on_rows[b, k] = mask[b, slot[b, k]]
    got = poselib.estimate_image_pairs_torch("calibrated", _t(kp), _t(dm), pairs, _t(matches), ipc.CAMERAS, ro, ipc.BO, sizes=t["sizes"], kp_counts=t["kp_counts"],
                                             scores=_t(scores))
    _assert_same_estimate(got, (res, on_rows, ref[4]), "extents")
    bad = IP_PAIRS.index(7)
    assert got[2][bad] == 0 and int(got[0][bad]["iterations"]) == 0 and not _np(got[1])[bad].any() and int(res["num_inliers"].max()) >= 20


# ---- 4. identities
def test_constant_scores_presorted_and_the_plain_front_end():
    import mdrp_amd.poselib as poselib
    batch, scores = _estimate_batch()
    t = fe.to_device(batch, np.float32, np.float32, np.int64)
    for kind in ("calibrated", "shared_focal"):
        const = _front_end(kind, batch, _t(np.full(scores.shape, 0.25), np.float32), 150, t)
        pre = _front_end(kind, batch, "presorted", 150, t)
        _assert_same_estimate(const, (pre[0], _np(pre[1]), pre[2]), (kind, "constant scores are the match order"))
        assert int(pre[0]["num_inliers"].max()) >= 20
        # progressive_sampling may be given: these calls sample progressively either way
        ranked = _front_end(kind, batch, _t(scores), 150, t)
        for flag in (True, False):
            same = _front_end(kind, batch, _t(scores), 150, t, progressive_sampling=flag)
            _assert_same_estimate(same, (ranked[0], _np(ranked[1]), ranked[2]), (kind, "progressive_sampling", flag))
        assert ranked[0].tobytes() != pre[0].tobytes()  # the scores do order the records
        # max_prosac_iterations = 1: the uniform sampler on the match-ordered records, which is the front end without scores
        focal = kind != "calibrated"
        cams = (None, None) if focal else (fe.CAM1, fe.CAM2)
        plain = poselib.estimate_matches_torch(kind, *t, *cams, _ro(1), fe.BO, center1=batch["c1"] if focal else None, center2=batch["c2"] if focal else None)
        _assert_same_estimate(_front_end(kind, batch, "presorted", 1, t), (plain[0], _np(plain[1]), plain[2]), (kind, "presorted, no progressive sample"))
    # the gather alone: "presorted" is the unranked gather, constant scores as well
    plain = poselib.gather_matches_torch(*t)
    for s in ("presorted", _t(np.zeros(scores.shape), np.float32)):
        got = poselib.gather_matches_torch(*t, scores=s)
        for a, b in zip(got, plain):
            assert _np(a).tobytes() == _np(b).tobytes()


# ---- 5. refusals
def test_refusals_leave_the_handle_usable():
    import torch
    import mdrp_amd.poselib as poselib
    from mdrp_amd import _capi
    batch, scores = _estimate_batch()
    t = fe.to_device(batch, np.float32, np.float32, np.int64)
    s = _t(scores, np.float32)
    before = _front_end("calibrated", batch, s, 150, t)
    B, M = scores.shape
    bad_scores = (s[:, :-1], s[:-1], s.reshape(-1), s.half(), s.to(torch.int32), s.cpu(), scores, "sorted", 1.0, s[..., None])
    for bad in bad_scores:
        with pytest.raises(ValueError):
            _front_end("calibrated", batch, bad, 150, t)
        with pytest.raises(ValueError):
            poselib.gather_matches_torch(*t, scores=bad)
    it = ipc.batch()
    kp, dm, matches = _t(it["keypoints"], np.float32), _t(it["depth_maps"], np.float32), _t(it["matches"][IP_GOOD])
    ok = _t(np.zeros((len(IP_GOOD), ipc.M)), np.float32)
    for bad in (ok[:, :-1], ok[0], ok.half(), ok.cpu(), "sorted"):
        with pytest.raises(ValueError):
            poselib.gather_image_pairs_torch(kp, dm, it["pairs"][IP_GOOD], matches, scores=bad)
        with pytest.raises(ValueError):
            poselib.estimate_image_pairs_torch("calibrated", kp, dm, it["pairs"][IP_GOOD], matches, ipc.CAMERAS, ipc.RO, ipc.BO, scores=bad)
    # the C ABI's own refusals, below the Python checks: MDRP_ERR_INVALID (1) before any device work
    h = poselib._torch_handle(0, int(torch.cuda.current_stream(t[0].device).cuda_stream))
    mm, keep, _, _, _ = poselib._matches_descriptor(*t, None, None, "both_inf")
    ro, bo = _capi.ransac_opt_from_dict(_ro(150)), _capi.bundle_opt_from_dict(fe.BO)
    cams = poselib._camera_records(fe.CAM1, B)
    out = [torch.empty((B, M, 2), dtype=torch.float64, device=_dev()) for _ in range(2)] + [torch.empty((B, M), dtype=torch.float64, device=_dev()) for _ in range(2)]
    slot = torch.empty((B, M), dtype=torch.int32, device=_dev())
    ptrs = [v.data_ptr() for v in out] + [slot.data_ptr()]
    for score_type in (2, -1, 7):
        with pytest.raises(_capi.MdrpError, match="mdrp error 1"):
            h.estimate_matches_ranked_device(_capi.CALIB, mm, s.data_ptr(), score_type, B, ro, bo, cams, cams)
        with pytest.raises(_capi.MdrpError, match="mdrp error 1"):
            h.gather_matches_ranked(mm, s.data_ptr(), score_type, B, *ptrs)
    h.gather_matches_ranked(mm, None, 7, B, *ptrs)  # without scores the type is not read
    for kind in (3, 4, 5, -1):
        with pytest.raises(_capi.MdrpError, match="mdrp error 1"):
            h.estimate_matches_ranked_device(kind, mm, s.data_ptr(), _capi.F32, B, ro, bo, cams, cams)
    with pytest.raises(_capi.MdrpError, match="mdrp error 1"):  # the estimator's own refusals: a calibrated estimate without cameras
        h.estimate_matches_ranked_device(_capi.CALIB, mm, s.data_ptr(), _capi.F32, B, ro, bo, None, None)
    was = mm.filter
    mm.filter = 2
    with pytest.raises(_capi.MdrpError, match="mdrp error 1"):
        h.estimate_matches_ranked_device(_capi.CALIB, mm, s.data_ptr(), _capi.F32, B, ro, bo, cams, cams)
    mm.filter = was
    ip, keep2, host_pairs, Bi, _, I, _ = poselib._image_pairs_descriptor(kp, dm, it["pairs"][IP_GOOD], matches, None, None, None, "both_inf", True)
    c1, c2 = poselib._pair_cameras(ipc.CAMERAS, host_pairs, I)
    with pytest.raises(_capi.MdrpError, match="mdrp error 1"):
        h.estimate_image_pairs_ranked_device(_capi.CALIB, ip, ok.data_ptr(), 2, Bi, ro, bo, c1, c2)
    with pytest.raises(_capi.MdrpError, match="mdrp error 1"):
        h.gather_image_pairs_ranked(ip, ok.data_ptr(), 2, Bi, 0, 0, 0, 0, 0)
    del keep, keep2
    # without scores the switch is refused as before
    with pytest.raises(NotImplementedError):
        poselib.estimate_matches_torch("calibrated", *t, fe.CAM1, fe.CAM2, _ro(150, progressive_sampling=True), fe.BO)
    with pytest.raises(NotImplementedError):
        poselib.estimate_image_pairs_torch("calibrated", kp, dm, it["pairs"][IP_GOOD], matches, ipc.CAMERAS, dict(ipc.RO, progressive_sampling=True), ipc.BO)
    after = _front_end("calibrated", batch, s, 150, t)
    _assert_same_estimate(after, (before[0], _np(before[1]), before[2]), "a ranked call after the refusals")
    # a plain front-end call on the handle that has ranked equals a fresh handle's
    plain = poselib.estimate_matches_torch("calibrated", *t, fe.CAM1, fe.CAM2, fe.RO, fe.BO)
    stream = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(stream):  # another stream: another handle, which has never seen a ranked call
        assert poselib._torch_handle(0, int(stream.cuda_stream)) is not h
        fresh = poselib.estimate_matches_torch("calibrated", *t, fe.CAM1, fe.CAM2, fe.RO, fe.BO)
    torch.cuda.synchronize()
    _assert_same_estimate(plain, (fresh[0], _np(fresh[1]), fresh[2]), "the plain front end after ranked calls")
