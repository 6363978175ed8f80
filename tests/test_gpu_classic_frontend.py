"""The baselines' device front end on a real MI355X (include/mdrp_classic_frontend.h): poselib.gather_point_*_torch against the NumPy statement of
the same definition (mdrp_amd/frontend.py), and poselib.estimate_baseline_*_torch against that NumPy gather followed by the estimator the project
already has (estimate_baseline_batch_torch with the gather's n_per_pair; ranked: scores="presorted" on the ranked gather).  Everything is compared
as bytes: the front end only moves and widens numbers, and the estimate is the same estimator run twice on identical buffers.  Inputs:
tests/classic_frontend_cases.py."""
import numpy as np
import pytest

import classic_frontend_cases as cf

pytestmark = pytest.mark.gpu

GATHER_BATCHES = ("small", "edges", "long")
TILE_BATCHES = ("m1024", "m1025", "m2048", "m2049")
PROSAC = 150  # max_prosac_iterations of the ranked calls


def _dev():
    import torch
    return torch.device("cuda", 0)


def _tables(batch, kp_dtype, match_dtype):
    import torch
    return (torch.from_numpy(batch["kp1"].astype(kp_dtype)).to(_dev()), torch.from_numpy(batch["kp2"].astype(kp_dtype)).to(_dev()),
            torch.from_numpy(batch["matches"].astype(match_dtype)).to(_dev()))


def _centres(batch, centres):
    import torch
    return (torch.from_numpy(batch["c1"]).to(_dev()), batch["c2"]) if centres else (None, None)  # a device tensor and a host array


def _assert_gather_equal(got, ref, what):
    x1, x2, n, slot = got
    for name, mine, want in (("x1", x1, ref[0]), ("x2", x2, ref[1]), ("slot", slot, ref[3])):
        mine = mine.cpu().numpy()
        assert mine.dtype == want.dtype and mine.shape == want.shape, (what, name)
        assert mine.tobytes() == want.tobytes(), (what, name, np.flatnonzero((mine != want).reshape(len(mine), -1).any(axis=1)))
    assert isinstance(n, np.ndarray) and n.dtype == np.int32 and np.array_equal(n, ref[2]), (what, n, ref[2])


def test_the_inputs_hold_the_planted_cases():
    """kept counts below and at every sample size, rows on the boundaries, non-finite coordinates and bad indices among the dropped rows"""
    b = cf.batches()
    assert cf.kept_rows(b["small"]).sum(axis=1).tolist() == [0, 1, 4, 5, 6, 7]
    assert [rows for rows, _ in b["edges"]["specs"]] == [63, 64, 65, 255, 256, 257] and b["long"]["specs"][0][0] == 600
    for name in ("edges", "long") + TILE_BATCHES:
        t = b[name]
        kept = cf.kept_rows(t)
        for k, (rows, _) in enumerate(t["specs"]):
            if rows < 64:
                assert kept[k].sum() == rows
                continue
            i, j = t["matches"][k, :rows, 0], t["matches"][k, :rows, 1]
            ok = (i >= 0) & (j >= 0) & (i < t["kp1"].shape[1]) & (j < t["kp2"].shape[1])
            p1, p2 = t["kp1"][k, np.where(ok, i, 0)], t["kp2"][k, np.where(ok, j, 0)]
            bad1, bad2 = ok & ~np.isfinite(p1).all(axis=1), ok & ~np.isfinite(p2).all(axis=1)
            assert np.isnan(p1[bad1]).any() and np.isinf(p1[bad1]).any() and np.isnan(p2[bad2]).any() and np.isinf(p2[bad2]).any(), (name, k)
            assert not kept[k, :rows][bad1 | bad2].any() and (~ok).sum() >= 5 and rows - 16 <= kept[k].sum() < rows - 8, (name, k, kept[k].sum())
            first, last = np.flatnonzero(kept[k])[[0, -1]]
            assert (~kept[k, first:last]).any()  # dropped rows between kept ones


@pytest.mark.parametrize("kp_dtype", [np.float32, np.float64])
def test_gather_equals_numpy_bitwise(kp_dtype):
    import mdrp_amd.poselib as poselib
    for name in GATHER_BATCHES + ("m1025",):
        batch = cf.batches()[name]
        for match_dtype in (np.int32, np.int64):
            t = _tables(batch, kp_dtype, match_dtype)
            for centres in (False, True):
                c = _centres(batch, centres)
                got = poselib.gather_point_matches_torch(*t, center1=c[0], center2=c[1])
                _assert_gather_equal(got, cf.twin(batch, kp_dtype, centres), (name, match_dtype.__name__, centres))
    one = cf.batches()["long"]  # one pair as a (K, 2) / (M, 2) call
    t = _tables(one, kp_dtype, np.int64)
    ref = cf.twin(one, kp_dtype, False)
    _assert_gather_equal(poselib.gather_point_matches_torch(t[0][1], t[1][1], t[2][1]), [a[1:] for a in ref], "B = 1")


@pytest.mark.parametrize("rows", (1, 63, 64, 65, 255, 256, 257))
def test_gather_at_every_row_count_without_padding(rows):
    """M itself on the boundaries: no padded tail behind the last row"""
    import mdrp_amd.poselib as poselib
    batch = cf.make_batch([(rows, None), (rows, None)], 300 + rows, pad=0)
    assert batch["matches"].shape[1] == rows
    sc = cf.scores_of(batch, rows % 7, rows)
    t = _tables(batch, np.float32, np.int64)
    _assert_gather_equal(poselib.gather_point_matches_torch(*t), cf.twin(batch, np.float32, False), rows)
    import torch
    got = poselib.gather_point_matches_torch(*t, scores=torch.from_numpy(sc.astype(np.float32)).to(_dev()))
    _assert_gather_equal(got, cf.twin(batch, np.float32, False, sc), (rows, "ranked"))


@pytest.mark.parametrize("name", GATHER_BATCHES + TILE_BATCHES)
def test_ranked_gather_equals_numpy_bitwise_under_every_score_pattern(name):
    """every pattern of frontend_ranked_cases.PATTERNS on every pair of the small batches (the offsets rotate them), two rotations on the large ones;
    float32 and float64 scores of the same values; a score never moves a row's membership"""
    import torch
    import mdrp_amd.poselib as poselib
    batch = cf.batches()[name]
    plain = cf.twin(batch, np.float32, False)
    offsets = range(7) if name in ("small", "edges") else (2, 3)
    tables = {dt: _tables(batch, dt, md) for dt, md in ((np.float32, np.int64), (np.float64, np.int32))}
    for offset in offsets:
        sc = cf.scores_of(batch, offset, 11)
        for kp_dtype, score_dtype, centres in ((np.float32, np.float32, False), (np.float64, np.float64, True), (np.float32, np.float64, True)):
            if name not in ("small", "edges") and kp_dtype != score_dtype:
                continue
            ref = cf.twin(batch, kp_dtype, centres, sc)
            assert np.array_equal(ref[2], plain[2]) and np.array_equal(ref[3] >= 0, plain[3] >= 0)  # the definition: membership is the unranked one
            c = _centres(batch, centres)
            got = poselib.gather_point_matches_torch(*tables[kp_dtype], center1=c[0], center2=c[1], scores=torch.from_numpy(sc.astype(score_dtype)).to(_dev()))
            _assert_gather_equal(got, ref, (name, offset, np.dtype(kp_dtype).name, np.dtype(score_dtype).name))
    # "presorted" is, for the gather alone, no scores at all
    _assert_gather_equal(poselib.gather_point_matches_torch(*tables[np.float32], scores="presorted"), plain, (name, "presorted"))


def _mask_through_slot(mask_ref, slot, n):
    expect = np.zeros(slot.shape, dtype=np.uint8)
    for b in range(len(n)):
        kept = slot[b] >= 0
        expect[b, kept] = mask_ref[b, slot[b, kept]]
    return expect


def _both_ways(kind, batch, kp_dtype, match_dtype, centres, scores=None, score_dtype=None, progressive=None):
    """(front-end route, NumPy front end + estimate_baseline_batch_torch); scores: (B, M) float64 or None"""
    import torch
    import mdrp_amd.poselib as poselib
    cam1, cam2, pp = cf.cameras(kind)
    ro = cf.options(kind, **({} if scores is None else {"max_prosac_iterations": PROSAC}))
    ref = cf.twin(batch, kp_dtype, centres, scores)
    x1, x2 = (torch.tensor(a, device=_dev()) for a in ref[:2])
    res_ref, mask_ref = poselib.estimate_baseline_batch_torch(kind, x1, x2, cam1, cam2, pp, ro, cf.BO, n_per_pair=ref[2], scores=None if scores is None else "presorted")
    if progressive is not None:
        ro = dict(ro, progressive_sampling=progressive)
    c = _centres(batch, centres)
    sc = None if scores is None else torch.from_numpy(scores.astype(score_dtype)).to(_dev())
    got = poselib.estimate_baseline_matches_torch(kind, *_tables(batch, kp_dtype, match_dtype), cam1, cam2, pp, ro, cf.BO, center1=c[0], center2=c[1], scores=sc)
    return got, (res_ref, mask_ref.cpu().numpy(), ref)


def _assert_estimates_equal(got, want, what):
    (res, match_mask, n_used), (res_ref, mask_ref, ref) = got, want
    n, slot = ref[2], ref[3]
    assert isinstance(n_used, np.ndarray) and n_used.dtype == np.int32 and np.array_equal(n_used, n), what
    assert res.dtype == res_ref.dtype and res.tobytes() == res_ref.tobytes(), (what, [k for k in range(len(res)) if res[k].tobytes() != res_ref[k].tobytes()])
    mm = match_mask.cpu().numpy()
    assert mm.dtype == np.uint8 and np.array_equal(mm, _mask_through_slot(mask_ref, slot, n)), what


def _for_kind(kind, batch):
    return cf.shared_focal_tables(batch) if kind == "shared_focal_6pt" else batch


@pytest.mark.parametrize("name", GATHER_BATCHES)
@pytest.mark.parametrize("kind", cf.KINDS)
def test_estimate_from_matches_equals_estimate_on_gathered_input(kind, name):
    """unranked and ranked, on the batches that cross the ordered compaction's boundaries and every sample size; float32 tables with int64 matches
    (what a matcher leaves behind) and float64 tables with int32 matches; with and without centres"""
    batch = _for_kind(kind, cf.batches()[name])
    K = cf.SAMPLE[kind]
    centred = kind == "shared_focal_6pt"
    got, want = _both_ways(kind, batch, np.float32, np.int64, centred)
    _assert_estimates_equal(got, want, (kind, name, "unranked"))
    res, n = got[0], got[2]
    assert (res["iterations"][n >= K] > 0).all() and (res["iterations"][n < K] == 0).all(), (res["iterations"].tolist(), n.tolist())
    if name != "small":
        assert int(res["num_inliers"].max()) > 2 * K and int(got[1].sum()) > 2 * K, res["num_inliers"].tolist()
    else:
        assert n.tolist() == [0, 1, 4, 5, 6, 7]
    sc = cf.scores_of(batch, {"small": 0, "edges": 1, "long": 2}[name], 23)
    progressive = {"small": None, "edges": True, "long": False}[name]
    got, want = _both_ways(kind, batch, np.float64, np.int32, kind != "relpose_5pt", sc, np.float64, progressive)
    _assert_estimates_equal(got, want, (kind, name, "ranked", progressive))


@pytest.mark.parametrize("kind,name", [("fundamental_7pt", "m1024"), ("relpose_5pt", "m1025"), ("shared_focal_6pt", "m1025"), ("relpose_5pt", "m2048"),
                                       ("fundamental_7pt", "m2049")])
def test_ranked_estimate_across_the_rank_block_and_the_key_tile(kind, name):
    batch = _for_kind(kind, cf.batches()[name])
    sc = cf.scores_of(batch, 0, 29)
    got, want = _both_ways(kind, batch, np.float32, np.int64, kind == "shared_focal_6pt", sc, np.float32, progressive=True)
    _assert_estimates_equal(got, want, (kind, name))
    assert int(got[0]["num_inliers"].max()) > 100, got[0]["num_inliers"].tolist()


def test_the_spellings_of_progressive_sampling_and_presorted_rows():
    """on the ranked calls progressive_sampling absent, False and True are one call; scores="presorted" takes the match rows as they are ranked
    already — the unranked gather followed by the progressive sampler — and differs from the plain estimate, which samples uniformly"""
    import mdrp_amd.poselib as poselib
    kind = "fundamental_7pt"
    batch = cf.batches()["edges"]
    sc = cf.scores_of(batch, 4, 31)
    runs = [_both_ways(kind, batch, np.float32, np.int64, False, sc, np.float32, spelling) for spelling in (None, False, True)]
    for got, want in runs:
        _assert_estimates_equal(got, want, "spelling")
    assert runs[0][0][0].tobytes() == runs[1][0][0].tobytes() == runs[2][0][0].tobytes()
    t = _tables(batch, np.float32, np.int64)
    ro = cf.options(kind, max_prosac_iterations=PROSAC)
    presorted = poselib.estimate_baseline_matches_torch(kind, *t, ransac_opt=ro, bundle_opt=cf.BO, scores="presorted")
    ref = cf.twin(batch, np.float32, False)
    import torch
    x1, x2 = (torch.tensor(a, device=_dev()) for a in ref[:2])
    res_ref, mask_ref = poselib.estimate_baseline_batch_torch(kind, x1, x2, ransac_opt=ro, bundle_opt=cf.BO, n_per_pair=ref[2], scores="presorted")
    _assert_estimates_equal(presorted, (res_ref, mask_ref.cpu().numpy(), ref), "presorted")
    plain, _ = _both_ways(kind, batch, np.float32, np.int64, False)
    assert presorted[0].tobytes() != plain[0].tobytes() and presorted[0].tobytes() != runs[0][0][0].tobytes()


# ---- per-image tables
def _image_tables(t, kp_dtype, match_dtype):
    import torch
    return torch.from_numpy(t["keypoints"].astype(kp_dtype)).to(_dev()), torch.from_numpy(t["matches"].astype(match_dtype)).to(_dev())


@pytest.mark.parametrize("kp_dtype", [np.float32, np.float64])
def test_image_pairs_gather_equals_numpy_and_the_per_pair_form(kp_dtype):
    """an image index past the set and a negative one, a == c, a repeated pair, kp_counts below K and past it: bytes of the NumPy definition, and
    of the per-pair form on the expanded tables"""
    import torch
    import mdrp_amd.poselib as poselib
    from mdrp_amd import frontend
    t = cf.image_batch()
    I = t["keypoints"].shape[0]
    pairs = t["pairs"].tolist()
    assert [5, 0] in pairs and [-1, 2] in pairs and [2, 2] in pairs and pairs.count([0, 1]) == 2 and (t["kp_counts"] < 700).sum() == 2 and (t["kp_counts"] > 700).any()
    kp, mt = _image_tables(t, kp_dtype, np.int64)
    exp = cf.expand_image_batch(t)
    sc = cf.rc.batch_scores(cf.image_kept_rows(t), 1, 37)
    for centres in (False, True):
        for scores in (None, sc):
            ref = frontend.gather_point_image_pairs_numpy(t["keypoints"].astype(kp_dtype), t["pairs"], t["matches"], t["centers"] if centres else None,
                                                          t["kp_counts"], scores)
            dev_sc = None if scores is None else torch.from_numpy(scores.astype(kp_dtype)).to(_dev())
            got = poselib.gather_point_image_pairs_torch(kp, t["pairs"] if centres else torch.from_numpy(t["pairs"].copy()).to(_dev()), mt,
                                                         centers=t["centers"] if centres else None, kp_counts=t["kp_counts"], scores=dev_sc)
            _assert_gather_equal(got, ref, ("image pairs", centres, scores is not None))
            c = _centres(exp, centres)
            per_pair = poselib.gather_point_matches_torch(*_tables(exp, kp_dtype, np.int32), center1=c[0], center2=c[1], scores=dev_sc)
            _assert_gather_equal(per_pair, ref, ("expanded", centres, scores is not None))
            bad = [b for b, (a, c_) in enumerate(pairs) if not (0 <= a < I and 0 <= c_ < I)]
            assert len(bad) == 2 and not ref[2][bad].any() and (ref[3][bad] == -1).all() and not ref[0][bad].any()
    none = frontend.gather_point_image_pairs_numpy(t["keypoints"].astype(kp_dtype), t["pairs"], t["matches"])
    _assert_gather_equal(poselib.gather_point_image_pairs_torch(kp, t["pairs"], mt), none, "no counts")
    assert none[2].sum() > ref[2].sum()  # (the counts cut rows off)


@pytest.mark.parametrize("kind", cf.KINDS)
def test_image_pairs_estimate_equals_the_per_pair_form(kind):
    """records, match mask and counts of the per-image call are those of the per-pair call on the expanded tables, unranked and ranked; the 5-point
    kind's per-image cameras expand through the pairs"""
    import torch
    import image_pairs_cases as ipc
    import mdrp_amd.poselib as poselib
    t = cf.image_batch()
    I = t["keypoints"].shape[0]
    exp = cf.expand_image_batch(t)
    kp, mt = _image_tables(t, np.float32, np.int64)
    pp = (0.0, 0.0) if kind == "shared_focal_6pt" else None
    cams = ipc.CAMERAS if kind == "relpose_5pt" else None
    cam1, cam2 = poselib._pair_cameras(ipc.CAMERAS, poselib._host_pairs(t["pairs"]), I) if kind == "relpose_5pt" else (None, None)
    centres = kind != "relpose_5pt"
    sc = cf.rc.batch_scores(cf.image_kept_rows(t), 5, 41)
    for scores in (None, sc):
        ro = cf.options(kind, **({} if scores is None else {"max_prosac_iterations": PROSAC, "progressive_sampling": True}))
        dev_sc = None if scores is None else torch.from_numpy(scores.astype(np.float32)).to(_dev())
        got = poselib.estimate_baseline_image_pairs_torch(kind, kp, t["pairs"], mt, cams, pp, ro, cf.BO, centers=t["centers"] if centres else None,
                                                          kp_counts=t["kp_counts"], scores=dev_sc)
        c = _centres(exp, centres)
        want = poselib.estimate_baseline_matches_torch(kind, *_tables(exp, np.float32, np.int64), cam1, cam2, pp, ro, cf.BO, center1=c[0], center2=c[1], scores=dev_sc)
        assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[2], want[2]) and torch.equal(got[1], want[1]), (kind, scores is not None)
        enough = (1 if kind == "shared_focal_6pt" else 2) * cf.SAMPLE[kind]  # (the images of a pair differ in scale and centre offset: one focal fits fewer)
        assert got[2].max() > 500 and (got[2] == 0).sum() >= 2 and int(got[0]["num_inliers"].max()) > enough, (got[2].tolist(), got[0]["num_inliers"].tolist())
    # and of the two-call route on the NumPy definition
    from mdrp_amd import frontend
    ref = frontend.gather_point_image_pairs_numpy(t["keypoints"].astype(np.float32), t["pairs"], t["matches"], t["centers"] if centres else None, t["kp_counts"], sc)
    x1, x2 = (torch.tensor(a, device=_dev()) for a in ref[:2])
    res_ref, mask_ref = poselib.estimate_baseline_batch_torch(kind, x1, x2, cam1, cam2, pp, ro, cf.BO, n_per_pair=ref[2], scores="presorted")
    _assert_estimates_equal(got, (res_ref, mask_ref.cpu().numpy(), ref), (kind, "image pairs, two-call route"))


def test_refusals_leave_the_handle_usable():
    """a monodepth kind, real_focal_check, progressive_sampling without scores, a NULL matches pointer: each refused, each followed by a good call
    that returns the bytes of a fresh handle"""
    import torch
    import mdrp_amd.poselib as poselib
    from mdrp_amd import _capi
    kind = "fundamental_7pt"
    batch = cf.batches()["edges"]
    t = _tables(batch, np.float32, np.int64)
    ro = cf.options(kind)
    B = t[0].shape[0]

    def good(h):
        pm, keep, B_, M, _ = poselib._point_matches_descriptor(*t, None, None)
        mask = torch.zeros((B_, M), dtype=torch.uint8, device=_dev())
        n = h.estimate_points_device(_capi.FUNDAMENTAL_7PT, pm, B_, _capi.ransac_opt_from_dict(ro), _capi.bundle_opt_from_dict(cf.BO), None, None, mask.data_ptr())
        return h.fetch_results(B_).tobytes(), mask.cpu().numpy().tobytes(), n.tobytes()

    fresh = _capi.Handle(0)
    try:
        want = good(fresh)
    finally:
        fresh.close()
    h = _capi.Handle(0)
    try:
        pm, keep, _, M, _ = poselib._point_matches_descriptor(*t, None, None)
        rop, bop = _capi.ransac_opt_from_dict(ro), _capi.bundle_opt_from_dict(cf.BO)
        cams = poselib._camera_records(cf.fe.CAM1, B)
        sc = torch.zeros((B, M), dtype=torch.float32, device=_dev())
        refusals = 0
        for mono in (_capi.CALIB, _capi.SHARED_FOCAL, _capi.VARYING_FOCAL, -1, 6):
            for ranked in (False, True):
                with pytest.raises(_capi.MdrpError, match="mdrp error 1"):
                    h.estimate_points_device(mono, pm, B, rop, bop, cams, cams, None, sc.data_ptr(), _capi.F32, ranked)
                refusals += 1
                assert good(h) == want, (mono, ranked)
        for ranked in (False, True):
            with pytest.raises(NotImplementedError):
                h.estimate_points_device(_capi.FUNDAMENTAL_7PT, pm, B, _capi.ransac_opt_from_dict(dict(ro, real_focal_check=True)), bop, None, None, None, sc.data_ptr(),
                                         _capi.F32, ranked)
            assert good(h) == want, ("real_focal_check", ranked)
        with pytest.raises(NotImplementedError):  # progressive_sampling needs the scores: refused on the unranked entry point alone
            h.estimate_points_device(_capi.FUNDAMENTAL_7PT, pm, B, _capi.ransac_opt_from_dict(dict(ro, progressive_sampling=True)), bop)
        assert good(h) == want, "progressive_sampling"
        with pytest.raises(_capi.MdrpError, match="mdrp error 1"):  # the 5-point kind without cameras, the 6-point kind without its principal point
            h.estimate_points_device(_capi.RELPOSE_5PT, pm, B, rop, bop)
        with pytest.raises(_capi.MdrpError, match="mdrp error 1"):
            h.estimate_points_device(_capi.SHARED_6PT, pm, B, rop, bop)
        for field, value in (("matches", None), ("kp1", None), ("kp_type", 2), ("m_max", -1), ("k2", -1)):
            was = getattr(pm, field)
            setattr(pm, field, value)
            for ranked in (False, True):
                with pytest.raises(_capi.MdrpError, match="mdrp error 1"):
                    h.estimate_points_device(_capi.FUNDAMENTAL_7PT, pm, B, rop, bop, None, None, None, sc.data_ptr(), _capi.F32, ranked)
                with pytest.raises(_capi.MdrpError, match="mdrp error 1"):
                    h.gather_points(pm, B, sc.data_ptr(), sc.data_ptr(), sc.data_ptr(), sc.data_ptr(), _capi.F32, ranked)
            setattr(pm, field, was)
            assert good(h) == want, field
        with pytest.raises(_capi.MdrpError, match="mdrp error 1"):  # a score type that is none
            h.estimate_points_device(_capi.FUNDAMENTAL_7PT, pm, B, rop, bop, None, None, None, sc.data_ptr(), 2, True)
        assert good(h) == want, "score_type"
        assert refusals == 10
        del keep
    finally:
        h.close()
    # the Python entry points: the same refusals before the library is reached; the monodepth front end keeps refusing the baselines
    with pytest.raises(ValueError, match="kind"):
        poselib.estimate_baseline_matches_torch("calibrated", *t, ransac_opt=ro, bundle_opt=cf.BO)
    with pytest.raises(NotImplementedError):
        poselib.estimate_baseline_matches_torch(kind, *t, ransac_opt=dict(ro, progressive_sampling=True), bundle_opt=cf.BO)
    with pytest.raises(NotImplementedError):
        poselib.estimate_baseline_matches_torch(kind, *t, ransac_opt=dict(ro, real_focal_check=True), bundle_opt=cf.BO)
    dm = torch.ones((B, 8, 8), dtype=torch.float32, device=_dev())
    for k in (_capi.FUNDAMENTAL_7PT, "fundamental_7pt"):
        with pytest.raises((ValueError, _capi.MdrpError)):
            poselib.estimate_matches_torch(k, *t, dm, dm, None, None, ro, cf.BO)
    got, want2 = _both_ways(kind, batch, np.float32, np.int64, False)
    _assert_estimates_equal(got, want2, "after the refusals")
