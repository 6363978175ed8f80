"""PROSAC on the 5- / 6- / 7-point baselines on a real MI355X (mdrp_estimate_classic_ranked): the device sampler for sample sizes 5, 6, 7
against the reference binary's tables, the estimators against the reference's runs under progressive_sampling
(tests/golden/classic_prosac_ref.npz), the identities with today's estimator on pre-sorted records, independence of the schedule and of the handle's
history, refusals and the blocking C entry."""
import numpy as np
import pytest

import classic_prosac_cases as ccs
import prosac_cases as pcs
import prosac_ref as ps
from mdrp_amd import synth
from test_oracle_classic import fund_diff, pose_diff

pytestmark = pytest.mark.gpu

KNOBS = ("MDRP_CHUNKS", "MDRP_LO_OVERLAP", "MDRP_BOUND", "MDRP_FUSE_TAIL", "MDRP_LO_THREADS", "MDRP_FINAL_THREADS", "MDRP_PAIRS_PER_PASS", "MDRP_SAMPLE_THREADS")
SIZES = (5, 6, 7)
SCORE_RTOL = 1e-9  # tests/test_gpu_classic.py on classic.npz


@pytest.fixture(scope="module")
def capi():
    from mdrp_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def handle(capi):
    return capi.default_handle(0)


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _torch(kind, x1, x2, ro, n_per_pair=None, scores=None):
    """(records, masks (B, N) uint8 numpy) through poselib.estimate_baseline_batch_torch; scores: None (today's estimator), "presorted" or (B, N)"""
    import torch
    import mdrp_amd.poselib as poselib
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev) for a in (x1, x2)]
    sc = scores if scores is None or isinstance(scores, str) else torch.from_numpy(np.ascontiguousarray(scores)).to(dev)
    res, mask = poselib.estimate_baseline_batch_torch(ccs.KIND_NAMES[kind], *t, ccs.CAMERA, ccs.CAMERA, (0.0, 0.0), ro, ccs.BUNDLE, n_per_pair=n_per_pair,
                                                      **({} if scores is None else {"scores": sc}))
    return res, mask.cpu().numpy()


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


# ---- 1. the sampler
def _chunkings(count):
    lens, left = [], count
    for v in (1, 63, 64, 65):
        if left > v:
            lens.append(v); left -= v
    return [[count], lens + [left]]


@pytest.mark.parametrize("threads", (None, "64"))
@pytest.mark.parametrize("K", SIZES)
def test_device_sampler_draws_the_reference_tables(handle, K, threads, monkeypatch):
    """mdrp_prosac_samples_k through the production launch, in one chunk and in chunks (1, 63, 64, 65, rest): every index of the reference's table for
    every row, with the carried (state, sample index) across chunk boundaries, the switch to uniform sampling and the end of the truncated table
    inside a step; with 64 sampler threads and the default"""
    if threads:
        monkeypatch.setenv("MDRP_SAMPLE_THREADS", threads)
    for row, (n, seed, mp, count) in enumerate(ccs.sampler_rows(K)):
        want = ccs.golden()[f"samples_{K}_{row}"].astype(np.uint32)
        for lens in _chunkings(count):
            got = handle.prosac_samples_k(seed, n, K, mp, lens)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert got.shape == want.shape and bad.size == 0, (K, row, lens, bad[:5], got[bad[:3]], want[bad[:3]])


def test_sample_size_three_is_the_monodepth_sampler(handle, capi):
    for n, seed, mp, count in pcs.SAMPLER_ROWS[:10]:
        for lens in _chunkings(count):
            assert np.array_equal(handle.prosac_samples_k(seed, n, 3, mp, lens), handle.prosac_samples(seed, n, mp, lens)), (n, seed, mp, lens)
    for K in SIZES:  # below K records nothing is written
        assert (handle.prosac_samples_k(0, K - 1, K, 100000, [5, 5], fill=0xABCD) == 0xABCD).all()
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        handle.prosac_samples_k(0, 20, 4, 100, [5])


# ---- 2. the estimators against the reference binary
def _record(kind, capi, r, mask_row):
    m = r["model"]
    if kind == 5:
        model = np.asarray(capi.model_to_fundamental(m)).reshape(-1)
    else:
        model = np.r_[m["q"], m["t"], m["f1"]]
    return dict(model=model, iterations=int(r["iterations"]), num_inliers=int(r["num_inliers"]), refinements=int(r["refinements"]),
                model_score=float(r["model_score"]), mask=np.asarray(mask_row))


def _want(g, uniform=False):
    m, st, mask = (g["umodel"], g["ustats"], g["umask"]) if uniform else (g["model"], g["stats"], g["mask"])
    return dict(model=m, refinements=int(st[0]), iterations=int(st[1]), num_inliers=int(st[2]), model_score=float(st[4]), mask=mask)


def deviation(kind, got, want, n):
    """fields in which got differs from the reference's record, under the comparisons tests/test_gpu_classic.py applies to classic.npz: |t| of a pose
    is a gauge, F up to sign and scale, models to 1e-6, scores to 1e-9, everything else equal"""
    out = []
    if got["iterations"] != want["iterations"]: out.append("iterations")
    if got["num_inliers"] != want["num_inliers"]: out.append("num_inliers")
    if not np.array_equal(got["mask"][:n], want["mask"][:n]): out.append("mask")
    if kind == 5:
        ok = fund_diff(got["model"], want["model"]) < 1e-6
    else:
        ok = pose_diff(got["model"][:7], want["model"][:7]) < 1e-6 and (kind != 4 or abs(got["model"][7] - want["model"][7]) < 1e-6 * abs(want["model"][7]))
    if not ok: out.append("model")
    if not abs(got["model_score"] - want["model_score"]) <= SCORE_RTOL * abs(want["model_score"]): out.append("model_score")
    if got["refinements"] != want["refinements"]: out.append("refinements")
    return out


# kind -> {case: fields}: at most one case of the 5- and of the 6-point estimator, none of the 7-point one, and only where the test itself shows that
# today's uniform estimator on the same records deviates from the reference's uniform record in the same fields
EXEMPT = {3: {}, 4: {}, 5: {}}


@pytest.mark.parametrize("kind", ccs.KINDS)
def test_against_the_reference_under_progressive_sampling(capi, kind):
    """every fixture case, fed in the caller's unsorted order with its scores: iterations, inlier counts, masks and LO counts identical to the reference
    binary's run under progressive_sampling on the pre-sorted records, model to 1e-6, score to 1e-9"""
    assert len(EXEMPT[kind]) <= (0 if kind == 5 else 1)
    for index in range(len(ccs.cases(kind))):
        c, g = ccs.case(kind, index), ccs.golden_case(kind, index)
        assert ccs.digest(c) == g["digest"], "the inputs are not the ones the fixture was recorded on"
        assert np.array_equal(c["order"], g["order"]) and np.array_equal(ps.order(c["scores"]), g["order"])
        n, o = c["n"], c["order"]
        res, mask = _torch(kind, c["x1"][None], c["x2"][None], ccs.ransac_dict(c), scores=c["scores"][None])
        got, want = _record(kind, capi, res[0], mask[0][o]), _want(g)  # (the fixture's mask is in rank order)
        dev = deviation(kind, got, want, n)
        print(kind, index, "LOs", got["refinements"], want["refinements"], "iterations", got["iterations"], want["iterations"], "inliers", got["num_inliers"],
              want["num_inliers"], "score", got["model_score"], want["model_score"], dev)
        allowed = EXEMPT[kind].get(index, [])
        assert [f for f in dev if f not in allowed] == [], (kind, index, dev)
        if index in EXEMPT[kind]:  # earned: today's uniform estimator deviates from the reference's uniform record on the same records, in the same fields
            assert set(allowed) <= set(dev), (kind, index, "the exemption is not needed", dev)
            ures, umask = _torch(kind, c["x1"][o][None], c["x2"][o][None], ccs.ransac_dict(c))
            udev = deviation(kind, _record(kind, capi, ures[0], umask[0]), _want(g, uniform=True), n)
            print("   today's estimator on the same records deviates from the reference's uniform record in", udev)
            assert set(allowed) <= set(udev), (kind, index, udev)


# ---- 3. identities
@pytest.mark.parametrize("kind", ccs.KINDS)
def test_identities_with_todays_estimator(capi, kind):
    """max_prosac_iterations 0 and 1: today's estimator on the pre-sorted records, records and masks bit for bit; "presorted" on sorted records = scores
    on shuffled ones with the mask permuted back; ties and NaN scores rank by k_rank's rule"""
    c = ccs.case(kind, 1)
    n, o = c["n"], c["order"]
    sx1, sx2 = c["x1"][o], c["x2"][o]
    plain = _torch(kind, sx1[None], sx2[None], ccs.ransac_dict(c))
    for mp in (0, 1):
        ro = dict(ccs.ransac_dict(c), max_prosac_iterations=mp)
        assert _same(_torch(kind, sx1[None], sx2[None], ro, scores="presorted"), plain), (kind, mp)
        res, mask = _torch(kind, c["x1"][None], c["x2"][None], ro, scores=c["scores"][None])
        assert res.tobytes() == plain[0].tobytes() and np.array_equal(mask[0][o], plain[1][0]), (kind, mp)
    pre = _torch(kind, sx1[None], sx2[None], ccs.ransac_dict(c), scores="presorted")
    assert not _same(pre, plain)  # (150 progressive samples: another sample sequence)
    # padded, float32 scores, progressive_sampling = True accepted
    pad = lambda a: np.concatenate([a, np.zeros((17,) + a.shape[1:])])[None]  # noqa: E731
    sc32 = pad(np.round(c["scores"], 3).astype(np.float32))
    o32 = ps.order(sc32[0, :n].astype(np.float64))
    res, mask = _torch(kind, pad(c["x1"]), pad(c["x2"]), dict(ccs.ransac_dict(c), progressive_sampling=True), n_per_pair=np.array([n], np.int32), scores=sc32)
    w = _torch(kind, c["x1"][o32][None], c["x2"][o32][None], ccs.ransac_dict(c), scores="presorted")
    assert res.tobytes() == w[0].tobytes() and np.array_equal(mask[0][:n][o32], w[1][0]) and not mask[0][n:].any()
    # ties and NaN: one decimal of the scores, a tenth of them NaN
    sc = np.round(c["scores"], 1)
    sc[::10] = np.nan
    ot = ps.order(sc)
    res, mask = _torch(kind, c["x1"][None], c["x2"][None], ccs.ransac_dict(c), scores=sc[None])
    w = _torch(kind, c["x1"][ot][None], c["x2"][ot][None], ccs.ransac_dict(c), scores="presorted")
    assert res.tobytes() == w[0].tobytes() and np.array_equal(mask[0][ot], w[1][0])


# ---- 4. independence of the schedule
@pytest.mark.parametrize("kind", ccs.KINDS)
def test_ragged_batch_under_other_schedules(capi, kind, monkeypatch):
    """four pairs with n = (K - 1, K, 97, 300) padded to 300: the same bytes under schedules that force several chunks, super-chunks and passes; the
    pair below the sample size returns what the plain estimator returns for it"""
    K = ccs.SAMPLE_SIZE[kind]
    ns = np.array([K - 1, K, 97, 300], dtype=np.int32)
    x1, x2, sc = np.zeros((4, 300, 2)), np.zeros((4, 300, 2)), np.zeros((4, 300))
    for i, n in enumerate(ns):
        p = synth.make_pair(7300 + 10 * kind + i, int(n), outlier_frac=0.3 if n > 7 else 0.0, random_focal="shared" if kind == 4 else None)
        x1[i, :n], x2[i, :n] = p["x1"], p["x2"]
        sc[i, :n] = np.round(-(p["is_outlier"] + np.random.default_rng(i).normal(0.0, 0.6, n)), 1)
    ro = dict(max_iterations=200, min_iterations=50, seed=5, max_epipolar_error=ccs.THRESHOLD, max_prosac_iterations=100)
    base = _torch(kind, x1, x2, ro, n_per_pair=ns, scores=sc)
    assert int(base[0]["iterations"][0]) == 0 and int(base[0]["iterations"][3]) >= 50 and int(base[0]["num_inliers"][3]) > 100
    for i, n in enumerate(ns):
        assert not base[1][i][n:].any()
    plain = _torch(kind, x1, x2, ro, n_per_pair=ns)
    assert base[0][0].tobytes() == plain[0][0].tobytes() and np.array_equal(base[1][0], plain[1][0])
    for env in ({"MDRP_CHUNKS": "16,32", "MDRP_PAIRS_PER_PASS": "3"}, {"MDRP_CHUNKS": "7,9,11"}, {"MDRP_LO_OVERLAP": "0"}):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        assert _same(_torch(kind, x1, x2, ro, n_per_pair=ns, scores=sc), base), (kind, env)


# ---- 5. independence of the handle's history
def _calls(capi, kind):
    c = ccs.case(kind, 0)
    cam = None
    if kind == 3:
        import mdrp_amd.poselib as poselib
        cam = poselib._camera_records(ccs.CAMERA, 1)
    elif kind == 4:
        cam = np.zeros(1, dtype=capi.CAMERA_DTYPE)
    ro, bo = capi.ransac_opt_from_dict(ccs.ransac_dict(c)), capi.bundle_opt_from_dict(ccs.BUNDLE)
    m = pcs.case(1, 6)
    mro, mbo = capi.ransac_opt_from_dict(pcs.ransac_dict(m)), capi.bundle_opt_from_dict({"loss_type": pcs.LOSS, "gradient_tol": 1e-10})
    return {"ranked": lambda h: h.estimate_classic_ranked(kind, c["x1"][None], c["x2"][None], c["scores"][None], ro, bo, None, cam, cam),
            "plain": lambda h: h.estimate_batch(kind, c["x1"][None], c["x2"][None], None, None, ro, bo, None, cam, cam),
            "mono": lambda h: h.estimate_batch_ranked(1, m["x1"][None], m["x2"][None], m["d1"][None], m["d2"][None], m["scores"][None], mro, mbo)}


@pytest.mark.parametrize("kind", ccs.KINDS)
def test_results_do_not_depend_on_the_handles_history(capi, kind):
    """behind a ranked baseline call, a plain baseline call and a monodepth ranked call return the bytes of a fresh handle; and in the other order"""
    calls = _calls(capi, kind)
    fresh = {}
    for name, call in calls.items():
        h = capi.Handle(0)
        fresh[name] = call(h)
        h.close()
    for sequence in (("ranked", "plain", "mono"), ("mono", "plain", "ranked")):
        h = capi.Handle(0)
        for name in sequence:
            assert _same(calls[name](h), fresh[name]), (kind, sequence, name)
        h.close()
    assert int(fresh["ranked"][0]["num_inliers"][0]) > 100


# ---- 6. refusals
def test_refusals_leave_the_handle_usable(capi):
    """kinds 0 - 2 and out-of-range kinds, missing cameras for the 5-point kind, a missing principal point for the 6-point kind, real_focal_check and
    n_per_pair > n_max: refused; a valid call behind them repeats its earlier answer"""
    import mdrp_amd.poselib as poselib
    c = ccs.case(3, 4)
    n = c["n"]
    x1, x2, sc = c["x1"][None], c["x2"][None], c["scores"][None]
    ro, bo = capi.ransac_opt_from_dict(ccs.ransac_dict(c, progressive_sampling=True)), capi.bundle_opt_from_dict(ccs.BUNDLE)
    cam = poselib._camera_records(ccs.CAMERA, 1)
    h = capi.Handle(0)
    before = h.estimate_classic_ranked(3, x1, x2, sc, ro, bo, None, cam, cam)
    for kind in (capi.CALIB, capi.SHARED_FOCAL, capi.VARYING_FOCAL, 6, 17, -1):
        with pytest.raises(capi.MdrpError, match="mdrp error 1"):
            h.estimate_classic_ranked(kind, x1, x2, sc, ro, bo, None, cam, cam)
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.estimate_classic_ranked(3, x1, x2, sc, ro, bo, None, None, None)
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.estimate_classic_ranked(3, x1, x2, sc, ro, bo, None, cam, None)
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.estimate_classic_ranked(4, x1, x2, sc, ro, bo, None, None, None)
    focal_check = capi.ransac_opt_from_dict(ccs.ransac_dict(c, real_focal_check=True))
    for kind in (4, 5):
        with pytest.raises(NotImplementedError):
            h.estimate_classic_ranked(kind, x1, x2, sc, focal_check, bo, None, cam, cam)
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.estimate_classic_ranked(3, x1, x2, sc, ro, bo, np.array([n + 1], np.int32), cam, cam)
    dev_args = (0, 0, 0, 1, n, ro, bo, None, cam, cam)  # (refused before any pointer is read)
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.estimate_classic_ranked_device(1, *dev_args)
    after = h.estimate_classic_ranked(3, x1, x2, sc, ro, bo, None, cam, cam)
    assert _same(after, before) and int(before[0]["num_inliers"][0]) > 30
    h.close()


# ---- 7. the blocking C entry and the drop-in functions
@pytest.mark.parametrize("kind", ccs.KINDS)
def test_blocking_entry_and_drop_in_functions(capi, handle, kind):
    """mdrp_estimate_classic_ranked on host buffers and on device buffers returns the records of the async form; scores= of the batch and single-pair
    functions returns them too, info["inliers"] in the caller's order"""
    import ctypes as C
    import torch
    import mdrp_amd.poselib as poselib
    c = ccs.case(kind, 3)
    n = c["n"]
    rod = ccs.ransac_dict(c)
    want = _torch(kind, c["x1"][None], c["x2"][None], rod, scores=c["scores"][None])
    cam = poselib._camera_records(ccs.CAMERA, 1) if kind == 3 else (np.zeros(1, dtype=capi.CAMERA_DTYPE) if kind == 4 else None)
    ro, bo = capi.ransac_opt_from_dict(rod), capi.bundle_opt_from_dict(ccs.BUNDLE)
    assert _same(handle.estimate_classic_ranked(kind, c["x1"][None], c["x2"][None], c["scores"][None], ro, bo, None, cam, cam), want)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(c[k][None])).to(dev) for k in ("x1", "x2", "scores")]
    mask = torch.zeros((1, n), dtype=torch.uint8, device=dev)
    out = np.zeros(1, dtype=capi.RESULT_DTYPE)
    torch.cuda.synchronize()
    rc = handle._lib.mdrp_estimate_classic_ranked(handle._h, kind, capi.MEM_DEVICE, *(C.c_void_p(v.data_ptr()) for v in t), 1, n, None, capi._ptr(cam), capi._ptr(cam),
                                                  C.byref(ro), C.byref(bo), capi._ptr(out), C.c_void_p(mask.data_ptr()))
    assert rc == 0 and _same((out, mask.cpu().numpy()), want)
    if kind == 3:
        models, infos = poselib.estimate_relative_pose_batch([c["x1"]], [c["x2"]], ccs.CAMERA, ccs.CAMERA, rod, ccs.BUNDLE, scores=[c["scores"]])
        one, info = poselib.estimate_relative_pose(c["x1"], c["x2"], ccs.CAMERA, ccs.CAMERA, dict(rod, progressive_sampling=True), ccs.BUNDLE, scores=c["scores"])
        assert np.array_equal(models[0].q, want[0][0]["model"]["q"]) and np.array_equal(one.q, models[0].q)
    elif kind == 4:
        models, infos = poselib.estimate_shared_focal_relative_pose_batch([c["x1"]], [c["x2"]], (0.0, 0.0), rod, ccs.BUNDLE, scores=[c["scores"]])
        one, info = poselib.estimate_shared_focal_relative_pose(c["x1"], c["x2"], (0.0, 0.0), dict(rod, progressive_sampling=True), ccs.BUNDLE, scores=c["scores"])
        assert models[0].camera1.focal() == float(want[0][0]["model"]["f1"]) == one.camera1.focal()
    else:
        models, infos = poselib.estimate_fundamental_batch([c["x1"]], [c["x2"]], rod, ccs.BUNDLE, scores=[c["scores"]])
        one, info = poselib.estimate_fundamental(c["x1"], c["x2"], dict(rod, progressive_sampling=True), ccs.BUNDLE, scores=c["scores"])
        assert np.array_equal(models[0], capi.model_to_fundamental(want[0][0]["model"])) and np.array_equal(one, models[0])
    for i in (infos[0], info):
        assert (i["refinements"], i["iterations"], i["num_inliers"]) == tuple(int(want[0][0][k]) for k in ("refinements", "iterations", "num_inliers"))
        assert np.array_equal(np.array(i["inliers"], dtype=np.uint8), want[1][0])
    o = c["order"]
    pres = poselib.estimate_fundamental(c["x1"][o], c["x2"][o], rod, ccs.BUNDLE, scores="presorted")[1] if kind == 5 else None
    if pres is not None:
        assert np.array_equal(np.array(pres["inliers"], dtype=np.uint8), want[1][0][o])
