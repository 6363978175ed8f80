"""mdrp_refine_batch on a real MI355X: caller-supplied models through k_from_model against the yardstick (tests/from_models_ref.py), against the
estimator itself, and at the boundary of the C ABI.  The inputs and the yardstick's answers come from tests/from_models_cases.py."""
import numpy as np
import pytest

import from_models_cases as fc
import from_models_ref as fm
import helpers

pytestmark = pytest.mark.gpu

SCORE_RTOL = 1e-6  # the relative tolerance test_gpu_parity.py::test_schedule_does_not_change_results applies to model_score, at same_model's 1e-6
BIG = dict(n_list=(8200, 8100), first=72000, start=())  # over LM_LIST_MAX_N = 8192: no 16-bit work lists


@pytest.fixture(scope="module")
def capi():
    from mdrp_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def handle(capi):
    return capi.default_handle(0)


def _against_the_yardstick(capi, handle, name, loss, **kw):
    kind = helpers.OPTIONS_KINDS[name][0]
    b = fc.batch(name, **kw)
    B = len(b["n"])
    # the conditions on the inputs, from the yardstick alone: every branch the batch is there for is taken, and no correspondence sits on the threshold
    # of the model whose inliers are compared
    if not kw:
        assert fc.branches(name, loss) >= {"lo_adopted", "lo_not_adopted", "inliers_skipped", "inliers_run", "nan", "n<3"}
    else:
        assert fc.branches(name, loss, **kw) >= {"lo_adopted", "inliers_run"}
    ro, bo = fc.library_options(name, loss, capi)
    c1, c2 = fc.camera_records(b, capi)
    models = capi.array_to_models(b["models"])
    compared = 0
    for stages in (0, 1, 2, 3):
        want = fc.yardstick(name, loss, stages, **kw)
        assert min(fc.threshold_margin(kind, r) for r in want) > 1e-6
        res, mask, score0, inl0 = handle.refine_batch(kind, b["x1"], b["x2"], b["d1"], b["d2"], models, ro, bo, stages, b["n"], c1, c2)
        for i, n in enumerate(b["n"]):
            r, w, tag = res[i], want[i], (name, loss, stages, i, int(n))
            got = capi.model_to_array(r["model"])
            print(tag, "inliers", int(r["num_inliers"]), w["num_inliers"], "initial", int(inl0[i]), w["initial_inliers"], "LMs", int(r["refinements"]), w["refinements"],
                  "model diff", helpers.model_diff(got, w["model"]) if np.isfinite(w["model"]).all() else "nan", "score", float(r["model_score"]), w["model_score"])
            assert np.array_equal(mask[i, :n], w["mask"]) and not mask[i, n:].any(), tag
            assert int(r["num_inliers"]) == w["num_inliers"] and int(inl0[i]) == w["initial_inliers"] and int(r["refinements"]) == w["refinements"], tag
            assert int(r["iterations"]) == 0 and float(r["inlier_ratio"]) == (w["num_inliers"] / n if n >= 3 else 0.0), tag
            assert helpers.same_model(got, w["model"]), (tag, got, w["model"])
            assert abs(float(r["model_score"]) - w["model_score"]) <= SCORE_RTOL * abs(w["model_score"]), tag
            assert abs(float(score0[i]) - w["initial_score"]) <= SCORE_RTOL * abs(w["initial_score"]), tag
            if w["refinements"] == 0:
                assert r["model"].tobytes() == models[i].tobytes(), tag  # no LM ran: bit for bit
            compared += 1
    assert compared == 4 * B  # no pair is left out of any comparison


@pytest.mark.parametrize("loss", sorted(fc.LOSSES))
@pytest.mark.parametrize("name", helpers.OPTIONS_NAMES)
def test_ragged_batch_against_the_yardstick(capi, handle, name, loss):
    """B = 12 ragged pairs (n = 0 .. 777 = n_max: below 3, around one wavefront's 64, over one workgroup's 256, no multiple of anything), start models
    perturbed / exact / identity / NaN / hopeless, all four values of `stages`: masks, counts and LM runs identical, models to 1e-6"""
    _against_the_yardstick(capi, handle, name, loss)


@pytest.mark.parametrize("loss", sorted(fc.LOSSES))
def test_beyond_the_16_bit_work_lists(capi, handle, loss):
    """n_max = 8200 > LM_LIST_MAX_N: the LM sweeps visit every record (stride 0), the inlier-only refinement reads the mask"""
    _against_the_yardstick(capi, handle, "varying", loss, **BIG)


@pytest.mark.parametrize("name", helpers.OPTIONS_NAMES)
def test_inliers_stage_alone_at_the_count_rule(capi, handle, name):
    """stages = INLIERS from a model with exactly 3 (7: varying focal) exact inliers among gross outliers, and with one more: the inlier-only refinement
    needs MORE than the rule's count, so `refinements` is 0, then 1 (tests/from_models_cases.exact_inlier_batch; the yardstick confirms both counts)"""
    kind = helpers.OPTIONS_KINDS[name][0]
    rule = 7 if kind == 2 else 3
    counts = (rule, rule + 1)
    b = fc.exact_inlier_batch(name, counts)
    want = fc.exact_inlier_yardstick(name, "TRUNCATED_CAUCHY", fm.STAGE_INLIERS, counts)
    assert [w["initial_inliers"] for w in want] == list(counts) and [w["refinements"] for w in want] == [0, 1]
    assert min(fc.threshold_margin(kind, w) for w in want) > 1e-6
    ro, bo = fc.library_options(name, "TRUNCATED_CAUCHY", capi)
    c1, c2 = fc.camera_records(b, capi)
    models = capi.array_to_models(b["models"])
    res, mask, score0, inl0 = handle.refine_batch(kind, b["x1"], b["x2"], b["d1"], b["d2"], models, ro, bo, fm.STAGE_INLIERS, b["n"], c1, c2)
    for i, w in enumerate(want):
        print(name, counts[i], "inliers", int(res[i]["num_inliers"]), int(inl0[i]), "LMs", int(res[i]["refinements"]), w["refinements"])
        assert int(inl0[i]) == counts[i] == int(res[i]["num_inliers"]) == int(mask[i].sum()) and np.array_equal(mask[i], w["mask"]), (name, i)
        assert int(res[i]["refinements"]) == w["refinements"] == (0 if counts[i] == rule else 1), (name, i)
        got = capi.model_to_array(res[i]["model"])
        assert helpers.same_model(got, w["model"]), (name, i, got, w["model"])
    assert res[0]["model"].tobytes() == models[0].tobytes()  # no LM ran: bit for bit


def _torch_batch(name, first, B, N):
    import torch
    from mdrp_amd import synth
    kind, es, rf = helpers.OPTIONS_KINDS[name]
    pairs = [synth.make_pair(first + i, N, noise_px=0.5, depth_noise=0.02, outlier_frac=0.3, random_focal=rf, shift1=0.2 if es else 0.0, shift2=-0.1 if es else 0.0)
             for i in range(B)]
    host = {k: np.ascontiguousarray(np.stack([p[k] for p in pairs])) for k in ("x1", "x2", "d1", "d2")}
    dev = torch.device("cuda", 0)
    return pairs, host, [torch.from_numpy(host[k]).to(dev) for k in ("x1", "x2", "d1", "d2")]


KIND_NAMES = {0: "calibrated", 1: "shared_focal", 2: "varying_focal"}
CAM = {"model": "SIMPLE_PINHOLE", "width": 1600, "height": 1200, "params": [800.0, 0.0, 0.0]}


@pytest.mark.parametrize("name", helpers.OPTIONS_NAMES)
def test_anchor_to_the_estimator(capi, name):
    """On the device alone: the estimator's records R, verified with stages = 0, come back bit for bit with a deterministic mask and the oracle's inlier
    count for that model.  And the CPU anchor through the kernel: stages = INLIERS from the oracle's ransac<> winner is the oracle's estimate."""
    import mdrp_amd.poselib as poselib
    from oracle import pyorc as po
    kind, es, _ = helpers.OPTIONS_KINDS[name]
    B, N = 4, 300
    pairs, host, t = _torch_batch(name, 73000, B, N)
    rod = dict(max_iterations=1000, min_iterations=1000, max_epipolar_error=2.0, max_reproj_error=16.0, seed=3)
    ro = dict(rod, monodepth_estimate_shift=es)
    bo = {"loss_type": "TRUNCATED_CAUCHY"}
    cams = (CAM, CAM) if kind == 0 else (None, None)
    R, _ = poselib.estimate_batch_torch(KIND_NAMES[kind], *t, *cams, ro, bo)
    res, mask, initial = poselib.refine_batch_torch(KIND_NAMES[kind], *t, R["model"].copy(), *cams, ro, bo, stages=())
    res2, mask2, _ = poselib.refine_batch_torch(KIND_NAMES[kind], *t, R["model"].copy(), *cams, ro, bo, stages=0)
    assert res["model"].tobytes() == R["model"].tobytes() and res.tobytes() == res2.tobytes()
    assert np.array_equal(mask.cpu().numpy(), mask2.cpu().numpy())
    oro, obo = po.ransac_opt(estimate_shift=es, **rod), po.bundle_opt(max_iterations=100, loss_type=4, loss_scale=1.0, gradient_tol=1e-10)
    cam = po.cam_flat(0, [800.0, 0.0, 0.0]) if kind == 0 else None
    winners = np.zeros((B, 12))
    for i in range(B):
        q = fm.prep(kind, host["x1"][i], host["x2"][i], oro, obo, cam, cam)
        m = capi.model_to_array(R[i]["model"])
        m[10:12] /= q["norm"]
        _, cnt = fm.score(kind, m, q)
        assert int(res[i]["num_inliers"]) == cnt == int(initial["inliers"][i]) == int(mask[i].sum()) and int(res[i]["refinements"]) == 0, (name, i)
        assert cnt > 150
        ro_n = po.ransac_opt(**dict(rod, estimate_shift=es, max_epipolar_error=q["eps"], max_reproj_error=q["rep"], weight_sampson=q["ws"]))
        winners[i], _, _ = po.ransac(kind, q["a1"], q["a2"], host["d1"][i], host["d2"][i], ro_n)
        winners[i, 10:12] *= q["norm"]
    res, mask, _ = poselib.refine_batch_torch(KIND_NAMES[kind], *t, capi.array_to_models(winners), *cams, ro, bo, stages=("inliers",))
    for i in range(B):
        want, st, wmask = po.estimate(kind, host["x1"][i], host["x2"][i], host["d1"][i], host["d2"][i], oro, obo, cam, cam)
        assert helpers.same_model(capi.model_to_array(res[i]["model"]), want), (name, i)
        assert np.array_equal(mask[i].cpu().numpy(), wmask) and int(res[i]["num_inliers"]) == st.num_inliers, (name, i)


@pytest.mark.parametrize("name", helpers.OPTIONS_NAMES)
def test_a_pairs_record_does_not_depend_on_its_batch_or_its_path(capi, name):
    """alone, as element 0 and as element 5 of a batch of six, through host buffers and through device pointers: the same bytes"""
    import torch
    kind, es, _ = helpers.OPTIONS_KINDS[name]
    b = fc.batch(name, n_list=(300, 290, 150, 64, 7, 299), first=74000, start=(), amount=0.15)
    ro, bo = fc.library_options(name, "TRUNCATED_CAUCHY", capi)
    c1, c2 = fc.camera_records(b, capi)
    models = capi.array_to_models(b["models"])
    h = capi.Handle(0)

    def host(order):
        o = list(order)
        res, mask, s0, i0 = h.refine_batch(kind, b["x1"][o], b["x2"][o], b["d1"][o], b["d2"][o], models[o], ro, bo, 3, b["n"][o],
                                           None if c1 is None else c1[o], None if c2 is None else c2[o])
        return res, mask, s0, i0

    alone = host([0])
    first = host([0, 1, 2, 3, 4, 5])
    last = host([1, 2, 3, 4, 5, 0])
    assert int(alone[0][0]["num_inliers"]) > 50 and int(alone[0][0]["refinements"]) == 2
    for got, at in ((first, 0), (last, 5)):
        assert got[0][at].tobytes() == alone[0][0].tobytes() and np.array_equal(got[1][at], alone[1][0])
        assert got[2][at] == alone[2][0] and got[3][at] == alone[3][0]
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(b[k])).to(dev) for k in ("x1", "x2", "d1", "d2")}
    mt = torch.from_numpy(models.view(np.uint8).reshape(6, 96).copy()).to(dev)
    mask = torch.zeros((6, 300), dtype=torch.uint8, device=dev)
    s0 = torch.zeros(6, dtype=torch.float64, device=dev)
    i0 = torch.zeros(6, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    h.refine_batch_device(kind, t["x1"].data_ptr(), t["x2"].data_ptr(), t["d1"].data_ptr(), t["d2"].data_ptr(), 6, 300, mt.data_ptr(), ro, bo, 3, b["n"], c1, c2,
                          mask.data_ptr(), s0.data_ptr(), i0.data_ptr())
    res = h.fetch_results(6)
    assert res.tobytes() == first[0].tobytes() and np.array_equal(mask.cpu().numpy(), first[1])
    assert np.array_equal(s0.cpu().numpy(), first[2]) and np.array_equal(i0.cpu().numpy(), first[3])
    h.close()


def test_boundary_of_the_entry_points(capi):
    """what is refused (before any device work) and what is not; the caller's device; the handle's buffers"""
    import torch
    b = fc.batch("calib_p3p", n_list=(300, 200), first=75000, start=(), amount=0.15)
    ro, bo = fc.library_options("calib_p3p", "TRUNCATED_CAUCHY", capi)
    c1, c2 = fc.camera_records(b, capi)
    models = capi.array_to_models(b["models"])
    h = capi.Handle(0)
    args = (b["x1"], b["x2"], b["d1"], b["d2"])
    for kind in (capi.RELPOSE_5PT, capi.SHARED_6PT, capi.FUNDAMENTAL_7PT, 17, -1):
        with pytest.raises(capi.MdrpError, match="mdrp error 1"):
            h.refine_batch(kind, *args, models, ro, bo, 3, b["n"], c1, c2)
    for stages in (4, -1):
        with pytest.raises(capi.MdrpError, match="mdrp error 1"):
            h.refine_batch(0, *args, models, ro, bo, stages, b["n"], c1, c2)
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.refine_batch(0, *args, None, ro, bo, 3, b["n"], c1, c2)
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.refine_batch(0, *args, models, ro, bo, 3, np.array([300, 301]), c1, c2)
    # an estimator call on the same handle returns the same bytes before and after a refine call (the handle's buffers are shared)
    ero = capi.ransac_opt_from_dict(dict(fc.RO, max_iterations=1000, min_iterations=1000))
    h.estimate_batch(0, *args, ero, bo, b["n"], c1, c2)
    before = h.estimate_batch(0, *args, ero, bo, b["n"], c1, c2)
    # progressive_sampling selects a sampler; nothing samples here, so it is not refused
    prosac = capi.ransac_opt_from_dict(dict(fc.RO, progressive_sampling=True))
    with pytest.raises(NotImplementedError):
        h.estimate_batch(0, *args, prosac, bo, b["n"], c1, c2)
    plain = h.refine_batch(0, *args, models, ro, bo, 3, b["n"], c1, c2)
    cur = torch.cuda.device_count() - 1  # (the last device: another one than the handle's where the machine has several)
    torch.cuda.set_device(cur)
    try:
        got = h.refine_batch(0, *args, models, prosac, bo, 3, b["n"], c1, c2)
        assert torch.cuda.current_device() == cur
    finally:
        torch.cuda.set_device(0)
    assert got[0].tobytes() == plain[0].tobytes() and np.array_equal(got[1], plain[1]) and int(plain[0][0]["num_inliers"]) > 100
    after = h.estimate_batch(0, *args, ero, bo, b["n"], c1, c2)
    assert after[0].tobytes() == before[0].tobytes() and np.array_equal(after[1], before[1])
    h.close()


def test_default_stream_orders_with_a_producer_of_the_models(capi):
    """refine_batch_torch on torch's default stream, the models written by a torch op queued just before the call behind a chain of matrix products:
    the records are those of models that were there all along"""
    import torch
    import mdrp_amd.poselib as poselib
    b = fc.batch("shared", n_list=(300, 200, 250, 120), first=76000, start=(), amount=0.15)
    dev = torch.device("cuda", 0)
    assert torch.cuda.current_stream(dev).cuda_stream == 0
    t = [torch.from_numpy(np.ascontiguousarray(b[k])).to(dev) for k in ("x1", "x2", "d1", "d2")]
    ro, bo = dict(fc.RO), {"loss_type": "TRUNCATED_CAUCHY"}
    want, wmask, winit = poselib.refine_batch_torch("shared_focal", *t, capi.array_to_models(b["models"]), ransac_opt=ro, bundle_opt=bo, n_per_pair=b["n"])
    assert int(want["num_inliers"].min()) > 30
    src = torch.from_numpy(b["models"]).to(dev)              # (B, 12) float64: the records' layout
    out = torch.full_like(src, float("nan"))                 # the models do not exist yet: poison
    big = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize()
    junk = big
    for _ in range(20):                                      # queued work in front of the producer
        junk = junk @ big
        junk = junk / junk.abs().max()
    torch.add(src, (junk[0, 0] * 0.0).double(), out=out)     # asynchronous producer of the models, data dependent on the chain
    res, mask, init = poselib.refine_batch_torch("shared_focal", *t, out, ransac_opt=ro, bundle_opt=bo, n_per_pair=b["n"])
    assert res.tobytes() == want.tobytes() and np.array_equal(mask.cpu().numpy(), wmask.cpu().numpy())
    assert np.array_equal(init["score"], winit["score"]) and np.array_equal(init["inliers"], winit["inliers"])


def test_the_drop_in_functions(capi):
    """the single-pair and list forms return the estimators' objects and info keys plus the start model's score and count"""
    import mdrp_amd.poselib as poselib
    b = fc.batch("calib_p3p", n_list=(300,), first=75000, start=(), amount=0.15)
    ro, bo = dict(fc.RO), {"loss_type": "TRUNCATED_CAUCHY"}
    cam1 = {"model": "SIMPLE_PINHOLE", "width": 1600, "height": 1200, "params": list(b["cams"][0][1])}
    cam2 = {"model": "PINHOLE", "width": 1600, "height": 1200, "params": list(b["cams"][1][1])}
    m = b["models"][0]
    g0 = poselib.MonoDepthTwoViewGeometry(poselib.CameraPose(m[:4], m[4:7]), m[7], m[8], m[9])
    g, info = poselib.refine_monodepth_relative_pose(b["x1"][0], b["x2"][0], b["d1"][0], b["d2"][0], cam1, cam2, ro, bo, g0)
    want = fc.yardstick("calib_p3p", "TRUNCATED_CAUCHY", 3, n_list=(300,), first=75000, start=(), amount=0.15)[0]
    assert helpers.same_model(np.r_[g.pose.q, g.pose.t, g.scale, g.shift1, g.shift2, 1.0, 1.0], want["model"])
    assert set(info) == {"refinements", "iterations", "num_inliers", "inlier_ratio", "model_score", "inliers", "initial_score", "initial_inliers"}
    assert info["num_inliers"] == want["num_inliers"] == sum(info["inliers"]) and info["initial_inliers"] == want["initial_inliers"] and info["refinements"] == 2
    with pytest.raises(ValueError):
        poselib.refine_monodepth_relative_pose(b["x1"][0], b["x2"][0], b["d1"][0], b["d2"][0], cam1, cam2, ro, bo)
    s = fc.batch("varying", n_list=(300, 200), first=76000, start=(), amount=0.15)
    pairs0 = [poselib.MonoDepthImagePair(poselib.MonoDepthTwoViewGeometry(poselib.CameraPose(v[:4], v[4:7]), v[7], v[8], v[9]),
                                         poselib.Camera("SIMPLE_PINHOLE", [v[10], 0.0, 0.0]), poselib.Camera("SIMPLE_PINHOLE", [v[11], 0.0, 0.0])) for v in s["models"]]
    x1, x2, d1, d2 = ([s[k][i, :n] for i, n in enumerate(s["n"])] for k in ("x1", "x2", "d1", "d2"))
    out, infos = poselib.refine_monodepth_varying_focal_relative_pose_batch(x1, x2, d1, d2, pairs0, ro, bo, stages=("lo",))
    want = fc.yardstick("varying", "TRUNCATED_CAUCHY", 1, n_list=(300, 200), first=76000, start=(), amount=0.15)
    for i in range(2):
        q = out[i]
        got = np.r_[q.geometry.pose.q, q.geometry.pose.t, q.geometry.scale, q.geometry.shift1, q.geometry.shift2, q.camera1.focal(), q.camera2.focal()]
        assert helpers.same_model(got, want[i]["model"]) and infos[i]["num_inliers"] == want[i]["num_inliers"] and len(infos[i]["inliers"]) == s["n"][i]
