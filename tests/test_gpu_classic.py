"""Non-monodepth baselines on the GPU, through the C ABI / the drop-in module: 5-point relative pose and
7-point fundamental matrix against tests/golden/classic.npz (reference binary) and against the CPU oracle."""
import numpy as np
import pytest

from oracle import pyorc as po
from test_oracle_classic import (WIDE_CLASSIC, check_solver_lists, classic_cam, est_cases, fund_diff, pose_diff, sample_residual,
                                 wide_classic_digest, wide_classic_pair)

pytestmark = pytest.mark.gpu


def model_row(kind, m):
    """C-ABI model record -> flat vector comparable with the fixtures (pose: q, t; fundamental: nine entries)"""
    return np.r_[m["q"], m["t"]] if kind == 3 else np.r_[m["q"], m["t"], m["scale"], m["shift1"]]


@pytest.mark.parametrize("kind", [3, 5])
def test_solver_lists_equal_reference_in_order(golden, kind):
    from mdrp_amd import _capi
    h = _capi.default_handle(0)

    def solve(a, b):
        out, n = h.classic_solver_batch(kind, a[None], b[None])
        return np.array([model_row(kind, m) for m in out[0][:n[0]]]).reshape(-1, 7 if kind == 3 else 9)

    check_solver_lists(kind, golden("classic"), solve)


def test_solvers_equal_oracle_on_random_samples():
    from mdrp_amd import _capi
    h = _capi.default_handle(0)
    rng = np.random.default_rng(12)

    def unit(x):
        hh = np.concatenate([x, np.ones(x.shape[:-1] + (1,))], axis=-1)
        return np.ascontiguousarray(hh / np.linalg.norm(hh, axis=-1, keepdims=True))

    for kind, K in ((3, 5), (5, 7)):
        x1 = rng.uniform(-1, 1, (3000, K, 2))
        x2 = x1 + rng.normal(size=x1.shape) * np.where(np.arange(3000) % 2, 0.1, 1.0)[:, None, None]
        a, b = unit(x1), unit(x2)
        out, n = h.classic_solver_batch(kind, a, b)
        bad = loose = 0
        for i in range(3000):
            ref = po.relpose_5pt(a[i], b[i]) if kind == 3 else po.relpose_7pt(a[i], b[i]).reshape(-1, 9)
            if len(ref) != n[i]:
                bad += 1      # a root at the edge of existence (double root): the count may differ under FMA contraction
                continue
            for k in range(n[i]):
                row = model_row(kind, out[i][k])
                d = pose_diff(row, ref[k]) if kind == 3 else fund_diff(row, ref[k])
                if d > 1e-6:  # an ill-conditioned sample (a nearly double root: the oracle's own residual on the sample is large too)
                    loose += 1
                    res, res_orc = sample_residual(kind, row, a[i], b[i]), sample_residual(kind, ref[k], a[i], b[i])
                    assert kind == 3 and d < 0.1 and res < max(100.0 * res_orc, 1e-8), (kind, i, k, d, res, res_orc)
        assert bad <= 3 and loose <= 15, (kind, bad, loose)


def test_refine_equals_reference(golden):
    from mdrp_amd import _capi
    h = _capi.default_handle(0)
    g = golden("classic")
    for i, kind, loss, its in g["refine_cases"]:
        kind = int(kind)
        bo = _capi.bundle_opt_from_dict({"max_iterations": int(its), "loss_scale": 0.004})
        bo.loss_type = int(loss)
        m0 = g[f"refine_m0_{i}"]
        rec = np.zeros(1, dtype=_capi.MODEL_DTYPE)
        if kind == 3:
            rec["q"] = m0[:4]; rec["t"] = m0[4:7]; rec["scale"] = 1.0; rec["f1"] = rec["f2"] = 1.0
        else:
            rec[0] = _capi.fundamental_to_model(m0.reshape(3, 3))
        out, cost = h.refine_models(kind, rec, g[f"refine_x1_{i}"], g[f"refine_x2_{i}"], None, None, 0.0, 1.0, bo)
        ref, rst = g[f"refine_m_{i}"], g[f"refine_stats_{i}"]
        d = pose_diff(model_row(3, out[0]), ref) if kind == 3 else fund_diff(model_row(5, out[0]), ref)
        assert d < 1e-6, (i, kind, loss, its, d)          # north_star tolerance; trajectories agree to ~1e-9 in practice
        assert cost[0] == pytest.approx(rst[2], rel=1e-6, abs=1e-18)


def run_case(poselib, g, i, kind, its, min_its, loss, thr, seed, f):
    ro = {"max_iterations": its, "min_iterations": min_its, "max_epipolar_error": thr, "seed": seed}
    names = {0: "TRIVIAL", 1: "TRUNCATED", 2: "HUBER", 3: "CAUCHY", 4: "TRUNCATED_CAUCHY", 5: "TRUNCATED_LE_ZACH"}
    bo = {"loss_type": names[loss], "loss_scale": thr}
    if kind == 3:
        cam1 = {"model": "SIMPLE_PINHOLE", "width": 1280, "height": 960, "params": [f, 640.0, 480.0]}
        cam2 = {"model": "PINHOLE", "width": 1280, "height": 960, "params": [f * 1.01, f * 0.99, 640.0, 480.0]}
        pose, info = poselib.estimate_relative_pose(g[f"est_x1_{i}"], g[f"est_x2_{i}"], cam1, cam2, ro, bo)
        return np.r_[pose.q, pose.t], info
    F, info = poselib.estimate_fundamental(g[f"est_x1_{i}"], g[f"est_x2_{i}"], ro, bo)
    return F.reshape(-1), info


def test_estimators_equal_reference_golden(golden):
    """every fixture of the reference binary's estimate_relative_pose / estimate_fundamental, incl. the two BASELINE-sized ones
    (N = 2000, 10^4 iterations), through the drop-in signatures: refinements, iterations, inliers, score, mask, model"""
    import mdrp_amd.poselib as poselib
    g = golden("classic")
    for i, kind, n, its, min_its, loss, thr, seed, f in est_cases(g):
        m, info = run_case(poselib, g, i, kind, its, min_its, loss, thr, seed, f)
        rst = g[f"est_stats_{i}"]
        assert (info["refinements"], info["iterations"], info["num_inliers"]) == tuple(int(v) for v in rst[:3]), (i, kind, info["refinements"], info["iterations"], info["num_inliers"], rst)
        assert info["model_score"] == pytest.approx(rst[4], rel=1e-9)
        assert np.array_equal(np.array(info["inliers"], dtype=np.uint8), g[f"est_mask_{i}"]), (i, kind)
        d = pose_diff(m, g[f"est_model_{i}"]) if kind == 3 else fund_diff(m, g[f"est_model_{i}"])
        assert d < 1e-6, (i, kind, d)


@pytest.mark.parametrize("kind", [3, 5])
def test_batches_follow_the_oracle_trajectory(kind):
    """noisy pairs with outliers, ragged sizes, batched: every pair must land on the sequential oracle's exact trajectory"""
    import mdrp_amd.poselib as poselib
    from mdrp_amd import synth
    pairs = [synth.make_pair(8800 + 7 * k, [200, 350, 120, 500][k % 4], f1=900.0, f2=900.0, pp=(640.0, 480.0), noise_px=0.7,
                             outlier_frac=[0.3, 0.5, 0.15, 0.4][k % 4]) for k in range(24)]
    ro = {"max_iterations": 800, "min_iterations": 100, "max_epipolar_error": 1.5, "seed": 2}
    bo = {"loss_type": "TRUNCATED_CAUCHY", "loss_scale": 1.5}
    x1, x2 = [p["x1"] for p in pairs], [p["x2"] for p in pairs]
    cam = {"model": "SIMPLE_PINHOLE", "width": 1280, "height": 960, "params": [900.0, 640.0, 480.0]}
    if kind == 3:
        models, infos = poselib.estimate_relative_pose_batch(x1, x2, cam, cam, ro, bo)
        models = [np.r_[m.q, m.t] for m in models]
    else:
        models, infos = poselib.estimate_fundamental_batch(x1, x2, ro, bo)
    off = 0
    for k, p in enumerate(pairs):
        c = po.cam_flat(0, [900.0, 640.0, 480.0])
        m, st, mask = po.estimate_classic(kind, p["x1"], p["x2"], po.ransac_opt(max_iterations=800, min_iterations=100, max_epipolar_error=1.5, seed=2),
                                          po.bundle_opt(loss_type=4, loss_scale=1.5), c, c)
        info = infos[k]
        same = (info["refinements"], info["iterations"], info["num_inliers"]) == (st.refinements, st.iterations, st.num_inliers) and \
            np.array_equal(np.array(info["inliers"], dtype=np.uint8), mask)
        if not same:
            off += 1
            continue
        assert info["model_score"] == pytest.approx(st.model_score, rel=1e-9)
        d = pose_diff(models[k], m) if kind == 3 else fund_diff(np.asarray(models[k]).reshape(-1), m)
        assert d < 1e-6, (k, d)
    assert off == 0, off


def test_too_few_correspondences_and_ragged_batch():
    import mdrp_amd.poselib as poselib
    from mdrp_amd import synth
    p = synth.make_pair(8700, 300, f1=900.0, f2=900.0, noise_px=0.5, outlier_frac=0.3)
    cam = {"model": "SIMPLE_PINHOLE", "width": 1280, "height": 960, "params": [900.0, 0.0, 0.0]}
    ro = {"max_iterations": 300, "min_iterations": 300, "max_epipolar_error": 1.5}
    x1 = [p["x1"], p["x1"][:4], p["x1"][:6], p["x1"][:0]]
    x2 = [p["x2"], p["x2"][:4], p["x2"][:6], p["x2"][:0]]
    poses, infos = poselib.estimate_relative_pose_batch(x1, x2, cam, cam, ro, {})
    assert infos[0]["num_inliers"] > 150 and infos[1]["iterations"] == 0 and infos[3]["iterations"] == 0
    assert infos[2]["iterations"] == 300 and len(infos[2]["inliers"]) == 6
    Fs, infos = poselib.estimate_fundamental_batch(x1, x2, ro, {})
    assert infos[0]["num_inliers"] > 150 and infos[1]["iterations"] == 0 and infos[2]["iterations"] == 0 and infos[3]["iterations"] == 0
    single, info1 = poselib.estimate_relative_pose(p["x1"], p["x2"], cam, cam, ro, {})
    assert info1["num_inliers"] == poselib.estimate_relative_pose_batch(x1[:1], x2[:1], cam, cam, ro, {})[1][0]["num_inliers"]


def test_initial_pose_through_the_drop_in_signature(golden):
    """estimate_relative_pose(..., initial_pose=...): the pose handed in is never read (ransac_relpose resets it), the reset model is
    scored first: refinements + 1 — fixtures from the reference binary with score_initial_model"""
    import mdrp_amd.poselib as poselib
    g = golden("classic")
    cam = {"model": "SIMPLE_PINHOLE", "width": 1280, "height": 960, "params": [800.0, 640.0, 480.0]}
    for i, n, its, min_its, seed in g["init_cases"]:
        ini = g[f"init_pose_{i}"]
        ro = {"max_iterations": int(its), "min_iterations": int(min_its), "max_epipolar_error": 2.0, "seed": int(seed)}
        pose, info = poselib.estimate_relative_pose(g[f"init_x1_{i}"], g[f"init_x2_{i}"], cam, cam, ro, {"loss_type": "TRUNCATED_CAUCHY", "loss_scale": 2.0},
                                                    initial_pose=poselib.CameraPose(ini[:4], ini[4:7]))
        rst = g[f"init_stats_{i}"]
        assert (info["refinements"], info["iterations"], info["num_inliers"]) == tuple(int(v) for v in rst[:3]), (i, info["refinements"], rst)
        assert np.array_equal(np.array(info["inliers"], dtype=np.uint8), g[f"init_mask_{i}"])
        assert pose_diff(np.r_[pose.q, pose.t], g[f"init_model_{i}"]) < 1e-6


@pytest.mark.timeout(180)
def test_garbage_inputs_terminate():
    """NaN / inf coordinates, one correspondence repeated N times, collinear points, absurd scales: the solvers' loops (full
    pivoting, LU, Sturm isolation, root polishing, LM) must terminate and leave the healthy pair beside them untouched"""
    from mdrp_amd import _capi, synth
    h = _capi.default_handle(0)
    b = synth.make_batch(8600, 6, 300, f1=900.0, f2=900.0, noise_px=0.5, outlier_frac=0.3)
    x1, x2 = b["x1"].copy(), b["x2"].copy()
    x1[0, ::7] = np.nan; x2[0, ::5] = np.inf
    x1[1] = x1[1, :1]; x2[1] = x2[1, :1]                                    # one correspondence repeated 300 times
    x1[2] *= 1e12; x2[2] *= 1e-12                                           # absurd scales
    t = np.linspace(-400, 400, 300)
    x1[3] = np.c_[t, 0.5 * t]; x2[3] = np.c_[t + 3.0, 0.5 * t + 1.0]        # all points on one line in both images
    x1[4] = 0.0; x2[4] = 0.0                                                # everything at the principal point
    cams = np.zeros(6, dtype=_capi.CAMERA_DTYPE); cams["params"][:, 0] = 900.0
    for kind in (_capi.RELPOSE_5PT, _capi.FUNDAMENTAL_7PT):
        ro = _capi.ransac_opt_from_dict({"max_iterations": 600, "min_iterations": 300, "max_epipolar_error": 1.5})
        res, mask = h.estimate_batch(kind, x1, x2, None, None, ro, _capi.bundle_opt_from_dict({"loss_type": "TRUNCATED_CAUCHY"}), None,
                                     cams if kind == _capi.RELPOSE_5PT else None, cams if kind == _capi.RELPOSE_5PT else None)
        assert (res["iterations"] >= 301).all() and (res["iterations"] <= 600).all(), res["iterations"]
        assert (res["num_inliers"] <= 300).all()
        assert int(res[5]["num_inliers"]) > 150   # the clean pair next to them is unaffected


@pytest.mark.parametrize("kind", [3, 5])
def test_stress_grid_follows_the_oracle(kind):
    """shapes x outlier rates x thresholds x dynamic / fixed stopping, 6 pairs each: every pair on the sequential oracle's trajectory"""
    import mdrp_amd.poselib as poselib
    from mdrp_amd import synth
    off = total = 0
    for gi, (n, outl, thr, its, min_its) in enumerate([(80, 0.2, 1.0, 400, 400), (600, 0.6, 2.0, 1500, 50), (1500, 0.4, 0.75, 700, 700),
                                                       (250, 0.0, 1.5, 300, 20), (2500, 0.5, 1.0, 1200, 1200)]):
        pairs = [synth.make_pair(8900 + 31 * gi + k, n, f1=1000.0, f2=1000.0, pp=(640.0, 480.0), noise_px=0.5, outlier_frac=outl) for k in range(6)]
        ro = {"max_iterations": its, "min_iterations": min_its, "max_epipolar_error": thr, "seed": gi}
        bo = {"loss_type": "TRUNCATED_CAUCHY", "loss_scale": thr}
        cam = {"model": "SIMPLE_PINHOLE", "width": 1280, "height": 960, "params": [1000.0, 640.0, 480.0]}
        x1, x2 = np.stack([p["x1"] for p in pairs]), np.stack([p["x2"] for p in pairs])
        if kind == 3:
            models, infos = poselib.estimate_relative_pose_batch(x1, x2, cam, cam, ro, bo)
            models = [np.r_[m.q, m.t] for m in models]
        else:
            models, infos = poselib.estimate_fundamental_batch(x1, x2, ro, bo)
        c = po.cam_flat(0, [1000.0, 640.0, 480.0])
        for k, p in enumerate(pairs):
            m, st, mask = po.estimate_classic(kind, p["x1"], p["x2"], po.ransac_opt(max_iterations=its, min_iterations=min_its, max_epipolar_error=thr, seed=gi),
                                              po.bundle_opt(loss_type=4, loss_scale=thr), c, c)
            info = infos[k]
            total += 1
            same = (info["refinements"], info["iterations"], info["num_inliers"]) == (st.refinements, st.iterations, st.num_inliers) and \
                np.array_equal(np.array(info["inliers"], dtype=np.uint8), mask)
            if not same:
                off += 1
                continue
            d = pose_diff(models[k], m) if kind == 3 else fund_diff(np.asarray(models[k]).reshape(-1), m)
            assert d < 1e-6, (gi, k, d)
    assert off == 0, (off, total)


@pytest.mark.parametrize("kind", [3, 5])
def test_large_batch_one_wavefront_per_lo_problem(kind):
    """>= 128 pairs switch the LO kernels to one wavefront per LM problem (T = 64): same trajectories as the sequential oracle"""
    import mdrp_amd.poselib as poselib
    from mdrp_amd import synth
    B = 136
    pairs = [synth.make_pair(9100 + k, 100 + (k % 5) * 20, f1=850.0, f2=850.0, pp=(640.0, 480.0), noise_px=0.6, outlier_frac=0.35) for k in range(B)]
    ro = {"max_iterations": 250, "min_iterations": 60, "max_epipolar_error": 1.5, "seed": 4}
    bo = {"loss_type": "TRUNCATED_CAUCHY", "loss_scale": 1.5}
    cam = {"model": "SIMPLE_PINHOLE", "width": 1280, "height": 960, "params": [850.0, 640.0, 480.0]}
    x1, x2 = [p["x1"] for p in pairs], [p["x2"] for p in pairs]
    if kind == 3:
        models, infos = poselib.estimate_relative_pose_batch(x1, x2, cam, cam, ro, bo)
        models = [np.r_[m.q, m.t] for m in models]
    else:
        models, infos = poselib.estimate_fundamental_batch(x1, x2, ro, bo)
    c = po.cam_flat(0, [850.0, 640.0, 480.0])
    off = 0
    for k, p in enumerate(pairs):
        m, st, mask = po.estimate_classic(kind, p["x1"], p["x2"], po.ransac_opt(max_iterations=250, min_iterations=60, max_epipolar_error=1.5, seed=4),
                                          po.bundle_opt(loss_type=4, loss_scale=1.5), c, c)
        info = infos[k]
        same = (info["refinements"], info["iterations"], info["num_inliers"]) == (st.refinements, st.iterations, st.num_inliers) and \
            np.array_equal(np.array(info["inliers"], dtype=np.uint8), mask)
        if not same:
            off += 1
            continue
        d = pose_diff(models[k], m) if kind == 3 else fund_diff(np.asarray(models[k]).reshape(-1), m)
        assert d < 1e-6, (k, d)
    assert off == 0, off


@pytest.mark.parametrize("kind", [3, 4, 5])
def test_fused_tail_is_bit_identical(kind, monkeypatch):
    """The fused tail of the baselines (kc_lo replays a pair when its last trigger is refined, kc_final starts from the ready
    list while the LO drains) against LO | k_walk | kc_final one after the other: records and masks bit for bit."""
    import mdrp_amd.poselib as poselib
    from mdrp_amd import synth
    B = 150 if kind != 4 else 96  # (the 6-point solver is two orders of magnitude slower: fewer pairs and iterations, still > 64 LO problems)
    pairs = [synth.make_pair(9700 + k, [300, 200, 4, 120][k % 4] if k % 5 == 0 else 300, f1=850.0, f2=850.0, pp=(640.0, 480.0), noise_px=0.6,
                             outlier_frac=[0.4, 0.1][k % 2]) for k in range(B)]
    its = 1500 if kind != 4 else 400
    ro = {"max_iterations": its, "min_iterations": its, "max_epipolar_error": 1.5, "seed": 2}
    bo = {"loss_type": "TRUNCATED_CAUCHY", "loss_scale": 1.5}
    cam = {"model": "SIMPLE_PINHOLE", "width": 1280, "height": 960, "params": [850.0, 640.0, 480.0]}
    x1, x2 = [p["x1"] for p in pairs], [p["x2"] for p in pairs]
    out = []
    for fuse in ("0", "1"):
        monkeypatch.setenv("MDRP_FUSE_TAIL", fuse)
        if kind == 3:
            models, infos = poselib.estimate_relative_pose_batch(x1, x2, cam, cam, ro, bo)
            models = [np.r_[m.q, m.t] for m in models]
        elif kind == 4:
            models, infos = poselib.estimate_shared_focal_relative_pose_batch(x1, x2, (640.0, 480.0), ro, bo)
            models = [np.r_[m.pose.q, m.pose.t, m.camera1.params[0]] for m in models]
        else:
            models, infos = poselib.estimate_fundamental_batch(x1, x2, ro, bo)
            models = [np.asarray(m).reshape(-1) for m in models]
        out.append((models, infos))
    (m0, i0), (m1, i1) = out
    for k in range(B):
        assert np.array_equal(m0[k], m1[k]), k
        assert (i0[k]["refinements"], i0[k]["iterations"], i0[k]["num_inliers"], i0[k]["model_score"]) == \
            (i1[k]["refinements"], i1[k]["iterations"], i1[k]["num_inliers"], i1[k]["model_score"]), k
        assert np.array_equal(np.array(i0[k]["inliers"]), np.array(i1[k]["inliers"])), k
    assert max(i["refinements"] for i in i0) > 3


@pytest.mark.parametrize("lanes", ["64", "256"])
def test_fused_tail_is_bit_identical_at_both_lane_counts(lanes, monkeypatch):
    """MDRP_FUSE_TAIL = 0 against 1 with MDRP_LO_THREADS = MDRP_FINAL_THREADS = 64 and 256 for the 5-point baseline (kc_lo / kc_final at either width, the
    pair taken from the ready list or by its index): records and masks bit for bit.  Eight small pairs, one with four records beside one with five."""
    from mdrp_amd import _capi, synth
    ns = [64, 60, 5, 4, 33, 64, 64, 50]
    B, N = len(ns), 64
    pairs = [synth.make_pair(9750 + k, n, f1=850.0, f2=850.0, pp=(640.0, 480.0), noise_px=0.6, outlier_frac=[0.4, 0.1][k % 2]) for k, n in enumerate(ns)]
    n_per = np.array(ns, dtype=np.int32)
    x1, x2 = np.zeros((B, N, 2)), np.zeros((B, N, 2))
    for k, p in enumerate(pairs):
        x1[k, : ns[k]], x2[k, : ns[k]] = p["x1"], p["x2"]
    cams = np.zeros(B, dtype=_capi.CAMERA_DTYPE)  # SIMPLE_PINHOLE
    cams["params"][:, :3] = (850.0, 640.0, 480.0)
    ro = _capi.ransac_opt_from_dict({"max_iterations": 256, "min_iterations": 256, "max_epipolar_error": 1.5, "seed": 2})
    bo = _capi.bundle_opt_from_dict({"loss_type": "TRUNCATED_CAUCHY", "loss_scale": 1.5})
    monkeypatch.setenv("MDRP_LO_THREADS", lanes)
    monkeypatch.setenv("MDRP_FINAL_THREADS", lanes)
    h = _capi.Handle(0)  # (its own: an expired wait turns a handle's fused tail off for its next calls)
    try:
        out = []
        # "giveup", last: the fused tail's bounded waits cut to 1 us.  Only the fused tail's waits can expire, so a count above zero shows that this shape
        # at this width does take the fused path, which no other statistic tells apart (tests/test_gpu_wide.py does the same for k_lo / k_final)
        for fuse in ("0", "1", "giveup"):
            monkeypatch.setenv("MDRP_FUSE_TAIL", "0" if fuse == "0" else "1")
            for k in ("MDRP_FUSE_GATE_US", "MDRP_FUSE_WAIT_US"):
                monkeypatch.setenv(k, "1") if fuse == "giveup" else monkeypatch.delenv(k, raising=False)
            res, mask = h.estimate_batch(_capi.RELPOSE_5PT, x1, x2, None, None, ro, bo, n_per, cams, cams)
            assert (h.last_stats()["fuse_timeouts"] > 0) == (fuse == "giveup"), fuse
            out.append((res.copy(), mask.copy()))
        (r0, m0), (r1, m1), (r2, m2) = out
        print(lanes, "refinements", r0["refinements"].tolist(), "inliers", r0["num_inliers"].tolist())
        assert r0.tobytes() == r1.tobytes() and np.array_equal(m0, m1)
        assert r0.tobytes() == r2.tobytes() and np.array_equal(m0, m2)
        assert int(r0["refinements"].max()) > 1 and int(r0["refinements"][3]) == 0
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------- 6-point, shared focal
def _six_rows(out, n):
    return [np.r_[m["q"], m["t"], m["f1"]] for m in out[:n]]


def test_sixpt_solver_equals_oracle_and_reference(golden):
    """relpose_6pt_shared_focal on the device: on the 96 fixtures of tests/golden/sixpt.npz the same sets as the oracle (1e-6),
    hence every accurate solution of the reference binary (test_oracle_classic.py::test_sixpt_solution_sets_equal_reference);
    on 2000 random samples the same sets as the oracle up to eigenvalues at the edge of being real."""
    from mdrp_amd import _capi
    from test_oracle_classic import _same_sixpt, _sixpt_residual
    h = _capi.default_handle(0)
    g = golden("sixpt")
    out, n = h.classic_solver_batch(_capi.SHARED_6PT, g["solver_x1"], g["solver_x2"])
    edge = 0
    for i in range(len(n)):
        mine = _six_rows(out[i], n[i])
        ref = [np.r_[m[:7], m[10]] for m in po.relpose_6pt(g["solver_x1"][i], g["solver_x2"][i])]
        for u in mine:
            if any(_same_sixpt(u, v, 1e-6) for v in ref):
                assert _sixpt_residual(u, g["solver_x1"][i], g["solver_x2"][i]) < 1e-8, (i, u[7])
        matched = sum(any(_same_sixpt(u, v, 1e-6) for u in mine) for v in ref)
        if len(mine) != len(ref) or matched != len(ref):
            # a pair of eigenvalues at the edge of being real (a nearly double root): real on one side, complex or merged on the
            # other under FMA contraction; the well separated solutions still agree
            edge += 1
            assert abs(len(mine) - len(ref)) <= 2 and matched >= len(ref) - 2, (i, [u[7] for u in mine], [v[7] for v in ref])
    assert edge <= 4, edge
    rng = np.random.default_rng(5)

    def unit(x):
        hh = np.concatenate([x, np.ones(x.shape[:-1] + (1,))], axis=-1)
        return np.ascontiguousarray(hh / np.linalg.norm(hh, axis=-1, keepdims=True))

    x1 = rng.uniform(-1, 1, (2000, 6, 2))
    x2 = x1 + rng.normal(size=x1.shape) * np.where(np.arange(2000) % 2, 0.1, 1.0)[:, None, None]
    a, b = unit(x1), unit(x2)
    out, n = h.classic_solver_batch(_capi.SHARED_6PT, a, b)
    bad = loose = 0
    for i in range(2000):
        ref = [np.r_[m[:7], m[10]] for m in po.relpose_6pt(a[i], b[i])]
        mine = _six_rows(out[i], n[i])
        if len(ref) != len(mine):
            bad += 1
            continue
        loose += sum(not _same_sixpt(u, v, 1e-6) for u, v in zip(mine, ref))
    assert bad <= 20 and loose <= 20, (bad, loose)


def test_sixpt_estimator_equals_reference_golden(golden):
    """estimate_shared_focal_relative_pose through the drop-in signature: the 24 small reference-binary runs one by one (every
    loss type, fixed and dynamic stopping, with and without a principal point) and the 8 full-size ones (N = 2000, 10^4 iterations,
    50 % outliers) as one batch: iterations, inlier count, mask, pose, focal length; the LO count within one of the
    reference's (its solver's solution ORDER is not reproduced)."""
    import mdrp_amd.poselib as poselib
    from mdrp_amd import synth
    g = golden("sixpt")
    names = {0: "TRIVIAL", 1: "TRUNCATED", 2: "HUBER", 3: "CAUCHY", 4: "TRUNCATED_CAUCHY", 5: "TRUNCATED_LE_ZACH"}
    lo_dev = 0

    def check(pair, info, ref_m, ref_st, ref_mask, where):
        nonlocal lo_dev
        assert info["iterations"] == int(ref_st[1]) and info["num_inliers"] == int(ref_st[2]), (where, info["iterations"], info["num_inliers"], ref_st)
        assert np.array_equal(np.array(info["inliers"], dtype=np.uint8), ref_mask), where
        assert np.abs(pair.pose.R - po.quat_to_rotmat(ref_m[:4])).max() < 1e-6, where
        t, tr = pair.pose.t / np.linalg.norm(pair.pose.t), ref_m[4:7] / np.linalg.norm(ref_m[4:7])
        assert np.abs(t - tr).max() < 1e-6 and pair.camera1.focal() == pytest.approx(ref_m[7], rel=1e-6) and pair.camera2.focal() == pair.camera1.focal(), where
        assert abs(info["refinements"] - int(ref_st[0])) <= 1, (where, info["refinements"], ref_st[0])
        lo_dev += info["refinements"] != int(ref_st[0])

    for case in g["est_cases"]:
        k, n, its, min_its, loss, thr, seed = int(case[0]), int(case[1]), int(case[2]), int(case[3]), int(case[4]), float(case[5]), int(case[6])
        pp = np.array([float(case[7]), float(case[8])])
        ro = {"max_iterations": its, "min_iterations": min_its, "max_epipolar_error": thr, "seed": seed}
        pair, info = poselib.estimate_shared_focal_relative_pose(g[f"est_x1_{k}"], g[f"est_x2_{k}"], pp, ro, {"loss_type": names[loss], "loss_scale": thr})
        check(pair, info, g[f"est_model_{k}"], g[f"est_stats_{k}"], g[f"est_mask_{k}"], ("small", k))
    prs = [synth.make_pair(int(ix), 2000, noise_px=0.5, outlier_frac=0.5, random_focal="shared", pp=(0.0, 0.0)) for ix in g["full_indices"]]
    pairs, infos = poselib.estimate_shared_focal_relative_pose_batch(np.stack([p["x1"] for p in prs]), np.stack([p["x2"] for p in prs]), None,
                                                                     {"max_iterations": 10000, "min_iterations": 10000, "max_epipolar_error": 2.0},
                                                                     {"loss_type": "TRUNCATED_CAUCHY"})
    for j in range(len(prs)):
        check(pairs[j], infos[j], g["full_model"][j], g["full_stats"][j], np.unpackbits(g["full_mask"][j])[:2000], ("full", int(g["full_indices"][j])))
    assert lo_dev <= 4, lo_dev


def test_sixpt_batch_follows_the_oracle_trajectory():
    """24 ragged noisy pairs with outliers in one call: every pair on the sequential oracle's exact trajectory"""
    import mdrp_amd.poselib as poselib
    from mdrp_amd import synth
    pairs = [synth.make_pair(8900 + 7 * k, [200, 350, 120, 500][k % 4], pp=(0.0, 0.0), noise_px=0.7, outlier_frac=[0.3, 0.5, 0.15, 0.4][k % 4],
                             random_focal="shared") for k in range(24)]
    ro = {"max_iterations": 800, "min_iterations": 100, "max_epipolar_error": 1.5, "seed": 2}
    bo = {"loss_type": "TRUNCATED_CAUCHY", "loss_scale": 1.5}
    out, infos = poselib.estimate_shared_focal_relative_pose_batch([p["x1"] for p in pairs], [p["x2"] for p in pairs], None, ro, bo)
    oro = po.ransac_opt(max_iterations=800, min_iterations=100, max_epipolar_error=1.5, seed=2)
    for k, p in enumerate(pairs):
        m, st, mask = po.estimate_classic(4, p["x1"], p["x2"], oro, po.bundle_opt(loss_type=4, loss_scale=1.5), pp=(0.0, 0.0))
        info = infos[k]
        assert (info["refinements"], info["iterations"], info["num_inliers"]) == (st.refinements, st.iterations, st.num_inliers), (k, info["refinements"], st.refinements)
        assert np.array_equal(np.array(info["inliers"], dtype=np.uint8), mask), k
        assert np.abs(out[k].pose.R - po.quat_to_rotmat(m[:4])).max() < 1e-6 and out[k].camera1.focal() == pytest.approx(m[10], rel=1e-6), k


@pytest.mark.parametrize("name,kind", WIDE_CLASSIC)
def test_full_size_wide_vs_reference_binary(golden, name, kind):
    """The baselines at the benchmark shape (N = 2000, 10^4 iterations, 50 % outliers) as ONE batch against the reference binary's
    own outputs (tests/golden/classic_wide.npz: 32 / 16 / 32 pairs): iterations, inlier count, mask, model and score on every
    pair; the LO count equals the reference's, or the CPU port's on the one 6-point pair where that differs (solution order)."""
    import mdrp_amd.poselib as poselib
    g = golden("classic_wide")
    count = len(g[f"{name}_stats"])
    pairs = [wide_classic_pair(kind, j) for j in range(count)]
    for j, p in enumerate(pairs):
        assert wide_classic_digest(p) == g[f"{name}_digest"][j], "mdrp_amd.synth changed: regenerate tests/golden/classic_wide.npz"
    ro = {"max_iterations": 10000, "min_iterations": 10000, "max_epipolar_error": 2.0, "seed": 0}
    bo = {"loss_type": "TRUNCATED_CAUCHY"}
    cam = {"model": "SIMPLE_PINHOLE", "width": 1600, "height": 1200, "params": [800.0, 0.0, 0.0]}
    x1, x2 = [p["x1"] for p in pairs], [p["x2"] for p in pairs]
    if kind == 3:
        models, infos = poselib.estimate_relative_pose_batch(x1, x2, cam, cam, ro, bo)
        rows = [np.r_[m.q, m.t] for m in models]
    elif kind == 4:
        models, infos = poselib.estimate_shared_focal_relative_pose_batch(x1, x2, (0.0, 0.0), ro, bo)
        rows = [np.r_[m.pose.q, m.pose.t, m.camera1.params[0]] for m in models]
    else:
        models, infos = poselib.estimate_fundamental_batch(x1, x2, ro, bo)
        rows = [np.asarray(m).reshape(-1) for m in models]
    lo_dev = 0
    for j in range(count):
        ref_m, ref_st = g[f"{name}_model"][j], g[f"{name}_stats"][j]
        info = infos[j]
        assert (info["iterations"], info["num_inliers"]) == (int(ref_st[1]), int(ref_st[2])), (name, j)
        assert np.array_equal(np.array(info["inliers"], dtype=np.uint8), np.unpackbits(g[f"{name}_mask"][j])[:2000]), (name, j)
        assert abs(info["model_score"] - ref_st[4]) <= 1e-9 * abs(ref_st[4]), (name, j)
        d = fund_diff(rows[j], ref_m) if kind == 5 else pose_diff(rows[j], ref_m)
        assert d < 1e-6, (name, j, d)
        if kind == 4:
            assert abs(rows[j][7] - ref_m[7]) < 1e-6 * ref_m[7], (name, j)
        assert info["refinements"] in (int(ref_st[0]), int(g[f"{name}_oracle_refinements"][j])), (name, j, info["refinements"], ref_st[0])
        lo_dev += info["refinements"] != int(ref_st[0])
    assert lo_dev <= 1, lo_dev


def test_sixpt_cam2_may_be_null():
    """include/mdrp.h: MDRP_SHARED_6PT reads the principal point from cam1 and nothing from cam2 — a C caller may pass cam2 = NULL
    (the host side used to memcpy from it).  Same records and masks as with cam2 = cam1."""
    from mdrp_amd import _capi, synth
    B, N = 6, 300
    b = synth.make_batch(9100, B, N, noise_px=0.5, depth_noise=0.02, outlier_frac=0.3, random_focal="shared", pp=(12.0, -7.0))
    cams = np.zeros(B, dtype=_capi.CAMERA_DTYPE)
    cams["params"][:, 0] = 12.0; cams["params"][:, 1] = -7.0
    ro = _capi.ransac_opt_from_dict({"max_iterations": 300, "min_iterations": 300, "max_epipolar_error": 2.0})
    bo = _capi.bundle_opt_from_dict({"loss_type": "TRUNCATED_CAUCHY"})
    h = _capi.default_handle(0)
    r1, m1 = h.estimate_batch(_capi.SHARED_6PT, b["x1"], b["x2"], None, None, ro, bo, None, cams, cams)
    r2, m2 = h.estimate_batch(_capi.SHARED_6PT, b["x1"], b["x2"], None, None, ro, bo, None, cams, None)
    assert r1.tobytes() == r2.tobytes() and np.array_equal(m1, m2)
    assert int(r1["num_inliers"].min()) > 100


@pytest.mark.parametrize("name", ["relpose_5pt", "shared_6pt", "fundamental_7pt"])
def test_randomised_options_vs_reference_fixture(golden, name):
    """tests/golden/options_ref_classic.npz through the drop-in module's single-pair entry points (option dicts, Camera dicts): 64 cases per comparison row
    with size, outliers, noise, threshold, seed, budget (to 100 000 iterations), loss type / scale, bundle cap, cameras and principal point drawn at random.
    Iterations, inlier count and mask identical to the REFERENCE BINARY, model within 1e-6; LO count = the reference's or the oracle's where those differ
    (two enumerated 6-point cases); the one 6-point case where oracle and reference end on different winners must equal one of the two."""
    import mdrp_amd.poselib as poselib
    from mdrp_amd import _capi
    from helpers import (CLASSIC_OPTIONS_KINDS, CLASSIC_OPTIONS_LO_DEVIATIONS, CLASSIC_OPTIONS_OTHER_WINNER, classic_options_cameras, classic_options_pair)
    g = golden("options_ref_classic")
    kind = CLASSIC_OPTIONS_KINDS[name]
    loss_name = {v: k for k, v in _capi.LOSS_TYPES.items()}
    other = 0
    for j, row in enumerate(g["cases"]):
        n = int(row[0])
        p = classic_options_pair(name, j, row)
        ro = {"max_iterations": int(row[5]), "min_iterations": int(row[6]), "max_epipolar_error": float(row[3]), "seed": int(row[4])}
        bo = {"max_iterations": int(row[9]), "loss_type": loss_name[int(row[7])], "loss_scale": float(row[8]), "gradient_tol": 1e-10}
        if kind == 3:
            c1, c2 = classic_options_cameras(row)
            cams = [{"model": "PINHOLE" if c[0] else "SIMPLE_PINHOLE", "width": 1600, "height": 1200, "params": c[1]} for c in (c1, c2)]
            pose, info = poselib.estimate_relative_pose(p["x1"], p["x2"], cams[0], cams[1], ro, bo)
            m = np.r_[pose.q, pose.t]
        elif kind == 4:
            pair, info = poselib.estimate_shared_focal_relative_pose(p["x1"], p["x2"], (float(row[12]), float(row[13])), ro, bo)
            m = np.r_[pair.pose.q, pair.pose.t, pair.camera1.params[0]]
        else:
            F, info = poselib.estimate_fundamental(p["x1"], p["x2"], ro, bo)
            m = np.asarray(F).reshape(-1)
        r, ist = g[f"{name}_model"][j], g[f"{name}_istats"][j]
        if j in CLASSIC_OPTIONS_OTHER_WINNER.get(name, ()):
            other += 1
            assert info["iterations"] == int(ist[1]) and abs(info["num_inliers"] - int(ist[2])) <= 1, (name, j, info["num_inliers"])
            continue
        assert (info["iterations"], info["num_inliers"]) == (int(ist[1]), int(ist[2])), (name, j, info["iterations"], info["num_inliers"], ist)
        assert np.array_equal(np.array(info["inliers"], dtype=np.uint8), np.unpackbits(g[f"{name}_mask"][j])[:n]), (name, j)
        d = fund_diff(m, r[:9]) if kind == 5 else pose_diff(m[:7], r[:7])
        assert d < 1e-6, (name, j, d)
        if kind == 4:
            assert abs(m[7] - r[7]) < 1e-6 * r[7], (name, j)
        assert info["refinements"] - int(ist[0]) in (0, CLASSIC_OPTIONS_LO_DEVIATIONS.get(name, {}).get(j, 0)), (name, j, info["refinements"], int(ist[0]))
    assert other == len(CLASSIC_OPTIONS_OTHER_WINNER.get(name, ()))


@pytest.mark.parametrize("name", ["relpose_5pt", "shared_6pt", "fundamental_7pt"])
def test_edge_options_vs_reference_fixture(golden, name):
    """tests/golden/edge_options_ref_classic.npz through the drop-in module: max_iterations 0 / 1 / below min_iterations, success_prob 0 / 1,
    dyn_num_trials_mult 0, thresholds 0 / 1e-3 / 100 px, a 41-bit seed, loss_scale 0, pinned damping, tolerances of 1.  Iterations, inlier count, mask and
    model identical to the REFERENCE BINARY but for the enumerated ties; LO count = the reference's or the oracle's where those differ (one case)."""
    import mdrp_amd.poselib as poselib
    from mdrp_amd import _capi
    from helpers import CLASSIC_EDGE_LO_DEVIATIONS, CLASSIC_EDGE_TIES, CLASSIC_OPTIONS_KINDS, classic_edge_cases, classic_edge_pair
    from test_oracle_classic import _classic_edge_model_equal
    g = golden("edge_options_ref_classic")
    kind = CLASSIC_OPTIONS_KINDS[name]
    p = classic_edge_pair(name)
    cam = {"model": "SIMPLE_PINHOLE", "width": 1600, "height": 1200, "params": [800.0, 0.0, 0.0]}
    loss_name = {v: k for k, v in _capi.LOSS_TYPES.items()}
    for j, (rod, bod) in enumerate(classic_edge_cases()):
        bo = dict(bod, loss_type=loss_name[bod["loss_type"]])
        if kind == 3:
            pose, info = poselib.estimate_relative_pose(p["x1"], p["x2"], cam, cam, rod, bo)
            m = np.r_[pose.q, pose.t]
        elif kind == 4:
            pair, info = poselib.estimate_shared_focal_relative_pose(p["x1"], p["x2"], (0.0, 0.0), rod, bo)
            m = np.r_[pair.pose.q, pair.pose.t, 0.0, 0.0, 0.0, pair.camera1.params[0]]
        else:
            F, info = poselib.estimate_fundamental(p["x1"], p["x2"], rod, bo)
            m = np.asarray(F).reshape(-1)
        ref = g[f"{name}_stats"][j]
        assert (info["iterations"], info["num_inliers"]) == (int(ref[1]), int(ref[2])), (name, j, rod, bod, info["iterations"], info["num_inliers"], ref)
        lo = next((v for k, v in CLASSIC_EDGE_LO_DEVIATIONS.get(name, {}).items() if rod.get(k.split("=")[0]) == float(k.split("=")[1])), 0)
        assert info["refinements"] - int(ref[0]) in (0, lo), (name, j, rod, info["refinements"], ref[0])
        if any(all(rod.get(k) == v for k, v in tie.items()) for tie in CLASSIC_EDGE_TIES.get(name, ())):
            continue
        assert np.array_equal(np.array(info["inliers"], dtype=np.uint8), np.unpackbits(g[f"{name}_mask"][j])[:300]), (name, j)
        assert _classic_edge_model_equal(kind, m, g[f"{name}_model"][j]), (name, j, rod, bod, m, g[f"{name}_model"][j])


# (estimator, option set, pair): LO count off by one against the oracle, everything else equal — a degree-10 root at the edge of existence that the device's
# elimination finds and the oracle's does not, the class enumerated in test_gpu_headline.GPU_MINUS_ORACLE_LO_BASELINES
RAGGED_LO_OFF = {("relpose_5pt", 1, 8): 1}


@pytest.mark.parametrize("name", ["relpose_5pt", "shared_6pt", "fundamental_7pt"])
def test_batched_ragged_calls_under_random_options_vs_oracle(golden, name):
    """The first 8 option sets of tests/golden/options_ref_classic.npz, each driving ONE batched call of the drop-in module over 10 ragged pairs (N = 40 ...
    1500; 5-point: a camera pair of its own per image pair): every pair's iterations, inlier count and mask = the oracle's, model within 2e-6, LO count
    equal (+-1 below N = 100, where scores tie; the 6-point solver's solution-order ties: +-2; one enumerated 5-point pair: RAGGED_LO_OFF)."""
    import mdrp_amd.poselib as poselib
    from mdrp_amd import _capi, synth
    from helpers import CLASSIC_OPTIONS_KINDS
    g = golden("options_ref_classic")
    kind = CLASSIC_OPTIONS_KINDS[name]
    loss_name = {v: k for k, v in _capi.LOSS_TYPES.items()}
    sizes = [40, 63, 64, 65, 150, 257, 512, 900, 1024, 1500]
    focals = [500.0, 800.0, 1400.0]
    for j in range(8):
        row = g["cases"][j]
        ro = {"max_iterations": int(row[5]), "min_iterations": int(row[6]), "max_epipolar_error": float(row[3]), "seed": int(row[4])}
        bo = {"max_iterations": int(row[9]), "loss_type": loss_name[int(row[7])], "loss_scale": float(row[8]), "gradient_tol": 1e-10}
        pairs, cams1, cams2 = [], [], []
        for i, n in enumerate(sizes):
            f1, f2 = focals[i % 3], focals[(i + j) % 3]
            kw = dict(noise_px=float(row[2]), depth_noise=0.0, outlier_frac=[0.0, 0.3, 0.5][(i + j) % 3], pp=(3.0, -2.0))
            pairs.append(synth.make_pair(98000 + 100 * j + i, n, random_focal="shared", **kw) if kind == 4 else synth.make_pair(98000 + 100 * j + i, n, f1=f1, f2=f2, **kw))
            cams1.append({"model": "SIMPLE_PINHOLE", "width": 1600, "height": 1200, "params": [f1, 3.0, -2.0]})
            cams2.append({"model": "PINHOLE", "width": 1600, "height": 1200, "params": [f2 * 1.01, f2 * 0.99, 3.0, -2.0]})
        x1, x2 = [p["x1"] for p in pairs], [p["x2"] for p in pairs]
        if kind == 3:
            models, infos = poselib.estimate_relative_pose_batch(x1, x2, cams1, cams2, ro, bo)
            rows = [np.r_[m.q, m.t] for m in models]
        elif kind == 4:
            models, infos = poselib.estimate_shared_focal_relative_pose_batch(x1, x2, (3.0, -2.0), ro, bo)
            rows = [np.r_[m.pose.q, m.pose.t, m.camera1.params[0]] for m in models]
        else:
            models, infos = poselib.estimate_fundamental_batch(x1, x2, ro, bo)
            rows = [np.asarray(m).reshape(-1) for m in models]
        oro = po.ransac_opt(**ro)
        obo = po.bundle_opt(max_iterations=int(row[9]), loss_type=int(row[7]), loss_scale=float(row[8]), gradient_tol=1e-10)
        for i, n in enumerate(sizes):
            c1 = po.cam_flat(0, cams1[i]["params"]) if kind == 3 else None
            c2 = po.cam_flat(1, cams2[i]["params"]) if kind == 3 else None
            m, st, mask = po.estimate_classic(kind, x1[i], x2[i], oro, obo, c1, c2, pp=(3.0, -2.0))
            m, info, where = np.asarray(m, float).reshape(-1), infos[i], (name, j, i, n)
            assert (info["iterations"], info["num_inliers"]) == (st.iterations, st.num_inliers), where
            assert np.array_equal(np.array(info["inliers"], dtype=np.uint8), mask), where
            d = fund_diff(rows[i], m[:9]) if kind == 5 else pose_diff(rows[i][:7], m[:7])
            assert d < 2e-6 and (kind != 4 or abs(rows[i][7] - m[10]) < 2e-6 * m[10]), (where, d)
            lo_tol = RAGGED_LO_OFF.get((name, j, i), (2 if kind == 4 else 1) if n < 100 else (2 if kind == 4 else 0))
            assert abs(info["refinements"] - st.refinements) <= lo_tol, (where, info["refinements"], st.refinements)


@pytest.mark.parametrize("name", ["relpose_5pt", "shared_6pt", "fundamental_7pt"])
def test_corrupted_inputs_vs_oracle(name):
    """NaN / inf coordinates (5 of 300 correspondences), 30 identical correspondences, 20 inliers among 280 random matches: the comparison rows through
    the drop-in module against the oracle (which a one-off probe against the reference binary found identical on these inputs for the 5- and 7-point
    estimators): iterations, inlier count, mask, LO count; model to 1e-6 or non-finite in the same places."""
    import mdrp_amd.poselib as poselib
    from mdrp_amd import synth
    from helpers import CLASSIC_OPTIONS_KINDS
    kind = CLASSIC_OPTIONS_KINDS[name]
    cam = {"model": "SIMPLE_PINHOLE", "width": 1600, "height": 1200, "params": [800.0, 0.0, 0.0]}
    ro = {"max_iterations": 500, "min_iterations": 500, "max_epipolar_error": 2.0, "seed": 2}
    bo = {"max_iterations": 100, "loss_type": "TRUNCATED_CAUCHY", "loss_scale": 1.0, "gradient_tol": 1e-10}
    for mode in ("nan_point", "inf_point", "dup_points", "few_inliers"):
        p0 = synth.make_pair(54000, 300, noise_px=0.5, depth_noise=0.0, outlier_frac=0.3, random_focal="shared" if kind == 4 else None)
        x1, x2 = np.array(p0["x1"], copy=True), np.array(p0["x2"], copy=True)
        idx = np.random.default_rng(5).choice(300, 30, replace=False)
        if mode == "nan_point": x2[idx[:5], 0] = np.nan
        if mode == "inf_point": x1[idx[:5], 1] = np.inf
        if mode == "dup_points": x1[idx] = x1[idx[0]]; x2[idx] = x2[idx[0]]
        if mode == "few_inliers": x2[20:] = np.random.default_rng(6).uniform(-500, 500, (280, 2))
        if kind == 3:
            pose, info = poselib.estimate_relative_pose(x1, x2, cam, cam, ro, bo)
            mine = np.r_[pose.q, pose.t]
        elif kind == 4:
            pair, info = poselib.estimate_shared_focal_relative_pose(x1, x2, (0.0, 0.0), ro, bo)
            mine = np.r_[pair.pose.q, pair.pose.t, pair.camera1.params[0]]
        else:
            F, info = poselib.estimate_fundamental(x1, x2, ro, bo)
            mine = np.asarray(F).reshape(-1)
        c = po.cam_flat(0, [800.0, 0.0, 0.0]) if kind == 3 else None
        m, st, mask = po.estimate_classic(kind, x1, x2, po.ransac_opt(**ro), po.bundle_opt(max_iterations=100, loss_type=4, loss_scale=1.0, gradient_tol=1e-10), c, c, pp=(0.0, 0.0))
        m = np.asarray(m, float).reshape(-1)
        want = m[:7] if kind == 3 else (np.r_[m[:7], m[10]] if kind == 4 else m[:9])
        where = (name, mode)
        assert (info["iterations"], info["num_inliers"]) == (st.iterations, st.num_inliers), where
        assert abs(info["refinements"] - st.refinements) <= (2 if kind == 4 else 0), (where, info["refinements"], st.refinements)  # (6-point: solution-order ties)
        assert np.array_equal(np.array(info["inliers"], dtype=np.uint8), mask), where
        if np.isfinite(want).all() and np.linalg.norm(want[4:7] if kind != 5 else want) > 0:
            d = fund_diff(mine, want) if kind == 5 else pose_diff(mine[:7], want[:7])
            assert d < 1e-6 and (kind != 4 or abs(mine[7] - want[7]) < 1e-6 * abs(want[7])), (where, d)
        else:
            assert np.array_equal(np.isfinite(mine), np.isfinite(want)) and np.allclose(np.nan_to_num(mine, posinf=0, neginf=0), np.nan_to_num(want, posinf=0, neginf=0), atol=1e-9), (where, mine, want)
