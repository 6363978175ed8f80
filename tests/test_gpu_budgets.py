"""Iteration budgets on a real MI355X (include/mdrp.h): one call returns the result at every budget of a list, each bit for bit what
a separate call with max_iterations = that budget returns.  Every comparison is equality of bytes (records, NaN models included, and masks)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RF = {1: "shared", 2: "varying", 4: "shared"}   # synth.make_pair random_focal per estimator
RO = {"max_epipolar_error": 2.0, "max_reproj_error": 16.0}
BO = {"loss_type": "TRUNCATED_CAUCHY"}
KNOBS = ("MDRP_CHUNKS", "MDRP_LO_OVERLAP", "MDRP_BOUND", "MDRP_FUSE_TAIL", "MDRP_LO_THREADS", "MDRP_FINAL_THREADS", "MDRP_PAIRS_PER_PASS")
PREFIX_BUDGETS = [1, 10, 127, 128, 129, 300]   # the default first chunk of a 300-iteration run is 128
PREFIX_N = [0, 2, 40, 150, 300]
VARIANTS = [(0, False), (0, True), (1, False), (2, False), (3, False), (4, False), (5, False)]   # (kind, monodepth_estimate_shift)

_cache = {}


def _batch(first, B, n, kind, **kw):
    """inputs of one call: correspondences, depths (monodepth kinds) and cameras as the C ABI takes them"""
    from mdrp_amd import _capi, synth
    b = synth.make_batch(first, B, n, noise_px=0.5, depth_noise=0.02, random_focal=RF.get(kind), **kw)
    cams = np.zeros(B, dtype=_capi.CAMERA_DTYPE)
    if kind in (0, 3):
        cams["params"][:, 0] = 800.0
    c = cams if kind in (0, 3, 4) else None
    mono = kind <= 2
    return dict(kind=kind, x1=b["x1"], x2=b["x2"], d1=b["d1"] if mono else None, d2=b["d2"] if mono else None, cam=c)


def _join(parts):
    return {k: (parts[0][k] if k == "kind" else None if parts[0][k] is None else np.concatenate([p[k] for p in parts])) for k in parts[0]}


def _opts(ro):
    from mdrp_amd import _capi
    return _capi.ransac_opt_from_dict(dict(RO, **ro)), _capi.bundle_opt_from_dict(BO)


def _plain(h, inp, ro, npp=None):
    r, b = _opts(ro)
    res, mask = h.estimate_batch(inp["kind"], inp["x1"], inp["x2"], inp["d1"], inp["d2"], r, b, npp, inp["cam"], inp["cam"])
    return res.copy(), mask.copy()


def _budgets(h, inp, ro, budgets, npp=None):
    r, b = _opts(dict(ro, max_iterations=budgets[-1]))
    res, mask = h.estimate_batch_budgets(inp["kind"], inp["x1"], inp["x2"], inp["d1"], inp["d2"], r, b, budgets, npp, inp["cam"], inp["cam"])
    return res.copy(), mask.copy()


def _same(res, mask, ref, ref_mask, what):
    assert res.shape == ref.shape and mask.shape == ref_mask.shape, what
    bad = [i for i in np.ndindex(res.shape) if res[i].tobytes() != ref[i].tobytes()]
    assert not bad, (what, bad[:8], [(res[i], ref[i]) for i in bad[:2]])
    assert mask.tobytes() == ref_mask.tobytes(), (what, np.argwhere((mask != ref_mask).any(axis=-1))[:8])


def _separate(h, inp, ro, budgets, npp=None):
    """the reference: one call per budget with max_iterations = the budget, stacked to (C, B) and (C, B, N)"""
    parts = [_plain(h, inp, dict(ro, max_iterations=k), npp) for k in budgets]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])


def _prefix_case(kind, shift):
    """inputs, options and the separate calls' results of the prefix test, computed once per estimator and shared with the schedule test"""
    from mdrp_amd import _capi
    key = (kind, shift)
    if key not in _cache:
        inp = _batch(7100 + 10 * kind, 5, 300, kind, outlier_frac=0.5)
        ro = {"min_iterations": 300, "monodepth_estimate_shift": shift}
        npp = np.array(PREFIX_N, dtype=np.int32)
        h = _capi.Handle(0)
        try:
            ref = _separate(h, inp, ro, PREFIX_BUDGETS, npp)
        finally:
            h.close()
        _cache[key] = (inp, ro, npp, ref)
    return _cache[key]


@pytest.fixture
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.mark.parametrize("kind,shift", VARIANTS)
def test_every_budget_equals_the_separate_call(clean_env, kind, shift):
    """All six estimators and the calibrated shift solver; ragged pairs down to none at all; budgets on both sides of the first chunk's end.  Host
    buffers and device pointers; the last budget is the call without budgets, and what mdrp_fetch_results returns afterwards."""
    import torch
    from mdrp_amd import _capi
    inp, ro, npp, (ref, ref_mask) = _prefix_case(kind, shift)
    C_, B, N = len(PREFIX_BUDGETS), 5, 300
    h = _capi.Handle(0)
    try:
        res, mask = _budgets(h, inp, ro, PREFIX_BUDGETS, npp)
        _same(res, mask, ref, ref_mask, "host buffers")
        last = h.fetch_results(B)
        assert last.tobytes() == ref[-1].tobytes()
        plain, plain_mask = _plain(h, inp, dict(ro, max_iterations=PREFIX_BUDGETS[-1]), npp)
        _same(res[-1], mask[-1], plain, plain_mask, "the call without budgets")
        assert res["iterations"][:, 0].tolist() == [0] * C_ and res["iterations"][:, 4].tolist() == PREFIX_BUDGETS   # (min_iterations = 300: nothing stops early)

        dev = torch.device("cuda", 0)
        t = {k: None if inp[k] is None else torch.from_numpy(inp[k]).to(dev) for k in ("x1", "x2", "d1", "d2")}
        dmask = torch.full((C_, B, N), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        r, b = _opts(dict(ro, max_iterations=PREFIX_BUDGETS[-1]))
        h.estimate_batch_budgets_device(kind, t["x1"].data_ptr(), t["x2"].data_ptr(), t["d1"].data_ptr() if t["d1"] is not None else 0,
                                        t["d2"].data_ptr() if t["d2"] is not None else 0, B, N, r, b, PREFIX_BUDGETS, npp, inp["cam"], inp["cam"], dmask.data_ptr())
        dres = h.fetch_budget_results(C_, B)
        _same(dres, dmask.cpu().numpy(), ref, ref_mask, "device pointers")
        assert h.fetch_results(B).tobytes() == ref[-1].tobytes()
        copy = torch.zeros(C_ * B * _capi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        h.copy_budget_results_device(copy.data_ptr(), C_, B)
        assert copy.cpu().numpy().tobytes() == ref.tobytes()
    finally:
        h.close()


@pytest.mark.parametrize("kind", [0, 2, 5])
def test_pairs_stopped_by_the_dynamic_rule_report_their_stopped_state(clean_env, kind):
    """two nearly outlier-free pairs stop just behind min_iterations = 50, two at 80 % outliers run on: budgets before, at and behind the stop"""
    from mdrp_amd import _capi
    budgets = [30, 50, 51, 200, 2000]
    inp = _join([_batch(7300 + 10 * kind, 2, 200, kind, outlier_frac=0.02), _batch(7350 + 10 * kind, 2, 200, kind, outlier_frac=0.8)])
    ro = {"min_iterations": 50}
    h = _capi.Handle(0)
    try:
        ref, ref_mask = _separate(h, inp, ro, budgets)
        res, mask = _budgets(h, inp, ro, budgets)
        print("iterations per budget:", res["iterations"].tolist())
        _same(res, mask, ref, ref_mask, kind)
        assert int(res["iterations"][-1, :2].max()) < 200, res["iterations"].tolist()       # the case is reached: these pairs stopped
        assert res["iterations"][0].tolist() == [30] * 4 and int(res["iterations"][-1, 2:].min()) > 200
    finally:
        h.close()


# 85 % outliers of N = 60 leave nine inliers; one of these pairs finds ten correspondences within the threshold, and 1/6 cubed ends its run at 5956
# iterations, before the last budget.  90 % (six inliers): none of them can stop before 6000, which the test asserts.
SUPER_OUTLIERS = 0.9


def test_budgets_on_a_super_chunk_edge(clean_env):
    """chunk_cap is 4096 for this run: budgets at the capacity and on both sides of it, pairs that run to the end"""
    from mdrp_amd import _capi
    budgets = [4095, 4096, 4097, 6000]
    inp = _batch(7500, 3, 60, 0, outlier_frac=SUPER_OUTLIERS)
    ro = {"min_iterations": 100}
    h = _capi.Handle(0)
    try:
        res, mask = _budgets(h, inp, ro, budgets)
        print("iterations per budget:", res["iterations"].tolist())
        assert res["iterations"][-1].tolist() == [6000] * 3        # nobody stopped early: every budget is reached by every pair
        ref, ref_mask = _separate(h, inp, ro, budgets)
        _same(res, mask, ref, ref_mask, "super-chunks")
    finally:
        h.close()


SCHEDULES = ({"MDRP_CHUNKS": "0", "MDRP_LO_OVERLAP": "0"}, {"MDRP_CHUNKS": "64,256"}, {"MDRP_FUSE_TAIL": "1"}, {"MDRP_PAIRS_PER_PASS": "2"})


@pytest.mark.parametrize("kind", [0, 3])
def test_schedules_do_not_change_a_budgets_call(clean_env, kind):
    """one chunk on one stream, other chunk lengths, the fused tail asked for (a budgets call runs unfused all the same) and three passes: the bytes
    of the default schedule, which are the separate calls'"""
    from mdrp_amd import _capi
    inp, ro, npp, (ref, ref_mask) = _prefix_case(kind, False)
    h = _capi.Handle(0)
    try:
        for env in SCHEDULES:
            for k in KNOBS:
                clean_env.delenv(k, raising=False)
            for k, v in env.items():
                clean_env.setenv(k, v)
            res, mask = _budgets(h, inp, ro, PREFIX_BUDGETS, npp)
            _same(res, mask, ref, ref_mask, env)
    finally:
        h.close()


@pytest.mark.parametrize("kind", [0, 3])
def test_score_initial_model_with_budgets(clean_env, kind):
    from mdrp_amd import _capi
    budgets = [1, 5, 40]
    inp = _batch(7600 + kind, 4, 120, kind, outlier_frac=0.3)
    ro = {"min_iterations": 40, "score_initial_model": True}
    h = _capi.Handle(0)
    try:
        ref, ref_mask = _separate(h, inp, ro, budgets)
        res, mask = _budgets(h, inp, ro, budgets)
        _same(res, mask, ref, ref_mask, kind)
        assert int(res["refinements"].min()) >= 2    # the initial model's refinement and the closing one
    finally:
        h.close()


def test_only_distinct_states_are_refined(clean_env):
    """pairs that stop before the first budget have one state: it is refined once, not once per budget — the LM sweeps of the budgets call evaluate
    exactly as many correspondences as those of the plain call"""
    from mdrp_amd import _capi
    budgets = [100, 200, 400]
    inp = _batch(7700, 8, 200, 0, outlier_frac=0.0)
    ro = {"min_iterations": 20}
    h = _capi.Handle(0)
    try:
        plain, plain_mask = _plain(h, inp, dict(ro, max_iterations=400))
        want = h.last_stats()
        res, mask = _budgets(h, inp, ro, budgets)
        got = h.last_stats()
        assert int(res["iterations"].max()) < 100, res["iterations"].tolist()
        assert want["final_accum_evals"] > 0 and want["final_cost_evals"] > 0
        assert got["final_accum_evals"] == want["final_accum_evals"] and got["final_cost_evals"] == want["final_cost_evals"]
        for c in range(3):
            _same(res[c], mask[c], plain, plain_mask, c)
    finally:
        h.close()


def test_invalid_budget_lists_and_options_are_refused(clean_env):
    from mdrp_amd import _capi
    import mdrp_amd.poselib as poselib
    inp = _batch(7800, 2, 50, 0)
    h = _capi.Handle(0)
    lib = h._lib
    out = np.zeros((17, 2), dtype=_capi.RESULT_DTYPE)
    bo = _capi.bundle_opt_from_dict(BO)

    def call(budgets, **ro):
        ks = np.asarray(budgets, dtype=np.uint64)
        r = _capi.ransac_opt_from_dict(dict(RO, **ro))
        rc = lib.mdrp_estimate_batch_budgets(h._h, 0, _capi.MEM_HOST, _capi._ptr(inp["x1"]), _capi._ptr(inp["x2"]), _capi._ptr(inp["d1"]), _capi._ptr(inp["d2"]),
                                             2, 50, None, _capi._ptr(inp["cam"]), _capi._ptr(inp["cam"]), C.byref(r), C.byref(bo), _capi._ptr(ks), len(ks),
                                             _capi._ptr(out), None)
        return rc, lib.mdrp_last_error().decode()
    try:
        cases = {"empty": ([], 100), "zero": ([0, 100], 100), "repeated": ([50, 50, 100], 100), "decreasing": ([100, 50], 50), "too many": (list(range(1, 18)), 17),
                 "last is not max_iterations": ([10, 100], 1000)}
        for why, (budgets, max_it) in cases.items():
            rc, msg = call(budgets, max_iterations=max_it, min_iterations=10)
            assert rc == 1 and msg.startswith("budgets"), (why, rc, msg)
        rc, msg = call([10, 100], max_iterations=100, min_iterations=10, progressive_sampling=True)
        assert rc == 4 and "progressive_sampling" in msg, (rc, msg)
        rc, msg = call([10, 100], max_iterations=100, min_iterations=10)
        assert rc == 0, msg
        cam = {"model": "SIMPLE_PINHOLE", "width": 1600, "height": 1200, "params": [800.0, 0.0, 0.0]}
        for budgets in ([], [0, 100], [100, 100], list(range(1, 18))):
            with pytest.raises(ValueError):
                poselib.estimate_monodepth_relative_pose_batch(inp["x1"], inp["x2"], inp["d1"], inp["d2"], cam, cam, dict(RO), BO, budgets=budgets)
        with pytest.raises(ValueError):
            poselib.estimate_monodepth_relative_pose_batch(inp["x1"], inp["x2"], inp["d1"], inp["d2"], cam, cam, dict(RO, max_iterations=1000), BO, budgets=[10, 100])
        with pytest.raises(NotImplementedError):
            poselib.estimate_monodepth_relative_pose_batch(inp["x1"], inp["x2"], inp["d1"], inp["d2"], cam, cam, dict(RO, progressive_sampling=True), BO, budgets=[10, 100])
    finally:
        h.close()


def test_poselib_entries_gain_a_budget_axis(clean_env):
    """estimate_batch_torch(..., budgets=) returns (C, B) records and a (C, B, N) device mask equal to the host route's, whose object form is a list
    over the budgets of the lists it returns without them"""
    import torch
    import mdrp_amd.poselib as poselib
    from mdrp_amd import synth
    budgets = [8, 64, 200]
    cam = {"model": "SIMPLE_PINHOLE", "width": 1600, "height": 1200, "params": [800.0, 0.0, 0.0]}
    b = synth.make_batch(7900, 4, 150, noise_px=0.5, depth_noise=0.02, outlier_frac=0.4)
    ro = dict(RO, min_iterations=200)
    res, mask, ns = poselib.estimate_monodepth_relative_pose_batch(b["x1"], b["x2"], b["d1"], b["d2"], cam, cam, ro, BO, as_arrays=True, budgets=budgets)
    assert res.shape == (3, 4) and mask.shape == (3, 4, 150) and res["iterations"].tolist() == [[k] * 4 for k in budgets]
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(b[k]).to(dev) for k in ("x1", "x2", "d1", "d2")]
    tres, tmask = poselib.estimate_batch_torch("calibrated", *t, cam, cam, ro, BO, budgets=budgets)
    assert tmask.is_cuda and tuple(tmask.shape) == (3, 4, 150)
    _same(tres, tmask.cpu().numpy(), res, mask, "torch")
    geoms, infos = poselib.estimate_monodepth_relative_pose_batch(b["x1"], b["x2"], b["d1"], b["d2"], cam, cam, ro, BO, budgets=budgets)
    one, one_info = poselib.estimate_monodepth_relative_pose_batch(b["x1"], b["x2"], b["d1"], b["d2"], cam, cam, dict(ro, max_iterations=64), BO)
    assert len(geoms) == len(infos) == 3 and len(geoms[1]) == 4
    assert infos[1] == one_info and all(np.array_equal(g.pose.R, o.pose.R) and g.scale == o.scale for g, o in zip(geoms[1], one))


def test_more_pairs_than_one_tile_of_the_planning_kernel(clean_env):
    """1100 pairs: k_ckpt_plan's workgroup walks the batch in tiles of 1024 and carries the list position across them; the LO runs one wavefront
    per problem and the fp32 bound stage is on (calls beyond 128 pairs).  Half the pairs stop by the dynamic rule between the budgets."""
    from mdrp_amd import _capi
    budgets = [16, 40, 41, 90, 400]
    inp = _join([_batch(8000, 550, 24, 0, outlier_frac=0.0), _batch(8600, 550, 24, 0, outlier_frac=0.6)])
    npp = np.where(np.arange(1100) % 97 == 5, 2, 24).astype(np.int32)     # a few pairs below the sample size
    ro = {"min_iterations": 40}
    h = _capi.Handle(0)
    try:
        ref, ref_mask = _separate(h, inp, ro, budgets, npp)
        res, mask = _budgets(h, inp, ro, budgets, npp)
        _same(res, mask, ref, ref_mask, "1100 pairs")
        stopped = res["iterations"][-1] < 400
        assert 100 < int(stopped.sum()) < 1100 and int(res["iterations"][-1].max()) == 400
    finally:
        h.close()
