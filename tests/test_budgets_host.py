"""Iteration budgets (include/mdrp.h), the parts that need no GPU: the new symbols in the header and the binding under the unchanged
ABI number, the argument checks of the Python layers, and evalio's graph mode around an injected estimator."""
import os
import re

import numpy as np
import pytest

from mdrp_amd import _capi, evalio, synth
import mdrp_amd.poselib as poselib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mdrp_estimate_batch_budgets", "mdrp_estimate_batch_budgets_async", "mdrp_fetch_budget_results", "mdrp_copy_budget_results_device")
BAD_LISTS = {"empty": [], "zero": [0, 10], "repeated": [5, 5], "decreasing": [10, 5], "too many": list(range(1, 18)), "fraction": [1.5, 3]}


def test_header_and_binding_declare_the_entry_points_under_abi_6():
    header = open(os.path.join(ROOT, "include", "mdrp.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(mdrp_handle \*h,", header), name
        assert name in _capi.EXPORTS, name
    assert re.search(r"#define MDRP_ABI_VERSION 0x00000006\b", header) and _capi.ABI_VERSION == 6
    assert re.search(r"#define MDRP_MAX_BUDGETS 16\b", header) and _capi.MAX_BUDGETS == 16
    # appended: every declaration that was there before comes first, unchanged in order
    assert header.index("mdrp_estimate_matches_async(") < min(header.index(n + "(") for n in NEW_SYMBOLS)
    source = open(os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_capi.hip")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int " + name + r"\(", source, re.M), name


def test_budget_list_sets_or_checks_max_iterations():
    ks, ro = _capi.budget_list([10, 20, 50], {"seed": 3})
    assert ks.dtype == np.uint64 and ks.tolist() == [10, 20, 50] and ro == {"seed": 3, "max_iterations": 50}
    assert _capi.budget_list((7,), {"max_iterations": 7})[1]["max_iterations"] == 7
    assert _capi.budget_list(np.array([1, 2, 16]))[0].tolist() == [1, 2, 16]
    assert len(_capi.budget_list(list(range(1, 17)))[0]) == 16
    with pytest.raises(ValueError, match="differs from the last budget"):
        _capi.budget_list([10, 20], {"max_iterations": 1000})
    for bad in BAD_LISTS.values():
        with pytest.raises(ValueError, match="budgets"):
            _capi.budget_list(bad)


def test_poselib_checks_budgets_before_a_library_is_needed(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was asked for before the budgets were checked")
    monkeypatch.setattr(_capi, "load_library", no_library)
    monkeypatch.setattr(_capi, "default_handle", no_library)
    b = synth.make_batch(9100, 2, 20)
    cam = {"model": "SIMPLE_PINHOLE", "width": 1600, "height": 1200, "params": [800.0, 0.0, 0.0]}
    x1, x2, d1, d2 = b["x1"], b["x2"], b["d1"], b["d2"]
    entries = {
        "calibrated": lambda **kw: poselib.estimate_monodepth_relative_pose_batch(x1, x2, d1, d2, cam, cam, **kw),
        "shared focal": lambda **kw: poselib.estimate_monodepth_shared_focal_relative_pose_batch(x1, x2, d1, d2, **kw),
        "varying focal": lambda **kw: poselib.estimate_monodepth_varying_focal_relative_pose_batch(x1, x2, d1, d2, **kw),
        "5-point": lambda **kw: poselib.estimate_relative_pose_batch(x1, x2, cam, cam, **kw),
        "6-point": lambda **kw: poselib.estimate_shared_focal_relative_pose_batch(x1, x2, None, **kw),
        "7-point": lambda **kw: poselib.estimate_fundamental_batch(x1, x2, **kw),
        "torch": lambda **kw: poselib.estimate_batch_torch("calibrated", x1, x2, d1, d2, cam, cam, **kw),
    }
    for call in entries.values():
        for bad in BAD_LISTS.values():
            with pytest.raises(ValueError, match="budgets"):
                call(budgets=bad)
        with pytest.raises(ValueError, match="differs from the last budget"):
            call(ransac_opt={"max_iterations": 1000}, budgets=[10, 100])


def _fake_h5(n_pairs, n=40):
    h5, gt = {}, []
    for i in range(n_pairs):
        p = synth.make_pair(9200 + i, n + i, noise_px=0.0, depth_noise=0.0, pp=(640.0, 480.0))
        a, b = f"img{i:02d}a_o", f"img{i:02d}b"
        data = np.zeros((len(p["x1"]), 32))
        data[:, :2] = p["x1"]; data[:, 2:4] = p["x2"]
        c1, c2 = evalio.depth_indices(10)
        data[:, c1] = p["d1"]; data[:, c2] = p["d2"]
        h5[f"corr_{a}_{b}"] = data
        h5[f"pose_{a}_{b}"] = np.c_[p["R"], p["t"]]
        h5[f"K_{a}"] = h5[f"K_{b}"] = np.array([[800.0, 0, 640.0], [0, 800.0, 480.0], [0, 0, 1]])
        gt.append(p)
    return h5, gt


class _Clock:
    """perf_counter that advances 12 ms per estimator call (two readings per call)"""
    def __init__(self):
        self.reads = 0

    def perf_counter(self):
        self.reads += 1
        return 0.012 * (self.reads // 2)


@pytest.mark.parametrize("focal", [False, True])
def test_evalio_graph_mode_emits_one_record_per_pair_and_budget(monkeypatch, focal):
    """one estimator call per batch with budgets = the list and min = max = its last entry; records ordered pair-major, budget innermost, each
    with the budget as `iterations` and the call's time per pair divided by the number of budgets as `runtime`"""
    h5, gt = _fake_h5(5)
    budgets = [10, 20, 50, 100]
    calls = []

    def objects(kps, c):   # the pair's ground truth, marked with the budget's index in the info record
        out = []
        for kp in kps:
            g = next(q for q in gt if len(q["x1"]) == len(kp))
            pose = type("P", (), {"R": g["R"], "t": g["t"]})()
            cam = type("C", (), {"focal": lambda self: 800.0})()
            out.append(type("G", (), {"pose": pose, "camera1": cam, "camera2": cam})())
        infos = [{"refinements": c, "iterations": 7, "num_inliers": len(kp), "inlier_ratio": 1.0, "model_score": 0.0, "inliers": [True]} for kp in kps]
        return out, infos

    def stub(k1, k2, d1, d2, *rest, budgets=None):
        ro = rest[-2]
        calls.append((len(k1), budgets, ro["max_iterations"], ro["min_iterations"]))
        parts = [objects(k1, c) for c in range(len(budgets))]
        return [p[0] for p in parts], [p[1] for p in parts]

    monkeypatch.setattr(evalio, "time", _Clock())
    if focal:
        res = evalio.evaluate_focal(h5, ["3p_ours_scale_hybrid_ctruncated+10"], shared=True, batch=3, estimate_batch=stub, iterations_list=budgets)
    else:
        res = evalio.evaluate_calibrated(h5, ["p3p_hybrid+10"], iters=77, batch=3, estimate_batch=stub, iterations_list=budgets)
    assert calls == [(3, budgets, 100, 100), (2, budgets, 100, 100)]            # one run per batch, min = max = the last budget
    assert len(res) == 5 * len(budgets)
    for i in range(5):
        for c, k in enumerate(budgets):
            r = res[i * len(budgets) + c]
            assert r["info"]["iterations"] == k and r["info"]["refinements"] == c and r["info"]["num_inliers"] == 40 + i, (i, c)
            assert r["R_err"] < 1e-6 and r["info"]["inliers"] == []
            assert r["info"]["runtime"] == pytest.approx(12.0 / (3 if i < 3 else 2) / len(budgets), rel=1e-12)
    with pytest.raises(ValueError):
        evalio.evaluate_calibrated(h5, ["p3p_hybrid+10"], estimate_batch=stub, iterations_list=[10, 10])


def test_evalio_without_a_list_calls_injected_estimators_as_before():
    h5, gt = _fake_h5(2)

    def stub(k1, k2, d1, d2, c1, c2, ro_, bo_):   # (no budgets keyword: the signature of the existing tests' estimators)
        poses = [type("G", (), {"pose": type("P", (), {"R": q["R"], "t": q["t"]})()})() for kp in k1 for q in gt if len(q["x1"]) == len(kp)]
        return poses, [{"refinements": 1, "iterations": 10, "num_inliers": len(kp), "inlier_ratio": 1.0, "model_score": 0.0, "inliers": []} for kp in k1]

    res = evalio.evaluate_calibrated(h5, ["p3p_hybrid+10"], iters=300, estimate_batch=stub)
    assert len(res) == 2 and res[0]["info"]["iterations"] == 10 and res[0]["R_err"] < 1e-6
