"""mdrp_refine_batch without a GPU: the yardstick (tests/from_models_ref.py) IS the estimator's tail, the header and the binding agree, and the
new kernel family keeps the register budget of the LM kernels (read from the code objects of the built library)."""
import os
import re
import sys

import numpy as np
import pytest

import from_models_ref as fm
import helpers
from oracle import pyorc as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.parametrize("name", helpers.OPTIONS_NAMES)
def test_the_yardstick_is_the_estimators_tail(name):
    """ransac<>'s winner on the normalised data, handed to the yardstick with stages = INLIERS, is the estimator's result: model to 1e-6, mask and
    inlier count identical"""
    kind, es, _ = helpers.OPTIONS_KINDS[name]
    p = helpers.edge_pair(name)
    cam = po.cam_flat(0, [800.0, 0.0, 0.0]) if kind == po.CALIB else None
    rod = dict(max_iterations=1000, min_iterations=1000, max_epipolar_error=2.0, max_reproj_error=16.0, seed=3, estimate_shift=es)
    ro, bo = po.ransac_opt(**rod), po.bundle_opt(max_iterations=100, loss_type=4, loss_scale=1.0, gradient_tol=1e-10)
    q = fm.prep(kind, p["x1"], p["x2"], ro, bo, cam, cam)
    ro_n = po.ransac_opt(**dict(rod, max_epipolar_error=q["eps"], max_reproj_error=q["rep"], weight_sampson=q["ws"]))
    winner, st_r, _ = po.ransac(kind, q["a1"], q["a2"], p["d1"], p["d2"], ro_n)
    winner[10:12] *= q["norm"]
    want, st, mask = po.estimate(kind, p["x1"], p["x2"], p["d1"], p["d2"], ro, bo, cam, cam)
    assert st.num_inliers > 150, st.num_inliers
    got = fm.refine_from_model(kind, p["x1"], p["x2"], p["d1"], p["d2"], winner, ro, bo, fm.STAGE_INLIERS, cam, cam)
    assert helpers.same_model(got["model"], want), helpers.model_diff(got["model"], want)
    assert np.array_equal(got["mask"], mask)
    assert got["num_inliers"] == st.num_inliers == got["initial_inliers"] and got["refinements"] == 1


def test_the_yardsticks_boundary_rules():
    """n < 3, a NaN start model and stages = 0 as the definition states them"""
    p = helpers.edge_pair("shared")
    ro, bo = po.ransac_opt(max_epipolar_error=2.0, max_reproj_error=16.0), po.bundle_opt(loss_type=4, gradient_tol=1e-10)
    m = po.new_model(); m[10:12] = p["f1"]
    r = fm.refine_from_model(po.SHARED, p["x1"][:2], p["x2"][:2], p["d1"][:2], p["d2"][:2], m, ro, bo, 3)
    assert r["model_score"] == fm.DBL_MAX == r["initial_score"] and r["refinements"] == 0 and not r["mask"].any() and np.array_equal(r["model"], m)
    nan = m.copy(); nan[:4] = np.nan
    r = fm.refine_from_model(po.SHARED, p["x1"], p["x2"], p["d1"], p["d2"], nan, ro, bo, 3)
    assert r["num_inliers"] == 0 and r["refinements"] == 0 and not r["mask"].any()
    assert abs(r["model_score"] - 300 * r["prep"]["sq_thr"]) <= 1e-12 * r["model_score"]  # (the oracle adds the threshold 300 times)
    assert np.array_equal(np.isnan(r["model"]), np.isnan(nan)) and np.array_equal(r["model"][4:], nan[4:])
    gt = np.r_[1.0, 0, 0, 0, p["t"], p["scale"], 0, 0, p["f1"], p["f2"]]
    r = fm.refine_from_model(po.SHARED, p["x1"], p["x2"], p["d1"], p["d2"], gt, ro, bo, 0)
    assert r["refinements"] == 0 and r["model"].tobytes() == gt.tobytes() and r["num_inliers"] == int(r["mask"].sum()) == r["initial_inliers"]


def _declaration(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, name
    return [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]


def test_header_and_binding_agree():
    from mdrp_amd import _capi, build
    hdr = open(os.path.join(ROOT, "include", "mdrp.h")).read()
    for name in ("mdrp_refine_batch", "mdrp_refine_batch_async", "MDRP_STAGE_LO", "MDRP_STAGE_INLIERS"):
        assert re.search(r"\b" + name + r"\b", hdr), name
    assert re.search(r"enum\s*\{\s*MDRP_STAGE_LO\s*=\s*1\s*,\s*MDRP_STAGE_INLIERS\s*=\s*2\s*\}", hdr)
    assert (_capi.STAGE_LO, _capi.STAGE_INLIERS) == (1, 2) == (fm.STAGE_LO, fm.STAGE_INLIERS)
    assert int(re.search(r"#define MDRP_ABI_VERSION (0x[0-9a-fA-F]+)", hdr).group(1), 16) == 6 == _capi.ABI_VERSION
    build.build()
    lib = _capi.load_library()
    assert lib.mdrp_abi_version() == 6
    for name in ("mdrp_refine_batch", "mdrp_refine_batch_async"):
        assert name in _capi.EXPORTS
        assert len(getattr(lib, name).argtypes) == len(_declaration(hdr, name)), name
    assert len(_declaration(hdr, "mdrp_refine_batch")) == 20 and len(_declaration(hdr, "mdrp_refine_batch_async")) == 18
    assert os.path.realpath(os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_from_model.h")) in [os.path.realpath(d) for d in build.DEPS]
    assert os.path.realpath(os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_tail.h")) in [os.path.realpath(d) for d in build.DEPS]


def test_kernel_family_and_resources():
    """four instantiations (kind x shift, one lane count, the loss read at run time), each within the LM kernels' budget: two wavefronts per SIMD,
    no AGPRs, no scratch access inside a record loop, and no more spilled VGPRs than the cap k_final is held to"""
    from mdrp_amd import build
    import kernel_table
    import spill_sites
    build.build()
    regs, sites = kernel_table.kernel_table(), spill_sites.spill_sites(only="k_from_model")
    fam = sorted(k for k in regs if k.startswith("mdrp::k_from_model<"))
    assert fam == ["mdrp::k_from_model<0, false>", "mdrp::k_from_model<0, true>", "mdrp::k_from_model<1, false>", "mdrp::k_from_model<2, false>"], fam
    for k in fam:
        r = regs[k]
        print(k, r, sites[k])
        assert r["vgpr"] <= 256 and r["waves_per_simd"] >= 2 and r.get("agpr", 0) == 0, (k, r)
        assert r.get("vgpr_spill", 0) <= 200, (k, r)
        assert sites[k]["scratch_in_sweep_loops"] == 0, (k, sites[k])
