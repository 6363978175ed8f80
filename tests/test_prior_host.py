"""mdrp_estimate_batch_prior without a GPU: the yardstick (tests/prior_ref.py) is pinned to the oracle where the two must agree, the inputs of the GPU tests
take every branch of the definition, the header and the binding agree, and the Python entry points check their arguments before any device work."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import from_models_cases as fc
import from_models_ref as fm
import helpers
import prior_cases as pc
import prior_ref as pr
from oracle import pyorc as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _same_as_oracle(r, m, st, mask, tag):
    assert r["model"].tobytes() == m.tobytes(), (tag, r["model"], m)
    assert (r["iterations"], r["refinements"], r["num_inliers"]) == (st.iterations, st.refinements, st.num_inliers), (tag, r["iterations"], r["refinements"])
    assert r["model_score"] == st.model_score and r["inlier_ratio"] == st.inlier_ratio, tag
    assert np.array_equal(r["mask"], mask), tag


@pytest.mark.parametrize("score_initial", (False, True))
@pytest.mark.parametrize("name", helpers.OPTIONS_NAMES)
def test_without_a_prior_the_yardstick_is_the_oracle(name, score_initial):
    """no prior: po.ransac on the normalised data and po.estimate on the pixels, bit for bit — model bytes, iterations, refinements, inliers, score, mask —
    on every size of the ragged batch the estimator runs on (n >= 3), under score_initial_model false and true; below 3 the estimators' empty record"""
    kind, es, _ = helpers.OPTIONS_KINDS[name]
    b = fc.batch(name)
    ro, bo = pc.oracle_options(name, score_initial)
    c1, c2 = pc._cams(b)
    for i, n in enumerate(b["n"]):
        x1, x2, d1, d2 = b["x1"][i, :n], b["x2"][i, :n], b["d1"][i, :n], b["d2"][i, :n]
        got = pr.estimate_from_prior(kind, x1, x2, d1, d2, ro, bo, None, c1, c2)
        if n < 3:
            assert got["model"].tobytes() == po.new_model().tobytes() and got["model_score"] == pr.DBL_MAX and not got["mask"].any()
            assert (got["iterations"], got["refinements"], got["num_inliers"], got["inlier_ratio"]) == (0, 0, 0, 0.0)
            continue
        _same_as_oracle(got, *po.estimate(kind, x1, x2, d1, d2, ro, bo, c1, c2), (name, "estimate", int(n)))
        q = fm.prep(kind, x1, x2, ro, bo, c1, c2)
        ro_n = po.ransac_opt(ro.max_iterations, ro.min_iterations, ro.dyn_num_trials_mult, ro.success_prob, q["rep"], q["eps"], ro.seed, es, q["ws"], score_initial)
        _same_as_oracle(pr.ransac_from_prior(kind, q["a1"], q["a2"], d1, d2, ro_n, None), *po.ransac(kind, q["a1"], q["a2"], d1, d2, ro_n), (name, "ransac", int(n)))
        nan = po.new_model(); nan[:4] = np.nan
        r = pr.estimate_from_prior(kind, x1, x2, d1, d2, ro, bo, nan, c1, c2)  # a NaN prior is no prior
        assert r["branch"] == "nan" and r["model"].tobytes() == got["model"].tobytes() and r["refinements"] == got["refinements"] and r["iterations"] == got["iterations"]


@pytest.mark.parametrize("name", helpers.OPTIONS_NAMES)
def test_the_identity_as_prior_is_the_oracles_scored_initial_model(name):
    """the identity model as initial model, not reset (it is what the reset gives): po.ransac(score_initial_model=True), bit for bit; and the switch is
    ignored by a pair that has a prior"""
    kind, es, _ = helpers.OPTIONS_KINDS[name]
    b = fc.batch(name)
    ro, bo = pc.oracle_options(name)
    c1, c2 = pc._cams(b)
    for i, n in enumerate(b["n"]):
        if n < 3:
            continue
        x1, x2, d1, d2 = b["x1"][i, :n], b["x2"][i, :n], b["d1"][i, :n], b["d2"][i, :n]
        q = fm.prep(kind, x1, x2, ro, bo, c1, c2)
        opts = [po.ransac_opt(ro.max_iterations, ro.min_iterations, ro.dyn_num_trials_mult, ro.success_prob, q["rep"], q["eps"], ro.seed, es, q["ws"], si) for si in (False, True)]
        want = po.ransac(kind, q["a1"], q["a2"], d1, d2, opts[1])
        for o in opts:
            got = pr.ransac_from_prior(kind, q["a1"], q["a2"], d1, d2, o, po.new_model())
            _same_as_oracle(got, *want, (name, int(n)))
            assert got["best_min"] == (0, q["sq_thr"] * n) or abs(got["best_min"][1] - q["sq_thr"] * n) <= 1e-12 * got["best_min"][1]


@pytest.mark.parametrize("name", helpers.OPTIONS_NAMES)
def test_the_inputs_of_the_gpu_tests_are_not_degenerate(name):
    """over the ragged batch with its start models as priors: every branch of the definition is taken, and a prior changes the trajectory of at
    least one pair"""
    b = fc.batch(name)
    with_p, without = pc.yardstick(name, True), pc.yardstick(name, False)
    seen = {r["branch"] for r in with_p}
    assert seen >= {"n<3", "nan", "lo_adopted", "lo_not_adopted"}, seen
    assert {r["branch"] for r in without} == {"n<3", "none"}
    differ = [int(n) for n, a, c in zip(b["n"], with_p, without) if (a["refinements"], a["iterations"]) != (c["refinements"], c["iterations"])]
    print(name, "branches", sorted(seen), "trajectory differs at n =", differ)
    assert differ
    for n, how in fc.RAGGED_START.items():
        i = fc.RAGGED_N.index(n)
        if how == "nan":  # no prior: the prior-free record
            assert with_p[i]["model"].tobytes() == without[i]["model"].tobytes() and with_p[i]["refinements"] == without[i]["refinements"]
        if how == "exact":  # the ground truth sets a bar no garbage sample passes
            assert with_p[i]["best_min"][0] > 0.5 * n and with_p[i]["refinements"] <= without[i]["refinements"]
    # max_iterations = 0: the loop ends behind the prior — the prior's LO and the closing LO, nothing sampled
    for r in pc.yardstick(name, True, 0, 0):
        assert r["iterations"] == 0 and r["refinements"] == {"n<3": 0, "nan": 1}.get(r["branch"], 2), (r["branch"], r["refinements"])


def test_the_dynamic_bound_of_the_yardstick():
    """f64_to_u64_x86 and the bound's edges, as the oracle's header states them"""
    assert pr.f64_to_u64_x86(float("inf")) == 0 and pr.f64_to_u64_x86(float("nan")) == 1 << 63 and pr.f64_to_u64_x86(-1.0) == 2 ** 64 - 1
    assert pr.f64_to_u64_x86(12.0) == 12 and pr.f64_to_u64_x86(2.0 ** 63) == 1 << 63 and pr.f64_to_u64_x86(-(2.0 ** 64)) == 1 << 63
    ro = po.ransac_opt(max_iterations=1000, min_iterations=100)
    lpm = np.log(1.0 - ro.success_prob)
    assert pr.dyn_max_iter(1.0, ro, lpm) == 100 and pr.dyn_max_iter(0.0, ro, lpm) == 1000
    assert pr.dyn_max_iter(0.5, ro, lpm) == int(np.ceil(lpm / np.log(1.0 - 0.125) * 3.0))


def _declaration(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, name
    return [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]


def test_header_and_binding_agree(tmp_path):
    """new symbols within ABI 6; the argument lists of the header, checked by a C compiler against the lists written out here, are the binding's"""
    from mdrp_amd import _capi, build
    hdr = open(os.path.join(ROOT, "include", "mdrp.h")).read()
    assert int(re.search(r"#define MDRP_ABI_VERSION (0x[0-9a-fA-F]+)", hdr).group(1), 16) == 6 == _capi.ABI_VERSION
    head = "mdrp_handle *, int, {}const double *, const double *, const double *, const double *, int, int, const int32_t *, const mdrp_camera *, const mdrp_camera *, " \
           "const mdrp_ransac_opt *, const mdrp_bundle_opt *, const mdrp_model *, "
    src = tmp_path / "abi.c"
    src.write_text('#include "mdrp.h"\n'
                   "typedef int (*blocking_t)(" + head.format("int, ") + "mdrp_result *, uint8_t *);\n"
                   "typedef int (*async_t)(" + head.format("") + "uint8_t *);\n"
                   "blocking_t a = mdrp_estimate_batch_prior;\nasync_t b = mdrp_estimate_batch_prior_async;\n")
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "abi.o")], check=True)
    build.build()
    lib = _capi.load_library()
    assert lib.mdrp_abi_version() == 6
    for name, count in (("mdrp_estimate_batch_prior", 17), ("mdrp_estimate_batch_prior_async", 15)):
        assert name in _capi.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(_declaration(hdr, name)) == count, name
    assert os.path.realpath(os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_prior.h")) in [os.path.realpath(d) for d in build.DEPS]


def test_kernel_family_and_resources():
    """four instantiations (kind x shift, one lane count), each within the LM kernels' budget: two wavefronts per SIMD, no AGPRs, no scratch access
    inside a record loop, and no more spilled VGPRs than the cap k_final and k_from_model are held to"""
    from mdrp_amd import build
    import kernel_table
    import spill_sites
    build.build()
    regs, sites = kernel_table.kernel_table(), spill_sites.spill_sites(only="k_prior")
    fam = sorted(k for k in regs if k.startswith("mdrp::k_prior<"))
    assert fam == ["mdrp::k_prior<0, false>", "mdrp::k_prior<0, true>", "mdrp::k_prior<1, false>", "mdrp::k_prior<2, false>"], fam
    for k in fam:
        r = regs[k]
        print(k, r, sites[k])
        assert r["vgpr"] <= 256 and r["waves_per_simd"] >= 2 and r.get("agpr", 0) == 0, (k, r)
        assert r.get("vgpr_spill", 0) <= 200, (k, r)
        assert sites[k]["scratch_in_sweep_loops"] == 0, (k, sites[k])


def test_python_argument_checks():
    """wrong length, wrong dtype, priors together with budgets: ValueError before any device work (no GPU here)"""
    import torch
    from mdrp_amd import _capi, poselib
    b = fc.batch("shared")
    x1, x2, d1, d2 = ([b[k][i, :n] for i, n in enumerate(b["n"])] for k in ("x1", "x2", "d1", "d2"))
    B = len(b["n"])
    good = _capi.array_to_models(b["models"])
    with pytest.raises(ValueError, match="priors and budgets"):
        poselib.estimate_monodepth_shared_focal_relative_pose_batch(x1, x2, d1, d2, {}, {}, budgets=[10, 20], priors=good)
    with pytest.raises(ValueError, match=f"expected {B} models, got {B - 1}"):
        poselib.estimate_monodepth_shared_focal_relative_pose_batch(x1, x2, d1, d2, {}, {}, priors=good[:-1])
    with pytest.raises(ValueError, match=f"expected {B} models, got 1"):
        poselib.estimate_monodepth_varying_focal_relative_pose_batch(x1, x2, d1, d2, {}, {}, priors=[None])
    with pytest.raises(ValueError, match="MODEL_DTYPE"):
        cam = {"model": "SIMPLE_PINHOLE", "width": 1600, "height": 1200, "params": [fc.F1, 0.0, 0.0]}
        poselib.estimate_monodepth_relative_pose_batch(x1, x2, d1, d2, cam, cam, {}, {}, priors=b["models"])  # (float64 (B, 12): not records)
    t = [torch.zeros((B, 8, 2), dtype=torch.float64), torch.zeros((B, 8, 2), dtype=torch.float64), torch.ones((B, 8), dtype=torch.float64), torch.ones((B, 8), dtype=torch.float64)]
    with pytest.raises(ValueError, match="priors and budgets"):
        poselib.estimate_batch_torch("shared_focal", *t, budgets=[10, 20], priors=good)
    with pytest.raises(ValueError, match="MODEL_DTYPE"):
        poselib.estimate_batch_torch("shared_focal", *t, priors=b["models"].astype(np.float32))
    with pytest.raises(ValueError, match=f"expected {B} models"):
        poselib.estimate_batch_torch("shared_focal", *t, priors=good[:3])
    with pytest.raises(ValueError, match="uint8 / float64"):
        poselib.estimate_batch_torch("shared_focal", *t, priors=torch.zeros((B, 12), dtype=torch.float32))
    with pytest.raises(ValueError, match=f"{B} records of 96 bytes"):
        poselib.estimate_batch_torch("shared_focal", *t, priors=torch.zeros((B, 11), dtype=torch.float64))
    # None entries are pairs without a prior: NaN records
    rec = poselib._prior_records([None, poselib.MonoDepthTwoViewGeometry(poselib.CameraPose([1.0, 0, 0, 0], [0.1, 0.2, 0.3]), 2.0, 0.0, 0.0)], _capi.CALIB, 2)
    assert np.isnan(rec[0]["q"]).all() and rec[1]["q"][0] == 1.0 and rec[1]["scale"] == 2.0 and rec[1]["f1"] == 1.0
