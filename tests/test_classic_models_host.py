"""The baselines from a caller's model without a GPU (include/mdrp_classic_models.h): the yardstick (tests/classic_models_ref.py) is pinned to the
oracle where the two must agree, the inputs of the GPU tests take every branch of the definition, the header, the binding and the build agree, the
new kernel families keep the budget of kc_lo and kc_final, and the Python entry points check their arguments before any device work."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import classic_models_cases as cc
import classic_models_ref as cm
from oracle import pyorc as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LOSS = "TRUNCATED_CAUCHY"
NAMES = ("mdrp_refine_classic", "mdrp_refine_classic_async", "mdrp_estimate_classic_prior", "mdrp_estimate_classic_prior_async")


def _same_as_oracle(r, m, st, mask, tag):
    assert r["model"].tobytes() == m.tobytes(), (tag, r["model"], m)
    assert (r["iterations"], r["refinements"], r["num_inliers"]) == (st.iterations, st.refinements, st.num_inliers), (tag, r["iterations"], r["refinements"])
    assert r["model_score"] == st.model_score and r["inlier_ratio"] == st.inlier_ratio, tag
    assert np.array_equal(r["mask"], mask), tag


@pytest.mark.parametrize("score_initial", (False, True))
@pytest.mark.parametrize("kind", cc.KINDS)
def test_without_a_prior_the_yardstick_is_the_oracle(kind, score_initial):
    """no prior: po.ransac_classic on the normalised data and po.estimate_classic on the pixels, bit for bit — model bytes, iterations, refinements,
    inliers, score, mask — on every size of the ragged batch the estimator runs on (n >= K), under score_initial_model false and true; below K the
    estimators' empty record; a NaN prior is no prior"""
    b = cc.batch(kind)
    ro, bo = cc.oracle_options(LOSS, *cc.ITERATIONS[kind], score_initial)
    c1, c2 = cc.oracle_cams(b)
    for i, n in enumerate(b["n"]):
        x1, x2 = b["x1"][i, :n], b["x2"][i, :n]
        got = cm.estimate_from_prior_classic(kind, x1, x2, ro, bo, None, c1, c2, b["pp"])
        if n < cm.K_OF[kind]:
            assert got["model"].tobytes() == po.classic_blob(kind).tobytes() and got["model_score"] == cm.DBL_MAX and not got["mask"].any()
            assert (got["iterations"], got["refinements"], got["num_inliers"], got["inlier_ratio"]) == (0, 0, 0, 0.0)
            continue
        _same_as_oracle(got, *po.estimate_classic(kind, x1, x2, ro, bo, c1, c2, b["pp"]), (kind, "estimate", int(n)))
        q = cm.prep(kind, x1, x2, ro, bo, c1, c2, b["pp"])
        ro_n = cm.normalised_options(ro, q)
        _same_as_oracle(cm.ransac_from_prior_classic(kind, q["a1"], q["a2"], ro_n, None), *po.ransac_classic(kind, q["a1"], q["a2"], ro_n), (kind, "ransac", int(n)))
        nan = po.classic_blob(kind); nan[0] = np.nan
        r = cm.estimate_from_prior_classic(kind, x1, x2, ro, bo, nan, c1, c2, b["pp"])
        assert r["branch"] == "nan" and r["model"].tobytes() == got["model"].tobytes() and (r["refinements"], r["iterations"]) == (got["refinements"], got["iterations"])


@pytest.mark.parametrize("kind", cc.KINDS)
def test_stage_inliers_alone_is_the_estimators_tail(kind):
    """po.ransac_classic's winner on the normalised data, handed to the yardstick in the caller's units with stages = INLIERS, is po.estimate_classic's
    result: model to 1e-6, mask and inlier count identical"""
    b = cc.batch(kind)
    i = list(b["n"]).index(500)
    x1, x2 = b["x1"][i, :500], b["x2"][i, :500]
    ro, bo = cc.oracle_options(LOSS, *cc.ITERATIONS[kind])
    c1, c2 = cc.oracle_cams(b)
    q = cm.prep(kind, x1, x2, ro, bo, c1, c2, b["pp"])
    winner, _, _ = po.ransac_classic(kind, q["a1"], q["a2"], cm.normalised_options(ro, q))
    want, st, mask = po.estimate_classic(kind, x1, x2, ro, bo, c1, c2, b["pp"])
    assert st.num_inliers > 250, st.num_inliers
    got = cm.refine_from_model_classic(kind, x1, x2, cm.to_caller_units(kind, winner, q), ro, bo, cm.STAGE_INLIERS, c1, c2, b["pp"])
    assert cc.model_diff(kind, got["model"], want) < 1e-6, cc.model_diff(kind, got["model"], want)
    assert np.array_equal(got["mask"], mask)
    assert got["num_inliers"] == st.num_inliers == got["initial_inliers"] and got["refinements"] == 1


def test_the_conversions_are_inverse_to_each_other_and_the_boundary_rules():
    """to_estimator_units and to_caller_units round-trip (F up to scale); n < K, a NaN model and stages = 0 as the header states them"""
    for kind in cc.KINDS:
        b = cc.batch(kind)
        i = list(b["n"]).index(500)
        x1, x2, m = b["x1"][i, :500], b["x2"][i, :500], b["models"][i]
        ro, bo = cc.oracle_options(LOSS)
        c1, c2 = cc.oracle_cams(b)
        q = cm.prep(kind, x1, x2, ro, bo, c1, c2, b["pp"])
        back = cm.to_caller_units(kind, cm.to_estimator_units(kind, m, q), q)
        assert cc.model_diff(kind, back, m) < 1e-12
        assert cm.to_estimator_units(kind, m, q, 1).tobytes() == m.tobytes()
        K = cm.K_OF[kind]
        r = cm.refine_from_model_classic(kind, x1[:K - 1], x2[:K - 1], m, ro, bo, 3, c1, c2, b["pp"])
        assert r["model_score"] == cm.DBL_MAX == r["initial_score"] and r["refinements"] == 0 and not r["mask"].any() and r["model"].tobytes() == m.tobytes()
        nan = m.copy(); nan[0] = np.nan
        r = cm.refine_from_model_classic(kind, x1, x2, nan, ro, bo, 3, c1, c2, b["pp"])
        assert r["num_inliers"] == 0 and r["refinements"] == 0 and not r["mask"].any() and r["model_score"] == 500 * q["sq_thr"] == r["initial_score"]
        assert r["model"].tobytes() == nan.tobytes()
        r = cm.refine_from_model_classic(kind, x1, x2, m, ro, bo, 0, c1, c2, b["pp"])
        assert r["refinements"] == 0 and r["model"].tobytes() == m.tobytes() and r["num_inliers"] == int(r["mask"].sum()) == r["initial_inliers"]


@pytest.mark.parametrize("kind", cc.KINDS)
def test_the_inputs_of_the_gpu_tests_are_not_degenerate(kind):
    """over the ragged batch with its start models: every branch of both definitions is taken, a prior changes the trajectory of at least one pair, the
    7-point start matrices have distinct singular values, and no correspondence of a compared model lies within 1e-6 of its threshold"""
    b = cc.batch(kind)
    K = cm.K_OF[kind]
    seen = cc.branches(kind, LOSS)
    want = {"n<K", "nan", "lo_adopted", "lo_not_adopted", "inliers_run", "inliers_skipped"} | ({"lo_skipped"} if kind != cm.SEVEN else set())
    assert seen >= want, (seen, want)
    for i, n in enumerate(b["n"]):
        if kind == cm.SEVEN and not np.isnan(b["models"][i][0]):
            assert cc.singular_value_gap(b["models"][i][:9]) > 1e-3, int(n)
    its = cc.ITERATIONS[kind]
    with_p, without = cc.prior_yardstick(kind, LOSS, *its), cc.prior_yardstick(kind, LOSS, *its, with_prior=False)
    assert {r["branch"] for r in with_p} >= {"n<K", "nan", "lo_adopted", "lo_not_adopted"}, {r["branch"] for r in with_p}
    assert {r["branch"] for r in without} == {"n<K", "none"}
    differ = [int(n) for n, a, c in zip(b["n"], with_p, without) if (a["refinements"], a["iterations"]) != (c["refinements"], c["iterations"])]
    print(kind, "refine branches", sorted(seen), "prior branches", sorted({r["branch"] for r in with_p}), "trajectory differs at n =", differ)
    assert differ
    i = cc.RAGGED_N.index(255)  # the NaN record: the prior-free run
    assert with_p[i]["model"].tobytes() == without[i]["model"].tobytes() and with_p[i]["refinements"] == without[i]["refinements"]
    i = cc.RAGGED_N.index(63)   # the ground truth sets a bar few samples pass
    assert with_p[i]["best_min"][0] > 0.5 * 63 and with_p[i]["refinements"] <= without[i]["refinements"]
    # max_iterations = 0: the loop ends behind the prior — the prior's LO and the closing LO, nothing sampled
    for r in cc.prior_yardstick(kind, LOSS, 0, 0):
        assert r["iterations"] == 0 and r["refinements"] == {"n<K": 0, "nan": 1}.get(r["branch"], 2), (r["branch"], r["refinements"])
    # the pairs without redundancy (n <= 8): the yardstick's own answer stands still, two orders below the 1e-6 the device is compared at, when the
    # inputs move by 1e-13 relative — where it does not (most sets of exactly 7 records for the 7-point kind), no comparison of models means anything
    for mx, mn in (its, (0, 0), (50, 50)):
        moved = cc.prior_sensitivity(kind, LOSS, mx, mn)
        print(kind, (mx, mn), "the yardstick under a 1e-13 perturbation", moved)
        assert len(moved) >= 2 and max(moved.values()) < 1e-8, (kind, mx, mn, moved)
    if kind == cm.SEVEN:  # seven records: one real root of the cubic, or the winner among three exact fits is the rounding of zero residuals
        assert cc.exact_fits(kind, LOSS) == {1}, cc.exact_fits(kind, LOSS)
    margins = [cc.threshold_margin(kind, r) for loss in cc.LOSSES for st in range(4) for r in cc.yardstick(kind, loss, st)]
    margins += [cc.threshold_margin(kind, r) for mx, mn in (its, (0, 0), (50, 50)) for r in cc.prior_yardstick(kind, LOSS, mx, mn)]
    assert min(margins) > 1e-6, min(margins)
    assert all(n >= K or r["prep"] is None for n, r in zip(b["n"], cc.yardstick(kind, LOSS, 3)))


def _declaration(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, name
    return [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]


def test_header_binding_and_build_agree(tmp_path):
    """four new symbols within ABI 6, declared in an extension header mdrp.h includes; the header's argument lists, checked by a C compiler against the
    lists written out here, are the binding's; a C host that includes mdrp.h alone links against the four symbols"""
    from mdrp_amd import _capi, build
    main = open(os.path.join(ROOT, "include", "mdrp.h")).read()
    assert int(re.search(r"#define MDRP_ABI_VERSION (0x[0-9a-fA-F]+)", main).group(1), 16) == 6 == _capi.ABI_VERSION
    assert '#include "mdrp_classic_models.h"' in main
    assert main.index('#include "mdrp_classic_ranked.h"') < main.index('#include "mdrp_classic_models.h"')
    for name in NAMES:  # declared in the extension header only: tests/history_cases.py enumerates mdrp.h's own entry points
        assert not re.search(r"\b" + name + r"\s*\(", main), name
    path = os.path.join(ROOT, "include", "mdrp_classic_models.h")
    hdr = open(path).read()
    deps = [os.path.realpath(d) for d in build.DEPS]
    assert os.path.realpath(path) in deps and os.path.realpath(os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_classic_models.h")) in deps
    assert sorted(_capi.EXPORTS_CLASSIC_MODELS) == sorted(NAMES) == sorted(set(re.findall(r"\b(mdrp_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))))
    assert not set(_capi.EXPORTS_CLASSIC_MODELS) & (set(_capi.EXPORTS) | set(_capi.EXPORTS_CLASSIC_RANKED))
    head = "mdrp_handle *, int, {}const double *, const double *, int, int, const int32_t *, const mdrp_camera *, const mdrp_camera *, " \
           "const mdrp_ransac_opt *, const mdrp_bundle_opt *, const mdrp_model *, int, "
    src = tmp_path / "abi.c"
    src.write_text('#include "mdrp.h"\n'
                   "typedef int (*refine_t)(" + head.format("int, ") + "mdrp_result *, uint8_t *, double *, int32_t *);\n"
                   "typedef int (*refine_async_t)(" + head.format("") + "uint8_t *, double *, int32_t *);\n"
                   "typedef int (*prior_t)(" + head.format("int, ") + "mdrp_result *, uint8_t *);\n"
                   "typedef int (*prior_async_t)(" + head.format("") + "uint8_t *);\n"
                   "refine_t a = mdrp_refine_classic;\nrefine_async_t b = mdrp_refine_classic_async;\n"
                   "prior_t c = mdrp_estimate_classic_prior;\nprior_async_t d = mdrp_estimate_classic_prior_async;\n"
                   "_Static_assert(sizeof(mdrp_ransac_opt) == 88, \"mdrp_ransac_opt\");\n"
                   "int main(void) { return (a && b && c && d) ? 0 : 1; }\n")
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "abi.o")], check=True)
    build.build()
    lib = _capi.load_library()
    assert lib.mdrp_abi_version() == 6
    # the object links against the built library: the four symbols are exported (the HIP runtime's symbols stay open, as in the library itself)
    subprocess.run(["gcc", str(tmp_path / "abi.o"), "-o", str(tmp_path / "abi"), build.OUT, "-Wl,--unresolved-symbols=ignore-in-shared-libs"], check=True)
    for name, count in zip(NAMES, (18, 16, 16, 14)):
        assert hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(_declaration(hdr, name)) == count, name
    for name in ("refine_classic", "refine_classic_device", "estimate_classic_prior", "estimate_classic_prior_device"):
        assert callable(getattr(_capi.Handle, name))


def test_every_entry_point_of_the_extension_header_is_in_its_history_table():
    """tests/test_history_host.py's rule for include/mdrp_classic_models.h: every function with a handle is run by tests/classic_models_history_cases.py,
    whose inputs are deterministic"""
    import classic_history_cases as chc
    import classic_models_history_cases as mhc
    import helpers
    import history_cases as hc
    named = {p for c in mhc.probes() for p in c.entry_points}
    assert set(mhc.extension_entry_points()) == set(NAMES) <= named
    assert {c.kind for c in mhc.probes()} == {3, 4, 5} and {c.device for c in mhc.probes()} == {False, True}
    assert {c.family for c in mhc.probes()} == {"prior", "refine"}
    assert not {c.name for c in mhc.probes()} & ({c.name for c in hc.predecessors()} | {c.name for c in chc.probes()})
    for c in mhc.probes() + tuple(x for pair in mhc.back_to_back() for x in pair):
        a, b = (helpers.input_digest(hc.four(c.digest_arrays(c.make()))) for _ in range(2))
        assert a == b, c


def test_kernel_families_and_resources():
    """three instantiations each (one lane count, the loss read at run time), within the budget tests/test_kernel_resources.py sets for kc_lo and
    kc_final: no AGPRs, at most 256 VGPRs, two wavefronts per SIMD, no scratch access inside a record loop — and no spilled VGPR at all"""
    from mdrp_amd import build
    import kernel_table
    import spill_sites
    build.build()
    regs = kernel_table.kernel_table()
    for family in ("kc_from_model", "kc_prior"):
        sites = spill_sites.spill_sites(only=family)
        fam = sorted(k for k in regs if k.startswith(f"mdrp::{family}<"))
        assert fam == [f"mdrp::{family}<{k}>" for k in (3, 4, 5)], fam
        for k in fam:
            r = regs[k]
            print(k, r, sites[k])
            assert r["vgpr"] <= 256 and r["waves_per_simd"] >= 2 and r.get("agpr", 0) == 0 and r.get("vgpr_spill", 0) == 0, (k, r)
            assert sites[k]["scratch_in_sweep_loops"] == 0, (k, sites[k])


def test_python_argument_checks():
    """a wrong kind, priors with budgets or scores, a wrong number of models, a wrong model type: ValueError before any device work (no GPU here)"""
    import torch
    from mdrp_amd import _capi, poselib
    n, B = 8, 2
    x1, x2 = [np.zeros((n, 2))] * B, [np.zeros((n, 2))] * B
    cam = {"model": "SIMPLE_PINHOLE", "width": 1600, "height": 1200, "params": [800.0, 640.0, 480.0]}
    pose, pair, Fm = poselib.CameraPose(), poselib.ImagePair(), np.eye(3)
    for fn, lead, good, wrong in ((poselib.estimate_relative_pose_batch, (cam, cam), pose, Fm),
                                  (poselib.estimate_shared_focal_relative_pose_batch, ((0.0, 0.0),), pair, pose),
                                  (poselib.estimate_fundamental_batch, (), Fm, pose)):
        with pytest.raises(ValueError, match="priors and budgets"):
            fn(x1, x2, *lead, {"max_iterations": 20}, {}, budgets=[10, 20], priors=[good] * B)
        with pytest.raises(ValueError, match="scores do not combine"):
            fn(x1, x2, *lead, {}, {}, scores="presorted", priors=[good] * B)
        with pytest.raises(ValueError, match=f"expected {B} models, got 1"):
            fn(x1, x2, *lead, {}, {}, priors=[good])
        with pytest.raises(ValueError, match="pair 1 needs"):
            fn(x1, x2, *lead, {}, {}, priors=[None, wrong])
        with pytest.raises(ValueError, match="one model per pair"):
            fn(x1, x2, *lead, {}, {}, priors=np.zeros((B, 12)))  # (float64 (B, 12): not records)
    with pytest.raises(ValueError, match="pair 0 needs a 3 x 3"):
        poselib.estimate_fundamental(x1[0], x2[0], {}, {}, prior=np.eye(4))
    with pytest.raises(ValueError, match="pair 0 needs a CameraPose"):
        poselib.estimate_relative_pose(x1[0], x2[0], cam, cam, {}, {}, prior=pair)
    with pytest.raises(ValueError, match="pair 0 needs an ImagePair"):
        poselib.estimate_shared_focal_relative_pose(x1[0], x2[0], (0.0, 0.0), {}, {}, prior=Fm)
    with pytest.raises(ValueError, match="initial_F and prior"):
        poselib.estimate_fundamental(x1[0], x2[0], {}, {}, initial_F=Fm, prior=Fm)
    with pytest.raises(ValueError, match="scores do not combine"):
        poselib.estimate_fundamental(x1[0], x2[0], {}, {}, initial_F=Fm, scores="presorted")
    with pytest.raises(ValueError, match="pair 0 needs a 3 x 3"):
        poselib.estimate_fundamental(x1[0], x2[0], {}, {}, initial_F=np.eye(4))
    # refine_baseline*: the kind, the number and the type of the models
    with pytest.raises(ValueError, match="kind"):
        poselib.refine_baseline_batch("calibrated", x1, x2, [pose] * B, cam, cam)
    with pytest.raises(ValueError, match="kind"):
        poselib.refine_baseline_batch(3, x1, x2, [pose] * B, cam, cam)
    with pytest.raises(ValueError, match=f"expected {B} models, got 3"):
        poselib.refine_baseline_batch("relpose_5pt", x1, x2, [pose] * 3, cam, cam)
    with pytest.raises(ValueError, match="pair 0 needs a 3 x 3"):
        poselib.refine_baseline_batch("fundamental_7pt", x1, x2, [pose] * B)
    with pytest.raises(ValueError, match="every pair needs a model"):
        poselib.refine_baseline_batch("fundamental_7pt", x1, x2, [Fm, None])
    with pytest.raises(ValueError, match="stages must be drawn"):
        poselib.refine_baseline_batch("fundamental_7pt", x1, x2, [Fm] * B, stages=("final",))
    with pytest.raises(ValueError, match="model is required"):
        poselib.refine_baseline("shared_focal_6pt", x1[0], x2[0], None)
    assert not hasattr(poselib, "refine_relative_pose") and not hasattr(poselib, "refine_fundamental")  # (upstream's names mean a plain LM: DESIGN.md 7b)
    t = [torch.zeros((B, n, 2), dtype=torch.float64), torch.zeros((B, n, 2), dtype=torch.float64)]
    good = np.zeros(B, dtype=_capi.MODEL_DTYPE)
    for kind in cc.KIND_NAMES.values():
        with pytest.raises(ValueError, match="scores do not combine"):
            poselib.estimate_baseline_batch_torch(kind, *t, cam, cam, scores="presorted", priors=good)
        with pytest.raises(ValueError, match="GPU"):
            poselib.refine_baseline_batch_torch(kind, *t, good, cam, cam)  # (host tensors)
    with pytest.raises(ValueError, match="kind"):
        poselib.refine_baseline_batch_torch("varying_focal", *t, good)
    with pytest.raises(ValueError, match=r"\(B, N, 2\)"):
        poselib.refine_baseline_batch_torch("fundamental_7pt", torch.zeros((B, n), dtype=torch.float64), t[1], good)
