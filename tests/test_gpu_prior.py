"""mdrp_estimate_batch_prior on a real MI355X: the estimators started from caller-supplied models (k_prior) against the yardstick (tests/prior_ref.py),
against the prior-free estimator where the two must coincide, over schedules, batch shapes and memory spaces, and at the boundary of the C ABI.
Inputs: the ragged batches of tests/from_models_cases.py (12 pairs, n = 0 .. 777, start models perturbed / exact / identity / NaN / hopeless) with
their start models as priors; options and yardstick answers from tests/prior_cases.py."""
import numpy as np
import pytest

import from_models_cases as fc
import helpers
import prior_cases as pc

pytestmark = pytest.mark.gpu

SCORE_RTOL = 1e-6  # as tests/test_gpu_from_models.py: the tolerance test_gpu_parity.py applies to model_score at same_model's 1e-6
KIND_NAMES = {0: "calibrated", 1: "shared_focal", 2: "varying_focal"}
KNOBS = ("MDRP_CHUNKS", "MDRP_LO_OVERLAP", "MDRP_BOUND", "MDRP_FUSE_TAIL", "MDRP_LO_THREADS", "MDRP_FINAL_THREADS", "MDRP_PAIRS_PER_PASS")
# Pairs exempt from a part of the comparison with the yardstick, by estimator: {pair index: (the fields it deviates in, cause)}; every other field of
# the pair is still compared.  A pair may stand here only if it deviates, and if the prior-free estimator deviates from po.estimate on the same pair
# in the same way (a class of DESIGN.md 5); at most one per estimator.  test_exemptions_are_earned checks both.
SCORE_TIE = "class (v) score_tie: N = 3 with a 3-point solver — every sample is the same three points, the winner fits them exactly, and its score " \
            "(1e-32 against a squared threshold of 1e-5) is the rounding of three zero residuals: no relative tolerance applies to it"
EXEMPT = {"calib_p3p": {2: (["model_score"], SCORE_TIE)}, "calib_shift": {}, "shared": {2: (["model_score"], SCORE_TIE)}, "varying": {}}


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


def _tiled(name, capi, tile):
    b = fc.batch(name)
    c1, c2 = fc.camera_records(b, capi)
    t = {k: np.ascontiguousarray(np.concatenate([b[k]] * tile)) for k in ("x1", "x2", "d1", "d2", "n")}
    t["c1"], t["c2"] = (None, None) if c1 is None else (np.concatenate([c1] * tile), np.concatenate([c2] * tile))
    return b, t


def _resident(name, capi, priors, tile=1, score_initial=False, **iters):
    """(records, masks) of the device-resident call through poselib.estimate_batch_torch; priors: [12 * tile] MODEL_DTYPE records or None"""
    import torch
    import mdrp_amd.poselib as poselib
    kind, es, _ = helpers.OPTIONS_KINDS[name]
    _, t = _tiled(name, capi, tile)
    dev = torch.device("cuda", 0)
    x = [torch.from_numpy(t[k]).to(dev) for k in ("x1", "x2", "d1", "d2")]
    ro = dict(fc.RO, monodepth_estimate_shift=es, score_initial_model=score_initial, **dict(pc.ITER, **iters))
    res, mask = poselib.estimate_batch_torch(KIND_NAMES[kind], *x, t["c1"], t["c2"], ro, {"loss_type": pc.LOSS}, n_per_pair=t["n"], priors=priors)
    return res, mask.cpu().numpy()


def _host(name, capi, handle, priors, tile=1, **iters):
    kind = helpers.OPTIONS_KINDS[name][0]
    _, t = _tiled(name, capi, tile)
    ro, bo = pc.library_options(name, capi, **iters)
    return handle.estimate_batch_prior(kind, t["x1"], t["x2"], t["d1"], t["d2"], priors, ro, bo, t["n"], t["c1"], t["c2"])


def _priors(name, capi, tile=1):
    return capi.array_to_models(np.concatenate([fc.batch(name)["models"]] * tile))


def _nan_priors(name, capi, which=None):
    m = fc.batch(name)["models"].copy()
    m[slice(None) if which is None else which, :4] = np.nan
    return capi.array_to_models(m)


def _deviation(capi, r, mask_row, w, n):
    """how a record differs from a yardstick / oracle answer w = dict(model, iterations, num_inliers, refinements, model_score, mask): a list of field names"""
    out = []
    if int(r["iterations"]) != w["iterations"]: out.append("iterations")
    if int(r["num_inliers"]) != w["num_inliers"]: out.append("num_inliers")
    if not (np.array_equal(mask_row[:n], w["mask"]) and not mask_row[n:].any()): out.append("mask")
    if not helpers.same_model(capi.model_to_array(r["model"]), w["model"]): out.append("model")
    if not abs(float(r["model_score"]) - w["model_score"]) <= SCORE_RTOL * abs(w["model_score"]): out.append("model_score")
    # a few dozen correspondences repeat samples and tie scores in the last bits (DESIGN.md 5 class v): the LO count may differ by one below N = 100,
    # exactly as tests/test_gpu_parity.py::test_batched_ragged_calls_under_random_options_vs_oracle allows
    if abs(int(r["refinements"]) - w["refinements"]) > (1 if n < 100 else 0): out.append("refinements")
    return out


def _against_the_yardstick(capi, name, res, mask, want, tag):
    b = fc.batch(name)
    exempt, compared = EXEMPT[name], 0
    assert len(exempt) <= 1
    for i, n in enumerate(b["n"]):
        r, w, n = res[i], want[i], int(n)
        dev = _deviation(capi, r, mask[i], w, n)
        print(tag, i, n, w["branch"], "iterations", int(r["iterations"]), w["iterations"], "inliers", int(r["num_inliers"]), w["num_inliers"], "LOs",
              int(r["refinements"]), w["refinements"], "score", float(r["model_score"]), w["model_score"], "model diff",
              helpers.model_diff(capi.model_to_array(r["model"]), w["model"]) if np.isfinite(w["model"]).all() else "nan", dev)
        assert [f for f in dev if i not in exempt or f not in exempt[i][0]] == [], (tag, i, n, dev)  # (test_exemptions_are_earned: that it deviates, and how)
        compared += 1
    assert compared == len(b["n"])  # no pair is left out


@pytest.mark.parametrize("iters", ((1000, 100), (0, 0), (50, 50)), ids=lambda v: f"i{v[0]}_{v[1]}")
@pytest.mark.parametrize("name", helpers.OPTIONS_NAMES)
def test_ragged_batch_against_the_yardstick(capi, name, iters):
    """B = 12: iterations, inlier counts and masks identical, models to 1e-6, LO counts equal (+-1 below N = 100); also with nothing sampled
    (max_iterations = 0: the loop ends behind the prior) and with a fixed 50 iterations"""
    mx, mn = iters
    res, mask = _resident(name, capi, _priors(name, capi), max_iterations=mx, min_iterations=mn)
    _against_the_yardstick(capi, name, res, mask, pc.yardstick(name, True, mx, mn), (name, iters))


@pytest.mark.parametrize("name", helpers.OPTIONS_NAMES)
def test_exemptions_are_earned(capi, name):
    """an exempt pair deviates from the yardstick, and the prior-free estimator deviates from po.estimate on the same pair in the same fields"""
    if not EXEMPT[name]:
        return
    res, mask = _resident(name, capi, _priors(name, capi))
    plain, pmask = _resident(name, capi, None)
    want, orc = pc.yardstick(name, True), pc.oracle_estimate(name)
    for i, (fields, cause) in EXEMPT[name].items():
        n = int(fc.batch(name)["n"][i])
        m, st, mk = orc[i]
        o = dict(model=m, iterations=st.iterations, num_inliers=st.num_inliers, refinements=st.refinements, model_score=st.model_score, mask=mk)
        with_prior, without = _deviation(capi, res[i], mask[i], want[i], n), _deviation(capi, plain[i], pmask[i], o, n)
        assert with_prior == fields == without, (name, i, cause, with_prior, without)


@pytest.mark.parametrize("name", helpers.OPTIONS_NAMES)
def test_without_priors_nothing_changes(capi, name):
    """bitwise: all-NaN priors are the prior-free call under score_initial_model false and true; identity-pose priors (scale 1, shifts 0, focals 1 in
    normalised units) are today's score_initial_model = True run, whatever the switch says"""
    for si in (False, True):
        want, wmask = _resident(name, capi, None, score_initial=si)
        got, gmask = _resident(name, capi, _nan_priors(name, capi), score_initial=si)
        assert got.tobytes() == want.tobytes() and np.array_equal(gmask, wmask), (name, si)
    assert int(want["refinements"].max()) > 2 and int(want["num_inliers"].max()) > 300
    for si in (False, True):
        got, gmask = _resident(name, capi, pc.identity_priors(name, capi), score_initial=si)
        for i in range(len(got)):
            assert got[i].tobytes() == want[i].tobytes(), (name, si, i, got[i], want[i])
        assert np.array_equal(gmask, wmask), (name, si)


@pytest.mark.parametrize("name", helpers.OPTIONS_NAMES)
def test_schedules_and_shapes(capi, handle, name, monkeypatch):
    """the 12 pairs tiled to B = 36 (k_score_w, with the fp32 bound), B = 132 (> SCORE_WAVE_MAX_PAIRS: k_score_split) and B = 516 through the blocking
    host-memory form (plain copies, never the sliced front): every tile the first tile's bytes, every pair on the yardstick; host = resident; several
    passes = one; every chunk schedule the same bytes"""
    want = pc.yardstick(name, True)
    for tile, host in ((3, False), (11, False), (43, True)):
        res, mask = _host(name, capi, handle, _priors(name, capi, tile), tile) if host else _resident(name, capi, _priors(name, capi, tile), tile)
        assert len(res) == 12 * tile
        for t in range(1, tile):
            assert res[12 * t:12 * t + 12].tobytes() == res[:12].tobytes() and np.array_equal(mask[12 * t:12 * t + 12], mask[:12]), (name, tile, t)
        _against_the_yardstick(capi, name, res[:12], mask[:12], want, (name, "B", 12 * tile, "host" if host else "resident"))
    ref, ref_mask = _resident(name, capi, _priors(name, capi))
    got, gmask = _host(name, capi, handle, _priors(name, capi))
    assert got.tobytes() == ref.tobytes() and np.array_equal(gmask, ref_mask), (name, "host form")
    for env in ({"MDRP_PAIRS_PER_PASS": "5"}, {"MDRP_CHUNKS": "0"}, {"MDRP_CHUNKS": "64"}, {"MDRP_CHUNKS": "64,256"}, {"MDRP_CHUNKS": "0", "MDRP_LO_OVERLAP": "0"}):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got, gmask = _resident(name, capi, _priors(name, capi))
        assert got.tobytes() == ref.tobytes() and np.array_equal(gmask, ref_mask), (name, env)


@pytest.mark.parametrize("name", helpers.OPTIONS_NAMES)
def test_mixed_batch(capi, name):
    """odd pairs without a prior (NaN): the even pairs are their records of the all-prior call, the odd pairs theirs of the prior-free call, bitwise"""
    all_p, all_mask = _resident(name, capi, _priors(name, capi))
    none, none_mask = _resident(name, capi, None)
    got, gmask = _resident(name, capi, _nan_priors(name, capi, slice(1, None, 2)))
    for i in range(12):
        w, wm = (none, none_mask) if i % 2 else (all_p, all_mask)
        assert got[i].tobytes() == w[i].tobytes() and np.array_equal(gmask[i], wm[i]), (name, i)
    assert all_p.tobytes() != none.tobytes()  # (the priors do change records)


def test_refusals_leave_the_handle_usable(capi):
    """kinds 3 - 5 and NULL priors: MDRP_ERR_INVALID; PROSAC: the estimator's own refusal; a valid call behind them returns what it returned before"""
    name = "calib_p3p"
    b = fc.batch(name)
    c1, c2 = fc.camera_records(b, capi)
    ro, bo = pc.library_options(name, capi)
    priors = _priors(name, capi)
    h = capi.Handle(0)
    args = (b["x1"], b["x2"], b["d1"], b["d2"])
    before = h.estimate_batch_prior(0, *args, priors, ro, bo, b["n"], c1, c2)
    for kind in (capi.RELPOSE_5PT, capi.SHARED_6PT, capi.FUNDAMENTAL_7PT, 17, -1):
        with pytest.raises(capi.MdrpError, match="mdrp error 1"):
            h.estimate_batch_prior(kind, *args, priors, ro, bo, b["n"], c1, c2)
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.estimate_batch_prior(0, *args, None, ro, bo, b["n"], c1, c2)
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.estimate_batch_prior(0, *args, priors, ro, bo, np.full(12, 778), c1, c2)
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.estimate_batch_prior(0, *args, priors, ro, bo, b["n"], None, None)
    prosac, _ = pc.library_options(name, capi, progressive_sampling=True)
    with pytest.raises(NotImplementedError):
        h.estimate_batch_prior(0, *args, priors, prosac, bo, b["n"], c1, c2)
    after = h.estimate_batch_prior(0, *args, priors, ro, bo, b["n"], c1, c2)
    assert after[0].tobytes() == before[0].tobytes() and np.array_equal(after[1], before[1]) and int(before[0]["num_inliers"].max()) > 300
    plain = h.estimate_batch(0, *args, ro, bo, b["n"], c1, c2)  # the prior-free estimator on the same handle, behind a call with priors
    want = capi.Handle(0).estimate_batch(0, *args, ro, bo, b["n"], c1, c2)
    assert plain[0].tobytes() == want[0].tobytes() and np.array_equal(plain[1], want[1])
    h.close()


def test_the_drop_in_functions(capi):
    """prior= / priors= of the poselib-style functions: the estimators' objects and info keys, on the yardstick's trajectory"""
    import mdrp_amd.poselib as poselib
    b = fc.batch("varying")
    want = pc.yardstick("varying", True)
    ro, bo = dict(fc.RO, **pc.ITER), {"loss_type": pc.LOSS}
    idx = [i for i, n in enumerate(b["n"]) if n >= 257]
    x1, x2, d1, d2 = ([b[k][i, :b["n"][i]] for i in idx] for k in ("x1", "x2", "d1", "d2"))
    pairs0 = [poselib.MonoDepthImagePair(poselib.MonoDepthTwoViewGeometry(poselib.CameraPose(v[:4], v[4:7]), v[7], v[8], v[9]),
                                         poselib.Camera("SIMPLE_PINHOLE", [v[10], 0.0, 0.0]), poselib.Camera("SIMPLE_PINHOLE", [v[11], 0.0, 0.0])) for v in b["models"][idx]]
    out, infos = poselib.estimate_monodepth_varying_focal_relative_pose_batch(x1, x2, d1, d2, ro, bo, priors=pairs0)
    for j, i in enumerate(idx):
        q = out[j]
        got = np.r_[q.geometry.pose.q, q.geometry.pose.t, q.geometry.scale, q.geometry.shift1, q.geometry.shift2, q.camera1.focal(), q.camera2.focal()]
        assert helpers.same_model(got, want[i]["model"]) and infos[j]["num_inliers"] == want[i]["num_inliers"] and infos[j]["iterations"] == want[i]["iterations"]
        assert infos[j]["refinements"] == want[i]["refinements"] and infos[j]["inliers"] == want[i]["mask"].astype(bool).tolist()
    one, info = poselib.estimate_monodepth_varying_focal_relative_pose(x1[0], x2[0], d1[0], d2[0], ro, bo, prior=pairs0[0])
    assert info["iterations"] == infos[0]["iterations"] and info["num_inliers"] == infos[0]["num_inliers"] and info["refinements"] == infos[0]["refinements"]
    got = np.r_[one.geometry.pose.q, one.geometry.pose.t, one.geometry.scale, one.geometry.shift1, one.geometry.shift2, one.camera1.focal(), one.camera2.focal()]
    assert helpers.same_model(got, want[idx[0]]["model"])
