"""The baselines from a caller's model on a real MI355X (include/mdrp_classic_models.h): mdrp_refine_classic through kc_from_model and
mdrp_estimate_classic_prior through kc_prior against the yardstick (tests/classic_models_ref.py), against the estimators themselves where the two must
coincide, over schedules, batch shapes and memory spaces, and at the boundary of the C ABI.  Inputs and the yardstick's answers:
tests/classic_models_cases.py (12 ragged pairs, n = 0 .. 777, start models perturbed / exact / identity or random rank-2 F / NaN / hopeless)."""
import numpy as np
import pytest

import classic_models_cases as cc
import classic_models_ref as cm

pytestmark = pytest.mark.gpu

SCORE_RTOL = 1e-6  # tests/test_gpu_from_models.py's: the relative tolerance of model_score at the models' 1e-6
LOSS = "TRUNCATED_CAUCHY"
BIG = dict(n_list=(8200, 8100), first=84000, start=())  # over LM_LIST_MAX_N = 8192: no 16-bit work lists
KNOBS = ("MDRP_CHUNKS", "MDRP_LO_OVERLAP", "MDRP_BOUND", "MDRP_FUSE_TAIL", "MDRP_LO_THREADS", "MDRP_FINAL_THREADS", "MDRP_PAIRS_PER_PASS")
CAM1 = {"model": "SIMPLE_PINHOLE", "width": 1600, "height": 1200, "params": [cc.F, cc.PP[0], cc.PP[1]]}
CAM2 = {"model": "PINHOLE", "width": 1600, "height": 1200, "params": [cc.F * 1.01, cc.F * 0.99, cc.PP[0], cc.PP[1]]}


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


def _lead(kind):
    """what estimate_baseline_batch_torch / refine_baseline_batch_torch take behind the points and models: cameras1, cameras2, pp"""
    return (CAM1, CAM2, None) if kind == cm.FIVE else ((None, None, cc.PP) if kind == cm.SIX else (None, None, None))


# ---------------------------------------------------------------------------------------------------------------- mdrp_refine_classic
def _refine_against_the_yardstick(capi, handle, kind, loss, **kw):
    b = cc.batch(kind, **kw)
    B, K = len(b["n"]), cm.K_OF[kind]
    if not kw:  # the conditions on the inputs, from the yardstick alone
        assert cc.branches(kind, loss) >= {"lo_adopted", "lo_not_adopted", "inliers_skipped", "inliers_run", "nan", "n<K"} | ({"lo_skipped"} if kind != cm.SEVEN else set())
    else:
        assert cc.branches(kind, loss, **kw) >= {"inliers_run"}
    ro, bo = cc.library_options(loss, capi)
    c1, c2 = cc.camera_records(kind, b, capi)
    models = capi.array_to_models(b["models"])
    compared = 0
    for stages in (0, 1, 2, 3):
        want = cc.yardstick(kind, loss, stages, **kw)
        assert min(cc.threshold_margin(kind, r) for r in want) > 1e-6
        res, mask, score0, inl0 = handle.refine_classic(kind, b["x1"], b["x2"], models, ro, bo, stages, b["n"], c1, c2)
        for i, n in enumerate(b["n"]):
            r, w, tag = res[i], want[i], (kind, loss, stages, i, int(n))
            got = capi.model_to_array(r["model"])
            diff = cc.model_diff(kind, got, w["model"]) if np.isfinite(w["model"]).all() else float("nan")
            print(tag, "inliers", int(r["num_inliers"]), w["num_inliers"], "initial", int(inl0[i]), w["initial_inliers"], "LMs", int(r["refinements"]), w["refinements"],
                  "model diff", diff, "score", float(r["model_score"]), w["model_score"])
            assert np.array_equal(mask[i, :n], w["mask"]) and not mask[i, n:].any(), tag
            assert int(r["num_inliers"]) == w["num_inliers"] and int(inl0[i]) == w["initial_inliers"] and int(r["refinements"]) == w["refinements"], tag
            assert int(r["iterations"]) == 0 and float(r["inlier_ratio"]) == (w["num_inliers"] / n if n >= K else 0.0), tag
            if w["refinements"] == 0:
                assert r["model"].tobytes() == models[i].tobytes(), tag  # no stage ran: the caller's bytes
            else:
                assert diff < 1e-6, (tag, got, w["model"])
            assert abs(float(r["model_score"]) - w["model_score"]) <= SCORE_RTOL * abs(w["model_score"]), tag
            assert abs(float(score0[i]) - w["initial_score"]) <= SCORE_RTOL * abs(w["initial_score"]), tag
            compared += 1
    assert compared == 4 * B  # no pair is left out of any comparison


@pytest.mark.parametrize("loss", sorted(cc.LOSSES))
@pytest.mark.parametrize("kind", cc.KINDS)
def test_ragged_batch_against_the_yardstick(capi, handle, kind, loss):
    """B = 12 ragged pairs (n = 0 .. 777 = n_max: below the sample size, around one wavefront's 64, around one workgroup's 256, no multiple of
    anything), all four values of `stages`: masks, counts and `refinements` identical, iterations 0, models to 1e-6, scores to 1e-6 relative"""
    _refine_against_the_yardstick(capi, handle, kind, loss)


def test_beyond_the_16_bit_work_lists(capi, handle):
    """n_max = 8200 > LM_LIST_MAX_N for the 5-point kind: the LM sweeps visit every record of the LO's subset (stride 0) and read the masks"""
    _refine_against_the_yardstick(capi, handle, cm.FIVE, LOSS, **BIG)


@pytest.mark.parametrize("kind", cc.KINDS)
def test_inliers_stage_alone_at_the_count_rule(capi, handle, kind):
    """stages = INLIERS from a model with exactly K exact inliers among gross outliers, and with one more: the inlier-only refinement needs MORE than
    K, so `refinements` is 0, then 1 (tests/classic_models_cases.exact_inlier_batch; the yardstick confirms both counts)"""
    K = cm.K_OF[kind]
    counts = (K, K + 1)
    b = cc.exact_inlier_batch(kind, counts)
    want = cc.exact_inlier_yardstick(kind, LOSS, cm.STAGE_INLIERS, counts)
    assert [w["initial_inliers"] for w in want] == list(counts) and [w["refinements"] for w in want] == [0, 1]
    assert min(cc.threshold_margin(kind, w) for w in want) > 1e-6
    ro, bo = cc.library_options(LOSS, capi)
    c1, c2 = cc.camera_records(kind, b, capi)
    models = capi.array_to_models(b["models"])
    res, mask, score0, inl0 = handle.refine_classic(kind, b["x1"], b["x2"], models, ro, bo, cm.STAGE_INLIERS, b["n"], c1, c2)
    for i, w in enumerate(want):
        got = capi.model_to_array(res[i]["model"])
        print(kind, counts[i], "inliers", int(res[i]["num_inliers"]), int(inl0[i]), "LMs", int(res[i]["refinements"]), w["refinements"], "model diff",
              cc.model_diff(kind, got, w["model"]))
        assert int(inl0[i]) == counts[i] == int(res[i]["num_inliers"]) == int(mask[i].sum()) and np.array_equal(mask[i], w["mask"]), (kind, i)
        assert int(res[i]["refinements"]) == w["refinements"] == (0 if counts[i] == K else 1), (kind, i)
        assert cc.model_diff(kind, got, w["model"]) < 1e-6, (kind, i, got, w["model"])
    assert res[0]["model"].tobytes() == models[0].tobytes()  # no LM ran: bit for bit


def _torch_batch(first, B, N):
    import torch
    pairs = [cc.make_pair(first + i, N) for i in range(B)]
    host = {k: np.ascontiguousarray(np.stack([p[k] for p in pairs])) for k in ("x1", "x2")}
    dev = torch.device("cuda", 0)
    return pairs, host, [torch.from_numpy(host[k]).to(dev) for k in ("x1", "x2")]


@pytest.mark.parametrize("kind", cc.KINDS)
def test_anchor_to_the_estimator(capi, kind):
    """On the device alone: the estimator's records R, verified with stages = 0, come back bit for bit with a deterministic mask and the yardstick's
    inlier count for that model.  And the CPU anchor through the kernel: stages = INLIERS from the oracle's ransac winner is the oracle's estimate."""
    import mdrp_amd.poselib as poselib
    from oracle import pyorc as po
    name = cc.KIND_NAMES[kind]
    B, N = 2, 300
    pairs, host, t = _torch_batch(85000, B, N)
    its = cc.ITERATIONS[kind][0]
    ro = dict(max_iterations=its, min_iterations=its, max_epipolar_error=cc.THR, seed=3)
    bo = {"loss_type": LOSS}
    c1, c2, pp = _lead(kind)
    R, _ = poselib.estimate_baseline_batch_torch(name, *t, c1, c2, pp, ro, bo)
    res, mask, initial = poselib.refine_baseline_batch_torch(name, *t, R["model"].copy(), c1, c2, pp, ro, bo, stages=())
    res2, mask2, _ = poselib.refine_baseline_batch_torch(name, *t, R["model"].copy(), c1, c2, pp, ro, bo, stages=0)
    assert res["model"].tobytes() == R["model"].tobytes() and res.tobytes() == res2.tobytes()
    assert np.array_equal(mask.cpu().numpy(), mask2.cpu().numpy())
    oro, obo = cc.oracle_options(LOSS, its, its)
    b = dict(cams=cc.cameras(kind))
    k1, k2 = cc.oracle_cams(b)
    winners = np.zeros((B, 12))
    for i in range(B):
        w = cm.refine_from_model_classic(kind, host["x1"][i], host["x2"][i], capi.model_to_array(R[i]["model"]), oro, obo, 0, k1, k2, cc.PP)
        assert cc.threshold_margin(kind, w) > 1e-6
        assert int(res[i]["num_inliers"]) == w["num_inliers"] == int(initial["inliers"][i]) == int(mask[i].sum()) and int(res[i]["refinements"]) == 0, (kind, i)
        assert w["num_inliers"] > 150
        q = w["prep"]
        winner, _, _ = po.ransac_classic(kind, q["a1"], q["a2"], cm.normalised_options(oro, q))
        winners[i] = cm.to_caller_units(kind, winner, q)
    res, mask, _ = poselib.refine_baseline_batch_torch(name, *t, capi.array_to_models(winners), c1, c2, pp, ro, bo, stages=("inliers",))
    for i in range(B):
        want, st, wmask = po.estimate_classic(kind, host["x1"][i], host["x2"][i], oro, obo, k1, k2, cc.PP)
        assert cc.model_diff(kind, capi.model_to_array(res[i]["model"]), want) < 1e-6, (kind, i)
        assert np.array_equal(mask[i].cpu().numpy(), wmask) and int(res[i]["num_inliers"]) == st.num_inliers, (kind, i)


@pytest.mark.parametrize("kind", cc.KINDS)
def test_a_pairs_record_does_not_depend_on_its_batch_or_its_path(capi, kind):
    """alone, as element 0 and as element 5 of a batch of six, through host buffers and through device pointers: the same bytes"""
    import torch
    b = cc.batch(kind, n_list=(300, 290, 150, 64, 9, 299), first=86000, start=())
    ro, bo = cc.library_options(LOSS, capi)
    c1, c2 = cc.camera_records(kind, b, capi)
    models = capi.array_to_models(b["models"])
    h = capi.Handle(0)

    def host(order):
        o = list(order)
        return h.refine_classic(kind, b["x1"][o], b["x2"][o], models[o], ro, bo, 3, b["n"][o], None if c1 is None else c1[o], None if c2 is None else c2[o])

    alone = host([0])
    first = host([0, 1, 2, 3, 4, 5])
    last = host([1, 2, 3, 4, 5, 0])
    assert int(alone[0][0]["num_inliers"]) > 50 and int(alone[0][0]["refinements"]) == 2
    for got, at in ((first, 0), (last, 5)):
        assert got[0][at].tobytes() == alone[0][0].tobytes() and np.array_equal(got[1][at], alone[1][0])
        assert got[2][at] == alone[2][0] and got[3][at] == alone[3][0]
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(b[k])).to(dev) for k in ("x1", "x2")}
    mt = torch.from_numpy(models.view(np.uint8).reshape(6, 96).copy()).to(dev)
    mask = torch.zeros((6, 300), dtype=torch.uint8, device=dev)
    s0 = torch.zeros(6, dtype=torch.float64, device=dev)
    i0 = torch.zeros(6, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    h.refine_classic_device(kind, t["x1"].data_ptr(), t["x2"].data_ptr(), 6, 300, mt.data_ptr(), ro, bo, 3, b["n"], c1, c2, mask.data_ptr(), s0.data_ptr(),
                            i0.data_ptr())
    res = h.fetch_results(6)
    assert res.tobytes() == first[0].tobytes() and np.array_equal(mask.cpu().numpy(), first[1])
    assert np.array_equal(s0.cpu().numpy(), first[2]) and np.array_equal(i0.cpu().numpy(), first[3])
    # without a caller's mask the handle's own serves the LO: the same records
    h.refine_classic_device(kind, t["x1"].data_ptr(), t["x2"].data_ptr(), 6, 300, mt.data_ptr(), ro, bo, 3, b["n"], c1, c2)
    assert h.fetch_results(6).tobytes() == first[0].tobytes()
    h.close()


def test_default_stream_orders_with_a_producer_of_the_models(capi):
    """refine_baseline_batch_torch on torch's default stream, the models written by a torch op queued just before the call behind a chain of matrix
    products: the records are those of models that were there all along"""
    import torch
    import mdrp_amd.poselib as poselib
    b = cc.batch(cm.SEVEN, n_list=(300, 200, 250, 120), first=87000, start=())
    dev = torch.device("cuda", 0)
    assert torch.cuda.current_stream(dev).cuda_stream == 0
    t = [torch.from_numpy(np.ascontiguousarray(b[k])).to(dev) for k in ("x1", "x2")]
    ro, bo = dict(max_epipolar_error=cc.THR), {"loss_type": LOSS}
    want, wmask, winit = poselib.refine_baseline_batch_torch("fundamental_7pt", *t, capi.array_to_models(b["models"]), ransac_opt=ro, bundle_opt=bo, n_per_pair=b["n"])
    assert int((want["num_inliers"] > 30).sum()) >= 3 and int(want["refinements"].max()) == 2
    src = torch.from_numpy(b["models"]).to(dev)              # (B, 12) float64: the records' layout
    out = torch.full_like(src, float("nan"))                 # the models do not exist yet: poison
    big = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize()
    junk = big
    for _ in range(20):                                      # queued work in front of the producer
        junk = junk @ big
        junk = junk / junk.abs().max()
    torch.add(src, (junk[0, 0] * 0.0).double(), out=out)     # asynchronous producer of the models, data dependent on the chain
    res, mask, init = poselib.refine_baseline_batch_torch("fundamental_7pt", *t, out, ransac_opt=ro, bundle_opt=bo, n_per_pair=b["n"])
    assert res.tobytes() == want.tobytes() and np.array_equal(mask.cpu().numpy(), wmask.cpu().numpy())
    assert np.array_equal(init["score"], winit["score"]) and np.array_equal(init["inliers"], winit["inliers"])


# ---------------------------------------------------------------------------------------------------------------- mdrp_estimate_classic_prior
def _tiled(kind, capi, tile):
    b = cc.batch(kind)
    t = {k: np.ascontiguousarray(np.concatenate([b[k]] * tile)) for k in ("x1", "x2", "n")}
    return b, t


def _resident(kind, capi, priors, tile=1, score_initial=False, iters=None, prior_space=0):
    """(records, masks) of the device-resident call through poselib.estimate_baseline_batch_torch; priors: [12 * tile] MODEL_DTYPE records or None"""
    import torch
    import mdrp_amd.poselib as poselib
    _, t = _tiled(kind, capi, tile)
    dev = torch.device("cuda", 0)
    x = [torch.from_numpy(t[k]).to(dev) for k in ("x1", "x2")]
    mx, mn = cc.ITERATIONS[kind] if iters is None else iters
    ro = dict(max_epipolar_error=cc.THR, max_iterations=mx, min_iterations=mn, seed=3, score_initial_model=score_initial)
    res, mask = poselib.estimate_baseline_batch_torch(cc.KIND_NAMES[kind], *x, *_lead(kind), ro, {"loss_type": LOSS}, n_per_pair=t["n"], priors=priors,
                                                      prior_space=prior_space)
    return res, mask.cpu().numpy()


def _host(kind, capi, handle, priors, tile=1):
    b, t = _tiled(kind, capi, tile)
    ro, bo = cc.library_options(LOSS, capi, *cc.ITERATIONS[kind])
    c1, c2 = cc.camera_records(kind, b, capi, 12 * tile)
    return handle.estimate_classic_prior(kind, t["x1"], t["x2"], priors, ro, bo, t["n"], c1, c2)


def _priors(kind, capi, tile=1):
    return capi.array_to_models(np.concatenate([cc.batch(kind)["models"]] * tile))


def _nan_priors(kind, capi, which=None):
    m = cc.batch(kind)["models"].copy()
    m[slice(None) if which is None else which, 0] = np.nan
    return capi.array_to_models(m)


def _deviation(capi, kind, r, mask_row, w, n):
    """how a record differs from a yardstick answer w: a list of field names"""
    out = []
    if int(r["iterations"]) != w["iterations"]: out.append("iterations")
    if int(r["num_inliers"]) != w["num_inliers"]: out.append("num_inliers")
    if not (np.array_equal(mask_row[:n], w["mask"]) and not mask_row[n:].any()): out.append("mask")
    if n >= cm.K_OF[kind] and not cc.model_diff(kind, capi.model_to_array(r["model"]), w["model"]) < 1e-6: out.append("model")
    width = 9 if kind == cm.SEVEN else 12  # (a fundamental matrix is the record's first nine doubles)
    if n < cm.K_OF[kind] and capi.model_to_array(r["model"])[:width].tobytes() != w["model"][:width].tobytes(): out.append("model")
    # (the prior-free estimator's tests make the same allowance for the same reason: tests/test_gpu_prior.py EXEMPT / SCORE_TIE, DESIGN.md 5 class (v))
    # the score to 1e-6 relative, or to 1e-12 of its full scale n * threshold^2: with n = K every sample is the same K records, the winner fits them
    # exactly and its score (1e-31 against a squared threshold of 1e-5) is the rounding of K zero residuals, to which no relative tolerance applies
    floor = 1e-12 * n * w["prep"]["sq_thr"] if w.get("prep") else 0.0
    if not abs(float(r["model_score"]) - w["model_score"]) <= max(SCORE_RTOL * abs(w["model_score"]), floor): out.append("model_score")
    # a few dozen correspondences repeat samples and tie scores in the last bits: the LO count may differ by one below N = 100, exactly as the ragged
    # estimator tests allow (tests/test_gpu_parity.py, tests/test_gpu_prior.py)
    if abs(int(r["refinements"]) - w["refinements"]) > (1 if n < 100 else 0): out.append("refinements")
    return out


def _prior_against_the_yardstick(capi, kind, res, mask, want, tag, plain=None):
    """plain: (records, masks) of the prior-free estimator under the same options — what a pair WITHOUT a prior is held to, byte for byte, where given"""
    b = cc.batch(kind)
    compared = 0
    for i, n in enumerate(b["n"]):
        r, w, n = res[i], want[i], int(n)
        if plain is not None and w["branch"] in ("nan", "n<K"):
            assert r.tobytes() == plain[0][i].tobytes() and np.array_equal(mask[i], plain[1][i]), (tag, i, n, "a pair without a prior")
            compared += 1
            continue
        dev = _deviation(capi, kind, r, mask[i], w, n)
        print(tag, i, n, w["branch"], "iterations", int(r["iterations"]), w["iterations"], "inliers", int(r["num_inliers"]), w["num_inliers"], "LOs",
              int(r["refinements"]), w["refinements"], "score", float(r["model_score"]), w["model_score"], "model diff",
              cc.model_diff(kind, capi.model_to_array(r["model"]), w["model"]) if n >= cm.K_OF[kind] else "-", dev)
        assert dev == [], (tag, i, n, dev)
        compared += 1
    assert compared == len(b["n"])  # no pair is left out


@pytest.mark.parametrize("iters", ("long", (0, 0), (50, 50)), ids=lambda v: v if isinstance(v, str) else f"i{v[0]}_{v[1]}")
@pytest.mark.parametrize("kind", cc.KINDS)
def test_priors_against_the_yardstick(capi, kind, iters):
    """B = 12: iterations, inlier counts and masks identical, models to 1e-6, LO counts equal (+-1 below N = 100); at (200, 50) iterations — (100, 50)
    for the 6-point kind —, with nothing sampled (max_iterations = 0: the estimator's tail on the prior's state) and with a fixed 50 iterations.

    The 7-point kind's pair of exactly seven records has a single exact fit (tests/classic_models_cases.py FIRST): with three, the estimator and the
    oracle end on different roots of the cubic — all of them score the rounding of seven zero residuals — with or without a prior."""
    mx, mn = cc.ITERATIONS[kind] if iters == "long" else iters
    want = cc.prior_yardstick(kind, LOSS, mx, mn)
    assert min(cc.threshold_margin(kind, r) for r in want) > 1e-6
    res, mask = _resident(kind, capi, _priors(kind, capi), iters=(mx, mn))
    _prior_against_the_yardstick(capi, kind, res, mask, want, (kind, mx, mn))


@pytest.mark.parametrize("kind", cc.KINDS)
def test_a_pair_with_a_prior_ignores_score_initial_model(capi, kind):
    """real priors under score_initial_model = True against the yardstick under the same switch: kc_prep has left the scored identity's records and
    one refinement in the pair states, and kc_prior has to replace every one of them.  The pairs without a prior (NaN, n < K) are, as the header
    says, mdrp_estimate_batch's under the same switch, byte for byte (for the 7-point kind that is not the oracle's record: kc_prep sets no records
    for score_initial_model there)"""
    mx, mn = cc.ITERATIONS[kind]
    want = cc.prior_yardstick(kind, LOSS, mx, mn, score_initial=True)
    assert min(cc.threshold_margin(kind, r) for r in want) > 1e-6
    res, mask = _resident(kind, capi, _priors(kind, capi), score_initial=True, iters=(mx, mn))
    plain = _resident(kind, capi, None, score_initial=True, iters=(mx, mn))
    _prior_against_the_yardstick(capi, kind, res, mask, want, (kind, mx, mn, "score_initial_model"), plain)
    off, _ = _resident(kind, capi, _priors(kind, capi), iters=(mx, mn))
    i = cc.RAGGED_N.index(500)  # a pair with a prior: the switch changes nothing
    assert res[i].tobytes() == off[i].tobytes()


@pytest.mark.parametrize("kind", cc.KINDS)
def test_without_priors_nothing_changes(capi, kind):
    """bitwise: all-NaN priors are the prior-free estimator under score_initial_model false and true"""
    for si in (False, True):
        want, wmask = _resident(kind, capi, None, score_initial=si)
        got, gmask = _resident(kind, capi, _nan_priors(kind, capi), score_initial=si)
        assert got.tobytes() == want.tobytes() and np.array_equal(gmask, wmask), (kind, si)
    assert int(want["refinements"].max()) > 2 and int(want["num_inliers"].max()) > 300


@pytest.mark.parametrize("kind", cc.KINDS)
def test_mixed_batch_and_prior_space(capi, kind):
    """odd pairs without a prior (NaN): the even pairs are their records of the all-prior call, the odd pairs theirs of the prior-free call, bitwise.
    prior_space = 1 with records converted on the CPU: the models of prior_space = 0 to 1e-6, the counts equal"""
    from oracle import pyorc as po
    all_p, all_mask = _resident(kind, capi, _priors(kind, capi))
    none, none_mask = _resident(kind, capi, None)
    got, gmask = _resident(kind, capi, _nan_priors(kind, capi, slice(1, None, 2)))
    for i in range(12):
        w, wm = (none, none_mask) if i % 2 else (all_p, all_mask)
        assert got[i].tobytes() == w[i].tobytes() and np.array_equal(gmask[i], wm[i]), (kind, i)
    assert all_p.tobytes() != none.tobytes()  # (the priors do change records)
    b = cc.batch(kind)
    ro, bo = cc.oracle_options(LOSS)
    k1, k2 = cc.oracle_cams(b)
    conv = b["models"].copy()
    for i, n in enumerate(b["n"]):
        if n >= cm.K_OF[kind] and not np.isnan(conv[i, 0]):
            conv[i] = cm.to_estimator_units(kind, conv[i], cm.prep(kind, b["x1"][i, :n], b["x2"][i, :n], ro, bo, k1, k2, b["pp"]))
    got, gmask = _resident(kind, capi, capi.array_to_models(conv), prior_space=1)
    for i, n in enumerate(b["n"]):
        assert (int(got[i]["iterations"]), int(got[i]["num_inliers"]), int(got[i]["refinements"])) == \
               (int(all_p[i]["iterations"]), int(all_p[i]["num_inliers"]), int(all_p[i]["refinements"])), (kind, i)
        assert np.array_equal(gmask[i], all_mask[i]), (kind, i)
        if n >= cm.K_OF[kind]:
            assert cc.model_diff(kind, capi.model_to_array(got[i]["model"]), capi.model_to_array(all_p[i]["model"])) < 1e-6, (kind, i)
    if kind == cm.FIVE:  # identical to prior_space = 0
        assert got.tobytes() == all_p.tobytes()


@pytest.mark.parametrize("kind", cc.KINDS)
def test_schedules_and_shapes(capi, handle, kind, monkeypatch):
    """the 12 pairs tiled to B = 36: every tile the first tile's bytes, every pair on the yardstick; host = resident; several passes = one; every
    chunk schedule the same bytes"""
    want = cc.prior_yardstick(kind, LOSS, *cc.ITERATIONS[kind])
    res, mask = _resident(kind, capi, _priors(kind, capi, 3), 3)
    assert len(res) == 36
    for t in range(1, 3):
        assert res[12 * t:12 * t + 12].tobytes() == res[:12].tobytes() and np.array_equal(mask[12 * t:12 * t + 12], mask[:12]), (kind, t)
    ref, ref_mask = _resident(kind, capi, _priors(kind, capi))
    got, gmask = _host(kind, capi, handle, _priors(kind, capi))
    assert got.tobytes() == ref.tobytes() and np.array_equal(gmask, ref_mask), (kind, "host form")
    for env in ({"MDRP_PAIRS_PER_PASS": "5"}, {"MDRP_CHUNKS": "0"}, {"MDRP_CHUNKS": "64"}, {"MDRP_CHUNKS": "64,256"}, {"MDRP_CHUNKS": "0", "MDRP_LO_OVERLAP": "0"}):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got, gmask = _resident(kind, capi, _priors(kind, capi))
        assert got.tobytes() == ref.tobytes() and np.array_equal(gmask, ref_mask), (kind, env)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    _prior_against_the_yardstick(capi, kind, res[:12], mask[:12], want, (kind, "B", 36))


# ---------------------------------------------------------------------------------------------------------------- the boundary
def test_refusals_leave_the_handle_usable(capi):
    """everything the header lists as MDRP_ERR_INVALID, the estimator's own option refusals on the prior call and none of them on the refine call; a
    valid call behind them returns what it returned before"""
    kind = cm.FIVE
    b = cc.batch(kind)
    c1, c2 = cc.camera_records(kind, b, capi)
    ro, bo = cc.library_options(LOSS, capi, 50, 50)
    models = capi.array_to_models(b["models"])
    h = capi.Handle(0)
    x = (b["x1"], b["x2"])
    before_r = h.refine_classic(kind, *x, models, ro, bo, 3, b["n"], c1, c2)
    before_p = h.estimate_classic_prior(kind, *x, models, ro, bo, b["n"], c1, c2)
    for bad in (0, 1, 2, 6, 17, -1):
        with pytest.raises(capi.MdrpError, match="mdrp error 1"):
            h.refine_classic(bad, *x, models, ro, bo, 3, b["n"], c1, c2)
        with pytest.raises(capi.MdrpError, match="mdrp error 1"):
            h.estimate_classic_prior(bad, *x, models, ro, bo, b["n"], c1, c2)
    for stages in (4, -1):
        with pytest.raises(capi.MdrpError, match="mdrp error 1"):
            h.refine_classic(kind, *x, models, ro, bo, stages, b["n"], c1, c2)
    for call in (lambda m, n, a, c: h.refine_classic(kind, *x, m, ro, bo, 3, n, a, c), lambda m, n, a, c: h.estimate_classic_prior(kind, *x, m, ro, bo, n, a, c)):
        with pytest.raises(capi.MdrpError, match="mdrp error 1"):
            call(None, b["n"], c1, c2)                 # NULL models / prior
        with pytest.raises(capi.MdrpError, match="mdrp error 1"):
            call(models, np.full(12, 778), c1, c2)     # n_per_pair out of range
        with pytest.raises(capi.MdrpError, match="mdrp error 1"):
            call(models, b["n"], None, None)           # the 5-point kind without cameras
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.refine_classic(cm.SIX, *x, models, ro, bo, 3, b["n"], None, None)  # the 6-point kind without a principal point
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.estimate_classic_prior(cm.SIX, *x, models, ro, bo, b["n"], None, None)
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.estimate_classic_prior(kind, *x, models, ro, bo, b["n"], c1, c2, prior_space=2)
    prosac, _ = cc.library_options(LOSS, capi, 50, 50)
    prosac.progressive_sampling = 1
    with pytest.raises(NotImplementedError):
        h.estimate_classic_prior(kind, *x, models, prosac, bo, b["n"], c1, c2)
    focal = capi.ransac_opt_from_dict(dict(max_epipolar_error=cc.THR, max_iterations=50, min_iterations=50, real_focal_check=True))
    with pytest.raises(NotImplementedError):
        h.estimate_classic_prior(cm.SEVEN, *x, models, focal, bo, b["n"], None, None)
    # NULL correspondences and a NULL `out` of the blocking forms, past the binding
    import ctypes as C
    out, msk = np.zeros(12, dtype=capi.RESULT_DTYPE), np.zeros((12, 777), dtype=np.uint8)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    npp = np.ascontiguousarray(b["n"], dtype=np.int32)

    def raw_refine(x1, x2, o):
        return h._lib.mdrp_refine_classic(h._h, kind, capi.MEM_HOST, ptr(x1), ptr(x2), 12, 777, ptr(npp), ptr(c1), ptr(c2), C.byref(ro), C.byref(bo), ptr(models), 3,
                                          ptr(o), ptr(msk), None, None)

    def raw_prior(x1, x2, o):
        return h._lib.mdrp_estimate_classic_prior(h._h, kind, capi.MEM_HOST, ptr(x1), ptr(x2), 12, 777, ptr(npp), ptr(c1), ptr(c2), C.byref(ro), C.byref(bo), ptr(models), 0,
                                                  ptr(o), ptr(msk))

    for raw in (raw_refine, raw_prior):
        assert raw(None, b["x2"], out) == 1 and raw(b["x1"], None, out) == 1 and raw(b["x1"], b["x2"], None) == 1
        assert raw(b["x1"], b["x2"], out) == 0
    # the device-resident forms refuse the same, before any device work: nothing here is a device pointer
    for bad in (0, 2, 6, -1):
        with pytest.raises(capi.MdrpError, match="mdrp error 1"):
            h.refine_classic_device(bad, 8, 8, 12, 777, 8, ro, bo, 3, b["n"], c1, c2)
        with pytest.raises(capi.MdrpError, match="mdrp error 1"):
            h.estimate_classic_prior_device(bad, 8, 8, 12, 777, 8, ro, bo, b["n"], c1, c2)
    for args in ((None, 8, 8), (8, None, 8), (8, 8, None)):  # NULL x1, x2, models / prior
        with pytest.raises(capi.MdrpError, match="mdrp error 1"):
            h.refine_classic_device(kind, args[0], args[1], 12, 777, args[2], ro, bo, 3, b["n"], c1, c2)
        with pytest.raises(capi.MdrpError, match="mdrp error 1"):
            h.estimate_classic_prior_device(kind, args[0], args[1], 12, 777, args[2], ro, bo, b["n"], c1, c2)
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.refine_classic_device(kind, 8, 8, 12, 777, 8, ro, bo, 4, b["n"], c1, c2)                 # stages
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.refine_classic_device(kind, 8, 8, 12, 777, 8, ro, bo, 3, np.full(12, 778), c1, c2)       # n_per_pair
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.estimate_classic_prior_device(kind, 8, 8, 12, 777, 8, ro, bo, np.full(12, -1), c1, c2)
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.refine_classic_device(kind, 8, 8, 12, 777, 8, ro, bo, 3, b["n"], None, None)             # cameras
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.estimate_classic_prior_device(cm.SIX, 8, 8, 12, 777, 8, ro, bo, b["n"], None, None)      # principal point
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.estimate_classic_prior_device(kind, 8, 8, 12, 777, 8, ro, bo, b["n"], c1, c2, prior_space=-1)
    with pytest.raises(NotImplementedError):
        h.estimate_classic_prior_device(kind, 8, 8, 12, 777, 8, prosac, bo, b["n"], c1, c2)
    got = h.refine_classic(kind, *x, models, prosac, bo, 3, b["n"], c1, c2)  # nothing samples: nothing is refused
    assert got[0].tobytes() == before_r[0].tobytes()
    after_r = h.refine_classic(kind, *x, models, ro, bo, 3, b["n"], c1, c2)
    after_p = h.estimate_classic_prior(kind, *x, models, ro, bo, b["n"], c1, c2)
    for a, c in ((after_r, before_r), (after_p, before_p)):
        assert a[0].tobytes() == c[0].tobytes() and np.array_equal(a[1], c[1])
    assert int(before_r[0]["num_inliers"].max()) > 30 and int(before_p[0]["num_inliers"].max()) > 300
    plain = h.estimate_batch(kind, *x, None, None, ro, bo, b["n"], c1, c2)  # the prior-free estimator on the same handle, behind calls with models
    want = capi.Handle(0).estimate_batch(kind, *x, None, None, ro, bo, b["n"], c1, c2)
    assert plain[0].tobytes() == want[0].tobytes() and np.array_equal(plain[1], want[1])
    h.close()


def test_the_drop_in_functions(capi):
    """refine_baseline / refine_baseline_batch and prior= / priors= of the poselib-style functions: the estimators' objects and info keys, on the
    yardstick's answers"""
    import mdrp_amd.poselib as poselib
    ro, bo = dict(max_epipolar_error=cc.THR), {"loss_type": LOSS}
    for kind in cc.KINDS:
        b = cc.batch(kind)
        idx = [i for i, n in enumerate(b["n"]) if n in (500, 777)]
        x1, x2 = ([b[k][i, :b["n"][i]] for i in idx] for k in ("x1", "x2"))
        if kind == cm.FIVE:
            start = [poselib.CameraPose(v[:4], v[4:7]) for v in b["models"][idx]]
        elif kind == cm.SIX:
            start = [poselib.ImagePair(poselib.CameraPose(v[:4], v[4:7]), poselib.Camera("SIMPLE_PINHOLE", [v[10], *cc.PP]), poselib.Camera("SIMPLE_PINHOLE", [v[10], *cc.PP]))
                     for v in b["models"][idx]]
        else:
            start = [v[:9].reshape(3, 3) for v in b["models"][idx]]

        def flat(o):
            if kind == cm.SEVEN:
                return np.r_[np.asarray(o).reshape(-1), 0.0, 1.0, 1.0]
            pose = o if kind == cm.FIVE else o.pose
            f = 1.0 if kind == cm.FIVE else o.camera1.focal()
            return np.r_[pose.q, pose.t, 1.0, 0.0, 0.0, f, f]

        out, infos = poselib.refine_baseline_batch(cc.KIND_NAMES[kind], x1, x2, start, CAM1, CAM2, cc.PP, ro, bo)
        want = cc.yardstick(kind, LOSS, 3)
        for j, i in enumerate(idx):
            assert cc.model_diff(kind, flat(out[j]), want[i]["model"]) < 1e-6, (kind, i)
            assert set(infos[j]) == {"refinements", "iterations", "num_inliers", "inlier_ratio", "model_score", "inliers", "initial_score", "initial_inliers"}
            assert infos[j]["num_inliers"] == want[i]["num_inliers"] == sum(infos[j]["inliers"]) and infos[j]["initial_inliers"] == want[i]["initial_inliers"]
        one, info = poselib.refine_baseline(cc.KIND_NAMES[kind], x1[0], x2[0], start[0], CAM1, CAM2, cc.PP, ro, bo, stages=("lo",))
        w = cc.yardstick(kind, LOSS, 1)[idx[0]]
        assert cc.model_diff(kind, flat(one), w["model"]) < 1e-6 and info["num_inliers"] == w["num_inliers"] and info["refinements"] == 1
        mx, mn = cc.ITERATIONS[kind]
        rop = dict(ro, max_iterations=mx, min_iterations=mn, seed=3)
        wantp = cc.prior_yardstick(kind, LOSS, mx, mn)
        if kind == cm.FIVE:
            outp, infop = poselib.estimate_relative_pose_batch(x1, x2, CAM1, CAM2, rop, bo, priors=start)
            onep, info1 = poselib.estimate_relative_pose(x1[0], x2[0], CAM1, CAM2, rop, bo, prior=start[0])
        elif kind == cm.SIX:
            outp, infop = poselib.estimate_shared_focal_relative_pose_batch(x1, x2, cc.PP, rop, bo, priors=start)
            onep, info1 = poselib.estimate_shared_focal_relative_pose(x1[0], x2[0], cc.PP, rop, bo, prior=start[0])
        else:
            outp, infop = poselib.estimate_fundamental_batch(x1, x2, rop, bo, priors=start)
            onep, info1 = poselib.estimate_fundamental(x1[0], x2[0], rop, bo, prior=start[0])
        for j, i in enumerate(idx):
            assert cc.model_diff(kind, flat(outp[j]), wantp[i]["model"]) < 1e-6, (kind, i)
            assert (infop[j]["iterations"], infop[j]["num_inliers"], infop[j]["refinements"]) == (wantp[i]["iterations"], wantp[i]["num_inliers"], wantp[i]["refinements"])
            assert infop[j]["inliers"] == wantp[i]["mask"].astype(bool).tolist()
        assert (info1["iterations"], info1["num_inliers"], info1["refinements"]) == (infop[0]["iterations"], infop[0]["num_inliers"], infop[0]["refinements"])
        assert cc.model_diff(kind, flat(onep), wantp[idx[0]]["model"]) < 1e-6
