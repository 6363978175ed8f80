"""Estimating in match-score order on a real MI355X (mdrp_estimate_batch_ranked): the device sampler and the ranking kernel against the
reference binary's tables and the definition (tests/prosac_ref.py), the plumbing against today's estimator on pre-sorted inputs, the estimator
against the reference's PROSAC runs (tests/golden/prosac_ref.npz) and against the definition at the small end, refusals and the drop-in functions."""
import numpy as np
import pytest

import helpers
import prosac_cases as pcs
import prosac_ref as ps
from mdrp_amd import synth

pytestmark = pytest.mark.gpu

KNOBS = ("MDRP_CHUNKS", "MDRP_LO_OVERLAP", "MDRP_BOUND", "MDRP_FUSE_TAIL", "MDRP_LO_THREADS", "MDRP_FINAL_THREADS", "MDRP_PAIRS_PER_PASS", "MDRP_SAMPLE_THREADS")
BO = {"loss_type": pcs.LOSS, "gradient_tol": 1e-10}
# class (v) score_tie of tests/test_gpu_prior.py: N = 3 with a 3-point solver — every sample is the same three points, the winner fits them exactly and
# its score is the rounding of three zero residuals: no relative tolerance applies to model_score there
SCORE_TIE_N = 3


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


def _torch(kind, x1, x2, d1, d2, ro, n_per_pair=None, scores=None):
    """(records, masks (B, N) uint8 numpy) through poselib.estimate_batch_torch; scores: None (today's estimator), "presorted" or a (B, N) array"""
    import torch
    import mdrp_amd.poselib as poselib
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev) for a in (x1, x2, d1, d2)]
    sc = scores if scores is None or isinstance(scores, str) else torch.from_numpy(np.ascontiguousarray(scores)).to(dev)
    cams = (pcs.CAMERA, pcs.CAMERA) if kind == 0 else (None, None)
    res, mask = poselib.estimate_batch_torch(pcs.KIND_NAMES[kind], *t, *cams, ro, BO, n_per_pair=n_per_pair, **({} if scores is None else {"scores": sc}))
    return res, mask.cpu().numpy()


def _three(c, perm_seed=7):
    """the B = 3 batch of a case: the sorted records with all-equal scores (every rank its own index), the sorted records with their descending
    scores, and a shuffle of the records with the scores shuffled alike; the sorted records themselves; the order of every row"""
    o = c["order"]
    s = {k: c[k][o] for k in ("x1", "x2", "d1", "d2")}
    s_scores = c["scores"][o]
    perm = np.random.default_rng(perm_seed).permutation(c["n"])
    rows = {k: np.stack([s[k], s[k], s[k][perm]]) for k in s}
    scores = np.stack([np.zeros(c["n"]), s_scores, s_scores[perm]])
    orders = [ps.order(r) for r in scores]
    assert orders[0].tolist() == list(range(c["n"])) == orders[1].tolist() and np.array_equal(perm[orders[2]], np.arange(c["n"]))
    return rows, scores, s, orders


# ---- 1. the sampler
def _chunkings(count):
    cut = [1000, 1000, count - 2000] if count > 2000 else ([1000, count - 1000] if count > 1000 else [count])
    return [cut, [count]] if len(cut) > 1 else [cut, [max(count // 3, 1), count - max(count // 3, 1)]]


@pytest.mark.parametrize("row", range(len(pcs.SAMPLER_ROWS)))
def test_device_sampler_draws_the_reference_tables(handle, row):
    """mdrp_prosac_samples, chunk by chunk through the production launch: every index of the reference's table, with the carried (state, sample index)
    across chunk boundaries and the switch to uniform sampling inside a chunk and inside one speculative step"""
    n, seed, mp, count = pcs.SAMPLER_ROWS[row]
    want = pcs.golden()[f"samples_{row}"].astype(np.uint32)
    for lens in _chunkings(count):
        got = handle.prosac_samples(seed, n, mp, lens)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (row, lens, bad[:5], got[bad[:3]], want[bad[:3]])


def test_device_sampler_writes_nothing_below_three_records(handle):
    for n in (0, 1, 2):
        assert (handle.prosac_samples(0, n, 100000, [5, 5], fill=0xABCD) == 0xABCD).all()


# ---- 2. the ranking
def _rank_cases():
    rng = np.random.default_rng(11)
    ns = [0, 1, 2, 97, 300]
    ragged = np.floor(rng.uniform(0, 8, (len(ns), 300)))  # 8 levels: ties
    ragged[3, [5, 40, 41]] = np.nan; ragged[3, [6, 50]] = np.inf; ragged[3, [7, 60]] = -np.inf; ragged[3, [8, 9, 70]] = [-0.0, 0.0, -0.0]
    ragged[4, [0, 299, 150]] = np.nan; ragged[4, [1, 298]] = -np.inf; ragged[4, [2, 297]] = np.inf; ragged[4, [3, 4, 296, 295]] = [0.0, -0.0, -0.0, 0.0]
    ragged[4, 10] = np.float64(np.frombuffer(np.uint64(0xFFF8000000000001).tobytes(), dtype=np.float64)[0])  # a negative NaN with a payload
    mono = np.stack([np.full(130, 2.5), -np.arange(130, dtype=np.float64), np.arange(130, dtype=np.float64)])
    big = rng.normal(0, 1, (1, 5000)); big[0, ::7] = np.round(big[0, ::7])
    return [("ragged", ragged, ns), ("all-equal / decreasing / increasing", mono, None), ("n = 5000", big, None),
            ("one tile exactly and one past it", np.floor(rng.uniform(0, 50, (2, 2049))), [2048, 2049])]


def test_ranking_kernel_against_the_definition(capi, handle):
    """mdrp_rank_scores, host and device memory: descending, NaN = -inf, zeros tie, ties by index; -1 at and past n.  k_rank has one path for every n;
    its LDS tile holds 2048 keys: n = 2048, 2049 and 5000 cross it"""
    import torch
    for name, scores, ns in _rank_cases():
        B, N = scores.shape
        want = np.full((B, N), -1, dtype=np.int32)
        for b in range(B):
            n = N if ns is None else ns[b]
            want[b, :n] = ps.order(scores[b, :n])
        got = handle.rank_scores(scores, ns)
        assert np.array_equal(got, want), (name, "host", np.argwhere(got != want)[:5])
        d_scores = torch.from_numpy(scores).to("cuda:0")
        d_order = torch.full((B, N), -2, dtype=torch.int32, device="cuda:0")
        handle.rank_scores_device(d_scores.data_ptr(), B, N, d_order.data_ptr(), ns)
        assert np.array_equal(d_order.cpu().numpy(), want), (name, "device")
    mono = handle.rank_scores(_rank_cases()[1][1])
    assert mono[0].tolist() == list(range(130)) == mono[1].tolist() and mono[2].tolist() == list(range(129, -1, -1))


# ---- 3. the plumbing, independent of the sampler
@pytest.mark.parametrize("kind", (0, 1, 2))
def test_with_uniform_sampling_a_ranked_call_is_todays_estimator_on_sorted_inputs(kind):
    """max_prosac_iterations = 0 at case 6's shape: "presorted", identity ranking, descending scores and shuffled records all give the bytes of
    estimate_batch_torch on the sorted records; masks equal after un-permuting; mask bytes beyond n are zero"""
    c = pcs.case(kind, 6)
    n = c["n"]
    ro = pcs.ransac_dict(c)
    ro["max_prosac_iterations"] = 0
    rows, scores, s, orders = _three(c)
    want, wmask = _torch(kind, *(s[k][None] for k in ("x1", "x2", "d1", "d2")), ro)
    assert int(want[0]["num_inliers"]) > 30 and int(want[0]["refinements"]) > 1
    pre, pmask = _torch(kind, *(np.stack([s[k]] * 3) for k in ("x1", "x2", "d1", "d2")), ro, scores="presorted")
    got, gmask = _torch(kind, *(rows[k] for k in ("x1", "x2", "d1", "d2")), ro, scores=scores)
    for i in range(3):
        assert pre[i].tobytes() == want[0].tobytes() and np.array_equal(pmask[i], wmask[0]), (kind, "presorted", i)
        assert got[i].tobytes() == want[0].tobytes(), (kind, i, got[i], want[0])
        assert np.array_equal(gmask[i][orders[i]], wmask[0]), (kind, i)
    # padded: n_max = n + 31, float32 scores, progressive_sampling = True accepted
    pad = {k: np.concatenate([rows[k], np.ones((3, 31) + rows[k].shape[2:])], axis=1) for k in rows}
    sc32 = np.concatenate([scores, np.full((3, 31), 9.0)], axis=1)
    got, gmask = _torch(kind, *(pad[k] for k in ("x1", "x2", "d1", "d2")), dict(ro, progressive_sampling=True), n_per_pair=np.full(3, n, np.int32), scores=sc32)
    for i in range(3):
        assert got[i].tobytes() == want[0].tobytes() and np.array_equal(gmask[i][:n][orders[i]], wmask[0]) and not gmask[i][n:].any(), (kind, "padded", i)


# ---- 4. the estimator against the reference
@pytest.fixture(scope="module")
def lo_deviations():
    seen = {"cases": 0, "lo_only": []}
    yield seen
    print("cases compared:", seen["cases"], "deviating in the LO count alone:", seen["lo_only"])


@pytest.mark.parametrize("index", range(len(pcs.CASES)))
@pytest.mark.parametrize("kind", (0, 1, 2))
def test_against_the_reference_under_progressive_sampling(kind, index, lo_deviations):
    """each of the 27 fixture cases as one B = 3 call: three records with the same bytes; iterations, inlier counts and masks identical to the
    reference's, models to 1e-6, scores to SCORE_RTOL; LO counts under the +-1-below-100 convention, at most 2 of the 27 cases deviating in the LO
    count alone (the reference's shift and shared-focal solvers miss roots; the CPU definition deviates on none).  Where the reference's
    uniform result differs from its progressive one, so do the GPU's."""
    c = pcs.case(kind, index)
    n = c["n"]
    assert pcs.digest(c) == pcs.golden_case(kind, index)["digest"]
    ro = pcs.ransac_dict(c)
    rows, scores, s, orders = _three(c)
    got, gmask = _torch(kind, *(rows[k] for k in ("x1", "x2", "d1", "d2")), ro, scores=scores)
    assert got[1].tobytes() == got[0].tobytes() == got[2].tobytes(), (kind, index, got)
    for i in range(3):
        assert np.array_equal(gmask[i][orders[i]], gmask[0]), (kind, index, i)
    from mdrp_amd import _capi
    want = pcs.golden_answer(kind, index)
    mine = dict(model=_capi.model_to_array(got[0]["model"]), iterations=got[0]["iterations"], num_inliers=got[0]["num_inliers"], refinements=got[0]["refinements"],
                model_score=got[0]["model_score"], mask=gmask[0])
    dev = pcs.deviation(mine, want, n)
    print(kind, index, "LOs", int(mine["refinements"]), want["refinements"], "iterations", int(mine["iterations"]), want["iterations"], "inliers",
          int(mine["num_inliers"]), want["num_inliers"], "model diff", helpers.model_diff(mine["model"], want["model"]), dev)
    lo_deviations["cases"] += 1
    if dev == ["refinements"]:
        lo_deviations["lo_only"].append((kind, index, int(mine["refinements"]), want["refinements"]))
        print("LO count alone deviates:", lo_deviations["lo_only"])
        assert len(lo_deviations["lo_only"]) <= 2, lo_deviations["lo_only"]
    else:
        assert dev == [], (kind, index, dev)
    uni = pcs.golden_answer(kind, index, uniform=True)
    plain, _ = _torch(kind, *(s[k][None] for k in ("x1", "x2", "d1", "d2")), ro)
    assert pcs.deviation(dict(model=_capi.model_to_array(plain[0]["model"]), iterations=plain[0]["iterations"], num_inliers=plain[0]["num_inliers"],
                              refinements=plain[0]["refinements"], model_score=plain[0]["model_score"], mask=_[0]), uni, n) in ([], ["refinements"])
    if (uni["model"] != want["model"]).any() or uni["refinements"] != want["refinements"]:
        assert plain[0].tobytes() != got[0].tobytes(), (kind, index, "progressive sampling changed nothing")


# ---- 5. against the definition at the small end
SMALL_N = (3, 4, 7, 40, 64, 65, 97, 130)
SMALL_RO = dict(pcs.RO, max_iterations=200, min_iterations=50, max_prosac_iterations=100, seed=5)
# Pairs exempt from a part of the comparison, by the rule of tests/test_gpu_prior.py: {(kind, n): (fields, cause)}, at most one per estimator, and
# only where TODAY'S estimator (uniform sampling, the same records pre-sorted) deviates from the oracle on the same pair within the same class;
# every other field of the pair is still compared, and the test checks that the exemption is earned.  Measured on an MI355X (ranked | today's
# estimator, each against its CPU answer; everything not listed agrees, models to 4e-15):
#   calibrated n = 3: model_score 8.5e-32 | 1.7e-31 (the N = 3 class); today's estimator: another model (0.044), another score, LO count 2 | 4
#   calibrated n = 4: model 0.026 apart at scores equal to 12 digits (1.1588985407848e-08 | ...830e-08); today's estimator: 0.048 apart, same digits
#   shared     n = 3: model 8.2 apart (another exact root), scores 1.9e-31 | 1.3e-31; today's estimator: scores 1.5e-31 | 6.4e-32
SCORE_TIE = "class (v) score_tie of tests/test_gpu_prior.py: N = 3 with a 3-point solver — every sample is the same three points, every root fits them " \
            "exactly and its score is the rounding of three zero residuals: no relative tolerance applies to the score, and which root wins is that rounding"
SCALE_TIE = "the same class one record up: the Sampson score does not see the depth scale, so with 4 records models of different scale tie to 12 digits " \
            "and the winner is decided by the last bits; today's estimator deviates from the oracle on the same pair in the same field"
EXEMPT = {0: {4: (["model"], SCALE_TIE)}, 1: {3: (["model"], SCORE_TIE)}, 2: {}}


def _small(kind):
    N = max(SMALL_N)
    b = {"x1": np.zeros((len(SMALL_N), N, 2)), "x2": np.zeros((len(SMALL_N), N, 2)), "d1": np.ones((len(SMALL_N), N)), "d2": np.ones((len(SMALL_N), N)),
         "scores": np.zeros((len(SMALL_N), N))}
    for i, n in enumerate(SMALL_N):
        p = synth.make_pair(700 + 10 * kind + i, n, outlier_frac=0.3 if n > 7 else 0.0)
        for k in ("x1", "x2", "d1", "d2"):
            b[k][i, :n] = p[k]
        b["scores"][i, :n] = np.round(-(p["is_outlier"] + np.random.default_rng(i).normal(0.0, 0.6, n)), 1)  # (one decimal: ties)
    return b


def _record(capi, r, mask_row):
    return dict(model=capi.model_to_array(r["model"]), iterations=r["iterations"], num_inliers=r["num_inliers"], refinements=r["refinements"],
                model_score=r["model_score"], mask=mask_row)


@pytest.mark.parametrize("kind", (0, 1, 2))
def test_small_ragged_batch_against_the_definition(capi, kind, monkeypatch):
    """one ragged B = 8 call with n = 3 .. 130 (the subset grows to n and the sampler turns uniform at sample 99 of 200) against prosac_ref.estimate:
    iterations, inlier counts and masks identical, models to 1e-6, scores to SCORE_RTOL but for the N = 3 score-tie class, LO counts equal (+-1 below
    N = 100); the same bytes under schedules that force several chunks, super-chunks and passes.  EXEMPT above lists the two pairs on which the winner
    among tied models differs, and each is checked to be earned."""
    import prior_ref as pr
    from oracle import pyorc as po
    b = _small(kind)
    ns = np.array(SMALL_N, dtype=np.int32)
    got, gmask = _torch(kind, b["x1"], b["x2"], b["d1"], b["d2"], SMALL_RO, n_per_pair=ns, scores=b["scores"])
    ro = po.ransac_opt(200, 50, pcs.RO["dyn_num_trials_mult"], pcs.RO["success_prob"], pcs.RO["max_reproj_error"], pcs.RO["max_epipolar_error"], 5, False,
                       pcs.RO["monodepth_weight_sampson"])
    bo = po.bundle_opt(max_iterations=100, loss_type=4, loss_scale=1.0, gradient_tol=1e-10)
    cam = po.cam_flat(0, [pcs.FOCAL, 0.0, 0.0])
    cams = (cam, cam) if kind == 0 else (None, None)
    assert len(EXEMPT[kind]) <= 1
    for i, n in enumerate(SMALL_N):
        row = {k: b[k][i, :n] for k in ("x1", "x2", "d1", "d2")}
        w = ps.estimate(kind, row["x1"], row["x2"], row["d1"], row["d2"], b["scores"][i, :n], ro, bo, 100, *cams)
        mine = _record(capi, got[i], gmask[i])
        dev = pcs.deviation(mine, w, n)
        print(kind, n, "LOs", int(mine["refinements"]), w["refinements"], "iterations", int(mine["iterations"]), w["iterations"], "inliers", int(mine["num_inliers"]),
              w["num_inliers"], "score", float(mine["model_score"]), w["model_score"], "model diff", helpers.model_diff(mine["model"], w["model"]), dev)
        allowed = (["model_score"] if n == SCORE_TIE_N else []) + (EXEMPT[kind][n][0] if n in EXEMPT[kind] else [])
        assert [f for f in dev if f not in allowed] == [], (kind, n, dev)
        assert not gmask[i][n:].any()
        if n in EXEMPT[kind]:  # earned: it deviates here, and today's estimator deviates from the oracle on the same records, in the tie's fields
            fields, cause = EXEMPT[kind][n]
            assert set(fields) <= set(dev), (kind, n, "the exemption is not needed", dev)
            o = w["order"]
            plain, pmask = _torch(kind, *(row[k][o][None] for k in ("x1", "x2", "d1", "d2")), SMALL_RO)
            u = pr.estimate_from_prior(kind, row["x1"][o], row["x2"][o], row["d1"][o], row["d2"][o], ro, bo, None, *cams)
            pdev = pcs.deviation(_record(capi, plain[0], pmask[0]), u, n)
            print("   today's estimator on the same records deviates from the oracle in", pdev, "—", cause)
            assert pdev and set(pdev) <= {"model", "model_score", "refinements"}, (kind, n, pdev)
    for env in ({"MDRP_CHUNKS": "16,32", "MDRP_PAIRS_PER_PASS": "3"}, {"MDRP_CHUNKS": "", "MDRP_LO_OVERLAP": "0"}, {"MDRP_CHUNKS": "7,9,11", "MDRP_SAMPLE_THREADS": "64"}):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        again, amask = _torch(kind, b["x1"], b["x2"], b["d1"], b["d2"], SMALL_RO, n_per_pair=ns, scores=b["scores"])
        assert again.tobytes() == got.tobytes() and np.array_equal(amask, gmask), (kind, env)


# ---- 6. refusals
def test_refusals_leave_the_handle_usable(capi):
    """kinds 3 - 5: MDRP_ERR_INVALID; NULL depths and n_per_pair out of range as the prior entry refuses them; a valid call behind them returns what
    it returned before; progressive_sampling = True without scores still raises, with a message that names scores="""
    import mdrp_amd.poselib as poselib
    c = pcs.case(0, 6)
    n = c["n"]
    x1, x2, d1, d2, sc = (c[k][None] for k in ("x1", "x2", "d1", "d2", "scores"))
    ro, bo = capi.ransac_opt_from_dict(pcs.ransac_dict(c, progressive_sampling=True)), capi.bundle_opt_from_dict(BO)
    cam = poselib._camera_records(pcs.CAMERA, 1)
    h = capi.Handle(0)
    before = h.estimate_batch_ranked(0, x1, x2, d1, d2, sc, ro, bo, None, cam, cam)
    for kind in (capi.RELPOSE_5PT, capi.SHARED_6PT, capi.FUNDAMENTAL_7PT, 17, -1):
        with pytest.raises(capi.MdrpError, match="mdrp error 1"):
            h.estimate_batch_ranked(kind, x1, x2, d1, d2, sc, ro, bo, None, cam, cam)
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.estimate_batch_ranked(0, x1, x2, None, None, sc, ro, bo, None, cam, cam)
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.estimate_batch_ranked(0, x1, x2, d1, d2, sc, ro, bo, np.array([n + 1], np.int32), cam, cam)
    with pytest.raises(capi.MdrpError, match="mdrp error 1"):
        h.estimate_batch_ranked(0, x1, x2, d1, d2, sc, ro, bo, None, None, None)
    with pytest.raises(NotImplementedError, match="scores="):
        h.estimate_batch(0, x1, x2, d1, d2, ro, bo, None, cam, cam)
    with pytest.raises(NotImplementedError, match="PROSAC"):
        poselib.estimate_monodepth_relative_pose(c["x1"], c["x2"], c["d1"], c["d2"], pcs.CAMERA, pcs.CAMERA, pcs.ransac_dict(c, progressive_sampling=True), BO)
    after = h.estimate_batch_ranked(0, x1, x2, d1, d2, sc, ro, bo, None, cam, cam)
    assert after[0].tobytes() == before[0].tobytes() and np.array_equal(after[1], before[1]) and int(before[0]["num_inliers"][0]) > 30
    plain_ro = capi.ransac_opt_from_dict(pcs.ransac_dict(c))
    plain = h.estimate_batch(0, x1, x2, d1, d2, plain_ro, bo, None, cam, cam)  # today's estimator on the same handle, behind ranked calls
    want = capi.Handle(0).estimate_batch(0, x1, x2, d1, d2, plain_ro, bo, None, cam, cam)
    assert plain[0].tobytes() == want[0].tobytes() and np.array_equal(plain[1], want[1])
    h.close()


# ---- 7. the drop-in functions
@pytest.mark.parametrize("kind", (0, 1, 2))
def test_the_drop_in_functions(capi, handle, kind):
    """scores= of the single-pair and batch forms, and the blocking C entry on host buffers: the records of estimate_batch_torch, info["inliers"] in the
    caller's order"""
    import mdrp_amd.poselib as poselib
    cases = [pcs.case(kind, 3), pcs.case(kind, 7)]
    ro = pcs.ransac_dict(cases[0])
    N = max(c["n"] for c in cases)
    pad = {k: np.stack([np.concatenate([c[k], np.ones((N - c["n"],) + c[k].shape[1:])]) for c in cases]) for k in ("x1", "x2", "d1", "d2")}
    sc = np.stack([np.concatenate([c["scores"], np.full(N - c["n"], -np.inf)]) for c in cases])
    ns = np.array([c["n"] for c in cases], dtype=np.int32)
    want, wmask = _torch(kind, pad["x1"], pad["x2"], pad["d1"], pad["d2"], ro, n_per_pair=ns, scores=sc)
    cam = poselib._camera_records(pcs.CAMERA, 2) if kind == 0 else None
    host, hmask = handle.estimate_batch_ranked(kind, pad["x1"], pad["x2"], pad["d1"], pad["d2"], sc, capi.ransac_opt_from_dict(ro), capi.bundle_opt_from_dict(BO), ns, cam, cam)
    assert host.tobytes() == want.tobytes() and np.array_equal(hmask, wmask)
    batch_fn = (poselib.estimate_monodepth_relative_pose_batch, poselib.estimate_monodepth_shared_focal_relative_pose_batch,
                poselib.estimate_monodepth_varying_focal_relative_pose_batch)[kind]
    one_fn = (poselib.estimate_monodepth_relative_pose, poselib.estimate_monodepth_shared_focal_relative_pose, poselib.estimate_monodepth_varying_focal_relative_pose)[kind]
    cams = (pcs.CAMERA, pcs.CAMERA) if kind == 0 else ()
    args = [[c[k] for c in cases] for k in ("x1", "x2", "d1", "d2")]
    res, masks, _ = batch_fn(*args, *cams, ro, BO, as_arrays=True, scores=[c["scores"] for c in cases])
    assert res.tobytes() == want.tobytes() and np.array_equal(masks, wmask)
    objs, infos = batch_fn(*args, *cams, ro, BO, scores=[c["scores"] for c in cases])
    for i, c in enumerate(cases):
        assert infos[i]["inliers"] == wmask[i, :c["n"]].astype(bool).tolist() and infos[i]["num_inliers"] == int(want[i]["num_inliers"])
        one, info = one_fn(c["x1"], c["x2"], c["d1"], c["d2"], *cams, ro, BO, scores=c["scores"])
        assert info["iterations"] == int(want[i]["iterations"]) and info["refinements"] == int(want[i]["refinements"]) and info["inliers"] == infos[i]["inliers"]
        o = c["order"]
        pre, pinfo = one_fn(c["x1"][o], c["x2"][o], c["d1"][o], c["d2"][o], *cams, ro, BO, scores="presorted")
        assert pinfo["iterations"] == info["iterations"] and pinfo["refinements"] == info["refinements"] and pinfo["inliers"] == np.asarray(info["inliers"])[o].tolist()
