"""A run's first chunk retires by the prefix records of a few hypotheses scored first (k_first_pick / k_first_score / k_first_filter, mdrp_kernels.h;
calls of more than 128 pairs, 3-point estimators).  The stage is scheduling only: whole estimates with it on and with it forced off give byte-identical
result records and inlier masks.  It is forced off through its own knob, MDRP_FIRST_PICK=0 (MDRP_CHUNKS set empty would also remove the second
chunk, and with it everything the stage runs beside).  Eight pairs of the same calls are anchored to the CPU oracle (oracle/pyorc.py) by the criteria
of tests/test_gpu_parity.py::test_batch_ragged_and_degenerate: iterations, inlier count and mask identical, model within 1e-6."""
import functools

import numpy as np
import pytest

from helpers import model_diff
from oracle import pyorc as po

B = 130                         # just above SCORE_WAVE_MAX_PAIRS = 128 (mdrp_kernels.h): the smallest call that takes the stage
NS = (3, 40, 257, 600)          # correspondences, cycling over the pairs: one sample only | less than a record tile | one past a tile | several tiles
NMAX = max(NS)
TWO = 7                         # the pair with two correspondences: no sample, never active
DEGENERATE = 11                 # the pair whose every sample is the same correspondence three times: no hypothesis, or NaN models only
OUTLIERS = (0.0, 0.5, 0.9)      # by pair index
ITS = 600                       # max = min: a first chunk of 128 iterations and a second chunk behind it
RF = {1: "shared", 2: "varying"}
RO = {"max_epipolar_error": 2.0, "max_reproj_error": 16.0}
BO = {"loss_type": "TRUNCATED_CAUCHY"}
MODEL_TOL = 1e-6                # tests/test_gpu_parity.py: the model against the oracle
ORACLE_PAIRS = (1, 2, 3, 5, 6, 9, 10, 129)  # n = 40, 257, 600 at 0 / 50 / 90 % outliers, and the call's last pair
CASES = [(0, False), (0, True), (1, False), (2, False)]
KNOBS = ("MDRP_FIRST_PICK", "MDRP_SOLVE_RESIDENT", "MDRP_CHUNKS", "MDRP_LO_OVERLAP", "MDRP_BOUND", "MDRP_FUSE_TAIL", "MDRP_SCORE_SPLIT")


@functools.lru_cache(maxsize=None)
def _inputs(kind):
    from mdrp_amd import _capi, synth
    ns = np.array([NS[i % len(NS)] for i in range(B)], dtype=np.int32)
    ns[TWO] = 2
    ns[DEGENERATE] = 40
    x1, x2 = np.zeros((B, NMAX, 2)), np.zeros((B, NMAX, 2))
    d1, d2 = np.ones((B, NMAX)), np.ones((B, NMAX))
    for i in range(B):
        n = int(ns[i])
        p = synth.make_pair(77000 + 1000 * kind + i, max(n, 3), noise_px=0.5, depth_noise=0.02, outlier_frac=OUTLIERS[i % 3], random_focal=RF.get(kind))
        x1[i, :n], x2[i, :n], d1[i, :n], d2[i, :n] = p["x1"][:n], p["x2"][:n], p["d1"][:n], p["d2"][:n]
    for a in (x1, x2, d1, d2):
        a[DEGENERATE, :40] = a[DEGENERATE, :1]
    cams = np.zeros(B, dtype=_capi.CAMERA_DTYPE)
    cams["params"][:, 0] = 800.0    # SIMPLE_PINHOLE f (synth's default focal), principal point 0
    return ns, x1, x2, d1, d2, cams


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _run(h, monkeypatch, kind, shift, env, max_it=ITS, min_it=ITS):
    from mdrp_amd import _capi
    ns, x1, x2, d1, d2, cams = _inputs(kind)
    c = cams if kind == 0 else None
    ro = _capi.ransac_opt_from_dict(dict(RO, max_iterations=max_it, min_iterations=min_it, monodepth_estimate_shift=shift))
    _env(monkeypatch, env)
    res, mask = h.estimate_batch(kind, x1, x2, d1, d2, ro, _capi.bundle_opt_from_dict(BO), ns, c, c)
    return res.copy(), mask.copy(), h.last_stats()


def test_the_inputs_hold_what_the_cases_need():
    """(no GPU) every n at every outlier fraction, the two special pairs, and oracle pairs that are ordinary"""
    ns = _inputs(0)[0]
    assert {(int(ns[i]), OUTLIERS[i % 3]) for i in range(B) if i not in (TWO, DEGENERATE)} == {(n, o) for n in NS for o in OUTLIERS}
    assert ns[TWO] == 2 and ns[DEGENERATE] == 40 and (np.diff(_inputs(0)[1][DEGENERATE, :40], axis=0) == 0).all()
    assert len(ORACLE_PAIRS) == 8 and not {TWO, DEGENERATE} & set(ORACLE_PAIRS) and all(ns[i] > 3 for i in ORACLE_PAIRS)
    assert {OUTLIERS[i % 3] for i in ORACLE_PAIRS} == set(OUTLIERS)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shift", CASES)
def test_front_stage_on_and_off_give_the_same_bytes_and_follow_the_oracle(monkeypatch, kind, shift):
    from mdrp_amd import _capi
    ns, x1, x2, d1, d2, cams = _inputs(kind)
    h = _capi.Handle(0)
    try:
        on, mask_on, st_on = _run(h, monkeypatch, kind, shift, {"MDRP_FIRST_PICK": "48"})
        off, mask_off, st_off = _run(h, monkeypatch, kind, shift, {"MDRP_FIRST_PICK": "0"})
        small, mask_small, st_small = _run(h, monkeypatch, kind, shift, {"MDRP_FIRST_PICK": "3"})  # the earliest hypothesis is most of P
    finally:
        h.close()
    # the stage ran, beside a second chunk, and left less for the exact sweep; forced off it did not run
    assert st_on["first_chunk"] == st_off["first_chunk"] == 128
    assert st_on["sweep_launches"] == st_off["sweep_launches"] + 1 == st_small["sweep_launches"], (st_on["sweep_launches"], st_off["sweep_launches"])
    assert st_on["evals_fp64"] < st_off["evals_fp64"], (st_on["evals_fp64"], st_off["evals_fp64"])
    for name, (res, mask) in {"on": (on, mask_on), "pick 3": (small, mask_small)}.items():
        assert res.tobytes() == off.tobytes(), (kind, shift, name, [i for i in range(B) if res[i:i + 1].tobytes() != off[i:i + 1].tobytes()][:16])
        assert np.array_equal(mask, mask_off), (kind, shift, name, np.flatnonzero((mask != mask_off).any(axis=1))[:16])
    assert int(on[TWO]["iterations"]) == 0 and int(on[TWO]["num_inliers"]) == 0 and mask_on[TWO].sum() == 0
    assert int(on[DEGENERATE]["iterations"]) == ITS
    assert int(on["num_inliers"].max()) > 300                    # not a comparison of empty results
    oro = po.ransac_opt(max_iterations=ITS, min_iterations=ITS, estimate_shift=shift, **RO)
    obo = po.bundle_opt(loss_type=4)
    cam = po.cam_flat(0, [800.0, 0.0, 0.0]) if kind == 0 else None
    bad = []
    for i in ORACLE_PAIRS:
        n = int(ns[i])
        m, st, mk = po.estimate(kind, x1[i, :n], x2[i, :n], d1[i, :n], d2[i, :n], oro, obo, cam, cam)
        r = on[i]
        same = (int(r["iterations"]), int(r["num_inliers"])) == (st.iterations, st.num_inliers) and np.array_equal(mask_on[i, :n], mk) and mask_on[i, n:].sum() == 0
        d = model_diff(_capi.model_to_array(r["model"]), np.asarray(m, dtype=np.float64)) if same and st.num_inliers > 0 else 0.0
        if not same or not d < MODEL_TOL:
            bad.append(f"pair {i} (N = {n}): iterations {int(r['iterations'])} / {st.iterations}, inliers {int(r['num_inliers'])} / {st.num_inliers}, model {d:.3g}")
    assert not bad, (kind, shift, bad)


@pytest.mark.gpu
def test_front_stage_under_dynamic_stopping(monkeypatch):
    """max 2000 / min 100: 101 iterations certainly run, so the first chunk is the whole certain range (one chunk, nothing beside it) and every
    later super-chunk starts from its records"""
    from mdrp_amd import _capi
    h = _capi.Handle(0)
    try:
        on, mask_on, st_on = _run(h, monkeypatch, 0, False, {"MDRP_FIRST_PICK": "48"}, max_it=2000, min_it=100)
        off, mask_off, st_off = _run(h, monkeypatch, 0, False, {"MDRP_FIRST_PICK": "0"}, max_it=2000, min_it=100)
    finally:
        h.close()
    assert st_on["first_chunk"] == 101 and st_on["sweep_launches"] == st_off["sweep_launches"] + 1
    assert on.tobytes() == off.tobytes(), [i for i in range(B) if on[i:i + 1].tobytes() != off[i:i + 1].tobytes()][:16]
    assert np.array_equal(mask_on, mask_off)
    its = on["iterations"][[i for i in range(B) if i != TWO]]
    assert int(its.min()) >= 101 and int(its.max()) == 2000 and len(set(its.tolist())) > 2  # pairs stop at their own iterations


# ---- the stage behind the other entry points: priors (an ARMED count in the first chunk), PROSAC, budgets, and the longest first chunk
BUDGETS = [10, 50, 128, 200, 600]   # two budgets inside the first chunk of 128 iterations, one on its last iteration, two behind it
LONG = 16384                        # sched::chunk_capacity: with MDRP_CHUNKS set empty the first chunk is the whole first super-chunk
N_LONG = 257


@functools.lru_cache(maxsize=None)
def _priors(kind):
    """by pair index modulo 3: the pair's true model | a hopeless one | NaN (no prior); focals in pixels, 1 for the calibrated kind"""
    from mdrp_amd import _capi, synth
    import from_models_cases as fmc
    ns = _inputs(kind)[0]
    rng = np.random.default_rng(77500 + kind)
    rows = np.zeros((B, 12))
    for i in range(B):
        p = synth.make_pair(77000 + 1000 * kind + i, max(int(ns[i]), 3), noise_px=0.5, depth_noise=0.02, outlier_frac=OUTLIERS[i % 3], random_focal=RF.get(kind))
        f = (1.0, 1.0) if kind == 0 else (p["f1"], p["f2"])
        R, t, scale = (p["R"], p["t"], p["scale"]) if i % 3 != 1 else (synth.rodrigues(rng.normal(0.0, 1.5, 3)), rng.normal(0.0, 0.5, 3), 1.0)
        rows[i] = np.r_[fmc.rotmat_to_quat(R), t, scale, 0.0, 0.0, f]
        if i % 3 == 2:
            rows[i, :4] = np.nan
    return _capi.array_to_models(rows)


@functools.lru_cache(maxsize=None)
def _scores(kind):
    """match scores a matcher might give: inliers mostly above outliers, rounded so that they tie"""
    from mdrp_amd import synth
    ns = _inputs(kind)[0]
    out = np.zeros((B, NMAX))
    rng = np.random.default_rng(77600 + kind)
    for i in range(B):
        n = int(ns[i])
        p = synth.make_pair(77000 + 1000 * kind + i, max(n, 3), noise_px=0.5, depth_noise=0.02, outlier_frac=OUTLIERS[i % 3], random_focal=RF.get(kind))
        out[i, :n] = -(p["is_outlier"][:n] + rng.normal(0.0, 0.6, n)).round(1)
    return out


def _call(h, monkeypatch, kind, env, how, max_it=ITS, min_it=ITS, n_cap=NMAX):
    """one estimate of the 130 pairs through the entry point `how`: (records, masks, statistics); n_cap: correspondences per pair at most"""
    from mdrp_amd import _capi
    ns, x1, x2, d1, d2, cams = _inputs(kind)
    ns = np.minimum(ns, n_cap).astype(np.int32)
    x1, x2, d1, d2 = (np.ascontiguousarray(a[:, :n_cap]) for a in (x1, x2, d1, d2))
    c = cams if kind == 0 else None
    ro = _capi.ransac_opt_from_dict(dict(RO, max_iterations=max_it, min_iterations=min_it))
    bo = _capi.bundle_opt_from_dict(BO)
    _env(monkeypatch, env)
    if how == "plain":
        res, mask = h.estimate_batch(kind, x1, x2, d1, d2, ro, bo, ns, c, c)
    elif how == "priors" or how == "no priors":
        pr = _priors(kind).copy()
        if how == "no priors":
            pr["q"][:] = np.nan
        res, mask = h.estimate_batch_prior(kind, x1, x2, d1, d2, pr, ro, bo, ns, c, c)
    elif how == "scores":
        res, mask = h.estimate_batch_ranked(kind, x1, x2, d1, d2, np.ascontiguousarray(_scores(kind)[:, :n_cap]), ro, bo, ns, c, c)
    else:
        assert how == "budgets"
        res, mask = h.estimate_batch_budgets(kind, x1, x2, d1, d2, ro, bo, BUDGETS, ns, c, c)
    return res.copy(), mask.copy(), h.last_stats()


def _on_off(monkeypatch, kind, how, **kw):
    from mdrp_amd import _capi
    h = _capi.Handle(0)
    try:
        on = _call(h, monkeypatch, kind, {"MDRP_FIRST_PICK": "48"}, how, **kw)
        off = _call(h, monkeypatch, kind, {"MDRP_FIRST_PICK": "0"}, how, **kw)
    finally:
        h.close()
    assert on[2]["sweep_launches"] == off[2]["sweep_launches"] + 1, (how, on[2]["sweep_launches"], off[2]["sweep_launches"])  # the stage ran
    assert on[2]["first_chunk"] == off[2]["first_chunk"]
    flat_on, flat_off = on[0].reshape(-1), off[0].reshape(-1)
    assert on[0].tobytes() == off[0].tobytes(), (kind, how, [i for i in range(len(flat_on)) if flat_on[i:i + 1].tobytes() != flat_off[i:i + 1].tobytes()][:16])
    assert np.array_equal(on[1], off[1]), (kind, how)
    assert int(on[0]["num_inliers"].max()) > 100
    return on, off


def test_the_inputs_of_the_other_entry_points():
    """(no GPU) a third of the pairs each with a true, a hopeless and no prior, at every n; scores that tie and tell inliers from outliers"""
    ns = _inputs(0)[0]
    pr = _priors(0)
    nan = np.isnan(pr["q"][:, 0])
    assert [int(nan[i::3].sum()) for i in range(3)] == [0, 0, len(range(2, B, 3))] and np.isfinite(pr["t"]).all()
    assert {int(ns[i]) for i in range(0, B, 3)} >= {40, 257, 600} and {int(ns[i]) for i in range(1, B, 3)} >= {40, 257, 600}
    sc = _scores(0)
    assert len(np.unique(sc[1, :257])) < 100 and BUDGETS[-1] == ITS and sorted(BUDGETS) == BUDGETS and sum(b < 128 for b in BUDGETS) == 2 and 128 in BUDGETS


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_front_stage_behind_priors(monkeypatch, kind):
    """a good prior arms the first chunk's count: the stage runs on what the prior's records left.  A NaN prior is no prior."""
    on, off = _on_off(monkeypatch, kind, "priors")
    assert on[2]["first_chunk"] == 128
    bare, _ = _on_off(monkeypatch, kind, "no priors")
    assert on[2]["evals_fp64"] < bare[2]["evals_fp64"], ("the good priors retired nothing in the first chunk", on[2]["evals_fp64"], bare[2]["evals_fp64"])
    nan = np.flatnonzero(np.isnan(_priors(kind)["q"][:, 0]))
    from mdrp_amd import _capi
    h = _capi.Handle(0)
    try:
        plain = _call(h, monkeypatch, kind, {"MDRP_FIRST_PICK": "48"}, "plain")
    finally:
        h.close()
    assert bare[0].tobytes() == plain[0].tobytes() and on[0][nan].tobytes() == plain[0][nan].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 2])
def test_front_stage_behind_prosac(monkeypatch, kind):
    """a first chunk full of near-best hypotheses: the progressive sampler draws from the best-scored matches first"""
    on, _ = _on_off(monkeypatch, kind, "scores")
    assert on[2]["first_chunk"] == 128
    ns = _inputs(kind)[0]
    half = [i for i in range(B) if i % 3 == 1 and ns[i] >= 40 and i not in (TWO, DEGENERATE)]  # the pairs at 50 % outliers with more than one sample
    assert len(half) > 20 and (on[0]["num_inliers"][half] > 0).all()


@pytest.mark.gpu
def test_front_stage_with_budgets_inside_the_first_chunk(monkeypatch):
    from mdrp_amd import _capi
    on, _ = _on_off(monkeypatch, 0, "budgets")
    assert on[2]["first_chunk"] == 128 and on[0].shape == (len(BUDGETS), B)
    h = _capi.Handle(0)
    try:
        for c, k in enumerate(BUDGETS):  # each budget's record is the separate call's with max_iterations = the budget (tests/test_gpu_budgets.py)
            res, mask, st = _call(h, monkeypatch, 0, {"MDRP_FIRST_PICK": "48"}, "plain", max_it=k)
            assert on[0][c].tobytes() == res.tobytes(), (k, [i for i in range(B) if on[0][c][i:i + 1].tobytes() != res[i:i + 1].tobytes()][:16])
            assert np.array_equal(on[1][c], mask), k
    finally:
        h.close()


@pytest.mark.gpu
def test_front_stage_on_the_longest_first_chunk(monkeypatch):
    """MDRP_CHUNKS set empty and 16384 certain iterations: the first chunk is its whole super-chunk, 65536 slots per pair (n <= 257: a short call)"""
    from mdrp_amd import _capi
    h = _capi.Handle(0)
    try:
        on = _call(h, monkeypatch, 0, {"MDRP_FIRST_PICK": "48", "MDRP_CHUNKS": ""}, "plain", max_it=LONG, min_it=LONG, n_cap=N_LONG)
        off = _call(h, monkeypatch, 0, {"MDRP_FIRST_PICK": "0", "MDRP_CHUNKS": ""}, "plain", max_it=LONG, min_it=LONG, n_cap=N_LONG)
    finally:
        h.close()
    assert on[2]["first_chunk"] == off[2]["first_chunk"] == LONG and on[2]["sweep_launches"] == off[2]["sweep_launches"] + 1
    assert on[2]["evals_fp64"] < off[2]["evals_fp64"], (on[2]["evals_fp64"], off[2]["evals_fp64"])
    assert on[0].tobytes() == off[0].tobytes(), [i for i in range(B) if on[0][i:i + 1].tobytes() != off[0][i:i + 1].tobytes()][:16]
    assert np.array_equal(on[1], off[1]) and int(on[0]["iterations"].max()) == LONG
