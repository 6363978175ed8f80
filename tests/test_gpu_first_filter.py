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
