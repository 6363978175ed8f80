"""The exact sweep of every chunk after a run's first (k_score_split: a workgroup per 64 hypotheses, each wavefront a quarter of the records, the
owner wavefront adding the slots in record order) against the lane-per-hypothesis k_score it replaces (MDRP_SCORE_SPLIT=0): every record field and
every inlier mask bit-identical, for the headline fixture batch and for every estimator on ragged batches just above SCORE_WAVE_MAX_PAIRS (the
smallest calls that take the split sweep) with pairs below 64 records, NaN records and all-outlier pairs, a short run and a call of two passes."""
import numpy as np
import pytest

from test_gpu_headline import WORKLOADS, DeviceBatch, _digest

pytestmark = pytest.mark.gpu

SCORE_WAVE_MAX_PAIRS = 128    # mdrp_kernels.h: calls of at most this many pairs score with k_score_w and never reach k_score_split
NMAX = 700
RF = {1: "shared", 2: "varying", 4: "shared"}  # synth.make_pair random_focal per estimator
RO = {"max_epipolar_error": 2.0, "max_reproj_error": 16.0}
BO = {"loss_type": "TRUNCATED_CAUCHY"}
KNOBS = ("MDRP_CHUNKS", "MDRP_LO_OVERLAP", "MDRP_BOUND", "MDRP_FUSE_TAIL", "MDRP_LO_THREADS", "MDRP_FINAL_THREADS", "MDRP_PAIRS_PER_PASS",
         "MDRP_SCORE_SPLIT")
# (pairs, max_iterations = min_iterations, environment): each has two chunks, so the second chunk's sweep is the split one
SHAPES = {
    "b136_i1500": (136, 1500, {}),
    "b129_i300": (129, 300, {}),                                          # one pair above the small-call path; a short run (128 | 172)
    "b272_i1000_pass136": (272, 1000, {"MDRP_PAIRS_PER_PASS": "136"}),    # two passes of 136 pairs
}
SIXPT_SHAPES = ("b129_i300",)  # the 6-point solver only where the runs are short
CASES = [(k, s) for k in range(6) for s in SHAPES if k != 4 or s in SIXPT_SHAPES]


def _set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _differs(a, b):
    """names of the record fields that are not bit-identical"""
    return [f for f in a.dtype.names if a[f].tobytes() != b[f].tobytes()]


def _batch(kind, B):
    """B ragged pairs, zero-padded to NMAX: N from 33 to NMAX (mostly not a multiple of 32), 20-50 % outliers; pair 3 has 37 records, pair 5 a run of NaN
    records, pairs 7 and 8 are all outliers (uniform random correspondences: no hypothesis has a candidate to speak of)"""
    from mdrp_amd import _capi, synth
    rng = np.random.default_rng(7700 + kind)
    ns = rng.integers(33, NMAX + 1, size=B).astype(np.int32)
    ns[3], ns[4] = 37, NMAX
    focal = rng.uniform(600.0, 1000.0, B)
    x1, x2 = np.zeros((B, NMAX, 2)), np.zeros((B, NMAX, 2))
    d1, d2 = np.ones((B, NMAX)), np.ones((B, NMAX))
    for i in range(B):
        n = int(ns[i])
        if i in (7, 8):
            x1[i, :n] = rng.uniform(-800.0, 800.0, (n, 2))
            x2[i, :n] = rng.uniform(-800.0, 800.0, (n, 2))
            d1[i, :n], d2[i, :n] = rng.uniform(1.0, 5.0, n), rng.uniform(1.0, 5.0, n)
            continue
        p = synth.make_pair(77000 + 1000 * kind + i, n, f1=focal[i], f2=focal[i], noise_px=0.5, depth_noise=0.02,
                            outlier_frac=(0.2, 0.35, 0.5)[i % 3], random_focal=RF.get(kind))
        x1[i, :n], x2[i, :n], d1[i, :n], d2[i, :n] = p["x1"], p["x2"], p["d1"], p["d2"]
    x1[5, 40:47] = np.nan
    x2[5, 90:93, 1] = np.nan
    cams = np.zeros(B, dtype=_capi.CAMERA_DTYPE)
    if kind in (0, 3):
        cams["params"][:, 0] = focal
    c1, c2 = (cams, cams) if kind in (0, 3, 4) else (None, None)
    return ns, x1, x2, d1, d2, c1, c2


@pytest.mark.parametrize("kind,shape", CASES)
def test_split_sweep_equals_lane_per_hypothesis_sweep(monkeypatch, kind, shape):
    from mdrp_amd import _capi
    B, its, env = SHAPES[shape]
    assert B > SCORE_WAVE_MAX_PAIRS
    ns, x1, x2, d1, d2, c1, c2 = _batch(kind, B)
    mono = kind <= 2
    ro = _capi.ransac_opt_from_dict(dict(RO, max_iterations=its, min_iterations=its))
    bo = _capi.bundle_opt_from_dict(BO)
    out = {}
    for split in ("0", "1"):
        _set_env(monkeypatch, dict(env, MDRP_SCORE_SPLIT=split))
        h = _capi.Handle(0)
        try:
            r, m = h.estimate_batch(kind, x1, x2, d1 if mono else None, d2 if mono else None, ro, bo, ns, c1, c2)
            first = int(h.last_stats()["first_chunk"])
        finally:
            h.close()
        assert 2 * first <= its, first                                    # a second chunk: its sweep is the one that differs
        out[split] = (r.copy(), m.copy())
    (r0, m0), (r1, m1) = out["0"], out["1"]
    bad = [i for i in range(B) if _differs(r0[i:i + 1], r1[i:i + 1])]
    assert not bad, (kind, shape, bad[:16], [_differs(r0[i:i + 1], r1[i:i + 1]) for i in bad[:4]])
    assert np.array_equal(m0, m1), (kind, shape, np.flatnonzero((m0 != m1).any(axis=1))[:16])
    assert int(r1["num_inliers"].max()) > 100                             # not a comparison of empty results
    assert int(r1["iterations"].max()) == its
    assert int(r1[7]["num_inliers"]) < 40 and int(r1[8]["num_inliers"]) < 40


def test_split_sweep_equals_lane_per_hypothesis_sweep_on_the_headline_batch(monkeypatch, golden):
    """the 1024 pairs bench.py times (tests/golden/headline_calib_p3p_n2000_i10k: the same generator), both sweeps, records and masks bit for bit"""
    from mdrp_amd import _capi
    g = golden("headline_calib_p3p_n2000_i10k")
    out = {}
    for split in ("0", "1"):
        _set_env(monkeypatch, {"MDRP_SCORE_SPLIT": split})
        db = DeviceBatch(_capi, "calib_p3p_n2000_i10k")
        try:
            if split == "0":
                for i in range(0, db.B, 97):
                    assert _digest(db.host, i) == g["digest"][i], "synthetic generator drifted"
            res = db.run()
            out[split] = (res.copy(), db.mask.cpu().numpy())
        finally:
            db.close()
    (r0, m0), (r1, m1) = out["0"], out["1"]
    bad = [i for i in range(len(r0)) if _differs(r0[i:i + 1], r1[i:i + 1])]
    assert not bad, (bad[:16], [_differs(r0[i:i + 1], r1[i:i + 1]) for i in bad[:4]])
    assert np.array_equal(m0, m1), np.flatnonzero((m0 != m1).any(axis=1))[:16]
    assert np.array_equal(r1["num_inliers"].astype(np.int64), g["istats"][:, 2])
    assert WORKLOADS["calib_p3p_n2000_i10k"][0] == 0
