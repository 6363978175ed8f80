"""Cases of the varying-focal baseline's tail for tests/test_classic_focals_host.py (CPU) and tests/test_gpu_classic_focals.py: the fixture of the
reference binary's focals, and batches of synthetic pairs for the pose vote with their yardstick records (tests/classic_focals_ref.py), computed once.

A vote batch: pairs of N records at the wavefront and 256-lane boundaries, n_max > n with the rows past n filled with NaN, a principal point per pair
and image (one pair: the origin), 30 % of the records replaced by random pixels, a mask per pair (one pair: all zero), and the special pairs — a NaN
F, a pair of fewer than seven records, a matrix of the fixture whose f^2 is negative.  Every batch is run with its mask and without one.
"""
import functools
import os

import numpy as np

import classic_focals_ref as fr
from mdrp_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "classic_focals_ref.npz")
SIZES = ((7, 8, 63, 64, 65, 255), (256, 257, 300, 600))
SEEDS = (4101, 4202)  # chosen on the CPU: the smallest |depth| of every case exceeds classic_focals_ref.MARGIN (asserted by the tests, for every case)


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(FIXTURE)
    return {k: z[k] for k in z.files}


def _skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def scene(rng, n, pp_zero=False, outliers=0.3):
    """a noise-free pair: (x1, x2 [n][2] pixels, F [9] with unit norm, pp1, pp2, truth dict, inlier flags [n])"""
    f1, f2 = rng.uniform(400.0, 1500.0, 2)
    rv = rng.normal(0.0, 0.2, 3)
    th = np.linalg.norm(rv)
    K = _skew(rv / th)
    R = np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * K @ K
    t = rng.normal(0.0, 1.0, 3)
    t /= np.linalg.norm(t)
    X = np.c_[rng.uniform(-2.0, 2.0, (n, 2)), rng.uniform(4.0, 8.0, n)]
    Y = X @ R.T + t
    pp1, pp2 = (np.zeros(2), np.zeros(2)) if pp_zero else (rng.normal(0.0, 30.0, 2), rng.normal(0.0, 30.0, 2))
    x1 = f1 * X[:, :2] / X[:, 2:] + pp1
    x2 = f2 * Y[:, :2] / Y[:, 2:] + pp2
    K1i = np.array([[1 / f1, 0.0, -pp1[0] / f1], [0.0, 1 / f1, -pp1[1] / f1], [0.0, 0.0, 1.0]])
    K2i = np.array([[1 / f2, 0.0, -pp2[0] / f2], [0.0, 1 / f2, -pp2[1] / f2], [0.0, 0.0, 1.0]])
    F = K2i.T @ _skew(t) @ R @ K1i
    good = np.ones(n, bool)
    if outliers > 0 and n > 8:
        bad = rng.random(n) < outliers
        x1[bad] = rng.uniform(-800.0, 800.0, (int(bad.sum()), 2))
        x2[bad] = rng.uniform(-800.0, 800.0, (int(bad.sum()), 2))
        good = ~bad
    return x1, x2, (F / np.linalg.norm(F)).reshape(-1), pp1, pp2, dict(R=R, t=t, f1=f1, f2=f2), good


def _negative_focal_matrix():
    fx = fixture()
    i = int(np.flatnonzero(np.isnan(fx["f"]).any(axis=1))[0])
    return fx["F"][i], fx["pp1"][i], fx["pp2"][i]


@functools.lru_cache(maxsize=None)
def batch(which):
    """dict: x1, x2 (B, n_max, 2), n (B,), models (B,) MODEL_DTYPE, mask (B, n_max) uint8, pp1, pp2 (B, 2), names"""
    rng = np.random.default_rng(SEEDS[which])
    sizes = list(SIZES[which])
    names = [f"n{n}" for n in sizes]
    rows = [scene(rng, n, pp_zero=(which == 1 and n == 257)) for n in sizes]
    masks = [(g & (rng.random(len(g)) < 0.9)) | (rng.random(len(g)) < 0.05) for *_, g in rows]  # the inliers, less a few, plus a few outliers
    if which == 0:
        x1, x2, F, a, b, _, g = scene(rng, 40)
        rows.append((x1, x2, np.full(9, np.nan), a, b, None, g)); masks.append(g.copy()); names.append("nan_F")
        x1, x2, F, a, b, _, g = scene(rng, 90)
        rows.append((x1, x2, F, a, b, None, g)); masks.append(np.zeros(90, bool)); names.append("zero_mask")
    else:
        x1, x2, F, a, b, _, g = scene(rng, 5)
        rows.append((x1, x2, F, a, b, None, g)); masks.append(g.copy()); names.append("n5")
        x1, x2, _, _, _, _, g = scene(rng, 70)
        F, a, b = _negative_focal_matrix()
        rows.append((x1, x2, F, a, b, None, g)); masks.append(g.copy()); names.append("negative_f")
    B = len(rows)
    n = np.array([len(r[0]) for r in rows], dtype=np.int32)
    n_max = int(n.max()) + 5
    x1 = np.full((B, n_max, 2), np.nan); x2 = np.full((B, n_max, 2), np.nan)
    mask = np.ones((B, n_max), dtype=np.uint8)  # (set past n as well: a byte there must not make its NaN row vote)
    models = np.zeros(B, dtype=_capi.MODEL_DTYPE)
    pp1, pp2 = np.zeros((B, 2)), np.zeros((B, 2))
    for i, (a1, a2, F, a, b, _, _) in enumerate(rows):
        x1[i, :n[i]], x2[i, :n[i]] = a1, a2
        mask[i, :n[i]] = masks[i]
        models[i] = _capi.fundamental_to_model(F)
        pp1[i], pp2[i] = a, b
    return dict(x1=x1, x2=x2, n=n, models=models, mask=mask, pp1=pp1, pp2=pp2, names=names)


@functools.lru_cache(maxsize=None)
def expected(which, with_mask):
    """the yardstick's records of a batch, computed once"""
    c = batch(which)
    return [fr.focal_pose(_capi.model_to_fundamental(c["models"][i]).reshape(-1), c["x1"][i], c["x2"][i], int(c["n"][i]),
                          c["mask"][i] if with_mask else None, c["pp1"][i], c["pp2"][i]) for i in range(len(c["n"]))]


def as_results(models):
    """the same matrices inside result records (stride 136), the other fields filled with values a reader of the wrong stride would trip over"""
    res = np.zeros(len(models), dtype=_capi.RESULT_DTYPE)
    res["model"] = models
    res["refinements"] = 3; res["iterations"] = 1000; res["num_inliers"] = 77; res["inlier_ratio"] = np.nan; res["model_score"] = -1.0
    return res


def check_record(got, want, where):
    """a FOCAL_POSE_DTYPE record against the yardstick's: integers equal, q up to sign and t to 1e-12, the focals' NaNs in place"""
    assert [int(v) for v in got["votes"]] == [int(v) for v in want["votes"]], where
    assert (int(got["voters"]), int(got["winner"]), int(got["status"]), int(got["pad_"])) == (want["voters"], want["winner"], want["status"], 0), where
    m = got["model"]
    q, t = np.asarray(m["q"]), np.asarray(m["t"])
    wq, wt = want["model"][:4], want["model"][4:7]
    assert min(np.abs(q - wq).max(), np.abs(q + wq).max()) <= 1e-12 and np.abs(t - wt).max() <= 1e-12, where
    assert (float(m["scale"]), float(m["shift1"]), float(m["shift2"])) == (1.0, 0.0, 0.0), where
    tol = float(fixture()["tolerance"])
    for f, wf in ((float(m["f1"]), want["model"][10]), (float(m["f2"]), want["model"][11])):
        assert np.isnan(f) == np.isnan(wf) and (np.isnan(f) or abs(f - wf) <= tol * abs(wf)), where
    if want["status"] == 0:
        assert abs(np.linalg.norm(t) - 1.0) <= 1e-12, where


def assert_margins(which, with_mask):
    """the condition every vote case must meet, asserted by the tests for every case: no cheirality test of the case comes closer to zero than
    MARGIN, so that the vote counts do not depend on the last bits of the arithmetic"""
    swept = 0
    for name, rec in zip(batch(which)["names"], expected(which, with_mask)):
        assert rec["margin"] > fr.MARGIN, (which, with_mask, name, rec["margin"])
        swept += rec["status"] == 0
    assert swept >= len(SIZES[which])
