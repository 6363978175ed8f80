"""The varying-focal baseline's tail on a real MI355X (include/mdrp_classic_focals.h): kc_focals against the reference binary's focals
(tests/golden/classic_focals_ref.npz), kc_focal_pose against the yardstick (tests/classic_focals_ref.py) in its host, device and resident forms and
at both record strides, the fused call against the 7-point estimate followed by the tail, the Python entry point on noise-free pairs against the
ground truth, and the refusals at the boundary of the C ABI.  Inputs and the yardstick's answers: tests/classic_focals_cases.py."""
import ctypes as C

import numpy as np
import pytest

import classic_focals_cases as fc
from test_classic_focals_host import check_focals

pytestmark = pytest.mark.gpu

ERR_INVALID = 1


@pytest.fixture(scope="module")
def capi():
    from mdrp_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def handle(capi):
    return capi.default_handle(0)


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()  # (the handle below has a stream of its own)
    return t


# ---------------------------------------------------------------------------------------------------------------- mdrp_focals_from_fundamental
def test_focals_against_the_binary(capi, handle):
    """400 matrices of the fixture through kc_focals, from host and from device memory: NaN exactly where the binary has one, the others within the
    fixture's tolerance; a NULL principal point is the origin"""
    import torch
    fx = fc.fixture()
    got = handle.focals_from_fundamental(fx["F"], fx["pp1"], fx["pp2"])
    check_focals(got, fx)
    F, a, b = _dev(fx["F"]), _dev(fx["pp1"]), _dev(fx["pp2"])
    out = torch.full((len(fx["F"]), 2), -7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    handle.focals_from_fundamental_device(F.data_ptr(), a.data_ptr(), b.data_ptr(), len(fx["F"]), out.data_ptr())
    assert out.cpu().numpy().tobytes() == got.tobytes()
    zero = (fx["pp1"] == 0).all(axis=1) & (fx["pp2"] == 0).all(axis=1)
    assert zero.sum() > 50 and handle.focals_from_fundamental(fx["F"][zero]).tobytes() == got[zero].tobytes()
    assert handle.focals_from_fundamental(np.zeros((0, 9))).shape == (0, 2)


# ---------------------------------------------------------------------------------------------------------------- mdrp_pose_from_fundamental
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("with_mask", [True, False])
def test_pose_against_the_yardstick(capi, handle, which, with_mask):
    """every pair of the vote batches (N at the wavefront and 256-lane boundaries, NaN rows past n, a NaN F, n < 7, f^2 < 0, an all-zero mask):
    integers equal, q up to sign and t to 1e-12 — from host memory at both strides, from device memory, and resident through torch"""
    import torch
    from mdrp_amd import poselib
    fc.assert_margins(which, with_mask)  # no case is exempt
    c = fc.batch(which)
    want = fc.expected(which, with_mask)
    B, N = c["x1"].shape[:2]
    assert N > c["n"].max() and np.isnan(c["x1"][np.arange(N)[None, :] >= c["n"][:, None]]).all() and 6 <= B <= 12
    mask = c["mask"] if with_mask else None
    host = handle.pose_from_fundamental(c["x1"], c["x2"], c["models"], c["n"], mask, c["pp1"], c["pp2"])
    for i, name in enumerate(c["names"]):
        print(which, with_mask, name, "votes", host[i]["votes"].tolist(), "voters", int(host[i]["voters"]), "winner", int(host[i]["winner"]),
              "status", int(host[i]["status"]), "margin", want[i]["margin"])
        fc.check_record(host[i], want[i], (which, with_mask, name))
    results = fc.as_results(c["models"])
    wide = handle.pose_from_fundamental(c["x1"], c["x2"], results, c["n"], mask, c["pp1"], c["pp2"])
    assert wide.tobytes() == host.tobytes()  # stride 136: the matrix inside result records
    x1, x2, md, rs, a, b = (_dev(v) for v in (c["x1"], c["x2"], c["models"].view(np.uint8), results.view(np.uint8), c["pp1"], c["pp2"]))
    mk = _dev(c["mask"]) if with_mask else None
    out = np.zeros(B, dtype=capi.FOCAL_POSE_DTYPE)
    handle.pose_from_fundamental_device(x1.data_ptr(), x2.data_ptr(), B, N, md.data_ptr(), 96, None, c["n"], None if mk is None else mk.data_ptr(),
                                        a.data_ptr(), b.data_ptr(), blocking_out=out)
    assert out.tobytes() == host.tobytes()  # the blocking call on device memory
    for models in (md, rs, c["models"], results):
        rec = poselib.pose_from_fundamental_batch_torch(x1, x2, models, c["n"], mk, a, b)
        assert rec.tobytes() == host.tobytes()  # resident, on torch's stream
    # one pair alone gives the record it has in its batch (a pair's record does not depend on its batch); pp as a plain pair of numbers
    i = len(fc.SIZES[which]) - 1
    one = poselib.pose_from_fundamental_batch_torch(x1[i:i + 1], x2[i:i + 1], c["models"][i:i + 1], c["n"][i:i + 1], None if mk is None else mk[i:i + 1],
                                                    c["pp1"][i], c["pp2"][i])
    assert one.tobytes() == host[i:i + 1].tobytes()


def test_pose_without_principal_points_is_the_origin(capi, handle):
    c = fc.batch(1)
    i = c["names"].index("n257")
    assert not c["pp1"][i].any() and not c["pp2"][i].any()
    s = slice(i, i + 1)
    given = handle.pose_from_fundamental(c["x1"][s], c["x2"][s], c["models"][s], c["n"][s], c["mask"][s], c["pp1"][s], c["pp2"][s])
    null = handle.pose_from_fundamental(c["x1"][s], c["x2"][s], c["models"][s], c["n"][s], c["mask"][s], None, None)
    assert null.tobytes() == given.tobytes() and given[0]["status"] == 0


def test_refusals_leave_the_handle_usable(capi, handle):
    """MDRP_ERR_INVALID before any device work: a NULL required buffer, n_per_pair out of range, a bad stride, a negative size, an unknown memory
    space, a NULL out of the fused call — and the same handle then returns what it returned before"""
    lib = handle._lib
    c = fc.batch(0)
    B, N = c["x1"].shape[:2]
    before = handle.pose_from_fundamental(c["x1"], c["x2"], c["models"], c["n"], c["mask"], c["pp1"], c["pp2"])
    x1, x2, n, md, out = (np.ascontiguousarray(v) for v in (c["x1"], c["x2"], c["n"], c["models"], np.zeros(B, dtype=capi.FOCAL_POSE_DTYPE)))
    p = capi._ptr
    f2 = np.zeros((B, 2))
    F = np.ascontiguousarray(np.stack([capi.model_to_fundamental(m).reshape(-1) for m in md]))
    big, neg = n.copy(), n.copy()
    big[2] = N + 1
    neg[3] = -1
    calls = {
        "null models": lambda: lib.mdrp_pose_from_fundamental(handle._h, 0, p(x1), p(x2), B, N, p(n), None, 96, None, None, None, p(out)),
        "null out": lambda: lib.mdrp_pose_from_fundamental(handle._h, 0, p(x1), p(x2), B, N, p(n), p(md), 96, None, None, None, None),
        "null x1": lambda: lib.mdrp_pose_from_fundamental(handle._h, 0, None, p(x2), B, N, p(n), p(md), 96, None, None, None, p(out)),
        "null x2, resident": lambda: lib.mdrp_pose_from_fundamental_async(handle._h, p(x1), None, B, N, p(n), p(md), 96, None, None, None, p(out)),
        "n above n_max": lambda: lib.mdrp_pose_from_fundamental(handle._h, 0, p(x1), p(x2), B, N, p(big), p(md), 96, None, None, None, p(out)),
        "negative n": lambda: lib.mdrp_pose_from_fundamental_async(handle._h, p(x1), p(x2), B, N, p(neg), p(md), 96, None, None, None, p(out)),
        "stride below a model": lambda: lib.mdrp_pose_from_fundamental(handle._h, 0, p(x1), p(x2), B, N, p(n), p(md), 72, None, None, None, p(out)),
        "stride no multiple of 8": lambda: lib.mdrp_pose_from_fundamental(handle._h, 0, p(x1), p(x2), B, N, p(n), p(md), 100, None, None, None, p(out)),
        "negative batch": lambda: lib.mdrp_pose_from_fundamental(handle._h, 0, p(x1), p(x2), -1, N, p(n), p(md), 96, None, None, None, p(out)),
        "memory space": lambda: lib.mdrp_pose_from_fundamental(handle._h, 2, p(x1), p(x2), B, N, p(n), p(md), 96, None, None, None, p(out)),
        "no handle": lambda: lib.mdrp_pose_from_fundamental(None, 0, p(x1), p(x2), B, N, p(n), p(md), 96, None, None, None, p(out)),
        "focals: null F": lambda: lib.mdrp_focals_from_fundamental(handle._h, 0, None, None, None, B, p(f2)),
        "focals: null out": lambda: lib.mdrp_focals_from_fundamental(handle._h, 0, p(F), None, None, B, None),
        "focals: memory space": lambda: lib.mdrp_focals_from_fundamental(handle._h, 3, p(F), None, None, B, p(f2)),
        "fused: null out": lambda: lib.mdrp_estimate_fundamental_focals_async(handle._h, p(x1), p(x2), B, N, p(n), C.byref(capi.ransac_opt_from_dict({})),
                                                                               C.byref(capi.bundle_opt_from_dict({})), None, None, None, None),
        "fused: n above n_max": lambda: lib.mdrp_estimate_fundamental_focals_async(handle._h, p(x1), p(x2), B, N, p(big), C.byref(capi.ransac_opt_from_dict({})),
                                                                                    C.byref(capi.bundle_opt_from_dict({})), None, None, None, p(out)),
        "fused: null options": lambda: lib.mdrp_estimate_fundamental_focals_async(handle._h, p(x1), p(x2), B, N, p(n), None, None, None, None, None, p(out)),
    }
    for name, call in calls.items():  # (every refusal comes before the first use of a pointer: host arrays stand in for device memory)
        assert call() == ERR_INVALID, name
        assert lib.mdrp_last_error(), name
    ro = capi.ransac_opt_from_dict({"real_focal_check": True})
    assert lib.mdrp_estimate_fundamental_focals_async(handle._h, p(x1), p(x2), B, N, p(n), C.byref(ro), C.byref(capi.bundle_opt_from_dict({})), None, None, None,
                                                      p(out)) == capi.ERR_UNSUPPORTED  # the estimator's own refusal keeps its code
    assert not out.view(np.uint8).any()
    after = handle.pose_from_fundamental(c["x1"], c["x2"], c["models"], c["n"], c["mask"], c["pp1"], c["pp2"])
    assert after.tobytes() == before.tobytes()


# ---------------------------------------------------------------------------------------------------------------- the fused call, the Python entry point
def _pairs(seed, sizes, outliers):
    rng = np.random.default_rng(seed)
    rows = [fc.scene(rng, n, pp_zero=(k == 1), outliers=outliers) for k, n in enumerate(sizes)]
    B, N = len(rows), max(sizes) + 3
    x1, x2 = np.zeros((B, N, 2)), np.zeros((B, N, 2))
    for i, r in enumerate(rows):
        x1[i, :len(r[0])], x2[i, :len(r[0])] = r[0], r[1]
    return rows, x1, x2, np.array(sizes, dtype=np.int32), np.stack([r[3] for r in rows]), np.stack([r[4] for r in rows])


OPTIONS = ({"max_iterations": 300, "min_iterations": 300, "max_epipolar_error": 1.0, "seed": 7}, {"loss_type": "TRUNCATED_CAUCHY"})


def test_the_fused_call_is_the_estimate_followed_by_the_tail(capi):
    """mdrp_estimate_fundamental_focals_async against estimate_baseline_batch_torch("fundamental_7pt") and then the tail on its records and mask:
    byte for byte, the 7-point records included; with and without a caller's mask buffer is the same call to the kernel"""
    from mdrp_amd import poselib
    rows, x1, x2, n, pp1, pp2 = _pairs(611, (7, 8, 63, 64, 65, 255, 256, 257, 300, 600, 5), 0.3)
    t1, t2 = _dev(x1), _dev(x2)
    ro, bo = OPTIONS
    rec, res, mask = poselib.estimate_varying_focal_baseline_batch_torch(t1, t2, pp1, pp2, ro, bo, n_per_pair=n)
    res2, mask2 = poselib.estimate_baseline_batch_torch("fundamental_7pt", t1, t2, ransac_opt=ro, bundle_opt=bo, n_per_pair=n)
    assert res.tobytes() == res2.tobytes() and mask.cpu().numpy().tobytes() == mask2.cpu().numpy().tobytes()  # today's 7-point records
    rec2 = poselib.pose_from_fundamental_batch_torch(t1, t2, res2, n, mask2, pp1, pp2)
    assert rec.tobytes() == rec2.tobytes()
    assert (rec["status"][:-1] == 0).all() and rec["status"][-1] == capi.FOCAL_NO_MODEL and (rec["voters"][:-1] == res["num_inliers"][:-1]).all()
    assert (rec["voters"][2:-1] < n[2:-1]).all()  # the outliers did not vote: the mask was read
    # behind a 7-point call with a prior: the tail composes with any of them
    res3, mask3 = poselib.estimate_baseline_batch_torch("fundamental_7pt", t1, t2, ransac_opt=ro, bundle_opt=bo, n_per_pair=n, priors=res2["model"].copy())
    rec3 = poselib.pose_from_fundamental_batch_torch(t1, t2, res3, n, mask3, pp1, pp2)
    assert (rec3["status"][:-1] == 0).all()
    for i in range(2, len(n) - 1):  # (another run's F may come with the other sign and its candidates in another order: the winning pose is the same)
        qa, qb = rec3["model"]["q"][i], rec["model"]["q"][i]
        assert min(np.abs(qa - qb).max(), np.abs(qa + qb).max()) < 1e-6 and np.abs(rec3["model"]["t"][i] - rec["model"]["t"][i]).max() < 1e-6, i


def test_noise_free_pairs_recover_the_ground_truth(capi):
    """estimate_varying_focal_relative_pose_batch: f1, f2 to 1e-6 relative, the rotation to 1e-6, and t with its sign"""
    from mdrp_amd import poselib
    sizes = (64, 100, 257, 300, 600, 40)
    rows, x1, x2, n, pp1, pp2 = _pairs(733, sizes, 0.25)
    ro, bo = OPTIONS
    pairs, infos = poselib.estimate_varying_focal_relative_pose_batch([r[0] for r in rows], [r[1] for r in rows], pp1, pp2, ro, bo)
    for i, (r, pair, info) in enumerate(zip(rows, pairs, infos)):
        truth, good = r[5], r[6]
        f1, f2 = pair.camera1.focal(), pair.camera2.focal()
        print(i, "f1", f1, truth["f1"], "f2", f2, truth["f2"], "R", np.abs(pair.pose.R - truth["R"]).max(), "t", np.abs(pair.pose.t - truth["t"]).max(),
              "votes", info["votes"], "inliers", info["num_inliers"], int(good.sum()))
        assert info["status"] == 0 and info["votes"][info["winner"]] == info["num_inliers"] == int(good.sum()) and info["F"].shape == (3, 3)
        assert abs(f1 - truth["f1"]) <= 1e-6 * truth["f1"] and abs(f2 - truth["f2"]) <= 1e-6 * truth["f2"]
        assert np.abs(pair.pose.R - truth["R"]).max() <= 1e-6
        assert np.abs(pair.pose.t - truth["t"]).max() <= 1e-6 and abs(np.linalg.norm(pair.pose.t) - 1.0) <= 1e-12
        assert pair.camera1.params[1:3] == list(pp1[i]) and pair.camera2.params[1:3] == list(pp2[i]) and (pair.camera1.width, pair.camera1.height) == (-1, -1)
    one, info = poselib.estimate_varying_focal_relative_pose(rows[1][0], rows[1][1], pp1[1], pp2[1], ro, bo)
    assert np.array_equal(one.pose.q, pairs[1].pose.q) and one.camera1.focal() == pairs[1].camera1.focal() and info["votes"] == infos[1]["votes"]
    c1, c2 = poselib.focals_from_fundamental(infos[0]["F"], pp1[0], pp2[0])
    assert (c1.focal(), c2.focal()) == (pairs[0].camera1.focal(), pairs[0].camera2.focal()) and c1.model_name() == "SIMPLE_PINHOLE" and c1.width == c1.height == -1
    F, a, b = fc._negative_focal_matrix()
    bad1, bad2 = poselib.focals_from_fundamental(F.reshape(3, 3), a, b)
    assert np.isnan(bad1.focal()) or np.isnan(bad2.focal())
