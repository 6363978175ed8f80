"""The history rule of include/mdrp.h for the entry points of include/mdrp_dense.h: each of them, called behind and in front of a larger dense call, a
sparse front-end call and a plain estimate on ONE handle, returns the bytes it returns on a fresh handle - and so do the calls around it.  The dense
calls share the sparse front end's gather buffers (fe_x1 .. fe_n) and have a scratch buffer of their own that is carved per call: a larger call in
front leaves it larger and differently carved.  Every comparison is of bytes; the fresh answers are computed once."""
import numpy as np
import pytest

import dense_cases as dc

pytestmark = pytest.mark.gpu

F32 = np.float32


def _small():
    return dc.tensors(*dc.as_seen(dc.batch("small")))


def _scene():
    b = dc.estimate_batch()
    return dc.tensors(b["warp"].astype(F32), b["cert"].astype(F32), b["dm1"].astype(F32), b["dm2"].astype(F32))


def sample_small(h, capi):
    return dc.sample_on(h, _small(), 100)


def sample_ranked(h, capi):
    return dc.sample_on(h, _small(), 64, ranked=True, grid=3, min_count=1)


def sample_larger(h, capi):  # more rows, more records, a larger stage 1: every part of the scratch grows and moves
    return dc.sample_on(h, dc.tensors(*dc.as_seen(dc.batch("blocks"))), 1100, expansion=2)


def estimate_dense(h, capi):
    return dc.estimate_on(h, capi.CALIB, _scene(), 300, (dc.ECAM1, dc.ECAM2), coords="pixel")


def estimate_dense_ranked(h, capi):
    return dc.estimate_on(h, capi.VARYING_FOCAL, _scene(), 200, coords="pixel", ranked=True, center1=dc.EC1, center2=dc.EC2)


def sparse_front_end(h, capi):
    """mdrp_estimate_matches_async on the scene's rows as keypoint tables and index pairs"""
    import torch
    from mdrp_amd import poselib
    b = dc.estimate_batch()
    B, R = b["cert"].shape
    matches = np.tile(np.stack([np.arange(R), np.arange(R)], 1)[None], (B, 1, 1)).astype(np.int32)
    t = dc.tensors(b["warp"][..., :2].astype(F32), b["warp"][..., 2:].astype(F32), matches, b["dm1"].astype(F32), b["dm2"].astype(F32))
    mm, keep, B, M, _ = poselib._matches_descriptor(*t, None, None, "both_inf")
    mask = torch.zeros((B, M), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    cams = poselib._camera_records(dc.ECAM1, B), poselib._camera_records(dc.ECAM2, B)
    n = h.estimate_matches_device(capi.CALIB, mm, B, capi.ransac_opt_from_dict(dc.ERO), capi.bundle_opt_from_dict(dc.EBO), *cams, mask.data_ptr())
    res = h.fetch_results(B)
    return (res.tobytes(), mask.cpu().numpy().tobytes(), n.tobytes())


def plain_estimate(h, capi):
    from mdrp_amd import synth
    b = synth.make_batch(5300, 4, 150, noise_px=0.5, outlier_frac=0.3)
    res, mask = h.estimate_batch(capi.SHARED_FOCAL, b["x1"], b["x2"], b["d1"], b["d2"], capi.ransac_opt_from_dict(dict(dc.ERO, max_epipolar_error=2.0, max_reproj_error=16.0)),
                                 capi.bundle_opt_from_dict(dc.EBO))
    return (res.tobytes(), mask.tobytes())


NEW = {"sample_small": sample_small, "sample_ranked": sample_ranked, "sample_larger": sample_larger, "estimate_dense": estimate_dense,
       "estimate_dense_ranked": estimate_dense_ranked}
OLD = {"sparse_front_end": sparse_front_end, "plain_estimate": plain_estimate}
ALL = {**NEW, **OLD}


@pytest.fixture(scope="module")
def capi():
    from mdrp_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def fresh(capi):
    """{name: byte strings} of every call on a handle of its own: computed once, never changed"""
    out = {}
    for name, call in ALL.items():
        h = capi.Handle(0)
        try:
            out[name] = call(h, capi)
        finally:
            h.close()
    return out


def test_fresh_results_are_reproducible_and_not_empty(capi, fresh):
    for name, call in NEW.items():
        h = capi.Handle(0)
        try:
            assert call(h, capi) == fresh[name], name
        finally:
            h.close()
    assert fresh["sample_small"][4] == dc.reference("small", 100, centres=False)[5].tobytes()
    for name in ("estimate_dense", "estimate_dense_ranked"):
        res = np.frombuffer(fresh[name][0], dtype=capi.RESULT_DTYPE)
        cnt = np.frombuffer(fresh[name][3], dtype=np.int32)
        assert (cnt > 100).all() and (res["num_inliers"] > 0.8 * cnt).all(), name


@pytest.mark.parametrize("new", sorted(NEW))
def test_a_dense_call_behind_and_in_front_of_every_other_call(capi, fresh, new):
    for other in sorted(ALL):
        for first, second in ((other, new), (new, other)):
            h = capi.Handle(0)
            try:
                got_first = ALL[first](h, capi)
                got_second = ALL[second](h, capi)
            finally:
                h.close()
            assert got_first == fresh[first], (first, "in front of", second)
            assert got_second == fresh[second], (second, "behind", first)
