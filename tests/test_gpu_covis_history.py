"""The history rule of include/mdrp.h for the entry points of include/mdrp_covis.h: each of them, called behind and in front of a larger call of its
own kind, a refused call, a two-view cloud, a scene, a dense sample and a plain estimate on ONE handle, returns the bytes it returns on a fresh
handle - and so do the calls around it.  Co-visibility carves the back end's one scratch buffer per call (the pairs' records, the camera tables),
as the two-view clouds and the scenes do, and it ADDS to the caller's counters: a call that did not clear them, or read a record of the call
before it, would show here.  Every comparison is of bytes; the fresh answers are computed once."""
import pytest

import covis_cases as cc
import dense_cases as dc
import reconstruct_cases as rc
import scene_cases as sc

pytestmark = pytest.mark.gpu


def pairs_small(h, capi):
    return cc.device_call(h)


def pairs_calibrated(h, capi):
    return cc.device_call(h, kind="calibrated", dtype_name="float64", B=5, rate=1.0, tol=0.0, stride=136)


def image_pairs(h, capi):
    return cc.device_call(h, image_form=True)


def pairs_larger(h, capi):  # more pairs, more tiles: the scratch grows and moves
    return cc.device_call(h, size=cc.SIZES[3], B=17, rate=0.5)


def refused(h, capi):
    with pytest.raises(capi.MdrpError) as e:
        cc.device_call(h, change=lambda a: setattr(a["opt"], "hi", 0.5))
    return (str(e.value).encode(),)


def two_view_cloud(h, capi):
    return rc.device_call(h)


def scene(h, capi):  # the scene's smallest good call: its records, images and tile counts lie where the pairs' records lay
    return sc.device_call(h)


def dense_sample(h, capi):
    return dc.sample_on(h, dc.tensors(*dc.as_seen(dc.batch("small"))), 100)


def larger_estimate(h, capi):
    from mdrp_amd import synth
    b = synth.make_batch(5300, 6, 300, noise_px=0.5, outlier_frac=0.3)
    ro = capi.ransac_opt_from_dict({"max_iterations": 200, "min_iterations": 200, "max_epipolar_error": 2.0, "max_reproj_error": 16.0})
    res, mask = h.estimate_batch(capi.SHARED_FOCAL, b["x1"], b["x2"], b["d1"], b["d2"], ro, capi.bundle_opt_from_dict({"loss_type": "TRUNCATED_CAUCHY"}))
    return (res.tobytes(), mask.tobytes())


NEW = {"pairs_small": pairs_small, "pairs_calibrated": pairs_calibrated, "image_pairs": image_pairs, "pairs_larger": pairs_larger}
OLD = {"refused": refused, "two_view_cloud": two_view_cloud, "scene": scene, "dense_sample": dense_sample, "larger_estimate": larger_estimate}
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


def test_fresh_results_are_the_definitions(capi, fresh):
    import numpy as np
    assert fresh["pairs_small"] == (cc.reference("varying_focal", "float32", cc.SIZES[2], 0.5, 0.05, 3).tobytes(),)
    assert fresh["pairs_calibrated"] == (cc.reference("calibrated", "float64", cc.SIZES[2], 1.0, 0.0, 5).tobytes(),)
    assert fresh["pairs_larger"] == (cc.reference("varying_focal", "float32", cc.SIZES[3], 0.5, 0.05, 17).tobytes(),)
    counts = np.frombuffer(fresh["pairs_larger"][0], dtype=np.int32).reshape(17, 2, 8)
    assert (counts[[0, 3, 8], :, 3] > 1000).all() and not counts[1].any()
    assert fresh["image_pairs"] != fresh["pairs_small"]
    assert fresh["two_view_cloud"] == tuple(w.tobytes() for w in rc.reference("varying_focal", "float32", rc.SIZES[2], "not_inf", 0.5, 3, 700))


@pytest.mark.parametrize("new", sorted(NEW))
def test_a_covisibility_call_behind_and_in_front_of_every_other_call(capi, fresh, new):
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
