"""The history rule of include/mdrp.h for the entry points of include/mdrp_scene.h: each of them, called behind and in front of a larger scene call, a
two-view reconstruct, a refused call and a plain estimate on ONE handle, returns the bytes it returns on a fresh handle - and so do the calls around
it.  The scene calls have a scratch buffer of their own that is carved per call (the images' records where the caller takes none, their intrinsics,
the camera table, the tile counts): a larger call in front leaves it larger and differently carved.  Every comparison is of bytes; the fresh answers
are computed once."""
import pytest

import reconstruct_cases as rc
import scene_cases as sc

pytestmark = pytest.mark.gpu


def scene_small(h, capi):
    return sc.device_call(h)


def scene_calibrated(h, capi):  # the camera table in the scratch, the records too (the caller takes none), result records as models
    return sc.device_call(h, kind="calibrated", dtype_name="float64", name="forest", rate=1.0, keep="finite", p_max=9000, stride=136, with_transforms=False)


def transforms(h, capi):
    return sc.device_call(h, kind="shared_focal", name="defects", transforms_only=True)


def scene_larger(h, capi):  # sixteen times the pixels and the tiles, more rows: every part of the scratch grows and moves
    return sc.device_call(h, tile=4, rate=0.5, p_max=120000)


def refused(h, capi):
    with pytest.raises(capi.MdrpError) as e:
        sc.device_call(h, change=lambda a: setattr(a["opt"], "thr", 0))
    return (str(e.value).encode(),)


def two_view(h, capi):
    return rc.device_call(h)


def larger_estimate(h, capi):
    from mdrp_amd import synth
    b = synth.make_batch(5300, 6, 300, noise_px=0.5, outlier_frac=0.3)
    ro = capi.ransac_opt_from_dict({"max_iterations": 200, "min_iterations": 200, "max_epipolar_error": 2.0, "max_reproj_error": 16.0})
    res, mask = h.estimate_batch(capi.SHARED_FOCAL, b["x1"], b["x2"], b["d1"], b["d2"], ro, capi.bundle_opt_from_dict({"loss_type": "TRUNCATED_CAUCHY"}))
    return (res.tobytes(), mask.tobytes())


NEW = {"scene_small": scene_small, "scene_calibrated": scene_calibrated, "transforms": transforms, "scene_larger": scene_larger}
OLD = {"refused": refused, "two_view": two_view, "larger_estimate": larger_estimate}
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
    want = sc.reference("varying_focal", "float32", "chain", "not_inf", 0.5, 6000)
    assert fresh["scene_small"] == tuple(w.tobytes() for w in want)
    want = sc.reference("calibrated", "float64", "forest", "finite", 1.0, 9000)
    assert fresh["scene_calibrated"][:3] == tuple(w.tobytes() for w in want[:3])
    assert fresh["transforms"] == (sc.transforms("shared_focal", "defects").tobytes(),)
    offsets = np.frombuffer(fresh["scene_larger"][2], dtype=np.int64)
    small = np.frombuffer(fresh["scene_small"][2], dtype=np.int64)
    assert offsets[-1] > 10 * small[-1] > 0 and fresh["scene_larger"][3] == fresh["scene_small"][3]  # the same tree: the same records
    assert fresh["two_view"] == tuple(w.tobytes() for w in rc.reference("varying_focal", "float32", rc.SIZES[2], "not_inf", 0.5, 3, 700))


@pytest.mark.parametrize("new", sorted(NEW))
def test_a_scene_call_behind_and_in_front_of_every_other_call(capi, fresh, new):
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
