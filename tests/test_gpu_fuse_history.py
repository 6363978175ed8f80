"""The history rule of include/mdrp.h for the entry point of include/mdrp_fuse.h: called behind and in front of a larger call of its own kind, a
refused call, a plain scene, a co-visibility call, a two-view cloud and a plain estimate on ONE handle, it returns the bytes it returns on a fresh
handle - and so do the calls around it.  The filter carves the back end's one scratch buffer per call as the scene does, with the views' records and
rows behind the tile counts: a call that read a record, a row or a tile count of the call before it would show here.  Every comparison is of bytes;
the fresh answers are computed once."""
import pytest

import covis_cases as cc
import fuse_cases as fc
import reconstruct_cases as rc
import scene_cases as sc

pytestmark = pytest.mark.gpu


def fuse_small(h, capi):
    return fc.device_call(h)


def fuse_calibrated(h, capi):  # the camera table in the scratch, the records too (the caller takes none), result records as models, every slot kind
    return fc.device_call(h, kind="calibrated", dtype_name="float64", shape="unequal", tree="forest", V=8, rate=1.0, tol=0.0, gate=(2, 1), keep="finite", p_max=9000,
                          stride=136, with_transforms=False)


def fuse_no_views(h, capi):
    return fc.device_call(h, kind="shared_focal", tree="broken", V=0, gate=(0, 0))


def fuse_larger(h, capi):  # more images' worth of rows at rate 1 and the open gate: the cloud and the offsets grow, the scratch is carved the same
    return fc.device_call(h, tree="star", V=8, rate=1.0, gate=(0, 8), p_max=12000)


def refused(h, capi):
    with pytest.raises(capi.MdrpError) as e:
        fc.device_call(h, change=lambda a: setattr(a["opt"], "n_views", 9))
    return (str(e.value).encode(),)


def scene(h, capi):
    return sc.device_call(h)


def scene_larger(h, capi):  # sixteen times the pixels and the tiles: every part of the scratch grows and moves
    return sc.device_call(h, tile=4, rate=0.5, p_max=120000)


def covisibility(h, capi):
    return cc.device_call(h)


def two_view_cloud(h, capi):
    return rc.device_call(h)


def larger_estimate(h, capi):
    from mdrp_amd import synth
    b = synth.make_batch(5300, 6, 300, noise_px=0.5, outlier_frac=0.3)
    ro = capi.ransac_opt_from_dict({"max_iterations": 200, "min_iterations": 200, "max_epipolar_error": 2.0, "max_reproj_error": 16.0})
    res, mask = h.estimate_batch(capi.SHARED_FOCAL, b["x1"], b["x2"], b["d1"], b["d2"], ro, capi.bundle_opt_from_dict({"loss_type": "TRUNCATED_CAUCHY"}))
    return (res.tobytes(), mask.tobytes())


NEW = {"fuse_small": fuse_small, "fuse_calibrated": fuse_calibrated, "fuse_no_views": fuse_no_views, "fuse_larger": fuse_larger}
OLD = {"refused": refused, "scene": scene, "scene_larger": scene_larger, "covisibility": covisibility, "two_view_cloud": two_view_cloud, "larger_estimate": larger_estimate}
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
    assert fresh["fuse_small"] == tuple(w.tobytes() for w in fc.reference("varying_focal", "float32", "37x53", "chain", 3, 0.5, 0.05, (1, 0), 6000))
    want = fc.reference("calibrated", "float64", "unequal", "forest", 8, 1.0, 0.0, (2, 1), 9000, "finite")
    assert fresh["fuse_calibrated"][:4] == tuple(w.tobytes() for w in want[:4])
    assert fresh["fuse_no_views"] == tuple(w.tobytes() for w in fc.reference("shared_focal", "float32", "37x53", "broken", 0, 0.5, 0.05, (0, 0), 6000))
    assert fresh["fuse_larger"] == tuple(w.tobytes() for w in fc.reference("varying_focal", "float32", "37x53", "star", 8, 1.0, 0.05, (0, 8), 12000))
    larger, small = (np.frombuffer(fresh[k][3], dtype=np.int64) for k in ("fuse_larger", "fuse_small"))
    assert larger[-1] > 4 * small[-1] > 0
    assert fresh["scene"] == tuple(w.tobytes() for w in sc.reference("varying_focal", "float32", "chain", "not_inf", 0.5, 6000))
    assert fresh["covisibility"] == (cc.reference("varying_focal", "float32", cc.SIZES[2], 0.5, 0.05, 3).tobytes(),)


@pytest.mark.parametrize("new", sorted(NEW))
def test_a_fuse_call_behind_and_in_front_of_every_other_call(capi, fresh, new):
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
