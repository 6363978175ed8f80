"""The three back ends on the shared tile walk at real map sizes and image counts on a real MI355X (include/mdrp_reconstruct.h, mdrp_covis.h,
mdrp_scene.h, mdrp_fuse.h), against the NumPy definitions (mdrp_amd/frontend.py) as BYTES, where the shapes of
tests/test_gpu_reconstruct.py, test_gpu_covis.py, test_gpu_scene.py and test_gpu_fuse.py cannot go: every chunked scan with runs of more than one value
per thread.  k_recon_scan and k_scene_scan's phase 0 sum a map's tiles of 1024 pixels in runs of per = ceil(tiles / 256): 409 x 643 is 257 tiles, the
smallest count with per = 2, the last tile ragged; 723 x 727 is 514 tiles, per = 3; each beside a map with another run length, so that s_run is
rewritten between the sides.  k_scene_scan's phase 1 sums the images' counts: 257 images are the smallest set with per = 2, and five workgroups of
k_scene_chain and k_fuse_views, with absent images, images detached by a NaN pose and a second root at indices of 64 and above.  Co-visibility has no
scan; it takes the tile walk past tile 33 for the first time.

The inputs are the existing generators' (tests/reconstruct_cases.py, covis_cases.py, fuse_cases.py: the planted depths, the full mantissas, both camera
models); tests/test_scan_runs_host.py asserts on the CPU that they reach what is claimed here.  Every definition's rows are computed once."""
import numpy as np
import pytest

import covis_cases as cc
import fuse_cases as fc
import reconstruct_cases as rc
import scene_cases as sc

pytestmark = pytest.mark.gpu

_size_id = lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}"  # noqa: E731


def _assert_cloud(got, want, what):
    for name, g, w in zip(("points", "pixel", "counts"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.shape) + what
        if g.tobytes() != w.tobytes():  # the first differing row: its tile against lo and hi tells whose run is wrong
            view = np.uint32 if name == "points" else np.int32
            bad = np.argwhere(g.view(view) != w.view(view))
            raise AssertionError((name,) + what + (len(bad), bad[:3].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


# ---- two-view clouds
@pytest.mark.parametrize("size", rc.WIDE_SIZES, ids=_size_id)
@pytest.mark.parametrize("kind", rc.WIDE_KINDS)
def test_clouds_equal_the_definition(kind, size):
    """B = 2, float32 maps, keep not_inf, rates 1.0 and 0.05, p_max at the true total and inside the last tile of the side with more tiles: the
    per-pair form and the per-image form (the maps as valid regions of one allocation)"""
    for rate in rc.WIDE_RATES:
        for p_max in rc.wide_p_max_cases(kind, "float32", size, "not_inf", rate):
            want = rc.reference(kind, "float32", size, "not_inf", rate, rc.WIDE_B, p_max)
            assert (want[2] > 0).all()
            _assert_cloud(rc.run(kind, "float32", size, "not_inf", rate, rc.WIDE_B, p_max), want, ("pairs", rate, p_max))
            _assert_cloud(rc.run_image_form(kind, "float32", size, "not_inf", rate, rc.WIDE_B, p_max), want, ("image pairs", rate, p_max))


# ---- co-visibility
@pytest.mark.parametrize("size", cc.WIDE_SIZES, ids=_size_id)
def test_covisibility_equals_the_definition(size):
    """one call per size: all 16 counters of both pairs"""
    kind = ("calibrated", "varying_focal", "shared_focal")[cc.WIDE_SIZES.index(size)]
    got, want = cc.run(kind, "float32", size, 1.0, 0.05, cc.WIDE_B), cc.reference(kind, "float32", size, 1.0, 0.05, cc.WIDE_B)
    assert got.dtype == want.dtype and got.shape == want.shape == (cc.WIDE_B, 2, 8) and got.tobytes() == want.tobytes(), (got, want)
    assert (want[:, :, 4:7] > 0).all()  # consistent, occluded and violating pixels in both directions


# ---- scenes
@pytest.mark.parametrize("case", sorted(fc.WIDE_CASES))
@pytest.mark.parametrize("kind", fc.WIDE_KINDS)
def test_scenes_equal_the_definition(kind, case):
    """reconstruct_scene_torch at rates 1.0 and 0.5, p_max at the true total and inside the last tile of image 0 ("wide") or of image 256 ("many"):
    transforms, offsets, points and pixel"""
    for rate in fc.WIDE_RATES:
        for p_max in fc.wide_p_max_cases(sc.wide_rows(kind, "float32", case, "not_inf", rate), fc.WIDE_CASES[case][2]):
            got = sc.wide_run(kind, "float32", case, "not_inf", rate, p_max)
            want = sc.wide_reference(kind, "float32", case, "not_inf", rate, p_max)
            assert got[3].tobytes() == want[3].tobytes(), ("transforms", rate, p_max, np.flatnonzero(got[3] != want[3])[:8])
            assert got[2].dtype == np.int64 and got[2].tobytes() == want[2].tobytes(), ("offsets", rate, p_max, np.flatnonzero(got[2] != want[2])[:8])
            _assert_cloud(got[:2], want[:2], (rate, p_max))


# ---- the consistency filter
@pytest.mark.parametrize("V", fc.WIDE_VS)
@pytest.mark.parametrize("case", sorted(fc.WIDE_CASES))
@pytest.mark.parametrize("kind", fc.WIDE_KINDS)
def test_filtered_scenes_equal_the_definition(kind, case, V):
    """fuse_scene_torch with V = 0 and V = 8 (the view table of fuse_cases.views: the image itself, a duplicate, -1 and I beside the real views),
    under the open gate and the default one, at rates 1.0 and 0.5, p_max at the kept count and inside the last tile of image 0 or of image 256:
    transforms, offsets, support, points and pixel"""
    shape, tree, image = fc.WIDE_CASES[case]
    kept = 0
    for rate in fc.WIDE_RATES:
        setting = (kind, "float32", shape, tree, V, rate, fc.WIDE_TOL)
        for gate in fc.wide_gates(V):
            for p_max in sorted(set(fc.wide_p_max_cases(fc.gated_rows(fc.open_rows(*setting), gate), image))):
                got, want = fc.run(*setting, gate, p_max), fc.reference(*setting, gate, p_max)
                what = (rate, gate, p_max)
                assert got[4].tobytes() == want[4].tobytes(), ("transforms",) + what
                assert got[3].dtype == np.int64 and got[3].tobytes() == want[3].tobytes(), ("offsets",) + what + (np.flatnonzero(got[3] != want[3])[:8],)
                assert got[2].dtype == np.uint8 and got[2].shape == want[2].shape and got[2].tobytes() == want[2].tobytes(), ("support",) + what
                _assert_cloud(got[:2], want[:2], what)
                kept += int(want[3][-1])
    assert kept > 0
