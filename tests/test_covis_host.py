"""Co-visibility without a GPU (include/mdrp_covis.h): the NumPy definition (mdrp_amd/frontend.py covisibility_pair_numpy and
covisibility_image_pairs_numpy, rules C1-C7) pinned by its own properties - class nesting, the subset rule of the subsample, batch independence, the
half-pixel rule on the identity model, a rendered two-view scene under the true and under a wrong model, the two directions against each other -
the Python layer's refusals, header, binding and build against each other, and the header's host arithmetic (tests/hostmath/covis_host.cpp) against
the definition as bytes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import covis_cases as cc
from mdrp_amd import _capi, frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mdrp_covisibility_pairs_async", "mdrp_covisibility_image_pairs_async")
S, F, I, K, CO, OC, VI = range(7)  # the slots of C7
ALL = frontend.RECON_ALL


def _pair(kind, dt, size, b, rate=1.0, tol=0.05):
    return cc.pair_counts(kind, dt, size, rate, tol, b)


def _direction(kind, dt, size, b, direction, rate=1.0, tol=0.05):
    x = cc.inputs(kind, dt, size)
    side = (("dm1", "c1", "cam1"), ("dm2", "c2", "cam2"))
    (ds, cs, ks), (dg, cg, kg) = side[direction], side[1 - direction]
    lo, hi = frontend.covis_band(tol)
    return frontend.covisibility_direction_numpy(x["models"][b], kind, direction, x[ds][b], x[dg][b], x[cs][b], x[cg][b], None if x[ks] is None else x[ks][b],
                                                 None if x[kg] is None else x[kg][b], frontend.recon_threshold(rate), cc.SEED, lo, hi)


# ---- the definition's own properties
@pytest.mark.parametrize("kind", cc.KINDS)
def test_classes_nest_and_the_last_three_partition_known(kind):
    seen = np.zeros(8, dtype=np.int64)
    for size in cc.SIZES:
        for tol in cc.TOLS:
            c = cc.reference(kind, "float32", size, 0.5, tol, cc.B_MAX).astype(np.int64)
            assert c.shape == (cc.B_MAX, 2, 8) and (c >= 0).all() and (c[..., 7] == 0).all()
            assert (c[..., S] >= c[..., F]).all() and (c[..., F] >= c[..., I]).all() and (c[..., I] >= c[..., K]).all()
            assert (c[..., K] == c[..., CO] + c[..., OC] + c[..., VI]).all()
            for b in cc.EMPTY:
                assert not c[b].any(), b                                                   # C1
            if size[0][0] >= 37:
                assert (c[cc.BEHIND, :, S] > 0).all() and not c[cc.BEHIND, :, F].any()     # every point behind the target
                assert (c[cc.OUTSIDE, :, F] > 0).all() and not c[cc.OUTSIDE, :, I].any()   # every point outside it
                assert c[cc.INF_MAP[0], 0, S] == 0 and c[cc.INF_MAP[0], 1, S] > 0 and c[cc.INF_MAP[0], 1, K] == 0  # a map of inf: no source, no known target
                assert (c[0, :, I] > c[0, :, K]).all()                                     # planted depths in the target
            seen += c.sum(axis=(0, 1))
    assert (seen[:7] > 0).all(), seen  # every class is populated somewhere: the cases do what they are there for


@pytest.mark.parametrize("kind", cc.KINDS)
def test_a_smaller_rate_counts_a_subset(kind):
    """C3: the candidates at a smaller thr are a subset, and the counts at the smaller rate are exactly the counts of that subset's pixels"""
    size, dt = cc.SIZES[3], "float64"
    for b in (0, 3):
        for direction in range(2):
            v, u, classes, _, _ = _direction(kind, dt, size, b, direction, 1.0)
            h, w = size[direction]
            prev = None
            for rate in (0.5, 0.05):
                cand = frontend.recon_candidates(h, w, frontend.recon_threshold(rate), cc.SEED, frontend.COVIS_STAGES[direction])
                want = frontend.covis_counts(classes[cand[v, u]])
                got = _pair(kind, dt, size, b, rate)[direction]
                assert got.tobytes() == want.tobytes(), (b, direction, rate)
                assert (got <= _pair(kind, dt, size, b, 1.0)[direction]).all() and (prev is None or (got <= prev).all())
                assert 0 < got[S] < (classes != 0).sum()
                prev = got
    assert frontend.COVIS_STAGES == (6, 7) and not set(frontend.COVIS_STAGES) & ({1, 2, frontend.SCENE_STAGE} | set(frontend.RECON_STAGES))


def test_a_pair_does_not_depend_on_its_batch():
    kind, dt = "varying_focal", "float32"
    x = cc.inputs(kind, dt, ((37, 53), (37, 53)))
    dm = np.concatenate([x["dm1"][:4], x["dm2"][:4]])
    ms = x["models"]
    lo, hi = frontend.covis_band(0.05)
    thr = frontend.recon_threshold(0.5)
    full = frontend.covisibility_image_pairs_numpy(ms[[0, 3, 2, 3]], kind, dm, [[0, 4], [3, 7], [9, 0], [1, 6]], x["c1"][:8], None, None, None, thr, cc.SEED, lo, hi)
    again = frontend.covisibility_image_pairs_numpy(ms[[3, 3, 0]], kind, dm, [[1, 6], [3, 7], [0, 4]], x["c1"][:8], None, None, None, thr, cc.SEED, lo, hi)
    assert full[3].tobytes() == again[0].tobytes() and full[1].tobytes() == again[1].tobytes() and full[0].tobytes() == again[2].tobytes()
    alone = frontend.covisibility_pair_numpy(ms[3], kind, dm[3], dm[7], x["c1"][3], x["c1"][7], None, None, thr, cc.SEED, lo, hi)
    assert alone.tobytes() == full[1].tobytes() and alone[:, S].min() > 100
    assert not full[2].any() and full[0].any()  # an index outside the set: all counters zero


@pytest.mark.parametrize("kind", cc.KINDS)
def test_the_identity_model_on_identical_maps_is_consistent_everywhere(kind):
    """the half-pixel rule: unprojection takes the integer u for the pixel's own coordinate, so the projection of a pixel's own point is u up to a
    rounding either way, and the nearest pixel - not the truncated one - is the pixel itself.  With tol = 0 the band is the depth itself."""
    rng = np.random.default_rng(5)
    h, w = 45, 61
    dm = rng.uniform(0.5, 30.0, size=(h, w))
    junk = {(3, 4): np.inf, (7, 50): -np.inf, (20, 20): np.nan, (44, 60): 0.0, (0, 0): -2.5, (30, 1): np.inf}
    for at, val in junk.items():
        dm[at] = val
    m = np.zeros((), dtype=_capi.MODEL_DTYPE)
    m["q"], m["scale"] = [1.0, 0.0, 0.0, 0.0], 1.0
    m["f1"] = m["f2"] = 1.0 if kind == "calibrated" else 77.7
    cam = {"model_id": 1, "params": [91.3, 88.1, 30.37, 22.61]} if kind == "calibrated" else None
    centre = np.array([0.25, -0.75]) if kind == "calibrated" else np.array([30.3, 22.9])
    for dtype in (np.float32, np.float64):
        d = dm.astype(dtype)
        for lo, hi in ((1.0, 1.0), (0.95, 1.05)):
            c = frontend.covisibility_pair_numpy(m, kind, d, d, centre, centre, cam, cam, ALL, 0, lo, hi)
            assert c[0].tobytes() == c[1].tobytes()
            assert c[0, S] == h * w - len(junk) and (c[:, CO] == c[:, S]).all() and not c[:, OC].any() and not c[:, VI].any(), c
        for direction in range(2):
            v, u, classes, vt, ut = frontend.covisibility_direction_numpy(m, kind, direction, d, d, centre, centre, cam, cam, ALL, 0, 1.0, 1.0)
            assert (vt == v).all() and (ut == u).all() and not set(zip(v.tolist(), u.tolist())) & set(junk)


# ---- a rendered scene: a fronto-parallel wall and a nearer box, two cameras side by side
FOCAL, TX, Z_WALL, Z_BOX, SCALE, H, W = 100.0, 0.2, 4.0, 2.0, 1.25, 64, 128
CENTRE = np.array([64.0, 32.0])
BOX = ((39.5, 79.5), (15.5, 47.5))  # the box's face in image 1, in pixels: its edges lie between pixel centres


def _render():
    """Depth maps of the two cameras.  Camera 2 sees X2 = (X1 + t) / scale with t = (TX, 0, 0): it stands to the left of camera 1, both look along z.
    The disparities FOCAL * TX / z are whole pixels (10 on the box, 5 on the wall), so a pixel centre of one image meets a pixel centre of the other
    and no comparison is decided by which of two neighbours is the nearer."""
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    maps = []
    for shift in (0.0, FOCAL * TX / Z_BOX):  # the box's face in image 2 lies 10 pixels to the right
        on_box = (u > BOX[0][0] + shift) & (u < BOX[0][1] + shift) & (v > BOX[1][0]) & (v < BOX[1][1])
        maps.append(np.where(on_box, Z_BOX, Z_WALL))
    return maps[0], maps[1] / SCALE  # image 2's depths are in its own unit


def _scene_model(kind, scale=SCALE):
    m = np.zeros((), dtype=_capi.MODEL_DTYPE)
    m["q"], m["t"], m["scale"] = [1.0, 0.0, 0.0, 0.0], [TX, 0.0, 0.0], scale
    m["f1"] = m["f2"] = 1.0 if kind == "calibrated" else FOCAL
    cam = {"model_id": 0, "params": [FOCAL, CENTRE[0], CENTRE[1], 0.0]} if kind == "calibrated" else None
    return m, cam, (None if kind == "calibrated" else CENTRE)


@pytest.mark.parametrize("kind", cc.KINDS)
def test_a_rendered_scene_under_the_true_and_under_a_wrong_model(kind):
    d1, d2 = _render()
    lo, hi = frontend.covis_band(0.05)
    m, cam, c = _scene_model(kind)
    good = frontend.covisibility_pair_numpy(m, kind, d1, d2, c, c, cam, cam, ALL, 0, lo, hi)
    assert (good[:, S] == H * W).all() and (good[:, F] == H * W).all()
    assert (good[:, VI] == 0).all(), good           # nothing floats in front of a surface the other camera saw
    assert (good[:, OC] > 0).all(), good            # each camera looks past the box's edge at wall the other one has the box in front of
    assert (good[:, CO] > H * W // 2).all(), good
    wrong, _, _ = _scene_model(kind, SCALE * 1.5)
    bad = frontend.covisibility_pair_numpy(wrong, kind, d1, d2, c, c, cam, cam, ALL, 0, lo, hi)
    assert (bad[:, CO] < good[:, CO]).all() and (bad[:, VI] > 0).all(), (good, bad)
    # and at a rate: the same statements on the subsample
    thr = frontend.recon_threshold(0.25)
    g, b = (frontend.covisibility_pair_numpy(mm, kind, d1, d2, c, c, cam, cam, thr, 9, lo, hi) for mm in (m, wrong))
    assert (g[:, VI] == 0).all() and (g[:, OC] > 0).all() and (b[:, CO] < g[:, CO]).all() and (b[:, VI] > 0).all()


@pytest.mark.parametrize("kind", cc.KINDS)
def test_direction_1_is_direction_0_of_the_swapped_pair_under_the_inverted_model(kind):
    """X2 = (R X1 + t) / s inverted is X1 = (R^T X2 - R^T t / s) / (1 / s).  The two computations round differently, so they are compared on the
    rendered scene, whose points meet pixel centres and whose depths are either equal or a factor of two apart: no rounding decides a class.  Every
    pixel is sampled (the two directions hash with different stages)."""
    d1, d2 = _render()
    lo, hi = frontend.covis_band(0.05)
    for scale in (SCALE, SCALE * 1.5):
        m, cam, c = _scene_model(kind, scale)
        inv = m.copy()
        inv["t"], inv["scale"] = [-TX / scale, 0.0, 0.0], 1.0 / scale
        fwd = frontend.covisibility_pair_numpy(m, kind, d1, d2, c, c, cam, cam, ALL, 0, lo, hi)
        swp = frontend.covisibility_pair_numpy(inv, kind, d2, d1, c, c, cam, cam, ALL, 0, lo, hi)
        assert fwd[1].tobytes() == swp[0].tobytes() and fwd[0].tobytes() == swp[1].tobytes(), (scale, fwd, swp)
        assert fwd[1, K] > 0


# ---- the Python layer
def test_python_refusals_and_scores():
    import mdrp_amd.poselib as poselib
    from mdrp_amd import covis
    for name in ("covisibility_pairs_torch", "covisibility_image_pairs_torch", "covisibility_pair", "covisibility_scores"):
        assert getattr(poselib, name) is getattr(covis, name)
    with pytest.raises(ValueError):
        poselib.covisibility_pairs_torch("relpose_5pt", None, None, None)
    with pytest.raises(ValueError):
        poselib.covisibility_pairs_torch("calibrated", None, np.zeros((1, 2, 2)), np.zeros((1, 2, 2)))  # not tensors on the GPU
    with pytest.raises(ValueError):
        poselib.covisibility_image_pairs_torch("calibrated", None, np.zeros((1, 2, 2)), [[0, 0]])
    with pytest.raises(ValueError):
        poselib.covisibility_pair(object(), np.zeros((2, 2)), np.zeros((2, 2)))  # a geometry without cameras
    for rate, seed, tol in ((0.0, 0, 0.05), (float("nan"), 0, 0.05), (-1.0, 0, 0.05), (1e-12, 0, 0.05), (0.5, -1, 0.05), (0.5, 1 << 64, 0.05),
                            (0.5, 0, -0.01), (0.5, 0, 1.01), (0.5, 0, float("nan")), (0.5, 0, float("inf"))):
        with pytest.raises(ValueError):
            covis._options(rate, seed, tol)
    o = covis._options(0.05, 7, 0.05)
    assert (o.thr, o.seed, o.lo, o.hi) == (frontend.recon_threshold(0.05), 7, 1.0 - 0.05, 1.0 + 0.05) and covis._options(2.0, 0, 0.0).thr == ALL
    assert frontend.covis_band(0.0) == (1.0, 1.0) and frontend.covis_band(1.0) == (0.0, 2.0)
    m = cc.models("shared_focal", 1)[0]
    for lo, hi in ((-0.1, 1.0), (1.1, 1.2), (0.9, 0.95), (0.5, np.inf), (np.nan, 1.0)):
        with pytest.raises(ValueError):
            frontend.covisibility_pair_numpy(m, "shared_focal", np.ones((2, 2)), np.ones((2, 2)), lo=lo, hi=hi)
    with pytest.raises(ValueError):
        frontend.covisibility_pair_numpy(m, "relpose_5pt", np.ones((2, 2)), np.ones((2, 2)))
    with pytest.raises(ValueError):
        frontend.covisibility_pair_numpy(cc.models("calibrated", 1)[0], "calibrated", np.ones((2, 2)), np.ones((2, 2)))  # no cameras
    # the scores: ratios with empty denominators, and the weight
    c = np.zeros((3, 2, 8), dtype=np.int32)
    c[0, 0], c[0, 1] = [10, 9, 8, 7, 4, 2, 1, 0], [5, 5, 5, 5, 0, 5, 0, 0]
    c[2, 1] = [6, 6, 6, 6, 6, 0, 0, 0]
    s = poselib.covisibility_scores(c)
    assert s["overlap"].tolist() == [[0.4, 0.0], [0.0, 0.0], [0.0, 1.0]] and s["agreement"].tolist() == [[0.8, 0.0], [0.0, 0.0], [0.0, 1.0]]
    assert s["weight"].tolist() == [4, 0, 6] and s["weight"].dtype == np.int64
    import torch
    t = poselib.covisibility_scores(torch.from_numpy(c))
    assert all(np.array_equal(t[k].numpy(), s[k]) for k in s) and t["weight"].dtype == torch.int64
    assert poselib.covisibility_scores(c[0])["weight"] == 4
    for bad in (np.zeros((2, 7), dtype=np.int32), np.zeros((2, 8)), torch.zeros((3, 2, 8)), np.zeros(8, dtype=np.int32)):
        with pytest.raises(ValueError):
            poselib.covisibility_scores(bad)
    from mdrp_amd import scene
    assert "covisibility_scores" in scene.scene_tree.__doc__
    tree = scene.scene_tree([[0, 1], [1, 2], [0, 2]], s["weight"], 3)  # the weights are taken as they come
    assert tree[:, 1].tolist().count(_capi.SCENE_ROOT) == 1


# ---- header, binding, build, library
def test_header_binding_and_build_agree(tmp_path):
    from mdrp_amd import build
    import __graft_entry__ as ge
    inc = os.path.join(ROOT, "include")
    main = open(os.path.join(inc, "mdrp.h")).read()
    assert int(re.search(r"#define MDRP_ABI_VERSION (0x[0-9a-fA-F]+)", main).group(1), 16) == 6 == _capi.ABI_VERSION  # new symbols only
    for other in sorted(os.listdir(inc)):  # no other header names the new identifiers
        if other != "mdrp_covis.h":
            text = open(os.path.join(inc, other)).read()
            for name in NAMES + ("mdrp_covis_opt", "MDRP_COVIS_SLOTS"):
                assert not re.search(r"\b" + name + r"\b", text), (other, name)
    assert '#include "mdrp_covis.h"' in open(os.path.join(inc, "mdrp_scene.h")).read().rstrip().splitlines()[-2]  # reached from the scene header's tail
    path = os.path.join(inc, "mdrp_covis.h")
    hdr = open(path).read()
    for rule in ("C1.", "C2.", "C3.", "C4.", "C5.", "C6.", "C7.", "32 bytes", "tests/test_gpu_covis_history.py"):
        assert rule in hdr, rule
    deps = [os.path.realpath(d) for d in build.DEPS]
    assert os.path.realpath(path) in deps and os.path.realpath(os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_covis.h")) in deps
    assert sorted(_capi.EXPORTS_COVIS) == sorted(NAMES) == sorted(set(re.findall(r"\b(mdrp_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))))
    others = (set(_capi.EXPORTS) | set(_capi.EXPORTS_CLASSIC_RANKED) | set(_capi.EXPORTS_CLASSIC_MODELS) | set(_capi.EXPORTS_CLASSIC_FRONTEND)
              | set(_capi.EXPORTS_CLASSIC_FOCALS) | set(_capi.EXPORTS_DENSE) | set(_capi.EXPORTS_RECONSTRUCT) | set(_capi.EXPORTS_SCENE))
    assert not set(_capi.EXPORTS_COVIS) & others
    assert "EXPORTS_COVIS" in open(ge.__file__).read()
    t = _capi.CovisOpt
    enums = ["MDRP_COVIS_" + n.upper() for n in _capi.COVIS_CLASSES]
    src = tmp_path / "layout.c"
    src.write_text('#include "mdrp.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n    printf("%zu ", sizeof(mdrp_covis_opt));\n'
                   + "".join(f'    printf("%zu ", offsetof(mdrp_covis_opt, {n}));\n' for n, _ in t._fields_)
                   + "".join(f'    printf("%d ", {e});\n' for e in enums) + '    printf("%d", MDRP_COVIS_SLOTS);\n'
                   + "    return (mdrp_covisibility_pairs_async && mdrp_covisibility_image_pairs_async) ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-Wno-address", str(src), "-I", inc, "-o", str(tmp_path / "layout.o")], check=True)
    build.build()
    lib = _capi.load_library()
    subprocess.run(["gcc", str(tmp_path / "layout.o"), "-o", str(tmp_path / "layout"), build.OUT, "-Wl,--unresolved-symbols=ignore-in-shared-libs"], check=True)
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(build.OUT) + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    out = [int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, env=env).stdout.split()]
    want = [C.sizeof(t)] + [getattr(t, n).offset for n, _ in t._fields_]
    assert out == want + list(range(7)) + [_capi.COVIS_SLOTS] and want[0] == 32, (out, want)
    assert _capi.COVIS_CLASSES == frontend.COVIS_CLASSES and _capi.COVIS_SLOTS == frontend.COVIS_SLOTS == 8
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{(.*?)\} mdrp_covis_opt;", hdr, flags=re.S).group(1), flags=re.S)
    assert re.findall(r"\b(\w+)(?:\[\d+\])?;", body) == [n for n, _ in t._fields_]  # the fields in the header's order
    syms = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        args = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", syms), name
        assert len(getattr(lib, name).argtypes) == len(args) == 10, name
    for method in ("covisibility_pairs_device", "covisibility_image_pairs_device"):
        assert callable(getattr(_capi.Handle, method))
        assert method not in vars(_capi.Handle)  # they sit in a base class: the binding's recorded per-method cases are Handle's own


def test_the_handle_methods_hand_their_arguments_on():
    """the two handle methods against a recording stand-in for the library: the symbol, the argument order, the cameras as host tables"""
    calls = []

    class Lib:
        def __getattr__(self, name):
            if not name.startswith("mdrp_"):
                raise AttributeError(name)
            return lambda *a: calls.append((name, a)) or 0

    h = _capi.Handle.__new__(_capi.Handle)
    h._lib, h._h = Lib(), C.c_void_p(0x1000)
    try:
        cam1, cam2 = cc.cameras(cc.SIZES[2], 3)
        opt = _capi.CovisOpt(77, 0, 5, 0.95, 1.05)
        h.covisibility_pairs_device(_capi.CALIB, _capi.DepthPairs(), opt, 3, 0x2000, 136, 0x3000, cam1, cam2)
        h.covisibility_pairs_device(_capi.SHARED_FOCAL, _capi.DepthImagePairs(), opt, 2, 0x2000, 96, 0x3000)
        h.covisibility_image_pairs_device(_capi.VARYING_FOCAL, _capi.DepthImagePairs(), opt, 2, 0x2000, 96, 0x3000)
        with pytest.raises(ValueError):
            h.covisibility_image_pairs_device(_capi.SHARED_FOCAL, _capi.DepthPairs(), opt, 2, 0x2000, 96, 0x3000)
    finally:
        h._h = None
    (n1, a1), (n2, a2), (n3, a3) = calls
    assert n1 == "mdrp_covisibility_pairs_async" and n2 == n3 == "mdrp_covisibility_image_pairs_async" and len(a1) == len(a2) == len(a3) == 10
    assert a1[1] == _capi.CALIB and a1[4] == 3 and a1[5].value == 0x2000 and a1[6] == 136 and a1[7] is not None and a1[8] is not None and a1[9].value == 0x3000
    assert a2[1] == _capi.SHARED_FOCAL and a2[4] == 2 and a2[6] == 96 and a2[7] is None and a2[8] is None and a2[9].value == 0x3000


# ---- the host build of the kernels' arithmetic (tests/hostmath/covis_host.cpp) against the definition
@pytest.fixture(scope="module")
def ch():
    here = os.path.join(ROOT, "tests", "hostmath")
    src, so = os.path.join(here, "covis_host.cpp"), os.path.join(here, "libcovis_host.so")
    deps = [src] + [os.path.join(ROOT, "mdrp_amd", "csrc", n) for n in ("mdrp_covis.h", "mdrp_reconstruct.h", "mdrp_dense.h", "mdrp_frontend.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", src, "-o", so])
    lib = C.CDLL(so)
    lib.ch_direction.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                 C.c_void_p, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_host_constants(ch):
    limits = (C.c_int * 12)()
    ch.ch_limits(limits)
    assert list(limits) == [*frontend.COVIS_STAGES, _capi.COVIS_SLOTS, len(_capi.COVIS_CLASSES), 224, *range(7)]


@pytest.mark.parametrize("size", cc.SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}")
@pytest.mark.parametrize("kind_id, kind", list(enumerate(cc.KINDS)))
def test_host_arithmetic_equals_the_definition_as_bytes(ch, kind_id, kind, size):
    """every pixel's class mask and target pixel, and the counters, for both directions of pairs that hold every case (both camera models, the
    unusable models, the model behind and the model outside), both depth types, a rate and both tolerances"""
    pairs = [b for b in (0, 1, 2, 3, 4, cc.BEHIND, cc.OUTSIDE, 8, 9) if size[0][0] >= 37 or b < 5]
    for dt in ("float32", "float64"):
        x = cc.inputs(kind, dt, size)
        for b in pairs:
            m = np.ascontiguousarray(x["models"][b:b + 1]).view(np.float64)
            cams = [None if x[k] is None else x[k][b] for k in ("cam1", "cam2")]
            ids = [0 if c is None else int(c["model_id"]) for c in cams]
            par = [None if c is None else np.ascontiguousarray(c["params"], dtype=np.float64) for c in cams]
            maps = [x["dm1"][b].astype(np.float64), x["dm2"][b].astype(np.float64)]
            cen = [x["c1"][b], x["c2"][b]]
            for rate, tol in ((1.0, 0.05), (0.5, 0.0)):
                thr = frontend.recon_threshold(rate)
                lo, hi = frontend.covis_band(tol)
                want = cc.pair_counts(kind, dt, size, rate, tol, b)
                for direction in range(2):
                    src, tgt = maps[direction], maps[1 - direction]
                    (h, w), (ht, wt) = src.shape, tgt.shape
                    c4 = np.ascontiguousarray(np.concatenate([cen[direction], cen[1 - direction]]))
                    classes, target, counts = np.full((h, w), 255, dtype=np.uint8), np.full((h, w, 2), -1, dtype=np.int32), np.full(8, -1, dtype=np.int32)
                    ch.ch_direction(_p(m), kind_id, ids[0], _p(par[0]), ids[1], _p(par[1]), direction, _p(c4), h, w, _p(np.ascontiguousarray(src)), ht, wt,
                                    _p(np.ascontiguousarray(tgt)), thr, cc.SEED & 0xFFFFFFFF, lo, hi, _p(classes), _p(target), _p(counts))
                    assert counts.tobytes() == want[direction].tobytes(), (dt, b, rate, direction, counts, want[direction])
                    if b in cc.EMPTY:
                        continue
                    v, u, cls, vt, ut = _direction(kind, dt, size, b, direction, rate, tol)
                    full_c, full_t = np.zeros((h, w), dtype=np.uint8), np.zeros((h, w, 2), dtype=np.int32)
                    full_c[v, u], full_t[v, u, 0], full_t[v, u, 1] = cls, vt, ut
                    assert classes.tobytes() == full_c.tobytes() and target.tobytes() == full_t.tobytes(), (dt, b, rate, direction)
