"""The back end without a GPU (include/mdrp_reconstruct.h): the NumPy definition (mdrp_amd/frontend.py reconstruct_pair_numpy, rules
R1-R7) against the model's own equation and the reference's expression, the subsample's properties, R7's truncation and filler, R1's empty pairs;
the header against the binding, the build and the library; the descriptors' layout; the Python entry points' argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reconstruct_cases as rc
from mdrp_amd import _capi, frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mdrp_reconstruct_pairs_async", "mdrp_reconstruct_image_pairs_async")


def _quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _model(q, t, scale, shift1=0.0, shift2=0.0, f1=1.0, f2=1.0):
    m = np.zeros((), dtype=_capi.MODEL_DTYPE)
    m["q"], m["t"], m["scale"], m["shift1"], m["shift2"], m["f1"], m["f2"] = q, t, scale, shift1, shift2, f1, f2
    return m


# ---- the definition against the geometry it states
@pytest.mark.parametrize("kind", rc.KINDS)
def test_model_equation(kind):
    """Random scene points seen from two cameras with known R, t, scale, shifts and focals: every pixel of image 1 carries the depth of a point, and the
    pixel of image 2 at the same index carries the depth the model's equation R (d1 + shift1) K1^-1 x1 + t = scale (d2 + shift2) K2^-1 x2 gives the
    same point.  Image 2's pixel grid cannot hold the projections, so the equation is checked where it is stated: image 1's transformed point must be
    (d2 + shift2) K2^-1 x2 for the x2 and d2 the scene gives, to 1e-9 relative - float64 rounding over about ten operations."""
    rng = np.random.default_rng(5)
    from mdrp_amd.poselib import _quat_to_R
    h, w = 24, 31
    q, t, scale, s1, s2 = _quat(rng), rng.normal(size=3) * 0.3, 1.7, 0.21, -0.13
    f1, f2 = (640.0, 580.0) if kind == "varying_focal" else ((610.0, 610.0) if kind == "shared_focal" else (1.0, 1.0))
    cam1 = {"model_id": 1, "params": [700.0, 650.0, 15.5, 12.25]} if kind == "calibrated" else None
    cam2 = {"model_id": 0, "params": [590.0, 14.0, 11.0, 0.0]} if kind == "calibrated" else None
    c1 = np.array([15.0, 12.0]) if kind != "calibrated" else np.array([0.5, -0.25])
    d1 = rng.uniform(2.0, 9.0, size=(h, w))
    m = _model(q, t, scale, s1, s2, f1, f2)
    X1, v, u = frontend.reconstruct_side_numpy(m, kind, 0, d1, c1, cam1)
    assert len(X1) == h * w and (v * w + u == np.arange(h * w)).all()
    # the scene by hand: the point of pixel (v, u) in camera 1, moved by the equation and divided by the scale, is what camera 2 sees
    if kind == "calibrated":
        K1inv = np.linalg.inv(np.array([[700.0, 0, 15.5], [0, 650.0, 12.25], [0, 0, 1]]))
        rays = (K1inv @ np.stack([u - c1[0], v - c1[1], np.ones(h * w)])).T
    else:
        rays = np.stack([(u - c1[0]) / f1, (v - c1[1]) / f1, np.ones(h * w)], axis=1)
    P2 = ((_quat_to_R(q) @ (rays * (d1.reshape(-1, 1) + s1)).T).T + t) / scale  # = (d2 + shift2) K2^-1 x2
    assert np.abs(X1 - P2).max() <= 1e-9 * np.abs(P2).max()
    # and image 2's own points from the x2, d2 of that scene land on the same points: unproject the projections through the definition's side 2
    d2 = P2[:, 2] - s2
    x2n = P2[:, :2] / P2[:, 2:3]
    if kind == "calibrated":
        px = x2n * 590.0 + np.array([14.0, 11.0])
    else:
        px = x2n * f2
    # side 2 reads integer pixels, the scene's x2 are not: evaluate R5 by its lines on the floating x2 instead
    rx, ry, cx, cy = frontend._recon_intrinsics(m, kind, 1, cam2)
    z = d2 + s2
    X2 = np.stack([((px[:, 0] - cx) * rx) * z, ((px[:, 1] - cy) * ry) * z, z], axis=1)
    assert np.abs(X1 - X2).max() <= 1e-9 * np.abs(X2).max()


def test_the_readme_expression():
    """zero shifts: the definition is (1 / scale) * (R @ (z * K^-1 [u, v, 1]) + t) with np.linalg.inv(K), to 1e-12 relative"""
    rng = np.random.default_rng(6)
    from mdrp_amd.poselib import _quat_to_R
    h, w = 17, 23
    q, t, scale = _quat(rng), rng.normal(size=3), 0.83
    K = np.array([[512.5, 0.0, 11.25], [0.0, 498.75, 8.5], [0.0, 0.0, 1.0]])
    d = rng.uniform(0.5, 30.0, size=(h, w)).astype(np.float32)
    X, v, u = frontend.reconstruct_side_numpy(_model(q, t, scale), "calibrated", 0, d, None, {"model_id": 1, "params": [512.5, 498.75, 11.25, 8.5]})
    xyz1 = (np.linalg.inv(K) @ np.stack([u, v, np.ones_like(u)]).astype(np.float64)).T * d.astype(np.float64).reshape(-1, 1)
    want = (1 / scale) * ((_quat_to_R(q) @ xyz1.T).T + t)
    assert np.abs(X - want).max() <= 1e-12 * np.abs(want).max()
    X2, _, _ = frontend.reconstruct_side_numpy(_model(q, t, scale), "calibrated", 1, d, None, {"model_id": 1, "params": [512.5, 498.75, 11.25, 8.5]})
    assert np.abs(X2 - xyz1).max() <= 1e-12 * np.abs(xyz1).max()


# ---- R3
def test_subsample_subsets_fraction_and_independence():
    h, w, seed = 480, 640, 77
    masks = {r: [frontend.recon_candidates(h, w, frontend.recon_threshold(r), seed, st) for st in frontend.RECON_STAGES] for r in (0.01, 0.05, 0.5, 1.0)}
    for side in range(2):
        for small, large in ((0.01, 0.05), (0.05, 0.5), (0.5, 1.0)):
            assert not (masks[small][side] & ~masks[large][side]).any()
        assert masks[1.0][side].all()
        for r in (0.05, 0.5):
            frac = masks[r][side].mean()
            print("rate", r, "side", side, "kept fraction", frac)
            assert abs(frac - r) <= 0.05 * r
    for r in (0.05, 0.5):  # the two sides' sets are independent: the overlap is rate^2, within six binomial standard deviations
        both = (masks[r][0] & masks[r][1]).mean()
        print("rate", r, "overlap", both)
        assert abs(both - r * r) <= 6.0 * np.sqrt(r * r * (1 - r * r) / (h * w))
    assert not (frontend.recon_candidates(h, w, frontend.recon_threshold(0.05), seed + 1, 3) == masks[0.05][0]).all()
    assert frontend.recon_threshold(1.0) == frontend.recon_threshold(7.0) == frontend.RECON_ALL and frontend.recon_threshold(0.5) == 1 << 31
    for bad in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            frontend.recon_threshold(bad)
    with pytest.raises(ValueError):
        frontend.recon_candidates(65537, 1, frontend.RECON_ALL, 0, 3)
    assert (frontend.recon_hash(1 << 32 | 5, 3, [7], [9]) == frontend.recon_hash(5, 3, [7], [9])).all()  # the seed's low 32 bits


def test_the_hash_is_d4s():
    """stage 3 / 4 of the dense sampler's hash on k = (v << 16) | u"""
    v, u = np.array([0, 1, 479, 65535]), np.array([0, 639, 5, 65535])
    for stage in frontend.RECON_STAGES:
        want = (frontend.dense_u(99, stage, (v.astype(np.uint64) << np.uint64(16)) | u.astype(np.uint64)))
        assert (frontend.recon_hash(99, stage, v, u) >> np.uint32(8) == want).all()


# ---- R4, R7, R1
def _small_pair():
    rng = np.random.default_rng(8)
    d1, d2 = rng.uniform(1.0, 5.0, size=(5, 6)), rng.uniform(1.0, 5.0, size=(4, 3))
    d1[0, 0], d1[1, 2], d1[2, 2], d2[0, 1] = np.inf, -np.inf, np.nan, np.nan
    return _model(_quat(rng), rng.normal(size=3), 1.3, 0.1, 0.2, 500.0, 600.0), d1, d2


def test_depth_filter():
    m, d1, d2 = _small_pair()
    _, pixel, counts = frontend.reconstruct_pair_numpy(m, "varying_focal", d1, d2)
    assert counts.tolist() == [28, 12] and 0 not in pixel[:28] and 8 not in pixel[:28] and 14 in pixel[:28]  # the NaN stays, as in the scripts
    points, pixel, counts = frontend.reconstruct_pair_numpy(m, "varying_focal", d1, d2, keep="finite")
    assert counts.tolist() == [27, 11] and 14 not in pixel[:27] and np.isfinite(points).all()
    with pytest.raises(ValueError):
        frontend.reconstruct_pair_numpy(m, "varying_focal", d1, d2, keep="both_inf")


def test_truncation_and_filler():
    m, d1, d2 = _small_pair()
    full_p, full_x, full_c = frontend.reconstruct_pair_numpy(m, "shared_focal", d1, d2)
    n1, n2 = (int(v) for v in full_c)
    assert len(full_x) == n1 + n2 and (full_x >= 0).all() and full_p.dtype == np.float32 and full_x.dtype == np.int32 and full_c.dtype == np.int32
    for p_max in (0, n1 // 2, n1, n1 + n2 // 2, n1 + n2, n1 + n2 + 3):
        p, x, c = frontend.reconstruct_pair_numpy(m, "shared_focal", d1, d2, p_max=p_max)
        k = min(p_max, n1 + n2)
        assert p.shape == (p_max, 3) and x.shape == (p_max,) and c.tolist() == [n1, n2]  # the counts are the true ones
        assert p[:k].tobytes() == full_p[:k].tobytes() and (x[:k] == full_x[:k]).all()  # image 2 starts at min(n1, p_max)
        assert not p[k:].any() and (x[k:] == -1).all()
    _, x, _ = frontend.reconstruct_pair_numpy(m, "shared_focal", d1, d2, w_alloc1=10, w_alloc2=4)
    assert x[0] == 1 and x[5] == 10 and x[n1] == 0 and x[n1 + 3] == 4  # pixel counts rows by the allocated length (maps 5 x 6 and 4 x 3)


@pytest.mark.parametrize("what, kind", [("nan_q", "calibrated"), ("zero_scale", "shared_focal"), ("f1", "varying_focal"), ("f2", "shared_focal"),
                                        ("inf_shift", "calibrated")])
def test_an_unusable_model_is_an_empty_pair(what, kind):
    m, d1, d2 = _small_pair()
    cam = {"model_id": 0, "params": [500.0, 3.0, 2.0, 0.0]}
    if what == "nan_q":
        m["q"][0] = np.nan
    elif what == "zero_scale":
        m["scale"] = 0.0
    elif what == "f1":
        m["f1"] = -1.0
    elif what == "f2":
        m["f2"] = np.inf
    else:
        m["shift1"] = np.inf
    p, x, c = frontend.reconstruct_pair_numpy(m, kind, d1, d2, camera1=cam, camera2=cam, p_max=9)
    assert c.tolist() == [0, 0] and not p.any() and (x == -1).all()
    m2 = _small_pair()[0]
    m2["f1"] = -1.0  # the focals are not the calibrated kind's
    assert frontend.reconstruct_pair_numpy(m2, "calibrated", d1, d2, camera1=cam, camera2=cam)[2].tolist() == [28, 12]


def test_image_pairs_are_a_loop_over_pairs():
    rng = np.random.default_rng(9)
    dm = rng.uniform(1.0, 4.0, size=(3, 6, 7)).astype(np.float32)
    sizes = np.array([[6, 7], [4, 5], [9, 3]])
    pairs = np.array([[0, 1], [1, 1], [2, 0], [0, 3], [-1, 0]])
    ms = rc.models("varying_focal", 5)
    ms[1] = ms[0]
    cs = rng.uniform(0, 3, size=(3, 2))
    p, x, c = frontend.reconstruct_image_pairs_numpy(ms, "varying_focal", dm, pairs, 60, cs, sizes)
    assert c.tolist() == [[42, 20], [20, 20], [18, 42], [0, 0], [0, 0]]
    want = frontend.reconstruct_pair_numpy(ms[2], "varying_focal", dm[2][:6, :3], dm[0], cs[2], cs[0], p_max=60, w_alloc1=7, w_alloc2=7)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((p[2], x[2], c[2]), want))
    assert x[2, 3] == 7 and x[1, 5] == 7  # row 1 of a map whose valid width is 3 (5): the allocated row length


# ---- header, binding, build, library
def test_header_binding_and_build_agree(tmp_path):
    from mdrp_amd import build
    import __graft_entry__ as ge
    main = open(os.path.join(ROOT, "include", "mdrp.h")).read()
    assert int(re.search(r"#define MDRP_ABI_VERSION (0x[0-9a-fA-F]+)", main).group(1), 16) == 6 == _capi.ABI_VERSION
    for name in NAMES + ("mdrp_depth_pairs", "MDRP_KEEP_FINITE"):
        assert not re.search(r"\b" + name + r"\b", main), name
    assert '#include "mdrp_reconstruct.h"' in open(os.path.join(ROOT, "include", "mdrp_dense.h")).read()  # mdrp.h reaches it through the dense header
    path = os.path.join(ROOT, "include", "mdrp_reconstruct.h")
    hdr = open(path).read()
    for rule in ("R1.", "R2.", "R3.", "R4.", "R5.", "R6.", "R7."):
        assert rule in hdr, rule
    deps = [os.path.realpath(d) for d in build.DEPS]
    assert os.path.realpath(path) in deps and os.path.realpath(os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_reconstruct.h")) in deps
    assert sorted(_capi.EXPORTS_RECONSTRUCT) == sorted(NAMES) == sorted(set(re.findall(r"\b(mdrp_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))))
    others = (set(_capi.EXPORTS) | set(_capi.EXPORTS_CLASSIC_RANKED) | set(_capi.EXPORTS_CLASSIC_MODELS) | set(_capi.EXPORTS_CLASSIC_FRONTEND)
              | set(_capi.EXPORTS_CLASSIC_FOCALS) | set(_capi.EXPORTS_DENSE))
    assert not set(_capi.EXPORTS_RECONSTRUCT) & others
    assert "EXPORTS_RECONSTRUCT" in open(ge.__file__).read()
    fields = {"mdrp_depth_pairs": _capi.DepthPairs, "mdrp_depth_image_pairs": _capi.DepthImagePairs, "mdrp_reconstruct_opt": _capi.ReconstructOpt}
    src = tmp_path / "layout.c"
    src.write_text('#include "mdrp.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n'
                   + "".join(f'    printf("%zu ", sizeof({s}));\n' + "".join(f'    printf("%zu ", offsetof({s}, {n}));\n' for n, _ in t._fields_) for s, t in fields.items())
                   + '    printf("%d %d %u %d", MDRP_KEEP_NOT_INF, MDRP_KEEP_FINITE, MDRP_RECON_ALL, MDRP_RECON_MAX_EXTENT);\n'
                   + "    return (mdrp_reconstruct_pairs_async && mdrp_reconstruct_image_pairs_async) ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-Wno-address", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout.o")], check=True)
    build.build()
    lib = _capi.load_library()
    subprocess.run(["gcc", str(tmp_path / "layout.o"), "-o", str(tmp_path / "layout"), build.OUT, "-Wl,--unresolved-symbols=ignore-in-shared-libs"], check=True)
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(build.OUT) + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    out = [int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, env=env).stdout.split()]
    want = []
    for t in fields.values():
        want += [C.sizeof(t)] + [getattr(t, n).offset for n, _ in t._fields_]
    assert out == want + [_capi.RECON_KEEP["not_inf"], _capi.RECON_KEEP["finite"], _capi.RECON_ALL, _capi.RECON_MAX_EXTENT], (out, want)
    for struct, t in fields.items():  # the fields in the header's order
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} " + struct + ";", hdr, flags=re.S).group(1), flags=re.S)
        declared = [n for decl in re.findall(r"[\w ]+?((?:\*?\w+\s*,\s*)*\*?\w+)\s*;", body) for n in re.findall(r"\w+", decl)]
        assert declared == [f[0] for f in t._fields_], (struct, declared)
    syms = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        args = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", syms), name
        assert len(getattr(lib, name).argtypes) == len(args) == 12, name
    for method in ("reconstruct_pairs_device", "reconstruct_image_pairs_device"):
        assert callable(getattr(_capi.Handle, method))


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
        cams = rc.cameras(2)
        opt = _capi.ReconstructOpt(1, 77, 5, 9, 0)
        h.reconstruct_pairs_device(_capi.CALIB, _capi.DepthPairs(), opt, 2, 0x2000, 136, 0x3000, 0x4000, 0x5000, cams[0], cams[1])
        h.reconstruct_image_pairs_device(_capi.SHARED_FOCAL, _capi.DepthImagePairs(), opt, 2, 0x2000, 96, 0x3000, 0x4000, 0x5000)
        with pytest.raises(ValueError):
            h.reconstruct_image_pairs_device(_capi.SHARED_FOCAL, _capi.DepthPairs(), opt, 2, 0x2000, 96, 0x3000, 0x4000, 0x5000)
    finally:
        h._h = None
    (n1, a1), (n2, a2) = calls
    assert n1 == "mdrp_reconstruct_pairs_async" and n2 == "mdrp_reconstruct_image_pairs_async" and len(a1) == len(a2) == 12
    assert a1[1] == _capi.CALIB and a1[4] == 2 and a1[5].value == 0x2000 and a1[6] == 136 and [p.value for p in a1[9:]] == [0x3000, 0x4000, 0x5000]
    assert a1[7] is not None and a1[8] is not None and a2[7] is None and a2[8] is None and a2[6] == 96


# ---- the Python entry points' own refusals (no device is touched)
def test_default_p_max_is_integer_and_covers_the_binomial():
    from mdrp_amd import reconstruct
    pixels = 2 * 480 * 640
    assert reconstruct.default_p_max(pixels, _capi.RECON_ALL) == pixels
    thr = frontend.recon_threshold(0.05)
    p = reconstruct.default_p_max(pixels, thr)
    mean, sd = pixels * 0.05, np.sqrt(pixels * 0.05 * 0.95)
    assert isinstance(p, int) and mean + 8 * sd + 64 <= p <= mean + 8 * sd + 64 + 10
    assert reconstruct.default_p_max(10, thr) == 10 and reconstruct.default_p_max(0, thr) == 0
    kept = sum(int(frontend.recon_candidates(480, 640, thr, 3, st).sum()) for st in frontend.RECON_STAGES)
    assert kept <= p


def test_the_entry_points_are_poselibs():
    import mdrp_amd.poselib as poselib
    from mdrp_amd import reconstruct
    for name in ("reconstruct_pairs_torch", "reconstruct_image_pairs_torch", "reconstruct_pair"):
        assert getattr(poselib, name) is getattr(reconstruct, name)
    with pytest.raises(ValueError):
        poselib.reconstruct_pairs_torch("relpose_5pt", None, None, None)
    with pytest.raises(ValueError):
        poselib.reconstruct_pairs_torch("calibrated", None, np.zeros((1, 2, 2)), np.zeros((1, 2, 2)))  # not tensors on the GPU
    with pytest.raises(ValueError):
        poselib.reconstruct_pair(poselib.MonoDepthTwoViewGeometry(), np.zeros((2, 2)), np.zeros((2, 2)))  # no cameras
    for bad in (dict(rate=0.0), dict(rate=float("nan")), dict(rate=1e-12), dict(keep="both_inf"), dict(seed=-1), dict(p_max=-1)):
        args = dict(rate=0.05, seed=0, keep="not_inf", p_max=None, pixels=100)
        args.update(bad)
        with pytest.raises(ValueError):
            reconstruct._options(**args)
    with pytest.raises(ValueError):
        reconstruct._check_maps(65537, 1)


# ---- the host build of the kernels' arithmetic (tests/hostmath/reconstruct_host.cpp) against the definition
@pytest.fixture(scope="module")
def rh():
    here = os.path.join(ROOT, "tests", "hostmath")
    src, so = os.path.join(here, "reconstruct_host.cpp"), os.path.join(here, "libreconstruct_host.so")
    deps = [src] + [os.path.join(ROOT, "mdrp_amd", "csrc", n) for n in ("mdrp_reconstruct.h", "mdrp_dense.h", "mdrp_frontend.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", src, "-o", so])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_host_arithmetic_equals_the_definition(rh):
    limits = (C.c_int * 6)()
    rh.rh_limits(limits)
    assert list(limits) == [_capi.RECON_KEEP["not_inf"], _capi.RECON_KEEP["finite"], _capi.RECON_MAX_EXTENT, *frontend.RECON_STAGES, _capi.MODEL_DTYPE.itemsize]
    rng = np.random.default_rng(17)
    v, u = rng.integers(0, 65536, 4000).astype(np.uint32), rng.integers(0, 65536, 4000).astype(np.uint32)
    v[:4], u[:4] = (0, 65535, 0, 65535), (0, 0, 65535, 65535)
    out = np.zeros(4000, dtype=np.uint32)
    for seed in (0, 1, 0xFFFFFFFF, 0x1234ABCD5 & 0xFFFFFFFF):
        for stage in frontend.RECON_STAGES:
            rh.rh_hash(C.c_uint32(seed), C.c_uint32(stage), 4000, _p(v), _p(u), _p(out))
            assert (out == frontend.recon_hash(seed, stage, v, u)).all()
    thr = frontend.recon_threshold(0.3)
    cand = frontend.recon_candidates(8, 9, thr, 5, 4)
    assert all(rh.rh_candidate(C.c_uint32(thr), 5, 4, i, j) == cand[i, j] for i in range(8) for j in range(9))
    assert rh.rh_candidate(C.c_uint32(frontend.RECON_ALL), 5, 4, 3, 3) == 1
    rh.rh_keep.argtypes = [C.c_double, C.c_int]
    for d in (0.0, -1.5, np.inf, -np.inf, np.nan, 1e308):
        for keep in frontend.KEEPS:
            assert rh.rh_keep(d, _capi.RECON_KEEP[keep]) == bool(frontend.recon_keep(np.float64(d), keep)), (d, keep)
    for kind_id, kind in enumerate(rc.KINDS):
        ms = rc.models(kind)
        for b in range(len(ms)):
            assert rh.rh_usable(_p(ms[b:b + 1]), kind_id) == frontend.recon_usable(ms[b], kind), (kind, b)
        for field in ("q", "t", "scale", "shift1", "shift2", "f1", "f2"):
            for bad in (np.nan, np.inf, 0.0, -2.0):
                m = ms[0:1].copy()
                m[field] = bad
                assert rh.rh_usable(_p(m), kind_id) == frontend.recon_usable(m[0], kind), (kind, field, bad)


@pytest.mark.parametrize("kind_id, kind", list(enumerate(rc.KINDS)))
def test_host_points_equal_the_definition_as_bytes(rh, kind_id, kind):
    """the pair's record and the point of every pixel, rounded: the bytes of the definition's rows for both images, both camera models, both depth types"""
    rh.rh_points.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p]
    for dtype_name in ("float32", "float64"):
        x = rc.inputs(kind, dtype_name, rc.SIZES[2])
        for b in (0, 3, 6):  # (usable models with no map of inf)
            want = rc.rows(kind, dtype_name, rc.SIZES[2], "not_inf", 1.0, b)
            cams = [(int(x[k][b]["model_id"]), np.ascontiguousarray(x[k][b]["params"])) if x[k] is not None else (0, None) for k in ("cam1", "cam2")]
            for side, dm, c in ((0, x["dm1"][b], x["c1"][b]), (1, x["dm2"][b], x["c2"][b])):
                pixel = want[side][1].astype(np.int64)
                v, u = (pixel // dm.shape[1]).astype(np.uint32), (pixel % dm.shape[1]).astype(np.uint32)
                d = np.ascontiguousarray(dm[v, u].astype(np.float64))
                out = np.zeros((len(pixel), 3), dtype=np.float32)
                rh.rh_points(_p(x["models"][b:b + 1]), kind_id, cams[0][0], None if cams[0][1] is None else _p(cams[0][1]), cams[1][0],
                             None if cams[1][1] is None else _p(cams[1][1]), side, c[0], c[1], len(pixel), _p(v), _p(u), _p(d), _p(out))
                assert len(pixel) > 500 and out.tobytes() == want[side][0].tobytes(), (dtype_name, b, side)
