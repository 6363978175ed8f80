"""Scenes without a GPU (include/mdrp_scene.h): the NumPy definition (mdrp_amd/frontend.py scene_transforms_numpy and
reconstruct_scene_numpy, rules S1-S6) against the geometry it states, the video demo's accumulation and the two-view back end; the tree's detached
images; the host helpers that build a tree; the header against the binding, the build and the library; the record's layout; the host build of the
header's arithmetic against the definition as bytes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import scene_cases as sc
from mdrp_amd import _capi, frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mdrp_scene_transforms_async", "mdrp_reconstruct_scene_async")
E, RT = _capi.SCENE_EDGE, _capi.SCENE_ROOT


def _rot(rng, angle=0.3):
    from mdrp_amd import synth
    return synth.rodrigues(rng.normal(0.0, angle, 3))


def _quat_of(R):
    """(w, x, y, z) of a rotation matrix with a positive trace"""
    w = np.sqrt(1.0 + np.trace(R)) / 2.0
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def _model(R, t, scale, shift1=0.0, shift2=0.0, f1=1.0, f2=1.0):
    m = np.zeros((), dtype=_capi.MODEL_DTYPE)
    m["q"], m["t"], m["scale"], m["shift1"], m["shift2"], m["f1"], m["f2"] = _quat_of(R), t, scale, shift1, shift2, f1, f2
    return m


def _world(kind, I=6, seed=3):
    """A noise-free image set: I cameras X_i = R_i X_w + t_i around the origin, each with its own depth unit alpha_i, shift beta_i and focal f_i
    (metric depth Z = alpha_i (d + beta_i)).  The model of the pair (a, c) is then R = R_c R_a^T, t = (t_c - R t_a) / alpha_a, scale = alpha_c / alpha_a,
    shift1 = beta_a, shift2 = beta_c."""
    rng = np.random.default_rng(seed)
    Rs, ts = [_rot(rng) for _ in range(I)], [rng.normal(0.0, 0.4, 3) for _ in range(I)]
    alpha, beta = rng.uniform(0.5, 2.0, I), rng.normal(0.0, 0.2, I)
    f = np.full(I, 520.0) if kind == "shared_focal" else rng.uniform(400.0, 700.0, I)
    cams = [{"model_id": 0, "params": [f[i], 3.5, -2.25, 0.0]} for i in range(I)] if kind == "calibrated" else None

    def model(a, c):
        R = Rs[c] @ Rs[a].T
        return _model(R, (ts[c] - R @ ts[a]) / alpha[a], alpha[c] / alpha[a], beta[a], beta[c], f[a], f[c])
    return dict(R=Rs, t=ts, alpha=alpha, beta=beta, f=f, cams=cams, model=model, I=I, rng=rng)


def _image_points(w, kind, T, i, Pw):
    """the world points Pw as image i holds them (sub-pixel projections and the depths its map would carry there), through the definition's S5 and S6"""
    Xi = (w["R"][i] @ Pw.T).T + w["t"][i]
    d = Xi[:, 2] / w["alpha"][i] - w["beta"][i]
    u, v = w["f"][i] * Xi[:, 0] / Xi[:, 2], w["f"][i] * Xi[:, 1] / Xi[:, 2]
    if kind == "calibrated":
        u, v = u + 3.5, v - 2.25
    X = frontend.scene_unproject(T[i], kind, v, u, d, None, None if w["cams"] is None else w["cams"][i])
    return frontend.scene_transform_points(T[i], X)


# ---- the definition against the geometry it states
@pytest.mark.parametrize("kind", sc.KINDS)
def test_every_image_meets_its_root(kind):
    """mixed directions, depth up to 3, two components: at corresponding pixels every image's points are its root's, to 1e-9 relative"""
    w = _world(kind)
    pairs = np.array([(1, 0), (1, 2), (3, 2), (5, 4), (0, 3)])
    tree = np.array([(0, RT), (0, E), (1, E), (2, E), (3, RT), (3, E)])
    ms = np.array([w["model"](a, c) for a, c in pairs])
    T = frontend.scene_transforms_numpy(ms, kind, pairs, tree, w["I"])
    assert T["root"].tolist() == [0, 0, 0, 0, 4, 4] and T["depth"].tolist() == [0, 1, 2, 3, 0, 1]
    Pw = w["rng"].normal(0.0, 1.0, (200, 3)) + np.array([0.0, 0.0, 9.0])
    for i in range(w["I"]):
        mine, roots = _image_points(w, kind, T, i, Pw), _image_points(w, kind, T, int(T["root"][i]), Pw)
        err = np.abs(mine - roots).max() / np.abs(roots).max()
        print(kind, "image", i, "depth", T["depth"][i], "relative distance to the root's points", err)
        assert err <= 1e-9
    if kind != "calibrated":
        assert T["f"].tolist() == w["f"].tolist()
    assert T["shift"].tolist() == w["beta"].tolist()


def test_an_edge_and_its_inverse_are_the_identity():
    w = _world("varying_focal")
    m = w["model"](1, 0)
    T = frontend.scene_transforms_numpy(np.array([m, m]), "varying_focal", [(1, 0), (1, 2)], [(0, RT), (0, E), (1, E)], 3)
    assert T["depth"].tolist() == [0, 1, 2] and T["root"].tolist() == [0, 0, 0]
    assert np.abs(T["R"][2].reshape(3, 3) - np.eye(3)).max() <= 1e-12 and np.abs(T["t"][2]).max() <= 1e-12 * np.abs(m["t"]).max()
    assert abs(T["s"][2] - 1.0) <= 1e-12


def test_a_forward_chain_is_the_video_demos_accumulation():
    """make_video.py:310-314 restated (every frame a keyframe): anchor_R' = anchor_R @ R, anchor_t' = anchor_R @ t + scale * anchor_t,
    anchor_scale' = anchor_scale * scale, from the first frame on; the tree composes the same edges from the leaf's end"""
    from mdrp_amd import scene
    w = _world("calibrated", I=9, seed=4)
    pairs, tree = scene.video_tree(9)
    assert pairs.tolist() == [[i, i - 1] for i in range(1, 9)] and tree.tolist() == [[0, RT]] + [[i - 1, E] for i in range(1, 9)]
    ms = np.array([w["model"](a, c) for a, c in pairs])
    T = frontend.scene_transforms_numpy(ms, "calibrated", pairs, tree, 9)
    from mdrp_amd.poselib import _quat_to_R
    anchor_R, anchor_t, anchor_scale = np.eye(3), np.zeros(3), 1.0
    for i in range(1, 9):
        R, t, scale = _quat_to_R(ms[i - 1]["q"]), ms[i - 1]["t"], ms[i - 1]["scale"]
        anchor_R, anchor_t = anchor_R @ R, anchor_R @ t + scale * anchor_t
        anchor_scale *= scale
        assert T["depth"][i] == i and T["root"][i] == 0
        assert np.abs(T["R"][i].reshape(3, 3) - anchor_R).max() <= 1e-12
        assert np.abs(T["t"][i] - anchor_t).max() <= 1e-12 * max(1.0, np.abs(anchor_t).max()) and abs(T["s"][i] - anchor_scale) <= 1e-12 * anchor_scale


def test_two_images_are_the_two_view_back_end():
    """root at c: image c's rows are reconstruct_pair_numpy's rows of image 2 exactly, image a's are its rows of image 1 (1e-12 before the rounding)"""
    rng = np.random.default_rng(7)
    m = sc.rc.models("varying_focal")[0]
    dm = rng.uniform(1.0, 6.0, size=(2, 9, 11)).astype(np.float32)
    dm[0, 2, 3], dm[1, 0, 0], dm[1, 4, 4] = np.inf, -np.inf, np.nan
    cs = rng.uniform(0.0, 5.0, size=(2, 2))
    p, x, off, T = frontend.reconstruct_scene_numpy(np.array([m]), "varying_focal", dm, [(0, 1)], [(0, E), (0, RT)], None, cs)
    want = frontend.reconstruct_rows_numpy(m, "varying_focal", dm[0], dm[1], cs[0], cs[1])
    assert off.tolist() == [0, len(want[0][1]), len(want[0][1]) + len(want[1][1])] and off.dtype == np.int64
    n1 = int(off[1])
    assert p[n1:].tobytes() == want[1][0].tobytes() and x[n1:].tobytes() == want[1][1].tobytes()
    assert x[:n1].tobytes() == want[0][1].tobytes()
    X64, v, u = frontend.reconstruct_side_numpy(m, "varying_focal", 0, dm[0], cs[0])
    mine = frontend.scene_transform_points(T[0], frontend.scene_unproject(T[0], "varying_focal", v, u, dm[0].astype(np.float64)[v, u], cs[0]))
    fin = np.isfinite(X64).all(axis=1)
    assert fin.sum() >= 90 and np.abs(mine - X64)[fin].max() <= 1e-12 * np.abs(X64[fin]).max()


def test_subsample_subsets_and_independence():
    h, w, seed = 120, 160, 77
    masks = {(r, i): frontend.recon_candidates(h, w, frontend.recon_threshold(r), frontend.scene_seed(seed, i), frontend.SCENE_STAGE)
             for r in (0.05, 0.5, 1.0) for i in (0, 1, 2)}
    for i in (0, 1, 2):
        assert not (masks[0.05, i] & ~masks[0.5, i]).any() and masks[1.0, i].all()
        assert abs(masks[0.5, i].mean() - 0.5) <= 0.05 * 0.5
    for i, j in ((0, 1), (1, 2), (0, 2)):  # two images' sets are independent: the overlap is rate^2 within six binomial standard deviations
        assert abs((masks[0.5, i] & masks[0.5, j]).mean() - 0.25) <= 6.0 * np.sqrt(0.25 * 0.75 / (h * w))
    two_view = [frontend.recon_candidates(h, w, frontend.recon_threshold(0.5), seed, st) for st in frontend.RECON_STAGES]
    assert not any((masks[0.5, 0] == m).all() for m in two_view)  # a stage of its own
    assert frontend.scene_seed(1 << 32 | 5, 3) == frontend.scene_seed(5, 3) and frontend.SCENE_STAGE == 5
    # an image's kept set depends on (seed, image, v, u) alone: the same rows whatever else the scene holds
    x = sc.inputs("varying_focal", "float32", "star")
    T = sc.transforms("varying_focal", "star")
    all_rows = sc.rows("varying_focal", "float32", "star", "not_inf", 0.5)
    alone = frontend.scene_image_rows_numpy(T[2], "varying_focal", 2, x["dm"][2][:17, :64], x["centers"][2], None, "not_inf", frontend.recon_threshold(0.5), sc.SEED, sc.W)
    assert alone[0].tobytes() == all_rows[2][0].tobytes() and alone[1].tobytes() == all_rows[2][1].tobytes() and len(alone[1]) > 300


# ---- S1: the tree and its detached images
@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("name", sorted(sc.TREES))
def test_tree_cases(kind, name):
    T = sc.transforms(kind, name)
    want = sc.attached(name, kind)
    for i in range(sc.TREES[name]["I"]):
        if i in want:
            assert (int(T["root"][i]), int(T["depth"][i])) == want[i], (name, i, T[i])
            assert np.isfinite(T["R"][i]).all() and T["s"][i] != 0.0
            assert (T["f"][i] > 0.0) == (kind != "calibrated")
        else:
            assert T[i].tobytes() == np.array([(np.zeros(9), np.zeros(3), 0, 0, 0, -1, -1)], dtype=frontend.SCENE_TRANSFORM_DTYPE).tobytes(), (name, i)
    rows = sc.rows(kind, "float32", name, "not_inf", 1.0)
    assert [r is not None for r in rows] == [i in want for i in range(len(rows))]


def test_a_detached_subtree_leaves_the_rest_as_it_was():
    """the NaN pose in mid-chain: the images on the root's side of it keep their bytes, everything below is detached"""
    kind = "shared_focal"
    x = sc.inputs(kind, "float32", "chain")
    good = sc.transforms(kind, "chain")
    ms = x["models"].copy()
    ms[4] = sc.rc.models(kind)[1]  # a NaN in q: the edge between images 4 and 5
    T = frontend.scene_transforms_numpy(ms, kind, x["pairs"], x["tree"], 9)
    assert T[:5].tobytes() == good[:5].tobytes() and (T["depth"][5:] == -1).all() and (T["root"][5:] == -1).all()
    assert good["depth"].tolist() == list(range(9))


def test_pair_less_roots_per_kind():
    dm = np.ones((1, 2, 2), dtype=np.float32)
    for kind in sc.KINDS:
        cams = [{"model_id": 0, "params": [50.0, 1.0, 1.0, 0.0]}] if kind == "calibrated" else None
        p, x, off, T = frontend.reconstruct_scene_numpy(np.zeros(0, dtype=_capi.MODEL_DTYPE), kind, dm, np.zeros((0, 2), int), [(-1, RT)], cameras=cams)
        if kind == "calibrated":
            assert off.tolist() == [0, 4] and T["depth"][0] == 0 and T["shift"][0] == 0.0 and p[3].tolist() == [0.0, 0.0, 1.0]
        else:
            assert off.tolist() == [0, 0] and T["depth"][0] == -1


def test_truncation_and_filler():
    kind, dt, name = "varying_focal", "float32", "star"
    full = sc.reference(kind, dt, name, "not_inf", 0.5, None)
    n = int(full[2][-1])
    assert len(full[1]) == n > 1000 and (np.diff(full[2]) >= 0).all()
    for p_max in sc.p_max_cases(kind, dt, name, "not_inf", 0.5):
        p, x, off, _ = sc.reference(kind, dt, name, "not_inf", 0.5, p_max)
        k = min(n, p_max)
        assert off.tobytes() == full[2].tobytes()  # the offsets are the true ones
        assert p[:k].tobytes() == full[0][:k].tobytes() and x[:k].tobytes() == full[1][:k].tobytes() and not p[k:].any() and (x[k:] == -1).all()
    px = full[1][int(full[2][2]):int(full[2][3])].astype(np.int64)  # image 2, valid region 17 x 64: pixel counts rows by the allocated width
    assert (px % sc.W < 64).all() and (px // sc.W).max() == 16 and (np.diff(px) > 0).all()


# ---- the host helpers
def test_scene_tree_is_the_maximum_spanning_forest_with_fixed_ties():
    from mdrp_amd import scene
    pairs = [(0, 1), (1, 2), (0, 2), (3, 4), (2, 2), (1, 9), (4, 3)]
    tree = scene.scene_tree(pairs, [5, 5, 9, 1, 100, 50, 1], 6)
    # pair 2 (weight 9), then pair 0 before pair 1 (a tie: the lower index), which closes a cycle; pairs 4 and 5 are not edges; pair 3 before pair 6
    assert tree.tolist() == [[0, RT], [0, E], [2, E], [3, RT], [3, E], [-1, RT]] and tree.dtype == np.int32
    assert scene.scene_tree(pairs, [5, 5, 9, 1, 100, 50, 1], 6, roots=[2, 4]).tolist() == [[2, E], [0, E], [2, RT], [3, E], [3, RT], [-1, RT]]
    assert scene.scene_tree(pairs, [5, 6, 9, 1, 100, np.nan, 1], 6).tolist()[1] == [1, E]  # the heavier edge now
    with pytest.raises(ValueError):
        scene.scene_tree(pairs, [1, 2, 3, 4, 5, 6, 7], 6, roots=[0, 2])
    with pytest.raises(ValueError):
        scene.scene_tree(pairs, [1, 2], 6)
    # whatever it returns chains: every image of a connected set is attached, with the depth of its path
    w = _world("varying_focal")
    prs = np.array([(0, 1), (2, 1), (2, 3), (4, 3), (5, 4), (0, 5), (1, 4)])
    tr = scene.scene_tree(prs, [3, 1, 4, 1, 5, 9, 2], 6)
    T = frontend.scene_transforms_numpy(np.array([w["model"](a, c) for a, c in prs]), "varying_focal", prs, tr, 6)
    assert (T["root"] == 0).all() and T["depth"][0] == 0 and (T["depth"][1:] >= 1).all()
    assert "host" in scene.scene_tree.__doc__.lower()


def test_video_tree():
    from mdrp_amd import scene
    pairs, tree = scene.video_tree(1)
    assert pairs.shape == (0, 2) and tree.tolist() == [[-1, RT]]
    pairs, tree = scene.video_tree(3)
    assert pairs.tolist() == [[1, 0], [2, 1]] and tree.tolist() == [[0, RT], [0, E], [1, E]] and pairs.dtype == tree.dtype == np.int32
    with pytest.raises(ValueError):
        scene.video_tree(0)


def test_the_entry_points_are_poselibs():
    import mdrp_amd.poselib as poselib
    from mdrp_amd import scene
    for name in ("scene_transforms_torch", "reconstruct_scene_torch", "reconstruct_scene", "scene_tree", "video_tree"):
        assert getattr(poselib, name) is getattr(scene, name)
    with pytest.raises(ValueError):
        poselib.reconstruct_scene_torch("relpose_5pt", None, None, None, None)
    with pytest.raises(ValueError):
        poselib.reconstruct_scene_torch("calibrated", None, np.zeros((1, 2, 2)), [], [])  # not a tensor on the GPU
    assert scene.TRANSFORM_DTYPE.itemsize == C.sizeof(_capi.SceneTransform) == 128


# ---- header, binding, build, library
def test_header_binding_and_build_agree(tmp_path):
    from mdrp_amd import build
    import __graft_entry__ as ge
    inc = os.path.join(ROOT, "include")
    main = open(os.path.join(inc, "mdrp.h")).read()
    assert int(re.search(r"#define MDRP_ABI_VERSION (0x[0-9a-fA-F]+)", main).group(1), 16) == 6 == _capi.ABI_VERSION
    assert main.rstrip().endswith("#endif") and '#include "mdrp_dense.h"' in main
    for other in sorted(os.listdir(inc)):  # no other header names the new identifiers
        if other != "mdrp_scene.h":
            text = open(os.path.join(inc, other)).read()
            for name in NAMES + ("mdrp_scene_transform", "MDRP_SCENE_ROOT"):
                assert not re.search(r"\b" + name + r"\b", text), (other, name)
    assert open(os.path.join(inc, "mdrp_reconstruct.h")).read().rstrip().endswith('one fused cloud per scene; it builds on the descriptors and rules above */\n#endif')
    assert '#include "mdrp_scene.h"' in open(os.path.join(inc, "mdrp_reconstruct.h")).read()  # mdrp.h reaches it through the dense and reconstruct headers
    path = os.path.join(inc, "mdrp_scene.h")
    hdr = open(path).read()
    for rule in ("S1.", "S2.", "S3.", "S4.", "S5.", "S6.", "128 bytes"):
        assert rule in hdr, rule
    deps = [os.path.realpath(d) for d in build.DEPS]
    assert os.path.realpath(path) in deps and os.path.realpath(os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_scene.h")) in deps
    assert sorted(_capi.EXPORTS_SCENE) == sorted(NAMES) == sorted(set(re.findall(r"\b(mdrp_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))))
    others = (set(_capi.EXPORTS) | set(_capi.EXPORTS_CLASSIC_RANKED) | set(_capi.EXPORTS_CLASSIC_MODELS) | set(_capi.EXPORTS_CLASSIC_FRONTEND)
              | set(_capi.EXPORTS_CLASSIC_FOCALS) | set(_capi.EXPORTS_DENSE) | set(_capi.EXPORTS_RECONSTRUCT))
    assert not set(_capi.EXPORTS_SCENE) & others
    assert "EXPORTS_SCENE" in open(ge.__file__).read()
    t = _capi.SceneTransform
    src = tmp_path / "layout.c"
    src.write_text('#include "mdrp.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n    printf("%zu ", sizeof(mdrp_scene_transform));\n'
                   + "".join(f'    printf("%zu ", offsetof(mdrp_scene_transform, {n}));\n' for n, _ in t._fields_)
                   + '    printf("%d %d %d", MDRP_SCENE_ABSENT, MDRP_SCENE_EDGE, MDRP_SCENE_ROOT);\n'
                   + "    return (mdrp_scene_transforms_async && mdrp_reconstruct_scene_async) ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-Wno-address", str(src), "-I", inc, "-o", str(tmp_path / "layout.o")], check=True)
    build.build()
    lib = _capi.load_library()
    subprocess.run(["gcc", str(tmp_path / "layout.o"), "-o", str(tmp_path / "layout"), build.OUT, "-Wl,--unresolved-symbols=ignore-in-shared-libs"], check=True)
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(build.OUT) + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    out = [int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, env=env).stdout.split()]
    want = [C.sizeof(t)] + [getattr(t, n).offset for n, _ in t._fields_]
    assert out == want + [_capi.SCENE_ABSENT, _capi.SCENE_EDGE, _capi.SCENE_ROOT] and want[0] == 128, (out, want)
    assert [frontend.SCENE_TRANSFORM_DTYPE.fields[n][1] for n, _ in t._fields_] == want[1:] and frontend.SCENE_TRANSFORM_DTYPE.names == tuple(n for n, _ in t._fields_)
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{(.*?)\} mdrp_scene_transform;", hdr, flags=re.S).group(1), flags=re.S)
    assert re.findall(r"\b(\w+)(?:\[\d+\])?;", body) == [n for n, _ in t._fields_]  # the fields in the header's order
    syms = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, n_args in zip(NAMES, (9, 13)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        args = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", syms), name
        assert len(getattr(lib, name).argtypes) == len(args) == n_args, name
    for method in ("scene_transforms_device", "reconstruct_scene_device"):
        assert callable(getattr(_capi.Handle, method))
        assert method not in vars(_capi.Handle)  # they sit in a base class: the binding's recorded per-method cases are Handle's own


def test_the_handle_methods_hand_their_arguments_on():
    """the two handle methods against a recording stand-in for the library: the symbol, the argument order, the cameras as a host table"""
    calls = []

    class Lib:
        def __getattr__(self, name):
            if not name.startswith("mdrp_"):
                raise AttributeError(name)
            return lambda *a: calls.append((name, a)) or 0

    h = _capi.Handle.__new__(_capi.Handle)
    h._lib, h._h = Lib(), C.c_void_p(0x1000)
    try:
        cams = sc.rc.cameras(3)[0]
        opt, desc = _capi.ReconstructOpt(1, 77, 5, 9, 0), _capi.DepthImagePairs()
        h.scene_transforms_device(_capi.SHARED_FOCAL, 2, 0x2000, 136, 0x2100, 3, 0x2200, 0x2300)
        h.reconstruct_scene_device(_capi.CALIB, desc, opt, 2, 0x2000, 96, 0x2200, 0x3000, 0x4000, 0x5000, cams, 0x2300)
        h.reconstruct_scene_device(_capi.VARYING_FOCAL, desc, opt, 2, 0x2000, 96, 0x2200, 0x3000, 0x4000, 0x5000)
        with pytest.raises(ValueError):
            h.reconstruct_scene_device(_capi.SHARED_FOCAL, _capi.DepthPairs(), opt, 2, 0x2000, 96, 0x2200, 0x3000, 0x4000, 0x5000)
    finally:
        h._h = None
    (n1, a1), (n2, a2), (n3, a3) = calls
    assert n1 == "mdrp_scene_transforms_async" and len(a1) == 9
    assert a1[1:3] == (_capi.SHARED_FOCAL, 2) and a1[3].value == 0x2000 and a1[4] == 136 and a1[5].value == 0x2100 and a1[6] == 3
    assert [p.value for p in a1[7:]] == [0x2200, 0x2300]
    assert n2 == n3 == "mdrp_reconstruct_scene_async" and len(a2) == len(a3) == 13
    assert a2[1] == _capi.CALIB and a2[4] == 2 and a2[5].value == 0x2000 and a2[6] == 96 and a2[7].value == 0x2200
    assert a2[8] is not None and a2[9].value == 0x2300 and [p.value for p in a2[10:]] == [0x3000, 0x4000, 0x5000]
    assert a3[8] is None and a3[9] is None


# ---- the host build of the kernels' arithmetic (tests/hostmath/scene_host.cpp) against the definition
@pytest.fixture(scope="module")
def sh():
    here = os.path.join(ROOT, "tests", "hostmath")
    src, so = os.path.join(here, "scene_host.cpp"), os.path.join(here, "libscene_host.so")
    deps = [src] + [os.path.join(ROOT, "mdrp_amd", "csrc", n) for n in ("mdrp_scene.h", "mdrp_reconstruct.h", "mdrp_dense.h", "mdrp_frontend.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", src, "-o", so])
    lib = C.CDLL(so)
    lib.sh_seed.restype = C.c_uint32
    lib.sh_seed.argtypes = [C.c_uint32, C.c_uint32]
    lib.sh_points.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_host_limits_and_seed(sh):
    limits = (C.c_int * 6)()
    sh.sh_limits(limits)
    assert list(limits) == [_capi.SCENE_ABSENT, _capi.SCENE_EDGE, _capi.SCENE_ROOT, frontend.SCENE_STAGE, 128, 48]
    for seed in (0, 1, 0xFFFFFFFF, sc.SEED & 0xFFFFFFFF):
        for image in (0, 1, 45, 9999, 0x7FFFFFFF):
            assert sh.sh_seed(seed, image) == frontend.scene_seed(seed, image)


@pytest.mark.parametrize("kind_id, kind", list(enumerate(sc.KINDS)))
@pytest.mark.parametrize("name", sorted(sc.TREES))
def test_host_transforms_equal_the_definition_as_bytes(sh, kind_id, kind, name):
    """S1 and S2 over every tree case (the depth-8 chain of mixed directions among them), with models as an array and inside result records"""
    x = sc.inputs(kind, "float32", name)
    want = sc.transforms(kind, name)
    for stride in (96, 136):
        rec = np.zeros(len(x["pairs"]), dtype=_capi.RESULT_DTYPE if stride == 136 else _capi.MODEL_DTYPE)
        (rec["model"] if stride == 136 else rec)[...] = x["models"]
        out = np.zeros(x["I"], dtype=frontend.SCENE_TRANSFORM_DTYPE)
        sh.sh_transforms(kind_id, len(rec), _p(rec), stride, _p(x["pairs"]), x["I"], _p(x["tree"]), _p(out))
        assert out.tobytes() == want.tobytes(), (kind, name, stride)
    if name == "chain":
        assert want["depth"].max() == 8


@pytest.mark.parametrize("kind_id, kind", list(enumerate(sc.KINDS)))
def test_host_points_equal_the_definition_as_bytes(sh, kind_id, kind):
    """the image's record, its intrinsics and the point of every kept pixel, rounded: the bytes of the definition's rows, root and chained images"""
    for dtype_name in ("float32", "float64"):
        x = sc.inputs(kind, dtype_name, "chain")
        T = sc.transforms(kind, "chain")
        rows = sc.rows(kind, dtype_name, "chain", "not_inf", 1.0)
        for i in (0, 2, 5, 8):
            pixel = rows[i][1].astype(np.int64)
            v, u = (pixel // sc.W).astype(np.uint32), (pixel % sc.W).astype(np.uint32)
            d = np.ascontiguousarray(x["dm"][i][v, u].astype(np.float64))
            cam = x["cams"][i] if x["cams"] is not None else None
            out = np.zeros((len(pixel), 3), dtype=np.float32)
            sh.sh_points(_p(T[i:i + 1]), kind_id, 0 if cam is None else int(cam["model_id"]), None if cam is None else _p(np.ascontiguousarray(cam["params"])),
                         x["centers"][i][0], x["centers"][i][1], len(pixel), _p(v), _p(u), _p(d), _p(out))
            assert len(pixel) > 500 and out.tobytes() == rows[i][0].tobytes(), (dtype_name, i)
