"""The varying-focal baseline's tail without a GPU (include/mdrp_classic_focals.h): the host build of
mdrp_amd/csrc/mdrp_classic_focals.h (tests/hostmath/focals_host.cpp) against the reference binary's focals (tests/golden/classic_focals_ref.npz) and
against the NumPy yardstick (tests/classic_focals_ref.py); the extension header against the binding, the build and the library; the record's layout;
the Python entry points' argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import classic_focals_cases as fc
import classic_focals_ref as fr
from mdrp_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostmath", "focals_host.cpp")
HDR = os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_classic_focals.h")
MATH = os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_classic_math.h")
SO = os.path.join(HERE, "hostmath", "libfocals_host.so")
NAMES = ("mdrp_focals_from_fundamental", "mdrp_pose_from_fundamental", "mdrp_pose_from_fundamental_async", "mdrp_estimate_fundamental_focals_async")


@pytest.fixture(scope="module")
def fh():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in (SRC, HDR, MATH)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", SRC, "-o", SO])
    return C.CDLL(SO)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def check_focals(got, fx):
    """focals [count][2] against the fixture: NaN positions exactly, the real ones within the fixture's tolerance (10 x the largest deviation of the
    NumPy restatement from the binary, measured by tests/tools/gen_golden_classic_focals.py)"""
    ref = fx["f"]
    tol = float(fx["tolerance"])
    assert tol == 10.0 * float(fx["measured_max_rel"]) and tol < 1e-8
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    real = ~np.isnan(ref)
    rel = np.abs(got[real] - ref[real]) / np.abs(ref[real])
    print("largest relative deviation from the binary %.3g (allowed %.3g)" % (rel.max(), tol))
    assert rel.max() <= tol


def test_the_fixture_is_what_the_issue_asks_for():
    fx = fc.fixture()
    assert 350 <= len(fx["F"]) <= 450 and fx["f"].shape == (len(fx["F"]), 2)
    assert np.isnan(fx["f"]).sum() >= 10 and (fx["pp1"] == 0).all(axis=1).any() and (fx["pp1"] != 0).any()
    assert np.abs(np.linalg.det(fx["F"].reshape(-1, 3, 3))).max() < 1e-12  # rank 2, unit norm


def test_the_numpy_restatement_reproduces_the_binary():
    fx = fc.fixture()
    check_focals(np.array([fr.focals(fx["F"][i], fx["pp1"][i], fx["pp2"][i]) for i in range(len(fx["F"]))]), fx)


def test_the_headers_focals_reproduce_the_binary(fh):
    fx = fc.fixture()
    F, a, b = (np.ascontiguousarray(fx[k]) for k in ("F", "pp1", "pp2"))
    got = np.full((len(F), 2), -7.0)
    fh.fh_focals(_p(F), _p(a), _p(b), len(F), _p(got))
    check_focals(got, fx)
    zero = (a == 0).all(axis=1) & (b == 0).all(axis=1)  # a NULL principal point is the origin
    F0 = np.ascontiguousarray(F[zero])
    got0 = np.full((len(F0), 2), -7.0)
    fh.fh_focals(_p(F0), None, None, len(F0), _p(got0))
    assert zero.sum() > 50 and got0.tobytes() == got[zero].tobytes()


def _host_records(fh, c, with_mask):
    B, n_max = c["x1"].shape[:2]
    out = np.zeros(B, dtype=_capi.FOCAL_POSE_DTYPE)
    cand = np.zeros((B, 4, 12))
    for i in range(B):
        x1, x2, F = np.ascontiguousarray(c["x1"][i]), np.ascontiguousarray(c["x2"][i]), np.ascontiguousarray(_capi.model_to_fundamental(c["models"][i]))
        mask = np.ascontiguousarray(c["mask"][i]) if with_mask else None
        rec = np.zeros(1, dtype=_capi.FOCAL_POSE_DTYPE)
        fh.fh_pose(_p(x1), _p(x2), n_max, int(c["n"][i]), _p(F), _p(mask), _p(np.ascontiguousarray(c["pp1"][i])), _p(np.ascontiguousarray(c["pp2"][i])),
                   _p(rec), _p(cand[i]))
        out[i] = rec[0]
    return out, cand


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("with_mask", [True, False])
def test_the_headers_records_equal_the_yardsticks(fh, which, with_mask):
    """candidates, votes, voters, winner and status of every pair of the vote batches: integers equal, q up to sign and t to 1e-12"""
    fc.assert_margins(which, with_mask)
    c = fc.batch(which)
    got, cand = _host_records(fh, c, with_mask)
    want = fc.expected(which, with_mask)
    for i, name in enumerate(c["names"]):
        fc.check_record(got[i], want[i], (which, with_mask, name))
        if want[i]["cand"] is not None:
            for k in range(4):
                q, wq = cand[i, k, :4], want[i]["cand"][k, :4]
                assert min(np.abs(q - wq).max(), np.abs(q + wq).max()) <= 1e-12 and np.abs(cand[i, k, 4:7] - want[i]["cand"][k, 4:7]).max() <= 1e-12, (name, k)
            # the order of orc_motion_from_essential: (R1, t), (R1, -t), (R2, -t), (R2, t)
            assert np.array_equal(cand[i, 0, :4], cand[i, 1, :4]) and np.array_equal(cand[i, 2, :4], cand[i, 3, :4])
            assert np.array_equal(cand[i, 0, 4:7], -cand[i, 1, 4:7]) and np.array_equal(cand[i, 1, 4:7], cand[i, 2, 4:7]) and np.array_equal(cand[i, 0, 4:7], cand[i, 3, 4:7])
    by = dict(zip(c["names"], got))
    if which == 0:
        assert by["nan_F"]["status"] == _capi.FOCAL_NO_MODEL and np.isnan(by["nan_F"]["model"]["f1"]) and np.isnan(by["nan_F"]["model"]["f2"])
        assert by["zero_mask"]["status"] == (_capi.FOCAL_NO_VOTERS if with_mask else 0) and by["zero_mask"]["winner"] == (0 if with_mask else by["zero_mask"]["winner"])
    else:
        assert by["n5"]["status"] == _capi.FOCAL_NO_MODEL and by["n5"]["winner"] == -1
        assert by["negative_f"]["status"] in (2, 4, 6) and by["negative_f"]["winner"] == -1 and not by["negative_f"]["votes"].any()
    for name in ("n7", "n64", "n255") if which == 0 else ("n256", "n257", "n600"):  # the winner is the true pose: every inlier among the voters votes for it
        r = by[name]                                                                 # (some 70 % of the records are inliers, some 95 % of the masked ones)
        assert r["status"] == 0 and r["votes"][r["winner"]] >= (0.8 if with_mask else 0.5) * r["voters"] > 0, name


def test_the_host_program_stands_alone_under_the_sanitizers(tmp_path):
    """the same source with its own main, built with -fsanitize=address,undefined: tables of their exact size, rows past n that must not be read"""
    exe = tmp_path / "focals_host_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DFOCALS_HOST_MAIN", SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "focals_host: ok" in r.stdout, (r.stdout, r.stderr)


# ---- header, binding, build, library
def _declaration(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, name
    return [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]


def test_header_binding_and_build_agree(tmp_path):
    """four new symbols within ABI 6, declared in a fourth extension header that mdrp.h includes last; the export list is the header's, disjoint from
    the others; both headers are build dependencies; a C host that includes mdrp.h alone links against the built library"""
    from mdrp_amd import build
    import __graft_entry__ as ge
    main = open(os.path.join(ROOT, "include", "mdrp.h")).read()
    assert int(re.search(r"#define MDRP_ABI_VERSION (0x[0-9a-fA-F]+)", main).group(1), 16) == 6 == _capi.ABI_VERSION
    assert main.index('#include "mdrp_classic_frontend.h"') < main.index('#include "mdrp_classic_focals.h"')
    for name in NAMES + ("mdrp_focal_pose",):
        assert not re.search(r"\b" + name + r"\b", main), name
    path = os.path.join(ROOT, "include", "mdrp_classic_focals.h")
    hdr = open(path).read()
    deps = [os.path.realpath(d) for d in build.DEPS]
    assert os.path.realpath(path) in deps and os.path.realpath(HDR) in deps
    assert sorted(_capi.EXPORTS_CLASSIC_FOCALS) == sorted(NAMES) == sorted(set(re.findall(r"\b(mdrp_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))))
    others = set(_capi.EXPORTS) | set(_capi.EXPORTS_CLASSIC_RANKED) | set(_capi.EXPORTS_CLASSIC_MODELS) | set(_capi.EXPORTS_CLASSIC_FRONTEND)
    assert not set(_capi.EXPORTS_CLASSIC_FOCALS) & others
    assert "EXPORTS_CLASSIC_FOCALS" in open(ge.__file__).read()
    src = tmp_path / "abi.c"
    src.write_text('#include "mdrp.h"\nint main(void) { return (mdrp_focals_from_fundamental && mdrp_pose_from_fundamental && mdrp_pose_from_fundamental_async '
                   '&& mdrp_estimate_fundamental_focals_async && sizeof(mdrp_focal_pose) == 128 && MDRP_FOCAL_NO_VOTERS == 8) ? 0 : 1; }\n')
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-Wno-address", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "abi.o")], check=True)
    build.build()
    lib = _capi.load_library()
    subprocess.run(["gcc", str(tmp_path / "abi.o"), "-o", str(tmp_path / "abi"), build.OUT, "-Wl,--unresolved-symbols=ignore-in-shared-libs"], check=True)
    syms = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, count in zip(NAMES, (7, 13, 12, 12)):
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", syms), name
        assert len(getattr(lib, name).argtypes) == len(_declaration(hdr, name)) == count, name
    for method in ("focals_from_fundamental", "pose_from_fundamental", "pose_from_fundamental_device", "estimate_fundamental_focals_device"):
        assert callable(getattr(_capi.Handle, method))


def test_record_layout(fh, tmp_path):
    """128 bytes; model | votes[4] | voters | winner | status | pad_ at the same offsets in the public header, the kernels' struct and the binding"""
    names = ["model", "votes", "voters", "winner", "status", "pad_"]
    src = tmp_path / "layout.c"
    src.write_text('#include "mdrp.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n    printf("%zu", sizeof(mdrp_focal_pose));\n'
                   + "".join(f'    printf(" %zu", offsetof(mdrp_focal_pose, {n}));\n' for n in names) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [128, 0, 96, 112, 116, 120, 124]
    d = _capi.FOCAL_POSE_DTYPE
    assert d.itemsize == 128 and [d.fields[n][1] for n in names] == out[1:] and list(d.names) == names
    o = (C.c_int * 5)()
    fh.fh_record_offsets(o)
    assert fh.fh_record_bytes() == 128 and list(o) == out[2:]
    assert (_capi.FOCAL_NO_MODEL, _capi.FOCAL_F1_NOT_REAL, _capi.FOCAL_F2_NOT_REAL, _capi.FOCAL_NO_VOTERS) == (1, 2, 4, 8)
    assert (fr.NO_MODEL, fr.F1_NOT_REAL, fr.F2_NOT_REAL, fr.NO_VOTERS) == (1, 2, 4, 8)


# ---- the Python entry points check their arguments before anything touches the device (there is none here)
def test_python_argument_checks():
    import torch
    from mdrp_amd import poselib
    F = np.eye(3)
    for bad in (np.eye(4), np.zeros(9), [[1, 2], [3, 4]]):
        with pytest.raises(ValueError, match="F"):
            poselib.focals_from_fundamental(bad, [0, 0], [0, 0])
    for pp1, pp2 in ((None, [0, 0]), ([0, 0], None), ([0, 0, 0], [0, 0]), ([0, 0], [1])):
        with pytest.raises(ValueError, match="pp"):
            poselib.focals_from_fundamental(F, pp1, pp2)
    with pytest.raises(ValueError, match="F"):
        poselib.focals_from_fundamental_batch(np.zeros((2, 9)))
    with pytest.raises(ValueError, match="F"):
        poselib.focals_from_fundamental_batch(np.zeros((2, 3, 3), dtype=object))
    with pytest.raises(ValueError, match="pp1"):
        poselib.focals_from_fundamental_batch(np.zeros((2, 3, 3)), pp1=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="pp2"):
        poselib.focals_from_fundamental_batch(np.zeros((2, 3, 3)), pp2=[np.nan, 0.0])
    pts = [np.zeros((9, 2)), np.zeros((8, 2))]
    with pytest.raises(ValueError, match="pp1"):
        poselib.estimate_varying_focal_relative_pose_batch(pts, pts, pp1=np.zeros((5, 2)))
    with pytest.raises(ValueError, match="pp2"):
        poselib.estimate_varying_focal_relative_pose_batch(pts, pts, pp2=[1.0, 2.0, 3.0])
    with pytest.raises(NotImplementedError, match="real_focal_check"):
        poselib.estimate_varying_focal_relative_pose_batch(pts, pts, ransac_opt={"real_focal_check": True})
    with pytest.raises(NotImplementedError, match="progressive_sampling"):
        poselib.estimate_varying_focal_relative_pose(pts[0], pts[0], ransac_opt={"progressive_sampling": True})
    with pytest.raises(ValueError):
        poselib.estimate_varying_focal_relative_pose_batch(pts, pts, scores=[np.zeros(9), np.zeros(8)], priors=[np.eye(3), np.eye(3)])
    t = torch.zeros((2, 9, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match="GPU"):
        poselib.pose_from_fundamental_batch_torch(t, t, np.zeros(2, dtype=_capi.MODEL_DTYPE))
    with pytest.raises(ValueError, match="GPU"):
        poselib.pose_from_fundamental_batch_torch(np.zeros((2, 9, 2)), np.zeros((2, 9, 2)), np.zeros(2, dtype=_capi.MODEL_DTYPE))
    with pytest.raises(ValueError, match="GPU"):
        poselib.estimate_varying_focal_baseline_batch_torch(t, t)
    with pytest.raises(ValueError, match="shapes"):
        poselib.estimate_varying_focal_baseline_batch_torch(t, torch.zeros((2, 8, 2), dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="real_focal_check"):
        poselib.estimate_varying_focal_baseline_batch_torch(t, t, ransac_opt={"real_focal_check": True})


def test_evalio_has_the_seven_point_row(monkeypatch):
    """evaluate_focal(shared=False) sends a `7p` experiment to estimate_varying_focal_relative_pose_batch with the core RANSAC keys only and writes
    the varying-focal record (pose error and f_err); _map_fork_options keeps refusing the fork's switch"""
    import json
    from mdrp_amd import evalio, poselib
    with pytest.raises(NotImplementedError):
        poselib._map_fork_options({"use_fundamental": True}, _capi.VARYING_FOCAL)
    rng = np.random.default_rng(5)
    x1, x2, F, a, b, truth, _ = fc.scene(rng, 30, pp_zero=True, outliers=0.0)
    K1, K2 = np.diag([truth["f1"], truth["f1"], 1.0]), np.diag([truth["f2"], truth["f2"], 1.0])
    h5 = {"pose_a_b": np.c_[truth["R"], truth["t"]], "K_a": K1, "K_b": K2, "corr_a_b": np.c_[x1, x2]}
    seen = {}

    def fake(p1, p2, pp1, pp2, ro, bo, device=0):
        seen.update(ro=dict(ro), pp=(pp1, pp2), n=len(p1[0]))
        cam1, cam2 = poselib.Camera("SIMPLE_PINHOLE", [truth["f1"] * 1.1, 0.0, 0.0]), poselib.Camera("SIMPLE_PINHOLE", [truth["f2"], 0.0, 0.0])
        pair = poselib.ImagePair(poselib.CameraPose(), cam1, cam2)
        return [pair], [{"inlier_ratio": 1.0, "num_inliers": 30, "inliers": [True] * 30, "F": np.eye(3), "votes": [30, 0, 0, 0], "winner": 0, "status": 0}]
    monkeypatch.setattr(poselib, "estimate_varying_focal_relative_pose_batch", fake)
    monkeypatch.setattr(evalio, "list_pairs", lambda h5, first=None: [("a", "b")])
    res = evalio.evaluate_focal(h5, ["7p"], shared=False, iters=100)
    assert len(res) == 1 and seen["n"] == 30 and seen["pp"] == (None, None)
    assert set(seen["ro"]) <= set(evalio.CORE_RANSAC_KEYS) and seen["ro"]["max_iterations"] == 100 and "use_fundamental" not in seen["ro"]
    assert abs(res[0]["f1_err"] - 0.1) < 1e-9 and res[0]["f2_err"] == 0.0 and res[0]["info"]["winner"] == 0
    json.dumps(res)
    with pytest.raises(NotImplementedError, match="budgets"):
        evalio.evaluate_focal(h5, ["7p"], shared=False, iterations_list=[10, 20])


def test_new_kernels_are_built_and_use_no_scratch():
    """kc_focal_pose and kc_focals are in the built library with no scratch and no spills (profiles/classic_focals_kernel_table.txt has the line)"""
    import sys
    from mdrp_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    build.build()
    regs = kernel_table.kernel_table()
    for name in ("mdrp::kc_focal_pose", "mdrp::kc_focals"):
        assert name in regs, (name, sorted(k for k in regs if "focal" in k))
        r = regs[name]
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (name, r)
    table = open(os.path.join(ROOT, "profiles", "classic_focals_kernel_table.txt")).read()
    assert "mdrp::kc_focal_pose" in table and "mdrp::kc_focals" in table
