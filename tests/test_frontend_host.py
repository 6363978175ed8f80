"""The device front end without a GPU: the per-row rules of mdrp_amd/csrc/mdrp_frontend.h (host build) against their NumPy statement
(mdrp_amd/frontend.py), that statement against a literal transcription of the indexing rule, the ctypes descriptor against the header,
and the register budget of the new kernels in the built library."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from mdrp_amd import _capi, frontend

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "hostmath", "libfrontend_host.so")
W, H = 64, 48


@pytest.fixture(scope="module")
def fh():
    src = os.path.join(HERE, "hostmath", "frontend_host.cpp")
    hdr = os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_frontend.h")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", src, "-o", SO])
    return C.CDLL(SO)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_pixel(fh, x, y, w, h):
    n = len(x)
    inside, xi, yi = (np.zeros(n, dtype=np.int32) for _ in range(3))
    fn = fh.fh_pixel_f32 if x.dtype == np.float32 else fh.fh_pixel_f64
    fn(_p(x), _p(y), n, w, h, _p(inside), _p(xi), _p(yi))
    return inside.astype(bool), xi, yi


def _edge_coordinates(dtype, size):
    """the coordinates the definition names and the representable values next to them, for a map side of `size`"""
    one = np.array([-0.5, -1.0, size - 0.001, size, np.nan, np.inf, -np.inf, 0.0, -0.0, 0.999, 1.0, size - 1, size - 0.5, -0.999,
                    1e30, -1e30, 2.0 ** 31, -2.0 ** 31, 2.0 ** 40], dtype=dtype)
    near = np.array([-1.0, float(size), 0.0, 1.0], dtype=dtype)
    return np.concatenate([one, np.nextafter(near, dtype(np.inf)), np.nextafter(near, dtype(-np.inf))]).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pixel_rule_equals_numpy_statement(fh, dtype):
    ex, ey = _edge_coordinates(dtype, W), _edge_coordinates(dtype, H)
    x = np.repeat(ex, len(ey)); y = np.tile(ey, len(ex))  # every edge x with every edge y
    rng = np.random.default_rng(7)
    x = np.concatenate([x, rng.uniform(-3.0, W + 3.0, 10000).astype(dtype)])
    y = np.concatenate([y, rng.uniform(-3.0, H + 3.0, 10000).astype(dtype)])
    x, y = np.ascontiguousarray(x, dtype=dtype), np.ascontiguousarray(y, dtype=dtype)
    inside, xi, yi = _host_pixel(fh, x, y, W, H)
    ref_in, ref_xi, ref_yi = frontend.pixel_index(x, y, W, H)
    assert np.array_equal(inside, ref_in) and np.array_equal(xi, ref_xi) and np.array_equal(yi, ref_yi)
    assert 0.2 < inside.mean() < 0.95  # both outcomes are exercised
    assert (xi[inside] >= 0).all() and (xi[inside] < W).all() and (yi[inside] >= 0).all() and (yi[inside] < H).all()
    # the cases the definition spells out, on x with y = 0
    cases = {-0.5: (True, 0), -1.0: (False, 0), W - 0.001: (True, W - 1), float(W): (False, 0), np.nan: (False, 0), np.inf: (False, 0), -np.inf: (False, 0)}
    cx = np.array(list(cases), dtype=dtype)
    inside, xi, _ = _host_pixel(fh, cx, np.zeros(len(cx), dtype=dtype), W, H)
    assert [(bool(a), int(b)) for a, b in zip(inside, xi)] == list(cases.values())


def test_keep_rule_equals_numpy_statement(fh):
    assert fh.fh_filter_both_inf() == _capi.FILTERS["both_inf"] == 0 and fh.fh_filter_finite() == _capi.FILTERS["finite"] == 1
    special = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1.5, -2.0, 5e-324, 1.7976931348623157e308])
    rng = np.random.default_rng(8)
    d1 = np.concatenate([np.repeat(special, len(special)), rng.choice(special, 10000), rng.normal(size=10000)])
    d2 = np.concatenate([np.tile(special, len(special)), rng.choice(special, 10000), rng.choice(special, 10000)])
    for name, code in _capi.FILTERS.items():
        keep = np.zeros(len(d1), dtype=np.int32)
        fh.fh_keep(_p(d1), _p(d2), len(d1), code, _p(keep))
        assert np.array_equal(keep.astype(bool), frontend.keep_depths(d1, d2, name)), name
    keep = np.zeros(4, dtype=np.int32)  # the scripts' rule: only inf & inf goes; the README's: anything not finite goes
    a, b = np.array([np.inf, np.inf, np.nan, 1.0]), np.array([-np.inf, 2.0, np.nan, 2.0])
    fh.fh_keep(_p(a), _p(b), 4, 0, _p(keep)); assert keep.tolist() == [0, 1, 1, 1]
    fh.fh_keep(_p(a), _p(b), 4, 1, _p(keep)); assert keep.tolist() == [0, 0, 0, 1]


def test_row_validity_equals_numpy_statement(fh):
    K1, K2 = 5, 7
    i = np.array([-1, 0, 4, 5, 0, 3, -2, 2 ** 31 - 1, -2 ** 31], dtype=np.int32)
    j = np.array([0, -1, 6, 0, 7, 3, -2, 0, 0], dtype=np.int32)
    ok = np.zeros(len(i), dtype=np.int32)
    fh.fh_row_valid(_p(i), _p(j), len(i), K1, K2, _p(ok))
    assert ok.tolist() == [0, 0, 1, 0, 0, 1, 0, 0, 0]
    kp1, kp2 = np.full((K1, 2), 1.0), np.full((K2, 2), 1.0)
    slot = frontend.gather_matches_numpy(kp1, kp2, np.stack([i, j], 1), np.ones((4, 4)), np.ones((4, 4)))[4]
    assert np.array_equal(slot >= 0, ok.astype(bool))


@pytest.mark.parametrize("kp_dtype,depth_dtype", [(np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64)])
def test_numpy_statement_equals_the_indexing_rule_transcribed(kp_dtype, depth_dtype):
    """in range, non-negative, "both_inf": fancy-index the keypoints, index the maps at astype(int), mask out inf & inf — kept set, order, values"""
    rng = np.random.default_rng(9)
    K1, K2, M = 300, 280, 700
    kp1 = np.stack([rng.uniform(0, W, K1), rng.uniform(0, H, K1)], 1).astype(kp_dtype)
    kp2 = np.stack([rng.uniform(0, 72, K2), rng.uniform(0, 40, K2)], 1).astype(kp_dtype)
    kp1 = np.minimum(kp1, np.nextafter(np.array([W, H], dtype=kp_dtype), kp_dtype(0)))  # a float32 rounding up to W would leave the range
    kp2 = np.minimum(kp2, np.nextafter(np.array([72, 40], dtype=kp_dtype), kp_dtype(0)))
    matches = np.stack([rng.integers(0, K1, M), rng.integers(0, K2, M)], 1)
    dm1 = rng.uniform(1, 5, (H, W)).astype(depth_dtype); dm2 = rng.uniform(1, 5, (40, 72)).astype(depth_dtype)
    dm1[rng.random((H, W)) < 0.3] = np.inf; dm2[rng.random((40, 72)) < 0.3] = np.inf
    dm1[rng.random((H, W)) < 0.05] = np.nan; dm2[rng.random((40, 72)) < 0.05] = -np.inf
    # the transcription
    points1 = kp1[matches[:, 0]]; points2 = kp2[matches[:, 1]]
    depths1 = dm1[points1[:, 1].astype(int), points1[:, 0].astype(int)]
    depths2 = dm2[points2[:, 1].astype(int), points2[:, 0].astype(int)]
    sel = ~np.logical_and(np.isinf(depths1), np.isinf(depths2))
    x1, x2, d1, d2, slot = frontend.gather_matches_numpy(kp1, kp2, matches, dm1, dm2)
    assert 0 < sel.sum() < M and np.isnan(d1).any() and (np.isinf(d1) ^ np.isinf(d2)).any()
    assert np.array_equal(slot >= 0, sel) and np.array_equal(slot[sel], np.arange(sel.sum()))
    for mine, ref in ((x1, points1[sel]), (x2, points2[sel]), (d1, depths1[sel]), (d2, depths2[sel])):
        assert mine.dtype == np.float64 and mine.tobytes() == ref.astype(np.float64).tobytes()


def test_numpy_statement_centres_and_padding():
    kp = np.array([[1.25, 2.5], [3.0, 4.0]], dtype=np.float32)
    dm = np.arange(48, dtype=np.float64).reshape(6, 8)
    matches = np.array([[1, 0], [-1, -1], [0, 1]])
    x1, x2, d1, d2, slot = frontend.gather_matches_numpy(kp, kp, matches, dm, dm, center1=[0.5, 0.25], center2=[1.0, 1.0], filter="finite")
    assert slot.tolist() == [0, -1, 1] and slot.dtype == np.int32
    assert x1.tolist() == [[2.5, 3.75], [0.75, 2.25]] and x2.tolist() == [[0.25, 1.5], [2.0, 3.0]]
    assert d1.tolist() == [dm[4, 3], dm[2, 1]] and d2.tolist() == [dm[2, 1], dm[4, 3]]
    px1, px2, pd1, pd2, n, ps = frontend.pad_pairs([(x1, x2, d1, d2, slot)], 4)
    assert n.tolist() == [2] and ps.tolist() == [[0, -1, 1, -1]] and px1[0, 2:].tolist() == [[0, 0], [0, 0]] and pd2[0, 2:].tolist() == [1, 1]
    with pytest.raises(ValueError):
        frontend.gather_matches_numpy(kp, kp, matches, dm, dm, filter="nonsense")
    with pytest.raises(ValueError):
        frontend.gather_matches_numpy(kp.astype(np.float16), kp, matches, dm, dm)


def test_descriptor_layout_matches_header(tmp_path):
    """sizeof and every field offset of the ctypes mdrp_matches against the header, through a C compiler"""
    names = [f for f, _ in _capi.Matches._fields_]
    hdr = open(os.path.join(ROOT, "include", "mdrp.h")).read()
    body = hdr[hdr.index("typedef struct {", hdr.index("enum { MDRP_FILTER_BOTH_INF")):hdr.index("} mdrp_matches;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in re.findall(r"[\w ]+?((?:\*?\w+\s*,\s*)*\*?\w+)\s*;", body) for n in re.findall(r"\w+", decl)]
    assert declared == names, declared
    src = tmp_path / "layout.c"
    src.write_text('#include "mdrp.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n    printf("%zu", sizeof(mdrp_matches));\n'
                   + "".join(f'    printf(" %zu", offsetof(mdrp_matches, {n}));\n' for n in names) + '    printf(" %d %d", MDRP_F32, MDRP_F64);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_capi.Matches)
    assert out[1:1 + len(names)] == [getattr(_capi.Matches, n).offset for n in names]
    assert out[-2:] == [_capi.F32, _capi.F64]


def test_abi_version_is_bumped_in_header_and_binding_together():
    hdr = open(os.path.join(ROOT, "include", "mdrp.h")).read()
    assert int(re.search(r"#define MDRP_ABI_VERSION (0x[0-9a-fA-F]+)", hdr).group(1), 16) == _capi.ABI_VERSION == 0x00000006
    assert {"mdrp_gather_matches", "mdrp_estimate_matches_async"} <= set(_capi.EXPORTS)


def test_front_end_kernels_are_built_and_use_no_scratch():
    from mdrp_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    build.build()
    regs = kernel_table.kernel_table()
    want = [f"mdrp::k_gather<{k}, {d}>" for k in ("float", "double") for d in ("float", "double")] + ["mdrp::k_match_mask"]
    for name in want:
        assert name in regs, (name, sorted(k for k in regs if "gather" in k or "match" in k))
        r = regs[name]
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (name, r)
    assert sum(1 for k in regs if k.startswith("mdrp::k_gather<")) == 4
