"""The dense front end without a GPU (include/mdrp_dense.h): the extension header against the binding, the build and the library; the
descriptor's layout; the host build of mdrp_amd/csrc/mdrp_dense.h's arithmetic (tests/hostmath/dense_host.cpp) against the pieces of the NumPy
definition (mdrp_amd/frontend.py); properties of the definition itself; the Python entry points' argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_cases as dc
from mdrp_amd import _capi, frontend

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostmath", "dense_host.cpp")
HDR = os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_dense.h")
FRONT = os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_frontend.h")
SO = os.path.join(HERE, "hostmath", "libdense_host.so")
NAMES = ("mdrp_sample_dense", "mdrp_estimate_dense_async")
FIELDS = ["warp", "warp_type", "rows", "certainty", "certainty_type", "coords", "depth1", "depth2", "depth_type", "h1", "w1", "h2", "w2", "filter",
          "center1", "center2", "n", "balanced", "expansion", "grid", "min_count", "ranked", "seed", "threshold", "rows_out", "score_out"]


@pytest.fixture(scope="module")
def dh():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in (SRC, HDR, FRONT)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", SRC, "-o", SO])
    return C.CDLL(SO)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- header, binding, build, library
def _declaration(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, name
    return [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]


def test_header_binding_and_build_agree(tmp_path):
    """two new symbols within ABI 6, declared in a fifth extension header that mdrp.h includes last and names nothing of; the export list is the
    header's, disjoint from the others and registered with the build check; both headers are build dependencies; a C host that includes mdrp.h alone
    links the two symbols against the built library"""
    from mdrp_amd import build
    import __graft_entry__ as ge
    main = open(os.path.join(ROOT, "include", "mdrp.h")).read()
    assert int(re.search(r"#define MDRP_ABI_VERSION (0x[0-9a-fA-F]+)", main).group(1), 16) == 6 == _capi.ABI_VERSION
    includes = re.findall(r'#include "(mdrp_\w+\.h)"', main)
    assert includes[-1] == "mdrp_dense.h" and includes.index("mdrp_classic_focals.h") == len(includes) - 2
    for name in NAMES + ("mdrp_dense_matches", "MDRP_DENSE_NORMALIZED"):
        assert not re.search(r"\b" + name + r"\b", main), name
    path = os.path.join(ROOT, "include", "mdrp_dense.h")
    hdr = open(path).read()
    deps = [os.path.realpath(d) for d in build.DEPS]
    assert os.path.realpath(path) in deps and os.path.realpath(HDR) in deps
    assert sorted(_capi.EXPORTS_DENSE) == sorted(NAMES) == sorted(set(re.findall(r"\b(mdrp_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))))
    others = (set(_capi.EXPORTS) | set(_capi.EXPORTS_CLASSIC_RANKED) | set(_capi.EXPORTS_CLASSIC_MODELS) | set(_capi.EXPORTS_CLASSIC_FRONTEND)
              | set(_capi.EXPORTS_CLASSIC_FOCALS))
    assert not set(_capi.EXPORTS_DENSE) & others
    assert "EXPORTS_DENSE" in open(ge.__file__).read()
    src = tmp_path / "abi.c"
    src.write_text('#include "mdrp.h"\nint main(void) { return (mdrp_sample_dense && mdrp_estimate_dense_async && sizeof(mdrp_dense_matches) == 144 '
                   '&& MDRP_DENSE_PIXEL == 1 && MDRP_DENSE_MAX_ROWS == 4194304) ? 0 : 1; }\n')
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-Wno-address", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "abi.o")], check=True)
    build.build()
    lib = _capi.load_library()
    subprocess.run(["gcc", str(tmp_path / "abi.o"), "-o", str(tmp_path / "abi"), build.OUT, "-Wl,--unresolved-symbols=ignore-in-shared-libs"], check=True)
    syms = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, count in zip(NAMES, (10, 10)):
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", syms), name
        assert len(getattr(lib, name).argtypes) == len(_declaration(hdr, name)) == count, name
    for method in ("sample_dense", "estimate_dense_device"):
        assert callable(getattr(_capi.Handle, method))


def test_descriptor_layout(dh, tmp_path):
    """sizeof and every field offset of mdrp_dense_matches through a C compiler against the ctypes structure; the fields in the header's order; the
    header's limits and enumerators against the kernels' and the binding's"""
    hdr = open(os.path.join(ROOT, "include", "mdrp_dense.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{(.*?)\} mdrp_dense_matches;", hdr, flags=re.S).group(1), flags=re.S)
    declared = [n for decl in re.findall(r"[\w ]+?((?:\*?\w+\s*,\s*)*\*?\w+)\s*;", body) for n in re.findall(r"\w+", decl)]
    assert declared == FIELDS == [f[0] for f in _capi.DenseMatches._fields_], declared
    src = tmp_path / "layout.c"
    src.write_text('#include "mdrp.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n    printf("%zu", sizeof(mdrp_dense_matches));\n'
                   + "".join(f'    printf(" %zu", offsetof(mdrp_dense_matches, {n}));\n' for n in FIELDS)
                   + '    printf(" %d %d %d %d %d %d", MDRP_DENSE_MAX_ROWS, MDRP_DENSE_MAX_STAGE1, MDRP_DENSE_MAX_N, MDRP_DENSE_MAX_GRID, MDRP_DENSE_NORMALIZED, '
                   "MDRP_DENSE_PIXEL);\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_capi.DenseMatches) == 144
    assert out[1:1 + len(FIELDS)] == [getattr(_capi.DenseMatches, n).offset for n in FIELDS]
    limits = (C.c_int * 6)()
    dh.dh_limits(limits)
    assert out[1 + len(FIELDS):] == list(limits) == [1 << 22, 65536, 16384, 8, 0, 1]
    assert (_capi.DENSE_MAX_ROWS, _capi.DENSE_MAX_STAGE1, _capi.DENSE_MAX_N, _capi.DENSE_MAX_GRID) == tuple(limits[:4])
    assert (frontend.DENSE_MAX_ROWS, frontend.DENSE_MAX_STAGE1, frontend.DENSE_MAX_N, frontend.DENSE_MAX_GRID) == tuple(limits[:4])
    assert _capi.DENSE_COORDS == {"normalized": 0, "pixel": 1} and tuple(_capi.DENSE_COORDS) == frontend.COORDS


# ---- the header's arithmetic against the definition's pieces, exactly
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pixel_coordinates_equal_the_definition(dh, dtype):
    """D1 at and around -1 and 1, NaN and +-inf, and on random values, for both coords and extents that are odd, even and 1"""
    rng = np.random.default_rng(1)
    around = [np.nextafter(dtype(c), dtype(t)) for c in (-1.0, 1.0) for t in (-2.0, 2.0)]
    with np.errstate(over="ignore"):
        v = np.concatenate([np.array(dc.SPECIAL_COORDS, dtype=np.float64).astype(dtype), np.array(around, dtype=dtype), rng.uniform(-1.1, 1.1, 500).astype(dtype),
                            rng.uniform(-5, 700, 200).astype(dtype)])
    fn = dh.dh_pixel_f32 if dtype == np.float32 else dh.dh_pixel_f64
    for extent in (1, 45, 61, 70, 640, 2 ** 31 - 1):
        for coords in frontend.COORDS:
            got = np.full(len(v), -7.0)
            fn(_p(v), len(v), extent, _capi.DENSE_COORDS[coords], _p(got))
            want = frontend.dense_pixel_coord(v, extent, coords)
            assert want.dtype == np.float64 and got.tobytes() == want.tobytes(), (extent, coords)
    # what the rule says at the borders: -1 is pixel coordinate 0, 1 is the extent itself (outside), the float32 just below 1 is inside; the float64
    # just below 1 is not: 2 - 2^-53 rounds to 2 in the sum, which is the rule as stated (the sum is made in float64, once)
    edge = frontend.dense_pixel_coord(np.array([-1.0, 1.0, float(np.nextafter(np.float32(1.0), np.float32(0.0))), np.nextafter(1.0, 0.0)]), 61, "normalized")
    assert edge[0] == 0.0 and edge[1] == 61.0 and 60.0 < edge[2] < 61.0 and edge[3] == 61.0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_weights_equal_the_definition(dh, dtype):
    """D3 on certainties 0, -0.0, negative, NaN, inf, denormal, just below / at / above the threshold, above 1, and on random values"""
    rng = np.random.default_rng(2)
    for threshold in (0.05, 0.0, 0.5, 2.0, float(np.float32(0.05))):
        near = [np.nextafter(dtype(threshold), dtype(t)) for t in (-1.0, 3.0)] + [dtype(threshold)]
        with np.errstate(over="ignore"):
            c = np.concatenate([np.array(dc.SPECIAL_CERTAINTIES, dtype=np.float64).astype(dtype), np.array(near, dtype=dtype),
                                rng.uniform(-0.1, 1.2, 2000).astype(dtype), (rng.uniform(0, 4, 500) / 65536.0).astype(dtype)])
        got = np.full(len(c), 7, dtype=np.uint32)
        (dh.dh_weight_f32 if dtype == np.float32 else dh.dh_weight_f64)(_p(c), len(c), C.c_double(threshold), _p(got))
        want = frontend.dense_weight(c, threshold)
        assert want.dtype == np.uint32 and np.array_equal(got, want), threshold
        assert got.max() == 65536 and ((got == 0) == ~(np.isfinite(c) & (c > 0))).all()
    q = frontend.dense_weight(np.array(dc.SPECIAL_CERTAINTIES), 0.05)  # in the order of the list, float64
    assert q.tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 3276, 3276, 65536, 65536, 65536, 65536, 1, 1, 2]


def test_hash_and_positions_equal_the_definition_at_the_limits(dh):
    """lowbias32, u_k and P_k for S at its maximum (R = 2^22 rows of weight 65536 = 2^38; stage 2: 65536 picks of weight 2^20 = 2^36), M = 65536 and
    every k, against NumPy and against Python's unbounded integers"""
    x = np.concatenate([np.array([0, 1, 2, 0x7fffffff, 0x80000000, 0xffffffff], dtype=np.uint32), np.random.default_rng(3).integers(0, 2 ** 32, 1000, dtype=np.uint32)])
    got = np.zeros_like(x)
    dh.dh_lowbias32(_p(x), len(x), _p(got))
    assert np.array_equal(got, frontend.lowbias32(x))

    def py_hash(v):
        v ^= v >> 16; v = v * 0x7feb352d & 0xffffffff
        v ^= v >> 15; v = v * 0x846ca68b & 0xffffffff
        return v ^ (v >> 16)
    assert [py_hash(int(v)) for v in x[:50]] == got[:50].tolist() and py_hash(0) == 0
    k = np.arange(65536, dtype=np.uint32)
    for seed, stage in ((0, 1), (0, 2), (12345, 1), (2 ** 32 - 1, 2), (2 ** 40 + 7, 1)):
        u = np.zeros_like(k)
        dh.dh_u(C.c_uint64(seed), stage, _p(k), len(k), _p(u))
        assert np.array_equal(u, frontend.dense_u(seed, stage, k)) and int(u.max()) < 1 << 24
        assert u[:20].tolist() == [py_hash((seed * 0x9E3779B1 + stage * 0x85EBCA77 + i) & 0xffffffff) >> 8 for i in range(20)]
        for S, M in (((1 << 22) << 16, 65536), (65536 << 20, 16384), (1, 1), (7, 3), ((1 << 38) - 12345, 65535)):
            kk = np.arange(M, dtype=np.uint64)
            P = np.zeros(M, dtype=np.uint64)
            dh.dh_position(_p(kk), _p(u[:M]), M, C.c_uint64(S), C.c_uint64(M), _p(P))
            assert np.array_equal(P, frontend.dense_position(kk, S, M, u[:M]))
            for i in sorted({0, min(1, M - 1), M // 2, M - 1}):
                assert int(P[i]) == (i * S + ((int(u[i]) * S) >> 24)) // M
            assert int(P.max()) < S and (np.diff(P.astype(np.int64)) >= 0).all()  # below the sum, non-decreasing in k
    assert frontend.dense_u(2 ** 32 + 5, 1, [3])[0] == frontend.dense_u(5, 1, [3])[0]  # only the seed's low 32 bits count


def test_cell_index_equals_the_definition(dh):
    """D6 at every pixel of maps whose sizes are no multiple of the grid, the last pixel included, and at the largest extents"""
    for grid in range(1, 9):
        xi1, yi1 = (a.reshape(-1).astype(np.int32) for a in np.meshgrid(np.arange(dc.W1), np.arange(dc.H1)))
        xi2, yi2 = (xi1 * 7 + 3) % dc.W2, (yi1 * 5 + 1) % dc.H2
        xi2[-1], yi2[-1] = dc.W2 - 1, dc.H2 - 1
        got = np.zeros(len(xi1), dtype=np.int32)
        dh.dh_cell(_p(xi1), _p(yi1), _p(np.ascontiguousarray(xi2)), _p(np.ascontiguousarray(yi2)), len(xi1), dc.W1, dc.H1, dc.W2, dc.H2, grid, _p(got))
        want = frontend.dense_cell(xi1, yi1, xi2, yi2, dc.W1, dc.H1, dc.W2, dc.H2, grid)
        assert np.array_equal(got, want) and got.min() == 0 and got.max() == grid ** 4 - 1 and got[-1] == grid ** 4 - 1, grid
    big = 2 ** 31 - 1
    one = np.array([big - 1], dtype=np.int32)
    got = np.zeros(1, dtype=np.int32)
    dh.dh_cell(_p(one), _p(one), _p(one), _p(one), 1, big, big, big, big, 8, _p(got))
    assert got[0] == 4095 == frontend.dense_cell(one, one, one, one, big, big, big, big, 8)[0]
    cnt = np.array([1, 2, 3, 7, 1000, 65536], dtype=np.uint32)
    for min_count in (1, 2, 8, 10 ** 6):
        w = np.zeros_like(cnt)
        dh.dh_cell_weight(_p(cnt), len(cnt), min_count, _p(w))
        assert np.array_equal(w.astype(np.uint64), frontend.dense_cell_weight(cnt, min_count)), min_count
    assert frontend.dense_cell_weight([1, 2, 3], 2).tolist() == [1, 1 << 19, (1 << 20) // 3]


# ---- properties of the definition itself
ARGS = [dict(), dict(balanced=False), dict(ranked=True), dict(grid=3, min_count=1), dict(grid=1), dict(min_count=10 ** 6), dict(filter="finite"), dict(seed=99)]


@pytest.mark.parametrize("kw", ARGS, ids=[",".join(f"{k}={v}" for k, v in kw.items()) or "defaults" for kw in ARGS])
def test_the_definition_picks_distinct_candidates_in_order(kw):
    b = dc.batch("blocks")
    warp, cert, dm1, dm2 = dc.as_seen(b)
    n = 200
    x1, x2, d1, d2, rows, score = frontend.sample_dense_numpy(warp[0], cert[0], dm1[0], dm2[0], n, **kw)
    q = frontend.dense_candidates(warp[0], cert[0], dm1[0], dm2[0], filter=kw.get("filter", "both_inf"))[0]
    assert 0 < len(rows) <= n and rows.dtype == np.int32 and len(x1) == len(x2) == len(d1) == len(d2) == len(score) == len(rows)
    assert (q[rows] > 0).all() and len(np.unique(rows)) == len(rows)  # every pick is a candidate, none twice
    if kw.get("ranked"):
        assert (np.diff(score) <= 0).all() and (np.diff(rows)[np.diff(score) == 0] > 0).all() and (np.diff(score) == 0).any()  # ties by ascending row
    else:
        assert (np.diff(rows) > 0).all()
    assert np.array_equal(score, cert[0][rows].astype(np.float64))
    if kw.get("filter") == "finite":
        assert np.isfinite(d1).all() and np.isfinite(d2).all()
    elif not kw.get("ranked"):
        assert not (np.isinf(d1) & np.isinf(d2)).any()
    other = frontend.sample_dense_numpy(warp[0], cert[0], dm1[0], dm2[0], n, **dict(kw, seed=kw.get("seed", 0) + 1))[4]
    assert not np.array_equal(np.sort(other), np.sort(rows))  # a different seed changes the picks


def test_an_empty_pair_a_large_n_and_the_batch_position():
    b = dc.batch("blocks")
    warp, cert, dm1, dm2 = dc.as_seen(b)
    assert not dc.candidates("blocks", 1).any()  # T = 0
    assert all(len(a) == 0 for a in frontend.sample_dense_numpy(warp[1], cert[1], dm1[1], dm2[1], 200))
    ref = dc.reference("blocks", 200, centres=False)
    assert ref[4].tolist() == [ref[4][0], 0, ref[4][0]] and ref[4][0] > 100
    for a in ref[:4] + ref[5:]:  # the same pair at two batch positions: the same result
        assert a[0].tobytes() == a[2].tobytes()
    assert (ref[5][1] == -1).all() and (ref[0][1] == 0).all() and (ref[2][1] == 1).all() and (ref[6][1] == 0).all()  # the filler
    K = int(np.count_nonzero(dc.candidates("small", 0)))
    for balanced in (True, False):
        rows = frontend.sample_dense_numpy(*[a[0] for a in dc.as_seen(dc.batch("small"))], 1000, balanced=balanced)[4]
        assert 0 < len(rows) <= K < dc.R_SMALL < 1000  # n above the candidate count: at most every candidate
    for bad in (dict(n=0), dict(n=16385), dict(n=100, expansion=0), dict(n=16384, expansion=5), dict(n=100, grid=0), dict(n=100, grid=9), dict(n=100, min_count=0)):
        with pytest.raises(ValueError):
            frontend.sample_dense_numpy(warp[0], cert[0], dm1[0], dm2[0], **bad)
    with pytest.raises(ValueError):
        frontend.sample_dense_numpy(warp[0], cert[0], dm1[0], dm2[0], 100, coords="pixels")


def test_forced_duplicates_are_dropped_and_the_picks_stay_sorted():
    """five rows of weight 65536 among thousands of weight 1 with M1 near K: the heavy rows span many strata, each is picked once"""
    q = dc.candidates("duplicates", 0)
    K = int(np.count_nonzero(q))
    heavy = np.flatnonzero(q == 65536)
    assert len(heavy) == 5 and K > 2000 and set(np.unique(q)) == {0, 1, 65536}
    M1 = K - 7
    picks = frontend.stratified_draw(q, M1, 1, 0)
    assert (np.diff(picks) > 0).all() and (q[picks] > 0).all() and set(heavy) <= set(picks)
    assert len(picks) < M1 // 50  # nearly every stratum lies inside a heavy row: its pick is a duplicate
    k = np.arange(M1, dtype=np.uint64)
    raw = np.searchsorted(np.cumsum(q, dtype=np.uint64), frontend.dense_position(k, int(q.sum(dtype=np.uint64)), M1, frontend.dense_u(0, 1, k)), side="right")
    assert (np.diff(raw) >= 0).all() and np.array_equal(np.unique(raw), picks)  # non-decreasing before the rule; the rule keeps each once
    warp, cert, dm1, dm2 = dc.as_seen(dc.batch("duplicates"))
    rows = frontend.sample_dense_numpy(warp[0], cert[0], dm1[0], dm2[0], M1, balanced=False)[4]
    assert np.array_equal(rows, picks)


def test_inclusion_frequency_of_stage_one():
    """Over S = 6000 seeds the inclusion frequency of a row in the stage-1 draw lies within 5 binomial standard deviations of p = q_r M1 / T, for
    every row with p <= 0.5: stratum k is uniform on its interval up to the 24-bit grid, and a row is hit with the probability of its share.
    The share is exact for a row inside one stratum; a row across a stratum boundary can be hit from both sides and is kept once, which lowers its
    frequency by the product of its two shares, at most p^2 / 4.  R = 300 rows (120 candidates with weights 20000 .. 65536, 150 with 4000 .. 12000,
    thirty non-candidates) and M1 = 12 keep p between 0.007 and 0.12: at least 44 expected hits per row (the normal bound holds) and a boundary
    term below 0.9 standard deviations.  On the CPU the definition's largest deviation here is 2.95 standard deviations (printed below); 13 rows of
    270 deviate by more than two, where a normal law expects 12."""
    rng = np.random.default_rng(7)
    R, M1, S = 300, 12, 6000
    q = np.concatenate([rng.integers(20000, 65537, 120), rng.integers(4000, 12001, 150), np.zeros(30, dtype=np.int64)]).astype(np.uint32)
    q = q[rng.permutation(R)]
    T = int(q.sum(dtype=np.uint64))
    hits = np.zeros(R)
    for seed in range(S):
        hits[frontend.stratified_draw(q, M1, 1, seed)] += 1
    p = q.astype(np.float64) * M1 / T
    check = (p <= 0.5) & (q > 0)
    sigma = np.sqrt(p[check] * (1 - p[check]) / S)
    z = np.abs(hits[check] / S - p[check]) / sigma
    print("rows checked %d of %d, p %.4f .. %.4f, largest deviation %.2f standard deviations, %d above two; boundary term at most %.2f" %
          (check.sum(), R, p[check].min(), p[check].max(), z.max(), (z > 2).sum(), (p[check] ** 2 / 4 / sigma).max()))
    assert check.sum() == 270 and (hits[q == 0] == 0).all() and S * p[check].min() >= 40
    assert z.max() <= 5.0


# ---- the Python entry points check their arguments before anything touches the device (there is none here)
def test_python_argument_checks():
    import torch
    from mdrp_amd import poselib
    warp, cert = torch.zeros((2, 50, 4)), torch.zeros((2, 50))
    dm = torch.ones((2, 8, 9))
    for bad in (dict(n=0), dict(n=16385), dict(expansion=0), dict(n=16384, expansion=5), dict(grid=0), dict(grid=9), dict(min_count=0), dict(coords="pixels"),
                dict(filter="nonsense"), dict(seed=-1)):
        with pytest.raises(ValueError, match=next(iter(bad)) if "n" not in bad else "n"):
            poselib.sample_dense_torch(warp, cert, dm, dm, **{"n": 100, **bad})
        with pytest.raises(ValueError):
            poselib.estimate_dense_torch("calibrated", warp, cert, dm, dm, None, None, **{"n": 100, **bad})
    with pytest.raises(ValueError, match="GPU"):
        poselib.sample_dense_torch(warp, cert, dm, dm, n=100)
    with pytest.raises(ValueError, match="GPU"):
        poselib.sample_dense_torch(warp.numpy(), cert, dm, dm, n=100)
    for kind in ("fundamental", _capi.RELPOSE_5PT, _capi.FUNDAMENTAL_7PT, -1):
        with pytest.raises(ValueError, match="kind|monodepth"):
            poselib.estimate_dense_torch(kind, warp, cert, dm, dm, n=100)
