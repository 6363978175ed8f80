"""The baselines' device front end without a GPU (include/mdrp_classic_frontend.h): the NumPy definitions (mdrp_amd/frontend.py) on planted tables,
the row rule of mdrp_amd/csrc/mdrp_frontend.h (host build, tests/hostmath/points_host.cpp) against them, the extension header against the binding,
the build and the library, the Python entry points' argument checks, the register budget of the new kernels, and the history table of
tests/classic_frontend_history_cases.py against the header's declarations."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import classic_frontend_cases as cf
from mdrp_amd import _capi, frontend

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SRC = os.path.join(HERE, "hostmath", "points_host.cpp")
HDR = os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_frontend.h")
SO = os.path.join(HERE, "hostmath", "libpoints_host.so")
NAMES = ("mdrp_gather_point_matches", "mdrp_gather_point_matches_ranked", "mdrp_gather_point_image_pairs", "mdrp_gather_point_image_pairs_ranked",
         "mdrp_estimate_classic_matches_async", "mdrp_estimate_classic_matches_ranked_async", "mdrp_estimate_classic_image_pairs_async",
         "mdrp_estimate_classic_image_pairs_ranked_async")
NAN, INF = np.nan, np.inf


# ---- the definition on planted tables
def test_the_per_pair_definition_on_a_planted_table():
    """padding between kept rows, indices past the table, NaN / +inf / -inf coordinates in either image, centres, float32 tables widened exactly"""
    kp1 = np.array([[1.25, 2.5], [3.0, 4.0], [NAN, 1.0], [5.0, INF], [7.0, 8.0], [0.1, 0.2]], dtype=np.float32)
    kp2 = np.array([[10.0, 20.0], [-INF, 1.0], [30.0, 40.0], [1.0, NAN], [50.0, 60.0]], dtype=np.float32)
    matches = np.array([[0, 0], [-1, -1], [1, 2], [2, 0], [3, 0], [0, 1], [0, 3], [-1, 2], [4, -3], [6, 0], [0, 5], [4, 4], [5, 2], [2 ** 31 - 1, 0]])
    x1, x2, slot = frontend.gather_point_matches_numpy(kp1, kp2, matches, center1=[0.5, 0.25], center2=[1.0, 2.0])
    assert slot.dtype == np.int32 and slot.tolist() == [0, -1, 1, -1, -1, -1, -1, -1, -1, -1, -1, 2, 3, -1]
    assert x1.dtype == x2.dtype == np.float64
    assert x1.tolist() == [[0.75, 2.25], [2.5, 3.75], [6.5, 7.75], [float(np.float32(0.1)) - 0.5, float(np.float32(0.2)) - 0.25]]
    assert x2.tolist() == [[9.0, 18.0], [29.0, 38.0], [49.0, 58.0], [29.0, 38.0]]
    y1, y2, s2 = frontend.gather_point_matches_numpy(kp1, kp2, matches)
    assert s2.tolist() == slot.tolist() and y1.tobytes() == kp1[[0, 1, 4, 5]].astype(np.float64).tobytes() and y2.tobytes() == kp2[[0, 2, 4, 2]].astype(np.float64).tobytes()
    px1, px2, n, ps = frontend.pad_point_pairs([(x1, x2, slot)], 16)
    assert n.tolist() == [4] and n.dtype == np.int32 and ps[0, :14].tolist() == slot.tolist() and (ps[0, 14:] == -1).all()
    assert not px1[0, 4:].any() and not px2[0, 4:].any() and px1[0, :4].tobytes() == x1.tobytes()
    with pytest.raises(ValueError):
        frontend.gather_point_matches_numpy(kp1.astype(np.float16), kp2, matches)
    with pytest.raises(ValueError):
        frontend.gather_point_matches_numpy(kp1[:, 0], kp2, matches)


def test_scores_rank_the_kept_rows_and_never_move_membership():
    """ties by ascending match row, NaN last (beside -inf, by row), -0.0 = +0.0, float32 scores; the highest scores, NaN and +inf on dropped rows"""
    kp = np.array([[1.0, 1.0], [2.0, 2.0], [3.0, 3.0], [NAN, 0.0]], dtype=np.float64)
    matches = np.array([[0, 0], [1, 1], [-1, 0], [2, 2], [3, 0], [0, 1], [1, 2], [0, 9], [2, 0], [1, 0]])
    kept = [0, 1, 3, 5, 6, 8, 9]
    scores = np.array([0.5, NAN, 99.0, 0.5, INF, -0.0, 0.0, NAN, -INF, 0.75])
    x1, x2, slot = frontend.gather_point_matches_numpy(kp, kp, matches, scores=scores)
    # kept rows by descending key, ties by row: 9 (0.75), 0 (0.5), 3 (0.5), 5 (-0.0), 6 (+0.0), 1 (NaN = -inf), 8 (-inf)
    assert slot.tolist() == [1, 5, -1, 2, -1, 3, 4, -1, 6, 0]
    order = [9, 0, 3, 5, 6, 1, 8]
    assert x1.tolist() == kp[matches[order, 0]].tolist() and x2.tolist() == kp[matches[order, 1]].tolist()
    plain = frontend.gather_point_matches_numpy(kp, kp, matches)[2]
    assert np.flatnonzero(plain >= 0).tolist() == kept == np.flatnonzero(slot >= 0).tolist()
    s32 = frontend.gather_point_matches_numpy(kp, kp, matches, scores=scores.astype(np.float32))[2]
    assert s32.tolist() == slot.tolist()
    for bad in (scores[:-1], np.zeros(len(scores), dtype=np.int64), np.stack([scores, scores])):
        with pytest.raises(ValueError):
            frontend.gather_point_matches_numpy(kp, kp, matches, scores=bad)
    # the planted batches: whatever the pattern, membership is the unranked one and the ranks are a permutation of 0 .. n - 1
    for name in ("small", "edges"):
        batch = cf.batches()[name]
        plain = cf.twin(batch, np.float32, True)
        for offset in range(7):
            ranked = cf.twin(batch, np.float32, True, cf.scores_of(batch, offset, 3))
            assert np.array_equal(ranked[2], plain[2]) and np.array_equal(ranked[3] >= 0, plain[3] >= 0)
            for b, n in enumerate(plain[2]):
                assert sorted(ranked[3][b][ranked[3][b] >= 0].tolist()) == list(range(n))
                assert sorted(map(tuple, ranked[0][b, :n].tolist())) == sorted(map(tuple, plain[0][b, :n].tolist()))


def test_the_per_image_definition_on_a_planted_table():
    """kp_counts above k_max and negative, an image index out of range on either side, a == c, a repeated pair, centres per image"""
    kp = np.arange(3 * 4 * 2, dtype=np.float64).reshape(3, 4, 2)
    kp[1, 2, 0] = NAN
    pairs = np.array([[0, 1], [1, 1], [0, 3], [-1, 0], [2, 0], [0, 1], [0, 2]])
    rows = np.array([[0, 0], [3, 3], [1, 2], [-1, 1], [2, 1], [4, 0]])
    matches = np.tile(rows, (len(pairs), 1, 1))
    counts = np.array([9, 3, -2])  # image 0: clamped to 4; image 1: its last keypoint is not valid; image 2: no keypoint at all
    centers = np.array([[0.5, 0.5], [1.0, 1.0], [2.0, 2.0]])
    x1, x2, n, slot = frontend.gather_point_image_pairs_numpy(kp, pairs, matches, centers, counts)
    assert n.tolist() == [2, 1, 0, 0, 0, 2, 0] and n.dtype == np.int32 and slot.dtype == np.int32
    assert slot[0].tolist() == [0, -1, -1, -1, 1, -1] == slot[5].tolist()  # (3, 3): past image 1's count; (1, 2): NaN; (4, 0): past the table
    assert x1[0, :2].tolist() == [[-0.5, 0.5], [3.5, 4.5]] and x2[0, :2].tolist() == [[7.0, 8.0], [9.0, 10.0]] and not x1[0, 2:].any()
    assert x1[0].tobytes() == x1[5].tobytes() and x2[0].tobytes() == x2[5].tobytes()
    # a == c: image 1 against itself; row (2, 1) reads the NaN keypoint on side 1 and is dropped, row (0, 0) is kept
    assert slot[1].tolist() == [0, -1, -1, -1, -1, -1]
    for b in (2, 3, 4, 6):
        assert (slot[b] == -1).all() and not x1[b].any() and not x2[b].any()
    everything = frontend.gather_point_image_pairs_numpy(kp, pairs, matches)
    assert everything[2].tolist() == [3, 2, 0, 0, 4, 3, 4]
    with pytest.raises(ValueError):
        frontend.gather_point_image_pairs_numpy(kp, pairs, matches[:3])
    with pytest.raises(ValueError):
        frontend.gather_point_image_pairs_numpy(kp, pairs, matches, centers[:2])
    # the reduction that is the definition: every pair is the per-pair function on the two images' valid tables
    t = cf.image_batch()
    got = frontend.gather_point_image_pairs_numpy(t["keypoints"], t["pairs"], t["matches"], t["centers"], t["kp_counts"])
    exp = cf.expand_image_batch(t)
    for a, b in zip(got, cf.twin(exp, np.float64, True)):
        assert a.tobytes() == b.tobytes()


# ---- the row rule of the header, compiled for the host
@pytest.fixture(scope="module")
def ph():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", SRC, "-o", SO])
    return C.CDLL(SO)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _host_gather(ph, batch, kp_dtype, centres):
    kp1, kp2 = np.ascontiguousarray(batch["kp1"].astype(kp_dtype)), np.ascontiguousarray(batch["kp2"].astype(kp_dtype))
    mt = np.ascontiguousarray(batch["matches"].astype(np.int32))
    B, M = mt.shape[:2]
    x1, x2 = np.full((B, M, 2), -7.0), np.full((B, M, 2), -7.0)
    slot, n = np.full((B, M), -7, dtype=np.int32), np.full(B, -7, dtype=np.int32)
    c1, c2 = (np.ascontiguousarray(batch["c1"]), np.ascontiguousarray(batch["c2"])) if centres else (None, None)
    fn = ph.ph_gather_points_f32 if kp_dtype == np.float32 else ph.ph_gather_points_f64
    fn(_p(kp1), _p(kp2), kp1.shape[1], kp2.shape[1], _p(mt), M, _p(c1), _p(c2), B, _p(x1), _p(x2), _p(slot), _p(n))
    return x1, x2, n, slot


@pytest.mark.parametrize("kp_dtype", [np.float32, np.float64])
def test_the_headers_row_rule_equals_the_numpy_definition(ph, kp_dtype):
    """fe_row_valid + fe_point_row + the per-image rules, walked in match order on the CPU, give the bytes of the NumPy definition: every planted
    batch, and a table of special values in every coordinate"""
    for name in ("small", "edges", "long", "m1025"):
        batch = cf.batches()[name]
        for centres in (False, True):
            for a, b in zip(_host_gather(ph, batch, kp_dtype, centres), cf.twin(batch, kp_dtype, centres)):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, centres)
    special = np.array([NAN, -NAN, INF, -INF, 0.0, -0.0, 1.5, np.finfo(kp_dtype).max, -np.finfo(kp_dtype).max, np.finfo(kp_dtype).tiny, 5e-324 if kp_dtype == np.float64 else 1e-45],
                       dtype=kp_dtype)
    grid = np.stack(np.meshgrid(special, special, indexing="ij"), -1).reshape(-1, 2)
    K = len(grid)
    rng = np.random.default_rng(51)
    table = {"kp1": grid[None], "kp2": grid[rng.permutation(K)][None], "matches": np.stack([rng.integers(-2, K + 2, 4000), rng.integers(-2, K + 2, 4000)], 1)[None],
             "c1": np.array([[0.5, -0.25]]), "c2": np.array([[3.0, 1e300]])}
    with np.errstate(invalid="ignore", over="ignore"):
        ref = cf.twin(table, kp_dtype, True)
    got = _host_gather(ph, table, kp_dtype, True)
    assert 100 < ref[2][0] < 3000 and (~np.isfinite(table["kp1"])).sum() > 50, ref[2]  # (the filter is on the keypoint, not on the centred value)
    for a, b in zip(got, ref):
        assert a.tobytes() == b.tobytes()
    # per-image tables
    t = cf.image_batch()
    kp = np.ascontiguousarray(t["keypoints"].astype(kp_dtype))
    mt, pairs, counts = (np.ascontiguousarray(t[k].astype(np.int32)) for k in ("matches", "pairs", "kp_counts"))
    cs = np.ascontiguousarray(t["centers"])
    B, M = mt.shape[:2]
    for centres, with_counts in ((True, True), (False, False)):
        x1, x2 = np.full((B, M, 2), -7.0), np.full((B, M, 2), -7.0)
        slot, n = np.full((B, M), -7, dtype=np.int32), np.full(B, -7, dtype=np.int32)
        fn = ph.ph_gather_point_images_f32 if kp_dtype == np.float32 else ph.ph_gather_point_images_f64
        fn(_p(kp), _p(counts) if with_counts else None, kp.shape[1], _p(cs) if centres else None, kp.shape[0], _p(pairs), _p(mt), M, B, _p(x1), _p(x2), _p(slot), _p(n))
        ref = frontend.gather_point_image_pairs_numpy(kp, pairs, mt, cs if centres else None, counts if with_counts else None)
        for a, b in zip((x1, x2, n, slot), ref):
            assert a.tobytes() == b.tobytes(), (centres, with_counts)


def test_the_host_program_stands_alone_under_the_sanitizers(tmp_path):
    """the same source with its own main, built with -fsanitize=address,undefined: tables of their exact size, rows that must not be read through"""
    exe = tmp_path / "points_host_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DPOINTS_HOST_MAIN", SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "points_host: ok" in r.stdout, (r.stdout, r.stderr)


# ---- header, binding, build, library
def _declaration(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, name
    return [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]


def test_header_binding_and_build_agree(tmp_path):
    """eight new symbols within ABI 6, declared in a third extension header that mdrp.h includes last; the export list is the header's, disjoint from
    the other three; the header is a build dependency; a C host that includes mdrp.h alone compiles against the declarations written out here and
    links against the built library"""
    from mdrp_amd import build
    main = open(os.path.join(ROOT, "include", "mdrp.h")).read()
    assert int(re.search(r"#define MDRP_ABI_VERSION (0x[0-9a-fA-F]+)", main).group(1), 16) == 6 == _capi.ABI_VERSION
    assert main.index('#include "mdrp_classic_ranked.h"') < main.index('#include "mdrp_classic_models.h"') < main.index('#include "mdrp_classic_frontend.h"')
    for name in NAMES + ("mdrp_point_matches", "mdrp_point_image_pairs"):  # declared in the extension header only: tests/history_cases.py enumerates mdrp.h's own
        assert not re.search(r"\b" + name + r"\b", main), name
    path = os.path.join(ROOT, "include", "mdrp_classic_frontend.h")
    hdr = open(path).read()
    assert os.path.realpath(path) in [os.path.realpath(d) for d in build.DEPS] and os.path.realpath(HDR) in [os.path.realpath(d) for d in build.DEPS]
    assert sorted(_capi.EXPORTS_CLASSIC_FRONTEND) == sorted(NAMES) == sorted(set(re.findall(r"\b(mdrp_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))))
    others = set(_capi.EXPORTS) | set(_capi.EXPORTS_CLASSIC_RANKED) | set(_capi.EXPORTS_CLASSIC_MODELS)
    assert not set(_capi.EXPORTS_CLASSIC_FRONTEND) & others
    out = "double *, double *, int32_t *, int32_t *"
    est = "const mdrp_camera *, const mdrp_camera *, const mdrp_ransac_opt *, const mdrp_bundle_opt *, uint8_t *, int32_t *"
    lines = ['#include "mdrp.h"']
    for k, (stem, desc) in enumerate((("matches", "mdrp_point_matches"), ("image_pairs", "mdrp_point_image_pairs"))):
        lines += [f"typedef int (*g{k}_t)(mdrp_handle *, const {desc} *, int, {out});", f"typedef int (*gr{k}_t)(mdrp_handle *, const {desc} *, const void *, int, int, {out});",
                  f"typedef int (*e{k}_t)(mdrp_handle *, int, const {desc} *, int, {est});",
                  f"typedef int (*er{k}_t)(mdrp_handle *, int, const {desc} *, const void *, int, int, {est});",
                  f"g{k}_t g{k} = mdrp_gather_point_{stem};", f"gr{k}_t gr{k} = mdrp_gather_point_{stem}_ranked;",
                  f"e{k}_t e{k} = mdrp_estimate_classic_{stem}_async;", f"er{k}_t er{k} = mdrp_estimate_classic_{stem}_ranked_async;"]
    lines += ["int main(void) { return (g0 && gr0 && e0 && er0 && g1 && gr1 && e1 && er1) ? 0 : 1; }"]
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "abi.o")], check=True)
    build.build()
    lib = _capi.load_library()
    subprocess.run(["gcc", str(tmp_path / "abi.o"), "-o", str(tmp_path / "abi"), build.OUT, "-Wl,--unresolved-symbols=ignore-in-shared-libs"], check=True)
    syms = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, count in zip(NAMES, (7, 9, 7, 9, 10, 12, 10, 12)):
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", syms), name
        assert len(getattr(lib, name).argtypes) == len(_declaration(hdr, name)) == count, name
    for method in ("gather_points", "estimate_points_device"):
        assert callable(getattr(_capi.Handle, method))


@pytest.mark.parametrize("struct,ctype", [("mdrp_point_matches", "PointMatches"), ("mdrp_point_image_pairs", "PointImagePairs")])
def test_descriptor_layout_matches_header(tmp_path, struct, ctype):
    """sizeof and every field offset of the ctypes descriptors against the header, through a C compiler; the fields are the ones the issue names"""
    cls = getattr(_capi, ctype)
    names = [f for f, _ in cls._fields_]
    assert names == {"mdrp_point_matches": ["kp1", "kp2", "kp_type", "k1", "k2", "matches", "m_max", "center1", "center2"],
                     "mdrp_point_image_pairs": ["kp", "kp_type", "k_max", "kp_count", "center", "n_images", "pairs", "matches", "m_max"]}[struct]
    hdr = open(os.path.join(ROOT, "include", "mdrp_classic_frontend.h")).read()
    end = hdr.index("} " + struct + ";")
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.rindex("typedef struct {", 0, end):end], flags=re.S)
    declared = [n for decl in re.findall(r"[\w ]+?((?:\*?\w+\s*,\s*)*\*?\w+)\s*;", body) for n in re.findall(r"\w+", decl)]
    assert declared == names, declared
    src = tmp_path / "layout.c"
    src.write_text('#include "mdrp.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n    printf("%zu", sizeof(' + struct + "));\n"
                   + "".join(f'    printf(" %zu", offsetof({struct}, {n}));\n' for n in names) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(cls) and out[1:] == [getattr(cls, n).offset for n in names]


# ---- the Python entry points check their arguments before anything touches the device (there is none here)
def test_python_argument_checks():
    import torch
    from mdrp_amd import poselib
    B, K, M, I = 2, 9, 12, 3
    kp = torch.zeros((B, K, 2))
    mt = torch.zeros((B, M, 2), dtype=torch.int64)
    ikp = torch.zeros((I, K, 2))
    pairs = [[0, 1], [1, 2]]
    per_pair = (poselib.gather_point_matches_torch, lambda *a, **k: poselib.estimate_baseline_matches_torch("fundamental_7pt", *a, **k))
    per_image = (poselib.gather_point_image_pairs_torch, lambda *a, **k: poselib.estimate_baseline_image_pairs_torch("fundamental_7pt", *a, **k))
    for fn in per_pair:  # host tensors, whatever else is right
        with pytest.raises(ValueError, match="on the GPU"):
            fn(kp, kp, mt)
        with pytest.raises(ValueError, match="on the GPU"):
            fn(kp.numpy(), kp.numpy(), mt.numpy())
    for fn in per_image:
        with pytest.raises(ValueError, match="on the GPU"):
            fn(ikp, pairs, mt)
    # everything else is checked on the tensors as they are, before the device is looked at: host tensors reach every check
    g = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)  # noqa: E731
    for fn in per_pair:
        with pytest.raises(ValueError, match="both be float32 or both float64"):
            fn(g((B, K, 2), torch.float16), g((B, K, 2), torch.float16), g((B, M, 2), torch.int64))
        with pytest.raises(ValueError, match="both be float32 or both float64"):
            fn(g((B, K, 2)), g((B, K, 2), torch.float64), g((B, M, 2), torch.int64))
        with pytest.raises(ValueError, match="int32 or int64"):
            fn(g((B, K, 2)), g((B, K, 2)), g((B, M, 2), torch.int16))
        with pytest.raises(ValueError, match=r"\(B, K, 2\)"):
            fn(g((B, K, 3)), g((B, K, 3)), g((B, M, 2), torch.int64))
        with pytest.raises(ValueError, match=r"\(B, M, 2\)"):
            fn(g((B, K, 2)), g((B, K, 2)), g((B + 1, M, 2), torch.int64))
        with pytest.raises(ValueError, match=r"\(B, M, 2\)"):
            fn(g((B, K, 2)), g((B, K, 2)), g((B, M), torch.int64))
        with pytest.raises(ValueError, match="the only string"):
            fn(g((B, K, 2)), g((B, K, 2)), g((B, M, 2), torch.int64), scores="sorted")
        with pytest.raises(ValueError, match="float32 / float64 tensor"):
            fn(g((B, K, 2)), g((B, K, 2)), g((B, M, 2), torch.int64), scores=g((B, M), torch.int32))
        with pytest.raises(ValueError, match="one per match row"):
            fn(g((B, K, 2)), g((B, K, 2)), g((B, M, 2), torch.int64), scores=g((B, M + 1)))
    for fn in per_image:
        with pytest.raises(ValueError, match="float32 or float64"):
            fn(g((I, K, 2), torch.float16), pairs, g((B, M, 2), torch.int64))
        with pytest.raises(ValueError, match="int32 or int64"):
            fn(g((I, K, 2)), pairs, g((B, M, 2), torch.uint8))
        with pytest.raises(ValueError, match=r"\(I, K, 2\)"):
            fn(g((I, K)), pairs, g((B, M, 2), torch.int64))
        with pytest.raises(ValueError, match="pairs' B"):
            fn(g((I, K, 2)), pairs, g((B + 1, M, 2), torch.int64))
        with pytest.raises(ValueError, match="integer image indices"):
            fn(g((I, K, 2)), [[0.5, 1.0]], g((1, M, 2), torch.int64))
        with pytest.raises(ValueError, match="one per match row"):
            fn(g((I, K, 2)), pairs, g((B, M, 2), torch.int64), scores=g((M, B)))
        with pytest.raises(ValueError, match="the only string"):
            fn(g((I, K, 2)), pairs, g((B, M, 2), torch.int64), scores="ranked")
    # the kind, and the options the estimator refuses, come before the tensors are looked at
    for est in (poselib.estimate_baseline_matches_torch, poselib.estimate_baseline_image_pairs_torch):
        args = (kp, kp, mt) if est is poselib.estimate_baseline_matches_torch else (ikp, pairs, mt)
        for kind in ("calibrated", "shared_focal", "varying_focal", 5, None, "fundamental"):
            with pytest.raises(ValueError, match="kind"):
                est(kind, *args)
        with pytest.raises(NotImplementedError, match="needs the match scores"):
            est("relpose_5pt", *args, ransac_opt={"progressive_sampling": True})
        with pytest.raises(NotImplementedError, match="real_focal_check"):
            est("fundamental_7pt", *args, ransac_opt={"real_focal_check": True}, scores="presorted")
        with pytest.raises(ValueError, match="the only string"):
            est("fundamental_7pt", *args, scores="by_score")
    assert sorted(poselib.BASELINE_KINDS) == sorted(cf.KINDS)
    # the monodepth front end keeps refusing the baselines
    dm = torch.zeros((B, 4, 4))
    for kind in (3, 4, 5, "fundamental_7pt"):
        with pytest.raises(ValueError):
            poselib.estimate_matches_torch(kind, kp, kp, mt, dm, dm)


# ---- the new kernels in the code object
@pytest.fixture(scope="module")
def regs():
    from mdrp_amd import build
    import kernel_table
    build.build()
    return kernel_table.kernel_table()


@pytest.mark.parametrize("family,lds", [("k_gather_points", 16), ("k_gather_points_images", 16), ("k_gather_points_ranked", 2048 * 8 + 16),
                                        ("k_gather_points_images_ranked", 2048 * 8 + 16)])
def test_new_kernels_are_built_without_scratch_or_spills(regs, family, lds):
    """two instantiations each (the keypoint type; the score type is read at run time), no spill, no scratch, the LDS of their depth siblings"""
    found = sorted(k for k in regs if k.startswith(f"mdrp::{family}<"))
    assert found == [f"mdrp::{family}<double>", f"mdrp::{family}<float>"], found
    for name in found:
        r = regs[name]
        print(name, r)
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0 and r.get("agpr", 0) == 0, (name, r)
        assert r["lds"] == lds and r["waves_per_simd"] == 8, (name, r)


# ---- the history table of the new header
def test_every_entry_point_of_the_extension_header_is_in_its_history_table():
    """tests/test_history_host.py's rule for include/mdrp_classic_frontend.h: every function with a handle is run by
    tests/classic_frontend_history_cases.py, whose inputs are deterministic; the predecessors hold a larger and a smaller call, other kinds and the
    monodepth front end, which shares the gather buffers"""
    import classic_frontend_history_cases as fhc
    import classic_history_cases as chc
    import classic_models_history_cases as mhc
    import helpers
    import history_cases as hc
    named = {p for c in fhc.probes() for p in c.entry_points}
    assert set(fhc.extension_entry_points()) == set(NAMES) == named - {fhc.FETCH}
    assert {c.kind for c in fhc.probes() if c.estimate} == {3, 4, 5} and {c.score_dtype for c in fhc.probes()} == {None, np.float32, np.float64}
    assert {c.progressive for c in fhc.probes() if c.estimate and c.score_dtype is not None} == {None, True, False}
    assert {c.which for c in fhc.probes() if not isinstance(c, fhc.PointImagePairs)} == {0, 1}
    others = {c.name for c in hc.predecessors()} | {c.name for c in chc.probes()} | {c.name for c in mhc.probes()}
    assert not {c.name for c in fhc.probes() + fhc.refusals()} & others
    preds = fhc.predecessors()
    assert len({c.name for c in preds}) == len(preds) and {"front_end", "estimate", "ranked", "refusal", "classic_front_end"} <= {c.family for c in preds}
    assert any(c.family == "estimate" and c.batch > 6 and c.n_max > 607 for c in preds) and any(c.family == "estimate" and c.batch == 1 and c.n_max == 8 for c in preds)
    assert {c.kind for c in preds if c.family == "estimate"} >= {0, 3, 4, 5}
    assert sum(c.family == "front_end" for c in preds) >= 7 and sum(c.family == "front_end" for c in fhc.followers()) >= 8
    assert all(set(c.entry_points) & set(NAMES) for c in fhc.refusals())
    for c in fhc.probes():
        a, b = (helpers.input_digest(hc.four(c.digest_arrays(c.make()))) for _ in range(2))
        assert a == b, c
