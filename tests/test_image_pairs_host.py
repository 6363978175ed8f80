"""The front end on per-image tables without a GPU (include/mdrp.h mdrp_image_pairs): the ctypes descriptor against the header, the new
per-image rules of mdrp_amd/csrc/mdrp_frontend.h (host build) against their NumPy statement, gather_image_pairs_numpy against the per-pair
definition it reduces to, the register budget of the new kernels, and a guard that the GPU test's batch is not degenerate."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import image_pairs_cases as cases
from mdrp_amd import _capi, frontend

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "hostmath", "libimage_pairs_host.so")


@pytest.fixture(scope="module")
def ih():
    src = os.path.join(HERE, "hostmath", "image_pairs_host.cpp")
    hdr = os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_frontend.h")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", src, "-o", SO])
    return C.CDLL(SO)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_descriptor_layout_matches_header(tmp_path):
    """sizeof, every field offset, the field names and their order of the ctypes mdrp_image_pairs against the header, through a C compiler"""
    names = [f for f, _ in _capi.ImagePairs._fields_]
    hdr = open(os.path.join(ROOT, "include", "mdrp.h")).read()
    end = hdr.index("} mdrp_image_pairs;")
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.rindex("typedef struct {", 0, end):end], flags=re.S)
    declared = [n for decl in re.findall(r"[\w ]+?((?:\*?\w+\s*,\s*)*\*?\w+)\s*;", body) for n in re.findall(r"\w+", decl)]
    assert declared == names, declared
    src = tmp_path / "layout.c"
    src.write_text('#include "mdrp.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n    printf("%zu", sizeof(mdrp_image_pairs));\n'
                   + "".join(f'    printf(" %zu", offsetof(mdrp_image_pairs, {n}));\n' for n in names) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_capi.ImagePairs)
    assert out[1:] == [getattr(_capi.ImagePairs, n).offset for n in names]


def test_symbols_are_exported_within_abi_6():
    from mdrp_amd import build
    hdr = open(os.path.join(ROOT, "include", "mdrp.h")).read()
    assert int(re.search(r"#define MDRP_ABI_VERSION (0x[0-9a-fA-F]+)", hdr).group(1), 16) == _capi.ABI_VERSION == 0x00000006
    want = {"mdrp_gather_image_pairs", "mdrp_estimate_image_pairs_async"}
    assert want <= set(_capi.EXPORTS)
    lib = build.build()
    dynamic = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert want <= {line.split()[-1] for line in dynamic.splitlines() if line.strip()}


def test_image_index_rule_equals_numpy_statement(ih):
    for n_images in (0, 1, cases.I, 2 ** 31 - 1):
        a = np.unique(np.array([-2 ** 31, -1, 0, n_images - 1, n_images, 2 ** 31 - 1], dtype=np.int64)).astype(np.int32)
        ok = np.zeros(len(a), dtype=np.int32)
        ih.ih_image_valid(_p(a), len(a), n_images, _p(ok))
        assert np.array_equal(ok.astype(bool), frontend.image_valid(a, n_images)), n_images
        assert ok.tolist() == [int(0 <= int(v) < n_images) for v in a], n_images
    a = np.array([-2 ** 31, -1, 0, cases.I - 1, cases.I, 2 ** 31 - 1], dtype=np.int32)  # the inputs the definition names, at I = 5
    ok = np.zeros(len(a), dtype=np.int32)
    ih.ih_image_valid(_p(a), len(a), cases.I, _p(ok))
    assert ok.tolist() == [0, 0, 1, 1, 0, 0]


def test_extent_clamp_equals_numpy_statement(ih):
    for maximum in (0, 1, cases.K, cases.H, cases.W, 2 ** 31 - 2):
        v = np.array([-2 ** 31, -1, 0, 1, maximum, maximum + 1, 2 ** 31 - 1], dtype=np.int32)
        out = np.zeros(len(v), dtype=np.int32)
        ih.ih_clamp_extent(_p(v), len(v), maximum, _p(out))
        assert np.array_equal(out, frontend.clamp_extent(v, maximum)), maximum
        assert out.tolist() == [min(max(int(x), 0), maximum) for x in v], maximum
    v = np.array([-1, 0, 1, cases.K, cases.K + 1], dtype=np.int32)  # the inputs the definition names, at max = K
    out = np.zeros(len(v), dtype=np.int32)
    ih.ih_clamp_extent(_p(v), len(v), cases.K, _p(out))
    assert out.tolist() == [0, 0, 1, cases.K, cases.K]


def test_table_offsets_come_from_the_image_index_in_64_bits(ih):
    """the offsets are the row-major ones of [I][k_max][2] and [I][h_max][w_max] (stride w_max) and do not wrap at 2^31 or 2^32 elements"""
    a = np.array([0, 1, 4, 45, 70000, 2 ** 31 - 1], dtype=np.int32)
    i = np.array([0, 699, 3, 2047, 2047, 2047], dtype=np.int32)
    out = np.zeros(len(a), dtype=np.uint64)
    ih.ih_kp_offset(_p(a), _p(i), len(a), 2048, _p(out))
    assert out.tolist() == [2 * (int(x) * 2048 + int(y)) for x, y in zip(a, i)]
    yi = np.array([0, 47, 3, 479, 479, 479], dtype=np.int32)
    xi = np.array([0, 71, 5, 639, 639, 639], dtype=np.int32)
    ih.ih_depth_offset(_p(a), _p(yi), _p(xi), len(a), 480, 640, _p(out))
    assert out.tolist() == [(int(x) * 480 + int(y)) * 640 + int(z) for x, y, z in zip(a, yi, xi)]
    ih.ih_depth_offset(_p(a[:3]), _p(yi[:3]), _p(xi[:3]), 3, cases.H, cases.W, _p(out))
    flat = np.arange(cases.I * cases.H * cases.W).reshape(cases.I, cases.H, cases.W)
    assert out[:3].tolist() == [int(flat[x, y, z]) for x, y, z in zip(a[:3], yi[:3], xi[:3])]


def test_numpy_statement_reduces_to_the_per_pair_definition():
    """sizes and kp_counts omitted, all indices valid: gather_matches_numpy on keypoints[pairs[:, 0]], ... pair by pair, byte for byte"""
    t = cases.batch()
    good = [b for b in range(len(cases.PAIRS)) if b not in cases.BAD]
    pairs, matches = t["pairs"][good], t["matches"][good]
    for kp_dtype, depth_dtype, filter, centres in ((np.float32, np.float32, "both_inf", False), (np.float64, np.float32, "finite", True),
                                                   (np.float32, np.float64, "both_inf", True)):
        kp, dm = t["keypoints"].astype(kp_dtype), t["depth_maps"].astype(depth_dtype)
        got = frontend.gather_image_pairs_numpy(kp, dm, pairs, matches, centers=t["centers"] if centres else None, filter=filter)
        kp1, kp2, dm1, dm2 = kp[pairs[:, 0]], kp[pairs[:, 1]], dm[pairs[:, 0]], dm[pairs[:, 1]]
        c1, c2 = t["centers"][pairs[:, 0]], t["centers"][pairs[:, 1]]
        ref = frontend.pad_pairs([frontend.gather_matches_numpy(kp1[b], kp2[b], matches[b], dm1[b], dm2[b], c1[b] if centres else None,
                                                                c2[b] if centres else None, filter) for b in range(len(pairs))], cases.M)
        for mine, want in zip(got, ref):
            assert mine.dtype == want.dtype and mine.shape == want.shape and mine.tobytes() == want.tobytes()
        assert got[4].sum() > 500
    one = frontend.gather_image_pairs_numpy(t["keypoints"], t["depth_maps"], pairs, matches, centers=t["centers"][2])  # one centre for all images
    ref = frontend.gather_image_pairs_numpy(t["keypoints"], t["depth_maps"], pairs, matches, centers=np.tile(t["centers"][2], (cases.I, 1)))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, ref))


def test_numpy_statement_extents_and_bad_indices():
    """a keypoint past the valid width but inside the allocation is dropped, as is an index past kp_count that is inside the table; extents
    are clamped to the allocation; a pair with a bad image index is empty"""
    kp = np.zeros((2, 6, 2), dtype=np.float32)
    kp[0, :, 0] = [1.0, 4.5, 3.999, 2.0, 2.0, 2.0]   # image 0 is 3 x 4 valid in a 5 x 8 allocation: x = w + 0.5 = 4.5 is inside W = 8
    kp[0, :, 1] = [1.0, 1.0, 2.999, 3.0, 1.0, 1.0]   # y = h = 3 is inside H = 5
    kp[1, :, 0] = 6.0
    kp[1, :, 1] = 4.0
    dm = np.arange(2 * 5 * 8, dtype=np.float64).reshape(2, 5, 8) + 1.0
    sizes, counts = np.array([[3, 4], [5, 8]]), np.array([5, 6])
    matches = np.array([[[0, 0], [1, 0], [2, 1], [3, 2], [4, 3], [5, 4]]])
    x1, x2, d1, d2, n, slot = frontend.gather_image_pairs_numpy(kp, dm, [(0, 1)], matches, sizes=sizes, kp_counts=counts)
    assert slot.tolist() == [[0, -1, 1, -1, 2, -1]] and n.tolist() == [3]   # 4.5 >= w, 3.0 >= h, index 5 >= kp_count[0] = 5 < K = 6
    assert d1[0, :3].tolist() == [dm[0, 1, 1], dm[0, 2, 3], dm[0, 1, 2]] and d2[0, :3].tolist() == [dm[1, 4, 6]] * 3   # the stride is W = 8, not w = 4
    full = frontend.gather_image_pairs_numpy(kp, dm, [(0, 1)], matches)
    assert full[5].tolist() == [[0, 1, 2, 3, 4, 5]] and full[2][0, 1] == dm[0, 1, 4] and full[2][0, 3] == dm[0, 3, 2]
    over = frontend.gather_image_pairs_numpy(kp, dm, [(0, 1)], matches, sizes=[[7, 99], [5, 8]], kp_counts=[9, 6])  # clamped to the allocation
    assert all(a.tobytes() == b.tobytes() for a, b in zip(over, full))
    none = frontend.gather_image_pairs_numpy(kp, dm, [(0, 1)], matches, sizes=[[-1, 4], [5, 8]], kp_counts=[5, -3])
    assert none[4].tolist() == [0] and (none[5] == -1).all()
    bad = frontend.gather_image_pairs_numpy(kp, dm, [(0, 2), (-1, 0), (1, 0)], np.repeat(matches, 3, axis=0), sizes=sizes, kp_counts=counts)
    assert bad[4].tolist() == [0, 0, 4] and (bad[5][:2] == -1).all() and not bad[0][:2].any() and not bad[1][:2].any()
    assert (bad[2][:2] == 1.0).all() and (bad[3][:2] == 1.0).all()
    with pytest.raises(ValueError):
        frontend.gather_image_pairs_numpy(kp, dm, [(0, 1)], matches, filter="nonsense")
    with pytest.raises(ValueError):
        frontend.gather_image_pairs_numpy(kp, dm, [(0, 1), (1, 0)], matches)


def test_the_batch_holds_the_planted_cases():
    t = cases.batch()
    assert t["keypoints"].shape == (cases.I, cases.K, 2) and t["depth_maps"].shape == (cases.I, cases.H, cases.W) and t["matches"].shape == (10, cases.M, 2)
    assert (t["kp_counts"] < cases.K).sum() == 2
    assert [(int((m[:, 0] != -1).sum()) if b in cases.BAD else None) for b, m in enumerate(t["matches"])][7:9] == [256, 257]
    both, fin, free = cases.twin(filter="both_inf"), cases.twin(filter="finite"), cases.twin(extents=False)
    assert both[4][list(cases.BAD)].tolist() == [0, 0] and free[4][list(cases.BAD)].tolist() == [0, 0]
    assert (free[4] >= both[4]).all() and free[4].sum() > both[4].sum() + 20  # the valid sizes and counts drop rows of their own
    for b, rows in enumerate(cases.ROW_COUNTS):
        if b in cases.BAD or rows < 64:
            continue
        a = int(cases.PAIRS[b][0])
        n = both[4][b]
        assert 3 <= fin[4][b] <= n - 3 and n < rows - 10, (b, n, fin[4][b])  # one-sided inf / NaN rows differ
        d1, d2 = both[2][b, :n], both[3][b, :n]
        assert np.isnan(d1).any() and np.isnan(d2).any() and (np.isinf(d1) ^ np.isinf(d2)).any()
        w = int(cases.SIZES[a][1])
        assert (both[0][b, :n, 0] == -0.5).any() and (both[0][b, :n, 0] == np.float32(w - 0.001)).any()
        assert not np.isin(both[0][b, :, 0], [-1.0, float(w)]).any()


def test_new_kernels_are_built_and_use_no_scratch():
    from mdrp_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    build.build()
    regs = kernel_table.kernel_table()
    for name in [f"mdrp::k_gather_images<{k}, {d}>" for k in ("float", "double") for d in ("float", "double")]:
        assert name in regs, (name, sorted(k for k in regs if "gather" in k))
        r = regs[name]
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (name, r)
    assert sum(1 for k in regs if k.startswith("mdrp::k_gather_images<")) == 4
    assert sum(1 for k in regs if k.startswith("mdrp::k_gather<")) == 4


def test_the_batch_is_not_degenerate_for_the_estimator():
    """the CPU oracle on the NumPy-gathered input: at least one pair of 64 or more rows ends with an inlier ratio above 0.3, so that identical
    records in the GPU tests are records of real estimates"""
    from oracle import pyorc as po
    x1, x2, d1, d2, n, _ = cases.twin(filter="both_inf")
    ratios = {}
    for b in np.flatnonzero(n >= 64):
        a, c = (int(v) for v in cases.PAIRS[b])
        cams = [po.cam_flat(0, cases.CAMERAS[i]["params"]) for i in (a, c)]
        ro = po.ransac_opt(max_iterations=200, min_iterations=200, max_epipolar_error=cases.RO["max_epipolar_error"], max_reproj_error=cases.RO["max_reproj_error"])
        _, st, _ = po.estimate(po.CALIB, x1[b, :n[b]], x2[b, :n[b]], d1[b, :n[b]], d2[b, :n[b]], ro, po.bundle_opt(loss_type=4), *cams)
        ratios[int(b)] = st.num_inliers / n[b]
    assert ratios and max(ratios.values()) > 0.3, ratios
