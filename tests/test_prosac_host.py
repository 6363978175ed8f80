"""Estimating in match-score order without a GPU: the NumPy definition (tests/prosac_ref.py) and the host part of mdrp_amd/csrc/mdrp_prosac.h against
the reference binary's sampler tables and PROSAC estimates (tests/golden/prosac_ref.npz, tests/tools/gen_golden_prosac.py), the ranking's edge
cases, and the header, the binding and the Python argument checks."""
import os
import re
import subprocess

import numpy as np
import pytest

import prosac_cases as pcs
import prosac_ref as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = range(len(pcs.SAMPLER_ROWS))


@pytest.mark.parametrize("row", ROWS)
def test_the_definition_draws_the_reference_samplers_tables(row):
    """growth table and every sample index, exactly"""
    n, seed, mp, count = pcs.SAMPLER_ROWS[row]
    g = pcs.golden()
    assert ps.growth(n, mp) == g[f"growth_{row}"].tolist()
    got, subs = ps.samples(n, seed, mp, count)
    assert np.array_equal(got, g[f"samples_{row}"].astype(np.int64))
    prog = np.arange(count) + 1 < mp
    assert (got[prog, 2] == subs[prog] - 1).all() and (got[prog, :2] < (subs[prog] - 1)[:, None]).all()  # K - 1 from the subset's head, then its last record
    if count > mp > 1:
        assert not (got[~prog, 2] == subs[~prog] - 1).all()  # (the uniform phase is not the progressive one continued)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prosac_host") / "prosac_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostmath", "prosac_host.cpp"), "-o", exe])
    text = "".join(f"{n} {mp} {count}\n" for n, _, mp, count in pcs.SAMPLER_ROWS)
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == 4 * len(pcs.SAMPLER_ROWS)
    return [{ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in lines[4 * r:4 * r + 4]} for r in ROWS]


@pytest.mark.parametrize("row", ROWS)
def test_the_headers_growth_table_and_schedule_are_the_reference_samplers(host_program, row):
    """mdrp_prosac.h compiled into a stand-alone host program: growth table exactly; the subset size of every progressive sample is one more than the
    reference sample's third index; the device's truncated table is that schedule up to the first sample whose subset is all n"""
    n, seed, mp, count = pcs.SAMPLER_ROWS[row]
    g, out = pcs.golden(), host_program[row]
    assert out["growth"] == g[f"growth_{row}"].tolist()
    n_prog = min(count, max(mp - 1, 0))
    assert out["progressive"] == [max(mp - 1, 0)]
    assert out["subset"] == (g[f"samples_{row}"][:n_prog, 2].astype(np.int64) + 1).tolist() == ps.samples(n, seed, mp, count)[1][:n_prog].tolist()
    t = out["truncated"]
    assert t == out["subset"][:len(t)] and all(v < n for v in t) and all(v == n for v in out["subset"][len(t):])
    if n_prog and n > 3:
        assert len(t) > 0


def test_ranking_edge_cases():
    nan, inf = float("nan"), float("inf")
    assert ps.order([]).tolist() == [] and ps.order([5.0]).tolist() == [0]
    assert ps.order([1.0, 1.0, 1.0, 1.0]).tolist() == [0, 1, 2, 3]                # ties: ascending caller index
    assert ps.order([4.0, 3.0, 2.0, 1.0]).tolist() == [0, 1, 2, 3] and ps.order([1.0, 2.0, 3.0, 4.0]).tolist() == [3, 2, 1, 0]
    assert ps.order([0.0, -0.0, 0.0, -0.0]).tolist() == [0, 1, 2, 3]              # the zeros tie
    assert ps.order([-0.0, 1.0, 0.0, -1.0]).tolist() == [1, 0, 2, 3]
    assert ps.order([nan, -inf, 1.0, inf, nan, -1e308]).tolist() == [3, 2, 5, 0, 1, 4]  # NaN = -inf, ties with it by index
    s = np.random.default_rng(3).integers(0, 8, 97).astype(np.float64)             # 8 levels: ties everywhere
    o = ps.order(s)
    assert sorted(o.tolist()) == list(range(97)) and all((s[a] > s[b]) or (s[a] == s[b] and a < b) for a, b in zip(o[:-1], o[1:]))


@pytest.mark.parametrize("index", range(len(pcs.CASES)))
@pytest.mark.parametrize("kind", (0, 1, 2))
def test_the_definition_is_the_reference_under_progressive_sampling(kind, index):
    """the loop of prior_ref fed the progressive sample table, on the 27 cases the reference ran with progressive_sampling = true: iterations, inlier
    counts and masks identical, models to 1e-6, scores to SCORE_RTOL, LO counts equal (+-1 below N = 100).  No exemptions."""
    c, g = pcs.case(kind, index), pcs.golden_case(kind, index)
    assert pcs.digest(c) == g["digest"], "the inputs are not the ones the fixture was recorded on"
    assert np.array_equal(c["order"], g["order"]) and np.array_equal(ps.order(c["scores"]), g["order"])
    ro, bo, cam = pcs.oracle_options(c)
    r = ps.estimate(kind, c["x1"], c["x2"], c["d1"], c["d2"], c["scores"], ro, bo, c["max_prosac"], *((cam, cam) if kind == 0 else (None, None)))
    want = pcs.golden_answer(kind, index)
    got = dict(r, mask=r["mask_ranked"])
    dev = pcs.deviation(got, want, c["n"])
    print(kind, index, "LOs", r["refinements"], want["refinements"], "iterations", r["iterations"], want["iterations"], "inliers", r["num_inliers"],
          want["num_inliers"], dev)
    assert dev == []
    assert np.array_equal(r["mask"][r["order"]], r["mask_ranked"])  # the mask in the caller's order is the ranked one scattered


def _declaration(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, name
    return [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]


def test_header_and_binding_agree(tmp_path):
    """new symbols within ABI 6; the header's argument lists, checked by a C compiler against the lists written out here, are the binding's"""
    from mdrp_amd import _capi, build
    hdr = open(os.path.join(ROOT, "include", "mdrp.h")).read()
    assert int(re.search(r"#define MDRP_ABI_VERSION (0x[0-9a-fA-F]+)", hdr).group(1), 16) == 6 == _capi.ABI_VERSION
    head = "mdrp_handle *, int, {}const double *, const double *, const double *, const double *, const double *, int, int, const int32_t *, " \
           "const mdrp_camera *, const mdrp_camera *, const mdrp_ransac_opt *, const mdrp_bundle_opt *, "
    src = tmp_path / "abi.c"
    src.write_text('#include "mdrp.h"\n'
                   "typedef int (*blocking_t)(" + head.format("int, ") + "mdrp_result *, uint8_t *);\n"
                   "typedef int (*async_t)(" + head.format("") + "uint8_t *);\n"
                   "typedef int (*samples_t)(mdrp_handle *, uint64_t, int, uint64_t, const int32_t *, int, uint32_t *);\n"
                   "typedef int (*rank_t)(mdrp_handle *, int, const double *, int, int, const int32_t *, int32_t *);\n"
                   "blocking_t a = mdrp_estimate_batch_ranked;\nasync_t b = mdrp_estimate_batch_ranked_async;\n"
                   "samples_t c = mdrp_prosac_samples;\nrank_t d = mdrp_rank_scores;\n"
                   "_Static_assert(sizeof(mdrp_ransac_opt) == 88, \"mdrp_ransac_opt\");\n")
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "abi.o")], check=True)
    build.build()
    lib = _capi.load_library()
    assert lib.mdrp_abi_version() == 6
    for name, count in (("mdrp_estimate_batch_ranked", 17), ("mdrp_estimate_batch_ranked_async", 15), ("mdrp_prosac_samples", 7), ("mdrp_rank_scores", 7)):
        assert name in _capi.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(_declaration(hdr, name)) == count, name
    assert os.path.realpath(os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_prosac.h")) in [os.path.realpath(d) for d in build.DEPS]


def test_python_argument_checks():
    """scores= with budgets= or priors=, a wrong string, a wrong shape or dtype: ValueError before any device work (no GPU here)"""
    import torch
    from mdrp_amd import poselib
    n = 8
    x1, x2, d1, d2 = [np.zeros((n, 2))] * 2, [np.zeros((n, 2))] * 2, [np.ones(n)] * 2, [np.ones(n)] * 2
    sc = [np.arange(n, dtype=np.float64)] * 2
    for fn, cams in ((poselib.estimate_monodepth_relative_pose_batch, (pcs.CAMERA, pcs.CAMERA)), (poselib.estimate_monodepth_shared_focal_relative_pose_batch, ()),
                     (poselib.estimate_monodepth_varying_focal_relative_pose_batch, ())):
        with pytest.raises(ValueError, match="scores do not combine"):
            fn(x1, x2, d1, d2, *cams, {"max_iterations": 20}, {}, budgets=[10, 20], scores=sc)
        with pytest.raises(ValueError, match="scores do not combine"):
            fn(x1, x2, d1, d2, *cams, {}, {}, priors=[None, None], scores="presorted")
        with pytest.raises(ValueError, match="presorted"):
            fn(x1, x2, d1, d2, *cams, {}, {}, scores="sorted")
        with pytest.raises(ValueError, match="expected 2 rows, got 1"):
            fn(x1, x2, d1, d2, *cams, {}, {}, scores=sc[:1])
        with pytest.raises(ValueError, match="pair 1 has 8 correspondences and 5 scores"):
            fn(x1, x2, d1, d2, *cams, {}, {}, scores=[sc[0], sc[1][:5]])
    with pytest.raises(ValueError, match="scores do not combine"):
        poselib.estimate_monodepth_shared_focal_relative_pose(x1[0], x2[0], d1[0], d2[0], {}, {}, prior=poselib.MonoDepthImagePair(
            poselib.MonoDepthTwoViewGeometry(poselib.CameraPose([1.0, 0, 0, 0], [0.0, 0.0, 1.0]), 1.0, 0.0, 0.0), poselib.Camera("SIMPLE_PINHOLE", [1.0, 0.0, 0.0]),
            poselib.Camera("SIMPLE_PINHOLE", [1.0, 0.0, 0.0])), scores=sc[0])
    t = [torch.zeros((2, n, 2), dtype=torch.float64), torch.zeros((2, n, 2), dtype=torch.float64), torch.ones((2, n), dtype=torch.float64), torch.ones((2, n), dtype=torch.float64)]
    with pytest.raises(ValueError, match="scores do not combine"):
        poselib.estimate_batch_torch("shared_focal", *t, ransac_opt={"max_iterations": 20}, budgets=[10, 20], scores=torch.zeros((2, n)))
    with pytest.raises(ValueError, match="scores do not combine"):
        poselib.estimate_batch_torch("shared_focal", *t, priors=torch.zeros((2, 12), dtype=torch.float64), scores="presorted")
    with pytest.raises(ValueError, match="float32 / float64"):
        poselib.estimate_batch_torch("shared_focal", *t, scores=torch.zeros((2, n), dtype=torch.int32))
    with pytest.raises(ValueError, match="float32 / float64"):
        poselib.estimate_batch_torch("shared_focal", *t, scores="sorted")
    with pytest.raises(ValueError, match="one per correspondence"):
        poselib.estimate_batch_torch("shared_focal", *t, scores=torch.zeros((2, n + 1)))
