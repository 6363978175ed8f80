"""PROSAC on the 5- / 6- / 7-point baselines without a GPU: the NumPy definition with the sample size as a parameter (tests/classic_prosac_ref.py) and
the host part of mdrp_amd/csrc/mdrp_prosac.h against the reference binary's sampler tables for sample sizes 5, 6, 7
(tests/golden/classic_prosac_ref.npz, tests/tools/gen_golden_classic_prosac.py), and the header, the binding and the Python argument checks."""
import os
import re
import subprocess

import numpy as np
import pytest

import classic_prosac_cases as ccs
import classic_prosac_ref as cps
import prosac_ref as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (5, 6, 7)
ROWS = [(K, r) for K in SIZES for r in range(len(ccs.sampler_rows(K)))]


def test_sample_size_three_is_the_monodepth_definition():
    """K = 3 of the parameterised definition is tests/prosac_ref.py's, table and samples"""
    for n, seed, mp, count in ((3, 0, 100000, 50), (20, 0, 50, 60), (97, 2, 2, 100), (300, 3, 150, 400)):
        assert cps.growth(n, mp, 3) == ps.growth(n, mp)
        a, b = cps.samples(n, seed, mp, count, 3), ps.samples(n, seed, mp, count)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("K,row", ROWS)
def test_the_definition_draws_the_reference_samplers_tables(K, row):
    """growth table, subset size before every sample and every sample index, exactly"""
    n, seed, mp, count = ccs.sampler_rows(K)[row]
    g = ccs.golden()
    assert cps.growth(n, mp, K) == g[f"growth_{K}_{row}"].tolist()
    got, subs = cps.samples(n, seed, mp, count, K)
    assert got.shape == (count, K) and np.array_equal(got, g[f"samples_{K}_{row}"].astype(np.int64))
    assert np.array_equal(subs, g[f"subset_{K}_{row}"].astype(np.int64))
    prog = np.arange(count) + 1 < mp
    # K - 1 distinct records from the subset's head, then its last record
    assert (got[prog, K - 1] == subs[prog] - 1).all() and (got[prog, :K - 1] < (subs[prog] - 1)[:, None]).all()
    assert all(len(set(s)) == K for s in got.tolist())
    if count > mp > 1 and n > K:
        assert not (got[~prog, K - 1] == subs[~prog] - 1).all()  # (the uniform phase is not the progressive one continued)


def _run_host(exe):
    text = "".join(f"{n} {K} {mp} {count}\n" for K in SIZES for n, _, mp, count in ccs.sampler_rows(K))
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == 4 * len(ROWS)
    return {ROWS[r]: {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in lines[4 * r:4 * r + 4]} for r in range(len(ROWS))}


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """the stand-alone host program, built plainly and with the address and undefined-behaviour sanitizers: both runs' output"""
    d = tmp_path_factory.mktemp("classic_prosac_host")
    src = os.path.join(ROOT, "tests", "hostmath", "classic_prosac_host.cpp")
    plain, san = str(d / "plain"), str(d / "san")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", src, "-o", plain])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", san])
    out = _run_host(plain)
    assert _run_host(san) == out  # (a sanitizer report ends the run with a non-zero status: check=True)
    return out


@pytest.mark.parametrize("K,row", ROWS)
def test_the_headers_growth_table_and_schedule_are_the_reference_samplers(host_program, K, row):
    """mdrp_prosac.h compiled into a stand-alone host program (-Wall -Werror, and once under -fsanitize=address,undefined): growth table exactly; the
    subset size of every progressive sample is the reference's; the device's truncated table is that schedule up to the first subset equal to n"""
    n, seed, mp, count = ccs.sampler_rows(K)[row]
    g, out = ccs.golden(), host_program[(K, row)]
    assert out["growth"] == g[f"growth_{K}_{row}"].tolist()
    n_prog = min(count, max(mp - 1, 0))
    assert out["progressive"] == [max(mp - 1, 0)]
    assert out["subset"] == g[f"subset_{K}_{row}"][:n_prog].astype(np.int64).tolist() == (g[f"samples_{K}_{row}"][:n_prog, K - 1].astype(np.int64) + 1).tolist()
    t = out["truncated"]
    assert t == out["subset"][:len(t)] and all(v < n for v in t) and all(v == n for v in out["subset"][len(t):])
    if n_prog and n > K:
        assert len(t) > 0


def test_the_existing_host_program_prints_what_it_printed(tmp_path):
    """tests/hostmath/prosac_host.cpp, unchanged, compiles against the parameterised header and prints the K = 3 tables of the definition"""
    exe = str(tmp_path / "prosac_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostmath", "prosac_host.cpp"), "-o", exe])
    lines = subprocess.run([exe], input="97 150 300\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert [int(v) for v in lines[0].split()[1:]] == ps.growth(97, 150)
    assert [int(v) for v in lines[1].split()[1:]] == ps.samples(97, 0, 150, 300)[1][:149].tolist()


def _declaration(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, name
    return [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]


def test_header_and_binding_agree(tmp_path):
    """three new symbols within ABI 6; the header's argument lists, checked by a C compiler against the lists written out here, are the binding's"""
    from mdrp_amd import _capi, build
    main = open(os.path.join(ROOT, "include", "mdrp.h")).read()
    assert int(re.search(r"#define MDRP_ABI_VERSION (0x[0-9a-fA-F]+)", main).group(1), 16) == 6 == _capi.ABI_VERSION
    assert '#include "mdrp_classic_ranked.h"' in main  # (the C compile below goes through mdrp.h alone)
    hdr = open(os.path.join(ROOT, "include", "mdrp_classic_ranked.h")).read()
    assert os.path.realpath(os.path.join(ROOT, "include", "mdrp_classic_ranked.h")) in [os.path.realpath(d) for d in build.DEPS]
    head = "mdrp_handle *, int, {}const double *, const double *, const double *, int, int, const int32_t *, " \
           "const mdrp_camera *, const mdrp_camera *, const mdrp_ransac_opt *, const mdrp_bundle_opt *, "
    src = tmp_path / "abi.c"
    src.write_text('#include "mdrp.h"\n'
                   "typedef int (*blocking_t)(" + head.format("int, ") + "mdrp_result *, uint8_t *);\n"
                   "typedef int (*async_t)(" + head.format("") + "uint8_t *);\n"
                   "typedef int (*samples_t)(mdrp_handle *, uint64_t, int, int, uint64_t, const int32_t *, int, uint32_t *);\n"
                   "blocking_t a = mdrp_estimate_classic_ranked;\nasync_t b = mdrp_estimate_classic_ranked_async;\nsamples_t c = mdrp_prosac_samples_k;\n"
                   "_Static_assert(sizeof(mdrp_ransac_opt) == 88, \"mdrp_ransac_opt\");\n")
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "abi.o")], check=True)
    build.build()
    lib = _capi.load_library()
    assert lib.mdrp_abi_version() == 6
    for name, count in (("mdrp_estimate_classic_ranked", 15), ("mdrp_estimate_classic_ranked_async", 13), ("mdrp_prosac_samples_k", 8)):
        assert name in _capi.EXPORTS_CLASSIC_RANKED and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(_declaration(hdr, name)) == count, name
    # the extension header's export list is what the header declares, as tests/test_capi_load.py holds EXPORTS against mdrp.h
    assert sorted(_capi.EXPORTS_CLASSIC_RANKED) == sorted(set(re.findall(r"\b(mdrp_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))))
    assert not set(_capi.EXPORTS_CLASSIC_RANKED) & set(_capi.EXPORTS)
    for name in ("estimate_classic_ranked", "estimate_classic_ranked_device", "prosac_samples_k"):
        assert callable(getattr(_capi.Handle, name))


def test_python_argument_checks():
    """scores= with budgets=, a wrong string, a wrong row count, a wrong length or dtype: ValueError before any device work (no GPU here);
    progressive_sampling without scores stays refused"""
    import torch
    from mdrp_amd import poselib
    n = 8
    x1, x2 = [np.zeros((n, 2))] * 2, [np.zeros((n, 2))] * 2
    sc = [np.arange(n, dtype=np.float64)] * 2
    for fn, lead in ((poselib.estimate_relative_pose_batch, (ccs.CAMERA, ccs.CAMERA)), (poselib.estimate_shared_focal_relative_pose_batch, ((0.0, 0.0),)),
                     (poselib.estimate_fundamental_batch, ())):
        with pytest.raises(ValueError, match="scores do not combine"):
            fn(x1, x2, *lead, {"max_iterations": 20}, {}, budgets=[10, 20], scores=sc)
        with pytest.raises(ValueError, match="presorted"):
            fn(x1, x2, *lead, {}, {}, scores="sorted")
        with pytest.raises(ValueError, match="expected 2 rows, got 1"):
            fn(x1, x2, *lead, {}, {}, scores=sc[:1])
        with pytest.raises(ValueError, match="pair 1 has 8 correspondences and 5 scores"):
            fn(x1, x2, *lead, {"progressive_sampling": True}, {}, scores=[sc[0], sc[1][:5]])
        with pytest.raises(NotImplementedError, match="scores"):
            fn(x1, x2, *lead, {"progressive_sampling": True}, {})
        for wrong in ([sc[0], ["high"] * n], [sc[0], np.array([object()] * n, dtype=object)], [sc[0], sc[1].astype(np.complex128) + 1j]):  # a wrong dtype
            with pytest.raises((ValueError, TypeError)):
                fn(x1, x2, *lead, {}, {}, scores=wrong)
    with pytest.raises(ValueError, match="presorted"):
        poselib.estimate_fundamental(x1[0], x2[0], {}, {}, scores="sorted")
    with pytest.raises((ValueError, TypeError)):
        poselib.estimate_fundamental(x1[0], x2[0], {}, {}, scores=["high"] * n)
    with pytest.raises(ValueError, match="pair 0 has 8 correspondences and 5 scores"):
        poselib.estimate_relative_pose(x1[0], x2[0], ccs.CAMERA, ccs.CAMERA, {}, {}, scores=sc[0][:5])
    with pytest.raises(ValueError, match="pair 0 has 8 correspondences and 5 scores"):
        poselib.estimate_shared_focal_relative_pose(x1[0], x2[0], (0.0, 0.0), {}, {}, scores=sc[0][:5])
    t = [torch.zeros((2, n, 2), dtype=torch.float64), torch.zeros((2, n, 2), dtype=torch.float64)]
    for kind in ("relpose_5pt", "shared_focal_6pt", "fundamental_7pt"):
        with pytest.raises(ValueError, match="float32 / float64"):
            poselib.estimate_baseline_batch_torch(kind, *t, ccs.CAMERA, ccs.CAMERA, scores=torch.zeros((2, n), dtype=torch.int32))
        with pytest.raises(ValueError, match="presorted"):
            poselib.estimate_baseline_batch_torch(kind, *t, ccs.CAMERA, ccs.CAMERA, scores="sorted")
        with pytest.raises(ValueError, match="one per correspondence"):
            poselib.estimate_baseline_batch_torch(kind, *t, ccs.CAMERA, ccs.CAMERA, scores=torch.zeros((2, n + 1)))
        with pytest.raises(ValueError, match="one per correspondence"):
            poselib.estimate_baseline_batch_torch(kind, *t, ccs.CAMERA, ccs.CAMERA, scores=torch.zeros((1, n)))
        with pytest.raises(NotImplementedError, match="scores"):
            poselib.estimate_baseline_batch_torch(kind, *t, ccs.CAMERA, ccs.CAMERA, ransac_opt={"progressive_sampling": True})
    with pytest.raises(ValueError, match="kind"):
        poselib.estimate_baseline_batch_torch("calibrated", *t, scores="presorted")
    with pytest.raises(ValueError, match="kind"):
        poselib.estimate_baseline_batch_torch(5, *t, scores="presorted")
    # malformed points are reported as such, not as a score error
    with pytest.raises(ValueError, match=r"\(B, N, 2\)"):
        poselib.estimate_baseline_batch_torch("fundamental_7pt", torch.zeros((2, n), dtype=torch.float64), t[1], scores=torch.zeros((2, n)))
    with pytest.raises(ValueError, match="tensors"):
        poselib.estimate_baseline_batch_torch("fundamental_7pt", np.zeros((2, n, 2)), np.zeros((2, n, 2)), scores=torch.zeros((2, n)))


@pytest.mark.parametrize("K", SIZES)
def test_the_baselines_sampler_kernels_have_no_spill_and_no_scratch(K):
    """kc_samples_prosac<K> in the built library's code objects, as tests/test_prosac_resources.py reads k_samples_prosac: one instantiation per K"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from mdrp_amd import build
    import kernel_table
    build.build()
    regs = kernel_table.kernel_table()
    r = regs[f"mdrp::kc_samples_prosac<{K}>"]
    assert r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0 and r.get("scratch", 0) == 0 and r["lds"] <= 1024, (K, r)


def test_every_entry_point_of_the_extension_header_is_in_its_history_table():
    """tests/test_history_host.py's rule for include/mdrp_classic_ranked.h: every function with a handle is run by tests/classic_history_cases.py,
    whose inputs are deterministic"""
    import classic_history_cases as chc
    import helpers
    import history_cases as hc
    named = {p for c in chc.probes() for p in c.entry_points}
    assert set(chc.extension_entry_points()) == {"mdrp_estimate_classic_ranked", "mdrp_estimate_classic_ranked_async", "mdrp_prosac_samples_k"} <= named
    assert {c.kind for c in chc.probes() if c.family == "ranked"} == {3, 4, 5} and {c.device for c in chc.probes() if c.family == "ranked"} == {False, True}
    assert not {c.name for c in chc.probes()} & {c.name for c in hc.predecessors()}
    for c in chc.probes() + tuple(x for pair in chc.back_to_back() for x in pair):
        a, b = (helpers.input_digest(hc.four(c.digest_arrays(c.make()))) for _ in range(2))
        assert a == b, c
