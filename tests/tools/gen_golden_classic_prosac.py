"""Writes tests/golden/classic_prosac_ref.npz: the reference binary's PROSAC sampler tables for sample sizes 5, 6, 7 and its 5- / 6- / 7-point
estimators under progressive_sampling, for tests/test_classic_prosac_host.py and tests/test_gpu_classic_prosac.py.  Runs in the build container only
(it needs the reference's PoseLib binary, as oracle/build_ref.sh extracts it); builds its own shim, tests/tools/classic_prosac_shim.cpp, into the
git-ignored oracle/_ref/.

    python tests/tools/gen_golden_classic_prosac.py [--check] [--choose]
        --check:  compare with the committed fixture instead of writing it
        --choose: apply the admission rule from the first pair of every case on and print the DATA_ID table for tests/classic_prosac_cases.py

Admission rule: a case enters the fixture only if the CPU oracle's uniform run (po.estimate_classic) reproduces the reference's uniform record on the
same pre-sorted records (LO count, iterations, inlier count, mask, model to 1e-6).  A pair that fails is replaced by the pair 1000 ids on, and the
generator says so.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import classic_prosac_cases as ccs  # noqa: E402
from test_oracle_classic import fund_diff, pose_diff  # noqa: E402

SHIM = os.path.join(ROOT, "oracle", "_ref", "libclassic_prosac_shim.so")
REF_SO = "/tmp/mdrp_ref_whl/poselib/_core.cpython-312-x86_64-linux-gnu.so"
OUT = os.path.join(ROOT, "tests", "golden", "classic_prosac_ref.npz")

# (LO count, iterations, inliers) of the reference under progressive_sampling, as recorded when the cases were chosen: a regenerated fixture must show them
EXPECTED = {
    3: [(8, 400, 150), (4, 400, 150), (9, 1000, 300), (6, 71, 160), (14, 300, 68), (9, 2000, 1002)],
    4: [(8, 200, 152), (6, 200, 150), (6, 500, 302), (5, 88, 161), (5, 150, 68)],
    5: [(10, 400, 150), (5, 400, 152), (6, 1000, 301), (7, 113, 161), (9, 300, 68), (4, 2000, 1006)],
}


def shim():
    subprocess.check_call([os.path.join(ROOT, "oracle", "build_ref.sh")])  # (extracts the binary; builds oracle/_ref/librefshim.so beside ours)
    src = os.path.join(HERE, "classic_prosac_shim.cpp")
    if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mavx", "-fPIC", "-shared", src, "-o", SHIM, "-Wl,--no-as-needed", "-lpython3.10", "-ldl"])
    C.CDLL("libpython3.10.so.1.0", mode=C.RTLD_GLOBAL)  # the reference binary's Py* data symbols
    lib = C.CDLL(SHIM)
    lib.cshim_init.argtypes = [C.c_char_p]
    if lib.cshim_init(REF_SO.encode()) != 0:
        raise RuntimeError("classic_prosac_shim init failed")
    lib.cshim_sampler.argtypes = [C.c_size_t, C.c_size_t, C.c_ulong, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cshim_growth_len.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def sampler(lib, K, n, seed, max_prosac, count):
    growth = np.zeros(lib.cshim_growth_len(n, K, max_prosac), dtype=np.int64)
    samples, subset = np.zeros((count, K), dtype=np.int64), np.zeros(count, dtype=np.int64)
    lib.cshim_sampler(n, K, seed, max_prosac, count, _p(growth), _p(samples), _p(subset))
    return growth, samples, subset


def estimate(lib, kind, c, x1, x2, progressive):
    x1, x2 = np.ascontiguousarray(x1, dtype=np.float64), np.ascontiguousarray(x2, dtype=np.float64)
    cam = np.array([0, 1600, 1200, 3, ccs.FOCAL, 0.0, 0.0], dtype=np.float64)
    pp = np.zeros(2)
    ro = np.array([c["max_it"], c["min_it"], 3.0, 0.9999, 12.0, ccs.THRESHOLD, c["seed"], 1.0 if progressive else 0.0, c["max_prosac"]], dtype=np.float64)
    bo = np.array([100, 4, 1.0, 1e-10, 1e-8, 1e-3, 1e-10, 1e10], dtype=np.float64)  # TRUNCATED_CAUCHY
    model, st, mask = np.zeros(9), np.zeros(5), np.zeros(len(x1), dtype=np.uint8)
    lib.cshim_estimate(kind, _p(x1), _p(x2), len(x1), _p(cam), _p(cam), _p(pp), _p(ro), _p(bo), _p(model), _p(st), _p(mask))
    if kind == 5:
        model = np.ascontiguousarray(model.reshape(3, 3).T).reshape(-1)  # the binary's F is column-major; the fixture holds it row by row
    return model, st, mask


def oracle_agrees(kind, c, x1, x2, mu, stu, masku):
    """the admission rule: po.estimate_classic's uniform run against the reference's uniform record"""
    m, st, mask = ccs.oracle_run(kind, c, x1, x2)
    m = np.asarray(m, float).reshape(-1)
    if (st.refinements, st.iterations, st.num_inliers) != (int(stu[0]), int(stu[1]), int(stu[2])) or not np.array_equal(mask, masku):
        return False
    if kind == 5:
        return fund_diff(m[:9], mu) < 1e-6
    return pose_diff(m[:7], mu[:7]) < 1e-6 and (kind != 4 or abs(m[10] - mu[7]) < 1e-6 * abs(mu[7]))


def main():
    lib = shim()
    choose = "--choose" in sys.argv
    out, chosen, triples = {}, {}, {}
    for kind in ccs.KINDS:
        K = ccs.SAMPLE_SIZE[kind]
        for i, (n, seed, mp, count) in enumerate(ccs.sampler_rows(K)):
            growth, samples, subset = sampler(lib, K, n, seed, mp, count)
            assert growth.max() < 2 ** 31 and samples.max() < 65536 and samples.min() >= 0
            prog = np.arange(count) + 1 < mp  # the last index of a progressive sample is the subset's last record
            assert (samples[prog, K - 1] == subset[prog] - 1).all()
            out[f"growth_{K}_{i}"] = growth.astype(np.int32)
            out[f"samples_{K}_{i}"] = samples.astype(np.uint16)
            out[f"subset_{K}_{i}"] = subset.astype(np.uint16)
    for kind in ccs.KINDS:
        chosen[kind], triples[kind] = [], []
        for index in range(len(ccs.cases(kind))):
            did = 100 * kind + index if choose else ccs.DATA_ID[kind][index]
            while True:
                c = ccs.case(kind, index, did)
                x1, x2 = c["x1"][c["order"]], c["x2"][c["order"]]  # the reference runs on the pre-sorted records
                mu, stu, masku = estimate(lib, kind, c, x1, x2, False)
                if oracle_agrees(kind, c, x1, x2, mu, stu, masku):
                    break
                assert choose, f"kind {kind} case {index}: the oracle's uniform run does not reproduce the reference's on pair {did} (run with --choose)"
                print(f"kind {kind} case {index}: pair {did} is not admitted (oracle and reference differ under uniform sampling), replaced by pair {did + 1000}")
                did += 1000
                assert did < 10000, f"kind {kind} case {index}: no pair admitted"
            m, st, mask = estimate(lib, kind, c, x1, x2, True)
            got = (int(st[0]), int(st[1]), int(st[2]))
            print(kind, index, "pair", did, "prosac", got, "uniform", (int(stu[0]), int(stu[1]), int(stu[2])), "differ" if (m != mu).any() else "same")
            chosen[kind].append(did); triples[kind].append(got)
            t = f"{kind}_{index}"
            out["order_" + t] = c["order"].astype(np.uint16)
            out["digest_" + t] = np.frombuffer(ccs.digest(c), dtype=np.uint8)
            out["model_" + t], out["stats_" + t], out["mask_" + t] = m, st, np.packbits(mask)
            out["umodel_" + t], out["ustats_" + t], out["umask_" + t] = mu, stu, np.packbits(masku)
    if choose:
        print("DATA_ID =", {k: tuple(v) for k, v in chosen.items()})
        print("EXPECTED =", triples)
        return
    assert triples == EXPECTED, (triples, EXPECTED)
    if "--check" in sys.argv:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out), "different arrays"
        for k in out:
            assert np.array_equal(old[k], out[k], equal_nan=True), k
        print("fixture unchanged")
        return
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
