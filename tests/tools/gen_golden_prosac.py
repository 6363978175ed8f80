"""Writes tests/golden/prosac_ref.npz: the reference binary's PROSAC sampler tables and its estimators under progressive_sampling, for
tests/test_prosac_host.py and tests/test_gpu_prosac.py.  Runs in the build container only (it needs the reference's PoseLib binary, as
oracle/build_ref.sh extracts it); builds its own shim, tests/tools/prosac_shim.cpp, into the git-ignored oracle/_ref/.

    python tests/tools/gen_golden_prosac.py [--check]      (--check: compare with the committed fixture instead of writing it)
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
import prosac_cases as pcs  # noqa: E402

SHIM = os.path.join(ROOT, "oracle", "_ref", "libprosac_shim.so")
REF_SO = "/tmp/mdrp_ref_whl/poselib/_core.cpython-312-x86_64-linux-gnu.so"
OUT = os.path.join(ROOT, "tests", "golden", "prosac_ref.npz")

# (LO count, iterations, inliers) of the reference under progressive_sampling, as recorded when the cases were chosen: a regenerated fixture must show them
EXPECTED = {
    0: [(10, 400, 150), (8, 400, 150), (8, 1000, 301), (5, 39, 161), (7, 2000, 1006), (10, 1500, 1003), (8, 300, 68), (2, 115, 78), (8, 419, 200)],
    1: [(8, 400, 151), (11, 400, 150), (6, 1000, 303), (4, 40, 160), (14, 2000, 1009), (9, 1500, 1006), (10, 300, 68), (7, 115, 78), (10, 394, 204)],
    2: [(7, 400, 134), (2, 400, 149), (5, 1000, 282), (5, 118, 119), (9, 2000, 940), (9, 1500, 991), (8, 300, 57), (11, 150, 72), (8, 580, 180)],
}


def shim():
    subprocess.check_call([os.path.join(ROOT, "oracle", "build_ref.sh")])  # (extracts the binary; builds oracle/_ref/librefshim.so beside ours)
    src = os.path.join(HERE, "prosac_shim.cpp")
    if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mavx", "-fPIC", "-shared", src, "-o", SHIM, "-Wl,--no-as-needed", "-lpython3.10", "-ldl"])
    C.CDLL("libpython3.10.so.1.0", mode=C.RTLD_GLOBAL)  # the reference binary's Py* data symbols
    lib = C.CDLL(SHIM)
    lib.pshim_init.argtypes = [C.c_char_p]
    if lib.pshim_init(REF_SO.encode()) != 0:
        raise RuntimeError("prosac_shim init failed")
    lib.pshim_sampler.argtypes = [C.c_size_t, C.c_ulong, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pshim_growth_len.argtypes = [C.c_size_t, C.c_size_t]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def sampler(lib, n, seed, max_prosac, count):
    growth = np.zeros(lib.pshim_growth_len(n, max_prosac), dtype=np.int64)
    samples, subset = np.zeros((count, 3), dtype=np.int64), np.zeros(count, dtype=np.int64)
    lib.pshim_sampler(n, seed, max_prosac, count, _p(growth), _p(samples), _p(subset))
    return growth, samples, subset


def estimate(lib, kind, c, progressive):
    x1, x2, d1, d2 = (np.ascontiguousarray(c[k], dtype=np.float64) for k in ("x1", "x2", "d1", "d2"))
    cam = np.array([0, 1600, 1200, 3, pcs.FOCAL, 0.0, 0.0], dtype=np.float64)
    ro = np.array([c["max_it"], c["min_it"], pcs.RO["dyn_num_trials_mult"], pcs.RO["success_prob"], pcs.RO["max_reproj_error"], pcs.RO["max_epipolar_error"],
                   c["seed"], c["shift"], pcs.RO["monodepth_weight_sampson"], 1.0 if progressive else 0.0, c["max_prosac"]], dtype=np.float64)
    bo = np.array([100, 4, 1.0, 1e-10, 1e-8, 1e-3, 1e-10, 1e10], dtype=np.float64)  # TRUNCATED_CAUCHY
    model, st, mask = np.zeros(12), np.zeros(5), np.zeros(len(x1), dtype=np.uint8)
    lib.pshim_estimate(kind, _p(x1), _p(x2), _p(d1), _p(d2), len(x1), _p(cam), _p(cam), _p(ro), _p(bo), _p(model), _p(st), _p(mask))
    return model, st, mask


def main():
    lib = shim()
    out = {}
    for i, (n, seed, mp, count) in enumerate(pcs.SAMPLER_ROWS):
        growth, samples, subset = sampler(lib, n, seed, mp, count)
        assert growth.max() < 2 ** 31 and samples.max() < 65536 and samples.min() >= 0
        # the third index of a progressive sample is the subset's last record
        prog = np.arange(count) + 1 < mp
        assert (samples[prog, 2] == subset[prog] - 1).all()
        out[f"growth_{i}"] = growth.astype(np.int32)
        out[f"samples_{i}"] = samples.astype(np.uint16)
    for kind in (0, 1, 2):
        for case in range(len(pcs.CASES)):
            c = pcs.case(kind, case)
            s = dict(c)
            s.update({k: c[k][c["order"]] for k in ("x1", "x2", "d1", "d2")})  # the reference runs on the pre-sorted records
            m, st, mask = estimate(lib, kind, s, True)
            mu, stu, masku = estimate(lib, kind, s, False)
            got = (int(st[0]), int(st[1]), int(st[2]))
            print(kind, case, "prosac", got, "uniform", (int(stu[0]), int(stu[1]), int(stu[2])), "differ" if (m != mu).any() else "same")
            assert got == EXPECTED[kind][case], (kind, case, got, EXPECTED[kind][case])
            t = f"{kind}_{case}"
            out["order_" + t] = c["order"].astype(np.uint16)
            out["digest_" + t] = np.frombuffer(pcs.digest(c), dtype=np.uint8)
            out["model_" + t], out["stats_" + t], out["mask_" + t] = m, st, np.packbits(mask)
            out["umodel_" + t], out["ustats_" + t], out["umask_" + t] = mu, stu, np.packbits(masku)
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
