"""Writes tests/golden/classic_focals_ref.npz: the reference binary's poselib::focals_from_fundamental(F, pp1, pp2) on random rank-2 matrices, for
tests/test_classic_focals_host.py and tests/test_gpu_classic_focals.py.  Runs in the build container only (it needs the reference's PoseLib binary, as
oracle/build_ref.sh extracts it); builds its own shim, tests/tools/classic_focals_shim.cpp, into the git-ignored oracle/_ref/.

    python tests/tools/gen_golden_classic_focals.py [--check] [--probe]
        --check:  compare with the committed fixture instead of writing it
        --probe:  the same comparison on 3000 draws, printed and not written

The draws (tests/classic_focals_ref.py random_F): f in U(300, 2000) per camera, rotation vector N(0, 0.3^2), t ~ N(0, 0.5^2), F = K2^-T [t]x R K1^-1
with K = diag(f, f, 1) and every entry multiplied by 1 + 10^U(-7,-3) N(0, 1), the rank restored by an SVD, unit Frobenius norm; the principal
points handed to the formula are drawn on their own, pp ~ N(0, 20^2) per image (which is what makes f^2 negative for some draws), and are (0, 0) for
every fourth draw.

Admission rule: a matrix enters only if the NumPy restatement with cross-product null vectors and the one with SVD null vectors agree on the sign of
both f^2 and, where the focal is real, on f to 1e-8 relative: a draw the two disagree on is one whose answer depends on how the epipole was computed,
and pins nothing.  The rule may reject at most 10 % of the draws (asserted); it rejected none of the 400 of the fixture and none of the probe's 3000.

What the binary returns: two SIMPLE_PINHOLE cameras [f, ppx, ppy] with width = height = -1 (asserted for every draw), the principal points handed
in, and a NaN focal exactly where the restatement's f^2 is negative (asserted: NaN positions match on every admitted draw).

Measured on the fixture (400 matrices, 800 focals, 27 of them NaN): the largest relative deviation of the NumPy restatement
(cross-product null vectors) from the binary is 6.91e-10 (99th percentile 2.9e-11, median 1.7e-14); the probe's 3000 draws (184 NaN of 6000) give
6.27e-10.  The tests allow 10 x the fixture's value = 6.91e-9 (the fixture carries both numbers, `measured_max_rel` and `tolerance`); the headroom is
for FMA contraction on the device under the same conditioning.
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
import classic_focals_ref as fr  # noqa: E402

SHIM = os.path.join(ROOT, "oracle", "_ref", "libclassic_focals_shim.so")
REF_SO = "/tmp/mdrp_ref_whl/poselib/_core.cpython-312-x86_64-linux-gnu.so"
OUT = os.path.join(ROOT, "tests", "golden", "classic_focals_ref.npz")
SEED, COUNT, PROBE_COUNT = 20260117, 400, 3000


def shim():
    subprocess.check_call([os.path.join(ROOT, "oracle", "build_ref.sh")])
    src = os.path.join(HERE, "classic_focals_shim.cpp")
    if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mavx", "-fPIC", "-shared", src, "-o", SHIM, "-Wl,--no-as-needed", "-lpython3.10", "-ldl"])
    C.CDLL("libpython3.10.so.1.0", mode=C.RTLD_GLOBAL)  # the reference binary's Py* data symbols
    lib = C.CDLL(SHIM)
    lib.focshim_init.argtypes = [C.c_char_p]
    if lib.focshim_init(REF_SO.encode()) != 0:
        raise RuntimeError("classic_focals_shim init failed")
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def reference(lib, F, pp1, pp2):
    """the binary's (f1, f2) [count][2]; asserts the shape of the cameras it returns"""
    F, pp1, pp2 = (np.ascontiguousarray(a, dtype=np.float64) for a in (F, pp1, pp2))
    cams = np.zeros((len(F), 2, 6))
    odd = lib.focshim_focals(_p(F), _p(pp1), _p(pp2), len(F), _p(cams))
    assert odd == 0, "a camera without three parameters"
    assert (cams[:, :, 0] == 0).all() and (cams[:, :, 1] == -1).all() and (cams[:, :, 2] == -1).all(), "SIMPLE_PINHOLE with width = height = -1"
    assert np.array_equal(cams[:, 0, 4:6], pp1) and np.array_equal(cams[:, 1, 4:6], pp2), "the principal points handed in"
    return cams[:, :, 3].copy()


def draws(count, seed):
    rng = np.random.default_rng(seed)
    F, a, b = np.zeros((count, 9)), np.zeros((count, 2)), np.zeros((count, 2))
    for i in range(count):
        F[i], a[i], b[i] = fr.random_F(rng, pp_sigma=0.0 if i % 4 == 3 else 20.0)
    return F, a, b


def admitted(F, pp1, pp2):
    sc, ss = fr.focals_squared(F, pp1, pp2, fr.null_cross), fr.focals_squared(F, pp1, pp2, fr.null_svd)
    for c, s in zip(sc, ss):
        if not (np.isfinite(c) and np.isfinite(s)) or (c < 0) != (s < 0):
            return False
        if c >= 0 and abs(np.sqrt(c) - np.sqrt(s)) > 1e-8 * np.sqrt(s):
            return False
    return True


def compare(lib, count, seed):
    F, pp1, pp2 = draws(count, seed)
    keep = np.array([admitted(F[i], pp1[i], pp2[i]) for i in range(count)])
    print("draws", count, "rejected by the admission rule", int((~keep).sum()))
    assert (~keep).sum() <= count // 10, "the admission rule rejects more than 10 % of the draws"
    F, pp1, pp2 = F[keep], pp1[keep], pp2[keep]
    ref = reference(lib, F, pp1, pp2)
    mine = np.array([fr.focals(F[i], pp1[i], pp2[i]) for i in range(len(F))])
    assert np.array_equal(np.isnan(ref), np.isnan(mine)), "NaN positions differ"
    real = ~np.isnan(ref)
    rel = np.abs(mine[real] - ref[real]) / np.abs(ref[real])
    print("focals", ref.size, "NaN", int((~real).sum()), "of them with pp = 0:", int((~real)[(pp1 == 0).all(axis=1)].sum()))
    print("relative deviation of the restatement from the binary: max %.3g  p99 %.3g  median %.3g" % (rel.max(), np.percentile(rel, 99), np.median(rel)))
    return F, pp1, pp2, ref, float(rel.max())


def main():
    lib = shim()
    if "--probe" in sys.argv:
        compare(lib, PROBE_COUNT, SEED + 1)
        return
    F, pp1, pp2, ref, worst = compare(lib, COUNT, SEED)
    assert np.isnan(ref).sum() >= 10 and (pp1 == 0).all(axis=1).any()
    out = {"F": F, "pp1": pp1, "pp2": pp2, "f": ref, "measured_max_rel": np.array(worst), "tolerance": np.array(10.0 * worst)}
    if "--check" in sys.argv:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out), "different arrays"
        for k in out:
            assert np.array_equal(old[k], out[k], equal_nan=True), k
        print("fixture unchanged")
        return
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(F), "matrices, tolerance", 10.0 * worst)


if __name__ == "__main__":
    main()
