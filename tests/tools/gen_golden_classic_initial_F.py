"""Writes tests/golden/classic_initial_F_ref.npz: the reference binary's estimate_fundamental called with a caller's matrix in *F (the Python
wrapper's initial_F), for tests/test_gpu_classic_initial_F.py.  Runs in the build container only (it needs the reference's PoseLib binary, as
oracle/build_ref.sh extracts it); builds its own shim, tests/tools/classic_initial_F_shim.cpp, into the git-ignored oracle/_ref/.

    python tests/tools/gen_golden_classic_initial_F.py [--check] [--probe]
        --check:  compare with the committed fixture instead of writing it
        --probe:  print, run by run, which reading of the caller's F reproduces the binary's record and write nothing

The probe.  Pairs in pixel coordinates around (800, 600) — a normalisation far from the identity —, N in {7, 8, 64, 300}; the matrix handed in is the
ground truth's F, a perturbed one, a random rank-2 matrix or the identity (the wrapper's "absent"); max_iterations in {0, 1, 100, 1000}; both values of
score_initial_model.  Each record of the binary is compared with three runs of the yardstick (tests/classic_models_ref.py): no prior, the F as a prior
converted into the estimator's normalised coordinates (prior_space = 0), the F as a prior taken as it stands in them (prior_space = 1).

Admission rule, as tests/tools/gen_golden_classic_prosac.py's: a run enters the fixture only if the reading the probe found (score_initial_model set:
prior_space = 0; not set: no prior, the matrix is not read) reproduces the binary's record on the CPU — LO count, iterations, inlier count, mask, F to
1e-6.  The pair of exactly seven records is one with a single real root of the 7-point cubic (classic_models_cases.FIRST says why).
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
import classic_models_cases as cc  # noqa: E402
import classic_models_ref as cm  # noqa: E402
from mdrp_amd import synth  # noqa: E402
from oracle import pyorc as po  # noqa: E402

SHIM = os.path.join(ROOT, "oracle", "_ref", "libclassic_initial_F_shim.so")
REF_SO = "/tmp/mdrp_ref_whl/poselib/_core.cpython-312-x86_64-linux-gnu.so"
OUT = os.path.join(ROOT, "tests", "golden", "classic_initial_F_ref.npz")
SIZES = (7, 8, 64, 300)
STARTS = ("exact", "perturbed", "garbage", "absent")
ITERATIONS = (0, 1, 100, 1000)
PP, FOCAL, THR, SEED, LOSS = (800.0, 600.0), 800.0, 2.0, 3, "TRUNCATED_CAUCHY"
PAIR_ID = {7: 92000, 8: 92100, 64: 92200, 300: 92300}  # first candidate per size; the seven-record pair moves on until it has one exact fit


def shim():
    subprocess.check_call([os.path.join(ROOT, "oracle", "build_ref.sh")])
    src = os.path.join(HERE, "classic_initial_F_shim.cpp")
    if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mavx", "-fPIC", "-shared", src, "-o", SHIM, "-Wl,--no-as-needed", "-lpython3.10", "-ldl"])
    C.CDLL("libpython3.10.so.1.0", mode=C.RTLD_GLOBAL)  # the reference binary's Py* data symbols
    lib = C.CDLL(SHIM)
    lib.fshim_init.argtypes = [C.c_char_p]
    if lib.fshim_init(REF_SO.encode()) != 0:
        raise RuntimeError("classic_initial_F_shim init failed")
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def reference(lib, x1, x2, F, mx, mn, si):
    ro = np.array([mx, mn, 3.0, 0.9999, 12.0, THR, SEED, float(si)], dtype=np.float64)
    bo = np.array([100, cc.LOSSES[LOSS], 1.0, 1e-10, 1e-8, 1e-3, 1e-10, 1e10], dtype=np.float64)
    F9 = np.ascontiguousarray(np.asarray(F, float).reshape(3, 3).T).reshape(-1).copy()  # the binary's F is column-major
    st, mask = np.zeros(5), np.zeros(len(x1), dtype=np.uint8)
    x1, x2 = np.ascontiguousarray(x1, dtype=np.float64), np.ascontiguousarray(x2, dtype=np.float64)
    lib.fshim_estimate(_p(x1), _p(x2), len(x1), _p(ro), _p(bo), _p(F9), _p(st), _p(mask))
    return F9.reshape(3, 3).T.reshape(-1).copy(), st, mask


def pair(n):
    pid = PAIR_ID[n]
    while True:
        p = synth.make_pair(pid, max(n, 8), f1=FOCAL, f2=FOCAL, pp=PP, noise_px=0.5, outlier_frac=0.3)
        x1, x2 = p["x1"][:n], p["x2"][:n]
        if n != 7:
            return pid, p, x1, x2
        q = cm.prep(cm.SEVEN, x1, x2, *cc.oracle_options(LOSS))
        if {len(cm.generate_models(cm.SEVEN, q["a1"], q["a2"], s)) for s in cm.draw_samples_k(SEED, 7, 7, 8)} == {1}:
            return pid, p, x1, x2
        pid += 1


def start(p, how, rng):
    if how == "absent":
        return np.eye(3).reshape(-1)
    return cc.start_model(cm.SEVEN, p, "identity" if how == "garbage" else how, rng)[:9]


def yardstick(x1, x2, F, mx, mn, si, reading):
    ro, bo = cc.oracle_options(LOSS, mx, mn, bool(si), SEED)
    prior = None if reading == "none" else np.r_[F, 0.0, 1.0, 1.0]
    return cm.estimate_from_prior_classic(cm.SEVEN, x1, x2, ro, bo, prior, prior_space=1 if reading == "space1" else 0)


def same(r, m, st, mask):
    return ((r["refinements"], r["iterations"], r["num_inliers"]) == tuple(int(v) for v in st[:3]) and np.array_equal(r["mask"], mask)
            and cc.model_diff(cm.SEVEN, r["model"], np.r_[m, 0.0, 1.0, 1.0]) < 1e-6)


def runs():
    """(size index, start index, max_iterations, min_iterations, score_initial_model): every size with every start, the iteration counts cycled so that
    each meets each size and each start, both values of the switch"""
    for a in range(len(SIZES)):
        for b in range(len(STARTS)):
            mx = ITERATIONS[(a + b) % 4]
            for si in (0, 1):
                yield a, b, mx, min(mx, 50), si


def main():
    lib = shim()
    probe = "--probe" in sys.argv
    out, rows = {}, []
    data = {}
    for a, n in enumerate(SIZES):
        pid, p, x1, x2 = pair(n)
        rng = np.random.default_rng(pid)
        data[a] = (p, x1, x2, [start(p, how, rng) for how in STARTS])
        out[f"x1_{a}"], out[f"x2_{a}"] = x1, x2
        out[f"F0_{a}"] = np.stack(data[a][3])
        print("N", n, "pair", pid)
    tally = {}
    for a, b, mx, mn, si in runs():
        p, x1, x2, Fs = data[a]
        m, st, mask = reference(lib, x1, x2, Fs[b], mx, mn, si)
        agree = [k for k in ("none", "space0", "space1") if same(yardstick(x1, x2, Fs[b], mx, mn, si, k), m, st, mask)]
        want = "space0" if si else "none"
        tally.setdefault((si, tuple(agree)), 0)
        tally[si, tuple(agree)] += 1
        print("N", SIZES[a], STARTS[b], "max_iterations", mx, "score_initial_model", si, "binary (LOs, iterations, inliers)", [int(v) for v in st[:3]],
              "reproduced by", agree, "" if want in agree else "NOT ADMITTED")
        if want not in agree:
            continue
        k = len(rows)
        rows.append((a, b, mx, mn, si))
        out[f"model_{k}"], out[f"stats_{k}"], out[f"mask_{k}"] = m, st, np.packbits(mask)
    print("readings that reproduce the binary, by score_initial_model:", tally)
    out["runs"] = np.array(rows, dtype=np.int64)
    out["options"] = np.array([THR, SEED, cc.LOSSES[LOSS]], dtype=np.float64)
    assert len(rows) >= 12
    if probe:
        return
    if "--check" in sys.argv:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out), "different arrays"
        for k in out:
            assert np.array_equal(old[k], out[k], equal_nan=True), k
        print("fixture unchanged")
        return
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(rows), "runs")


if __name__ == "__main__":
    main()
