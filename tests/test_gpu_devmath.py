"""The device branches of mdrp_math.h's numeric primitives against mpmath (tests/devmath/devmath.hip: one element-wise kernel per primitive,
compiled here with the library's flags).  tests/test_hostmath.py only reaches the header's host branch; these are the hardware seeds with
their Newton steps, the LDS-table log1p of the Cauchy losses, the FAST cubic and the quartic built on it, and the rsqrt Cholesky of the LM.
References: mpmath at 120 bits, rounded to fp64; errors in ulps of the correctly rounded result (or, for the polynomial and linear solvers,
in units of eps times the problem's scale).  Each contract is the bound the header's comment states on the domain it states."""
import ctypes as C
import math
import os
import subprocess

import mpmath
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "devmath", "devmath.hip")
EPS = 2.0 ** -52
DMIN = 2.0 ** -1022                                  # DBL_MIN
DMAX = np.finfo(np.float64).max
SUB_MIN, SUB_MAX = 2.0 ** -1074, DMIN - 2.0 ** -1074  # smallest / largest subnormal
PREC = 120
OPS = {"sv_rcp": 0, "sv_div": 1, "sv_rsqrt": 2, "sv_sqrt": 3, "lm_rcp": 4, "lm_rsqrt": 5, "lm_log1p": 6, "loss3": 7, "loss4": 8}
dp = C.POINTER(C.c_double)


def compile_probe(out_dir):
    from mdrp_amd import build
    so = os.path.join(str(out_dir), "libdevmath.so")
    subprocess.check_call([build.hipcc(), *build.FLAGS, SRC, "-o", so])
    return so


def test_probe_compiles(tmp_path):
    """(no GPU) the probe builds against the current header: a change of a primitive's signature or of the log table's layout fails here"""
    import sys
    sys.path.insert(0, os.path.join(HERE, "..", "tools"))
    import kernel_table
    so = compile_probe(tmp_path)
    syms = subprocess.run([kernel_table._tool("llvm-readelf"), "--dyn-syms", so], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and " UND " not in ln}
    assert {"dm_unary", "dm_cubic", "dm_quartic", "dm_chol", "dm_cubic_host", "dm_quartic_host"} <= defined, defined


_LIB = {}


def _child_call(so, fname, ints, arrays, out_shape, n):
    """runs in the probe's child process: one launcher call on host arrays -> (return code, output array)"""
    if so not in _LIB:
        from mdrp_amd import _capi
        _capi._ensure_hip_runtime()                  # the probe is linked like the library (-no-hip-rt): it binds to this process's runtime
        _LIB[so] = C.CDLL(so)
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
    out = np.zeros(out_shape)
    rc = getattr(_LIB[so], fname)(*[C.c_int(int(i)) for i in ints], *[a.ctypes.data_as(dp) for a in arrays], out.ctypes.data_as(dp), C.c_int(n))
    return rc, out


class Probe:
    """the probe library in a child process of its own: the pytest process keeps no device state of it (code object, queues, buffers)"""

    def __init__(self, so):
        import multiprocessing
        from concurrent.futures import ProcessPoolExecutor
        self.so = so
        self.pool = ProcessPoolExecutor(max_workers=1, mp_context=multiprocessing.get_context("spawn"))

    def call(self, fname, ints, arrays, out_shape, n):
        return self.pool.submit(_child_call, self.so, fname, ints, arrays, out_shape, n).result(timeout=300)

    def close(self):
        self.pool.shutdown()


@pytest.fixture(scope="module")
def dm(tmp_path_factory):
    probe = Probe(compile_probe(tmp_path_factory.mktemp("devmath")))
    yield probe
    probe.close()


def run_unary(dm, op, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b if b is not None else a, dtype=np.float64)
    rc, out = dm.call("dm_unary", [OPS[op]], [a, b], a.shape, len(a))
    assert rc == 0
    return out


# ---------------------------------------------------------------- inputs
def pow2_neighbours(lo=-1022, hi=1023):
    """every power of two in [2^lo, 2^hi] and its two 1-ulp neighbours"""
    p = np.ldexp(1.0, np.arange(lo, hi + 1))
    return np.concatenate([p, np.nextafter(p, 0.0), np.nextafter(p, np.inf)])


def log_uniform(rng, n, lo, hi):
    """|x| log-uniform over [2^lo, 2^hi)"""
    return np.ldexp(1.0 + rng.random(n), rng.integers(lo, hi, n))


def positive_sweep(seed, n=3000, lo=-1022, hi=1023):
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([log_uniform(rng, n, lo, hi), pow2_neighbours(lo, hi - 1), [DMIN, DMAX, 1.0, 2.0, 3.0]]))


SPECIALS = np.array([0.0, -0.0, SUB_MIN, SUB_MAX, DMIN, DMAX, np.inf, -np.inf, np.nan, -1.0])


# ---------------------------------------------------------------- error measures
def ulps(got, exact):
    """|got - exact| / ulp(fl(exact)) per element (exact: mpf list); inf where got is not finite but exact is"""
    out = np.empty(len(got))
    for i, (g, e) in enumerate(zip(got, exact)):
        r = float(e)
        if not math.isfinite(g):
            out[i] = 0.0 if g == r else np.inf
            continue
        u = np.spacing(abs(r)) if r != 0.0 else SUB_MIN
        out[i] = float(abs(mpmath.mpf(g) - e)) / u
    return out


def _ref(fn, *cols):
    with mpmath.workprec(PREC):
        return [fn(*(mpmath.mpf(float(c)) for c in row)) for row in zip(*cols)]


UNARY_REF = {
    "sv_rcp": lambda x: 1 / x, "lm_rcp": lambda x: 1 / x,
    "sv_rsqrt": lambda x: 1 / mpmath.sqrt(x), "lm_rsqrt": lambda x: 1 / mpmath.sqrt(x),
    "sv_sqrt": mpmath.sqrt, "lm_log1p": mpmath.log1p,
}

# the header's bound on the header's domain (mdrp_math.h: sv_* and lm_rsqrt "<= 1.5 ulp", lm_rcp "<= 1 ulp", the Heron correction of sv_sqrt
# "<= 1 ulp" — every normal argument, both signs for the reciprocals —, lm_log1p "<= 2 ulp for every finite x >= 0", subnormals included)
UNARY_BOUND = {"sv_rcp": 1.5, "lm_rcp": 1.0, "sv_rsqrt": 1.5, "lm_rsqrt": 1.5, "sv_sqrt": 1.0, "lm_log1p": 2.0}


def unary_domain(op, seed):
    if op in ("sv_rcp", "lm_rcp"):
        x = positive_sweep(seed)
        return np.concatenate([x, -x[::7]])
    if op in ("sv_rsqrt", "lm_rsqrt", "sv_sqrt"):
        return positive_sweep(seed)
    rng = np.random.default_rng(seed)                # lm_log1p: all finite x >= 0, subnormals included, and where 1 + x rounds
    cells = 1.0 + np.arange(129) / 128.0
    cells = np.concatenate([cells, np.nextafter(cells, 0.0), np.nextafter(cells, 9.0)]) - 1.0
    near = np.concatenate([np.ldexp(1.0, k) * np.array([1.0, 1.0 - EPS / 2, 1.0 + EPS, 0.75, 1.5]) for k in (-8, -9, -52, -53, -54)])
    x = np.unique(np.concatenate([positive_sweep(seed), log_uniform(rng, 3000, -60, 3), log_uniform(rng, 300, -1074, -1022), cells, near,
                                  [0.0, SUB_MIN, SUB_MAX, 1e-4, 1e-8, 1e-12, 1e-16]]))
    return x[x >= 0.0]


def measure_unary(dm, op, seed=1):
    x = unary_domain(op, seed)
    got = run_unary(dm, op, x)
    err = ulps(got, _ref(UNARY_REF[op], x))
    return x, got, err


def measure_div(dm, seed=2):
    rng = np.random.default_rng(seed)
    a = log_uniform(rng, 4000, -500, 500) * rng.choice([-1.0, 1.0], 4000)
    b = log_uniform(rng, 4000, -500, 500) * rng.choice([-1.0, 1.0], 4000)
    got = run_unary(dm, "sv_div", a, b)
    return a, b, got, ulps(got, _ref(lambda p, q: p / q, a, b))


def loss_inputs(seed=3):
    """thr over 1e-150 .. 1e150; r2 = 0, r2 around t2 (the truncation point of loss 4), far below and far above t2"""
    rng = np.random.default_rng(seed)
    thr = 10.0 ** rng.uniform(-150, 150, 600)
    thr = np.concatenate([thr, [1e-150, 1e150, 1.0, 0.5, 2.0, 1e-3]])
    t2 = thr * thr
    rel = np.concatenate([[0.0, 1e-300, 1e-20, 1e-12, 1e-8, 1e-4, 2.0 ** -8, 0.01, 0.3, 1.0, 3.0, 1e3, 1e12, 1e40]])
    T, R = np.meshgrid(thr, rel, indexing="ij")
    with np.errstate(over="ignore"):
        thr_all, r2 = T.ravel(), (R * (T * T)).ravel()                  # (r2 = inf where 1e40 t2 overflows: loss 4 is then t2 ln 2)
    near = np.concatenate([np.nextafter(t2, 0.0), t2, np.nextafter(t2, np.inf)])
    return np.concatenate([thr_all, np.tile(thr, 3)]), np.concatenate([r2, near])


def loss_ref(kind):
    def f(thr, r2):
        t2 = mpmath.mpf(float(np.float64(float(thr)) * np.float64(float(thr))))  # t2 as the function forms it: fl(thr * thr)
        x = (mpmath.mpf(min(float(r2), float(t2))) if kind == 4 else r2) / t2
        return t2 * mpmath.log1p(x)
    return f


def measure_loss(dm, kind):
    thr, r2 = loss_inputs()
    got = run_unary(dm, f"loss{kind}", thr, r2)
    return thr, r2, got, ulps(got, _ref(loss_ref(kind), thr, r2))


# ---------------------------------------------------------------- polynomials
def run_poly(dm, degree, coef, device=True):
    """device: "fast" (cubic only), True (the device's IEEE branch / the quartic) or False (the header's host build, on the CPU)"""
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    n = len(coef)
    if not device:
        return dm.call(f"dm_{'cubic' if degree == 3 else 'quartic'}_host", [], [coef], (n, degree + 1), n)[1]
    ints = [1 if device == "fast" else 0] if degree == 3 else []
    rc, out = dm.call("dm_cubic" if degree == 3 else "dm_quartic", ints, [coef], (n, degree + 1), n)
    assert rc == 0
    return out


def cubic_inputs(seed=4):
    """monic cubics from their roots (x - r0)(x - r1)(x - r2), rounded to fp64 coefficients: well separated roots, two nearly coinciding
    (discriminant just below zero: arg near +-1, where A&S 4.4.46 is least accurate and Newton converges only linearly), a triple root,
    one real root; root scales 1e-8 .. 1e8"""
    rng = np.random.default_rng(seed)
    rows, tags = [], []
    for s in 10.0 ** np.arange(-8, 9, 2, dtype=np.float64):
        for _ in range(20):
            rows.append(s * (np.array([-1.0, -0.2, 0.6]) + 0.4 * rng.random(3)) * rng.choice([-1.0, 1.0])); tags.append("separated")
            m = rng.uniform(-1, 1) * s
            d = s * 10.0 ** rng.uniform(-7, -2)
            rows.append(np.array([m - d, m + d * rng.uniform(0.5, 2), rng.uniform(-1, 1) * s])); tags.append("near_double")
            rows.append(np.array([m + d, m, m - d * 0.5])); tags.append("cluster")
        rows.append(np.array([s, s, s])); tags.append("triple")
        rows.append(np.array([-s / 3, -s / 3, -s / 3])); tags.append("triple")
    coef = [(-(r[0] + r[1] + r[2]), r[0] * r[1] + r[1] * r[2] + r[0] * r[2], -r[0] * r[1] * r[2]) for r in rows]
    # one real root and a complex pair: x^3 + c x + d with c > 0
    for s in 10.0 ** np.arange(-8, 9, 2, dtype=np.float64):
        for _ in range(10):
            a, w = rng.uniform(-1, 1) * s, rng.uniform(0.1, 1) * s
            coef.append((-a, w * w, -a * w * w)); tags.append("one_real")   # (x - a)(x^2 + w^2)
    return np.array(coef, dtype=np.float64), tags


def quartic_inputs(seed=5):
    rng = np.random.default_rng(seed)
    coef, tags = [], []
    for s in 10.0 ** np.arange(-4, 5, 1, dtype=np.float64):
        for _ in range(25):
            r = rng.uniform(-1, 1, 4) * s
            tags.append("four_real")
            if rng.random() < 0.3:
                r[1] = r[0] + s * 10.0 ** rng.uniform(-7, -3); tags[-1] = "near_double"
            coef.append(np.poly(r)[1:])
            a, w = rng.uniform(-1, 1, 2) * s, rng.uniform(0.1, 1) * s    # two real roots, one complex pair
            coef.append(np.poly([a[0], a[1], complex(a[0], w), complex(a[0], -w)]).real[1:]); tags.append("two_real")
    return np.array(coef, dtype=np.float64), tags


def exact_roots(coef):
    with mpmath.workprec(PREC):
        out = []
        for c in coef:
            rs = mpmath.polyroots([1] + [mpmath.mpf(float(v)) for v in c], maxsteps=400, extraprec=4 * PREC)
            out.append([complex(r) for r in rs])
    return out


def conditioning_floor(coef, exact, seed=7, rel=4 * EPS):
    """how far the exact roots move when every coefficient is perturbed by `rel` relative (two random sign patterns), in units of eps times
    the root scale: the error a backward-stable solver may have.  Large near multiple roots (~eps^(1/m) for multiplicity m)."""
    rng = np.random.default_rng(seed)
    out = np.zeros(len(coef))
    with mpmath.workprec(PREC):
        for i, (c, ex) in enumerate(zip(coef, exact)):
            scale = max(max(abs(r) for r in ex), 1e-300)
            for _ in range(2):
                cp = [1] + [mpmath.mpf(float(v)) * (1 + rel * rng.choice([-1, 1])) for v in c]
                rs = [complex(r) for r in mpmath.polyroots(cp, maxsteps=400, extraprec=4 * PREC)]
                out[i] = max(out[i], max(min(abs(r - q) for q in rs) for r in ex) / (EPS * scale))
    return out


def root_error(got, valid, exact):
    """max over the returned roots of the distance to the nearest exact root, in units of eps * (max |exact root| or 1e-300)"""
    scale = max(max(abs(r) for r in exact), 1e-300)
    e = 0.0
    for k, g in enumerate(got):
        if valid[k]:
            if not math.isfinite(g):
                return np.inf
            e = max(e, min(abs(g - r) for r in exact))
    return e / (EPS * scale)


def measure_cubic(dm):
    coef, tags = cubic_inputs()
    exact = exact_roots(coef)
    res = {"floor": conditioning_floor(coef, exact)}
    for name, dev in (("fast", "fast"), ("device_ieee", True), ("host", False)):
        out = run_poly(dm, 3, coef, dev)
        res[name] = np.array([root_error(o[:3], [True, o[3] == 3, o[3] == 3], ex) for o, ex in zip(out, exact)])
        res[name + "_n"] = out[:, 3]
    return coef, tags, res


def measure_quartic(dm):
    coef, tags = quartic_inputs()
    exact = exact_roots(coef)
    res = {"floor": conditioning_floor(coef, exact)}
    for name, dev in (("device", True), ("host", False)):
        out = run_poly(dm, 4, coef, dev)
        m = out[:, 4].astype(int)
        res[name] = np.array([root_error(o[:4], [(mk >> k) & 1 for k in range(4)], ex) for o, mk, ex in zip(out, m, exact)])
        res[name + "_mask"] = m
    return coef, tags, res


# ---------------------------------------------------------------- Cholesky
def chol_inputs(N, seed):
    """SPD normal matrices Q diag(s) Q^T with condition numbers 1 .. 1e12, damped as the LM damps them (A + lambda on the diagonal,
    lambda from 1e-10 to 1e-3 times the largest eigenvalue, and undamped)"""
    rng = np.random.default_rng(seed)
    conds = np.repeat(10.0 ** np.arange(0, 13, dtype=np.float64), 8)
    A, b = [], []
    for i, k in enumerate(conds):
        q, _ = np.linalg.qr(rng.standard_normal((N, N)))
        s = np.exp(np.linspace(0, -np.log(k), N)) * 10.0 ** rng.uniform(-3, 3)
        M = (q * s) @ q.T
        M = 0.5 * (M + M.T)
        lam = 0.0 if i % 4 == 0 else s[0] * 10.0 ** rng.uniform(-10, -3)
        M = M + lam * np.eye(N)
        A.append(M); b.append(rng.standard_normal(N))
    return np.array(A), np.array(b), conds


def measure_chol(dm, N, seed=6):
    A, b, conds = chol_inputs(N, seed + N)
    rc, x = dm.call("dm_chol", [N], [A, b], b.shape, len(A))
    assert rc == 0
    bwd, fwd = np.zeros(len(A)), np.zeros(len(A))
    with mpmath.workprec(PREC):
        for i in range(len(A)):
            Am = mpmath.matrix(A[i].tolist()); bm = mpmath.matrix(b[i].tolist()); xm = mpmath.matrix(x[i].tolist())
            r = bm - Am * xm
            # normwise backward error (Rigal-Gaches): |b - A x| / (|A| |x| + |b|), infinity norms
            bwd[i] = float(mpmath.norm(r, mpmath.inf) / (mpmath.mnorm(Am, mpmath.inf) * mpmath.norm(xm, mpmath.inf) + mpmath.norm(bm, mpmath.inf)))
            xe = mpmath.lu_solve(Am, bm)
            fwd[i] = float(mpmath.norm(xm - xe, mpmath.inf) / mpmath.norm(xe, mpmath.inf))
    return x, bwd / EPS, fwd / (EPS * conds), conds


# ---------------------------------------------------------------- the tests
@pytest.mark.gpu
@pytest.mark.parametrize("op", list(UNARY_BOUND))
def test_unary_primitive_within_its_stated_ulp_bound(dm, op):
    x, got, err = measure_unary(dm, op)
    bad = np.flatnonzero(~(err <= UNARY_BOUND[op]))
    assert not len(bad), (op, f"max {err.max():.3g} ulp", [(float(x[i]), float(got[i]), float(err[i])) for i in bad[:8]])


@pytest.mark.gpu
def test_sv_div_within_two_ulp(dm):
    """a * sv_rcp(b): the reciprocal's 1.5 ulp and the product's rounding"""
    a, b, got, err = measure_div(dm)
    bad = np.flatnonzero(~(err <= 2.0))
    assert not len(bad), (f"max {err.max():.3g}", [(float(a[i]), float(b[i]), float(err[i])) for i in bad[:8]])


@pytest.mark.gpu
def test_lm_log1p_small_arguments_and_special_values(dm):
    """the cancellation of table cell 0 (centred on 1 + 1 / 256) left lm_log1p(0) = 1.7e-18 and an absolute error of ~1.7e-18 below 2^-8;
    exact 0 at 0, x itself where x^2 / 2 is below half an ulp, inf and NaN passed through"""
    x = np.array([0.0, -0.0, SUB_MIN, SUB_MAX, DMIN, 1e-300, 2.0 ** -60, 1e-12, 1e-8, 1e-4, np.inf, np.nan])
    got = run_unary(dm, "lm_log1p", x)
    assert got[0] == 0.0 and got[1] == 0.0, got[:2]
    assert np.array_equal(got[2:7], x[2:7]), got[2:7]                   # log1p(x) = x - x^2 / 2 + ... rounds to x
    ref = [float(mpmath.log1p(mpmath.mpf(float(v)))) for v in x[7:10]]
    assert np.all(np.abs(got[7:10] - ref) <= 2 * np.spacing(ref)), (got[7:10], ref)
    assert got[10] == np.inf and np.isnan(got[11])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [3, 4])
def test_cauchy_loss_value_tab_within_four_ulp(dm, kind):
    """loss_value_tab = t2 * lm_log1p(min(r2, t2) / t2) with lm_rcp: <= 1 ulp (rcp) + 0.5 (product) + 2 (log1p, condition <= 1) + 0.5"""
    thr, r2, got, err = measure_loss(dm, kind)
    bad = np.flatnonzero(~(err <= 4.0))
    assert not len(bad), (kind, f"max {err.max():.3g}", [(float(thr[i]), float(r2[i]), float(got[i]), float(err[i])) for i in bad[:8]])
    t2 = thr * thr
    zero = r2 == 0.0
    assert np.all(got[zero] == 0.0)
    if kind == 4:                                                       # truncated at r2 = t2: exactly the value at t2 beyond it
        hi = r2 > t2
        assert np.all(got[hi] == run_unary(dm, "loss4", thr[hi], t2[hi]))


@pytest.mark.gpu
def test_special_values_of_the_reciprocals_and_roots(dm):
    """what the hardware seeds with their Newton steps return outside the domain, as mdrp_math.h states it (measured, then pinned):
    1 / 0, 1 / inf and 1 / x for |x| < 2^-1024 are NaN where IEEE division gives inf / 0; the reciprocal of the largest subnormal and of DBL_MAX
    (a subnormal result) are exact; sv_sqrt keeps signed zeros and turns inf into NaN; the roots of subnormals are finite but inaccurate"""
    for op in ("sv_rcp", "lm_rcp"):
        got = run_unary(dm, op, np.array([0.0, -0.0, np.inf, -np.inf, np.nan, SUB_MIN, 2.0 ** -1025]))
        assert np.isnan(got).all(), (op, got)
        got = run_unary(dm, op, np.array([SUB_MAX, DMAX, -DMAX]))
        assert np.array_equal(got, [float(1 / mpmath.mpf(v)) for v in (SUB_MAX, DMAX, -DMAX)]), (op, got)
    got = run_unary(dm, "sv_sqrt", np.array([0.0, -0.0, -1.0, np.nan, np.inf]))
    assert got[0] == 0.0 and got[1] == 0.0 and np.signbit(got[1]) and np.isnan(got[2:]).all(), got
    for op in ("sv_rsqrt", "lm_rsqrt"):
        got = run_unary(dm, op, np.array([0.0, -1.0, np.nan, np.inf]))
        assert np.isnan(got).all(), (op, got)
    sub = np.array([SUB_MIN, 1e-320, SUB_MAX / 3])
    for op, ref in (("sv_sqrt", mpmath.sqrt), ("sv_rsqrt", lambda v: 1 / mpmath.sqrt(v)), ("lm_rsqrt", lambda v: 1 / mpmath.sqrt(v))):
        got = run_unary(dm, op, sub)
        rel = np.array([float(g / ref(mpmath.mpf(v))) for g, v in zip(got, sub)])
        assert np.all((rel > 1 / 3) & (rel < 3)), (op, rel)            # finite, positive, the right magnitude: no more


# FAST against the IEEE branch: within CUBIC_FACTOR x the larger of the IEEE branch's error and the conditioning floor, plus CUBIC_ABS.
# Near-triple clusters and triple roots are held to CLUSTER_FACTOR instead: there the Newton polish both branches share converges only linearly
# from the A&S acos's 2e-8, and on exact triple roots it is itself unstable (f / f' of two rounding-level numbers): measured on the device, both
# branches up to 7e5 x the conditioning floor there (a root off by up to 10 x its scale), the FAST one at most 12 x the IEEE one's error.
CUBIC_FACTOR, CUBIC_ABS, CLUSTER_FACTOR = 4.0, 8.0, 16.0


@pytest.mark.gpu
def test_fast_cubic_roots_match_the_ieee_branch(dm):
    """solve_cubic_real<true> (A&S 4.4.46 acos, Taylor cos / sin, three Newton steps) against solve_cubic_real<false> on the device, both
    against mpmath: root error within CUBIC_FACTOR x max(IEEE error, conditioning floor) + CUBIC_ABS eps x the root scale for separated roots,
    one real root and two nearly coinciding roots (arg near +-1), CLUSTER_FACTOR for three; the same count of real roots; separated roots to
    2 eps"""
    coef, tags, res = measure_cubic(dm)
    factor = np.array([CLUSTER_FACTOR if t in ("cluster", "triple") else CUBIC_FACTOR for t in tags])
    bound = factor * np.maximum(res["device_ieee"], res["floor"]) + CUBIC_ABS
    bad = np.flatnonzero(~(res["fast"] <= bound))
    assert not len(bad), [(tags[i], coef[i].tolist(), float(res["fast"][i]), float(res["device_ieee"][i]), float(res["floor"][i])) for i in bad[:8]]
    assert np.array_equal(res["fast_n"], res["device_ieee_n"])
    sep = np.array([t in ("separated", "one_real") for t in tags])
    assert res["fast"][sep].max() <= 2.0, res["fast"][sep].max()


@pytest.mark.gpu
def test_quartic_roots_match_the_host_build(dm):
    """solve_quartic_real on the device (FAST resolvent cubic, sv_* arithmetic) against its host build (IEEE): root error within CUBIC_FACTOR x
    max(host error, conditioning floor) + CUBIC_ABS; the same validity masks but where two roots nearly coincide (whether their quadratic
    factor's discriminant is >= 0 is then decided by rounding)"""
    coef, tags, res = measure_quartic(dm)
    near = np.array([t == "near_double" for t in tags])
    diff = res["device_mask"] != res["host_mask"]
    assert not (diff & ~near).any(), np.flatnonzero(diff & ~near)[:8]
    bound = CUBIC_FACTOR * np.maximum(res["host"], res["floor"]) + CUBIC_ABS
    bad = np.flatnonzero(~(res["device"] <= bound))
    assert not len(bad), [(tags[i], coef[i].tolist(), float(res["device"][i]), float(res["host"][i]), float(res["floor"][i])) for i in bad[:8]]


CHOL_C = 0.5                                                            # measured: <= 0.12 N on every N


@pytest.mark.gpu
@pytest.mark.parametrize("N", [5, 6, 7, 8, 9])
def test_chol_solve_backward_stable(dm, N):
    """chol_solve<N> (rsqrt per column): normwise backward error <= CHOL_C * N * eps on SPD systems of condition 1 .. 1e12"""
    x, bwd, fwd, conds = measure_chol(dm, N)
    assert np.isfinite(x).all()
    assert bwd.max() <= CHOL_C * N, (N, float(bwd.max()), float(conds[int(np.argmax(bwd))]))
    assert fwd.max() <= N, (N, float(fwd.max()))                       # forward error <= N cond eps
