"""The cases of tests/test_gpu_front_stages.py and tests/test_front_stages_host.py: the smallest shapes at which k_prep / kc_prep, the samplers and the
solver kernels can still go wrong.  A helper, not a test; nothing here touches the GPU.

One batch of six pairs per estimator, n_max = 300, n_per_pair = [300, 300, 257, 37, K, K - 1] (K the sample size): the two pairs of 300 share a
sample table; 257 gives one lane of the prep two records and the rest one; 37 ends inside a 16-row fragment group; at n = K nearly every speculation
step of the sampler sees a rejection; K - 1 is inactive.  A second batch with n_max = 291 (three rows into its last fragment group; neither width is a multiple of 16: the
fragments' pair stride is ceil(n_max / 16) groups) runs with score_initial_model.  Chunk lists: one iteration; [63, 1, 64]; [65, 255, 257] (partial last wavefront, partial last 256-lane workgroup, both chunk
parities, sampler state carried twice) — [65, 69, 66] for the 6-point solver, which is slow."""
import functools

import numpy as np

import front_stages_ref as fr
from mdrp_amd import synth

KINDS = ((0, False), (0, True), (1, False), (2, False), (3, False), (4, False), (5, False))  # (kind, the shift solver)
N_MAX, N_MAX_ODD = 300, 291
CHUNK_LISTS = ((1,), (63, 1, 64), (65, 255, 257))
CHUNK_LISTS_6PT = ((1,), (63, 1, 64), (65, 69, 66))
SPARE = 3          # iterations of the slot tables behind the last chunk: they keep the fill pattern
SEED = 32          # (of forty seeds the one with the most P3P NaN iterations in front of a wavefront's first real pose: three)
P3P_NAN_TRIPLE = (7000, (1, 4, 6))  # a synth pair and three of its records on which the reference's P3P returns NaN poses in every order
PP = (640.0, 480.0)
UNJUDGED_CAP = 0.01  # of the live iterations of a case: where the references themselves disagree
SIXPT_CAP = 0.01     # 6-point: count differences, and solutions beyond 1e-6 (tests/test_gpu_classic.py::test_sixpt_solver_equals_oracle_and_reference)


def kind_id(kind, shift):
    return fr.solver_name(kind, shift)


def chunk_lists(kind):
    return CHUNK_LISTS_6PT if kind == 4 else CHUNK_LISTS


def counts(kind, n_max):
    K = fr.SAMPLE_SIZE[kind]
    return np.array([n_max, n_max, 257, 37, K, K - 1], dtype=np.int32)


def camera_records(kind, batch, seed=0):
    """calibrated kinds: PINHOLE with fx != fy on the even pairs, SIMPLE_PINHOLE on the odd ones, parameters of their own per pair and image;
    6-point: the principal point in cam1; the others take none"""
    from mdrp_amd import _capi as capi
    if kind not in (0, 3, 4):
        return None, None
    c1, c2 = np.zeros(batch, dtype=capi.CAMERA_DTYPE), np.zeros(batch, dtype=capi.CAMERA_DTYPE)
    for i in range(batch):
        if kind == 4:
            c1["params"][i, :2] = (PP[0] + 3.0 * i, PP[1] - 2.0 * i)
            continue
        for c, f in ((c1, 780.0 + 13.0 * i + seed), (c2, 835.0 - 7.0 * i + seed)):
            if i % 2 == 0:
                c["model_id"][i] = 1
                c["params"][i] = (f * 1.01, f * 0.99, PP[0] + i, PP[1] - i)
            else:
                c["params"][i, :3] = (f, PP[0] - 2.0 * i, PP[1] + i)
    return c1, (c2 if kind != 4 else None)


@functools.lru_cache(maxsize=None)
def batch(kind, shift, n_max):
    """x1, x2 (6, n_max, 2) pixels about the principal point PP, d1, d2 (6, n_max), n (6,), cam1, cam2: 40 % outliers, half a pixel of noise"""
    ns = counts(kind, n_max)
    rf = {1: "shared", 2: "varying", 4: "shared"}.get(kind)
    B = len(ns)
    x1, x2, d1, d2 = np.zeros((B, n_max, 2)), np.zeros((B, n_max, 2)), np.ones((B, n_max)), np.ones((B, n_max))
    for i, n in enumerate(ns):
        p = synth.make_pair(7000 + 10 * kind + i, max(int(n), 8), pp=PP, noise_px=0.5, depth_noise=0.02, outlier_frac=0.4, random_focal=rf,
                            shift1=0.2 if shift else 0.0, shift2=-0.1 if shift else 0.0)
        rows = np.arange(n)
        if (kind, shift, i) == (0, False, 4):  # P3P: the pair of three records never has a real pose, every iteration of it holds the NaN model
            p, rows = synth.make_pair(P3P_NAN_TRIPLE[0], 8, pp=PP, noise_px=0.5, depth_noise=0.02, outlier_frac=0.4), np.array(P3P_NAN_TRIPLE[1])
        x1[i, :n], x2[i, :n], d1[i, :n], d2[i, :n] = p["x1"][rows], p["x2"][rows], p["d1"][rows], p["d2"][rows]
    cam1, cam2 = camera_records(kind, B)
    return dict(x1=x1, x2=x2, d1=d1, d2=d2, n=ns, cam1=cam1, cam2=cam2)


def options(kind, shift, chunks, initial=False):
    total = int(sum(chunks)) + SPARE
    ro = dict(max_iterations=total, min_iterations=total, max_epipolar_error=2.0, max_reproj_error=16.0, seed=SEED, estimate_shift=bool(shift),
              score_initial_model=bool(initial))
    return ro, dict(loss_type="TRUNCATED_CAUCHY", loss_scale=1.5)


def capi_options(ro, bo):
    from mdrp_amd import _capi as capi
    r = capi.ransac_opt_from_dict({k: v for k, v in ro.items() if k not in ("estimate_shift", "score_initial_model")})
    r.monodepth_estimate_shift, r.score_initial_model = int(ro["estimate_shift"]), int(ro["score_initial_model"])
    return r, capi.bundle_opt_from_dict(bo)


# ---- corrupted records (calibrated kind): four pairs of 64 records; pair 0 is clean, pairs 1 - 3 hold a NaN, an inf and 1e16
CORRUPT_N = 64
CORRUPT = {1: [(5, "x2", 0, np.nan)], 2: [(17, "x1", 1, np.inf)],
           # 1e16 pixels are 1.2e13 focal lengths: record 9 stays below the kernel's 1e15 bound on a monomial (its row is its own business, the box must
           # cover it); in record 40 the product of two such coordinates is beyond it
           3: [(9, "x1", 0, 1e16), (40, "x1", 0, 1e16), (40, "x2", 1, 1e16)]}
CORRUPT_ZERO_ROWS = {1: (5,), 2: (17,), 3: (40,)}


@functools.lru_cache(maxsize=None)
def corrupted_batch(corrupt=True):
    ns = np.full(4, CORRUPT_N, dtype=np.int32)
    x1, x2, d1, d2 = np.zeros((4, CORRUPT_N, 2)), np.zeros((4, CORRUPT_N, 2)), np.ones((4, CORRUPT_N)), np.ones((4, CORRUPT_N))
    for i in range(4):
        p = synth.make_pair(7900 + i, CORRUPT_N, pp=PP, noise_px=0.5, depth_noise=0.02, outlier_frac=0.3)
        x1[i], x2[i], d1[i], d2[i] = p["x1"], p["x2"], p["d1"], p["d2"]
    if corrupt:
        for pair, edits in CORRUPT.items():
            for rec, which, axis, value in edits:
                (x1 if which == "x1" else x2)[pair, rec, axis] = value
    cam1, cam2 = camera_records(0, 4, seed=5)
    return dict(x1=x1, x2=x2, d1=d1, d2=d2, n=ns, cam1=cam1, cam2=cam2)


# ---- the prep on the host, for the host test: the definitions of front_stages_ref rounded to double
def host_prep(kind, d):
    """pts (B, n_max, 6) and dep (B, n_max, 2) as the definitions give them in float64 (rows from n on are zero)"""
    B, n_max = d["x1"].shape[:2]
    pts, dep = np.zeros((B, n_max, 6)), np.stack([d["d1"], d["d2"]], axis=2)
    for i, n in enumerate(d["n"]):
        n = int(n)
        if n == 0:
            continue
        c1 = None if d["cam1"] is None else d["cam1"][i]
        c2 = None if d["cam2"] is None else d["cam2"][i]
        x1, x2 = d["x1"][i, :n], d["x2"][i, :n]
        norm = cen = None
        if kind not in (0, 3):
            cen, _ = fr.scale_and_centre(kind, x1, x2, c1)
            cen = cen.astype(np.float64)
            norm = np.float64(fr.norm_of(x1, x2, cen))
        pts[i, :n, :4] = fr.points(kind, x1, x2, c1, c2, norm, cen)
        pts[i, :n, 4:] = fr.inverse_lengths(pts[i, :n, :4]).astype(np.float64)
    return pts, dep


@functools.lru_cache(maxsize=None)
def definition_records(kind, shift, n_max):
    """host_prep of batch(kind, shift, n_max): the records as the definitions give them (the device's differ from them by at most 2 ulp in the
    inverse lengths and, where it normalises, by the last bits of its norm)"""
    return host_prep(kind, batch(kind, shift, n_max))


# ---- the references of one pair's iterations, shared by every case that reaches them
_SOLVED = {}


def references(name, kind, x1h, x2h, d1, d2):
    """(oracle solutions, host solutions or None, judged, the P3P NaN predicate): judged is False only where the two references differ in count or
    by more than the tolerance.  The 6-point solver has no host build: every sample is judged, against the oracle with its allowance."""
    key = (name, x1h.tobytes(), x2h.tobytes(), None if d1 is None else d1.tobytes(), None if d2 is None else d2.tobytes())
    if key not in _SOLVED:
        orc = fr.oracle_solutions(name, x1h, x2h, d1, d2)
        host = fr.host_solutions(name, x1h, x2h, d1, d2)
        _SOLVED[key] = (orc, host, host is None or fr.same_solutions(name, orc, host), name == "p3p" and fr.p3p_nan(x1h, x2h, d1))
    return _SOLVED[key]


def chunk_of(chunks):
    """[(offset, length)] of a chunk list"""
    offs = np.concatenate([[0], np.cumsum(chunks)[:-1]])
    return [(int(o), int(c)) for o, c in zip(offs, chunks)]


def nan_front(counts_, pred, chunks):
    """the iterations of a P3P run that must hold the NaN model (slot state -3): inside each chunk, in each group of 64 iterations (a wavefront of
    the solver), those in front of the group's first iteration with a real pose for which the reference's P3P returns NaN poses"""
    out = []
    for off, length in chunk_of(chunks):
        for g0 in range(0, length, 64):
            for it in range(off + g0, off + min(g0 + 64, length)):
                if counts_[it] > 0:
                    break
                if pred[it]:
                    out.append(it)
    return out


def pair_references(kind, shift, pts, dep, samples):
    """references() for every sample [iterations][K] of one pair, from its records pts (n, 6) and dep (n, 2) or None"""
    name = fr.solver_name(kind, shift)
    out = []
    for s in samples:
        s = np.asarray(s, dtype=np.int64)
        out.append(references(name, kind, *fr.solver_inputs(kind, pts[s], None if dep is None else dep[s])))
    return out
