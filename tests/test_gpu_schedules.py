"""Every schedule of run_pass (mdrp_capi.hip; the chunk rules: mdrp_schedule.h) must give the same records and masks, for all six estimators: one chunk on one stream (the plain
sequential schedule), the three-stream chunk pipeline, the fused tail, and the sliced host-buffer front (a host-buffer call of >= 2 x HOST_SLICE_PAIRS
pairs copies the correspondences in 256-pair slices; k_prep and the second chunk's solver of each slice run on the aux stream while the main stream
solves and sweeps the first chunk).  The sequential schedule itself is anchored to the CPU oracle on the pairs around the slice edges."""
import functools

import numpy as np
import pytest

from helpers import model_diff
from oracle import pyorc as po
from test_oracle_classic import fund_diff, pose_diff

SLICE = 256                   # HOST_SLICE_PAIRS (mdrp_capi.hip)
NMAX = 400                    # correspondences per pair of the sliced-front inputs (ragged below that)
POOL = 1100                   # pairs generated per estimator; every shape takes a prefix
TINY = {5: 2, 255: 0, 256: 3, 510: 2, 511: 3, 599: 0, 767: 3, 1099: 2}  # pairs below (or at) the sample size, on slice edges and call ends
SAMPLE = {0: 3, 1: 3, 2: 3, 3: 5, 4: 6, 5: 7}
RF = {1: "shared", 2: "varying", 4: "shared"}  # synth.make_pair random_focal per estimator
ORC_RO = dict(max_epipolar_error=2.0, max_reproj_error=16.0)
RO = {"max_epipolar_error": 2.0, "max_reproj_error": 16.0}
BO = {"loss_type": "TRUNCATED_CAUCHY"}
KNOBS = ("MDRP_CHUNKS", "MDRP_LO_OVERLAP", "MDRP_BOUND", "MDRP_FUSE_TAIL", "MDRP_LO_THREADS", "MDRP_FINAL_THREADS", "MDRP_PAIRS_PER_PASS")

# shape: (pairs, max_iterations = min_iterations, environment).  Every one has two chunks in its first super-chunk, [L0, span - L0].
SHAPES = {
    "b511_i1500": (511, 1500, {}),                                    # one pair short of slicing: the unsliced control
    "b512_i1500": (512, 1500, {}),                                    # two slices; the first is the last-but-one
    "b600_i300": (600, 300, {}),                                      # 128 | 172: solver grids of 2 and 3 blocks per pair
    "b768_i300": (768, 300, {}),
    "b1100_i2100_c1024": (1100, 2100, {"MDRP_CHUNKS": "1024"}),       # 1024 | 1076: the last-but-one and the last slice both overlap
    "b1100_i300_pass550": (1100, 300, {"MDRP_PAIRS_PER_PASS": "550"}),  # two passes, both sliced: host source offsets of a later pass
}
SIXPT_SHAPES = ("b600_i300", "b768_i300", "b1100_i300_pass550")      # the 6-point solver only where the runs are short
CASES = [(k, s) for k in range(6) for s in SHAPES if k != 4 or s in SIXPT_SHAPES]

# Pairs of the oracle anchor in a deviation class of DESIGN.md 5, by (estimator, pair): their MODEL is not compared (iterations, inliers and mask are).
# Class (v), score_tie: a pair of exactly three correspondences with a 3-point solver — every sample is the same three points in another order, every
# record a tie decided in the last bits of the score, so which of the equally good models wins is rounding.
ORACLE_MODEL_EXCLUDED = {(0, 256): "class (v) score_tie: N = 3, three inliers", (1, 511): "class (v) score_tie: N = 3, three inliers"}


def red5_overlaps(batch, len0, len1):
    """5-point Reduce5 block ranges [first, last) of the two solves the sliced front may run at the same time, laid out as before the first chunk had a
    region of its own (both at red5 + p0 * ceil(len / 64) blocks): chunk 0 on the main stream (pairs [0, p0 + pc) behind the last-but-one slice's k_prep,
    the rest behind the last one's) against chunk 1 of the same slice on aux.  Returns the overlapping pairs of ranges."""
    if batch < 2 * SLICE:
        return []
    sg0, sg1 = -(-len0 // 64), -(-len1 // 64)
    out, swept0 = [], 0
    for p0 in range(0, batch, SLICE):
        pc = min(SLICE, batch - p0)
        last = p0 + SLICE >= batch
        r1 = (p0 * sg1, (p0 + pc) * sg1)
        if not last and p0 + 2 * SLICE >= batch:
            swept0 = p0 + pc
            r0 = (0, swept0 * sg0)
        elif last:
            r0 = (swept0 * sg0, batch * sg0)
        else:
            continue
        if r0[0] < r1[1] and r1[0] < r0[1]:
            out.append((r0, r1))
    return out


def test_shapes_reach_the_former_red5_overlap():
    """The arithmetic behind the shapes above (no GPU): the old layout overlapped on every sliced shape of this file and on none of the shapes the suite
    ran the sliced front with before (B = 600 at 1500 iterations, the benchmark shape)."""
    assert red5_overlaps(511, 128, 1372) == []
    assert red5_overlaps(512, 128, 1372) == [((0, 512), (0, 5632))]
    assert red5_overlaps(600, 128, 172) and red5_overlaps(768, 128, 172) and red5_overlaps(550, 128, 172)
    assert len(red5_overlaps(1100, 1024, 1076)) == 2                  # last-but-one and last slice
    assert red5_overlaps(600, 128, 1372) == [] and red5_overlaps(1024, 512, 9488) == []


@functools.lru_cache(maxsize=None)
def _pool(kind):
    """POOL ragged pairs of one estimator, zero-padded to NMAX; per-pair cameras (kinds 0 and 3: focal length of the pair's own synthetic camera)"""
    from mdrp_amd import _capi, synth
    rng = np.random.default_rng(5100 + kind)
    ns = rng.integers(200, NMAX + 1, size=POOL).astype(np.int32)
    for i, n in TINY.items():
        ns[i] = n
    focal = rng.uniform(600.0, 1000.0, POOL)
    x1, x2 = np.zeros((POOL, NMAX, 2)), np.zeros((POOL, NMAX, 2))
    d1, d2 = np.ones((POOL, NMAX)), np.ones((POOL, NMAX))
    for i in range(POOL):
        n = int(ns[i])
        if n:
            p = synth.make_pair(61000 + 1000 * kind + i, n, f1=focal[i], f2=focal[i], noise_px=0.5, depth_noise=0.02,
                                outlier_frac=(0.2, 0.35, 0.5)[i % 3], random_focal=RF.get(kind))
            x1[i, :n], x2[i, :n], d1[i, :n], d2[i, :n] = p["x1"], p["x2"], p["d1"], p["d2"]
    cams = np.zeros(POOL, dtype=_capi.CAMERA_DTYPE)
    if kind in (0, 3):
        cams["params"][:, 0] = focal                                  # SIMPLE_PINHOLE f, principal point 0
    return ns, x1, x2, d1, d2, cams, focal


def _cams(kind, cams):
    """kinds 0 and 3 take both cameras, the 6-point one its principal point from cam1 (all zero here), the focal estimators none"""
    if kind in (0, 3, 4):
        return cams, cams
    return None, None


def _set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _differs(a, b):
    """names of the record fields that are not bit-identical"""
    out = [f for f in ("refinements", "iterations", "num_inliers") if not np.array_equal(a[f], b[f])]
    for f in ("inlier_ratio", "model_score"):
        if a[f].tobytes() != b[f].tobytes():
            out.append(f)
    if a["model"].tobytes() != b["model"].tobytes():
        out.append("model")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape", CASES)
def test_sliced_host_front_equals_resident_and_sequential_schedules(monkeypatch, kind, shape):
    """(1) the host-buffer call, sliced from 512 pairs on, equals the same batch resident on the device bit for bit; (2) the same host call again on the
    same handle equals the first (one repeat: determinism, not a loop); (3) iterations, inliers, LO count, model and mask equal those of the plain
    sequential schedule (MDRP_CHUNKS=0 MDRP_LO_OVERLAP=0: one chunk, no aux stream).  Ragged pairs incl. 0, 2 and 3 correspondences on slice edges.
    The shapes are those where the 5-point solver's Reduce5 scratch of the first chunk (main stream) and of the second (aux) used to overlap
    (red5_overlaps, asserted from mdrp_stats::first_chunk)."""
    import torch
    from mdrp_amd import _capi
    B, its, env = SHAPES[shape]
    ns, x1, x2, d1, d2, cams, _ = _pool(kind)
    ns, x1, x2, d1, d2, cams = ns[:B], x1[:B], x2[:B], d1[:B], d2[:B], cams[:B]
    c1, c2 = _cams(kind, cams)
    mono = kind <= 2
    ro = _capi.ransac_opt_from_dict(dict(RO, max_iterations=its, min_iterations=its))
    bo = _capi.bundle_opt_from_dict(BO)
    dev = torch.device("cuda", 0)
    _set_env(monkeypatch, env)
    h = _capi.Handle(0)
    try:
        def host():
            r, m = h.estimate_batch(kind, x1, x2, d1 if mono else None, d2 if mono else None, ro, bo, ns, c1, c2)
            return r.copy(), m.copy()

        res_h, mask_h = host()
        len0 = int(h.last_stats()["first_chunk"])
        assert 2 * len0 <= its, len0                                  # two chunks: the front is sliced from 2 x SLICE pairs on
        per_pass = int(env.get("MDRP_PAIRS_PER_PASS", B))
        sliced = B >= 2 * SLICE
        assert bool(red5_overlaps(min(per_pass, B), len0, its - len0)) == sliced, (len0, its)

        t = [torch.from_numpy(a).to(dev) for a in (x1, x2, d1, d2)]
        mask_d = torch.zeros((B, NMAX), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        h.estimate_batch_device(kind, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr() if mono else 0, t[3].data_ptr() if mono else 0, B, NMAX,
                                ro, bo, ns, c1, c2, mask_d.data_ptr())
        res_d = h.fetch_results(B)
        mask_d = mask_d.cpu().numpy()
        assert res_h.tobytes() == res_d.tobytes(), (kind, shape, _differs(res_h, res_d), np.flatnonzero(res_h.tobytes() != res_d.tobytes())[:8])
        assert np.array_equal(mask_h, mask_d), (kind, shape, np.flatnonzero((mask_h != mask_d).any(axis=1))[:16])

        res_h2, mask_h2 = host()
        assert res_h.tobytes() == res_h2.tobytes(), (kind, shape, _differs(res_h, res_h2))
        assert np.array_equal(mask_h, mask_h2), (kind, shape, np.flatnonzero((mask_h != mask_h2).any(axis=1))[:16])

        _set_env(monkeypatch, dict(env, MDRP_CHUNKS="0", MDRP_LO_OVERLAP="0"))
        res_s, mask_s = host()
        assert int(h.last_stats()["first_chunk"]) == its
        bad = [i for i in range(B) if _differs(res_h[i:i + 1], res_s[i:i + 1])]
        assert not bad, (kind, shape, bad[:16], [_differs(res_h[i:i + 1], res_s[i:i + 1]) for i in bad[:4]])
        assert np.array_equal(mask_h, mask_s), (kind, shape, np.flatnonzero((mask_h != mask_s).any(axis=1))[:16])

        assert int(res_h["num_inliers"].max()) > 200                  # not a comparison of empty results
        tiny = [i for i in TINY if i < B and TINY[i] < SAMPLE[kind]]
        assert all(int(res_h[i]["iterations"]) == 0 and int(res_h[i]["num_inliers"]) == 0 for i in tiny), tiny
        assert int(res_h["iterations"].max()) == its
    finally:
        h.close()


def _orc_model_diff(kind, got, ref):
    """model distance as the trajectory tests measure it: model_diff (monodepth), pose / fundamental distance (5- / 7-point), pose and focal (6-point)"""
    if kind <= 2:
        return model_diff(got, ref)
    if kind == 5:
        return fund_diff(got, ref)
    d = pose_diff(got[:7], ref[:7])
    if kind == 4:
        d = max(d, abs(got[10] - ref[10]) / abs(ref[10]))
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape", [(k, s) for k in range(6) for s in ("b600_i300", "b512_i1500") if k != 4 or s in SIXPT_SHAPES])
def test_sequential_schedule_follows_the_oracle_on_slice_edges(monkeypatch, kind, shape):
    """The reference of the test above (one chunk, one stream) against the CPU oracle (oracle/pyorc.py: estimate for kinds 0-2, estimate_classic for 3-5),
    on the pairs around the slice edges and a few more: iterations, inliers and mask identical, model within 1e-6 but on ORACLE_MODEL_EXCLUDED (LO counts
    may differ by rounding ties, DESIGN.md 5, and are not compared)."""
    from mdrp_amd import _capi
    B, its, env = SHAPES[shape]
    ns, x1, x2, d1, d2, cams, focal = _pool(kind)
    c1, c2 = _cams(kind, cams[:B])
    mono = kind <= 2
    ro = _capi.ransac_opt_from_dict(dict(RO, max_iterations=its, min_iterations=its))
    bo = _capi.bundle_opt_from_dict(BO)
    _set_env(monkeypatch, dict(env, MDRP_CHUNKS="0", MDRP_LO_OVERLAP="0"))
    h = _capi.Handle(0)
    try:
        res, mask = h.estimate_batch(kind, x1[:B], x2[:B], d1[:B] if mono else None, d2[:B] if mono else None, ro, bo, ns[:B], c1, c2)
    finally:
        h.close()
    oro = po.ransac_opt(max_iterations=its, min_iterations=its, **ORC_RO)
    obo = po.bundle_opt(loss_type=4)
    picks = sorted(i for i in {0, 1, 5, 100, SLICE - 1, SLICE, SLICE + 1, 300, 2 * SLICE - 1, 2 * SLICE, B - 2, B - 1} if i < B)
    bad, checked = [], 0
    for i in picks:
        n = int(ns[i])
        if kind <= 2:
            cam = po.cam_flat(0, [focal[i], 0.0, 0.0]) if kind == 0 else None
            m, st, mk = po.estimate(kind, x1[i, :n], x2[i, :n], d1[i, :n], d2[i, :n], oro, obo, cam, cam)
        elif kind == 3:
            cam = po.cam_flat(0, [focal[i], 0.0, 0.0])
            m, st, mk = po.estimate_classic(kind, x1[i, :n], x2[i, :n], oro, obo, cam, cam)
        else:
            m, st, mk = po.estimate_classic(kind, x1[i, :n], x2[i, :n], oro, obo, pp=(0.0, 0.0))
        r = res[i]
        same = (int(r["iterations"]), int(r["num_inliers"])) == (st.iterations, st.num_inliers) and np.array_equal(mask[i, :n], mk)
        compare_model = same and st.num_inliers > 0 and (kind, i) not in ORACLE_MODEL_EXCLUDED
        d = _orc_model_diff(kind, _capi.model_to_array(r["model"]), np.asarray(m, dtype=np.float64)) if compare_model else 0.0
        if not same or not d < 1e-6:
            bad.append(f"pair {i} (N = {n}): iterations {int(r['iterations'])} / {st.iterations}, inliers {int(r['num_inliers'])} / {st.num_inliers}, "
                       f"mask {'same' if np.array_equal(mask[i, :n], mk) else 'differs'}, model {d:.3g}")
        checked += 1
    assert not bad, (kind, shape, bad)
    assert checked >= 10


# chunk-schedule variants against the single-chunk, one-stream reference (as test_gpu_parity.py::test_schedule_does_not_change_results for kind 0).
# No thread-count knob among them: every variant schedules the same summation trees, so records must be bit-identical.
SCHEDULES = ({}, {"MDRP_CHUNKS": "128"}, {"MDRP_CHUNKS": "512"}, {"MDRP_CHUNKS": "128,1024"}, {"MDRP_CHUNKS": "128,256,512"},
             {"MDRP_CHUNKS": "512", "MDRP_LO_OVERLAP": "0"}, {"MDRP_CHUNKS": "128", "MDRP_BOUND": "0"}, {"MDRP_CHUNKS": "128", "MDRP_FUSE_TAIL": "0"},
             {"MDRP_CHUNKS": "128,512", "MDRP_FUSE_TAIL": "1"}, {"MDRP_CHUNKS": "64,256", "MDRP_FUSE_TAIL": "0", "MDRP_BOUND": "0"})


@pytest.mark.gpu
@pytest.mark.parametrize("B", [12, 136])
@pytest.mark.parametrize("kind", [1, 2, 3, 4, 5])
def test_chunk_schedule_does_not_change_results(monkeypatch, kind, B):
    """Which hypotheses k_count / k_bound retire against which records, the three-stream pipeline, the fp32 bound stage and the fused tail are scheduling
    only, for the focal, 5-, 6- and 7-point estimators too: records and masks bit-identical to one chunk on one stream (nothing retired, no overlap).
    N = 2300 (nine 256-record tiles): k_count's two-phase retirement is active in every chunked schedule.  3000 iterations: room for "128,1024".
    B = 12: the small-call path (k_score_w, no fp32 stage); B = 136: k_bound and the lane-per-hypothesis k_score."""
    from mdrp_amd import _capi, synth
    b = synth.make_batch(6300 + 10 * kind, B, 2300, noise_px=0.5, depth_noise=0.02, outlier_frac=0.4, random_focal=RF.get(kind))
    cams = np.zeros(B, dtype=_capi.CAMERA_DTYPE)
    if kind == 3:
        cams["params"][:, 0] = 800.0
    c1, c2 = _cams(kind, cams)
    mono = kind <= 2
    ro = _capi.ransac_opt_from_dict(dict(RO, max_iterations=3000, min_iterations=3000))
    bo = _capi.bundle_opt_from_dict(BO)
    h = _capi.Handle(0)
    try:
        def run(env):
            _set_env(monkeypatch, env)
            r, m = h.estimate_batch(kind, b["x1"], b["x2"], b["d1"] if mono else None, b["d2"] if mono else None, ro, bo, None, c1, c2)
            return r.copy(), m.copy()

        ref, ref_mask = run({"MDRP_CHUNKS": "0", "MDRP_LO_OVERLAP": "0"})
        assert int(ref["iterations"].min()) == 3000 and int(ref["num_inliers"].min()) > 300
        for env in SCHEDULES:
            res, mask = run(env)
            bad = [i for i in range(B) if _differs(res[i:i + 1], ref[i:i + 1])]
            assert not bad, (kind, B, env, bad[:16], [_differs(res[i:i + 1], ref[i:i + 1]) for i in bad[:4]])
            assert np.array_equal(mask, ref_mask), (kind, B, env, np.flatnonzero((mask != ref_mask).any(axis=1)))
    finally:
        h.close()
