"""The glue of a step is scheduling only (run_pass, mdrp_capi.hip): the second chunk's solver behind k_prep instead of behind the first chunk's solver
(sched::second_solver_after, MDRP_SOLVE_BEHIND_PREP), one clear kernel in front of k_prep instead of a memset per block (Pass::clear_front,
MDRP_FRONT_CLEAR) and the scan of the later chunks from the exact sweep's lists instead of over every slot (k_scan_list, MDRP_SCAN_LIST) must leave
every record and every inlier mask of a resident-buffer call bit-identical to the old order, with the fused tail and without it.  Shapes: 130 pairs
(above the 128-pair threshold: first-chunk stage, k_bound and k_score_split run), ragged 3 / 37 / 257 / 300 correspondences, 600 iterations as
128 | 472 and as 128 | 256 | 216, every estimator whose second solver moves, hard and hopeless pairs, a run of several super-chunks (only the first
takes the new clear), and outlier-free pairs under a small capacity of the list scan (the pairs above it are walked in full)."""
import functools

import numpy as np
import pytest

B, NMAX = 130, 300
NS = (3, 37, 257, 300)
RF = {1: "shared", 2: "varying"}  # synth.make_pair random_focal per estimator
RO = {"max_epipolar_error": 2.0, "max_reproj_error": 16.0}
BO = {"loss_type": "TRUNCATED_CAUCHY"}
KNOBS = ("MDRP_CHUNKS", "MDRP_LO_OVERLAP", "MDRP_BOUND", "MDRP_FUSE_TAIL", "MDRP_PAIRS_PER_PASS", "MDRP_SOLVE_BEHIND_PREP", "MDRP_FRONT_CLEAR",
         "MDRP_SCAN_LIST", "MDRP_SCAN_LIST_CAP")
OLD = {"MDRP_SOLVE_BEHIND_PREP": "0", "MDRP_FRONT_CLEAR": "0", "MDRP_SCAN_LIST": "0"}
TWO, THREE = {}, {"MDRP_CHUNKS": "128,256"}  # 600 iterations: 128 | 472 by every estimator's default, 128 | 256 | 216

# (name, kind, shift solver, data, (max, min) iterations, environment)
CASES = [(f"kind{k}{'_shift' if sh else ''}_{'three' if env else 'two'}", k, sh, "mixed", (600, 600), env)
         for k, sh in ((0, False), (0, True), (1, False), (2, False)) for env in (TWO, THREE)]
CASES += [("kind3_two", 3, False, "mixed", (600, 600), TWO), ("kind5_two", 5, False, "mixed", (600, 600), TWO),
          ("outliers75", 0, False, "outliers75", (600, 600), TWO), ("hopeless_pairs", 0, False, "hopeless", (600, 600), TWO),
          ("super_chunks", 0, False, "outliers75", (100000, 1000), TWO)]
# more candidates than the list scan takes: outlier-free pairs of 300 correspondences (every hypothesis is a good one, records keep falling), and a
# capacity of 0, 1 and 4 candidates per pair, so that the pairs above it are walked in full by the same launch
CASES += [(f"clean_cap{cap}", 0, False, "clean", (600, 600), {"MDRP_SCAN_LIST_CAP": str(cap)}) for cap in (0, 1, 4)]


@functools.lru_cache(maxsize=None)
def _data(kind, what):
    """130 ragged pairs, zero-padded to NMAX.  mixed: 20 / 35 / 50 % outliers by pair; outliers75: 75 %; hopeless: every fifth pair has no
    geometry at all (second image and depths drawn at random: no trigger beyond the first record)"""
    from mdrp_amd import _capi, synth
    rng = np.random.default_rng(7300 + kind)
    ns = np.array([NS[i % 4] for i in range(B)], dtype=np.int32)
    rng.shuffle(ns)
    if what == "clean":
        ns[:] = NMAX
    x1, x2 = np.zeros((B, NMAX, 2)), np.zeros((B, NMAX, 2))
    d1, d2 = np.ones((B, NMAX)), np.ones((B, NMAX))
    for i in range(B):
        n = int(ns[i])
        frac = {"outliers75": 0.75, "clean": 0.0}.get(what, (0.2, 0.35, 0.5)[i % 3])
        p = synth.make_pair(73000 + 1000 * kind + i, n, noise_px=0.5, depth_noise=0.02, outlier_frac=frac, random_focal=RF.get(kind))
        x1[i, :n], x2[i, :n], d1[i, :n], d2[i, :n] = p["x1"], p["x2"], p["d1"], p["d2"]
        if what == "hopeless" and i % 5 == 0:
            x2[i, :n] = rng.uniform(-600.0, 600.0, (n, 2))
            d2[i, :n] = rng.uniform(1.0, 10.0, n)
    cams = np.zeros(B, dtype=_capi.CAMERA_DTYPE)
    cams["params"][:, 0] = 800.0
    return ns, x1, x2, d1, d2, cams


def _differs(a, b):
    return [f for f in a.dtype.names if a[f].tobytes() != b[f].tobytes()]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,shift,what,its,env", CASES, ids=[c[0] for c in CASES])
def test_new_order_and_front_clear_leave_records_and_masks_bit_identical(monkeypatch, name, kind, shift, what, its, env):
    import torch
    from mdrp_amd import _capi
    ns, x1, x2, d1, d2, cams = _data(kind, what)
    mono = kind <= 2
    c1, c2 = (cams, cams) if kind in (0, 3) else (None, None)
    ro = _capi.ransac_opt_from_dict(dict(RO, max_iterations=its[0], min_iterations=its[1], monodepth_estimate_shift=shift))
    bo = _capi.bundle_opt_from_dict(BO)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a).to(dev) for a in (x1, x2, d1, d2)]
    h = _capi.Handle(0)
    try:
        def run(extra):
            for k in KNOBS:
                monkeypatch.delenv(k, raising=False)
            for k, v in dict(env, **extra).items():
                monkeypatch.setenv(k, v)
            mask = torch.full((B, NMAX), 0xA5, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            h.estimate_batch_device(kind, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr() if mono else 0, t[3].data_ptr() if mono else 0, B, NMAX,
                                    ro, bo, ns, c1, c2, mask.data_ptr())
            res = h.fetch_results(B)
            return res.copy(), mask.cpu().numpy(), h.last_stats()

        new, new_mask, stats = run({})
        assert new.dtype == _capi.RESULT_DTYPE
        assert int(stats["first_chunk"]) == 128 and int(stats["fuse_timeouts"]) == 0
        variants = {"old order": OLD, "old solver order": {"MDRP_SOLVE_BEHIND_PREP": "0"}, "memsets": {"MDRP_FRONT_CLEAR": "0"},
                    "walked scan": {"MDRP_SCAN_LIST": "0"}, "whole list": {"MDRP_SCAN_LIST_CAP": "64"},
                    "unfused": {"MDRP_FUSE_TAIL": "0"}, "unfused, old order": dict(OLD, MDRP_FUSE_TAIL="0"), "new order again": {}}
        if its[0] != its[1]:  # (the long run: 100000 iterations for its hopeless pairs, so the whole old order, fused and not, and no more)
            variants = {k: variants[k] for k in ("old order", "unfused, old order")}
        for label, extra in variants.items():
            res, mask, _ = run(extra)
            bad = [i for i in range(B) if new[i:i + 1].tobytes() != res[i:i + 1].tobytes()]
            assert not bad, (name, label, bad[:16], [_differs(new[i:i + 1], res[i:i + 1]) for i in bad[:4]])
            assert new_mask.tobytes() == mask.tobytes(), (name, label, np.flatnonzero((new_mask != mask).any(axis=1))[:16])

        # not a comparison of empty results: the large pairs found their model, the pairs below the sample size did not run
        size = {3: 5, 5: 7}.get(kind, 3)
        ran = ns >= size if kind > 2 else ns >= 3
        assert (new["iterations"][~ran] == 0).all() and (new["iterations"][ran] >= min(its)).all()
        if its[0] == its[1]:
            assert (new["iterations"][ran] == its[0]).all()
        else:
            assert int(new["iterations"].max()) > its[1] + 1  # several super-chunks: some pair went on beyond the certain range
        good = (ns == 300) & (np.arange(B) % 5 != 0)
        assert float(np.median(new["num_inliers"][good])) > (40 if what == "outliers75" else 100), new["num_inliers"][good]
    finally:
        h.close()
