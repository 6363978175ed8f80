"""Inputs of tests/test_classic_frontend_host.py and tests/test_gpu_classic_frontend.py: batches of the baselines' device front end
(include/mdrp_classic_frontend.h).  A helper, not a test.

The pairs are those of tests/test_gpu_frontend.py (synth.make_pair correspondences scattered into keypoint tables through random permutations, NaN
and +-inf coordinates, indices at and past the table, one-sided and two-sided -1 rows planted where a pair has 64 rows or more) with the depth maps
dropped; the score patterns are tests/frontend_ranked_cases.PATTERNS, planted against the rows THIS front end keeps.  Row counts sit on the wavefront
(64) and tile (256) boundaries of the ordered compaction, on the 1024-row block and the 2048-key LDS tile of the ranked one, and kept-row counts
below and at each estimator's sample size (5, 6, 7)."""
import functools

import numpy as np

import frontend_ranked_cases as rc
import test_gpu_frontend as fe

KINDS = ("relpose_5pt", "shared_focal_6pt", "fundamental_7pt")
SAMPLE = {"relpose_5pt": 5, "shared_focal_6pt": 6, "fundamental_7pt": 7}
RO = dict(fe.RO)   # 200 certain iterations, thresholds for the 64 x 48 images
BO = dict(fe.BO)
ITERATIONS = {"relpose_5pt": 200, "shared_focal_6pt": 64, "fundamental_7pt": 300}  # (the 6-point solver is two orders slower than the others)


def options(kind, **more):
    it = ITERATIONS[kind]
    return dict(RO, max_iterations=it, min_iterations=it, **more)


def cameras(kind):
    """what estimate_baseline_* take for the kind: (cameras1, cameras2, pp)"""
    if kind == "relpose_5pt":
        return fe.CAM1, fe.CAM2, None
    return None, None, ((0.0, 0.0) if kind == "shared_focal_6pt" else None)


def make_batch(specs, first_seed, pad=7):
    """rc.make_batch without the maps: kp1, kp2, matches (int64), c1, c2"""
    b = rc.make_batch(specs, first_seed, pad)
    return {k: b[k] for k in ("kp1", "kp2", "matches", "c1", "c2", "specs")}


def shared_focal_tables(batch):
    """a copy of the batch for the 6-point estimator, which takes ONE focal length: image 2's keypoints rescaled about its principal point to image
    1's scale (NaN and +-inf coordinates stay what they are)"""
    out = dict(batch)
    with np.errstate(invalid="ignore"):
        out["kp2"] = (batch["kp2"] - np.array(fe.C2)) * (fe.A1 / fe.A2) + np.array(fe.C2)
    return out


def kept_rows(batch):
    """(B, M) bool: the rows the definition keeps (float32 and float64 tables hold the same finite / non-finite coordinates: the answer is one)"""
    from mdrp_amd import frontend
    B = len(batch["matches"])
    out = [np.stack([frontend.gather_point_matches_numpy(batch["kp1"][b].astype(t), batch["kp2"][b].astype(t), batch["matches"][b])[2] >= 0 for b in range(B)])
           for t in (np.float32, np.float64)]
    assert np.array_equal(out[0], out[1])
    return out[0]


def keep_only(batch, b, count):
    """leave pair b exactly `count` of its kept rows: the others become padding, two-sided and one-sided in turn"""
    kept = np.flatnonzero(kept_rows(batch)[b])
    assert len(kept) >= count
    gone = kept[count:]
    batch["matches"][b, gone[::2]] = -1
    batch["matches"][b, gone[1::2], 1] = -1


def twin(batch, kp_dtype, centres, scores=None):
    """the NumPy definition on the batch as the device sees it: x1, x2 (B, M, 2), n (B,), slot (B, M) of frontend.pad_point_pairs"""
    from mdrp_amd import frontend
    kp1, kp2 = batch["kp1"].astype(kp_dtype), batch["kp2"].astype(kp_dtype)
    B, M = batch["matches"].shape[:2]
    g = [frontend.gather_point_matches_numpy(kp1[b], kp2[b], batch["matches"][b], batch["c1"][b] if centres else None, batch["c2"][b] if centres else None,
                                             None if scores is None else scores[b]) for b in range(B)]
    return frontend.pad_point_pairs(g, M)


def scores_of(batch, offset=0, seed=0):
    """(B, M) float64 scores, one pattern of rc.PATTERNS per pair (rounded through float32 once)"""
    return rc.batch_scores(kept_rows(batch), offset, seed)


@functools.lru_cache(maxsize=None)
def batches():
    """name -> batch, built once.  B is 2 - 6.
      small    six pairs of 70 rows keeping 0, 1, 4, 5, 6 and 7 of them: below and at every sample size
      edges    63 / 64 / 65 and 255 / 256 / 257 rows
      long     about 600 rows beside a short pair
      m1024 / m1025, m2048 / m2049   M on and one past the ranked kernels' 1024-row rank block and 2048-key LDS tile"""
    small = make_batch([(70, None)] * 6, 100)
    for b, count in enumerate((0, 1, 4, 5, 6, 7)):
        keep_only(small, b, count)
    out = {"small": small,
           "edges": make_batch([(63, None), (64, None), (65, None), (255, None), (256, None), (257, None)], 120),
           "long": make_batch([(600, None), (130, None)], 140),
           "m1024": make_batch([(1000, None), (300, None)], 160, pad=24), "m1025": make_batch([(1000, None), (300, None)], 160, pad=25),
           "m2048": make_batch([(2040, None), (100, None)], 180, pad=8), "m2049": make_batch([(2040, None), (100, None)], 180, pad=9)}
    assert [out[k]["matches"].shape[1] for k in ("m1024", "m1025", "m2048", "m2049")] == [1024, 1025, 2048, 2049]
    return out


# ---- per-image tables: the pairs of tests/image_pairs_cases.py without the maps
IP_PAIRS = [0, 2, 6, 7, 9, 5, 8, 3]  # (0, 1) twice, a == c, an image index past the set, the 600-row pair, (4, 0), a negative image index, (0, 3): a count below K


@functools.lru_cache(maxsize=None)
def image_batch():
    """keypoints (I, K, 2), pairs (B, 2), matches (B, M, 2), kp_counts (two below K, one past it), centers: read-only"""
    import image_pairs_cases as ipc
    t = ipc.batch()
    return {"keypoints": t["keypoints"], "pairs": t["pairs"][IP_PAIRS], "matches": t["matches"][IP_PAIRS], "kp_counts": t["kp_counts"], "centers": t["centers"]}


def image_kept_rows(t, kp_dtype=np.float32):
    from mdrp_amd import frontend
    return frontend.gather_point_image_pairs_numpy(t["keypoints"].astype(kp_dtype), t["pairs"], t["matches"], kp_counts=t["kp_counts"])[3] >= 0


def expand_image_batch(t):
    """the per-pair tables of an image batch: kp1 = keypoints[a] and kp2 = keypoints[c], cut to nothing past the clamped counts by pointing every row
    past them at -1 (the per-pair descriptor has one k per side for the whole batch); a pair with an image index outside the set gets all -1 rows"""
    from mdrp_amd import frontend
    I, K = t["keypoints"].shape[:2]
    counts = frontend.clamp_extent(t["kp_counts"], K)
    B, M = t["matches"].shape[:2]
    kp1, kp2 = np.zeros((B, K, 2)), np.zeros((B, K, 2))
    matches = np.array(t["matches"], dtype=np.int64)
    c1, c2 = np.zeros((B, 2)), np.zeros((B, 2))
    for b, (a, c) in enumerate(t["pairs"]):
        if not (0 <= a < I and 0 <= c < I):
            matches[b] = -1
            continue
        kp1[b], kp2[b], c1[b], c2[b] = t["keypoints"][a], t["keypoints"][c], t["centers"][a], t["centers"][c]
        matches[b][(matches[b, :, 0] >= counts[a]) | (matches[b, :, 1] >= counts[c])] = -1
    return {"kp1": kp1, "kp2": kp2, "matches": matches, "c1": c1, "c2": c2}
