"""The device front end's definition, in plain NumPy for one image pair.

`poselib.gather_matches_torch` / `poselib.estimate_matches_torch` turn a matcher's output (two keypoint tables, index pairs) and two
depth maps into the estimators' correspondences on the GPU (mdrp_amd/csrc/mdrp_frontend.h).  This module states what they compute; it is
written from the definition in include/mdrp.h (ABI 0.6), it is the yardstick of the tests, and it is not used by the product path.

For match row m = (i, j), in row order:

1. the row is padding and dropped when i < 0 or j < 0; it is dropped as well when i >= K1 or j >= K2;
2. p1 = keypoints1[i], p2 = keypoints2[j]; the row is dropped unless x > -1, x < W, y > -1 and y < H hold for the floating value in its
   image (-0.5 is pixel 0, W - 0.001 is pixel W - 1; -1, W, NaN and +-inf are dropped); the pixel is the coordinate truncated toward zero;
3. d1 = depth_map1[yi1, xi1], d2 = depth_map2[yi2, xi2], widened to float64;
4. filter "both_inf" drops the row iff both depths are infinite (a NaN or a one-sided infinity is kept); "finite" keeps it only when
   both depths are finite;
5. kept rows, in match order, give x1 = float64(p1) - center1, x2 = float64(p2) - center2, d1, d2; slot[m] is the position of row m
   among the kept rows, -1 for a dropped row.

With `scores` (one per match row, higher is better: a matcher's confidence) the kept rows leave in QUALITY order instead of match order, the order
the progressive sampler (PROSAC) wants.  Rules 1-4 decide what is kept exactly as above: a score never drops or keeps a row.  Then

6. key(m) = float64(scores[m]) with NaN replaced by -inf; -0.0 and +0.0 are one key; rank(m) = the number of kept rows m' with key(m') > key(m), or
   key(m') == key(m) and m' < m: a stable descending sort of the kept rows' scores in match order (`score_order`).  slot[m] = rank(m), -1 for a
   dropped row, and the record of row m sits at index rank(m).

`poselib.gather_image_pairs_torch` / `estimate_image_pairs_torch` take the batch as its producer holds it: keypoints and depth maps once per
image, pairs as image indices (include/mdrp.h mdrp_image_pairs).  `gather_image_pairs_numpy` below states them as a loop over the pairs that
calls `gather_matches_numpy` on the two images' valid tables: that reduction is the definition.

`poselib.gather_point_matches_torch` / `estimate_baseline_matches_torch` and their per-image siblings are the front end of the 5- / 6- / 7-point
baselines, which have no depths (include/mdrp_classic_frontend.h): `gather_point_matches_numpy` / `gather_point_image_pairs_numpy`
state them.  Rule 1 is unchanged; rule 2 becomes "all four coordinates are finite" (no map to be inside of), rules 3 and 4 fall away, rules 5 and 6
hold without d1 and d2.
"""
import numpy as np

FILTERS = ("both_inf", "finite")


def pixel_index(x, y, width, height):
    """(in range, xi, yi) of float32 / float64 coordinates in a width x height map (rule 2); xi = yi = 0 where out of range"""
    x = np.asarray(x).astype(np.float64)
    y = np.asarray(y).astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = (x > -1.0) & (x < float(width)) & (y > -1.0) & (y < float(height))
    xi = np.trunc(np.where(inside, x, 0.0)).astype(np.int64)
    yi = np.trunc(np.where(inside, y, 0.0)).astype(np.int64)
    return inside, xi, yi


def keep_depths(d1, d2, filter="both_inf"):
    """the depth filter (rule 4) on float64 depths"""
    if filter not in FILTERS:
        raise ValueError(f"filter must be one of {FILTERS}, not {filter!r}")
    d1 = np.asarray(d1, dtype=np.float64)
    d2 = np.asarray(d2, dtype=np.float64)
    if filter == "finite":
        return np.isfinite(d1) & np.isfinite(d2)
    return ~(np.isinf(d1) & np.isinf(d2))


def _table(a, what):
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float64):
        raise ValueError(f"{what} must be float32 or float64")
    return a


def score_order(scores):
    """rule 6 on the scores of the kept rows, in match order: the position (among the kept rows) of the row at every rank — descending key, NaN as
    -inf, -0.0 = +0.0, ties by ascending position"""
    with np.errstate(invalid="ignore"):  # (a signalling NaN widens to a quiet one: NaN either way)
        key = np.array(scores, dtype=np.float64).reshape(-1)  # (a copy; float32 widens exactly)
    key[np.isnan(key)] = -np.inf
    key = key + 0.0  # -0.0 + 0.0 = +0.0
    return np.argsort(-key, kind="stable")


def _row_scores(scores, rows):
    s = np.asarray(scores)
    if s.dtype not in (np.float32, np.float64):
        raise ValueError("scores must be float32 or float64")
    if s.size != rows or s.ndim > 2 or (s.ndim == 2 and s.shape[0] != 1):
        raise ValueError(f"scores: expected one per match row ({rows}), got shape {s.shape}")
    return s.reshape(-1)


def gather_matches_numpy(keypoints1, keypoints2, matches, depth_map1, depth_map2, center1=None, center2=None, filter="both_inf", scores=None):
    """One pair: keypoints (K, 2) and depth maps (H, W) in float32 / float64, matches (M, 2) integers (taken as int32).
    Returns (x1 (n, 2), x2 (n, 2), d1 (n,), d2 (n,), slot (M,) int32), the first four float64; n = len(d1).
    scores: (M,) float32 / float64, one per match row, higher is better — the kept rows in rank order (rule 6), slot[m] the rank of row m."""
    kp1, kp2 = _table(keypoints1, "keypoints"), _table(keypoints2, "keypoints")
    dm1, dm2 = _table(depth_map1, "depth maps"), _table(depth_map2, "depth maps")
    if kp1.ndim != 2 or kp1.shape[1] != 2 or kp2.ndim != 2 or kp2.shape[1] != 2 or dm1.ndim != 2 or dm2.ndim != 2:
        raise ValueError("expected keypoints (K, 2) and depth maps (H, W)")
    m = np.asarray(matches).astype(np.int32).reshape(-1, 2).astype(np.int64)
    i, j = m[:, 0], m[:, 1]
    ok = (i >= 0) & (j >= 0) & (i < len(kp1)) & (j < len(kp2))                           # rule 1
    p1 = np.zeros((len(m), 2)); p2 = np.zeros((len(m), 2))
    p1[ok] = kp1[i[ok]].astype(np.float64); p2[ok] = kp2[j[ok]].astype(np.float64)
    in1, xi1, yi1 = pixel_index(p1[:, 0], p1[:, 1], dm1.shape[1], dm1.shape[0])       # rule 2 (float -> double is exact: the test is the same)
    in2, xi2, yi2 = pixel_index(p2[:, 0], p2[:, 1], dm2.shape[1], dm2.shape[0])
    ok &= in1 & in2
    d1 = np.zeros(len(m)); d2 = np.zeros(len(m))
    d1[ok] = dm1[yi1[ok], xi1[ok]].astype(np.float64)                                    # rule 3
    d2[ok] = dm2[yi2[ok], xi2[ok]].astype(np.float64)
    ok &= keep_depths(d1, d2, filter)                                                    # rule 4
    slot = np.where(ok, np.cumsum(ok) - 1, -1).astype(np.int32)                          # rule 5
    c1 = np.zeros(2) if center1 is None else np.asarray(center1, dtype=np.float64).reshape(2)
    c2 = np.zeros(2) if center2 is None else np.asarray(center2, dtype=np.float64).reshape(2)
    x1, x2, e1, e2 = p1[ok] - c1, p2[ok] - c2, d1[ok], d2[ok]
    if scores is None:
        return x1, x2, e1, e2, slot
    o = score_order(_row_scores(scores, len(m))[ok])                                    # rule 6: o[r] = kept position of the row at rank r
    rank = np.empty(len(o), dtype=np.int32)
    rank[o] = np.arange(len(o), dtype=np.int32)
    slot[ok] = rank
    return x1[o], x2[o], e1[o], e2[o], slot


def pad_pairs(gathered, m_max):
    """per-pair results of gather_matches_numpy -> the padded buffers the device front end writes: x1, x2 (B, m_max, 2), d1, d2 (B, m_max),
    n (B,) int32, slot (B, m_max) int32; slots past n hold x = 0, d = 1"""
    B = len(gathered)
    x1 = np.zeros((B, m_max, 2)); x2 = np.zeros((B, m_max, 2)); d1 = np.ones((B, m_max)); d2 = np.ones((B, m_max))
    n = np.zeros(B, dtype=np.int32)
    slot = np.full((B, m_max), -1, dtype=np.int32)
    for b, (a1, a2, e1, e2, s) in enumerate(gathered):
        n[b] = len(e1)
        x1[b, :n[b]] = a1; x2[b, :n[b]] = a2; d1[b, :n[b]] = e1; d2[b, :n[b]] = e2
        slot[b, :len(s)] = s
    return x1, x2, d1, d2, n, slot


# ---- per-image tables (include/mdrp.h mdrp_image_pairs): keypoints and depth maps exist once per image, a pair is two image indices
def image_valid(a, n_images):
    """an image index addresses the set: a in [0, n_images)"""
    a = np.asarray(a, dtype=np.int64)
    return (a >= 0) & (a < int(n_images))


def clamp_extent(v, maximum):
    """a per-image extent (a kp_count, the h or w of a size) against the allocated one: clamped to [0, maximum]"""
    return np.clip(np.asarray(v, dtype=np.int64), 0, int(maximum))


def gather_image_pairs_numpy(keypoints, depth_maps, pairs, matches, centers=None, sizes=None, kp_counts=None, filter="both_inf", scores=None):
    """keypoints (I, K, 2) and depth_maps (I, H, W) in float32 / float64, pairs (B, 2) image indices (a, c), matches (B, M, 2) integers.
    sizes (I, 2) (h, w) and kp_counts (I,): the valid part of each image's map and table, clamped to the allocation, None = all of it;
    centers (I, 2) or (2,).  Pair b is gather_matches_numpy on image a's and image c's valid tables; a pair with an index outside [0, I) is
    empty.  Returns pad_pairs of the per-pair results: x1, x2 (B, M, 2), d1, d2 (B, M), n (B,) int32, slot (B, M) int32.
    scores: (B, M) float32 / float64, one per match row — every pair in rank order (gather_matches_numpy's rule 6)."""
    if filter not in FILTERS:
        raise ValueError(f"filter must be one of {FILTERS}, not {filter!r}")
    kp, dm = _table(keypoints, "keypoints"), _table(depth_maps, "depth maps")
    if kp.ndim != 3 or kp.shape[2] != 2 or dm.ndim != 3 or len(dm) != len(kp):
        raise ValueError("expected keypoints (I, K, 2) and depth maps (I, H, W)")
    I, K = kp.shape[:2]
    H, W = dm.shape[1:]
    pairs = np.asarray(pairs).astype(np.int32).reshape(-1, 2)
    matches = np.asarray(matches)
    if matches.ndim != 3 or len(matches) != len(pairs) or matches.shape[2] != 2:
        raise ValueError("expected matches (B, M, 2) with the pairs' B")
    M = matches.shape[1]
    if scores is not None:
        scores = np.asarray(scores)
        if scores.dtype not in (np.float32, np.float64) or scores.shape != (len(pairs), M):
            raise ValueError("scores must be (B, M) float32 or float64, one per match row")
    counts = np.full(I, K, dtype=np.int64) if kp_counts is None else clamp_extent(np.asarray(kp_counts).reshape(I), K)
    hw = np.tile(np.array([H, W], dtype=np.int64), (I, 1)) if sizes is None else np.asarray(sizes).reshape(I, 2)
    hs, ws = clamp_extent(hw[:, 0], H), clamp_extent(hw[:, 1], W)
    cs = None if centers is None else np.asarray(centers, dtype=np.float64)
    if cs is not None and cs.size == 2:
        cs = np.tile(cs.reshape(1, 2), (I, 1))
    if cs is not None and cs.shape != (I, 2):
        raise ValueError("centers must have shape (I, 2) or (2,)")
    empty = (np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0), np.zeros(0), np.full(M, -1, dtype=np.int32))
    gathered = []
    for b, (a, c) in enumerate(pairs):
        if not (image_valid(a, I) and image_valid(c, I)):
            gathered.append(empty)
            continue
        gathered.append(gather_matches_numpy(kp[a][:counts[a]], kp[c][:counts[c]], matches[b], dm[a][:hs[a], :ws[a]], dm[c][:hs[c], :ws[c]],
                                             None if cs is None else cs[a], None if cs is None else cs[c], filter,
                                             None if scores is None else scores[b]))
    return pad_pairs(gathered, M)


# ---- the front end without depth maps (include/mdrp_classic_frontend.h): the 5- / 6- / 7-point baselines take correspondences alone
def gather_point_matches_numpy(keypoints1, keypoints2, matches, center1=None, center2=None, scores=None):
    """One pair: keypoints (K, 2) in float32 / float64, matches (M, 2) integers (taken as int32).  A row is kept iff both indices address their
    tables and the four coordinates are finite.  Returns (x1 (n, 2), x2 (n, 2) float64, slot (M,) int32): gather_matches_numpy's return minus the
    depths.  scores: (M,) float32 / float64 — the kept rows in rank order (rule 6), slot[m] the rank of row m."""
    kp1, kp2 = _table(keypoints1, "keypoints"), _table(keypoints2, "keypoints")
    if kp1.ndim != 2 or kp1.shape[1] != 2 or kp2.ndim != 2 or kp2.shape[1] != 2:
        raise ValueError("expected keypoints (K, 2)")
    m = np.asarray(matches).astype(np.int32).reshape(-1, 2).astype(np.int64)
    i, j = m[:, 0], m[:, 1]
    ok = (i >= 0) & (j >= 0) & (i < len(kp1)) & (j < len(kp2))                           # rule 1
    p1 = np.zeros((len(m), 2)); p2 = np.zeros((len(m), 2))
    p1[ok] = kp1[i[ok]].astype(np.float64); p2[ok] = kp2[j[ok]].astype(np.float64)
    ok &= np.isfinite(p1).all(axis=1) & np.isfinite(p2).all(axis=1)                      # rule 2 without a map: finite coordinates
    slot = np.where(ok, np.cumsum(ok) - 1, -1).astype(np.int32)
    c1 = np.zeros(2) if center1 is None else np.asarray(center1, dtype=np.float64).reshape(2)
    c2 = np.zeros(2) if center2 is None else np.asarray(center2, dtype=np.float64).reshape(2)
    x1, x2 = p1[ok] - c1, p2[ok] - c2
    if scores is None:
        return x1, x2, slot
    o = score_order(_row_scores(scores, len(m))[ok])                                    # rule 6
    rank = np.empty(len(o), dtype=np.int32)
    rank[o] = np.arange(len(o), dtype=np.int32)
    slot[ok] = rank
    return x1[o], x2[o], slot


def pad_point_pairs(gathered, m_max):
    """pad_pairs without depths: per-pair results of gather_point_matches_numpy -> x1, x2 (B, m_max, 2), n (B,) int32, slot (B, m_max) int32;
    slots past n hold x = 0"""
    B = len(gathered)
    x1 = np.zeros((B, m_max, 2)); x2 = np.zeros((B, m_max, 2))
    n = np.zeros(B, dtype=np.int32)
    slot = np.full((B, m_max), -1, dtype=np.int32)
    for b, (a1, a2, s) in enumerate(gathered):
        n[b] = len(a1)
        x1[b, :n[b]] = a1; x2[b, :n[b]] = a2
        slot[b, :len(s)] = s
    return x1, x2, n, slot


def gather_point_image_pairs_numpy(keypoints, pairs, matches, centers=None, kp_counts=None, scores=None):
    """keypoints (I, K, 2) in float32 / float64, pairs (B, 2) image indices (a, c), matches (B, M, 2) integers; kp_counts (I,) clamped to [0, K],
    None = K; centers (I, 2) or (2,).  Pair b is gather_point_matches_numpy on image a's and image c's valid tables; a pair with an index outside
    [0, I) is empty.  Returns pad_point_pairs of the per-pair results: x1, x2 (B, M, 2), n (B,) int32, slot (B, M) int32.  scores: (B, M)."""
    kp = _table(keypoints, "keypoints")
    if kp.ndim != 3 or kp.shape[2] != 2:
        raise ValueError("expected keypoints (I, K, 2)")
    I, K = kp.shape[:2]
    pairs = np.asarray(pairs).astype(np.int32).reshape(-1, 2)
    matches = np.asarray(matches)
    if matches.ndim != 3 or len(matches) != len(pairs) or matches.shape[2] != 2:
        raise ValueError("expected matches (B, M, 2) with the pairs' B")
    M = matches.shape[1]
    if scores is not None:
        scores = np.asarray(scores)
        if scores.dtype not in (np.float32, np.float64) or scores.shape != (len(pairs), M):
            raise ValueError("scores must be (B, M) float32 or float64, one per match row")
    counts = np.full(I, K, dtype=np.int64) if kp_counts is None else clamp_extent(np.asarray(kp_counts).reshape(I), K)
    cs = None if centers is None else np.asarray(centers, dtype=np.float64)
    if cs is not None and cs.size == 2:
        cs = np.tile(cs.reshape(1, 2), (I, 1))
    if cs is not None and cs.shape != (I, 2):
        raise ValueError("centers must have shape (I, 2) or (2,)")
    empty = (np.zeros((0, 2)), np.zeros((0, 2)), np.full(M, -1, dtype=np.int32))
    gathered = []
    for b, (a, c) in enumerate(pairs):
        if not (image_valid(a, I) and image_valid(c, I)):
            gathered.append(empty)
            continue
        gathered.append(gather_point_matches_numpy(kp[a][:counts[a]], kp[c][:counts[c]], matches[b], None if cs is None else cs[a],
                                                   None if cs is None else cs[c], None if scores is None else scores[b]))
    return pad_point_pairs(gathered, M)
