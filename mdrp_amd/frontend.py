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

`poselib.sample_dense_torch` / `estimate_dense_torch` are the front end for DENSE matchers (include/mdrp_dense.h): a warp of rows
(xA, yA, xB, yB) and its certainty instead of keypoints and index pairs.  `sample_dense_numpy` at the end of this module is their definition, rules
D1-D7 of the header: pixel coordinates, rules 2-4 above as the candidate test, integer weights from the certainty, a stratified draw, a
density-balanced second draw, the records.  Every quantity that decides a pick is an integer, so the device equals it as bytes.

`poselib.reconstruct_pairs_torch` / `reconstruct_image_pairs_torch` are the BACK end (include/mdrp_reconstruct.h): from the estimators'
models and the pairs' depth maps to the fused two-view point cloud in camera 2's frame.  `reconstruct_pair_numpy` and `reconstruct_image_pairs_numpy`
at the end of this module are their definition, rules R1-R7 of the header: the usable-model rule, the pixel order, the integer subsample, the depth
filter, the unprojection and the transform in float64 with one rounding per arithmetic sign, the rows and their truncation.

`poselib.scene_transforms_torch` / `reconstruct_scene_torch` chain an image set's pairs along a tree and fuse ONE cloud per scene
(include/mdrp_scene.h).  `scene_transforms_numpy` and `reconstruct_scene_numpy` at the end of this module are their definition, rules
S1-S6 of the header: the tree and its detached images, the accumulation leaf upward in float64 without a fused multiply-add, R3-R5 on a stage of
their own with the image mixed into the seed, the rows in image order and the int64 offsets.

`poselib.covisibility_pairs_torch` / `covisibility_image_pairs_torch` judge a pair by its depth maps (include/mdrp_covis.h): 16 integer
counts per pair.  `covisibility_pair_numpy` and `covisibility_image_pairs_numpy` at the end of this module are their definition, rules C1-C7 of the
header: R3's subsample on two stages of its own, the point carried into the other camera's frame, the nearest target pixel, the three-way comparison
of depths, all in float64 with one rounding per arithmetic sign.
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


# ---- the front end for dense matchers (include/mdrp_dense.h): a warp sampled by certainty.  Rules D1-D7 of the header, for one pair.
# Every quantity that decides a pick is an integer (weights, the 24-bit stratum offsets, running sums, cell counts): the device result equals this
# statement as bytes whatever order a parallel scan or an atomic adds in.
COORDS = ("normalized", "pixel")
DENSE_MAX_ROWS, DENSE_MAX_STAGE1, DENSE_MAX_N, DENSE_MAX_GRID = 1 << 22, 65536, 16384, 8
_M32 = 0xFFFFFFFF


def dense_pixel_coord(v, extent, coords="normalized"):
    """D1: float64 pixel coordinate of float32 / float64 warp values in an image `extent` wide (or high)"""
    if coords not in COORDS:
        raise ValueError(f"coords must be one of {COORDS}, not {coords!r}")
    with np.errstate(invalid="ignore"):
        v = np.asarray(v).astype(np.float64)
        return (v + 1.0) * (0.5 * float(extent)) if coords == "normalized" else v


def dense_weight(certainty, threshold=0.05):
    """D2 (the certainty's part) and D3: uint32 weights; 0 where the certainty is not finite or not above zero, otherwise
    min(65536, max(1, floor(c' * 65536))) with c' = 1 above the threshold"""
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.asarray(certainty).astype(np.float64)
        ok = np.isfinite(c) & (c > 0.0)
        cp = np.where(c > float(threshold), 1.0, c)
        f = np.floor(np.where(ok, cp, 0.0) * 65536.0)
    q = np.minimum(65536.0, np.maximum(1.0, f)).astype(np.uint32)
    return np.where(ok, q, np.uint32(0)).astype(np.uint32)


def lowbias32(x):
    """the 32-bit integer hash of D4 on uint32 values (array or scalar): uint32 array"""
    x = np.atleast_1d(np.asarray(x, dtype=np.uint64)) & _M32  # (uint64 holds every 32 x 32-bit product)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & _M32
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & _M32
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def dense_u(seed, stage, k):
    """D4: the 24-bit stratum offset of draw k (array) for a seed and a stage; only the seed's low 32 bits count"""
    k = np.atleast_1d(np.asarray(k, dtype=np.uint64))
    x = ((int(seed) & _M32) * 0x9E3779B1 + int(stage) * 0x85EBCA77) & _M32
    return lowbias32((np.uint64(x) + k) & _M32) >> np.uint32(8)


def dense_position(k, S, M, u):
    """D4: P_k = (k * S + ((u_k * S) >> 24)) div M in uint64 (S <= 2^38, k < M <= 2^16, u < 2^24: below 2^63)"""
    k = np.atleast_1d(np.asarray(k, dtype=np.uint64))
    u = np.atleast_1d(np.asarray(u, dtype=np.uint64))
    S, M = np.uint64(S), np.uint64(M)
    return (k * S + ((u * S) >> np.uint64(24))) // M


def stratified_draw(weights, M, stage, seed):
    """D4: indices picked by the stratified draw of M from integer weights (sum > 0 unless M == 0), ascending, duplicates of the predecessor dropped"""
    w = np.asarray(weights, dtype=np.uint64)
    if M <= 0 or len(w) == 0:
        return np.zeros(0, dtype=np.int64)
    cum = np.cumsum(w, dtype=np.uint64)
    k = np.arange(M, dtype=np.uint64)
    P = dense_position(k, cum[-1], M, dense_u(seed, stage, k))
    pick = np.searchsorted(cum, P, side="right").astype(np.int64)  # the smallest i whose inclusive running sum exceeds P
    keep = np.ones(M, dtype=bool)
    keep[1:] = pick[1:] != pick[:-1]
    return pick[keep]


def dense_cell(xi1, yi1, xi2, yi2, w1, h1, w2, h2, grid):
    """D6: the 4-D cell of integer pixel indices as one index below grid^4"""
    g = int(grid)
    a, b = np.asarray(xi1, dtype=np.int64) * g // int(w1), np.asarray(yi1, dtype=np.int64) * g // int(h1)
    c, d = np.asarray(xi2, dtype=np.int64) * g // int(w2), np.asarray(yi2, dtype=np.int64) * g // int(h2)
    return ((a * g + b) * g + c) * g + d


def dense_cell_weight(count, min_count=2):
    """D6: (1 << 20) div count where count >= min_count, else 1"""
    count = np.asarray(count, dtype=np.int64)
    return np.where(count >= int(min_count), (1 << 20) // np.maximum(count, 1), 1).astype(np.uint64)


def check_dense_arguments(rows, n, expansion, grid, min_count):
    """the limits the host refuses (D4, D6)"""
    if not 0 <= int(rows) <= DENSE_MAX_ROWS:
        raise ValueError(f"a pair's warp has at most 2^22 rows, not {rows}")
    if not 1 <= int(n) <= DENSE_MAX_N:
        raise ValueError(f"n must be 1 .. {DENSE_MAX_N}, not {n}")
    if int(expansion) < 1 or int(expansion) * int(n) > DENSE_MAX_STAGE1:
        raise ValueError(f"expansion must be at least 1 and expansion * n at most {DENSE_MAX_STAGE1}")
    if not 1 <= int(grid) <= DENSE_MAX_GRID:
        raise ValueError(f"grid must be 1 .. {DENSE_MAX_GRID}, not {grid}")
    if int(min_count) < 1:
        raise ValueError("min_count must be at least 1")


def dense_candidates(warp, certainty, depth_map1, depth_map2, coords="normalized", threshold=0.05, filter="both_inf"):
    """D1-D3 for one pair: (q (R,) uint32 weights, 0 for a non-candidate; p1, p2 (R, 2) float64 pixel coordinates; pixel indices xi1, yi1, xi2, yi2;
    d1, d2 (R,) float64 depths, 0 where the points are not inside)"""
    wp, ct = _table(warp, "warp"), _table(certainty, "certainty")
    dm1, dm2 = _table(depth_map1, "depth maps"), _table(depth_map2, "depth maps")
    if dm1.ndim != 2 or dm2.ndim != 2 or wp.shape[-1] != 4 or wp.size != 4 * ct.size:
        raise ValueError("expected warp (R, 4) or (Hc, Wc, 4), certainty with one value per row and depth maps (H, W)")
    wp, ct = wp.reshape(-1, 4), ct.reshape(-1)
    (h1, w1), (h2, w2) = dm1.shape, dm2.shape
    p1 = np.stack([dense_pixel_coord(wp[:, 0], w1, coords), dense_pixel_coord(wp[:, 1], h1, coords)], axis=1)
    p2 = np.stack([dense_pixel_coord(wp[:, 2], w2, coords), dense_pixel_coord(wp[:, 3], h2, coords)], axis=1)
    in1, xi1, yi1 = pixel_index(p1[:, 0], p1[:, 1], w1, h1)                               # rule 2
    in2, xi2, yi2 = pixel_index(p2[:, 0], p2[:, 1], w2, h2)
    ok = in1 & in2 & bool(dm1.size > 0 and dm2.size > 0)                                 # (a map without pixels has no row inside)
    d1 = np.zeros(len(ct)); d2 = np.zeros(len(ct))
    d1[ok] = dm1[yi1[ok], xi1[ok]].astype(np.float64)                                    # rule 3
    d2[ok] = dm2[yi2[ok], xi2[ok]].astype(np.float64)
    ok &= keep_depths(d1, d2, filter)                                                    # rule 4
    q = np.where(ok, dense_weight(ct, threshold), np.uint32(0)).astype(np.uint32)        # D2, D3
    return q, p1, p2, (xi1, yi1, xi2, yi2), d1, d2


def sample_dense_numpy(warp, certainty, depth_map1, depth_map2, n, seed=0, coords="normalized", threshold=0.05, balanced=True, expansion=4, grid=8,
                       min_count=2, filter="both_inf", ranked=False, center1=None, center2=None):
    """One pair: warp (R, 4) or (Hc, Wc, 4) rows (xA, yA, xB, yB), certainty (R,) or (Hc, Wc), depth maps (H, W), all float32 / float64.
    Returns (x1 (m, 2), x2 (m, 2), d1 (m,), d2 (m,) float64, rows (m,) int32, score (m,) float64), m <= n: the records of the sampled rows in
    ascending row order, or (ranked) in descending certainty with ties by ascending row.  This function is the definition (D1-D7)."""
    ct = np.asarray(certainty).reshape(-1)
    check_dense_arguments(ct.size, n, expansion, grid, min_count)
    q, p1, p2, (xi1, yi1, xi2, yi2), d1, d2 = dense_candidates(warp, certainty, depth_map1, depth_map2, coords, threshold, filter)
    K = int(np.count_nonzero(q))
    M1 = min((int(expansion) if balanced else 1) * int(n), K)                             # D5
    rows = stratified_draw(q, M1, 1, seed)
    if balanced and len(rows):                                                            # D6
        (h1, w1), (h2, w2) = np.asarray(depth_map1).shape, np.asarray(depth_map2).shape
        cell = dense_cell(xi1[rows], yi1[rows], xi2[rows], yi2[rows], w1, h1, w2, h2, grid)
        count = np.bincount(cell, minlength=int(grid) ** 4)[cell]
        rows = rows[stratified_draw(dense_cell_weight(count, min_count), min(int(n), len(rows)), 2, seed)]
    score = ct[rows].astype(np.float64)
    if ranked:                                                                            # D7: rule 6's order on the raw certainty
        o = score_order(score)
        rows, score = rows[o], score[o]
    c1 = np.zeros(2) if center1 is None else np.asarray(center1, dtype=np.float64).reshape(2)
    c2 = np.zeros(2) if center2 is None else np.asarray(center2, dtype=np.float64).reshape(2)
    return p1[rows] - c1, p2[rows] - c2, d1[rows], d2[rows], rows.astype(np.int32), score


def pad_dense_pairs(sampled, n):
    """per-pair results of sample_dense_numpy -> the padded buffers the device writes: x1, x2 (B, n, 2), d1, d2 (B, n), n_per_pair (B,) int32,
    rows (B, n) int32, score (B, n); behind the count x = 0, d = 1, rows = -1, score = 0"""
    B = len(sampled)
    x1 = np.zeros((B, n, 2)); x2 = np.zeros((B, n, 2)); d1 = np.ones((B, n)); d2 = np.ones((B, n))
    cnt = np.zeros(B, dtype=np.int32)
    rows = np.full((B, n), -1, dtype=np.int32)
    score = np.zeros((B, n))
    for b, (a1, a2, e1, e2, r, s) in enumerate(sampled):
        m = cnt[b] = len(r)
        x1[b, :m] = a1; x2[b, :m] = a2; d1[b, :m] = e1; d2[b, :m] = e2; rows[b, :m] = r; score[b, :m] = s
    return x1, x2, d1, d2, cnt, rows, score


# ---- the back end (include/mdrp_reconstruct.h): the fused two-view point cloud of a pair from its model and its two depth maps.  Rules
# R1-R7 of the header, for one pair.  Whether a pixel is kept is decided by integers (the hash of its coordinates against a threshold) and a test of
# its depth; a kept pixel's point is a fixed sequence of float64 operations, one rounding per arithmetic sign, rounded once to float32: the device
# result equals this statement as bytes.
KINDS = ("calibrated", "shared_focal", "varying_focal")
KEEPS = ("not_inf", "finite")
RECON_ALL, RECON_MAX_EXTENT = 0xFFFFFFFF, 65536
RECON_STAGES = (3, 4)  # D4's stage of image 1 | image 2 (1 and 2 are the dense sampler's)


def recon_threshold(rate):
    """R3: a rate to the integer threshold: floor(rate * 2^32) for 0 < rate < 1, "all" for rate >= 1; rate <= 0 or NaN is refused"""
    rate = float(rate)
    if not rate > 0.0:
        raise ValueError(f"rate must be above 0, not {rate!r}")
    return RECON_ALL if rate >= 1.0 else int(np.floor(rate * 4294967296.0))


def recon_hash(seed, stage, v, u):
    """R3: uint32 hash of pixels (v, u) (arrays) for a seed and a stage; only the seed's low 32 bits count"""
    k = (np.asarray(v, dtype=np.uint64) << np.uint64(16)) | np.asarray(u, dtype=np.uint64)
    x = ((int(seed) & _M32) * 0x9E3779B1 + int(stage) * 0x85EBCA77) & _M32
    return lowbias32((np.uint64(x) + k) & _M32).reshape(np.shape(k))


def recon_candidates(h, w, thr, seed, stage):
    """R3: (h, w) bool, True where the pixel is a candidate"""
    if h > RECON_MAX_EXTENT or w > RECON_MAX_EXTENT:
        raise ValueError(f"a map extent is at most {RECON_MAX_EXTENT}")
    if not 1 <= int(thr) <= RECON_ALL:
        raise ValueError("thr must be 1 .. 0xFFFFFFFF")
    if int(thr) == RECON_ALL or h * w == 0:
        return np.ones((h, w), dtype=bool)
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return recon_hash(seed, stage, v, u) < np.uint32(thr)


def recon_keep(d, keep="not_inf"):
    """R4 on float64 depths"""
    if keep not in KEEPS:
        raise ValueError(f"keep must be one of {KEEPS}, not {keep!r}")
    return np.isfinite(d) if keep == "finite" else ~np.isinf(d)


def recon_usable(m, kind):
    """R1: the model (a MODEL_DTYPE scalar) can be reconstructed from"""
    with np.errstate(invalid="ignore"):
        ok = bool(np.isfinite(m["q"]).all() and np.isfinite(m["t"]).all() and np.isfinite([m["scale"], m["shift1"], m["shift2"]]).all() and m["scale"] != 0.0)
        if kind != "calibrated":
            ok = ok and bool(np.isfinite(m["f1"]) and np.isfinite(m["f2"]) and m["f1"] > 0.0 and m["f2"] > 0.0)
    return ok


def _recon_intrinsics(m, kind, side, camera):
    """(1 / fx, 1 / fy, cx, cy) of R5 for image `side`: from the camera (a record or dict with model_id 0 {f, cx, cy} | 1 {fx, fy, cx, cy} and params)
    for the calibrated kind, from the model's focal otherwise (the principal point is the centre's business there)"""
    if kind != "calibrated":
        f = np.float64(m["f2"] if side else m["f1"])
        return np.float64(1.0) / f, np.float64(1.0) / f, np.float64(0.0), np.float64(0.0)
    if camera is None:
        raise ValueError("the calibrated kind needs both cameras")
    mid, p = int(camera["model_id"]), np.asarray(camera["params"], dtype=np.float64)
    if mid not in (0, 1):
        raise ValueError("only SIMPLE_PINHOLE (0) and PINHOLE (1) cameras")
    fx, fy, cx, cy = (p[0], p[1], p[2], p[3]) if mid == 1 else (p[0], p[0], p[1], p[2])
    return np.float64(1.0) / fx, np.float64(1.0) / fy, cx, cy


def _quat_rows(q):
    """R6: R from q = (w, x, y, z), the expressions of poselib._quat_to_R as they are written there"""
    w, x, y, z = (np.float64(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _recon_unproject(v, u, d, c, rx, ry, cx, cy, shift):
    """R5 for kept pixels (v, u) with depths d: (n, 3) float64, every line one rounding per sign"""
    x = u.astype(np.float64) - c[0]
    y = v.astype(np.float64) - c[1]
    xn = (x - cx) * rx
    yn = (y - cy) * ry
    z = d + shift
    return np.stack([xn * z, yn * z, z], axis=1)


def reconstruct_side_numpy(model, kind, side, depth_map, center=None, camera=None, keep="not_inf", thr=RECON_ALL, seed=0):
    """R2-R6 for one image of one pair whose model is usable: (points (n, 3) FLOAT64 in camera 2's frame, before R7's rounding; v (n,), u (n,) int64,
    the kept pixels in row-major order).  side 0 is image 1 (transformed), side 1 is image 2 (as it stands)."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, not {kind!r}")
    dm = _table(depth_map, "depth maps")
    if dm.ndim != 2:
        raise ValueError("expected a depth map (H, W)")
    h, w = dm.shape
    m = np.asarray(model).reshape(())
    with np.errstate(all="ignore"):
        d_all = dm.astype(np.float64)                                                     # R4 (float -> double is exact)
        kept = recon_candidates(h, w, thr, seed, RECON_STAGES[side]) & recon_keep(d_all, keep)
        v, u = np.nonzero(kept)                                                           # R2: row-major
        d = d_all[v, u]
        c = np.zeros(2) if center is None else np.asarray(center, dtype=np.float64).reshape(2)
        rx, ry, cx, cy = _recon_intrinsics(m, kind, side, camera)
        X = _recon_unproject(v, u, d, c, rx, ry, cx, cy, np.float64(m["shift2"] if side else m["shift1"]))
        if side == 0:                                                                     # R6
            R, t, inv = _quat_rows(m["q"]), np.asarray(m["t"], dtype=np.float64), np.float64(1.0) / np.float64(m["scale"])
            X = np.stack([inv * (((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r]) for r in range(3)], axis=1)
    return X.reshape(-1, 3), v.astype(np.int64), u.astype(np.int64)


def reconstruct_rows_numpy(model, kind, depth_map1, depth_map2, center1=None, center2=None, camera1=None, camera2=None, keep="not_inf", thr=RECON_ALL,
                           seed=0, w_alloc1=None, w_alloc2=None):
    """R1-R6 and R7's rounding for one pair: ((points1 (n1, 3) float32, pixel1 (n1,) int32), (points2, pixel2)), every kept point of image 1 and of
    image 2 in pixel order; both empty where the model is not usable"""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, not {kind!r}")
    if keep not in KEEPS:
        raise ValueError(f"keep must be one of {KEEPS}, not {keep!r}")
    m = np.asarray(model).reshape(())
    sides = []
    for side, (dm, c, cam, wa) in enumerate(((depth_map1, center1, camera1, w_alloc1), (depth_map2, center2, camera2, w_alloc2))):
        wa = np.shape(dm)[1] if wa is None else int(wa)
        if recon_usable(m, kind):                                                          # R1
            X, v, u = reconstruct_side_numpy(m, kind, side, dm, c, cam, keep, thr, seed)
        else:
            X, v, u = np.zeros((0, 3)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        with np.errstate(over="ignore", invalid="ignore"):
            sides.append((X.astype(np.float32), (v * wa + u).astype(np.int32)))          # R7: one rounding, to nearest
    return tuple(sides)


def pack_rows(sides, p_max=None):
    """R7's placement: the two images' kept rows -> (points (p_max, 3) float32, pixel (p_max,) int32, counts (2,) int32); p_max None = n1 + n2.
    Rows are written while they fit, image 2's behind image 1's; the counts are the true ones; behind the last written row 0, 0, 0 and -1."""
    n1, n2 = len(sides[0][1]), len(sides[1][1])
    p_max = n1 + n2 if p_max is None else int(p_max)
    if p_max < 0:
        raise ValueError("p_max must not be negative")
    points, pixel = np.zeros((p_max, 3), dtype=np.float32), np.full(p_max, -1, dtype=np.int32)
    start = 0
    for P, px in sides:
        k = min(len(px), p_max - start)
        points[start:start + k] = P[:k]; pixel[start:start + k] = px[:k]
        start += k
    return points, pixel, np.array([n1, n2], dtype=np.int32)


def reconstruct_pair_numpy(model, kind, depth_map1, depth_map2, center1=None, center2=None, camera1=None, camera2=None, keep="not_inf", thr=RECON_ALL,
                           seed=0, p_max=None, w_alloc1=None, w_alloc2=None):
    """One pair: model (a MODEL_DTYPE scalar), depth maps (h, w) float32 / float64, centres (2,) or None, cameras (calibrated kind) as records or
    dicts with model_id and params.  Returns (points (p_max, 3) float32, pixel (p_max,) int32, counts (2,) int32) by R1-R7; p_max None = n1 + n2;
    w_alloc: the allocated row length `pixel` counts rows by, None = the map's width.  This function is the definition."""
    return pack_rows(reconstruct_rows_numpy(model, kind, depth_map1, depth_map2, center1, center2, camera1, camera2, keep, thr, seed, w_alloc1, w_alloc2),
                     p_max)


def reconstruct_image_pairs_numpy(models, kind, depth_maps, pairs, p_max, centers=None, sizes=None, cameras1=None, cameras2=None, keep="not_inf",
                                  thr=RECON_ALL, seed=0):
    """models (B,) MODEL_DTYPE, depth_maps (I, H, W) float32 / float64, pairs (B, 2) image indices (a, c); sizes (I, 2) (h, w) clamped to the
    allocation, None = all of it; centers (I, 2) or (2,); cameras1 / cameras2: one per PAIR (calibrated kind).  Pair b is reconstruct_pair_numpy on
    the two images' valid regions with w_alloc = W; a pair with an index outside [0, I) is empty.  Returns (points (B, p_max, 3) float32, pixel
    (B, p_max) int32, counts (B, 2) int32)."""
    dm = _table(depth_maps, "depth maps")
    if dm.ndim != 3:
        raise ValueError("expected depth maps (I, H, W)")
    I, H, W = dm.shape
    pairs = np.asarray(pairs).astype(np.int32).reshape(-1, 2)
    models = np.asarray(models).reshape(-1)
    if len(models) != len(pairs):
        raise ValueError("one model per pair")
    hw = np.tile(np.array([H, W], dtype=np.int64), (I, 1)) if sizes is None else np.asarray(sizes).reshape(I, 2)
    hs, ws = clamp_extent(hw[:, 0], H), clamp_extent(hw[:, 1], W)
    cs = None if centers is None else np.asarray(centers, dtype=np.float64)
    if cs is not None and cs.size == 2:
        cs = np.tile(cs.reshape(1, 2), (I, 1))
    if cs is not None and cs.shape != (I, 2):
        raise ValueError("centers must have shape (I, 2) or (2,)")
    B, p_max = len(pairs), int(p_max)
    points, pixel = np.zeros((B, p_max, 3), dtype=np.float32), np.full((B, p_max), -1, dtype=np.int32)
    counts = np.zeros((B, 2), dtype=np.int32)
    for b, (a, c) in enumerate(pairs):
        if not (image_valid(a, I) and image_valid(c, I)):
            continue
        points[b], pixel[b], counts[b] = reconstruct_pair_numpy(
            models[b], kind, dm[a][:hs[a], :ws[a]], dm[c][:hs[c], :ws[c]], None if cs is None else cs[a], None if cs is None else cs[c],
            None if cameras1 is None else cameras1[b], None if cameras2 is None else cameras2[b], keep, thr, seed, p_max, W, W)
    return points, pixel, counts


# ---- a scene (include/mdrp_scene.h): the pairs of an image set chained along a tree, every image unprojected once into the frame of
# its root.  Rules S1-S6 of the header.  The tree is walked in a fixed order and every product and sum of the accumulation is rounded on its own, so
# the transform records, and with them the points, are defined as bytes.
SCENE_STAGE = 5          # R3's stage for a scene (3 and 4 are the two-view back end's)
SCENE_ABSENT, SCENE_EDGE, SCENE_ROOT = 0, 1, 2  # tree[i][1], the role
SCENE_SEED_MUL = 0xC2B2AE35
SCENE_TRANSFORM_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("s", "<f8"), ("f", "<f8"), ("shift", "<f8"), ("root", "<i4"), ("depth", "<i4")])
assert SCENE_TRANSFORM_DTYPE.itemsize == 128  # mdrp_scene_transform


def scene_seed(seed, image):
    """S3: the seed of image `image`: lowbias32(seed + 0xC2B2AE35 * (image + 1)) in uint32 arithmetic; R3's hash takes it in the seed's place"""
    return int(lowbias32(((int(seed) & _M32) + SCENE_SEED_MUL * (int(image) + 1)) & _M32)[0])


def _scene_edge(models, kind, pairs, tree, I, i):
    """S1 for image i: None where it is absent or detached by its own entry, else (role, the other image of its pair or -1, R (3, 3), t (3,), s, the
    image's own f, its own shift), the edge that takes a point of image i's camera to the other image's: (R X + t) / s"""
    one, zero = np.float64(1.0), np.float64(0.0)
    p, role = int(tree[i][0]), int(tree[i][1])
    if role not in (SCENE_EDGE, SCENE_ROOT):
        return None
    if role == SCENE_ROOT and p == -1:
        return (SCENE_ROOT, -1, np.eye(3), np.zeros(3), one, zero, zero) if kind == "calibrated" else None
    if not 0 <= p < len(pairs):
        return None
    a, c = int(pairs[p][0]), int(pairs[p][1])
    if a == c or i not in (a, c):
        return None
    other = c if i == a else a
    if not image_valid(other, I):
        return None
    m = models[p]
    if not recon_usable(m, kind):
        return None
    first = i == a
    shift = np.float64(m["shift1"] if first else m["shift2"])
    f = zero if kind == "calibrated" else np.float64(m["f1"] if first else m["f2"])
    if role == SCENE_ROOT:
        return SCENE_ROOT, other, np.eye(3), np.zeros(3), one, f, shift
    R, t, scale = _quat_rows(m["q"]), np.asarray(m["t"], dtype=np.float64), np.float64(m["scale"])
    if first:                                                                             # the model itself: X_c = (R X_a + t) / scale
        return SCENE_EDGE, other, R, t, scale, f, shift
    inv = one / scale                                                                     # its inverse: X_a = (R^T X_c - (R^T t) inv) / inv
    ti = np.array([-(((R[0, r] * t[0] + R[1, r] * t[1]) + R[2, r] * t[2]) * inv) for r in range(3)])
    return SCENE_EDGE, other, np.ascontiguousarray(R.T), ti, inv, f, shift


def _scene_compose(Re, te, se, R, t, s):
    """S2: the edge e behind the accumulated (R, t, s): R' = Re R with each sum taken left to right, t' = Re t + s te, s' = s se"""
    Rn = np.array([[(Re[r, 0] * R[0, c] + Re[r, 1] * R[1, c]) + Re[r, 2] * R[2, c] for c in range(3)] for r in range(3)])
    tn = np.array([((Re[r, 0] * t[0] + Re[r, 1] * t[1]) + Re[r, 2] * t[2]) + s * te[r] for r in range(3)])
    return Rn, tn, s * se


def scene_transforms_numpy(models, kind, pairs, tree, n_images):
    """S1 and S2: models (B,) MODEL_DTYPE, pairs (B, 2) image indices (a, c), tree (I, 2) (pair, role) -> (I,) SCENE_TRANSFORM_DTYPE.  The record of
    an absent or detached image is zeros with root = depth = -1.  This function is the definition."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, not {kind!r}")
    I = int(n_images)
    pairs = np.asarray(pairs).astype(np.int64).reshape(-1, 2)
    tree = np.asarray(tree).astype(np.int64).reshape(I, 2)
    models = np.asarray(models).reshape(-1)
    if len(models) != len(pairs):
        raise ValueError("one model per pair")
    out = np.zeros(I, dtype=SCENE_TRANSFORM_DTYPE)
    out["root"] = out["depth"] = -1
    with np.errstate(all="ignore"):
        edges = [_scene_edge(models, kind, pairs, tree, I, i) for i in range(I)]
        for i, e in enumerate(edges):
            if e is None:
                continue
            role, node, R, t, s, f, shift = e
            root, depth = (i, 0) if role == SCENE_ROOT else (-1, 1)
            if role == SCENE_EDGE:
                for _ in range(I):                                                        # the walk is cut after I steps: a cycle ends as detached
                    en = edges[node]
                    if en is None:
                        break
                    if en[0] == SCENE_ROOT:
                        root = node
                        break
                    R, t, s = _scene_compose(en[2], en[3], en[4], R, t, s)
                    depth += 1
                    node = en[1]
            if root < 0:
                continue
            out[i] = (R.reshape(9), t, s, f, shift, root, depth)
    return out


def scene_unproject(transform, kind, v, u, d, center=None, camera=None):
    """S5: pixels (v, u) (arrays; an integer pixel is its own coordinate) with float64 depths d of an image with record `transform` -> (n, 3) float64
    in the image's own camera frame, by R5's lines with the image's own focal and shift"""
    T = np.asarray(transform).reshape(())
    c = np.zeros(2) if center is None else np.asarray(center, dtype=np.float64).reshape(2)
    rx, ry, cx, cy = _recon_intrinsics({"f1": T["f"], "f2": T["f"]}, kind, 0, camera)
    return _recon_unproject(np.asarray(v), np.asarray(u), d, c, rx, ry, cx, cy, np.float64(T["shift"]))


def scene_transform_points(transform, X):
    """S6: points X (n, 3) float64 of an image's camera frame into its root's frame; a root's points are X as it stands"""
    T = np.asarray(transform).reshape(())
    if T["depth"] == 0:
        return X
    R, t, inv = T["R"].reshape(3, 3), T["t"], np.float64(1.0) / np.float64(T["s"])
    return np.stack([(((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r]) * inv for r in range(3)], axis=1).reshape(-1, 3)


def scene_image_rows_numpy(transform, kind, image, depth_map, center=None, camera=None, keep="not_inf", thr=RECON_ALL, seed=0, w_alloc=None):
    """S3-S6 for one attached image: (points (n, 3) float32 in its root's frame, pixel (n,) int32), every kept pixel in row-major order"""
    dm = _table(depth_map, "depth maps")
    h, w = dm.shape
    T = np.asarray(transform).reshape(())
    wa = w if w_alloc is None else int(w_alloc)
    with np.errstate(all="ignore"):
        d_all = dm.astype(np.float64)
        kept = recon_candidates(h, w, thr, scene_seed(seed, image), SCENE_STAGE) & recon_keep(d_all, keep)      # S3, S4
        v, u = np.nonzero(kept)
        X = scene_transform_points(T, scene_unproject(T, kind, v, u, d_all[v, u], center, camera))
        return X.reshape(-1, 3).astype(np.float32), (v * wa + u).astype(np.int32)                                # S6: one rounding


def pack_scene_rows(rows, p_max=None):
    """S6's placement: per image (points, pixel) or None -> (points (p_max, 3) float32, pixel (p_max,) int32, offsets (I + 1,) int64); p_max None =
    every row.  Rows are written while they fit; the offsets are the true ones; behind the last written row 0, 0, 0 and -1."""
    n = [0 if r is None else len(r[1]) for r in rows]
    offsets = np.concatenate([[0], np.cumsum(n, dtype=np.int64)]).astype(np.int64)
    p_max = int(offsets[-1]) if p_max is None else int(p_max)
    if p_max < 0:
        raise ValueError("p_max must not be negative")
    points, pixel = np.zeros((p_max, 3), dtype=np.float32), np.full(p_max, -1, dtype=np.int32)
    for r, start in zip(rows, offsets[:-1]):
        if r is None or start >= p_max:
            continue
        k = min(len(r[1]), p_max - int(start))
        points[start:start + k] = r[0][:k]; pixel[start:start + k] = r[1][:k]
    return points, pixel, offsets


def scene_rows_numpy(transforms, kind, depth_maps, centers=None, sizes=None, cameras=None, keep="not_inf", thr=RECON_ALL, seed=0):
    """per image the kept rows of scene_image_rows_numpy on its valid region, None for an absent or detached image"""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, not {kind!r}")
    if keep not in KEEPS:
        raise ValueError(f"keep must be one of {KEEPS}, not {keep!r}")
    dm = _table(depth_maps, "depth maps")
    if dm.ndim != 3:
        raise ValueError("expected depth maps (I, H, W)")
    I, H, W = dm.shape
    if len(transforms) != I:
        raise ValueError("one transform per image")
    hw = np.tile(np.array([H, W], dtype=np.int64), (I, 1)) if sizes is None else np.asarray(sizes).reshape(I, 2)
    hs, ws = clamp_extent(hw[:, 0], H), clamp_extent(hw[:, 1], W)
    cs = None if centers is None else np.asarray(centers, dtype=np.float64)
    if cs is not None and cs.size == 2:
        cs = np.tile(cs.reshape(1, 2), (I, 1))
    if cs is not None and cs.shape != (I, 2):
        raise ValueError("centers must have shape (I, 2) or (2,)")
    if kind == "calibrated" and (cameras is None or len(cameras) != I):
        raise ValueError("the calibrated kind needs one camera per image")
    return [None if transforms[i]["depth"] < 0 else
            scene_image_rows_numpy(transforms[i], kind, i, dm[i][:hs[i], :ws[i]], None if cs is None else cs[i], None if cameras is None else cameras[i],
                                   keep, thr, seed, W) for i in range(I)]


def reconstruct_scene_numpy(models, kind, depth_maps, pairs, tree, p_max=None, centers=None, sizes=None, cameras=None, keep="not_inf", thr=RECON_ALL,
                            seed=0):
    """models (B,) MODEL_DTYPE, depth_maps (I, H, W) float32 / float64, pairs (B, 2), tree (I, 2) (pair, role); sizes (I, 2) clamped to the
    allocation; centers (I, 2) or (2,); cameras: one per IMAGE (calibrated kind), records or dicts with model_id and params.  Returns (points
    (p_max, 3) float32, pixel (p_max,) int32 = v * W + u, offsets (I + 1,) int64, transforms (I,) SCENE_TRANSFORM_DTYPE) by S1-S6; p_max None =
    every row.  This function is the definition."""
    I = np.shape(depth_maps)[0]
    T = scene_transforms_numpy(models, kind, pairs, tree, I)
    return (*pack_scene_rows(scene_rows_numpy(T, kind, depth_maps, centers, sizes, cameras, keep, thr, seed), p_max), T)


# ---- co-visibility (include/mdrp_covis.h): how far a pair's two depth maps agree under its model.  Rules C1-C7 of the header.  A sampled
# pixel of the source image is unprojected (R5), carried into the target camera's frame, projected to the nearest pixel of the target map, and its
# depth there is compared with the target's own.  Every count is an integer and every quantity that decides one is a fixed sequence of float64
# operations, one rounding per arithmetic sign: the device result equals this statement as bytes.
COVIS_STAGES = (6, 7)  # C3: R3's stage of direction 0 | direction 1 (1 and 2: the dense sampler's, 3 and 4: the two-view cloud's, 5: the scene's)
COVIS_SLOTS = 8
COVIS_CLASSES = ("sampled", "front", "inside", "known", "consistent", "occluded", "violating")  # C7: the slot of each class, and its bit in a class mask


def covis_band(tol):
    """(lo, hi) = (1.0 - tol, 1.0 + tol) of C6, computed once here so that the device never derives them; 0 <= tol <= 1"""
    tol = float(tol)
    if not 0.0 <= tol <= 1.0:
        raise ValueError(f"tol must be in [0, 1], not {tol!r}")
    return 1.0 - tol, 1.0 + tol


def _covis_check_band(lo, hi):
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 <= lo <= 1.0 <= hi):
        raise ValueError(f"lo and hi must be finite with 0 <= lo <= 1 <= hi, not {lo!r}, {hi!r}")
    return np.float64(lo), np.float64(hi)


def _covis_focals(m, kind, side, camera):
    """(fx, fy) a point is projected with into image `side` (C5): the camera's for the calibrated kind, the model's focal otherwise"""
    if kind != "calibrated":
        f = np.float64(m["f2"] if side else m["f1"])
        return f, f
    mid, p = int(camera["model_id"]), np.asarray(camera["params"], dtype=np.float64)
    return (p[0], p[1]) if mid == 1 else (p[0], p[0])


def covisibility_direction_numpy(model, kind, direction, depth_src, depth_tgt, center_src=None, center_tgt=None, camera_src=None, camera_tgt=None,
                                 thr=RECON_ALL, seed=0, lo=0.95, hi=1.05):
    """C3-C6 for one direction of one pair whose model is usable: (v (n,), u (n,) int64: the SAMPLED source pixels in row-major order; classes (n,)
    uint8: bit k set iff the pixel is in class COVIS_CLASSES[k]; vt, ut (n,) int64: the target pixel of an INSIDE one, 0 elsewhere).  direction 0:
    the source is image 1 and the target image 2; direction 1 the other way round."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, not {kind!r}")
    lo, hi = _covis_check_band(lo, hi)
    src, tgt = _table(depth_src, "depth maps"), _table(depth_tgt, "depth maps")
    if src.ndim != 2 or tgt.ndim != 2:
        raise ValueError("expected depth maps (H, W)")
    s, t = int(direction), 1 - int(direction)
    m = np.asarray(model).reshape(())
    (h, w), (ht, wt) = src.shape, tgt.shape
    shift_s, shift_t = (np.float64(m["shift2"]), np.float64(m["shift1"])) if s else (np.float64(m["shift1"]), np.float64(m["shift2"]))
    with np.errstate(all="ignore"):
        d_all = src.astype(np.float64)
        sampled = recon_candidates(h, w, thr, seed, COVIS_STAGES[s]) & np.isfinite(d_all) & (d_all + shift_s > 0.0)  # C3
        v, u = np.nonzero(sampled)
        d = d_all[v, u]
        cs = np.zeros(2) if center_src is None else np.asarray(center_src, dtype=np.float64).reshape(2)
        ct = np.zeros(2) if center_tgt is None else np.asarray(center_tgt, dtype=np.float64).reshape(2)
        rx, ry, cx, cy = _recon_intrinsics(m, kind, s, camera_src)
        X = _recon_unproject(v, u, d, cs, rx, ry, cx, cy, shift_s)
        R, tr, scale = _quat_rows(m["q"]), np.asarray(m["t"], dtype=np.float64), np.float64(m["scale"])
        if s == 0:                                                                            # C4: R6
            inv = np.float64(1.0) / scale
            P = [inv * (((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + tr[r]) for r in range(3)]
        else:                                                                                 # C4: the inverse, sums left to right
            Y = [scale * X[:, r] - tr[r] for r in range(3)]
            P = [(R[0, r] * Y[0] + R[1, r] * Y[1]) + R[2, r] * Y[2] for r in range(3)]
        front = np.isfinite(P[2]) & (P[2] > 0.0)
        _, _, ox, oy = _recon_intrinsics(m, kind, t, camera_tgt)                              # C5
        fx, fy = _covis_focals(m, kind, t, camera_tgt)
        xo, yo = P[0] / P[2], P[1] / P[2]
        px, py = (xo * fx + ox) + ct[0], (yo * fy + oy) + ct[1]
        a, b = px + 0.5, py + 0.5
        inside = front & (a >= 0.0) & (a < np.float64(wt)) & (b >= 0.0) & (b < np.float64(ht))
        ut, vt = np.where(inside, a, 0.0).astype(np.int64), np.where(inside, b, 0.0).astype(np.int64)  # truncation
        dt = np.zeros(len(v))
        dt[inside] = tgt[vt[inside], ut[inside]].astype(np.float64)                           # C6: one read, of an INSIDE pixel alone
        zt = dt + shift_t
        known = inside & np.isfinite(dt) & (zt > 0.0)
        l, hgh = lo * zt, hi * zt
        consistent, occluded, violating = known & (P[2] >= l) & (P[2] <= hgh), known & (P[2] > hgh), known & (P[2] < l)
    classes = np.zeros(len(v), dtype=np.uint8)
    for k, member in enumerate((np.ones(len(v), dtype=bool), front, inside, known, consistent, occluded, violating)):
        classes |= (member.astype(np.uint8) << np.uint8(k))
    return v.astype(np.int64), u.astype(np.int64), classes, vt, ut


def covis_counts(classes):
    """C7: the (8,) int32 counters of one direction from its pixels' class masks"""
    classes = np.asarray(classes, dtype=np.uint8)
    return np.array([int(((classes >> k) & 1).sum()) for k in range(len(COVIS_CLASSES))] + [0], dtype=np.int32)


def covisibility_pair_numpy(model, kind, depth_map1, depth_map2, center1=None, center2=None, camera1=None, camera2=None, thr=RECON_ALL, seed=0,
                            lo=0.95, hi=1.05):
    """One pair: model (a MODEL_DTYPE scalar), depth maps (h, w) float32 / float64, centres (2,) or None, cameras (calibrated kind) as records or
    dicts with model_id and params; thr, seed: R3's; lo, hi: C6's band (covis_band(tol)).  Returns counts (2, 8) int32 by C1-C7: per direction
    sampled, front, inside, known, consistent, occluded, violating, 0; all zero where the model is not usable.  This function is the definition."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, not {kind!r}")
    _covis_check_band(lo, hi)
    m = np.asarray(model).reshape(())
    counts = np.zeros((2, COVIS_SLOTS), dtype=np.int32)
    if not recon_usable(m, kind):                                                             # C1
        return counts
    if kind == "calibrated" and (camera1 is None or camera2 is None):
        raise ValueError("the calibrated kind needs both cameras")
    sides = ((depth_map1, center1, camera1), (depth_map2, center2, camera2))
    for direction in range(2):                                                                # C2
        (ds, cs, ks), (dt, ct, kt) = sides[direction], sides[1 - direction]
        counts[direction] = covis_counts(covisibility_direction_numpy(m, kind, direction, ds, dt, cs, ct, ks, kt, thr, seed, lo, hi)[2])
    return counts


def covisibility_image_pairs_numpy(models, kind, depth_maps, pairs, centers=None, sizes=None, cameras1=None, cameras2=None, thr=RECON_ALL, seed=0,
                                   lo=0.95, hi=1.05):
    """models (B,) MODEL_DTYPE, depth_maps (I, H, W) float32 / float64, pairs (B, 2) image indices (a, c); sizes (I, 2) (h, w) clamped to the
    allocation, None = all of it; centers (I, 2) or (2,); cameras1 / cameras2: one per PAIR (calibrated kind).  Pair b is covisibility_pair_numpy on
    the two images' valid regions; a pair with an index outside [0, I) has all counters zero.  Returns counts (B, 2, 8) int32."""
    dm = _table(depth_maps, "depth maps")
    if dm.ndim != 3:
        raise ValueError("expected depth maps (I, H, W)")
    I, H, W = dm.shape
    pairs = np.asarray(pairs).astype(np.int32).reshape(-1, 2)
    models = np.asarray(models).reshape(-1)
    if len(models) != len(pairs):
        raise ValueError("one model per pair")
    hw = np.tile(np.array([H, W], dtype=np.int64), (I, 1)) if sizes is None else np.asarray(sizes).reshape(I, 2)
    hs, ws = clamp_extent(hw[:, 0], H), clamp_extent(hw[:, 1], W)
    cs = None if centers is None else np.asarray(centers, dtype=np.float64)
    if cs is not None and cs.size == 2:
        cs = np.tile(cs.reshape(1, 2), (I, 1))
    if cs is not None and cs.shape != (I, 2):
        raise ValueError("centers must have shape (I, 2) or (2,)")
    counts = np.zeros((len(pairs), 2, COVIS_SLOTS), dtype=np.int32)
    for b, (a, c) in enumerate(pairs):
        if not (image_valid(a, I) and image_valid(c, I)):
            continue
        counts[b] = covisibility_pair_numpy(models[b], kind, dm[a][:hs[a], :ws[a]], dm[c][:hs[c], :ws[c]], None if cs is None else cs[a],
                                            None if cs is None else cs[c], None if cameras1 is None else cameras1[b],
                                            None if cameras2 is None else cameras2[b], thr, seed, lo, hi)
    return counts


# ---- the consistency filter of a scene (include/mdrp_fuse.h): a scene's point stays if enough other images' depth maps confirm it and
# few enough see through it.  Rules F1-F6 of the header.  A candidate pixel's point in its root's frame (S5, S6 before the rounding) is carried into the
# camera frame of each of its image's views, projected to the nearest pixel there and compared with that map's own depth (C5, C6); the gate takes the
# numbers of consistent and of violating views.  Every quantity that decides is a fixed sequence of float64 operations, one rounding per arithmetic
# sign: the device result equals this statement as bytes.
FUSE_MAX_VIEWS = 8
FUSE_CLASSES = ("invalid", "not_front", "outside", "unknown", "consistent", "occluded", "violating")  # F5: what one slot says of one pixel (0: F3)


def fuse_valid_slots(transforms, views_row, i):
    """F3: per slot of image i's row of `views` the image it names, -1 where the slot is inert: an index outside [0, I), the image itself, an image
    that is not attached or hangs on another root, or one an earlier slot of the row holds.  Nothing is read through an inert slot."""
    I, out = len(transforms), []
    for n in (int(x) for x in np.asarray(views_row).reshape(-1)):
        ok = (0 <= n < I and n != i and transforms[n]["depth"] >= 0 and transforms[i]["depth"] >= 0 and transforms[n]["root"] == transforms[i]["root"]
              and n not in out)
        out.append(n if ok else -1)
    return out


def fuse_to_view(transform, Q):
    """F4: points Q (n, 3) float64 of a root's frame in the camera frame of the view with record `transform`: the inverse of the record, sums left
    to right; a root view's are Q as it stands"""
    T = np.asarray(transform).reshape(())
    if T["depth"] == 0:
        return [Q[:, 0], Q[:, 1], Q[:, 2]]
    R, t, s = T["R"].reshape(3, 3), T["t"], np.float64(T["s"])
    Y = [s * Q[:, r] - t[r] for r in range(3)]
    return [(R[0, r] * Y[0] + R[1, r] * Y[1]) + R[2, r] * Y[2] for r in range(3)]


def fuse_slot_numpy(transform, kind, P, depth_tgt, center_tgt=None, camera_tgt=None, lo=0.95, hi=1.05):
    """F4's FRONT and F5 for one view: points P (three (n,) float64 arrays) of the view's camera frame against its depth map (its valid region) ->
    (n,) uint8 indices into FUSE_CLASSES, none of them 0.  C5 and C6 with the view as the target."""
    T = np.asarray(transform).reshape(())
    tgt = _table(depth_tgt, "depth maps")
    ht, wt = tgt.shape
    ct = np.zeros(2) if center_tgt is None else np.asarray(center_tgt, dtype=np.float64).reshape(2)
    m = {"f1": T["f"], "f2": T["f"]}
    with np.errstate(all="ignore"):
        front = np.isfinite(P[2]) & (P[2] > 0.0)
        _, _, ox, oy = _recon_intrinsics(m, kind, 0, camera_tgt)
        fx, fy = _covis_focals(m, kind, 0, camera_tgt)
        xo, yo = P[0] / P[2], P[1] / P[2]
        px, py = (xo * fx + ox) + ct[0], (yo * fy + oy) + ct[1]
        a, b = px + 0.5, py + 0.5
        inside = front & (a >= 0.0) & (a < np.float64(wt)) & (b >= 0.0) & (b < np.float64(ht))
        ut, vt = np.where(inside, a, 0.0).astype(np.int64), np.where(inside, b, 0.0).astype(np.int64)
        dt = np.zeros(len(P[2]))
        dt[inside] = tgt[vt[inside], ut[inside]].astype(np.float64)
        zt = dt + np.float64(T["shift"])
        known = inside & np.isfinite(dt) & (zt > 0.0)
        l, hgh = lo * zt, hi * zt
        consistent, occluded, violating = known & (P[2] >= l) & (P[2] <= hgh), known & (P[2] > hgh), known & (P[2] < l)
    cls = np.full(len(P[2]), 1, dtype=np.uint8)
    for code, member in ((2, front), (3, inside), (4, consistent), (5, occluded), (6, violating)):
        cls[member] = code
    return cls


def fuse_image_support_numpy(transforms, kind, i, views_row, depth_maps, hs, ws, cs=None, cameras=None, keep="not_inf", thr=RECON_ALL, seed=0, lo=0.95,
                             hi=1.05):
    """F1-F5 for one attached image i: (Q (n, 3) float64: its candidates' points in the root's frame, before the rounding; v, u (n,) int64: the
    candidates, row-major; support (n, 2) uint8: (n_cons, n_viol); classes (n, V) uint8: per slot an index into FUSE_CLASSES).  depth_maps (I, H, W);
    hs, ws (I,): the valid regions; cs (I, 2) or None; cameras: per image or None."""
    lo, hi = _covis_check_band(lo, hi)
    T = transforms[i]
    cam = (lambda n: None if cameras is None else cameras[n])
    cen = (lambda n: None if cs is None else cs[n])
    slots = fuse_valid_slots(transforms, views_row, i)
    with np.errstate(all="ignore"):
        d_all = depth_maps[i][:hs[i], :ws[i]].astype(np.float64)
        kept = recon_candidates(int(hs[i]), int(ws[i]), thr, scene_seed(seed, i), SCENE_STAGE) & recon_keep(d_all, keep)   # F1: S3, S4
        v, u = np.nonzero(kept)
        d = d_all[v, u]
        Q = scene_transform_points(T, scene_unproject(T, kind, v, u, d, cen(i), cam(i))).reshape(-1, 3)
        tested = np.isfinite(d) & (d + np.float64(T["shift"]) > 0.0)                                                        # F2
        classes = np.zeros((len(v), len(slots)), dtype=np.uint8)
        for k, n in enumerate(slots):
            if n < 0:                                                                                                      # F3
                continue
            cls = fuse_slot_numpy(transforms[n], kind, fuse_to_view(transforms[n], Q), depth_maps[n][:hs[n], :ws[n]], cen(n), cam(n), lo, hi)
            classes[:, k] = np.where(tested, cls, 0)
    support = np.stack([(classes == 4).sum(axis=1), (classes == 6).sum(axis=1)], axis=1).astype(np.uint8).reshape(-1, 2)
    return Q, v.astype(np.int64), u.astype(np.int64), support, classes


def fuse_gate(support, min_consistent, max_violating):
    """F6: (n,) bool, the candidates the gate keeps"""
    s = np.asarray(support).reshape(-1, 2).astype(np.int64)
    return (s[:, 0] >= int(min_consistent)) & (s[:, 1] <= int(max_violating))


def pack_fuse_rows(rows, p_max=None):
    """F6's placement: per image (points, pixel, support) or None -> (points (p_max, 3) float32, pixel (p_max,) int32, support (p_max, 2) uint8,
    offsets (I + 1,) int64), as pack_scene_rows places its rows; the filler of support is 0, 0"""
    points, pixel, offsets = pack_scene_rows([None if r is None else r[:2] for r in rows], p_max)
    support = np.zeros((len(pixel), 2), dtype=np.uint8)
    for r, start in zip(rows, offsets[:-1]):
        if r is None or start >= len(pixel):
            continue
        k = min(len(r[1]), len(pixel) - int(start))
        support[start:start + k] = r[2][:k]
    return points, pixel, support, offsets


def fuse_rows_numpy(transforms, kind, depth_maps, views, centers=None, sizes=None, cameras=None, keep="not_inf", thr=RECON_ALL, seed=0, lo=0.95, hi=1.05,
                    min_consistent=1, max_violating=0):
    """per image the kept rows (points (n, 3) float32, pixel (n,) int32, support (n, 2) uint8) by F1-F6, None for an absent or detached image"""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, not {kind!r}")
    if keep not in KEEPS:
        raise ValueError(f"keep must be one of {KEEPS}, not {keep!r}")
    if int(min_consistent) < 0 or int(max_violating) < 0:
        raise ValueError("min_consistent and max_violating must not be negative")
    dm = _table(depth_maps, "depth maps")
    if dm.ndim != 3:
        raise ValueError("expected depth maps (I, H, W)")
    I, H, W = dm.shape
    if len(transforms) != I:
        raise ValueError("one transform per image")
    views = np.asarray(views).astype(np.int64)
    views = views.reshape(I, views.size // I if I and views.size else 0)
    if views.shape[1] > FUSE_MAX_VIEWS:
        raise ValueError(f"views has at most {FUSE_MAX_VIEWS} columns")
    hw = np.tile(np.array([H, W], dtype=np.int64), (I, 1)) if sizes is None else np.asarray(sizes).reshape(I, 2)
    hs, ws = clamp_extent(hw[:, 0], H), clamp_extent(hw[:, 1], W)
    cs = None if centers is None else np.asarray(centers, dtype=np.float64)
    if cs is not None and cs.size == 2:
        cs = np.tile(cs.reshape(1, 2), (I, 1))
    if cs is not None and cs.shape != (I, 2):
        raise ValueError("centers must have shape (I, 2) or (2,)")
    if kind == "calibrated" and (cameras is None or len(cameras) != I):
        raise ValueError("the calibrated kind needs one camera per image")
    rows = []
    for i in range(I):
        if transforms[i]["depth"] < 0:
            rows.append(None)
            continue
        Q, v, u, support, _ = fuse_image_support_numpy(transforms, kind, i, views[i], dm, hs, ws, cs, cameras, keep, thr, seed, lo, hi)
        g = fuse_gate(support, min_consistent, max_violating)                                                              # F6
        with np.errstate(over="ignore", invalid="ignore"):
            rows.append((Q[g].astype(np.float32), (v[g] * W + u[g]).astype(np.int32), support[g]))
    return rows


def fuse_scene_numpy(models, kind, depth_maps, pairs, tree, views, p_max=None, centers=None, sizes=None, cameras=None, keep="not_inf", thr=RECON_ALL,
                     seed=0, lo=0.95, hi=1.05, min_consistent=1, max_violating=0):
    """What reconstruct_scene_numpy takes, views (I, V) int32 with 0 <= V <= 8 - per image the images its points are tested against; a view need not
    be a partner of the image in `pairs` - C6's band lo, hi (covis_band(tol)) and the gate.  Returns (points (p_max, 3) float32, pixel (p_max,)
    int32, support (p_max, 2) uint8 = (n_cons, n_viol) per row, offsets (I + 1,) int64, transforms (I,) SCENE_TRANSFORM_DTYPE) by F1-F6; p_max None
    = every kept row.  With min_consistent = 0 and max_violating >= V the first, second and fourth are reconstruct_scene_numpy's.  This function is
    the definition."""
    I = np.shape(depth_maps)[0]
    T = scene_transforms_numpy(models, kind, pairs, tree, I)
    rows = fuse_rows_numpy(T, kind, depth_maps, views, centers, sizes, cameras, keep, thr, seed, lo, hi, min_consistent, max_violating)
    return (*pack_fuse_rows(rows, p_max), T)
