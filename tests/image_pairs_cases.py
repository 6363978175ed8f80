"""The batch of tests/test_gpu_image_pairs.py and of the degeneracy guard in tests/test_image_pairs_host.py: pairs as indices into five images.

I = 5 images whose tables are allocated K = 700 keypoints and 48 x 72 depths each; every image has its own valid size (a kernel that takes
the valid width for the row stride, or swaps h and w, reads wrong depths) and two of them a keypoint count below K.  The pairs repeat an
image on both sides, repeat a pair, use one image twice and hold two indices outside the set.  Correspondences are made as in
tests/test_gpu_frontend.py: synth.make_pair, scaled into the two images' valid regions, placed through random permutations into a segment of
each image's keypoint table, their depths painted into that image's ONE map (a later keypoint on the same pixel wins: the earlier one
becomes an outlier).  Images 1 and 4 take part in more rows than K: the 600-row pair is laid first, at the end of its tables, and the other
pairs' segments, filled from the front, overwrite some of its entries, which become its outliers.  The planted edge cases go, after all
painting, into rows that are still their pair's own."""
import numpy as np

I, K, H, W = 5, 700, 48, 72
SIZES = np.array([(48, 64), (40, 72), (48, 72), (33, 50), (40, 64)], dtype=np.int32)  # valid (h, w) of each map
KP_COUNTS = np.array([K, 650, K + 5, 120, K], dtype=np.int32)                        # two below K, one past it (clamped)
PAIRS = np.array([(0, 1), (1, 0), (2, 2), (0, 3), (3, 4), (4, 0), (0, 1), (5, 0), (-1, 2), (1, 4)], dtype=np.int32)
ROW_COUNTS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 600)
M = 607
BAD = (7, 8)  # the pairs with an image index outside [0, I)
RO = {"max_iterations": 200, "min_iterations": 200, "max_epipolar_error": 0.1, "max_reproj_error": 0.8}
BO = {"loss_type": "TRUNCATED_CAUCHY"}


def image_scale(i):
    """pixel = scale * synth pixel + centre: a camera with focal scale * 800 and its principal point at the middle of the valid region"""
    h, w = (int(v) for v in SIZES[i])
    return 0.035 * min(w / 64.0, h / 48.0), np.array([w / 2.0, h / 2.0])


CENTERS = np.stack([image_scale(i)[1] for i in range(I)]) + np.arange(I)[:, None] * 0.125
CAMERAS = [{"model": "SIMPLE_PINHOLE", "width": int(SIZES[i][1]), "height": int(SIZES[i][0]), "params": [image_scale(i)[0] * 800.0, *image_scale(i)[1]]}
           for i in range(I)]


def _pixel(p):
    return int(p[1]), int(p[0])


def make_batch():
    """dict of float64 / integer NumPy arrays: keypoints (I, K, 2), depth_maps (I, H, W), matches (B, M, 2) int64, pairs, sizes, kp_counts, centers"""
    from mdrp_amd import synth
    rng = np.random.default_rng(4100)
    kp = np.zeros((I, K, 2))
    dm = rng.uniform(1.0, 6.0, (I, H, W))
    for i in range(I):
        h, w = SIZES[i]
        kp[i] = np.stack([rng.uniform(0, w - 1, K), rng.uniform(0, h - 1, K)], 1)
    owner = np.full((I, K), -1)       # the pair whose keypoint sits in an entry (the last writer)
    painter = np.full((I, H, W), -1)  # the pair that painted a pixel last
    cursor = [0] * I
    matches = np.full((len(PAIRS), M, 2), -1, dtype=np.int64)
    points = {}
    for b in [9] + list(range(9)):
        (a, c), rows = PAIRS[b], ROW_COUNTS[b]
        if b in BAD:  # no image to put anything into: rows that look like any other pair's
            matches[b, :rows] = rng.integers(0, K, (rows, 2))
            continue
        p = synth.make_pair(7300 + b, rows, noise_px=0.5, depth_noise=0.02, outlier_frac=0.2)
        idx = []
        for side, img in ((1, a), (2, c)):
            scale, centre = image_scale(img)
            pt = scale * p[f"x{side}"] + centre
            start = K - rows if b == 9 else cursor[img]
            cursor[img] += 0 if b == 9 else rows
            assert start + rows <= K
            at = start + rng.permutation(rows)
            kp[img, at] = pt
            owner[img, at] = b
            h, w = SIZES[img]
            inside = (pt[:, 0] >= 0) & (pt[:, 0] < w - 1) & (pt[:, 1] >= 0) & (pt[:, 1] < h - 1)
            for m in np.flatnonzero(inside):
                dm[img][_pixel(pt[m])] = p[f"d{side}"][m]
                painter[img][_pixel(pt[m])] = b
            idx.append(at)
            points[b, side] = (pt, inside)
        matches[b, :rows] = np.stack(idx, 1)
    used = [set() for _ in range(I)]
    for b, ((a, c), rows) in enumerate(zip(PAIRS, ROW_COUNTS)):
        if b in BAD or rows < 64:
            continue
        (pt1, in1), (pt2, in2) = points[b, 1], points[b, 2]
        i, j = matches[b, :rows, 0], matches[b, :rows, 1]
        own = (owner[a, i] == b) & (owner[c, j] == b) & in1 & in2 & (i < min(KP_COUNTS[a], K)) & (j < min(KP_COUNTS[c], K))
        planted = []
        for m in rng.permutation(np.flatnonzero(own)):  # 24 rows of the pair's own, on pixels it painted last and no other planted row uses
            q1, q2 = _pixel(pt1[m]), _pixel(pt2[m])
            if len(planted) < 24 and painter[a][q1] == b and painter[c][q2] == b and q1 not in used[a] and q2 not in used[c] and (a != c or q1 != q2):
                planted.append(m); used[a].add(q1); used[c].add(q2)
        assert len(planted) == 24, (b, len(planted))
        r = iter(planted)
        h1, w1 = (int(v) for v in SIZES[a])
        h2, w2 = (int(v) for v in SIZES[c])
        d1 = lambda m: (a,) + _pixel(pt1[m])  # noqa: E731
        d2 = lambda m: (c,) + _pixel(pt2[m])  # noqa: E731
        m = next(r); dm[d1(m)] = np.inf; dm[d2(m)] = np.inf            # both infinite: dropped
        m = next(r); dm[d1(m)] = -np.inf; dm[d2(m)] = np.inf
        m = next(r); dm[d1(m)] = np.inf                                  # one-sided: kept by "both_inf", dropped by "finite"
        m = next(r); dm[d2(m)] = -np.inf
        m = next(r); dm[d1(m)] = np.nan                                  # NaN depth: likewise
        m = next(r); dm[d2(m)] = np.nan
        m = next(r); dm[d1(m)] = np.nan; dm[d2(m)] = np.inf
        for x in (-0.5, -1.0, w1 - 0.001, float(w1), np.nan, np.inf):    # coordinates at the edges of image a's VALID width ...
            kp[a, matches[b, next(r), 0], 0] = x
        for y in (-0.5, -1.0, h2 - 0.001, float(h2), np.nan, -np.inf):   # ... and of image c's valid height
            kp[c, matches[b, next(r), 1], 1] = y
        matches[b, next(r), 0] = K                                       # index == K
        matches[b, next(r), 1] = K
        matches[b, next(r), 1] = -1                                      # one-sided -1
        matches[b, next(r), 0] = -7
        matches[b, rng.choice(np.setdiff1d(np.arange(rows), planted), 3, replace=False)] = -1  # padding rows in mid-list
    out = {"keypoints": kp, "depth_maps": dm, "matches": matches, "pairs": PAIRS.copy(), "sizes": SIZES.copy(), "kp_counts": KP_COUNTS.copy(),
           "centers": CENTERS.copy()}
    for v in out.values():
        v.setflags(write=False)
    return out


_batch = None
_twins = {}


def batch():
    """the batch, built once and read-only"""
    global _batch
    if _batch is None:
        _batch = make_batch()
    return _batch


def twin(kp_dtype=np.float32, depth_dtype=np.float32, filter="both_inf", centres=False, extents=True, pairs=None):
    """frontend.gather_image_pairs_numpy on the batch as the device sees it (tables cast to their dtypes), computed once per variant and read-only.
    extents=False omits sizes and kp_counts; pairs: a list of pair numbers to keep (default all)."""
    from mdrp_amd import frontend
    key = (np.dtype(kp_dtype).name, np.dtype(depth_dtype).name, filter, centres, extents, None if pairs is None else tuple(pairs))
    if key not in _twins:
        t = batch()
        sel = slice(None) if pairs is None else list(pairs)
        out = frontend.gather_image_pairs_numpy(t["keypoints"].astype(kp_dtype), t["depth_maps"].astype(depth_dtype), t["pairs"][sel], t["matches"][sel],
                                                centers=t["centers"] if centres else None, sizes=t["sizes"] if extents else None,
                                                kp_counts=t["kp_counts"] if extents else None, filter=filter)
        for a in out:
            a.setflags(write=False)
        _twins[key] = out
    return _twins[key]
