"""Inputs of tests/test_frontend_ranked_host.py and tests/test_gpu_frontend_ranked.py: batches of the device front end (the pairs of
tests/test_gpu_frontend.py, stacked) with one score per MATCH ROW planted across the pairs.  A helper, not a test.

The score patterns, one per pair of a batch (`PATTERNS`, rotated over the pairs by `offset`):
  random        uniform scores, no two alike
  levels        scores quantised to four levels: long runs of ties, which go by ascending match row
  special       NaN (both signs, three payloads), +inf, -inf, -0.0 and +0.0 sprinkled over uniform scores, on kept and on dropped rows
  dropped_high  the HIGHEST scores of the pair (and a NaN, a +inf) on the rows the front end drops — -1 padding, an index past the table, a
                keypoint outside its map, both depths infinite; the padding rows sit between kept ones.  A score that took part in the
                ranking of a dropped row, or in whether a row is kept, moves every rank.
  ascending / descending / constant
Scores are made in float64 and rounded through float32 once, so that the float32 and the float64 tensor of one case hold the same values."""
import numpy as np

import test_gpu_frontend as fe

PATTERNS = ("random", "levels", "special", "dropped_high", "ascending", "descending", "constant")
NANS = (0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000000000001, 0xfff4000000000000, 0x7ff0000020000000)  # quiet / signalling, both signs, payloads


def _nan(bits):
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


def make_batch(specs, first_seed, pad=7):
    """fe.make_batch_inputs with a chosen number of -1 rows behind the longest pair (pad = 0: M is the largest row count itself)"""
    pairs = [fe.make_pair_inputs(first_seed + k, rows, special) for k, (rows, special) in enumerate(specs)]
    M = max(len(q[2]) for q in pairs) + pad
    K1, K2 = max(len(q[0]) for q in pairs), max(len(q[1]) for q in pairs)
    B = len(pairs)
    kp1 = np.full((B, K1, 2), 5.0); kp2 = np.full((B, K2, 2), 5.0)
    matches = np.full((B, M, 2), -1, dtype=np.int64)
    for b, q in enumerate(pairs):
        kp1[b, :len(q[0])] = q[0]; kp2[b, :len(q[1])] = q[1]; matches[b, :len(q[2])] = q[2]
    return {"kp1": kp1, "kp2": kp2, "matches": matches, "dm1": np.stack([q[3] for q in pairs]), "dm2": np.stack([q[4] for q in pairs]),
            "c1": np.tile(np.array(fe.C1), (B, 1)) + np.arange(B)[:, None] * 0.125, "c2": np.tile(np.array(fe.C2), (B, 1)), "specs": specs}


def keep_only(batch, b, count):
    """leave pair b of a batch exactly `count` of its kept rows (the others become padding)"""
    from mdrp_amd import frontend
    slot = frontend.gather_matches_numpy(batch["kp1"][b].astype(np.float32), batch["kp2"][b].astype(np.float32), batch["matches"][b],
                                         batch["dm1"][b].astype(np.float32), batch["dm2"][b].astype(np.float32), filter="finite")[4]
    kept = np.flatnonzero(slot >= 0)
    assert len(kept) >= count
    batch["matches"][b, kept[count:]] = -1


def pair_scores(pattern, kept, seed):
    """(M,) float64 scores of one pair; kept: (M,) bool, the rows the front end keeps (with the most permissive filter)"""
    rng = np.random.default_rng(seed)
    M = len(kept)
    if pattern == "random":
        s = rng.permutation(M) / max(M, 1) + rng.uniform(0.0, 0.4 / max(M, 1), M)
    elif pattern == "levels":
        s = rng.integers(0, 4, M) / 4.0
    elif pattern == "special":
        s = rng.uniform(-1.0, 1.0, M)
        values = [_nan(b) for b in NANS] + [np.inf, -np.inf, -0.0, 0.0, -0.0, 0.0, np.inf, -np.inf]
        for rows in (np.flatnonzero(kept), np.flatnonzero(~kept)):  # on kept rows first, then on dropped ones
            at = rng.permutation(rows)[:len(values)]
            s[at] = values[:len(at)]
    elif pattern == "dropped_high":
        s = rng.uniform(0.0, 1.0, M)
        gone = np.flatnonzero(~kept)
        s[gone] = 10.0 + rng.uniform(0.0, 1.0, len(gone))
        s[gone[::5]] = np.inf
        s[gone[1::5]] = _nan(NANS[1])
    elif pattern == "ascending":
        s = np.arange(M, dtype=np.float64)
    elif pattern == "descending":
        s = -np.arange(M, dtype=np.float64)
    elif pattern == "constant":
        s = np.full(M, 0.5)
    else:
        raise ValueError(pattern)
    with np.errstate(invalid="ignore"):  # (a signalling NaN is quieted by the conversion: it stays a NaN of its sign)
        return s.astype(np.float32).astype(np.float64)


def batch_scores(kept, offset=0, seed=0):
    """(B, M) float64 scores: pair b gets PATTERNS[(b + offset) % 7]; kept: (B, M) bool"""
    return np.stack([pair_scores(PATTERNS[(b + offset) % len(PATTERNS)], kept[b], 1000 * seed + 17 * b + offset) for b in range(len(kept))])


def kept_rows(batch):
    """(B, M) bool: the rows the definition keeps under "both_inf" with float32 or with float64 tables — every other row is dropped in every
    variant of a test"""
    from mdrp_amd import frontend
    B = len(batch["matches"])
    return np.stack([np.logical_or.reduce([frontend.gather_matches_numpy(batch["kp1"][b].astype(t), batch["kp2"][b].astype(t), batch["matches"][b],
                                                                         batch["dm1"][b].astype(t), batch["dm2"][b].astype(t))[4] >= 0
                                           for t in (np.float32, np.float64)]) for b in range(B)])


def ranked_twin(batch, scores, kp_dtype, depth_dtype, filter, centres):
    """the NumPy definition with scores on the batch as the device sees it: the padded buffers of frontend.pad_pairs"""
    from mdrp_amd import frontend
    kp1, kp2 = batch["kp1"].astype(kp_dtype), batch["kp2"].astype(kp_dtype)
    dm1, dm2 = batch["dm1"].astype(depth_dtype), batch["dm2"].astype(depth_dtype)
    B, M = batch["matches"].shape[:2]
    g = [frontend.gather_matches_numpy(kp1[b], kp2[b], batch["matches"][b], dm1[b], dm2[b], batch["c1"][b] if centres else None,
                                       batch["c2"][b] if centres else None, filter, None if scores is None else scores[b]) for b in range(B)]
    return frontend.pad_pairs(g, M)


_batches = None


def batches():
    """two batches of six pairs, built once: row counts on the wavefront and tile boundaries of the gather, pairs that keep 0, 1, 2 and 3 rows"""
    global _batches
    if _batches is None:
        a = make_batch([(1, None), (2, None), (3, None), (63, None), (64, None), (600, None)], 0)
        b = make_batch([(255, None), (256, None), (257, None), (64, "none_kept"), (70, 2), (100, 3)], 20)
        c = make_batch([(65, None), (70, 2)], 40)
        keep_only(c, 1, 1)
        _batches = (a, b, c)
    return _batches
