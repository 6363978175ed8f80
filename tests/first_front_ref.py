"""The first chunk's pick and filter restated in plain NumPy (k_first_pick, k_first_filter: mdrp_kernels.h; the test they apply: mdrp_front.h).

Nothing here touches the GPU or the library.  tests/test_first_front_host.py checks this file against the host build of mdrp_front.h and against a
brute-force sort before tests/test_gpu_first_front.py trusts it.

A tag is  slot | key << 24 : the hypothesis in slot `slot` of the pair's slot table (four slots per iteration) with k_count's candidate density key.
  pick    sort by (-min(key, 64), slot), take the first `pick`, add the smallest slot if it is not among them
  filter  a hypothesis of the rest list at iteration t = slot // 4 with cand = (min(key, 64) * n) >> 6 is retired when
              cand <= rec_cnt  and  thr (n - cand) >= rec_score (1 + 1e-12)
          for (rec_cnt, rec_score) = (max count, min score) over the picked slots of iterations < t that hold a count >= 0; none: nothing retires"""
import numpy as np

PROBE_PTS = 64      # mdrp_kernels.h: the scale of the density key
MPS = 4             # model slots per iteration of the 3-point estimators
PICK_LIMIT = 64     # mdrp_schedule.h sched::FIRST_PICK_LIMIT
DBL_MAX = float(np.finfo(np.float64).max)
INFLATE = 1.0 + 1e-12


def slot_of(tags):
    return (np.asarray(tags, dtype=np.uint32) & np.uint32(0xFFFFFF)).astype(np.int64)


def key_of(tags):
    return np.minimum(np.asarray(tags, dtype=np.uint32) >> np.uint32(24), PROBE_PTS).astype(np.int64)


def cand_of_key(key, n):
    return (np.asarray(key, dtype=np.int64) * int(n)) >> 6


def key_of_cand(cand, n):
    """k_count: min(64, ceil(64 cand / n))"""
    return np.minimum(PROBE_PTS, -(-np.asarray(cand, dtype=np.int64) * PROBE_PTS // int(n)))


def pick(tags, pick):
    """mask over the list: True for the entries of P"""
    tags = np.asarray(tags, dtype=np.uint32)
    picked = np.zeros(len(tags), dtype=bool)
    if len(tags) == 0:
        return picked
    slot, key = slot_of(tags), key_of(tags)
    picked[np.lexsort((slot, -key))[:pick]] = True
    picked[np.argmin(slot)] = True
    return picked


def prefix_records(tags_pick, slot_inl, slot_score, iters):
    """(rec_cnt, rec_score, inflated) per entry of `iters`: the records of the picked hypotheses of strictly earlier iterations; (-1, DBL_MAX, DBL_MAX) = none"""
    ps = slot_of(tags_pick)
    it_p, cnt_p, sc_p = ps // MPS, np.asarray(slot_inl)[ps].astype(np.int64), np.asarray(slot_score, dtype=np.float64)[ps]
    iters = np.asarray(iters, dtype=np.int64)
    rc, rs = np.full(len(iters), -1, dtype=np.int64), np.full(len(iters), DBL_MAX)
    for i, t in enumerate(iters):
        before = (it_p < t) & (cnt_p >= 0)
        if before.any():
            rc[i] = cnt_p[before].max()
            rs[i] = min(DBL_MAX, float(np.fmin.reduce(np.where(sc_p[before] < DBL_MAX, sc_p[before], DBL_MAX))))
    with np.errstate(over="ignore"):
        inflated = np.where(rs < DBL_MAX, rs * INFLATE, DBL_MAX)
    return rc, rs, inflated


def prefix_records_fast(tags_pick, slot_inl, slot_score, iters):
    """prefix_records for long rest lists: the same records from one pass over P in iteration order (test_first_front_host.py pins the two together)"""
    ps = slot_of(tags_pick)
    it_p, cnt_p, sc_p = ps // MPS, np.asarray(slot_inl)[ps].astype(np.int64), np.asarray(slot_score, dtype=np.float64)[ps]
    ok = cnt_p >= 0
    it_p, cnt_p, sc_p = it_p[ok], cnt_p[ok], sc_p[ok]
    order = np.argsort(it_p, kind="stable")
    it_s = it_p[order]
    run_c = np.concatenate([[-1], np.maximum.accumulate(cnt_p[order])]) if len(order) else np.array([-1], dtype=np.int64)
    sc = np.where(sc_p[order] < DBL_MAX, sc_p[order], DBL_MAX)
    run_s = np.concatenate([[DBL_MAX], np.minimum.accumulate(sc)]) if len(order) else np.array([DBL_MAX])
    k = np.searchsorted(it_s, np.asarray(iters, dtype=np.int64), side="left")  # picked entries of strictly earlier iterations
    rc, rs = run_c[k].astype(np.int64), run_s[k]
    with np.errstate(over="ignore"):
        inflated = np.where(rs < DBL_MAX, rs * INFLATE, DBL_MAX)
    return rc, rs, inflated


def filter_retires(tags_pick, tags_rest, slot_inl, slot_score, n, thr, records=prefix_records_fast):
    """mask over the rest list: True for the hypotheses k_first_filter retires"""
    tags_rest = np.asarray(tags_rest, dtype=np.uint32)
    if len(tags_rest) == 0:
        return np.zeros(0, dtype=bool)
    rc, _, inflated = records(tags_pick, slot_inl, slot_score, slot_of(tags_rest) // MPS)
    cand = cand_of_key(key_of(tags_rest), n)
    return ~((cand > rc) | (float(thr) * (int(n) - cand).astype(np.float64) < inflated))


def front(tags, pick_n, slot_inl, slot_score, n, thr):
    """what the two kernels leave for one active pair: dict(picked, rest, kept, retired: tag arrays sorted by value; evals)"""
    tags = np.asarray(tags, dtype=np.uint32)
    p = pick(tags, pick_n)
    picked, rest = tags[p], tags[~p]
    ret = filter_retires(picked, rest, slot_inl, slot_score, n, thr)
    return dict(picked=np.sort(picked), rest=np.sort(rest), kept=np.sort(rest[~ret]), retired=np.sort(rest[ret]), evals=len(picked) * int(n))


def sequential_records(count, score):
    """the loop k_scan reproduces over a pair's slots in order: True where a slot with a count >= 0 has more inliers or a lower score than every one
    before it; slots with a negative count are skipped"""
    run_cnt, run_score, rec = 0, DBL_MAX, np.zeros(len(count), dtype=bool)
    for i in range(len(count)):
        if count[i] < 0:
            continue
        if count[i] > run_cnt or score[i] < run_score:
            rec[i] = True
            run_cnt, run_score = max(run_cnt, int(count[i])), min(run_score, float(score[i]))
    return rec
