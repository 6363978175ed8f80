"""Inputs of tests/test_gpu_first_front.py (table form): survivor lists and slot tables for k_first_pick / k_first_filter, one case per pair.

Nothing here touches the GPU.  A case is one pair: its list of tags (in shuffled order: k_count appends through atomics), the counts and scores planted
in its slot table, n, thr, and the edges it was built for.  A GROUP is one call of mdrp_front_lists: the cases that share `pick` and the table size.
tests/test_first_front_host.py asserts over this table, by the restatement alone, that every edge the issue lists is reached and that the three
outcomes of the filter each occur some hundred times.

Largest first chunk: sched::chunk_capacity caps a super-chunk at 16384 iterations; a LEADING chunk of MDRP_CHUNKS is taken only while at least as much
again remains behind it (at most 8192), but a run of 16384 certain iterations with MDRP_CHUNKS set empty has a first chunk that is its whole
super-chunk: 16384 iterations x 4 = 65536 slots, slot numbers 0 .. 65535.  The scheduler therefore never sets the third byte of a slot; the kernels
select on all 24 bits, so one group runs on a table of 0x30000 slots all the same."""
import functools

import numpy as np

import first_front_ref as ref

NS = (3, 40, 257, 600)
THRS = (1.0, 0.25, 3.7e-6)
PICKS = (1, 3, 48, 64)
SMALL, CHUNK_MAX, THIRD_BYTE = 1024, 65536, 0x30000  # slots per pair of the three table sizes
COUNTS_SMALL, COUNTS_LARGE = (0, 1, 65, 66, 257), (4096, CHUNK_MAX)
TINY = float(np.finfo(np.float64).tiny)
# every edge a group's cases must reach between them (edges_of computes them from the restatement)
EDGES_EVERY_PICK = frozenset({
    "count 0", "count 1", "count pick - 1", "count pick", "count pick + 1", "count 65", "count 66", "count 257", "count 4096", "count 65536",
    "earliest among the densest", "earliest not among the densest", "earliest alone in its iteration", "one key", "tied slots differ in the low byte only",
    "tied slots differ in the second byte only", "exactly s_need at the threshold key", "one more than s_need at the threshold key", "threshold key 0",
    "slots missing", "empty iterations", "key above 64", "slot above 255", "empty rest list", "rest list retired in full", "inactive"})
EDGES_ANY_PICK = frozenset({
    "tied slots differ in the third byte", "exact tie stays", "one ulp above the tie", "one ulp below the tie", "largest score that retires",
    "smallest score that keeps", "cand = rec_cnt + 1", "sibling of the only picked hypothesis", "later picked hypothesis is no bar",
    "picked slot with -2 sets no record", "no picked hypothesis earlier", "cand_of_key above the count decides", "P of 65 entries"})


class Case:
    def __init__(self, name, n, thr, slots, keys, counts, scores, active=1, edges=(), table=SMALL, rng=None):
        slots, keys = np.asarray(slots, dtype=np.int64), np.asarray(keys, dtype=np.int64)
        assert len(set(slots.tolist())) == len(slots) and (len(slots) == 0 or (0 <= slots.min() and slots.max() < table)) and (keys >= 0).all() and (keys < 256).all()
        self.name, self.n, self.thr, self.active, self.planted, self.table = name, int(n), float(thr), active, frozenset(edges), table
        order = (rng or np.random.default_rng(len(slots))).permutation(len(slots))
        self.tags = (slots | (keys << 24)).astype(np.uint32)[order]
        self.slot_inl = np.full(table, -1, dtype=np.int32)       # empty slots, as k_solve leaves an iteration with fewer than four models
        self.slot_score = np.full(table, ref.DBL_MAX)
        self.slot_inl[slots] = counts
        self.slot_score[slots] = scores

    def __repr__(self):
        return f"Case({self.name}, n={self.n}, thr={self.thr}, {len(self.tags)} tags)"


def _consistent(rng, n, thr, keys):
    """counts at or below what the key stands for, scores at or above thr (n - count): what an exact sweep would find"""
    cand = ref.cand_of_key(np.minimum(keys, 64), n)
    count = np.maximum(cand - rng.integers(0, max(n // 16, 1) + 1, len(keys)), 0)
    score = thr * (n - count) + np.where(rng.random(len(keys)) < 0.2, 0.0, rng.random(len(keys)) * thr * count)
    return count.astype(np.int32), score


def _listed(rng, name, n, thr, slots, keys, **kw):
    count, score = _consistent(rng, n, thr, np.asarray(keys))
    return Case(name, n, thr, slots, keys, count, score, rng=rng, **kw)


def _random_keys(rng, m, above=False):
    keys = np.where(rng.random(m) < 0.1, rng.integers(40, 65, m), rng.integers(0, 12, m))
    if above:
        keys = np.where(rng.random(m) < 0.05, rng.integers(65, 256, m), keys)  # k_count never writes one: the kernels clamp
    return keys


def _count_cases(rng, pick, counts, table):
    out = []
    for c in counts:
        n, thr = int(rng.choice(NS)), float(rng.choice(THRS))
        slots = np.sort(rng.choice(table, c, replace=False)) if c < table else np.arange(table)
        out.append(_listed(rng, f"count {c}", n, thr, slots, _random_keys(rng, c, above=True), table=table))
    return out


def _selection_cases(rng, pick, table):
    """ties at the threshold key and the earliest hypothesis; `table` >= 65536 adds the second-byte ties"""
    out = []
    n, thr = 257, 0.25
    a = pick // 2  # entries above the threshold key

    def tied(name, tie_slots, n_tied, extra_low=20, key_t=30, low_key=3):
        tie_slots = np.asarray(tie_slots)[:n_tied]
        free = np.setdiff1d(np.arange(min(table, 4096)), tie_slots)
        others = rng.choice(free, a + extra_low, replace=False)
        slots = np.concatenate([others[:a], tie_slots, others[a:]])
        keys = np.concatenate([np.full(a, 64), np.full(len(tie_slots), key_t), np.full(extra_low, low_key)])
        return _listed(rng, name, n, thr, slots, keys, table=table)

    low = 0x200 + rng.permutation(256)
    out.append(tied("ties in the low byte", low, 2 * pick + 3))
    out.append(tied("exactly s_need tied", low, pick - a))
    out.append(tied("one more than s_need tied", low, pick - a + 1))
    if table >= 65536:
        out.append(tied("ties in the second byte", (rng.permutation(256) << 8) | 0x33, 2 * pick + 3))
    out.append(_listed(rng, "one key", n, thr, np.sort(rng.choice(min(table, 4096), 300, replace=False)), np.full(300, 17), table=table))
    # the key walk reaches 0: fewer than `pick` entries above it
    m = pick + 40
    out.append(_listed(rng, "key walk to 0", n, thr, np.sort(rng.choice(min(table, 4096), a + m, replace=False)), np.concatenate([np.full(a, 64), np.zeros(m, dtype=np.int64)]), table=table))
    # the earliest hypothesis: among the densest | not (P has pick + 1 entries) | alone in its iteration
    body = 8 + np.sort(rng.choice(min(table, 4096) - 8, pick + 30, replace=False))
    keys = rng.integers(1, 64, len(body))
    out.append(_listed(rng, "earliest among the densest", n, thr, np.concatenate([[5], body]), np.concatenate([[64], keys]), table=table))
    out.append(_listed(rng, "earliest not among the densest", n, thr, np.concatenate([[5, 6], body]), np.concatenate([[0, 0], keys]), table=table))
    out.append(_listed(rng, "earliest alone in its iteration", n, thr, np.concatenate([[2], body]), np.concatenate([[0], keys]), table=table))
    return out


def _rest_cases(rng, pick, table):
    """an empty rest list (count = pick + 1 with the earliest hypothesis not among the densest) and one that is retired in full: `pick` perfect models in
    the first iterations, everything behind them below the full density"""
    n, thr = 600, 1.0
    out = [_listed(rng, "empty rest list", n, thr, np.arange(3, 3 + pick + 1), np.concatenate([[0], np.full(pick, 9)]), table=table)]
    behind = 4 * ((pick + 3) // 4) + np.sort(rng.choice(table - 4 * ((pick + 3) // 4), 150, replace=False))
    slots, keys = np.concatenate([np.arange(pick), behind]), np.concatenate([np.full(pick, 64), rng.integers(0, 64, 150)])
    count, score = _consistent(rng, n, thr, keys)
    count[:pick], score[:pick] = n, 0.0
    out.append(Case("rest list retired in full", n, thr, slots, keys, count, score, table=table, rng=rng))
    return out


def _random_table_cases(rng, count, first_trial):
    """the tables of tests/test_front_host.py (same-iteration models, empty iterations, planted ties) as lists: slot = 4 iteration + position, the key
    k_count would give the candidate count"""
    import test_front_host as tfh
    out = []
    for trial in range(first_trial, first_trial + count):
        n, thr, iters, cand, cnt, score = tfh._tables(rng, trial)
        if len(iters) == 0:
            continue
        pos = np.concatenate([np.arange(c) for c in np.bincount(iters) if c])
        out.append(Case(f"table {trial}", n, thr, 4 * iters.astype(np.int64) + pos, ref.key_of_cand(cand, n), cnt, score, rng=rng))
    return out


def _largest_retiring(s):
    """the largest double r with r (1 + 1e-12) <= s, for s > 0: the record score at which a bound of exactly s is still retired"""
    r = s / ref.INFLATE
    while r * ref.INFLATE > s:
        r = float(np.nextafter(r, 0.0))
    while float(np.nextafter(r, np.inf)) * ref.INFLATE <= s:
        r = float(np.nextafter(r, np.inf))
    return r


def margin_cases():
    """pick = 3.  P = A (iteration 2), B (iteration 5, count -2 and a stale score of 0), C (iteration 30, perfect), all at key 64, and the earliest
    hypothesis E (slot 1, no inlier).  X (iteration 3) sits on A's bar: cand_of_key(X) = cA and thr (n - cand) = sA, in six variants of (cA, sA)."""
    out = []
    for n in NS:
        for thr in THRS:
            kx = {3: 43, 40: 33, 257: 31, 600: 37}[n]
            cx = int(ref.cand_of_key(kx, n))
            s = thr * float(n - cx)
            r = _largest_retiring(s)
            variants = [("exact tie stays", cx, s), ("one ulp above the tie", cx, float(np.nextafter(s, np.inf))), ("one ulp below the tie", cx, float(np.nextafter(s, 0.0))),
                        ("largest score that retires", cx, r), ("smallest score that keeps", cx, float(np.nextafter(r, np.inf))), ("cand = rec_cnt + 1", cx - 1, TINY)]
            for name, ca, sa in variants:
                #        E   sib sib  A   S(A) X    X'   B    Y    W(C) C    Z
                slots = [1,  2,  3,   8,  9,   12,  13,  20,  24,  121, 120, 124]
                keys = [0,   kx, 5,   64, kx,  kx,  kx,  64,  kx,  64,  64,  63]  # (W ties with A, B, C at key 64 and loses by its slot)
                # true counts: X holds fewer inliers than its key stands for — a filter that tested the count would retire it in every variant
                cnts = [0,   0,  0,   ca, 0,   max(cx - 2, 0), 0, -2, 0, 0,  n,   0]
                scs = [thr * n] + [thr * n] * 2 + [sa, thr * n, thr * (n - max(cx - 2, 0)), thr * n, 0.0, thr * n, thr * n, 0.0, thr * n]
                edges = {name, "later picked hypothesis is no bar", "picked slot with -2 sets no record", "no picked hypothesis earlier", "cand_of_key above the count decides"}
                out.append(Case(f"margin n={n} thr={thr} {name}", n, thr, slots, keys, cnts, scs, edges=edges, rng=np.random.default_rng(n)))
    return out


def sibling_cases():
    """pick = 1.  The only picked hypothesis A (earliest and densest, perfect) and its three siblings, which stay; everything behind it is retired."""
    out = []
    for n in NS:
        for thr in THRS:
            slots, keys = [4, 5, 6, 7, 8, 9, 40], [64, 10, 63, 0, 10, 63, 0]
            out.append(Case(f"siblings n={n} thr={thr}", n, thr, slots, keys, [n, 0, 0, 0, 0, 0, 0], [0.0] + [thr * n] * 6,
                            edges={"sibling of the only picked hypothesis"}, rng=np.random.default_rng(n)))
    return out


def _inactive(rng, table):
    c = _listed(rng, "inactive", 257, 1.0, np.sort(rng.choice(table, 200, replace=False)), _random_keys(rng, 200), active=0, table=table)
    return c


@functools.lru_cache(maxsize=None)
def groups():
    """{(pick, slots per pair): [Case]} — one call of mdrp_front_lists each"""
    out = {}
    for pick in PICKS:
        rng = np.random.default_rng(5100 + pick)
        small = _count_cases(rng, pick, sorted(set(COUNTS_SMALL) | {pick - 1, pick, pick + 1}), SMALL)
        small += _selection_cases(rng, pick, SMALL) + _rest_cases(rng, pick, SMALL) + _random_table_cases(rng, 60, 100 * pick) + [_inactive(rng, SMALL)]
        if pick == 3:
            small += margin_cases()
        if pick == 1:
            small += sibling_cases()
        out[(pick, SMALL)] = small
        out[(pick, CHUNK_MAX)] = _count_cases(rng, pick, COUNTS_LARGE, CHUNK_MAX) + _selection_cases(rng, pick, CHUNK_MAX) + [_inactive(rng, CHUNK_MAX)]
    rng = np.random.default_rng(5200)
    third = (np.arange(3) << 16) | 0x1234
    tie = _listed(rng, "ties in the third byte", 257, 0.25, np.concatenate([[0x77], third, [0x20000, 0x2FFFF]]), [64, 30, 30, 30, 3, 3], table=THIRD_BYTE)
    wide = _listed(rng, "slots across three bytes", 600, 1.0, np.sort(rng.choice(THIRD_BYTE, 5000, replace=False)), _random_keys(rng, 5000), table=THIRD_BYTE)
    out[(3, THIRD_BYTE)] = [tie, wide]
    return out


def pick_analysis(tags, pick):
    """the threshold key, s_need and the tied slots of k_first_pick's select, restated by the histogram walk (for the edges only)"""
    slot, key = ref.slot_of(tags), ref.key_of(tags)
    if len(tags) <= pick:
        return None
    hist = np.bincount(key, minlength=65)
    k, above = 64, 0
    while k > 0 and above + hist[k] < pick:
        above += hist[k]
        k -= 1
    return dict(key=k, need=pick - above, tied=np.sort(slot[key == k]))


def edges_of(case, pick):
    """the edges a case reaches, from the restatement: its planted ones (each verified in test_first_front_host.py) and the structural ones"""
    e = set(case.planted)
    if not case.active:
        return {"inactive"}
    tags = case.tags
    c = len(tags)
    for name, v in (("count pick - 1", pick - 1), ("count pick", pick), ("count pick + 1", pick + 1)):
        if c == v:
            e.add(name)
    if c in (0, 1, 65, 66, 257, 4096, 65536):
        e.add(f"count {c}")
    if c == 0:
        return e
    slot, raw_key = ref.slot_of(tags), np.asarray(tags, dtype=np.uint32) >> np.uint32(24)
    r = ref.front(tags, pick, case.slot_inl, case.slot_score, case.n, case.thr)
    first = slot.min()
    if c > pick:
        e.add("earliest not among the densest" if len(r["picked"]) == pick + 1 else "earliest among the densest")
        if len(r["picked"]) == 65:
            e.add("P of 65 entries")
    if (slot // 4 == first // 4).sum() == 1 and c > 1:
        e.add("earliest alone in its iteration")
    if (raw_key > 64).any():
        e.add("key above 64")
    if (slot > 255).any():
        e.add("slot above 255")
    its = np.unique(slot // 4)
    if len(its) < its.max() - its.min() + 1:
        e.add("empty iterations")
    if c < 4 * len(its):
        e.add("slots missing")
    a = pick_analysis(tags, pick)
    if a:
        t = a["tied"]
        if len(np.unique(ref.key_of(tags))) == 1:
            e.add("one key")
        if a["key"] == 0:
            e.add("threshold key 0")
        if len(t) == a["need"]:
            e.add("exactly s_need at the threshold key")
        if len(t) == a["need"] + 1:
            e.add("one more than s_need at the threshold key")
        if len(t) > a["need"]:  # the slot select decides: which bytes tell the tied slots apart
            differ = [len(np.unique((t >> s) & 255)) > 1 for s in (0, 8, 16)]
            if differ == [True, False, False]:
                e.add("tied slots differ in the low byte only")
            if differ == [False, True, False]:
                e.add("tied slots differ in the second byte only")
            if differ[2]:
                e.add("tied slots differ in the third byte")
    if len(r["rest"]) == 0 and c > 1:
        e.add("empty rest list")
    if len(r["rest"]) > 0 and len(r["kept"]) == 0:
        e.add("rest list retired in full")
    return e
