"""The restatement of the first chunk's pick and filter (tests/first_front_ref.py) and the case table of tests/test_gpu_first_front.py
(tests/first_front_cases.py), checked without a GPU: the restated filter against the host build of mdrp_front.h on the tables of
tests/test_front_host.py, the restated pick against a brute-force stable sort, and — by the restatement alone — that the cases reach every edge they
were built for and that the filter's three outcomes each occur some hundred times."""
import numpy as np

import first_front_cases as fc
import first_front_ref as ref
import test_front_host as tfh
from test_front_host import fh  # noqa: F401  (the fixture: the host build of mdrp_front.h)


def test_restated_filter_is_the_header_predicate(fh):  # noqa: F811
    rng = np.random.default_rng(20261)
    decided = retired = 0
    for trial in range(300):
        n, thr, iters, cand, count, score = tfh._tables(rng, trial)
        m = len(iters)
        if m == 0:
            continue
        pos = np.concatenate([np.arange(c) for c in np.bincount(iters) if c])
        slots = 4 * iters.astype(np.int64) + pos
        keys = ref.key_of_cand(cand, n)
        tags = (slots | (keys << 24)).astype(np.uint32)
        slot_inl, slot_score = np.full(slots.max() + 1, -1, dtype=np.int32), np.full(slots.max() + 1, ref.DBL_MAX)
        slot_inl[slots], slot_score[slots] = count, score
        picked = ref.pick(tags, int(rng.integers(1, 9)))
        if trial % 5 == 0 and picked.sum() > 1:
            slot_inl[slots[np.flatnonzero(picked)[1]]] = -2        # a picked hypothesis the sweep's own bail-out retired: it sets no record
        tp, tr = tags[picked], tags[~picked]
        pi = np.ascontiguousarray((ref.slot_of(tp) // 4).astype(np.int32))
        pc, ps = np.ascontiguousarray(slot_inl[ref.slot_of(tp)]), np.ascontiguousarray(slot_score[ref.slot_of(tp)])
        slow = ref.filter_retires(tp, tr, slot_inl, slot_score, n, thr, records=ref.prefix_records)
        fast = ref.filter_retires(tp, tr, slot_inl, slot_score, n, thr)
        assert np.array_equal(slow, fast), trial
        for j, t in enumerate(tr):
            slot, key = int(t & 0xFFFFFF), int(t >> 24)
            assert int(fh.fh_cand_of_key(key, n)) == int(ref.cand_of_key(key, n))
            got = fh.fh_retires(pi.ctypes.data, pc.ctypes.data, ps.ctypes.data, len(pi), slot // 4, n, thr, fh.fh_cand_of_key(key, n))
            assert bool(got) == bool(fast[j]), (trial, slot)
            decided += 1
            retired += got
    assert decided > 10000 and retired > 2000 and decided - retired > 2000


def test_restated_pick_is_the_first_of_a_stable_sort():
    rng = np.random.default_rng(20262)
    for trial in range(400):
        m = int(rng.choice([0, 1, 2, 5, 64, 65, 66, 300]))
        slots = rng.choice(70000, m, replace=False)
        keys = rng.integers(0, 256 if trial % 3 == 0 else 8, m)              # few distinct keys: ties at the threshold
        tags = (slots | (keys << 24)).astype(np.uint32)
        for pick in (1, 3, 48, 64):
            got = ref.pick(tags, pick)
            by_slot = sorted(range(m), key=lambda i: int(slots[i]))                                   # brute force: Python's stable sort, twice
            order = sorted(by_slot, key=lambda i: -min(int(keys[i]), 64))
            want = set(order[:pick]) | ({by_slot[0]} if m else set())
            assert set(np.flatnonzero(got).tolist()) == want, (trial, pick)
            assert got.sum() <= pick + 1


def test_largest_retiring_score_is_the_margin():
    for s in (1.0, 0.25 * 133, 3.7e-6 * 254, 3.7e-6):
        r = fc._largest_retiring(s)
        assert r * ref.INFLATE <= s < float(np.nextafter(r, np.inf)) * ref.INFLATE and r < s


def _by_slot(tags):
    return {int(t & 0xFFFFFF): int(t) for t in tags}


def test_planted_margins_decide_as_named(fh):  # noqa: F811
    """the margin and sibling cases: X, Y, the siblings, W and Z end where the case's name says, by the restatement and by the header's predicate"""
    seen = set()
    for case in fc.margin_cases():
        r = ref.front(case.tags, 3, case.slot_inl, case.slot_score, case.n, case.thr)
        name = next(e for e in case.planted if e in fc.EDGES_ANY_PICK and e not in ("later picked hypothesis is no bar", "picked slot with -2 sets no record",
                                                                                   "no picked hypothesis earlier", "cand_of_key above the count decides"))
        seen.add(name)
        assert set(_by_slot(r["picked"])) == {1, 8, 20, 120}, case
        kept, retired = set(_by_slot(r["kept"])), set(_by_slot(r["retired"]))
        x_retired = name == "largest score that retires"
        assert (12 in retired) == x_retired and (24 in retired) == x_retired, (case, sorted(retired))  # Y behind B decides as X: B's stale 0.0 is no record
        assert {2, 3, 9, 121} <= kept and 124 in retired, (case, sorted(kept))     # siblings of E, of A and of C stay; behind the perfect C nothing does
        # the header's predicate on X, from A's record alone (E holds no inlier and a score no bound reaches)
        cand = int(ref.cand_of_key(_by_slot(case.tags)[12] >> 24, case.n))
        pi, pc, ps = np.array([0, 2], np.int32), case.slot_inl[[1, 8]].copy(), case.slot_score[[1, 8]].copy()
        assert bool(fh.fh_retires(pi.ctypes.data, pc.ctypes.data, ps.ctypes.data, 2, 3, case.n, case.thr, cand)) == x_retired, case
        # a filter that tested X's count instead of what its key stands for would retire it in every variant
        cnt = int(case.slot_inl[12])
        assert cnt < cand and fh.fh_retires(pi.ctypes.data, pc.ctypes.data, ps.ctypes.data, 2, 3, case.n, case.thr, cnt) == 1, case
        # ... and one that read B's slot as a record would retire Y wherever A's count reaches its candidates
        pi3, pc3, ps3 = np.array([0, 2, 5], np.int32), np.array([pc[0], pc[1], 0], np.int32), np.array([ps[0], ps[1], 0.0])
        assert fh.fh_retires(pi3.ctypes.data, pc3.ctypes.data, ps3.ctypes.data, 3, 6, case.n, case.thr, cand) == (1 if pc[1] >= cand else 0), case
    assert len(seen) == 6, seen
    for case in fc.sibling_cases():
        r = ref.front(case.tags, 1, case.slot_inl, case.slot_score, case.n, case.thr)
        assert set(_by_slot(r["picked"])) == {4} and set(_by_slot(r["kept"])) == {5, 6, 7} and set(_by_slot(r["retired"])) == {8, 9, 40}, case


def test_the_cases_reach_every_edge_and_every_outcome():
    groups = fc.groups()
    assert {p for p, _ in groups} == set(fc.PICKS) and {s for _, s in groups} == {fc.SMALL, fc.CHUNK_MAX, fc.THIRD_BYTE}
    outcome = dict(retired=0, kept_not_record=0, kept_record=0)
    reached_any = set()
    for pick in fc.PICKS:
        reached = set()
        for (p, table), cases in groups.items():
            if p != pick:
                continue
            assert len({c.name for c in cases}) == len(cases)
            for c in cases:
                assert c.table == table and (c.n, c.thr) in {(n, t) for n in fc.NS for t in fc.THRS}
                reached |= fc.edges_of(c, pick)
                if not c.active or not c.name.startswith("table "):
                    continue
                # the sequential loop over the pair's slots against the filter's decisions: a retired hypothesis is never a record
                r = ref.front(c.tags, pick, c.slot_inl, c.slot_score, c.n, c.thr)
                rec = ref.sequential_records(c.slot_inl, c.slot_score)
                ret, kept = ref.slot_of(r["retired"]), ref.slot_of(r["kept"])
                assert not rec[ret].any(), (c, "a record is retired")
                outcome["retired"] += len(ret)
                outcome["kept_record"] += int(rec[kept].sum())
                outcome["kept_not_record"] += int((~rec[kept]).sum())
        assert fc.EDGES_EVERY_PICK <= reached, (pick, sorted(fc.EDGES_EVERY_PICK - reached))
        reached_any |= reached
    assert fc.EDGES_ANY_PICK <= reached_any, sorted(fc.EDGES_ANY_PICK - reached_any)
    print("filter outcomes over the random tables:", outcome)
    assert min(outcome.values()) >= 300, outcome
    ns = {(c.n, c.thr) for c in fc.margin_cases()}
    assert ns == {(n, t) for n in fc.NS for t in fc.THRS}
