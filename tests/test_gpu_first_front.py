"""The first chunk's prefix retirement, decision by decision (mdrp_front_lists, mdrp_front_models).

tests/test_gpu_first_filter.py runs whole estimates with the stage on and off: any picked set is valid there, and a wrong retirement shows only when a
true record breaker happens to sit on the margin of a bar.  Here k_first_pick and k_first_filter run

  1. on planted lists and slot tables (tests/first_front_cases.py), one case per pair, one call per (pick, table size): picked set, rest set, kept set
     (compared as sorted arrays: the kernels fill them through LDS atomics), their three counts, the evals increment and what an inactive pair keeps
     are EXACTLY those of the NumPy restatement tests/first_front_ref.py, which tests/test_first_front_host.py pins to mdrp_front.h and to a
     brute-force sort.  First chunks reach 16384 iterations x 4 = 65536 slots (sched::chunk_capacity; a run of 16384 certain iterations with
     MDRP_CHUNKS set empty: the first chunk is its whole super-chunk), so slot numbers stay below 2^16 in the scheduler; one group runs on a table of
     0x30000 slots, where the select's first round decides.
  2. on one pair with real models (tests/retirement_cases.py), behind k_count — unarmed, or armed the way a prior arms it — and in front of k_score,
     through the function the estimator launches the stage with: every slot's `left_at` is what mdrp_count_candidates -> key, the restated pick,
     mdrp_score_models on P and the restated filter predict; slots hold the unarmed sweep's bits or -2; no retired slot is a record of the oracle's
     sequential loop (score margin 1e-9, ten times the suite's 1e-10), and the loop over the returned slots ends in the records of the loop over all.
     Among copies of one model the earliest slot is the picked one (equal keys, ties by slot), so a copy cannot lie BEFORE the picked copy on the rest
     list; copies in the picked copy's iteration and in the next one are planted, and the prediction says where each ends.
Needs an MI355X:  pytest -m gpu."""
import ctypes as C

import numpy as np
import pytest

import first_front_cases as fc
import first_front_ref as ref
import retirement_cases as rc

pytestmark = pytest.mark.gpu

TAG_FILL, COUNT_FILL = 0xDEADBEEF, -7
KINDS = ("CALIB", "SHARED_FOCAL", "VARYING_FOCAL")
MODEL_PAIRS = (1, 3)  # of retirement_cases.PAIRS: 40 % outliers at 1 px of noise | no outlier at 0.5 px
TINY = float(np.finfo(np.float64).tiny)


@pytest.fixture(scope="module")
def handle():
    from mdrp_amd import _capi
    return _capi.default_handle(0)


@pytest.fixture(scope="module")
def capi():
    from mdrp_amd import _capi
    return _capi


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


# ------------------------------------------------------------------------------------------------------------------------ 1. table form
@pytest.mark.parametrize("pick,table", sorted(fc.groups()))
def test_pick_and_filter_on_planted_lists(handle, pick, table):
    cases = fc.groups()[(pick, table)]
    got = handle.front_lists([c.n for c in cases], [c.thr for c in cases], [c.active for c in cases], [c.tags for c in cases], pick,
                             np.stack([c.slot_score for c in cases]), np.stack([c.slot_inl for c in cases]),
                             fill=dict(tags_pick=TAG_FILL, tags_rest=TAG_FILL, tags_out=TAG_FILL, pick_count=COUNT_FILL, rest_count=COUNT_FILL, surv_count=COUNT_FILL))
    assert (got["rest_count"][1::2] == COUNT_FILL).all(), "rest_count has stride 2: the odd entries belong to another stage"
    evals, bad = 0, []
    for p, c in enumerate(cases):
        counts = (int(got["pick_count"][p]), int(got["rest_count"][2 * p]), int(got["surv_count"][p]))
        if not c.active:
            same = counts == (COUNT_FILL,) * 3 and all((got[k][p] == TAG_FILL).all() for k in ("tags_pick", "tags_rest", "tags_out"))
            if not same:
                bad.append((c.name, "an inactive pair's outputs changed", counts))
            continue
        want = ref.front(c.tags, pick, c.slot_inl, c.slot_score, c.n, c.thr)
        evals += want["evals"]
        if counts != (len(want["picked"]), len(want["rest"]), len(want["kept"])):
            bad.append((c.name, "counts (picked, rest, kept)", counts, (len(want["picked"]), len(want["rest"]), len(want["kept"]))))
            continue
        for k in ("picked", "rest", "kept"):
            if not np.array_equal(np.sort(got[k][p]), want[k]):
                d = np.setxor1d(got[k][p], want[k])
                bad.append((c.name, k, len(d), [hex(int(t)) for t in d[:6]]))
        for k, m in (("tags_pick", counts[0]), ("tags_rest", counts[1]), ("tags_out", counts[2])):
            if not (got[k][p, m:] == TAG_FILL).all():
                bad.append((c.name, k, "written past its count"))
        assert len(want["picked"]) <= pick + 1
    assert not bad, (pick, table, len(bad), bad[:12])
    assert got["evals"] == evals, (got["evals"], evals)


def test_front_lists_refuses_what_it_cannot_run(handle, capi):
    c = fc.sibling_cases()[0]
    args = ([c.n], [c.thr], [1], [c.tags])
    tables = (c.slot_score[None, :64].copy(), c.slot_inl[None, :64].copy())
    handle.front_lists(*args, 1, *tables)                                                          # the good call
    for pick in (0, -1, capi.FRONT_PICK_LIMIT + 1):
        with pytest.raises(capi.MdrpError, match="pick"):
            handle.front_lists(*args, pick, *tables)
    with pytest.raises(capi.MdrpError, match="outside the table"):
        handle.front_lists([c.n], [c.thr], [1], [np.array([64 | (5 << 24)], dtype=np.uint32)], 1, *tables)
    with pytest.raises(capi.MdrpError, match="slots"):
        handle.front_lists(*args, 1, c.slot_score[None, :62].copy(), c.slot_inl[None, :62].copy())
    # a NULL buffer: every pointer of the descriptor in turn
    one = np.zeros(64, dtype=np.uint64)
    names = [f for f, t in capi.FrontTables._fields_ if t is C.c_void_p]
    assert len(names) == 14
    for missing in names:
        io = capi.FrontTables(1, 64, 1, 0, *[None if f == missing else C.c_void_p(one.ctypes.data) for f in names])
        assert handle._lib.mdrp_front_lists(handle._h, C.byref(io)) == 1 and b"NULL" in handle._lib.mdrp_last_error(), missing
    with pytest.raises(capi.MdrpError, match="pick"):
        handle.front_models(0, np.zeros(4, dtype=capi.MODEL_DTYPE), np.zeros((8, 2)), np.zeros((8, 2)), rc.THR, 65)
    with pytest.raises(capi.MdrpError, match="3-point"):
        handle.front_models(5, np.zeros(4, dtype=capi.MODEL_DTYPE), np.zeros((8, 2)), np.zeros((8, 2)), rc.THR, 3)


# ------------------------------------------------------------------------------------------------------------------------ 2. model form
_UNARMED = {}


def _unarmed(handle, capi, kind_name, n, pi, layout):
    """the models of a layout and the unarmed stages' numbers on them (computed once and shared): candidates -> keys, exact (score, count), the oracle.
    Layouts:  plain       the pair's 1100 models, the bar model's copies in retirement_cases.DUP_SLOTS
              copies      copies of the median near-true model in slots 0 (the earliest hypothesis: picked), 1 (its sibling), 4 and 5 (the next iteration)
              nan first   the NaN model in slot 0 as well: the earliest hypothesis is slot 1
              garbage first  slot 0 holds the garbage model of slot 2: behind an armed count the earliest SURVIVOR is a later slot"""
    key = (kind_name, n, pi, layout)
    if key in _UNARMED:
        return _UNARMED[key]
    kind = getattr(capi, kind_name)
    x1, x2, ms = rc.pair_case(n, pi)
    so, co = rc.oracle_scores(n, pi, kind == capi.CALIB)
    s0, c0 = handle.score_models(kind, capi.array_to_models(ms), x1, x2, rc.THR)
    order = sorted(rc.NEAR_TRUE, key=lambda k: (int(c0[k]), -float(s0[k])))
    best, median = order[-1], order[len(order) // 2]
    ms, so, co = rc.with_duplicates(ms, best), rc.with_duplicates(so, best), rc.with_duplicates(co, best)  # the best model's copies in DUP_SLOTS
    src = np.arange(rc.NUM_MODELS)                      # slot -> the row it holds
    if layout == "copies":
        src[[0, 1, 4, 5]] = median
    elif layout == "nan first":
        src[0] = rc.NAN_SLOT
    elif layout == "garbage first":
        src[0] = 2
    else:
        assert layout == "plain"
    models = capi.array_to_models(ms[src])
    cand = handle.count_candidates(kind, models, x1, x2, rc.THR).astype(np.int64)
    su, cu = handle.score_models(kind, models, x1, x2, rc.THR)
    nan = np.isin(src, [rc.NAN_SLOT])
    d = dict(kind=kind, x1=x1, x2=x2, models=models, cand=cand, keys=ref.key_of_cand(cand, n), su=su, cu=cu.astype(np.int64), so=so[src], co=co[src], nan=nan,
             inf=np.flatnonzero(src == rc.INF_SLOT), n=n)
    _UNARMED[key] = d
    return d


def _loop(count, score, start=(0, ref.DBL_MAX)):
    """the sequential loop's final records over the slots with a count >= 0"""
    run_cnt, run_score = start
    for c, s in zip(count, score):
        if c >= 0 and (c > run_cnt or s < run_score):
            run_cnt, run_score = max(run_cnt, int(c)), min(run_score, float(s))
    return run_cnt, run_score


def _check_front(d, pick, bar, res, where):
    """one run of mdrp_front_models against the prediction; returns the left_at it predicted"""
    n, cand, keys, su, cu, so, co = d["n"], d["cand"], d["keys"], d["su"], d["cu"], d["so"], d["co"]
    sc, cn, la, info = res
    M = len(la)
    rec_cnt, rec_score = bar if bar else (0, None)
    armed = rec_score is not None
    inflated = rec_score * ref.INFLATE if armed else ref.DBL_MAX
    listed = ~d["nan"]
    # ---- the count: what a prior's records leave
    surv = listed & ((cand > rec_cnt) | (rc.THR * (n - cand).astype(np.float64) < inflated)) if armed else listed
    want = np.where(listed, 1, 0)
    slots = np.flatnonzero(surv)
    tags = (slots | (keys[slots] << 24)).astype(np.uint32)
    # ---- the pick, on the keys of mdrp_count_candidates
    p = ref.pick(tags, pick)
    want[slots[p]] = 4
    picked = slots[p]
    assert np.array_equal(np.flatnonzero(la == 4), picked), (where, "P", np.flatnonzero(la == 4)[:10], picked[:10])
    # ---- the picked slots: the unarmed sweep's bits; behind an armed count the sweep may bail out of a model that breaks no record
    out = cn[picked] == -2
    assert np.array_equal(cn[picked][~out], cu[picked][~out]) and _same_bits(sc[picked][~out], su[picked][~out]), (where, "slots of P")
    assert armed or not out.any(), (where, "a picked model without a count and without a record to bail out against")
    if armed:
        assert (cu[picked][out] <= rec_cnt).all() and (su[picked][out] >= rec_score).all(), (where, "a picked model was bailed out without proof")
    # ---- the filter, on those slots
    ret = ref.filter_retires(tags[p], tags[~p], cn, sc, n, rc.THR)
    want[slots[~p][ret]] = 5
    want[slots[~p][~ret]] = 3
    assert np.array_equal(la, want), (where, "left_at", [(int(i), int(la[i]), int(want[i])) for i in np.flatnonzero(la != want)[:10]])
    assert tuple(info) == (len(slots), int(p.sum()), int((~p).sum()), int((~ret).sum()), int(p.sum())), (where, info)
    # ---- slot contents
    assert (cn[d["nan"]] == -3).all() and (la[d["nan"]] == 0).all(), (where, "the NaN model")
    gone = (la == 1) | (la == 5)
    assert (cn[gone] == -2).all() and (sc[gone] == ref.DBL_MAX).all(), (where, "a retired slot holds something")
    swept = (la == 3) | (la == 4)
    done = swept & (cn != -2)
    assert np.array_equal(cn[done], cu[done]) and _same_bits(sc[done], su[done]), (where, "slots of the two sweeps")
    if armed:
        bailed = swept & (cn == -2)
        assert (cu[bailed] <= rec_cnt).all() and (su[bailed] >= rec_score).all(), (where, "bailed out without proof")
    else:
        assert (cn[swept] >= 0).all(), where
    # ---- soundness by the oracle: no slot without a count is a record of the loop over ALL exact scores, and the loop over the returned slots
    # ends where the loop over all of them ends
    # (the inf and the zero-quaternion model have no oracle score: the unarmed sweep's stands in for it)
    so, co = np.where(np.isfinite(so), so, su), np.where(np.isfinite(so), co, cu)
    start = (rec_cnt, rec_score) if armed else (0, ref.DBL_MAX)
    run_cnt, run_score = start
    for i in np.flatnonzero(listed):
        if cn[i] == -2:
            assert not (co[i] > run_cnt or so[i] < run_score * (1.0 - 1e-9)), (where, "a record of the oracle's loop was retired", i, int(la[i]))
        if co[i] > run_cnt or so[i] < run_score:
            run_cnt, run_score = max(run_cnt, int(co[i])), min(run_score, float(so[i]))
    end_got = _loop(cn, sc, start)
    assert end_got == _loop(np.where(listed, cu, -1), su, start), (where, "records of the loop over the returned slots", end_got)
    assert end_got[0] == run_cnt and abs(end_got[1] - run_score) <= 1e-10 * abs(run_score), (where, "against the oracle's loop", end_got, (run_cnt, run_score))
    return want


@pytest.mark.parametrize("n", rc.FRONT_NS)
@pytest.mark.parametrize("kind_name", KINDS)
def test_front_behind_an_unarmed_count_is_predicted_exactly(handle, capi, kind_name, n):
    reached = set()
    for pi in MODEL_PAIRS:
        for layout in ("plain", "copies", "nan first"):
            d = _unarmed(handle, capi, kind_name, n, pi, layout)
            for pick in (1, 3, 48, 64):
                res = handle.front_models(d["kind"], d["models"], d["x1"], d["x2"], rc.THR, pick)
                where = (kind_name, n, pi, layout, pick)
                la = _check_front(d, pick, None, res, where)
                reached |= {int(v) for v in la}
                assert (la[d["inf"]] >= 3).all(), (where, "the inf model was retired without a sweep's proof")
                if layout == "copies":
                    # the copy in slot 0 is the earliest hypothesis: picked; its sibling stays whatever the records; 4 and 5 end where the prediction says
                    assert la[0] == 4 and la[1] in (3, 4), (where, la[:8])
                    if la[1] == 3 and la[4] == 5:
                        reached.add("copy retired behind the picked copy")
                    if la[4] == 3:
                        reached.add("copy kept behind the picked copy")
                if layout == "nan first":
                    assert la[0] == 0 and la[1] == 4 and res[1][0] == -3, (where, la[:4])
    assert {0, 3, 4, 5} <= reached, (kind_name, n, reached)
    print(kind_name, n, "reached:", sorted(map(str, reached)))


@pytest.mark.parametrize("n", rc.FRONT_NS)
@pytest.mark.parametrize("kind_name", KINDS)
def test_front_behind_an_armed_count(handle, capi, kind_name, n):
    """the bars of tests/test_gpu_retirement.py, planted from the unarmed numbers of the pair's best near-true model"""
    moved = 0
    for pi in MODEL_PAIRS:
        for layout in ("plain", "garbage first"):
            d = _unarmed(handle, capi, kind_name, n, pi, layout)
            k = rc.DUP_SLOTS[1]  # a copy of the best near-true model, in every layout
            ck, sk = int(d["cu"][k]), float(d["su"][k])
            bars = [("tie", ck, sk), ("score + 1 ulp", ck, float(np.nextafter(sk, np.inf))), ("nothing breaks", n - 1, TINY)] + ([("count - 1", ck - 1, sk)] if ck > 0 else [])
            for name, rec_cnt, rec_score in bars:
                for pick in (3, 48):
                    res = handle.front_models(d["kind"], d["models"], d["x1"], d["x2"], rc.THR, pick, rec_cnt, rec_score)
                    where = (kind_name, n, pi, layout, name, pick)
                    la = _check_front(d, pick, (rec_cnt, rec_score), res, where)
                    on_lists = np.flatnonzero(la >= 3)
                    if name == "nothing breaks":
                        # only a hypothesis every correspondence is a candidate of (the inf model is one, whatever the pair) passes this count
                        assert len(on_lists) and (d["cand"][on_lists] == n).all(), (where, on_lists[:8])
                        continue
                    assert len(on_lists) and la[on_lists[0]] == 4, (where, "the earliest SURVIVOR is picked", on_lists[:4], la[on_lists[:4]])
                    if layout == "garbage first":
                        assert la[0] == 1 and on_lists[0] > 0, (where, "slot 0 holds garbage a near-true bar retires", la[:4])
                        moved += 1
    assert moved >= 6
