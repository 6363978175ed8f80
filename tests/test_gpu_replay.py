"""The bookkeeping train against the sequential loop, exactly (mdrp_replay_slots).

k_scan (all four instantiations), k_lo_plan, walk_pair as k_walk and k_walk_ckpt, and the budget checkpoints carry the claim that the reference's
sequential LO-RANSAC is reproduced in phase-split form.  Whole estimates reach them with 5 to 18 triggers per run; here they run on planted slot
tables (tests/replay_cases.py) where every iteration can break a record, and are compared with the reference's loop restated over tables
(tests/replay_ref.py, pinned to the oracle's orc_ransac by tests/test_replay_host.py).  No tolerance anywhere.  For every case:
  1. the trigger list (iter, k_ref, k_min, cnt_min, cnt_ref, score_min bit for bit) behind each chunk's scan and for the super-chunk
  2. best_min_cnt / best_min_score behind each scan
  3. the LO plan: begin, end, prefix, total
  4. the state behind the walk: iterations, refinements, num_inliers, model_score, inlier_ratio, dyn_max_iter, active, and `best` by the id in q[0]
  5. n_active and max_needed
  6. a chain of super-chunks, and any other split of the same iterations, against the one-shot loop
  7. every checkpoint against the loop run with max_iterations = K_c
The dynamic bound of 2^64 - 1 (dyn_num_trials_mult = -1, success_prob = 0.5, an inlier ratio near 0.7; or planted) is among the cases: first_stop
once computed dyn_max_iter + 1 in uint64_t, which wrapped to 0 there and ended the run at min_iterations + 1 where the reference runs to
max_iterations.  Needs an MI355X:  pytest -m gpu."""
import numpy as np
import pytest

import replay_cases as rc
import replay_ref as rr

pytestmark = pytest.mark.gpu

WALK_FIELDS = ("iterations", "refinements", "num_inliers", "model_score", "inlier_ratio", "dyn_max_iter", "active", "best")


@pytest.fixture(scope="module")
def handle():
    from mdrp_amd import _capi
    return _capi.default_handle(0)


def _bits(x):
    return np.float64(x).view(np.uint64)


def _state_records(capi, states):
    a = np.zeros(len(states), dtype=capi.REPLAY_STATE_DTYPE)
    for f in rr.STATE_FIELDS[:-1]:
        a[f] = [s[f] for s in states]
    a["best"]["q"][:, 0] = [s["best"] for s in states]
    return a


def _state_of(rec):
    st = {f: rec[f].item() for f in rr.STATE_FIELDS[:-1]}
    st["best"] = float(rec["best"]["q"][0])
    return st


_MODELS, _RUNS = {}, {}


def _model_table(capi, ids):
    key = id(ids)
    if key not in _MODELS:
        m = np.zeros(ids.shape, dtype=capi.MODEL_DTYPE)
        m["q"][..., 0] = ids
        _MODELS[key] = (ids, m)  # (keeps `ids` alive: its id is the key)
    return _MODELS[key][1]


def run_case(handle, case):
    """the case's chain on the device: one replay_slots result per super-chunk (states and checkpoints of one call feed the next)"""
    from mdrp_amd import _capi as capi
    if case["name"] in _RUNS:
        return _RUNS[case["name"]]
    opt = case["opt"]
    ro = capi.ransac_opt_from_dict(dict(max_iterations=opt.max_iterations, min_iterations=opt.min_iterations, dyn_num_trials_mult=opt.dyn_num_trials_mult,
                                        success_prob=opt.success_prob))
    states, ck, c0, out = _state_records(capi, case["states"]), None, case["chunk_start"], []
    for lens in case["supers"]:
        r0, r1 = c0 - case["chunk_start"], c0 - case["chunk_start"] + sum(lens)
        cut = lambda get: np.stack([get(t)[r0:r1].reshape(-1) for t in case["tables"]])
        res = handle.replay_slots(case["mps"], opt.sample_sz, c0, lens, ro, states, cut(lambda t: t.score), cut(lambda t: t.cnt),
                                  cut(lambda t: _model_table(capi, t.ids)), cut(lambda t: t.lo_score), cut(lambda t: t.lo_cnt),
                                  cut(lambda t: _model_table(capi, t.lo_ids)), budgets=case["budgets"], checkpoints=ck)
        out.append(res)
        states, ck, c0 = res["states"], res["checkpoints"] if case["budgets"] else None, c0 + sum(lens)
    _MODELS.clear()
    _RUNS[case["name"]] = out
    return out


def _check_super_chunk(case, c0, lens, res, exp):
    """items 1 to 5 for one call; exp: replay_ref.super_chunk's dict per pair"""
    name, batch, opt = case["name"], len(exp), case["opt"]
    assert list(res["scan_inst"]) == [10 * case["mps"] + (4 if case["mps"] == 4 and ln >= 1024 else 1) for ln in lens], (name, res["scan_inst"])
    ends = []
    for p, e in enumerate(exp):
        want = [t for ch in e["chunk_triggers"] for t in ch]
        got = res["triggers"][p]
        assert len(got) == len(want), (name, p, case["patterns"][p], case["starts"][p], len(got), len(want))
        for f in ("iter", "k_ref", "k_min", "cnt_min", "cnt_ref"):
            w = np.array([t[f] - (c0 if f == "iter" else 0) for t in want], dtype=np.int64)
            bad = np.nonzero(got[f].astype(np.int64) != w)[0]
            assert not len(bad), (name, p, case["patterns"][p], f, int(bad[0]), got[f][bad[:4]], w[bad[:4]])
        assert np.array_equal(got["score_min"].view(np.uint64), np.array([t["score_min"] for t in want], dtype=np.float64).view(np.uint64)), (name, p, "score_min")
        seen = 0
        for c, ch in enumerate(e["chunk_triggers"]):  # behind each chunk's scan: the list so far, and the running records
            seen += len(ch)
            assert res["n_triggers"][c, p] == seen, (name, p, c, res["n_triggers"][c, p], seen)
            assert int(res["scan_cnt"][c, p]) == e["records"][c][0] and _bits(res["scan_score"][c, p]) == _bits(e["records"][c][1]), \
                (name, p, c, res["scan_cnt"][c, p], res["scan_score"][c, p], e["records"][c])
        ends.append(seen)
        st, ws = _state_of(res["states"][p]), e["state"]
        for f in rr.STATE_FIELDS:
            same = _bits(st[f]) == _bits(ws[f]) if isinstance(ws[f], float) else st[f] == ws[f]
            assert same, (name, p, case["patterns"][p], case["starts"][p], f, st[f], ws[f], "stop iterations", st["iterations"], ws["iterations"])
    ends = np.array(ends)
    assert np.array_equal(res["begin"], np.zeros(batch, np.int32)) and np.array_equal(res["end"], ends), (name, "plan ranges")
    assert np.array_equal(res["prefix"], np.r_[0, np.cumsum(ends)]) and res["total"] == ends.sum(), (name, "plan prefix")
    live = [e["state"] for e in exp if e["state"]["active"]]
    assert res["n_active"] == len(live), (name, res["n_active"], len(live))
    assert res["max_needed"] == max([rr.need_of(s, opt) for s in live], default=0), (name, res["max_needed"])


def _check_checkpoints(case, results, expected):
    """item 7: behind the chain, checkpoint c of every pair is the loop run with max_iterations = K_c"""
    ck = results[-1]["checkpoints"]
    for p, st0 in enumerate(case["states"]):
        want = {}
        for res in expected:
            want.update(res[p]["checkpoints"])
        for c, K in enumerate(case["budgets"]):
            got = _state_of(ck[c, p])
            if not st0["active"]:  # a pair that never iterates reports its state at every budget
                w, skip = dict(st0), ()
            else:
                assert K in want, (case["name"], p, K)
                w, from_max = want[K]
                # (the bound copied from max_iterations on the <= 0.0001 branch is K in the run with that maximum: not a property of the result)
                skip = ("dyn_max_iter",) if from_max else ()
            for f in WALK_FIELDS:
                if f not in skip:
                    same = _bits(got[f]) == _bits(w[f]) if isinstance(w[f], float) else got[f] == w[f]
                    assert same, (case["name"], p, "budget", K, f, got[f], w[f])


@pytest.mark.parametrize("index", range(len(rc.case_list())), ids=[name for name, _, _ in rc.case_list()])
def test_the_train_is_the_sequential_loop(handle, index):
    """items 1 to 5 behind every call of the case's chain, item 7 behind the chain"""
    case = rc.case_list()[index][2]()
    results, expected = run_case(handle, case), rc.expected(case)
    c0 = case["chunk_start"]
    for lens, res, exp in zip(case["supers"], results, expected):
        _check_super_chunk(case, c0, lens, res, exp)
        c0 += sum(lens)
    if case["budgets"]:
        _check_checkpoints(case, results, expected)


@pytest.mark.parametrize("mps", (4, 12, 16))
def test_any_split_of_the_iterations_gives_the_same_run(handle, mps):
    """item 6: three super-chunks (63 | 65, 256, 1024 | 100), two chunks (1024 | 484) and one chunk of 1508 iterations over the same tables — the
    same state behind the last call, which is the one-shot loop's, and the same triggers up to each pair's stop (the scans of a super-chunk run
    to its end, so what lies behind a stop depends on the split)"""
    runs = {w: run_case(handle, rc.multi_case(mps, w)) for w in ("chain", "chain_b", "chain_c")}
    case = rc.multi_case(mps, "chain")
    stops = 0
    for p, (st0, tab) in enumerate(zip(case["states"], case["tables"])):
        one_shot, executed, _ = rr.loop(tab, st0, case["opt"], 1508)
        stops += st0["active"] and not one_shot["active"]
        lists = {}
        for w, results in runs.items():
            got = _state_of(results[-1]["states"][p])
            for f in WALK_FIELDS:
                assert _bits(got[f]) == _bits(one_shot[f]) if isinstance(one_shot[f], float) else got[f] == one_shot[f], (mps, w, p, f, got[f], one_shot[f])
            c0, tr = 0, []
            for lens, res in zip(rc.MULTI[w], results):
                tr += [(int(t["iter"]) + c0, int(t["k_ref"]), int(t["k_min"]), int(t["cnt_min"]), int(t["cnt_ref"]), int(_bits(t["score_min"])))
                       for t in res["triggers"][p] if int(t["iter"]) + c0 < one_shot["iterations"]]
                c0 += sum(lens)
            lists[w] = tr
        want = [(t["iter"], t["k_ref"], t["k_min"], t["cnt_min"], t["cnt_ref"], int(_bits(t["score_min"]))) for t in executed] if st0["active"] else []
        # (a trigger ON the stop iteration is listed but not executed: it is not below the stop)
        assert lists["chain"] == lists["chain_b"] == lists["chain_c"] == want, (mps, p)
    assert stops >= 3, stops


def test_the_cases_reach_what_they_claim(handle):
    """all four k_scan instantiations; n_triggers == trig_cap; a step the early-out skips and one it does not; a lane with two triggers; each stop
    position — on the device's own output (tests/test_replay_host.py asserts the same on the yardstick)"""
    inst, full, skipped, taken, lane2, positions = set(), 0, 0, 0, 0, set()
    for name, claim, make in rc.case_list():
        if not (name.startswith(("long", "stop")) or name.startswith("edge") and name.endswith("_257")):
            continue
        case = make()
        res = run_case(handle, case)[0]
        inst |= set(int(i) for i in res["scan_inst"])
        ln = case["supers"][0][0]
        for p, tr in enumerate(res["triggers"]):
            its = tr["iter"].astype(np.int64)
            full += len(its) == ln and ln >= 1024
            if len(its):
                steps = 64 * (4 if res["scan_inst"][0] == 44 else 1)
                skipped += len(np.unique(its // steps)) < (ln + steps - 1) // steps
                taken += 1
                lane2 += res["scan_inst"][0] == 44 and len(np.unique(its // 4)) < len(its)
        if claim in rc.STOP_POSITIONS:
            st = _state_of(res["states"][0])
            its = res["triggers"][0]["iter"].tolist()
            if claim == "nowhere":
                assert st["active"] and st["iterations"] == 200
            elif claim == "at_max":
                assert not st["active"] and st["iterations"] == case["opt"].max_iterations < 200
            elif claim == "on_trigger":
                assert not st["active"] and st["iterations"] in its and st["refinements"] == sum(i < st["iterations"] for i in its)
            elif claim == "after_trigger":
                assert not st["active"] and st["iterations"] - 1 in its and st["refinements"] == sum(i < st["iterations"] for i in its)
            else:
                assert not st["active"] and min(its) < st["iterations"] - 1 and max(its) > st["iterations"] and st["iterations"] not in its and st["iterations"] - 1 not in its
            positions.add((case["opt"].sample_sz, claim))
    assert inst == {41, 44, 121, 161}, inst
    assert min(full, skipped, taken, lane2) > 0, (full, skipped, taken, lane2)
    assert positions == {(s, c) for s in (3, 5, 7) for c in rc.STOP_POSITIONS}, positions
