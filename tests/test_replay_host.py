"""The bookkeeping train's yardstick and inputs without a GPU: tests/replay_ref.py is pinned to the oracle's orc_ransac on real pairs (tables filled
from the oracle's own sampler, solvers, scorers and LM), and the planted cases of tests/replay_cases.py meet the conditions the GPU tests rely on."""
import numpy as np
import pytest

import from_models_cases as fc
import from_models_ref as fm
import helpers
import prior_ref as pr
import replay_cases as rc
import replay_ref as rr
from oracle import pyorc as po

ANCHOR = [(name, n, its, dyn, si) for name, n, its in (("calib_p3p", 40, 1000), ("calib_p3p", 200, 300), ("calib_shift", 120, 400), ("shared", 60, 600),
                                                       ("shared", 200, 300), ("varying", 90, 500), ("varying", 150, 300))
          for dyn in (False, True) for si in (False, True) if not si or (n in (40, 60, 90) and dyn)]


@pytest.mark.parametrize("name,n,its,dyn,si", ANCHOR)
def test_the_table_loop_is_orc_ransac(name, n, its, dyn, si):
    """iterations, refinements, num_inliers, inlier_ratio and model_score of pyorc's orc_ransac, bit for bit, from a table that holds what the oracle's
    pieces give for every sample of the run — with dynamic stopping on and off, and (si) from the state score_initial_model leaves"""
    kind, es, _ = helpers.OPTIONS_KINDS[name]
    p = fc.make_pair(name, 91000 + n, n)
    ro, bo = fc.oracle_options(name, "HUBER")
    c1, c2 = (po.cam_flat(*fc.cameras(kind)[0]), po.cam_flat(*fc.cameras(kind)[1])) if kind == po.CALIB else (None, None)
    q = fm.prep(kind, p["x1"], p["x2"], ro, bo, c1, c2)
    d1, d2 = po.f64(p["d1"]), po.f64(p["d2"])
    min_it = 30 if dyn else its
    ro_n = po.ransac_opt(its, min_it, 3.0, 0.9999, q["rep"], q["eps"], 5 + n, es, q["ws"], si)
    lo = po.bundle_opt(max_iterations=25, loss_type=1, loss_scale=q["lo_loss_scale"], gradient_tol=1e-10, step_tol=1e-8, initial_lambda=1e-3, min_lambda=1e-10,
                       max_lambda=1e10)
    refine = lambda m: po.refine(kind, q["a1"], q["a2"], d1, d2, m, q["scale_reproj"], q["ws"], lo, es)[0]
    samples = po.draw_samples(int(ro_n.seed), n, its)
    mps = 4
    cnt, score, lo_cnt, lo_score = np.full((its, mps), -1, np.int32), np.zeros((its, mps)), np.zeros((its, mps), np.int32), np.zeros((its, mps))
    ids = 1.0 + np.arange(its * mps, dtype=np.float64).reshape(its, mps)
    model_of = {0.0: po.new_model()}
    nan_score = float(np.float64(n) * np.float64(q["sq_thr"]))
    n_nan = 0
    for i in range(its):
        for k, m in enumerate(pr.generate_models(kind, es, q["a1"], q["a2"], d1, d2, samples[i])):
            s, c = fm.score(kind, m, q)
            if np.isnan(m[0]) and (s, c) == (nan_score, 0):  # the reference's NaN pose: the slot state the solver kernel writes for it
                assert k == 0
                cnt[i, k], score[i, k] = -3, 0.0
                n_nan += 1
            else:
                cnt[i, k], score[i, k] = c, s
            r = refine(m)
            lo_score[i, k], lo_cnt[i, k] = fm.score(kind, r, q)
            model_of[float(ids[i, k])], model_of[-float(ids[i, k])] = np.array(m, copy=True), r
    tab = rr.Table(0, cnt, score, ids, lo_score, lo_cnt, -ids)
    opt = rr.options(its, min_it, 3.0, 0.9999, 3)
    st0 = rr.new_state(n, q["sq_thr"], dyn_max_iter=its)
    if si:  # the reset identity model, scored and LO-refined to no effect: records (0, its score), one refinement
        s0, c0 = fm.score(kind, po.new_model(), q)
        assert c0 == 0 and abs(s0 - nan_score) <= 1e-12 * nan_score
        st0.update(best_min_score=s0, model_score=s0, refinements=1)
    got, trig, _ = rr.loop(tab, st0, opt, its)
    slow, trig_slow, _ = rr.loop(tab, st0, opt, its, fast=False)
    assert got == slow and trig == trig_slow
    _, want, _ = po.ransac(kind, q["a1"], q["a2"], d1, d2, ro_n)
    print(name, n, its, "dyn" if dyn else "fixed", "stopped at", got["iterations"], "triggers", len(trig), "NaN models", n_nan, "oracle refinements", want.refinements)
    assert not got["active"] and got["iterations"] == want.iterations and (not dyn or want.iterations < its)
    assert got["model_score"] == want.model_score and got["inlier_ratio"] == want.inlier_ratio
    # the closing LO of ransac<>: one more refinement, which hands over its inlier count (not its score) when it scores below model_score
    s, c = fm.score(kind, refine(model_of[got["best"]]), q)
    assert got["refinements"] + 1 == want.refinements
    assert (c if s < got["model_score"] else got["num_inliers"]) == want.num_inliers
    assert len(trig) >= 3


def test_planted_inputs_meet_their_conditions():
    """every count that can become num_inliers keeps the bound before ceil 1e-9 (relative) away from every integer; fewer than 1 % of the drawn counts
    had to be redrawn for it; every start state keeps model_score <= best_min_score with a consistent ratio; no pair starts at or behind its stop"""
    cases = rc.all_cases()
    assert rc.DRAWS[0] > 10 ** 5 and rc.REDRAWS[0] < 0.01 * rc.DRAWS[0], (rc.DRAWS, rc.REDRAWS)
    seen = set()
    for case, _ in cases:
        opt = case["opt"]
        for st, tab in zip(case["states"], case["tables"]):
            assert st["model_score"] <= st["best_min_score"] and (st["n"] == 0 or st["inlier_ratio"] == st["num_inliers"] / st["n"]), (case["name"], st)
            assert st["active"] in (0, 1) and (st["n"] > 0 or not st["active"])
            if st["active"]:
                assert st["iterations"] == case["chunk_start"] and (st["iterations"] < opt.max_iterations or opt.max_iterations == 0), case["name"]
                assert not (st["iterations"] > opt.min_iterations and st["iterations"] > st["dyn_max_iter"]), case["name"]
            key = (id(tab.cnt), opt.dyn_num_trials_mult, opt.success_prob, opt.sample_sz)
            if st["n"] == 0 or key in seen:
                continue
            seen.add(key)
            for c in np.unique(np.r_[tab.cnt[tab.cnt >= 0], tab.lo_cnt.reshape(-1), st["num_inliers"]]).tolist():
                assert 0 <= c <= st["n"] and rc.safe_count(c, st["n"], opt), (case["name"], c)
        if case["budgets"]:
            b = case["budgets"]
            assert all(x < y for x, y in zip(b, b[1:])) and 1 <= b[0] and b[-1] <= opt.max_iterations


def test_the_skip_of_dull_iterations_changes_nothing():
    """loop(fast=True) leaves out iterations whose largest count and smallest score cannot break a record: same states and triggers as reading every slot"""
    for case in (rc.edge_case(4, 257), rc.edge_case(16, 65), rc.multi_case(12, "chain"), rc.budget_case(4)):
        rows = sum(sum(s) for s in case["supers"])
        for st, tab in zip(case["states"], case["tables"]):
            for stop in (True, False):
                assert rr.loop(tab, st, case["opt"], case["chunk_start"] + rows, stop=stop) == rr.loop(tab, st, case["opt"], case["chunk_start"] + rows, stop=stop, fast=False)


def test_the_planted_cases_reach_what_they_claim():
    """on the yardstick alone: a trigger in every iteration of a super-chunk, a lane of the four-iterations-per-lane scan with two triggers, a 64-lane
    step without a trigger and one with triggers in neighbouring lanes, k_ref != k_min and k_min = -1, every stop position for every sample size, the
    2^64 - 1 bound reached through the conversion, budgets on and next to triggers, and both sides of every chunk boundary"""
    full = lane2 = quiet = neighbours = differ = no_min = boundary = 0
    for case, _ in rc.all_cases():
        c0 = case["chunk_start"]
        for lens, res in zip(case["supers"], rc.expected(case)):
            for r in res:
                its = [t["iter"] - c0 for ch in r["chunk_triggers"] for t in ch]
                full += len(its) == sum(lens) and sum(lens) >= 1024
                if case["mps"] == 4 and len(lens) == 1 and lens[0] >= 1024:
                    lane2 += len({i // 4 for i in its}) < len(its)
                steps = {i // 64 for i in its}
                quiet += len(steps) < (sum(lens) + 63) // 64 and len(its) > 0
                neighbours += any(a + 1 == b and a // 64 == b // 64 for a, b in zip(its, its[1:]))
                differ += any(t["k_min"] >= 0 and t["k_min"] != t["k_ref"] for ch in r["chunk_triggers"] for t in ch)
                no_min += any(t["k_min"] < 0 for ch in r["chunk_triggers"] for t in ch)
                edges, off = [], 0
                for ln in lens[:-1]:
                    off += ln
                    edges.append(off)
                boundary += any(e - 1 in its and e in its for e in edges)
            c0 += sum(lens)
    print("full lists", full, "two in a lane", lane2, "quiet steps", quiet, "neighbouring lanes", neighbours, "k_ref != k_min", differ, "k_min = -1", no_min,
          "both sides of a chunk boundary", boundary)
    assert min(full, lane2, quiet, neighbours, differ, no_min, boundary) > 0
    for ssz in (3, 5, 7):
        claims = {}
        for case, claim in rc.stop_cases(ssz):
            r = rc.expected(case)[0][0]
            claims[claim] = r
            if claim in rc.STOP_POSITIONS:
                assert rc.stop_position(r, 0, 200, case["opt"]) == claim, (ssz, claim, r["state"], [t["iter"] for t in r["executed"]])
        assert set(rc.STOP_POSITIONS) <= set(claims)
        st = {k: v["state"] for k, v in claims.items()}
        tb = claims["trigger_on_bound"]
        assert tb["state"]["iterations"] == tb["state"]["dyn_max_iter"] + 1 and tb["executed"][-1]["iter"] == tb["state"]["dyn_max_iter"] - 1 and len(tb["executed"]) == 2
        assert (st["prob_one"]["dyn_max_iter"], st["prob_one"]["iterations"]) == (0, 31)
        assert (st["prob_above_one"]["dyn_max_iter"], st["prob_above_one"]["iterations"]) == (1 << 63, 150)
        assert st["mult_zero"]["dyn_max_iter"] == 0 and st["mult_zero"]["iterations"] == 31
        assert (st["mult_minus_one"]["dyn_max_iter"], st["mult_minus_one"]["iterations"]) == (2 ** 64 - 1, 180)  # never exceeded: the run ends at max_iterations
        assert (st["dyn_m1_no_trigger"]["dyn_max_iter"], st["dyn_m1_no_trigger"]["iterations"]) == (2 ** 64 - 1, 180)
        assert st["min_is_max_u64"]["iterations"] == 180 and st["max_zero"]["iterations"] == 0 and not st["max_zero"]["active"]
        assert st["ratio_high"]["dyn_max_iter"] == 25 and st["ratio_high"]["iterations"] == 26 and st["ratio_low"]["dyn_max_iter"] == 170
    for mps in (4, 12, 16):
        case = rc.budget_case(mps)
        b, on, after, behind_stop, before_first = set(case["budgets"]), 0, 0, 0, 0
        for chain in zip(*rc.expected(case)):
            done = [t["iter"] for r in chain for t in r["executed"]]
            on += any(i in b for i in done)
            after += any(i + 1 in b for i in done)
            last = chain[-1]["state"]
            behind_stop += (not last["active"]) and last["n"] > 0 and any(k > last["iterations"] for k in b) and bool(done)
            before_first += bool(done) and done[0] >= min(b)
        assert min(on, after, behind_stop, before_first) > 0, (on, after, behind_stop, before_first)
        assert 160 in b and 300 in b and [sum(s) for s in case["supers"]] == [160, 140]


def test_header_and_binding_agree(tmp_path):
    """mdrp_replay_slots is a new symbol within ABI 6, and the three structs of include/mdrp.h have the binding's sizes and field offsets (checked by a
    C compiler)"""
    import os
    import subprocess
    import ctypes as C
    from mdrp_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stddef.h>', '#include "mdrp.h"',
             f"_Static_assert(sizeof(mdrp_replay_state) == {_capi.REPLAY_STATE_DTYPE.itemsize}, \"state\");",
             f"_Static_assert(sizeof(mdrp_replay_trigger) == {_capi.REPLAY_TRIGGER_DTYPE.itemsize}, \"trigger\");",
             f"_Static_assert(sizeof(mdrp_replay) == {C.sizeof(_capi.Replay)}, \"replay\");"]
    for struct, dt in (("mdrp_replay_state", _capi.REPLAY_STATE_DTYPE), ("mdrp_replay_trigger", _capi.REPLAY_TRIGGER_DTYPE)):
        lines += [f"_Static_assert(offsetof({struct}, {f}) == {dt.fields[f][1]}, \"{f}\");" for f in dt.names]
    lines += [f"_Static_assert(offsetof(mdrp_replay, {f}) == {getattr(_capi.Replay, f).offset}, \"{f}\");" for f, _ in _capi.Replay._fields_]
    lines += ["typedef int (*replay_t)(mdrp_handle *, const mdrp_ransac_opt *, mdrp_replay *);", "replay_t a = mdrp_replay_slots;"]
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", str(src), "-I", os.path.join(root, "include"), "-o", str(tmp_path / "abi.o")], check=True)
    assert "mdrp_replay_slots" in _capi.EXPORTS and _capi.ABI_VERSION == 6
