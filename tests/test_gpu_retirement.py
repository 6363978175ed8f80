"""The three retirement stages ARMED, decision by decision (mdrp_retire_models).

k_count (both phases), k_bound (monotone exit, repack through LDS) and the bail-out of the three exact sweeps drop ~98 % of the hypotheses by proving that
they cannot beat the pair's running records.  The older unit entry points run those kernels without records; with records they were reached through
whole-estimator runs only, where a wrong retirement shows only when a true record breaker happens to sit on the margin of a bar.  Here the bars are
planted ON the margin: from the unarmed device results (c_k, s_k) of a near-true model k — the exact tie, one ulp above in score, one below in count
(with the score tied, and with a score k does not beat), a bar nothing breaks, and no record — and every decision of the armed train is compared with the record test evaluated in NumPy on the UNARMED stages'
own numbers (mdrp_count_candidates, mdrp_bound_models, mdrp_score_models, which the suite pins to the oracle) and with the oracle's exact scores.

What is asserted, for one-phase and two-phase counts at every split point the pair's statistics and three fixed garbage rates give, with and without
k_bound, through each of k_score / k_score_split / k_score_w:
  1. a model that beats a record on the unarmed numbers reaches the sweep and leaves the slot of the run without records, bit for bit; one that beats it
     by the oracle (score margin 1e-9 = ten times the suite's score tolerance 1e-10) is not retired, with the oracle's count and its score to 1e-10
  2. a retired model (count -2) beats no record, on the unarmed numbers and by the oracle
  3. k_count's survivors are exactly  cand > rec_cnt  or  thr (n - cand) < rec_score (1 + 1e-12), whatever the split; phase A leaves undecided
     exactly the hypotheses that could still break a record if all records behind the split point of count_split_tiles (restated in
     retirement_cases.split_tiles) were candidates, and none where the rule does not split the pair; a count without records leaves the pair's
     statistics (sum of cand, models x n)
  4. of those, k_bound retires exactly  count_ub <= rec_cnt  and  score_lb >= rec_score (1 + 1e-12)  (count_ub = n is not judged against
     rec_cnt >= n: the unit entry point reports min(n, .), which hides the kernel's + 1 there)
  5. the NaN and the inf model (and the zero matrix of the 7-point kind) are never retired by k_count or k_bound.  The zero-QUATERNION pose is the
     rotation I (quat_to_R), a finite garbage model like any other: 3 and 4 decide it.  In the sweep a special model leaves its slot of the run
     without records or is bailed out with the proof of 2 (the NaN model has no inlier: score thr n, which beats no record here)
  6. k_bound adds no survivor: without it nothing is left at stage 2, and what reaches the sweep with it reaches it without it
Needs an MI355X:  pytest -m gpu."""
import numpy as np
import pytest

import retirement_cases as rc

pytestmark = pytest.mark.gpu

M = rc.NUM_MODELS
KINDS = ("CALIB", "VARYING_FOCAL", "FUNDAMENTAL_7PT")  # the instantiations <true, false>, <false, false>, <false, true> of every sweep
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
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


_PLANS = {}


def _plan(handle, capi, kind_name, n, pi):
    """Per bar model k of the pair: the device models (with k's duplicates), the three unarmed stages on them, the oracle, and the bars.  Computed once
    per (kind, n, pair) and shared by the tests."""
    key = (kind_name, n, pi)
    if key in _PLANS:
        return _PLANS[key]
    kind = getattr(capi, kind_name)
    x1, x2, ms = rc.pair_case(n, pi)
    raw = kind == capi.FUNDAMENTAL_7PT
    rows = rc.fundamentals(n, pi) if raw else ms
    so, co = rc.oracle_scores(n, pi, kind == capi.CALIB)

    def device_models(r):
        return np.array([capi.fundamental_to_model(f.reshape(3, 3)) for f in r]) if raw else capi.array_to_models(r)

    s0, c0 = handle.score_models(kind, device_models(rows), x1, x2, rc.THR)
    order = sorted(rc.NEAR_TRUE, key=lambda k: (int(c0[k]), -float(s0[k])))
    out = []
    for k in rc.bar_models(order):
        models = device_models(rc.with_duplicates(rows, k))
        cand = handle.count_candidates(kind, models, x1, x2, rc.THR).astype(np.int64)
        lb, ub = handle.bound_models(kind, models, x1, x2, rc.THR)
        su, cu = handle.score_models(kind, models, x1, x2, rc.THR)
        ck, sk = int(cu[k]), float(su[k])
        bars = [("tie", ck, sk), ("score + 1 ulp", ck, float(np.nextafter(sk, np.inf))), ("nothing breaks", n - 1, TINY), ("no record", 0, None)]
        if ck > 0:  # (a bar one inlier below a model without inliers cannot be planted)
            bars.insert(2, ("count - 1", ck - 1, sk))
            # ... and one that k breaks on count ALONE: its score is no better than the inflated record (1e-12), so only  cnt > rec_cnt  keeps it
            bars.insert(3, ("count - 1, score worse", ck - 1, sk * (1.0 - 4e-12)))
        out.append(dict(k=k, models=models, cand=cand, lb=lb, ub=ub.astype(np.int64), su=su, cu=cu.astype(np.int64), bars=bars,
                        so=rc.with_duplicates(so, k), co=rc.with_duplicates(co, k), stat=(int(cand.sum()), M * n), raw=raw, cand_a={}))
    _PLANS[key] = (kind, x1, x2, out)
    return _PLANS[key]


def _prefix_candidates(handle, kind, x1, x2, d, n, ta):
    """k_count's candidates among the pair's first ta tiles (256 records each), per model, from the UNARMED count.  The filter's threshold depends on
    the pair's coordinate box, so the prefix is counted together with the records X behind it that span the box (at most four), once and twice:
    cand(P + X) = cand(P) + cand(X)  and  cand(P + X + X) = cand(P) + 2 cand(X)."""
    if ta not in d["cand_a"]:
        r = 256 * ta
        assert r < n
        far = sorted({int(np.argmax(np.abs(c))) for c in (x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1])} - set(range(r)))
        once = handle.count_candidates(kind, d["models"], np.concatenate([x1[:r], x1[far]]), np.concatenate([x2[:r], x2[far]]), rc.THR).astype(np.int64)
        twice = handle.count_candidates(kind, d["models"], np.concatenate([x1[:r], x1[far], x1[far]]), np.concatenate([x2[:r], x2[far], x2[far]]), rc.THR).astype(np.int64)
        d["cand_a"][ta] = 2 * once - twice
    return d["cand_a"][ta]


def _count_modes(n, rec_cnt, rec_score, stat):
    """[(two_phase flag, cand_stat, tiles of phase A)]: one armed launch, and a two-phase count per distinct split point (one unsplit at least)"""
    n_tiles = rc.count_tiles(n)
    modes, seen = [(0, (0, 0), n_tiles)], set()
    for st in (stat,) + rc.RATE_STATS:
        ta = rc.split_tiles(n, rc.THR, rec_cnt, rc.DBL_MAX if rec_score is None else rec_score, *st)
        if ta not in seen:
            seen.add(ta)
            modes.append((1, st, ta))
    return modes


def _check_run(n, d, bar, mode, bound, res, baseline, where, cand_a=None):
    name, rec_cnt, rec_score = bar
    two_phase, stat_in, ta = mode
    sc, cn, la, info, stat_out = res
    nr_sc, nr_cn = baseline
    armed = rec_score is not None
    inflated = rec_score * (1.0 + 1e-12) if armed else rc.DBL_MAX
    cand, lb, ub, su, cu, so, co = d["cand"], d["lb"], d["ub"], d["su"], d["cu"], d["so"], d["co"]
    ok = np.isfinite(so)  # (the special models have no oracle score)
    assert np.isin(la, (1, 2, 3)).all(), where
    # 3. the count's decisions
    count_surv = (cand > rec_cnt) | (rc.THR * (n - cand).astype(np.float64) < inflated) if armed else np.ones(M, dtype=bool)
    assert np.array_equal(la >= 2, count_surv), (where, "k_count's survivors", np.nonzero((la >= 2) != count_surv)[0][:8])
    assert info[1] == count_surv.sum(), (where, info)
    if two_phase and ta < rc.count_tiles(n):
        # phase A has seen ta tiles: undecided is who may still break a record if ALL the remaining records were candidates
        most = cand_a + (n - 256 * ta)
        undecided = (most > rec_cnt) | (rc.THR * (n - most).astype(np.float64) < inflated)
        assert info[0] == undecided.sum(), (where, "phase A of a split pair: undecided hypotheses", info, int(undecided.sum()), ta)
        assert 0 < info[0] < M, (where, "phase A of a split pair", info, ta)
    else:
        assert info[0] == 0, (where, "undecided hypotheses of a pair that is not split", info, ta)
    if two_phase and not armed:
        assert tuple(int(v) for v in stat_out) == (stat_in[0] + d["stat"][0], stat_in[1] + d["stat"][1]), (where, stat_out, d["stat"])
    else:
        assert tuple(int(v) for v in stat_out) == tuple(stat_in), (where, stat_out)
    # 4. the bound's decisions
    if bound:
        unjudged = (ub >= n) & (rec_cnt >= n)
        bound_out = count_surv & (ub <= rec_cnt) & (lb >= inflated)
        assert np.array_equal((la == 2)[~unjudged], bound_out[~unjudged]), (where, "k_bound's retirements", np.nonzero(((la == 2) != bound_out) & ~unjudged)[0][:8])
        assert not (la[(lb == 0) & (ub == n)] == 2).any(), where
    else:
        assert not (la == 2).any(), where
    assert info[2] == (la == 3).sum(), (where, info)
    # slots: a model that left early keeps "no record"; one that the sweep finished has the slot of the run without records
    ret = cn == -2
    assert ret[la < 3].all() and (sc[ret] == rc.DBL_MAX).all(), where
    assert np.array_equal(cn[~ret], nr_cn[~ret]) and _same_bits(sc[~ret], nr_sc[~ret]), (where, "slots of the finished models")
    # 1. must survive
    must = (cu > rec_cnt) | (su < rec_score) if armed else np.ones(M, dtype=bool)
    assert (la[must] == 3).all() and not ret[must].any(), (where, "a record breaker was retired", np.nonzero(must & ret)[0][:8], la[must & ret][:8])
    must_o = ok & ((co > rec_cnt) | (so < rec_score * (1.0 - 1e-9))) if armed else ok
    assert not ret[must_o].any(), (where, "a record breaker (oracle) was retired", np.nonzero(must_o & ret)[0][:8])
    assert np.array_equal(cn[must_o], co[must_o]), (where, np.nonzero(must_o & (cn != co))[0][:8])
    assert (np.abs(sc[must_o] - so[must_o]) <= 1e-10 * np.abs(so[must_o])).all(), where
    # 2. retired is proven
    if armed:
        assert (cu[ret] <= rec_cnt).all() and (su[ret] >= rec_score).all(), (where, "retired without proof", np.nonzero(ret & ((cu > rec_cnt) | (su < rec_score)))[0][:8])
        ro = ret & ok
        assert (co[ro] <= rec_cnt).all() and (so[ro] > rec_score * (1.0 - 1e-9)).all(), (where, "retired without proof (oracle)")
    else:
        assert not ret.any(), where
    # 5. special models
    unjudgeable = (rc.NAN_SLOT, rc.INF_SLOT) + ((rc.ZEROQ_SLOT,) if d["raw"] else ())
    assert (la[list(unjudgeable)] == 3).all(), (where, "a model no filter can judge was retired by one", la[list(rc.SPECIAL_SLOTS)])
    return la == 3


@pytest.mark.parametrize("n", rc.NS)
@pytest.mark.parametrize("kind_name", KINDS)
def test_armed_stages_decide_exactly_by_the_record_test(handle, capi, kind_name, n):
    for pi in range(len(rc.PAIRS)):
        kind, x1, x2, plans = _plan(handle, capi, kind_name, n, pi)
        for d in plans:
            assert (d["cand"][[rc.NAN_SLOT, rc.INF_SLOT]] == n).all() and (d["ub"][[rc.NAN_SLOT, rc.INF_SLOT]] == n).all() and (d["lb"][[rc.NAN_SLOT, rc.INF_SLOT]] == 0).all()
            # the run without records through each sweep kernel: nothing retired, and every slot the unarmed k_score's bit for bit (the three sweeps add
            # the inliers' r^2 in record order)
            baseline = {}
            for sweep in (capi.RETIRE_SWEEP_SCORE, capi.RETIRE_SWEEP_SPLIT, capi.RETIRE_SWEEP_WAVE):
                sc, cn, la, info, _ = handle.retire_models(kind, d["models"], x1, x2, rc.THR, 0, None, (0, 0), sweep)
                w = (kind_name, n, pi, d["k"], "no record", sweep)
                assert (la == 3).all() and tuple(info) == (0, M, M), (w, info)
                assert np.array_equal(cn, d["cu"]) and _same_bits(sc, d["su"]), (w, "the sweep without records against mdrp_score_models", np.nonzero(cn != d["cu"])[0][:8])
                baseline[sweep] = (sc, cn)
            for bar in d["bars"]:
                name, rec_cnt, rec_score = bar
                survivors = {}
                for mode in _count_modes(n, rec_cnt, rec_score, d["stat"]):
                    for bound in (0, capi.RETIRE_BOUND):
                        for sweep in (capi.RETIRE_SWEEP_SCORE, capi.RETIRE_SWEEP_SPLIT, capi.RETIRE_SWEEP_WAVE):
                            flags = (capi.RETIRE_TWO_PHASE if mode[0] else 0) | bound | sweep
                            stat_in = mode[1] if mode[0] else (0, 0)
                            if mode[0] and rec_score is None:
                                stat_in = (0, 0)  # (a count without records ADDS its statistics to these)
                            res = handle.retire_models(kind, d["models"], x1, x2, rc.THR, rec_cnt, rec_score, stat_in, flags)
                            w = (kind_name, n, pi, d["k"], name, "two-phase" if mode[0] else "one launch", mode[2], "bound" if bound else "no bound", sweep)
                            cand_a = _prefix_candidates(handle, kind, x1, x2, d, n, mode[2]) if mode[0] and mode[2] < rc.count_tiles(n) else None
                            reached = _check_run(n, d, bar, (mode[0], stat_in, mode[2]), bound, res, baseline[sweep], w, cand_a)
                            survivors.setdefault(bound, []).append(reached)
                # 6. the same set reaches the sweep whatever the count's split and the sweep kernel; the bound only takes away
                for bound, sets in survivors.items():
                    assert all(np.array_equal(s, sets[0]) for s in sets), (kind_name, n, pi, d["k"], name, bound)
                assert not (survivors[capi.RETIRE_BOUND][0] & ~survivors[0][0]).any(), (kind_name, n, pi, d["k"], name)


def test_the_cases_reach_the_split_points(handle, capi):
    """The split points (tiles of phase A of the pair's tiles) the cases above run, by the restated rule — which those tests assert through und_count:
    2 of 4; 2 and 3 of 5; 3, 5 and 6 of 8; 3, 5 and 7 of 9 (and a split after ONE tile: the bar nothing breaks gives it)."""
    reached = set()
    for kind_name in KINDS:
        for n in (1000, 1024, 1025, 2000, 2049):
            for pi in range(len(rc.PAIRS)):
                _, _, _, plans = _plan(handle, capi, kind_name, n, pi)
                for d in plans:
                    for _, rec_cnt, rec_score in d["bars"]:
                        reached |= {(ta, rc.count_tiles(n)) for two, _, ta in _count_modes(n, rec_cnt, rec_score, d["stat"]) if two and ta < rc.count_tiles(n)}
    print("split points reached:", sorted(reached))
    assert rc.REQUIRED_SPLITS <= reached, sorted(rc.REQUIRED_SPLITS - reached)
    assert {(1, 4), (1, 5), (1, 8), (1, 9)} <= reached, sorted(reached)
