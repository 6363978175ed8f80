"""Every entry point's result is independent of what the handle did before (include/mdrp.h "The handle's history").

One mdrp_handle carries about sixty grow-only device buffers that no call clears, host-side state that steers the next call's schedule (the
first-chunk wish, the fused tail's back-off) and staging buffers from one call to the next.  Here every probe of tests/history_cases.py runs behind
every predecessor — itself, the other probes, its clean twin, larger calls, calls under other schedule knobs, a backed-off fused tail, refusals — on
one handle, and must return the bytes it returns on a fresh handle.  Stale data is only ever what a real earlier call leaves.  Every comparison is
of bytes."""
import numpy as np
import pytest

import history_cases as hc

pytestmark = pytest.mark.gpu

ESTIMATORS = ("estimate", "budgets", "prior", "ranked", "refine")


def _run(call, h, monkeypatch):
    """the call under its own schedule knobs (none for a probe), every knob unset again behind it"""
    hc.apply_env(call.env, monkeypatch.setenv, monkeypatch.delenv)
    try:
        call.stats = None
        return call.run(h)
    finally:
        hc.apply_env(None, monkeypatch.setenv, monkeypatch.delenv)


def _fresh_run(call, monkeypatch):
    from mdrp_amd import _capi as capi
    h = capi.Handle(0)
    try:
        out = _run(call, h, monkeypatch)
        return out, (dict(call.stats) if call.stats else None)
    finally:
        h.close()


@pytest.fixture(scope="module")
def fresh():
    """{probe name: (byte strings, last_stats() or None)} of every probe on a handle of its own: computed once, shared by the tests, never changed"""
    with pytest.MonkeyPatch.context() as mp:
        return {p.name: _fresh_run(p, mp) for p in hc.probes()}


def _records(raw):
    from mdrp_amd import _capi as capi
    return np.frombuffer(raw, dtype=capi.RESULT_DTYPE)


def test_fresh_results_are_reproducible(fresh, monkeypatch):
    """the baseline of everything below: a probe on two fresh handles"""
    bad = []
    for p in hc.probes():
        again, _ = _fresh_run(p, monkeypatch)
        assert len(again) == len(p.outputs) == len(fresh[p.name][0]), p
        bad += hc.mismatches("a fresh handle", p, again, fresh[p.name][0])
    assert not bad, bad


@pytest.mark.parametrize("predecessor", [c.name for c in hc.predecessors()])
def test_a_calls_result_does_not_depend_on_the_call_before(fresh, monkeypatch, predecessor):
    from mdrp_amd import _capi as capi
    pred = hc.by_name(predecessor)
    gives_up = pred.env == hc.FUSE_GIVE_UP
    bad = []
    for p in hc.probes():
        h = capi.Handle(0)
        try:
            _run(pred, h, monkeypatch)
            if gives_up:  # (f) reaches what it claims: expired waits behind it, a handle that has backed off and runs the probe unfused
                assert pred.stats["fuse_timeouts"] > 0, (predecessor, pred.stats)
            got = _run(p, h, monkeypatch)
            if gives_up and p.family in ESTIMATORS:
                assert p.stats["fuse_timeouts"] == 0, (predecessor, p, p.stats)
            bad += hc.mismatches(pred, p, got, fresh[p.name][0])
        finally:
            h.close()
    assert not bad, bad


@pytest.mark.parametrize("pair", range(len(hc.back_to_back())), ids=[f"{a.name}-{b.name}" for a, b in hc.back_to_back()])
def test_device_calls_back_to_back_without_draining(monkeypatch, pair):
    """Two device-resident calls with caller-owned outputs, the second issued while the first may still be running: no synchronize, no fetch and no
    allocation of ours between them.  Behind one final synchronise the first call's caller-owned outputs and the second call's records and
    outputs are those of fresh handles (the first call's records are gone: the contract of include/mdrp.h).  The calls share batch and n_max and
    differ in seed, cameras and n_per_pair, so per-call parameters that mixed would stay inside every buffer."""
    from mdrp_amd import _capi as capi
    first, second = hc.back_to_back()[pair]
    (want_first, _), (want_second, _) = _fresh_run(first, monkeypatch), _fresh_run(second, monkeypatch)
    assert first.data()["n"].tolist() != second.data()["n"].tolist() and first.focal != second.focal and first.shapes()[:2] == second.shapes()[:2]
    assert want_first[1:] != want_second[1:]
    h = capi.Handle(0)
    try:
        hc.apply_env(None, monkeypatch.setenv, monkeypatch.delenv)
        s1, s2 = first.prepare(), second.prepare()
        first.issue(h, s1)
        second.issue(h, s2)
        h.synchronize()
        bad = hc.mismatches(first, second, second.collect(h, s2), want_second)
        for name, a, b in zip(first.outputs[1:], first.owned(s1), want_first[1:]):
            at = hc.first_difference(a, b)
            if at is not None:
                bad.append((first.name, "its own " + name + " behind " + second.name, at))
        assert not bad, bad
    finally:
        h.close()


def _legal_first_chunk(call, first_chunk):
    """mdrp_schedule.h: a calibrated run of fewer than 8192 certain iterations keeps a sixteenth of them, at least 128 and at most 256, as its first
    chunk — or runs as one chunk where not twice as much remains; a longer one takes 128 ... 1024 in steps of 64 from the call before"""
    certain = min(call.max_iterations, call.min_iterations + 1)
    if certain >= 8192:
        return first_chunk in range(128, 1025, 64)
    lead = min(256, max(128, certain // 16 // 64 * 64))
    return first_chunk == (lead if 2 * lead <= certain else certain)


def test_a_long_walk_over_one_handle(fresh, monkeypatch):
    from mdrp_amd import _capi as capi
    calls = hc.predecessors()
    long_run = hc.long_run()
    want_long, stats_long = _fresh_run(long_run, monkeypatch)
    assert stats_long["first_chunk"] == 256  # (a fresh handle has seen no inlier ratio)
    order = np.random.default_rng(20261019).permutation(len(calls))
    bad = []
    h = capi.Handle(0)
    try:
        for lap in range(3):
            for at in np.roll(order, 17 * lap):
                c = calls[at]
                got = _run(c, h, monkeypatch)
                if c.probe:
                    bad += hc.mismatches(f"lap {lap}", c, got, fresh[c.name][0])
        assert not bad, bad
        plain = hc.by_name("k0_host")
        bad = hc.mismatches("the walk", plain, _run(plain, h, monkeypatch), fresh[plain.name][0])
        assert _legal_first_chunk(plain, plain.stats["first_chunk"]) and plain.stats["first_chunk"] == fresh[plain.name][1]["first_chunk"], plain.stats
        # ... which the handle may size from the hard pairs it has just seen (mdrp_stats::first_chunk): another schedule, the same bytes
        bad += hc.mismatches("the walk", long_run, _run(long_run, h, monkeypatch), want_long)
        assert _legal_first_chunk(long_run, long_run.stats["first_chunk"]), long_run.stats
        assert not bad, bad
    finally:
        h.close()


def test_the_cases_reach_what_they_claim(fresh, monkeypatch):
    from mdrp_amd import _capi as capi
    # a probe that runs fused and one that runs unfused: with the fused tail's bounded waits cut to 1 us the first one's expire, the second has none
    fused, unfused = hc.by_name("k0_host"), hc.by_name("k2_host")
    for p, expired in ((fused, True), (unfused, False)):
        h = capi.Handle(0)
        try:
            hc.apply_env(hc.FUSE_GIVE_UP, monkeypatch.setenv, monkeypatch.delenv)
            got = p.run(h)
            assert (p.stats["fuse_timeouts"] > 0) == expired, (p, p.stats)
            assert not hc.mismatches("bounded waits of 1 us", p, got, fresh[p.name][0])
        finally:
            hc.apply_env(None, monkeypatch.setenv, monkeypatch.delenv)
            h.close()
        assert fresh[p.name][1]["fuse_timeouts"] == 0
    assert fresh[fused.name][1]["first_chunk"] == 128 < fused.max_iterations and fresh[unfused.name][1]["first_chunk"] == 64 == unfused.max_iterations
    # no estimator probe is an empty result: a pair of each ends on a model that more correspondences support than its sample holds
    for p in hc.probes():
        if p.family in ("estimate", "budgets", "prior", "ranked"):
            r = _records(fresh[p.name][0][0])
            assert int(r["num_inliers"].max()) > {3: 5, 4: 6, 5: 7}.get(p.kind, 3) and int(r["refinements"].max()) >= 1, (p, r["num_inliers"].tolist())
    # the budgets probe refines more than one distinct state: more correspondences in the final refinements' sweeps than the plain run to its last budget
    budgets = hc.by_name("budgets_host")
    plain = hc.Estimate("plain_run_of_the_budgets_probe", hc.HOST, kind=budgets.kind, batch=budgets.batch, n_max=budgets.n_max, max_iterations=budgets.max_iterations,
                        min_iterations=budgets.min_iterations, seed=budgets.seed, probe=False)
    want, stats = _fresh_run(plain, monkeypatch)
    planes = _records(fresh[budgets.name][0][0]).reshape(len(budgets.budgets), budgets.batch)
    assert planes[-1].tobytes() == want[0]
    assert fresh[budgets.name][1]["final_cost_evals"] > stats["final_cost_evals"] > 0
    assert any(planes[0][k]["model"].tobytes() != planes[-1][k]["model"].tobytes() for k in range(budgets.batch))
    # the dynamic probe stops before max_iterations
    dynamic = hc.by_name("k0_device")
    it = _records(fresh[dynamic.name][0][0])["iterations"]
    assert dynamic.min_iterations < dynamic.max_iterations and ((it > dynamic.min_iterations) & (it < dynamic.max_iterations)).any(), it.tolist()
    # (d) ends in its first super-chunk, behind a run that filled the chunks it never reaches
    early = hc.by_name("early_dynamic_stop")
    out, stats = _fresh_run(early, monkeypatch)
    it, n = _records(out[0])["iterations"], early.calls[-1].data()["n"]
    assert stats["first_chunk"] == early.min_iterations + 1 < early.max_iterations  # (one chunk of the certain iterations: the whole first super-chunk)
    assert (it[n >= 3] > 0).all() and it.max() <= stats["first_chunk"] and (it[n < 3] == 0).all(), (stats, it.tolist())
    # the ranked probe's progressive samples were used: another course of the run than its "presorted" twin's
    ranked, presorted = (_records(fresh[name][0][0]) for name in ("ranked_host_150", "ranked_host_presorted"))
    assert (ranked["refinements"] != presorted["refinements"]).any() or (ranked["iterations"] != presorted["iterations"]).any()
    # (c) the two calls are beyond the limits of the LM kernels' LDS lists, every probe is inside both
    import os
    import re
    src = open(os.path.join(os.path.dirname(capi.__file__), "csrc", "mdrp_kernels.h")).read()
    list_max = int(re.search(r"LM_LIST_MAX_N = (\d+)", src).group(1))
    index_max = max(n for n in range(64, list_max + 1, 64) if 3 * n * 2 <= 32768)  # lm_mask_index_on: three u16 lists of the padded n in 32 KiB
    assert index_max < hc.by_name("beyond_the_lm_mask_index").n_max <= list_max < hc.by_name("beyond_the_lm_list").n_max
    assert max(p.n_max for p in hc.probes() if p.n_max) <= index_max
