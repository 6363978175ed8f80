"""The history matrix of tests/test_gpu_history.py for the entry points of include/mdrp_classic_models.h: every call of
tests/classic_models_history_cases.py behind every predecessor of tests/history_cases.py, behind the ranked baseline calls of
tests/classic_history_cases.py and behind the other new calls, and every probe of those two tables behind every new call, on one handle each, must
return the bytes of a fresh handle.  Every comparison is of bytes."""
import pytest

import classic_history_cases as chc
import classic_models_history_cases as mhc
import history_cases as hc
from test_gpu_history import _fresh_run, _records, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fresh():
    """{name: byte strings} of every new call and of every probe of the two tables on a handle of its own: computed once, never changed"""
    with pytest.MonkeyPatch.context() as mp:
        return {p.name: _fresh_run(p, mp)[0] for p in mhc.probes() + chc.probes() + hc.probes()}


def test_fresh_results_are_reproducible_and_no_empty_result(fresh, monkeypatch):
    bad = []
    for p in mhc.probes():
        again, _ = _fresh_run(p, monkeypatch)
        assert len(again) == len(p.outputs) == len(fresh[p.name]), p
        bad += hc.mismatches("a fresh handle", p, again, fresh[p.name])
        r = _records(fresh[p.name][0])
        assert int(r["num_inliers"].max()) > {3: 5, 4: 6, 5: 7}[p.kind], (p, r["num_inliers"].tolist())
        assert int(r["refinements"].max()) >= (1 if getattr(p, "stages", 3) else 0) and (p.family == "prior" or int(r["iterations"].max()) == 0), p
    assert not bad, bad
    # the models were read: the prior-free call on the same pairs is another run
    prior = next(p for p in mhc.probes() if p.name == "classic_prior_device")
    plain = hc._estimate("plain_twin", prior.kind, hc.S5, prior.seed, True, probe=False)
    assert _records(fresh[prior.name][0]).tobytes() != _records(_fresh_run(plain, monkeypatch)[0][0]).tobytes()


def _behind(pred, probes, fresh, monkeypatch):
    from mdrp_amd import _capi as capi
    bad = []
    for p in probes:
        h = capi.Handle(0)
        try:
            _run(pred, h, monkeypatch)
            bad += hc.mismatches(pred, p, _run(p, h, monkeypatch), fresh[p.name])
        finally:
            h.close()
    return bad


@pytest.mark.parametrize("probe", [p.name for p in mhc.probes()])
def test_a_new_calls_result_does_not_depend_on_the_call_before(fresh, monkeypatch, probe):
    """behind every predecessor of the table (probes, clean twins, larger calls, other schedule knobs, a backed-off fused tail, refusals), behind the
    ranked baseline calls and behind the other new calls"""
    p = next(c for c in mhc.probes() if c.name == probe)
    bad = []
    for pred in hc.predecessors() + chc.probes() + mhc.probes():
        bad += _behind(pred, [p], fresh, monkeypatch)
    assert not bad, bad


@pytest.mark.parametrize("predecessor", [p.name for p in mhc.probes()])
def test_no_probe_of_the_tables_depends_on_a_new_call_before_it(fresh, monkeypatch, predecessor):
    pred = next(c for c in mhc.probes() if c.name == predecessor)
    bad = _behind(pred, hc.probes() + chc.probes(), fresh, monkeypatch)
    assert not bad, bad


@pytest.mark.parametrize("pair", range(len(mhc.back_to_back())), ids=[f"{a.name}-{b.name}" for a, b in mhc.back_to_back()])
def test_device_calls_back_to_back_without_draining(monkeypatch, pair):
    """tests/test_gpu_history.py's back-to-back test on pairs with a call from models: the second call queued while the first may still run"""
    from mdrp_amd import _capi as capi
    first, second = mhc.back_to_back()[pair]
    (want_first, _), (want_second, _) = _fresh_run(first, monkeypatch), _fresh_run(second, monkeypatch)
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
