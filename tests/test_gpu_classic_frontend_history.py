"""The history matrix of tests/test_gpu_history.py for the entry points of include/mdrp_classic_frontend.h: every call of
tests/classic_frontend_history_cases.py behind a larger and a smaller call, other kinds, the monodepth front end in every form (it gathers into
the same buffers of the handle), a ranked baseline, the other new calls and refusals, and the probes of the other tables behind every new call, on
one handle each, must return the bytes of a fresh handle.  Every comparison is of bytes."""
import numpy as np
import pytest

import classic_frontend_history_cases as fhc
import history_cases as hc
from test_gpu_history import _fresh_run, _records, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fresh():
    """{name: byte strings} of every new call and of every follower on a handle of its own: computed once, never changed"""
    with pytest.MonkeyPatch.context() as mp:
        return {p.name: _fresh_run(p, mp)[0] for p in fhc.probes() + fhc.followers()}


def test_fresh_results_are_reproducible_and_no_empty_result(fresh, monkeypatch):
    bad = []
    for p in fhc.probes():
        again, _ = _fresh_run(p, monkeypatch)
        assert len(again) == len(p.outputs) == len(fresh[p.name]), p
        bad += hc.mismatches("a fresh handle", p, again, fresh[p.name])
        n = np.frombuffer(fresh[p.name][-1], dtype=np.int32)
        assert n.max() >= 200 and (n < 5).any(), (p, n.tolist())
        if p.estimate:
            r = _records(fresh[p.name][0])
            assert int(r["num_inliers"].max()) > {3: 5, 4: 6, 5: 7}[p.kind], (p, r["num_inliers"].tolist())
            assert int(r["refinements"].max()) >= 1 and int(r["iterations"].max()) == p.ransac_options()["max_iterations"], p
            mask = np.frombuffer(fresh[p.name][1], dtype=np.uint8)
            assert mask.max() == 1, p
    assert not bad, bad
    # the scores were read: the ranked estimate is another run than the unranked one on the same rows
    ranked = fhc.by_name("estimate_classic_image_pairs_ranked_5pt_f64")
    plain = fhc.PointImagePairs("unranked_twin_of_" + ranked.name, ranked.entry_points, kind=ranked.kind, estimate=True)
    assert fresh[ranked.name][0] != _fresh_run(plain, monkeypatch)[0][0]


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


@pytest.mark.parametrize("probe", [p.name for p in fhc.probes()])
def test_a_new_calls_result_does_not_depend_on_the_call_before(fresh, monkeypatch, probe):
    p = fhc.by_name(probe)
    bad = []
    for pred in fhc.predecessors():
        bad += _behind(pred, [p], fresh, monkeypatch)
    assert not bad, bad


@pytest.mark.parametrize("predecessor", [p.name for p in fhc.probes() + fhc.refusals()])
def test_no_probe_of_the_tables_depends_on_a_new_call_before_it(fresh, monkeypatch, predecessor):
    pred = next(c for c in fhc.probes() + fhc.refusals() if c.name == predecessor)
    bad = _behind(pred, fhc.followers(), fresh, monkeypatch)
    assert not bad, bad
