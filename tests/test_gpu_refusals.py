"""The entry layer's refusals, pinned: every probe of tests/refusal_cases.py (one valid tiny call per entry point with one defect, and every pair of
defects for one entry point of each family) must return the (return code, mdrp_last_error()) that tests/golden/entry_refusals.json records.  The
table was recorded (tests/tools/gen_golden_refusals.py) from the library as it was before the entry layer was single-sourced: codes, strings and
which of two refusals wins are the ABI's behaviour, not an implementation detail.  The raw symbols are called: the Handle wrappers would refuse first.

No probe relies on a crash: each is refused by host-side checks before the defective argument could be dereferenced.  Left out, because the entry
point named does NOT refuse the defect (the call would run, and a NULL would be read on the device):
  - null x1 on the device-resident estimators, which take their correspondences on trust: mdrp_estimate_batch_async,
    mdrp_estimate_batch_budgets_async, mdrp_estimate_batch_prior_async, mdrp_estimate_batch_ranked_async, mdrp_estimate_classic_ranked_async; and on
    mdrp_estimate_batch / mdrp_estimate_batch_budgets, which hand them to the sliced host front unchecked;
  - mem_space = 2 on mdrp_estimate_batch / mdrp_estimate_batch_budgets: anything but MDRP_MEM_HOST is taken as device memory there;
  - progressive_sampling = 1 on the refine entry points (they draw no samples and ignore it) and on the ranked ones (it is what they build);
  - real_focal_check = 1 on mdrp_refine_classic[_async]: no hypotheses, no check;
  - a budgets list that matches on mdrp_fetch_budget_results / mdrp_copy_budget_results_device: whether it is refused depends on the handle's last call.
Defects that do not apply to an entry point (no such argument) have no probe.  Pairs of defects that change the same argument are skipped."""
import json
import os

import pytest

import refusal_cases as rc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entry_refusals.json")


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        doc = json.load(f)
    return {e: {d: (code, doc["messages"][i]) for d, (code, i) in probes.items()} for e, probes in doc["table"].items()}


@pytest.fixture(scope="module")
def got():
    from mdrp_amd import _capi as capi
    h = capi.Handle(0)
    try:
        return rc.run_table(capi.load_library(), rc.Base(capi, h._h))
    finally:
        h.close()


def test_the_fixture_covers_the_probes_and_every_probe_is_a_refusal(want):
    assert sorted((e, "+".join(d)) for e, d in rc.probes()) == sorted((e, d) for e, probes in want.items() for d in probes)
    assert set(want) == set(rc.ENTRIES) == set(rc.SIGNATURES)
    assert all(code != 0 and msg for probes in want.values() for code, msg in probes.values())
    for e in rc.PAIRED:
        assert any("+" in d for d in want[e]), e


@pytest.mark.parametrize("entry", sorted(rc.ENTRIES))
def test_every_refusal_is_the_recorded_one(want, got, entry):
    bad = [(d, tuple(got[entry].get(d, ())), w) for d, w in want[entry].items() if tuple(got[entry].get(d, ())) != w]
    assert not bad and len(got[entry]) == len(want[entry]), bad


def test_a_refused_handle_still_estimates(got):
    """behind the whole table, on a handle of its own: a refusal leaves nothing behind that a later call could trip over"""
    import numpy as np
    from mdrp_amd import _capi as capi
    h = capi.Handle(0)
    try:
        base = rc.Base(capi, h._h)
        rc.run_table(capi.load_library(), base)
        a, names = base.args("mdrp_estimate_batch")
        a.update(kind=5, cam1=None, cam2=None)
        out, mask = h.estimate_batch(5, a["x1"], a["x2"], None, None, a["ropt"], a["bopt"])
        fresh = capi.Handle(0)
        try:
            out2, mask2 = fresh.estimate_batch(5, a["x1"], a["x2"], None, None, a["ropt"], a["bopt"])
        finally:
            fresh.close()
        assert out.tobytes() == out2.tobytes() and np.array_equal(mask, mask2)
    finally:
        h.close()
