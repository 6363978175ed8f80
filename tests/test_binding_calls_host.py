"""mdrp_amd/_capi.py is the one route from Python to the kernels; this pins it on the CPU, call by call.  Every public method of Handle runs against
a recording stub of the library (tests/binding_cases.py): the symbol it calls, each argument after normalisation, and what it returns must equal
tests/golden/binding_calls.json, recorded from the binding before its per-family copies were folded (tests/tools/gen_golden_binding.py).  The same
file pins the refusals the binding raises itself, with type and message, and the signature of every public callable of _capi and poselib."""
import json
import os

import pytest

import binding_cases as bc
import mdrp_amd.poselib as poselib
from mdrp_amd import _capi

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_calls.json")) as f:
    GOLDEN = json.load(f)


def _plain(doc):
    return json.loads(json.dumps(doc))


def test_the_cases_are_the_golden_files_cases():
    assert sorted(GOLDEN["calls"]) == sorted(c[0] for c in bc.CASES) and len(GOLDEN["calls"]) == len(bc.CASES)
    assert sorted(GOLDEN["refusals"]) == sorted(c[0] for c in bc.REFUSALS) and sorted(GOLDEN["missing"]) == sorted(bc.MISSING)


def test_every_public_handle_method_has_a_case():
    covered = {method for _, method, _ in bc.CASES}
    assert not [m for m in bc.handle_methods() if m not in covered]
    for m in bc.handle_methods():  # a *_device method: with every optional pointer absent and with every one present
        if m.endswith("_device") and m not in ("copy_results_device", "copy_budget_results_device", "score_models_device"):
            ids = [cid for cid, method, _ in bc.CASES if method == m]
            assert any("absent" in i for i in ids) and any("present" in i for i in ids), m


@pytest.mark.parametrize("cid", [c[0] for c in bc.CASES])
def test_call(cid):
    got = _plain(bc.run_case(cid))
    assert got["calls"] == GOLDEN["calls"][cid]["calls"]
    assert got["returns"] == GOLDEN["calls"][cid]["returns"]


@pytest.mark.parametrize("cid", [c[0] for c in bc.REFUSALS])
def test_refusal_needs_no_library(cid):
    assert bc.run_refusal(cid) == GOLDEN["refusals"][cid]


@pytest.mark.parametrize("symbol", sorted(bc.MISSING))
def test_missing_symbol_is_refused(symbol):
    got = bc.run_missing(symbol)
    assert got == GOLDEN["missing"][symbol]
    assert got["type"] == "MdrpError" and symbol in got["message"] and "<library>" in got["message"] and "rebuild" in got["message"]


@pytest.mark.parametrize("name, module", [("_capi", _capi), ("poselib", poselib)])
def test_signatures(name, module):
    assert bc.signatures(module) == GOLDEN["signatures"][name]
