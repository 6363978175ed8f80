"""The long soak (not collected by pytest): handles created and destroyed, then one handle walked over every call of tests/history_cases.py for many
laps, every probe checked against its fresh-handle bytes, with the device memory still free reported as it goes.  python tests/tools/endurance.py [laps]"""
import os
import sys
import time

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (TESTS, os.path.dirname(TESTS)):
    if path not in sys.path:
        sys.path.insert(0, path)
import numpy as np, torch
import history_cases as hc
from mdrp_amd import _capi as capi

laps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
setenv, delenv = hc.environ_setters()


def run(call, h):
    hc.apply_env(call.env, setenv, delenv)
    try:
        return call.run(h)
    finally:
        hc.apply_env(None, setenv, delenv)


def free_mb():
    return (free0 - torch.cuda.mem_get_info()[0]) / 2**20


free0 = torch.cuda.mem_get_info()[0]
fresh = {}
t0 = time.time()
for p in hc.probes():                     # create / use / destroy: the fresh-handle bytes, twice
    for it in range(2):
        h = capi.Handle(0, None)
        out = run(p, h)
        assert fresh.setdefault(p.name, out) == out, (p, it)
        h.close()
print("create/destroy x%d ok, %.1f s" % (2 * len(fresh), time.time() - t0), "free delta MB", free_mb())
calls = hc.predecessors()
rng = np.random.default_rng(0)
h = capi.Handle(0, None)
t0 = time.time()
for lap in range(laps):                   # same handle, every call in another order each lap
    for at in rng.permutation(len(calls)):
        out = run(calls[at], h)
        if calls[at].probe:
            bad = hc.mismatches(f"lap {lap}", calls[at], out, fresh[calls[at].name])
            assert not bad, bad
    print("lap %d ok, %d calls, %.1f s" % (lap, (lap + 1) * len(calls), time.time() - t0), "free delta MB", free_mb(), flush=True)
h.close()
