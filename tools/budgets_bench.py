#!/usr/bin/env python3
"""What a budgets call buys: ONE call with the reference's graph list [10, 20, 50, 100, 200, 500, 1000] (eval.py:290-294,
min_iterations = max_iterations) against SEVEN plain calls, one per budget, at the headline shape (1024 pairs, N = 2000, 50 % outliers) and
for one pair per call at eval.py's N ~ 1000, from host buffers and from resident tensors.  The baseline is the seven plain calls on a library
built from the commit BEFORE the budgets entry points (--base-lib, or MDRP_BASE_LIB); the same seven calls on this tree's library are timed
beside it.  Both libraries are loaded into this one process (they share its HIP runtime), the three variants alternate within every
repetition, every timed region ends in fetched records, and the medians of --reps repetitions are written with their spreads (max - min).
The budgets call's records and masks are compared with this library's seven plain calls first: bytes.
    python tools/budgets_bench.py --base-lib /path/to/parent/libmdrp_hip.so [--reps 11] [--out profiles/budgets_bench.json]"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mdrp_amd import _capi, synth  # noqa: E402

GRAPH = [10, 20, 50, 100, 200, 500, 1000]
RO = {"max_epipolar_error": 2.0, "max_reproj_error": 16.0}
BO = {"loss_type": "TRUNCATED_CAUCHY"}


def binding_of(lib_path):
    """a second instance of the ctypes binding, bound to another build of the library"""
    spec = importlib.util.spec_from_file_location("mdrp_capi_base", _capi.__file__)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.LIB_PATH = lib_path
    return m


def opts(capi, k):
    return capi.ransac_opt_from_dict(dict(RO, max_iterations=k, min_iterations=k)), capi.bundle_opt_from_dict(BO)


class Shape:
    def __init__(self, name, B, n, first):
        self.name, self.B, self.n = name, B, n
        b = synth.make_batch(first, B, n, noise_px=0.5, depth_noise=0.02, outlier_frac=0.5)
        self.host = [b[k] for k in ("x1", "x2", "d1", "d2")]
        self.cams = np.zeros(B, dtype=_capi.CAMERA_DTYPE)
        self.cams["params"][:, 0] = 800.0
        dev = torch.device("cuda", 0)
        self.dev = [torch.from_numpy(a).to(dev) for a in self.host]
        self.mask1 = torch.zeros((B, n), dtype=torch.uint8, device=dev)
        self.maskc = torch.zeros((len(GRAPH), B, n), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    # each returns (records (C, B), masks (C, B, N) or None)
    def plain7(self, capi, h, resident):
        recs, masks = [], []
        for k in GRAPH:
            r, b = opts(capi, k)
            cams = np.ascontiguousarray(self.cams, dtype=capi.CAMERA_DTYPE)
            if resident:
                h.estimate_batch_device(0, *(t.data_ptr() for t in self.dev), self.B, self.n, r, b, None, cams, cams, self.mask1.data_ptr())
                recs.append(h.fetch_results(self.B))
            else:
                res, m = h.estimate_batch(0, *self.host, r, b, None, cams, cams)
                recs.append(res); masks.append(m)
        return np.stack(recs), (np.stack(masks) if masks else None)

    def budgets(self, capi, h, resident):
        r, b = opts(capi, GRAPH[-1])
        if resident:
            h.estimate_batch_budgets_device(0, *(t.data_ptr() for t in self.dev), self.B, self.n, r, b, GRAPH, None, self.cams, self.cams, self.maskc.data_ptr())
            return h.fetch_budget_results(len(GRAPH), self.B), None
        return h.estimate_batch_budgets(0, *self.host, r, b, GRAPH, None, self.cams, self.cams)


def timed(fn):
    t0 = time.perf_counter()
    fn()          # (ends in fetched records: the fetch waits for the handle's stream)
    return 1000.0 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base-lib", default=os.environ.get("MDRP_BASE_LIB"), help="libmdrp_hip.so built from the commit before the budgets entry points")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "budgets_bench.json"))
    a = ap.parse_args()
    if not a.base_lib or not os.path.exists(a.base_lib):
        sys.exit("budgets_bench: --base-lib (or MDRP_BASE_LIB) must name the baseline library")
    if a.reps < 11:
        sys.exit("budgets_bench: at least 11 repetitions")
    base = binding_of(os.path.abspath(a.base_lib))
    h_new, h_base = _capi.Handle(0), base.Handle(0)
    out = {"budgets": GRAPH, "reps": a.reps, "library": _capi.library_version(), "base_library": base.library_version(), "unit": "ms per call group, host clock",
           "cases": {}}
    for shape in (Shape("headline_1024x2000", 1024, 2000, 0), Shape("one_pair_1000", 1, 1000, 5000)):
        for resident in (False, True):
            variants = {"base_seven_plain_calls": lambda: shape.plain7(base, h_base, resident),
                        "seven_plain_calls": lambda: shape.plain7(_capi, h_new, resident),
                        "one_budgets_call": lambda: shape.budgets(_capi, h_new, resident)}
            want, got = variants["seven_plain_calls"](), variants["one_budgets_call"]()      # warm-up of both shapes of call, and the check
            variants["base_seven_plain_calls"]()
            same = want[0].tobytes() == got[0].tobytes() and (want[1] is None or want[1].tobytes() == got[1].tobytes())
            if resident:
                same = same and shape.maskc[-1].cpu().numpy().tobytes() == shape.mask1.cpu().numpy().tobytes()
            if not same:
                sys.exit(f"budgets_bench: {shape.name}: the budgets call does not return the seven plain calls' bytes")
            ms = {k: [] for k in variants}
            for _ in range(a.reps):
                for k, fn in variants.items():
                    ms[k].append(timed(fn))
            case = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v)} for k, v in ms.items()}
            b7, bc = case["base_seven_plain_calls"], case["one_budgets_call"]
            case["speedup_over_base"] = b7["median_ms"] / bc["median_ms"]
            case["gain_ms"] = b7["median_ms"] - bc["median_ms"]
            case["faster_by_more_than_both_spreads"] = bool(case["gain_ms"] > b7["spread_ms"] + bc["spread_ms"])
            case["bytes_equal_to_seven_plain_calls"] = True
            out["cases"][f"{shape.name}_{'resident' if resident else 'host'}"] = case
            print(shape.name, "resident" if resident else "host", json.dumps(case), flush=True)
    h_new.close(); h_base.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
