"""What keeps tests/test_gpu_history.py from being vacuous, checked without a GPU: the table of tests/history_cases.py names every entry point of
include/mdrp.h that takes a handle, every estimator probe has the predecessors that could hurt it, the inputs are deterministic, and the probes are
harder than their clean twins."""
import os
import re

import history_cases as hc
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry points that take a handle and are no call of the matrix, each with its reason
EXEMPT = {
    "mdrp_destroy": "ends the handle: every test of tests/test_gpu_history.py closes its handles through it",
    "mdrp_synchronize": "waits for the handle's stream and computes nothing; the back-to-back test ends with it",
    "mdrp_last_stats": "reads host-side counters of the last call; superseded by mdrp_last_stats_sized, which every run() reads its statistics through",
    "mdrp_last_stats_sized": "reads host-side counters of the last call: the matrix reads them behind the calls, they are no result",
    "mdrp_last_sweep_stats": "reads host-side timing of the last call",
}


def handle_entry_points():
    """names of the functions declared in include/mdrp.h with an `mdrp_handle *` parameter (mdrp_create_'s `mdrp_handle **out` is none)"""
    src = open(os.path.join(ROOT, "include", "mdrp.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = "\n".join(line for line in src.splitlines() if not line.lstrip().startswith("#"))
    decls = re.findall(r"\b(mdrp_\w+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S)
    return sorted({name for name, args in decls if re.search(r"\bmdrp_handle\s*\*\s*\w", args)})


def test_the_header_is_parsed():
    names = handle_entry_points()
    assert len(names) >= 37 and "mdrp_create_" not in names and "mdrp_version" not in names
    for known in ("mdrp_estimate_batch", "mdrp_estimate_image_pairs_ranked_async", "mdrp_replay_slots", "mdrp_copy_budget_results_device", "mdrp_destroy"):
        assert known in names


def test_every_entry_point_with_a_handle_is_in_the_table():
    named = {p for c in hc.predecessors() for p in c.entry_points}
    declared = set(handle_entry_points())
    assert set(EXEMPT) <= declared, sorted(set(EXEMPT) - declared)
    assert not (named & set(EXEMPT)), sorted(named & set(EXEMPT))
    assert named <= declared, sorted(named - declared)
    missing = sorted(declared - named - set(EXEMPT))
    assert not missing, f"no call of tests/history_cases.py goes through {missing}: add one (or an exemption with its reason)"
    probed = {p for c in hc.probes() for p in c.entry_points}
    assert probed == named, sorted(named - probed)  # every one of them is checked, not only left behind


def test_the_probes_cover_the_shapes_and_families():
    est = hc.estimator_probes()
    assert {p.batch for p in est} >= {1, 5, 24} and {p.n_max for p in est} == {40, 130, 300}
    assert {(p.max_iterations, p.min_iterations) for p in est} >= {(64, 64), (300, 300), (300, 20)}
    assert {(p.kind, p.shift, p.device) for p in est} == {(k, s, d) for k, s in ((0, False), (0, True), (1, False), (2, False), (3, False), (4, False), (5, False))
                                                          for d in (False, True)}
    assert {p.want_mask for p in est} == {True, False} and sum(p.score_initial for p in est) == 1
    for p in est:
        n = p.data()["n"]
        assert n.max() == p.n_max and (p.batch < 5 or ((n == 0).any() and ((n > 0) & (n < 3)).any() and (n % 16 != 0).any())), p
    assert {p.family for p in hc.probes()} == {"estimate", "budgets", "prior", "ranked", "refine", "front_end", "unit"}
    names = {c.name for c in hc.predecessors()}
    assert len(names) == len(hc.predecessors())
    nan_priors = [p for p in hc.probes() if p.family == "prior"]
    assert nan_priors and all((p.data()["models"]["q"][:, 0] != p.data()["models"]["q"][:, 0]).any() for p in nan_priors)


def test_every_estimator_probe_has_the_predecessors_that_could_hurt_it():
    preds = [c for c in hc.predecessors() if None not in c.shapes()]
    for p in hc.estimator_probes():
        others = [c for c in preds if c is not p]
        s = p.shapes()
        larger = [c for c in others if all(a >= b for a, b in zip(c.shapes(), s)) and c.shapes() != s]
        # smaller: in no dimension above the probe and in at least one strictly below it (a probe of one pair has no predecessor of fewer)
        smaller = [c for c in others if all(a <= b for a, b in zip(c.shapes(), s)) and c.shapes() != s and c.family in ("estimate", "budgets", "prior", "ranked")]
        twins = [c for c in others if c.twin_of == p.name]
        other_kind = [c for c in others if c.shapes() == s and c.min_iterations == p.min_iterations and c.kind != p.kind]
        assert larger and smaller and other_kind, (p, larger, smaller, other_kind)
        assert len(twins) == 1, (p, twins)
        t = twins[0]
        assert (t.kind, t.shift, t.shapes(), t.min_iterations) == (p.kind, p.shift, s, p.min_iterations) and (t.data()["n"] == p.data()["n"]).all(), p
        # the hard probe's planted inlier ratio is below its clean twin's, which has no outlier at all
        assert p.data()["inlier_ratio"] <= 0.31 and t.data()["inlier_ratio"] == 1.0, (p, p.data()["inlier_ratio"], t.data()["inlier_ratio"])
        assert p.data()["inlier_ratio"] < t.data()["inlier_ratio"]


def test_every_entry_builds_the_same_inputs_twice():
    for c in hc.predecessors():
        a, b = (helpers.input_digest(hc.four(c.digest_arrays(c.make()))) for _ in range(2))
        assert a == b, c
        assert helpers.input_digest(hc.four(c.digest_arrays(c.data()))) == a, c  # (and the copy the GPU test runs on is that build)


def test_the_knob_predecessors_and_the_refusals():
    extra = {c.name: c for c in hc.extra_predecessors()}
    assert [extra["knobs_" + t].env for t in ("chunks", "unfused", "two_pairs_per_pass")] == [{"MDRP_CHUNKS": "64,256"}, {"MDRP_FUSE_TAIL": "0"}, {"MDRP_PAIRS_PER_PASS": "2"}]
    assert extra["fused_tail_gives_up"].env == {"MDRP_FUSE_GATE_US": "1", "MDRP_FUSE_WAIT_US": "1"}  # (MDRP_FUSE_TAIL stays unset: the handle's own choice)
    assert all(c.env is None for c in hc.probes()) and all(set(c.env) <= set(hc.KNOBS) for c in extra.values() if c.env)
    assert extra["beyond_the_lm_mask_index"].n_max == 5500 and extra["beyond_the_lm_list"].n_max == 8200 and [c.shapes() for c in extra.values() if c.name.startswith("larger_")] == [(40, 700, 600)] * 3
    assert sum(c.family == "refusal" for c in extra.values()) >= 9
    seen = {}
    hc.apply_env({"MDRP_CHUNKS": "7"}, seen.__setitem__, lambda k, raising=False: seen.pop(k, None))
    assert seen == {"MDRP_CHUNKS": "7"}
    assert hc.first_difference(b"abc", b"abc") is None and hc.first_difference(b"abc", b"abd") == 2 and hc.first_difference(b"ab", b"abc") == 2
