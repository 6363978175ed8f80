"""What the solver of a run's second chunk waits for, without a GPU: sched::second_solver_after (mdrp_amd/csrc/mdrp_schedule.h, host build
tests/hostmath/solver_order_host.cpp) over every estimator, presampled or not, host or resident buffers, one to three chunks and the knob
MDRP_SOLVE_BEHIND_PREP — and that run_pass and the clear in front of k_prep are wired to it."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_schedule.h")
SO = os.path.join(HERE, "hostmath", "libsolver_order_host.so")
CALIB, SHARED, VARYING, FIVE, SIX, SEVEN = range(6)  # include/mdrp.h
NOT_SET = -1


@pytest.fixture(scope="module")
def so():
    src = os.path.join(HERE, "hostmath", "solver_order_host.cpp")
    deps = [src, HDR, os.path.join(ROOT, "include", "mdrp.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", src, "-o", SO])
    lib = C.CDLL(SO)
    lib.so_second_solver_behind_prep.argtypes = [C.c_int] * 5
    return lib


def expected(kind, presampled, host, n_chunks, knob):
    """the rule restated: resident inputs, a second chunk whose sample table was drawn ahead, any estimator but the 6-point one, knob not 0"""
    return int(knob != 0 and not host and presampled and n_chunks >= 2 and kind != SIX)


@pytest.mark.parametrize("kind", range(6))
def test_every_combination_of_one_estimator(so, kind):
    for presampled, host, n_chunks, knob in itertools.product((False, True), (False, True), (1, 2, 3), (NOT_SET, 0, 1)):
        got = so.so_second_solver_behind_prep(kind, presampled, host, n_chunks, knob)
        assert got == expected(kind, presampled, host, n_chunks, knob), (kind, presampled, host, n_chunks, knob)


def test_the_default_on_the_benchmark_shape_and_its_exceptions(so):
    for kind in (CALIB, SHARED, VARYING, FIVE, SEVEN):
        assert so.so_second_solver_behind_prep(kind, True, False, 2, NOT_SET) == 1
        assert so.so_second_solver_behind_prep(kind, True, False, 3, NOT_SET) == 1  # (the third chunk's wait is not this rule's)
    assert so.so_second_solver_behind_prep(SIX, True, False, 2, NOT_SET) == 0       # two 6-point solvers at once: two scratch areas
    assert so.so_second_solver_behind_prep(SIX, True, False, 2, 1) == 0             # ... which the knob cannot ask for either
    assert so.so_second_solver_behind_prep(CALIB, True, True, 2, NOT_SET) == 0      # the sliced host front issues that solver itself
    assert so.so_second_solver_behind_prep(CALIB, False, False, 2, NOT_SET) == 0    # not pipelined: the tables advance in chunk order
    assert so.so_second_solver_behind_prep(CALIB, True, False, 1, NOT_SET) == 0     # no second chunk
    assert so.so_second_solver_behind_prep(CALIB, True, False, 2, 0) == 0           # MDRP_SOLVE_BEHIND_PREP=0: the old order


def test_the_scheduler_asks_the_rule_and_keeps_the_later_chunks_wait():
    host = open(os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_capi.hip")).read()
    assert "sched::second_solver_after(" in host and 'env_int("MDRP_SOLVE_BEHIND_PREP", -1)' in host
    assert "c > 0 ? h->ev_scanned[c - 1]" in host  # the third and later chunks wait for the scan of the chunk whose lists they reuse
    assert 'env_int("MDRP_FRONT_CLEAR", 1)' in host and "k_clear" in host
