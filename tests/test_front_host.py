"""The first chunk's front without a GPU (host build: tests/hostmath/front_host.cpp): the LDS reservation that caps the solver's residency
(sched::solver_reservation, mdrp_schedule.h), when the stage is on (sched::first_pick), and the prefix-record retirement predicate of k_first_filter
(prefix_bar / RecordBar::retires, mdrp_front.h) against the sequential loop it must never contradict."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mdrp_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "mdrp_amd", "csrc")
SO = os.path.join(HERE, "hostmath", "libfront_host.so")
DBL_MAX = np.finfo(np.float64).max
KB = 1024
GRANULE = 2560  # sched::LDS_GRANULE: a multiple of both LDS allocation granularities (512 B, 1280 B)


@pytest.fixture(scope="module")
def fh():
    src = os.path.join(HERE, "hostmath", "front_host.cpp")
    deps = [src, os.path.join(ROOT, "include", "mdrp.h")] + [os.path.join(CSRC, f) for f in ("mdrp_front.h", "mdrp_schedule.h", "mdrp_math.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", src, "-o", SO])
    lib = C.CDLL(SO)
    lib.fh_solver_reservation.restype = C.c_uint64
    lib.fh_solver_reservation.argtypes = [C.c_uint64, C.c_int, C.c_uint64]
    lib.fh_retires.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int]
    lib.fh_bar_retires.argtypes = [C.c_longlong, C.c_double, C.c_int, C.c_double, C.c_int]
    return lib


@pytest.mark.parametrize("lds", [64 * KB, 160 * KB])
def test_reservation_fits_exactly_four_workgroups_per_resident_wavefront(fh, lds):
    assert fh.fh_solver_reservation(lds, 0, 0) == 0 and fh.fh_solver_reservation(lds, -1, 0) == 0      # R = 0: uncapped
    for r in (1, 2, 3):
        b = fh.fh_solver_reservation(lds, r, 0)
        assert b > 0 and b % 512 == 0 and b % 1280 == 0                                                 # whole allocation granules, either size
        assert 4 * r * b <= lds < (4 * r + 1) * b, (lds, r, b)                                          # 4 R fit, one more does not
    assert fh.fh_solver_reservation(160 * KB, 2, 0) == 20 * KB and fh.fh_solver_reservation(64 * KB, 1, 0) == 15 * KB


@pytest.mark.parametrize("lds", [64 * KB, 160 * KB])
def test_reservation_keeps_lds_free_or_answers_uncapped(fh, lds):
    for r in (1, 2, 3):
        limit = lds // (4 * r + 1)              # a cap through LDS takes 4 R / (4 R + 1) of it at least: no more than this can stay free
        sure = limit - 4 * r * GRANULE - 1       # ... and rounding down to whole granules costs at most one per workgroup
        for keep in (0, 1 * KB, max(sure, 0), limit - 1, limit, limit + 1, lds // 2, lds - 1, lds, lds + 1, 4 * lds):
            b = fh.fh_solver_reservation(lds, r, keep)
            if b:
                assert 4 * r * b + keep <= lds < (4 * r + 1) * b, (lds, r, keep, b)
            else:
                assert keep > sure, (lds, r, keep)
            if keep >= limit:
                assert b == 0, (lds, r, keep, b)
    # the front's sweep workgroups hold 32 - 39 KiB: two of them cannot be kept free beside a capped solver on either size
    assert fh.fh_solver_reservation(lds, 2, 2 * 38928) == 0 and fh.fh_solver_reservation(lds, 1, 2 * 38928) == 0


def test_stage_is_on_for_three_point_estimators_in_calls_above_the_wave_limit(fh):
    assert [fh.fh_first_pick(k, 1024, 128, -1) for k in range(6)] == [48, 48, 48, 0, 0, 0]
    assert fh.fh_first_pick(0, 128, 128, -1) == 0 and fh.fh_first_pick(0, 129, 128, -1) == 48
    assert fh.fh_first_pick(0, 1024, 128, 0) == 0 and fh.fh_first_pick(0, 1024, 128, 32) == 32 and fh.fh_first_pick(0, 1024, 128, 1000) == 64
    assert fh.fh_first_pick(0, 64, 128, 32) == 0


def test_key_bounds_the_candidate_count(fh):
    for n in (3, 40, 257, 600, 2000, 70001):
        for cand in sorted({0, 1, 2, n // 3, n // 2, n - 1, n}):
            key = min(64, -(-cand * 64 // n))  # k_count: min(PROBE_PTS, ceil(cand * PROBE_PTS / n))
            assert cand <= fh.fh_cand_of_key(key, n) <= min(n, cand + n // 64 + 1), (n, cand, key)


def _tables(rng, trial):
    """(n, thr, iteration, cand, count, score) of a chunk's hypotheses in solver order: up to four models per iteration, candidate counts at or
    above the inlier counts, scores at or above thr (n - count), with planted exact ties of count, score and bound"""
    n = int(rng.choice([3, 40, 257, 600]))
    thr = float(rng.choice([1.0, 0.25, 3.7e-6]))
    iters = np.repeat(np.arange(40), rng.integers(0, 5, 40))           # same-iteration models, empty iterations
    m = len(iters)
    good = rng.random(m) < (0.05, 0.3, 0.9)[trial % 3]
    count = np.where(good, rng.integers(n // 2, n + 1, m), rng.integers(0, max(n // 8, 1) + 1, m))
    cand = np.minimum(n, count + np.where(rng.random(m) < 0.3, 0, rng.integers(0, max(n // 16, 1) + 1, m)))
    score = thr * (n - count) + np.where(rng.random(m) < 0.2, 0.0, rng.random(m) * thr * count)
    for _ in range(m // 4):                                            # exact ties: a later hypothesis repeats an earlier one's count and score,
        a, b = sorted(rng.integers(0, m, 2))                           # and its candidate bound meets them exactly
        count[b], score[b], cand[b] = count[a], score[a], max(cand[b], count[a])
        if rng.random() < 0.5:
            cand[b] = count[a]
    return n, thr, iters.astype(np.int32), cand.astype(np.int32), count.astype(np.int32), score.astype(np.float64)


def _sequential_records(iters, count, score):
    """the loop k_scan reproduces: a hypothesis is a record when it has more inliers or a lower score than everything before it"""
    run_cnt, run_score, rec = 0, DBL_MAX, np.zeros(len(iters), dtype=bool)
    for i in range(len(iters)):
        if count[i] > run_cnt or score[i] < run_score:
            rec[i] = True
            run_cnt, run_score = max(run_cnt, int(count[i])), min(run_score, float(score[i]))
    return rec


def test_filter_never_retires_a_record_and_is_the_stated_test(fh):
    rng = np.random.default_rng(20260)
    retired_total = records_total = kept_nonrecords = 0
    for trial in range(300):
        n, thr, iters, cand, count, score = _tables(rng, trial)
        m = len(iters)
        if m == 0:
            continue
        rec = _sequential_records(iters, count, score)
        picked = np.zeros(m, dtype=bool)
        picked[np.argsort(-cand, kind="stable")[:int(rng.integers(0, 9))]] = True
        picked[0] = True                                               # the chunk's earliest hypothesis
        pc = count[picked].copy()
        if trial % 5 == 0 and pc.size > 1:
            pc[1] = -2                                                 # a picked hypothesis the sweep's own bail-out retired: it sets no record
        pi, ps = np.ascontiguousarray(iters[picked]), np.ascontiguousarray(score[picked])
        for i in np.flatnonzero(~picked):
            got = fh.fh_retires(pi.ctypes.data, pc.ctypes.data, ps.ctypes.data, len(pi), int(iters[i]), n, thr, int(cand[i]))
            before = (pi < iters[i]) & (pc >= 0)                       # strictly earlier iterations only
            rc = int(pc[before].max()) if before.any() else -1
            rs = float(ps[before].min()) * (1.0 + 1e-12) if before.any() else DBL_MAX
            want = cand[i] <= rc and thr * float(n - cand[i]) >= rs
            assert bool(got) == bool(want), (trial, i)
            assert not (got and rec[i]), (trial, i, "a record was retired")
            retired_total += got
            records_total += rec[i]
            kept_nonrecords += (not got) and (not rec[i])
    assert retired_total > 2000 and records_total > 100 and kept_nonrecords > 100  # all three outcomes are exercised


def test_same_iteration_models_and_exact_ties_stay(fh):
    pi, pc, ps = np.array([5], np.int32), np.array([100], np.int32), np.array([60.0])
    args = (pi.ctypes.data, pc.ctypes.data, ps.ctypes.data, 1)
    n, thr = 200, 0.5
    assert fh.fh_retires(*args, 6, n, thr, 50) == 1                    # 50 <= 100 and 0.5 * 150 = 75 >= 60 (1 + 1e-12)
    assert fh.fh_retires(*args, 5, n, thr, 50) == 0                    # the same iteration is no bar
    assert fh.fh_retires(*args, 4, n, thr, 50) == 0                    # nor a later one
    assert fh.fh_retires(*args, 6, n, thr, 100) == 0                   # 0.5 * 100 = 50 < 60: it might score lower
    assert fh.fh_retires(*args, 6, n, thr, 101) == 0                   # it might have more inliers
    assert fh.fh_retires(*args, 6, n, thr, 80) == 0                    # the score bound ties the record exactly: inflated by 1e-12, it stays
    assert fh.fh_retires(*args, 6, n, thr, 79) == 1
    assert fh.fh_bar_retires(100, 60.0, n, thr, 50) == 1 and fh.fh_bar_retires(100, DBL_MAX, n, thr, 0) == 0  # no record yet: nothing retires
    assert fh.fh_bar_retires(100, 60.0, n, thr, 80) == 0 and fh.fh_bar_retires(100, 60.0, n, thr, 79) == 1


def test_headers_are_hashed_and_the_kernels_use_the_shared_predicate():
    deps = [os.path.realpath(d) for d in build.DEPS]
    assert os.path.realpath(os.path.join(CSRC, "mdrp_front.h")) in deps and os.path.realpath(os.path.join(CSRC, "mdrp_schedule.h")) in deps
    kern = open(os.path.join(CSRC, "mdrp_kernels.h")).read()
    code = re.sub(r"//[^\n]*", "", kern)
    assert "struct Bar : RecordBar" in code and code.count(".retires(") == 2 and "prefix_bar(" in code  # k_count and k_first_filter, one test
    host = open(os.path.join(CSRC, "mdrp_capi.hip")).read()
    assert "sched::solver_reservation(" in host and "sched::first_pick(" in host
