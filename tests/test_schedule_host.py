"""The host scheduler's decisions without a GPU: the rules of mdrp_amd/csrc/mdrp_schedule.h (host build, tests/hostmath/schedule_host.cpp) against
the values the scheduler has always computed — leading chunks per estimator, the MDRP_CHUNKS parser, the cut of a super-chunk into chunks, chunk
capacity, sample-table grouping, pairs per pass, lanes per LM problem and the fused tail's waits — and the header's place in the build."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mdrp_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_schedule.h")
SO = os.path.join(HERE, "hostmath", "libschedule_host.so")
CALIB, SHARED, VARYING, FIVE, SIX, SEVEN = range(6)  # include/mdrp.h
U64 = C.c_uint64
GIB, MIB = 1 << 30, 1 << 20


@pytest.fixture(scope="module")
def sh():
    src = os.path.join(HERE, "hostmath", "schedule_host.cpp")
    deps = [src, HDR, os.path.join(ROOT, "include", "mdrp.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", src, "-o", SO])
    lib = C.CDLL(SO)
    lib.sh_certain.restype = U64
    lib.sh_certain.argtypes = [U64, U64]
    lib.sh_chunk_capacity.argtypes = [U64, U64]
    lib.sh_parse_chunks.argtypes = [C.c_char_p, C.POINTER(U64)]
    lib.sh_default_lead.argtypes = [C.c_int, U64, C.c_double, C.POINTER(U64)]
    lib.sh_lead_budget.restype = U64
    lib.sh_layout.argtypes = [U64, U64, C.c_int, C.POINTER(U64), C.c_int, U64, U64, C.POINTER(U64), C.POINTER(C.c_int), C.POINTER(U64)]
    lib.sh_pairs_per_pass.argtypes = [U64, U64, C.c_int]
    return lib


def _lead(sh, kind, certain, seen_wish=-1.0):
    out = (U64 * sh.sh_nc_max())()
    return list(out[:sh.sh_default_lead(kind, certain, seen_wish, out)])


def _parse(sh, spec):
    out = (U64 * sh.sh_nc_max())()
    n = sh.sh_parse_chunks(None if spec is None else spec.encode(), out)
    return None if n < 0 else list(out[:n])


def _layout(sh, it0, certain, cap, lead, max_needed=0, max_it=None):
    nc = sh.sh_nc_max()
    lens, offs, total = (U64 * nc)(), (C.c_int * nc)(), U64()
    n = sh.sh_layout(it0, certain, cap, (U64 * max(len(lead), 1))(*lead), len(lead), max_needed, certain if max_it is None else max_it, lens, offs, C.byref(total))
    lens, offs = list(lens[:n]), list(offs[:n])
    assert offs == [sum(lens[:c]) for c in range(n)] and total.value == sum(lens)  # offsets are the prefix sums of the lengths
    return lens


def test_sample_sizes_model_slots_and_chunk_limit(sh):
    assert sh.sh_nc_max() == 8
    assert [sh.sh_sample_size(k) for k in range(6)] == [3, 3, 3, 5, 6, 7]
    assert [sh.sh_model_slots(k) for k in range(6)] == [4, 4, 4, 12, 16, 4]


@pytest.mark.parametrize("kind, certain, seen_wish, expected", [
    (SEVEN, 10000, -1.0, [128, 1024]), (SEVEN, 1, -1.0, [128, 1024]), (SIX, 10000, -1.0, [128]), (SIX, 1001, -1.0, [128]),
    (FIVE, 10000, -1.0, [512]), (FIVE, 1001, -1.0, [128]), (FIVE, 4096, -1.0, [256]),
    (CALIB, 10000, -1.0, [256]), (CALIB, 3000, -1.0, [128]), (CALIB, 1001, -1.0, [128]),
    (CALIB, 10000, 700.0, [704]), (CALIB, 10000, 90.0, [128]), (CALIB, 10000, 2000.0, [1024]),
    (CALIB, 8191, 700.0, [256]),  # the predictor is off below 8192 certain iterations
])
def test_leading_chunks_when_mdrp_chunks_is_not_set(sh, kind, certain, seen_wish, expected):
    assert _lead(sh, kind, certain, seen_wish) == expected
    if kind == CALIB:  # the three monodepth estimators share the rule
        assert _lead(sh, SHARED, certain, seen_wish) == expected and _lead(sh, VARYING, certain, seen_wish) == expected
    else:              # ... and the predictor is theirs alone
        assert _lead(sh, kind, certain, 700.0) == expected


def test_pass_budget_covers_the_longest_default_first_chunk_of_the_5_point_estimator(sh):
    assert sh.sh_lead_budget() == 512
    assert max(_lead(sh, FIVE, c)[0] for c in (1, 1001, 4096, 8192, 10000, 16384, 10 ** 6, 2 ** 40)) == sh.sh_lead_budget()


def test_mdrp_chunks_parser(sh):
    assert _parse(sh, "128,1024") == [128, 1024]
    assert _parse(sh, "0,x,256") == [256]                 # positive entries only
    assert _parse(sh, "") == []                           # set and empty: the first super-chunk is one chunk
    assert _layout(sh, 0, 10000, 10000, _parse(sh, "")) == [10000]
    assert _parse(sh, "1,2,3,4,5,6,7,8,9") == [1, 2, 3, 4, 5, 6, 7]  # NC_MAX - 1
    assert _parse(sh, None) is None                       # not set


@pytest.mark.parametrize("span, lead, chunks", [
    (10000, [256], [256, 9744]), (10000, [128, 1024], [128, 1024, 8848]),
    (512, [256], [256, 256]), (511, [256], [511]), (300, [128, 1024], [128, 172]),
])
def test_first_super_chunk_layout(sh, span, lead, chunks):
    assert _layout(sh, 0, span, span, lead) == chunks


def test_chunk_capacity_and_later_super_chunks(sh):
    # the default options: max 100000 / min 1000
    assert sh.sh_certain(100000, 1000) == 1001 and sh.sh_chunk_capacity(100000, 1000) == 4096
    assert _layout(sh, 0, 1001, 4096, [128], max_it=100000) == [128, 873]
    assert _layout(sh, 1001, 1001, 4096, [128], max_needed=100, max_it=100000) == [256]
    assert _layout(sh, 1001, 1001, 4096, [128], max_needed=50000, max_it=100000) == [4096]
    assert _layout(sh, 99900, 1001, 4096, [128], max_needed=50000, max_it=100000) == [100]
    # a certain range longer than the capacity
    assert sh.sh_certain(100000, 20000) == 20001 and sh.sh_chunk_capacity(100000, 20000) == 16384
    for lead0 in (128, 256, 1024):
        assert _layout(sh, 0, 20001, 16384, [lead0], max_it=100000) == [lead0, 16384 - lead0]
    assert _layout(sh, 16384, 20001, 16384, [256], max_it=100000) == [3617]  # no leading chunk behind the run's start
    assert sh.sh_certain(0, 1000) == 1 and sh.sh_chunk_capacity(0, 1000) == 1
    # the benchmark's fixed 10^4 iterations
    assert sh.sh_certain(10000, 10000) == 10000 and sh.sh_chunk_capacity(10000, 10000) == 10000


def test_sample_tables_are_numbered_by_first_appearance(sh):
    def group(n):
        n = np.asarray(n, dtype=np.int32)
        of, tn = np.zeros(len(n), dtype=np.int32), np.zeros(len(n), dtype=np.int32)
        k = sh.sh_group_tables(n.ctypes.data_as(C.c_void_p), len(n), of.ctypes.data_as(C.c_void_p), tn.ctypes.data_as(C.c_void_p))
        return of.tolist(), tn[:k].tolist()
    assert group([5, 9, 5, 7, 9]) == ([0, 1, 0, 2, 1], [5, 9, 7])
    assert group([2000] * 6) == ([0] * 6, [2000])


def test_pairs_per_pass(sh):
    assert sh.sh_pairs_per_pass(8 * GIB, MIB, 100000) == 4096          # half of the free memory
    assert sh.sh_pairs_per_pass(8 * GIB, MIB, 100) == 100              # ... or the whole batch
    assert sh.sh_pairs_per_pass(400 * GIB, 4 * MIB, 100000) == 24576   # at most 96 GiB
    assert sh.sh_pairs_per_pass(400 * GIB, MIB, 100000) == 65535       # the pair index is a grid's y
    assert sh.sh_pairs_per_pass(MIB, 8 * MIB, 10) == 1                 # at least one


@pytest.mark.parametrize("batch, n_max, lo, final", [(127, 2000, 256, 256), (128, 2000, 64, 256), (128, 4096, 256, 256), (4096, 2000, 64, 64)])
def test_default_lanes_per_lm_problem(sh, batch, n_max, lo, final):
    assert (sh.sh_lo_lanes(batch, n_max), sh.sh_final_lanes(batch)) == (lo, final)


@pytest.mark.parametrize("batch, n_max, gate, wait", [(1024, 2000, 90960, 24096), (1024, 5000, 200000, 72288), (12500, 2000, 200000, 70000)])
def test_default_waits_of_the_fused_tail(sh, batch, n_max, gate, wait):
    assert 3 * 90960 > 200000  # (1024 pairs at N = 5000: the gate's wait is the cap)
    assert (sh.sh_fuse_gate_us(batch, n_max), sh.sh_fuse_wait_us(batch, n_max)) == (gate, wait)


def test_header_is_hashed_and_host_only():
    assert os.path.realpath(HDR) in [os.path.realpath(d) for d in build.DEPS]
    text = open(HDR).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S)).lower()
    assert "hip" not in code and "getenv" not in code
    host = open(os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_capi.hip")).read()
    assert '#include "mdrp_schedule.h"' in host and "sched::super_chunk_layout(" in host and "sched::default_lead(" in host
