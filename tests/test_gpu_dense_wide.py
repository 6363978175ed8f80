"""The dense front end at real warp sizes on a real MI355X (include/mdrp_dense.h): poselib.sample_dense_torch against the NumPy
definition (mdrp_amd/frontend.py sample_dense_numpy) as BYTES where tests/test_gpu_dense.py's shapes cannot go: k_dense_scan with runs of two, three
and sixteen blocks per thread (nblk = 257, 513, 4096), every 64-bit quantity of the sampler beyond 2^32 (the weight sum T, bpre, P - bstart,
dense_position, dense_search on uint64), stage 1 at its limit (n = 16384, expansion 4: M1 = m1_max = 65536, ntile = 256, all 257 entries of s_toff,
64 chunks of k_dense_balance's weight loop, 16 chunks of the stage-2 draw), k_dense_rank over more than one RANK_TILE with gridDim.y = 16, and
rows = 2^22, the most the host accepts.

Inputs (tests/dense_cases.py WIDE_BATCHES): "wide", B = 2, R = 256 * 1024 + 17; "wide3", B = 1, R = 512 * 1024 + 1; "max", B = 1, R = 2^22; the planted
rows of make_pair's "mixed" kind come along.  tests/test_scan_runs_host.py asserts on the CPU that these inputs reach what is claimed here.  Stage 2's
running sum cannot pass about 2^32 (each of at most 4096 cells contributes at most 2^20): no case is hunted for it."""
import numpy as np
import pytest

import dense_cases as dc
from test_gpu_dense import F32, F64, _ids, _sample, assert_sample_equal

pytestmark = pytest.mark.gpu

N = dc.N_WIDE
_ON_BOTH = [(N, dict()), (N, dict(ranked=True)), (N, dict(balanced=False)), (200, dict()), (N, dict(min_count=1, grid=3))]
# (batch, n, arguments of dense_cases.reference beside the sampler's)
WIDE_VARIANTS = [(name, n, kw) for name in ("wide", "wide3") for n, kw in _ON_BOTH] + [
    ("wide", N, dict(warp_dtype=F64, cert_dtype=F64, depth_dtype=F64, coords="pixel")),
    ("max", N, dict(ranked=True)),                 # the slowest two: R = 2^22
    ("max", 200, dict(balanced=False)),
]


@pytest.mark.parametrize("variant", WIDE_VARIANTS, ids=_ids)
def test_sampler_equals_the_numpy_definition_as_bytes(variant):
    name, n, kw = variant
    assert_sample_equal(_sample(name, n, **kw), dc.reference(name, n, **kw), variant)


def test_a_wide_pair_does_not_depend_on_its_batch():
    """pair 1 of "wide" alone (B = 1) gives the bytes it gives behind pair 0: bpre, qpre, the tiles and the metas are carved per pair"""
    from mdrp_amd import poselib
    got = _sample("wide", N, centres=False)
    alone = poselib.sample_dense_torch(*dc.tensors(*[a[1:] for a in dc.as_seen(dc.batch("wide"))]), n=N)
    assert alone[4][0] == got[4][1] > 2048
    for a, g in zip(alone[:4] + alone[5:], got[:4] + got[5:]):
        assert a.cpu().numpy()[0].tobytes() == g.cpu().numpy()[1].tobytes()
    assert_sample_equal(got, dc.reference("wide", N, centres=False), "wide, no centres")
