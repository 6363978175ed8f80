"""Register / spill / LDS budget of the dense front end's kernels (mdrp_amd/csrc/mdrp_dense.h), read from the built library's code
objects (no GPU), as tests/test_prosac_resources.py does for the ranked estimator: every kernel is in the library once, has no spill and no
scratch, its static LDS is within a CU's 160 KiB, and k_dense_balance's is the 8^4 histogram plus its small tables."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("mdrp::k_dense_weights", "mdrp::k_dense_scan", "mdrp::k_dense_pick", "mdrp::k_dense_balance", "mdrp::k_dense_rank", "mdrp::k_dense_emit")


@pytest.fixture(scope="module")
def regs():
    from mdrp_amd import build
    import kernel_table
    build.build()
    return kernel_table.kernel_table()


def _named(regs, name):
    return [k for k in regs if k == name or k.startswith(name + "(")]


@pytest.mark.parametrize("name", KERNELS)
def test_no_spill_no_scratch_and_lds_within_a_cu(regs, name):
    found = _named(regs, name)
    assert len(found) == 1, (name, sorted(k for k in regs if "dense" in k))
    r = regs[found[0]]
    print(found[0], r)
    assert r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (name, r)
    assert r["lds"] <= 160 * 1024, (name, r)


def test_no_other_dense_kernel_is_built(regs):
    assert sorted(k.split("(")[0] for k in regs if "k_dense" in k) == sorted(KERNELS)


def test_the_histogram_is_what_the_lds_figure_says(regs):
    """grid = 8: 8^4 cells of 4 bytes; beside them 257 tile offsets of 4 bytes and the sixteen wavefronts' two tables (8 and 4 bytes an entry),
    each array aligned to its element or to 16 bytes: at most 48 bytes of padding"""
    lds = regs[_named(regs, "mdrp::k_dense_balance")[0]]["lds"]
    small = 257 * 4 + 16 * 8 + 16 * 4
    assert 8 ** 4 * 4 + small <= lds <= 8 ** 4 * 4 + small + 48, lds
    assert regs[_named(regs, "mdrp::k_dense_rank")[0]]["lds"] == 2048 * 8  # RANK_TILE keys of 8 bytes, as k_rank
    table = open(os.path.join(ROOT, "profiles", "dense_kernel_table.txt")).read()
    for name in KERNELS:
        assert name in table, name
