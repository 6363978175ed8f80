"""Register / spill / LDS budget of the ranked estimator's kernels (mdrp_amd/csrc/mdrp_prosac.h), read from the built library's code objects (no GPU),
as tests/test_score_split_resources.py does for the split sweep: k_rank, the gather / scatter kernels and k_samples_prosac have no spill and no
scratch, and their static LDS is within a CU's 160 KiB."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("mdrp::k_rank", "mdrp::k_rank_gather", "mdrp::k_rank_scatter", "mdrp::k_samples_prosac")


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
    assert len(found) == 1, (name, sorted(k for k in regs if "rank" in k or "prosac" in k))
    r = regs[found[0]]
    print(found[0], r)
    assert r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (name, r)
    assert r["lds"] <= 160 * 1024, (name, r)


def test_the_ranking_tile_is_what_the_lds_figure_says(regs):
    assert regs[_named(regs, "mdrp::k_rank")[0]]["lds"] == 2048 * 8  # RANK_TILE keys of 8 bytes
