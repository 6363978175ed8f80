"""Register / spill / LDS budget of k_score_split (the split exact sweep), read from the built library's code objects (no GPU), as
tests/test_kernel_resources.py does for the other sweeps: three instantiations, no spill, no scratch, four wavefronts per SIMD, and static LDS that
lets four 256-thread workgroups share a CU (160 KiB)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def regs():
    from mdrp_amd import build
    import kernel_table
    build.build()
    return kernel_table.kernel_table()


def test_split_sweep_is_built_once_per_model_kind(regs):
    assert sorted(k for k in regs if k.startswith("mdrp::k_score_split<")) == \
        ["mdrp::k_score_split<false, false>", "mdrp::k_score_split<false, true>", "mdrp::k_score_split<true, false>"]


def test_split_sweep_does_not_spill_and_keeps_four_workgroups_per_cu(regs):
    for k, r in regs.items():
        if k.startswith("mdrp::k_score_split<"):
            assert r.get("vgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (k, r)
            assert r["vgpr"] <= 128 and r.get("agpr", 0) == 0 and r["waves_per_simd"] >= 4, (k, r)
            assert 4 * r["lds"] <= 160 * 1024, (k, r)
