"""Register / spill / LDS budget of the back end's kernels (mdrp_amd/csrc/mdrp_reconstruct.h), read from the built library's code objects
(no GPU), as tests/test_dense_resources.py does for the dense front end: every kernel is in the library once, has no spill and no scratch, its static
LDS is the few words its wavefronts exchange, and it stands in profiles/recon_kernel_table.txt."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("mdrp::k_recon_count", "mdrp::k_recon_scan", "mdrp::k_recon_emit")


@pytest.fixture(scope="module")
def regs():
    from mdrp_amd import build
    import kernel_table
    build.build()
    return kernel_table.kernel_table()


def _named(regs, name):
    return [k for k in regs if k == name or k.startswith(name + "(")]


@pytest.mark.parametrize("name", KERNELS)
def test_no_spill_no_scratch_and_small_lds(regs, name):
    found = _named(regs, name)
    assert len(found) == 1, (name, sorted(k for k in regs if "recon" in k))
    r = regs[found[0]]
    print(found[0], r)
    assert r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (name, r)
    assert r["lds"] <= 1024, (name, r)  # four wavefront counts (16 bytes), or the scan's 256 run totals of 4 bytes
    assert r["waves_per_simd"] == 8, (name, r)  # memory-bound kernels: nothing but the register file should limit the wavefronts in flight


def test_no_other_recon_kernel_is_built(regs):
    assert sorted(k.split("(")[0] for k in regs if "k_recon" in k) == sorted(KERNELS)


def test_the_kernels_are_in_the_committed_table():
    table = open(os.path.join(ROOT, "profiles", "recon_kernel_table.txt")).read()
    for name in KERNELS:
        assert name in table, name
