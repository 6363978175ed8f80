"""Register / spill / LDS budget of the scene kernels (mdrp_amd/csrc/mdrp_scene.h), read from the built library's code objects (no GPU),
as tests/test_reconstruct_resources.py does for the two-view back end: every kernel is in the library once, has no spill and no scratch, and stands
in profiles/scene_kernel_table.txt; the count, scan and emit kernels run at 8 wavefronts per SIMD as their k_recon_* counterparts do.  k_scene_chain
walks a tree with one lane per image and holds two edges and an accumulated transform in registers: its occupancy is recorded, not gated."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PIXEL_KERNELS = ("mdrp::k_scene_count", "mdrp::k_scene_scan", "mdrp::k_scene_emit")
KERNELS = ("mdrp::k_scene_chain",) + PIXEL_KERNELS


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
    assert len(found) == 1, (name, sorted(k for k in regs if "scene" in k))
    r = regs[found[0]]
    print(found[0], r)
    assert r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (name, r)
    assert r["lds"] <= 2048, (name, r)  # four wavefront counts (16 bytes), or the scan's 256 run totals of 8 bytes (the scene's rows are int64)
    if name in PIXEL_KERNELS:
        assert r["waves_per_simd"] == 8, (name, r)  # memory-bound kernels: nothing but the register file should limit the wavefronts in flight
    else:
        print("k_scene_chain: wavefronts per SIMD (recorded, not gated):", r["waves_per_simd"])


def test_no_other_scene_kernel_is_built_and_none_is_a_recon_kernel(regs):
    assert sorted(k.split("(")[0] for k in regs if "k_scene" in k) == sorted(KERNELS)
    assert not [k for k in regs if "k_scene" in k and "k_recon" in k]


def test_the_kernels_are_in_the_committed_table():
    table = open(os.path.join(ROOT, "profiles", "scene_kernel_table.txt")).read()
    for name in KERNELS:
        assert name in table, name
