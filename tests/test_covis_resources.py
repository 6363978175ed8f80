"""Register / spill / LDS budget of the co-visibility kernels (mdrp_amd/csrc/mdrp_covis.h), read from the built library's code objects
(no GPU), as tests/test_scene_resources.py does for the scene kernels: every kernel is in the library once, has no spill and no scratch, holds at
most 2 KiB of LDS and stands in profiles/covis_kernel_table.txt; k_covis_count runs at 8 wavefronts per SIMD as its k_recon_* siblings do.  The
kernels of the two-view and scene back ends, whose walk it shares, keep the rows of their committed tables."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("mdrp::k_covis_pair", "mdrp::k_covis_count")
COLUMNS = ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch", "lds", "waves_per_simd")


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
    assert len(found) == 1, (name, sorted(k for k in regs if "covis" in k))
    r = regs[found[0]]
    print(found[0], r)
    assert r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (name, r)
    assert r["lds"] <= 2048, (name, r)
    if name == "mdrp::k_covis_count":
        assert r["waves_per_simd"] == 8, (name, r)  # a memory-bound kernel: nothing but the register file should limit the wavefronts in flight
    else:
        print("k_covis_pair: wavefronts per SIMD (recorded, not gated):", r["waves_per_simd"])


def test_no_other_covis_kernel_is_built(regs):
    assert sorted(k.split("(")[0] for k in regs if "k_covis" in k) == sorted(KERNELS)


def test_the_kernels_are_in_the_committed_table():
    table = open(os.path.join(ROOT, "profiles", "covis_kernel_table.txt")).read()
    for name in KERNELS:
        assert name in table, name


@pytest.mark.parametrize("table, stem", [("recon_kernel_table.txt", "k_recon"), ("scene_kernel_table.txt", "k_scene")])
def test_the_shared_walks_kernels_keep_their_committed_rows(regs, table, stem):
    """recon_view and recon_lane are shared with k_covis_count: the kernels that had them first are built as they were"""
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", table)).read().splitlines()[1:] if line.strip()]
    assert len(rows) >= 3 and sorted(r[0] for r in rows) == sorted(k.split("(")[0] for k in regs if stem in k)
    for row in rows:
        found = _named(regs, row[0])
        assert len(found) == 1, row[0]
        assert [regs[found[0]].get(c, 0) for c in COLUMNS] == [int(v) for v in row[1:]], (row, regs[found[0]])
