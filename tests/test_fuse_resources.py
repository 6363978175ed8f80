"""Register / spill / LDS budget of the consistency filter's kernels (mdrp_amd/csrc/mdrp_fuse.h), read from the built library's code
objects (no GPU), as tests/test_covis_resources.py does for the co-visibility kernels: every kernel is in the library once, has no spill and no
scratch, holds no LDS beyond the tile helpers' word per wavefront, and its row in profiles/fuse_kernel_table.txt is what the build produced.  The
register counts are written down as built, not chosen in advance: nobody has measured which count serves the multi-view gather best."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("mdrp::k_fuse_views", "mdrp::k_fuse_count", "mdrp::k_fuse_emit")
COLUMNS = ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch", "lds", "waves_per_simd")
TILE_LDS = 16  # recon_tile_total / recon_tile_rank: one word per wavefront of a 256-thread workgroup


@pytest.fixture(scope="module")
def regs():
    from mdrp_amd import build
    import kernel_table
    build.build()
    return kernel_table.kernel_table()


def _named(regs, name):
    return [k for k in regs if k == name or k.startswith(name + "(")]


@pytest.mark.parametrize("name", KERNELS)
def test_no_spill_no_scratch_and_no_lds_of_its_own(regs, name):
    found = _named(regs, name)
    assert len(found) == 1, (name, sorted(k for k in regs if "fuse" in k))
    r = regs[found[0]]
    print(found[0], r)
    assert r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0 and r.get("scratch", 0) == 0, (name, r)
    assert r.get("lds", 0) == (0 if name == "mdrp::k_fuse_views" else TILE_LDS), (name, r)
    assert r.get("agpr", 0) == 0


def test_no_other_fuse_kernel_is_built(regs):
    assert sorted(k.split("(")[0] for k in regs if "k_fuse" in k) == sorted(KERNELS)


def test_the_committed_table_is_what_the_build_produced(regs):
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "fuse_kernel_table.txt")).read().splitlines()[1:] if line.strip()]
    assert sorted(r[0] for r in rows) == sorted(KERNELS)
    for row in rows:
        found = _named(regs, row[0])
        assert len(found) == 1, row[0]
        assert [regs[found[0]].get(c, 0) for c in COLUMNS] == [int(v) for v in row[1:]], (row, regs[found[0]])
