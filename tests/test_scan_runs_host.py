"""The wide cases without a GPU: what makes the inputs of tests/test_gpu_dense_wide.py and tests/test_gpu_backend_wide.py mean what they claim.

Every dense stage reduces its per-block counts with one chunked scan (k_dense_scan, k_recon_scan, k_scene_scan): a thread sums a run of
per = ceil(n / 256) consecutive values, thread 0 scans the 256 run totals, the thread walks its run again.  The wide cases are the smallest inputs with
per = 2 and per = 3, the largest the sampler accepts, weight sums beyond 2^32 and image sets of more than four workgroups of the per-image kernels.
A later change of a generator could move a case back to per = 1, or below 2^32, with every GPU test still green: the conditions are asserted here, on
the NumPy definition alone (mdrp_amd/frontend.py), from the constants the Python side mirrors (blocks and tiles of 1024, workgroups of 256)."""
import numpy as np
import pytest

import dense_cases as dc
import fuse_cases as fc
import reconstruct_cases as rc
import scene_cases as sc
from mdrp_amd import _capi, frontend

N = dc.N_WIDE


# ---- the dense sampler
@pytest.mark.parametrize("name, blocks, per", [("wide", 257, 2), ("wide3", 513, 3), ("max", 4096, 16)])
def test_dense_batches(name, blocks, per):
    R, seeds = dc.WIDE_BATCHES[name]
    b = dc.batch(name)
    assert b["warp"].shape == (len(seeds), R, 4) and dc.nblk(R) == blocks and dc.scan_run(blocks) == per
    assert dc.scan_run(dc.nblk(R - dc.BLOCK_ROWS)) < per or name == "max"  # the smallest row count of that run length (one block fewer: a shorter run)
    busy = -(-blocks // per)                                                # threads that hold a block
    assert (busy, blocks - (busy - 1) * per) == {"wide": (129, 1), "wide3": (171, 3), "max": (256, 16)}[name]  # ... and the last one's run
    assert R == frontend.DENSE_MAX_ROWS or name != "max"
    assert R % dc.BLOCK_ROWS == {"wide": 17, "wide3": 1, "max": 0}[name]    # the ragged last block
    balanced = dc.reference(name, N, ranked=True)                           # (the ranked records are the balanced ones in another order)
    unbalanced = dc.reference(name, N, balanced=False)
    for i in range(len(seeds)):
        q = dc.candidates(name, i)
        T, K = int(q.astype(np.uint64).sum()), int(np.count_nonzero(q))
        assert T > 2 ** 32, (name, i, T)                                    # DenseMeta::T, bpre, P - bstart and dense_position beyond 32 bits
        assert K >= frontend.DENSE_MAX_STAGE1                               # M1 = m1_max = 65536: ntile = 256, all 257 entries of s_toff
        rows = balanced[5][i][:balanced[4][i]]
        hit = len(np.unique(rows // dc.BLOCK_ROWS))
        assert hit >= blocks - (1 if name == "wide3" else 0), (name, i, hit)  # (wide3's last block is one row)
        assert balanced[4][i] > 2048                                        # k_dense_rank: more than one RANK_TILE
        assert unbalanced[4][i] < K                                         # the unbalanced draw is a draw, not every candidate
        # stage 2's running sum cannot pass about 2^32 - each of at most 8^4 = 4096 cells contributes at most count * ((1 << 20) div count) <= 2^20 -
        # so no case is hunted for it


def test_dense_wide_pairs_differ():
    b = dc.batch("wide")
    assert not np.array_equal(b["cert"][0], b["cert"][1]) and dc.reference("wide", N)[5][0].tobytes() != dc.reference("wide", N)[5][1].tobytes()


# ---- the two-view clouds
@pytest.mark.parametrize("size", rc.WIDE_SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_cloud_sizes(size):
    """A map of 409 x 643 has 262 987 pixels, of which the generator plants a twentieth as +inf or -inf: its kept count at rate 1 (about 249 800) cannot
    pass 2^18 = 262 144, and is held above 2^17 here; the 514-tile side's (about 499 000) is held above 2^18."""
    nt = [rc.tiles(*s) for s in size]
    assert sorted(nt) in ([33, 257], [257, 514])
    assert [rc.scan_run(n) for n in nt] == {(257, 33): [2, 1], (33, 257): [1, 2], (514, 257): [3, 2]}[tuple(nt)]
    for kind in rc.WIDE_KINDS:
        x = rc.inputs(kind, "float32", size)
        assert len(x["models"]) == rc.WIDE_B and all(frontend.recon_usable(m, kind) for m in x["models"])
        for b in range(rc.WIDE_B):
            for rate in rc.WIDE_RATES:
                sides = rc.rows(kind, "float32", size, "not_inf", rate, b)
                for s in range(2):
                    pixel = sides[s][1].astype(np.int64)
                    counts = np.bincount(pixel // rc.TILE, minlength=nt[s])
                    assert len(counts) == nt[s] and counts[-1] > 0, (kind, b, rate, s)       # a kept pixel in the last tile
                    if nt[s] > 256:
                        assert (counts[256:] != counts[255:-1]).any()                         # a tile beyond 256 differs from its neighbour
                        if rate == 1.0:
                            assert len(pixel) > (2 ** 18 if nt[s] == 514 else 2 ** 17), (kind, b, s, len(pixel))
        for rate in rc.WIDE_RATES:
            cut, total = rc.wide_p_max_cases(kind, "float32", size, "not_inf", rate)
            sides = rc.rows(kind, "float32", size, "not_inf", rate, 0)
            big = int(nt[1] > nt[0])
            first = (len(sides[0][1]) if big else 0) + int((sides[big][1] // rc.TILE < nt[big] - 1).sum())   # the first row of the big side's last tile
            assert first < cut < first + int((sides[big][1] // rc.TILE == nt[big] - 1).sum()) <= total      # the cut is inside that tile


# ---- the scenes
def test_wide_scene_shape():
    (H, W), sizes = fc.WIDE_SHAPES["wide"]
    assert rc.tiles(H, W) == 257 and rc.scan_run(257) == 2 and fc.TREES["mixed"]["I"] == 3
    assert [rc.tiles(*s) for s in sizes] == [257, 1, 189]                   # the full allocation | one tile | ends before the allocation's tiles
    for kind in fc.WIDE_KINDS:
        assert (fc.transforms(kind, "mixed")["depth"] == [0, 1, 2]).all()   # a chain
        for rate in fc.WIDE_RATES:
            rows = sc.wide_rows(kind, "float32", "wide", "not_inf", rate)
            assert (rows[0][1].astype(np.int64) // rc.TILE == 256).any() and len(rows[2][1]) > 0
            assert rows[1] is not None and len(rows[1][1]) == 0             # the one-pixel image is attached; its pixel is a planted inf
            cut, total = fc.wide_p_max_cases(rows, 0)
            in_last = int((rows[0][1].astype(np.int64) // rc.TILE == 256).sum())
            assert len(rows[0][1]) - in_last < cut < len(rows[0][1]) < total


def test_many_images():
    I = fc.MANY
    t = fc.WIDE_TREES["many"]
    assert I == 257 and rc.scan_run(I) == 2 and rc.scan_run(I - 1) == 1 and t["I"] == I and len(t["pairs"]) <= 255
    assert -(-I // 64) == 5                                                 # workgroups of k_scene_chain and k_fuse_views (64 lanes, one per image)
    (H, W), sizes = fc.WIDE_SHAPES["many"]
    assert (H, W) == (5, 7) and len(sizes) == I and len(set(sizes)) == 5
    role = np.array(t["tree"])[:, 1]
    for kind in fc.WIDE_KINDS:
        T = fc.transforms(kind, "many")
        attached, absent, detached = T["depth"] >= 0, role == _capi.SCENE_ABSENT, (T["depth"] < 0) & (role != _capi.SCENE_ABSENT)
        for g in range(1, 5):                                               # every later workgroup holds attached images; absent and detached ones at 64 and above
            assert attached[64 * g:64 * (g + 1)].any()
        assert absent[64:].any() and detached[64:].any() and absent[64:128].any() and detached[64:128].any() and absent[192:].any() and detached[192:].any()
        roots = np.unique(T["root"][attached])
        assert len(roots) >= 2 and (roots >= 64).any()
        for r in roots:
            assert (T["depth"][T["root"] == r] == 1).sum() >= 3 and T["depth"][T["root"] == r].max() >= 3   # a star, and chains below it
        assert T["depth"].max() <= 4                                        # ... of modest depth: the transforms stay near the identity
        for rate in fc.WIDE_RATES:
            rows = sc.wide_rows(kind, "float32", "many", "not_inf", rate)
            offsets = frontend.pack_scene_rows(rows)[2]
            assert offsets[I] > offsets[I - 1] > offsets[I - 2]             # strictly increasing beyond image 256's start
            assert rows[99] is not None and len(rows[99][1]) == 0           # an attached image without a row (a map of inf)
            cut, total = fc.wide_p_max_cases(rows, I - 1)
            assert offsets[I - 1] <= cut < total == offsets[I]
        support = np.concatenate([r[2] for r in fc.open_rows(kind, "float32", "many", "many", 8, 1.0, fc.WIDE_TOL) if r is not None])
        kept = frontend.fuse_gate(support, 1, 0)
        assert (support[:, 0] > 0).any() and (support[:, 1] > 0).any() and kept.any() and not kept.all()   # consistent, violating, kept and dropped points
    views = fc.views(I, 8)
    assert (views == -1).any() and (views == I).any()                       # the inert slots
    assert ((views > 255) & (views < I)).any(axis=1).sum() >= 4             # images whose view is image 256
