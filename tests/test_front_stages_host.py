"""The cases and references of tests/test_gpu_front_stages.py, checked without a GPU: the cases hold what they claim, the sampler restatement is the
oracle's, the header and the binding agree, and — the condition the GPU test stands on — the share of iterations on which the references themselves
disagree (the oracle's solver against the host build of the device's) stays under 1 % of the live iterations of every case.

Measured here (oracle against host build, g++ -O2, on the records as the definitions give them; live iterations of the five active pairs of a batch
under its longest chunk list, n_max = 300 / 291):
  p3p 0 of 2885 / 0 of 2885    shift 0 / 0    shared 0 / 0    varying 0 / 0    5-point 3 / 2    7-point 0 / 0    (6-point: no host build, 1000 iterations)
  P3P: 580 / 578 iterations hold the NaN model, 577 of them in the pair of three records that never has a real pose"""
import numpy as np
import pytest

import front_stages_cases as fc
import front_stages_ref as fr
from oracle import pyorc as po

IDS = [f"{fc.kind_id(k, s)}-{n}" for k, s in fc.KINDS for n in (fc.N_MAX, fc.N_MAX_ODD)]
PARAMS = [(k, s, n) for k, s in fc.KINDS for n in (fc.N_MAX, fc.N_MAX_ODD)]


def test_draw_is_the_oracles_sampler_for_three():
    for n, seed in ((3, 0), (7, 5), (37, fc.SEED), (257, fc.SEED), (300, fc.SEED), (2000, 0)):
        assert np.array_equal(fr.draw_table(seed, n, 3, 200), po.draw_samples(seed, n, 200)), (n, seed)


def test_sampler_restatement_meets_the_golden_tables(golden):
    g = golden("sampler")
    for key in g.files:
        n, seed = (int(v[1:]) for v in key.split("_"))
        assert np.array_equal(fr.draw_table(seed, n, 3, len(g[key])), g[key]), key


def test_bf16_restatement():
    """known patterns: exact values, ties to even, the NaN rule, and a split that reproduces its input to 2^-16"""
    x = np.array([1.0, -2.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, np.inf, np.nan, 0.0], dtype=np.float32)
    assert fr.bf16_bits(x).tolist() == [0x3F80, 0xC000, 0x3F80, 0x3F82, 0x7F80, 0x7FC0, 0x0000]
    v = np.random.default_rng(3).normal(size=1000) * 10.0 ** np.random.default_rng(4).integers(-6, 7, 1000)
    h, l = fr.bf16_split(v)
    back = fr.bf16_value(h).astype(np.float64) + fr.bf16_value(l).astype(np.float64)
    assert np.abs(back - v).max() <= np.abs(v).max() * 2.0 ** -16 and (np.abs(back - v) <= np.abs(v) * 2.0 ** -15).all()
    blk, written = fr.fragments(np.array([[1.0, 2.0, 3.0, 4.0]] * 17), 17, 40)
    assert blk.shape == (3, 64, 4) and written[:2].all() and not written[2].any() and not blk[1, 1:16].any() and not blk[2].any()
    assert blk[0, 48].tolist() == [0x3F803F80, 0x00003F80, 0, 0] and np.array_equal(blk[0, 0], blk[0, 32]) and np.array_equal(blk[0, 0], blk[1, 0])
    assert blk[0, 0].tolist() == [0x40C04040, 0x40804040, 0x40804100, 0x40003F80]  # (3, 6 | 3, 4 | 8, 4 | 1, 2), the even one in the low half


def test_the_cases_hold_what_they_claim():
    for kind, shift in fc.KINDS:
        K = fr.SAMPLE_SIZE[kind]
        for n_max in (fc.N_MAX, fc.N_MAX_ODD):
            d = fc.batch(kind, shift, n_max)
            n = d["n"].tolist()
            assert n == [n_max, n_max, 257, 37, K, K - 1] and n_max >= 257 and n_max % 16 != 0  # (the fragments' pair stride is ceil(n_max / 16) groups)
            assert 257 == 256 + 1 and 37 % 16 != 0 and d["x1"].shape == (6, n_max, 2)
            if kind in (0, 3):  # both camera models, fx != fy, parameters of their own per pair
                for c in (d["cam1"], d["cam2"]):
                    assert set(c["model_id"].tolist()) == {0, 1} and len({tuple(p) for p in c["params"].tolist()}) == 6
                    assert all(p[0] != p[1] for m, p in zip(c["model_id"], c["params"]) if m == 1)
            if kind == 4:
                assert d["cam2"] is None and len({tuple(p[:2]) for p in d["cam1"]["params"].tolist()}) == 6
        for chunks in fc.chunk_lists(kind):
            assert sum(chunks) <= (201 if kind == 4 else 577)
        longest = fc.chunk_lists(kind)[-1]
        assert longest[0] % 64 == 1 and len(longest) == 3 and (kind == 4 or (longest[1] % 256 == 255 and longest[2] % 256 == 1))
    c = fc.corrupted_batch()
    clean = fc.corrupted_batch(False)
    assert np.isnan(c["x2"][1]).sum() == 1 and np.isinf(c["x1"][2]).sum() == 1 and (c["x1"][3] == 1e16).sum() == 2 and (c["x2"][3] == 1e16).sum() == 1
    assert np.array_equal(c["x1"][0], clean["x1"][0]) and np.isfinite(clean["x1"]).all() and np.isfinite(clean["x2"]).all()
    pts, _ = fc.host_prep(0, c)
    for pair, rows in fc.CORRUPT_ZERO_ROWS.items():
        bad = np.nonzero(fr.unusable_rows(pts[pair, :fc.CORRUPT_N, :4]))[0].tolist()
        assert bad == list(rows), (pair, bad)
    assert not fr.unusable_rows(pts[0, :fc.CORRUPT_N, :4]).any()


@pytest.mark.parametrize("kind,shift,n_max", PARAMS, ids=IDS)
def test_the_references_agree_on_the_cases(kind, shift, n_max):
    """the share of live iterations on which the oracle's solver and the host build of the device's differ (count, or beyond the tolerance) is at most
    1 % — of the longest chunk list, which holds the iterations of the shorter ones (one sample sequence per table).  P3P: at least a handful of
    iterations in front of a wavefront's first real pose are ones the reference's P3P answers with NaN poses."""
    d = fc.batch(kind, shift, n_max)
    K = fr.SAMPLE_SIZE[kind]
    chunks = fc.chunk_lists(kind)[-1]
    pts, dep = fc.host_prep(kind, d)
    live = unjudged = nan_front = nan_then_pose = 0
    for p, n in enumerate(d["n"]):
        if n < K:
            continue
        refs = fc.pair_references(kind, shift, pts[p], dep[p] if kind <= 2 else None, fr.draw_table(fc.SEED, int(n), K, sum(chunks)))
        live += len(refs)
        unjudged += sum(not r[2] for r in refs)
        if (kind, shift) == (0, False):
            front = fc.nan_front([len(r[0]) for r in refs], [r[3] for r in refs], chunks)
            nan_front += len(front)
            nan_then_pose += len(front) if any(len(r[0]) for r in refs) else 0
    print(f"{fc.kind_id(kind, shift)} n_max {n_max}: {unjudged} of {live} live iterations unjudged" + (f", {nan_front} NaN iterations" if nan_front else ""))
    assert live == 5 * sum(chunks) and unjudged <= fc.UNJUDGED_CAP * live, (unjudged, live)
    if (kind, shift) == (0, False):
        assert nan_front >= 5 and nan_then_pose >= 1, (nan_front, nan_then_pose)  # (... and not only in the pair that never has a real pose)


def test_header_and_binding_agree(tmp_path):
    """mdrp_front_stages is a new symbol within ABI 6; the two structs of include/mdrp.h have the binding's sizes and field offsets (a C compiler checks)"""
    import ctypes as C
    import os
    import subprocess
    from mdrp_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dt = _capi.FRONT_STATE_DTYPE
    lines = ['#include <stddef.h>', '#include "mdrp.h"', f"_Static_assert(sizeof(mdrp_front_state) == {dt.itemsize}, \"state\");",
             f"_Static_assert(sizeof(mdrp_front_run) == {C.sizeof(_capi.FrontRun)}, \"run\");", f"_Static_assert(MDRP_FRONT_FILL == {_capi.FRONT_FILL}, \"fill\");"]
    lines += [f"_Static_assert(offsetof(mdrp_front_state, {f}) == {dt.fields[f][1]}, \"{f}\");" for f in dt.names]
    lines += [f"_Static_assert(offsetof(mdrp_front_run, {f}) == {getattr(_capi.FrontRun, f).offset}, \"{f}\");" for f, _ in _capi.FrontRun._fields_]
    lines += ["typedef int (*stages_t)(mdrp_handle *, const mdrp_ransac_opt *, const mdrp_bundle_opt *, mdrp_front_run *);", "stages_t a = mdrp_front_stages;"]
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", str(src), "-I", os.path.join(root, "include"), "-o", str(tmp_path / "abi.o")], check=True)
    assert "mdrp_front_stages" in _capi.EXPORTS and _capi.ABI_VERSION == 6
    assert _capi.SAMPLE_SIZE == fr.SAMPLE_SIZE and _capi.MODEL_SLOTS == fr.MODEL_SLOTS
