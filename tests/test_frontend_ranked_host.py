"""The front end with match scores without a GPU: the NumPy definition (mdrp_amd/frontend.py, scores=) against its parts — the
unranked gather, then the ranking of tests/prosac_ref.py on the kept rows' scores, then the permutation —, the ranking key of
mdrp_amd/csrc/mdrp_prosac.h (host build) against the NumPy order, the binding against the header, and the resources of the new kernels in
the built library.

frontend.score_order states the same rule as prosac_ref.order in the same words, so the first test checks the COMPOSITION (which rows are kept,
that only their scores rank, the slot mapping, the permutation), not the ordering rule; the ordering rule's independent witness is the key test,
which compares the C++ key of every pair of values with plain floating-point comparisons."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import frontend_ranked_cases as rc
import image_pairs_cases as ipc
import prosac_ref
from mdrp_amd import _capi, frontend

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "hostmath", "librank_key_host.so")
NEW = ("mdrp_gather_matches_ranked", "mdrp_estimate_matches_ranked_async", "mdrp_gather_image_pairs_ranked", "mdrp_estimate_image_pairs_ranked_async")


def _from_parts(unranked, scores):
    """(x1, x2, d1, d2, slot) of one pair from the unranked gather: prosac_ref.order on the kept rows' scores in gathered order, then the permutation"""
    x1, x2, d1, d2, slot = unranked
    kept = np.flatnonzero(slot >= 0)
    assert np.array_equal(slot[kept], np.arange(len(kept)))  # gathered order is match order
    o = prosac_ref.order(np.asarray(scores)[kept])
    ranked = np.full(len(slot), -1, dtype=np.int32)
    ranked[kept[o]] = np.arange(len(kept), dtype=np.int32)
    return x1[o], x2[o], d1[o], d2[o], ranked


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k)


@pytest.mark.parametrize("score_dtype", [np.float32, np.float64])
def test_definition_equals_gather_then_rank_then_permute(score_dtype):
    seen = set()
    for which, batch in enumerate(rc.batches()):
        kept = rc.kept_rows(batch)
        for offset in range(len(rc.PATTERNS)):
            scores = rc.batch_scores(kept, offset, which).astype(score_dtype)
            filter, centres = ("both_inf", "finite")[offset % 2], bool(offset & 2)
            for b in range(len(scores)):
                args = (batch["kp1"][b].astype(np.float32), batch["kp2"][b].astype(np.float32), batch["matches"][b], batch["dm1"][b].astype(np.float32),
                        batch["dm2"][b], batch["c1"][b] if centres else None, batch["c2"][b] if centres else None, filter)
                plain = frontend.gather_matches_numpy(*args)
                _same(frontend.gather_matches_numpy(*args, scores=None), plain, "scores=None")
                got = frontend.gather_matches_numpy(*args, scores=scores[b])
                _same(got, _from_parts(plain, scores[b]), (which, offset, b))
                n = len(plain[2])
                assert len(got[2]) == n and sorted(got[4][got[4] >= 0].tolist()) == list(range(n))  # n and the kept set do not depend on the scores
                assert np.array_equal(got[4] >= 0, plain[4] >= 0)
                seen.add((rc.PATTERNS[(b + offset) % len(rc.PATTERNS)], min(n, 3)))
    assert {p for p, _ in seen} == set(rc.PATTERNS) and {k for _, k in seen} == {0, 1, 2, 3}  # every pattern; pairs that keep 0, 1, 2 and more rows


def test_the_planted_scores_are_what_the_cases_promise():
    a, b, c = rc.batches()
    kept = rc.kept_rows(a)
    s = rc.batch_scores(kept, 0, 0)  # pair 5 (600 rows): PATTERNS[5]; with offset 5 it gets "dropped_high" ((5 + 5) % 7 == 3), with 4 "special"
    hi = rc.batch_scores(kept, 5, 0)[5]
    assert (~kept[5]).sum() >= 20 and np.nanmin(hi[~kept[5]]) > hi[kept[5]].max() and np.isnan(hi[~kept[5]]).any() and np.isinf(hi[~kept[5]]).any()
    m = a["matches"][5]
    gone = np.flatnonzero(~kept[5][:600])
    assert ((m[gone] < 0).any(axis=1)).sum() >= 5 and (m[gone, 0] >= len(a["kp1"][5]) - 1).any()  # padding in mid-list, an index past the table
    assert kept[5][gone.min() + 1:gone.max()].any()  # dropped rows are interleaved with kept ones
    sp = rc.batch_scores(kept, 4, 0)[5]
    k5 = sp[kept[5]]
    assert np.isnan(k5).sum() >= 3 and (k5 == np.inf).any() and (k5 == -np.inf).any() and (np.signbit(k5) & (k5 == 0)).any() and (~np.signbit(k5) & (k5 == 0)).any()
    assert len({np.signbit(v) for v in k5[np.isnan(k5)]}) == 2  # NaN of both signs
    lv = rc.batch_scores(kept, 3, 0)[5]
    assert len(np.unique(lv)) == 4
    assert s.dtype == np.float64 and np.array_equal(s, s.astype(np.float32).astype(np.float64), equal_nan=True)
    n = [int(v.sum()) for v in rc.kept_rows(b)] + [int(v.sum()) for v in rc.kept_rows(c)]
    assert n[3:6] == [0, 2, 3] and n[7] == 1


@pytest.mark.parametrize("score_dtype", [np.float32, np.float64])
def test_image_pairs_definition_is_the_per_pair_definition(score_dtype):
    t = ipc.batch()
    B, M = t["matches"].shape[:2]
    plain = ipc.twin(centres=True)
    kept = plain[5] >= 0
    scores = rc.batch_scores(kept, 2, 9).astype(score_dtype)
    kp, dm = t["keypoints"].astype(np.float32), t["depth_maps"].astype(np.float32)
    kw = dict(centers=t["centers"], sizes=t["sizes"], kp_counts=t["kp_counts"])
    _same(frontend.gather_image_pairs_numpy(kp, dm, t["pairs"], t["matches"], scores=None, **kw), plain, "scores=None")
    got = frontend.gather_image_pairs_numpy(kp, dm, t["pairs"], t["matches"], scores=scores, **kw)
    per_pair = []
    for b in range(B):
        n = plain[4][b]
        per_pair.append(_from_parts((plain[0][b, :n], plain[1][b, :n], plain[2][b, :n], plain[3][b, :n], plain[5][b]), scores[b]))
    _same(got, frontend.pad_pairs(per_pair, M), "image pairs")
    assert np.array_equal(got[4], plain[4]) and all(got[4][b] == 0 and (got[5][b] == -1).all() for b in ipc.BAD)
    with pytest.raises(ValueError):
        frontend.gather_image_pairs_numpy(kp, dm, t["pairs"], t["matches"], scores=scores[:, :-1], **kw)
    with pytest.raises(ValueError):
        frontend.gather_image_pairs_numpy(kp, dm, t["pairs"], t["matches"], scores=scores.astype(np.float16), **kw)


# ---- the ranking key
@pytest.fixture(scope="module")
def rk():
    src = os.path.join(HERE, "hostmath", "rank_key_host.cpp")
    hdr = os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_prosac.h")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", src, "-o", SO])
    lib = C.CDLL(SO)
    lib.rk_key_dropped.restype = C.c_uint64
    return lib


def _keys(rk, s):
    s = np.ascontiguousarray(s)
    key = np.zeros(len(s), dtype=np.uint64)
    (rk.rk_keys_f32 if s.dtype == np.float32 else rk.rk_keys_f64)(s.ctypes.data_as(C.c_void_p), len(s), key.ctypes.data_as(C.c_void_p))
    return key


def _numpy_key(s):
    key = np.array(s, dtype=np.float64)
    key[np.isnan(key)] = -np.inf
    return key + 0.0


def _special_values():
    bits = np.array(list(rc.NANS) + [0x7fffffffffffffff, 0xffffffffffffffff, 0x7ff0000000000001, 0xfff0000000000001], dtype=np.uint64)
    dmax, tiny = np.finfo(np.float64).max, 5e-324
    return np.concatenate([bits.view(np.float64), [np.inf, -np.inf, 0.0, -0.0, tiny, -tiny, 2.2250738585072014e-308, -2.2250738585072014e-308,
                                                    2.225073858507201e-308, dmax, -dmax, 1.0, -1.0, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0)]])


def test_key_orders_like_the_numpy_definition(rk):
    rng = np.random.default_rng(3)
    special = _special_values()
    s = np.concatenate([special, special, rng.normal(size=300), rng.normal(size=100) * 1e300, rng.normal(size=100) * 1e-310, rng.integers(-3, 4, 100) / 2.0])
    s = s[rng.permutation(len(s))]
    key, ref = _keys(rk, s), _numpy_key(s)
    assert np.isnan(s).sum() >= 18 and (np.abs(s[np.isfinite(s)]) < 2.3e-308).sum() > 50  # NaNs and denormals took part
    # every pair of values: the keys compare as the definition's keys do
    assert np.array_equal(key[:, None] > key[None, :], ref[:, None] > ref[None, :])
    assert np.array_equal(key[:, None] == key[None, :], ref[:, None] == ref[None, :])
    # and the stable descending order by key is the definition's order
    by_key = np.argsort(np.iinfo(np.uint64).max - key, kind="stable")
    assert np.array_equal(by_key, frontend.score_order(s)) and np.array_equal(by_key, prosac_ref.order(s))
    # NaN of either sign and any payload is -inf; the zeros are one key; the key of a dropped row is below the smallest key there is
    lowest = _keys(rk, np.array([-np.inf]))[0]
    assert lowest == 0x000fffffffffffff == key.min() and (key[np.isnan(s)] == lowest).all()
    assert _keys(rk, np.array([0.0]))[0] == _keys(rk, np.array([-0.0]))[0] == 0x8000000000000000
    assert rk.rk_key_dropped() == 0 < lowest


def test_float_scores_give_the_keys_of_their_double_values(rk):
    rng = np.random.default_rng(4)
    nan32 = np.array([0x7fc00000, 0xffc00000, 0x7fc00001, 0xffa00000, 0x7f800001], dtype=np.uint32).view(np.float32)
    fmax, ftiny = np.finfo(np.float32).max, np.float32(1e-45)
    s = np.concatenate([nan32, np.array([np.inf, -np.inf, 0.0, -0.0, ftiny, -ftiny, fmax, -fmax, 1.17549435e-38, -1.17549421e-38], dtype=np.float32),
                        rng.normal(size=500).astype(np.float32), (rng.normal(size=100) * 1e-40).astype(np.float32)]).astype(np.float32)
    with np.errstate(invalid="ignore"):
        wide = s.astype(np.float64)
    assert np.array_equal(_keys(rk, s), _keys(rk, wide))
    assert np.array_equal(np.argsort(np.iinfo(np.uint64).max - _keys(rk, s), kind="stable"), frontend.score_order(s))


# ---- binding
def test_new_symbols_are_declared_and_bound_within_abi_6():
    hdr = open(os.path.join(ROOT, "include", "mdrp.h")).read()
    assert int(re.search(r"#define MDRP_ABI_VERSION (0x[0-9a-fA-F]+)", hdr).group(1), 16) == _capi.ABI_VERSION == 0x00000006
    declared = set(re.findall(r"\b(mdrp_[a-z_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _capi.EXPORTS, name
    for method in ("gather_matches_ranked", "estimate_matches_ranked_device", "gather_image_pairs_ranked", "estimate_image_pairs_ranked_device"):
        assert callable(getattr(_capi.Handle, method))
    assert (_capi.F32, _capi.F64) == (0, 1)


# ---- resources
@pytest.fixture(scope="module")
def regs():
    from mdrp_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    build.build()
    return kernel_table.kernel_table()


def test_library_exports_the_new_symbols(regs):
    syms = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\bT {name}\b", syms), name


@pytest.mark.parametrize("family", ["k_gather_ranked", "k_gather_images_ranked"])
def test_ranked_gather_kernels_are_built_without_scratch_or_spills(regs, family):
    want = [f"mdrp::{family}<{k}, {d}>" for k in ("float", "double") for d in ("float", "double")]
    found = sorted(k for k in regs if k.startswith(f"mdrp::{family}<"))
    assert found == sorted(want), found  # exactly four: the score type is a runtime switch, not a template parameter
    for name in want:
        r = regs[name]
        print(name, r)
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (name, r)
        assert r["lds"] == 2048 * 8 + 16, (name, r)  # the key tile of k_rank (RANK_TILE keys of 8 bytes) and the four wavefront counts


def test_the_existing_kernels_did_not_move(regs):
    assert sum(1 for k in regs if k.startswith("mdrp::k_gather<")) == 4 and sum(1 for k in regs if k.startswith("mdrp::k_gather_images<")) == 4
    r = regs["mdrp::k_rank"]  # as built before the counting loop was shared with the ranked front end
    assert (r["vgpr"], r["sgpr"], r["lds"], r.get("agpr", 0)) == (36, 55, 2048 * 8, 0), r
    assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, r
