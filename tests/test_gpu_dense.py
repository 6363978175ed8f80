"""The dense front end on a real MI355X (include/mdrp_dense.h): poselib.sample_dense_torch against the NumPy definition
(mdrp_amd/frontend.py sample_dense_numpy) as BYTES - every quantity that decides a pick is an integer -, poselib.estimate_dense_torch against
estimate_batch_torch on the sampler's output, and every refusal through the raw symbols and through Python.

Inputs (tests/dense_cases.py): B = 3, maps of 45 x 61 and 39 x 70 pixels (non-square, different, no multiple of a grid), R = 3 blocks + 17 rows and
R = 300 (less than a block), a pair of zero certainties between two live ones, the same pair at two batch positions, rows on the maps' borders,
infinite and NaN depths, tied certainties, and the duplicate case (five rows of weight 65536 among thousands of weight 1 with M1 near K).  These
shapes keep k_dense_scan at one block per thread and every running sum below 2^32: the warps of a real matcher (257, 513 and 4096 blocks, weight
sums beyond 2^32, stage 1 at its limit) are tests/test_gpu_dense_wide.py's."""
import ctypes as C

import numpy as np
import pytest

import dense_cases as dc

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
K_DUP = 2770  # the duplicate pairs have 2777 and 2799 candidates (checked below)

# (batch, n, arguments of dense_cases.reference beside the sampler's)
VARIANTS = [
    ("blocks", 200, dict()),
    ("blocks", 200, dict(warp_dtype=F64, cert_dtype=F64, depth_dtype=F64)),
    ("blocks", 200, dict(warp_dtype=F64, cert_dtype=F32, depth_dtype=F64, coords="pixel")),
    ("blocks", 200, dict(warp_dtype=F32, cert_dtype=F64, coords="pixel", filter="finite")),
    ("blocks", 200, dict(filter="finite", centres=False)),
    ("blocks", 200, dict(balanced=False)),
    ("blocks", 257, dict(balanced=False, ranked=True)),
    ("blocks", 200, dict(ranked=True)),
    ("blocks", 200, dict(grid=1)),
    ("blocks", 200, dict(grid=3, min_count=1)),
    ("blocks", 200, dict(min_count=10 ** 6)),
    ("blocks", 64, dict(expansion=1, seed=2 ** 40 + 3)),
    ("blocks", 1100, dict(expansion=2, threshold=0.5)),
    ("small", 100, dict()),
    ("small", 1000, dict()),                       # n above the candidate count
    ("small", 1000, dict(balanced=False, ranked=True)),
    ("duplicates", K_DUP, dict(balanced=False)),   # M1 near K: the heavy rows are picked from hundreds of strata each
    ("duplicates", K_DUP, dict(expansion=1, ranked=True)),
]


def _ids(v):
    name, n, kw = v
    return f"{name}-{n}-" + ",".join(f"{k}={getattr(x, '__name__', x)}" for k, x in kw.items())


def _sample(name, n, centres=True, warp_dtype=F32, cert_dtype=F32, depth_dtype=F32, coords="normalized", **kw):
    from mdrp_amd import poselib
    b = dc.batch(name)
    t = dc.tensors(*dc.as_seen(b, warp_dtype, cert_dtype, depth_dtype, coords))
    return poselib.sample_dense_torch(*t, n=n, coords=coords, center1=b["c1"].copy() if centres else None, center2=b["c2"].copy() if centres else None, **kw)


def assert_sample_equal(got, ref, what):
    x1, x2, d1, d2, cnt, rows, score = got
    assert isinstance(cnt, np.ndarray) and cnt.dtype == np.int32 and np.array_equal(cnt, ref[4]), (what, cnt, ref[4])
    for name, mine, want in (("rows", rows, ref[5]), ("score", score, ref[6]), ("x1", x1, ref[0]), ("x2", x2, ref[1]), ("d1", d1, ref[2]), ("d2", d2, ref[3])):
        mine = mine.cpu().numpy()
        assert mine.dtype == want.dtype and mine.shape == want.shape, (what, name)
        assert mine.tobytes() == want.tobytes(), (what, name, [np.flatnonzero((mine[b] != want[b]).reshape(len(mine[b]), -1).any(axis=1))[:8] for b in range(len(mine))])


def test_the_inputs_hold_the_planted_cases():
    ref, fin = dc.reference("blocks", 200), dc.reference("blocks", 200, filter="finite")
    assert ref[4][1] == 0 and ref[4][0] == ref[4][2] > 100
    assert np.isinf(ref[2]).any() and np.isnan(ref[2]).any() and np.isfinite(fin[2]).all() and np.isfinite(fin[3]).all()  # one-sided infinities and NaN kept | dropped
    ranked = dc.reference("blocks", 200, ranked=True)
    assert (np.diff(ranked[6][0][:ranked[4][0]]) == 0).any()  # tied certainties among the records
    for i in (0, 1):
        q = dc.candidates("duplicates", i)
        assert K_DUP + 7 <= np.count_nonzero(q) <= K_DUP + 200 and 3 <= (q == 65536).sum() <= 5  # (a heavy row outside a map is no candidate)
    dup = dc.reference("duplicates", K_DUP, balanced=False)
    assert 5 <= dup[4][0] < 100 and dup[4][2] > 1000  # nearly every stratum of the duplicate pairs is a duplicate
    assert dc.reference("small", 1000)[4].max() < dc.R_SMALL
    q = dc.candidates("blocks", 0)
    warp = dc.as_seen(dc.batch("blocks"))[0][0]
    for v in (-1.0, np.nextafter(F32(1.0), F32(0.0))):  # rows exactly on the first pixel and inside the last one are candidates ...
        assert q[np.flatnonzero((warp == F32(v)).any(axis=1))].any(), v
    for v in (1.0, np.inf, -np.inf):  # ... the extent itself and beyond are not (just below -1 still truncates to pixel 0: rule 2)
        assert not q[np.flatnonzero((warp == F32(v)).any(axis=1))].any(), v


@pytest.mark.parametrize("variant", VARIANTS, ids=_ids)
def test_sampler_equals_the_numpy_definition_as_bytes(variant):
    name, n, kw = variant
    assert_sample_equal(_sample(name, n, **kw), dc.reference(name, n, **kw), variant)


def test_a_pair_does_not_depend_on_its_batch():
    """pair 0 = pair 2 of the batch give the same bytes; so does pair 0 alone (B = 1) and behind two other pairs"""
    from mdrp_amd import poselib
    got = _sample("blocks", 200, centres=False)
    for a in got[:4] + got[5:]:
        a = a.cpu().numpy()
        assert a[0].tobytes() == a[2].tobytes()
    warp, cert, dm1, dm2 = dc.as_seen(dc.batch("blocks"))
    alone = poselib.sample_dense_torch(*dc.tensors(warp[:1], cert[:1], dm1[:1], dm2[:1]), n=200)
    sm = dc.as_seen(dc.batch("duplicates"))
    order = [2, 1, 0]  # pair 0 of "blocks" last, behind pairs of the same shape
    mixed = poselib.sample_dense_torch(*dc.tensors(*[np.concatenate([s[1:], a[:1]]) for s, a in zip(sm, (warp, cert, dm1, dm2))]), n=200)
    assert order and alone[4][0] == mixed[4][2] == got[4][0]
    for a, m, g in zip(alone[:4] + alone[5:], mixed[:4] + mixed[5:], got[:4] + got[5:]):
        assert a.cpu().numpy()[0].tobytes() == m.cpu().numpy()[2].tobytes() == g.cpu().numpy()[0].tobytes()


def test_warp_as_an_image_and_inputs_on_a_side_stream():
    """(B, Hc, Wc, 4) is the same rows; inputs produced on a non-default current stream just before the call are seen (the call runs on that stream)"""
    import torch
    from mdrp_amd import poselib
    b = dc.batch("small")
    warp, cert, dm1, dm2 = dc.as_seen(b)
    ref = dc.reference("small", 100, centres=False)
    t = dc.tensors(warp.reshape(3, 15, 20, 4), cert.reshape(3, 15, 20), dm1, dm2)
    assert_sample_equal(poselib.sample_dense_torch(*t, n=100), ref, "image")
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        late = [torch.full_like(v, float("nan")) for v in t]
        for v, o in zip(t, late):
            torch.add(v, 0.0, out=o)
        assert_sample_equal(poselib.sample_dense_torch(*late, n=100), ref, "stream")
    torch.cuda.synchronize()


# ---- sampler + estimator
def _estimate_inputs(kind):
    b = dc.estimate_batch()
    t = dc.tensors(b["warp"].astype(F32), b["cert"].astype(F32), b["dm1"].astype(F32), b["dm2"].astype(F32))
    focal = kind != "calibrated"
    cams = (None, None) if focal else (dc.ECAM1, dc.ECAM2)
    centres = dict(center1=dc.EC1, center2=dc.EC2) if focal else {}
    return b, t, cams, centres


@pytest.mark.parametrize("ranked", [False, True])
@pytest.mark.parametrize("kind", ["calibrated", "shared_focal", "varying_focal"])
def test_estimate_from_the_warp_equals_estimate_on_the_sampled_records(kind, ranked):
    import torch
    from mdrp_amd import poselib, synth
    b, t, cams, centres = _estimate_inputs(kind)
    n = 500  # of 2200 rows, 1760 of them inliers: stage 1 keeps some 1700, stage 2's 500 strata fall on about 400 distinct rows
    x1, x2, d1, d2, cnt, rows, score = poselib.sample_dense_torch(*t, n=n, coords="pixel", ranked=ranked, **centres)
    assert (cnt >= 330).all() and (cnt <= 450).all(), cnt  # about 400 rows kept
    low = (score.cpu().numpy() < 0.25) & (rows.cpu().numpy() >= 0)
    assert low.sum(axis=1).max() <= 0.05 * n  # the outliers' certainties are low: few of them are drawn
    res_ref, mask_ref = poselib.estimate_batch_torch(kind, x1, x2, d1, d2, *cams, dc.ERO, dc.EBO, n_per_pair=cnt, scores="presorted" if ranked else None)
    res, mask, n_used, rows2 = poselib.estimate_dense_torch(kind, *t, *cams, dc.ERO, dc.EBO, n=n, coords="pixel", ranked=ranked, **centres)
    assert isinstance(n_used, np.ndarray) and n_used.dtype == np.int32 and np.array_equal(n_used, cnt)
    assert res.dtype == res_ref.dtype and res.tobytes() == res_ref.tobytes(), [k for k in range(len(res)) if res[k].tobytes() != res_ref[k].tobytes()]
    assert mask.dtype == torch.uint8 and mask.cpu().numpy().tobytes() == mask_ref.cpu().numpy().tobytes()
    assert rows2.cpu().numpy().tobytes() == rows.cpu().numpy().tobytes()
    assert (res["iterations"] == 200).all() and (res["num_inliers"] > 0).all()  # (the scene has two focals: the shared-focal estimator fits a part of it)
    if kind == "calibrated":  # noise-free: the pose is recovered
        assert (res["num_inliers"] >= 0.9 * cnt).all()
        for i, truth in enumerate(b["truth"]):
            R = poselib._quat_to_R(res[i]["model"]["q"])
            assert synth.rotation_error_deg(truth["R"], R) < 1e-3 and abs(res[i]["model"]["scale"] - truth["scale"]) < 1e-3 * truth["scale"], i
    if ranked:
        with_switch = poselib.estimate_dense_torch(kind, *t, *cams, dict(dc.ERO, progressive_sampling=True), dc.EBO, n=n, coords="pixel", ranked=True, **centres)
        assert with_switch[0].tobytes() == res.tobytes()


# ---- refusals
def _valid(h):
    b = dc.batch("small")
    return dc.sample_on(h, dc.tensors(*dc.as_seen(b)), 100)


def test_refusals_leave_the_handle_usable():
    import torch
    from mdrp_amd import _capi, poselib
    fresh_h = _capi.Handle(0)
    fresh = _valid(fresh_h)
    fresh_h.close()
    ref = dc.reference("small", 100, centres=False)
    assert fresh[4] == ref[5].tobytes() and fresh[6] == ref[4].tobytes()
    t = dc.tensors(*dc.as_seen(dc.batch("small")))
    h = _capi.Handle(0)
    lib = h._lib
    ro, bo = _capi.ransac_opt_from_dict(dc.ERO), _capi.bundle_opt_from_dict(dc.EBO)
    cams = poselib._camera_records(dc.ECAM1, 3)
    n = 100
    out = [torch.zeros((3, n, 2), dtype=torch.float64, device="cuda:0") for _ in range(2)] + [torch.zeros((3, n), dtype=torch.float64, device="cuda:0") for _ in range(3)]
    rows = torch.zeros((3, n), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    cnt = np.zeros(3, dtype=np.int32)
    ptrs = [C.c_void_p(o.data_ptr()) for o in (out[0], out[1], out[2], out[3])] + [C.c_void_p(rows.data_ptr()), C.c_void_p(out[4].data_ptr()), C.c_void_p(cnt.ctypes.data)]
    refused = 0

    def both(desc, batch=3):
        nonlocal refused
        d = C.byref(desc) if desc is not None else None
        assert lib.mdrp_sample_dense(h._h, d, batch, *ptrs) == 1 and lib.mdrp_last_error()
        assert lib.mdrp_estimate_dense_async(h._h, _capi.CALIB, d, batch, cams.ctypes.data_as(C.c_void_p), cams.ctypes.data_as(C.c_void_p), C.byref(ro), C.byref(bo), None, None) == 1
        assert _valid(h) == fresh  # the handle is usable and gives the fresh handle's bytes
        refused += 1

    desc, keep, B = dc.descriptor(t, n)
    assert lib.mdrp_sample_dense(None, C.byref(desc), 3, *ptrs) == 1  # a NULL handle
    assert lib.mdrp_estimate_dense_async(None, _capi.CALIB, C.byref(desc), 3, None, None, C.byref(ro), C.byref(bo), None, None) == 1
    both(None)                                                           # a NULL descriptor
    both(desc, batch=-1)
    for field, value in (("warp_type", 2), ("certainty_type", -1), ("depth_type", 5), ("coords", 2), ("coords", -1), ("filter", 2), ("rows", -1), ("rows", (1 << 22) + 1),
                         ("h1", -1), ("w2", -1), ("n", 0), ("n", 16385), ("expansion", 0), ("expansion", 656), ("grid", 0), ("grid", 9), ("min_count", 0),
                         ("warp", None), ("certainty", None), ("depth1", None), ("depth2", None)):
        was = getattr(desc, field)
        setattr(desc, field, value)
        both(desc)
        setattr(desc, field, was)
    assert refused == 23
    for i in range(len(ptrs)):                                           # a NULL output of the sampler
        assert lib.mdrp_sample_dense(h._h, C.byref(desc), 3, *[None if j == i else p for j, p in enumerate(ptrs)]) == 1
    for kind in (3, 4, 5, -1):                                           # a kind outside 0 .. 2
        assert lib.mdrp_estimate_dense_async(h._h, kind, C.byref(desc), 3, cams.ctypes.data_as(C.c_void_p), cams.ctypes.data_as(C.c_void_p), C.byref(ro), C.byref(bo), None, None) == 1
    for r, b_ in ((None, bo), (ro, None)):                               # NULL options
        assert lib.mdrp_estimate_dense_async(h._h, 0, C.byref(desc), 3, cams.ctypes.data_as(C.c_void_p), cams.ctypes.data_as(C.c_void_p),
                                             None if r is None else C.byref(r), None if b_ is None else C.byref(b_), None, None) == 1
    assert lib.mdrp_estimate_dense_async(h._h, 0, C.byref(desc), 3, None, None, C.byref(ro), C.byref(bo), None, None) != 0  # the estimator's own: no cameras
    prog = _capi.ransac_opt_from_dict(dict(dc.ERO, progressive_sampling=True))  # unranked: progressive_sampling is refused as on every unranked entry point
    assert lib.mdrp_estimate_dense_async(h._h, 0, C.byref(desc), 3, cams.ctypes.data_as(C.c_void_p), cams.ctypes.data_as(C.c_void_p), C.byref(prog), C.byref(bo), None, None) not in (0, 1)
    assert _valid(h) == fresh
    h.close()
    # through Python
    for bad in (dict(n=0), dict(n=16385), dict(expansion=0), dict(n=16384, expansion=5), dict(grid=0), dict(grid=9), dict(min_count=0), dict(coords="pixels"),
                dict(filter="nonsense")):
        with pytest.raises(ValueError):
            poselib.sample_dense_torch(*t, **{"n": 100, **bad})
        with pytest.raises(ValueError):
            poselib.estimate_dense_torch("calibrated", *t, dc.ECAM1, dc.ECAM2, dc.ERO, dc.EBO, **{"n": 100, **bad})
    for bad in ((t[0].half(), t[1], t[2], t[3]), (t[0], t[1].cpu(), t[2], t[3]), (t[0], t[1], t[2], t[3].double()), (t[0][..., :3], t[1], t[2], t[3]),
                (t[0], t[1][:, :50], t[2], t[3]), (t[0], t[1], t[2][0], t[3]), (t[0], t[1], t[2][:2], t[3])):
        with pytest.raises(ValueError):
            poselib.sample_dense_torch(*bad, n=100)
    for kind in (_capi.RELPOSE_5PT, _capi.FUNDAMENTAL_7PT, "fundamental"):
        with pytest.raises(ValueError):
            poselib.estimate_dense_torch(kind, *t, dc.ECAM1, dc.ECAM2, dc.ERO, dc.EBO, n=100)
    with pytest.raises(NotImplementedError):
        poselib.estimate_dense_torch("calibrated", *t, dc.ECAM1, dc.ECAM2, dict(dc.ERO, progressive_sampling=True), dc.EBO, n=100)
    assert_sample_equal(poselib.sample_dense_torch(*t, n=100), ref, "after the refusals")
