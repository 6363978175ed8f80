"""The consistency filter of a scene without a GPU (include/mdrp_fuse.h): the NumPy definition (mdrp_amd/frontend.py fuse_scene_numpy,
rules F1-F6) pinned by its own properties - the open gate is the scene's cloud, a gated cloud is the open one's rows that pass, the subset rule of the
subsample, an image's independence of the other rows of `views`, every inert kind of slot, V = 0, a rendered three-view scene whose every support
pair is predicted by integer geometry - scene_views, the Python layer's refusals, header, binding and build against each other, and the header's
host arithmetic (tests/hostmath/fuse_host.cpp, a stand-alone program) against the definition as bytes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fuse_cases as fc
from mdrp_amd import _capi, frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mdrp_fuse_scene_async",)
ALL = frontend.RECON_ALL


def _definition(kind, dt, shape, tree, V, rate, tol, gate, p_max=None, view_table=None, keep="not_inf"):
    x = fc.inputs(kind, dt, shape, tree)
    lo, hi = frontend.covis_band(tol)
    return frontend.fuse_scene_numpy(x["models"], kind, x["dm"], x["pairs"], x["tree"], fc.views(x["I"], V) if view_table is None else view_table, p_max, x["centers"],
                                     x["sizes"], x["cams"], keep, frontend.recon_threshold(rate), fc.SEED, lo, hi, gate[0], gate[1])


# ---- the definition's own properties
@pytest.mark.parametrize("kind", fc.KINDS)
def test_the_open_gate_is_the_scenes_cloud_and_support_labels_every_point(kind):
    seen = np.zeros(len(frontend.FUSE_CLASSES), dtype=np.int64)
    for tree in fc.TREES:
        for shape, V, rate, keep in (("37x53", 8, 0.5, "not_inf"), ("unequal", 3, 1.0, "finite"), ("5x7", 0, 1.0, "not_inf")):
            x = fc.inputs(kind, "float32", shape, tree)
            for p_max in (None, 40):
                want = frontend.reconstruct_scene_numpy(x["models"], kind, x["dm"], x["pairs"], x["tree"], p_max, x["centers"], x["sizes"], x["cams"], keep,
                                                        frontend.recon_threshold(rate), fc.SEED)
                got = _definition(kind, "float32", shape, tree, V, rate, 0.05, (0, V), p_max, keep=keep)
                assert fc.same_bytes((got[0], got[1], got[3], got[4]), want), (tree, shape, p_max)
                n = min(int(got[3][-1]), len(got[1]))
                assert got[2].shape == (len(got[1]), 2) and got[2].dtype == np.uint8 and not got[2][n:].any()
                assert (got[2][:n].astype(int).sum(axis=1) <= V).all()
            T = fc.transforms(kind, tree)
            hw = np.tile([x["H"], x["W"]], (x["I"], 1)) if x["sizes"] is None else x["sizes"]
            for i in range(x["I"]):
                if T[i]["depth"] >= 0:
                    cls = frontend.fuse_image_support_numpy(T, kind, i, fc.views(x["I"], V)[i], x["dm"], hw[:, 0], hw[:, 1], x["centers"], x["cams"], keep,
                                                            frontend.recon_threshold(rate), fc.SEED)[4]
                    seen += np.bincount(cls.reshape(-1), minlength=len(seen))
    assert (seen > 0).all(), seen  # every class of F5 is populated somewhere: the cases do what they are there for


@pytest.mark.parametrize("kind", fc.KINDS)
def test_a_gated_cloud_is_the_open_clouds_rows_that_pass_in_order(kind):
    for tree, shape, V, rate, tol in (("chain", "37x53", 8, 1.0, 0.05), ("star", "unequal", 3, 0.5, 0.0), ("forest", "37x53", 8, 0.5, 0.05), ("broken", "5x7", 3, 1.0, 0.05),
                                      ("mixed", "37x53", 1, 1.0, 0.05)):
        everything = fc.reference(kind, "float64", shape, tree, V, rate, tol, (0, V), None)
        dropped = 0
        for gate in fc.gates(V) + ((0, 0), (1, V)):
            got = _definition(kind, "float64", shape, tree, V, rate, tol, gate)
            s = everything[2].astype(int)
            g = (s[:, 0] >= gate[0]) & (s[:, 1] <= gate[1])
            assert got[0].tobytes() == everything[0][g].tobytes() and got[1].tobytes() == everything[1][g].tobytes() and got[2].tobytes() == everything[2][g].tobytes()
            per_image = [int(g[a:b].sum()) for a, b in zip(everything[3][:-1], everything[3][1:])]
            assert got[3].tolist() == [0] + np.cumsum(per_image).tolist()
            assert fc.same_bytes(got, fc.reference(kind, "float64", shape, tree, V, rate, tol, gate, None))  # the shared reference of the GPU tests
            if gate == (V + 1, 0):
                assert got[3][-1] == 0
            dropped += int((~g).sum())
            for p_max in (0, 7, int(got[3][-1]), int(got[3][-1]) + 9):  # F6's placement: truncated, exact, with filler
                cut = _definition(kind, "float64", shape, tree, V, rate, tol, gate, p_max)
                n = min(p_max, int(got[3][-1]))
                assert cut[3].tobytes() == got[3].tobytes() and cut[0][:n].tobytes() == got[0][:n].tobytes() and cut[2][:n].tobytes() == got[2][:n].tobytes()
                assert not cut[0][n:].any() and (cut[1][n:] == -1).all() and not cut[2][n:].any() and len(cut[1]) == p_max
        assert dropped > 0 or tree == "broken" and kind != "calibrated" or V == 0


def test_a_smaller_rate_keeps_a_subset_with_equal_support():
    kind, dt, shape, tree, V = "varying_focal", "float32", "37x53", "chain", 8
    full = fc.open_rows(kind, dt, shape, tree, V, 1.0, 0.05)
    prev = None
    for rate in (0.5, 0.05):
        part = fc.open_rows(kind, dt, shape, tree, V, rate, 0.05)
        for i, (f, p) in enumerate(zip(full, part)):
            at = {int(px): k for k, px in enumerate(f[1])}
            rows = [at[int(px)] for px in p[1]]  # (a KeyError: not a subset)
            assert rows == sorted(rows) and 0 < len(rows) < len(f[1])
            assert p[0].tobytes() == f[0][rows].tobytes() and p[2].tobytes() == f[2][rows].tobytes(), (rate, i)
            assert prev is None or set(p[1].tolist()) <= set(prev[i][1].tolist())
        prev = part


def test_an_images_rows_depend_on_its_own_row_of_views_alone():
    kind, dt, shape, tree, V = "calibrated", "float32", "37x53", "star", 3
    base = fc.open_rows(kind, dt, shape, tree, V, 1.0, 0.05)
    x = fc.inputs(kind, dt, shape, tree)
    rng = np.random.default_rng(3)
    for i in range(x["I"]):
        table = rng.integers(-2, x["I"] + 2, size=(x["I"], V)).astype(np.int32)
        table[i] = fc.views(x["I"], V)[i]
        lo, hi = frontend.covis_band(0.05)
        rows = frontend.fuse_rows_numpy(fc.transforms(kind, tree), kind, x["dm"], table, x["centers"], x["sizes"], x["cams"], "not_inf", ALL, fc.SEED, lo, hi, 0, V)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(rows[i], base[i])), i
    assert any(r[2].any() for r in base)


@pytest.mark.parametrize("kind", fc.KINDS)
def test_every_inert_slot_is_inert(kind):
    """F3: the image itself, a duplicate, an index outside the set, a detached image, an absent one and an image of another component change nothing"""
    dt, shape = "float32", "37x53"
    lo, hi = frontend.covis_band(0.05)

    def rows(tree, table, extra=None):
        x = fc.inputs(kind, dt, shape, tree)
        models, tr = x["models"], x["tree"].copy()
        if extra is not None:
            extra(tr)
        T = frontend.scene_transforms_numpy(models, kind, x["pairs"], tr, x["I"])
        return T, frontend.fuse_rows_numpy(T, kind, x["dm"], np.array(table, dtype=np.int32), x["centers"], x["sizes"], x["cams"], "not_inf", ALL, fc.SEED, lo, hi, 0, 8)

    def same(a, b, images):
        return all(x.tobytes() == y.tobytes() for i in images for x, y in zip(a[i], b[i]))

    # forest: {0, 1} and {2, 3, 4}.  Image 3's real views are 2 and 4.
    _, plain = rows("forest", [[1], [0], [3], [2], [3]])
    T, with_4 = rows("forest", [[1, -1, -1], [0, -1, -1], [3, -1, -1], [2, 4, -1], [3, -1, -1]])
    assert T[0]["root"] == 0 and T[3]["root"] == 2 and not same(plain, with_4, [3]) and plain[3][2][:, 0].max() == 1 and with_4[3][2][:, 0].max() == 2
    for name, slot in (("self", 3), ("duplicate", 2), ("duplicate of the second", 4), ("below the set", -1), ("above the set", 5), ("far outside", 2 ** 31 - 1),
                       ("another component", 0), ("another component's leaf", 1)):
        _, got = rows("forest", [[1, -1, -1], [0, -1, -1], [3, -1, -1], [2, 4, slot], [3, -1, -1]])
        assert same(got, with_4, range(5)), name
        _, front = rows("forest", [[1, -1, -1], [0, -1, -1], [3, -1, -1], [slot, 2, 4], [3, -1, -1]])  # an inert slot in FRONT of the valid ones
        assert same(front, with_4, range(5)), name
    assert frontend.fuse_valid_slots(T, [3, 2, 2, -1, 5, 0, 4, 4], 3) == [-1, 2, -1, -1, -1, -1, 4, -1]
    # detached: in "broken" a NaN pose detaches 2, 3 and 4, which images 0 and 1 list; absent: the star with image 1 made absent
    T, got = rows("broken", [[1, 2, 3], [0, 2, 4], [1, 3, 0], [2, 4, 0], [3, 0, 1]])
    _, want = rows("broken", [[1, -1, -1], [0, -1, -1], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1]])
    assert [int(t["depth"]) for t in T] == [0, 1, -1, -1, -1] and got[2] is None and same(got, want, [0, 1])
    assert got[0][2][:, 0].max() == 1
    T, got = rows("star", [[1, 2, 3], [2, 0, 4], [1, 0, 3], [0, 1, 2], [0, 1, 2]], lambda tr: tr.__setitem__(1, (0, fc.ABSENT)))
    _, want = rows("star", [[-1, 2, 3], [2, 0, 4], [-1, 0, 3], [0, -1, 2], [0, -1, 2]], lambda tr: tr.__setitem__(1, (0, fc.ABSENT)))
    assert T[1]["depth"] == -1 and got[1] is None and same(got, want, [0, 2, 3, 4]) and got[0][2][:, 0].max() == 2


@pytest.mark.parametrize("kind", fc.KINDS)
def test_no_views(kind):
    x = fc.inputs(kind, "float32", "37x53", "chain")
    for table in (np.zeros((5, 0), dtype=np.int32), np.full((5, 4), -1, dtype=np.int32)):
        for gate, empty in (((0, 0), False), ((1, 0), True)):
            got = _definition(kind, "float32", "37x53", "chain", 0, 0.5, 0.05, gate, None, table)
            want = frontend.reconstruct_scene_numpy(x["models"], kind, x["dm"], x["pairs"], x["tree"], None, x["centers"], x["sizes"], x["cams"], "not_inf",
                                                    frontend.recon_threshold(0.5), fc.SEED)
            if empty:
                assert got[3].tolist() == [0] * 6 and len(got[1]) == 0
            else:
                assert fc.same_bytes((got[0], got[1], got[3]), want[:3]) and not got[2].any() and len(got[1]) > 1000


# ---- a rendered scene: a fronto-parallel wall and a nearer box, three cameras side by side (the construction of tests/test_covis_host.py)
FOCAL, TX, Z_WALL, Z_BOX, H, W = 100.0, 0.2, 4.0, 2.0, 64, 128
CENTRE = np.array([64.0, 32.0])
BOX = ((39.5, 79.5), (15.5, 47.5))             # the box's face in image 0, in pixels: its edges lie between pixel centres
UNIT = (1.0, 2.0, 0.5)                          # image k stores its depths in its own unit (powers of two: every depth stays exact)
FLOATERS = (slice(50, 58), slice(20, 30))       # image 1: a block of the wall below the box at HALF the wall's depth
JUNK = (slice(0, 4), slice(100, 112))           # image 1: inf, NaN, 0 and a negative depth in turn
JUNK_VALUES = (np.inf, np.nan, 0.0, -1.0)
TREE_SHAPES = {"star": ([(1, 0), (2, 0)], [(0, fc.ROOT), (0, fc.E), (1, fc.E)]), "chain": ([(1, 0), (2, 1)], [(0, fc.ROOT), (0, fc.E), (1, fc.E)])}


def _true_maps():
    """Camera k stands k * TX to the left of camera 0: X_k = X_0 + (k TX, 0, 0).  The disparities FOCAL * TX / z are whole pixels per step (10 on the
    box and on the floaters, 5 on the wall), so a pixel centre of one image meets a pixel centre of every other."""
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    maps = []
    for k in range(3):
        shift = k * FOCAL * TX / Z_BOX
        on_box = (u > BOX[0][0] + shift) & (u < BOX[0][1] + shift) & (v > BOX[1][0]) & (v < BOX[1][1])
        maps.append(np.where(on_box, Z_BOX, Z_WALL))
    maps[1][FLOATERS] = Z_WALL / 2
    maps[1][JUNK] = np.tile(JUNK_VALUES, 3)[None, :]
    return np.stack(maps)


def _rendered(kind, shape, wrong=None):
    true = _true_maps()
    pairs, tree = TREE_SHAPES[shape]
    m = np.zeros(len(pairs), dtype=_capi.MODEL_DTYPE)
    for b, (a, c) in enumerate(pairs):  # X_c = (X_a + t) / scale in the images' own units
        m[b]["q"], m[b]["t"], m[b]["scale"] = [1.0, 0.0, 0.0, 0.0], [(c - a) * TX / UNIT[a], 0.0, 0.0], UNIT[c] / UNIT[a]
        m[b]["f1"] = m[b]["f2"] = 1.0 if kind == "calibrated" else FOCAL
    if wrong is not None:
        m[wrong]["scale"] *= 1.5
    cams = [{"model_id": 0, "params": [FOCAL, CENTRE[0], CENTRE[1], 0.0]}] * 3 if kind == "calibrated" else None
    dm = np.stack([true[k] / UNIT[k] for k in range(3)])
    return true, m, dm, np.array(pairs), np.array(tree), cams, (None if kind == "calibrated" else CENTRE)


def _predicted(true):
    """(3, H, W, 2): (n_cons, n_viol) of every pixel against the two other images, by whole-pixel geometry alone; -1 where the pixel is no candidate
    or is not tested"""
    out = np.full((3, H, W, 2), -1, dtype=np.int64)
    for i in range(3):
        for v in range(H):
            for u in range(W):
                z = true[i, v, u]
                if np.isinf(z):
                    continue
                out[i, v, u] = 0
                if not (np.isfinite(z) and z > 0):
                    continue
                for n in range(3):
                    ut = u + (n - i) * int(FOCAL * TX / z)
                    if n == i or not 0 <= ut < W:
                        continue
                    zt = true[n, v, ut]
                    if np.isfinite(zt) and zt > 0:
                        out[i, v, u] += (int(z == zt), int(z < zt))
    return out


@pytest.mark.parametrize("shape", sorted(TREE_SHAPES))
@pytest.mark.parametrize("kind", fc.KINDS)
def test_a_rendered_scene_keeps_what_a_second_image_confirms(kind, shape):
    """tol = 0, min_consistent = 1, max_violating = 0, every pixel a candidate.  Every pixel's support is predicted by whole-pixel geometry, which is
    more than the statements that follow from it: no floater survives, no survivor is violated, and a pixel of the wall survives iff it lands in
    another image on a known depth of the WALL.  (A wall pixel that every image it lands in has the box in front of is occluded there, which F5
    counts for neither side: 'lands on a known depth' alone does not keep it.)"""
    true, m, dm, pairs, tree, cams, centre = _rendered(kind, shape)
    table = np.array([[1, 2], [0, 2], [0, 1]], dtype=np.int32)
    want = _predicted(true)
    everything = frontend.fuse_scene_numpy(m, kind, dm, pairs, tree, table, None, centre, None, cams, "not_inf", ALL, 0, 1.0, 1.0, 0, 2)
    points, pixel, support, offsets, T = frontend.fuse_scene_numpy(m, kind, dm, pairs, tree, table, None, centre, None, cams, "not_inf", ALL, 0, 1.0, 1.0, 1, 0)
    assert [int(t["depth"]) for t in T] == ([0, 1, 1] if shape == "star" else [0, 1, 2]) and (T["root"] == 0).all()
    got = np.full((3, H, W, 2), -1, dtype=np.int64)
    survives = np.zeros((3, H, W), dtype=bool)
    for i in range(3):
        px = everything[1][everything[3][i]:everything[3][i + 1]]
        got[i, px // W, px % W] = everything[2][everything[3][i]:everything[3][i + 1]]
        px = pixel[offsets[i]:offsets[i + 1]]
        survives[i, px // W, px % W] = True
    assert (got == want).all(), np.argwhere((got != want).any(axis=-1))[:5]
    assert (survives == ((want[..., 0] >= 1) & (want[..., 1] == 0))).all()
    assert not survives[1][FLOATERS].any() and (want[1][FLOATERS][..., 1] >= 1).all()         # no floater pixel survives: each is seen through
    assert not survives[1][JUNK].any() and (got[1][JUNK][:, 1::4] == 0).all()                  # NaN, 0 and negative depths: candidates without support
    assert (support[:, 1] == 0).all() and (support[:, 0] >= 1).all() and len(support) == survives.sum() > 3 * H * W // 2
    wall = np.isclose(true, Z_WALL)
    assert survives[wall].sum() > 0.8 * wall.sum() and (survives[wall] == (want[wall][:, 0] >= 1)).all() and (want[wall][:, 1] == 0).all()
    hidden = wall & ~survives & (got[..., 0] == 0)
    assert hidden[0].any()  # wall beside the box that both other cameras have the box in front of
    # the points of all three images lie on the two surfaces, in image 0's unit
    assert set(np.unique(points[:, 2]).tolist()) == {Z_BOX, Z_WALL}
    # a wrong scale on image 2's pair: its survivors drop strictly, and so do those of the images that look at it
    _, mw, _, _, _, _, _ = _rendered(kind, shape, wrong=1)
    _, _, sup_w, off_w, _ = frontend.fuse_scene_numpy(mw, kind, dm, pairs, tree, table, None, centre, None, cams, "not_inf", ALL, 0, 1.0, 1.0, 1, 0)
    assert off_w[3] - off_w[2] < offsets[3] - offsets[2] and off_w[3] < offsets[3] and (sup_w[:, 1] == 0).all()


# ---- scene_views
def test_scene_views_orders_partners_by_weight_then_index():
    from mdrp_amd import fuse
    pairs = [[0, 1], [2, 0], [0, 3], [3, 0], [4, 4], [0, 9], [1, 2], [-1, 2], [0, 5], [0, 6]]
    weights = [5.0, 7.0, 5.0, 6.0, 9.0, 9.0, 1.0, 9.0, 0.0, -3.0]
    v = fuse.scene_views(pairs, 7, 4, weights)
    assert v.dtype == np.int32 and v.shape == (7, 4)
    assert v.tolist() == [[2, 3, 1, -1], [0, 2, -1, -1], [0, 1, -1, -1], [0, -1, -1, -1], [-1] * 4, [-1] * 4, [-1] * 4]  # 3 by its best weight, once
    assert fuse.scene_views(pairs, 7, 2, weights)[0].tolist() == [2, 3] and fuse.scene_views(pairs, 7, 0, weights).shape == (7, 0)
    tie = fuse.scene_views([[3, 0], [0, 2], [1, 0]], 4)  # no weights: every pair 1, ties by ascending image index
    assert tie.shape == (4, 8) and tie[0, :4].tolist() == [1, 2, 3, -1]
    nan = fuse.scene_views([[0, 1], [0, 2]], 3, 8, [float("nan"), 2.0])
    assert nan[0, :2].tolist() == [2, -1] and nan[1, 0] == -1
    for bad in (lambda: fuse.scene_views(pairs, 7, 9), lambda: fuse.scene_views(pairs, 7, -1), lambda: fuse.scene_views(pairs, -1), lambda: fuse.scene_views(pairs, 7, 4, [1.0])):
        with pytest.raises(ValueError):
            bad()
    assert "NEED NOT be a partner" in fuse.scene_views.__doc__


# ---- the Python layer
def test_python_refusals():
    import torch
    import mdrp_amd.poselib as poselib
    from mdrp_amd import fuse
    for name in ("fuse_scene_torch", "fuse_scene", "scene_views"):
        assert getattr(poselib, name) is getattr(fuse, name)
    with pytest.raises(ValueError, match="kind"):
        poselib.fuse_scene_torch("relpose_5pt", None, None, None, None, None)
    with pytest.raises(ValueError):
        poselib.fuse_scene_torch("calibrated", None, np.zeros((1, 2, 2)), [[0, 0]], [[-1, 2]], [[0]])  # not a tensor on the GPU
    good = dict(rate=0.5, seed=0, keep="not_inf", p_max=None, pixels=100, n_views=3, tol=0.05, min_consistent=1, max_violating=0)
    for field, value, word in (("rate", 0.0, "rate"), ("rate", float("nan"), "rate"), ("rate", 1e-12, "rate"), ("seed", -1, "seed"), ("seed", 1 << 64, "seed"),
                               ("keep", "all", "keep"), ("p_max", -1, "p_max"), ("p_max", 1 << 31, "p_max"), ("tol", -0.01, "tol"), ("tol", 1.01, "tol"),
                               ("tol", float("nan"), "tol"), ("min_consistent", -1, "min_consistent"), ("max_violating", -1, "max_violating")):
        with pytest.raises(ValueError, match=word):
            fuse._options(**dict(good, **{field: value}))
    o = fuse._options(**good)
    assert (o.keep, o.thr, o.seed, o.p_max, o.n_views, o.lo, o.hi, o.min_consistent, o.max_violating) == (
        0, frontend.recon_threshold(0.5), 0, _capi_default_p_max(100, 0.5), 3, 0.95, 1.05, 1, 0)
    assert fuse._options(**dict(good, rate=2.0, p_max=7)).thr == ALL
    cpu = torch.device("cpu")
    for table, word in ((np.zeros((2, 9), dtype=np.int32), "at most 8"), (np.zeros((3, 2), dtype=np.int32), "one row per image"), (np.zeros((2, 2)), "integers"),
                        (np.zeros(4, dtype=np.int32), "integers"), (torch.zeros((2, 2)), "integers"), (torch.zeros((2, 9), dtype=torch.int64), "at most 8")):
        with pytest.raises(ValueError, match=word):
            fuse._views_table(table, 2, cpu)
    t, V = fuse._views_table([[1, -1], [2 ** 40, 0]], 2, cpu)
    assert V == 2 and t.dtype == torch.int32 and t.tolist() == [[1, -1], [2 ** 31 - 1, 0]]
    assert fuse._views_table(np.zeros((2, 0), dtype=np.int32), 2, cpu)[1] == 0 and fuse._views_table([], 2, cpu)[1] == 0
    assert "UNTUNED" in fuse.fuse_scene_torch.__doc__ and "need not be a partner" in fuse.fuse_scene_torch.__doc__
    x = fc.inputs("shared_focal", "float32", "5x7", "two")
    for bad in (dict(views=np.zeros((2, 9), dtype=np.int64)), dict(lo=0.9, hi=0.95), dict(lo=np.nan), dict(min_consistent=-1), dict(max_violating=-1), dict(keep="all")):
        kw = dict(dict(views=fc.views(2, 1)), **bad)
        with pytest.raises(ValueError):
            frontend.fuse_scene_numpy(x["models"], "shared_focal", x["dm"], x["pairs"], x["tree"], kw.pop("views"), None, x["centers"], **kw)
    with pytest.raises(ValueError):
        frontend.fuse_scene_numpy(x["models"], "relpose_5pt", x["dm"], x["pairs"], x["tree"], fc.views(2, 1))


def _capi_default_p_max(pixels, rate):
    from mdrp_amd import reconstruct
    return reconstruct.default_p_max(pixels, frontend.recon_threshold(rate))


# ---- header, binding, build, library
def test_header_binding_and_build_agree(tmp_path):
    from mdrp_amd import build
    import __graft_entry__ as ge
    inc = os.path.join(ROOT, "include")
    main = open(os.path.join(inc, "mdrp.h")).read()
    assert int(re.search(r"#define MDRP_ABI_VERSION (0x[0-9a-fA-F]+)", main).group(1), 16) == 6 == _capi.ABI_VERSION  # new symbols only
    for other in sorted(os.listdir(inc)):  # no other header names the new identifiers
        if other != "mdrp_fuse.h":
            text = open(os.path.join(inc, other)).read()
            for name in NAMES + ("mdrp_fuse_opt", "MDRP_FUSE_MAX_VIEWS"):
                assert not re.search(r"\b" + name + r"\b", text), (other, name)
    assert '#include "mdrp_fuse.h"' in open(os.path.join(inc, "mdrp_covis.h")).read().rstrip().splitlines()[-2]  # reached from the covis header's tail
    path = os.path.join(inc, "mdrp_fuse.h")
    hdr = open(path).read()
    for rule in ("F1.", "F2.", "F3.", "F4.", "F5.", "F6.", "48 bytes", "tests/test_gpu_fuse_history.py"):
        assert rule in hdr, rule
    deps = [os.path.realpath(d) for d in build.DEPS]
    assert os.path.realpath(path) in deps and os.path.realpath(os.path.join(ROOT, "mdrp_amd", "csrc", "mdrp_fuse.h")) in deps
    assert sorted(_capi.EXPORTS_FUSE) == sorted(NAMES) == sorted(set(re.findall(r"\b(mdrp_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))))
    others = (set(_capi.EXPORTS) | set(_capi.EXPORTS_CLASSIC_RANKED) | set(_capi.EXPORTS_CLASSIC_MODELS) | set(_capi.EXPORTS_CLASSIC_FRONTEND)
              | set(_capi.EXPORTS_CLASSIC_FOCALS) | set(_capi.EXPORTS_DENSE) | set(_capi.EXPORTS_RECONSTRUCT) | set(_capi.EXPORTS_SCENE) | set(_capi.EXPORTS_COVIS))
    assert not set(_capi.EXPORTS_FUSE) & others
    assert "EXPORTS_FUSE" in open(ge.__file__).read()
    t = _capi.FuseOpt
    src = tmp_path / "layout.c"
    src.write_text('#include "mdrp.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n    printf("%zu ", sizeof(mdrp_fuse_opt));\n'
                   + "".join(f'    printf("%zu ", offsetof(mdrp_fuse_opt, {n}));\n' for n, _ in t._fields_) + '    printf("%d", MDRP_FUSE_MAX_VIEWS);\n'
                   + "    return mdrp_fuse_scene_async ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-Wno-address", str(src), "-I", inc, "-o", str(tmp_path / "layout.o")], check=True)
    build.build()
    lib = _capi.load_library()
    subprocess.run(["gcc", str(tmp_path / "layout.o"), "-o", str(tmp_path / "layout"), build.OUT, "-Wl,--unresolved-symbols=ignore-in-shared-libs"], check=True)
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(build.OUT) + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    out = [int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, env=env).stdout.split()]
    want = [C.sizeof(t)] + [getattr(t, n).offset for n, _ in t._fields_]
    assert out == want + [_capi.FUSE_MAX_VIEWS] and want == [48, 0, 4, 8, 16, 20, 24, 32, 40, 44], (out, want)
    assert _capi.FUSE_MAX_VIEWS == frontend.FUSE_MAX_VIEWS == 8
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{(.*?)\} mdrp_fuse_opt;", hdr, flags=re.S).group(1), flags=re.S)
    assert re.findall(r"\b(\w+)(?:\[\d+\])?;", body) == [n for n, _ in t._fields_]  # the fields in the header's order
    syms = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    m = re.search(r"\bint\s+mdrp_fuse_scene_async\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    args = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
    assert hasattr(lib, NAMES[0]) and re.search(rf"\bT {NAMES[0]}\b", syms)
    assert len(getattr(lib, NAMES[0]).argtypes) == len(args) == 15
    assert callable(_capi.Handle.fuse_scene_device) and "fuse_scene_device" not in vars(_capi.Handle)  # in a base class: the recorded per-method cases are Handle's own


def test_the_handle_method_hands_its_arguments_on():
    """the handle method against a recording stand-in for the library: the symbol, the argument order, the cameras as a host table"""
    calls = []

    class Lib:
        def __getattr__(self, name):
            if not name.startswith("mdrp_"):
                raise AttributeError(name)
            return lambda *a: calls.append((name, a)) or 0

    h = _capi.Handle.__new__(_capi.Handle)
    h._lib, h._h = Lib(), C.c_void_p(0x1000)
    try:
        cams = fc.inputs("calibrated", "float32", "5x7", "mixed")["cams"]
        opt = _capi.FuseOpt(0, 77, 5, 100, 3, 0.95, 1.05, 1, 0)
        h.fuse_scene_device(_capi.CALIB, _capi.DepthImagePairs(), opt, 2, 0x2000, 136, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, cams, 0x9000)
        h.fuse_scene_device(_capi.SHARED_FOCAL, _capi.DepthImagePairs(), opt, 2, 0x2000, 96, 0x3000, None, 0x5000, 0x6000, 0x7000, 0x8000)
        with pytest.raises(ValueError):
            h.fuse_scene_device(_capi.SHARED_FOCAL, _capi.DepthPairs(), opt, 2, 0x2000, 96, 0x3000, None, 0x5000, 0x6000, 0x7000, 0x8000)
    finally:
        h._h = None
    (n1, a1), (n2, a2) = calls
    assert n1 == n2 == "mdrp_fuse_scene_async" and len(a1) == len(a2) == 15
    assert a1[1] == _capi.CALIB and a1[4] == 2 and a1[5].value == 0x2000 and a1[6] == 136 and a1[9] is not None
    assert [a1[k].value for k in (7, 8, 10, 11, 12, 13, 14)] == [0x3000, 0x4000, 0x9000, 0x5000, 0x6000, 0x7000, 0x8000]  # tree, views, transforms, points, pixel, support, offsets
    assert a2[1] == _capi.SHARED_FOCAL and a2[6] == 96 and a2[8] is None and a2[9] is None and a2[10] is None and a2[13].value == 0x7000


# ---- the host build of the kernels' arithmetic (tests/hostmath/fuse_host.cpp, a stand-alone program) against the definition
@pytest.fixture(scope="module")
def fuse_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fuse_host") / "fuse_host"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "hostmath", "fuse_host.cpp"), "-o", str(exe)])
    return str(exe)


def _host_run(exe, tmp_path, kind_id, x, T, table, keep, thr, lo, hi, gate):
    I, H, W, V = x["I"], x["H"], x["W"], table.shape[1]
    cams = np.zeros(I, dtype=_capi.CAMERA_DTYPE) if x["cams"] is None else x["cams"]
    sizes = np.tile(np.array([H, W], dtype=np.int32), (I, 1)) if x["sizes"] is None else x["sizes"]
    hdr = np.array([kind_id, I, H, W, V, _capi.RECON_KEEP[keep], gate[0], gate[1], thr, fc.SEED & 0xFFFFFFFF, 0, 0], dtype=np.uint32)
    blob = b"".join(np.ascontiguousarray(a).tobytes() for a in (hdr, np.array([lo, hi]), T, cams, x["centers"].astype(np.float64), sizes.astype(np.int32),
                                                              table.astype(np.int32), x["dm"].astype(np.float64)))
    assert cams.dtype.itemsize == 40
    (tmp_path / "in.bin").write_bytes(blob)
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    return np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint8).reshape(I, H, W, 3)


@pytest.mark.parametrize("shape", sorted(fc.SHAPES))
@pytest.mark.parametrize("kind_id, kind", list(enumerate(fc.KINDS)))
def test_host_arithmetic_equals_the_definition_as_bytes(fuse_host, tmp_path, kind_id, kind, shape):
    """every candidate's (n_cons, n_viol) and keep bit, for trees of every shape (the cameras of the calibrated kind alternate between both models), both
    depth types, rates, both tolerances and both filters"""
    checked = 0
    for n, tree in enumerate(("one", "mixed", "chain", "forest", "broken")):
        for dt, V, rate, tol, gate, keep in (("float32", 8, 1.0, 0.05, (1, 0), "not_inf"), ("float64", 3, 0.5, 0.0, (2, 1), "finite"), ("float32", 0, 1.0, 0.05, (0, 0), "not_inf")):
            x = fc.inputs(kind, dt, shape, tree)
            T = fc.transforms(kind, tree)
            lo, hi = frontend.covis_band(tol)
            got = _host_run(fuse_host, tmp_path, kind_id, x, T, fc.views(x["I"], V), keep, frontend.recon_threshold(rate), lo, hi, gate)
            want = np.zeros_like(got)
            for i, r in enumerate(fc.open_rows(kind, dt, shape, tree, V, rate, tol, keep)):
                if r is not None:
                    want[i, r[1] // x["W"], r[1] % x["W"]] = np.concatenate([r[2], (1 + 2 * frontend.fuse_gate(r[2], *gate))[:, None].astype(np.uint8)], axis=1)
            assert got.tobytes() == want.tobytes(), (tree, dt, V, np.argwhere((got != want).any(axis=-1))[:5])
            checked += int((want[..., 2] & 1).sum())
    assert checked > (0 if shape == "1x1" and kind != "calibrated" else 3)
