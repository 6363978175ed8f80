"""Case builders for the consistency-filter tests (include/mdrp_fuse.h): small image sets under trees of every shape - one image, a
pair, mixed edge directions, a star, two roots, a subtree detached by an unusable model - with the models, maps, cameras and centres of
tests/covis_cases.py (near the identity, so that most of an image lands inside the others and every class of F5 is populated; depth maps around one
surface with outliers and planted +inf, -inf, NaN, 0 and negative depths), view tables that hold every inert kind of slot, and the reference as the
NumPy definition states it (mdrp_amd/frontend.py fuse_rows_numpy), computed once per case under the OPEN gate and shared: a gated cloud is the
open one's rows whose support passes (tests/test_fuse_host.py pins that against the definition itself)."""
import functools

import numpy as np

import covis_cases as cc
from mdrp_amd import _capi, frontend

KINDS = cc.KINDS
DTYPES = ("float32", "float64")
SEED = cc.SEED
RATES = (1.0, 0.5, 0.05)
TOLS = (0.0, 0.05)
VS = (0, 1, 3, 8)
E, ROOT, ABSENT = _capi.SCENE_EDGE, _capi.SCENE_ROOT, _capi.SCENE_ABSENT
# name: (H, W) of the allocation and the valid regions, None = all of it.  37 * 53 = 1961 pixels straddle a tile of 1024 and leave a lane's run hanging.
SHAPES = {"1x1": ((1, 1), None), "5x7": ((5, 7), None), "37x53": ((37, 53), None),
          "unequal": ((41, 60), ((41, 60), (37, 53), (1, 1), (20, 60), (41, 9)))}
_USABLE = (0, 2, 3, 4, 8, 10, 11, 12)  # cc.models: near the identity and usable
_NAN_POSE = 1

# name: I, pairs, tree (pair, role), the pairs whose model is a NaN pose
TREES = {
    "one": dict(I=1, pairs=[(0, 1)], tree=[(-1, ROOT)]),                                    # attached for the calibrated kind alone
    "two": dict(I=2, pairs=[(0, 1)], tree=[(0, E), (0, ROOT)]),
    "mixed": dict(I=3, pairs=[(1, 0), (1, 2)], tree=[(0, ROOT), (0, E), (1, E)]),           # a chain: a forward edge below the root, then an inverse one
    "chain": dict(I=5, pairs=[(1, 0), (1, 2), (3, 2), (3, 4)], tree=[(0, ROOT), (0, E), (1, E), (2, E), (3, E)]),
    "star": dict(I=5, pairs=[(1, 0), (0, 2), (3, 0), (0, 4)], tree=[(0, ROOT), (0, E), (1, E), (2, E), (3, E)]),
    "forest": dict(I=5, pairs=[(1, 0), (3, 2), (3, 4)], tree=[(0, ROOT), (0, E), (1, ROOT), (1, E), (2, E)]),   # two roots: {0, 1} and {2, 3, 4}
    "broken": dict(I=5, pairs=[(1, 0), (1, 2), (3, 2), (3, 4)], tree=[(0, ROOT), (0, E), (1, E), (2, E), (3, E)], nan=(1,)),  # 2, 3 and 4 detached
}


# ---- the wide cases (tests/test_gpu_backend_wide.py, tests/test_scan_runs_host.py; scenes and the filter alike).  Only the wide tests take them.
MANY = 257  # the smallest image count at which k_scene_scan's phase 1 runs per = 2 (thread 128 holds one image); five workgroups of k_scene_chain / k_fuse_views


def _many_tree(I=MANY, second_root=200, absent=(72, 250), nan_images=(100, 209)):
    """Two roots, 0 and 200.  Below a root every fourth image hangs on the root itself (a star) and starts a chain of depth 4; forward and inverse
    edges alternate.  Images 72 and 250 are absent: 72 ends its chain, 251 and 252 hang on 250 and are detached with it.  The pairs of images 100 and
    209 carry a NaN pose: 100 ends its chain, 210-212 hang below 209.  So lanes of the second and of the last workgroups of the per-image kernels
    take every branch, and no composed transform is more than four edges from the identity."""
    pairs, tree, nan = [], [], []
    for i in range(I):
        base = 0 if i < second_root else second_root
        if i == base:
            tree.append((len(pairs), ROOT))  # the pair of the next image, which hangs on this root
        elif i in absent:
            tree.append((0, ABSENT))
        else:
            parent = base if (i - base) % 4 == 1 else i - 1
            if i in nan_images:
                nan.append(len(pairs))
            tree.append((len(pairs), E))
            pairs.append((i, parent) if i % 2 else (parent, i))
    return dict(I=I, pairs=pairs, tree=tree, nan=tuple(nan))


# "wide": 409 * 643 pixels are 257 tiles, the smallest count at which k_scene_scan's phase 0 runs per = 2, beside an image of one tile (its pixel is one of
# cc.depth_maps' planted inf: attached, no row) and one whose valid region (189 tiles) ends before the allocation's tile count.  "many": the valid regions of SHAPES["unequal"] repeated; an allocation of 5 x 7
# clamps them, which leaves 5 x 7 and 1 x 1, and cc.depth_maps makes map 99 all inf: an attached image without a row in the middle of the scan.
WIDE_SHAPES = {"wide": ((409, 643), ((409, 643), (1, 1), (300, 643))), "many": ((5, 7), tuple(SHAPES["unequal"][1][i % 5] for i in range(MANY)))}
WIDE_TREES = {"many": _many_tree()}
# name: shape, tree, the image inside whose last tile the smaller p_max cuts (wide_p_max_cases)
WIDE_CASES = {"wide": ("wide", "mixed", 0), "many": ("many", "many", MANY - 1)}
WIDE_KINDS = ("varying_focal", "calibrated")
WIDE_VS = (0, 8)
WIDE_RATES = (1.0, 0.5)
WIDE_TOL = 0.05


def wide_gates(V):
    """the open gate | the default"""
    return ((0, V), (1, 0))


def wide_p_max_cases(rows, image):
    """rows: per image (points, pixel, ...) or None.  A cut inside the last tile of `image` (half of that tile's rows are written; the tile index
    is pixel // 1024 where the image's valid width is the allocation's) | the true total"""
    n = [0 if r is None else len(r[1]) for r in rows]
    pix = np.zeros(0, dtype=np.int64) if rows[image] is None else rows[image][1].astype(np.int64) // 1024
    last = int((pix == pix.max()).sum()) if len(pix) else 0
    return (max(sum(n[:image + 1]) - max(last // 2, 1), 0), sum(n))


def views(I, V):
    """(I, V) int32: every row of V = 8 holds the image itself, a duplicate, -1 and I beside its real views; V = 3 ends on the image itself and row 0
    is made of inert slots alone; V = 1 is the next image"""
    out = np.full((I, V), -1, dtype=np.int32)
    for i in range(I):
        nxt = [(i + k) % I for k in range(1, 5)]
        out[i] = ([i, nxt[0], nxt[0], -1, I, nxt[1], nxt[2], nxt[3]] if V == 8 else [nxt[0], nxt[1], i] if V == 3 else [nxt[0]])[:V]
    if V == 3:
        out[0] = [0, -1, I]
    return out


@functools.lru_cache(maxsize=None)
def inputs(kind, dtype_name, shape, tree):
    """everything a call takes but the views and the gate"""
    (H, W), sizes = SHAPES[shape] if shape in SHAPES else WIDE_SHAPES[shape]
    t = TREES[tree] if tree in TREES else WIDE_TREES[tree]
    I = t["I"]
    all_models = cc.models(kind)
    m = all_models[[_USABLE[b % len(_USABLE)] for b in range(len(t["pairs"]))]].copy()  # (the usable models go round where a tree has more pairs)
    for b in t.get("nan", ()):
        m[b] = all_models[_NAN_POSE]
    size = ((H, W), (H, W))
    return {"models": m, "dm": cc.depth_maps(H, W, np.dtype(dtype_name), n=I, seed=61, whole_inf=99), "pairs": np.array(t["pairs"], dtype=np.int32).reshape(-1, 2),
            "tree": np.array(t["tree"], dtype=np.int32).reshape(-1, 2), "sizes": None if sizes is None else np.array(sizes[:I], dtype=np.int32),
            "centers": cc.centres(kind, size, n=I)[0], "cams": cc.cameras(size, n=I)[0] if kind == "calibrated" else None, "I": I, "H": H, "W": W}


@functools.lru_cache(maxsize=None)
def transforms(kind, tree):
    x = inputs(kind, "float32", "5x7", tree)
    return frontend.scene_transforms_numpy(x["models"], kind, x["pairs"], x["tree"], x["I"])


@functools.lru_cache(maxsize=None)
def open_rows(kind, dtype_name, shape, tree, V, rate, tol, keep="not_inf"):
    """the definition's rows under the open gate: per image (points, pixel, support) of EVERY candidate, or None"""
    x = inputs(kind, dtype_name, shape, tree)
    lo, hi = frontend.covis_band(tol)
    return frontend.fuse_rows_numpy(transforms(kind, tree), kind, x["dm"], views(x["I"], V), x["centers"], x["sizes"], x["cams"], keep,
                                    frontend.recon_threshold(rate), SEED, lo, hi, 0, V)


def gated_rows(rows, gate):
    out = []
    for r in rows:
        g = None if r is None else frontend.fuse_gate(r[2], *gate)
        out.append(None if r is None else (r[0][g], r[1][g], r[2][g]))
    return out


def gates(V):
    """the open gate | the default | a looser one | one that keeps nothing"""
    return ((0, V), (1, 0), (2, 1), (V + 1, 0))


def reference(kind, dtype_name, shape, tree, V, rate, tol, gate, p_max, keep="not_inf"):
    """(points (p_max, 3), pixel (p_max,), support (p_max, 2), offsets (I + 1,), transforms (I,)) by the definition"""
    return (*frontend.pack_fuse_rows(gated_rows(open_rows(kind, dtype_name, shape, tree, V, rate, tol, keep), gate), p_max), transforms(kind, tree))


def kept_count(kind, dtype_name, shape, tree, V, rate, tol, gate, keep="not_inf"):
    return sum(0 if r is None else len(r[1]) for r in gated_rows(open_rows(kind, dtype_name, shape, tree, V, rate, tol, keep), gate))


def run(kind, dtype_name, shape, tree, V, rate, tol, gate, p_max, keep="not_inf", models=None, device="cuda:0", view_table=None):
    """poselib.fuse_scene_torch on the case: (points, pixel, support, offsets, transform records) as NumPy arrays"""
    import torch
    from mdrp_amd import poselib, scene
    x = inputs(kind, dtype_name, shape, tree)
    out = poselib.fuse_scene_torch(kind, x["models"] if models is None else models, torch.from_numpy(x["dm"]).to(torch.device(device)), x["pairs"], x["tree"],
                                   views(x["I"], V) if view_table is None else view_table, x["cams"], x["centers"], x["sizes"], rate, SEED, keep, tol, gate[0],
                                   gate[1], p_max, return_transforms=True)
    return tuple(t.cpu().numpy() for t in out[:4]) + (scene._records(out[4]),)


def same_bytes(got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


# ---- straight through a handle (refusals, history): the call on a case's inputs, the outputs as byte strings
def device_call(h, kind="varying_focal", dtype_name="float32", shape="37x53", tree="chain", V=3, rate=0.5, tol=0.05, gate=(1, 0), keep="not_inf", p_max=6000,
                stride=96, change=None, with_transforms=True):
    """h.fuse_scene_device on the inputs of the case; change(args) may overwrite any entry of the argument dict before the call (desc, opt, kind,
    batch, models, stride, tree, views, points, pixel, support, offsets, cams, transforms)."""
    import torch
    from mdrp_amd import poselib
    x = inputs(kind, dtype_name, shape, tree)
    dev = torch.device("cuda:0")
    I, B, H, W = x["I"], len(x["pairs"]), x["H"], x["W"]
    rec = np.zeros(B, dtype=_capi.RESULT_DTYPE if stride == 136 else _capi.MODEL_DTYPE)
    (rec["model"] if stride == 136 else rec)[...] = x["models"]
    mt = torch.from_numpy(rec.view(np.uint8).reshape(B, stride).copy()).to(dev)
    dm, cs = torch.from_numpy(x["dm"]).to(dev), torch.from_numpy(x["centers"]).to(dev)
    sz = None if x["sizes"] is None else torch.from_numpy(x["sizes"]).to(dev)
    pr, tr, vw = torch.from_numpy(x["pairs"]).to(dev), torch.from_numpy(x["tree"]).to(dev), torch.from_numpy(views(I, V)).to(dev)
    desc = _capi.DepthImagePairs(dm.data_ptr(), _capi.F32 if dtype_name == "float32" else _capi.F64, H, W, I, None if sz is None else sz.data_ptr(), cs.data_ptr(),
                                 pr.data_ptr())
    lo, hi = frontend.covis_band(tol)
    opt = _capi.FuseOpt(_capi.RECON_KEEP[keep], frontend.recon_threshold(rate), SEED, p_max, V, lo, hi, gate[0], gate[1])
    points = torch.full((p_max, 3), 7.0, dtype=torch.float32, device=dev)
    pixel = torch.full((p_max,), 7, dtype=torch.int32, device=dev)
    support = torch.full((p_max, 2), 7, dtype=torch.uint8, device=dev)
    offsets = torch.full((I + 1,), 7, dtype=torch.int64, device=dev)
    T = torch.full((I, 128), 7, dtype=torch.uint8, device=dev)
    a = {"kind": poselib.MONODEPTH_KINDS[kind], "desc": desc, "opt": opt, "batch": B, "models": mt.data_ptr(), "stride": stride, "tree": tr.data_ptr(),
         "views": vw.data_ptr() if V else None, "points": points.data_ptr(), "pixel": pixel.data_ptr(), "support": support.data_ptr(), "offsets": offsets.data_ptr(),
         "cams": x["cams"], "transforms": T.data_ptr() if with_transforms else None}
    if change is not None:
        change(a)
    torch.cuda.synchronize()
    h.fuse_scene_device(a["kind"], a["desc"], a["opt"], a["batch"], a["models"], a["stride"], a["tree"], a["views"], a["points"], a["pixel"], a["support"],
                        a["offsets"], a["cams"], a["transforms"])
    h.synchronize()
    return tuple(t.cpu().numpy().tobytes() for t in (points, pixel, support, offsets, T))
