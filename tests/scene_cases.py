"""Case builders for the scene tests (include/mdrp_scene.h): trees over small image sets - chain, star, mixed directions, two roots, and
every way an image can be detached - with the models, maps, cameras and centres of tests/reconstruct_cases.py, and the reference as the NumPy
definition states it (mdrp_amd/frontend.py scene_transforms_numpy, scene_rows_numpy), computed once per case and shared."""
import functools

import numpy as np

import reconstruct_cases as rc
from mdrp_amd import _capi, frontend

KINDS = rc.KINDS
KEEPS = rc.KEEPS
RATES = (1.0, 0.5, 0.05)
SEED = rc.SEED
H, W = 33, 70  # the allocation; the valid regions below run from 1 x 1 to all of it
SIZES = ((33, 70), (1, 1), (17, 64), (33, 1), (1, 70), (20, 33), (32, 32), (5, 7), (29, 69))
_USABLE = [b for b in range(rc.B_MAX) if b not in rc.EMPTY]
_NAN_POSE = 1  # rc.EMPTY: a NaN in q

E, ROOT, ABSENT = _capi.SCENE_EDGE, _capi.SCENE_ROOT, _capi.SCENE_ABSENT
_chain_pairs = [(i, i - 1) if i % 2 else (i - 1, i) for i in range(1, 9)]  # forward and inverse edges alternate

# name: I, pairs, tree (pair, role), the pairs whose model is a NaN pose, and what must come out: {image: (root, depth)}, every other image detached
TREES = {
    "one": dict(I=1, pairs=[(0, 1)], tree=[(-1, ROOT)], attached={"calibrated": {0: (0, 0)}}),  # a pair-less root is the calibrated kind's alone
    "two": dict(I=2, pairs=[(0, 1)], tree=[(0, E), (0, ROOT)], attached={0: (1, 1), 1: (1, 0)}),
    "two_inverse": dict(I=2, pairs=[(0, 1)], tree=[(0, ROOT), (0, E)], attached={0: (0, 0), 1: (0, 1)}),
    "star": dict(I=5, pairs=[(1, 0), (0, 2), (3, 0), (0, 4)], tree=[(0, ROOT), (0, E), (1, E), (2, E), (3, E)],
                 attached={0: (0, 0), 1: (0, 1), 2: (0, 1), 3: (0, 1), 4: (0, 1)}),
    "forest": dict(I=5, pairs=[(1, 0), (3, 2), (3, 4)], tree=[(0, ROOT), (0, E), (1, ROOT), (1, E), (2, E)],
                   attached={0: (0, 0), 1: (0, 1), 2: (2, 0), 3: (2, 1), 4: (2, 2)}),
    "small_defects": dict(I=5, pairs=[(0, 1), (2, 4)], tree=[(0, ROOT), (0, ABSENT), (2, E), (0, E), (1, 3)],  # absent | pair index B | pair without image 3 | role 3
                          attached={0: (0, 0)}),
    "chain": dict(I=9, pairs=_chain_pairs, tree=[(0, ROOT)] + [(i - 1, E) for i in range(1, 9)], attached={i: (0, i) for i in range(9)}),
    # 2 hangs on a NaN pose and 3 below it; 4's pair has a == c; 5 and 6 hang on each other; 8's pair leaves the set; 0, 1 and 7 are unaffected
    "defects": dict(I=9, pairs=[(0, 1), (1, 2), (2, 3), (4, 4), (5, 6), (6, 5), (7, 0), (8, 9), (-3, 8)],
                    tree=[(0, ROOT), (0, E), (1, E), (2, E), (3, E), (4, E), (5, E), (6, E), (7, E)], nan=(1,),
                    attached={0: (0, 0), 1: (0, 1), 7: (0, 1)}),
    "hangs_on_absent": dict(I=5, pairs=[(0, 1), (1, 2), (3, 2), (4, 3)], tree=[(0, ROOT), (0, ABSENT), (1, E), (2, E), (-2, ROOT)],
                            attached={0: (0, 0)}),
}


def attached(name, kind):
    a = TREES[name]["attached"]
    return a.get(kind, {}) if any(isinstance(k, str) for k in a) else a


def tree_arrays(name):
    t = TREES[name]
    return np.array(t["pairs"], dtype=np.int32).reshape(-1, 2), np.array(t["tree"], dtype=np.int32).reshape(-1, 2)


def models(kind, name):
    """one usable model per pair of the case (full mantissas everywhere, negative scales among them), a NaN pose where the case plants one"""
    t = TREES[name]
    all_models = rc.models(kind)
    m = all_models[_USABLE[:len(t["pairs"])]].copy()
    for b in t.get("nan", ()):
        m[b] = all_models[_NAN_POSE]
    return m


@functools.lru_cache(maxsize=None)
def inputs(kind, dtype_name, name):
    """everything a scene call takes for the case"""
    I = TREES[name]["I"]
    pairs, tree = tree_arrays(name)
    dm = rc.depth_maps(H, W, np.dtype(dtype_name), n=I, seed=21, whole_inf=3)
    return {"models": models(kind, name), "dm": dm, "pairs": pairs, "tree": tree, "sizes": np.array(SIZES[:I], dtype=np.int32), "centers": rc.centres(I)[0],
            "cams": rc.cameras(I)[0] if kind == "calibrated" else None, "I": I}


@functools.lru_cache(maxsize=None)
def transforms(kind, name):
    x = inputs(kind, "float32", name)
    return frontend.scene_transforms_numpy(x["models"], kind, x["pairs"], x["tree"], x["I"])


@functools.lru_cache(maxsize=None)
def rows(kind, dtype_name, name, keep, rate):
    """the definition's kept rows per image: computed once, shared by every p_max"""
    x = inputs(kind, dtype_name, name)
    return frontend.scene_rows_numpy(transforms(kind, name), kind, x["dm"], x["centers"], x["sizes"], x["cams"], keep, frontend.recon_threshold(rate), SEED)


def reference(kind, dtype_name, name, keep, rate, p_max):
    """(points (p_max, 3), pixel (p_max,), offsets (I + 1,), transforms (I,)) by the definition"""
    return (*frontend.pack_scene_rows(rows(kind, dtype_name, name, keep, rate), p_max), transforms(kind, name))


def p_max_cases(kind, dtype_name, name, keep, rate):
    """S6's five cases: 0, inside image 0, exact - 1, exact, generous (equal ones collapse)"""
    r = rows(kind, dtype_name, name, keep, rate)
    n0, n = (0 if r[0] is None else len(r[0][1])), sum(0 if x is None else len(x[1]) for x in r)
    return sorted({0, n0 // 2, max(n - 1, 0), n, n + 1500})


def run(kind, dtype_name, name, keep, rate, p_max, models=None, device="cuda:0"):
    """poselib.reconstruct_scene_torch on the case: (points, pixel, offsets, transform records) as NumPy arrays"""
    import torch
    from mdrp_amd import poselib, scene
    x = inputs(kind, dtype_name, name)
    out = poselib.reconstruct_scene_torch(kind, x["models"] if models is None else models, torch.from_numpy(x["dm"]).to(torch.device(device)), x["pairs"], x["tree"],
                                          x["cams"], x["centers"], x["sizes"], rate, SEED, keep, p_max, return_transforms=True)
    return tuple(t.cpu().numpy() for t in out[:3]) + (scene._records(out[3]),)


# ---- the wide cases (tests/test_gpu_backend_wide.py): the scenes of fuse_cases.WIDE_CASES - maps of 257 tiles, and 257 images - with that module's
# inputs (models near the identity, so the same scenes serve the consistency filter), by the same definition
@functools.lru_cache(maxsize=None)
def wide_rows(kind, dtype_name, case, keep, rate):
    import fuse_cases as fc
    shape, tree, _ = fc.WIDE_CASES[case]
    x = fc.inputs(kind, dtype_name, shape, tree)
    return frontend.scene_rows_numpy(fc.transforms(kind, tree), kind, x["dm"], x["centers"], x["sizes"], x["cams"], keep, frontend.recon_threshold(rate), fc.SEED)


def wide_reference(kind, dtype_name, case, keep, rate, p_max):
    """(points (p_max, 3), pixel (p_max,), offsets (I + 1,), transforms (I,)) by the definition"""
    import fuse_cases as fc
    return (*frontend.pack_scene_rows(wide_rows(kind, dtype_name, case, keep, rate), p_max), fc.transforms(kind, fc.WIDE_CASES[case][1]))


def wide_run(kind, dtype_name, case, keep, rate, p_max, device="cuda:0"):
    """poselib.reconstruct_scene_torch on the wide case: (points, pixel, offsets, transform records) as NumPy arrays"""
    import torch
    import fuse_cases as fc
    from mdrp_amd import poselib, scene
    shape, tree, _ = fc.WIDE_CASES[case]
    x = fc.inputs(kind, dtype_name, shape, tree)
    out = poselib.reconstruct_scene_torch(kind, x["models"], torch.from_numpy(x["dm"]).to(torch.device(device)), x["pairs"], x["tree"], x["cams"], x["centers"],
                                          x["sizes"], rate, fc.SEED, keep, p_max, return_transforms=True)
    return tuple(t.cpu().numpy() for t in out[:3]) + (scene._records(out[3]),)


def same_bytes(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


# ---- straight through a handle (refusals, history): the call on a case's inputs, the outputs as byte strings
def device_call(h, kind="varying_focal", dtype_name="float32", name="chain", rate=0.5, keep="not_inf", p_max=6000, stride=96, change=None, transforms_only=False,
                with_transforms=True, tile=1):
    """h.reconstruct_scene_device (or h.scene_transforms_device) on the inputs of (kind, dtype, case); change(args) may overwrite any entry of the
    argument dict before the call (desc, opt, kind, batch, models, stride, tree, points, pixel, offsets, cams, transforms, n_images, pairs).  tile:
    every map repeated tile x tile times (the allocation and the valid regions grow with it)."""
    import torch
    from mdrp_amd import poselib
    x = inputs(kind, dtype_name, name)
    dev = torch.device("cuda:0")
    I, B = x["I"], len(x["pairs"])
    rec = np.zeros(B, dtype=_capi.RESULT_DTYPE if stride == 136 else _capi.MODEL_DTYPE)
    (rec["model"] if stride == 136 else rec)[...] = x["models"]
    mt = torch.from_numpy(rec.view(np.uint8).reshape(B, stride).copy()).to(dev)
    dm, cs, sz = torch.from_numpy(np.tile(x["dm"], (1, tile, tile))).to(dev), torch.from_numpy(x["centers"]).to(dev), torch.from_numpy(x["sizes"] * tile).to(dev)
    pr, tr = torch.from_numpy(x["pairs"]).to(dev), torch.from_numpy(x["tree"]).to(dev)
    desc = _capi.DepthImagePairs(dm.data_ptr(), _capi.F32 if dtype_name == "float32" else _capi.F64, H * tile, W * tile, I, sz.data_ptr(), cs.data_ptr(), pr.data_ptr())
    opt = _capi.ReconstructOpt(_capi.RECON_KEEP[keep], frontend.recon_threshold(rate), SEED, p_max, 0)
    points = torch.full((p_max, 3), 7.0, dtype=torch.float32, device=dev)
    pixel = torch.full((p_max,), 7, dtype=torch.int32, device=dev)
    offsets = torch.full((I + 1,), 7, dtype=torch.int64, device=dev)
    T = torch.full((I, 128), 7, dtype=torch.uint8, device=dev)
    a = {"kind": poselib.MONODEPTH_KINDS[kind], "desc": desc, "opt": opt, "batch": B, "models": mt.data_ptr(), "stride": stride, "tree": tr.data_ptr(),
         "points": points.data_ptr(), "pixel": pixel.data_ptr(), "offsets": offsets.data_ptr(), "cams": x["cams"],
         "transforms": T.data_ptr() if with_transforms else None, "n_images": I, "pairs": pr.data_ptr()}
    if change is not None:
        change(a)
    torch.cuda.synchronize()
    if transforms_only:
        h.scene_transforms_device(a["kind"], a["batch"], a["models"], a["stride"], a["pairs"], a["n_images"], a["tree"], a["transforms"])
        h.synchronize()
        return (T.cpu().numpy().tobytes(),)
    h.reconstruct_scene_device(a["kind"], a["desc"], a["opt"], a["batch"], a["models"], a["stride"], a["tree"], a["points"], a["pixel"], a["offsets"], a["cams"],
                               a["transforms"])
    h.synchronize()
    return points.cpu().numpy().tobytes(), pixel.cpu().numpy().tobytes(), offsets.cpu().numpy().tobytes(), T.cpu().numpy().tobytes()
