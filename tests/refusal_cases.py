"""The refusal table of the C ABI's entry layer: every estimator, refine, gather, rank and budgets entry point of include/mdrp*.h, called through the
raw library symbols (the Handle wrappers would refuse first) with ONE valid tiny call (batch = 2, n_max = 8, max_iterations = 16, descriptors of 8
keypoints and 8 match rows) to which single defects, and for one entry point of each family every pair of defects, are applied.
tests/tools/gen_golden_refusals.py records (return code, mdrp_last_error()) of every probe into tests/golden/entry_refusals.json;
tests/test_gpu_refusals.py asserts that the library returns the same table.

Every probe is refused by host-side checks: ENTRIES lists, per entry point, only the defects that its checks catch before any pointer of the call
is dereferenced (a few are caught behind a gather of the valid descriptor or behind the handle's per-call reset: still without touching the
defective argument).  The defects an entry point would NOT refuse are left out; tests/test_gpu_refusals.py's docstring lists them."""
import ctypes as C
import itertools

import numpy as np

B, N, IMAGES, MAP = 2, 8, 3, 16
BUDGETS = (4, 8, 16)

SIGNATURES = {
    "mdrp_estimate_batch_async": "h kind x1 x2 d1 d2 batch n_max npp cam1 cam2 ropt bopt mask",
    "mdrp_estimate_batch": "h kind mem x1 x2 d1 d2 batch n_max npp cam1 cam2 ropt bopt out mask",
    "mdrp_estimate_batch_budgets_async": "h kind x1 x2 d1 d2 batch n_max npp cam1 cam2 ropt bopt budgets n_budgets bmask",
    "mdrp_estimate_batch_budgets": "h kind mem x1 x2 d1 d2 batch n_max npp cam1 cam2 ropt bopt budgets n_budgets bout bmask",
    "mdrp_fetch_results": "h out batch",
    "mdrp_copy_results_device": "h out batch",
    "mdrp_fetch_budget_results": "h bout n_budgets batch",
    "mdrp_copy_budget_results_device": "h bout n_budgets batch",
    "mdrp_estimate_batch_prior_async": "h kind x1 x2 d1 d2 batch n_max npp cam1 cam2 ropt bopt models mask",
    "mdrp_estimate_batch_prior": "h kind mem x1 x2 d1 d2 batch n_max npp cam1 cam2 ropt bopt models out mask",
    "mdrp_refine_batch_async": "h kind x1 x2 d1 d2 batch n_max npp cam1 cam2 ropt bopt models stages mask iscore iinl",
    "mdrp_refine_batch": "h kind mem x1 x2 d1 d2 batch n_max npp cam1 cam2 ropt bopt models stages out mask iscore iinl",
    "mdrp_estimate_batch_ranked_async": "h kind x1 x2 d1 d2 scores batch n_max npp cam1 cam2 ropt bopt mask",
    "mdrp_estimate_batch_ranked": "h kind mem x1 x2 d1 d2 scores batch n_max npp cam1 cam2 ropt bopt out mask",
    "mdrp_estimate_classic_ranked_async": "h kind x1 x2 scores batch n_max npp cam1 cam2 ropt bopt mask",
    "mdrp_estimate_classic_ranked": "h kind mem x1 x2 scores batch n_max npp cam1 cam2 ropt bopt out mask",
    "mdrp_rank_scores": "h mem scores batch n_max npp order",
    "mdrp_refine_classic_async": "h kind x1 x2 batch n_max npp cam1 cam2 ropt bopt models stages mask iscore iinl",
    "mdrp_refine_classic": "h kind mem x1 x2 batch n_max npp cam1 cam2 ropt bopt models stages out mask iscore iinl",
    "mdrp_estimate_classic_prior_async": "h kind x1 x2 batch n_max npp cam1 cam2 ropt bopt models prior_space mask",
    "mdrp_estimate_classic_prior": "h kind mem x1 x2 batch n_max npp cam1 cam2 ropt bopt models prior_space out mask",
}
for _stem, _point in (("matches", False), ("image_pairs", False), ("matches", True), ("image_pairs", True)):
    _outs = "x1 x2 slot n_host" if _point else "x1 x2 d1 d2 slot n_host"
    _gather = f"mdrp_gather_point_{_stem}" if _point else f"mdrp_gather_{_stem}"
    _est = f"mdrp_estimate_classic_{_stem}" if _point else f"mdrp_estimate_{_stem}"
    SIGNATURES[_gather] = f"h desc batch {_outs}"
    SIGNATURES[_gather + "_ranked"] = f"h desc fscores score_type batch {_outs}"
    SIGNATURES[_est + "_async"] = "h kind desc batch cam1 cam2 ropt bopt mmask n_used"
    SIGNATURES[_est + "_ranked_async"] = "h kind desc fscores score_type batch cam1 cam2 ropt bopt mmask n_used"


# ---------------------------------------------------------------------------------------------------------------------------------- defects
def _with(a, key, **fields):
    """a copy of the ctypes struct a[key] with some fields changed"""
    s = type(a[key]).from_buffer_copy(a[key])
    for f, v in fields.items():
        setattr(s, f, v)
    a[key] = s


def _set(**kw):
    return lambda a: a.update(kw)


DEFECTS = {
    "null_handle": _set(h=None),
    "null_ropt": _set(ropt=None),
    "null_bopt": _set(bopt=None),
    "kind_other_family": lambda a: a.update(kind=3 if a["kind"] <= 2 else 0),
    "kind_minus1": _set(kind=-1),
    "kind_6": _set(kind=6),
    "batch_minus1": _set(batch=-1),
    "n_max_minus1": _set(n_max=-1),
    "npp_negative": _set(npp=np.array([-1, N], dtype=np.int32)),
    "npp_past_n_max": _set(npp=np.array([N, N + 1], dtype=np.int32)),
    "null_x1": _set(x1=None),
    "null_d1": _set(d1=None),
    "null_cameras_kind0": _set(kind=0, cam1=None, cam2=None),
    "null_cameras_kind3": _set(kind=3, cam1=None, cam2=None),
    "null_cam1_kind4": _set(kind=4, cam1=None),
    "null_models": _set(models=None),
    "null_scores": _set(scores=None),
    "stages_minus1": _set(stages=-1),
    "stages_4": _set(stages=4),
    "prior_space_2": _set(prior_space=2),
    "mem_space_2": _set(mem=2),
    "null_out": _set(out=None, bout=None, order=None),
    "progressive_sampling": lambda a: _with(a, "ropt", progressive_sampling=1),
    "real_focal_check_kind4": lambda a: (a.update(kind=4), _with(a, "ropt", real_focal_check=1)),
    "real_focal_check_kind5": lambda a: (a.update(kind=5), _with(a, "ropt", real_focal_check=1)),
    "score_type_7": _set(score_type=7),
    "budgets_empty": _set(n_budgets=0),
    "budgets_not_increasing": _set(budgets=np.array([4, 4, 16], dtype=np.uint64)),
    "budgets_last_not_max_iterations": _set(budgets=np.array([4, 8, 12], dtype=np.uint64)),
    "budgets_too_many": _set(budgets=np.arange(1, 18, dtype=np.uint64), n_budgets=17),
    "desc_bad_kp_type": lambda a: _with(a, "desc", kp_type=2),
    "desc_bad_filter": lambda a: _with(a, "desc", filter=2),
    "desc_negative_size": lambda a: _with(a, "desc", m_max=-1),
    "desc_null_matches": lambda a: _with(a, "desc", matches=None),
}

_SHAPE = ["batch_minus1", "n_max_minus1", "npp_negative", "npp_past_n_max"]
_KINDS = ["kind_minus1", "kind_6"]
_OPTS = ["null_handle", "null_ropt", "null_bopt"]
_MONO_CAMS, _CLASSIC_CAMS = ["null_cameras_kind0"], ["null_cameras_kind3", "null_cam1_kind4"]
_RFC = ["real_focal_check_kind4", "real_focal_check_kind5"]
_BLOCKING = ["mem_space_2", "null_out"]
_BUDGETS = ["budgets_empty", "budgets_not_increasing", "budgets_last_not_max_iterations", "budgets_too_many"]
_STAGES = ["stages_minus1", "stages_4"]
_PLAIN = _OPTS + _KINDS + _SHAPE + ["null_d1"] + _MONO_CAMS + _CLASSIC_CAMS + ["progressive_sampling"] + _RFC
_MONO = _OPTS + ["kind_other_family"] + _KINDS + _SHAPE + ["null_d1"] + _MONO_CAMS
_CLASSIC = _OPTS + ["kind_other_family"] + _KINDS + _SHAPE + _CLASSIC_CAMS
_DESC, _POINT_DESC = ["desc_bad_kp_type", "desc_bad_filter", "desc_negative_size", "desc_null_matches"], ["desc_bad_kp_type", "desc_negative_size", "desc_null_matches"]
_FE_MONO = _OPTS + ["kind_other_family"] + _KINDS + ["batch_minus1"] + _MONO_CAMS + _DESC
_FE_CLASSIC = _OPTS + ["kind_other_family"] + _KINDS + ["batch_minus1"] + _CLASSIC_CAMS + _RFC + _POINT_DESC

# entry point -> (family of the base call: "mono" | "classic", the defects it refuses)
ENTRIES = {
    "mdrp_estimate_batch_async": ("mono", _PLAIN),
    "mdrp_estimate_batch": ("mono", _PLAIN + ["null_out"]),
    "mdrp_estimate_batch_budgets_async": ("mono", _PLAIN + _BUDGETS),
    "mdrp_estimate_batch_budgets": ("mono", _PLAIN + ["null_out"] + _BUDGETS),
    "mdrp_fetch_results": ("mono", ["null_handle", "null_out", "batch_minus1"]),
    "mdrp_copy_results_device": ("mono", ["null_handle", "null_out", "batch_minus1"]),
    "mdrp_fetch_budget_results": ("mono", ["null_handle", "null_out", "batch_minus1", "budgets_empty"]),
    "mdrp_copy_budget_results_device": ("mono", ["null_handle", "null_out", "batch_minus1", "budgets_empty"]),
    "mdrp_estimate_batch_prior_async": ("mono", _MONO + ["null_models", "progressive_sampling"]),
    "mdrp_estimate_batch_prior": ("mono", _MONO + ["null_x1", "null_models", "progressive_sampling"] + _BLOCKING),
    "mdrp_refine_batch_async": ("mono", _MONO + ["null_x1", "null_models"] + _STAGES),
    "mdrp_refine_batch": ("mono", _MONO + ["null_x1", "null_models"] + _STAGES + _BLOCKING),
    "mdrp_estimate_batch_ranked_async": ("mono", _MONO),
    "mdrp_estimate_batch_ranked": ("mono", _MONO + ["null_x1"] + _BLOCKING),
    "mdrp_estimate_classic_ranked_async": ("classic", _CLASSIC + _RFC),
    "mdrp_estimate_classic_ranked": ("classic", _CLASSIC + _RFC + ["null_x1"] + _BLOCKING),
    "mdrp_rank_scores": ("mono", ["null_handle"] + _SHAPE + ["null_scores", "mem_space_2", "null_out"]),
    "mdrp_refine_classic_async": ("classic", _CLASSIC + ["null_x1", "null_models"] + _STAGES),
    "mdrp_refine_classic": ("classic", _CLASSIC + ["null_x1", "null_models"] + _STAGES + _BLOCKING),
    "mdrp_estimate_classic_prior_async": ("classic", _CLASSIC + ["null_x1", "null_models", "prior_space_2", "progressive_sampling"] + _RFC),
    "mdrp_estimate_classic_prior": ("classic", _CLASSIC + ["null_x1", "null_models", "prior_space_2", "progressive_sampling"] + _RFC + _BLOCKING),
}
for _stem in ("matches", "image_pairs"):
    ENTRIES[f"mdrp_gather_{_stem}"] = ("mono", ["null_handle", "batch_minus1", "null_x1", "null_d1"] + _DESC)
    ENTRIES[f"mdrp_gather_{_stem}_ranked"] = ("mono", ["null_handle", "batch_minus1", "null_x1", "null_d1", "score_type_7"] + _DESC)
    ENTRIES[f"mdrp_estimate_{_stem}_async"] = ("mono", _FE_MONO + ["progressive_sampling"])
    ENTRIES[f"mdrp_estimate_{_stem}_ranked_async"] = ("mono", _FE_MONO + ["score_type_7"])
    ENTRIES[f"mdrp_gather_point_{_stem}"] = ("classic", ["null_handle", "batch_minus1", "null_x1"] + _POINT_DESC)
    ENTRIES[f"mdrp_gather_point_{_stem}_ranked"] = ("classic", ["null_handle", "batch_minus1", "null_x1", "score_type_7"] + _POINT_DESC)
    ENTRIES[f"mdrp_estimate_classic_{_stem}_async"] = ("classic", _FE_CLASSIC + ["progressive_sampling"])
    ENTRIES[f"mdrp_estimate_classic_{_stem}_ranked_async"] = ("classic", _FE_CLASSIC + ["score_type_7"])

# one entry point of each family: every pair of its defects that do not change the same argument
PAIRED = ("mdrp_estimate_batch", "mdrp_estimate_batch_budgets", "mdrp_estimate_batch_prior", "mdrp_refine_batch", "mdrp_estimate_batch_ranked",
          "mdrp_estimate_classic_ranked", "mdrp_rank_scores", "mdrp_refine_classic", "mdrp_estimate_classic_prior", "mdrp_gather_matches_ranked",
          "mdrp_estimate_image_pairs_ranked_async", "mdrp_gather_point_image_pairs_ranked", "mdrp_estimate_classic_matches_ranked_async")


# ------------------------------------------------------------------------------------------------------------------------------ the valid call
class Base:
    """the arguments of the valid call, by name, for both families; blocking entry points take the host arrays (mem = MDRP_MEM_HOST)"""

    def __init__(self, capi, handle):
        import torch
        dev = torch.device("cuda", 0)
        rng = np.random.default_rng(5)
        self.capi, self.keep = capi, []
        host = {"x1": rng.uniform(-200, 200, (B, N, 2)), "x2": rng.uniform(-200, 200, (B, N, 2)), "d1": rng.uniform(1, 3, (B, N)), "d2": rng.uniform(1, 3, (B, N)),
                "scores": rng.uniform(0, 1, (B, N)), "models": np.zeros(B, dtype=capi.MODEL_DTYPE)}
        host["models"]["q"][:, 0] = 1.0
        host["models"]["scale"] = host["models"]["f1"] = host["models"]["f2"] = 1.0
        self.host = dict(host, mask=np.zeros((B, N), np.uint8), bmask=np.zeros((len(BUDGETS), B, N), np.uint8), iscore=np.zeros(B), iinl=np.zeros(B, np.int32),
                         order=np.zeros((B, N), np.int32))
        self.dev = {k: torch.from_numpy(v.view(np.uint8) if v.dtype.fields else v).to(dev) for k, v in self.host.items()}
        cam = np.zeros(B, dtype=capi.CAMERA_DTYPE)
        cam["params"][:, 0] = 500.0
        kp = rng.uniform(1, MAP - 1, (IMAGES, N, 2)).astype(np.float32)
        matches = np.repeat(np.arange(N, dtype=np.int32)[None, :, None], B, 0).repeat(2, 2)
        fe = {"kp": kp, "depth": np.full((IMAGES, MAP, MAP), 2.0, np.float32), "matches": matches, "pairs": np.array([[0, 1], [1, 2]], np.int32),
              "fscores": rng.uniform(0, 1, (B, N)), "x1": np.zeros((B, N, 2)), "x2": np.zeros((B, N, 2)), "d1": np.zeros((B, N)), "d2": np.zeros((B, N)),
              "slot": np.zeros((B, N), np.int32), "mmask": np.zeros((B, N), np.uint8)}
        t = self.fe = {k: torch.from_numpy(v).to(dev) for k, v in fe.items()}
        torch.cuda.synchronize()
        p = lambda x: x.data_ptr()
        descs = {
            "mdrp_matches": capi.Matches(p(t["kp"]), p(t["kp"][1:]), capi.F32, N, N, p(t["matches"]), N, p(t["depth"]), p(t["depth"][1:]), capi.F32, MAP, MAP, MAP, MAP, None,
                                         None, 0),
            "mdrp_image_pairs": capi.ImagePairs(p(t["kp"]), capi.F32, N, None, p(t["depth"]), capi.F32, MAP, MAP, None, None, IMAGES, p(t["pairs"]), p(t["matches"]), N, 0),
            "mdrp_point_matches": capi.PointMatches(p(t["kp"]), p(t["kp"][1:]), capi.F32, N, N, p(t["matches"]), N, None, None),
            "mdrp_point_image_pairs": capi.PointImagePairs(p(t["kp"]), capi.F32, N, None, None, IMAGES, p(t["pairs"]), p(t["matches"]), N)}
        ropt = capi.ransac_opt_from_dict({"max_iterations": BUDGETS[-1], "min_iterations": BUDGETS[-1], "seed": 1})
        self.common = dict(h=handle, batch=B, n_max=N, npp=np.full(B, N, np.int32), cam1=cam, cam2=cam.copy(), ropt=ropt, bopt=capi.bundle_opt_from_dict({}),
                           out=np.zeros(B, capi.RESULT_DTYPE), bout=np.zeros((len(BUDGETS), B), capi.RESULT_DTYPE), budgets=np.array(BUDGETS, np.uint64),
                           n_budgets=len(BUDGETS), stages=3, prior_space=0, score_type=capi.F64, n_host=np.zeros(B, np.int32), n_used=np.zeros(B, np.int32))
        self.descs = descs

    def args(self, entry):
        family = ENTRIES[entry][0]
        names = SIGNATURES[entry].split()
        a = dict(self.common, kind=0 if family == "mono" else 3)
        if "desc" in names:  # the front end: device memory throughout
            a.update(self.fe)
            stem = "image_pairs" if "image_pairs" in entry else "matches"
            a["desc"] = self.descs[("mdrp_point_" if family == "classic" else "mdrp_") + stem]
        elif "mem" in names:
            a.update(self.host, mem=self.capi.MEM_HOST)
        else:
            a.update(self.dev)
            if "copy_" in entry:
                a.update(out=self.dev["mask"], bout=self.dev["bmask"])  # (never written: every probe is refused)
        return a, names


def marshal(v):
    if v is None or isinstance(v, (int, C.c_void_p)):
        return v
    if isinstance(v, C.Structure):
        return C.byref(v)
    if isinstance(v, np.ndarray):
        return C.c_void_p(v.ctypes.data)
    return C.c_void_p(v.data_ptr())  # a torch tensor


def probes():
    """[(entry point, (defect, ...))]: every single defect of every entry point, then the pairs of the PAIRED ones"""
    out = [(e, (d,)) for e, (_, ds) in ENTRIES.items() for d in ds]
    for e in PAIRED:
        touched = {}
        for d in ENTRIES[e][1]:
            probe = {k: object() for k in SIGNATURES[e].split()}
            probe.update(ropt=_Dummy(), desc=_Dummy(), kind=_Kind(0 if ENTRIES[e][0] == "mono" else 3))
            before = dict(probe)
            DEFECTS[d](probe)
            touched[d] = {k for k in before if probe[k] is not before[k]}
        out += [(e, (a, b)) for a, b in itertools.combinations(ENTRIES[e][1], 2) if not touched[a] & touched[b]]
    return out


class _Kind(int):
    """an int that is no other int's object: any assignment to `kind` shows"""


class _Dummy(C.Structure):
    _fields_ = [("progressive_sampling", C.c_int32), ("real_focal_check", C.c_int32), ("kp_type", C.c_int32), ("filter", C.c_int32), ("m_max", C.c_int32),
                ("matches", C.c_void_p)]


def run_table(lib, base):
    """{entry point: {"defect" | "defect+defect": [return code, message]}} of the library `lib` (mdrp_amd._capi.load_library())"""
    table = {}
    for entry, defects in probes():
        a, names = base.args(entry)
        for d in defects:
            DEFECTS[d](a)
        rc = getattr(lib, entry)(*[marshal(a[n]) for n in names])
        table.setdefault(entry, {})["+".join(defects)] = [int(rc), lib.mdrp_last_error().decode(errors="replace")]
    return table
