"""The calls mdrp_amd/_capi.py makes into the library, case by case, for tests/test_binding_calls_host.py and tests/tools/gen_golden_binding.py.

A Handle is built without a device (Handle.__new__) around a Stub that answers every mdrp_* symbol with a function which records its name and its
normalised arguments and returns 0.  Normalised: ints and floats as they are; None and a null pointer alike (None); a pointer whose value is an
integer the case handed in, that integer (a device pointer); a pointer to an array the case owns, "array:<name>" (the case passes it contiguous and
in its final dtype, so the binding hands the same buffer on); any other pointer "host"; a byref struct without pointer fields as its bytes, one with
pointer fields field by field (the addresses in it normalised the same way: its bytes would differ from run to run); a byref scalar as "out:<type>".
Return values are pinned as shapes, dtypes and contents (the stub writes nothing, so the contents are what the binding filled in).
"""
import contextlib
import ctypes as C
import hashlib
import inspect

import numpy as np

from mdrp_amd import _capi

B, N = 2, 4
_DEV0 = 0xD0000000
_BYREF = type(C.byref(C.c_int()))


class Env:
    """what one case owns: named host arrays and device-pointer integers"""

    def __init__(self):
        self.arrays, self.ints = {}, set()

    def arr(self, name, a):
        assert isinstance(a, np.ndarray) and a.flags.c_contiguous and a.size, name
        self.arrays[name] = a
        return a

    def dev(self, k):
        self.ints.add(_DEV0 + 0x1000 * k)
        return _DEV0 + 0x1000 * k

    def pointer(self, value):
        if not value:
            return None
        if value in self.ints:
            return value
        for name, a in self.arrays.items():
            if a.ctypes.data == value:
                return "array:" + name
        return "host"

    def struct(self, s):
        if not any(t is C.c_void_p for _, t in s._fields_):
            return {"struct": type(s).__name__, "bytes": bytes(s).hex()}
        fields = {}
        for f, t in s._fields_:
            v = getattr(s, f)
            fields[f] = self.pointer(v) if t is C.c_void_p else v
        return {"struct": type(s).__name__, "fields": fields}

    def norm(self, a):
        if a is None or (isinstance(a, (int, float)) and not isinstance(a, bool)):
            return a
        if isinstance(a, C.c_void_p):
            return self.pointer(a.value)
        if isinstance(a, _BYREF):
            return self.struct(a._obj) if isinstance(a._obj, C.Structure) else "out:" + type(a._obj).__name__
        raise TypeError(f"an argument the recorder does not know: {a!r}")


class Stub:
    """stands in for the loaded library: every mdrp_* attribute except `missing` is a recording function"""

    def __init__(self, missing=()):
        self.calls, self.env, self._missing = [], Env(), frozenset(missing)

    def __getattr__(self, name):
        if not name.startswith("mdrp_") or name in self._missing:
            raise AttributeError(name)

        def fn(*args):
            self.calls.append([name, [self.env.norm(a) for a in args]])
            return 0
        return fn


@contextlib.contextmanager
def handle(stub):
    """a Handle on `stub` that never saw a device; load_library() answers with the stub meanwhile (solver_residency)"""
    h = _capi.Handle.__new__(_capi.Handle)
    h._lib, h._h, h.device, h.stream = stub, C.c_void_p(0x1000), 0, None
    saved, _capi._lib = _capi._lib, stub
    try:
        yield h
    finally:
        _capi._lib = saved
        h._h = None  # (close() then does nothing)


def returned(v):
    if isinstance(v, np.ndarray):
        out = {"shape": list(v.shape), "dtype": str(v.dtype), "sha256": hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16]}
        if v.dtype.kind in "iuf" and v.size <= 64:
            out["values"] = v.tolist()
        return out
    if isinstance(v, (tuple, list)):
        return [returned(x) for x in v]
    if isinstance(v, dict):
        return {k: returned(x) for k, x in v.items()}
    if isinstance(v, (np.integer, np.floating)):
        return v.item()
    assert v is None or isinstance(v, (int, float, str)), v
    return v


# ---------------------------------------------------------------------------------------------------- what the cases are made of
def opts():
    return _capi.ransac_opt_from_dict({"seed": 7, "max_iterations": 50}), _capi.bundle_opt_from_dict({"loss_type": "TRUNCATED"})


def points(env):
    x1 = env.arr("x1", np.arange(B * N * 2, dtype=np.float64).reshape(B, N, 2))
    return x1, env.arr("x2", x1 + 100.0)


def depths(env):
    return env.arr("d1", np.full((B, N), 2.0)), env.arr("d2", np.full((B, N), 3.0))


def models(env, name="models", dtype=None):
    m = np.zeros(B, dtype=dtype or _capi.MODEL_DTYPE)
    (m["model"] if dtype is _capi.RESULT_DTYPE else m)["q"][:, 0] = 1.0
    return env.arr(name, m)


def tables(env):
    """ragged n_per_pair and the two camera tables"""
    cams = np.zeros((2, B), dtype=_capi.CAMERA_DTYPE)
    cams["params"][..., 0] = 800.0
    return {"n_per_pair": env.arr("npp", np.array([N, N - 1], dtype=np.int32)), "cam1": env.arr("cam1", cams[0].copy()), "cam2": env.arr("cam2", cams[1].copy())}


def cameras(env):
    t = tables(env)
    return {"cam1": t["cam1"], "cam2": t["cam2"]}


def scores(env):
    return env.arr("scores", np.arange(B * N, dtype=np.float64).reshape(B, N))


def matches(env, point=False):
    if point:
        return _capi.PointMatches(env.dev(1), env.dev(2), _capi.F32, 9, 8, env.dev(3), N, env.dev(6), None)
    return _capi.Matches(env.dev(1), env.dev(2), _capi.F32, 9, 8, env.dev(3), N, env.dev(4), env.dev(5), _capi.F64, 12, 16, 10, 14, env.dev(6), None,
                         _capi.FILTERS["finite"])


def image_pairs(env, point=False):
    if point:
        return _capi.PointImagePairs(env.dev(1), _capi.F64, 9, None, env.dev(6), 3, env.dev(7), env.dev(3), N)
    return _capi.ImagePairs(env.dev(1), _capi.F64, 9, env.dev(2), env.dev(4), _capi.F32, 12, 16, None, env.dev(6), 3, env.dev(7), env.dev(3), N,
                            _capi.FILTERS["both_inf"])


def dense(env):
    return _capi.DenseMatches(env.dev(1), _capi.F32, 64, env.dev(2), _capi.F32, _capi.DENSE_COORDS["pixel"], env.dev(4), env.dev(5), _capi.F32, 12, 16, 10, 14,
                              _capi.FILTERS["both_inf"], None, env.dev(6), N, 1, 4, 8, 2, 1, 11, 0.05, env.dev(8), None)


CASES = []  # (id, Handle method or "module:<function>", build(env) -> (args, kwargs))


def case(cid, method=None):
    def deco(build):
        CASES.append((cid, method or cid.split("[")[0], build))
        return build
    return deco


def _both(method, required, optional):
    """two cases of a *_device method: every optional pointer absent, every optional pointer present"""
    case(f"{method}[absent]", method)(lambda env: (required(env), {}))
    case(f"{method}[present]", method)(lambda env: (required(env), optional(env)))


# ---------------------------------------------------------------------------------------------------- the handle itself
case("synchronize")(lambda env: ((), {}))
case("close")(lambda env: ((), {}))
case("fetch_results")(lambda env: ((B,), {}))
case("copy_results_device")(lambda env: ((env.dev(20), B), {}))
case("last_sweep_stats")(lambda env: ((), {}))
case("last_stats")(lambda env: ((), {}))
case("solver_residency", "module:solver_residency")(lambda env: ((_capi.SOLVER_SHIFT, 2), {"keep_free_bytes": 4096, "device": 1}))

# ---------------------------------------------------------------------------------------------------- host estimators
for kind in (_capi.CALIB, _capi.RELPOSE_5PT):  # (the depth policy: a baseline takes none)
    case(f"estimate_batch[kind{kind}]")(lambda env, kind=kind: ((kind, *points(env), *depths(env), *opts()), {}))
    case(f"estimate_batch_budgets[kind{kind}]")(lambda env, kind=kind: ((kind, *points(env), *depths(env), *opts(), env.arr("ks", np.array([10, 50], np.uint64))), {}))
case("estimate_batch[tables]")(lambda env: ((_capi.CALIB, *points(env), *depths(env), *opts()), {**tables(env), "want_mask": False}))
case("estimate_batch[no depths]")(lambda env: ((_capi.SHARED_6PT, *points(env), None, None, *opts()), cameras(env)))
case("estimate_batch_budgets[tables]")(lambda env: ((_capi.SHARED_FOCAL, *points(env), *depths(env), *opts(), [10, 20, 50]), {**tables(env), "want_mask": False}))
case("refine_batch")(lambda env: ((_capi.CALIB, *points(env), *depths(env), models(env), *opts()), {}))
case("refine_batch[tables]")(lambda env: ((_capi.CALIB, *points(env), *depths(env), None, *opts()), {"stages": _capi.STAGE_LO, **tables(env), "want_mask": False}))
case("estimate_batch_prior")(lambda env: ((_capi.CALIB, *points(env), *depths(env), models(env, "priors"), *opts()), {}))
case("estimate_batch_prior[no depths]")(lambda env: ((_capi.RELPOSE_5PT, *points(env), None, None, None, *opts()), {**tables(env), "want_mask": False}))
case("estimate_batch_prior[one depth]")(lambda env: ((_capi.CALIB, *points(env), depths(env)[0], None, None, *opts()), {}))
case("estimate_batch_ranked")(lambda env: ((_capi.CALIB, *points(env), *depths(env), scores(env), *opts()), {}))
case("estimate_batch_ranked[no depths]")(lambda env: ((_capi.FUNDAMENTAL_7PT, *points(env), None, None, None, *opts()), {**tables(env), "want_mask": False}))
case("estimate_classic_ranked")(lambda env: ((_capi.RELPOSE_5PT, *points(env), scores(env), *opts()), {}))
case("estimate_classic_ranked[tables]")(lambda env: ((_capi.SHARED_6PT, *points(env), None, *opts()), {**tables(env), "want_mask": False}))
case("refine_classic")(lambda env: ((_capi.RELPOSE_5PT, *points(env), models(env), *opts()), {}))
case("refine_classic[tables]")(lambda env: ((_capi.FUNDAMENTAL_7PT, *points(env), None, *opts()), {"stages": 0, **tables(env), "want_mask": False}))
case("estimate_classic_prior")(lambda env: ((_capi.RELPOSE_5PT, *points(env), models(env, "priors"), *opts()), {}))
case("estimate_classic_prior[tables]")(lambda env: ((_capi.SHARED_6PT, *points(env), None, *opts()), {**tables(env), "want_mask": False, "prior_space": 1}))
case("prosac_samples")(lambda env: ((3, 40, 1000, env.arr("lens", np.array([2, 3], np.int32))), {"fill": 9}))
case("prosac_samples_k")(lambda env: ((3, 40, 5, 1000, [2, 3]), {}))
case("rank_scores")(lambda env: ((scores(env),), {}))
case("rank_scores[ragged]")(lambda env: ((scores(env),), {"n_per_pair": tables(env)["n_per_pair"]}))

# ---------------------------------------------------------------------------------------------------- device estimators


def _xd(env):
    return env.dev(1), env.dev(2), env.dev(3), env.dev(4)


_both("estimate_batch_device", lambda env: (_capi.CALIB, env.dev(1), env.dev(2), None, None, B, N, *opts()), lambda env: {**tables(env), "mask_ptr": env.dev(9)})
case("estimate_batch_device[depths]")(lambda env: ((_capi.SHARED_FOCAL, *_xd(env), B, N, *opts()), {"mask_ptr": env.dev(9)}))
_both("estimate_batch_budgets_device", lambda env: (_capi.CALIB, env.dev(1), env.dev(2), None, None, B, N, *opts(), [10, 50]), lambda env: {**tables(env), "mask_ptr": env.dev(9)})
case("estimate_batch_budgets_device[depths]")(lambda env: ((_capi.CALIB, *_xd(env), B, N, *opts(), env.arr("ks", np.array([5], np.uint64))), {}))
case("fetch_budget_results")(lambda env: ((3, B), {}))
case("copy_budget_results_device")(lambda env: ((env.dev(20), 3, B), {}))
_both("refine_batch_device", lambda env: (_capi.CALIB, env.dev(1), env.dev(2), None, None, B, N, None, *opts()),
      lambda env: {"stages": _capi.STAGE_INLIERS, **tables(env), "mask_ptr": env.dev(9), "initial_score_ptr": env.dev(10), "initial_inliers_ptr": env.dev(11)})
case("refine_batch_device[depths]")(lambda env: ((_capi.CALIB, *_xd(env), B, N, env.dev(5), *opts()), {}))
_both("estimate_batch_prior_device", lambda env: (_capi.CALIB, env.dev(1), env.dev(2), None, None, B, N, None, *opts()), lambda env: {**tables(env), "mask_ptr": env.dev(9)})
case("estimate_batch_prior_device[depths]")(lambda env: ((_capi.CALIB, *_xd(env), B, N, env.dev(5), *opts()), {}))
_both("estimate_batch_ranked_device", lambda env: (_capi.CALIB, env.dev(1), env.dev(2), None, None, None, B, N, *opts()), lambda env: {**tables(env), "mask_ptr": env.dev(9)})
case("estimate_batch_ranked_device[depths]")(lambda env: ((_capi.CALIB, *_xd(env), env.dev(5), B, N, *opts()), {}))
_both("estimate_classic_ranked_device", lambda env: (_capi.RELPOSE_5PT, env.dev(1), env.dev(2), None, B, N, *opts()), lambda env: {**tables(env), "mask_ptr": env.dev(9)})
case("estimate_classic_ranked_device[scores]")(lambda env: ((_capi.RELPOSE_5PT, env.dev(1), env.dev(2), env.dev(5), B, N, *opts()), {}))
_both("refine_classic_device", lambda env: (_capi.RELPOSE_5PT, env.dev(1), env.dev(2), B, N, None, *opts()),
      lambda env: {"stages": 0, **tables(env), "mask_ptr": env.dev(9), "initial_score_ptr": env.dev(10), "initial_inliers_ptr": env.dev(11)})
case("refine_classic_device[models]")(lambda env: ((_capi.RELPOSE_5PT, env.dev(1), env.dev(2), B, N, env.dev(5), *opts()), {}))
_both("estimate_classic_prior_device", lambda env: (_capi.SHARED_6PT, env.dev(1), env.dev(2), B, N, None, *opts()),
      lambda env: {**tables(env), "mask_ptr": env.dev(9), "prior_space": 1})
case("estimate_classic_prior_device[priors]")(lambda env: ((_capi.SHARED_6PT, env.dev(1), env.dev(2), B, N, env.dev(5), *opts()), {}))
_both("rank_scores_device", lambda env: (env.dev(1), B, N, env.dev(2)), lambda env: {"n_per_pair": tables(env)["n_per_pair"]})
case("score_models_device")(lambda env: ((_capi.CALIB, env.dev(1), 5, env.dev(2), env.dev(3), N, 2.25, env.dev(4), env.dev(5)), {}))

# ---------------------------------------------------------------------------------------------------- device front ends
_out5 = lambda env: (B, env.dev(11), env.dev(12), env.dev(13), env.dev(14), env.dev(15))  # noqa: E731
for stem, desc in (("matches", matches), ("image_pairs", image_pairs)):
    case(f"gather_{stem}")(lambda env, desc=desc: ((desc(env), *_out5(env)), {}))
    case(f"gather_{stem}_ranked[absent]", f"gather_{stem}_ranked")(lambda env, desc=desc: ((desc(env), None, _capi.F64, *_out5(env)), {}))
    case(f"gather_{stem}_ranked[present]", f"gather_{stem}_ranked")(lambda env, desc=desc: ((desc(env), env.dev(16), _capi.F32, *_out5(env)), {}))
    _both(f"estimate_{stem}_device", lambda env, desc=desc: (_capi.CALIB, desc(env), B, *opts()), lambda env: {**cameras(env), "match_mask_ptr": env.dev(9)})
    _both(f"estimate_{stem}_ranked_device", lambda env, desc=desc: (_capi.CALIB, desc(env), None, _capi.F64, B, *opts()), lambda env: {**cameras(env), "match_mask_ptr": env.dev(9)})
    case(f"estimate_{stem}_ranked_device[scores]", f"estimate_{stem}_ranked_device")(lambda env, desc=desc: ((_capi.SHARED_FOCAL, desc(env), env.dev(16), _capi.F32, B, *opts()), {}))
    for ranked in (False, True):
        case(f"gather_points[{stem}, ranked={ranked}, absent]", "gather_points")(
            lambda env, desc=desc, ranked=ranked: ((desc(env, True), B, env.dev(11), env.dev(12), env.dev(15)), {"ranked": ranked}))
        case(f"gather_points[{stem}, ranked={ranked}, present]", "gather_points")(
            lambda env, desc=desc, ranked=ranked: ((desc(env, True), B, env.dev(11), env.dev(12), env.dev(15)), {"scores_ptr": env.dev(16), "score_type": _capi.F32, "ranked": ranked}))
        case(f"estimate_points_device[{stem}, ranked={ranked}, absent]", "estimate_points_device")(
            lambda env, desc=desc, ranked=ranked: ((_capi.RELPOSE_5PT, desc(env, True), B, *opts()), {"ranked": ranked}))
        case(f"estimate_points_device[{stem}, ranked={ranked}, present]", "estimate_points_device")(
            lambda env, desc=desc, ranked=ranked: ((_capi.RELPOSE_5PT, desc(env, True), B, *opts()),
                                                   {**cameras(env), "match_mask_ptr": env.dev(9), "scores_ptr": env.dev(16), "score_type": _capi.F32, "ranked": ranked}))
case("sample_dense[absent]", "sample_dense")(lambda env: ((dense(env), B, None, None, None, None, None, None), {}))
case("sample_dense[present]", "sample_dense")(lambda env: ((dense(env), *_out5(env), env.dev(16)), {}))
_both("estimate_dense_device", lambda env: (_capi.CALIB, dense(env), B, *opts()), lambda env: {**cameras(env), "record_mask_ptr": env.dev(9)})

# ---------------------------------------------------------------------------------------------------- focals and pose from F
case("focals_from_fundamental")(lambda env: ((env.arr("F", np.arange(B * 9, dtype=np.float64).reshape(B, 9)),), {}))
case("focals_from_fundamental[pp]")(lambda env: ((np.ones((B, 3, 3)), env.arr("pp1", np.ones((B, 2))), env.arr("pp2", np.zeros((B, 2)) + 2.0)), {}))
case("focals_from_fundamental_device[absent]")(lambda env: ((env.dev(1), None, None, B, env.dev(2)), {}))
case("focals_from_fundamental_device[present]")(lambda env: ((env.dev(1), env.dev(3), env.dev(4), B, env.dev(2)), {}))
case("pose_from_fundamental")(lambda env: ((*points(env), models(env)), {}))
case("pose_from_fundamental[results]")(lambda env: ((*points(env), models(env, dtype=_capi.RESULT_DTYPE)),
                                                    {"n_per_pair": tables(env)["n_per_pair"], "mask": env.arr("mask", np.ones((B, N), np.uint8)),
                                                     "pp1": env.arr("pp1", np.ones((B, 2))), "pp2": env.arr("pp2", np.zeros((B, 2)) + 2.0)}))
_pose_dev = lambda env: (env.dev(1), env.dev(2), B, N, env.dev(3), 136, env.dev(4))  # noqa: E731
_pose_opt = lambda env: {"n_per_pair": tables(env)["n_per_pair"], "mask_ptr": env.dev(9), "pp1_ptr": env.dev(5), "pp2_ptr": env.dev(6)}  # noqa: E731
_both("pose_from_fundamental_device", _pose_dev, _pose_opt)
case("pose_from_fundamental_device[blocking, absent]")(lambda env: (_pose_dev(env), {"blocking_out": env.arr("out", np.zeros(B, _capi.FOCAL_POSE_DTYPE))}))
case("pose_from_fundamental_device[blocking, present]")(lambda env: (_pose_dev(env), {**_pose_opt(env), "blocking_out": env.arr("out", np.zeros(B, _capi.FOCAL_POSE_DTYPE))}))
_both("estimate_fundamental_focals_device", lambda env: (env.dev(1), env.dev(2), B, N, *opts(), env.dev(4)), _pose_opt)

# ---------------------------------------------------------------------------------------------------- unit-parity entry points
_one_pair = lambda env: (models(env), env.arr("x1", np.arange(N * 2, dtype=np.float64).reshape(N, 2)), env.arr("x2", np.ones((N, 2))))  # noqa: E731
case("solver_batch")(lambda env: ((_capi.SOLVER_P3P, env.arr("x1h", np.ones((B, 3, 3))), env.arr("x2h", np.zeros((B, 3, 3)) + 2.0), env.arr("d1", np.ones((B, 3))),
                                   env.arr("d2", np.ones((B, 3)) * 2.0)), {}))
case("classic_solver_batch")(lambda env: ((_capi.SHARED_6PT, env.arr("x1h", np.ones((B, 6, 3))), env.arr("x2h", np.zeros((B, 6, 3)) + 2.0)), {}))
case("score_models")(lambda env: ((_capi.CALIB, *_one_pair(env), 2.25), {}))
case("count_candidates")(lambda env: ((_capi.CALIB, *_one_pair(env), 2.25), {}))
case("bound_models")(lambda env: ((_capi.CALIB, *_one_pair(env), 2.25), {}))
case("retire_models")(lambda env: ((_capi.CALIB, *_one_pair(env), 2.25, 3, None), {}))
case("retire_models[record]")(lambda env: ((_capi.CALIB, *_one_pair(env), 2.25, 3, 1.5), {"cand_stat": (5, 6), "flags": _capi.RETIRE_TWO_PHASE | _capi.RETIRE_BOUND}))
case("front_models")(lambda env: ((_capi.CALIB, *_one_pair(env), 2.25, 8), {}))
case("front_models[record]")(lambda env: ((_capi.CALIB, *_one_pair(env), 2.25, 8), {"rec_cnt": 3, "rec_score": 1.5}))
case("refine_models")(lambda env: ((_capi.CALIB, models(env), np.ones((N, 2)), np.ones((N, 2)), None, None, 1.0, 0.5, opts()[1]), {}))
case("refine_models[depths]")(lambda env: ((_capi.CALIB, models(env), env.arr("x1", np.ones((N, 2))), env.arr("x2", np.ones((N, 2)) * 2.0), env.arr("d1", np.ones(N)),
                                            env.arr("d2", np.ones(N) * 2.0), 1.0, 0.5, opts()[1]), {"estimate_shift": True}))


def _replay(env, budgets):
    slots = 3 * 2  # three hypotheses in all, two models per sample
    tabs = [env.arr(n, np.zeros((B, slots), dtype=dt)) for n, dt in (("slot_score", np.float64), ("slot_inl", np.int32), ("models", _capi.MODEL_DTYPE),
                                                                        ("lo_score", np.float64), ("lo_cnt", np.int32), ("lo_models", _capi.MODEL_DTYPE))]
    kw = {} if budgets is None else {"budgets": env.arr("budgets", np.array(budgets, np.uint64))}
    return (2, 3, 64, env.arr("lens", np.array([1, 2], np.int32)), opts()[0], np.zeros(B, _capi.REPLAY_STATE_DTYPE), *tabs), kw


case("replay_slots")(lambda env: _replay(env, None))
case("replay_slots[budgets]")(lambda env: _replay(env, [10, 50]))
_front = lambda env: ([N, N], [1.0, 2.0], [1, 0], [np.array([1, 2], np.uint32), np.array([3], np.uint32)], 2, env.arr("slot_score", np.ones((B, 3))),  # noqa: E731
                      env.arr("slot_inl", np.ones((B, 3), np.int32)))
case("front_lists")(lambda env: (_front(env), {}))
case("front_lists[fill]")(lambda env: (_front(env), {"fill": {"tags_pick": 7, "rest_count": -1}}))
case("front_stages")(lambda env: ((_capi.CALIB, *points(env), *depths(env), *opts(), env.arr("lens", np.array([2, 3], np.int32))), tables(env)))
case("front_stages[no depths]")(lambda env: ((_capi.SHARED_6PT, *points(env), None, None, *opts(), [4]), {"cam1": cameras(env)["cam1"], "slot_iters": 6}))

# ---------------------------------------------------------------------------------------------------- refusals that need no library
REFUSALS = []  # (id, Handle method, build(env) -> (args, kwargs)): the exception's type and message are pinned, and that nothing was called


def refusal(cid, method, build):
    REFUSALS.append((cid, method, build))


_bad_x = lambda env: (np.zeros((B, N, 3)), np.zeros((B, N, 3)))  # noqa: E731
_bad_d = lambda env: (np.zeros((B, N + 1)), np.zeros((B, N + 1)))  # noqa: E731
_three = lambda env: np.zeros(B + 1, _capi.MODEL_DTYPE)  # noqa: E731
refusal("estimate_batch[x]", "estimate_batch", lambda env: ((0, *_bad_x(env), *depths(env), *opts()), {}))
refusal("estimate_batch[d]", "estimate_batch", lambda env: ((0, *points(env), *_bad_d(env), *opts()), {}))
refusal("estimate_batch[d None]", "estimate_batch", lambda env: ((0, *points(env), None, None, *opts()), {}))
refusal("estimate_batch[d2]", "estimate_batch", lambda env: ((2, *points(env), depths(env)[0], np.zeros((B, N, 1)), *opts()), {}))
refusal("estimate_batch_budgets[x]", "estimate_batch_budgets", lambda env: ((0, *_bad_x(env), *depths(env), *opts(), [5]), {}))
refusal("estimate_batch_budgets[d]", "estimate_batch_budgets", lambda env: ((0, *points(env), *_bad_d(env), *opts(), [5]), {}))
refusal("estimate_batch_budgets[d None]", "estimate_batch_budgets", lambda env: ((1, *points(env), None, None, *opts(), [5]), {}))
refusal("refine_batch[x]", "refine_batch", lambda env: ((0, *_bad_x(env), *depths(env), models(env), *opts()), {}))
refusal("refine_batch[d]", "refine_batch", lambda env: ((0, *points(env), *_bad_d(env), models(env), *opts()), {}))
refusal("refine_batch[d None, baseline]", "refine_batch", lambda env: ((3, *points(env), None, None, models(env), *opts()), {}))
refusal("refine_batch[models]", "refine_batch", lambda env: ((0, *points(env), *depths(env), _three(env), *opts()), {}))
refusal("estimate_batch_prior[x]", "estimate_batch_prior", lambda env: ((0, *_bad_x(env), *depths(env), models(env), *opts()), {}))
refusal("estimate_batch_prior[d]", "estimate_batch_prior", lambda env: ((0, *points(env), *_bad_d(env), models(env), *opts()), {}))
refusal("estimate_batch_prior[priors]", "estimate_batch_prior", lambda env: ((0, *points(env), *depths(env), _three(env), *opts()), {}))
refusal("estimate_batch_ranked[x]", "estimate_batch_ranked", lambda env: ((0, *_bad_x(env), *depths(env), scores(env), *opts()), {}))
refusal("estimate_batch_ranked[d]", "estimate_batch_ranked", lambda env: ((0, *points(env), *_bad_d(env), scores(env), *opts()), {}))
refusal("estimate_batch_ranked[scores]", "estimate_batch_ranked", lambda env: ((0, *points(env), *depths(env), np.zeros((B, N + 1)), *opts()), {}))
refusal("estimate_classic_ranked[x]", "estimate_classic_ranked", lambda env: ((3, *_bad_x(env), scores(env), *opts()), {}))
refusal("estimate_classic_ranked[scores]", "estimate_classic_ranked", lambda env: ((3, *points(env), np.zeros(B * N), *opts()), {}))
refusal("refine_classic[x]", "refine_classic", lambda env: ((3, *_bad_x(env), models(env), *opts()), {}))
refusal("refine_classic[models]", "refine_classic", lambda env: ((3, *points(env), _three(env), *opts()), {}))
refusal("estimate_classic_prior[x]", "estimate_classic_prior", lambda env: ((3, *_bad_x(env), models(env), *opts()), {}))
refusal("estimate_classic_prior[priors]", "estimate_classic_prior", lambda env: ((3, *points(env), _three(env), *opts()), {}))
refusal("pose_from_fundamental[x]", "pose_from_fundamental", lambda env: ((*_bad_x(env), models(env)), {}))
refusal("pose_from_fundamental[models]", "pose_from_fundamental", lambda env: ((*points(env), _three(env)), {}))
refusal("pose_from_fundamental[dtype]", "pose_from_fundamental", lambda env: ((*points(env), np.zeros((B, 12))), {}))
refusal("replay_slots[table]", "replay_slots", lambda env: ((lambda a, kw: ((*a[:7], np.zeros((B, 5), np.int32), *a[8:]), kw))(*_replay(env, None))))
refusal("front_lists[tables]", "front_lists", lambda env: ((*_front(env)[:5], np.ones((B, 4)), np.ones((B, 3), np.int32)), {}))
refusal("front_lists[long list]", "front_lists", lambda env: ((*_front(env)[:3], [np.arange(4, dtype=np.uint32), np.array([3], np.uint32)], *_front(env)[4:]), {}))

# a symbol the library lacks -> the case whose call needs it (one per family of entry points): MdrpError naming the library and the symbol
MISSING = {"mdrp_estimate_batch_budgets": "estimate_batch_budgets[kind0]", "mdrp_copy_budget_results_device": "copy_budget_results_device",
           "mdrp_refine_batch_async": "refine_batch_device[absent]", "mdrp_estimate_batch_prior": "estimate_batch_prior",
           "mdrp_rank_scores": "rank_scores", "mdrp_prosac_samples_k": "prosac_samples_k", "mdrp_refine_classic": "refine_classic",
           "mdrp_estimate_image_pairs_async": "estimate_image_pairs_device[absent]", "mdrp_gather_matches_ranked": "gather_matches_ranked[absent]",
           "mdrp_gather_point_image_pairs_ranked": "gather_points[image_pairs, ranked=True, absent]", "mdrp_pose_from_fundamental": "pose_from_fundamental",
           "mdrp_estimate_dense_async": "estimate_dense_device[absent]", "mdrp_retire_models": "retire_models", "mdrp_replay_slots": "replay_slots",
           "mdrp_front_lists": "front_lists", "mdrp_front_models": "front_models", "mdrp_front_stages": "front_stages", "mdrp_solver_residency": "solver_residency"}


# ---------------------------------------------------------------------------------------------------- running them
def _invoke(h, method, build, env):
    args, kwargs = build(env)
    fn = getattr(_capi, method[7:]) if method.startswith("module:") else getattr(h, method)
    return fn(*args, **kwargs)


def run_case(cid, missing=()):
    """{"calls": [[symbol, arguments], ...], "returns": ...} of one case"""
    _, method, build = next(c for c in CASES if c[0] == cid)
    stub = Stub(missing)
    with handle(stub) as h:
        out = returned(_invoke(h, method, build, stub.env))
    return {"calls": stub.calls, "returns": out}


def _raised(e):
    return {"type": type(e).__name__, "message": str(e).replace(_capi.LIB_PATH, "<library>")}


def run_refusal(cid):
    _, method, build = next(c for c in REFUSALS if c[0] == cid)
    stub = Stub()
    with handle(stub) as h:
        try:
            _invoke(h, method, build, stub.env)
        except Exception as e:  # noqa: BLE001 (the type is what is pinned)
            assert not stub.calls, stub.calls
            return _raised(e)
    raise AssertionError(f"{cid}: nothing was raised")


def run_missing(symbol):
    try:
        run_case(MISSING[symbol], missing=(symbol,))
    except Exception as e:  # noqa: BLE001
        return _raised(e)
    raise AssertionError(f"{symbol}: nothing was raised")


def signatures(module):
    """{qualified name: str(inspect.signature)} of the public functions of a module and the public methods (and __init__) of its classes"""
    out = {}
    for name, obj in sorted(vars(module).items()):
        if name.startswith("_") or getattr(obj, "__module__", None) != module.__name__:
            continue
        if inspect.isfunction(obj):
            out[name] = str(inspect.signature(obj))
        elif inspect.isclass(obj):
            for m, f in sorted(vars(obj).items()):
                f = f.__func__ if isinstance(f, (staticmethod, classmethod)) else f
                if inspect.isfunction(f) and (not m.startswith("_") or m == "__init__"):
                    out[f"{name}.{m}"] = str(inspect.signature(f))
    return out


def handle_methods():
    return sorted(m for m, f in vars(_capi.Handle).items() if inspect.isfunction(f) and not m.startswith("_"))


def snapshot():
    """everything the golden file holds"""
    import mdrp_amd.poselib as poselib
    return {"calls": {cid: run_case(cid) for cid, _, _ in CASES}, "refusals": {cid: run_refusal(cid) for cid, _, _ in REFUSALS},
            "missing": {s: run_missing(s) for s in MISSING},
            "signatures": {"_capi": signatures(_capi), "poselib": signatures(poselib)}}
