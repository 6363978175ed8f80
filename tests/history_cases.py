"""The calls of tests/test_history_host.py, tests/test_gpu_history.py and tests/tools/endurance.py (a helper, not a test): one table of calls on an
mdrp handle, each with the C entry points it goes through, its shapes and a run(handle) that returns everything the call defines as byte strings.

PROBES are the calls whose result is checked: small, ragged, 70 - 85 % outliers and noisy, so that any stale "better" score, count, record or
checkpoint left in the handle's grow-only buffers by an earlier call would win.  PREDECESSORS only leave state behind: every probe, plus
  (a) each estimator probe's clean twin (same kind, shapes and correspondence counts; no outliers, no noise),
  (b) strictly larger calls, (c) one beyond each limit of the LM kernels' LDS lists, (d) a run that stops in its first super-chunk behind a long one,
  (e) calls under non-default schedule knobs, (f) a call whose fused tail gives up its bounded waits (the handle backs off), (g) refused calls,
  and one call below every probe's shapes.
Nothing here touches the GPU before run() is called; torch is imported only by the device-resident calls.  Inputs come from mdrp_amd.synth and
the builders of the other *_cases.py files."""
import functools
import os

import numpy as np

from mdrp_amd import synth

KNOBS = ("MDRP_CHUNKS", "MDRP_LO_OVERLAP", "MDRP_BOUND", "MDRP_FUSE_TAIL", "MDRP_LO_THREADS", "MDRP_FINAL_THREADS", "MDRP_PAIRS_PER_PASS", "MDRP_SAMPLE_THREADS",
         "MDRP_FUSE_GATE_US", "MDRP_FUSE_WAIT_US")
RO = dict(max_epipolar_error=2.0, max_reproj_error=16.0)
LOSS = "TRUNCATED_CAUCHY"
# dynamic stopping that can end a run of 300 iterations at 70 % outliers: log(1 - 0.9) / log(1 - 0.3^3) = 84 iterations
DYNAMIC = dict(success_prob=0.9, dyn_num_trials_mult=1.0)
OUTLIERS = (0.7, 0.8, 0.85)
NAMES = {(0, False): "calib_p3p", (0, True): "calib_shift", (1, False): "shared", (2, False): "varying"}  # helpers.OPTIONS_KINDS
FILL = 7  # what a caller-owned device mask holds before a call: the comparison is deterministic wherever a call leaves a byte alone


def ragged(batch, n_max):
    """correspondence counts of a batch: the full width first, a pair below every sample size, an empty pair, odd counts"""
    cycle = [n_max, 2, 0, n_max - 17, n_max // 2 + 1, 8, n_max - 1] if batch >= 5 else [n_max, n_max - 7]
    return np.array([cycle[i % len(cycle)] for i in range(batch)], dtype=np.int32)


def estimator_batch(kind, shift, batch, n_max, seed, clean=False, focal=800.0, outliers=OUTLIERS, ns=None):
    """padded arrays x1, x2 (B, n_max, 2), d1, d2 (B, n_max), n (B,), the pairs' ground truth and outlier flags, the planted inlier ratio"""
    ns = ragged(batch, n_max) if ns is None else np.asarray(ns, dtype=np.int32)
    rf = {1: "shared", 2: "varying", 4: "shared"}.get(kind)
    x1 = np.zeros((batch, n_max, 2)); x2 = np.zeros((batch, n_max, 2)); d1 = np.ones((batch, n_max)); d2 = np.ones((batch, n_max))
    flags = np.zeros((batch, n_max), dtype=bool)
    pairs = []
    for i, n in enumerate(ns):
        p = synth.make_pair(seed + i, max(int(n), 8), f1=focal, f2=focal, noise_px=0.0 if clean else 1.0, depth_noise=0.0 if clean else 0.05,
                            outlier_frac=0.0 if clean else outliers[i % len(outliers)], random_focal=rf, shift1=0.2 if shift else 0.0,
                            shift2=-0.1 if shift else 0.0)
        x1[i, :n], x2[i, :n], d1[i, :n], d2[i, :n], flags[i, :n] = p["x1"][:n], p["x2"][:n], p["d1"][:n], p["d2"][:n], p["is_outlier"][:n]
        pairs.append(p)
    valid = np.arange(n_max)[None, :] < ns[:, None]
    return dict(x1=x1, x2=x2, d1=d1, d2=d2, n=ns, pairs=pairs, is_outlier=flags, focal=focal,
                inlier_ratio=float(1.0 - flags[valid].mean()) if valid.any() else 1.0)


def cameras(capi, kind, batch, focal=800.0):
    """[B] camera records of the estimators that take them (5-point and calibrated: SIMPLE_PINHOLE; 6-point: the principal point 0, 0), else None"""
    if kind not in (0, 3, 4):
        return None
    rec = np.zeros(batch, dtype=capi.CAMERA_DTYPE)
    if kind != 4:
        rec["params"][:, 0] = focal
    return rec


def four(arrays):
    """any list of arrays as the dict helpers.input_digest hashes"""
    flat = [np.ascontiguousarray(np.asarray(a, dtype=np.float64)).reshape(-1) for a in arrays]
    flat += [np.zeros(0)] * max(0, 4 - len(flat))
    return dict(x1=flat[0], x2=flat[1], d1=flat[2], d2=np.concatenate(flat[3:]))


def apply_env(env, setenv, delenv):
    """every schedule knob unset, then `env` (a dict or None) set: through the setters of pytest's monkeypatch, or os.environ's own"""
    for k in KNOBS:
        delenv(k, raising=False)
    for k, v in (env or {}).items():
        setenv(k, v)


def environ_setters():
    return os.environ.__setitem__, lambda k, raising=False: os.environ.pop(k, None)


class Call:
    """one entry of the table.  make(): the inputs, built anew; data(): the same, built once; run(handle): the call, everything it defines as a
    tuple of byte strings named by `outputs`.  Device-resident calls also have issue(handle) -> state, which queues the call and waits for nothing
    the entry point itself does not wait for, and collect(handle, state) -> the byte strings."""
    kind = batch = n_max = max_iterations = min_iterations = None
    family = "unit"          # estimate | budgets | prior | ranked | refine | front_end | unit | refusal
    shift = False
    env = None               # schedule knobs this call runs under (predecessors only)
    twin_of = None           # (a): the name of the probe this is the clean twin of
    outputs = ("records", "mask")
    probe = True

    def __init__(self, name, entry_points, **kw):
        self.name, self.entry_points = name, tuple(entry_points)
        for k, v in kw.items():
            setattr(self, k, v)
        self._data = None
        self.stats = None    # last_stats() behind the last run, where run() fetches them

    def data(self):
        if self._data is None:
            self._data = self.make()
        return self._data

    def digest_arrays(self, d):
        return [d["x1"], d["x2"], d["d1"], d["d2"], d["n"]]

    @property
    def flags(self):
        """the switches of the call that are on, by name"""
        on = [k for k in ("shift", "device", "clean", "score_initial", "presorted", "estimate", "copy_records") if getattr(self, k, False)]
        return tuple(on + (["no_mask"] if getattr(self, "want_mask", True) is False else []))

    def shapes(self):
        return (self.batch, self.n_max, self.max_iterations)

    def __repr__(self):
        return self.name


def _capi():
    from mdrp_amd import _capi as capi
    return capi


# ------------------------------------------------------------------------------------------------------------------------ device plumbing
_DEV = {}


def _torch():
    import torch
    return torch


def device_arrays(key, arrays):
    """the arrays as tensors on cuda:0, uploaded once per process and complete before they are returned (the handles run on streams of their own)"""
    if key not in _DEV:
        torch = _torch()
        dev = torch.device("cuda", 0)
        _DEV[key] = [None if a is None else torch.from_numpy(np.array(a)).to(dev) for a in arrays]
        torch.cuda.synchronize()
    return _DEV[key]


def device_out(shape, dtype, fill=None):
    """a caller-owned output buffer on cuda:0; complete (filled, where a fill is given) before it is returned"""
    torch = _torch()
    dev = torch.device("cuda", 0)
    t = torch.empty(shape, dtype=dtype, device=dev) if fill is None else torch.full(shape, fill, dtype=dtype, device=dev)
    torch.cuda.synchronize()
    return t


def host_bytes(t):
    return t.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------------------------------ estimators
class Estimate(Call):
    """mdrp_estimate_batch (host buffers) / mdrp_estimate_batch_async + mdrp_fetch_results | mdrp_copy_results_device"""
    family = "estimate"
    device = False
    want_mask = True
    clean = False
    seed = 0
    focal = 800.0
    score_initial = False
    outliers = OUTLIERS
    copy_records = False   # device-resident: the records through mdrp_copy_results_device instead of mdrp_fetch_results
    more_ro = None
    ns = None

    def make(self):
        return estimator_batch(self.kind, self.shift, self.batch, self.n_max, self.seed, self.clean, self.focal, self.outliers, self.ns)

    def options(self):
        capi = _capi()
        ro = dict(RO, max_iterations=self.max_iterations, min_iterations=self.min_iterations, seed=self.seed % 5, monodepth_estimate_shift=self.shift,
                  score_initial_model=self.score_initial, **(DYNAMIC if self.min_iterations < self.max_iterations else {}), **(self.more_ro or {}))
        return capi.ransac_opt_from_dict(ro), capi.bundle_opt_from_dict({"loss_type": LOSS})

    def cams(self):
        return cameras(_capi(), self.kind, self.batch, self.focal)

    def tensors(self):
        d = self.data()
        mono = self.kind <= 2
        return device_arrays(self.name, [d["x1"], d["x2"], d["d1"] if mono else None, d["d2"] if mono else None])

    def run(self, h):
        if self.device:
            return self.collect(h, self.issue(h))
        d = self.data()
        ro, bo = self.options()
        cam = self.cams()
        res, mask = h.estimate_batch(self.kind, d["x1"], d["x2"], d["d1"], d["d2"], ro, bo, d["n"], cam, cam, want_mask=self.want_mask)
        self.stats = h.last_stats()
        return (res.tobytes(),) + ((mask.tobytes(),) if self.want_mask else ())

    mask_planes = ()

    def prepare(self):
        """the call's device buffers, complete: inputs (uploaded once per process) and the caller-owned outputs"""
        state = dict(x=self.tensors(), mask=device_out(tuple(self.mask_planes) + (self.batch, self.n_max), _torch().uint8, FILL) if self.want_mask else None)
        self.prepare_more(state)
        return state

    def prepare_more(self, state):
        pass

    def issue(self, h, state=None):
        state = self.prepare() if state is None else state
        ro, bo = self.options()
        self.queue(h, *state["x"], ro, bo, self.cams(), state["mask"], state)
        return state

    def owned(self, state):
        """the caller-owned outputs of an issued call, once the stream has drained: run()'s byte strings behind the records"""
        return (host_bytes(state["mask"]),) if self.want_mask else ()

    def queue(self, h, x1, x2, d1, d2, ro, bo, cam, mask, state):
        h.estimate_batch_device(self.kind, x1.data_ptr(), x2.data_ptr(), d1.data_ptr() if d1 is not None else None, d2.data_ptr() if d2 is not None else None,
                                self.batch, self.n_max, ro, bo, self.data()["n"], cam, cam, mask.data_ptr() if mask is not None else None)

    def collect(self, h, state):
        if self.copy_records:
            rec = device_out((self.batch, _capi().RESULT_DTYPE.itemsize), _torch().uint8, FILL)
            h.copy_results_device(rec.data_ptr(), self.batch)
            records = host_bytes(rec)
        else:
            records = h.fetch_results(self.batch).tobytes()
        self.stats = h.last_stats()
        return (records,) + self.owned(state)

    @property
    def outputs(self):
        return ("records", "mask") if self.want_mask else ("records",)


class Budgets(Estimate):
    """mdrp_estimate_batch_budgets / mdrp_estimate_batch_budgets_async + mdrp_fetch_budget_results (+ mdrp_copy_budget_results_device): every plane"""
    family = "budgets"
    budgets = (64, 150, 300)

    def run(self, h):
        if self.device:
            return self.collect(h, self.issue(h))
        d = self.data()
        ro, bo = self.options()
        cam = self.cams()
        res, mask = h.estimate_batch_budgets(self.kind, d["x1"], d["x2"], d["d1"], d["d2"], ro, bo, self.budgets, d["n"], cam, cam)
        self.stats = h.last_stats()
        return res.tobytes(), mask.tobytes()

    @property
    def mask_planes(self):
        return (len(self.budgets),)

    def queue(self, h, x1, x2, d1, d2, ro, bo, cam, mask, state):
        h.estimate_batch_budgets_device(self.kind, x1.data_ptr(), x2.data_ptr(), d1.data_ptr(), d2.data_ptr(), self.batch, self.n_max, ro, bo, self.budgets,
                                        self.data()["n"], cam, cam, mask.data_ptr())

    def collect(self, h, state):
        C = len(self.budgets)
        records = h.fetch_budget_results(C, self.batch).tobytes()
        self.stats = h.last_stats()
        rec = device_out((C, self.batch, _capi().RESULT_DTYPE.itemsize), _torch().uint8, FILL)
        h.copy_budget_results_device(rec.data_ptr(), C, self.batch)
        return records, host_bytes(state["mask"]), host_bytes(rec), h.fetch_results(self.batch).tobytes()

    @property
    def outputs(self):
        return ("planes", "mask planes", "planes copied on the device", "records of the last budget") if self.device else ("planes", "mask planes")


def start_models(e, d, how):
    """[B] model records from the pairs' ground truth through from_models_cases.start_model; how: one word per pair"""
    import from_models_cases as fc
    rng = np.random.default_rng(e.seed + 977)
    return _capi().array_to_models(np.stack([fc.start_model(NAMES[e.kind, e.shift], p, how[i % len(how)], rng, e.amount) for i, p in enumerate(d["pairs"])]))


class Prior(Estimate):
    """mdrp_estimate_batch_prior / mdrp_estimate_batch_prior_async: a prior per pair, one of them a NaN record (no prior), one hopeless"""
    family = "prior"
    how = ("perturbed", "exact", "identity", "nan", "hopeless", "perturbed", "perturbed")  # (beside ragged(): the NaN record on a pair of n_max - 17)
    amount = 1.0  # of from_models_cases.start_model's perturbation (1: about 2 deg / 5 % / 3 %)

    def make(self):
        d = Estimate.make(self)
        d["models"] = start_models(self, d, self.how)
        return d

    def digest_arrays(self, d):
        return Estimate.digest_arrays(self, d) + [d["models"].view(np.float64)]

    def run(self, h):
        if self.device:
            return self.collect(h, self.issue(h))
        d = self.data()
        ro, bo = self.options()
        cam = self.cams()
        res, mask = h.estimate_batch_prior(self.kind, d["x1"], d["x2"], d["d1"], d["d2"], d["models"], ro, bo, d["n"], cam, cam)
        self.stats = h.last_stats()
        return res.tobytes(), mask.tobytes()

    def prepare_more(self, state):
        state["models"], = device_arrays(self.name + "/models", [self.data()["models"].view(np.uint8)])

    def queue(self, h, x1, x2, d1, d2, ro, bo, cam, mask, state):
        pri = state["models"]
        h.estimate_batch_prior_device(self.kind, x1.data_ptr(), x2.data_ptr(), d1.data_ptr(), d2.data_ptr(), self.batch, self.n_max, pri.data_ptr(), ro, bo,
                                      self.data()["n"], cam, cam, mask.data_ptr())


class Ranked(Estimate):
    """mdrp_estimate_batch_ranked / mdrp_estimate_batch_ranked_async: scores as tests/prosac_cases.py plants them (the outlier flag plus noise), or
    none ("presorted": the records are taken to be in quality order)"""
    family = "ranked"
    presorted = False
    max_prosac = 150

    def make(self):
        d = Estimate.make(self)
        d["scores"] = -(d["is_outlier"] + np.random.default_rng(self.seed + 31).normal(0.0, 0.6, d["is_outlier"].shape))
        return d

    def digest_arrays(self, d):
        return Estimate.digest_arrays(self, d) + [d["scores"]]

    def options(self):
        self.more_ro = dict(max_prosac_iterations=self.max_prosac)
        return Estimate.options(self)

    def run(self, h):
        if self.device:
            return self.collect(h, self.issue(h))
        d = self.data()
        ro, bo = self.options()
        cam = self.cams()
        res, mask = h.estimate_batch_ranked(self.kind, d["x1"], d["x2"], d["d1"], d["d2"], None if self.presorted else d["scores"], ro, bo, d["n"], cam, cam)
        self.stats = h.last_stats()
        return res.tobytes(), mask.tobytes()

    def prepare_more(self, state):
        state["scores"] = None if self.presorted else device_arrays(self.name + "/scores", [self.data()["scores"]])[0]

    def queue(self, h, x1, x2, d1, d2, ro, bo, cam, mask, state):
        sc = state["scores"]
        h.estimate_batch_ranked_device(self.kind, x1.data_ptr(), x2.data_ptr(), d1.data_ptr(), d2.data_ptr(), None if sc is None else sc.data_ptr(), self.batch,
                                       self.n_max, ro, bo, self.data()["n"], cam, cam, mask.data_ptr())


class Refine(Prior):
    """mdrp_refine_batch / mdrp_refine_batch_async: records, mask, and the start models' scores and inlier counts"""
    family = "refine"
    stages = 3
    amount = 0.25  # (near enough for the refinement to reach the planted inliers: the start model is all a refine call has)
    max_iterations = min_iterations = 0  # (no sample is drawn)
    outputs = ("records", "mask", "start scores", "start counts")

    def run(self, h):
        if self.device:
            return self.collect(h, self.issue(h))
        d = self.data()
        ro, bo = self.options()
        cam = self.cams()
        res, mask, score0, inl0 = h.refine_batch(self.kind, d["x1"], d["x2"], d["d1"], d["d2"], d["models"], ro, bo, self.stages, d["n"], cam, cam)
        self.stats = h.last_stats()
        return res.tobytes(), mask.tobytes(), score0.tobytes(), inl0.tobytes()

    def prepare_more(self, state):
        Prior.prepare_more(self, state)
        state["score0"], state["inl0"] = device_out((self.batch,), _torch().float64, -1.0), device_out((self.batch,), _torch().int32, -1)

    def queue(self, h, x1, x2, d1, d2, ro, bo, cam, mask, state):
        h.refine_batch_device(self.kind, x1.data_ptr(), x2.data_ptr(), d1.data_ptr(), d2.data_ptr(), self.batch, self.n_max, state["models"].data_ptr(), ro, bo,
                              self.stages, self.data()["n"], cam, cam, mask.data_ptr(), state["score0"].data_ptr(), state["inl0"].data_ptr())

    def owned(self, state):
        return host_bytes(state["mask"]), host_bytes(state["score0"]), host_bytes(state["inl0"])


# ------------------------------------------------------------------------------------------------------------------------ front ends
class Matches(Call):
    """mdrp_gather_matches(_ranked) / mdrp_estimate_matches(_ranked)_async on a batch of tests/frontend_ranked_cases.py (float32 tables, int64 matches)"""
    family = "front_end"
    estimate = False
    score_dtype = None     # ranked forms: np.float32 | np.float64
    which = 1              # of the two six-pair batches of frontend_ranked_cases.batches()
    score_type_override = None
    max_iterations = min_iterations = 200

    def make(self):
        import frontend_ranked_cases as rc
        specs = ([(1, None), (2, None), (3, None), (63, None), (64, None), (600, None)], [(255, None), (256, None), (257, None), (64, "none_kept"), (70, 2), (100, 3)])
        b = dict(rc.make_batch(specs[self.which], 20 * self.which))
        if self.score_dtype is not None:
            b["scores"] = rc.batch_scores(rc.kept_rows(b), 2, 5).astype(self.score_dtype)
        return b

    def digest_arrays(self, d):
        return [d["kp1"], d["kp2"], d["dm1"], d["dm2"], d["matches"]] + ([d["scores"]] if "scores" in d else [])

    def descriptor(self):
        """(mdrp_matches, B, M, score pointer) over tensors uploaded once"""
        key = self.name + "/descriptor"
        if key not in _DEV:
            import mdrp_amd.poselib as poselib
            d = self.data()
            t = device_arrays(self.name, [d["kp1"].astype(np.float32), d["kp2"].astype(np.float32), d["matches"], d["dm1"].astype(np.float32),
                                          d["dm2"].astype(np.float32)] + ([d["scores"]] if "scores" in d else []))
            mm, keep, B, M, _ = poselib._matches_descriptor(*t[:5], d["c1"] if self.kind else None, d["c2"] if self.kind else None, "both_inf")
            _torch().cuda.synchronize()  # (the descriptor's own copies: matches narrowed to int32, the centres)
            _DEV[key] = (mm, B, M, t[5].data_ptr() if len(t) > 5 else None, keep)
        return _DEV[key][:4]

    def score_type(self):
        capi = _capi()
        if self.score_type_override is not None:
            return self.score_type_override
        return capi.F32 if self.score_dtype == np.float32 else capi.F64

    def gather_buffers(self, B, M):
        torch = _torch()
        return [device_out((B, M, 2), torch.float64), device_out((B, M, 2), torch.float64), device_out((B, M), torch.float64), device_out((B, M), torch.float64),
                device_out((B, M), torch.int32)]

    def run(self, h):
        capi = _capi()
        mm, B, M, sp = self.descriptor()
        if not self.estimate:
            out = self.gather_buffers(B, M)
            ptrs = [t.data_ptr() for t in out]
            n = h.gather_matches(mm, B, *ptrs) if self.score_dtype is None else h.gather_matches_ranked(mm, sp, self.score_type(), B, *ptrs)
            h.synchronize()
            return tuple(host_bytes(t) for t in out) + (n.tobytes(),)
        import test_gpu_frontend as fe
        import mdrp_amd.poselib as poselib
        ro, bo = capi.ransac_opt_from_dict(dict(fe.RO, max_prosac_iterations=150)), capi.bundle_opt_from_dict(fe.BO)
        cam1, cam2 = (poselib._camera_records(fe.CAM1, B), poselib._camera_records(fe.CAM2, B)) if self.kind == 0 else (None, None)
        mask = device_out((B, M), _torch().uint8, FILL)
        if self.score_dtype is None:
            n = h.estimate_matches_device(self.kind, mm, B, ro, bo, cam1, cam2, mask.data_ptr())
        else:
            n = h.estimate_matches_ranked_device(self.kind, mm, sp, self.score_type(), B, ro, bo, cam1, cam2, mask.data_ptr())
        records = h.fetch_results(B).tobytes()
        self.stats = h.last_stats()
        return records, host_bytes(mask), n.tobytes()

    @property
    def outputs(self):
        return ("records", "match mask", "n") if self.estimate else ("x1", "x2", "d1", "d2", "slot", "n")


IP_PAIRS = [0, 2, 6, 7, 9, 5]  # of image_pairs_cases.PAIRS: (0, 1) twice, a == c, an image index outside the set, the 600-row pair, (4, 0)


class ImagePairs(Matches):
    """the same four on per-image tables (tests/image_pairs_cases.py)"""

    def make(self):
        import frontend_ranked_cases as rc
        import image_pairs_cases as ipc
        from mdrp_amd import frontend
        t = ipc.make_batch()
        b = dict(t, pairs=t["pairs"][IP_PAIRS], matches=t["matches"][IP_PAIRS])
        if self.score_dtype is not None:
            kept = frontend.gather_image_pairs_numpy(t["keypoints"].astype(np.float32), t["depth_maps"].astype(np.float32), b["pairs"], b["matches"],
                                                     sizes=t["sizes"], kp_counts=t["kp_counts"])[5] >= 0
            b["scores"] = rc.batch_scores(kept, 3, 12).astype(self.score_dtype)
        return b

    def digest_arrays(self, d):
        return [d["keypoints"], d["depth_maps"], d["pairs"], d["matches"], d["sizes"], d["kp_counts"], d["centers"]] + ([d["scores"]] if "scores" in d else [])

    def descriptor(self):
        key = self.name + "/descriptor"
        if key not in _DEV:
            import mdrp_amd.poselib as poselib
            d = self.data()
            t = device_arrays(self.name, [d["keypoints"].astype(np.float32), d["depth_maps"].astype(np.float32), d["matches"]] + ([d["scores"]] if "scores" in d else []))
            ip, keep, host_pairs, B, M, I, _ = poselib._image_pairs_descriptor(t[0], t[1], d["pairs"], t[2], d["centers"] if self.kind else None, d["sizes"],
                                                                              d["kp_counts"], "both_inf", True)
            _torch().cuda.synchronize()
            _DEV[key] = (ip, B, M, t[3].data_ptr() if len(t) > 3 else None, keep, host_pairs, I)
        return _DEV[key][:4]

    def run(self, h):
        capi = _capi()
        ip, B, M, sp = self.descriptor()
        if not self.estimate:
            out = self.gather_buffers(B, M)
            ptrs = [t.data_ptr() for t in out]
            n = h.gather_image_pairs(ip, B, *ptrs) if self.score_dtype is None else h.gather_image_pairs_ranked(ip, sp, self.score_type(), B, *ptrs)
            h.synchronize()
            return tuple(host_bytes(t) for t in out) + (n.tobytes(),)
        import image_pairs_cases as ipc
        import mdrp_amd.poselib as poselib
        ro, bo = capi.ransac_opt_from_dict(dict(ipc.RO, max_prosac_iterations=150)), capi.bundle_opt_from_dict(ipc.BO)
        host_pairs, I = _DEV[self.name + "/descriptor"][5:7]
        cam1, cam2 = poselib._pair_cameras(ipc.CAMERAS, host_pairs, I) if self.kind == 0 else (None, None)
        mask = device_out((B, M), _torch().uint8, FILL)
        if self.score_dtype is None:
            n = h.estimate_image_pairs_device(self.kind, ip, B, ro, bo, cam1, cam2, mask.data_ptr())
        else:
            n = h.estimate_image_pairs_ranked_device(self.kind, ip, sp, self.score_type(), B, ro, bo, cam1, cam2, mask.data_ptr())
        records = h.fetch_results(B).tobytes()
        self.stats = h.last_stats()
        return records, host_bytes(mask), n.tobytes()


# ------------------------------------------------------------------------------------------------------------------------ unit entry points
class Unit(Call):
    """a unit entry point: fn(handle, capi, data) -> arrays"""

    def __init__(self, name, entry_points, make, fn, outputs, digest):
        Call.__init__(self, name, entry_points, outputs=outputs)
        self.make, self._fn, self._digest = make, fn, digest

    def digest_arrays(self, d):
        return self._digest(d)

    def run(self, h):
        return tuple(np.ascontiguousarray(a).tobytes() for a in self._fn(h, _capi(), self.data()))


def _minimal_problems(size, seed, count=70, bearings=False):
    """`count` minimal problems of `size` correspondences drawn from one hard pair, normalised by the focal length"""
    p = synth.make_pair(seed, 260, noise_px=1.0, depth_noise=0.05, outlier_frac=0.7)
    idx = np.stack([np.random.default_rng([seed, k]).choice(260, size, replace=False) for k in range(count)])
    h1 = np.concatenate([p["x1"][idx] / 800.0, np.ones((count, size, 1))], axis=2)
    h2 = np.concatenate([p["x2"][idx] / 800.0, np.ones((count, size, 1))], axis=2)
    if bearings:
        h1, h2 = h1 / np.linalg.norm(h1, axis=-1, keepdims=True), h2 / np.linalg.norm(h2, axis=-1, keepdims=True)
    return dict(x1h=np.ascontiguousarray(h1), x2h=np.ascontiguousarray(h2), d1=np.ascontiguousarray(p["d1"][idx]), d2=np.ascontiguousarray(p["d2"][idx]))


def _retirement_pair():
    """one small case of tests/retirement_cases.py: 257 correspondences at 40 % outliers and its 1100 models; a record most of them cannot beat"""
    import retirement_cases as rtc
    x1, x2, ms = rtc.pair_case.__wrapped__(257, 1)
    return dict(x1=x1, x2=x2, models=ms, thr=rtc.THR, rec_cnt=120, rec_score=rtc.THR * (257 - 120))


def _replay_case():
    """one small case of tests/replay_cases.py: 65 pairs (every pattern and start state), one chunk of 65 iterations of four slots"""
    import replay_cases as rc
    return rc.head_of(rc._edge_base.__wrapped__(4), 65, "history")


def _replay_digest(c):
    t = c["tables"]
    return [np.stack([x.score for x in t]), np.stack([x.cnt for x in t]), np.stack([x.lo_score for x in t]), np.stack([x.lo_cnt for x in t]),
            np.stack([x.ids for x in t]), np.stack([x.lo_ids for x in t])]


def _run_replay(h, capi, c):
    import test_gpu_replay as trp
    opt = c["opt"]
    ro = capi.ransac_opt_from_dict(dict(max_iterations=opt.max_iterations, min_iterations=opt.min_iterations, dyn_num_trials_mult=opt.dyn_num_trials_mult,
                                        success_prob=opt.success_prob))
    lens = c["supers"][0]
    rows = sum(lens)

    def models(ids):
        m = np.zeros(ids.shape, dtype=capi.MODEL_DTYPE)
        m["q"][..., 0] = ids
        return m
    cut = lambda get: np.stack([get(t)[:rows].reshape(-1) for t in c["tables"]])  # noqa: E731
    r = h.replay_slots(c["mps"], opt.sample_sz, c["chunk_start"], lens, ro, trp._state_records(capi, c["states"]), cut(lambda t: t.score), cut(lambda t: t.cnt),
                       cut(lambda t: models(t.ids)), cut(lambda t: t.lo_score), cut(lambda t: t.lo_cnt), cut(lambda t: models(t.lo_ids)))
    trig = np.concatenate(r["triggers"]) if len(r["triggers"]) else np.zeros(0, dtype=capi.REPLAY_TRIGGER_DTYPE)
    return (r["states"], trig, r["n_triggers"], r["scan_cnt"], r["scan_score"], r["scan_inst"], r["prefix"], r["begin"], r["end"],
            np.array([r["total"], r["n_active"], r["max_needed"]], dtype=np.int64))


def _front_lists_case():
    """part of one group of tests/first_front_cases.py (pick 3): the margin cases, the ties, ten random tables and the inactive pair"""
    import first_front_cases as ffc
    cases = [c for c in ffc.groups()[(3, ffc.SMALL)] if c.name.startswith(("margin", "table 30", "inactive", "ties"))]
    return dict(n=np.array([c.n for c in cases], dtype=np.int32), thr=np.array([c.thr for c in cases]), active=np.array([c.active for c in cases], dtype=np.int32),
                tags=[c.tags for c in cases], lens=np.array([len(c.tags) for c in cases], dtype=np.int32), slot_score=np.stack([c.slot_score for c in cases]),
                slot_inl=np.stack([c.slot_inl for c in cases]))


def _run_front_lists(h, capi, d):
    r = h.front_lists(d["n"], d["thr"], d["active"], d["tags"], 3, d["slot_score"], d["slot_inl"])
    return (np.concatenate([np.sort(t) for t in r["picked"]]), np.concatenate([np.sort(t) for t in r["rest"]]), np.concatenate([np.sort(t) for t in r["kept"]]),
            r["pick_count"], r["rest_count"], r["surv_count"], np.array([r["evals"]], dtype=np.uint64))


def _front_stages_case():
    """a ragged calibrated batch (a pair below the sample size, an empty pair) and two chunks, the second ending inside a wavefront"""
    d = estimator_batch(0, False, 5, 130, 9400)
    return dict(d, lens=np.array([64, 41], dtype=np.int32))


def _run_front_stages(h, capi, d):
    ro = capi.ransac_opt_from_dict(dict(RO, max_iterations=110, min_iterations=110, seed=5))
    r = h.front_stages(0, d["x1"], d["x2"], d["d1"], d["d2"], ro, capi.bundle_opt_from_dict({"loss_type": LOSS}), d["lens"], n_per_pair=d["n"],
                       cam1=cameras(capi, 0, 5), cam2=cameras(capi, 0, 5), slot_iters=110)
    tags = r["tags"].copy()  # (the order of a tag list is not defined: the live entries sorted, the untouched rest as it is)
    for c in range(tags.shape[0]):
        for p in range(tags.shape[1]):
            k = max(0, min(int(r["model_count"][c, p, 0]), tags.shape[2]))
            tags[c, p, :k] = np.sort(tags[c, p, :k])
    return (r["pts"], r["dep"], r["rfrag"], r["states"], r["table_of_pair"], r["table_n"], r["samples"], r["slot_inl"], r["models"], tags, r["model_count"])


def _refine_problem():
    import from_models_cases as fc
    p = synth.make_pair(9107, 130, noise_px=1.0, depth_noise=0.05, outlier_frac=0.7)
    rng = np.random.default_rng(9107)
    models = np.stack([fc.start_model("calib_p3p", p, "perturbed", rng, amount) for amount in (0.5, 1.0, 2.0, 3.0)])
    return dict(x1=p["x1"] / 800.0, x2=p["x2"] / 800.0, d1=p["d1"], d2=p["d2"], models=models)


def _rank_problem():
    d = estimator_batch(0, False, 5, 130, 9300)
    return dict(scores=-(d["is_outlier"] + np.random.default_rng(9300).normal(0.0, 0.6, d["is_outlier"].shape)).round(1), n=d["n"])  # (rounded: ties)


def _units():
    xs = lambda d: [d["x1h"], d["x2h"], d["d1"], d["d2"]]  # noqa: E731
    mods = lambda d: [d["x1"], d["x2"], d["models"]]  # noqa: E731
    M = lambda capi, d: capi.array_to_models(d["models"])  # noqa: E731
    return [
        Unit("solver_batch", ["mdrp_solver_batch"], lambda: _minimal_problems(3, 9101), lambda h, capi, d: h.solver_batch(1, d["x1h"], d["x2h"], d["d1"], d["d2"]),
             ("models", "counts"), xs),
        Unit("classic_solver_batch", ["mdrp_classic_solver_batch"], lambda: _minimal_problems(5, 9102, bearings=True),
             lambda h, capi, d: h.classic_solver_batch(capi.RELPOSE_5PT, d["x1h"], d["x2h"]), ("models", "counts"), xs),
        Unit("score_models", ["mdrp_score_models"], _retirement_pair, lambda h, capi, d: h.score_models(0, M(capi, d), d["x1"], d["x2"], d["thr"]),
             ("scores", "counts"), mods),
        Unit("count_candidates", ["mdrp_count_candidates"], _retirement_pair, lambda h, capi, d: (h.count_candidates(2, M(capi, d), d["x1"], d["x2"], d["thr"]),),
             ("candidates",), mods),
        Unit("bound_models", ["mdrp_bound_models"], _retirement_pair, lambda h, capi, d: h.bound_models(0, M(capi, d), d["x1"], d["x2"], d["thr"]),
             ("score bounds", "count bounds"), mods),
        Unit("retire_models", ["mdrp_retire_models"], _retirement_pair,
             lambda h, capi, d: h.retire_models(0, M(capi, d), d["x1"], d["x2"], d["thr"], d["rec_cnt"], d["rec_score"], (50_000, 1_000_000),
                                                capi.RETIRE_TWO_PHASE | capi.RETIRE_BOUND | capi.RETIRE_SWEEP_SPLIT),
             ("scores", "counts", "left at", "info", "candidate statistics"), mods),
        Unit("replay_slots", ["mdrp_replay_slots"], _replay_case, _run_replay,
             ("states", "triggers", "n_triggers", "scan_cnt", "scan_score", "scan_inst", "prefix", "begin", "end", "total | n_active | max_needed"), _replay_digest),
        Unit("front_lists", ["mdrp_front_lists"], _front_lists_case, _run_front_lists,
             ("picked (sorted)", "rest (sorted)", "kept (sorted)", "pick_count", "rest_count", "surv_count", "evals"),
             lambda d: [d["n"], d["thr"], d["active"], np.concatenate(d["tags"]), d["lens"], d["slot_score"], d["slot_inl"]]),
        Unit("front_models", ["mdrp_front_models"], _retirement_pair,
             lambda h, capi, d: h.front_models(1, M(capi, d), d["x1"], d["x2"], d["thr"], 48, d["rec_cnt"], d["rec_score"]),
             ("scores", "counts", "left at", "info"), mods),
        Unit("front_stages", ["mdrp_front_stages"], _front_stages_case, _run_front_stages,
             ("pts", "dep", "rfrag", "states", "table_of_pair", "table_n", "samples", "slot_inl", "models", "tags (sorted)", "model_count"),
             lambda d: [d["x1"], d["x2"], d["d1"], d["d2"], d["n"], d["lens"]]),
        Unit("refine_models", ["mdrp_refine_models"], _refine_problem,
             lambda h, capi, d: h.refine_models(0, M(capi, d), d["x1"], d["x2"], d["d1"], d["d2"], 1 / 64.0, 1.0, capi.bundle_opt_from_dict({"loss_type": LOSS})),
             ("models", "costs"), lambda d: [d["x1"], d["x2"], d["d1"], d["d2"], d["models"]]),
        Unit("prosac_samples", ["mdrp_prosac_samples"], lambda: dict(row=np.array([300, 3, 150], dtype=np.int64), lens=np.array([128, 372], dtype=np.int32)),
             lambda h, capi, d: (h.prosac_samples(int(d["row"][1]), int(d["row"][0]), int(d["row"][2]), d["lens"]),), ("samples",), lambda d: [d["row"], d["lens"]]),
        Unit("rank_scores", ["mdrp_rank_scores"], _rank_problem, lambda h, capi, d: (h.rank_scores(d["scores"], d["n"]),), ("order",), lambda d: [d["scores"], d["n"]]),
    ]


# ------------------------------------------------------------------------------------------------------------------------ sequences and refusals
class Sequence(Call):
    """several calls as one predecessor"""
    probe = False
    outputs = ()

    def __init__(self, name, calls, **kw):
        Call.__init__(self, name, [p for c in calls for p in c.entry_points], **kw)
        self.calls = calls
        for k in ("kind", "batch", "n_max", "max_iterations", "min_iterations", "shift"):
            setattr(self, k, getattr(calls[-1], k))

    def make(self):
        return [c.make() for c in self.calls]

    def digest_arrays(self, d):
        return [a for c, x in zip(self.calls, d) for a in c.digest_arrays(x)]

    def run(self, h):
        out = ()
        for c in self.calls:
            out = c.run(h)
        self.stats = self.calls[-1].stats
        return out


class Refusal(Call):
    """a call its entry point refuses (MdrpError or NotImplementedError); what it returns says that it was refused"""
    family = "refusal"
    probe = False
    outputs = ()

    def __init__(self, name, good, spoil):
        Call.__init__(self, name, good.entry_points, kind=good.kind, batch=good.batch, n_max=good.n_max, max_iterations=good.max_iterations,
                      min_iterations=good.min_iterations)
        self.good, self.spoil = good, spoil

    def make(self):
        return self.good.make()

    def digest_arrays(self, d):
        return self.good.digest_arrays(d)

    def run(self, h):
        capi = _capi()
        self.good.data()  # (inputs and descriptors are the good call's: built before it is spoiled)
        if hasattr(self.good, "descriptor"):
            self.good.descriptor()
        undo = self.spoil(self.good)
        try:
            self.good.run(h)
        except (capi.MdrpError, NotImplementedError) as e:
            return (("refused: " + str(e)).encode(),)
        finally:
            undo()
        raise AssertionError(f"{self.name}: the call was not refused")


def _spoil_attr(attr, value):
    def spoil(call):
        was = getattr(call, attr)
        setattr(call, attr, value)
        return lambda: setattr(call, attr, was)
    return spoil


def _spoil_counts(call):
    """n_per_pair past n_max: refused behind the call's first device work"""
    n = call.data()["n"]
    was = n[0]
    n[0] = call.n_max + 1
    return lambda: n.__setitem__(0, was)


def _spoil_descriptor(field, value):
    def spoil(call):
        desc = call.descriptor()[0]
        was = getattr(desc, field)
        setattr(desc, field, value)
        return lambda: setattr(desc, field, was)
    return spoil


# ------------------------------------------------------------------------------------------------------------------------ the table
HOST, ASYNC = ["mdrp_estimate_batch"], ["mdrp_estimate_batch_async", "mdrp_fetch_results"]
S1, S2, S3, S4, S5, S6, S7 = (5, 130, 300, 300), (24, 300, 300, 20), (24, 40, 64, 64), (1, 300, 300, 20), (5, 40, 300, 300), (24, 130, 64, 64), (2, 40, 40, 40)


def _estimate(name, kind, shape, seed, device=False, cls=Estimate, entry_points=None, **kw):
    B, N, mx, mn = shape
    if mn < mx and not kw.get("clean"):
        kw.setdefault("outliers", (0.7,))  # (DYNAMIC stops a pair at 70 % outliers inside 300 iterations)
    return cls(name, entry_points or (ASYNC if device else HOST), kind=kind, batch=B, n_max=N, max_iterations=mx, min_iterations=mn, seed=seed, device=device, **kw)


@functools.lru_cache(maxsize=None)
def probes():
    e = _estimate
    copy = ["mdrp_estimate_batch_async", "mdrp_copy_results_device"]
    out = [
        # plain estimators, host buffers and device-resident; two kinds share every shape
        e("k0_host", 0, S1, 1000), e("k0_shift_device", 0, S1, 1100, True, shift=True), e("k3_host", 3, S1, 1200),
        e("k0_device", 0, S2, 1300, True), e("k5_host", 5, S2, 1400),
        e("k0_shift_host_no_mask", 0, S3, 1500, shift=True, want_mask=False), e("k3_device", 3, S3, 1600, True, entry_points=copy, copy_records=True),
        e("k1_host", 1, S4, 1700), e("k5_device", 5, S4, 1800, True),
        e("k1_device", 1, S5, 1900, True, want_mask=False), e("k2_device", 2, S5, 2000, True),
        e("k2_host", 2, S6, 2100), e("k5_host_short", 5, S6, 2200),
        e("k4_host", 4, S7, 2300), e("k4_device", 4, S7, 2400, True), e("k0_host_score_initial", 0, S7, 2500, score_initial=True),
        # budgets: three planes; the device-resident one stops dynamically
        e("budgets_host", 0, S1, 2600, cls=Budgets, entry_points=["mdrp_estimate_batch_budgets"]),
        e("budgets_device", 1, (5, 130, 300, 20), 2700, True, cls=Budgets,
          entry_points=["mdrp_estimate_batch_budgets_async", "mdrp_fetch_budget_results", "mdrp_copy_budget_results_device", "mdrp_fetch_results"]),
        e("prior_host", 1, S1, 2800, cls=Prior, entry_points=["mdrp_estimate_batch_prior"]),
        e("prior_device", 0, S6, 2900, True, cls=Prior, entry_points=["mdrp_estimate_batch_prior_async", "mdrp_fetch_results"]),
        e("ranked_host_1", 0, S1, 3000, cls=Ranked, entry_points=["mdrp_estimate_batch_ranked"], max_prosac=1),
        e("ranked_host_150", 0, S1, 3000, cls=Ranked, entry_points=["mdrp_estimate_batch_ranked"]),
        e("ranked_host_presorted", 0, S1, 3000, cls=Ranked, entry_points=["mdrp_estimate_batch_ranked"], presorted=True),
        e("ranked_device_150", 2, S2, 3100, True, cls=Ranked, entry_points=["mdrp_estimate_batch_ranked_async", "mdrp_fetch_results"]),
        e("refine_host_count_only", 0, (5, 130, 0, 0), 3200, cls=Refine, entry_points=["mdrp_refine_batch"], stages=0, shift=True),
        e("refine_host", 2, (24, 300, 0, 0), 3300, cls=Refine, entry_points=["mdrp_refine_batch"]),
        e("refine_device", 1, (5, 130, 0, 0), 3400, True, cls=Refine, entry_points=["mdrp_refine_batch_async", "mdrp_fetch_results"]),
    ]
    for cls, tag, points in ((Matches, "matches", ("mdrp_gather_matches", "mdrp_estimate_matches_async")),
                             (ImagePairs, "image_pairs", ("mdrp_gather_image_pairs", "mdrp_estimate_image_pairs_async"))):
        out.append(cls("gather_" + tag, [points[0]], kind=0))
        out.append(cls("estimate_" + tag, [points[1], "mdrp_fetch_results"], kind=0, estimate=True))
        for dt in (np.float32, np.float64):
            t = np.dtype(dt).name
            out.append(cls(f"gather_{tag}_ranked_{t}", [points[0] + "_ranked"], kind=0, score_dtype=dt))
            out.append(cls(f"estimate_{tag}_ranked_{t}", [points[1].replace("_async", "_ranked_async"), "mdrp_fetch_results"], kind=1 if dt == np.float64 else 0,
                           estimate=True, score_dtype=dt))
    return tuple(out + _units())


def estimator_probes():
    return [p for p in probes() if p.family == "estimate"]


def clean_twin(p):
    """(a) the probe's call on the same pairs without outliers and noise, through host buffers"""
    return Estimate("clean_twin_of_" + p.name, HOST, kind=p.kind, batch=p.batch, n_max=p.n_max, max_iterations=p.max_iterations, min_iterations=p.min_iterations,
                    seed=p.seed, shift=p.shift, clean=True, twin_of=p.name, probe=False)


FUSE_GIVE_UP = {"MDRP_FUSE_GATE_US": "1", "MDRP_FUSE_WAIT_US": "1"}
LARGER = (40, 700, 600, 600)


@functools.lru_cache(maxsize=None)
def extra_predecessors():
    e = functools.partial(_estimate, probe=False)
    p = {q.name: q for q in probes()}
    out = [clean_twin(q) for q in estimator_probes()]
    out += [e(f"larger_k{k}", k, LARGER, 4000 + 100 * k) for k in (0, 1, 3)]                                                             # (b)
    # (c) mdrp_capi.hip lm_mask_index_on / lm_list_stride: past 5461 correspondences the final refinement keeps no mask index beside its LDS lists,
    # past LM_LIST_MAX_N = 8192 the LM kernels keep no lists at all (lm_list_stride is 0)
    out.append(e("beyond_the_lm_mask_index", 0, (2, 5500, 64, 64), 4400, ns=(5500, 5203)))
    out.append(e("beyond_the_lm_list", 0, (2, 8200, 64, 64), 4450, ns=(8200, 8193)))
    out.append(Sequence("early_dynamic_stop", [e("long_before_the_stop", 0, (24, 300, 600, 600), 4500),                               # (d)
                                               e("stops_in_its_first_super_chunk", 0, (24, 300, 600, 20), 4600, clean=True)], probe=False))
    for tag, env in (("chunks", {"MDRP_CHUNKS": "64,256"}), ("unfused", {"MDRP_FUSE_TAIL": "0"}), ("two_pairs_per_pass", {"MDRP_PAIRS_PER_PASS": "2"})):
        out.append(e("knobs_" + tag, 0, (24, 300, 300, 300), 4700, env=env))                                                           # (e)
    out.append(e("fused_tail_gives_up", 0, (160, 600, 3000, 3000), 8800, env=FUSE_GIVE_UP, outliers=(0.5, 0.2, 0.0)))                  # (f)
    out.append(e("below_every_probe", 0, (1, 8, 16, 16), 4900, ns=(8,)))
    refused = [("estimate", p["k0_host"], _spoil_attr("kind", 7)), ("estimate_counts", e("counts_past_n_max", 0, S1, 5000, True), _spoil_counts),   # (g)
               ("budgets", p["budgets_host"], _spoil_attr("budgets", (300, 150, 64))), ("prior", p["prior_host"], _spoil_attr("kind", 3)),
               ("ranked", p["ranked_host_150"], _spoil_attr("kind", 5)), ("refine", p["refine_host"], _spoil_attr("stages", 4)),
               ("matches", p["estimate_matches"], _spoil_descriptor("filter", 2)), ("matches_ranked", p["estimate_matches_ranked_float32"], _spoil_attr("kind", 3)),
               ("image_pairs", p["estimate_image_pairs"], _spoil_descriptor("depth_type", -1)),
               ("image_pairs_ranked", p["gather_image_pairs_ranked_float64"], _spoil_attr("score_type_override", 2))]
    out += [Refusal("refused_" + tag, good, spoil) for tag, good, spoil in refused]
    return tuple(out)


def predecessors():
    return probes() + extra_predecessors()


@functools.lru_cache(maxsize=None)
def back_to_back():
    """[(predecessor, probe)] of device-resident calls issued without a wait between them: the same batch and n_max, other seeds, cameras and counts"""
    shape = (5, 130, 300, 300)
    a = dict(device=True, probe=False, focal=800.0)
    b = dict(device=True, probe=False, focal=640.0, ns=(113, 130, 0, 2, 97))
    e = _estimate
    ranked, prior, refine = ["mdrp_estimate_batch_ranked_async"], ["mdrp_estimate_batch_prior_async"], ["mdrp_refine_batch_async"]
    return ((e("b2b_estimate", 0, shape, 6000, **a), e("b2b_then_estimate", 0, shape, 6100, **b)),
            (e("b2b_no_iterations", 0, (5, 130, 0, 0), 6200, **a), e("b2b_then_estimate_2", 0, shape, 6300, **b)),
            (e("b2b_refine", 0, (5, 130, 0, 0), 6400, cls=Refine, entry_points=refine, **a), e("b2b_then_estimate_3", 0, shape, 6500, **b)),
            (e("b2b_estimate_2", 0, shape, 6600, **a), e("b2b_then_refine", 0, (5, 130, 0, 0), 6700, cls=Refine, entry_points=refine, **b)),
            (e("b2b_prior", 0, shape, 6800, cls=Prior, entry_points=prior, **a), e("b2b_then_ranked", 0, shape, 6900, cls=Ranked, entry_points=ranked, **b)),
            (e("b2b_ranked", 0, shape, 7000, cls=Ranked, entry_points=ranked, **a), e("b2b_then_plain", 0, shape, 7100, **b)))


def long_run():
    """a calibrated run long enough (8192 certain iterations) for its first chunk to follow the inlier ratios the handle saw in the call before"""
    return _estimate("long_run", 0, (5, 130, 8192, 8192), 7200, probe=False)


def by_name(name):
    for c in predecessors():
        if c.name == name:
            return c
    raise KeyError(name)


def first_difference(a, b):
    """index of the first differing byte of two byte strings (their common length where only the lengths differ), or None"""
    if a == b:
        return None
    x, y = np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)
    n = min(len(x), len(y))
    at = np.flatnonzero(x[:n] != y[:n])
    return int(at[0]) if len(at) else n


def mismatches(pred, probe, got, want):
    """[(predecessor, probe, which output, first differing index)] of a probe's byte strings against its fresh-handle ones"""
    out = [(str(pred), probe.name, "number of outputs", min(len(got), len(want)))] if len(got) != len(want) else []
    for name, a, b in zip(probe.outputs, got, want):
        at = first_difference(a, b)
        if at is not None:
            out.append((str(pred), probe.name, name, at))
    return out
