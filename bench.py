#!/usr/bin/env python3
"""bench.py — image-pairs/s of the RePoseD RANSAC hot path on MI355X (BASELINE.json metric).

A step = one pass of estimate_monodepth_relative_pose over one batch of synthetic image pairs that already sit in
HBM: calibrated 3-point solver (P3P path, shift off), 2000 correspondences per pair, max_iterations = min_iterations
= 10000 (BASELINE.json configs[1]; /root/reference/make_video.py:192-194), 50 % outliers, 0.5 px / 2 % noise,
1024 pairs per GPU.  Pairs shard across ranks with no data-path collective (weak scaling); for N > 1 the step ends
with one device-side RCCL all_gather of the fixed-size result records.  --total-pairs P switches to BASELINE.json
configs[4]: P pairs in total, ceil(P/N) contiguous pairs per rank, each rank generating only its own block (strong scaling).

A plain run generates its inputs, warms up, times the steps and prints the line (with what the timed steps' own counters give:
roofline, per-kernel times, quality).  --full also runs everything else the line can carry: the CPU baselines, the in-flight and
host-buffer steps and, on the default run, the other configs, one rank's share of configs[4] and the latency block.

    python bench.py --gpus 1 --steps 3 --warmup 1
    python bench.py --full
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
    python -m torch.distributed.run ... bench.py --gpus 8 --total-pairs 100000
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec
BYTES_PER_EVAL = 32.0      # x1,x2 as four fp64 per (model x correspondence) Sampson evaluation

WORKLOADS = {
    # name: (kind, n, iters, outliers, estimate_shift, random_focal)
    "calib_p3p_n2000_i10k": (0, 2000, 10000, 0.5, False, None),
    "calib_shift_n2000_i10k": (0, 2000, 10000, 0.5, True, None),
    "shared_n2000_i10k": (1, 2000, 10000, 0.5, False, "shared"),
    "varying_n5000_i10k": (2, 5000, 10000, 0.5, False, "varying"),  # + the shift FLAG (SHIFT_FLAG_ONLY): BASELINE configs[3]
    # SURVEY.md §8(d) C2 also asks for the outlier-free shape
    "calib_p3p_n2000_i10k_clean": (0, 2000, 10000, 0.0, False, None),
    "calib_shift_n2000_i10k_clean": (0, 2000, 10000, 0.0, True, None),
    # beyond BASELINE.json: the headline shape at 75 % / 85 % outliers (one 3-point sample in 64 / 300 is outlier-free: DESIGN.md §10, MDRP_CHUNKS)
    "calib_p3p_n2000_i10k_o75": (0, 2000, 10000, 0.75, False, None),
    "calib_p3p_n2000_i10k_o85": (0, 2000, 10000, 0.85, False, None),
    "shared_n2000_i10k_o75": (1, 2000, 10000, 0.75, False, "shared"),
    # ... and a batch whose pairs differ: outlier fraction 20 / 50 / 70 / 85 % by pair index
    "calib_p3p_n2000_i10k_mixed": (0, 2000, 10000, (0.2, 0.5, 0.7, 0.85), False, None),
    # non-monodepth baselines on the same kernels: 5-point relative pose, 7-point fundamental matrix
    "relpose_5pt_n2000_i10k": (3, 2000, 10000, 0.5, False, None),
    "fundamental_7pt_n2000_i10k": (5, 2000, 10000, 0.5, False, None),
    "shared_6pt_n2000_i10k": (4, 2000, 10000, 0.5, False, "shared"),
}

# BASELINE.json configs[3] sets monodepth_estimate_shift=True on the varying-focal estimator.  The reference ignores the flag there
# (include/mdrp.h, tests/golden/estimate_wide.npz `varying_shiftflag`); it is passed all the same, the synthetic depths carry no shift.
SHIFT_FLAG_ONLY = {"varying_n5000_i10k"}


def make_inputs(workload, first_index, batch):
    from mdrp_amd import synth
    kind, n, iters, of, es, rf = WORKLOADS[workload]
    kw = dict(noise_px=0.5, depth_noise=0.02, random_focal=rf, shift1=0.2 if es else 0.0, shift2=-0.1 if es else 0.0)
    if isinstance(of, tuple):  # per pair, by its index
        pairs = [synth.make_pair(first_index + i, n, outlier_frac=of[(first_index + i) % len(of)], **kw) for i in range(batch)]
        b = {k: np.ascontiguousarray(np.stack([p[k] for p in pairs])) for k in ("x1", "x2", "d1", "d2")}
        b["gt"] = pairs
        return b
    return synth.make_batch(first_index, batch, n, outlier_frac=of, **kw)


_GEN_SHARED = None  # (workload, first index, {name: shared numpy array}) of make_inputs_pool, inherited by its forked workers


def _gen_chunk(args):
    off, count = args
    workload, first, arrs = _GEN_SHARED
    b = make_inputs(workload, first + off, count)
    for k in ("x1", "x2", "d1", "d2"):
        arrs[k][off:off + count] = b[k]
    return [{"R": g["R"]} for g in b["gt"]] if off < 64 else []  # bench.py's quality check looks at the first 64 pairs only


def under_profiler():
    """Never fork under a profiler: rocprofv3 (with --pmc) initialises the GPU in its preloaded library before this program starts, and
    forked children of such a process hang (found by a profile pass of round 4 that waited 56 minutes for its pool)."""
    return any(("rocprof" in os.environ.get(k, "").lower()) for k in ("LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "HSA_TOOLS_LIB", "ROCPROFILER_REGISTER_LIBRARY"))


def make_inputs_pool(workload, first_index, batch, workers):
    """the same batch as make_inputs (per-pair seeds: identical data), generated by `workers` forked processes straight into shared
    memory — one rank's share of BASELINE configs[4] (12 500 pairs x 2000 correspondences) is ~15 s of per-pair numpy RNG on one
    core.  Must run BEFORE the process touches the GPU (fork).  (1024 pairs are 1.2 s on one core: the pool is for one rank's share of configs[4].)"""
    global _GEN_SHARED
    profiled = under_profiler()
    if workers <= 1 or batch < 4096 or profiled:
        return make_inputs(workload, first_index, batch)
    import multiprocessing as mp
    n = WORKLOADS[workload][1]
    arrs = {}
    for k, shape in (("x1", (batch, n, 2)), ("x2", (batch, n, 2)), ("d1", (batch, n)), ("d2", (batch, n))):
        raw = mp.RawArray("d", int(np.prod(shape)))
        arrs[k] = np.frombuffer(raw, dtype=np.float64).reshape(shape)
    _GEN_SHARED = (workload, first_index, arrs)
    step = max(16, (batch + 8 * workers - 1) // (8 * workers))
    jobs = [(o, min(step, batch - o)) for o in range(0, batch, step)]
    with mp.get_context("fork").Pool(workers) as pool:
        gts = pool.map(_gen_chunk, jobs, chunksize=1)
    _GEN_SHARED = None
    out = dict(arrs)
    out["gt"] = [g for part in gts for g in part]
    return out


def _cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _cpu_worker(args):
    """one host core: `count` pairs of the workload starting at `first` through the CPU oracle; returns busy seconds"""
    workload, first, count = args
    from oracle import pyorc as po
    kind, n, iters, of, es, rf = WORKLOADS[workload]
    b = make_inputs(workload, first, count)
    ro = po.ransac_opt(max_iterations=iters, min_iterations=iters, max_epipolar_error=2.0, max_reproj_error=16.0,
                       estimate_shift=es or workload in SHIFT_FLAG_ONLY)
    bo = po.bundle_opt(loss_type=4)
    cam = po.cam_flat(0, [800.0, 0.0, 0.0])
    po.lib()
    t0 = time.perf_counter()
    for i in range(count):
        if kind >= 3:
            po.estimate_classic(kind, b["x1"][i], b["x2"][i], ro, bo, cam, cam, pp=(0.0, 0.0))
        else:
            po.estimate(kind, b["x1"][i], b["x2"][i], b["d1"][i], b["d2"][i], ro, bo, cam if kind == 0 else None, cam if kind == 0 else None)
    return time.perf_counter() - t0


def cpu_baseline(workload, pairs, multi=True):
    """the CPU oracle (oracle/*.c — our port of the reference algorithm, pinned against the reference binary) on the
    same workload: single thread on the first `pairs` pairs (the reported baseline), then up to 32
    worker processes with their own pairs (like the reference's `eval.py -nw`).  Must run BEFORE the process touches
    the GPU: the workers are forked."""
    import multiprocessing as mp
    dt = _cpu_worker((workload, 0, pairs))
    cores = os.cpu_count() or 1
    out = {"value": pairs / dt, "unit": "image-pairs/s", "cores": 1, "kind": "port",
           "sample": f"{pairs} pairs of {workload} (same generator, indices 0..{pairs - 1}), {dt:.1f} s wall, 1 thread",
           "cpu_model": _cpu_model(), "host_cores": cores}
    if cores > 1 and multi and not under_profiler():  # (forked workers: never under rocprofv3, see under_profiler)
        # bounded: at most 32 workers x 6 pairs (the GPU boxes advertise 256 CPUs but schedule ~8 cores' worth of time to
        # the job: 256 workers x 16 pairs took 54 s for 75 pairs/s)
        workers = min(cores, 32)
        per = max(2, min(6, pairs // 6))
        t0 = time.perf_counter()
        with mp.get_context("fork").Pool(workers) as pool:
            busy = pool.map(_cpu_worker, [(workload, w * per, per) for w in range(workers)], chunksize=1)
        dta = time.perf_counter() - t0
        out["multi_process"] = {"value": workers * per / max(busy), "unit": "image-pairs/s", "cores": workers,
                                "sample": f"{workers} worker processes x {per} pairs, slowest worker {max(busy):.1f} s busy "
                                          f"({dta:.1f} s wall with process start-up and input generation)"}
    return out


_PMC_USED, _PMC_STALE = set(), set()  # PMC files whose numbers went onto the line / that were refused (another build's)


def pmc_profile(workload, batch, kernel):
    """Per-launch PMC numbers of `kernel` from the committed rocprofv3 passes of this round (profiles/r*_pmc_*.json, written
    by tools/pmc_json.py on the GPU box): HBM bytes (FETCH_SIZE x2 + WRITE_SIZE, the gfx950 correction of
    MI355X_MICROARCH.md) and the SQ issue counters, when they were taken on this workload and batch; else {}.
    These numbers are REPLAYED, not observed in this run (counters need a profiler pass): they are attached only if the PMC file
    records the source hash of the library this process runs (mdrp_version()); a file from another build is refused and listed
    under `pmc_stale` on the line.  Every file that was used is named once, under `pmc_replayed_from`."""
    import glob
    from mdrp_amd import _capi
    try:
        lib_hash = _capi.library_source_hash()
    except Exception:
        lib_hash = None
    out = {}
    import re
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_*.json")))
    rounds = [int(m.group(1)) for f in files for m in [re.match(r"r(\d+)", os.path.basename(f))] if m]
    newest = max(rounds) if rounds else None  # only the newest round's counter passes are candidates (older rounds profiled older kernels)
    for f in files:
        m = re.match(r"r(\d+)_pmc_", os.path.basename(f))
        if not m or int(m.group(1)) != newest:
            continue
        try:
            d = json.load(open(f))
        except Exception:
            continue
        if d.get("workload") != workload or d.get("pairs_per_gpu") != batch:
            continue
        if lib_hash is None or d.get("source_hash") != lib_hash:
            _PMC_STALE.add(os.path.basename(f))
            continue
        for k, v in d.get("kernels", {}).items():
            if k.split("<")[0] == "mdrp::" + kernel:
                out.update(v)
                out["source"] = os.path.basename(f)
                _PMC_USED.add(os.path.basename(f))
    return out


def sweep_hbm_roofline(w, kern, steps):
    """north_star's own number: achieved HBM GB/s of the SCORING SWEEP — k_count + k_bound + k_score — as PMC bytes per step (2 x FETCH_SIZE +
    WRITE_SIZE per launch x launches per step, replayed from the round's counter passes) over the three kernels' summed event time of THIS
    run, against the 8 TB/s peak.  (roofline_hbm_algorithmic prices the CPU loop's 32 B per evaluation instead and exceeds 1.)"""
    by, parts = 0.0, {}
    for kname in ("k_count", "k_bound", "k_score"):
        pr = pmc_profile(w.name, w.B, kname)
        if "hbm_bytes_corrected" not in pr:
            return None
        parts[kname] = pr["hbm_bytes_corrected"] * pr.get("launches_per_step", 1.0)
        by += parts[kname]
    ms = sum(kern[k] for k in ("k_count", "k_bound", "k_score")) / max(steps, 1)
    if ms <= 0:
        return None
    gbs = by / (ms / 1e3) / 1e9
    return {"bound": "hbm", "kernels": "k_count + k_bound + k_score", "bytes_per_step": by, "bytes_per_step_by_kernel": parts, "event_ms_per_step": ms,
            "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
            "note": "HBM-side bytes from PMC (replayed, see pmc_replayed_from) over this run's event time of the three sweep kernels: the sweep is bound by "
                    "matrix / vector issue, not by HBM (the correspondences of a pair stay in LDS / L2 while thousands of hypotheses sweep them)"}


MFMA_BF16_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA peak (~2.5 PFLOP/s; 512 MAC per cycle and SIMD)
FLOP_PER_MFMA_EVAL = 64.0       # one (model x correspondence) evaluation in k_count = 32 bf16 MACs of the K = 32 contraction
# fp64 vector peak.  MI355X_MICROARCH.md states the FP32 vector peak, 157.3 TFLOP/s (256 CUs x 4 SIMDs x 16 lanes x 2 packed x 2 flop
# x 2.4 GHz); the guide has no fp64 line.  CDNA4's published fp64 vector rate is half of that (one 64-bit FMA per lane and cycle, no
# packing): 78.6 TFLOP/s.  tools/ubench/fp64_peak.hip measured 69 TFLOP/s of it at 8 waves/SIMD.
FP32_VALU_PEAK_TFLOPS_GUIDE = 157.3
FP64_VALU_PEAK_TFLOPS = FP32_VALU_PEAK_TFLOPS_GUIDE / 2.0
# fp64 flop per correspondence of the LM sweeps, (cost sweep: residuals | normal-equation sweep: residuals + Jacobians + J'J),
# read off the ISA of this build by tools/lm_flops.py (FMA-class instructions 2 flop, every other fp64 VALU instruction 1);
# keyed by (estimator kind, monodepth_estimate_shift on the calibrated estimator).
# k_lo (round 4): the TRUNCATED loss is a compile-time constant there — rows of weight 1 skip the products by the weight, 1 / f is
# hoisted out of the sweeps, and the three reciprocals per correspondence are a hardware seed + two Newton steps instead of IEEE
# division chains: fewer flop per correspondence than in round 3 (179 | 716 calibrated).  The count is the loop's static
# fp64 content, i.e. every row accumulated; rows of weight zero are skipped at run time, so `achieved` is an upper estimate there.
# k_final runs the general path (run-time loss type, weights multiplied in): round 3's counts.
LM_FLOP = {(0, False): (132.0, 550.0), (0, True): (132.0, 626.0), (1, False): (140.0, 687.0), (2, False): (140.0, 735.0)}
# k_final (general path: run-time loss, the NP products by the weight per row stay; its loops are split by the loss switch, which
# tools/lm_flops.py cannot attribute): k_lo's counts + 5 NP flop per correspondence for the normal equations; loss-specific extras
# (log1p of the Cauchy losses) are not counted
LM_FLOP_FINAL = {(0, False): (132.0, 585.0), (0, True): (132.0, 671.0), (1, False): (140.0, 727.0), (2, False): (140.0, 780.0)}
# BASELINE.json configs[2] and configs[3]: measured after the headline on the default N = 1 run and reported under `configs`
# ... and, round 5, the other two variants of SURVEY.md 8(d) C2: the calibrated estimator with shifts (relpose_monodepth_3pt) and the outlier-free shape
# (workload, pairs of its CPU baseline); the last one is beyond BASELINE.json: the headline shape at 75 % outliers (no PMC replay: traffic null)
EXTRA_CONFIGS = (("shared_n2000_i10k", 24), ("varying_n5000_i10k", 16), ("calib_shift_n2000_i10k", 12), ("calib_p3p_n2000_i10k_clean", 8),
                 ("calib_p3p_n2000_i10k_o75", 8))
ESTIMATOR_NAMES = ["calibrated", "shared_focal", "varying_focal", "relative_pose_5pt", "shared_focal_6pt", "fundamental_7pt"]


def port_vs_reference():
    """pairs/s of the CPU port (oracle/*.c, what `cpu_baseline` times) relative to the reference's own PoseLib binary on the same
    core and inputs, per workload: measured in the build container by tests/tools/port_vs_reference.py (the reference binary cannot
    travel to the GPU box) and committed as profiles/r04_port_vs_reference.json; {} if that file is missing"""
    try:
        return json.load(open(os.path.join(ROOT, "profiles", "r04_port_vs_reference.json")))
    except Exception:
        return {}


class Workload:
    """one synthetic workload resident in HBM on this rank + the handle that runs it"""

    def __init__(self, name, lo, hi, per, local_rank, dev, inputs=None):
        import torch
        from mdrp_amd import _capi
        self.name = name
        self.kind, self.n, self.iters, self.of, self.es, self.rf = WORKLOADS[name]
        self.B, self.per = hi - lo, per
        B1 = max(self.B, 1)
        self.b = inputs if inputs is not None else make_inputs(name, lo, B1)
        self.x1 = torch.from_numpy(self.b["x1"]).to(dev); self.x2 = torch.from_numpy(self.b["x2"]).to(dev)
        self.d1 = torch.from_numpy(self.b["d1"]).to(dev); self.d2 = torch.from_numpy(self.b["d2"]).to(dev)
        self.mask = torch.zeros((B1, self.n), dtype=torch.uint8, device=dev)
        self.cams = np.zeros(B1, dtype=_capi.CAMERA_DTYPE)
        self.cams["params"][:, 0] = 800.0
        if self.kind == 4:
            self.cams["params"][:] = 0.0  # MDRP_SHARED_6PT: cam1 carries the principal point; the synthetic pixels are centred
        self.ro = _capi.ransac_opt_from_dict({"max_iterations": self.iters, "min_iterations": self.iters, "max_epipolar_error": 2.0,
                                              "max_reproj_error": 16.0, "monodepth_estimate_shift": self.es or name in SHIFT_FLAG_ONLY})
        self.bo = _capi.bundle_opt_from_dict({"loss_type": "TRUNCATED_CAUCHY"})
        self.with_cams = self.kind in (0, 3, 4)  # kind 4: the principal point travels in cam1 (0, 0 here)
        self.classic = self.kind >= 3
        self.h = _capi.Handle(local_rank)  # its own stream; every kernel class is timed with HIP events recorded on the stream it runs on
        torch.cuda.synchronize(dev)  # the inputs were written on torch's stream, the handle runs on its own: order them once

    def launch(self, h=None, mask=None):
        """queue one pass of the hot path over the resident batch (mdrp_estimate_batch_async on device pointers)"""
        h = h or self.h
        c = self.cams if self.with_cams else None
        h.estimate_batch_device(self.kind, self.x1.data_ptr(), self.x2.data_ptr(), 0 if self.classic else self.d1.data_ptr(),
                                0 if self.classic else self.d2.data_ptr(), self.B, self.n, self.ro, self.bo, None, c, c,
                                (mask if mask is not None else self.mask).data_ptr())

    def close(self):
        self.h.close()


def timed_steps(step, barrier, steps, warmup, stats_of=None):
    """W untimed warm-up steps, then exactly K steps between barrier + synchronize on both sides; returns (seconds, last result, summed stats)"""
    res = None
    for _ in range(warmup):
        step()
    acc = {}
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        res = step()
        if stats_of is not None:
            for k, v in stats_of().items():
                acc[k] = acc.get(k, 0) + v
    barrier()
    return time.perf_counter() - t0, res, acc


def rooflines_of(w, acc, steps, dt):
    """per-kernel time of the step (HIP events around every launch, on the stream it runs on) and the rooflines that have a work model.
    k_count: executed MFMA work (64 flop per evaluation, 16 x 16 tiles, padding included, counted on the device) against the dense bf16
    MFMA peak.  The LM kernels (k_lo, k_final): fp64 flop = correspondences their sweeps evaluated (counted on the device) x the flop
    per correspondence of LM_FLOP, against the fp64 vector peak.
    With the fused tail (the default where the run's end is known) k_final's events bracket its wait for the LO queue as well, and its
    interval overlaps the last k_lo launch: `k_lo+k_final` gives the two as ONE interval (union on the device timeline is not available
    from events on two streams; the sum is an upper bound) and the dominant kernel is never chosen from k_final's overlapped time."""
    kind, B, steps = w.kind, w.B, max(steps, 1)
    kern = {"k_count": acc.get("count_ms", 0.0), "k_score": acc.get("sweep_ms", 0.0), "k_bound": acc.get("bound_ms", 0.0),
            "k_solve": acc.get("solve_ms", 0.0), "k_lo": acc.get("lo_ms", 0.0), "k_final": acc.get("final_ms", 0.0)}
    launches = {"k_count": acc.get("count_launches", 0), "k_score": acc.get("sweep_launches", 0), "k_bound": acc.get("bound_launches", 0),
                "k_solve": acc.get("solve_launches", 0), "k_lo": acc.get("lo_launches", 0), "k_final": acc.get("final_launches", 0)}
    lm_key = (kind, bool(w.es) and kind == 0)
    rooflines = {}
    cl = max(launches["k_count"], 1)
    count_s = kern["k_count"] / 1e3
    flop = FLOP_PER_MFMA_EVAL * acc.get("evals_mfma", 0)
    achieved = flop / count_s / 1e12 if count_s > 0 else 0.0
    prof = pmc_profile(w.name, B, "k_count")
    hbm = prof.get("hbm_bytes_corrected")
    avg_launch_s = count_s / cl
    rooflines["k_count"] = {
        "bound": "mfma", "kernel": "k_count (v_mfma_f32_16x16x32_bf16)", "achieved": achieved, "peak": MFMA_BF16_PEAK_TFLOPS,
        "unit": "TFLOP/s", "frac": achieved / MFMA_BF16_PEAK_TFLOPS, "traffic": hbm, "traffic_unit": "HBM bytes per launch (PMC: 2 x FETCH_SIZE + WRITE_SIZE)",
        "traffic_source": prof.get("source"), "avg_launch_ms": 1e3 * avg_launch_s, "launches_per_step": cl / steps,
        "executed_evals_per_step": acc.get("evals_mfma", 0) / steps, "share_of_step": count_s / dt,
        "hbm_GBs": (hbm / avg_launch_s / 1e9) if (hbm and avg_launch_s > 0) else None,
        "hbm_frac": (hbm / avg_launch_s / 1e9 / HBM_PEAK_GBS) if (hbm and avg_launch_s > 0) else None,
        "mfma_busy_frac_pmc": prof.get("mfma_busy_frac"), "valu_active_per_simd_cycle_pmc": prof.get("valu_active_per_simd_cycle")}
    if lm_key in LM_FLOP:
        for name, ce, ae in (("k_lo", "lm_cost_evals", "lm_accum_evals"), ("k_final", "final_cost_evals", "final_accum_evals")):
            fc, fa = (LM_FLOP if name == "k_lo" else LM_FLOP_FINAL)[lm_key]
            ksec, nl = kern[name] / 1e3, max(launches[name], 1)
            fl = fc * acc.get(ce, 0) + fa * acc.get(ae, 0)
            ach = fl / ksec / 1e12 if ksec > 0 else 0.0
            pr = pmc_profile(w.name, B, name)
            hb = pr.get("hbm_bytes_corrected")
            rooflines[name] = {
                "bound": "fp64", "kernel": f"{name} (LM refinements: v_fma_f64)", "achieved": ach, "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": ach / FP64_VALU_PEAK_TFLOPS, "traffic": hb, "traffic_unit": "HBM bytes per launch (PMC: 2 x FETCH_SIZE + WRITE_SIZE)",
                "traffic_source": pr.get("source"), "avg_launch_ms": 1e3 * ksec / nl, "launches_per_step": nl / steps, "share_of_step": ksec / dt,
                "fp64_flop_per_step": fl / steps, "flop_per_correspondence": {"cost_sweep": fc, "normal_equations": fa},
                "correspondences_per_step": {"cost_sweep": acc.get(ce, 0) / steps, "normal_equations": acc.get(ae, 0) / steps},
                "hbm_GBs": (hb / (ksec / nl) / 1e9) if (hb and ksec > 0) else None,
                "hbm_frac": (hb / (ksec / nl) / 1e9 / HBM_PEAK_GBS) if (hb and ksec > 0) else None,
                "valu_active_per_simd_cycle_pmc": pr.get("valu_active_per_simd_cycle"), "mean_waves_per_simd_pmc": pr.get("mean_waves_per_simd"),
                "peak_note": "fp64 vector peak = half the guide's FP32 vector peak (157.3 TFLOP/s); the guide has no fp64 line"}
        if acc.get("fuse_timeouts", 0):
            rooflines["k_final"]["note"] = "fused tail hit a bounded-wait timeout in this run: k_final's interval includes give-up waits"
    # k_final's event interval overlaps the last k_lo launch when the tail is fused and includes its wait for ready pairs:
    # the dominant kernel is chosen among the others
    cand = {k: v for k, v in kern.items() if k != "k_final"}
    top = max(cand, key=lambda k: cand[k])
    if top not in rooflines and any(kern.values()):
        # k_solve / k_score / k_bound on top (the 5-/6-point baselines, the outlier-free shape): no device-side flop counter exists for
        # these (data-dependent root finders, early exits) - the entry carries the event time and the PMC issue fraction, no `achieved`
        tsec, tl = kern[top] / 1e3, max(launches[top], 1)
        pt = pmc_profile(w.name, B, {"k_solve": ("kc_solve5_reduce" if w.kind == 3 else "kc_solve") if w.classic else "k_solve"}.get(top, top))  # (5-point: the first of its two kernels)
        rooflines[top] = {
            "bound": "fp64" if top != "k_bound" else "fp32", "kernel": top, "achieved": None, "peak": FP64_VALU_PEAK_TFLOPS if top != "k_bound" else None,
            "unit": "TFLOP/s", "frac": None, "traffic": pt.get("hbm_bytes_corrected"), "traffic_source": pt.get("source"),
            "avg_launch_ms": 1e3 * tsec / tl, "launches_per_step": tl / steps, "share_of_step": tsec / dt,
            "valu_active_per_simd_cycle_pmc": pt.get("valu_active_per_simd_cycle"), "mean_waves_per_simd_pmc": pt.get("mean_waves_per_simd"),
            "note": "no flop model for this kernel: time and PMC issue fraction only; the LM and MFMA rooflines are in roofline_lm / roofline_count"}
    dominant = max((k for k in cand if k in rooflines), key=lambda k: cand[k]) if any(kern.values()) else "k_count"
    return kern, rooflines, dominant, top


def hbm_algorithmic(acc, steps, dt):
    """SURVEY.md 8(d)'s own figure: every (model x correspondence) Sampson evaluation of the CPU loop reads x1, x2 = 32 bytes.
    frac > 1 says what it has to say: the timed kernels do NOT stream 32 B per evaluation from HBM - a pair's correspondences stay
    in LDS / L2 while thousands of hypotheses sweep them, and 98 % of the evaluations are retired by conservative bf16-MFMA / fp32
    bounds instead of being evaluated in fp64."""
    ev = acc.get("evals_algorithmic", 0) / max(steps, 1)
    by = BYTES_PER_EVAL * ev
    gbs = by / (dt / max(steps, 1)) / 1e9 if dt > 0 else 0.0
    return {"bound": "hbm", "evals": ev, "bytes_per_eval": BYTES_PER_EVAL, "bytes": by, "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": gbs / HBM_PEAK_GBS,
            "note": "algorithmic bytes of the CPU loop over the whole step time; > 1 because correspondences are reused from LDS / L2 and "
                    "hypotheses are retired by conservative bounds (evals executed: work.evals_*_per_step)"}


LATENCY_SHAPES = {
    # name: (correspondences, RansacOptions) — the headline shape, and what /root/reference/eval.py:99-100 sets per call (max = min = 1000; its pairs have ~1000 matches)
    "headline_n2000_i10k": (2000, {"max_iterations": 10000, "min_iterations": 10000, "max_epipolar_error": 2.0, "max_reproj_error": 16.0}),
    "eval_py_n1000_i1k": (1000, {"max_iterations": 1000, "min_iterations": 1000, "max_epipolar_error": 2.0, "max_reproj_error": 16.0}),
}
LATENCY_CAM = {"model": "SIMPLE_PINHOLE", "width": 1600, "height": 1200, "params": [800.0, 0.0, 0.0]}


def latency_inputs(shape, count):
    from mdrp_amd import synth
    n, _ = LATENCY_SHAPES[shape]
    return synth.make_batch(0, count, n, noise_px=0.5, depth_noise=0.02, outlier_frac=0.5)


def cpu_latency(pairs=6):
    """ms per pair of the CPU port (oracle/*.c, one thread) on the latency shapes' own inputs — before the GPU is touched, like cpu_baseline"""
    from oracle import pyorc as po
    out = {}
    for shape, (n, rd) in LATENCY_SHAPES.items():
        b = latency_inputs(shape, pairs)
        ro = po.ransac_opt(max_iterations=rd["max_iterations"], min_iterations=rd["min_iterations"], max_epipolar_error=2.0, max_reproj_error=16.0, estimate_shift=False)
        bo = po.bundle_opt(loss_type=4)
        cam = po.cam_flat(0, [800.0, 0.0, 0.0])
        po.lib()
        t0 = time.perf_counter()
        for i in range(pairs):
            po.estimate(0, b["x1"][i], b["x2"][i], b["d1"][i], b["d2"][i], ro, bo, cam, cam)
        out[shape] = 1e3 * (time.perf_counter() - t0) / pairs
    return out


def latency_block(cpu_ms, calls=30):
    """what a caller of the drop-in module waits for.  eval.py calls the estimator ONE pair per call and times each call
    (/root/reference/eval.py:152-154): median / p90 ms per call of poselib.estimate_monodepth_relative_pose at B = 1 on both latency shapes, and of the
    batch entry point (as_arrays) at B = 8 / 64 / 256 on the headline shape — host numpy buffers in, Python objects out, H2D and D2H inside.
    Never `value`."""
    from mdrp_amd import poselib
    bo = {"loss_type": "TRUNCATED_CAUCHY"}
    out = {"single_pair": {}, "batch_entry_point_headline_shape": {}, "calls": calls,
           "note": "wall time per call through the drop-in Python entry points from pageable numpy buffers (H2D, kernels, D2H, result objects); "
                   "cpu_port_ms_per_pair = oracle/*.c on one host core on the same pairs"}
    for shape, (n, rd) in LATENCY_SHAPES.items():
        b = latency_inputs(shape, 8)
        ts = []
        for k in range(calls + 3):
            i = k % 8
            t0 = time.perf_counter()
            g, info = poselib.estimate_monodepth_relative_pose(b["x1"][i], b["x2"][i], b["d1"][i], b["d2"][i], LATENCY_CAM, LATENCY_CAM, rd, bo)
            if k >= 3:
                ts.append(time.perf_counter() - t0)
        e = {"median_ms": 1e3 * float(np.median(ts)), "p90_ms": 1e3 * float(np.percentile(ts, 90)), "min_ms": 1e3 * float(np.min(ts)),
             "correspondences": n, "ransac_iterations": rd["max_iterations"], "last_num_inliers": int(info["num_inliers"])}
        if cpu_ms and shape in cpu_ms:
            e["cpu_port_ms_per_pair"] = cpu_ms[shape]
            e["speedup_vs_cpu_port"] = cpu_ms[shape] / e["median_ms"]
        out["single_pair"][shape] = e
    n, rd = LATENCY_SHAPES["headline_n2000_i10k"]
    b = latency_inputs("headline_n2000_i10k", 256)
    for B in (8, 64, 256):
        ts = []
        for k in range(8):
            t0 = time.perf_counter()
            poselib.estimate_monodepth_relative_pose_batch(b["x1"][:B], b["x2"][:B], b["d1"][:B], b["d2"][:B], LATENCY_CAM, LATENCY_CAM, rd, bo, as_arrays=True)
            if k >= 2:
                ts.append(time.perf_counter() - t0)
        out["batch_entry_point_headline_shape"][str(B)] = {"median_ms_per_call": 1e3 * float(np.median(ts)), "median_ms_per_pair": 1e3 * float(np.median(ts)) / B,
                                                           "pairs_per_s": B / float(np.median(ts))}
    return out


DUMP_BUDGET_BYTES = 63_000_000  # array bytes of --dump-outputs: under 64 MB with the .npy headers


def dump_outputs(out_dir, res, mask):
    """--dump-outputs: what the timed path handed its caller in the last step, as DIR/<name>.npy: every field of the result records (float64; the
    counters are exact there) and the inlier masks (float32, 0 / 1).  Masks that would exceed the budget are written for a fixed, seeded sample of
    pairs (rows listed in inlier_mask_pairs.npy) so that two runs with the same arguments write the same files."""
    from mdrp_amd import _capi
    os.makedirs(out_dir, exist_ok=True)
    arrays = {f"model_{k}": np.asarray(res["model"][k], dtype=np.float64) for k in _capi.MODEL_DTYPE.names}
    for k in ("refinements", "iterations", "num_inliers", "inlier_ratio", "model_score"):
        arrays[k] = np.asarray(res[k], dtype=np.float64)
    if mask is not None:
        B, n = mask.shape
        left = DUMP_BUDGET_BYTES - sum(a.nbytes for a in arrays.values())
        rows = np.arange(B)
        if B * n * 4 > left:
            keep = max(1, (left - 8 * B) // (n * 4 + 8))
            rows = np.sort(np.random.default_rng(0).choice(B, size=min(keep, B), replace=False))
            arrays["inlier_mask_pairs"] = rows.astype(np.float64)
        arrays["inlier_mask"] = mask[rows].astype(np.float32)
    assert sum(a.nbytes for a in arrays.values()) <= DUMP_BUDGET_BYTES
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)
    return sorted(arrays)


def visible_gpu_count():
    """GPUs this process could use, WITHOUT initialising one: torch.cuda.device_count() (reads the driver's topology under the ROCR_ / HIP_VISIBLE_DEVICES
    masks; no HIP context on this image)"""
    import torch
    return int(torch.cuda.device_count())


def self_launch(gpus, argv=None, out=None):
    """Run `python -m torch.distributed.run --nnodes=1 --nproc-per-node <gpus> bench.py <same arguments>` as a child process and return its exit code.
    On a box with fewer than `gpus` devices nothing is launched: the message says how many distinct devices there are, rc 3, within seconds."""
    import socket
    import subprocess
    argv = list(sys.argv[1:] if argv is None else argv)
    try:
        have = visible_gpu_count()
    except Exception as e:  # no torch / no driver: let the launcher fail with its own message rather than guess
        print(f"bench.py: cannot count GPUs ({e!r})", file=sys.stderr)
        have = None
    if have is not None and have < gpus:
        print(f"bench.py: --gpus {gpus} needs {gpus} distinct devices, this box shows distinct_devices = {have}: every rank needs its own GPU "
              f"(nothing was launched)", file=sys.stderr)
        return 3
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: what this pool's driver supports (RCCL over xGMI needs it)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    print("bench.py: launching " + " ".join(cmd), file=sys.stderr)
    return subprocess.run(cmd, env=env, stdout=out).returncode


# the measurements beyond the headline: (value with --full, value without).  An option given on the command line wins either way.
EXTRA_DEFAULTS = {"cpu_pairs": (96, 0), "inflight": (2, 1), "host_steps": (6, 0), "extra_configs": (5, 0), "c5_share": (12500, 0), "latency": (1, 0)}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=1024, help="image pairs per GPU per step (weak scaling)")
    ap.add_argument("--total-pairs", type=int, default=0,
                    help="BASELINE configs[4]: this many pairs in total, ceil(P/G) contiguous pairs per rank (strong scaling); "
                         "e.g. --total-pairs 100000 --gpus 8, or --total-pairs 12500 --gpus 1 for one rank's share")
    ap.add_argument("--workload", default="calib_p3p_n2000_i10k", choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, run every other measurement: CPU baselines, the in-flight and host-buffer steps and, on the default "
                         "run, the other configs, one rank's share of configs[4] and the latency block.  Without it these are skipped unless "
                         "their own option below asks for them")
    ap.add_argument("--cpu-pairs", type=int, default=None, help="pairs timed on the CPU baseline (default 96 with --full; 0 = skip)")
    ap.add_argument("--inflight", type=int, default=None, help="extra measurement at N = 1: the same steps with this many in flight "
                                                                 "(one handle + host thread each, mdrp_amd.pipeline; default 2 with --full); 1 = skip.  Never `value`.")
    ap.add_argument("--host-steps", type=int, default=None,
                    help="extra steps through the host-buffer (PCIe-inclusive) entry point, N = 1 only (default 6 with --full; 0 = skip)")
    ap.add_argument("--extra-configs", type=int, default=None,
                    help="after the headline, also measure BASELINE configs[2] and [3] (shared focal; varying focal N = 5000 with the shift flag) "
                         "with this many steps each and report them under `configs` (N = 1, default workload only; default 5 with --full; 0 = skip)")
    ap.add_argument("--c5-share", type=int, default=None,
                    help="pairs of the `c5_one_rank_share` entry under `configs` (one rank's share of BASELINE configs[4]: 100000 pairs / 8 GPUs = 12500; "
                         "N = 1 default run only; default 12500 there with --full; 0 = skip)")
    ap.add_argument("--latency", type=int, default=None,
                    help="single-pair / small-batch latency block on the line (N = 1 default run only; on with --full; 0 = skip)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the result records and inlier masks of the last step as DIR/<name>.npy (float64 / float32, "
                         "at most 64 MB; masks of a larger batch for a fixed sample of pairs).  N > 1: rank 0 writes the gathered records and its own masks")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    for k, (with_full, without) in EXTRA_DEFAULTS.items():
        if getattr(args, k) is None:
            setattr(args, k, with_full if args.full else without)
    return args


def main():
    args = parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the one-process-per-GPU job OURSELVES, as a CHILD process, before this process touches
        # the GPU or spends a second on the CPU baseline (never exec: a process that has initialised the GPU must not be replaced, and this one may
        # run under a profiler's preloaded library).  Rank 0's JSON line goes to our stdout untouched; our exit code is the child's.
        sys.exit(self_launch(args.gpus))

    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    default_run = world_env == 1 and args.workload == "calib_p3p_n2000_i10k" and args.total_pairs == 0 and args.batch == 1024
    extra_steps = args.extra_configs if default_run else 0
    cpu_line, cpu_extra = None, {}
    if world_env == 1 and args.cpu_pairs > 0:  # forks workers: before anything initialises the GPU
        cpu_line = cpu_baseline(args.workload, args.cpu_pairs)
        if extra_steps > 0:
            for wname, cp in EXTRA_CONFIGS:
                cpu_extra[wname] = cpu_baseline(wname, cp, multi=False)
    # this rank's block of the inputs, generated before anything initialises the GPU (forked workers): rank, world and the shard bounds
    # need no torch.  With --total-pairs a rank owns ceil(P/G) contiguous pairs (mdrp_amd.dist.shard_bounds).
    rank_env = int(os.environ.get("RANK", "0"))
    if args.total_pairs > 0:
        per_env = (args.total_pairs + world_env - 1) // world_env
        lo_env = min(rank_env * per_env, args.total_pairs)
        hi_env = min(lo_env + per_env, args.total_pairs)
    else:
        lo_env, hi_env = rank_env * args.batch, (rank_env + 1) * args.batch
    gen_workers = max(1, min(8, (os.cpu_count() or 1) // max(world_env, 1)))
    t_gen = time.perf_counter()
    pre_inputs = make_inputs_pool(args.workload, lo_env, max(hi_env - lo_env, 1), gen_workers)
    t_gen = time.perf_counter() - t_gen
    # one rank's share of BASELINE configs[4] (100 000 pairs over 8 GPUs = 12 500 pairs) on the N = 1 line: its inputs are generated here, by forked
    # workers, before the GPU is touched and outside every timed region (rank 3 of 8 would own pairs [37500, 50000): those)
    c5_pairs = max(args.c5_share, 0) if default_run else 0
    c5_first = 3 * c5_pairs
    c5_inputs, t_gen_c5 = None, 0.0
    if c5_pairs > 0:
        t_gen_c5 = time.perf_counter()
        c5_inputs = make_inputs_pool(args.workload, c5_first, c5_pairs, gen_workers)
        t_gen_c5 = time.perf_counter() - t_gen_c5
    want_latency = default_run and args.latency != 0
    cpu_lat = cpu_latency() if (want_latency and args.cpu_pairs > 0) else None
    pvr = port_vs_reference()
    for name, cl in [(args.workload, cpu_line)] + list(cpu_extra.items()):
        if cl is not None and name in pvr.get("workloads", {}):
            cl["port_vs_reference_binary"] = pvr["workloads"][name]

    import torch
    import torch.distributed as dist
    from mdrp_amd import _capi
    from mdrp_amd import dist as mdist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:  # (an external launcher's world disagrees with --gpus: the launcher wins, the line reports n_gpus = WORLD_SIZE)
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: running with {world} ranks", file=sys.stderr)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    # device ordinal: LOCAL_RANK modulo what this process can see (one visible device per rank under ROCR_/HIP_VISIBLE_DEVICES masks -> ordinal 0)
    dev_index = mdist.local_device_index(local_rank)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    ranks_seen = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        # which physical GPU each rank runs on, gathered over RCCL: the N > 1 line carries the proof that N distinct devices took part
        ranks_seen = mdist.gather_device_identities(dev_index)
        distinct = len({d for _, d in ranks_seen})
        if distinct != world:
            raise SystemExit(f"bench.py: {world} ranks on {distinct} distinct GPUs ({ranks_seen}): every rank needs its own device")

    strong = args.total_pairs > 0
    if strong:  # contiguous block of ceil(P/G) pairs per rank, generated by the rank that owns it (never replicated)
        total = args.total_pairs
        lo, hi, per = mdist.shard_bounds(total, rank, world)
    else:
        total = args.batch * world
        lo, hi, per = rank * args.batch, (rank + 1) * args.batch, args.batch
    assert (lo, hi) == (lo_env, hi_env)
    w = Workload(args.workload, lo, hi, per, dev_index, dev, inputs=pre_inputs)
    kind, n, iters, of, es, B, b, h = w.kind, w.n, w.iters, w.of, w.es, w.B, w.b, w.h
    rec_local = torch.zeros((per, mdist.RECORD_BYTES), dtype=torch.uint8, device=dev)  # this rank's block of the gather
    rec_all = torch.empty((world * per, mdist.RECORD_BYTES), dtype=torch.uint8, device=dev) if world > 1 else None

    def step():
        if B > 0:
            w.launch()
        if world > 1:  # final gather of the pose records over RCCL/xGMI, device to device: 136 B per pair
            if B > 0:
                h.copy_results_device(rec_local.data_ptr(), B)
            dist.all_gather_into_tensor(rec_all, rec_local)
            return None
        return h.fetch_results(B)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    dt, res, acc = timed_steps(step, barrier, args.steps, args.warmup, h.last_stats if B > 0 else None)
    last_mask = w.mask[:B].cpu().numpy() if args.dump_outputs else None  # the last timed step's masks, before anything else reuses the device
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        res = h.fetch_results(B) if B > 0 else np.zeros(0, dtype=_capi.RESULT_DTYPE)
        gathered = mdist._unpad(rec_all.cpu().numpy(), total, world, per)
        assert gathered.shape[0] == total
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, gathered.view(_capi.RESULT_DTYPE).reshape(-1) if world > 1 else res, last_mask)

    host_rate = None
    if world == 1 and args.host_steps > 0 and B > 0:  # the same step through mdrp_estimate_batch with HOST buffers: H2D of the
        xs = [b["x1"], b["x2"], b["d1"], b["d2"]]      # correspondences (48 B each) and D2H of records + masks inside the timed region
        c = w.cams if w.with_cams else None
        h.estimate_batch(kind, *xs, w.ro, w.bo, None, c, c)
        host_ts = []
        for _ in range(args.host_steps):  # timed call by call, the MEDIAN reported (the first calls after the staging buffers are made still page them in)
            th = time.perf_counter()
            h.estimate_batch(kind, *xs, w.ro, w.bo, None, c, c)
            host_ts.append(time.perf_counter() - th)
        host_rate = B / float(np.median(host_ts))

    pipelined = None
    if world == 1 and args.inflight > 1 and B > 0:  # consecutive steps with several in flight: an EXTRA key, `value` stays sequential
        import threading
        L = args.inflight
        hs = [_capi.Handle(dev_index) for _ in range(L)]
        masks = [torch.zeros((B, n), dtype=torch.uint8, device=dev) for _ in range(L)]
        torch.cuda.synchronize(dev)

        def lane(i, steps_):
            for _ in range(steps_):
                w.launch(hs[i], masks[i])
                hs[i].fetch_results(B)
        for i in range(L):
            lane(i, 1)
        per_lane = max(1, args.steps // L)
        torch.cuda.synchronize()
        tp = time.perf_counter()
        th = [threading.Thread(target=lane, args=(i, per_lane)) for i in range(L)]
        [t.start() for t in th]; [t.join() for t in th]
        torch.cuda.synchronize()
        dtp = time.perf_counter() - tp
        pipelined = {"in_flight": L, "steps": per_lane * L, "value": B * per_lane * L / dtp, "unit": "image-pairs/s", "ms_per_step": 1e3 * dtp / (per_lane * L),
                     "note": "the same steps, this many in flight at a time (one handle, stream set and host thread each: mdrp_amd.pipeline.BatchPipeline); "
                             "the next step's solver and sweeps fill the SIMDs the LM phases leave idle.  Not `value`."}
        for hh in hs:
            hh.close()

    # ---- BASELINE configs[2] and configs[3] on the same line (N = 1 default run): 1024 pairs each, same timing protocol
    extra = []
    if extra_steps > 0 and rank == 0:
        w.close()
        del w.x1, w.x2, w.d1, w.d2, w.mask
        for wname, _cp in EXTRA_CONFIGS:
            we = Workload(wname, 0, 1024, 1024, dev_index, dev)

            def step_e():
                we.launch()
                return we.h.fetch_results(we.B)
            dte, rese, acce = timed_steps(step_e, barrier, extra_steps, 1, we.h.last_stats)
            kern_e, roof_e, dom_e, top_e = rooflines_of(we, acce, extra_steps, dte)
            r = roof_e[dom_e]
            entry = {"workload": wname, "value": we.B * extra_steps / dte, "unit": "image-pairs/s", "ms_per_step": 1e3 * dte / extra_steps,
                     "steps": extra_steps, "warmup": 1, "pairs": we.B, "correspondences": we.n, "ransac_iterations": we.iters,
                     "estimator": ESTIMATOR_NAMES[we.kind], "monodepth_estimate_shift_flag": bool(we.es or wname in SHIFT_FLAG_ONLY), "outlier_fraction": we.of,
                     "roofline": {"kernel": r.get("kernel"), "bound": r.get("bound"), "achieved": r.get("achieved"), "peak": r.get("peak"), "unit": r.get("unit"),
                                  "frac": r.get("frac"), "traffic": r.get("traffic"), "avg_launch_ms": r.get("avg_launch_ms"),
                                  "launches_per_step": r.get("launches_per_step")},
                     "roofline_hbm_algorithmic": hbm_algorithmic(acce, extra_steps, dte),
                     "roofline_sweep_hbm": sweep_hbm_roofline(we, kern_e, extra_steps),
                     "kernel_ms_per_step": {k: v / extra_steps for k, v in kern_e.items()},
                     "lo_plus_final_ms_per_step": (kern_e["k_lo"] + kern_e["k_final"]) / extra_steps,
                     "mean_inlier_ratio": float(np.mean(rese["num_inliers"] / we.n))}
            if wname in cpu_extra:
                entry["cpu_baseline"] = cpu_extra[wname]
                entry["speedup_vs_cpu_1thread"] = entry["value"] / cpu_extra[wname]["value"]
            extra.append(entry)
            we.close()
            del we

    # ---- one rank's share of BASELINE configs[4] (12 500 pairs, one call, one pass) with the same timing protocol, then the latency block
    latency = None
    if default_run and rank == 0:
        if extra_steps <= 0:
            w.close()
            del w.x1, w.x2, w.d1, w.d2, w.mask
        torch.cuda.empty_cache()
        if c5_inputs is not None:
            c5_steps = 3
            wc = Workload(args.workload, c5_first, c5_first + c5_pairs, c5_pairs, dev_index, dev, inputs=c5_inputs)

            def step_c():
                wc.launch()
                return wc.h.fetch_results(wc.B)
            dtc, resc, accc = timed_steps(step_c, barrier, c5_steps, 1, wc.h.last_stats)
            kern_c, roof_c, dom_c, top_c = rooflines_of(wc, accc, c5_steps, dtc)
            rc_ = roof_c[dom_c]
            extra.append({"workload": "c5_one_rank_share_12500" if c5_pairs == 12500 else f"c5_one_rank_share_{c5_pairs}", "base_workload": args.workload,
                          "value": wc.B * c5_steps / dtc, "unit": "image-pairs/s", "ms_per_step": 1e3 * dtc / c5_steps, "steps": c5_steps, "warmup": 1,
                          "pairs": wc.B, "first_pair_index": c5_first, "correspondences": wc.n, "ransac_iterations": wc.iters, "estimator": ESTIMATOR_NAMES[wc.kind],
                          "monodepth_estimate_shift_flag": False, "outlier_fraction": wc.of,
                          "what": "BASELINE configs[4] as ONE rank sees it: 100000 pairs / 8 GPUs = 12500 pairs in one mdrp_estimate_batch_async call on resident buffers "
                                  "(tests/test_gpu_headline.py::test_one_rank_share_of_configs4_12500_pairs_vs_the_reference pins this size pair by pair)",
                          "roofline": {"kernel": rc_.get("kernel"), "bound": rc_.get("bound"), "achieved": rc_.get("achieved"), "peak": rc_.get("peak"), "unit": rc_.get("unit"),
                                       "frac": rc_.get("frac"), "traffic": rc_.get("traffic"), "avg_launch_ms": rc_.get("avg_launch_ms"),
                                       "launches_per_step": rc_.get("launches_per_step")},
                          "roofline_hbm_algorithmic": hbm_algorithmic(accc, c5_steps, dtc),
                          "kernel_ms_per_step": {k: v / c5_steps for k, v in kern_c.items()},
                          "lo_plus_final_ms_per_step": (kern_c["k_lo"] + kern_c["k_final"]) / c5_steps,
                          "mean_inlier_ratio": float(np.mean(resc["num_inliers"] / wc.n)),
                          "input_generation": {"seconds": t_gen_c5, "worker_processes": gen_workers, "pairs": c5_pairs,
                                               "note": "generated before the GPU is touched; outside every timed region"},
                          "cpu_baseline": cpu_line, "speedup_vs_cpu_1thread": (wc.B * c5_steps / dtc) / cpu_line["value"] if cpu_line else None})
            wc.close()
            del wc.x1, wc.x2, wc.d1, wc.d2, wc.mask, wc, c5_inputs
            torch.cuda.empty_cache()
        if want_latency:
            latency = latency_block(cpu_lat)

    if rank == 0:
        pairs = total * args.steps
        value = pairs / dt
        from mdrp_amd import synth
        from mdrp_amd.poselib import _quat_to_R
        R_err = None if kind == 5 else float(np.median([synth.rotation_error_deg(g["R"], _quat_to_R(r["model"]["q"])) for r, g in zip(res[:64], b["gt"][:64])]))
        steps = max(args.steps, 1)
        kern, rooflines, dominant, top = rooflines_of(w, acc, args.steps, dt)
        line = {
            "metric": "image-pairs/sec (2000 corrs, 10k RANSAC iters)", "value": value, "unit": "image-pairs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
            "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": args.workload, "pairs_per_gpu": per, "total_pairs": total, "correspondences": n, "ransac_iterations": iters,
                       "outlier_fraction": of, "estimator": ESTIMATOR_NAMES[kind],
                       "monodepth_estimate_shift": bool(es or args.workload in SHIFT_FLAG_ONLY),
                       "parallelism": f"{'ceil(P/G) contiguous pairs per rank' if strong else 'fixed pairs per rank'} x{world}, device-side all_gather of the 136-B records"},
            # the kernel with the largest event-timed share of the step (k_final excluded: fused, its interval overlaps k_lo); the MFMA figure of k_count stays beside it
            "roofline": rooflines[dominant],
            "roofline_count": rooflines["k_count"],
            "roofline_lm": rooflines.get("k_lo"),
            "roofline_final": rooflines.get("k_final"),
            # SURVEY.md 8(d)'s figure, explicit: 32 algorithmic bytes per (model x correspondence) evaluation of the CPU loop
            "roofline_hbm_algorithmic": hbm_algorithmic(acc, args.steps, dt),
            # ... and what north_star asks for by name: achieved HBM GB/s of the scoring sweep (PMC bytes, replayed) against the 8 TB/s peak
            "roofline_sweep_hbm": sweep_hbm_roofline(w, kern, args.steps),
            "kernel_ms_per_step": {k: v / steps for k, v in kern.items()},
            "lo_plus_final_ms_per_step": (kern["k_lo"] + kern["k_final"]) / steps,
            "fuse_timeouts": acc.get("fuse_timeouts", 0),
            "top_kernel_by_event_time": top,
            # what the CPU loop would do vs what runs: SURVEY.md 8(d)'s 32 B per evaluation is an ALGORITHMIC figure (the
            # correspondences stay in LDS / L2, HBM is not the bound), next to the evaluations actually executed
            "work": {"evals_algorithmic_per_step": acc.get("evals_algorithmic", 0) / args.steps, "algorithmic_bytes_per_eval": BYTES_PER_EVAL,
                     "algorithmic_GBs_whole_step": BYTES_PER_EVAL * acc.get("evals_algorithmic", 0) / dt / 1e9,
                     "evals_mfma_count_per_step": acc.get("evals_mfma", 0) / args.steps,
                     "evals_fp32_bound_per_step": acc.get("evals_bound", 0) / args.steps,
                     "evals_fp64_sweep_per_step": acc.get("evals_fp64", 0) / args.steps,
                     "k_count_ms_per_step": acc.get("count_ms", 0.0) / args.steps, "k_score_ms_per_step": acc.get("sweep_ms", 0.0) / args.steps,
                     "lm_fp64_flop_per_step": sum(r.get("fp64_flop_per_step", 0.0) for r in rooflines.values())},
            "input_generation": {"seconds": t_gen, "worker_processes": gen_workers, "pairs": B,
                                 "note": "synthetic inputs of this rank, generated before the GPU is touched; outside every timed region"},
            "quality": {"median_rotation_error_deg_first64": R_err,
                        "mean_inlier_ratio": float(np.mean(res["num_inliers"] / n)) if len(res) else None},
        }
        # every PMC-derived field of this line (`traffic`, `hbm_GBs`, `*_pmc`, roofline_sweep_hbm) is replayed from these files of the round's
        # profiler passes, accepted only because they record the source hash of the library that ran; files of another build are refused
        line["pmc_replayed_from"] = {"files": sorted(_PMC_USED), "library_source_hash": _capi.library_source_hash(),
                                     "fields": "roofline*.traffic, roofline*.hbm_GBs, roofline*.hbm_frac, *_pmc, roofline_sweep_hbm"} if _PMC_USED else None
        if _PMC_STALE:
            line["pmc_stale"] = sorted(_PMC_STALE)
        if ranks_seen is not None:
            line["rccl_ranks_seen"] = [r for r, _ in sorted(ranks_seen)]
            line["distinct_devices"] = len({d for _, d in ranks_seen})
            line["devices"] = [d for _, d in sorted(ranks_seen)]
        if extra:
            line["configs"] = extra
        if pipelined is not None:
            line["pipelined"] = pipelined
        if latency is not None:
            line["latency"] = latency
        if host_rate is not None:
            line["host_buffers"] = {"value": host_rate, "unit": "image-pairs/s", "ratio_to_resident": host_rate / value, "ms_per_call": [round(1e3 * t, 3) for t in host_ts],
                                    "note": "mdrp_estimate_batch with MDRP_MEM_HOST: pageable numpy buffers, H2D of 48 B per correspondence (in 256-pair slices on a copy "
                                            "stream, the long solver of a slice beside the next slices' copies) and D2H of records + inlier masks inside the timed region; "
                                            "median of the calls (PCIe-inclusive; never `value`)"}
        if cpu_line is not None:
            line["cpu_baseline"] = cpu_line
            line["speedup_vs_cpu_1thread"] = value / line["cpu_baseline"]["value"]
            pv = cpu_line.get("port_vs_reference_binary")
            if pv and pv.get("port_over_reference"):
                # the port is slower than the reference binary on the same core: the honest ratio is against the reference's rate
                line["speedup_vs_reference_binary_1thread_est"] = line["speedup_vs_cpu_1thread"] * pv["port_over_reference"]
            if "multi_process" in line["cpu_baseline"]:
                line["speedup_vs_cpu_multi_process"] = value / line["cpu_baseline"]["multi_process"]["value"]
        print(json.dumps(line))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
