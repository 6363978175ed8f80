"""Case builders for the dense front end's tests (include/mdrp_dense.h): batches of warps, certainties and depth maps in float64 NumPy,
the NumPy definition (mdrp_amd/frontend.py sample_dense_numpy) applied to them as the device sees them, and a synthetic pair for the estimate.
Shared by tests/test_dense_host.py (no GPU) and tests/test_gpu_dense*.py; every reference is computed once and left unchanged."""
import numpy as np

H1, W1, H2, W2 = 45, 61, 39, 70          # non-square, different, no multiple of any grid > 1
BLOCK_ROWS = 1024                        # mdrp_dense.h DENSE_BLOCK_ROWS
R_BLOCKS = 3 * BLOCK_ROWS + 17           # more than one block, no multiple of the block or of a wavefront
R_SMALL = 300                            # less than one block
SPECIAL_COORDS = (-1.0, 1.0, np.nextafter(-1.0, 0.0), np.nextafter(1.0, 0.0), np.nextafter(-1.0, -2.0), np.nextafter(1.0, 2.0), np.nan, np.inf, -np.inf,
                  0.0, -0.0, float(np.nextafter(np.float32(1.0), np.float32(0.0))), float(np.nextafter(np.float32(-1.0), np.float32(-2.0))))  # (the last two: float32's neighbours)
SPECIAL_CERTAINTIES = (0.0, -0.0, -0.25, np.nan, np.inf, -np.inf, 5e-324, 1e-310, np.nextafter(0.05, 0.0), 0.05, np.nextafter(0.05, 1.0), 1.0, 1.5, 1e300,
                       1.0 / 65536.0, np.nextafter(1.0 / 65536.0, 0.0), 2.5 / 65536.0)


def make_pair(seed, R, kind="mixed"):
    """one pair in float64, normalized coordinates: warp (R, 4), certainty (R,), depth maps.  kind: "mixed" (tied and small certainties, border rows,
    infinite and NaN depths) | "zero" (every certainty zero) | "duplicates" (five rows of weight 65536 among rows of weight 1)"""
    rng = np.random.default_rng(4100 + seed)
    warp = rng.uniform(-1.04, 1.04, (R, 4))
    u = rng.uniform(0.0, 1.0, R)
    cert = np.where(rng.uniform(size=R) < 0.5, np.round(u * 16.0) / 16.0, u * 0.05)  # ties at the sixteenths (0 among them) | below the threshold
    dm1, dm2 = rng.uniform(1.0, 6.0, (H1, W1)), rng.uniform(1.0, 6.0, (H2, W2))
    for dm in (dm1, dm2):  # a tenth of the pixels infinite (both maps: about 1 % of the rows both-infinite), some NaN and -inf
        r = rng.uniform(size=dm.shape)
        dm[r < 0.10] = np.inf
        dm[(r >= 0.10) & (r < 0.12)] = np.nan
        dm[(r >= 0.12) & (r < 0.14)] = -np.inf
    if kind == "zero":
        cert[:] = 0.0
    elif kind == "duplicates":
        cert[:] = 1e-7  # floor(1e-7 * 65536) = 0: weight 1
        cert[rng.choice(R, 5, replace=False)] = 1.0
    else:
        at = rng.choice(R, len(SPECIAL_COORDS) * 4 + len(SPECIAL_CERTAINTIES), replace=False)
        for i, v in enumerate(SPECIAL_COORDS):  # every special coordinate once in every column, the row's other points well inside
            for col in range(4):
                row = at[4 * i + col]
                warp[row] = rng.uniform(-0.9, 0.9, 4)
                warp[row, col] = v
                cert[row] = 0.75
        for i, v in enumerate(SPECIAL_CERTAINTIES):
            row = at[4 * len(SPECIAL_COORDS) + i]
            warp[row] = rng.uniform(-0.9, 0.9, 4)
            cert[row] = v
    return warp, cert, dm1, dm2


def stack(pairs):
    B = len(pairs)
    return {"warp": np.stack([p[0] for p in pairs]), "cert": np.stack([p[1] for p in pairs]), "dm1": np.stack([p[2] for p in pairs]),
            "dm2": np.stack([p[3] for p in pairs]), "c1": np.array([W1 / 2.0, H1 / 2.0]) + 0.125 * np.arange(B)[:, None], "c2": np.tile([W2 / 2.0, H2 / 2.0], (B, 1))}


_batches = {}

# ---- the wide batches (tests/test_gpu_dense_wide.py, tests/test_scan_runs_host.py): row counts at which k_dense_scan's threads hold runs of more than
# one block (per = ceil(nblk / 256) > 1) and the weight sum T passes 2^32.  name: (R, make_pair's seeds); every pair is of kind "mixed".
SCAN_THREADS = 256                       # mdrp_dense.h DENSE_THREADS: the scan's workgroup
R_WIDE = 256 * BLOCK_ROWS + 17           # the smallest R with nblk = 257, per = 2: threads 0-127 hold two blocks, thread 128 one, the last block is ragged
R_WIDE3 = 512 * BLOCK_ROWS + 1           # nblk = 513, per = 3: thread 171's lo is clamped to nblk; the last block is one row
R_MAX = 1 << 22                          # mdrp_dense.h MDRP_DENSE_MAX_ROWS: nblk = 4096, per = 16, every thread busy
WIDE_BATCHES = {"wide": (R_WIDE, (30, 31)), "wide3": (R_WIDE3, (30,)), "max": (R_MAX, (30,))}
N_WIDE = 16384                           # mdrp_dense.h's largest n: with expansion 4, m1_max = 65536 and ntile = 256


def scan_run(n, threads=SCAN_THREADS):
    """the run length of the chunked scans (k_dense_scan, k_recon_scan, k_scene_scan): a thread sums per = ceil(n / threads) consecutive values"""
    return -(-int(n) // threads)


def nblk(R):
    return -(-int(R) // BLOCK_ROWS)


def batch(name):
    """B = 3 each.  "blocks": R = 3 blocks + 17, a pair of zero certainties between two live ones, pair 2 = pair 0 (the same pair at two batch
    positions); "small": R below one block; "duplicates": the duplicate case, pairs 0 and 1.  The names of WIDE_BATCHES: B = 2 or 1 mixed pairs of
    that many rows"""
    if name not in _batches:
        if name in WIDE_BATCHES:
            R, seeds = WIDE_BATCHES[name]
            b = stack([make_pair(s, R) for s in seeds])
        elif name == "blocks":
            a = make_pair(0, R_BLOCKS)
            b = stack([a, make_pair(1, R_BLOCKS, "zero"), a])
        elif name == "small":
            b = stack([make_pair(10, R_SMALL), make_pair(11, R_SMALL), make_pair(12, R_SMALL)])
        elif name == "duplicates":
            b = stack([make_pair(20, R_BLOCKS, "duplicates"), make_pair(21, R_BLOCKS, "duplicates"), make_pair(22, R_BLOCKS)])
        else:
            raise KeyError(name)
        for v in b.values():
            v.setflags(write=False)
        _batches[name] = b
    return _batches[name]


def as_seen(b, warp_dtype=np.float32, cert_dtype=np.float32, depth_dtype=np.float32, coords="normalized"):
    """the batch as the device sees it: cast to the dtypes; coords "pixel": the warp in pixel coordinates (computed in float64, then cast)"""
    warp = b["warp"]
    if coords == "pixel":
        warp = (warp + 1.0) * (0.5 * np.array([W1, H1, W2, H2], dtype=np.float64))
    with np.errstate(over="ignore"):  # (1e300 is inf in float32: a non-candidate there)
        return warp.astype(warp_dtype), b["cert"].astype(cert_dtype), b["dm1"].astype(depth_dtype), b["dm2"].astype(depth_dtype)


_refs = {}


def reference(name, n, centres=True, warp_dtype=np.float32, cert_dtype=np.float32, depth_dtype=np.float32, coords="normalized", **kw):
    """frontend.pad_dense_pairs of sample_dense_numpy per pair of batch(name), computed once per argument set"""
    from mdrp_amd import frontend
    key = (name, n, centres, np.dtype(warp_dtype).name, np.dtype(cert_dtype).name, np.dtype(depth_dtype).name, coords, tuple(sorted(kw.items())))
    if key not in _refs:
        b = batch(name)
        warp, cert, dm1, dm2 = as_seen(b, warp_dtype, cert_dtype, depth_dtype, coords)
        out = frontend.pad_dense_pairs([frontend.sample_dense_numpy(warp[i], cert[i], dm1[i], dm2[i], n, coords=coords, center1=b["c1"][i] if centres else None,
                                                                    center2=b["c2"][i] if centres else None, **kw) for i in range(len(warp))], n)
        for a in out:
            a.setflags(write=False)
        _refs[key] = out
    return _refs[key]


def candidates(name, i, **kw):
    """weights of pair i of a batch as the float32 device sees it"""
    from mdrp_amd import frontend
    warp, cert, dm1, dm2 = as_seen(batch(name))
    return frontend.dense_candidates(warp[i], cert[i], dm1[i], dm2[i], **kw)[0]


# ---- a synthetic pair for the estimate: synth.make_pair correspondences scaled into two maps, their depths painted at the truncated pixel (as
# tests/test_gpu_frontend.py paints them), one warp row per correspondence; outliers get a low certainty
EH1, EW1, EH2, EW2 = 480, 640, 400, 720
EA1, EC1 = 0.35, (320.0, 240.0)  # pixel = A * synth pixel + C: a camera with focal A * 800 and principal point C
EA2, EC2 = 0.30, (360.0, 200.0)
ECAM1 = {"model": "SIMPLE_PINHOLE", "width": EW1, "height": EH1, "params": [EA1 * 800.0, *EC1]}
ECAM2 = {"model": "SIMPLE_PINHOLE", "width": EW2, "height": EH2, "params": [EA2 * 800.0, *EC2]}


def estimate_pair(seed, rows=2200):
    from mdrp_amd import synth
    rng = np.random.default_rng(4700 + seed)
    p = synth.make_pair(7300 + seed, rows, noise_px=0.0, depth_noise=0.0, outlier_frac=0.2)
    pt1, pt2 = EA1 * p["x1"] + np.array(EC1), EA2 * p["x2"] + np.array(EC2)
    dm1, dm2 = rng.uniform(1.0, 6.0, (EH1, EW1)), rng.uniform(1.0, 6.0, (EH2, EW2))
    inside = (pt1[:, 0] >= 0) & (pt1[:, 0] < EW1) & (pt1[:, 1] >= 0) & (pt1[:, 1] < EH1) & (pt2[:, 0] >= 0) & (pt2[:, 0] < EW2) & (pt2[:, 1] >= 0) & (pt2[:, 1] < EH2)
    for m in np.flatnonzero(inside):
        dm1[int(pt1[m, 1]), int(pt1[m, 0])] = p["d1"][m]
        dm2[int(pt2[m, 1]), int(pt2[m, 0])] = p["d2"][m]
    warp = np.concatenate([pt1, pt2], axis=1)  # pixel coordinates: exact
    # a correspondence whose pixel was painted over by a later one reads a foreign depth: it is an outlier as well
    lost = ~inside | (dm1[pt1[:, 1].astype(int).clip(0, EH1 - 1), pt1[:, 0].astype(int).clip(0, EW1 - 1)] != p["d1"]) \
        | (dm2[pt2[:, 1].astype(int).clip(0, EH2 - 1), pt2[:, 0].astype(int).clip(0, EW2 - 1)] != p["d2"])
    cert = np.where(p["is_outlier"] | lost, rng.uniform(1e-6, 1e-5, rows), rng.uniform(0.5, 1.0, rows))  # weight 1 against 65536
    return {"warp": warp, "cert": cert, "dm1": dm1, "dm2": dm2, "truth": p}


_estimate_batches = {}


def estimate_batch(B=3):
    if B not in _estimate_batches:
        pairs = [estimate_pair(i) for i in range(B)]
        b = {k: np.stack([q[k] for q in pairs]) for k in ("warp", "cert", "dm1", "dm2")}
        b["truth"] = [q["truth"] for q in pairs]
        _estimate_batches[B] = b
    return _estimate_batches[B]


# ---- calls on a given handle, as byte strings (the GPU tests' refusal and history checks): the descriptor is poselib's own
SAMPLER_DEFAULTS = dict(seed=0, coords="normalized", threshold=0.05, balanced=True, expansion=4, grid=8, min_count=2, filter="both_inf", ranked=False,
                        center1=None, center2=None)
ERO = {"max_iterations": 200, "min_iterations": 200, "max_epipolar_error": 0.7, "max_reproj_error": 5.6, "seed": 5}
EBO = {"loss_type": "TRUNCATED_CAUCHY"}


def tensors(*arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
    torch.cuda.synchronize()  # (a handle of these tests has a stream of its own)
    return out


def descriptor(t, n, **kw):
    """poselib's validated descriptor of four device tensors (warp, certainty, depth maps) -> (descriptor, what it points into, B)"""
    from mdrp_amd import poselib
    a = dict(SAMPLER_DEFAULTS, **kw)
    desc, keep, B, _ = poselib._dense_descriptor(*t, n, a["seed"], a["coords"], a["threshold"], a["balanced"], a["expansion"], a["grid"], a["min_count"], a["filter"],
                                                 a["ranked"], a["center1"], a["center2"])
    return desc, keep, B


def sample_on(h, t, n, **kw):
    """mdrp_sample_dense on handle h: (x1, x2, d1, d2, rows, score, counts) as byte strings"""
    import torch
    desc, keep, B = descriptor(t, n, **kw)
    out = [torch.full((B, n, 2), -7.0, dtype=torch.float64, device="cuda:0") for _ in range(2)] + [torch.full((B, n), -7.0, dtype=torch.float64, device="cuda:0") for _ in range(2)]
    rows = torch.full((B, n), -7, dtype=torch.int32, device="cuda:0")
    score = torch.full((B, n), -7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    cnt = h.sample_dense(desc, B, *[o.data_ptr() for o in out], rows.data_ptr(), score.data_ptr())
    h.synchronize()
    return tuple(o.cpu().numpy().tobytes() for o in out + [rows, score]) + (cnt.tobytes(),)


def estimate_on(h, kind, t, n, cams=(None, None), ro=ERO, **kw):
    """mdrp_estimate_dense_async on handle h: (records, record mask, rows, counts) as byte strings"""
    import torch
    from mdrp_amd import _capi, poselib
    desc, keep, B = descriptor(t, n, **kw)
    mask = torch.zeros((B, n), dtype=torch.uint8, device="cuda:0")
    rows = torch.full((B, n), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    desc.rows_out = rows.data_ptr()
    c1, c2 = (None if c is None else poselib._camera_records(c, B) for c in cams)
    cnt = h.estimate_dense_device(kind, desc, B, _capi.ransac_opt_from_dict(ro), _capi.bundle_opt_from_dict(EBO), c1, c2, mask.data_ptr())
    res = h.fetch_results(B)
    return (res.tobytes(), mask.cpu().numpy().tobytes(), rows.cpu().numpy().tobytes(), cnt.tobytes())
