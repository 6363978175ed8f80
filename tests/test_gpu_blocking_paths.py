"""The blocking entry points that stage host buffers in one piece on the handle's stream (mdrp_capi_entry.h: stage_host_call, finish_blocking) -
mdrp_estimate_batch_prior, mdrp_refine_batch, mdrp_estimate_batch_ranked, mdrp_estimate_classic_ranked, mdrp_estimate_classic_prior, mdrp_refine_classic -
called through the raw symbols with MDRP_MEM_HOST and with MDRP_MEM_DEVICE on the same inputs: batch = 3, ragged n_per_pair = {0, 7, 64}, n_max = 64.
Records, masks and start-model outputs must be the same bytes.  On the same handle a second host call at n_max = 16 then follows the first: the staging
is sized and the call repointed per call, so it must return the bytes of the device call at n_max = 16 on a handle of its own.
(A mask's bytes at and past a pair's n are not part of the result: the host form copies them from the handle's buffer, the device form leaves the caller's.)

tests/test_gpu_classic_prosac.py and tests/test_gpu_from_models.py / test_gpu_classic_models.py compare host and device forms too, on single pairs and
through the asynchronous device form; the sliced host front of mdrp_estimate_batch[_budgets] has tests/test_gpu_boundary.py."""
import numpy as np
import pytest

import refusal_cases as rc

pytestmark = pytest.mark.gpu
N_LIST, N_MAX, N_SMALL = (0, 7, 64), 64, 16
START = ((64, "exact"),)  # start model / prior of the 64-record pair: its ground truth (the 7-record pair: perturbed), so that a refine call has inliers to report
ENTRIES = ("mdrp_estimate_batch_prior", "mdrp_refine_batch", "mdrp_estimate_batch_ranked", "mdrp_estimate_classic_ranked", "mdrp_estimate_classic_prior",
           "mdrp_refine_classic")


def _inputs(entry, capi, n_max):
    """the host arguments of `entry` by name (tests/refusal_cases.py SIGNATURES), cut to n_max columns"""
    classic = "classic" in entry
    if classic:
        import classic_models_cases as cases
        b = cases.batch(3, n_list=N_LIST, start=START)
        cam1, cam2 = cases.camera_records(3, b, capi)
    else:
        import from_models_cases as cases
        b = cases.batch("calib_p3p", n_list=N_LIST, start=START)
        cam1, cam2 = cases.camera_records(b, capi)
    a = {k: np.ascontiguousarray(b[k][:, :n_max]) for k in (("x1", "x2") if classic else ("x1", "x2", "d1", "d2"))}
    a.update(kind=3 if classic else 0, batch=len(N_LIST), n_max=n_max, npp=np.minimum(b["n"], n_max).astype(np.int32), cam1=cam1, cam2=cam2,
             models=np.ascontiguousarray(b["models"]).view(capi.MODEL_DTYPE).reshape(-1), stages=3, prior_space=0,
             scores=np.random.default_rng(11).uniform(0, 1, (len(N_LIST), n_max)),
             ropt=capi.ransac_opt_from_dict(dict(max_epipolar_error=2.0, max_reproj_error=16.0, max_iterations=200, min_iterations=50, seed=3)),
             bopt=capi.bundle_opt_from_dict({"loss_type": "TRUNCATED_CAUCHY"}))
    return a


def _call(entry, capi, h, a, mem):
    """the outputs of one blocking call as byte strings: records, the masks' valid rows, and the start-model outputs of a refine call"""
    import torch
    B, n_max = a["batch"], a["n_max"]
    a = dict(a, h=h._h, mem=mem, out=np.zeros(B, capi.RESULT_DTYPE), iscore=np.full(B, -1.0), iinl=np.full(B, -1, np.int32))
    mask = np.full((B, n_max), 7, np.uint8)
    if mem == capi.MEM_DEVICE:
        dev = torch.device("cuda", 0)
        for k in ("x1", "x2", "d1", "d2", "scores"):
            if k in a:
                a[k] = torch.from_numpy(a[k]).to(dev)
        a["models"] = torch.from_numpy(a["models"].view(np.uint8)).to(dev)
        mask = torch.from_numpy(mask).to(dev)
        torch.cuda.synchronize()
    a["mask"] = mask
    lib = capi.load_library()
    code = getattr(lib, entry)(*[rc.marshal(a[n]) for n in rc.SIGNATURES[entry].split()])
    assert code == 0, (entry, mem, lib.mdrp_last_error())
    if mem == capi.MEM_DEVICE:
        torch.cuda.synchronize()
        mask = mask.cpu().numpy()
    out = [a["out"].tobytes(), b"".join(mask[i, :n].tobytes() for i, n in enumerate(a["npp"]))]
    if "refine" in entry:
        out += [a["iscore"].tobytes(), a["iinl"].tobytes()]
    return out


@pytest.mark.parametrize("entry", ENTRIES)
def test_host_and_device_buffers_give_the_same_bytes(entry):
    from mdrp_amd import _capi as capi
    big, small = _inputs(entry, capi, N_MAX), _inputs(entry, capi, N_SMALL)
    h, fresh = capi.Handle(0), capi.Handle(0)
    try:
        host_big = _call(entry, capi, h, big, capi.MEM_HOST)
        host_small = _call(entry, capi, h, small, capi.MEM_HOST)  # behind the larger call, on its handle
        dev_big = _call(entry, capi, h, big, capi.MEM_DEVICE)
        dev_small = _call(entry, capi, fresh, small, capi.MEM_DEVICE)
    finally:
        h.close()
        fresh.close()
    assert host_big == dev_big
    assert host_small == dev_small
    records = np.frombuffer(host_big[0], capi.RESULT_DTYPE)
    # a run, not an empty answer: the start-model outputs of a refine call were written, an estimator found the 64-record pair's inliers
    assert records["num_inliers"][0] == 0
    if "refine" in entry:
        assert -1.0 not in np.frombuffer(host_big[2])[1:] and -1 not in np.frombuffer(host_big[3], np.int32)[1:]
    else:
        assert records["num_inliers"][2] > 7 and host_big[1].count(1) >= records["num_inliers"][2]
    assert host_small[0] != host_big[0]
