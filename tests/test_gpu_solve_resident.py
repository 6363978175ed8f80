"""The residency of the solver that runs beside a first chunk's sweeps is scheduling only (MDRP_SOLVE_RESIDENT: one-wavefront workgroups that each
reserve dynamic LDS, sched::solver_reservation in mdrp_schedule.h): results with 0 (uncapped), 1 and 2 wavefronts per SIMD are byte-identical, through
the resident call and through the sliced host-buffer front; and the runtime's occupancy query places exactly 4 R such workgroups on a compute unit for
the reservation the rule grants (no kernel runs)."""
import numpy as np
import pytest

import test_gpu_first_filter as ff

SLICED_B, SLICED_N = 512, 40    # two 256-pair slices of the host-buffer front


def _sliced_inputs():
    from mdrp_amd import _capi, synth
    x1, x2 = np.zeros((SLICED_B, SLICED_N, 2)), np.zeros((SLICED_B, SLICED_N, 2))
    d1, d2 = np.ones((SLICED_B, SLICED_N)), np.ones((SLICED_B, SLICED_N))
    for i in range(SLICED_B):
        p = synth.make_pair(88000 + i, SLICED_N, noise_px=0.5, depth_noise=0.02, outlier_frac=ff.OUTLIERS[i % 3])
        x1[i], x2[i], d1[i], d2[i] = p["x1"], p["x2"], p["d1"], p["d2"]
    cams = np.zeros(SLICED_B, dtype=_capi.CAMERA_DTYPE)
    cams["params"][:, 0] = 800.0
    return x1, x2, d1, d2, cams


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [False, True])
def test_solver_residency_does_not_change_results(monkeypatch, shift):
    from mdrp_amd import _capi
    h = _capi.Handle(0)
    try:
        runs = {r: ff._run(h, monkeypatch, 0, shift, {"MDRP_FIRST_PICK": "48", "MDRP_SOLVE_RESIDENT": r}) for r in ("0", "1", "2")}
    finally:
        h.close()
    ref, ref_mask, st = runs["0"]
    assert st["first_chunk"] == 128 and int(ref["num_inliers"].max()) > 300
    for r in ("1", "2"):
        res, mask, _ = runs[r]
        assert res.tobytes() == ref.tobytes(), (shift, r, [i for i in range(ff.B) if res[i:i + 1].tobytes() != ref[i:i + 1].tobytes()][:16])
        assert np.array_equal(mask, ref_mask), (shift, r)


@pytest.mark.gpu
def test_solver_residency_does_not_change_results_through_the_sliced_host_front(monkeypatch):
    from mdrp_amd import _capi
    x1, x2, d1, d2, cams = _sliced_inputs()
    ro = _capi.ransac_opt_from_dict(dict(ff.RO, max_iterations=ff.ITS, min_iterations=ff.ITS))
    bo = _capi.bundle_opt_from_dict(ff.BO)
    h = _capi.Handle(0)
    out = {}
    try:
        for r in ("0", "1", "2"):
            ff._env(monkeypatch, {"MDRP_FIRST_PICK": "48", "MDRP_SOLVE_RESIDENT": r})
            res, mask = h.estimate_batch(0, x1, x2, d1, d2, ro, bo, None, cams, cams)
            out[r] = (res.copy(), mask.copy())
            assert h.last_stats()["first_chunk"] == 128
    finally:
        h.close()
    assert int(out["0"][0]["num_inliers"].max()) >= 20
    for r in ("1", "2"):
        assert out[r][0].tobytes() == out["0"][0].tobytes() and np.array_equal(out[r][1], out["0"][1]), r


@pytest.mark.gpu
@pytest.mark.parametrize("solver", [0, 1])  # P3P and the shift solver: the two whose launch may be capped
def test_the_reservation_places_four_workgroups_per_simd_and_resident_wavefront(solver):
    from mdrp_amd import _capi
    lds0, bytes0, free = _capi.solver_residency(solver, 0)
    assert bytes0 == 0 and free >= 8 and lds0 >= 65536          # uncapped: what registers allow, at least two wavefronts per SIMD
    for r in (1, 2):
        lds, reserve, wgs = _capi.solver_residency(solver, r)
        assert lds == lds0 and 0 < reserve <= lds // (4 * r) and (4 * r + 1) * reserve > lds
        assert wgs == 4 * r, (solver, r, reserve, wgs)
    assert _capi.solver_residency(solver, 2, keep_free_bytes=2 * lds0)[1] == 0  # more to keep free than there is: no cap
