"""bench.py's host logic that needs no GPU: the N > 1 self-launch."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_n_without_a_launcher_refuses_cleanly_on_a_box_with_fewer_devices():
    """`python bench.py --gpus 8` with WORLD_SIZE unset on a box that has fewer than 8 GPUs (this container: none): non-zero exit, the
    distinct_devices message, no JSON line, no CPU baseline run, no hang — within seconds (the time is `import torch`)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "1", "--warmup", "0"], env=env, capture_output=True, text=True, timeout=120)
    dt = time.perf_counter() - t0
    assert r.returncode == 3, (r.returncode, r.stderr[-400:])
    assert "distinct_devices" in r.stderr and "--gpus 8" in r.stderr
    assert r.stdout.strip() == ""
    assert dt < 60, dt  # (a cold `import torch` on a fresh container is the only cost; 2-3 s warm)


def test_self_launch_starts_one_child_launcher_and_forwards_its_exit_code(monkeypatch, tmp_path):
    """with enough devices the parent starts `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py <args>` as a
    CHILD (subprocess, never exec), hands its own arguments on unchanged and returns the child's code"""
    sys.path.insert(0, ROOT)
    import bench
    seen = {}

    class R:
        returncode = 7

    def fake_run(cmd, env=None, stdout=None):
        seen["cmd"], seen["env"] = cmd, env
        return R()
    monkeypatch.setattr(bench, "visible_gpu_count", lambda: 8)
    monkeypatch.setattr(subprocess, "run", fake_run)
    rc = bench.self_launch(4, ["--gpus", "4", "--steps", "2", "--warmup", "1"])
    assert rc == 7
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "2", "--warmup", "1"]
    assert seen["env"].get("HSA_ENABLE_IPC_MODE_LEGACY") == "0"


def test_dump_outputs_writes_float_arrays_within_64_mb_and_samples_a_fixed_set_of_pairs(tmp_path):
    """--dump-outputs: every record field as float64, the masks as float32; a batch whose masks exceed the budget (one rank's share of
    BASELINE configs[4] at N = 5000) is written for the same seeded sample of pairs on every run"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from mdrp_amd import _capi
    rng = np.random.default_rng(5)
    for B, n in ((1024, 2000), (12500, 5000)):
        res = np.zeros(B, dtype=_capi.RESULT_DTYPE)
        res["num_inliers"] = rng.integers(0, n, B)
        res["model"]["t"] = rng.normal(size=(B, 3))
        mask = (rng.random((B, n)) < 0.5).astype(np.uint8)
        dirs = [tmp_path / f"{B}_a", tmp_path / f"{B}_b"]
        for d in dirs:
            bench.dump_outputs(str(d), res, mask)
        files = sorted(os.listdir(dirs[0]))
        assert files == sorted(os.listdir(dirs[1])) and "inlier_mask.npy" in files and "model_t.npy" in files
        assert sum(os.path.getsize(dirs[0] / f) for f in files) <= 64_000_000
        for f in files:
            a, b = np.load(dirs[0] / f), np.load(dirs[1] / f)
            assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
        assert np.array_equal(np.load(dirs[0] / "num_inliers.npy"), res["num_inliers"].astype(np.float64))
        assert np.array_equal(np.load(dirs[0] / "model_t.npy"), res["model"]["t"])
        rows = np.load(dirs[0] / "inlier_mask_pairs.npy").astype(np.int64) if "inlier_mask_pairs.npy" in files else np.arange(B)
        assert (B == 1024) == (len(rows) == B)
        assert np.array_equal(np.load(dirs[0] / "inlier_mask.npy"), mask[rows].astype(np.float32))


def test_a_plain_run_skips_every_extra_measurement_and_full_restores_them():
    """a plain `bench.py --gpus 1 --steps N --warmup W` times the headline alone; --full brings back every other measurement with the
    defaults it had, and an option given on the command line wins either way"""
    sys.path.insert(0, ROOT)
    import bench
    extras = ("cpu_pairs", "inflight", "host_steps", "extra_configs", "c5_share", "latency")
    plain = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not plain.full and (plain.steps, plain.warmup) == (20, 5)
    assert {k: getattr(plain, k) for k in extras} == {"cpu_pairs": 0, "inflight": 1, "host_steps": 0, "extra_configs": 0, "c5_share": 0, "latency": 0}
    full = bench.parse_args(["--full", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert full.full and (full.steps, full.warmup) == (20, 5)
    assert {k: getattr(full, k) for k in extras} == {"cpu_pairs": 96, "inflight": 2, "host_steps": 6, "extra_configs": 5, "c5_share": 12500, "latency": 1}
    assert bench.parse_args(["--cpu-pairs", "8"]).cpu_pairs == 8
    assert bench.parse_args(["--full", "--cpu-pairs", "0", "--inflight", "1"]).cpu_pairs == 0
