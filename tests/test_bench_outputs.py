"""bench.py's plain run and --dump-outputs: the writer's formats and size cap (no GPU), and
on the GPU a small plain run whose line carries the headline alone, times the --steps it
was given, and whose dumped outputs repeat bit for bit in a second process."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY_KEYS = ("roofline", "constraint_solver", "cpu_baseline", "obs_max_rel_err", "per_step_api",
                  "c2_single_cylinder_256", "c3_random_actions", "c3_scripted_mix_only", "c1_single_env_200_steps",
                  "c5_device_policy_rollout", "overflow_envs", "finite")


def test_dump_outputs_formats(tmp_path):
    """Every array lands as <name>.npy with its shape and values; float64 stays float64,
    ints, bools and float32 become float32."""
    import bench
    arrays = {"f32": np.linspace(-1, 1, 12, dtype=np.float32).reshape(3, 4),
              "f64": np.linspace(0, 1e-9, 5),
              "i32": np.arange(6, dtype=np.int32).reshape(2, 3),
              "flag": np.array([True, False, True])}
    written = bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == sorted(k + ".npy" for k in arrays)
    for k, a in arrays.items():
        got = np.load(tmp_path / "d" / (k + ".npy"))
        assert got.dtype == (np.float64 if k == "f64" else np.float32), k
        assert list(got.shape) == list(a.shape) == written[k], k
        np.testing.assert_array_equal(got, a.astype(got.dtype))


def test_dump_outputs_size_cap(tmp_path):
    """Over the byte budget an array is cut to a fixed sample of its elements in index order
    (the same ones on every call); arrays within their share stay whole; the total stays
    inside the budget."""
    import bench
    big = np.arange(1000, dtype=np.float32).reshape(100, 10)        # value == flat index
    small = np.arange(8, dtype=np.float64)
    cap = 1024                                                      # 512 bytes each
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small}, max_bytes=cap)
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    np.testing.assert_array_equal(a, b)
    assert a.shape == (128,) and (np.diff(a) > 0).all() and a.min() >= 0 and a.max() < 1000
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    assert a.nbytes + small.nbytes <= cap


@pytest.mark.gpu
def test_gpu_plain_run_dumps_repeatable_outputs(tmp_path):
    """Two plain runs in two processes: 64 envs, --steps 6 with --rollout 4, so launches of
    R = gcd(6, 4) = 2 env-steps (three timed, and ceil(3 / 2) = 2 for --warmup 3).  Each prints
    the headline alone, with steps = 6, the warmup it ran = 4 env-steps and value consistent
    with ms_per_step, and writes obs / reward / done and the [R, envs] episode records of the
    last timed launch, float32, finite, and equal bit for bit between the two runs.  A third
    process drives the same 4 + 6 env-steps one per launch (--rollout 0 --warmup 4): the fused
    launches equal the per-step API bit for bit, so its outputs are the same only if each run
    stepped the batch exactly warmup + steps times."""
    from conftest import gpu_available
    if not gpu_available():
        pytest.skip("no GPU")
    n, K, W, rollout = 64, 6, 3, 4
    R = math.gcd(K, rollout)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    W_run = -(-W // R) * R
    runs = {"a": (W, rollout), "b": (W, rollout), "per_step": (W_run, 0)}
    procs = [subprocess.Popen([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(K),
                               "--warmup", str(w), "--envs", str(n), "--rollout", str(r),
                               "--dump-outputs", str(tmp_path / d)],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
             for d, (w, r) in runs.items()]
    lines = []
    for p in procs:
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, err[-2000:]
        lines.append(json.loads(out.strip().split("\n")[-1]))
    ps_line = lines.pop()
    assert ps_line["steps"] == K and ps_line["warmup_steps_run"] == W_run
    for line in lines:
        for key in HEADLINE_KEYS:
            assert key in line, key
        for key in FULL_ONLY_KEYS:
            assert key not in line, key
        assert line["steps"] == K and line["n_gpus"] == 1 and line["higher_is_better"] is True
        assert line["warmup"] == W and line["warmup_steps_run"] == W_run
        assert f"launches of {R} env-steps" in line["config"]["workload"]
        assert line["ms_per_step"] > 0
        # both are rounded from the same wall time: ms_per_step to 0.001 ms, value to 0.1
        ms = line["ms_per_step"]
        assert abs(line["value"] - n / ms * 1e3) <= (0.0005 / (ms - 0.0005) + 1e-9) * line["value"] + 0.1
    shapes = {"obs": (n, None), "reward": (n,), "done": (n,),
              "episode_return": (R, n), "episode_length": (R, n), "episode_success": (R, n)}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in shapes)
    total = 0
    for k, shape in shapes.items():
        a, b = np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))
        assert a.dtype == np.float32 and np.isfinite(a).all(), k
        assert a.ndim == len(shape) and all(want in (None, got) for got, want in zip(a.shape, shape)), (k, a.shape)
        assert list(a.shape) == lines[0]["dumped_outputs"][k], k
        np.testing.assert_array_equal(a, b, err_msg=k)
        ps = np.load(tmp_path / "per_step" / (k + ".npy"))          # [1, n] records: the last env-step's
        np.testing.assert_array_equal(a[-1:] if k.startswith("episode") else a, ps, err_msg=k + " vs per-step")
        total += a.nbytes
    assert total <= 64 << 20
    assert np.abs(np.load(tmp_path / "a" / "obs.npy")).max() > 0        # sensor readings, not an untouched buffer
