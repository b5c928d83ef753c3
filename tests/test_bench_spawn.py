"""bench.py --gpus N started without a launcher spawns N ranks itself (ref:scripts/train_SMB_decoder.sh:123-153)
and relays rank 0's line; driven here with a fake launcher, no GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "helpers", "fake_launcher.py")


def _run(extra_env, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(extra_env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          env=env, timeout=300)


def test_spawn_relays_rank0_line():
    r = _run({"GAMER_BENCH_LAUNCHER": f"{sys.executable} {FAKE}"}, "--gpus", "4", "--steps", "3", "--warmup", "1")
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1                          # ONE JSON line on stdout, the child's noise went to stderr
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 4
    assert rec["argv"] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]


def test_spawn_fails_when_fewer_ranks_joined():
    r = _run({"GAMER_BENCH_LAUNCHER": f"{sys.executable} {FAKE} --lie 1"}, "--gpus", "2")
    assert r.returncode == 4
    assert r.stdout.strip() == ""


def test_gpus_mismatch_inside_a_launcher_is_an_error():
    r = _run({"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}, "--gpus", "4")
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


def test_no_devices_is_an_error_not_a_one_rank_run():
    # this container has no GPU: asking for 2 must fail loudly instead of printing an n_gpus=1 record
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a box with fewer than 2 devices")
    r = _run({}, "--gpus", "2")
    assert r.returncode == 2 and r.stdout.strip() == ""


def test_batch_arithmetic():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args(["--gpus", "8"])
    assert a.batch == 128 and not a.weak            # north star: global 1024 over 8 GPUs
    a = bench.parse_args(["--gpus", "8", "--weak"])
    assert a.batch == 1024 and a.weak               # BASELINE configs[2]
    a = bench.parse_args(["--batch", "128"])
    assert a.batch == 128 and a.weak
    with pytest.raises(SystemExit):
        bench.parse_args(["--gpus", "3"])           # 1024 is not divisible by 3
    cmd = bench.launcher_command(8, 1234, ["--gpus", "8"])
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=8" in cmd and "127.0.0.1" in cmd


def test_steps_and_optional_legs_arguments():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "0", "--dump-outputs", "out"])
    assert a.steps == 7 and a.warmup == 0 and a.dump_outputs == "out"
    assert not a.secondary and not a.cpu_baseline            # the headline leg alone unless asked
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--secondary", "--no-secondary"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_contract_line_is_small_and_keeps_the_headline():
    sys.path.insert(0, ROOT)
    import bench
    fam = {"bound": "mfma", "kernel": "k" * 150, "achieved": 96.9, "peak": 833.3, "unit": "TFLOP/s", "frac": 0.116,
           "algorithmic_GBps": None, "hbm_frac": None, "traffic": 1.0e10, "traffic_source": "s" * 120,
           "traffic_profiled_command": "c" * 200, "algorithmic_flop_per_launch": 4.0e11, "avg_launch_ms": 4.1,
           "ms_per_step": 33.2, "flop_convention": "f" * 200}
    rows = [{"kernel": f"family_{i}", "ms_per_step": 1.0, "launches_per_step": 8.0, "avg_launch_ms": 0.1, "tflops": 50.0,
             "algorithmic_GBps": 900.0} for i in range(60)]
    result = {"metric": "m", "value": 5092.4, "unit": "sequences/s", "n_gpus": 1, "steps": 20, "warmup": 5,
              "ms_per_step": 201.1, "dtype": "f32", "data": "synthetic", "config": {"workload": "w" * 600, "seq_len": 505},
              "roofline": dict(fam, gemm=dict(fam), all_gemm_tflops=246.2, step_algorithmic_tflops=142.0,
                               step_frac_of_matrix_peak=0.17),
              "kernels": rows, "kernel_choice": {"env": {f"GAMER_{i}": "1" for i in range(50)}}, "loss": 5.6,
              "secondary": [{"name": f"leg{i}", "ms_per_step": 30.0, "value": 4000.0, "kernels": rows[:8]} for i in range(9)]
              + [{"name": "broken", "error": "RuntimeError()"}],
              "secondary_eval": [{"name": "decode", "ms_per_batch": 24.7, "value": 10361.0}]}
    line = json.dumps(bench.contract_line(result))
    assert len(line) < 4096, len(line)
    back = json.loads(line)
    assert back["ms_per_step"] == 201.1 and back["steps"] == 20 and back["value"] == 5092.4 and back["config"]["seq_len"] == 505
    assert back["roofline"]["frac"] == 0.116 and back["roofline"]["gemm"]["achieved"] == 96.9 and "kernels" not in back
    assert back["secondary"]["leg3"] == [30.0, 4000.0] and back["secondary"]["broken"] == "error"
    assert back["secondary_eval"] == {"decode": [24.7, 10361.0]}
    assert json.loads(json.dumps(bench.contract_line(dict(result, roofline=None))))["roofline"] is None


def test_dump_outputs_writes_a_fixed_float_sample(tmp_path):
    sys.path.insert(0, ROOT)
    import types

    import numpy as np
    import torch

    import bench
    assert 2 * bench.DUMP_SAMPLE * 4 + 4096 <= 64 << 20        # --dump-outputs stays within 64 MB
    n = 10_000
    eng = types.SimpleNamespace(flat_p=torch.arange(n, dtype=torch.float32), flat_g=2.0 * torch.arange(n, dtype=torch.float32))
    shapes = bench.dump_outputs(str(tmp_path / "a"), eng, torch.tensor([1.5]), sample=1000)
    assert shapes == {"loss": [1], "params": [1000], "grads": [1000]}
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in shapes}
    assert all(a.dtype == np.float32 for a in got.values()) and float(got["loss"][0]) == 1.5
    p = got["params"]
    assert bool((np.diff(p) > 0).all()) and p[0] >= 0 and p[-1] < n                # distinct positions, ascending
    assert np.array_equal(got["grads"], 2.0 * p)                                   # the same positions in both buffers
    bench.dump_outputs(str(tmp_path / "b"), eng, torch.tensor([1.5]), sample=1000)
    assert all(np.array_equal(got[k], np.load(tmp_path / "b" / f"{k}.npy")) for k in shapes)     # seeded: run to run
    bench.dump_outputs(str(tmp_path / "c"), eng, 2.0, sample=n)
    assert np.array_equal(np.load(tmp_path / "c" / "params.npy"), eng.flat_p.numpy())      # small buffers: every position
