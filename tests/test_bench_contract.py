"""The driver's bench contract: torchrun-launched bench.py must emit exactly
one valid JSON line from rank 0 (CPU/gloo here; the driver runs the same
invocation on MI355X boxes)."""

import json
import os
import subprocess
import sys

import pytest

TINY = [
    "--override", "algo.world_model.recurrent_model.recurrent_state_size=64",
    "--override", "algo.world_model.transition_model.hidden_size=64",
    "--override", "algo.world_model.representation_model.hidden_size=64",
    "--override", "algo.world_model.encoder.cnn_channels_multiplier=4",
    "--override", "algo.dense_units=64",
    "--override", "algo.mlp_layers=1",
    "--override", "algo.world_model.discrete_size=8",
    "--override", "algo.world_model.stochastic_size=8",
    "--override", "algo.per_rank_batch_size=2",
    "--override", "algo.per_rank_sequence_length=8",
    "--override", "algo.horizon=3",
    "--override", "env.num_envs=1",
]


@pytest.mark.timeout(600)
def test_bench_two_rank_gloo_emits_single_json(tmp_path):
    env = dict(os.environ)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = f"{repo}:{env.get('PYTHONPATH', '')}"
    env["MASTER_ADDR"] = "127.0.0.1"
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
         "--master-addr", "127.0.0.1", "--master-port", "29611",
         os.path.join(repo, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", *TINY],
        capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=570,
    )
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    json_lines = [l for l in out.stdout.splitlines() if l.strip().startswith("{")]
    assert len(json_lines) == 1, out.stdout
    rec = json.loads(json_lines[0])
    assert rec["metric"] == "env_frames_per_sec"
    assert rec["n_gpus"] == 2 and rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["value"] > 0 and rec["higher_is_better"] is True
    assert rec["scaling"] == "weak" and rec["data"] == "synthetic"
    assert "ms_per_step" in rec and "config" in rec


@pytest.mark.timeout(600)
def test_bench_single_rank_default(tmp_path):
    """Plain `python bench.py` (the driver's N=1 run) with tiny overrides."""
    env = dict(os.environ)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = f"{repo}:{env.get('PYTHONPATH', '')}"
    out = subprocess.run(
        [sys.executable, os.path.join(repo, "bench.py"), "--steps", "2", "--warmup", "1", *TINY],
        capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=570,
    )
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    json_lines = [l for l in out.stdout.splitlines() if l.strip().startswith("{")]
    assert len(json_lines) == 1, out.stdout
    rec = json.loads(json_lines[0])
    assert rec["n_gpus"] == 1 and rec["metric"] == "env_frames_per_sec"


@pytest.mark.timeout(600)
def test_bench_full_and_dump_outputs(tmp_path):
    """`--full --dump-outputs DIR`: same result line, plus the last timed
    step's outputs as float .npy files within the 64 MB budget."""
    import numpy as np

    env = dict(os.environ)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = f"{repo}:{env.get('PYTHONPATH', '')}"
    dump = tmp_path / "dump"
    out = subprocess.run(
        [sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
         "--full", "--dump-outputs", str(dump), *TINY],
        capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=570,
    )
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    json_lines = [l for l in out.stdout.splitlines() if l.strip().startswith("{")]
    assert len(json_lines) == 1, out.stdout
    rec = json.loads(json_lines[0])
    assert rec["metric"] == "env_frames_per_sec" and rec["unit"] == "frames/s"
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["higher_is_better"] is True
    files = sorted(dump.glob("*.npy"))
    names = {f.stem for f in files}
    assert {"player_actions", "train_rec_loss", "train_policy_loss", "train_value_loss",
            "params_world_model", "params_actor", "params_critic"} <= names, names
    assert sum(f.stat().st_size for f in files) <= 64 * 1000 * 1000
    for f in files:
        a = np.load(f)
        assert a.dtype in (np.float32, np.float64), (f.name, a.dtype)
        assert a.size > 0 and np.isfinite(a).all(), f.name
    # same arguments, second run: the fp32 CPU path has no atomics, so the
    # outputs must be bit-identical (on the GPU: equal to bf16 rounding)
    dump2 = tmp_path / "dump2"
    out2 = subprocess.run(
        [sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
         "--dump-outputs", str(dump2), *TINY],
        capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=570,
    )
    assert out2.returncode == 0, out2.stdout[-2000:] + out2.stderr[-2000:]
    assert {f.name for f in dump2.glob("*.npy")} == {f.name for f in files}
    for f in files:
        assert np.array_equal(np.load(f), np.load(dump2 / f.name)), f.name


def test_dump_outputs_samples_large_arrays(tmp_path):
    """An array over its share of the budget is cut to a fixed sample: the
    same elements on every call, and the whole dump stays within 64 MB."""
    import numpy as np
    import torch

    import bench

    big = torch.arange(20_000_000, dtype=torch.float32)
    for d in ("a", "b"):
        bench._dump_outputs(tmp_path / d, {"big": big, "big2": big * 2, "small": np.ones((3, 2))})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.size < big.numel() and np.array_equal(a, b)
    assert np.array_equal(np.load(tmp_path / "a" / "big2.npy"), 2 * a)  # same indices
    assert np.load(tmp_path / "a" / "small.npy").shape == (3, 2)
    assert sum(f.stat().st_size for f in (tmp_path / "a").glob("*.npy")) <= 64 * 1000 * 1000


@pytest.mark.timeout(600)
def test_bench_ppo_algo_single_rank(tmp_path):
    """`python bench.py --algo ppo` emits one valid contract JSON line."""
    env = dict(os.environ)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = f"{repo}:{env.get('PYTHONPATH', '')}"
    out = subprocess.run(
        [sys.executable, os.path.join(repo, "bench.py"), "--algo", "ppo", "--steps", "1",
         "--warmup", "0", "--override", "algo.rollout_steps=8", "--override", "env.num_envs=2",
         "--override", "algo.per_rank_batch_size=8", "--override", "algo.update_epochs=1"],
        capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=570,
    )
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    json_lines = [l for l in out.stdout.splitlines() if l.strip().startswith("{")]
    assert len(json_lines) == 1, out.stdout
    rec = json.loads(json_lines[0])
    assert rec["metric"] == "env_frames_per_sec" and rec["config"]["model"] == "ppo_pixel"
    assert rec["value"] > 0 and rec["scaling"] == "weak"
