"""bench.py's contract: a plain run times exactly `--steps` iterations and nothing else;
`--dump-outputs DIR` writes the last timed step's outputs as float32 / float64 arrays."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def test_dump_outputs_names_dtypes_and_exact_keys(tmp_path):
    import bench

    _, _, ts = bench.build(torch.device("cpu"))
    metrics = {"losses/actor/mean": torch.tensor(0.25), "losses/critic/mean": 1.5}
    nbytes = bench.dump_outputs(str(tmp_path), ts, metrics)
    files = {p.name: np.load(p) for p in tmp_path.glob("*.npy")}
    assert sum(a.nbytes for a in files.values()) == nbytes <= bench.DUMP_MAX_BYTES
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    names = set(files)
    assert {"metrics.losses_actor_mean.npy", "metrics.losses_critic_mean.npy",
            "optimizer.m.npy", "optimizer.v.npy", "steps_taken.npy", "env_states.obs.npy",
            "variables.layers.0.mean.npy"} <= names
    params = dict(ts.networks.named_parameters())
    for n, p in params.items():
        assert np.array_equal(files[f"params.{n}.npy"], p.data.float().numpy()), n
    # a 64-bit key is stored as its exact [high, low] 32-bit halves
    hi, lo = (int(x) for x in files["rng_key.npy"])
    assert (hi << 32) + lo == int(ts.rng_key)


@pytest.mark.gpu
def test_plain_run_times_exactly_steps_and_dumps(dev, tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "4",
                        "--warmup", "3", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 4 and line["timing"]["windows"] == 1
    assert line["timing"]["iteration_ms"]["n"] == 3  # host sync to host sync within the window
    assert line["ms_per_step"] > 0 and line["unit"] == "env-steps/s" and line["higher_is_better"]
    assert line["dtype"] == "bf16"
    assert not {"windows", "roofline", "train_ppo", "configs", "cpu_baseline"} & set(line)
    arrays = {p.name: np.load(p) for p in out.glob("*.npy")}
    assert "metrics.losses_actor_mean.npy" in arrays and "steps_taken.npy" in arrays
    # 3 warm-up + 4 timed iterations of 4096 envs x 30 steps, as [high, low] halves
    hi, lo = arrays["steps_taken.npy"]
    assert (int(hi) << 32) + int(lo) == 7 * 4096 * 30
    assert float(arrays["metrics.losses_actor_mean.npy"]) == pytest.approx(
        line["final_losses"]["losses/actor/mean"])
