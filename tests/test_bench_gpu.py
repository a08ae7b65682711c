"""bench.py end to end on the GPU at a toy size: a plain run times exactly --steps steps and prints the headline alone (the
rooflines, per-kernel figures and the CPU baseline belong to --full), and --dump-outputs leaves the last step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--layers", "2",
                          "--batch", "8", "--ctx", "128", "--dump-outputs", str(tmp_path / "dump")],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["steps"] == 3 and r["warmup"] == 1 and r["unit"] == "tokens/s" and r["higher_is_better"] is True and r["dtype"] == "f16"
    assert r["ms_per_step"] > 0 and abs(r["value"] - 8 / (r["ms_per_step"] * 1e-3)) <= 1e-3 * r["value"]
    for key in ("roofline", "rooflines", "kernels", "hot_path_share_of_step", "cpu_baseline", "sweep"):
        assert key not in r
    tokens = np.load(tmp_path / "dump" / "next_tokens.npy")
    logits = np.load(tmp_path / "dump" / "logits.npy")
    assert tokens.dtype == np.float64 and tokens.shape == (8, )
    assert logits.dtype == np.float32 and logits.shape == (8, 128256)  # under the sampling threshold: every column
    assert np.isfinite(logits).all()
    # the ids are the greedy choice over these logits (fp16 logits tie: any column that holds the row's maximum is one)
    assert np.array_equal(logits[np.arange(8), tokens.astype(np.int64)], logits.max(-1))


# every single-GPU config at its default workload: (config, vocabulary of its lm_head, logits columns kept in the dump)
DEFAULT_WORKLOADS = [("int4", 128256, 49152), ("sparse24", 128256, 49152), ("fp8", 128256, 49152), ("gptq-exllama", 128256, 49152),
                     ("awq70b-tp8rank", 16032, 16032)]


@pytest.mark.parametrize("config,vocab,kept", DEFAULT_WORKLOADS, ids=[w[0] for w in DEFAULT_WORKLOADS])
def test_default_workload_outputs_are_finite_and_bounded(tmp_path, config, vocab, kept):
    """Each config at its own depth and batch: the synthetic weights must keep the fp16 residual stream of all layers in range
    (every logit finite), and the dump stays under 64 MB by sampling columns."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--config", config,
                          "--dump-outputs", str(tmp_path / "dump")], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    tokens = np.load(tmp_path / "dump" / "next_tokens.npy")
    logits = np.load(tmp_path / "dump" / "logits.npy")
    assert tokens.shape == (256, ) and logits.dtype == np.float32 and logits.shape == (256, kept)
    assert sum(os.path.getsize(tmp_path / "dump" / f) for f in os.listdir(tmp_path / "dump")) <= 64 * 10**6
    assert np.isfinite(logits).all()
    assert ((tokens >= 0) & (tokens < vocab) & (tokens == np.floor(tokens))).all()


def test_steps_sets_the_number_of_timed_steps(monkeypatch, capsys):
    """--steps N --warmup W replays the captured step W + N times and no more: a plain run launches nothing besides (counted at
    the graph's replay, in this process, at a toy size)."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    replays = []
    replay = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda g: (replays.append(1), replay(g))[1])
    for var in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    for steps, warmup in ((5, 2), (11, 0)):
        del replays[:]
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--layers", "2",
                                          "--batch", "8", "--ctx", "128"])
        bench.main()
        r = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
        assert len(replays) == steps + warmup
        assert r["steps"] == steps and r["warmup"] == warmup and r["ms_per_step"] > 0
