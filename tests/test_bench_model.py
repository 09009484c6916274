"""CPU: the bench writes its model with bench.write_model, which must give synth.write_model_dir's files byte for byte (the
same inputs as every earlier bench run), and a plain run's model directory is its own and gone when the run ends."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_skip_matches_numpy_draw():
    import bench
    assert bench._skip_is_exact()
    # the walk's draws for every type it skips leave the stream where synth.random_blocks leaves it
    from powerserve_amd import gguf, synth
    for t in (gguf.Q4_0, gguf.Q4_K, gguf.Q5_K, gguf.Q6_K):
        for lead in (0, 1):
            a, b = np.random.default_rng(3), np.random.default_rng(3)
            for g in (a, b):
                g.integers(0, 2 ** 32, lead, dtype=np.uint32)
            synth.random_blocks(a, t, 64, 2048, 0.02)
            assert bench._skip_blocks(b, t, 64 * 2048 // gguf.BLOCK[t][0])
            assert np.array_equal(a.integers(0, 2 ** 32, 4, dtype=np.uint32), b.integers(0, 2 ** 32, 4, dtype=np.uint32)), (t, lead)


@pytest.mark.parametrize("preset,wt", [("tiny-llama", "Q4_K"), ("tiny-qwen2", "Q4_K"), ("small-llama-hs128", "Q4_K_M"), ("tiny-llama", "Q5_K_M"),
                                       ("tiny-llama", "Q4_0"), ("tiny-qwen2", "Q8_0"), ("tiny-llama", "F16"), ("small-llama", "Q6_K")])
@pytest.mark.parametrize("threads", [1, 3])
def test_write_model_is_synth_byte_for_byte(tmp_path, preset, wt, threads):
    import bench
    from powerserve_amd import gguf, synth
    wtype = {"Q4_K_M": synth.Q4_K_M, "Q5_K_M": synth.Q5_K_M}.get(wt) or gguf.NAME_TYPE[wt]
    a, b = str(tmp_path / "synth"), str(tmp_path / "bench")
    synth.write_model_dir(a, preset, wtype, n_ctx=256, seed=1234)
    bench.write_model(b, preset, wtype, 256, 1234, threads=threads)
    for f in ("model.json", os.path.join("ggml", "weights.gguf")):
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f


def test_run_model_directory_is_fresh_and_removed(tmp_path):
    """two runs' model directories differ, each holds the model while its run lasts and is gone once the process exits"""
    code = ("import argparse, os, sys; sys.path.insert(0, %r); import bench\n"
            "args = argparse.Namespace(model_dir=None, preset='tiny-llama', wtype='Q4_K', seed=1234, n_ctx=64)\n"
            "d = bench.ensure_model(args, 0, 1, lambda: None)\n"
            "assert os.path.exists(os.path.join(d, 'ggml', 'weights.gguf'))\n"
            "print(d)\n") % ROOT
    env = dict(os.environ, TMPDIR=str(tmp_path))
    dirs = []
    for _ in range(2):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        dirs.append(r.stdout.strip().splitlines()[-1])
    assert dirs[0] != dirs[1] and all(os.path.dirname(d) == str(tmp_path) for d in dirs)
    assert os.listdir(tmp_path) == []


def test_full_is_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse().full is True
