"""F16 weights on the CPU: synth writes and gguf reads them, the other types' random streams are untouched, the reference's F16 mul_mat
is an F32 mul_mat on fp16-rounded inputs for K % 32 == 0 (what the GPU tests at real dimensions rely on), and the fixture generator
reproduces the committed fixtures byte for byte."""
import hashlib
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_golden_f16", os.path.join(ROOT, "tools", "gen_golden_f16.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_random_blocks_f16_rows():
    from powerserve_amd import gguf, synth
    w = synth.random_blocks(np.random.default_rng(3), gguf.F16, 5, 96, std=0.1)
    assert w.dtype == np.uint8 and w.size == 5 * 96 * 2
    h = w.view(np.float16).astype(np.float32)
    assert np.isfinite(h).all() and 0.05 < h.std() < 0.2


@pytest.mark.parametrize("wt", ["F16", "F16_Q8_0"])
def test_synth_writes_and_gguf_reads_f16_model(tmp_path, wt):
    from powerserve_amd import gguf, synth
    t = synth.F16 if wt == "F16" else synth.F16_Q8_0
    mj = synth.write_model_dir(str(tmp_path), "tiny-llama", t, n_ctx=64, seed=5, embd_type=gguf.F32)
    assert mj["model_id"] == f"tiny-llama-{wt}"
    rd = gguf.GGUFReader(os.path.join(str(tmp_path), "ggml", "weights.gguf"))
    ti = rd.tensors["blk.0.attn_q.weight"]
    assert ti.type == gguf.F16 and rd.data("blk.0.attn_q.weight").size == 256 * 256 * 2
    assert rd.tensors["blk.1.ffn_down.weight"].type == (gguf.F16 if wt == "F16" else gguf.Q8_0)
    assert rd.tensors["output.weight"].type == gguf.F16 and rd.tensors["token_embd.weight"].type == gguf.F32


def test_other_types_streams_unchanged(tmp_path):
    """the committed Q8_0 e2e fixture's GGUF is still what synth writes"""
    from powerserve_amd import gguf, synth
    g = np.load(os.path.join(GOLD, "e2e_tiny-llama_Q8_0.npz"))
    synth.write_model_dir(str(tmp_path), "tiny-llama", gguf.Q8_0, n_ctx=int(g["n_ctx"]), seed=int(g["seed"]))
    assert hashlib.sha256(open(os.path.join(str(tmp_path), "ggml", "weights.gguf"), "rb").read()).hexdigest() == str(g["gguf_sha256"])


@pytest.mark.parametrize("K", [256, 896, 4096])
def test_ref_f16_mul_mat_is_f32_on_rounded_inputs(ref, oracle, K):
    from powerserve_amd import gguf, synth
    rng = np.random.default_rng(K)
    N, bs = 24, 3
    w = synth.random_blocks(rng, gguf.F16, N, K, std=0.3)
    x = rng.standard_normal((bs, K)).astype(np.float32)
    want = ref.mul_mat(gguf.F16, w, K, N, x)
    w32 = w.view(np.float16).astype(np.float32)
    x16 = x.astype(np.float16).astype(np.float32)
    got = oracle.mul_mat(gguf.F32, w32.view(np.uint8), K, N, x16)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(ref.mul_mat(gguf.F32, w32.view(np.uint8), K, N, x16).view(np.uint32), want.view(np.uint32))


def test_ref_f16_leftovers_are_summed_in_double(ref, oracle):
    """K = 100: the n % 32 tail of ggml_vec_dot_f16 goes through a double -- an F32 mul_mat does not model it, the fixture does"""
    from powerserve_amd import gguf
    gen = _gen()
    w, x = gen.mul_mat_inputs(100, 3)
    g = np.load(os.path.join(GOLD, "f16_mul_mat.npz"))
    assert np.array_equal(ref.mul_mat(gguf.F16, w, 100, gen.MUL_N, x).view(np.uint32), g["y_100_3"].view(np.uint32))


def test_generator_reproduces_committed_fixtures(ref, tmp_path):
    gen = _gen()
    gen.main(str(tmp_path))
    for f in sorted(os.listdir(str(tmp_path))):
        assert open(os.path.join(str(tmp_path), f), "rb").read() == open(os.path.join(GOLD, f), "rb").read(), f
