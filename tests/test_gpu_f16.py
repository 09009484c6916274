"""F16 weights on the MI355X, every result on bits: the activation rounding against numpy.float16, ps_hip_mul_mat against the real
reference's vectors (tests/golden/f16_mul_mat.npz, K = 100 included) and against the oracle's F32 mul_mat on fp16-rounded inputs at real
dimensions (equal to the reference's F16 mul_mat for K % 32 == 0: tests/test_f16_weights.py), get_embedding, whole models against the real
LlamaModel / Qwen2Model::forward (tests/golden/e2e_f16_*.npz, tools/gen_golden_f16.py), the token-tree forward, the captured decode step,
super-chunk prefill and the contract build."""
import ctypes as C
import hashlib
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F32, F16 = 0, 1
E2E = ["tiny-llama_F16", "tiny-qwen2_F16", "tiny-llama_F16_Q8_0"]


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def _gen():
    spec = importlib.util.spec_from_file_location("gen_golden_f16", os.path.join(ROOT, "tools", "gen_golden_f16.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _mul_mat(ctx, w, K, N, x):
    W = ctx.upload_weight(F16, w, K, N)
    dx, dy = ctx.to_device(np.ascontiguousarray(x, dtype=np.float32)), ctx.empty((x.shape[0], N))
    ctx.check(ctx.L.ps_hip_mul_mat(ctx.h, C.byref(dy.tensor()), C.byref(W.tensor()), C.byref(dx.tensor())))
    y = dy.numpy()
    W.free(); dx.free(); dy.free()
    return y


def test_type_helpers(ctx):
    assert ctx.L.ps_hip_vec_dot_type(F16) == F16
    w = np.zeros(24 * 100 * 2, dtype=np.uint8)
    W = ctx.upload_weight(F16, w, 100, 24)
    assert W.gguf_bytes == 24 * 100 * 2
    W.free()


@pytest.mark.parametrize("K", [7, 256, 4099])
def test_act_rounding_is_numpy_float16(ctx, K):
    rng = np.random.default_rng(K)
    rows = 4
    x = (rng.standard_normal((rows, K)) * 10).astype(np.float32)
    x[0, ::3] = rng.uniform(-70000, 70000, x[0, ::3].size)       # around and beyond the fp16 range (65504; inf from 65520)
    x[0, :4] = [65519.996, 65520.0, -65520.0, 65504.0]
    x[1] *= 1e-6                                                  # fp16 subnormals
    x[1, :3] = [2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -26]           # ties at the bottom of the subnormals
    k = np.arange(K, dtype=np.float32)
    x[2] = (1.0 + (2 * (k % 512) + 1) * 2.0 ** -11).astype(np.float32)  # every value halfway between two fp16 neighbours
    x[3, ::2] = 0.0
    x[3, 1::4] = -0.0
    dx, out = ctx.to_device(x), ctx.empty((rows, K), np.uint16)
    ctx.check(ctx.L.ps_hip_quantize_act(ctx.h, F16, dx.ptr, K, rows, out.ptr))
    assert np.array_equal(out.numpy(), x.astype(np.float16).view(np.uint16))


def test_mul_mat_golden(ctx):
    gen = _gen()
    g = np.load(os.path.join(GOLD, "f16_mul_mat.npz"))
    for K in gen.MUL_K:
        for bs in gen.MUL_BS:
            w, x = gen.mul_mat_inputs(K, bs)
            key = f"{K}_{bs}"
            assert hashlib.sha256(w.tobytes() + x.tobytes()).hexdigest() == str(g["sha_" + key])
            got = _mul_mat(ctx, w, K, gen.MUL_N, x)
            assert np.array_equal(got.view(np.uint32), g["y_" + key].view(np.uint32)), key


@pytest.mark.parametrize("K,N", [(4096, 14336), (14336, 4096), (2048, 8192), (896, 4864), (4864, 896)])
@pytest.mark.parametrize("bs", [1, 2, 16, 128, 512])
def test_mul_mat_real_dims(ctx, oracle, K, N, bs):
    """every output of the GPU; the oracle checks all rows, or (wide batches of the two 8B matrices: its CPU time) 768 rows spread over the matrix,
    the first and last 16-row tiles included"""
    from powerserve_amd import synth
    rng = np.random.default_rng(K + N + bs)
    w = synth.random_blocks(rng, F16, N, K, std=0.02)
    x = rng.standard_normal((bs, K)).astype(np.float32)
    got = _mul_mat(ctx, w, K, N, x)
    rows = np.arange(N)
    if bs >= 128 and K * N > 2048 * 8192:
        rows = np.unique(np.concatenate([np.arange(16), np.arange(N - 16, N), rng.choice(N, 736, replace=False)]))
    w32 = w.view(np.float16).reshape(N, K)[rows].astype(np.float32)
    want = oracle.mul_mat(F32, w32.view(np.uint8).reshape(-1), K, len(rows), x.astype(np.float16).astype(np.float32), n_threads=16)
    assert np.array_equal(got[:, rows].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("K,N,bs", [(2048, 8192, 128), (896, 4864, 17), (4100, 256, 5)])
def test_matrix_core_and_valu_batches_agree(ctx, K, N, bs):
    """the two batch forms (ps_hip_debug_set 10: matrix cores, default / VALU chains) give the same bits"""
    from powerserve_amd import synth
    rng = np.random.default_rng(K * 7 + bs)
    w = synth.random_blocks(rng, F16, N, K, std=0.02)
    x = rng.standard_normal((bs, K)).astype(np.float32)
    a = _mul_mat(ctx, w, K, N, x)
    assert ctx.L.ps_hip_debug_set(10, 1) == 0
    try:
        b = _mul_mat(ctx, w, K, N, x)
    finally:
        ctx.L.ps_hip_debug_set(10, 0)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_get_embedding_f16(ctx):
    from powerserve_amd import hip as H, synth
    K, V = 96, 50
    w = synth.random_blocks(np.random.default_rng(9), F16, V, K)
    W = ctx.upload_weight(F16, w, K, V)
    toks = np.array([0, 49, 7, 7], dtype=np.int32)
    out = ctx.empty((4, K))
    ctx.check(ctx.L.ps_hip_get_embedding(ctx.h, C.byref(out.tensor()), C.byref(W.tensor()), toks.ctypes.data_as(C.c_void_p), 4))
    assert np.array_equal(out.numpy(), w.view(np.float16).reshape(V, K)[toks].astype(np.float32))
    W.free()


def _model(ctx, tmp_path, g, max_batch=16):
    from powerserve_amd import hip, synth
    d = str(tmp_path / "m")
    synth.write_model_dir(d, str(g["preset"]), int(g["wt"]), n_ctx=int(g["n_ctx"]), seed=int(g["seed"]), embd_type=int(g["embd_type"]))
    assert _sha(os.path.join(d, "ggml", "weights.gguf")) == str(g["gguf_sha256"])
    return hip.Model(ctx, d, max_batch=max_batch), d


@pytest.mark.parametrize("name", E2E)
@pytest.mark.parametrize("mode", [0, 1])
def test_e2e_golden(ctx, tmp_path, name, mode):
    """ids, per-step logits and batch logits of the real reference's forward; mode 0 = captured decode step, 1 = eager launches"""
    g = np.load(os.path.join(GOLD, f"e2e_f16_{name}.npz"))
    m, _ = _model(ctx, tmp_path, g)
    m.set_mode(mode)
    prompt = g["prompt"]
    assert np.array_equal(m.generate(prompt, 8, 24), g["ids"])
    m.reset()
    for lo in range(0, 20, 8):
        hi = min(lo + 8, 20)
        m.forward(prompt[lo:hi], np.arange(lo, hi), lm_head=False)
    cur = int(prompt[-1])
    for s in range(24):
        lg, _ = m.forward([cur], [m.position], lm_head=True)
        assert np.array_equal(lg[0].view(np.uint32), g["logits"][s].view(np.uint32)), s
        cur = int(g["ids"][s])
    m.reset()
    lg, _ = m.forward(prompt[:9], np.arange(9), lm_head=True)
    assert np.array_equal(lg.view(np.uint32), g["batch_logits"].view(np.uint32))
    m.close()


def test_decode_greedy_replay_equals_eager_steps_and_prefill_superchunks(ctx, tmp_path):
    g = np.load(os.path.join(GOLD, "e2e_f16_tiny-llama_F16.npz"))
    m, _ = _model(ctx, tmp_path, g, max_batch=64)
    prompt = np.random.default_rng(5).integers(0, 512, 61).astype(np.int32)
    m.prefill(prompt[:-1], 8)  # super-chunks of 8-token reference chunks
    k_sc = [m.k_cache(L)[:60].copy() for L in range(2)]
    replay = m.decode_greedy(int(prompt[-1]), 12)
    m.reset()
    for lo in range(0, 60, 8):
        m.forward(prompt[lo:min(lo + 8, 60)], np.arange(lo, min(lo + 8, 60)), lm_head=False)
    for L in range(2):
        assert np.array_equal(m.k_cache(L)[:60].view(np.uint32), k_sc[L].view(np.uint32))
    m.set_mode(1)
    cur, eager = int(prompt[-1]), []
    for _ in range(12):
        _, am = m.forward([cur], [m.position], lm_head=True, want_logits=False)
        cur = int(am[0])
        eager.append(cur)
    assert np.array_equal(replay, eager)
    m.close()


def test_tree_forward_golden(ctx, tmp_path):
    g = np.load(os.path.join(GOLD, "tree_forward_f16.npz"))
    gm, _ = _model(ctx, tmp_path, g, max_batch=32)
    prefix, P = g["prefix"], len(g["prefix"])
    for lo in range(0, P, 32):
        gm.forward(prefix[lo:min(lo + 32, P)], np.arange(lo, min(lo + 32, P)), lm_head=False)
    for h in g["hidden"]:
        gm.kv_mask(int(h), False)
    got, am = gm.forward_tree(g["tokens"], g["rope"], g["tree"], lm_head=True, want_logits=True, advance=False)
    assert np.array_equal(got.view(np.uint32), g["logits"].view(np.uint32))
    for u, a in enumerate(g["accept"]):
        if a != u:
            gm.kv_move(P + u, P + int(a))
    gm.kv_advance(len(g["accept"]))
    step, _ = gm.forward_tree(g["next"], [P + len(g["accept"])], None, lm_head=True, want_logits=True, advance=False)
    assert np.array_equal(step.view(np.uint32), g["step_logits"].view(np.uint32))
    gm.close()


def test_f16_perf_mode_runs_on_an_f16_model(ctx, tmp_path):
    """mode bit 5 (not bit-exact) on an F16 model: the perf GEMMs take the F16 matrices themselves (csrc/model.hip ensure_perf16); runs, finite logits"""
    g = np.load(os.path.join(GOLD, "e2e_f16_tiny-llama_F16.npz"))
    m, _ = _model(ctx, tmp_path, g, max_batch=64)
    prompt = g["prompt"]
    m.set_mode(32)
    m.forward(prompt[:16], np.arange(16), lm_head=False)
    lg, _ = m.forward(prompt[16:17], [16], lm_head=True)
    assert np.isfinite(lg).all()
    m.close()


_CONTRACT = r"""
import ctypes as C, importlib.util, os, sys, numpy as np
sys.path.insert(0, sys.argv[1])
from powerserve_amd import hip, synth
spec = importlib.util.spec_from_file_location("gen", os.path.join(sys.argv[1], "tools", "gen_golden_f16.py"))
gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
G = os.path.join(sys.argv[1], "tests", "golden")
g = np.load(os.path.join(G, "f16_mul_mat.npz"))
ctx = hip.Ctx(0)
assert ctx.L.ps_hip_build_contract() == 1
for K in gen.MUL_K:
    for bs in gen.MUL_BS:
        w, x = gen.mul_mat_inputs(K, bs)
        W = ctx.upload_weight(1, w, K, gen.MUL_N)
        dx, dy = ctx.to_device(x), ctx.empty((bs, gen.MUL_N))
        ctx.check(ctx.L.ps_hip_mul_mat(ctx.h, C.byref(dy.tensor()), C.byref(W.tensor()), C.byref(dx.tensor())))
        assert np.array_equal(dy.numpy().view(np.uint32), g[f"y_{K}_{bs}"].view(np.uint32)), (K, bs)
        W.free(); dx.free(); dy.free()
for name in ("tiny-llama_F16", "tiny-qwen2_F16"):  # whole models: the stock -ffp-contract=fast build of the reference, bit for bit
    e = np.load(os.path.join(G, f"e2e_f16_{name}.npz"))
    d = os.path.join(sys.argv[2], name)
    synth.write_model_dir(d, str(e["preset"]), int(e["wt"]), n_ctx=int(e["n_ctx"]), seed=int(e["seed"]), embd_type=int(e["embd_type"]))
    m = hip.Model(ctx, d, max_batch=16)
    p = e["prompt"]
    assert np.array_equal(m.generate(p, 8, 24), e["ids_fast"]), name
    m.reset()
    for lo in range(0, 20, 8):
        m.forward(p[lo:min(lo + 8, 20)], np.arange(lo, min(lo + 8, 20)), lm_head=False)
    cur = int(p[-1])
    for s in range(24):
        lg, _ = m.forward([cur], [m.position], lm_head=True)
        assert np.array_equal(lg[0].view(np.uint32), e["logits_fast"][s].view(np.uint32)), (name, s)
        cur = int(e["ids_fast"][s])
    m.reset()
    lg, _ = m.forward(p[:9], np.arange(9), lm_head=True)
    assert np.array_equal(lg.view(np.uint32), e["batch_logits_fast"].view(np.uint32)), name
    m.close()
ctx.close()
print("contract f16 ok")
"""


def test_contract_build_same_bits(tmp_path):
    """lib/libps_hip_contract.so: the F16 mul_mat needs no contraction case (products of fp16 values are exact in fp32) -- the reference's
    -ffp-contract=off vectors bit for bit, K = 99 and 100 included -- and whole F16 models reproduce the stock build of the reference
    (tests/golden/e2e_f16_*.npz, *_fast) bit for bit"""
    from powerserve_amd import hip
    lib = os.path.join(os.path.dirname(hip.LIB_PATH), "libps_hip_contract.so")
    assert os.path.exists(lib)
    r = subprocess.run([sys.executable, "-c", _CONTRACT, ROOT, str(tmp_path)], env=dict(os.environ, PS_HIP_LIB=lib), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "contract f16 ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("name", ["tiny-llama_F16", "tiny-qwen2_F16"])
def test_host_graph_and_lowered_paths(tmp_path, name):
    """The host façade (libps_host: json_gguf loader, Graph -> Executor, HIPBackend::plan / match_canonical) on an F16 model: every graph is
    lowered to the fused forward (ps_hip_model_forward_lowered, ps_hip_model_prefill), and with lowering off the op-by-op path (HIPBackend's
    mat-muls through ps_hip_mul_mat on the F16 weights) gives the same ids and bits -- both the reference's"""
    from powerserve_amd import host, synth
    g = np.load(os.path.join(GOLD, f"e2e_f16_{name}.npz"))
    d = str(tmp_path / "m")
    synth.write_model_dir(d, str(g["preset"]), int(g["wt"]), n_ctx=int(g["n_ctx"]), seed=int(g["seed"]), embd_type=int(g["embd_type"]))
    hm = host.HostModel(d, 0, max_batch=16)
    prompt = g["prompt"]
    for fused in (True, False):
        hm.set_fused(fused)
        hm.reset()
        p0 = hm.plan_stats()
        assert np.array_equal(hm.generate(prompt, 8, 24), g["ids"]), fused
        n_plans, n_low = hm.plan_stats()
        if fused:
            assert n_plans > p0[0] and n_low - p0[1] == n_plans - p0[0]  # every graph recognised and lowered
        else:
            assert n_low == p0[1]
        hm.reset()
        lg = hm.forward(prompt[:9], np.arange(9), True)
        assert np.array_equal(lg.view(np.uint32), g["batch_logits"].view(np.uint32)), fused
        hm.reset()
        hm.prefill(prompt[:-1], 8)
        cur, ids = int(prompt[-1]), []
        for s in range(24):  # Model::decode: the lowered single-token forward (fused) / the op graph
            cur = int(hm.decode([cur], [20 + s])[0])
            ids.append(cur)
        assert np.array_equal(ids, g["ids"]), fused
    hm.close()
