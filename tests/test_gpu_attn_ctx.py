"""Single-token attention at context windows that are NOT multiples of 32, on every path, with the path each forward took asserted through
ps_hip_last_attention_kernel.

The V cache is [kv_dim][n_ctx]: row r of a kv head starts r * n_ctx * 4 bytes into the layer's cache, so with n_ctx % 32 != 0 its 128-byte lines are
shifted against its columns.  The fused Q / K / V + attention launch (k_qkvattn.hip) pulls V lines before its rendezvous that must be lines nobody
writes in that launch; that holds only with n_ctx % 32 == 0, and psk_qkv_attn declines every other window.  The prompts here are short -- the hazard
needs a new position past the first line (pos0 >= 32) and a row r >= 1, not a long cache -- and the decode walks the new position across the
32-column boundaries at 32 and 64 in every row phase (r * n_ctx) % 32 of a workgroup's four rows.  n_ctx only sets the row stride: the oracle's
results do not depend on it, so each preset's oracle run serves every window."""
import os

import numpy as np
import pytest

from attn_reference import attention_reference
from conftest import load_tensors

pytestmark = pytest.mark.gpu

WINDOWS = [1000, 1028, 2100, 4092, 1024, 4096]  # = 8, 4, 20, 28 (mod 32); the last two are the controls
P, STEPS = 30, 44  # decode positions 29 .. 72: across the lines at 32 and 64
HIDDEN = [31, 32, 63, 64]  # slots on both sides of two 32-column boundaries


def last_attention(ctx):
    return ctx.L.ps_hip_last_attention_kernel().decode()


def expected_path(mode, hs, r2, fused_ok):
    """the single-token attention a forward in `mode` takes (model.hip, enqueue_forward)"""
    nv = hs // 32
    if mode & 16:
        return f"attn_scores_kernel<{nv}> + attn_softmax_pv_kernel"
    if fused_ok and not mode & 128:
        return f"qkv_attn_kernel<{nv}, "
    if r2 <= 4:
        return f"attn_decode2_kernel<{nv}, "
    return f"attn_scores_kernel<{nv}> + attn_softmax_pv_kernel"  # (attn_decode2 declines more than 4 query heads per kv head)


def bits(x):
    return np.asarray(x).view(np.uint32)


def oracle_run(oracle, tmp_path, preset, wt, seed):
    from oracle import binding as B
    from powerserve_amd import synth
    d = str(tmp_path / "m")
    mj = synth.write_model_dir(d, preset, wt, n_ctx=4096, seed=seed)
    cfg = B.make_config(mj["llm_config"])
    om = oracle.model(cfg, mj["model_arch"], load_tensors(os.path.join(d, "ggml/weights.gguf")), n_threads=min(32, os.cpu_count() or 8))
    prompt = np.random.default_rng(seed).integers(0, cfg.vocab_size, P)
    want_ids, want_logits, *_ = om.generate(prompt, 32, STEPS, want_logits=True)
    om.close()
    return d, cfg, prompt, want_ids, want_logits


def decode_steps(ctx, gm, prompt, want_ids, want_logits, want_path, tag):
    """prefill as the oracle did (one chunk), then every step teacher-forced: logits on bits, and the path taken"""
    gm.reset()
    gm.forward(prompt[:-1], np.arange(P - 1), lm_head=False)
    cur = int(prompt[-1])
    for s in range(STEPS):
        lg, am = gm.forward([cur], [gm.position], lm_head=True)
        assert np.array_equal(bits(lg[0]), bits(want_logits[s])), (tag, s)
        assert last_attention(ctx).startswith(want_path), (tag, s, last_attention(ctx))
        cur = int(want_ids[s])


@pytest.mark.parametrize("preset,force", [("llama-8b-dims-4l", 0), ("small-llama-hs128", 1), ("llama-1b-dims-2l", 1)])
def test_fused_launch_runs_only_on_line_aligned_windows(ctx, oracle, tmp_path, preset, force):
    """llama-8b-dims-4l takes the fused launch by default; the two smaller shapes only with ps_hip_debug_set(7, 1).  At every window: greedy ids through
    the captured step, per-step logits eager and through the captured single-token forward, and the same bits from the two launches (mode bit 7) and
    from scores + soft-max.V.p (mode bit 4), all against the oracle -- the fused kernel having run at the controls and at no other window.  Then
    hidden slots on both sides of a line boundary: the three plans agree bit for bit."""
    from powerserve_amd import hip
    d, cfg, prompt, want_ids, want_logits = oracle_run(oracle, tmp_path, preset, 12, 21)
    hs, r2 = cfg.head_size, cfg.n_heads // cfg.n_kv_heads
    assert ctx.L.ps_hip_debug_set(7, force) == 0
    try:
        for n_ctx in WINDOWS:
            aligned = n_ctx % 32 == 0
            gm = hip.Model(ctx, d, max_batch=32, n_ctx=n_ctx)
            try:
                assert np.array_equal(gm.generate(prompt, 32, STEPS), want_ids), n_ctx          # hipGraph replay
                assert last_attention(ctx).startswith(expected_path(0, hs, r2, aligned)), (n_ctx, last_attention(ctx))  # (what the capture enqueued)
                for mode in (1, 0, 129, 17):  # eager / the captured single-token forward; the two launches; scores + soft-max.V.p
                    gm.set_mode(mode)
                    decode_steps(ctx, gm, prompt, want_ids, want_logits, expected_path(mode, hs, r2, aligned), (n_ctx, mode))
                outs = []
                for mode in (1, 129, 17):
                    gm.set_mode(mode)
                    gm.kv_rollback(6)
                    for h in HIDDEN:
                        gm.kv_mask(h, False)
                    res = []
                    for s in range(6):
                        lg, _ = gm.forward([int(want_ids[STEPS - 7 + s])], [gm.position], lm_head=True)  # (teacher forcing: step k is fed id k - 1)
                        assert last_attention(ctx).startswith(expected_path(mode, hs, r2, aligned)), (n_ctx, mode, last_attention(ctx))
                        res.append(np.asarray(lg[0]).copy())
                    for h in HIDDEN:
                        gm.kv_mask(h, True)
                    outs.append(np.stack(res))
                assert np.array_equal(bits(outs[0]), bits(outs[1])) and np.array_equal(bits(outs[0]), bits(outs[2])), n_ctx
                assert not np.array_equal(outs[0][0], np.asarray(want_logits[STEPS - 6]))  # (unmasked, these would be that step's logits)
            finally:
                gm.close()
    finally:
        ctx.L.ps_hip_debug_set(7, 0)


def test_fused_launch_path_at_the_bench_window(ctx, tmp_path):
    """The observable at the benchmark's shape: llama-8b-dims-4l in Q4_K names the fused launch at n_ctx 4096 and the one-launch attention behind the
    separate Q / K / V mat-vec at 4092 -- eager and captured (no oracle: the bits are the test above's)."""
    from powerserve_amd import hip, synth
    d = str(tmp_path / "m")
    synth.write_model_dir(d, "llama-8b-dims-4l", 12, n_ctx=4096, seed=3)
    for n_ctx, want in ((4096, "qkv_attn_kernel<4, "), (4092, "attn_decode2_kernel<4, ")):
        gm = hip.Model(ctx, d, max_batch=8, n_ctx=n_ctx)
        try:
            prompt = np.arange(1, 40)
            gm.generate(prompt, 8, 3)
            assert last_attention(ctx).startswith(want), (n_ctx, last_attention(ctx))
            gm.set_mode(1)
            gm.forward([5], [gm.position], lm_head=True)
            assert last_attention(ctx).startswith(want), (n_ctx, last_attention(ctx))
        finally:
            gm.close()


@pytest.mark.parametrize("preset,wt", [("odd-llama-r1", 12), ("odd-qwen2-r3", 8), ("odd-llama-r5", 8), ("odd-llama-r6", 12), ("odd-llama-r8", 12)])
def test_single_token_paths_at_unaligned_windows(ctx, oracle, tmp_path, preset, wt):
    """attn_decode2 (mode bit 7: the two launches; it declines more than 4 query heads per kv head, which then take the pair) and scores + soft-max.V.p
    (mode bit 4) at the same windows, 1, 3, 5, 6 and 8 query heads per kv head: greedy ids through the captured step and per-step logits eager, on bits
    against the oracle, and the path each took.  8 query heads per kv head keep 8 LDS-resident soft-max rows of n_ctx floats: 4092 is refused."""
    from powerserve_amd import hip
    d, cfg, prompt, want_ids, want_logits = oracle_run(oracle, tmp_path, preset, wt, 23)
    hs, r2 = cfg.head_size, cfg.n_heads // cfg.n_kv_heads
    windows = [1000, 2100] if r2 == 8 else WINDOWS
    if r2 == 8:
        with pytest.raises(hip.PSHipError, match="n_ctx too large"):
            hip.Model(ctx, d, max_batch=32, n_ctx=4092)
    for n_ctx in windows:
        gm = hip.Model(ctx, d, max_batch=32, n_ctx=n_ctx)
        try:
            for mode in (128, 16):
                gm.set_mode(mode)
                assert np.array_equal(gm.generate(prompt, 32, STEPS), want_ids), (n_ctx, mode)
                assert last_attention(ctx).startswith(expected_path(mode, hs, r2, False)), (n_ctx, mode, last_attention(ctx))
                gm.set_mode(mode | 1)
                decode_steps(ctx, gm, prompt, want_ids, want_logits, expected_path(mode, hs, r2, False), (n_ctx, mode))
        finally:
            gm.close()


# (preset, wt, n_ctx, prompt length, hidden slots): windows off multiples of 32; 1 and 8 query heads per kv head; from an empty cache (n_kv < 32
# splits: empty splits the merge must skip); hidden slots 40 .. 47 that empty splits 10 and 11 whole (n_kv 97 .. 128: 4 positions per split)
F16_CASES = [("small-llama-hs128", 12, 1028, 150, ()), ("small-llama-hs128", 12, 2100, 1100, ()), ("llama-1b-dims-2l", 12, 1000, 70, ()),
             ("odd-llama-r1", 12, 1028, 90, ()), ("odd-llama-r8", 12, 2100, 120, ()), ("odd-llama-r8", 12, 1000, 1, ()),
             ("small-llama-hs128", 12, 4092, 1, ()), ("small-llama-hs128", 12, 1028, 97, tuple(range(40, 48)))]


@pytest.mark.parametrize("preset,wt,n_ctx,n_prompt,hidden", F16_CASES)
def test_fp16_kv_decode_mode_edges(ctx, tmp_path, preset, wt, n_ctx, n_prompt, hidden):
    """The fp16-KV decode mode (bit 3, attn_flash16_kernel: not bit-exact) at the edges test_gpu_model.py's parity test leaves out: the attention output
    of the last layer against the float64 soft-max over the model's own q and FP32 caches (hidden slots excluded) within 2e-3 of its largest value at
    every step, and more than 1e-6 off somewhere (really the other path) -- where the parity path, same inputs, is within 1e-6."""
    from powerserve_amd import hip, synth
    d = str(tmp_path / "m")
    synth.write_model_dir(d, preset, wt, n_ctx=n_ctx, seed=6)
    m = hip.Model(ctx, d, max_batch=64)
    try:
        hs, r2 = m.cfg.head_size, m.cfg.n_heads // m.cfg.n_kv_heads
        prompt = np.random.default_rng(2).integers(0, m.cfg.vocab_size, n_prompt)
        steps = 40 if n_prompt == 1 else 24

        def run(mode):
            m.reset()
            assert ctx.L.ps_hip_model_set_mode(m.h, mode) == 0
            for lo in range(0, n_prompt - 1, 64):
                hi = min(lo + 64, n_prompt - 1)
                m.forward(prompt[lo:hi], np.arange(lo, hi), lm_head=False)
            for h in hidden:
                m.kv_mask(h, False)
            cur, errs = int(prompt[-1]), []
            for s in range(steps):
                _, am = m.forward([cur], [m.position], lm_head=True)
                ref = attention_reference(m, m.position, hidden)
                errs.append(float(np.abs(m.scratch(2, 1)[0] - ref).max() / np.abs(ref).max()))
                want_path = f"attn_flash16_kernel<{hs}>" if mode & 8 else expected_path(0, hs, r2, False)
                assert last_attention(ctx).startswith(want_path), (mode, s, last_attention(ctx))
                cur = int(am[0])
            return errs

        parity = run(0)
        assert max(parity) < 1e-6, parity
        fp16 = run(8)
        assert max(fp16) < 2e-3, fp16
        assert max(fp16) > 1e-6, fp16  # (close, and really a different path)
    finally:
        m.close()


@pytest.mark.parametrize("preset,wt", [("odd-qwen2-r3", 8), ("odd-llama-r5", 8), ("odd-llama-r6", 12)])
def test_fp16_kv_decode_mode_declines_other_ratios(ctx, tmp_path, preset, wt):
    """attn_flash16_kernel takes 1, 2, 4 or 8 query heads per kv head; at 3, 5 and 6 the fp16-KV mode's single-token forward falls back to the parity
    kernels (attn_decode2 up to 4 query heads per kv head, scores + soft-max.V.p above) -- and is then bit-identical to the mode without bit 3."""
    from powerserve_amd import hip, synth
    d = str(tmp_path / "m")
    synth.write_model_dir(d, preset, wt, n_ctx=1028, seed=6)
    m = hip.Model(ctx, d, max_batch=64)
    try:
        r2, hs = m.cfg.n_heads // m.cfg.n_kv_heads, m.cfg.head_size
        want_path = expected_path(0, hs, r2, False)
        prompt = np.random.default_rng(2).integers(0, m.cfg.vocab_size, 50)
        outs = []
        for mode in (0, 8):
            m.reset()
            assert ctx.L.ps_hip_model_set_mode(m.h, mode) == 0
            m.forward(prompt[:-1], np.arange(prompt.size - 1), lm_head=False)
            cur, res = int(prompt[-1]), []
            for s in range(12):
                lg, am = m.forward([cur], [m.position], lm_head=True)
                assert last_attention(ctx).startswith(want_path), (mode, s, last_attention(ctx))
                res.append(np.asarray(lg[0]).copy())
                cur = int(am[0])
            outs.append(np.stack(res))
        assert np.array_equal(bits(outs[0]), bits(outs[1]))
    finally:
        m.close()
