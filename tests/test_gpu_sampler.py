"""The standard sampler chain on the device (include/ps_hip.h ps_hip_sample / ps_hip_model_decode_sampled, csrc/k_sample.hip):
token for token and engine word for engine word what the host SamplerChain (csrc/host/sampler.cpp) and the reference's own
sampler classes (oracle/_ref) draw from the same logits."""
import ctypes as C
import os

import numpy as np
import pytest

from test_sampler_vs_ref import CASES

pytestmark = pytest.mark.gpu


def load_tensors(path):
    from powerserve_amd import gguf
    rd = gguf.GGUFReader(path)
    return {n: (ti.type, np.array(rd.data(n)), ti.ne[0], (list(ti.ne) + [1])[1]) for n, ti in rd.tensors.items()}


def _has_tie(v, k):
    if np.isnan(v).any():
        return True
    top = np.sort(v)[::-1][:k + 1]
    return bool((top[:-1] == top[1:]).any())


def _adversarial(n, k, rng):
    base = rng.standard_normal(n).astype(np.float32)
    out = [np.full(n, 0.25, np.float32), rng.choice(np.array([-1.0, 0.0, 2.0], np.float32), n),
           np.arange(n, dtype=np.float32) / n, (np.arange(n)[::-1] / n).astype(np.float32),
           ((np.arange(n) // 2) / n).astype(np.float32)]
    nan = base.copy(); nan[rng.integers(0, n, 7)] = np.nan; out.append(nan)
    inf = base.copy(); inf[rng.integers(0, n, 3)] = np.inf; inf[rng.integers(0, n, 3)] = -np.inf; out.append(inf)
    z = base.copy(); z[np.argsort(z)[-(k + 1):]] = 0.0; z[np.argsort(base)[-1]] = -0.0; out.append(z)
    return out


OP_CONFIGS = [(512, kw) for kw in CASES if kw.get("top_k", 40) < 512] + [
    (128256, dict()), (128256, CASES[4]), (128256, dict(top_k=256, top_p=1.0, temperature=1.0)), (151936, dict()), (151936, CASES[5])]


@pytest.mark.parametrize("n_vocab,kw", OP_CONFIGS)
def test_op_matches_host_and_reference(ctx, ref, n_vocab, kw):
    from oracle import binding as B
    from powerserve_amd import hip, host
    steps = 300
    cfg = host.SamplerCfg.make(n_vocab, **kw)
    chain = host.Sampler(cfg)
    dc, st = chain.device_state()
    rh = ref.L.ref_sampler_create(C.byref(B.SamplerCfg.from_buffer_copy(bytes(cfg))))
    k = int(cfg.top_k)
    active = cfg.penalty_last_n != 0 and not (cfg.penalty_repeat == 1.0 and cfg.penalty_freq == 0.0 and cfg.penalty_present == 0.0)
    rng = np.random.default_rng(n_vocab + k)
    adv = _adversarial(n_vocab, k, rng)
    dev = ctx.malloc(n_vocab * 4)
    try:
        n_tie_steps = 0
        for s in range(steps):
            lg = (rng.standard_normal(n_vocab) * 2.5).astype(np.float32)
            if s % 7 == 0:
                lg[rng.integers(0, n_vocab, 3)] = lg.max()  # ties at the top
            elif s % 11 == 0:
                lg[rng.integers(0, n_vocab, 4)] = np.sort(lg)[-k]  # ties straddling place k
            elif s % 13 == 0:
                lg = adv[(s // 13) % len(adv)].copy()
            ctx.check(ctx.L.ps_hip_memcpy_h2d(ctx.h, dev, lg.ctypes.data, lg.nbytes))
            e0 = st.n_exact
            got = hip.sample(ctx, dev, n_vocab, dc, st)
            want = chain.sample(lg)
            assert got == want, (s, got, want)
            assert ref.L.ref_sampler_sample(rh, lg.ctypes.data, n_vocab) == want, s
            if not active and not cfg.ignore_eos:  # the list top-k sees is the raw row: its ties decide the path
                tie = _has_tie(lg, k)
                assert (st.n_exact - e0) == int(tie), (s, tie)
                n_tie_steps += tie
        words, pos = chain.engine_state()
        assert np.array_equal(np.array(st.mt[:], np.uint32), words) and st.mt_pos == pos
        if not active and not cfg.ignore_eos:
            assert n_tie_steps > 0
        assert "sample_final_kernel" in hip.last_sample_kernels()
    finally:
        ctx.free(dev)
        ref.L.ref_sampler_free(rh)
        chain.close()


def test_op_refuses_uncovered(ctx):
    from powerserve_amd import hip, host
    dev = ctx.malloc(512 * 4)
    try:
        for kw in (dict(top_k=hip.SAMPLE_K_MAX + 1), dict(top_k=512)):
            dc, st = host.Sampler(host.SamplerCfg.make(512, **kw)).device_state()
            with pytest.raises(hip.PSHipError):
                hip.sample(ctx, dev, 512, dc, st)
    finally:
        ctx.free(dev)


MODEL_PRESETS = [("small-llama-hs128", 12), ("llama-1b-dims-2l", 2), ("qwen2-0.5b-dims-2l", 8)]


@pytest.mark.parametrize("preset,wt", MODEL_PRESETS)
@pytest.mark.parametrize("kw", [CASES[0], CASES[5]])
def test_generate_device_equals_host_loop_equals_reference(oracle, ref, tmp_path, preset, wt, kw):
    """Model::generate with a standard chain takes the device sampler; == the forced host loop == oracle logits through the
    reference's own sampler classes; the chain's engine afterwards is the same either way."""
    from oracle import binding as B
    from powerserve_amd import hip, host, synth
    d = str(tmp_path / "m")
    mj = synth.write_model_dir(d, preset, wt, n_ctx=96, seed=5)
    cfg = B.make_config(mj["llm_config"])
    hm = host.HostModel(d, 0, max_batch=16)
    prompt = np.random.default_rng(2).integers(0, cfg.vocab_size, 11)
    steps = 40
    scfg = host.SamplerCfg.make(cfg.vocab_size, **kw)
    c0 = hip.sample_counters()
    s_dev = host.Sampler(scfg)
    got = host.generate_with(hm, prompt, 8, steps, s_dev)
    assert hip.sample_counters()[1] > c0[1]  # the device drew
    hm.set_device_sampling(False)
    s_host = host.Sampler(scfg)
    c1 = hip.sample_counters()
    loop = host.generate_with(hm, prompt, 8, steps, s_host)
    assert hip.sample_counters() == c1  # the host loop did not touch the device sampler
    hm.set_device_sampling(True)
    assert np.array_equal(got, loop)
    w1, p1 = s_dev.engine_state(); w2, p2 = s_host.engine_state()
    assert np.array_equal(w1, w2) and p1 == p2
    # the chains carry on identically (penalty history included)
    lg = np.random.default_rng(4).standard_normal(cfg.vocab_size).astype(np.float32)
    assert s_dev.sample(lg) == s_host.sample(lg)
    s_dev.close(); s_host.close()
    om = oracle.model(cfg, mj["model_arch"], load_tensors(os.path.join(d, "ggml/weights.gguf")), n_threads=8)
    rh = ref.L.ref_sampler_create(C.byref(B.SamplerCfg.from_buffer_copy(bytes(scfg))))
    om.forward(prompt[:8], np.arange(8), False)
    om.forward(prompt[8:10], np.arange(8, 10), False)
    cur, want = int(prompt[-1]), []
    for _ in range(steps):
        lg = om.forward([cur], [om.position], True)
        cur = ref.L.ref_sampler_sample(rh, lg.ctypes.data, cfg.vocab_size)
        want.append(cur)
    ref.L.ref_sampler_free(rh)
    assert list(got) == want
    hm.close(); om.close()


def _host_loop(m, token, steps, chain):
    """single-token forwards with the logits on the host, the chain on the host"""
    out, cur = [], int(token)
    for _ in range(steps):
        lg, _ = m.forward([cur], [m.position])
        cur = chain.sample(lg[0])
        out.append(cur)
    return np.array(out, np.int32)


@pytest.fixture(scope="module")
def small_model(tmp_path_factory):
    from powerserve_amd import synth
    d = str(tmp_path_factory.mktemp("sm") / "m")
    synth.write_model_dir(d, "small-llama-hs128", 12, n_ctx=160, seed=7)
    return d


def _prefilled(ctx, d, mode=0, n_prompt=9):
    from powerserve_amd import hip
    m = hip.Model(ctx, d, max_batch=16)
    if mode:
        m.set_mode(mode)
    prompt = np.random.default_rng(1).integers(0, m.cfg.vocab_size, n_prompt)
    m.forward(prompt[:-1], np.arange(n_prompt - 1), lm_head=False)
    return m, int(prompt[-1])


@pytest.mark.parametrize("mode", [0, 1, 16, 8])
def test_decode_sampled_equals_host_loop_in_every_mode(ctx, small_model, mode):
    """captured (0), eager (1), two-launch attention (16), fp16-KV (8): decode_sampled == the host loop in the same mode"""
    from powerserve_amd import host
    kw = dict(CASES[4])
    m, tok = _prefilled(ctx, small_model, mode)
    chain = host.Sampler(host.SamplerCfg.make(m.cfg.vocab_size, **kw))
    dc, st = chain.device_state()
    got = m.decode_sampled(tok, 48, dc, st)
    m.close()
    m, tok = _prefilled(ctx, small_model, mode)
    want = _host_loop(m, tok, 48, chain)
    m.close()
    assert np.array_equal(got, want)
    words, pos = chain.engine_state()
    assert np.array_equal(np.array(st.mt[:], np.uint32), words) and st.mt_pos == pos
    chain.close()


def test_decode_sampled_split_runs_and_recapture(ctx, small_model):
    """one run of N steps == two runs of N/2 (state carried); a second pass from an earlier position re-captures the step
    (its position hint) and draws what an eager run draws"""
    from powerserve_amd import hip, host
    cfg = host.SamplerCfg.make(1024, seed=3)
    m, tok = _prefilled(ctx, small_model)
    p0 = m.position
    dc, st = host.Sampler(cfg).device_state()
    one = m.decode_sampled(tok, 40, dc, st)
    m.ctx.check(m.ctx.L.ps_hip_model_kv_truncate(m.h, p0))
    dc2, st2 = host.Sampler(cfg).device_state()
    a = m.decode_sampled(tok, 20, dc2, st2)
    b = m.decode_sampled(int(a[-1]), 20, dc2, st2)
    assert np.array_equal(one, np.concatenate([a, b]))
    assert np.array_equal(np.array(st.mt[:]), np.array(st2.mt[:])) and st.mt_pos == st2.mt_pos and st.n_outputs == st2.n_outputs
    m.close()
    m, tok = _prefilled(ctx, small_model, 1)
    dc3, st3 = host.Sampler(cfg).device_state()
    assert np.array_equal(m.decode_sampled(tok, 40, dc3, st3), one)
    m.close()
    assert isinstance(st3, hip.SampleState)


def test_decode_sampled_retries_after_attention_timeout(ctx, small_model):
    from powerserve_amd import host
    cfg = host.SamplerCfg.make(1024, seed=8)
    m, tok = _prefilled(ctx, small_model)
    dc, st = host.Sampler(cfg).device_state()
    want = m.decode_sampled(tok, 24, dc, st)
    m.close()
    m, tok = _prefilled(ctx, small_model)
    dc2, st2 = host.Sampler(cfg).device_state()
    try:
        ctx.L.ps_hip_debug_set(5, 1)
        got = m.decode_sampled(tok, 24, dc2, st2)
    finally:
        ctx.L.ps_hip_debug_set(5, 0)
    assert np.array_equal(got, want)
    assert np.array_equal(np.array(st.mt[:]), np.array(st2.mt[:])) and st.mt_pos == st2.mt_pos and st.n_outputs == st2.n_outputs
    m.close()


def test_decode_sampled_refuses_hidden_slots_and_uncovered(ctx, small_model):
    from powerserve_amd import hip, host
    m, tok = _prefilled(ctx, small_model)
    for kw in (dict(top_k=hip.SAMPLE_K_MAX + 1), dict(top_k=1024)):
        dc, st = host.Sampler(host.SamplerCfg.make(1024, **kw)).device_state()
        with pytest.raises(hip.PSHipError):
            m.decode_sampled(tok, 4, dc, st)
    dc, st = host.Sampler(host.SamplerCfg.make(1024)).device_state()
    ctx.check(ctx.L.ps_hip_model_kv_mask(m.h, 2, 0))
    with pytest.raises(hip.PSHipError):
        m.decode_sampled(tok, 4, dc, st)
    m.close()


def test_generate_serves_uncovered_chains_with_the_host_loop(tmp_path):
    """k > K_MAX, k >= vocab and a chain with a plug-in stage: Model::generate keeps the host loop (same tokens as the forced loop)"""
    from powerserve_amd import hip, host, synth
    d = str(tmp_path / "m")
    synth.write_model_dir(d, "small-llama-hs128", 12, n_ctx=96, seed=5)
    hm = host.HostModel(d, 0, max_batch=16)
    prompt = np.random.default_rng(2).integers(0, 1024, 11)
    for kw, noop in ((dict(top_k=300, top_p=1.0), False), (dict(top_k=1024), False), (dict(), True)):
        cfg = host.SamplerCfg.make(1024, **kw)
        sa, sb = host.Sampler(cfg), host.Sampler(cfg)
        if noop:
            sa.append_noop(); sb.append_noop()
        c0 = hip.sample_counters()
        got = host.generate_with(hm, prompt, 8, 16, sa)
        assert hip.sample_counters() == c0, kw
        hm.set_device_sampling(False)
        assert np.array_equal(got, host.generate_with(hm, prompt, 8, 16, sb)), kw
        hm.set_device_sampling(True)
        sa.close(); sb.close()
    hm.close()


def test_workspace_default_hparams_equal_the_host_loop(tmp_path):
    import json
    from powerserve_amd import host, synth
    wf = tmp_path / "work"
    synth.write_model_dir(str(wf / "main"), "small-llama-hs128", 12, n_ctx=128, seed=3)
    (wf / "hparams.json").write_text(json.dumps({"batch_size": 16, "sampler": {"seed": 5}}))
    (wf / "workspace.json").write_text(json.dumps({"hparams_config": "hparams.json", "model_main": "main"}))
    prompt = np.random.default_rng(0).integers(0, 1024, 19)
    ws = host.Workspace(str(wf))
    got = ws.generate(prompt, 24)
    ws.main.set_device_sampling(False)
    assert np.array_equal(ws.generate(prompt, 24), got)
    ws.close()
