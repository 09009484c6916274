"""Long-window models (ps_hip_model_create_long, hip.Model(..., long_window=True)): score and probability rows in device memory, attn_softmax_long_kernel
and attn_pv_long_kernel (csrc/k_attn_long.hip).  The kernels do not care how large the window is, so most of this runs at windows of a few hundred to a few
thousand slots, with the V.p tile (ps_hip_debug_set key 13) cut down to 64 positions so that a short cache walks several tiles, and the row-sum
certificate (key 14) both at its default and forced open (every row through the sequential sum).  One test goes to the far end of a 131 072-slot window
on an uploaded cache.  Every comparison is on bits."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_tensors

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Q4_0, Q8_0, Q4_K = 2, 8, 12
STEPS = 40
PROMPTS = {23: 5, 340: 32}  # prompt length: prefill chunk.  23 in chunks of 5, 5, 5, 5, 2 (attn_pv_long_kernel on 5 and 2 columns); 340 in chunks of 32 (the matrix-core V.p), and with the tile at 64 positions its decode walks five tiles plus leftovers
GEOMETRIES = [("odd-llama-r1", Q4_K), ("tiny-llama", Q4_K), ("odd-qwen2-r3", Q8_0), ("odd-llama-r5", Q8_0), ("odd-llama-r8", Q4_K),
              ("odd-llama-hs96", Q4_K), ("odd-llama-hs32", Q4_K)]


def bits(x):
    return np.asarray(x).view(np.uint32)


def last_attention(ctx):
    return ctx.L.ps_hip_last_attention_kernel().decode()


def single_token_path(cfg):
    return f"attn_scores_kernel<{cfg.head_size // 32}> + attn_softmax_long_kernel + attn_pv_long_kernel<"


class debug_keys:
    """ps_hip_debug_set keys 13 (V.p tile) and 14 (eps shift), restored on the way out"""

    def __init__(self, ctx, tile=0, shift=0):
        self.ctx, self.tile, self.shift = ctx, tile, shift

    def __enter__(self):
        from powerserve_amd import hip
        try:
            assert self.ctx.L.ps_hip_debug_set(hip.DEBUG_LONG_PV_TILE, self.tile) == 0
            assert self.ctx.L.ps_hip_debug_set(hip.DEBUG_LONG_EPS_SHIFT, self.shift) == 0
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        from powerserve_amd import hip
        self.ctx.L.ps_hip_debug_set(hip.DEBUG_LONG_PV_TILE, 0)
        self.ctx.L.ps_hip_debug_set(hip.DEBUG_LONG_EPS_SHIFT, 0)
        return False


_ORACLE_RUNS = {}


@pytest.fixture(scope="module")
def model_root(tmp_path_factory):
    return tmp_path_factory.mktemp("long_ctx")


def oracle_run(oracle, root, preset, wt):
    """the preset's model directory, its configuration, and per prompt length (prompt, greedy ids, per-step logits) from the oracle.  The window only sets
    row strides: the oracle's results do not depend on it, so one run serves every window"""
    if preset in _ORACLE_RUNS:
        return _ORACLE_RUNS[preset]
    from oracle import binding as B
    from powerserve_amd import synth
    d = str(root / preset)
    mj = synth.write_model_dir(d, preset, wt, n_ctx=4096, seed=31)
    cfg = B.make_config(mj["llm_config"])
    om = oracle.model(cfg, mj["model_arch"], load_tensors(os.path.join(d, "ggml/weights.gguf")), n_threads=min(16, os.cpu_count() or 8))
    runs = {}
    for P, chunk in PROMPTS.items():
        prompt = np.random.default_rng(P).integers(0, cfg.vocab_size, P)
        ids, logits, *_ = om.generate(prompt, chunk, STEPS, want_logits=True)
        runs[P] = (prompt, ids, logits, chunk)
    om.close()
    _ORACLE_RUNS[preset] = (d, cfg, runs)
    return _ORACLE_RUNS[preset]


def check_against_oracle(ctx, gm, cfg, run, tag):
    """greedy ids through the captured step, then every step's logits eagerly (teacher-forced), and the kernels each took"""
    prompt, want_ids, want_logits, chunk = run
    gm.set_mode(16)  # (a mode change drops the captured steps -- bit 4 itself changes nothing here: the next capture reads the debug keys as they are now)
    gm.set_mode(0)
    assert np.array_equal(gm.generate(prompt, chunk, STEPS), want_ids), tag
    assert last_attention(ctx).startswith(single_token_path(cfg)), (tag, last_attention(ctx))
    gm.set_mode(1)
    gm.reset()
    for lo in range(0, prompt.size - 1, chunk):
        hi = min(lo + chunk, prompt.size - 1)
        gm.forward(prompt[lo:hi], np.arange(lo, hi), lm_head=False)
    cur = int(prompt[-1])
    for s in range(STEPS):
        lg, _ = gm.forward([cur], [gm.position], lm_head=True)
        assert np.array_equal(bits(lg[0]), bits(want_logits[s])), (tag, s)
        assert last_attention(ctx).startswith(single_token_path(cfg)), (tag, s, last_attention(ctx))
        cur = int(want_ids[s])


@pytest.mark.parametrize("preset,wt", GEOMETRIES)
def test_small_windows_every_geometry(ctx, oracle, model_root, preset, wt):
    """head sizes 128 / 64 / 96 / 32, 1, 2, 3, 5 and 8 query heads per kv head, NEOX RoPE with bias: windows 1000 and 2100 (not multiples of 32), captured and
    eager, the V.p tile at 64 positions and at its default, the certificate forced open and at its default."""
    from powerserve_amd import hip
    d, cfg, runs = oracle_run(oracle, model_root, preset, wt)
    for n_ctx in (1000, 2100):
        gm = hip.Model(ctx, d, max_batch=32, n_ctx=n_ctx, long_window=True)
        try:
            assert gm.is_long
            for tile, shift in ((64, 100), (64, 0), (0, 100), (0, 0)):
                with debug_keys(ctx, tile, shift):
                    hip.softmax_long_counters(reset=True)
                    for P in PROMPTS:
                        check_against_oracle(ctx, gm, cfg, runs[P], (preset, n_ctx, tile, shift, P))
                    rows, seq = hip.softmax_long_counters()
                    assert rows > 0 and (seq == rows if shift == 100 else seq < rows), (rows, seq, shift)
        finally:
            gm.close()


def test_past_the_cap(ctx, oracle, model_root):
    """8 query heads per kv head at 4092 slots: the regular model still refuses, the long-window model runs and matches the oracle"""
    from powerserve_amd import hip
    d, cfg, runs = oracle_run(oracle, model_root, "odd-llama-r8", Q4_K)
    with pytest.raises(hip.PSHipError, match="n_ctx too large"):
        hip.Model(ctx, d, max_batch=32, n_ctx=4092)
    gm = hip.Model(ctx, d, max_batch=32, n_ctx=4092, long_window=True)
    try:
        for P in PROMPTS:
            check_against_oracle(ctx, gm, cfg, runs[P], ("r8@4092", P))
    finally:
        gm.close()


def _golden(preset, tn):
    return np.load(os.path.join(GOLD, f"long_cache_{preset}_{tn}.npz"))


def _golden_dir(tmp_path, preset, tn, g):
    from powerserve_amd import synth
    d = str(tmp_path / f"{preset}_{tn}")
    synth.write_model_dir(d, preset, {"Q8_0": Q8_0, "Q4_0": Q4_0}[tn], n_ctx=int(g["n_ctx"]), seed=int(g["seed"]))
    return d


@pytest.mark.parametrize("preset,tn", [("tiny-llama", "Q8_0"), ("tiny-qwen2", "Q4_0")])
def test_depth_from_the_reference_fixtures(ctx, tmp_path, preset, tn):
    """tests/golden/long_cache_*.npz (the REAL reference: a 4 300-token prompt in chunks of 128 behind 4 608 slots, then 6 steps) through a long-window
    model: prefill chunks on the matrix-core V.p behind the long soft-max, single tokens through three tiles.  Ids and every step's logits."""
    from powerserve_amd import hip
    g = _golden(preset, tn)
    m = hip.Model(ctx, _golden_dir(tmp_path, preset, tn, g), max_batch=256, long_window=True)
    try:
        prompt, bs, steps = g["prompt"], int(g["batch"]), len(g["ids"])
        assert np.array_equal(m.generate(prompt, bs, steps), g["ids"])
        m.reset()
        m.prefill(prompt[:-1], bs)
        cur = int(prompt[-1])
        for s in range(steps):
            lg, _ = m.forward([cur], [m.position], lm_head=True)
            assert np.array_equal(bits(lg[0]), bits(g["logits"][s])), s
            cur = int(g["ids"][s])
    finally:
        m.close()


def test_equal_to_the_regular_model_at_depth(ctx, tmp_path):
    """the same fixture prompt in a regular and in a long-window model: a 5-column forward, a 6-node tree forward (non-causal tree, its own RoPE
    positions), a single token with four cached slots hidden, and 300 scored tokens at chunk 128 -- equal bits."""
    from powerserve_amd import hip
    g = _golden("tiny-llama", "Q8_0")
    d = _golden_dir(tmp_path, "tiny-llama", "Q8_0", g)
    prompt = g["prompt"]
    rng = np.random.default_rng(5)
    vocab = 512
    cols5 = rng.integers(0, vocab, 5)
    tree_tok = rng.integers(0, vocab, 6)
    tree = np.array([[1, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0], [1, 1, 0, 1, 0, 0], [1, 0, 1, 0, 1, 0], [1, 1, 0, 1, 0, 1]], dtype=np.uint8)
    score_tok = rng.integers(0, vocab, 300)
    score_tgt = rng.integers(0, vocab, 300)
    outs = []
    for long_window in (False, True):
        m = hip.Model(ctx, d, max_batch=256, long_window=long_window)
        try:
            m.prefill(prompt[:-1], 128)
            p0 = m.position
            res = {}
            res["cols5"], _ = m.forward(cols5, np.arange(p0, p0 + 5), lm_head=True)
            p1 = m.position
            res["tree"], _ = m.forward_tree(tree_tok, p1 + np.array([0, 1, 1, 2, 2, 3]), tree=tree, lm_head=True, want_logits=True)
            assert m.position == p1
            for slot in (3, 40, 2150, 4298):
                m.kv_mask(slot, False)
            res["hidden"], _ = m.forward([7], [m.position], lm_head=True)
            for slot in (3, 40, 2150, 4298):
                m.kv_mask(slot, True)
            res["score"] = m.score(score_tok, score_tgt, 128)
            assert m.position == p1 + 1 + 300
            outs.append(res)
        finally:
            m.close()
    a, b = outs
    for k in ("cols5", "tree", "hidden"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert a["score"].tobytes() == b["score"].tobytes()


def test_far_positions_on_an_uploaded_cache(ctx, oracle, tmp_path):
    """tiny-llama at a window of 131 072 slots.  Nobody prefills that far in a test: the same seeded random K / V rows go into the slots below P of the
    device model (ps_hip_memcpy_h2d to the cache pointers) and of the oracle (its writable cache views), both are advanced to P, and from there 8 greedy
    steps, a 5-column and a 24-column forward agree on bits.  P = 131 072 - 40 runs up to the last slot (one more step is refused, rc 2); P = 65 530
    crosses 2^16."""
    from oracle import binding as B
    from powerserve_amd import hip, synth
    N_CTX = hip.LONG_CTX_MAX
    d = str(tmp_path / "m")
    mj = synth.write_model_dir(d, "tiny-llama", Q4_K, n_ctx=N_CTX, seed=77)
    cfg = B.make_config(mj["llm_config"])
    om = oracle.model(cfg, mj["model_arch"], load_tensors(os.path.join(d, "ggml/weights.gguf")), n_threads=min(16, os.cpu_count() or 8))
    gm = hip.Model(ctx, d, max_batch=32, long_window=True)
    try:
        rng = np.random.default_rng(99)
        for L in range(cfg.n_layers):
            k = rng.standard_normal((N_CTX, cfg.kv_dim), dtype=np.float32)
            v = rng.standard_normal((cfg.kv_dim, N_CTX), dtype=np.float32)
            om.k_cache(L)[:] = k
            om.v_cache(L)[:] = v
            ctx.check(ctx.L.ps_hip_memcpy_h2d(ctx.h, ctx.L.ps_hip_model_k_cache(gm.h, L), k.ctypes.data_as(C.c_void_p), k.nbytes))
            ctx.check(ctx.L.ps_hip_memcpy_h2d(ctx.h, ctx.L.ps_hip_model_v_cache(gm.h, L), v.ctypes.data_as(C.c_void_p), v.nbytes))
        for P in (N_CTX - 40, 65530):  # (the deeper one first: what it writes lies behind the other's positions)
            om.reset()
            om.kv_advance(P)
            gm.reset()
            gm.kv_advance(P)
            tok = np.random.default_rng(P).integers(0, cfg.vocab_size, 1 + 5 + 24)
            ids = gm.decode_greedy(int(tok[0]), 8)
            cur, want = int(tok[0]), []
            for s in range(8):
                cur = int(np.argmax(om.forward([cur], [om.position], True)[0]))
                want.append(cur)
            assert np.array_equal(ids, want), (P, ids, want)
            assert last_attention(ctx).startswith(single_token_path(cfg))
            for lo, n in ((1, 5), (6, 24)):
                lg, _ = gm.forward(tok[lo:lo + n], np.arange(gm.position, gm.position + n), lm_head=True)
                ref = om.forward(tok[lo:lo + n], np.arange(om.position, om.position + n), True)
                assert np.array_equal(bits(lg), bits(ref)), (P, n)
            assert gm.position == om.position == P + 37
            if P == N_CTX - 40:
                cur = 3
                for s in range(3):  # up to the last slot
                    lg, am = gm.forward([cur], [gm.position], lm_head=True)
                    ref = om.forward([cur], [om.position], True)
                    assert np.array_equal(bits(lg), bits(ref)), s
                    cur = int(am[0])
                assert gm.position == N_CTX
                one, pos, am = np.array([cur], np.int32), np.array([N_CTX], np.int32), np.zeros(1, np.int32)
                assert ctx.L.ps_hip_model_forward(gm.h, one.ctypes.data_as(C.c_void_p), 1, pos.ctypes.data_as(C.c_void_p), None, 1, am.ctypes.data_as(C.c_void_p)) == 2
                assert ctx.L.ps_hip_model_decode_greedy(gm.h, cur, 1, am.ctypes.data_as(C.c_void_p)) == 2
                assert gm.position == N_CTX
    finally:
        gm.close()
        om.close()


def test_decode_recaptures_at_the_end_of_a_capture_window(ctx, tmp_path):
    """A captured step's score grid covers the 1 024 positions the capture is valid for.  A capture taken at position 0, then a prompt up to position 1 010,
    then decode_greedy of 40 steps: the replay loop must stop at position 1 024 and capture again (slots past the old grid would never be scored).
    Equal to 40 eager forwards."""
    from powerserve_amd import hip, synth
    d = str(tmp_path / "m")
    synth.write_model_dir(d, "tiny-llama", Q4_K, n_ctx=2100, seed=12)
    prompt = np.random.default_rng(8).integers(0, 512, 1010)
    runs = []
    for mode in (0, 1):
        m = hip.Model(ctx, d, max_batch=128, long_window=True)
        try:
            m.set_mode(mode)
            first = m.decode_greedy(int(prompt[0]), 2)  # (mode 0: the capture of positions 0 .. 1023)
            m.kv_rollback(2)
            m.prefill(prompt[:-1], 128)
            assert m.position == 1009
            m.forward([int(prompt[-1])], [1009], lm_head=False)
            if mode == 0:
                ids = m.decode_greedy(5, STEPS)
            else:
                ids, cur = [], 5
                for s in range(STEPS):
                    _, am = m.forward([cur], [m.position], lm_head=True)
                    cur = int(am[0])
                    ids.append(cur)
            assert m.position == 1010 + STEPS
            runs.append((first, np.asarray(ids)))
        finally:
            m.close()
    assert np.array_equal(runs[0][0], runs[1][0])
    assert np.array_equal(runs[0][1], runs[1][1]), runs


def test_refusals(ctx, tmp_path):
    """a second sequence, the batched step and the fp16-KV mode are refused (rc 2) with nothing changed; mode bits 4 and 7 are accepted and change nothing"""
    from powerserve_amd import hip, synth
    d = str(tmp_path / "m")
    synth.write_model_dir(d, "tiny-llama", Q4_K, n_ctx=1000, seed=4)
    m = hip.Model(ctx, d, max_batch=16, long_window=True)
    try:
        prompt = np.arange(3, 30)
        ids = m.generate(prompt, 16, 12)
        pos = m.position
        assert ctx.L.ps_hip_model_seq_reserve(m.h, 2) == 2 and b"long-window" in ctx.L.ps_hip_last_error(ctx.h)
        assert ctx.L.ps_hip_model_seq_reserve(m.h, 1) == 0
        assert ctx.L.ps_hip_model_set_mode(m.h, 8) == 2 and b"long-window" in ctx.L.ps_hip_last_error(ctx.h)
        seq, tok, am = np.zeros(1, np.int32), np.ones(1, np.int32), np.zeros(1, np.int32)
        assert ctx.L.ps_hip_model_decode_batch(m.h, seq.ctypes.data_as(C.c_void_p), tok.ctypes.data_as(C.c_void_p), 1, 1, am.ctypes.data_as(C.c_void_p)) == 2
        assert m.position == pos and m.seq_count == 1 and m.is_long
        for mode in (16, 128, 144, 0):
            assert ctx.L.ps_hip_model_set_mode(m.h, mode) == 0
            assert np.array_equal(m.generate(prompt, 16, 12), ids), mode
            assert last_attention(ctx).startswith(single_token_path(m.cfg)), (mode, last_attention(ctx))
    finally:
        m.close()


@pytest.mark.parametrize("n", [38401, 40000, 131072 + 5])
def test_op_api_rows_above_the_lds_cap(ctx, oracle, n):
    """ps_hip_softmax_ext / ps_hip_soft_max on rows above 150 KiB ([3 heads, 2 columns, n]): masks with -inf runs and a fully visible row, the certificate at
    its default and forced open, against the oracle."""
    from powerserve_amd import hip
    rng = np.random.default_rng(n)
    nh, bs = 3, 2
    s = (rng.standard_normal((nh, bs, n)) * 4).astype(np.float32)
    mask = np.zeros((bs, n), np.float32)  # row 0 fully visible
    mask[1, 100:5000] = -np.inf
    mask[1, n - 777:] = -np.inf
    mask[1, 20000:20009] = -np.inf
    ds, dm, do = ctx.to_device(s), ctx.to_device(mask), ctx.empty(s.shape)
    want = oracle.softmax_ext(s, mask, 0.125)
    want1 = oracle.softmax_ext(s, None, 1.0)
    try:
        for shift in (0, 100):
            with debug_keys(ctx, 0, shift):
                hip.softmax_long_counters(reset=True)
                ctx.check(ctx.L.ps_hip_softmax_ext(ctx.h, C.byref(do.tensor()), C.byref(ds.tensor()), C.byref(dm.tensor()), 0.125, 0.0))
                got = do.numpy()
                assert np.array_equal(bits(got), bits(want)), shift
                assert np.all(got[:, 1, 100:5000] == 0.0)
                ctx.check(ctx.L.ps_hip_soft_max(ctx.h, C.byref(do.tensor()), C.byref(ds.tensor())))
                assert np.array_equal(bits(do.numpy()), bits(want1)), shift
                rows, seq = hip.softmax_long_counters()
                assert rows == 2 * nh * bs and (seq == rows if shift == 100 else seq < rows), (rows, seq)
        big = ctx.empty((1, hip.LONG_CTX_MAX + 65))
        assert ctx.L.ps_hip_soft_max(ctx.h, C.byref(big.tensor()), C.byref(big.tensor())) != 0  # beyond PS_HIP_LONG_CTX_MAX + 64 elements: refused
        big.free()
    finally:
        for a in (ds, dm, do):
            a.free()


def test_decode_sampled_across_a_capture_window(ctx, tmp_path):
    """decode_sampled shares decode_greedy's replay loop: a capture from position 0, then 40 sampled steps from position 1 010 (across the window's end at
    1 024) equal the host loop (forward + the host chain) on a second model, engine state included."""
    from powerserve_amd import hip, host, synth
    d = str(tmp_path / "m")
    synth.write_model_dir(d, "tiny-llama", Q4_K, n_ctx=2100, seed=12)
    prompt = np.random.default_rng(8).integers(0, 512, 1010)
    chain = host.Sampler(host.SamplerCfg.make(512, seed=5, temperature=0.9, top_p=0.9, top_k=30))
    dc, st = chain.device_state()
    outs = []
    for device in (True, False):
        m = hip.Model(ctx, d, max_batch=128, long_window=True)
        try:
            if device:
                dc0, st0 = host.Sampler(host.SamplerCfg.make(512, seed=1)).device_state()
                m.decode_sampled(int(prompt[0]), 2, dc0, st0)  # (the capture of positions 0 .. 1023)
                m.kv_rollback(2)
            m.prefill(prompt, 128)
            if device:
                outs.append(m.decode_sampled(5, STEPS, dc, st))
            else:
                ids, cur = [], 5
                for s in range(STEPS):
                    lg, _ = m.forward([cur], [m.position], lm_head=True)
                    cur = chain.sample(lg[0])
                    ids.append(cur)
                outs.append(np.asarray(ids, np.int32))
            assert m.position == 1010 + STEPS
        finally:
            m.close()
    assert np.array_equal(outs[0], outs[1]), outs
    words, pos = chain.engine_state()
    assert np.array_equal(np.array(st.mt[:], np.uint32), words) and st.mt_pos == pos
    chain.close()


def test_host_facade_long_window(ctx, oracle, model_root):
    """load_model(..., long_window) through psh_model_load_long: 8 query heads per kv head at 4092 slots is refused without it; with it Model::generate (the
    lowered forward: prefill chunks and the single-token steps of a long-window device model) gives the oracle's ids, and forward its logits"""
    from powerserve_amd import host
    d, cfg, runs = oracle_run(oracle, model_root, "odd-llama-r8", Q4_K)
    with pytest.raises(host.HostError, match="n_ctx too large"):
        host.HostModel(d, 0, 32, 4092)
    hm = host.HostModel(d, 0, 32, 4092, long_window=True)
    try:
        for P in PROMPTS:
            prompt, want_ids, want_logits, chunk = runs[P]
            hm.reset()
            assert np.array_equal(hm.generate(prompt, chunk, STEPS), want_ids), P
            if P == 23:  # (noted at enqueue time: the second prompt's steps replay the first one's capture, and the last enqueue was a prefill chunk's)
                assert last_attention(ctx).startswith(single_token_path(cfg)), last_attention(ctx)
        hm.reset()
        prompt, want_ids, want_logits, chunk = runs[23]
        for lo in range(0, 22, chunk):
            hi = min(lo + chunk, 22)
            hm.forward(prompt[lo:hi], np.arange(lo, hi), lm_head=False)
        lg = hm.forward([int(prompt[-1])], [22], lm_head=True)
        assert np.array_equal(bits(lg[0]), bits(want_logits[0]))
    finally:
        hm.close()
