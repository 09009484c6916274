"""GPU: batched decode -- several sequences per step, each on its own KV cache (ps_hip_model_seq_* / ps_hip_model_decode_batch*).

The contract: column i of a batched step is BIT-identical to what a single-sequence model with the same history produces.  Expected values
come from the CPU oracle, one independent oracle model per sequence, or (at real layer shapes) from ps_hip_model_forward on a one-sequence
model given the same history; every comparison is on the float32 bit patterns.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_tensors

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def oracle_prefill(om, tokens, chunk):
    """the chunks ps_hip_model_prefill's contract names: forward(chunk tokens, no lm_head) at the cache position, chunk after chunk"""
    done = 0
    while done < len(tokens):
        bs = min(chunk, len(tokens) - done)
        om.forward(tokens[done:done + bs], np.arange(done, done + bs), False)
        done += bs


def make(tmp_path, preset, wt, n_ctx, seed, name="m"):
    from oracle import binding as B
    from powerserve_amd import synth
    d = str(tmp_path / name)
    mj = synth.write_model_dir(d, preset, wt, n_ctx=n_ctx, seed=seed)
    return d, mj, B.make_config(mj["llm_config"])


def raw_batch(gm, seq_ids, tokens, lm_head=1):
    """ps_hip_model_decode_batch's return code (refusals are return codes, not exceptions)"""
    s = np.ascontiguousarray(seq_ids, dtype=np.int32)
    t = np.ascontiguousarray(tokens, dtype=np.int32)
    am = np.empty(max(t.size, 1), dtype=np.int32)
    return gm.ctx.L.ps_hip_model_decode_batch(gm.h, s.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), int(t.size), lm_head, am.ctypes.data_as(C.c_void_p))


# ---------------------------------------------------------------- 1. batch equals oracle, tiny models
class SoloDevice:
    """A one-sequence ps_hip_model with the oracle model's interface.  It stands in for the oracle for F16 weights only: the CPU oracle (oracle/ps_oracle.c)
    has no F16-weight model path (the single-sequence F16 model is pinned to the real reference's recorded results by tests/test_gpu_f16.py, tests/golden/f16_*),
    so for that type a sequence's expected bits are what a single-sequence model with the same history produces on the device -- the contract's own wording."""

    def __init__(self, ctx, d):
        from powerserve_amd import hip
        self.m = hip.Model(ctx, d, max_batch=16)

    def forward(self, tokens, pos, lm_head=True):
        lg, _ = self.m.forward(tokens, pos, lm_head=lm_head)
        return lg

    def k_cache(self, L):
        return self.m.k_cache(L)

    def v_cache(self, L):
        return self.m.v_cache(L)

    def close(self):
        self.m.close()


@pytest.mark.parametrize("preset", ["tiny-llama", "tiny-qwen2"])
@pytest.mark.parametrize("wt", [2, 8, 1])  # Q4_0, Q8_0, F16
def test_batch_equals_oracle_tiny(ctx, oracle, tmp_path, preset, wt):
    from powerserve_amd import hip
    d, mj, cfg = make(tmp_path, preset, wt, 128, seed=3 + wt)
    tensors = load_tensors(os.path.join(d, "ggml/weights.gguf"))
    rng = np.random.default_rng(17)
    lens = [5, 21, 1, 40]
    steps = 24
    prompts = [rng.integers(0, cfg.vocab_size, n) for n in lens]
    forced = rng.integers(0, cfg.vocab_size, (steps, 4))
    oms = [SoloDevice(ctx, d) if wt == 1 else oracle.model(cfg, mj["model_arch"], tensors, n_threads=4) for _ in lens]
    gm = hip.Model(ctx, d, max_batch=16)
    gm.seq_reserve(4)
    assert gm.seq_count == 4
    for s, p in enumerate(prompts):
        gm.seq_select(s)
        gm.prefill(p, 8)
        oracle_prefill(oms[s], p, 8)
        assert gm.seq_position(s) == len(p) == gm.position
    for k in range(steps):
        lg, am = gm.decode_batch([0, 1, 2, 3], forced[k])
        for s in range(4):
            want = oms[s].forward([int(forced[k, s])], [lens[s] + k], True)[0]
            assert same(lg[s], want), (k, s)
            assert int(am[s]) == int(np.argmax(want)), (k, s)
    for s in range(4):
        n = lens[s] + steps
        assert gm.seq_position(s) == n
        gm.seq_select(s)
        for L in range(cfg.n_layers):
            assert same(gm.k_cache(L)[:n], oms[s].k_cache(L)[:n]), (s, L)
            assert same(gm.v_cache(L)[:, :n], oms[s].v_cache(L)[:, :n]), (s, L)
    gm.close()
    for om in oms:
        om.close()


# the head sizes and head ratios the tiny presets do not reach -- head size 96 (three 32-lane blocks per row), head size 32 with one query head per kv head, eight
# query heads per kv head (the most the column kernels hold) -- with both load forms of the per-sequence kernels forced (ps_hip_debug_set(9, 0 / 1): plain / non-temporal)
ODD_PRESETS = ["odd-llama-hs96", "odd-llama-hs32", "odd-llama-r8"]
ODD_LENS = [1, 31, 33, 70]  # prompts that end before, at and behind a 32-position block, leaving n % 8 and n % 32 tails
ODD_STEPS = 6


@pytest.fixture(scope="module")
def odd_refs(tmp_path_factory):
    """per preset, filled on first use and then only read: the model directory, the prompts, the forced tokens, and the oracle's logits and caches"""
    return {"base": tmp_path_factory.mktemp("odd"), "refs": {}}


def odd_reference(odd_refs, oracle, preset):
    if preset in odd_refs["refs"]:
        return odd_refs["refs"][preset]
    d, mj, cfg = make(odd_refs["base"], preset, 8, 128, seed=29, name=preset)
    tensors = load_tensors(os.path.join(d, "ggml/weights.gguf"))
    rng = np.random.default_rng(23)
    prompts = [rng.integers(0, cfg.vocab_size, n) for n in ODD_LENS]
    forced = rng.integers(0, cfg.vocab_size, (ODD_STEPS, len(ODD_LENS)))
    want, kc, vc = [], [], []
    for s, p in enumerate(prompts):  # one independent oracle model per sequence
        om = oracle.model(cfg, mj["model_arch"], tensors, n_threads=4)
        oracle_prefill(om, p, 8)
        want.append([om.forward([int(forced[k, s])], [len(p) + k], True)[0].copy() for k in range(ODD_STEPS)])
        n = len(p) + ODD_STEPS
        kc.append([om.k_cache(L)[:n].copy() for L in range(cfg.n_layers)])
        vc.append([om.v_cache(L)[:, :n].copy() for L in range(cfg.n_layers)])
        om.close()
    odd_refs["refs"][preset] = (d, cfg, prompts, forced, want, kc, vc)
    return odd_refs["refs"][preset]


@pytest.mark.parametrize("kvs", [0, 1])
@pytest.mark.parametrize("preset", ODD_PRESETS)
def test_batch_equals_oracle_odd_shapes(ctx, oracle, odd_refs, preset, kvs):
    from powerserve_amd import hip
    d, cfg, prompts, forced, want, kc, vc = odd_reference(odd_refs, oracle, preset)
    assert ctx.L.ps_hip_debug_set(9, kvs) == 0
    try:
        gm = hip.Model(ctx, d, max_batch=16)
        gm.seq_reserve(len(prompts))
        for s, p in enumerate(prompts):
            gm.seq_select(s)
            gm.prefill(p, 8)
            assert gm.seq_position(s) == len(p)
        for k in range(ODD_STEPS):
            lg, am = gm.decode_batch(np.arange(len(prompts)), forced[k])
            for s in range(len(prompts)):
                assert same(lg[s], want[s][k]), (k, s)
                assert int(am[s]) == int(np.argmax(want[s][k])), (k, s)
        for s, p in enumerate(prompts):
            n = len(p) + ODD_STEPS
            assert gm.seq_position(s) == n
            gm.seq_select(s)
            for L in range(cfg.n_layers):
                assert same(gm.k_cache(L)[:n], kc[s][L]), (s, L)
                assert same(gm.v_cache(L)[:, :n], vc[s][L]), (s, L)
        gm.close()
    finally:
        ctx.L.ps_hip_debug_set(9, -1)


# ---------------------------------------------------------------- 2. batch equals solo on the device, real layer shapes
# 8B Q4_K (cut to 2 layers), Llama-3.2-1B Q4_0 (head size 64), Q4_K_M mix (all 4 layers: Q4_K V in layers 0 and 1, Q6_K V in 2 and 3); third field: layers kept (0 = all)
SHAPES = [("llama-8b-dims-4l", 12, 2), ("llama-1b-dims-2l", 2, 0), ("llama-8b-dims-4l", 1015, 0)]


@pytest.fixture(scope="module")
def shape_dirs(tmp_path_factory):
    """the model directories of SHAPES, written once (the 8B shapes cut to 2 layers)"""
    from powerserve_amd import synth
    out = {}
    for preset, wt, keep in SHAPES:
        base = tmp_path_factory.mktemp(f"{preset}-{wt}")
        d = str(base / "full")
        synth.write_model_dir(d, preset, wt, n_ctx=4096, seed=41 + wt % 7)
        if keep:
            d2 = str(base / "cut")
            synth.truncate_model_dir(d, d2, keep)
            d = d2
        out[(preset, wt)] = d
    return out


def ragged_positions(n_ctx):
    return [0, 1, 31, 33, 255, 700, 2100, n_ctx - 2]


@pytest.mark.parametrize("n_ctx", [4092, 4096])
@pytest.mark.parametrize("preset,wt,keep", SHAPES)
def test_batch_equals_solo_real_shapes(ctx, shape_dirs, preset, wt, keep, n_ctx):
    from powerserve_amd import hip
    d = shape_dirs[(preset, wt)]
    rng = np.random.default_rng(n_ctx + wt)
    pos = ragged_positions(n_ctx)
    gm = hip.Model(ctx, d, max_batch=128, n_ctx=n_ctx)
    vocab = gm.cfg.vocab_size
    hist = [rng.integers(0, vocab, p) for p in pos]
    gm.seq_reserve(8)
    for s, h in enumerate(hist):
        gm.seq_select(s)
        if len(h):
            gm.prefill(h, 128)
    order = [3, 7, 0, 5, 1, 6, 2, 4]  # column i is sequence order[i]
    got = []
    toks = rng.integers(0, vocab, (2, 8))
    for k in range(2):  # the second step takes the longest sequence to its last slot
        lg, am = gm.decode_batch(order, toks[k])
        got.append((lg, am))
    for s in range(8):
        assert gm.seq_position(s) == pos[s] + 2
    solo = hip.Model(ctx, d, max_batch=128, n_ctx=n_ctx)
    for i, s in enumerate(order):
        solo.reset()
        if len(hist[s]):
            solo.prefill(hist[s], 128)
        for k in range(2):
            lg, am = solo.forward([int(toks[k, i])], [pos[s] + k], lm_head=True)
            assert same(got[k][0][i], lg[0]), (k, i, s)
            assert int(got[k][1][i]) == int(am[0])
        gm.seq_select(s)
        n = pos[s] + 2
        for L in (0, gm.cfg.n_layers - 1):
            assert same(gm.k_cache(L)[:n], solo.k_cache(L)[:n]), (s, L)
            assert same(gm.v_cache(L)[:, :n], solo.v_cache(L)[:, :n]), (s, L)
    solo.close()
    gm.close()


def test_batch_equals_oracle_real_shape(ctx, oracle, shape_dirs):
    """the Llama-3.2-1B layer shape at n_ctx = 4092 (a multiple of 4, not of 32), ragged positions, against one oracle model per sequence"""
    import json

    from oracle import binding as B
    from powerserve_amd import hip
    n_ctx = 4092
    d = shape_dirs[("llama-1b-dims-2l", 2)]
    mj = json.load(open(os.path.join(d, "model.json")))
    llm = dict(mj["llm_config"])
    llm["n_ctx"] = n_ctx
    cfg = B.make_config(llm)
    tensors = load_tensors(os.path.join(d, "ggml/weights.gguf"))
    rng = np.random.default_rng(99)
    pos = ragged_positions(n_ctx)
    hist = [rng.integers(0, cfg.vocab_size, p) for p in pos]
    toks = rng.integers(0, cfg.vocab_size, (2, 8))
    gm = hip.Model(ctx, d, max_batch=128, n_ctx=n_ctx)
    gm.seq_reserve(8)
    for s, h in enumerate(hist):
        gm.seq_select(s)
        if len(h):
            gm.prefill(h, 128)
    got = [gm.decode_batch(np.arange(8), toks[k])[0] for k in range(2)]
    gm.close()
    for s in range(8):
        om = oracle.model(cfg, mj["model_arch"], tensors, n_threads=min(16, os.cpu_count() or 8))
        oracle_prefill(om, hist[s], 128)
        for k in range(2):
            want = om.forward([int(toks[k, s])], [pos[s] + k], True)[0]
            assert same(got[k][s], want), (k, s)
        om.close()


# ---------------------------------------------------------------- 3. membership does not matter
def test_membership_does_not_matter(ctx, tmp_path):
    from powerserve_amd import hip
    d, mj, cfg = make(tmp_path, "small-llama-hs128", 12, 256, seed=8)
    rng = np.random.default_rng(5)
    n_seq, steps = 16, 12
    prompts = [rng.integers(0, cfg.vocab_size, int(n)) for n in rng.integers(1, 90, n_seq)]
    forced = rng.integers(0, cfg.vocab_size, steps)
    alone = hip.Model(ctx, d, max_batch=16)
    alone.prefill(prompts[0], 16)
    want = [alone.forward([int(forced[k])], [alone.position], lm_head=True)[0][0] for k in range(steps)]
    alone.close()
    gm = hip.Model(ctx, d, max_batch=16)
    gm.seq_reserve(n_seq)
    for s, p in enumerate(prompts):
        gm.seq_select(s)
        gm.prefill(p, 16)
    sizes = [1, 2, 5, 16, 5, 2, 16, 1, 2, 5, 16, 5]
    for k in range(steps):
        n = sizes[k]
        others = [int(x) for x in rng.permutation(np.arange(1, n_seq))[:n - 1]]  # who else is in: changes every step
        col = int(rng.integers(0, n))                                            # and so does the column of sequence 0
        ids = others[:col] + [0] + others[col:]
        toks = [int(t) for t in rng.integers(0, cfg.vocab_size, n)]
        toks[col] = int(forced[k])
        lg, _ = gm.decode_batch(ids, toks)
        assert same(lg[col], want[k]), (k, n, col)
    gm.close()


# ---------------------------------------------------------------- 4. decode_batch_greedy
def test_decode_batch_greedy(ctx, tmp_path):
    from powerserve_amd import hip
    d, mj, cfg = make(tmp_path, "small-llama-hs128", 12, 256, seed=12)
    rng = np.random.default_rng(6)
    n, steps = 5, 32
    prompts = [rng.integers(0, cfg.vocab_size, int(k)) for k in (3, 70, 33, 1, 128)]
    first = [int(t) for t in rng.integers(0, cfg.vocab_size, n)]
    ids = [4, 0, 3, 1, 2]

    def fresh():
        gm = hip.Model(ctx, d, max_batch=16)
        gm.seq_reserve(n)
        for s, p in enumerate(prompts):
            gm.seq_select(s)
            gm.prefill(p, 16)
        return gm

    a = fresh()
    got = a.decode_batch_greedy(ids, first, steps)
    assert got.shape == (steps, n)
    last_a = a.logits(n)
    b = fresh()
    cur, rows = list(first), []
    for _ in range(steps):
        lg, am = b.decode_batch(ids, cur)
        rows.append(am.copy())
        cur = [int(x) for x in am]
    assert np.array_equal(got, np.array(rows))
    assert same(last_a, lg)
    for s in range(n):
        assert a.seq_position(s) == b.seq_position(s) == len(prompts[s]) + steps
    c = fresh()
    for i, s in enumerate(ids):  # per-sequence decode_greedy on the same histories
        c.seq_select(s)
        assert np.array_equal(c.decode_greedy(first[i], steps), got[:, i]), s
    for m in (a, b, c):
        m.close()


# ---------------------------------------------------------------- 5. nothing else moved
def test_single_sequence_paths_unmoved(ctx, tmp_path):
    from powerserve_amd import hip
    d, mj, cfg = make(tmp_path, "small-llama-hs128", 12, 256, seed=21)
    rng = np.random.default_rng(7)
    p0, p1, p2 = (rng.integers(0, cfg.vocab_size, k) for k in (40, 9, 77))
    plain = hip.Model(ctx, d, max_batch=16)  # never reserves
    plain.prefill(p0, 16)
    w1 = plain.decode_greedy(7, 6)
    gm = hip.Model(ctx, d, max_batch=16)
    gm.prefill(p0, 16)                       # sequence 0 is the cache the model was created with
    k0_addr = gm.ctx.L.ps_hip_model_k_cache(gm.h, 0)
    assert np.array_equal(gm.decode_greedy(7, 6), w1)  # (captures the single-token step)
    gm.seq_reserve(3)
    assert gm.ctx.L.ps_hip_model_k_cache(gm.h, 0) == k0_addr
    for s, p in ((1, p1), (2, p2)):
        gm.seq_select(s)
        gm.prefill(p, 16)
    t = rng.integers(0, cfg.vocab_size, (4, 2))
    for k in range(4):
        gm.decode_batch([2, 1], t[k])        # sequence 0 does not take part: untouched
    gm.seq_select(0)
    assert gm.position == 46 and gm.ctx.L.ps_hip_model_k_cache(gm.h, 0) == k0_addr
    w2 = plain.decode_greedy(int(w1[-1]), 10)
    assert np.array_equal(gm.decode_greedy(int(w1[-1]), 10), w2)
    lg_p, _ = plain.forward([3], [plain.position], lm_head=True)
    lg_g, _ = gm.forward([3], [gm.position], lm_head=True)
    assert same(lg_g, lg_p)
    # a batch that includes sequence 0, then the single-sequence step again
    lg_b, _ = gm.decode_batch([1, 0], [5, 11])
    lg_p, _ = plain.forward([11], [plain.position], lm_head=True)
    assert same(lg_b[1], lg_p[0])
    assert np.array_equal(gm.decode_greedy(2, 5), plain.decode_greedy(2, 5))

    # interleaving select / prefill / decode_batch / kv_rollback on sequence 1 leaves 0 and 2 alone
    def snap(s):
        gm.seq_select(s)
        return gm.position, gm.k_cache(1).copy(), gm.v_cache(0).copy()
    before = {s: snap(s) for s in (0, 2)}
    gm.seq_select(1)
    gm.kv_rollback(3)
    gm.prefill(rng.integers(0, cfg.vocab_size, 20), 16)
    gm.decode_batch([1], [9])
    gm.kv_rollback(5)
    gm.decode_batch([1], [4])
    assert gm.seq_position(1) == 9 + 4 + 1 - 3 + 20 + 1 - 5 + 1
    for s in (0, 2):
        pos, k, v = snap(s)
        assert pos == before[s][0] and same(k, before[s][1]) and same(v, before[s][2]), s
    plain.close()
    gm.close()


# ---------------------------------------------------------------- 6. refusals (argument refusals only)
def test_refusals(ctx, tmp_path):
    from powerserve_amd import hip
    d, mj, cfg = make(tmp_path, "tiny-llama", 12, 64, seed=2)
    rng = np.random.default_rng(1)
    gm = hip.Model(ctx, d, max_batch=4)      # min(16, max_batch) = 4
    ref = hip.Model(ctx, d, max_batch=4)
    gm.seq_reserve(6)
    prompts = [rng.integers(0, cfg.vocab_size, k) for k in (5, 9, 63, 2, 3, 4)]
    for s, p in enumerate(prompts):
        gm.seq_select(s)
        gm.prefill(p, 4)
    gm.seq_select(2)
    gm.forward([1], [63], lm_head=False)     # sequence 2 is full now
    gm.seq_select(0)

    def positions():
        return [gm.seq_position(s) for s in range(6)]
    p_before = positions()

    def refused(ids, toks):
        gm.ctx.L.ps_hip_last_error(gm.ctx.h)
        rc = raw_batch(gm, ids, toks)
        msg = gm.ctx.L.ps_hip_last_error(gm.ctx.h).decode()
        assert rc == 2 and msg, (ids, rc, msg)
        assert positions() == p_before
        return msg
    assert "twice" in refused([0, 1, 0], [1, 2, 3])
    refused([0, 6], [1, 2])                  # id out of range
    refused([-1], [1])
    assert "full" in refused([1, 2], [1, 2])  # a full sequence
    refused([0, 1, 3, 4, 5], [1, 2, 3, 4, 5])  # n > min(16, max_batch)
    refused([], [])
    refused([0], [cfg.vocab_size])
    gm.seq_select(3)
    gm.kv_mask(0, False)                     # a hidden slot in sequence 3
    gm.seq_select(0)
    assert "hidden" in refused([0, 3], [1, 2])
    gm.seq_select(3)
    gm.kv_mask(0, True)
    gm.seq_select(0)
    assert gm.ctx.L.ps_hip_model_seq_reserve(gm.h, 2) == 2       # shrinking
    assert gm.ctx.L.ps_hip_model_seq_select(gm.h, 6) == 2
    assert gm.ctx.L.ps_hip_model_set_mode(gm.h, 8) == 2          # the fp16-KV mode mirrors one cache
    # fp16-KV mode on a model of its own (one sequence): batched steps are refused there
    f16 = hip.Model(ctx, d, max_batch=4)
    assert f16.ctx.L.ps_hip_model_set_mode(f16.h, 8) == 0
    assert raw_batch(f16, [0], [1]) == 2 and f16.ctx.L.ps_hip_last_error(f16.ctx.h).decode()
    assert f16.position == 0
    assert f16.ctx.L.ps_hip_model_seq_reserve(f16.h, 2) == 2
    f16.close()
    # the next valid call is still bit-exact
    lg, _ = gm.decode_batch([3, 0], [7, 8])
    ref.prefill(prompts[0], 4)
    want0, _ = ref.forward([8], [5], lm_head=True)
    ref.reset()
    ref.prefill(prompts[3], 4)
    want3, _ = ref.forward([7], [2], lm_head=True)
    assert same(lg[1], want0[0]) and same(lg[0], want3[0])
    # n == 1 equals ps_hip_model_forward on that sequence
    lg1, _ = gm.decode_batch([0], [9])
    ref.reset()
    ref.prefill(prompts[0], 4)
    ref.forward([8], [5], lm_head=False)
    want, _ = ref.forward([9], [6], lm_head=True)
    assert same(lg1[0], want[0])
    gm.close()
    ref.close()


# ---------------------------------------------------------------- 7. host facade
def test_host_facade_decode_batch(ctx, tmp_path):
    from powerserve_amd import hip, host
    d, mj, cfg = make(tmp_path, "tiny-llama", 12, 96, seed=5)
    rng = np.random.default_rng(4)
    prompts = [rng.integers(0, cfg.vocab_size, k) for k in (14, 3, 30)]
    hm = host.HostModel(d, 0, max_batch=16)
    gm = hip.Model(ctx, d, max_batch=16)
    hm.reserve_sequences(3)
    gm.seq_reserve(3)
    for s, p in enumerate(prompts):
        hm.select_sequence(s)
        hm.prefill(p, 8)
        gm.seq_select(s)
        gm.prefill(p, 8)
        assert hm.position == gm.position == len(p) == hm.sequence_position(s)
    cur = [1, 2, 3]
    for k in range(6):
        ids_h, lg_h = hm.decode_batch([2, 0, 1], cur, want_logits=True)
        lg_g, am_g = gm.decode_batch([2, 0, 1], cur)
        assert np.array_equal(ids_h, am_g) and same(lg_h, lg_g), k
        cur = [int(x) for x in ids_h]
    assert [hm.sequence_position(s) for s in range(3)] == [20, 9, 36]
    # the op-by-op graph path follows the current sequence's cache tensors
    hm.select_sequence(1)
    gm.seq_select(1)
    hm.set_fused(False)
    lg_h = hm.forward([5], [hm.position], True)
    lg_g, _ = gm.forward([5], [gm.position], lm_head=True)
    assert same(lg_h, lg_g)
    with pytest.raises(host.HostError):
        hm.decode_batch([0, 0], [1, 2])
    with pytest.raises(ValueError):
        hm.decode_batch([0, 1], [1])
    hm.close()
    gm.close()
