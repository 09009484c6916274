"""GPU: fork a prefilled sequence on the device, save and restore its KV state (ps_hip_model_seq_fork / _export / _import).

The contract: after a fork (or an import) the destination behaves in every entry point BIT for bit like a sequence that had the source's history of n_tokens tokens.
Expected values come from the CPU oracle fed the same tokens with the same prefill chunking (a history of n < 37 tokens is the oracle's 37-token prefill rolled back
to n: the first n slots of the same forwards, which is what a fork copies); every comparison is on the float32 bit patterns.
"""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from conftest import load_tensors

pytestmark = pytest.mark.gpu

CHUNK = 16


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def make(tmp_path, preset, wt, n_ctx, seed, name="m"):
    from oracle import binding as B
    from powerserve_amd import synth
    d = str(tmp_path / name)
    mj = synth.write_model_dir(d, preset, wt, n_ctx=n_ctx, seed=seed)
    return d, mj, B.make_config(mj["llm_config"])


def oracle_model(oracle, d, mj, cfg):
    return oracle.model(cfg, mj["model_arch"], load_tensors(os.path.join(d, "ggml/weights.gguf")), n_threads=4)


def oracle_history(om, tokens, n):
    """the oracle behind the first n tokens of a prefill of `tokens` in chunks of CHUNK"""
    om.reset()
    done = 0
    while done < len(tokens):
        bs = min(CHUNK, len(tokens) - done)
        om.forward(tokens[done:done + bs], np.arange(done, done + bs), False)
        done += bs
    om.rollback(len(tokens) - n)
    assert om.position == n


def oracle_greedy(om, first, steps):
    tok, ids = int(first), []
    for _ in range(steps):
        tok = int(np.argmax(om.forward([tok], [om.position], True)[0]))
        ids.append(tok)
    return np.array(ids, dtype=np.int32)


def raw_fork(gm, src, dsts, n_tokens, n_dst=None):
    """ps_hip_model_seq_fork's return code (refusals are return codes, not exceptions)"""
    d = np.ascontiguousarray(dsts, dtype=np.int32)
    return gm.ctx.L.ps_hip_model_seq_fork(gm.h, int(src), d.ctypes.data_as(C.c_void_p), int(d.size if n_dst is None else n_dst), int(n_tokens))


def raw_import(gm, seq, blob):
    b = np.ascontiguousarray(blob, dtype=np.uint8)
    return gm.ctx.L.ps_hip_model_seq_import(gm.h, int(seq), b.ctypes.data_as(C.c_void_p), b.nbytes)


def raw_export(gm, seq, n_tokens, nbytes):
    buf = np.zeros(max(int(nbytes), 1), dtype=np.uint8)
    return gm.ctx.L.ps_hip_model_seq_export(gm.h, int(seq), int(n_tokens), buf.ctypes.data_as(C.c_void_p), int(nbytes))


def caches(gm, seq):
    """every layer's (K, V) of a sequence, read back through the current-sequence accessors; the current sequence is put back"""
    gm.seq_select(seq)
    return [(gm.k_cache(L), gm.v_cache(L)) for L in range(gm.cfg.n_layers)]


def caches_equal(a, b):
    return all(same(ka, kb) and same(va, vb) for (ka, va), (kb, vb) in zip(a, b))


# ---------------------------------------------------------------- 1. fork equals history
@pytest.mark.parametrize("preset", ["tiny-llama", "tiny-qwen2"])
@pytest.mark.parametrize("wt", [12, 8])  # Q4_K, Q8_0
def test_fork_equals_history(ctx, oracle, tmp_path, preset, wt):
    from powerserve_amd import hip
    d, mj, cfg = make(tmp_path, preset, wt, 1000, seed=30 + wt)  # n_ctx a multiple of 4, not of 32
    rng = np.random.default_rng(wt)
    prompt = rng.integers(0, cfg.vocab_size, 37)
    om, om_src = oracle_model(oracle, d, mj, cfg), oracle_model(oracle, d, mj, cfg)
    gm = hip.Model(ctx, d, max_batch=16)
    gm.seq_reserve(4)
    gm.seq_select(2)
    gm.prefill(prompt, CHUNK)
    oracle_history(om_src, prompt, 37)
    for n in (37, 34, 1, 0):  # V tails of 1, 2, 1 and 0 floats; a single slot; nothing
        gm.seq_fork(2, [0, 3], n)
        assert gm.seq_position(0) == gm.seq_position(3) == n and gm.seq_position(2) == om_src.position
        a, b, s = (rng.integers(0, cfg.vocab_size, 2) for _ in range(3))
        gm.seq_select(0)  # child 0: single-sequence forwards
        assert gm.position == n
        oracle_history(om, prompt, n)
        for k in range(2):
            lg, _ = gm.forward([int(a[k])], [n + k], lm_head=True)
            assert same(lg[0], om.forward([int(a[k])], [n + k], True)[0]), (n, k)
        oracle_history(om, prompt, n)
        for k in range(2):  # child 3: batched steps together with the source, which continues its own history
            lg, _ = gm.decode_batch([3, 2], [int(b[k]), int(s[k])])
            assert same(lg[0], om.forward([int(b[k])], [n + k], True)[0]), (n, k)
            assert same(lg[1], om_src.forward([int(s[k])], [om_src.position], True)[0]), (n, k)
    gm.close()
    om.close()
    om_src.close()


# ---------------------------------------------------------------- 2. nothing else is touched
def test_fork_touches_nothing_else(ctx, tmp_path):
    from powerserve_amd import hip
    d, mj, cfg = make(tmp_path, "tiny-llama", 8, 1000, seed=4)
    rng = np.random.default_rng(2)
    gm = hip.Model(ctx, d, max_batch=16)
    gm.seq_reserve(4)
    for s, n in ((0, 60), (1, 10), (2, 37)):  # 0: the destination, with a history of its own; 1: uninvolved; 2: the source; 3: uninvolved and empty
        gm.seq_select(s)
        gm.prefill(rng.integers(0, cfg.vocab_size, n), CHUNK)
    before = [caches(gm, s) for s in range(4)]
    gm.seq_select(1)
    gm.seq_fork(2, [0], 34)
    assert [gm.seq_position(s) for s in range(4)] == [34, 10, 37, 0]
    after = [caches(gm, s) for s in range(4)]
    for s in (1, 2, 3):
        assert caches_equal(before[s], after[s]), s
    for L in range(cfg.n_layers):
        (k0, v0), (k1, v1), (ks, vs) = before[0][L], after[0][L], before[2][L]
        assert np.any(k0[:34] != ks[:34])  # (the two histories differ: the copy is visible)
        assert same(k1[:34], ks[:34]) and same(v1[:, :34], vs[:, :34]), L   # the prefix is the source's
        assert same(k1[34:60], k0[34:60]) and same(v1[:, 34:60], v0[:, 34:60]), L  # behind it the old bytes
        assert np.any(k0[34:60]) and np.any(v0[:, 34:60])
        assert not np.any(bits(k1[60:])) and not np.any(bits(v1[:, 60:])), L       # and the never-written slots still zero
    gm.close()


# ---------------------------------------------------------------- 3. a full window
def test_fork_full_window(ctx, tmp_path):
    from powerserve_amd import hip
    d, mj, cfg = make(tmp_path, "tiny-llama", 8, 64, seed=6)
    gm = hip.Model(ctx, d, max_batch=16)
    gm.seq_reserve(2)
    gm.prefill(np.random.default_rng(3).integers(0, cfg.vocab_size, 64), CHUNK)
    gm.seq_fork(0, [1])  # n_tokens None: all of it
    assert gm.seq_position(1) == 64
    assert caches_equal(caches(gm, 0), caches(gm, 1))
    tok, pos, am = (np.array([x], dtype=np.int32) for x in (1, 64, 0))
    for s in (0, 1):  # one more step is refused on the child as on the source
        gm.seq_select(s)
        rc = gm.ctx.L.ps_hip_model_forward(gm.h, tok.ctypes.data_as(C.c_void_p), 1, pos.ctypes.data_as(C.c_void_p), None, 1, am.ctypes.data_as(C.c_void_p))
        assert rc == 2 and gm.position == 64, s
    gm.close()


# ---------------------------------------------------------------- 4. GQA, several layers, three children in one call
def test_fork_gqa_three_children_greedy(ctx, oracle, tmp_path):
    from powerserve_amd import hip
    d, mj, cfg = make(tmp_path, "odd-llama-r8", 12, 256, seed=9)  # 8 query heads per kv head, 2 layers
    assert cfg.n_layers >= 2 and cfg.n_heads // cfg.n_kv_heads == 8
    rng = np.random.default_rng(4)
    prompt = rng.integers(0, cfg.vocab_size, 37)
    first = [int(t) for t in rng.choice(cfg.vocab_size, 3, replace=False)]
    om = oracle_model(oracle, d, mj, cfg)
    gm = hip.Model(ctx, d, max_batch=16)
    gm.seq_reserve(4)
    gm.seq_select(1)
    gm.prefill(prompt, CHUNK)
    gm.seq_fork(1, [3, 0, 2], 35)
    got = gm.decode_batch_greedy([0, 2, 3], first, 8)
    for i in range(3):
        oracle_history(om, prompt, 35)
        assert np.array_equal(got[:, i], oracle_greedy(om, first[i], 8)), i
    assert gm.seq_position(1) == 37 and [gm.seq_position(s) for s in (0, 2, 3)] == [43] * 3
    gm.close()
    om.close()


# ---------------------------------------------------------------- 5. the captured step survives a fork into its sequence
def test_fork_into_sequence_with_captured_step(ctx, oracle, tmp_path):
    from powerserve_amd import hip
    d, mj, cfg = make(tmp_path, "tiny-llama", 12, 1000, seed=11)
    rng = np.random.default_rng(5)
    own, prompt = rng.integers(0, cfg.vocab_size, 5), rng.integers(0, cfg.vocab_size, 21)
    om = oracle_model(oracle, d, mj, cfg)
    gm = hip.Model(ctx, d, max_batch=16)
    gm.seq_reserve(2)
    gm.seq_select(1)
    gm.prefill(prompt, CHUNK)
    gm.seq_select(0)
    gm.prefill(own, CHUNK)
    oracle_history(om, own, 5)
    assert np.array_equal(gm.decode_greedy(7, 4), oracle_greedy(om, 7, 4))  # (captures the single-token step of sequence 0)
    gm.seq_fork(1, [0], 21)  # sequence 0 is the current one
    assert gm.position == 21
    oracle_history(om, prompt, 21)
    assert np.array_equal(gm.decode_greedy(9, 6), oracle_greedy(om, 9, 6))
    gm.close()
    om.close()


# ---------------------------------------------------------------- 6. refusals
def test_fork_refusals(ctx, tmp_path):
    from powerserve_amd import hip
    d, mj, cfg = make(tmp_path, "tiny-llama", 8, 64, seed=2)
    rng = np.random.default_rng(1)
    gm = hip.Model(ctx, d, max_batch=4)
    gm.seq_reserve(4)
    for s, n in enumerate((5, 9, 3, 0)):
        gm.seq_select(s)
        if n:
            gm.prefill(rng.integers(0, cfg.vocab_size, n), 4)
    before = [caches(gm, s) for s in range(4)]
    gm.seq_select(0)
    p_before = [gm.seq_position(s) for s in range(4)]

    def refused(rc):
        msg = gm.ctx.L.ps_hip_last_error(gm.ctx.h).decode()
        assert rc == 2 and msg, (rc, msg)
        assert [gm.seq_position(s) for s in range(4)] == p_before
        return msg
    refused(raw_fork(gm, 1, [0], 9, n_dst=0))
    refused(raw_fork(gm, 1, [0, 2, 3, 0], 9))            # n_dst > seq_count - 1
    refused(raw_fork(gm, 1, [0], 9, n_dst=-1))
    refused(raw_fork(gm, 1, [4], 9))                     # ids out of range
    refused(raw_fork(gm, 1, [0, -1], 9))
    refused(raw_fork(gm, 4, [0], 0))
    refused(raw_fork(gm, -1, [0], 0))
    refused(raw_fork(gm, 1, [0, 1], 9))                  # a destination equal to the source
    assert "twice" in refused(raw_fork(gm, 1, [2, 0, 2], 9))
    refused(raw_fork(gm, 1, [0], 10))                    # n_tokens > position(src)
    refused(raw_fork(gm, 3, [0], 1))
    gm.seq_select(1)
    gm.kv_mask(2, False)                                 # a hidden slot in the source
    gm.seq_select(0)
    assert "hidden" in refused(raw_fork(gm, 1, [0], 9))
    gm.seq_select(1)
    gm.kv_mask(2, True)
    for s in range(4):
        assert caches_equal(before[s], caches(gm, s)), s
    # a destination's hidden slots do not stand in the way: all its slots are visible afterwards
    gm.seq_select(2)
    gm.kv_mask(1, False)
    assert raw_fork(gm, 1, [2], 9) == 0
    lg, _ = gm.decode_batch([2, 1], [7, 7])              # (refused while a participating sequence has hidden slots)
    assert same(lg[0], lg[1])
    gm.close()
    # one sequence: nothing to fork into -- a model that never reserved, a long-window model, the fp16-KV mode
    for long_window, mode in ((False, 0), (True, 0), (False, 8)):
        one = hip.Model(ctx, d, max_batch=4, long_window=long_window)
        if mode:
            assert one.ctx.L.ps_hip_model_set_mode(one.h, mode) == 0
        one.prefill([1, 2, 3], 4)
        assert raw_fork(one, 0, [0], 3) == 2 and raw_fork(one, 0, [1], 3) == 2 and one.position == 3
        one.close()


# ---------------------------------------------------------------- 7. export / import
def test_export_import_round_trip(ctx, oracle, tmp_path):
    from powerserve_amd import hip
    d, mj, cfg = make(tmp_path, "tiny-llama", 8, 1000, seed=13)
    d2, _, cfg2 = make(tmp_path, "odd-llama-r8", 8, 64, seed=13, name="other")  # another kv_dim
    rng = np.random.default_rng(8)
    prompt, cont = rng.integers(0, cfg.vocab_size, 37), rng.integers(0, cfg.vocab_size, 6)
    L, kvd = cfg.n_layers, cfg.kv_dim
    om = oracle_model(oracle, d, mj, cfg)
    oracle_history(om, prompt, 37)
    want = [om.forward([int(t)], [37 + k], True)[0] for k, t in enumerate(cont)]  # computed once, compared three times
    om.close()
    gm = hip.Model(ctx, d, max_batch=16)
    gm.seq_reserve(2)
    gm.prefill(prompt, CHUNK)
    blob = gm.seq_export(0, 37)
    # the blob: its length, its header, its payload
    assert blob.dtype == np.uint8 and blob.size == gm.seq_state_bytes(37) == 64 + L * 2 * 37 * kvd * 4
    assert blob[:64].tobytes() == struct.pack("<4sIIIIQI32x", b"PSKV", 1, L, kvd, cfg.head_size, 37, gm.ctx.L.ps_hip_build_contract())
    pay = blob[64:].view(np.float32).reshape(L, 2, 37 * kvd)
    for i in range(L):
        assert same(pay[i, 0].reshape(37, kvd), gm.k_cache(i)[:37]) and same(pay[i, 1].reshape(kvd, 37), gm.v_cache(i)[:, :37]), i
    assert gm.position == 37  # (an export changes nothing)
    # refusals of export
    for rc in (raw_export(gm, 0, 38, gm.seq_state_bytes(38)), raw_export(gm, 0, 37, blob.size - 1), raw_export(gm, 2, 0, 64), raw_export(gm, -1, 0, 64)):
        assert rc == 2 and gm.ctx.L.ps_hip_last_error(gm.ctx.h).decode()
    gm.kv_mask(3, False)
    assert raw_export(gm, 0, 37, blob.size) == 2
    gm.kv_mask(3, True)
    # refusals of import: nothing changes
    gm.seq_select(1)
    gm.prefill(rng.integers(0, cfg.vocab_size, 9), CHUNK)
    before = caches(gm, 1)
    bad_magic, bad_version, other_build = blob.copy(), blob.copy(), blob.copy()
    bad_magic[0] ^= 1
    bad_version[4] = 2
    other_build[28] ^= 1
    for b in (blob[:-1], np.concatenate([blob, blob[:1]]), blob[:63], bad_magic, bad_version, other_build):
        assert raw_import(gm, 1, b) == 2 and gm.ctx.L.ps_hip_last_error(gm.ctx.h).decode() and gm.seq_position(1) == 9
    assert raw_import(gm, 2, blob) == 2
    assert caches_equal(before, caches(gm, 1))
    for dd, n_ctx in ((d2, 64), (d, 36)):  # another kv_dim; a window shorter than the state
        m = hip.Model(ctx, dd, max_batch=16, n_ctx=n_ctx)
        m.prefill([1, 2], CHUNK)
        z = caches(m, 0)
        assert raw_import(m, 0, blob) == 2 and m.position == 2 and caches_equal(z, caches(m, 0))
        m.close()
    f16 = hip.Model(ctx, d, max_batch=16)  # the fp16-KV mode: its mirrors are not part of a state
    assert f16.ctx.L.ps_hip_model_set_mode(f16.h, 8) == 0
    assert raw_import(f16, 0, blob) == 2 and raw_export(f16, 0, 0, 64) == 2 and f16.position == 0
    f16.close()
    # (a) another sequence of the same model (its own 9 tokens go), (b) a second instance with another window, (c) a long-window model
    gm.seq_import(1, blob)
    assert gm.seq_position(1) == 37
    after = caches(gm, 1)
    for i in range(L):  # behind the state the sequence's bytes stay: it had written 9 slots only, the rest is still zero
        assert not np.any(bits(after[i][0][37:])) and not np.any(bits(after[i][1][:, 37:])), i
    mb = hip.Model(ctx, d, max_batch=8, n_ctx=512)
    mc = hip.Model(ctx, d, max_batch=16, n_ctx=4092, long_window=True)
    assert mc.is_long
    for m in (mb, mc):
        m.seq_import(0, blob)
        assert m.position == 37
    for name, m in (("same model", gm), ("n_ctx 512", mb), ("long window", mc)):
        for k, t in enumerate(cont):
            lg, _ = m.forward([int(t)], [37 + k], lm_head=True)
            assert same(lg[0], want[k]), (name, k)
    # a state goes back out as it came in, whatever the window
    assert np.array_equal(mc.seq_export(0, 37), blob) and np.array_equal(mb.seq_export(0, 37), blob)
    empty = gm.seq_export(0, 0)
    assert empty.size == 64
    mb.seq_import(0, empty)
    assert mb.position == 0
    for m in (gm, mb, mc):
        m.close()


# ---------------------------------------------------------------- 8. host facade
def test_host_facade_fork_and_state(ctx, oracle, tmp_path):
    from powerserve_amd import host
    d, mj, cfg = make(tmp_path, "tiny-llama", 12, 96, seed=5)
    rng = np.random.default_rng(4)
    prompt = rng.integers(0, cfg.vocab_size, 14)
    toks = [int(t) for t in rng.choice(cfg.vocab_size, 4, replace=False)]
    om = oracle_model(oracle, d, mj, cfg)
    want = []
    for t in toks:
        oracle_history(om, prompt, 14)
        want.append(om.forward([t], [14], True)[0])
    om.close()
    hm = host.HostModel(d, 0, max_batch=16)
    hm.reserve_sequences(3)
    hm.prefill(prompt, CHUNK)
    hm.fork_sequence(0, [2, 1])
    assert [hm.sequence_position(s) for s in range(3)] == [14, 14, 14]
    ids, lg = hm.decode_batch([1, 2, 0], toks[:3], want_logits=True)
    for i in range(3):
        assert same(lg[i], want[i]) and int(ids[i]) == int(np.argmax(want[i])), i
    with pytest.raises(host.HostError):
        hm.fork_sequence(0, [3])
    with pytest.raises(host.HostError):
        hm.fork_sequence(1, [0], 16)
    blob = hm.export_sequence(1, 14)
    assert blob.size == 64 + cfg.n_layers * 2 * 14 * cfg.kv_dim * 4
    hm2 = host.HostModel(d, 0, max_batch=8, n_ctx=128)
    with pytest.raises(host.HostError):
        hm2.import_sequence(0, blob[:-1])
    hm2.import_sequence(0, blob)
    assert hm2.position == 14
    assert same(hm2.forward([toks[3]], [14], True)[0], want[3])
    hm.close()
    hm2.close()
