"""Scoring on the device (include/ps_hip.h ps_hip_score_rows / ps_hip_model_score, csrc/k_score.hip): the probability of every target token
bit for bit what ProbArray::softmax gives (the library's host exact routine, itself checked against a restatement in tests/test_score_cpu.py),
on caller logits and behind a model's lm_head; the cache a scored text leaves is the one ps_hip_model_prefill leaves."""
import os

import numpy as np
import pytest

from test_score_cpu import bits, crafted_rows, first_argmax, outside_rows

pytestmark = pytest.mark.gpu


def load_tensors(path):
    from powerserve_amd import gguf
    rd = gguf.GGUFReader(path)
    return {n: (ti.type, np.array(rd.data(n)), ti.ne[0], (list(ti.ne) + [1])[1]) for n, ti in rd.tensors.items()}


def targets_for(lg, rng):
    """per row, in turn: none, column 0, the last (ragged) column, the arg-max, the smallest logit, a random column"""
    rows, n = lg.shape
    out = np.empty(rows, np.int32)
    for r in range(rows):
        out[r] = (-1, 0, n - 1, int(np.argmax(lg[r])), int(np.argmin(lg[r])), int(rng.integers(0, n)))[r % 6]
    return out


def check_records(rec, lg, tg, n_exact_max=None):
    """records against the host exact routine, the first maximum and the flag rules; returns the number of rows on the exact path"""
    from powerserve_amd import hip, host
    n_exact = 0
    for r in range(lg.shape[0]):
        am = first_argmax(lg[r])
        assert rec["argmax"][r] == am and bits(rec["max_logit"][r]) == bits(lg[r, am]), r
        fl = int(rec["flags"][r])
        if tg[r] < 0:
            assert fl == hip.SCORE_NO_TARGET and np.isnan(rec["prob"][r]), r
            continue
        assert fl in (0, hip.SCORE_EXACT), (r, fl)
        n_exact += fl == hip.SCORE_EXACT
        want = host.score_row_exact(lg[r], int(tg[r]))
        assert bits(rec["prob"][r]) == bits(want), (r, int(tg[r]), rec["prob"][r], want, fl)
    return n_exact


def score_on_device(ctx, lg, tg, stride=None, offset=0):
    """lg [rows][n] placed on the device with a row stride and a base offset (floats)"""
    from powerserve_amd import hip
    rows, n = lg.shape
    stride = stride or n
    buf = np.full(offset + rows * stride + 8, np.nan, np.float32)  # (NaN in the gaps: a read outside a row would show)
    for r in range(rows):
        buf[offset + r * stride: offset + r * stride + n] = lg[r]
    dev = ctx.to_device(buf)
    try:
        return hip.score_rows(ctx, dev.ptr + 4 * offset, n, stride, tg)
    finally:
        dev.free()


@pytest.mark.parametrize("rows", [1, 3, 130])
@pytest.mark.parametrize("n_vocab", [2, 7, 1000, 32003])
def test_op_matches_host_exact(ctx, n_vocab, rows):
    rng = np.random.default_rng(n_vocab * 131 + rows)
    lg = (rng.standard_normal((rows, n_vocab)) * 3).astype(np.float32)
    tg = targets_for(lg, rng)
    if rows == 1:
        tg[0] = int(np.argmin(lg[0]))
    rec = score_on_device(ctx, lg, tg)
    check_records(rec, lg, tg)


def test_op_row_stride_and_unaligned_base(ctx):
    rng = np.random.default_rng(17)
    for n, stride, offset in ((1000, 1012, 1), (1000, 1003, 0), (4100, 4101, 3)):
        lg = (rng.standard_normal((9, n)) * 3).astype(np.float32)
        tg = targets_for(lg, rng)
        check_records(score_on_device(ctx, lg, tg, stride, offset), lg, tg)


@pytest.mark.parametrize("n", [7, 1000, 4099])
def test_op_crafted_rows(ctx, n):
    """equal logits, one finite entry among -inf, copies of the maximum, a spread of 250, -0 / +0 as maxima; a NaN row and a +inf row between ordinary
    neighbours: flag bit 1 and a NaN prob for them, the neighbours unaffected"""
    from powerserve_amd import hip
    rows, tgs, outside = [], [], []
    out_rows = outside_rows(n)
    for i, (name, x, tg) in enumerate(crafted_rows(n)):
        for t in tg:
            rows.append(x); tgs.append(t); outside.append(False)
        if i < len(out_rows):
            rows.append(out_rows[i][1]); tgs.append(0); outside.append(True)
            rows.append(x); tgs.append(-1); outside.append(False)
    lg, tg, outside = np.stack(rows), np.array(tgs, np.int32), np.array(outside)
    rec = score_on_device(ctx, lg, tg)
    assert outside.sum() == 2
    assert (rec["flags"][outside] == hip.SCORE_OUTSIDE).all() and np.isnan(rec["prob"][outside]).all()
    check_records(rec[~outside], lg[~outside], tg[~outside])


def test_op_exact_path_and_counters(ctx):
    from powerserve_amd import hip
    L = hip.lib()
    rng = np.random.default_rng(23)
    cases = []
    for n in (1000, 32003):
        lg = (rng.standard_normal((130, n)) * 3).astype(np.float32)
        cases.append((lg, rng.integers(0, n, 130).astype(np.int32)))
    hip.score_counters(reset=True)
    n_exact = sum(check_records(score_on_device(ctx, lg, tg), lg, tg) for lg, tg in cases)
    assert hip.score_counters(reset=True) == (260, n_exact, 0)
    assert n_exact <= 0.02 * 260, n_exact
    try:
        assert L.ps_hip_debug_set(hip.DEBUG_SCORE_EPS_SHIFT, 60) == 0  # eps >= 1: no row is certified
        lg, tg = cases[0]
        tg = tg.copy(); tg[0] = int(np.argmin(lg[0])); tg[1] = -1
        rec = score_on_device(ctx, lg, tg)
        assert check_records(rec, lg, tg) == 129
        assert hip.score_counters(reset=True) == (129, 129, 0)
    finally:
        L.ps_hip_debug_set(hip.DEBUG_SCORE_EPS_SHIFT, 0)
    assert L.ps_hip_debug_set(hip.DEBUG_SCORE_EPS_SHIFT, -1) != 0 and L.ps_hip_debug_set(hip.DEBUG_SCORE_EPS_SHIFT, 101) != 0


def test_op_refusals(ctx):
    from powerserve_amd import hip
    dev = ctx.to_device(np.zeros(64, np.float32))
    try:
        for n, stride, tg in ((1, 1, [0]), (8, 8, [8]), (8, 8, [-2]), (8, 4, [0])):
            with pytest.raises(hip.PSHipError):
                hip.score_rows(ctx, dev.ptr, n, stride, np.array(tg, np.int32))
    finally:
        dev.free()


@pytest.mark.parametrize("preset,wt,max_batch", [("tiny-llama-v1000", 12, 128), ("tiny-llama-v1000", 12, 48), ("tiny-qwen2-v1000", 8, 128)])
def test_model_score(ctx, oracle, tmp_path, preset, wt, max_batch):
    """70 tokens in chunks of 32 (two full chunks and a ragged one; max_batch 128: one launch sequence, 48: one per chunk): the records equal the ones built from
    per-chunk forward(lm_head = 1) logits and from the oracle's, by the host exact routine; the cache and what is decoded from it equal prefill's"""
    from oracle import binding as B
    from powerserve_amd import hip, host, synth
    d = str(tmp_path / "m")
    mj = synth.write_model_dir(d, preset, wt, n_ctx=128, seed=31)
    cfg = B.make_config(mj["llm_config"])
    assert cfg.vocab_size == 1000
    n, chunk = 70, 32
    rng = np.random.default_rng(7)
    toks = rng.integers(0, cfg.vocab_size, n).astype(np.int32)
    tg = np.concatenate([toks[1:], [5]]).astype(np.int32)
    tg[0] = -1
    gm = hip.Model(ctx, d, max_batch=max_batch, n_ctx=128)
    gp = hip.Model(ctx, d, max_batch=max_batch, n_ctx=128)
    om = oracle.model(cfg, mj["model_arch"], load_tensors(os.path.join(d, "ggml/weights.gguf")), n_threads=16)
    try:
        rec = gm.score(toks, tg, chunk)
        assert gm.position == n
        for name, fwd in (("forward", lambda t, p: gp.forward(t, p, True)[0]), ("oracle", lambda t, p: om.forward(t, p, True))):
            for c0 in range(0, n, chunk):
                c1 = min(n, c0 + chunk)
                lg = fwd(toks[c0:c1], np.arange(c0, c1))
                check_records(rec[c0:c1], lg, tg[c0:c1])
        gp.reset()
        gp.prefill(toks, chunk)
        assert gp.position == n
        L = cfg.n_layers - 1
        assert np.array_equal(gm.k_cache(L)[:n].view(np.uint32), gp.k_cache(L)[:n].view(np.uint32))
        assert np.array_equal(gm.v_cache(L)[:, :n].view(np.uint32), gp.v_cache(L)[:, :n].view(np.uint32))
        assert np.array_equal(gm.decode_greedy(int(toks[-1]), 8), gp.decode_greedy(int(toks[-1]), 8))
    finally:
        gm.close(); gp.close(); om.close()


def test_model_score_refusals_and_facade(ctx, tmp_path):
    from powerserve_amd import hip, host, synth
    d = str(tmp_path / "m")
    synth.write_model_dir(d, "tiny-llama-v1000", 12, n_ctx=16, seed=3)
    gm = hip.Model(ctx, d, max_batch=16, n_ctx=16)
    try:
        toks = np.arange(4, dtype=np.int32)
        gm.forward(toks[:2], np.arange(2), lm_head=False)
        for bad in ([1, 2, 3, 1000], [1, -2, 3, 4]):
            with pytest.raises(hip.PSHipError):
                gm.score(toks, np.array(bad, np.int32), 4)
            assert gm.position == 2
        with pytest.raises(hip.PSHipError):  # 2 + 15 > n_ctx
            gm.score(np.zeros(15, np.int32), np.zeros(15, np.int32), 4)
        assert gm.position == 2
        gm.set_mode(32)
        with pytest.raises(hip.PSHipError):
            gm.score(toks, toks, 4)
        assert gm.position == 2
        gm.set_mode(0)
        rec = gm.score(toks, np.array([1, 2, 3, -1], np.int32), 4)
        assert gm.position == 6
    finally:
        gm.close()
    # Model::score of the C++ facade: the same records from an empty cache behind the same two tokens
    hm = host.HostModel(d, max_batch=16, n_ctx=16)
    try:
        hm.prefill(toks[:2], 4)
        rec2 = hm.score(toks, np.array([1, 2, 3, -1], np.int32), 4)
        assert hm.position == 6
        assert rec2.tobytes() == rec.tobytes()
    finally:
        hm.close()


def test_model_score_fp16_kv_mode_runs_single_tokens(ctx, tmp_path):
    """mode bit 3 with chunk 1 (tools/perplexity.py --chunk 1 --mode 8): every token is a single-token forward on the fp16-KV attention -- the records
    equal the ones built from that mode's own single-token forward(lm_head = 1) logits (the mode is not bit-exact against parity, it is against itself)"""
    from powerserve_amd import hip, synth
    d = str(tmp_path / "m")
    synth.write_model_dir(d, "tiny-llama-v1000", 12, n_ctx=64, seed=3)
    gm = hip.Model(ctx, d, max_batch=16, n_ctx=64)
    gf = hip.Model(ctx, d, max_batch=16, n_ctx=64)
    try:
        gm.set_mode(8); gf.set_mode(8)
        rng = np.random.default_rng(1)
        toks = rng.integers(0, 1000, 12).astype(np.int32)
        tg = np.roll(toks, -1).astype(np.int32)
        rec = gm.score(toks, tg, 1)
        assert gm.position == 12 and "flash16" in hip.lib().ps_hip_last_attention_kernel().decode()
        for i in range(12):
            lg, _ = gf.forward(toks[i:i + 1], [i], True)
            check_records(rec[i:i + 1], lg, tg[i:i + 1])
    finally:
        gm.close(); gf.close()
