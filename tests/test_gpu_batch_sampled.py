"""GPU: sampled batched decode -- one sampler chain per sequence inside the batched step (ps_hip_sample_rows, ps_hip_model_decode_batch_sampled; csrc/k_sample.hip's
rows kernels; DESIGN.md "Sampled batched decode").

The contract: column i is, id for id and engine word for engine word, what the single-sequence entry points draw for that sequence alone.  Expected values come from the
host Sampler (powerserve_amd/host.py, pinned to the reference's classes by tests/test_sampler_vs_ref.py) and from solo runs of ps_hip_sample / ps_hip_model_decode_sampled;
the new entry points are never compared against themselves alone.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def engine(st):
    return np.array(st.mt[:], dtype=np.uint32), int(st.mt_pos)


def same_engine(a, b):
    (wa, pa), (wb, pb) = (x if isinstance(x, tuple) else engine(x) for x in (a, b))
    return np.array_equal(wa, wb) and pa == pb


def same_state(a, b):
    """engine, its position and the accumulated diagnostics of two ps_sample_state"""
    return same_engine(a, b) and a.n_outputs == b.n_outputs and a.n_exact == b.n_exact


def clone(st):
    from powerserve_amd import hip
    c = hip.SampleState()
    C.memmove(C.byref(c), C.byref(st), C.sizeof(st))
    return c


# ---------------------------------------------------------------- 1. the rows op
ROWS = 16
PLANT_TOP, PLANT_STRADDLE, PLANT_NAN = 5, 8, 13  # three equal maxima / ties straddling place k / NaNs: the rows that must take the exact path
TWIST_ROWS = (1, 4, 10, 14)                      # start at engine position 622: the next twist falls inside the three calls (k > 1 there: k = 1 never draws)
PEN = dict(penalty_repeat=1.3, penalty_freq=0.2, penalty_present=0.1, penalty_last_n=16, penalize_nl=True)


def row_kw(r):
    kw = dict(top_k=(1, 40, 256)[r % 3], temperature=(1.0, 0.8)[(r // 3) % 2], top_p=(1.0, 0.95)[(r // 2) % 2], seed=100 + r)
    if r % 4 == 3:
        kw.update(PEN)
    return kw


def penalised(lg, cfg, st):
    """the row top-k sees: RepeatPenalty::apply (csrc/ps_sample_dev.h ps_penalize, float32 operation for operation) on the counted window's tokens"""
    active = cfg.penalty_last_n != 0 and not (cfg.penalty_repeat == 1.0 and cfg.penalty_freq == 0.0 and cfg.penalty_present == 0.0)
    if not active:
        return lg
    out = lg.copy()
    toks, cnt = np.unique(np.array(st.window[:st.n_window], dtype=np.int64), return_counts=True)
    rep, fr, pr = np.float32(cfg.penalty_repeat), np.float32(cfg.penalty_freq), np.float32(cfg.penalty_present)
    for t, c in zip(toks, cnt):
        x = out[t]
        x = np.float32(x / rep) if x > 0 else np.float32(x * rep)
        out[t] = np.float32(x - np.float32(np.float32(np.float32(c) * fr) + np.float32(np.float32(1.0) * pr)))
    return out


def has_tie(v, k):
    """does std::partial_sort's order among the k + 1 largest depend on more than the values (the exact path's condition)"""
    if np.isnan(v).any():
        return True
    top = np.sort(v)[::-1][:k + 1]
    return bool((top[:-1] == top[1:]).any())


@pytest.mark.parametrize("n_vocab", [1000, 32003, 128256])  # two slices with a ragged second; 63 x 257 candidates > the 12 288 staged in LDS (k = 256 rows); the real size
def test_rows_op_equals_host_sampler_and_solo_op(ctx, n_vocab):
    from powerserve_amd import hip, host
    stride = n_vocab + 3  # rows misaligned
    rng = np.random.default_rng(n_vocab)
    chains, cfgs, st_rows, st_solo = [], [], [], []
    warm = (rng.standard_normal(n_vocab) * 2.5).astype(np.float32)
    for r in range(ROWS):
        ch = host.Sampler(host.SamplerCfg.make(n_vocab, **row_kw(r)))
        if r in TWIST_ROWS:
            for _ in range(400):
                if ch.engine_state()[1] == 622:
                    break
                ch.sample(warm)
            assert ch.engine_state()[1] == 622, r
        dc, st = ch.device_state()
        chains.append(ch); cfgs.append(dc); st_rows.append(st); st_solo.append(clone(st))
    dev = ctx.malloc(ROWS * stride * 4)
    try:
        exact_rows = set()
        for call in range(3):
            lg = np.full((ROWS, stride), 1e30, dtype=np.float32)  # (the three floats between two rows: larger than any logit, never to be read)
            lg[:, :n_vocab] = (rng.standard_normal((ROWS, n_vocab)) * 2.5).astype(np.float32)
            row = lg[PLANT_TOP, :n_vocab]
            row[rng.choice(n_vocab, 3, replace=False)] = row.max()
            row = lg[PLANT_STRADDLE, :n_vocab]
            kth = np.sort(row)[-int(cfgs[PLANT_STRADDLE].top_k)]
            row[rng.choice(np.flatnonzero(row < kth), 3, replace=False)] = kth
            lg[PLANT_NAN, rng.choice(n_vocab, 5, replace=False)] = np.nan
            ctx.check(ctx.L.ps_hip_memcpy_h2d(ctx.h, dev, lg.ctypes.data, lg.nbytes))
            must = [has_tie(penalised(lg[r, :n_vocab], cfgs[r], st_rows[r]), int(cfgs[r].top_k)) for r in range(ROWS)]
            # the seeds are chosen so that exactly the planted rows tie: the random rows are tie-free among their k + 1 largest
            assert [r for r in range(ROWS) if must[r]] == [PLANT_TOP, PLANT_STRADDLE, PLANT_NAN], (call, must)
            e0 = [int(s.n_exact) for s in st_rows]
            got = hip.sample_rows(ctx, dev, n_vocab, stride, cfgs, st_rows)
            assert "sample_final_rows_kernel" in hip.last_sample_kernels() and "sample_slice_rows_kernel" in hip.last_sample_kernels()
            took = [int(s.n_exact) - e for s, e in zip(st_rows, e0)]
            assert took == [int(x) for x in must], (call, took, must)  # exactly the rows that must took the exact path: no row rides on its neighbour's
            exact_rows |= {r for r in range(ROWS) if took[r]}
            for r in range(ROWS):
                want = chains[r].sample(lg[r, :n_vocab])
                assert int(got[r]) == want, (call, r, int(got[r]), want)
                assert same_engine(st_rows[r], chains[r].engine_state()), (call, r)
                solo = hip.sample(ctx, dev + 4 * r * stride, n_vocab, cfgs[r], st_solo[r])
                assert solo == int(got[r]) and same_state(st_rows[r], st_solo[r]), (call, r)
        assert exact_rows == {PLANT_TOP, PLANT_STRADDLE, PLANT_NAN}
        for r in TWIST_ROWS:  # the twist happened inside the calls: the position wrapped
            assert st_rows[r].mt_pos < 622, r
    finally:
        ctx.free(dev)
        for ch in chains:
            ch.close()


def test_rows_op_refusals(ctx):
    from powerserve_amd import hip, host
    n_vocab = 1000
    dev = ctx.malloc(4 * (n_vocab + 3) * 4)
    try:
        def pair(**kw):
            return host.Sampler(host.SamplerCfg.make(n_vocab, **kw)).device_state()
        good = [pair(seed=s) for s in range(3)]
        for bad in (dict(top_k=0), dict(top_k=n_vocab), dict(temperature=0.0), dict(top_k=hip.SAMPLE_K_MAX + 1)):
            cfgs = [good[0][0], good[1][0], pair(**bad)[0], good[2][0]]
            states = [good[0][1], good[1][1], pair(**bad)[1], good[2][1]]
            before = [bytes(s) for s in states]
            with pytest.raises(hip.PSHipError, match="row 2"):
                hip.sample_rows(ctx, dev, n_vocab, n_vocab + 3, cfgs, states)
            assert [bytes(s) for s in states] == before
        cfgs, states = [g[0] for g in good], [g[1] for g in good]
        with pytest.raises(hip.PSHipError):
            hip.sample_rows(ctx, dev, n_vocab, n_vocab - 1, cfgs, states)  # row_stride < n_vocab
        with pytest.raises(hip.PSHipError):
            hip.sample_rows(ctx, dev, n_vocab, n_vocab, [], [])
        with pytest.raises(hip.PSHipError):
            hip.sample_rows(ctx, dev, n_vocab, n_vocab, cfgs * 6, states * 6)  # 18 rows
    finally:
        ctx.free(dev)


# ---------------------------------------------------------------- 2. the model, a ragged batch
LENS = (3, 70, 33, 1, 128)
SEQ_IDS = [4, 0, 3, 1, 2]  # column i is sequence SEQ_IDS[i]
COLUMN_KW = [
    dict(seed=11),                                                                                            # the reference's defaults: top-k 40, T 0.8, top-p 0.95
    dict(top_k=12, temperature=1.7, top_p=0.6, seed=99),
    dict(seed=3, **PEN),
    dict(top_k=256, top_p=1.0, temperature=1.0, seed=4),
    dict(penalty_repeat=1.15, penalty_last_n=8, penalize_nl=False, linefeed_id=13, ignore_eos=True, special_eos_id=2, seed=5),
]


def make(tmp_path, preset, wt, n_ctx, seed, name="m"):
    from powerserve_amd import synth
    d = str(tmp_path / name)
    mj = synth.write_model_dir(d, preset, wt, n_ctx=n_ctx, seed=seed)
    return d, int(mj["llm_config"]["vocab_size"])


def column_chains(vocab, kws):
    """per column: the host chain, and the device's view of its start"""
    from powerserve_amd import host
    chains = [host.Sampler(host.SamplerCfg.make(vocab, **kw)) for kw in kws]
    cfgs, states = zip(*[ch.device_state() for ch in chains])
    return chains, list(cfgs), list(states)


def prefilled(ctx, d, prompts, max_batch=16):
    """a model with one sequence behind each prompt (prefilled in chunks of min(16, max_batch)); sequence 0 is the current one"""
    from powerserve_amd import hip
    gm = hip.Model(ctx, d, max_batch=max_batch)
    gm.seq_reserve(len(prompts))
    for s, p in enumerate(prompts):
        gm.seq_select(s)
        gm.prefill(p, min(16, max_batch))
    gm.seq_select(0)
    return gm


@pytest.mark.parametrize("preset,wt,steps", [("small-llama-hs128", 12, 24), ("tiny-qwen2", 8, 8), ("tiny-llama", 1, 8)])
def test_ragged_batch_equals_solo_host_loop_and_split(ctx, tmp_path, preset, wt, steps):
    d, vocab = make(tmp_path, preset, wt, 256, seed=12)
    rng = np.random.default_rng(6)
    n = len(LENS)
    prompts = [rng.integers(0, vocab, k) for k in LENS]
    first = [int(t) for t in rng.integers(0, vocab, n)]

    a = prefilled(ctx, d, prompts)
    chains, cfgs, states = column_chains(vocab, COLUMN_KW)
    got = a.decode_batch_sampled(SEQ_IDS, first, steps, cfgs, states)
    assert got.shape == (steps, n)
    # per column: decode_sampled on that sequence of a model that never saw a batch
    c = prefilled(ctx, d, prompts)
    _, cfgs_c, states_c = column_chains(vocab, COLUMN_KW)
    for i, s in enumerate(SEQ_IDS):
        c.seq_select(s)
        assert np.array_equal(c.decode_sampled(first[i], steps, cfgs_c[i], states_c[i]), got[:, i]), (i, s)
        assert same_state(states[i], states_c[i]), i
    # the host loop: a batched step with the logits on the host, the host chain per row
    b = prefilled(ctx, d, prompts)
    cur, rows = list(first), []
    for _ in range(steps):
        lg, _ = b.decode_batch(SEQ_IDS, cur)
        cur = [chains[i].sample(lg[i]) for i in range(n)]
        rows.append(cur)
    assert np.array_equal(got, np.array(rows))
    for i in range(n):
        assert same_engine(states[i], chains[i].engine_state()), i
    # the same call split, the states carried over
    e = prefilled(ctx, d, prompts)
    _, cfgs_e, states_e = column_chains(vocab, COLUMN_KW)
    k1 = steps * 10 // 24 or 1
    p1 = e.decode_batch_sampled(SEQ_IDS, first, k1, cfgs_e, states_e)
    p2 = e.decode_batch_sampled(SEQ_IDS, [int(t) for t in p1[-1]], steps - k1, cfgs_e, states_e)
    assert np.array_equal(np.concatenate([p1, p2]), got)
    for i in range(n):
        assert same_state(states[i], states_e[i]), i
    for s in range(n):
        assert a.seq_position(s) == b.seq_position(s) == c.seq_position(s) == e.seq_position(s) == LENS[s] + steps
    for m in (a, b, c, e):
        m.close()
    for ch in chains:
        ch.close()


def test_one_step_leaves_decode_batch_logits(ctx, tmp_path):
    """steps = 1: the logits rows behind the call are decode_batch's"""
    d, vocab = make(tmp_path, "small-llama-hs128", 12, 256, seed=12)
    rng = np.random.default_rng(9)
    prompts = [rng.integers(0, vocab, k) for k in LENS]
    first = [int(t) for t in rng.integers(0, vocab, len(LENS))]
    a, b = prefilled(ctx, d, prompts), prefilled(ctx, d, prompts)
    _, cfgs, states = column_chains(vocab, COLUMN_KW)
    a.decode_batch_sampled(SEQ_IDS, first, 1, cfgs, states)
    want, _ = b.decode_batch(SEQ_IDS, first)
    assert np.array_equal(bits(a.logits(len(LENS))), bits(want))
    a.close(); b.close()


# ---------------------------------------------------------------- 3. membership does not matter
def test_membership_does_not_matter(ctx, tmp_path):
    d, vocab = make(tmp_path, "small-llama-hs128", 12, 256, seed=8)
    rng = np.random.default_rng(5)
    n_seq, steps = 16, 12
    prompts = [rng.integers(0, vocab, int(k)) for k in rng.integers(1, 90, n_seq)]
    gm = prefilled(ctx, d, prompts)
    mine = dict(seed=77)
    pool = COLUMN_KW + [dict(top_k=1), dict(top_k=2, temperature=0.5)]
    ref_ids = ref_state = None
    for n in (1, 2, 7, 16):
        others = [int(x) for x in rng.permutation(np.arange(1, n_seq))[:n - 1]]
        col = int(rng.integers(0, n))
        ids = others[:col] + [0] + others[col:]
        kws = [dict(pool[int(rng.integers(0, len(pool)))], seed=int(rng.integers(0, 1 << 30))) for _ in range(n)]
        kws[col] = mine
        toks = [int(t) for t in rng.integers(0, vocab, n)]
        toks[col] = 7
        chains, cfgs, states = column_chains(vocab, kws)
        got = gm.decode_batch_sampled(ids, toks, steps, cfgs, states)
        if ref_ids is None:
            ref_ids, ref_state = got[:, col].copy(), clone(states[col])
        assert np.array_equal(got[:, col], ref_ids), n
        assert same_state(states[col], ref_state), n
        for ch in chains:
            ch.close()
        for s in ids:  # back behind the prompts
            gm.seq_select(s)
            gm.ctx.check(gm.ctx.L.ps_hip_model_kv_truncate(gm.h, len(prompts[s])))
    # ... and alone means alone: the single-sequence entry point on a one-sequence model
    from powerserve_amd import hip
    solo = hip.Model(ctx, d, max_batch=16)
    solo.prefill(prompts[0], 16)
    _, cfgs, states = column_chains(vocab, [mine])
    assert np.array_equal(solo.decode_sampled(7, steps, cfgs[0], states[0]), ref_ids)
    assert same_state(states[0], ref_state)
    solo.close()
    gm.close()


# ---------------------------------------------------------------- 4. n completions of one prompt
def test_fork_then_sample_n_completions(ctx, tmp_path):
    from powerserve_amd import hip
    d, vocab = make(tmp_path, "small-llama-hs128", 12, 256, seed=31)
    rng = np.random.default_rng(2)
    prompt = rng.integers(0, vocab, 41)
    steps, n = 16, 8
    gm = hip.Model(ctx, d, max_batch=16)
    gm.seq_reserve(n)
    gm.prefill(prompt[:-1], 16)
    gm.seq_fork(0, list(range(1, n)))
    kws = [dict(seed=1000 + i) for i in range(n)]
    kws[7] = kws[6]  # two columns with the same seed and configuration
    _, cfgs, states = column_chains(vocab, kws)
    got = gm.decode_batch_sampled(list(range(n)), [int(prompt[-1])] * n, steps, cfgs, states)
    solo = hip.Model(ctx, d, max_batch=16)
    solo.prefill(prompt[:-1], 16)
    _, cfgs_s, states_s = column_chains(vocab, kws)
    for i in range(n):
        assert np.array_equal(solo.decode_sampled(int(prompt[-1]), steps, cfgs_s[i], states_s[i]), got[:, i]), i
        assert same_state(states[i], states_s[i]), i
        solo.ctx.check(solo.ctx.L.ps_hip_model_kv_truncate(solo.h, 40))
    assert len({tuple(got[:, i]) for i in range(n)}) >= 2  # the point of the feature: n completions, not n copies
    assert np.array_equal(got[:, 6], got[:, 7])
    solo.close()
    gm.close()


# ---------------------------------------------------------------- 5. refusals
def raw_sampled(gm, seq_ids, tokens, steps, cfg_arr, st_arr, out):
    s = np.ascontiguousarray(seq_ids, dtype=np.int32)
    t = np.ascontiguousarray(tokens, dtype=np.int32)
    return gm.ctx.L.ps_hip_model_decode_batch_sampled(gm.h, s.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), int(t.size), int(steps), cfg_arr, st_arr,
                                                      out.ctypes.data_as(C.c_void_p) if out is not None else None)


def test_refusals(ctx, tmp_path):
    from powerserve_amd import hip, host
    d, vocab = make(tmp_path, "tiny-llama", 12, 64, seed=2)
    rng = np.random.default_rng(1)
    lens = (5, 9, 60, 2, 3, 4)
    prompts = [rng.integers(0, vocab, k) for k in lens]
    gm = prefilled(ctx, d, prompts, max_batch=4)  # min(16, max_batch) = 4

    def arrays(kws, tweak=None):
        pairs = [host.Sampler(host.SamplerCfg.make(vocab, **kw)).device_state() for kw in kws]
        if tweak:
            tweak(pairs)
        return hip._struct_array(hip.SampleCfg, [p[0] for p in pairs]), hip._struct_array(hip.SampleState, [p[1] for p in pairs])

    def positions():
        return [gm.seq_position(s) for s in range(len(lens))]
    p_before = positions()
    out = np.full((8, 4), -7, dtype=np.int32)

    def refused(m, ids, toks, steps, ca, sa, o=out):
        before = bytes(sa) if sa is not None else b""
        rc = raw_sampled(m, ids, toks, steps, ca, sa, o)
        msg = m.ctx.L.ps_hip_last_error(m.ctx.h).decode()
        assert rc == 2 and msg, (ids, rc, msg)
        assert sa is None or bytes(sa) == before  # no state modified
        assert (out == -7).all()
        return msg
    good = [dict(seed=s) for s in range(4)]

    def too_long(pairs):
        pairs[1][1].n_window = hip.SAMPLE_WINDOW_MAX + 1
    # one uncovered column among covered ones: the whole call is refused, and the message names the column
    for bad in (dict(top_k=0), dict(top_k=vocab), dict(temperature=0.0)):
        ca, sa = arrays([good[0], dict(bad, seed=9), good[2]])
        assert "column 1" in refused(gm, [0, 1, 3], [1, 2, 3], 4, ca, sa)
    ca, sa = arrays(good[:3], too_long)
    assert "column 1" in refused(gm, [0, 1, 3], [1, 2, 3], 4, ca, sa)
    ca, sa = arrays(good[:3])
    assert "twice" in refused(gm, [0, 1, 0], [1, 2, 3], 4, ca, sa)                   # duplicate ids (the message names the sequence of the column)
    assert "sequence 2" in refused(gm, [0, 2, 1], [1, 2, 3], 5, ca, sa)              # 60 + 5 > 64: `steps` would overfill sequence 2
    refused(gm, [0, 6, 1], [1, 2, 3], 1, ca, sa)                                     # no such sequence
    refused(gm, [0, 1, 3], [1, vocab, 3], 1, ca, sa)                                 # token out of range
    gm.seq_select(3)
    gm.kv_mask(0, False)
    gm.seq_select(0)
    assert "sequence 3" in refused(gm, [0, 1, 3], [1, 2, 3], 4, ca, sa)              # a hidden slot
    gm.seq_select(3)
    gm.kv_mask(0, True)
    gm.seq_select(0)
    refused(gm, [0, 1, 3], [1, 2, 3], 4, None, sa)                                   # null pointers
    refused(gm, [0, 1, 3], [1, 2, 3], 4, ca, None)
    refused(gm, [0, 1, 3], [1, 2, 3], 4, ca, sa, None)
    ca5, sa5 = arrays([dict(seed=s) for s in range(5)])
    refused(gm, [0, 1, 3, 4, 5], [1, 2, 3, 4, 5], 1, ca5, sa5)                       # n > min(16, max_batch)
    assert positions() == p_before
    # steps <= 0: rc 0, nothing changed
    before = bytes(sa)
    assert raw_sampled(gm, [0, 1, 3], [1, 2, 3], 0, ca, sa, out) == 0 and bytes(sa) == before and positions() == p_before and (out == -7).all()
    # mode bit 3 and a long-window model: no batched steps there
    f16 = hip.Model(ctx, d, max_batch=4)
    assert f16.ctx.L.ps_hip_model_set_mode(f16.h, 8) == 0
    assert "mode bit 3" in refused(f16, [0], [1], 1, ca, sa)
    assert f16.position == 0
    f16.close()
    lw = hip.Model(ctx, d, max_batch=4, long_window=True)
    assert "long-window" in refused(lw, [0], [1], 1, ca, sa)
    assert lw.position == 0
    lw.close()
    # the next valid call is still what the solo entry draws
    _, cfgs, states = column_chains(vocab, good[:2])
    got = gm.decode_batch_sampled([3, 0], [7, 8], 4, cfgs, states)
    solo = hip.Model(ctx, d, max_batch=4)
    _, cfgs_s, states_s = column_chains(vocab, good[:2])
    for i, s in enumerate((3, 0)):
        solo.reset()
        solo.prefill(prompts[s], 4)
        assert np.array_equal(solo.decode_sampled((7, 8)[i], 4, cfgs_s[i], states_s[i]), got[:, i]), s
    solo.close()
    gm.close()


# ---------------------------------------------------------------- 6. nothing else moved
def test_other_entry_points_unmoved(ctx, tmp_path):
    """after a sampled batched run: decode_sampled, decode_greedy, decode_batch_greedy and ps_hip_sample give what a model that never made the call gives"""
    from powerserve_amd import hip
    d, vocab = make(tmp_path, "small-llama-hs128", 12, 256, seed=21)
    rng = np.random.default_rng(7)
    prompts = [rng.integers(0, vocab, k) for k in (40, 9, 77)]
    plain, gm = prefilled(ctx, d, prompts), prefilled(ctx, d, prompts)
    # both capture the sampled single-token step first: the batched run must leave gm's alone
    _, c0, s0 = column_chains(vocab, [dict(seed=1), dict(seed=1)])
    assert np.array_equal(plain.decode_sampled(5, 3, c0[0], s0[0]), gm.decode_sampled(5, 3, c0[1], s0[1]))
    _, cfgs, states = column_chains(vocab, COLUMN_KW[:3])
    gm.decode_batch_sampled([2, 0, 1], [1, 2, 3], 6, cfgs, states)
    for s, p in enumerate(prompts):  # back to plain's histories
        gm.seq_select(s)
        gm.ctx.check(gm.ctx.L.ps_hip_model_kv_truncate(gm.h, plain.seq_position(s)))
    gm.seq_select(0)
    _, c1, s1 = column_chains(vocab, [COLUMN_KW[2], COLUMN_KW[2]])
    assert np.array_equal(plain.decode_sampled(9, 10, c1[0], s1[0]), gm.decode_sampled(9, 10, c1[1], s1[1]))
    assert same_state(s1[0], s1[1])
    assert np.array_equal(plain.decode_greedy(4, 8), gm.decode_greedy(4, 8))
    assert np.array_equal(plain.decode_batch_greedy([1, 2, 0], [5, 6, 7], 5), gm.decode_batch_greedy([1, 2, 0], [5, 6, 7], 5))
    assert np.array_equal(bits(plain.logits(3)), bits(gm.logits(3)))
    _, c2, s2 = column_chains(vocab, [dict(seed=8), dict(seed=8)])
    toks = [hip.sample(ctx, m.ctx.L.ps_hip_model_logits(m.h), vocab, c2[i], s2[i]) for i, m in enumerate((plain, gm))]
    assert toks[0] == toks[1] and same_state(s2[0], s2[1])
    assert "sample_final_kernel" in hip.last_sample_kernels()
    plain.close(); gm.close()


# ---------------------------------------------------------------- 7. host facade
def test_host_facade_device_route_equals_host_routes(tmp_path):
    from powerserve_amd import hip, host
    d, vocab = make(tmp_path, "tiny-llama", 12, 96, seed=5)
    rng = np.random.default_rng(4)
    prompts = [rng.integers(0, vocab, k) for k in (14, 3, 30)]
    kws = COLUMN_KW[:3]
    steps, ids, first = 10, [2, 0, 1], [1, 2, 3]
    probe = rng.standard_normal(vocab).astype(np.float32)

    def run(device_sampling=True, noop=None):
        hm = host.HostModel(d, 0, max_batch=16)
        hm.reserve_sequences(3)
        for s, p in enumerate(prompts):
            hm.select_sequence(s)
            hm.prefill(p, 8)
        hm.set_device_sampling(device_sampling)
        chains = [host.Sampler(host.SamplerCfg.make(vocab, **kw)) for kw in kws]
        if noop is not None:
            chains[noop].append_noop()
        c0 = hip.sample_counters()
        got = hm.decode_batch_sampled(ids, first, steps, chains)
        drew = hip.sample_counters()[1] - c0[1]
        nxt = [ch.sample(probe) for ch in chains]  # engine and penalty history carry on
        pos = [hm.sequence_position(s) for s in range(3)]
        for ch in chains:
            ch.close()
        hm.close()
        return got, nxt, pos, drew
    dev, dev_next, dev_pos, dev_drew = run()
    assert dev.shape == (steps, 3) and dev_drew > 0  # the device drew
    for kwargs in (dict(device_sampling=False), dict(noop=1)):
        got, nxt, pos, drew = run(**kwargs)
        assert drew == 0, kwargs  # the host loop for the whole call
        assert np.array_equal(got, dev) and nxt == dev_next and pos == dev_pos == [14 + steps, 3 + steps, 30 + steps], kwargs
