"""Rendezvous A of the fused Q / K / V + attention launch (k_qkvattn.hip): the tagged-granule hand-off (default) against the counter hand-off
(ps_hip_debug_set(11, 1)), on bits.

The counter form is the one test_gpu_attn_ctx.py / test_gpu_model.py check against the oracle; here every observable of the granule form must equal
it: greedy ids, every step's logits, the last layer's q and attention output, and the K / V cache rows of every layer -- eager and through the
captured graphs, from an empty cache (the new position on the first K row and the first V line) and behind a long prompt, at the windows 1024 and
4096.  Then two models in one process whose steps interleave, and the forced time-out (ps_hip_debug_set(5, n)) that sends a forward back through
the two launches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PRESET, WT = "llama-8b-dims-4l", 12
FUSED = "qkv_attn_kernel<4, "
STEPS = 40  # (across the 32-column boundary behind an empty cache)


def bits(x):
    return np.asarray(x).view(np.uint32)


def last_attention(ctx):
    return ctx.L.ps_hip_last_attention_kernel().decode()


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from powerserve_amd import synth
    d = str(tmp_path_factory.mktemp("handoff") / "m")
    synth.write_model_dir(d, PRESET, WT, n_ctx=4096, seed=11)
    return d


def set_counter(ctx, on):
    assert ctx.L.ps_hip_debug_set(11, 1 if on else 0) == 0


def prefill(gm, prompt):
    gm.reset()
    for lo in range(0, prompt.size - 1, 128):
        hi = min(lo + 128, prompt.size - 1)
        gm.forward(prompt[lo:hi], np.arange(lo, hi), lm_head=False)


def caches(gm):
    n = gm.position
    return [(gm.k_cache(L)[:n].copy(), gm.v_cache(L)[:, :n].copy()) for L in range(gm.cfg.n_layers)]


def run(ctx, d, n_ctx, prompt, counter):
    """everything one hand-off computes: per-step logits / q / att eager (mode 1) and through the captured single-token forward (mode 0), the
    caches behind each, and the greedy ids of the captured step (decode_greedy)"""
    from powerserve_amd import hip
    set_counter(ctx, counter)  # (read at enqueue: a fresh model, so no graph captured under the other setting is replayed)
    gm = hip.Model(ctx, d, max_batch=128, n_ctx=n_ctx)
    try:
        out = {}
        for mode in (1, 0):
            gm.set_mode(mode)
            prefill(gm, prompt)
            cur, res = int(prompt[-1]), []
            for s in range(STEPS):
                lg, am = gm.forward([cur], [gm.position], lm_head=True)
                assert last_attention(ctx).startswith(FUSED), (mode, s, last_attention(ctx))
                res.append((np.asarray(lg[0]).copy(), gm.scratch(1, 1)[0].copy(), gm.scratch(2, 1)[0].copy()))
                cur = int(am[0])
            out[mode] = (res, caches(gm))
        prefill(gm, prompt)
        out["ids"] = gm.decode_greedy(int(prompt[-1]), STEPS)
        assert last_attention(ctx).startswith(FUSED), last_attention(ctx)
        out["ids_caches"] = caches(gm)
        return out
    finally:
        gm.close()
        set_counter(ctx, False)


def assert_same(a, b, tag):
    for mode in (1, 0):
        (ra, ca), (rb, cb) = a[mode], b[mode]
        for s, (x, y) in enumerate(zip(ra, rb)):
            for what, u, v in zip(("logits", "q", "att"), x, y):
                assert np.array_equal(bits(u), bits(v)), (tag, mode, s, what)
        for L, ((ka, va), (kb, vb)) in enumerate(zip(ca, cb)):
            assert np.array_equal(bits(ka), bits(kb)) and np.array_equal(bits(va), bits(vb)), (tag, mode, L)
    assert np.array_equal(a["ids"], b["ids"]), tag
    for L, ((ka, va), (kb, vb)) in enumerate(zip(a["ids_caches"], b["ids_caches"])):
        assert np.array_equal(bits(ka), bits(kb)) and np.array_equal(bits(va), bits(vb)), (tag, "decode_greedy", L)


@pytest.mark.parametrize("n_ctx,n_prompt", [(1024, 1), (1024, 960), (4096, 1), (4096, 2100)])
def test_granules_match_counter(ctx, model_dir, n_ctx, n_prompt):
    prompt = np.random.default_rng(n_prompt).integers(0, 4096, n_prompt)
    want = run(ctx, model_dir, n_ctx, prompt, counter=True)
    got = run(ctx, model_dir, n_ctx, prompt, counter=False)
    assert_same(got, want, (n_ctx, n_prompt))
    # (greedy decode of a synthetic model can settle on one id: the eager logits must at least move from step to step)
    assert not np.array_equal(got[1][0][0][0], got[1][0][-1][0])


def test_two_models_interleaved(ctx, model_dir):
    """Two models in one process, their single-token forwards (eager, then captured) alternating step by step: each computes what it computes alone."""
    from powerserve_amd import hip
    prompts = [np.random.default_rng(5).integers(0, 4096, 300), np.random.default_rng(6).integers(0, 4096, 40)]
    shapes = [4096, 1024]

    def steps(models, mode):
        for gm, p in zip(models, prompts):
            gm.set_mode(mode)
            prefill(gm, p)
        curs, res = [int(p[-1]) for p in prompts], [[] for _ in models]
        for s in range(24):
            for i, gm in enumerate(models):
                lg, am = gm.forward([curs[i]], [gm.position], lm_head=True)
                assert last_attention(ctx).startswith(FUSED), (i, s, last_attention(ctx))
                res[i].append(np.asarray(lg[0]).copy())
                curs[i] = int(am[0])
        return res, [caches(gm) for gm in models]

    set_counter(ctx, False)
    alone = []
    for p, n_ctx in zip(prompts, shapes):
        gm = hip.Model(ctx, model_dir, max_batch=128, n_ctx=n_ctx)
        try:
            alone.append({})
            for mode in (1, 0):
                gm.set_mode(mode)
                prefill(gm, p)
                cur, r = int(p[-1]), []
                for s in range(24):
                    lg, am = gm.forward([cur], [gm.position], lm_head=True)
                    r.append(np.asarray(lg[0]).copy())
                    cur = int(am[0])
                alone[-1][mode] = (r, caches(gm))
        finally:
            gm.close()
    models = [hip.Model(ctx, model_dir, max_batch=128, n_ctx=n) for n in shapes]
    try:
        for mode in (1, 0):
            res, cs = steps(models, mode)
            for i in range(2):
                ra, ca = alone[i][mode]
                for s in range(24):
                    assert np.array_equal(bits(res[i][s]), bits(ra[s])), (mode, i, s)
                for L, ((k1, v1), (k2, v2)) in enumerate(zip(cs[i], ca)):
                    assert np.array_equal(bits(k1), bits(k2)) and np.array_equal(bits(v1), bits(v2)), (mode, i, L)
    finally:
        for gm in models:
            gm.close()


def test_forced_timeout_falls_back_with_the_same_bits(ctx, model_dir):
    """A time-out reported by the granule form (ps_hip_debug_set(5, 1): the flag the sweep raises) re-runs that forward on the two launches: the
    same logits and caches as the counter form, the model then on the two launches until re-armed (mode bit 6), and on the granules again after."""
    from powerserve_amd import hip
    prompt = np.random.default_rng(9).integers(0, 4096, 200)

    def go(counter, force_at):
        set_counter(ctx, counter)
        gm = hip.Model(ctx, model_dir, max_batch=128, n_ctx=4096)
        try:
            gm.set_mode(65)
            prefill(gm, prompt)
            cur, res, paths = int(prompt[-1]), [], []
            for s in range(12):
                if s == force_at:
                    assert ctx.L.ps_hip_debug_set(5, 1) == 0
                if s == force_at + 4:
                    gm.set_mode(65)  # re-arm the one-launch form
                lg, am = gm.forward([cur], [gm.position], lm_head=True)
                res.append(np.asarray(lg[0]).copy())
                paths.append(last_attention(ctx))
                cur = int(am[0])
            return res, caches(gm), paths, gm.position
        finally:
            ctx.L.ps_hip_debug_set(5, 0)
            gm.close()
            set_counter(ctx, False)

    want, want_c, _, _ = go(True, -10)
    got, got_c, paths, pos = go(False, 3)
    assert pos == prompt.size - 1 + 12
    for s in range(12):
        assert np.array_equal(bits(got[s]), bits(want[s])), s
    for L, ((k1, v1), (k2, v2)) in enumerate(zip(got_c, want_c)):
        assert np.array_equal(bits(k1), bits(k2)) and np.array_equal(bits(v1), bits(v2)), L
    assert paths[3].startswith("attn_scores_kernel<4>"), paths[3]  # (the re-run behind the time-out: the two launches)
    assert all(not p.startswith(FUSED) for p in paths[4:7]), paths
    assert all(p.startswith(FUSED) for p in paths[:3] + paths[7:]), paths
