"""CPU build of the device sampler's arithmetic (powerserve_amd/csrc/ps_sample_dev.h, exported from libps_host.so as psh_debug_*)
against the C++ standard library itself: std::mt19937, std::discrete_distribution as ProbArray::stochastic_sample builds it,
std::partial_sort with std::greater<ProbIndex>; and the whole chain against host.Sampler (csrc/host/sampler.cpp)."""
import ctypes as C

import numpy as np
import pytest

from test_sampler_vs_ref import CASES

K_MAX = 256


@pytest.fixture(scope="module")
def L():
    from powerserve_amd import host
    return host.lib()


def _mt(L, seed):
    from powerserve_amd import host
    s = host.MtState()
    L.psh_debug_mt_seed(C.byref(s), seed)
    return s


def _words(s):
    return np.array(s.x[:], dtype=np.uint32), int(s.p)


def test_mt19937_matches_std(L):
    from powerserve_amd import host
    for seed in (0, 5489, 0xdeadbeef):
        mine, std = _mt(L, seed), host.MtState()
        L.psh_debug_std_mt_seed(C.byref(std), seed)
        assert _words(mine)[0].tolist() == _words(std)[0].tolist() and mine.p == std.p
        n = 1_000_000  # 1602 twists
        got, want = np.empty(n, np.uint32), np.empty(n, np.uint32)
        L.psh_debug_mt_next(C.byref(mine), n, got.ctypes.data)
        after = host.MtState()
        L.psh_debug_std_mt(C.byref(std), n, want.ctypes.data, C.byref(after))
        assert np.array_equal(got, want)
        assert _words(mine)[0].tolist() == _words(after)[0].tolist() and mine.p == after.p
        # round trip through the state: both continue identically from the exported words
        got2, want2 = np.empty(1000, np.uint32), np.empty(1000, np.uint32)
        L.psh_debug_mt_next(C.byref(mine), 1000, got2.ctypes.data)
        L.psh_debug_std_mt(C.byref(after), 1000, want2.ctypes.data, C.byref(host.MtState()))
        assert np.array_equal(got2, want2)


def test_discrete_draw_matches_std(L):
    rng = np.random.default_rng(3)
    mine, std = _mt(L, 11), _mt(L, 11)
    for n in list(range(1, K_MAX + 1)) + [1, 2, 3]:
        for variant in range(3):
            w = rng.random(n).astype(np.float32)
            if variant == 1:
                w[rng.integers(0, n, max(1, n // 3))] = 0.0
            if variant == 2:
                w[rng.integers(0, n, max(1, n // 4))] = np.float32(1e-40)  # subnormal
            if w.sum() == 0:
                w[0] = 1.0
            calls = C.c_uint64(0)
            p0 = mine.p
            got = L.psh_debug_discrete(C.byref(mine), w.ctypes.data, n, C.byref(calls))
            want = L.psh_debug_std_discrete(C.byref(std), w.ctypes.data, n)
            assert got == want, (n, variant)
            assert _words(mine)[0].tolist() == _words(std)[0].tolist() and mine.p == std.p, (n, variant)
            assert calls.value == (0 if n < 2 else 2)
            if n < 2:
                assert mine.p == p0  # no engine call


def _arrays():
    rng = np.random.default_rng(9)
    n = 1000
    out = {
        "all_equal": np.full(n, 0.5, np.float32),
        "three_values": rng.choice(np.array([-1.0, 0.0, 2.0], np.float32), n),
        "ascending": np.arange(n, dtype=np.float32),
        "descending": np.arange(n, dtype=np.float32)[::-1].copy(),
        "ascending_pairs": (np.arange(n) // 2).astype(np.float32),
        "signed_zeros": rng.choice(np.array([-0.0, 0.0, 1.0], np.float32), n),
        "random": rng.standard_normal(n).astype(np.float32),
    }
    nan = rng.standard_normal(n).astype(np.float32)
    nan[rng.integers(0, n, 20)] = np.nan
    out["nan_sprinkled"] = nan
    nan0 = rng.standard_normal(n).astype(np.float32)
    nan0[:5] = np.nan
    out["nan_in_first_k"] = nan0
    inf = rng.standard_normal(n).astype(np.float32)
    inf[rng.integers(0, n, 10)] = np.inf
    inf[rng.integers(0, n, 10)] = -np.inf
    out["infs"] = inf
    return out


@pytest.mark.parametrize("name,v", list(_arrays().items()))
def test_heap_path_matches_partial_sort(L, name, v):
    for n, k in [(v.size, 1), (v.size, 40), (v.size, K_MAX), (41, 40), (K_MAX + 1, K_MAX), (2, 1)]:
        x = np.ascontiguousarray(v[:n])
        gv, gt = np.empty(k, np.float32), np.empty(k, np.int32)
        wv, wt = np.empty(k, np.float32), np.empty(k, np.int32)
        L.psh_debug_partial_sort(x.ctypes.data, n, k, gv.ctypes.data, gt.ctypes.data)
        L.psh_debug_std_partial_sort(x.ctypes.data, n, k, wv.ctypes.data, wt.ctypes.data)
        assert np.array_equal(gt, wt), (name, n, k)
        assert gv.tobytes() == wv.tobytes(), (name, n, k)


@pytest.mark.parametrize("kw", [kw for kw in CASES if kw.get("top_k", 40) < 1000])
def test_chain_matches_host_sampler(L, kw):
    from powerserve_amd import hip, host
    n_vocab, steps = 1000, 300
    cfg = host.SamplerCfg.make(n_vocab, **kw)
    chain = host.Sampler(cfg)
    dc, st = chain.device_state()
    assert chain.is_standard()
    rng = np.random.default_rng(17)
    for s in range(steps):
        lg = (rng.standard_normal(n_vocab) * 2.5).astype(np.float32)
        if s % 7 == 0:
            lg[rng.integers(0, n_vocab, 3)] = lg.max()  # exact ties at the top
        if s % 11 == 0:
            lg[rng.integers(0, n_vocab, 5)] = np.sort(lg)[-int(cfg.top_k)]  # ties straddling place k
        got = L.psh_debug_chain(C.byref(dc), C.byref(st), lg.ctypes.data, n_vocab)
        assert got == chain.sample(lg), s
    words, pos = chain.engine_state()
    assert np.array_equal(np.array(st.mt[:], np.uint32), words) and st.mt_pos == pos
    chain.close()
    assert isinstance(dc, hip.SampleCfg)


def test_coverage_rules():
    from powerserve_amd import hip, host
    ok = hip.SampleCfg.from_host(host.SamplerCfg.make(1000))
    assert hip.sample_covered(ok, 1000)
    for kw in (dict(top_k=K_MAX + 1), dict(top_k=1000), dict(temperature=0.0)):
        assert not hip.sample_covered(hip.SampleCfg.from_host(host.SamplerCfg.make(1000, **kw)), 1000), kw
    s = hip.SampleState()
    s.n_window = hip.SAMPLE_WINDOW_MAX + 1
    assert not hip.sample_covered(ok, 1000, s)
    chain = host.Sampler(host.SamplerCfg.make(1000))
    assert chain.is_standard()
    chain.append_noop()
    assert not chain.is_standard()
    chain.close()
