"""CPU: the long-window entry points exist, and the row sum of the long soft-max (csrc/ps_softmax_long_dev.h, the source the kernels of
csrc/k_attn_long.hip compile) through its CPU build in the host facade: the sequential routine against a numpy restatement of the reference's
loop (ggml_vec_soft_max_f32, ggml.c:2825-2863), and the certificate -- whenever it closes on a sum formed in another order, (float)(1 / sum)
is the sequential routine's.  The routine takes the row's numerators e_j (any non-negative floats: how they were exponentiated is not its
business), so the rows here are made of numerators directly.  Every comparison is on bits."""
import numpy as np
import pytest

LANES = (64, 256, 1024)
N_ROWS = 100_000
N_MIN, N_MAX = 8, 40_000


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def restate(e):
    """sum += (double)(((e4 + e0) + (e6 + e2)) + ((e5 + e1) + (e7 + e3))) group after group, then sum += (double)e_j for the n % 8 leftovers;
    the factor is (float)(1.0 / sum)"""
    e = np.asarray(e, dtype=np.float32)
    n8 = e.size & ~7
    g = e[:n8].reshape(-1, 8)
    a = g[:, 4:] + g[:, :4]                        # float32: (e4 + e0), (e5 + e1), (e6 + e2), (e7 + e3)
    gs = (a[:, 0] + a[:, 2]) + (a[:, 1] + a[:, 3])  # float32
    terms = np.concatenate([gs.astype(np.float64), e[n8:].astype(np.float64)])
    s = np.cumsum(terms)[-1] if terms.size else np.float64(0)  # one addition after the other
    with np.errstate(divide="ignore"):
        return np.float32(np.float64(1.0) / s)


def test_exports():
    """the new entry points exist in both libraries (this test fails before the long-window feature)"""
    from powerserve_amd import hip, host
    L, H = hip.lib(), host.lib()
    for n in ("ps_hip_model_create_long", "ps_hip_model_is_long", "ps_hip_softmax_long_counters"):
        assert hasattr(L, n) and n in hip.EXPORTS, n
    for n in ("psh_model_load_long", "psh_debug_softmax_long_sum"):
        assert hasattr(H, n) and n in host.EXPORTS, n
    assert L.ps_hip_abi_version() == 2
    assert hip.LONG_CTX_MAX == 131072
    for key, good, bad in ((hip.DEBUG_LONG_PV_TILE, (64, 2048, 0), (33, -32, 4096)), (hip.DEBUG_LONG_EPS_SHIFT, (100, 0), (-1, 101))):
        for v in bad:
            assert L.ps_hip_debug_set(key, v) != 0, (key, v)
        for v in good:  # (ends on the default)
            assert L.ps_hip_debug_set(key, v) == 0, (key, v)


@pytest.fixture(scope="module")
def pools():
    """numerator pools the rows are cut from: soft-max-like (exp of a normal spread below the maximum) and a spread over 80 binades"""
    rng = np.random.default_rng(20260)
    m = 1 << 21
    like = np.exp(-np.abs(rng.standard_normal(m, dtype=np.float32) * 3)).astype(np.float32)
    spread = np.exp2(-80 * rng.random(m, dtype=np.float32)).astype(np.float32)
    return like, spread


def make_row(rng, pools, kind, n):
    like, spread = pools
    if kind == "equal":
        return np.full(n, 1.0, np.float32)
    if kind == "one_finite":  # every other logit -inf: e = 0
        e = np.zeros(n, np.float32)
        e[int(rng.integers(0, n))] = 1.0
        return e
    pool = spread if kind == "spread80" else like
    off = int(rng.integers(0, pool.size - n))
    e = pool[off:off + n].copy()
    if kind == "minus_inf_runs":  # runs of masked positions
        for _ in range(int(rng.integers(1, 5))):
            a = int(rng.integers(0, n))
            e[a:a + int(rng.integers(1, max(2, n // 3)))] = 0.0
    e[int(rng.integers(0, n))] = 1.0  # the row's maximum
    return e


def test_certificate_and_sequential_sum(pools):
    """~10^5 seeded rows of 8 .. 40 000 numerators (lengths log-uniform, every n % 8), the partial orders of 64, 256 and 1 024 lanes in turn: a closed
    certificate means the reordered factor IS the sequential one; eps x 2^100 never closes; the sequential factor is the restatement's.
    An uncertified row is rare: the end points differ by a relative 2 eps = M 2^-50 (M = n / 8 + n % 8 <= 5 007 terms) and a float's rounding
    boundaries are a relative 2^-24 apart, so a row fails to close with probability about M 2^-26 < 8e-5 -- 99.9 % of the rows must close."""
    from powerserve_amd import host
    rng = np.random.default_rng(131072)
    kinds = ["like"] * 10 + ["spread80"] * 4 + ["minus_inf_runs"] * 4 + ["equal", "one_finite"]
    closed = total = 0
    seen_mod = set()
    for r in range(N_ROWS):
        n = int(np.exp(rng.uniform(np.log(N_MIN), np.log(N_MAX + 1))))
        n = min(max(n, N_MIN), N_MAX)
        if r % 16 < 8:
            n = min(N_MAX, (n & ~7) + r % 8)  # every leftover count, often
        seen_mod.add(n % 8)
        kind = kinds[r % len(kinds)]
        e = make_row(rng, pools, kind, n)
        lanes = LANES[r % 3]
        ok, fast, seq = host.softmax_long_sum(e, lanes, 0)
        total += 1
        closed += ok
        if ok:
            assert bits(fast) == bits(seq), (r, kind, n, lanes)
        if r % 10 == 0:
            ok100, _, seq100 = host.softmax_long_sum(e, lanes, 100)
            assert not ok100 and bits(seq100) == bits(seq), (r, kind, n)
        if r % 25 == 0 or n < 64:
            assert bits(seq) == bits(restate(e)), (r, kind, n)
    assert seen_mod == set(range(8))
    assert closed >= 0.999 * total, (closed, total)


def test_a_row_that_does_not_certify():
    """1 / sum on a float's rounding boundary: numerators 1, 1 - 2^-23 and 2^-47 behind a group of zeros sum to S = 2 (1 - 2^-24 + 2^-48) exactly, and
    1 / S = (1 + 2^-24 + O(2^-72)) / 2 is the midpoint of the floats 0.5 and 0.5 + 2^-24 to the last bit of a double.  S (1 + eps) and S (1 - eps), eps = 4 x 2^-51,
    land on its two sides: the default certificate must stay open, and the factor comes from the sequential sum."""
    from powerserve_amd import host
    e = np.zeros(11, np.float32)
    e[8], e[9], e[10] = 1.0, np.float32(1.0) - np.float32(2.0 ** -23), np.float32(2.0 ** -47)
    for lanes in LANES:
        ok, fast, seq = host.softmax_long_sum(e, lanes, 0)
        assert not ok, lanes
        assert bits(seq) == bits(restate(e)) == bits(np.float32(0.5))  # (the tie rounds to even)
    # the same numerators where the boundary is far: closes
    e[10] = 0.0
    e[9] = 0.25
    ok, fast, seq = host.softmax_long_sum(e, 64, 0)
    assert ok and bits(fast) == bits(seq) == bits(restate(e))
