"""CPU: the scoring arithmetic (csrc/ps_score_dev.h, the source the kernels of csrc/k_score.hip compile) through its CPU build in the host
facade: the exact row routine against a restatement of ProbArray::softmax written here, the fast path's certificate against the exact
routine, the PerplexityCalculator against a float32 restatement of app/perplexity/main.cpp:50-61.  Every comparison is on bits."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

_LIBM = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in ("expf", "logf"):
    getattr(_LIBM, _f).restype = C.c_float
    getattr(_LIBM, _f).argtypes = [C.c_float]


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def libm_expf(v):
    """glibc's expf, element by element (numpy's exp is another implementation)"""
    return np.array([_LIBM.expf(float(x)) for x in np.asarray(v, dtype=np.float32)], dtype=np.float32)


def restate(x, t):
    """ProbArray::softmax (src/sampler/prob_array.cpp:38-59) for the target's entry: max, expf(x - max) in float, a double sum from the
    smallest logit to the largest, (float)((double)e_t / sum)"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        d = np.sort(x) - x.max()  # ascending, float32 subtraction
        e = libm_expf(d)
        s = np.cumsum(e.astype(np.float64))[-1]  # one addition after the other
        et = np.float32(_LIBM.expf(float(np.float32(x[t] - x.max()))))
        return np.float32(np.float64(et) / s)


def crafted_rows(n):
    """(name, row, targets): the rows random data never gives.  Targets: column 0, the last column, the arg-max, the smallest logit."""
    rng = np.random.default_rng(n)
    base = (rng.standard_normal(n) * 3).astype(np.float32)
    rows = []
    rows.append(("equal", np.full(n, 1.5, np.float32)))
    one = np.full(n, -np.inf, np.float32); one[n // 3] = 0.75
    rows.append(("one_finite", one))
    cop = base.copy(); cop[rng.choice(n, min(5, n), replace=False)] = base.max() + 1
    rows.append(("max_copies", cop))
    spread = (rng.random(n) * 250 - 125).astype(np.float32)
    rows.append(("spread250", spread))
    z = -np.abs(base) - 1; z[0] = -0.0; z[n - 1] = 0.0
    if n > 4:
        z[n // 2] = -0.0
    rows.append(("zeros_max", z.astype(np.float32)))
    z2 = z.copy(); z2[0] = 0.0; z2[n - 1] = -0.0
    rows.append(("zeros_max_swapped", z2.astype(np.float32)))
    minf = base.copy(); minf[rng.choice(n, max(1, n // 4), replace=False)] = -np.inf; minf[n - 1] = 2.0
    rows.append(("some_minus_inf", minf))
    out = []
    for name, r in rows:
        finite_min = int(np.argmin(np.where(np.isfinite(r), r, np.inf)))
        tg = sorted({0, n - 1, int(np.argmax(r)), int(np.argmin(r)), finite_min})
        out.append((name, r, tg))
    return out


def outside_rows(n):
    rng = np.random.default_rng(n + 1)
    base = (rng.standard_normal(n) * 3).astype(np.float32)
    nan = base.copy(); nan[n // 2] = np.nan
    inf = base.copy(); inf[n - 1] = np.inf
    return [("nan", nan), ("plus_inf", inf)]


def first_argmax(r):
    return int(np.argmax(r))  # numpy returns the first maximum; -0 == +0


def test_exports():
    """the new entry points exist in both libraries (this test fails before the scoring feature)"""
    from powerserve_amd import hip, host
    L, H = hip.lib(), host.lib()
    for n in ("ps_hip_score_rows", "ps_hip_model_score", "ps_hip_score_counters"):
        assert hasattr(L, n) and n in hip.EXPORTS, n
    for n in ("psh_model_score", "psh_debug_score_row", "psh_debug_score_certify", "psh_ppl_create", "psh_ppl_add"):
        assert hasattr(H, n) and n in host.EXPORTS, n
    assert L.ps_hip_abi_version() == 2
    assert L.ps_hip_debug_set(hip.DEBUG_SCORE_EPS_SHIFT, 0) == 0


def test_host_exact_row_matches_restatement():
    from powerserve_amd import host
    rng = np.random.default_rng(11)
    n = 1000
    for i in range(60):
        x = (rng.standard_normal(n) * 3).astype(np.float32)
        for t in (int(rng.integers(0, n)), int(np.argmax(x)), int(np.argmin(x))):
            assert bits(host.score_row_exact(x, t)) == bits(restate(x, t)), (i, t)
    for n in (2, 7, 1000):
        for name, x, tg in crafted_rows(n):
            for t in tg:
                got, want = host.score_row_exact(x, t), restate(x, t)
                assert bits(got) == bits(want), (n, name, t, got, want)
    # what the crafted rows are for: exact values where they are known
    assert host.score_row_exact(np.full(4, 1.5, np.float32), 2) == np.float32(0.25)
    one = np.full(9, -np.inf, np.float32); one[3] = 0.75
    assert host.score_row_exact(one, 3) == np.float32(1.0) and host.score_row_exact(one, 0) == np.float32(0.0)


@pytest.mark.parametrize("n", [1000, 32003])
def test_certificate(n):
    """every row the fast path certifies carries the exact prob; few rows are not certified; eps x 2^30 certifies none"""
    from powerserve_amd import hip, host
    rng = np.random.default_rng(n)
    rows, flagged = 400, 0
    for i in range(rows):
        x = (rng.standard_normal(n) * 3).astype(np.float32)
        t = int(rng.integers(0, n))
        fl, p, mx, am = host.score_row_certify(x, t, 0)
        assert fl in (0, hip.SCORE_EXACT) and am == first_argmax(x) and bits(mx) == bits(x[am])
        if fl:
            flagged += 1
        else:
            assert bits(p) == bits(host.score_row_exact(x, t)), (i, t)
        assert host.score_row_certify(x, t, 30)[0] == hip.SCORE_EXACT
    assert flagged <= rows * 0.02, flagged


def test_certificate_crafted_and_outside():
    from powerserve_amd import hip, host
    for n in (2, 7, 1000, 4099):
        for name, x, tg in crafted_rows(n):
            for t in tg:
                fl, p, mx, am = host.score_row_certify(x, t, 0)
                assert am == first_argmax(x), (n, name)
                if not fl:
                    assert bits(p) == bits(host.score_row_exact(x, t)), (n, name, t)
        for name, x in outside_rows(n):
            fl, p, _, _ = host.score_row_certify(x, 0, 0)
            assert fl == hip.SCORE_OUTSIDE and np.isnan(p), (n, name)
    # eps >= 1 certifies nothing, not even a prob of 0
    x = np.array([0.0, -300.0], np.float32)
    assert host.score_row_certify(x, 1, 0) == (0, np.float32(0.0), np.float32(0.0), 0)
    assert host.score_row_certify(x, 1, 60)[0] == hip.SCORE_EXACT


def test_perplexity_calculator():
    """apply + accept (app/perplexity/main.cpp:50-61) in float32: log_logits[token] = logf(prob); sum += ...; ppl = expf(-sum / n)"""
    from powerserve_amd import host
    rng = np.random.default_rng(5)
    probs = np.concatenate([rng.random(300).astype(np.float32), np.array([1.0, 1e-30, 1e-42, 0.5], np.float32)])
    calc = host.PerplexityCalculator(1000)
    s, n = np.float32(0), 0
    for i, p in enumerate(probs):
        got = calc.add(int(rng.integers(0, 1000)), p)
        n += 1
        s = np.float32(s + np.float32(_LIBM.logf(float(p))))
        want = np.float32(_LIBM.expf(float(np.float32(-s / np.float32(n)))))
        assert bits(np.float32(got)) == bits(want), (i, got, want)
        assert bits(np.float32(calc.logit_sum)) == bits(s) and calc.n_tokens == n
    assert bits(np.float32(calc.current_ppl)) == bits(want)
    calc.close()
