// The standard sampler chain's arithmetic (csrc/host/sampler.cpp on top of libstdc++ 11), restated once for the device and
// for a CPU build (csrc/host/sample_dev.cpp exports that build as psh_debug_*; tests/test_sampler_device_cpu.py checks it
// against the C++ standard library itself).  What has to agree, operation for operation:
//   std::mt19937                    bits/random.tcc (_M_gen_rand, operator()): the twist, the tempering
//   generate_canonical<double, 53>  bits/random.tcc:3348-3380: p = (u0 + u1 2^32) / 2^64 in double, nextafter(1, 0) if p >= 1
//   discrete_distribution           bits/random.tcc:2656-2713: weights fw(k + 0.5) as double, < 2 weights: no engine call and 0,
//                                   forward double sum, w / sum, partial_sum, last entry = 1.0, lower_bound(p)
//   std::partial_sort(greater)      bits/stl_algo.h:1642-1650,1912-1919 + bits/stl_heap.h: __heap_select + __sort_heap
//   RepeatPenalty::apply / top_k / temperature / softmax / top_p / normalize   csrc/host/sampler.cpp
#pragma once
#include "ps_expf.h"

#define PS_MT_N 624
#define PS_MT_M 397

// libstdc++'s mt19937 state: _M_x[624], _M_p
struct ps_mt_state {
    uint32_t x[PS_MT_N];
    uint32_t p;
};

PS_HD void ps_mt_seed(ps_mt_state *s, uint32_t seed) {
    s->x[0] = seed;
    for (uint32_t i = 1; i < PS_MT_N; i++) s->x[i] = 1812433253u * (s->x[i - 1] ^ (s->x[i - 1] >> 30)) + i;
    s->p = PS_MT_N;
}

PS_HD uint32_t ps_mt_mix(uint32_t cur, uint32_t next, uint32_t far) {
    const uint32_t y = (cur & 0x80000000u) | (next & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

PS_HD void ps_mt_twist(uint32_t *x) {
    for (int k = 0; k < PS_MT_N - PS_MT_M; k++) x[k] = ps_mt_mix(x[k], x[k + 1], x[k + PS_MT_M]);
    for (int k = PS_MT_N - PS_MT_M; k < PS_MT_N - 1; k++) x[k] = ps_mt_mix(x[k], x[k + 1], x[k + (PS_MT_M - PS_MT_N)]);
    x[PS_MT_N - 1] = ps_mt_mix(x[PS_MT_N - 1], x[0], x[PS_MT_M - 1]);
}

PS_HD uint32_t ps_mt_next(uint32_t *x, uint32_t *p) {
    if (*p >= PS_MT_N) { ps_mt_twist(x); *p = 0; }
    uint32_t z = x[(*p)++];
    z ^= z >> 11;
    z ^= (z << 7) & 0x9d2c5680u;
    z ^= (z << 15) & 0xefc60000u;
    z ^= z >> 18;
    return z;
}

// generate_canonical<double, 53>(mt19937): two outputs
PS_HD double ps_mt_canonical(uint32_t *x, uint32_t *p) {
    double sum = 0.0;
    sum += (double)ps_mt_next(x, p) * 1.0;
    sum += (double)ps_mt_next(x, p) * 4294967296.0;
    double r = sum / 18446744073709551616.0;
    if (r >= 1.0) r = 0x1.fffffffffffffp-1; // nextafter(1.0, 0.0)
    return r;
}

// discrete_distribution<size_t>(n, 0, n, [](double x) { return w[(size_t)x]; })(engine); cp: n doubles of scratch.
// *calls += engine outputs consumed (0 or 2).
PS_HD int ps_discrete_draw(const float *w, int n, uint32_t *x, uint32_t *p, double *cp, uint64_t *calls) {
    if (n < 2) return 0;
    double sum = 0.0;
    for (int i = 0; i < n; i++) sum += (double)w[i];
    double acc = 0.0;
    for (int i = 0; i < n; i++) {
        const double q = (double)w[i] / sum;
        acc = i == 0 ? q : acc + q;
        cp[i] = acc;
    }
    cp[n - 1] = 1.0;
    const double u = ps_mt_canonical(x, p);
    *calls += 2;
    int first = 0, len = n; // std::lower_bound
    while (len > 0) {
        const int half = len >> 1, mid = first + half;
        if (cp[mid] < u) { first = mid + 1; len = len - half - 1; }
        else len = half;
    }
    return first;
}

// RepeatPenalty::apply on one entry seen n > 0 times in the window.  One form for both of the reference's builds: its stock
// (-ffp-contract=fast, FMA) build contracts the sum as fma(float(count > 0), present, round(float(count) * freq)), and with a
// factor of exactly 1 that fused multiply-add rounds once, like the plain sum (DESIGN.md "Sampled decode on the device").
PS_HD float ps_penalize(float x, int n, float repeat, float freq, float present) {
    x = x > 0 ? x / repeat : x * repeat;
    x -= float(n) * freq + 1.0f * present;
    return x;
}

// ---- libstdc++'s heap routines over (prob, token) with std::greater<ProbIndex> (compares prob only)
struct ps_pi {
    float v;
    int32_t t;
};

PS_HD void ps_push_heap(ps_pi *a, int hole, int top, ps_pi value) {
    int parent = (hole - 1) / 2;
    while (hole > top && a[parent].v > value.v) {
        a[hole] = a[parent];
        hole    = parent;
        parent  = (hole - 1) / 2;
    }
    a[hole] = value;
}

PS_HD void ps_adjust_heap(ps_pi *a, int hole, int len, ps_pi value) {
    const int top = hole;
    int second    = hole;
    while (second < (len - 1) / 2) {
        second = 2 * (second + 1);
        if (a[second].v > a[second - 1].v) second--;
        a[hole] = a[second];
        hole    = second;
    }
    if ((len & 1) == 0 && second == (len - 2) / 2) {
        second  = 2 * (second + 1);
        a[hole] = a[second - 1];
        hole    = second - 1;
    }
    ps_push_heap(a, hole, top, value);
}

PS_HD void ps_make_heap(ps_pi *a, int len) {
    if (len < 2) return;
    for (int parent = (len - 2) / 2;; parent--) {
        ps_adjust_heap(a, parent, len, a[parent]);
        if (parent == 0) return;
    }
}

// __pop_heap(first, first + len, result) where *result is `value`; the old top is what *result would receive
PS_HD ps_pi ps_pop_heap_into(ps_pi *a, int len, ps_pi value) {
    const ps_pi top = a[0];
    ps_adjust_heap(a, 0, len, value);
    return top;
}

PS_HD void ps_sort_heap(ps_pi *a, int len) {
    while (len > 1) {
        --len;
        a[len] = ps_pop_heap_into(a, len, a[len]);
    }
}

// std::partial_sort(a, a + k, a + n, greater) in place
PS_HD void ps_partial_sort(ps_pi *a, int k, int n) {
    ps_make_heap(a, k);
    for (int i = k; i < n; i++)
        if (a[i].v > a[0].v) a[i] = ps_pop_heap_into(a, k, a[i]);
    ps_sort_heap(a, k);
}

// ---- the chain behind top-k, on the n sorted candidates (v descending as top_k left them): temperature -> soft-max -> top-p
// -> normalize -> draw.  Returns the index of the drawn candidate; cp: n doubles of scratch.
PS_HD int ps_sample_tail(float *v, int n, float temperature, float top_p, uint32_t *x, uint32_t *p, double *cp, uint64_t *calls) {
    if (temperature != 1)
        for (int i = 0; i < n; i++) v[i] /= temperature;
    const float top = v[0];
    double total    = 0.;
    for (int i = n; i-- > 0;) {
        const float e = ps_expf_glibc(v[i] - top);
        v[i]          = e;
        total += e;
    }
    for (int i = 0; i < n; i++) v[i] = (float)((double)v[i] / total);
    if (top_p < 1.0f) {
        float mass = 0.0f;
        int keep   = 0;
        while (keep < n) {
            mass += v[keep++];
            if (mass >= top_p && keep >= 1) break;
        }
        if (keep < n) {
            n = keep;
            double t2 = 0.;
            for (int i = 0; i < n; i++) t2 += v[i];
            for (int i = 0; i < n; i++) v[i] = (float)((double)v[i] / t2);
        }
    }
    return ps_discrete_draw(v, n, x, p, cp, calls);
}
