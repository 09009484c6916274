// Scoring a row of logits against a target token (include/ps_hip.h ps_hip_score_rows / ps_hip_model_score; DESIGN.md "Scoring a text on
// the device"): the arithmetic of the reference's PerplexityCalculator::apply (app/perplexity/main.cpp:50-56) over ProbArray::softmax
// (src/sampler/prob_array.cpp:38-59), restated once for the kernels of csrc/k_score.hip and for a CPU build (csrc/host/perplexity.cpp
// exports that build as psh_debug_score_*; tests/test_score_cpu.py checks it).  Stage by stage, for a row x of n logits and a target t:
//   max    = the largest logit (std::sort descending leaves it in m_probs[0])
//   e_i    = expf(x_i - max)                         float subtraction, glibc expf (ps_expf.h)
//   sum    = e_i added one at a time IN DOUBLE, from the smallest logit to the largest
//   prob_t = (float)((double)e_t / sum)
// The sum's roundings depend on the sorted order, which no parallel reduction has.  The device adds in a fixed order of its own
// (ps_score_sum_dev_order below states it) and certifies the result: both sums are n - 1 double additions of non-negative terms, each
// within (n-1) 2^-53 / (1 - (n-1) 2^-53) of the exact sum, so they lie within eps = n 2^-51 of each other, relatively (a factor of two in
// hand, which also covers the two roundings of the end points below).  s -> (float)((double)e_t / s) is monotone: when both end points
// sum_dev (1 -+ eps) give the same float, that float IS the reference's prob_t.  A row whose end points differ is flagged and redone on
// the host, literally (ps_score_row_exact).  2 <= n <= 2^24.
#pragma once
#include "ps_expf.h"

#include <algorithm>
#include <cmath>
#include <functional>
#include <vector>

#define PS_SCORE_SL 4096 // logits per slice (one workgroup of pass 1 and of pass 2)
#define PS_SCORE_NT 256  // threads of that workgroup: lane l of it takes the quads l, l + NT, ... of its slice, four columns each, in column order
#define PS_SCORE_N_MIN 2
#define PS_SCORE_N_MAX (1 << 24)
// ps_score::flags
#define PS_SCORE_EXACT 1u     // the certificate did not close: prob comes from the host's exact routine
#define PS_SCORE_OUTSIDE 2u   // the row holds a NaN or a +inf (the reference's sort is undefined there): prob = NaN
#define PS_SCORE_NO_TARGET 4u // target -1: nothing scored, argmax and max_logit are still valid

struct ps_score_best {
    float v;
    int32_t i;
};
// the first maximum: the larger value, among equal values (-0 == +0) the smaller index.  Starts from {-inf, INT32_MAX}
PS_HD ps_score_best ps_score_better(ps_score_best a, ps_score_best b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
PS_HD int ps_score_outside(float x) { return x != x || x == __builtin_inff(); }

// eps = n 2^-51 2^shift (shift: ps_hip_debug_set key 12, tests and A/B only)
PS_HD double ps_score_eps(int n, int shift) { return ldexp((double)n, shift - 51); }

// The certificate on sum_dev: returns 0 and the certified prob_t, or PS_SCORE_EXACT (and the uncertified quotient).  eps >= 1 certifies nothing.
PS_HD uint32_t ps_score_certify(float e_t, double sum_dev, int n, int shift, float *prob) {
    const double eps = ps_score_eps(n, shift);
    const double lo = sum_dev * (1.0 - eps), hi = sum_dev * (1.0 + eps);
    const float p_hi = (float)((double)e_t / lo), p_lo = (float)((double)e_t / hi);
    if (eps < 1.0 && p_hi == p_lo) { *prob = p_lo; return 0; }
    *prob = (float)((double)e_t / sum_dev);
    return PS_SCORE_EXACT;
}

// ProbArray::softmax itself on one row: std::sort, the reverse loop, std::exp.  (The reference sorts (prob, token) pairs by prob alone; equal
// values give equal terms, so their order cannot change the sum.)
static inline float ps_score_row_exact(const float *x, int n, int t) {
    std::vector<float> p(x, x + n);
    std::sort(p.begin(), p.end(), std::greater<float>());
    const float max_prob = p[0];
    double exp_prob_sum  = 0;
    for (auto it = p.rbegin(); it != p.rend(); it++) {
        *it = std::exp(*it - max_prob);
        exp_prob_sum += *it;
    }
    float e_t = std::exp(x[t] - max_prob);
    e_t /= exp_prob_sum;
    return e_t;
}

#if !defined(__HIPCC__) // the CPU build of the fast path (ps_expf_glibc is device code under hipcc)
// The device's order of additions (csrc/k_score.hip score_sum_kernel + score_final_kernel), on the host: per slice of PS_SCORE_SL columns lane l adds
// its quads' terms serially in column order; the 64 lanes of a wave combine over an xor tree (offsets 32 .. 1), the waves in wave order; the
// slice sums are added in slice order.
static inline double ps_score_sum_dev_order(const float *x, int n, float max) {
    double total = 0.0;
    for (int c0 = 0; c0 < n; c0 += PS_SCORE_SL) {
        const int c1 = std::min(n, c0 + PS_SCORE_SL);
        double lane[PS_SCORE_NT] = {};
        for (int c = c0; c < c1; c++) lane[((c - c0) / 4) % PS_SCORE_NT] += (double)ps_expf_glibc(x[c] - max);
        for (int o = 32; o > 0; o >>= 1) {
            double next[PS_SCORE_NT];
            for (int l = 0; l < PS_SCORE_NT; l++) next[l] = lane[l] + lane[l ^ o];
            std::copy(next, next + PS_SCORE_NT, lane);
        }
        double s = lane[0];
        for (int w = 1; w < PS_SCORE_NT / 64; w++) s += lane[w * 64];
        total = c0 == 0 ? s : total + s;
    }
    return total;
}

// One row through the fast path as the device takes it: returns the flags (PS_SCORE_OUTSIDE, PS_SCORE_EXACT or 0), *prob the certified value
static inline uint32_t ps_score_row_fast(const float *x, int n, int t, int shift, float *prob, float *max_out, int32_t *argmax_out) {
    ps_score_best b{-__builtin_inff(), INT32_MAX};
    int outside = 0;
    for (int i = 0; i < n; i++) { outside |= ps_score_outside(x[i]); b = ps_score_better(b, ps_score_best{x[i], i}); }
    if (max_out) *max_out = b.v;
    if (argmax_out) *argmax_out = b.i;
    if (outside) { *prob = NAN; return PS_SCORE_OUTSIDE; }
    return ps_score_certify(ps_expf_glibc(x[t] - b.v), ps_score_sum_dev_order(x, n, b.v), n, shift, prob);
}
#endif
