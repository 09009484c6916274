// The row sum of a long soft-max row (csrc/k_attn_long.hip; DESIGN.md "Long context"), restated once for the kernels and for a CPU build
// (csrc/host/perplexity.cpp exports that build as psh_debug_softmax_long_sum; tests/test_long_ctx_cpu.py checks it).
//
// ggml_vec_soft_max_f32 (libs/ggml/src/ggml.c:2814-2865, the AVX2 build) turns a row of n logits into numerators e_j and returns their sum:
//   for every whole group of 8:  sum += (double)(((e4 + e0) + (e6 + e2)) + ((e5 + e1) + (e7 + e3)))      a float tree, then ONE double addition
//   for the n % 8 leftovers:     sum += (double)e_j                                                        one double addition each
// in this order, and the caller scales the row by (float)(1.0 / sum).  So the sum is M = n / 8 + n % 8 double additions of non-negative terms (floats,
// exact as doubles) in ONE fixed order, which no parallel reduction has.
//
// The certificate.  Let T be the exact sum of the M terms.  Any order of adding M non-negative doubles takes M - 1 additions, each with a relative rounding
// error of at most u = 2^-53 and no cancellation, so the computed value is T (1 + t) with |t| <= g = (M - 1) u / (1 - (M - 1) u) (Higham, Accuracy and
// Stability of Numerical Algorithms, section 4.2).  That holds for the reference's sequential sum R and for the device's S alike, hence
//   R / S  lies in  [(1 - g) / (1 + g), (1 + g) / (1 - g)]  which is inside  [1 - 2 g, 1 + 2 g / (1 - g)].
// With M <= 2^15 (n <= PS_SML_N_MAX), g < 1.0001 (M - 1) u, so |R / S - 1| < 2.0003 (M - 1) u.  The check uses eps = 4 M u = M 2^-51: its end points
// lo = fl(S fl(1 - eps)) and hi = fl(S fl(1 + eps)) carry two roundings each, a relative 2 u + u^2, and
//   lo <= S (1 - 4 M u)(1 + 2 u + u^2) < S (1 - 2.0003 (M - 1) u) <= R   for every M >= 1,  and likewise  R <= hi.
// x -> (float)(1.0 / x) is a correctly rounded division followed by a correctly rounded conversion: monotone (non-increasing).  So when both end points give
// the same float, (float)(1.0 / R) is that float, and so is (float)(1.0 / S).  Otherwise the row is NOT certified and the sum is formed again in the
// reference's own order (ps_sml_sum_seq).  A NaN or an infinity anywhere fails the comparison and takes that path too.
// ps_hip_debug_set(14, v) multiplies eps by 2^v (0 <= v <= 100; tests): at eps >= 1 nothing is certified.
#pragma once
#include "ps_expf.h"

#define PS_SML_N_MAX (131072 + 64) // PS_HIP_LONG_CTX_MAX + 64 elements: the longest row
#define PS_SML_GROUPS_MAX (PS_SML_N_MAX / 8)

// the reference's in-group association (ggml.c:2829-2833): (hi128 + lo128), movehl, movehdup.  The only copy: the single-token kernels (a1_exp8), attn_softmax_rows and
// the long rows take it from here.  Seven additions and nothing else, each rounded on its own: on the device they are __fadd_rn, which no contraction setting of a
// build (PS_CONTRACT) can fuse with a multiply of an inlined caller
PS_HD float ps_sml_group8(const float v0, const float v1, const float v2, const float v3, const float v4, const float v5, const float v6, const float v7) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float a0 = __fadd_rn(v4, v0), a1 = __fadd_rn(v5, v1), a2 = __fadd_rn(v6, v2), a3 = __fadd_rn(v7, v3);
    return __fadd_rn(__fadd_rn(a0, a2), __fadd_rn(a1, a3));
#else
    const float a0 = v4 + v0, a1 = v5 + v1, a2 = v6 + v2, a3 = v7 + v3;
    return (a0 + a2) + (a1 + a3);
#endif
}
PS_HD int ps_sml_terms(int n) { return n / 8 + n % 8; }
PS_HD double ps_sml_eps(int n, int shift) { return ldexp((double)ps_sml_terms(n), shift - 51); }

// The certificate on a sum S formed in any order: 1 = (float)(1.0 / S) is the reference's factor, 0 = not certified.  *inv = (float)(1.0 / S) either way.
PS_HD int ps_sml_certify(double S, int n, int shift, float *inv) {
    const double eps = ps_sml_eps(n, shift);
    const double lo = S * (1.0 - eps), hi = S * (1.0 + eps);
    const float f_hi = (float)(1.0 / lo), f_lo = (float)(1.0 / hi);
    *inv = (float)(1.0 / S);
    return eps < 1.0 && f_hi == f_lo;
}

// The reference's own order: the group sums one after the other, then the leftovers.  gs: the n / 8 group sums (ps_sml_group8), tail: the n % 8 last numerators.
PS_HD double ps_sml_sum_seq(const float *gs, int n_groups, const float *tail, int n_tail) {
    double sum = 0.0;
    for (int g = 0; g < n_groups; g++) sum += (double)gs[g];
    for (int t = 0; t < n_tail; t++) sum += (double)tail[t];
    return sum;
}

#if !defined(__HIPCC__)
#include <vector>
// The device's order on the host, for `lanes` lanes (64, 256, 1024: any power of two): lane l adds the group sums l, l + lanes, ... in that order, lane 0
// then the leftovers; the lanes combine over an xor tree.  (The kernel's tree pairs other partners; the certificate covers every order.)
static inline double ps_sml_sum_lanes(const float *e, int n, int lanes) {
    std::vector<double> part((size_t)lanes, 0.0);
    const int ng = n / 8;
    for (int g = 0; g < ng; g++) {
        const float *v = e + (size_t)g * 8;
        part[(size_t)(g % lanes)] += (double)ps_sml_group8(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
    }
    for (int j = ng * 8; j < n; j++) part[0] += (double)e[j];
    for (int o = lanes / 2; o > 0; o >>= 1)
        for (int l = 0; l < o; l++) part[(size_t)l] += part[(size_t)(l + o)];
    return part[0];
}
// One row of numerators e (n of them, non-negative) through both paths.  *inv_fast: (float)(1.0 / S) of the lane order; *inv_seq: the reference's factor.
// Returns 1 when the certificate closed on S (then the two are equal, or the bound is wrong).
static inline int ps_sml_row(const float *e, int n, int lanes, int shift, float *inv_fast, float *inv_seq) {
    const int ng = n / 8;
    std::vector<float> gs((size_t)ng);
    for (int g = 0; g < ng; g++) {
        const float *v = e + (size_t)g * 8;
        gs[(size_t)g] = ps_sml_group8(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
    }
    *inv_seq = (float)(1.0 / ps_sml_sum_seq(gs.data(), ng, e + (size_t)ng * 8, n - ng * 8));
    return ps_sml_certify(ps_sml_sum_lanes(e, n, lanes), n, shift, inv_fast);
}
#endif
