// The quantized / F16 mat-mul dispatcher (host code): which launch(es) run a group of matrices that share an activation, for the model,
// the op API (ps_hip_mul_mat) and the plans that must know it in advance (psk_matmul_fuses_rope) -- one chain, walked to enqueue or to plan:
//   F16 group: gemvh.  Single column, all Q6_K / Q5_K: gemvk.  Mixed types or Q6_K / Q5_K: each(), a launch per run of a type.
//   One lane-major type (Q4_K / Q4_0 / Q8_0): from GEMM_MIN_BS columns on, the activation quantized once and gemm4k, else gemm8;
//   what they decline in column groups of 4 (one column: gemv4, gemvb, else gemv).
#include "ps_internal.h"
#include "ps_ops.h"

namespace {

// from this many columns on a launch quantizes its activation ONCE into `act` and goes to the batched kernels (2-4 columns: 4.8-4.9 ms
// per 8B forward through the batched kernel, 5.4-6.3 ms through the 4-column mat-vec)
constexpr int GEMM_MIN_BS = 2;

// One walk of the chain.  s == nullptr: a plan -- the rungs are chosen as for the real thing, nothing is enqueued.
struct Mm {
    ps_hip_ctx *c;
    const psk_mm_scratch *s;
    int n_cu;
    int64_t K, bs;

    int fail(const std::string &msg) const { if (s) c->err = msg; return 2; }
    int launched(int rc, const char *what) const { return rc ? fail(std::string(what) + " launch rc=" + std::to_string(rc)) : 0; }
    void quantize(int vdt, const psk_gemv_args &g) const { // the activation of g (with its RMSNorm for pro 1) into act
        if (s) psk_quantize_act(c->stream, vdt, g.pro == 1 ? 1 : 0, g.pro_x, nullptr, g.pro_norm_w, g.pro_eps, K, bs, s->act);
    }
};

int f16(const Mm &m, const psk_gemv_args &g) {
    if (!g.pro || g.rope) return m.fail("F16 mat-mul: needs the fp32 activation and takes no fused RoPE");
    if (!psk_gemvh_takes(g, m.K, m.bs)) return m.fail("F16 mat-mul: shape not covered");
    return m.s ? m.launched(psk_gemvh(m.c->stream, m.n_cu, g, m.s->h16, m.K, m.bs), "F16 mat-mul") : 0;
}

// One lane-major type.  *q8k: the activation was quantized to Q8_K into act (the K-quants of a split group can share it).
int lane_major(const Mm &m, const psk_gemv_args &g, bool *q8k) {
    const int64_t K = m.K, bs = m.bs;
    const int vdt = ps_hip_vec_dot_type(g.w[0]->dtype);
    const int64_t blk = vdt == PS_Q8_0 ? 32 : 256;
    const ps_act act = m.s ? m.s->act : ps_act{};
    psk_gemv_args gq = g;
    if (bs >= GEMM_MIN_BS) {
        // batches: the activation is quantized ONCE (with its RMSNorm when the launch carries one) and the weights are
        // streamed once per column group of up to 16 instead of once per 4 columns
        if (g.pro) {
            m.quantize(vdt, g);
            gq.pro = 0; gq.pro_x = nullptr;
            *q8k = vdt == PS_Q8_K;
        }
        if (psk_gemm4k_takes(gq, K, bs)) return m.s ? m.launched(psk_gemm4k(m.c->stream, m.n_cu, gq, act, K, bs), "gemm4k") : 0;
        if (psk_gemm8_takes(gq, K, bs)) return m.s ? m.launched(psk_gemm8(m.c->stream, m.n_cu, gq, act, K, bs), "gemm8") : 0;
    }
    for (int64_t c0 = 0; c0 < bs; c0 += 4) {
        const int64_t nb = bs - c0 < 4 ? bs - c0 : 4;
        psk_gemv_args gg = gq;
        for (int i = 0; i < g.n_w; i++) gg.out[i] = g.out[i] + c0 * g.ldo[i];
        if (g.residual) gg.residual = g.residual + c0 * g.ldo[0];
        if (gq.pro) gg.pro_x = g.pro_x + c0 * K;
        ps_act ac = act;
        if (m.s) { ac.qs += c0 * K; ac.d += c0 * (K / blk); ac.bs16 += c0 * (K / 16); }
        int (*launch)(hipStream_t, int, const psk_gemv_args &, ps_act, int64_t) = nullptr;
        if (psk_gemv4_takes(gg, K, nb)) launch = psk_gemv4;
        else if (psk_gemvb_takes(gg, K, nb, m.n_cu)) launch = psk_gemvb;
        else if (!psk_gemv_takes(gg, K, nb)) return m.fail("mat-vec: shape not covered");
        if (!m.s) continue;
        const int rc = launch ? launch(m.c->stream, m.n_cu, gg, ac, K) : psk_gemv(m.c->stream, m.n_cu, gg, ac, K, nb);
        if (rc) return m.launched(rc, "gemv");
    }
    return 0;
}

// Q6_K / Q5_K from the activation quantized into act
int k_quant(const Mm &m, const psk_gemv_args &g) {
    const ps_act act = m.s ? m.s->act : ps_act{};
    int (*launch)(hipStream_t, int, const psk_gemv_args &, ps_act, int64_t, int64_t);
    if (psk_gemm5k_takes(g, m.K, m.bs)) launch = psk_gemm5k; // batches: the matrix-core mat-mul with the Q5_K producer (k_gemm4k.hip)
    else if (psk_gemv5_takes(g, m.K, m.bs)) launch = psk_gemv5;
    else if (psk_gemm6k_takes(g, m.K, m.bs)) launch = psk_gemm6k; // chunks and wide trees
    else if (psk_gemv6_takes(g, m.K, m.bs)) launch = psk_gemv6;
    else return m.fail("Q5_K / Q6_K mat-mul: shape not covered");
    return m.s ? m.launched(launch(m.c->stream, m.n_cu, g, act, m.K, m.bs), "Q5_K / Q6_K mat-mul") : 0;
}

// Launches whose matrices are not all of one lane-major type (stock Q4_K_M files: attn_v / ffn_down / output in Q6_K next
// to Q4_K): one launch per run of a type, exactly the reference's op sequence (mat-mul, + bias, silu_hadamard).
int each(const Mm &m, const psk_gemv_args &g) {
    const int64_t K = m.K, bs = m.bs;
    float *const tmp[2] = {m.s ? m.s->pair[0] : nullptr, m.s ? m.s->pair[1] : nullptr};
    bool quantized = false; // the K-quants of a group share ONE Q8_K quantization of the activation
    auto quantize_once = [&]() {
        if (g.pro && !quantized) m.quantize(PS_Q8_K, g);
        quantized = true;
    };
    auto finish = [&]() {
        if (m.s && g.silu_pair) psl_silu_hadamard(m.c->stream, g.out[0], tmp[0], tmp[1], (int64_t)g.ldo[0] * bs);
        return 0;
    };
    // matrix i of the group: its own outputs, the group's epilogue parts as every type gets them
    auto one = [&](int i) {
        psk_gemv_args s{};
        s.n_w = 1; s.w[0] = g.w[i]; s.out[0] = g.silu_pair ? tmp[i] : g.out[i]; s.bias[0] = g.bias[i];
        s.ldo[0] = g.ldo[i]; s.residual = (i == 0 && !g.silu_pair) ? g.residual : nullptr;
        s.pro = g.pro; s.pro_x = g.pro_x; s.pro_norm_w = g.pro_norm_w; s.pro_eps = g.pro_eps;
        s.rope = g.rope; s.rope_wi0 = g.rope_wi0 + i; // (a Q / K / V group split by type: every launch does its part of RoPE + KV append)
        return s;
    };
    // Q5_K_M: Q / K / V and gate / up as one launch each (when k_gemvk.hip did not take them)
    psk_gemv_args all5{};
    all5.n_w = g.n_w; all5.residual = g.silu_pair ? nullptr : g.residual;
    for (int i = 0; i < g.n_w; i++) { const psk_gemv_args s = one(i); all5.w[i] = s.w[0]; all5.out[i] = s.out[0]; all5.bias[i] = s.bias[0]; all5.ldo[i] = s.ldo[0]; }
    if (g.n_w > 1 && bs == 1 && !g.rope && psk_gemv5_takes(all5, K, bs)) {
        quantize_once();
        if (m.s) if (int rc = m.launched(psk_gemv5(m.c->stream, m.n_cu, all5, m.s->act, K, bs), "Q5_K mat-vec")) return rc;
        return finish();
    }
    for (int i = 0; i < g.n_w; i++) {
        psk_gemv_args s = one(i);
        const int wt = g.w[i]->dtype;
        if (wt == PS_F16) { // (its own rounding, in its prologue for one column)
            if (int rc = f16(m, s)) return rc;
        } else if (wt == PS_Q6_K || wt == PS_Q5_K) {
            // one matrix of a mixed group (Q4_K_M: a Q6_K V next to Q4_K Q and K), or a run of Q5_K ones (Q5_K_M: Q and K next to a Q6_K V):
            // its own prologue
            int run = 1;
            while (wt == PS_Q5_K && !g.silu_pair && i + run < g.n_w && g.w[i + run]->dtype == PS_Q5_K) run++;
            for (int j = 1; j < run; j++) { s.w[j] = g.w[i + j]; s.out[j] = g.out[i + j]; s.bias[j] = g.bias[i + j]; s.ldo[j] = g.ldo[i + j]; }
            s.n_w = run;
            if (psk_gemvk_takes(s, K, bs)) {
                if (m.s) if (int rc = m.launched(psk_gemvk(m.c->stream, m.n_cu, s, m.s->act, K), "Q5_K / Q6_K mat-vec")) return rc;
                i += run - 1;
                continue;
            }
            if (g.rope) return m.fail("Q5_K / Q6_K mat-vec: RoPE epilogue not covered");
            quantize_once();
            s.n_w = 1; s.pro = 0; s.pro_x = nullptr;
            if (int rc = k_quant(m, s)) return rc;
        } else {
            // a run of matrices of one lane-major type goes out as ONE launch (Q4_K_M: Q and K next to a Q6_K V)
            int run = 1;
            while (!g.silu_pair && i + run < g.n_w && g.w[i + run]->dtype == wt) run++;
            for (int j = 1; j < run; j++) { s.w[j] = g.w[i + j]; s.out[j] = g.out[i + j]; s.bias[j] = g.bias[i + j]; s.ldo[j] = g.ldo[i + j]; }
            s.n_w = run;
            bool q8k = false;
            if (int rc = lane_major(m, s, &q8k)) return rc;
            i += run - 1;
            quantized = q8k;
        }
    }
    return finish();
}

int matmul(const Mm &m, const psk_gemv_args &g) {
    bool any16 = false, all16 = true, one_type = true;
    for (int i = 0; i < g.n_w; i++) {
        any16 = any16 || g.w[i]->dtype == PS_F16;
        all16 = all16 && g.w[i]->dtype == PS_F16;
        one_type = one_type && g.w[i]->dtype == g.w[0]->dtype;
    }
    // F16 group: ONE launch for all matrices, the activation (with its RMSNorm) rounded to fp16 in its prologue (one column) or once before it
    if (all16) return f16(m, g);
    const int wt = g.w[0]->dtype;
    const bool k_quants = wt == PS_Q6_K || wt == PS_Q5_K;
    // single token: the launch with its fused prologue / epilogue (k_gemvk.hip)
    if (k_quants && psk_gemvk_takes(g, m.K, m.bs))
        return m.s ? m.launched(psk_gemvk(m.c->stream, m.n_cu, g, m.s->act, m.K), "Q5_K / Q6_K mat-vec") : 0;
    if (any16 || k_quants || !one_type) return each(m, g);
    bool q8k = false;
    return lane_major(m, g, &q8k);
}

} // namespace

int psk_matmul(ps_hip_ctx *c, const psk_gemv_args &g, const psk_mm_scratch &s, int64_t K, int64_t bs) {
    return matmul(Mm{c, &s, c->n_cu, K, bs}, g);
}

bool psk_matmul_fuses_rope(const ps_hip_ctx *c, const psk_gemv_args &g, int64_t K, int64_t bs) {
    if (!g.rope) return false;
    // every launch of the chain takes its part of the rotation: a rung without the epilogue is "not covered", so the plan fails
    return matmul(Mm{nullptr, nullptr, c->n_cu, K, bs}, g) == 0;
}
