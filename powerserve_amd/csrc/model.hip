// Whole-model fast path: what HIPBackend::plan() lowers the reference's per-layer op sequence to
// (LlamaModel::forward, src/model/llama/llama_model.cpp:52-117; NormAttention::build,
// src/model/module/norm_attention.cpp:26-160; FFN::build, src/model/module/ffn.cpp:22-42).
//
// Launch plan per layer (single token, Q4_K, the headline's shape):
//   [matvec[Wq|Wk|Wv] + RMSNorm + quantizer + RoPE + KV append + attention]  (k_qkvattn.hip; elsewhere the mat-vec, then attn_decode2 or scores + soft-max.V.p)
//   -> matvec[Wo] + quantizer + residual -> matvec[Wgate|Wup] + RMSNorm + quantizer + SiLU*up -> matvec[Wdown] + quantizer + residual
// Batches: quantize_act(rmsnorm) -> mat-mul[Wq|Wk|Wv] -> rope_append -> attn_scores -> soft-max -> V.p (+ quantize) -> mat-mul[Wo] + residual
//   -> quantize_act(rmsnorm) -> mat-mul[Wgate|Wup] SiLU*up -> quantize_act -> mat-mul[Wdown] + residual
// A persistent arena replaces the reference's malloc-per-intermediate (src/executor/executor.cpp:23-45);
// the single-token step is captured once into a hipGraph and replayed (all position-dependent values are
// read from a device-resident ps_step_state).
#include "ps_internal.h"
#include <algorithm>
#include "ps_ops.h"
#include "ps_kv_state.h"

#include <cstdio>
#include <cstring>


namespace {
__global__ void set_state_kernel(ps_step_state *s, int pos0, int bs, int n_out) {
    s->pos0 = pos0; s->bs = bs; s->n_out = n_out;
}
// prefill in super-chunks: one state per reference-sized chunk of the forward (the attention of chunk k sees n_kv = its own end)
__global__ void set_sub_states_kernel(ps_step_state *s, int pos0, int chunk, int n) {
    const int k = threadIdx.x;
    if (k * chunk < n) { s[k].pos0 = pos0 + k * chunk; s[k].bs = min(chunk, n - k * chunk); s[k].n_out = 0; }
}
__global__ void null_kernel(int *p) { if (p && threadIdx.x == 12345) *p = 0; }
__global__ void kv_move_kernel(float *k, float *v, _Float16 *k16, _Float16 *v16, int kvd, int n_ctx, int dst, int src) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= kvd) return;
    k[(int64_t)dst * kvd + d]   = k[(int64_t)src * kvd + d];
    v[(int64_t)d * n_ctx + dst] = v[(int64_t)d * n_ctx + src];
    if (k16) { k16[(int64_t)dst * kvd + d] = k16[(int64_t)src * kvd + d]; v16[(int64_t)dst * kvd + d] = v16[(int64_t)src * kvd + d]; }
}
} // namespace

// a captured single-token step and the KV position it was given as its prefetch hint (n_kv_lo)
struct step_graph {
    hipGraphExec_t exec = nullptr;
    size_t hint = 0;
};
enum { G_GREEDY, G_SAMPLED, G_FWD1, G_FWD1_LM, G_COUNT }; // ps_hip_model::graphs: decode_greedy's, decode_sampled's, the lowered forward's without / with lm_head

struct ps_hip_model {
    ps_hip_ctx *ctx = nullptr;
    ps_llm_config cfg{};
    bool qwen2 = false;
    int max_batch = 1;
    bool long_window = false; // ps_hip_model_create_long: score / probability rows in device memory (k_attn_long.hip), fixed at creation
    const ps_weight *token_embd = nullptr, *output = nullptr;
    const float *output_norm = nullptr;
    std::vector<const float *> attn_norm, ffn_norm, bq, bk, bv;
    std::vector<const ps_weight *> wq, wk, wv, wo, wg, wu, wd;
    // arena
    float *x = nullptr, *q = nullptr, *k = nullptr, *v = nullptr, *att = nullptr, *hb = nullptr, *g1 = nullptr, *u1 = nullptr;
    unsigned *attn_sync = nullptr; // [2048] words: [31] the one-launch attention's rendezvous-timeout flag
    unsigned *attn_flag_host = nullptr; // pinned: [31] travels here behind every single-token forward (async copy on the stream)
    bool attn_unchecked = false;        // such a forward was enqueued and its flag has not been looked at yet
    // pinned staging of the lowered single-token path (Model::decode over the op API: one stream synchronisation per token instead of three)
    int32_t *pin_tokens = nullptr;      // [max_batch] the token behind an async upload; pin_busy: not yet known to have been read
    int32_t *pin_argmax = nullptr;      // [max_batch] arg-max ids copied behind a lowered forward; valid for pin_argmax_n columns once pin_argmax_pending is clear
    bool pin_busy = false, pin_argmax_pending = false;
    int pin_argmax_n = 0;
    bool attn1_disabled = false;        // the one-launch attention timed out once on this device: mode bit 4 is sticky (set_mode ORs it back in; bit 6 re-arms)
    float *attn_xchg = nullptr;    // attn_decode2: scores in flight between workgroups (k_attn.hip)
    unsigned *attn_tick = nullptr; // attn_decode2: [64 * kv head] arrival counters
    unsigned long long *attn_gran = nullptr; // the fused Q / K / V + attention launch: rendezvous A's granules (k_qkvattn.hip)
    float *scores = nullptr, *logits = nullptr, *rope_table = nullptr;
    void *act_mem = nullptr;
    std::vector<_Float16 *> k16, v16; // fp16 mirrors, both [n_ctx][kv_dim]: allocated when mode bit 3 is first set
    float *attn_part = nullptr;       // split-KV partials of the fp16 decode attention
    ps_step_state *state = nullptr;
    int32_t *tokens_dev = nullptr, *argmax_dev = nullptr, *ids_dev = nullptr;
    float *am_v = nullptr;
    int *am_i = nullptr;
    uint8_t *tree_dev = nullptr;
    int32_t *rope_pos_dev = nullptr; // [max_batch] RoPE positions of a tree forward
    int mode = 0;
    psf16 *pf = nullptr;                // fp16 prefill perf mode (mode bit 5): fp16 copies of the layer matrices, fp16 activation scratch
    std::vector<_Float16 *> hq, hk, hv, ho, hg, hu, hd;
    _Float16 *xh = nullptr;
    _Float16 *h16 = nullptr;            // [max_batch][max(dim, hidden)] fp16-rounded activation columns of the F16 mat-muls (k_gemvh.hip); only with F16 weights
    ps_step_state *state_sub = nullptr; // [64] per-chunk states of a super-chunk prefill (ps_hip_model_prefill)
    step_graph graphs[G_COUNT];            // the captured single-token steps (dropped together: drop_graphs)
    ps_sample_dev *sample_dev = nullptr;   // sampler configuration + engine state of the current sampled run (allocated at first use)
    void *sample_scratch = nullptr;
    ps_sample_dev *sample_devs = nullptr;  // [min(16, max_batch)] one per column of a sampled batched run (ps_hip_model_decode_batch_sampled; allocated at first use),
    void *sample_rows_scratch = nullptr;   // and as many scratches of psl_sample_scratch_bytes
    void *score_scratch = nullptr;         // scoring (ps_hip_model_score; allocated at first use): k_score.hip's scratch for max_batch rows,
    int32_t *score_targets = nullptr;      // [max_batch] the targets of the forward's columns,
    ps_score *score_out = nullptr;         // [max_batch] their records
    uint64_t weight_bytes = 0;
    std::vector<void *> owned;
    // ---- sequences (ps_hip_model_seq_*): the KV state lives here and nowhere else.  Sequence 0 is the cache model_create allocated; the single-sequence
    // entry points work on cur().
    struct seq_state {
        std::vector<float *> k_cache, v_cache;
        uint8_t *kv_vis_dev = nullptr;   // [n_ctx] 1 = visible (KVCacheInterface::mask / unmask)
        std::vector<uint8_t> kv_vis_host;
        size_t n_hidden = 0, position = 0;
    };
    std::vector<seq_state> seqs; // every sequence, from model_create on
    int cur_seq = 0;
    seq_state &cur() { return seqs[cur_seq]; }
    const seq_state &cur() const { return seqs[cur_seq]; }
    float **seq_kv_dev = nullptr;      // [n_seq][n_layers][2] cache bases (psl_seqs_args::kv); the three device tables are allocated by the first batched entry point
    ps_seq_table *seq_tab = nullptr;   // the batched step's device table
    int32_t *seq_ids_dev = nullptr;    // [n_ctx][PS_SEQ_COLS_MAX] ids of a greedy batched run
};

// PS_HIP_MODE_OR: mode bits OR-ed into every model's mode (A/B runs of unmodified drivers, e.g. bench.py with 16 = two-launch attention)
static int mode_env_or() {
    static const int v = [] { const char *e = getenv("PS_HIP_MODE_OR"); return e ? atoi(e) : 0; }();
    return v;
}
static void graph_drop(step_graph &g) {
    if (g.exec) { (void)hipGraphExecDestroy(g.exec); g.exec = nullptr; }
}
static void drop_graphs(ps_hip_model *m) { // every captured launch plan (they bake the mode, the prefetch hint and the visibility pointers in)
    for (auto &g : m->graphs) graph_drop(g);
}
// the captured step carries the position it was captured at as a prefetch hint (n_kv_lo): keep it a LOWER bound that
// is not far behind (a stale hint costs time, never results)
static void graph_drop_if_stale(step_graph &g, size_t pos) {
    if (pos < g.hint || pos >= g.hint + 1024) graph_drop(g);
}
// long-window models: the score grid of a step captured at `hint` covers the slots it can meet before graph_drop_if_stale drops it (n_kv <= hint + 1024), not
// n_ctx -- 32 768 mostly empty workgroups per layer at 131 072 slots
static size_t graph_window_end(const ps_hip_model *m, size_t hint) { return std::min<size_t>(hint + 1024, m->cfg.seq_len); }
// capture what `enqueue` puts on the stream into g (nothing executes), with `pos` as its hint.  False: g is empty, and c->err says why
template <class F> static bool graph_capture(ps_hip_model *m, step_graph &g, size_t pos, F &&enqueue) {
    ps_hip_ctx *c = m->ctx;
    hipGraph_t gr = nullptr;
    int rc = 0;
    hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
        rc = enqueue();
        e = hipStreamEndCapture(c->stream, &gr);
    }
    if (!rc && e == hipSuccess) e = hipGraphInstantiate(&g.exec, gr, nullptr, nullptr, 0);
    if (gr) (void)hipGraphDestroy(gr);
    if (!rc && e != hipSuccess) c->err = hipGetErrorString(e);
    if (rc || e != hipSuccess) { g.exec = nullptr; return false; }
    g.hint = pos;
    return true;
}
static int dmalloc(ps_hip_model *m, void **p, size_t bytes) {
    ps_hip_ctx *c = m->ctx;
    PS_CHECK(c, ps_dev_malloc(p, bytes ? bytes : 16));
    m->owned.push_back(*p);
    return 0;
}

// a quantized / F16 mat-mul of the model (matmul.hip); `act` is carved for this K
static int mm(ps_hip_model *m, const psk_gemv_args &g, ps_act act, int64_t K, int64_t bs) {
    return psk_matmul(m->ctx, g, psk_mm_scratch{act, m->h16, {m->g1, m->u1}}, K, bs);
}

// fp16 prefill perf mode: the first use dequantizes every layer matrix into an fp16 copy (rows through get_rows, the logits buffer as
// fp32 scratch); the GEMMs are perf16.hip's own kernel
static int ensure_perf16(ps_hip_model *m) {
    if (m->pf) return 0;
    ps_hip_ctx *c = m->ctx;
    const ps_llm_config &f = m->cfg;
    const int64_t dim = f.dim, hid = f.hidden_dim;
    if (dim % 4 || hid % 4) PS_FAIL(c, "fp16 perf mode: dim and hidden_dim must be multiples of 4");
    // the mode's own GEMM (csrc/perf16.hip) takes row lengths and row counts that are multiples of 64: refused HERE, before +2 bytes per weight are allocated
    if (dim % 64 || hid % 64 || f.kv_dim % 64) PS_FAIL(c, "fp16 perf mode: dim, hidden_dim and kv_dim must be multiples of 64 (csrc/perf16.hip's GEMM tiles)");
    psf16 *pf = nullptr;
    if (int rc = psf16_create(c, &pf)) return rc;
    const int64_t kmax = dim > hid ? dim : hid;
    int cap = (int)((int64_t)m->max_batch * f.vocab_size / kmax);
    if (cap > m->max_batch) cap = m->max_batch;
    if (cap < 1) { psf16_destroy(pf); PS_FAIL(c, "fp16 perf mode: no scratch for the dequantizer"); }
    auto copy = [&](const ps_weight *w, std::vector<_Float16 *> &dst) -> int {
        if (w->dtype == PS_F16) { dst.push_back((_Float16 *)w->qs); return 0; } // already the [N][K] fp16 matrix: no second copy
        _Float16 *h = nullptr;
        if (dmalloc(m, (void **)&h, (size_t)w->N * w->K * 2)) return 2;
        dst.push_back(h);
        return psf16_dequantize(c, w, m->logits, m->tokens_dev, cap, h);
    };
    // a failed attempt leaves nothing behind: the fp16 copies made so far are freed (and taken off the model's list of owned allocations), so a retry does
    // not allocate them a second time
    auto fail = [&]() {
        for (auto *v : {&m->hq, &m->hk, &m->hv, &m->ho, &m->hg, &m->hu, &m->hd}) {
            for (_Float16 *h : *v) {
                auto it = std::find(m->owned.begin(), m->owned.end(), (void *)h);
                if (it == m->owned.end()) continue; // an F16 weight's own matrix
                m->owned.erase(it);
                (void)ps_dev_free(h);
            }
            v->clear();
        }
        psf16_destroy(pf);
        return 2;
    };
    for (auto *v : {&m->hq, &m->hk, &m->hv, &m->ho, &m->hg, &m->hu, &m->hd}) v->clear();
    for (uint32_t L = 0; L < f.n_layers; L++)
        if (copy(m->wq[L], m->hq) || copy(m->wk[L], m->hk) || copy(m->wv[L], m->hv) || copy(m->wo[L], m->ho) || copy(m->wg[L], m->hg) ||
            copy(m->wu[L], m->hu) || copy(m->wd[L], m->hd)) return fail();
    if (!m->xh && dmalloc(m, (void **)&m->xh, (size_t)m->max_batch * kmax * 2)) return fail();
    PS_CHECK(c, hipStreamSynchronize(c->stream));
    m->pf = pf;
    return 0;
}

// The mat-mul argument groups of a forward, built HERE and nowhere else: a layer's [Wq|Wk|Wv] (bias, RMSNorm prologue), Wo, the [Wgate|Wup] SiLU pair, Wdown,
// and the lm_head (L unused).  What a caller decides per launch (the RoPE epilogue, whether `down` quantizes in its prologue) it sets on the result.
enum mm_group { MM_QKV, MM_O, MM_GATE_UP, MM_DOWN, MM_LM_HEAD };
static psk_gemv_args mm_args(const ps_hip_model *m, mm_group which, uint32_t L) {
    const ps_llm_config &f = m->cfg;
    const int64_t dim = f.dim, kvd = f.kv_dim, hid = f.hidden_dim;
    psk_gemv_args g{};
    switch (which) {
    case MM_QKV:
        g.n_w = 3;
        g.w[0] = m->wq[L]; g.w[1] = m->wk[L]; g.w[2] = m->wv[L];
        g.out[0] = m->q; g.out[1] = m->k; g.out[2] = m->v;
        g.ldo[0] = dim; g.ldo[1] = kvd; g.ldo[2] = kvd;
        if (m->qwen2) { g.bias[0] = m->bq[L]; g.bias[1] = m->bk[L]; g.bias[2] = m->bv[L]; }
        g.pro = 1; g.pro_x = m->x; g.pro_norm_w = m->attn_norm[L]; g.pro_eps = f.norm_eps; // RMSNorm + quantize in the prologue
        break;
    case MM_O:
        g.n_w = 1; g.w[0] = m->wo[L]; g.out[0] = m->x; g.ldo[0] = dim; g.residual = m->x;
        g.pro = 2; g.pro_x = m->att;
        break;
    case MM_GATE_UP:
        g.n_w = 2; g.w[0] = m->wg[L]; g.w[1] = m->wu[L]; g.out[0] = m->hb; g.out[1] = m->hb; g.ldo[0] = hid; g.ldo[1] = hid;
        g.silu_pair = 1;
        g.pro = 1; g.pro_x = m->x; g.pro_norm_w = m->ffn_norm[L]; g.pro_eps = f.norm_eps;
        break;
    case MM_DOWN: // (pro 0: the activation is quantized by the caller, or it selects the prologue)
        g.n_w = 1; g.w[0] = m->wd[L]; g.out[0] = m->x; g.ldo[0] = dim; g.residual = m->x;
        break;
    case MM_LM_HEAD:
        g.n_w = 1; g.w[0] = m->output ? m->output : m->token_embd; // tied lm_head (weights.hpp:67-68)
        g.out[0] = m->logits; g.ldo[0] = f.vocab_size;
        g.pro = 1; g.pro_x = m->x; g.pro_norm_w = m->output_norm; g.pro_eps = f.norm_eps;
        break;
    }
    return g;
}

int g_kv_stream_force = -1; // ps_hip_debug_set(9, v)
// What one forward consists of: everything enqueue_forward is told, by name (nothing is set on the model before a call and cleared after it)
struct fwd_opts {
    bool lm_head = false;  // final norm + lm_head + arg-max (or the sampler chain)
    bool tree = false;     // tree_dev is the attention's mask
    bool rope_pos = false; // RoPE positions from rope_pos_dev (a tree forward)
    bool advance = false;  // with lm_head: the step feeds its own id back and moves the device-side state on (the decode loops)
    bool sampled = false;  // with lm_head: the sampler chain (sample_dev; with sq: column i's own, sample_devs[i]) in place of the arg-max
    bool score = false;    // with lm_head: every column scored against score_targets (k_score.hip) in place of the arg-max
    // sq: a batched decode step -- column i is a token of ITS OWN sequence (sq->tab); the mat-muls are the column-wise ones of any batch, RoPE + KV append and the
    // attention go per column to that sequence's cache (k_attn.hip, "batched decode")
    const psl_seqs_args *sq = nullptr;
    int n_kv_host = 0;     // pos0 + bs of a forward that is enqueued eagerly (0 while a graph is captured / replayed)
    int n_kv_grid = 0;     // long-window models, with n_kv_host == 0 (a captured or device-positioned single-token step): an upper bound of n_kv that sizes the score grid
    int n_kv_hint = 0;     // capture of a single-token forward: the lower bound of n_kv its prefetch hint is baked with
    int attn_chunk = 0;    // > 0: a super-chunk (ps_hip_model_prefill), the attention runs chunk by chunk
};
// enqueue one forward over `bs` tokens whose ids are in tokens_dev and whose state is in m->state
static int enqueue_forward(ps_hip_model *m, int bs, const fwd_opts &o) {
    ps_hip_ctx *c = m->ctx;
    hipStream_t st = c->stream;
    const ps_llm_config &f = m->cfg;
    const ps_hip_model::seq_state &kv = m->cur();
    const bool lm_head = o.lm_head, use_tree = o.tree, use_rope_pos = o.rope_pos;
    const psl_seqs_args *sq = o.sq;
    const int64_t dim = f.dim, kvd = f.kv_dim, hid = f.hidden_dim;
    // activation rows are laid out with the row strides of the *current* K, so carve per use:
    auto act_for = [&](int64_t K) { return ps_act_carve(m->act_mem, K, m->max_batch); };

    psl_get_rows(st, m->token_embd, m->tokens_dev, bs, m->x);
    psl_attn_args aa{};
    aa.n_heads = (int)f.n_heads; aa.n_kv_heads = (int)f.n_kv_heads; aa.head_size = (int)f.head_size; aa.n_ctx = (int)f.seq_len;
    aa.neox = (f.rope.mode & 2) ? 1 : 0; aa.n_dims = f.rope.n_dims; aa.state = m->state; aa.rope_table = m->rope_table;
    aa.q = m->q; aa.k = m->k; aa.v = m->v; aa.scores = m->scores; aa.att = m->att;
    aa.tree = use_tree ? m->tree_dev : nullptr;
    aa.rope_pos = use_rope_pos ? m->rope_pos_dev : nullptr;
    aa.kv_vis = kv.n_hidden ? kv.kv_vis_dev : nullptr;
    aa.scale = 1.0f / sqrtf((float)f.head_size);
    aa.n_kv_host = o.n_kv_host > 0 ? o.n_kv_host : o.n_kv_grid; // (without bs_host it only sizes the score grid)
    aa.bs_host = o.n_kv_host > 0 ? bs : 0;
    aa.sync = m->attn_sync;
    // fp16 perf mode (NOT bit-exact, mode bit 5): the layer mat-muls of a prefill batch as dense fp16 GEMMs (perf16.hip); single tokens,
    // tree forwards and anything that produces logits stay on the parity kernels
    const bool f16 = (m->mode & 32) && bs >= 2 && !lm_head && !use_tree && !use_rope_pos && !sq;
    if (f16) if (int rc = ensure_perf16(m)) return rc;
    const bool lw = m->long_window; // scores, then the long soft-max and V.p, whatever the forward (k_attn_long.hip); the one-launch forms hold LDS rows
    const bool one_launch = (m->mode & 16) == 0 && !lw; // default; mode bit 4 switches attn_decode2 off (two launches)
    auto softmax_pv = [&](const psl_attn_args &as, int nb) { if (lw) psl_attn_long_softmax_pv(st, as, nb); else psl_attn_softmax_pv(st, as, nb); };
    aa.xchg = m->attn_xchg; aa.tick = m->attn_tick; aa.gran = m->attn_gran;
    // Single-token attention: are the cached K rows / V channels read with non-temporal loads (psl_attn_args::kv_stream)?  Measured (profiles/r06_kv_stream_threshold.txt,
    // r06_ad2_nt_small_models.txt): the fused Q / K / V + attention launch is faster with them at every cache length tried (8B: +1.0 % behind a 256-token prompt, +1.6 % behind
    // 1024, +2.2 % behind 2048); the attention launch of its own (attn_decode2) gains where the whole cache -- every layer, K and V -- is more than the memory-side cache keeps
    // from token to token (8B behind 2048 tokens, 537 MB: +0.8 %) and loses where it fits (Llama-3.2-1B behind 512 tokens, 42 MB: -2.2 %).  ps_hip_debug_set(9, 0 / 1) forces both (A/B).
    const int kvs_force = g_kv_stream_force; // (ps_hip_debug_set(9, v): -1 by the rule below, 0 / 1 forced)
    const int n_kv_now = o.n_kv_host > 0 ? o.n_kv_host : (o.n_kv_hint > 0 ? o.n_kv_hint : (int)kv.position);
    const int kvs_fused = kvs_force >= 0 ? kvs_force : 1;
    const int kvs_own = kvs_force >= 0 ? kvs_force : ((int64_t)f.n_layers * 2 * n_kv_now * kvd * 4 > ((int64_t)160 << 20) ? 1 : 0);
    aa.kv_stream = kvs_own;
    aa.n_kv_lo = n_kv_now; // (a hint: rows below it are requested before the device-side position has arrived)

    for (uint32_t L = 0; L < f.n_layers; L++) {
        ps_act a1 = act_for(dim);
        psk_gemv_args g = mm_args(m, MM_QKV, L);
        aa.k_cache = kv.k_cache[L]; aa.v_cache = kv.v_cache[L];
        const bool kv16 = (m->mode & 8) && !m->k16.empty();
        aa.k16 = kv16 ? m->k16[L] : nullptr; aa.v16 = kv16 ? m->v16[L] : nullptr; aa.part = m->attn_part;
        // adjacent-pair RoPE: rotation and the KV append ride in the epilogue of the Q / K / V launch(es) wherever the dispatcher's
        // choice has it -- single tokens (mixed types -- Q4_K_M's Q6_K V next to Q4_K Q and K -- and pure Q6_K: one launch per run of a
        // type, each with its part of the epilogue, psk_gemv_args::rope_wi0) and Q4_K batches (the chunk mat-mul, k_gemm4k.hip)
        psk_rope_kv rk{m->state, m->rope_table, aa.k_cache, aa.v_cache, (int)f.head_size, (int)f.rope.n_dims, (int)f.seq_len, (int)kvd, aa.rope_pos, aa.k16, aa.v16};
        g.rope = &rk;
        if (f16 || aa.neox || sq || !psk_matmul_fuses_rope(c, g, dim, bs)) g.rope = nullptr;
        psl_seqs_args sl{};
        if (sq) { sl = *sq; sl.layer = (int)L; }
        bool fused_qa = false;
        if (f16) {
            psf16_rmsnorm_to_h(st, m->x, m->attn_norm[L], f.norm_eps, dim, bs, m->xh);
            {
                const _Float16 *W3[3] = {m->hq[L], m->hk[L], m->hv[L]};
                float *o3[3] = {m->q, m->k, m->v};
                const int64_t n3[3] = {dim, kvd, kvd};
                if (psf16_gemm_n(c, m->pf, 3, W3, n3, dim, m->xh, bs, o3, n3, 0.f)) return 2; // Q, K, V: one launch
            }
            if (m->qwen2) { psf16_add_bias(st, m->q, m->bq[L], dim, bs); psf16_add_bias(st, m->k, m->bk[L], kvd, bs); psf16_add_bias(st, m->v, m->bv[L], kvd, bs); }
        } else if (bs == 1 && !use_tree && one_launch && !kv16 && g.rope && (m->mode & 128) == 0 && // (one_launch: never in a long-window model)
                   (aa.dbg = psk_gemv_dbg_buf(10, 3), aa.kv_stream = kvs_fused, psk_qkv_attn(st, c->n_cu, g, dim, aa))) { // timeline key 43
            // the head of the layer in ONE launch: Q / K / V mat-vec + RoPE + KV append + single-token attention (k_qkvattn.hip); mode bit 7 brings the two launches back
            aa.dbg = nullptr; aa.kv_stream = kvs_own;
            fused_qa = true;
        } else if (mm(m, g, a1, dim, bs)) return 2;

        aa.kv_stream = kvs_own; aa.dbg = nullptr; // (also when the fused launch declined the shape)
        if (sq) psl_rope_append_seqs(st, aa, sl, bs);
        else if (!g.rope) psl_rope_append(st, aa, bs);
        bool att_quantized = false;
        if (sq) {
            psl_attn_seqs(st, aa, sl, bs);
        } else if (fused_qa) {
        } else if (bs == 1 && !use_tree && kv16 && psl_attn_decode_f16(st, aa)) {
            // fp16-KV decode mode (not bit-exact): split-KV online soft-max over the fp16 mirrors
        } else if (bs == 1 && !use_tree && one_launch && (aa.dbg = psk_gemv_dbg_buf(10, 2), psl_attn_decode2(st, c->n_cu, aa))) { // timeline key 42
            aa.dbg = nullptr;
        } else if (o.attn_chunk > 0 && bs > o.attn_chunk) {
            // a super-chunk of several reference-sized chunks (ps_hip_model_prefill): the mat-muls above and below take all bs columns
            // at once (they are column-wise: chunking cannot change their bits), the attention runs chunk by chunk with the n_kv the
            // reference's chunk would have seen -- its soft-max and V.p sums depend on where a chunk ends
            for (int c0 = 0, k = 0; c0 < bs; c0 += o.attn_chunk, k++) {
                const int nb = bs - c0 < o.attn_chunk ? bs - c0 : o.attn_chunk;
                psl_attn_args as = aa;
                as.state = m->state_sub + k;
                as.q = m->q + (int64_t)c0 * dim; as.att = m->att + (int64_t)c0 * dim;
                as.n_kv_host = o.n_kv_host > 0 ? o.n_kv_host - (bs - c0 - nb) : 0;
                as.bs_host = as.n_kv_host > 0 ? nb : 0;
                as.qact = ps_act{}; as.dbg = nullptr;
                psl_attn_scores(st, as, nb);
                softmax_pv(as, nb);
            }
        } else {
            aa.dbg = bs == 1 ? psk_gemv_dbg_buf(10, 0) : nullptr; // timeline key 40
            psl_attn_scores(st, aa, bs);
            aa.dbg = bs == 1 ? psk_gemv_dbg_buf(10, 1) : nullptr; // timeline key 41
            // batches: the V.p kernel can leave `att` quantized for the O projection (one launch less per layer) when the O weight
            // takes Q8_K activations through the batched path
            aa.qact = ps_act{}; aa.qact_K = dim;
            if (!f16 && bs >= 2 && ps_hip_vec_dot_type(m->wo[L]->dtype) == PS_Q8_K && dim % 256 == 0) {
                aa.qact = a1;
                if (!psk_gemm4k_frag(dim, bs)) { aa.qact.qf = nullptr; aa.qact.mf = nullptr; } // (as psk_quantize_act decides)
                if (!psl_attn_pv_quantizes(aa, bs)) aa.qact = ps_act{};
            }
            att_quantized = aa.qact.qs != nullptr;
            softmax_pv(aa, bs);
            aa.qact = ps_act{};
            aa.dbg = nullptr;
        }

        psk_gemv_args go = mm_args(m, MM_O, L);
        if (att_quantized) { go.pro = 0; go.pro_x = nullptr; } // (the V.p kernel left `att` quantized in a1)
        ps_act a2 = act_for(hid);
        const int vdt_d = ps_hip_vec_dot_type(m->wd[L]->dtype);
        const psk_gemv_args gf = mm_args(m, MM_GATE_UP, L);
        psk_gemv_args gd = mm_args(m, MM_DOWN, L);
        if (f16) { // x += O att;  x += down(silu(gate x') * up x'),  x' = rmsnorm(x): residuals through beta = 1
            psf16_to_h(st, m->att, (int64_t)bs * dim, m->xh);
            if (psf16_gemm(c, m->pf, m->ho[L], dim, dim, m->xh, bs, m->x, dim, 1.f)) return 2;
            psf16_rmsnorm_to_h(st, m->x, m->ffn_norm[L], f.norm_eps, dim, bs, m->xh);
            {
                const _Float16 *W2[2] = {m->hg[L], m->hu[L]};
                float *o2[2] = {m->g1, m->u1};
                const int64_t n2[2] = {hid, hid};
                if (psf16_gemm_n(c, m->pf, 2, W2, n2, dim, m->xh, bs, o2, n2, 0.f)) return 2; // gate, up: one launch
            }
            psf16_silu_mul_to_h(st, m->g1, m->u1, (int64_t)bs * hid, m->xh);
            if (psf16_gemm(c, m->pf, m->hd[L], dim, hid, m->xh, bs, m->x, dim, 1.f)) return 2;
            continue;
        }
        if (mm(m, go, a1, dim, bs)) return 2;
        if (mm(m, gf, a1, dim, bs)) return 2;
        if (m->wd[L]->dtype == PS_F16 || (psk_gemv_lds_col_bytes(m->wd[L]->dtype, hid) * (bs == 1 ? 1 : 4) <= 64 * 1024 && (hid <= 8192 || bs == 1))) {
            gd.pro = 2; gd.pro_x = m->hb; // short rows: quantize in the prologue
        } else {
            psk_quantize_act(st, vdt_d, 0, m->hb, nullptr, nullptr, 0.f, hid, bs, a2);
        }
        if (mm(m, gd, a2, hid, bs)) return 2;
    }
    if (lm_head) {
        if (mm(m, mm_args(m, MM_LM_HEAD, 0), act_for(dim), dim, bs)) return 2;
        const bool advance = o.advance;
        if (o.score) psl_score(st, m->logits, (int)f.vocab_size, (int64_t)f.vocab_size, bs, m->score_targets, m->score_scratch, m->score_out);
        else if (sq && o.sampled) { // column i draws from its own chain; the drawn ids take the arg-max's place in the batched step's bookkeeping
            psl_sample_rows(st, m->logits, (int)f.vocab_size, (int64_t)f.vocab_size, bs, m->sample_devs, m->sample_rows_scratch, m->argmax_dev);
            if (advance) psl_seqs_advance(st, m->seq_tab, m->argmax_dev, m->tokens_dev, m->seq_ids_dev, bs);
        } else if (o.sampled) psl_sample(st, m->logits, (int)f.vocab_size, m->sample_dev, m->sample_scratch, nullptr, advance ? m->state : nullptr, m->tokens_dev, m->ids_dev);
        else if (sq) {
            psl_argmax2(st, m->logits, f.vocab_size, bs, m->argmax_dev, m->am_v, m->am_i, nullptr, nullptr, nullptr);
            if (advance) psl_seqs_advance(st, m->seq_tab, m->argmax_dev, m->tokens_dev, m->seq_ids_dev, bs);
        } else psl_argmax2(st, m->logits, f.vocab_size, bs, m->argmax_dev, m->am_v, m->am_i, advance ? m->state : nullptr, m->tokens_dev, m->ids_dev);
    }
    PS_CHECK(c, hipGetLastError());
    return 0;
}

// Wait for the stream.  It is idle afterwards: everything enqueued before this point has run, so no upload from the pinned token word is queued any
// more and the arg-max ids copied behind a lowered forward have arrived.
static hipError_t sync_stream(ps_hip_model *m) {
    const hipError_t e = hipStreamSynchronize(m->ctx->stream);
    if (e == hipSuccess) { m->pin_busy = false; m->pin_argmax_pending = false; }
    return e;
}
static int check_tokens(ps_hip_model *m, const int32_t *tokens, int n, const char *who) {
    for (int i = 0; i < n; i++)
        if (tokens[i] < 0 || (uint32_t)tokens[i] >= m->cfg.vocab_size) PS_FAIL(m->ctx, std::string(who) + ": token id out of range");
    return 0;
}
// KVCache::advance_tokens unmasks the slots it walks over (core/kv_cache.hpp:249-255)
static void unmask_range(ps_hip_model *m, size_t from, size_t n) {
    ps_hip_model::seq_state &kv = m->cur();
    if (!kv.n_hidden) return;
    for (size_t i = from; i < from + n && i < m->cfg.seq_len; i++) {
        if (!kv.kv_vis_host[i]) {
            kv.kv_vis_host[i] = 1;
            kv.n_hidden--;
            (void)hipMemcpyAsync(kv.kv_vis_dev + i, &kv.kv_vis_host[i], 1, hipMemcpyHostToDevice, m->ctx->stream);
        }
    }
}
// The one-launch attentions wait for each other's workgroups inside the launch (bounded); a wait that gave up raises
// attn_sync[31].  Read it behind every synchronised single-token forward, clear it, and fall back to the two launches
// from here on (mode bit 4): the forward that timed out has no valid result.  Expects the stream to be idle.
// Every single-token forward that may have used the one-launch attention is followed, on the stream, by a 4-byte copy of the flag into pinned
// host memory (note_single_token): looking at it costs no round trip once the stream is idle.
int g_force_attn_timeout = 0; // ps_hip_debug_set(5, n): the next n single-token forwards on the one-launch attention report a time-out (tests of the retry paths)
static void note_single_token(ps_hip_model *m) {
    if (m->mode & 16) return; // the one-launch form is not in use
    if (g_force_attn_timeout > 0) { g_force_attn_timeout--; (void)hipMemsetAsync(m->attn_sync + 31, 1, 1, m->ctx->stream); } // (word = 1, behind the forward's launches)
    (void)hipMemcpyAsync(m->attn_flag_host, m->attn_sync + 31, 4, hipMemcpyDeviceToHost, m->ctx->stream);
    m->attn_unchecked = true;
}
// 0: nothing pending or the flag is clear.  PS_HIP_ATTN_TIMEOUT (3): the forward(s) since the last check have no valid result; the model has
// switched to the two-launch attention (mode bit 4, sticky; graphs dropped) and c->err says so -- the callers that still know their inputs run
// them again, ONCE (behind the switch no forward can time out: note_single_token arms nothing under mode bit 4).  1: a HIP error (c->err),
// never retried.  The switch happens before anything that can fail, so a failing memset cannot leave the one-launch form armed with its flag up.
static int check_attn_timeout(ps_hip_model *m, const char *who) {
    ps_hip_ctx *c = m->ctx;
    if (!m->attn_unchecked) return 0;
    m->attn_unchecked = false;
    if (!*(volatile unsigned *)m->attn_flag_host) return 0;
    *(volatile unsigned *)m->attn_flag_host = 0;
    m->mode |= 16;
    m->attn1_disabled = true;
    drop_graphs(m);
    PS_CHECK(c, hipMemset(m->attn_sync + 31, 0, 4));
    c->err = std::string(who) + ": the one-launch attention timed out at its score exchange (GPU shared or partitioned?); this forward has no valid "
             "result, the cache position is unchanged, and the model now uses the two-launch attention (mode bit 4)";
    return PS_HIP_ATTN_TIMEOUT;
}
// The retry of every entry point that still knows its inputs: `run` enqueues, waits and ends in check_attn_timeout.  A time-out: the model is on the
// two-launch attention now, the same work once more; any other code, and a second time-out, are the caller's.
template <class F> static int with_attn_retry(ps_hip_model *m, F &&run) {
    const int rc = run();
    if (rc != PS_HIP_ATTN_TIMEOUT) return rc;
    m->ctx->err.clear();
    return run();
}
// A lowered forward that nobody has consumed yet (no kv_advance / sync_check since) must not leave its flag to the next, unrelated forward:
// every entry point settles it first and hands a time-out back to the caller, who still owns that forward's inputs.
static int settle_pending(ps_hip_model *m) {
    if (!m->attn_unchecked) return 0;
    return ps_hip_model_sync_check(m);
}

extern "C" {

static int model_create(ps_hip_ctx *c, const ps_model_desc *d, ps_hip_model **out, const bool long_window) {
    *out = nullptr;
    const ps_llm_config &f = d->cfg;
    if (f.n_kv_heads == 0 || f.n_heads == 0 || f.n_layers == 0 || f.seq_len == 0) PS_FAIL(c, "model_create: zero-sized configuration");
    if (f.n_heads % f.n_kv_heads || f.head_size * f.n_heads != f.dim || f.head_size * f.n_kv_heads != f.kv_dim)
        PS_FAIL(c, "model_create: inconsistent head configuration");
    { // the descriptor is trusted by every kernel: weight handles must exist and agree with the configuration
        auto okw = [](const ps_weight *w, int64_t K, int64_t N) {
            return w && w->K == K && w->N == N && w->qs && (w->dtype == PS_Q4_0 || w->dtype == PS_Q8_0 || w->dtype == PS_Q4_K || w->dtype == PS_Q5_K || w->dtype == PS_Q6_K || w->dtype == PS_F16);
        };
        if (!d->token_embd || d->token_embd->K != f.dim || d->token_embd->N != f.vocab_size || !d->token_embd->qs) PS_FAIL(c, "model_create: token_embd missing or of the wrong shape");
        if (d->output && !okw(d->output, f.dim, f.vocab_size)) PS_FAIL(c, "model_create: output.weight of the wrong shape / type");
        if (!d->output && !okw(d->token_embd, f.dim, f.vocab_size)) PS_FAIL(c, "model_create: tied lm_head needs a quantized or F16 token_embd");
        if (!d->output_norm || !d->attn_norm || !d->ffn_norm || !d->attn_q || !d->attn_k || !d->attn_v || !d->attn_output || !d->ffn_gate || !d->ffn_up || !d->ffn_down)
            PS_FAIL(c, "model_create: null weight table");
        for (uint32_t i = 0; i < f.n_layers; i++) {
            if (!d->attn_norm[i] || !d->ffn_norm[i]) PS_FAIL(c, "model_create: null norm weights in layer " + std::to_string(i));
            if (!okw(d->attn_q[i], f.dim, f.dim) || !okw(d->attn_k[i], f.dim, f.kv_dim) || !okw(d->attn_v[i], f.dim, f.kv_dim) || !okw(d->attn_output[i], f.dim, f.dim) ||
                !okw(d->ffn_gate[i], f.dim, f.hidden_dim) || !okw(d->ffn_up[i], f.dim, f.hidden_dim) || !okw(d->ffn_down[i], f.hidden_dim, f.dim))
                PS_FAIL(c, "model_create: weight of layer " + std::to_string(i) + " missing or of the wrong shape / type (model.json and weights.gguf disagree?)");
            if (d->is_qwen2 && (!d->attn_q_bias || !d->attn_k_bias || !d->attn_v_bias || !d->attn_q_bias[i] || !d->attn_k_bias[i] || !d->attn_v_bias[i]))
                PS_FAIL(c, "model_create: qwen2 needs the attention biases");
        }
    }
    if (f.head_size % 32 || f.head_size > 128) PS_FAIL(c, "model_create: head_size must be 32, 64, 96 or 128");
    if (f.n_heads / f.n_kv_heads > 8) PS_FAIL(c, "model_create: GQA ratio > 8 not supported");
    if ((int)f.rope.n_dims != (int)f.head_size) PS_FAIL(c, "model_create: rope n_dims != head_size (reference asserts the same, norm_attention.cpp:38)");
    if (f.seq_len % 4) PS_FAIL(c, "model_create: n_ctx must be a multiple of 4");
    if (!long_window && (size_t)(f.n_heads / f.n_kv_heads) * f.seq_len * 4 + 44 * 1024 > 158 * 1024)
        PS_FAIL(c, "model_create: n_ctx too large for the LDS-resident softmax rows (cap n_ctx, or create a long-window model: ps_hip_model_create_long)");
    if (long_window && f.seq_len > PS_HIP_LONG_CTX_MAX) PS_FAIL(c, "model_create_long: n_ctx above PS_HIP_LONG_CTX_MAX");
    PS_CHECK(c, hipSetDevice(c->device));
    auto m = new ps_hip_model();
    m->ctx = c; m->cfg = f; m->qwen2 = d->is_qwen2 != 0; m->max_batch = d->max_batch > 0 ? d->max_batch : 1;
    m->long_window = long_window;
    m->mode = mode_env_or() & ~8; // (the fp16-KV mode allocates: only through set_mode)
    m->seqs.resize(1);
    ps_hip_model::seq_state &s0 = m->seqs[0];
    m->token_embd = d->token_embd; m->output = d->output; m->output_norm = d->output_norm;
    const uint32_t L = f.n_layers;
    auto cpf = [&](std::vector<const float *> &v, const float *const *src) { v.assign(L, nullptr); if (src) for (uint32_t i = 0; i < L; i++) v[i] = src[i]; };
    auto cpw = [&](std::vector<const ps_weight *> &v, const ps_weight *const *src) { v.assign(L, nullptr); for (uint32_t i = 0; i < L; i++) v[i] = src[i]; };
    cpf(m->attn_norm, d->attn_norm); cpf(m->ffn_norm, d->ffn_norm);
    cpf(m->bq, d->attn_q_bias); cpf(m->bk, d->attn_k_bias); cpf(m->bv, d->attn_v_bias);
    cpw(m->wq, d->attn_q); cpw(m->wk, d->attn_k); cpw(m->wv, d->attn_v); cpw(m->wo, d->attn_output);
    cpw(m->wg, d->ffn_gate); cpw(m->wu, d->ffn_up); cpw(m->wd, d->ffn_down);
    m->weight_bytes = (m->output ? m->output : m->token_embd)->gguf_bytes;
    for (uint32_t i = 0; i < L; i++)
        m->weight_bytes += m->wq[i]->gguf_bytes + m->wk[i]->gguf_bytes + m->wv[i]->gguf_bytes + m->wo[i]->gguf_bytes +
                           m->wg[i]->gguf_bytes + m->wu[i]->gguf_bytes + m->wd[i]->gguf_bytes;

    const size_t mb = (size_t)m->max_batch, dim = f.dim, kvd = f.kv_dim, hid = f.hidden_dim, nctx = f.seq_len;
    auto fail = [&]() { ps_hip_model_destroy(m); return 1; };
    if (dmalloc(m, (void **)&m->x, mb * dim * 4) || dmalloc(m, (void **)&m->q, mb * dim * 4) ||
        dmalloc(m, (void **)&m->k, mb * kvd * 4) || dmalloc(m, (void **)&m->v, mb * kvd * 4) ||
        dmalloc(m, (void **)&m->att, mb * dim * 4) || dmalloc(m, (void **)&m->hb, mb * hid * 4) ||
        dmalloc(m, (void **)&m->g1, mb * hid * 4) || dmalloc(m, (void **)&m->u1, mb * hid * 4) ||
        dmalloc(m, (void **)&m->attn_sync, 2048 * 4) ||
        dmalloc(m, (void **)&m->attn_xchg, long_window ? 0 : psl_attn_decode2_xchg_bytes((int)f.n_kv_heads, (int)nctx)) || dmalloc(m, (void **)&m->attn_tick, (size_t)f.n_kv_heads * 64 * 4) ||
        dmalloc(m, (void **)&m->attn_gran, (size_t)(f.n_heads + 2 * f.n_kv_heads) * f.head_size * 8) ||
        dmalloc(m, (void **)&m->scores, mb * f.n_heads * nctx * 4) || dmalloc(m, (void **)&m->logits, mb * f.vocab_size * 4) ||
        dmalloc(m, (void **)&m->rope_table, nctx * f.head_size * 4) ||
        dmalloc(m, &m->act_mem, ps_act_bytes(dim > hid ? dim : hid, mb)) ||
        dmalloc(m, (void **)&m->state, sizeof(ps_step_state)) || dmalloc(m, (void **)&m->state_sub, 64 * sizeof(ps_step_state)) || dmalloc(m, (void **)&m->tokens_dev, mb * 4) ||
        dmalloc(m, (void **)&m->argmax_dev, mb * 4) || dmalloc(m, (void **)&m->ids_dev, (nctx + 1) * 4) ||
        dmalloc(m, (void **)&m->tree_dev, mb * mb) || dmalloc(m, (void **)&m->rope_pos_dev, mb * 4) || dmalloc(m, (void **)&s0.kv_vis_dev, nctx) || dmalloc(m, (void **)&m->am_v, mb * 64 * 4) || dmalloc(m, (void **)&m->am_i, mb * 64 * 4))
        return fail();
    {
        bool any16 = (m->output ? m->output : m->token_embd)->dtype == PS_F16;
        for (uint32_t i = 0; i < L; i++)
            for (const ps_weight *w : {m->wq[i], m->wk[i], m->wv[i], m->wo[i], m->wg[i], m->wu[i], m->wd[i]}) any16 = any16 || w->dtype == PS_F16;
        if (any16 && dmalloc(m, (void **)&m->h16, mb * (dim > hid ? dim : hid) * 2)) return fail();
    }
    (void)hipMemsetAsync(m->attn_sync, 0, 2048 * 4, c->stream);
    if (hipHostMalloc((void **)&m->attn_flag_host, 64, hipHostMallocDefault) != hipSuccess) return fail();
    *m->attn_flag_host = 0;
    if (hipHostMalloc((void **)&m->pin_tokens, (2 * mb + 16) * 4, hipHostMallocDefault) != hipSuccess) return fail();
    m->pin_argmax = m->pin_tokens + mb;
    (void)hipMemsetAsync(m->attn_tick, 0, (size_t)f.n_kv_heads * 64 * 4, c->stream);
    (void)hipMemsetAsync(m->attn_gran, 0, (size_t)(f.n_heads + 2 * f.n_kv_heads) * f.head_size * 8, c->stream); // (tag 0: no launch's)
    (void)hipMemsetAsync(s0.kv_vis_dev, 1, nctx, c->stream);
    s0.kv_vis_host.assign(nctx, 1);
    s0.k_cache.assign(L, nullptr); s0.v_cache.assign(L, nullptr);
    for (uint32_t i = 0; i < L; i++) {
        if (dmalloc(m, (void **)&s0.k_cache[i], nctx * kvd * 4) || dmalloc(m, (void **)&s0.v_cache[i], nctx * kvd * 4)) return fail();
        (void)hipMemsetAsync(s0.k_cache[i], 0, nctx * kvd * 4, c->stream);
        (void)hipMemsetAsync(s0.v_cache[i], 0, nctx * kvd * 4, c->stream);
    }
    // RoPE table for every cache position, host-built with the reference recurrence
    std::vector<float> tab(nctx * f.head_size);
    ps_rope_table_host(&f.rope, f.head_size, nullptr, (int)nctx, tab.data());
    if (hipMemcpyAsync(m->rope_table, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail();
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail();
    *out = m;
    return 0;
}

int ps_hip_model_create(ps_hip_ctx *c, const ps_model_desc *d, ps_hip_model **out) { return model_create(c, d, out, false); }
int ps_hip_model_create_long(ps_hip_ctx *c, const ps_model_desc *d, ps_hip_model **out) { return model_create(c, d, out, true); }
int ps_hip_model_is_long(const ps_hip_model *m) { return m->long_window ? 1 : 0; }

void ps_hip_model_destroy(ps_hip_model *m) {
    if (!m) return;
    (void)hipStreamSynchronize(m->ctx->stream);
    drop_graphs(m);
    if (m->attn_flag_host) (void)hipHostFree(m->attn_flag_host);
    if (m->pin_tokens) (void)hipHostFree(m->pin_tokens);
    psf16_destroy(m->pf);
    for (void *p : m->owned) (void)ps_dev_free(p);
    delete m;
}

size_t ps_hip_model_kv_position(const ps_hip_model *m) { return m->cur().position; }
int ps_hip_model_max_batch(const ps_hip_model *m) { return m->max_batch; }
// slots at or behind the position are never consulted through the visibility table (the causal / tree mask governs them)
// and KVCache::advance_tokens / append un-hides what it walks over (core/kv_cache.hpp:249-255): a rollback or truncate
// leaves no hidden slot behind the new position, so a model that served as a speculative draft can decode again
int ps_hip_model_kv_truncate(ps_hip_model *m, size_t n) {
    if (int rc = settle_pending(m)) return rc; // (every KV entry point: an unconsumed lowered forward's time-out belongs to ITS caller, not to the next forward)
    size_t &position = m->cur().position;
    if (n < position) position = n;
    unmask_range(m, position, m->cfg.seq_len - position);
    return 0;
}
int ps_hip_model_kv_advance(ps_hip_model *m, size_t n) {
    if (int rc = ps_hip_model_sync_check(m)) return rc; // (an unsynchronised lowered forward: its rows must be valid before they count)
    size_t &position = m->cur().position;
    if (position + n > m->cfg.seq_len) { m->ctx->err = "kv_advance: KV cache is full (n_ctx)"; return 2; }
    unmask_range(m, position, n);
    position += n;
    return 0;
}
int ps_hip_model_kv_rollback(ps_hip_model *m, size_t n) {
    if (int rc = settle_pending(m)) return rc;
    size_t &position = m->cur().position;
    if (n > position) { m->ctx->err = "kv_rollback: more tokens than cached"; return 2; }
    position -= n;
    unmask_range(m, position, m->cfg.seq_len - position);
    return 0;
}
int ps_hip_model_kv_move(ps_hip_model *m, size_t dst, size_t src) {
    if (int rc = settle_pending(m)) return rc; // (rows of a forward whose result is invalid must not be copied)
    if (dst == src) return 0;
    if (dst >= m->cfg.seq_len || src >= m->cfg.seq_len) { m->ctx->err = "kv_move: index out of range"; return 2; }
    const ps_hip_model::seq_state &kv = m->cur();
    for (uint32_t L = 0; L < m->cfg.n_layers; L++)
        hipLaunchKernelGGL(kv_move_kernel, dim3((m->cfg.kv_dim + 255) / 256), dim3(256), 0, m->ctx->stream, kv.k_cache[L],
                           kv.v_cache[L], m->k16.empty() ? nullptr : m->k16[L], m->v16.empty() ? nullptr : m->v16[L], (int)m->cfg.kv_dim, (int)m->cfg.seq_len, (int)dst, (int)src);
    return 0;
}
// ---- the rest of KVCacheInterface (core/kv_cache.hpp:120-162; see include/ps_hip.h for why they reduce to these)
int ps_hip_model_kv_copy(ps_hip_model *m, size_t dst_cache_index, size_t src_token_index) {
    return ps_hip_model_kv_move(m, dst_cache_index, m->cur().position + src_token_index);
}
int ps_hip_model_kv_save_tokens(ps_hip_model *m, size_t n) {
    if (int rc = settle_pending(m)) return rc;
    if (m->cur().position + n > m->cfg.seq_len) { m->ctx->err = "kv_save_tokens: the length of kvcache is up to the preset threshold (n_ctx)"; return 2; }
    return 0;
}
int ps_hip_model_kv_unmask_tokens(ps_hip_model *m, size_t n) {
    if (int rc = settle_pending(m)) return rc;
    if (m->cur().position + n > m->cfg.seq_len) { m->ctx->err = "kv_unmask_tokens: the length of kvcache is up to the preset threshold (n_ctx)"; return 2; }
    unmask_range(m, m->cur().position, n);
    return 0;
}
int ps_hip_model_kv_append_tokens(ps_hip_model *m, size_t n, size_t *old_position) {
    const size_t old = m->cur().position;
    if (int rc = ps_hip_model_kv_save_tokens(m, n)) return rc;
    if (int rc = ps_hip_model_kv_unmask_tokens(m, n)) return rc;
    if (int rc = ps_hip_model_kv_advance(m, n)) return rc;
    if (old_position) *old_position = old;
    return 0;
}

// The lowered op-API path (ps_hip_model_forward_lowered) returns before its launches have run: whoever consumes its result next -- the
// cache advance (LlamaModel::forward advances right behind Executor::run, llama_model.cpp:109) or a logits read -- looks at the flag.
int ps_hip_model_sync_check(ps_hip_model *m) {
    ps_hip_ctx *c = m->ctx;
    if (!m->attn_unchecked) return 0;
    PS_CHECK(c, sync_stream(m));
    return check_attn_timeout(m, "lowered forward");
}
static int model_forward(ps_hip_model *m, const int32_t *tokens, int n, const int32_t *pos, const uint8_t *tree, int lm_head,
                         int32_t *argmax_host, bool advance) {
    ps_hip_ctx *c = m->ctx;
    if (int rc = settle_pending(m)) return rc;
    if (n <= 0 || n > m->max_batch) PS_FAIL(c, "model_forward: batch size out of range");
    for (int i = 1; i < n; i++)
        if (pos[i] != pos[0] + i) PS_FAIL(c, "model_forward: positions must be consecutive (KV append is one contiguous copy, norm_attention.cpp:82-91)");
    if (pos[0] < 0 || (size_t)pos[0] + (size_t)n > m->cfg.seq_len) PS_FAIL(c, "model_forward: KV cache is full (n_ctx)");
    if (int rc = check_tokens(m, tokens, n, "model_forward")) return rc;
    return with_attn_retry(m, [&]() -> int {
        PS_CHECK(c, hipSetDevice(c->device));
        m->pin_argmax_n = 0; // (the arg-max ids on the device are about to change)
        if (n == 1 && !tree) { // a decode step: the token travels from a pinned word, nothing to wait for before the launches go out
            if (m->pin_busy) PS_CHECK(c, sync_stream(m)); // (an upload from that word may still be queued)
            m->pin_tokens[0] = tokens[0];
            PS_CHECK(c, hipMemcpyAsync(m->tokens_dev, m->pin_tokens, 4, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, c->stream, m->state, pos[0], n, 0);
            m->pin_busy = true;
        } else {
            PS_CHECK(c, hipMemcpyAsync(m->tokens_dev, tokens, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
            if (tree) PS_CHECK(c, hipMemcpyAsync(m->tree_dev, tree, (size_t)n * n, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, c->stream, m->state, pos[0], n, 0);
            PS_CHECK(c, sync_stream(m)); // tokens/tree may be host temporaries
        }
        // A single token through this entry (ModelTokenIterator::decode over the op API, HIPBackend::plan's lowered graph) replays
        // a captured launch plan like ps_hip_model_decode_greedy does: the first call at a position range runs eagerly and captures.
        step_graph &g = m->graphs[lm_head ? G_FWD1_LM : G_FWD1];
        const bool graphable = n == 1 && !tree && (m->mode & 1) == 0 && m->cur().n_hidden == 0;
        if (graphable) graph_drop_if_stale(g, (size_t)pos[0]);
        if (graphable && g.exec) {
            PS_CHECK(c, hipGraphLaunch(g.exec, c->stream));
        } else {
            fwd_opts o;
            o.lm_head = lm_head != 0; o.tree = tree != nullptr; o.n_kv_host = pos[0] + n;
            if (int rc = enqueue_forward(m, n, o)) return rc;
            if (graphable) { // capture the same launches (nothing executes); the hint stays a lower bound of n_kv for 1024 positions
                PS_CHECK(c, sync_stream(m));
                o.n_kv_host = 0; o.n_kv_hint = pos[0]; // (no host-side n_kv inside a graph: the score grids cover n_ctx)
                if (m->long_window) o.n_kv_grid = (int)graph_window_end(m, (size_t)pos[0]); // (... or, at a long window, the positions this capture stays valid for)
                (void)graph_capture(m, g, (size_t)pos[0], [&] { return enqueue_forward(m, 1, o); }); // (a failure: stay eager)
            }
        }
        if (n == 1 && !tree) note_single_token(m);
        if (lm_head && argmax_host) PS_CHECK(c, hipMemcpyAsync(argmax_host, m->argmax_dev, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        if (lm_head && !advance) { // lowered graph: the ids ride to pinned memory behind the launches; ps_hip_model_argmax finds them there after the cache advance's wait
            PS_CHECK(c, hipMemcpyAsync(m->pin_argmax, m->argmax_dev, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
            m->pin_argmax_n = n; m->pin_argmax_pending = true;
        }
        if (!advance) return 0; // lowered graph: ps_hip_model_kv_advance / ps_hip_model_sync_check look at the time-out flag before the result counts
        PS_CHECK(c, sync_stream(m));
        if (const int rc = check_attn_timeout(m, "model_forward")) return rc; // (a time-out: the same forward once more, the inputs are the caller's)
        unmask_range(m, (size_t)pos[0], (size_t)n);
        m->cur().position = (size_t)pos[0] + (size_t)n; // m_kv->advance (llama_model.cpp:109)
        return 0;
    });
}
int ps_hip_model_forward(ps_hip_model *m, const int32_t *tokens, int n, const int32_t *pos, const uint8_t *tree, int lm_head,
                         int32_t *argmax_host) {
    return model_forward(m, tokens, n, pos, tree, lm_head, argmax_host, true);
}
int ps_hip_model_forward_lowered(ps_hip_model *m, const int32_t *tokens, int n, const int32_t *pos, const uint8_t *tree, int lm_head) {
    return model_forward(m, tokens, n, pos, tree, lm_head, nullptr, false);
}

// ModelTokenIterator's prefill (src/model/model.hpp:147-163): forward(tokens[done .. done + chunk), lm_head = false) chunk after chunk, the
// cache advanced after each -- with the SAME bits, but up to max_batch / chunk reference chunks per launch sequence ("super-chunk"): every
// mat-mul of a layer sees all their columns at once (per-chunk fixed costs paid a quarter as often at chunk 128 / max_batch 512), only the
// attention is evaluated per reference chunk (fwd_opts::attn_chunk).  8B, chunk 128: 14.4 k -> ~17 k tok/s.
// The super-chunk loop of ps_hip_model_prefill and ps_hip_model_score (the caller has checked its arguments): `per` reference chunks per launch sequence.
// With targets / out_host the lm_head runs for every column and the scoring launches behind it; the records come back per super-chunk, and a row whose
// certificate did not close is redone from the logits buffer, which still holds it.
static int append_chunks(ps_hip_model *m, const int32_t *tokens, int n, int chunk, int per, const char *who, const int32_t *targets, ps_score *out_host) {
    ps_hip_ctx *c = m->ctx;
    const bool score = targets != nullptr;
    m->pin_argmax_n = 0;
    if (per > 64) per = 64;
    if (per < 1) per = 1;
    for (int done = 0; done < n;) {
        const int ns = n - done < per * chunk ? n - done : per * chunk;
        const int pos = (int)m->cur().position;
        const int rc = with_attn_retry(m, [&]() -> int { // (per super-chunk: the ones before it have advanced the position)
            PS_CHECK(c, hipMemcpyAsync(m->tokens_dev, tokens + done, (size_t)ns * 4, hipMemcpyHostToDevice, c->stream));
            if (score) PS_CHECK(c, hipMemcpyAsync(m->score_targets, targets + done, (size_t)ns * 4, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, c->stream, m->state, pos, ns, 0);
            hipLaunchKernelGGL(set_sub_states_kernel, dim3(1), dim3(64), 0, c->stream, m->state_sub, pos, chunk, ns);
            fwd_opts o;
            o.lm_head = score; o.score = score; o.n_kv_host = pos + ns; o.attn_chunk = chunk;
            if (int rc_fw = enqueue_forward(m, ns, o)) return rc_fw;
            if (ns == 1) note_single_token(m);
            if (score) PS_CHECK(c, hipMemcpyAsync(out_host + done, m->score_out, (size_t)ns * sizeof(ps_score), hipMemcpyDeviceToHost, c->stream));
            PS_CHECK(c, sync_stream(m));
            return check_attn_timeout(m, who); // a one-token tail: once more, with the two launches
        });
        if (rc) return rc;
        if (score)
            if (int rc2 = psl_score_finish(c, m->logits, (int)m->cfg.vocab_size, (int64_t)m->cfg.vocab_size, ns, targets + done, out_host + done)) return rc2;
        unmask_range(m, (size_t)pos, (size_t)ns);
        m->cur().position += (size_t)ns;
        done += ns;
    }
    return 0;
}

int ps_hip_model_prefill(ps_hip_model *m, const int32_t *tokens, int n, int chunk) {
    ps_hip_ctx *c = m->ctx;
    if (n <= 0) return 0;
    if (int rc = settle_pending(m)) return rc;
    if (chunk <= 0 || chunk > m->max_batch) PS_FAIL(c, "model_prefill: chunk size out of range");
    if (m->cur().position + (size_t)n > m->cfg.seq_len) PS_FAIL(c, "model_prefill: KV cache is full (n_ctx)");
    if (int rc = check_tokens(m, tokens, n, "model_prefill")) return rc;
    PS_CHECK(c, hipSetDevice(c->device));
    return append_chunks(m, tokens, n, chunk, m->max_batch / chunk, "model_prefill", nullptr, nullptr);
}

// ps_hip_model_prefill with logits: the same super-chunks (the lm_head is column-wise like every other mat-mul), every column scored on the device behind
// the lm_head.  One exception to "the same": in the fp16-KV mode (mode bit 3) at chunk 1 every token is a launch sequence of its own, since that mode's
// attention serves single-token forwards only -- there the cache rows are those of single-token forwards in that mode, not prefill's.
int ps_hip_model_score(ps_hip_model *m, const int32_t *tokens, const int32_t *targets, int n, int chunk, ps_score *out_host) {
    ps_hip_ctx *c = m->ctx;
    if (n <= 0) return 0;
    if (int rc = settle_pending(m)) return rc;
    if (chunk <= 0 || chunk > m->max_batch) PS_FAIL(c, "model_score: chunk size out of range");
    if (m->cur().position + (size_t)n > m->cfg.seq_len) PS_FAIL(c, "model_score: KV cache is full (n_ctx)");
    if (int rc = check_tokens(m, tokens, n, "model_score")) return rc;
    if (m->mode & 32) PS_FAIL(c, "model_score: not in the fp16 prefill perf mode (mode bit 5: its batches have no logits)");
    const int vocab = (int)m->cfg.vocab_size;
    if (int rc = psl_score_check(c, vocab, targets, n, "model_score")) return rc;
    PS_CHECK(c, hipSetDevice(c->device));
    if (!m->score_out) { // first use; score_out is assigned last, so a failed allocation is tried again by the next call
        if (!m->score_scratch && dmalloc(m, &m->score_scratch, psl_score_scratch_bytes(vocab, m->max_batch))) return 1;
        if (!m->score_targets && dmalloc(m, (void **)&m->score_targets, (size_t)m->max_batch * 4)) return 1;
        if (dmalloc(m, (void **)&m->score_out, (size_t)m->max_batch * sizeof(ps_score))) return 1;
    }
    const bool single = (m->mode & 8) && chunk == 1;
    return append_chunks(m, tokens, n, chunk, single ? 1 : m->max_batch / chunk, "model_score", targets, out_host);
}

int ps_hip_model_forward_tree(ps_hip_model *m, const int32_t *tokens, int n, const int32_t *rope_pos, const uint8_t *tree, int lm_head,
                              int32_t *argmax_host, int advance) {
    ps_hip_ctx *c = m->ctx;
    if (int rc = settle_pending(m)) return rc;
    const size_t position = m->cur().position;
    if (n <= 0 || n > m->max_batch) PS_FAIL(c, "model_forward_tree: batch size out of range");
    if (position + (size_t)n > m->cfg.seq_len) PS_FAIL(c, "model_forward_tree: KV cache is full (n_ctx)");
    if (int rc = check_tokens(m, tokens, n, "model_forward_tree")) return rc;
    for (int i = 0; i < n; i++)
        if (rope_pos[i] < 0 || (uint32_t)rope_pos[i] >= m->cfg.seq_len) PS_FAIL(c, "model_forward_tree: position out of range");
    const int rc = with_attn_retry(m, [&]() -> int {
        PS_CHECK(c, hipSetDevice(c->device));
        m->pin_argmax_n = 0;
        PS_CHECK(c, hipMemcpyAsync(m->tokens_dev, tokens, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        PS_CHECK(c, hipMemcpyAsync(m->rope_pos_dev, rope_pos, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        if (tree) PS_CHECK(c, hipMemcpyAsync(m->tree_dev, tree, (size_t)n * n, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, c->stream, m->state, (int)position, n, 0);
        PS_CHECK(c, sync_stream(m));
        fwd_opts o;
        o.lm_head = lm_head != 0; o.tree = tree != nullptr; o.rope_pos = true; o.n_kv_host = (int)position + n;
        if (int rc_fw = enqueue_forward(m, n, o)) return rc_fw;
        if (n == 1 && !tree) note_single_token(m);
        if (lm_head && argmax_host) PS_CHECK(c, hipMemcpyAsync(argmax_host, m->argmax_dev, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        PS_CHECK(c, sync_stream(m));
        return check_attn_timeout(m, "model_forward_tree");
    });
    if (rc) return rc;
    if (advance) { unmask_range(m, position, (size_t)n); m->cur().position += (size_t)n; }
    return 0;
}

int ps_hip_model_kv_mask(ps_hip_model *m, size_t index, int visible) {
    ps_hip_ctx *c = m->ctx;
    if (int rc = settle_pending(m)) return rc;
    if (index >= m->cfg.seq_len) PS_FAIL(c, "kv_mask: index out of range");
    ps_hip_model::seq_state &kv = m->cur();
    const uint8_t v = visible ? 1 : 0;
    if (kv.kv_vis_host[index] == v) return 0;
    kv.kv_vis_host[index] = v;
    if (v) kv.n_hidden--; else kv.n_hidden++;
    PS_CHECK(c, hipMemcpyAsync(kv.kv_vis_dev + index, &kv.kv_vis_host[index], 1, hipMemcpyHostToDevice, c->stream));
    return 0;
}

// `steps` single-token steps, each fed the id the one before it chose: the arg-max (ps_hip_model_decode_greedy, cfg == nullptr), or the sampler chain in
// its place (ps_hip_model_decode_sampled, k_sample.hip): the configuration and the engine go to the device once per run, the engine comes back at the end.
// A time-out retry starts again from the caller's state, which is untouched until success.
static int decode_run(ps_hip_model *m, int32_t token, int steps, const ps_sample_cfg *cfg, ps_sample_state *state, int32_t *out_ids) {
    ps_hip_ctx *c = m->ctx;
    const char *who = cfg ? "decode_sampled" : "decode_greedy";
    const std::string w = std::string(who) + ": ";
    if (steps <= 0) return 0;
    if (int rc = settle_pending(m)) return rc;
    if (m->cur().n_hidden) PS_FAIL(c, w + "hidden KV slots (kv_mask) are not part of the captured step; unmask first");
    if (m->cur().position + (size_t)steps > m->cfg.seq_len) PS_FAIL(c, w + "KV cache would overflow n_ctx");
    if (int rc = check_tokens(m, &token, 1, who)) return rc;
    fwd_opts step;
    step.lm_head = true; step.advance = true; step.sampled = cfg != nullptr;
    step_graph &g = m->graphs[cfg ? G_SAMPLED : G_GREEDY];
    ps_sample_dev h; // (staging of the sampler's upload / read-back; the stream is idle between the two)
    return with_attn_retry(m, [&]() -> int {
        const size_t position = m->cur().position;
        if (cfg) {
            std::string err;
            if (psl_sample_pack(cfg, state, (int)m->cfg.vocab_size, &h, &err)) { c->err = w + err; return 2; }
        }
        PS_CHECK(c, hipSetDevice(c->device));
        if (cfg && !m->sample_dev && (dmalloc(m, (void **)&m->sample_dev, sizeof(ps_sample_dev)) || dmalloc(m, &m->sample_scratch, psl_sample_scratch_bytes((int)m->cfg.vocab_size)))) return 1;
        m->pin_argmax_n = 0;
        if (cfg) PS_CHECK(c, hipMemcpyAsync(m->sample_dev, &h, sizeof h, hipMemcpyHostToDevice, c->stream));
        PS_CHECK(c, hipMemcpyAsync(m->tokens_dev, &token, 4, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, c->stream, m->state, (int)position, 1, 0);
        PS_CHECK(c, sync_stream(m));
        // One loop for both kinds of model.  A regular model looks at its capture once per call (the hint it carries is a prefetch hint: stale costs time, never
        // results) and replays it to the end.  A long-window model's capture sizes its score grid for the end of its validity window (graph_window_end), so the
        // run is split there: the step at the boundary runs eagerly, the next window is captured, the replay goes on; its eager steps get the grid of their own position
        // (Eager mode, bit 0, no longer looks at the capture at all -- it used to drop a stale one on the way in.  Nothing replays it in that mode, and the next call
        // in mode 0 drops it at s == 0 as before.)
        const bool lw = m->long_window;
        for (int s = 0; s < steps;) {
            const size_t pos = position + (size_t)s;
            fwd_opts so = step;
            if (lw) so.n_kv_grid = (int)pos + 1;
            if (m->mode & 1) {
                if (int rc = enqueue_forward(m, 1, so)) return rc;
                s++;
                continue;
            }
            if (lw || s == 0) graph_drop_if_stale(g, pos);
            if (!g.exec) {
                // this step runs eagerly (the first one also performs every one-time hipFuncSetAttribute), then the identical launch sequence is captured;
                // capture itself executes nothing
                if (int rc = enqueue_forward(m, 1, so)) return rc;
                PS_CHECK(c, sync_stream(m));
                s++;
                if (lw) { so.n_kv_grid = (int)graph_window_end(m, pos); so.n_kv_hint = (int)pos; }
                if (!graph_capture(m, g, pos, [&] { return enqueue_forward(m, 1, so); })) { c->err.insert(0, w + "graph capture failed: "); return 2; }
                continue;
            }
            const int until = lw ? (int)std::min<size_t>((size_t)steps, g.hint + 1024 - position) : steps; // (lw: pos < g.hint + 1024, at least one step)
            for (; s < until; s++) PS_CHECK(c, hipGraphLaunch(g.exec, c->stream));
        }
        note_single_token(m);
        PS_CHECK(c, hipMemcpyAsync(out_ids, m->ids_dev, (size_t)steps * 4, hipMemcpyDeviceToHost, c->stream));
        if (cfg) PS_CHECK(c, hipMemcpyAsync(&h, m->sample_dev, sizeof h, hipMemcpyDeviceToHost, c->stream));
        PS_CHECK(c, sync_stream(m));
        // a time-out anywhere in the run: the position has not moved and the first token is the caller's -- the whole run once more on the
        // two-launch attention (every cache row it wrote is written again with the same values)
        if (const int rc = check_attn_timeout(m, who)) return rc;
        if (cfg) psl_sample_unpack(&h, state);
        m->cur().position += (size_t)steps;
        return 0;
    });
}
int ps_hip_model_decode_greedy(ps_hip_model *m, int32_t token, int steps, int32_t *out_ids) { return decode_run(m, token, steps, nullptr, nullptr, out_ids); }
int ps_hip_model_decode_sampled(ps_hip_model *m, int32_t token, int steps, const ps_sample_cfg *cfg, ps_sample_state *state, int32_t *out_ids) {
    return decode_run(m, token, steps, cfg, state, out_ids);
}

// ---- sequences: several KV caches (and positions, and visibility tables) on one model; include/ps_hip.h "Sequences"
int ps_hip_model_seq_count(const ps_hip_model *m) { return (int)m->seqs.size(); }
size_t ps_hip_model_seq_position(const ps_hip_model *m, int s) {
    if (s < 0 || s >= (int)m->seqs.size()) return (size_t)-1;
    return m->seqs[s].position;
}
// the model holds n_seq sequences and the batched step's tables.  Everything new is allocated before anything of the model changes: a failure (1) leaves it as it was.
static int seq_grow(ps_hip_model *m, int n_seq) {
    ps_hip_ctx *c = m->ctx;
    const int have = (int)m->seqs.size();
    if (n_seq < have) n_seq = have;
    if (m->seq_kv_dev && n_seq == have) return 0;
    const size_t L = m->cfg.n_layers, nctx = m->cfg.seq_len, cache_bytes = nctx * m->cfg.kv_dim * 4;
    PS_CHECK(c, hipSetDevice(c->device));
    PS_CHECK(c, sync_stream(m)); // (the table in use is about to be replaced)
    std::vector<void *> fresh;
    auto grab = [&](void **p, size_t bytes) {
        if (ps_dev_malloc(p, bytes ? bytes : 16) != hipSuccess) { (void)hipGetLastError(); return 1; }
        fresh.push_back(*p);
        return 0;
    };
    auto fail = [&]() {
        for (void *p : fresh) (void)ps_dev_free(p);
        c->err = "seq_reserve: out of device memory for " + std::to_string(n_seq) + " sequences (the model is unchanged)";
        return 1;
    };
    float **kv = nullptr;
    ps_seq_table *tab = m->seq_tab;
    int32_t *ids = m->seq_ids_dev;
    if (grab((void **)&kv, (size_t)n_seq * L * 2 * sizeof(float *))) return fail();
    if (!tab && (grab((void **)&tab, sizeof(ps_seq_table)) || grab((void **)&ids, nctx * PS_SEQ_COLS_MAX * 4))) return fail();
    std::vector<ps_hip_model::seq_state> add((size_t)(n_seq - have));
    for (auto &q : add) {
        q.k_cache.assign(L, nullptr); q.v_cache.assign(L, nullptr);
        for (size_t i = 0; i < L; i++)
            if (grab((void **)&q.k_cache[i], cache_bytes) || grab((void **)&q.v_cache[i], cache_bytes)) return fail();
        if (grab((void **)&q.kv_vis_dev, nctx)) return fail();
        q.kv_vis_host.assign(nctx, 1);
    }
    for (auto &q : add) {
        for (size_t i = 0; i < L; i++) { (void)hipMemsetAsync(q.k_cache[i], 0, cache_bytes, c->stream); (void)hipMemsetAsync(q.v_cache[i], 0, cache_bytes, c->stream); }
        (void)hipMemsetAsync(q.kv_vis_dev, 1, nctx, c->stream);
    }
    std::vector<float *> host((size_t)n_seq * L * 2);
    for (int q = 0; q < n_seq; q++) {
        const ps_hip_model::seq_state &s = q < have ? m->seqs[q] : add[q - have];
        for (size_t i = 0; i < L; i++) {
            host[((size_t)q * L + i) * 2]     = s.k_cache[i];
            host[((size_t)q * L + i) * 2 + 1] = s.v_cache[i];
        }
    }
    if (hipMemcpyAsync(kv, host.data(), host.size() * sizeof(float *), hipMemcpyHostToDevice, c->stream) != hipSuccess || sync_stream(m) != hipSuccess) {
        (void)hipGetLastError();
        return fail();
    }
    // committed from here on
    if (m->seq_kv_dev) {
        auto it = std::find(m->owned.begin(), m->owned.end(), (void *)m->seq_kv_dev);
        if (it != m->owned.end()) m->owned.erase(it);
        (void)ps_dev_free(m->seq_kv_dev);
    }
    for (void *p : fresh) m->owned.push_back(p);
    m->seq_kv_dev = kv; m->seq_tab = tab; m->seq_ids_dev = ids;
    for (auto &q : add) m->seqs.push_back(std::move(q));
    return 0;
}
int ps_hip_model_seq_reserve(ps_hip_model *m, int n_seq) {
    ps_hip_ctx *c = m->ctx;
    if (int rc = settle_pending(m)) return rc;
    if (n_seq < 1) PS_FAIL(c, "seq_reserve: at least one sequence");
    if (n_seq < (int)m->seqs.size()) PS_FAIL(c, "seq_reserve: the model holds more sequences already (growing only)");
    if (n_seq > 1 && m->long_window) PS_FAIL(c, "seq_reserve: a long-window model holds one sequence (the batched step's kernels keep their soft-max rows in LDS)");
    if (n_seq > 1 && (m->mode & 8)) PS_FAIL(c, "seq_reserve: the fp16-KV decode mode (mode bit 3) mirrors one cache; it does not combine with sequences");
    return seq_grow(m, n_seq);
}
// The current sequence is what every single-sequence entry point works on.  Captured steps bake the cache and visibility pointers in: a switch drops them
// (the next decode on the new sequence captures again, as it does after a mode change).
int ps_hip_model_seq_select(ps_hip_model *m, int s) {
    ps_hip_ctx *c = m->ctx;
    if (int rc = settle_pending(m)) return rc;
    if (s < 0 || s >= (int)m->seqs.size()) PS_FAIL(c, "seq_select: no such sequence");
    if (s == m->cur_seq) return 0;
    m->cur_seq = s;
    m->pin_argmax_n = 0;
    drop_graphs(m);
    return 0;
}

// One batched step (or `steps` greedy ones): argument checks first -- a refusal (2) has changed nothing.
static int batch_check(ps_hip_model *m, const int32_t *seq_ids, const int32_t *tokens, int n, int steps, const char *who) {
    ps_hip_ctx *c = m->ctx;
    const std::string w = std::string(who) + ": ";
    const int cap = m->max_batch < PS_SEQ_COLS_MAX ? m->max_batch : PS_SEQ_COLS_MAX;
    if (n < 1 || n > cap) PS_FAIL(c, w + "1 <= n <= min(16, max_batch) sequences per step");
    if (m->long_window) PS_FAIL(c, w + "not on a long-window model (the batched step's kernels keep their soft-max rows in LDS)");
    if (m->mode & 8) PS_FAIL(c, w + "the fp16-KV decode mode (mode bit 3) is not available for batched steps");
    if (!seq_ids || !tokens) PS_FAIL(c, w + "null argument");
    for (int i = 0; i < n; i++) {
        const int s = seq_ids[i];
        if (s < 0 || s >= (int)m->seqs.size()) PS_FAIL(c, w + "no such sequence: " + std::to_string(s));
        for (int j = 0; j < i; j++) if (seq_ids[j] == s) PS_FAIL(c, w + "sequence " + std::to_string(s) + " appears twice in one step");
        if (m->seqs[s].n_hidden) PS_FAIL(c, w + "sequence " + std::to_string(s) + " has hidden KV slots (kv_mask); unmask first");
        if (m->seqs[s].position + (size_t)steps > m->cfg.seq_len) PS_FAIL(c, w + "KV cache of sequence " + std::to_string(s) + " is full (n_ctx)");
    }
    return check_tokens(m, tokens, n, who);
}
// tables and tokens to the device; the stream is idle afterwards
static int batch_begin(ps_hip_model *m, const int32_t *seq_ids, const int32_t *tokens, int n, psl_seqs_args *sq) {
    ps_hip_ctx *c = m->ctx;
    if (int rc = seq_grow(m, 1)) return rc; // (a model that never reserved: the device tables of its one sequence)
    PS_CHECK(c, hipSetDevice(c->device));
    ps_seq_table t{};
    int64_t rows = 0;
    int top = 0;
    for (int i = 0; i < n; i++) {
        const int pos = (int)m->seqs[seq_ids[i]].position;
        t.col[i].seq = seq_ids[i]; t.col[i].pos = pos;
        rows += pos + 1;
        if (pos + 1 > top) top = pos + 1;
    }
    m->pin_argmax_n = 0;
    PS_CHECK(c, hipMemcpyAsync(m->seq_tab, &t, sizeof t, hipMemcpyHostToDevice, c->stream));
    PS_CHECK(c, hipMemcpyAsync(m->tokens_dev, tokens, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    PS_CHECK(c, sync_stream(m)); // (both sources are host temporaries)
    sq->tab = m->seq_tab; sq->kv = m->seq_kv_dev; sq->n_layers = (int)m->cfg.n_layers; sq->layer = 0; sq->n_kv_max = top;
    // the rows this step reads, K and V of every layer: read once per step, so non-temporal where they cannot stay in the memory-side cache anyway (as enqueue_forward's rule)
    sq->kv_stream = g_kv_stream_force >= 0 ? g_kv_stream_force : ((int64_t)m->cfg.n_layers * 2 * rows * m->cfg.kv_dim * 4 > ((int64_t)160 << 20) ? 1 : 0);
    return 0;
}
static void batch_advance(ps_hip_model *m, const int32_t *seq_ids, int n, size_t by) {
    for (int i = 0; i < n; i++) m->seqs[seq_ids[i]].position += by;
}
int ps_hip_model_decode_batch(ps_hip_model *m, const int32_t *seq_ids, const int32_t *tokens, int n, int lm_head, int32_t *argmax_host) {
    ps_hip_ctx *c = m->ctx;
    if (int rc = settle_pending(m)) return rc;
    if (int rc = batch_check(m, seq_ids, tokens, n, 1, "decode_batch")) return rc;
    psl_seqs_args sq{};
    if (int rc = batch_begin(m, seq_ids, tokens, n, &sq)) return rc;
    fwd_opts o;
    o.lm_head = lm_head != 0; o.sq = &sq;
    if (int rc = enqueue_forward(m, n, o)) return rc;
    if (lm_head && argmax_host) PS_CHECK(c, hipMemcpyAsync(argmax_host, m->argmax_dev, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    PS_CHECK(c, sync_stream(m));
    batch_advance(m, seq_ids, n, 1);
    return 0;
}
// `steps` such steps, every column fed its own arg-max.  The table (positions), the next tokens and the ids stay on the device; the host enqueues the steps back to
// back and waits once.  Eager launches, no hipGraph: the host's enqueue of a step is shorter than the step (DESIGN.md "Batched decode"), and a captured step would
// have to be keyed by the batch's composition.
int ps_hip_model_decode_batch_greedy(ps_hip_model *m, const int32_t *seq_ids, const int32_t *tokens, int n, int steps, int32_t *out_ids) {
    ps_hip_ctx *c = m->ctx;
    if (steps <= 0) return 0;
    if (int rc = settle_pending(m)) return rc;
    if (int rc = batch_check(m, seq_ids, tokens, n, steps, "decode_batch_greedy")) return rc;
    if (!out_ids) PS_FAIL(c, "decode_batch_greedy: null argument");
    psl_seqs_args sq{};
    if (int rc = batch_begin(m, seq_ids, tokens, n, &sq)) return rc;
    const int top0 = sq.n_kv_max;
    fwd_opts o;
    o.lm_head = true; o.advance = true; o.sq = &sq;
    for (int s = 0; s < steps; s++) {
        sq.n_kv_max = top0 + s;
        if (int rc = enqueue_forward(m, n, o)) { (void)sync_stream(m); return rc; }
    }
    PS_CHECK(c, hipMemcpyAsync(out_ids, m->seq_ids_dev, (size_t)steps * n * 4, hipMemcpyDeviceToHost, c->stream));
    PS_CHECK(c, sync_stream(m));
    batch_advance(m, seq_ids, n, (size_t)steps);
    return 0;
}
// The same loop with every column fed the token its own sampler chain drew (k_sample.hip's rows kernels behind the lm_head; DESIGN.md "Sampled batched decode").  Every
// column is packed before anything is uploaded: a column that is not covered refuses the whole call.  The chains go to the device once and come back once.
int ps_hip_model_decode_batch_sampled(ps_hip_model *m, const int32_t *seq_ids, const int32_t *tokens, int n, int steps, const ps_sample_cfg *cfgs, ps_sample_state *states,
                                      int32_t *out_ids) {
    ps_hip_ctx *c = m->ctx;
    if (steps <= 0) return 0;
    if (int rc = settle_pending(m)) return rc;
    if (int rc = batch_check(m, seq_ids, tokens, n, steps, "decode_batch_sampled")) return rc;
    if (!cfgs || !states || !out_ids) PS_FAIL(c, "decode_batch_sampled: null argument");
    std::vector<ps_sample_dev> h((size_t)n); // (staging of the chains' upload / read-back; the stream is idle between the two)
    for (int i = 0; i < n; i++) {
        std::string err;
        if (psl_sample_pack(cfgs + i, states + i, (int)m->cfg.vocab_size, &h[i], &err)) PS_FAIL(c, "decode_batch_sampled: column " + std::to_string(i) + ": " + err);
    }
    PS_CHECK(c, hipSetDevice(c->device));
    const size_t cap = (size_t)(m->max_batch < PS_SEQ_COLS_MAX ? m->max_batch : PS_SEQ_COLS_MAX);
    if (!m->sample_devs && dmalloc(m, (void **)&m->sample_devs, cap * sizeof(ps_sample_dev))) return 1;
    if (!m->sample_rows_scratch && dmalloc(m, &m->sample_rows_scratch, cap * psl_sample_scratch_bytes((int)m->cfg.vocab_size))) return 1;
    psl_seqs_args sq{};
    if (int rc = batch_begin(m, seq_ids, tokens, n, &sq)) return rc;
    PS_CHECK(c, hipMemcpyAsync(m->sample_devs, h.data(), (size_t)n * sizeof(ps_sample_dev), hipMemcpyHostToDevice, c->stream));
    const int top0 = sq.n_kv_max;
    fwd_opts o;
    o.lm_head = true; o.advance = true; o.sampled = true; o.sq = &sq;
    for (int s = 0; s < steps; s++) {
        sq.n_kv_max = top0 + s;
        if (int rc = enqueue_forward(m, n, o)) { (void)sync_stream(m); return rc; }
    }
    PS_CHECK(c, hipMemcpyAsync(out_ids, m->seq_ids_dev, (size_t)steps * n * 4, hipMemcpyDeviceToHost, c->stream));
    PS_CHECK(c, hipMemcpyAsync(h.data(), m->sample_devs, (size_t)n * sizeof(ps_sample_dev), hipMemcpyDeviceToHost, c->stream));
    PS_CHECK(c, sync_stream(m));
    for (int i = 0; i < n; i++) psl_sample_unpack(&h[i], states + i);
    batch_advance(m, seq_ids, n, (size_t)steps);
    return 0;
}

// ---- fork / save / restore (include/ps_hip.h "Sequences").  A forward only ever writes slots at or behind the position, so the first n slots of a
// sequence are, bit for bit, a valid history of n tokens for any other cache of the same shape.
// the sequence stands behind n tokens, every slot visible (what kv_truncate leaves); the captured steps hold cache pointers and no position: they stay
static void seq_set_history(ps_hip_model *m, ps_hip_model::seq_state &s, size_t n) {
    s.position = n;
    if (!s.n_hidden) return;
    std::fill(s.kv_vis_host.begin(), s.kv_vis_host.end(), (uint8_t)1);
    s.n_hidden = 0;
    (void)hipMemsetAsync(s.kv_vis_dev, 1, m->cfg.seq_len, m->ctx->stream);
}
int ps_hip_model_seq_fork(ps_hip_model *m, int src, const int32_t *dst, int n_dst, size_t n_tokens) {
    ps_hip_ctx *c = m->ctx;
    if (int rc = settle_pending(m)) return rc;
    const int n_seq = (int)m->seqs.size();
    if (n_dst < 1 || n_dst > n_seq - 1) PS_FAIL(c, "seq_fork: 1 <= n_dst <= seq_count - 1 destinations");
    if (!dst) PS_FAIL(c, "seq_fork: null argument");
    if (src < 0 || src >= n_seq) PS_FAIL(c, "seq_fork: no such sequence: " + std::to_string(src));
    for (int i = 0; i < n_dst; i++) {
        if (dst[i] < 0 || dst[i] >= n_seq) PS_FAIL(c, "seq_fork: no such sequence: " + std::to_string(dst[i]));
        if (dst[i] == src) PS_FAIL(c, "seq_fork: sequence " + std::to_string(src) + " is the source and a destination");
        for (int j = 0; j < i; j++) if (dst[j] == dst[i]) PS_FAIL(c, "seq_fork: sequence " + std::to_string(dst[i]) + " appears twice");
    }
    if (n_tokens > m->seqs[src].position) PS_FAIL(c, "seq_fork: more tokens than the source holds");
    if (m->seqs[src].n_hidden) PS_FAIL(c, "seq_fork: the source has hidden KV slots (kv_mask); unmask first");
    PS_CHECK(c, hipSetDevice(c->device));
    psl_fork_args a{};
    a.kv = m->seq_kv_dev; // (two sequences exist: seq_grow made the table)
    a.n_layers = (int)m->cfg.n_layers; a.kv_dim = (int)m->cfg.kv_dim; a.n_ctx = (int)m->cfg.seq_len; a.n_tokens = (int)n_tokens; a.src = src;
    for (int i = 0; n_tokens && i < n_dst; i += PS_FORK_DST_MAX) {
        a.n_dst = std::min(n_dst - i, PS_FORK_DST_MAX);
        std::copy(dst + i, dst + i + a.n_dst, a.dst);
        psl_seq_fork(c->stream, a);
    }
    PS_CHECK(c, hipGetLastError());
    for (int i = 0; i < n_dst; i++) seq_set_history(m, m->seqs[dst[i]], n_tokens);
    PS_CHECK(c, sync_stream(m));
    return 0;
}

size_t ps_hip_model_seq_state_bytes(const ps_hip_model *m, size_t n_tokens) { return ps_kv_state_bytes(m->cfg.n_layers, m->cfg.kv_dim, n_tokens); }
// K is a contiguous prefix, V a pitched copy (rows of n_tokens floats at pitch n_ctx); all on the ctx stream, one wait at the end
static int seq_state_copy(ps_hip_model *m, ps_hip_model::seq_state &s, uint8_t *host, size_t n, bool to_host) {
    ps_hip_ctx *c = m->ctx;
    const size_t kvd = m->cfg.kv_dim, plane = ps_kv_state_plane_bytes(m->cfg.kv_dim, n), pitch = (size_t)m->cfg.seq_len * 4;
    PS_CHECK(c, hipSetDevice(c->device));
    uint8_t *p = host + PS_KV_STATE_HEADER;
    for (uint32_t L = 0; n && L < m->cfg.n_layers; L++, p += 2 * plane) {
        if (to_host) {
            PS_CHECK(c, hipMemcpyAsync(p, s.k_cache[L], plane, hipMemcpyDeviceToHost, c->stream));
            PS_CHECK(c, hipMemcpy2DAsync(p + plane, n * 4, s.v_cache[L], pitch, n * 4, kvd, hipMemcpyDeviceToHost, c->stream));
        } else {
            PS_CHECK(c, hipMemcpyAsync(s.k_cache[L], p, plane, hipMemcpyHostToDevice, c->stream));
            PS_CHECK(c, hipMemcpy2DAsync(s.v_cache[L], pitch, p + plane, n * 4, n * 4, kvd, hipMemcpyHostToDevice, c->stream));
        }
    }
    PS_CHECK(c, sync_stream(m));
    return 0;
}
int ps_hip_model_seq_export(ps_hip_model *m, int seq, size_t n_tokens, void *host_buf, size_t bytes) {
    ps_hip_ctx *c = m->ctx;
    if (int rc = settle_pending(m)) return rc;
    if (seq < 0 || seq >= (int)m->seqs.size()) PS_FAIL(c, "seq_export: no such sequence");
    if (m->mode & 8) PS_FAIL(c, "seq_export: not in the fp16-KV decode mode (mode bit 3: the single-token attention reads the fp16 mirrors, which a state does not carry)");
    ps_hip_model::seq_state &s = m->seqs[seq];
    if (n_tokens > s.position) PS_FAIL(c, "seq_export: more tokens than the sequence holds");
    if (s.n_hidden) PS_FAIL(c, "seq_export: the sequence has hidden KV slots (kv_mask); unmask first");
    if (!host_buf || bytes < ps_hip_model_seq_state_bytes(m, n_tokens)) PS_FAIL(c, "seq_export: buffer smaller than ps_hip_model_seq_state_bytes");
    ps_kv_state_write_header(host_buf, m->cfg.n_layers, m->cfg.kv_dim, m->cfg.head_size, n_tokens, (uint32_t)ps_hip_build_contract());
    return seq_state_copy(m, s, (uint8_t *)host_buf, n_tokens, true);
}
int ps_hip_model_seq_import(ps_hip_model *m, int seq, const void *host_buf, size_t bytes) {
    ps_hip_ctx *c = m->ctx;
    if (int rc = settle_pending(m)) return rc;
    if (seq < 0 || seq >= (int)m->seqs.size()) PS_FAIL(c, "seq_import: no such sequence");
    if (m->mode & 8) PS_FAIL(c, "seq_import: not in the fp16-KV decode mode (mode bit 3: the fp16 mirrors would not follow)");
    uint64_t n = 0;
    if (const char *why = ps_kv_state_check(host_buf, bytes, m->cfg.n_layers, m->cfg.kv_dim, m->cfg.head_size, m->cfg.seq_len, (uint32_t)ps_hip_build_contract(), &n))
        PS_FAIL(c, std::string("seq_import: ") + why);
    ps_hip_model::seq_state &s = m->seqs[seq];
    if (int rc = seq_state_copy(m, s, (uint8_t *)const_cast<void *>(host_buf), (size_t)n, false)) return rc;
    seq_set_history(m, s, (size_t)n);
    return 0;
}

const float *ps_hip_model_logits(const ps_hip_model *m) { return m->logits; }
int ps_hip_model_argmax(ps_hip_model *m, int n, int32_t *ids_host) {
    ps_hip_ctx *c = m->ctx;
    if (n <= 0 || n > m->max_batch) PS_FAIL(c, "model_argmax: batch size out of range");
    if (int rc = settle_pending(m)) return rc;
    if (m->pin_argmax_n >= n) { // the last forward was a lowered one and left its ids in pinned memory
        if (m->pin_argmax_pending) PS_CHECK(c, sync_stream(m));
        memcpy(ids_host, m->pin_argmax, (size_t)n * 4);
        return 0;
    }
    PS_CHECK(c, hipMemcpyAsync(ids_host, m->argmax_dev, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    PS_CHECK(c, sync_stream(m));
    return 0;
}
const float *ps_hip_model_scratch(const ps_hip_model *m, int which) {
    switch (which) {
    case 0: return m->x;      // [max_batch][dim]     residual stream after the last layer
    case 1: return m->q;      // [max_batch][dim]     rotated q of the last layer
    case 2: return m->att;    // [max_batch][dim]     attention output of the last layer
    case 3: return m->hb;     // [max_batch][hidden]  silu(gate)*up of the last layer
    case 4: return m->scores; // [max_batch][n_heads][n_ctx] raw scores of the last layer
    }
    return nullptr;
}
const float *ps_hip_model_k_cache(const ps_hip_model *m, int L) { return m->cur().k_cache[L]; }
const float *ps_hip_model_v_cache(const ps_hip_model *m, int L) { return m->cur().v_cache[L]; }
uint64_t ps_hip_model_weight_bytes_per_token(const ps_hip_model *m) { return m->weight_bytes; }
// Roofline helper for bench.py: replay mat-vec launches of one single-token forward exactly as the decode step issues
// them (same kernels, same fused prologues; every layer's own weights -> the stream is HBM-cold like a real step),
// `reps` times, bracketed by HIP events on the backend stream.  which = 0: every quantized mat-vec of a token;
// which = 1: only the gate/up launch of each layer (the dominant kernel).  Then the same number of empty launches to
// expose the launch boundary.
int ps_hip_model_bench_gemv(ps_hip_model *m, int reps, int which, double *seq_ms, double *null_ms, int *n_launches) {
    return ps_hip_model_bench_matmul(m, reps, which, 1, seq_ms, null_ms, n_launches);
}
// the same replay with `bs` activation columns (bs = 128: the mat-muls of a prefill chunk, quantizer launches included)
int ps_hip_model_bench_matmul(ps_hip_model *m, int reps, int which, int bs, double *seq_ms, double *null_ms, int *n_launches) {
    ps_hip_ctx *c = m->ctx;
    if (bs < 1 || bs > m->max_batch) PS_FAIL(c, "bench_matmul: batch size out of range");
    const ps_llm_config &f = m->cfg;
    const int64_t dim = f.dim, hid = f.hidden_dim;
    hipEvent_t e0, e1;
    PS_CHECK(c, hipEventCreate(&e0));
    PS_CHECK(c, hipEventCreate(&e1));
    int launches = 0;
    auto pass = [&](bool count) -> int {
        ps_act a1 = ps_act_carve(m->act_mem, dim, m->max_batch), a2 = ps_act_carve(m->act_mem, hid, m->max_batch);
        const bool qkv = which == 0 || which == 2, op = which == 0 || which == 3, gu = which == 0 || which == 1, dn = which == 0 || which == 4;
        for (uint32_t L = 0; L < f.n_layers; L++) {
            if (qkv) {
                if (mm(m, mm_args(m, MM_QKV, L), a1, dim, bs)) return 2;
                if (count) launches += 1;
            }
            if (op) {
                psk_gemv_args go = mm_args(m, MM_O, L);
                go.out[0] = m->hb; go.residual = nullptr; // (not into x: the replay must not drift)
                if (mm(m, go, a1, dim, bs)) return 2;
                if (count) launches += 1;
            }
            if (gu) {
                psk_gemv_args gf = mm_args(m, MM_GATE_UP, L);
                gf.out[0] = m->g1; gf.out[1] = m->g1; // (hb is the O replay's output)
                if (mm(m, gf, a1, dim, bs)) return 2;
                if (count) launches += 1;
            }
            if (dn) {
                psk_gemv_args gd = mm_args(m, MM_DOWN, L);
                gd.out[0] = m->att; gd.residual = nullptr; // (no residual either: x stays what it was)
                gd.pro = 2; gd.pro_x = m->g1;              // (always the prologue quantizer, on the gate/up replay's output)
                if (mm(m, gd, a2, hid, bs)) return 2;
                if (count) launches += 1;
            }
        }
        if (which == 0 || which == 5) {
            if (mm(m, mm_args(m, MM_LM_HEAD, 0), a1, dim, bs)) return 2;
            if (count) launches += 1;
        }
        return 0;
    };
    if (pass(true)) return 2; // warm-up + launch count
    PS_CHECK(c, hipStreamSynchronize(c->stream));
    PS_CHECK(c, hipEventRecord(e0, c->stream));
    for (int r = 0; r < reps; r++) if (pass(false)) return 2;
    PS_CHECK(c, hipEventRecord(e1, c->stream));
    PS_CHECK(c, hipEventSynchronize(e1));
    float ms = 0.f;
    PS_CHECK(c, hipEventElapsedTime(&ms, e0, e1));
    *seq_ms = (double)ms / reps;
    PS_CHECK(c, hipEventRecord(e0, c->stream));
    for (int r = 0; r < reps * launches; r++) hipLaunchKernelGGL(null_kernel, dim3(256), dim3(256), 0, c->stream, (int *)nullptr);
    PS_CHECK(c, hipEventRecord(e1, c->stream));
    PS_CHECK(c, hipEventSynchronize(e1));
    PS_CHECK(c, hipEventElapsedTime(&ms, e0, e1));
    *null_ms = (double)ms / reps;
    *n_launches = launches;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

int ps_hip_model_set_mode(ps_hip_model *m, int mode) {
    mode |= m->long_window ? mode_env_or() & ~8 : mode_env_or(); // (a long-window model has no fp16-KV mode: the A/B variable does not ask it for one)
    if (mode & 64) { m->attn1_disabled = false; mode &= ~64; } // explicit re-arm of the one-launch attention after a time-out
    if (m->attn1_disabled) mode |= 16;                         // sticky: a later set_mode without bit 4 does not bring the form that timed out back
    if ((mode & 8) && m->long_window) { m->ctx->err = "set_mode: the fp16-KV decode mode (mode bit 3) is not available on a long-window model"; return 2; }
    if ((mode & 8) && m->seqs.size() > 1) { m->ctx->err = "set_mode: the fp16-KV decode mode mirrors one cache; it does not combine with sequences (seq_reserve)"; return 2; }
    if ((mode & 8) && m->k16.empty()) { // fp16 mirrors of the caches: filled from now on, so the cache must be empty
        if (m->cur().position != 0) { m->ctx->err = "set_mode: the fp16-KV decode mode must be switched on while the cache is empty"; return 2; }
        const size_t n = (size_t)m->cfg.seq_len * m->cfg.kv_dim * 2;
        m->k16.assign(m->cfg.n_layers, nullptr); m->v16.assign(m->cfg.n_layers, nullptr);
        for (uint32_t i = 0; i < m->cfg.n_layers; i++) {
            if (dmalloc(m, (void **)&m->k16[i], n) || dmalloc(m, (void **)&m->v16[i], n)) { m->k16.clear(); m->v16.clear(); return 2; }
            (void)hipMemsetAsync(m->k16[i], 0, n, m->ctx->stream);
            (void)hipMemsetAsync(m->v16[i], 0, n, m->ctx->stream);
        }
        if (dmalloc(m, (void **)&m->attn_part, (size_t)m->cfg.n_heads * 32 * (m->cfg.head_size + 2) * 4)) return 2;
    }
    if ((mode & 8) && !(m->mode & 8) && m->cur().position != 0) { m->ctx->err = "set_mode: the fp16-KV decode mode must be switched on while the cache is empty"; return 2; }
    if ((m->mode ^ mode) & (62 | 128)) drop_graphs(m); // the captured steps bake the launch plan in
    m->mode = mode;
    return 0;
}

} // extern "C"
