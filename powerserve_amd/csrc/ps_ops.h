// Launchers of the reference-shaped operator kernels (k_ops.hip) and the fused attention kernels
// (k_attn.hip).  Everything enqueues on `st`; pointers are device pointers.
#pragma once
#include "ps_internal.h"

void psl_mul_mat_f32(hipStream_t st, const ps_tensor *dst, const ps_tensor *a, const ps_tensor *b);
void psl_rms_norm(hipStream_t st, const ps_tensor *dst, const ps_tensor *src, const float *w, float eps);
void psl_rope(hipStream_t st, const ps_tensor *dst, const ps_tensor *src, const float *cache, int n_dims, int neox);
void psl_softmax_ext(hipStream_t st, const ps_tensor *dst, const ps_tensor *src, const float *mask, float scale);
void psl_add(hipStream_t st, const ps_tensor *dst, const ps_tensor *a, const ps_tensor *b);
void psl_dup(hipStream_t st, const ps_tensor *dst, const ps_tensor *src);
void psl_silu_hadamard(hipStream_t st, float *out, const float *g, const float *u, int64_t n);
void psl_get_rows(hipStream_t st, const ps_weight *w, const int32_t *tokens_dev, int n, float *out);
void psl_get_mask(hipStream_t st, float *out, int64_t n_kv, int bs, const int32_t *pos_dev, const uint8_t *tree_dev);
void psl_argmax(hipStream_t st, const float *src, int64_t n, int64_t rows, int32_t *out);

// device-resident per-step state of the fused model path (read by kernels so a captured graph replays)
struct ps_step_state {
    int32_t pos0;    // KV position of the first token of this forward
    int32_t bs;      // tokens in this forward
    int32_t n_out;   // decode: number of ids written so far
    int32_t _pad;
};

struct psl_attn_args {
    int n_heads, n_kv_heads, head_size, n_ctx, neox, n_dims;
    const ps_step_state *state;
    const float *rope_table; // [n_ctx][head_size] (cos, sin) pairs, host-built (ggml.c:15344-15358)
    float *q;                // [bs][n_heads*hs]   in: raw q, out: rotated q
    const float *k, *v;      // [bs][kv_dim]
    float *k_cache;          // [n_ctx][kv_dim]
    float *v_cache;          // [kv_dim][n_ctx]
    float *scores;           // [bs][n_heads][n_ctx] scratch
    float *att;              // [bs][n_heads*hs]
    const uint8_t *tree;     // optional [bs][bs] tree mask
    const int32_t *rope_pos; // optional [bs]: RoPE position of each batch column (default: its cache slot pos0 + i)
    const uint8_t *kv_vis;   // optional [n_ctx]: 0 hides a cached slot (KVCacheInterface::mask / unmask)
    float scale;
    ps_act qact;             // optional (qs != null): the V.p kernel of a batch also leaves `att` quantized (Q8_K, + the fragment copies when qf is set) for the O projection
    int64_t qact_K;          // = n_heads * head_size
    int n_kv_host;           // pos0 + bs when the host knows it at enqueue time (eager forwards), 0 inside a captured graph: sizes the score grids
    int bs_host;             // with n_kv_host: the batch size, so that the batch kernels need not wait for the device-resident state (an L2 miss at the head of every launch)
    _Float16 *k16, *v16;     // optional fp16 mirrors of the caches, both [n_ctx][kv_dim] (fp16-KV decode mode: ps_hip_model_set_mode bit 3)
    float *part;             // [n_heads][FL_SPLITS][head_size + 2] partial (o, m, l) of the split-KV decode attention
    unsigned long long *dbg; // timeline buffer of the single-token kernels (ps_hip_debug_timeline keys 40 / 41), or null
    unsigned *sync;          // [2048] words, zeroed once: [31] the one-launch decode attention's spin-timeout flag
    float *xchg;             // attn_decode2: raw scores in flight between the workgroups of a kv head, [n_kv_heads][4][n_ctx rounded up to 32]; null: not used
    unsigned *tick;          // attn_decode2: [64 * kv head] arrival counters, zeroed once (epoch = ticket / workgroups per head)
    unsigned long long *gran; // the fused Q / K / V + attention launch: [n_kv_heads][(r2 + 2) * head_size] {tag, value} granules of rendezvous A, zeroed with `tick`; null: the counter hand-off
    int n_kv_lo;             // attn_decode2: a lower bound of pos0 + 1 known to the host at enqueue time (a prefetch HINT only)
    int kv_stream;           // single-token kernels: 1 = the cached K rows / V channels are read with non-temporal loads (the model's whole cache does not fit the memory-side
                             // cache, so nothing of it survives from token to token and it should not displace what does); 0 = plain loads (a small cache is served from there)
};
void psl_rope_append(hipStream_t st, const psl_attn_args &a, int bs);
void psl_attn_scores(hipStream_t st, const psl_attn_args &a, int bs);
void psl_attn_softmax_pv(hipStream_t st, const psl_attn_args &a, int bs);
bool psl_attn_pv_quantizes(const psl_attn_args &a, int bs); // whether psl_attn_softmax_pv(a, bs) would fill a.qact (shape conditions of the fused epilogue)
bool psl_attn_decode_f16(hipStream_t st, const psl_attn_args &a); // single token over the fp16 mirrors: split-KV online soft-max + combine (NOT bit-exact); false: not covered
bool psl_attn_decode2(hipStream_t st, int n_cu, const psl_attn_args &a); // single token: scores + soft-max + V.p in one launch (counter exchange of the scores, V.p on the matrix cores); false: not covered
size_t psl_attn_decode2_xchg_bytes(int n_kv_heads, int n_ctx);
// Q / K / V mat-vec (RMSNorm + quantizer prologue, RoPE + KV append: g.rope set) AND the single-token attention in one launch (k_qkvattn.hip): four launches per decode
// layer instead of five; false: not covered, the caller issues the Q / K / V mat-vec (psk_matmul) + psl_attn_decode2
bool psk_qkv_attn(hipStream_t st, int n_cu, const psk_gemv_args &g, int64_t K, const psl_attn_args &a);
size_t psl_attn_softmax_pv_lds(const psl_attn_args &a); // dynamic LDS bytes (grows with n_ctx)
void psl_attn_pv_mfma(hipStream_t st, const psl_attn_args &a, int bs); // bs >= 8: V.p on the matrix cores over the probabilities in a.scores (what psl_attn_softmax_pv launches behind its soft-max)
// long-window models (k_attn_long.hip): soft-max with the rows in device memory + V.p, behind psl_attn_scores; any n_ctx up to PS_HIP_LONG_CTX_MAX
void psl_attn_long_softmax_pv(hipStream_t st, const psl_attn_args &a, int bs);
void psl_softmax_long_ext(hipStream_t st, const ps_tensor *dst, const ps_tensor *src, const float *mask, float scale); // softmax_ext rows above the LDS-resident kernel's cap
int psl_attn_long_set_tile(int positions); // ps_hip_debug_set(13, v)

// ---- batched decode: one token per SEQUENCE, each sequence on a KV cache of its own (ps_hip_model_decode_batch)
// Device table of a batched step.  col[i] = (sequence, position) of batch column i: the token goes to cache slot `pos` of that sequence (its RoPE position too)
// and attends over slots [0, pos].  A greedy run updates the table itself (psl_seqs_advance): nothing position-dependent comes from the host between steps.
#define PS_SEQ_COLS_MAX 16 // the narrow mat-mul's width (k_gemm4k.hip)
struct ps_seq_col { int32_t seq, pos; };
struct ps_seq_table {
    int32_t n_out;   // greedy run: steps recorded so far
    int32_t _pad[3];
    ps_seq_col col[PS_SEQ_COLS_MAX];
};
struct psl_seqs_args {
    const ps_seq_table *tab;
    float *const *kv;   // [n_seq][n_layers][2] cache bases: K [n_ctx][kv_dim], V [kv_dim][n_ctx] of (sequence, layer)
    int n_layers, layer;
    int n_kv_max;       // upper bound of pos + 1 over the columns, known to the host at enqueue time: sizes the score grid (workgroups past a column's own length exit)
    int kv_stream;      // as psl_attn_args::kv_stream
};
void psl_rope_append_seqs(hipStream_t st, const psl_attn_args &a, const psl_seqs_args &s, int n);
// scores, then soft-max + V.p, of n columns in two launches; no workgroup waits for another (k_attn.hip)
void psl_attn_seqs(hipStream_t st, const psl_attn_args &a, const psl_seqs_args &s, int n);
// bookkeeping of a greedy batched step: token[i] = argmax[i], ids[n_out * n + i] = argmax[i], col[i].pos++, n_out++
void psl_seqs_advance(hipStream_t st, ps_seq_table *tab, const int32_t *argmax, int32_t *tokens, int32_t *ids, int n);
// fork (k_seqcopy.hip): slots [0, n_tokens) of sequence `src`, K and V of every layer, into the n_dst sequences dst[] in one launch; kv as psl_seqs_args::kv.
// More destinations than PS_FORK_DST_MAX take another launch (ps_hip_model_seq_fork).
#define PS_FORK_DST_MAX 15
struct psl_fork_args {
    float *const *kv;
    int n_layers, kv_dim, n_ctx, n_tokens; // n_tokens >= 1
    int src, n_dst;
    int dst[PS_FORK_DST_MAX];
};
void psl_seq_fork(hipStream_t st, const psl_fork_args &a);
// two-stage arg-max (64 partials per row).  With state != NULL the final stage also does the greedy-decode
// bookkeeping: token[0] = id, ids[state->n_out++] = id, state->pos0++.
void psl_argmax2(hipStream_t st, const float *src, int64_t n, int64_t rows, int32_t *out, float *part_v, int *part_i,
                 ps_step_state *state, int32_t *token, int32_t *ids);

// host restatement of ggml_rope_cache_init for positions [0, n_pos) -> table[n_pos][ne0]
void ps_rope_table_host(const ps_rope_params *rp, int64_t ne0, const int32_t *pos, int n_pos, float *table);

// device sampler (k_sample.hip): configuration + engine state in one device buffer, so that a captured step serves every
// configuration; the host packs it from ps_sample_cfg / ps_sample_state (psl_sample_pack) and reads the engine back (psl_sample_unpack)
struct ps_sample_dev {
    uint32_t mt[624];
    uint32_t mt_pos;
    int32_t k;
    float temperature, top_p, repeat, freq, present;
    int32_t ban_id;   // EOS entry set to -inf (ignore_eos), -1: none
    int32_t spare_id; // line feed left unpenalised (!penalize_nl), -1: none
    int32_t n_pen;    // distinct tokens of the counted window (0: penalty inactive)
    uint64_t n_outputs, n_exact;
    int32_t pen_tok[PS_SAMPLE_WINDOW_MAX], pen_cnt[PS_SAMPLE_WINDOW_MAX];
};
int psl_sample_pack(const ps_sample_cfg *c, const ps_sample_state *s, int n_vocab, ps_sample_dev *out, std::string *err);
void psl_sample_unpack(const ps_sample_dev *d, ps_sample_state *s);
size_t psl_sample_scratch_bytes(int n_vocab);
// penalty + top-k + tail + draw of one row of n logits; token_out (device) optional; with state != NULL also the decode
// bookkeeping of psl_argmax2: token[0] = id, ids[state->n_out++] = id, state->pos0++
void psl_sample(hipStream_t st, const float *logits, int n, ps_sample_dev *d, void *scratch, int32_t *token_out, ps_step_state *state, int32_t *tokens, int32_t *ids);
// the same chain on `rows` rows in one pair of launches: row r of n logits at logits + r * row_stride (any alignment) with devs[r], its own scratch of
// psl_sample_scratch_bytes(n) at scratch + r * that, its id to drawn[r] (device).  No bookkeeping: a batched step feeds drawn[] to psl_seqs_advance
void psl_sample_rows(hipStream_t st, const float *logits, int n, int64_t row_stride, int rows, ps_sample_dev *devs, void *scratch, int32_t *drawn);

// scoring (k_score.hip): three launches over rows x n logits (row r at logits + r * stride), targets and records on the device; then, with the records on the
// host and the stream idle, psl_score_finish redoes the flagged rows exactly and counts
size_t psl_score_scratch_bytes(int n_vocab, int rows);
void psl_score(hipStream_t st, const float *logits, int n, int64_t stride, int rows, const int32_t *targets_dev, void *scratch, ps_score *out_dev);
int psl_score_check(ps_hip_ctx *c, int n_vocab, const int32_t *targets, int rows, const char *who);
int psl_score_finish(ps_hip_ctx *c, const float *logits_dev, int n, int64_t stride, int rows, const int32_t *targets, ps_score *out);
