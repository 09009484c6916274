/* include/ps_hip.h — C-ABI of the MI355X (gfx950) backend for PowerServe's ggml decode hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  Each entry
 * point names the reference interface it replaces (paths relative to the PowerServe tree).
 *
 *   reference                                             this library
 *   ---------------------------------------------------   ---------------------------------------------
 *   powerserve_compute_forward_mul_mat  (ggml.h:767)      ps_hip_mul_mat
 *   powerserve_compute_forward_add      (ggml.h:774)      ps_hip_add
 *   powerserve_compute_forward_rms_norm (ggml.h:787)      ps_hip_rms_norm
 *   powerserve_compute_forward_rope     (ggml.h:795)      ps_hip_rope
 *   powerserve_compute_forward_dup      (ggml.h:804)      ps_hip_dup
 *   powerserve_compute_forward_softmax_ext (ggml.h:810)   ps_hip_softmax_ext
 *   powerserve_compute_forward_soft_max (ggml.h:781)      ps_hip_soft_max
 *   powerserve_get_vec_dot_type         (ggml.h:765)      ps_hip_vec_dot_type
 *   GGMLBackend::silu_hadamard (backend/ggml/ggml.cpp:115)        ps_hip_silu_hadamard
 *   GGMLBackend::get_embedding (backend/ggml/ggml_wrapper.cpp:181) ps_hip_get_embedding
 *   Executor GET_MASK          (executor/executor.cpp:210-224)    ps_hip_get_mask
 *   quantize_row_q8_0 / q8_K   (ggml-quants.c:887, :3849)         ps_hip_quantize_act
 *   GGMLBackend::plan + fused decode (backend/ggml/ggml.cpp:30)   ps_hip_model_* (one call per forward)
 *
 * Conventions
 *   - ps_tensor mirrors ggml_tensor's (type, ne[4], nb[4] in BYTES, data) as built by convert_to_ggml
 *     (backend/ggml/ggml.hpp:87-96).  `data` is a DEVICE pointer, except for quantized weights where it is
 *     the ps_weight handle returned by ps_hip_weight_upload (the device copy is repacked).
 *   - every function returns 0 on success, non-zero on failure; ps_hip_last_error(ctx) gives the message.
 *     Nothing throws across this boundary; the C++ façade converts failures into the reference's
 *     abort/throw behaviour (core/logger.hpp:56-82).
 *   - one HIP stream per ctx; ops are asynchronous in stream order; ps_hip_sync waits.  A ctx is not
 *     thread-safe (same as one GGMLBackend).
 */
#ifndef PS_HIP_H
#define PS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_HIP_ABI_VERSION 2
/* return codes: 0 ok; 1 a HIP runtime error; 2 a refused call (bad argument, unsupported shape ...); 3 see ps_hip_model_sync_check */
#define PS_HIP_ATTN_TIMEOUT 3

/* ggml_type values (libs/ggml/include/ggml.h:361-398); Q4_K/Q5_K/Q6_K extend PowerServe's DataType enum
 * (core/data_type.hpp:24-35) which stops at Q8_0. */
enum ps_dtype {
    PS_F32  = 0,
    PS_F16  = 1,
    PS_Q4_0 = 2,
    PS_Q8_0 = 8,
    PS_Q4_K = 12,
    PS_Q5_K = 13,
    PS_Q6_K = 14,
    PS_Q8_K = 15,
    PS_I32  = 26,
};

typedef struct ps_hip_ctx ps_hip_ctx;
typedef struct ps_weight ps_weight;   /* device-resident quantized weight matrix [K, N] */
typedef struct ps_hip_model ps_hip_model;
typedef struct ps_hip_graph ps_hip_graph;

typedef struct {
    int32_t dtype;
    int32_t _pad;
    int64_t ne[4];  /* elements per dim, dim0 fastest */
    uint64_t nb[4]; /* strides in bytes */
    void *data;
} ps_tensor;

/* rope_compute_params (ggml.h:651-661) */
typedef struct {
    int32_t n_dims, n_ctx_orig;
    float freq_base, freq_scale, ext_factor, attn_factor, beta_fast, beta_slow;
    int32_t mode; /* rope_type: 0 adjacent pairs, 2 NEOX */
} ps_rope_params;

/* ModelConfig::LLMConfig (core/config.hpp:86-109) */
typedef struct {
    uint32_t dim, hidden_dim, n_layers, n_heads, n_kv_heads, seq_len, vocab_size, kv_dim, head_size;
    float norm_eps;
    ps_rope_params rope;
} ps_llm_config;

/* ------------------------------------------------------------------ context, memory, timing */
int ps_hip_abi_version(void);
/* Which build of the reference this library's fp32 arithmetic follows bit for bit.  0 (lib/libps_hip.so, the default and what every "bit-exact"
 * in this repository refers to): the reference compiled with -ffp-contract=off -- each operation rounds where the C source rounds.  1
 * (lib/libps_hip_contract.so, built with -DPS_CONTRACT by powerserve_amd/build.py): the reference as its own CMake compiles it on an FMA machine
 * (no contraction flag: GCC's default -ffp-contract=fast; CMakeLists.txt:24-33, libs/ggml/src/CMakeLists.txt:1173), which fuses the RoPE rotation
 * (ggml.c:15455-15475) and the n % 32 leftovers of ggml_vec_dot_f32 (ggml.c:2123-2125); Q5_K (a third fused site, ggml-quants.c:8411) is
 * refused by that build. */
int ps_hip_build_contract(void);
int ps_hip_device_count(void);
int ps_hip_create(int device, ps_hip_ctx **out);
void ps_hip_destroy(ps_hip_ctx *ctx);
const char *ps_hip_last_error(const ps_hip_ctx *ctx);
int ps_hip_device_name(const ps_hip_ctx *ctx, char *buf, size_t cap);
int ps_hip_malloc(ps_hip_ctx *ctx, size_t bytes, void **dptr);
int ps_hip_free(ps_hip_ctx *ctx, void *dptr);
int ps_hip_memcpy_h2d(ps_hip_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int ps_hip_memcpy_d2h(ps_hip_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int ps_hip_memset(ps_hip_ctx *ctx, void *dst_dev, int value, size_t bytes);
int ps_hip_sync(ps_hip_ctx *ctx);
void *ps_hip_stream(ps_hip_ctx *ctx); /* hipStream_t */
/* HIP events on the ctx stream (bench.py measures kernel time with these) */
int ps_hip_event_create(ps_hip_ctx *ctx, void **ev);
int ps_hip_event_record(ps_hip_ctx *ctx, void *ev);
int ps_hip_event_elapsed_ms(ps_hip_ctx *ctx, void *ev_start, void *ev_stop, float *ms); /* syncs ev_stop */
int ps_hip_event_destroy(ps_hip_ctx *ctx, void *ev);

/* ------------------------------------------------------------------ weights */
/* host_blocks: N rows of GGUF blocks of `dtype` (row stride = ggml_row_size(dtype, K)), or F32 / F16 rows (any K).
 * The device copy of a quantized matrix is repacked into a structure-of-arrays layout private to the backend; F32 / F16 rows are kept as they are.
 * F16 mat-muls follow ggml_vec_dot_f16 (activation rounded by ggml_fp32_to_fp16_row, n % 32 leftovers in double): bit-exact like the other types. */
int ps_hip_weight_upload(ps_hip_ctx *ctx, int dtype, const void *host_blocks, int64_t K, int64_t N, ps_weight **out);
void ps_hip_weight_free(ps_hip_ctx *ctx, ps_weight *w);
/* GGUF bytes of the matrix = N * ggml_row_size(dtype, K): the roofline's algorithmic byte count */
uint64_t ps_hip_weight_gguf_bytes(const ps_weight *w);
int ps_hip_weight_dtype(const ps_weight *w);

/* ------------------------------------------------------------------ op level (reference-shaped) */
int ps_hip_vec_dot_type(int dtype);
size_t ps_hip_row_size(int dtype, int64_t k);
/* x: [K, rows] F32 contiguous (device) -> out: rows x GGUF-layout block_q8_0 / block_q8_K (device), or (vdt PS_F16) rows x K fp16.
 * Bit-exact with quantize_row_q8_0 (AVX2 branch) / quantize_row_q8_K / ggml_fp32_to_fp16_row (F16C). */
int ps_hip_quantize_act(ps_hip_ctx *ctx, int vdt, const float *x, int64_t K, int64_t rows, void *out_blocks);
/* dst[ne01, ne11, ne12] = src0 x src1.  src0: quantized weight handle (2-D) or F32 tensor with arbitrary
 * nb[1..3] (K/V-cache views, GQA broadcast over dim 2); src1: F32, nb[0]==4; dst: F32 contiguous rows. */
int ps_hip_mul_mat(ps_hip_ctx *ctx, const ps_tensor *dst, const ps_tensor *src0, const ps_tensor *src1);
int ps_hip_rms_norm(ps_hip_ctx *ctx, const ps_tensor *dst, const ps_tensor *src, const ps_tensor *weight, float eps);
/* pos: HOST int32[n_pos] (the reference passes a std::vector<int>, executor.cpp:123-128) */
int ps_hip_rope(ps_hip_ctx *ctx, const ps_tensor *dst, const ps_tensor *src, const int32_t *pos, int n_pos,
                const ps_rope_params *rp);
/* rows of up to 150 KiB stay in LDS; longer ones, up to PS_HIP_LONG_CTX_MAX + 64 elements (contiguous F32), take the long-window row routine (same bits) */
int ps_hip_softmax_ext(ps_hip_ctx *ctx, const ps_tensor *dst, const ps_tensor *src, const ps_tensor *mask,
                       float scale, float max_bias);
/* GGMLBackend::softmax (backend/ggml/ggml_wrapper.cpp:57-69) -> powerserve_compute_forward_soft_max (ggml.c:15060-15089): the same
 * row soft-max with scale 1, no mask, max_bias 0 (it sets exactly those op_params and calls ggml_compute_forward_soft_max_f32). */
int ps_hip_soft_max(ps_hip_ctx *ctx, const ps_tensor *dst, const ps_tensor *src);
int ps_hip_add(ps_hip_ctx *ctx, const ps_tensor *dst, const ps_tensor *a, const ps_tensor *b);
int ps_hip_dup(ps_hip_ctx *ctx, const ps_tensor *dst, const ps_tensor *src); /* COPY and CONT */
int ps_hip_silu_hadamard(ps_hip_ctx *ctx, const ps_tensor *dst, const ps_tensor *gate, const ps_tensor *up);
/* weight->data: ps_weight handle (quantized, F32 or F16 table [dim, vocab]); tokens: HOST int32[n].  F16 rows are widened exactly -- beyond the
 * reference, whose GGMLBackend::get_embedding asserts on FP16 tables (ggml_wrapper.cpp:193-206); a tied F16 lm_head needs it. */
int ps_hip_get_embedding(ps_hip_ctx *ctx, const ps_tensor *dst, const ps_tensor *weight, const int32_t *tokens,
                         int n);
/* dst [n_kv, bs] F32: (j <= pos[i]) ? 0 : -inf  — or, with tree != NULL (bs x bs bytes, row i = which batch
 * tokens token i may attend to), the speculative-decode tree mask over the last bs cache slots. */
int ps_hip_get_mask(ps_hip_ctx *ctx, const ps_tensor *dst, const int32_t *pos, int n_pos, const uint8_t *tree);
/* rows of `src` ([n, rows] F32) -> int32 index of the first maximum per row, written to out_dev */
int ps_hip_argmax(ps_hip_ctx *ctx, const float *src, int64_t n, int64_t rows, int32_t *out_dev);

/* ------------------------------------------------------------------ whole-model fast path
 * What HIPBackend::plan() lowers the reference's 28-op layer sequence to: fused kernels, a persistent
 * arena, a device-resident FP32 KV cache (K [n_ctx][kv_dim], V [kv_dim][n_ctx] — the reference's layout,
 * backend/ggml/ggml_kv_cache.cpp:48-57, model/module/norm_attention.cpp:82-104) and a captured hipGraph
 * for the single-token step. */
typedef struct {
    ps_llm_config cfg;
    int32_t is_qwen2; /* QKV bias (model/qwen2/qwen2_model.cpp:75) */
    int32_t max_batch; /* largest forward batch (prefill chunk) */
    const ps_weight *token_embd, *output; /* output == NULL -> tied lm_head (weights.hpp:67-68) */
    const float *output_norm;             /* device F32 [dim] */
    /* per layer arrays of n_layers entries */
    const float *const *attn_norm, *const *ffn_norm;
    const ps_weight *const *attn_q, *const *attn_k, *const *attn_v, *const *attn_output;
    const ps_weight *const *ffn_gate, *const *ffn_up, *const *ffn_down;
    const float *const *attn_q_bias, *const *attn_k_bias, *const *attn_v_bias; /* NULL unless is_qwen2 */
} ps_model_desc;

int ps_hip_model_create(ps_hip_ctx *ctx, const ps_model_desc *desc, ps_hip_model **out);
/* Long windows.  ps_hip_model_create keeps a forward's soft-max rows in LDS and refuses a window they do not fit in ("n_ctx too large": 7 296 slots at 4 query
 * heads per kv head, 3 648 at 8).  ps_hip_model_create_long is ps_hip_model_create for a LONG-WINDOW model: any n_ctx that is a multiple of 4, up to
 * PS_HIP_LONG_CTX_MAX.  Its attention keeps score and probability rows in device memory: EVERY forward (single tokens, batches, prefill super-chunks, tree
 * forwards, hidden slots, ps_hip_model_score, the decode loops, the lowered forward) runs the score kernel, attn_softmax_long_kernel and a V.p kernel
 * (attn_pv_long_kernel below 8 columns, the matrix-core kernels from 8 on) -- bit for bit what a regular model computes, at any depth.  The fused head, the
 * one-launch attention and the fp16-KV kernel are never chosen: mode bits 4 and 7 are accepted and change nothing; mode bit 3 and ps_hip_model_seq_reserve
 * beyond one sequence are refused (rc 2, nothing changed; the batched step's kernels hold LDS rows).  The property is fixed at creation.
 * The score buffer is max_batch * n_heads * n_ctx * 4 bytes and the FP32 KV cache 2 * n_layers * n_ctx * kv_dim * 4: rc 1 when the device has no room. */
#define PS_HIP_LONG_CTX_MAX 131072
int ps_hip_model_create_long(ps_hip_ctx *ctx, const ps_model_desc *desc, ps_hip_model **out);
int ps_hip_model_is_long(const ps_hip_model *m);
/* diagnostics: [0] rows soft-maxed by the long kernels (attention rows and ps_hip_softmax_ext rows above the LDS-resident kernel's cap), [1] of them through the
 * sequential sum -- the row sum is formed in the device's order and CERTIFIED to give the reference's (float)(1 / sum), else redone in the reference's order
 * (csrc/ps_softmax_long_dev.h).  Process-wide (per loaded library: the default and the -DPS_CONTRACT build count their own launches), since the last reset;
 * waits for the devices that ran such a kernel. */
void ps_hip_softmax_long_counters(uint64_t *out2, int reset);
void ps_hip_model_destroy(ps_hip_model *m);
/* KVCacheInterface bookkeeping (core/kv_cache.hpp:97-163) */
size_t ps_hip_model_kv_position(const ps_hip_model *m);
int ps_hip_model_max_batch(const ps_hip_model *m); /* widest forward the model's buffers hold (ps_model_desc::max_batch) */
int ps_hip_model_kv_truncate(ps_hip_model *m, size_t n_tokens);
int ps_hip_model_kv_advance(ps_hip_model *m, size_t n_tokens); /* after an op-by-op forward through the ps_hip_* operators */
int ps_hip_model_kv_rollback(ps_hip_model *m, size_t n_tokens);
int ps_hip_model_kv_move(ps_hip_model *m, size_t dst_index, size_t src_index);
/* The rest of KVCacheInterface (core/kv_cache.hpp:120-162).  The reference keeps a forward's K / V rows in a per-batch staging area
 * (GGMLKV::chunk.current_k / current_v) and copies them into the cache afterwards; here every forward writes its rows straight into
 * the cache slots kv_position + i (norm_attention.cpp:82-104 does the same through VIEW + COPY on the ggml path), so "token i of the
 * last batch" IS cache slot kv_position + i:
 *   copy(dst_cache_index, src_token_index)  = move(dst_cache_index, kv_position + src_token_index)
 *   save_tokens(n)                          = nothing left to copy (checks kv_position + n <= n_ctx like the reference's assert)
 *   unmask_tokens(n)                        = slots kv_position .. kv_position + n - 1 visible again; the position is not modified
 *   append_tokens(n)                        = save_tokens + unmask_tokens + advance_tokens; returns 0 and the OLD position in *old_position
 *                                             (may be NULL) */
int ps_hip_model_kv_copy(ps_hip_model *m, size_t dst_cache_index, size_t src_token_index);
int ps_hip_model_kv_save_tokens(ps_hip_model *m, size_t n_tokens);
int ps_hip_model_kv_unmask_tokens(ps_hip_model *m, size_t n_tokens);
int ps_hip_model_kv_append_tokens(ps_hip_model *m, size_t n_tokens, size_t *old_position);
/* One Model::forward (model/llama/llama_model.cpp:52-117).  tokens/pos: HOST arrays of n entries,
 * positions consecutive from pos[0].  tree (may be NULL): bs x bs attention mask among the batch tokens
 * (speculative tree verify).  lm_head != 0: logits for all n tokens are left in the model's device buffer
 * (ps_hip_model_logits) and their arg-max ids are written to argmax_host (may be NULL).  Advances the KV
 * position by n (m_kv->advance, llama_model.cpp:109). */
int ps_hip_model_forward(ps_hip_model *m, const int32_t *tokens, int n, const int32_t *pos, const uint8_t *tree,
                         int lm_head, int32_t *argmax_host);
/* The same launches as ps_hip_model_forward, for a graph that HIPBackend::plan lowered (src/executor/executor.cpp:47-49,79:
 * the whole op vector goes to the backend's plan() before it runs): enqueues only -- no host sync, the KV position is left
 * to the caller (LlamaModel::forward advances it after Executor::run, llama_model.cpp:109).  The result counts once
 * ps_hip_model_kv_advance or ps_hip_model_sync_check has returned 0. */
int ps_hip_model_forward_lowered(ps_hip_model *m, const int32_t *tokens, int n, const int32_t *pos, const uint8_t *tree, int lm_head);
/* Waits for a pending ps_hip_model_forward_lowered and looks at the one-launch attention's time-out flag (k_attn.hip: its
 * workgroups wait for each other inside the launch, bounded).  0: the result is valid.  PS_HIP_ATTN_TIMEOUT: it is not -- the model
 * has switched to the two-launch attention (sticky, see ps_hip_model_set_mode) and the caller runs the forward again, once (nothing
 * was advanced; behind the switch a forward cannot time out).  1: a HIP error -- not a time-out, do not retry.
 * ps_hip_model_kv_advance calls it, and so does every other model entry point before it enqueues anything, so an unconsumed lowered
 * forward's time-out is reported to the caller that still holds its inputs instead of being pinned on the next forward. */
int ps_hip_model_sync_check(ps_hip_model *m);
/* ModelTokenIterator's prefill loop (src/model/model.hpp:147-163: forward(chunk, lm_head = false) + advance, chunk after chunk of
 * `chunk` tokens = hparams batch_size) for tokens appended at the current cache position -- bit-identical to calling
 * ps_hip_model_forward per chunk, but up to max_batch / chunk chunks share one launch sequence: the mat-muls take all their columns at
 * once, only the attention is evaluated per reference chunk (its sums depend on where a chunk ends). */
int ps_hip_model_prefill(ps_hip_model *m, const int32_t *tokens, int n, int chunk);
/* Token-tree forward (speculative verify / draft, src/speculative/token_tree.cpp): the n tokens are appended at the
 * cache slots kv_position .. kv_position+n-1, column i is rotated with RoPE position rope_pos[i] (its depth in the tree,
 * not its slot) and sees the cached prefix (minus slots hidden with ps_hip_model_kv_mask) plus the batch columns j with
 * tree[i*n + j] != 0 (NULL: causal).  advance = 0 leaves kv_position where it was: the caller keeps the accepted path
 * with ps_hip_model_kv_move(dst, src) + ps_hip_model_kv_advance(1) per node, as TokenTree::verify does. */
int ps_hip_model_forward_tree(ps_hip_model *m, const int32_t *tokens, int n, const int32_t *rope_pos, const uint8_t *tree,
                              int lm_head, int32_t *argmax_host, int advance);
/* KVCacheInterface::mask / unmask (core/kv_cache.hpp:97-163): hide / show one cached slot in every later forward */
int ps_hip_model_kv_mask(ps_hip_model *m, size_t index, int visible);
/* Greedy single-token steps, the decode hot loop (model/model.hpp:170-183): feeds `token` at the current
 * KV position, then its own arg-max, `steps` times, without host round trips (hipGraph replay).  out_ids
 * HOST int32[steps]. */
int ps_hip_model_decode_greedy(ps_hip_model *m, int32_t token, int steps, int32_t *out_ids);

/* ---- sampled decoding on the device: the standard sampler chain (repeat penalty / EOS ban -> top-k -> temperature -> soft-max ->
 * top-p -> normalize -> std::mt19937 + std::discrete_distribution), token for token what the host SamplerChain (csrc/host/sampler.cpp)
 * draws from the same logits, configuration and engine state (DESIGN.md "Sampled decode on the device").
 * Covered: 1 <= top_k <= PS_SAMPLE_K_MAX, top_k < n_vocab, temperature > 0, at most PS_SAMPLE_WINDOW_MAX window entries;
 * anything else is refused (rc 2), never served some other way. */
#define PS_SAMPLE_K_MAX 256
#define PS_SAMPLE_WINDOW_MAX 1024
typedef struct ps_sample_cfg { /* the fields of the host's psh_sampler_cfg except the seed */
    float temperature, top_p;
    uint64_t top_k;
    int32_t penalty_last_n;
    float penalty_repeat, penalty_freq, penalty_present;
    int32_t penalize_nl, ignore_eos, n_vocabs, special_eos_id, linefeed_id;
} ps_sample_cfg;
typedef struct ps_sample_state {
    uint32_t mt[624];       /* std::mt19937's words and position (what libstdc++'s operator<< writes) */
    uint32_t mt_pos;
    int32_t n_window;       /* the counted repeat-penalty window: history[0 .. min(last_n, size)) (fixed for a whole run) */
    int32_t window[PS_SAMPLE_WINDOW_MAX];
    uint64_t n_outputs;     /* engine outputs consumed, accumulated */
    uint64_t n_exact;       /* steps whose top-k took the exact libstdc++ heap path (ties / NaN), accumulated */
} ps_sample_state;
/* 0: the configuration is covered for this vocabulary size */
int ps_hip_sample_covered(const ps_sample_cfg *cfg, int n_vocab, const ps_sample_state *state);
/* one step on caller logits (device float[n_vocab]): *token_out (host) = the drawn token, *state advanced */
int ps_hip_sample(ps_hip_ctx *ctx, const float *logits_dev, int n_vocab, const ps_sample_cfg *cfg, ps_sample_state *state, int32_t *token_out);
/* ps_hip_sample for `rows` rows of caller logits in one pair of launches: row r at logits_dev + r * row_stride (floats, row_stride >= n_vocab; any alignment),
 * its own cfgs[r] / states[r]; tokens_out HOST int32[rows].  1 <= rows <= 16.  Row r draws what ps_hip_sample draws on that row alone, and states[r] advances
 * the same way.  A row whose configuration is not covered refuses the whole call (rc 2, the message names the row, no state modified). */
int ps_hip_sample_rows(ps_hip_ctx *ctx, const float *logits_dev, int n_vocab, int64_t row_stride, int rows,
                       const ps_sample_cfg *cfgs, ps_sample_state *states, int32_t *tokens_out);
/* ps_hip_model_decode_greedy with the drawn token in place of the arg-max: its own captured step (dropped where the greedy one is),
 * eager in mode bit 0, hidden slots refused, one retry from the start state after an attention time-out.  *state advanced. */
int ps_hip_model_decode_sampled(ps_hip_model *m, int32_t token, int steps, const ps_sample_cfg *cfg, ps_sample_state *state, int32_t *out_ids);
/* diagnostics: [0] exact-path steps, [1] engine outputs, process-wide since the last reset (reset != 0 clears after reading) */
void ps_hip_sample_counters(uint64_t *out2, int reset);
const char *ps_hip_last_sample_kernels(void);

/* ---- scoring a text on the device: the probability the model gives each target token, as the reference's perplexity tool computes it
 * (app/perplexity/main.cpp:50-61 over ProbArray::softmax, src/sampler/prob_array.cpp:38-59: max, expf(x - max), a double sum from the
 * smallest logit to the largest, (float)((double)e_t / sum)), bit for bit (DESIGN.md "Scoring a text on the device").  The device adds in an
 * order of its own and certifies each row's prob; a row whose certificate does not close is redone on the host with the reference's own
 * operations (flag bit 0).  log and exp of the perplexity stay with the caller (csrc/host/perplexity.hpp), on the host's libm like the reference's. */
typedef struct ps_score {
    float prob;       /* of the row's target; NaN with flag bit 1 or 2 */
    float max_logit;
    int32_t argmax;   /* the first maximum, as ps_hip_argmax gives it */
    uint32_t flags;   /* bit 0: took the exact path; bit 1: the row holds a NaN or a +inf (outside the contract, nothing scored); bit 2: no target */
} ps_score;
/* rows of n_vocab logits on the device, row r at logits_dev + r * row_stride (floats; any alignment); targets_host[r] in [-1, n_vocab), -1 = score nothing
 * (flag bit 2; argmax and max_logit still returned); out_host: rows records.  2 <= n_vocab <= 2^24; anything else is rc 2. */
int ps_hip_score_rows(ps_hip_ctx *ctx, const float *logits_dev, int n_vocab, int64_t row_stride, int rows, const int32_t *targets_host, ps_score *out_host);
/* ps_hip_model_prefill(m, tokens, n, chunk) -- same cache rows, same position afterwards, same retry -- that also runs the lm_head for every column and scores
 * column i against targets[i] (out_host: n records).  The logits are bit-identical to ps_hip_model_forward(chunk tokens, lm_head = 1) called once per chunk
 * (app/perplexity/main.cpp:113-121); up to max_batch / chunk chunks share a launch sequence as in prefill (in the fp16-KV mode, bit 3, chunks of one token
 * run one at a time: that mode's attention exists for single-token forwards only).  Refused with rc 2 and nothing advanced: what prefill refuses, a target
 * outside [-1, vocab), and the fp16 prefill perf mode (bit 5), whose definition excludes batches with logits. */
int ps_hip_model_score(ps_hip_model *m, const int32_t *tokens, const int32_t *targets, int n, int chunk, ps_score *out_host);
/* diagnostics: [0] rows scored, [1] of them on the exact path, [2] rows refused for a NaN / +inf, process-wide since the last reset */
void ps_hip_score_counters(uint64_t *out3, int reset);

/* ---- Sequences: several conversations on one model, decoded together (DESIGN.md "Batched decode").
 * A model holds one or more sequences: a KV cache (K [n_ctx][kv_dim], V [kv_dim][n_ctx] per layer), a position and a visibility table each.  Sequence 0
 * is the cache ps_hip_model_create allocated; a model on which none of these is called behaves exactly as before.  One sequence is the CURRENT one: every
 * single-sequence entry point above and below (forward, forward_lowered, prefill, forward_tree, decode_greedy, decode_sampled, kv_*, kv_position, k_cache /
 * v_cache) works on it -- a prompt gets into sequence s by seq_select(s) + prefill.  Switching drops the captured single-token steps (they hold cache pointers).
 * seq_reserve: the model holds n_seq sequences afterwards (growing only: fewer than it has is rc 2); rc 1 = out of device memory, the model unchanged.
 * seq_position: (size_t)-1 for an id out of range. */
int ps_hip_model_seq_reserve(ps_hip_model *m, int n_seq);
int ps_hip_model_seq_count(const ps_hip_model *m);
size_t ps_hip_model_seq_position(const ps_hip_model *m, int seq);
int ps_hip_model_seq_select(ps_hip_model *m, int seq);
/* One decode step of n sequences: column i feeds tokens[i] to sequence seq_ids[i] at that sequence's position, appends its K / V there, attends over
 * that sequence's cache only and advances that sequence by one.  Row i of ps_hip_model_logits is column i's logits (lm_head != 0), argmax_host (optional,
 * HOST int32[n]) its arg-max.  Column i is bit-identical to ps_hip_model_forward of that token on a one-sequence model with the same history, whoever else
 * is in the batch.  1 <= n <= min(16, max_batch), ids distinct and < seq_count, every position < n_ctx, no hidden slot (kv_mask) in a participating
 * sequence, not in the fp16-KV mode (mode bit 3): anything else is rc 2 with nothing advanced. */
int ps_hip_model_decode_batch(ps_hip_model *m, const int32_t *seq_ids, const int32_t *tokens, int n, int lm_head, int32_t *argmax_host);
/* `steps` such steps, each column fed its own arg-max, without a host round trip per step.  out_ids HOST int32[steps][n]. */
int ps_hip_model_decode_batch_greedy(ps_hip_model *m, const int32_t *seq_ids, const int32_t *tokens, int n, int steps, int32_t *out_ids);
/* ps_hip_model_decode_batch_greedy with column i fed the token its own chain drew: cfgs / states are arrays of n entries (column i: cfgs[i], states[i]);
 * out_ids HOST int32[steps][n]; states advanced.  Column i is, id for id, what ps_hip_model_decode_sampled draws on a one-sequence model with the same history,
 * first token, cfgs[i] and start state states[i], whoever else is in the batch and whatever their configurations (DESIGN.md "Sampled batched decode").
 * rc 2, nothing advanced and no state modified (the message names the column): what decode_batch_greedy refuses, a null pointer, a column whose configuration
 * ps_hip_sample_covered refuses for the model's vocabulary.  steps <= 0: 0, nothing changed. */
int ps_hip_model_decode_batch_sampled(ps_hip_model *m, const int32_t *seq_ids, const int32_t *tokens, int n, int steps,
                                      const ps_sample_cfg *cfgs, ps_sample_state *states, int32_t *out_ids);
/* Fork (DESIGN.md "Fork, save and restore").  A forward only writes slots at or behind the position, so a prefix of one sequence is, bit for bit, a valid prefix of
 * another: one prefill serves every conversation behind the same system prompt and every one of n / best_of completions.
 * dst sequences get slots [0, n_tokens) of src's K / V in every layer; their position becomes n_tokens, all their slots visible.  Afterwards each destination behaves in
 * every entry point (single-sequence calls after seq_select, decode_batch, decode_batch_greedy, forward_tree, score, the captured decode steps) bit for bit like a
 * sequence that had src's history of n_tokens tokens.  One launch for all layers and up to 15 destinations (csrc/k_seqcopy.hip); src is not modified; slots >= n_tokens
 * of a destination keep their bytes; n_tokens == 0 empties the destinations; src or a destination may be the current sequence.
 * rc 2, nothing changed: n_dst outside 1 .. seq_count - 1, an id out of range, a destination equal to src or listed twice, n_tokens > src's position, src with hidden
 * slots (kv_mask).  (A long-window or fp16-KV model holds one sequence: the id checks refuse it.) */
int ps_hip_model_seq_fork(ps_hip_model *m, int src_seq, const int32_t *dst_seqs, int n_dst, size_t n_tokens);
/* Save / restore.  The state of a sequence's first n_tokens slots as a host blob that does not depend on n_ctx: a 64-byte little-endian header ("PSKV", version 1,
 * n_layers, kv_dim, head_size, n_tokens u64, the writer's ps_hip_build_contract(), zeros; csrc/ps_kv_state.h), then per layer K [n_tokens][kv_dim] f32 and
 * V [kv_dim][n_tokens] f32: seq_state_bytes = 64 + n_layers * 2 * n_tokens * kv_dim * 4.  A blob restores into a sequence of any model with the same n_layers,
 * kv_dim, head_size and build -- another window, another max_batch, a long-window model.  THE BLOB DOES NOT IDENTIFY THE WEIGHTS: keeping a state with the model
 * it was computed by is the caller's responsibility.
 * seq_export refuses (rc 2): an id out of range, n_tokens > the sequence's position, hidden slots, bytes < seq_state_bytes(n_tokens), mode bit 3.
 * seq_import sets the position to the header's n_tokens with all slots visible; slots beyond stay as they are.  It refuses (rc 2, nothing changed): an id out of range,
 * a bad magic, version or contract flag, another n_layers / kv_dim / head_size, n_tokens > n_ctx, bytes != what the header implies, mode bit 3. */
size_t ps_hip_model_seq_state_bytes(const ps_hip_model *m, size_t n_tokens);
int ps_hip_model_seq_export(ps_hip_model *m, int seq, size_t n_tokens, void *host_buf, size_t bytes);
int ps_hip_model_seq_import(ps_hip_model *m, int seq, const void *host_buf, size_t bytes);

const float *ps_hip_model_logits(const ps_hip_model *m); /* device [max_batch][vocab] */
/* Arg-max ids of the most recent forward with lm_head (first maximum per token, what greedy_sample / TopK(1) returns: src/sampler/prob_array.cpp:65-67,
 * sampler.cpp:39-56), computed on the device behind the lm_head: 4 bytes per token come to the host instead of vocab x 4 (513 KB for 128 256 logits,
 * src/model/model.hpp:170-183).  For a lowered forward call it after ps_hip_model_sync_check / ps_hip_model_kv_advance: the ids have then already arrived
 * in pinned memory behind the forward's launches and the call does not wait on the stream again (one wait per decode step on the op-API path). */
int ps_hip_model_argmax(ps_hip_model *m, int n, int32_t *ids_host);
/* diagnostics: device scratch tensors of the most recent forward, last layer (0 x, 1 q, 2 att, 3 ffn hidden, 4 scores) */
const float *ps_hip_model_scratch(const ps_hip_model *m, int which);
const float *ps_hip_model_k_cache(const ps_hip_model *m, int layer);
const float *ps_hip_model_v_cache(const ps_hip_model *m, int layer);
/* per-forward accounting for the roofline: GGUF bytes of all mat-mul weights streamed by one token */
uint64_t ps_hip_model_weight_bytes_per_token(const ps_hip_model *m);
/* Measurement helper (bench.py roofline): replays mat-vec launches of one single-token forward exactly as the decode
 * step issues them (same kernels and fused prologues, every layer's own weights) `reps` times between HIP events on
 * the ctx stream -> seq_ms per token.  which = 0: all quantized mat-vecs; 1: the gate/up launch of every layer only.
* (which: 0 every quantized mat-vec of a token, 1 gate/up, 2 QKV, 3 O, 4 down, 5 lm_head)
 * null_ms = the same number of empty launches (launch-boundary cost); n_launches = launches per token. */
int ps_hip_model_bench_gemv(ps_hip_model *m, int reps, int which, double *seq_ms, double *null_ms, int *n_launches);
/* the same replay with bs activation columns (a prefill chunk's mat-muls with their quantizer launches) */
int ps_hip_model_bench_matmul(ps_hip_model *m, int reps, int which, int bs, double *seq_ms, double *null_ms, int *n_launches);
/* Diagnostic: in-kernel timeline of the decode mat-vec (tools/gpu_timeline.py).  With host_out == NULL, arm
 * (key >= 0: record launches with epilogue*4 + prologue == key; key < 0: disarm).  With host_out != NULL, copy
 * the last recorded launch: n_words uint64 = [workgroup][role 0 producer wave 0 / 1 chain wave][32 events],
 * shader-clock ticks (s_memtime).  key = k1 + 100 * (k2 + 1) records a second launch family into a second block of
 * the same size (kernel-boundary gaps). */
/* diagnostics: the kernel (rocprofv3's template name) the most recent quantized mat-mul launch of this process went to */
const char *ps_hip_last_matmul_kernel(void);
/* diagnostics: the single-token attention the most recent single-token forward of this process enqueued (rocprofv3's template name):
 * (a long-window model: "attn_scores_kernel<NV> + attn_softmax_long_kernel + attn_pv_long_kernel<KVS>" below 8 columns, "attn_scores_mfma_kernel<NV> + attn_softmax_long_kernel + attn_pv_mfma" from 8 on, noted by every forward)
 * "qkv_attn_kernel<NV, KVS>" (fused with the Q / K / V mat-vec), "attn_decode2_kernel<NV, NT, KVS>" (one launch), "attn_scores_kernel<NV> + attn_softmax_pv_kernel"
 * (two launches, mode bit 4) or "attn_flash16_kernel<HS>" (fp16-KV decode mode, bit 3); "" before any.  Noted at enqueue time: after a captured step's
 * replay it names what the capture enqueued. */
const char *ps_hip_last_attention_kernel(void);
int ps_hip_debug_timeline(ps_hip_ctx *ctx, int key, uint64_t *host_out, int n_words);
/* Diagnostic: tunables of the library (process-wide).  (Keys 1 and 2 selected wave configurations of the decode mat-vec that are no longer compiled, key 6 the column blocks per XCD of the wide Q4_K / Q5_K
 * mat-mul's item order, a constant now (k_gemm4k.hip G4K_CBX): unknown keys.)
 * key 3: the narrow-batch Q4_K mat-mul for few row tiles (k_gemm4k.hip: 0 = gemm4k_par_kernel off (the wave-per-tile / staged forms take the launch: A/B only),
 * 4 / 8 = gemm4k_par_kernel with that many waves per tile, 1 = by tile count, the default); key 4: the fp16 perf mode's GEMM (perf16.hip:
 * 0 = by shape, 1 = 128-token tiles, 2 = 256 x 256 tiles); key 5: the next `value` single-token forwards on the one-launch attention
 * report a time-out of its score exchange (tests of the retry paths: forward, forward_tree, prefill tail, decode_greedy, lowered forward +
 * kv_advance); key 7: 1 = the fused Q / K / V + attention launch (k_qkvattn.hip) wherever it is covered -- by default only where its grid fills three quarters
 * of the chip (head size 128 with 8 kv heads), the head-size-64 instance otherwise runs under test only; key 9: the single-token attention kernels read the cached K rows / V channels
 * with plain (0) or non-temporal (1) loads whatever the cache's size, -1 (default): by the rule of csrc/model.hip (a cache-policy hint: no result bit depends on it); key 10: F16 batches on the matrix cores (0, default) or on the VALU chain kernel (1: A/B only, same bits);
 * key 11: the fused launch's first rendezvous on tagged granules (0, default) or on the counter (1: A/B and fallback);
 * key 12: the scoring certificate's eps (csrc/ps_score_dev.h) multiplied by 2^value, 0 <= value <= 100 (default 0; tests and A/B only: eps >= 1 sends every row down the exact path).
 * key 13: long-window models, positions per LDS tile of attn_pv_long_kernel: a multiple of 32 up to 2048, 0 = the default (2048); read at enqueue time (tests: several tiles at a small window);
 * key 14: the long soft-max's row-sum certificate, eps (csrc/ps_softmax_long_dev.h) multiplied by 2^value, 0 <= value <= 100 (default 0; tests: at 100 every row takes the sequential sum).
 * Returns non-zero for an unknown key.  (A captured single-token step keeps the launch plan it was captured with: ps_hip_model_set_mode drops it.) */
int ps_hip_debug_set(int key, int value);
/* Diagnostic: one GEMM shape of the fp16 perf mode on synthetic operands (tools/f16_gemm_bench.py): out[M][N] = x[M][K] . W[N][K]^T, timed over
 * `reps` launches (with beta: out = beta out + ...), max |difference| to a k-ordered fp32 reference (beta != 0: of a second launch on top of
 * the first result against (1 + beta) x the reference). */
int ps_hip_debug_f16_gemm(ps_hip_ctx *ctx, int M, int64_t N, int64_t K, int reps, float beta, double *us_per_launch, double *max_abs_err);
/* bit 0: 0 = hipGraph replay of the decode step (default), 1 = eager launches (rocprofv3 needs them);
 * bits 1, 2: unused (round 1 / 2 experiments, removed);
 * bit 3: 1 = fp16-KV decode mode — NOT bit-exact: K and V are mirrored in fp16 as they are appended and the
 * single-token attention reads only the mirrors (half the KV bytes) with a split-KV online soft-max; prefill, batches and
 * tree verify keep reading the FP32 caches.  Must be switched on while the cache is empty (position 0).;
 * bit 4: 1 = single-token attention as TWO launches (scores, then soft-max + V.p) instead of the one-launch form
 * (attn_decode2_kernel: scores exchanged inside the launch; it needs every workgroup of its grid resident, its wait is bounded,
 * and a wait that gives up switches this bit on: the forward that hit it runs again on the two launches -- ps_hip_model_forward,
 * _forward_tree, _prefill and _decode_greedy do that themselves, a lowered forward reports it through ps_hip_model_sync_check /
 * ps_hip_model_kv_advance).  Same results bit for bit.  Sticky after a time-out: a later set_mode without bit 4 keeps the two launches;
 * bit 6 (write-only): re-arm the one-launch attention after a time-out (clears the sticky state, then the other bits apply);
 * bit 5: 1 = fp16 prefill perf mode — NOT bit-exact: the layer mat-muls of batches without logits (prefill chunks) run
 * as dense fp16 GEMMs (fp32 accumulation) on dequantized fp16 copies of the matrices made at first use (+2 bytes per weight), the
 * backend's own matrix-core kernel (csrc/perf16.hip; row lengths must be multiples of 64); RoPE, KV append and attention stay the parity kernels on
 * the FP32 cache, single tokens and tree forwards stay entirely on the parity path.
 * bit 7: 1 = the head of a single-token layer as TWO launches (Q / K / V mat-vec with RoPE + KV append, then the one-launch attention) instead of the fused
 * qkv_attn_kernel (k_qkvattn.hip, round 6: four launches per decode layer where the shape is covered).  Same results bit for bit; bit 4 implies it
 * (the fused launch contains the one-launch attention's exchange, its time-out is the same flag and the same fallback).
 * The environment variable PS_HIP_MODE_OR is OR-ed into every mode (A/B runs of unmodified drivers). */
int ps_hip_model_set_mode(ps_hip_model *m, int mode);

#ifdef __cplusplus
}
#endif
#endif /* PS_HIP_H */
