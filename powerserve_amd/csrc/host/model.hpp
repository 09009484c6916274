// Model layer: weights, graph builders and the token loop, mirroring
//   Weight / LayerWeights        src/model/common/weights.hpp:24-74, llama_weight.hpp:24-34, qwen2_weight.hpp:24-37
//   NormAttention::build          src/model/module/norm_attention.cpp:26-160
//   FFN::build                    src/model/module/ffn.cpp:22-42
//   LlamaModel / Qwen2Model       src/model/llama/llama_model.cpp:52-132, src/model/qwen2/qwen2_model.cpp:75
//   ModelTokenIterator            src/model/model.hpp:117-184
//   load_model                    src/model/model_loader.cpp:23-41
#pragma once
#include <set>
#include "hip_backend.hpp"
#include "sampler.hpp"

#include <deque>
#include <span>

namespace powerserve {

struct LayerWeights {
    Tensor attn_norm, ffn_norm, attn_q, attn_k, attn_v, attn_output, ffn_gate, ffn_up, ffn_down, attn_q_bias, attn_k_bias, attn_v_bias;
};
struct Weight {
    Tensor token_embedding_table, output_weight, rms_final_weight;
    std::vector<LayerWeights> lw;
    bool tied = false;
};

struct LogitsVector { // src/model/model.hpp:27-39
    BufferPtr buffer;
    std::vector<std::span<const float>> logits_vector;
    LogitsVector() = default;
    LogitsVector(BufferPtr buf, size_t vocab_size, size_t batch_size) : buffer(buf) {
        const float *l = static_cast<const float *>(dynamic_cast<CPUBuffer &>(*buffer).m_data);
        for (size_t i = 0; i < batch_size; i++, l += vocab_size) logits_vector.emplace_back(l, l + vocab_size);
    }
};

struct NormAttention {
    const ModelConfig::LLMConfig &m_config;
    std::shared_ptr<Weight> m_weights;
    NormAttention(const ModelConfig::LLMConfig &c, std::shared_ptr<Weight> w) : m_config(c), m_weights(std::move(w)) {}
    TensorNode *build(Graph &g, TensorNode *x, int64_t L, const TensorNode *k_cache, const TensorNode *v_cache, const std::vector<int> &pos,
                      const CausalAttentionMask &mask, bool is_need_bias = false);
};
struct FFN {
    const ModelConfig::LLMConfig &m_config;
    std::shared_ptr<Weight> m_weights;
    FFN(const ModelConfig::LLMConfig &c, std::shared_ptr<Weight> w) : m_config(c), m_weights(std::move(w)) {}
    TensorNode *build(Graph &g, TensorNode *attn_o, int64_t L);
};

struct Model {
    std::string m_filename;
    std::shared_ptr<ModelConfig> m_config;
    std::shared_ptr<Weight> m_weights;
    std::shared_ptr<NormAttention> m_attn;
    std::shared_ptr<FFN> m_ffn;
    std::shared_ptr<Platform> m_platform;
    bool m_is_need_bias = false; // Qwen2
    bool m_use_plan_cache = true;  // a (batch size, lm_head) shape whose graph has been lowered once runs its launches without a second graph (false: every forward builds + plans)
    std::set<std::pair<size_t, bool>> m_lowered_shapes;
    int n_plan_cache_hits = 0;
    bool m_use_fused    = true;  // HIPBackend::plan lowers the canonical graph to the fused launches; false: op-by-op (A/B, tests)
    bool m_device_sampling = true; // generate(.., SamplerChain &): a standard chain the device covers runs inside the captured step; false: the host loop

    Model(const std::string &model_dir, const std::shared_ptr<ModelConfig> &config, const std::shared_ptr<Platform> &platform, int device,
          size_t max_batch, bool long_window = false);
    virtual ~Model();

    // one forward over `tokens` at consecutive positions `pos`; lm_head: logits for every token
    auto forward(const std::vector<int> &tokens, const std::vector<int> &pos, const CausalAttentionMask &mask, bool lm_head = true) -> LogitsVector;
    // greedy (top_k = 1 == arg-max, src/sampler/prob_array.cpp:65-67).  A lowered graph returns the device arg-max (4 bytes per token come to the host,
    // the logits stay on the GPU: SURVEY a21); an op-by-op graph copies the logits and takes the first maximum on the host like the reference.
    auto decode(const std::vector<Token> &tokens, const std::vector<int> &pos, bool lm_head) -> std::vector<Token>;
    // ModelTokenIterator's prefill loop (src/model/model.hpp:147-163): forward(chunk of batch_size tokens, lm_head = false) + advance, chunk after chunk, for
    // tokens appended at the cache position.  The first chunk's graph goes through Executor::plan like any forward; when the backend lowers it, the LOOP is
    // lowered too (ps_hip_model_prefill: the same bits, several reference chunks per launch sequence), else every chunk runs through forward().
    void prefill(const std::vector<Token> &tokens, size_t batch_size);
    // prefill that also scores: tokens appended at the cache position in chunks of batch_size with the lm_head for every column, record i = the probability the
    // model gives targets[i] behind tokens[0 .. i] (-1: none), bit for bit what the reference's perplexity tool computes (ps_hip_model_score; csrc/host/perplexity.cpp)
    auto score(const std::vector<Token> &tokens, const std::vector<Token> &targets, size_t batch_size) -> std::vector<ps_score>;
    // ModelTokenIterator: prefill all but the last prompt token in chunks of batch_size (no lm_head), then `steps`
    // single-token greedy steps
    auto generate(const std::vector<Token> &prompt, int steps, size_t batch_size) -> std::vector<Token>;
    // the same loop with a sampler chain instead of arg-max: logits come back to the host every step (model.hpp:170-183)
    auto generate(const std::vector<Token> &prompt, int steps, size_t batch_size, SamplerChain &sampler) -> std::vector<Token>;

    // ---- sequences: several conversations on one model, decoded together.  The reference's KVCacheInterface has no notion of a sequence (its server keeps a
    // session map over a one-cache model, app/server/server_handler.hpp), so this extends the facade; it is not a lowering of a reference graph.
    // The CURRENT sequence is what forward / decode / prefill / generate and the platform's KV position work on.
    void reserve_sequences(size_t n_seq);
    void select_sequence(size_t seq);
    size_t sequence_count();
    size_t sequence_position(size_t seq);
    // one greedy step: tokens[i] goes to sequence seq_ids[i] at that sequence's position and advances it; returns the arg-max id per column.
    // logits_out (optional): host [n][vocab] logits of the columns
    auto decode_batch(const std::vector<int> &seq_ids, const std::vector<Token> &tokens, float *logits_out = nullptr) -> std::vector<Token>;
    // `steps` batched steps, column i fed the token samplers[i] drew from its logits; returns the ids [steps][n], row after row.  Standard chains the device covers
    // (device_sampler_state) run on the device in one call (ps_hip_model_decode_batch_sampled) and take their ids (accept) and engines back; one chain that is
    // not, or m_device_sampling off, and the whole call is the host loop: decode_batch with the logits to the host, sample per row.  Same ids, same chains afterwards
    auto decode_batch_sampled(const std::vector<int> &seq_ids, const std::vector<Token> &tokens, int steps, const std::vector<SamplerChain *> &samplers)
        -> std::vector<Token>;
    // fork: the first n_tokens slots of sequence src become the history of every sequence of dsts (ps_hip_model_seq_fork: one launch, src untouched) -- one prefill
    // of a shared system prompt, or of the prompt of n / best_of completions (app/server/openai_api.hpp:122-123), serves them all
    void fork_sequence(size_t src, const std::vector<int> &dsts, size_t n_tokens);
    // save / restore: a sequence's first n_tokens slots as a host blob independent of n_ctx (ps_hip_model_seq_export / _import; csrc/ps_kv_state.h).  The blob
    // does not identify the weights.  import_sequence takes a blob of any compatible model (same layers, kv_dim, head_size and build)
    auto export_sequence(size_t seq, size_t n_tokens) -> std::vector<uint8_t>;
    void import_sequence(size_t seq, const void *blob, size_t bytes);

    hip::HIPBackend &backend() { return *m_platform->hip_backends[m_config->model_id]; }

private:
    std::unique_ptr<GGUFFile> m_gguf;
    std::vector<ps_weight *> m_dev_weights;
    std::vector<void *> m_dev_f32;
    // ids != nullptr (greedy callers): a lowered graph fills it from the device arg-max and returns no logits
    auto forward_graph(const std::vector<int> &tokens, const std::vector<int> &pos, const CausalAttentionMask &mask, bool lm_head,
                       std::vector<Token> *ids = nullptr, bool plan_only = false) -> LogitsVector;
    bool m_last_lowered = false; // the most recent forward_graph was lowered by HIPBackend::plan
};
using LlamaModel = Model;
using Qwen2Model = Model;

// long_window: a long-window device model (ps_hip_model_create_long): any n_ctx up to PS_HIP_LONG_CTX_MAX, attention rows in device memory, one sequence
auto load_model(const std::string &model_dir, const std::shared_ptr<Platform> &platform, int device = 0, size_t max_batch = 128, int n_ctx_cap = 0,
                bool long_window = false) -> std::shared_ptr<Model>;

// the device sampler's view of a standard chain (configuration, engine, fixed penalty window); false: not expressible
bool device_sampler_state(const SamplerChain &sampler, ps_sample_cfg &c, ps_sample_state &st);

} // namespace powerserve

// handle behind the C driver API (psh_model_*, psh_spec_*)
struct psh_model {
    std::shared_ptr<powerserve::Platform> platform;
    std::shared_ptr<powerserve::Model> model;
    std::string err;
};
