// Model::score (the façade over ps_hip_model_score), the PerplexityCalculator's C driver, and the CPU builds of the scoring arithmetic
// (csrc/ps_score_dev.h, the same source the kernels of csrc/k_score.hip compile) exported as psh_debug_score_* for tests/test_score_cpu.py and of the long
// soft-max's row sum (csrc/ps_softmax_long_dev.h) exported as psh_debug_softmax_long_sum for tests/test_long_ctx_cpu.py.
#include "perplexity.hpp"

#include "model.hpp"

#include "../ps_score_dev.h"
#include "../ps_softmax_long_dev.h"

using namespace powerserve;

auto Model::score(const std::vector<Token> &tokens, const std::vector<Token> &targets, size_t batch_size) -> std::vector<ps_score> {
    POWERSERVE_ASSERT(tokens.size() == targets.size());
    POWERSERVE_ASSERT(batch_size > 0);
    std::vector<ps_score> out(tokens.size());
    if (tokens.empty()) return out;
    auto &be = backend();
    std::vector<int32_t> t(tokens.begin(), tokens.end()), g(targets.begin(), targets.end());
    if (ps_hip_model_score(be.m_model, t.data(), g.data(), (int)t.size(), (int)batch_size, out.data()))
        POWERSERVE_ABORT(std::string("score: ") + ps_hip_last_error(be.m_ctx));
    return out;
}

extern "C" void psh_set_error(const char *msg);
extern "C" {

int psh_model_score(void *h, const int32_t *tokens, const int32_t *targets, int n, int batch_size, ps_score *out) { // Model::score
    try {
        auto r = ((psh_model *)h)->model->score(std::vector<Token>(tokens, tokens + n), std::vector<Token>(targets, targets + n), (size_t)batch_size);
        std::copy(r.begin(), r.end(), out);
        return 0;
    } catch (const std::exception &e) { psh_set_error(e.what()); return 1; }
}

void *psh_ppl_create(int n_vocabs) { return new PerplexityCalculator((size_t)n_vocabs); }
void psh_ppl_destroy(void *p) { delete (PerplexityCalculator *)p; }
// apply + accept of one scored position (app/perplexity/main.cpp:125-126); returns current_ppl
float psh_ppl_add(void *p, int32_t token, float prob) {
    auto c = (PerplexityCalculator *)p;
    c->apply(token, prob);
    c->accept(token);
    return c->current_ppl;
}
float psh_ppl_current(void *p) { return ((PerplexityCalculator *)p)->current_ppl; }
float psh_ppl_logit_sum(void *p) { return ((PerplexityCalculator *)p)->m_logit_sum; }
int64_t psh_ppl_n_tokens(void *p) { return (int64_t)((PerplexityCalculator *)p)->n_tokens; }

// ---- ps_score_dev.h, CPU build
// ProbArray::softmax's own operations on one row: the target's probability
float psh_debug_score_row(const float *x, int n, int t) { return ps_score_row_exact(x, n, t); }
// the fast path as the device takes it (its order of additions, the certificate with eps x 2^shift): returns the flags, *prob the certified value (or, flagged,
// the uncertified quotient), *max_out / *argmax_out (optional) the first maximum
uint32_t psh_debug_score_certify(const float *x, int n, int t, int shift, float *prob, float *max_out, int32_t *argmax_out) {
    return ps_score_row_fast(x, n, t, shift, prob, max_out, argmax_out);
}

// ---- ps_softmax_long_dev.h, CPU build: one row of n soft-max numerators through the long kernels' row sum.  *inv_fast = (float)(1 / S), S summed by `lanes`
// lanes in an order of their own; *inv_seq = the reference's factor (its sequential sum).  Returns 1 when the certificate (eps x 2^shift) closed on S
int psh_debug_softmax_long_sum(const float *e, int n, int lanes, int shift, float *inv_fast, float *inv_seq) { return ps_sml_row(e, n, lanes, shift, inv_fast, inv_seq); }

} // extern "C"
