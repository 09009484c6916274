// The reference's PerplexityCalculator (app/perplexity/main.cpp:29-61) on per-token probabilities: its members and its update rule.  The reference's
// apply() takes the whole ProbArray, soft-maxes it and keeps the log of every entry; accept() then reads the target's.  Here the probability of the target alone
// arrives (ps_score::prob, the same float bit for bit: csrc/ps_score_dev.h), so apply() takes it and the target's id, and the log -- the same std::log on the
// same float -- lands in the same slot of log_logits.
#pragma once
#include "core.hpp"

#include <cmath>
#include <cstddef>
#include <vector>

namespace powerserve {

constexpr int PPL_START_ID = 18; // app/perplexity/main.cpp:27: scoring starts with this batch (counted from 1)

struct PerplexityCalculator {
    size_t n_tokens   = 0;
    float m_logit_sum = 0;
    std::vector<float> log_logits;
    size_t num_vocabs = 0;
    float current_ppl = 0;

    explicit PerplexityCalculator(size_t n_vocabs) : log_logits(n_vocabs), num_vocabs(n_vocabs) {}

    void apply(Token token, float prob) {
        log_logits[(size_t)token] = std::log(prob);
        n_tokens++;
    }
    void accept(Token token) {
        m_logit_sum += log_logits[(size_t)token];
        current_ppl = std::exp(-m_logit_sum / n_tokens);
    }
};

} // namespace powerserve
