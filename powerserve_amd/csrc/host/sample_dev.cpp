// CPU build of the device sampler's arithmetic (csrc/ps_sample_dev.h, the same source the kernels of csrc/k_sample.hip compile)
// and the C++ standard library's own counterparts, exported as psh_debug_* for tests/test_sampler_device_cpu.py; plus the
// façade's device-sampling switches.
#include "model.hpp"

#include "../ps_sample_dev.h"

#include <algorithm>
#include <map>
#include <random>
#include <sstream>

using namespace powerserve;

static void to_words(const std::mt19937 &e, ps_mt_state *s) {
    std::ostringstream os;
    os << e;
    std::istringstream is(os.str());
    for (uint32_t &w : s->x) is >> w;
    is >> s->p;
}
static void from_words(std::mt19937 &e, const ps_mt_state *s) {
    std::ostringstream os;
    for (uint32_t w : s->x) os << w << ' ';
    os << s->p;
    std::istringstream is(os.str());
    is >> e;
}

extern "C" void psh_set_error(const char *msg);
extern "C" {

// ---- ps_sample_dev.h, CPU build
void psh_debug_mt_seed(ps_mt_state *s, uint32_t seed) { ps_mt_seed(s, seed); }
void psh_debug_mt_next(ps_mt_state *s, int n, uint32_t *out) {
    for (int i = 0; i < n; i++) out[i] = ps_mt_next(s->x, &s->p);
}
int psh_debug_discrete(ps_mt_state *s, const float *w, int n, uint64_t *calls) {
    std::vector<double> cp((size_t)std::max(n, 1));
    return ps_discrete_draw(w, n, s->x, &s->p, cp.data(), calls);
}
void psh_debug_partial_sort(const float *v, int n, int k, float *out_v, int32_t *out_t) {
    std::vector<ps_pi> a((size_t)n);
    for (int i = 0; i < n; i++) a[(size_t)i] = ps_pi{v[i], i};
    ps_partial_sort(a.data(), k, n);
    for (int i = 0; i < k; i++) { out_v[i] = a[(size_t)i].v; out_t[i] = a[(size_t)i].t; }
}
// the whole chain as the device runs it (penalty, top-k by the heap path, tail, draw) on one row of logits; *state advanced
int32_t psh_debug_chain(const ps_sample_cfg *c, ps_sample_state *st, const float *logits, int n) {
    std::vector<float> v(logits, logits + n);
    const int eos = (c->ignore_eos && c->special_eos_id >= 0) ? c->special_eos_id : -1;
    const int spare = (!c->penalize_nl && c->linefeed_id >= 0) ? c->linefeed_id : -1;
    if (eos >= 0 && eos < n) v[(size_t)eos] = -INFINITY;
    const bool active = c->penalty_last_n != 0 && !(c->penalty_repeat == 1.0f && c->penalty_freq == 0.0f && c->penalty_present == 0.0f);
    if (active) {
        std::map<int32_t, int> seen;
        for (int i = 0; i < st->n_window; i++)
            if (st->window[i] >= 0) seen[st->window[i]]++;
        for (auto &kv : seen)
            if (kv.first < n && kv.first != spare) v[(size_t)kv.first] = ps_penalize(v[(size_t)kv.first], kv.second, c->penalty_repeat, c->penalty_freq, c->penalty_present);
    }
    const int k = (int)c->top_k;
    std::vector<float> tv((size_t)k);
    std::vector<int32_t> tt((size_t)k);
    psh_debug_partial_sort(v.data(), n, k, tv.data(), tt.data());
    std::vector<double> cp((size_t)k);
    uint64_t calls = 0;
    const int idx = ps_sample_tail(tv.data(), k, c->temperature, c->top_p, st->mt, &st->mt_pos, cp.data(), &calls);
    st->n_outputs += calls;
    return tt[(size_t)idx];
}

// ---- the standard library itself
void psh_debug_std_mt(const ps_mt_state *in, int n, uint32_t *out, ps_mt_state *after) {
    std::mt19937 e;
    from_words(e, in);
    for (int i = 0; i < n; i++) out[i] = (uint32_t)e();
    to_words(e, after);
}
void psh_debug_std_mt_seed(ps_mt_state *s, uint32_t seed) { to_words(std::mt19937(seed), s); }
int psh_debug_std_discrete(ps_mt_state *s, const float *w, int n) { // ProbArray::stochastic_sample's construction
    std::mt19937 e;
    from_words(e, s);
    std::discrete_distribution<size_t> pick((size_t)n, 0, (double)n, [w](double x) { return w[(size_t)x]; });
    const int r = (int)pick(e);
    to_words(e, s);
    return r;
}
void psh_debug_std_partial_sort(const float *v, int n, int k, float *out_v, int32_t *out_t) {
    std::vector<ProbIndex> a((size_t)n);
    for (int i = 0; i < n; i++) a[(size_t)i] = ProbIndex{v[i], i};
    std::partial_sort(a.begin(), a.begin() + k, a.end(), std::greater<ProbIndex>());
    for (int i = 0; i < k; i++) { out_v[i] = a[(size_t)i].prob; out_t[i] = a[(size_t)i].token; }
}

// ---- façade: the chain's state as the device sampler takes it, and the switch of Model::generate
int psh_sampler_device_state(void *s, ps_sample_cfg *c, ps_sample_state *st) { return device_sampler_state(*(SamplerChain *)s, *c, *st) ? 0 : 1; }
void psh_sampler_engine_state(void *s, ps_mt_state *out) {
    std::istringstream is(((SamplerChain *)s)->engine_state());
    for (uint32_t &w : out->x) is >> w;
    is >> out->p;
}
int psh_sampler_is_standard(void *s) { return ((SamplerChain *)s)->standard() ? 1 : 0; }
// Model::generate(prompt, steps, batch, chain) with a chain the caller built (and may have extended)
int psh_model_generate_with_chain(void *h, const int32_t *prompt, int n_prompt, int batch_size, int steps, void *chain, int32_t *out) {
    try {
        auto r = ((psh_model *)h)->model->generate(std::vector<Token>(prompt, prompt + n_prompt), steps, (size_t)batch_size, *(SamplerChain *)chain);
        std::copy(r.begin(), r.end(), out);
        return 0;
    } catch (const std::exception &e) { psh_set_error(e.what()); return 1; }
}
// a plug-in stage that changes nothing (tests: a chain that is no longer the standard one)
void psh_sampler_append_noop(void *s) {
    struct Noop final : Sampler { void apply(ProbArray &) override {} };
    ((SamplerChain *)s)->append(std::make_shared<Noop>());
}

} // extern "C"
