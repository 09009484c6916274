// The standard sampler chain on the device (include/ps_hip.h ps_hip_sample / ps_hip_model_decode_sampled; DESIGN.md "Sampled
// decode on the device").  Two launches behind the lm_head, both read everything from device buffers so that one captured
// step serves every configuration:
//   sample_slice_kernel  one workgroup per 512 logits: EOS ban + repeat penalty (the penalised row also goes to `pen`),
//                        the slice's top-(k+1) as 64-bit keys (value descending, token ascending), a NaN flag
//   sample_final_kernel  one workgroup: radix select of the k-th key over the slice lists, gather + sort of the k winners;
//                        when the k + 1 largest values are not pairwise distinct or a NaN is anywhere, std::partial_sort's
//                        own heap mechanics over `pen` instead (the exact path); then the chain's tail and the draw
//                        (ps_sample_dev.h) on the device-resident mt19937, and the decode bookkeeping of psl_argmax2
#include "ps_internal.h"
#include "ps_ops.h"
#include "ps_sample_dev.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <string>

namespace {

constexpr int SL = 512;      // logits per slice workgroup
constexpr int SL_NT = 256;
constexpr int FN_NT = 1024;  // final workgroup
constexpr int EX_PER = 8;    // exact path: logits per thread and chunk
constexpr int EX_CHUNK = FN_NT * EX_PER;
constexpr int DK_CAP = 12288; // candidate keys the final workgroup keeps in LDS (251 slices x 41 at k = 40); more are read from global memory

// float -> key that orders like the value (ascending), and back
__device__ __forceinline__ uint32_t fkey(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_val(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }
// 64-bit candidate key: ascending = value descending, then token ascending.  ~0: no candidate
__device__ __forceinline__ unsigned long long ckey(float v, int t) { return ((unsigned long long)~fkey(v) << 32) | (uint32_t)t; }
__device__ __forceinline__ float ckey_val(unsigned long long k) { return fkey_val(~(uint32_t)(k >> 32)); }

template <int N, int NT> __device__ void bitonic_sort_asc(unsigned long long *s) {
    for (int size = 2; size <= N; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < N / 2; t += NT) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const bool asc = (i & size) == 0;
                const unsigned long long a = s[i], b = s[j];
                if ((a > b) == asc) { s[i] = b; s[j] = a; }
            }
        }
    __syncthreads();
}

__global__ __launch_bounds__(SL_NT) void sample_slice_kernel(const float *logits, int n, const ps_sample_dev *d, float *pen, unsigned long long *cand, int *flags) {
    __shared__ float sv[SL];
    __shared__ unsigned long long sk[SL];
    __shared__ int snan;
    const int base = blockIdx.x * SL, tid = threadIdx.x, kp1 = d->k + 1, ban = d->ban_id, spare = d->spare_id;
    if (tid == 0) snan = 0;
    for (int j = tid; j < SL; j += SL_NT) {
        const int t = base + j;
        float v     = t < n ? logits[t] : 0.f;
        if (t == ban) v = -INFINITY;
        sv[j] = v;
    }
    __syncthreads();
    const float rep = d->repeat, fr = d->freq, pr = d->present;
    for (int j = tid; j < d->n_pen; j += SL_NT) { // the window's tokens are distinct: one writer per entry
        const int t = d->pen_tok[j];
        if (t >= base && t < base + SL && t < n && t != spare) sv[t - base] = ps_penalize(sv[t - base], d->pen_cnt[j], rep, fr, pr);
    }
    __syncthreads();
    int nan = 0;
    for (int j = tid; j < SL; j += SL_NT) {
        const int t = base + j;
        if (t < n) {
            const float v = sv[j];
            pen[t]        = v;
            nan |= v != v;
            sk[j] = ckey(v, t);
        } else {
            sk[j] = ~0ull;
        }
    }
    if (nan) snan = 1;
    bitonic_sort_asc<SL, SL_NT>(sk);
    for (int r = tid; r < kp1; r += SL_NT) cand[(size_t)blockIdx.x * kp1 + r] = sk[r];
    if (tid == 0) flags[blockIdx.x] = snan;
}

__device__ __forceinline__ unsigned wave_incl_scan(unsigned x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

__global__ __launch_bounds__(FN_NT) void sample_final_kernel(const unsigned long long *cand, const int *flags, int nwg, const float *pen, int n,
                                                             ps_sample_dev *d, int32_t *token_out, ps_step_state *st, int32_t *tokens, int32_t *ids) {
    __shared__ uint32_t smt[PS_MT_N];
    __shared__ unsigned hist[256];
    __shared__ unsigned long long sk[PS_SAMPLE_K_MAX];
    __shared__ ps_pi heap[PS_SAMPLE_K_MAX];
    __shared__ float tv[PS_SAMPLE_K_MAX];
    __shared__ int32_t tt[PS_SAMPLE_K_MAX];
    __shared__ double cp[PS_SAMPLE_K_MAX];
    __shared__ int surv[EX_CHUNK];
    __shared__ unsigned wsum[FN_NT / 64];
    __shared__ uint32_t sdk[DK_CAP];
    __shared__ double s_sum;
    __shared__ int s_nan, s_tie, s_r, s_eq, s_cnt, s_total, s_n, s_cut, s_idx;
    __shared__ uint32_t s_prefix, s_next;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = d->k, kp1 = k + 1, n_cand = nwg * kp1;
    for (int i = tid; i < PS_MT_N; i += FN_NT) smt[i] = d->mt[i];
    if (tid == 0) { s_nan = 0; s_tie = 0; s_cnt = 0; s_next = 0xffffffffu; }
    __syncthreads();
    for (int i = tid; i < nwg; i += FN_NT)
        if (flags[i]) s_nan = 1;
    __syncthreads();
    bool exact = s_nan != 0;
    if (!exact) {
        // ---- fast path: the k-th smallest key (= k-th largest value), radix select 8 bits at a time
        // the high halves (value keys) in LDS when they fit; each thread walks a contiguous range (runs of one sorted slice list share
        // their digits: one LDS atomic per run instead of one per key)
        const bool staged = n_cand <= DK_CAP;
        if (staged) {
            int i = tid;
            for (; i + 3 * FN_NT < n_cand; i += 4 * FN_NT) {
                const unsigned long long a0 = cand[i], a1 = cand[i + FN_NT], a2 = cand[i + 2 * FN_NT], a3 = cand[i + 3 * FN_NT];
                sdk[i] = (uint32_t)(a0 >> 32); sdk[i + FN_NT] = (uint32_t)(a1 >> 32); sdk[i + 2 * FN_NT] = (uint32_t)(a2 >> 32); sdk[i + 3 * FN_NT] = (uint32_t)(a3 >> 32);
            }
            for (; i < n_cand; i += FN_NT) sdk[i] = (uint32_t)(cand[i] >> 32);
        }
        const int per = (n_cand + FN_NT - 1) / FN_NT, i0 = min(tid * per, n_cand), i1 = min(i0 + per, n_cand);
        uint32_t prefix = 0;
        int r = k;
        for (int pass = 0; pass < 4; pass++) {
            const int shift = 24 - 8 * pass;
            for (int i = tid; i < 256; i += FN_NT) hist[i] = 0;
            __syncthreads();
            unsigned run_bin = 0xffffffffu, run_cnt = 0;
            for (int i = i0; i < i1; i++) {
                const uint32_t dk = staged ? sdk[i] : (uint32_t)(cand[i] >> 32);
                if (pass == 0 || (dk >> (shift + 8)) == prefix) {
                    const unsigned b = (dk >> shift) & 255;
                    if (b == run_bin) run_cnt++;
                    else { if (run_cnt) atomicAdd(&hist[run_bin], run_cnt); run_bin = b; run_cnt = 1; }
                }
            }
            if (run_cnt) atomicAdd(&hist[run_bin], run_cnt);
            __syncthreads();
            if (tid < 64) {
                unsigned h[4], s = 0;
                for (int j = 0; j < 4; j++) { h[j] = hist[4 * tid + j]; s += h[j]; }
                const unsigned incl = wave_incl_scan(s), excl = incl - s;
                if (excl < (unsigned)r && incl >= (unsigned)r) { // the bin that holds rank r
                    unsigned cum = excl;
                    for (int j = 0; j < 4; j++) {
                        if (cum + h[j] >= (unsigned)r) { s_r = r - (int)cum; s_prefix = (prefix << 8) | (uint32_t)(4 * tid + j); s_eq = (int)h[j]; break; }
                        cum += h[j];
                    }
                }
            }
            __syncthreads();
            r = s_r; prefix = s_prefix;
        }
        if (s_eq > r) exact = true; // the k-th and the (k+1)-th value have the same bits
        if (!exact) {
            uint32_t next = 0xffffffffu;
            for (int i = i0; i < i1; i++) {
                const uint32_t dk = staged ? sdk[i] : (uint32_t)(cand[i] >> 32);
                if (dk <= prefix) { const int slot = atomicAdd(&s_cnt, 1); if (slot < PS_SAMPLE_K_MAX) sk[slot] = cand[i]; }
                else next = min(next, dk);
            }
            atomicMin(&s_next, next);
            __syncthreads();
            for (int i = k + tid; i < PS_SAMPLE_K_MAX; i += FN_NT) sk[i] = ~0ull;
            bitonic_sort_asc<PS_SAMPLE_K_MAX, FN_NT>(sk);
            for (int i = tid; i < k; i += FN_NT) { // -0 and +0: different keys, equal values
                const float v = ckey_val(sk[i]), w = i + 1 < k ? ckey_val(sk[i + 1]) : fkey_val(~s_next);
                if (v == w) s_tie = 1;
                tv[i] = v; tt[i] = (int32_t)(uint32_t)sk[i];
            }
            __syncthreads();
            exact = s_tie != 0 || s_cnt != k;
        }
    }
    if (exact) {
        // ---- std::partial_sort's heap mechanics: make_heap over the first k entries, then every later entry that is greater than
        // the top replaces it.  Only an entry greater than the top at the start of its chunk can enter (the top only rises while no
        // NaN sits in the heap; when it falls, the rest of that chunk is walked entry by entry).
        if (tid == 0) {
            for (int i = 0; i < k; i++) heap[i] = ps_pi{pen[i], i};
            ps_make_heap(heap, k);
        }
        __syncthreads();
        for (int base = k; base < n; base += EX_CHUNK) {
            const float thr = heap[0].v;
            const int j0 = base + tid * EX_PER;
            unsigned m = 0;
#pragma unroll
            for (int e = 0; e < EX_PER; e++)
                if (j0 + e < n && pen[j0 + e] > thr) m |= 1u << e;
            const unsigned c = __popc(m), incl = wave_incl_scan(c);
            if (lane == 63) wsum[wave] = incl;
            __syncthreads();
            unsigned off = incl - c;
            for (int w = 0; w < wave; w++) off += wsum[w];
            for (int e = 0; e < EX_PER; e++)
                if (m & (1u << e)) surv[off++] = j0 + e;
            if (tid == FN_NT - 1) s_total = (int)off;
            __syncthreads();
            if (tid == 0) {
                const int end = min(base + EX_CHUNK, n);
                for (int s = 0; s < s_total; s++) {
                    const int i = surv[s];
                    const float v = pen[i];
                    if (!(v > heap[0].v)) continue;
                    ps_pop_heap_into(heap, k, ps_pi{v, i});
                    if (heap[0].v < thr) { // the top fell below the filter's threshold: the rest of the chunk one by one
                        for (int ii = i + 1; ii < end; ii++) {
                            const float vv = pen[ii];
                            if (vv > heap[0].v) ps_pop_heap_into(heap, k, ps_pi{vv, ii});
                        }
                        break;
                    }
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            ps_sort_heap(heap, k);
            for (int i = 0; i < k; i++) { tv[i] = heap[i].v; tt[i] = heap[i].t; }
        }
    }
    __syncthreads();
    // ---- the chain's tail (ps_sample_tail, same operations): the per-candidate steps spread over the workgroup, the ordered sums and
    // the draw on thread 0
    const float temp = d->temperature, top_p = d->top_p;
    if (temp != 1)
        for (int i = tid; i < k; i += FN_NT) tv[i] /= temp;
    __syncthreads();
    const float top = tv[0];
    __syncthreads();
    for (int i = tid; i < k; i += FN_NT) tv[i] = ps_expf_glibc(tv[i] - top);
    __syncthreads();
    if (tid == 0) {
        double total = 0.;
        for (int i = k; i-- > 0;) total += tv[i];
        s_sum = total;
    }
    __syncthreads();
    for (int i = tid; i < k; i += FN_NT) tv[i] = (float)((double)tv[i] / s_sum);
    __syncthreads();
    if (tid == 0) {
        int n_keep = k, cut = 0;
        if (top_p < 1.0f) {
            float mass = 0.0f;
            int keep   = 0;
            while (keep < k) {
                mass += tv[keep++];
                if (mass >= top_p && keep >= 1) break;
            }
            if (keep < k) {
                n_keep = keep; cut = 1;
                double t2 = 0.;
                for (int i = 0; i < n_keep; i++) t2 += tv[i];
                s_sum = t2;
            }
        }
        s_n = n_keep; s_cut = cut;
    }
    __syncthreads();
    const int nk = s_n;
    if (s_cut)
        for (int i = tid; i < nk; i += FN_NT) tv[i] = (float)((double)tv[i] / s_sum);
    __syncthreads();
    uint64_t calls = 0;
    uint32_t p = d->mt_pos;
    if (nk >= 2) { // ps_discrete_draw
        if (tid == 0) {
            double sum = 0.0;
            for (int i = 0; i < nk; i++) sum += (double)tv[i];
            s_sum = sum;
        }
        __syncthreads();
        for (int i = tid; i < nk; i += FN_NT) cp[i] = (double)tv[i] / s_sum;
        __syncthreads();
        if (tid == 0) {
            double acc = cp[0];
            for (int i = 1; i < nk; i++) { acc = acc + cp[i]; cp[i] = acc; }
            cp[nk - 1] = 1.0;
            const double u = ps_mt_canonical(smt, &p);
            calls = 2;
            int first = 0, len = nk;
            while (len > 0) {
                const int half = len >> 1, mid = first + half;
                if (cp[mid] < u) { first = mid + 1; len = len - half - 1; }
                else len = half;
            }
            s_idx = first;
        }
    } else if (tid == 0) {
        s_idx = 0;
    }
    __syncthreads();
    if (tid == 0) {
        const int idx = s_idx;
        const int32_t tok = tt[idx];
        d->mt_pos = p;
        d->n_outputs += calls;
        d->n_exact += exact ? 1 : 0;
        if (token_out) token_out[0] = tok;
        if (st) { tokens[0] = tok; ids[st->n_out] = tok; st->n_out += 1; st->pos0 += 1; }
    }
    __syncthreads();
    for (int i = tid; i < PS_MT_N; i += FN_NT) d->mt[i] = smt[i];
}

const char *g_last_sample = "";
uint64_t g_sample_counters[2] = {0, 0};

} // namespace

static int slices(int n) { return (n + SL - 1) / SL; }
size_t psl_sample_scratch_bytes(int n_vocab) {
    const size_t nwg = (size_t)slices(n_vocab);
    return nwg * (PS_SAMPLE_K_MAX + 1) * 8 + (((size_t)n_vocab * 4 + nwg * 4 + 255) & ~(size_t)255);
}
void psl_sample(hipStream_t st, const float *logits, int n, ps_sample_dev *d, void *scratch, int32_t *token_out, ps_step_state *state, int32_t *tokens, int32_t *ids) {
    const int nwg = slices(n);
    unsigned long long *cand = (unsigned long long *)scratch;
    float *pen = (float *)(cand + (size_t)nwg * (PS_SAMPLE_K_MAX + 1));
    int *flags = (int *)(pen + n);
    g_last_sample = "sample_slice_kernel + sample_final_kernel";
    hipLaunchKernelGGL(sample_slice_kernel, dim3((unsigned)nwg), dim3(SL_NT), 0, st, logits, n, d, pen, cand, flags);
    hipLaunchKernelGGL(sample_final_kernel, dim3(1), dim3(FN_NT), 0, st, cand, flags, nwg, pen, n, d, token_out, state, tokens, ids);
}

int psl_sample_pack(const ps_sample_cfg *c, const ps_sample_state *s, int n_vocab, ps_sample_dev *out, std::string *err) {
    if (n_vocab < 2) { *err = "sample: n_vocab must be at least 2"; return 2; }
    if (c->top_k < 1 || c->top_k > PS_SAMPLE_K_MAX) { *err = "sample: top_k outside 1.." + std::to_string(PS_SAMPLE_K_MAX) + " is not covered on the device"; return 2; }
    if (c->top_k >= (uint64_t)n_vocab) { *err = "sample: top_k >= n_vocab is not covered on the device"; return 2; }
    if (!(c->temperature > 0)) { *err = "sample: temperature must be > 0"; return 2; }
    if (s->n_window < 0 || s->n_window > PS_SAMPLE_WINDOW_MAX) { *err = "sample: penalty window longer than PS_SAMPLE_WINDOW_MAX"; return 2; }
    if (s->mt_pos > PS_MT_N) { *err = "sample: engine position out of range"; return 2; }
    memcpy(out->mt, s->mt, sizeof out->mt);
    out->mt_pos = s->mt_pos;
    out->k = (int32_t)c->top_k;
    out->temperature = c->temperature; out->top_p = c->top_p;
    out->repeat = c->penalty_repeat; out->freq = c->penalty_freq; out->present = c->penalty_present;
    // RepeatPenalty(cfg, eos, linefeed) (csrc/host/sampler.cpp): the ban and the line-feed spare need the ids; a negative id is "none"
    out->ban_id = (c->ignore_eos && c->special_eos_id >= 0) ? c->special_eos_id : -1;
    const bool active = c->penalty_last_n != 0 && !(c->penalty_repeat == 1.0f && c->penalty_freq == 0.0f && c->penalty_present == 0.0f);
    out->spare_id = (!c->penalize_nl && c->linefeed_id >= 0) ? c->linefeed_id : -1;
    out->n_pen = 0;
    if (active) {
        std::map<int32_t, int32_t> seen;
        for (int i = 0; i < s->n_window; i++)
            if (s->window[i] >= 0) seen[s->window[i]]++;
        for (auto &kv : seen) { out->pen_tok[out->n_pen] = kv.first; out->pen_cnt[out->n_pen] = kv.second; out->n_pen++; }
    }
    out->n_outputs = 0; out->n_exact = 0;
    return 0;
}
void psl_sample_unpack(const ps_sample_dev *d, ps_sample_state *s) {
    memcpy(s->mt, d->mt, sizeof s->mt);
    s->mt_pos = d->mt_pos;
    s->n_outputs += d->n_outputs;
    s->n_exact += d->n_exact;
    g_sample_counters[0] += d->n_exact;
    g_sample_counters[1] += d->n_outputs;
}

extern "C" {

int ps_hip_sample_covered(const ps_sample_cfg *cfg, int n_vocab, const ps_sample_state *state) {
    static ps_sample_dev tmp; // (packing only: not used concurrently by the callers of this check)
    std::string err;
    return psl_sample_pack(cfg, state, n_vocab, &tmp, &err);
}

int ps_hip_sample(ps_hip_ctx *c, const float *logits_dev, int n_vocab, const ps_sample_cfg *cfg, ps_sample_state *state, int32_t *token_out) {
    ps_sample_dev h;
    if (int rc = psl_sample_pack(cfg, state, n_vocab, &h, &c->err)) return rc;
    PS_CHECK(c, hipSetDevice(c->device));
    void *dd = nullptr, *scratch = nullptr;
    PS_CHECK(c, hipMalloc(&dd, sizeof(ps_sample_dev) + 64));
    if (hipMalloc(&scratch, psl_sample_scratch_bytes(n_vocab)) != hipSuccess) { (void)hipFree(dd); PS_FAIL(c, "sample: scratch allocation failed"); }
    int32_t *tok_dev = (int32_t *)((char *)dd + sizeof(ps_sample_dev));
    hipError_t e = hipMemcpyAsync(dd, &h, sizeof h, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        psl_sample(c->stream, logits_dev, n_vocab, (ps_sample_dev *)dd, scratch, tok_dev, nullptr, nullptr, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h, dd, sizeof h, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(token_out, tok_dev, 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(dd); (void)hipFree(scratch);
    if (e != hipSuccess) { c->err = std::string("sample: ") + hipGetErrorString(e); return 1; }
    psl_sample_unpack(&h, state);
    return 0;
}

void ps_hip_sample_counters(uint64_t *out2, int reset) {
    out2[0] = g_sample_counters[0]; out2[1] = g_sample_counters[1];
    if (reset) g_sample_counters[0] = g_sample_counters[1] = 0;
}
const char *ps_hip_last_sample_kernels(void) { return g_last_sample; }

} // extern "C"
