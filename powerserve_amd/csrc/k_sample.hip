// The standard sampler chain on the device (include/ps_hip.h ps_hip_sample / ps_hip_model_decode_sampled; DESIGN.md "Sampled
// decode on the device").  Two launches behind the lm_head, both read everything from device buffers so that one captured
// step serves every configuration:
//   sample_slice_kernel  one workgroup per 512 logits: EOS ban + repeat penalty (the penalised row also goes to `pen`),
//                        the slice's top-(k+1) as 64-bit keys (value descending, token ascending), a NaN flag
//   sample_final_kernel  one workgroup: radix select of the k-th key over the slice lists, gather + sort of the k winners;
//                        when the k + 1 largest values are not pairwise distinct or a NaN is anywhere, std::partial_sort's
//                        own heap mechanics over `pen` instead (the exact path); then the chain's tail and the draw
//                        (ps_sample_dev.h) on the device-resident mt19937, and the decode bookkeeping of psl_argmax2
// Each kernel has a second entry for the rows of a batched step (psl_sample_rows: a ps_sample_dev and a scratch of psl_sample_scratch_bytes per row), both on row
// blockIdx.y: sample_slice_rows_kernel on a (slices, rows) grid calls sample_slice_body like sample_slice_kernel; sample_final_rows_kernel on a (1, rows) grid holds the
// same statements as sample_final_kernel, one copy of text included into both (ps_sample_final_body.h says why it is not a function).  A row's workgroups touch that
// row's buffers only.
#include "ps_internal.h"
#include "ps_ops.h"
#include "ps_sample_dev.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <vector>

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

// ENTRY: one instance per kernel that sorts, so that each has the single caller it always had (the compiler inlines those; with two callers it keeps a function, and
// under __forceinline__ sample_final_kernel comes out differently: HISTORY round 19)
template <int N, int NT, int ENTRY = 0> __device__ void bitonic_sort_asc(unsigned long long *s) {
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

// one row's scratch: the slices' candidate lists, the penalised row, the slices' NaN flags (psl_sample_scratch_bytes)
struct sample_scratch {
    unsigned long long *cand;
    float *pen;
    int *flags;
};
__host__ __device__ __forceinline__ sample_scratch sample_carve(void *scratch, int nwg, int n) {
    sample_scratch s;
    s.cand = (unsigned long long *)scratch;
    s.pen = (float *)(s.cand + (size_t)nwg * (PS_SAMPLE_K_MAX + 1));
    s.flags = (int *)(s.pen + n);
    return s;
}

// slice blockIdx.x of one row
template <int ENTRY> __device__ __forceinline__ void sample_slice_body(const float *logits, int n, const ps_sample_dev *d, float *pen, unsigned long long *cand, int *flags) {
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
    bitonic_sort_asc<SL, SL_NT, ENTRY>(sk);
    for (int r = tid; r < kp1; r += SL_NT) cand[(size_t)blockIdx.x * kp1 + r] = sk[r];
    if (tid == 0) flags[blockIdx.x] = snan;
}
__global__ __launch_bounds__(SL_NT) void sample_slice_kernel(const float *logits, int n, const ps_sample_dev *d, float *pen, unsigned long long *cand, int *flags) {
    sample_slice_body<0>(logits, n, d, pen, cand, flags);
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
    constexpr int ENTRY = 0;
#include "ps_sample_final_body.h"
}
// the same statements on row blockIdx.y of a batched step: the drawn id to drawn[row], that row's engine advanced, nothing else
__global__ __launch_bounds__(FN_NT) void sample_final_rows_kernel(int nwg, int n, ps_sample_dev *devs, char *scratch, size_t row_bytes, int32_t *drawn) {
    const sample_scratch s = sample_carve(scratch + (size_t)blockIdx.y * row_bytes, nwg, n);
    const unsigned long long *cand = s.cand;
    const int *flags = s.flags;
    const float *pen = s.pen;
    ps_sample_dev *d = devs + blockIdx.y;
    int32_t *token_out = drawn + blockIdx.y, *tokens = nullptr, *ids = nullptr;
    ps_step_state *st = nullptr;
    constexpr int ENTRY = 1;
#include "ps_sample_final_body.h"
}
__global__ __launch_bounds__(SL_NT) void sample_slice_rows_kernel(const float *logits, int n, int64_t row_stride, const ps_sample_dev *devs, char *scratch, size_t row_bytes) {
    const int row = blockIdx.y;
    const sample_scratch s = sample_carve(scratch + (size_t)row * row_bytes, (int)gridDim.x, n);
    sample_slice_body<1>(logits + (int64_t)row * row_stride, n, devs + row, s.pen, s.cand, s.flags);
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
    const sample_scratch s = sample_carve(scratch, nwg, n);
    g_last_sample = "sample_slice_kernel + sample_final_kernel";
    hipLaunchKernelGGL(sample_slice_kernel, dim3((unsigned)nwg), dim3(SL_NT), 0, st, logits, n, d, s.pen, s.cand, s.flags);
    hipLaunchKernelGGL(sample_final_kernel, dim3(1), dim3(FN_NT), 0, st, s.cand, s.flags, nwg, s.pen, n, d, token_out, state, tokens, ids);
}
void psl_sample_rows(hipStream_t st, const float *logits, int n, int64_t row_stride, int rows, ps_sample_dev *devs, void *scratch, int32_t *drawn) {
    const int nwg = slices(n);
    const size_t row_bytes = psl_sample_scratch_bytes(n);
    g_last_sample = "sample_slice_rows_kernel + sample_final_rows_kernel";
    hipLaunchKernelGGL(sample_slice_rows_kernel, dim3((unsigned)nwg, (unsigned)rows), dim3(SL_NT), 0, st, logits, n, row_stride, devs, (char *)scratch, row_bytes);
    hipLaunchKernelGGL(sample_final_rows_kernel, dim3(1, (unsigned)rows), dim3(FN_NT), 0, st, nwg, n, devs, (char *)scratch, row_bytes, drawn);
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

int ps_hip_sample_rows(ps_hip_ctx *c, const float *logits_dev, int n_vocab, int64_t row_stride, int rows, const ps_sample_cfg *cfgs, ps_sample_state *states, int32_t *tokens_out) {
    if (rows < 1 || rows > PS_SEQ_COLS_MAX) PS_FAIL(c, "sample_rows: 1 <= rows <= 16");
    if (!logits_dev || !cfgs || !states || !tokens_out) PS_FAIL(c, "sample_rows: null argument");
    if (row_stride < (int64_t)n_vocab) PS_FAIL(c, "sample_rows: row_stride < n_vocab");
    std::vector<ps_sample_dev> h((size_t)rows); // every row packed before anything reaches the device: a refusal has changed nothing
    for (int r = 0; r < rows; r++) {
        std::string err;
        if (int rc = psl_sample_pack(cfgs + r, states + r, n_vocab, &h[r], &err)) { c->err = "sample_rows: row " + std::to_string(r) + ": " + err; return rc; }
    }
    PS_CHECK(c, hipSetDevice(c->device));
    const size_t dev_bytes = (size_t)rows * sizeof(ps_sample_dev);
    void *dd = nullptr, *scratch = nullptr;
    PS_CHECK(c, hipMalloc(&dd, dev_bytes + 64));
    if (hipMalloc(&scratch, (size_t)rows * psl_sample_scratch_bytes(n_vocab)) != hipSuccess) { (void)hipFree(dd); PS_FAIL(c, "sample_rows: scratch allocation failed"); }
    int32_t *tok_dev = (int32_t *)((char *)dd + dev_bytes);
    hipError_t e = hipMemcpyAsync(dd, h.data(), dev_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        psl_sample_rows(c->stream, logits_dev, n_vocab, row_stride, rows, (ps_sample_dev *)dd, scratch, tok_dev);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), dd, dev_bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(tokens_out, tok_dev, (size_t)rows * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(dd); (void)hipFree(scratch);
    if (e != hipSuccess) { c->err = std::string("sample_rows: ") + hipGetErrorString(e); return 1; }
    for (int r = 0; r < rows; r++) psl_sample_unpack(&h[r], states + r);
    return 0;
}

void ps_hip_sample_counters(uint64_t *out2, int reset) {
    out2[0] = g_sample_counters[0]; out2[1] = g_sample_counters[1];
    if (reset) g_sample_counters[0] = g_sample_counters[1] = 0;
}
const char *ps_hip_last_sample_kernels(void) { return g_last_sample; }

} // extern "C"
