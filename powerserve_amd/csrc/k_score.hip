// Scoring rows of logits against target tokens on the device (include/ps_hip.h ps_hip_score_rows / ps_hip_model_score; DESIGN.md
// "Scoring a text on the device"; the arithmetic and its certificate: ps_score_dev.h).  Three launches, ordered by nothing but the stream:
//   score_max_kernel    grid (slices, rows): a slice's first maximum and whether it holds a NaN or a +inf
//   score_sum_kernel    grid (slices, rows): every workgroup reduces the row's slice maxima itself, then adds its slice's expf(x - max) in double
//                       (per lane serially, then a fixed tree); the workgroup that owns the target's column leaves e_t
//   score_final_kernel  one wave per row: first maximum over the slices, the slice sums added in slice order, the certificate, the record
// Every row is read twice, once by each of the first two launches.
#include "ps_internal.h"
#include "ps_ops.h"
#include "ps_score_dev.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int SL = PS_SCORE_SL, NT = PS_SCORE_NT, NW = NT / 64;

// four columns c .. c + 3 of a row (c a multiple of 4 from the row's start): one 16-byte load where the row is aligned and the quad is whole, scalar loads otherwise
// (a ragged tail, an unaligned row base or stride).  Columns at or behind `end` are not read.
__device__ __forceinline__ void load_quad(const float *row, bool aligned, int c, int end, float v[4]) {
    if (aligned && c + 4 <= end) {
        const float4 q = *(const float4 *)(row + c);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = c + e < end ? row[c + e] : 0.f;
    }
}

__device__ __forceinline__ ps_score_best wave_best(ps_score_best b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ps_score_best other;
        other.v = __shfl_xor(b.v, o, 64);
        other.i = __shfl_xor(b.i, o, 64);
        b = ps_score_better(b, other);
    }
    return b;
}

__global__ __launch_bounds__(NT) void score_max_kernel(const float *logits, int n, int64_t stride, int nsl, float *smax, int32_t *sidx, uint32_t *sflag) {
    __shared__ ps_score_best sb[NW];
    __shared__ int sbad[NW];
    const int s = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *row = logits + (int64_t)r * stride;
    const bool aligned = ((uintptr_t)row & 15) == 0;
    const int c0 = s * SL, c1 = min(n, c0 + SL);
    ps_score_best b{-INFINITY, INT32_MAX};
    int bad = 0;
    for (int c = c0 + 4 * tid; c < c1; c += 4 * NT) {
        float v[4];
        load_quad(row, aligned, c, c1, v);
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (c + e < c1) { bad |= ps_score_outside(v[e]); b = ps_score_better(b, ps_score_best{v[e], c + e}); }
    }
    b = wave_best(b);
    bad = __any(bad);
    if (lane == 0) { sb[wave] = b; sbad[wave] = bad; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NW; w++) { b = ps_score_better(b, sb[w]); bad |= sbad[w]; }
        const int64_t o = (int64_t)r * nsl + s;
        smax[o] = b.v; sidx[o] = b.i; sflag[o] = bad ? PS_SCORE_OUTSIDE : 0u;
    }
}

__global__ __launch_bounds__(NT) void score_sum_kernel(const float *logits, int n, int64_t stride, int nsl, const float *smax, const int32_t *targets, double *ssum, float *et) {
    __shared__ float sm[NW];
    __shared__ double sd[NW];
    const int s = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *row = logits + (int64_t)r * stride;
    const bool aligned = ((uintptr_t)row & 15) == 0;
    const int c0 = s * SL, c1 = min(n, c0 + SL);
    // the row's maximum (its value only: -0 and +0 give the same terms)
    float mx = -INFINITY;
    for (int i = tid; i < nsl; i += NT) mx = fmaxf(mx, smax[(int64_t)r * nsl + i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) sm[wave] = mx;
    __syncthreads();
    mx = sm[0];
    for (int w = 1; w < NW; w++) mx = fmaxf(mx, sm[w]);
    double acc = 0.0;
    for (int c = c0 + 4 * tid; c < c1; c += 4 * NT) {
        float v[4];
        load_quad(row, aligned, c, c1, v);
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (c + e < c1) acc += (double)ps_expf_glibc(v[e] - mx);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
    if (lane == 0) sd[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        double t = sd[0];
        for (int w = 1; w < NW; w++) t += sd[w];
        ssum[(int64_t)r * nsl + s] = t;
        const int tg = targets[r];
        if (tg >= c0 && tg < c1) et[r] = ps_expf_glibc(row[tg] - mx);
    }
}

__global__ __launch_bounds__(64) void score_final_kernel(int n, int nsl, const float *smax, const int32_t *sidx, const uint32_t *sflag, const double *ssum, const float *et,
                                                         const int32_t *targets, int shift, ps_score *out) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int64_t o = (int64_t)r * nsl;
    ps_score_best b{-INFINITY, INT32_MAX};
    uint32_t fl = 0;
    for (int i = lane; i < nsl; i += 64) { b = ps_score_better(b, ps_score_best{smax[o + i], sidx[o + i]}); fl |= sflag[o + i]; }
    b = wave_best(b);
    fl = __any(fl != 0) ? PS_SCORE_OUTSIDE : 0u;
    if (lane != 0) return;
    const int tg = targets[r];
    ps_score rec;
    rec.max_logit = b.v; rec.argmax = b.i; rec.flags = fl; rec.prob = NAN;
    if (tg < 0) {
        rec.flags |= PS_SCORE_NO_TARGET;
    } else if (!fl) {
        double total = ssum[o];
        for (int i = 1; i < nsl; i++) total += ssum[o + i];
        rec.flags |= ps_score_certify(et[r], total, n, shift, &rec.prob);
    }
    out[r] = rec;
}

uint64_t g_score_counters[3] = {0, 0, 0}; // rows scored, of them on the exact path, rows refused (NaN / +inf)

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
int slices(int n) { return (n + SL - 1) / SL; }

} // namespace

int g_score_shift = 0; // ps_hip_debug_set(12, v): eps x 2^v

// scratch of `rows` rows: slice sums, slice maxima, slice arg-max, slice flags, e_t
size_t psl_score_scratch_bytes(int n_vocab, int rows) {
    const size_t k = (size_t)slices(n_vocab) * (size_t)rows;
    return al256(k * 8) + 3 * al256(k * 4) + al256((size_t)rows * 4);
}
// the three launches over rows x n logits (row r at logits + r * stride); targets_dev and out_dev: `rows` device entries
void psl_score(hipStream_t st, const float *logits, int n, int64_t stride, int rows, const int32_t *targets_dev, void *scratch, ps_score *out_dev) {
    const int nsl = slices(n);
    const size_t k = (size_t)nsl * (size_t)rows;
    char *p = (char *)scratch;
    double *ssum = (double *)p;      p += al256(k * 8);
    float *smax = (float *)p;        p += al256(k * 4);
    int32_t *sidx = (int32_t *)p;    p += al256(k * 4);
    uint32_t *sflag = (uint32_t *)p; p += al256(k * 4);
    float *et = (float *)p;
    for (int r0 = 0; r0 < rows; r0 += 32768) { // (grid y is limited to 65 535)
        const int nr = std::min(rows - r0, 32768);
        const float *lg = logits + (int64_t)r0 * stride;
        const size_t ko = (size_t)r0 * nsl;
        hipLaunchKernelGGL(score_max_kernel, dim3((unsigned)nsl, (unsigned)nr), dim3(NT), 0, st, lg, n, stride, nsl, smax + ko, sidx + ko, sflag + ko);
        hipLaunchKernelGGL(score_sum_kernel, dim3((unsigned)nsl, (unsigned)nr), dim3(NT), 0, st, lg, n, stride, nsl, smax + ko, targets_dev + r0, ssum + ko, et + r0);
        hipLaunchKernelGGL(score_final_kernel, dim3((unsigned)nr), dim3(64), 0, st, n, nsl, smax + ko, sidx + ko, sflag + ko, ssum + ko, et + r0, targets_dev + r0, g_score_shift, out_dev + r0);
    }
}
int psl_score_check(ps_hip_ctx *c, int n_vocab, const int32_t *targets, int rows, const char *who) {
    if (n_vocab < PS_SCORE_N_MIN || n_vocab > PS_SCORE_N_MAX) PS_FAIL(c, std::string(who) + ": n_vocab outside 2 .. 2^24");
    for (int i = 0; i < rows; i++)
        if (targets[i] < -1 || targets[i] >= n_vocab) PS_FAIL(c, std::string(who) + ": target outside [-1, n_vocab)");
    return 0;
}
// The exact path and the counters, on records that have arrived on the host (the stream is idle): every flagged row is copied back and
// goes through ProbArray::softmax's own operations (ps_score_row_exact)
int psl_score_finish(ps_hip_ctx *c, const float *logits_dev, int n, int64_t stride, int rows, const int32_t *targets, ps_score *out) {
    std::vector<float> row;
    for (int r = 0; r < rows; r++) {
        if (out[r].flags & PS_SCORE_OUTSIDE) { g_score_counters[2]++; continue; }
        if (out[r].flags & PS_SCORE_NO_TARGET) continue;
        g_score_counters[0]++;
        if (!(out[r].flags & PS_SCORE_EXACT)) continue;
        g_score_counters[1]++;
        row.resize((size_t)n);
        PS_CHECK(c, hipMemcpy(row.data(), logits_dev + (int64_t)r * stride, (size_t)n * 4, hipMemcpyDeviceToHost));
        out[r].prob = ps_score_row_exact(row.data(), n, targets[r]);
    }
    return 0;
}

extern "C" {

int ps_hip_score_rows(ps_hip_ctx *c, const float *logits_dev, int n_vocab, int64_t row_stride, int rows, const int32_t *targets_host, ps_score *out_host) {
    if (rows <= 0) return 0;
    if (row_stride < n_vocab) PS_FAIL(c, "score_rows: row_stride < n_vocab");
    if (int rc = psl_score_check(c, n_vocab, targets_host, rows, "score_rows")) return rc;
    PS_CHECK(c, hipSetDevice(c->device));
    void *scratch = nullptr;
    const size_t sb = psl_score_scratch_bytes(n_vocab, rows), tb = al256((size_t)rows * 4);
    PS_CHECK(c, hipMalloc(&scratch, sb + tb + (size_t)rows * sizeof(ps_score)));
    int32_t *tg = (int32_t *)((char *)scratch + sb);
    ps_score *out_dev = (ps_score *)((char *)scratch + sb + tb);
    hipError_t e = hipMemcpyAsync(tg, targets_host, (size_t)rows * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        psl_score(c->stream, logits_dev, n_vocab, row_stride, rows, tg, scratch, out_dev);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out_host, out_dev, (size_t)rows * sizeof(ps_score), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(scratch);
    if (e != hipSuccess) { c->err = std::string("score_rows: ") + hipGetErrorString(e); return 1; }
    return psl_score_finish(c, logits_dev, n_vocab, row_stride, rows, targets_host, out_host);
}

void ps_hip_score_counters(uint64_t *out3, int reset) {
    for (int i = 0; i < 3; i++) out3[i] = g_score_counters[i];
    if (reset) g_score_counters[0] = g_score_counters[1] = g_score_counters[2] = 0;
}

} // extern "C"
