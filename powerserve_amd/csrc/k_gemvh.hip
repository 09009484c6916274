// F16 weights (gfx950): the activation rounding and the mat-vec / mat-mul of powerserve_compute_forward_mul_mat with an F16 src0.
//
// The reference (libs/ggml/src/ggml.c:13502-13530, 2199-2237) rounds each activation row to fp16 with ggml_fp32_to_fp16_row (F16C
// round-to-nearest-even: +-inf from |x| >= 65520 on, subnormals kept) and runs one ggml_vec_dot_f16 per (row, column): in the AVX build
// 32 fp32 FMA chains over elements 32 i + c (GGML_F16_STEP 32, EPR 8), GGML_F32x8_REDUCE, then the n % 32 leftovers added in DOUBLE and
// a cast to float.  A product of two fp16 values is exact in fp32, so FMA and multiply + add agree and the contract build needs no case.
//
// Device layout of an F16 weight: the GGUF rows as they are, qs [N][K] fp16 (ps_internal.h).
//
// Mat-vec / mat-mul mapping: LPR = 32 / CPL lanes own one weight row, lane q of the row owns the CPL chains q * CPL .. q * CPL + CPL - 1
// and loads them (CPL fp16 = 16 / 8 / 2 bytes, non-temporal) at every step i, in order; a wave holds 64 / LPR rows.  NC activation columns
// are taken per pass (batches loop over column groups; the weight strip of the wave is then served from L2).  The fixed reduction is
// done in registers: c += c + 16, c + 8, c + 4 (across lanes where the partner chain lives in another lane), then the two hadds.
//
// Built with -ffp-contract=off like every file of the library.
#include "ps_dev.h"
#include "ps_internal.h"
#include "ps_quant_dev.h"

namespace {

// ---------------------------------------------------------------- activation rows -> fp16 (MODE 1: RMSNorm first, as k_ops.hip rms_norm_kernel)
template <int MODE>
__global__ __launch_bounds__(256) void f16_act_kernel(const float *x, const float *nw, float eps, int64_t K, _Float16 *out) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = blockIdx.x;
    const float *xr = x + row * K;
    _Float16 *yr = out + row * K;
    float scale = 1.0f;
    if (MODE == 1) {
        // sum += (double)(x*x); mean = sum/ne00; scale = 1/sqrtf(mean + eps)  (ggml.c:12667-12720)
        double s = 0.0;
        for (int64_t i = threadIdx.x; i < K; i += 256) s += (double)__fmul_rn(xr[i], xr[i]);
        s = wave_sum_d(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        const double tot = (red[0] + red[1]) + (red[2] + red[3]);
        const float mean = (float)(tot / (double)K);
        scale = __fdiv_rn(1.0f, sqrtf(__fadd_rn(mean, eps)));
    }
    for (int64_t i = threadIdx.x; i < K; i += 256) {
        float v = MODE == 1 ? __fmul_rn(xr[i], __fmul_rn(nw[i], scale)) : xr[i];
        // the fp32 product must exist: left alone, the compiler fuses multiply and conversion into v_fma_mixlo_f16, which rounds the
        // exact product once to fp16 -- the reference rounds it to fp32 first (measured: a Llama step differed 1 in ~10^3 tokens)
        asm volatile("" : "+v"(v));
        yr[i] = (_Float16)v; // v_cvt_f16_f32: round to nearest even, overflow to inf, fp16 subnormals kept
    }
}

struct HParams {
    int n_w, pair;                 // pair: out[0][r] = silu(y0[r]) * y1[r] (gate / up), both rows by the same lanes
    const _Float16 *w[3];
    int64_t N[3], ldo[3];
    float *out[3];
    const float *bias[3];
    const float *residual;         // out[0] = residual + y
    int64_t wave0[4];              // first row group (mat-vec: wave, mat-mul: 16-row tile) of matrix i (pair: one "matrix")
    const _Float16 *x;             // [bs][K] fp16 (PRO 0)
    const float *xf, *norm_w;      // PRO 1 / 2: the fp32 column (and the RMSNorm weights), rounded in the prologue
    float eps;
    int64_t K;
    int bs;
};

template <int CPL> struct HVec;
template <> struct HVec<8> { typedef uint32_t T __attribute__((ext_vector_type(4))); };
template <> struct HVec<4> { typedef uint32_t T __attribute__((ext_vector_type(2))); };
template <> struct HVec<1> { typedef uint16_t T; };

template <int CPL>
__device__ __forceinline__ typename HVec<CPL>::T h_raw(const _Float16 *p, bool nt) {
    typedef typename HVec<CPL>::T T;
    return nt ? __builtin_nontemporal_load((const T *)p) : *(const T *)p;
}
template <int CPL>
__device__ __forceinline__ void h_cvt(typename HVec<CPL>::T raw, float (&v)[CPL]) {
    _Float16 h[CPL];
    __builtin_memcpy(h, &raw, sizeof(h));
#pragma unroll
    for (int r = 0; r < CPL; r++) v[r] = (float)h[r];
}

// GGML_F32x8_REDUCE over the 32 chains held as (lane q of the row) x (CPL registers): result in lane q == 0, register 0
template <int CPL>
__device__ __forceinline__ float h_reduce(float (&v)[CPL]) {
    constexpr int offs[5] = {16, 8, 4, 1, 2};
#pragma unroll
    for (int s = 0; s < 5; s++) {
        const int o = offs[s];
        if (o >= CPL) {
            const int lane = threadIdx.x & 63;
#pragma unroll
            for (int r = 0; r < CPL; r++) v[r] = __fadd_rn(v[r], __shfl(v[r], (lane + o / CPL) & 63, 64));
        } else {
#pragma unroll
            for (int r = 0; r + o < CPL; r++)
                if (s < 3 ? r < o : (o == 1 ? (r == 0 || r == 2) : r == 0)) v[r] = __fadd_rn(v[r], v[r + o]);
        }
    }
    return v[0];
}

// The prologue of a single-column launch: the workgroup rounds the fp32 column (PRO 1: RMSNorm first, exactly as f16_act_kernel) into LDS
template <int PRO>
__device__ __forceinline__ void h_prologue(const HParams &p, _Float16 *xs, double *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t K = p.K;
    float scale = 1.0f;
    if (PRO == 1) {
        double s = 0.0;
        for (int64_t i = threadIdx.x; i < K; i += 256) s += (double)__fmul_rn(p.xf[i], p.xf[i]);
        s = wave_sum_d(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        const double tot = (red[0] + red[1]) + (red[2] + red[3]);
        const float mean = (float)(tot / (double)K);
        scale = __fdiv_rn(1.0f, sqrtf(__fadd_rn(mean, p.eps)));
    }
    for (int64_t i = threadIdx.x; i < K; i += 256) {
        float v = PRO == 1 ? __fmul_rn(p.xf[i], __fmul_rn(p.norm_w[i], scale)) : p.xf[i];
        asm volatile("" : "+v"(v)); // the fp32 value first (no v_fma_mixlo_f16: see f16_act_kernel)
        xs[i] = (_Float16)v;
    }
    __syncthreads();
}

// Mat-vec / narrow mat-mul on the VALU: 4 waves per workgroup, each wave 64 / LPR rows; U steps of every row in flight per lane.
template <int CPL, int NC, int PAIR, int PRO>
__global__ __launch_bounds__(256) void gemvh_kernel(HParams p) {
    constexpr int LPR = 32 / CPL, RPW = 64 / LPR, U = NC == 1 ? 16 : 8, NM = PAIR ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) _Float16 xs[];
    __shared__ double red[4];
    if (PRO) h_prologue<PRO>(p, xs, red);
    const _Float16 *X = PRO ? xs : p.x;
    const int lane = threadIdx.x & 63, q = lane % LPR, slot = lane / LPR;
    const int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nmat = PAIR ? 1 : p.n_w;
    if (wv >= p.wave0[nmat]) return; // (after the prologue's barriers)
    int mi = 0;
    while (mi + 1 < nmat && wv >= p.wave0[mi + 1]) mi++;
    const int64_t N = p.N[mi], K = p.K, np = K & ~(int64_t)31, steps = np / 32;
    const int64_t row = (wv - p.wave0[mi]) * RPW + slot;
    const bool live = row < N;
    const int64_t rr = live ? row : N - 1;
    const _Float16 *wrow[NM];
    wrow[0] = p.w[mi] + rr * K + q * CPL;
    if (PAIR) wrow[NM - 1] = p.w[1] + rr * K + q * CPL;
    typedef typename HVec<CPL>::T T;
    for (int c0 = 0; c0 < p.bs; c0 += NC) {
        float acc[NM][NC][CPL];
#pragma unroll
        for (int m = 0; m < NM; m++)
#pragma unroll
            for (int j = 0; j < NC; j++)
#pragma unroll
                for (int r = 0; r < CPL; r++) acc[m][j][r] = 0.f;
        const _Float16 *xc[NC];
#pragma unroll
        for (int j = 0; j < NC; j++) xc[j] = X + (int64_t)min(c0 + j, p.bs - 1) * K + q * CPL;
        const bool nt = c0 + NC >= p.bs; // the last pass over the strip streams it past the caches
        int64_t i = 0;
        for (; i + U <= steps; i += U) {
            T wr[NM][U];
#pragma unroll
            for (int m = 0; m < NM; m++)
#pragma unroll
                for (int u = 0; u < U; u++) wr[m][u] = h_raw<CPL>(wrow[m] + (i + u) * 32, nt);
#pragma unroll
            for (int j = 0; j < NC; j++) {
#pragma unroll
                for (int u = 0; u < U; u++) {
                    float xf[CPL];
                    h_cvt<CPL>(h_raw<CPL>(xc[j] + (i + u) * 32, false), xf);
#pragma unroll
                    for (int m = 0; m < NM; m++) {
                        float wf[CPL];
                        h_cvt<CPL>(wr[m][u], wf);
#pragma unroll
                        for (int r = 0; r < CPL; r++) acc[m][j][r] = __fmaf_rn(wf[r], xf[r], acc[m][j][r]);
                    }
                }
            }
        }
        for (; i < steps; i++) {
            float wf[NM][CPL];
#pragma unroll
            for (int m = 0; m < NM; m++) h_cvt<CPL>(h_raw<CPL>(wrow[m] + i * 32, nt), wf[m]);
#pragma unroll
            for (int j = 0; j < NC; j++) {
                float xf[CPL];
                h_cvt<CPL>(h_raw<CPL>(xc[j] + i * 32, false), xf);
#pragma unroll
                for (int m = 0; m < NM; m++)
#pragma unroll
                    for (int r = 0; r < CPL; r++) acc[m][j][r] = __fmaf_rn(wf[m][r], xf[r], acc[m][j][r]);
            }
        }
#pragma unroll
        for (int j = 0; j < NC; j++) {
            float y[NM];
#pragma unroll
            for (int m = 0; m < NM; m++) {
                y[m] = h_reduce<CPL>(acc[m][j]);
                if (np < K && q == 0) { // leftovers in double (ggml_float), then the cast to float
                    const _Float16 *wl = wrow[m] + np, *xl = X + (int64_t)min(c0 + j, p.bs - 1) * K + np;
                    double s = (double)y[m];
                    for (int64_t k = 0; k < K - np; k++) s += (double)__fmul_rn((float)wl[k], (float)xl[k]);
                    y[m] = (float)s;
                }
            }
            if (!live || q != 0 || c0 + j >= p.bs) continue;
            const int64_t col = c0 + j;
            float v;
            if (PAIR) {
                v = ps_silu_mul(y[0], y[NM - 1]);
            } else {
                v = y[0];
                if (p.bias[mi]) v = __fadd_rn(v, p.bias[mi][row]);
                if (mi == 0 && p.residual) v = __fadd_rn(p.residual[col * p.ldo[0] + row], v);
            }
            p.out[mi][col * p.ldo[mi] + row] = v;
        }
    }
}

// Batches on the matrix cores.  v_mfma_f32_16x16x4_f32 with its accumulator chained from one instruction to the next is a k-ordered fp32
// fma chain (as attn_pv_mfma_kernel, k_attn.hip): per ggml chain c one accumulator tile of 16 weight rows x 16 columns, k = four
// consecutive steps i (elements 32 i + c of the row and of the fp16-rounded column; lane l: A = W[row l & 15][32 (i0 + l / 16) + c],
// B = X[column l & 15][same]).  After the last step the 32 tiles are added in GGML_F32x8_REDUCE's association, per lane and register:
// no data moves.  A workgroup = 4 waves = the same 16 rows x 4 column tiles (the weight strip is fetched once per 64 columns).
// Steps past the end are zeros: fma(0, 0, acc) == acc (an accumulator is never -0: it starts at +0).
template <int PAIR>
__global__ __launch_bounds__(256) void gemmh_mfma_kernel(HParams p) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    constexpr int NM = PAIR ? 2 : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, kq = lane >> 4;
    const int64_t tile = blockIdx.x;
    const int nmat = PAIR ? 1 : p.n_w;
    int mi = 0;
    while (mi + 1 < nmat && tile >= p.wave0[mi + 1]) mi++;
    const int64_t N = p.N[mi], K = p.K, np = K & ~(int64_t)31, steps = np / 32;
    const int64_t r0 = (tile - p.wave0[mi]) * 16, c0 = ((int64_t)blockIdx.y * 4 + wave) * 16;
    if (c0 >= p.bs) return;
    const int64_t ra = min(r0 + lr, N - 1), cb = min(c0 + lr, (int64_t)p.bs - 1);
    const _Float16 *xrow = p.x + cb * K;
    float y[NM][4];
#pragma unroll
    for (int m = 0; m < NM; m++) {
        const _Float16 *wbase = PAIR ? p.w[m] : p.w[mi];
        const _Float16 *wrow = wbase + ra * K;
        f32x4 acc[32];
#pragma unroll
        for (int c = 0; c < 32; c++) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int64_t i0 = 0; i0 < steps; i0 += 4) {
            const int64_t i = i0 + kq;
            const bool in = i < steps;
            const int64_t ic = in ? i : 0;
            u32x4 wr[4], xr[4];
#pragma unroll
            for (int v = 0; v < 4; v++) {
                wr[v] = __builtin_nontemporal_load((const u32x4 *)(wrow + ic * 32 + v * 8));
                xr[v] = *(const u32x4 *)(xrow + ic * 32 + v * 8);
            }
            _Float16 wh[32], xh[32];
            __builtin_memcpy(wh, wr, 64);
            __builtin_memcpy(xh, xr, 64);
#pragma unroll
            for (int c = 0; c < 32; c++) {
                const float a = in ? (float)wh[c] : 0.f, b = in ? (float)xh[c] : 0.f;
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[c], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float v[32];
#pragma unroll
            for (int c = 0; c < 32; c++) v[c] = acc[c][j];
#pragma unroll
            for (int c = 0; c < 16; c++) v[c] = __fadd_rn(v[c], v[c + 16]);
#pragma unroll
            for (int c = 0; c < 8; c++) v[c] = __fadd_rn(v[c], v[c + 8]);
#pragma unroll
            for (int c = 0; c < 4; c++) v[c] = __fadd_rn(v[c], v[c + 4]);
            float yy = __fadd_rn(__fadd_rn(v[0], v[1]), __fadd_rn(v[2], v[3]));
            if (np < K) { // leftovers in double, then the cast to float
                const int64_t row = min(r0 + kq * 4 + j, N - 1);
                const _Float16 *wl = wbase + row * K + np, *xl = xrow + np;
                double s = (double)yy;
                for (int64_t k = 0; k < K - np; k++) s += (double)__fmul_rn((float)wl[k], (float)xl[k]);
                yy = (float)s;
            }
            y[m][j] = yy;
        }
    }
    const int64_t col = c0 + lr;
    if (col >= p.bs) return;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t row = r0 + kq * 4 + j;
        if (row >= N) continue;
        float v;
        if (PAIR) {
            v = ps_silu_mul(y[0][j], y[NM - 1][j]);
        } else {
            v = y[0][j];
            if (p.bias[mi]) v = __fadd_rn(v, p.bias[mi][row]);
            if (mi == 0 && p.residual) v = __fadd_rn(p.residual[col * p.ldo[0] + row], v);
        }
        p.out[mi][col * p.ldo[mi] + row] = v;
    }
}

template <int CPL, int NC, int PAIR, int PRO>
void launch_h(hipStream_t st, HParams &p) {
    constexpr int RPW = 64 / (32 / CPL);
    int64_t w0 = 0;
    const int nm = PAIR ? 1 : p.n_w;
    for (int i = 0; i < nm; i++) { p.wave0[i] = w0; w0 += (p.N[i] + RPW - 1) / RPW; }
    p.wave0[nm] = w0;
    psk_note_kernel("gemvh_kernel<%d, %d, %d, %d>", CPL, NC, PAIR, PRO);
    const size_t lds = PRO ? (size_t)(p.K + 8) * 2 : 0;
    hipLaunchKernelGGL((gemvh_kernel<CPL, NC, PAIR, PRO>), dim3((unsigned)((w0 + 3) / 4)), dim3(256), lds, st, p);
}
template <int CPL, int PAIR>
void launch_hc(hipStream_t st, HParams &p, int pro) {
    if (p.bs == 1) {
        if (pro == 1) launch_h<CPL, 1, PAIR, 1>(st, p);
        else if (pro == 2) launch_h<CPL, 1, PAIR, 2>(st, p);
        else launch_h<CPL, 1, PAIR, 0>(st, p);
    } else {
        launch_h<CPL, 4, PAIR, 0>(st, p);
    }
}
template <int PAIR>
void launch_mfma(hipStream_t st, HParams &p) {
    int64_t t0 = 0;
    const int nm = PAIR ? 1 : p.n_w;
    for (int i = 0; i < nm; i++) { p.wave0[i] = t0; t0 += (p.N[i] + 15) / 16; }
    p.wave0[nm] = t0;
    psk_note_kernel("gemmh_mfma_kernel<%d>", PAIR);
    hipLaunchKernelGGL((gemmh_mfma_kernel<PAIR>), dim3((unsigned)t0, (unsigned)((p.bs + 63) / 64)), dim3(256), 0, st, p);
}

} // namespace

void psk_f16_act(hipStream_t st, int mode, const float *x, const float *norm_w, float eps, int64_t K, int64_t rows, _Float16 *out) {
    if (mode == 1) hipLaunchKernelGGL(f16_act_kernel<1>, dim3((unsigned)rows), dim3(256), 0, st, x, norm_w, eps, K, out);
    else hipLaunchKernelGGL(f16_act_kernel<0>, dim3((unsigned)rows), dim3(256), 0, st, x, nullptr, 0.f, K, out);
}

int g_f16_batch = 0; // ps_hip_debug_set(10, v): F16 batches on 0 = the matrix cores where covered (default), 1 = the VALU chains (A/B)

bool psk_gemvh_takes(const psk_gemv_args &a, int64_t K, int64_t bs) {
    if (a.n_w < 1 || a.n_w > 3 || a.rope || (a.silu_pair && a.n_w != 2) || bs < 1 || bs > (1 << 30)) return false;
    if ((a.pro && !a.pro_x) || (a.pro == 1 && !a.pro_norm_w)) return false;
    for (int i = 0; i < a.n_w; i++)
        if (!a.w[i] || a.w[i]->dtype != PS_F16 || a.w[i]->K != K) return false;
    return !a.silu_pair || (a.w[0]->N == a.w[1]->N && !a.bias[0] && !a.bias[1] && !a.residual);
}
int psk_gemvh(hipStream_t st, int n_cu, const psk_gemv_args &a, _Float16 *x16, int64_t K, int64_t bs) {
    HParams p{};
    p.n_w = a.n_w; p.pair = a.silu_pair; p.x = x16; p.K = K; p.bs = (int)bs; p.residual = a.residual;
    int64_t rows = 0;
    for (int i = 0; i < a.n_w; i++) {
        p.w[i] = (const _Float16 *)a.w[i]->qs; p.N[i] = a.w[i]->N; p.ldo[i] = a.ldo[i]; p.out[i] = a.out[i]; p.bias[i] = a.bias[i];
        rows += a.w[i]->N;
    }
    if (a.silu_pair) rows = a.w[0]->N; // one row group takes row r of both matrices
    // one column: the rounding (with its RMSNorm) in the launch's own prologue, into LDS, whenever the column fits (64 KiB)
    int pro = 0;
    if (a.pro && bs == 1 && K * 2 + 16 <= 64 * 1024) {
        pro = a.pro == 1 ? 1 : 2;
        p.xf = a.pro_x; p.norm_w = a.pro_norm_w; p.eps = a.pro_eps;
    } else if (a.pro) {
        psk_f16_act(st, a.pro == 1 ? 1 : 0, a.pro_x, a.pro_norm_w, a.pro_eps, K, bs, x16);
    }
    if (bs >= 2 && K % 8 == 0 && g_f16_batch == 0) {
        if (a.silu_pair) launch_mfma<1>(st, p); else launch_mfma<0>(st, p);
        return 0;
    }
    // 16-byte rows (K % 8 == 0): 8 chains per lane, 16 rows per wave -- or 4 chains, 8 rows per wave, when that leaves fewer than
    // two waves per CU; any other K: 4 chains (K % 4 == 0) or one chain per lane (2-byte loads)
    const int cpl = K % 8 == 0 ? (rows / 16 >= 2 * n_cu ? 8 : 4) : (K % 4 == 0 ? 4 : 1);
    if (a.silu_pair) {
        if (cpl == 8) launch_hc<8, 1>(st, p, pro); else if (cpl == 4) launch_hc<4, 1>(st, p, pro); else launch_hc<1, 1>(st, p, pro);
    } else {
        if (cpl == 8) launch_hc<8, 0>(st, p, pro); else if (cpl == 4) launch_hc<4, 0>(st, p, pro); else launch_hc<1, 0>(st, p, pro);
    }
    return 0;
}
