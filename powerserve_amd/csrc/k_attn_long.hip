// Long-window attention (gfx950): the soft-max and V.p of a model whose score rows do not fit in LDS (ps_hip_model_create_long; DESIGN.md
// "Long context").  The scores come from k_attn.hip's score kernels (they write scores[bs][n_heads][n_ctx] to device memory at any window), then
//   attn_softmax_long_kernel   one workgroup per (column, head) row, in place: raw scores -> probabilities.  The row stays in device memory / L2; three passes
//                              (max; e_j and the sum; p_j = e_j * (float)(1 / sum)), every lane re-reading only what it wrote itself.
//   attn_pv_long_kernel<KVS>   forwards of 1..7 columns: out = V.p with attn_softmax_pv_kernel's geometry and chains, the V tile AND the p tile of the r2 rows
//                              streamed through LDS one tile ahead.
// Batches of 8 and more columns keep k_attn.hip's matrix-core V.p kernels behind the long soft-max (psl_attn_pv_mfma).
// The same row routine serves ps_hip_softmax_ext / ps_hip_soft_max for rows above the LDS-resident kernel's cap (softmax_long_ext_kernel).
// Bit-exact: the arithmetic of ggml_vec_soft_max_f32 / ggml_vec_dot_f32 as k_attn.hip states it; the row sum is certified or redone in the reference's own
// order (ps_softmax_long_dev.h).
#include "ps_dev.h"
#include "ps_expf.h"
#include "ps_ops.h"
#include "ps_attn_dev.h"

static_assert(PS_SML_N_MAX == PS_HIP_LONG_CTX_MAX + 64, "ps_softmax_long_dev.h and include/ps_hip.h disagree");

namespace {

constexpr int SML_NT = 1024, SML_NW = SML_NT / 64;

// rows soft-maxed by the long kernels, of them through the sequential sum.  A device global: one per device and per loaded library (a process that loads the
// default AND the -DPS_CONTRACT library has two sets, each counting its own launches); ps_hip_softmax_long_counters adds up the devices this library launched on
__device__ unsigned long long g_sml_counters[2];

// One row of n logits -> probabilities at `out` (n floats), by all SML_NT threads of the workgroup.
//   ld8(gi, v)  the eight logits of group gi (elements 8 gi .. 8 gi + 7);  ld1(j)  logit j (the n % 8 leftovers)
//   st8 / rd8   store / re-read eight values of `out` (16-byte accesses where the row is aligned)
// gsl: LDS, n / 8 floats (the group sums, kept for the sequential sum).  A lane re-reads from `out` only what it stored itself.
template <bool AL, class LD8, class LD1>
__device__ __forceinline__ void sml_row(const int n, float *out, const int shift, float *gsl, LD8 &&ld8, LD1 &&ld1) {
    __shared__ float redf[SML_NW];
    __shared__ double redd[SML_NW];
    __shared__ float tails[8];
    __shared__ float inv_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ng = n >> 3, n8 = ng << 3, ntail = n - n8;
    auto st8 = [&](int gi, const float (&v)[8]) {
        float *p = out + (size_t)gi * 8;
        if (AL) { *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]); *(float4 *)(p + 4) = make_float4(v[4], v[5], v[6], v[7]); }
        else {
#pragma unroll
            for (int l = 0; l < 8; l++) p[l] = v[l];
        }
    };
    auto rd8 = [&](int gi, float (&v)[8]) {
        const float *p = out + (size_t)gi * 8;
        if (AL) { const float4 lo = *(const float4 *)p, hi = *(const float4 *)(p + 4); v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w; }
        else {
#pragma unroll
            for (int l = 0; l < 8; l++) v[l] = p[l];
        }
    };
    // ---- pass 1: the row maximum
    float mx = -INFINITY;
    for (int gi = tid; gi < ng; gi += SML_NT) {
        float v[8];
        ld8(gi, v);
#pragma unroll
        for (int l = 0; l < 8; l++) mx = fmaxf(mx, v[l]);
    }
    float xt = 0.f;
    if (tid < ntail) { xt = ld1(n8 + tid); mx = fmaxf(mx, xt); }
    mx = wave_max_dpp(mx);
    if (lane == 0) redf[wave] = mx;
    __syncthreads();
    mx = redf[0];
#pragma unroll
    for (int w = 1; w < SML_NW; w++) mx = fmaxf(mx, redf[w]);
    // ---- pass 2: e_j = exp(x_j - max) (ggml_v_expf on whole groups of 8, libm's expf on the leftovers), group sums in the reference's association,
    //      a double sum per lane
    double rs = 0.0;
    for (int gi = tid; gi < ng; gi += SML_NT) {
        float v[8];
        ld8(gi, v);
#pragma unroll
        for (int l = 0; l < 8; l++) v[l] = ps_v_expf(__fsub_rn(v[l], mx));
        st8(gi, v);
        const float gs = ps_sml_group8(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
        gsl[gi] = gs;
        rs += (double)gs;
    }
    float et = 0.f;
    if (tid < ntail) { et = ps_expf_glibc(__fsub_rn(xt, mx)); tails[tid] = et; rs += (double)et; }
    rs = wave_sum_d_dpp(rs);
    if (lane == 0) redd[wave] = rs;
    __syncthreads();
    // ---- the sum settled: certified as it is, or once more in the reference's order (one lane, from the group sums in LDS)
    if (tid == 0) {
        double S = redd[0];
#pragma unroll
        for (int w = 1; w < SML_NW; w++) S += redd[w];
        float inv;
        const int ok = ps_sml_certify(S, n, shift, &inv);
        if (!ok) inv = (float)(1.0 / ps_sml_sum_seq(gsl, ng, tails, ntail));
        inv_s = inv;
        atomicAdd(&g_sml_counters[0], 1ull);
        if (!ok) atomicAdd(&g_sml_counters[1], 1ull);
    }
    __syncthreads();
    const float inv = inv_s;
    // ---- pass 3: p_j = e_j * (float)(1 / sum) (ggml_vec_scale_f32)
    for (int gi = tid; gi < ng; gi += SML_NT) {
        float v[8];
        rd8(gi, v);
#pragma unroll
        for (int l = 0; l < 8; l++) v[l] = __fmul_rn(v[l], inv);
        st8(gi, v);
    }
    if (tid < ntail) out[n8 + tid] = __fmul_rn(et, inv);
}

// grid (n_heads, bs): row (column i, head h) of a.scores, in place.  Dynamic LDS: n_ctx / 8 floats.
__global__ __launch_bounds__(SML_NT) void attn_softmax_long_kernel(psl_attn_args a, int shift) {
    extern __shared__ __attribute__((aligned(16))) float gsl[];
    const int h = blockIdx.x, i = blockIdx.y, bs = att_bs(a), pos0 = att_pos0(a), n_kv = pos0 + bs;
    float *row = a.scores + ((int64_t)i * a.n_heads + h) * a.n_ctx;
    auto logit = [&](const float s, const int j) { return att_logit(s, a.scale, att_visible(a, i, bs, pos0, j)); }; // (as attn_softmax_rows)
    sml_row<true>(n_kv, row, shift, gsl,
                  [&](int gi, float (&v)[8]) {
                      const float4 lo = *(const float4 *)(row + (size_t)gi * 8), hi = *(const float4 *)(row + (size_t)gi * 8 + 4);
                      const float s[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
                      for (int l = 0; l < 8; l++) v[l] = logit(s[l], gi * 8 + l);
                  },
                  [&](int j) { return logit(row[j], j); });
}

// The op API's rows above the LDS-resident kernel's cap (softmax_ext_kernel, k_ops.hip): x = src * scale (+ mask), one workgroup per row, rows of any
// alignment.  Dynamic LDS: nc / 8 floats.
__global__ __launch_bounds__(SML_NT) void softmax_long_ext_kernel(char *dst, uint64_t dst_nb1, const char *src, uint64_t src_nb1, int nc, int64_t ne1, const float *mask,
                                                                  float scale, int shift) {
    extern __shared__ __attribute__((aligned(16))) float gsl[];
    const int64_t row = blockIdx.x;
    const float *sp = (const float *)(src + row * src_nb1);
    float *dp       = (float *)(dst + row * dst_nb1);
    const float *mp = mask ? mask + (row % ne1) * nc : nullptr;
    auto logit = [&](const int j) {
        float v = __fmul_rn(sp[j], scale);
        if (mp) v = __fadd_rn(v, mp[j]); // slope == 1
        return v;
    };
    sml_row<false>(nc, dp, shift, gsl,
                   [&](int gi, float (&v)[8]) {
#pragma unroll
                       for (int l = 0; l < 8; l++) v[l] = logit(gi * 8 + l);
                   },
                   logit);
}

// ---------------------------------------------------------------- V.p, 1..7 columns
// out[i][h][d] = ggml_vec_dot_f32(n_kv, V^T[kvh * hs + d], p[i][h]): grid (hs / 4, n_kv_heads, bs), 1024 threads; thread = (chain c = tid & 31, channel
// dl = (tid >> 5) & 3, head g = tid >> 7), as attn_softmax_pv_kernel.  LDS holds one tile of T positions: rows 0..3 the four V channels, rows 4..4 + r2 - 1 the
// probability rows of the kv head's q heads, row stride STR floats.  The next tile is in flight (registers) while the chains run over the current one; the chain
// state stays in registers across tiles; GGML_F32x8_REDUCE and the n_kv % 32 leftovers (ps_dot_left) follow the last tile.
// Banks: a wave is two half-waves on channels dl, dl + 1 of one head: the V reads are 32 consecutive floats each, STR = 32 (mod 64) floats apart -> all 64
// banks once; the p reads of the two half-waves are the same 32 addresses (broadcast).  tools/lds_bank_check.py: one pass each, and for the 16-byte parks.
constexpr int PVL_NT = 1024, PVL_TMAX = 2048, PVL_SLOTS = (4 + R2MAX) * (PVL_TMAX / 4) / PVL_NT; // float4 loads per thread and tile, at most
__host__ __device__ constexpr int pvl_stride(int T) { return ((T + 63) & ~63) + 32; }
template <int KVS>
__global__ __launch_bounds__(PVL_NT) void attn_pv_long_kernel(psl_attn_args a, int T) {
    extern __shared__ __attribute__((aligned(16))) float tl[]; // [4 + r2][STR]
    const int hs = a.head_size, dim = a.n_heads * hs, r2 = a.n_heads / a.n_kv_heads;
    const int kvh = blockIdx.y, i = blockIdx.z, bs = att_bs(a), pos0 = att_pos0(a);
    const int n_kv = pos0 + bs, np = n_kv & ~31, n_kv4 = (n_kv + 3) & ~3; // (n_kv4 <= n_ctx: n_ctx is a multiple of 4)
    const int STR = pvl_stride(T), T4 = T >> 2, tid = threadIdx.x;
    const float *vbase = a.v_cache + ((int64_t)kvh * hs + blockIdx.x * 4) * a.n_ctx;
    const float *pbase = a.scores + ((int64_t)i * a.n_heads + (int64_t)kvh * r2) * a.n_ctx;
    // ---- this thread's part of a tile: slot k is the 16-byte segment f = tid + NT k -> (row f / T4, column 4 (f % T4)); the same for every tile
    const float *src[PVL_SLOTS];
    int dst[PVL_SLOTS], lim[PVL_SLOTS]; // LDS float index (-1: no such segment); the segment exists in tile t0 while t0 < lim
    bool isv[PVL_SLOTS];
#pragma unroll
    for (int k = 0; k < PVL_SLOTS; k++) {
        const int f = tid + PVL_NT * k, row = f / T4, col = (f - row * T4) * 4;
        const bool in = row < 4 + r2;
        isv[k] = row < 4;
        src[k] = (row < 4 ? vbase + (int64_t)row * a.n_ctx : pbase + (int64_t)(in ? row - 4 : 0) * a.n_ctx) + col;
        dst[k] = in ? row * STR + col : -1;
        lim[k] = in ? n_kv4 - col : 0;
    }
    float4 ld[PVL_SLOTS];
    auto load_tile = [&](int t0) {
#pragma unroll
        for (int k = 0; k < PVL_SLOTS; k++) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t0 < lim[k]) { // columns t0 + col .. + 3 < n_kv4 <= n_ctx: inside the row
                if (KVS && isv[k]) {
                    const ps_u32x4 t = __builtin_nontemporal_load((const ps_u32x4 *)(src[k] + t0));
                    __builtin_memcpy(&v, &t, 16);
                } else v = *(const float4 *)(src[k] + t0);
            }
            ld[k] = v;
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int k = 0; k < PVL_SLOTS; k++)
            if (dst[k] >= 0) *(float4 *)(tl + dst[k]) = ld[k];
    };
    load_tile(0);
    store_tile();
    __syncthreads();
    const int c = tid & 31, dl = (tid >> 5) & 3, g = tid >> 7;
    const bool live = g < r2;
    const float *vr = tl + dl * STR, *pg = tl + (4 + (live ? g : 0)) * STR;
    float acc = 0.f, out = 0.f;
    for (int t0 = 0; t0 < n_kv; t0 += T) {
        const int tn = min(T, np - t0); // chain columns of this tile (a multiple of 32; 0 on a leftover-only tile)
        if (t0 > 0) {
            __syncthreads(); // previous tile consumed
            store_tile();
            __syncthreads();
        }
        if (t0 + T < n_kv) load_tile(t0 + T);
        if (live) {
            int j = c;
            for (; j + 7 * 32 < tn; j += 8 * 32) { // eight LDS round trips in flight per chain step group
                float v[8], p[8];
#pragma unroll
                for (int k = 0; k < 8; k++) { v[k] = vr[j + 32 * k]; p[k] = pg[j + 32 * k]; }
#pragma unroll
                for (int k = 0; k < 8; k++) acc = __fmaf_rn(v[k], p[k], acc); // x = V row (src0), y = p
            }
            for (; j < tn; j += 32) acc = __fmaf_rn(vr[j], pg[j], acc);
            if (t0 + T >= n_kv) { // last tile (t0 <= np: T is a multiple of 32): reduce the 32 chains, then the n_kv % 32 leftovers in order
                float sres = reduce_f32x8x4(acc);
                for (int jj = np; jj < n_kv; jj++) sres = ps_dot_left(sres, vr[jj - t0], pg[jj - t0], jj - np, n_kv - np);
                out = sres;
            }
        }
    }
    if (live && c == 0) a.att[(int64_t)i * dim + ((int64_t)kvh * r2 + g) * hs + blockIdx.x * 4 + dl] = out;
}

} // namespace

int g_pvl_tile = 0;   // ps_hip_debug_set(13, positions): the V.p tile, a multiple of 32 up to 2048; 0 = default
int g_sml_shift = 0;  // ps_hip_debug_set(14, v): the certificate's eps x 2^v
int psl_attn_long_set_tile(int positions) {
    if (positions < 0 || positions > PVL_TMAX || positions % 32) return 1;
    g_pvl_tile = positions;
    return 0;
}

static size_t sml_lds(int n) { return ((size_t)n / 8 + 8) * 4; }
static unsigned long long g_sml_devs = 0; // devices the long kernels have been launched on: whose counters exist
static void sml_attrs() {
    if (!ps_lds_opt_in<attn_softmax_long_kernel, softmax_long_ext_kernel>((int)sml_lds(PS_SML_N_MAX))) return;
    ps_lds_opt_in<attn_pv_long_kernel<0>, attn_pv_long_kernel<1>>(); // (the first launch on this device)
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && dev < 64) g_sml_devs |= 1ull << dev;
}

// soft-max + V.p of a long-window model behind psl_attn_scores(st, a, bs)
void psl_attn_long_softmax_pv(hipStream_t st, const psl_attn_args &a, int bs) {
    sml_attrs();
    const int r2 = a.n_heads / a.n_kv_heads, nv = a.head_size / 32;
    hipLaunchKernelGGL(attn_softmax_long_kernel, dim3((unsigned)a.n_heads, (unsigned)bs), dim3(SML_NT), sml_lds(a.n_ctx), st, a, g_sml_shift);
    if (bs >= 8) {
        psk_note_attn("attn_scores_mfma_kernel<%d> + attn_softmax_long_kernel + attn_pv_mfma", nv);
        psl_attn_pv_mfma(st, a, bs);
        return;
    }
    const int T = g_pvl_tile > 0 ? g_pvl_tile : PVL_TMAX;
    const size_t lds = (size_t)(4 + r2) * pvl_stride(T) * 4;
    const dim3 g((unsigned)(a.head_size / 4), (unsigned)a.n_kv_heads, (unsigned)bs);
    psk_note_attn("attn_scores_kernel<%d> + attn_softmax_long_kernel + attn_pv_long_kernel<%d>", nv, a.kv_stream ? 1 : 0);
    if (a.kv_stream) hipLaunchKernelGGL(attn_pv_long_kernel<1>, g, dim3(PVL_NT), lds, st, a, T);
    else hipLaunchKernelGGL(attn_pv_long_kernel<0>, g, dim3(PVL_NT), lds, st, a, T);
}

// ps_hip_softmax_ext for rows of more than 150 KiB, up to PS_SML_N_MAX elements
void psl_softmax_long_ext(hipStream_t st, const ps_tensor *dst, const ps_tensor *src, const float *mask, float scale) {
    sml_attrs();
    const int64_t rows = src->ne[1] * src->ne[2] * src->ne[3];
    hipLaunchKernelGGL(softmax_long_ext_kernel, dim3((unsigned)rows), dim3(SML_NT), sml_lds((int)src->ne[0]), st, (char *)dst->data, (uint64_t)dst->nb[1],
                       (const char *)src->data, (uint64_t)src->nb[1], (int)src->ne[0], (int64_t)src->ne[1], mask, scale, g_sml_shift);
}

extern "C" void ps_hip_softmax_long_counters(uint64_t *out2, int reset) {
    out2[0] = out2[1] = 0;
    int cur = 0;
    if (!g_sml_devs || hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); return; }
    const unsigned long long zero[2] = {0, 0};
    for (int d = 0; d < 64; d++) { // (only devices that ran a long kernel: no other device is opened)
        if (!(g_sml_devs >> d & 1)) continue;
        unsigned long long v[2] = {0, 0};
        if (hipSetDevice(d) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpyFromSymbol(v, HIP_SYMBOL(g_sml_counters), sizeof v) != hipSuccess) { (void)hipGetLastError(); continue; }
        out2[0] += v[0]; out2[1] += v[1];
        if (reset) (void)hipMemcpyToSymbol(HIP_SYMBOL(g_sml_counters), zero, sizeof zero);
    }
    (void)hipSetDevice(cur);
}
