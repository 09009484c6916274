// The single-token attention's arithmetic, one copy: attn_decode2_kernel<NV, NT, KVS> (k_attn.hip) and qkv_attn_kernel<NV, KVS> (k_qkvattn.hip: the NT = 512 geometry plus
// a ninth wave that only keeps the barriers company) call these, so the statements that must round where ggml rounds exist once.  They take and return VALUES: a piece
// that also computed its LDS / global addresses compiled to different address arithmetic in the kernels (HISTORY.md, round 9), so loops, addresses, barriers and
// timeline marks stay in the kernels.  k_attn.hip's header describes the algorithm.
#pragma once
#include "ps_dev.h"
#include "ps_expf.h"
#include "ps_softmax_long_dev.h"

namespace {
typedef float ps_f32x4 __attribute__((ext_vector_type(4)));

// The bounded rendezvous of the G workgroups of a kv head on a counter that is never reset (epoch = count / G), one lane.  TICKET: the epoch comes from the ticket the
// arrival returns (exactly G arrivals per head and launch).  Otherwise from `base`, the counter as this workgroup read it at kernel ENTRY: every earlier launch is complete
// (a multiple of G) and of this launch fewer than G workgroups can have arrived before this one has, so base / G IS this launch's epoch whatever the timing -- the arrival
// is then an atomic add nobody waits for (a returned ticket is a memory round trip on the critical path: 2.0 us in profiles/r06_fused_timeline_v1.txt).
template <bool TICKET>
__device__ __forceinline__ void a1_rendezvous(unsigned *ctr, const unsigned base, const unsigned G, unsigned *flag) {
    const unsigned ticket = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned target = ((TICKET ? ticket : base) / G + 1u) * G;
    int spins = 0;
    while ((int)(__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1 << 16)) { __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; } // never hang the GPU: the host turns the flag into an error / a re-run
    }
}

// One score.  ggml_vec_dot_f32 (ggml.c:2092-2133): chain c = 8 a + u runs over the elements 32 i + c; eight lanes hold a cached position's K row (kf[m]: elements
// 32 m + 4 tq .. + 3) and lane tq holds chains 4 tq + e (e = 0..3) with all their steps; q = the head's row + 4 tq.  GGML_F32x8_REDUCE (ggml.c:1354-1371): acc0 += acc2,
// acc1 += acc3 = chain c + chain c + 16 = lane tq + lane tq + 4; acc0 += acc1 = lane + 2; low + high 128 bits = lane + 1; then the two hadds inside lane 0:
// (x0 + x1) + (x2 + x3).  Valid in the lane with tq == 0.
template <int NV>
__device__ __forceinline__ float a1_score(const float4 (&kf)[NV], const float *q) {
    float x[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < NV; m++) {
        const float4 qv = *(const float4 *)(q + m * 32);
        x[0] = __fmaf_rn(kf[m].x, qv.x, x[0]); // sum = x*y + sum, x = K row (src0)
        x[1] = __fmaf_rn(kf[m].y, qv.y, x[1]);
        x[2] = __fmaf_rn(kf[m].z, qv.z, x[2]);
        x[3] = __fmaf_rn(kf[m].w, qv.w, x[3]);
    }
#pragma unroll
    for (int e = 0; e < 4; e++) x[e] = __fadd_rn(x[e], dpp_f<0x104>(x[e])); // tq < 4: + lane tq + 4
#pragma unroll
    for (int e = 0; e < 4; e++) x[e] = __fadd_rn(x[e], dpp_f<0x102>(x[e])); // tq < 2: + lane tq + 2
#pragma unroll
    for (int e = 0; e < 4; e++) x[e] = __fadd_rn(x[e], dpp_f<0x101>(x[e])); // tq = 0: + lane 1
    return __fadd_rn(__fadd_rn(x[0], x[1]), __fadd_rn(x[2], x[3]));
}

// e_j = exp(x_j - max) of a whole group of 8 (ggml_v_expf) in place, and the group's sum by the reference's in-group tree (ggml.c:2831-2866)
__device__ __forceinline__ float a1_exp8(float (&sv)[8], const float mx) {
    ps_v_expf_n<8>(sv, mx);
    return ps_sml_group8(sv[0], sv[1], sv[2], sv[3], sv[4], sv[5], sv[6], sv[7]);
}

// one step of V.p on v_mfma_f32_16x16x4_f32, a k-ordered fma chain with one rounding per product: p_j = e_j * (float)(1/sum) formed where it is used (the same single
// rounding as ggml_vec_scale_f32), masked to 0 -- a mask, not a branch -- for heads and steps that do not exist: fma(v, 0, acc) = acc
__device__ __forceinline__ ps_f32x4 a1_pv_step(const ps_f32x4 acc, const float v, const float e, const float inv, const bool on) {
    const float p = __fmul_rn(e, inv);
    const float b = __uint_as_float(__float_as_uint(p) & (on ? 0xffffffffu : 0u));
    return __builtin_amdgcn_mfma_f32_16x16x4f32(v, b, acc, 0, 0, 0); // sum = x*y + sum, x = V row (src0)
}

} // namespace
