// Forking a sequence (include/ps_hip.h ps_hip_model_seq_fork): slots [0, n_tokens) of one sequence's K / V caches, every layer, copied into up to
// PS_FORK_DST_MAX other sequences of the same model in ONE launch.
//   seq_fork_kernel   grid (tiles, n_layers, 2 = K | V), 256 lanes; the cache bases come from the model's device table [n_seq][n_layers][2]
//     K [n_ctx][kv_dim]: the prefix is the first n_tokens * kv_dim floats, contiguous, a multiple of 4
//     V [kv_dim][n_ctx]: kv_dim rows of n_tokens floats at pitch n_ctx; n_ctx % 4 == 0 keeps every row base 16-byte aligned, so the groups 0 .. n_tokens / 4 - 1
//                        of a row go as 16-byte accesses and its n_tokens % 4 tail as scalars -- nothing at or behind slot n_tokens of a destination is written
// A 16-byte group is loaded once and stored to every destination: a fork to k children moves 1 + k streams.  Each lane keeps UN groups in flight.
// Offsets are 64-bit (n_ctx * kv_dim reaches 2^27 floats); group COUNTS fit 32 bits (at most n_ctx * kv_dim / 4).
#include "ps_internal.h"
#include "ps_ops.h"

namespace {

constexpr int NT = 256, UN = 4;
typedef float f32x4 __attribute__((ext_vector_type(4)));
// the cache bases come out of a table in memory, so the compiler cannot tell their address space and would emit flat_ accesses: say that they are global
#define PS_GLOBAL __attribute__((address_space(1)))
template <class T> __device__ __forceinline__ PS_GLOBAL T *as_global(const float *p) { return (PS_GLOBAL T *)(uintptr_t)p; }

// Non-temporal loads and stores: every byte is touched once, and the destinations of a fork (537 MB per sequence at the 8B shape, 2 048 tokens) leave nothing in
// the memory-side cache worth keeping.  Measured against plain loads / stores in all four combinations (profiles/r15_bench_fork.json "load_store_ab"): equal within
// 1 % at 7 and 15 children, 10 % ahead of the next best at one child.
template <class T> __device__ __forceinline__ T fork_ld(const float *p) { return __builtin_nontemporal_load(as_global<T>(p)); }
template <class T> __device__ __forceinline__ void fork_st(float *p, T v) { __builtin_nontemporal_store(v, as_global<T>(p)); }

__global__ __launch_bounds__(NT) void seq_fork_kernel(const psl_fork_args a) {
    const int layer = blockIdx.y, part = blockIdx.z;
    const size_t plane = (size_t)layer * 2 + part, per_seq = (size_t)a.n_layers * 2;
    // this plane's bases, read before anything is stored (LDS: the loop over destinations indexes them)
    __shared__ float *bases[PS_FORK_DST_MAX + 1];
    if (threadIdx.x <= a.n_dst) bases[threadIdx.x] = a.kv[(size_t)(threadIdx.x ? a.dst[threadIdx.x - 1] : a.src) * per_seq + plane];
    __syncthreads();
    const float *src = bases[0];
    // the prefix as `rows` rows of `gpr` 16-byte groups + `tail` floats at a pitch: K is one row (n_tokens * kv_dim floats, no tail), V kv_dim rows of n_tokens floats
    const uint32_t rows = part ? (uint32_t)a.kv_dim : 1u;
    const uint32_t gpr = part ? (uint32_t)(a.n_tokens / 4) : (uint32_t)((uint64_t)a.n_tokens * a.kv_dim / 4);
    const uint32_t tail = part ? (uint32_t)(a.n_tokens % 4) : 0u;
    const int64_t pitch = a.n_ctx;
    const uint32_t G = rows * gpr, stride = gridDim.x * NT, first = blockIdx.x * NT + threadIdx.x;
    for (uint32_t g0 = first; g0 < G; g0 += stride * UN) {
        f32x4 v[UN];
        int64_t off[UN];
#pragma unroll
        for (int u = 0; u < UN; u++) {
            const uint32_t g = g0 + u * stride;
            if (g < G) {
                const uint32_t r = g / gpr;
                off[u] = r * pitch + (int64_t)(g - r * gpr) * 4;
                v[u] = fork_ld<f32x4>(src + off[u]);
            }
        }
        for (int d = 0; d < a.n_dst; d++) {
            float *dst = bases[d + 1];
#pragma unroll
            for (int u = 0; u < UN; u++)
                if (g0 + u * stride < G) fork_st<f32x4>(dst + off[u], v[u]);
        }
    }
    for (uint32_t i = first; i < rows * tail; i += stride) {
        const uint32_t r = i / tail;
        const int64_t o = r * pitch + (int64_t)gpr * 4 + (i - r * tail);
        const float x = fork_ld<float>(src + o);
        for (int d = 0; d < a.n_dst; d++) fork_st<float>(bases[d + 1] + o, x);
    }
}

} // namespace

// n_tokens >= 1; ids, n_dst <= PS_FORK_DST_MAX and n_tokens <= n_ctx are the caller's checks (ps_hip_model_seq_fork)
void psl_seq_fork(hipStream_t st, const psl_fork_args &a) {
    const uint64_t groups = (uint64_t)a.n_tokens * a.kv_dim / 4; // K's count; V has at most as many
    const uint64_t want = (groups + NT - 1) / NT;                // one group per lane while the grid is small,
    const uint64_t cap = (uint64_t)(8192 + 2 * a.n_layers - 1) / (2 * a.n_layers); // then ~8192 workgroups in all (32 per CU), each lane looping with UN groups in flight
    const unsigned tiles = (unsigned)(want < 1 ? 1 : want > cap ? cap : want);
    hipLaunchKernelGGL(seq_fork_kernel, dim3(tiles, (unsigned)a.n_layers, 2), dim3(NT), 0, st, a);
}
