// What the attention kernels of k_attn.hip and k_attn_long.hip have in common, one copy: where a forward sits in the cache, which cached slot a column may see, and the
// logit the soft-max starts from.  Value functions only (HISTORY.md, rounds 9 and 16: a shared piece that computes addresses from lane and wave indices compiles to other
// address arithmetic in its callers; one that takes and returns values does not).  The in-group sum tree of the soft-max is ps_sml_group8 (ps_softmax_long_dev.h); the
// single-token kernels' own pieces are in ps_attn1_dev.h.
#pragma once
#include "ps_dev.h"
#include "ps_ops.h"
#include "ps_softmax_long_dev.h"

namespace {

constexpr int R2MAX = 8; // q heads per kv head, at most

// (pos0, bs) of the forward: from the launch arguments when the host knew them at enqueue time (eager batches), else from the device-resident state
__device__ __forceinline__ int att_pos0(const psl_attn_args &a) { return a.bs_host > 0 ? a.n_kv_host - a.bs_host : a.state->pos0; }
__device__ __forceinline__ int att_bs(const psl_attn_args &a) { return a.bs_host > 0 ? a.bs_host : a.state->bs; }

// GET_MASK (src/executor/executor.cpp:210-224) for column i of a forward of bs columns at cache position pos0: a cached slot j < pos0 is visible unless hidden
// (KVCacheInterface::mask), a slot of this forward by the tree mask or, without one, causally
__device__ __forceinline__ bool att_visible(const psl_attn_args &a, const int i, const int bs, const int pos0, const int j) {
    return (j < pos0) ? (a.kv_vis ? a.kv_vis[j] != 0 : true) : (a.tree ? a.tree[i * bs + (j - pos0)] != 0 : (j - pos0) <= i);
}
// SOFTMAX_EXT's input (ggml.c:14889-14914): the score scaled, then the mask added (0 or -inf) -- two roundings
__device__ __forceinline__ float att_logit(const float s, const float scale, const bool ok) { return __fadd_rn(__fmul_rn(s, scale), ok ? 0.f : -INFINITY); }

} // namespace
