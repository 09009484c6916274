// The saved KV state of a sequence (include/ps_hip.h ps_hip_model_seq_export / _import): the header's layout, written and checked in one place.
// Header-only and plain C++: csrc/model.hip writes and checks it on the device side, libps_host.so exports the check as psh_debug_kv_state_check (tests/test_seq_state_cpu.py).
//
//   offset  0  "PSKV"
//           4  u32 version (1)
//           8  u32 n_layers
//          12  u32 kv_dim
//          16  u32 head_size
//          20  u64 n_tokens
//          28  u32 ps_hip_build_contract() of the writer (the two builds rotate K differently: a K row of one is not a K row of the other)
//          32  zeros up to 64
//   then per layer: K [n_tokens][kv_dim] f32, V [kv_dim][n_tokens] f32 -- no n_ctx anywhere, so a window of another size (or a long-window model) can take it.
// Every field little-endian.  The blob does NOT identify the weights: restoring a state into a model with other weights of the same shape is not detected, the
// caller keeps the two together.
#pragma once
#include <stdint.h>
#include <string.h>

#define PS_KV_STATE_VERSION 1u
#define PS_KV_STATE_HEADER 64u

static inline void ps_kv_put32(uint8_t *p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i)); }
static inline void ps_kv_put64(uint8_t *p, uint64_t v) { for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i)); }
static inline uint32_t ps_kv_get32(const uint8_t *p) { uint32_t v = 0; for (int i = 0; i < 4; i++) v |= (uint32_t)p[i] << (8 * i); return v; }
static inline uint64_t ps_kv_get64(const uint8_t *p) { uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i); return v; }

// bytes of one layer's K (or V) payload, and of the whole blob (n_tokens <= PS_HIP_LONG_CTX_MAX, 32-bit shapes: no overflow)
static inline uint64_t ps_kv_state_plane_bytes(uint32_t kv_dim, uint64_t n_tokens) { return n_tokens * kv_dim * 4; }
static inline uint64_t ps_kv_state_bytes(uint32_t n_layers, uint32_t kv_dim, uint64_t n_tokens) {
    return PS_KV_STATE_HEADER + (uint64_t)n_layers * 2 * ps_kv_state_plane_bytes(kv_dim, n_tokens);
}

static inline void ps_kv_state_write_header(void *buf, uint32_t n_layers, uint32_t kv_dim, uint32_t head_size, uint64_t n_tokens, uint32_t contract) {
    uint8_t *p = (uint8_t *)buf;
    memset(p, 0, PS_KV_STATE_HEADER);
    memcpy(p, "PSKV", 4);
    ps_kv_put32(p + 4, PS_KV_STATE_VERSION);
    ps_kv_put32(p + 8, n_layers);
    ps_kv_put32(p + 12, kv_dim);
    ps_kv_put32(p + 16, head_size);
    ps_kv_put64(p + 20, n_tokens);
    ps_kv_put32(p + 28, contract);
}

// Whether a model of (n_layers, kv_dim, head_size, n_ctx) built with `contract` can take the blob of `bytes` bytes at buf.  nullptr: yes, *n_tokens = its length;
// else the reason.  Nothing behind the header is read.
static inline const char *ps_kv_state_check(const void *buf, uint64_t bytes, uint32_t n_layers, uint32_t kv_dim, uint32_t head_size, uint64_t n_ctx,
                                            uint32_t contract, uint64_t *n_tokens) {
    const uint8_t *p = (const uint8_t *)buf;
    if (!p || bytes < PS_KV_STATE_HEADER) return "shorter than the header";
    if (memcmp(p, "PSKV", 4)) return "not a KV state (magic)";
    if (ps_kv_get32(p + 4) != PS_KV_STATE_VERSION) return "unknown version";
    if (ps_kv_get32(p + 28) != contract) return "written by the other build of the library (ps_hip_build_contract: K is rotated differently)";
    if (ps_kv_get32(p + 8) != n_layers) return "another number of layers";
    if (ps_kv_get32(p + 12) != kv_dim) return "another kv_dim";
    if (ps_kv_get32(p + 16) != head_size) return "another head_size";
    const uint64_t n = ps_kv_get64(p + 20);
    if (n > n_ctx) return "more tokens than the window holds (n_ctx)";
    if (bytes != ps_kv_state_bytes(n_layers, kv_dim, n)) return "length does not match the header";
    if (n_tokens) *n_tokens = n;
    return nullptr;
}
