"""float64 restatement of the single-token attention, shared by the GPU tests of its approximate (fp16-KV) form."""
import numpy as np


def attention_reference(m, n_kv, hidden=()):
    """softmax(q K^T / sqrt(hs)) V of the LAST layer in float64 from the model's own q and FP32 caches; `hidden` cache slots (kv_mask) take no part,
    the newest slot n_kv - 1 always does (as the kernels keep it)"""
    c = m.cfg
    hs, r2 = c.head_size, c.n_heads // c.n_kv_heads
    q = m.scratch(1, 1)[0].astype(np.float64).reshape(c.n_heads, hs)
    K = m.k_cache(c.n_layers - 1)[:n_kv].astype(np.float64).reshape(n_kv, c.n_kv_heads, hs)
    V = m.v_cache(c.n_layers - 1).astype(np.float64)[:, :n_kv].reshape(c.n_kv_heads, hs, n_kv)
    vis = np.ones(n_kv, bool)
    vis[[h for h in hidden if h < n_kv - 1]] = False
    out = np.empty((c.n_heads, hs))
    for h in range(c.n_heads):
        s = K[:, h // r2, :] @ q[h] / np.sqrt(hs)
        s[~vis] = -np.inf
        p = np.exp(s - s.max()); p /= p.sum()
        out[h] = V[h // r2] @ p
    return out.reshape(-1)
