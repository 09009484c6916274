#!/usr/bin/env python3
"""F16-weight speed: one JSON line with greedy decode tokens/s (hipGraph replay), prefill tokens/s (prompt 512 in chunks of 128) for
llama-3.2-1b and qwen2-0.5b in F16 (synthetic weights, powerserve_amd/synth.py), and the gate/up mat-vec replay
(ps_hip_model_bench_gemv which = 1) as TB/s of GGUF bytes and as a fraction of 8 TB/s.
    python tools/bench_f16.py [--presets llama-3.2-1b,qwen2-0.5b] [--steps 64] [--valu-batch]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from powerserve_amd import gguf, hip, synth  # noqa: E402

PEAK = 8.0e12


def run(ctx, preset, steps, prompt_len=512, chunk=128):
    with tempfile.TemporaryDirectory() as d:
        synth.write_model_dir(d, preset, gguf.F16, n_ctx=1024, seed=11)
        m = hip.Model(ctx, d, max_batch=512, n_ctx=1024)
        prompt = np.random.default_rng(1).integers(0, m.cfg.vocab_size, prompt_len + 1).astype(np.int32)
        m.prefill(prompt[:prompt_len], chunk)  # warm-up (and the first use of every kernel)
        m.reset()
        ctx.sync()
        t0 = time.perf_counter()
        m.prefill(prompt[:prompt_len], chunk)
        ctx.sync()
        t_pf = time.perf_counter() - t0
        m.decode_greedy(int(prompt[-1]), 8)  # capture + warm-up
        t0 = time.perf_counter()
        m.decode_greedy(int(prompt[-1]), steps)
        t_dec = time.perf_counter() - t0
        # gate/up replay of every layer
        L = m.cfg.n_layers
        gu_bytes = sum(m.weights[f"blk.{i}.ffn_gate.weight"].gguf_bytes + m.weights[f"blk.{i}.ffn_up.weight"].gguf_bytes for i in range(L)) / L
        seq, null, nl = C.c_double(), C.c_double(), C.c_int()
        ctx.check(ctx.L.ps_hip_model_bench_gemv(m.h, 20, 1, C.byref(seq), C.byref(null), C.byref(nl)))
        us = seq.value * 1e3 / L  # one layer's gate/up launch
        m.close()
        return {"decode_tok_s": round(steps / t_dec, 1), "prefill_tok_s": round(prompt_len / t_pf, 1),
                "gate_up_us": round(us, 2), "gate_up_MB": round(gu_bytes / 1e6, 2), "gate_up_TBps": round(gu_bytes / us / 1e6, 3),
                "gate_up_frac_8TBps": round(gu_bytes / (us * 1e-6) / PEAK, 3), "last_kernel": ctx.L.ps_hip_last_matmul_kernel().decode()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="llama-3.2-1b,qwen2-0.5b")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--valu-batch", action="store_true", help="batches on the VALU chain kernel instead of the matrix cores (A/B; same bits)")
    a = ap.parse_args()
    ctx = hip.Ctx(0)
    out = {"wtype": "F16", "device": ctx.name(), "batch_kernel": "valu" if a.valu_batch else "mfma"}
    if a.valu_batch:
        ctx.check(ctx.L.ps_hip_debug_set(10, 1))
    for p in a.presets.split(","):
        out[p] = run(ctx, p, a.steps)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
