"""Long-window models at the headline shape (hip.Model(..., long_window=True), csrc/k_attn_long.hip): decode at depth on an uploaded cache, the cost of
the three-launch attention at short depth against the regular model's fused head, a long prefill, and the share of soft-max rows that took the sequential
sum.  Nobody prefills 131 072 tokens to time a decode step: the cache is filled with seeded random rows by upload and the position advanced.

    python tools/bench_long_ctx.py [--depths 2048,8192,32768,131072] [--steps 48] [--prefill 32768] [--out FILE | --no-json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python tools/bench_long_ctx.py --trace-only   # eager steps at every depth, nothing else
    python tools/bench_long_ctx.py --merge-trace DIR/.../kt_kernel_trace.csv --out FILE      # (no GPU) per-depth shares of the attention launches into FILE
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TRACE_WARM, TRACE_STEPS = 2, 4  # --trace-only: eager steps before the first depth, and per depth
STREAM_TBS = (5.8, 5.9)         # the project's measured streaming rate (README.md), TB/s


def fill_cache(ctx, m, slots, seed):
    """seeded random K / V into the slots [0, slots) of every layer: one 32 MiB block, uploaded over and over (the attention's time does not depend on the values,
    the certificate's outcome does: real-looking rows, not a constant)"""
    cfg = m.cfg
    block = np.random.default_rng(seed).standard_normal(8 << 20, dtype=np.float32)
    for L in range(cfg.n_layers):
        kp, vp = ctx.L.ps_hip_model_k_cache(m.h, L), ctx.L.ps_hip_model_v_cache(m.h, L)
        n = slots * cfg.kv_dim  # K: rows [0, slots) are contiguous
        for o in range(0, n, block.size):
            k = min(block.size, n - o)
            ctx.check(ctx.L.ps_hip_memcpy_h2d(ctx.h, C.c_void_p(kp + 4 * o), block.ctypes.data_as(C.c_void_p), 4 * k))
        for d in range(cfg.kv_dim):  # V: channel d is a row of n_ctx floats
            for o in range(0, slots, block.size):
                k = min(block.size, slots - o)
                ctx.check(ctx.L.ps_hip_memcpy_h2d(ctx.h, C.c_void_p(vp + 4 * (d * cfg.seq_len + o)), block[d:].ctypes.data_as(C.c_void_p), 4 * k))


def decode_rate(ctx, m, depth, steps, rounds):
    """tokens/s of `steps` captured greedy steps that END at position `depth` (median of `rounds`, after a warm-up run that captures)"""
    from powerserve_amd import hip
    rates = []
    for r in range(rounds + 1):
        m.reset()
        m.kv_advance(depth - steps)
        if r == 1:
            hip.softmax_long_counters(reset=True)
        t0 = time.perf_counter()
        m.decode_greedy(1, steps)
        dt = time.perf_counter() - t0
        if r:
            rates.append(steps / dt)
    return float(np.median(rates)), [round(x, 1) for x in rates]


def merge_trace(path, depths, n_layers, out):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    marks = [i for i, r in enumerate(rows) if "attn_softmax_long_kernel" in r[2]]
    per = TRACE_STEPS * n_layers
    assert len(marks) == (TRACE_WARM + TRACE_STEPS * len(depths)) * n_layers, (len(marks), per)
    rec = json.load(open(out)) if os.path.exists(out) else {}
    shares = {}
    for k, depth in enumerate(depths):
        lo = marks[TRACE_WARM * n_layers + k * per]
        hi = marks[TRACE_WARM * n_layers + (k + 1) * per] if k + 1 < len(depths) else len(rows)
        t = {"scores": 0, "softmax": 0, "pv": 0, "all": 0}
        for s, e, name in rows[lo:hi]:
            t["all"] += e - s
            if "attn_scores_kernel" in name: t["scores"] += e - s
            elif "attn_softmax_long_kernel" in name: t["softmax"] += e - s
            elif "attn_pv_long_kernel" in name: t["pv"] += e - s
        us = {k2: v / 1e3 / TRACE_STEPS for k2, v in t.items()}  # per token
        kv_bytes = 2 * n_layers * depth * rec.get("kv_dim", 1024) * 4
        shares[str(depth)] = {"kernel_us_per_token": round(us["all"], 1), "scores_us": round(us["scores"], 1), "softmax_us": round(us["softmax"], 1), "pv_us": round(us["pv"], 1),
                              "share_scores": round(us["scores"] / us["all"], 4), "share_softmax": round(us["softmax"] / us["all"], 4), "share_pv": round(us["pv"] / us["all"], 4),
                              "kv_TB_per_s_in_scores_and_pv": round(kv_bytes / ((us["scores"] + us["pv"]) * 1e-6) / 1e12, 3), "streaming_rate_TB_per_s": list(STREAM_TBS)}
    rec["attention_launches_by_depth"] = shares
    rec["attention_launches_how"] = f"rocprofv3 --kernel-trace of {TRACE_STEPS} eager steps per depth; shares are of the summed kernel time of a token"
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(shares))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="llama-3.1-8b")
    ap.add_argument("--wtype", default="Q4_K")
    ap.add_argument("--n-ctx", type=int, default=131072)
    ap.add_argument("--depths", default="2048,8192,32768,131072")
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--prefill", type=int, default=32768, help="tokens of the timed prefill (0: skip)")
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--max-batch", type=int, default=128)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--model-dir", default=None)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--merge-trace", default=None, metavar="CSV")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_bench_long_ctx.json"))
    ap.add_argument("--no-json", action="store_true")
    args = ap.parse_args()
    depths = [int(x) for x in args.depths.split(",")]
    from powerserve_amd import gguf, synth
    if args.merge_trace:
        merge_trace(args.merge_trace, depths, synth.llm_config(args.preset, args.n_ctx)["n_layers"], args.out)
        return
    from powerserve_amd import hip
    d = args.model_dir or os.path.join(os.environ.get("TMPDIR", "/tmp"), f"ps_bench_{args.preset}_{args.wtype}_{args.seed}")
    if not os.path.exists(os.path.join(d, ".done")):
        synth.write_model_dir(d, args.preset, gguf.NAME_TYPE[args.wtype], n_ctx=4096, seed=args.seed)
        open(os.path.join(d, ".done"), "w").write("ok")
    ctx = hip.Ctx(0)
    m = hip.Model(ctx, d, max_batch=args.max_batch, n_ctx=args.n_ctx, long_window=True)
    cfg = m.cfg
    fill_cache(ctx, m, max(depths), args.seed)
    if args.trace_only:
        m.set_mode(1)
        m.kv_advance(depths[0] - TRACE_STEPS - TRACE_WARM)
        m.decode_greedy(1, TRACE_WARM)
        for depth in depths:
            m.reset()
            m.kv_advance(depth - TRACE_STEPS)
            m.decode_greedy(1, TRACE_STEPS)
        m.close(); ctx.close()
        return
    rec = {"shape": f"{args.preset} {args.wtype}, long-window model, n_ctx {args.n_ctx}, max_batch {args.max_batch}", "kv_dim": cfg.kv_dim, "steps": args.steps, "rounds": args.rounds,
           "cache": "seeded random rows by upload", "decode_by_depth": {}}
    for depth in depths:
        med, runs = decode_rate(ctx, m, depth, args.steps, args.rounds)
        rows, seq = hip.softmax_long_counters()
        rec["decode_by_depth"][str(depth)] = {"tokens_per_s": round(med, 1), "runs": runs, "ms_per_token": round(1e3 / med, 3), "softmax_rows": rows, "rows_on_sequential_sum": seq,
                                              "sequential_share": round(seq / max(rows, 1), 7),
                                              "kv_bytes_per_token": 2 * cfg.n_layers * depth * cfg.kv_dim * 4}
        print(depth, rec["decode_by_depth"][str(depth)], flush=True)
    if args.prefill:
        toks = np.random.default_rng(args.seed).integers(0, cfg.vocab_size, args.prefill).astype(np.int32)
        m.reset()
        m.prefill(toks[:args.chunk], args.chunk)  # first use of the batch kernels
        m.reset()
        hip.softmax_long_counters(reset=True)
        t0 = time.perf_counter()
        m.prefill(toks, args.chunk)
        ctx.sync()
        dt = time.perf_counter() - t0
        rows, seq = hip.softmax_long_counters()
        rec["prefill"] = {"tokens": args.prefill, "chunk": args.chunk, "tokens_per_s": round(args.prefill / dt, 1), "seconds": round(dt, 3), "softmax_rows": rows,
                          "rows_on_sequential_sum": seq, "sequential_share": round(seq / max(rows, 1), 7)}
        print("prefill", rec["prefill"], flush=True)
    m.close()
    # the cost of the long path at short depth: the same shape as a regular model (the fused head) and as a long-window model, both behind 2 048 cached tokens
    short = {}
    for name, lw in (("regular", False), ("long_window", True), ("regular_again", False), ("long_window_again", True)):
        mm = hip.Model(ctx, d, max_batch=args.max_batch, n_ctx=4096, long_window=lw)
        fill_cache(ctx, mm, 2048, args.seed)
        med, runs = decode_rate(ctx, mm, 2048, args.steps, args.rounds)
        short[name] = {"tokens_per_s": round(med, 1), "runs": runs, "attention": ctx.L.ps_hip_last_attention_kernel().decode()}
        mm.close()
        print(name, short[name], flush=True)
    rec["short_depth_2048_n_ctx_4096"] = short
    print(json.dumps(rec))
    if not args.no_json:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
