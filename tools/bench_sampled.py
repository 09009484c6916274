"""Sampled decode at the headline shape: greedy decode_greedy vs decode_sampled (the standard chain inside the captured step,
csrc/k_sample.hip) vs the host loop (single-token forward, logits to the host, host SamplerChain), alternating in one process.
Also the cost of one ps_hip_sample step on tie-free, typical-tie and worst-case (ascending with ties) rows.
Writes one JSON record (default profiles/r07_bench_sampled.json).

    python tools/bench_sampled.py [--steps 256] [--rounds 3] [--eager] [--out FILE | --no-json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="llama-3.1-8b")
    ap.add_argument("--wtype", default="Q4_K")
    ap.add_argument("--n-ctx", type=int, default=4096)
    ap.add_argument("--prompt-len", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--eager", action="store_true", help="eager launches (mode bit 0) for a kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_bench_sampled.json"))
    ap.add_argument("--no-json", action="store_true")
    args = ap.parse_args()
    from powerserve_amd import gguf, hip, host, synth
    d = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"ps_bench_{args.preset}_{args.wtype}_{args.seed}")
    if not os.path.exists(os.path.join(d, ".done")) or synth.load_model_json(d)["llm_config"] != synth.llm_config(args.preset, args.n_ctx):
        synth.write_model_dir(d, args.preset, gguf.NAME_TYPE[args.wtype], n_ctx=args.n_ctx, seed=args.seed)
        open(os.path.join(d, ".done"), "w").write("ok")
    ctx = hip.Ctx(0)
    m = hip.Model(ctx, d, max_batch=128, n_ctx=args.n_ctx)
    if args.eager:
        m.set_mode(1)
    V = m.cfg.vocab_size
    prompt = np.random.default_rng(args.seed).integers(0, V, args.prompt_len).astype(np.int32)
    scfg = host.SamplerCfg.make(V, seed=args.seed)  # the reference's default chain: top-k 40, T 0.8, top-p 0.95

    def prefilled():
        m.reset()
        m.prefill(prompt[:-1], 128)
        ctx.sync()
        return int(prompt[-1])

    def greedy():
        tok = prefilled()
        t0 = time.perf_counter()
        ids = m.decode_greedy(tok, args.steps)
        return time.perf_counter() - t0, ids

    def sampled():
        tok = prefilled()
        chain = host.Sampler(scfg)
        dc, st = chain.device_state()
        chain.close()
        t0 = time.perf_counter()
        ids = m.decode_sampled(tok, args.steps, dc, st)
        return time.perf_counter() - t0, ids

    def host_loop():
        cur = prefilled()
        chain = host.Sampler(scfg)
        out = []
        t0 = time.perf_counter()
        for _ in range(args.steps):
            lg, _ = m.forward([cur], [m.position])
            cur = chain.sample(lg[0])
            out.append(cur)
        dt = time.perf_counter() - t0
        chain.close()
        return dt, np.array(out, np.int32)

    legs = {"greedy": greedy, "sampled": sampled, "host_loop": host_loop}
    for f in legs.values():  # warm-up: first use of every kernel, the captures
        f()
    rates = {k: [] for k in legs}
    ids = {}
    for _ in range(args.rounds):
        for k, f in legs.items():
            dt, got = f()
            rates[k].append(args.steps / dt)
            ids[k] = got
    med = {k: float(np.median(v)) for k, v in rates.items()}
    rec = {"shape": f"{args.preset} {args.wtype} n_ctx {args.n_ctx} prompt {args.prompt_len}", "steps": args.steps, "rounds": args.rounds,
           "chain": "reference default: top-k 40, temperature 0.8, top-p 0.95, penalty window 64 (inactive: repeat 1)", "eager": args.eager,
           "tokens_per_s": {k: [round(x, 2) for x in v] for k, v in rates.items()}, "median_tokens_per_s": {k: round(v, 2) for k, v in med.items()},
           "sampled_over_greedy": round(med["sampled"] / med["greedy"], 4), "host_loop_over_greedy": round(med["host_loop"] / med["greedy"], 4),
           "sampled_ids_equal_host_loop": bool(np.array_equal(ids["sampled"], ids["host_loop"]))}
    # one ps_hip_sample step (host wall time around the call, which also allocates and frees its scratch): the exact path's extra cost
    dev = ctx.malloc(V * 4)
    rng = np.random.default_rng(1)
    rows = {"tie_free": (rng.standard_normal(V) * 2.5).astype(np.float32)}
    typ = rows["tie_free"].copy()
    typ[rng.integers(0, V, 3)] = typ.max()
    rows["typical_tie"] = typ
    rows["worst_ascending_with_ties"] = ((np.arange(V) // 2) / V).astype(np.float32)
    dc, st = host.Sampler(scfg).device_state()
    step_us = {}
    for name, row in rows.items():
        ctx.check(ctx.L.ps_hip_memcpy_h2d(ctx.h, dev, row.ctypes.data, row.nbytes))
        hip.sample(ctx, dev, V, dc, st)
        e0 = st.n_exact
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            hip.sample(ctx, dev, V, dc, st)
            ts.append(time.perf_counter() - t0)
        step_us[name] = {"us": round(float(np.median(ts)) * 1e6, 1), "exact_path": int(st.n_exact - e0) == 5}
    ctx.free(dev)
    rec["ps_hip_sample_wall_us"] = step_us
    rec["sample_kernels"] = hip.last_sample_kernels()
    print(json.dumps(rec))
    if not args.no_json:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    m.close()
    ctx.close()


if __name__ == "__main__":
    main()
