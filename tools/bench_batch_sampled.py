"""Sampled batched decode at the headline shape: n completions of one prompt (one 2048-token prefill, ps_hip_model_seq_fork to the other sequences), every column on
the reference's default sampler chain with a seed of its own.  Three routes, alternated in one process, every leg rolled back so that all of them decode the same positions:
  (a) greedy        ps_hip_model_decode_batch_greedy (no sampling: what the batched step costs without a chain)
  (b) sampled       ps_hip_model_decode_batch_sampled (csrc/k_sample.hip's rows kernels inside the step, one wait per call)
  (c) rows_on_host  what a caller had before: per step ps_hip_model_decode_batch(lm_head = 1), one ps_hip_sample per row on the model's logits, the tokens up again
(b) and (c) must emit the same ids (checked every round).  Writes one JSON record (default profiles/r19_bench_batch_sampled.json).

    python tools/bench_batch_sampled.py [--steps 64] [--rounds 3] [--out FILE | --no-json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_batch import model_dir  # noqa: E402  (tools/bench_batch.py: the cached bench model)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="llama-3.1-8b")
    ap.add_argument("--wtype", default="Q4_K")
    ap.add_argument("--n-ctx", type=int, default=4096)
    ap.add_argument("--prompt-len", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--ns", default="1,4,8,16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_bench_batch_sampled.json"))
    ap.add_argument("--no-json", action="store_true")
    args = ap.parse_args()
    from powerserve_amd import hip, host
    ns = [int(x) for x in args.ns.split(",")]
    ctx = hip.Ctx(0)
    m = hip.Model(ctx, model_dir(args.preset, args.wtype, args.n_ctx, args.seed), max_batch=128, n_ctx=args.n_ctx)
    V = m.cfg.vocab_size
    prompt = np.random.default_rng(args.seed).integers(0, V, args.prompt_len).astype(np.int32)
    m.seq_reserve(max(ns))
    m.prefill(prompt[:-1], 128)
    if max(ns) > 1:
        m.seq_fork(0, list(range(1, max(ns))))
    ctx.sync()
    first = int(prompt[-1])
    logits = ctx.L.ps_hip_model_logits(m.h)

    def chains(n):
        """the reference's default chain (top-k 40, T 0.8, top-p 0.95), column i seeded args.seed + i: the device's view of its start"""
        out = []
        for i in range(n):
            ch = host.Sampler(host.SamplerCfg.make(V, seed=args.seed + i))
            out.append(ch.device_state())
            ch.close()
        return [c for c, _ in out], [s for _, s in out]

    def rollback(n):
        for s in range(n):
            m.seq_select(s)
            m.kv_rollback(args.steps)
        ctx.sync()

    def greedy(n):
        t0 = time.perf_counter()
        ids = m.decode_batch_greedy(list(range(n)), [first] * n, args.steps)
        return time.perf_counter() - t0, ids

    def sampled(n):
        cfgs, states = chains(n)
        t0 = time.perf_counter()
        ids = m.decode_batch_sampled(list(range(n)), [first] * n, args.steps, cfgs, states)
        dt = time.perf_counter() - t0
        kernels["sampled"] = hip.last_sample_kernels()
        return dt, ids

    def rows_on_host(n):
        cfgs, states = chains(n)
        seqs, cur, out = list(range(n)), [first] * n, []
        t0 = time.perf_counter()
        for _ in range(args.steps):
            m.decode_batch(seqs, cur, lm_head=True, want_logits=False)
            cur = [hip.sample(ctx, logits + 4 * r * V, V, cfgs[r], states[r]) for r in range(n)]
            out.append(cur)
        dt = time.perf_counter() - t0
        kernels["rows_on_host"] = hip.last_sample_kernels()
        return dt, np.array(out, np.int32)

    kernels = {}
    routes = {"greedy": greedy, "sampled": sampled, "rows_on_host": rows_on_host}

    def leg(route, n):
        ctx.sync()
        dt, ids = routes[route](n)
        rollback(n)
        return dt, ids

    for n in ns:  # warm-up: every kernel shape of the timed window
        for r in routes:
            leg(r, n)
    times = {(r, n): [] for r in routes for n in ns}
    for _ in range(args.rounds):
        for n in ns:
            ids = {}
            for r in routes:
                dt, ids[r] = leg(r, n)
                times[(r, n)].append(dt)
            assert np.array_equal(ids["sampled"], ids["rows_on_host"]), f"n = {n}: the batched chain and one ps_hip_sample per row drew different ids"
            assert n < 2 or len({tuple(ids["sampled"][:, i]) for i in range(n)}) > 1, "every column drew the same text"
    rec = {"device": ctx.name(), "shape": f"{args.preset} {args.wtype} n_ctx {args.n_ctx}, every sequence forked from one prefill of {args.prompt_len} tokens",
           "steps": args.steps, "rounds": args.rounds, "chain": "reference default: top-k 40, temperature 0.8, top-p 0.95; seed + column",
           "timing": "host clock around calls that end in a stream synchronisation; median of the rounds, routes alternated in one process",
           "sample_kernels": kernels, "sampled_ids_equal_rows_on_host": True, "n": {}}
    for n in ns:
        e = {}
        for r in routes:
            t = sorted(times[(r, n)])
            med = t[len(t) // 2]
            e[r] = {"step_ms_median": round(med / args.steps * 1e3, 4), "step_ms_all": [round(x / args.steps * 1e3, 4) for x in times[(r, n)]],
                    "aggregate_tok_s": round(n * args.steps / med, 1)}
        e["sampled_minus_greedy_us_per_step"] = round((e["sampled"]["step_ms_median"] - e["greedy"]["step_ms_median"]) * 1e3, 1)
        e["sampled_over_greedy"] = round(e["sampled"]["aggregate_tok_s"] / e["greedy"]["aggregate_tok_s"], 4)
        e["sampled_over_rows_on_host"] = round(e["sampled"]["aggregate_tok_s"] / e["rows_on_host"]["aggregate_tok_s"], 4)
        rec["n"][str(n)] = e
    print(json.dumps(rec))
    if not args.no_json:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    m.close()
    ctx.close()


if __name__ == "__main__":
    main()
