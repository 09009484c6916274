"""Batched decode at the headline shape: aggregate tokens/s of n sequences decoded together (ps_hip_model_decode_batch_greedy) against the
single-sequence decode_greedy of the same build, same process, alternated.  Every sequence sits behind its own prompt; after a leg its
sequences are rolled back, so every leg of every round decodes the same positions.  Also a ragged leg (prompts of 16 / 300 / 2048 / 4000
tokens in one batch) and, with --small, the same legs at the Llama-3.2-1B Q4_0 shape.  Writes one JSON record.

    python tools/bench_batch.py [--steps 64] [--rounds 3] [--small] [--out FILE | --no-json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_batch.py --only 8 --steps 8 --no-json     (per-launch times of the new kernels)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def model_dir(preset, wtype, n_ctx, seed):
    import bench
    from powerserve_amd import gguf, synth
    d = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"ps_bench_{preset}_{wtype}_{seed}")
    if not os.path.exists(os.path.join(d, ".done")) or synth.load_model_json(d)["llm_config"] != synth.llm_config(preset, n_ctx):
        bench.write_model(d, preset, gguf.NAME_TYPE[wtype], n_ctx, seed)
        open(os.path.join(d, ".done"), "w").write("ok")
    return d


def run_shape(ctx, preset, wtype, args, ns, ragged):
    from powerserve_amd import hip
    d = model_dir(preset, wtype, args.n_ctx, args.seed)
    m = hip.Model(ctx, d, max_batch=128, n_ctx=args.n_ctx)
    V = m.cfg.vocab_size
    rng = np.random.default_rng(args.seed)
    n_seq = max(ns) + (4 if ragged else 0)
    m.seq_reserve(n_seq)
    lens = [args.prompt_len] * max(ns) + ([16, 300, 2048, 4000] if ragged else [])
    first = []
    for s, n in enumerate(lens):
        p = rng.integers(0, V, n).astype(np.int32)
        m.seq_select(s)
        m.prefill(p[:-1], 128)
        first.append(int(p[-1]))
    ctx.sync()

    def rollback(seqs):
        for s in seqs:
            m.seq_select(s)
            m.kv_rollback(args.steps)
        ctx.sync()

    def leg(seqs, solo=False):
        if solo:
            m.seq_select(seqs[0])
            ctx.sync()
            t0 = time.perf_counter()
            ids = m.decode_greedy(first[seqs[0]], args.steps)  # (returns after its own stream synchronisation)
            dt = time.perf_counter() - t0
        else:
            ctx.sync()
            t0 = time.perf_counter()
            ids = m.decode_batch_greedy(seqs, [first[s] for s in seqs], args.steps)
            dt = time.perf_counter() - t0
        rollback(seqs)
        return dt, ids

    legs = {}
    for n in ns:
        legs[f"n{n}"] = (list(range(n)), n == 1 and not args.batch_path_for_1)
    if ragged:
        legs["ragged4"] = (list(range(max(ns), max(ns) + 4)), False)
    ref_ids = {}
    for name, (seqs, solo) in legs.items():  # warm-up: every kernel shape of the timed window, graph capture of the solo step
        _, ref_ids[name] = leg(seqs, solo)
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, (seqs, solo) in legs.items():
            dt, ids = leg(seqs, solo)
            assert np.array_equal(ids, ref_ids[name]), name  # the same positions decode to the same ids every round
            times[name].append(dt)
    # a batch column decodes what its sequence decodes alone (bits are the tests' business; ids are a cheap tripwire here)
    if "n1" in legs and len(ns) > 1:
        n2 = f"n{sorted(ns)[1]}"
        assert np.array_equal(np.asarray(ref_ids[n2])[:, 0], np.asarray(ref_ids["n1"]).reshape(-1)), "column 0 of a batch differs from the solo decode"
    out = {}
    for name, (seqs, solo) in legs.items():
        t = sorted(times[name])
        med = t[len(t) // 2]
        out[name] = {"sequences": len(seqs), "path": "decode_greedy" if solo else "decode_batch_greedy", "prompt_lens": [lens[s] for s in seqs],
                     "step_ms_median": round(med / args.steps * 1e3, 4), "step_ms_all": [round(x / args.steps * 1e3, 4) for x in times[name]],
                     "aggregate_tok_s": round(len(seqs) * args.steps / med, 1)}
    if "n1" in out:
        for name in out:
            out[name]["x_single_stream"] = round(out[name]["aggregate_tok_s"] / out["n1"]["aggregate_tok_s"], 3)
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ctx", type=int, default=4096)
    ap.add_argument("--prompt-len", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--only", type=int, default=0, help="one leg of n sequences only (kernel traces)")
    ap.add_argument("--batch-path-for-1", action="store_true", help="n = 1 through decode_batch_greedy instead of decode_greedy")
    ap.add_argument("--small", action="store_true", help="also the Llama-3.2-1B Q4_0 shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_bench_batch.json"))
    ap.add_argument("--no-json", action="store_true")
    args = ap.parse_args()
    from powerserve_amd import hip
    ctx = hip.Ctx(0)
    ns = [args.only] if args.only else [1, 2, 4, 8, 16]
    if args.only:
        args.batch_path_for_1 = True
    rec = {"device": ctx.name(), "steps": args.steps, "rounds": args.rounds, "n_ctx": args.n_ctx, "prompt_len": args.prompt_len,
           "timing": "host clock around a call that ends in a stream synchronisation; median of the rounds, legs alternated in one process",
           "llama-3.1-8b_Q4_K": run_shape(ctx, "llama-3.1-8b", "Q4_K", args, ns, ragged=not args.only)}
    if args.small and not args.only:
        rec["llama-3.2-1b_Q4_0"] = run_shape(ctx, "llama-3.2-1b", "Q4_0", args, ns, ragged=False)
    print(json.dumps(rec))
    if not args.no_json:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
