"""Scoring a text at the headline shape: ps_hip_model_score against ps_hip_model_prefill on the same tokens (the floor: the same work minus lm_head and
scoring) and against the route without it (per-chunk forward with logits, the logits copied to the host, the host exact routine on every row), alternating
in one process.  Also a plain streaming read of the logits bytes of one launch sequence (torch's sum over as many floats, twice: the scoring kernels read
every row twice; in a child process), to set the scoring launches' times from a kernel trace against.  Writes one JSON record (default profiles/r10_bench_score.json).

    python tools/bench_score.py [--tokens 2048] [--chunk 128] [--rounds 3] [--out FILE | --no-json]
    rocprofv3 --kernel-trace -d DIR -o kt -- python tools/bench_score.py --trace-only       # one scored pass, nothing else
    python tools/prof_summary.py DIR/.../kt_results.db score_ > stats.txt; python tools/bench_score.py --kernel-stats stats.txt   # merge the per-launch times
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def streaming_read(n_floats):
    """microseconds for two plain reads of n_floats floats (what the first two scoring launches read)"""
    import torch
    x = torch.zeros(n_floats, dtype=torch.float32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(6):
        e0.record(); x.sum(); x.sum(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return round(float(np.median(ts[1:])), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streaming-read", type=int, default=0, help="internal: time two reads of that many floats with torch, print the microseconds, exit")
    ap.add_argument("--preset", default="llama-3.1-8b")
    ap.add_argument("--wtype", default="Q4_K")
    ap.add_argument("--n-ctx", type=int, default=4096)
    ap.add_argument("--tokens", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--max-batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--kernel-stats", help="tools/prof_summary.py output of a --trace-only run: its score_* lines go into the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_bench_score.json"))
    ap.add_argument("--no-json", action="store_true")
    args = ap.parse_args()
    if args.streaming_read:
        print(json.dumps(streaming_read(args.streaming_read)))
        return
    from powerserve_amd import gguf, hip, host, synth
    d = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"ps_bench_{args.preset}_{args.wtype}_{args.seed}")
    if not os.path.exists(os.path.join(d, ".done")) or synth.load_model_json(d)["llm_config"] != synth.llm_config(args.preset, args.n_ctx):
        synth.write_model_dir(d, args.preset, gguf.NAME_TYPE[args.wtype], n_ctx=args.n_ctx, seed=args.seed)
        open(os.path.join(d, ".done"), "w").write("ok")
    ctx = hip.Ctx(0)
    m = hip.Model(ctx, d, max_batch=args.max_batch, n_ctx=args.n_ctx)
    V, n, chunk = m.cfg.vocab_size, args.tokens, args.chunk
    toks = np.random.default_rng(args.seed).integers(0, V, n).astype(np.int32)
    tg = np.concatenate([toks[1:], [-1]]).astype(np.int32)

    def score():
        m.reset()
        t0 = time.perf_counter()
        rec = m.score(toks, tg, chunk)
        return time.perf_counter() - t0, rec

    def prefill():
        m.reset()
        t0 = time.perf_counter()
        m.prefill(toks, chunk)
        ctx.sync()
        return time.perf_counter() - t0, None

    def host_route():
        m.reset()
        out = np.zeros(n, np.float32)
        t0 = time.perf_counter()
        for c0 in range(0, n, chunk):
            c1 = min(n, c0 + chunk)
            lg, _ = m.forward(toks[c0:c1], np.arange(c0, c1), True)
            for i in range(c0, c1):
                if tg[i] >= 0:
                    out[i] = host.score_row_exact(lg[i - c0], int(tg[i]))
        return time.perf_counter() - t0, out

    if args.trace_only:
        score(); score()
        m.close(); ctx.close()
        return
    score(); prefill()  # warm-up: first use of every kernel
    legs = {"score": score, "prefill": prefill, "host_route": host_route}
    rates = {k: [] for k in legs}
    last = {}
    hip.score_counters(reset=True)
    for _ in range(args.rounds):
        for k, f in legs.items():
            dt, got = f()
            rates[k].append(n / dt)
            last[k] = got
    scored, exact, outside = hip.score_counters()
    med = {k: float(np.median(v)) for k, v in rates.items()}
    scored_rows = tg >= 0
    same = bool(np.array_equal(last["score"]["prob"][scored_rows].view(np.uint32), last["host_route"][scored_rows].view(np.uint32)))
    rec = {"shape": f"{args.preset} {args.wtype} n_ctx {args.n_ctx}", "tokens": n, "chunk": chunk, "max_batch": args.max_batch, "rounds": args.rounds,
           "tokens_per_s": {k: [round(x, 1) for x in v] for k, v in rates.items()}, "median_tokens_per_s": {k: round(v, 1) for k, v in med.items()},
           "score_over_prefill": round(med["score"] / med["prefill"], 4), "score_over_host_route": round(med["score"] / med["host_route"], 2),
           "probs_equal_host_route_bits": same, "rows_scored": scored, "rows_on_exact_path": exact, "rows_outside": outside,
           "exact_path_share": round(exact / max(scored, 1), 6)}
    # the streaming bound of one launch sequence's scoring: rows x vocab x 4 bytes, read twice.  torch carries a HIP runtime of its own, which finds no
    # device in a process where the library's runtime holds it: the read runs in a child process
    rows = min(n, args.max_batch // chunk * chunk)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--streaming-read", str(rows * V)], capture_output=True, text=True)
    if child.returncode != 0:
        sys.exit("bench_score: the streaming read failed\n" + child.stderr[-2000:])
    rec["streaming_read"] = {"rows": rows, "bytes_per_pass": rows * V * 4, "two_passes_us": json.loads(child.stdout.strip().splitlines()[-1]),
                             "how": "torch.sum over rows x vocab floats, twice, between events (median of 5 after a warm-up), in a process of its own"}
    if args.kernel_stats:
        ks = {}
        for line in open(args.kernel_stats):
            p = line.split()
            if p and p[0].startswith("score_") and len(p) >= 7:
                ks[p[0]] = {"calls": int(p[1]), "avg_us": float(p[3]), "min_us": float(p[4]), "max_us": float(p[5])}
        rec["score_kernels_per_launch"] = ks
        if ks:
            rec["score_launches_us_per_sequence"] = round(sum(v["avg_us"] for v in ks.values()), 1)
    print(json.dumps(rec))
    if not args.no_json:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    m.close()
    ctx.close()


if __name__ == "__main__":
    main()
