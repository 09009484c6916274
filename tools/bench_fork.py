"""Fork, save and restore at the headline shape: synthetic 8B Q4_K, n_ctx 4096, a 2 048-token prompt.

  fork         ps_hip_model_seq_fork of the prompt's slots to 1, 7 and 15 children: time per call and bytes moved per second (one read stream + k write streams)
  end to end   until 8 sequences stand behind the same prompt: one prefill + a fork to 7 children, against 8 prefills (the only way without the fork)
  state        ps_hip_model_seq_export / _import of the prompt's slots: host-buffer GB/s (pageable memory, as a caller's buffer is)

Legs alternate inside a round; every figure is the median of the rounds.  Writes one JSON record.

    python tools/bench_fork.py [--rounds 3] [--out FILE | --no-json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_fork.py --fork-only --no-json      (seq_fork_kernel's own time)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STREAM_TBS = (5.8, 5.9)  # what the project measured for a streaming kernel on this device: the yardstick of the fork's bytes/s, not a pass mark


def med(xs):
    return sorted(xs)[len(xs) // 2]


def timed(ctx, fn):
    """(host seconds around fn, which ends in a stream synchronisation; milliseconds between two events on the ctx stream around it)"""
    e0, e1 = ctx.event(), ctx.event()
    ctx.sync()
    ctx.record(e0)
    t0 = time.perf_counter()
    fn()
    dt = time.perf_counter() - t0
    ctx.record(e1)
    ms = ctx.elapsed_ms(e0, e1)
    for e in (e0, e1):
        ctx.check(ctx.L.ps_hip_event_destroy(ctx.h, e))
    return dt, ms


def plane_bytes(m, n_tokens):
    """one stream of a fork: K and V of every layer, n_tokens slots"""
    return m.cfg.n_layers * 2 * n_tokens * m.cfg.kv_dim * 4


def fork_legs(ctx, m, n_tokens, ks, rounds, src=0):
    """{k: record} for forks of sequence src's first n_tokens slots to k children (sequences src + 1 ..)"""
    times = {k: [] for k in ks}
    for k in ks:  # warm-up: the kernel's first launch, every destination's pages touched
        m.seq_fork(src, list(range(src + 1, src + 1 + k)), n_tokens)
    for _ in range(rounds):
        for k in ks:
            times[k].append(timed(ctx, lambda: m.seq_fork(src, list(range(src + 1, src + 1 + k)), n_tokens)))
    out = {}
    for k in ks:
        host_ms, ev_ms = med([t[0] for t in times[k]]) * 1e3, med([t[1] for t in times[k]])
        moved = (1 + k) * plane_bytes(m, n_tokens)
        out[f"children_{k}"] = {"bytes_moved": moved, "call_ms_median": round(host_ms, 4), "call_ms_all": [round(t[0] * 1e3, 4) for t in times[k]],
                                "event_ms_median": round(ev_ms, 4), "TB_per_s_call": round(moved / host_ms / 1e9, 3), "TB_per_s_event": round(moved / ev_ms / 1e9, 3),
                                "fraction_of_streaming_rate": round(moved / ev_ms / 1e9 / STREAM_TBS[0], 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ctx", type=int, default=4096)
    ap.add_argument("--prompt-len", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--fork-only", action="store_true", help="the fork legs only (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_bench_fork.json"))
    ap.add_argument("--no-json", action="store_true")
    args = ap.parse_args()
    from bench_batch import model_dir
    from powerserve_amd import hip
    ctx = hip.Ctx(0)
    m = hip.Model(ctx, model_dir("llama-3.1-8b", "Q4_K", args.n_ctx, args.seed), max_batch=128, n_ctx=args.n_ctx)
    m.seq_reserve(16)
    n = args.prompt_len
    prompt = np.random.default_rng(args.seed).integers(0, m.cfg.vocab_size, n).astype(np.int32)

    def prefill_into(s):
        m.seq_select(s)
        m.reset()
        m.prefill(prompt, 128)

    prefill_into(0)  # (also the warm-up of the prefill kernels)
    rec = {"device": ctx.name(), "shape": "llama-3.1-8b Q4_K (synthetic)", "n_ctx": args.n_ctx, "prompt_len": n, "rounds": args.rounds,
           "timing": "host clock around a call that ends in a stream synchronisation, and HIP events on the ctx stream around the same call; medians of the rounds, legs alternated",
           "bytes_per_stream": plane_bytes(m, n), "streaming_rate_TB_per_s_measured_by_the_project": list(STREAM_TBS),
           "fork": fork_legs(ctx, m, n, (1, 7, 15), args.rounds)}
    if not args.fork_only:
        # ---- until 8 sequences stand behind the prompt
        first = [int(t) for t in np.random.default_rng(args.seed + 1).integers(0, m.cfg.vocab_size, 8)]

        def with_fork():
            prefill_into(0)
            m.seq_fork(0, list(range(1, 8)), n)

        def eight_prefills():
            for s in range(8):
                prefill_into(s)

        ids, t = {}, {"prefill_and_fork": [], "eight_prefills": []}
        for r in range(args.rounds + 1):  # (round 0: warm-up)
            for name, fn in (("prefill_and_fork", with_fork), ("eight_prefills", eight_prefills)):
                dt, _ = timed(ctx, fn)
                got = m.decode_batch_greedy(list(range(8)), first, 4)  # a cheap tripwire (bits are the tests' business): both ways decode the same ids
                assert np.array_equal(ids.setdefault("ids", got), got), name
                if r:
                    t[name].append(dt)
        a, b = med(t["prefill_and_fork"]), med(t["eight_prefills"])
        rec["eight_sequences_behind_one_prompt"] = {"prefill_and_fork_ms": round(a * 1e3, 3), "eight_prefills_ms": round(b * 1e3, 3), "ratio": round(b / a, 3),
                                                    "required_ratio": 5.0, "all_ms": {k: [round(x * 1e3, 3) for x in v] for k, v in t.items()}}
        # ---- save / restore
        prefill_into(0)
        blob = m.seq_export(0, n)  # (warm-up; the blob that is imported)
        m.seq_import(1, blob)
        te, ti = [], []
        for _ in range(args.rounds):
            te.append(timed(ctx, lambda: m.seq_export(0, n))[0])
            ti.append(timed(ctx, lambda: m.seq_import(1, blob))[0])
        assert np.array_equal(m.seq_export(1, n), blob)
        rec["state"] = {"blob_bytes": int(blob.size), "export_ms": round(med(te) * 1e3, 2), "import_ms": round(med(ti) * 1e3, 2),
                        "export_GB_per_s": round(blob.size / med(te) / 1e9, 2), "import_GB_per_s": round(blob.size / med(ti) / 1e9, 2),
                        "note": "pageable host memory (a numpy array): the export figure includes allocating the blob"}
    print(json.dumps(rec))
    if not args.no_json:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    m.close()
    ctx.close()


if __name__ == "__main__":
    main()
