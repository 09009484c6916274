"""Perplexity of a token sequence, by the protocol of the reference's tool (app/perplexity/main.cpp:94-136): whole batches of --batch-size tokens only, one
forward with logits per batch on a growing cache, scoring from batch 18 on (PPL_START_ID) with the first token of that batch skipped, the target of position
pos is token pos + 1, a running perplexity printed per batch.  The probabilities come from ps_hip_model_score (bit for bit the reference's soft-max), the log,
the float sum and the exp from the PerplexityCalculator of the C++ facade.

    python tools/perplexity.py --model-dir DIR --tokens-file ids.txt [--batch-size 128]
    python tools/perplexity.py [--preset small-llama-hs128 --wtype Q4_K] --synthetic-ids 640 --batch-size 32            # parity path
    python tools/perplexity.py ... --chunk 1 --mode 8                                                                   # the fp16-KV mode on the same ids

--chunk (default: the batch size) is the size of the forwards a batch is fed in; 1 makes every token a single-token forward, which is where the fp16-KV decode
mode (--mode 8) acts.  On synthetic weights and ids the figure is near the vocabulary size and means nothing by itself: only the delta between two modes does.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PPL_START_ID = 18


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir")
    ap.add_argument("--preset", default="small-llama-hs128")
    ap.add_argument("--wtype", default="Q4_K")
    ap.add_argument("--tokens-file", help="whitespace-separated token ids")
    ap.add_argument("--synthetic-ids", type=int, default=0, help="that many seeded random ids instead of a file")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--mode", type=int, default=0, help="ps_hip_model_set_mode bits (8: fp16-KV decode mode)")
    ap.add_argument("--n-ctx", type=int, default=0)
    args = ap.parse_args()
    from powerserve_amd import gguf, hip, host, synth
    if args.tokens_file:
        ids = np.array(open(args.tokens_file).read().split(), dtype=np.int64)
    elif args.synthetic_ids > 0:
        ids = None
    else:
        ap.error("--tokens-file or --synthetic-ids")
    n_tokens = int(ids.size if ids is not None else args.synthetic_ids)
    bs = min(args.batch_size, n_tokens)
    if n_tokens < bs * PPL_START_ID:
        sys.exit(f"perplexity: {n_tokens} tokens are fewer than {PPL_START_ID} batches of {bs} (the reference asserts the same)")
    n_ctx = args.n_ctx or (n_tokens + 3) // 4 * 4
    d = args.model_dir
    if not d:
        d = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"ps_ppl_{args.preset}_{args.wtype}_{args.seed}_{n_ctx}")
        if not os.path.exists(os.path.join(d, ".done")):
            synth.write_model_dir(d, args.preset, gguf.NAME_TYPE[args.wtype], n_ctx=n_ctx, seed=args.seed)
            open(os.path.join(d, ".done"), "w").write("ok")
    chunk = args.chunk or bs
    ctx = hip.Ctx(0)
    m = hip.Model(ctx, d, max_batch=max(chunk, min(bs, 512)), n_ctx=n_ctx)
    V = m.cfg.vocab_size
    if ids is None:
        ids = np.random.default_rng(args.seed).integers(0, V, n_tokens)
    if ids.min() < 0 or ids.max() >= V:
        sys.exit("perplexity: token id outside the vocabulary")
    ids = ids.astype(np.int32)
    if args.mode:
        ctx.check(ctx.L.ps_hip_model_set_mode(m.h, args.mode))
    calc = host.PerplexityCalculator(V)
    hip.score_counters(reset=True)
    print(f"dataset: {n_tokens} tokens, batch_size {bs}, chunk {chunk}, mode {args.mode}, vocabulary {V}")
    pos, batch_id = 0, 1
    while pos + bs <= n_tokens:  # (a ragged last batch ends the loop, main.cpp:108-111)
        tg = np.full(bs, -1, np.int32)
        if batch_id >= PPL_START_ID:
            for i in range(bs):
                p = pos + i
                if p + 1 < n_tokens and p != (PPL_START_ID - 1) * bs:  # skip the first token
                    tg[i] = ids[p + 1]
        rec = m.score(ids[pos:pos + bs], tg, chunk)
        for i in range(bs):
            if tg[i] < 0:
                continue
            if rec["flags"][i] & hip.SCORE_OUTSIDE:
                sys.exit(f"perplexity: the logits of position {pos + i} hold a NaN or a +inf")
            calc.add(int(tg[i]), rec["prob"][i])
        if batch_id >= PPL_START_ID:
            print(f"ppl {calc.n_tokens}: {calc.current_ppl}")
        pos += bs
        batch_id += 1
    scored, exact, _ = hip.score_counters()
    print(json.dumps({"ppl": calc.current_ppl, "n_scored": calc.n_tokens, "logit_sum": calc.logit_sum, "batch_size": bs, "chunk": chunk, "mode": args.mode,
                      "rows_on_exact_path": exact, "rows_scored": scored, "synthetic": args.tokens_file is None and not args.model_dir}))
    calc.close()
    m.close()
    ctx.close()


if __name__ == "__main__":
    main()
