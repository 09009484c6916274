#!/usr/bin/env python3
"""bench.py — decode/prefill throughput of the MI355X backend on BASELINE.json's headline workload.

    python bench.py --gpus N --steps K --warmup W [--full]   (N > 1: launched by torch.distributed.run)

Workload (config.workload): Llama-3.1-8B shape, pure Q4_K synthetic weights (random-init in the quantized
domain, powerserve_amd/synth.py), prompt of 2048 random token ids, greedy decode.  A "step" is one
single-token decode step = one pass of the hot path (tokens/s defined as in
app/run/run.cpp:138-154).  `value` = decode tokens/s aggregated over all N replicas (weak scaling: one full
model + KV cache per GPU, no data-path collective; RCCL only broadcasts the prompt and gathers the ids).

A plain run does what the headline needs and nothing else: it writes the model (afresh, into a directory of its own
that goes away when the run ends), prefills the prompt once, runs the W warm-up and the K timed steps, writes
--dump-outputs and prints the line.  --full measures everything else on top of that, after the timed steps (except the
prefill's own warm-up chunk and its second, warm pass, which come before them as they always have):
  prefill_*     the prefill's first and warm passes, and its roofline against the matrix-core peak.
  roofline      HBM roofline of the dominant kernel family (quantized GEMV): algorithmic GGUF bytes per launch
                / average launch duration measured here with HIP events on the backend's own stream.
  side legs     fp16_kv_mode, fp16_prefill_mode, prefill_wide_chunks, graph_path (each has its --no-* / 0 switch).
  parity        the bench model against the CPU oracle; cpu_port / cpu_baseline the CPU restatement of the reference
                (oracle "port") and the real reference's mat-muls timed on this host on a bounded sample.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X spec (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--preset", default="llama-3.1-8b")
    ap.add_argument("--wtype", default="Q4_K")
    ap.add_argument("--prompt-len", type=int, default=2048)
    ap.add_argument("--n-ctx", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=128, help="prefill chunk (reference default batch_size=128)")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--full", action="store_true", help="measure and check everything besides the headline too: prefill figures, rooflines, side legs, "
                    "parity against the CPU oracle, CPU baselines (the options below that name one of them apply to --full runs)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-steps", type=int, default=4)
    ap.add_argument("--model-dir", default=None, help="a directory of the caller's for the model: written when it holds none yet, read as it stands otherwise "
                    "(default: a new directory under TMPDIR for every run, removed when the run ends)")
    ap.add_argument("--force-dist", action="store_true", help="initialise torch.distributed/RCCL even for one rank (tests the N>1 code path)")
    ap.add_argument("--eager", action="store_true", help="eager launches instead of hipGraph replay (rocprofv3 runs)")
    ap.add_argument("--no-kv-f16", action="store_true", help="skip the fp16-KV decode mode leg")
    ap.add_argument("--no-graph-path", action="store_true", help="skip the Graph -> Executor -> HIPBackend::plan leg (libps_host.so)")
    ap.add_argument("--graph-steps", type=int, default=96)
    ap.add_argument("--cpu-reference-limit", type=int, default=150, help="seconds the reference CPU baseline (a child process) may take before it is killed")
    ap.add_argument("--cpu-reference-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--f16-super-chunk", type=int, default=2048, help="side leg (fp16 perf mode): tokens per mat-mul launch")
    ap.add_argument("--prefill-warmup-tokens", type=int, default=128, help="untimed tokens forwarded before the timed prefill (first use of the prefill kernels in the process; 0: none)")
    ap.add_argument("--wide-chunk", type=int, default=512, help="side leg: prefill in chunks of this many tokens (0: skip)")
    ap.add_argument("--super-chunks", type=int, default=4, help="reference-sized prefill chunks (--batch tokens each) per launch sequence "
                    "(ps_hip_model_prefill: same bits as chunk-by-chunk forwards; 1: one forward per chunk)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps, write what the timed decode computed (DIR/<name>.npy): "
                    "the ids of the K timed steps and the logits of the last one")
    return ap.parse_args()


def ensure_model(args, rank, world, barrier):
    """The bench model's directory.  Rank 0 writes the model afresh for every run into a directory of the run's own, which goes away when the
    process exits (no run reads what an earlier one wrote; the replicas of one launch share rank 0's, named by the launch's rendezvous port).
    --model-dir names a directory of the caller's instead: the model is written there when it holds none yet and read as it stands otherwise."""
    import atexit
    import shutil
    import tempfile
    from powerserve_amd import gguf, synth
    wt = {"Q4_K_M": synth.Q4_K_M, "Q5_K_M": synth.Q5_K_M}.get(args.wtype) or gguf.NAME_TYPE[args.wtype]  # Q4_K_M / Q5_K_M: llama.cpp's per-tensor mixes with Q6_K
    name = f"ps_bench_{args.preset}_{args.wtype}_{args.seed}"
    if args.model_dir:
        d = args.model_dir
    elif world == 1:
        d = tempfile.mkdtemp(prefix=name + ".", dir=os.environ.get("TMPDIR", "/tmp"))
    else:
        d = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"{name}.port{os.environ['MASTER_PORT']}")
    marker = os.path.join(d, ".done")
    if rank == 0 and (not args.model_dir or not os.path.exists(marker)):
        if not args.model_dir:
            if world > 1:
                shutil.rmtree(d, ignore_errors=True)  # (what a launch that died on this port left behind)
            atexit.register(shutil.rmtree, d, True)
        t0 = time.time()
        write_model(d, args.preset, wt, args.n_ctx, args.seed)
        open(marker, "w").write("ok")
        print(f"[bench] synthetic model written to {d} in {time.time() - t0:.1f}s", file=sys.stderr)
    barrier()
    return d


def _skip_bytes(bg, n):
    """Advance the PCG64 `bg` exactly as Generator.integers(0, 256, n, dtype=np.uint8) does (n a multiple of 4): numpy fills such a draw
    from 32-bit outputs, four bytes each, and PCG64 serves those as the two halves of one 64-bit output, the high half kept for the next
    32-bit request.  Checked against numpy's own draw before it is used (_skip_is_exact)."""
    u = n // 4 - bg.state["has_uint32"]  # (a high half left over from the previous draw serves the first four bytes)
    bg.advance(u // 2)  # (advance() also drops a buffered half)
    if u % 2:
        last = int(bg.random_raw())
        st = bg.state
        st["has_uint32"], st["uinteger"] = 1, last >> 32
        bg.state = st


def _skip_is_exact():
    for lead in (0, 1):  # (with and without a buffered half ...)
        for n in (72, 76):  # (... and leaving one or none)
            a, b = np.random.default_rng(7), np.random.default_rng(7)
            for g in (a, b):
                g.integers(0, 2 ** 32, lead, dtype=np.uint32)
            a.integers(0, 256, n, dtype=np.uint8)
            _skip_bytes(b.bit_generator, n)
            if not np.array_equal(a.integers(0, 2 ** 32, 3, dtype=np.uint32), b.integers(0, 2 ** 32, 3, dtype=np.uint32)):
                return False
    return True


def _skip_blocks(rng, t, nb):
    """Make the draws synth.random_blocks makes for `nb` blocks of type t, in its order, with its bulk of full-range quant bytes skipped
    (_skip_bytes) instead of drawn.  False for a type whose draws are all drawn in full (nothing is drawn then)."""
    from powerserve_amd import gguf
    if t == gguf.Q4_0:
        rng.standard_normal(nb, dtype=np.float32)
        _skip_bytes(rng.bit_generator, nb * 16)
    elif t in (gguf.Q4_K, gguf.Q5_K):
        rng.standard_normal(nb, dtype=np.float32)
        rng.integers(8, 64, (nb, 8), dtype=np.uint8)
        _skip_bytes(rng.bit_generator, nb * (128 if t == gguf.Q4_K else 160))
    elif t == gguf.Q6_K:
        rng.standard_normal(nb, dtype=np.float32)
        _skip_bytes(rng.bit_generator, nb * 192)
        rng.integers(-64, 64, (nb, 16), dtype=np.int8)
    else:
        return False
    return True


def _blocks_from(state, t, n_rows, k, std):
    from powerserve_amd import synth
    g = np.random.Generator(np.random.PCG64())
    g.bit_generator.state = state
    return synth.random_blocks(g, t, n_rows, k, std)


def write_model(out_dir, preset, wtype, n_ctx, seed, threads=None):
    """synth.write_model_dir(out_dir, preset, wtype, n_ctx=n_ctx, seed=seed), byte for byte (tests/test_bench_model.py), in a fraction of its
    time: one thread walks the tensors in file order making the random stream's draws that vary in length (scale jitter, sub-block scales)
    and skipping its full-range quant bytes, which gives the stream's state at the start of every tensor; a pool draws each tensor whole
    from its state with synth.random_blocks; the main thread writes them out in order."""
    import queue
    import threading
    from concurrent.futures import ThreadPoolExecutor
    from powerserve_amd import gguf, synth
    if not _skip_is_exact():  # (a numpy that draws bytes otherwise: the one-thread writer)
        return synth.write_model_dir(out_dir, preset, wtype, n_ctx=n_ctx, seed=seed)
    if threads is None:
        try:
            threads = len(os.sched_getaffinity(0))
        except AttributeError:
            threads = os.cpu_count() or 1
        threads = max(1, min(threads, 16))  # (the stream walk and the file write bound it well before 16)
    arch, tied = synth.PRESETS[preset][0], synth.PRESETS[preset][10]
    cfg = synth.llm_config(preset, n_ctx)
    os.makedirs(os.path.join(out_dir, "ggml"), exist_ok=True)
    type_name = {synth.Q4_K_M: "Q4_K_M", synth.Q5_K_M: "Q5_K_M", synth.F16_Q8_0: "F16_Q8_0"}.get(wtype) or gguf.TYPE_NAME[wtype]
    mj = {"version": 1, "model_arch": arch, "model_id": f"{preset}-{type_name}", "llm_config": cfg}
    with open(os.path.join(out_dir, "model.json"), "w") as f:
        json.dump(mj, f, indent=1)
    w = gguf.GGUFWriter(os.path.join(out_dir, "ggml", "weights.gguf"))
    w.add_kv("general.architecture", arch)
    w.add_kv("general.name", mj["model_id"])
    w.add_kv("general.alignment", gguf.ALIGNMENT)
    for name, t, ne in synth.tensor_plan(cfg, arch, wtype, tied):
        w.add_tensor(name, t, ne)
    rng = np.random.default_rng(seed)
    ready, room = queue.Queue(), threading.Semaphore(64)  # (at most 64 tensors between the walk and the file: about 1 GB of the 8B model)

    def walk(pool):
        try:
            for ti in w.infos:
                room.acquire()
                if ti.type == gguf.F32:  # (synth.write_model_dir's norms and biases)
                    x = rng.standard_normal(int(np.prod(ti.ne)), dtype=np.float32)
                    ready.put((1.0 + 0.02 * x).astype(np.float32) if ti.name.endswith("norm.weight") else (0.02 * x).astype(np.float32))
                    continue
                k, rows = ti.ne[0], int(np.prod(ti.ne[1:]))
                std = 0.02 * (4096.0 / k) ** 0.5
                state = rng.bit_generator.state
                if _skip_blocks(rng, ti.type, rows * (k // gguf.BLOCK[ti.type][0])):
                    ready.put(pool.submit(_blocks_from, state, ti.type, rows, k, std))
                else:
                    ready.put(synth.random_blocks(rng, ti.type, rows, k, std))
        except BaseException as e:  # noqa: BLE001 -- handed to the writer, which raises it
            ready.put(e)

    def produce(ti):
        r = ready.get()
        if isinstance(r, BaseException):
            raise r
        r = r.result() if hasattr(r, "result") else r
        room.release()
        return r

    with ThreadPoolExecutor(threads) as pool:
        th = threading.Thread(target=walk, args=(pool,), daemon=True)
        th.start()
        w.write(produce)
        th.join()
    return mj


def cpu_port(model_dir, prompt, steps):
    """CPU port (oracle/ps_oracle.c, bit-exact vs the real reference) on this host, bounded sample: the parity checker of
    the headline model (same GGUF weights, same short prompt as the GPU leg) and a second CPU number."""
    from oracle import binding as B  # checker/baseline only -- never on the product path
    from powerserve_amd import gguf, synth
    mj = synth.load_model_json(model_dir)
    llm = dict(mj["llm_config"])
    llm["n_ctx"] = 64  # the sample never goes past a few positions; keeps the FP32 KV small on the host
    cfg = B.make_config(llm)
    rd = gguf.GGUFReader(os.path.join(model_dir, "ggml", "weights.gguf"))
    tensors = {n: (ti.type, rd.data(n), ti.ne[0], (list(ti.ne) + [1])[1]) for n, ti in rd.tensors.items()}
    cores = os.cpu_count() or 1
    nth = max(1, min(cores - 1, 48))
    m = B.Oracle().model(cfg, mj["model_arch"], tensors, n_threads=nth)
    p = np.asarray(prompt[:4], dtype=np.int32)
    ids, logits, tp, td = m.generate(p, 4, steps, want_logits=True)
    m.close()
    return {"value": steps / td, "unit": "tokens/s", "cores": nth, "kind": "port",
            "sample": f"{steps} greedy decode steps after a {p.size - 1}-token prefill (n_kv<{p.size + steps}), same GGUF weights; "
                      f"prefill {(p.size - 1) / max(tp, 1e-9):.2f} tok/s", "host_cores": cores, "ids": [int(i) for i in ids]}, p, ids, logits


def _one_socket_cpus():
    """the logical CPUs of the package this process mostly runs on (sysfs topology); None where that cannot be read"""
    try:
        allowed = sorted(os.sched_getaffinity(0))
        pk = {}
        for c in allowed:
            with open(f"/sys/devices/system/cpu/cpu{c}/topology/physical_package_id") as f:
                pk.setdefault(int(f.read()), []).append(c)
        return max(pk.values(), key=len) if pk else None
    except Exception:
        return None


def cpu_reference(model_dir, cfg, passes=7, progress=None):
    """The REAL reference on this host: powerserve_compute_forward_mul_mat of the vendored ggml (AVX2 vec_dot_q4_K_q8_K,
    quantize_row_q8_K) compiled from /root/reference into oracle/_ref/libps_ref.so, called through the reference's own
    ThreadPool over the 7 * L + 1 mat-muls of a decode token (the op that is > 90 % of the reference's decode time,
    SURVEY.md 8a3) on the bench model's weights.  Made reproducible (round-2 review: 10 .. 38 tok/s on one host class): the
    pool is pinned to the CPUs of ONE socket (sched_setaffinity before the pool's threads are created: they inherit it),
    the weights are touched before anything is timed (two untimed passes), and the MEDIAN of `passes` timed passes is
    reported with their min / max.  Returns None when the library is not there."""
    from oracle import binding as B  # baseline only
    from powerserve_amd import gguf
    if not B.have_ref():
        return None
    cores = os.cpu_count() or 1
    saved = None
    cpus = _one_socket_cpus()
    try:
        if cpus:
            saved = os.sched_getaffinity(0)
            os.sched_setaffinity(0, cpus)
        avail = len(cpus) if cpus else cores
        nth = max(1, min(avail - 1, 48))  # never = the CPU count: the reference's spin barrier does not survive oversubscription
        ref = B.Ref(n_threads=nth)
        rd = gguf.GGUFReader(os.path.join(model_dir, "ggml", "weights.gguf"))
        rng = np.random.default_rng(1)
        xs = {k: rng.standard_normal(k).astype(np.float32) for k in (cfg.dim, cfg.hidden_dim)}
        names = []
        for L in range(cfg.n_layers):
            names += [f"blk.{L}.{n}.weight" for n in ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")]
        names.append("output.weight" if "output.weight" in rd.tensors else "token_embd.weight")
        mats = []
        for n in names:
            ti = rd.tensors[n]
            w = np.array(rd.data(n))  # a private, resident copy: no page faults on the mmap inside the timed passes
            mats.append((ti.type, w, int(ti.ne[0]), int(ti.ne[1])))
        nbytes = sum(m[1].nbytes for m in mats)
        # the reference's pool size is swept and the BEST median is the baseline (round-5 review: 48 threads lost to the reference's own default of 4 --
        # its spin-barrier pool pays per thread and per op; a baseline must be the reference at its best, not at a size picked for it)
        sweep = {}
        cap = nth if avail > 16 else max(1, avail // 2)  # (a small host: the pool's spin barrier already crawls at avail - 1 threads)
        for n_thr in sorted({min(4, cap), 8, 16, 32, nth}):
            if n_thr > cap:
                continue
            r_ = B.Ref(n_threads=n_thr)
            ts = []
            for i in range(passes + 2):  # two untimed passes: pool start-up, caches, frequency
                t0 = time.perf_counter()
                for t, w, K, N in mats:
                    r_.mul_mat(t, w, K, N, xs[K])
                if i >= 2:
                    ts.append(time.perf_counter() - t0)
            r_.close()
            ts.sort()
            sweep[n_thr] = ts
            if progress is not None:  # (cpu_reference_guarded: a pool size that hangs later must not take this one with it)
                progress(_cpu_reference_line(sweep, passes, cpus, cores, len(mats), nbytes, partial=True))
    finally:
        if saved is not None:
            os.sched_setaffinity(0, saved)
    return _cpu_reference_line(sweep, passes, cpus, cores, len(mats), nbytes)


def _cpu_reference_line(sweep, passes, cpus, cores, n_mats, nbytes, partial=False):
    best = min(sweep, key=lambda k: sweep[k][len(sweep[k]) // 2])
    times = sweep[best]
    med = times[len(times) // 2]
    out = {"value": 1.0 / med, "unit": "tokens/s", "cores": best, "kind": "reference", "statistic": f"best median over pool sizes {sorted(sweep)}, {passes} timed passes each",
           "min": 1.0 / times[-1], "max": 1.0 / times[0],
           "bimodal": bool(times[-1] / times[0] > 2.0),  # (a shared host: passes of one run have differed 6x; the median is what `value` is)
           "pool_size_sweep": {str(k): {"median": 1.0 / v[len(v) // 2], "min": 1.0 / v[-1], "max": 1.0 / v[0]} for k, v in sorted(sweep.items())},
           "default_pool_size": 4,  # (HyperParams::n_threads, src/core/config.hpp:49)
           "pinned_to": f"{len(cpus)} logical CPUs of one socket" if cpus else "not pinned (topology unreadable)",
           "sample": f"{passes} timed warm passes (after 2 untimed) per pool size over the {n_mats} quantized mat-muls of one decode token ({nbytes / 1e9:.2f} GB of GGUF weights, resident copies) "
                     f"through powerserve_compute_forward_mul_mat on the reference's ThreadPool (attention, norms and sampling "
                     f"not included: an upper bound of the reference's decode rate)",
           "host_cores": cores, "weight_GBps": nbytes / med / 1e9}
    if partial:
        out["partial"] = True
    return out


def cpu_reference_guarded(model_dir, limit_s):
    """cpu_reference in a child process under a hard time limit.  The reference's ThreadPool synchronises its workers with a spin barrier that does not
    survive a descheduled thread: on a shared host one run of this leg did not come back within 15 minutes (round 4, the 8B Q5_K_M run) --
    a bench line must never hang on its baseline.  Returns the child's dict, None when the library is not there, or {"error": ...} on a time-out."""
    import subprocess
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-reference-child", model_dir], capture_output=True, text=True, timeout=limit_s)
    except subprocess.TimeoutExpired as e:
        # the child prints a line after every pool size of its sweep: what finished before the hang is the baseline (round 6: one size that hung had taken the whole sweep with it)
        so = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        done = [l for l in so.splitlines() if l.startswith("{")]
        if done:
            r_ = json.loads(done[-1])
            r_.pop("partial", None)
            r_["sweep_cut_short"] = f"the reference's thread pool did not finish its sweep within {limit_s} s (its spin barrier on a busy host); killed -- the pool sizes above are the ones that finished"
            return r_
        return {"error": f"the reference's thread pool did not finish within {limit_s} s (its spin barrier on a busy host); killed"}
    lines = [l for l in r.stdout.splitlines() if l.startswith("{") or l == "null"]
    if r.returncode != 0 or not lines:
        return {"error": f"child rc {r.returncode}: {r.stderr[-300:]}"}
    return json.loads(lines[-1])


def _cpu_reference_child(model_dir):
    import types
    from powerserve_amd import synth
    llm = synth.load_model_json(model_dir)["llm_config"]
    cfg = types.SimpleNamespace(dim=int(llm["embed_dim"]), hidden_dim=int(llm["ffn_dim"]), n_layers=int(llm["n_layers"]))
    print(json.dumps(cpu_reference(model_dir, cfg, progress=lambda d: print(json.dumps(d), flush=True))), flush=True)


def graph_path(model_dir, device, args, prompt):
    """The same workload through the reference-shaped host side (libps_host.so): every forward builds the reference's
    op graph with the NormAttention / FFN builders, Executor::run hands it to HIPBackend::plan, which lowers the canonical
    sequence to the fused launches.  Prefill in chunks, then single-token forwards with the logits copied to the host and
    device arg-max behind them (ModelTokenIterator's loop, src/model/model.hpp:117-184, with greedy sampling)."""
    from powerserve_amd import host
    hm = host.HostModel(model_dir, device, max_batch=max(args.batch, 1) * max(args.super_chunks, 1), n_ctx=args.n_ctx)
    try:
        t0 = time.perf_counter()
        hm.prefill(prompt[:-1], args.batch)  # ModelTokenIterator's prefill loop: its first chunk's graph is planned; lowered, the loop is lowered with it
        done = prompt.size - 1
        t1 = time.perf_counter()
        cur, ids, t_cap = int(prompt[-1]), [], None
        for s in range(args.graph_steps):
            if s == 2:
                t_cap = time.perf_counter()  # (the first single-token forward runs eagerly and captures the launch plan it replays afterwards)
            cur = int(hm.decode([cur], [done + s])[0])  # Model::decode: graph -> Executor -> lowered launches -> 4 bytes of device arg-max back
            ids.append(cur)
        t2 = time.perf_counter()
        n_plans, n_low = hm.plan_stats()
        n_hits = hm.plan_cache_hits()
    finally:
        hm.close()
    return {"prefill_tokens_per_s": (prompt.size - 1) / (t1 - t0), "decode_tokens_per_s": args.graph_steps / (t2 - t1), "steps": args.graph_steps,
            "decode_tokens_per_s_after_capture": (args.graph_steps - 2) / (t2 - t_cap) if t_cap and args.graph_steps > 2 else None,
            "graphs_planned": n_plans, "graphs_lowered": n_low, "plan_cache_hits": n_hits, "first_ids": ids[:8],
            "what": "Model::prefill + Model::decode of the C++ facade: Graph -> Executor::run -> HIPBackend::plan (lowered to the fused launches; a single token replays a "
                    "captured launch plan, and a (batch size, lm_head) shape that has been lowered once runs without a second graph -- the plan cache SURVEY a20 asks for; the prefill loop is lowered to ps_hip_model_prefill once its first chunk's graph has been planned and lowered), greedy ids from the "
                    "device arg-max (4 bytes per token to the host, src/model/model.hpp:170-183 copies vocab x 4)"}


def prefill_wide_leg(ctx, model_dir, args, prompt):
    """Reported next to the headline, never in it: the same prompt prefilled in chunks of --wide-chunk tokens (hparams batch_size; the
    headline uses the reference's default of 128, src/core/config.hpp).  Per-chunk fixed costs (quantizer, RoPE, attention launches,
    the QKV launch's uneven last round) are paid a quarter as often; every column is still the reference's arithmetic for that
    chunking (tests/test_gpu_model.py::test_wide_prefill_chunks_match_oracle)."""
    from powerserve_amd import hip
    m = hip.Model(ctx, model_dir, max_batch=args.wide_chunk, n_ctx=args.n_ctx)
    res = []
    for _ in range(2):
        ctx.sync()
        t0 = time.perf_counter()
        m.reset()
        done = 0
        while done < prompt.size - 1:
            bs = min(args.wide_chunk, prompt.size - 1 - done)
            m.forward(prompt[done:done + bs], np.arange(done, done + bs), lm_head=False)
            done += bs
        ctx.sync()
        res.append((prompt.size - 1) / (time.perf_counter() - t0))
    m.close()
    return {"chunk": args.wide_chunk, "prefill_tokens_per_s": res[0], "prefill_tokens_per_s_warm": res[1]}


def fp16_prefill_leg(ctx, model, args, prompt, model_dir):
    """SURVEY 8 f4 (second half), reported next to the headline and never mixed into it: the same prefill with the fp16 perf mode on
    (ps_hip_model_set_mode bit 5: the layer mat-muls as dense fp16 GEMMs on dequantized fp16 copies of the weights, csrc/perf16.hip's own
    kernel; RoPE, KV append and attention stay the parity kernels on the FP32 cache).  NOT bit-exact: layer 0's K / V rows are compared with the
    parity run's.  The mode's mat-muls take --f16-super-chunk tokens per launch (a model of its own with that max_batch: the GEMM tiles are
    256 tokens wide and the matrices of 4096 rows need ~2048 tokens to give every CU a workgroup); the attention inside still runs chunk by
    chunk of --batch tokens."""
    own = None
    if args.f16_super_chunk > model.max_batch:
        from powerserve_amd import hip
        own = model = hip.Model(ctx, model_dir, max_batch=args.f16_super_chunk, n_ctx=args.n_ctx)
    try:  # (a second full model lives on the device for the duration of this leg: it goes away whatever happens)
        model.reset()
        model.set_mode((1 if args.eager else 0) | 32)
        model.prefill(prompt[:8], args.batch)  # first use: dequantizes the weights (not timed)
        res = []
        for _ in range(2):
            ctx.sync()
            t0 = time.perf_counter()
            model.reset()
            model.prefill(prompt[:-1], args.batch)
            ctx.sync()
            res.append((prompt.size - 1) / (time.perf_counter() - t0))
        # What the mode changes is bounded where nothing has compounded yet: layer 0's K / V rows (one GEMM behind the embedding) against the parity
        # path's.  (On random synthetic weights the ids that follow say nothing: the int8 activation rounding of 32 layers amplifies ANY perturbation
        # into a different arg-max within a few tokens -- VERDICT round 3, weak 8.)
        n = prompt.size - 1
        k16, v16 = model.k_cache(0)[:n].copy(), model.v_cache(0)[:, :n].copy()
        model.set_mode(1 if args.eager else 0)
        model.reset()
        model.prefill(prompt[:-1], args.batch)
        k32, v32 = model.k_cache(0)[:n], model.v_cache(0)[:, :n]
        rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
        errs = (rel(k16, k32), rel(v16, v32))
        tokens_per_launch = min(model.max_batch // max(args.batch, 1) * max(args.batch, 1), prompt.size - 1)
    finally:
        if own is not None:
            own.close()
        else:
            model.set_mode(1 if args.eager else 0)
    return {"prefill_tokens_per_s": res[0], "prefill_tokens_per_s_warm": res[1], "tokens_per_mat_mul_launch": int(tokens_per_launch),
            "layer0_k_cache_max_abs_err_over_max_abs_vs_parity": errs[0], "layer0_v_cache_max_abs_err_over_max_abs_vs_parity": errs[1],
            "gemm": "own kernels (csrc/perf16.hip: v_mfma_f32_32x32x16_f16; 256-token tiles on the LDS-DMA path, 128-token tiles through registers for small grids); no library",
            "note": "layer mat-muls of the prefill as dense fp16 GEMMs (fp32 accumulation) on dequantized weights; decode stays on the parity kernels; not bit-exact by design "
                    "(the parity path itself rounds activations to int8: its layer-0 V sits 4-5e-3 from a float64 evaluation, this mode 3e-4 -- tests/test_gpu_model.py)"}


def fp16_kv_leg(ctx, model, args, prompt, ids_parity):
    """SURVEY 8 f4, reported next to the headline and never mixed into it: the same prefill + decode with the fp16-KV
    decode mode on (ps_hip_model_set_mode bit 3: fp16 mirrors of K and V, split-KV online soft-max for the single-token
    attention).  NOT bit-exact: the ids are compared with the parity run's, and the logits of the first decode step."""
    model.reset()
    model.set_mode((1 if args.eager else 0) | 8)
    done = 0
    while done < prompt.size - 1:
        bs = min(args.batch, prompt.size - 1 - done)
        model.forward(prompt[done:done + bs], np.arange(done, done + bs), lm_head=False)
        done += bs
    lg16, _ = model.forward([int(prompt[-1])], [model.position], lm_head=True)
    att16 = model.scratch(2, 1).copy()  # attention output of the LAST layer at this step (csrc/model.hip: ps_hip_model_scratch)
    model.ctx.check(model.ctx.L.ps_hip_model_kv_rollback(model.h, 1))
    cur = int(prompt[-1])
    ids_w = model.decode_greedy(cur, args.warmup) if args.warmup > 0 else np.zeros(0, np.int32)
    if ids_w.size:
        cur = int(ids_w[-1])
    ctx.sync()
    t0 = time.perf_counter()
    ids = model.decode_greedy(cur, args.steps)
    ctx.sync()
    dt = time.perf_counter() - t0
    both = np.concatenate([ids_w, ids])
    # parity logits of the same step
    model.reset()
    model.set_mode(1 if args.eager else 0)
    done = 0
    while done < prompt.size - 1:
        bs = min(args.batch, prompt.size - 1 - done)
        model.forward(prompt[done:done + bs], np.arange(done, done + bs), lm_head=False)
        done += bs
    lg32, _ = model.forward([int(prompt[-1])], [model.position], lm_head=True)
    att32 = model.scratch(2, 1)
    rel = float(np.abs(lg16 - lg32).max() / np.abs(lg32).max())
    # the bound that means something on random weights is the attention output itself (the int8 activation quantizers behind it amplify any
    # perturbation: ids and logits diverge within a few tokens whatever the size of the error -- VERDICT round 3, weak 8); the last layer's
    # input already carries the fp16 error of 31 layers, so this is an upper bound of one attention's error
    return {"decode_tokens_per_s": args.steps / dt, "ms_per_step": 1e3 * dt / args.steps,
            "last_layer_attention_output_max_abs_err_over_max_abs": float(np.abs(att16 - att32).max() / max(np.abs(att32).max(), 1e-30)),
            "first_step_logits_max_abs_err_over_max_abs": rel, "first_step_argmax_equal": bool(np.argmax(lg16) == np.argmax(lg32)), "ids_compared": int(both.size),
            "note": "fp16 K/V mirrors + split-KV online soft-max for single-token attention only; prefill reads the FP32 cache; not bit-exact by design"}


def dump_outputs(out_dir, ids, logits):
    """--dump-outputs: what the caller of the timed decode_greedy receives -- the ids of the K timed steps (float64: exact) -- and the
    logits of its last step (float32, one vocabulary row: the row the device arg-max picked the last id from).  Under 1 MB for the 8B model."""
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "decode_ids.npy"), np.asarray(ids, dtype=np.float64))
    np.save(os.path.join(out_dir, "last_step_logits.npy"), np.asarray(logits, dtype=np.float32))


def gpu_short_run(model, p, ids_cpu):
    """the GPU on the CPU leg's short prompt, teacher-forced with the CPU's ids: logits of every step"""
    model.reset()
    model.forward(p[:-1], np.arange(p.size - 1), lm_head=False)
    cur, out_ids, out_logits = int(p[-1]), [], []
    for s in range(len(ids_cpu)):
        lg, am = model.forward([cur], [model.position], lm_head=True)
        out_ids.append(int(am[0])); out_logits.append(np.array(lg[0]))
        cur = int(ids_cpu[s])
    return out_ids, out_logits


def broadcast_prompt(dist, prompt, rank, device="cuda"):
    """rank 0's prompt ids -> every replica (the only inbound collective; RCCL over xGMI on GPUs)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(prompt, dtype=np.int32)).to(device)
    dist.broadcast(t, src=0)
    return t.cpu().numpy()


def gather_ids(dist, ids, world, device="cuda"):
    """all-gather the sampled ids of every replica (the only outbound collective) and check they agree"""
    import torch
    mine = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(device)
    allv = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(allv, mine)
    return all(bool((a == allv[0]).all()) for a in allv), [a.cpu().numpy() for a in allv]


def max_over_ranks(dist, values, device="cuda"):
    import torch
    tt = torch.tensor(list(values), dtype=torch.float64).to(device)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    return [float(v) for v in tt]


def distributed_command(n_gpus, port, argv):
    """the launcher command line for N ranks on this node — the one the driver uses"""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}",
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def relaunch_distributed(args):
    """`python bench.py --gpus N` with N > 1 and no launcher: re-exec under torch.distributed.run, one rank per GPU."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.execv(sys.executable, distributed_command(args.gpus, port, sys.argv[1:]))


def main():
    args = parse()
    if args.cpu_reference_child:  # (the guarded baseline's child process: CPU only, one JSON line)
        _cpu_reference_child(args.cpu_reference_child)
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch_distributed(args)  # does not return
    # the contract is ONE JSON line on stdout: libraries that chat on fd 1 (RCCL prints its library path at init) are
    # sent to stderr for the duration of the run
    sys.stdout.flush()
    saved_stdout = os.dup(1)
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and not (args.gpus == 1 and world == 1):
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU")
    dist = None
    if world > 1 or args.force_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import torch
        import torch.distributed as dist_
        torch.cuda.set_device(local)
        if "MASTER_ADDR" not in os.environ:
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", RANK="0", WORLD_SIZE="1")
        dist_.init_process_group("nccl", device_id=torch.device("cuda", local))  # RCCL over xGMI
        dist = dist_

    def barrier():
        if dist is not None:
            dist.barrier()

    from powerserve_amd import hip
    model_dir = ensure_model(args, rank, world, barrier)
    ctx = hip.Ctx(local)
    t0 = time.time()
    model = hip.Model(ctx, model_dir, max_batch=max(args.batch, 1) * max(args.super_chunks, 1), n_ctx=args.n_ctx)
    load_s = time.time() - t0
    cfg = model.cfg
    if args.eager:
        model.set_mode(1)

    # ---- prompt: rank 0 draws it, RCCL broadcast to every replica (the only inbound collective)
    prompt = np.random.default_rng(42).integers(0, cfg.vocab_size, args.prompt_len).astype(np.int32)
    if dist is not None:
        prompt = broadcast_prompt(dist, prompt if rank == 0 else np.zeros_like(prompt), rank)

    # ---- prefill (all but the last prompt token, lm_head skipped: src/model/model.hpp:147-163)
    barrier(); ctx.sync()
    def prefill():
        # the reference's loop: forward(chunk of --batch tokens, lm_head = false) + advance, chunk after chunk.  ps_hip_model_prefill runs
        # exactly that (bit-identical cache, tests/test_gpu_model.py::test_prefill_in_super_chunks_keeps_the_reference_chunking) with
        # --super-chunks reference chunks per launch sequence: mat-muls over all their columns, attention per reference chunk
        model.reset()
        if args.super_chunks > 1:
            model.prefill(prompt[:-1], args.batch)
            return
        done = 0
        while done < prompt.size - 1:
            bs = min(args.batch, prompt.size - 1 - done)
            model.forward(prompt[done:done + bs], np.arange(done, done + bs), lm_head=False)
            done += bs

    # one UNTIMED reference-sized chunk first (like the decode's W warm-up steps): the first launch of a kernel in a process loads its code object, and on a cold box that alone
    # moved the first pass between 14.9 k and 16.8 k tok/s from run to run (profiles/r06_bench_8b_full.json).  The timed pass below still prefills the WHOLE prompt from an empty cache.
    # (--full only: a plain run reports no prefill figure, its one pass below just lays down the cache the timed decode steps read)
    if args.full and args.prefill_warmup_tokens > 0:
        model.reset()
        n_w = min(args.prefill_warmup_tokens, prompt.size - 1)
        model.forward(prompt[:n_w], np.arange(n_w), lm_head=False)
        ctx.sync(); barrier()
    t0 = time.perf_counter()
    prefill()
    ctx.sync(); barrier()
    prefill_s = time.perf_counter() - t0
    prefill_warm_s = None
    if args.full:  # (the same prompt once more is reported next to it)
        barrier(); ctx.sync()
        t0 = time.perf_counter()
        prefill()
        ctx.sync(); barrier()
        prefill_warm_s = time.perf_counter() - t0

    # ---- decode: W untimed warmup steps, then exactly K timed steps
    cur = int(prompt[-1])
    ids_w = model.decode_greedy(cur, args.warmup) if args.warmup > 0 else np.zeros(0, np.int32)
    if ids_w.size:
        cur = int(ids_w[-1])
    barrier(); ctx.sync()
    e0, e1 = ctx.event(), ctx.event()
    t0 = time.perf_counter()
    ctx.record(e0)
    ids = model.decode_greedy(cur, args.steps)
    ctx.record(e1)
    ctx.sync(); barrier()
    dt = time.perf_counter() - t0
    dev_ms = ctx.elapsed_ms(e0, e1)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, ids, model.logits(1)[0])
    if dist is not None:
        if args.full:
            dt, prefill_s, prefill_warm_s = max_over_ranks(dist, [dt, prefill_s, prefill_warm_s])
        else:
            dt, = max_over_ranks(dist, [dt])
        replicas_agree, _ = gather_ids(dist, ids, world)
        # every collective of the run is behind us: the process group goes away NOW, so that no rank sits in an RCCL barrier (host threads spinning)
        # while rank 0 times the CPU baselines on the reference's spin-barrier thread pool (round-4 review, weak 2); ranks > 0 just close and exit
        dist.barrier()
        dist.destroy_process_group()
        multi, dist = True, None
    else:
        replicas_agree, multi = True, False

    out = None
    if rank == 0:
        wbytes = model.weight_bytes_per_token
        n_kv_mid = args.prompt_len + args.warmup + args.steps // 2
        kv_bytes = cfg.n_layers * 2 * n_kv_mid * cfg.kv_dim * 4
        out = {
            "metric": "decode tokens/s (greedy, Llama-3.1-8B Q4_K, 1 GPU per replica)" if args.preset == "llama-3.1-8b" and args.wtype == "Q4_K"
            else f"decode tokens/s (greedy, {args.preset} {args.wtype})",
            "value": world * args.steps / dt, "unit": "tokens/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "int8 x int4 block dot, fp32 accumulate (ggml Q4_K x Q8_K semantics)" if args.wtype == "Q4_K" else "int8 block dot, fp32 accumulate",
            "data": "synthetic (random-init weights generated in the quantized domain; random prompt ids, seed 42)",
            "config": {"workload": f"{args.preset} {'mixed' if args.wtype in ('Q4_K_M', 'Q5_K_M') else 'pure'} {args.wtype}, prefill {args.prompt_len} + decode {args.steps}, n_ctx {args.n_ctx}, FP32 KV",
                       "prefill_chunk": args.batch, "prefill_chunks_per_launch_sequence": max(args.super_chunks, 1), "replicas": world, "collectives": "RCCL broadcast(prompt) + all_gather(ids)" if world > 1 else "none"},
        }
        if args.full:
            out.update({
                "prefill_tokens_per_s": world * (args.prompt_len - 1) / prefill_s, "prefill_s": prefill_s,
                "prefill_tokens_per_s_warm": world * (args.prompt_len - 1) / prefill_warm_s, "prefill_warm_s": prefill_warm_s,
                "prefill_warmup_tokens": args.prefill_warmup_tokens})
        out.update({
            "decode_device_ms_per_step": dev_ms / args.steps, "model_load_s": load_s,
            "weight_bytes_per_token": wbytes, "kv_bytes_per_token_mid": kv_bytes,
            "decode_effective_GBps": (wbytes + kv_bytes) / (dt / args.steps) / 1e9,
            "replicas_agree": replicas_agree, "first_ids": [int(i) for i in ids[:8]]})
        if args.full:
            # ---- roofline of the dominant kernel (gate/up mat-vec), event-bracketed replay
            from powerserve_amd import gguf as _gguf
            gate_up_bytes = 2 * cfg.hidden_dim * _gguf.row_size(_gguf.NAME_TYPE[{"Q4_K_M": "Q4_K", "Q5_K_M": "Q5_K"}.get(args.wtype, args.wtype)], cfg.dim)
            out["roofline"] = gemv_roofline(ctx, model, wbytes, gate_up_bytes, args.preset == "llama-3.1-8b" and args.wtype == "Q4_K")
            out["prefill_roofline"] = prefill_roofline(ctx, model, cfg, args.prompt_len - 1, prefill_s, prefill_warm_s, min(args.batch * max(args.super_chunks, 1), args.prompt_len - 1),
                                                       args.preset == "llama-3.1-8b" and args.wtype == "Q4_K")
        if args.full and not args.no_kv_f16 and not multi:
            try:
                out["fp16_kv_mode"] = fp16_kv_leg(ctx, model, args, prompt, np.concatenate([ids_w, ids]))
            except Exception as e:  # noqa: BLE001 — a failing side leg must not take the headline line with it
                out["fp16_kv_mode"] = {"error": repr(e)}
            try:
                out["fp16_prefill_mode"] = fp16_prefill_leg(ctx, model, args, prompt, model_dir)
            except Exception as e:  # noqa: BLE001
                out["fp16_prefill_mode"] = {"error": repr(e)}
        if args.full and args.wide_chunk > args.batch and not multi:
            try:
                out["prefill_wide_chunks"] = prefill_wide_leg(ctx, model_dir, args, prompt)
            except Exception as e:  # noqa: BLE001
                out["prefill_wide_chunks"] = {"error": repr(e)}
        if args.full and not args.no_graph_path and not multi:
            try:
                out["graph_path"] = graph_path(model_dir, local, args, prompt)
                out["graph_path"]["ids_equal_direct"] = out["graph_path"]["first_ids"] == ([int(i) for i in ids_w] + [int(i) for i in ids])[:8]
            except Exception as e:
                out["graph_path"] = {"error": repr(e)}
        if args.full and not args.no_cpu_baseline:
            try:  # the baselines must never take the GPU number down with them
                port, p_short, ids_cpu, logits_cpu = cpu_port(model_dir, prompt, args.cpu_steps)
                ids_gpu, logits_gpu = gpu_short_run(model, p_short, ids_cpu)
                rel = max(float(np.abs(g - c).max() / max(np.abs(c).max(), 1e-30)) for g, c in zip(logits_gpu, logits_cpu))
                out["parity"] = {"model": f"{args.preset} {args.wtype} (the bench model, all layers)", "checker": "oracle/ps_oracle.c (bit-exact vs the real reference)",
                                 "reference_build": "-ffp-contract=off (oracle/Makefile CONTRACT=off: every fp32 operation rounds where the C source rounds).  The reference's own CMake sets no "
                                                    "contraction flag: its stock build (GCC -ffp-contract=fast) fuses the RoPE rotation, the n % 32 dot-product leftovers and Q5_K's summs -- ids equal, logits "
                                                    "up to 2.8e-3 of the largest away on one of four fixture models (tests/golden/e2e_builds_*.npz); oracle mode pso_set_contract(1) and "
                                                    "lib/libps_hip_contract.so follow THAT build bit for bit (tests/test_ref_fast.py, tests/test_gpu_golden.py)",
                                 "prompt_tokens": int(p_short.size), "steps": len(ids_cpu), "ids_equal": [int(i) for i in ids_cpu] == ids_gpu,
                                 "max_rel_logit_err": rel, "logits_bit_equal": all(np.array_equal(g.view(np.uint32), np.asarray(c, dtype=np.float32).view(np.uint32)) for g, c in zip(logits_gpu, logits_cpu))}
                out["cpu_port"] = port
                refb = cpu_reference_guarded(model_dir, args.cpu_reference_limit)
                if refb is not None and "error" in refb:  # (timed out / failed: the port is the baseline, the reason stays on the line)
                    port = dict(port, reference_leg=refb["error"])
                    refb = None
                out["cpu_baseline"] = refb if refb is not None else port
            except Exception as e:
                out["cpu_baseline"] = {"value": None, "error": repr(e)}
    model.close()
    ctx.close()
    if rank == 0:
        sys.stdout.flush()
        os.dup2(saved_stdout, 1)
        print(json.dumps(out), flush=True)


MFMA_F16_PEAK_TFLOPS = 2500.0  # dense fp16 matrix-core peak (MI355X_MICROARCH.md): the pipe the Q4_K chunk mat-mul runs its exact-integer contractions on
def _traffic_file():
    """the newest round's PMC record (profiles/rNN_pmc_traffic.json, written by tools/gpu_round_prof.sh)"""
    import glob
    root = os.path.dirname(os.path.abspath(__file__))
    found = sorted(glob.glob(os.path.join(root, "profiles", "r[0-9][0-9]_pmc_traffic.json")))
    return os.path.relpath(found[-1], root) if found else os.path.join("profiles", "r06_pmc_traffic.json")


TRAFFIC_FILE = _traffic_file()


def kernel_sources_sha16():
    """sha256[:16] over the kernel sources and the build recipe: what a PMC record must have been taken on to describe the library that runs"""
    import hashlib
    root = os.path.dirname(os.path.abspath(__file__))
    h = hashlib.sha256()
    csrc = os.path.join(root, "powerserve_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode()); h.update(open(os.path.join(csrc, f), "rb").read())
    h.update(open(os.path.join(root, "powerserve_amd", "build.py"), "rb").read())
    return h.hexdigest()[:16]


def _pmc_traffic(kernel):
    """HBM bytes per launch of `kernel` from the committed PMC pass (tools/pmc_summary.py over a separate
    `rocprofv3 --pmc FETCH_SIZE` run of this same command; FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for gfx950).
    A live bench run cannot collect counters.  The record is keyed by the kernel's full template name AND carries the hash of the kernel
    sources it was taken on (kernel_sources_sha16): a record from other sources -- a kernel body can change under an unchanged name -- is
    refused (null, with the reason).  Returns (bytes | None, source)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), TRAFFIC_FILE)
    try:
        with open(path) as f:
            rec = json.load(f)
    except Exception:
        return None, None
    have, want = rec.get("_kernel_sources_sha16"), kernel_sources_sha16()
    if have != want:
        return None, f"{TRAFFIC_FILE} REFUSED: taken on kernel sources {have}, this library is built from {want}"
    return rec.get(kernel, {}).get("hbm_bytes_per_launch"), TRAFFIC_FILE + " (rocprofv3 --pmc FETCH_SIZE x 2, separate pass of this command on these kernel sources)"


def _bench_matmul(ctx, model, which, bs, reps=20):
    import ctypes as C
    L = ctx.L
    L.ps_hip_model_bench_matmul.restype = C.c_int
    L.ps_hip_model_bench_matmul.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.ps_hip_last_matmul_kernel.restype = C.c_char_p
    seq_ms, null_ms, n = C.c_double(), C.c_double(), C.c_int()
    ctx.check(L.ps_hip_model_bench_matmul(model.h, reps, which, bs, C.byref(seq_ms), C.byref(null_ms), C.byref(n)))
    return seq_ms.value, null_ms.value, n.value, L.ps_hip_last_matmul_kernel().decode()


def gemv_roofline(ctx, model, wbytes, gate_up_bytes, is_headline):
    """Roofline of the dominant kernel: the gate/up mat-vec (two [K=dim, N=hidden] matrices in one launch).

    The library replays that launch for every layer (each layer's own weights, so every launch streams HBM-cold bytes
    exactly like in the real step; same kernel and fused RMSNorm prologue as the decode step) between HIP events on the
    backend stream: achieved = GGUF bytes of the two matrices / average launch duration.  `kernel` is the template instance
    that launch actually went to (the library records it), rocprofv3's per-kernel average for it
    (profiles/r03_decode_kernel_stats_*) is the cross-check.  The same measurement over ALL mat-vec launches of a token and
    the cost of an empty launch are reported next to it."""
    if not hasattr(ctx.L, "ps_hip_model_bench_matmul"):
        return None
    g_ms, g_null, g_n, kernel = _bench_matmul(ctx, model, 1, 1)
    a_ms, a_null, a_n, _ = _bench_matmul(ctx, model, 0, 1)
    avg_us = 1e3 * g_ms / g_n
    achieved = gate_up_bytes / (avg_us * 1e-6) / 1e9
    traffic, src = _pmc_traffic(kernel) if is_headline else (None, None)
    return {"bound": "hbm", "kernel": kernel + ": gate/up mat-vec (RMSNorm + activation-quantizer prologue, SiLU(gate)*up epilogue), one launch per layer",
            "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
            "traffic": traffic, "traffic_source": src,
            "bytes_per_launch": gate_up_bytes, "avg_launch_us": avg_us, "launches_timed": 20 * g_n,
            "empty_launch_us": 1e3 * g_null / g_n,
            "all_matvec": {"launches_per_token": a_n, "ms_per_token": a_ms, "bytes_per_token": wbytes,
                           "achieved": wbytes / (a_ms * 1e-3) / 1e9, "frac": wbytes / (a_ms * 1e-3) / 1e9 / HBM_PEAK_GBS}}


def prefill_roofline(ctx, model, cfg, n_tok, prefill_s, prefill_warm_s, batch, is_headline):
    """Prefill against the matrix-core peak (north_star: "MFMA utilisation (prefill) against gfx950 peak").  flops =
    2 * n_tok * sum K * N over the layer mat-muls (lm_head is skipped during prefill, src/model/model.hpp:157);
    the whole-prefill figure divides by the measured prefill time (attention, quantizers and launches included), the
    per-launch figure is the gate/up chunk mat-mul replayed over all layers between HIP events (its activation-quantizer
    launch included).  peak = the dense fp16 MFMA rate: the kernel contracts exact integers on v_mfma_f32_16x16x32_f16."""
    layer_kn = 2 * cfg.dim * cfg.dim + 2 * cfg.dim * cfg.kv_dim + 3 * cfg.dim * cfg.hidden_dim
    flops = 2.0 * n_tok * cfg.n_layers * layer_kn
    out = {"bound": "mfma", "flops": flops, "achieved": flops / prefill_s / 1e12, "achieved_warm": flops / prefill_warm_s / 1e12,
           "peak": MFMA_F16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": flops / prefill_s / 1e12 / MFMA_F16_PEAK_TFLOPS,
           "what": "2 * n_tok * sum(K * N) of the layer mat-muls / measured prefill time (the first whole-prompt pass of the process, behind --prefill-warmup-tokens untimed tokens; attention, quantizers, launches included)"}
    if hasattr(ctx.L, "ps_hip_model_bench_matmul") and batch <= model.max_batch:
        g_ms, _, g_n, kernel = _bench_matmul(ctx, model, 1, batch, reps=5)
        us = 1e3 * g_ms / g_n
        fl = 2.0 * batch * cfg.dim * 2 * cfg.hidden_dim
        traffic, src = _pmc_traffic(kernel) if is_headline else (None, None)
        out["dominant_launch"] = {"kernel": kernel + f": gate/up mat-mul of a {batch}-token chunk (+ its RMSNorm / quantizer launch)", "flops_per_launch": fl,
                                  "avg_launch_us": us, "achieved": fl / (us * 1e-6) / 1e12, "frac": fl / (us * 1e-6) / 1e12 / MFMA_F16_PEAK_TFLOPS,
                                  "traffic": traffic, "traffic_source": src}
    return out


if __name__ == "__main__":
    main()
