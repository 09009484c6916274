#!/usr/bin/env python3
"""Golden vectors of the F16 weight path, made by the real reference (oracle/_ref, built by oracle.binding.build(ref=True)):

  tests/golden/f16_mul_mat.npz      (outputs + input sha256; inputs from mul_mat_inputs) powerserve_compute_forward_mul_mat with an F16 src0 (ggml_fp32_to_fp16_row + ggml_vec_dot_f16) for
                                    K in {99, 100, 256, 896, 4096, 4100} x bs in {1, 2, 3, 17}; the activations hold values that overflow fp16
                                    (|x| >= 65520: one per column, so the sums are +-inf, never NaN), fp16 subnormals and fp16 ties
  tests/golden/e2e_f16_<case>.npz   LlamaModel / Qwen2Model::forward on synthetic models (powerserve_amd/synth.py; the GGUF's sha256 is
                                    recorded, the GPU test regenerates the file): ids of a greedy run, per-step logits, batch logits
  tests/golden/tree_forward_f16.npz a branching token-tree forward through oracle/ref_ops_forward.py, in the form of tree_forward.npz

Seeded: every run writes the same bytes (tests/test_f16_weights.py checks that where oracle/_ref exists).
    python tools/gen_golden_f16.py [out_dir]
"""
import hashlib
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import binding as B  # noqa: E402
from powerserve_amd import gguf, synth  # noqa: E402

MUL_K = (99, 100, 256, 896, 4096, 4100)  # 99: one chain per lane (2-byte loads); 100, 4100: K % 8 == 4 (8-byte loads)
MUL_BS = (1, 2, 3, 17)
MUL_N = 40
# (name, preset, weight type, token_embd type or None = the weight type)
E2E = (("tiny-llama_F16", "tiny-llama", synth.F16, B.F32),   # untied, every matrix F16, F32 embedding (the reference cannot look up F16 rows)
       ("tiny-qwen2_F16", "tiny-qwen2", synth.F16, B.Q8_0),  # F16 layers, tied Q8_0 embedding / lm_head
       ("tiny-llama_F16_Q8_0", "tiny-llama", synth.F16_Q8_0, B.F32))  # F16 attention + output, Q8_0 FFN
TREE_CASE = ("tiny-llama", synth.F16, B.F32, 96, 37)
# a branching 12-node token tree (node -> parent), the shape of tests/golden/tree_forward.npz's
TREE_PARENT = (-1, 0, 0, 0, 1, 1, 2, 4, 7, 6, 8, 3)


def tree_mask():
    """[n][n] uint8: node i sees itself and its ancestors; and each node's depth"""
    n = len(TREE_PARENT)
    mask, depth = np.zeros((n, n), dtype=np.uint8), np.zeros(n, dtype=np.int64)
    for i in range(n):
        j = i
        while j >= 0:
            mask[i, j] = 1
            j = TREE_PARENT[j]
        depth[i] = int(mask[i].sum()) - 1
    return mask, depth


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def save(path, **arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same file bytes"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.save(b, np.asanyarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, b.getvalue())
    with open(path, "wb") as f:
        f.write(buf.getvalue())


def special_activations(rng, bs, K):
    x = rng.standard_normal((bs, K)).astype(np.float32)
    x[:, ::7] *= 1e-5                                     # fp16 subnormals (< 6.1e-5)
    x[:, 3::11] = np.float32(1.0 + 2.0 ** -11)            # exactly halfway between two fp16 values: ties to even
    x[:, 5::13] = np.float32(1.0 + 3 * 2.0 ** -11)        # the other side of a tie
    x[:, 1::17] = np.float32(2.0 ** -25)                  # half the smallest subnormal: ties to zero
    for j in range(bs):
        if j % 2 == 1:                                    # every second column: one element beyond the fp16 range
            x[j, (31 * j + 2) % K] = np.float32(65520.0 if j % 4 == 1 else -70000.0)
    return x


def mul_mat_inputs(K, bs):
    """the weights and activations of one mul_mat case (seeded per case: the GPU test rebuilds them, the fixture keeps their sha256)"""
    rng = np.random.default_rng([1601, K, bs])
    return synth.random_blocks(rng, B.F16, MUL_N, K, std=0.5), special_activations(rng, bs, K)


def mul_mat(r):
    d = {}
    for K in MUL_K:
        for bs in MUL_BS:
            w, x = mul_mat_inputs(K, bs)
            key = f"{K}_{bs}"
            d["sha_" + key] = hashlib.sha256(w.tobytes() + x.tobytes()).hexdigest()
            d["y_" + key] = r.mul_mat(B.F16, w, K, MUL_N, x)
    return d


def e2e(r, rf, preset, wt, et):
    with tempfile.TemporaryDirectory() as td:
        mj = synth.write_model_dir(td, preset, wt, n_ctx=128, seed=1616, embd_type=et)
        path = os.path.join(td, "ggml", "weights.gguf")
        cfg = B.make_config(mj["llm_config"])
        prompt = np.random.default_rng(46).integers(0, cfg.vocab_size, 21).astype(np.int32)
        out = {}
        # sfx "": the -ffp-contract=off build ("bit-exact" here); "_fast": the reference as its own CMake builds it (lib/libps_hip_contract.so)
        for sfx, ref in (("", r), ("_fast", rf)):
            m = ref.model(path, mj["model_arch"], cfg, 2)
            ids, logits, *_ = m.generate(prompt, 8, 24, want_logits=True)
            m.reset()
            out["ids" + sfx], out["logits" + sfx], out["batch_logits" + sfx] = ids, logits, m.forward(prompt[:9], np.arange(9), True)
            m.close()
        return dict(gguf_sha256=sha(path), preset=preset, wt=wt, embd_type=et, prompt=prompt, seed=1616, n_ctx=128, **out)


def tree(r):
    from oracle.ref_ops_forward import RefOpsModel
    TREE, TREE_DEPTH = tree_mask()
    preset, wt, et, n_ctx, P = TREE_CASE
    hidden, accept = (5, 33), (0, 1, 4)
    with tempfile.TemporaryDirectory() as d:
        seed = 1617
        mj = synth.write_model_dir(d, preset, wt, n_ctx=n_ctx, seed=seed, embd_type=et)
        cfg = B.make_config(mj["llm_config"])
        path = os.path.join(d, "ggml", "weights.gguf")
        rd = gguf.GGUFReader(path)
        tensors = {n: (ti.type, np.array(rd.data(n)), ti.ne[0], (list(ti.ne) + [1])[1]) for n, ti in rd.tensors.items()}
        m = RefOpsModel(r, cfg, mj["model_arch"], tensors)
        rng = np.random.default_rng(seed)
        prefix = rng.integers(0, cfg.vocab_size, P).astype(np.int32)
        for lo in range(0, P, 32):
            hi = min(lo + 32, P)
            m.forward_causal(prefix[lo:hi], np.arange(lo, hi), False)
        kv_vis = np.ones(n_ctx, dtype=np.uint8)
        kv_vis[list(hidden)] = 0
        toks = rng.integers(0, cfg.vocab_size, 12).astype(np.int32)
        rope = (P + TREE_DEPTH).astype(np.int32)
        logits = m.forward_tree(toks, rope, TREE, kv_vis, True, advance=False)
        for L in range(cfg.n_layers):  # accept 0 -> 1 -> 4
            m.k_cache[L][P + 2] = m.k_cache[L][P + 4]
            m.v_cache[L][:, P + 2] = m.v_cache[L][:, P + 4]
        m.position = P + 3
        nxt = np.array([int(np.argmax(logits[4]))], dtype=np.int32)
        step = m.forward_tree(nxt, np.array([P + 3], dtype=np.int32), None, kv_vis, True, advance=False)
        return dict(preset=preset, wt=wt, embd_type=et, n_ctx=n_ctx, seed=seed, gguf_sha256=sha(path), prefix=prefix, hidden=np.array(hidden),
                    tokens=toks, rope=rope, tree=TREE, logits=logits, accept=np.array(accept), next=nxt, step_logits=step)


def main(out_dir):
    if not B.have_ref():
        raise SystemExit("oracle/_ref/libps_ref.so is missing: python -c 'from oracle import binding; binding.build(ref=True)'")
    os.makedirs(out_dir, exist_ok=True)
    if not B.have_ref_fast():
        raise SystemExit("oracle/_ref/libps_ref_fast.so is missing: python -c 'from oracle import binding; binding.build(ref=True)'")
    r, rf = B.Ref(2), B.Ref(2, so=B.REF_FAST_SO)
    save(os.path.join(out_dir, "f16_mul_mat.npz"), **mul_mat(r))
    for name, preset, wt, et in E2E:
        save(os.path.join(out_dir, f"e2e_f16_{name}.npz"), **e2e(r, rf, preset, wt, et))
    save(os.path.join(out_dir, "tree_forward_f16.npz"), **tree(r))
    print("wrote", out_dir)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden"))
