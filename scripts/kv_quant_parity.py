"""End-to-end deviation of a quantised KV cache (writes profiles/kv_quant_parity.json; recorded,
not gated).

A config-5-width DecoderLM (V = 10000, E = 256, 8 heads, 4 layers, d = 32; random weights, one
fixed seed) prefills a batch of random prompts into an fp32, a bf16 and an fp8 KVCache and then
takes 32 decode steps on each. Every cache is fed the same tokens (the fp32 cache's greedy ids),
so a step's logits differ through the cached K / V values alone. Recorded per format: the max and
mean |logit - fp32 logit| over all steps, rows and vocabulary entries, the largest |fp32 logit|
for scale, and the share of (step, row) greedy ids that agree with the fp32 cache's.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "llmsys-project-flashattn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

STEPS = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_quant_parity.json"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prompt-len", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("kv_quant_parity.py needs an MI355X")
    import minitorch
    np.random.seed(args.seed)
    backend = minitorch.TensorBackend(minitorch.HipKernelOps)
    kw = dict(n_vocab=10000, n_embd=256, n_head=8, n_positions=args.prompt_len + STEPS, p_dropout=0.0)
    lm = minitorch.DecoderLM(backend=backend, use_fused_kernel=True, use_flash_attention=True, n_layer=4, **kw)
    lm.eval()
    rng = np.random.default_rng(args.seed)
    B, T = args.batch, args.prompt_len
    prompts = rng.integers(0, kw["n_vocab"], (B, T)).astype(np.float32)
    lens = np.full(B, T, np.float32)

    def run(kv_dtype, feed):
        """Logits [STEPS, B, V] of the decode steps; feed: the ids to feed ([STEPS, B]) or None (greedy)."""
        cache = lm.new_cache(B, kv_dtype)
        logits = lm(minitorch.tensor_from_numpy(prompts, backend), kv_len=lens, cache=cache).to_numpy()[:, -1]
        nxt = np.argmax(logits, -1)
        out, ids = [], []
        for t in range(STEPS):
            tok = nxt if feed is None else feed[t]
            ids.append(tok)
            step = minitorch.tensor_from_numpy(tok.astype(np.float32).reshape(B, 1), backend)
            logits = lm(step, cache=cache).to_numpy()[:, 0]
            out.append(logits)
            nxt = np.argmax(logits, -1)
        return np.stack(out), np.stack(ids), cache.nbytes
    ref, fed, ref_bytes = run(None, None)
    res = {"device": torch.cuda.get_device_name(0), "model": dict(kw, n_layer=lm.n_layer, head_dim=32),
           "seed": args.seed, "batch": B, "prompt_len": T, "decode_steps": STEPS,
           "max_abs_fp32_logit": float(np.abs(ref).max()), "fp32_cache_bytes": ref_bytes, "formats": {}}
    top2 = np.sort(ref, -1)[..., -2:]
    res["fp32_smallest_top2_gap"] = float((top2[..., 1] - top2[..., 0]).min())
    res["fp32_median_top2_gap"] = float(np.median(top2[..., 1] - top2[..., 0]))
    for kv_dtype in ("bf16", "fp8"):
        got, _, nbytes = run(kv_dtype, fed)
        err = np.abs(got.astype(np.float64) - ref)
        res["formats"][kv_dtype] = {
            "cache_bytes": nbytes, "cache_bytes_over_fp32": nbytes / ref_bytes,
            "max_abs_dlogit": float(err.max()), "mean_abs_dlogit": float(err.mean()),
            "greedy_ids_agreeing": float((np.argmax(got, -1) == np.argmax(ref, -1)).mean()),
        }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
