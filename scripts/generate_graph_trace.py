"""The target of a kernel trace of the graph-replayed decode step:

  rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- \\
      python scripts/generate_graph_trace.py

One sequence through DecoderLM.generate(graph=True) at config-5 width (V = 10000, E = 256,
8 heads, 4 layers): a short call that captures the graph, then the traced call. The stats give
the kernels of a replayed step and their durations (profiles/generate_graph_kernel_stats.csv);
the script prints the untraced-comparable wall time of the second call as one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "llmsys-project-flashattn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-positions", type=int, default=1024)
    ap.add_argument("--prompt-len", type=int, default=768)
    ap.add_argument("--new-tokens", type=int, default=200)
    ap.add_argument("--batch", type=int, default=1)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("generate_graph_trace.py needs an MI355X")
    import minitorch
    np.random.seed(0)
    backend = minitorch.TensorBackend(minitorch.HipKernelOps)
    lm = minitorch.DecoderLM(n_vocab=10000, n_embd=256, n_head=8, n_positions=args.n_positions, p_dropout=0.0,
                             backend=backend, use_fused_kernel=True, use_flash_attention=True)
    rng = np.random.default_rng(0)
    prompts = [[int(t) for t in rng.integers(0, 10000, args.prompt_len)] for _ in range(args.batch)]
    lm.generate(prompts, 8, graph=True)  # captures
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = lm.generate(prompts, args.new_tokens, graph=True)  # ends in a device-to-host copy
    dt = time.perf_counter() - t0
    print(json.dumps({"n_positions": args.n_positions, "prompt_len": args.prompt_len, "batch": args.batch,
                      "tokens": sum(len(t) for t in out), "seconds": dt, "graph_captures": lm.graph_captures}))


if __name__ == "__main__":
    main()
