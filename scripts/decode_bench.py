"""Decode-attention and generation timings (writes profiles/decode_bench.json).

Per shape (B, H, L, d) and dtype, alternated in one process and timed with device events:

  decode   one mt_flash_attn_decode step at Nq = 1 against a full cache of L rows
           ([B, L, H, d] storage, the KVCache layout), caller-provided workspace
  copy     a device-to-device copy of the same K and V bytes: the bandwidth this box reaches
           on those bytes, the yardstick for the decode step's bytes/s
  full     flash_fwd(causal=True) at N = L: what one generation step's attention costs
           without a cache (a full causal forward over the prefix)

The decode and copy legs rotate over enough cache copies to exceed the 256 MiB Infinity Cache,
so that both read HBM (a single 134 MB cache would be served from that cache on every call
after the first). Algorithmic bytes of the decode step: 2 B H L d esize for K and V, plus Q, O
and the split workspace written once and read once.

End to end: DecoderLM.generate tokens/s at config-5 width (V = 10000, E = 256, 8 heads,
4 layers), cached against uncached (the reference's loop), at n_positions 40 and 1024.

--graph-legs instead writes profiles/generate_graph_bench.json (decode_bench.json is left alone):

  generate      the same two rows with generate(graph=True) (the captured decode step, tokens
                chosen on the device) beside the cached-eager and uncached legs, batch 1 and 8,
                greedy, and one sampled graph leg (T = 0.8, top_k = 50); host clock around calls
                that end in a device-to-host copy; the legs alternate inside every round
  select_token  mt_select_token alone at (B, V) = (8, 10000) and (64, 10000): greedy, top_k = 50
                and the whole vocabulary at T = 1, and the nucleus legs top_p = 0.9 over the whole
                vocabulary, top_k = 50 with top_p = 0.9, and min_p = 0.05 (mt_select_token_p; left
                out with a --lib build that predates it); device events around 64 launches,
                alternated

--gqa-legs instead writes profiles/decode_gqa_bench.json: per large shape and Hkv in {H, H/4, H/8},
alternated in one process like the legs above:

  gqa       one mt_flash_attn_decode_gqa step at Nq = 1: H query heads, caches of Hkv heads
            ([B, L, Hkv, d] storage)
  repeated  mt_flash_attn_decode on K / V of H heads (what the same model costs with its K / V
            repeated per group: H / Hkv times the bytes, the same arithmetic)
  copy      a device-to-device copy of the gqa leg's own K and V bytes

Each leg rotates over enough cache copies of its own to exceed twice the Infinity Cache.

--extend-legs instead writes profiles/extend_bench.json: per row of EXTEND_ROWS (B, H, Hkv, n, d,
dtype), 512 new tokens on a cached prefix of n - 512, alternated in one process like the legs above:

  extend    one mt_flash_attn_extend step: the last 512 rows of every sequence against its cache
  full      mt_flash_attn_fwd_varlen, causal, at N = n with a kv_len vector, K / V repeated to H
            heads for the grouped-query row: what gives the same rows without the extend step
  chunked   the whole n tokens as n / 512 extend steps (a chunked prefill; its first step stands in
            for the prefill of an empty cache, the same arithmetic), against that one-shot forward

The script exits non-zero unless the extend step is faster than the full forward at every row.

--extend-legs then (--extend-src-legs: only) writes profiles/extend_src_bench.json: per row of
EXTEND_ROWS the same 512-token causal step on the caches a serving loop holds, fp32 queries and O in the
paged and quantised legs, alternated in one process and swapping places each round:

  extend         the plain leg above, unchanged (the row's own dtype)
  paged_direct   one mt_flash_attn_extend_paged step on fp32 pools, P = 16, pages shuffled by one randperm
  paged_gather   its yardstick, the two launches it replaces: mt_kv_cache_gather_paged into a contiguous
                 fp32 pair, then mt_flash_attn_extend on it
  kvq_direct_*   one mt_flash_attn_extend_kvq step on bf16 / e4m3 caches
  kvq_dequant_*  its yardstick: mt_kv_cache_dequant into an fp32 pair, then mt_flash_attn_extend(MT_F32)

Each leg rotates over enough caches (pools) to exceed twice the Infinity Cache; a direct leg and its
yardstick read the same sets. The script exits non-zero if a direct leg's median exceeds its two-launch
yardstick of the same run. --lib PATH loads another build of the library (an A/B against an older one:
the legs whose entry points it lacks are left out).

--kvq-legs instead writes profiles/decode_kvq_bench.json: per shape of KVQ_SHAPES and Hkv in {H, H/4},
Nq = 1, fp32 queries and O in every leg, alternated in one process and swapping places each round:

  fp32      one mt_flash_attn_decode_gqa step (MT_F32) on fp32 caches: what DecoderLM pays without kv_dtype
  bf16      one mt_flash_attn_decode_kvq step on bf16 caches
  fp8       one mt_flash_attn_decode_kvq step on e4m3 caches with their row scales
  copy_*    a device-to-device copy of each leg's own K / V (and scale) bytes

and the append kernels alone for a 1-token step (mt_kv_cache_append fp32, mt_kv_cache_append_quant).
Each leg rotates over enough cache copies of its own to exceed twice the Infinity Cache. The script
exits non-zero unless, with Hkv = H, each quantised step is faster than the fp32 step of the same
run by more than the 4 % box-to-box variation (t_quant * 1.04 < t_fp32).

--paged-legs instead writes profiles/decode_paged_bench.json: per shape of KVQ_SHAPES, Hkv in {H, H/4}
and dtype in {fp32, bf16}, Nq = 1, alternated in one process and swapping places each round:

  contig    one mt_flash_attn_decode_gqa step on a contiguous cache: the yardstick of the same run
  paged16   one mt_flash_attn_decode_paged step, P = 16, the pages of every row shuffled over the pool
  paged128  the same with P = 128

Each leg rotates over enough caches (pools) of its own to exceed twice the Infinity Cache. No gate: the
ratios paged / contig are recorded. The memory side is recorded too: nbytes of a one-layer KVCache and of
PagedKVCaches holding a ragged batch of one row of 4096 tokens and seven of 64.

--rope-legs instead writes profiles/rope_bench.json:

  rope / copy   mt_rope on Q and K (one two-tensor launch, [B,T,H,d] storage, positions from a device
                vector) of an (8,16,1,64) decode step and an (8,16,512,64) extend step, against a
                device-to-device copy of the same bytes (the floor of a read-once, write-once kernel);
                alternated, swapping places each round, over sets that exceed twice the Infinity Cache;
                each leg eagerly (device events around the launches: at these sizes the host's time to
                issue a launch) and as one captured graph of the same launches (*_graph: the kernels)
  generate     generate(graph=True) tokens/s with pos_encoding="rope" against "learned", batch 1 and 8,
                at the sizes of the graph legs, alternated inside every round

--spec-legs instead writes profiles/spec_bench.json (speculative decoding):

  verify       mt_flash_attn_decode on k + 1 = 2, 4, 8 query rows against the one-row step at (8,16,4096,64),
                fp32 cache, every leg a captured graph over rotated cache sets
  draft_accept mt_spec_draft + mt_spec_accept alone (B = 8, V = 10000, rows of 1025 tokens, k = 1, 3, 7), as a
                captured graph, beside mt_select_token on [B, V]
  generate     generate(graph=True) tokens/s with speculate in {2, 4, 7} against speculate=None on the same
                model, batch 1 and 8, with the acceptance rate and the tokens per row and step of each leg: a
                rotary model over a 97-token vocabulary, whose greedy continuation falls into cycles, and
                random prompts over 10000 tokens (next to nothing is accepted: the overhead)

No gate: what is measured is recorded.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "llmsys-project-flashattn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [(8, 16, 4096, 64, "bf16"), (8, 16, 4096, 64, "f32"), (1, 16, 16384, 128, "bf16"),
          (64, 8, 40, 32, "f32")]
ICACHE = 256 << 20


def _timed(torch, fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(inner):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def bench_shape(torch, _hip, B, H, L, d, name, rounds, warmup):
    dt = torch.bfloat16 if name == "bf16" else torch.float32
    es = 2 if name == "bf16" else 4
    code = 1 if name == "bf16" else 0
    kv_bytes = 2 * B * H * L * d * es
    nset = min(8, max(2, -(-2 * ICACHE // kv_bytes) + 1))  # small caches: launch-bound, a few sets do
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32).to(dt)  # noqa: E731
    caches = [(rnd(B, L, H, d).permute(0, 2, 1, 3), rnd(B, L, H, d).permute(0, 2, 1, 3)) for _ in range(nset)]
    dst = (torch.empty_like(caches[0][0]), torch.empty_like(caches[0][1]))
    q = rnd(B, 1, H, d).permute(0, 2, 1, 3)
    kvl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    o = torch.empty((B, 1, H, d), dtype=dt, device="cuda").permute(0, 2, 1, 3)
    m, l = (torch.empty((B, H, 1), dtype=torch.float32, device="cuda") for _ in range(2))
    nsplit, span, tile = _hip.decode_splits(code, B, H, 1, L, d)
    ws_bytes = _hip.decode_workspace_bytes(code, B, H, 1, L, d)
    ws = torch.empty(max(1, ws_bytes // 4), dtype=torch.float32, device="cuda") if ws_bytes else None
    Q, K, V = (rnd(B, H, L, d) for _ in range(3))
    O = torch.empty_like(Q)
    M, Lw = (torch.empty((B, H, L), dtype=torch.float32, device="cuda") for _ in range(2))

    def decode(i):
        kc, vc = caches[i % nset]
        _hip.flash_decode(q, kc, vc, kv_len=kvl, causal=True, out=o, m=m, l=l, workspace=ws)

    def copy(i):
        kc, vc = caches[i % nset]
        dst[0].copy_(kc)
        dst[1].copy_(vc)

    def full(i):
        _hip.flash_fwd(Q, K, V, True, out=O, m=M, l=Lw)
    legs = {"decode": (decode, 4 * nset), "copy": (copy, 2 * nset), "full": (full, 2)}
    for fn, inner in legs.values():
        for _ in range(warmup):
            _timed(torch, fn, inner)
    times = {k: [] for k in legs}
    for _ in range(rounds):  # the legs alternate inside every round
        for k, (fn, inner) in legs.items():
            times[k].append(_timed(torch, fn, inner))
    alg_bytes = kv_bytes + 2 * B * H * d * es + 2 * ws_bytes
    med = {k: statistics.median(v) for k, v in times.items()}
    return {
        "shape": [B, H, L, d], "dtype": name, "nq": 1, "splits": nsplit, "span_keys": span, "tile_keys": tile,
        "workspace_bytes": ws_bytes, "kv_bytes": kv_bytes, "decode_algorithmic_bytes": alg_bytes,
        "cache_sets_rotated": nset, "rounds": rounds,
        "decode_s_median": med["decode"], "decode_s_min": min(times["decode"]),
        "copy_s_median": med["copy"], "copy_s_min": min(times["copy"]),
        "full_causal_fwd_s_median": med["full"], "full_causal_fwd_s_min": min(times["full"]),
        "decode_bytes_per_s": alg_bytes / med["decode"],
        "copy_read_bytes_per_s": kv_bytes / med["copy"],      # bytes read (as many are written)
        "copy_moved_bytes_per_s": 2 * kv_bytes / med["copy"],  # read + written
        "decode_vs_copy_read_rate": (alg_bytes / med["decode"]) / (kv_bytes / med["copy"]),
        "full_over_decode": med["full"] / med["decode"],
    }


def bench_gqa(torch, _hip, B, H, L, d, name, rounds, warmup):
    dt = torch.bfloat16 if name == "bf16" else torch.float32
    es = 2 if name == "bf16" else 4
    code = 1 if name == "bf16" else 0
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32).to(dt)  # noqa: E731

    def make_caches(heads):
        kv_bytes = 2 * B * heads * L * d * es
        nset = min(72, max(2, -(-2 * ICACHE // kv_bytes) + 1))
        return kv_bytes, nset, [(rnd(B, L, heads, d).permute(0, 2, 1, 3), rnd(B, L, heads, d).permute(0, 2, 1, 3))
                                for _ in range(nset)]
    q = rnd(B, 1, H, d).permute(0, 2, 1, 3)
    kvl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    o = torch.empty((B, 1, H, d), dtype=dt, device="cuda").permute(0, 2, 1, 3)
    m, l = (torch.empty((B, H, 1), dtype=torch.float32, device="cuda") for _ in range(2))
    rep_bytes, rep_nset, rep_caches = make_caches(H)
    rep_ws_bytes = _hip.decode_workspace_bytes(code, B, H, 1, L, d)
    rep_ws = torch.empty(max(1, rep_ws_bytes // 4), dtype=torch.float32, device="cuda")
    rows = []
    for Hkv in (H, H // 4, H // 8):
        kv_bytes, nset, caches = (rep_bytes, rep_nset, rep_caches) if Hkv == H else make_caches(Hkv)
        dst = (torch.empty_like(caches[0][0]), torch.empty_like(caches[0][1]))
        nsplit, span, tile = _hip.decode_splits(code, B, H, 1, L, d, Hkv=Hkv)
        ws_bytes = _hip.decode_workspace_bytes(code, B, H, 1, L, d, Hkv=Hkv)
        ws = torch.empty(max(1, ws_bytes // 4), dtype=torch.float32, device="cuda")

        def gqa(i):
            kc, vc = caches[i % nset]
            _hip.flash_decode(q, kc, vc, kv_len=kvl, causal=True, out=o, m=m, l=l, workspace=ws)

        def repeated(i):
            kc, vc = rep_caches[i % rep_nset]
            _hip.flash_decode(q, kc, vc, kv_len=kvl, causal=True, out=o, m=m, l=l, workspace=rep_ws)

        def copy(i):
            kc, vc = caches[i % nset]
            dst[0].copy_(kc)
            dst[1].copy_(vc)
        # the two decode legs take as many launches per timing, whole turns over their cache sets
        calls = 2 * nset * rep_nset
        legs = {"gqa": (gqa, calls), "repeated": (repeated, calls), "copy": (copy, nset)}
        for fn, inner in legs.values():
            for _ in range(warmup):
                _timed(torch, fn, inner)
        times = {k: [] for k in legs}
        for r in range(rounds):  # the legs alternate inside every round, the decode legs swapping places
            order = ("gqa", "repeated", "copy") if r % 2 == 0 else ("repeated", "gqa", "copy")
            for k in order:
                fn, inner = legs[k]
                times[k].append(_timed(torch, fn, inner))
        med = {k: statistics.median(v) for k, v in times.items()}
        alg_bytes = kv_bytes + 2 * B * H * d * es + 2 * ws_bytes
        rep_alg_bytes = rep_bytes + 2 * B * H * d * es + 2 * rep_ws_bytes
        G = H // Hkv
        gs = min(G, 8)
        rows.append({
            "shape": [B, H, L, d], "dtype": name, "nq": 1, "kv_heads": Hkv, "group": G, "heads_per_workgroup": gs,
            "workgroups_per_split": B * Hkv * -(-G // gs), "splits": nsplit, "span_keys": span, "tile_keys": tile,
            "workspace_bytes": ws_bytes, "kv_bytes": kv_bytes, "gqa_algorithmic_bytes": alg_bytes,
            "repeated_kv_bytes": rep_bytes, "repeated_algorithmic_bytes": rep_alg_bytes,
            "cache_sets_rotated": nset, "repeated_cache_sets_rotated": rep_nset, "rounds": rounds,
            "decode_launches_per_timing": calls,
            "gqa_s_median": med["gqa"], "gqa_s_min": min(times["gqa"]),
            "repeated_s_median": med["repeated"], "repeated_s_min": min(times["repeated"]),
            "copy_s_median": med["copy"], "copy_s_min": min(times["copy"]),
            "gqa_bytes_per_s": alg_bytes / med["gqa"],
            "repeated_bytes_per_s": rep_alg_bytes / med["repeated"],
            "copy_read_bytes_per_s": kv_bytes / med["copy"],
            "gqa_over_repeated_time": med["gqa"] / med["repeated"],
            # the one condition: fewer bytes, the same arithmetic -> not slower beyond the 4 % box-to-box variation
            "gqa_not_slower_than_repeated": bool(med["gqa"] <= 1.04 * med["repeated"]),
        })
        print(json.dumps(rows[-1]), flush=True)
        if Hkv != H:
            del caches, dst
            torch.cuda.empty_cache()
    return rows


def gqa_legs(args, torch, _hip):
    res = {"device": torch.cuda.get_device_name(0), "kernels": []}
    for B, H, L, d, name in SHAPES[:3]:
        res["kernels"] += bench_gqa(torch, _hip, B, H, L, d, name, args.rounds, args.warmup)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.gqa_out), exist_ok=True)
    with open(args.gqa_out, "w") as f:
        json.dump(res, f, indent=1)
    slower = [(r["shape"], r["dtype"], r["kv_heads"]) for r in res["kernels"]
              if r["group"] > 1 and not r["gqa_not_slower_than_repeated"]]
    if slower:
        raise SystemExit(f"the GQA step is slower than the repeated-K/V step at {slower}")


EXTEND_ROWS = [(8, 16, 16, 4096, 64, "f32"), (8, 16, 16, 4096, 64, "bf16"), (8, 16, 4, 4096, 64, "bf16"),
               (1, 16, 16, 16384, 128, "bf16")]
EXTEND_NEW = 512


def bench_extend(torch, _hip, B, H, Hkv, n, d, name, rounds, warmup, new=EXTEND_NEW):
    dt = torch.bfloat16 if name == "bf16" else torch.float32
    es = 2 if name == "bf16" else 4
    code = 1 if name == "bf16" else 0
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32).to(dt)  # noqa: E731

    def make_caches(heads):
        kv_bytes = 2 * B * heads * n * d * es
        nset = min(24, max(2, -(-2 * ICACHE // kv_bytes) + 1))
        return kv_bytes, nset, [(rnd(B, n, heads, d).permute(0, 2, 1, 3), rnd(B, n, heads, d).permute(0, 2, 1, 3))
                                for _ in range(nset)]
    kv_bytes, nset, caches = make_caches(Hkv)
    # the full forward reads K / V of H heads: the caches themselves, or (GQA) K / V repeated to H heads
    full_bytes, full_nset, full_caches = (kv_bytes, nset, caches) if Hkv == H else make_caches(H)
    kid, bq, bk = _hip.extend_plan(code, B, H, new, n, d, Hkv=Hkv)
    q = rnd(B, new, H, d).permute(0, 2, 1, 3)
    o = torch.empty((B, new, H, d), dtype=dt, device="cuda").permute(0, 2, 1, 3)
    m, l = (torch.empty((B, H, new), dtype=torch.float32, device="cuda") for _ in range(2))
    qln = torch.full((B,), new, dtype=torch.int32, device="cuda")
    kvl = torch.full((B,), n, dtype=torch.int32, device="cuda")
    chunk_kvl = [torch.full((B,), s + new, dtype=torch.int32, device="cuda") for s in range(0, n, new)]
    Q = rnd(B, n, H, d).permute(0, 2, 1, 3)
    O = torch.empty((B, n, H, d), dtype=dt, device="cuda").permute(0, 2, 1, 3)
    M, Lw = (torch.empty((B, H, n), dtype=torch.float32, device="cuda") for _ in range(2))

    def extend(i):  # the last `new` tokens of every row on the n - new cached ones
        kc, vc = caches[i % nset]
        _hip.flash_extend(q, kc, vc, kv_len=kvl, q_len=qln, causal=True, out=o, m=m, l=l)

    def full(i):  # what gives the same rows without the extend step: the whole causal prefill
        kc, vc = full_caches[i % full_nset]
        _hip.flash_fwd(Q, kc, vc, True, out=O, m=M, l=Lw, kv_len=kvl)

    def chunked(i):  # the whole row in n / new extend steps (the first on an empty prefix)
        kc, vc = caches[i % nset]
        for kv in chunk_kvl:
            _hip.flash_extend(q, kc, vc, kv_len=kv, q_len=qln, causal=True, out=o, m=m, l=l)
    legs = {"extend": (extend, 2 * nset), "full": (full, full_nset), "chunked": (chunked, nset)}
    for fn, inner in legs.values():
        for _ in range(warmup):
            _timed(torch, fn, inner)
    times = {k: [] for k in legs}
    orders = (("extend", "full", "chunked"), ("full", "chunked", "extend"), ("chunked", "extend", "full"))
    for r in range(rounds):  # the legs alternate inside every round and swap places between rounds
        for k in orders[r % 3]:
            fn, inner = legs[k]
            times[k].append(_timed(torch, fn, inner))
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    # multiply-adds of both products, two flops each, over the (query, visible key) pairs
    pairs_extend = new * (n - new) + new * (new + 1) // 2
    pairs_full = n * (n + 1) // 2
    return {
        "shape": [B, H, n, d], "dtype": name, "kv_heads": Hkv, "new_tokens": new, "cached_prefix": n - new,
        "kernel": kid, "block_queries": bq, "tile_keys": bk, "workgroups": B * H * -(-new // bq),
        "kv_bytes": kv_bytes, "cache_sets_rotated": nset, "full_cache_sets_rotated": full_nset, "rounds": rounds,
        "extend_steps_in_chunked_prefill": len(chunk_kvl),
        **{f"{k}_s_median": med[k] for k in legs}, **{f"{k}_s_min": min(times[k]) for k in legs},
        **{f"{k}_s_max": max(times[k]) for k in legs}, **{f"{k}_round_spread": spread[k] for k in legs},
        "extend_flops": 4 * B * H * d * pairs_extend, "full_flops": 4 * B * H * d * pairs_full,
        "extend_flops_per_s": 4 * B * H * d * pairs_extend / med["extend"],
        "full_flops_per_s": 4 * B * H * d * pairs_full / med["full"],
        "extend_share_of_full_flops": pairs_extend / pairs_full,
        "extend_over_full_time": med["extend"] / med["full"],
        "chunked_over_full_time": med["chunked"] / med["full"],
        # the one condition: the step beats re-prefilling everything, in the same run
        "extend_faster_than_full": bool(med["extend"] < med["full"]),
    }


def extend_legs(args, torch, _hip):
    res = {"device": torch.cuda.get_device_name(0), "kernels": []}
    for B, H, Hkv, n, d, name in EXTEND_ROWS:
        r = bench_extend(torch, _hip, B, H, Hkv, n, d, name, args.rounds, args.warmup)
        print(json.dumps(r), flush=True)
        res["kernels"].append(r)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.extend_out), exist_ok=True)
    with open(args.extend_out, "w") as f:
        json.dump(res, f, indent=1)
    slower = [(r["shape"], r["dtype"], r["kv_heads"], round(r["extend_over_full_time"], 3)) for r in res["kernels"]
              if not r["extend_faster_than_full"]]
    if slower:
        raise SystemExit(f"the extend step is not faster than the full causal forward at {slower}")


def bench_extend_src(torch, _hip, B, H, Hkv, n, d, name, rounds, warmup, new=EXTEND_NEW, P=16):
    """The plain extend leg of bench_extend, and the step on paged and quantised caches against the two
    launches each direct kernel replaces."""
    dt = torch.bfloat16 if name == "bf16" else torch.float32
    es = 2 if name == "bf16" else 4
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd32 = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32)  # noqa: E731
    have = lambda sym: hasattr(_hip.lib(), sym)  # noqa: E731

    def nsets(kv_bytes):  # more than twice the Infinity Cache for every leg (the smallest set here is 17.8 MB)
        return max(2, -(-2 * ICACHE // kv_bytes) + 1)
    # the plain leg: bench_extend's, in the row's dtype
    kv_bytes = 2 * B * Hkv * n * d * es
    nset = nsets(kv_bytes)
    caches = [(rnd32(B, n, Hkv, d).to(dt).permute(0, 2, 1, 3), rnd32(B, n, Hkv, d).to(dt).permute(0, 2, 1, 3))
              for _ in range(nset)]
    q = rnd32(B, new, H, d).to(dt).permute(0, 2, 1, 3)
    o = torch.empty((B, new, H, d), dtype=dt, device="cuda").permute(0, 2, 1, 3)
    # the paged and quantised legs: fp32 queries and O, as DecoderLM runs them
    q32 = rnd32(B, new, H, d).permute(0, 2, 1, 3)
    o32 = torch.empty((B, new, H, d), dtype=torch.float32, device="cuda").permute(0, 2, 1, 3)
    m, l = (torch.empty((B, H, new), dtype=torch.float32, device="cuda") for _ in range(2))
    qln = torch.full((B,), new, dtype=torch.int32, device="cuda")
    kvl = torch.full((B,), n, dtype=torch.int32, device="cuda")
    # one contiguous fp32 pair, KVCache's layout: what the gather and the dequantising copy fill
    sk, sv = (torch.empty((B, n, Hkv, d), dtype=torch.float32, device="cuda").permute(0, 2, 1, 3) for _ in range(2))
    scratch_bytes = 2 * B * Hkv * n * d * 4

    W = n // P
    assert W * P == n
    pool_bytes = 2 * B * W * P * Hkv * d * 4
    pset = nsets(pool_bytes)
    pools = [(rnd32(B * W, P, Hkv, d).permute(0, 2, 1, 3), rnd32(B * W, P, Hkv, d).permute(0, 2, 1, 3))
             for _ in range(pset)]
    table = torch.randperm(B * W, generator=g, device="cuda").to(torch.int32).view(B, W)

    def quantised(kv):
        dq = torch.bfloat16 if kv == "bf16" else torch.uint8
        nb = 2 * B * Hkv * n * d * (2 if kv == "bf16" else 1) + (2 * B * Hkv * n * 4 if kv == "fp8" else 0)
        sets = []
        for _ in range(nsets(nb)):
            kc, vc = (torch.empty((B, n, Hkv, d), dtype=dq, device="cuda").permute(0, 2, 1, 3) for _ in range(2))
            ks = vs = None
            if kv == "fp8":
                ks, vs = (torch.empty((B, Hkv, n), dtype=torch.float32, device="cuda") for _ in range(2))
            for lo in range(0, n, 1024):  # the fp32 rows to quantise, a slice at a time
                kn, vn = (rnd32(B, 1024, Hkv, d).permute(0, 2, 1, 3) for _ in range(2))
                _hip.kv_cache_append_quant(kn, vn, kc, vc, torch.full((B,), lo, dtype=torch.int32, device="cuda"), ks, vs)
            sets.append((kc, vc, ks, vs))
        return nb, sets
    qsets = {kv: quantised(kv) for kv in ("bf16", "fp8")}

    def extend(i):
        kc, vc = caches[i % nset]
        _hip.flash_extend(q, kc, vc, kv_len=kvl, q_len=qln, causal=True, out=o, m=m, l=l)

    def paged_direct(i):
        kp, vp = pools[i % pset]
        _hip.flash_extend_paged(q32, kp, vp, table, kv_len=kvl, q_len=qln, causal=True, out=o32, m=m, l=l)

    def paged_gather(i):
        kp, vp = pools[i % pset]
        _hip.kv_cache_gather_paged(kp, vp, table, kv_len=kvl, k_out=sk, v_out=sv)
        _hip.flash_extend(q32, sk, sv, kv_len=kvl, q_len=qln, causal=True, out=o32, m=m, l=l)

    def kvq_direct(kv):
        sets = qsets[kv][1]

        def fn(i):
            kc, vc, ks, vs = sets[i % len(sets)]
            _hip.flash_extend_kvq(q32, kc, vc, ks, vs, kv_len=kvl, q_len=qln, causal=True, out=o32, m=m, l=l)
        return fn, 2 * len(sets)

    def kvq_dequant(kv):
        sets = qsets[kv][1]

        def fn(i):
            kc, vc, ks, vs = sets[i % len(sets)]
            _hip.kv_cache_dequant(kc, vc, ks, vs, kv_len=kvl, k_out=sk, v_out=sv)
            _hip.flash_extend(q32, sk, sv, kv_len=kvl, q_len=qln, causal=True, out=o32, m=m, l=l)
        return fn, 2 * len(sets)
    legs = {"extend": (extend, 2 * nset), "paged_gather": (paged_gather, 2 * pset)}
    pairs = {}  # direct leg -> its yardstick
    if have("mt_flash_attn_extend_paged"):
        legs["paged_direct"] = (paged_direct, 2 * pset)
        pairs["paged_direct"] = "paged_gather"
    for kv in ("bf16", "fp8"):
        legs[f"kvq_dequant_{kv}"] = kvq_dequant(kv)
        if have("mt_flash_attn_extend_kvq"):
            legs[f"kvq_direct_{kv}"] = kvq_direct(kv)
            pairs[f"kvq_direct_{kv}"] = f"kvq_dequant_{kv}"
    for fn, inner in legs.values():
        for _ in range(warmup):
            _timed(torch, fn, inner)
    names = list(legs)
    times = {k: [] for k in legs}
    for r in range(rounds):  # the legs alternate inside every round and swap places between rounds
        for k in names[r % len(names):] + names[:r % len(names)]:
            fn, inner = legs[k]
            times[k].append(_timed(torch, fn, inner))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {
        "shape": [B, H, n, d], "dtype": name, "kv_heads": Hkv, "new_tokens": new, "cached_prefix": n - new,
        "page_size": P, "rounds": rounds, "kv_bytes": kv_bytes, "pool_bytes": pool_bytes,
        "kvq_bytes": {kv: qsets[kv][0] for kv in qsets},
        "cache_sets_rotated": {"extend": nset, "paged": pset, **{f"kvq_{kv}": len(qsets[kv][1]) for kv in qsets}},
        # what each yardstick's copy moves beyond its reads of the cache: one fp32 write and one read of all rows
        "copy_bytes_written_and_read": 2 * scratch_bytes,
        **{f"{k}_s_median": med[k] for k in legs}, **{f"{k}_s_min": min(times[k]) for k in legs},
        **{f"{k}_s_max": max(times[k]) for k in legs},
        **{f"{k}_round_spread": (max(times[k]) - min(times[k])) / med[k] for k in legs},
        **{f"{a}_over_{b}": med[a] / med[b] for a, b in pairs.items()},
        "direct_not_slower": {a: bool(med[a] <= med[b]) for a, b in pairs.items()},
    }


def extend_src_legs(args, torch, _hip):
    library = "this checkout's"
    if args.lib:
        library = os.path.join(os.path.basename(os.path.dirname(_hip.LIB_PATH)), os.path.basename(_hip.LIB_PATH))
    res = {"device": torch.cuda.get_device_name(0), "library": library, "kernels": []}
    for B, H, Hkv, n, d, name in EXTEND_ROWS:
        r = bench_extend_src(torch, _hip, B, H, Hkv, n, d, name, args.rounds, args.warmup)
        print(json.dumps(r), flush=True)
        res["kernels"].append(r)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.extend_src_out), exist_ok=True)
    with open(args.extend_src_out, "w") as f:
        json.dump(res, f, indent=1)
    slower = [(r["shape"], r["dtype"], r["kv_heads"], k) for r in res["kernels"]
              for k, ok in r["direct_not_slower"].items() if not ok]
    if slower:
        raise SystemExit(f"a direct extend leg is slower than the two launches it replaces at {slower}")


KVQ_SHAPES = [(8, 16, 4096, 64), (1, 16, 16384, 128)]


def bench_kvq(torch, _hip, B, H, L, d, rounds, warmup):
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32)  # noqa: E731
    q = rnd(B, 1, H, d).permute(0, 2, 1, 3)
    kvl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    zero = torch.zeros(B, dtype=torch.int32, device="cuda")
    o = torch.empty((B, 1, H, d), dtype=torch.float32, device="cuda").permute(0, 2, 1, 3)
    m, l = (torch.empty((B, H, 1), dtype=torch.float32, device="cuda") for _ in range(2))
    kinds = {"fp32": (torch.float32, 4, None), "bf16": (torch.bfloat16, 2, _hip.MT_KV_BF16),
             "fp8": (torch.uint8, 1, _hip.MT_KV_FP8)}
    rows = []
    for Hkv in (H, H // 4):
        src = (rnd(B, L, Hkv, d).permute(0, 2, 1, 3), rnd(B, L, Hkv, d).permute(0, 2, 1, 3))
        legs, info = {}, {}
        for name, (dt, es, code) in kinds.items():
            kv_bytes = 2 * B * Hkv * L * d * es + (2 * B * Hkv * L * 4 if name == "fp8" else 0)
            nset = min(72, max(2, -(-2 * ICACHE // kv_bytes) + 1))
            sets = []
            for _ in range(nset):  # every set holds the same values in buffers of its own
                kc, vc = (torch.empty((B, L, Hkv, d), dtype=dt, device="cuda").permute(0, 2, 1, 3) for _ in range(2))
                ks = vs = None
                if name == "fp8":
                    ks, vs = (torch.empty((B, Hkv, L), dtype=torch.float32, device="cuda") for _ in range(2))
                if code is None:
                    kc.copy_(src[0])
                    vc.copy_(src[1])
                else:
                    _hip.kv_cache_append_quant(src[0], src[1], kc, vc, zero, ks, vs)
                sets.append((kc, vc, ks, vs))
            if code is None:
                nsplit, span, tile = _hip.decode_splits(0, B, H, 1, L, d, Hkv=Hkv)
                ws_bytes = _hip.decode_workspace_bytes(0, B, H, 1, L, d, Hkv=Hkv)
            else:
                nsplit, span, tile = _hip.decode_kvq_splits(code, B, H, 1, L, d, Hkv=Hkv)
                ws_bytes = _hip.decode_kvq_workspace_bytes(code, B, H, 1, L, d, Hkv=Hkv)
            ws = torch.empty(max(1, ws_bytes // 4), dtype=torch.float32, device="cuda")
            dst = tuple(None if t is None else torch.empty_like(t) for t in sets[0])

            def step(i, sets=sets, nset=nset, ws=ws, quant=code is not None):
                kc, vc, ks, vs = sets[i % nset]
                if quant:
                    _hip.flash_decode_kvq(q, kc, vc, ks, vs, kv_len=kvl, causal=True, out=o, m=m, l=l, workspace=ws)
                else:
                    _hip.flash_decode(q, kc, vc, kv_len=kvl, causal=True, out=o, m=m, l=l, workspace=ws)

            def copy(i, sets=sets, nset=nset, dst=dst):
                for a, b in zip(dst, sets[i % nset]):
                    if a is not None:
                        a.copy_(b)
            legs[name] = (step, nset * -(-24 // nset))   # whole turns over the leg's cache sets
            legs["copy_" + name] = (copy, nset)
            info[name] = dict(kv_bytes=kv_bytes, nset=nset, splits=nsplit, span=span, tile=tile, ws_bytes=ws_bytes,
                              alg=kv_bytes + 2 * B * H * d * 4 + 2 * ws_bytes)
        for fn, inner in legs.values():
            for _ in range(warmup):
                _timed(torch, fn, inner)
        times = {k: [] for k in legs}
        steps = ["fp32", "bf16", "fp8"]
        for r in range(rounds):  # the legs alternate inside every round, the decode legs swapping places
            order = steps[r % 3:] + steps[:r % 3] + ["copy_" + k for k in steps]
            for k in order:
                fn, inner = legs[k]
                times[k].append(_timed(torch, fn, inner))
        med = {k: statistics.median(v) for k, v in times.items()}
        G = H // Hkv
        row = {"shape": [B, H, L, d], "nq": 1, "kv_heads": Hkv, "group": G, "rounds": rounds}
        for k in steps:
            i = info[k]
            row.update({
                f"{k}_s_median": med[k], f"{k}_s_min": min(times[k]), f"{k}_s_max": max(times[k]),
                f"{k}_copy_s_median": med["copy_" + k], f"{k}_kv_bytes": i["kv_bytes"],
                f"{k}_algorithmic_bytes": i["alg"], f"{k}_bytes_per_s": i["alg"] / med[k],
                f"{k}_copy_read_bytes_per_s": i["kv_bytes"] / med["copy_" + k],
                f"{k}_splits": i["splits"], f"{k}_span_keys": i["span"], f"{k}_tile_keys": i["tile"],
                f"{k}_workspace_bytes": i["ws_bytes"], f"{k}_cache_sets_rotated": i["nset"],
                f"{k}_launches_per_timing": legs[k][1]})
        for k in ("bf16", "fp8"):
            row[f"{k}_over_fp32_time"] = med[k] / med["fp32"]
            row[f"{k}_over_fp32_bytes"] = info[k]["kv_bytes"] / info["fp32"]["kv_bytes"]
            # the one condition (gated at Hkv = H): faster than the fp32-cache step by more than the 4 %
            # box-to-box variation
            row[f"{k}_faster_than_fp32"] = bool(med[k] * 1.04 < med["fp32"])
        rows.append(row)
        print(json.dumps(row), flush=True)
        del legs, src
        torch.cuda.empty_cache()
    return rows


def bench_kvq_append(torch, _hip, B, H, L, d, rounds, warmup, inner=64):
    """The append kernels alone for a 1-token step on caches of L rows."""
    g = torch.Generator(device="cuda").manual_seed(0)
    kn, vn = (torch.randn(B, 1, H, d, generator=g, device="cuda").permute(0, 2, 1, 3) for _ in range(2))
    pos = torch.full((B,), L - 1, dtype=torch.int32, device="cuda")
    legs = {}
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp8", torch.uint8)):
        kc, vc = (torch.zeros((B, L, H, d), dtype=dt, device="cuda").permute(0, 2, 1, 3) for _ in range(2))
        ks = vs = None
        if name == "fp8":
            ks, vs = (torch.zeros((B, H, L), dtype=torch.float32, device="cuda") for _ in range(2))
        if name == "fp32":
            legs[name] = lambda i, kc=kc, vc=vc: _hip.kv_cache_append(kn, vn, kc, vc, pos)
        else:
            legs[name] = lambda i, kc=kc, vc=vc, ks=ks, vs=vs: _hip.kv_cache_append_quant(kn, vn, kc, vc, pos, ks, vs)
    for fn in legs.values():
        for _ in range(warmup):
            _timed(torch, fn, inner)
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(_timed(torch, fn, inner))
    return {"shape": [B, H, L, d], "new_tokens": 1, "rounds": rounds, "launches_per_timing": inner,
            **{f"append_{k}_s_median": statistics.median(v) for k, v in times.items()},
            **{f"append_{k}_s_min": min(v) for k, v in times.items()}}


def kvq_legs(args, torch, _hip):
    res = {"device": torch.cuda.get_device_name(0), "kernels": [], "append": []}
    for B, H, L, d in KVQ_SHAPES:
        res["kernels"] += bench_kvq(torch, _hip, B, H, L, d, args.rounds, args.warmup)
        r = bench_kvq_append(torch, _hip, B, H, L, d, args.rounds, args.warmup)
        print(json.dumps(r), flush=True)
        res["append"].append(r)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.kvq_out), exist_ok=True)
    with open(args.kvq_out, "w") as f:
        json.dump(res, f, indent=1)
    slow = [(r["shape"], k, round(r[f"{k}_over_fp32_time"], 3)) for r in res["kernels"] if r["group"] == 1
            for k in ("bf16", "fp8") if not r[f"{k}_faster_than_fp32"]]
    if slow:
        raise SystemExit(f"a quantised-cache step is not faster than the fp32-cache step by more than 4 % at {slow}")


PAGED_SIZES = (16, 128)


def bench_paged(torch, _hip, B, H, L, d, name, rounds, warmup):
    dt = torch.bfloat16 if name == "bf16" else torch.float32
    es = 2 if name == "bf16" else 4
    code = 1 if name == "bf16" else 0
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32).to(dt)  # noqa: E731
    q = rnd(B, 1, H, d).permute(0, 2, 1, 3)
    kvl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    o = torch.empty((B, 1, H, d), dtype=dt, device="cuda").permute(0, 2, 1, 3)
    m, l = (torch.empty((B, H, 1), dtype=torch.float32, device="cuda") for _ in range(2))
    rows = []
    for Hkv in (H, H // 4):
        kv_bytes = 2 * B * Hkv * L * d * es
        nset = min(72, max(2, -(-2 * ICACHE // kv_bytes) + 1))
        nsplit, span, tile = _hip.decode_splits(code, B, H, 1, L, d, Hkv=Hkv)
        ws_bytes = _hip.decode_workspace_bytes(code, B, H, 1, L, d, Hkv=Hkv)
        ws = torch.empty(max(1, ws_bytes // 4), dtype=torch.float32, device="cuda")
        legs = {}
        sets = [(rnd(B, L, Hkv, d).permute(0, 2, 1, 3), rnd(B, L, Hkv, d).permute(0, 2, 1, 3)) for _ in range(nset)]

        def contig(i, sets=sets):
            kc, vc = sets[i % nset]
            _hip.flash_decode(q, kc, vc, kv_len=kvl, causal=True, out=o, m=m, l=l, workspace=ws)
        legs["contig"] = contig
        for P in PAGED_SIZES:
            W = L // P
            assert W * P == L
            assert _hip.decode_paged_splits(code, B, H, 1, W, P, d, Hkv=Hkv) == (nsplit, span, tile)
            assert _hip.decode_paged_workspace_bytes(code, B, H, 1, W, P, d, Hkv=Hkv) == ws_bytes
            # every page of the pool in use, handed out in a shuffled order
            table = torch.randperm(B * W, generator=g, device="cuda").to(torch.int32).reshape(B, W).contiguous()
            pools = [(rnd(B * W, P, Hkv, d).permute(0, 2, 1, 3), rnd(B * W, P, Hkv, d).permute(0, 2, 1, 3))
                     for _ in range(nset)]

            def paged(i, pools=pools, table=table):
                kp, vp = pools[i % nset]
                _hip.flash_decode_paged(q, kp, vp, table, kv_len=kvl, causal=True, out=o, m=m, l=l, workspace=ws)
            legs[f"paged{P}"] = paged
        inner = nset * -(-24 // nset)   # whole turns over the leg's cache sets
        for fn in legs.values():
            for _ in range(warmup):
                _timed(torch, fn, inner)
        times = {k: [] for k in legs}
        names = list(legs)
        for r in range(rounds):  # the legs alternate inside every round, swapping places
            for k in names[r % len(names):] + names[:r % len(names)]:
                times[k].append(_timed(torch, legs[k], inner))
        med = {k: statistics.median(v) for k, v in times.items()}
        alg = kv_bytes + 2 * B * H * d * es + 2 * ws_bytes
        row = {"shape": [B, H, L, d], "dtype": name, "nq": 1, "kv_heads": Hkv, "group": H // Hkv, "rounds": rounds,
               "kv_bytes": kv_bytes, "algorithmic_bytes": alg, "splits": nsplit, "span_keys": span, "tile_keys": tile,
               "workspace_bytes": ws_bytes, "cache_sets_rotated": nset, "launches_per_timing": inner}
        for k in names:
            row.update({f"{k}_s_median": med[k], f"{k}_s_min": min(times[k]), f"{k}_s_max": max(times[k]),
                        f"{k}_bytes_per_s": alg / med[k]})
        for P in PAGED_SIZES:
            row[f"paged{P}_over_contig_time"] = med[f"paged{P}"] / med["contig"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del legs, sets, pools
        torch.cuda.empty_cache()
    return rows


def paged_memory(minitorch, lengths=(4096,) + (64,) * 7, n_head=16, head_dim=64):
    """nbytes of one-layer caches for a ragged batch: the contiguous KVCache pays B * n_positions rows,
    a PagedKVCache the pages the rows fill."""
    backend = minitorch.TensorBackend(minitorch.HipKernelOps)
    B, npos = len(lengths), max(lengths)
    plain = minitorch.KVCache(1, B, n_head, npos, head_dim, backend)
    out = {"lengths": list(lengths), "n_layer": 1, "n_head": n_head, "head_dim": head_dim, "n_positions": npos,
           "contiguous_nbytes": plain.nbytes}
    del plain
    for P in PAGED_SIZES:
        pages = sum(-(-n // P) for n in lengths)
        cache = minitorch.PagedKVCache(1, B, n_head, npos, head_dim, backend, page_size=P, n_pages=pages)
        cache.reserve(lengths)
        assert cache.pages_free == 0
        out[f"paged{P}_pages"] = pages
        out[f"paged{P}_nbytes"] = cache.nbytes
        out[f"paged{P}_over_contiguous_bytes"] = cache.nbytes / out["contiguous_nbytes"]
        del cache
    return out


def paged_legs(args, torch, minitorch, _hip):
    res = {"device": torch.cuda.get_device_name(0), "kernels": [], "memory": paged_memory(minitorch)}
    print(json.dumps(res["memory"]), flush=True)
    torch.cuda.empty_cache()
    for B, H, L, d in KVQ_SHAPES:
        for name in ("f32", "bf16"):
            res["kernels"] += bench_paged(torch, _hip, B, H, L, d, name, args.rounds, args.warmup)
    os.makedirs(os.path.dirname(args.paged_out), exist_ok=True)
    with open(args.paged_out, "w") as f:
        json.dump(res, f, indent=1)


def bench_generate(minitorch, n_positions, prompt_len, new_tokens, batch, rounds):
    np.random.seed(0)
    backend = minitorch.TensorBackend(minitorch.HipKernelOps)
    lm = minitorch.DecoderLM(n_vocab=10000, n_embd=256, n_head=8, n_positions=n_positions, p_dropout=0.0,
                             backend=backend, use_fused_kernel=True, use_flash_attention=True)
    rng = np.random.default_rng(0)
    prompts = [[int(t) for t in rng.integers(0, 10000, prompt_len)] for _ in range(batch)]
    legs = {"cached_batch": lambda: lm.generate(prompts, new_tokens, use_cache=True),
            "cached_one": lambda: lm.generate(prompts[:1], new_tokens, use_cache=True),
            "uncached_one": lambda: lm.generate(prompts[:1], new_tokens, use_cache=False)}
    out = {k: fn() for k, fn in legs.items()}  # warm-up; the legs must agree
    same = out["cached_one"] == out["uncached_one"] and out["cached_batch"][0] == out["cached_one"][0]
    rate = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            toks = fn()  # ends in a device-to-host copy of the last logits: synchronised
            rate[k].append(sum(len(t) for t in toks) / (time.perf_counter() - t0))
    return {"n_positions": n_positions, "prompt_len": prompt_len, "new_tokens": new_tokens, "batch": batch,
            "rounds": rounds, "legs_agree": bool(same),
            **{f"{k}_tokens_per_s_median": statistics.median(v) for k, v in rate.items()},
            **{f"{k}_tokens_per_s_best": max(v) for k, v in rate.items()}}


def bench_generate_graph(minitorch, n_positions, prompt_len, new_tokens, batch, rounds):
    np.random.seed(0)
    backend = minitorch.TensorBackend(minitorch.HipKernelOps)
    lm = minitorch.DecoderLM(n_vocab=10000, n_embd=256, n_head=8, n_positions=n_positions, p_dropout=0.0,
                             backend=backend, use_fused_kernel=True, use_flash_attention=True)
    rng = np.random.default_rng(0)
    prompts = [[int(t) for t in rng.integers(0, 10000, prompt_len)] for _ in range(batch)]
    sample = dict(temperature=0.8, top_k=50, seed=1)
    legs = {"graph_one": lambda: lm.generate(prompts[:1], new_tokens, graph=True),
            "cached_one": lambda: lm.generate(prompts[:1], new_tokens, use_cache=True),
            "uncached_one": lambda: lm.generate(prompts[:1], new_tokens, use_cache=False),
            "graph_batch": lambda: lm.generate(prompts, new_tokens, graph=True),
            "cached_batch": lambda: lm.generate(prompts, new_tokens, use_cache=True),
            "graph_batch_sampled": lambda: lm.generate(prompts, new_tokens, graph=True, **sample),
            "cached_batch_sampled": lambda: lm.generate(prompts, new_tokens, use_cache=True, **sample)}
    out = {k: fn() for k, fn in legs.items()}  # warm-up (captures the graphs); the legs must agree
    same = (out["graph_one"] == out["cached_one"] == out["uncached_one"] and out["graph_batch"] == out["cached_batch"]
            and out["graph_batch_sampled"] == out["cached_batch_sampled"])
    captures = lm.graph_captures
    rate = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            toks = fn()  # every leg ends in a device-to-host copy: synchronised
            rate[k].append(sum(len(t) for t in toks) / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in rate.items()}
    return {"n_positions": n_positions, "prompt_len": prompt_len, "new_tokens": new_tokens, "batch": batch,
            "rounds": rounds, "legs_agree": bool(same), "graph_captures": captures,
            "recaptured_while_timing": lm.graph_captures != captures,
            **{f"{k}_tokens_per_s_median": v for k, v in med.items()},
            **{f"{k}_tokens_per_s_best": max(v) for k, v in rate.items()},
            "graph_over_cached_one": med["graph_one"] / med["cached_one"],
            "graph_over_cached_batch": med["graph_batch"] / med["cached_batch"]}


def bench_select(torch, _hip, B, V, rounds, warmup, inner=64):
    g = torch.Generator(device="cuda").manual_seed(0)
    logits = 3.0 * torch.randn(B, V, generator=g, device="cuda", dtype=torch.float32)
    out = torch.empty(B, dtype=torch.float32, device="cuda")
    out_i = torch.empty(B, dtype=torch.int32, device="cuda")
    kinds = {"greedy": dict(temperature=0.0), "top_k_50": dict(temperature=1.0, top_k=50),
             "whole_vocabulary": dict(temperature=1.0, top_k=0)}
    if hasattr(_hip.lib(), "mt_select_token_p"):  # an older build under --lib runs the three legs above
        kinds.update({"top_p_0.9": dict(temperature=1.0, top_k=0, top_p=0.9),
                      "top_k_50_top_p_0.9": dict(temperature=1.0, top_k=50, top_p=0.9),
                      "min_p_0.05": dict(temperature=1.0, top_k=0, min_p=0.05)})
    legs = {k: (lambda i, kw=kw: _hip.select_token(logits, seed=i, out=out, out_i32=out_i, **kw)) for k, kw in kinds.items()}
    for fn in legs.values():
        for _ in range(warmup):
            _timed(torch, fn, inner)
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(_timed(torch, fn, inner))
    return {"B": B, "V": V, "rounds": rounds, "launches_per_timing": inner, "row_bytes": 4 * V,
            **{f"{k}_s_median": statistics.median(v) for k, v in times.items()},
            **{f"{k}_s_min": min(v) for k, v in times.items()}}


def graph_legs(args, torch, minitorch, _hip):
    res = {"device": torch.cuda.get_device_name(0), "select_token": [], "generate": []}
    for B, V in ((8, 10000), (64, 10000)):
        r = bench_select(torch, _hip, B, V, args.rounds, args.warmup)
        print(json.dumps(r), flush=True)
        res["select_token"].append(r)
    for npos, plen, new, batch, rounds in ((40, 8, 32, 8, 5), (1024, 768, 128, 8, 3)):
        r = bench_generate_graph(minitorch, npos, plen, new, batch, rounds)
        print(json.dumps(r), flush=True)
        res["generate"].append(r)
    os.makedirs(os.path.dirname(args.graph_out), exist_ok=True)
    with open(args.graph_out, "w") as f:
        json.dump(res, f, indent=1)


ROPE_SHAPES = [(8, 16, 1, 64, "decode step"), (8, 16, 512, 64, "extend step")]


def bench_rope(torch, minitorch, _hip, B, H, T, d, what, rounds, warmup):
    """mt_rope on Q and K [B,H,T,d] (the model's [B,T,H,d] projection storage, one two-tensor
    launch, positions from a device vector) against a device-to-device copy of the same bytes,
    the floor of a kernel that reads every byte once and writes it once. Both legs rotate over the
    same source / destination sets, enough of them to exceed twice the Infinity Cache."""
    n_pos = 4096
    tab = minitorch.RotaryTable(n_pos, d)
    cos, sin = torch.from_numpy(tab.cos_host).cuda(), torch.from_numpy(tab.sin_host).cuda()
    nbytes = 2 * B * H * T * d * 4  # Q and K, read once and written once each
    sets = max(2, min(64, -(-2 * ICACHE // (2 * nbytes))))
    g = torch.Generator(device="cuda").manual_seed(0)
    src = [torch.randn(2, B, T, H, d, generator=g, device="cuda") for _ in range(sets)]
    dst = [torch.empty_like(s) for s in src]
    pos0 = torch.randint(0, n_pos - T, (B,), generator=g, device="cuda", dtype=torch.int32)
    view = lambda t: t.permute(0, 2, 1, 3)  # noqa: E731
    inner = 64 if T == 1 else 16

    def rope(i):
        s, o = src[i % sets], dst[i % sets]
        _hip.rope(view(s[0]), cos, sin, pos0=pos0, out=view(o[0]), x2=view(s[1]), out2=view(o[1]))

    def copy(i):
        dst[i % sets].copy_(src[i % sets])
    legs = {"rope": rope, "copy": copy}
    for fn in legs.values():
        for _ in range(warmup):
            _timed(torch, fn, inner)
    # the same `inner` launches as one captured graph each: an eager leg cannot go below the host's
    # time to issue a launch, which exceeds these kernels' run time; a replay issues nothing
    graphs = {}
    for k, fn in list(legs.items()):
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k]):
            for i in range(inner):
                fn(i)
        legs[k + "_graph"] = lambda i, g=graphs[k]: g.replay()
        for _ in range(warmup):
            _timed(torch, legs[k + "_graph"], 4)
    times = {k: [] for k in legs}
    for r in range(rounds):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            if k.endswith("_graph"):  # one replay is `inner` launches
                times[k].append(_timed(torch, legs[k], 4) / inner)
            else:
                times[k].append(_timed(torch, legs[k], inner))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"what": what, "B": B, "H": H, "Hkv": H, "T": T, "d": d, "rounds": rounds, "launches_per_timing": inner,
            "sets": sets, "bytes_read_plus_written": 2 * nbytes,
            **{f"{k}_s_median": v for k, v in med.items()}, **{f"{k}_s_min": min(v) for k, v in times.items()},
            "rope_bytes_per_s": 2 * nbytes / med["rope"], "copy_bytes_per_s": 2 * nbytes / med["copy"],
            "rope_over_copy_time": med["rope"] / med["copy"],
            "rope_graph_bytes_per_s": 2 * nbytes / med["rope_graph"],
            "copy_graph_bytes_per_s": 2 * nbytes / med["copy_graph"],
            "rope_over_copy_time_graph": med["rope_graph"] / med["copy_graph"]}


def bench_generate_rope(minitorch, n_positions, prompt_len, new_tokens, batch, rounds):
    """generate(graph=True) tokens/s of the rotary model against the learned-position model, the
    sizes of the graph legs; the legs alternate inside every round."""
    backend = minitorch.TensorBackend(minitorch.HipKernelOps)
    rng = np.random.default_rng(0)
    prompts = [[int(t) for t in rng.integers(0, 10000, prompt_len)] for _ in range(batch)]
    legs, agree = {}, {}
    for enc in ("learned", "rope"):
        np.random.seed(0)
        lm = minitorch.DecoderLM(n_vocab=10000, n_embd=256, n_head=8, n_positions=n_positions, p_dropout=0.0,
                                 backend=backend, use_fused_kernel=True, use_flash_attention=True, pos_encoding=enc)
        legs[f"{enc}_graph_one"] = lambda lm=lm: lm.generate(prompts[:1], new_tokens, graph=True)
        legs[f"{enc}_graph_batch"] = lambda lm=lm: lm.generate(prompts, new_tokens, graph=True)
        # warm-up (captures the graphs); the graph leg must give the eager cached leg's ids
        agree[enc] = (legs[f"{enc}_graph_batch"]() == lm.generate(prompts, new_tokens, use_cache=True)
                      and legs[f"{enc}_graph_one"]() == lm.generate(prompts[:1], new_tokens, use_cache=True))
    rate = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            toks = fn()  # ends in a device-to-host copy: synchronised
            rate[k].append(sum(len(t) for t in toks) / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in rate.items()}
    return {"n_positions": n_positions, "prompt_len": prompt_len, "new_tokens": new_tokens, "batch": batch,
            "rounds": rounds, "graph_equals_eager": agree,
            **{f"{k}_tokens_per_s_median": v for k, v in med.items()},
            **{f"{k}_tokens_per_s_best": max(v) for k, v in rate.items()},
            "rope_over_learned_one": med["rope_graph_one"] / med["learned_graph_one"],
            "rope_over_learned_batch": med["rope_graph_batch"] / med["learned_graph_batch"]}


def rope_legs(args, torch, minitorch, _hip):
    res = {"device": torch.cuda.get_device_name(0), "kernels": [], "generate": []}
    for B, H, T, d, what in ROPE_SHAPES:
        r = bench_rope(torch, minitorch, _hip, B, H, T, d, what, args.rounds, args.warmup)
        print(json.dumps(r), flush=True)
        res["kernels"].append(r)
        torch.cuda.empty_cache()
    for npos, plen, new, batch, rounds in ((40, 8, 32, 8, 5), (1024, 768, 128, 8, 3)):
        r = bench_generate_rope(minitorch, npos, plen, new, batch, rounds)
        print(json.dumps(r), flush=True)
        res["generate"].append(r)
    os.makedirs(os.path.dirname(args.rope_out), exist_ok=True)
    with open(args.rope_out, "w") as f:
        json.dump(res, f, indent=1)


def _graph_of(torch, fn, inner):
    """`inner` calls of fn(i) as one captured graph (after one eager pass); returns a leg for _timed."""
    for i in range(inner):
        fn(i)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(inner):
            fn(i)
    return lambda i: g.replay()


def bench_spec_verify(torch, _hip, B, H, L, d, rounds, warmup, inner=16):
    """The attention of a verify step: mt_flash_attn_decode on k + 1 = 2, 4, 8 query rows per
    (batch, head) against the one-row step, fp32 cache, every leg a captured graph of `inner`
    launches over rotated cache sets (as bench_shape rotates them); the legs alternate."""
    kv_bytes = 2 * B * H * L * d * 4
    nset = min(8, max(2, -(-2 * ICACHE // kv_bytes) + 1))
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32)  # noqa: E731
    caches = [(rnd(B, L, H, d).permute(0, 2, 1, 3), rnd(B, L, H, d).permute(0, 2, 1, 3)) for _ in range(nset)]
    kvl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    legs, plans = {}, {}
    for nq in (1, 2, 4, 8):
        q = rnd(B, nq, H, d).permute(0, 2, 1, 3)
        o = torch.empty((B, nq, H, d), dtype=torch.float32, device="cuda").permute(0, 2, 1, 3)
        m, l = (torch.empty((B, H, nq), dtype=torch.float32, device="cuda") for _ in range(2))
        ws_bytes = _hip.decode_workspace_bytes(0, B, H, nq, L, d)
        ws = torch.empty(max(1, ws_bytes // 4), dtype=torch.float32, device="cuda") if ws_bytes else None
        plans[nq] = _hip.decode_splits(0, B, H, nq, L, d)[0]

        def decode(i, q=q, o=o, m=m, l=l, ws=ws):
            kc, vc = caches[i % nset]
            _hip.flash_decode(q, kc, vc, kv_len=kvl, causal=True, out=o, m=m, l=l, workspace=ws)
        legs[nq] = _graph_of(torch, decode, inner)
    for fn in legs.values():
        for _ in range(warmup):
            _timed(torch, fn, 4)
    times = {k: [] for k in legs}
    for r in range(rounds):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            times[k].append(_timed(torch, legs[k], 4) / inner)
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"shape": [B, H, L, d], "dtype": "f32", "rounds": rounds, "launches_per_graph": inner,
            "cache_sets_rotated": nset, "splits": plans,
            **{f"decode_nq{k}_s_median": v for k, v in med.items()},
            **{f"decode_nq{k}_s_min": min(v) for k, v in times.items()},
            **{f"nq{k}_over_nq1": med[k] / med[1] for k in (2, 4, 8)}}


def bench_spec_kernels(torch, _hip, B, V, S, k, rounds, warmup, inner=32):
    """mt_spec_draft + mt_spec_accept alone (the step's overhead beside the model): a captured
    graph of `inner` draft + accept pairs over rows of S tokens and [B, k + 1, V] logits, greedy
    and top-k sampling, against mt_select_token on [B, V] (what a one-token step pays)."""
    g = torch.Generator(device="cuda").manual_seed(0)
    n = k + 1
    logits = 3.0 * torch.randn(B, n, V, generator=g, device="cuda", dtype=torch.float32)
    tokens = torch.randint(0, 50, (B, S), generator=g, device="cuda", dtype=torch.int32)
    i32 = lambda *s, v=0: torch.full(s, v, dtype=torch.int32, device="cuda")  # noqa: E731
    st = dict(held=i32(B, v=S - n - 1), count=i32(B, v=1), limit=i32(B, v=1 << 30), done=i32(B),
              history=i32(B, S), scratch=i32(B, n), feed_i32=i32(B, n), n_draft=i32(B),
              feed_f32=torch.zeros(B * n, dtype=torch.float32, device="cuda"), cache=i32(B), a=i32(B), dr=i32(B))
    seed = torch.zeros(1, dtype=torch.int64, device="cuda")
    out, out_i = torch.empty(B, dtype=torch.float32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    kinds = {"greedy": dict(temperature=0.0), "top_k_50": dict(temperature=1.0, top_k=50)}

    def pair(i, kw):
        # the rows' state is put back first (two tiny fills), so that every pair does the same work
        st["held"].fill_(S - n - 1)
        st["count"].fill_(1)
        _hip.spec_draft(tokens, st["held"], k, 3, feed_f32=st["feed_f32"], feed_i32=st["feed_i32"],
                        n_draft=st["n_draft"])
        _hip.spec_accept(logits, st["feed_i32"], st["n_draft"], st["limit"], st["count"], st["held"], st["done"],
                         tokens, st["history"], scratch=st["scratch"], cache_len=st["cache"], drafted=st["dr"],
                         accepted=st["a"], seed_dev=seed, **kw)
    legs = {}
    for name, kw in kinds.items():
        legs[f"spec_{name}"] = _graph_of(torch, lambda i, kw=kw: pair(i, kw), inner)
        legs[f"select_{name}"] = _graph_of(
            torch, lambda i, kw=kw: _hip.select_token(logits[:, 0], seed_dev=seed, out=out, out_i32=out_i, **kw), inner)
    for fn in legs.values():
        for _ in range(warmup):
            _timed(torch, fn, 4)
    times = {name: [] for name in legs}
    for r in range(rounds):
        for name in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            times[name].append(_timed(torch, legs[name], 4) / inner)
    return {"B": B, "V": V, "S": S, "k": k, "rounds": rounds, "launches_per_graph": inner,
            "note": "spec_* = two fills + mt_spec_draft + mt_spec_accept (select over B (k + 1) rows + bookkeeping)",
            **{f"{name}_s_median": statistics.median(v) for name, v in times.items()},
            **{f"{name}_s_min": min(v) for name, v in times.items()}}


def bench_generate_spec(minitorch, workload, n_positions, prompts, new_tokens, rounds, pos_encoding="learned",
                        n_vocab=10000):
    """generate(graph=True) tokens/s with speculate in {2, 4, 7} against speculate=None on the same
    model, with each leg's acceptance rate (accepted / drafted) and emitted tokens per row and step;
    the legs alternate inside every round and must return the plain ids."""
    np.random.seed(0)
    backend = minitorch.TensorBackend(minitorch.HipKernelOps)
    lm = minitorch.DecoderLM(n_vocab=n_vocab, n_embd=256, n_head=8, n_positions=n_positions, p_dropout=0.0,
                             backend=backend, use_fused_kernel=True, use_flash_attention=True,
                             pos_encoding=pos_encoding)
    batch = len(prompts)
    legs = {"plain": lambda: lm.generate(prompts, new_tokens, graph=True)}
    for k in (2, 4, 7):
        legs[f"speculate_{k}"] = lambda k=k: lm.generate(prompts, new_tokens, graph=True, speculate=k)
    out, stats = {}, {}
    for name, fn in legs.items():  # warm-up (captures the graphs)
        out[name] = fn()
        stats[name] = dict(lm.spec_stats) if name != "plain" else None
    rate = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            toks = fn()  # ends in a device-to-host copy: synchronised
            rate[name].append(sum(len(t) for t in toks) / (time.perf_counter() - t0))
    med = {name: statistics.median(v) for name, v in rate.items()}
    res = {"workload": workload, "pos_encoding": pos_encoding, "n_vocab": n_vocab, "n_positions": n_positions,
           "prompt_len": len(prompts[0]), "new_tokens": new_tokens, "batch": batch, "rounds": rounds,
           "ids_equal_plain": all(out[name] == out["plain"] for name in legs),
           "tokens_returned": sum(len(t) for t in out["plain"]),
           "plain_tokens_per_s_median": med["plain"], "plain_tokens_per_s_best": max(rate["plain"])}
    for name, s in stats.items():
        if s is None:
            continue
        res[name] = {"tokens_per_s_median": med[name], "tokens_per_s_best": max(rate[name]),
                     "over_plain": med[name] / med["plain"], **s,
                     "acceptance_rate": s["accepted"] / s["drafted"] if s["drafted"] else 0.0,
                     "tokens_per_row_step": (s["tokens"] - batch) / (batch * s["steps"]) if s["steps"] else 0.0}
    lm.drop_decode_graphs()
    return res


def spec_legs(args, torch, minitorch, _hip):
    res = {"device": torch.cuda.get_device_name(0), "verify_attention": [], "draft_accept": [], "generate": []}
    r = bench_spec_verify(torch, _hip, 8, 16, 4096, 64, args.rounds, args.warmup)
    print(json.dumps(r), flush=True)
    res["verify_attention"].append(r)
    torch.cuda.empty_cache()
    for k in (1, 3, 7):
        r = bench_spec_kernels(torch, _hip, 8, 10000, 1025, k, args.rounds, args.warmup)
        print(json.dumps(r), flush=True)
        res["draft_accept"].append(r)
    rng = np.random.default_rng(0)
    # a workload whose greedy continuation loops: a randomly initialised rotary model over a
    # 97-token vocabulary falls into short cycles (what it accepts is recorded); and one whose
    # drafts are (nearly) never right: random prompts over 10000 tokens, the overhead
    small = [[int(t) for t in rng.integers(0, 97, 64)] for _ in range(8)]
    rand = [[int(t) for t in rng.integers(0, 10000, 64)] for _ in range(8)]
    for workload, prompts, enc, n_vocab in (("looping continuation", small[:1], "rope", 97),
                                            ("looping continuation", small, "rope", 97),
                                            ("random prompt", rand[:1], "learned", 10000),
                                            ("random prompt", rand, "learned", 10000)):
        r = bench_generate_spec(minitorch, workload, 1024, prompts, 256, 3, pos_encoding=enc, n_vocab=n_vocab)
        print(json.dumps(r), flush=True)
        res["generate"].append(r)
    os.makedirs(os.path.dirname(args.spec_out), exist_ok=True)
    with open(args.spec_out, "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spec-legs", action="store_true",
                    help="run the speculative-decoding legs instead, into --spec-out")
    ap.add_argument("--spec-out", default=os.path.join(ROOT, "profiles", "spec_bench.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_bench.json"))
    ap.add_argument("--graph-legs", action="store_true",
                    help="run the generate(graph=True) and select_token legs instead, into --graph-out")
    ap.add_argument("--graph-out", default=os.path.join(ROOT, "profiles", "generate_graph_bench.json"))
    ap.add_argument("--gqa-legs", action="store_true",
                    help="run the grouped-query decode legs instead, into --gqa-out")
    ap.add_argument("--gqa-out", default=os.path.join(ROOT, "profiles", "decode_gqa_bench.json"))
    ap.add_argument("--extend-legs", action="store_true",
                    help="run the extend-attention legs instead, into --extend-out")
    ap.add_argument("--extend-out", default=os.path.join(ROOT, "profiles", "extend_bench.json"))
    ap.add_argument("--extend-src-legs", action="store_true",
                    help="run only the paged / quantised extend legs, into --extend-src-out")
    ap.add_argument("--extend-src-out", default=os.path.join(ROOT, "profiles", "extend_src_bench.json"))
    ap.add_argument("--lib", default=None,
                    help="another build of libminitorch_hip.so to load (the extend source legs' A/B)")
    ap.add_argument("--kvq-legs", action="store_true",
                    help="run the quantised-KV-cache decode legs instead, into --kvq-out")
    ap.add_argument("--kvq-out", default=os.path.join(ROOT, "profiles", "decode_kvq_bench.json"))
    ap.add_argument("--paged-legs", action="store_true",
                    help="run the paged-KV-cache decode legs instead, into --paged-out")
    ap.add_argument("--paged-out", default=os.path.join(ROOT, "profiles", "decode_paged_bench.json"))
    ap.add_argument("--rope-legs", action="store_true",
                    help="run the rotary-embedding legs instead, into --rope-out")
    ap.add_argument("--rope-out", default=os.path.join(ROOT, "profiles", "rope_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-generate", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench.py needs an MI355X (no timing is taken on a CPU)")
    import minitorch
    from minitorch import _hip
    if args.lib:
        _hip.use_library(os.path.abspath(args.lib), allow_missing=True)
    if args.spec_legs:
        return spec_legs(args, torch, minitorch, _hip)
    if args.extend_src_legs:
        return extend_src_legs(args, torch, _hip)
    if args.graph_legs:
        return graph_legs(args, torch, minitorch, _hip)
    if args.gqa_legs:
        return gqa_legs(args, torch, _hip)
    if args.extend_legs:
        try:
            extend_legs(args, torch, _hip)
        finally:
            extend_src_legs(args, torch, _hip)
        return
    if args.kvq_legs:
        return kvq_legs(args, torch, _hip)
    if args.paged_legs:
        return paged_legs(args, torch, minitorch, _hip)
    if args.rope_legs:
        return rope_legs(args, torch, minitorch, _hip)
    res = {"device": torch.cuda.get_device_name(0), "kernels": [], "generate": []}
    for B, H, L, d, name in SHAPES:
        r = bench_shape(torch, _hip, B, H, L, d, name, args.rounds, args.warmup)
        print(json.dumps(r), flush=True)
        res["kernels"].append(r)
        torch.cuda.empty_cache()
    if not args.skip_generate:
        for npos, plen, new, batch, rounds in ((40, 8, 32, 8, 3), (1024, 768, 128, 8, 2)):
            r = bench_generate(minitorch, npos, plen, new, batch, rounds)
            print(json.dumps(r), flush=True)
            res["generate"].append(r)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
