#!/usr/bin/env python3
"""Headline benchmark: FlashAttention forward TFLOP/s + HBM GB/s at (B,H,N,d) =
(8,16,4096,64) bf16 (BASELINE.json metric, configs[2]), on 1, 2, 4 or 8 GPUs.

    python bench.py --gpus N --steps K --warmup W [--config c3|c4] [--split strong|weak]
                    [--full] [--dump-outputs DIR]

A plain run does only what the headline figure needs: it builds the inputs, warms up, times
exactly K steps and prints the result line. --full adds the side legs (N = 1): `extra`
(causal, backward, fp32 config 2, the config-4 shard, the config-5 training step), the
`cpu_baseline` and the `parity` of the timed output against the CPU reference; --no-extra
and --no-cpu drop one of them from a --full run. --dump-outputs DIR writes what the last
timed step computed (O, and with N = 1 the row statistics m and l) as DIR/<name>.npy,
float32, at most 64 MB in all: whole arrays when they fit, else the same fixed seeded sample
of (b,h,row) rows of each. The inputs are counter-seeded, so two runs with the same arguments
see identical Q/K/V and two builds can be compared output for output.

One "step" = one pass of the hot path (the bf16 MFMA forward kernel) over this rank's
shard of the workload, with synthetic Q/K/V already resident in HBM. Since round 6 the timed
form writes an fp32 O (bf16 Q/K/V, bf16 MFMAs with fp32 accumulation, O without a final
bf16 rounding: MT_BF16_F32OUT), the form that meets north_star's flat 1e-3 max-abs against
the CPU reference on every head; --out bf16 times the bf16-O form, whose rounding of O alone
is up to 9.8e-4 where |O| reaches 0.5 (its throughput is in "extra"). Multi-GPU: one
process per GPU (torch.distributed.run, RCCL). The flattened batch x heads axis is
sharded into contiguous per-rank ranges (every (b,h) head is
independent, so there is no collective on the data path):

  --config c3 (default)  the global problem is (8,16,4096,64).
      --split strong (default): rank r owns heads [r*128/N, (r+1)*128/N): the total work
                         is fixed, "scaling": "strong".
      --split weak:      every rank owns a full (8,16,4096,64) slice of a global
                         (8N,16,4096,64) problem: "scaling": "weak".
  --config c4            BASELINE config 4: global (64,16,16384,128), strong split
                         (1024/N heads per rank; at N = 1 the whole 2^31-element-per-tensor
                         problem runs on one GPU).

`value` = the global problem's flops per step x steps / the max-over-ranks wall time of
the timed region (compute only: the forward kernel on every rank). With N > 1 the line
also carries "end_to_end": the same steps with the RCCL all-gather of every rank's O
shard (all_gather_into_tensor over xGMI) inside the timed region, max over ranks.

rank 0 prints ONE JSON line with the contract fields plus:
  roofline     : achieved TFLOP/s of the forward kernel (algorithmic flops / mean kernel
                 duration from HIP events on the launch stream) vs the dense bf16 MFMA
                 peak; "traffic" = HBM bytes per launch from the committed rocprofv3 PMC
                 capture (profiles/pmc_*.json), or null.
  cpu_baseline : (--full) the C restatement of the reference's CPU fast_ops attention
                 (oracle/attn_ref.c), timed on a bounded sample of heads of the same
                 workload on this host's cores (rank 0, N = 1 only).

The orchestration (`run`) takes the attention function, the device and the process group
as arguments, so tests/test_bench_dist.py drives the N > 1 code path on CPU with gloo
and an injected attention.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "llmsys-project-flashattn_amd"))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2516.6   # 256 CU x 4096 flop/clk x 2.4 GHz (MI355X_MICROARCH.md, dense)
PEAK_F32_TFLOPS = 157.3
PEAK_HBM_GBPS = 8000.0
CONFIGS = {"c3": (8, 16, 4096, 64), "c4": (64, 16, 16384, 128)}
WORKLOAD = CONFIGS["c3"]
PREWARM_S = 0.3  # untimed steady-clock ramp before the timed region (seconds)
METRIC = "FlashAttn fwd TFLOP/s (+ HBM GB/s) at (B,H,N,d)=(8,16,4096,64); 1/2/4/8 GPU"


def _sig(x, n=6):
    """x to n significant digits (tiny CPU-test throughputs must not round to 0)."""
    return float(f"{x:.{n}g}")


def fwd_flops(B, H, N, d, causal=False):
    f = 4.0 * B * H * N * N * d
    return f / 2 if causal else f


def fwd_bytes(B, H, N, d, esize=2, out_esize=None):
    # read Q, K, V + write O (out_esize bytes per element; default: the input size), plus the
    # fp32 row statistics m and l
    oe = esize if out_esize is None else out_esize
    return (3.0 * esize + oe) * B * H * N * d + 2.0 * B * H * N * 4


# ---- sharding plan -------------------------------------------------------------------
def shard_plan(global_shape, world, rank, split="strong"):
    """Per-rank slice of the flattened B*H axis.

    strong: the global problem is fixed and rank r owns heads [r*BH/W, (r+1)*BH/W); the
    shard is (B/W, H, N, d) when W divides B, else (1, BH/W, N, d) (both are one
    contiguous block of the [B,H,N,d] layout). weak: every rank owns a full copy-shaped
    slice, global = (W*B, H, N, d). Returns dict(global_shape, shard_shape, bh_lo, bh_hi)."""
    B, H, N, d = global_shape
    if split == "weak":
        return {"global_shape": (B * world, H, N, d), "shard_shape": (B, H, N, d),
                "bh_lo": rank * B * H, "bh_hi": (rank + 1) * B * H}
    if split != "strong":
        raise ValueError(f"unknown split {split!r}")
    BH = B * H
    if BH % world:
        raise ValueError(f"B*H = {BH} heads do not split evenly over {world} ranks")
    per = BH // world
    shard = (B // world, H, N, d) if B % world == 0 else (1, per, N, d)
    return {"global_shape": (B, H, N, d), "shard_shape": shard, "bh_lo": rank * per,
            "bh_hi": (rank + 1) * per}


def make_shard(torch, shard_shape, bh_lo, dtype, seed, device):
    """Synthetic N(0,1) inputs from a generator keyed by (seed, global head index), so the
    shard of rank r equals heads [bh_lo, bh_lo + rows) of the global tensor whatever W is."""
    Bs, Hs, N, d = shard_shape
    out = torch.empty(shard_shape, dtype=dtype, device=device)
    flat = out.view(Bs * Hs, N, d)
    g = torch.Generator(device=device)
    for i in range(Bs * Hs):
        g.manual_seed(seed * 1000003 + bh_lo + i)
        flat[i].copy_(torch.randn((N, d), generator=g, device=device, dtype=torch.float32))
    return out


class Clock:
    """Device timing: HIP events on the launch stream on a GPU, perf_counter on CPU."""

    def __init__(self, torch, device):
        self.torch = torch
        self.gpu = device != "cpu"

    def sync(self):
        if self.gpu:
            self.torch.cuda.synchronize()

    def span(self, fn, steps):
        """(mean ms per call of fn over `steps` calls, measured on the device)."""
        if self.gpu:
            st = self.torch.cuda.current_stream()
            e0 = self.torch.cuda.Event(enable_timing=True)
            e1 = self.torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(steps):
                fn()
            e1.record(st)
            self.torch.cuda.synchronize()
            return e0.elapsed_time(e1) / steps
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / steps


def _timed_region(torch, clock, dist, world, fn, steps):
    """Barrier + sync on both sides of exactly `steps` calls; returns (wall s and device ms
    per call, both the MAX over ranks; this rank's own device ms per call)."""
    if world > 1:
        dist.barrier()
    clock.sync()
    t0 = time.perf_counter()
    dev_ms = clock.span(fn, steps)
    clock.sync()
    if world > 1:
        dist.barrier()
    clock.sync()
    wall = time.perf_counter() - t0
    own_ms = dev_ms
    if world > 1:
        t = torch.tensor([wall, dev_ms], dtype=torch.float64)
        if clock.gpu:
            t = t.cuda()
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall, dev_ms = float(t[0]), float(t[1])
    return wall, dev_ms, own_ms


def run(args, attn_fwd, torch, dist, world, rank, device, dtype, esize=2, out_esize=None):
    """The bench's timed legs for this rank. attn_fwd(q, k, v, causal, out) runs the hot
    path on a shard; out_esize 4 with bf16 inputs: an fp32 O (the headline form since round
    6, MT_BF16_F32OUT: the one that meets north_star's flat 1e-3). Returns the result dict
    (rank 0 prints it) and, for tests, the gathered output (N > 1) or this rank's output."""
    out_esize = esize if out_esize is None else out_esize
    base = CONFIGS[args.config] if args.shape is None else tuple(args.shape)
    split = "strong" if args.config == "c4" else args.split
    plan = shard_plan(base, world, rank, split)
    gshape, sshape = plan["global_shape"], plan["shard_shape"]
    q, k, v = (make_shard(torch, sshape, plan["bh_lo"], dtype, s, device) for s in (1, 2, 3))
    o = torch.empty_like(q, dtype=torch.float32 if out_esize == 4 else dtype)
    clock = Clock(torch, device)

    def step():
        attn_fwd(q, k, v, args.causal, o)

    for _ in range(args.warmup):
        step()
    clock.sync()
    # untimed clock ramp: keep stepping until PREWARM_S of device work has run, so the
    # timed region starts at the steady-state clock whatever W the caller passes (the
    # first launches on a cold GPU run up to 30 % slower: profiles/r1e_kernel_stats.csv)
    t_ramp = time.perf_counter()
    while clock.gpu and time.perf_counter() - t_ramp < PREWARM_S:
        for _ in range(10):
            step()
        clock.sync()

    # kern_ms: this rank's mean kernel time from HIP events on the launch stream over the
    # timed region (the roofline's denominator)
    wall, kern_ms_max, kern_ms = _timed_region(torch, clock, dist, world, step, args.steps)
    B, H, N, d = gshape
    total_flops = fwd_flops(B, H, N, d, args.causal) * args.steps
    value = total_flops / wall / 1e12
    flops_rank = fwd_flops(*sshape, args.causal)
    achieved = flops_rank / (kern_ms * 1e-3) / 1e12
    alg_bytes = fwd_bytes(*sshape, esize=esize, out_esize=out_esize)
    tag = (("fwd_bf16_c4" if args.config == "c4" else "fwd_bf16_c3") + ("_causal" if args.causal else "")
           + ("_f32out" if esize == 2 and out_esize == 4 else ""))
    traffic, traffic_src, pmc_extra = load_pmc_traffic(tag) if world == 1 else (None, None, {})

    result = {
        "metric": METRIC,
        "value": _sig(value),
        "unit": "TFLOP/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "prewarm_s": PREWARM_S,
        "ms_per_step": round(wall * 1e3 / args.steps, 5),
        "higher_is_better": True,
        "scaling": split,
        "vs_baseline": None,
        "dtype": "bf16" if esize == 2 else "f32",
        "data": "synthetic N(0,1) Q/K/V (counter-seeded per global head), resident in HBM",
        "config": {"workload": f"flash_attention_fwd {args.config}", "B": B, "H": H, "N": N,
                   "d": d, "per_gpu_shape": list(sshape), "causal": bool(args.causal),
                   "output": "fp32 O" if out_esize == 4 else ("bf16 O" if esize == 2 else "fp32 O"),
                   "parallelism": f"bh-shard x{world} ({split})"},
        "hbm_gbps": round(fwd_bytes(B, H, N, d, esize, out_esize) * args.steps / wall / 1e9, 2),
        "roofline": {
            "bound": "mfma",
            "achieved": round(achieved, 2),
            "peak": PEAK_BF16_TFLOPS if esize == 2 else PEAK_F32_TFLOPS,
            "unit": "TFLOP/s",
            "frac": round(achieved / (PEAK_BF16_TFLOPS if esize == 2 else PEAK_F32_TFLOPS), 4),
            "traffic": traffic,
            "traffic_source": traffic_src,
            "pmc_mfma_busy_frac": pmc_extra.get("mfma_busy_frac"),
            "pmc_effective_clock_ghz": pmc_extra.get("effective_clock_ghz"),
            "algorithmic_bytes": alg_bytes,
            "algorithmic_flops": flops_rank,
            "kernel_ms": round(kern_ms, 5),
            "kernel_ms_max_over_ranks_timed": round(kern_ms_max, 5),
        },
    }

    gathered = None
    if world > 1:
        # end to end: the forward plus the RCCL all-gather of the O shards, both inside the
        # timed region (SURVEY.md §8(e) leg (ii)); serial = one gather after the whole
        # forward, overlapped = the rank's rows in `chunks` block-cyclic pieces, each piece's
        # gather issued asynchronously while the next piece computes (minitorch/shard.py
        # chunk_rows: every gather lands in place in the global head order)
        gathered = torch.empty((world * o.shape[0],) + tuple(o.shape[1:]), dtype=o.dtype,
                               device=o.device)

        def step_gather():
            step()
            dist.all_gather_into_tensor(gathered, o)

        for _ in range(2):
            step_gather()
        clock.sync()
        tg, _, _ = _timed_region(torch, clock, dist, world, step_gather, args.steps)
        obytes = o.numel() * o.element_size()
        serial = {
            "what": "forward + one all_gather_into_tensor of every rank's O shard, per step",
            "ms_per_step": round(tg * 1e3 / args.steps, 4),
            "tflops": _sig(total_flops / tg / 1e12),
            "gathered_bytes_per_rank": int(obytes * world),
            "allgather_gbps_per_rank": round(obytes * (world - 1) * args.steps
                                             / max(tg - wall, 1e-9) / 1e9, 2),
        }
        result["end_to_end"] = serial
        # default: as many chunks (up to 4) as keep each chunk's forward grid at one
        # workgroup per CU (minitorch/shard.py occupancy_chunks: C3 from 4 ranks up stays
        # unchunked, C4 at 8 ranks takes 4)
        from minitorch.shard import occupancy_chunks
        chunks = args.chunks if args.chunks is not None else occupancy_chunks(
            B, H, N, d, world, args.causal, max_chunks=4)
        BHg = B * H
        if chunks > 1 and BHg % (world * chunks) == 0:
            from minitorch.shard import chunk_rows
            rc = BHg // (world * chunks)
            pieces = []
            for c in range(chunks):
                lo = chunk_rows(BHg, world, rank, chunks, c)[0]
                qc, kc, vc = (make_shard(torch, (1, rc, N, d), lo, dtype, s_, device) for s_ in (1, 2, 3))
                pieces.append((qc, kc, vc, torch.empty_like(qc, dtype=o.dtype)))
            gathered_c = torch.empty_like(gathered)

            def step_overlap():
                works = []
                for c, (qc, kc, vc, oc) in enumerate(pieces):
                    attn_fwd(qc, kc, vc, args.causal, oc)
                    n = world * rc
                    works.append(dist.all_gather_into_tensor(
                        gathered_c.view(BHg, N, d)[c * n:(c + 1) * n], oc.view(rc, N, d),
                        async_op=True))
                for w_ in works:
                    w_.wait()

            for _ in range(2):
                step_overlap()
            clock.sync()
            tc, _, _ = _timed_region(torch, clock, dist, world, step_overlap, args.steps)
            result["end_to_end"] = {
                "what": f"forward + all-gather of O, the rank's rows in {chunks} chunks, each "
                        "chunk's gather overlapping the next chunk's forward, per step",
                "chunks": chunks,
                "ms_per_step": round(tc * 1e3 / args.steps, 4),
                "tflops": _sig(total_flops / tc / 1e12),
                "gathered_bytes_per_rank": int(obytes * world),
            }
            result["end_to_end_serial"] = serial
            gathered = gathered_c
    return result, (gathered if gathered is not None else o), (q, k, v)


def _cpu_cores():
    """Cores this process may use: the affinity mask, capped by a cgroup CPU quota when
    one is set (the GPU boxes show the whole machine in the mask)."""
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    quota = None
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = int(q) / int(p)
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / p
        except (OSError, ValueError):
            pass
    cores = avail if quota is None else max(1, min(avail, int(quota + 0.5)))
    return cores, avail, quota


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def cpu_baseline(shape, seconds=12.0):
    """Time the C oracle on a bounded sample of (b,h) heads at full N and d, on every
    core this process may use."""
    import numpy as np
    from oracle import cref
    B, H, N, d = shape
    threads, avail, quota = _cpu_cores()
    rng = np.random.default_rng(0)
    one = [rng.standard_normal((1, N, d)).astype(np.float32) for _ in range(3)]
    t0 = time.perf_counter()
    cref.attn_fwd(*one, causal=False, nthreads=threads)
    t_one = time.perf_counter() - t0
    heads = max(threads, min(B * H, int(seconds / max(t_one, 1e-6))))
    heads = max(1, (heads // threads) * threads)
    qkv = [rng.standard_normal((heads, N, d)).astype(np.float32) for _ in range(3)]
    reps, dt = 0, 0.0
    t0 = time.perf_counter()
    while dt < seconds:  # whole passes over the sample until ~`seconds` of CPU work
        cref.attn_fwd(*qkv, causal=False, nthreads=threads)
        reps += 1
        dt = time.perf_counter() - t0
    flops = fwd_flops(1, heads, N, d) * reps
    return {
        "value": round(flops / dt / 1e12, 6),
        "unit": "TFLOP/s",
        "cores": threads,
        "cores_in_affinity_mask": avail,
        "cgroup_cpu_quota": quota,
        "cpu_model": _cpu_model(),
        "kind": "port",
        "sample": f"{reps} pass(es) over {heads} of {B*H} (b,h) heads at N={N}, d={d}, fp32 "
                  f"(C restatement of the reference fast_ops attention, oracle/attn_ref.c, "
                  f"OpenMP over (head,row) on {threads} threads), {dt:.1f} s",
        "seconds": round(dt, 2),
    }


def timed_parity(torch, _hip, q, k, v, o, causal, heads=8):
    """Part of the CPU leg (rank 0, N = 1): the max-abs error of the output the timed region
    wrote (o: the fp32-output forward by default) and of the other output form of the same
    forward (bf16 O), on `heads` heads spread over B*H (C3: all 128), against the C
    restatement of the reference's CPU attention (oracle/attn_ref.c, fp32) fed the same bf16
    inputs. north_star's bound is a flat 1e-3."""
    import numpy as np
    from oracle import cref
    B, H, N, d = q.shape
    BH = B * H
    pick = sorted({int(round(i * (BH - 1) / max(heads - 1, 1))) for i in range(heads)})
    other_dtype = torch.bfloat16 if o.dtype == torch.float32 else torch.float32
    o2 = torch.empty(q.shape, dtype=other_dtype, device=q.device)
    _hip.flash_fwd(q, k, v, causal, out=o2)
    torch.cuda.synchronize()
    flat = lambda t: t.reshape(BH, N, d)  # noqa: E731
    idx = torch.tensor(pick, device=q.device)
    qs, ks, vs = (flat(t).index_select(0, idx).float().cpu().numpy() for t in (q, k, v))
    ref, _, _ = cref.attn_fwd(qs, ks, vs, causal=causal, nthreads=_cpu_cores()[0])
    err = float(np.abs(flat(o).index_select(0, idx).float().cpu().numpy() - ref).max())
    err2 = float(np.abs(flat(o2).index_select(0, idx).float().cpu().numpy() - ref).max())
    del o2
    name = lambda t: "fp32 O" if t == torch.float32 else "bf16 O"  # noqa: E731
    return {"bound": 1e-3, "heads_checked": len(pick), "of_heads": BH,
            "reference": "oracle/attn_ref.c fp32 on the same bf16 Q/K/V (C restatement of fast_ops attention)",
            "timed_form": name(o.dtype), "timed_max_abs": err, "timed_within_bound": err <= 1e-3,
            "other_form": name(other_dtype), "other_max_abs": err2, "other_within_bound": err2 <= 1e-3}


def load_pmc_traffic(tag):
    """HBM bytes per launch (and MFMA-busy fraction, effective clock) of the forward kernel
    from the committed rocprofv3 PMC capture (profiles/pmc_<tag>.json)."""
    path = os.path.join(ROOT, "profiles", f"pmc_{tag}.json")
    if not os.path.exists(path):
        return None, None, {}
    try:
        with open(path) as f:
            j = json.load(f)
        extra = {k: j[k] for k in ("mfma_busy_frac", "effective_clock_ghz") if k in j}
        return j.get("hbm_bytes_per_launch"), os.path.relpath(path, ROOT), extra
    except Exception:
        return None, None, {}


DUMP_BUDGET_BYTES = 60 * 1000 * 1000  # all of --dump-outputs' files together stay under 64 MB


def dump_outputs(torch, out_dir, o, m=None, l=None):
    """--dump-outputs: the last timed step's O [.., N, d] (and m, l [.., N] when given) as
    float32 out_dir/<name>.npy. When they do not fit the budget whole, every array keeps the
    same sorted sample of its flattened (b,h,row) rows, drawn once from a fixed seed."""
    import numpy as np
    d = o.shape[-1]
    rows = o.numel() // d
    stats = [(n_, t) for n_, t in (("m", m), ("l", l)) if t is not None]
    assert all(t.numel() == rows for _, t in stats)
    keep = min(rows, DUMP_BUDGET_BYTES // (4 * (d + len(stats))))
    idx = None
    if keep < rows:
        g = torch.Generator(device="cpu")
        g.manual_seed(0)
        idx = torch.randperm(rows, generator=g)[:keep].sort().values.to(o.device)
    os.makedirs(out_dir, exist_ok=True)
    for name, t in [("O", o.reshape(rows, d))] + [(n_, t.reshape(rows)) for n_, t in stats]:
        a = t if idx is None else t.index_select(0, idx)
        np.save(os.path.join(out_dir, f"{name}.npy"), a.float().cpu().numpy())


def extra_legs(torch, _hip, time_fn):
    """Single-GPU side legs (rank 0, N = 1): causal forward, bf16 backward, config 2 fp32,
    and the config-4 per-GPU shard at 8 GPUs."""
    extra = {}
    B, H, N, d = WORKLOAD
    q, k, v, do = (make_shard(torch, WORKLOAD, 0, torch.bfloat16, s, "cuda") for s in (1, 2, 3, 4))
    o = torch.empty_like(q)
    m = torch.empty((B, H, N), dtype=torch.float32, device="cuda")
    l = torch.empty_like(m)
    extra["fwd_causal_tflops"] = round(fwd_flops(B, H, N, d, True) / (time_fn(
        lambda: _hip.flash_fwd(q, k, v, True, out=o, m=m, l=l), 20, 3) * 1e-3) / 1e12, 2)
    # the bf16-output form of the headline (O rounded to bf16: half an ulp of |O| up to 0.5 is
    # already 9.8e-4, so it cannot meet north_star's flat 1e-3 on every head)
    extra["fwd_bf16out_tflops"] = round(fwd_flops(B, H, N, d) / (time_fn(
        lambda: _hip.flash_fwd(q, k, v, False, out=o, m=m, l=l), 20, 3) * 1e-3) / 1e12, 2)
    # the fp32-output forms (MT_BF16_F32OUT: bf16 Q/K/V, O without its final bf16 rounding),
    # the configuration that meets north_star's flat 1e-3 on every C3 head, causal included
    o32 = torch.empty(q.shape, dtype=torch.float32, device="cuda")
    for c_, key in ((False, "fwd_f32out_tflops"), (True, "fwd_causal_f32out_tflops")):
        extra[key] = round(fwd_flops(B, H, N, d, c_) / (time_fn(
            lambda: _hip.flash_fwd(q, k, v, c_, out=o32, m=m, l=l), 20, 3) * 1e-3) / 1e12, 2)
    del o32
    # backward (bf16), FA-2 flop convention 2.5 x fwd
    _hip.flash_fwd(q, k, v, False, out=o, m=m, l=l)
    ws = torch.empty(_hip.lib().mt_flash_attn_bwd_workspace_bytes(B, H, N, d) // 4,
                     dtype=torch.float32, device="cuda")
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    bwd_ms = time_fn(lambda: _hip.flash_bwd(q, k, v, o, do, m, l, False, dq=dq, dk=dk, dv=dv,
                                            workspace=ws), 10, 2)
    extra["bwd_ms"] = round(bwd_ms, 4)
    extra["bwd_tflops"] = round(2.5 * fwd_flops(B, H, N, d) / (bwd_ms * 1e-3) / 1e12, 2)
    _hip.flash_fwd(q, k, v, True, out=o, m=m, l=l)
    bwdc_ms = time_fn(lambda: _hip.flash_bwd(q, k, v, o, do, m, l, True, dq=dq, dk=dk, dv=dv,
                                             workspace=ws), 10, 2)
    extra["bwd_causal_ms"] = round(bwdc_ms, 4)
    extra["bwd_causal_tflops"] = round(2.5 * fwd_flops(B, H, N, d, True) / (bwdc_ms * 1e-3) / 1e12, 2)
    del q, k, v, do, o, m, l, dq, dk, dv, ws
    # the d = 128 bf16 backward (config 4's head dim) at (8,16,4096,128), FA-2 convention
    s128 = (8, 16, 4096, 128)
    q, k, v, do = (make_shard(torch, s128, 0, torch.bfloat16, s, "cuda") for s in (12, 13, 14, 15))
    o = torch.empty_like(q)
    m = torch.empty(s128[:3], dtype=torch.float32, device="cuda")
    l = torch.empty_like(m)
    ws = torch.empty(_hip.lib().mt_flash_attn_bwd_workspace_bytes(*s128) // 4 + 64, dtype=torch.float32,
                     device="cuda")
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    for c_, tag in ((False, ""), (True, "_causal")):
        _hip.flash_fwd(q, k, v, c_, out=o, m=m, l=l)
        ms_ = time_fn(lambda: _hip.flash_bwd(q, k, v, o, do, m, l, c_, dq=dq, dk=dk, dv=dv, workspace=ws), 5, 2)
        extra[f"bwd_d128{tag}_ms"] = round(ms_, 4)
        extra[f"bwd_d128{tag}_tflops"] = round(2.5 * fwd_flops(*s128, c_) / (ms_ * 1e-3) / 1e12, 2)
    del q, k, v, do, o, m, l, dq, dk, dv, ws
    # config 2: (8,16,1024,64) fp32 forward, and the fp32 backward minitorch's MHA runs
    # (the reference's own precision)
    c2 = (8, 16, 1024, 64)
    q2, k2, v2, do2 = (make_shard(torch, c2, 0, torch.float32, s, "cuda") for s in (5, 6, 7, 11))
    o2 = torch.empty_like(q2)
    m2 = torch.empty(c2[:3], dtype=torch.float32, device="cuda")
    l2 = torch.empty_like(m2)
    c2_ms = time_fn(lambda: _hip.flash_fwd(q2, k2, v2, False, out=o2, m=m2, l=l2), 20, 3)
    extra["c2_fp32_fwd_ms"] = round(c2_ms, 4)
    extra["c2_fp32_fwd_tflops"] = round(fwd_flops(*c2) / (c2_ms * 1e-3) / 1e12, 2)
    extra["c2_fp32_frac_of_f32_peak"] = round(extra["c2_fp32_fwd_tflops"] / PEAK_F32_TFLOPS, 4)
    # since round 6 the fp32 products run on the bf16 MFMA, every operand in three bf16 pieces
    # (six bf16 products per fp32 product, fp32 accuracy), so the fp32-peak fraction can pass 1;
    # the bf16 pipe's own fraction is 6 x the flops over the dense bf16 peak
    extra["c2_fp32_method"] = "x3: fp32 products as six bf16 MFMA products (DESIGN.md §3)"
    extra["c2_fp32_bf16_pipe_frac"] = round(6 * extra["c2_fp32_fwd_tflops"] / PEAK_BF16_TFLOPS, 4)
    ws2 = torch.empty(_hip.lib().mt_flash_attn_bwd_workspace_bytes(*c2) // 4, dtype=torch.float32,
                      device="cuda")
    g2 = [torch.empty_like(q2) for _ in range(3)]
    c2b_ms = time_fn(lambda: _hip.flash_bwd(q2, k2, v2, o2, do2, m2, l2, False, dq=g2[0], dk=g2[1],
                                            dv=g2[2], workspace=ws2), 10, 2)
    extra["c2_fp32_bwd_ms"] = round(c2b_ms, 4)
    extra["c2_fp32_bwd_tflops"] = round(2.5 * fwd_flops(*c2) / (c2b_ms * 1e-3) / 1e12, 2)
    # the causal fp32 pair minitorch's decoder self-attention runs (flash_attention_causal_*)
    c2c_ms = time_fn(lambda: _hip.flash_fwd(q2, k2, v2, True, out=o2, m=m2, l=l2), 20, 3)
    extra["c2_fp32_causal_fwd_ms"] = round(c2c_ms, 4)
    c2cb_ms = time_fn(lambda: _hip.flash_bwd(q2, k2, v2, o2, do2, m2, l2, True, dq=g2[0], dk=g2[1],
                                             dv=g2[2], workspace=ws2), 10, 2)
    extra["c2_fp32_causal_bwd_ms"] = round(c2cb_ms, 4)
    del q2, k2, v2, do2, o2, m2, l2, ws2, g2
    # config 4's per-GPU shard at 8 GPUs: (8,16,16384,128) bf16 forward (1/8 of B = 64)
    c4 = (8, 16, 16384, 128)
    q4, k4, v4 = (make_shard(torch, c4, 0, torch.bfloat16, s, "cuda") for s in (8, 9, 10))
    o4 = torch.empty_like(q4)
    m4 = torch.empty(c4[:3], dtype=torch.float32, device="cuda")
    l4 = torch.empty_like(m4)
    c4_ms = time_fn(lambda: _hip.flash_fwd(q4, k4, v4, False, out=o4, m=m4, l=l4), 5, 1)
    extra["c4_shard_bf16_fwd_ms"] = round(c4_ms, 3)
    extra["c4_shard_bf16_fwd_tflops"] = round(fwd_flops(*c4) / (c4_ms * 1e-3) / 1e12, 2)
    del q4, k4, v4, o4, m4, l4
    try:  # a side leg: a failure here is reported, it does not void the headline line
        extra.update(c5_step_leg(torch))
    except Exception as e:  # noqa: BLE001
        extra["c5_error"] = repr(e)[:200]
    return extra


def synthetic_mt_batch(rng, B, T, V, pad_id=0):
    """A right-padded token batch shaped like the reference's collate_fn output
    (reference project/run_machine_translation.py:119-141): each row is source tokens + target tokens
    + padding, input_ids = tokens[:, :-1], labels = tokens[:, 1:], label_token_weights = the
    target mask shifted by one; kv_len = the valid input tokens per row."""
    import numpy as np
    total = rng.integers(T // 2, T + 2, B)  # row length in tokens of T + 1 columns
    src = np.maximum(1, total // 2)
    tok = rng.integers(1, V, (B, T + 1))
    tgt_mask = np.zeros((B, T + 1), np.float32)
    for b in range(B):
        tok[b, total[b]:] = pad_id
        tgt_mask[b, src[b]:total[b]] = 1.0
    return {"input_ids": tok[:, :-1].astype(np.float32), "labels": tok[:, 1:].astype(np.float32),
            "label_token_weights": tgt_mask[:, 1:], "kv_len": np.minimum(total, T).astype(np.int64)}


def c5_step_leg(torch, steps: int = 20) -> dict:
    """Config 5: one DecoderLM training step (forward, backward, Adam) of the reference's
    machine-translation setup (project/run_machine_translation.py:397-407: vocab 10000,
    n_embd 256, 8 heads, batch 128, seq 39) on the HIP backend with fused LayerNorm + softmax
    and flash attention, random init, on a synthetic right-padded batch with the reference's
    weighted loss (loss_fn, :164-192: softmax_loss · label_token_weights, summed, over the
    weight sum); the flash path masks the padding keys (kv_len). Host-bound in minitorch's
    Python autodiff; reported beside the kernels, not the headline."""
    import numpy as np
    import minitorch
    B, T, V, E, H = 128, 39, 10000, 256, 8
    backend = minitorch.TensorBackend(minitorch.HipKernelOps)
    rng = np.random.default_rng(0)
    lm = minitorch.DecoderLM(n_vocab=V, n_embd=E, n_head=H, n_positions=40, p_dropout=0.1,
                             backend=backend, use_fused_kernel=True, use_flash_attention=True)
    opt = minitorch.Adam(lm.parameters(), lr=1e-4)
    batch = synthetic_mt_batch(rng, B, T, V)
    x = minitorch.tensor_from_numpy(batch["input_ids"], backend)
    y = minitorch.tensor_from_numpy(batch["labels"].reshape(-1), backend)
    w = minitorch.tensor_from_numpy(batch["label_token_weights"].reshape(-1), backend)
    kv = batch["kv_len"]

    def step():
        opt.zero_grad()
        loss = (minitorch.softmax_loss(lm(x, kv_len=kv).view(B * T, V), y) * w).sum() / w.sum()
        loss.backward()
        opt.step()
        return loss

    import gc
    # warm-up: the host-side caches (shape / stride memos, ctypes argument arrays), the
    # allocator's pools and rocBLAS's kernel selection settle over the first few steps
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    # the model, optimizer state and batch live for the whole run: freeze them out of the
    # cyclic collector (gc.freeze, what a long training loop does) so its passes scan only the
    # step's own garbage (scripts/mt_step_bench.py gc_variants_ms: ≈ 1 ms per step)
    gc.collect()
    gc.freeze()
    try:
        t0, h0 = time.perf_counter(), time.thread_time()
        for _ in range(steps):
            loss = step()
        host_ms = (time.thread_time() - h0) / steps * 1e3
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
    finally:
        gc.unfreeze()
    cores, _, quota = _cpu_cores()
    out = {"c5_step_ms": round(ms, 2), "c5_tokens_per_s": round(B * T / ms * 1e3, 1),
           "c5_loss": round(float(loss.item()), 4),
           # the host thread's CPU time per step (minitorch's Python autodiff and the launches):
           # when it is close to c5_step_ms the step is host-bound
           "c5_host_ms": round(host_ms, 2), "c5_host_cpu_quota": quota, "c5_host_cores": cores,
           "c5_batch": "right-padded synthetic tokens, weighted loss, kv_len key padding"}
    try:  # the GPU's busy time per step: the kernels' own durations (torch.profiler)
        out.update(_gpu_busy_ms(torch, step, 3, "c5"))
    except Exception as e:  # noqa: BLE001
        out["c5_gpu_ms_error"] = repr(e)[:160]
    try:  # the same step captured once as a hipGraph and replayed (minitorch/graphs.py):
        # fresh dropout seeds and Adam step size per replay, bitwise the eager step's results
        # (tests/test_graphs_gpu.py); the host only refills the per-step slots and launches
        from minitorch.graphs import StepGraph
        g = StepGraph(step, warmup=2)
        g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = g.replay()
        torch.cuda.synchronize()
        gms = (time.perf_counter() - t0) / steps * 1e3
        out.update({"c5_graph_step_ms": round(gms, 2), "c5_graph_tokens_per_s": round(B * T / gms * 1e3, 1),
                    "c5_graph_loss": round(float(loss.item()), 4)})
    except Exception as e:  # noqa: BLE001
        out["c5_graph_error"] = repr(e)[:200]
    return out


def _gpu_busy_ms(torch, fn, steps, tag):
    """Sum of the device kernels' durations per call of fn (torch.profiler's device activity:
    every HIP kernel of the process, the library's included), and their count per call."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    tot_us, n = 0.0, 0
    for e in prof.key_averages():
        us = getattr(e, "self_device_time_total", None)
        if us is None:
            us = getattr(e, "self_cuda_time_total", 0.0)
        if us and us > 0:
            tot_us += us
            n += e.count
    return {f"{tag}_gpu_ms": round(tot_us / steps / 1e3, 3), f"{tag}_gpu_kernels_per_step": round(n / steps, 1)}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # default: ~1 s of timed device work at C3 (0.5 ms per step)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", choices=sorted(CONFIGS), default="c3")
    ap.add_argument("--split", choices=("strong", "weak"), default="strong")
    ap.add_argument("--causal", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the side legs (N = 1): extra (causal, bwd, "
                         "fp32, config 4 and 5), the CPU baseline and the parity check")
    ap.add_argument("--no-cpu", action="store_true", help="--full without the CPU baseline leg")
    ap.add_argument("--no-extra", action="store_true", help="--full without the extra (bwd, fp32) legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy (float32, at "
                         "most 64 MB: a fixed seeded sample of rows when larger)")
    ap.add_argument("--policy", type=int, default=0, help="kernel policy (0 default)")
    ap.add_argument("--out", choices=("f32", "bf16"), default="f32",
                    help="the timed forward's O: f32 (default, MT_BF16_F32OUT: within north_star's "
                         "flat 1e-3) or bf16")
    ap.add_argument("--chunks", type=int, default=None,
                    help="end-to-end leg: chunks of the rank's rows whose all-gather overlaps "
                         "the next chunk's forward (default: minitorch.shard.occupancy_chunks, "
                         "up to 4 while each chunk keeps a workgroup per CU; 1 = serial)")
    ap.add_argument("--shape", type=int, nargs=4, default=None, help=argparse.SUPPRESS)
    return ap.parse_args(argv)


def main():
    args = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch N processes with "
              f"torch.distributed.run --nproc-per-node N and pass --gpus N", file=sys.stderr)
        sys.exit(2)

    import torch
    import torch.distributed as dist
    from minitorch import _hip

    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    _hip.set_policy(args.policy)

    # m / l outputs are part of the forward's contract: keep them written every step
    ml = {}

    def attn_ml(q, k, v, causal, out):
        key = tuple(q.shape[:3])
        if key not in ml:
            ml[key] = (torch.empty(key, dtype=torch.float32, device=q.device),
                       torch.empty(key, dtype=torch.float32, device=q.device))
        m, l = ml[key]
        _hip.flash_fwd(q, k, v, causal, out=out, m=m, l=l)

    result, o_timed, qkv = run(args, attn_ml, torch, dist, world, rank, f"cuda:{local}", torch.bfloat16,
                               esize=2, out_esize=4 if args.out == "f32" else 2)

    if rank == 0 and args.dump_outputs:
        # N > 1: the all-gathered O (m and l stay per rank)
        m_l = ml[tuple(qkv[0].shape[:3])] if world == 1 else (None, None)
        dump_outputs(torch, args.dump_outputs, o_timed, *m_l)

    if rank == 0 and world == 1 and args.full and not args.no_extra and args.config == "c3":
        clock = Clock(torch, "cuda")

        def time_fn(fn, steps, warmup):
            # warm-up, then a ~0.15 s clock ramp, then at least `steps` calls and ~0.2 s of them
            for _ in range(warmup):
                fn()
            clock.sync()
            t0 = time.perf_counter()
            fn()
            clock.sync()
            one = max(time.perf_counter() - t0, 1e-5)
            for _ in range(int(0.15 / one)):
                fn()
            return clock.span(fn, max(steps, int(0.2 / one)))

        result["extra"] = extra_legs(torch, _hip, time_fn)

    if rank == 0 and world == 1 and args.full and not args.no_cpu:
        cpu = cpu_baseline(CONFIGS[args.config])
        cpu["gpu_over_cpu"] = round(result["value"] / cpu["value"], 1) if cpu["value"] > 0 else None
        result["cpu_baseline"] = cpu
        # the error of what the timed region computed (CPU leg: the oracle as the checker)
        result["parity"] = timed_parity(torch, _hip, *qkv, o_timed, args.causal,
                                        heads=128 if args.config == "c3" else 2)

    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
