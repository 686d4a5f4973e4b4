#!/usr/bin/env python3
"""LoRA at a bench.py workload: the low-rank kernels one by one, and the train step with and without adapters.

    python tools/bench_lora.py --workload c3b --ranks 16,64 --out profiles/lora/bench_lora_c3b.jsonl
    python tools/bench_lora.py --kernels-only            # no model is built
    python tools/bench_lora.py --steps-only --ranks 16

Kernels (one JSON line each): every vds_lowrank_* call a DiT block makes at the workload's shape (M = B*L token rows, D
hidden, Lc*B context rows of width Cc), timed with HIP events around single launches, the calls alternated round by
round in ONE process next to rmsnorm_mod_fwd on the same rows; reported are the median microseconds, the algorithmic
bytes (each operand once) and that rate as a fraction of the 8 TB/s HBM3E peak.
Train step (one JSON line per leg and round): three models in the same process, their steps alternated --
    full     every parameter trains (the parent's step)
    frozen   every parameter but the register tokens frozen, no adapters: what skipping the weight gradients saves
    lora     add_lora(rank) with the base frozen
-- median milliseconds over --steps steps after --warmup, and the peak of torch's allocator inside the leg's steps
(the other legs' parameters and optimizer state are resident too; `resident_before` says how much)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_PEAK = 8.0e12


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(line + "\n")


def median(v):
    v = sorted(v)
    return (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2


def kernel_legs(args, torch, bench, ops):
    kw, lat, B0, _ = bench.WORKLOADS[args.workload]
    B = args.batch or B0
    D = kw["hidden_size"]
    L = (lat[1] // kw["time_patch_size"]) * (lat[2] // 2) * (lat[3] // 2) + 16
    M, Mc, Cc = B * L, B * bench.LC, bench.CC
    dev = torch.device("cuda", 0)
    bf16, f32 = torch.bfloat16, torch.float32
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf16)  # noqa: E731
    x, y3, ctx = rnd(M, D), rnd(M, 3 * D), rnd(Mc, Cc)
    mod = torch.randn(B, 9 * D, device=dev, generator=g)
    for r in args.ranks:
        A, Bq = rnd(r, D) * 0.03, rnd(3 * D, r) * 0.03
        Ac = rnd(r, Cc) * 0.03
        u, uc = rnd(M, r), rnd(Mc, r)
        gB, gA = torch.zeros(3 * D, r, device=dev), torch.zeros(r, D, device=dev)
        ws = torch.empty(int(ops._lib.load().vds_lowrank_wgrad_workspace_floats(M, 3 * D, r)), dtype=f32, device=dev)
        # name -> (call, algorithmic bytes: every operand once, y twice)
        legs = {
            "rmsnorm_mod_fwd": (lambda: ops.rmsnorm_mod_fwd(x, None, mod, 0, D, B, L), 4.0 * M * D + 4.0 * M),
            "down x A^T [K=D]": (lambda: ops.lowrank_down(x, A, 1.0, 0, out=u), 2.0 * M * D + 2.0 * M * r + 2.0 * r * D),
            "down dY B [K=3D]": (lambda: ops.lowrank_down(y3, Bq, 1.0, 1, out=u),
                                 2.0 * M * 3 * D + 2.0 * M * r + 2.0 * 3 * D * r),
            "down ctx A^T [K=Cc]": (lambda: ops.lowrank_down(ctx, Ac, 1.0, 0, out=uc),
                                    2.0 * Mc * Cc + 2.0 * Mc * r + 2.0 * r * Cc),
            "up_add y += u B^T [N=3D]": (lambda: ops.lowrank_up_add(u, Bq, y3, 0.001, 0),
                                         4.0 * M * 3 * D + 2.0 * M * r + 2.0 * 3 * D * r),
            "up_add dx += dU A [N=D]": (lambda: ops.lowrank_up_add(u, A, x, 0.001, 1),
                                        4.0 * M * D + 2.0 * M * r + 2.0 * r * D),
            "wgrad dB = dY^T u [N=3D]": (lambda: ops.lowrank_wgrad(y3, u, gB, 1.0, 0, ws=ws),
                                         2.0 * M * 3 * D + 2.0 * M * r + 8.0 * 3 * D * r),
            "wgrad dA = dU^T x [N=D]": (lambda: ops.lowrank_wgrad(x, u, gA, 1.0, 1, ws=ws),
                                        2.0 * M * D + 2.0 * M * r + 8.0 * D * r),
        }
        for fn, _ in legs.values():  # warm-up: code objects, allocator
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(args.kernel_rounds):
            for k, (fn, _) in legs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b) * 1e3)
        for k, (_, nbytes) in legs.items():
            us = median(times[k])
            emit({"tool": "bench_lora", "kind": "kernel", "workload": args.workload, "B": B, "M": M, "D": D, "rank": r,
                  "kernel": k, "us_median": round(us, 2), "us_min": round(min(times[k]), 2), "bytes": nbytes,
                  "hbm_fraction": round(nbytes / (us * 1e-6) / HBM_PEAK, 4), "rounds": args.kernel_rounds,
                  "device": torch.cuda.get_device_name(0)}, args.out)


def step_legs(args, torch, bench):
    from video_diffusion_speedrun_amd.optim import MuAdamW
    from video_diffusion_speedrun_amd.train import get_schedule, train_step
    kw, lat, B0, _ = bench.WORKLOADS[args.workload]
    B = args.batch or B0
    dev = torch.device("cuda", 0)
    bf16 = torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(1234)
    torch.manual_seed(1234)
    batch = {"latent": torch.randn(B, *lat, device=dev, generator=gen).to(bf16),
             "context": torch.randn(B, bench.LC, bench.CC, device=dev, generator=gen).to(bf16), "prompt": [""] * B}
    const = ["patch_proj", "context_kv", "positional_embedding"]
    for r in args.ranks:
        legs = {}
        for name in ("full", "frozen", "lora"):
            m = bench.build_model(kw, dev, seed=1234)
            if name == "frozen":
                for n, p in m.named_parameters():
                    p.requires_grad_(n == "register_tokens")
                m.refresh_paramstatus()
            if name == "lora":
                m.add_lora(rank=r, generator=torch.Generator().manual_seed(1))
                groups, _ = m.get_lora_setup(1e-4)
            else:
                groups, _ = m.get_mup_setup(1e-4, 0.1, const)
            opt = MuAdamW(groups, betas=(0.95, 0.99))
            legs[name] = (m, opt, get_schedule(opt, "cosine", 20, 10000))
        for _ in range(args.warmup):
            for m, opt, sched in legs.values():
                train_step(m, opt, sched, batch, dev, generator=gen)
        torch.cuda.synchronize()
        resident = torch.cuda.memory_allocated()
        times, peaks, losses = {k: [] for k in legs}, {k: 0 for k in legs}, {}
        for _ in range(args.steps):
            for k, (m, opt, sched) in legs.items():
                torch.cuda.reset_peak_memory_stats()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                loss = train_step(m, opt, sched, batch, dev, generator=gen)
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b))
                peaks[k] = max(peaks[k], torch.cuda.max_memory_allocated())
                losses[k] = float(loss.detach())
        for k in legs:
            emit({"tool": "bench_lora", "kind": "step", "workload": args.workload, "B": B, "rank": r, "leg": k,
                  "ms_per_step_median": round(median(times[k]), 2), "ms_min": round(min(times[k]), 2),
                  "ms_max": round(max(times[k]), 2), "steps": args.steps, "warmup": args.warmup,
                  "peak_allocated_in_step": peaks[k], "resident_before": resident, "loss": losses[k],
                  "trainable_params": sum(p.numel() for p in legs[k][0].parameters() if p.requires_grad),
                  "device": torch.cuda.get_device_name(0)}, args.out)
        del legs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", default="c3b")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (default: the workload's own)")
    ap.add_argument("--ranks", default="16,64")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-rounds", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--out", default="", help="append the JSON lines to this file too")
    args = ap.parse_args()
    args.ranks = [int(r) for r in args.ranks.split(",") if r]
    import torch
    import bench
    from video_diffusion_speedrun_amd import ops
    if args.workload not in bench.WORKLOADS:
        raise SystemExit(f"unknown workload {args.workload!r}: one of {sorted(bench.WORKLOADS)}")
    if any(r not in ops.LOWRANK_RANKS for r in args.ranks):
        raise SystemExit(f"--ranks: each of {ops.LOWRANK_RANKS}")
    if not torch.cuda.is_available():
        raise SystemExit("bench_lora measures on the GPU: none found (there is no CPU fallback)")
    if not args.steps_only:
        kernel_legs(args, torch, bench, ops)
    if not args.kernels_only:
        step_legs(args, torch, bench)


if __name__ == "__main__":
    main()
