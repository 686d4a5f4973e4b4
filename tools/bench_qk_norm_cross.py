#!/usr/bin/env python3
"""QK-norm in cross-attention at the C3b shapes: the two head-norm kernels next to rmsnorm_mod_fwd, and the train step of a
qk_norm=True model against a qk_norm="all" model.

    python tools/bench_qk_norm_cross.py --out profiles/qk_norm_cross/c3b_bench.jsonl
    python tools/bench_qk_norm_cross.py --kernels-only          # no model is built
    python tools/bench_qk_norm_cross.py --steps-only

Kernels (one JSON line each): vds_head_rmsnorm_fwd / _bwd on the q rows (M = B L = 98 496 token rows, H = 16, head_dim 72,
contiguous) and on the k columns of the context_kv output (M = B Lc = 6 144 rows, the left half of a [M, 2 D] parent), and
rmsnorm_mod_fwd on the same q rows as the yardstick; HIP events around single launches, the legs alternated round by round
in ONE process; median (min .. max) microseconds, the algorithmic bytes (forward: the rows read and written once;
backward: dy and y read, dy written; rstd once) and that rate as a fraction of the 8 TB/s HBM3E peak.
Train step (one JSON line per leg): the two models in the same process, their steps alternated -- median (min .. max)
milliseconds over --steps steps after --warmup."""
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


def shapes(bench, workload, batch):
    kw, lat, B0, _ = bench.WORKLOADS[workload]
    B = batch or B0
    D, H = kw["hidden_size"], kw["num_heads"]
    L = (lat[1] // kw["time_patch_size"]) * (lat[2] // 2) * (lat[3] // 2) + 16
    return kw, lat, B, D, H, D // H, L


def kernel_legs(args, torch, bench, ops):
    kw, lat, B, D, H, hd, L = shapes(bench, args.workload, args.batch)
    M, Mc = B * L, B * bench.LC
    dev = torch.device("cuda", 0)
    bf16 = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf16)  # noqa: E731
    q, dq, ckv, dckv = rnd(M, D), rnd(M, D), rnd(Mc, 2 * D), rnd(Mc, 2 * D)
    mod = torch.randn(B, 9 * D, device=dev, generator=g)
    # (the forward works in place: normed rows stay normed, so every round does the same work; the backward's y / rstd are
    # one forward's results)
    rq, rk = ops.head_rmsnorm_fwd(q, H, hd), ops.head_rmsnorm_fwd(ckv[:, :D], H, hd)
    legs = {
        "rmsnorm_mod_fwd [q rows]": (lambda: ops.rmsnorm_mod_fwd(q, None, mod, 0, D, B, L), 4.0 * M * D + 4.0 * M),
        "head_rmsnorm_fwd [q rows]": (lambda: ops.head_rmsnorm_fwd(q, H, hd), 4.0 * M * D + 4.0 * M * H),
        "head_rmsnorm_bwd [q rows]": (lambda: ops.head_rmsnorm_bwd(dq, q, rq, H, hd), 6.0 * M * D + 4.0 * M * H),
        "head_rmsnorm_fwd [k columns]": (lambda: ops.head_rmsnorm_fwd(ckv[:, :D], H, hd), 4.0 * Mc * D + 4.0 * Mc * H),
        "head_rmsnorm_bwd [k columns]": (lambda: ops.head_rmsnorm_bwd(dckv[:, :D], ckv[:, :D], rk, H, hd),
                                         6.0 * Mc * D + 4.0 * Mc * H),
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
        emit({"tool": "bench_qk_norm_cross", "kind": "kernel", "workload": args.workload, "B": B, "M_q": M, "M_k": Mc, "H": H,
              "hd": hd, "kernel": k, "us_median": round(us, 2), "us_min": round(min(times[k]), 2),
              "us_max": round(max(times[k]), 2), "bytes": nbytes, "hbm_fraction": round(nbytes / (us * 1e-6) / HBM_PEAK, 4),
              "rounds": args.kernel_rounds, "device": torch.cuda.get_device_name(0)}, args.out)


def step_legs(args, torch, bench):
    from video_diffusion_speedrun_amd.optim import MuAdamW
    from video_diffusion_speedrun_amd.train import get_schedule, train_step
    kw, lat, B, D, H, hd, L = shapes(bench, args.workload, args.batch)
    dev = torch.device("cuda", 0)
    bf16 = torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(1234)
    torch.manual_seed(1234)
    batch = {"latent": torch.randn(B, *lat, device=dev, generator=gen).to(bf16),
             "context": torch.randn(B, bench.LC, bench.CC, device=dev, generator=gen).to(bf16), "prompt": [""] * B}
    const = ["patch_proj", "context_kv", "positional_embedding"]
    legs = {}
    for name, flag in (("qk_norm=True", True), ("qk_norm=all", "all")):
        m = bench.build_model(dict(kw, qk_norm=flag), dev, seed=1234)
        groups, _ = m.get_mup_setup(1e-4, 0.1, const)
        opt = MuAdamW(groups, betas=(0.95, 0.99))
        legs[name] = (m, opt, get_schedule(opt, "cosine", 20, 10000))
    for _ in range(args.warmup):
        for m, opt, sched in legs.values():
            train_step(m, opt, sched, batch, dev, generator=gen)
    torch.cuda.synchronize()
    times, losses = {k: [] for k in legs}, {}
    for _ in range(args.steps):
        for k, (m, opt, sched) in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            loss = train_step(m, opt, sched, batch, dev, generator=gen)
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
            losses[k] = float(loss.detach())
    base = median(times["qk_norm=True"])
    for k in legs:
        emit({"tool": "bench_qk_norm_cross", "kind": "step", "workload": args.workload, "B": B, "leg": k,
              "ms_per_step_median": round(median(times[k]), 2), "ms_min": round(min(times[k]), 2),
              "ms_max": round(max(times[k]), 2), "ms_over_qk_norm_true": round(median(times[k]) - base, 2),
              "steps": args.steps, "warmup": args.warmup, "loss": losses[k], "device": torch.cuda.get_device_name(0)},
             args.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", default="c3b")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (default: the workload's own)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-rounds", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--out", default="", help="append the JSON lines to this file too")
    args = ap.parse_args()
    import torch
    import bench
    from video_diffusion_speedrun_amd import ops
    if args.workload not in bench.WORKLOADS:
        raise SystemExit(f"unknown workload {args.workload!r}: one of {sorted(bench.WORKLOADS)}")
    if not torch.cuda.is_available():
        raise SystemExit("bench_qk_norm_cross measures on the GPU: none found (there is no CPU fallback)")
    if not args.steps_only:
        kernel_legs(args, torch, bench, ops)
    if not args.kernels_only:
        step_legs(args, torch, bench)


if __name__ == "__main__":
    main()
