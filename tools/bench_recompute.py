#!/usr/bin/env python3
"""Step time and peak memory of the activation-recomputation modes (DiT.enable_recompute) on a bench.py workload.

    python tools/bench_recompute.py --workload c3b --batches 12 --modes none,full,selective --repeat 2
    python tools/bench_recompute.py --workload c4 --batches 2,4 --modes selective
    python tools/bench_recompute.py --workload c3b --batches 2 --modes fwd      # the no_grad forward (sampler's pass)

One JSON line per leg.  A leg is a fresh child process under its own time limit (a leg's allocator state, and its
failure, stay its own); the legs of one batch are alternated mode by mode and the whole round repeated --repeat times,
so that the run-to-run spread is on the page next to every difference.  A leg that fails ends the run.

Before it builds anything a leg predicts its peak from shapes alone -- model.activation_bytes (kept + one block's
transient) + 18 bytes per parameter (fp32 master, bf16 compute copy, fp32 gradient, AdamW m and v) + one more block's
worth of intermediates for the backward's own temporaries -- and is SKIPPED (reported, not tried) when that exceeds
90 % of torch.cuda.mem_get_info()'s free bytes.

--tree DIR times another checkout of the package (mode "none" / "fwd" only when it predates enable_recompute): the
yardstick for "mode none costs nothing" is the parent commit on the same box in the same run.
Timing as bench.py does: warm-up steps, then HIP events between the steps, the median."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("none", "full", "selective", "fwd")
BYTES_PER_PARAM = 18


def predicted_bytes(M, model, B, lat, Lc, mode):
    n_params = sum(p.numel() for p in model.parameters())
    if mode == "fwd":
        a = M.activation_bytes(model, B, lat[1:], Lc, "none")
        # master, compute copy and the gradient arena (allocated with the flat groups); one block's intermediates in flight
        return 10 * n_params + a["per_block"], a, n_params
    a = M.activation_bytes(model, B, lat[1:], Lc, mode)
    one_block = M.activation_bytes(model, B, lat[1:], Lc, "none")["per_block"]
    return BYTES_PER_PARAM * n_params + a["kept"] + a["transient"] + one_block, a, n_params


def leg(args):
    tree = os.path.abspath(args.tree) if args.tree else REPO
    sys.path.insert(0, tree)
    if REPO not in sys.path:
        sys.path.append(REPO)
    import torch
    import bench  # workload table and model init of the flagship benchmark
    from video_diffusion_speedrun_amd import model as M
    from video_diffusion_speedrun_amd.optim import MuAdamW
    from video_diffusion_speedrun_amd.train import get_schedule, train_step

    kw, lat, _, desc = bench.WORKLOADS[args.workload]
    B, mode = args.batch, args.mode
    out = {"tool": "bench_recompute", "workload": args.workload, "B": B, "mode": mode, "round": args.round,
           "tree": os.path.relpath(tree, REPO) if args.tree else "."}
    has_api = hasattr(M, "activation_bytes")
    if not has_api and mode in ("full", "selective"):
        raise SystemExit(f"--tree {args.tree} has no enable_recompute: only modes none / fwd can be timed there")
    device = torch.device("cuda", 0)
    free, total = torch.cuda.mem_get_info(device)
    if has_api:
        with torch.device("meta"):
            shell = M.DiT(in_channels=16, patch_size=2, cross_attn_input_size=bench.CC, residual_v=True,
                          train_bias_and_rms=False, **kw)
        pred, a, n_params = predicted_bytes(M, shell, B, lat, bench.LC, mode)
        out.update(predicted_bytes=pred, kept_bytes=a["kept"], transient_bytes=a["transient"], params=n_params,
                   free_bytes=free)
        if pred > 0.9 * free:
            out.update(skipped=True, reason=f"predicted {pred / 1e9:.1f} GB > 90 % of the {free / 1e9:.1f} GB free")
            print(json.dumps(out), flush=True)
            return
    model = bench.build_model(kw, device, seed=1234)
    if mode in ("full", "selective"):
        model.enable_recompute(mode)
    gen = torch.Generator(device=device).manual_seed(1234)
    torch.manual_seed(1234)
    bf16 = torch.bfloat16
    batch = {"latent": torch.randn(B, *lat, device=device, generator=gen).to(bf16),
             "context": torch.randn(B, bench.LC, bench.CC, device=device, generator=gen).to(bf16), "prompt": [""] * B}
    if mode == "fwd":
        t = torch.rand(B, device=device, generator=gen).to(bf16)

        def one_step():
            with torch.no_grad():
                return model(batch["latent"], batch["context"], t, rope_start=(1, 2, 3))
    else:
        groups, _ = model.get_mup_setup(1e-4, 0.1, ["patch_proj", "context_kv", "positional_embedding"])
        opt = MuAdamW(groups, betas=(0.95, 0.99))
        sched = get_schedule(opt, "cosine", 20, 10000)

        def one_step():
            return train_step(model, opt, sched, batch, device, generator=gen)
    for _ in range(args.warmup):
        r = one_step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    marks[0].record()
    for i in range(args.steps):
        r = one_step()
        marks[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    out.update(ms_per_step_median=(ms[(len(ms) - 1) // 2] + ms[len(ms) // 2]) / 2, ms_min=ms[0], ms_max=ms[-1],
               steps=args.steps, warmup=args.warmup, max_memory_allocated=torch.cuda.max_memory_allocated(),
               max_memory_reserved=torch.cuda.max_memory_reserved(),
               loss=float(r.detach()) if mode != "fwd" else None, device=torch.cuda.get_device_name(0))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", default="c3b")
    ap.add_argument("--batches", default="", help="comma-separated per-GPU batches (default: the workload's own)")
    ap.add_argument("--modes", default="none,full,selective", help="comma-separated, of " + ", ".join(MODES))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=1, help="rounds over the alternated legs")
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds one leg may take")
    ap.add_argument("--tree", default="", help="import the package from this checkout instead of the one the tool is in")
    ap.add_argument("--also-tree", default="", help="additionally time mode none (and fwd, if asked for) of this checkout "
                                                    "in every round, beside the tool's own")
    ap.add_argument("--out", default="", help="append the JSON lines to this file too")
    # one leg (what the children run)
    ap.add_argument("--leg", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--batch", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--mode", default="none", help=argparse.SUPPRESS)
    ap.add_argument("--round", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    sys.path.insert(0, REPO)
    import bench
    if args.workload not in bench.WORKLOADS:
        raise SystemExit(f"unknown workload {args.workload!r}: one of {sorted(bench.WORKLOADS)}")
    modes = [m for m in args.modes.split(",") if m]
    for m in modes:
        if m not in MODES:
            raise SystemExit(f"unknown mode {m!r}: one of {MODES}")
    batches = [int(b) for b in args.batches.split(",") if b] or [bench.WORKLOADS[args.workload][2]]
    legs = []
    for rnd in range(args.repeat):
        for B in batches:
            for m in modes:
                if args.also_tree and m in ("none", "fwd"):
                    legs.append((rnd, B, m, args.also_tree))
                legs.append((rnd, B, m, args.tree))
    for rnd, B, m, tree in legs:
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg",
               "--workload", args.workload, "--batch", str(B), "--mode", m, "--round", str(rnd),
               "--steps", str(args.steps), "--warmup", str(args.warmup)]
        if tree:
            cmd += ["--tree", tree]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=REPO)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if args.out and p.stdout:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(p.stdout)
        if p.returncode != 0:  # a failed leg ends the run: nothing more is started on the GPU
            raise SystemExit(f"bench_recompute: leg (B={B}, mode={m}, tree={tree or '.'}) exited with {p.returncode}; stopping")


if __name__ == "__main__":
    main()
