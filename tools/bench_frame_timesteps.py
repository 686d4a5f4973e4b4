"""Per-frame timesteps at the C3b shape (DiT-XL/2, latents [12,16,16,64,64], pt = 2: t = 8 token-frames, G = 9 modulation
groups per sample, B*G = 108 modulation rows, L = 8208 rows per sample), legs alternated inside one process:

  step            one train step with timesteps [B]     (train.train_step)
  step_frames     one train step with timesteps [B, 8]  (frame_mode="independent")
  and per kernel family, per-sample against grouped, at B*L = 98496 rows, D = 1152:
  norm_fwd / norm_fwd_grouped          vds_rmsnorm_mod_fwd / _grouped
  norm_bwd / norm_bwd_grouped          vds_rmsnorm_mod_bwd / _grouped (with a residual gradient)
  gate_bwd / gate_bwd_grouped          vds_gate_bwd / _grouped
  gate_res_k1152 / _grouped / _rows    the attn_proj / cross_proj GEMM with the GATE_RES epilogue: per sample (lean
                                       epilogue), grouped (per-row epilogue, [B*G] gate rows), and rows_per_batch = 1 with an
                                       expanded [B*L, D] fp32 gate table (the per-row epilogue's other caller)
  gate_res_k4608 / _grouped            the mlp.2 GEMM
Kernel legs: HIP events around ITERS calls per sample, median over ROUNDS samples per leg.  Step legs: after two warm-up
steps each, STEPS samples of ONE step each (HIP events around the step), median.  One JSON line at the end, which records
rounds, iters and steps.  STEPS=0 skips the two step legs (kernels only); KERNELS=0 skips the kernel legs."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from video_diffusion_speedrun_amd import ops  # noqa: E402
from video_diffusion_speedrun_amd._lib import EPI_GATE_RES, VDS_NT  # noqa: E402

bf16, f32 = torch.bfloat16, torch.float32
B = int(os.environ.get("B", 12))
ROUNDS, ITERS, WARM = int(os.environ.get("ROUNDS", 7)), int(os.environ.get("ITERS", 5)), 3
STEPS, KERNELS = int(os.environ.get("STEPS", 4)), int(os.environ.get("KERNELS", 1))
dev = "cuda"
kw, latent_shape = bench.WORKLOADS["c3b"][0], bench.WORKLOADS["c3b"][1]
D, pt = kw["hidden_size"], kw["time_patch_size"]
t = latent_shape[1] // pt
L = 16 + t * (latent_shape[2] // 2) * (latent_shape[3] // 2)
G, grp = 1 + t, (16, t)
res = {"B": B, "L": L, "D": D, "t": t, "G": G, "rounds": ROUNDS, "iters": ITERS, "steps": STEPS, "step_warmup": 2}


def sample(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def report(times):
    for leg, xs in times.items():
        med = statistics.median(xs)
        res[f"{leg}_ms"] = round(med, 4)
        res[f"{leg}_min_max_ms"] = [round(min(xs), 4), round(max(xs), 4)]
        print(f"{leg:24s}: median {med:10.4f} ms  (min {min(xs):.4f}, max {max(xs):.4f})", flush=True)


if KERNELS:
    g = torch.Generator(device=dev).manual_seed(0)
    rows = B * L
    x, dy, dres, y = (torch.randn(rows, D, device=dev, generator=g).to(bf16) for _ in range(4))
    mod_b = torch.randn(B, 9 * D, device=dev, generator=g) * 0.5
    mod_g = torch.randn(B * G, 9 * D, device=dev, generator=g) * 0.5
    dmod_b, dmod_g = torch.zeros_like(mod_b), torch.zeros_like(mod_g)
    _, rstd = ops.rmsnorm_mod_fwd(x, None, mod_b, 0, D, B, L)
    W1 = (torch.randn(D, D, device=dev, generator=g) / 34).to(bf16)
    W4 = (torch.randn(D, 4 * D, device=dev, generator=g) / 68).to(bf16)
    a4 = torch.randn(rows, 4 * D, device=dev, generator=g).to(bf16)
    gidx = torch.tensor([ops.mod_group_of(l, *grp) for l in range(L)], device=dev)
    mrow = torch.cat([b * G + gidx for b in range(B)])
    expanded = mod_g[mrow, 2 * D:3 * D].contiguous()  # [B*L, D] fp32: 454 MB at B = 12
    yo, xo = torch.empty(rows, D, dtype=bf16, device=dev), torch.empty(rows, D, dtype=bf16, device=dev)

    def gemm_rows():
        ops.gemm(VDS_NT, EPI_GATE_RES, rows, D, D, x, D, W1, D, yo, D, xo, D, aux=dres, ldaux=D, gate=expanded, ldgate=D,
                 rows_per_batch=1)

    LEGS = {
        "norm_fwd": lambda: ops.rmsnorm_mod_fwd(x, None, mod_b, 0, D, B, L),
        "norm_fwd_grouped": lambda: ops.rmsnorm_mod_fwd_grouped(x, None, mod_g, 0, D, B, L, grp),
        "norm_bwd": lambda: ops.rmsnorm_mod_bwd(dy, x, None, mod_b, 0, D, rstd, dres, dmod_b, None, B, L),
        "norm_bwd_grouped": lambda: ops.rmsnorm_mod_bwd_grouped(dy, x, None, mod_g, 0, D, rstd, dres, dmod_g, None, B, L, grp),
        "gate_bwd": lambda: ops.gate_bwd(dy, y, mod_b, 2 * D, dmod_b, None, B, L),
        "gate_bwd_grouped": lambda: ops.gate_bwd_grouped(dy, y, mod_g, 2 * D, dmod_g, None, B, L, grp),
        "gate_res_k1152": lambda: ops.linear_fwd_gate_res(x, W1, None, mod_b, 2 * D, dres, L),
        "gate_res_k1152_grouped": lambda: ops.linear_fwd_gate_res_grouped(x, W1, None, mod_g, 2 * D, dres, L, grp),
        "gate_res_k1152_rows": gemm_rows,
        "gate_res_k4608": lambda: ops.linear_fwd_gate_res(a4, W4, None, mod_b, 8 * D, dres, L),
        "gate_res_k4608_grouped": lambda: ops.linear_fwd_gate_res_grouped(a4, W4, None, mod_g, 8 * D, dres, L, grp),
    }
    for fn in LEGS.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    times = {leg: [] for leg in LEGS}
    for _ in range(ROUNDS):  # the legs alternate, so that clock and neighbour drift hits all of them alike
        for leg, fn in LEGS.items():
            times[leg].append(sample(fn, ITERS))
    report(times)
    del x, dy, dres, y, a4, expanded, yo, xo, LEGS
    torch.cuda.empty_cache()

if STEPS:
    from video_diffusion_speedrun_amd.optim import MuAdamW
    from video_diffusion_speedrun_amd.train import get_schedule, train_step
    model = bench.build_model(kw, dev, seed=1234)
    groups, _ = model.get_mup_setup(1e-4, 0.1, ["patch_proj", "context_kv", "positional_embedding"])
    opt = MuAdamW(groups, betas=(0.95, 0.99))
    sched = get_schedule(opt, "cosine", 20, 10000)
    gen = torch.Generator(device=dev).manual_seed(1234)
    torch.manual_seed(1234)
    batch = {"latent": torch.randn(B, *latent_shape, device=dev, generator=gen).to(bf16),
             "context": torch.randn(B, bench.LC, bench.CC, device=dev, generator=gen).to(bf16), "prompt": [""] * B}
    LEGS = {"step": lambda: train_step(model, opt, sched, batch, dev, generator=gen),
            "step_frames": lambda: train_step(model, opt, sched, batch, dev, generator=gen, frame_mode="independent")}
    for fn in LEGS.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {leg: [] for leg in LEGS}
    for _ in range(STEPS):
        for leg, fn in LEGS.items():
            times[leg].append(sample(fn, 1))
    report(times)
print(json.dumps(res))
