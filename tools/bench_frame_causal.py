"""Frame-causal self-attention at the C3b shape (DiT-XL/2, latents [12,16,16,64,64], pt = 2: t = 8 token-frames,
L = 8208 rows per sample, 16 heads of 72), legs alternated inside one process:

  attn_fwd / attn_fwd_causal      the self-attention forward as the model calls it (kv_pad_ones = 1, the ones-column
                                  kernels): unmasked and with frames = {16, 8}
  attn_bwd / attn_bwd_causal      the backward (dQ with the folded preprocess, then dK/dV)
  step / step_causal              one C3b train step without / with DiT(frame_causal=True)
(The masked kernels have one form for every {lead, period}: there is no second period to time.)
Kernel legs: HIP events around ITERS calls per sample, median over ROUNDS samples per leg.  Step legs: after two warm-up
steps each, STEPS samples of ONE step each, median.  One JSON line at the end.  STEPS=0 skips the step legs, KERNELS=0 the
kernel legs."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from video_diffusion_speedrun_amd import ops  # noqa: E402

bf16, f32 = torch.bfloat16, torch.float32
B = int(os.environ.get("B", 12))
ROUNDS, ITERS, WARM = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("ITERS", 3)), 2
STEPS, KERNELS = int(os.environ.get("STEPS", 4)), int(os.environ.get("KERNELS", 1))
dev = "cuda"
kw, latent_shape = bench.WORKLOADS["c3b"][0], bench.WORKLOADS["c3b"][1]
D, H, pt = kw["hidden_size"], kw["num_heads"], kw["time_patch_size"]
hd, hdp = D // H, 96
t = latent_shape[1] // pt
L = 16 + t * (latent_shape[2] // 2) * (latent_shape[3] // 2)
res = {"B": B, "H": H, "L": L, "head_dim": hd, "t": t, "rounds": ROUNDS, "iters": ITERS, "steps": STEPS, "step_warmup": 2}


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


def run_legs(legs, warm, rounds, iters):
    for fn in legs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {leg: [] for leg in legs}
    for _ in range(rounds):  # the legs alternate, so that clock and neighbour drift hits all of them alike
        for leg, fn in legs.items():
            times[leg].append(sample(fn, iters))
    report(times)


if KERNELS:
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B * L, 3 * D, device=dev, generator=g).to(bf16)
    cos = torch.ones(L, hd // 2, dtype=f32, device=dev)
    sin = torch.zeros(L, hd // 2, dtype=f32, device=dev)
    q, k, v = ops.qkv_rope_fwd(qkv, cos, sin, None, None, B, L, H, hd, hdp)
    del qkv
    o = torch.empty(B * L, D, dtype=bf16, device=dev)
    do = torch.randn(B * L, D, device=dev, generator=g).to(bf16)
    lse = torch.empty(B, H, L, dtype=f32, device=dev)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    delta = torch.empty(ops.attn_bwd_workspace_floats(B, H, L, L, hd, True), dtype=f32, device=dev)
    ov, dov = ops.heads_view(o, B, L, H, hd), ops.heads_view(do, B, L, H, hd)

    def fwd(frames):
        return lambda: ops.attn_fwd(q[..., :hd], k[..., :hd], v[..., :hd], ov, lse, kv_pad_ones=True, frames=frames)

    def bwd(frames):
        return lambda: ops.attn_bwd(q[..., :hd], k[..., :hd], v[..., :hd], ov, lse, dov, dq[..., :hd], dk[..., :hd],
                                    dv[..., :hd], delta, kv_pad_ones=True, frames=frames)

    # (each backward leg follows a forward with the same mask in the warm-up only: the timing does not depend on o / lse)
    run_legs({"attn_fwd": fwd(None), "attn_fwd_causal": fwd((16, t)), "attn_bwd": bwd(None), "attn_bwd_causal": bwd((16, t))},
             WARM, ROUNDS, ITERS)
    del q, k, v, o, do, dq, dk, dv, delta
    torch.cuda.empty_cache()

if STEPS:
    from video_diffusion_speedrun_amd.optim import MuAdamW
    from video_diffusion_speedrun_amd.train import get_schedule, train_step
    gen = torch.Generator(device=dev).manual_seed(1234)
    torch.manual_seed(1234)
    batch = {"latent": torch.randn(B, *latent_shape, device=dev, generator=gen).to(bf16),
             "context": torch.randn(B, bench.LC, bench.CC, device=dev, generator=gen).to(bf16), "prompt": [""] * B}
    # ONE model (a C3b step peaks near 200 GB): frame_causal adds no parameter, the blocks read their flag at every call
    model = bench.build_model(kw, dev, seed=1234)
    groups, _ = model.get_mup_setup(1e-4, 0.1, ["patch_proj", "context_kv", "positional_embedding"])
    opt = MuAdamW(groups, betas=(0.95, 0.99))
    sched = get_schedule(opt, "cosine", 20, 10000)

    def step(causal):
        def run():
            model.frame_causal = causal
            for blk in model.blocks:
                blk.frame_causal = causal
            train_step(model, opt, sched, batch, dev, generator=gen)
        return run
    legs = {"step": step(False), "step_causal": step(True)}
    run_legs(legs, 2, STEPS, 1)
print(json.dumps(res))
