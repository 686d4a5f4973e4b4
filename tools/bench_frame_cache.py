"""Frame KV cache at the C3b latent (DiT-XL/2 built with frame_causal=True, latents [1,16,16,64,64], pt = 2: t = 8
token-frames of 1024 tokens, 16 registers, L = 8208), legs alternated inside one process:

  rollout1 / rollout1_cached   generate_latents(rollout_frames=1), guided (batch 2), STEPS Euler steps per chunk: 8 chunks x
                               STEPS full-sequence calls against 8 x STEPS calls on 1040 rows + 7 commit calls
  rollout2 / rollout2_cached   rollout_frames=2: 4 chunks, 2064 rows per cached call
  and one kernel family at B = 2, H = 16, head dim 72 in the ones-column layout, Lq = 1040 (one frame + registers):
  attn_past_P / attn_rect_P    vds_attn_fwd_causal_past with P = 1024, 4096, 7168 past rows against the unmasked
                               rectangular vds_attn_fwd at the same Lq, Lk = Lq + P
Kernel legs: HIP events around ITERS calls per sample, median over ROUNDS samples per leg.  Rollout legs: one warm-up run
each, then ROUNDS samples of ONE rollout each (HIP events around it), median.  One JSON line at the end.  ROLLOUT=0 skips
the rollout legs; KERNELS=0 the kernel legs."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from video_diffusion_speedrun_amd import ops, sampling  # noqa: E402
from video_diffusion_speedrun_amd.model import DiT  # noqa: E402

bf16, f32 = torch.bfloat16, torch.float32
ROUNDS, ITERS, WARM = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("ITERS", 10)), 3
STEPS = int(os.environ.get("STEPS", 2))
ROLLOUT, KERNELS = int(os.environ.get("ROLLOUT", 1)), int(os.environ.get("KERNELS", 1))
dev = "cuda"
kw, latent_shape = bench.WORKLOADS["c3b"][0], bench.WORKLOADS["c3b"][1]
res = {"latent": [1, *latent_shape], "rounds": ROUNDS, "iters": ITERS, "steps_per_chunk": STEPS, "cfg_scale": 6.0}


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


def alternate(legs, iters, warm):
    for fn in legs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {leg: [] for leg in legs}
    for _ in range(ROUNDS):  # the legs alternate, so that clock and neighbour drift hits all of them alike
        for leg, fn in legs.items():
            times[leg].append(sample(fn, iters))
    report(times)


if KERNELS:
    Bk, H, hd, hdp, Lq, lead, period = 2, 16, 72, 96, 1040, 16, 1
    g = torch.Generator(device=dev).manual_seed(0)

    def rows(L, which):
        t = torch.zeros(Bk, H, L, hdp, dtype=bf16, device=dev)
        t[..., :hd] = torch.randn(Bk, H, L, hd, device=dev, generator=g).to(bf16)
        if which == "k":
            t[..., hd:hd + 2] = 1
        if which == "v":
            t[..., hd] = 1
            t[..., hd + 4] = 1
        return t[..., :hd]
    q = rows(Lq, "q")
    o = torch.empty(Bk * Lq, H * hd, dtype=bf16, device=dev)
    ov = ops.heads_view(o, Bk, Lq, H, hd)
    lse = torch.empty(Bk, H, Lq, dtype=f32, device=dev)
    LEGS = {}
    for past in (1024, 4096, 7168):
        k, v = rows(Lq + past, "k"), rows(Lq + past, "v")
        LEGS[f"attn_past_{past}"] = lambda k=k, v=v, past=past: ops.attn_fwd(q, k, v, ov, lse, kv_pad_ones=True,
                                                                             frames=(lead, period), past=past)
        LEGS[f"attn_rect_{past}"] = lambda k=k, v=v: ops.attn_fwd(q, k, v, ov, lse, kv_pad_ones=True)
    alternate(LEGS, ITERS, WARM)
    for past in (1024, 4096, 7168):
        res[f"attn_past_over_rect_{past}"] = round(res[f"attn_past_{past}_ms"] / res[f"attn_rect_{past}_ms"], 4)
    del LEGS, q, o, lse
    torch.cuda.empty_cache()

if ROLLOUT:
    torch.manual_seed(1234)
    with torch.device(dev):
        model = DiT(in_channels=16, patch_size=2, cross_attn_input_size=bench.CC, residual_v=True, train_bias_and_rms=False,
                    use_rope=True, frame_causal=True, **kw)
    gen = torch.Generator(device=dev).manual_seed(1234)
    prompt = torch.randn(1, bench.LC, bench.CC, device=dev, generator=gen).to(bf16)
    lat = torch.randn(1, *latent_shape, device=dev, generator=gen).to(bf16)
    base = (3, 5, 7)
    T = latent_shape[1] // kw["time_patch_size"]

    def rollout(k, cached):
        n_calls = -(-T // k) * STEPS * 2
        return sampling.generate_latents(model, prompt, latents=lat, inference_steps=STEPS, cfg_scale=6.0, rollout_frames=k,
                                         rope_starts=[base] if cached else [base] * n_calls, kv_cache=cached)
    LEGS = {"rollout1": lambda: rollout(1, False), "rollout1_cached": lambda: rollout(1, True),
            "rollout2": lambda: rollout(2, False), "rollout2_cached": lambda: rollout(2, True)}
    alternate(LEGS, 1, 1)
    for k in (1, 2):
        res[f"rollout{k}_speedup"] = round(res[f"rollout{k}_ms"] / res[f"rollout{k}_cached_ms"], 3)
print(json.dumps(res))
