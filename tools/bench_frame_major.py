"""Frame-major self-attention at the C3b shape (DiT-XL/2, latents [12,16,16,64,64], pt = 2: t = 8 token-frames,
L = 8208 rows per sample, 16 heads of 72, frames = {16, 8}), legs alternated inside one process.  Three variants:

  *_plain    unmasked (vds_attn_fwd / vds_attn_bwd on the ones-column 16x16x32 kernels, as the default model runs)
  *_causal   interleaved-masked (vds_attn_*_causal, the same kernels: every tile computed, compare / select per element)
  *_fm       frame-major (vds_attn_*_causal_fm, the same kernels: the key tiles no query of a tile attends are skipped)
  *_fm_mfma32  frame-major on the plain 32x32x16 kernels (variant mask 0: what every other head dim runs)

and for each: the forward kernel, the backward (delta preprocess + dQ + dK/dV), the qkv / RoPE forward and the qkv / RoPE
backward (plain and frame-major only: the price of the scatter / gather), and one C3b train step.  The fractions of key
tiles visited at this geometry are printed first, per kernel and workgroup size.
Kernel legs: HIP events around ITERS calls per sample, median (min .. max) over ROUNDS samples per leg.  Step legs: after
two warm-up steps each, STEPS samples of ONE step each.  One JSON line at the end.  STEPS=0 skips the step legs, KERNELS=0
the kernel legs.  The *_fm_plain_order legs are the frame-major kernels with the knob attn_fm_heavy_first = 0 (the
forward and dQ kernels walk a head's query tiles in their natural order instead of the longest first)."""
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
LEAD = 16
L = LEAD + t * (latent_shape[2] // 2) * (latent_shape[3] // 2)
S = (L - LEAD) // t
FR = (LEAD, t)
res = {"B": B, "H": H, "L": L, "head_dim": hd, "t": t, "rounds": ROUNDS, "iters": ITERS, "steps": STEPS, "step_warmup": 2,
       "heavy_first": int(ops.knob_get("attn_fm_heavy_first"))}

# Fractions of 64-row tiles visited, from the bounds the kernels use, per kernel and its workgroup size:
#   forward on attn_fwd16_kernel (the *_fm leg at this shape): 256 queries per workgroup
#   forward on attn_fwd_kernel (the *_fm_mfma32 leg), dQ kernels (both legs): 128 queries per workgroup
#   dK/dV kernels (both legs): 128 keys per workgroup, query tiles of 64
def key_tiles(qtile):
    vis = tot = 0
    for q0 in range(0, L, qtile):
        rows = min(q0 + qtile, L) - q0
        vis += rows * -(-ops.fm_key_end(q0, q0 + rows, LEAD, S) // 64)
        tot += rows * -(-L // 64)
    return vis / tot


visk = totk = 0
for k0 in range(0, L, 128):
    visk += -(-L // 64) - ops.fm_query_start(k0, LEAD, S) // 64
    totk += -(-L // 64)
res["key_tiles_visited_fwd16_q256"] = round(key_tiles(256), 4)
res["key_tiles_visited_q128"] = round(key_tiles(128), 4)
res["query_tiles_visited_dkv"] = round(visk / totk, 4)
print(f"key tiles visited: forward, 256 queries per workgroup (attn_fwd16_kernel) {key_tiles(256):.4f}; forward (mfma32) and "
      f"dQ, 128 queries per workgroup {key_tiles(128):.4f}; query tiles visited, dK/dV {visk / totk:.4f}; "
      f"(t + 1) / (2 t) = {(t + 1) / (2 * t):.4f}", flush=True)


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


def with_knobs(fn, call):
    """call() under the knobs a leg carries (fn.knobs), restored afterwards"""
    prev = {k: ops.knob_set(k, v) for k, v in getattr(fn, "knobs", {}).items()}
    try:
        return call()
    finally:
        for k, v in prev.items():
            ops.knob_set(k, v)


def run_legs(legs, warm, rounds, iters):
    for fn in legs.values():
        with_knobs(fn, lambda: [fn() for _ in range(warm)])
    torch.cuda.synchronize()
    times = {leg: [] for leg in legs}
    for _ in range(rounds):  # the legs alternate, so that clock and neighbour drift hits all of them alike
        for leg, fn in legs.items():
            times[leg].append(with_knobs(fn, lambda: sample(fn, iters)))
    report(times)


if KERNELS:
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B * L, 3 * D, device=dev, generator=g).to(bf16)
    cos = torch.ones(L, hd // 2, dtype=f32, device=dev)
    sin = torch.zeros(L, hd // 2, dtype=f32, device=dev)
    q, k, v = ops.qkv_rope_fwd(qkv, cos, sin, None, None, B, L, H, hd, hdp)
    qf, kf, vf = ops.qkv_rope_fwd(qkv, cos, sin, None, None, B, L, H, hd, hdp, frames=FR)
    o = torch.empty(B * L, D, dtype=bf16, device=dev)
    do = torch.randn(B * L, D, device=dev, generator=g).to(bf16)
    lse = torch.empty(B, H, L, dtype=f32, device=dev)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    delta = torch.empty(ops.attn_bwd_workspace_floats(B, H, L, L, hd, True), dtype=f32, device=dev)
    ov, dov = ops.heads_view(o, B, L, H, hd), ops.heads_view(do, B, L, H, hd)

    def fwd(frames, fm=False):
        a, b_, c = (qf, kf, vf) if fm else (q, k, v)
        return lambda: ops.attn_fwd(a[..., :hd], b_[..., :hd], c[..., :hd], ov, lse, kv_pad_ones=True, frames=frames,
                                    frame_major=fm)

    def bwd(frames, fm=False):
        a, b_, c = (qf, kf, vf) if fm else (q, k, v)
        return lambda: ops.attn_bwd(a[..., :hd], b_[..., :hd], c[..., :hd], ov, lse, dov, dq[..., :hd], dk[..., :hd],
                                    dv[..., :hd], delta, kv_pad_ones=True, frames=frames, frame_major=fm)

    def plain_order(fn):
        """the leg under the knob attn_fm_heavy_first = 0 (a head's row tiles in their natural order); run_legs sets the
        knob around the leg's warm-up and around each of its samples, outside the timed region"""
        fn.knobs = {"attn_fm_heavy_first": 0}
        return fn

    def mfma32(fn):
        fn.knobs = {"attn_mfma16": 0}
        return fn

    def rope_fwd(frames):
        return lambda: ops.qkv_rope_fwd(qkv, cos, sin, None, None, B, L, H, hd, hdp, frames=frames)

    def rope_bwd(frames):
        return lambda: ops.qkv_rope_bwd(dq, dk, dv, cos, sin, None, None, None, None, None, 0, 0, B, L, H, hd, hdp,
                                        frames=frames)

    # (each backward leg follows a forward of its own variant in the warm-up only: the timing does not depend on o / lse;
    # dq / dk / dv hold the last backward's finite values when the RoPE backward legs read them)
    run_legs({"attn_fwd_plain": fwd(None), "attn_fwd_causal": fwd(FR), "attn_fwd_fm": fwd(FR, True),
              "attn_fwd_fm_plain_order": plain_order(fwd(FR, True)), "attn_fwd_fm_mfma32": mfma32(fwd(FR, True)),
              "attn_bwd_plain": bwd(None), "attn_bwd_causal": bwd(FR), "attn_bwd_fm": bwd(FR, True),
              "attn_bwd_fm_plain_order": plain_order(bwd(FR, True)), "attn_bwd_fm_mfma32": mfma32(bwd(FR, True)),
              "rope_fwd_plain": rope_fwd(None), "rope_fwd_fm": rope_fwd(FR),
              "rope_bwd_plain": rope_bwd(None), "rope_bwd_fm": rope_bwd(FR)}, WARM, ROUNDS, ITERS)
    del q, k, v, qf, kf, vf, qkv, o, do, dq, dk, dv, delta
    torch.cuda.empty_cache()

if STEPS:
    from video_diffusion_speedrun_amd.optim import MuAdamW
    from video_diffusion_speedrun_amd.train import get_schedule, train_step
    gen = torch.Generator(device=dev).manual_seed(1234)
    torch.manual_seed(1234)
    batch = {"latent": torch.randn(B, *latent_shape, device=dev, generator=gen).to(bf16),
             "context": torch.randn(B, bench.LC, bench.CC, device=dev, generator=gen).to(bf16), "prompt": [""] * B}
    # ONE model (a C3b step peaks near 200 GB): neither flag adds a parameter, the blocks read their flags at every call
    model = bench.build_model(kw, dev, seed=1234)
    groups, _ = model.get_mup_setup(1e-4, 0.1, ["patch_proj", "context_kv", "positional_embedding"])
    opt = MuAdamW(groups, betas=(0.95, 0.99))
    sched = get_schedule(opt, "cosine", 20, 10000)

    def step(causal, fm):
        def run():
            model.frame_causal, model.frame_major = causal, fm
            for blk in model.blocks:
                blk.frame_causal, blk.frame_major = causal, fm
            train_step(model, opt, sched, batch, dev, generator=gen)
        return run
    run_legs({"step_plain": step(False, False), "step_causal": step(True, False), "step_fm": step(True, True)}, 2, STEPS, 1)
print(json.dumps(res))
