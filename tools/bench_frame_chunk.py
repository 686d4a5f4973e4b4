"""Chunk-causal self-attention at the C3b shape (DiT-XL/2, latents [12,16,16,64,64], pt = 2: t = 8 token-frames,
L = 8208 rows per sample, 16 heads of 72, frames = {16, 8}), legs alternated inside one process:

  *_plain    unmasked (vds_attn_fwd / vds_attn_bwd on the ones-column 16x16x32 kernels, as the default model runs)
  *_c1       frame-major, frame-causal (vds_attn_*_causal_fm: chunk = 1, the leg tools/bench_frame_major.py calls *_fm)
  *_c2, *_c4 frame-major, chunks of 2 / 4 token-frames (vds_attn_*_causal_fm_chunk, the same kernel instances)

and for each: the forward kernel, the backward (delta preprocess + dQ + dK/dV) and one C3b train step (frame_chunk on the
model, one noise level per sample as bench.py draws it).  The weighted fractions of 64-row tiles visited at this geometry
are printed first, per kernel and workgroup size, next to the ideal (n + 1) / (2 n) of n = t / c chunks; after the legs,
time / unmasked against those fractions.
Kernel legs: HIP events around ITERS calls per sample, median (min .. max) over ROUNDS samples per leg.  Step legs: after
two warm-up steps each, STEPS samples of ONE step each.  One JSON line at the end.  STEPS=0 skips the step legs, KERNELS=0
the kernel legs; CHUNKS=1,2,4 picks the chunk sizes."""
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
CHUNKS = [int(c) for c in os.environ.get("CHUNKS", "1,2,4").split(",")]
dev = "cuda"
kw, latent_shape = bench.WORKLOADS["c3b"][0], bench.WORKLOADS["c3b"][1]
D, H, pt = kw["hidden_size"], kw["num_heads"], kw["time_patch_size"]
hd, hdp = D // H, 96
t = latent_shape[1] // pt
LEAD = 16
L = LEAD + t * (latent_shape[2] // 2) * (latent_shape[3] // 2)
S = (L - LEAD) // t
FR = (LEAD, t)
res = {"B": B, "H": H, "L": L, "head_dim": hd, "t": t, "chunks": CHUNKS, "rounds": ROUNDS, "iters": ITERS, "steps": STEPS,
       "step_warmup": 2, "heavy_first": int(ops.knob_get("attn_fm_heavy_first"))}


# Fractions of 64-row tiles visited, from the bounds the kernels use, weighted by the rows of a workgroup:
#   forward on attn_fwd16_kernel (the forward legs at this shape): 256 queries per workgroup
#   dQ kernels: 128 queries per workgroup;  dK/dV kernels: 128 keys per workgroup, query tiles of 64
def key_tiles(qtile, c):
    vis = tot = 0
    for q0 in range(0, L, qtile):
        rows = min(q0 + qtile, L) - q0
        vis += rows * -(-ops.fm_key_end(q0, q0 + rows, LEAD, S, c, L) // 64)
        tot += rows * -(-L // 64)
    return vis / tot


def query_tiles(c):
    vis = tot = 0
    for k0 in range(0, L, 128):
        vis += -(-L // 64) - ops.fm_query_start(k0, LEAD, S, c) // 64
        tot += -(-L // 64)
    return vis / tot


frac = {}
for c in CHUNKS:
    n = -(-t // c)
    frac[c] = {"fwd": key_tiles(256, c), "dq": key_tiles(128, c), "dkv": query_tiles(c), "ideal": (n + 1) / (2 * n)}
    res[f"tiles_visited_c{c}"] = {k: round(v, 4) for k, v in frac[c].items()}
    print(f"c = {c} ({n} chunks): key tiles visited, forward (256 queries per workgroup) {frac[c]['fwd']:.4f}, dQ (128) "
          f"{frac[c]['dq']:.4f}; query tiles visited, dK/dV {frac[c]['dkv']:.4f}; (n + 1) / (2 n) = {frac[c]['ideal']:.4f}",
          flush=True)


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


def ratios(kind, fractions):
    """time / unmasked of every chunk leg of `kind` next to the fraction of tiles it visits"""
    for c in CHUNKS:
        r = res[f"{kind}_c{c}_ms"] / res[f"{kind}_plain_ms"]
        res[f"{kind}_c{c}_over_plain"] = round(r, 4)
        print(f"{kind}_c{c} / {kind}_plain = {r:.4f}   ({fractions(c)})", flush=True)


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

    def fwd(c):
        if c is None:
            return lambda: ops.attn_fwd(q[..., :hd], k[..., :hd], v[..., :hd], ov, lse, kv_pad_ones=True)
        return lambda: ops.attn_fwd(qf[..., :hd], kf[..., :hd], vf[..., :hd], ov, lse, kv_pad_ones=True, frames=FR,
                                    frame_major=True, chunk=c)

    def bwd(c):
        if c is None:
            return lambda: ops.attn_bwd(q[..., :hd], k[..., :hd], v[..., :hd], ov, lse, dov, dq[..., :hd], dk[..., :hd],
                                        dv[..., :hd], delta, kv_pad_ones=True)
        return lambda: ops.attn_bwd(qf[..., :hd], kf[..., :hd], vf[..., :hd], ov, lse, dov, dq[..., :hd], dk[..., :hd],
                                    dv[..., :hd], delta, kv_pad_ones=True, frames=FR, frame_major=True, chunk=c)

    # (each backward leg follows a forward of its own variant in the warm-up only: the timing does not depend on o / lse)
    legs = {"attn_fwd_plain": fwd(None), **{f"attn_fwd_c{c}": fwd(c) for c in CHUNKS},
            "attn_bwd_plain": bwd(None), **{f"attn_bwd_c{c}": bwd(c) for c in CHUNKS}}
    run_legs(legs, WARM, ROUNDS, ITERS)
    ratios("attn_fwd", lambda c: f"key tiles visited {frac[c]['fwd']:.4f}, ideal {frac[c]['ideal']:.4f}")
    ratios("attn_bwd", lambda c: f"tiles visited: dQ {frac[c]['dq']:.4f}, dK/dV {frac[c]['dkv']:.4f}, ideal "
                                 f"{frac[c]['ideal']:.4f}")
    del q, k, v, qf, kf, vf, qkv, o, do, dq, dk, dv, delta
    torch.cuda.empty_cache()

if STEPS:
    from video_diffusion_speedrun_amd.optim import MuAdamW
    from video_diffusion_speedrun_amd.train import get_schedule, train_step
    gen = torch.Generator(device=dev).manual_seed(1234)
    torch.manual_seed(1234)
    batch = {"latent": torch.randn(B, *latent_shape, device=dev, generator=gen).to(bf16),
             "context": torch.randn(B, bench.LC, bench.CC, device=dev, generator=gen).to(bf16), "prompt": [""] * B}
    # ONE model (a C3b step peaks near 200 GB): no flag adds a parameter, the blocks read their flags at every call
    model = bench.build_model(kw, dev, seed=1234)
    groups, _ = model.get_mup_setup(1e-4, 0.1, ["patch_proj", "context_kv", "positional_embedding"])
    opt = MuAdamW(groups, betas=(0.95, 0.99))
    sched = get_schedule(opt, "cosine", 20, 10000)

    def step(c):
        def run():
            on = c is not None
            for m in [model] + list(model.blocks):
                m.frame_causal, m.frame_major, m.frame_chunk = on, on, (c if on else 1)
            train_step(model, opt, sched, batch, dev, generator=gen)
        return run
    run_legs({"step_plain": step(None), **{f"step_c{c}": step(c) for c in CHUNKS}}, 2, STEPS, 1)
    ratios("step", lambda c: f"attention tiles: ideal {frac[c]['ideal']:.4f}")
print(json.dumps(res))
