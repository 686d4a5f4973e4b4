"""Sliding-window self-attention at the C3b shape (DiT-XL/2, latents [12,16,16,64,64], pt = 2: t = 8 token-frames,
L = 8208 rows per sample, 16 heads of 72, frames = {16, 8}), legs alternated inside one process:

  *_plain    unmasked (vds_attn_fwd / vds_attn_bwd on the ones-column 16x16x32 kernels, as the default model runs)
  *_fm       frame-major, frame-causal, no window (vds_attn_*_causal_fm: the leg tools/bench_frame_chunk.py calls *_c1)
  *_w1, *_w2, *_w4   frame-major with a window of 1 / 2 / 4 token-frames at frame_chunk = 1 (vds_attn_*_causal_fm_window:
             the WIN instances of the same kernel families)

and for each: the forward kernel, the backward (delta preprocess + dQ + dK/dV) and one C3b train step (frame_window on the
model, one noise level per sample as bench.py draws it).  The fractions of 64-row tiles visited at this geometry are printed
first, per kernel and workgroup size, from the bounds the kernels use; after the legs, time / unmasked against those
fractions, and each time divided by its fraction.  The K / V bytes of the ring cache of a w = 2 model against the unbounded
cache of the same video are printed too (DiT.new_frame_cache's row counts; nothing is allocated).
Kernel legs: HIP events around ITERS calls per sample, median (min .. max) over ROUNDS samples per leg.  Step legs: after
two warm-up steps each, STEPS samples of ONE step each.  One JSON line at the end.  STEPS=0 skips the step legs, KERNELS=0
the kernel legs; WINDOWS=1,2,4 picks the windows."""
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
WINDOWS = [int(w) for w in os.environ.get("WINDOWS", "1,2,4").split(",")]
dev = "cuda"
kw, latent_shape = bench.WORKLOADS["c3b"][0], bench.WORKLOADS["c3b"][1]
D, H, pt = kw["hidden_size"], kw["num_heads"], kw["time_patch_size"]
hd, hdp = D // H, 96
t = latent_shape[1] // pt
LEAD = 16
HW = (latent_shape[2] // 2) * (latent_shape[3] // 2)
L = LEAD + t * HW
S = (L - LEAD) // t
FR = (LEAD, t)
LEGS = [None] + WINDOWS  # None: frame-major without a window
name = lambda w: "fm" if w is None else f"w{w}"
res = {"B": B, "H": H, "L": L, "head_dim": hd, "t": t, "windows": WINDOWS, "rounds": ROUNDS, "iters": ITERS, "steps": STEPS,
       "step_warmup": 2, "heavy_first": int(ops.knob_get("attn_fm_heavy_first"))}


# Fractions of 64-row tiles visited, from the bounds the kernels use, weighted by the rows of a workgroup:
#   forward on attn_fwd16_kernel (the forward legs at this shape): 256 queries per workgroup
#   dQ kernels: 128 queries per workgroup;  dK/dV kernels: 128 keys per workgroup, query tiles of 64
def key_tiles(qtile, w):
    vis = tot = 0
    for q0 in range(0, L, qtile):
        rows = min(q0 + qtile, L) - q0
        nkt = -(-ops.fm_key_end(q0, q0 + rows, LEAD, S, 1, L) // 64)
        n = nkt
        if w is not None and q0 + rows > LEAD:  # the lead tiles, then from the tile that holds kbeg of the first token query
            nl = min(nkt, -(-LEAD // 64))
            n = nl + nkt - max(nl, ops.fm_key_begin(max(q0, LEAD), LEAD, S, 1, w) // 64)
        vis += rows * n
        tot += rows * -(-L // 64)
    return vis / tot


def query_tiles(w):
    vis = tot = 0
    for k0 in range(0, L, 128):
        k1 = min(k0 + 128, L)
        end = -(-L // 64) if (w is None or k0 < LEAD) else -(-ops.fm_query_end(k1, LEAD, S, 1, w, L) // 64)
        vis += end - ops.fm_query_start(k0, LEAD, S, 1) // 64
        tot += -(-L // 64)
    return vis / tot


frac = {}
for w in LEGS:
    frac[w] = {"fwd": key_tiles(256, w), "dq": key_tiles(128, w), "dkv": query_tiles(w)}
    res[f"tiles_visited_{name(w)}"] = {k: round(v, 4) for k, v in frac[w].items()}
    print(f"{name(w):3s}: key tiles visited, forward (256 queries per workgroup) {frac[w]['fwd']:.4f}, dQ (128) "
          f"{frac[w]['dq']:.4f}; query tiles visited, dK/dV {frac[w]['dkv']:.4f}", flush=True)

# K / V bytes of a rollout's cache at this shape: per block and buffer [batch, H, rows, hdp] bf16
depth = kw["depth"]
cache_bytes = lambda rows: 2 * depth * 2 * H * rows * hdp * 2  # (k, v) x blocks x (guided pair) x heads x rows x bytes
res["cache_bytes_unbounded"] = cache_bytes(LEAD + t * HW)
res["cache_bytes_ring_w2"] = cache_bytes(LEAD + 2 * HW)
print(f"frame KV cache, guided pair, {t} frames: unbounded {res['cache_bytes_unbounded'] / 2**20:.1f} MiB, ring of w = 2 "
      f"{res['cache_bytes_ring_w2'] / 2**20:.1f} MiB (constant in the video's length)", flush=True)


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


def ratios(kind, fraction):
    """time / unmasked of every frame-major leg of `kind` next to the fraction of tiles it visits, and their quotient"""
    for w in LEGS:
        r = res[f"{kind}_{name(w)}_ms"] / res[f"{kind}_plain_ms"]
        res[f"{kind}_{name(w)}_over_plain"] = round(r, 4)
        f = fraction(w)
        if f is None:
            print(f"{kind}_{name(w)} / {kind}_plain = {r:.4f}", flush=True)
        else:
            res[f"{kind}_{name(w)}_over_plain_over_fraction"] = round(r / f, 4)
            print(f"{kind}_{name(w)} / {kind}_plain = {r:.4f}   (tiles visited {f:.4f}: time / fraction = {r / f:.3f})", flush=True)


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
    wkw = lambda w: dict(kv_pad_ones=True, frames=FR, frame_major=True, **({} if w is None else {"window": w}))

    def fwd(w, plain=False):
        if plain:
            return lambda: ops.attn_fwd(q[..., :hd], k[..., :hd], v[..., :hd], ov, lse, kv_pad_ones=True)
        return lambda: ops.attn_fwd(qf[..., :hd], kf[..., :hd], vf[..., :hd], ov, lse, **wkw(w))

    def bwd(w, plain=False):
        if plain:
            return lambda: ops.attn_bwd(q[..., :hd], k[..., :hd], v[..., :hd], ov, lse, dov, dq[..., :hd], dk[..., :hd],
                                        dv[..., :hd], delta, kv_pad_ones=True)
        return lambda: ops.attn_bwd(qf[..., :hd], kf[..., :hd], vf[..., :hd], ov, lse, dov, dq[..., :hd], dk[..., :hd],
                                    dv[..., :hd], delta, **wkw(w))

    # (each backward leg follows a forward of its own variant in the warm-up only: the timing does not depend on o / lse)
    legs = {"attn_fwd_plain": fwd(None, True), **{f"attn_fwd_{name(w)}": fwd(w) for w in LEGS},
            "attn_bwd_plain": bwd(None, True), **{f"attn_bwd_{name(w)}": bwd(w) for w in LEGS}}
    run_legs(legs, WARM, ROUNDS, ITERS)
    ratios("attn_fwd", lambda w: frac[w]["fwd"])
    # (the backward runs two kernels of about equal work: the mean of their fractions)
    ratios("attn_bwd", lambda w: 0.5 * (frac[w]["dq"] + frac[w]["dkv"]))
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

    def step(w, plain=False):
        def run():
            for m in [model] + list(model.blocks):
                m.frame_causal, m.frame_major, m.frame_window = not plain, not plain, w
            train_step(model, opt, sched, batch, dev, generator=gen)
        return run
    run_legs({"step_plain": step(None, True), **{f"step_{name(w)}": step(w) for w in LEGS}}, 2, STEPS, 1)
    ratios("step", lambda w: None)
print(json.dumps(res))
