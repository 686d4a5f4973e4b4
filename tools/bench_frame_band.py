"""Frame-band self-attention of the bidirectional model at a bench.py workload (--workload c3b: DiT-XL/2, latents
[12,16,16,64,64], pt = 2: t = 8 token-frames, L = 8208 rows per sample, 16 heads of 72, frames = {16, 8}), legs alternated
inside one process:

  *_plain          unmasked (vds_attn_fwd / vds_attn_bwd on the ones-column 16x16x32 kernels, as the default model runs)
  *_b0, *_b1, *_b2 the frame band of 0 / 1 / 2 token-frames on each side at chunk = 1 (vds_band_attn_fwd / _bwd: the BAND
                   instances of the plain 32x32x16 frame-major kernels, on frame-major rows)

and for each: the forward kernel, the backward (delta preprocess + dK/dV + dQ) and one train step (enable_frame_band on the
model, one noise level per sample as bench.py draws it).  The fraction of 64-row tiles visited at this geometry is printed
first, from the bounds the kernels use (ops.fm_band_lo / fm_band_hi; the forward, dQ and dK/dV kernels all hold 128 rows per
workgroup and the relation is symmetric, so the three fractions are one number); after the legs, time / unmasked next to
that fraction, and their quotient.
Kernel legs: HIP events around ITERS calls per sample, median (min .. max) over ROUNDS samples per leg.  Step legs: after
two warm-up steps each, STEPS samples of ONE step each.  One JSON line at the end.  STEPS=0 skips the step legs, KERNELS=0
the kernel legs; BANDS=0,1,2 picks the bands, STEP_BANDS=1 those of the step legs."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from video_diffusion_speedrun_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="c3b", choices=sorted(bench.WORKLOADS))
args = ap.parse_args()

bf16, f32 = torch.bfloat16, torch.float32
ROUNDS, ITERS, WARM = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("ITERS", 3)), 2
STEPS, KERNELS = int(os.environ.get("STEPS", 4)), int(os.environ.get("KERNELS", 1))
BANDS = [int(b) for b in os.environ.get("BANDS", "0,1,2").split(",")]
STEP_BANDS = [int(b) for b in os.environ.get("STEP_BANDS", "1").split(",")]
dev = "cuda"
kw, latent_shape = bench.WORKLOADS[args.workload][0], bench.WORKLOADS[args.workload][1]
B = int(os.environ.get("B", 12))
D, H, pt = kw["hidden_size"], kw["num_heads"], kw["time_patch_size"]
hd = D // H
hdp = 96 if hd == 72 else hd
ones = hdp - hd >= 8
t = latent_shape[1] // pt
LEAD = 16
HW = (latent_shape[2] // 2) * (latent_shape[3] // 2)
L = LEAD + t * HW
S = (L - LEAD) // t
FR = (LEAD, t)
name = lambda b: f"b{b}"
res = {"workload": args.workload, "B": B, "H": H, "L": L, "head_dim": hd, "t": t, "bands": BANDS, "rounds": ROUNDS,
       "iters": ITERS, "steps": STEPS, "step_warmup": 2}


def tiles(b, tile=128):
    """fraction of 64-row tiles a BAND workgroup of `tile` rows visits: all of them with a lead row in it, else the lead
    tiles and those from lo of its first row to below hi of its last"""
    vis = tot = 0
    for r0 in range(0, L, tile):
        r1 = min(r0 + tile, L)
        n_all = -(-L // 64)
        if r0 < LEAD:
            n = n_all
        else:
            end = -(-ops.fm_band_hi(r1 - 1, LEAD, S, 1, b, L) // 64)
            nl = min(end, -(-LEAD // 64))
            n = nl + end - max(nl, ops.fm_band_lo(r0, LEAD, S, 1, b) // 64)
        vis += (r1 - r0) * n
        tot += (r1 - r0) * n_all
    return vis / tot


frac = {b: tiles(b) for b in sorted(set(BANDS + STEP_BANDS))}
pairs = lambda b: sum(1 for x in range(t) for y in range(t) if abs(x - y) <= b) / (t * t)
for b, f in frac.items():
    res[f"tiles_visited_{name(b)}"] = round(f, 4)
    print(f"{name(b)}: 64-row tiles visited (forward, dQ, dK/dV: 128 rows per workgroup) {f:.4f}; frame pairs a token "
          f"attends {pairs(b):.4f}", flush=True)


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


def ratios(kind, bands, with_fraction=True):
    """time / unmasked of every band leg of `kind` next to the fraction of tiles it visits, and their quotient"""
    for b in bands:
        r = res[f"{kind}_{name(b)}_ms"] / res[f"{kind}_plain_ms"]
        res[f"{kind}_{name(b)}_over_plain"] = round(r, 4)
        if with_fraction:
            res[f"{kind}_{name(b)}_over_plain_over_fraction"] = round(r / frac[b], 4)
            print(f"{kind}_{name(b)} / {kind}_plain = {r:.4f}   (tiles visited {frac[b]:.4f}: time / fraction = "
                  f"{r / frac[b]:.3f})", flush=True)
        else:
            print(f"{kind}_{name(b)} / {kind}_plain = {r:.4f}", flush=True)


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
    delta = torch.empty(ops.attn_bwd_workspace_floats(B, H, L, L, hd, ones), dtype=f32, device=dev)
    ov, dov = ops.heads_view(o, B, L, H, hd), ops.heads_view(do, B, L, H, hd)
    bkw = lambda b: dict(kv_pad_ones=ones, frames=FR, frame_major=True, chunk=1, band=b)

    def fwd(b):
        if b is None:
            return lambda: ops.attn_fwd(q[..., :hd], k[..., :hd], v[..., :hd], ov, lse, kv_pad_ones=ones)
        return lambda: ops.band_attn_fwd(qf[..., :hd], kf[..., :hd], vf[..., :hd], ov, lse, **bkw(b))

    def bwd(b):
        if b is None:
            return lambda: ops.attn_bwd(q[..., :hd], k[..., :hd], v[..., :hd], ov, lse, dov, dq[..., :hd], dk[..., :hd],
                                        dv[..., :hd], delta, kv_pad_ones=ones)
        return lambda: ops.band_attn_bwd(qf[..., :hd], kf[..., :hd], vf[..., :hd], ov, lse, dov, dq[..., :hd], dk[..., :hd],
                                         dv[..., :hd], delta, **bkw(b))

    # (each backward leg follows a forward of its own variant in the warm-up only: the timing does not depend on o / lse)
    legs = {"attn_fwd_plain": fwd(None), **{f"attn_fwd_{name(b)}": fwd(b) for b in BANDS},
            "attn_bwd_plain": bwd(None), **{f"attn_bwd_{name(b)}": bwd(b) for b in BANDS}}
    run_legs(legs, WARM, ROUNDS, ITERS)
    ratios("attn_fwd", BANDS)
    ratios("attn_bwd", BANDS)
    del q, k, v, qf, kf, vf, qkv, o, do, dq, dk, dv, delta
    torch.cuda.empty_cache()

if STEPS:
    from video_diffusion_speedrun_amd.optim import MuAdamW
    from video_diffusion_speedrun_amd.train import get_schedule, train_step
    gen = torch.Generator(device=dev).manual_seed(1234)
    torch.manual_seed(1234)
    batch = {"latent": torch.randn(B, *latent_shape, device=dev, generator=gen).to(bf16),
             "context": torch.randn(B, bench.LC, bench.CC, device=dev, generator=gen).to(bf16), "prompt": [""] * B}
    # ONE model (a C3b step peaks near 200 GB): the switch adds no parameter, the blocks read it at every call
    model = bench.build_model(kw, dev, seed=1234)
    groups, _ = model.get_mup_setup(1e-4, 0.1, ["patch_proj", "context_kv", "positional_embedding"])
    opt = MuAdamW(groups, betas=(0.95, 0.99))
    sched = get_schedule(opt, "cosine", 20, 10000)

    def step(b):
        def run():
            model.enable_frame_band(b)
            train_step(model, opt, sched, batch, dev, generator=gen)
        return run
    run_legs({"step_plain": step(None), **{f"step_{name(b)}": step(b) for b in STEP_BANDS}}, 2, STEPS, 1)
    ratios("step", STEP_BANDS, with_fraction=False)
print(json.dumps(res))
