"""Cross-attention with per-sample context lengths at the C3b shape (Lq = 8208, Lk = 512, H = 16, head_dim 72, B = 12):
forward and backward of the calls the model makes (kv_pad_ones = 2, token-major queries, padded K / V copies), three legs
alternated inside one process:
  unmasked   vds_attn_fwd / vds_attn_bwd (the call without lengths: the kernels every earlier commit runs)
  full       vds_attn_*_kvlen with every length = Lk
  short      vds_attn_*_kvlen with lengths drawn uniformly from 32..160 (seeded)
HIP events around ITERS calls per sample, median over ROUNDS samples per leg.  One JSON line at the end."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from video_diffusion_speedrun_amd import ops  # noqa: E402

bf16, f32 = torch.bfloat16, torch.float32
B, H, hd, hdp = int(os.environ.get("B", 12)), 16, 72, 96
Lq, Lk = int(os.environ.get("LQ", 8208)), int(os.environ.get("LK", 512))
ROUNDS, ITERS, WARM = int(os.environ.get("ROUNDS", 7)), int(os.environ.get("ITERS", 5)), 3
D = H * hd
dev = "cuda"

g = torch.Generator(device=dev).manual_seed(0)
q = torch.randn(B * Lq, D, device=dev, generator=g).to(bf16)
kv = torch.randn(B * Lk, 2 * D, device=dev, generator=g).to(bf16)
do = torch.randn(B * Lq, D, device=dev, generator=g).to(bf16)
o = torch.empty(B * Lq, D, dtype=bf16, device=dev)
lse = torch.empty(B, H, Lq, dtype=f32, device=dev)
dq, dkv = torch.empty_like(q), torch.empty_like(kv)
ws = torch.empty(ops.attn_bwd_workspace_floats(B, H, Lq, Lk, hd, 2), dtype=f32, device=dev)
kp, vp = ops.kv_pad_ones(kv, B, Lk, H, hd, hdp, 0, D)
qv, ov, dov, dqv = (ops.heads_view(t, B, Lq, H, hd) for t in (q, o, do, dq))
dkw, dvw = ops.heads_view(dkv, B, Lk, H, hd, 0), ops.heads_view(dkv, B, Lk, H, hd, D)
cg = torch.Generator().manual_seed(1)
LEGS = {"unmasked": None,
        "full": torch.full((B,), Lk, dtype=torch.int32, device=dev),
        "short": torch.randint(32, 161, (B,), generator=cg).to(torch.int32).to(dev)}


def fwd(lens):
    ops.attn_fwd(qv, kp[..., :hd], vp[..., :hd], ov, lse, kv_pad_ones=2, kv_lens=lens)


def bwd(lens):
    ops.attn_bwd(qv, kp[..., :hd], vp[..., :hd], ov, lse, dov, dqv, dkw, dvw, ws, kv_pad_ones=2, kv_lens=lens)


def sample(fn, lens):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(ITERS):
        fn(lens)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / ITERS


times = {leg: {"fwd": [], "bwd": []} for leg in LEGS}
for leg, lens in LEGS.items():
    for _ in range(WARM):
        fwd(lens)
        bwd(lens)
torch.cuda.synchronize()
for _ in range(ROUNDS):  # the legs alternate, so that clock and neighbour drift hits all of them alike
    for leg, lens in LEGS.items():
        times[leg]["fwd"].append(sample(fwd, lens))
        fwd(lens)  # the backward of a leg reads that leg's o / lse
        times[leg]["bwd"].append(sample(bwd, lens))
res = {"B": B, "H": H, "head_dim": hd, "Lq": Lq, "Lk": Lk, "short_lens": LEGS["short"].tolist(), "rounds": ROUNDS, "iters": ITERS}
for leg in LEGS:
    for k in ("fwd", "bwd"):
        xs = times[leg][k]
        res[f"{leg}_{k}_ms"] = round(statistics.median(xs), 4)
        res[f"{leg}_{k}_min_max_ms"] = [round(min(xs), 4), round(max(xs), 4)]
        print(f"{leg:9s} {k}: median {statistics.median(xs):8.3f} ms  (min {min(xs):.3f}, max {max(xs):.3f})")
print(json.dumps(res))
