"""The qkv / RoPE kernels with and without QK-norm at the C3b shape (B = 12, L = 8208, H = 16, head_dim 72 padded to 96,
residual-V mixing on, mix = 2 as DiT's backward calls it): forward and backward, four legs alternated inside one process:
  plain_fwd / plain_bwd    vds_qkv_rope_fwd / vds_qkv_rope_bwd (the instances every earlier commit runs)
  normed_fwd / normed_bwd  vds_qkv_rope_norm_fwd / vds_qkv_rope_norm_bwd
HIP events around ITERS calls per sample, median over ROUNDS samples per leg.  One JSON line at the end, with the bytes each
call moves by its shapes.  On a build without the normed entry points only the plain legs run (for a same-box comparison
of the plain kernels across commits)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from video_diffusion_speedrun_amd import ops  # noqa: E402

bf16, f32 = torch.bfloat16, torch.float32
B, L, H, hd, hdp = int(os.environ.get("B", 12)), int(os.environ.get("L", 8208)), 16, 72, 96
ROUNDS, ITERS, WARM = int(os.environ.get("ROUNDS", 7)), int(os.environ.get("ITERS", 5)), 3
D = H * hd
dev = "cuda"

g = torch.Generator(device=dev).manual_seed(0)
qkv = torch.randn(B * L, 3 * D, device=dev, generator=g).to(bf16)
v0 = torch.randn(B, H, L, hdp, device=dev, generator=g).to(bf16)
dq, dk, dv = (torch.randn(B, H, L, hdp, device=dev, generator=g).to(bf16) for _ in range(3))
lam = torch.tensor([0.5], device=dev).to(bf16)
dlam = torch.zeros(1, dtype=f32, device=dev)
ang = torch.rand(L, hd // 2, device=dev, generator=g) * 6.2832
cos, sin = torch.cos(ang).float().contiguous(), torch.sin(ang).float().contiguous()

has_norm = hasattr(ops, "qkv_rope_norm_fwd")
LEGS = {"plain_fwd": lambda: ops.qkv_rope_fwd(qkv, cos, sin, v0, lam, B, L, H, hd, hdp),
        "plain_bwd": lambda: ops.qkv_rope_bwd(dq, dk, dv, cos, sin, qkv, v0, lam, None, dlam, 2, False, B, L, H, hd, hdp)}
if has_norm:
    LEGS["normed_fwd"] = lambda: ops.qkv_rope_norm_fwd(qkv, cos, sin, v0, lam, B, L, H, hd, hdp)
    LEGS["normed_bwd"] = lambda: ops.qkv_rope_norm_bwd(dq, dk, dv, cos, sin, qkv, v0, lam, None, dlam, 2, False, B, L, H,
                                                       hd, hdp)


def sample(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / ITERS


for fn in LEGS.values():
    for _ in range(WARM):
        fn()
torch.cuda.synchronize()
times = {leg: [] for leg in LEGS}
for _ in range(ROUNDS):  # the legs alternate, so that clock and neighbour drift hits all of them alike
    for leg, fn in LEGS.items():
        times[leg].append(sample(fn))

rows = B * L
# bytes by shape: forward reads qkv (3D) + v0 (D) and writes q, k, v rows of hdp columns; backward reads dq, dk, dv (hd of the
# hdp columns), the raw v (D) and v0 (D), writes dqkv (3D); the normed backward reads the raw q and k columns (2D) on top
fwd_bytes = 2 * rows * (3 * D + D) + 2 * 3 * rows * H * hdp
bwd_bytes = 2 * rows * (3 * D + 2 * D + 3 * D)
res = {"B": B, "L": L, "H": H, "head_dim": hd, "hdp": hdp, "mix": 2, "rounds": ROUNDS, "iters": ITERS,
       "bytes": {"plain_fwd": fwd_bytes, "normed_fwd": fwd_bytes, "plain_bwd": bwd_bytes,
                 "normed_bwd": bwd_bytes + 2 * rows * 2 * D}}
for leg, xs in times.items():
    med = statistics.median(xs)
    res[f"{leg}_ms"] = round(med, 4)
    res[f"{leg}_min_max_ms"] = [round(min(xs), 4), round(max(xs), 4)]
    res[f"{leg}_TB_per_s"] = round(res["bytes"][leg] / med / 1e9, 3)
    print(f"{leg:10s}: median {med:8.4f} ms  (min {min(xs):.4f}, max {max(xs):.4f})  {res['bytes'][leg] / med / 1e9:.2f} TB/s by shape")
print(json.dumps(res))
