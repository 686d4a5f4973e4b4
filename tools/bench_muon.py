"""The optimizer step alone, MuAdamW against MuonAdamW, on a DiT of the size given on the command line (HIP events;
the two legs alternate inside ONE process and the spread over the rounds is printed).

    python tools/bench_muon.py                                  # DiT-XL: hidden 1152, depth 28, context width 4096
    python tools/bench_muon.py --hidden 128 --depth 3 --heads 2 --context 64

The gradients are seeded Gaussians written into the model's gradient buffers (no forward / backward runs).  Printed:
the Newton-Schulz FLOPs of one step computed from the model's real shapes -- per matrix [m, n] (m <= n) and iteration
2 m^2 n (A = X X^T) + 2 m^3 (A A) + 2 m^2 n (B X), full products: the symmetric halves the kernels skip are NOT
subtracted --, and the TFLOP/s that the orthogonalisation launches alone achieve against that count.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from video_diffusion_speedrun_amd import ops, optim
from video_diffusion_speedrun_amd.model import DiT

ap = argparse.ArgumentParser()
ap.add_argument("--hidden", type=int, default=1152)
ap.add_argument("--depth", type=int, default=28)
ap.add_argument("--heads", type=int, default=16)
ap.add_argument("--context", type=int, default=4096, help="cross-attention input width")
ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds")
ap.add_argument("--iters", type=int, default=3, help="steps per timed window")
ap.add_argument("--ns-steps", type=int, default=5)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_muon.py measures on the GPU: no device, no number"
CONSTS = ["patch_proj", "context_kv", "positional_embedding"]


def make(muon: bool):
    torch.manual_seed(0)
    m = DiT(in_channels=16, hidden_size=args.hidden, depth=args.depth, num_heads=args.heads,
            cross_attn_input_size=args.context, residual_v=True).to("cuda")
    m._ensure_groups(torch.device("cuda", torch.cuda.current_device()))
    gen = torch.Generator(device="cuda").manual_seed(1)
    for grp in m._groups:
        grp.gfull.normal_(0.0, 1e-3, generator=gen)
        grp.publish_grads()
    if muon:
        groups, table = m.get_muon_setup(1e-4, 0.1, CONSTS, ns_steps=args.ns_steps)
        return m, optim.MuonAdamW(groups, betas=(0.95, 0.99)), table
    groups, table = m.get_mup_setup(1e-4, 0.1, CONSTS)
    return m, optim.MuAdamW(groups, betas=(0.95, 0.99)), table


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


_, adam, _ = make(False)
model, muon, table = make(True)
flops, nmat, nparam = 0.0, 0, 0
for name, info in table.items():
    if info.get("muon"):
        rows, cols = info["shape"][0] // info["split"], info["shape"][1]
        m_, n_ = min(rows, cols), max(rows, cols)
        flops += info["split"] * args.ns_steps * (4.0 * m_ * m_ * n_ + 2.0 * m_ ** 3)
        nmat += info["split"]
        nparam += info["shape"][0] * info["shape"][1]


def ns_only():  # the orthogonalisation launches of one step, on whatever the last step left in the workspace
    for (rows, cols, _, _, _, _, steps), b in muon._muon.items():
        for _, n in b["slices"]:
            ops.muon_orthogonalize(muon._muon_ws, n, rows, cols, steps)


for o in (adam, muon):
    for _ in range(2):
        o.step()
torch.cuda.synchronize()
legs = [("MuAdamW step", adam.step), ("MuonAdamW step", muon.step), ("Newton-Schulz launches", ns_only)]
times = {k: [] for k, _ in legs}
for _ in range(args.rounds):
    for k, fn in legs:
        times[k].append(timed(fn, args.iters))
total = sum(p.numel() for p in model.parameters())
print(f"bench_muon: hidden {args.hidden} depth {args.depth} heads {args.heads} context {args.context}: "
      f"{total/1e6:.1f}M parameters, {nparam/1e6:.1f}M of them in {nmat} Muon matrices; Newton-Schulz "
      f"{flops/1e12:.3f} TFLOP per step ({args.ns_steps} iterations); {args.rounds} interleaved rounds x {args.iters} steps")
med = {}
for k, _ in legs:
    ts = sorted(times[k])
    med[k] = ts[len(ts) // 2]
    print(f"  {k:24s} {med[k]:9.3f} ms (min {ts[0]:.3f} max {ts[-1]:.3f})")
print(f"  Newton-Schulz achieved {flops / (med['Newton-Schulz launches'] * 1e-3) / 1e12:.1f} TFLOP/s; "
      f"MuonAdamW - MuAdamW = {med['MuonAdamW step'] - med['MuAdamW step']:+.3f} ms per step")
print(json.dumps({"tool": "bench_muon", "hidden": args.hidden, "depth": args.depth, "context": args.context,
                  "ns_tflop_per_step": flops / 1e12, "adamw_ms": med["MuAdamW step"], "muon_adamw_ms": med["MuonAdamW step"],
                  "ns_ms": med["Newton-Schulz launches"],
                  "ns_tflops": flops / (med["Newton-Schulz launches"] * 1e-3) / 1e12}))
