"""AdamW kernel alone on DiT-XL-sized state (HIP events): GB/s of the 30 B/parameter stream.

    python tools/bench_adamw.py                      # the plain step, as always (VDS_LIB_PATH selects another library build)
    python tools/bench_adamw.py --guard              # plain, clipped and clipped + EMA steps in ONE process, interleaved,
                                                     # + the sum-of-squares and the guarded kernel on their own
Each variant is priced against its own byte count per parameter: plain 30 B (16 read + 14 written), the sum of squares
4 B, the guarded kernel with an EMA 38 B, a clipped step 34 B and a clipped + EMA step 42 B.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from video_diffusion_speedrun_amd.optim import MuAdamW

ap = argparse.ArgumentParser()
ap.add_argument("--guard", action="store_true", help="also time the clipped and the clipped + EMA step, interleaved with the plain one")
ap.add_argument("--rounds", type=int, default=5, help="--guard: interleaved rounds (the spread over them is printed)")
ap.add_argument("--iters", type=int, default=10, help="steps per timed window")
args = ap.parse_args()

n = int(os.environ.get("N", 675_000_000)) // 8 * 8
ps = []
for i in range(8):  # a few big tensors like the flat groups
    p = torch.nn.Parameter(torch.randn(n // 8, device="cuda"))
    p.grad = torch.randn(n // 8, device="cuda") * 1e-3
    p._vds_shadow = torch.empty(n // 8, dtype=torch.bfloat16, device="cuda")
    ps.append(p)


def make(**opts):
    return MuAdamW([{"params": ps, "lr": 1e-4, "weight_decay": 0.1}], betas=(0.95, 0.99), **opts)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


opt = make()
for _ in range(3):
    opt.step()
torch.cuda.synchronize()
if not args.guard:
    t = timed(opt.step, args.iters)
    print(f"adamw {n/1e6:.0f}M params: {t*1e3:.3f} ms  {30*n/t/1e9:.0f} GB/s  lib={os.environ.get('VDS_LIB_PATH','default')}")
    sys.exit(0)

from video_diffusion_speedrun_amd import _lib, ops
from video_diffusion_speedrun_amd.optim import CHUNK

# max_grad_norm far above the norm: the coefficient is 1 and the parameters walk as in the plain step
clip = make(max_grad_norm=1e9, skip_nonfinite=True)
clip_ema = make(max_grad_norm=1e9, skip_nonfinite=True, ema_decay=0.999)
for o in (clip, clip_ema):
    for _ in range(3):
        o.step()
torch.cuda.synchronize()
lib, d = _lib.load(), clip_ema._dev


def sumsq_only():
    lib.vds_grad_sumsq_multi(d["desc"].data_ptr(), d["ct"].data_ptr(), d["cs"].data_ptr(), d["n"], CHUNK, d["ws"].data_ptr(),
                             d["sumsq"].data_ptr(), 1e9, 1, clip_ema._guard.data_ptr(), ops._stream())


def guarded_only():  # reads the record the last finalize left (applied, coefficient 1)
    lib.vds_adamw_guarded_multi(d["desc"].data_ptr(), d["ct"].data_ptr(), d["cs"].data_ptr(), d["n"], CHUNK, 0.95, 0.99, 1e-8,
                                100, 1.0, 1.0, clip_ema._guard.data_ptr(), d["ema"].data_ptr(), 0.999, ops._stream())


variants = [("plain step", opt.step, 30), ("clipped step", clip.step, 34), ("clipped + EMA step", clip_ema.step, 42),
            ("sum-of-squares kernels", sumsq_only, 4), ("guarded kernel + EMA", guarded_only, 38)]
times = {name: [] for name, _, _ in variants}
for r in range(args.rounds):
    for name, fn, _ in variants:
        times[name].append(timed(fn, args.iters))
print(f"adamw variants, {n/1e6:.0f}M params, {args.rounds} interleaved rounds x {args.iters} steps, "
      f"lib={os.environ.get('VDS_LIB_PATH','default')}")
base = sorted(times["plain step"])[len(times["plain step"]) // 2]
for name, _, bpp in variants:
    ts = sorted(times[name])
    med = ts[len(ts) // 2]
    print(f"  {name:24s} {med*1e3:7.3f} ms (min {ts[0]*1e3:.3f} max {ts[-1]*1e3:.3f})  {bpp:2d} B/param  "
          f"{bpp*n/med/1e9:5.0f} GB/s  {(med-base)*1e3:+.3f} ms vs plain")
assert clip_ema.skipped_steps() == 0
