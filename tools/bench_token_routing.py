"""Token routing (DiT.enable_token_routing) at a bench.py workload (--workload c3b: DiT-XL/2, latents [12,16,16,64,64], pt = 2:
N = 8192 tokens, L = 8208 rows per sample, 16 heads of 72), legs alternated inside one process:

  step_off            the train step with routing off (the kernel sequence of a model without the switch)
  step_k50, step_k75  the train step with enable_token_routing(FIRST, LAST, keep), keep = 0.5 and 0.75 (KEEPS), blocks
                      FIRST..LAST = 2..23 of 28; a new route is drawn every step, as in training

After two warm-up steps each, STEPS samples of ONE step each, timed with device events; per leg the peak of
torch.cuda.max_memory_allocated next to model.activation_bytes(routing=).  step / step_off is printed next to the FLOP
estimate of the routed step -- a routed block at keep f costs (1 - a) f + a f^2 of a full one with a = ATTN_SHARE, the
self-attention's share of a block (0.51 at C3b) -- which is an estimate, not a threshold.

CLASSES=1 (default): one more step per leg with the library's per-class profiler on (ops.prof_enable: an event pair per
launch, so this step is not a timing of the step), printed by kernel class: where the time of a routed step goes.

KERNELS=1 (default): the three row movers on the tensors the routed step moves -- the token buffer [B, L, D] bf16, residual-V's
v_0 [B*H, L, hdp] bf16 and its fp32 gradient -- ITERS = 200 calls between two device events (windows of 10-40 ms), rotating
over NBUF buffer sets so that no call finds its rows in the 256 MiB Infinity Cache, median over ROUNDS; bytes = what the
kernel must read and write, computed from the shapes; the fraction of the 8 TB/s HBM peak is printed next to
rmsnorm_mod_fwd's 0.65.
One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from video_diffusion_speedrun_amd import model as M  # noqa: E402
from video_diffusion_speedrun_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="c3b", choices=sorted(bench.WORKLOADS))
args = ap.parse_args()

bf16, f32 = torch.bfloat16, torch.float32
ROUNDS, ITERS, NBUF = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("ITERS", 200)), int(os.environ.get("NBUF", 3))
STEPS, KERNELS, CLASSES = int(os.environ.get("STEPS", 4)), int(os.environ.get("KERNELS", 1)), int(os.environ.get("CLASSES", 1))
KEEPS = [float(k) for k in os.environ.get("KEEPS", "0.5,0.75").split(",")]
FIRST, LAST = int(os.environ.get("FIRST", 2)), int(os.environ.get("LAST", 23))
ATTN_SHARE = float(os.environ.get("ATTN_SHARE", 0.51))
HBM_PEAK = 8.0e12
dev = "cuda"
kw, latent_shape = bench.WORKLOADS[args.workload][0], bench.WORKLOADS[args.workload][1]
B = int(os.environ.get("B", 12))
D, H, pt, depth = kw["hidden_size"], kw["num_heads"], kw["time_patch_size"], kw["depth"]
hd = D // H
hdp = M.HDP_OF[hd]
N = (latent_shape[1] // pt) * (latent_shape[2] // 2) * (latent_shape[3] // 2)
L = M.N_REG + N
LAST = min(LAST, depth - 1)
name = lambda keep: f"k{int(round(keep * 100))}"
res = {"workload": args.workload, "B": B, "H": H, "L": L, "head_dim": hd, "depth": depth, "span": [FIRST, LAST],
       "keeps": KEEPS, "steps": STEPS, "step_warmup": 2, "rounds": ROUNDS, "iters": ITERS, "nbuf": NBUF}


def estimate(keep):
    """FLOP estimate of the routed step over the unrouted one"""
    block = (1 - ATTN_SHARE) * keep + ATTN_SHARE * keep * keep
    n = LAST - FIRST + 1
    return (depth - n + n * block) / depth


def sample(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def run_legs(legs, warm, rounds, iters):
    for fn in legs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {leg: [] for leg in legs}
    for _ in range(rounds):  # the legs alternate, so that clock and neighbour drift hits all of them alike
        for leg, fn in legs.items():
            times[leg].append(sample(fn, iters))
    for leg, xs in times.items():
        med = statistics.median(xs)
        res[f"{leg}_ms"] = round(med, 4)
        res[f"{leg}_min_max_ms"] = [round(min(xs), 4), round(max(xs), 4)]
        print(f"{leg:24s}: median {med:10.4f} ms  (min {min(xs):.4f}, max {max(xs):.4f})", flush=True)


if KERNELS:
    keep = KEEPS[0]
    k = M.route_keep_count(N, keep)
    Ls = M.N_REG + k
    gen = torch.Generator().manual_seed(0)
    idx_c, inv_c = M.route_tables(torch.randperm(N, generator=gen)[:k].sort().values, N)
    idx, inv = idx_c.to(dev), inv_c.to(dev)
    sets = []
    for _ in range(NBUF):
        sets.append(dict(X=torch.randn(B, L, D, device=dev).to(bf16), Xs=torch.empty(B, Ls, D, dtype=bf16, device=dev),
                         v0=torch.randn(B * H, L, hdp, device=dev).to(bf16),
                         v0s=torch.empty(B * H, Ls, hdp, dtype=bf16, device=dev),
                         dv0=torch.zeros(B * H, L, hdp, dtype=f32, device=dev),
                         dv0s=torch.randn(B * H, Ls, hdp, device=dev)))
    turn = {"i": 0}

    def rot(fn):
        def run():
            turn["i"] = (turn["i"] + 1) % NBUF
            fn(sets[turn["i"]])
        return run
    row_x, row_v, row_g = 2 * D, 2 * hdp, 4 * hdp
    # bytes a call must move: the gather reads and writes Ls rows; the in-place merge reads Ls part rows and writes them;
    # the scatter-add reads Ls part rows, reads and writes Ls accumulator rows; plus the table
    legs = {
        "gather_X": (rot(lambda s: ops.rows_gather(s["X"], idx, out=s["Xs"])), 2 * B * Ls * row_x + 4 * Ls),
        "gather_v0": (rot(lambda s: ops.rows_gather(s["v0"], idx, out=s["v0s"])), 2 * B * H * Ls * row_v + 4 * Ls),
        "merge_X_in_place": (rot(lambda s: ops.rows_merge(s["X"], s["Xs"], inv)), 2 * B * Ls * row_x + 4 * L),
        "scatter_add_dv0": (rot(lambda s: ops.rows_scatter_add(s["dv0s"], s["dv0"], idx)), 3 * B * H * Ls * row_g + 4 * Ls),
    }
    run_legs({n: fn for n, (fn, _) in legs.items()}, 2, ROUNDS, ITERS)
    for n, (_, nbytes) in legs.items():
        rate = nbytes / (res[f"{n}_ms"] * 1e-3)
        res[f"{n}_bytes"] = nbytes
        res[f"{n}_hbm_fraction"] = round(rate / HBM_PEAK, 4)
        print(f"{n:24s}: {nbytes / 1e6:9.1f} MB -> {rate / 1e12:6.3f} TB/s = {rate / HBM_PEAK:.3f} of the HBM peak "
              "(rmsnorm_mod_fwd: 0.65)", flush=True)
    del sets
    torch.cuda.empty_cache()

if STEPS:
    from video_diffusion_speedrun_amd.optim import MuAdamW
    from video_diffusion_speedrun_amd.train import get_schedule, train_step
    gen = torch.Generator(device=dev).manual_seed(1234)
    torch.manual_seed(1234)
    batch = {"latent": torch.randn(B, *latent_shape, device=dev, generator=gen).to(bf16),
             "context": torch.randn(B, bench.LC, bench.CC, device=dev, generator=gen).to(bf16), "prompt": [""] * B}
    # ONE model (a C3b step peaks near 200 GB): the switch adds no parameter, the model reads it at every call
    model = bench.build_model(kw, dev, seed=1234)
    groups, _ = model.get_mup_setup(1e-4, 0.1, ["patch_proj", "context_kv", "positional_embedding"])
    opt = MuAdamW(groups, betas=(0.95, 0.99))
    sched = get_schedule(opt, "cosine", 20, 10000)

    def step(keep):
        def run():
            model.enable_token_routing(None) if keep is None else model.enable_token_routing(FIRST, LAST, keep)
            train_step(model, opt, sched, batch, dev, generator=gen)
        return run
    legs = {"step_off": step(None), **{f"step_{name(k)}": step(k) for k in KEEPS}}
    run_legs(legs, 2, STEPS, 1)
    for keep in KEEPS:
        r = res[f"step_{name(keep)}_ms"] / res["step_off_ms"]
        res[f"step_{name(keep)}_over_off"] = round(r, 4)
        res[f"step_{name(keep)}_flop_estimate"] = round(estimate(keep), 4)
        print(f"step_{name(keep)} / step_off = {r:.4f}   (FLOP estimate {estimate(keep):.4f}: time / estimate = "
              f"{r / estimate(keep):.3f})", flush=True)
    Lc = bench.LC
    for leg, fn in legs.items():  # memory: one more step per leg from a reset peak counter
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        keep = None if leg == "step_off" else KEEPS[list(legs).index(leg) - 1]
        kept = M.activation_bytes(model, B, latent_shape[1:], Lc, routing=None if keep is None else (FIRST, LAST, keep))["kept"]
        res[f"{leg}_peak_gb"], res[f"{leg}_resident_gb"], res[f"{leg}_activation_gb"] = (round(peak / 1e9, 3),
                                                                                          round(base / 1e9, 3),
                                                                                          round(kept / 1e9, 3))
        print(f"{leg:24s}: peak {peak / 1e9:8.3f} GB, {base / 1e9:.3f} GB resident before the step; activation_bytes kept "
              f"{kept / 1e9:8.3f} GB", flush=True)
    if CLASSES:
        for leg, fn in legs.items():
            torch.cuda.synchronize()
            ops.prof_enable()
            try:
                fn()
                torch.cuda.synchronize()
                stats = ops.prof_collect()
            finally:
                ops.prof_enable(0)
            res[f"{leg}_classes_ms"] = {k_: round(v["ms"], 3) for k_, v in stats.items()}
            total = sum(v["ms"] for v in stats.values())
            print(f"{leg}: {total:.1f} ms in profiled classes: " +
                  ", ".join(f"{k_} {v['ms']:.1f}" for k_, v in sorted(stats.items(), key=lambda kv: -kv[1]["ms"])), flush=True)
print(json.dumps(res))
