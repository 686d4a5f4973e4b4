"""Teacher-forcing self-attention (vds_teacher_attn_fwd / _bwd) on one MI355X, legs alternated inside one process.

Kernel legs (lead 16, S = 1024 rows per frame, n = 8 frames, 16 heads of 72 in the ones layout, B samples):
  tf_c1, tf_c2   the TF kernels on L = 16 + 16 * 1024 rows ([lead | 8 clean | 8 noisy frames]), frame_chunk 1 / 2
  fm_c1, fm_c2   yardstick: the chunk-causal frame-major call (vds_attn_*_causal_fm[_chunk]) on the same 16 + 16 * 1024 rows
  plain          yardstick: the unmasked call on L = 16 + 8 * 1024 rows
Every leg is timed per kernel through the library's profiler (HIP event pairs around each launch, ops.prof_collect), and
every time is also given per VISITED (query, key) pair: the pairs are the profiler's FLOP credit divided by the FLOPs of one
pair, and for the TF legs they are checked against tests/helpers/teacher_ref.py (pairs_q / pairs_k).  Median (min .. max)
over ROUNDS samples of ITERS calls.

Step legs (STEPS > 0): one C3b train step with frame_mode="teacher" at B_STEP samples against frame_mode="chunk" at
2 * B_STEP samples -- the same number of token rows -- on a frame_causal, frame_major model with frame_chunk = CHUNK.
One JSON line at the end.  KERNELS=0 skips the kernel legs, STEPS=0 the step legs."""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import torch  # noqa: E402

import bench  # noqa: E402
from video_diffusion_speedrun_amd import ops  # noqa: E402

bf16, f32 = torch.bfloat16, torch.float32
B = int(os.environ.get("B", 2))
ROUNDS, ITERS, WARM = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("ITERS", 2)), 1
STEPS, KERNELS = int(os.environ.get("STEPS", 3)), int(os.environ.get("KERNELS", 1))
B_STEP, CHUNK = int(os.environ.get("B_STEP", 6)), int(os.environ.get("CHUNK", 2))
dev = "cuda"
H, hd, hdp = 16, 72, 96
D = H * hd
LEAD, S, N = 16, 1024, 8
res = {"B": B, "H": H, "head_dim": hd, "lead": LEAD, "S": S, "n": N, "rounds": ROUNDS, "iters": ITERS}

KINDS = (("fwd", "attn_fwd"), ("dq", "attn_bwd_dq"), ("dkv", "attn_bwd_dkv"), ("delta", "attn_bwd_delta"))


def kind_of(cls):
    for kind, prefix in reversed(KINDS):
        if cls.lower().startswith(prefix):
            return kind
    return None


def buffers(L, frames):
    g = torch.Generator(device=dev).manual_seed(L)
    qkv = torch.randn(B * L, 3 * D, device=dev, generator=g).to(bf16)
    cos = torch.ones(L, hd // 2, dtype=f32, device=dev)
    sin = torch.zeros(L, hd // 2, dtype=f32, device=dev)
    fkw = {} if frames is None else {"frames": frames}
    q, k, v = ops.qkv_rope_fwd(qkv, cos, sin, None, None, B, L, H, hd, hdp, **fkw)
    o = torch.empty(B * L, D, dtype=bf16, device=dev)
    do = torch.randn(B * L, D, device=dev, generator=g).to(bf16)
    lse = torch.empty(B, H, L, dtype=f32, device=dev)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    delta = torch.empty(ops.attn_bwd_workspace_floats(B, H, L, L, hd, True), dtype=f32, device=dev)
    return dict(q=q, k=k, v=v, ov=ops.heads_view(o, B, L, H, hd), dov=ops.heads_view(do, B, L, H, hd), lse=lse, dq=dq, dk=dk,
                dv=dv, delta=delta, o=o, do=do)


def leg(buf, **kw):
    def run():
        b = buf
        ops.attn_fwd(b["q"][..., :hd], b["k"][..., :hd], b["v"][..., :hd], b["ov"], b["lse"], kv_pad_ones=True, **kw)
        ops.attn_bwd(b["q"][..., :hd], b["k"][..., :hd], b["v"][..., :hd], b["ov"], b["lse"], b["dov"], b["dq"][..., :hd],
                     b["dk"][..., :hd], b["dv"][..., :hd], b["delta"], kv_pad_ones=True, **kw)
    return run


def profiled(fn, iters):
    """-> {kind: (ms per call, FLOP credit per call)}"""
    ops.prof_enable()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    out = {}
    for cls, st in ops.prof_collect().items():
        kind = kind_of(cls)
        if kind is None or not st["launches"]:
            continue
        ms, fl = out.get(kind, (0.0, 0.0))
        out[kind] = (ms + st["ms"] / iters, fl + st["flops"] / iters)
    ops.prof_enable(0)
    return out


if KERNELS:
    import teacher_ref as TR
    L2, L1 = LEAD + 2 * N * S, LEAD + N * S
    big_tf = buffers(L2, (LEAD, 2 * N))
    small = buffers(L1, None)
    legs = {"tf_c1": leg(big_tf, frames=(LEAD, 2 * N), frame_major=True, chunk=1, teacher=True),
            "tf_c2": leg(big_tf, frames=(LEAD, 2 * N), frame_major=True, chunk=2, teacher=True),
            "fm_c1": leg(big_tf, frames=(LEAD, 2 * N), frame_major=True),
            "fm_c2": leg(big_tf, frames=(LEAD, 2 * N), frame_major=True, chunk=2),
            "plain": leg(small)}
    for fn in legs.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in legs}
    for _ in range(ROUNDS):  # the legs alternate, so that clock and neighbour drift hits all of them alike
        for name, fn in legs.items():
            samples[name].append(profiled(fn, ITERS))
    per_pair = {"fwd": 4.0 * B * H * hd, "dq": 4.0 * B * H * hd, "dkv": 4.0 * B * H * hd}  # FLOPs credited per visited pair
    for name, xs in samples.items():
        for kind in ("fwd", "dq", "dkv"):
            ms = [x[kind][0] for x in xs if kind in x]
            if not ms:
                continue
            pairs = xs[0][kind][1] / per_pair[kind]
            med = statistics.median(ms)
            res[f"{name}_{kind}_ms"] = round(med, 4)
            res[f"{name}_{kind}_min_max_ms"] = [round(min(ms), 4), round(max(ms), 4)]
            res[f"{name}_{kind}_pairs"] = pairs
            res[f"{name}_{kind}_ps_per_pair"] = round(med * 1e9 / (pairs * B * H), 4)
            print(f"{name:6s} {kind:4s}: median {med:9.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}); {pairs:.4e} visited pairs "
                  f"per head, {med * 1e9 / (pairs * B * H):.3f} ps per pair and head", flush=True)
    for c in (1, 2):  # the profiler's credit of the TF legs is the reference's count of the visited tiles
        shape = TR.shape_of(N, S, c)
        want_q, want_k = TR.pairs_q(*shape), TR.pairs_k(*shape)
        got_q, got_k = res[f"tf_c{c}_fwd_pairs"], res[f"tf_c{c}_dkv_pairs"]
        vis, tot = TR.tiles_visited(*shape)
        res[f"tf_c{c}_key_tiles_visited"] = [vis, tot]
        print(f"tf_c{c}: pairs credited {got_q:.0f} / {got_k:.0f}, teacher_ref {want_q} / {want_k}; forward / dQ visit {vis} of "
              f"{tot} key tiles", flush=True)
        assert got_q == want_q and got_k == want_k and res[f"tf_c{c}_dq_pairs"] == want_q, "the profiler's credit is off"
    del big_tf, small
    torch.cuda.empty_cache()

if STEPS:
    from video_diffusion_speedrun_amd.optim import MuAdamW
    from video_diffusion_speedrun_amd.train import get_schedule, train_step
    kw, latent_shape = dict(bench.WORKLOADS["c3b"][0]), bench.WORKLOADS["c3b"][1]
    gen = torch.Generator(device=dev).manual_seed(1234)
    torch.manual_seed(1234)
    model = bench.build_model(kw, dev, seed=1234)
    for m in [model] + list(model.blocks):  # no flag adds a parameter: the blocks read their flags at every call
        m.frame_causal, m.frame_major, m.frame_chunk = True, True, CHUNK
    groups, _ = model.get_mup_setup(1e-4, 0.1, ["patch_proj", "context_kv", "positional_embedding"])
    opt = MuAdamW(groups, betas=(0.95, 0.99))
    sched = get_schedule(opt, "cosine", 20, 10000)

    def batch(b):
        return {"latent": torch.randn(b, *latent_shape, device=dev, generator=gen).to(bf16),
                "context": torch.randn(b, bench.LC, bench.CC, device=dev, generator=gen).to(bf16), "prompt": [""] * b}
    b_t, b_c = batch(B_STEP), batch(2 * B_STEP)
    legs = {"step_teacher": lambda: train_step(model, opt, sched, b_t, dev, generator=gen, frame_mode="teacher"),
            "step_chunk": lambda: train_step(model, opt, sched, b_c, dev, generator=gen, frame_mode="chunk")}
    times = {name: [] for name in legs}
    for fn in legs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(STEPS):
        for name, fn in legs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e))
    for name, xs in times.items():
        res[f"{name}_ms"] = round(statistics.median(xs), 3)
        res[f"{name}_min_max_ms"] = [round(min(xs), 3), round(max(xs), 3)]
        print(f"{name}: median {statistics.median(xs):.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})", flush=True)
    res["step_teacher_over_chunk"] = round(res["step_teacher_ms"] / res["step_chunk_ms"], 4)
print(json.dumps(res))
