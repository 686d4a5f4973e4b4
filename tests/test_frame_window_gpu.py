"""Sliding-window models on the GPU: DiT(frame_causal=True, frame_major=True, frame_chunk=c, frame_window=w) on the tiny
hd72 / hd64 configurations of tests/test_frame_causal_gpu.py with t = 4 token-frames, (c, w) = (1, 2) and (2, 2), against the
helper model under the window mask (tests/helpers/frame_window_ref.py) at the bounds of the frame-major model tests (output
2.5e-2, loss 1e-2, worst gradient 3e-2); frames outside the last chunk's reach leave its output bit-identical; recomputation
bit for bit; the entry points a model launches with and without the keyword; GraphedTrainStep; a ring-cached rollout that
wraps (t = 5, c = 1, w = 2) against the model's own full-sequence call at every chunk, and the sampler's cached against its
uncached rollout; the ring cache's byte size."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_chunk_ref as CH  # noqa: E402
import frame_window_ref as FW  # noqa: E402
from test_frame_causal_gpu import (B_GRAD, B_LOSS, B_OUT, B_SAMPLER, CONST, START, bits, build, model_case,  # noqa: E402
                                   rel, step, within_bounds)

KC, R = FW.KC, FW.R
pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
TS4 = [[0.0, 0.5, 0.96875, 0.25], [0.9375, 0.25, 0.0625, 0.5]]
CW = [(1, 2), (2, 2)]
cw_ids = [f"c{c}_w{w}" for c, w in CW]


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import _lib, model, ops, optim, sampling, train
    return dict(model=model, ops=ops, optim=optim, train=train, sampling=sampling, lib=_lib)


@pytest.fixture
def deterministic(vds, request):
    vds["ops"].set_deterministic(True, 256 << 20)
    request.addfinalizer(lambda: vds["ops"].set_deterministic(False))


_cases, _refs = {}, {}


def case4(name):
    """model_case(name)'s configuration, parameters and context with a latent of t = 4 token-frames: [2,16,8,8,8], L = 80"""
    if name not in _cases:
        cfg, P, _, ctx, _ = model_case(name)
        g = torch.Generator().manual_seed(900 + len(name) + cfg.depth)
        latent = torch.randn(2, 16, 8, 8, 8, generator=g).to(bf16)
        noise = torch.randn(2, 16, 8, 8, 8, generator=g).to(bf16)
        ts = torch.tensor(TS4).to(bf16)
        zt, v = R.noise_frames(latent, noise, ts, cfg.time_patch_size)
        _cases[name] = dict(cfg=cfg, P=P, ctx=ctx, latent=latent, zt=zt, v=v, ts=ts, w=(ts > 0).float())
    return _cases[name]


def reference_step(name, c, w):
    """one fp32 step of the helper model, once per case; w = None: the chunk mask without a window"""
    key = (name, c, w)
    if key not in _refs:
        cs = case4(name)
        Pg = {k: p.clone().requires_grad_(True) for k, p in cs["P"].items()}
        if w is None:
            out = CH.dit_forward(Pg, cs["cfg"], cs["zt"].float(), cs["ctx"].float(), cs["ts"].float(), START, c)
        else:
            out = FW.dit_forward(Pg, cs["cfg"], cs["zt"].float(), cs["ctx"].float(), cs["ts"].float(), START, c, w)
        loss, _, _ = R.frame_loss(cs["v"], out, cs["w"], cs["cfg"].time_patch_size)
        loss.backward()
        _refs[key] = dict(out=out.detach(), loss=loss.item(), grads={k: p.grad for k, p in Pg.items() if p.grad is not None})
    return _refs[key]


def flags(c, w):
    return dict(frame_major=True, frame_chunk=c, frame_window=w)


def args_of(cs):
    return (cs["zt"], cs["v"], cs["ctx"], cs["ts"], cs["w"], cs["cfg"].time_patch_size)


@pytest.mark.parametrize("c,w", CW, ids=cw_ids)
@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_model_step_against_the_window_masked_reference(vds, name, c, w):
    cs = case4(name)
    ref, chunked = reference_step(name, c, w), reference_step(name, c, None)
    d_out = rel(chunked["out"], ref["out"])  # discrimination, on the CPU references alone
    print(f"{name} c={c} w={w}: window-masked vs chunk-masked reference: out {d_out:.3f}")
    assert d_out >= 2 * B_OUT, d_out
    m = build(vds, cs["cfg"], cs["P"], **flags(c, w))
    assert m.frame_window == w and all(b.frame_window == w for b in m.blocks)
    out, loss, grads = step(vds, m, *args_of(cs))
    within_bounds(f"{name} frame_chunk={c} frame_window={w}", out, loss, grads, ref)
    t1 = cs["ts"][:, 1].contiguous()  # [B] timesteps run the window mask too
    with torch.no_grad():
        o1 = m(cs["zt"].cuda(), cs["ctx"].cuda(), t1.cuda(), rope_start=START)
        r1 = FW.dit_forward(cs["P"], cs["cfg"], cs["zt"].float(), cs["ctx"].float(), t1.float(), START, c, w)
    assert rel(o1, r1) <= B_OUT, rel(o1, r1)


def test_a_window_of_every_frame_is_the_model_without_one_bit_for_bit(vds, deterministic):
    cs = case4("hd72")
    out0, loss0, g0 = step(vds, build(vds, cs["cfg"], cs["P"], frame_major=True, frame_chunk=2), *args_of(cs))
    out1, loss1, g1 = step(vds, build(vds, cs["cfg"], cs["P"], **flags(2, 4)), *args_of(cs))
    assert torch.equal(bits(out0), bits(out1)) and loss0 == loss1 and set(g0) == set(g1)
    for k in g0:
        assert torch.equal(bits(g0[k]), bits(g1[k])), k


@pytest.mark.parametrize("name,c,w,frames", [("hd72", 2, 2, (0, 1)), ("hd64", 2, 2, (0, 1)), ("hd72", 1, 2, (0,))],
                         ids=["hd72_c2_w2", "hd64_c2_w2", "hd72_c1_w2"])
def test_frames_outside_the_last_chunks_reach_leave_it_bit_identical(vds, name, c, w, frames):
    """registers pinned.  (2, 2): the last chunk (frames 2, 3) attends itself and the registers in every block, so other
    latents in chunk 0 move it by exactly 0.0 at any depth.  (1, 2) at depth 2: frame 3 attends frames 2 and 3, whose block-0
    outputs read frames 1 .. 3 -- frame 0 is outside its reach, and frame 1, which it reaches through frame 2 only, still moves
    it.  Frame 2, which the last chunk attends itself, moves it far beyond the model bound."""
    cs = case4(name)
    pt = cs["cfg"].time_patch_size
    assert not (c == 1 and cs["cfg"].depth != 2)
    ts = torch.tensor(TS4).to(bf16)
    reg = torch.tensor([1.0, 0.75])
    far, near = cs["latent"].clone(), cs["latent"].clone()
    for f in frames:
        far[:, :, f * pt:(f + 1) * pt] = (cs["latent"][:, :, f * pt:(f + 1) * pt].float() + 3.0).to(bf16)
    f_in = 2  # a frame the last chunk attends
    near[:, :, f_in * pt:(f_in + 1) * pt] = (cs["latent"][:, :, f_in * pt:(f_in + 1) * pt].float() + 3.0).to(bf16)
    last = slice((4 - c) * pt, 4 * pt)
    m = build(vds, cs["cfg"], cs["P"], **flags(c, w))
    with torch.no_grad():
        run = lambda x: m(x.cuda(), cs["ctx"].cuda(), ts.cuda(), rope_start=START, register_timesteps=reg)
        a, b, d = run(cs["latent"]), run(far), run(near)
    moved = (b[:, :, last].float() - a[:, :, last].float()).abs().max().item()
    inside = rel(d[:, :, last], a[:, :, last])
    print(f"{name} c={c} w={w}: the last chunk moves by {moved} (frames {frames}), by {inside:.3f} (frame {f_in})")
    assert rel(b[:, :, :pt], a[:, :, :pt]) > 4 * B_OUT  # the edited frame itself moved
    assert moved == 0.0
    assert inside > 2 * B_OUT, inside
    if c == 1:  # the edge of the reach: frame 1, two blocks away
        edge = cs["latent"].clone()
        edge[:, :, pt:2 * pt] = (cs["latent"][:, :, pt:2 * pt].float() + 3.0).to(bf16)
        with torch.no_grad():
            e = run(edge)
        assert not torch.equal(bits(e[:, :, last]), bits(a[:, :, last]))


def test_recompute_is_bit_identical(vds, deterministic):
    cs = case4("hd64")
    ref = reference_step("hd64", 1, 2)
    out0, _, g0 = step(vds, build(vds, cs["cfg"], cs["P"], "none", **flags(1, 2)), *args_of(cs))
    assert float(g0["blocks.0.qkv.weight"].abs().max()) > 0
    assert rel(out0, ref["out"]) <= B_OUT
    for mode in ("selective", "full"):
        out1, _, g1 = step(vds, build(vds, cs["cfg"], cs["P"], mode, **flags(1, 2)), *args_of(cs))
        assert torch.equal(bits(out0), bits(out1)), mode
        for k in g0:
            assert torch.equal(bits(g0[k]), bits(g1[k])), (mode, k)


def test_entry_points_with_and_without_the_keyword(vds, monkeypatch):
    """a model without frame_window calls none of the new entry points and passes no window to the attention calls; a
    frame_window model runs every full-sequence self-attention through them, with the window in chunks"""
    cs = case4("hd72")
    ops, lib = vds["ops"], vds["lib"].load()
    seen, hits = [], []
    for name in ("vds_attn_fwd_causal_fm_window", "vds_attn_bwd_causal_fm_window"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _n=name: (hits.append(_n), _fn(*a))[1])
    for name in ("attn_fwd", "attn_bwd"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name,
                            lambda *a, _fn=fn, _n=name, **k: (seen.append((_n, "window" in k, k.get("window"))), _fn(*a, **k))[1])
    for kw in (dict(frame_causal=False), dict(), dict(frame_major=True), dict(frame_major=True, frame_chunk=2),
               dict(frame_major=True, frame_window=None)):
        del seen[:], hits[:]
        step(vds, build(vds, cs["cfg"], cs["P"], **kw), *args_of(cs))
        assert seen and not any(has for _, has, _ in seen), (kw, seen)
        assert not hits, (kw, hits)
    depth = cs["cfg"].depth
    del seen[:], hits[:]
    step(vds, build(vds, cs["cfg"], cs["P"], **flags(2, 2)), *args_of(cs))
    assert sorted(hits) == ["vds_attn_bwd_causal_fm_window"] * depth + ["vds_attn_fwd_causal_fm_window"] * depth
    assert [wd for _, _, wd in seen].count(1) == 2 * depth  # W = 2 // 2 chunks; the cross-attention passes none


# ---------------------------------------------------------------------------------------- ring ----
_long = {}


def long_inputs(name, frames):
    if (name, frames) not in _long:
        _, _, _, ctx = KC.model_case(name)
        g = torch.Generator().manual_seed(31 + frames)
        _long[(name, frames)] = (torch.randn(2, 16, 2 * frames, 8, 8, generator=g).to(bf16), ctx)
    return _long[(name, frames)]


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_a_ring_cached_rollout_that_wraps_agrees_with_the_full_sequence_call_at_every_chunk(vds, name):
    """t = 5, c = 1, w = 2: two slots, chunks 2, 3 and 4 overwrite a slot; every chunk at its noise levels against the
    model's own windowed full-sequence call (earlier frames at t = 0, later ones at 1), then committed at t = 0"""
    from test_frame_cache_gpu import BASE, REG, chunk_call
    from test_frame_cache_gpu import build as cache_build
    frames = 5
    m = cache_build(vds, name, **flags(1, 2))
    latent, ctx = long_inputs(name, frames)
    cache = m.new_frame_cache(2, frames, 4, 4)
    assert cache.k[0].shape[2] == FW.N_REG + 2 * 16
    levels = torch.tensor(KC.T_CHUNK)[:, :1]
    worst = 0.0
    for f0 in range(frames):
        out = chunk_call(m, cache, latent, ctx, f0, 1, levels.to(bf16))
        ts = torch.ones(2, frames)
        ts[:, :f0] = 0
        ts[:, f0:f0 + 1] = levels
        with torch.no_grad():
            full = m(latent.cuda(), ctx.cuda(), ts.to(bf16).cuda(), rope_start=BASE, register_timesteps=torch.tensor(REG))
        e = rel(out, full[:, :, 2 * f0:2 * f0 + 2])
        worst = max(worst, e)
        assert torch.isfinite(out.float()).all() and e <= B_OUT, (f0, e)
        chunk_call(m, cache, latent, ctx, f0, 1, torch.zeros(2, 1, dtype=bf16))
        cache.commit()
    assert cache.past_frames == frames
    print(f"{name}: ring-cached vs full-sequence call over {frames} chunks, worst {worst:.3e} (bound {B_OUT:.1e})")
    # the helper's ring, for the record (CPU-checked against the helper's full-sequence call to 1e-5): the last chunk
    cfg, P, _, _ = KC.model_case(name)
    href = FW.ring_rollout(P, cfg, latent, ctx, frames, 1, 2, [float(levels[0, 0]), float(levels[1, 0])])[-1]
    assert rel(out, href) <= B_OUT, rel(out, href)
    # and the unbounded cache of the model without a window is another model by then
    with torch.no_grad():
        other = cache_build(vds, name, frame_major=True)(latent.cuda(), ctx.cuda(), ts.to(bf16).cuda(), rope_start=BASE,
                                                        register_timesteps=torch.tensor(REG))
    assert rel(other[:, :, 2 * (frames - 1):], full[:, :, 2 * (frames - 1):]) > 1e-3


def test_rollout_with_and_without_the_cache(vds):
    """5 token-frames, rollout_frames = 1 on a (c, w) = (1, 2) model: five chunks of 3 steps through two slots.  The cached
    rollout against the uncached one with the same RoPE base in every call: the first chunk within one sampler budget (its
    registers sit at 1.0 in both)"""
    S = vds["sampling"]
    cfg, P, _, _, _ = model_case("hd72")
    g = torch.Generator().manual_seed(8)
    prompt = torch.randn(1, 12, 64, generator=g).to(bf16)
    lat0 = torch.randn(1, 16, 10, 8, 8, generator=g).to(bf16)
    m = build(vds, cfg, P, **flags(1, 2))
    base = (1, 2, 3)
    kw = dict(latents=lat0.cuda(), inference_steps=3, cfg_scale=4.0, rollout_frames=1)
    cached = S.generate_latents(m, prompt.cuda(), rope_starts=[base], kv_cache=True, **kw)
    unc = S.generate_latents(m, prompt.cuda(), rope_starts=[base] * 30, **kw)
    assert tuple(cached.shape) == tuple(unc.shape) == (1, 16, 10, 8, 8) and torch.isfinite(cached).all()
    c0 = rel(cached[:, :, :2], unc[:, :, :2])
    print(f"frame_window=2: cached vs uncached rollout, first chunk {c0:.3e} (bound {B_SAMPLER:.1e})")
    assert c0 <= B_SAMPLER, c0
    # the conditioning prefill: one call and one commit per chunk, three frames through two slots
    cond = lat0[:, :, :6]
    pre = S.generate_latents(m, prompt.cuda(), rope_starts=[base], kv_cache=True, cond_latents=cond.cuda(), **kw)
    assert torch.equal(pre[:, :, :6].cpu(), cond.float()) and torch.isfinite(pre).all()
    with pytest.raises(ValueError, match="pass rollout_frames=1"):
        S.generate_latents(m, prompt.cuda(), rope_starts=[base], kv_cache=True, **dict(kw, rollout_frames=2))


def test_the_ring_caches_byte_size(vds):
    cfg, P, _, _, _ = model_case("hd72")
    m = build(vds, cfg, P, **flags(2, 4))
    plain = build(vds, cfg, P, frame_major=True, frame_chunk=2)
    size = lambda c: sum(t.numel() * t.element_size() for t in c.k + c.v)
    for frames in (4, 16, 64):
        ring = m.new_frame_cache(2, frames, 4, 4)
        assert size(ring) == 2 * cfg.depth * 2 * cfg.num_heads * (FW.N_REG + 4 * 16) * 96 * 2
        assert size(plain.new_frame_cache(2, frames, 4, 4)) == 2 * cfg.depth * 2 * cfg.num_heads * (FW.N_REG + frames * 16) * 96 * 2


def test_graph_replay_matches_eager(vds):
    """GraphedTrainStep on a frame_window model (the window travels by value): eager and captured steps agree"""
    from oracle import dit_oracle as O
    from video_diffusion_speedrun_amd.graph import GraphedTrainStep
    cfg = O.DiTConfig(in_channels=16, hidden_size=128, depth=3, num_heads=2, cross_attn_input_size=64,
                      residual_v=True, train_bias_and_rms=False)
    P = O.init_params(cfg, seed=41, randomize_zero_init=True, init_std_factor=1.0)
    g = torch.Generator().manual_seed(5)
    batches = [{"latent": torch.randn(2, 16, 8, 8, 8, generator=g).cuda(), "context": torch.randn(2, 16, 64, generator=g).cuda(),
                "prompt": ["", ""]} for _ in range(5)]
    results = []
    for graphed in (False, True):
        m = build(vds, cfg, P, **flags(2, 2))
        groups, _ = m.get_mup_setup(3e-3, 0.1, CONST)
        opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99))
        sched = vds["train"].get_schedule(opt, "cosine", 3, 50)
        torch.manual_seed(77)
        torch.cuda.manual_seed(77)
        losses = []
        if graphed:
            gs = GraphedTrainStep(m, opt, sched, "cuda", eager_steps=2, frame_mode="chunk")
            for b in batches:
                losses.append(gs.step(b).item())
            assert gs.n_replays == 3 and opt._step == 5
        else:
            for b in batches:
                losses.append(vds["train"].train_step(m, opt, sched, b, "cuda", frame_mode="chunk").item())
        torch.cuda.synchronize()
        results.append((losses, {k: v.clone() for k, v in m.full_state_dict().items()}))
    (l0, p0), (l1, p1) = results
    assert len(set(l0)) == 5
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    for k in p0:
        assert rel(p1[k], p0[k]) <= 2e-4, (k, rel(p1[k], p0[k]))
