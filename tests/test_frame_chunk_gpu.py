"""Chunk-causal models on the GPU: DiT(frame_causal=True, frame_major=True, frame_chunk=2) on the tiny hd72 / hd64 cases of
tests/test_frame_causal_gpu.py (t = 3 token-frames: the chunks are frames (0, 1) and the short last chunk (2)) against the
helper model under the chunk mask (tests/helpers/frame_chunk_ref.py) at the bounds of the frame-major model tests (output
2.5e-2, loss 1e-2, worst gradient 3e-2); frame_chunk=1 against the frame_major model, bit for bit; causality over chunks on
the device, exactly, and visibility inside a chunk; recomputation bit for bit; GraphedTrainStep(frame_mode="chunk"); a cached
chunk call against the model's own full-sequence call; the cached against the uncached rollout; and the entry points a
model launches with and without the keyword."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_chunk_ref as CH  # noqa: E402
from test_frame_causal_gpu import (B_GRAD, B_LOSS, B_OUT, B_SAMPLER, CONST, START, TS, bits, build, model_case,  # noqa: E402
                                   reference_step, rel, step, within_bounds)

KC, R = CH.KC, CH.R
pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
CHUNK = 2
FLAGS = dict(frame_major=True, frame_chunk=CHUNK)


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


_refs = {}


def chunk_reference_step(name):
    """one fp32 step of the helper model under the chunk mask, once per case: the inputs of reference_step(name, True)"""
    if name not in _refs:
        cfg, P, latent, ctx, noise = model_case(name)
        base = reference_step(name, True)  # zt, v, ts, w: the same noising and weights
        Pg = {k: p.clone().requires_grad_(True) for k, p in P.items()}
        out = CH.dit_forward(Pg, cfg, base["zt"].float(), ctx.float(), base["ts"].float(), START, CHUNK)
        loss, _, _ = R.frame_loss(base["v"], out, base["w"], cfg.time_patch_size)
        loss.backward()
        _refs[name] = dict(out=out.detach(), loss=loss.item(), zt=base["zt"], v=base["v"], ts=base["ts"], w=base["w"],
                           grads={k: p.grad for k, p in Pg.items() if p.grad is not None})
    return _refs[name]


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_model_step_against_the_chunk_masked_reference(vds, name):
    cfg, P, latent, ctx, noise = model_case(name)
    ref, causal = chunk_reference_step(name), reference_step(name, True)
    # discrimination, on the CPU references alone: the frame-causal model is another model
    d_out = rel(causal["out"], ref["out"])
    print(f"{name}: chunk-masked vs frame-causal reference: out {d_out:.3f}")
    assert d_out >= 2 * B_OUT, d_out
    m = build(vds, cfg, P, **FLAGS)
    assert m.frame_chunk == CHUNK and all(b.frame_chunk == CHUNK for b in m.blocks)
    out, loss, grads = step(vds, m, ref["zt"], ref["v"], ctx, ref["ts"], ref["w"], cfg.time_patch_size)
    within_bounds(name + " frame_chunk=2", out, loss, grads, ref)
    # [B] timesteps run the chunk mask too
    t1 = ref["ts"][:, 1].contiguous()
    with torch.no_grad():
        o1 = m(ref["zt"].cuda(), ctx.cuda(), t1.cuda(), rope_start=START)
        r1 = CH.dit_forward(P, cfg, ref["zt"].float(), ctx.float(), t1.float(), START, CHUNK)
    assert rel(o1, r1) <= B_OUT, rel(o1, r1)


def test_frame_chunk_1_is_the_frame_major_model_bit_for_bit(vds, deterministic):
    cfg, P, latent, ctx, noise = model_case("hd72")
    ref = reference_step("hd72", True)
    args = (ref["zt"], ref["v"], ctx, ref["ts"], ref["w"], cfg.time_patch_size)
    out0, loss0, g0 = step(vds, build(vds, cfg, P, frame_major=True), *args)
    out1, loss1, g1 = step(vds, build(vds, cfg, P, frame_major=True, frame_chunk=1), *args)
    assert torch.equal(bits(out0), bits(out1)) and loss0 == loss1
    assert set(g0) == set(g1)
    for k in g0:
        assert torch.equal(bits(g0[k]), bits(g1[k])), k


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_model_is_causal_over_chunks_exactly_and_not_inside_one(vds, name):
    """registers pinned: other latents in the last chunk (token-frame 2) move the earlier chunk's output by exactly 0.0;
    other latents in token-frame 1 move token-frame 0, its own chunk's"""
    cfg, P, latent, ctx, noise = model_case(name)
    ts = torch.tensor(TS).to(bf16)
    reg = torch.tensor([1.0, 0.75])
    last, mid = latent.clone(), latent.clone()
    last[:, :, 4:] = (latent[:, :, 4:].float() + 3.0).to(bf16)
    mid[:, :, 2:4] = (latent[:, :, 2:4].float() + 3.0).to(bf16)
    m = build(vds, cfg, P, **FLAGS)
    with torch.no_grad():
        run = lambda x: m(x.cuda(), ctx.cuda(), ts.cuda(), rope_start=START, register_timesteps=reg)
        a, b, c = run(latent), run(last), run(mid)
    assert rel(b[:, :, 4:], a[:, :, 4:]) > 4 * B_OUT
    moved = (b[:, :, :4].float() - a[:, :, :4].float()).abs().max().item()
    inside = rel(c[:, :, :2], a[:, :, :2])
    print(f"{name}: the earlier chunk moves by {moved}; frame 0 moves by {inside:.3f} with its chunk's other frame")
    assert moved == 0.0
    assert inside > 2 * B_OUT, inside


def test_recompute_is_bit_identical(vds, deterministic):
    cfg, P, latent, ctx, noise = model_case("hd64")
    ref = chunk_reference_step("hd64")
    args = (ref["zt"], ref["v"], ctx, ref["ts"], ref["w"], cfg.time_patch_size)
    out0, _, g0 = step(vds, build(vds, cfg, P, "none", **FLAGS), *args)
    assert float(g0["blocks.0.qkv.weight"].abs().max()) > 0
    assert rel(out0, ref["out"]) <= B_OUT
    for mode in ("selective", "full"):
        out1, _, g1 = step(vds, build(vds, cfg, P, mode, **FLAGS), *args)
        assert torch.equal(bits(out0), bits(out1)), mode
        for k in g0:
            assert torch.equal(bits(g0[k]), bits(g1[k])), (mode, k)


def test_entry_points_with_and_without_the_keyword(vds, monkeypatch):
    """a frame_chunk=1 model and a model without the flag call none of the new entry points and pass no chunk to the
    attention calls; a frame_chunk=2 model runs every full-sequence self-attention through them"""
    cfg, P, latent, ctx, noise = model_case("hd72")
    ref = reference_step("hd72", True)
    ops, lib = vds["ops"], vds["lib"].load()
    seen, hits = [], []
    for name in ("vds_attn_fwd_causal_fm_chunk", "vds_attn_bwd_causal_fm_chunk"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _n=name: (hits.append(_n), _fn(*a))[1])
    for name in ("attn_fwd", "attn_bwd"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _fn=fn, _n=name, **k: (seen.append((_n, k.get("chunk"))), _fn(*a, **k))[1])
    args = (ref["zt"], ref["v"], ctx, ref["ts"], ref["w"], cfg.time_patch_size)
    for kw in (dict(frame_causal=False), dict(), dict(frame_major=True), dict(frame_major=True, frame_chunk=1)):
        del seen[:], hits[:]
        step(vds, build(vds, cfg, P, **kw), *args)
        assert seen and all(c is None for _, c in seen), (kw, seen)
        assert not hits, (kw, hits)
    del seen[:], hits[:]
    step(vds, build(vds, cfg, P, **FLAGS), *args)
    assert sorted(hits) == ["vds_attn_bwd_causal_fm_chunk"] * cfg.depth + ["vds_attn_fwd_causal_fm_chunk"] * cfg.depth
    assert [c for _, c in seen].count(CHUNK) == 2 * cfg.depth  # the self-attention calls; the cross-attention has none


@pytest.mark.parametrize("f0,k", [(0, 2), (2, 1)], ids=["first_chunk", "short_last_chunk"])
@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_a_cached_chunk_call_agrees_with_the_models_own_full_sequence_call(vds, name, f0, k):
    from test_frame_cache_gpu import BASE, REG, chunk_call
    from test_frame_cache_gpu import build as cache_build
    m = cache_build(vds, name, **FLAGS)
    _, _, latent, ctx = KC.model_case(name)
    cache = m.new_frame_cache(2, 3, 4, 4)
    for g0 in range(0, f0, CHUNK):  # the chunks before: one t = 0 call and one commit per chunk
        chunk_call(m, cache, latent, ctx, g0, CHUNK, torch.zeros(2, CHUNK, dtype=bf16))
        cache.commit()
    levels = torch.tensor(KC.T_CHUNK)[:, :k]
    out = chunk_call(m, cache, latent, ctx, f0, k, levels.to(bf16))
    torch.cuda.synchronize()
    assert cache.past_frames == f0 and cache.pending_frames == k
    ts = torch.ones(2, 3)
    ts[:, :f0] = 0
    ts[:, f0:f0 + k] = levels
    with torch.no_grad():
        full = m(latent.cuda(), ctx.cuda(), ts.to(bf16).cuda(), rope_start=BASE, register_timesteps=torch.tensor(REG))
    e = rel(out, full[:, :, 2 * f0:2 * (f0 + k)])
    # the helper's cached call, for the record (CPU-checked against the helper's full-sequence call to 1e-5)
    cfg, P, _, _ = KC.model_case(name)
    href, _ = CH.cached_chunk(P, cfg, latent, ctx, 3, CHUNK, f0, k, levels=KC.T_CHUNK)
    eh = rel(out, href)
    print(f"{name} frames {f0}..{f0 + k - 1}: cached vs full-sequence {e:.3e}, vs the helper {eh:.3e} (bound {B_OUT:.1e})")
    assert e <= B_OUT and eh <= B_OUT, (e, eh)
    if k == 2:  # the call runs ONE token group: frame f0 sees frame f0 + 1 (a frame-causal cached call would not)
        with torch.no_grad():
            causal = build(vds, *KC.model_case(name)[:2], frame_major=True)(
                latent.cuda(), ctx.cuda(), ts.to(bf16).cuda(), rope_start=BASE, register_timesteps=torch.tensor(REG))
        assert rel(out[:, :, :2], causal[:, :, 2 * f0:2 * f0 + 2]) > 2 * B_OUT


def test_cached_call_refusals_on_the_device(vds):
    from test_frame_cache_gpu import build as cache_build
    from test_frame_cache_gpu import chunk_call
    m = cache_build(vds, "hd64", **FLAGS)
    _, _, latent, ctx = KC.model_case("hd64")
    cache = m.new_frame_cache(2, 3, 4, 4)
    with pytest.raises(ValueError, match="ONE chunk"):
        chunk_call(m, cache, latent, ctx, 0, 3, torch.zeros(2, 3, dtype=bf16))
    with pytest.raises(ValueError, match="ONE chunk"):
        chunk_call(m, cache, latent, ctx, 0, 1, torch.zeros(2, 1, dtype=bf16))


def test_rollout_with_and_without_the_cache(vds):
    """4 token-frames, rollout_frames = frame_chunk = 2: two chunks of 3 steps.  The cached rollout against the uncached one
    with the same RoPE base in every call: the first chunk within one sampler budget (its registers sit at 1.0 in both)"""
    S = vds["sampling"]
    cfg, P, _, _, _ = model_case("hd72")
    g = torch.Generator().manual_seed(8)
    prompt = torch.randn(1, 12, 64, generator=g).to(bf16)
    lat0 = torch.randn(1, 16, 8, 8, 8, generator=g).to(bf16)
    m = build(vds, cfg, P, **FLAGS)
    base = (1, 2, 3)
    kw = dict(latents=lat0.cuda(), inference_steps=3, cfg_scale=4.0, rollout_frames=CHUNK)
    cached = S.generate_latents(m, prompt.cuda(), rope_starts=[base], kv_cache=True, **kw)
    unc = S.generate_latents(m, prompt.cuda(), rope_starts=[base] * 12, **kw)
    assert tuple(cached.shape) == tuple(unc.shape) == (1, 16, 8, 8, 8) and torch.isfinite(cached).all()
    c0 = rel(cached[:, :, :4], unc[:, :, :4])
    print(f"frame_chunk=2: cached vs uncached rollout, first chunk {c0:.3e} (bound {B_SAMPLER:.1e})")
    assert c0 <= B_SAMPLER, c0
    # the conditioning prefill of the cached rollout: one call and one commit per chunk
    cond = lat0[:, :, :4]
    pre = S.generate_latents(m, prompt.cuda(), rope_starts=[base], kv_cache=True, cond_latents=cond.cuda(), **kw)
    assert torch.equal(pre[:, :, :4].cpu(), cond.float()) and torch.isfinite(pre).all()
    with pytest.raises(ValueError, match="multiple of 2"):
        S.generate_latents(m, prompt.cuda(), rope_starts=[base], **dict(kw, rollout_frames=1))


def test_graph_replay_matches_eager(vds):
    """GraphedTrainStep(frame_mode="chunk") on a frame_chunk=2 model, the way tests/test_frame_major_gpu.py runs the
    "first_frame" mode; 4 token-frames: two chunks, one noise level each"""
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
        m = build(vds, cfg, P, **FLAGS)
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
