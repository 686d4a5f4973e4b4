"""Frame-major models on the GPU: DiT(frame_causal=True, frame_major=True) against the masked helper reference
(tests/helpers/frame_causal_ref.py) at the bounds tests/test_frame_causal_gpu.py uses for the interleaved model (output
2.5e-2, loss 1e-2, worst gradient 3e-2), and against the interleaved device model within the sum of the two bounds (the
triangle inequality); causality on the device, exactly; recomputation bit for bit; composition with qk_norm, residual_v,
context_lens, [B, t] timesteps and GraphedTrainStep; a checkpoint from one layout in the other; a cached chunk call; and
the entry points a model launches with and without the keyword."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_causal_ref as FC  # noqa: E402
from test_frame_causal_gpu import (B_GRAD, B_LOSS, B_OUT, CONST, START, TS, bits, build, model_case,  # noqa: E402
                                   reference_step, rel, step, within_bounds)

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import model, ops, optim, sampling, train
    return dict(model=model, ops=ops, optim=optim, train=train, sampling=sampling)


@pytest.fixture
def deterministic(vds, request):
    vds["ops"].set_deterministic(True, 256 << 20)
    request.addfinalizer(lambda: vds["ops"].set_deterministic(False))


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_model_step_against_the_masked_reference_and_the_interleaved_model(vds, name):
    cfg, P, latent, ctx, noise = model_case(name)  # residual_v=True: v_0 and its gradient travel in frame-major rows
    ref = reference_step(name, True)
    args = (ref["zt"], ref["v"], ctx, ref["ts"], ref["w"], cfg.time_patch_size)
    m = build(vds, cfg, P, frame_major=True)
    assert m.frame_major and all(b.frame_major for b in m.blocks)
    out, loss, grads = step(vds, m, *args)
    within_bounds(name + " frame_major", out, loss, grads, ref)
    # the interleaved device model: both are within the bounds of the reference, so within their sum of each other
    out_i, loss_i, grads_i = step(vds, build(vds, cfg, P), *args)
    d_out, d_loss = rel(out, out_i), abs(loss - loss_i) / abs(loss_i)
    worst = max((rel(grads[k], grads_i[k]), k) for k in grads if float(grads_i[k].abs().max()) > 0
                and not k.endswith("lambda_param"))
    print(f"{name}: frame_major vs interleaved on the device: out {d_out:.3e}, loss {d_loss:.2e}, worst grad {worst}")
    assert d_out <= 2 * B_OUT and d_loss <= 2 * B_LOSS and worst[0] <= 2 * B_GRAD
    # [B] timesteps run the frame-major kernels too
    t1 = ref["ts"][:, 1].contiguous()
    with torch.no_grad():
        o1 = m(ref["zt"].cuda(), ctx.cuda(), t1.cuda(), rope_start=START)
        r1 = FC.dit_forward(P, cfg, ref["zt"].float(), ctx.float(), t1.float(), START)
    assert rel(o1, r1) <= B_OUT, rel(o1, r1)


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_model_is_causal_over_frames_exactly(vds, name):
    """other latents in the last token-frame: the output of the earlier frames moves by exactly 0.0"""
    cfg, P, latent, ctx, noise = model_case(name)
    ts = torch.tensor(TS).to(bf16)
    other = latent.clone()
    other[:, :, 4:] = (latent[:, :, 4:].float() + 3.0).to(bf16)
    m = build(vds, cfg, P, frame_major=True)
    with torch.no_grad():
        a = m(latent.cuda(), ctx.cuda(), ts.cuda(), rope_start=START)
        b = m(other.cuda(), ctx.cuda(), ts.cuda(), rope_start=START)
    assert rel(b[:, :, 4:], a[:, :, 4:]) > 4 * B_OUT
    moved = (b[:, :, :4].float() - a[:, :, :4].float()).abs().max().item()
    print(f"{name}: earlier frames move by {moved}")
    assert moved == 0.0


def test_recompute_is_bit_identical(vds, deterministic):
    cfg, P, latent, ctx, noise = model_case("hd64")
    ref = reference_step("hd64", True)
    args = (ref["zt"], ref["v"], ctx, ref["ts"], ref["w"], cfg.time_patch_size)
    out0, _, g0 = step(vds, build(vds, cfg, P, "none", frame_major=True), *args)
    assert float(g0["blocks.0.qkv.weight"].abs().max()) > 0
    for mode in ("selective", "full"):
        out1, _, g1 = step(vds, build(vds, cfg, P, mode, frame_major=True), *args)
        assert torch.equal(bits(out0), bits(out1)), mode
        for k in g0:
            assert torch.equal(bits(g0[k]), bits(g1[k])), (mode, k)


def test_composes_with_qk_norm_and_context_lens(vds):
    cfg, P, latent, ctx, noise = model_case("hd72")
    lens = [24, 7]
    ref = reference_step("hd72", True, qk_norm=True, context_lens=lens)
    m = build(vds, cfg, P, qk_norm=True, frame_major=True)
    out, loss, grads = step(vds, m, ref["zt"], ref["v"], ctx, ref["ts"], ref["w"], cfg.time_patch_size, context_lens=lens)
    within_bounds("frame_major qk_norm+context_lens", out, loss, grads, ref)


def test_checkpoints_cross_the_layouts(vds):
    """no parameter is added: the state dict of one layout loads strictly into the other, identical"""
    cfg, P, latent, ctx, noise = model_case("hd64")
    a, b = build(vds, cfg, P, frame_major=True), build(vds, cfg, P)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    b.load_state_dict(sa, strict=True)
    a.load_state_dict(sb, strict=True)
    for k in sa:
        assert torch.equal(a.state_dict()[k], b.state_dict()[k]), k
    with pytest.raises(ValueError, match="frame_causal=True"):
        build(vds, cfg, P, frame_causal=False, frame_major=True)


def test_entry_points_with_and_without_the_keyword(vds, monkeypatch):
    """without the keyword a frame_causal model and a plain model launch what they launched before: no frames reach the
    qkv / RoPE calls and frame_major never reaches the attention calls; with it every self-attention call is frame-major"""
    cfg, P, latent, ctx, noise = model_case("hd72")
    ref = reference_step("hd72", True)
    ops, seen = vds["ops"], []

    def spy(name):
        fn = getattr(ops, name)

        def wrapped(*a, **k):
            seen.append((name, k.get("frames"), bool(k.get("frame_major", False)), a[0].shape[2] == a[1].shape[2]
                         if name.startswith("attn") else True))
            return fn(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)
    for n in ("attn_fwd", "attn_bwd", "qkv_rope_fwd", "qkv_rope_bwd", "qkv_rope_norm_fwd", "qkv_rope_norm_bwd"):
        spy(n)
    args = (ref["zt"], ref["v"], ctx, ref["ts"], ref["w"], cfg.time_patch_size)
    for kw in (dict(frame_causal=False), dict()):
        del seen[:]
        step(vds, build(vds, cfg, P, **kw), *args)
        assert seen and not any(fm for _, _, fm, _ in seen), seen
        assert all(fr is None for n, fr, _, _ in seen if n.startswith("qkv_rope")), seen
    del seen[:]
    step(vds, build(vds, cfg, P, frame_major=True), *args)
    rope = [s for s in seen if s[0].startswith("qkv_rope")]
    selfs = [s for s in seen if s[0].startswith("attn") and s[3]]
    cross = [s for s in seen if s[0].startswith("attn") and not s[3]]
    assert len(rope) == 2 * cfg.depth and all(fr == (16, 3) for _, fr, _, _ in rope), seen
    assert len(selfs) == 2 * cfg.depth and all(fr == (16, 3) and fm for _, fr, fm, _ in selfs), seen
    assert len(cross) == 2 * cfg.depth and not any(fm or fr for _, fr, fm, _ in cross), seen


def test_a_cached_chunk_agrees_with_the_models_own_full_sequence_call(vds):
    """DiT.forward(frame_cache=) on a frame_major model runs the cache kernels (their own key order); its result agrees
    with the model's own frame-major full-sequence call within the bound of tests/test_frame_cache_gpu.py"""
    import frame_cache_ref as KC
    from test_frame_cache_gpu import BASE, REG, cached
    from test_frame_cache_gpu import build as cache_build
    name, f0, k = "hd72", 1, 2
    m = cache_build(vds, name, frame_major=True)
    _, _, latent, ctx = KC.model_case(name)
    out, _ = cached(m, name, f0, k)
    ts = torch.ones(2, 3)
    ts[:, :f0] = 0
    ts[:, f0:f0 + k] = torch.tensor(KC.T_CHUNK)[:, :k]
    with torch.no_grad():
        full = m(latent.cuda(), ctx.cuda(), ts.to(bf16).cuda(), rope_start=BASE, register_timesteps=torch.tensor(REG))
    e = rel(out, full[:, :, 2 * f0:2 * (f0 + k)])
    print(f"frame_major: cached vs full-sequence {e:.3e} (bound {B_OUT:.1e})")
    assert e <= B_OUT, e


def test_graph_replay_matches_eager(vds):
    """GraphedTrainStep(frame_mode="first_frame") on a frame_major model, as tests/test_frame_causal_gpu.py runs it"""
    from oracle import dit_oracle as O
    from video_diffusion_speedrun_amd.graph import GraphedTrainStep
    cfg = O.DiTConfig(in_channels=16, hidden_size=128, depth=3, num_heads=2, cross_attn_input_size=64,
                      residual_v=True, train_bias_and_rms=False)
    P = O.init_params(cfg, seed=41, randomize_zero_init=True, init_std_factor=1.0)
    g = torch.Generator().manual_seed(5)
    batches = [{"latent": torch.randn(2, 16, 4, 8, 8, generator=g).cuda(), "context": torch.randn(2, 16, 64, generator=g).cuda(),
                "prompt": ["", ""]} for _ in range(5)]
    results = []
    for graphed in (False, True):
        m = build(vds, cfg, P, frame_major=True)
        groups, _ = m.get_mup_setup(3e-3, 0.1, CONST)
        opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99))
        sched = vds["train"].get_schedule(opt, "cosine", 3, 50)
        torch.manual_seed(77)
        torch.cuda.manual_seed(77)
        losses = []
        if graphed:
            gs = GraphedTrainStep(m, opt, sched, "cuda", eager_steps=2, frame_mode="first_frame")
            for b in batches:
                losses.append(gs.step(b).item())
            assert gs.n_replays == 3 and opt._step == 5
        else:
            for b in batches:
                losses.append(vds["train"].train_step(m, opt, sched, b, "cuda", frame_mode="first_frame").item())
        torch.cuda.synchronize()
        results.append((losses, {k: v.clone() for k, v in m.full_state_dict().items()}))
    (l0, p0), (l1, p1) = results
    assert len(set(l0)) == 5
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    for k in p0:
        assert rel(p1[k], p0[k]) <= 2e-4, (k, rel(p1[k], p0[k]))


def test_rollout_with_and_without_the_cache(vds):
    """generate_latents(rollout_frames=) on a frame_major model: the uncached rollout against the helper loop at the bounds
    of tests/test_frame_causal_gpu.py (the whole result within two sampler budgets, the first token-frame within one), and
    the cached rollout against the uncached one as tests/test_frame_cache_gpu.py compares them: the same base in every
    rope_starts entry, the first token-frame within one sampler budget"""
    from test_frame_causal_gpu import B_SAMPLER, SCALE, STARTS, STEPS, rollout_inputs
    S = vds["sampling"]
    cfg, P, _, _, _ = model_case("hd72")
    prompt, lat0, _ = rollout_inputs()
    m = build(vds, cfg, P, frame_major=True)
    kw = dict(latents=lat0.cuda(), inference_steps=STEPS, cfg_scale=SCALE, rollout_frames=1)
    acc = S.generate_latents(m, prompt.cuda(), rope_starts=STARTS, **kw)
    ref = FC.rollout_loop(P, cfg, lat0, prompt, torch.zeros_like(prompt), STEPS, SCALE, STARTS, 1)
    e, e0 = rel(acc, ref), rel(acc[:, :, :2], ref[:, :, :2])
    print(f"frame_major rollout: rel err {e:.3e} (first token-frame {e0:.3e}), bound {2 * B_SAMPLER:.1e}")
    assert e <= 2 * B_SAMPLER and e0 <= B_SAMPLER, (e, e0)
    base = (1, 2, 3)
    cached = S.generate_latents(m, prompt.cuda(), rope_starts=[base], kv_cache=True, **kw)
    unc = S.generate_latents(m, prompt.cuda(), rope_starts=[base] * 12, **kw)
    assert tuple(cached.shape) == tuple(unc.shape) and torch.isfinite(cached).all()
    c0 = rel(cached[:, :, :2], unc[:, :, :2])
    print(f"frame_major: cached vs uncached rollout, first token-frame {c0:.3e} (bound {B_SAMPLER:.1e})")
    assert c0 <= B_SAMPLER, c0
