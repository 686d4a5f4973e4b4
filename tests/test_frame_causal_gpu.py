"""Frame-causal models on the GPU: DiT(frame_causal=True) against the masked helper reference
(tests/helpers/frame_causal_ref.py) on the tiny configurations, inputs, TS, START and bounds of
tests/test_frame_timesteps_gpu.py (output 2.5e-2, loss 1e-2, worst gradient 3e-2); causality of the model on the device;
recomputation, qk_norm + context_lens, graph replay; the sampler's frame rollout against the helper loop."""
import os
import sys

import pytest
import torch

from oracle import dit_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_causal_ref as FC  # noqa: E402
from qk_norm_ref import qk_normed_oracle  # noqa: E402

R = FC.R
pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
CONST = ["patch_proj", "context_kv", "positional_embedding"]
B_OUT, B_LOSS, B_GRAD = 2.5e-2, 1e-2, 3e-2
B_SAMPLER = 1.5e-2  # test_sampler_holds_the_conditioning_frames: one 3-step pass of the sampler against its helper loop


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


def rel(a, b):
    a, b = a.float().cpu().flatten(), b.float().cpu().flatten()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


def build(vds, cfg, P, mode="none", frame_causal=True, **kw):
    m = vds["model"].DiT(in_channels=cfg.in_channels, patch_size=cfg.patch_size, time_patch_size=cfg.time_patch_size,
                         hidden_size=cfg.hidden_size, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
                         cross_attn_input_size=cfg.cross_attn_input_size, residual_v=cfg.residual_v,
                         train_bias_and_rms=cfg.train_bias_and_rms, frame_causal=frame_causal, **kw)
    m.load_state_dict(P, strict=True)
    return m.to("cuda").enable_recompute(mode)


TS = [[0.0, 0.5, 0.96875], [0.9375, 0.25, 0.0625]]
START = (2, 3, 4)
_cases = {}


def model_case(name):
    """cfg, parameters (both time_embed weights x 8) and inputs: latent [2,16,6,8,8] with (pt, p) = (2, 2), so t = 3 and
    L = 64; context [2,24,64]"""
    if name in _cases:
        return _cases[name]
    if name == "hd72":
        cfg = O.DiTConfig(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=144, depth=2, num_heads=2,
                          cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False)
        seed = 3
    else:
        cfg = O.DiTConfig(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=128, depth=3, num_heads=2,
                          cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False)
        seed = 13
    P = O.init_params(cfg, seed=seed, randomize_zero_init=True, init_std_factor=1.0)
    P["time_embed.0.weight"] = P["time_embed.0.weight"] * 8
    P["time_embed.2.weight"] = P["time_embed.2.weight"] * 8
    g = torch.Generator().manual_seed(seed + 1)
    latent = torch.randn(2, 16, 6, 8, 8, generator=g).to(bf16)
    ctx = torch.randn(2, 24, 64, generator=g).to(bf16)
    noise = torch.randn(2, 16, 6, 8, 8, generator=g).to(bf16)
    _cases[name] = (cfg, P, latent, ctx, noise)
    return _cases[name]


_refs = {}


def reference_step(name, frame_causal, qk_norm=False, context_lens=None):
    """one fp32 step of the helper reference, once per case: per-frame timesteps TS, the frame-weighted loss"""
    key = (name, frame_causal, qk_norm, None if context_lens is None else tuple(context_lens))
    if key in _refs:
        return _refs[key]
    cfg, P, latent, ctx, noise = model_case(name)
    ts = torch.tensor(TS).to(bf16)
    w = (ts > 0).float()
    zt, v = R.noise_frames(latent, noise, ts, cfg.time_patch_size)
    Pg = {k: p.clone().requires_grad_(True) for k, p in P.items()}
    if qk_norm:
        with qk_normed_oracle():
            out = FC.dit_forward(Pg, cfg, zt.float(), ctx.float(), ts.float(), START, frame_causal, context_lens)
    else:
        out = FC.dit_forward(Pg, cfg, zt.float(), ctx.float(), ts.float(), START, frame_causal, context_lens)
    loss, _, _ = R.frame_loss(v, out, w, cfg.time_patch_size)
    loss.backward()
    _refs[key] = dict(out=out.detach(), loss=loss.item(), zt=zt, v=v, ts=ts, w=w,
                      grads={k: p.grad for k, p in Pg.items() if p.grad is not None})
    return _refs[key]


def step(vds, m, zt, v, ctx, ts, w, pt, **kw):
    m.zero_grad()
    out = m(zt.cuda(), ctx.cuda(), ts.cuda(), rope_start=START, **kw)
    loss, _ = vds["train"].frame_flow_loss(out, v.cuda(), w.cuda(), pt)
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().clone(), loss.item(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def within_bounds(tag, out, loss, grads, ref):
    e_out = rel(out, ref["out"])
    e_loss = abs(loss - ref["loss"]) / abs(ref["loss"])
    worst = max((rel(grads[k], ref["grads"][k]), k) for k in grads
                if k in ref["grads"] and not k.endswith("lambda_param") and float(ref["grads"][k].abs().max()) > 0)
    print(f"{tag}: out rel err {e_out:.3e}, loss rel {e_loss:.2e}, worst grad rel err {worst[0]:.3e} ({worst[1]})")
    assert torch.isfinite(out.float()).all()
    assert e_out <= B_OUT and e_loss <= B_LOSS, (e_out, e_loss)
    assert worst[0] <= B_GRAD, worst
    return e_out, e_loss, worst


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_model_step_against_the_masked_reference(vds, name, parity_log):
    cfg, P, latent, ctx, noise = model_case(name)
    ref, plain = reference_step(name, True), reference_step(name, False)
    # discrimination, on the CPU references alone: the unmasked model is >= 4 x the output bound and >= 2.5 x the gradient
    # bound away (closest of the weight gradients named below)
    d_out = rel(plain["out"], ref["out"])
    keys = [k for k in ref["grads"] if k.startswith("blocks.") and
            k.endswith(("qkv.weight", "attn_proj.weight", "cross_proj.weight", "mlp.0.weight"))]
    d_grad = min((rel(plain["grads"][k], ref["grads"][k]), k) for k in keys)
    print(f"{name}: masked vs unmasked reference: out {d_out:.3f}, closest gradient {d_grad}")
    assert d_out >= 4 * B_OUT and d_grad[0] >= 2.5 * B_GRAD, (d_out, d_grad)
    m = build(vds, cfg, P)
    out, loss, grads = step(vds, m, ref["zt"], ref["v"], ctx, ref["ts"], ref["w"], cfg.time_patch_size)
    e_out, e_loss, worst = within_bounds(name, out, loss, grads, ref)
    parity_log(f"frame_causal_model_{name}", out=e_out, loss=e_loss, worst_grad=worst[0], worst_grad_name=worst[1],
               ref_distance_out=d_out, ref_distance_grad=d_grad[0])
    # [B] timesteps run the masked kernels too
    t1 = ref["ts"][:, 1].contiguous()
    with torch.no_grad():
        o1 = m(ref["zt"].cuda(), ctx.cuda(), t1.cuda(), rope_start=START)
        r1 = FC.dit_forward(P, cfg, ref["zt"].float(), ctx.float(), t1.float(), START)
    assert rel(o1, r1) <= B_OUT, rel(o1, r1)


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_model_is_causal_over_frames_on_the_device(vds, name):
    """two forwards whose inputs differ only in the latents of the last token-frame: the outputs of the earlier frames
    agree within the output bound on a frame_causal model and are >= 4 x the bound apart on a plain one"""
    cfg, P, latent, ctx, noise = model_case(name)
    ts = torch.tensor(TS).to(bf16)
    other = latent.clone()
    other[:, :, 4:] = (latent[:, :, 4:].float() + 3.0).to(bf16)  # (the fp32 references: 0.171 / 0.187 apart without the mask)
    moved = {}
    with torch.no_grad():
        for causal in (True, False):
            m = build(vds, cfg, P, frame_causal=causal)
            a = m(latent.cuda(), ctx.cuda(), ts.cuda(), rope_start=START)
            b = m(other.cuda(), ctx.cuda(), ts.cuda(), rope_start=START)
            moved[causal] = rel(b[:, :, :4], a[:, :, :4])
            assert rel(b[:, :, 4:], a[:, :, 4:]) > 4 * B_OUT
    print(f"{name}: earlier frames move by {moved[True]:.3e} with frame_causal, {moved[False]:.3f} without")
    assert moved[True] <= B_OUT, moved
    assert moved[False] >= 4 * B_OUT, moved


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_a_loss_on_frame_0_sends_no_gradient_through_later_frames(vds, name):
    """DiT.forward returns no input gradient, so the check is on the patch embedding: with a loss that weights frame 0
    only, its weight gradient sums dX over the rows of frame 0 (and the register rows, whose patches are zero) alone, so
    it is the same -- within the gradient bound -- when the later frames hold other latents.  On a plain model it is not."""
    cfg, P, latent, ctx, noise = model_case(name)
    ts = torch.tensor(TS).to(bf16)
    w = torch.zeros(2, 3)
    w[:, 0] = 1
    other = latent.clone()
    other[:, :, 2:] = torch.randn(2, 16, 4, 8, 8, generator=torch.Generator().manual_seed(98)).to(bf16)
    key = "patch_embed.patch_proj.weight"
    moved = {}
    for causal in (True, False):
        m = build(vds, cfg, P, frame_causal=causal)
        _, _, ga = step(vds, m, latent, latent, ctx, ts, w, cfg.time_patch_size)
        _, _, gb = step(vds, m, other, latent, ctx, ts, w, cfg.time_patch_size)
        assert float(ga[key].abs().max()) > 0
        moved[causal] = rel(gb[key], ga[key])
    print(f"{name}: patch-embed gradient moves by {moved[True]:.3e} with frame_causal, {moved[False]:.3f} without")
    assert moved[True] <= B_GRAD, moved
    assert moved[False] >= 2.5 * B_GRAD, moved


def test_recompute_is_bit_identical(vds, deterministic):
    cfg, P, latent, ctx, noise = model_case("hd64")
    ref = reference_step("hd64", True)
    args = (ref["zt"], ref["v"], ctx, ref["ts"], ref["w"], cfg.time_patch_size)
    out0, _, g0 = step(vds, build(vds, cfg, P, "none"), *args)
    assert float(g0["blocks.0.qkv.weight"].abs().max()) > 0
    for mode in ("selective", "full"):
        out1, _, g1 = step(vds, build(vds, cfg, P, mode), *args)
        assert torch.equal(bits(out0), bits(out1)), mode
        for k in g0:
            assert torch.equal(bits(g0[k]), bits(g1[k])), (mode, k)


def test_composes_with_qk_norm_and_context_lens(vds):
    cfg, P, latent, ctx, noise = model_case("hd72")
    lens = [24, 7]
    ref = reference_step("hd72", True, qk_norm=True, context_lens=lens)
    m = build(vds, cfg, P, qk_norm=True)
    out, loss, grads = step(vds, m, ref["zt"], ref["v"], ctx, ref["ts"], ref["w"], cfg.time_patch_size, context_lens=lens)
    within_bounds("qk_norm+context_lens", out, loss, grads, ref)


def test_a_plain_model_launches_no_masked_kernel(vds, monkeypatch):
    cfg, P, latent, ctx, noise = model_case("hd72")
    ref = reference_step("hd72", True)
    ops, seen = vds["ops"], []
    fwd, bwd = ops.attn_fwd, ops.attn_bwd
    monkeypatch.setattr(ops, "attn_fwd", lambda *a, **k: (seen.append(("fwd", a[0].shape[2], a[1].shape[2], k.get("frames"))), fwd(*a, **k))[1])
    monkeypatch.setattr(ops, "attn_bwd", lambda *a, **k: (seen.append(("bwd", a[0].shape[2], a[1].shape[2], k.get("frames"))), bwd(*a, **k))[1])
    args = (ref["zt"], ref["v"], ctx, ref["ts"], ref["w"], cfg.time_patch_size)
    step(vds, build(vds, cfg, P, frame_causal=False), *args)
    assert seen and all(fr is None for _, _, _, fr in seen), seen
    del seen[:]
    step(vds, build(vds, cfg, P), *args)
    selfs = [s for s in seen if s[1] == s[2]]
    cross = [s for s in seen if s[1] != s[2]]
    assert len(selfs) == 2 * cfg.depth and all(fr == (16, 3) for _, _, _, fr in selfs), seen
    assert len(cross) == 2 * cfg.depth and all(fr is None for _, _, _, fr in cross), seen


def test_fp8_linears_with_masked_bf16_attention(vds):
    """enable_fp8(attention=False) on a frame_causal model: [B] timesteps run, [B, t] timesteps stay refused"""
    cfg, P, latent, ctx, noise = model_case("hd72")
    m = build(vds, cfg, P).enable_fp8(attention=False)
    t1 = torch.tensor([0.5, 0.25]).to(bf16)
    with torch.no_grad():
        out = m(latent.cuda(), ctx.cuda(), t1.cuda(), rope_start=START)
        r1 = FC.dit_forward(P, cfg, latent.float(), ctx.float(), t1.float(), START)
        r0 = FC.dit_forward(P, cfg, latent.float(), ctx.float(), t1.float(), START, frame_causal=False)
    assert torch.isfinite(out.float()).all()
    e1, e0 = rel(out, r1), rel(out, r0)
    print(f"fp8 linears + masked attention: {e1:.3e} from the masked reference, {e0:.3e} from the unmasked one")
    # e4m3 operands carry 2^-4 relative rounding per element, so no bf16 bound applies: the output has to sit on the
    # masked reference's side of the two, which are >= 4 x the output bound apart
    assert rel(r0, r1) >= 4 * B_OUT and e1 < e0, (e1, e0)
    with pytest.raises(NotImplementedError, match="per-frame timesteps"):
        m(latent.cuda(), ctx.cuda(), torch.tensor(TS).cuda(), rope_start=START)


def test_graph_replay_matches_eager(vds):
    """GraphedTrainStep(frame_mode="first_frame") on a frame_causal model: two eager steps, capture, three replays against
    five eager steps with the same seeds, within the bounds the graph tests use (losses 1e-4, parameters 2e-4 relative)"""
    from video_diffusion_speedrun_amd.graph import GraphedTrainStep
    cfg = O.DiTConfig(in_channels=16, hidden_size=128, depth=3, num_heads=2, cross_attn_input_size=64,
                      residual_v=True, train_bias_and_rms=False)
    P = O.init_params(cfg, seed=41, randomize_zero_init=True, init_std_factor=1.0)
    g = torch.Generator().manual_seed(5)
    batches = [{"latent": torch.randn(2, 16, 4, 8, 8, generator=g).cuda(), "context": torch.randn(2, 16, 64, generator=g).cuda(),
                "prompt": ["", ""]} for _ in range(5)]
    results = []
    for graphed in (False, True):
        m = build(vds, cfg, P)
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
    print("graph frame_causal: worst loss rel", max(abs(a - b) / abs(a) for a, b in zip(l0, l1)),
          "worst param rel", max(rel(p1[k], p0[k]) for k in p0))
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    for k in p0:
        assert rel(p1[k], p0[k]) <= 2e-4, (k, rel(p1[k], p0[k]))


# --------------------------------------------------------------------------------------- rollout ----
STEPS, SCALE = 3, 4.0
STARTS = [(1, 2, 3), (1, 2, 3), (4, 5, 6), (4, 5, 6), (7, 8, 9), (7, 8, 9),
          (2, 1, 3), (2, 1, 3), (5, 4, 6), (5, 4, 6), (8, 7, 9), (8, 7, 9)]  # 2 chunks x 3 steps x the guided pair


def rollout_inputs():
    g = torch.Generator().manual_seed(8)
    prompt = torch.randn(1, 12, 64, generator=g).to(bf16)
    lat0 = torch.randn(1, 16, 4, 8, 8, generator=g).to(bf16)
    lat1 = lat0.clone()
    lat1[:, :, 2:] = torch.randn(1, 16, 2, 8, 8, generator=g).to(bf16)  # other initial noise in the second token-frame
    return prompt, lat0, lat1


def test_rollout_against_the_helper_loop(vds, parity_log):
    """a [1,16,4,8,8] latent = 2 token-frames, rollout_frames=1: 2 chunks of 3 steps.  A later chunk starts from the earlier
    chunk's result, so the bound is one 3-step sampler budget (1.5e-2) per chunk."""
    S = vds["sampling"]
    cfg, P, _, _, _ = model_case("hd72")
    prompt, lat0, lat1 = rollout_inputs()
    m = build(vds, cfg, P)
    kw = dict(inference_steps=STEPS, cfg_scale=SCALE, rope_starts=STARTS, rollout_frames=1)
    acc = S.generate_latents(m, prompt.cuda(), latents=lat0.cuda(), **kw)
    assert acc.dtype == f32 and tuple(acc.shape) == (1, 16, 4, 8, 8) and torch.isfinite(acc).all()
    ref = FC.rollout_loop(P, cfg, lat0, prompt, torch.zeros_like(prompt), STEPS, SCALE, STARTS, 1)
    e = rel(acc, ref)
    e0 = rel(acc[:, :, :2], ref[:, :, :2])
    print(f"rollout: rel err {e:.3e} (first token-frame {e0:.3e}), bound {2 * B_SAMPLER:.1e}")
    parity_log("frame_causal_rollout", rel_err=e, first_frame=e0)
    assert e <= 2 * B_SAMPLER and e0 <= B_SAMPLER, (e, e0)
    # a finished chunk does not depend on the noise of later frames -- on a frame_causal model
    acc1 = S.generate_latents(m, prompt.cuda(), latents=lat1.cuda(), **kw)
    d_causal = rel(acc1[:, :, :2], acc[:, :, :2])
    assert rel(acc1[:, :, 2:], acc[:, :, 2:]) > 4 * B_SAMPLER
    mp = build(vds, cfg, P, frame_causal=False)
    pa = S.generate_latents(mp, prompt.cuda(), latents=lat0.cuda(), **kw)
    pb = S.generate_latents(mp, prompt.cuda(), latents=lat1.cuda(), **kw)
    d_plain = rel(pb[:, :, :2], pa[:, :, :2])
    print(f"rollout: other noise in frame 1 moves frame 0 by {d_causal:.3e} (frame_causal), {d_plain:.3f} (plain)")
    assert d_causal <= B_SAMPLER, d_causal
    assert d_plain > 4 * B_SAMPLER, d_plain


def test_rollout_off_is_the_plain_loop(vds):
    """one chunk that holds every frame runs the plain loop's calls with constant [B, t] rows, which give the bits of the
    [B] call: the rollout's bookkeeping adds nothing of its own.  (rollout_frames=None takes the same path as leaving the
    argument out; that comparison only pins the default.)"""
    S = vds["sampling"]
    cfg, P, _, _, _ = model_case("hd72")
    prompt, lat0, _ = rollout_inputs()
    m = build(vds, cfg, P)
    kw = dict(inference_steps=STEPS, cfg_scale=SCALE, rope_starts=STARTS[:6])
    base = S.generate_latents(m, prompt.cuda(), latents=lat0.cuda(), **kw)
    none = S.generate_latents(m, prompt.cuda(), latents=lat0.cuda(), rollout_frames=None, **kw)
    one = S.generate_latents(m, prompt.cuda(), latents=lat0.cuda(), rollout_frames=2, **kw)
    assert torch.equal(bits(base), bits(none))
    assert torch.equal(bits(base), bits(one))
    with pytest.raises(ValueError, match="rollout_frames"):
        S.generate_latents(m, prompt.cuda(), latents=lat0.cuda(), rollout_frames=0, **kw)
