"""Frame KV cache on the GPU: DiT.forward(frame_cache=) against the helper's cached call and against the device's own
full-sequence frame_causal call (tests/helpers/frame_cache_ref.py), on the tiny configurations and bounds of
tests/test_frame_causal_gpu.py (one model call 2.5e-2, one 3-step sampler pass 1.5e-2); what a cached call may and may not
read; register_timesteps; the sampler's cached rollout against the helper loop and against the uncached rollout."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_cache_ref as KC  # noqa: E402

FC, R = KC.FC, KC.R
pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
B_OUT, B_LOSS, B_GRAD = 2.5e-2, 1e-2, 3e-2
B_SAMPLER = 1.5e-2
BASE, REG = KC.BASE, KC.REG
HW = 16  # tokens per frame of the tiny case


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import model, ops, sampling, train
    return dict(model=model, ops=ops, train=train, sampling=sampling)


def rel(a, b):
    a, b = a.float().cpu().flatten(), b.float().cpu().flatten()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


_models = {}


def build(vds, name, frame_causal=True, **kw):
    key = (name, frame_causal, tuple(sorted(kw.items())))
    if key not in _models:
        cfg, P, _, _ = KC.model_case(name)
        m = vds["model"].DiT(in_channels=cfg.in_channels, patch_size=cfg.patch_size, time_patch_size=cfg.time_patch_size,
                             hidden_size=cfg.hidden_size, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
                             cross_attn_input_size=cfg.cross_attn_input_size, residual_v=cfg.residual_v,
                             train_bias_and_rms=cfg.train_bias_and_rms, frame_causal=frame_causal, **kw)
        m.load_state_dict(P, strict=True)
        _models[key] = m.to("cuda")
    return _models[key]


def chunk_call(m, cache, latent, ctx, f0, k, ts, **kw):
    """the model on token-frames f0 .. f0 + k - 1 (f0 = cache.past_frames) at the noise levels ts [2, k]"""
    assert cache.past_frames == f0
    with torch.no_grad():
        return m(latent[:, :, 2 * f0:2 * (f0 + k)].cuda(), ctx.cuda(), ts.cuda(), rope_start=(BASE[0] + f0, BASE[1], BASE[2]),
                 register_timesteps=torch.tensor(REG), frame_cache=cache, **kw)


def cached(m, name, f0, k, **kw):
    """a fresh cache, frames 0 .. f0 - 1 committed through t = 0 calls (one per frame), then the chunk at KC.T_CHUNK"""
    _, _, latent, ctx = KC.model_case(name)
    cache = m.new_frame_cache(2, 3, 4, 4)
    for f in range(f0):
        chunk_call(m, cache, latent, ctx, f, 1, torch.zeros(2, 1, dtype=bf16), **kw)
        cache.commit()
    out = chunk_call(m, cache, latent, ctx, f0, k, torch.tensor(KC.T_CHUNK)[:, :k].to(bf16), **kw)
    torch.cuda.synchronize()
    return out, cache


IDS = [f"f{f}_k{k}" for f, k in KC.CHUNKS]


@pytest.mark.parametrize("f0,k", KC.CHUNKS, ids=IDS)
@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_chunk_against_the_helper(vds, name, f0, k, parity_log):
    m = build(vds, name)
    out, cache = cached(m, name, f0, k)
    assert out.dtype == bf16 and tuple(out.shape) == (2, 16, 2 * k, 8, 8) and torch.isfinite(out.float()).all()
    assert cache.past_frames == f0 and cache.pending_frames == k
    ref, _ = KC.chunk_reference(name, f0, k)
    e = rel(out, ref)
    print(f"{name} frames {f0}..{f0 + k - 1}: cached call vs helper {e:.3e} (bound {B_OUT:.1e})")
    parity_log(f"frame_cache_chunk_{name}_f{f0}_k{k}", out=e)
    assert e <= B_OUT, e
    if f0:  # (CPU-checked: the helper without the past is > 4 x B_OUT away)
        assert rel(out, KC.chunk_reference(name, f0, k, use_past=False)[0]) > 2 * B_OUT


@pytest.mark.parametrize("f0,k", KC.CHUNKS, ids=IDS)
@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_cached_against_the_full_sequence_call_on_the_device(vds, name, f0, k, parity_log):
    """the device's own full-sequence frame_causal call with the registers pinned, earlier frames at 0, later frames at 1,
    restricted to the chunk's frames"""
    m = build(vds, name)
    _, _, latent, ctx = KC.model_case(name)
    out, _ = cached(m, name, f0, k)
    ts = torch.ones(2, 3)
    ts[:, :f0] = 0
    ts[:, f0:f0 + k] = torch.tensor(KC.T_CHUNK)[:, :k]
    with torch.no_grad():
        full = m(latent.cuda(), ctx.cuda(), ts.to(bf16).cuda(), rope_start=BASE, register_timesteps=torch.tensor(REG))
    e = rel(out, full[:, :, 2 * f0:2 * (f0 + k)])
    print(f"{name} frames {f0}..{f0 + k - 1}: cached vs full-sequence on the device {e:.3e} (bound {B_OUT:.1e})")
    parity_log(f"frame_cache_vs_full_{name}_f{f0}_k{k}", out=e)
    assert e <= B_OUT, e


def test_composes_with_qk_norm_and_context_lens(vds):
    lens = [24, 7]
    m = build(vds, "hd72", qk_norm=True)
    out, _ = cached(m, "hd72", 1, 2, context_lens=lens)
    ref, _ = KC.chunk_reference("hd72", 1, 2, qk_norm=True, context_lens=lens)
    e = rel(out, ref)
    print(f"qk_norm + context_lens: cached call vs helper {e:.3e}")
    assert e <= B_OUT, e
    plain, _ = KC.chunk_reference("hd72", 1, 2)
    assert rel(plain, ref) > 4 * B_OUT  # (the two options do change the result)


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_a_cached_call_reads_the_past_rows_only(vds, name):
    """a call on frame 1 is unmoved -- exactly -- by what the buffers hold outside the 16 committed rows: the register rows
    and its own rows are written before they are read, the rows behind them are never read"""
    m = build(vds, name)
    _, _, latent, ctx = KC.model_case(name)
    ts = torch.tensor(KC.T_CHUNK)[:, :1].to(bf16)
    _, cache = cached(m, name, 1, 1)
    a = chunk_call(m, cache, latent, ctx, 1, 1, ts)
    for buf in cache.k + cache.v:
        keep = buf[:, :, 16:16 + HW].clone()
        buf.fill_(float("nan"))
        buf[:, :, 16:16 + HW] = keep
    b = chunk_call(m, cache, latent, ctx, 1, 1, ts)
    torch.cuda.synchronize()
    assert torch.isfinite(b.float()).all()
    assert torch.equal(bits(a), bits(b))
    assert all(torch.isnan(buf[:, :, 16 + 2 * HW:].float()).all() for buf in cache.k + cache.v)  # nothing written behind


def test_commit_copies_nothing(vds):
    m = build(vds, "hd72")
    _, _, latent, ctx = KC.model_case("hd72")
    _, cache = cached(m, "hd72", 1, 1)
    ptrs = [t.data_ptr() for t in cache.k + cache.v]
    rows = [t[:, :, :16 + 2 * HW].clone() for t in cache.k + cache.v]
    cache.commit()
    torch.cuda.synchronize()
    assert cache.past_frames == 2 and cache.pending_frames == 0
    assert ptrs == [t.data_ptr() for t in cache.k + cache.v]
    assert all(torch.equal(bits(r), bits(t[:, :, :16 + 2 * HW])) for r, t in zip(rows, cache.k + cache.v))
    with pytest.raises(RuntimeError, match="commit"):
        cache.commit()
    out = chunk_call(m, cache, latent, ctx, 2, 1, torch.tensor(KC.T_CHUNK)[:, :1].to(bf16))  # finds both frames in place
    assert torch.isfinite(out.float()).all() and cache.pending_frames == 1
    cache.reset()
    assert cache.past_frames == 0 and ptrs == [t.data_ptr() for t in cache.k + cache.v]


def test_without_a_frame_cache_no_new_kernel_is_launched(vds, monkeypatch):
    m = build(vds, "hd72")
    cfg, _, latent, ctx = KC.model_case("hd72")
    ops, seen, cache_rope = vds["ops"], [], []
    fwd, rc, rcn = ops.attn_fwd, ops.qkv_rope_fwd_cache, ops.qkv_rope_norm_fwd_cache
    monkeypatch.setattr(ops, "attn_fwd", lambda *a, **k: (seen.append((a[0].shape[2], a[1].shape[2], k.get("frames"), k.get("past", 0))), fwd(*a, **k))[1])
    monkeypatch.setattr(ops, "qkv_rope_fwd_cache", lambda *a, **k: (cache_rope.append(1), rc(*a, **k))[1])
    monkeypatch.setattr(ops, "qkv_rope_norm_fwd_cache", lambda *a, **k: (cache_rope.append(1), rcn(*a, **k))[1])
    ts = torch.tensor(FC_TS).to(bf16)
    with torch.no_grad():
        m(latent.cuda(), ctx.cuda(), ts.cuda(), rope_start=BASE)
        m(latent.cuda(), ctx.cuda(), ts.cuda(), rope_start=BASE, register_timesteps=torch.tensor(REG))
    m.zero_grad()
    m(latent.cuda(), ctx.cuda(), ts.cuda(), rope_start=BASE, register_timesteps=torch.tensor(REG)).float().sum().backward()
    assert seen and not cache_rope and all(p == 0 for _, _, _, p in seen), seen
    del seen[:]
    cached(m, "hd72", 1, 2)
    selfs = [s for s in seen if s[2] is not None]
    assert len(cache_rope) == 2 * cfg.depth
    assert selfs == [(16 + HW, 16 + HW, (16, 1), 0)] * cfg.depth + [(16 + 2 * HW, 16 + 3 * HW, (16, 2), HW)] * cfg.depth, seen
    assert all(p == 0 for _, _, fr, p in seen if fr is None)


FC_TS = [[0.0, 0.5, 0.96875], [0.9375, 0.25, 0.0625]]
REG0 = [0.0, 0.0]  # far from the row maxima 0.96875, 0.9375


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_register_timesteps(vds, name):
    """None gives the bits the call gave; pinned to the row maximum the same bits again; pinned elsewhere the helper's
    pinned model, with and without grad"""
    m = build(vds, name)
    cfg, P, latent, ctx = KC.model_case(name)
    ts = torch.tensor(FC_TS).to(bf16)
    args = (latent.cuda(), ctx.cuda(), ts.cuda())
    with torch.no_grad():
        base = m(*args, rope_start=BASE)
        none = m(*args, rope_start=BASE, register_timesteps=None)
        rmax = m(*args, rope_start=BASE, register_timesteps=ts.float().max(dim=1).values)
        pinned = m(*args, rope_start=BASE, register_timesteps=REG0)
        ref0 = FC.dit_forward(P, cfg, latent.float(), ctx.float(), ts.float(), BASE)
    assert torch.equal(bits(base), bits(none)) and torch.equal(bits(base), bits(rmax))
    Pg = {k: p.clone().requires_grad_(True) for k, p in P.items()}
    ref = KC.full_forward(Pg, cfg, latent.float(), ctx.float(), ts.float(), BASE, torch.tensor(REG0))
    w = torch.ones(2, 3)
    loss_r, _, _ = R.frame_loss(latent, ref, w, cfg.time_patch_size)
    loss_r.backward()
    # the register level matters: on the CPU references alone the row-maximum model is > 3 x B_OUT away (0.102 / 0.077),
    # so an output within B_OUT of the pinned reference is > 2 x B_OUT from the other and cannot pass for it
    assert rel(ref0, ref.detach()) > 3 * B_OUT
    e = rel(pinned, ref.detach())
    print(f"{name}: pinned registers, no grad: {e:.3e}")
    assert e <= B_OUT, e
    m.zero_grad()
    out = m(*args, rope_start=BASE, register_timesteps=REG0)
    assert torch.equal(bits(out.detach()), bits(pinned))
    loss, _ = vds["train"].frame_flow_loss(out, latent.cuda(), w.cuda(), cfg.time_patch_size)
    loss.backward()
    torch.cuda.synchronize()
    e_loss = abs(loss.item() - loss_r.item()) / abs(loss_r.item())
    worst = max((rel(p.grad, Pg[k].grad), k) for k, p in m.named_parameters()
                if p.grad is not None and Pg[k].grad is not None and not k.endswith("lambda_param")
                and float(Pg[k].grad.abs().max()) > 0)
    print(f"{name}: pinned registers, grad: loss rel {e_loss:.2e}, worst grad rel err {worst[0]:.3e} ({worst[1]})")
    assert e_loss <= B_LOSS and worst[0] <= B_GRAD, (e_loss, worst)
    m.zero_grad()


# --------------------------------------------------------------------------------------- rollout ----
STEPS, SCALE = 3, 4.0
RBASE = (1, 2, 3)


def rollout_inputs():
    g = torch.Generator().manual_seed(8)
    prompt = torch.randn(1, 12, 64, generator=g).to(bf16)
    lat0 = torch.randn(1, 16, 4, 8, 8, generator=g).to(bf16)
    cond = torch.randn(1, 16, 2, 8, 8, generator=g).to(bf16)
    return prompt, lat0, cond


def test_rollout_against_the_helper_loop(vds, parity_log):
    """a [1,16,4,8,8] latent = 2 token-frames, rollout_frames=1, guided, 3 steps: 2 chunks, the second starting from the
    first one's result and reading its K / V from the cache -- one 3-step sampler budget per chunk"""
    S = vds["sampling"]
    cfg, P, _, _ = KC.model_case("hd72")
    prompt, lat0, _ = rollout_inputs()
    m = build(vds, "hd72")
    acc = S.generate_latents(m, prompt.cuda(), latents=lat0.cuda(), inference_steps=STEPS, cfg_scale=SCALE,
                             rope_starts=[RBASE], rollout_frames=1, kv_cache=True)
    assert acc.dtype == f32 and tuple(acc.shape) == (1, 16, 4, 8, 8) and torch.isfinite(acc).all()
    with torch.no_grad():
        ref = KC.cached_rollout(P, cfg, lat0, prompt, torch.zeros_like(prompt), STEPS, SCALE, RBASE, 1)
    e, e0 = rel(acc, ref), rel(acc[:, :, :2], ref[:, :, :2])
    print(f"cached rollout: rel err {e:.3e} (first token-frame {e0:.3e}), bound {2 * B_SAMPLER:.1e}")
    parity_log("frame_cache_rollout", rel_err=e, first_frame=e0)
    assert e <= 2 * B_SAMPLER and e0 <= B_SAMPLER, (e, e0)


def test_rollout_against_the_uncached_rollout(vds, parity_log):
    """the uncached rollout with the same base in every rope_starts entry: the first token-frame -- the chunk that has a
    frame after it, so the uncached registers sit at 1.0 too -- agrees with the cached one"""
    S = vds["sampling"]
    prompt, lat0, _ = rollout_inputs()
    m = build(vds, "hd72")
    kw = dict(latents=lat0.cuda(), inference_steps=STEPS, cfg_scale=SCALE, rollout_frames=1)
    acc = S.generate_latents(m, prompt.cuda(), rope_starts=[RBASE], kv_cache=True, **kw)
    unc = S.generate_latents(m, prompt.cuda(), rope_starts=[RBASE] * 12, **kw)
    off = S.generate_latents(m, prompt.cuda(), rope_starts=[RBASE] * 12, kv_cache=False, **kw)
    assert torch.equal(bits(unc), bits(off))  # kv_cache=False is the existing loop, bit for bit
    e0 = rel(acc[:, :, :2], unc[:, :, :2])
    print(f"cached vs uncached rollout: first token-frame {e0:.3e} (bound {B_SAMPLER:.1e}), "
          f"last {rel(acc[:, :, 2:], unc[:, :, 2:]):.3e}")
    parity_log("frame_cache_rollout_vs_uncached", first_frame=e0)
    assert e0 <= B_SAMPLER, e0


def test_rollout_with_conditioning_frames(vds):
    """cond_latents + kv_cache=True: one t = 0 call commits the conditioning frame, which comes back as given; the
    generated frame follows the helper loop within one 3-step budget"""
    S = vds["sampling"]
    cfg, P, _, _ = KC.model_case("hd72")
    prompt, lat0, cond = rollout_inputs()
    m = build(vds, "hd72")
    acc = S.generate_latents(m, prompt.cuda(), latents=lat0.cuda(), inference_steps=STEPS, cfg_scale=SCALE,
                             rope_starts=[RBASE], rollout_frames=1, kv_cache=True, cond_latents=cond.cuda())
    assert torch.equal(acc[:, :, :2].cpu(), cond.float())
    with torch.no_grad():
        ref = KC.cached_rollout(P, cfg, lat0, prompt, torch.zeros_like(prompt), STEPS, SCALE, RBASE, 1, cond_latents=cond)
    e = rel(acc[:, :, 2:], ref[:, :, 2:])
    print(f"cached rollout behind a conditioning frame: generated frame {e:.3e} (bound {B_SAMPLER:.1e})")
    assert e <= B_SAMPLER, e
    # unguided: a cache of batch 1
    acc1 = S.generate_latents(m, prompt.cuda(), latents=lat0.cuda(), inference_steps=STEPS, cfg_scale=1.0,
                              rope_starts=[RBASE], rollout_frames=1, kv_cache=True)
    with torch.no_grad():
        ref1 = KC.cached_rollout(P, cfg, lat0, prompt, None, STEPS, 1.0, RBASE, 1)
    assert rel(acc1, ref1) <= 2 * B_SAMPLER, rel(acc1, ref1)
