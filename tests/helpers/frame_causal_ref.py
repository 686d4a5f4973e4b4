"""Frame-causal self-attention references (tests/test_frame_causal_cpu.py, tests/test_attn_causal_gpu.py,
tests/test_frame_causal_gpu.py), in fp32 on CPU tensors.

One definition at every layer: group(l) = 0 if l < lead else 1 + (l - lead) % period (the row groups of per-frame
timesteps, frame_timesteps_ref.group_of), and query row q may attend key row k iff group(k) <= group(q).

  allowed            the mask as a bool [L, L] (rows: queries)
  masked_attention   scores masked_fill(-inf), softmax, autograd
  dit_forward        frame_timesteps_ref's helper model with that attention in the self-attention ONLY (the cross-attention
                     stays unmasked); frame_causal=False is that model unchanged
  rollout_loop       the sampler's frame rollout: chunk after chunk of token-frames, each with its own full Euler pass"""
import math

import torch

from oracle import dit_oracle as O

import frame_timesteps_ref as R

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16
N_REG = R.N_REG


def allowed(L, lead, period):
    """bool [L, L]: allowed[q, k] = group(k) <= group(q)"""
    g = R.group_index(L, lead, period)
    return g[None, :] <= g[:, None]


def masked_attention(q, k, v, mask):
    """q, k, v [..., L, hd], mask bool [L, L] -> (o [..., L, hd], lse [..., L]); differentiable"""
    s = (q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    s = s.masked_fill(~mask, float("-inf"))
    return torch.softmax(s, dim=-1) @ v, torch.logsumexp(s, dim=-1)


def cross_attention(q, k, v, context_lens):
    """the (unmasked-over-frames) cross-attention; context_lens [B] or None: sample b attends its first context_lens[b]
    context rows, none at all when that is 0 (the attention then adds nothing)"""
    if context_lens is None:
        return O.attention(q, k, v)
    Lc = k.shape[-2]
    keep = torch.arange(Lc)[None, :] < torch.as_tensor(context_lens)[:, None]  # [B, Lc]
    s = (q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.where(keep.any(dim=1)[:, None, None, None], p, torch.zeros_like(p)) @ v


def block_forward(P, pre, cfg, x, context, c, gidx, v_0, cos, sin, mask, context_lens=None):
    """frame_timesteps_ref.block_forward with the self-attention restricted by `mask` (None: unrestricted)"""
    H = cfg.num_heads
    g = lambda n: P.get(pre + n)
    (shift_sa, scale_sa, gate_sa, shift_ca, scale_ca, gate_ca,
     shift_mlp, scale_mlp, gate_mlp) = R._mods(c, g("adaLN_modulation.1.weight"), g("adaLN_modulation.1.bias"), gidx, 9)
    xn = O.rms_norm(x, g("norm1.weight")) * (1 + scale_sa) + shift_sa
    q, k, v = O.split_heads(O.linear(xn, g("qkv.weight"), g("qkv.bias")), 3, H)
    if cfg.residual_v and v_0 is not None:
        lam = g("lambda_param")
        v = lam * v + (1 - lam) * v_0
    qr, kr = O.apply_rotary(q, cos, sin), O.apply_rotary(k, cos, sin)
    att = O.merge_heads(O.attention(qr, kr, v) if mask is None else masked_attention(qr, kr, v, mask)[0])
    x1 = x + O.linear(att, g("attn_proj.weight")) * gate_sa
    x2 = x1
    if g("q_cross.weight") is not None:
        xn2 = O.rms_norm(x1, g("norm2.weight")) * (1 + scale_ca) + shift_ca
        (qc,) = O.split_heads(O.linear(xn2, g("q_cross.weight"), g("q_cross.bias")), 1, H)
        kc, vc = O.split_heads(O.linear(context, g("context_kv.weight"), g("context_kv.bias")), 2, H)
        x2 = x1 + O.linear(O.merge_heads(cross_attention(qc, kc, vc, context_lens)), g("cross_proj.weight")) * gate_ca
    xn3 = O.rms_norm(x2, g("norm3.weight")) * (1 + scale_mlp) + shift_mlp
    hmid = O.gelu_erf(O.linear(xn3, g("mlp.0.weight"), g("mlp.0.bias")))
    x3 = x2 + O.linear(hmid, g("mlp.2.weight"), g("mlp.2.bias")) * gate_mlp
    return x3, v


def dit_forward(P, cfg, x, context, timesteps, rope_start, frame_causal=True, context_lens=None):
    """DiT.forward with timesteps [B, t] (a [B] tensor is expanded to constant rows) and, with frame_causal, every
    self-attention restricted to allowed(L, N_REG, t)"""
    B, C, T, Hh, Ww = x.shape
    pt, p = cfg.time_patch_size, cfg.patch_size
    t, h, w = T // pt, Hh // p, Ww // p
    if timesteps.dim() == 1:
        timesteps = timesteps[:, None].expand(B, t)
    assert tuple(timesteps.shape) == (B, t)
    tok = O.patch_embed(x, P["patch_embed.patch_proj.weight"], P["patch_embed.patch_proj.bias"], pt, p)
    tok = torch.cat([P["register_tokens"].expand(B, -1, -1).to(tok.dtype), tok], dim=1)
    L = tok.shape[1]
    gidx = R.group_index(L, N_REG, t)
    mask = allowed(L, N_REG, t) if frame_causal else None
    cos, sin = O.rope_cos_sin(cfg.head_dim, (t, h, w), rope_start)
    G = 1 + t
    temb = O.timestep_embedding(R.group_timesteps(timesteps).reshape(B * G), cfg.hidden_size).to(tok.dtype)
    c = O.linear(O.silu(O.linear(temb, P["time_embed.0.weight"], P["time_embed.0.bias"])),
                 P["time_embed.2.weight"], P["time_embed.2.bias"]).reshape(B, G, -1)
    v_0 = None
    for i in range(cfg.depth):
        tok, v = block_forward(P, f"blocks.{i}.", cfg, tok, context, c, gidx, v_0, cos, sin, mask, context_lens)
        if v_0 is None:
            v_0 = v
    fshift, fscale = R._mods(c, P["final_modulation.1.weight"], P["final_modulation.1.bias"], gidx, 2)
    tok = (O.rms_norm(tok, P.get("final_norm.weight")) * (1 + fscale) + fshift)[:, N_REG:, :]
    y = O.linear(tok, P["final_proj.weight"], P["final_proj.bias"])
    return O.unpatchify(y, C, t, h, w, pt, p)


def rollout_loop(P, cfg, latents, prompt_embeds, negative_embeds, steps, cfg_scale, rope_starts, rollout_frames,
                 frame_causal=True, dtype=f32, alpha=8.0):
    """The sampler's frame rollout: the token-frames are generated `rollout_frames` at a time, in order; every chunk runs
    the whole Euler loop with a timesteps row that is 0 before the chunk, the step's t on it and 1.0 after it, and after
    every step the frames outside the chunk are put back to what they were when the chunk started.  Returns the fp32
    accumulator."""
    Pd = {k: v.to(dtype) for k, v in P.items()}
    pt = cfg.time_patch_size
    n = latents.shape[2] // pt
    lat = latents.to(dtype).clone()
    acc = lat.to(f32)
    call = 0
    for f0 in range(0, n, rollout_frames):
        f1 = min(f0 + rollout_frames, n)
        acc0 = acc.clone()
        for i in range(steps, 0, -1):
            t, t_next = i / steps, (i - 1) / steps
            t = t * alpha / (1 + (alpha - 1) * t)
            t_next = t_next * alpha / (1 + (alpha - 1) * t_next)
            row = torch.ones(n)
            row[:f0] = 0
            row[f0:f1] = t
            tt = row.to(bf16).to(dtype)[None, :].repeat(lat.shape[0], 1)
            out = dit_forward(Pd, cfg, lat, prompt_embeds.to(dtype), tt, tuple(rope_starts[call]), frame_causal)
            call += 1
            if cfg_scale > 1:
                un = dit_forward(Pd, cfg, lat, negative_embeds.to(dtype), tt, tuple(rope_starts[call]), frame_causal)
                call += 1
                out = un + cfg_scale * (out - un)
            acc = acc + (t - t_next) * out.to(f32)
            acc[:, :, :f0 * pt] = acc0[:, :, :f0 * pt]
            acc[:, :, f1 * pt:] = acc0[:, :, f1 * pt:]
            lat = acc.to(dtype)
    return acc
