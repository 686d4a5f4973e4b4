"""Per-frame timestep references (tests/test_frame_timesteps_cpu.py, tests/test_frame_timesteps_gpu.py), on CPU tensors.

The model: a restatement of the oracle's dit_forward / block_forward from oracle.dit_oracle's primitives in which the
conditioning path runs on [B, G, .] -- G = 1 + t modulation groups per sample, group 0 (the register rows) on the sample's
largest timestep, group 1 + f on timesteps[b, f] -- and every modulation (shift, scale, gate) is gathered to the token rows
by group(l) = 0 if l < lead else 1 + (l - lead) % period.  With constant rows it is the oracle's model.
Also: per-frame noising in the input dtype, the frame-weighted loss in float64, and the sampler loop with conditioning
frames."""
import torch

from oracle import dit_oracle as O

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16
N_REG = O.N_REG


def group_of(l, lead, period):
    return 0 if l < lead else 1 + (l - lead) % period


def group_index(L, lead, period):
    """int64 [L]: the modulation group of every row of a sample"""
    return torch.tensor([group_of(l, lead, period) for l in range(L)], dtype=torch.int64)


def group_timesteps(timesteps):
    """[B, t] -> [B, 1 + t]: the timestep of every modulation group (group 0: the row maximum)"""
    return torch.cat([timesteps.max(dim=1, keepdim=True).values, timesteps], dim=1)


def _mods(c, w, b, gidx, n):
    """the n modulation tensors of a layer, each [B, L, D]: linear(silu(c)) on [B, G, D], gathered to rows"""
    return O.linear(O.silu(c), w, b)[:, gidx, :].chunk(n, dim=2)


def block_forward(P, pre, cfg, x, context, c, gidx, v_0, cos, sin):
    """DiTBlock.forward with c [B, G, D] and per-row modulation.  Returns (x, v)."""
    H = cfg.num_heads
    g = lambda n: P.get(pre + n)
    (shift_sa, scale_sa, gate_sa, shift_ca, scale_ca, gate_ca,
     shift_mlp, scale_mlp, gate_mlp) = _mods(c, g("adaLN_modulation.1.weight"), g("adaLN_modulation.1.bias"), gidx, 9)
    xn = O.rms_norm(x, g("norm1.weight")) * (1 + scale_sa) + shift_sa
    q, k, v = O.split_heads(O.linear(xn, g("qkv.weight"), g("qkv.bias")), 3, H)
    if cfg.residual_v and v_0 is not None:
        lam = g("lambda_param")
        v = lam * v + (1 - lam) * v_0
    att = O.merge_heads(O.attention(O.apply_rotary(q, cos, sin), O.apply_rotary(k, cos, sin), v))
    x1 = x + O.linear(att, g("attn_proj.weight")) * gate_sa
    x2 = x1
    if g("q_cross.weight") is not None:
        xn2 = O.rms_norm(x1, g("norm2.weight")) * (1 + scale_ca) + shift_ca
        (qc,) = O.split_heads(O.linear(xn2, g("q_cross.weight"), g("q_cross.bias")), 1, H)
        kc, vc = O.split_heads(O.linear(context, g("context_kv.weight"), g("context_kv.bias")), 2, H)
        x2 = x1 + O.linear(O.merge_heads(O.attention(qc, kc, vc)), g("cross_proj.weight")) * gate_ca
    xn3 = O.rms_norm(x2, g("norm3.weight")) * (1 + scale_mlp) + shift_mlp
    hmid = O.gelu_erf(O.linear(xn3, g("mlp.0.weight"), g("mlp.0.bias")))
    x3 = x2 + O.linear(hmid, g("mlp.2.weight"), g("mlp.2.bias")) * gate_mlp
    return x3, v


def dit_forward(P, cfg, x, context, timesteps, rope_start):
    """DiT.forward with timesteps [B, t], t = T // time_patch_size"""
    B, C, T, Hh, Ww = x.shape
    pt, p = cfg.time_patch_size, cfg.patch_size
    t, h, w = T // pt, Hh // p, Ww // p
    assert tuple(timesteps.shape) == (B, t)
    tok = O.patch_embed(x, P["patch_embed.patch_proj.weight"], P["patch_embed.patch_proj.bias"], pt, p)
    tok = torch.cat([P["register_tokens"].expand(B, -1, -1).to(tok.dtype), tok], dim=1)
    L = tok.shape[1]
    gidx = group_index(L, N_REG, t)
    cos, sin = O.rope_cos_sin(cfg.head_dim, (t, h, w), rope_start)
    G = 1 + t
    temb = O.timestep_embedding(group_timesteps(timesteps).reshape(B * G), cfg.hidden_size).to(tok.dtype)
    c = O.linear(O.silu(O.linear(temb, P["time_embed.0.weight"], P["time_embed.0.bias"])),
                 P["time_embed.2.weight"], P["time_embed.2.bias"]).reshape(B, G, -1)
    v_0 = None
    for i in range(cfg.depth):
        tok, v = block_forward(P, f"blocks.{i}.", cfg, tok, context, c, gidx, v_0, cos, sin)
        if v_0 is None:
            v_0 = v
    fshift, fscale = _mods(c, P["final_modulation.1.weight"], P["final_modulation.1.bias"], gidx, 2)
    tok = (O.rms_norm(tok, P.get("final_norm.weight")) * (1 + fscale) + fshift)[:, N_REG:, :]
    y = O.linear(tok, P["final_proj.weight"], P["final_proj.bias"])
    return O.unpatchify(y, C, t, h, w, pt, p)


def frame_of_latent(T, pt):
    """int64 [T]: the token-frame of every latent frame"""
    return torch.arange(T) // pt


def noise_frames(x, noise, t, pt):
    """z_t = x (1 - t) + noise t, v = x - noise in x.dtype, latent frame j of sample b at t[b, j // pt]"""
    tr = t[:, frame_of_latent(x.shape[2], pt)].to(x.dtype)[:, None, :, None, None]
    return x * (1 - tr) + noise * tr, x - noise


def frame_loss(v, out, w, pt):
    """float64 (loss, per_sample [B], sse [B, t]): per_sample[b] = sum_f w[b,f] SSE[b,f] / (n_f sum_f w[b,f]), 0 where the
    weights of a sample sum to 0; loss = mean_b.  Differentiable in `out`."""
    B, C, T, H, W = v.shape
    t = T // pt
    d = (out.to(f64) - v.to(f64)).reshape(B, C, t, pt * H * W)
    sse = (d * d).sum(dim=(1, 3))
    n_f = C * pt * H * W
    w = w.to(f64)
    ws = w.sum(dim=1)
    per = torch.where(ws > 0, (w * sse).sum(dim=1) / (n_f * torch.where(ws > 0, ws, torch.ones_like(ws))),
                      torch.zeros_like(ws))
    return per.mean(), per, sse


def sample_loop(P, cfg, latents, prompt_embeds, negative_embeds, steps, cfg_scale, rope_starts, cond_latents,
                dtype=f32, alpha=8.0):
    """the oracle's Euler + guidance loop with the first Tc latent frames held at cond_latents: their token-frames are
    given t = 0 in every model call and they are written back into the latents and the accumulator after every step.
    Returns the fp32 accumulator."""
    Pd = {k: v.to(dtype) for k, v in P.items()}
    pt = cfg.time_patch_size
    Tc = cond_latents.shape[2]
    n_cond, n = Tc // pt, latents.shape[2] // pt
    lat = latents.to(dtype).clone()
    acc = lat.to(f32)
    acc[:, :, :Tc] = cond_latents.to(f32)
    lat = acc.to(dtype)
    call = 0
    for i in range(steps, 0, -1):
        t, t_next = i / steps, (i - 1) / steps
        t = t * alpha / (1 + (alpha - 1) * t)
        t_next = t_next * alpha / (1 + (alpha - 1) * t_next)
        tt = torch.tensor([t] * lat.shape[0]).to(bf16).to(dtype)[:, None].repeat(1, n)
        tt[:, :n_cond] = 0
        out = dit_forward(Pd, cfg, lat, prompt_embeds.to(dtype), tt, tuple(rope_starts[call]))
        call += 1
        if cfg_scale > 1:
            un = dit_forward(Pd, cfg, lat, negative_embeds.to(dtype), tt, tuple(rope_starts[call]))
            call += 1
            out = un + cfg_scale * (out - un)
        acc = acc + (t - t_next) * out.to(f32)
        acc[:, :, :Tc] = cond_latents.to(f32)
        lat = acc.to(dtype)
    return acc
