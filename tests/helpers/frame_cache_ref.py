"""Frame KV cache references (tests/test_frame_cache_cpu.py, tests/test_attn_past_gpu.py, tests/test_frame_cache_gpu.py), in
fp32 on CPU tensors, built on frame_causal_ref.

  past_allowed       the mask of an attention call with a past as a bool [Lq, Lq + past] (rows: queries)
  full_forward       frame_causal_ref.dit_forward with the register group's noise level pinned (register_timesteps)
  chunk_forward      the helper model run on the rows of one chunk of token-frames -- registers + the chunk's tokens --
                     with a list of cached K / V rows per block and a pinned register level
  Cache              that list: per block the rotated k rows and the (residual-mixed) v rows of the committed frames
  cached_rollout     the sampler's cached rollout loop

Keys of a call with a past: [lead rows | past rows | the call's token rows].  A lead query attends the lead keys only; a
token query the lead keys, every past key, and own key j iff group(j - past) <= group(query).

RoPE: the reference flattens its table (t h w) while the tokens are ordered (h w t), so token row i of a video of T frames
gets table row i -- the rotation of another position than its own, which depends on T.  A chunk's tokens therefore take the
rows they have in the table of the WHOLE video (chunk_rope); only then is a chunk call the full-sequence call restricted to
the chunk's frames."""
import torch

from oracle import dit_oracle as O

import frame_causal_ref as FC

R = FC.R
f32, bf16 = torch.float32, torch.bfloat16
N_REG = FC.N_REG


def past_allowed(Lq, lead, period, past):
    """bool [Lq, Lq + past]"""
    gq = R.group_index(Lq, lead, period)
    own = gq[None, lead:] <= gq[:, None]  # own token keys
    lead_k = torch.ones(Lq, lead, dtype=torch.bool)
    past_k = (gq >= 1)[:, None].expand(Lq, past)
    return torch.cat([lead_k, past_k, own], dim=1)


def with_register_level(timesteps, reg):
    """[B, t], [B] -> [B, 1 + t]: group 0 at the pinned level"""
    return torch.cat([torch.as_tensor(reg, dtype=timesteps.dtype).reshape(-1, 1), timesteps], dim=1)


def _conditioning(P, cfg, timesteps, reg, dtype):
    B, t = timesteps.shape
    G = 1 + t
    temb = O.timestep_embedding(with_register_level(timesteps, reg).reshape(B * G), cfg.hidden_size).to(dtype)
    return O.linear(O.silu(O.linear(temb, P["time_embed.0.weight"], P["time_embed.0.bias"])),
                    P["time_embed.2.weight"], P["time_embed.2.bias"]).reshape(B, G, -1)


def full_forward(P, cfg, x, context, timesteps, rope_start, reg, context_lens=None):
    """FC.dit_forward (frame_causal) with the register group modulated from reg [B] instead of the row maximum"""
    B, C, T, Hh, Ww = x.shape
    pt, p = cfg.time_patch_size, cfg.patch_size
    t, h, w = T // pt, Hh // p, Ww // p
    tok = O.patch_embed(x, P["patch_embed.patch_proj.weight"], P["patch_embed.patch_proj.bias"], pt, p)
    tok = torch.cat([P["register_tokens"].expand(B, -1, -1).to(tok.dtype), tok], dim=1)
    L = tok.shape[1]
    gidx = R.group_index(L, N_REG, t)
    mask = FC.allowed(L, N_REG, t)
    cos, sin = O.rope_cos_sin(cfg.head_dim, (t, h, w), rope_start)
    c = _conditioning(P, cfg, timesteps, reg, tok.dtype)
    v_0 = None
    for i in range(cfg.depth):
        tok, v = FC.block_forward(P, f"blocks.{i}.", cfg, tok, context, c, gidx, v_0, cos, sin, mask, context_lens)
        if v_0 is None:
            v_0 = v
    fshift, fscale = R._mods(c, P["final_modulation.1.weight"], P["final_modulation.1.bias"], gidx, 2)
    tok = (O.rms_norm(tok, P.get("final_norm.weight")) * (1 + fscale) + fshift)[:, N_REG:, :]
    y = O.linear(tok, P["final_proj.weight"], P["final_proj.bias"])
    return O.unpatchify(y, C, t, h, w, pt, p)


class Cache:
    """per block: k, v [B, H, past rows, hd] of the committed frames (k rotated, v after the residual-V mix)"""

    def __init__(self, depth, frames):
        self.frames = frames  # token-frames of the whole video
        self.k, self.v = [None] * depth, [None] * depth
        self.past_frames = 0
        self.pending = None

    def commit(self):
        ks, vs, n = self.pending
        for i, (k, v) in enumerate(zip(ks, vs)):
            self.k[i] = k if self.k[i] is None else torch.cat([self.k[i], k], dim=2)
            self.v[i] = v if self.v[i] is None else torch.cat([self.v[i], v], dim=2)
        self.past_frames += n
        self.pending = None


def chunk_rope(head_dim, frames, h, w, base, f0, k):
    """cos / sin rows of registers + the tokens of frames f0 .. f0 + k - 1, taken from the whole video's table"""
    cos, sin = O.rope_cos_sin(head_dim, (frames, h, w), base)
    rows = N_REG + torch.arange(h * w)[:, None] * frames + f0 + torch.arange(k)[None, :]
    idx = torch.cat([torch.arange(N_REG), rows.reshape(-1)])
    return cos[idx], sin[idx]


def _block_chunk(P, pre, cfg, x, context, c, gidx, v_0, cos, sin, mask, past_k, past_v, context_lens, use_past=True):
    """FC.block_forward on the chunk's rows, the self-attention's keys / values extended by the past rows"""
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
    K, V = kr, v
    if past_k is not None and use_past:
        K = torch.cat([kr[:, :, :N_REG], past_k, kr[:, :, N_REG:]], dim=2)
        V = torch.cat([v[:, :, :N_REG], past_v, v[:, :, N_REG:]], dim=2)
    att = O.merge_heads(FC.masked_attention(qr, K, V, mask)[0])
    x1 = x + O.linear(att, g("attn_proj.weight")) * gate_sa
    x2 = x1
    if g("q_cross.weight") is not None:
        xn2 = O.rms_norm(x1, g("norm2.weight")) * (1 + scale_ca) + shift_ca
        (qc,) = O.split_heads(O.linear(xn2, g("q_cross.weight"), g("q_cross.bias")), 1, H)
        kc, vc = O.split_heads(O.linear(context, g("context_kv.weight"), g("context_kv.bias")), 2, H)
        x2 = x1 + O.linear(O.merge_heads(FC.cross_attention(qc, kc, vc, context_lens)), g("cross_proj.weight")) * gate_ca
    xn3 = O.rms_norm(x2, g("norm3.weight")) * (1 + scale_mlp) + shift_mlp
    hmid = O.gelu_erf(O.linear(xn3, g("mlp.0.weight"), g("mlp.0.bias")))
    x3 = x2 + O.linear(hmid, g("mlp.2.weight"), g("mlp.2.bias")) * gate_mlp
    return x3, v, kr


def chunk_forward(P, cfg, x, context, timesteps, base, reg, cache, context_lens=None, use_past=True):
    """The helper model on one chunk: x [B, C, k*pt, H, W] holds the k token-frames behind cache.past_frames, timesteps
    [B, k], base = the RoPE start of the WHOLE video, reg [B] the register level.  The chunk's K / V are left in
    cache.pending (cache.commit() appends them).  use_past=False drops the past keys (the discrimination check)."""
    B, C, T, Hh, Ww = x.shape
    pt, p = cfg.time_patch_size, cfg.patch_size
    k, h, w = T // pt, Hh // p, Ww // p
    assert tuple(timesteps.shape) == (B, k) and cache.past_frames + k <= cache.frames
    tok = O.patch_embed(x, P["patch_embed.patch_proj.weight"], P["patch_embed.patch_proj.bias"], pt, p)
    tok = torch.cat([P["register_tokens"].expand(B, -1, -1).to(tok.dtype), tok], dim=1)
    L = tok.shape[1]
    gidx = R.group_index(L, N_REG, k)
    past = cache.past_frames * h * w if use_past else 0
    mask = past_allowed(L, N_REG, k, past)
    cos, sin = chunk_rope(cfg.head_dim, cache.frames, h, w, base, cache.past_frames, k)
    c = _conditioning(P, cfg, timesteps, reg, tok.dtype)
    v_0 = None
    ks, vs = [], []
    for i in range(cfg.depth):
        tok, v, kr = _block_chunk(P, f"blocks.{i}.", cfg, tok, context, c, gidx, v_0, cos, sin, mask, cache.k[i], cache.v[i],
                                  context_lens, use_past)
        if v_0 is None:
            v_0 = v
        ks.append(kr[:, :, N_REG:])
        vs.append(v[:, :, N_REG:])
    cache.pending = (ks, vs, k)
    fshift, fscale = R._mods(c, P["final_modulation.1.weight"], P["final_modulation.1.bias"], gidx, 2)
    tok = (O.rms_norm(tok, P.get("final_norm.weight")) * (1 + fscale) + fshift)[:, N_REG:, :]
    y = O.linear(tok, P["final_proj.weight"], P["final_proj.bias"])
    return O.unpatchify(y, C, k, h, w, pt, p)


def cached_rollout(P, cfg, latents, prompt_embeds, negative_embeds, steps, cfg_scale, base, rollout_frames,
                   cond_latents=None, dtype=f32, alpha=8.0):
    """The sampler's cached rollout (generate_latents(rollout_frames=, kv_cache=True)): one RoPE base, the guided pair as
    one batch of 2, registers at level 1.0 in every call; per chunk `steps` calls on the chunk alone, then -- after every
    chunk but the last -- one call on the finished chunk at t = 0 whose K / V are committed.  Returns the fp32
    accumulator."""
    Pd = {k: v.to(dtype) for k, v in P.items()}
    pt = cfg.time_patch_size
    n = latents.shape[2] // pt
    guided = cfg_scale > 1
    nb = 2 if guided else 1
    ctx = torch.cat([prompt_embeds, negative_embeds]).to(dtype) if guided else prompt_embeds.to(dtype)
    lat = latents.to(dtype).clone()
    acc = lat.to(f32)
    n_cond = 0
    if cond_latents is not None:
        n_cond = cond_latents.shape[2] // pt
        acc[:, :, :n_cond * pt] = cond_latents.to(f32)
        lat = acc.to(dtype)
    cache = Cache(cfg.depth, n)
    reg = torch.ones(nb)

    def call(f0, f1, t):
        x = lat[:, :, f0 * pt:f1 * pt]
        tt = torch.full((nb, f1 - f0), float(t)).to(bf16).to(dtype)
        return chunk_forward(Pd, cfg, torch.cat([x, x]) if guided else x, ctx, tt, tuple(base), reg, cache)

    if n_cond:
        call(0, n_cond, 0.0)
        cache.commit()
    for f0 in range(n_cond, n, rollout_frames):
        f1 = min(f0 + rollout_frames, n)
        for i in range(steps, 0, -1):
            t, t_next = i / steps, (i - 1) / steps
            t = t * alpha / (1 + (alpha - 1) * t)
            t_next = t_next * alpha / (1 + (alpha - 1) * t_next)
            out = call(f0, f1, t)
            if guided:
                out = out[1:2] + cfg_scale * (out[0:1] - out[1:2])
            acc[:, :, f0 * pt:f1 * pt] += (t - t_next) * out.to(f32)
            lat = acc.to(dtype)
        if f1 < n:
            call(f0, f1, 0.0)
            cache.commit()
    return acc


_cases = {}


def model_case(name):
    """the tiny configurations, parameters and inputs of the frame-causal tests (tests/test_frame_causal_gpu.py): latent
    [2,16,6,8,8] with (pt, p) = (2, 2), so t = 3 token-frames of 16 tokens; context [2,24,64]"""
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
    _cases[name] = (cfg, P, latent, ctx)
    return _cases[name]


# chunks of the tiny case: (first token-frame, token-frames)
CHUNKS = [(0, 1), (1, 1), (2, 1), (1, 2)]
BASE = (2, 3, 4)  # RoPE start of the whole video
REG = [1.0, 0.75]  # pinned register levels
T_CHUNK = [[0.5, 0.96875], [0.25, 0.0625]]  # noise levels of the chunk's frames (first k columns)


def chunk_reference(name, f0, k, qk_norm=False, context_lens=None, use_past=True):
    """fp32, once per case: the helper's cached call on frames f0 .. f0 + k - 1 of model_case(name), the frames before
    them committed through t = 0 calls (one per frame).  Returns (out [2,16,2k,8,8], cache)."""
    key = (name, f0, k, qk_norm, None if context_lens is None else tuple(context_lens), use_past)
    if key in _cases:
        return _cases[key]
    from contextlib import nullcontext
    from qk_norm_ref import qk_normed_oracle
    cfg, P, latent, ctx = model_case(name)
    pt = cfg.time_patch_size
    n = latent.shape[2] // pt
    reg = torch.tensor(REG)
    with torch.no_grad(), (qk_normed_oracle() if qk_norm else nullcontext()):
        cache = Cache(cfg.depth, n)
        for f in range(f0):
            chunk_forward(P, cfg, latent[:, :, f * pt:(f + 1) * pt].float(), ctx.float(), torch.zeros(2, 1), BASE, reg, cache,
                          context_lens)
            cache.commit()
        tt = torch.tensor(T_CHUNK)[:, :k].to(bf16).float()
        out = chunk_forward(P, cfg, latent[:, :, f0 * pt:(f0 + k) * pt].float(), ctx.float(), tt, BASE, reg, cache,
                            context_lens, use_past=use_past)
    _cases[key] = (out, cache)
    return _cases[key]
