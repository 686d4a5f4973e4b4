"""Token routing, the reference side (tests/test_token_routing_cpu.py and tests/test_token_routing_gpu.py).  CPU only, no
import of the library: written from the definition of DiT.enable_token_routing on oracle.dit_oracle.block_forward.

With N video tokens, 16 register rows in front and `route` = the kept token indices (sorted, distinct, in [0, N)):
  idx = [0 .. 15] ++ (16 + route)        the rows of the full sequence that run the span, Ls = 16 + k of L = 16 + N
  inv[idx[i]] = i, -1 elsewhere
  before block span[0]      tok = tok[:, idx]
  blocks span[0]..span[1]   run on Ls rows with v_0[:, :, idx], cos[idx], sin[idx]
  after block span[1]       out = full.clone(); out[:, idx] = tok      (full: the rows as they were before span[0])

Defects, each a wrong implementation the tests must tell from the right one:
  "dv0"     the gathered v_0 is detached: the routed blocks' share of d v_0 never reaches block 0
  "rope"    the routed blocks rotate with the FIRST Ls rows of the tables, not the gathered ones
  "bypass"  `full` is detached: the rows that skipped the span carry no gradient to the blocks before it"""
import contextlib

import torch

from oracle import dit_oracle as O

N_REG = O.N_REG
bf16 = torch.bfloat16
START = (2, 3, 4)
SPAN = (1, 2)
KEEP = 0.5
N_TOK = 256  # latent [2, 16, 8, 16, 16] with (pt, p) = (2, 2): t, h, w = 4, 8, 8


def keep_count(N, keep):
    return max(1, int(keep * N + 0.5))


def tables(route, N):
    """(idx int64 [16 + k], inv int64 [16 + N])"""
    route = torch.as_tensor(route, dtype=torch.int64)
    idx = torch.cat([torch.arange(N_REG), N_REG + route])
    inv = torch.full((N_REG + N,), -1, dtype=torch.int64)
    inv[idx] = torch.arange(idx.shape[0])
    return idx, inv


def routed_forward(P, cfg, x, ctx, ts, start, span, route, defect=None):
    """oracle.dit_forward with the blocks span[0] .. span[1] (inclusive) on the rows idx; route None: every row runs every
    block (oracle.dit_forward itself)"""
    assert defect in (None, "dv0", "rope", "bypass")
    B, C, T, Hh, Ww = x.shape
    pt, p = cfg.time_patch_size, cfg.patch_size
    t, h, w = T // pt, Hh // p, Ww // p
    tok = O.patch_embed(x, P["patch_embed.patch_proj.weight"], P["patch_embed.patch_proj.bias"], pt, p)
    tok = torch.cat([P["register_tokens"].expand(B, -1, -1).to(tok.dtype), tok], dim=1)
    cos, sin = O.rope_cos_sin(cfg.head_dim, (t, h, w), start)
    temb = O.timestep_embedding(ts, cfg.hidden_size).to(tok.dtype)
    c = O.linear(O.silu(O.linear(temb, P["time_embed.0.weight"], P["time_embed.0.bias"])),
                 P["time_embed.2.weight"], P["time_embed.2.bias"])
    idx = tables(route, t * h * w)[0] if route is not None else None
    v_0 = full = None
    for i in range(cfg.depth):
        routed = idx is not None and span[0] <= i <= span[1]
        if routed and i == span[0]:
            full = tok.detach() if defect == "bypass" else tok
            tok = tok[:, idx]
        if routed:
            Ls = idx.shape[0]
            v0_i = v_0[:, :, idx]
            if defect == "dv0":
                v0_i = v0_i.detach()
            cos_i, sin_i = (cos[:Ls], sin[:Ls]) if defect == "rope" else (cos[idx], sin[idx])
        else:
            v0_i, cos_i, sin_i = v_0, cos, sin
        tok, v = O.block_forward(P, f"blocks.{i}.", cfg, tok, ctx, c, v0_i, cos_i, sin_i)
        if v_0 is None:
            v_0 = v
        if routed and i == span[1]:
            out = full.clone()
            out[:, idx] = tok
            tok = out
    tok = tok[:, N_REG:, :]
    fshift, fscale = O.linear(O.silu(c), P["final_modulation.1.weight"], P["final_modulation.1.bias"]).chunk(2, dim=1)
    tok = O.modulate(O.rms_norm(tok, P.get("final_norm.weight")), fshift, fscale)
    y = O.linear(tok, P["final_proj.weight"], P["final_proj.bias"])
    return O.unpatchify(y, C, t, h, w, pt, p)


@contextlib.contextmanager
def context_lens_oracle(context_lens):
    """For the duration of the block, a call of oracle.dit_oracle.attention whose key count differs from its query count
    -- the cross-attention: Lc = 24 against L = 272 and Ls = 144 here -- lets sample b attend its first context_lens[b]
    context rows only (none at all at 0: the attention adds nothing).  Nests with qk_norm_ref.qk_normed_oracle and, entered
    before it, with head_norm_ref.cross_normed_oracle."""
    import math
    orig = O.attention
    lens = torch.as_tensor(context_lens)

    def attention(q, k, v):
        if k.shape[-2] == q.shape[-2]:
            return orig(q, k, v)
        keep = torch.arange(k.shape[-2])[None, :] < lens[:, None]  # [B, Lc]
        s = (q.float() @ k.float().transpose(-1, -2)) / math.sqrt(q.shape[-1])
        s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
        pr = torch.softmax(s, dim=-1)
        return (torch.where(keep.any(dim=1)[:, None, None, None], pr, torch.zeros_like(pr)) @ v.float()).to(q.dtype)

    O.attention = attention
    try:
        yield
    finally:
        O.attention = orig


_cases = {}


def case(name):
    """hd72: D = 144, H = 2; hd64: D = 128, H = 2.  depth 4 with the span (1, 2): one block before, two routed, one after;
    residual_v with distinct lambdas 0.3 + 0.1 i; latent [2, 16, 8, 16, 16] -> N = 256, L = 272 and, at keep 0.5, Ls = 144:
    more than one 128-row query tile on both lengths; context [2, 24, 64]; [B] timesteps; a route from a seeded generator"""
    if name in _cases:
        return _cases[name]
    D, seed = {"hd72": (144, 23), "hd64": (128, 29)}[name]
    cfg = O.DiTConfig(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=D, depth=4, num_heads=2,
                      cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False)
    P = O.init_params(cfg, seed=seed, randomize_zero_init=True, init_std_factor=1.0)
    P["time_embed.0.weight"] = P["time_embed.0.weight"] * 8  # (as tests/test_frame_causal_gpu.py: gates of order one, so
    P["time_embed.2.weight"] = P["time_embed.2.weight"] * 8  # that every block is in the output)
    for i in range(cfg.depth):
        P[f"blocks.{i}.lambda_param"] = torch.full_like(P[f"blocks.{i}.lambda_param"], 0.3 + 0.1 * i)
    g = torch.Generator().manual_seed(seed + 1)
    latent = torch.randn(2, 16, 8, 16, 16, generator=g).to(bf16)
    ctx = torch.randn(2, 24, 64, generator=g).to(bf16)
    noise = torch.randn(2, 16, 8, 16, 16, generator=g).to(bf16)
    ts = torch.tensor([0.25, 0.8125]).to(bf16)
    zt, v = O.noise_latents(latent, noise, ts)
    k = keep_count(N_TOK, KEEP)
    route = torch.randperm(N_TOK, generator=g)[:k].sort().values
    _cases[name] = dict(cfg=cfg, P=P, latent=latent, ctx=ctx, noise=noise, ts=ts, zt=zt, v=v, route=route)
    return _cases[name]


_refs = {}


def reference_step(name, route="case", defect=None, P=None, wrap=(), key=None):
    """one fp32 step (forward, flow loss, backward) of routed_forward, cached per (name, route, defect, key); route "case":
    the case's own, None: the unrouted model; P: other parameters (leaves that require grad), wrap: context managers"""
    cs = case(name)
    if isinstance(route, str):
        route = cs["route"]
    rk = None if route is None else tuple(int(r) for r in route)
    ck = (name, rk, defect, key)
    if ck in _refs and (P is None or key is not None):
        return _refs[ck]
    Pg = {k: p.clone().requires_grad_(True) for k, p in cs["P"].items()} if P is None else P
    with contextlib.ExitStack() as st:
        for w in wrap:
            st.enter_context(w)
        out = routed_forward(Pg, cs["cfg"], cs["zt"].float(), cs["ctx"].float(), cs["ts"].float(), START, SPAN, route, defect)
        loss, _ = O.flow_loss(cs["v"], out)
        loss.backward()
    ref = dict(out=out.detach(), loss=loss.item(),
               grads={k: p.grad for k, p in Pg.items() if p.is_leaf and p.grad is not None})
    if P is None or key is not None:
        _refs[ck] = ref
    return ref


def rel(a, b):
    a, b = a.float().cpu().flatten(), b.float().cpu().flatten()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()
