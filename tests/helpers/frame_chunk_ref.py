"""Chunk-causal self-attention, the reference side (tests/test_frame_chunk_cpu.py and the GPU modules).  CPU only, no
import of the library: everything here is written from the definitions in include/vds.h.

With `lead` register rows, `period` = t token-frames and a chunk of c >= 1 token-frames:
  token rows         group(l) = 0 for l < lead, else 1 + ((l - lead) % period) // c
  frame-major rows   group(r) = 0 for r < lead, else 1 + (r - lead) // (c * S),  S = (L - lead) // period
and query attends key iff group(key) <= group(query).  period % c != 0: the last chunk is short; c >= period: one token
group (tokens attend everything, registers the registers); c = 1: the frame-causal mask of frame_major_ref.

  allowed_tok / allowed      the dense mask in token rows / in frame-major rows
  key_end / query_start      the bounds the kernels state (kend clipped to L)
  mask_by_tiles              the mask as the forward / dQ kernels apply it: the key loop to kend of the tile's last query,
                             open sub-blocks, the per-lane compare key < kend(query)
  mask_by_key_tiles          ... and as the dK/dV kernels do: the first query tile from qstart, open sub-blocks, the
                             per-lane compare query >= qstart(key)
  census_*                   attn_census inputs in frame-major rows, the chunk boundaries among the first probes
  dit_forward                frame_causal_ref's helper model under the chunk mask (register level: row maximum, or pinned)
  chunk_forward              frame_cache_ref's cached call for a chunk model: the call's frames are ONE chunk, so every token
                             query attends every own key -- the past mask with one token group"""
import torch

from oracle import dit_oracle as O

import attn_census as AC
import frame_cache_ref as KC
import frame_major_ref as FM

FC, R = KC.FC, KC.R
N_REG = FC.N_REG
f32, bf16 = torch.float32, torch.bfloat16

# (L, lead, period, c): the shapes of frame_major_ref with a chunk -- short last chunks (3 % 2, 8 % 3, 7 % 3), c >= period
# (one token group), no lead, S = 1, several 256-row tiles per chunk
SHAPES = [(166, 16, 3, 2), (280, 16, 8, 2), (280, 16, 8, 4), (280, 16, 8, 3), (280, 16, 8, 11), (203, 0, 7, 3),
          (140, 5, 3, 2), (293, 33, 4, 2), (80, 16, 64, 16), (1024, 0, 4, 2), (1040, 16, 4, 2)]
TILES = FM.TILES
ids = lambda s: "L{}_{}_{}_c{}".format(*s)


def rows_per_frame(L, lead, period):
    return max(FM.rows_per_frame(L, lead, period), 1)


def group_of_tok(l, lead, period, c):
    return 0 if l < lead else 1 + ((l - lead) % period) // c


def group_of(r, lead, S, c):
    return 0 if r < lead else 1 + (r - lead) // (c * S)


def group_index_tok(L, lead, period, c):
    l = torch.arange(L)
    return torch.where(l < lead, torch.zeros_like(l), 1 + ((l - lead).clamp(min=0) % period) // c)


def allowed_tok(L, lead, period, c):
    """bool [L, L] in token rows: [q, k] = group(k) <= group(q)"""
    g = group_index_tok(L, lead, period, c)
    return g[None, :] <= g[:, None]


def allowed(L, lead, period, c):
    """bool [L, L] in frame-major rows"""
    S = rows_per_frame(L, lead, period)
    r = torch.arange(L)
    g = torch.where(r < lead, torch.zeros_like(r), 1 + (r - lead).clamp(min=0) // (c * S))
    return g[None, :] <= g[:, None]


def key_end(q0, q1, lead, S, c, L):
    """the key loop of the query rows [q0, q1) ends here: kend of the last query, clipped to L (a short last chunk)"""
    if q1 <= lead:
        return lead
    G = c * S
    return min(L, lead + ((q1 - 1 - lead) // G + 1) * G)


def query_start(k0, lead, S, c):
    """the query loop of the key rows from k0 starts here (rounded down to the query tile by the kernel)"""
    if k0 < lead:
        return 0
    G = c * S
    return lead + ((k0 - lead) // G) * G


def mask_by_tiles(L, lead, period, c, tile, wave_rows=32, sub=32):
    """forward / dQ kernels: a workgroup of `tile` queries visits the keys [0, kend of its last query); a wave of wave_rows
    queries from w0 takes a sub-block of `sub` keys without a compare when w0 is a token row and the sub-block ends at or
    below kend(w0); every other element is compared against its own query's kend"""
    S = rows_per_frame(L, lead, period)
    kend = torch.tensor([key_end(q, q + 1, lead, S, c, L) for q in range(L)])
    keys = torch.arange(L)
    out = torch.zeros(L, L, dtype=torch.bool)
    for q0 in range(0, L, tile):
        q1 = min(q0 + tile, L)
        lk = key_end(q0, q1, lead, S, c, L)
        assert lk <= L
        for w0 in range(q0, q1, wave_rows):
            w1 = min(w0 + wave_rows, q1)
            wklim = key_end(w0, w0 + 1, lead, S, c, L) if w0 >= lead else 0
            for k0 in range(0, lk, sub):
                k1 = min(k0 + sub, lk)
                if k0 + sub <= wklim:  # (the kernels test the whole sub-block, ragged or not)
                    out[w0:w1, k0:k1] = True
                else:
                    out[w0:w1, k0:k1] = keys[None, k0:k1] < kend[w0:w1, None]
    return out


def mask_by_key_tiles(L, lead, period, c, tile, qtile=64, wave_keys=32, sub=32):
    """dK/dV kernels: a workgroup of `tile` keys from k0 starts its query loop at the qtile-row tile that holds qstart(k0);
    a wave of wave_keys keys takes a sub-block of `sub` queries without a compare when it starts at or past qstart of the
    wave's last key (the sequence's last row at most); every other element is compared against its own key's qstart"""
    S = rows_per_frame(L, lead, period)
    qstart = torch.tensor([query_start(k, lead, S, c) for k in range(L)])
    rows = torch.arange(L)
    out = torch.zeros(L, L, dtype=torch.bool)
    for k0 in range(0, L, tile):
        k1 = min(k0 + tile, L)
        first = query_start(k0, lead, S, c) // qtile * qtile
        for w0 in range(k0, k1, wave_keys):
            w1 = min(w0 + wave_keys, k1)
            wqlim = query_start(min(w0 + wave_keys - 1, L - 1), lead, S, c)
            for q0 in range(first, L, sub):
                q1 = min(q0 + sub, L)
                if q0 >= wqlim:
                    out[q0:q1, w0:w1] = True
                else:
                    out[q0:q1, w0:w1] = rows[q0:q1, None] >= qstart[None, w0:w1]
    return out


def tiles_visited(L, lead, period, c, tile=64, qtile=128):
    """(visited, all) key tiles of `tile` rows summed over the query tiles of `qtile` rows"""
    S = rows_per_frame(L, lead, period)
    vis = tot = 0
    for q0 in range(0, L, qtile):
        q1 = min(q0 + qtile, L)
        vis += -(-key_end(q0, q1, lead, S, c, L) // tile)
        tot += -(-L // tile)
    return vis, tot


# ---------------------------------------------------------------------------- census, frame-major ----
def census_mask(B, L, lead, period, c):
    return allowed(L, lead, period, c)[None].expand(B, L, L)


def census_signs(B, H, L):
    """alternating over the frame-major rows: the attended keys of a query are a prefix of the rows at every chunk size, so
    every attended set is balanced to within one key (frame_major_ref.census_signs)"""
    return AC.signs(B, H, L)


def census_probes(B, H, hd, L, lead, period, c):
    """attn_census.probe_rows in frame-major rows, the chunk and frame boundaries among the first probes"""
    S = rows_per_frame(L, lead, period)
    edges = []
    for n in range(-(-period // c) + 1):
        edges += [lead + n * c * S - 1, lead + n * c * S]
    for f in range(period + 1):
        edges += [lead + f * S - 1, lead + f * S]
    seen, out = set(), []
    for r in edges + AC.probe_order(L):
        if 0 <= r < L and r not in seen:
            seen.add(r)
            out.append(r)
    idx = (torch.arange(B * H * hd) % L).view(B, H, hd)
    return torch.tensor(out)[idx]


def census(tag, hd, B, H, L, lead, period, c, run=AC.emulate, bwd=True):
    """test_attn_census_cpu.census on the chunk mask, with the signs and probes above"""
    mask = census_mask(B, L, lead, period, c)
    q, k, v = AC.forward_inputs(hd, B, H, L, L)
    o, lse = run(q, k, v, None, mask)[:2]
    AC.check_count(tag, lse, mask)
    AC.check_labels(tag, o, mask)
    if not bwd:
        return
    w = census_signs(B, H, L)
    p = census_probes(B, H, hd, L, lead, period, c)
    q, k, v, do = AC.dkv_probe_inputs(hd, B, H, L, L, p, w)
    o, lse, dq, dk, dv = run(q, k, v, do, mask)
    edv, edk, gap = AC.expect_dkv(mask, p, w, hd)
    assert gap >= AC.MIN_GAP
    AC.check_count(tag + ".dkv", lse, mask)
    AC.check_support_and_values(tag + ".dv", dv, edv, AC.REL_DV)
    AC.check_support_and_values(tag + ".dk", dk, edk, AC.REL_DK)
    AC.check_zero(tag + ".dkv.dq", dq)
    q, k, v, do = AC.dq_probe_inputs(hd, B, H, L, L, p, w)
    o, lse, dq, dk, dv = run(q, k, v, do, mask)
    edq, gap = AC.expect_dq(mask, p, w, hd)
    assert gap >= AC.MIN_GAP
    AC.check_support_and_values(tag + ".dq", dq, edq, AC.REL_DK)
    AC.check_zero(tag + ".dq.dk", dk)


# --------------------------------------------------------------------------------------- models ----
def dit_forward(P, cfg, x, context, timesteps, rope_start, chunk, context_lens=None, reg=None):
    """frame_causal_ref.dit_forward with every self-attention restricted to allowed_tok(L, N_REG, t, chunk); reg [B]: the
    register group's noise level pinned (frame_cache_ref.full_forward), None: the row maximum"""
    B, C, T, Hh, Ww = x.shape
    pt, p = cfg.time_patch_size, cfg.patch_size
    t, h, w = T // pt, Hh // p, Ww // p
    if timesteps.dim() == 1:
        timesteps = timesteps[:, None].expand(B, t)
    assert tuple(timesteps.shape) == (B, t)
    tok = O.patch_embed(x, P["patch_embed.patch_proj.weight"], P["patch_embed.patch_proj.bias"], pt, p)
    tok = torch.cat([P["register_tokens"].expand(B, -1, -1).to(tok.dtype), tok], dim=1)
    L = tok.shape[1]
    gidx = R.group_index(L, N_REG, t)  # the modulation groups stay per frame
    mask = allowed_tok(L, N_REG, t, chunk)
    cos, sin = O.rope_cos_sin(cfg.head_dim, (t, h, w), rope_start)
    lead_t = timesteps.max(dim=1).values if reg is None else torch.as_tensor(reg, dtype=timesteps.dtype)
    c = KC._conditioning(P, cfg, timesteps, lead_t, tok.dtype)
    v_0 = None
    for i in range(cfg.depth):
        tok, v = FC.block_forward(P, f"blocks.{i}.", cfg, tok, context, c, gidx, v_0, cos, sin, mask, context_lens)
        if v_0 is None:
            v_0 = v
    fshift, fscale = R._mods(c, P["final_modulation.1.weight"], P["final_modulation.1.bias"], gidx, 2)
    tok = (O.rms_norm(tok, P.get("final_norm.weight")) * (1 + fscale) + fshift)[:, N_REG:, :]
    y = O.linear(tok, P["final_proj.weight"], P["final_proj.bias"])
    return O.unpatchify(y, C, t, h, w, pt, p)


def chunk_forward(P, cfg, x, context, timesteps, base, reg, cache, chunk, context_lens=None):
    """frame_cache_ref.chunk_forward on a frame_chunk model: x holds k <= chunk token-frames of ONE chunk behind
    cache.past_frames (a multiple of chunk); the self-attention mask is the past mask with one token group, the modulation
    groups stay (N_REG, k)"""
    B, C, T, Hh, Ww = x.shape
    pt, p = cfg.time_patch_size, cfg.patch_size
    k, h, w = T // pt, Hh // p, Ww // p
    assert cache.past_frames % chunk == 0 and k <= chunk and (k == chunk or cache.past_frames + k == cache.frames)
    assert tuple(timesteps.shape) == (B, k)
    tok = O.patch_embed(x, P["patch_embed.patch_proj.weight"], P["patch_embed.patch_proj.bias"], pt, p)
    tok = torch.cat([P["register_tokens"].expand(B, -1, -1).to(tok.dtype), tok], dim=1)
    L = tok.shape[1]
    gidx = R.group_index(L, N_REG, k)
    past = cache.past_frames * h * w
    mask = KC.past_allowed(L, N_REG, 1, past)
    cos, sin = KC.chunk_rope(cfg.head_dim, cache.frames, h, w, base, cache.past_frames, k)
    c = KC._conditioning(P, cfg, timesteps, reg, tok.dtype)
    v_0 = None
    ks, vs = [], []
    for i in range(cfg.depth):
        tok, v, kr = KC._block_chunk(P, f"blocks.{i}.", cfg, tok, context, c, gidx, v_0, cos, sin, mask, cache.k[i],
                                     cache.v[i], context_lens)
        if v_0 is None:
            v_0 = v
        ks.append(kr[:, :, N_REG:])
        vs.append(v[:, :, N_REG:])
    cache.pending = (ks, vs, k)
    fshift, fscale = R._mods(c, P["final_modulation.1.weight"], P["final_modulation.1.bias"], gidx, 2)
    tok = (O.rms_norm(tok, P.get("final_norm.weight")) * (1 + fscale) + fshift)[:, N_REG:, :]
    y = O.linear(tok, P["final_proj.weight"], P["final_proj.bias"])
    return O.unpatchify(y, C, k, h, w, pt, p)


_cases = {}
T_FRAMES = 5  # token-frames of long_case: chunks of 2 are (0, 2), (2, 2), (4, 1) -- a short last chunk
T_LEVELS = [[0.5, 0.96875], [0.25, 0.0625]]


def long_case():
    """the hd64 configuration of frame_cache_ref.model_case on a latent of 5 token-frames ([2,16,10,8,8], 16 tokens each)"""
    if "long" not in _cases:
        cfg, P, _, ctx = KC.model_case("hd64")
        g = torch.Generator().manual_seed(77)
        _cases["long"] = (cfg, P, torch.randn(2, 16, 2 * T_FRAMES, 8, 8, generator=g).to(bf16), ctx)
    return _cases["long"]


def cached_chunk(P, cfg, latent, ctx, n_frames, chunk, f0, k, levels=T_LEVELS):
    """a fresh Cache, the chunks before frame f0 committed through t = 0 calls (one per chunk), then the call on frames
    f0 .. f0 + k - 1 at `levels`.  fp32.  Returns (out, cache)."""
    pt = cfg.time_patch_size
    reg = torch.tensor(KC.REG)
    cache = KC.Cache(cfg.depth, n_frames)
    with torch.no_grad():
        for g0 in range(0, f0, chunk):
            g1 = min(g0 + chunk, n_frames)
            chunk_forward(P, cfg, latent[:, :, g0 * pt:g1 * pt].float(), ctx.float(), torch.zeros(2, g1 - g0), KC.BASE, reg,
                          cache, chunk)
            cache.commit()
        tt = torch.tensor(levels)[:, :k].to(bf16).float()
        out = chunk_forward(P, cfg, latent[:, :, f0 * pt:(f0 + k) * pt].float(), ctx.float(), tt, KC.BASE, reg, cache, chunk)
    return out, cache
