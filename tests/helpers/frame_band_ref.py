"""Frame-band self-attention of the bidirectional model, the reference side (tests/test_frame_band_cpu.py and the GPU
modules).  CPU only, no import of the library: everything here is written from the definitions in include/vds.h.

With `lead` register rows, `period` = t token-frames, a chunk of c token-frames and a band of `band` token-frames on each
side, band % c == 0, b = band // c chunks (notation of frame_chunk_ref):
  a lead query attends every key, and every query attends the lead keys;
  a token query of chunk n attends the token keys of chunks n - b .. n + b.
In frame-major rows, with G = min(c, period) * S and chunk(x) = (x - lead) // G, a token row x has
  lo(x) = lead + max(0, chunk(x) - b) * G
  hi(x) = min(L, lead + (chunk(x) + b + 1) * G)
and query r attends key j iff r < lead, or j < lead, or lo(r) <= j < hi(r).  The relation is symmetric: the readers of
token key j are [0, lead) and [lo(j), hi(j)).  b >= ceil(period / c) - 1 attends every pair.

  allowed_tok / allowed      the dense mask in token rows / in frame-major rows
  lo / hi                    the two bounds of a token row
  fwd_tiles                  the key tiles a forward / dQ workgroup visits: every tile with a lead row in it, else the lead
                             tiles, then [jb, nkt) -- and, the relation being symmetric, the query tiles of a dK/dV workgroup
  mask_by_tiles              the mask as the forward / dQ kernels apply it: the tile ranges, the open test, the compare
  mask_by_key_tiles          ... and as the dK/dV kernels do
  tiles_visited              (visited, all) 64-key tiles of the forward / dQ kernels
  census                     attn_census on the band mask in frame-major rows
  dit_forward                frame_chunk_ref's helper model under the band mask"""
import torch

from oracle import dit_oracle as O

import attn_census as AC
import frame_chunk_ref as CH
import frame_major_ref as FM

KC, FC, R = CH.KC, CH.FC, CH.R
N_REG = FC.N_REG
f32, bf16 = torch.float32, torch.bfloat16

# (L, lead, period, c, band): band in token-frames.  A first workgroup that mixes lead and token rows, short last chunks
# (8 % 3, 7 % 1 ..), runs that start and end inside a 64-row tile, a gap between the lead tiles and the run, chunk edges off
# the tile grid, no lead, two lead tiles, a band that covers every pair
SHAPES = [(166, 16, 3, 1, 1), (280, 16, 8, 1, 1), (280, 16, 8, 1, 0), (280, 16, 8, 2, 2), (280, 16, 8, 3, 3),
          (280, 16, 8, 1, 7), (203, 0, 7, 1, 2), (140, 5, 3, 1, 1), (293, 33, 4, 1, 1), (656, 80, 9, 1, 2),
          (1040, 16, 8, 1, 1), (1040, 16, 8, 2, 2)]
TILES = FM.TILES
ids = lambda s: "L{}_{}_{}_c{}_b{}".format(*s)


def chunks_of(c, band):
    assert band % c == 0 and band >= 0
    return band // c


def covers(period, c, band):
    """the band attends every pair"""
    return chunks_of(c, band) >= -(-period // c) - 1


def rows_per_frame(L, lead, period):
    return CH.rows_per_frame(L, lead, period)


def _band(g, b):
    """groups [L] (0: lead, 1 + chunk) -> bool [L, L]"""
    gq, gk = g[:, None], g[None, :]
    return (gq == 0) | (gk == 0) | ((gk - gq).abs() <= b)


def allowed_tok(L, lead, period, c, band):
    """bool [L, L] in token rows"""
    return _band(CH.group_index_tok(L, lead, period, c), chunks_of(c, band))


def allowed(L, lead, period, c, band):
    """bool [L, L] in frame-major rows"""
    S = rows_per_frame(L, lead, period)
    r = torch.arange(L)
    g = torch.where(r < lead, torch.zeros_like(r), 1 + (r - lead).clamp(min=0) // (min(c, period) * S))
    return _band(g, chunks_of(c, band))


def lo(x, lead, S, c, b, period=None):
    """the first token row that token row x attends and is attended by"""
    assert x >= lead
    G = (c if period is None else min(c, period)) * S
    return lead + max(0, (x - lead) // G - b) * G


def hi(x, lead, S, c, b, L, period=None):
    """one past the last token row that token row x attends and is attended by"""
    assert x >= lead
    G = (c if period is None else min(c, period)) * S
    return min(L, lead + ((x - lead) // G + b + 1) * G)


def fwd_tiles(q0, q1, lead, S, c, b, L, ktile=64):
    """(nl, jb, nkt): a workgroup with rows [q0, q1) visits the tiles [0, nl) and [jb, nkt) of the other side"""
    if q0 < lead:
        nkt = -(-L // ktile)
        return nkt, nkt, nkt
    nkt = -(-hi(q1 - 1, lead, S, c, b, L) // ktile)
    nl = min(nkt, -(-lead // ktile))
    jb = max(nl, lo(q0, lead, S, c, b) // ktile)
    assert nl <= jb <= nkt
    return nl, jb, nkt


def _bounds(L, lead, S, c, b):
    """per row: (pend, lo, hi) -- a lead row keeps everything below pend = L and has an empty run at L"""
    pend = torch.tensor([L if x < lead else lead for x in range(L)])
    lo_ = torch.tensor([L if x < lead else lo(x, lead, S, c, b) for x in range(L)])
    hi_ = torch.tensor([L if x < lead else hi(x, lead, S, c, b, L) for x in range(L)])
    return pend, lo_, hi_


def _walk(L, lead, period, c, band, tile, wave_rows, sub, ktile):
    """[own row, other row]: a workgroup of `tile` own rows visits the tiles of fwd_tiles; a wave of wave_rows own rows takes
    a sub-block of `sub` other rows without a compare when it holds lead rows only and the sub-block ends at or below L, or
    when it holds token rows only and the sub-block lies wholly below lead or wholly inside [lo of the wave's last row, hi
    of its first); every other element is kept iff other < pend(own) or lo(own) <= other < hi(own).  Also returns whether
    every workgroup's second range is tight (its first tile holds a row its first own row attends)."""
    S = rows_per_frame(L, lead, period)
    b = chunks_of(c, band)
    c = min(c, period)
    pend, lo_, hi_ = _bounds(L, lead, S, c, b)
    other = torch.arange(L)
    out = torch.zeros(L, L, dtype=torch.bool)
    tight = True
    for q0 in range(0, L, tile):
        q1 = min(q0 + tile, L)
        nl, jb, nkt = fwd_tiles(q0, q1, lead, S, c, b, L, ktile)
        visited = list(range(nl)) + list(range(jb, nkt))
        assert len(set(visited)) == len(visited)
        if jb < nkt:
            tight &= jb == nl or jb * ktile <= int(lo_[q0]) < (jb + 1) * ktile
        for w0 in range(q0, q1, wave_rows):
            w1 = min(w0 + wave_rows, q1)
            wl = min(w0 + wave_rows, L) - 1  # the wave's last row
            wlead = wkbeg = wkend = 0
            if wl < lead:
                wlead = L
            elif w0 >= lead:
                wlead, wkbeg, wkend = lead, int(lo_[wl]), int(hi_[w0])
            for j in visited:
                for k0 in range(j * ktile, min((j + 1) * ktile, L), sub):
                    k1 = min(k0 + sub, L)
                    if k0 + sub <= wlead or (k0 >= wkbeg and k0 + sub <= wkend):
                        out[w0:w1, k0:k1] = True
                    else:
                        kk = other[None, k0:k1]
                        out[w0:w1, k0:k1] = (kk < pend[w0:w1, None]) | ((kk >= lo_[w0:w1, None]) & (kk < hi_[w0:w1, None]))
    return out, tight


def mask_by_tiles(L, lead, period, c, band, tile, wave_rows=32, sub=32, ktile=64):
    """forward / dQ kernels: [query, key] (see _walk), and whether every second range is tight"""
    return _walk(L, lead, period, c, band, tile, wave_rows, sub, ktile)


def mask_by_key_tiles(L, lead, period, c, band, tile, qtile=64, wave_keys=32, sub=32):
    """dK/dV kernels: a workgroup of `tile` keys sweeps the query tiles of fwd_tiles -- the relation is symmetric and so is
    the walk --; [query, key]"""
    return _walk(L, lead, period, c, band, tile, wave_keys, sub, qtile)[0].T


def tiles_visited(L, lead, period, c, band, tile=64, qtile=128):
    """(visited, all) key tiles of `tile` rows summed over the query tiles of `qtile` rows (forward / dQ kernels; the query
    tiles of the dK/dV kernel are the same count)"""
    S = rows_per_frame(L, lead, period)
    b = chunks_of(c, band)
    vis = tot = 0
    for q0 in range(0, L, qtile):
        q1 = min(q0 + qtile, L)
        nl, jb, nkt = fwd_tiles(q0, q1, lead, S, min(c, period), b, L, tile)
        vis += nl + nkt - jb
        tot += -(-L // tile)
    return vis, tot


# ---------------------------------------------------------------------------- census, frame-major ----
def census_mask(B, L, lead, period, c, band):
    return allowed(L, lead, period, c, band)[None].expand(B, L, L)


def census_signs(B, H, L):
    """alternating over the frame-major rows: the attended keys of a query are all rows, or two contiguous runs of rows --
    the lead rows and its band -- so every attended set is balanced to within two keys"""
    return AC.signs(B, H, L)


def census_probes(B, H, hd, L, lead, period, c):
    """frame_chunk_ref's probes: lo and hi are chunk boundaries, which come first there"""
    return CH.census_probes(B, H, hd, L, lead, period, c)


def census(tag, hd, B, H, shape, run=AC.emulate, bwd=True, mask=None):
    """frame_chunk_ref.census on the band mask (mask: another one to hold `run` against, for the defect tests)"""
    L, lead, period, c, band = shape
    if mask is None:
        mask = census_mask(B, L, lead, period, c, band)
    q, k, v = AC.forward_inputs(hd, B, H, L, L)
    o, lse = run(q, k, v, None, mask)[:2]
    AC.check_count(tag, lse, mask)
    AC.check_labels(tag, o, mask)
    if not bwd:
        return
    sg = census_signs(B, H, L)
    p = census_probes(B, H, hd, L, lead, period, c)
    q, k, v, do = AC.dkv_probe_inputs(hd, B, H, L, L, p, sg)
    o, lse, dq, dk, dv = run(q, k, v, do, mask)
    edv, edk, gap = AC.expect_dkv(mask, p, sg, hd)
    assert gap >= AC.MIN_GAP
    AC.check_count(tag + ".dkv", lse, mask)
    AC.check_support_and_values(tag + ".dv", dv, edv, AC.REL_DV)
    AC.check_support_and_values(tag + ".dk", dk, edk, AC.REL_DK)
    AC.check_zero(tag + ".dkv.dq", dq)
    q, k, v, do = AC.dq_probe_inputs(hd, B, H, L, L, p, sg)
    o, lse, dq, dk, dv = run(q, k, v, do, mask)
    edq, gap = AC.expect_dq(mask, p, sg, hd)
    assert gap >= AC.MIN_GAP
    AC.check_support_and_values(tag + ".dq", dq, edq, AC.REL_DK)
    AC.check_zero(tag + ".dq.dk", dk)


# --------------------------------------------------------------------------------------- models ----
def dit_forward(P, cfg, x, context, timesteps, rope_start, chunk, band, context_lens=None, reg=None):
    """frame_chunk_ref.dit_forward with every self-attention restricted to allowed_tok(L, N_REG, t, chunk, band); [B]
    timesteps run as constant rows, which the per-frame conditioning reproduces"""
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
    mask = allowed_tok(L, N_REG, t, chunk, band)
    cos, sin = O.rope_cos_sin(cfg.head_dim, (t, h, w), rope_start)
    lead_t = timesteps.max(dim=1).values if reg is None else torch.as_tensor(reg, dtype=timesteps.dtype)
    cv = KC._conditioning(P, cfg, timesteps, lead_t, tok.dtype)
    v_0 = None
    for i in range(cfg.depth):
        tok, v = FC.block_forward(P, f"blocks.{i}.", cfg, tok, context, cv, gidx, v_0, cos, sin, mask, context_lens)
        if v_0 is None:
            v_0 = v
    fshift, fscale = R._mods(cv, P["final_modulation.1.weight"], P["final_modulation.1.bias"], gidx, 2)
    tok = (O.rms_norm(tok, P.get("final_norm.weight")) * (1 + fscale) + fshift)[:, N_REG:, :]
    y = O.linear(tok, P["final_proj.weight"], P["final_proj.bias"])
    return O.unpatchify(y, C, t, h, w, pt, p)
