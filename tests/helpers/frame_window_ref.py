"""Sliding-window chunk-causal self-attention, the reference side (tests/test_frame_window_cpu.py and the GPU modules).
CPU only, no import of the library: everything here is written from the definitions in include/vds.h.

With `lead` register rows, `period` = t token-frames, a chunk of c token-frames and a window of w token-frames, w % c == 0,
W = w // c >= 1 chunks (notation of frame_chunk_ref):
  a lead query attends the lead keys only;
  a token query of chunk n attends every lead key and the token keys of chunks max(0, n - W + 1) .. n.
In frame-major rows, with G = c * S and chunk(r) = (r - lead) // G:
  kbeg(r) = lead + max(0, chunk(r) - W + 1) * G     query r attends [0, lead) and [kbeg(r), kend(r))
  qend(j) = min(L, lead + (chunk(j) + W) * G)       key j >= lead is attended by [qstart(j), qend(j)); a lead key by all
kend / qstart are frame_chunk_ref's.  W >= ceil(period / c) is the chunk mask.

  allowed_tok / allowed      the dense mask in token rows / in frame-major rows
  key_begin / query_end      the two new bounds
  fwd_tiles                  the key tiles a forward / dQ workgroup visits: the lead tiles, then [jb, nkt)
  mask_by_tiles              the mask as the forward / dQ kernels apply it: the two tile ranges, the open test, the compare
  mask_by_key_tiles          ... and as the dK/dV kernels do: the sweep [qstart tile, qend tile) or, with a lead key in
                             the workgroup, every tile; the open test; the per-lane compare
  tiles_visited              (visited, all) 64-key tiles of the forward / dQ kernels
  census                     attn_census on the window mask in frame-major rows
  dit_forward                frame_chunk_ref's helper model under the window mask
  Ring / ring_forward        the ring cache: W slots of one chunk each, chunk n in slot n % W, the keys in buffer order"""
import torch

from oracle import dit_oracle as O

import attn_census as AC
import frame_chunk_ref as CH
import frame_major_ref as FM

KC, FC, R = CH.KC, CH.FC, CH.R
N_REG = FC.N_REG
f32, bf16 = torch.float32, torch.bfloat16

# (L, lead, period, c, w): w in token-frames
SHAPES = [(166, 16, 3, 1, 2), (280, 16, 8, 1, 3), (280, 16, 8, 2, 4), (280, 16, 8, 3, 3), (280, 16, 8, 3, 6),
          (203, 0, 7, 1, 2), (140, 5, 3, 1, 1), (293, 33, 4, 1, 2), (656, 80, 9, 1, 2), (1024, 0, 4, 1, 1),
          (1040, 16, 8, 1, 2), (1040, 16, 8, 2, 2)]
TILES = FM.TILES
ids = lambda s: "L{}_{}_{}_c{}_w{}".format(*s)


def chunks_of(c, w):
    assert w % c == 0 and w >= c
    return w // c


def rows_per_frame(L, lead, period):
    return CH.rows_per_frame(L, lead, period)


def _window(g, W):
    """groups [L] (0: lead, 1 + chunk) -> bool [L, L]"""
    gq, gk = g[:, None], g[None, :]
    return (gk <= gq) & ((gk == 0) | (gk > gq - W))


def allowed_tok(L, lead, period, c, w):
    """bool [L, L] in token rows"""
    return _window(CH.group_index_tok(L, lead, period, c), chunks_of(c, w))


def allowed(L, lead, period, c, w):
    """bool [L, L] in frame-major rows"""
    S = rows_per_frame(L, lead, period)
    r = torch.arange(L)
    g = torch.where(r < lead, torch.zeros_like(r), 1 + (r - lead).clamp(min=0) // (c * S))
    return _window(g, chunks_of(c, w))


def key_begin(r, lead, S, c, W):
    """the first token key row query row r attends (lead for a lead query: it attends none)"""
    if r < lead:
        return lead
    G = c * S
    return lead + max(0, (r - lead) // G - W + 1) * G


def query_end(j, lead, S, c, W, L):
    """one past the last query row that attends key row j"""
    if j < lead:
        return L
    G = c * S
    return min(L, lead + ((j - lead) // G + W) * G)


def fwd_tiles(q0, q1, lead, S, c, W, L, ktile=64):
    """(nl, jb, nkt): a forward / dQ workgroup with query rows [q0, q1) visits the key tiles [0, nl) and [jb, nkt)"""
    lk = CH.key_end(q0, q1, lead, S, c, L)
    nkt = -(-lk // ktile)
    nl = min(nkt, -(-lead // ktile))
    qf = max(q0, lead)
    jb = max(nl, key_begin(qf, lead, S, c, W) // ktile) if qf < q1 else nkt
    assert nl <= jb <= nkt
    return nl, jb, nkt


def mask_by_tiles(L, lead, period, c, w, tile, wave_rows=32, sub=32, ktile=64):
    """forward / dQ kernels: a workgroup of `tile` queries visits the tiles of fwd_tiles; a wave of wave_rows queries from w0
    takes a sub-block of `sub` keys without a compare when w0 is a token row and the sub-block lies wholly below lead or
    wholly inside [kbeg of the wave's last query, kend of its first); every other element is kept iff key < lead or
    kbeg(query) <= key < kend(query).  Also returns whether every workgroup's second range is tight (its first tile holds
    a key that its first token query attends)."""
    S = rows_per_frame(L, lead, period)
    W = chunks_of(c, w)
    kend = torch.tensor([CH.key_end(q, q + 1, lead, S, c, L) for q in range(L)])
    kbeg = torch.tensor([key_begin(q, lead, S, c, W) for q in range(L)])
    keys = torch.arange(L)
    out = torch.zeros(L, L, dtype=torch.bool)
    tight = True
    for q0 in range(0, L, tile):
        q1 = min(q0 + tile, L)
        nl, jb, nkt = fwd_tiles(q0, q1, lead, S, c, W, L, ktile)
        visited = list(range(nl)) + list(range(jb, nkt))
        assert len(set(visited)) == len(visited)
        if jb < nkt:
            qf = max(q0, lead)
            tight &= jb == nl or jb * ktile <= int(kbeg[qf]) < (jb + 1) * ktile
        for w0 in range(q0, q1, wave_rows):
            w1 = min(w0 + wave_rows, q1)
            tokens = w0 >= lead
            wlead = lead if tokens else 0
            wkend = int(kend[w0]) if tokens else 0
            wkbeg = int(kbeg[min(w0 + wave_rows, L) - 1])
            for j in visited:
                for k0 in range(j * ktile, min((j + 1) * ktile, L), sub):
                    k1 = min(k0 + sub, L)
                    if k0 + sub <= wlead or (k0 >= wkbeg and k0 + sub <= wkend):
                        out[w0:w1, k0:k1] = True
                    else:
                        kk = keys[None, k0:k1]
                        out[w0:w1, k0:k1] = (kk < lead) | ((kk >= kbeg[w0:w1, None]) & (kk < kend[w0:w1, None]))
    return out, tight


def mask_by_key_tiles(L, lead, period, c, w, tile, qtile=64, wave_keys=32, sub=32):
    """dK/dV kernels: a workgroup of `tile` keys from k0 sweeps every qtile-row query tile if k0 < lead, else the tiles from
    the one that holds qstart(k0) to the one below qend of its last key; a wave of wave_keys keys takes a sub-block of `sub`
    queries without a compare when it starts at or past qstart of the wave's last key and ends at or below qend of its first
    TOKEN key (the smallest of the wave: a lead key's is L);
    every other element is kept iff qstart(key) <= query < qend(key)"""
    S = rows_per_frame(L, lead, period)
    W = chunks_of(c, w)
    qstart = torch.tensor([CH.query_start(k, lead, S, c) for k in range(L)])
    qend = torch.tensor([query_end(k, lead, S, c, W, L) for k in range(L)])
    rows = torch.arange(L)
    out = torch.zeros(L, L, dtype=torch.bool)
    for k0 in range(0, L, tile):
        k1 = min(k0 + tile, L)
        first = CH.query_start(k0, lead, S, c) // qtile * qtile
        last = L if k0 < lead else min(L, -(-query_end(k1 - 1, lead, S, c, W, L) // qtile) * qtile)
        assert first < last
        for w0 in range(k0, k1, wave_keys):
            w1 = min(w0 + wave_keys, k1)
            wqlim = CH.query_start(min(w0 + wave_keys - 1, L - 1), lead, S, c)
            wqhi = query_end(min(max(w0, lead), w0 + wave_keys - 1, L - 1), lead, S, c, W, L)  # the first token key's
            for q0 in range(first, last, sub):
                q1 = min(q0 + sub, L)
                if q0 >= wqlim and q0 + sub <= wqhi:
                    out[q0:q1, w0:w1] = True
                else:
                    rr = rows[q0:q1, None]
                    out[q0:q1, w0:w1] = (rr >= qstart[None, w0:w1]) & (rr < qend[None, w0:w1])
    return out


def tiles_visited(L, lead, period, c, w, tile=64, qtile=128):
    """(visited, all) key tiles of `tile` rows summed over the query tiles of `qtile` rows (forward / dQ kernels)"""
    S = rows_per_frame(L, lead, period)
    W = chunks_of(c, w)
    vis = tot = 0
    for q0 in range(0, L, qtile):
        q1 = min(q0 + qtile, L)
        nl, jb, nkt = fwd_tiles(q0, q1, lead, S, c, W, L, tile)
        vis += nl + nkt - jb
        tot += -(-L // tile)
    return vis, tot


def query_tiles_visited(L, lead, period, c, w, tile=128, qtile=64):
    """(visited, all) query tiles of `qtile` rows summed over the key tiles of `tile` rows (dK/dV kernels)"""
    S = rows_per_frame(L, lead, period)
    W = chunks_of(c, w)
    vis = tot = 0
    for k0 in range(0, L, tile):
        k1 = min(k0 + tile, L)
        first = CH.query_start(k0, lead, S, c) // qtile
        last = -(-L // qtile) if k0 < lead else -(-query_end(k1 - 1, lead, S, c, W, L) // qtile)
        vis += last - first
        tot += -(-L // qtile)
    return vis, tot


# ---------------------------------------------------------------------------- census, frame-major ----
def census_mask(B, L, lead, period, c, w):
    return allowed(L, lead, period, c, w)[None].expand(B, L, L)


def census_signs(B, H, L):
    """alternating over the frame-major rows: the attended keys of a query are two contiguous runs of rows -- the lead rows
    and its window -- so every attended set is balanced to within two keys"""
    return AC.signs(B, H, L)


def census_probes(B, H, hd, L, lead, period, c):
    """frame_chunk_ref's probes: the window's bounds kbeg / qend are chunk boundaries, which come first there"""
    return CH.census_probes(B, H, hd, L, lead, period, c)


def census(tag, hd, B, H, shape, run=AC.emulate, bwd=True):
    """frame_chunk_ref.census on the window mask"""
    L, lead, period, c, w = shape
    mask = census_mask(B, L, lead, period, c, w)
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
def dit_forward(P, cfg, x, context, timesteps, rope_start, chunk, window, context_lens=None, reg=None):
    """frame_chunk_ref.dit_forward with every self-attention restricted to allowed_tok(L, N_REG, t, chunk, window)"""
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
    mask = allowed_tok(L, N_REG, t, chunk, window)
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


def ring_rows(W, c, h, w):
    """rows of a ring cache buffer: the registers and W slots of one chunk"""
    return N_REG + W * c * h * w


class Ring:
    """per block: W slots of k, v rows [B, H, c*h*w, hd]; chunk n lives in slot n % W.  past_frames counts the committed
    token-frames of the whole video, as in frame_cache_ref.Cache"""

    def __init__(self, depth, frames, chunk, W):
        self.frames, self.chunk, self.W = frames, chunk, W
        self.k = [[None] * W for _ in range(depth)]
        self.v = [[None] * W for _ in range(depth)]
        self.past_frames = 0
        self.pending = None

    def commit(self):
        self.past_frames += self.pending
        self.pending = None


def ring_forward(P, cfg, x, context, timesteps, base, reg, ring, context_lens=None):
    """the helper model on ONE chunk behind ring.past_frames: the chunk's K / V go to slot n % W first, then every token query
    attends the register keys and the slots in BUFFER order -- the first min(n, W - 1) + 1 slots while the ring fills (the
    own slot is then the last of them), all W once it is full, wherever the own slot sits among them"""
    B, C, T, Hh, Ww = x.shape
    pt, p = cfg.time_patch_size, cfg.patch_size
    k, h, w = T // pt, Hh // p, Ww // p
    c, W = ring.chunk, ring.W
    assert ring.past_frames % c == 0 and k <= c and (k == c or ring.past_frames + k == ring.frames)
    n = ring.past_frames // c
    assert tuple(timesteps.shape) == (B, k)
    tok = O.patch_embed(x, P["patch_embed.patch_proj.weight"], P["patch_embed.patch_proj.bias"], pt, p)
    tok = torch.cat([P["register_tokens"].expand(B, -1, -1).to(tok.dtype), tok], dim=1)
    L = tok.shape[1]
    gidx = R.group_index(L, N_REG, k)
    cos, sin = KC.chunk_rope(cfg.head_dim, ring.frames, h, w, base, ring.past_frames, k)
    cv = KC._conditioning(P, cfg, timesteps, reg, tok.dtype)
    H = cfg.num_heads
    used = min(n, W - 1) + 1
    v_0 = None
    for i in range(cfg.depth):
        pre = f"blocks.{i}."
        g = lambda name: P.get(pre + name)
        (shift_sa, scale_sa, gate_sa, shift_ca, scale_ca, gate_ca,
         shift_mlp, scale_mlp, gate_mlp) = R._mods(cv, g("adaLN_modulation.1.weight"), g("adaLN_modulation.1.bias"), gidx, 9)
        xn = O.rms_norm(tok, g("norm1.weight")) * (1 + scale_sa) + shift_sa
        q, kk, v = O.split_heads(O.linear(xn, g("qkv.weight"), g("qkv.bias")), 3, H)
        if cfg.residual_v and v_0 is not None:
            lam = g("lambda_param")
            v = lam * v + (1 - lam) * v_0
        qr, kr = O.apply_rotary(q, cos, sin), O.apply_rotary(kk, cos, sin)
        ring.k[i][n % W], ring.v[i][n % W] = kr[:, :, N_REG:], v[:, :, N_REG:]
        K = torch.cat([kr[:, :, :N_REG]] + ring.k[i][:used], dim=2)
        V = torch.cat([v[:, :, :N_REG]] + ring.v[i][:used], dim=2)
        Lk = K.shape[2]
        mask = torch.ones(L, Lk, dtype=torch.bool)
        mask[:N_REG, N_REG:] = False  # a register query attends the register keys only
        att = O.merge_heads(FC.masked_attention(qr, K, V, mask)[0])
        x1 = tok + O.linear(att, g("attn_proj.weight")) * gate_sa
        x2 = x1
        if g("q_cross.weight") is not None:
            xn2 = O.rms_norm(x1, g("norm2.weight")) * (1 + scale_ca) + shift_ca
            (qc,) = O.split_heads(O.linear(xn2, g("q_cross.weight"), g("q_cross.bias")), 1, H)
            kc, vc = O.split_heads(O.linear(context, g("context_kv.weight"), g("context_kv.bias")), 2, H)
            x2 = x1 + O.linear(O.merge_heads(FC.cross_attention(qc, kc, vc, context_lens)), g("cross_proj.weight")) * gate_ca
        xn3 = O.rms_norm(x2, g("norm3.weight")) * (1 + scale_mlp) + shift_mlp
        hmid = O.gelu_erf(O.linear(xn3, g("mlp.0.weight"), g("mlp.0.bias")))
        tok = x2 + O.linear(hmid, g("mlp.2.weight"), g("mlp.2.bias")) * gate_mlp
        if v_0 is None:
            v_0 = v
    ring.pending = k
    fshift, fscale = R._mods(cv, P["final_modulation.1.weight"], P["final_modulation.1.bias"], gidx, 2)
    tok = (O.rms_norm(tok, P.get("final_norm.weight")) * (1 + fscale) + fshift)[:, N_REG:, :]
    y = O.linear(tok, P["final_proj.weight"], P["final_proj.bias"])
    return O.unpatchify(y, C, k, h, w, pt, p)


_cases = {}


def long_case(frames):
    """the hd64 configuration of frame_cache_ref.model_case on a latent of `frames` token-frames of 16 tokens"""
    if frames not in _cases:
        cfg, P, _, ctx = KC.model_case("hd64")
        g = torch.Generator().manual_seed(700 + frames)
        _cases[frames] = (cfg, P, torch.randn(2, 16, 2 * frames, 8, 8, generator=g).to(bf16), ctx)
    return _cases[frames]


def ring_rollout(P, cfg, latent, ctx, frames, chunk, window, levels):
    """every chunk of the video through the ring: the chunk at `levels` [2] first (its output is kept), then at t = 0 and
    committed.  fp32.  Returns the list of the chunks' outputs."""
    pt = cfg.time_patch_size
    reg = torch.tensor(KC.REG)
    ring = Ring(cfg.depth, frames, chunk, chunks_of(chunk, window))
    outs = []
    with torch.no_grad():
        for f0 in range(0, frames, chunk):
            f1 = min(f0 + chunk, frames)
            x = latent[:, :, f0 * pt:f1 * pt].float()
            tt = torch.tensor(levels)[:, None].expand(2, f1 - f0).to(bf16).float()
            outs.append(ring_forward(P, cfg, x, ctx.float(), tt, KC.BASE, reg, ring))
            ring_forward(P, cfg, x, ctx.float(), torch.zeros(2, f1 - f0), KC.BASE, reg, ring)
            ring.commit()
    return outs
