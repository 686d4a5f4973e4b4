"""Teacher forcing (the clean-context attention mask), the reference side (tests/test_teacher_cpu.py and the GPU modules).
CPU only, no import of the library: everything here is written from the definitions in include/vds.h.

A sample's rows are [lead register rows | n clean token-frames | their n noisy copies]: period = 2n token-frames, S rows per
frame, a chunk of c token-frames, G = min(c, n) * S rows, base = lead + n * S the first noisy row (frame-major rows).  For
a token row r, half(r) = r >= base and chunk(r) = (r - lead - half(r) * n * S) // G: chunks restart at base, the last chunk
of each half may be short.  Query r attends key j iff
  j < lead                                                  (a lead query attends nothing else)
  r clean:  j clean and chunk(j) <= chunk(r)                (the chunk-causal mask of the first base rows)
  r noisy:  j clean and chunk(j) < chunk(r), or j noisy and chunk(j) == chunk(r).

  allowed / allowed_tok      the dense mask in frame-major rows (a double loop over the definition) / in token rows
  query_bounds               (pend, kbeg, kend) of a query: it attends [0, pend) and [kbeg, kend)
  key_bounds                 (qstart, qend, q2) of a key: its readers are [qstart, qend) and [q2, L) -- a hole for a clean key
  fwd_tiles / key_sweep      the two tile ranges of a forward / dQ workgroup and of a dK/dV workgroup
  mask_by_tiles              the mask as the forward / dQ kernels apply it: the tile ranges, the open test, the compare
  mask_by_key_tiles          ... and as the dK/dV kernel does
  tiles_visited / query_tiles_visited / pairs_q / pairs_k      what the sweeps visit (pairs: the profiler's credit)
  census                     attn_census on the teacher mask in frame-major rows
  dit_forward                the fp32 helper model on the doubled sequence, token-frame n + f on the RoPE rows of frame f"""
import torch

from oracle import dit_oracle as O

import attn_census as AC
import frame_chunk_ref as CH
import frame_major_ref as FM

KC, FC, R = CH.KC, CH.FC, CH.R
N_REG = FC.N_REG
f32, bf16 = torch.float32, torch.bfloat16

LEAD = 16


def shape_of(n, S, c, lead=LEAD):
    """(L, lead, period, c) of n clean + n noisy frames of S rows"""
    return (lead + 2 * n * S, lead, 2 * n, c)


# (n, S, c) -> (L, lead, period, c): base and the chunk edges inside 32-key sub-blocks, 64-row and 128-row tiles; a workgroup
# that straddles base; one wholly in the noisy half behind a gap of key tiles (568: noisy chunk 1 visits the tile that ends
# at row 64 and resumes at the one that holds row 338); a short last chunk (316); one chunk per half (108)
NSC = [(3, 23, 1), (4, 46, 2), (3, 50, 2), (5, 64, 1), (6, 46, 1), (2, 23, 4)]
SHAPES = [shape_of(*s) for s in NSC]
# further shapes for the CPU proofs: no lead rows, a lead that is no multiple of anything, S = 1, several tiles per chunk
CPU_SHAPES = SHAPES + [(0 + 2 * 3 * 29, 0, 6, 1), (5 + 2 * 4 * 17, 5, 8, 3), (33 + 2 * 2 * 65, 33, 4, 1), (16 + 2 * 7, 16, 14, 2),
                       (16 + 2 * 2 * 512, 16, 4, 1)]
TILES = FM.TILES
ids = lambda s: "L{}_{}_{}_c{}".format(*s)


def geometry(L, lead, period, c):
    """(n, S, G, base)"""
    assert period % 2 == 0 and (L - lead) % period == 0
    n = period // 2
    S = max((L - lead) // period, 1)
    return n, S, min(c, n) * S, lead + n * S


def half_chunk(r, lead, base, G):
    """(half, chunk) of token row r >= lead"""
    half = r >= base
    return half, (r - (base if half else lead)) // G


_dense = {}


def allowed(L, lead, period, c):
    """bool [L, L] in frame-major rows, by a double loop over the definition"""
    key = (L, lead, period, c)
    if key not in _dense:
        n, S, G, base = geometry(L, lead, period, c)
        rows = []
        for r in range(L):
            row = [False] * L
            for j in range(L):
                if j < lead:
                    row[j] = True
                elif r < lead:
                    row[j] = False
                else:
                    hr, cr = half_chunk(r, lead, base, G)
                    hj, cj = half_chunk(j, lead, base, G)
                    if not hr:
                        row[j] = (not hj) and cj <= cr
                    else:
                        row[j] = (cj < cr) if not hj else (cj == cr)
            rows.append(row)
        _dense[key] = torch.tensor(rows)
    return _dense[key]


def allowed_tok(L, lead, period, c):
    """bool [L, L] in token rows: row l >= lead belongs to token-frame (l - lead) % period"""
    n = period // 2
    cc = min(c, n)
    l = torch.arange(L)
    f = (l - lead).clamp(min=0) % period
    is_lead = l < lead
    noisy = (f >= n) & ~is_lead
    ch = (f - n * noisy.long()) // cc
    q_lead, k_lead = is_lead[:, None], is_lead[None, :]
    qn, kn = noisy[:, None], noisy[None, :]
    cq, ck = ch[:, None], ch[None, :]
    clean_q = ~kn & (ck <= cq)
    noisy_q = (~kn & (ck < cq)) | (kn & (ck == cq))
    return k_lead | (~q_lead & ~k_lead & torch.where(qn, noisy_q, clean_q))


def query_bounds(r, L, lead, period, c):
    """(pend, kbeg, kend): query r attends [0, pend) and [kbeg, kend); an empty run is kbeg = kend = pend"""
    n, S, G, base = geometry(L, lead, period, c)
    if r < lead:
        return lead, lead, lead
    half, ch = half_chunk(r, lead, base, G)
    if not half:
        pend = min(base, lead + (ch + 1) * G)
        return pend, pend, pend
    return lead + ch * G, base + ch * G, min(L, base + (ch + 1) * G)


def key_bounds(j, L, lead, period, c):
    """(qstart, qend, q2): key j is read by [qstart, qend) and [q2, L)"""
    n, S, G, base = geometry(L, lead, period, c)
    if j < lead:
        return 0, L, L
    half, ch = half_chunk(j, lead, base, G)
    if not half:
        return lead + ch * G, base, min(L, base + (ch + 1) * G)
    return base + ch * G, min(L, base + (ch + 1) * G), L


def mask_from_query_bounds(L, lead, period, c):
    out = torch.zeros(L, L, dtype=torch.bool)
    for r in range(L):
        pend, kbeg, kend = query_bounds(r, L, lead, period, c)
        out[r, :pend] = True
        out[r, kbeg:kend] = True
    return out


def mask_from_key_bounds(L, lead, period, c):
    out = torch.zeros(L, L, dtype=torch.bool)
    for j in range(L):
        qstart, qend, q2 = key_bounds(j, L, lead, period, c)
        out[qstart:qend, j] = True
        out[q2:, j] = True
    return out


def fwd_tiles(q0, q1, L, lead, period, c, ktile=64):
    """(nl, jb, nkt): a forward / dQ workgroup with query rows [q0, q1) visits the key tiles [0, nl) -- below its largest
    pend -- and [jb, nkt) -- from its smallest kbeg to its largest kend"""
    n, S, G, base = geometry(L, lead, period, c)
    nkt = -(-query_bounds(q1 - 1, L, lead, period, c)[2] // ktile)
    last_prefix = (min(q1, base) - 1) if q0 < base else q1 - 1
    nl = -(-query_bounds(last_prefix, L, lead, period, c)[0] // ktile)
    jb = max(nl, query_bounds(max(q0, base), L, lead, period, c)[1] // ktile) if q1 > base else nkt
    assert nl <= jb <= nkt
    return nl, jb, nkt


def key_sweep(k0, k1, L, lead, period, c, qtile=64):
    """(a0, a1, b0, nqt): a dK/dV workgroup with key rows [k0, k1) sweeps the query tiles [a0, a1) and [b0, nqt)"""
    nqt = -(-L // qtile)
    if k0 < lead:
        return 0, nqt, nqt, nqt
    a0 = key_bounds(k0, L, lead, period, c)[0] // qtile
    a1 = -(-key_bounds(k1 - 1, L, lead, period, c)[1] // qtile)
    q2 = key_bounds(k0, L, lead, period, c)[2]
    b0 = nqt if q2 >= L else max(a1, q2 // qtile)
    assert a0 < a1 <= b0 <= nqt
    return a0, a1, b0, nqt


def mask_by_tiles(L, lead, period, c, tile, wave_rows=32, sub=32, ktile=64):
    """forward / dQ kernels: a workgroup of `tile` queries visits the tiles of fwd_tiles (never one twice: asserted); a wave of
    wave_rows queries takes a sub-block of `sub` keys without a compare when the wave lies wholly in one half (no lead
    query) and the keys lie wholly below its first query's pend or -- a noisy wave -- wholly inside [kbeg of its last query,
    kend of its first); every other element is kept iff key < pend or kbeg <= key < kend of its own query"""
    n, S, G, base = geometry(L, lead, period, c)
    qb = [query_bounds(r, L, lead, period, c) for r in range(L)]
    pend, kbeg, kend = (torch.tensor([b[i] for b in qb]) for i in range(3))
    keys = torch.arange(L)
    out = torch.zeros(L, L, dtype=torch.bool)
    for q0 in range(0, L, tile):
        q1 = min(q0 + tile, L)
        nl, jb, nkt = fwd_tiles(q0, q1, L, lead, period, c, ktile)
        visited = list(range(nl)) + list(range(jb, nkt))
        assert len(set(visited)) == len(visited)
        for w0 in range(q0, q1, wave_rows):
            w1 = min(w0 + wave_rows, q1)
            wl = min(w0 + wave_rows, L) - 1
            noisy, clean = w0 >= base, w0 >= lead and wl < base
            wpend = qb[w0][0] if (noisy or clean) else 0
            wkbeg = qb[wl][1] if noisy else 0
            wkend = qb[w0][2] if noisy else 0
            for j in visited:
                for k0 in range(j * ktile, min((j + 1) * ktile, L), sub):
                    k1 = min(k0 + sub, L)
                    if k0 + sub <= wpend or (k0 >= wkbeg and k0 + sub <= wkend):
                        out[w0:w1, k0:k1] = True
                    else:
                        kk = keys[None, k0:k1]
                        out[w0:w1, k0:k1] = (kk < pend[w0:w1, None]) | ((kk >= kbeg[w0:w1, None]) & (kk < kend[w0:w1, None]))
    return out


def mask_by_key_tiles(L, lead, period, c, tile, qtile=64, wave_keys=32, sub=32):
    """dK/dV kernel: a workgroup of `tile` keys sweeps the query tiles of key_sweep; a wave of wave_keys keys takes a sub-block
    of `sub` queries without a compare when it lies between qstart of the wave's last key and qend of its first token key, or
    at or past q2 of its last key (L with a lead key in the wave); every other element is kept iff qstart <= query < qend or
    query >= q2 of its own key"""
    kb = [key_bounds(j, L, lead, period, c) for j in range(L)]
    qstart, qend, q2 = (torch.tensor([b[i] for b in kb]) for i in range(3))
    rows = torch.arange(L)
    out = torch.zeros(L, L, dtype=torch.bool)
    for k0 in range(0, L, tile):
        k1 = min(k0 + tile, L)
        a0, a1, b0, nqt = key_sweep(k0, k1, L, lead, period, c, qtile)
        visited = list(range(a0, a1)) + list(range(b0, nqt))
        assert len(set(visited)) == len(visited)
        for w0 in range(k0, k1, wave_keys):
            w1 = min(w0 + wave_keys, k1)
            wl = min(w0 + wave_keys - 1, L - 1)
            wqlim = kb[wl][0]
            wqhi = kb[min(max(w0, lead), wl)][1]
            wq2 = kb[wl][2] if w0 >= lead else L
            for j in visited:
                for q0 in range(j * qtile, min((j + 1) * qtile, L), sub):
                    q1 = min(q0 + sub, L)
                    if (q0 >= wqlim and q0 + sub <= wqhi) or q0 >= wq2:
                        out[q0:q1, w0:w1] = True
                    else:
                        rr = rows[q0:q1, None]
                        out[q0:q1, w0:w1] = ((rr >= qstart[None, w0:w1]) & (rr < qend[None, w0:w1])) | (rr >= q2[None, w0:w1])
    return out


def tiles_visited(L, lead, period, c, tile=64, qtile=128):
    """(visited, all) key tiles of `tile` rows summed over the query tiles of `qtile` rows (forward / dQ kernels)"""
    vis = tot = 0
    for q0 in range(0, L, qtile):
        nl, jb, nkt = fwd_tiles(q0, min(q0 + qtile, L), L, lead, period, c, tile)
        vis += nl + nkt - jb
        tot += -(-L // tile)
    return vis, tot


def query_tiles_visited(L, lead, period, c, tile=128, qtile=64):
    """(visited, all) query tiles of `qtile` rows summed over the key tiles of `tile` rows (dK/dV kernel)"""
    vis = tot = 0
    for k0 in range(0, L, tile):
        a0, a1, b0, nqt = key_sweep(k0, min(k0 + tile, L), L, lead, period, c, qtile)
        vis += a1 - a0 + nqt - b0
        tot += nqt
    return vis, tot


def pairs_q(L, lead, period, c, tile=64, qtile=128):
    """(query, key) pairs of the visited key tiles, the last tile of a workgroup counted up to its key bound: the profiler's
    credit of the forward / dQ kernels"""
    n = 0
    for q0 in range(0, L, qtile):
        q1 = min(q0 + qtile, L)
        nl, jb, nkt = fwd_tiles(q0, q1, L, lead, period, c, tile)
        keys = query_bounds(q1 - 1, L, lead, period, c)[2]
        n += (q1 - q0) * (keys - (jb - nl) * tile)
    return n


def pairs_k(L, lead, period, c, tile=128, qtile=64):
    """... and of the visited query tiles (rows up to L) of the dK/dV kernel"""
    n = 0
    for k0 in range(0, L, tile):
        k1 = min(k0 + tile, L)
        a0, a1, b0, nqt = key_sweep(k0, k1, L, lead, period, c, qtile)
        rows = lambda j0, j1: min(j1 * qtile, L) - min(j0 * qtile, L)
        n += (k1 - k0) * (rows(a0, a1) + rows(b0, nqt))
    return n


# ---------------------------------------------------------------------------- census, frame-major ----
def census_mask(B, L, lead, period, c):
    return allowed(L, lead, period, c)[None].expand(B, L, L)


def census_probes(B, H, hd, L, lead, period, c):
    """attn_census probe rows in frame-major rows: the chunk edges of both halves, base and the frame edges come first"""
    n, S, G, base = geometry(L, lead, period, c)
    edges = []
    for start in (lead, base):
        for i in range(-(-n * S // G) + 1):
            e = min(start + i * G, start + n * S)
            edges += [e - 1, e]
    for f in range(period + 1):
        edges += [lead + f * S - 1, lead + f * S]
    seen, out = set(), []
    for r in edges + AC.probe_order(L):
        if 0 <= r < L and r not in seen:
            seen.add(r)
            out.append(r)
    idx = (torch.arange(B * H * hd) % L).view(B, H, hd)
    return torch.tensor(out)[idx]


def census(tag, hd, B, H, shape, run=AC.emulate, bwd=True):
    """frame_chunk_ref.census on the teacher mask: the expectations come from the dense mask, `run(q, k, v, do, mask)`
    computes under whatever mask it implements (the library ignores the argument)"""
    L, lead, period, c = shape
    truth = mask = census_mask(B, L, lead, period, c)
    q, k, v = AC.forward_inputs(hd, B, H, L, L)
    o, lse = run(q, k, v, None, truth)[:2]
    AC.check_count(tag, lse, mask)
    AC.check_labels(tag, o, mask)
    if not bwd:
        return
    sg = AC.signs(B, H, L)
    p = census_probes(B, H, hd, L, lead, period, c)
    q, k, v, do = AC.dkv_probe_inputs(hd, B, H, L, L, p, sg)
    o, lse, dq, dk, dv = run(q, k, v, do, truth)
    edv, edk, gap = AC.expect_dkv(mask, p, sg, hd)
    assert gap >= AC.MIN_GAP
    AC.check_count(tag + ".dkv", lse, mask)
    AC.check_support_and_values(tag + ".dv", dv, edv, AC.REL_DV)
    AC.check_support_and_values(tag + ".dk", dk, edk, AC.REL_DK)
    AC.check_zero(tag + ".dkv.dq", dq)
    q, k, v, do = AC.dq_probe_inputs(hd, B, H, L, L, p, sg)
    o, lse, dq, dk, dv = run(q, k, v, do, truth)
    edq, gap = AC.expect_dq(mask, p, sg, hd)
    assert gap >= AC.MIN_GAP
    AC.check_support_and_values(tag + ".dq", dq, edq, AC.REL_DK)
    AC.check_zero(tag + ".dq.dk", dk)


# --------------------------------------------------------------------------------------- models ----
def teacher_rope(head_dim, n, h, w, rope_start):
    """cos / sin rows of [registers | (h w t) tokens of 2n token-frames]: token-frame n + f on the rows of token-frame f"""
    cos, sin = O.rope_cos_sin(head_dim, (n, h, w), rope_start)
    rows = N_REG + torch.arange(h * w)[:, None] * n + (torch.arange(2 * n) % n)[None, :]
    idx = torch.cat([torch.arange(N_REG), rows.reshape(-1)])
    return cos[idx], sin[idx]


def dit_forward(P, cfg, clean, noisy, context, timesteps, rope_start, chunk, context_lens=None, reg=None, keep_clean=True,
                whole=False):
    """the fp32 helper model on cat([clean, noisy], dim=2): 2n token-frames at the levels [0 ... 0 | timesteps], the registers
    at reg [B] (default 1.0), every self-attention under allowed_tok(L, N_REG, 2n, chunk).  Returns the noisy half
    [B, C, T, H, W] (whole=True: both halves).  keep_clean=False drops the clean token keys from every noisy query (the
    discrimination check: what a model without its clean context computes)."""
    x = torch.cat([clean, noisy], dim=2)
    B, C, T2, Hh, Ww = x.shape
    pt, p = cfg.time_patch_size, cfg.patch_size
    t2, h, w = T2 // pt, Hh // p, Ww // p
    n = t2 // 2
    assert tuple(timesteps.shape) == (B, n)
    ts = torch.cat([torch.zeros_like(timesteps), timesteps], dim=1)
    tok = O.patch_embed(x, P["patch_embed.patch_proj.weight"], P["patch_embed.patch_proj.bias"], pt, p)
    tok = torch.cat([P["register_tokens"].expand(B, -1, -1).to(tok.dtype), tok], dim=1)
    L = tok.shape[1]
    gidx = R.group_index(L, N_REG, t2)
    mask = allowed_tok(L, N_REG, t2, chunk)
    if not keep_clean:
        f = (torch.arange(L) - N_REG).clamp(min=0) % t2
        tokrow = torch.arange(L) >= N_REG
        noisy_row, clean_row = tokrow & (f >= n), tokrow & (f < n)
        mask = mask & ~(noisy_row[:, None] & clean_row[None, :])
    cos, sin = teacher_rope(cfg.head_dim, n, h, w, rope_start)
    lead_t = torch.ones(B, dtype=ts.dtype) if reg is None else torch.as_tensor(reg, dtype=ts.dtype)
    cv = KC._conditioning(P, cfg, ts, lead_t, tok.dtype)
    v_0 = None
    for i in range(cfg.depth):
        tok, v = FC.block_forward(P, f"blocks.{i}.", cfg, tok, context, cv, gidx, v_0, cos, sin, mask, context_lens)
        if v_0 is None:
            v_0 = v
    fshift, fscale = R._mods(cv, P["final_modulation.1.weight"], P["final_modulation.1.bias"], gidx, 2)
    tok = (O.rms_norm(tok, P.get("final_norm.weight")) * (1 + fscale) + fshift)[:, N_REG:, :]
    y = O.linear(tok, P["final_proj.weight"], P["final_proj.bias"])
    out = O.unpatchify(y, C, t2, h, w, pt, p)
    return out if whole else out[:, :, T2 // 2:]
