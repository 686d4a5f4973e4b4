"""Frame-major self-attention, the reference side (tests/test_frame_major_cpu.py and the GPU modules): the row maps as
index tensors, the frame-major mask, the tile bounds as the kernels state them and the census inputs in frame-major order.
CPU only, no import of the library: everything here is written from the definitions in include/vds.h.

Token row l of a sample lives at frame-major row fm(l) = l for l < lead, lead + ((l - lead) % period) * S + (l - lead) //
period otherwise, S = (L - lead) // period; query row r attends key row j iff group(j) <= group(r) with group(r) = 0 for
r < lead, 1 + (r - lead) // S otherwise."""
import torch

import attn_census as AC

FC = AC.FC

# (L, lead, period): S = 50; S = 33; no lead; odd everything; S = 65; one frame (nothing but the register rule); S = 1
# (lower-triangular); frames aligned with every tile size; frames offset from the tiles by 16 (5 tiles of 256 queries)
SHAPES = [(166, 16, 3), (280, 16, 8), (203, 0, 7), (140, 5, 3), (293, 33, 4), (193, 64, 1), (80, 16, 64), (1024, 0, 4),
          (1040, 16, 4)]
HEAD_DIMS = [32, 64, 72, 96, 128]
TILES = [16, 32, 64, 128, 256]


def rows_per_frame(L, lead, period):
    assert L >= lead >= 0 and period >= 1 and (L - lead) % period == 0, (L, lead, period)
    return (L - lead) // period


def fm_index(L, lead, period):
    """int64 [L]: fm(l) of every token row l"""
    S = rows_per_frame(L, lead, period)
    l = torch.arange(L)
    x = (l - lead).clamp(min=0)
    return torch.where(l < lead, l, lead + (x % period) * S + x // period)


def tok_index(L, lead, period):
    """int64 [L]: tok(r) of every frame-major row r; t[..., tok_index, :] takes a token-major tensor to frame-major rows"""
    S = max(rows_per_frame(L, lead, period), 1)
    r = torch.arange(L)
    x = (r - lead).clamp(min=0)
    return torch.where(r < lead, r, lead + (x % S) * period + x // S)


def group_of(r, lead, S):
    return 0 if r < lead else 1 + (r - lead) // S


def allowed(L, lead, period):
    """bool [L, L] in frame-major rows: [r, j] = query r attends key j"""
    S = max(rows_per_frame(L, lead, period), 1)
    r = torch.arange(L)
    g = torch.where(r < lead, torch.zeros_like(r), 1 + (r - lead).clamp(min=0) // S)
    return g[None, :] <= g[:, None]


def key_end(q0, q1, lead, S):
    """the key loop of the query rows [q0, q1) ends here (vds_attn_fwd_causal_fm, the dQ kernels)"""
    return lead if q1 <= lead else lead + ((q1 - 1 - lead) // S + 1) * S


def query_start(k0, lead, S):
    """the query loop of the key rows from k0 starts here, rounded down to the query tile by the kernel (dK/dV kernels)"""
    return 0 if k0 < lead else lead + ((k0 - lead) // S) * S


def sub_block_open(k0, k1, wq0, lead, S):
    """the wave-uniform test that branches around the element-wise mask: the wave's lowest query wq0 is a token row (no
    lead query in the wave) and the keys [k0, k1) all lie below the first frame boundary above it"""
    return wq0 >= lead and k1 <= key_end(wq0, wq0 + 1, lead, S)


def mask_by_tiles(L, lead, period, tile, wave_rows=32, sub=32):
    """the mask as the kernels apply it: nothing at or past key_end of the query tile, `open` sub-blocks attended without a
    compare, element by element otherwise"""
    S = max(rows_per_frame(L, lead, period), 1)
    dense = allowed(L, lead, period)
    out = torch.zeros_like(dense)
    for q0 in range(0, L, tile):
        q1 = min(q0 + tile, L)
        kend = min(key_end(q0, q1, lead, S), L)
        for w0 in range(q0, q1, wave_rows):
            w1 = min(w0 + wave_rows, q1)
            for k0 in range(0, kend, sub):
                k1 = min(k0 + sub, kend)
                if sub_block_open(k0, k1, w0, lead, S):
                    out[w0:w1, k0:k1] = True
                else:
                    out[w0:w1, k0:k1] = dense[w0:w1, k0:k1]
    return out


def mask_by_key_tiles(L, lead, period, tile, qtile=64):
    """the same from the dK/dV side: a key tile's query loop starts at query_start rounded down to the query tile"""
    S = max(rows_per_frame(L, lead, period), 1)
    dense = allowed(L, lead, period)
    out = torch.zeros_like(dense)
    for k0 in range(0, L, tile):
        qs = query_start(k0, lead, S) // qtile * qtile
        out[qs:, k0:k0 + tile] = dense[qs:, k0:k0 + tile]
    return out


def tiles_visited(L, lead, period, tile=64, qtile=128):
    """(visited, all) key tiles of `tile` rows summed over the query tiles of `qtile` rows"""
    S = max(rows_per_frame(L, lead, period), 1)
    vis = tot = 0
    for q0 in range(0, L, qtile):
        q1 = min(q0 + qtile, L)
        vis += -(-min(key_end(q0, q1, lead, S), L) // tile)
        tot += -(-L // tile)
    return vis, tot


# ---------------------------------------------------------------------------- census, frame-major ----
def census_mask(B, L, lead, period):
    return allowed(L, lead, period)[None].expand(B, L, L)


def census_signs(B, H, L, lead, period):
    """w [B, H, L] in {+1, -1} alternating over the frame-major rows (flipped from head to head): the keys a query attends
    are a prefix of the rows, so every attended set is balanced to within one key, at any S (S = 1 included)"""
    return AC.signs(B, H, L)


def census_probes(B, H, hd, L, lead, period):
    """attn_census.probe_rows in frame-major rows, the frame boundaries among the first probes"""
    S = max(rows_per_frame(L, lead, period), 1)
    order = AC.probe_order(L)
    edges = []
    for f in range(period + 1):
        edges += [lead + f * S - 1, lead + f * S]
    seen, out = set(), []
    for r in edges + order:
        if 0 <= r < L and r not in seen:
            seen.add(r)
            out.append(r)
    idx = (torch.arange(B * H * hd) % L).view(B, H, hd)
    return torch.tensor(out)[idx]
