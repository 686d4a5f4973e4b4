"""Frame-major self-attention without a GPU: the row maps and the frame-major mask against a double loop over the
definition, the tile bounds the kernels are to use (no attended pair outside them, `open` sub-blocks hold attended pairs
only), one flipped pair at each bound against the mask census, and every refusal that is raised before the device is
touched (the C symbols, bad frames)."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from video_diffusion_speedrun_amd import _lib, ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_census as AC  # noqa: E402
import frame_major_ref as FM  # noqa: E402
from test_attn_census_cpu import census, flipped, norm_checks_accept  # noqa: E402

FC = AC.FC
bf16 = torch.bfloat16
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = lambda s: "L{}_{}_{}".format(*s)


# ------------------------------------------------------------------------------------------ maps ----
@pytest.mark.parametrize("shape", FM.SHAPES, ids=ids)
def test_maps_against_the_definition(shape):
    L, lead, period = shape
    S = (L - lead) // period
    fm = [ops.fm_row(l, lead, period, L) for l in range(L)]
    tok = [ops.tok_row(r, lead, period, L) for r in range(L)]
    for l in range(L):
        want = l if l < lead else lead + ((l - lead) % period) * S + (l - lead) // period
        assert fm[l] == want and tok[want] == l, l
    assert sorted(fm) == list(range(L)) and sorted(tok) == list(range(L))  # permutations, inverse of each other
    assert FM.fm_index(L, lead, period).tolist() == fm and FM.tok_index(L, lead, period).tolist() == tok
    # a frame's rows are contiguous, in token order, and the frame is the token's modulation group
    for r in range(L):
        assert ops.fm_group_of(r, lead, S) == ops.mod_group_of(tok[r], lead, period) == FM.group_of(r, lead, S)
        if r > lead and ops.fm_group_of(r, lead, S) == ops.fm_group_of(r - 1, lead, S):
            assert tok[r] == tok[r - 1] + period


@pytest.mark.parametrize("shape", [s for s in FM.SHAPES if s[0] <= 300], ids=ids)
def test_mask_is_the_interleaved_mask_permuted(shape):
    L, lead, period = shape
    S = (L - lead) // period
    m = FM.allowed(L, lead, period)
    tok = FM.tok_index(L, lead, period)
    assert torch.equal(m, FC.allowed(L, lead, period)[tok][:, tok])
    for r in range(L):
        for j in range(L):
            assert bool(m[r, j]) == (FM.group_of(j, lead, S) <= FM.group_of(r, lead, S)), (r, j)
    assert m[:, 0].all(), "key 0 is attended by every query: no empty row"


def test_the_large_masks_are_the_interleaved_masks_permuted():
    for L, lead, period in [s for s in FM.SHAPES if s[0] > 300]:
        tok = FM.tok_index(L, lead, period)
        assert torch.equal(FM.allowed(L, lead, period), FC.allowed(L, lead, period)[tok][:, tok])


# ----------------------------------------------------------------------------------- tile bounds ----
@pytest.mark.parametrize("shape", FM.SHAPES, ids=ids)
def test_no_attended_pair_lies_outside_the_tile_bounds(shape):
    L, lead, period = shape
    S = (L - lead) // period
    m = FM.allowed(L, lead, period)
    last_key = torch.where(m, torch.arange(L)[None, :], torch.full((1, 1), -1)).amax(1)   # per query
    first_query = torch.where(m, torch.arange(L)[:, None], torch.full((1, 1), L)).amin(0)  # per key
    for tile in FM.TILES:
        for q0 in range(0, L, tile):
            q1 = min(q0 + tile, L)
            kend = ops.fm_key_end(q0, q1, lead, S)
            assert kend == FM.key_end(q0, q1, lead, S) and 0 < kend <= L
            assert int(last_key[q0:q1].max()) == kend - 1, (tile, q0)  # tight: the last visited key is attended
        for k0 in range(0, L, tile):
            qs = ops.fm_query_start(k0, lead, S)
            assert qs == FM.query_start(k0, lead, S)
            assert int(first_query[k0:min(k0 + tile, L)].min()) == qs, (tile, k0)  # tight as well
        # the mask as the kernels apply it -- skipped tiles, open sub-blocks, compares elsewhere -- is the dense mask
        for wave_rows, sub in ((32, 32), (64, 32), (16, 16), (32, 16)):
            if wave_rows <= tile:
                assert torch.equal(FM.mask_by_tiles(L, lead, period, tile, wave_rows, sub), m), (tile, wave_rows, sub)
        for qtile in (32, 64, 128):
            assert torch.equal(FM.mask_by_key_tiles(L, lead, period, tile, qtile), m), (tile, qtile)


@pytest.mark.parametrize("shape", FM.SHAPES, ids=ids)
def test_open_sub_blocks_hold_attended_pairs_only(shape):
    L, lead, period = shape
    S = (L - lead) // period
    m = FM.allowed(L, lead, period)
    n_open = 0
    for wave_rows in (16, 32, 64):
        for sub in (16, 32):
            for w0 in range(0, L, wave_rows):
                for k0 in range(0, L, sub):
                    k1 = min(k0 + sub, L)
                    if FM.sub_block_open(k0, k1, w0, lead, S):
                        n_open += 1
                        assert m[w0:w0 + wave_rows, k0:k1].all(), (wave_rows, sub, w0, k0)
    assert n_open > 0 or L - lead < 16
    # a lead query in the wave closes it: the wave [lead - 1, ...) must compare
    if lead:
        assert not FM.sub_block_open(lead, lead + 1, lead - 1, lead, S)


def test_tile_fraction_at_the_training_shape():
    """C3b: L = 8208 = 16 + 8 * 1024; 64-key tiles under 128-query tiles: 9/16 of the token tiles plus the lead's share"""
    vis, tot = FM.tiles_visited(8208, 16, 8)
    assert tot == 65 * 129 and 0.56 < vis / tot < 0.58


# ---------------------------------------------------------------------------------------- census ----
@pytest.mark.parametrize("hd", FM.HEAD_DIMS)
def test_census_conditions_hold_in_frame_major_rows(hd):
    """n_c <= 64 (the condition of the 0.25 bound) and |w - mean_w| >= 0.25 or exactly 0, with every row a probe"""
    for L, lead, period in FM.SHAPES:
        if hd > L:  # (80, 16, 64) at head dims 96 and 128: a head cannot hold hd distinct probe rows; census at hd <= 72
            continue
        BH = -(-L // hd)
        B, H = (BH + 1) // 2, 2
        mask = FM.census_mask(B, L, lead, period)
        assert AC.label_counts(mask[:1], hd).max().item() <= AC.MAX_LABEL, (L, lead, period)
        w = FM.census_signs(B, H, L, lead, period)
        p = FM.census_probes(B, H, hd, L, lead, period)
        assert len(set(p.flatten().tolist())) == L
        assert all(len(set(r.tolist())) == hd for r in p.reshape(-1, hd))
        if L <= 300:
            assert AC.expect_dkv(mask, p, w, hd)[2] >= AC.MIN_GAP and AC.expect_dq(mask, p, w, hd)[1] >= AC.MIN_GAP


def fm_census(tag, hd, B, H, L, lead, period, run=AC.emulate, bwd=True):
    """test_attn_census_cpu.census on the frame-major mask, signs and probes"""
    mask = FM.census_mask(B, L, lead, period)
    q, k, v = AC.forward_inputs(hd, B, H, L, L)
    o, lse = run(q, k, v, None, mask)[:2]
    AC.check_count(tag, lse, mask)
    AC.check_labels(tag, o, mask)
    if not bwd:
        return
    w = FM.census_signs(B, H, L, lead, period)
    p = FM.census_probes(B, H, hd, L, lead, period)
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


def test_the_emulation_passes_the_frame_major_census():
    for L, lead, period in [s for s in FM.SHAPES if s[0] <= 300]:
        fm_census(ids((L, lead, period)), 64, 3, 2, L, lead, period)


# (280, 16, 8): S = 33, frames at 16, 49, 82, 115, 148, ...  The 128-query tile [0, 128) ends in frame 3: kend = 148; the
# 128-key tile from 128 starts in frame 3: qstart = 115.
BITE = {
    "a_frame_boundary": (213, 214),       # the last row of frame 5 gains the first key of frame 6
    "kend_minus_1": (127, 147),           # the tile's last query loses the last key its loop visits
    "kend": (127, 148),                   # ... and gains the first one it skips
    "qstart_minus_1": (114, 128),         # the last query before the key tile's loop gains the tile's first key
}


@pytest.mark.parametrize("name", list(BITE))
def test_one_flipped_pair_fails_the_census_and_passes_the_norm_checks(name):
    L, lead, period = 280, 16, 8
    S = 33
    qr, kr = BITE[name]
    assert FM.key_end(0, 128, lead, S) == 148 and FM.query_start(128, lead, S) == 115
    hd, H, B = 64, 2, 5
    right = FM.census_mask(B, L, lead, period).clone()
    p = FM.census_probes(B, H, hd, L, lead, period)
    b = next(i for i in range(B) if (p[i] == qr).any() and (p[i] == kr).any())
    wrong = flipped(right, b, qr, kr)
    assert (wrong != right).sum().item() == 1
    fm_census(name, hd, B, H, L, lead, period)
    bad_run = lambda q, k, v, do, m: AC.emulate(q, k, v, do, wrong)
    with pytest.raises(AssertionError, match=rf"\[b={b}, h=0, q={qr}\]"):
        fm_census(name, hd, B, H, L, lead, period, run=bad_run, bwd=False)
    q, k, v = AC.forward_inputs(hd, B, H, L, L)
    with pytest.raises(AssertionError, match=rf"o\[b={b}, h=0, q={qr}, c={kr % hd}\]"):
        AC.check_labels(name, AC.emulate(q, k, v, None, wrong)[0], right)
    w = FM.census_signs(B, H, L, lead, period)
    q, k, v, do = AC.dkv_probe_inputs(hd, B, H, L, L, p, w)
    edv, edk, _ = AC.expect_dkv(right, p, w, hd)
    _, _, _, dk, dv = AC.emulate(q, k, v, do, wrong)
    with pytest.raises(AssertionError, match=rf"\[b={b}, h=\d, row={kr}, c="):
        AC.check_support_and_values(name + ".dv", dv, edv, AC.REL_DV)
    with pytest.raises(AssertionError, match=rf"\[b={b}, h=\d, row={kr}, c="):
        AC.check_support_and_values(name + ".dk", dk, edk, AC.REL_DK)
    q, k, v, do = AC.dq_probe_inputs(hd, B, H, L, L, p, w)
    edq, _ = AC.expect_dq(right, p, w, hd)
    with pytest.raises(AssertionError, match=rf"\[b={b}, h=\d, row={qr}, c="):
        AC.check_support_and_values(name + ".dq", AC.emulate(q, k, v, do, wrong)[2], edq, AC.REL_DK)
    # random inputs in frame-major rows: the Frobenius-norm checks of the attention tests accept the wrong mask
    g = torch.Generator().manual_seed(401)
    rand = [torch.randn(B, H, L, hd, generator=g).to(bf16) for _ in range(4)]
    assert norm_checks_accept(*rand, wrong, right), "the norm checks see this flip"


# ------------------------------------------------------------------------------------- refusals ----
FM_SYMBOLS = {
    "vds_qkv_rope_fwd_fm": "vds_qkv_rope_fwd", "vds_qkv_rope_norm_fwd_fm": "vds_qkv_rope_norm_fwd",
    "vds_qkv_rope_bwd_fm": "vds_qkv_rope_bwd", "vds_qkv_rope_norm_bwd_fm": "vds_qkv_rope_norm_bwd",
}


def test_abi_declares_the_frame_major_qkv_rope_symbols():
    """each takes the arguments of its plain call plus `const vds_mod_groups* frames` before the stream"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vds.h")).read(), flags=re.S)
    for name, plain in FM_SYMBOLS.items():
        assert re.search(rf"\bint\s+{name}\s*\([^;]*,\s*const\s+vds_mod_groups\s*\*\s*frames\s*,\s*vds_stream_t\s+stream\s*\)\s*;",
                         src), name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[plain][:-1] + [C.c_void_p, C.c_void_p], name
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    one = C.c_void_p(16)  # never dereferenced: every call below is refused on the host
    good, bad = C.byref(_lib.ModGroups(16, 8)), C.byref(_lib.ModGroups(16, 7))
    B, L, H, hd, hdp = 1, 48, 2, 72, 96
    for frames, want in ((None, -1), (bad, -1), (C.byref(_lib.ModGroups(-1, 8)), -1), (C.byref(_lib.ModGroups(16, 0)), -1),
                         (C.byref(_lib.ModGroups(64, 1)), -1)):
        assert lib.vds_qkv_rope_fwd_fm(one, one, one, None, None, one, one, one, B, L, H, hd, hdp, frames, None) == want
        assert lib.vds_qkv_rope_norm_fwd_fm(one, one, one, None, None, one, one, one, B, L, H, hd, hdp, 1e-6, frames,
                                            None) == want
        assert lib.vds_qkv_rope_bwd_fm(one, one, one, one, one, None, None, None, None, None, one, 0, 0, B, L, H, hd, hdp,
                                       frames, None) == want
        assert lib.vds_qkv_rope_norm_bwd_fm(one, one, one, one, one, one, None, None, None, None, one, 0, 0, B, L, H, hd,
                                            hdp, 1e-6, frames, None) == want
    # the plain calls' own refusals still come first
    assert lib.vds_qkv_rope_fwd_fm(None, one, one, None, None, one, one, one, B, L, H, hd, hdp, good, None) == -1
    assert lib.vds_qkv_rope_norm_fwd_fm(one, one, one, None, None, one, one, one, B, L, H, hd, hdp, 0.0, good, None) == -1
    assert lib.vds_qkv_rope_norm_bwd_fm(one, one, one, one, one, None, None, None, None, None, one, 0, 0, B, L, H, hd, hdp,
                                        1e-6, good, None) == -1


def test_ops_refuse_bad_frames_before_the_device():
    x = torch.zeros(1)  # a CPU tensor: a launch would fail loudly
    for fn, args in ((ops.qkv_rope_fwd, (x, x, x, None, None, 1, 48, 2, 72, 96)),
                     (ops.qkv_rope_norm_fwd, (x, x, x, None, None, 1, 48, 2, 72, 96)),
                     (ops.qkv_rope_bwd, (x, x, x, x, x, None, None, None, None, None, 0, 0, 1, 48, 2, 72, 96)),
                     (ops.qkv_rope_norm_bwd, (x, x, x, x, x, x, None, None, None, None, 0, 0, 1, 48, 2, 72, 96))):
        for bad in ((16, 7), (-1, 8), (16, 0), (64, 1)):
            with pytest.raises(ValueError, match="do not fit 48 rows"):
                fn(*args, frames=bad)


def test_abi_declares_the_frame_major_attention_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vds.h")).read(), flags=re.S)
    for name in ("vds_attn_fwd_causal_fm", "vds_attn_bwd_causal_fm"):
        assert re.search(rf"\bint\s+{name}\s*\(\s*const\s+vds_attn_args\s*\*[^,]*,\s*const\s+vds_mod_groups\s*\*[^,]*,"
                         rf"\s*vds_stream_t", src), name
        assert _lib.SIGNATURES[name] == [C.POINTER(_lib.AttnArgs), C.c_void_p, C.c_void_p]
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    fr = C.byref(_lib.ModGroups(16, 8))

    def args(L=48, Lk=None, ones=0):
        a = _lib.AttnArgs()
        a.B, a.H, a.Lq, a.Lk, a.head_dim = 1, 2, L, L if Lk is None else Lk, 64
        for f in ("q", "k", "v", "o", "lse", "d_o", "dq", "dk", "dv", "delta"):
            setattr(a, f, 16)  # never dereferenced: every call below is refused on the host
        a.kv_pad_ones = ones
        return a
    for fn in (lib.vds_attn_fwd_causal_fm, lib.vds_attn_bwd_causal_fm):
        assert fn(None, fr, None) == -1
        assert fn(C.byref(_lib.AttnArgs()), fr, None) == -1
        assert fn(C.byref(args()), None, None) == -1                                    # NULL frames
        assert fn(C.byref(args(Lk=56)), fr, None) == -1                                 # Lq != Lk
        assert fn(C.byref(args(ones=2)), fr, None) == -1                                # the cross-attention layout
        assert fn(C.byref(args()), C.byref(_lib.ModGroups(16, 5)), None) == -1          # frames that do not fit
        assert fn(C.byref(args(L=(1 << 21) + 8)), C.byref(_lib.ModGroups(0, 8)), None) == -2  # past the exact quotient


def test_ops_refuse_frame_major_misuse_before_the_device():
    x = torch.zeros(1, 2, 48, 64, dtype=bf16)  # CPU tensors: a launch would fail loudly
    lse = torch.zeros(1, 2, 48)
    with pytest.raises(ValueError, match="needs frames"):
        ops.attn_fwd(x, x, x, x, lse, frame_major=True)
    with pytest.raises(ValueError, match="not with past or kv_lens"):
        ops.attn_fwd(x, x, x, x, lse, frames=(16, 8), past=8, frame_major=True)
    with pytest.raises(ValueError, match="not with past or kv_lens"):
        ops.attn_bwd(x, x, x, x, lse, x, x, x, x, frames=(16, 8), kv_lens=torch.zeros(1, dtype=torch.int32),
                     frame_major=True)
    with pytest.raises(ValueError, match="do not fit"):
        ops.attn_fwd(x, x, x, x, lse, frames=(16, 5), frame_major=True)


def test_frame_major_needs_frame_causal():
    from video_diffusion_speedrun_amd import model as M
    kw = dict(in_channels=16, hidden_size=128, depth=1, num_heads=2, cross_attn_input_size=64)
    with pytest.raises(ValueError, match="frame_causal=True"):
        M.DiT(frame_major=True, **kw)
    with pytest.raises(ValueError, match="frame_causal=True"):
        M.DiTBlock(128, 64, 2, frame_major=True)
    plain, fm = M.DiT(frame_causal=True, **kw), M.DiT(frame_causal=True, frame_major=True, **kw)
    assert fm.frame_major and not plain.frame_major and all(b.frame_major for b in fm.blocks)
    assert [n for n, _ in plain.named_parameters()] == [n for n, _ in fm.named_parameters()]  # no parameter is added
    with pytest.raises(NotImplementedError, match=r"enable_fp8\(attention=False\)"):
        fm.enable_fp8()  # fp8 attention stays refused, as for frame_causal
