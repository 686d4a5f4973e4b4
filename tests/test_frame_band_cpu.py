"""Frame-band self-attention of the bidirectional model (enable_frame_band) without a GPU: the dense band mask against a
double loop over its definition in token rows and in frame-major rows, symmetric, with every row attending itself and the
lead rows; the mask as the BAND kernels apply it -- the tile ranges of the forward / dQ workgroups and of the dK/dV
workgroups, the full sweep of the workgroup that holds a lead row, the open tests, the per-lane compares -- against the
dense mask for every GPU shape and every tile size, with tight bounds; the tiles skipped; one flipped pair at each bound
against the mask census; every refusal raised before the device is touched, in ops, in the model and -- in a child process
that sees no GPU -- in the C entry points; what enable_frame_band sets and unsets; the unchanged constructors; the C
symbols."""
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

from video_diffusion_speedrun_amd import _lib, model as M, ops, sampling

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_census as AC  # noqa: E402
import frame_band_ref as FB  # noqa: E402
import frame_major_ref as FM  # noqa: E402
from test_attn_census_cpu import norm_checks_accept  # noqa: E402

bf16 = torch.bfloat16
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = FB.ids
N_REG = FB.N_REG


# ------------------------------------------------------------------------------------------ mask ----
@pytest.mark.parametrize("shape", [s for s in FB.SHAPES if s[0] <= 300], ids=ids)
def test_dense_mask_against_a_double_loop(shape):
    L, lead, period, c, band = shape
    S = (L - lead) // period
    b = band // c
    assert (L - lead) % period == 0 and band % c == 0
    mt, mf = FB.allowed_tok(L, lead, period, c, band), FB.allowed(L, lead, period, c, band)
    ct = [None if l < lead else ((l - lead) % period) // c for l in range(L)]  # chunk of a token row, None: a lead row
    cf = [None if r < lead else (r - lead) // (c * S) for r in range(L)]        # ... of a frame-major row

    def attends(cq, ck):  # the definition
        return cq is None or ck is None or abs(cq - ck) <= b
    for q in range(L):
        for k in range(L):
            assert bool(mt[q, k]) == attends(ct[q], ct[k]), (q, k)
            assert bool(mf[q, k]) == attends(cf[q], cf[k]), (q, k)
    tok = FM.tok_index(L, lead, period)
    assert torch.equal(mf, mt[tok][:, tok])  # the same mask, rows permuted
    # the bounds state the mask, for a query and -- the same pair -- for a key
    for r in range(L):
        want = torch.ones(L, dtype=torch.bool)
        if r >= lead:
            lo, hi = FB.lo(r, lead, S, c, b), FB.hi(r, lead, S, c, b, L)
            want[lead:] = False
            want[lo:hi] = True
            assert lo <= r < hi
            assert ops.fm_band_lo(r, lead, S, c, b) == lo and ops.fm_band_hi(r, lead, S, c, b, L) == hi
        else:
            assert ops.fm_band_lo(r, lead, S, c, b) == 0 and ops.fm_band_hi(r, lead, S, c, b, L) == L
        assert torch.equal(mf[r], want), r
        assert torch.equal(mf[:, r], want), r


@pytest.mark.parametrize("shape", FB.SHAPES, ids=ids)
def test_the_mask_is_symmetric_and_no_row_is_empty(shape):
    L, lead, period, c, band = shape
    for m in (FB.allowed(L, lead, period, c, band), FB.allowed_tok(L, lead, period, c, band)):
        assert torch.equal(m, m.T)
        assert m.diagonal().all(), "every row attends itself"
        assert m[:, :lead].all() and m[:lead].all(), "every row attends the lead rows, a lead row everything"
    tok = FM.tok_index(L, lead, period)
    assert torch.equal(FB.allowed(L, lead, period, c, band), FB.allowed_tok(L, lead, period, c, band)[tok][:, tok])
    assert FB.allowed(L, lead, period, c, band).all() == FB.covers(period, c, band)


def test_a_band_of_every_chunk_attends_every_pair():
    for L, lead, period, c, _ in FB.SHAPES:
        n = -(-period // c)
        for b in (n - 1, n, 4 * n):
            assert FB.allowed(L, lead, period, c, b * c).all() and FB.allowed_tok(L, lead, period, c, b * c).all()
        if n > 1:
            assert not FB.allowed(L, lead, period, c, (n - 2) * c).all()
    assert FB.allowed(280, 16, 8, 11, 0).all()  # chunk >= period: one chunk


# ----------------------------------------------------------------------------------- tile bounds ----
@pytest.mark.parametrize("shape", FB.SHAPES, ids=ids)
def test_the_mask_as_the_kernels_apply_it_is_the_dense_mask(shape):
    L, lead, period, c, band = shape
    m = FB.allowed(L, lead, period, c, band)
    for tile in FB.TILES:
        for wave_rows, sub in ((32, 32), (64, 32), (16, 16), (32, 16), (64, 16)):
            if wave_rows <= tile:
                got, tight = FB.mask_by_tiles(L, lead, period, c, band, tile, wave_rows, sub)
                assert torch.equal(got, m), (tile, wave_rows, sub)
                assert tight, (tile, "a second range starts before the tile that holds lo of the first query")
        for qtile in (32, 64, 128):
            for wave_keys in (32, 16):
                if wave_keys <= tile:
                    assert torch.equal(FB.mask_by_key_tiles(L, lead, period, c, band, tile, qtile, wave_keys), m), (tile, qtile)


def test_tight_sweeps():
    """a workgroup without a lead row ends at the tile that holds the last row it attends"""
    for L, lead, period, c, band in FB.SHAPES:
        S, b = (L - lead) // period, band // c
        m = FB.allowed(L, lead, period, c, band)
        last = torch.where(m, torch.arange(L)[None, :], torch.full((1, 1), -1)).amax(1)  # per query: its last key
        for q0 in range(0, L, 128):
            q1 = min(q0 + 128, L)
            nl, jb, nkt = FB.fwd_tiles(q0, q1, lead, S, min(c, period), b, L)
            assert int(last[q0:q1].max()) // 64 == nkt - 1, (L, q0)


@pytest.mark.parametrize("shape", FB.SHAPES, ids=ids)
def test_tiles_are_skipped_unless_the_band_covers_every_pair(shape):
    """the walk visits exactly the tiles that hold an attended pair -- no walk of whole tiles can visit fewer -- at the
    kernels' geometry (64-key tiles, 128 queries) and at every finer one.  With 16-row tiles that is strictly fewer than all
    tiles whenever the band does not cover every pair.  In the kernels' geometry four of the small shapes have no tile to
    skip (NO_SKIP: frames of 29 .. 50 rows, or chunks of 99, leave no 64-key tile without an attended key for any 128-query
    workgroup); every other shape that does not cover every pair skips there too."""
    L, lead, period, c, band = shape
    m = FB.allowed(L, lead, period, c, band)
    for tile, qtile in ((64, 128), (64, 64), (32, 32), (16, 16)):
        vis, tot = FB.tiles_visited(L, lead, period, c, band, tile, qtile)
        need = sum(int(m[q0:q0 + qtile, k0:k0 + tile].any()) for q0 in range(0, L, qtile) for k0 in range(0, L, tile))
        assert vis == need <= tot, (shape, tile, qtile)
        if FB.covers(period, c, band):
            assert vis == tot
        elif (tile, qtile) == (16, 16) or ((tile, qtile) == (64, 128) and shape not in NO_SKIP):
            assert vis < tot, (shape, tile, qtile)
        elif (tile, qtile) == (64, 128):
            assert vis == tot, (shape, tile, qtile)


NO_SKIP = [(166, 16, 3, 1, 1), (280, 16, 8, 3, 3), (203, 0, 7, 1, 2), (140, 5, 3, 1, 1)]


def test_the_skips_and_the_open_sub_blocks_do_occur():
    """(1040, 16, 8, 1, 1): S = 128, frame f at rows 16 + 128 f.  The workgroup of rows 512 .. 639 lies in frames 3 and 4:
    lo(512) = 16 + 2 * 128 = 272 (tile 4), hi(639) = 16 + 6 * 128 = 784 (tile 12 holds its last key): after tile 0 it skips
    the tiles 1 .. 3 and visits 4 .. 12.  The first workgroup holds the lead rows and visits all 17 tiles; the 16-row last
    one (frame 7) visits tile 0 and 12 .. 16."""
    L, lead, S = 1040, 16, 128
    assert FB.fwd_tiles(512, 640, lead, S, 1, 1, L) == (1, 4, 13)
    assert FB.fwd_tiles(0, 128, lead, S, 1, 1, L) == (17, 17, 17)
    assert FB.fwd_tiles(1024, 1040, lead, S, 1, 1, L) == (1, 12, 17)
    assert FB.fwd_tiles(128, 256, lead, S, 1, 1, L) == (1, 1, 7)  # lead tile and run touch: nothing skipped
    assert FB.fwd_tiles(512, 640, lead, S, 1, 0, L) == (1, 6, 11)  # band 0: own chunks only
    # (656, 80, 9, 1, 2): the lead rows span two key tiles
    assert FB.fwd_tiles(512, 640, 80, 64, 1, 2, 656)[0] == 2
    # lead = 0: no lead tile, the first workgroup is a token workgroup and the loop starts at the run
    assert FB.fwd_tiles(0, 128, 0, 29, 1, 2, 203) == (0, 0, 4)
    assert FB.fwd_tiles(128, 203, 0, 29, 1, 2, 203) == (0, 0, 4)


def test_tile_fraction_at_the_training_shape():
    """C3b: L = 8208 = 16 + 8 * 1024, c = 1, t = 8: a token query of band 1 attends 22 of the 64 frame pairs"""
    prev = 0.0
    for band in (0, 1, 2, 7):
        vis, tot = FB.tiles_visited(8208, 16, 8, 1, band)
        assert tot == 65 * 129 and prev < vis / tot
        prev = vis / tot
    assert prev == 1.0
    pairs = sum(1 for a in range(8) for b in range(8) if abs(a - b) <= 1)
    assert pairs == 22
    f1 = FB.tiles_visited(8208, 16, 8, 1, 1)[0] / tot
    assert 22 / 64 < f1 < 0.42, f1  # the frame pairs, the lead tile, the first workgroup's full sweep, tile edges
    assert FB.tiles_visited(8208, 16, 8, 1, 0)[0] / tot < 0.19


# ---------------------------------------------------------------------------------------- census ----
@pytest.mark.parametrize("hd", FM.HEAD_DIMS)
def test_census_conditions_hold_under_the_band_mask(hd):
    for shape in FB.SHAPES:
        L, lead, period, c, band = shape
        if hd > L:
            continue
        BH = -(-L // hd)
        B, H = (BH + 1) // 2, 2
        mask = FB.census_mask(B, L, lead, period, c, band)
        assert AC.label_counts(mask[:1], hd).max().item() <= AC.MAX_LABEL, shape
        sg = FB.census_signs(B, H, L)
        p = FB.census_probes(B, H, hd, L, lead, period, c)
        assert len(set(p.flatten().tolist())) == L
        if L <= 300:
            assert AC.expect_dkv(mask, p, sg, hd)[2] >= AC.MIN_GAP and AC.expect_dq(mask, p, sg, hd)[1] >= AC.MIN_GAP


def test_the_emulation_passes_the_band_census():
    for shape in [s for s in FB.SHAPES if s[0] <= 300]:
        FB.census(ids(shape), 64, 3, 2, shape)


# (280, 16, 8, c = 1, band = 1): S = G = 33; frame f at rows 16 + 33 f.  Row 148 = 16 + 4 * 33 is the first row of frame 4: it
# attends [0, 16) and [115, 214) = frames 3 .. 5.
BITE = {
    "lo": (148, 115),             # the first row of frame 4 loses the first key of its run
    "lo_minus_1": (148, 114),     # ... and gains the last key before it
    "hi_minus_1": (148, 213),     # ... loses the last key of its run
    "lead_minus_1": (279, 15),    # the last row loses the last register key, far from its run
    "a_lead_querys_last_key": (15, 279),  # the last register row loses the sequence's last key
}


@pytest.mark.parametrize("name", list(BITE))
def test_one_flipped_pair_fails_the_census_and_passes_the_norm_checks(name):
    shape = (280, 16, 8, 1, 1)
    L, lead, period, c, band = shape
    qr, kr = BITE[name]
    assert FB.lo(148, lead, 33, 1, 1) == 115 and FB.hi(148, lead, 33, 1, 1, L) == 214
    hd, H, B = 64, 2, 3
    right = FB.census_mask(B, L, lead, period, c, band).clone()
    assert bool(right[0, qr, kr]) == (name != "lo_minus_1")
    wrong = right.clone()
    wrong[:, qr, kr] = ~wrong[:, qr, kr]  # the one pair, in every sample: whichever holds the probe sees it
    assert (wrong != right).sum().item() == B
    p = FB.census_probes(B, H, hd, L, lead, period, c)
    assert (p == qr).any() and (p == kr).any()
    FB.census(name, hd, B, H, shape)
    bad_run = lambda q, k, v, do, m: AC.emulate(q, k, v, do, wrong)
    with pytest.raises(AssertionError, match=rf"\[b=0, h=0, q={qr}\]"):
        FB.census(name, hd, B, H, shape, run=bad_run, bwd=False)
    q, k, v = AC.forward_inputs(hd, B, H, L, L)
    with pytest.raises(AssertionError, match=rf"o\[b=0, h=0, q={qr}, c={kr % hd}\]"):
        AC.check_labels(name, AC.emulate(q, k, v, None, wrong)[0], right)
    sg = FB.census_signs(B, H, L)
    q, k, v, do = AC.dkv_probe_inputs(hd, B, H, L, L, p, sg)
    edv, edk, _ = AC.expect_dkv(right, p, sg, hd)
    _, _, _, dk, dv = AC.emulate(q, k, v, do, wrong)
    with pytest.raises(AssertionError, match=rf"\[b=\d, h=\d, row={kr}, c="):
        AC.check_support_and_values(name + ".dv", dv, edv, AC.REL_DV)
    with pytest.raises(AssertionError, match=rf"\[b=\d, h=\d, row={kr}, c="):
        AC.check_support_and_values(name + ".dk", dk, edk, AC.REL_DK)
    q, k, v, do = AC.dq_probe_inputs(hd, B, H, L, L, p, sg)
    edq, _ = AC.expect_dq(right, p, sg, hd)
    with pytest.raises(AssertionError, match=rf"\[b=\d, h=\d, row={qr}, c="):
        AC.check_support_and_values(name + ".dq", AC.emulate(q, k, v, do, wrong)[2], edq, AC.REL_DK)
    g = torch.Generator().manual_seed(401)
    rand = [torch.randn(B, H, L, hd, generator=g).to(bf16) for _ in range(4)]
    assert norm_checks_accept(*rand, wrong, right), "the norm checks see this flip"


# ------------------------------------------------------------------------------------- refusals ----
def tiny(**kw):
    return M.DiT(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=144, depth=2, num_heads=2,
                 cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False, **kw)


def test_ops_refuse_band_misuse_before_the_device():
    x = torch.zeros(1, 2, 48, 64, dtype=bf16)  # CPU tensors: a launch would fail loudly
    lse = torch.zeros(1, 2, 48)
    fwd = lambda **kw: ops.band_attn_fwd(x, x, x, x, lse, **kw)
    bwd = lambda **kw: ops.band_attn_bwd(x, x, x, x, lse, x, x, x, x, **kw)
    for call in (fwd, bwd):
        with pytest.raises(ValueError, match="needs frame_major=True and frames=.*pass frame_major=True"):
            call(frames=(16, 8), band=1)
        with pytest.raises(ValueError, match="needs frame_major=True and frames=.*pass frame_major=True"):
            call(frame_major=True, band=1)
        with pytest.raises(ValueError, match="excludes window = 2 .*pass window=None"):
            call(frames=(16, 8), frame_major=True, window=2, band=1)
        with pytest.raises(ValueError, match="excludes teacher=True .*pass teacher=False"):
            call(frames=(16, 8), frame_major=True, teacher=True, band=1)
        with pytest.raises(ValueError, match="pass kv_lens=None"):
            call(frames=(16, 8), frame_major=True, kv_lens=torch.zeros(1, dtype=torch.int32), band=1)
        for bad in (1.0, True, "1", (1,)):
            with pytest.raises(ValueError, match="band = .* must be an int >= 0 .*pass band=None"):
                call(frames=(16, 8), frame_major=True, band=bad)
        with pytest.raises(ValueError, match="band = -1 must be >= 0 .*pass band=None"):
            call(frames=(16, 8), frame_major=True, band=-1)
        for bad in (0, -1, 2.0, True):
            with pytest.raises(ValueError, match="chunk = .* must be an int >= 1"):
                call(frames=(16, 8), frame_major=True, chunk=bad, band=1)
        with pytest.raises(ValueError, match="do not fit"):  # the _fm refusals stay
            call(frames=(16, 5), frame_major=True, band=1)
    with pytest.raises(ValueError, match="excludes past = 8 .*pass past=0"):
        fwd(frames=(16, 8), frame_major=True, past=8, band=1)
    # band=None is attn_fwd / attn_bwd, with their own refusals
    with pytest.raises(ValueError, match="window = 2 needs frame_major=True"):
        fwd(frames=(16, 8), window=2)
    with pytest.raises(ValueError, match="window = 2 needs frame_major=True"):
        bwd(frames=(16, 8), window=2)


def test_the_ops_signatures():
    for fn, base in ((ops.band_attn_fwd, ops.attn_fwd), (ops.band_attn_bwd, ops.attn_bwd)):
        names = list(inspect.signature(fn).parameters)
        assert names[:-1] == list(inspect.signature(base).parameters) and names[-1] == "band"
        assert inspect.signature(fn).parameters["band"].default is None
        for n, prm in inspect.signature(base).parameters.items():
            assert inspect.signature(fn).parameters[n].default == prm.default, n


def test_enable_frame_band_sets_and_unsets():
    m = tiny()
    assert m.frame_band is None and all(b.frame_band is None for b in m.blocks)
    assert m.enable_frame_band(1) is m
    assert m.frame_band == (1, 1) and all(b.frame_band == (1, 1) for b in m.blocks)
    assert all(b._fm_rows and not b.frame_major and not b.frame_causal for b in m.blocks)
    m.enable_frame_band(4, chunk=2)
    assert m.frame_band == (2, 2) and all(b.frame_band == (2, 2) for b in m.blocks)
    m.enable_frame_band(0, chunk=3)
    assert m.frame_band == (3, 0)
    assert m.enable_frame_band(None) is m
    assert m.frame_band is None and all(b.frame_band is None and not b._fm_rows for b in m.blocks)
    assert M.DiTBlock.frame_band is None
    # no parameter, no checkpoint key, the same activation_bytes
    plain = tiny()
    band = tiny().enable_frame_band(1)
    assert [n for n, _ in plain.named_parameters()] == [n for n, _ in band.named_parameters()]
    assert list(plain.state_dict()) == list(band.state_dict())
    band.load_state_dict(plain.state_dict(), strict=True)
    for mode in M.RECOMPUTE_MODES:
        assert M.activation_bytes(plain, 2, (8, 8, 8), 24, mode) == M.activation_bytes(band, 2, (8, 8, 8), 24, mode)


def test_enable_frame_band_refusals():
    m = tiny()
    for bad in (-1, 1.0, True, "2"):
        with pytest.raises(ValueError, match="band = .* must be an int >= 0 .* or None"):
            m.enable_frame_band(bad)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="chunk = .* must be an int >= 1"):
            m.enable_frame_band(2, chunk=bad)
    with pytest.raises(ValueError, match="band=3 must be a multiple of chunk=2 .* pass band=4"):
        m.enable_frame_band(3, chunk=2)
    assert m.frame_band is None  # a refused call changes nothing
    for kw in (dict(frame_causal=True), dict(frame_causal=True, frame_major=True),
               dict(frame_causal=True, frame_major=True, frame_chunk=2, frame_window=2)):
        with pytest.raises(ValueError, match="built with frame_causal=True .*frame_window="):
            tiny(**kw).enable_frame_band(1)
    # fp8 attention, in either order
    with pytest.raises(NotImplementedError, match=r"enable_fp8\(attention=False\)"):
        tiny().enable_fp8().enable_frame_band(1)
    with pytest.raises(NotImplementedError, match=r"enable_fp8\(attention=False\)"):
        tiny().enable_frame_band(1).enable_fp8()
    ok = tiny().enable_fp8(attention=False).enable_frame_band(1)  # the linears in fp8, the band attention in bf16
    assert ok.frame_band == (1, 1) and ok.fp8 and not ok.fp8_attn
    assert tiny().enable_frame_band(1).enable_fp8(attention=False).frame_band == (1, 1)
    assert tiny().enable_fp8().enable_frame_band(None).frame_band is None  # switching off is always allowed


def test_a_band_model_refuses_caches_and_teacher_forcing_before_the_device():
    m = tiny().enable_frame_band(1)
    x = torch.zeros(2, 16, 8, 8, 8, dtype=bf16)
    ctx = torch.zeros(2, 24, 64, dtype=bf16)
    ts = torch.full((2, 4), 0.5)
    with pytest.raises(ValueError, match=r"has no K / V cache .*generate_latents\(kv_cache=False\)"):
        m.new_frame_cache(2, 4, 4, 4, device="cpu")
    with pytest.raises(ValueError, match=r"has no K / V cache .*pass frame_cache=None"):
        m(x, ctx, ts, frame_cache=object())
    with pytest.raises(ValueError, match=r"drop teacher_latents .*enable_frame_band\(None\)"):
        m(x, ctx, ts, teacher_latents=x)
    with pytest.raises(ValueError, match="use kv_cache=False on this model"):
        sampling.generate_latents(m, ctx[:1], inference_steps=1, latents=x[:1], device="cpu", rollout_frames=1, kv_cache=True)
    # a block: frames are required with the band, and stay refused without it
    blk = m.blocks[0]
    with pytest.raises(ValueError, match=r"frame-band block needs frames=\(lead, period\)"):
        blk._check_frames(None, 80)
    assert blk._check_frames((16, 4), 80) == (16, 4)
    with pytest.raises(ValueError, match="do not fit|must"):
        blk._check_frames((16, 5), 80)
    m.enable_frame_band(None)
    with pytest.raises(ValueError, match="frames given to a block built without frame_causal=True"):
        blk._check_frames((16, 4), 80)
    assert blk._check_frames(None, 80) is None


def test_the_constructors_are_unchanged():
    for cls in (M.DiT, M.DiTBlock):
        names = list(inspect.signature(cls.__init__).parameters)
        assert names[-5:] == ["frame_causal", "frame_major", "frame_chunk", "frame_window", "qk_norm"]
        assert "frame_band" not in names and "band" not in names
    assert list(inspect.signature(M.DiT.forward).parameters)[-1] == "teacher_latents"
    assert list(inspect.signature(M.DiT.enable_frame_band).parameters) == ["self", "band", "chunk"]
    assert inspect.signature(M.DiT.enable_frame_band).parameters["chunk"].default == 1
    kw = dict(in_channels=16, hidden_size=128, depth=1, num_heads=2, cross_attn_input_size=64)
    with pytest.raises(ValueError, match="frame_major=True lays out the frame-causal self-attention"):
        M.DiT(frame_major=True, **kw)  # stays refused: the band is a method, not a layout flag
    with pytest.raises(ValueError, match="frame_major=True lays out the frame-causal self-attention"):
        M.DiTBlock(128, 64, 2, frame_major=True)


# ------------------------------------------------------------------------------------------ C ABI ----
def test_abi_declares_the_band_symbols():
    hdr = open(os.path.join(REPO, "include", "vds.h")).read()
    for name in ("vds_band_attn_fwd", "vds_band_attn_bwd"):
        assert re.search(rf"\bint\s+{name}\s*\(\s*const\s+vds_attn_args\s*\*[^,]*,\s*const\s+vds_mod_groups\s*\*\s*frames\s*,"
                         rf"\s*int32_t\s+chunk\s*,\s*int32_t\s+band_chunks\s*,\s*vds_stream_t\s+\w+\s*\)\s*;", hdr), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == 5
        assert not name.startswith("vds_attn_")  # the set of vds_attn_* entry points stays what test_attn_dispatch_cpu pins
        assert hasattr(_lib.load(), name)


def test_the_c_entries_refuse_bad_arguments_in_a_process_without_a_gpu():
    """ARG before UNSUPPORTED, nothing launched (tests/helpers/frame_band_refusals.py)"""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "frame_band_refusals.py")
    import frame_band_refusals
    env = dict(os.environ, **frame_band_refusals.HIDE)
    r = subprocess.run([sys.executable, script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout
    assert "42 calls checked, 0 wrong" in r.stdout, r.stdout
