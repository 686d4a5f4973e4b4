"""Chunk-causal self-attention (frame_chunk) without a GPU: the dense chunk mask against a double loop over its definition
in token rows and in frame-major rows; the mask as the kernels apply it -- key loop to kend, first query tile from qstart,
open sub-blocks, per-lane compares, the clip at L -- against the dense mask at every tile size, with tight bounds; one
flipped pair at each chunk bound against the mask census; the helper model's cached chunk call against its full-sequence
call; the trainer's "chunk" schedule; every refusal that is raised before the device is touched; the C symbols."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from video_diffusion_speedrun_amd import _lib, model as M, ops, sampling, train

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_census as AC  # noqa: E402
import frame_chunk_ref as CH  # noqa: E402
import frame_major_ref as FM  # noqa: E402
from test_attn_census_cpu import flipped, norm_checks_accept  # noqa: E402

KC, FC = CH.KC, CH.FC
bf16, f32 = torch.bfloat16, torch.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = CH.ids


def rel(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


# ------------------------------------------------------------------------------------------ mask ----
@pytest.mark.parametrize("shape", [s for s in CH.SHAPES if s[0] <= 300], ids=ids)
def test_dense_mask_against_a_double_loop(shape):
    L, lead, period, c = shape
    S = (L - lead) // period
    assert (L - lead) % period == 0
    mt, mf = CH.allowed_tok(L, lead, period, c), CH.allowed(L, lead, period, c)
    gt = [0 if l < lead else 1 + ((l - lead) % period) // c for l in range(L)]      # the definition, token rows
    gf = [0 if r < lead else 1 + (r - lead) // (c * S) for r in range(L)]            # ... frame-major rows
    for q in range(L):
        for k in range(L):
            assert bool(mt[q, k]) == (gt[k] <= gt[q]), (q, k)
            assert bool(mf[q, k]) == (gf[k] <= gf[q]), (q, k)
    tok = FM.tok_index(L, lead, period)
    assert torch.equal(mf, mt[tok][:, tok])  # the same mask, rows permuted
    for r in range(L):
        l = int(tok[r])
        assert gf[r] == gt[l] == ops.fm_group_of(r, lead, S, c) == ops.chunk_group_of(l, lead, period, c)
        assert ops.fm_group_of(r, lead, S) == FM.group_of(r, lead, S)  # default chunk: today's result
    assert mf[:, 0].all(), "key 0 is attended by every query: no empty row"
    if c >= period:  # one token group: tokens attend everything, registers the registers
        assert mf[lead:].all() and not mf[:lead, lead:].any() and mf[:lead, :lead].all()
    assert torch.equal(CH.allowed(L, lead, period, 1), FM.allowed(L, lead, period))  # c = 1 is today's mask


def test_the_large_masks_are_the_token_masks_permuted():
    for L, lead, period, c in [s for s in CH.SHAPES if s[0] > 300]:
        tok = FM.tok_index(L, lead, period)
        assert torch.equal(CH.allowed(L, lead, period, c), CH.allowed_tok(L, lead, period, c)[tok][:, tok])


# ----------------------------------------------------------------------------------- tile bounds ----
@pytest.mark.parametrize("shape", CH.SHAPES, ids=ids)
def test_the_mask_as_the_kernels_apply_it_is_the_dense_mask(shape):
    L, lead, period, c = shape
    S = (L - lead) // period
    m = CH.allowed(L, lead, period, c)
    last_key = torch.where(m, torch.arange(L)[None, :], torch.full((1, 1), -1)).amax(1)   # per query
    first_query = torch.where(m, torch.arange(L)[:, None], torch.full((1, 1), L)).amin(0)  # per key
    for tile in CH.TILES:
        for q0 in range(0, L, tile):
            q1 = min(q0 + tile, L)
            kend = ops.fm_key_end(q0, q1, lead, S, c, L)
            assert kend == CH.key_end(q0, q1, lead, S, c, L) and 0 < kend <= L  # the clip at L
            assert int(last_key[q0:q1].max()) == kend - 1, (tile, q0)  # tight: the last visited key is attended
        for k0 in range(0, L, tile):
            qs = ops.fm_query_start(k0, lead, S, c)
            assert qs == CH.query_start(k0, lead, S, c)
            assert int(first_query[k0:min(k0 + tile, L)].min()) == qs, (tile, k0)  # tight: the first visited query attends
        for wave_rows, sub in ((32, 32), (64, 32), (16, 16), (32, 16), (64, 16)):
            if wave_rows <= tile:
                assert torch.equal(CH.mask_by_tiles(L, lead, period, c, tile, wave_rows, sub), m), (tile, wave_rows, sub)
        for qtile in (32, 64, 128):
            for wave_keys in (32, 16):
                if wave_keys <= tile:
                    assert torch.equal(CH.mask_by_key_tiles(L, lead, period, c, tile, qtile, wave_keys), m), (tile, qtile)
    # without the clip a short last chunk runs past L
    if period % c and c < period:
        G = c * S
        assert lead + ((L - 1 - lead) // G + 1) * G > L
        assert ops.fm_key_end(0, L, lead, S, c) > L and ops.fm_key_end(0, L, lead, S, c, L) == L
    # defaults keep the current results
    assert ops.fm_key_end(0, lead + 1, lead, S) == FM.key_end(0, lead + 1, lead, S)
    assert ops.fm_query_start(L - 1, lead, S) == FM.query_start(L - 1, lead, S)


def test_the_open_sub_blocks_do_occur():
    """the emulation's open branch is exercised: whole sub-blocks below a chunk's first row, on both sides"""
    L, lead, period, c = 1040, 16, 4, 2
    S = 256
    assert CH.key_end(528, 529, lead, S, c, L) == 1040 and CH.key_end(16, 17, lead, S, c, L) == 528
    assert CH.query_start(600, lead, S, c) == 528 and CH.query_start(527, lead, S, c) == 16


def test_tile_fraction_at_the_training_shape():
    """C3b: L = 8208 = 16 + 8 * 1024: n = t / c chunks visit about (n + 1) / (2 n) of the key tiles"""
    for c, n in ((1, 8), (2, 4), (4, 2), (8, 1)):
        vis, tot = CH.tiles_visited(8208, 16, 8, c)
        ideal = (n + 1) / (2 * n)
        assert tot == 65 * 129 and ideal <= vis / tot < ideal + 0.02, (c, vis / tot)
    assert CH.tiles_visited(8208, 16, 8, 1) == FM.tiles_visited(8208, 16, 8)


# ---------------------------------------------------------------------------------------- census ----
@pytest.mark.parametrize("hd", FM.HEAD_DIMS)
def test_census_conditions_hold_under_the_chunk_mask(hd):
    """n_c <= 64 (the condition of the 0.25 bound) and |w - mean_w| >= 0.25 or exactly 0, with every row a probe"""
    for L, lead, period, c in CH.SHAPES:
        if hd > L:
            continue
        BH = -(-L // hd)
        B, H = (BH + 1) // 2, 2
        mask = CH.census_mask(B, L, lead, period, c)
        assert AC.label_counts(mask[:1], hd).max().item() <= AC.MAX_LABEL, (L, lead, period, c)
        w = CH.census_signs(B, H, L)
        p = CH.census_probes(B, H, hd, L, lead, period, c)
        assert len(set(p.flatten().tolist())) == L
        assert all(len(set(r.tolist())) == hd for r in p.reshape(-1, hd))
        if L <= 300:
            assert AC.expect_dkv(mask, p, w, hd)[2] >= AC.MIN_GAP and AC.expect_dq(mask, p, w, hd)[1] >= AC.MIN_GAP


def test_the_emulation_passes_the_chunk_census():
    for L, lead, period, c in [s for s in CH.SHAPES if s[0] <= 300]:
        CH.census(ids((L, lead, period, c)), 64, 3, 2, L, lead, period, c)


# (280, 16, 8, c = 2): S = 33, G = 66, chunks at 16, 82, 148, 214; frames at 16, 49, 82, 115, 148, ...  The 128-query tile
# [0, 128) ends in chunk 1: kend = 148; the 128-key tile from 128 starts in chunk 1: qstart = 82.
BITE = {
    "kend_minus_1": (127, 147),           # the tile's last query loses the last key its loop visits
    "kend": (127, 148),                   # ... and gains the first one it skips
    "qstart_minus_1": (81, 128),          # the last query before the key tile's loop gains the tile's first key
    "two_frames_of_one_chunk": (114, 115),  # the last row of frame 2 loses the first key of frame 3, its own chunk's
}


@pytest.mark.parametrize("name", list(BITE))
def test_one_flipped_pair_fails_the_census_and_passes_the_norm_checks(name):
    L, lead, period, c = 280, 16, 8, 2
    S = 33
    qr, kr = BITE[name]
    assert CH.key_end(0, 128, lead, S, c, L) == 148 and CH.query_start(128, lead, S, c) == 82
    hd, H, B = 64, 2, 5
    right = CH.census_mask(B, L, lead, period, c).clone()
    assert bool(right[0, qr, kr]) == (name in ("kend_minus_1", "two_frames_of_one_chunk"))
    if name == "two_frames_of_one_chunk":  # attended here, excluded by the frame-causal mask
        assert not FM.allowed(L, lead, period)[qr, kr]
    p = CH.census_probes(B, H, hd, L, lead, period, c)
    b = next(i for i in range(B) if (p[i] == qr).any() and (p[i] == kr).any())
    wrong = flipped(right, b, qr, kr)
    assert (wrong != right).sum().item() == 1
    CH.census(name, hd, B, H, L, lead, period, c)
    bad_run = lambda q, k, v, do, m: AC.emulate(q, k, v, do, wrong)
    with pytest.raises(AssertionError, match=rf"\[b={b}, h=0, q={qr}\]"):
        CH.census(name, hd, B, H, L, lead, period, c, run=bad_run, bwd=False)
    q, k, v = AC.forward_inputs(hd, B, H, L, L)
    with pytest.raises(AssertionError, match=rf"o\[b={b}, h=0, q={qr}, c={kr % hd}\]"):
        AC.check_labels(name, AC.emulate(q, k, v, None, wrong)[0], right)
    w = CH.census_signs(B, H, L)
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


# ------------------------------------------------------------------------------- model and cache ----
@pytest.mark.parametrize("f0", [0, 2, 4])
def test_cached_chunk_is_the_full_sequence_chunk_model_on_the_chunks_frames(f0):
    """5 token-frames in chunks of 2: (0, 2), (2, 2) and the short last chunk (4, 1)"""
    cfg, P, latent, ctx = CH.long_case()
    c, n, pt = 2, CH.T_FRAMES, cfg.time_patch_size
    k = min(c, n - f0)
    out, cache = CH.cached_chunk(P, cfg, latent, ctx, n, c, f0, k)
    assert cache.past_frames == f0 and tuple(out.shape) == (2, 16, k * pt, 8, 8)
    ts = torch.ones(2, n)
    ts[:, :f0] = 0
    ts[:, f0:f0 + k] = torch.tensor(CH.T_LEVELS)[:, :k].to(bf16).float()
    with torch.no_grad():
        full = CH.dit_forward(P, cfg, latent.float(), ctx.float(), ts, KC.BASE, c, reg=torch.tensor(KC.REG))
        causal = CH.dit_forward(P, cfg, latent.float(), ctx.float(), ts, KC.BASE, 1, reg=torch.tensor(KC.REG))
    e = rel(out, full[:, :, f0 * pt:(f0 + k) * pt])
    print(f"frames {f0}..{f0 + k - 1}: cached vs full-sequence chunk model {e:.2e}")
    assert e <= 1e-5, e
    if k > 1:  # the frame-causal model is another model: frame f0 there does not see frame f0 + 1
        assert rel(causal[:, :, f0 * pt:(f0 + 1) * pt], full[:, :, f0 * pt:(f0 + 1) * pt]) > 1e-2


def test_the_chunk_model_is_causal_over_chunks_and_not_inside_one():
    cfg, P, latent, ctx = CH.long_case()
    pt = cfg.time_patch_size
    ts = torch.tensor([[0.5, 0.25, 0.75, 0.125, 0.9375]] * 2)
    other = latent.clone()
    other[:, :, 3 * pt:4 * pt] = (latent[:, :, 3 * pt:4 * pt].float() + 3.0).to(bf16)  # frame 3, the second of chunk 1
    with torch.no_grad():
        a = CH.dit_forward(P, cfg, latent.float(), ctx.float(), ts, KC.BASE, 2, reg=torch.ones(2))
        b = CH.dit_forward(P, cfg, other.float(), ctx.float(), ts, KC.BASE, 2, reg=torch.ones(2))
    assert torch.equal(a[:, :, :2 * pt], b[:, :, :2 * pt])                       # chunk 0: exactly unmoved
    assert rel(b[:, :, 2 * pt:3 * pt], a[:, :, 2 * pt:3 * pt]) > 1e-2            # frame 2, the same chunk: moved
    assert rel(b[:, :, 4 * pt:], a[:, :, 4 * pt:]) > 1e-2                        # the later chunk: moved


# -------------------------------------------------------------------------------------- trainer ----
def test_chunk_schedule_shapes_and_repetition():
    assert "chunk" in train.FRAME_MODES
    for n, c in ((8, 2), (8, 4), (8, 3), (3, 2), (5, 7), (4, 1)):
        g = torch.Generator().manual_seed(5)
        lv = train.draw_frame_levels("chunk", 3, n, "cpu", g, chunk=c)
        assert tuple(lv.shape) == (3, -(-n // c)) and lv.dtype == bf16
        g2 = torch.Generator().manual_seed(5)  # the draw is one randn of that shape, time-shifted
        assert torch.equal(lv, train.time_shift_from_normal(torch.randn(3, -(-n // c), dtype=bf16, generator=g2)))
        t, w = train.frame_schedule("chunk", lv, n, chunk=c)
        assert tuple(t.shape) == tuple(w.shape) == (3, n) and t.dtype == bf16 and w.dtype == f32
        assert float(w.min()) == 1.0 and float(w.max()) == 1.0
        for f in range(n):
            assert torch.equal(t[:, f], lv[:, f // c]), (n, c, f)
    with pytest.raises(ValueError, match=r"\[B, 4\] expected"):
        train.frame_schedule("chunk", torch.zeros(3, 8), 8, chunk=2)
    with pytest.raises(ValueError, match="int >= 1"):
        train.draw_frame_levels("chunk", 3, 8, "cpu", chunk=0)
    with pytest.raises(ValueError, match="frame_mode must be one of"):
        train.draw_frame_levels("chunks", 3, 8, "cpu")


def test_the_old_modes_consume_the_generator_as_before():
    for mode, shape in (("first_frame", (3,)), ("independent", (3, 8))):
        g, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
        lv = train.draw_frame_levels(mode, 3, 8, "cpu", g)
        assert torch.equal(lv, train.time_shift_from_normal(torch.randn(shape, dtype=bf16, generator=g2)))
        t, w = train.frame_schedule(mode, lv, 8, 0.5, g)
        if mode == "first_frame":
            cond = torch.rand(3, generator=g2) < 0.5
            assert torch.equal(w[:, 0] == 0, cond) and float(w[:, 1:].min()) == 1.0
            assert torch.equal(t[:, 1], lv)
        else:
            assert t is lv and float(w.min()) == 1.0
        assert torch.equal(torch.randn(4, generator=g), torch.randn(4, generator=g2))  # the same state afterwards


# ------------------------------------------------------------------------------------- refusals ----
def tiny(**kw):
    return M.DiT(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=144, depth=2, num_heads=2,
                 cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False, **kw)


def test_ops_refuse_chunk_misuse_before_the_device():
    x = torch.zeros(1, 2, 48, 64, dtype=bf16)  # CPU tensors: a launch would fail loudly
    lse = torch.zeros(1, 2, 48)
    with pytest.raises(ValueError, match="needs frame_major=True"):
        ops.attn_fwd(x, x, x, x, lse, frames=(16, 8), chunk=2)
    with pytest.raises(ValueError, match="needs frame_major=True"):
        ops.attn_bwd(x, x, x, x, lse, x, x, x, x, frames=(16, 8), chunk=2)
    with pytest.raises(ValueError, match="needs frame_major=True"):
        ops.attn_fwd(x, x, x, x, lse, chunk=4)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="int >= 1"):
            ops.attn_fwd(x, x, x, x, lse, frames=(16, 8), frame_major=True, chunk=bad)
        with pytest.raises(ValueError, match="int >= 1"):
            ops.attn_bwd(x, x, x, x, lse, x, x, x, x, frames=(16, 8), frame_major=True, chunk=bad)
    with pytest.raises(ValueError, match="do not fit"):  # the _fm refusals stay
        ops.attn_fwd(x, x, x, x, lse, frames=(16, 5), frame_major=True, chunk=2)
    with pytest.raises(ValueError, match="not with past or kv_lens"):
        ops.attn_fwd(x, x, x, x, lse, frames=(16, 8), past=8, frame_major=True, chunk=2)


def test_model_refusals_and_no_new_parameter():
    kw = dict(in_channels=16, hidden_size=128, depth=1, num_heads=2, cross_attn_input_size=64)
    for flags in (dict(), dict(frame_causal=True), ):
        with pytest.raises(ValueError, match="frame_causal=True, frame_major=True"):
            M.DiT(frame_chunk=2, **flags, **kw)
        with pytest.raises(ValueError, match="frame_causal=True, frame_major=True"):
            M.DiTBlock(128, 64, 2, frame_chunk=2, **flags)
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="int >= 1"):
            M.DiT(frame_causal=True, frame_major=True, frame_chunk=bad, **kw)
    with pytest.raises(TypeError):
        M.DiTBlock(128, 64, 2, 4.0, True, False, 2)  # keyword-only
    plain = M.DiT(frame_causal=True, frame_major=True, **kw)
    one = M.DiT(frame_causal=True, frame_major=True, frame_chunk=1, **kw)
    two = M.DiT(frame_causal=True, frame_major=True, frame_chunk=2, **kw)
    assert plain.frame_chunk == one.frame_chunk == 1 and M.DiT(**kw).frame_chunk == 1
    assert two.frame_chunk == 2 and all(b.frame_chunk == 2 for b in two.blocks)
    assert [n for n, _ in plain.named_parameters()] == [n for n, _ in two.named_parameters()]  # no parameter is added
    two.load_state_dict(plain.state_dict(), strict=True)  # a frame_chunk=1 checkpoint loads
    with pytest.raises(NotImplementedError, match=r"enable_fp8\(attention=False\)"):
        two.enable_fp8()  # fp8 attention stays refused, as for frame_causal


def test_cached_call_refusals_before_the_device():
    m = tiny(frame_causal=True, frame_major=True, frame_chunk=2)
    ctx = torch.zeros(2, 24, 64)
    x = lambda k: torch.zeros(2, 16, 2 * k, 8, 8)
    with torch.no_grad():
        cache = m.new_frame_cache(2, 5, 4, 4, device="cpu")
        with pytest.raises(ValueError, match="ONE chunk"):  # three frames: more than a chunk
            m(x(3), ctx, torch.zeros(2, 3), rope_start=(2, 3, 4), frame_cache=cache)
        with pytest.raises(ValueError, match="ONE chunk"):  # one frame, and the chunk is not the cache's last
            m(x(1), ctx, torch.zeros(2, 1), rope_start=(2, 3, 4), frame_cache=cache)
        cache.past_frames = 1
        with pytest.raises(ValueError, match="ONE chunk"):  # the past is no whole number of chunks
            m(x(2), ctx, torch.zeros(2, 2), rope_start=(3, 3, 4), frame_cache=cache)
        # valid calls get as far as the device check: a whole chunk, and the short last chunk of the cache's 5 frames
        cache.past_frames = 2
        with pytest.raises(RuntimeError, match="GPU only"):
            m(x(2), ctx, torch.zeros(2, 2), rope_start=(4, 3, 4), frame_cache=cache)
        cache.past_frames = 4
        with pytest.raises(RuntimeError, match="GPU only"):
            m(x(1), ctx, torch.zeros(2, 1), rope_start=(6, 3, 4), frame_cache=cache)
        # a frame_chunk=1 model takes any chunk of frames, as before
        m1 = tiny(frame_causal=True, frame_major=True)
        c1 = m1.new_frame_cache(2, 5, 4, 4, device="cpu")
        c1.past_frames = 1
        with pytest.raises(RuntimeError, match="GPU only"):
            m1(x(3), ctx, torch.zeros(2, 3), rope_start=(3, 3, 4), frame_cache=c1)


def test_sampler_refusals_before_any_model_call():
    class NoCall:
        time_patch_size = 2
        frame_causal = True
        frame_chunk = 2

        def __call__(self, *a, **k):
            raise AssertionError("the model must not be called")

    lat = torch.zeros(1, 16, 16, 8, 8, dtype=bf16)
    kw = dict(latents=lat, device="cpu")
    prompt = torch.zeros(1, 4, 64)
    with pytest.raises(ValueError, match="multiple of 2"):
        sampling.generate_latents(NoCall(), prompt, rollout_frames=3, **kw)
    with pytest.raises(ValueError, match="multiple of 2"):
        sampling.generate_latents(NoCall(), prompt, rollout_frames=1, kv_cache=True, **kw)
    with pytest.raises(ValueError, match="rollout_frames=2"):
        sampling.generate_latents(NoCall(), prompt, rollout_frames=4, kv_cache=True, **kw)
    with pytest.raises(ValueError, match="whole number of chunks"):  # one token-frame of conditioning: half a chunk
        sampling.generate_latents(NoCall(), prompt, rollout_frames=2, cond_latents=torch.zeros(1, 16, 2, 8, 8), **kw)
    with pytest.raises(ValueError, match="whole number of chunks"):
        sampling.generate_latents(NoCall(), prompt, rollout_frames=2, kv_cache=True,
                                  cond_latents=torch.zeros(1, 16, 6, 8, 8), **kw)
    with pytest.raises(AssertionError, match="must not be called"):  # valid arguments reach the model
        sampling.generate_latents(NoCall(), prompt, rollout_frames=2, cond_latents=torch.zeros(1, 16, 4, 8, 8),
                                  cfg_scale=1.0, inference_steps=1, rope_starts=[(0, 0, 0)] * 8, **kw)


# ------------------------------------------------------------------------------------------- ABI ----
def test_abi_declares_the_chunk_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vds.h")).read(), flags=re.S)
    names = ("vds_attn_fwd_causal_fm_chunk", "vds_attn_bwd_causal_fm_chunk")
    for name in names:
        assert re.search(rf"\bint\s+{name}\s*\(\s*const\s+vds_attn_args\s*\*[^,]*,\s*const\s+vds_mod_groups\s*\*\s*frames\s*,"
                         rf"\s*int32_t\s+chunk\s*,\s*vds_stream_t\s+stream\s*\)\s*;", src), name
        assert _lib.SIGNATURES[name] == [C.POINTER(_lib.AttnArgs), C.c_void_p, C.c_int32, C.c_void_p]
    assert C.sizeof(_lib.ModGroups) == 8  # vds_mod_groups keeps its layout
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), name
    fr = C.byref(_lib.ModGroups(16, 8))

    def args(L=48, Lk=None, ones=0):
        a = _lib.AttnArgs()
        a.B, a.H, a.Lq, a.Lk, a.head_dim = 1, 2, L, L if Lk is None else Lk, 64
        for f in ("q", "k", "v", "o", "lse", "d_o", "dq", "dk", "dv", "delta"):
            setattr(a, f, 16)  # never dereferenced: every call below is refused on the host
        a.kv_pad_ones = ones
        return a
    for fn in (lib.vds_attn_fwd_causal_fm_chunk, lib.vds_attn_bwd_causal_fm_chunk):
        for chunk in (1, 2, 11):
            assert fn(None, fr, chunk, None) == -1
            assert fn(C.byref(_lib.AttnArgs()), fr, chunk, None) == -1
            assert fn(C.byref(args()), None, chunk, None) == -1                               # NULL frames
            assert fn(C.byref(args(Lk=56)), fr, chunk, None) == -1                            # Lq != Lk
            assert fn(C.byref(args(ones=2)), fr, chunk, None) == -1                           # the cross-attention layout
            assert fn(C.byref(args()), C.byref(_lib.ModGroups(16, 5)), chunk, None) == -1     # frames that do not fit
            assert fn(C.byref(args(L=(1 << 21) + 8)), C.byref(_lib.ModGroups(0, 8)), chunk, None) == -2
        for chunk in (0, -1, -(1 << 31)):
            assert fn(C.byref(args()), fr, chunk, None) == -1                                 # chunk < 1
