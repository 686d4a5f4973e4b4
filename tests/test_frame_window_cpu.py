"""Sliding-window chunk-causal self-attention (frame_window) without a GPU: the dense window mask against a double loop
over its definition in token rows and in frame-major rows; the mask as the WIN kernels apply it -- the two key-tile ranges
of the forward / dQ kernels, the query sweep of the dK/dV kernels and the full sweep of a workgroup that holds a lead key,
the open tests, the per-lane compares -- against the dense mask for every GPU shape and every tile size, with tight bounds;
a window that covers every chunk against the chunk mask; one flipped pair at each window bound against the mask census; the
fp32 helper model under the window mask against its ring-cached chunk calls at every position of videos that wrap the ring;
every refusal that is raised before the device is touched; the ring cache's row count; the C symbols."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from video_diffusion_speedrun_amd import _lib, model as M, ops, sampling

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_census as AC  # noqa: E402
import frame_chunk_ref as CH  # noqa: E402
import frame_major_ref as FM  # noqa: E402
import frame_window_ref as FW  # noqa: E402
from test_attn_census_cpu import flipped, norm_checks_accept  # noqa: E402

KC = FW.KC
bf16, f32 = torch.bfloat16, torch.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = FW.ids
N_REG = FW.N_REG


def rel(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


# ------------------------------------------------------------------------------------------ mask ----
@pytest.mark.parametrize("shape", [s for s in FW.SHAPES if s[0] <= 300], ids=ids)
def test_dense_mask_against_a_double_loop(shape):
    L, lead, period, c, w = shape
    S = (L - lead) // period
    W = w // c
    assert (L - lead) % period == 0 and w % c == 0 and W >= 1
    mt, mf = FW.allowed_tok(L, lead, period, c, w), FW.allowed(L, lead, period, c, w)
    ct = [None if l < lead else ((l - lead) % period) // c for l in range(L)]  # chunk of a token row, None: a lead row
    cf = [None if r < lead else (r - lead) // (c * S) for r in range(L)]        # ... of a frame-major row

    def attends(cq, ck):  # the definition
        if cq is None:
            return ck is None
        return ck is None or max(0, cq - W + 1) <= ck <= cq
    for q in range(L):
        for k in range(L):
            assert bool(mt[q, k]) == attends(ct[q], ct[k]), (q, k)
            assert bool(mf[q, k]) == attends(cf[q], cf[k]), (q, k)
    tok = FM.tok_index(L, lead, period)
    assert torch.equal(mf, mt[tok][:, tok])  # the same mask, rows permuted
    assert mf.diagonal().all(), "every row attends at least itself: no empty row"
    # the bounds state the mask: [0, lead) and [kbeg, kend) per query, [qstart, qend) per key
    for r in range(L):
        kb, ke = FW.key_begin(r, lead, S, c, W), CH.key_end(r, r + 1, lead, S, c, L)
        want = torch.zeros(L, dtype=torch.bool)
        want[:lead] = True
        want[kb:ke] = True
        assert torch.equal(mf[r], want), r
        assert ops.fm_key_begin(r, lead, S, c, W) == kb and ops.fm_key_begin(r, lead, S, c) == lead
        qs, qe = CH.query_start(r, lead, S, c), FW.query_end(r, lead, S, c, W, L)
        want = torch.zeros(L, dtype=torch.bool)
        want[qs:qe] = True
        assert torch.equal(mf[:, r], want), r
        assert ops.fm_query_end(r + 1, lead, S, c, W, L) == qe and ops.fm_query_end(r + 1, lead, S, c, None, L) == L


def test_the_large_masks_are_the_token_masks_permuted():
    for L, lead, period, c, w in [s for s in FW.SHAPES if s[0] > 300]:
        tok = FM.tok_index(L, lead, period)
        assert torch.equal(FW.allowed(L, lead, period, c, w), FW.allowed_tok(L, lead, period, c, w)[tok][:, tok])


def test_a_window_of_every_chunk_is_the_chunk_mask():
    for L, lead, period, c, w in FW.SHAPES:
        n = -(-period // c)
        for W in (n, n + 1, 4 * n):
            assert torch.equal(FW.allowed(L, lead, period, c, W * c), CH.allowed(L, lead, period, c))
            assert torch.equal(FW.allowed_tok(L, lead, period, c, W * c), CH.allowed_tok(L, lead, period, c))
        if n > 1:
            assert not torch.equal(FW.allowed(L, lead, period, c, (n - 1) * c), CH.allowed(L, lead, period, c))


# ----------------------------------------------------------------------------------- tile bounds ----
@pytest.mark.parametrize("shape", FW.SHAPES, ids=ids)
def test_the_mask_as_the_kernels_apply_it_is_the_dense_mask(shape):
    L, lead, period, c, w = shape
    m = FW.allowed(L, lead, period, c, w)
    for tile in FW.TILES:
        for wave_rows, sub in ((32, 32), (64, 32), (16, 16), (32, 16), (64, 16)):
            if wave_rows <= tile:
                got, tight = FW.mask_by_tiles(L, lead, period, c, w, tile, wave_rows, sub)
                assert torch.equal(got, m), (tile, wave_rows, sub)
                assert tight, (tile, "a second range starts before the tile that holds kbeg of the first token query")
        for qtile in (32, 64, 128):
            for wave_keys in (32, 16):
                if wave_keys <= tile:
                    assert torch.equal(FW.mask_by_key_tiles(L, lead, period, c, w, tile, qtile, wave_keys), m), (tile, qtile)


def test_tight_query_sweeps_of_the_key_tiles():
    """the dK/dV sweep of a workgroup without a lead key ends at the tile that holds the last attending query"""
    for L, lead, period, c, w in FW.SHAPES:
        S, W = (L - lead) // period, w // c
        m = FW.allowed(L, lead, period, c, w)
        last_query = torch.where(m, torch.arange(L)[:, None], torch.full((1, 1), -1)).amax(0)  # per key
        for k0 in range(0, L, 128):
            k1 = min(k0 + 128, L)
            qe = L if k0 < lead else FW.query_end(k1 - 1, lead, S, c, W, L)
            assert int(last_query[k0:k1].max()) == qe - 1, (L, k0)


def test_the_skips_and_the_open_sub_blocks_do_occur():
    """(1040, 16, 8, 1, 2): S = 128, frame f at rows 16 + 128 f.  The last full 256-query workgroup (768 .. 1023) starts in
    frame 5: its first token query's window starts at frame 4 (row 528), so after tile 0 (the lead keys) it skips the tiles
    1 .. 7 and visits 8 .. 16; the 16-row workgroup from 1024 (frame 7) skips 1 .. 11.  The dK/dV workgroup of keys
    128 .. 255 (frames 0, 1) ends below qend = 16 + 3 * 128 = 400: the query tiles past row 448 are skipped."""
    L, lead, period, c, w = 1040, 16, 8, 1, 2
    S, W = 128, 2
    assert FW.fwd_tiles(768, 1024, lead, S, c, W, L) == (1, 8, 17)
    assert FW.fwd_tiles(1024, 1040, lead, S, c, W, L) == (1, 12, 17)
    assert FW.fwd_tiles(896, 1024, lead, S, c, W, L) == (1, 10, 17)
    assert FW.fwd_tiles(0, 128, lead, S, c, W, L) == (1, 1, 3)  # lead tile and first range touch: nothing skipped
    assert FW.query_end(255, lead, S, c, W, L) == 400 and CH.query_start(128, lead, S, c) == 16
    vis, tot = FW.tiles_visited(L, lead, period, c, w)
    assert vis < CH.tiles_visited(L, lead, period, c)[0] < tot
    # (656, 80, 9, 1, 2): the lead rows span two key tiles
    assert FW.fwd_tiles(512, 640, 80, 64, 1, 2, 656)[0] == 2
    # lead = 0: no lead tile, the loop starts at the window
    assert FW.fwd_tiles(768, 1024, 0, 256, 1, 1, 1024) == (0, 12, 16)


def test_tile_fraction_at_the_training_shape():
    """C3b: L = 8208 = 16 + 8 * 1024, c = 1: a window of w frames visits about (w + 1) 16 of the 129 key tiles per late
    query tile; w = 8 is the frame-causal loop"""
    prev = 0.0
    for w in (1, 2, 4, 8):
        vis, tot = FW.tiles_visited(8208, 16, 8, 1, w)
        assert tot == 65 * 129 and prev < vis / tot
        prev = vis / tot
    assert FW.tiles_visited(8208, 16, 8, 1, 8) == CH.tiles_visited(8208, 16, 8, 1)
    assert FW.tiles_visited(8208, 16, 8, 1, 1)[0] / tot < 0.16 and FW.tiles_visited(8208, 16, 8, 1, 2)[0] / tot < 0.27


# ---------------------------------------------------------------------------------------- census ----
@pytest.mark.parametrize("hd", FM.HEAD_DIMS)
def test_census_conditions_hold_under_the_window_mask(hd):
    for shape in FW.SHAPES:
        L, lead, period, c, w = shape
        if hd > L:
            continue
        BH = -(-L // hd)
        B, H = (BH + 1) // 2, 2
        mask = FW.census_mask(B, L, lead, period, c, w)
        assert AC.label_counts(mask[:1], hd).max().item() <= AC.MAX_LABEL, shape
        sg = FW.census_signs(B, H, L)
        p = FW.census_probes(B, H, hd, L, lead, period, c)
        assert len(set(p.flatten().tolist())) == L
        if L <= 300:
            assert AC.expect_dkv(mask, p, sg, hd)[2] >= AC.MIN_GAP and AC.expect_dq(mask, p, sg, hd)[1] >= AC.MIN_GAP


def test_the_emulation_passes_the_window_census():
    for shape in [s for s in FW.SHAPES if s[0] <= 300]:
        FW.census(ids(shape), 64, 3, 2, shape)


# (280, 16, 8, c = 2, w = 4): S = 33, G = 66, W = 2; chunks at 16, 82, 148, 214.  Query 148 (chunk 2) attends [0, 16) and
# [82, 214); key 82 (chunk 1) is attended by [82, 214).
BITE = {
    "kbeg_minus_1": (148, 81),   # the first row of chunk 2 gains the last key before its window
    "kbeg": (148, 82),           # ... and loses the first key of its window
    "qend_minus_1": (213, 82),   # the last query that attends key 82 loses it
    "qend": (214, 82),           # ... and the first one past its window gains it
    "lead_key_from_a_far_chunk": (279, 15),  # the last row loses a register key, far outside its window's run
}


@pytest.mark.parametrize("name", list(BITE))
def test_one_flipped_pair_fails_the_census_and_passes_the_norm_checks(name):
    shape = (280, 16, 8, 2, 4)
    L, lead, period, c, w = shape
    S, W = 33, 2
    qr, kr = BITE[name]
    assert FW.key_begin(148, lead, S, c, W) == 82 and FW.query_end(82, lead, S, c, W, L) == 214
    hd, H, B = 64, 2, 5
    right = FW.census_mask(B, L, lead, period, c, w).clone()
    assert bool(right[0, qr, kr]) == (name in ("kbeg", "qend_minus_1", "lead_key_from_a_far_chunk"))
    if name in ("kbeg_minus_1", "qend"):  # excluded here, attended under the chunk mask
        assert CH.allowed(L, lead, period, c)[qr, kr]
    p = FW.census_probes(B, H, hd, L, lead, period, c)
    b = next(i for i in range(B) if (p[i] == qr).any() and (p[i] == kr).any())
    wrong = flipped(right, b, qr, kr)
    assert (wrong != right).sum().item() == 1
    FW.census(name, hd, B, H, shape)
    bad_run = lambda q, k, v, do, m: AC.emulate(q, k, v, do, wrong)
    with pytest.raises(AssertionError, match=rf"\[b={b}, h=0, q={qr}\]"):
        FW.census(name, hd, B, H, shape, run=bad_run, bwd=False)
    q, k, v = AC.forward_inputs(hd, B, H, L, L)
    with pytest.raises(AssertionError, match=rf"o\[b={b}, h=0, q={qr}, c={kr % hd}\]"):
        AC.check_labels(name, AC.emulate(q, k, v, None, wrong)[0], right)
    sg = FW.census_signs(B, H, L)
    q, k, v, do = AC.dkv_probe_inputs(hd, B, H, L, L, p, sg)
    edv, edk, _ = AC.expect_dkv(right, p, sg, hd)
    _, _, _, dk, dv = AC.emulate(q, k, v, do, wrong)
    with pytest.raises(AssertionError, match=rf"\[b={b}, h=\d, row={kr}, c="):
        AC.check_support_and_values(name + ".dv", dv, edv, AC.REL_DV)
    with pytest.raises(AssertionError, match=rf"\[b={b}, h=\d, row={kr}, c="):
        AC.check_support_and_values(name + ".dk", dk, edk, AC.REL_DK)
    q, k, v, do = AC.dq_probe_inputs(hd, B, H, L, L, p, sg)
    edq, _ = AC.expect_dq(right, p, sg, hd)
    with pytest.raises(AssertionError, match=rf"\[b={b}, h=\d, row={qr}, c="):
        AC.check_support_and_values(name + ".dq", AC.emulate(q, k, v, do, wrong)[2], edq, AC.REL_DK)
    g = torch.Generator().manual_seed(401)
    rand = [torch.randn(B, H, L, hd, generator=g).to(bf16) for _ in range(4)]
    assert norm_checks_accept(*rand, wrong, right), "the norm checks see this flip"


# ------------------------------------------------------------------------------- model and ring ----
LEVELS = [0.5, 0.25]


@pytest.mark.parametrize("frames,c,w", [(7, 1, 2), (8, 2, 4), (5, 2, 4)], ids=["t7_c1_w2", "t8_c2_w4", "t5_c2_w4_short"])
def test_ring_cached_chunks_are_the_window_model_at_every_position(frames, c, w):
    """(7, 1, 2): seven chunks through two slots, the ring wraps three times; (8, 2, 4): four chunks through two slots;
    (5, 2, 4): the video fits the ring, its short last chunk sits in the last slot"""
    cfg, P, latent, ctx = FW.long_case(frames)
    pt = cfg.time_patch_size
    outs = FW.ring_rollout(P, cfg, latent, ctx, frames, c, w, LEVELS)
    assert len(outs) == -(-frames // c)
    worst = 0.0
    for n, out in enumerate(outs):
        f0, f1 = n * c, min(n * c + c, frames)
        ts = torch.ones(2, frames)
        ts[:, :f0] = 0
        ts[:, f0:f1] = torch.tensor(LEVELS)[:, None].to(bf16).float()
        with torch.no_grad():
            full = FW.dit_forward(P, cfg, latent.float(), ctx.float(), ts, KC.BASE, c, w, reg=torch.tensor(KC.REG))
        e = rel(out, full[:, :, f0 * pt:f1 * pt])
        worst = max(worst, e)
        assert e <= 1e-5, (n, e)
        if n * c >= w:  # the unwindowed chunk model is another model from the first chunk that loses a frame
            other = CH.dit_forward(P, cfg, latent.float(), ctx.float(), ts, KC.BASE, c, reg=torch.tensor(KC.REG))
            assert rel(other[:, :, f0 * pt:f1 * pt], full[:, :, f0 * pt:f1 * pt]) > 1e-3
    print(f"t = {frames}, c = {c}, w = {w}: ring-cached vs full-sequence window model, worst {worst:.2e}")


def test_the_window_model_forgets_frames_behind_its_window():
    cfg, P, latent, ctx = FW.long_case(7)
    pt = cfg.time_patch_size
    ts = torch.tensor([[0.5, 0.25, 0.75, 0.125, 0.9375, 0.375, 0.625]] * 2)
    other = latent.clone()
    other[:, :, 2 * pt:3 * pt] = (latent[:, :, 2 * pt:3 * pt].float() + 3.0).to(bf16)  # frame 2
    with torch.no_grad():
        a = FW.dit_forward(P, cfg, latent.float(), ctx.float(), ts, KC.BASE, 1, 2, reg=torch.ones(2))
        b = FW.dit_forward(P, cfg, other.float(), ctx.float(), ts, KC.BASE, 1, 2, reg=torch.ones(2))
    assert torch.equal(a[:, :, :2 * pt], b[:, :, :2 * pt])            # earlier frames: causal
    assert rel(b[:, :, 3 * pt:4 * pt], a[:, :, 3 * pt:4 * pt]) > 1e-2  # frame 3 sees frame 2
    # (frame 4 does not ATTEND frame 2, but reads frame 3's hidden states, which moved: the window is per layer)
    assert rel(b[:, :, 4 * pt:5 * pt], a[:, :, 4 * pt:5 * pt]) > 0


# ------------------------------------------------------------------------------------- refusals ----
def tiny(**kw):
    return M.DiT(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=144, depth=2, num_heads=2,
                 cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False, **kw)


def test_ops_refuse_window_misuse_before_the_device():
    x = torch.zeros(1, 2, 48, 64, dtype=bf16)  # CPU tensors: a launch would fail loudly
    lse = torch.zeros(1, 2, 48)
    with pytest.raises(ValueError, match="needs frame_major=True"):
        ops.attn_fwd(x, x, x, x, lse, frames=(16, 8), window=2)
    with pytest.raises(ValueError, match="needs frame_major=True"):
        ops.attn_bwd(x, x, x, x, lse, x, x, x, x, frames=(16, 8), window=2)
    with pytest.raises(ValueError, match="needs frame_major=True and no past"):
        ops.attn_fwd(x, x, x, x, lse, frames=(16, 8), past=8, frame_major=True, window=2)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="window = .* must be an int >= 1"):
            ops.attn_fwd(x, x, x, x, lse, frames=(16, 8), frame_major=True, window=bad)
        with pytest.raises(ValueError, match="window = .* must be an int >= 1"):
            ops.attn_bwd(x, x, x, x, lse, x, x, x, x, frames=(16, 8), frame_major=True, chunk=2, window=bad)
    with pytest.raises(ValueError, match="do not fit"):  # the _fm refusals stay
        ops.attn_fwd(x, x, x, x, lse, frames=(16, 5), frame_major=True, window=2)


def test_model_refusals_and_no_new_parameter():
    kw = dict(in_channels=16, hidden_size=128, depth=1, num_heads=2, cross_attn_input_size=64)
    for flags in (dict(), dict(frame_causal=True)):
        with pytest.raises(ValueError, match="frame_causal=True, frame_major=True"):
            M.DiT(frame_window=2, **flags, **kw)
        with pytest.raises(ValueError, match="frame_causal=True, frame_major=True"):
            M.DiTBlock(128, 64, 2, frame_window=2, **flags)
    fm = dict(frame_causal=True, frame_major=True)
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="int >= 1"):
            M.DiT(frame_window=bad, **fm, **kw)
    with pytest.raises(ValueError, match="multiple of frame_chunk=2 .* pass frame_window=4"):
        M.DiT(frame_chunk=2, frame_window=3, **fm, **kw)
    with pytest.raises(TypeError):
        M.DiTBlock(128, 64, 2, 4.0, True, False, True, True, 1, 2)  # keyword-only
    import inspect
    for cls in (M.DiT, M.DiTBlock):
        names = list(inspect.signature(cls.__init__).parameters)
        assert names[-2:] == ["frame_window", "qk_norm"] and names[-3] == "frame_chunk"
    plain = M.DiT(**fm, **kw)
    two = M.DiT(frame_window=2, **fm, **kw)
    four = M.DiT(frame_chunk=2, frame_window=4, **fm, **kw)
    assert plain.frame_window is None and M.DiT(**kw).frame_window is None
    assert two.frame_window == 2 and all(b.frame_window == 2 for b in two.blocks)
    assert plain.blocks[0]._mask_kw() == {} and two.blocks[0]._mask_kw() == {"window": 2}
    assert four.blocks[0]._mask_kw() == {"chunk": 2, "window": 2}  # the kernels take the window in chunks
    assert [n for n, _ in plain.named_parameters()] == [n for n, _ in two.named_parameters()]  # no parameter is added
    two.load_state_dict(plain.state_dict(), strict=True)  # a checkpoint without it loads
    with pytest.raises(NotImplementedError, match=r"enable_fp8\(attention=False\)"):
        two.enable_fp8()  # fp8 attention stays refused, as for frame_causal


def test_the_ring_cache_has_a_constant_row_count():
    h = w = 4
    for c, win in ((1, 2), (2, 4), (2, 2), (1, 1)):
        m = tiny(frame_causal=True, frame_major=True, frame_chunk=c, frame_window=win)
        for frames in (win, 8, 50):
            cache = m.new_frame_cache(2, frames, h, w, device="cpu")
            assert cache.frames == frames and cache.ring == (win // c, c)
            for t in cache.k + cache.v:
                assert tuple(t.shape) == (2, 2, N_REG + win * h * w, 96) == (2, 2, FW.ring_rows(win // c, c, h, w), 96)
    unbounded = tiny(frame_causal=True, frame_major=True).new_frame_cache(2, 50, h, w, device="cpu")
    assert unbounded.ring is None and unbounded.k[0].shape[2] == N_REG + 50 * h * w
    m = tiny(frame_causal=True, frame_major=True, frame_chunk=2, frame_window=4)
    with pytest.raises(ValueError, match="whole number of chunks .*e.g. 8"):
        m.new_frame_cache(2, 7, h, w, device="cpu")  # wraps, and the last chunk is short
    assert m.new_frame_cache(2, 3, h, w, device="cpu").frames == 3  # a short last chunk inside the ring is fine


def test_ring_slots_and_key_rows():
    m = tiny(frame_causal=True, frame_major=True, frame_chunk=2, frame_window=6)  # W = 3 slots of 2 frames of 16 tokens
    cache = m.new_frame_cache(2, 12, 4, 4, device="cpu")
    seen = []
    for n in range(6):
        cache.past_frames = 2 * n
        seen.append(cache.ring_call(2))
    assert seen == [(0, 16 + 32), (32, 16 + 64), (64, 16 + 96), (0, 16 + 96), (32, 16 + 96), (64, 16 + 96)]
    small = m.new_frame_cache(2, 5, 4, 4, device="cpu")  # the short last chunk (one frame) while the ring fills
    small.past_frames = 4
    assert small.ring_call(1) == (64, 16 + 64 + 16)


def test_cached_call_refusals_before_the_device():
    ctx = torch.zeros(2, 24, 64)
    x = lambda k: torch.zeros(2, 16, 2 * k, 8, 8)
    with torch.no_grad():
        m1 = tiny(frame_causal=True, frame_major=True, frame_window=2)
        cache = m1.new_frame_cache(2, 9, 4, 4, device="cpu")
        with pytest.raises(ValueError, match="ONE token group .* one token-frame per call"):
            m1(x(2), ctx, torch.zeros(2, 2), rope_start=(2, 3, 4), frame_cache=cache)
        with pytest.raises(RuntimeError, match="GPU only"):  # one frame: as far as the device check
            m1(x(1), ctx, torch.zeros(2, 1), rope_start=(2, 3, 4), frame_cache=cache)
        cache.past_frames = 8  # far past the ring's two slots: `frames` is the whole video's length
        with pytest.raises(RuntimeError, match="GPU only"):
            m1(x(1), ctx, torch.zeros(2, 1), rope_start=(10, 3, 4), frame_cache=cache)
        cache.past_frames = 9
        with pytest.raises(ValueError, match="make a larger cache"):
            m1(x(1), ctx, torch.zeros(2, 1), rope_start=(11, 3, 4), frame_cache=cache)
        m2 = tiny(frame_causal=True, frame_major=True, frame_chunk=2, frame_window=4)
        c2 = m2.new_frame_cache(2, 8, 4, 4, device="cpu")
        with pytest.raises(ValueError, match="ONE chunk"):
            m2(x(3), ctx, torch.zeros(2, 3), rope_start=(2, 3, 4), frame_cache=c2)
        with pytest.raises(RuntimeError, match="GPU only"):
            m2(x(2), ctx, torch.zeros(2, 2), rope_start=(2, 3, 4), frame_cache=c2)
        # the caches are not interchangeable
        cache.past_frames = 0
        plain = tiny(frame_causal=True, frame_major=True)
        with pytest.raises(ValueError, match="not made by this model's new_frame_cache"):
            plain(x(1), ctx, torch.zeros(2, 1), rope_start=(2, 3, 4), frame_cache=cache)
        with pytest.raises(ValueError, match="not made by this model's new_frame_cache"):
            m1(x(1), ctx, torch.zeros(2, 1), rope_start=(2, 3, 4), frame_cache=plain.new_frame_cache(2, 9, 4, 4, device="cpu"))
        with pytest.raises(ValueError, match="not made by this model's new_frame_cache"):
            m2(x(2), ctx, torch.zeros(2, 2), rope_start=(2, 3, 4), frame_cache=cache)


def test_sampler_refusals_before_any_model_call():
    class NoCall:
        time_patch_size = 2
        frame_causal = True
        frame_chunk = 1
        frame_window = 2

        def __call__(self, *a, **k):
            raise AssertionError("the model must not be called")

    lat = torch.zeros(1, 16, 16, 8, 8, dtype=bf16)
    prompt = torch.zeros(1, 4, 64)
    with pytest.raises(ValueError, match="pass rollout_frames=1"):
        sampling.generate_latents(NoCall(), prompt, rollout_frames=2, kv_cache=True, latents=lat, device="cpu")
    with pytest.raises(AssertionError, match="must not be called"):  # uncached: any number of frames at a time
        sampling.generate_latents(NoCall(), prompt, rollout_frames=2, cfg_scale=1.0, inference_steps=1,
                                  rope_starts=[(0, 0, 0)] * 8, latents=lat, device="cpu")


# ------------------------------------------------------------------------------------------- ABI ----
def test_abi_declares_the_window_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vds.h")).read(), flags=re.S)
    names = ("vds_attn_fwd_causal_fm_window", "vds_attn_bwd_causal_fm_window")
    for name in names:
        assert re.search(rf"\bint\s+{name}\s*\(\s*const\s+vds_attn_args\s*\*[^,]*,\s*const\s+vds_mod_groups\s*\*\s*frames\s*,"
                         rf"\s*int32_t\s+chunk\s*,\s*int32_t\s+window_chunks\s*,\s*vds_stream_t\s+stream\s*\)\s*;", src), name
        assert _lib.SIGNATURES[name] == [C.POINTER(_lib.AttnArgs), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
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
    for fn in (lib.vds_attn_fwd_causal_fm_window, lib.vds_attn_bwd_causal_fm_window):
        for chunk, win in ((1, 2), (2, 2), (1, 8), (3, 40), (11, 1)):  # windowed, and forwarded to the _fm_chunk calls
            assert fn(None, fr, chunk, win, None) == -1
            assert fn(C.byref(_lib.AttnArgs()), fr, chunk, win, None) == -1
            assert fn(C.byref(args()), None, chunk, win, None) == -1                               # NULL frames
            assert fn(C.byref(args(Lk=56)), fr, chunk, win, None) == -1                            # Lq != Lk
            assert fn(C.byref(args(ones=2)), fr, chunk, win, None) == -1                           # the cross-attention layout
            assert fn(C.byref(args()), C.byref(_lib.ModGroups(16, 5)), chunk, win, None) == -1     # frames that do not fit
            assert fn(C.byref(args(L=(1 << 21) + 8)), C.byref(_lib.ModGroups(0, 8)), chunk, win, None) == -2
        for chunk, win in ((0, 1), (-1, 2), (1, 0), (2, -1), (1, -(1 << 31))):
            assert fn(C.byref(args()), fr, chunk, win, None) == -1                                 # chunk < 1, window < 1
