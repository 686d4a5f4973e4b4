"""Teacher forcing without a GPU: the teacher mask -- a double loop over its definition -- against both views of its bounds
(a prefix plus one run for a query, a run with a hole for a key), in frame-major and in token rows; the mask as the kernels
apply it, two tile ranges per workgroup, no tile twice; the layout proof -- the helper's teacher forward restricted to noisy
chunk i IS frame_chunk_ref's cached chunk call on chunk i, and it is far from a model without its clean context; one flipped
pair at each new bound against the mask census; every refusal raised before the device is touched; the C symbols and their
defect table; the trainer's "teacher" mode consumes the generator like "chunk"."""
import ctypes as C
import inspect
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from video_diffusion_speedrun_amd import _lib, graph, model as M, ops, train

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_census as AC  # noqa: E402
import frame_chunk_ref as CH  # noqa: E402
import frame_major_ref as FM  # noqa: E402
import teacher_defects as TD  # noqa: E402
import teacher_ref as TR  # noqa: E402
from test_attn_census_cpu import flipped, norm_checks_accept  # noqa: E402

KC = CH.KC
bf16, f32 = torch.bfloat16, torch.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = TR.ids


def rel(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


# ------------------------------------------------------------------------------------------ mask ----
def test_the_issue_shapes():
    assert [s[0] for s in TR.SHAPES] == [154, 384, 316, 656, 568, 108]
    L, lead, period, c = TR.SHAPES[4]  # (6, 46, 1): noisy chunk 1 reads [0, 62) and [338, 384)
    assert TR.query_bounds(340, L, lead, period, c) == (62, 338, 384)
    assert TR.fwd_tiles(338, 384, L, lead, period, c)[:2] == (1, 5)  # a gap of key tiles between the two ranges


@pytest.mark.parametrize("shape", TR.CPU_SHAPES, ids=ids)
def test_both_views_of_the_bounds_are_the_dense_mask(shape):
    L, lead, period, c = shape
    want = TR.allowed(*shape)
    assert torch.equal(TR.mask_from_query_bounds(*shape), want)
    assert torch.equal(TR.mask_from_key_bounds(*shape), want)
    tok = FM.tok_index(L, lead, period)
    assert torch.equal(want, TR.allowed_tok(*shape)[tok][:, tok])  # the same mask in token rows, permuted
    n, S, G, base = TR.geometry(*shape)
    # the clean half is the chunk-causal mask of the first base rows
    assert torch.equal(want[:base, :base], CH.allowed(base, lead, n, min(c, n)))
    assert not want[:base, base:].any(), "a clean or lead query attends no noisy key"
    if lead:
        assert want[:, :lead].all() and not want[:lead, lead:].any()
    for r in range(lead, L):  # every token row attends its own chunk: no empty row even without lead rows
        assert want[r, r]
    for r in range(L):
        pend, kbeg, kend = TR.query_bounds(r, *shape)
        assert pend <= kbeg <= kend <= L
        qstart, qend, q2 = TR.key_bounds(r, *shape)
        assert qstart < qend <= q2 <= L


@pytest.mark.parametrize("shape", TR.CPU_SHAPES, ids=ids)
def test_the_mask_as_the_kernels_apply_it_is_the_dense_mask(shape):
    """the tile sweeps cover every attended pair and visit no tile twice (asserted inside); 128 is the kernels' workgroup"""
    want = TR.allowed(*shape)
    for tile in (64, 128, 256):
        assert torch.equal(TR.mask_by_tiles(*shape, tile), want), tile
        assert torch.equal(TR.mask_by_key_tiles(*shape, tile), want), tile


def test_the_skips_occur_and_the_pair_counts_match_the_tiles():
    shape = TR.shape_of(8, 1024, 1)
    vis, tot = TR.tiles_visited(*shape)
    kvis, ktot = TR.query_tiles_visited(*shape)
    print(f"n = 8, S = 1024, c = 1: forward / dQ visit {vis} of {tot} key tiles, dK/dV {kvis} of {ktot} query tiles")
    assert vis < 0.4 * tot and kvis < 0.4 * ktot
    for shape in TR.SHAPES:
        L = shape[0]
        vis, _ = TR.tiles_visited(*shape)
        assert TR.pairs_q(*shape) <= vis * 64 * 128 and TR.pairs_q(*shape) >= int(TR.allowed(*shape).sum())
        assert TR.pairs_k(*shape) >= int(TR.allowed(*shape).sum())
    # a workgroup of noisy keys sweeps its own chunk's query tiles only
    L, lead, period, c = shape = TR.shape_of(4, 256, 1)
    base = lead + 4 * 256
    a0, a1, b0, nqt = TR.key_sweep(base + 256 + 112, base + 256 + 240, *shape)
    assert (a0, a1, b0) == ((base + 256) // 64, -(-(base + 512) // 64), nqt)


# ---------------------------------------------------------------------------------------- census ----
@pytest.mark.parametrize("hd", FM.HEAD_DIMS)
def test_census_conditions_hold_under_the_teacher_mask(hd):
    for shape in TR.SHAPES:
        L, lead, period, c = shape
        BH = -(-L // hd)
        B, H = (BH + 1) // 2, 2
        mask = TR.census_mask(B, *shape)
        assert AC.label_counts(mask[:1], hd).max().item() <= AC.MAX_LABEL, shape
        p = TR.census_probes(B, H, hd, *shape)
        assert len(set(p.flatten().tolist())) == L
        if L <= 320:
            sg = AC.signs(B, H, L)
            assert AC.expect_dkv(mask, p, sg, hd)[2] >= AC.MIN_GAP and AC.expect_dq(mask, p, sg, hd)[1] >= AC.MIN_GAP


def test_the_emulation_passes_the_teacher_census():
    for shape in [s for s in TR.SHAPES if s[0] <= 320]:
        TR.census(ids(shape), 64, 3, 2, shape)


# (316, 16, 6, c = 2): n = 3, S = 50, G = 100, base = 166; clean chunks at 16, 116; noisy chunks at 166, 266.
# Query 266 (noisy chunk 1) attends [0, 116) and [266, 316); clean key 16 is read by [16, 166) and [266, 316).
BITE = {
    "pend_minus_1": (266, 115),    # the noisy chunk loses the last clean key of the chunk before it
    "pend": (266, 116),            # ... and gains the first clean key of its own chunk (the one it must not see)
    "kbeg_minus_1": (266, 265),    # gains the last key of the noisy chunk before it
    "kbeg": (266, 266),            # loses its own first key
    "hole_first": (166, 16),       # the first noisy row gains a clean key of chunk 0: the first row of the hole
    "hole_last": (265, 16),        # ... the last row of the hole
    "q2": (266, 16),               # the first reader behind the hole loses the key
    "clean_sees_noisy": (165, 166),  # the last clean row gains the first noisy key
}


@pytest.mark.parametrize("name", list(BITE))
def test_one_flipped_pair_fails_the_census_and_passes_the_norm_checks(name):
    shape = TR.SHAPES[2]
    L, lead, period, c = shape
    assert shape == (316, 16, 6, 2)
    qr, kr = BITE[name]
    assert TR.query_bounds(266, *shape) == (116, 266, 316) and TR.key_bounds(16, *shape) == (16, 166, 266)
    hd, H, B = 64, 2, 5
    right = TR.census_mask(B, *shape).clone()
    assert bool(right[0, qr, kr]) == (name in ("pend_minus_1", "kbeg", "q2"))
    p = TR.census_probes(B, H, hd, *shape)
    b = next(i for i in range(B) if (p[i] == qr).any() and (p[i] == kr).any())
    wrong = flipped(right, b, qr, kr)
    assert (wrong != right).sum().item() == 1
    bad_run = lambda q, k, v, do, m: AC.emulate(q, k, v, do, wrong)
    with pytest.raises(AssertionError, match=rf"\[b={b}, h=0, q={qr}\]"):
        TR.census(name, hd, B, H, shape, run=bad_run, bwd=False)
    sg = AC.signs(B, H, L)
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


# ---------------------------------------------------------------------------------- layout proof ----
LEVELS = [[0.5, 0.25, 0.9375], [0.125, 0.75, 0.0625]]  # one level per chunk and sample


def teacher_case(chunk):
    """frame_chunk_ref.long_case (5 token-frames of 16 tokens, hd64, depth 3): clean latents, a noisy copy, per-frame levels"""
    cfg, P, latent, ctx = CH.long_case()
    n = CH.T_FRAMES
    n_chunks = -(-n // chunk)
    lv = torch.tensor(LEVELS)[:, :n_chunks] if n_chunks <= 3 else torch.linspace(0.1, 0.9, 2 * n_chunks).view(2, n_chunks)
    ts = lv.repeat_interleave(chunk, dim=1)[:, :n].to(bf16).float()
    # the trainer's noising: z_t = (1 - t) x + t noise, per token-frame
    g = torch.Generator().manual_seed(4242)
    tt = ts.repeat_interleave(cfg.time_patch_size, dim=1)[:, None, :, None, None]
    noisy = ((1 - tt) * latent.float() + tt * torch.randn(latent.shape, generator=g)).to(bf16)
    return cfg, P, latent, noisy, ctx, ts


@pytest.mark.parametrize("chunk", [1, 2, 3, 5])
def test_teacher_forward_is_the_cached_chunk_call_at_every_chunk_position(chunk):
    """one teacher call computes for every noisy chunk what the cached rollout computes for it: the cache filled by the
    helper's clean chunk calls at t = 0, the registers at 1.0.  1e-5 in fp32, the bound of test_frame_cache_cpu.py"""
    cfg, P, latent, noisy, ctx, ts = teacher_case(chunk)
    pt, n = cfg.time_patch_size, CH.T_FRAMES
    reg = torch.ones(2)
    with torch.no_grad():
        out = TR.dit_forward(P, cfg, latent.float(), noisy.float(), ctx.float(), ts, KC.BASE, chunk)
        assert tuple(out.shape) == tuple(latent.shape)
        cache = KC.Cache(cfg.depth, n)
        for f0 in range(0, n, chunk):
            f1 = min(f0 + chunk, n)
            sl = slice(f0 * pt, f1 * pt)
            want = CH.chunk_forward(P, cfg, noisy[:, :, sl].float(), ctx.float(), ts[:, f0:f1], KC.BASE, reg, cache, chunk)
            e = rel(out[:, :, sl], want)
            print(f"chunk {chunk}, frames {f0}..{f1 - 1}: teacher vs cached call {e:.2e}")
            assert e < 1e-5, (chunk, f0, e)
            CH.chunk_forward(P, cfg, latent[:, :, sl].float(), ctx.float(), torch.zeros(2, f1 - f0), KC.BASE, reg, cache, chunk)
            cache.commit()


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_the_sibling_case_and_dropping_the_clean_half(name):
    """frame_cache_ref's own case (3 token-frames, its pinned register levels, its chunk levels, the clean latent as the
    chunk's input): the teacher forward at chunk 1 IS chunk_reference at every frame, and -- the statement
    test_frame_cache_cpu.py makes about the past -- without the clean half every later frame is > 4 x 2.5e-2 away, so the
    GPU comparison at 2.5e-2 cannot pass with the clean context ignored"""
    cfg, P, latent, ctx = KC.model_case(name)
    pt = cfg.time_patch_size
    ts = torch.tensor(KC.T_CHUNK)[:, :1].to(bf16).float().expand(2, 3).contiguous()
    reg = torch.tensor(KC.REG)
    with torch.no_grad():
        out = TR.dit_forward(P, cfg, latent.float(), latent.float(), ctx.float(), ts, KC.BASE, 1, reg=reg)
        bare = TR.dit_forward(P, cfg, latent.float(), latent.float(), ctx.float(), ts, KC.BASE, 1, reg=reg, keep_clean=False)
    for f0 in range(3):
        want, _ = KC.chunk_reference(name, f0, 1)
        sl = slice(f0 * pt, (f0 + 1) * pt)
        e, d = rel(out[:, :, sl], want), rel(bare[:, :, sl], want)
        print(f"{name} frame {f0}: teacher vs cached call {e:.2e}, without the clean half {d:.3f}")
        assert e < 1e-5, (name, f0, e)
        if f0:
            assert d > 4 * 2.5e-2, (name, f0, d)
        else:
            assert d < 1e-5  # chunk 0 has no clean context


def test_the_clean_half_is_the_chunk_model_at_level_zero():
    cfg, P, latent, noisy, ctx, ts = teacher_case(2)
    with torch.no_grad():
        both = TR.dit_forward(P, cfg, latent.float(), noisy.float(), ctx.float(), ts, KC.BASE, 2, whole=True)
        clean = CH.dit_forward(P, cfg, latent.float(), ctx.float(), torch.zeros(2, CH.T_FRAMES), KC.BASE, 2, reg=torch.ones(2))
    assert rel(both[:, :, :latent.shape[2]], clean) < 1e-5


# ------------------------------------------------------------------------------------- refusals ----
def tiny(**kw):
    return M.DiT(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=144, depth=2, num_heads=2,
                 cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False, **kw)


def test_ops_refuse_teacher_misuse_before_the_device():
    x = torch.zeros(1, 2, 48, 64, dtype=bf16)  # CPU tensors: a launch would fail loudly
    lse = torch.zeros(1, 2, 48)
    for fn, more in ((ops.attn_fwd, ()), (ops.attn_bwd, (x, x, x, x))):
        with pytest.raises(ValueError, match="teacher=True needs frame_major=True"):
            fn(x, x, x, x, lse, *more, frames=(16, 8), teacher=True)
        with pytest.raises(ValueError, match="teacher=True needs frame_major=True"):
            fn(x, x, x, x, lse, *more, teacher=True)
        with pytest.raises(ValueError, match="excludes window = 2 .* pass window=None"):
            fn(x, x, x, x, lse, *more, frames=(16, 8), frame_major=True, window=2, teacher=True)
        with pytest.raises(ValueError, match="pass kv_lens=None"):
            fn(x, x, x, x, lse, *more, frames=(16, 8), frame_major=True, kv_lens=torch.zeros(1, dtype=torch.int32),
               teacher=True)
        with pytest.raises(ValueError, match=r"even period .* pass frames=\(lead, 2 \* n\)"):
            fn(x, x, x, x, lse, *more, frames=(0, 3), frame_major=True, teacher=True)
        with pytest.raises(ValueError, match="do not fit"):  # the _fm refusals stay
            fn(x, x, x, x, lse, *more, frames=(16, 6), frame_major=True, teacher=True)
        with pytest.raises(ValueError, match="int >= 1"):
            fn(x, x, x, x, lse, *more, frames=(16, 8), frame_major=True, chunk=0, teacher=True)
        assert list(inspect.signature(fn).parameters)[-1] == "teacher"
        assert inspect.signature(fn).parameters["teacher"].default is False
    with pytest.raises(ValueError, match="excludes past = 8 .* pass past=0"):
        ops.attn_fwd(x, x, x, x, lse, frames=(16, 8), frame_major=True, past=8, teacher=True)
    # the routing: the two new entries with (frames, chunk); without the keyword the entry points of before
    a = _lib.AttnArgs()
    a.B, a.H, a.Lq, a.Lk, a.head_dim = 1, 2, 48, 48, 64
    for d in ("fwd", "bwd"):
        name, extra, what = ops._attn_entry(d, a, None, (16, 8), "fr", 0, True, 2, None, True)
        assert (name, extra) == (f"vds_teacher_attn_{d}", ("fr", 2)) and "chunk=2" in what
        assert ops._attn_entry(d, a, None, (16, 8), "fr", 0, True, 2, None)[0] == f"vds_attn_{d}_causal_fm_chunk"
        assert ops._attn_entry(d, a, None, (16, 8), "fr", 0, True, 1, None)[0] == f"vds_attn_{d}_causal_fm"


def test_model_refusals_before_the_device():
    ctx = torch.zeros(2, 24, 64)
    x = torch.zeros(2, 16, 6, 8, 8)
    ts = torch.zeros(2, 3)
    fm = dict(frame_causal=True, frame_major=True)
    assert list(inspect.signature(M.DiT.forward).parameters)[-1] == "teacher_latents"
    with torch.no_grad():
        for flags in (dict(), dict(frame_causal=True)):
            with pytest.raises(ValueError, match="teacher_latents needs .* frame_causal=True, frame_major=True"):
                tiny(**flags)(x, ctx, ts, teacher_latents=x)
        with pytest.raises(ValueError, match="frame_window=2 .* frame_window=None"):
            tiny(frame_window=2, **fm)(x, ctx, ts, teacher_latents=x)
        m = tiny(frame_chunk=2, **fm)
        with pytest.raises(ValueError, match="teacher_latents and frame_cache exclude each other"):
            m(x, ctx, ts, teacher_latents=x, frame_cache=m.new_frame_cache(2, 3, 4, 4, device="cpu"))
        with pytest.raises(ValueError, match=r"per-frame timesteps of shape \[2, 3\] .*expand\(2, 3\)"):
            m(x, ctx, torch.zeros(2), teacher_latents=x)
        with pytest.raises(ValueError, match=r"timesteps must have shape"):
            m(x, ctx, torch.zeros(2, 6), teacher_latents=x)
        for bad in (torch.zeros(2, 16, 4, 8, 8), torch.zeros(2, 16, 12, 8, 8), [1.0]):
            with pytest.raises(ValueError, match=r"teacher_latents must have x's shape \(2, 16, 6, 8, 8\)"):
                m(x, ctx, ts, teacher_latents=bad)
        with pytest.raises(ValueError, match=r"register_timesteps must have shape \[2\]"):
            m(x, ctx, ts, teacher_latents=x, register_timesteps=torch.ones(3))
        with pytest.raises(RuntimeError, match="GPU only"):  # a well-formed call gets as far as the device check
            m(x, ctx, ts, teacher_latents=x, rope_start=(2, 3, 4))
        with pytest.raises(RuntimeError, match="GPU only"):  # without the keyword: the call of before
            m(x, ctx, ts, rope_start=(2, 3, 4))
    blk = m.blocks[0]
    assert blk._mask_kw() == blk._mask_kw((16, 6)) == {"chunk": 2}
    assert blk._mask_kw(M.TeacherFrames((16, 6))) == {"chunk": 2, "teacher": True}
    one = tiny(**fm).blocks[0]
    assert one._mask_kw() == {} and one._mask_kw(M.TeacherFrames((16, 6))) == {"chunk": 1, "teacher": True}
    assert isinstance(blk._check_frames(M.TeacherFrames((16, 6)), 112), M.TeacherFrames)
    assert type(blk._check_frames((16, 6), 112)) is tuple
    with pytest.raises(ValueError, match="frame_major=True and without frame_window"):
        tiny(frame_window=2, **fm).blocks[0]._check_frames(M.TeacherFrames((16, 6)), 112)
    assert "doubled" in M.activation_bytes.__doc__


# ------------------------------------------------------------------------------------- trainer ----
class Recorder:
    """stands in for a DiT: records the call, returns zeros"""
    time_patch_size = 2
    frame_chunk = 2
    frame_causal = frame_major = True
    frame_window = None

    def __init__(self):
        self.calls = []

    def __call__(self, z, ctx, t, **kw):
        self.calls.append((z.clone(), t.clone(), dict(kw)))
        return torch.zeros_like(z)


def host_step(monkeypatch, mode, model=None, **kw):
    """train.forward on the CPU: the noising and the loss kernels replaced by torch stand-ins, everything else as it is"""
    def noise(lat, noise, t, pt):
        tt = t.repeat_interleave(pt, dim=1)[:, None, :, None, None]
        return ((1 - tt) * lat.float() + tt * noise.float()).to(bf16), (noise.float() - lat.float()).to(bf16)
    seen = {}

    def loss(out, v, w, pt):
        seen["out"], seen["w"] = tuple(out.shape), w.clone()
        return torch.zeros(()), torch.zeros(out.shape[0])
    monkeypatch.setattr(ops, "noise_latents_frames", noise)
    monkeypatch.setattr(train, "frame_flow_loss", loss)
    model = Recorder() if model is None else model
    g = torch.Generator().manual_seed(31)
    gl = torch.Generator().manual_seed(32)
    batch = {"latent": torch.randn(3, 16, 10, 8, 8, generator=gl).to(bf16), "context": torch.randn(3, 8, 64, generator=gl)}
    torch.manual_seed(7)  # (the caption dropout draws from the global generator)
    train.forward(model, batch, None, None, "cpu", 0, False, generator=g, rope_start=(2, 3, 4), frame_mode=mode, **kw)
    return model, batch, seen, torch.randn(4, generator=g)


def test_teacher_mode_consumes_the_generator_like_chunk(monkeypatch):
    assert train.FRAME_MODES[-1] == "teacher" and train.FRAME_MODES[:4] == (None, "first_frame", "independent", "chunk")
    mc, _, sc, after_c = host_step(monkeypatch, "chunk")
    mt, batch, st, after_t = host_step(monkeypatch, "teacher")
    (zc, tc, kc), (zt, tt, kt) = mc.calls[0], mt.calls[0]
    assert torch.equal(after_c, after_t), "the generator is left in another state"
    assert torch.equal(zc, zt) and torch.equal(tc, tt), "other draws"
    assert tuple(tt.shape) == (3, 5) and torch.equal(tt[:, 0], tt[:, 1]) and torch.equal(tt[:, 2], tt[:, 3])  # per chunk
    assert "teacher_latents" not in kc and torch.equal(kt["teacher_latents"], batch["latent"])
    assert kt["rope_start"] == kc["rope_start"] == (2, 3, 4)
    assert st["out"] == (3, 16, 10, 8, 8) and float(st["w"].min()) == float(st["w"].max()) == 1.0
    # the overrides work as in the other modes
    ft = torch.full((3, 5), 0.25)
    fw = torch.tensor([[1.0, 0.0, 1.0, 1.0, 0.5]] * 3)
    mo, _, so, _ = host_step(monkeypatch, "teacher", frame_timesteps=ft, frame_weights=fw)
    assert torch.equal(mo.calls[0][1].float(), ft) and torch.equal(so["w"], fw) and "teacher_latents" in mo.calls[0][2]


def test_trainer_refusals(monkeypatch):
    for flags in (dict(frame_causal=False), dict(frame_major=False), dict(frame_window=2)):
        bad = Recorder()
        for k, v in flags.items():
            setattr(bad, k, v)
        with pytest.raises(ValueError, match="frame_mode='teacher' needs a model built with frame_causal=True, frame_major=True"):
            host_step(monkeypatch, "teacher", model=bad)
        assert not bad.calls
    with pytest.raises(ValueError, match="frame_mode must be one of"):
        graph.GraphedTrainStep(None, None, None, "cpu", frame_mode="teachers")


# ------------------------------------------------------------------------------------------- ABI ----
def test_abi_declares_the_teacher_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vds.h")).read(), flags=re.S)
    for name in TD.ENTRIES:
        assert re.search(rf"\bint\s+{name}\s*\(\s*const\s+vds_attn_args\s*\*[^,]*,\s*const\s+vds_mod_groups\s*\*\s*frames\s*,"
                         rf"\s*int32_t\s+chunk\s*,\s*vds_stream_t\s+stream\s*\)\s*;", src), name
        assert _lib.SIGNATURES[name] == [C.POINTER(_lib.AttnArgs), C.c_void_p, C.c_int32, C.c_void_p]
        assert not name.startswith("vds_attn_")
    assert C.sizeof(_lib.ModGroups) == 8 and C.sizeof(_lib.AttnArgs) == C.sizeof(_lib.AttnArgs)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in TD.ENTRIES:
        assert hasattr(raw, name), name
    a = _lib.AttnArgs()
    a.B, a.H, a.Lq, a.Lk, a.head_dim, a.kv_pad_ones = 2, 2, 384, 384, 72, 1
    before = _lib.load().vds_attn_bwd_workspace_bytes(C.byref(a))
    assert before == 2 * 2 * 2 * 384 * 4  # unchanged: the statistics only


def test_every_defect_gets_its_documented_code_in_a_process_without_a_gpu():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "helpers", "teacher_defects.py")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["rows"] >= 80 and not got["wrong"], f"(entry, defect, returned, documented) {got['wrong']}"
