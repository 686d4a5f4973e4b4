"""Frame-causal self-attention without a GPU: the mask map against a literal double loop, argument validation in ops and
the model, the fp8 refusal, the two C symbols, and the causality property of the helper reference model
(tests/helpers/frame_causal_ref.py) that the GPU tests compare the kernels and the model against."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from oracle import dit_oracle as O
from video_diffusion_speedrun_amd import _lib, model as M, ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_causal_ref as FC  # noqa: E402

bf16, f32 = torch.bfloat16, torch.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


# ------------------------------------------------------------------------------------------ mask ----
@pytest.mark.parametrize("L,lead,period", [(40, 16, 8), (23, 5, 3), (28, 16, 1), (28, 16, 12), (12, 0, 4), (9, 0, 1),
                                           (9, 0, 9), (16, 16, 1)],
                         ids=["model", "odd", "period1", "one_row_per_frame", "lead0", "lead0_period1", "triangular", "lead_only"])
def test_mask_against_a_double_loop(L, lead, period):
    m = FC.allowed(L, lead, period)
    assert m.dtype == torch.bool and tuple(m.shape) == (L, L)
    for q in range(L):
        gq = 0 if q < lead else 1 + (q - lead) % period
        assert gq == ops.mod_group_of(q, lead, period)
        for k in range(L):
            gk = 0 if k < lead else 1 + (k - lead) % period
            assert bool(m[q, k]) == (gk <= gq), (q, k)
    assert m.any(dim=1).all(), "every query has a key"
    if L:
        assert m[:, 0].all(), "row 0 is attended by every query"
    if period == 1:  # registers see registers, tokens see everything
        assert m[lead:].all() and m[:lead, :lead].all() and not m[:lead, lead:].any()
    if period == L - lead and period > 0:  # a lower-triangular mask behind the registers
        assert torch.equal(m[lead:, lead:], torch.ones(period, period).tril().bool())
        assert m[lead:, :lead].all()


def test_masked_attention_is_the_softmax_over_the_allowed_keys():
    g = torch.Generator().manual_seed(1)
    L, hd = 22, 8
    q, k, v = (torch.randn(2, L, hd, generator=g) for _ in range(3))
    mask = FC.allowed(L, 4, 6)
    o, lse = FC.masked_attention(q, k, v, mask)
    for b in range(2):
        for i in range(L):
            keys = [j for j in range(L) if mask[i, j]]
            s = (k[b, keys] @ q[b, i]) / hd ** 0.5
            assert torch.allclose(o[b, i], torch.softmax(s, 0) @ v[b, keys], atol=1e-5)
            assert torch.allclose(lse[b, i], torch.logsumexp(s, 0), atol=1e-5)


def fcmap_x(l, lead, period):
    """host mirror of FcMap::x in csrc/attention.hip: (l - lead) - trunc(fma(float(l - lead), fl(1 / period), 0.5 *
    fl(1 / period))) * period.  The fma's exact argument inv * (2 kk + 1) / 2 has at most 22 + 24 significant bits, so
    float64 holds it exactly and ONE rounding to float32 reproduces the device's fused result."""
    import numpy as np
    kk = np.asarray(l, dtype=np.int64) - lead
    inv = np.float32(1.0) / np.float32(period)
    v = (np.float64(inv) * (kk.astype(np.float64) + 0.5)).astype(np.float32)
    return kk - np.trunc(v).astype(np.int64) * period


@pytest.mark.parametrize("period", [1, 2, 3, 5, 7, 8, 24, 127, 1000, 4099, 65537, 699051, (1 << 21) - 17])
def test_division_free_group_map_up_to_its_limit(period):
    """the fp32 quotient of the kernels' row-group map is exact for every row below 2^21 -- around every multiple of the
    period near the limit, at random rows, and for the lead rows (negative l - lead, which must land in [-period, -1])"""
    import numpy as np
    top = 1 << 21
    rng = np.random.default_rng(period)
    for lead in (0, 16, 5):
        mult = np.arange(max(0, top // period - 4000), top // period + 1, dtype=np.int64) * period + lead
        near = np.concatenate([mult - 1, mult, mult + 1, np.arange(top - 5000, top), np.arange(0, 5000),
                               rng.integers(0, top, 20000)])
        near = near[(near >= lead) & (near < top)]
        assert np.array_equal(fcmap_x(near, lead, period), (near - lead) % period), (lead, period)
        regs = np.arange(0, lead)
        if lead:
            x = fcmap_x(regs, lead, period)
            assert (x <= -1).all() and (x >= -period).all(), (lead, period)
    # worst case for the lead rows: a lead as long as the limit allows
    lead = top - 1
    x = fcmap_x(np.concatenate([np.arange(0, 3000), rng.integers(0, lead, 20000)]), lead, period)
    assert (x <= -1).all() and (x >= -period).all()


def test_sequences_past_the_limit_are_refused():
    """L > 2^21 rows: VDS_ERR_UNSUPPORTED from both entry points, before anything is launched (the pointers are never read)"""
    lib = _lib.load()
    a = _lib.AttnArgs()
    a.B, a.H, a.head_dim = 1, 1, 64
    for name in ("q", "k", "v", "o", "d_o", "dq", "dk", "dv"):
        setattr(a, name, 4096)
    a.lse = a.delta = 4096
    for L, want in (((1 << 21) + 8, -2), ((1 << 21) + 9, -1)):  # the second: (L - lead) % period != 0 comes first
        a.Lq = a.Lk = L
        fr = C.byref(_lib.ModGroups(0, 8))
        assert lib.vds_attn_fwd_causal(C.byref(a), fr, None) == want
        assert lib.vds_attn_bwd_causal(C.byref(a), fr, None) == want


# ------------------------------------------------------------------------------------ validation ----
def test_ops_argument_validation():
    q = torch.zeros(1, 2, 40, 64, dtype=bf16)
    k48 = torch.zeros(1, 2, 48, 64, dtype=bf16)
    o, lse = torch.zeros_like(q), torch.zeros(1, 2, 40)
    with pytest.raises(ValueError, match="self-attention"):
        ops.attn_fwd(q, k48, k48, o, lse, frames=(16, 8))
    with pytest.raises(ValueError, match="self-attention"):
        ops.attn_bwd(q, k48, k48, o, lse, q, q, k48, k48, frames=(16, 8))
    for bad in ((-1, 3), (16, 0), (16, 5), (41, 1)):
        with pytest.raises(ValueError, match="period"):
            ops.attn_fwd(q, q, q, o, lse, frames=bad)
        with pytest.raises(ValueError, match="period"):
            ops.attn_bwd(q, q, q, o, lse, q, q, q, q, frames=bad)
    lens = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="kv_lens"):
        ops.attn_fwd(q, q, q, o, lse, frames=(16, 8), kv_lens=lens)
    with pytest.raises(ValueError, match="kv_lens"):
        ops.attn_bwd(q, q, q, o, lse, q, q, q, q, frames=(16, 8), kv_lens=lens)


def tiny(**kw):
    return M.DiT(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=144, depth=2, num_heads=2,
                 cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False, **kw)


def test_model_keyword_adds_no_parameter():
    plain, causal = tiny(), tiny(frame_causal=True)
    assert causal.frame_causal and not plain.frame_causal
    assert all(b.frame_causal for b in causal.blocks) and not any(b.frame_causal for b in plain.blocks)
    assert [(n, tuple(p.shape)) for n, p in plain.named_parameters()] == [(n, tuple(p.shape)) for n, p in causal.named_parameters()]
    causal.load_state_dict(plain.state_dict(), strict=True)
    blk = M.DiTBlock(144, 64, 2, frame_causal=True)
    assert blk._check_frames((16, 8), 48) == (16, 8)
    with pytest.raises(ValueError, match="frames"):
        blk._check_frames(None, 48)
    with pytest.raises(ValueError, match="period"):
        blk._check_frames((16, 5), 48)
    with pytest.raises(ValueError, match="frame_causal"):
        M.DiTBlock(144, 64, 2)._check_frames((16, 8), 48)
    assert M.DiTBlock(144, 64, 2)._check_frames(None, 48) is None


def test_fp8_attention_is_refused():
    m = tiny(frame_causal=True)
    with pytest.raises(NotImplementedError, match=r"enable_fp8\(attention=False\)"):
        m.enable_fp8()
    assert not m.fp8
    m.enable_fp8(attention=False)  # fp8 linears, bf16 masked attention
    assert m.fp8 and m.fp8_attn == 0
    tiny().enable_fp8()  # a plain model is not affected


def test_rollout_frames_is_validated_before_any_model_call():
    from video_diffusion_speedrun_amd import sampling

    class NoCall:
        time_patch_size = 2

        def __call__(self, *a, **k):
            raise AssertionError("the model must not be called")
    lat = torch.zeros(1, 16, 4, 8, 8, dtype=bf16)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="rollout_frames"):
            sampling.generate_latents(NoCall(), torch.zeros(1, 4, 64), latents=lat, rollout_frames=bad, device="cpu")


# ------------------------------------------------------------------------------------------- ABI ----
def test_abi_declares_the_two_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vds.h")).read(), flags=re.S)
    for name in ("vds_attn_fwd_causal", "vds_attn_bwd_causal"):
        assert re.search(rf"\bint\s+{name}\s*\(\s*const\s+vds_attn_args\s*\*[^,]*,\s*const\s+vds_mod_groups\s*\*[^,]*,"
                         rf"\s*vds_stream_t", src), name
        assert _lib.SIGNATURES[name] == [C.POINTER(_lib.AttnArgs), C.c_void_p, C.c_void_p]
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "vds_attn_fwd_causal") and hasattr(raw, "vds_attn_bwd_causal")
    # host-side checks, nothing is launched: null arguments, then a bad description on otherwise empty arguments
    a = _lib.AttnArgs()
    fr = C.byref(_lib.ModGroups(16, 8))
    assert lib.vds_attn_fwd_causal(None, fr, None) == -1 and lib.vds_attn_bwd_causal(None, fr, None) == -1
    assert lib.vds_attn_fwd_causal(C.byref(a), fr, None) == -1 and lib.vds_attn_bwd_causal(C.byref(a), fr, None) == -1
    assert lib.vds_attn_fwd_causal(C.byref(a), None, None) == -1  # NULL frames: vds_attn_fwd's own refusal


# ---------------------------------------------------------------------------- reference model ----
def model_case(name):
    """the tiny configurations and inputs of tests/test_frame_timesteps_gpu.py (t = 3 token-frames, L = 64)"""
    if name == "hd72":
        cfg = O.DiTConfig(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=144, depth=2, num_heads=2,
                          cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False)
        seed = 3
    else:
        cfg = O.DiTConfig(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=128, depth=3, num_heads=2,
                          cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False)
        seed = 13
    P = O.init_params(cfg, seed=seed, randomize_zero_init=True, init_std_factor=1.0)
    P["time_embed.0.weight"] = P["time_embed.0.weight"] * 8
    P["time_embed.2.weight"] = P["time_embed.2.weight"] * 8
    g = torch.Generator().manual_seed(seed + 1)
    latent = torch.randn(2, 16, 6, 8, 8, generator=g).to(bf16)
    ctx = torch.randn(2, 24, 64, generator=g).to(bf16)
    return cfg, P, latent, ctx


TS = [[0.0, 0.5, 0.96875], [0.9375, 0.25, 0.0625]]
START = (2, 3, 4)


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_reference_model_is_causal_over_frames(name):
    """other latents in the last token-frame leave the output of the earlier frames exactly as it was -- and move it by
    5-20 % without the mask"""
    cfg, P, latent, ctx = model_case(name)
    ts = torch.tensor(TS).to(bf16).float()
    other = latent.float().clone()
    other[:, :, 4:] = (latent[:, :, 4:].float() + 3.0).to(bf16).float()
    with torch.no_grad():
        moved = {}
        for causal in (True, False):
            a = FC.dit_forward(P, cfg, latent.float(), ctx.float(), ts, START, frame_causal=causal)
            b = FC.dit_forward(P, cfg, other, ctx.float(), ts, START, frame_causal=causal)
            moved[causal] = rel(b[:, :, :4], a[:, :, :4])
            assert rel(b[:, :, 4:], a[:, :, 4:]) > 0.1
        # frame_causal=False is the per-frame helper model itself
        assert torch.equal(FC.dit_forward(P, cfg, latent.float(), ctx.float(), ts, START, frame_causal=False),
                           FC.R.dit_forward(P, cfg, latent.float(), ctx.float(), ts, START))
    print(f"{name}: earlier frames move by {moved[True]} with the mask, {moved[False]:.3f} without")
    assert moved[True] == 0.0
    # measured 0.171 (hd72) / 0.187 (hd64) with this perturbation (+3.0 on the last token-frame); other latents drawn
    # N(0, 1) there move hd64 by 0.10 only, too close to the 4 x 2.5e-2 the device test asks for
    assert moved[False] > 0.15
