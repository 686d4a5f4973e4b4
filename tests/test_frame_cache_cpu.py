"""Frame KV cache without a GPU: the past mask against a literal double loop over its definition, the helper's cached chunk
call against the helper's full-sequence masked model (the layout, the RoPE rows and the register-level argument, before any
kernel), the weight of the past in the chunk's output, argument validation in ops, the model and the sampler, and the C
symbols."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from video_diffusion_speedrun_amd import _lib, model as M, ops, sampling

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_cache_ref as KC  # noqa: E402

FC, R = KC.FC, KC.R
bf16, f32 = torch.bfloat16, torch.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_OUT = 2.5e-2  # the project's bound for one model call (tests/test_frame_causal_gpu.py)


def rel(a, b):
    a, b = a.float().flatten(), b.float().flatten()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


# ------------------------------------------------------------------------------------------ mask ----
@pytest.mark.parametrize("past", [0, 1, 23, 64])
@pytest.mark.parametrize("period", [1, 2, 3])
@pytest.mark.parametrize("lead", [0, 16])
def test_past_mask_against_a_double_loop(lead, period, past):
    Lq = lead + 4 * period
    got = KC.past_allowed(Lq, lead, period, past)
    assert got.dtype == torch.bool and tuple(got.shape) == (Lq, Lq + past)
    x = lambda l: (l - lead) % period  # token-frame of a token row
    for i in range(Lq):
        for j in range(Lq + past):
            if j < lead:
                want = True  # register keys: everyone
            elif i < lead:
                want = False  # a register query: the register keys only
            elif j < lead + past:
                want = True  # a token query: every past key
            else:
                want = x(j - past) <= x(i)
            assert bool(got[i, j]) == want, (i, j)
    if past == 0:
        assert torch.equal(got, FC.allowed(Lq, lead, period))
    assert got[:, 0].all() or lead == 0 and past == 0 and not got.numel()  # key 0: no empty row
    # the kernels' form: one compare xk <= fq with xk = -1 | 0 | x(j - past) and fq = max(x(i), -1), x(i) < 0 on lead rows
    xk = torch.tensor([-1 if j < lead else 0 if j < lead + past else x(j - past) for j in range(Lq + past)])
    fq = torch.tensor([-1 if i < lead else x(i) for i in range(Lq)])
    assert torch.equal(got, xk[None, :] <= fq[:, None])


# ---------------------------------------------------------------------------- reference model ----
def full_reference(name, f0, k):
    """the helper's full-sequence masked model with the register level pinned, earlier frames at 0, later frames at 1"""
    cfg, P, latent, ctx = KC.model_case(name)
    ts = torch.ones(2, 3)
    ts[:, :f0] = 0
    ts[:, f0:f0 + k] = torch.tensor(KC.T_CHUNK)[:, :k].to(bf16).float()
    with torch.no_grad():
        return KC.full_forward(P, cfg, latent.float(), ctx.float(), ts, KC.BASE, torch.tensor(KC.REG))


@pytest.mark.parametrize("f0,k", KC.CHUNKS, ids=[f"f{f}_k{k}" for f, k in KC.CHUNKS])
@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_cached_chunk_is_the_full_sequence_model_on_the_chunks_frames(name, f0, k):
    cfg, P, latent, ctx = KC.model_case(name)
    pt = cfg.time_patch_size
    out, cache = KC.chunk_reference(name, f0, k)
    assert cache.past_frames == f0 and tuple(out.shape) == (2, 16, k * pt, 8, 8)
    full = full_reference(name, f0, k)[:, :, f0 * pt:(f0 + k) * pt]
    e = rel(out, full)
    print(f"{name} frames {f0}..{f0 + k - 1}: cached vs full-sequence {e:.2e}")
    assert e <= 1e-5, e


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_the_pinned_register_level_makes_the_model_causal_in_the_noise_levels(name):
    """the full-sequence helper with the register level pinned: other noise levels on the LAST frame leave the earlier
    frames' output exactly as it was; with the row maximum (FC.dit_forward) they move it"""
    cfg, P, latent, ctx = KC.model_case(name)
    a, b = torch.tensor([[0.0, 0.5, 0.25], [0.0, 0.25, 0.5]]), torch.tensor([[0.0, 0.5, 0.96875], [0.0, 0.25, 1.0]])
    reg = torch.tensor(KC.REG)
    with torch.no_grad():
        pa, pb = (KC.full_forward(P, cfg, latent.float(), ctx.float(), t, KC.BASE, reg) for t in (a, b))
        ma, mb = (FC.dit_forward(P, cfg, latent.float(), ctx.float(), t, KC.BASE) for t in (a, b))
    assert rel(pb[:, :, :4], pa[:, :, :4]) == 0.0
    assert rel(mb[:, :, :4], ma[:, :, :4]) > 1e-3
    # pinned to the row maximum it is FC.dit_forward
    assert torch.equal(KC.full_forward(P, cfg, latent.float(), ctx.float(), a, KC.BASE, a.max(dim=1).values), ma)


@pytest.mark.parametrize("f0,k", [(1, 1), (2, 1), (1, 2)], ids=["f1_k1", "f2_k1", "f1_k2"])
@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_dropping_the_past_moves_the_chunk(name, f0, k):
    """the GPU comparison cannot pass with the past ignored: the chunk's output is > 4 x B_OUT away without it"""
    out, _ = KC.chunk_reference(name, f0, k)
    nopast, _ = KC.chunk_reference(name, f0, k, use_past=False)
    d = rel(nopast, out)
    print(f"{name} frames {f0}..{f0 + k - 1}: without the past {d:.3f}")
    assert d > 4 * B_OUT, d


# ------------------------------------------------------------------------------------ validation ----
def tiny(**kw):
    return M.DiT(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=144, depth=2, num_heads=2,
                 cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False, **kw)


def test_ops_argument_validation():
    q = torch.zeros(1, 2, 40, 64, dtype=bf16)
    k63 = torch.zeros(1, 2, 63, 64, dtype=bf16)
    k64 = torch.zeros(1, 2, 64, 64, dtype=bf16)
    o, lse = torch.zeros_like(q), torch.zeros(1, 2, 40)
    with pytest.raises(ValueError, match="past"):
        ops.attn_fwd(q, k63, k63, o, lse, frames=(16, 8), past=24)  # Lk != Lq + past
    with pytest.raises(ValueError, match="past"):
        ops.attn_fwd(q, k64, k64, o, lse, past=24)  # no frames
    with pytest.raises(ValueError, match="past"):
        ops.attn_fwd(q, q, q, o, lse, frames=(16, 8), past=-1)
    with pytest.raises(ValueError, match="period"):
        ops.attn_fwd(q, k64, k64, o, lse, frames=(16, 5), past=24)
    with pytest.raises(ValueError, match="kv_lens"):
        ops.attn_fwd(q, k64, k64, o, lse, frames=(16, 8), past=24, kv_lens=torch.zeros(1, dtype=torch.int32))
    qkv = torch.zeros(40, 3 * 128, dtype=bf16)
    cs = torch.zeros(40, 32)
    kb, vb = torch.zeros(1, 2, 64, 64, dtype=bf16), torch.zeros(1, 2, 64, 64, dtype=bf16)
    with pytest.raises(ValueError, match="kv cache"):
        ops.qkv_rope_fwd_cache(qkv, cs, cs, None, None, kb, vb, 16, 25, 1, 40, 2, 64, 64)  # 40 + 25 rows > 64
    with pytest.raises(ValueError, match="kv cache"):
        ops.qkv_rope_norm_fwd_cache(qkv, cs, cs, None, None, kb, vb[:, :, :, :32], 16, 24, 1, 40, 2, 64, 64)
    with pytest.raises(ValueError, match="kv cache"):
        ops.qkv_rope_fwd_cache(qkv, cs, cs, None, None, kb, vb, 41, 24, 1, 40, 2, 64, 64)  # lead > L


def test_register_timesteps_validation():
    m = tiny(frame_causal=True)
    x, ctx = torch.zeros(2, 16, 6, 8, 8), torch.zeros(2, 24, 64)
    with pytest.raises(ValueError, match="register_timesteps"):
        m(x, ctx, torch.zeros(2), register_timesteps=[1.0, 1.0])  # [B] timesteps
    with pytest.raises(ValueError, match="register_timesteps"):
        m(x, ctx, torch.zeros(2, 3), register_timesteps=[1.0])
    with pytest.raises(ValueError, match="register_timesteps"):
        m(x, ctx, torch.zeros(2, 3), register_timesteps=torch.ones(2, 3))
    with pytest.raises(RuntimeError, match="GPU only"):  # valid arguments: the call gets as far as the device check
        m(x, ctx, torch.zeros(2, 3), register_timesteps=torch.ones(2))


def test_frame_cache_validation():
    m = tiny(frame_causal=True)
    with pytest.raises(ValueError, match="frame_causal=True"):
        tiny().new_frame_cache(2, 3, 4, 4)
    with pytest.raises(ValueError, match=">= 1"):
        m.new_frame_cache(2, 0, 4, 4)
    cache = m.new_frame_cache(2, 3, 4, 4, device="cpu")
    assert isinstance(cache, M.FrameKVCache) and cache.past_frames == 0
    assert len(cache.k) == len(cache.v) == 2
    assert all(tuple(t.shape) == (2, 2, 16 + 3 * 16, 96) and t.dtype == bf16 for t in cache.k + cache.v)
    with pytest.raises(RuntimeError, match="commit"):
        cache.commit()
    x1, ctx = torch.zeros(2, 16, 2, 8, 8), torch.zeros(2, 24, 64)
    ok = dict(rope_start=(2, 3, 4), frame_cache=cache)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="GPU only"):  # valid arguments: as far as the device check
            m(x1, ctx, torch.zeros(2, 1), **ok)
        with pytest.raises(ValueError, match="new_frame_cache"):
            m(x1, ctx, torch.zeros(2, 1), rope_start=(2, 3, 4), frame_cache=object())
        with pytest.raises(ValueError, match="frame_causal=True"):
            tiny()(x1, ctx, torch.zeros(2, 1), **ok)
        with pytest.raises(ValueError, match=r"\[2, 1\]"):
            m(x1, ctx, torch.zeros(2), **ok)  # [B] timesteps
        with pytest.raises(ValueError, match="new_frame_cache"):
            m(x1[:1], ctx[:1], torch.zeros(1, 1), **ok)  # batch
        with pytest.raises(ValueError, match="new_frame_cache"):
            m(torch.zeros(2, 16, 2, 8, 4), ctx, torch.zeros(2, 1), **ok)  # w
        with pytest.raises(ValueError, match="larger cache"):
            m(torch.zeros(2, 16, 8, 8, 8), ctx, torch.zeros(2, 4), **ok)  # 4 frames into a cache of 3
        with pytest.raises(ValueError, match="rope_start"):
            m(x1, ctx, torch.zeros(2, 1), frame_cache=cache)
        with pytest.raises(ValueError, match="rope_start"):
            m(x1, ctx, torch.zeros(2, 1), rope_start=(126, 3, 4), frame_cache=cache)  # 126 + 3 frames > 128 positions
        cache.past_frames = 2
        with pytest.raises(ValueError, match="larger cache"):
            m(torch.zeros(2, 16, 4, 8, 8), ctx, torch.zeros(2, 2), rope_start=(4, 3, 4), frame_cache=cache)
        with pytest.raises(ValueError, match="rope_start"):
            m(x1, ctx, torch.zeros(2, 1), rope_start=(1, 3, 4), frame_cache=cache)  # base 1 - 2 < 0
        cache.reset()
        assert cache.past_frames == 0
        f8 = tiny(frame_causal=True).enable_fp8(attention=False)
        with pytest.raises(NotImplementedError, match=r"enable_fp8\(False\)"):
            f8(x1, ctx, torch.zeros(2, 1), rope_start=(2, 3, 4), frame_cache=f8.new_frame_cache(2, 3, 4, 4, device="cpu"))
        sharded = tiny(frame_causal=True)
        sharded._fsdp = object()
        with pytest.raises(NotImplementedError, match="apply_fsdp"):
            sharded(x1, ctx, torch.zeros(2, 1), **ok)
    with pytest.raises(RuntimeError, match="no_grad"):
        m(x1, ctx, torch.zeros(2, 1), **ok)


def test_fp8_attention_with_a_cache_names_the_remedy():
    """a frame_causal model refuses fp8 attention at enable_fp8 already; forced on, the cached call refuses it too"""
    m = tiny(frame_causal=True)
    with pytest.raises(NotImplementedError, match=r"enable_fp8\(attention=False\)"):
        m.enable_fp8()
    m.fp8, m.fp8_attn = True, 1
    with torch.no_grad(), pytest.raises(NotImplementedError, match=r"enable_fp8\(attention=False\)"):
        m(torch.zeros(2, 16, 2, 8, 8), torch.zeros(2, 24, 64), torch.zeros(2, 1), rope_start=(2, 3, 4),
          frame_cache=m.new_frame_cache(2, 3, 4, 4, device="cpu"))


def test_sampler_validation_before_any_model_call():
    class NoCall:
        time_patch_size = 2
        frame_causal = True

        def __call__(self, *a, **k):
            raise AssertionError("the model must not be called")

    class Plain(NoCall):
        frame_causal = False
    lat = torch.zeros(1, 16, 4, 8, 8, dtype=bf16)
    kw = dict(latents=lat, device="cpu")
    with pytest.raises(ValueError, match="rollout_frames"):
        sampling.generate_latents(NoCall(), torch.zeros(1, 4, 64), kv_cache=True, **kw)
    with pytest.raises(ValueError, match="frame_causal=True"):
        sampling.generate_latents(Plain(), torch.zeros(1, 4, 64), kv_cache=True, rollout_frames=1, **kw)
    for bad in ([], [(1, 2, 3)] * 2):
        with pytest.raises(ValueError, match="rope_starts"):
            sampling.generate_latents(NoCall(), torch.zeros(1, 4, 64), kv_cache=True, rollout_frames=1, rope_starts=bad, **kw)


# ------------------------------------------------------------------------------------------- ABI ----
def test_abi_declares_the_new_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vds.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+vds_attn_fwd_causal_past\s*\(\s*const\s+vds_attn_args\s*\*[^,]*,\s*const\s+vds_mod_groups\s*\*"
                     r"[^,]*,\s*int32_t[^,]*,\s*vds_stream_t", src)
    assert _lib.SIGNATURES["vds_attn_fwd_causal_past"] == [C.POINTER(_lib.AttnArgs), C.c_void_p, C.c_int32, C.c_void_p]
    for name, n in (("vds_qkv_rope_fwd_cache", 19), ("vds_qkv_rope_norm_fwd_cache", 20)):
        assert re.search(rf"\bint\s+{name}\s*\(", src), name
        assert len(_lib.SIGNATURES[name]) == n
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("vds_attn_fwd_causal_past", "vds_qkv_rope_fwd_cache", "vds_qkv_rope_norm_fwd_cache"):
        assert hasattr(raw, name), name
    # host-side checks, nothing is launched
    a = _lib.AttnArgs()
    fr = C.byref(_lib.ModGroups(16, 8))
    assert lib.vds_attn_fwd_causal_past(None, fr, 8, None) == -1
    assert lib.vds_attn_fwd_causal_past(C.byref(a), fr, -1, None) == -1
    assert lib.vds_attn_fwd_causal_past(C.byref(a), None, 8, None) == -1  # NULL frames with a past
    assert lib.vds_attn_fwd_causal_past(C.byref(a), None, 0, None) == -1  # past = 0: vds_attn_fwd_causal's own refusal
    assert lib.vds_qkv_rope_fwd_cache(*([None] * 8), 0, 0, 0, 0, 0, 1, 1, 1, 64, 64, None) == -1
    assert lib.vds_qkv_rope_norm_fwd_cache(*([None] * 8), 0, 0, 0, 0, 0, 1, 1, 1, 64, 64, 1e-6, None) == -1
