"""QK-norm, the parts that need no GPU: the constructor keyword and what it leaves alone (parameters, state-dict keys,
optimizer groups, the activation accounting), the refusal of the fp8 attention producers, the two C entry points and their
host-side argument checks, and the float64 reference of the GPU tests against autograd."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from oracle import dit_oracle as O
from video_diffusion_speedrun_amd import _lib
from video_diffusion_speedrun_amd import model as M
from video_diffusion_speedrun_amd.model import DiT, DiTBlock

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import qk_norm_ref as R  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64, bf16 = torch.float64, torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _smoke_model(**kw):
    return DiT(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=144, depth=2, num_heads=2,
               cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False, **kw)


def test_keyword_defaults_to_off_and_comes_last():
    import inspect
    assert list(inspect.signature(DiT.__init__).parameters)[-1] == "qk_norm"
    assert list(inspect.signature(DiTBlock.__init__).parameters)[-1] == "qk_norm"
    assert inspect.signature(DiT.__init__).parameters["qk_norm"].default is False
    assert inspect.signature(DiTBlock.__init__).parameters["qk_norm"].default is False
    m = _smoke_model()
    assert m.qk_norm is False and not any(b.qk_norm for b in m.blocks)
    n = _smoke_model(qk_norm=True)
    assert n.qk_norm is True and all(b.qk_norm for b in n.blocks)
    assert DiTBlock(128, 32, 2).qk_norm is False and DiTBlock(128, 32, 2, qk_norm=True).qk_norm is True


def test_the_flag_adds_no_parameter_and_no_group():
    m, n = _smoke_model(), _smoke_model(qk_norm=True)
    assert list(m.state_dict().keys()) == list(n.state_dict().keys())
    assert [(k, tuple(p.shape)) for k, p in m.named_parameters()] == [(k, tuple(p.shape)) for k, p in n.named_parameters()]
    n.load_state_dict(m.state_dict(), strict=True)  # a checkpoint of either loads into the other
    const = ["patch_proj", "context_kv", "positional_embedding"]
    gm, gn = m.get_mup_setup(1e-3, 0.1, const)[0], n.get_mup_setup(1e-3, 0.1, const)[0]
    assert [len(g["params"]) for g in gm] == [len(g["params"]) for g in gn]
    assert [{k: v for k, v in g.items() if k != "params"} for g in gm] == \
           [{k: v for k, v in g.items() if k != "params"} for g in gn]
    um, un = m.get_muon_setup(1e-3, 0.1, const), n.get_muon_setup(1e-3, 0.1, const)
    shape_of = lambda groups: [[tuple(p.shape) for p in g["params"]] for g in groups]
    assert shape_of(um[0]) == shape_of(un[0])


def test_activation_bytes_already_counts_the_qkv_rows_the_backward_reads():
    """The normed backward reads the qkv GEMM output in EVERY block.  DiTBlock._fwd keeps that tensor in every block as it
    is (block 0, which mixes no v_0 and whose plain RoPE backward does not read it, included), and activation_bytes
    counts it per block: 3 D bf16 elements = 3 D * 2 bytes per token row.  So the flag changes no figure."""
    for mode in M.RECOMPUTE_MODES:
        a = M.activation_bytes(_smoke_model(), 2, (4, 8, 8), 24, mode)
        b = M.activation_bytes(_smoke_model(qk_norm=True), 2, (4, 8, 8), 24, mode)
        assert a == b, (mode, a, b)
    m = _smoke_model(qk_norm=True)
    a = M.activation_bytes(m, 2, (4, 8, 8), 24, "none")
    D, H, hd, hdp, rows = 144, 2, 72, 96, a["rows"]
    L = rows // 2
    assert rows == 2 * (2 * 4 * 4 + M.N_REG)
    # the per-block sum, written out: the qkv term is the 3 * rows * D below
    bf16_elems = (3 * rows * D + rows * D + 3 * rows * D + 3 * 2 * H * L * hdp + rows * D + rows * D + 4 * rows * D
                  + rows * D + 2 * rows * 4 * D + rows * D + 2 * 24 * 2 * D)
    f32_elems = 3 * rows + 2 * 2 * H * L + 2 * 9 * D
    assert a["per_block"] == 2 * bf16_elems + 4 * f32_elems
    assert a["kept"] == m.depth * a["per_block"]  # block 0 keeps what block 1 keeps: 3 D * 2 bytes per row for qkv too


def test_fp8_attention_is_refused_and_names_the_way_out():
    m = _smoke_model(qk_norm=True)
    with pytest.raises(NotImplementedError, match=r"enable_fp8\(attention=False\)"):
        m.enable_fp8()
    with pytest.raises(NotImplementedError, match=r"enable_fp8\(attention=False\)"):
        m.enable_fp8(cross_attention=False)  # still fp8 self-attention
    assert m.fp8 is False and m.fp8_attn == 0  # a refused call changes nothing
    assert m.enable_fp8(attention=False) is m and m.fp8 and m.fp8_attn == 0 and m.fp8_lin
    assert m.enable_fp8(False) is m and not m.fp8
    assert _smoke_model().enable_fp8().fp8_attn == 2  # the model without the flag: as before
    # recompute and the flag combine freely
    assert _smoke_model(qk_norm=True).enable_recompute("selective").recompute == "selective"


PTR = r"(?:const\s+)?(?:void|float)\s*\*\s*\w+"
I32 = r"int32_t\s+\w+"


def test_symbols_are_declared_bound_and_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vds.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    sep = r"\s*,\s*"
    fwd = sep.join([PTR] * 8 + [I32] * 5 + [r"float\s+eps", r"vds_stream_t\s+\w+"])
    bwd = sep.join([PTR] * 11 + [I32] * 7 + [r"float\s+eps", r"vds_stream_t\s+\w+"])
    for name, args, n in (("vds_qkv_rope_norm_fwd", fwd, 15), ("vds_qkv_rope_norm_bwd", bwd, 20)):
        assert re.search(rf"\bint\s+{name}\s*\(\s*{args}\s*\)\s*;", src), f"{name} is not declared in include/vds.h"
        assert len(_lib.SIGNATURES[name]) == n and _lib.SIGNATURES[name][-2] is C.c_float
        assert hasattr(raw, name), name
    # the plain entry points keep their signatures
    assert len(_lib.SIGNATURES["vds_qkv_rope_fwd"]) == 14 and len(_lib.SIGNATURES["vds_qkv_rope_bwd"]) == 19


def test_host_side_argument_checks(lib):
    """every call below is refused before a launch: the pointers are never dereferenced"""
    P = 0x1000  # a non-null "pointer"
    f, b = lib.vds_qkv_rope_norm_fwd, lib.vds_qkv_rope_norm_bwd
    assert f(None, None, None, None, None, None, None, None, 1, 8, 1, 72, 96, 1e-6, None) == -1      # null operands
    assert f(P, P, P, None, None, P, P, P, 1, 8, 1, 72, 96, 0.0, None) == -1                         # eps must be > 0
    assert f(P, P, P, None, None, P, P, P, 1, 8, 1, 72, 96, -1e-6, None) == -1
    assert f(P, P, P, None, None, P, P, P, 1, 8, 1, 72, 96, float("nan"), None) == -1
    assert f(P, P, P, None, None, P, P, P, 1, 8, 1, 70, 96, 1e-6, None) == -1                        # hd % 8, as the plain call
    assert f(P, P, P, P, None, P, P, P, 1, 8, 1, 72, 96, 1e-6, None) == -1                           # v0 without lam
    assert f(P, P, P, None, None, P, P, P, 1, 8, 1, 72, 64, 1e-6, None) == -1                        # hdp < hd
    assert lib.vds_qkv_rope_fwd(P, P, P, P, None, P, P, P, 1, 8, 1, 72, 96, None) == -1              # (the plain call agrees)
    assert b(None, None, None, None, None, None, None, None, None, None, None, 0, 0, 1, 8, 1, 72, 96, 1e-6, None) == -1
    assert b(P, P, P, P, P, None, None, None, None, None, P, 0, 0, 1, 8, 1, 72, 96, 1e-6, None) == -1  # qkv_raw, even with mix = 0
    assert b(P, P, P, P, P, P, None, None, None, None, P, 0, 0, 1, 8, 1, 72, 96, 0.0, None) == -1      # eps
    assert b(P, P, P, P, P, P, None, None, None, None, P, 1, 0, 1, 8, 1, 72, 96, 1e-6, None) == -1     # mix without v0 / lam / dlam
    assert b(P, P, P, P, P, P, P, P, P, P, P, 3, 0, 1, 8, 1, 72, 96, 1e-6, None) == -1                 # mix out of range
    assert b(P, P, P, P, P, P, None, None, None, None, P, 0, 1, 1, 8, 1, 72, 96, 1e-6, None) == -1     # add_dv0 without dv0_acc
    assert b(P, P, P, P, P, P, None, None, None, None, P, 0, 0, 1, 8, 1, 70, 96, 1e-6, None) == -1     # hd % 8


# ------------------------------------------------------------------- the float64 reference itself ----
def _f64_composition(x, cos, sin, eps=R.EPS):
    """rms_norm (no weight) followed by the half-split rotation, in float64 with autograd -- oracle.rms_norm and
    oracle.apply_rotary written out, because those two compute in fp32 whatever they are given"""
    xn = x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + eps)
    d = x.shape[-1] // 2
    x1, x2 = xn[..., :d], xn[..., d:]
    return torch.cat([x1 * cos + x2 * sin, x2 * cos - x1 * sin], dim=-1)


@pytest.mark.parametrize("hd,hdp,H,L", [(72, 96, 2, 7), (64, 64, 3, 5), (24, 24, 1, 4)])
def test_float64_reference_against_autograd(hd, hdp, H, L):
    B, D = 2, H * hd
    g = torch.Generator().manual_seed(hd + L)
    qkv = torch.randn(B * L, 3 * D, generator=g).to(bf16)
    qkv[1, hd:2 * hd] = 0  # a zero head row of q (token 1, head 1 -- head 0 when H = 1)
    if H == 1:
        qkv[1, :hd] = 0
    ang = torch.rand(L, hd // 2, generator=g) * 6.28
    cos, sin = torch.cos(ang).float(), torch.sin(ang).float()
    dq = torch.randn(B, H, L, hdp, generator=g).to(bf16)
    dk = torch.randn(B, H, L, hdp, generator=g).to(bf16)
    fwd = R.forward_ref(qkv, cos, sin, B, L, H, hd)
    bwd = R.backward_ref(dq, dk, qkv, cos, sin, B, L, H, hd)
    for section, grad in ((0, dq), (1, dk)):
        x = R._heads(qkv, B, L, H, hd, section).to(f64).clone().requires_grad_(True)
        y = _f64_composition(x, cos.to(f64), sin.to(f64))
        ref, partners = fwd[section]
        # forward: the reference rounds the normalised rows to bf16 (half an ulp of 8 significant bits: at most 2^-8
        # relative, on each of the two partners; |cos|, |sin| <= 1)
        assert torch.all((ref - y.detach()).abs() <= 2.0 ** -8 * partners + 1e-12)
        assert torch.all(partners >= 0) and partners.shape == ref.shape
        y.backward(grad[..., :hd].to(f64))
        dref, scale, xraw = bwd[section]
        assert torch.equal(xraw, x.detach())
        assert torch.all((dref - x.grad).abs() <= 1e-12 * scale + 1e-300), (dref - x.grad).abs().max()
        assert torch.all(dref.abs() <= scale * (1 + 1e-12))
        # the norm's Jacobian removes the radial component (up to eps: r^2 mean(x^2) = 1 - eps r^2)
        radial = (dref * xraw).sum(-1).abs()
        assert torch.all(radial <= 2e-5 * (dref * xraw).abs().sum(-1) + 1e-12)
        assert torch.isfinite(dref).all() and torch.isfinite(ref).all()
    # the zero row: output 0, gradient r * g with r = eps^-1/2 = 1000
    h0 = 0 if H == 1 else 1
    assert torch.equal(fwd[0][0][0, h0, 1], torch.zeros(hd, dtype=f64))
    g0 = R._rotate(dq[0, h0, 1, :hd].to(f64), cos[1].to(f64), sin[1].to(f64), inverse=True)
    assert torch.allclose(bwd[0][0][0, h0, 1], 1000.0 * g0, rtol=1e-12, atol=0)
    # and the fp32 oracle pair the model tests wrap agrees with the float64 forward up to fp32 / bf16 rounding
    with R.qk_normed_oracle():
        got = O.apply_rotary(R._heads(qkv, B, L, H, hd, 0), cos, sin)  # bf16 in: rms_norm rounds to bf16, as the kernels do
    assert torch.all((got.to(f64) - fwd[0][0]).abs() <= 2.0 ** -8 * fwd[0][1] + 2.0 ** -8 * fwd[0][0].abs() + 1e-6)


def test_the_wrapper_restores_the_oracle():
    orig = O.apply_rotary
    x = torch.randn(1, 1, 3, 8)
    ang = torch.rand(3, 4)
    cos, sin = torch.cos(ang), torch.sin(ang)
    plain = O.apply_rotary(x, cos, sin)
    with R.qk_normed_oracle():
        assert O.apply_rotary is not orig
        assert torch.allclose(O.apply_rotary(x, cos, sin), orig(O.rms_norm(x), cos, sin))
        assert not torch.allclose(O.apply_rotary(x, cos, sin), plain)
    assert O.apply_rotary is orig
    with pytest.raises(RuntimeError):
        with R.qk_normed_oracle():
            raise RuntimeError("boom")
    assert O.apply_rotary is orig
