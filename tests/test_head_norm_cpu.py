"""QK-norm in cross-attention (qk_norm="all"), the parts that need no GPU: the flag's semantics and what it leaves alone
(parameters, state-dict keys, optimizer groups), the activation accounting, the two C entry points and every host-side
refusal, the operand checks of the ops wrappers, the exact-input builder of the kernel tests and the four faults its
bitwise compare has to flag, and the bound on the cross-attention logits of the wrapped oracle."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from oracle import dit_oracle as O
from video_diffusion_speedrun_amd import _lib, ops
from video_diffusion_speedrun_amd import model as M
from video_diffusion_speedrun_amd.model import DiT, DiTBlock

HELPERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers")
sys.path.insert(0, HELPERS)
import head_norm_ref as R  # noqa: E402
from qk_norm_ref import qk_normed_oracle  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16
CONST = ["patch_proj", "context_kv", "positional_embedding"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _model(**kw):
    kw.setdefault("cross_attn_input_size", 64)
    return DiT(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=144, depth=2, num_heads=2, residual_v=True,
               train_bias_and_rms=False, **kw)


# ------------------------------------------------------------------------------------------- the flag ----
def test_all_selects_the_cross_attention_norm_and_nothing_else_does():
    m = _model(qk_norm="all")
    assert m.qk_norm is True and m.qk_norm_cross is True
    assert all(b.qk_norm is True and b.qk_norm_cross is True for b in m.blocks)
    for value in (False, True, 1, "", "ALL", "All", "cross", "all ", ["all"], None):  # every other value: today's bool()
        n = _model(qk_norm=value)
        assert n.qk_norm is bool(value) and n.qk_norm_cross is False, value
        assert all(b.qk_norm is bool(value) and b.qk_norm_cross is False for b in n.blocks), value
    assert _model().qk_norm_cross is False
    # without cross-attention "all" is True
    s = _model(qk_norm="all", cross_attn_input_size=None)
    assert s.qk_norm is True and s.qk_norm_cross is False and not any(b.qk_norm_cross for b in s.blocks)
    b = DiTBlock(128, 32, 2, qk_norm="all")
    assert b.qk_norm is True and b.qk_norm_cross is True
    assert DiTBlock(128, None, 2, qk_norm="all").qk_norm_cross is False
    assert DiTBlock(128, 32, 2, qk_norm=True).qk_norm_cross is False and DiTBlock(128, 32, 2).qk_norm_cross is False


def test_all_adds_no_parameter_and_no_group():
    m, n = _model(qk_norm=True), _model(qk_norm="all")
    assert list(m.state_dict().keys()) == list(n.state_dict().keys())
    assert [(k, tuple(p.shape)) for k, p in m.named_parameters()] == [(k, tuple(p.shape)) for k, p in n.named_parameters()]
    gm, gn = m.get_mup_setup(1e-3, 0.1, CONST)[0], n.get_mup_setup(1e-3, 0.1, CONST)[0]
    assert [len(g["params"]) for g in gm] == [len(g["params"]) for g in gn]
    assert [{k: v for k, v in g.items() if k != "params"} for g in gm] == \
           [{k: v for k, v in g.items() if k != "params"} for g in gn]
    um, un = m.get_muon_setup(1e-3, 0.1, CONST), n.get_muon_setup(1e-3, 0.1, CONST)
    shape_of = lambda groups: [[tuple(p.shape) for p in g["params"]] for g in groups]  # noqa: E731
    assert shape_of(um[0]) == shape_of(un[0])


def test_state_dict_round_trip_between_the_three_settings():
    models = {v: _model(qk_norm=v) for v in (False, True, "all")}
    src = models[False].state_dict()
    for a in models.values():
        for b in models.values():
            b.load_state_dict(a.state_dict(), strict=True)
    for m in models.values():
        got = m.state_dict()
        assert list(got.keys()) == list(src.keys()) and all(torch.equal(got[k], src[k]) for k in src)


def test_fp8_attention_stays_refused_with_the_same_text():
    m = _model(qk_norm="all")
    with pytest.raises(NotImplementedError) as e_all:
        m.enable_fp8()
    with pytest.raises(NotImplementedError) as e_true:
        _model(qk_norm=True).enable_fp8()
    assert str(e_all.value) == str(e_true.value) == M._FP8_QK_NORM
    assert m.enable_fp8(attention=False) is m and m.fp8 and m.fp8_attn == 0 and m.fp8_lin


def test_activation_bytes_counts_the_two_rstd_tensors():
    B, Lc, H = 2, 24, 2
    plain = M.activation_bytes(_model(), B, (4, 8, 8), Lc, "none")
    rows = plain["rows"]
    assert rows == B * (2 * 4 * 4 + M.N_REG)
    for mode in M.RECOMPUTE_MODES:
        off = M.activation_bytes(_model(), B, (4, 8, 8), Lc, mode)
        on = M.activation_bytes(_model(qk_norm=True), B, (4, 8, 8), Lc, mode)
        both = M.activation_bytes(_model(qk_norm="all"), B, (4, 8, 8), Lc, mode)
        assert off == on, mode  # the figures of False and True models do not move
        extra = 4 * H * (rows + B * Lc)  # rstd_qc [B L, H] + rstd_kc [B Lc, H], fp32
        if mode == "none":
            assert both["per_block"] - on["per_block"] == extra and both["kept"] - on["kept"] == 2 * extra
            assert both["transient"] == 0
        else:  # a recomputing model keeps neither; the replayed block holds them
            assert both["per_block"] == on["per_block"] and both["transient"] - on["transient"] == extra
    none = M.activation_bytes(_model(qk_norm="all", cross_attn_input_size=None), B, (4, 8, 8), Lc, "none")
    assert none == M.activation_bytes(_model(cross_attn_input_size=None), B, (4, 8, 8), Lc, "none")


# -------------------------------------------------------------------------------------------- the ABI ----
def test_symbols_are_declared_bound_and_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vds.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    sep = r"\s*,\s*"
    i32, i64 = r"int32_t\s+\w+", r"int64_t\s+\w+"
    fwd = sep.join([r"void\s*\*\s*x", i64, r"float\s*\*\s*rstd", i32, i32, i32, r"float\s+eps", r"vds_stream_t\s+\w+"])
    bwd = sep.join([r"void\s*\*\s*dy", i64, r"const\s+void\s*\*\s*y", i64, r"const\s+float\s*\*\s*rstd", i32, i32, i32,
                    r"vds_stream_t\s+\w+"])
    for name, args in (("vds_head_rmsnorm_fwd", fwd), ("vds_head_rmsnorm_bwd", bwd)):
        assert re.search(rf"\bint\s+{name}\s*\(\s*{args}\s*\)\s*;", src), f"{name} is not declared in include/vds.h"
        assert hasattr(raw, name), name
    c = _lib
    assert c.SIGNATURES["vds_head_rmsnorm_fwd"] == [c.c_vp, c.c_i64, c.c_vp, c.c_i32, c.c_i32, c.c_i32, c.c_f32, c.c_vp]
    assert c.SIGNATURES["vds_head_rmsnorm_bwd"] == [c.c_vp, c.c_i64, c.c_vp, c.c_i64, c.c_vp, c.c_i32, c.c_i32, c.c_i32,
                                                    c.c_vp]
    # no attention entry point was added, and the three kernel files of the parent are not this feature's
    assert not any(n.startswith("vds_attn") and "head" in n for n in c.SIGNATURES)
    mk = open(os.path.join(REPO, "video_diffusion_speedrun_amd", "csrc", "Makefile")).read()
    assert "headnorm.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()


def test_host_side_refusals_launch_nothing(lib):
    """every NULL / non-positive size / bad hd / bad stride / misaligned pointer / bad eps call returns VDS_ERR_ARG and
    leaves its own message.  The calls carry made-up device addresses, so they run in a child process that sees no GPU
    (tests/helpers/head_norm_refusals.py): were a host-side check ever lost, the launch fails there instead of running."""
    script = os.path.join(HELPERS, "head_norm_refusals.py")
    import head_norm_refusals
    env = dict(os.environ, **head_norm_refusals.HIDE)
    r = subprocess.run([sys.executable, script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout
    assert "38 refusals checked, 0 wrong" in r.stdout, r.stdout  # 22 + 16 defects


def test_wrappers_refuse_operands_the_kernel_would_misread():
    """ops.head_rmsnorm_*: a wrong dtype, shape or stride raises ValueError before anything is handed to the library (CPU
    tensors here: a well-formed call would go on to the GPU-only assertion, which is not reached)"""
    z = lambda *s, dt=bf16: torch.zeros(*s, dtype=dt)  # noqa: E731
    H, hd = 2, 72
    x, wide = z(4, 144), z(4, 288)
    for bad in (lambda: ops.head_rmsnorm_fwd(x.float(), H, hd), lambda: ops.head_rmsnorm_fwd(z(4, 136), H, hd),
                lambda: ops.head_rmsnorm_fwd(z(4, 2, 72), H, hd), lambda: ops.head_rmsnorm_fwd(z(0, 144), H, hd),
                lambda: ops.head_rmsnorm_fwd(z(4, 290)[:, :144], H, hd),  # a row stride that is no multiple of 8
                lambda: ops.head_rmsnorm_fwd(wide[:, ::2], H, hd),          # columns not contiguous
                lambda: ops.head_rmsnorm_fwd(z(144, 4).t(), H, hd),
                lambda: ops.head_rmsnorm_fwd(x, H, 70), lambda: ops.head_rmsnorm_fwd(z(4, 272), H, 136),
                lambda: ops.head_rmsnorm_fwd(x, 0, hd), lambda: ops.head_rmsnorm_fwd(x, 2.0, hd),
                lambda: ops.head_rmsnorm_fwd(x, H, hd, eps=0.0), lambda: ops.head_rmsnorm_fwd(x, H, hd, eps=float("nan")),
                lambda: ops.head_rmsnorm_fwd(x, H, hd, eps=float("inf")), lambda: ops.head_rmsnorm_fwd(None, H, hd)):
        with pytest.raises(ValueError):
            bad()
    rstd = z(4, 2, dt=f32)
    for bad in (lambda: ops.head_rmsnorm_bwd(x.float(), x, rstd, H, hd), lambda: ops.head_rmsnorm_bwd(x, x.float(), rstd, H, hd),
                lambda: ops.head_rmsnorm_bwd(x, z(5, 144), rstd, H, hd), lambda: ops.head_rmsnorm_bwd(x, z(4, 72), rstd, H, hd),
                lambda: ops.head_rmsnorm_bwd(x, x, z(4, 2), H, hd), lambda: ops.head_rmsnorm_bwd(x, x, z(2, 4, dt=f32), H, hd),
                lambda: ops.head_rmsnorm_bwd(x, x, z(8, dt=f32), H, hd), lambda: ops.head_rmsnorm_bwd(x, x, z(4, 4, dt=f32)[:, ::2], H, hd),
                lambda: ops.head_rmsnorm_bwd(x, x, None, H, hd), lambda: ops.head_rmsnorm_bwd(x, z(4, 290)[:, :144], rstd, H, hd),
                lambda: ops.head_rmsnorm_bwd(x, x, rstd, H, 64)):
        with pytest.raises(ValueError):
            bad()
    # column windows such as ckv[:, :D] pass the checks: the call goes on to the GPU-only assertion
    for good in (lambda: ops.head_rmsnorm_fwd(wide[:, :144], H, hd), lambda: ops.head_rmsnorm_fwd(wide[:, 144:], H, hd),
                 lambda: ops.head_rmsnorm_bwd(wide[:, :144], x, rstd, H, hd)):
        with pytest.raises(AssertionError, match="GPU tensors"):
            good()


# ---------------------------------------------------------------------------------- builder and faults ----
@pytest.mark.parametrize("hd", [24, 32, 64, 72, 96, 128])
def test_builder_conditions(hd):
    """the exact inputs are what the issue of the kernels states: c_i in {0, +-1, +-2} with sum c_i^2 = hd, a mean square of
    4^a, an integer mean in the backward -- and the float64 restatement reproduces every expectation bit for bit (the
    builder itself asserts that r / the mean may move by a relative 2^-21)"""
    twos, ones, zeros = R.pattern_counts(hd)
    assert 4 * twos + ones == hd and twos + ones + zeros == hd
    if hd == 64:
        assert (twos, ones, zeros) == (8, 32, 24)
    if hd == 72:
        assert (twos, ones, zeros) == (6, 48, 18)
    M_, H = 9, 3
    x, want, r = R.exact_forward(M_, H, hd)
    xh = x.to(f64).reshape(M_, H, hd)
    zero = torch.tensor([R.zero_row(i) for i in range(M_ * H)]).reshape(M_, H)
    assert zero.any() and not zero.all()
    ms = (xh * xh).mean(dim=-1)
    assert torch.equal(ms == 0, zero)
    a = torch.log2(ms[~zero]) / 2
    assert torch.equal(a, a.round()) and a.min() >= -5 and len(set(a.tolist())) > 3
    wh = want.to(f64).reshape(M_, H, hd)
    assert set(wh.abs().unique().tolist()) == {0.0, 1.0, 2.0}
    assert torch.equal((wh * wh).sum(-1)[~zero], torch.full((int((~zero).sum()),), float(hd), dtype=f64))
    assert torch.equal(r[zero], torch.full((int(zero.sum()),), 1e-6, dtype=f64).rsqrt())
    y, r2 = R.forward_ref(x, H, hd)
    assert R._same_bits(y, want) and torch.equal(r, r2)
    k = torch.tensor([[-3, 0, 2]]).expand(M_, H)
    dy, yy, rstd, dwant = R.exact_backward(M_, H, hd, k)
    g, yh = dy.to(f64).reshape(M_, H, hd), yy.to(f64).reshape(M_, H, hd)
    assert torch.equal(g, g.round()) and torch.equal(rstd.to(f64), 2.0 ** k.to(f64))
    s = (g * yh).sum(-1)
    assert torch.equal(s % hd, torch.zeros_like(s)) and len(set((s / hd).flatten().tolist())) > 2
    dx, scale = R.backward_ref(dy, yy, rstd, H, hd)
    assert R._same_bits(dx, dwant) and float(dwant.float().abs().max()) > 0
    assert torch.all(dx.abs() <= scale)


@pytest.mark.parametrize("hd", [64, 72])
@pytest.mark.parametrize("fault", R.FAULTS)
def test_the_bitwise_compare_flags_every_injected_fault(hd, fault):
    M_, H = 9, 3
    x, want, _ = R.exact_forward(M_, H, hd)
    assert R._same_bits(R.forward_ref(x, H, hd)[0], want)
    assert not R._same_bits(R.forward_ref(x, H, hd, fault=fault)[0], want), f"forward: {fault} goes unnoticed"
    if fault != "no_eps":  # the backward has no eps: it works from the stored r
        k = torch.tensor([[-3, 0, 2]]).expand(M_, H)
        dy, y, rstd, dwant = R.exact_backward(M_, H, hd, k)
        assert R._same_bits(R.backward_ref(dy, y, rstd, H, hd)[0], dwant)
        assert not R._same_bits(R.backward_ref(dy, y, rstd, H, hd, fault=fault)[0], dwant), f"backward: {fault} goes unnoticed"


def test_float64_backward_is_the_gradient_of_the_float64_forward():
    H, hd, M_ = 3, 72, 5
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M_, H * hd, generator=g).to(bf16)
    dy = torch.randn(M_, H * hd, generator=g).to(bf16)
    xx = x.to(f64).clone().requires_grad_(True)
    xh = xx.reshape(M_, H, hd)
    yy = (xh * torch.rsqrt((xh * xh).mean(-1, keepdim=True) + R.EPS)).reshape(M_, H * hd)
    y, r = R.forward_ref(x, H, hd)
    assert torch.allclose(y, yy.detach(), rtol=1e-14, atol=0)
    yy.backward(dy.to(f64))
    dx, scale = R.backward_ref(dy, y, r, H, hd)  # from the UNROUNDED y and r: the exact Jacobian up to eps r^2
    assert torch.all((dx - xx.grad).abs() <= 2e-6 * scale + 1e-300)


# ------------------------------------------------------------------------------------------- the oracle ----
def test_the_wrapper_norms_only_the_cross_attention_and_restores_the_oracle():
    orig = O.attention
    g = torch.Generator().manual_seed(1)
    q, k, v = torch.randn(1, 2, 6, 8, generator=g) * 5, torch.randn(1, 2, 4, 8, generator=g) * 5, torch.randn(1, 2, 4, 8, generator=g)
    ks, vs = torch.randn(1, 2, 6, 8, generator=g) * 5, torch.randn(1, 2, 6, 8, generator=g)
    with R.cross_normed_oracle():
        assert O.attention is not orig
        assert torch.equal(O.attention(q, k, v), orig(O.rms_norm(q), O.rms_norm(k), v))
        assert not torch.allclose(O.attention(q, k, v), orig(q, k, v))
        assert torch.equal(O.attention(q, ks, vs), orig(q, ks, vs))  # equal counts: the self-attention, untouched
        with qk_normed_oracle():  # the two wrappers nest, in either order
            assert O.attention is not orig and O.apply_rotary is not None
    assert O.attention is orig
    with qk_normed_oracle():
        rot = O.apply_rotary
        with R.cross_normed_oracle():
            assert O.apply_rotary is rot and O.attention is not orig
        assert O.attention is orig and O.apply_rotary is rot
    with pytest.raises(RuntimeError):
        with R.cross_normed_oracle():
            raise RuntimeError("boom")
    assert O.attention is orig


def test_cross_attention_logits_of_the_wrapped_oracle_are_bounded():
    """|q^ . k^| / sqrt(hd) <= sqrt(hd) (1 + 2^-7) for every (query, key) of every block's cross-attention, whatever the
    scale of q_cross / context_kv -- the bound the norm exists for (the rows have an rms of at most 1, up to fp32 rounding)"""
    cfg = O.DiTConfig(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=144, depth=2, num_heads=2,
                      cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False)
    P = O.init_params(cfg, seed=3, randomize_zero_init=True, init_std_factor=1.0)
    for i in range(cfg.depth):
        P[f"blocks.{i}.q_cross.weight"] = P[f"blocks.{i}.q_cross.weight"] * 40
        P[f"blocks.{i}.context_kv.weight"] = P[f"blocks.{i}.context_kv.weight"] * 40
    g = torch.Generator().manual_seed(4)
    x, ctx, t = torch.randn(2, 16, 4, 8, 8, generator=g), torch.randn(2, 24, 64, generator=g), torch.rand(2, generator=g)
    hd = cfg.head_dim
    seen = {True: [], False: []}
    inner = O.attention

    def spy(normed):
        def attention(q, k, v):
            if k.shape[-2] != q.shape[-2]:
                seen[normed].append(float((q.float() @ k.float().transpose(-1, -2)).abs().max()) / math.sqrt(hd))
            return inner(q, k, v)
        return attention

    try:
        O.attention = spy(False)
        with torch.no_grad():
            O.dit_forward(P, cfg, x, ctx, t, (2, 3, 4))
            O.attention = spy(True)  # below the wrapper: it sees what the wrapper hands on
            with R.cross_normed_oracle(), qk_normed_oracle():
                O.dit_forward(P, cfg, x, ctx, t, (2, 3, 4))
    finally:
        O.attention = inner
    assert len(seen[True]) == len(seen[False]) == cfg.depth
    bound = math.sqrt(hd) * (1 + 2.0 ** -7)
    print("largest cross-attention logit per block, un-normed", seen[False], "normed", seen[True], "bound", bound)
    assert all(s <= bound for s in seen[True]), (seen[True], bound)
    assert all(s > 4 * bound for s in seen[False]), seen[False]  # the un-normed logits of the same weights are far outside
