"""Drop-in host API of the reference's `model.py` (DiT / DiTBlock / PatchEmbed / RMSNorm /
ThreeDimRotary / timestep_embedding / get_mup_setup) with the compute re-built as hand-written
gfx950 kernels behind the C ABI of include/vds.h.

Same constructor arguments, parameter names (state-dict keys) and call signatures as the
reference (model.py:279-292,358-402,404-465), so `train.py`-style code keeps working:

    dit = DiT(in_channels=16, patch_size=2, depth=28, num_heads=16, hidden_size=1152,
              cross_attn_input_size=4096, residual_v=True, train_bias_and_rms=False).to("cuda")
    out = dit(z_t, caption_encoded, t)          # [B,C,T,H,W] bf16
    loss.backward()                              # hand-written backward, fills p.grad (fp32)

What is different underneath (by design):
  * the modules below hold parameters only; `DiT.forward` runs ONE autograd node whose forward
    and backward are explicit sequences of HIP kernel launches (no torch compute ops);
  * parameters live in flat fp32 groups (params.py); kernels read a bf16 copy (the reference's
    bf16 param policy, model.py:516-518) and write fp32 gradients straight into the flat
    gradient buffer that `p.grad` aliases;
  * RoPE offsets can be pinned (`rope_start=`) -- by default they are drawn from the global CPU
    RNG with the reference's exact call sequence (model.py:223-226), so equal seeds give equal
    offsets.
There is no CPU fallback: a CPU tensor or a missing libvds_hip.so raises.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

import os

from . import fp8 as F8
from . import ops
from .params import FlatGroup

_NO_EMIT = os.environ.get("VDS_FP8_NO_EMIT") == "1"  # experiments: quantise every fp8 operand in a separate pass
_NO_PRODUCER_EMIT = os.environ.get("VDS_FP8_PRODUCER_EMIT") == "0"  # experiments: only the GEMM epilogues emit fp8
_NO_ATTN_EMIT = os.environ.get("VDS_FP8_ATTN_EMIT") == "0"  # experiments: attention results quantised in a separate pass
_CROSS_ONES = os.environ.get("VDS_CROSS_ONES", "1") != "0"  # head_dim 72: cross-attention forward / dQ on the ones-column kernels
# residual-V: d v_0 = sum over the mixed blocks of (1 - lambda_i) dv_i, summed in ONE pass before block 0's RoPE backward
# (ops.dv0_reduce) instead of an fp32 read-modify-write of the accumulator in every block (0: the per-block form)
_DV0_DEFER = os.environ.get("VDS_DV0_DEFER", "1") != "0"
_DV0_CHUNK = max(1, int(os.environ.get("VDS_DV0_CHUNK", "9")))  # dv tensors kept alive between two reductions


bf16, f32 = torch.bfloat16, torch.float32
N_REG = 16  # register tokens (model.py:316,362,386)
# head_dim -> row length of the head-major q / k / v buffers: head_dim itself, except 72 -> 96, which leaves room for the
# ones columns of the DiT-XL kernels.  The reference accepts any head_dim = hidden_size // num_heads that its RoPE table
# can be built for (a multiple of 8: model.py:192-209 reshapes arange(0, hd/2, 4) to hd/8 columns); so does this model up
# to 128 (round 5): the attention kernels are templates on a padded head dim (32 / 64 / 80+96 / 96 / 128) that fetch a
# row's chunks past head_dim as zeros, so e.g. 48 runs on the 64 instance and 112 on the 128 one (csrc/attention.hip,
# kernel_instance); head dims above 128 raise in DiT.__init__.
HDP_OF = {hd: hd for hd in range(8, 129, 8)}
HDP_OF[72] = 96


def timestep_embedding(t: torch.Tensor, dim: int, max_period: int = 10000) -> torch.Tensor:
    """[cos | sin](t * f_i), t unscaled (model.py:12-22).  HIP kernel; returns f32 [B, dim]
    holding bf16-rounded values (the reference casts the embedding to the model dtype)."""
    assert max_period == 10000
    return ops.timestep_embedding(t.to(f32).contiguous(), dim)


# ------------------------------------------------------------------ parameter holders ----
class _Linear(nn.Module):
    """nn.Linear-compatible parameter holder (weight [out,in], optional bias), reference init."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features)) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if bias:
            bound = 1 / math.sqrt(in_features)
            nn.init.uniform_(self.bias, -bound, bound)


class _Conv3dParams(nn.Module):
    """Conv3d(kernel=stride) parameter holder: weight [D, C, pt, p, p], bias [D] (model.py:173-178)."""

    def __init__(self, in_channels, out_channels, kernel):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, *kernel))
        self.bias = nn.Parameter(torch.empty(out_channels))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        fan_in = in_channels * kernel[0] * kernel[1] * kernel[2]
        nn.init.uniform_(self.bias, -1 / math.sqrt(fan_in), 1 / math.sqrt(fan_in))


class _Act(nn.Module):
    """parameter-free placeholder keeping the reference's nn.Sequential indices (SiLU / GELU)."""

    def __init__(self, kind):
        super().__init__()
        self.kind = kind


def _bf16_copy(p: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """bf16 compute copy of a stand-alone module's fp32 parameter (cast kernel, not a torch op)"""
    if p is None:
        return None
    if p.dtype == bf16:
        return p.detach().contiguous()
    out = torch.empty(p.shape, dtype=bf16, device=p.device)
    ops.cast_f32_bf16(p.detach().to(f32).contiguous(), out)
    return out


def _need_gpu(x, what):
    if not x.is_cuda:
        raise RuntimeError(f"video_diffusion_speedrun_amd.{what} runs on the GPU only (no CPU fallback)")


class _RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        D = x.shape[-1]
        x2 = x.reshape(-1, D).to(bf16).contiguous()
        rows = x2.shape[0]
        mod = torch.zeros(1, 2 * D, dtype=f32, device=x.device)  # shift = scale = 0: the bare norm of model.py:34-41
        w = _bf16_copy(weight)
        y, rstd = ops.rmsnorm_mod_fwd(x2, w, mod, 0, D, 1, rows, eps)
        ctx.save_for_backward(x2, w, mod, rstd)
        ctx.meta = (x.shape, x.dtype, weight.dtype if weight is not None else None)
        return y.view(x.shape).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        x2, w, mod, rstd = ctx.saved_tensors
        shape, xdt, wdt = ctx.meta
        D = shape[-1]
        dmod = torch.zeros(1, 2 * D, dtype=f32, device=dy.device)
        dw = torch.zeros(D, dtype=f32, device=dy.device) if w is not None else None
        dx = ops.rmsnorm_mod_bwd(dy.reshape(-1, D).to(bf16).contiguous(), x2, w, mod, 0, D, rstd, None, dmod, dw, 1,
                                 x2.shape[0])
        return dx.view(shape).to(xdt), (dw.to(wdt) if dw is not None else None), None


class RMSNorm(nn.Module):
    """model.py:25-41: y = (x.float() * rsqrt(mean(x^2) + eps) [* weight]).to(x.dtype), over the last dim.
    Inside DiT the norm runs fused with the adaLN modulation (`vds_rmsnorm_mod_fwd` with the block's shift / scale);
    called on its own it is the same kernel with zero shift / scale, differentiable through `vds_rmsnorm_mod_bwd`."""

    def __init__(self, dim, eps=1e-6, trainable=False):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim)) if trainable else None

    def forward(self, x):
        _need_gpu(x, "RMSNorm")
        return _RMSNormFn.apply(x, self.weight, self.eps)


class _RotaryFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin):
        hd = x.shape[-1]
        cos2 = cos.reshape(-1, hd // 2).to(f32).contiguous()
        sin2 = sin.reshape(-1, hd // 2).to(f32).contiguous()
        ctx.save_for_backward(cos2, sin2)
        ctx.xdt = x.dtype
        xb = x if x.dtype == bf16 and x.stride(-1) == 1 else x.to(bf16).contiguous()
        return ops.rope_apply(xb, cos2, sin2).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        cos2, sin2 = ctx.saved_tensors
        dyb = dy if dy.dtype == bf16 and dy.stride(-1) == 1 else dy.to(bf16).contiguous()
        return ops.rope_apply(dyb, cos2, sin2, inverse=True).to(ctx.xdt), None, None


def apply_rotary_emb(x, cos, sin):
    """model.py:266-275: rotate the two halves of every head row, x [B,H,L,hd], cos / sin broadcastable
    [1,1,L,hd/2]; fp32 math, result in x.dtype.  (Inside DiTBlock the rotation is fused with the qkv head split.)"""
    _need_gpu(x, "apply_rotary_emb")
    if x.dim() != 4 or cos.numel() != x.shape[2] * (x.shape[3] // 2) or sin.numel() != cos.numel():
        raise ValueError(f"apply_rotary_emb: x {tuple(x.shape)} needs cos / sin of L x hd/2 = "
                         f"{x.shape[2]} x {x.shape[3] // 2} elements, got {tuple(cos.shape)}")
    return _RotaryFn.apply(x, cos, sin)


class _PatchEmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, pt, p):
        if x.requires_grad:
            raise NotImplementedError("PatchEmbed: the gradient w.r.t. the input latents is not implemented (the "
                                      "train step never needs it: the latents are data)")
        B = x.shape[0]
        D = weight.shape[0]
        patches = ops.patchify(x.to(bf16).contiguous(), pt, p)           # [B*N, C*pt*p*p], tokens in (h w t) order
        y = ops.linear_fwd(patches, _bf16_copy(weight).view(D, -1), _bf16_copy(bias))
        ctx.save_for_backward(patches)
        ctx.meta = (weight.shape, weight.dtype, bias.dtype)
        return y.view(B, -1, D)

    @staticmethod
    def backward(ctx, dy):
        (patches,) = ctx.saved_tensors
        wshape, wdt, bdt = ctx.meta
        D = wshape[0]
        dy2 = dy.reshape(-1, D).to(bf16).contiguous()
        dW = torch.zeros(D, patches.shape[1], dtype=f32, device=dy.device)
        ops.linear_wgrad(dy2, patches, dW)
        db = torch.zeros(D, dtype=f32, device=dy.device)
        ops.colsum(dy2, db)
        return None, dW.view(wshape).to(wdt), db.to(bdt), None, None


class PatchEmbed(nn.Module):
    """model.py:170-186: Conv3d(kernel = stride = (pt, p, p)) + bias, tokens ordered (h w t): [B,C,T,H,W] ->
    [B, N, D] bf16.  A conv whose kernel equals its stride is a GEMM over gathered patches: `vds_patchify` +
    `vds_gemm_bf16`; backward = weight-gradient GEMM + column sums."""

    def __init__(self, patch_size=16, in_channels=3, embed_dim=768, time_patch_size=16):
        super().__init__()
        self.patch_proj = _Conv3dParams(in_channels, embed_dim, (time_patch_size, patch_size, patch_size))
        self.patch_size, self.time_patch_size = patch_size, time_patch_size

    def forward(self, x):
        _need_gpu(x, "PatchEmbed")
        return _PatchEmbedFn.apply(x, self.patch_proj.weight, self.patch_proj.bias, self.time_patch_size,
                                   self.patch_size)


class ThreeDimRotary(nn.Module):
    """model.py:189-263.  Keeps the per-axis factors of the reference's [128,128,128,d] cos/sin
    buffers (37 KB instead of 2 x 302 MB at head_dim 72); rows are gathered on the device."""

    def __init__(self, dim, base=100, h=128, w=128, t=128):
        super().__init__()
        assert h == 128 and w == 128 and t == 128
        self.dim, self.h, self.w, self.t = dim, h, w, t
        inv_s = 1.0 / (base ** (torch.arange(0, dim, 4).float() / dim))
        inv_t = 1.0 / (base ** (torch.arange(0, dim, 2).float() / dim))
        pos = torch.arange(128).float()
        ft, fs = torch.outer(pos, inv_t), torch.outer(pos, inv_s)
        self.register_buffer("tab_t_cos", ft.cos().contiguous(), persistent=False)
        self.register_buffer("tab_t_sin", ft.sin().contiguous(), persistent=False)
        self.register_buffer("tab_s_cos", fs.cos().contiguous(), persistent=False)
        self.register_buffer("tab_s_sin", fs.sin().contiguous(), persistent=False)

    def draw_start(self, thw) -> Tuple[int, int, int]:
        """(start_t, start_h, start_w); drawn h, w, t from the global CPU RNG (model.py:224-226)."""
        this_t, this_h, this_w = thw
        start_h = torch.randint(0, self.h - this_h + 1, (1,)).item()
        start_w = torch.randint(0, self.w - this_w + 1, (1,)).item()
        start_t = torch.randint(0, self.t - this_t + 1, (1,)).item()
        return int(start_t), int(start_h), int(start_w)

    def rows(self, thw, start, n_reg):
        tabs = (self.tab_t_cos, self.tab_t_sin, self.tab_s_cos, self.tab_s_sin)
        return ops.rope_rows(tabs, thw, start, n_reg, self.tab_t_cos.device)

    def forward(self, x, time_height_width=None, extend_with_register_tokens=0, start=None):
        if start is None:
            start = self.draw_start(time_height_width)
        cos, sin = self.rows(time_height_width, start, extend_with_register_tokens)
        return cos[None, None], sin[None, None]


def check_context_lens(context_lens, B: int, Lc: int) -> torch.Tensor:
    """Per-sample context lengths as an int32 tensor of shape [B].  A sequence of ints or a CPU integer tensor is checked
    here, on the host (B entries, each in [0, Lc]; ValueError otherwise) and comes back as a CPU tensor; a CUDA integer
    tensor is only checked for its shape and dtype and stays on the device -- no host sync, so a captured graph can
    replay it with new contents (the kernels clamp what they read to [0, Lc])."""
    if isinstance(context_lens, torch.Tensor):
        t = context_lens
        if t.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise ValueError(f"context_lens: integer tensor expected, got {t.dtype}")
        if tuple(t.shape) != (B,):
            raise ValueError(f"context_lens: shape [{B}] expected (one length per sample), got {tuple(t.shape)}")
        if t.is_cuda:
            return t.to(torch.int32).contiguous()
        vals = [int(v) for v in t.tolist()]
    else:
        try:
            vals = list(context_lens)
        except TypeError:
            raise ValueError("context_lens: a sequence of ints or an integer tensor expected") from None
        if any(isinstance(v, bool) or not isinstance(v, int) for v in vals):
            raise ValueError("context_lens: a sequence of ints expected")
        if len(vals) != B:
            raise ValueError(f"context_lens: {B} entries expected (one length per sample), got {len(vals)}")
    bad = [v for v in vals if v < 0 or v > Lc]
    if bad:
        raise ValueError(f"context_lens: every length must be in [0, {Lc}] (the context has {Lc} rows), got {bad}")
    return torch.tensor(vals, dtype=torch.int32)


def check_timesteps(timesteps, B: int, t: int) -> bool:
    """DiT.forward's timesteps: a tensor [B] (one noise level per sample; returns False) or [B, t] (one per token-frame, t = T //
    time_patch_size; returns True).  Any other shape: ValueError naming the expected t."""
    if not (isinstance(timesteps, torch.Tensor) and timesteps.dim() in (1, 2) and timesteps.shape[0] == B
            and (timesteps.dim() == 1 or timesteps.shape[1] == t)):
        got = tuple(timesteps.shape) if isinstance(timesteps, torch.Tensor) else type(timesteps).__name__
        raise ValueError(f"DiT: timesteps must have shape [{B}] (one per sample) or [{B}, {t}] (one per token-frame: "
                         f"t = T // time_patch_size = {t}), got {got}")
    return timesteps.dim() == 2


_FP8_CONTEXT_LENS = ("context_lens is not implemented for the fp8 cross-attention kernels: call "
                     "enable_fp8(cross_attention=False) to keep the cross-attention products on the bf16 kernels")


_FP8_FRAME_TIMESTEPS = ("per-frame timesteps (timesteps [B, t]) are not implemented for the fp8 kernels -- the fp8 forms of "
                        "RMSNorm+modulate, the gate backward and the GATE_RES GEMM read one modulation row per sample: "
                        "call enable_fp8(False), or pass timesteps [B]")


# the modulated kernels of a block / the final layer: per-sample (groups None: one modulation row per sample, the calls
# this model always made) or grouped (groups = (lead, period): mod / dmod are [B*G, .] tables, ops.*_grouped)
def _norm_fwd(groups, X, w, mod, shift_col, scale_col, B, L):
    if groups is None:
        return ops.rmsnorm_mod_fwd(X, w, mod, shift_col, scale_col, B, L)
    return ops.rmsnorm_mod_fwd_grouped(X, w, mod, shift_col, scale_col, B, L, groups)


def _gate_res(groups, x, W, bias, mod, gate_col, res, L, want_y=True):
    if groups is None:
        return ops.linear_fwd_gate_res(x, W, bias, mod, gate_col, res, L, want_y=want_y)
    return ops.linear_fwd_gate_res_grouped(x, W, bias, mod, gate_col, res, L, groups, want_y=want_y)


def _gate_bwd(groups, dxn, y, mod, gate_col, dmod, dbias, B, L):
    if groups is None:
        return ops.gate_bwd(dxn, y, mod, gate_col, dmod, dbias, B, L)
    return ops.gate_bwd_grouped(dxn, y, mod, gate_col, dmod, dbias, B, L, groups)


def _norm_bwd(groups, dy, x, w, mod, shift_col, scale_col, rstd, dres, dmod, dw, B, L):
    if groups is None:
        return ops.rmsnorm_mod_bwd(dy, x, w, mod, shift_col, scale_col, rstd, dres, dmod, dw, B, L)
    return ops.rmsnorm_mod_bwd_grouped(dy, x, w, mod, shift_col, scale_col, rstd, dres, dmod, dw, B, L, groups)


_FP8_QK_NORM = ("qk_norm is not implemented for the fp8 attention producers (vds_qkv_rope_fwd_fp8 has no normed form): "
                "call enable_fp8(attention=False) to keep the attention products on the bf16 kernels")


def _qk_norm_all(qk_norm) -> bool:
    """qk_norm="all": self-attention as True plus the cross-attention; every other value is its bool()"""
    return isinstance(qk_norm, str) and qk_norm == "all"


def check_frame_chunk(who: str, frame_chunk, frame_causal: bool, frame_major: bool) -> int:
    """frame_chunk of a DiT / DiTBlock: an int >= 1; more than 1 needs the frame-major frame-causal self-attention"""
    if isinstance(frame_chunk, bool) or not isinstance(frame_chunk, int) or frame_chunk < 1:
        raise ValueError(f"{who}: frame_chunk = {frame_chunk!r} must be an int >= 1 (token-frames per causal chunk)")
    if frame_chunk > 1 and not (frame_causal and frame_major):
        raise ValueError(f"{who}: frame_chunk={frame_chunk} is a mask of the frame-major frame-causal self-attention -- build "
                         "the model with frame_causal=True, frame_major=True (the interleaved kernels have no chunk mask)")
    return frame_chunk


class TeacherFrames(tuple):
    """frames = (lead, 2n) of a teacher-forcing call (DiT.forward(teacher_latents=)): the token-frames are n clean frames
    and then their n noisy copies.  A plain (lead, period) pair for every per-row kernel; the self-attention calls of a
    block run the teacher mask under it (DiTBlock._mask_kw)."""
    __slots__ = ()


def check_frame_window(who: str, frame_window, frame_chunk: int, frame_causal: bool, frame_major: bool):
    """frame_window of a DiT / DiTBlock: None, or an int >= 1 of token-frames that is a multiple of frame_chunk, on the
    frame-major frame-causal self-attention"""
    if frame_window is None:
        return None
    if isinstance(frame_window, bool) or not isinstance(frame_window, int) or frame_window < 1:
        raise ValueError(f"{who}: frame_window = {frame_window!r} must be an int >= 1 (token-frames a token attends, its own "
                         "chunk included) or None (no window)")
    if not (frame_causal and frame_major):
        raise ValueError(f"{who}: frame_window={frame_window} is a mask of the frame-major frame-causal self-attention -- "
                         "build the model with frame_causal=True, frame_major=True (the interleaved kernels have no "
                         "window: it would skip no tile there)")
    if frame_window % frame_chunk != 0:
        raise ValueError(f"{who}: frame_window={frame_window} must be a multiple of frame_chunk={frame_chunk} -- the window "
                         f"is a whole number of chunks; pass frame_window={-(-frame_window // frame_chunk) * frame_chunk}")
    return frame_window


_FP8_FRAME_BAND = ("the frame band is not implemented for the fp8 attention kernels (they have no masked instance): call "
                   "enable_fp8(attention=False) to keep the attention products on the bf16 kernels, or "
                   "enable_frame_band(None) to run without the band")
_BAND_NO_CACHE = ("a frame-band model has no K / V cache (its mask is two-sided: the K / V rows of finished frames are read "
                  "by, and change with, the frames after them)")
_FP8_FRAME_CAUSAL = ("frame_causal is not implemented for the fp8 attention kernels (they have no masked instance): "
                     "call enable_fp8(attention=False) to keep the attention products on the bf16 kernels")


class DiTBlock(nn.Module):
    """model.py:44-167.  `forward(x, context, c, v_0=None, rope=None) -> (x, v)` has the reference's signature and
    runs the block's HIP kernel sequence (`_fwd`) under one autograd node whose backward is `_bwd`; DiT.forward
    drives the same two methods for all blocks inside its own whole-model node."""

    def __init__(self, hidden_size, cross_attn_input_size, num_heads, mlp_ratio=4.0, qkv_bias=True,
                 residual_v=False, *, frame_causal=False, frame_major=False, frame_chunk=1, frame_window=None,
                 qk_norm=False):
        super().__init__()
        self.hidden_size, self.num_heads = hidden_size, num_heads
        self.head_dim = hidden_size // num_heads
        self.residual_v = residual_v
        # QK-norm (no reference counterpart): a weightless RMSNorm on every head row of the self-attention's q and k
        # before the rotation, inside the qkv / RoPE kernels (ops.qkv_rope_norm_fwd / _bwd).  No parameter.
        self.qk_norm = bool(qk_norm)
        # qk_norm="all" (exactly that string): the same norm on the cross-attention's q and k head rows as well -- the
        # q_cross output and the k columns of the context_kv output, in place right behind their linears
        # (ops.head_rmsnorm_fwd / _bwd).  v is not normed.  No parameter.  Without cross-attention: as True.
        self.qk_norm_cross = _qk_norm_all(qk_norm) and cross_attn_input_size is not None
        # frame-causal self-attention (no reference counterpart): row q attends row k iff ops.mod_group_of(k) <=
        # ops.mod_group_of(q) for the frames = (lead, period) of the call -- the masked attention kernels
        # (ops.attn_fwd / attn_bwd, frames=).  Every other kernel of the block works per row and the cross-attention only
        # reads the text, so the block (and the model) is then causal over token-frames.  No parameter.
        self.frame_causal = bool(frame_causal)
        # frame-major self-attention (with frame_causal): the head-major tensors between the qkv / RoPE
        # kernels and the attention kernels -- q, k, v, lse, dq, dk, dv, residual-V's v_0 and its gradient -- keep a
        # frame's rows contiguous (ops.fm_row), so the masked attention skips the key tiles no query of a tile attends.
        # The token order of x, qkv, attn and their gradients stays (h w t); the mathematics and the parameters are those
        # of the frame_causal block.  A cached chunk call keeps the cache's own key order and kernels.  No parameter.
        if frame_major and not frame_causal:
            raise ValueError("DiTBlock: frame_major=True lays out the frame-causal self-attention: it needs frame_causal=True")
        self.frame_major = bool(frame_major)
        # chunk-causal mask (with frame_causal and frame_major): the self-attention is causal over chunks of
        # frame_chunk token-frames and bidirectional inside a chunk -- token-frame f belongs to group 1 + f // frame_chunk
        # (ops.chunk_group_of; the last chunk may be short) -- on the same frame-major kernels (ops.attn_fwd / attn_bwd,
        # chunk=).  1 is the frame-causal mask, call for call.  A cached chunk call covers frames of ONE chunk, inside which
        # every token attends every own key: it runs the cache's past kernel with one token group.  No parameter.
        self.frame_chunk = check_frame_chunk("DiTBlock", frame_chunk, self.frame_causal, self.frame_major)
        # sliding window (with frame_causal and frame_major): a token of chunk n attends the registers and
        # the token-frames of chunks n - W + 1 .. n, W = frame_window // frame_chunk -- the WIN instances of the frame-major
        # kernels (ops.attn_fwd / attn_bwd, window=W), which also skip the key tiles BEFORE the window.  None: no window,
        # call for call.  A cached chunk call attends whatever the ring cache holds (DiT.new_frame_cache).  No parameter.
        self.frame_window = check_frame_window("DiTBlock", frame_window, self.frame_chunk, self.frame_causal,
                                               self.frame_major)
        self.norm1 = RMSNorm(hidden_size, trainable=qkv_bias)
        self.qkv = _Linear(hidden_size, hidden_size * 3, bias=qkv_bias)
        self.attn_proj = _Linear(hidden_size, hidden_size, bias=False)
        if residual_v:
            self.lambda_param = nn.Parameter(torch.tensor(0.5).reshape(1))
        if cross_attn_input_size is not None:
            self.norm2 = RMSNorm(hidden_size, trainable=qkv_bias)
            self.q_cross = _Linear(hidden_size, hidden_size, bias=qkv_bias)
            self.context_kv = _Linear(cross_attn_input_size, hidden_size * 2, bias=qkv_bias)
            self.cross_proj = _Linear(hidden_size, hidden_size, bias=False)
        else:
            self.norm2 = self.q_cross = self.context_kv = self.cross_proj = None
        self.norm3 = RMSNorm(hidden_size, trainable=qkv_bias)
        mlp_hidden = int(hidden_size * mlp_ratio)
        self.mlp = nn.Sequential(_Linear(hidden_size, mlp_hidden), _Act("gelu"), _Linear(mlp_hidden, hidden_size))
        self.adaLN_modulation = nn.Sequential(_Act("silu"), _Linear(hidden_size, 9 * hidden_size, bias=True))
        self.adaLN_modulation[-1].weight.data.zero_()
        self.adaLN_modulation[-1].bias.data.zero_()

    lora_scale: Optional[float] = None  # s = alpha / rank of the adapters DiT.add_lora put on this block's linears
    # frame band (DiT.enable_frame_band; not with frame_causal): None, or (chunk, band_chunks) -- a token of
    # chunk n attends the registers and the token-frames of chunks n - band_chunks .. n + band_chunks, the registers attend
    # everything: the BAND instances of the frame-major kernels (ops.band_attn_fwd / band_attn_bwd).  The block then takes
    # frames=(lead, period) and keeps its head-major tensors in frame-major rows exactly as a frame_major block does.
    # No parameter.
    frame_band: Optional[Tuple[int, int]] = None

    @property
    def _fm_rows(self) -> bool:
        """q, k, v, lse, dq, dk, dv, v_0 and its gradient in frame-major rows: a frame_major block or a band block"""
        return self.frame_major or self.frame_band is not None

    # ---- stand-alone call (reference signature, model.py:96-167) ---------------------------------------
    _own_group: Optional[FlatGroup] = None

    def _group_and_prefix(self, device):
        """the FlatGroup that holds this block's parameters + the name prefix they carry in it: the enclosing
        DiT's block group when there is a current one, else a group of its own (built on first use)"""
        named = list(self.named_parameters())
        g = getattr(named[0][1], "_vds_group", None)
        if g is not None and g.master is not None and g.is_current() and g.device == device:
            if g.world > 1:
                raise RuntimeError("DiTBlock.forward on a block of a sharded DiT: call the model (the sharding "
                                   "runtime gathers / reduces per block inside DiT.forward)")
            full0 = named[0][1]._vds_name
            pre = full0[:len(full0) - len(named[0][0])]
            if all(getattr(p, "_vds_group", None) is g and p._vds_name == pre + n for n, p in named):
                return g, pre
        g = FlatGroup("block", named)
        g.materialize(device)
        self._own_group = g
        return g, ""

    def _mask_kw(self, frames=None):
        """the chunk / window keywords of the full-sequence self-attention calls (nothing for the frame-causal mask);
        frames a TeacherFrames: the teacher-forcing mask over chunks of frame_chunk frames (chunk 1 included)"""
        if isinstance(frames, TeacherFrames):
            return {"chunk": self.frame_chunk, "teacher": True}
        kw = {"chunk": self.frame_chunk} if self.frame_chunk > 1 else {}
        if self.frame_window is not None:
            kw["window"] = self.frame_window // self.frame_chunk
        return kw

    def _check_frames(self, frames, L):
        if self.frame_band is not None:
            if frames is None or isinstance(frames, TeacherFrames):
                raise ValueError("DiTBlock: a frame-band block needs frames=(lead, period), the row groups of its sequence "
                                 "(lead register rows, then `period` token-frames); enable_frame_band(None) runs without")
            return ops.check_mod_groups(frames, L)
        if not self.frame_causal:
            if frames is not None:
                raise ValueError("DiTBlock: frames given to a block built without frame_causal=True")
            return None
        if frames is None:
            raise ValueError("DiTBlock: a frame_causal block needs frames=(lead, period), the row groups of its sequence")
        if isinstance(frames, TeacherFrames):
            if not self.frame_major or self.frame_window is not None:
                raise ValueError("DiTBlock: a teacher-forcing call needs a block built with frame_major=True and without "
                                 "frame_window")
            return TeacherFrames(ops.check_mod_groups(frames, L))
        return ops.check_mod_groups(frames, L)

    def forward(self, x, context, c, v_0=None, rope=None, context_lens=None, frames=None):
        """x [B,L,D], context [B,Lc,Cc] (None without cross-attention), c [B,D] conditioning, v_0 [B,H,L,hd] (block
        0's v; None in block 0), rope = (cos, sin) each [1,1,L,hd/2] or None -> (x [B,L,D], v [B,H,L,hd]) in bf16.
        Gradients flow to x, c, v_0 and the block's parameters (fp32 .grad); `context` is data (the frozen text
        encoder's output, train.py:70-87) and gets none.  context_lens (see DiT.forward): sample b attends its first
        context_lens[b] context rows only.  frames = (lead, period): required by (and only by) a frame_causal block --
        the first `lead` rows are register rows, row l >= lead belongs to token-frame (l - lead) % period."""
        frames = self._check_frames(frames, x.shape[1])
        kv_lens = None
        if context_lens is not None:
            if context is None:
                raise ValueError("DiTBlock: context_lens given to a block without cross-attention")
            kv_lens = check_context_lens(context_lens, x.shape[0], context.shape[1])
        _need_gpu(x, "DiTBlock")
        if kv_lens is not None:
            kv_lens = kv_lens.to(x.device)
        params = [p for p in self.parameters()]
        save = torch.is_grad_enabled()  # (always off inside an autograd.Function's forward: decided here)
        return _BlockFunction.apply(self, save, x, context, c, v_0, rope[0] if rope is not None else None,
                                    rope[1] if rope is not None else None, kv_lens, frames, *params)

    # ---- the kernel sequence of one block (used by DiT's whole-model autograd node and by `forward`) ----
    def _fwd(self, G, pre, X, ctx2d, cvec, v0, cos, sin, B, L, Lc, save, fp8=None, mod=None, keep=None, replay=None,
             kv_lens=None, groups=None, frames=None, cache=None):
        """X [B*L, D] bf16 token buffer -> (X_out, v [B,H,L,hdp], saved).  G: the FlatGroup holding this block's
        parameters under the name prefix `pre`; cvec f32 [B, D]; v0: block 0's v in the padded head-major layout
        or None; cos / sin f32 [L, hd/2]; fp8 = (AmaxHistory | None, block index) when the fp8 linears are on.
        Activation recomputation (DiT.enable_recompute): with save=False, keep = "full" | "selective" returns as `saved`
        only what the replay needs (X, mod; selective: attn, lse1 too).  replay = that object, with save=True: the run
        before the block's `_bwd` -- the self-attention forward is not launched when attn / lse1 were kept, and the
        new residual stream after the MLP is not stored (X_out is None: the next block's kept X already holds it).
        kv_lens: int32 device tensor [B] or None -- per-sample key counts of the cross-attention (bf16 kernels only).
        groups: None, or (lead, period) -- per-frame timesteps: cvec is f32 [B*G, D] and the modulation table [B*G, 9D],
        G = 1 + period, row b*G + g for modulation group g of sample b (bf16 kernels only).
        frames: (lead, period) of a frame_causal block's masked self-attention (bf16 attention kernels only), else None.
        cache: (k_buf, v_buf, past) of a cached chunk call (DiT.forward(frame_cache=)), inference only -- the block's k / v
        rows go straight to their place in its cache buffers [B,H,rows,hdp], the self-attention reads the first L + past
        rows of them, and the returned v IS v_buf (block 0's: the v0 later blocks read through the same row map).
        A ring cache (frame_window) passes (k_buf, v_buf, slot, rows): the token rows go behind `slot` cached rows, the
        self-attention reads the first `rows` rows with one token group (FrameKVCache.ring_call)."""
        D, H, hd = self.hidden_size, self.num_heads, self.head_dim
        frames = self._check_frames(frames, L)
        if cache is not None and (save or keep is not None or replay is not None or fp8 is not None or frames is None):
            raise RuntimeError("DiTBlock: a frame cache runs the bf16 inference forward of a frame_causal block only")
        hdp = HDP_OF[hd]
        use_fp8 = fp8 is not None
        if kv_lens is not None and use_fp8 and fp8[2] >= 2:
            raise NotImplementedError(_FP8_CONTEXT_LENS)
        if self.qk_norm and use_fp8 and fp8[2]:
            raise NotImplementedError(_FP8_QK_NORM)
        if frames is not None and use_fp8 and fp8[2]:
            raise NotImplementedError(_FP8_FRAME_BAND if self.frame_band is not None else _FP8_FRAME_CAUSAL)
        if groups is not None and use_fp8:
            raise NotImplementedError(_FP8_FRAME_TIMESTEPS)
        if use_fp8 and (keep is not None or replay is not None):
            raise ValueError("activation recomputation does not cover the fp8 path")
        fp8_hist, i, fp8_attn, fp8_lin, q_ctx = fp8 if use_fp8 else (None, 0, 0, False, None)
        W = lambda n: G.w(pre + n)
        Wo = lambda n: G.w(pre + n) if G.has(pre + n) else None
        dev = X.device
        s_lora = self.lora_scale

        def lora(name, x, y):
            """y += s (x A^T) B^T, in place, when the linear `name` carries an adapter (DiT.add_lora); returns u = x A^T"""
            if s_lora is None or not G.has(pre + name + ".lora_A"):
                return None
            u = ops.lowrank_down(x, W(name + ".lora_A"))
            ops.lowrank_up_add(u, W(name + ".lora_B"), y, s_lora)
            return u

        u_qkv = u_qc = u_ckv = None
        R0 = F8.ROWS * i
        moved = bool(getattr(G, "recast", True))  # fp8: this group's weights changed outside the fused optimizer
        if mod is None:  # (DiT.forward computes the modulation of all blocks in one batched launch and passes it in)
            mod = ops.small_linear_fwd(cvec, W("adaLN_modulation.1.weight"), W("adaLN_modulation.1.bias"), 1)
        # --- self attention (model.py:122-139)
        f8 = use_fp8 and F8.supported(B * L, 3 * D, D)
        if use_fp8 and not f8:
            raise ValueError(f"fp8 linears need B*L ({B * L}) and hidden size ({D}) to be multiples of 16")
        hist = fp8_hist if (f8 and save) else None
        emit = hist is not None and hist.ready and not _NO_EMIT  # delayed scaling: producers write fp8 themselves
        pemit = emit and not _NO_PRODUCER_EMIT
        xn1 = xn3 = None
        if pemit:
            fq, fs, rstd1 = ops.rmsnorm_mod_fwd_fp8(X, Wo("norm1.weight"), mod, 0, D, B, L, F8.E4M3,
                                                  hist.prev(F8.ROWS * i + 2), hist.part(F8.ROWS * i + 2, B * L))
            q_xn1 = F8.Q.from_rowmajor(fq, fs, save)
        else:
            xn1, rstd1 = _norm_fwd(groups, X, Wo("norm1.weight"), mod, 0, D, B, L)
        if f8:
            if not pemit:
                q_xn1 = F8.Q(xn1, F8.E4M3, True, save, hist, F8.ROWS * i + 2)
            q_wqkv = F8.Q(W("qkv.weight"), F8.E4M3, True, save, hist, R0 + F8.ROW_W + 0, weight=True, remeasure=moved)
            qkv = torch.empty(B * L, 3 * D, dtype=bf16, device=dev)
            F8.fwd(q_xn1, q_wqkv, qkv, Wo("qkv.bias"))
        else:
            qkv = ops.linear_fwd(xn1, W("qkv.weight"), Wo("qkv.bias"))
            u_qkv = lora("qkv", xn1, qkv)
        mix = self.residual_v and v0 is not None
        kept_attn = replay is not None and getattr(replay, "attn", None) is not None
        if kept_attn:
            attn, lse1 = replay.attn, replay.lse1
        else:
            attn = torch.empty(B * L, D, dtype=bf16, device=dev)
            lse1 = torch.empty(B, H, L, dtype=f32, device=dev)
        # fp8 attention (csrc/attention_fp8.hip): delayed scaling only -- q, k, v leave the RoPE kernel as e4m3 scaled by
        # the previous step's amax; until a complete step has been recorded the bf16 kernels run and the amax is taken
        a8_on = use_fp8 and fp8_attn and ops.attn_fp8_supported(hd)
        a8 = a8_on and fp8_hist.ready
        q = k = q8 = k8 = v8 = deq = e_attn = None
        if a8:
            r0 = F8.ROWS * i + F8.ROW_Q
            deq = torch.empty(8, dtype=f32, device=dev)  # {s_q, s_k, s_v, s_do, E}: include/vds.h, vds_attn_fp8_args
            cur = fp8_hist.tab[r0:r0 + 3, 1] if save else fp8_hist.scratch(5)[0::2]  # (no-grad forwards record nothing; the producers write elements 0, 2, 4 at amax_stride 2)
            q8, k8, v8, v = ops.qkv_rope_fwd_fp8(qkv, cos, sin, v0 if mix else None, W("lambda_param") if mix else None,
                                                 B, L, H, hd, hdp, fp8_hist.tab[r0:r0 + 3, 0], cur, 2, deq,
                                                 want_v=self.residual_v and v0 is None)
            # (the attn_proj operand leaves the attention epilogue as e4m3: no quantisation pass over `attn`)
            e_attn = ops.attn_fp8_fwd(q8, k8, v8, deq, ops.heads_view(attn, B, L, H, hd), lse1, hd,
                                      emit=(hist.prev(R0 + F8.ROW_ATTN), hist.cur(R0 + F8.ROW_ATTN))
                                      if (pemit and fp8_lin and not _NO_ATTN_EMIT) else None)
        else:
            if cache is not None:
                ring = len(cache) == 4
                if ring:  # the rows of slot n % W; the keys are [lead | the other slots' rows and this one's, in buffer order]
                    kb, vb, slot, rows = cache
                    past = rows - L
                else:
                    kb, vb, past = cache
                    slot, rows = past, L + past
                rope_fwd = ops.qkv_rope_norm_fwd_cache if self.qk_norm else ops.qkv_rope_fwd_cache
                q = rope_fwd(qkv, cos, sin, v0 if mix else None, W("lambda_param") if mix else None, kb, vb, frames[0], slot,
                             B, L, H, hd, hdp)
                # (frame_chunk > 1 or a ring: the call's frames are of one chunk -- one token group, frames = (lead, 1), under
                # which every token query attends every token key wherever it sits among the `rows` rows)
                ops.attn_fwd(q[..., :hd], kb[:, :, :rows, :hd], vb[:, :, :rows, :hd],
                             ops.heads_view(attn, B, L, H, hd), lse1, kv_pad_ones=(hdp - hd) >= 8,
                             frames=(frames[0], 1) if (self.frame_chunk > 1 or ring) else frames, past=past)
                k, v = kb, vb
            else:
                rope_fwd = ops.qkv_rope_norm_fwd if self.qk_norm else ops.qkv_rope_fwd
                fm_kw = dict(frames=frames) if self._fm_rows else {}  # q, k, v (and the v0 read) in frame-major rows
                q, k, v = rope_fwd(qkv, cos, sin, v0 if mix else None, W("lambda_param") if mix else None, B, L, H, hd, hdp,
                                   **fm_kw)
            if cache is None and not kept_attn and self.frame_band is not None:
                ops.band_attn_fwd(q[..., :hd], k[..., :hd], v[..., :hd], ops.heads_view(attn, B, L, H, hd), lse1,
                                  kv_pad_ones=(hdp - hd) >= 8, frames=frames, frame_major=True, chunk=self.frame_band[0],
                                  band=self.frame_band[1])
            elif cache is None and not kept_attn:
                ops.attn_fwd(q[..., :hd], k[..., :hd], v[..., :hd], ops.heads_view(attn, B, L, H, hd), lse1,
                             kv_pad_ones=(hdp - hd) >= 8, frames=frames, frame_major=self.frame_major,
                             **self._mask_kw(frames))
            if a8_on and save:  # first steps: record the amax the next step quantises with
                for j, t in enumerate((q, k, v)):
                    ops.absmax(t.view(B * H * L, hdp)[:, :hd], fp8_hist.cur(F8.ROWS * i + F8.ROW_Q + j))
        f8l = f8 and fp8_lin  # the 1152^2-class linears in fp8 too
        q_attn = q_wap = q_xn2 = q_wqc = q_wkv = q_catt = q_wcp = None
        if f8l:
            q_attn = (F8.Q.from_rowmajor(*e_attn, save) if e_attn is not None else
                      F8.Q(attn, F8.E4M3, True, save, hist, R0 + F8.ROW_ATTN))
            q_wap = F8.Q(W("attn_proj.weight"), F8.E4M3, True, save, hist, R0 + F8.ROW_W + 1, weight=True, remeasure=moved)
            y_sa, X1 = F8.fwd_gate_res(q_attn, q_wap, None, mod, 2 * D, X, L)
        else:
            y_sa, X1 = _gate_res(groups, attn, W("attn_proj.weight"), None, mod, 2 * D, X, L, want_y=save)
        # --- cross attention (model.py:142-160)
        has_cross = G.has(pre + "q_cross.weight")
        if has_cross:
            f8c = f8l and q_ctx is not None and F8.supported(B * Lc, 2 * D, ctx2d.shape[1])
            xn2 = None
            if f8c and pemit:
                fq, fs, rstd2 = ops.rmsnorm_mod_fwd_fp8(X1, Wo("norm2.weight"), mod, 3 * D, 4 * D, B, L, F8.E4M3,
                                                      hist.prev(R0 + F8.ROW_XN2), hist.part(R0 + F8.ROW_XN2, B * L))
                q_xn2 = F8.Q.from_rowmajor(fq, fs, save)
            else:
                xn2, rstd2 = _norm_fwd(groups, X1, Wo("norm2.weight"), mod, 3 * D, 4 * D, B, L)
            if f8c:
                if q_xn2 is None:
                    q_xn2 = F8.Q(xn2, F8.E4M3, True, save, hist, R0 + F8.ROW_XN2)
                q_wqc = F8.Q(W("q_cross.weight"), F8.E4M3, True, save, hist, R0 + F8.ROW_W + 2, weight=True, remeasure=moved)
                qc = torch.empty(B * L, D, dtype=bf16, device=dev)
                F8.fwd(q_xn2, q_wqc, qc, Wo("q_cross.bias"))
                q_wkv = F8.Q(W("context_kv.weight"), F8.E4M3, True, save, hist, R0 + F8.ROW_W + 3, weight=True, remeasure=moved)
                ckv = torch.empty(B * Lc, 2 * D, dtype=bf16, device=dev)
                F8.fwd(q_ctx, q_wkv, ckv, Wo("context_kv.bias"))
            else:
                qc = ops.linear_fwd(xn2, W("q_cross.weight"), Wo("q_cross.bias"))
                u_qc = lora("q_cross", xn2, qc)
                ckv = ops.linear_fwd(ctx2d, W("context_kv.weight"), Wo("context_kv.bias"))
                u_ckv = lora("context_kv", ctx2d, ckv)
            rstd_qc = rstd_kc = None
            if self.qk_norm_cross:  # in place, before anything reads qc / ckv: from here on they hold the normed rows
                rstd_qc = ops.head_rmsnorm_fwd(qc, H, hd)
                rstd_kc = ops.head_rmsnorm_fwd(ckv[:, :D], H, hd)
            catt = torch.empty(B * L, D, dtype=bf16, device=dev)
            lse2 = torch.empty(B, H, L, dtype=f32, device=dev)
            # fp8 cross-attention: the same kernels as the self-attention (Lk = context length), operands quantised by
            # vds_cross_qkv_fp8 with the previous step's amax; the bf16 kernels record the amax until a step is complete
            qc8 = kc8 = vc8 = deqc = e_catt = None
            c8_on = a8_on and fp8_attn >= 2 and Lc >= 4  # (vds_cross_qkv_fp8 works on tiles of 4 tokens)
            c8 = c8_on and fp8_hist.ready
            if c8:
                rc = R0 + F8.ROW_QC
                deqc = torch.empty(8, dtype=f32, device=dev)
                cur = fp8_hist.tab[rc:rc + 3, 1] if save else fp8_hist.scratch(5)[0::2]
                qc8, kc8, vc8 = ops.cross_qkv_fp8(qc, ckv, B, L, Lc, H, hd, fp8_hist.tab[rc:rc + 3, 0], cur, 2, deqc)
                e_catt = ops.attn_fp8_fwd(qc8, kc8, vc8, deqc, ops.heads_view(catt, B, L, H, hd), lse2, hd,
                                          emit=(hist.prev(R0 + F8.ROW_CATT), hist.cur(R0 + F8.ROW_CATT))
                                          if (pemit and f8c and not _NO_ATTN_EMIT) else None)
            else:
                if _CROSS_ONES and hd == 72:
                    # round 5: forward (and dQ) of the cross-attention on the ones-column 16x16x32 kernels of the
                    # self-attention: K / V get head-major padded copies with the ones columns (512 context rows: a 38 MB
                    # copy), the queries stay token-major (the kernels keep them in registers and set their pad columns there)
                    # (with kv_lens the copy is still of all Lc rows: the kernels bound what they read)
                    kp, vp = ops.kv_pad_ones(ckv, B, Lc, H, hd, hdp, 0, D)
                    ops.attn_fwd(ops.heads_view(qc, B, L, H, hd), kp[..., :hd], vp[..., :hd],
                                 ops.heads_view(catt, B, L, H, hd), lse2, kv_pad_ones=2, kv_lens=kv_lens)
                    del kp, vp  # (the backward pass makes them again from ckv: 12 us, nothing extra saved)
                else:
                    ops.attn_fwd(ops.heads_view(qc, B, L, H, hd), ops.heads_view(ckv, B, Lc, H, hd, 0),
                                 ops.heads_view(ckv, B, Lc, H, hd, D), ops.heads_view(catt, B, L, H, hd), lse2,
                                 kv_lens=kv_lens)
                if c8_on and save:
                    for j, t in enumerate((qc, ckv[:, :D], ckv[:, D:])):
                        ops.absmax(t, fp8_hist.cur(R0 + F8.ROW_QC + j))
            if f8c:
                q_catt = (F8.Q.from_rowmajor(*e_catt, save) if e_catt is not None else
                          F8.Q(catt, F8.E4M3, True, save, hist, R0 + F8.ROW_CATT))
                q_wcp = F8.Q(W("cross_proj.weight"), F8.E4M3, True, save, hist, R0 + F8.ROW_W + 4, weight=True, remeasure=moved)
                y_ca, X2 = F8.fwd_gate_res(q_catt, q_wcp, None, mod, 5 * D, X1, L)
            else:
                y_ca, X2 = _gate_res(groups, catt, W("cross_proj.weight"), None, mod, 5 * D, X1, L, want_y=save)
        else:
            X2 = X1
            f8c = False
        # --- MLP (model.py:163-165)
        if pemit:
            fq, fs, rstd3 = ops.rmsnorm_mod_fwd_fp8(X2, Wo("norm3.weight"), mod, 6 * D, 7 * D, B, L, F8.E4M3,
                                                  hist.prev(F8.ROWS * i + 3), hist.part(F8.ROWS * i + 3, B * L))
            q_xn3 = F8.Q.from_rowmajor(fq, fs, save)
        else:
            xn3, rstd3 = _norm_fwd(groups, X2, Wo("norm3.weight"), mod, 6 * D, 7 * D, B, L)
        if f8:
            if not pemit:
                q_xn3 = F8.Q(xn3, F8.E4M3, True, save, hist, F8.ROWS * i + 3)
            q_w1 = F8.Q(W("mlp.0.weight"), F8.E4M3, True, save, hist, R0 + F8.ROW_W + 5, weight=True, remeasure=moved)
            if emit:  # gelu(fc1) leaves the GEMM as fp8
                hpre, q_hact = F8.fwd_gelu_emit(q_xn3, q_w1, W("mlp.0.bias"), hist.prev(F8.ROWS * i), hist.cur(F8.ROWS * i), save)
                hact = None
            else:
                hpre, hact = F8.fwd_gelu(q_xn3, q_w1, W("mlp.0.bias"))
                q_hact = F8.Q(hact, F8.E4M3, True, save, hist, F8.ROWS * i)
            q_w2 = F8.Q(W("mlp.2.weight"), F8.E4M3, True, save, hist, R0 + F8.ROW_W + 6, weight=True, remeasure=moved)
            y_mlp, X3 = F8.fwd_gate_res(q_hact, q_w2, W("mlp.2.bias"), mod, 8 * D, X2, L)
            if hist is not None:
                G.recast = False  # every weight of the block has recorded its current amax
        else:
            hpre, hact = ops.linear_fwd_gelu(xn3, W("mlp.0.weight"), W("mlp.0.bias"), want_pre=save)
            if replay is not None:  # the backward reads y_mlp only: the store epilogue writes the same bits
                y_mlp, X3 = ops.linear_fwd(hact, W("mlp.2.weight"), W("mlp.2.bias")), None
            else:
                y_mlp, X3 = _gate_res(groups, hact, W("mlp.2.weight"), W("mlp.2.bias"), mod, 8 * D, X2, L,
                                                    want_y=save)
        bs = None
        if keep is not None and not save:
            bs = _Saved()
            bs.X, bs.mod = X, mod
            bs.attn, bs.lse1 = (attn, lse1) if keep == "selective" else (None, None)
        if save:
            bs = _Saved()
            bs.mod, bs.X, bs.X1, bs.X2 = mod, X, X1, X2
            bs.xn1, bs.rstd1, bs.qkv, bs.q, bs.k, bs.v, bs.attn, bs.lse1, bs.y_sa = xn1, rstd1, qkv, q, k, v, attn, lse1, y_sa
            bs.a8, bs.a8_on, bs.q8, bs.k8, bs.v8, bs.deq = a8, a8_on, q8, k8, v8, deq
            if a8:
                bs.v = None  # (block 0's bf16 v lives on as v_0; the backward contracts the fp8 copies)
            bs.mix, bs.has_cross = mix, has_cross
            bs.frames = frames
            bs.u_qkv, bs.u_qc, bs.u_ckv = u_qkv, u_qc, u_ckv  # the adapters' x A^T (None without an adapter)
            if has_cross:
                bs.xn2, bs.rstd2, bs.qc, bs.ckv, bs.catt, bs.lse2, bs.y_ca = xn2, rstd2, qc, ckv, catt, lse2, y_ca
                bs.rstd_qc, bs.rstd_kc = rstd_qc, rstd_kc  # (qk_norm="all": bs.qc / bs.ckv hold the normed rows)
                bs.c8, bs.c8_on, bs.qc8, bs.kc8, bs.vc8, bs.deqc = c8, c8_on, qc8, kc8, vc8, deqc
                if c8:
                    bs.qc = bs.ckv = None  # the backward contracts the fp8 rows
            bs.xn3, bs.rstd3, bs.hpre, bs.hact, bs.y_mlp = xn3, rstd3, hpre, hact, y_mlp
            bs.f8, bs.f8l, bs.f8c = f8, f8l, f8c
            if f8:  # the backward contracts the fp8 copies: the bf16 GEMM inputs need not be kept
                bs.q_xn1, bs.q_wqkv, bs.q_xn3, bs.q_w1, bs.q_hact, bs.q_w2 = q_xn1, q_wqkv, q_xn3, q_w1, q_hact, q_w2
                bs.xn1 = bs.xn3 = bs.hact = None
            if f8l:
                bs.q_attn, bs.q_wap = q_attn, q_wap
                if not F8.TN:
                    q_attn.q = None  # (the weight gradient contracts the transposed copy only)
            if f8c:
                bs.q_xn2, bs.q_wqc, bs.q_wkv, bs.q_catt, bs.q_wcp = q_xn2, q_wqc, q_wkv, q_catt, q_wcp
                if not F8.TN:
                    q_catt.q = q_xn2.q = None
                bs.xn2 = None
        return X3, v, bs


    def _bwd(self, G, pre, bs, dX, sv, dc, dv0, B, L, Lc, first, fp8=None, dmod=None, groups=None):
        """backward of `_fwd`: dX [B*L, D] bf16 -> d(input tokens); parameter gradients go to G's fp32 gradient
        buffer; dc (f32 [B, D]) and dv0 (f32 [B,H,L,hdp]) accumulate the conditioning / residual-V gradients.
        sv carries cos, sin, v0, ctx2d, cvec.  first: this is the block whose v was handed out as v_0.
        groups: as in `_fwd` (dc is then f32 [B*G, D])."""
        D, H, hd = self.hidden_size, self.num_heads, self.head_dim
        hdp = HDP_OF[hd]
        fp8_hist, i, _, _, q_ctx = fp8 if fp8 is not None else (None, 0, False, False, None)
        R0 = F8.ROWS * i
        W = lambda n: G.w(pre + n)
        Wo = lambda n: G.w(pre + n) if G.has(pre + n) else None
        Gr = lambda n: G.g(pre + n)
        Go = lambda n: G.g(pre + n) if G.has(pre + n) else None
        dev = dX.device
        mod = bs.mod
        batched_adaln = dmod is not None  # DiT.backward: the adaLN weight gradients of all blocks in one launch at the end
        # (round 5 measured the weight-gradient GEMMs on a second stream: +3.3 % slower -- two MFMA kernels with different LDS
        # footprints fragment the CUs; removed in round 6, profiles/r05/wgrad_side_stream_ab.log)
        # a frozen parameter (requires_grad False) gets no weight-gradient GEMM and no separate column-sum pass; a launch
        # that also produces a data gradient stays, its parameter result is simply not published (FlatGroup.publish_grads)
        T = lambda n: G.has(pre + n) and G.params[pre + n].requires_grad

        def wgrad(dy, x, n):
            if T(n):
                ops.linear_wgrad(dy, x, Gr(n))

        def wgrad8(qdy, qx, n):
            if T(n):
                F8.wgrad(qdy, qx, Gr(n))

        s_lora = self.lora_scale

        def lora_bwd(name, dY, x, u, dx):
            """backward of `lora` in _fwd on dY = the gradient of the linear's output: dB = s dY^T u and dA = dU^T x with dU
            = s dY B into the adapter's gradients, and dx += dU A (dx None: the linear's input is data)"""
            if u is None:
                return
            tA, tB = T(name + ".lora_A"), T(name + ".lora_B")
            if tB:
                ops.lowrank_wgrad(dY, u, Gr(name + ".lora_B"), s_lora, 0)
            if tA or dx is not None:
                dU = ops.lowrank_down(dY, W(name + ".lora_B"), s_lora, layout=1)
                if tA:
                    ops.lowrank_wgrad(x, dU, Gr(name + ".lora_A"), 1.0, 1)
                if dx is not None:
                    ops.lowrank_up_add(dU, W(name + ".lora_A"), dx, 1.0, layout=1)
        if dmod is None:
            dmod = torch.zeros(mod.shape[0], 9 * D, dtype=f32, device=dev)
        # --- MLP
        hist = fp8_hist if bs.f8 else None
        # (deterministic mode: the fc2 input gradient keeps its separate, fixed-order bias-gradient pass -- the GEMM epilogue's
        # fused column sums are per-tile atomics -- so the producers do not emit fp8 in backward)
        emit = hist is not None and hist.ready and not _NO_EMIT and not ops.is_deterministic()
        pemit = emit and not _NO_PRODUCER_EMIT
        if pemit:  # the fc2 output gradient leaves gate_bwd as e5m2
            fq, fs = ops.gate_bwd_fp8(dX, bs.y_mlp, mod, 8 * D, dmod, Gr("mlp.2.bias"), B, L, F8.E5M2,
                                    hist.prev(F8.ROWS * i + 4), hist.part(F8.ROWS * i + 4, B * L))
            q_dy = F8.Q.from_rowmajor(fq, fs, True)
            dy = None
        else:
            dy = _gate_bwd(groups, dX, bs.y_mlp, mod, 8 * D, dmod, Gr("mlp.2.bias"), B, L)
        if bs.f8:
            if not pemit:
                q_dy = F8.Q(dy, F8.E5M2, True, True, hist, F8.ROWS * i + 4)
            wgrad8(q_dy, bs.q_hact, "mlp.2.weight")
            if emit:  # the fc2 input gradient leaves the GEMM as e5m2 (+ transposed, + bias gradient)
                dh = None
                q_dh = F8.dgrad_gelu_emit(q_dy, bs.q_w2, bs.hpre, hist.prev(F8.ROWS * i + 1), hist.cur(F8.ROWS * i + 1),
                                          Gr("mlp.0.bias"))
            else:
                dh = F8.dgrad(q_dy, bs.q_w2, pre=bs.hpre)
                q_dh = F8.Q(dh, F8.E5M2, True, True, hist, F8.ROWS * i + 1)
                if T("mlp.0.bias"):
                    ops.colsum(dh, Gr("mlp.0.bias"))
            wgrad8(q_dh, bs.q_xn3, "mlp.0.weight")
            dxn = F8.dgrad(q_dh, bs.q_w1)
            del q_dy, q_dh
        else:
            wgrad(dy, bs.hact, "mlp.2.weight")
            dh = ops.linear_dgrad(dy, W("mlp.2.weight"), pre=bs.hpre, colsum=Gr("mlp.0.bias"))  # + fc1 bias gradient
            wgrad(dh, bs.xn3, "mlp.0.weight")
            dxn = ops.linear_dgrad(dh, W("mlp.0.weight"))
        del dh
        dX2 = _norm_bwd(groups, dxn, bs.X2, Wo("norm3.weight"), mod, 6 * D, 7 * D, bs.rstd3, dX, dmod,
                                  Go("norm3.weight"), B, L)
        # --- cross attention
        def gate_bwd_q(dXo, y, col, row):
            """the gradient w.r.t. a gated projection's output as an fp8 operand (e5m2, row-major + transposed)"""
            if pemit:
                fq, fs = ops.gate_bwd_fp8(dXo, y, mod, col, dmod, None, B, L, F8.E5M2, hist.prev(row), hist.part(row, B * L))
                return F8.Q.from_rowmajor(fq, fs, True)
            return F8.Q(_gate_bwd(groups, dXo, y, mod, col, dmod, None, B, L), F8.E5M2, True, True, hist, row)

        if bs.has_cross:
            if bs.f8c:
                q_dy = gate_bwd_q(dX2, bs.y_ca, 5 * D, R0 + F8.ROW_DY_CP)
                wgrad8(q_dy, bs.q_catt, "cross_proj.weight")
                dcatt = F8.dgrad(q_dy, bs.q_wcp)
                del q_dy
            else:
                dy = _gate_bwd(groups, dX2, bs.y_ca, mod, 5 * D, dmod, None, B, L)
                wgrad(dy, bs.catt, "cross_proj.weight")
                dcatt = ops.linear_dgrad(dy, W("cross_proj.weight"))
            # fp8 cross-attention + fp8 q_cross: dQ leaves the attention kernel as e5m2 (and as bf16 only for a bias gradient)
            emit_dqc = bs.c8 and bs.f8c and pemit and not _NO_ATTN_EMIT
            need_dqc = not emit_dqc or G.has(pre + "q_cross.bias")
            dqc = torch.empty(B * L, D, dtype=bf16, device=dev) if need_dqc else None
            dckv = torch.empty(B * Lc, 2 * D, dtype=bf16, device=dev)
            e_dqc = None
            if bs.c8:
                rd = R0 + F8.ROW_DOC
                if getattr(sv, "doq", None) is None:  # one e5m2 dO buffer per backward pass; its pad bytes stay zero
                    sv.doq = torch.zeros(B, H, L, ops.FP8_ROW, dtype=torch.float8_e5m2, device=dev)
                stats = ops.attn_fp8_delta(bs.catt, dcatt, bs.lse2, sv.doq, fp8_hist.prev(rd), fp8_hist.cur(rd), bs.deqc,
                                           B, H, L, hd)
                e_dqc = ops.attn_fp8_bwd(bs.qc8, bs.kc8, bs.vc8, sv.doq, stats, bs.deqc,
                                         ops.heads_view(dqc, B, L, H, hd) if need_dqc else None,
                                         ops.heads_view(dckv, B, Lc, H, hd, 0), ops.heads_view(dckv, B, Lc, H, hd, D), hd,
                                         emit_dq=(hist.prev(R0 + F8.ROW_DQC), hist.cur(R0 + F8.ROW_DQC))
                                         if emit_dqc else None)
            else:
                # (workspace sized by the library: statistics + the fp32 partials of its query-split dK/dV launch)
                if _CROSS_ONES and hd == 72:
                    kp, vp = ops.kv_pad_ones(bs.ckv, B, Lc, H, hd, hdp, 0, D)
                    kvw, vvw, ones = kp[..., :hd], vp[..., :hd], 2
                else:
                    kvw, vvw, ones = ops.heads_view(bs.ckv, B, Lc, H, hd, 0), ops.heads_view(bs.ckv, B, Lc, H, hd, D), 0
                ops.attn_bwd(ops.heads_view(bs.qc, B, L, H, hd), kvw, vvw, ops.heads_view(bs.catt, B, L, H, hd), bs.lse2,
                             ops.heads_view(dcatt, B, L, H, hd), ops.heads_view(dqc, B, L, H, hd),
                             ops.heads_view(dckv, B, Lc, H, hd, 0), ops.heads_view(dckv, B, Lc, H, hd, D), None,
                             kv_pad_ones=ones, kv_lens=sv.kv_lens)
                if bs.c8_on:
                    ops.absmax(dcatt, fp8_hist.cur(R0 + F8.ROW_DOC))
            if self.qk_norm_cross:  # the gradients w.r.t. the normed rows -> w.r.t. the linears' outputs, in place
                ops.head_rmsnorm_bwd(dqc, bs.qc, bs.rstd_qc, H, hd)
                ops.head_rmsnorm_bwd(dckv[:, :D], bs.ckv[:, :D], bs.rstd_kc, H, hd)
            if T("context_kv.bias"):
                ops.colsum(dckv, Gr("context_kv.bias"))
            if T("q_cross.bias"):
                ops.colsum(dqc, Gr("q_cross.bias"))
            if bs.f8c:
                q_dckv = F8.Q(dckv, F8.E5M2, F8.TN, not F8.TN, hist, R0 + F8.ROW_DCKV)  # (a weight-gradient operand only)
                wgrad8(q_dckv, q_ctx, "context_kv.weight")
                q_dqc = (F8.Q.from_rowmajor(*e_dqc, True) if e_dqc is not None else
                         F8.Q(dqc, F8.E5M2, True, True, hist, R0 + F8.ROW_DQC))
                wgrad8(q_dqc, bs.q_xn2, "q_cross.weight")
                dxn = F8.dgrad(q_dqc, bs.q_wqc)
                del q_dckv, q_dqc
            else:
                wgrad(dckv, sv.ctx2d, "context_kv.weight")
                wgrad(dqc, bs.xn2, "q_cross.weight")
                dxn = ops.linear_dgrad(dqc, W("q_cross.weight"))
                lora_bwd("context_kv", dckv, sv.ctx2d, bs.u_ckv, None)
                lora_bwd("q_cross", dqc, bs.xn2, bs.u_qc, dxn)
            dX1 = _norm_bwd(groups, dxn, bs.X1, Wo("norm2.weight"), mod, 3 * D, 4 * D, bs.rstd2, dX2, dmod,
                                      Go("norm2.weight"), B, L)
        else:
            dX1 = dX2
        # --- self attention
        if bs.f8l:
            q_dy = gate_bwd_q(dX1, bs.y_sa, 2 * D, R0 + F8.ROW_DY_AP)
            wgrad8(q_dy, bs.q_attn, "attn_proj.weight")
            dattn = F8.dgrad(q_dy, bs.q_wap)
            del q_dy
        else:
            dy = _gate_bwd(groups, dX1, bs.y_sa, mod, 2 * D, dmod, None, B, L)
            wgrad(dy, bs.attn, "attn_proj.weight")
            dattn = ops.linear_dgrad(dy, W("attn_proj.weight"))
        dq = torch.empty(B, H, L, hdp, dtype=bf16, device=dev)
        dk = torch.empty_like(dq)
        dv = torch.empty_like(dq)
        if bs.a8:
            r9 = F8.ROWS * i + F8.ROW_DO
            if getattr(sv, "doq", None) is None:  # one e5m2 dO buffer per backward pass; its pad bytes stay zero
                sv.doq = torch.zeros(B, H, L, ops.FP8_ROW, dtype=torch.float8_e5m2, device=dev)
            stats = ops.attn_fp8_delta(bs.attn, dattn, bs.lse1, sv.doq, fp8_hist.prev(r9), fp8_hist.cur(r9), bs.deq,
                                       B, H, L, hd)
            ops.attn_fp8_bwd(bs.q8, bs.k8, bs.v8, sv.doq, stats, bs.deq, dq[..., :hd], dk[..., :hd], dv[..., :hd], hd)
        else:
            delta = torch.empty(2, B, H, L, dtype=f32, device=dev)
            if self.frame_band is not None:
                ops.band_attn_bwd(bs.q[..., :hd], bs.k[..., :hd], bs.v[..., :hd], ops.heads_view(bs.attn, B, L, H, hd),
                                  bs.lse1, ops.heads_view(dattn, B, L, H, hd), dq[..., :hd], dk[..., :hd], dv[..., :hd],
                                  delta, kv_pad_ones=(hdp - hd) >= 8, frames=bs.frames, frame_major=True,
                                  chunk=self.frame_band[0], band=self.frame_band[1])
            else:
                ops.attn_bwd(bs.q[..., :hd], bs.k[..., :hd], bs.v[..., :hd], ops.heads_view(bs.attn, B, L, H, hd), bs.lse1,
                             ops.heads_view(dattn, B, L, H, hd), dq[..., :hd], dk[..., :hd], dv[..., :hd], delta,
                             kv_pad_ones=(hdp - hd) >= 8, frames=bs.frames, frame_major=self.frame_major,
                             **self._mask_kw(bs.frames))
            if bs.a8_on:
                ops.absmax(dattn, fp8_hist.cur(F8.ROWS * i + F8.ROW_DO))
        defer = getattr(sv, "dv_terms", None)  # DiT.backward: [(dv, lambda)] of the mixed blocks, summed at block 0
        mix_mode = (2 if defer is not None else 1) if bs.mix else 0
        if mix_mode == 2:
            lam = W("lambda_param")
            snap = getattr(sv, "lam_snap", None)
            if snap is not None:
                # the gathered copy this view points into is released behind this block and refilled with another block's
                # weights before the reduction runs (fsdp.ReshardRuntime): the reduction reads a copy of the value instead
                k, sv.lam_used = sv.lam_used, sv.lam_used + 1
                snap[k:k + 1].copy_(lam)
                lam = snap[k:k + 1]
            defer.append((dv, lam))  # (keeps dv alive until the next reduction)
        # summed every _DV0_CHUNK blocks (and at block 0): at most that many dv tensors stay alive (DiT-XL, B = 12: 9 x 303 MB
        # instead of 27 x 303 MB = 8 GB), for one more read-modify-write of the fp32 accumulator per chunk
        if dv0 is not None and defer and (first or len(defer) >= _DV0_CHUNK):
            ops.dv0_reduce([t for t, _ in defer], [l for _, l in defer], dv0, B, H, L, hd, hdp,
                           accumulate=getattr(sv, "dv0_started", False))
            sv.dv0_started = True
            defer.clear()
        # (QK-norm: the backward recomputes the rows' rsqrt from the qkv GEMM output, which every block keeps)
        rope_args = (dq, dk, dv, sv.cos, sv.sin, bs.qkv if (bs.mix or self.qk_norm) else None, sv.v0 if bs.mix else None,
                     W("lambda_param") if bs.mix else None, dv0 if bs.mix else (dv0 if first else None),
                     Gr("lambda_param") if bs.mix else None, mix_mode, first and dv0 is not None, B, L, H, hd, hdp)
        # the qkv output gradient leaves the RoPE backward as e5m2 (a qkv bias gradient needs the bf16 tensor)
        # (QK-norm: the normed backward has no fp8-emitting form -- the quantisation pass below takes its bf16 result)
        # (frame-major: likewise -- the fp8-emitting backward has no frame-major form)
        emit_dqkv = (pemit and not G.has(pre + "qkv.bias") and hdp % 8 == 0 and D <= 2048 and not self.qk_norm
                     and not self._fm_rows)
        if emit_dqkv:
            fq, fs = ops.qkv_rope_bwd_fp8(*rope_args, F8.E5M2, hist.prev(F8.ROWS * i + 5), hist.part(F8.ROWS * i + 5, B * L))
            q_dqkv = F8.Q.from_rowmajor(fq, fs, True)
        else:
            fm_kw = dict(frames=bs.frames) if self._fm_rows else {}  # dq, dk, dv, v0, dv0 in frame-major rows
            dqkv = (ops.qkv_rope_norm_bwd if self.qk_norm else ops.qkv_rope_bwd)(*rope_args, **fm_kw)
        if T("qkv.bias"):
            ops.colsum(dqkv, Gr("qkv.bias"))
        if bs.f8:
            if not emit_dqkv:
                q_dqkv = F8.Q(dqkv, F8.E5M2, True, True, fp8_hist, F8.ROWS * i + 5)
            wgrad8(q_dqkv, bs.q_xn1, "qkv.weight")
            dxn = F8.dgrad(q_dqkv, bs.q_wqkv)
            del q_dqkv
        else:
            wgrad(dqkv, bs.xn1, "qkv.weight")
            dxn = ops.linear_dgrad(dqkv, W("qkv.weight"))
            lora_bwd("qkv", dqkv, bs.xn1, bs.u_qkv, dxn)
        dX0 = _norm_bwd(groups, dxn, bs.X, Wo("norm1.weight"), mod, 0, D, bs.rstd1, dX1, dmod, Go("norm1.weight"),
                                  B, L)
        # --- adaLN modulation (model.py:89-94,107)
        if not batched_adaln:
            ops.small_linear_bwd(dmod, sv.cvec, W("adaLN_modulation.1.weight"), Gr("adaLN_modulation.1.weight"),
                                 Gr("adaLN_modulation.1.bias"), dc, 1)
        return dX0


class FrameKVCache:
    """K / V rows of the finished token-frames of a cached frame rollout (DiT.new_frame_cache, DiT.forward(frame_cache=)).
    Per block one K and one V buffer [batch, H, N_REG + frames*h*w, hdp] bf16 in the padded head-major layout the qkv / RoPE
    kernel writes (ones columns included): rows [0, N_REG) the register rows of the last call, then the committed frames'
    token rows, then the rows of the last call's chunk.  past_frames counts the committed token-frames.
    ring = (W, c) (a frame_window model): the buffers hold N_REG + W*c*h*w rows instead -- W slots of one chunk of c
    token-frames -- and chunk n of the video lives in slot n % W, so their size does not grow with `frames`, which stays the
    whole video's length (the RoPE table and past_frames are absolute)."""

    def __init__(self, depth, batch, heads, frames, h_tokens, w_tokens, hdp, device, ring=None):
        self.batch, self.frames, self.h_tokens, self.w_tokens = batch, frames, h_tokens, w_tokens
        self.ring = ring
        rows = N_REG + (frames if ring is None else ring[0] * ring[1]) * h_tokens * w_tokens
        self.k = [torch.zeros(batch, heads, rows, hdp, dtype=bf16, device=device) for _ in range(depth)]
        self.v = [torch.zeros(batch, heads, rows, hdp, dtype=bf16, device=device) for _ in range(depth)]
        self.past_frames = 0
        self.pending_frames = 0  # token-frames of the last forward, not yet committed
        self._rope = None  # (base, cos, sin) of the whole video's RoPE table

    def rope_rows(self, rope, start, k):
        """cos / sin rows [N_REG + k*h*w, hd/2] of a chunk of k token-frames whose first frame sits at t = start[0]: the rows
        the chunk's tokens have in the table of the WHOLE video (`frames` x h x w from the base start[0] - past_frames).  The
        reference's table is flattened (t h w) while the tokens are ordered (h w t), so a token's rotation depends on the
        video's frame count, not on its own position alone: only these rows make a chunk call equal to the full-sequence
        call restricted to the chunk's frames."""
        base = (int(start[0]) - self.past_frames, int(start[1]), int(start[2]))
        if self._rope is None or self._rope[0] != base:
            self._rope = (base,) + tuple(rope.rows((self.frames, self.h_tokens, self.w_tokens), base, N_REG))
        _, cos, sin = self._rope
        dev = cos.device
        tok = torch.arange(self.h_tokens * self.w_tokens, device=dev)[:, None] * self.frames
        rows = N_REG + tok + self.past_frames + torch.arange(k, device=dev)[None, :]
        idx = torch.cat([torch.arange(N_REG, device=dev), rows.reshape(-1)])
        return cos.index_select(0, idx), sin.index_select(0, idx)

    def ring_call(self, k):
        """(slot, rows) of a call on the k token-frames of chunk n = past_frames // c of a ring cache: the chunk's token rows
        go behind `slot` cached rows -- slot n % W -- and the self-attention reads the first `rows` rows of the buffers:
        the registers, the min(n, W - 1) chunks before this one and its own k frames while the ring fills (n < W: the own
        slot is the last of them), the whole buffer once it is full (k = c then: no stale row is read)"""
        W, c = self.ring
        hw = self.h_tokens * self.w_tokens
        n = self.past_frames // c
        if n < W:
            return n * c * hw, N_REG + n * c * hw + k * hw
        return (n % W) * c * hw, N_REG + W * c * hw

    def commit(self):
        """the token rows of the last forward become part of the past: a counter increment, the rows already sit behind
        the earlier ones (a ring: in their slot)"""
        if not self.pending_frames:
            raise RuntimeError("FrameKVCache.commit: no forward(frame_cache=) has run since the last commit() / reset()")
        self.past_frames += self.pending_frames
        self.pending_frames = 0

    def reset(self):
        """forget every frame (the buffers are kept and overwritten)"""
        self.past_frames = self.pending_frames = 0


class _Saved:
    """activations kept for the backward pass"""
    pass


class TokenRoute:
    """The row tables of one routed call (DiT.enable_token_routing), both int32 on the device: idx [Ls] -- the rows of the
    full sequence that run the routed span, [0 .. N_REG - 1] ++ (N_REG + the kept token indices), Ls = N_REG + k -- and inv
    [L], its inverse: inv[idx[i]] = i, -1 for every row that skips the span.  DiT.make_route builds one."""
    __slots__ = ("idx", "inv")

    def __init__(self, idx: torch.Tensor, inv: torch.Tensor):
        self.idx, self.inv = idx, inv


def route_keep_count(N: int, keep: float) -> int:
    """tokens of N that run the routed span at keep fraction `keep`: max(1, int(keep * N + 0.5))"""
    return max(1, int(keep * N + 0.5))


def route_tables(route, N: int):
    """host form of a TokenRoute: route = sorted, distinct token indices in [0, N) (a CPU integer tensor [k]) ->
    (idx int32 [N_REG + k], inv int32 [N_REG + N]) on the CPU"""
    k = route.shape[0]
    idx = torch.cat([torch.arange(N_REG, dtype=torch.int32), route.to(torch.int32) + N_REG])
    inv = torch.full((N_REG + N,), -1, dtype=torch.int32)
    inv[idx.long()] = torch.arange(N_REG + k, dtype=torch.int32)
    return idx, inv


_ROUTE_WHAT = ("token routing runs a span of blocks on a subset of the rows, and the rows of a subset have no frame "
               "structure: ")
_ROUTE_FRAME_CAUSAL = (_ROUTE_WHAT + "a model built with frame_causal=True (frame_major / frame_chunk / frame_window "
                       "included) derives its attention mask from a row's index -- build the model without frame_causal to "
                       "route it, or call enable_token_routing(None)")
_ROUTE_FRAME_BAND = (_ROUTE_WHAT + "the frame band derives its mask from a row's index -- call enable_frame_band(None) to "
                     "route the model, or enable_token_routing(None) to run the band")
_ROUTE_FP8 = ("token routing is not implemented for the fp8 path (the amax tables are sized by the rows of the full "
              "sequence): call enable_fp8(False) to route the model, or enable_token_routing(None) to run it in fp8")
_ROUTE_FSDP = ("token routing is not implemented for a model sharded with apply_fsdp (the reshard runtime's lambda snapshot "
               "interacts with the deferred d v_0 reduction, and no multi-GPU box exists to run it): route an unsharded "
               "model, or call enable_token_routing(None)")
_ROUTE_FRAME_TIMESTEPS = (_ROUTE_WHAT + "per-frame timesteps (timesteps [B, t]) make the grouped kernels derive a row's "
                          "modulation group from its index -- pass timesteps [B], or route=False for this call")
_ROUTE_TEACHER = (_ROUTE_WHAT + "teacher_latents needs the teacher-forcing mask of a frame-causal model -- drop "
                  "teacher_latents, or pass route=False for this call")
_ROUTE_CACHE = (_ROUTE_WHAT + "frame_cache keeps the K / V rows of whole frames -- pass frame_cache=None, or route=False "
                "for this call (a cached call is inference: call model.eval() and it runs every token)")


LORA_TARGETS = ("qkv", "q_cross", "context_kv")  # the linears DiT.add_lora can adapt: plain-store GEMMs, no fused epilogue
_FP8_LORA = ("LoRA adapters are not implemented for the fp8 linears (the adapter reads the bf16 input of the linear, which "
             "the fp8 path does not keep)")
RECOMPUTE_MODES = ("none", "full", "selective")
_FP8_RECOMPUTE = ("enable_fp8() and enable_recompute() cannot be combined: the fp8 producers write amax-history rows "
                  "during the forward pass, which a replayed forward would write a second time")


def activation_bytes(dit, B: int, latent_shape, Lc: int, mode: str = "none", routing=None) -> Dict[str, int]:
    """Bytes of the tensors a grad-enabled forward of `dit` keeps inside its blocks for the backward pass, from their
    shapes alone (no GPU): latent_shape = (T, H, W) of the input latents, Lc = context length.
      per_block   what ONE block keeps in `mode`
      kept        depth x per_block (+ nothing else: the root-level saves are the same in every mode)
      transient   one block's full set of intermediates -- what a replay holds between a block's second `_fwd` and
                  the end of its `_bwd` (0 in mode "none", whose `kept` already is depth x that)
    bf16 fp8-free path; the lists mirror the `bs.*` assignments of DiTBlock._fwd.  qk_norm="all" adds the two rstd tensors
    of the cross-attention's head norm (4 H bytes per token row and per context row).  qk_norm=True changes nothing: its
    backward reads the qkv GEMM output (3 D bf16 elements per token row), which every block -- block 0, which mixes no
    v_0, included -- already keeps and this sum already counts.
    A teacher-forcing call (forward(teacher_latents=)) runs the clean and the noisy frames as one sequence: call this with
    the doubled T, latent_shape = (2 * T, H, W), for its numbers.
    routing = (first_block, last_block, keep), the arguments of DiT.enable_token_routing: the blocks first_block ..
    last_block keep their tensors at Ls = N_REG + k rows per sample instead of L -- `kept` is then the sum over the blocks
    of the per-block figure at L or at Ls, `per_block_routed` the figure at Ls (`per_block` and `transient` stay those of a
    full-length block, the largest), `rows_routed` = B * Ls.  Not counted: the routed call's gathered v_0 (B H Ls hdp bf16)
    and its two RoPE tables, kept once per call.  None (the default): the numbers of the unrouted model, as before."""
    if mode not in RECOMPUTE_MODES:
        raise ValueError(f"activation_bytes: mode must be one of {RECOMPUTE_MODES}, got {mode!r}")
    T, Hh, Ww = latent_shape
    N = (T // dit.time_patch_size) * (Hh // dit.patch_size) * (Ww // dit.patch_size)
    per_block, full, R = _block_activation_bytes(dit, B, N + N_REG, Lc, mode)
    out = {"per_block": per_block, "kept": dit.depth * per_block, "transient": 0 if mode == "none" else full, "rows": R}
    if routing is not None:
        first, last, keep = check_token_routing(routing[0], routing[1], routing[2], dit.depth)
        routed, _, Rs = _block_activation_bytes(dit, B, N_REG + route_keep_count(N, keep), Lc, mode)
        n = last - first + 1
        out.update(kept=(dit.depth - n) * per_block + n * routed, per_block_routed=routed, rows_routed=Rs)
    return out


def check_token_routing(first_block, last_block, keep, depth: int):
    """the arguments of DiT.enable_token_routing: (first_block, last_block, keep) checked, or ValueError"""
    for name, v in (("first_block", first_block), ("last_block", last_block)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"enable_token_routing: {name} = {v!r} must be an int (a block index)")
    if not 1 <= first_block <= last_block <= depth - 1:
        raise ValueError(f"enable_token_routing: blocks {first_block} .. {last_block} must satisfy 1 <= first_block <= "
                         f"last_block <= depth - 1 = {depth - 1} (both inclusive; block 0 is never routed: it produces "
                         "residual-V's v_0 from every row)")
    if isinstance(keep, bool) or not isinstance(keep, (int, float)) or not 0.0 < float(keep) < 1.0:
        raise ValueError(f"enable_token_routing: keep = {keep!r} must be a fraction with 0 < keep < 1 (the share of the "
                         "video tokens that runs the routed blocks; 0.5 is TREAD's)")
    return first_block, last_block, float(keep)


def _block_activation_bytes(dit, B: int, L: int, Lc: int, mode: str):
    """(what one block keeps in `mode`, one block's full set of intermediates, B * L) at L rows per sample"""
    D, H, hd = dit.hidden_size, dit.num_heads, dit.head_dim
    hdp = HDP_OF[hd]
    R = B * L
    Dm = int(D * dit.mlp_ratio)
    cross = dit.cross_attn_input_size is not None
    mod = 4 * B * 9 * D
    lse = 4 * B * H * L
    full = 2 * R * D * 3                 # X, X1, X2 (X1 is X2 without cross-attention: one tensor)
    full += 2 * R * D + 4 * R            # xn1, rstd1
    full += 2 * R * 3 * D                # qkv
    full += 2 * 3 * B * H * L * hdp      # q, k, v (head-major, rows padded to hdp)
    full += 2 * R * D + lse              # attn, lse1
    full += 2 * R * D                    # y_sa
    if cross:
        full += 2 * R * D * 4 + 4 * R + lse  # xn2, qc, catt, y_ca, rstd2, lse2
        full += 2 * B * Lc * 2 * D           # ckv
        if getattr(dit, "qk_norm_cross", False):
            full += 4 * H * (R + B * Lc)     # rstd_qc, rstd_kc (qk_norm="all")
    else:
        full -= 2 * R * D                # (no X2 of its own)
    full += 2 * R * D + 4 * R            # xn3, rstd3
    full += 2 * R * Dm * 2               # hpre, hact
    full += 2 * R * D                    # y_mlp
    lora = getattr(dit, "lora", None)
    if lora is not None:                 # u = x A^T of every adapted linear
        r = lora["rank"]
        full += 2 * r * sum({"qkv": R, "q_cross": R if cross else 0, "context_kv": B * Lc if cross else 0}[t]
                            for t in lora["targets"])
    full += mod
    per_block = {"none": full, "full": 2 * R * D + mod, "selective": 2 * R * D + mod + 2 * R * D + lse}[mode]
    return per_block, full, R


def _offsets(groups):
    off = 0
    for g in groups:
        yield off
        off += g.padded


def grad_arena(groups, device):
    """one fp32 allocation for the full-size gradient buffers of all flat groups (4.5 GB for DiT-XL), 1 KiB-aligned
    slices (a group's padded size is a multiple of 256 elements)"""
    return torch.zeros(sum(g.padded for g in groups), dtype=f32, device=device)


class DiT(nn.Module):
    def __init__(self, in_channels=4, patch_size=2, time_patch_size=2, hidden_size=1152, depth=28, num_heads=16,
                 mlp_ratio=4.0, cross_attn_input_size=128, residual_v=False, train_bias_and_rms=True,
                 use_rope=True, *, frame_causal=False, frame_major=False, frame_chunk=1, frame_window=None,
                 qk_norm=False):
        super().__init__()
        self.qk_norm = bool(qk_norm)  # see DiTBlock: parameter-free RMSNorm of q and k in the self-attention
        # see DiTBlock: qk_norm="all" norms the cross-attention's q and k too (a model without cross-attention: as True)
        self.qk_norm_cross = _qk_norm_all(qk_norm) and cross_attn_input_size is not None
        # see DiTBlock: every self-attention runs with frames = (N_REG, t) -- the registers attend each other, a token of
        # frame f the registers and frames 0 .. f.  The model is then causal over token-frames in the LATENTS; with
        # per-frame timesteps the registers are still modulated from the row maximum of the timesteps, so it is not causal
        # in the noise levels of later frames.
        self.frame_causal = bool(frame_causal)
        # see DiTBlock: the full-sequence self-attention of every block in frame-major rows (training, rollout without a
        # cache); the same mathematics, parameters and checkpoints as the frame_causal model
        if frame_major and not frame_causal:
            raise ValueError("DiT: frame_major=True lays out the frame-causal self-attention: it needs frame_causal=True")
        self.frame_major = bool(frame_major)
        # see DiTBlock: causal over chunks of frame_chunk token-frames, bidirectional inside a chunk (1: frame-causal);
        # the model that a rollout of frame_chunk frames at a time (generate_latents(rollout_frames=)) is trained as
        self.frame_chunk = check_frame_chunk("DiT", frame_chunk, self.frame_causal, self.frame_major)
        # see DiTBlock: a token attends the registers and the last frame_window token-frames (whole chunks) only -- the
        # training cost of a token and the rollout's cache (new_frame_cache: a ring) no longer grow with the video
        self.frame_window = check_frame_window("DiT", frame_window, self.frame_chunk, self.frame_causal, self.frame_major)
        self.in_channels = self.out_channels = in_channels
        self.patch_size, self.time_patch_size = patch_size, time_patch_size
        self.hidden_size, self.num_heads, self.depth, self.mlp_ratio = hidden_size, num_heads, depth, mlp_ratio
        self.use_rope = use_rope
        self.residual_v = residual_v
        self.cross_attn_input_size = cross_attn_input_size
        self.head_dim = hidden_size // num_heads
        if self.head_dim not in HDP_OF:
            raise ValueError(f"head_dim {self.head_dim} = hidden_size / num_heads has no attention kernel instance "
                             "(multiples of 8 up to 128: DiT-S/B = 64, DiT-XL = 72, the reference's sweep = 128, its "
                             "smoke test = 32; the reference's own RoPE table needs a multiple of 8 too, model.py:192-209); "
                             "the kernels are templates on the padded head dim, see csrc/attention.hip")
        self.patch_embed = PatchEmbed(patch_size, in_channels, hidden_size, time_patch_size)
        if use_rope:
            self.rope = ThreeDimRotary(hidden_size // (2 * num_heads), h=128, w=128, t=128)
        else:
            # model.py:312-314: without RoPE the reference registers a learned table it never reads -- its forward
            # calls self.rope unconditionally (model.py:364) and raises AttributeError.  The parameter is
            # kept so that such a model's state dict (and train.py:287's constant class "positional_embedding") round
            # trips with strict loading; forward refuses like the reference does.
            self.positional_embedding = nn.Parameter(torch.zeros(1, 2048, hidden_size))
        self.register_tokens = nn.Parameter(torch.randn(1, N_REG, hidden_size))
        self.time_embed = nn.Sequential(_Linear(hidden_size, 4 * hidden_size), _Act("silu"),
                                        _Linear(4 * hidden_size, hidden_size))
        self.blocks = nn.ModuleList([
            DiTBlock(hidden_size=hidden_size, num_heads=num_heads, mlp_ratio=mlp_ratio,
                     cross_attn_input_size=cross_attn_input_size, residual_v=residual_v,
                     qkv_bias=train_bias_and_rms, qk_norm=qk_norm, frame_causal=frame_causal,
                     frame_major=frame_major, frame_chunk=self.frame_chunk, frame_window=self.frame_window)
            for _ in range(depth)])
        self.final_modulation = nn.Sequential(_Act("silu"), _Linear(hidden_size, 2 * hidden_size, bias=True))
        self.final_norm = RMSNorm(hidden_size, trainable=train_bias_and_rms)
        self.final_proj = _Linear(hidden_size, patch_size * patch_size * time_patch_size * self.out_channels)
        nn.init.zeros_(self.final_modulation[-1].weight)
        nn.init.zeros_(self.final_modulation[-1].bias)
        nn.init.zeros_(self.final_proj.weight)
        nn.init.zeros_(self.final_proj.bias)
        self.paramstatus = {}
        for n, p in self.named_parameters():
            self.paramstatus[n] = {"shape": p.shape, "requires_grad": p.requires_grad}
        # flat groups (built lazily on the device): root + one per block, FSDP units of model.py:523-541
        self._groups: Optional[List[FlatGroup]] = None
        self._world, self._rank, self._pg = 1, 0, None
        self._fsdp = None  # set by fsdp.apply_fsdp
        self.fp8 = False   # enable_fp8(): qkv / mlp GEMMs on the fp8 MFMA path (fp8.py; BASELINE config 5)
        self.fp8_attn = 0  # ... and the attention products (1: self-attention, 2: cross-attention too)
        self.fp8_lin = False   # ... and the four remaining linears of a block
        self.recompute = "none"  # enable_recompute(): what the forward keeps for the backward ("none" | "full" | "selective")
        self.lora = None  # add_lora(): {"rank", "alpha", "targets"} of the low-rank adapters on the blocks' q/k/v linears
        self.frame_band = None  # enable_frame_band(): (chunk, band_chunks) of the blocks' two-sided frame band, or None
        self._lora_frozen: List[str] = []  # names add_lora(freeze_base=True) froze (merge_lora un-freezes exactly these)
        self.token_routing = None  # enable_token_routing(): (first_block, last_block, keep) of the routed span, or None

    def enable_token_routing(self, first_block, last_block=None, keep: float = 0.5):
        """Token routing (TREAD): in training, the blocks first_block .. last_block (both inclusive, 1 <=
        first_block <= last_block <= depth - 1) run on the 16 register rows and a random subset of k = max(1, int(keep * N +
        0.5)) of the N video tokens, drawn per call and shared by the batch; the other tokens skip the span -- they enter
        block last_block + 1 with the value they had before block first_block -- and rejoin at their places.  The routed
        blocks are the block code at the shorter length Ls = 16 + k with gathered side inputs (v_0, the RoPE rows); the
        rows move through ops.rows_gather / rows_merge / rows_scatter_add.  enable_token_routing(None) switches it off, and
        the model launches exactly the kernels it launched before.  No parameter, no checkpoint key.
        A call is routed when the switch is on, the model is in training mode and gradients are enabled: model.eval() and
        torch.no_grad() (the sampler) run every token.  forward(route=) overrides that per call.  The subset is
        torch.randperm(N)[:k].sort() from the global CPU RNG (draw_route), drawn after the RoPE offsets.
        Works with residual_v, qk_norm, context_lens, enable_recompute, set_deterministic, LoRA, GraphedTrainStep and every
        optimizer.  Refused -- everything that derives something from a row's index: a frame_causal model, the frame band,
        timesteps [B, t], teacher_latents, frame_cache; and enable_fp8 and apply_fsdp.  Returns self."""
        if first_block is None:
            self.token_routing = None
            return self
        args = check_token_routing(first_block, first_block if last_block is None else last_block, keep, self.depth)
        if self.frame_causal:
            raise ValueError("enable_token_routing: " + _ROUTE_FRAME_CAUSAL)
        if self.frame_band is not None:
            raise ValueError("enable_token_routing: " + _ROUTE_FRAME_BAND)
        if self.fp8:
            raise NotImplementedError("enable_token_routing: " + _ROUTE_FP8)
        if self._fsdp is not None or self._world > 1:
            raise NotImplementedError("enable_token_routing: " + _ROUTE_FSDP)
        self.token_routing = args
        return self

    def draw_route(self, N: int) -> torch.Tensor:
        """the kept token indices of one routed call on N video tokens: int32 [k], k = max(1, int(keep * N + 0.5)), sorted and
        distinct -- torch.randperm(N)[:k].sort().values from the global CPU RNG (equal seeds give equal subsets)"""
        if self.token_routing is None:
            raise ValueError("draw_route: token routing is off -- call enable_token_routing(first_block, last_block, keep) "
                             "first")
        k = route_keep_count(int(N), self.token_routing[2])
        return torch.randperm(int(N))[:k].sort().values.to(torch.int32)

    def make_route(self, route, N: int, device) -> TokenRoute:
        """route -> the device tables of a routed call on N video tokens.  route: sorted, distinct token indices in [0, N)
        as a list or a CPU integer tensor (validated here, on the host; one small copy to the device), or a device int32
        tensor [k] that is NOT validated (no host sync, so a captured graph can replay it with new contents; the row
        kernels guard every index they read); a TokenRoute passes through."""
        device = torch.device(device)
        if isinstance(route, TokenRoute):  # (host tables are uploaded: one small copy each)
            return route if route.idx.device == device else TokenRoute(route.idx.to(device), route.inv.to(device))
        if isinstance(route, torch.Tensor) and route.is_cuda:
            if route.dtype != torch.int32 or route.dim() != 1 or route.shape[0] < 1:
                raise ValueError(f"DiT: a device route must be an int32 tensor of shape [k], k >= 1, got {route.dtype} "
                                 f"{tuple(route.shape)} -- pass route.to(torch.int32), or a list / CPU tensor to have it "
                                 "checked")
            k = route.shape[0]
            idx = torch.cat([torch.arange(N_REG, dtype=torch.int32, device=route.device), route + N_REG])
            # inv without a scatter (an unchecked index must not address memory): row l = N_REG + tok is routed iff tok is
            # in the sorted route, at the position a binary search finds
            tok = torch.arange(N, dtype=torch.int32, device=route.device)
            pos = torch.searchsorted(route, tok).clamp_(max=k - 1)
            hit = route[pos] == tok
            inv_tok = torch.where(hit, (pos + N_REG).to(torch.int32), torch.full_like(tok, -1))
            inv = torch.cat([torch.arange(N_REG, dtype=torch.int32, device=route.device), inv_tok])
            return TokenRoute(idx.contiguous(), inv.contiguous())
        if isinstance(route, torch.Tensor):
            if route.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) or route.dim() != 1:
                raise ValueError(f"DiT: route must be a 1-D integer tensor of token indices, got {route.dtype} "
                                 f"{tuple(route.shape)}")
            vals = [int(v) for v in route.tolist()]
        else:
            try:
                vals = list(route)
            except TypeError:
                raise ValueError("DiT: route must be False, None, a sequence of ints or an integer tensor (the kept token "
                                 "indices)") from None
            if any(isinstance(v, bool) or not isinstance(v, int) for v in vals):
                raise ValueError("DiT: route must hold ints (the kept token indices)")
        if not vals:
            raise ValueError("DiT: route is empty -- at least one token runs the routed span; pass route=False to run the "
                             "full model")
        bad = [v for v in vals if v < 0 or v >= N]
        if bad:
            raise ValueError(f"DiT: every route index must be in [0, {N}) (this call has {N} video tokens), got {bad[:8]}")
        if any(b <= a for a, b in zip(vals, vals[1:])):
            raise ValueError("DiT: route must be sorted and distinct (strictly increasing token indices) -- pass "
                             "sorted(set(route))")
        idx, inv = route_tables(torch.tensor(vals, dtype=torch.int32), N)
        return TokenRoute(idx.to(device), inv.to(device))  # one small copy each

    def _route_requested(self, route) -> bool:
        """does this call run the routed span?  (route of DiT.forward; the switch, the mode and the override)"""
        if self.token_routing is None:
            if route is not None and route is not False:
                raise ValueError("DiT: route= given to a model without token routing -- call enable_token_routing("
                                 "first_block, last_block, keep) first, or drop route")
            return False
        if route is False:
            return False
        if route is None:
            return self.training and torch.is_grad_enabled()
        if isinstance(route, bool):
            raise ValueError("DiT: route=True is no route -- pass None (routed in training mode, on a drawn subset), False "
                             "(the full model) or the kept token indices")
        return True

    def enable_fp8(self, on: bool = True, attention: bool = True, all_linears: bool = True,
                   cross_attention: bool = True):
        """Run the qkv and MLP linears of every block in OCP fp8 (e4m3 activations / weights, e5m2 gradients,
        per-tensor scaling) and, with `attention`, the attention products on the fp8 MFMA as well (head_dim 72:
        e4m3 Q / K / V / P, e5m2 dO / dS; fp8.py states the recipe).  The reference has no such mode.
        `cross_attention=False` keeps the cross-attention products (L x 512 context keys) on the bf16 kernels: in fp8
        they are 1.1 % of the step faster at the C3b shape and leave the 200-step loss curve where it was, at a
        cross-attention output 4.6 % instead of 0.3 % from the fp32 oracle.
        A model built with qk_norm=True has no fp8 attention producer: `attention=True` raises NotImplementedError there
        (enable_fp8(attention=False) runs its linears in fp8 and the normed attention in bf16).  The same
        holds for a model built with frame_causal=True: the fp8 attention kernels have no masked instance."""
        if on and self.token_routing is not None:
            raise NotImplementedError("enable_fp8: " + _ROUTE_FP8)
        if on and self.recompute != "none":
            raise ValueError(_FP8_RECOMPUTE)
        if on and self.lora is not None:
            raise NotImplementedError(_FP8_LORA + ": call merge_lora() first, or keep the model in bf16 (enable_fp8(False))")
        if on and attention and self.qk_norm:
            raise NotImplementedError(_FP8_QK_NORM)
        if on and attention and self.frame_causal:
            raise NotImplementedError(_FP8_FRAME_CAUSAL)
        if on and attention and self.frame_band is not None:
            raise NotImplementedError(_FP8_FRAME_BAND)
        self.fp8 = bool(on)
        self.fp8_attn = (2 if cross_attention else 1) if (on and attention) else 0  # 0 none, 1 self, 2 self + cross
        self.fp8_lin = bool(on and all_linears)  # attn_proj, q_cross, context_kv, cross_proj too (qkv / MLP always)
        self._fp8_hist = None  # fp8.AmaxHistory: 6 rows per block (gelu(fc1), d fc2-in, xn1, xn3, d mlp-out, d qkv)
        return self

    def enable_frame_band(self, band, chunk: int = 1):
        """Frame-band self-attention for the bidirectional model: a token of chunk n -- chunks of `chunk`
        token-frames, the last one short when the video's frame count is no multiple -- attends the register tokens and
        the token-frames of chunks n - band // chunk .. n + band // chunk; the register tokens attend, and are attended
        by, every token.  `band` counts token-frames on EACH side of the token's own chunk: an int >= 0 and a multiple
        of `chunk` (0: own chunk plus registers); None switches the band off, and the model launches exactly the kernels
        it launched before.  The mask is symmetric, not causal: there is no cache for it.
        Every block then runs the frame-major qkv / RoPE kernels and the BAND attention kernels (ops.band_attn_fwd /
        band_attn_bwd), which skip the key tiles outside a workgroup's band, in forward, backward and recompute replay; its
        head-major tensors and residual-V's v_0 live in frame-major rows as on a frame_major=True model.  No parameter, no
        checkpoint key, the same activation_bytes.  Works with residual_v, qk_norm, context_lens, per-frame timesteps,
        enable_recompute, GraphedTrainStep, train.forward's frame modes (not "teacher"), generate_latents without
        kv_cache, and LoRA.  Not on a frame_causal model (its masks are causal: frame_window is the bounded one there) and
        not with fp8 attention (enable_fp8(attention=False) keeps the linears in fp8).  Returns self."""
        if band is None:
            self.frame_band = None
            for blk in self.blocks:
                blk.frame_band = None
            return self
        if self.token_routing is not None:
            raise ValueError("enable_frame_band: " + _ROUTE_FRAME_BAND)
        if self.frame_causal:
            raise ValueError("enable_frame_band: the frame band is the two-sided mask of the bidirectional model; this model "
                             "was built with frame_causal=True -- bound its causal attention with frame_window= (with "
                             "frame_major=True) instead, or build the model without frame_causal")
        if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
            raise ValueError(f"enable_frame_band: chunk = {chunk!r} must be an int >= 1 (token-frames per chunk)")
        if isinstance(band, bool) or not isinstance(band, int) or band < 0:
            raise ValueError(f"enable_frame_band: band = {band!r} must be an int >= 0 (token-frames attended on each side of "
                             "a token's own chunk; 0: own chunk plus registers) or None (no band)")
        if band % chunk != 0:
            raise ValueError(f"enable_frame_band: band={band} must be a multiple of chunk={chunk} -- the band is a whole "
                             f"number of chunks on each side; pass band={-(-band // chunk) * chunk}")
        if self.fp8 and self.fp8_attn:
            raise NotImplementedError(_FP8_FRAME_BAND)
        self.frame_band = (chunk, band // chunk)
        for blk in self.blocks:
            blk.frame_band = self.frame_band
        return self

    def enable_recompute(self, mode: str = "selective"):
        """Activation recomputation: what the forward pass keeps per block for the hand-written backward.
          "none"       every intermediate of `_fwd` (27 D bf16 elements per token row and block);
          "full"       the block's input token buffer and its modulation row; `_backward_impl` runs the block's `_fwd`
                       again right before its `_bwd`, so only ONE block's intermediates exist at a time;
          "selective"  additionally the self-attention output and its log-sum-exp (2 D per row): the replay does not
                       launch the self-attention forward, the one kernel that dominates a long clip's forward.
        The replay launches the forward's own fixed-order kernels on the same inputs: gradients are bit-identical to
        "none" in deterministic mode.  Not together with enable_fp8() (the fp8 producers record amax rows
        during the forward; a replay would record them twice).  Returns self."""
        if mode not in RECOMPUTE_MODES:
            raise ValueError(f"enable_recompute: mode must be one of {RECOMPUTE_MODES}, got {mode!r}")
        if mode != "none" and self.fp8:
            raise ValueError(_FP8_RECOMPUTE)
        self.recompute = mode
        return self

    # ---------------------------------------------------------------- low-rank adapters ----
    def refresh_paramstatus(self):
        """rebuild `paramstatus` (what get_mup_setup / get_muon_setup read) from the parameters as they are now: call it
        after freezing or un-freezing parameters by hand (`p.requires_grad_(False)`); add_lora / merge_lora do."""
        self.paramstatus = {n: {"shape": p.shape, "requires_grad": p.requires_grad} for n, p in self.named_parameters()}

    def _lora_linears(self, targets=None):
        """[(name of the linear, its _Linear)] of the blocks' linears that carry (or, with `targets`, would carry) an adapter"""
        targets = self.lora["targets"] if targets is None else targets
        out = []
        for i, blk in enumerate(self.blocks):
            for t in targets:
                lin = getattr(blk, t, None)
                if lin is not None:
                    out.append((f"blocks.{i}.{t}", lin))
        return out

    def add_lora(self, rank: int = 16, alpha=None, targets=LORA_TARGETS, freeze_base: bool = True, generator=None):
        """Low-rank adapters (LoRA) on the attention input projections of every block: a targeted linear computes
        y = x W^T + b + s (x A^T) B^T with s = alpha / rank (alpha defaults to rank), A = `lora_A` [rank, in] drawn uniformly
        in +-1/sqrt(in) from `generator`, B = `lora_B` [out, rank] zero -- so the model's output is unchanged until the
        adapters are trained.  targets: any of "qkv", "q_cross", "context_kv"; the other linears of a block (attn_proj,
        cross_proj, the MLP) run GEMMs with fused gate / GELU epilogues and take no adapter.  The adapter products are the
        vds_lowrank_* kernels (csrc/lowrank.hip), in every path that runs the linear: training, recompute replay,
        per-frame timesteps, frame-major / windowed attention, QK-norm, context_lens and the cached rollout.
        freeze_base=True: every parameter that existed before the call stops training (requires_grad False) -- it gets no
        .grad, and the backward launches none of its weight-gradient GEMMs.  get_lora_setup() returns the optimizer groups
        of the adapters; merge_lora() folds them into the weights.  bf16 only (not with enable_fp8), unsharded only (not
        with apply_fsdp).  Returns self."""
        if self.lora is not None:
            raise ValueError("add_lora: this model already carries adapters -- call merge_lora() to fold them into the "
                             "weights first, or load other adapter values with load_lora_state_dict()")
        if isinstance(rank, bool) or rank not in ops.LOWRANK_RANKS:
            raise ValueError(f"add_lora: rank = {rank!r} has no kernel instance -- pass one of {ops.LOWRANK_RANKS}")
        targets = tuple(targets)
        bad = [t for t in targets if t not in LORA_TARGETS]
        if bad or not targets or len(set(targets)) != len(targets):
            raise ValueError(f"add_lora: targets = {targets!r}: pass distinct names out of {LORA_TARGETS} (attn_proj, "
                             "cross_proj and the MLP linears have fused-epilogue GEMMs and take no adapter)")
        if self.fp8:
            raise NotImplementedError(_FP8_LORA + ": call enable_fp8(False) before add_lora()")
        if self._fsdp is not None or self._world > 1:
            raise NotImplementedError("add_lora: adapters on a model sharded with apply_fsdp are not implemented -- add them "
                                      "to an unsharded copy of the weights (full_state_dict())")
        alpha = float(rank if alpha is None else alpha)
        if not alpha > 0.0 or alpha != alpha or alpha == float("inf"):
            raise ValueError(f"add_lora: alpha = {alpha!r} must be a positive finite number (s = alpha / rank)")
        linears = self._lora_linears(targets)
        if not linears:
            raise ValueError(f"add_lora: no block of this model has any of {targets} (cross_attn_input_size=None leaves "
                             "only \"qkv\")")
        for name, lin in linears:
            if lin.in_features % 8 or lin.out_features % 8:
                raise ValueError(f"add_lora: {name} is {lin.out_features} x {lin.in_features}; the low-rank kernels need "
                                 "both to be multiples of 8 -- drop it from `targets`")
        before = list(self.named_parameters())
        for name, lin in linears:
            w = lin.weight
            a = torch.empty(rank, lin.in_features, dtype=torch.float32)
            bound = 1.0 / math.sqrt(lin.in_features)
            a.uniform_(-bound, bound, generator=generator)
            lin.lora_A = nn.Parameter(a.to(device=w.device, dtype=w.dtype))
            lin.lora_B = nn.Parameter(torch.zeros(lin.out_features, rank, device=w.device, dtype=w.dtype))
        self._lora_frozen = []
        if freeze_base:
            for n, p in before:
                if p.requires_grad:
                    p.requires_grad_(False)
                    self._lora_frozen.append(n)
        self.lora = {"rank": int(rank), "alpha": alpha, "targets": targets}
        for blk in self.blocks:
            blk.lora_scale = alpha / rank
        self.refresh_paramstatus()
        self._groups = None  # the flat groups are rebuilt with the adapters as members
        return self

    def lora_parameters(self):
        """[(name, parameter)] of the adapter tensors, in named_parameters() order"""
        if self.lora is None:
            return []
        return [(n, p) for n, p in self.named_parameters() if n.endswith((".lora_A", ".lora_B"))]

    def get_lora_setup(self, learning_rate, weight_decay=0.0):
        """(optimizer param groups, {name: {"lr", "wd", "shape"}}) in get_mup_setup's format for the adapter parameters
        only: ONE group, every trainable lora_A / lora_B at `learning_rate` and `weight_decay` (an adapter is its own
        small model: the width-dependent muP factors of get_mup_setup, whose cascade is unchanged, do not apply)."""
        if self.lora is None:
            raise ValueError("get_lora_setup: this model has no adapters -- call add_lora() first")
        group = {"params": [], "weight_decay": float(weight_decay), "lr": float(learning_rate)}
        table = {}
        for n, p in self.lora_parameters():
            if not p.requires_grad:
                continue
            group["params"].append(p)
            table[n] = {"lr": float(learning_rate), "wd": float(weight_decay), "shape": self.paramstatus[n]["shape"]}
        return [group], table

    def lora_state_dict(self) -> Dict[str, object]:
        """the adapter tensors (fp32 copies, keyed like named_parameters()) plus "rank", "alpha" and "targets": what a
        fine-tune has to ship next to the base checkpoint"""
        if self.lora is None:
            raise ValueError("lora_state_dict: this model has no adapters -- call add_lora() first")
        sd: Dict[str, object] = {n: p.detach().clone() for n, p in self.lora_parameters()}
        sd.update(rank=self.lora["rank"], alpha=self.lora["alpha"], targets=list(self.lora["targets"]))
        return sd

    def load_lora_state_dict(self, sd):
        """load what lora_state_dict() returned into this model's adapters; the rank, alpha, targets, the set of names
        and every shape must match (ValueError otherwise: build the adapters with the add_lora() arguments of the file)"""
        if self.lora is None:
            raise ValueError("load_lora_state_dict: this model has no adapters -- call add_lora(rank=sd['rank'], "
                             "alpha=sd['alpha'], targets=sd['targets']) first")
        meta = {k: sd.get(k) for k in ("rank", "alpha", "targets")}
        if (meta["rank"] != self.lora["rank"] or meta["alpha"] is None or float(meta["alpha"]) != self.lora["alpha"]
                or meta["targets"] is None or tuple(meta["targets"]) != self.lora["targets"]):
            raise ValueError(f"load_lora_state_dict: the file holds adapters of {meta}, this model has {self.lora} -- call "
                             "add_lora() with the file's rank, alpha and targets")
        own = dict(self.lora_parameters())
        keys = {k for k in sd if k not in ("rank", "alpha", "targets")}
        if keys != set(own):
            raise ValueError(f"load_lora_state_dict: adapter names differ: missing {sorted(set(own) - keys)}, unexpected "
                             f"{sorted(keys - set(own))}")
        for n, p in own.items():
            if tuple(sd[n].shape) != tuple(p.shape):
                raise ValueError(f"load_lora_state_dict: {n} is {tuple(sd[n].shape)} in the file, {tuple(p.shape)} here")
        with torch.no_grad():
            for n, p in own.items():
                p.copy_(sd[n].to(device=p.device, dtype=p.dtype))
        self.invalidate_compute_copy()

    def merge_lora(self):
        """fold the adapters into the weights: W += s B A in fp32 on the masters, then remove lora_A / lora_B, give back
        requires_grad to what add_lora froze and re-cast the compute copies.  The state dict has the reference's keys
        again; up to the bf16 rounding of the merged weight the model computes what it computed with the adapters."""
        if self.lora is None:
            raise ValueError("merge_lora: this model has no adapters -- call add_lora() first")
        s = self.lora["alpha"] / self.lora["rank"]
        with torch.no_grad():
            for _, lin in self._lora_linears():
                lin.weight.data.add_(lin.lora_B.data.float() @ lin.lora_A.data.float(), alpha=s)
                del lin.lora_A, lin.lora_B
        named = dict(self.named_parameters())
        for n in self._lora_frozen:
            named[n].requires_grad_(True)
        self._lora_frozen = []
        self.lora = None
        for blk in self.blocks:
            blk.lora_scale = None
        self.refresh_paramstatus()
        self.invalidate_compute_copy()
        self._groups = None  # the flat groups are rebuilt without the adapters
        return self

    # --------------------------------------------------------------------- parameters ----
    def _group_members(self):
        root, blocks = [], [[] for _ in range(self.depth)]
        for n, p in self.named_parameters():
            if n.startswith("blocks."):
                i = int(n.split(".")[1])
                blocks[i].append((n, p))
            else:
                root.append((n, p))
        return root, blocks

    def _ensure_groups(self, device):
        if self._groups is not None and all(g.is_current() and g.device == device for g in self._groups):
            return
        full_values = None
        if self._groups is not None and self._world > 1:
            raise RuntimeError("parameters of a sharded DiT were replaced; re-apply apply_fsdp")
        root, blocks = self._group_members()
        groups = [FlatGroup("root", root, self._world, self._rank, self._pg)]
        groups += [FlatGroup(f"blocks.{i}", m, self._world, self._rank, self._pg) for i, m in enumerate(blocks)]
        self._grad_arena = grad_arena(groups, device)
        off = 0
        for g in groups:
            g.materialize(device, full_values, gfull=self._grad_arena[off:off + g.padded])
            off += g.padded
        self._groups = groups

    def _apply(self, fn, *a, **k):  # .to()/.cuda() replace tensors: flat views are rebuilt lazily
        r = super()._apply(fn, *a, **k)
        if self._world == 1:
            self._groups = None
        return r

    def _adaln_tables(self):
        """device pointer tables (weights, biases, weight gradients, bias gradients) of the blocks' adaLN linears for
        the batched launches; rebuilt when the flat buffers move"""
        key = tuple(g.full.data_ptr() for g in self._groups[1:]) + tuple(g.gfull.data_ptr() for g in self._groups[1:])
        if getattr(self, "_adaln_key", None) != key:
            W = [self.block_group(i).w(f"blocks.{i}.adaLN_modulation.1.weight") for i in range(self.depth)]
            b = [self.block_group(i).w(f"blocks.{i}.adaLN_modulation.1.bias") for i in range(self.depth)]
            gW = [self.block_group(i).g(f"blocks.{i}.adaLN_modulation.1.weight") for i in range(self.depth)]
            gb = [self.block_group(i).g(f"blocks.{i}.adaLN_modulation.1.bias") for i in range(self.depth)]
            self._adaln_tabs = tuple(ops.ptr_table(t) for t in (W, b, gW, gb))
            self._adaln_key = key
        return self._adaln_tabs

    @property
    def root_group(self) -> FlatGroup:
        return self._groups[0]

    def block_group(self, i) -> FlatGroup:
        return self._groups[1 + i]

    def zero_grad(self, set_to_none: bool = True):
        super().zero_grad(set_to_none)

    def _zero_grad_buffers(self):
        """clear the full-size fp32 gradient buffers the weight-gradient kernels accumulate into: ONE fill when the
        groups' buffers are slices of the model's arena (the normal case), else one per group"""
        arena = getattr(self, "_grad_arena", None)
        if arena is not None and all(g.gfull.data_ptr() == arena.data_ptr() + 4 * o for g, o in
                                     zip(self._groups, _offsets(self._groups))):
            arena.zero_()
        else:
            for g in self._groups:
                g.gfull.zero_()

    # ------------------------------------------------------------------------ forward ----
    def forward(self, x, context, timesteps, rope_start: Optional[Tuple[int, int, int]] = None, context_lens=None,
                register_timesteps=None, frame_cache=None, route=None, teacher_latents=None):
        """x [B,C,T,H,W], context [B,Lc,Cc], timesteps [B] -> [B,C,T,H,W] bf16 (model.py:358-402).
        timesteps [B, t], t = T // time_patch_size: one noise level per token-frame (image-to-video, video extension,
        diffusion forcing).  The tokens of frame f of sample b are modulated from timesteps[b, f], the register tokens
        from max_f timesteps[b, f]; constant rows reproduce the [B] call.  bf16 kernels only.
        context_lens: per-sample context lengths -- sample b cross-attends its first context_lens[b] context rows only, 0
        = no context at all (the cross-attention adds nothing for that sample).  A sequence of ints or a CPU integer tensor
        [B] is validated on the host and uploaded once; a CUDA integer tensor [B] is used as it is, without a host sync.
        None (the default, the reference's behaviour): all Lc rows of every sample are attended.
        register_timesteps ([B] tensor or sequence, with timesteps [B, t] only): the noise level the register tokens are
        modulated from, in place of the row maximum.  Pinned, a frame_causal model is causal in the noise levels too: what
        it computes for frame f depends on timesteps[:, :f + 1] and this value alone.  Works with and without grad.  None:
        the row maximum, call for call.
        frame_cache (a FrameKVCache of new_frame_cache; inference on a frame_causal model): x holds only a chunk of k
        token-frames, the ones after the cache's past_frames committed frames; N_REG + k*h*w rows run through the model,
        every block's self-attention reads the committed frames' K / V from the cache and writes the chunk's into it (a
        later frame_cache.commit() makes them part of the past).  timesteps must be [B, k] and rope_start's t component the
        chunk's absolute position (the rollout's base t + past_frames); the chunk's tokens get the RoPE rows they have in the
        table of the whole video of frame_cache.frames frames (FrameKVCache.rope_rows), so the cache must be made for the
        video's full frame count.  Returns [B, C, k*pt, H, W].  The cached K / V are only valid if every call pins the
        same register_timesteps.  With those two, the call computes what the full-sequence call (earlier frames at t = 0,
        later ones at any level) computes for the chunk's frames.
        teacher_latents ([B,C,T,H,W], the clean latents that x is the noised copy of; a frame_causal, frame_major model
        without frame_window; timesteps [B, t]): teacher forcing.  The model runs cat([teacher_latents, x], dim=2) as a
        video of 2t token-frames at the levels [0 ... 0 | timesteps], the registers at register_timesteps (default 1.0 per
        sample, the level the cached rollout pins); token-frame t + f takes the RoPE rows of token-frame f; every
        self-attention runs the teacher mask -- a noisy chunk attends the registers, the CLEAN chunks before it and
        itself -- so that each chunk is computed as generate_latents(rollout_frames=frame_chunk, kv_cache=True) computes it.
        Returns the noisy half, [B,C,T,H,W]; the clean rows get their gradients through K / V.
        route (a model with enable_token_routing): None -- the call is routed iff the model is in training mode and
        gradients are enabled, on a subset drawn from the global CPU RNG after the RoPE offsets (draw_route); False -- the
        full model; sorted, distinct token indices in [0, N) -- this subset (a list or CPU integer tensor is validated on
        the host; a device int32 tensor [k] is used unchecked, make_route).  Anything but None / False on a model without
        token routing: ValueError."""
        if self._route_requested(route):
            self._check_routed_call(timesteps, frame_cache, teacher_latents)
            if route is None:
                route = True  # drawn in _forward, behind the RoPE offsets
        else:
            route = None
        if teacher_latents is not None:
            return self._forward_teacher(x, context, timesteps, rope_start, context_lens, register_timesteps, frame_cache,
                                         teacher_latents)
        return self._forward(x, context, timesteps, rope_start, context_lens, register_timesteps, frame_cache, route=route)

    def _check_routed_call(self, timesteps, frame_cache, teacher_latents):
        """what a routed call refuses (every refusal before the device is touched); enable_token_routing and the other
        switches refuse each other where both are set on the model, these show at the call only"""
        if teacher_latents is not None:
            raise ValueError("DiT: " + _ROUTE_TEACHER)
        if frame_cache is not None:
            raise ValueError("DiT: " + _ROUTE_CACHE)
        if isinstance(timesteps, torch.Tensor) and timesteps.dim() == 2:
            raise ValueError("DiT: " + _ROUTE_FRAME_TIMESTEPS)
        if self.frame_causal:
            raise ValueError("DiT: " + _ROUTE_FRAME_CAUSAL)
        if self.frame_band is not None:
            raise ValueError("DiT: " + _ROUTE_FRAME_BAND)
        if self.fp8:
            raise NotImplementedError("DiT: " + _ROUTE_FP8)
        if self._fsdp is not None or self._world > 1:
            raise NotImplementedError("DiT: " + _ROUTE_FSDP)

    def _forward_teacher(self, x, context, timesteps, rope_start, context_lens, register_timesteps, frame_cache,
                         teacher_latents):
        # every refusal before the device is touched
        if self.frame_band is not None:
            raise ValueError("DiT: teacher_latents is the training form of the cached causal rollout; a frame-band model is "
                             "bidirectional and has neither -- drop teacher_latents (train it with frame_mode=None, "
                             "'first_frame' or 'independent'), or call enable_frame_band(None)")
        if not (self.frame_causal and self.frame_major):
            raise ValueError("DiT: teacher_latents needs the teacher-forcing mask of the frame-major frame-causal "
                             "self-attention -- build the model with frame_causal=True, frame_major=True")
        if self.frame_window is not None:
            raise ValueError(f"DiT: teacher_latents is not built for a frame_window={self.frame_window} model (the ring's "
                             "clean context is a different mask) -- build the model with frame_window=None, or train it "
                             "with frame_mode='chunk'")
        if frame_cache is not None:
            raise ValueError("DiT: teacher_latents and frame_cache exclude each other -- a teacher-forcing call carries its "
                             "clean context in the sequence; pass frame_cache=None (training) or drop teacher_latents "
                             "(the cached rollout)")
        if not isinstance(teacher_latents, torch.Tensor) or tuple(teacher_latents.shape) != tuple(x.shape):
            got = tuple(teacher_latents.shape) if isinstance(teacher_latents, torch.Tensor) else type(teacher_latents).__name__
            raise ValueError(f"DiT: teacher_latents must have x's shape {tuple(x.shape)} (the clean latents of the same "
                             f"frames), got {got}")
        b, T = x.shape[0], x.shape[2]
        t = T // self.time_patch_size
        if not check_timesteps(timesteps, b, t):
            raise ValueError(f"DiT: teacher_latents takes per-frame timesteps of shape [{b}, {t}] (one level per noisy "
                             f"token-frame, equal inside a chunk), got {tuple(timesteps.shape)} -- pass "
                             f"timesteps[:, None].expand({b}, {t})")
        if self.fp8:
            raise NotImplementedError(_FP8_FRAME_TIMESTEPS)
        if register_timesteps is None:
            register_timesteps = torch.ones(b, dtype=f32, device=x.device)
        if rope_start is None and self.use_rope:
            rope_start = self.rope.draw_start((t, x.shape[3] // self.patch_size, x.shape[4] // self.patch_size))
        x2 = torch.cat([teacher_latents.to(x.dtype), x], dim=2)
        ts2 = torch.cat([torch.zeros_like(timesteps), timesteps], dim=1)
        out = self._forward(x2, context, ts2, rope_start, context_lens, register_timesteps, None, teacher=True)
        return out[:, :, T:]

    def _forward(self, x, context, timesteps, rope_start, context_lens, register_timesteps, frame_cache, teacher=False,
                 route=None):
        """route: None (every token runs every block), True (a routed call whose subset is drawn here) or the subset"""
        reg_t = None
        if route is not None and route is not True:  # a host route is checked before anything else happens
            n_tok = ((x.shape[2] // self.time_patch_size) * (x.shape[3] // self.patch_size) * (x.shape[4] // self.patch_size))
            route = self.make_route(route, n_tok, x.device)
        if register_timesteps is not None or frame_cache is not None:  # validated before the device is touched
            b = x.shape[0]
            thw = (x.shape[2] // self.time_patch_size, x.shape[3] // self.patch_size, x.shape[4] // self.patch_size)
            per_frame = check_timesteps(timesteps, b, thw[0])
            if frame_cache is not None:
                self._check_frame_cache(frame_cache, b, thw, per_frame, rope_start)
            if register_timesteps is not None:
                if not per_frame:
                    raise ValueError("DiT: register_timesteps pins the register tokens' noise level of a per-frame call -- "
                                     f"pass timesteps of shape [{b}, {thw[0]}] (one per token-frame), or drop "
                                     "register_timesteps")
                reg_t = torch.as_tensor(register_timesteps).to(device=x.device, dtype=f32)
                if tuple(reg_t.shape) != (b,):
                    raise ValueError(f"DiT: register_timesteps must have shape [{b}] (one per sample), got "
                                     f"{tuple(reg_t.shape)}")
        kv_lens = None
        if context_lens is not None:
            if self.cross_attn_input_size is None:
                raise ValueError("DiT: context_lens given to a model without cross-attention (cross_attn_input_size=None)")
            kv_lens = check_context_lens(context_lens, x.shape[0], context.shape[1])
            if self.fp8 and self.fp8_attn >= 2:
                raise NotImplementedError(_FP8_CONTEXT_LENS)
        if not x.is_cuda:
            raise RuntimeError("video_diffusion_speedrun_amd.DiT runs on the GPU only (no CPU fallback)")
        if not self.use_rope:
            raise AttributeError("'DiT' object has no attribute 'rope': a DiT built with use_rope=False cannot run -- the "
                                 "reference's forward calls self.rope unconditionally (model.py:364) and fails the same "
                                 "way; the model only exists to hold / convert such a checkpoint")
        b, c, t, h, w = x.shape
        thw = (t // self.time_patch_size, h // self.patch_size, w // self.patch_size)
        if check_timesteps(timesteps, b, thw[0]):
            if self.fp8:
                raise NotImplementedError(_FP8_FRAME_TIMESTEPS)
        if rope_start is None:
            rope_start = self.rope.draw_start(thw)
        if not isinstance(rope_start, torch.Tensor):  # a device int32[3] tensor is read by the kernel (graph.py)
            rope_start = tuple(rope_start)
        if route is not None:  # (the draw comes after the RoPE offsets': a seeded run draws both in this order)
            n_tok = thw[0] * thw[1] * thw[2]
            if route is True:
                route = self.make_route(self.draw_route(n_tok), n_tok, x.device)
            if tuple(route.inv.shape) != (N_REG + n_tok,) or not N_REG < route.idx.shape[0] <= N_REG + n_tok:
                raise ValueError(f"DiT: the route's tables are for {route.inv.shape[0] - N_REG} video tokens, this call has "
                                 f"{n_tok} -- build them with make_route(route, {n_tok}, device)")
        self._ensure_groups(x.device)
        params = [p for p in self.parameters() if p.requires_grad]
        need_grad = torch.is_grad_enabled() and len(params) > 0
        if kv_lens is not None:
            kv_lens = kv_lens.to(x.device)
        if need_grad:
            return _DiTFunction.apply(self, x, context, timesteps, rope_start, kv_lens, reg_t, teacher, route, *params)
        out, _ = self._forward_impl(x, context, timesteps, rope_start, save=False, kv_lens=kv_lens, reg_t=reg_t,
                                    cache=frame_cache, teacher=teacher, route=route)
        if frame_cache is not None:
            frame_cache.pending_frames = thw[0]
        return out

    def new_frame_cache(self, batch: int, frames: int, h_tokens: int, w_tokens: int, device=None) -> "FrameKVCache":
        """The K / V store of a cached frame rollout (forward(frame_cache=)): per block, K and V buffers
        [batch, heads, N_REG + frames*h_tokens*w_tokens, padded head dim] bf16 -- the register rows, then the token rows of
        up to `frames` token-frames of h_tokens x w_tokens tokens, in the order the chunks are run.
        A frame_window model gets a ring: N_REG + W*c*h_tokens*w_tokens rows per buffer (W = frame_window // frame_chunk
        slots of one chunk of c = frame_chunk token-frames), whatever `frames` is -- `frames` stays the whole video's length
        (the RoPE table depends on it) and may exceed anything seen in training.  A video longer than the ring (frames >
        W*c) must consist of whole chunks: a short last chunk would leave stale rows of chunk n - W in its slot."""
        if self.frame_band is not None:
            raise ValueError("DiT.new_frame_cache: " + _BAND_NO_CACHE + " -- run it on whole videos "
                             "(generate_latents(kv_cache=False))")
        if not self.frame_causal:
            raise ValueError("DiT.new_frame_cache: a frame KV cache needs a model built with frame_causal=True (on any other "
                             "model the K / V rows of finished frames change with the frames after them)")
        if min(int(batch), int(frames), int(h_tokens), int(w_tokens)) < 1:
            raise ValueError(f"DiT.new_frame_cache: batch, frames, h_tokens, w_tokens must be >= 1, got "
                             f"{(batch, frames, h_tokens, w_tokens)}")
        if device is None:
            device = next(self.parameters()).device
        ring = None
        if self.frame_window is not None:
            c = self.frame_chunk
            ring = (self.frame_window // c, c)
            if int(frames) > self.frame_window and int(frames) % c != 0:
                raise ValueError(f"DiT.new_frame_cache: {frames} token-frames wrap the ring of frame_window="
                                 f"{self.frame_window} frames, and the short last chunk ({int(frames) % c} of {c} frames) "
                                 f"would leave stale rows in its slot -- make the video a whole number of chunks (frames a "
                                 f"multiple of {c}, e.g. {-(-int(frames) // c) * c})")
        return FrameKVCache(self.depth, int(batch), self.num_heads, int(frames), int(h_tokens), int(w_tokens),
                            HDP_OF[self.head_dim], device, ring=ring)

    def _check_frame_cache(self, cache, b, thw, per_frame, rope_start):
        """the conditions of a cached chunk call, each with its remedy (all before the device is touched)"""
        k, h, w = thw
        if self.frame_band is not None:
            raise ValueError("DiT: frame_cache: " + _BAND_NO_CACHE + " -- pass frame_cache=None "
                             "(generate_latents(kv_cache=False))")
        if not isinstance(cache, FrameKVCache):
            raise ValueError("DiT: frame_cache must be a FrameKVCache -- make one with DiT.new_frame_cache(batch, frames, "
                             "h_tokens, w_tokens)")
        if not self.frame_causal:
            raise ValueError("DiT: frame_cache needs a model built with frame_causal=True; run this model without "
                             "frame_cache (generate_latents(kv_cache=False))")
        if torch.is_grad_enabled():
            raise RuntimeError("DiT: frame_cache is inference only (the past layout has no backward kernel) -- call the "
                               "model under torch.no_grad()")
        if self.fp8 and self.fp8_attn:
            raise NotImplementedError("frame_cache is not implemented for the fp8 attention kernels (they have no masked "
                                      "instance): call enable_fp8(attention=False), or enable_fp8(False)")
        if self.fp8:
            raise NotImplementedError(_FP8_FRAME_TIMESTEPS)
        if self._fsdp is not None:
            raise NotImplementedError("frame_cache is not implemented for a model sharded with apply_fsdp: sample from an "
                                      "unsharded copy of the weights (full_state_dict())")
        if not per_frame:
            raise ValueError(f"DiT: a frame_cache call takes per-frame timesteps of shape [{b}, {k}] (one per token-frame of "
                             "the chunk), not [B]")
        if (cache.batch, cache.h_tokens, cache.w_tokens) != (b, h, w) or len(cache.k) != self.depth:
            raise ValueError(f"DiT: frame_cache was made for batch {cache.batch} and {cache.h_tokens} x {cache.w_tokens} "
                             f"tokens per frame, this call has batch {b} and {h} x {w}: make a cache with "
                             f"new_frame_cache({b}, frames, {h}, {w})")
        if cache.past_frames + k > cache.frames:
            raise ValueError(f"DiT: frame_cache holds {cache.frames} token-frames, {cache.past_frames} are committed and this "
                             f"chunk brings {k}: make a larger cache (new_frame_cache(frames=...)) or reset() it")
        if (cache.ring is None) != (self.frame_window is None) or (
                cache.ring is not None and cache.ring != (self.frame_window // self.frame_chunk, self.frame_chunk)):
            raise ValueError("DiT: frame_cache was not made by this model's new_frame_cache -- a frame_window model takes a "
                             "ring cache of its own window and chunk, any other model an unbounded one")
        c = self.frame_chunk
        if self.frame_window is not None and c == 1 and k != 1:
            raise ValueError(f"DiT: a frame_cache call on a frame_window model covers ONE token group -- with frame_chunk=1 "
                             f"that is one token-frame per call, this call brings {k}: pass the frames one at a time "
                             "(generate_latents(rollout_frames=1, kv_cache=True)), or run several frames without "
                             "frame_cache")
        if c > 1 and (cache.past_frames % c != 0 or k > c or (k < c and cache.past_frames + k != cache.frames)):
            raise ValueError(f"DiT: a frame_cache call on a frame_chunk={c} model covers the frames of ONE chunk: "
                             f"{cache.past_frames} frames are committed and this call brings {k} -- commit whole chunks "
                             f"(past_frames % {c} == 0) and pass {c} frames per call, fewer only for the short last chunk "
                             f"of the cache's {cache.frames} frames; several chunks at once run without frame_cache")
        if rope_start is None or isinstance(rope_start, torch.Tensor):
            raise ValueError("DiT: a frame_cache call needs rope_start=(t, h, w) as host ints, t being the chunk's absolute "
                             "position: the rollout's base t + frame_cache.past_frames")
        base_t = int(tuple(rope_start)[0]) - cache.past_frames
        if base_t < 0 or base_t + cache.frames > self.rope.t:
            raise ValueError(f"DiT: rope_start t = {tuple(rope_start)[0]} is the chunk's absolute position (the rollout's "
                             f"base t + past_frames = {cache.past_frames}): it puts the base at {base_t}, and the cache's "
                             f"{cache.frames} frames must lie inside the RoPE table's {self.rope.t} positions -- pass "
                             f"rope_start=(base_t + frame_cache.past_frames, h, w) with 0 <= base_t <= "
                             f"{self.rope.t - cache.frames}")

    def _gather_all(self):
        """bf16 compute copies of every group.  world == 1: one cast kernel per group."""
        if self._fsdp is not None:
            return  # the sharding runtime gathers group by group, overlapped with compute
        for g in self._groups:
            g.gather(ops.cast_f32_bf16, None)

    def _forward_impl(self, x, context, timesteps, rope_start, save: bool, kv_lens=None, reg_t=None, cache=None,
                      teacher=False, route=None):
        D, H, hd = self.hidden_size, self.num_heads, self.head_dim
        pt, p = self.time_patch_size, self.patch_size
        B, C, T, Hh, Ww = x.shape
        t, h, w = T // pt, Hh // p, Ww // p
        N = t * h * w
        L = N + N_REG
        dev = x.device
        fs = self._fsdp
        self._gather_all()
        if fs is not None:
            fs.pre_forward_root()
        R = self.root_group
        x = x.to(bf16).contiguous()
        context = context.to(bf16).contiguous()
        Lc, Cc = context.shape[1], context.shape[2]
        ctx2d = context.view(B * Lc, Cc)
        sv = _Saved() if save else None
        if self.fp8:
            if getattr(self, "_fp8_hist", None) is None or self._fp8_hist.tab.device != dev:
                self._fp8_hist = F8.AmaxHistory(F8.ROWS * self.depth + 1, dev)
            if save:
                self._fp8_hist.ensure_part(B * (t * h * w + N_REG))  # before roll(): see AmaxHistory.ensure_part
                self._fp8_hist.roll()
            # the text context is the same operand for every block's context_kv: quantised once per step
            q_ctx = None
            if self.fp8_lin and self.cross_attn_input_size is not None and F8.supported(B * Lc, 2 * D, Cc):
                q_ctx = F8.Q(ctx2d, F8.E4M3, True, save, self._fp8_hist if save else None, F8.ROWS * self.depth)
            if save:
                sv.q_ctx = q_ctx

        # patch embed + register tokens -> token buffer X [B*L, D]   (model.py:360-362).  ONE GEMM over all B*L rows:
        # the patches are laid out as rows of the token buffer (16 zero rows in front of every sample, whose outputs --
        # the bias -- are then overwritten by the register tokens)
        patches = ops.patchify(x, pt, p, lead_rows=N_REG)
        P = patches.shape[1]
        Wpe = R.w("patch_embed.patch_proj.weight").view(D, P)
        X = ops.linear_fwd(patches, Wpe, R.w("patch_embed.patch_proj.bias"))
        ops.fill_registers(R.w("register_tokens").view(N_REG, D), X, L * D, B, N_REG, D)
        if cache is not None:
            cos, sin = cache.rope_rows(self.rope, rope_start, t)
        elif teacher:
            # token-frame t/2 + f takes the rows of token-frame f: the table of (t/2, h, w), its token rows ((h w t) order, t
            # fastest) taken twice along t
            def twice(tab):
                tok = tab[N_REG:].view(h * w, t // 2, -1)
                return torch.cat([tab[:N_REG], torch.cat([tok, tok], dim=1).reshape(N, -1)], dim=0).contiguous()
            cos, sin = (twice(tab) for tab in self.rope.rows((t // 2, h, w), rope_start, N_REG))
        else:
            cos, sin = self.rope.rows((t, h, w), rope_start, N_REG)

        # timestep conditioning (model.py:374-377), kept in fp32
        # per-frame timesteps [B, t]: the conditioning path runs on B*G rows, G = 1 + t modulation groups per sample --
        # group 0 (the register rows) on the sample's noisiest frame, group 1 + f (the rows of token-frame f: the token
        # order is (h w t), t fastest) on timesteps[b, f] -- and every modulated kernel looks its row up per group
        # [B] and [B, t] timesteps alike; a frame-band model (enable_frame_band) derives it from the latent shape too
        frames = (N_REG, t) if (self.frame_causal or self.frame_band is not None) else None
        if teacher:
            frames = TeacherFrames(frames)  # (the blocks' self-attention: the teacher mask over t/2 clean + t/2 noisy frames)
        groups = None
        if timesteps.dim() == 2:
            groups = (N_REG, t)
            tf = timesteps.to(f32)
            lead_t = tf.max(dim=1, keepdim=True).values if reg_t is None else reg_t.view(B, 1)
            timesteps = torch.cat([lead_t, tf], dim=1).reshape(B * (1 + t))
        temb = ops.timestep_embedding(timesteps.to(f32).contiguous(), D)
        h1 = ops.small_linear_fwd(temb, R.w("time_embed.0.weight"), R.w("time_embed.0.bias"), 0)
        cvec = ops.small_linear_fwd(h1, R.w("time_embed.2.weight"), R.w("time_embed.2.bias"), 1)
        if save:
            sv.patches, sv.temb, sv.h1, sv.cvec, sv.cos, sv.sin = patches, temb, h1, cvec, cos, sin
            sv.dims = (B, C, T, Hh, Ww, t, h, w, N, L, Lc, Cc)
            sv.ctx2d = ctx2d
            sv.kv_lens = kv_lens
            sv.groups = groups
            sv.frames = frames
            sv.blocks = []

        # adaLN modulation of every block in ONE launch (K4 of SURVEY 2.3): all blocks read the same conditioning vector.
        # Not under sharding -- it would need every group's gathered weights before block 0 -- nor beyond 16 samples.
        mods = None
        # Nor with per-frame timesteps: B*G modulation rows exceed the launch's 16 at every real shape, so such a call
        # always takes the per-block linears (any number of rows; what sharded models run) -- one path to test.
        if fs is None and groups is None and B <= 16 and self.depth > 1 and os.environ.get("VDS_ADALN_BATCH", "1") != "0":
            wt, bt, _, _ = self._adaln_tables()
            mods = ops.small_linear_fwd_batched(cvec, wt, bt, self.depth, 9 * D, 1)
        v0 = None
        past = cache.past_frames * h * w if cache is not None else 0
        ring_call = cache.ring_call(t) if (cache is not None and cache.ring is not None) else None
        keep = self.recompute if (save and self.recompute != "none") else None  # blocks keep their inputs, not their work
        # token routing (a TokenRoute): the blocks r_first .. r_last run the block code at Ls = N_REG + k rows -- the
        # registers and the kept tokens, gathered with residual-V's v_0 rows and the RoPE rows -- and the result goes back
        # to its rows of the full buffer, whose other rows still hold what they held before block r_first
        r_first, r_last = self.token_routing[:2] if route is not None else (self.depth, -1)
        X_full = routed_in = None
        for i in range(self.depth):
            if fs is not None:
                fs.pre_forward_block(i)
            if i == r_first:
                Ls = route.idx.shape[0]
                X_full = X
                routed_in = (ops.rows_gather(v0, route.idx) if v0 is not None and self.residual_v else None,
                             ops.rows_gather(cos, route.idx), ops.rows_gather(sin, route.idx), Ls)
                X = ops.rows_gather(X.view(B, L, D), route.idx).view(B * Ls, D)
            v0_i, cos_i, sin_i, L_i = routed_in if r_first <= i <= r_last else (v0, cos, sin, L)
            X, v, bs = self.blocks[i]._fwd(self.block_group(i), f"blocks.{i}.", X, ctx2d, cvec, v0_i, cos_i, sin_i, B, L_i, Lc,
                                           save and keep is None,
                                           (self._fp8_hist, i, self.fp8_attn, self.fp8_lin, q_ctx) if self.fp8 else None,
                                           mods[i] if mods is not None else None, keep=keep, kv_lens=kv_lens,
                                           groups=groups, frames=frames,
                                           **({} if cache is None else {"cache": (cache.k[i], cache.v[i], past)}
                                              if ring_call is None else {"cache": (cache.k[i], cache.v[i]) + ring_call}))
            if v0 is None:
                v0 = v
            if i == r_last:  # in place: nothing keeps the full buffer (block r_first kept its gathered input)
                X = ops.rows_merge(X_full.view(B, L, D), X.view(B, L_i, D), route.inv).view(B * L, D)
                X_full = None
            if save:
                sv.blocks.append(bs)
            if fs is not None:
                fs.post_forward_block(i)
        if save:
            # (the backward and its recompute replay read v_0 / cos / sin at Ls rows: routed_in stays alive)
            sv.route, sv.route_span, sv.routed_in = route, (r_first, r_last), routed_in
            sv.v0 = v0
            sv.x_last = X
            sv.batched_adaln = mods is not None
            sv.recompute = keep is not None

        # final layer (model.py:386-401)
        fmod = ops.small_linear_fwd(cvec, R.w("final_modulation.1.weight"), R.w("final_modulation.1.bias"), 1)
        wfn = R.w("final_norm.weight") if R.has("final_norm.weight") else None
        # norm, modulation and projection run over all B*L rows (the 16 register rows of a sample are 0.2 % of them and
        # are simply not read back: the reference slices them off first, model.py:386); unpatchify picks the token rows
        xnf, rstdf = _norm_fwd(groups, X, wfn, fmod, 0, D, B, L)
        yf = ops.linear_fwd(xnf, R.w("final_proj.weight"), R.w("final_proj.bias"))
        out = ops.unpatchify(yf, B, C, T, Hh, Ww, pt, p, lead_rows=N_REG)
        if save:
            sv.fmod, sv.xnf, sv.rstdf = fmod, xnf, rstdf
        if fs is not None:
            fs.post_forward_root()
        return out, sv

    # ----------------------------------------------------------------------- backward ----
    def _backward_impl(self, sv: _Saved, dout: torch.Tensor):
        D, H, hd = self.hidden_size, self.num_heads, self.head_dim
        pt, p = self.time_patch_size, self.patch_size
        B, C, T, Hh, Ww, t, h, w, N, L, Lc, Cc = sv.dims
        dev = dout.device
        fs = self._fsdp
        R = self.root_group
        groups = sv.groups
        Bc = sv.cvec.shape[0]  # rows of the conditioning path: B, or B*G with per-frame timesteps
        # gradients already held in p.grad (a second backward before zero_grad: micro-batch accumulation, like
        # autograd's accumulate-into-.grad in the reference loop) are set aside and added back at the end
        held = [g.hold_grads() for g in self._groups]  # per parameter: only slices whose .grad is live are kept
        self._zero_grad_buffers()
        if fs is not None:
            fs.pre_backward_root()
        Pd = p * p * pt * C
        dout = dout.to(bf16).contiguous()
        # final layer
        dyf = ops.unpatchify_bwd(dout, pt, p, lead_rows=N_REG)  # [B*L, P], register rows zero
        Tr = lambda n: R.params[n].requires_grad  # frozen parameters skip their weight-gradient GEMM / column sums
        if Tr("final_proj.weight"):
            ops.linear_wgrad(dyf, sv.xnf, R.g("final_proj.weight"))
        if Tr("final_proj.bias"):
            ops.colsum(dyf, R.g("final_proj.bias"))
        dxnf = ops.linear_dgrad(dyf, R.w("final_proj.weight"))
        # the small zero-initialised accumulators of this pass come out of ONE fill: d(final modulation) [B, 2D],
        # d(conditioning vector) [B, D], d(time-embed hidden) [B, 4D] and the adaLN modulation gradients of all blocks
        nmods = self.depth * Bc * 9 * D if sv.batched_adaln else 0
        zs = torch.zeros(Bc * 7 * D + nmods, dtype=f32, device=dev)
        dfmod, dc, dh1 = (zs[:Bc * 2 * D].view(Bc, 2 * D), zs[Bc * 2 * D:Bc * 3 * D].view(Bc, D),
                          zs[Bc * 3 * D:Bc * 7 * D].view(Bc, 4 * D))
        dmods = zs[Bc * 7 * D:].view(self.depth, Bc, 9 * D) if sv.batched_adaln else None
        wfn = R.w("final_norm.weight") if R.has("final_norm.weight") else None
        dwfn = R.g("final_norm.weight") if wfn is not None else None
        # register rows: dxnf = 0 there, so they get a zero gradient from the final layer (they were sliced off)
        dX = _norm_bwd(groups, dxnf, sv.x_last, wfn, sv.fmod, 0, D, sv.rstdf, None, dfmod, dwfn, B, L)
        ops.small_linear_bwd(dfmod, sv.cvec, R.w("final_modulation.1.weight"), R.g("final_modulation.1.weight"),
                             R.g("final_modulation.1.bias"), dc, 1)
        hdp = HDP_OF[hd]
        dv0 = torch.zeros(B, H, L, hdp, dtype=f32, device=dev) if (self.residual_v and self.depth > 1) else None
        sv.dv_terms = [] if (_DV0_DEFER and dv0 is not None) else None
        # one bf16 lambda per deferred block, copied when the block defers: only where the runtime releases a block's
        # gathered weights before the deferred reduction reads them (resident and unsharded weights stay where they are)
        snap = sv.dv_terms is not None and fs is not None and fs.releases_params
        sv.lam_snap, sv.lam_used = (torch.empty(self.depth, dtype=bf16, device=dev) if snap else None), 0
        # token routing: the blocks r_first .. r_last ran at Ls rows.  Their backward runs on a routed view of sv -- the
        # gathered v_0 / cos / sin, its OWN list of deferred dv terms and its own dv0_started flag (the full-length terms
        # pending in sv.dv_terms are of another length and stay pending across the span) -- and on an accumulator dv0_r of
        # Ls rows.  The rows that skipped the span keep the gradient from behind it (dX_full); the routed rows take the
        # span's input gradient.
        route = getattr(sv, "route", None)
        r_first, r_last = sv.route_span
        rv = dX_full = dv0_r = None
        for i in reversed(range(self.depth)):
            if fs is not None:
                fs.pre_backward_block(i)
            bs = sv.blocks[i]
            routed = r_first <= i <= r_last
            if i == r_last:
                rv = _Saved()
                rv.v0, rv.cos, rv.sin, Ls = sv.routed_in
                rv.ctx2d, rv.cvec, rv.kv_lens = sv.ctx2d, sv.cvec, sv.kv_lens
                rv.dv_terms = [] if sv.dv_terms is not None else None
                rv.dv0_started = False
                dv0_r = torch.zeros(B, H, Ls, hdp, dtype=f32, device=dev) if dv0 is not None else None
                dX_full = dX
                dX = ops.rows_gather(dX.view(B, L, D), route.idx).view(B * Ls, D)
            sv_i, dv0_i, L_i = (rv, dv0_r, Ls) if routed else (sv, dv0, L)
            if sv.recompute:
                # replay: the block's forward kernels once more, on its kept input and the same conditioning / RoPE rows /
                # block-0 v (sv.v0 stays the v handed out in the first forward; block 0 makes its own copy again); a routed
                # block on the routed view's rows
                _, _, bs = self.blocks[i]._fwd(self.block_group(i), f"blocks.{i}.", bs.X, sv.ctx2d, sv.cvec,
                                               sv_i.v0 if i > 0 else None, sv_i.cos, sv_i.sin, B, L_i, Lc, True, None, bs.mod,
                                               replay=bs, kv_lens=sv.kv_lens, groups=groups, frames=sv.frames)
            dX = self.blocks[i]._bwd(self.block_group(i), f"blocks.{i}.", bs, dX, sv_i, dc, dv0_i, B, L_i, Lc,
                                     i == 0, (self._fp8_hist, i, self.fp8_attn, self.fp8_lin, sv.q_ctx) if self.fp8 else None,
                                     dmods[i] if dmods is not None else None, groups=groups)
            sv.blocks[i] = bs = None
            if i == r_first:
                if dv0 is not None:
                    if rv.dv_terms:  # what the span's last chunk left
                        ops.dv0_reduce([t for t, _ in rv.dv_terms], [l for _, l in rv.dv_terms], dv0_r, B, H, Ls, hd, hdp,
                                       accumulate=rv.dv0_started)
                        rv.dv_terms.clear()
                    ops.rows_scatter_add(dv0_r, dv0, route.idx)
                    # dv0 now holds the span's share: the first full-length reduction behind it must ADD to it
                    # (DiTBlock._bwd overwrites while sv.dv0_started is unset)
                    sv.dv0_started = True
                dX = ops.rows_merge(dX_full.view(B, L, D), dX.view(B, Ls, D), route.inv).view(B * L, D)
                rv = dX_full = dv0_r = None
            if fs is not None:
                fs.post_backward_block(i)
        if dmods is not None:  # adaLN weight / bias gradients of all blocks and their fan-in to dc: one launch each
            wt, _, gwt, gbt = self._adaln_tables()
            ops.small_linear_bwd_batched(dmods, sv.cvec, wt, gwt, gbt, dc, 1)
        # registers + patch embed (model.py:360-362)
        ops.registers_bwd(dX, L * D, R.g("register_tokens").view(N_REG, D), B, N_REG, D)
        # patch embedding: weight gradient over all B*L rows (the register rows of `patches` are zero), bias gradient
        # over the token rows only
        if Tr("patch_embed.patch_proj.weight"):
            ops.linear_wgrad(dX, sv.patches, R.g("patch_embed.patch_proj.weight").view(D, Pd))
        if Tr("patch_embed.patch_proj.bias"):
            ops.colsum(dX, R.g("patch_embed.patch_proj.bias"), rows_per_sample=L, row_offset=N_REG)
        # time embed MLP
        ops.small_linear_bwd(dc, sv.h1, R.w("time_embed.2.weight"), R.g("time_embed.2.weight"),
                             R.g("time_embed.2.bias"), dh1, 1)
        ops.small_linear_bwd(dh1, sv.temb, None, R.g("time_embed.0.weight"), R.g("time_embed.0.bias"), None, 0)
        if fs is not None:
            fs.post_backward_root()
        else:
            for g in self._groups:
                g.publish_grads()
        for g, h in zip(self._groups, held):
            g.add_held(h)
        if self.fp8 and getattr(self, "_fp8_hist", None) is not None:
            self._fp8_hist.backward_done()

    # ------------------------------------------------------------------- muP table ----
    def get_mup_setup(self, learning_rate, weight_decay, constant_param_classes):
        """muP-style per-parameter (lr, weight decay) table; same contract as the reference
        (model.py:404-465): returns (optimizer param groups -- one per distinct (lr, wd) pair, in first-use
        order --, {name: {"lr", "wd", "shape"}}).  The cascade, later stages overriding earlier ones:
          1. vectors / scalars (name has bias | norm | lambda): lr/100, no decay; matrices: lr * 32/fan_in and
             wd * fan_in/1024, fan_in = last dim of the FULL tensor shape;
          2. names containing one of `constant_param_classes`: lr/100, no decay;
          3. names containing "time", then "modulation": lr/10 (decay untouched)."""
        table, buckets = {}, {}
        for name, p in self.named_parameters():
            name = name.replace("_fsdp_wrapped_module.", "")  # the prefix the reference strips (model.py:417)
            info = self.paramstatus[name]
            if not info["requires_grad"]:
                continue
            fan_in = info["shape"][-1]
            if "bias" in name or "norm" in name or "lambda" in name:
                lr, wd = learning_rate * 0.01, 0.0
            else:
                lr, wd = learning_rate * (32 / fan_in), weight_decay * fan_in / 1024
            if any(c in name for c in constant_param_classes):
                lr, wd = learning_rate * 0.01, 0.0
            for tag in ("time", "modulation"):
                if tag in name:
                    lr = learning_rate * 0.1
            bucket = buckets.setdefault((lr, wd), {"params": [], "weight_decay": wd, "lr": lr})
            bucket["params"].append(p)
            table[name] = {"lr": lr, "wd": wd, "shape": info["shape"]}
        return list(buckets.values()), table

    # Muon: which parameters of a DiTBlock it manages (name suffix -> how many row slices the tensor is made of)
    MUON_MATRICES = {"qkv.weight": 3, "attn_proj.weight": 1, "q_cross.weight": 1, "context_kv.weight": 2,
                     "cross_proj.weight": 1, "mlp.0.weight": 1, "mlp.2.weight": 1}

    def get_muon_setup(self, learning_rate, weight_decay, constant_param_classes, muon_lr=0.02, muon_weight_decay=0.0,
                       momentum=0.95, nesterov=True, ns_steps=5):
        """`get_mup_setup` for `optim.MuonAdamW`: the 2-D matrices of every DiTBlock -- qkv (three row slices: q, k, v
        are orthogonalised separately), attn_proj, q_cross, context_kv (two slices), cross_proj and the two MLP weights
        -- leave the AdamW groups and form Muon groups (`use_muon=True`, `muon_split` = 1 | 2 | 3, lr `muon_lr`,
        `weight_decay` `muon_weight_decay`, plus `momentum`, `nesterov`, `ns_steps`); biases, norms, lambda_param, the
        adaLN modulation, patch embedding, timestep MLP, registers and the final layer keep exactly the (lr, wd) of
        `get_mup_setup`.  Returns (groups, table); Muon entries of the table carry "muon": True and "split"."""
        if not float(muon_lr) > 0.0:
            raise ValueError(f"get_muon_setup: muon_lr must be > 0, got {muon_lr}")
        if not float(muon_weight_decay) >= 0.0:
            raise ValueError(f"get_muon_setup: muon_weight_decay must be >= 0, got {muon_weight_decay}")
        if not 0.0 <= float(momentum) < 1.0:
            raise ValueError(f"get_muon_setup: momentum must be in [0, 1), got {momentum}")
        if int(ns_steps) != ns_steps or not 0 <= ns_steps <= 64:
            raise ValueError(f"get_muon_setup: ns_steps must be an integer in [0, 64], got {ns_steps}")
        groups, table = self.get_mup_setup(learning_rate, weight_decay, constant_param_classes)
        split_of = {}
        for name, p in self.named_parameters():
            name = name.replace("_fsdp_wrapped_module.", "")
            if name not in table or not name.startswith("blocks."):
                continue
            suffix = name.split(".", 2)[2]
            if suffix in self.MUON_MATRICES:
                split_of[id(p)] = (self.MUON_MATRICES[suffix], name, p)
        out = []
        for g in groups:
            keep = [p for p in g["params"] if id(p) not in split_of]
            if keep:
                out.append(dict(g, params=keep))
        for split in (1, 2, 3):
            ps = [p for s_, _, p in split_of.values() if s_ == split]
            if ps:
                out.append({"params": ps, "lr": float(muon_lr), "weight_decay": float(muon_weight_decay),
                            "use_muon": True, "muon_split": split, "momentum": float(momentum),
                            "nesterov": bool(nesterov), "ns_steps": int(ns_steps)})
        for split, name, _ in split_of.values():
            table[name] = {"lr": float(muon_lr), "wd": float(muon_weight_decay), "shape": table[name]["shape"],
                           "muon": True, "split": split}
        return out, table

    # --------------------------------------------------------------- state / copies ----
    def invalidate_compute_copy(self):
        """Force the next forward to re-cast the fp32 masters into the bf16 compute copies.  In-place writes
        through the nn.Parameters are detected by themselves (FlatGroup.mark_shadow_fresh); call this after
        writing parameter memory some other way (`p.data.xxx_()`, raw pointers, custom kernels)."""
        for g in self._groups or []:
            g.invalidate_shadow()
        # fp8: the weights' delayed-scaling history describes the OLD values (a larger checkpoint would be clipped at the
        # old amax for a step): re-measure everything on the next step
        if getattr(self, "_fp8_hist", None) is not None:
            self._fp8_hist.reset()

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        r = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self.invalidate_compute_copy()
        return r

    def full_state_dict(self) -> Dict[str, torch.Tensor]:
        """fp32 full tensors keyed like the reference state dict (one all-gather per group when sharded)."""
        if self._groups is None:
            return {k: v.detach().clone() for k, v in self.state_dict().items()}
        out = {}
        for g in self._groups:
            out.update(g.full_tensors())
        return out


class _BlockFunction(torch.autograd.Function):
    """DiTBlock.forward as one autograd node (see DiTBlock.forward for the contract)."""

    @staticmethod
    def forward(ctx, block, need, x, context, c, v_0, cos, sin, kv_lens, frames, *params):
        B, L, D = x.shape
        H, hd = block.num_heads, block.head_dim
        hdp = HDP_OF[hd]
        dev = x.device
        if (context is None) != (block.q_cross is None):
            raise ValueError("DiTBlock: `context` must be given exactly when the block has cross-attention")
        G, pre = block._group_and_prefix(dev)
        G.gather(ops.cast_f32_bf16, None)
        X = x.reshape(B * L, D).to(bf16).contiguous()
        if context is not None:
            Lc = context.shape[1]
            ctx2d = context.to(bf16).contiguous().view(B * Lc, context.shape[2])
        else:
            Lc, ctx2d = 0, None
        cvec = c.to(f32).contiguous()
        if cos is None:  # rope=None: no rotation (model.py:132-134) = the identity rotation
            cos2 = torch.ones(L, hd // 2, dtype=f32, device=dev)
            sin2 = torch.zeros(L, hd // 2, dtype=f32, device=dev)
        else:
            cos2 = cos.reshape(L, hd // 2).to(f32).contiguous()
            sin2 = sin.reshape(L, hd // 2).to(f32).contiguous()
        v0p = None
        if v_0 is not None and block.residual_v:
            if tuple(v_0.shape) != (B, H, L, hd):
                raise ValueError(f"DiTBlock: v_0 must be [B,H,L,hd] = {(B, H, L, hd)}, got {tuple(v_0.shape)}")
            if v_0.dtype == bf16 and v_0.stride() == (H * L * hdp, L * hdp, hdp, 1):
                v0p = v_0.as_strided((B, H, L, hdp), (H * L * hdp, L * hdp, hdp, 1))  # a `v` this class returned
            else:
                v0p = torch.zeros(B, H, L, hdp, dtype=bf16, device=dev)
                v0p[..., :hd].copy_(v_0)
        Xo, v, bs = block._fwd(G, pre, X, ctx2d, cvec, v0p, cos2, sin2, B, L, Lc, need, kv_lens=kv_lens, frames=frames)
        if need:
            sv = _Saved()
            sv.cos, sv.sin, sv.v0, sv.ctx2d, sv.cvec, sv.kv_lens = cos2, sin2, v0p, ctx2d, cvec, kv_lens
            ctx.state = (block, G, pre, bs, sv, (B, L, Lc, D, H, hd, hdp), x.dtype, c.dtype,
                         v_0.dtype if v_0 is not None else None)
        ctx.set_materialize_grads(False)
        return Xo.view(B, L, D), v[..., :hd]

    @staticmethod
    def backward(ctx, dx, dv_out):
        block, G, pre, bs, sv, (B, L, Lc, D, H, hd, hdp), xdt, cdt, v0dt = ctx.state
        ctx.state = None
        dev = sv.cvec.device
        held = G.hold_grads()  # accumulate like autograd (see DiT._backward_impl)
        G.gfull.zero_()
        dX = (dx.reshape(B * L, D).to(bf16).contiguous() if dx is not None
              else torch.zeros(B * L, D, dtype=bf16, device=dev))
        dc = torch.zeros(B, D, dtype=f32, device=dev)
        dv0 = None
        if bs.mix:
            if dv_out is not None:
                raise NotImplementedError("DiTBlock: a gradient through the returned (lambda-mixed) v of a block "
                                          "that was given v_0 is not implemented; the model only consumes block 0's v")
            dv0 = torch.zeros(B, H, L, hdp, dtype=f32, device=dev)
        elif dv_out is not None:
            dv0 = torch.zeros(B, H, L, hdp, dtype=f32, device=dev)
            dv0[..., :hd].copy_(dv_out)
        dX0 = block._bwd(G, pre, bs, dX, sv, dc, dv0, B, L, Lc, first=(not bs.mix and dv0 is not None))
        G.publish_grads()
        G.add_held(held)
        gv0 = dv0[..., :hd].to(v0dt) if (bs.mix and v0dt is not None) else None
        n_params = len(list(block.parameters()))
        return (None, None, dX0.view(B, L, D).to(xdt), None, dc.to(cdt), gv0, None, None, None, None) + (None,) * n_params


class _DiTFunction(torch.autograd.Function):
    """One autograd node for the whole model: forward/backward are explicit kernel sequences;
    parameter gradients are written into the flat fp32 gradient buffers that p.grad aliases."""

    @staticmethod
    def forward(ctx, model, x, context, timesteps, rope_start, kv_lens, reg_t, teacher, route, *params):
        out, sv = model._forward_impl(x, context, timesteps, rope_start, save=True, kv_lens=kv_lens, reg_t=reg_t,
                                      teacher=teacher, route=route)
        ctx.model, ctx.sv = model, sv
        return out

    @staticmethod
    def backward(ctx, dout):
        model, sv = ctx.model, ctx.sv
        ctx.sv = None
        model._backward_impl(sv, dout)
        return (None,) * (9 + len([p for p in model.parameters() if p.requires_grad]))
