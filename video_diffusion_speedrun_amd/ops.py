"""Tensor-level wrappers over the C ABI (include/vds.h).  torch is used for device memory and
the current HIP stream only; every computation below is a hand-written gfx950 kernel.

All tensors must live on the GPU; bf16 activations are torch.bfloat16, statistics / modulation
/ gradients of parameters are torch.float32.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import (EPI_BIAS_GELU, EPI_DGELU, EPI_F32, EPI_GATE_RES, EPI_STORE, VDS_NN, VDS_NT, VDS_TN,
                   AttnArgs, GemmArgs, check)

bf16 = torch.bfloat16
f32 = torch.float32


# private torch entry point (resolved once; a torch version without it falls back to the public, slower form)
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """raw handle of torch's current HIP stream.  (`torch.cuda.current_stream().cuda_stream` builds a Stream object per
    call: 2.65 us against 0.3 us for this form -- a third of the host cost of a small launch, and launch-bound
    workloads (C1: ~1600 launches of a few microseconds per step) are host-bound; tools/bench_host_overhead.py)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    assert t.is_cuda, "vds ops need GPU tensors (no CPU fallback)"
    return t.data_ptr()


def _rows(t: torch.Tensor) -> Tuple[int, int]:
    """(ld, cols) of a 2-D row-major view whose last dim is contiguous."""
    assert t.dim() == 2 and t.stride(1) == 1, (t.shape, t.stride())
    return t.stride(0), t.shape[1]


# ------------------------------------------------------------------------------- GEMM ----
def _gemm_args(layout: int, epi: int, M: int, N: int, K: int, A, lda, B, ldb, Cp=None, ldc=0, C2=None, ldc2=0, bias=None,
               aux=None, ldaux=0, gate=None, ldgate=0, rows_per_batch=0, split_k=1, colsum=None):
    """vds_gemm_args (by reference) from tensors and leading dimensions: the one place that knows the field order"""
    return C.byref(GemmArgs(layout, epi, M, N, K, _p(A), lda, _p(B), ldb, _p(Cp), ldc, _p(C2), ldc2, _p(bias), _p(aux),
                            ldaux, _p(gate), ldgate, rows_per_batch, split_k, _p(colsum)))


def gemm(layout: int, epi: int, M: int, N: int, K: int, A, lda, B, ldb, Cp=None, ldc=0, C2=None, ldc2=0,
         bias=None, aux=None, ldaux=0, gate=None, ldgate=0, rows_per_batch=0, split_k=1, colsum=None):
    a = _gemm_args(layout, epi, M, N, K, A, lda, B, ldb, Cp, ldc, C2, ldc2, bias, aux, ldaux, gate, ldgate, rows_per_batch,
                   split_k, colsum)
    check(_lib.load().vds_gemm_bf16(a, _stream()), f"vds_gemm_bf16(layout={layout},epi={epi},M={M},N={N},K={K})")


def gemm_force_tile(tile: int) -> int:
    """tests / experiments: pin the GEMM tiling (0 auto, 128, 256, 2 = 256x128); returns the previous setting"""
    prev = _lib.load().vds_gemm_force_tile(int(tile))
    if prev < 0:
        raise ValueError(f"vds_gemm_force_tile({tile}): not a tiling")
    return prev


def knob_set(name: str, value: float) -> float:
    """set one entry of the library's knob table (csrc/config.h); returns the previous value"""
    lib = _lib.load()
    prev = lib.vds_knob_get(name.encode())
    check(lib.vds_knob_set(name.encode(), float(value)), f"vds_knob_set({name})")
    return prev


def knob_get(name: str) -> float:
    v = _lib.load().vds_knob_get(name.encode())
    if v != v:
        raise KeyError(name)
    return v


_det_ws = [None]


def is_deterministic() -> bool:
    return _det_ws[0] is not None


def set_deterministic(on: bool, workspace_bytes: int = 1 << 30, device="cuda") -> bool:
    """fixed-order reductions in every backward kernel (include/vds.h: vds_set_deterministic); the workspace for the
    partial results is a torch allocation this module keeps alive while the mode is on.  Returns the previous mode."""
    lib = _lib.load()
    if on:
        ws = torch.empty(int(workspace_bytes), dtype=torch.uint8, device=device)
        prev = lib.vds_set_deterministic(1, ws.data_ptr(), ws.numel())
        if prev < 0:  # rejected: the library's mode and workspace are what they were, and so is is_deterministic()
            raise ValueError("vds_set_deterministic")
        _det_ws[0] = ws
    else:
        torch.cuda.synchronize()
        prev = lib.vds_set_deterministic(0, None, 0)
        if prev < 0:
            raise ValueError("vds_set_deterministic")
        _det_ws[0] = None
    return bool(prev)


def linear_fwd(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x W^T + b.  x [M,K] bf16, W [N,K] bf16 -> y [M,N] bf16."""
    M, K = x.shape
    N = W.shape[0]
    y = out if out is not None else torch.empty(M, N, dtype=bf16, device=x.device)
    gemm(VDS_NT, EPI_STORE, M, N, K, x, x.stride(0), W, W.stride(0), y, y.stride(0), bias=bias)
    return y


def linear_fwd_gelu(x, W, bias, want_pre: bool = True):
    """(pre, act) = (x W^T + b, gelu_erf(pre))   (model.py:84-85).  want_pre=False: only `act` is stored (a forward
    that keeps nothing for a backward); `pre` comes back as None and `act` has the same bits."""
    M, K = x.shape
    N = W.shape[0]
    pre = torch.empty(M, N, dtype=bf16, device=x.device) if want_pre else None
    act = torch.empty(M, N, dtype=bf16, device=x.device)
    gemm(VDS_NT, EPI_BIAS_GELU, M, N, K, x, x.stride(0), W, W.stride(0), pre, N, act, N, bias=bias)
    return pre, act


def linear_fwd_gate_res(x, W, bias, mod, gate_col: int, res, rows_per_batch: int, want_y: bool = True):
    """y = x W^T + b ; x_new = res + y * gate[b]  (model.py:138-139,159-160,165).
    mod: f32 [B, 9D] modulation table, gate at column gate_col.  want_y=False: only `x_new` is stored (`y` is read by
    the backward pass alone); `y` comes back as None and `x_new` has the same bits."""
    M, K = x.shape
    N = W.shape[0]
    y = torch.empty(M, N, dtype=bf16, device=x.device) if want_y else None
    xn = torch.empty(M, N, dtype=bf16, device=x.device)
    gate = mod[:, gate_col:]
    gemm(VDS_NT, EPI_GATE_RES, M, N, K, x, x.stride(0), W, W.stride(0), y, N, xn, N, bias=bias, aux=res,
         ldaux=res.stride(0), gate=gate, ldgate=mod.stride(0), rows_per_batch=rows_per_batch)
    return y, xn


def linear_fwd_gate_res_grouped(x, W, bias, mod, gate_col: int, res, L: int, groups, want_y: bool = True):
    """linear_fwd_gate_res with one gate row per modulation group: mod f32 [B*G, 9D], `groups` = (lead, period), L rows
    per sample; output row r takes the gate row of its group (vds_gemm_bf16_grouped)"""
    M, K = x.shape
    N = W.shape[0]
    y = torch.empty(M, N, dtype=bf16, device=x.device) if want_y else None
    xn = torch.empty(M, N, dtype=bf16, device=x.device)
    gate = mod[:, gate_col:]
    a = _gemm_args(VDS_NT, EPI_GATE_RES, M, N, K, x, x.stride(0), W, W.stride(0), y, N, xn, N, bias=bias, aux=res,
                   ldaux=res.stride(0), gate=gate, ldgate=mod.stride(0), rows_per_batch=L)
    check(_lib.load().vds_gemm_bf16_grouped(a, _groups(groups, L, mod, M // L), _stream()),
          f"vds_gemm_bf16_grouped(M={M},N={N},K={K},L={L},groups={tuple(groups)})")
    return y, xn


def linear_dgrad(dy, W, pre: Optional[torch.Tensor] = None, colsum: Optional[torch.Tensor] = None):
    """dx = dy W  (dy [M,N], W [N,K] -> [M,K]); with `pre`: dx *= gelu'(pre) (fused), and then optionally
    colsum[k] += sum_m dx[m,k] (f32; the bias gradient of the layer whose pre-activation `pre` is)."""
    M, N = dy.shape
    K = W.shape[1]
    dx = torch.empty(M, K, dtype=bf16, device=dy.device)
    if pre is None:
        assert colsum is None
        gemm(VDS_NN, EPI_STORE, M, K, N, dy, dy.stride(0), W, W.stride(0), dx, K)
    else:
        gemm(VDS_NN, EPI_DGELU, M, K, N, dy, dy.stride(0), W, W.stride(0), dx, K, aux=pre, ldaux=pre.stride(0),
             colsum=colsum)
    return dx


# --------------------------------------------------------------------------- fp8 GEMM ----
FP8_E4M3, FP8_E5M2 = 0, 1
fp8_dtypes = (torch.float8_e4m3fn, torch.float8_e5m2)


def absmax(x: torch.Tensor, amax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """amax[0] = max |x| of a bf16 matrix (f32 device scalar; accumulates into `amax` when given)."""
    ld, K = _rows(x)
    if amax is None:
        amax = torch.zeros(1, dtype=f32, device=x.device)
    check(_lib.load().vds_absmax(_p(x), ld, x.shape[0], K, _p(amax), _stream()), "vds_absmax")
    return amax


def quant_fp8(x: torch.Tensor, fmt: int, amax: torch.Tensor, rowmajor: bool = True, transposed: bool = False,
              amax_out: Optional[torch.Tensor] = None):
    """bf16 [M,K] -> (q [M,K] fp8 | None, qt [K,M] fp8 | None, dq f32[1]) with per-tensor scale fmax / amax;
    amax_out (f32[1]) additionally accumulates max |x| (delayed scaling: the next step's `amax`)."""
    ld, K = _rows(x)
    M = x.shape[0]
    assert (M % 4 == 0 or not transposed) and K % 8 == 0
    q = torch.empty(M, K, dtype=fp8_dtypes[fmt], device=x.device) if rowmajor else None
    qt = torch.empty(K, M, dtype=fp8_dtypes[fmt], device=x.device) if transposed else None
    dq = torch.empty(1, dtype=f32, device=x.device)
    check(_lib.load().vds_quant_fp8(_p(x), ld, M, K, fmt, _p(amax), _p(q), K, _p(qt), M, _p(dq), _p(amax_out),
                                    _stream()), "vds_quant_fp8")
    return q, qt, dq


def gemm_fp8(epi: int, M: int, N: int, K: int, A, B, sa, sb, a_fmt: int, Cp=None, ldc=0, C2=None, ldc2=0, bias=None,
             aux=None, ldaux=0, gate=None, ldgate=0, rows_per_batch=0, split_k=1, emit=None, tn: bool = False):
    """C = epilogue((A[M,K] . B[N,K]^T) * sa * sb), A / B contiguous fp8 (A e4m3 or e5m2, B e4m3).
    tn: C[M,N] = sum_k A[k,m] B[k,n] with A [K,M] (e5m2) and B [K,N] (e4m3) row-major -- the weight gradient read
    straight from the token-major fp8 copies (EPI_F32 only).
    emit = dict(q=, qt=, amax_in=, amax_out=, dq_out=, fmt=, colsum=): fp8 copies of the epilogue result (vds_fp8_out)."""
    assert A.is_contiguous() and B.is_contiguous()
    assert (A.shape == (K, M) and B.shape == (K, N) and emit is None) if tn else (A.shape == (M, K) and B.shape == (N, K))
    a = _gemm_args(VDS_TN if tn else VDS_NT, epi, M, N, K, A, M if tn else K, B, N if tn else K, Cp, ldc, C2, ldc2, bias, aux,
                   ldaux, gate, ldgate, rows_per_batch, split_k)
    e = None
    if emit is not None:
        q, qt = emit.get("q"), emit.get("qt")
        assert (q is None or q.shape == (M, N)) and (qt is None or qt.shape == (N, M))
        e = C.byref(_lib.Fp8Out(_p(q), N, _p(qt), M, _p(emit.get("amax_in")), _p(emit.get("amax_out")),
                                _p(emit.get("dq_out")), int(emit.get("fmt", 0)), _p(emit.get("colsum"))))
    check(_lib.load().vds_gemm_fp8(a, _p(sa), _p(sb), a_fmt, 0, e, _stream()),
          f"vds_gemm_fp8({'tn' if tn else f'epi={epi}'},M={M},N={N},K={K})")


def _wgrad_split(tiles: int, kt: int, slots: int) -> int:
    """split-K factor of a weight-gradient GEMM: minimise (rounds of `slots` co-resident workgroups) x
    (K tiles per workgroup) plus the fp32-atomic traffic of the partial tiles (64 KB each at the
    chip-wide ~1.3 TB/s atomic rate, priced in units of one K-tile step ~1.5 us)."""
    best, best_cost = 1, None
    for s in range(1, 17):
        if s > 1 and kt // s < 8:
            break
        rounds = -(-(tiles * s) // slots)
        cost = rounds * -(-kt // s) + (tiles * s * 0.034 if s > 1 else 0.0)
        if best_cost is None or cost < best_cost - 1e-9:
            best, best_cost = s, cost
    return best


def linear_wgrad(dy, x, dW: torch.Tensor, accumulate: bool = False, split_k: Optional[int] = None):
    """dW[N,K] (f32) = dy^T x   (dy [M,N], x [M,K]).  The library picks tiling and split-K itself (split_k=None):
    a split over the tokens adds atomically into dW, which must then be pre-zeroed (the model zeroes its flat gradient
    buffers once per step); accumulate=True forces the atomic path so several calls sum into dW."""
    M, N = dy.shape
    K = x.shape[1]
    assert dW.dtype == f32 and dW.numel() == N * K and dW.is_contiguous()
    if split_k is None:
        split = -1 if accumulate else 0
    else:
        split = -max(2, split_k) if accumulate else split_k
    gemm(VDS_TN, EPI_F32, N, K, M, dy, dy.stride(0), x, x.stride(0), dW, K, split_k=split)


# -------------------------------------------------------------------------- attention ----
def _st(t):
    assert t.stride(3) == 1
    return t.stride(0), t.stride(1), t.stride(2)


def _kv_lens_ptr(kv_lens, B: int) -> int:
    """device pointer of a per-sample key-count tensor: int32, CUDA, shape [B], contiguous -- anything else is an error"""
    if not (isinstance(kv_lens, torch.Tensor) and kv_lens.is_cuda and kv_lens.dtype == torch.int32
            and tuple(kv_lens.shape) == (B,) and kv_lens.is_contiguous()):
        raise ValueError(f"kv_lens must be a contiguous int32 CUDA tensor of shape [{B}]")
    return kv_lens.data_ptr()


def _frames(frames, kv_lens, Lq: int, Lk: int, past: int = 0):
    """vds_mod_groups of a frame-causal self-attention call: (lead, period) checked against the sequence, or ValueError"""
    if kv_lens is not None:
        raise ValueError("attention: frames (frame-causal self-attention) and kv_lens (cross-attention) exclude each other")
    if Lq + past != Lk:
        raise ValueError(f"frame-causal attention is self-attention: Lq = {Lq}" + (f" + past = {past}" if past else "") +
                         f" != Lk = {Lk}")
    lead, period = check_mod_groups(frames, Lq)
    return C.byref(_lib.ModGroups(lead, period))


def _frame_major(frame_major, frames, kv_lens, past=0, chunk=1, window=None) -> bool:
    """frame_major needs frames and excludes past / kv_lens, chunk != 1 and a window need frame_major: refused here, before
    anything is launched"""
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"attention: chunk = {chunk!r} must be an int >= 1 (token-frames per causal chunk)")
    if window is not None:
        if isinstance(window, bool) or not isinstance(window, int) or window < 1:
            raise ValueError(f"attention: window = {window!r} must be an int >= 1 (chunks a token query attends, its own "
                             "included) or None")
        if not frame_major or past:
            raise ValueError(f"attention: window = {window} needs frame_major=True and no past -- the sliding window exists "
                             "on the frame-major kernels only; a cached call attends whatever rows the cache holds")
    if not frame_major:
        if chunk != 1:
            raise ValueError(f"attention: chunk = {chunk} needs frame_major=True -- the chunk-causal mask exists on the "
                             "frame-major kernels only (the interleaved and the past calls are frame-causal: chunk = 1)")
        return False
    if frames is None:
        raise ValueError("attention: frame_major=True needs frames=(lead, period)")
    if past or kv_lens is not None:
        raise ValueError("attention: frame_major=True is the full-sequence self-attention: not with past or kv_lens")
    return True


def _teacher(teacher, frame_major, frames, kv_lens, past, window, Lq) -> bool:
    """teacher=True (the clean-context mask of teacher forcing) needs frame_major=True and frames=(lead, 2n), and excludes
    window, past and kv_lens: refused here, before anything is launched"""
    if not teacher:
        return False
    if not frame_major or frames is None:
        raise ValueError("attention: teacher=True needs frame_major=True and frames=(lead, 2n) -- the teacher-forcing mask "
                         "exists on the frame-major kernels only; pass frame_major=True with frame-major q / k / v rows")
    if window is not None:
        raise ValueError(f"attention: teacher=True excludes window = {window} -- the sliding window over a clean context is "
                         "not built; pass window=None")
    if past:
        raise ValueError(f"attention: teacher=True excludes past = {past} -- the clean context is part of the sequence "
                         "([lead | clean frames | noisy frames]), not a cache; pass past=0")
    if kv_lens is not None:
        raise ValueError("attention: teacher=True is self-attention: pass kv_lens=None")
    lead, period = frames
    if int(period) % 2:
        raise ValueError(f"attention: teacher=True needs an even period (n clean frames and their n noisy copies), got "
                         f"frames = {tuple(frames)}; pass frames=(lead, 2 * n)")
    return True


def _band(band, frame_major, frames, kv_lens, past, window, teacher, chunk) -> int:
    """band (chunks on each side of a token's own chunk; the frame band of the bidirectional model) needs frame_major=True
    and frames=(lead, period), and excludes window, teacher, past and kv_lens: refused here, before anything is launched"""
    if isinstance(band, bool) or not isinstance(band, int):
        raise ValueError(f"attention: band = {band!r} must be an int >= 0 (chunks attended on each side of a token's own "
                         "chunk) or None; pass band=None for the call without a band")
    if band < 0:
        raise ValueError(f"attention: band = {band} must be >= 0 -- 0 is 'own chunk plus the lead rows'; pass band=None for "
                         "the call without a band")
    if not frame_major or frames is None:
        raise ValueError(f"attention: band = {band} needs frame_major=True and frames=(lead, period) -- the frame band exists "
                         "on the frame-major kernels only; pass frame_major=True with frame-major q / k / v rows")
    if window is not None:
        raise ValueError(f"attention: band = {band} excludes window = {window} -- the window is the causal mask's, the band "
                         "is two-sided; pass window=None (or band=None for the sliding-window call)")
    if teacher:
        raise ValueError(f"attention: band = {band} excludes teacher=True -- teacher forcing is a causal mask; pass "
                         "teacher=False (or band=None)")
    if past:
        raise ValueError(f"attention: band = {band} excludes past = {past} -- the band call is the full-sequence "
                         "self-attention and has no cache; pass past=0")
    if kv_lens is not None:
        raise ValueError(f"attention: band = {band} is self-attention: pass kv_lens=None")
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"attention: chunk = {chunk!r} must be an int >= 1 (token-frames per chunk of the band)")
    return band


def _attn_args(q, k, v, o, lse, kv_pad_ones, grads=None, delta=None) -> AttnArgs:
    """vds_attn_args of a call.  Forward: shapes, q / k / v / o with their strides, lse; the backward adds
    grads = (do, dq, dk, dv) with theirs and the delta workspace with its size"""
    a = AttnArgs()
    a.B, a.H, a.Lq, a.head_dim = q.shape
    a.Lk = k.shape[2]
    tensors = {"q": q, "k": k, "v": v, "o": o}
    if grads is not None:
        tensors.update(zip(("do", "dq", "dk", "dv"), grads))
    for name, t in tensors.items():
        setattr(a, "d_o" if name == "do" else name, _p(t))
        for ax, stride in zip(("_sb", "_sh", "_sl"), _st(t)):
            setattr(a, name + ax, stride)
    a.lse = _p(lse)
    a.kv_pad_ones = int(kv_pad_ones)  # (True = 1: self-attention layout; 2: ones in k / v only, cross-attention)
    if grads is not None:
        a.delta, a.ws_floats = _p(delta), delta.numel()
    return a


def _attn_entry(direction: str, a: AttnArgs, kv_lens, frames, fr, past: int, fmaj: bool, chunk: int, window,
                teacher: bool = False):
    """(C entry point, its arguments after vds_attn_args, the text of its error message): the one place that maps
    (direction, kv_lens, frames, past, frame_major, chunk, window) to one of the 13 calls, or with teacher to
    vds_teacher_attn_fwd / _bwd.  Without a flag every call is the entry point it always was; fr is the vds_mod_groups of
    frames (_frames)"""
    B, H, Lq, Lk, hd = a.B, a.H, a.Lq, a.Lk, a.head_dim
    cross = f"B={B},H={H},Lq={Lq},Lk={Lk},hd={hd}"
    self_ = f"B={B},H={H},L={Lq},hd={hd},frames={tuple(frames)}" if fr is not None else None
    if teacher:
        name = f"vds_teacher_attn_{direction}"
        return name, (fr, chunk), f"{name}({self_},chunk={chunk})"
    if fmaj and window is not None:
        name, extra, what = "_causal_fm_window", (fr, chunk, window), f"{self_},chunk={chunk},window={window}"
    elif fmaj and chunk != 1:
        name, extra, what = "_causal_fm_chunk", (fr, chunk), f"{self_},chunk={chunk}"
    elif fmaj:
        name, extra, what = "_causal_fm", (fr,), self_
    elif fr is not None and past:
        name, extra, what = "_causal_past", (fr, past), f"{cross},frames={tuple(frames)},past={past}"
    elif fr is not None:
        name, extra, what = "_causal", (fr,), self_
    elif kv_lens is None:
        name, extra, what = "", (), cross
    else:
        name, extra, what = "_kvlen", (_kv_lens_ptr(kv_lens, B),), cross
    name = f"vds_attn_{direction}{name}"
    return name, extra, f"{name}({what})"


def _attn_call(direction: str, a: AttnArgs, kv_lens, frames, fr, past, fmaj, chunk, window, teacher=False):
    lib = _lib.load()
    name, extra, what = _attn_entry(direction, a, kv_lens, frames, fr, past, fmaj, chunk, window, teacher)
    check(getattr(lib, name)(C.byref(a), *extra, _stream()), what)


def attn_fwd(q, k, v, o, lse, kv_pad_ones: bool = False, kv_lens=None, frames=None, past: int = 0,
             frame_major: bool = False, chunk: int = 1, window=None, teacher: bool = False):
    """q [B,H,Lq,hd], k/v [B,H,Lk,hd], o [B,H,Lq,hd] strided views (last dim contiguous); lse f32 [B,H,Lq].
    kv_pad_ones: k / v are views into qkv_rope_fwd outputs whose pad carries the ones columns.
    kv_lens: int32 CUDA tensor [B]; sample b attends its first kv_lens[b] keys only (vds_attn_fwd_kvlen).
    frames: (lead, period) -- frame-causal self-attention: row q attends row k iff mod_group_of(k) <= mod_group_of(q)
    (vds_attn_fwd_causal); not together with kv_lens.
    past (with frames): k / v hold Lk = Lq + past rows [lead rows | past cached token rows | this call's token rows]; a
    token query also attends every past key, a lead query none of them (vds_attn_fwd_causal_past).  Forward only.
    frame_major (with frames; not with past / kv_lens): q, k, v and lse rows are frame-major (fm_row), o stays token-major
    and the key tiles no query of a tile attends are skipped (vds_attn_fwd_causal_fm).
    chunk (with frame_major): the mask is causal over chunks of `chunk` token-frames and bidirectional inside a chunk --
    fm_group_of(key, chunk) <= fm_group_of(query, chunk) (vds_attn_fwd_causal_fm_chunk); 1 is the frame-causal mask.
    window (with frame_major; in chunks): a token query of chunk n attends the lead keys and the token keys of chunks
    max(0, n - window + 1) .. n only (vds_attn_fwd_causal_fm_window); None: no window.
    teacher (with frame_major, frames=(lead, 2n); not with window / past / kv_lens): teacher forcing -- the token-frames are n
    clean frames then their n noisy copies; a clean query attends the lead keys and the clean chunks up to its own, a noisy
    query the lead keys, the clean chunks BEFORE its own and its own noisy chunk (vds_teacher_attn_fwd)."""
    B, H, Lq, hd = q.shape
    Lk = k.shape[2]
    past = int(past)
    teacher = _teacher(teacher, frame_major, frames, kv_lens, past, window, Lq)
    fmaj = _frame_major(frame_major, frames, kv_lens, past, chunk, window)
    if past < 0 or (past and frames is None):
        raise ValueError(f"attention: past = {past} must be >= 0 and needs frames=(lead, period)")
    fr = _frames(frames, kv_lens, Lq, Lk, past) if frames is not None else None
    a = _attn_args(q, k, v, o, lse, kv_pad_ones)
    _attn_call("fwd", a, kv_lens, frames, fr, past, fmaj, chunk, window, teacher)


def _band_call(direction: str, a: AttnArgs, frames, fr, chunk: int, band: int):
    name = f"vds_band_attn_{direction}"
    what = f"{name}(B={a.B},H={a.H},L={a.Lq},hd={a.head_dim},frames={tuple(frames)},chunk={chunk},band={band})"
    check(getattr(_lib.load(), name)(C.byref(a), fr, chunk, band, _stream()), what)


def band_attn_fwd(q, k, v, o, lse, kv_pad_ones: bool = False, kv_lens=None, frames=None, past: int = 0,
                  frame_major: bool = False, chunk: int = 1, window=None, teacher: bool = False, band=None):
    """attn_fwd with the trailing keyword band.  band=None: attn_fwd, unchanged.
    band (with frame_major and frames=(lead, period); not with window / teacher / past / kv_lens; in chunks): the frame
    band of the bidirectional model, not causal -- a token row of chunk n attends the lead rows and the token rows of
    chunks n - band .. n + band (frame-major rows [fm_band_lo, fm_band_hi)), a lead row attends every row
    (vds_band_attn_fwd).  q, k, v and lse rows are frame-major, o token-major, as in every frame_major call."""
    if band is None:
        return attn_fwd(q, k, v, o, lse, kv_pad_ones, kv_lens, frames, past, frame_major, chunk, window, teacher)
    band = _band(band, frame_major, frames, kv_lens, int(past), window, teacher, chunk)
    Lq, Lk = q.shape[2], k.shape[2]
    fr = _frames(frames, kv_lens, Lq, Lk)
    _band_call("fwd", _attn_args(q, k, v, o, lse, kv_pad_ones), frames, fr, chunk, band)


def band_attn_bwd(q, k, v, o, lse, do, dq, dk, dv, delta=None, kv_pad_ones: bool = False, kv_lens=None, frames=None,
                  frame_major: bool = False, chunk: int = 1, window=None, teacher: bool = False, band=None):
    """attn_bwd with the trailing keyword band (band_attn_fwd); band=None: attn_bwd, unchanged.  The workspace is that of
    the frame_major call (vds_band_attn_bwd)."""
    if band is None:
        return attn_bwd(q, k, v, o, lse, do, dq, dk, dv, delta, kv_pad_ones, kv_lens, frames, frame_major, chunk, window,
                        teacher)
    band = _band(band, frame_major, frames, kv_lens, 0, window, teacher, chunk)
    B, H, Lq, hd = q.shape
    assert lse.is_contiguous()
    Lk = k.shape[2]
    fr = _frames(frames, kv_lens, Lq, Lk)
    if delta is None:
        delta = torch.empty(attn_bwd_workspace_floats(B, H, Lq, Lk, hd, kv_pad_ones), dtype=f32, device=q.device)
    assert delta.numel() >= 2 * B * H * Lq and delta.is_contiguous(), "attn_bwd: delta workspace is [2,B,H,Lq] f32"
    _band_call("bwd", _attn_args(q, k, v, o, lse, kv_pad_ones, (do, dq, dk, dv), delta), frames, fr, chunk, band)


def kv_pad_ones(kv: torch.Tensor, B: int, Lk: int, H: int, hd: int, hdp: int, k_col0: int, v_col0: int):
    """kv [B*Lk, ld] token-major bf16 (the context_kv output) -> (k, v) [B,H,Lk,hdp] with the ones columns of the
    head_dim-72 attention kernels in the pad (vds_kv_pad_ones)"""
    kp = torch.empty(B, H, Lk, hdp, dtype=bf16, device=kv.device)
    vp = torch.empty(B, H, Lk, hdp, dtype=bf16, device=kv.device)
    check(_lib.load().vds_kv_pad_ones(_p(kv), kv.stride(0), k_col0, v_col0, _p(kp), _p(vp), B, Lk, H, hd, hdp, _stream()),
          "vds_kv_pad_ones")
    return kp, vp


def attn_bwd_workspace_floats(B, H, Lq, Lk, hd, kv_pad_ones: bool = False) -> int:
    """floats of workspace vds_attn_bwd wants: the [2,B,H,Lq] statistics + the fp32 partials of a query-split dK/dV launch"""
    a = AttnArgs()
    a.B, a.H, a.Lq, a.Lk, a.head_dim = B, H, Lq, Lk, hd
    a.kv_pad_ones = int(kv_pad_ones)
    return _lib.load().vds_attn_bwd_workspace_bytes(C.byref(a)) // 4


def attn_bwd(q, k, v, o, lse, do, dq, dk, dv, delta=None, kv_pad_ones: bool = False, kv_lens=None, frames=None,
             frame_major: bool = False, chunk: int = 1, window=None, teacher: bool = False):
    """delta: f32 workspace of 2*B*H*Lq elements (rowsum(dO*O), then lse*log2 e); allocated here when None
    (size from vds_attn_bwd_workspace_bytes).
    kv_lens: as in attn_fwd; rows kv_lens[b].. of dk[b] / dv[b] are written as zeros (vds_attn_bwd_kvlen).
    frames: as in attn_fwd; a dk / dv row sums over the queries that attend it (vds_attn_bwd_causal).
    frame_major: as in attn_fwd -- q, k, v, lse, dq, dk, dv (and the delta workspace) rows are frame-major, o and do
    token-major (vds_attn_bwd_causal_fm).
    chunk: as in attn_fwd (vds_attn_bwd_causal_fm_chunk).
    window: as in attn_fwd (vds_attn_bwd_causal_fm_window).
    teacher: as in attn_fwd (vds_teacher_attn_bwd); the workspace is unchanged."""
    B, H, Lq, hd = q.shape
    assert lse.is_contiguous()
    Lk = k.shape[2]
    teacher = _teacher(teacher, frame_major, frames, kv_lens, 0, window, Lq)
    fmaj = _frame_major(frame_major, frames, kv_lens, 0, chunk, window)
    fr = _frames(frames, kv_lens, Lq, Lk) if frames is not None else None
    if delta is None:
        delta = torch.empty(attn_bwd_workspace_floats(B, H, Lq, Lk, hd, kv_pad_ones), dtype=f32, device=q.device)
    assert delta.numel() >= 2 * B * H * Lq and delta.is_contiguous(), "attn_bwd: delta workspace is [2,B,H,Lq] f32"
    a = _attn_args(q, k, v, o, lse, kv_pad_ones, (do, dq, dk, dv), delta)
    _attn_call("bwd", a, kv_lens, frames, fr, 0, fmaj, chunk, window, teacher)


# ---------------------------------------------------------------------- fp8 attention ----
FP8_ROW = 128  # bytes of an fp8 head row ([B,H,L,128]: head_dim data bytes + pad)


def attn_fp8_supported(hd: int) -> bool:
    return bool(_lib.load().vds_attn_fp8_supported(int(hd)))


def qkv_rope_fwd_fp8(qkv, cos, sin, v0, lam, B, L, H, hd, hdp, amax_prev, amax_cur, amax_stride, deq, want_v=False):
    """qkv_rope_fwd with e4m3 outputs: -> (q8, k8, v8 [B,H,L,128] float8_e4m3fn, v bf16 [B,H,L,hdp] or None).
    amax_prev / amax_cur: f32 views whose elements 0, stride, 2*stride are the q, k, v amax of the previous / this
    step; deq: f32[8], entries 0..2 receive the dequantisation factors, entry 4 the exponent E that ties q's factor
    to k's (s_q s_k log2(e) / sqrt(hd) = 2^-E: include/vds.h)."""
    dev = qkv.device
    q8 = torch.empty(B, H, L, FP8_ROW, dtype=torch.float8_e4m3fn, device=dev)
    k8 = torch.empty_like(q8)
    v8 = torch.empty_like(q8)
    v = torch.empty(B, H, L, hdp, dtype=bf16, device=dev) if want_v else None
    check(_lib.load().vds_qkv_rope_fwd_fp8(_p(qkv), _p(cos), _p(sin), _p(v0), _p(lam), _p(q8), _p(k8), _p(v8), _p(v),
                                           _p(amax_prev), _p(amax_cur), amax_stride, _p(deq), B, L, H, hd, hdp,
                                           _stream()), "vds_qkv_rope_fwd_fp8")
    return q8, k8, v8, v


def cross_qkv_fp8(qc, ckv, B, Lq, Lk, H, hd, amax_prev, amax_cur, amax_stride, deq):
    """the cross-attention operands as fp8 rows: qc [B*Lq, H*hd] (q_cross output), ckv [B*Lk, 2*H*hd] (context_kv output:
    k columns, then v columns) -> (q8 [B,H,Lq,128], k8, v8 [B,H,Lk,128]) e4m3; amax / deq as qkv_rope_fwd_fp8"""
    dev = qc.device
    assert qc.is_contiguous() and ckv.is_contiguous() and qc.shape == (B * Lq, H * hd) and ckv.shape == (B * Lk, 2 * H * hd)
    q8 = torch.empty(B, H, Lq, FP8_ROW, dtype=torch.float8_e4m3fn, device=dev)
    k8 = torch.empty(B, H, Lk, FP8_ROW, dtype=torch.float8_e4m3fn, device=dev)
    v8 = torch.empty_like(k8)
    check(_lib.load().vds_cross_qkv_fp8(_p(qc), _p(ckv), _p(q8), _p(k8), _p(v8), _p(amax_prev), _p(amax_cur), amax_stride,
                                        _p(deq), B, Lq, Lk, H, hd, _stream()), "vds_cross_qkv_fp8")
    return q8, k8, v8


def _attn8_args(q8, k8, v8, deq, hd):
    B, H, Lq, row = q8.shape
    assert row == FP8_ROW and q8.is_contiguous() and k8.is_contiguous() and v8.is_contiguous()
    assert deq.dtype == f32 and deq.numel() >= 5 and deq.is_contiguous()
    a = _lib.Attn8Args()
    a.B, a.H, a.Lq, a.Lk, a.head_dim = B, H, Lq, k8.shape[2], hd
    a.q, a.k, a.v, a.deq = _p(q8), _p(k8), _p(v8), _p(deq)
    return a


def attn_fp8_fwd(q8, k8, v8, deq, o, lse, hd, emit=None):
    """fp8 self-attention forward: q8/k8/v8 from qkv_rope_fwd_fp8, o [B,H,Lq,hd] bf16 strided view, lse f32 [B,H,Lq].
    emit = (amax_prev f32[1], amax_cur f32[1]): also returns (o as e4m3 [B*Lq, H*hd], dequantisation factor f32[1]),
    written by the kernel's epilogue with the previous step's amax (the attn_proj / cross_proj operand)."""
    a = _attn8_args(q8, k8, v8, deq, hd)
    a.o, (a.o_sb, a.o_sh, a.o_sl) = _p(o), _st(o)
    a.lse = _p(lse)
    out = None
    if emit is not None:
        oq = torch.empty(a.B * a.Lq, a.H * hd, dtype=fp8_dtypes[0], device=q8.device)
        sc = torch.empty(1, dtype=f32, device=q8.device)
        a.o_q, a.o_q_ld = _p(oq), oq.stride(0)
        a.e_amax_prev, a.e_amax_cur, a.e_dq_out = _p(emit[0]), _p(emit[1]), _p(sc)
        out = (oq, sc)
    check(_lib.load().vds_attn_fp8_fwd(C.byref(a), _stream()), f"vds_attn_fp8_fwd(B={a.B},H={a.H},Lq={a.Lq},Lk={a.Lk})")
    return out


def attn_fp8_delta(o2d, do2d, lse, doq, amax_prev, amax_cur, deq, B, H, L, hd):
    """backward preprocess over the token-major bf16 o / dO [B*L, H*hd]: -> stats f32 [2,B,H,L]; fills doq (e5m2
    [B,H,L,128], pad bytes untouched: allocate it zeroed once), deq[3]; records dO's amax"""
    assert o2d.stride(1) == 1 and do2d.stride(1) == 1 and doq.is_contiguous() and doq.shape == (B, H, L, FP8_ROW)
    stats = torch.empty(2, B, H, L, dtype=f32, device=o2d.device)
    check(_lib.load().vds_attn_fp8_delta(_p(o2d), L * o2d.stride(0), o2d.stride(0), _p(do2d), L * do2d.stride(0),
                                         do2d.stride(0), _p(lse), _p(stats), _p(doq), _p(amax_prev), _p(amax_cur),
                                         _p(deq), B, H, L, hd, _stream()), "vds_attn_fp8_delta")
    return stats


def attn_fp8_bwd(q8, k8, v8, doq, stats, deq, dq, dk, dv, hd, emit_dq=None):
    """dq / dk / dv: bf16 strided [B,H,L,hd] views.  emit_dq = (amax_prev, amax_cur): dQ additionally -- or, with
    dq=None, only -- as e5m2 [B*Lq, H*hd] from the kernel's epilogue; returns (dq_q, dequantisation factor)."""
    a = _attn8_args(q8, k8, v8, deq, hd)
    a.d_o, a.stats = _p(doq), _p(stats)
    out = None
    if emit_dq is not None:
        dqq = torch.empty(a.B * a.Lq, a.H * hd, dtype=fp8_dtypes[1], device=q8.device)
        sc = torch.empty(1, dtype=f32, device=q8.device)
        a.dq_q, a.dq_q_ld = _p(dqq), dqq.stride(0)
        a.e_amax_prev, a.e_amax_cur, a.e_dq_out = _p(emit_dq[0]), _p(emit_dq[1]), _p(sc)
        out = (dqq, sc)
    if dq is not None:
        a.dq, (a.dq_sb, a.dq_sh, a.dq_sl) = _p(dq), _st(dq)
    a.dk, (a.dk_sb, a.dk_sh, a.dk_sl) = _p(dk), _st(dk)
    a.dv, (a.dv_sb, a.dv_sh, a.dv_sl) = _p(dv), _st(dv)
    check(_lib.load().vds_attn_fp8_bwd(C.byref(a), _stream()), f"vds_attn_fp8_bwd(B={a.B},H={a.H},Lq={a.Lq},Lk={a.Lk})")
    return out


def attn_fp8_qk_factors(amax_q: float, amax_k: float, hd: int):
    """(alpha_q, alpha_k, E) the fp8 RoPE producer derives from the two amax values: k onto 448, q so that
    log2(e) / sqrt(hd) / (alpha_q alpha_k) = 2^-E with its amax in (224, 448].  For tests and tools that build fp8
    operands by hand; the product path gets them from vds_qkv_rope_fwd_fp8."""
    import math
    alpha_k = 448.0 / amax_k
    cl = math.log2(math.e) / math.sqrt(hd)
    E = math.floor(math.log2(448.0 * alpha_k / (cl * amax_q)))
    return cl * 2.0 ** E / alpha_k, alpha_k, float(E)


def attn_set_variant(mask: int) -> int:
    """tests / A-B: which head_dim-72 attention kernels use the 16x16x32 MFMA shape (bit 0 dK/dV, 1 dQ, 2 forward;
    -1 = default); returns the previous mask"""
    return _lib.load().vds_attn_set_variant(int(mask))


def heads_view(t: torch.Tensor, B: int, L: int, H: int, hd: int, offset: int = 0) -> torch.Tensor:
    """[B*L, ld] token-major buffer -> [B,H,L,hd] view of columns offset + h*hd + d."""
    ld = t.stride(0)
    return t.as_strided((B, H, L, hd), (L * ld, hd, ld, 1), t.storage_offset() + offset)


# ---------------------------------------------------------- norm / modulation / gates ----
def mod_group_of(l: int, lead: int, period: int) -> int:
    """modulation group of row l of a sample (include/vds.h: vds_mod_groups): 0 for the `lead` rows at its head, then
    1 + (l - lead) % period"""
    return 0 if l < lead else 1 + (l - lead) % period


def check_mod_groups(groups, L: int):
    """(lead, period) that splits L rows per sample into 1 + period groups, or ValueError"""
    lead, period = (int(v) for v in groups)
    if lead < 0 or period < 1 or lead > L or (L - lead) % period != 0:
        raise ValueError(f"modulation groups (lead={lead}, period={period}) do not fit {L} rows per sample: lead >= 0, "
                         f"period >= 1 and (L - lead) % period == 0 are required")
    return lead, period


def _groups(groups, L: int, mod: torch.Tensor, B: int):
    lead, period = check_mod_groups(groups, L)
    assert mod.shape[0] == B * (1 + period), f"grouped modulation table: {B * (1 + period)} rows expected, got {mod.shape[0]}"
    return C.byref(_lib.ModGroups(lead, period))


def _grouped_tables(mod, dmod):
    assert dmod.shape[0] == mod.shape[0] and dmod.stride(0) == mod.stride(0)


# One marshalling helper per kernel family.  `entry` is the C entry point the public wrapper reaches; `out` the arguments
# of its output -- (y, ldy) of a bf16 result, (q, ldq, fmt, amax_in, amax_part, dq_out) of an fp8 one --; `tail` what the
# entry takes after D (eps) and the shape (groups).
def _rmsnorm_fwd(entry, x, w, mod, shift_col, scale_col, out, B, L, eps, tail=()):
    rstd = torch.empty(B * L, dtype=f32, device=x.device)
    check(getattr(_lib.load(), entry)(_p(x), x.stride(0), _p(w), _p(mod), mod.stride(0), shift_col, scale_col, *out,
                                      _p(rstd), B, L, x.shape[1], eps, *tail, _stream()), entry)
    return rstd


def _rmsnorm_bwd(entry, dy, x, w, mod, shift_col, scale_col, rstd, dres, dmod, dw, B, L, tail=()):
    D = x.shape[1]
    dx = torch.empty(B * L, D, dtype=bf16, device=x.device)
    check(getattr(_lib.load(), entry)(_p(dy), dy.stride(0), _p(x), x.stride(0), _p(w), _p(mod), mod.stride(0), shift_col,
                                      scale_col, _p(rstd), _p(dres), dres.stride(0) if dres is not None else 0, _p(dx), D,
                                      _p(dmod), _p(dw), B, L, D, *tail, _stream()), entry)
    return dx


def _gate_bwd(entry, dxn, y, mod, gate_col, out, dmod, dbias, B, L, tail=()):
    check(getattr(_lib.load(), entry)(_p(dxn), dxn.stride(0), _p(y), y.stride(0), _p(mod), mod.stride(0), gate_col, *out,
                                      _p(dmod), _p(dbias), B, L, y.shape[1], *tail, _stream()), entry)


def rmsnorm_mod_fwd(x, w, mod, shift_col, scale_col, B, L, eps=1e-6):
    D = x.shape[1]
    y = torch.empty(B * L, D, dtype=bf16, device=x.device)
    return y, _rmsnorm_fwd("vds_rmsnorm_mod_fwd", x, w, mod, shift_col, scale_col, (_p(y), D), B, L, eps)


def rmsnorm_mod_fwd_grouped(x, w, mod, shift_col, scale_col, B, L, groups, eps=1e-6):
    """rmsnorm_mod_fwd with mod f32 [B*G, ld]: row l of sample b reads modulation row b*G + mod_group_of(l)"""
    D = x.shape[1]
    y = torch.empty(B * L, D, dtype=bf16, device=x.device)
    return y, _rmsnorm_fwd("vds_rmsnorm_mod_fwd_grouped", x, w, mod, shift_col, scale_col, (_p(y), D), B, L, eps,
                           (_groups(groups, L, mod, B),))


def rmsnorm_mod_bwd(dy, x, w, mod, shift_col, scale_col, rstd, dres, dmod, dw, B, L):
    return _rmsnorm_bwd("vds_rmsnorm_mod_bwd", dy, x, w, mod, shift_col, scale_col, rstd, dres, dmod, dw, B, L)


def rmsnorm_mod_bwd_grouped(dy, x, w, mod, shift_col, scale_col, rstd, dres, dmod, dw, B, L, groups):
    """rmsnorm_mod_bwd with mod / dmod [B*G, ld]: dmod row b*G + g accumulates the sums over the rows of that group"""
    _grouped_tables(mod, dmod)
    return _rmsnorm_bwd("vds_rmsnorm_mod_bwd_grouped", dy, x, w, mod, shift_col, scale_col, rstd, dres, dmod, dw, B, L,
                        (_groups(groups, L, mod, B),))


def gate_bwd(dxn, y, mod, gate_col, dmod, dbias, B, L):
    D = y.shape[1]
    dy = torch.empty(B * L, D, dtype=bf16, device=y.device)
    _gate_bwd("vds_gate_bwd", dxn, y, mod, gate_col, (_p(dy), D), dmod, dbias, B, L)
    return dy


def gate_bwd_grouped(dxn, y, mod, gate_col, dmod, dbias, B, L, groups):
    D = y.shape[1]
    dy = torch.empty(B * L, D, dtype=bf16, device=y.device)
    _grouped_tables(mod, dmod)
    _gate_bwd("vds_gate_bwd_grouped", dxn, y, mod, gate_col, (_p(dy), D), dmod, dbias, B, L, (_groups(groups, L, mod, B),))
    return dy


def _fp8_out(rows, cols, fmt, device):
    return torch.empty(rows, cols, dtype=fp8_dtypes[fmt], device=device), torch.empty(1, dtype=f32, device=device)


def transpose_fp8(q: torch.Tensor) -> torch.Tensor:
    """fp8 [M,K] (contiguous, K % 16 == 0) -> [K,M]"""
    M, K = q.shape
    assert q.is_contiguous() and K % 16 == 0 and M % 4 == 0
    qt = torch.empty(K, M, dtype=q.dtype, device=q.device)
    check(_lib.load().vds_transpose_fp8(_p(q), K, M, K, _p(qt), M, _stream()), "vds_transpose_fp8")
    return qt


def _part_ok(t, rows):
    assert t is None or (t.dtype == f32 and t.is_contiguous() and t.numel() >= rows)


def _fp8_rows(rows, cols, fmt, amax_in, amax_part, device):
    """(q, dq f32[1]) of an fp8-emitting call and the `out` arguments that describe them"""
    _part_ok(amax_part, rows)
    q, dq = _fp8_out(rows, cols, fmt, device)
    return q, dq, (_p(q), cols, fmt, _p(amax_in), _p(amax_part), _p(dq))


def rmsnorm_mod_fwd_fp8(x, w, mod, shift_col, scale_col, B, L, fmt, amax_in, amax_part, eps=1e-6):
    """rmsnorm_mod_fwd whose result leaves the kernel as fp8 (row-major) -> (q, dq f32[1], rstd);
    amax_part: f32 [>= B*L], zeroed by the caller: per-wave maxima of |result|; its maximum is the tensor's amax (or None)"""
    q, dq, out = _fp8_rows(B * L, x.shape[1], fmt, amax_in, amax_part, x.device)
    return q, dq, _rmsnorm_fwd("vds_rmsnorm_mod_fwd_fp8", x, w, mod, shift_col, scale_col, out, B, L, eps)


def gate_bwd_fp8(dxn, y, mod, gate_col, dmod, dbias, B, L, fmt, amax_in, amax_part):
    """gate_bwd whose dy leaves the kernel as fp8 (row-major) -> (q, dq f32[1])"""
    q, dq, out = _fp8_rows(B * L, y.shape[1], fmt, amax_in, amax_part, y.device)
    _gate_bwd("vds_gate_bwd_fp8", dxn, y, mod, gate_col, out, dmod, dbias, B, L)
    return q, dq


def qkv_rope_bwd_fp8(dq, dk, dv, cos, sin, qkv_raw, v0, lam, dv0_acc, dlam, mix, add_dv0, B, L, H, hd, hdp, fmt,
                     amax_in, amax_part):
    """qkv_rope_bwd whose [B*L, 3D] result leaves the kernel as fp8 (row-major) -> (q, dq f32[1])"""
    _part_ok(amax_part, B * L)
    q, s = _fp8_out(B * L, 3 * H * hd, fmt, dq.device)
    check(_lib.load().vds_qkv_rope_bwd_fp8(_p(dq), _p(dk), _p(dv), _p(cos), _p(sin), _p(qkv_raw), _p(v0), _p(lam),
                                           _p(dv0_acc), _p(dlam), _p(q), 3 * H * hd, fmt, _p(amax_in), _p(amax_part),
                                           _p(s), int(mix), int(add_dv0), B, L, H, hd, hdp, _stream()),
          "vds_qkv_rope_bwd_fp8")
    return q, s


def colsum(x, out, rows_per_sample: int = 0, row_offset: int = 0):
    """out[n] += sum_m x[m, n]; with rows_per_sample: only rows m with m % rows_per_sample >= row_offset (token rows)"""
    M, N = x.shape
    check(_lib.load().vds_colsum_bf16_rows(_p(x), x.stride(0), _p(out), M, N, rows_per_sample, row_offset, _stream()),
          "vds_colsum_bf16_rows")


# -------------------------------------------------------------- low-rank adapters ----
LOWRANK_RANKS = (16, 32, 64)


def lowrank_chunk(which: str, r: int) -> int:
    """the kernels' chunk sizes for rank r: "down" elements of K per LDS stage, "up" columns of y per workgroup, "wgrad"
    rows per fp32 partial"""
    return int(_lib.load().vds_lowrank_chunk({"down": 0, "up": 1, "wgrad": 2}[which], int(r)))


def _lowrank_operands(what: str, layout: int, **tensors):
    """the operands of a low-rank call against the shapes and dtypes the kernel will assume: name=(tensor, dtype, shape);
    a mismatch raises here instead of becoming an out-of-range read in the kernel"""
    if layout not in (0, 1):
        raise ValueError(f"{what}: layout = {layout!r} must be 0 or 1")
    for name, (t, dtype, shape) in tensors.items():
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape):
            got = (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{what}: {name} must be {dtype} of shape {tuple(shape)}, got {got}")


def lowrank_down(x, w, scale: float = 1.0, layout: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """u = bf16(scale * x w^T) for layout 0 (w [r, K], the adapter's A) or bf16(scale * x w) for layout 1 (w [K, r], the
    adapter's B).  x [M, K] bf16 -> u [M, r] bf16."""
    M, K = x.shape
    r = w.shape[0] if layout == 0 else w.shape[1]
    u = out if out is not None else torch.empty(M, r, dtype=bf16, device=x.device)
    _lowrank_operands("lowrank_down", layout, x=(x, bf16, (M, K)), w=(w, bf16, (r, K) if layout == 0 else (K, r)),
                      u=(u, bf16, (M, r)))
    check(_lib.load().vds_lowrank_down(_p(x), _rows(x)[0], _p(w), _rows(w)[0], int(layout), _p(u), _rows(u)[0], M, K, r,
                                       float(scale), _stream()), f"vds_lowrank_down(M={M},K={K},r={r},layout={layout})")
    return u


def lowrank_up_add(u, w, y, scale: float = 1.0, layout: int = 0) -> torch.Tensor:
    """y += scale * u w^T in place for layout 0 (w [N, r], the adapter's B) or scale * u w for layout 1 (w [r, N], the
    adapter's A).  u [M, r], y [M, N] bf16."""
    M, N = y.shape
    r = u.shape[1]
    _lowrank_operands("lowrank_up_add", layout, u=(u, bf16, (M, r)), w=(w, bf16, (N, r) if layout == 0 else (r, N)),
                      y=(y, bf16, (M, N)))
    check(_lib.load().vds_lowrank_up_add(_p(u), _rows(u)[0], _p(w), _rows(w)[0], int(layout), _p(y), _rows(y)[0], M, N, r,
                                         float(scale), _stream()), f"vds_lowrank_up_add(M={M},N={N},r={r},layout={layout})")
    return y


def lowrank_wgrad(a, u, g, scale: float = 1.0, layout: int = 0, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """g += scale * a^T u in fp32 for layout 0 (g [N, r]: dB from dY and U) or scale * u^T a for layout 1 (g [r, N]: dA
    from x and dU).  a [M, N], u [M, r] bf16; ws: f32 workspace of vds_lowrank_wgrad_workspace_floats(M, N, r) floats
    (allocated here when not given)."""
    M, N = a.shape
    r = u.shape[1]
    _lowrank_operands("lowrank_wgrad", layout, a=(a, bf16, (M, N)), u=(u, bf16, (M, r)),
                      g=(g, f32, (N, r) if layout == 0 else (r, N)))
    if ws is None:
        ws = torch.empty(max(1, int(_lib.load().vds_lowrank_wgrad_workspace_floats(M, N, r))), dtype=f32, device=a.device)
    if ws.dtype != f32 or ws.dim() != 1 or not ws.is_contiguous():
        raise ValueError(f"lowrank_wgrad: ws must be a contiguous 1-D float32 tensor, got {ws.dtype} {tuple(ws.shape)}")
    check(_lib.load().vds_lowrank_wgrad(_p(a), _rows(a)[0], _p(u), _rows(u)[0], _p(g), _rows(g)[0], int(layout), M, N, r,
                                        float(scale), _p(ws), ws.numel(), _stream()),
          f"vds_lowrank_wgrad(M={M},N={N},r={r},layout={layout})")
    return g


# ------------------------------------------------------------------ frame-major rows ----
# The head-major tensors of a frame-major self-attention (q, k, v, dq, dk, dv, lse, v0, dv0) keep a frame's rows
# contiguous; the model's token order stays (h w t).  With S = (L - lead) // period rows per frame (include/vds.h):
def fm_row(l: int, lead: int, period: int, L: int) -> int:
    """frame-major row of token row l"""
    if l < lead:
        return l
    S = (L - lead) // period
    return lead + ((l - lead) % period) * S + (l - lead) // period


def tok_row(r: int, lead: int, period: int, L: int) -> int:
    """token row of frame-major row r (the inverse of fm_row)"""
    if r < lead:
        return r
    S = (L - lead) // period
    return lead + ((r - lead) % S) * period + (r - lead) // S


def fm_group_of(r: int, lead: int, S: int, chunk: int = 1) -> int:
    """group of frame-major row r: 0 for the lead rows, then 1 + (r - lead) // (chunk * S); query r attends key j iff
    fm_group_of(j) <= fm_group_of(r) -- mod_group_of's mask, permuted (chunk = 1), or the chunk-causal mask: causal over
    chunks of `chunk` frames, bidirectional inside one"""
    return 0 if r < lead else 1 + (r - lead) // (chunk * S)


def chunk_group_of(l: int, lead: int, period: int, chunk: int = 1) -> int:
    """fm_group_of in token rows: 0 for the lead rows, then 1 + ((l - lead) % period) // chunk"""
    return 0 if l < lead else 1 + ((l - lead) % period) // chunk


def fm_key_end(q0: int, q1: int, lead: int, S: int, chunk: int = 1, L=None) -> int:
    """first frame-major key row that no query row of [q0, q1) attends: a query tile's key loop ends here.  L (rows per
    sample): the bound is clipped to it, as the kernels do -- a short last chunk (period % chunk != 0) would pass it"""
    if q1 <= lead:
        return lead
    G = chunk * S
    end = lead + ((q1 - 1 - lead) // G + 1) * G
    return end if L is None else min(end, L)


def fm_query_start(k0: int, lead: int, S: int, chunk: int = 1) -> int:
    """first frame-major query row that may attend a key row of [k0, ...): a key tile's query loop starts here (rounded
    down to the query tile by the kernels)"""
    if k0 < lead:
        return 0
    G = chunk * S
    return lead + ((k0 - lead) // G) * G


def fm_key_begin(q0: int, lead: int, S: int, chunk: int = 1, window=None) -> int:
    """first frame-major TOKEN key row that query row q0 attends under a window of `window` chunks (None: no window): a
    query tile's second key range starts at the tile that holds this row for its first token query.  lead for a lead query
    (it attends no token key)"""
    if q0 < lead or window is None:
        return lead
    G = chunk * S
    return lead + max(0, (q0 - lead) // G - window + 1) * G


def fm_query_end(k1: int, lead: int, S: int, chunk: int = 1, window=None, L=None) -> int:
    """first frame-major query row past the ones that attend key row k1 - 1, the last of a key tile [.., k1): a key
    tile's query loop ends here unless the tile holds a lead key (every query attends those: L)"""
    if window is None or k1 - 1 < lead:
        return L
    G = chunk * S
    end = lead + ((k1 - 1 - lead) // G + window) * G
    return end if L is None else min(end, L)


def fm_band_lo(x: int, lead: int, S: int, chunk: int = 1, band: int = 0, L=None) -> int:
    """first frame-major TOKEN row that token row x attends (and is attended by) under a frame band of `band` chunks on
    each side: lead + max(0, chunk(x) - band) * G with G = chunk * S.  A lead row attends everything: 0"""
    if x < lead:
        return 0
    G = chunk * S
    return lead + max(0, (x - lead) // G - band) * G


def fm_band_hi(x: int, lead: int, S: int, chunk: int = 1, band: int = 0, L=None) -> int:
    """first frame-major row past the token rows that token row x attends (and is attended by) under the frame band:
    lead + (chunk(x) + band + 1) * G, clipped to L when given (the last chunk may be short).  A lead row: L"""
    if x < lead:
        return L
    G = chunk * S
    end = lead + ((x - lead) // G + band + 1) * G
    return end if L is None else min(end, L)


def _fm_frames(frames, L: int):
    """vds_mod_groups of a frame-major qkv / RoPE call, checked against L before anything is launched"""
    lead, period = check_mod_groups(frames, L)
    return C.byref(_lib.ModGroups(lead, period))


# ----------------------------------------------------------------- qkv / rope / res-V ----
QK_NORM_EPS = 1e-6  # RMSNorm's eps (model.py:34-41)


def _fm_entry(entry, frames, L: int, tail):
    """the entry point and its arguments after hdp: with frames=(lead, period) the _fm form, which takes them last"""
    if frames is None:
        return entry, tail
    return entry + "_fm", tail + (_fm_frames(frames, L),)


def _qkv_rope_fwd(entry, qkv, cos, sin, v0, lam, B, L, H, hd, hdp, frames, tail=()):
    entry, tail = _fm_entry(entry, frames, L, tail)
    q = torch.empty(B, H, L, hdp, dtype=bf16, device=qkv.device)
    k = torch.empty_like(q)
    v = torch.empty_like(q)
    check(getattr(_lib.load(), entry)(_p(qkv), _p(cos), _p(sin), _p(v0), _p(lam), _p(q), _p(k), _p(v), B, L, H, hd, hdp,
                                      *tail, _stream()), entry)
    return q, k, v


def _qkv_rope_bwd(entry, dq, dk, dv, cos, sin, qkv_raw, v0, lam, dv0_acc, dlam, mix, add_dv0, B, L, H, hd, hdp, frames,
                  tail=()):
    entry, tail = _fm_entry(entry, frames, L, tail)
    dqkv = torch.empty(B * L, 3 * H * hd, dtype=bf16, device=dq.device)
    check(getattr(_lib.load(), entry)(_p(dq), _p(dk), _p(dv), _p(cos), _p(sin), _p(qkv_raw), _p(v0), _p(lam), _p(dv0_acc),
                                      _p(dlam), _p(dqkv), int(mix), int(add_dv0), B, L, H, hd, hdp, *tail, _stream()), entry)
    return dqkv


def qkv_rope_fwd(qkv, cos, sin, v0, lam, B, L, H, hd, hdp, frames=None):
    """frames=(lead, period): the q / k / v head rows of token l are written, and v0 read, at row fm_row(l)
    (vds_qkv_rope_fwd_fm)"""
    return _qkv_rope_fwd("vds_qkv_rope_fwd", qkv, cos, sin, v0, lam, B, L, H, hd, hdp, frames)


def qkv_rope_bwd(dq, dk, dv, cos, sin, qkv_raw, v0, lam, dv0_acc, dlam, mix, add_dv0, B, L, H, hd, hdp, frames=None):
    """frames=(lead, period): dq / dk / dv, v0 and dv0_acc are addressed at row fm_row(l), dqkv stays token-major
    (vds_qkv_rope_bwd_fm)"""
    return _qkv_rope_bwd("vds_qkv_rope_bwd", dq, dk, dv, cos, sin, qkv_raw, v0, lam, dv0_acc, dlam, mix, add_dv0, B, L, H,
                         hd, hdp, frames)


def qkv_rope_norm_fwd(qkv, cos, sin, v0, lam, B, L, H, hd, hdp, eps: float = QK_NORM_EPS, frames=None):
    """qkv_rope_fwd with QK-norm: every head row of q and k goes through a weightless RMSNorm (fp32 math, rounded to
    bf16) before the rotation; v, the pad and the ones columns are qkv_rope_fwd's (vds_qkv_rope_norm_fwd).
    frames: as in qkv_rope_fwd (vds_qkv_rope_norm_fwd_fm)"""
    return _qkv_rope_fwd("vds_qkv_rope_norm_fwd", qkv, cos, sin, v0, lam, B, L, H, hd, hdp, frames, (float(eps),))


def qkv_rope_norm_bwd(dq, dk, dv, cos, sin, qkv_raw, v0, lam, dv0_acc, dlam, mix, add_dv0, B, L, H, hd, hdp,
                      eps: float = QK_NORM_EPS, frames=None):
    """backward of qkv_rope_norm_fwd; qkv_raw (the forward's qkv) is needed in every call (vds_qkv_rope_norm_bwd).
    frames: as in qkv_rope_bwd (vds_qkv_rope_norm_bwd_fm)"""
    return _qkv_rope_bwd("vds_qkv_rope_norm_bwd", dq, dk, dv, cos, sin, qkv_raw, v0, lam, dv0_acc, dlam, mix, add_dv0, B, L,
                         H, hd, hdp, frames, (float(eps),))


def _kv_cache_args(k, v, v0, B, H, hdp, lead, past, L):
    """(kv_sb, kv_sh, kv_sl) shared by the cache buffers k, v (and v0) [B,H,rows,hdp] of the cache forms below"""
    for t in (k, v) + ((v0,) if v0 is not None else ()):
        if not (t.dtype == bf16 and t.dim() == 4 and t.shape[0] == B and t.shape[1] == H and t.shape[3] == hdp
                and t.stride(3) == 1 and t.stride() == k.stride() and t.shape[2] >= L + past):
            raise ValueError(f"kv cache buffers must be bf16 [B={B},H={H},rows>={L + past},hdp={hdp}] with equal strides")
    if not 0 <= lead <= L or past < 0:
        raise ValueError(f"kv cache: lead = {lead} not in [0, {L}] or past = {past} < 0")
    return k.stride(0), k.stride(1), k.stride(2)


def _qkv_rope_fwd_cache(entry, qkv, cos, sin, v0, lam, k, v, lead, past, B, L, H, hd, hdp, tail=()):
    st = _kv_cache_args(k, v, v0, B, H, hdp, lead, past, L)
    q = torch.empty(B, H, L, hdp, dtype=bf16, device=qkv.device)
    check(getattr(_lib.load(), entry)(_p(qkv), _p(cos), _p(sin), _p(v0), _p(lam), _p(q), _p(k), _p(v), *st, lead, past, B,
                                      L, H, hd, hdp, *tail, _stream()), entry)
    return q


def qkv_rope_fwd_cache(qkv, cos, sin, v0, lam, k, v, lead, past, B, L, H, hd, hdp):
    """qkv_rope_fwd whose k / v rows go to row (l < lead ? l : l + past) of the cache buffers k, v [B,H,rows,hdp]; v0 is
    block 0's cache v buffer, read through the same map (vds_qkv_rope_fwd_cache).  Returns q [B,H,L,hdp]."""
    return _qkv_rope_fwd_cache("vds_qkv_rope_fwd_cache", qkv, cos, sin, v0, lam, k, v, lead, past, B, L, H, hd, hdp)


def qkv_rope_norm_fwd_cache(qkv, cos, sin, v0, lam, k, v, lead, past, B, L, H, hd, hdp, eps: float = QK_NORM_EPS):
    """qkv_rope_fwd_cache with QK-norm (vds_qkv_rope_norm_fwd_cache)"""
    return _qkv_rope_fwd_cache("vds_qkv_rope_norm_fwd_cache", qkv, cos, sin, v0, lam, k, v, lead, past, B, L, H, hd, hdp,
                               (float(eps),))


def _head_rows(what: str, name: str, t, H: int, hd: int):
    """a head-norm operand: a bf16 [M, H * hd] tensor or column window whose rows are 16-byte segments of a parent"""
    if not isinstance(t, torch.Tensor) or t.dtype != bf16 or t.dim() != 2 or t.shape[1] != H * hd:
        got = (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{what}: {name} must be bfloat16 of shape [M, H * hd = {H * hd}], got {got}")
    if t.shape[0] < 1 or t.stride(1) != 1 or t.stride(0) % 8 != 0 or t.stride(0) < H * hd:
        raise ValueError(f"{what}: {name} {tuple(t.shape)} with strides {t.stride()} is no window of rows -- at least one "
                         f"row, contiguous columns and a row stride that is a multiple of 8 and at least {H * hd}")


def _head_dims(what: str, H, hd):
    if not (isinstance(H, int) and isinstance(hd, int)) or H < 1 or hd < 8 or hd % 8 != 0 or hd > 128:
        raise ValueError(f"{what}: H = {H!r} must be an int >= 1 and hd = {hd!r} a multiple of 8 up to 128")


def head_rmsnorm_fwd(x, H: int, hd: int, eps: float = QK_NORM_EPS) -> torch.Tensor:
    """QK-norm of the head rows of x [M, H * hd] bf16 (a tensor or a column window such as ckv[:, :D]), IN PLACE:
    x[m, h] <- bf16(float(x[m, h]) * r), r = rsqrt(mean_d(x^2) + eps) -> rstd [M, H] f32 (vds_head_rmsnorm_fwd)"""
    _head_dims("head_rmsnorm_fwd", H, hd)
    _head_rows("head_rmsnorm_fwd", "x", x, H, hd)
    eps = float(eps)
    if not (0.0 < eps < float("inf")):
        raise ValueError(f"head_rmsnorm_fwd: eps = {eps!r} must be positive and finite")
    M = x.shape[0]
    rstd = torch.empty(M, H, dtype=f32, device=x.device)
    check(_lib.load().vds_head_rmsnorm_fwd(_p(x), x.stride(0), _p(rstd), M, H, hd, eps, _stream()),
          f"vds_head_rmsnorm_fwd(M={M},H={H},hd={hd})")
    return rstd


def head_rmsnorm_bwd(dy, y, rstd, H: int, hd: int) -> torch.Tensor:
    """backward of head_rmsnorm_fwd, IN PLACE on dy [M, H * hd] bf16: dy[m, h] <- bf16(r (g - y mean_d(g y))) with y the
    forward's output rows and rstd [M, H] f32 the forward's (vds_head_rmsnorm_bwd); dy and y may be column windows"""
    _head_dims("head_rmsnorm_bwd", H, hd)
    _head_rows("head_rmsnorm_bwd", "dy", dy, H, hd)
    _head_rows("head_rmsnorm_bwd", "y", y, H, hd)
    M = dy.shape[0]
    if y.shape[0] != M or y.device != dy.device:
        raise ValueError(f"head_rmsnorm_bwd: y has {y.shape[0]} rows on {y.device}, dy {M} on {dy.device}")
    if (not isinstance(rstd, torch.Tensor) or rstd.dtype != f32 or tuple(rstd.shape) != (M, H) or not rstd.is_contiguous()
            or rstd.device != dy.device):
        got = (rstd.dtype, tuple(rstd.shape)) if isinstance(rstd, torch.Tensor) else type(rstd).__name__
        raise ValueError(f"head_rmsnorm_bwd: rstd must be contiguous float32 of shape ({M}, {H}) on dy's device, got {got}")
    check(_lib.load().vds_head_rmsnorm_bwd(_p(dy), dy.stride(0), _p(y), y.stride(0), _p(rstd), M, H, hd, _stream()),
          f"vds_head_rmsnorm_bwd(M={M},H={H},hd={hd})")
    return dy


# ------------------------------------------------------- row movers of token routing ----
def _row_tensor(what: str, name: str, t, dtype=None):
    """a [outer, n, row] operand of the row movers: a contiguous GPU tensor of at least 2 dims (the last is the row, the one
    before counts the rows, the others multiply to `outer`) whose row is a whole number of 16-byte pieces"""
    if not isinstance(t, torch.Tensor) or t.dim() < 2 or (dtype is not None and t.dtype != dtype):
        got = (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{what}: {name} must be a {'tensor' if dtype is None else dtype} of shape [..., rows, row], got "
                         f"{got}")
    if not t.is_cuda:
        raise ValueError(f"{what}: {name} is on {t.device}; the kernels run on the GPU only -- pass {name}.cuda()")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} {tuple(t.shape)} with strides {t.stride()} is not contiguous -- pass "
                         f"{name}.contiguous()")
    row_bytes = t.shape[-1] * t.element_size()
    if row_bytes == 0 or row_bytes % 16 or t.data_ptr() % 16:
        raise ValueError(f"{what}: a row of {name} is {row_bytes} bytes at address {t.data_ptr():#x}; rows move in 16-byte "
                         "pieces -- pad the last dim to a multiple of 16 bytes and pass a 16-byte aligned tensor")
    outer = 1
    for s in t.shape[:-2]:
        outer *= s
    return outer, t.shape[-2], row_bytes


def _row_table(what: str, name: str, t, n: int, like):
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (n,) or not t.is_contiguous()
            or t.device != like.device):
        got = (t.dtype, tuple(t.shape), str(t.device)) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{what}: {name} must be a contiguous int32 tensor of shape [{n}] on {like.device} (the kernel reads "
                         f"it on the device), got {got} -- pass torch.as_tensor({name}, dtype=torch.int32).to(device)")


def _row_pair(what: str, a_name: str, a, b_name: str, b):
    """two row operands that differ in their row count only"""
    if a.dtype != b.dtype or a.device != b.device or a.shape[:-2] != b.shape[:-2] or a.shape[-1] != b.shape[-1]:
        raise ValueError(f"{what}: {a_name} {tuple(a.shape)} {a.dtype} on {a.device} and {b_name} {tuple(b.shape)} {b.dtype} "
                         f"on {b.device} must agree in dtype, device and every dim but the row count (dim -2)")


def rows_gather(src, idx, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[..., i, :] = src[..., idx[i], :] (vds_rows_gather): src [..., n_in, row] contiguous, any dtype whose row is a
    multiple of 16 bytes; idx int32 [n_out] on src's device, duplicates allowed; an index outside [0, n_in) gives a row of
    zeros.  Returns out [..., n_out, row] (allocated when not given; it must not overlap src)."""
    what = "rows_gather"
    outer, n_in, row_bytes = _row_tensor(what, "src", src)
    if not isinstance(idx, torch.Tensor) or idx.dim() != 1:
        raise ValueError(f"{what}: idx must be a 1-D int32 tensor on {src.device}")
    n_out = idx.shape[0]
    _row_table(what, "idx", idx, n_out, src)
    if n_in < 1:
        raise ValueError(f"{what}: src {tuple(src.shape)} has no rows to gather from")
    if out is None:
        out = torch.empty(src.shape[:-2] + (n_out, src.shape[-1]), dtype=src.dtype, device=src.device)
    elif n_out:
        _row_tensor(what, "out", out)
        _row_pair(what, "src", src, "out", out)
        if out.shape[-2] != n_out:
            raise ValueError(f"{what}: out has {out.shape[-2]} rows, idx {n_out} entries")
    if n_out == 0 or outer == 0:
        return out
    check(_lib.load().vds_rows_gather(_p(src), _p(out), _p(idx), outer, n_in, n_out, row_bytes, _stream()),
          f"vds_rows_gather(outer={outer},n_in={n_in},n_out={n_out},row_bytes={row_bytes})")
    return out


def rows_merge(full, part, inv, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[..., l, :] = part[..., inv[l], :] where 0 <= inv[l] < n_part, else full[..., l, :] (vds_rows_merge): full
    [..., n_full, row] and part [..., n_part, row] contiguous with rows of a multiple of 16 bytes, inv int32 [n_full] on
    their device.  out None: IN PLACE into full (returned); otherwise out gets every row and must not overlap part."""
    what = "rows_merge"
    outer, n_full, row_bytes = _row_tensor(what, "full", full)
    _row_tensor(what, "part", part)
    _row_pair(what, "full", full, "part", part)
    _row_table(what, "inv", inv, n_full, full)
    n_part = part.shape[-2]
    if out is None:
        out = full
    else:
        _row_tensor(what, "out", out)
        if out.shape != full.shape or out.dtype != full.dtype or out.device != full.device:
            raise ValueError(f"{what}: out {tuple(out.shape)} {out.dtype} must have full's shape {tuple(full.shape)}, dtype "
                             "and device (out=None merges in place into full)")
    if outer == 0 or n_full == 0:
        return out
    if n_part == 0:
        if out is not full:
            out.copy_(full)
        return out
    check(_lib.load().vds_rows_merge(_p(full), _p(part), _p(out), _p(inv), outer, n_full, n_part, row_bytes, _stream()),
          f"vds_rows_merge(outer={outer},n_full={n_full},n_part={n_part},row_bytes={row_bytes})")
    return out


def rows_scatter_add(part, acc, idx) -> torch.Tensor:
    """acc[..., idx[i], :] += part[..., i, :] in fp32, IN PLACE (vds_rows_scatter_add_f32): part [..., n_part, row] and acc
    [..., n_full, row] contiguous float32 with rows of a multiple of 4 elements, idx int32 [n_part] on their device.  The
    entries of idx must be DISTINCT (a plain read-add-write: a duplicate would lose an add); an index outside [0, n_full)
    is skipped.  Returns acc."""
    what = "rows_scatter_add"
    outer, n_part, _ = _row_tensor(what, "part", part, f32)
    _, n_full, _ = _row_tensor(what, "acc", acc, f32)
    _row_pair(what, "part", part, "acc", acc)
    _row_table(what, "idx", idx, n_part, part)
    if outer == 0 or n_part == 0:
        return acc
    if n_full < 1:
        raise ValueError(f"{what}: acc {tuple(acc.shape)} has no rows to add into")
    check(_lib.load().vds_rows_scatter_add_f32(_p(part), _p(acc), _p(idx), outer, n_full, n_part, part.shape[-1],
                                               _stream()),
          f"vds_rows_scatter_add_f32(outer={outer},n_full={n_full},n_part={n_part},row_elems={part.shape[-1]})")
    return acc


def dv0_reduce(dvs, lams, out, B, H, L, hd, hdp, accumulate: bool = False):
    """out[B,H,L,hdp] f32 (+)= sum_i (1 - lam_i) dvs[i][..., :hd]: the residual-V gradient of v_0 from all mixed blocks in one
    pass (vds_dv0_reduce; the blocks' RoPE backward then runs with mix = 2)"""
    import ctypes
    n = len(dvs)
    assert n == len(lams) and out.dtype == f32 and out.is_contiguous()
    for t in dvs:
        assert t.dtype == bf16 and t.is_contiguous() and tuple(t.shape) == (B, H, L, hdp)
    pa = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t in dvs])
    la = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t in lams])
    check(_lib.load().vds_dv0_reduce(ctypes.cast(pa, ctypes.c_void_p), ctypes.cast(la, ctypes.c_void_p), n, _p(out),
                                     int(accumulate), B, H, L, hd, hdp, _stream()), "vds_dv0_reduce")


def rope_apply(x, cos, sin, inverse: bool = False):
    """apply_rotary_emb (model.py:266-275): x [B,H,L,hd] bf16 (last dim contiguous), cos / sin f32 [L, hd/2]"""
    B, H, L, hd = x.shape
    assert x.dtype == bf16 and x.stride(3) == 1 and cos.dtype == f32 and cos.shape == (L, hd // 2) == sin.shape
    assert cos.is_contiguous() and sin.is_contiguous()
    y = torch.empty(B, H, L, hd, dtype=bf16, device=x.device)
    check(_lib.load().vds_rope_apply(_p(x), x.stride(0), x.stride(1), x.stride(2), _p(cos), _p(sin), _p(y),
                                     y.stride(0), y.stride(1), y.stride(2), B, H, L, hd, int(inverse), _stream()),
          "vds_rope_apply")
    return y


def rope_rows(tabs, thw, start, n_reg, device):
    """tabs = (t_cos, t_sin, s_cos, s_sin) device tables; returns cos, sin [n_reg + t*h*w, hd/2] f32."""
    t, h, w = thw
    nt, ns = tabs[0].shape[1], tabs[2].shape[1]
    rows = n_reg + t * h * w
    cos = torch.empty(rows, nt + 2 * ns, dtype=f32, device=device)
    sin = torch.empty_like(cos)
    if isinstance(start, torch.Tensor):  # offsets in device memory (int32[3]): whole-step graph replay
        assert start.is_cuda and start.dtype == torch.int32 and start.numel() == 3
        check(_lib.load().vds_rope_rows_dev(_p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(tabs[3]), nt, ns, t, h, w,
                                            _p(start), n_reg, _p(cos), _p(sin), _stream()), "vds_rope_rows_dev")
        return cos, sin
    check(_lib.load().vds_rope_rows(_p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(tabs[3]), nt, ns, t, h, w, start[0],
                                    start[1], start[2], n_reg, _p(cos), _p(sin), _stream()), "vds_rope_rows")
    return cos, sin


# ------------------------------------------------------------------- small linears ----
def small_linear_fwd(x, W, bias, act_in: int):
    M, K = x.shape
    N = W.shape[0]
    assert x.dtype == f32 and x.is_contiguous() and W.is_contiguous()
    y = torch.empty(M, N, dtype=f32, device=x.device)
    check(_lib.load().vds_small_linear_fwd(_p(x), _p(W), _p(bias), _p(y), M, N, K, act_in, _stream()),
          "vds_small_linear_fwd")
    return y


def small_linear_bwd(dy, x, W, dW, dbias, dx, act_in: int):
    M, N = dy.shape
    K = x.shape[1]
    assert dy.is_contiguous() and x.is_contiguous()
    check(_lib.load().vds_small_linear_bwd(_p(dy), _p(x), _p(W), _p(dW), _p(dbias), _p(dx), M, N, K, act_in,
                                           _stream()), "vds_small_linear_bwd")


def ptr_table(tensors) -> torch.Tensor:
    """device array of the tensors' device pointers (int64), for the batched entry points"""
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64, device=tensors[0].device)


def small_linear_fwd_batched(x, W_tab, bias_tab, nb: int, N: int, act_in: int):
    """y[i] = act(x) W_i^T + b_i for the nb weight sets of the pointer tables; x f32 [M <= 16, K] -> f32 [nb, M, N]"""
    M, K = x.shape
    assert x.dtype == f32 and x.is_contiguous() and M <= 16
    y = torch.empty(nb, M, N, dtype=f32, device=x.device)
    check(_lib.load().vds_small_linear_fwd_batched(_p(x), _p(W_tab), _p(bias_tab), _p(y), M * N, nb, M, N, K, act_in,
                                                   _stream()), "vds_small_linear_fwd_batched")
    return y


def small_linear_bwd_batched(dy, x, W_tab, dW_tab, dbias_tab, dx, act_in: int):
    """dy f32 [nb, M, N]; writes every dW_i / dbias_i, accumulates dx (f32 [M, K]) over the sets"""
    nb, M, N = dy.shape
    K = x.shape[1]
    assert dy.is_contiguous() and x.is_contiguous() and M <= 16
    check(_lib.load().vds_small_linear_bwd_batched(_p(dy), M * N, _p(x), _p(W_tab), _p(dW_tab), _p(dbias_tab), _p(dx),
                                                   nb, M, N, K, act_in, _stream()), "vds_small_linear_bwd_batched")


def timestep_embedding(t, D):
    B = t.shape[0]
    out = torch.empty(B, D, dtype=f32, device=t.device)
    check(_lib.load().vds_timestep_embedding(_p(t), _p(out), B, D, _stream()), "vds_timestep_embedding")
    return out


# ------------------------------------------------------------- patches / registers ----
def patchify(x, pt, p, lead_rows: int = 0):
    """[B,C,T,H,W] -> patch rows; lead_rows = R: rows of a [B * (R + N)] token buffer (R zero rows per sample first)"""
    B, Cc, T, H, W = x.shape
    n = (T // pt) * (H // p) * (W // p)
    alloc = torch.zeros if lead_rows else torch.empty
    out = alloc(B * (lead_rows + n), Cc * pt * p * p, dtype=bf16, device=x.device)
    check(_lib.load().vds_patchify_rows(_p(x), _p(out), B, Cc, T, H, W, pt, p, lead_rows + n, lead_rows, _stream()),
          "vds_patchify_rows")
    return out


def unpatchify(y, B, Cc, T, H, W, pt, p, lead_rows: int = 0):
    n = (T // pt) * (H // p) * (W // p)
    out = torch.empty(B, Cc, T, H, W, dtype=bf16, device=y.device)
    check(_lib.load().vds_unpatchify_rows(_p(y), _p(out), B, Cc, T, H, W, pt, p, lead_rows + n, lead_rows, 0, _stream()),
          "vds_unpatchify_rows")
    return out


def unpatchify_bwd(dout, pt, p, lead_rows: int = 0):
    B, Cc, T, H, W = dout.shape
    n = (T // pt) * (H // p) * (W // p)
    alloc = torch.zeros if lead_rows else torch.empty
    dy = alloc(B * (lead_rows + n), Cc * pt * p * p, dtype=bf16, device=dout.device)
    check(_lib.load().vds_unpatchify_rows(_p(dout), _p(dy), B, Cc, T, H, W, pt, p, lead_rows + n, lead_rows, 1, _stream()),
          "vds_unpatchify_rows(bwd)")
    return dy


def fill_registers(reg, x, batch_stride, B, R, D):
    check(_lib.load().vds_fill_registers(_p(reg), _p(x), batch_stride, B, R, D, _stream()), "vds_fill_registers")


def registers_bwd(dx, batch_stride, dreg, B, R, D):
    check(_lib.load().vds_registers_bwd(_p(dx), batch_stride, _p(dreg), B, R, D, _stream()), "vds_registers_bwd")


# ---------------------------------------------------------------- noising / loss ----
def noise_latents(x, noise, t):
    B = x.shape[0]
    per = x.numel() // B
    zt = torch.empty_like(x)
    v = torch.empty_like(x)
    check(_lib.load().vds_noise_latents(_p(x), _p(noise), _p(t), _p(zt), _p(v), B, per, _stream()),
          "vds_noise_latents")
    return zt, v


def flow_loss(v, out, want_grad: bool, gscale: float = 1.0):
    B = v.shape[0]
    per = v.numel() // B
    lib = _lib.load()
    # [loss | per-sample | per-workgroup partials]: every word is written by the kernels (fixed-order two-stage reduction)
    acc = torch.empty(1 + B + lib.vds_flow_loss_workspace_floats(B, per), dtype=f32, device=v.device)
    dout = torch.empty_like(out) if want_grad else None
    check(lib.vds_flow_loss(_p(v), _p(out), _p(acc), _p(acc[1:]), _p(dout), gscale, B, per, _p(acc[1 + B:]), _stream()),
          "vds_flow_loss")
    return acc[0], acc[1:1 + B], dout


def _frames_tab(t, B: int, T: int, tps: int, what: str) -> torch.Tensor:
    assert T % tps == 0
    assert t.is_cuda and t.dtype == f32 and tuple(t.shape) == (B, T // tps) and t.is_contiguous(), \
        f"{what}: a contiguous f32 CUDA tensor [{B}, {T // tps}] expected"
    return t


def noise_latents_frames(x, noise, t, time_patch: int):
    """noise_latents with t f32 [B, T / time_patch]: latent frame j of sample b is noised with t[b, j // time_patch]"""
    B, Cc, T, H, W = x.shape
    assert x.is_contiguous() and noise.is_contiguous()
    zt = torch.empty_like(x)
    v = torch.empty_like(x)
    check(_lib.load().vds_noise_latents_frames(_p(x), _p(noise), _p(_frames_tab(t, B, T, time_patch, "t")), _p(zt), _p(v),
                                               B, Cc, T, H * W, time_patch, _stream()), "vds_noise_latents_frames")
    return zt, v


def flow_loss_frames(v, out, w, time_patch: int, want_grad: bool, gscale: float = 1.0):
    """frame-weighted flow loss (include/vds.h: vds_flow_loss_frames): v / out [B,C,T,H,W] bf16, w f32 [B, T / time_patch]
    -> (loss, per_sample [B], dout | None)"""
    B, Cc, T, H, W = v.shape
    assert v.is_contiguous() and out.is_contiguous()
    lib = _lib.load()
    F = T // time_patch
    acc = torch.empty(1 + B + lib.vds_flow_loss_frames_workspace_floats(B, F, Cc * time_patch * H * W), dtype=f32,
                      device=v.device)
    dout = torch.empty_like(out) if want_grad else None
    check(lib.vds_flow_loss_frames(_p(v), _p(out), _p(_frames_tab(w, B, T, time_patch, "w")), _p(acc), _p(acc[1:]),
                                   _p(dout), gscale, B, Cc, T, H * W, time_patch, _p(acc[1 + B:]), _stream()),
          "vds_flow_loss_frames")
    return acc[0], acc[1:1 + B], dout


def flow_loss_frames_bwd(v, out, w, time_patch: int, gloss):
    """d loss / d out of flow_loss_frames; gloss: f32 device scalar (the upstream gradient)"""
    B, Cc, T, H, W = v.shape
    assert gloss.is_cuda and gloss.dtype == f32 and gloss.numel() == 1 and out.is_contiguous() and v.is_contiguous()
    dout = torch.empty_like(out)
    check(_lib.load().vds_flow_loss_frames_bwd(_p(v), _p(out), _p(_frames_tab(w, B, T, time_patch, "w")), _p(gloss),
                                               _p(dout), B, Cc, T, H * W, time_patch, _stream()),
          "vds_flow_loss_frames_bwd")
    return dout


def flow_loss_bwd(v, out, gloss):
    """d loss / d out = 2 (out - v) gloss / numel, bf16; gloss: f32 device scalar (the upstream gradient)"""
    B = v.shape[0]
    assert gloss.is_cuda and gloss.dtype == f32 and gloss.numel() == 1 and out.is_contiguous() and v.is_contiguous()
    dout = torch.empty_like(out)
    check(_lib.load().vds_flow_loss_bwd(_p(v), _p(out), _p(gloss), _p(dout), B, v.numel() // B, _stream()),
          "vds_flow_loss_bwd")
    return dout


def cfg_euler_step(cond, uncond, acc, latents, cfg_scale: float, dt: float):
    """acc (f32) += dt * (uncond + cfg*(cond-uncond)) [bf16 math like the reference]; latents = bf16(acc)."""
    n = cond.numel()
    assert acc.dtype == f32 and acc.numel() == n and latents.numel() == n and cond.is_contiguous()
    check(_lib.load().vds_cfg_euler_step(_p(cond), _p(uncond), _p(acc), _p(latents), float(cfg_scale), float(dt), n,
                                         _stream()), "vds_cfg_euler_step")


# ------------------------------------------------------------------------------- Muon ----
def muon_workspace_bytes(nmat: int, rows: int, cols: int) -> int:
    n = int(_lib.load().vds_muon_workspace_bytes(nmat, rows, cols))
    if n == 0:
        raise ValueError(f"Muon: unsupported group ({nmat} matrices of [{rows}, {cols}]): dimensions must be multiples of 8")
    return n


def muon_views(ws: torch.Tensor, nmat: int, rows: int, cols: int):
    """the sections of a Muon workspace (uint8 tensor) as tensors: x0 / x1 bf16 [nmat, m, n], a / b bf16 [nmat, m, m],
    sumsq f32 [nmat]; m = min(rows, cols), n = max(rows, cols)"""
    off = (C.c_int64 * 6)()
    check(_lib.load().vds_muon_workspace_layout(nmat, rows, cols, C.addressof(off)), "vds_muon_workspace_layout")
    m, n = min(rows, cols), max(rows, cols)

    def sec(o, shape, dt):
        numel = 1
        for d in shape:
            numel *= d
        return ws[o:o + numel * dt.itemsize].view(dt).view(shape)
    return {"x0": sec(off[0], (nmat, m, n), bf16), "x1": sec(off[1], (nmat, m, n), bf16),
            "a": sec(off[2], (nmat, m, m), bf16), "b": sec(off[3], (nmat, m, m), bf16), "sumsq": sec(off[4], (nmat,), f32)}


def muon_table(mats, device) -> torch.Tensor:
    """device array of vds_muon_mat from (p, g, buf, p_bf16 | None, ema | None) tuples of data pointers"""
    descs = (_lib.MuonMat * len(mats))()
    for d, (pp, g, buf, pb, ema) in zip(descs, mats):
        d.p, d.g, d.buf, d.p_bf16, d.ema = pp, g, buf, pb, ema
    return torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(device)


def muon_momentum(table_ptr: int, nmat, rows, cols, mu, nesterov, guard_ptr, ws: torch.Tensor):
    check(_lib.load().vds_muon_momentum(table_ptr, nmat, rows, cols, mu, 1 if nesterov else 0, guard_ptr, _p(ws),
                                        _stream()), "vds_muon_momentum")


def muon_orthogonalize(ws: torch.Tensor, nmat, rows, cols, steps: int = 5):
    check(_lib.load().vds_muon_orthogonalize(_p(ws), nmat, rows, cols, steps, _stream()), "vds_muon_orthogonalize")


def muon_update(table_ptr: int, nmat, rows, cols, lr, wd, lr_mult, ema_decay, scalars_ptr, guard_ptr, ws: torch.Tensor):
    check(_lib.load().vds_muon_update(table_ptr, nmat, rows, cols, lr, wd, lr_mult, ema_decay, scalars_ptr, guard_ptr,
                                      _p(ws), _stream()), "vds_muon_update")


def cast_f32_bf16(src, dst):
    check(_lib.load().vds_cast_f32_bf16(_p(src), _p(dst), src.numel(), _stream()), "vds_cast_f32_bf16")


def cast_bf16_f32(src, dst):
    check(_lib.load().vds_cast_bf16_f32(_p(src), _p(dst), src.numel(), _stream()), "vds_cast_bf16_f32")


def selftest_lanemaps(device="cuda"):
    scratch = torch.zeros(2080 // 4 + 8, dtype=torch.int32, device=device)
    check(_lib.load().vds_selftest_lanemaps(_p(scratch), _stream()), "vds_selftest_lanemaps")
    torch.cuda.synchronize()
    return scratch[512:520].tolist()


# ------------------------------------------------------------------ live profiling ----
def prof_enable(mask: int = 0xFFFFFFFF):
    """record HIP event pairs (on the launch stream) around every launch of the enabled kernel classes"""
    check(_lib.load().vds_prof_enable(mask & 0xFFFFFFFF), "vds_prof_enable")


def prof_collect():
    """-> {class name: dict(launches, ms, flops, bytes)} of the launches since prof_enable; resets."""
    lib = _lib.load()
    arr = (_lib.ProfStat * _lib.PROF_NCLASS)()
    check(lib.vds_prof_collect(C.cast(arr, C.c_void_p)), "vds_prof_collect")
    out = {}
    for i in range(_lib.PROF_NCLASS):
        if arr[i].launches:
            out[lib.vds_prof_class_name(i).decode()] = dict(launches=arr[i].launches, ms=arr[i].ms, flops=arr[i].flops,
                                                            bytes=arr[i].bytes)
    return out
