"""Frame-causal self-attention kernels (vds_attn_fwd_causal / vds_attn_bwd_causal) against fp32 torch on the CPU
(tests/helpers/frame_causal_ref.py: scores masked_fill(-inf) where group(k) > group(q), softmax, autograd).  Token-major
buffers, every output pre-filled with NaN, relative Frobenius error at the tolerances tests/test_attn_kvlen_gpu.py and
tests/test_kernels_gpu.py use for the same quantities: o 6e-3, lse 1e-3, dq / dk / dv 8e-3."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_causal_ref as FC  # noqa: E402

pytestmark = pytest.mark.gpu

bf16, f32 = torch.bfloat16, torch.float32
TOL_O, TOL_LSE, TOL_G = 6e-3, 1e-3, 8e-3
NAMES = ["o", "lse", "dq", "dk", "dv"]
TOLS = [TOL_O, TOL_LSE, TOL_G, TOL_G, TOL_G]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import ops as _ops
    return _ops


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def close(name, got, ref, tol):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{name}: an element was left unwritten or is not finite"
    e = rel(got, ref)
    print(f"{name}: rel {e:.3e} (bound {tol:.1e})")
    assert e < tol, f"{name}: rel {e:.3e} >= {tol:.1e}"


def gen(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(bf16)


def heads(t2d, B, L, H, hd, off=0):
    """[B*L, ld] token-major rows -> [B,H,L,hd] (CPU copy of what ops.heads_view addresses)"""
    return t2d[:, off:off + H * hd].reshape(B, L, H, hd).permute(0, 2, 1, 3)


def groups_of(L, frames):
    return FC.R.group_index(L, *frames)


_inputs = {}
_refs = {}


def inputs(hd, B, H, L, boost=None, do_groups=None):
    """(qkv [B*L, 3D], dO [B*L, D]) bf16, shared and never modified.  boost = (lead, period): the K and V rows of the last
    group x 32; do_groups = ((lead, period), g): dO zero on the rows of groups > g."""
    key = (hd, B, H, L, boost, do_groups)
    if key not in _inputs:
        D = H * hd
        qkv, do = gen(B * L, 3 * D, seed=201), gen(B * L, D, seed=202)
        if boost is not None:
            last = (groups_of(L, boost) == boost[1]).repeat(B)
            qkv = qkv.clone()
            qkv[last, D:] = (qkv[last, D:].float() * 32).to(bf16)  # exact in bf16
        if do_groups is not None:
            fr, g = do_groups
            do = do.clone()
            do[(groups_of(L, fr) > g).repeat(B)] = 0
        _inputs[key] = (qkv, do)
    return _inputs[key]


def reference(hd, B, H, L, frames, boost=None, do_groups=None):
    """fp32 reference, once per case: o, lse, dq, dk, dv as [B,H,L,hd] / [B,H,L]; frames = None: unmasked"""
    key = (hd, B, H, L, frames, boost, do_groups)
    if key not in _refs:
        qkv, do = inputs(hd, B, H, L, boost, do_groups)
        D = H * hd
        q, k, v = (heads(qkv, B, L, H, hd, i * D).float().requires_grad_(True) for i in range(3))
        mask = FC.allowed(L, *frames) if frames is not None else torch.ones(L, L, dtype=torch.bool)
        o, lse = FC.masked_attention(q, k, v, mask)
        o.backward(heads(do, B, L, H, hd).float())
        _refs[key] = (o.detach(), lse.detach(), q.grad, k.grad, v.grad)
    return _refs[key]


def run(ops, hd, B, H, L, frames, ones=False, legacy_ws=False, bwd=True, boost=None, do_groups=None, graph=False,
        pass_frames=True):
    """the library on the shared inputs -> CPU tensors o, lse[, dq, dk, dv] laid out like the reference.  ones: q / k / v
    are the padded head-major rows ops.qkv_rope_fwd writes (identity rotation), with the ones columns the head_dim-72
    kernels read (kv_pad_ones = 1); else token-major views of the qkv buffer (kv_pad_ones = 0).  graph: forward and backward
    are captured once and replayed on re-poisoned outputs."""
    qkv, do = inputs(hd, B, H, L, boost, do_groups)
    D = H * hd
    qkvd, dod = qkv.cuda(), do.cuda()
    nan = float("nan")
    o = torch.full((B * L, D), nan, dtype=bf16, device="cuda")
    lse = torch.full((B, H, L), nan, dtype=f32, device="cuda")
    ov = ops.heads_view(o, B, L, H, hd)
    if ones:
        hdp = 96
        cos = torch.ones(L, hd // 2, dtype=f32, device="cuda")
        sin = torch.zeros(L, hd // 2, dtype=f32, device="cuda")
        qp, kp, vp = ops.qkv_rope_fwd(qkvd, cos, sin, None, None, B, L, H, hd, hdp)
        qv, kk, vv = qp[..., :hd], kp[..., :hd], vp[..., :hd]
        dqb, dkb, dvb = (torch.full((B, H, L, hdp), nan, dtype=bf16, device="cuda") for _ in range(3))
        dqv, dkv, dvv = dqb[..., :hd], dkb[..., :hd], dvb[..., :hd]
    else:
        qv, kk, vv = (ops.heads_view(qkvd, B, L, H, hd, i * D) for i in range(3))
        dqkv = torch.full_like(qkvd, nan)
        dqv, dkv, dvv = (ops.heads_view(dqkv, B, L, H, hd, i * D) for i in range(3))
    delta = None
    if bwd:
        n = 2 * B * H * L if legacy_ws else ops.attn_bwd_workspace_floats(B, H, L, L, hd, ones)
        delta = torch.full((n,), nan, dtype=f32, device="cuda")
    kw = {"frames": frames} if pass_frames else {}

    def call():
        ops.attn_fwd(qv, kk, vv, ov, lse, kv_pad_ones=ones, **kw)
        if bwd:
            ops.attn_bwd(qv, kk, vv, ov, lse, ops.heads_view(dod, B, L, H, hd), dqv, dkv, dvv, delta, kv_pad_ones=ones, **kw)

    if graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()  # warm-up outside the capture (first-launch attribute calls)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call()
        for t in (o, lse, dqv, dkv, dvv):
            t.fill_(nan)
        g.replay()
    else:
        call()
    torch.cuda.synchronize()
    out = [heads(o.cpu(), B, L, H, hd), lse.cpu()]
    if bwd:
        out += [t.cpu() for t in (dqv, dkv, dvv)]
    return out


def check(tag, got, ref):
    for name, g, r, tol in zip(NAMES, got, ref, TOLS):
        close(f"{tag}.{name}", g, r, tol)


HEAD_DIMS = [32, 64, 72, 96, 128]
# B * H = 10 crosses the 8-head grouping of the workgroup order.  280 = 256 + 24: a second 128-row query tile, a ragged last
# one and a ragged 64-key tile; {5, 3}: lead no multiple of 16, period no divisor of 16; {0, 1}: everything attended;
# {16, 128}: one row per frame, the lower-triangular mask behind the registers; {0, 150}: the plain lower-triangular mask
PLAIN = {"L280_16_8": (280, (16, 8)), "L140_5_3": (140, (5, 3)), "L200_0_1": (200, (0, 1)), "L144_16_128": (144, (16, 128)),
         "L150_0_150": (150, (0, 150))}


@pytest.mark.parametrize("case", list(PLAIN))
@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_plain_kernels(ops, hd, case):
    L, frames = PLAIN[case]
    check(f"plain.hd{hd}.{case}", run(ops, hd, 5, 2, L, frames), reference(hd, 5, 2, L, frames))


# head_dim 72, kv_pad_ones = 1.  2096 >= 2048: the 64-queries-per-wave forward, 2096 = 8 * 256 + 48 leaves a partly filled
# last workgroup; 1300: attn_fwd_kernel
ONES = {"L2096_16_8": (2096, (16, 8)), "L1300_16_4": (1300, (16, 4))}
VARIANTS = {"default": (None, None), "mfma32": (0, None), "all16_separate_delta": (7, 0), "all16_folded_delta": (7, 1)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", list(ONES))
def test_ones_column_kernels(ops, case, variant):
    """every vds_attn_set_variant / attn_delta_fold setting has masked instances: none is refused"""
    L, frames = ONES[case]
    mask, fold = VARIANTS[variant]
    prev_v = ops.attn_set_variant(mask) if mask is not None else None
    prev_f = ops.knob_set("attn_delta_fold", fold) if fold is not None else None
    try:
        got = run(ops, 72, 2, 2, L, frames, ones=True)
    finally:
        if prev_v is not None:
            ops.attn_set_variant(prev_v)
        if prev_f is not None:
            ops.knob_set("attn_delta_fold", prev_f)
    check(f"ones.{case}.{variant}", got, reference(72, 2, 2, L, frames))


@pytest.mark.parametrize("hd", [64, 96])
def test_plain_wide_forward(ops, hd):
    """L >= 2048 at head dims 64 and 96 (and 72 without the ones columns under the attn_fwd_wide knob): the plain
    64-queries-per-wave forward, attn_fwd_wide_kernel<.., false>"""
    B, H, L, frames = 1, 2, 2096, (16, 8)
    prev = ops.knob_set("attn_fwd_wide", 1) if hd == 96 else None  # (head dim 96 takes it only when forced)
    try:
        got = run(ops, hd, B, H, L, frames, bwd=False)
    finally:
        if prev is not None:
            ops.knob_set("attn_fwd_wide", prev)
    ref = reference(hd, B, H, L, frames)
    close(f"wide.hd{hd}.o", got[0], ref[0], TOL_O)
    close(f"wide.hd{hd}.lse", got[1], ref[1], TOL_LSE)


@pytest.mark.parametrize("legacy_ws", [False, True], ids=["split", "unsplit"])
def test_query_split_dkv(ops, legacy_ws):
    """B = 1, H = 2, L = 1024 + 16: the smallest self-attention shape whose plain dK/dV launch splits the query range
    (fp32 partials + dkv_reduce_kernel) when it gets the workspace the library asks for"""
    B, H, L, hd, frames = 1, 2, 1040, 64, (16, 8)
    assert ops.attn_bwd_workspace_floats(B, H, L, L, hd) > 2 * B * H * L
    got = run(ops, hd, B, H, L, frames, legacy_ws=legacy_ws)
    check(f"qsplit.{'unsplit' if legacy_ws else 'split'}", got, reference(hd, B, H, L, frames))


@pytest.mark.parametrize("kind,variant", [("plain64", None), ("plain72", None), ("ones", None), ("ones", 0)],
                         ids=["plain_hd64", "plain_hd72", "ones_default", "ones_mfma32"])
def test_masked_scores_stay_out_of_the_maximum(ops, kind, variant):
    """the K and V rows of the last group x 32: their scores dwarf every other, but no query of groups < 8 may see them --
    a kernel that masked after its running maximum would underflow the attended keys"""
    frames = (16, 8)
    hd, B, H, L, ones = {"plain64": (64, 5, 2, 280, False), "plain72": (72, 5, 2, 280, False),
                         "ones": (72, 2, 2, 2096, True)}[kind]
    prev = ops.attn_set_variant(variant) if variant is not None else None
    try:
        o, lse = run(ops, hd, B, H, L, frames, ones=ones, bwd=False, boost=frames)
    finally:
        if prev is not None:
            ops.attn_set_variant(prev)
    ro, rl = reference(hd, B, H, L, frames, boost=frames)[:2]
    rows = groups_of(L, frames) < 8
    close(f"max.{kind}.o", o[:, :, rows], ro[:, :, rows], TOL_O)
    close(f"max.{kind}.lse", lse[:, :, rows], rl[:, :, rows], TOL_LSE)


@pytest.mark.parametrize("kind", ["plain64", "plain128", "ones_L1300", "ones_L2096"])
def test_excluded_pairs_give_exact_zeros(ops, kind):
    """dO nonzero only on the rows of groups <= 3: the dk / dv rows of groups > 3 get nothing from their own queries
    (dO = 0, delta = 0) and P = 0 exactly from the others"""
    hd, B, H, L, frames, ones = {"plain64": (64, 5, 2, 280, (16, 8), False), "plain128": (128, 5, 2, 280, (16, 8), False),
                                 "ones_L1300": (72, 2, 2, 1300, (16, 4), True),
                                 "ones_L2096": (72, 2, 2, 2096, (16, 8), True)}[kind]
    got = run(ops, hd, B, H, L, frames, ones=ones, do_groups=(frames, 3))
    check(f"zeros.{kind}", got, reference(hd, B, H, L, frames, do_groups=(frames, 3)))
    late = groups_of(L, frames) > 3
    assert late.any()
    assert got[3][:, :, late].float().abs().max().item() == 0.0, "dk rows of groups > 3 must be exact zeros"
    assert got[4][:, :, late].float().abs().max().item() == 0.0, "dv rows of groups > 3 must be exact zeros"
    assert got[3][:, :, ~late].float().abs().max().item() > 0


@pytest.mark.parametrize("hd", [64, 72])
def test_no_frames_is_the_plain_call(ops, hd):
    """frames=None gives the bits of the call without the argument; {0, 1} (everything attended) agrees with it within the
    tolerances"""
    L = 200
    plain = run(ops, hd, 5, 2, L, None, pass_frames=False)
    none = run(ops, hd, 5, 2, L, None)
    for name, a, b in zip(NAMES, none, plain):
        assert torch.equal(a.view(torch.int16 if a.dtype == bf16 else torch.int32),
                           b.view(torch.int16 if b.dtype == bf16 else torch.int32)), name
    check(f"plain_vs_ref.hd{hd}", plain, reference(hd, 5, 2, L, None))
    full = run(ops, hd, 5, 2, L, (0, 1))
    for name, a, b, tol in zip(NAMES, full, plain, TOLS):
        close(f"all_attended.hd{hd}.{name}", a, b, tol)


@pytest.mark.parametrize("kind", ["plain", "ones"])
def test_graph_replay(ops, kind):
    """lead and period travel by value in the kernel arguments: a captured forward + backward replays them"""
    hd, B, H, L, frames, ones = (64, 5, 2, 280, (16, 8), False) if kind == "plain" else (72, 2, 2, 1300, (16, 4), True)
    eager = run(ops, hd, B, H, L, frames, ones=ones)
    replay = run(ops, hd, B, H, L, frames, ones=ones, graph=True)
    check(f"graph.{kind}", replay, reference(hd, B, H, L, frames))
    for name, a, b in zip(NAMES, replay, eager):
        assert torch.equal(a.float(), b.float()), f"{name}: replay differs from eager"


def test_argument_errors(ops):
    from video_diffusion_speedrun_amd import _lib
    hd, B, H, L = 64, 2, 2, 32
    D = H * hd
    q = torch.zeros(B * L, D, dtype=bf16, device="cuda")
    kv = torch.zeros(B * 48, 2 * D, dtype=bf16, device="cuda")
    o, lse = torch.zeros_like(q), torch.zeros(B, H, L, dtype=f32, device="cuda")
    qv, ov = ops.heads_view(q, B, L, H, hd), ops.heads_view(o, B, L, H, hd)
    k48, v48 = ops.heads_view(kv, B, 48, H, hd, 0), ops.heads_view(kv, B, 48, H, hd, D)
    k32, v32 = ops.heads_view(kv, B, L, H, hd, 0), ops.heads_view(kv, B, L, H, hd, D)
    with pytest.raises(ValueError, match="self-attention"):
        ops.attn_fwd(qv, k48, v48, ov, lse, frames=(16, 8))
    for bad in ((-1, 4), (16, 0), (16, 5), (40, 1)):
        with pytest.raises(ValueError):
            ops.attn_fwd(qv, k32, v32, ov, lse, frames=bad)
        with pytest.raises(ValueError):
            ops.attn_bwd(qv, k32, v32, ov, lse, qv, qv, k32, v32, frames=bad)
    with pytest.raises(ValueError, match="kv_lens"):
        ops.attn_fwd(qv, k32, v32, ov, lse, frames=(16, 8), kv_lens=torch.full((B,), L, dtype=torch.int32, device="cuda"))
    with pytest.raises(_lib.VdsError):  # the cross-attention layout has no frames
        ops.attn_fwd(qv, k32, v32, ov, lse, kv_pad_ones=2, frames=(16, 8))
    # the C entry points themselves: the same refusals as error codes, NULL frames = the plain call
    lib = _lib.load()
    a = _lib.AttnArgs()
    a.B, a.H, a.Lq, a.Lk, a.head_dim = B, H, L, L, hd
    for name, t in (("q", qv), ("k", k32), ("v", v32), ("o", ov)):
        setattr(a, name, t.data_ptr())
        for s, val in zip(("sb", "sh", "sl"), t.stride()[:3]):
            setattr(a, f"{name}_{s}", val)
    a.lse = lse.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    fr = lambda lead, period: C.byref(_lib.ModGroups(lead, period))
    assert lib.vds_attn_fwd_causal(C.byref(a), fr(16, 8), stream) == 0
    assert lib.vds_attn_fwd_causal(C.byref(a), None, stream) == 0
    for lead, period in ((-1, 4), (16, 0), (16, 5), (40, 1)):
        assert lib.vds_attn_fwd_causal(C.byref(a), fr(lead, period), stream) == -1, (lead, period)
        assert lib.vds_attn_bwd_causal(C.byref(a), fr(lead, period), stream) == -1, (lead, period)
    a.kv_pad_ones = 2
    assert lib.vds_attn_fwd_causal(C.byref(a), fr(16, 8), stream) == -1
    a.kv_pad_ones = 0
    a.Lk = 48
    assert lib.vds_attn_fwd_causal(C.byref(a), fr(16, 8), stream) == -1
    torch.cuda.synchronize()
