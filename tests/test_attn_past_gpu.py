"""Frame-causal attention forward with a past (vds_attn_fwd_causal_past) against fp32 torch on the CPU: scores
masked_fill(-inf) outside tests/helpers/frame_cache_ref.past_allowed, softmax.  Every forward family of the dispatcher, every
head dim, both layouts, every vds_attn_set_variant bit that reaches a forward kernel; outputs pre-filled with NaN; relative
Frobenius error at the tolerances of tests/test_attn_causal_gpu.py: o 6e-3, lse 1e-3.

Shapes: B = H = 2, lead = 16, (period, n) in {(1, 46), (2, 23), (3, 50)} -- Lq = 62 (no tile multiple) and 166 (more than one
128-row query tile) -- and past in {0, 23, 115, 300}: the plain frame-causal call (bit for bit), a past that ends inside the
first 64-key tile, a wholly past 32-key sub-block plus a straddling one, several wholly past tiles (the branch around the
mask)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_cache_ref as KC  # noqa: E402

FC = KC.FC
pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
TOL_O, TOL_LSE = 6e-3, 1e-3
B, H, LEAD = 2, 2, 16
SHAPES = {"p1_n46": (1, 46), "p2_n23": (2, 23), "p3_n50": (3, 50)}
PASTS = [0, 23, 115, 300]
MAX_PAST = max(PASTS)


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


_inputs, _refs = {}, {}


def inputs(hd, shape, past, trap=None):
    """bf16 CPU tensors q [B,H,Lq,hd], k, v [B,H,Lq + past,hd], shared and never modified.  The own rows and the first
    `past` of MAX_PAST past rows come from fixed seeds, so calls that differ in `past` only share their queries and own keys.
    trap = "past": the past keys x 32 and the past values 1000; "future": the K and V rows of the call's last frame x 32."""
    key = (hd, shape, past, trap)
    if key not in _inputs:
        period, n = SHAPES[shape]
        Lq = LEAD + n * period
        g = torch.Generator().manual_seed(301)
        q, ko, vo = (torch.randn(B, H, Lq, hd, generator=g).to(bf16) for _ in range(3))
        kp, vp = (torch.randn(B, H, MAX_PAST, hd, generator=g).to(bf16)[:, :, :past] for _ in range(2))
        if trap == "past":
            kp = (kp.float() * 32).to(bf16)  # exact in bf16
            vp = torch.full_like(vp, 1000.0)
        if trap == "future":
            last = KC.R.group_index(Lq, LEAD, period) == period
            ko, vo = ko.clone(), vo.clone()
            ko[:, :, last] = (ko[:, :, last].float() * 32).to(bf16)
            vo[:, :, last] = (vo[:, :, last].float() * 32).to(bf16)
        k = torch.cat([ko[:, :, :LEAD], kp, ko[:, :, LEAD:]], dim=2)
        v = torch.cat([vo[:, :, :LEAD], vp, vo[:, :, LEAD:]], dim=2)
        _inputs[key] = (q, k, v)
    return _inputs[key]


def reference(hd, shape, past, trap=None):
    """fp32 dense-mask attention, once per case: o [B,H,Lq,hd], lse [B,H,Lq]"""
    key = (hd, shape, past, trap)
    if key not in _refs:
        q, k, v = inputs(hd, shape, past, trap)
        period, n = SHAPES[shape]
        _refs[key] = FC.masked_attention(q.float(), k.float(), v.float(), KC.past_allowed(q.shape[2], LEAD, period, past))
    return _refs[key]


def padded(t, which):
    """[B,H,L,72] -> the padded rows [B,H,L,96] the qkv / RoPE kernel writes: zeros, K[72] = K[73] = 1, V[72] = V[76] = 1"""
    p = torch.zeros(*t.shape[:3], 96, dtype=bf16)
    p[..., :72] = t
    if which == "k":
        p[..., 72:74] = 1
    if which == "v":
        p[..., 72] = 1
        p[..., 76] = 1
    return p


def attn_args(q, k, v, o, lse, ones):
    from video_diffusion_speedrun_amd import _lib
    a = _lib.AttnArgs()
    a.B, a.H, a.Lq, a.Lk, a.head_dim = q.shape[0], q.shape[1], q.shape[2], k.shape[2], q.shape[3]
    for name, t in (("q", q), ("k", k), ("v", v), ("o", o)):
        setattr(a, name, t.data_ptr())
        for s, val in zip(("sb", "sh", "sl"), t.stride()[:3]):
            setattr(a, f"{name}_{s}", val)
    a.lse = lse.data_ptr()
    a.kv_pad_ones = int(ones)
    return a


def run(ops, hd, shape, past, ones=False, wide=False, variant=None, trap=None, entry=False):
    """the library on the shared inputs -> CPU o [B,H,Lq,hd], lse.  ones: the head-dim-72 layout (kv_pad_ones = 1); wide:
    knob attn_fwd_wide = 1 (the 64-queries-per-wave kernels, which short sequences reach only when forced); variant: the
    vds_attn_set_variant mask; entry: through the C entry point itself (ops.attn_fwd sends past = 0 to
    vds_attn_fwd_causal)."""
    q, k, v = inputs(hd, shape, past, trap)
    period, n = SHAPES[shape]
    Lq = q.shape[2]
    if ones:
        qd, kd, vd = padded(q, "q").cuda(), padded(k, "k").cuda(), padded(v, "v").cuda()
        qd, kd, vd = qd[..., :hd], kd[..., :hd], vd[..., :hd]
    else:
        qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    nan = float("nan")
    o = torch.full((B * Lq, H * hd), nan, dtype=bf16, device="cuda")
    lse = torch.full((B, H, Lq), nan, dtype=f32, device="cuda")
    ov = ops.heads_view(o, B, Lq, H, hd)
    prev_w = ops.knob_set("attn_fwd_wide", 1) if wide else None
    prev_v = ops.attn_set_variant(variant) if variant is not None else None
    try:
        if entry:
            from video_diffusion_speedrun_amd import _lib
            a = attn_args(qd, kd, vd, ov, lse, ones)
            rc = _lib.load().vds_attn_fwd_causal_past(C.byref(a), C.byref(_lib.ModGroups(LEAD, period)), past,
                                                      torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc
        else:
            ops.attn_fwd(qd, kd, vd, ov, lse, kv_pad_ones=ones, frames=(LEAD, period), past=past)
    finally:
        if prev_v is not None:
            ops.attn_set_variant(prev_v)
        if prev_w is not None:
            ops.knob_set("attn_fwd_wide", prev_w)
    torch.cuda.synchronize()
    return o.cpu().view(B, Lq, H, hd).permute(0, 2, 1, 3), lse.cpu()


def check(tag, got, ref):
    close(f"{tag}.o", got[0], ref[0], TOL_O)
    close(f"{tag}.lse", got[1], ref[1], TOL_LSE)


def same_bits(a, b):
    return torch.equal(a[0].contiguous().view(torch.int16), b[0].contiguous().view(torch.int16)) and \
        torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# kernel family -> (head dim, run() keywords).  attn_fwd_kernel: every head-dim instance of run_fwd, and head dim 72 in the
# ones-column layout; attn_fwd_wide_kernel<.., false>: head dims 64, 72, 96 (HDP 64 and 96) under the knob;
# attn_fwd_wide_kernel<.., true> / attn_fwd16_kernel: the ones-column layout under the knob, forward bit (4) of the variant
# mask off / on, the other bits both ways
FAMILIES = {
    "fwd_hd32": (32, {}), "fwd_hd64": (64, {}), "fwd_hd72": (72, {}), "fwd_hd96": (96, {}), "fwd_hd128": (128, {}),
    "fwd_hd72_ones": (72, dict(ones=True)),
    "wide_hd64": (64, dict(wide=True)), "wide_hd72": (72, dict(wide=True)), "wide_hd96": (96, dict(wide=True)),
    "wide_ones_mask0": (72, dict(ones=True, wide=True, variant=0)),
    "wide_ones_mask3": (72, dict(ones=True, wide=True, variant=3)),
    "fwd16_mask4": (72, dict(ones=True, wide=True, variant=4)),
    "fwd16_mask7": (72, dict(ones=True, wide=True, variant=7)),
    "fwd16_default": (72, dict(ones=True, wide=True)),
}


@pytest.mark.parametrize("past", PASTS)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_kernels_against_the_dense_mask(ops, family, shape, past):
    hd, kw = FAMILIES[family]
    got = run(ops, hd, shape, past, **kw)
    check(f"{family}.{shape}.past{past}", got, reference(hd, shape, past))
    if past == 0:  # the entry point forwards to vds_attn_fwd_causal: the same bits
        assert same_bits(run(ops, hd, shape, 0, entry=True, **kw), got)
    else:  # ... and ops.attn_fwd calls it
        assert same_bits(run(ops, hd, shape, past, entry=True, **kw), got)


TRAPPED = ["fwd_hd64", "fwd_hd72", "fwd_hd128", "fwd_hd72_ones", "wide_hd64", "wide_hd96", "wide_ones_mask0", "fwd16_default"]


@pytest.mark.parametrize("past", [23, 115, 300])
@pytest.mark.parametrize("family", TRAPPED)
def test_past_keys_stay_out_of_the_register_queries(ops, family, past):
    """the past keys x 32 and the past values 1000: their scores and values dwarf everything, but the register queries'
    rows of o and lse equal those of the same call without a past -- a past key enters neither the maximum nor the sum of a
    register query"""
    hd, kw = FAMILIES[family]
    o, lse = run(ops, hd, "p3_n50", past, trap="past", **kw)
    o0, lse0 = run(ops, hd, "p3_n50", 0, **kw)
    close(f"reg.{family}.past{past}.o", o[:, :, :LEAD], o0[:, :, :LEAD], TOL_O)
    close(f"reg.{family}.past{past}.lse", lse[:, :, :LEAD], lse0[:, :, :LEAD], TOL_LSE)
    ro, rl = reference(hd, "p3_n50", past, trap="past")
    close(f"reg.{family}.past{past}.o.ref", o[:, :, :LEAD], ro[:, :, :LEAD], TOL_O)
    close(f"reg.{family}.past{past}.lse.ref", lse[:, :, :LEAD], rl[:, :, :LEAD], TOL_LSE)
    assert float(o[:, :, LEAD:].float().abs().median()) > 100  # (the token queries do see them)


@pytest.mark.parametrize("past", [23, 115, 300])
@pytest.mark.parametrize("family", TRAPPED)
def test_own_future_frame_keys_stay_out_of_the_maximum(ops, family, past):
    """the K and V rows of the call's last frame x 32: no query of an earlier frame may see them -- a kernel that masked
    after its running maximum, or compared a key with the wrong row behind the past, would underflow the attended keys"""
    hd, kw = FAMILIES[family]
    o, lse = run(ops, hd, "p3_n50", past, trap="future", **kw)
    ro, rl = reference(hd, "p3_n50", past, trap="future")
    rows = KC.R.group_index(LEAD + 150, LEAD, 3) < 3
    close(f"future.{family}.past{past}.o", o[:, :, rows], ro[:, :, rows], TOL_O)
    close(f"future.{family}.past{past}.lse", lse[:, :, rows], rl[:, :, rows], TOL_LSE)


@pytest.mark.parametrize("family", ["fwd_hd64", "fwd_hd72_ones", "wide_hd64", "fwd16_default"])
def test_a_token_query_lse_grows_with_the_past(ops, family):
    hd, kw = FAMILIES[family]
    prev = None
    for past in PASTS:
        lse = run(ops, hd, "p2_n23", past, **kw)[1]
        if prev is not None:
            assert (lse[:, :, LEAD:] > prev[:, :, LEAD:]).all(), past
            close(f"lse_reg.{family}.past{past}", lse[:, :, :LEAD], prev[:, :, :LEAD], TOL_LSE)
        prev = lse


def test_argument_errors(ops):
    from video_diffusion_speedrun_amd import _lib
    hd, Lq, past = 64, 48, 24
    q = torch.zeros(B, H, Lq, hd, dtype=bf16, device="cuda")
    k = torch.zeros(B, H, Lq + past, hd, dtype=bf16, device="cuda")
    o, lse = torch.zeros_like(q), torch.zeros(B, H, Lq, dtype=f32, device="cuda")
    with pytest.raises(ValueError, match="past"):
        ops.attn_fwd(q, k[:, :, :-1], k[:, :, :-1], o, lse, frames=(16, 8), past=past)
    with pytest.raises(ValueError, match="past"):
        ops.attn_fwd(q, k, k, o, lse, past=past)
    with pytest.raises(ValueError, match="past"):
        ops.attn_fwd(q, q, q, o, lse, frames=(16, 8), past=-1)
    with pytest.raises(_lib.VdsError):  # the cross-attention layout has no frames
        ops.attn_fwd(q, k, k, o, lse, kv_pad_ones=2, frames=(16, 8), past=past)
    # the C entry point itself
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    fr = lambda lead, period: C.byref(_lib.ModGroups(lead, period))
    call = lambda a, f, p: lib.vds_attn_fwd_causal_past(C.byref(a), f, p, stream)
    a = attn_args(q, k, k, o, lse, 0)
    assert call(a, fr(16, 8), past) == 0
    assert call(a, None, past) == -1  # no frames with a past
    assert call(a, fr(16, 8), -1) == -1
    assert call(a, fr(16, 8), past - 1) == -1 and call(a, fr(16, 8), past + 1) == -1  # Lk != Lq + past
    for lead, period in ((-1, 4), (16, 0), (16, 5), (49, 1)):  # the (lead, period) checks, against Lq
        assert call(a, fr(lead, period), past) == -1, (lead, period)
    a.kv_pad_ones = 2
    assert call(a, fr(16, 8), past) == -1
    a.kv_pad_ones = 0
    a0 = attn_args(q, q, q, o, lse, 0)
    assert call(a0, fr(16, 8), 0) == 0 and call(a0, None, 0) == 0  # past = 0: vds_attn_fwd_causal, NULL frames included
    a.Lq, a.Lk = 16 + 8 * (1 << 18), 16 + 8 * (1 << 18) + past  # > 2^21 key rows: refused before anything is launched
    assert call(a, fr(16, 8), past) == -2
    torch.cuda.synchronize()


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "qk_norm"])
@pytest.mark.parametrize("hd,hdp", [(72, 96), (64, 64)])
def test_qkv_rope_cache_form_writes_the_rows_in_place(ops, hd, hdp, norm):
    """vds_qkv_rope_fwd_cache / _norm_fwd_cache against the plain forms: q bit for bit, the k / v rows bit for bit at row
    (l < lead ? l : l + past) of strided cache buffers (pad and ones columns included), every other row untouched; v0 is
    read through the same map"""
    Bq, Hq, L, lead, past, rows = 2, 2, 16 + 21, 16, 19, 80
    D = Hq * hd
    g = torch.Generator().manual_seed(77)
    qkv = torch.randn(Bq * L, 3 * D, generator=g).to(bf16).cuda()
    ang = torch.rand(L, hd // 2, generator=g) * 6.28
    cos, sin = ang.cos().cuda(), ang.sin().cuda()
    lam = torch.tensor([0.75], dtype=bf16, device="cuda")
    v0 = torch.randn(Bq, Hq, L, hdp, generator=g).to(bf16).cuda()
    plain = ops.qkv_rope_norm_fwd if norm else ops.qkv_rope_fwd
    cached = ops.qkv_rope_norm_fwd_cache if norm else ops.qkv_rope_fwd_cache
    idx = torch.cat([torch.arange(lead), lead + past + torch.arange(L - lead)]).cuda()
    for mix in (False, True):
        q, k, v = plain(qkv, cos, sin, v0 if mix else None, lam if mix else None, Bq, L, Hq, hd, hdp)
        big = torch.full((3, Bq, Hq, rows, hdp + 8), 7.0, dtype=bf16, device="cuda")  # row stride hdp + 8: not contiguous
        kb, vb, v0b = (big[i, ..., :hdp] for i in range(3))
        v0b[:, :, idx] = v0
        qc = cached(qkv, cos, sin, v0b if mix else None, lam if mix else None, kb, vb, lead, past, Bq, L, Hq, hd, hdp)
        torch.cuda.synchronize()
        assert torch.equal(qc.view(torch.int16), q.view(torch.int16))
        assert torch.equal(kb[:, :, idx].contiguous().view(torch.int16), k.view(torch.int16))
        assert torch.equal(vb[:, :, idx].contiguous().view(torch.int16), v.view(torch.int16))
        other = torch.ones(rows, dtype=torch.bool, device="cuda")
        other[idx] = False
        assert (kb[:, :, other] == 7).all() and (vb[:, :, other] == 7).all()
        assert (big[0, ..., hdp:] == 7).all() and (big[1, ..., hdp:] == 7).all()
