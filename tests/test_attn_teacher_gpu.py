"""Teacher-forcing frame-major attention on the GPU: vds_teacher_attn_fwd / vds_teacher_attn_bwd through the whole frame-major
path -- token-major qkv -> the frame-major qkv / RoPE kernel (identity rotation, period 2n) -> frame-major q, k, v, lse, dq,
dk, dv with TOKEN-major o and dO -- against fp32 torch attention in TOKEN order under the dense teacher mask of
tests/helpers/teacher_ref.py, at the bounds of tests/test_attn_frame_window_gpu.py (imported from
tests/test_attn_frame_major_gpu.py): o 6e-3, lse 1e-3, gradients 8e-3 (relative Frobenius norm).  Also: the clean half's o and
lse against the _fm_chunk call on the first base rows, bit for bit; containment -- traps on every token row a noisy chunk
does not attend leave its o, lse and dq bit-identical; every call twice to equal bits; a captured forward + backward; the
refusals on live buffers.

Shapes (L, lead, period, c) are teacher_ref.SHAPES, B = H = 2.  HEADS is tests/test_attn_frame_major_gpu.py's: every head dim
of the dispatcher, and the ones layout at head dim 72 under every variant mask and knob setting of that table -- the TF
runners take the plain 32x32x16 TF kernels under all of them."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_major_ref as FM  # noqa: E402
import teacher_ref as TR  # noqa: E402
from test_attn_frame_major_gpu import AB, AH, HEADS, NAMES, TOL_G, TOL_LSE, TOL_O, TOLS, Variant, heads_of, rel, same  # noqa: E402

FC = TR.FC
pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
ids = TR.ids


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import _lib, ops
    return dict(ops=ops, lib=_lib)


_ain, _aref = {}, {}


def outside_tok(L, lead, period, c, i):
    """bool [L], token rows: the token rows that NOISY chunk i does not attend -- the clean chunks from its own on and every
    other noisy chunk"""
    keep = TR.allowed_tok(L, lead, period, c)
    n = period // 2
    l = torch.arange(L)
    f = (l - lead).clamp(min=0) % period
    mine = (l >= lead) & (f >= n) & ((f - n) // min(c, n) == i)
    return ~keep[mine].any(dim=0), mine


def attn_inputs(hd, L, trap=None, seed=0):
    """(qkv [B*L, 3D], dO [B*L, D]) bf16 in token order.  trap = (lead, period, c, i): the token rows outside what noisy chunk
    i attends carry OTHER values -- q and dO redrawn, K redrawn and scaled by 32, V = 1000; seed: another draw of them"""
    key = (hd, L, trap, seed)
    if key not in _ain:
        D = AH * hd
        g = torch.Generator().manual_seed(9300 + hd + L)
        qkv, do = torch.randn(AB * L, 3 * D, generator=g).to(bf16), torch.randn(AB * L, D, generator=g).to(bf16)
        if trap is not None:
            g = torch.Generator().manual_seed(78 + seed)
            sel = outside_tok(L, *trap)[0].repeat(AB)
            n = int(sel.sum())
            qkv, do = qkv.clone(), do.clone()
            qkv[sel, :D] = torch.randn(n, D, generator=g).to(bf16)
            qkv[sel, D:2 * D] = (torch.randn(n, D, generator=g) * 32).to(bf16)
            qkv[sel, 2 * D:] = 1000.0
            do[sel] = torch.randn(n, D, generator=g).to(bf16)
        _ain[key] = (qkv, do)
    return _ain[key]


def attn_reference(hd, shape, trap=None):
    """fp32 torch under the dense teacher mask, token rows, once per case"""
    key = (hd, shape, trap)
    if key not in _aref:
        L, lead, period, c = shape
        qkv, do = attn_inputs(hd, L, trap)
        D = AH * hd
        q, k, v = (heads_of(qkv, AB, L, AH, hd, i * D).float().requires_grad_(True) for i in range(3))
        o, lse = FC.masked_attention(q, k, v, TR.allowed_tok(L, lead, period, c))
        o.backward(heads_of(do, AB, L, AH, hd).float())
        _aref[key] = (o.detach(), lse.detach(), q.grad, k.grad, v.grad)
    return _aref[key]


def clean_rows_tok(L, lead, period):
    """token rows of the lead rows and the clean frames, in the token order of the sequence without its noisy half"""
    l = torch.arange(L)
    return l[(l < lead) | (((l - lead) % period) < period // 2)]


def attn_run(ops, head, shape, trap=None, seed=0, graph=False, clean_only=False, bwd=True):
    """the library on the shared inputs -> CPU o [B,H,L,hd] (token rows), lse, dq, dk, dv (frame-major rows).
    clean_only: the _fm_chunk call on the lead rows and the clean frames alone (period n, the first base rows), forward"""
    hd, hdp, ones, kn = HEADS[head]
    L, lead, period, c = shape
    D = AH * hd
    qkv, do = (t.cuda() for t in attn_inputs(hd, L, trap, seed))
    akw = dict(kv_pad_ones=ones, frames=(lead, period), frame_major=True, chunk=c, teacher=True)
    if clean_only:
        rows = clean_rows_tok(L, lead, period).cuda()
        n = period // 2
        qkv = qkv.view(AB, L, 3 * D)[:, rows].reshape(-1, 3 * D).contiguous()
        do = do.view(AB, L, D)[:, rows].reshape(-1, D).contiguous()
        L, period = int(rows.numel()), n
        akw = dict(kv_pad_ones=ones, frames=(lead, n), frame_major=True, chunk=min(c, n))
        bwd = False
    cos = torch.ones(L, hd // 2, dtype=f32, device="cuda")
    sin = torch.zeros(L, hd // 2, dtype=f32, device="cuda")
    qp, kp, vp = ops.qkv_rope_fwd(qkv, cos, sin, None, None, AB, L, AH, hd, hdp, frames=(lead, period))
    nan = float("nan")
    o = torch.full((AB * L, D), nan, dtype=bf16, device="cuda")
    lse = torch.full((AB, AH, L), nan, dtype=f32, device="cuda")
    dqb, dkb, dvb = (torch.full((AB, AH, L, hdp), nan, dtype=bf16, device="cuda") for _ in range(3))
    ov, dov = ops.heads_view(o, AB, L, AH, hd), ops.heads_view(do, AB, L, AH, hd)
    delta = torch.empty(ops.attn_bwd_workspace_floats(AB, AH, L, L, hd, ones), dtype=f32, device="cuda")

    def step():
        ops.attn_fwd(qp[..., :hd], kp[..., :hd], vp[..., :hd], ov, lse, **akw)
        if bwd:
            ops.attn_bwd(qp[..., :hd], kp[..., :hd], vp[..., :hd], ov, lse, dov, dqb[..., :hd], dkb[..., :hd], dvb[..., :hd],
                         delta, **akw)
    with Variant(ops, kn):
        if graph:
            step()  # (loads the kernels outside the capture)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                step()
            for t in (o, lse, dqb, dkb, dvb):
                t.fill_(nan)
            gr.replay()
        else:
            step()
        torch.cuda.synchronize()
    return [heads_of(o.cpu(), AB, L, AH, hd), lse.cpu()] + [t[..., :hd].cpu() for t in (dqb, dkb, dvb)]


def to_fm(ref, shape):
    """the token-order reference in the rows a frame-major call uses: o stays, lse / dq / dk / dv rows permuted"""
    tok = FM.tok_index(*shape[:3])
    return [ref[0], ref[1][:, :, tok]] + [t[:, :, tok] for t in ref[2:]]


@pytest.mark.parametrize("head", list(HEADS))
@pytest.mark.parametrize("shape", TR.SHAPES, ids=ids)
def test_attention_against_fp32_attention_under_the_teacher_mask(vds, shape, head):
    got = attn_run(vds["ops"], head, shape)
    again = attn_run(vds["ops"], head, shape)
    ref = to_fm(attn_reference(HEADS[head][0], shape), shape)
    errs = []
    for name, g_, r_ in zip(NAMES, got, ref):
        assert torch.isfinite(g_.float()).all(), f"{name}: an element was left unwritten or is not finite"
        errs.append(rel(g_, r_))
    print(ids(shape), head, " ".join(f"{n} {e:.2e}" for n, e in zip(NAMES, errs)))
    for name, e, tol in zip(NAMES, errs, TOLS):
        assert e < tol, f"{name}: rel {e:.3e} >= {tol:.1e}"
    for name, a, b in zip(NAMES, got, again):  # no atomics: every call twice gives equal bits
        assert same(a.contiguous(), b.contiguous()), (name, "run to run")


def test_the_teacher_mask_changes_the_result(vds):
    """the flag is read: the chunk-causal result on the same rows is far outside the bounds on the noisy half"""
    shape = TR.SHAPES[1]
    L, lead, period, c = shape
    ops = vds["ops"]
    got = attn_run(ops, "hd64", shape)
    hd, hdp, ones, kn = HEADS["hd64"]
    qkv, _ = (t.cuda() for t in attn_inputs(hd, L))
    cos = torch.ones(L, hd // 2, dtype=f32, device="cuda")
    sin = torch.zeros(L, hd // 2, dtype=f32, device="cuda")
    qp, kp, vp = ops.qkv_rope_fwd(qkv, cos, sin, None, None, AB, L, AH, hd, hdp, frames=(lead, period))
    o = torch.zeros(AB * L, AH * hd, dtype=bf16, device="cuda")
    lse = torch.zeros(AB, AH, L, dtype=f32, device="cuda")
    ops.attn_fwd(qp, kp, vp, ops.heads_view(o, AB, L, AH, hd), lse, frames=(lead, period), frame_major=True, chunk=c)
    torch.cuda.synchronize()
    base = lead + (period // 2) * ((L - lead) // period)
    assert rel(got[1][:, :, base:], lse.cpu()[:, :, base:]) > 10 * TOL_LSE


# (the heads whose _fm_chunk forward is the plain 32x32x16 kernel too: the same arithmetic per row)
@pytest.mark.parametrize("head", ["hd32", "hd64", "hd72", "hd96", "hd128", "hd72_ones", "ones_mfma32"])
@pytest.mark.parametrize("shape", TR.SHAPES, ids=ids)
def test_the_clean_half_is_the_fm_chunk_call_on_the_first_base_rows_bit_for_bit(vds, shape, head):
    """o and lse of the lead rows and the clean frames: what vds_attn_fwd_causal_fm_chunk computes on those rows alone"""
    L, lead, period, c = shape
    base = TR.geometry(*shape)[3]
    got = attn_run(vds["ops"], head, shape, bwd=False)
    want = attn_run(vds["ops"], head, shape, clean_only=True)
    rows = clean_rows_tok(L, lead, period)
    assert int(rows.numel()) == base
    assert same(got[1][:, :, :base].contiguous(), want[1].contiguous()), "lse of the clean half"
    assert same(got[0][:, :, rows].contiguous(), want[0].contiguous()), "o of the clean half"


@pytest.mark.parametrize("head", ["hd32", "hd64", "hd96", "hd128", "hd72_ones"])
@pytest.mark.parametrize("shape", TR.SHAPES, ids=ids)
def test_rows_a_noisy_chunk_does_not_attend_change_nothing_bit_for_bit_and_traps_stay_out(vds, shape, head):
    """K x 32 and V = 1000 on every token row that noisy chunk i does not attend -- its own clean chunk and the later ones,
    every other noisy chunk -- and two different draws of those rows' Q / K / dO: o, lse and dq of the rows of noisy chunk i
    are bit-identical, to each other and to the untrapped run; the trapped problem still matches its own reference there"""
    L, lead, period, c = shape
    n, S, G, base = TR.geometry(*shape)
    hd = HEADS[head][0]
    n_chunks = -(-n * S // G)
    plain = attn_run(vds["ops"], head, shape)
    for i in sorted({0, n_chunks // 2, n_chunks - 1}):
        trap = (lead, period, c, i)
        out_tok, keep_tok = outside_tok(L, *trap)
        assert int(out_tok.sum()) >= min(G, n * S) and not (out_tok & keep_tok).any()
        got = attn_run(vds["ops"], head, shape, trap=trap)
        again = attn_run(vds["ops"], head, shape, trap=trap, seed=1)
        r0, r1 = base + i * G, min(L, base + (i + 1) * G)  # frame-major rows of noisy chunk i
        rows = slice(r0, r1)
        assert int(keep_tok.sum()) == r1 - r0
        for other in (plain, again):
            assert same(got[0][:, :, keep_tok].contiguous(), other[0][:, :, keep_tok].contiguous()), ("o", i)
            assert same(got[1][:, :, rows].contiguous(), other[1][:, :, rows].contiguous()), ("lse", i)
            assert same(got[2][:, :, rows].contiguous(), other[2][:, :, rows].contiguous()), ("dq", i)
        assert not same(got[0], plain[0]) and not same(got[1], again[1]), "the trapped rows did not change"
        assert float(got[0][:, :, keep_tok].float().abs().max()) < 100.0  # V = 1000 stayed out
        ref = to_fm(attn_reference(hd, shape, trap), shape)
        assert rel(got[0][:, :, keep_tok], ref[0][:, :, keep_tok]) < TOL_O
        assert rel(got[1][:, :, rows], ref[1][:, :, rows]) < TOL_LSE
        assert rel(got[2][:, :, rows], ref[2][:, :, rows]) < TOL_G


def test_graph_replay(vds):
    """lead, period and the chunk travel by value: a captured forward + backward replays to the eager bits"""
    ops = vds["ops"]
    for head, shape in (("hd72_ones", TR.SHAPES[3]), ("hd64", TR.SHAPES[4]), ("hd128", TR.SHAPES[2])):
        eager = attn_run(ops, head, shape)
        replay = attn_run(ops, head, shape, graph=True)
        for name, a, b in zip(NAMES, eager, replay):
            assert same(a.contiguous(), b.contiguous()), (head, name)


def test_argument_errors_on_live_buffers(vds):
    ops, _lib = vds["ops"], vds["lib"]
    L, hd = 154, 64
    q = torch.zeros(1, 2, L, hd, dtype=bf16, device="cuda")
    o = torch.zeros(1 * L, 2 * hd, dtype=bf16, device="cuda")
    lse = torch.zeros(1, 2, L, dtype=f32, device="cuda")
    ov = ops.heads_view(o, 1, L, 2, hd)
    with pytest.raises(ValueError, match="teacher=True needs frame_major=True"):
        ops.attn_fwd(q, q, q, ov, lse, frames=(16, 6), teacher=True)
    with pytest.raises(ValueError, match="excludes window"):
        ops.attn_fwd(q, q, q, ov, lse, frames=(16, 6), frame_major=True, window=2, teacher=True)
    with pytest.raises(ValueError, match="even period"):
        ops.attn_fwd(q, q, q, ov, lse, frames=(16, 3), frame_major=True, teacher=True)
    with pytest.raises(ValueError, match="do not fit"):
        ops.attn_fwd(q, q, q, ov, lse, frames=(16, 4), frame_major=True, teacher=True)
    a = _lib.AttnArgs()
    a.B, a.H, a.Lq, a.Lk, a.head_dim = 1, 2, L, L, hd
    for f, t in (("q", q), ("k", q), ("v", q), ("o", ov)):
        setattr(a, f, t.data_ptr())
        s = (t.stride(0), t.stride(1), t.stride(2))
        setattr(a, f + "_sb", s[0]), setattr(a, f + "_sh", s[1]), setattr(a, f + "_sl", s[2])
    a.lse = lse.data_ptr()
    lib = _lib.load()
    fr = C.byref(_lib.ModGroups(16, 6))
    lse.fill_(7.0)
    assert lib.vds_teacher_attn_fwd(C.byref(a), fr, 0, None) == -1
    assert lib.vds_teacher_attn_fwd(C.byref(a), None, 1, None) == -1
    assert lib.vds_teacher_attn_fwd(C.byref(a), C.byref(_lib.ModGroups(16, 3)), 1, None) == -1   # an odd period
    assert lib.vds_teacher_attn_fwd(C.byref(a), C.byref(_lib.ModGroups(16, 4)), 1, None) == -1   # does not fit
    assert lib.vds_teacher_attn_bwd(C.byref(a), fr, 1, None) == -1                              # no gradient buffers
    torch.cuda.synchronize()
    assert float(lse.min()) == 7.0 and float(o.abs().max()) == 0.0, "a refused call wrote"
