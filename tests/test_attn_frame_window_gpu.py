"""Sliding-window chunk-causal frame-major attention on the GPU: vds_attn_fwd_causal_fm_window /
vds_attn_bwd_causal_fm_window through the whole frame-major path -- token-major qkv -> the frame-major qkv / RoPE kernel
(identity rotation) -> frame-major q, k, v, lse, dq, dk, dv with TOKEN-major o and dO -- against fp32 torch attention in
TOKEN order under the dense window mask of tests/helpers/frame_window_ref.py, at the bounds
tests/test_attn_frame_chunk_gpu.py uses for the same kernel families: o 6e-3, lse 1e-3, gradients 8e-3 (relative Frobenius
norm).  Also: a window of every chunk through the new entry points against the _fm_chunk calls, bit for bit; containment --
traps on every token row outside a chunk's window leave o, lse and dq of that chunk bit-identical, while K / V inside the
window and in the lead rows move them; a captured forward + backward; the refusals on live buffers.

Shapes (L, lead, period, c, w) are frame_window_ref.SHAPES, B = H = 2.  HEADS is tests/test_attn_frame_major_gpu.py's: every
head dim of the dispatcher, and the ones layout at head dim 72 under the variant masks 7 / 5 / 2 / 0, attn_delta_fold 0 / 1
and attn_fwd_wide = 1, which reach every WIN kernel family at small L (the table in that module)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_chunk_ref as CH  # noqa: E402
import frame_major_ref as FM  # noqa: E402
import frame_window_ref as FW  # noqa: E402
from test_attn_frame_major_gpu import AB, AH, HEADS, NAMES, TOL_G, TOL_LSE, TOL_O, TOLS, Variant, heads_of, rel, same  # noqa: E402

FC = CH.FC
pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
ids = FW.ids


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import _lib, ops
    return dict(ops=ops, lib=_lib)


_ain, _aref = {}, {}


def outside_tok(L, lead, period, c, W, n):
    """bool [L], token rows: the token rows of the chunks that chunk n does not attend -- before its window or after it"""
    g = CH.group_index_tok(L, lead, period, c) - 1  # chunk of a token row, -1: a lead row
    return (g >= 0) & ((g < n - W + 1) | (g > n))


def attn_inputs(hd, L, trap=None, seed=0):
    """(qkv [B*L, 3D], dO [B*L, D]) bf16 in token order.  trap = (lead, period, c, W, n): the token rows outside the window
    of chunk n carry OTHER values -- q and dO redrawn, K redrawn and scaled by 32, V = 1000; seed: another draw of them"""
    key = (hd, L, trap, seed)
    if key not in _ain:
        D = AH * hd
        g = torch.Generator().manual_seed(9100 + hd + L)
        qkv, do = torch.randn(AB * L, 3 * D, generator=g).to(bf16), torch.randn(AB * L, D, generator=g).to(bf16)
        if trap is not None:
            g = torch.Generator().manual_seed(78 + seed)
            sel = outside_tok(L, *trap).repeat(AB)
            n = int(sel.sum())
            qkv, do = qkv.clone(), do.clone()
            qkv[sel, :D] = torch.randn(n, D, generator=g).to(bf16)
            qkv[sel, D:2 * D] = (torch.randn(n, D, generator=g) * 32).to(bf16)
            qkv[sel, 2 * D:] = 1000.0
            do[sel] = torch.randn(n, D, generator=g).to(bf16)
        _ain[key] = (qkv, do)
    return _ain[key]


def attn_reference(hd, shape, trap=None):
    """fp32 torch under the dense window mask, token rows, once per case"""
    key = (hd, shape, trap)
    if key not in _aref:
        L, lead, period, c, w = shape
        qkv, do = attn_inputs(hd, L, trap)
        D = AH * hd
        q, k, v = (heads_of(qkv, AB, L, AH, hd, i * D).float().requires_grad_(True) for i in range(3))
        o, lse = FC.masked_attention(q, k, v, FW.allowed_tok(L, lead, period, c, w))
        o.backward(heads_of(do, AB, L, AH, hd).float())
        _aref[key] = (o.detach(), lse.detach(), q.grad, k.grad, v.grad)
    return _aref[key]


def attn_run(ops, head, shape, trap=None, seed=0, graph=False, window="shape", edit=None):
    """the library on the shared inputs -> CPU o [B,H,L,hd] (token rows), lse, dq, dk, dv (frame-major rows).
    window: the window in chunks passed to the library (default: the shape's; None: the _fm_chunk call);
    edit(qkv, do): changes the device inputs in place"""
    hd, hdp, ones, kn = HEADS[head]
    L, lead, period, c, w = shape
    D = AH * hd
    qkv, do = (t.cuda() for t in attn_inputs(hd, L, trap, seed))
    if edit is not None:
        edit(qkv, do)
    cos = torch.ones(L, hd // 2, dtype=f32, device="cuda")
    sin = torch.zeros(L, hd // 2, dtype=f32, device="cuda")
    qp, kp, vp = ops.qkv_rope_fwd(qkv, cos, sin, None, None, AB, L, AH, hd, hdp, frames=(lead, period))
    nan = float("nan")
    o = torch.full((AB * L, D), nan, dtype=bf16, device="cuda")
    lse = torch.full((AB, AH, L), nan, dtype=f32, device="cuda")
    dqb, dkb, dvb = (torch.full((AB, AH, L, hdp), nan, dtype=bf16, device="cuda") for _ in range(3))
    ov, dov = ops.heads_view(o, AB, L, AH, hd), ops.heads_view(do, AB, L, AH, hd)
    delta = torch.empty(ops.attn_bwd_workspace_floats(AB, AH, L, L, hd, ones), dtype=f32, device="cuda")
    akw = dict(kv_pad_ones=ones, frames=(lead, period), frame_major=True, chunk=c)
    if window is not None:
        akw["window"] = w // c if window == "shape" else window

    def step():
        ops.attn_fwd(qp[..., :hd], kp[..., :hd], vp[..., :hd], ov, lse, **akw)
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
@pytest.mark.parametrize("shape", FW.SHAPES, ids=ids)
def test_attention_against_fp32_attention_under_the_window_mask(vds, shape, head):
    got = attn_run(vds["ops"], head, shape)
    ref = to_fm(attn_reference(HEADS[head][0], shape), shape)
    errs = []
    for name, g_, r_ in zip(NAMES, got, ref):
        assert torch.isfinite(g_.float()).all(), f"{name}: an element was left unwritten or is not finite"
        errs.append(rel(g_, r_))
    print(ids(shape), head, " ".join(f"{n} {e:.2e}" for n, e in zip(NAMES, errs)))
    for name, e, tol in zip(NAMES, errs, TOLS):
        assert e < tol, f"{name}: rel {e:.3e} >= {tol:.1e}"


def test_the_window_changes_the_result(vds):
    """the window is read: the chunk-causal result on the same inputs is far outside the bounds"""
    shape = (280, 16, 8, 2, 4)
    got, plain = attn_run(vds["ops"], "hd64", shape), attn_run(vds["ops"], "hd64", shape, window=None)
    assert rel(got[0], plain[0]) > 10 * TOL_O


@pytest.mark.parametrize("head", ["hd64", "hd128", "hd72_ones", "ones_all16_fold", "ones_all16_delta", "ones_mfma32"])
def test_a_window_of_every_chunk_is_the_fm_chunk_call_bit_for_bit(vds, head):
    ops = vds["ops"]
    for shape in ((280, 16, 8, 2, 4), (280, 16, 8, 1, 3), (1040, 16, 8, 2, 2)):
        n = -(-shape[2] // shape[3])  # chunks of the sequence
        want = attn_run(ops, head, shape, window=None)  # ops routes to vds_attn_*_causal_fm_chunk / _fm
        for W in (n, n + 3):
            got = attn_run(ops, head, shape, window=W)  # vds_attn_*_causal_fm_window
            for name, a, b in zip(NAMES, got, want):
                assert same(a.contiguous(), b.contiguous()), (head, shape, W, name)
        assert not same(attn_run(ops, head, shape, window=n - 1)[1], want[1])  # one chunk less: the WIN instances


@pytest.mark.parametrize("head", ["hd32", "hd96", "hd72_ones", "ones_all16_fold", "ones_all16_delta", "ones_fwd16_dkv16",
                                  "ones_dq16"])
@pytest.mark.parametrize("shape", [(166, 16, 3, 1, 2), (280, 16, 8, 1, 3), (280, 16, 8, 2, 4), (280, 16, 8, 3, 3),
                                   (203, 0, 7, 1, 2), (293, 33, 4, 1, 2), (1040, 16, 8, 1, 2)], ids=ids)
def test_rows_outside_the_window_change_nothing_bit_for_bit_and_traps_stay_out(vds, shape, head):
    """K x 32 and V = 1000 on every token row outside the window of chunk n -- the chunks before it and after it -- and two
    different draws of those rows' Q / K / dO: o, lse and dq of the rows of chunk n are bit-identical, to each other and to
    the untrapped run; the trapped problem still matches its own reference on those rows"""
    L, lead, period, c, w = shape
    S = (L - lead) // period
    W = w // c
    hd = HEADS[head][0]
    n_chunks = -(-period // c)
    base = attn_run(vds["ops"], head, shape)
    ran = 0
    for n in sorted({W, (n_chunks + W) // 2, n_chunks - 1}):  # chunks with rows before their window
        if not W <= n < n_chunks:
            continue
        trap = (lead, period, c, W, n)
        got = attn_run(vds["ops"], head, shape, trap=trap)
        again = attn_run(vds["ops"], head, shape, trap=trap, seed=1)
        r0, r1 = lead + n * c * S, min(L, lead + (n + 1) * c * S)  # frame-major rows of chunk n
        rows = slice(r0, r1)
        keep_tok = CH.group_index_tok(L, lead, period, c) == n + 1
        assert int(keep_tok.sum()) == r1 - r0 and int(outside_tok(L, *trap).sum()) >= c * S
        for other in (base, again):
            assert same(got[0][:, :, keep_tok].contiguous(), other[0][:, :, keep_tok].contiguous()), ("o", n)
            assert same(got[1][:, :, rows].contiguous(), other[1][:, :, rows].contiguous()), ("lse", n)
            assert same(got[2][:, :, rows].contiguous(), other[2][:, :, rows].contiguous()), ("dq", n)
        assert not same(got[0], base[0]) and not same(got[1], again[1]), "the rows outside the window did not change"
        assert float(got[0][:, :, keep_tok].float().abs().max()) < 100.0  # V = 1000 stayed out
        ref = to_fm(attn_reference(hd, shape, trap), shape)
        assert rel(got[0][:, :, keep_tok], ref[0][:, :, keep_tok]) < TOL_O
        assert rel(got[1][:, :, rows], ref[1][:, :, rows]) < TOL_LSE
        assert rel(got[2][:, :, rows], ref[2][:, :, rows]) < TOL_G
        ran += 1
    assert ran, "no chunk was trapped"


@pytest.mark.parametrize("head", ["hd64", "hd72_ones", "ones_all16_fold"])
@pytest.mark.parametrize("shape", [(280, 16, 8, 1, 3), (280, 16, 8, 2, 4), (1040, 16, 8, 1, 2)], ids=ids)
def test_keys_inside_the_window_and_lead_keys_are_seen(vds, shape, head):
    """other K / V on the FIRST chunk of the last chunk's window, and on the lead rows, move lse of the last chunk; other
    K / V on the chunk just before that window move it by exactly nothing"""
    L, lead, period, c, w = shape
    S = (L - lead) // period
    W = w // c
    hd = HEADS[head][0]
    D = AH * hd
    n = -(-period // c) - 1  # the last chunk
    grp = CH.group_index_tok(L, lead, period, c)
    rows = slice(lead + n * c * S, L)
    base = attn_run(vds["ops"], head, shape)

    def moved(sel):
        sel = sel.repeat(AB).cuda()

        def edit(qkv, do):
            qkv[sel, D:] = (qkv[sel, D:].float() * -3.0 + 0.25).to(bf16)
        b = attn_run(vds["ops"], head, shape, edit=edit)
        return b[1][:, :, rows], rel(b[1][:, :, rows], base[1][:, :, rows])
    _, d_in = moved(grp == n - W + 2)       # chunk n - W + 1, the window's first
    _, d_lead = moved(grp == 0)
    out, d_out = moved(grp == n - W + 1)    # chunk n - W, just outside
    print(ids(shape), head, f"lse of the last chunk moves by {d_in:.3e} (window's first chunk), {d_lead:.3e} (lead), {d_out}")
    assert d_in > 10 * TOL_LSE and d_lead > 10 * TOL_LSE
    assert same(out.contiguous(), base[1][:, :, rows].contiguous())


def test_graph_replay(vds):
    """lead, period, the chunk and the window travel by value: a captured forward + backward replays to the eager bits"""
    ops = vds["ops"]
    for head, shape in (("ones_all16_fold", (1040, 16, 8, 2, 2)), ("ones_mfma32", (1040, 16, 8, 1, 2)),
                        ("hd64", (280, 16, 8, 3, 3))):
        eager = attn_run(ops, head, shape)
        replay = attn_run(ops, head, shape, graph=True)
        for name, a, b in zip(NAMES, eager, replay):
            assert same(a.contiguous(), b.contiguous()), (head, name)


def test_argument_errors_on_live_buffers(vds):
    ops, _lib = vds["ops"], vds["lib"]
    L, hd = 166, 64
    q = torch.zeros(1, 2, L, hd, dtype=bf16, device="cuda")
    o = torch.zeros(1 * L, 2 * hd, dtype=bf16, device="cuda")
    lse = torch.zeros(1, 2, L, dtype=f32, device="cuda")
    ov = ops.heads_view(o, 1, L, 2, hd)
    with pytest.raises(ValueError, match="needs frame_major=True"):
        ops.attn_fwd(q, q, q, ov, lse, frames=(16, 3), window=2)
    with pytest.raises(ValueError, match="int >= 1"):
        ops.attn_fwd(q, q, q, ov, lse, frames=(16, 3), frame_major=True, window=0)
    with pytest.raises(ValueError, match="do not fit"):
        ops.attn_fwd(q, q, q, ov, lse, frames=(16, 4), frame_major=True, window=2)
    a = _lib.AttnArgs()
    a.B, a.H, a.Lq, a.Lk, a.head_dim = 1, 2, L, L, hd
    for f, t in (("q", q), ("k", q), ("v", q), ("o", ov)):
        setattr(a, f, t.data_ptr())
        s = (t.stride(0), t.stride(1), t.stride(2))
        setattr(a, f + "_sb", s[0]), setattr(a, f + "_sh", s[1]), setattr(a, f + "_sl", s[2])
    a.lse = lse.data_ptr()
    lib = _lib.load()
    fr = C.byref(_lib.ModGroups(16, 3))
    lse.fill_(7.0)
    assert lib.vds_attn_fwd_causal_fm_window(C.byref(a), fr, 1, 0, None) == -1
    assert lib.vds_attn_fwd_causal_fm_window(C.byref(a), fr, 0, 2, None) == -1
    assert lib.vds_attn_fwd_causal_fm_window(C.byref(a), None, 1, 2, None) == -1
    assert lib.vds_attn_fwd_causal_fm_window(C.byref(a), C.byref(_lib.ModGroups(16, 4)), 1, 2, None) == -1
    torch.cuda.synchronize()
    assert float(lse.min()) == 7.0 and float(o.abs().max()) == 0.0, "a refused call wrote"
