"""Chunk-causal frame-major attention on the GPU: vds_attn_fwd_causal_fm_chunk / vds_attn_bwd_causal_fm_chunk through the
whole frame-major path -- token-major qkv -> the frame-major qkv / RoPE kernel (identity rotation) -> frame-major q, k, v,
lse, dq, dk, dv with TOKEN-major o and dO -- against fp32 torch attention in TOKEN order under the dense chunk mask of
tests/helpers/frame_chunk_ref.py, at the bounds tests/test_attn_frame_major_gpu.py uses for the same kernels: o 6e-3, lse
1e-3, gradients 8e-3 (relative Frobenius norm).  Also: chunk = 1 through the new entry points against the _fm entry
points, bit for bit; exact causality over chunks with traps on every later chunk, and visibility inside a chunk; a
captured forward + backward; the refusals on live buffers.

Shapes (L, lead, period, c) are frame_chunk_ref.SHAPES, B = H = 2.  HEADS is that module's: every head dim of the
dispatcher, and the ones layout at head dim 72 under the variant masks 7 / 5 / 2 / 0, attn_delta_fold 0 / 1 and
attn_fwd_wide = 1, which reach every frame-major kernel family at small L (the table in that module)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_chunk_ref as CH  # noqa: E402
import frame_major_ref as FM  # noqa: E402
from test_attn_frame_major_gpu import AB, AH, HEADS, NAMES, TOL_G, TOL_LSE, TOL_O, TOLS, Variant, heads_of, rel, same  # noqa: E402

FC = CH.FC
pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
ids = CH.ids


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import _lib, ops
    return dict(ops=ops, lib=_lib)


_ain, _aref = {}, {}


def attn_inputs(hd, L, later=None, seed=0):
    """(qkv [B*L, 3D], dO [B*L, D]) bf16 in token order.  later = (lead, period, c, g): the rows of the chunk groups > g carry
    OTHER values -- q and dO redrawn, K redrawn and scaled by 32, V = 1000 (the traps); seed: another draw of them"""
    key = (hd, L, later, seed)
    if key not in _ain:
        D = AH * hd
        g = torch.Generator().manual_seed(9000 + hd + L)
        qkv, do = torch.randn(AB * L, 3 * D, generator=g).to(bf16), torch.randn(AB * L, D, generator=g).to(bf16)
        if later is not None:
            lead, period, c, grp = later
            g = torch.Generator().manual_seed(77 + seed)
            sel = (CH.group_index_tok(L, lead, period, c) > grp).repeat(AB)
            n = int(sel.sum())
            qkv, do = qkv.clone(), do.clone()
            qkv[sel, :D] = torch.randn(n, D, generator=g).to(bf16)
            qkv[sel, D:2 * D] = (torch.randn(n, D, generator=g) * 32).to(bf16)
            qkv[sel, 2 * D:] = 1000.0
            do[sel] = torch.randn(n, D, generator=g).to(bf16)
        _ain[key] = (qkv, do)
    return _ain[key]


def attn_reference(hd, shape, later=None):
    """fp32 torch under the dense chunk mask, token rows, once per case"""
    key = (hd, shape, later)
    if key not in _aref:
        L, lead, period, c = shape
        qkv, do = attn_inputs(hd, L, later)
        D = AH * hd
        q, k, v = (heads_of(qkv, AB, L, AH, hd, i * D).float().requires_grad_(True) for i in range(3))
        o, lse = FC.masked_attention(q, k, v, CH.allowed_tok(L, lead, period, c))
        o.backward(heads_of(do, AB, L, AH, hd).float())
        _aref[key] = (o.detach(), lse.detach(), q.grad, k.grad, v.grad)
    return _aref[key]


def attn_run(ops, head, shape, later=None, seed=0, graph=False, chunk=None, edit=None):
    """the library on the shared inputs -> CPU o [B,H,L,hd] (token rows), lse, dq, dk, dv (frame-major rows).
    chunk: the chunk passed to the library (default: the shape's); edit(qkv, do): changes the device inputs in place"""
    hd, hdp, ones, kn = HEADS[head]
    L, lead, period, c = shape
    c = c if chunk is None else chunk
    D = AH * hd
    qkv, do = (t.cuda() for t in attn_inputs(hd, L, later, seed))
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
@pytest.mark.parametrize("shape", CH.SHAPES, ids=ids)
def test_attention_against_fp32_attention_under_the_chunk_mask(vds, shape, head):
    got = attn_run(vds["ops"], head, shape)
    ref = to_fm(attn_reference(HEADS[head][0], shape), shape)
    errs = []
    for name, g_, r_ in zip(NAMES, got, ref):
        assert torch.isfinite(g_.float()).all(), f"{name}: an element was left unwritten or is not finite"
        errs.append(rel(g_, r_))
    print(ids(shape), head, " ".join(f"{n} {e:.2e}" for n, e in zip(NAMES, errs)))
    for name, e, tol in zip(NAMES, errs, TOLS):
        assert e < tol, f"{name}: rel {e:.3e} >= {tol:.1e}"


def test_the_chunk_changes_the_result(vds):
    """the chunk is read: the frame-causal result on the same inputs is far outside the bounds"""
    shape = (280, 16, 8, 2)
    got, plain = attn_run(vds["ops"], "hd64", shape), attn_run(vds["ops"], "hd64", shape, chunk=1)
    assert rel(got[0], plain[0]) > 10 * TOL_O


@pytest.mark.parametrize("head", ["hd64", "hd128", "hd72_ones", "ones_all16_fold", "ones_all16_delta", "ones_mfma32"])
def test_chunk_1_through_the_new_entry_points_is_the_fm_call_bit_for_bit(vds, head, monkeypatch):
    ops, lib = vds["ops"], vds["lib"].load()
    calls = []
    for shape in ((280, 16, 8, 1), (1040, 16, 4, 1)):
        want = attn_run(ops, head, shape)  # ops routes chunk = 1 to vds_attn_*_causal_fm
        with monkeypatch.context() as mp:
            fwd, bwd = lib.vds_attn_fwd_causal_fm_chunk, lib.vds_attn_bwd_causal_fm_chunk
            mp.setattr(lib, "vds_attn_fwd_causal_fm", lambda a, fr, s: (calls.append("f"), fwd(a, fr, 1, s))[1])
            mp.setattr(lib, "vds_attn_bwd_causal_fm", lambda a, fr, s: (calls.append("b"), bwd(a, fr, 1, s))[1])
            got = attn_run(ops, head, shape)
        for name, a, b in zip(NAMES, got, want):
            assert same(a.contiguous(), b.contiguous()), (head, shape, name)
    assert calls == ["f", "b"] * 2


@pytest.mark.parametrize("head", ["hd32", "hd96", "hd72_ones", "ones_all16_fold", "ones_all16_delta", "ones_fwd16_dkv16",
                                  "ones_dq16"])
@pytest.mark.parametrize("shape", [s for s in CH.SHAPES if s[3] < s[2]], ids=ids)
def test_later_chunks_change_nothing_bit_for_bit_and_traps_stay_out(vds, shape, head):
    """K x 32 and V = 1000 on every chunk > n, and two different draws of the later chunks' Q / K / dO: o, lse and dq of the
    rows of the chunks <= n are bit-identical, to each other and to the untrapped run; the trapped problem still matches
    its own reference"""
    L, lead, period, c = shape
    S = (L - lead) // period
    hd = HEADS[head][0]
    n_chunks = -(-period // c)
    base = attn_run(vds["ops"], head, shape)
    ran = 0
    for n in sorted({1, (n_chunks + 1) // 2, n_chunks - 1}):  # chunk group n is the last one kept
        if not 1 <= n < n_chunks:
            continue
        later = (lead, period, c, n)
        got = attn_run(vds["ops"], head, shape, later=later)
        again = attn_run(vds["ops"], head, shape, later=later, seed=1)
        rows = lead + n * c * S  # frame-major rows of the groups <= n
        keep_tok = CH.group_index_tok(L, lead, period, c) <= n
        for other in (base, again):
            assert same(got[0][:, :, keep_tok].contiguous(), other[0][:, :, keep_tok].contiguous()), ("o", n)
            assert same(got[1][:, :, :rows].contiguous(), other[1][:, :, :rows].contiguous()), ("lse", n)
            assert same(got[2][:, :, :rows].contiguous(), other[2][:, :, :rows].contiguous()), ("dq", n)
        # (o of the trapped rows is 1000 in both draws: V = 1000 on every key they prefer; their lse tells the draws apart)
        assert not same(got[0], base[0]) and not same(got[1], again[1]), "the later chunks did not change"
        assert float(got[0][:, :, keep_tok].float().abs().max()) < 100.0  # V = 1000 stayed out
        # the trapped problem against its own reference: o and lse on every row, dq on the kept rows (the gradients of the
        # trapped rows cancel numbers near 1000 |dO|: an ill-conditioned input, not a mask question)
        ref = to_fm(attn_reference(hd, shape, later), shape)
        assert rel(got[0], ref[0]) < TOL_O and rel(got[1], ref[1]) < TOL_LSE, (n, rel(got[0], ref[0]), rel(got[1], ref[1]))
        assert rel(got[2][:, :, :rows], ref[2][:, :, :rows]) < TOL_G, (n, rel(got[2][:, :, :rows], ref[2][:, :, :rows]))
        ran += 1
    assert ran, "no chunk was trapped"


@pytest.mark.parametrize("head", ["hd64", "hd72_ones", "ones_all16_fold"])
@pytest.mark.parametrize("shape", [(280, 16, 8, 2), (280, 16, 8, 3), (1040, 16, 4, 2)], ids=ids)
def test_frames_of_one_chunk_see_each_other(vds, shape, head):
    """other K / V on frame 1 (the second frame of chunk 0) move o and lse of frame 0; the frame-causal call is unmoved"""
    L, lead, period, c = shape
    S = (L - lead) // period
    hd = HEADS[head][0]
    D = AH * hd
    f1 = (CH.R.group_index(L, lead, period) == 2).repeat(AB).cuda()  # token rows of frame 1

    def edit(qkv, do):
        qkv[f1, D:] = (qkv[f1, D:].float() * -3.0 + 0.25).to(bf16)
    rows0 = slice(lead, lead + S)  # frame-major rows of frame 0
    for chunk, moves in ((c, True), (1, False)):
        a = attn_run(vds["ops"], head, shape, chunk=chunk)
        b = attn_run(vds["ops"], head, shape, chunk=chunk, edit=edit)
        d = rel(b[1][:, :, rows0], a[1][:, :, rows0])
        print(ids(shape), head, f"chunk {chunk}: lse of frame 0 moves by {d:.3e}")
        assert same(a[1][:, :, :lead].contiguous(), b[1][:, :, :lead].contiguous())  # the registers never see a token
        if moves:
            assert d > 10 * TOL_LSE, d
        else:
            assert same(a[1][:, :, rows0].contiguous(), b[1][:, :, rows0].contiguous())


def test_graph_replay(vds):
    """lead, period and the chunk travel by value: a captured forward + backward replays to the eager bits"""
    ops = vds["ops"]
    for head, shape in (("ones_all16_fold", (1040, 16, 4, 2)), ("ones_mfma32", (1040, 16, 4, 2)), ("hd64", (280, 16, 8, 3))):
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
        ops.attn_fwd(q, q, q, ov, lse, frames=(16, 3), chunk=2)
    with pytest.raises(ValueError, match="int >= 1"):
        ops.attn_fwd(q, q, q, ov, lse, frames=(16, 3), frame_major=True, chunk=0)
    with pytest.raises(ValueError, match="do not fit"):
        ops.attn_fwd(q, q, q, ov, lse, frames=(16, 4), frame_major=True, chunk=2)
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
    assert lib.vds_attn_fwd_causal_fm_chunk(C.byref(a), fr, 0, None) == -1
    assert lib.vds_attn_fwd_causal_fm_chunk(C.byref(a), None, 2, None) == -1
    assert lib.vds_attn_fwd_causal_fm_chunk(C.byref(a), C.byref(_lib.ModGroups(16, 4)), 2, None) == -1
    torch.cuda.synchronize()
    assert float(lse.min()) == 7.0 and float(o.abs().max()) == 0.0, "a refused call wrote"
