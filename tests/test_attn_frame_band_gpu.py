"""Frame-band frame-major attention on the GPU: vds_band_attn_fwd / vds_band_attn_bwd through the whole frame-major path --
token-major qkv -> the frame-major qkv / RoPE kernel (identity rotation) -> frame-major q, k, v, lse, dq, dk, dv with
TOKEN-major o and dO -- against fp32 torch attention in TOKEN order under the dense band mask of
tests/helpers/frame_band_ref.py, at the bounds of tests/test_attn_frame_major_gpu.py: o 6e-3, lse 1e-3, gradients 8e-3
(relative Frobenius norm).  Also: a band of every chunk against the unmasked ops.attn_fwd / attn_bwd on the permuted rows
at the same bounds (only the summation order differs); the chunk-causal call on the same inputs is far outside them;
containment -- traps on every token row outside the band of a chunk leave o, lse and dq of that chunk bit-identical, while
K / V inside the band and in the lead rows move them; a captured forward + backward; every call twice, in both determinism
modes; the refusals on live buffers.

Shapes (L, lead, period, c, band) are frame_band_ref.SHAPES, B = H = 2.  HEADS is tests/test_attn_frame_major_gpu.py's: every
head dim of the dispatcher, and the ones layout at head dim 72 under the variant masks and knobs that select the 16x16x32
and 64-queries-per-wave families elsewhere -- there is no BAND instance of those: every entry must land on the plain BAND
kernels, on the same rows."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_band_ref as FB  # noqa: E402
import frame_chunk_ref as CH  # noqa: E402
import frame_major_ref as FM  # noqa: E402
from test_attn_frame_major_gpu import AB, AH, HEADS, NAMES, TOL_G, TOL_LSE, TOL_O, TOLS, Variant, heads_of, rel, same  # noqa: E402

FC = CH.FC
pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
ids = FB.ids


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import _lib, ops
    return dict(ops=ops, lib=_lib)


_ain, _aref = {}, {}


def outside_tok(L, lead, period, c, b, n):
    """bool [L], token rows: the token rows of the chunks that chunk n does not attend -- before its band or after it"""
    g = CH.group_index_tok(L, lead, period, c) - 1  # chunk of a token row, -1: a lead row
    return (g >= 0) & ((g < n - b) | (g > n + b))


def attn_inputs(hd, L, trap=None, seed=0):
    """(qkv [B*L, 3D], dO [B*L, D]) bf16 in token order.  trap = (lead, period, c, b, n): the token rows outside the band of
    chunk n carry OTHER values -- q and dO redrawn, K redrawn and scaled by 32, V = 1000; seed: another draw of them"""
    key = (hd, L, trap, seed)
    if key not in _ain:
        D = AH * hd
        g = torch.Generator().manual_seed(9300 + hd + L)
        qkv, do = torch.randn(AB * L, 3 * D, generator=g).to(bf16), torch.randn(AB * L, D, generator=g).to(bf16)
        if trap is not None:
            g = torch.Generator().manual_seed(79 + seed)
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
    """fp32 torch under the dense band mask, token rows, once per case"""
    key = (hd, shape, trap)
    if key not in _aref:
        L, lead, period, c, band = shape
        qkv, do = attn_inputs(hd, L, trap)
        D = AH * hd
        q, k, v = (heads_of(qkv, AB, L, AH, hd, i * D).float().requires_grad_(True) for i in range(3))
        o, lse = FC.masked_attention(q, k, v, FB.allowed_tok(L, lead, period, c, band))
        o.backward(heads_of(do, AB, L, AH, hd).float())
        _aref[key] = (o.detach(), lse.detach(), q.grad, k.grad, v.grad)
    return _aref[key]


def attn_run(ops, head, shape, trap=None, seed=0, graph=False, mode="band", band="shape", edit=None):
    """the library on the shared inputs -> CPU o [B,H,L,hd], lse, dq, dk, dv (lse and the gradients in frame-major rows).
    mode "band": ops.band_attn_* with the shape's band in chunks (or `band`); o in token rows.  "chunk": the chunk-causal
    ops.attn_* call; o in token rows.  "unmasked": the plain ops.attn_* on the frame-major q, k, v and a frame-major dO; o
    in frame-major rows.  edit(qkv, do): changes the device inputs in place"""
    hd, hdp, ones, kn = HEADS[head]
    L, lead, period, c, bnd = shape
    D = AH * hd
    qkv, do = (t.cuda() for t in attn_inputs(hd, L, trap, seed))
    if edit is not None:
        edit(qkv, do)
    if mode == "unmasked":  # dO in frame-major rows, as o will be
        tok = FM.tok_index(L, lead, period).cuda()
        do = do.view(AB, L, D)[:, tok].reshape(AB * L, D).contiguous()
    cos = torch.ones(L, hd // 2, dtype=f32, device="cuda")
    sin = torch.zeros(L, hd // 2, dtype=f32, device="cuda")
    qp, kp, vp = ops.qkv_rope_fwd(qkv, cos, sin, None, None, AB, L, AH, hd, hdp, frames=(lead, period))
    nan = float("nan")
    o = torch.full((AB * L, D), nan, dtype=bf16, device="cuda")
    lse = torch.full((AB, AH, L), nan, dtype=f32, device="cuda")
    dqb, dkb, dvb = (torch.full((AB, AH, L, hdp), nan, dtype=bf16, device="cuda") for _ in range(3))
    ov, dov = ops.heads_view(o, AB, L, AH, hd), ops.heads_view(do, AB, L, AH, hd)
    delta = torch.empty(ops.attn_bwd_workspace_floats(AB, AH, L, L, hd, ones), dtype=f32, device="cuda")
    if mode == "band":
        fwd, bwd = ops.band_attn_fwd, ops.band_attn_bwd
        akw = dict(kv_pad_ones=ones, frames=(lead, period), frame_major=True, chunk=c, band=bnd // c if band == "shape" else band)
    elif mode == "chunk":
        fwd, bwd = ops.attn_fwd, ops.attn_bwd
        akw = dict(kv_pad_ones=ones, frames=(lead, period), frame_major=True, chunk=c)
    else:
        fwd, bwd = ops.attn_fwd, ops.attn_bwd
        akw = dict(kv_pad_ones=ones)

    def step():
        fwd(qp[..., :hd], kp[..., :hd], vp[..., :hd], ov, lse, **akw)
        bwd(qp[..., :hd], kp[..., :hd], vp[..., :hd], ov, lse, dov, dqb[..., :hd], dkb[..., :hd], dvb[..., :hd], delta, **akw)
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
@pytest.mark.parametrize("shape", FB.SHAPES, ids=ids)
def test_attention_against_fp32_attention_under_the_band_mask(vds, shape, head):
    got = attn_run(vds["ops"], head, shape)  # (every output NaN-prefilled)
    ref = to_fm(attn_reference(HEADS[head][0], shape), shape)
    errs = []
    for name, g_, r_ in zip(NAMES, got, ref):
        assert torch.isfinite(g_.float()).all(), f"{name}: an element was left unwritten or is not finite"
        errs.append(rel(g_, r_))
    print(ids(shape), head, " ".join(f"{n} {e:.2e}" for n, e in zip(NAMES, errs)))
    for name, e, tol in zip(NAMES, errs, TOLS):
        assert e < tol, f"{name}: rel {e:.3e} >= {tol:.1e}"


@pytest.mark.parametrize("head", [h for h in HEADS if HEADS[h][3]])
def test_every_variant_setting_lands_on_the_plain_band_kernels(vds, head):
    """no BAND instance of the 16x16x32 or 64-queries-per-wave families: whatever the variant bits and knobs of the entry,
    the bits are those of the same layout under variant 0 and the default knobs"""
    hd, hdp, ones, kn = HEADS[head]
    plain = next(h for h, (hd2, hdp2, ones2, kn2) in HEADS.items() if (hd2, hdp2, ones2) == (hd, hdp, ones) and not kn2)
    for shape in ((280, 16, 8, 1, 1), (1040, 16, 8, 2, 2)):
        for name, a, b in zip(NAMES, attn_run(vds["ops"], head, shape), attn_run(vds["ops"], plain, shape)):
            assert same(a.contiguous(), b.contiguous()), (head, shape, name)


@pytest.mark.parametrize("head", ["hd32", "hd64", "hd72", "hd96", "hd128", "hd72_ones", "ones_all16_fold", "ones_mfma32"])
def test_a_band_of_every_chunk_is_the_unmasked_attention_on_the_permuted_rows(vds, head):
    """only the summation order differs: the same bounds, and the two results agree with each other to them as well"""
    ops = vds["ops"]
    hd = HEADS[head][0]
    for shape in ((280, 16, 8, 1, 7), (280, 16, 8, 3, 6), (203, 0, 7, 1, 6), (1040, 16, 8, 2, 6)):
        L, lead, period, c, band = shape
        n = -(-period // c)
        tok = FM.tok_index(L, lead, period)
        want = attn_run(ops, head, shape, mode="unmasked")
        want[0] = want[0][:, :, torch.argsort(tok)]  # o of frame-major row r is o of token row tok(r)
        ref = to_fm(attn_reference(hd, shape), shape)
        for b in (n - 1, n, n + 3, 1 << 30):
            got = attn_run(ops, head, shape, band=b)
            for name, a, w_, r_, tol in zip(NAMES, got, want, ref, TOLS):
                assert torch.isfinite(a.float()).all(), name
                assert rel(a, w_) < tol, (head, shape, b, name, rel(a, w_))
                assert rel(a, r_) < tol and rel(w_, r_) < tol, (head, shape, b, name)
        if n > 2:
            assert rel(attn_run(ops, head, shape, band=n - 3)[0], want[0]) > TOL_O  # fewer chunks: another result


def test_the_band_changes_the_result(vds):
    """the mask is read: the chunk-causal result on the same inputs is far outside the bounds"""
    for shape in ((280, 16, 8, 2, 2), (1040, 16, 8, 1, 1)):
        got, causal = attn_run(vds["ops"], "hd64", shape), attn_run(vds["ops"], "hd64", shape, mode="chunk")
        assert rel(got[0], causal[0]) > 10 * TOL_O and rel(got[1], causal[1]) > 10 * TOL_LSE


@pytest.mark.parametrize("head", ["hd32", "hd64", "hd96", "hd128", "hd72_ones", "ones_all16_fold"])
@pytest.mark.parametrize("shape", [(166, 16, 3, 1, 1), (280, 16, 8, 1, 1), (280, 16, 8, 1, 0), (280, 16, 8, 2, 2),
                                   (203, 0, 7, 1, 2), (293, 33, 4, 1, 1), (656, 80, 9, 1, 2), (1040, 16, 8, 1, 1)], ids=ids)
def test_rows_outside_the_band_change_nothing_bit_for_bit_and_traps_stay_out(vds, shape, head):
    """K x 32 and V = 1000 on every token row outside the band of chunk n -- the chunks before it and after it -- and two
    different draws of those rows' Q / K / dO: o, lse and dq of the rows of chunk n are bit-identical, to each other and to
    the untrapped run; the trapped problem still matches its own reference on those rows"""
    L, lead, period, c, band = shape
    S = (L - lead) // period
    b = band // c
    hd = HEADS[head][0]
    n_chunks = -(-period // c)
    base = attn_run(vds["ops"], head, shape)
    ran = 0
    for n in sorted({0, n_chunks // 2, n_chunks - 1}):  # rows after the band only, on both sides, before it only
        trap = (lead, period, c, b, n)
        if not bool(outside_tok(L, *trap).any()):
            continue
        got = attn_run(vds["ops"], head, shape, trap=trap)
        again = attn_run(vds["ops"], head, shape, trap=trap, seed=1)
        r0, r1 = lead + n * c * S, min(L, lead + (n + 1) * c * S)  # frame-major rows of chunk n
        rows = slice(r0, r1)
        keep_tok = CH.group_index_tok(L, lead, period, c) == n + 1
        assert int(keep_tok.sum()) == r1 - r0 and int(outside_tok(L, *trap).sum()) >= S
        for other in (base, again):
            assert same(got[0][:, :, keep_tok].contiguous(), other[0][:, :, keep_tok].contiguous()), ("o", n)
            assert same(got[1][:, :, rows].contiguous(), other[1][:, :, rows].contiguous()), ("lse", n)
            assert same(got[2][:, :, rows].contiguous(), other[2][:, :, rows].contiguous()), ("dq", n)
        assert not same(got[0], base[0]) and not same(got[1], again[1]), "the rows outside the band did not change"
        assert float(got[0][:, :, keep_tok].float().abs().max()) < 100.0  # V = 1000 stayed out
        ref = to_fm(attn_reference(hd, shape, trap), shape)
        assert rel(got[0][:, :, keep_tok], ref[0][:, :, keep_tok]) < TOL_O
        assert rel(got[1][:, :, rows], ref[1][:, :, rows]) < TOL_LSE
        assert rel(got[2][:, :, rows], ref[2][:, :, rows]) < TOL_G
        ran += 1
    assert ran, "no chunk was trapped"


@pytest.mark.parametrize("head", ["hd64", "hd72_ones", "hd128"])
@pytest.mark.parametrize("shape", [(280, 16, 8, 1, 1), (280, 16, 8, 1, 2), (1040, 16, 8, 1, 1)], ids=ids)
def test_keys_inside_the_band_and_lead_keys_are_seen(vds, shape, head):
    """other K / V on the first and on the last chunk of a middle chunk's band, and on the lead rows, move lse of that
    chunk; other K / V on the chunks just outside the band move it by exactly nothing -- and move lse of the lead rows"""
    L, lead, period, c, band = shape
    S = (L - lead) // period
    b = band // c
    hd = HEADS[head][0]
    D = AH * hd
    n_chunks = -(-period // c)
    n = n_chunks // 2
    assert n - b - 1 >= 0 and n + b + 1 < n_chunks
    grp = CH.group_index_tok(L, lead, period, c)
    rows = slice(lead + n * c * S, min(L, lead + (n + 1) * c * S))
    base = attn_run(vds["ops"], head, shape)

    def moved(sel):
        sel = sel.repeat(AB).cuda()

        def edit(qkv, do):
            qkv[sel, D:] = (qkv[sel, D:].float() * -3.0 + 0.25).to(bf16)
        r = attn_run(vds["ops"], head, shape, edit=edit)
        return r[1], rel(r[1][:, :, rows], base[1][:, :, rows])
    d_first, d_last = moved(grp == 1 + n - b)[1], moved(grp == 1 + n + b)[1]
    d_lead = moved(grp == 0)[1]
    print(ids(shape), head, f"lse of chunk {n} moves by {d_first:.3e}, {d_last:.3e} (band edges), {d_lead:.3e} (lead)")
    assert d_first > 10 * TOL_LSE and d_last > 10 * TOL_LSE and d_lead > 10 * TOL_LSE
    for g_out in (1 + n - b - 1, 1 + n + b + 1):
        out, _ = moved(grp == g_out)
        assert same(out[:, :, rows].contiguous(), base[1][:, :, rows].contiguous()), g_out
        assert rel(out[:, :, :lead], base[1][:, :, :lead]) > TOL_LSE, "a lead query attends every key"


def test_graph_replay(vds):
    """lead, period, the chunk and the band travel by value: a captured forward + backward replays to the eager bits"""
    ops = vds["ops"]
    for head, shape in (("ones_all16_fold", (1040, 16, 8, 2, 2)), ("hd72_ones", (1040, 16, 8, 1, 1)),
                        ("hd64", (280, 16, 8, 3, 3)), ("hd128", (203, 0, 7, 1, 2))):
        eager = attn_run(ops, head, shape)
        replay = attn_run(ops, head, shape, graph=True)
        for name, a, b in zip(NAMES, eager, replay):
            assert same(a.contiguous(), b.contiguous()), (head, name)


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
def test_every_call_twice_gives_equal_bits(vds, det, request):
    """no atomics: the results are bit-identical run to run in both determinism modes"""
    ops = vds["ops"]
    if det:
        ops.set_deterministic(True, 64 << 20)
        request.addfinalizer(lambda: ops.set_deterministic(False))
    for head in ("hd32", "hd64", "hd72", "hd96", "hd128", "hd72_ones"):
        for shape in ((280, 16, 8, 1, 1), (656, 80, 9, 1, 2), (1040, 16, 8, 2, 2), (203, 0, 7, 1, 2)):
            one, two = attn_run(ops, head, shape), attn_run(ops, head, shape)
            for name, a, b in zip(NAMES, one, two):
                assert same(a.contiguous(), b.contiguous()), (head, shape, name)


def test_argument_errors_on_live_buffers(vds):
    ops, _lib = vds["ops"], vds["lib"]
    L, hd = 166, 64
    q = torch.zeros(1, 2, L, hd, dtype=bf16, device="cuda")
    o = torch.zeros(1 * L, 2 * hd, dtype=bf16, device="cuda")
    lse = torch.zeros(1, 2, L, dtype=f32, device="cuda")
    ov = ops.heads_view(o, 1, L, 2, hd)
    with pytest.raises(ValueError, match="needs frame_major=True"):
        ops.band_attn_fwd(q, q, q, ov, lse, frames=(16, 3), band=1)
    with pytest.raises(ValueError, match="must be >= 0"):
        ops.band_attn_fwd(q, q, q, ov, lse, frames=(16, 3), frame_major=True, band=-1)
    with pytest.raises(ValueError, match="excludes window"):
        ops.band_attn_fwd(q, q, q, ov, lse, frames=(16, 3), frame_major=True, window=1, band=1)
    with pytest.raises(ValueError, match="do not fit"):
        ops.band_attn_fwd(q, q, q, ov, lse, frames=(16, 4), frame_major=True, band=1)
    with pytest.raises(ValueError, match="must be >= 0"):
        ops.band_attn_bwd(q, q, q, ov, lse, ov, q, q, q, frames=(16, 3), frame_major=True, band=-2)
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
    assert lib.vds_band_attn_fwd(C.byref(a), fr, 1, -1, None) == -1
    assert lib.vds_band_attn_fwd(C.byref(a), fr, 0, 1, None) == -1
    assert lib.vds_band_attn_fwd(C.byref(a), None, 1, 1, None) == -1
    assert lib.vds_band_attn_fwd(C.byref(a), C.byref(_lib.ModGroups(16, 4)), 1, 1, None) == -1
    a.kv_pad_ones = 2
    assert lib.vds_band_attn_fwd(C.byref(a), fr, 1, 1, None) == -1
    a.kv_pad_ones = 0
    a.Lk = L + 1
    assert lib.vds_band_attn_fwd(C.byref(a), fr, 1, 1, None) == -1
    a.Lk = L
    a.head_dim = 256
    assert lib.vds_band_attn_fwd(C.byref(a), fr, 1, 1, None) == -2
    assert lib.vds_band_attn_fwd(C.byref(a), fr, 1, -1, None) == -1  # ARG before UNSUPPORTED
    a.head_dim = hd
    torch.cuda.synchronize()
    assert float(lse.min()) == 7.0 and float(o.abs().max()) == 0.0, "a refused call wrote"
    assert lib.vds_band_attn_fwd(C.byref(a), fr, 1, 1, None) == 0  # and the same arguments, whole, run
    torch.cuda.synchronize()
    assert float((lse - 7.0).abs().min()) > 0.0
