"""Frame-major head rows on the GPU: the frame-major qkv / RoPE kernels (vds_qkv_rope_fwd_fm / _norm_fwd_fm / _bwd_fm /
_norm_bwd_fm) against the plain calls with the head rows permuted by fm, BIT FOR BIT -- q, k, v with their pad and ones
columns forward; dqkv, the dv0 accumulator and (deterministic mode) dlam backward -- with and without v0, with and without
QK-norm, and in every kernel form: the token-tile forward at 2 / 4 / 8 tokens, the wave-per-token backward, and the
element-wise kernels that the knobs rope_tile = 0 / rope_tok = 0 and the shapes without a tile instance select.

Shapes (L, lead, period) are those of tests/helpers/frame_major_ref.py: S = 50, 33, 65, one frame, S = 1 (every frame one
row), no lead rows, frames aligned with and offset from the tiles.  B = 2, so token tiles span the sample boundary."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_major_ref as FM  # noqa: E402

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
ids = lambda s: "L{}_{}_{}".format(*s)

# (H, hd, hdp) of each shape, in the order of FM.SHAPES: every head dim of the dispatcher, head dim 72 with its ones
# columns at the training-like shapes, and two layouts without a tile instance (element-wise kernels only)
LAYOUT = {(166, 16, 3): (2, 72, 96), (280, 16, 8): (3, 64, 64), (203, 0, 7): (1, 128, 128), (140, 5, 3): (2, 96, 96),
          (293, 33, 4): (4, 32, 32), (193, 64, 1): (2, 72, 96), (80, 16, 64): (2, 72, 76), (1024, 0, 4): (2, 24, 24),
          (1040, 16, 4): (2, 72, 96)}
B = 2


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import _lib, ops
    return dict(ops=ops, lib=_lib)


class Knobs:
    def __init__(self, ops, knobs):
        self.ops, self.knobs, self.prev = ops, knobs, {}

    def __enter__(self):
        for k, v in self.knobs.items():
            self.prev[k] = self.ops.knob_set(k, v)

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            self.ops.knob_set(k, v)


_inputs = {}


def inputs(shape):
    """the shape's device tensors in token order and their frame-major copies, made once (never modified)"""
    if shape in _inputs:
        return _inputs[shape]
    L, lead, period = shape
    H, hd, hdp = LAYOUT[shape]
    D = H * hd
    g = torch.Generator().manual_seed(7000 + L + 10 * hd)
    qkv = (torch.randn(B * L, 3 * D, generator=g) * 1.5).to(bf16)
    ang = torch.rand(L, hd // 2, generator=g) * 6.2832
    v0 = torch.randn(B, H, L, hdp, generator=g).to(bf16)
    lam = torch.tensor([0.625]).to(bf16)
    dq, dk, dv = (torch.randn(B, H, L, hdp, generator=g).to(bf16) for _ in range(3))  # random pad columns too
    acc = torch.randn(B, H, L, hdp, generator=g)
    tok = FM.tok_index(L, lead, period).cuda()
    d = dict(L=L, H=H, hd=hd, hdp=hdp, frames=(lead, period), tok=tok, qkv=qkv.cuda(), cos=torch.cos(ang).float().cuda(),
             sin=torch.sin(ang).float().cuda(), lam=lam.cuda())
    for name, t in (("v0", v0), ("dq", dq), ("dk", dk), ("dv", dv), ("acc", acc)):
        d[name] = t.cuda()
        d[name + "_fm"] = d[name][:, :, tok].contiguous()  # row r of the frame-major tensor is token row tok(r)
    _inputs[shape] = d
    return d


def bits(t):
    return t.view(torch.int16) if t.dtype == bf16 else t.view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


FWD_KNOBS = [{}, {"rope_tile": 2}, {"rope_tile": 8}, {"rope_tile": 0}]
BWD_KNOBS = [{}, {"rope_tok": 0}]


@pytest.mark.parametrize("mix", [False, True], ids=["plain_v", "mixed_v"])
@pytest.mark.parametrize("norm", [False, True], ids=["rope", "qk_norm"])
@pytest.mark.parametrize("shape", FM.SHAPES, ids=ids)
def test_forward_is_the_plain_forward_with_rows_permuted(vds, shape, norm, mix):
    ops, d = vds["ops"], inputs(shape)
    L, H, hd, hdp = d["L"], d["H"], d["hd"], d["hdp"]
    fn = ops.qkv_rope_norm_fwd if norm else ops.qkv_rope_fwd
    head = (d["qkv"], d["cos"], d["sin"])
    tail = (d["lam"] if mix else None, B, L, H, hd, hdp)
    for knobs in FWD_KNOBS:
        with Knobs(ops, knobs):
            q, k, v = fn(*head, d["v0"] if mix else None, *tail)
            qf, kf, vf = fn(*head, d["v0_fm"] if mix else None, *tail, frames=d["frames"])
        torch.cuda.synchronize()
        for name, plain, got in (("q", q, qf), ("k", k, kf), ("v", v, vf)):
            assert same(got, plain[:, :, d["tok"]]), (name, knobs)  # data, pad and ones columns of every row
        if hdp - hd >= 8:
            assert float(kf[..., hd].min()) == 1.0 and float(vf[..., hd + 4].min()) == 1.0
    if d["frames"][1] > 1 and L - d["frames"][0] > d["frames"][1]:
        assert not same(qf, q), "the permutation moved nothing"


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("mix", [0, 1, 2])
@pytest.mark.parametrize("norm", [False, True], ids=["rope", "qk_norm"])
@pytest.mark.parametrize("shape", FM.SHAPES, ids=ids)
def test_backward_is_the_plain_backward_on_rows_permuted_back(vds, shape, norm, mix, det, request):
    ops, d = vds["ops"], inputs(shape)
    L, H, hd, hdp = d["L"], d["H"], d["hd"], d["hdp"]
    if det:
        ops.set_deterministic(True, 64 << 20)
        request.addfinalizer(lambda: ops.set_deterministic(False))
    fn = ops.qkv_rope_norm_bwd if norm else ops.qkv_rope_bwd
    add_dv0 = mix == 0 and hd == 72  # block 0's call: dv + the accumulated v_0 gradient

    def call(sfx, **kw):
        acc = d["acc" + sfx].clone() if (mix == 1 or add_dv0) else None
        dlam = torch.full((1,), 0.25, dtype=f32, device="cuda") if mix else None
        out = fn(d["dq" + sfx], d["dk" + sfx], d["dv" + sfx], d["cos"], d["sin"], d["qkv"] if (norm or mix) else None,
                 d["v0" + sfx] if mix else None, d["lam"] if mix else None, acc, dlam, mix, add_dv0, B, L, H, hd, hdp, **kw)
        torch.cuda.synchronize()
        return out, acc, dlam

    for knobs in BWD_KNOBS:
        with Knobs(ops, knobs):
            want, acc, dlam = call("")
            got, acc_fm, dlam_fm = call("_fm", frames=d["frames"])
        assert got.shape == (B * L, 3 * H * hd) and same(got, want), knobs  # dqkv stays token-major
        if acc is not None:
            assert same(acc_fm, acc[:, :, d["tok"]]), knobs
        if mix and det:
            assert same(dlam_fm, dlam), knobs
        elif mix:
            assert abs(dlam_fm.item() - dlam.item()) <= 1e-4 * max(1.0, abs(dlam.item())), knobs


def test_argument_errors(vds):
    """frames == NULL and frames that do not fit L are VDS_ERR_ARG on live device buffers too; ops raises ValueError first"""
    import ctypes as C
    ops, _lib = vds["ops"], vds["lib"]
    d = inputs((166, 16, 3))
    L, H, hd, hdp = d["L"], d["H"], d["hd"], d["hdp"]
    lib = _lib.load()
    q, k, v = (torch.zeros(B, H, L, hdp, dtype=bf16, device="cuda") for _ in range(3))
    p = lambda t: t.data_ptr()
    for frames in (None, C.byref(_lib.ModGroups(16, 4)), C.byref(_lib.ModGroups(167, 1))):
        rc = lib.vds_qkv_rope_fwd_fm(p(d["qkv"]), p(d["cos"]), p(d["sin"]), None, None, p(q), p(k), p(v), B, L, H, hd, hdp,
                                     frames, None)
        assert rc == -1
    torch.cuda.synchronize()
    assert float(q.abs().max()) == 0.0, "a refused call wrote"
    with pytest.raises(ValueError, match="do not fit"):
        ops.qkv_rope_fwd(d["qkv"], d["cos"], d["sin"], None, None, B, L, H, hd, hdp, frames=(16, 4))


# ============================================================================ attention kernels ====
# vds_attn_fwd_causal_fm / vds_attn_bwd_causal_fm through the whole frame-major path: token-major qkv -> the frame-major
# qkv / RoPE kernel (identity rotation) -> frame-major q, k, v, lse, dq, dk, dv with TOKEN-major o and dO.  The reference is
# fp32 torch masked attention in TOKEN order under frame_causal_ref.allowed (tests/test_attn_causal_gpu.py's), so the
# comparison also pins the row maps: o and dO are compared row for row, lse / dq / dk / dv after the permutation.
# Tolerances are the project's: o 6e-3, lse 1e-3, gradients 8e-3 (relative Frobenius norm).
import frame_causal_ref as FC  # noqa: E402

TOL_O, TOL_LSE, TOL_G = 6e-3, 1e-3, 8e-3
NAMES = ["o", "lse", "dq", "dk", "dv"]
TOLS = [TOL_O, TOL_LSE, TOL_G, TOL_G, TOL_G]
# (hd, hdp, kv_pad_ones, knobs): every head dim of the dispatcher; head dim 72 without a pad and in the ones layout, there
# under the settings tests/test_attn_causal_gpu.py uses to reach every kernel family at small L -- the variant mask
# (vds_attn_set_variant: bit 0 dK/dV, bit 1 dQ, bit 2 forward on the 16x16x32 MFMA), attn_delta_fold, and attn_fwd_wide = 1
# (the 64-queries-per-wave forward, which the rule takes from 2048 queries):
#   hd72_ones          defaults: attn_fwd_kernel FM (narrow), attn_bwd_dq16_kernel<FOLD> FM, attn_bwd_dkv16_kernel FM
#   ones_all16_fold    attn_fwd16_kernel FM, attn_bwd_dq16_kernel<FOLD> FM (first), attn_bwd_dkv16_kernel FM
#   ones_all16_delta   attn_fwd16_kernel FM, attn_delta_tokmajor_kernel FM, dkv16 FM, attn_bwd_dq16_kernel<no FOLD> FM
#   ones_fwd16_dkv16   fwd16 FM, delta kernel FM (annotates the q pad dkv16 reads), dkv16 FM, plain attn_bwd_dq_kernel FM
#   ones_dq16          plain forward FM, delta kernel FM, plain attn_bwd_dkv_kernel FM, dq16<no FOLD> FM
#   ones_mfma32        the plain 32x32x16 FM kernels on padded rows
HEADS = {"hd32": (32, 32, False, {}), "hd64": (64, 64, False, {}), "hd72": (72, 72, False, {}),
         "hd96": (96, 96, False, {}), "hd128": (128, 128, False, {}), "hd72_ones": (72, 96, True, {}),
         "ones_all16_fold": (72, 96, True, dict(variant=7, attn_delta_fold=1, attn_fwd_wide=1)),
         "ones_all16_delta": (72, 96, True, dict(variant=7, attn_delta_fold=0, attn_fwd_wide=1)),
         "ones_fwd16_dkv16": (72, 96, True, dict(variant=5, attn_fwd_wide=1)),
         "ones_dq16": (72, 96, True, dict(variant=2, attn_delta_fold=0, attn_fwd_wide=1)),
         "ones_mfma32": (72, 96, True, dict(variant=0, attn_fwd_wide=1))}
AB, AH = 2, 2


class Variant:
    """the variant mask and knobs of a HEADS entry for the length of a call"""

    def __init__(self, ops, kn):
        self.ops, self.kn = ops, dict(kn)

    def __enter__(self):
        v = self.kn.pop("variant", None)
        self.prev_v = self.ops.attn_set_variant(v) if v is not None else None
        self.prev = {k: self.ops.knob_set(k, x) for k, x in self.kn.items()}

    def __exit__(self, *exc):
        for k, x in self.prev.items():
            self.ops.knob_set(k, x)
        if self.prev_v is not None:
            self.ops.attn_set_variant(self.prev_v)


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def heads_of(t2d, Bn, L, H, hd, off=0):
    return t2d[:, off:off + H * hd].reshape(Bn, L, H, hd).permute(0, 2, 1, 3)


_ain, _aref = {}, {}


def attn_inputs(hd, L, later=None):
    """(qkv [B*L, 3D], dO [B*L, D]) bf16 in token order.  later = (lead, period, g): the rows of the groups > g carry OTHER
    values -- q and dO redrawn, K redrawn and scaled by 32, V = 1000 (the traps)"""
    key = (hd, L, later)
    if key not in _ain:
        D = AH * hd
        g = torch.Generator().manual_seed(9000 + hd + L)
        qkv, do = torch.randn(AB * L, 3 * D, generator=g).to(bf16), torch.randn(AB * L, D, generator=g).to(bf16)
        if later is not None:
            lead, period, grp = later
            sel = (FC.R.group_index(L, lead, period) > grp).repeat(AB)
            qkv, do = qkv.clone(), do.clone()
            qkv[sel, :D] = torch.randn(int(sel.sum()), D, generator=g).to(bf16)
            qkv[sel, D:2 * D] = (torch.randn(int(sel.sum()), D, generator=g) * 32).to(bf16)
            qkv[sel, 2 * D:] = 1000.0
            do[sel] = torch.randn(int(sel.sum()), D, generator=g).to(bf16)
        _ain[key] = (qkv, do)
    return _ain[key]


def attn_reference(hd, shape, later=None):
    key = (hd, shape, later)
    if key not in _aref:
        L, lead, period = shape
        qkv, do = attn_inputs(hd, L, later)
        D = AH * hd
        q, k, v = (heads_of(qkv, AB, L, AH, hd, i * D).float().requires_grad_(True) for i in range(3))
        o, lse = FC.masked_attention(q, k, v, FC.allowed(L, lead, period))
        o.backward(heads_of(do, AB, L, AH, hd).float())
        _aref[key] = (o.detach(), lse.detach(), q.grad, k.grad, v.grad)
    return _aref[key]


def attn_run(ops, head, shape, later=None, frame_major=True, graph=False):
    """the library on the shared inputs -> CPU o [B,H,L,hd] (token rows), lse, dq, dk, dv in the rows the call uses
    (frame-major, or token rows with frame_major=False: the interleaved kernels)"""
    hd, hdp, ones, kn = HEADS[head]
    L, lead, period = shape
    D = AH * hd
    qkv, do = (t.cuda() for t in attn_inputs(hd, L, later))
    cos = torch.ones(L, hd // 2, dtype=f32, device="cuda")
    sin = torch.zeros(L, hd // 2, dtype=f32, device="cuda")
    kw = dict(frames=(lead, period)) if frame_major else {}
    qp, kp, vp = ops.qkv_rope_fwd(qkv, cos, sin, None, None, AB, L, AH, hd, hdp, **kw)
    nan = float("nan")
    o = torch.full((AB * L, D), nan, dtype=bf16, device="cuda")
    lse = torch.full((AB, AH, L), nan, dtype=f32, device="cuda")
    dqb, dkb, dvb = (torch.full((AB, AH, L, hdp), nan, dtype=bf16, device="cuda") for _ in range(3))
    ov, dov = ops.heads_view(o, AB, L, AH, hd), ops.heads_view(do, AB, L, AH, hd)
    delta = torch.empty(ops.attn_bwd_workspace_floats(AB, AH, L, L, hd, ones), dtype=f32, device="cuda")
    akw = dict(kv_pad_ones=ones, frames=(lead, period), frame_major=frame_major)

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
    tok = FM.tok_index(*shape)
    return [ref[0], ref[1][:, :, tok]] + [t[:, :, tok] for t in ref[2:]]


@pytest.mark.parametrize("head", list(HEADS))
@pytest.mark.parametrize("shape", FM.SHAPES, ids=ids)
def test_attention_against_fp32_masked_attention(vds, shape, head):
    got = attn_run(vds["ops"], head, shape)
    ref = to_fm(attn_reference(HEADS[head][0], shape), shape)
    errs = []
    for name, g_, r_, tol in zip(NAMES, got, ref, TOLS):
        assert torch.isfinite(g_.float()).all(), f"{name}: an element was left unwritten or is not finite"
        errs.append(rel(g_, r_))
    print(ids(shape), head, " ".join(f"{n} {e:.2e}" for n, e in zip(NAMES, errs)))
    for name, e, tol in zip(NAMES, errs, TOLS):
        assert e < tol, f"{name}: rel {e:.3e} >= {tol:.1e}"


@pytest.mark.parametrize("head", ["hd64", "hd128", "hd72_ones", "ones_all16_fold", "ones_all16_delta"])
@pytest.mark.parametrize("shape", FM.SHAPES, ids=ids)
def test_cross_check_against_the_interleaved_kernels(vds, shape, head):
    """the device's own vds_attn_*_causal on the un-permuted rows, under the same variant mask and knobs (the CAUSAL
    siblings of the same kernel families): within twice the tolerances"""
    got = attn_run(vds["ops"], head, shape)
    other = to_fm(attn_run(vds["ops"], head, shape, frame_major=False), shape)
    errs = [rel(g_, r_) for g_, r_ in zip(got, other)]
    print("fm vs interleaved", ids(shape), head, " ".join(f"{n} {e:.2e}" for n, e in zip(NAMES, errs)))
    for name, e, tol in zip(NAMES, errs, TOLS):
        assert e < 2 * tol, f"{name}: rel {e:.3e} >= {2 * tol:.1e}"


@pytest.mark.parametrize("head", ["hd32", "hd96", "hd72_ones", "ones_all16_fold", "ones_all16_delta", "ones_fwd16_dkv16",
                                  "ones_dq16"])
@pytest.mark.parametrize("shape", [s for s in FM.SHAPES if s[2] > 1], ids=ids)
def test_later_frames_change_nothing_bit_for_bit_and_traps_stay_out(vds, shape, head):
    """other Q / dO rows, K x 32 and V = 1000 on the frames > f: o and lse of the rows of frames <= f move by exactly 0.0 and
    their dq is bit-identical -- the trapped keys sit in the diagonal sub-blocks of frame f's queries and in the tiles the
    early query tiles skip, and enter neither a running maximum nor o; the whole output still matches the reference"""
    L, lead, period = shape
    S = (L - lead) // period
    hd = HEADS[head][0]
    base = attn_run(vds["ops"], head, shape)
    ran = 0
    for f in sorted({0, period // 2, period - 2}):  # group f + 1 is the last one kept
        if f + 1 >= period:
            continue
        later = (lead, period, f + 1)
        got = attn_run(vds["ops"], head, shape, later=later)
        n = lead + (f + 1) * S  # frame-major rows of the groups <= f + 1
        keep_tok = FC.R.group_index(L, lead, period) <= f + 1
        assert same(got[0][:, :, keep_tok].contiguous(), base[0][:, :, keep_tok].contiguous()), ("o", f)
        assert same(got[1][:, :, :n].contiguous(), base[1][:, :, :n].contiguous()), ("lse", f)
        assert same(got[2][:, :, :n].contiguous(), base[2][:, :, :n].contiguous()), ("dq", f)
        assert not same(got[0], base[0]), "the later frames did not change"
        assert float(got[0][:, :, keep_tok].float().abs().max()) < 100.0  # V = 1000 stayed out
        # the trapped problem against its own reference: o and lse on every row, dq on the kept rows.  (Not the gradients
        # of the trapped rows themselves: with V = 1000 their dP - delta cancels two numbers near 1000 * |dO| of which the
        # kernels' delta comes from a bf16 o -- an ill-conditioned input, not a mask question; dk / dv of the early keys
        # sum over those queries.)
        ref = to_fm(attn_reference(hd, shape, later), shape)
        assert rel(got[0], ref[0]) < TOL_O and rel(got[1], ref[1]) < TOL_LSE, (f, rel(got[0], ref[0]), rel(got[1], ref[1]))
        assert rel(got[2][:, :, :n], ref[2][:, :, :n]) < TOL_G, (f, rel(got[2][:, :, :n], ref[2][:, :, :n]))
        ran += 1
    assert ran, "no frame was trapped"


def test_graph_replay_and_tile_order(vds):
    """lead / period travel by value: a captured forward + backward replays to the eager bits; the heaviest-first tile
    order (knob attn_fm_heavy_first) changes no bit"""
    ops = vds["ops"]
    shape = (1040, 16, 4)
    for head in ("ones_all16_fold", "ones_mfma32"):
        eager = attn_run(ops, head, shape)
        replay = attn_run(ops, head, shape, graph=True)
        with Knobs(ops, {"attn_fm_heavy_first": 0}):
            plain_order = attn_run(ops, head, shape)
        for name, a, b, c in zip(NAMES, eager, replay, plain_order):
            assert same(a.contiguous(), b.contiguous()), (head, name)
            assert same(a.contiguous(), c.contiguous()), (head, name)


def test_attention_argument_errors(vds):
    import ctypes as C
    ops, _lib = vds["ops"], vds["lib"]
    L, hd = 166, 64
    q = torch.zeros(1, 2, L, hd, dtype=bf16, device="cuda")
    o = torch.zeros(1 * L, 2 * hd, dtype=bf16, device="cuda")
    lse = torch.zeros(1, 2, L, dtype=f32, device="cuda")
    ov = ops.heads_view(o, 1, L, 2, hd)
    with pytest.raises(ValueError, match="needs frames"):
        ops.attn_fwd(q, q, q, ov, lse, frame_major=True)
    with pytest.raises(ValueError, match="not with past or kv_lens"):
        ops.attn_fwd(q, q, q, ov, lse, frames=(16, 3), frame_major=True, kv_lens=torch.zeros(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="do not fit"):
        ops.attn_fwd(q, q, q, ov, lse, frames=(16, 4), frame_major=True)
    with pytest.raises(ValueError, match="self-attention"):
        ops.attn_fwd(q, q[:, :, :100], q[:, :, :100], ov, lse, frames=(16, 3), frame_major=True)
