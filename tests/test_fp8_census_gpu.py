"""Exact census of the fp8 path on the GPU: vds_quant_fp8, vds_absmax, vds_transpose_fp8, every instance vds_gemm_fp8
can launch, its fp8-emitting epilogues, and the three fp8-emitting row kernels -- bytes against tests/helpers/fp8_census.py.

Every call goes through the C entry point with explicit leading dimensions (the ops wrappers refuse M % 4 != 0 and
padded strides).  Every operand and output with a stride in the ABI runs dense and as a window of a wider parent: input
parents hold NaN (bf16 / f32) or 0x7f (fp8: NaN in both formats) outside the window, output parents the sentinel; after
the call the window equals the expectation bit for bit and every byte outside it is unchanged.  A quantised byte has ONE
right value, quant_ref's (proved against a float64 restatement on all finite bf16 patterns by
tests/test_fp8_census_cpu.py); the GEMM operands are small dyadic values whose products and fp32 sums are exact.  The
only bounded comparisons are the two GELU outputs and the fused column sums, with the bounds of the bf16 GEMM census.

Instance -> cases
  quant_kernel<fmt, trans>        all finite bf16 patterns x 5 amax x {q, qt, both}        test_quant_exhaustive
                                  16 shapes (M % 4 = 1, 2, 3: byte tails) x 3 amax         test_quant_shapes
  absmax_kernel                   the same parents, from a start below and one above        test_quant_shapes
  transpose_u8_kernel             16 shapes, all 256 byte values                            test_transpose
  gemm_kernel<NT, STORE, 1 | 2>   20 shapes, with and without bias                          test_gemm_store
  gemm_kernel<NT, F32, 1 | 2>     20 shapes x split_k 1, 3, -1, -3                          test_gemm_f32_nt
  gemm_kernel<TN, F32, 3>         12 shapes x split_k 0, 1, 3, -1, -3, atomics and deterministic   test_gemm_f32_tn
  gemm_kernel<NT, GATE_RES, 1>    20 shapes x rows_per_batch 73 (bias, none), 128; C == NULL  test_gemm_gate_res
  gemm_kernel<NT, BIAS_GELU, 1>   20 shapes, two outputs and C == NULL                      test_gemm_bias_gelu
  gemm_kernel<NT, DGELU, 2>       20 shapes                                                  test_gemm_dgelu
  the operand decoders            every finite byte, NT A / B side, a_fmt 0 / 1, TN A / B    test_gemm_decodes_every_byte
  the emitting epilogues          6 shapes x 5 amax_in x fmt 0 / 1, emit-only forms          test_gemm_emit
  rmsnorm / gate / qkv-RoPE _fp8  row_census cases, ldq = D + 8, 3 amax_in, fmt 0 / 1        test_*_emits_exact_fp8
  non-finite inputs               containment only; the bytes are printed, not asserted     test_nonfinite_inputs_are_contained
"""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import fp8_census as F  # noqa: E402
import gemm_census as G  # noqa: E402
import row_census as R  # noqa: E402

from video_diffusion_speedrun_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

bf16, f32, f64, u8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
NT, TN = _lib.VDS_NT, _lib.VDS_TN
EMBED = pytest.mark.parametrize("embedded", [False, True], ids=["dense", "embedded"])
FMT = pytest.mark.parametrize("fmt", [0, 1], ids=["e4m3", "e5m2"])
INF = float("inf")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Slot:
    """one operand or output on the GPU: the parent as it was (CPU), the parent on the device, the window handed to the
    kernel.  Bytes: `align` is the call's alignment rule for this pointer (16 fp8 operands, 8 q, 4 qt); the parent's
    leading dimension is the row length rounded up to it (dense) plus a gap of one step on either side (embedded)."""

    def __init__(self, t, embedded, fill="nan", align=16, pad_rows=3):
        if t.dim() == 1:
            t = t.view(1, -1)
        self.bytes = t.dtype == u8
        if self.bytes:
            extra = -t.shape[1] % align
            if embedded:
                self.before, self.where = F.embed_u8(t, pad_rows, 2 * align + extra, align)
            elif extra:
                self.before, self.where = F.embed_u8(t, 0, extra, 0)
            else:
                self.before, self.where = t.clone(), (0, 0, t.shape[0], t.shape[1])
        else:
            self.before, self.where = G.place(t, embedded, fill)
        self.dev = self.before.cuda()
        self.view = G.window(self.dev, self.where)

    @property
    def ptr(self):
        return self.view.data_ptr()

    @property
    def ld(self):
        return self.dev.stride(0)

    def poke(self, row, col, value):
        """write `value` at (row, col) RELATIVE to the window (outside it: a gap element) in both copies"""
        r0, c0 = self.where[0] + row, self.where[1] + col
        self.before[r0, c0] = value
        self.dev[r0, c0] = value

    def exact(self, want, what, allow_sentinel=False):
        if self.bytes:
            if allow_sentinel:
                got = G.window(self.dev.cpu(), self.where)
                assert torch.equal(got, want), (what, int((got != want).sum()))
                F.assert_outside_u8(self.dev, self.before, self.where, what)
            else:
                F.assert_window_u8(self.dev, self.before, self.where, want, what)
        else:
            G.assert_window(self.dev, self.before, self.where, want, what)

    def contained(self, what):
        if self.bytes:
            F.assert_outside_u8(self.dev, self.before, self.where, what)
        else:
            G.assert_outside(self.dev, self.before, self.where, what)

    def value(self):
        return self.view.cpu()


def src(t, embedded, align=16):
    return Slot(t, embedded, "nan", align)


def dst(rows, cols, dtype, embedded, init=None, align=16):
    if dtype == u8:
        return Slot(F.blank_u8(rows, cols) if init is None else init, embedded, "sentinel", align)
    return Slot(G.blank(rows, cols, dtype) if init is None else init, embedded, "sentinel")


class Scalar:
    """one device float between two sentinels"""

    def __init__(self, value=None):
        self.before = G.fill_value(f32, "sentinel").repeat(3)
        if value is not None:
            self.before[1] = value
        self.dev = self.before.cuda()
        self.ptr = self.dev.data_ptr() + 4

    def get(self):
        got = self.dev.cpu()
        assert torch.equal(G.bits(got[::2]), G.bits(self.before[::2])), "a neighbour of a device scalar changed"
        return got[1:2]


def f32bits(v):
    return int(G.bits(torch.as_tensor(v, dtype=f32).reshape(1))[0])


def check_dq(got, fmt, amax, what):
    """*dq_out as fp32 bits: amax / fmax exactly where the quotient is exact (dyadic amax, 0 -> 1), else within one ulp"""
    _, want = F.scale_of(fmt, amax)
    dyadic = amax == 0 or math.frexp(amax / F.FMAX[fmt])[0] == 0.5
    d = abs(f32bits(got) - f32bits(want))
    assert d <= (0 if dyadic else 1), f"{what}: dq_out {got.item()!r}, want {want.item()!r} ({d} ulps)"


# ---- quantiser ---------------------------------------------------------------------------------------------------------
def quant(lib, x, M, K, fmt, amax, q, qt, dq, rec):
    rc = lib.vds_quant_fp8(x.ptr, x.ld, M, K, fmt, amax.ptr, q.ptr if q else None, q.ld if q else 0, qt.ptr if qt else None,
                           qt.ld if qt else 0, dq.ptr if dq else None, rec.ptr if rec else None, stream())
    assert rc == 0, rc


@EMBED
@FMT
@pytest.mark.parametrize("outputs", ["q", "qt", "both"])
def test_quant_exhaustive(lib, fmt, outputs, embedded):
    """all 65 536 bf16 patterns (the 256 non-finite ones replaced by finite ones): 252 / 246 exact ties at a dyadic scale,
    the subnormal range, both zeros, saturation -- against quant_ref, byte for byte, row-major and transposed"""
    xm = F.pattern_matrix(True)
    top = float(xm.to(f32).abs().max())
    n = 0
    for i, amax in enumerate(F.amax_values(fmt)):
        want, _ = F.quant_ref(xm, fmt, amax)
        for start in (0.0, 1.0, INF):
            what = f"quant fmt {fmt} {outputs} amax {F.AMAX_NAMES[i]} start {start} {'embedded' if embedded else 'dense'}"
            x = src(xm, embedded)
            q = dst(256, 256, u8, embedded, align=8) if outputs != "qt" else None
            qt = dst(256, 256, u8, embedded, align=4) if outputs != "q" else None
            am, dq, rec = Scalar(amax), Scalar(), Scalar(start)
            quant(lib, x, 256, 256, fmt, am, q, qt, dq, rec)
            if q:
                q.exact(want, what + " q")
            if qt:
                qt.exact(want.t().contiguous(), what + " qt")
            check_dq(dq.get(), fmt, amax, what)
            assert f32bits(rec.get()) == f32bits(max(start, top)), (what, rec.get())
            assert f32bits(am.get()) == f32bits(amax), what + ": amax was written"
            n += 1
    assert n == 15


@EMBED
@FMT
def test_quant_shapes(lib, fmt, embedded):
    """the shape list (byte tails of the transposed copy: M % 4 = 1, 2, 3; one element; tiles below / at / past 128): the
    largest magnitude is the LAST valid element, a larger finite value sits in the gap right of it and below it (embedded)
    and must not reach amax_out; vds_absmax on the same parent, accumulating from a nonzero start"""
    n = 0
    for M, K in F.SHAPES_QUANT:
        xm = F.draw(M, K)
        for amax in F.SHAPE_AMAX:
            want, _ = F.quant_ref(xm, fmt, amax)
            for both in (True, False):
                what = f"quant fmt {fmt} {M}x{K} amax {amax} {'q + qt' if both else 'qt'} {'embedded' if embedded else 'dense'}"
                x = src(xm, embedded)
                if embedded:
                    x.poke(M - 1, K, F.BEYOND)
                    x.poke(M, K - 1, F.BEYOND)
                q = dst(M, K, u8, embedded, align=8) if both else None
                qt = dst(K, M, u8, embedded, align=4)
                am, dq, rec = Scalar(amax), Scalar(), Scalar(0.5)
                quant(lib, x, M, K, fmt, am, q, qt, dq, rec)
                if q:
                    q.exact(want, what + " q")
                qt.exact(want.t().contiguous(), what + " qt")
                check_dq(dq.get(), fmt, amax, what)
                assert f32bits(rec.get()) == f32bits(F.PEAK), (what, rec.get())
                n += 1
        for start, end in ((7.0, F.PEAK), (1000.0, 1000.0)):
            rec = Scalar(start)
            assert lib.vds_absmax(x.ptr, x.ld, M, K, rec.ptr, stream()) == 0
            assert f32bits(rec.get()) == f32bits(end), (f"absmax {M}x{K} from {start}", rec.get())
    assert n == len(F.SHAPES_QUANT) * 6


@EMBED
def test_transpose(lib, embedded):
    """all 256 byte values on the shape list.  The output window starts as the COMPLEMENT of the expectation (the byte
    sentinel is one of the values here), the parent around it as the sentinel."""
    for M, K in F.SHAPES_TRANSPOSE:
        idx = torch.arange(M * K).view(M, K)
        qm = ((idx * 37 + idx // K * 11 + 5) % 256).to(u8)
        assert M * K < 2048 or len(torch.unique(qm)) == 256
        want = qm.t().contiguous()
        q = src(qm, embedded)
        qt = dst(K, M, u8, embedded, init=255 - want, align=4)
        rc = lib.vds_transpose_fp8(q.ptr, q.ld, M, K, qt.ptr, qt.ld, stream())
        assert rc == 0, rc
        qt.exact(want, f"transpose {M}x{K} {'embedded' if embedded else 'dense'}", allow_sentinel=True)


# ---- fp8 GEMM ----------------------------------------------------------------------------------------------------------
def dev_scalar(v):
    return None if v is None else Scalar(v)


def gemm8(lib, layout, epi, M, N, K, A, B, Cs=None, C2=None, bias=None, aux=None, gate=None, rpb=0, split_k=1, sa=None, sb=None,
          a_fmt=0, emit=None):
    def p(s):
        return s.ptr if s is not None else None

    def ld(s):
        return s.ld if s is not None else 0

    a = _lib.GemmArgs(layout, epi, M, N, K, p(A), ld(A), p(B), ld(B), p(Cs), ld(Cs), p(C2), ld(C2), p(bias), p(aux), ld(aux),
                      p(gate), ld(gate), rpb, split_k, None)
    s_a, s_b = dev_scalar(sa), dev_scalar(sb)
    e = None
    if emit is not None:
        e = C.byref(_lib.Fp8Out(p(emit.get("q")), ld(emit.get("q")), p(emit.get("qt")), ld(emit.get("qt")), p(emit.get("amax_in")),
                                p(emit.get("amax_out")), p(emit.get("dq_out")), emit["fmt"], p(emit.get("colsum"))))
    rc = lib.vds_gemm_fp8(C.byref(a), p(s_a), p(s_b), a_fmt, 0, e, stream())
    _lib.check(rc, f"gemm_fp8(layout={layout}, epi={epi}, {M}x{N}x{K}, split_k={split_k}, a_fmt={a_fmt})")


def tag(name, embedded, shape, extra=""):
    return f"{name} {'embedded' if embedded else 'dense'} {shape[0]}x{shape[1]}x{shape[2]} {extra}"


@EMBED
@FMT
def test_gemm_store(lib, fmt, embedded):
    """NT STORE, a_fmt 0 and 1, with and without bias: C == bf16(exact product x scales [+ bias])"""
    for i, shape in enumerate(F.SHAPES_GEMM_NT):
        M, N, K = shape
        d = F.dense_case("NT", M, N, K, fmt, i)
        A, B = src(d.A, embedded), src(d.B, embedded)
        for with_bias in (False, True):
            out = dst(M, N, bf16, embedded)
            gemm8(lib, NT, _lib.EPI_STORE, M, N, K, A, B, out, bias=src(d.bias, embedded) if with_bias else None, sa=d.sa, sb=d.sb,
                  a_fmt=fmt)
            out.exact(d.want_bias if with_bias else d.want, tag(f"STORE a_fmt {fmt} bias {with_bias} scales {d.sa} {d.sb}", embedded, shape))


def f32_want(c0, acc):
    want = (c0.double() + acc).to(f32)
    assert torch.equal(want.double(), c0.double() + acc), "C0 + the exact product must be an fp32 number"
    return want


@EMBED
@FMT
def test_gemm_f32_nt(lib, fmt, embedded):
    """NT F32, both a_fmt, split_k 1 (plain stores onto the sentinel), 3 (atomics onto zeros), -1 and -3 (onto nonzero
    integers); K = 400 with 3 splits leaves one split without a K tile"""
    for i, shape in enumerate(F.SHAPES_GEMM_NT):
        M, N, K = shape
        d = F.dense_case("NT", M, N, K, fmt, i + 1)
        A, B = src(d.A, embedded), src(d.B, embedded)
        for split in (1, 3, -1, -3):
            c0 = G.ints((M, N), -5, 5, 901 + M + N + K).to(f32) if split < 0 else torch.zeros(M, N, dtype=f32)
            out = dst(M, N, f32, embedded, init=None if split == 1 else c0)
            gemm8(lib, NT, _lib.EPI_F32, M, N, K, A, B, out, split_k=split, sa=d.sa, sb=d.sb, a_fmt=fmt)
            out.exact(f32_want(c0, d.acc), tag(f"NT F32 a_fmt {fmt} split_k {split} scales {d.sa} {d.sb}", embedded, shape))


@EMBED
@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
def test_gemm_f32_tn(ops, lib, det, embedded):
    """TN F32 (A [K, M] e5m2, B [K, N] e4m3, both token-major), split_k 0, 1, 3, -1, -3, also in deterministic mode"""
    if det:
        ops.set_deterministic(True, 16 << 20)
    try:
        for i, shape in enumerate(F.SHAPES_GEMM_TN):
            M, N, K = shape
            d = F.dense_case("TN", M, N, K, 1, i)
            A, B = src(d.A, embedded), src(d.B, embedded)
            for split in (0, 1, 3, -1, -3):
                c0 = G.ints((M, N), -5, 5, 901 + M + N + K).to(f32) if split < 0 else torch.zeros(M, N, dtype=f32)
                out = dst(M, N, f32, embedded, init=None if split in (0, 1) else c0)
                gemm8(lib, TN, _lib.EPI_F32, M, N, K, A, B, out, split_k=split, sa=d.sa, sb=d.sb, a_fmt=1)
                out.exact(f32_want(c0, d.acc), tag(f"TN F32 split_k {split} det {det} scales {d.sa} {d.sb}", embedded, shape))
    finally:
        if det:
            ops.set_deterministic(False)


@EMBED
def test_gemm_gate_res(lib, embedded):
    """NT GATE_RES on fp8 operands: y and x_new bit exact with rows_per_batch 73 (64-row steps straddle samples: the
    predicated epilogue) and 128, with and without bias; the C == NULL form gives the same x_new and leaves y alone"""
    for i, shape in enumerate(F.SHAPES_GEMM_NT):
        M, N, K = shape
        d = F.dense_case("NT", M, N, K, 0, i + 2)
        A, B = src(d.A, embedded), src(d.B, embedded)
        for rpb, with_bias in ((F.ROWS_PER_BATCH, True), (F.ROWS_PER_BATCH, False), (128, True)):
            gr = G.gate_res_case(F.as_dense(d), G.gate_rows_plain(M, rpb), -(-M // rpb), with_bias)
            bias = src(d.bias, embedded) if with_bias else None
            aux, gate = src(gr.aux, embedded), src(gr.gate, embedded)
            y, xn = dst(M, N, bf16, embedded), dst(M, N, bf16, embedded)
            what = tag(f"GATE_RES rows_per_batch {rpb} bias {with_bias} scales {d.sa} {d.sb}", embedded, shape)
            gemm8(lib, NT, _lib.EPI_GATE_RES, M, N, K, A, B, y, xn, bias=bias, aux=aux, gate=gate, rpb=rpb, sa=d.sa, sb=d.sb)
            y.exact(gr.y, what + "y")
            xn.exact(gr.x_new, what + "x_new")
            xn1 = dst(M, N, bf16, embedded)
            gemm8(lib, NT, _lib.EPI_GATE_RES, M, N, K, A, B, None, xn1, bias=bias, aux=aux, gate=gate, rpb=rpb, sa=d.sa, sb=d.sb)
            xn1.exact(gr.x_new, what + "x_new of the C == NULL form")
            y.exact(gr.y, what + "y after the C == NULL launch")


def bounded(got, want64, bound, what):
    err = (got.double() - want64).abs()
    ok = bound > 0
    ratio = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
    bad = ~(err <= bound)   # (also catches NaN)
    assert not bad.any(), (what, int(bad.sum()), got[bad][:4], want64[bad][:4])
    return ratio


@EMBED
def test_gemm_bias_gelu(lib, embedded, parity_log):
    """NT BIAS_GELU (a_fmt 0), sparse dyadic set: `pre` bit exact; `act` within 2^-8 |want| + 1.5e-4 min(|x|, 1), the table
    bound of the bf16 census (the fp8 GEMM always runs the 256^2 kernel, whose epilogues read g_gelu_lut); C == NULL
    gives the same act bits"""
    worst = 0.0
    for shape in F.SHAPES_GEMM_NT:
        M, N, K = shape
        s = F.sparse_case(M, N, K)
        A, B, bias = src(s.A, embedded), src(s.B, embedded), src(s.bias, embedded)
        pre, act = dst(M, N, bf16, embedded), dst(M, N, bf16, embedded)
        what = tag("BIAS_GELU", embedded, shape)
        gemm8(lib, NT, _lib.EPI_BIAS_GELU, M, N, K, A, B, pre, act, bias=bias, sa=s.sa, sb=s.sb)
        pre.exact(s.pre, what + "pre")
        act.contained(what + "act")
        got = act.value()
        r = bounded(got, s.act64, G.gelu_bound(s.act64, s.pre64, True), what + "act")
        print(f"{what}: act worst error / bound {r:.4f}")
        worst = max(worst, r)
        act1 = dst(M, N, bf16, embedded)
        gemm8(lib, NT, _lib.EPI_BIAS_GELU, M, N, K, A, B, None, act1, bias=bias, sa=s.sa, sb=s.sb)
        act1.exact(got, what + "act of the C == NULL form against the two-output launch")
        pre.exact(s.pre, what + "pre after the C == NULL launch")
    parity_log("fp8_census.bias_gelu.act", embedded=embedded, cases=len(F.SHAPES_GEMM_NT), worst_error_over_bound=worst)


@EMBED
def test_gemm_dgelu(lib, embedded, parity_log):
    """NT DGELU (a_fmt 1): C = bf16(acc gelu'(aux)) within 2^-8 |want| + 1.5e-4 |acc| (the table bound)"""
    worst = 0.0
    for shape in F.SHAPES_GEMM_NT:
        M, N, K = shape
        dg = F.dgelu_case(M, N, K)
        A, B, aux = src(dg.A, embedded), src(dg.B, embedded), src(dg.aux, embedded)
        out = dst(M, N, bf16, embedded)
        what = tag("DGELU", embedded, shape)
        gemm8(lib, NT, _lib.EPI_DGELU, M, N, K, A, B, out, aux=aux, sa=dg.sa, sb=dg.sb, a_fmt=1)
        out.contained(what)
        r = bounded(out.value(), dg.want64, G.dgelu_bound(dg.want64, dg.acc, True), what)
        print(f"{what}: worst error / bound {r:.4f}")
        worst = max(worst, r)
    parity_log("fp8_census.dgelu", embedded=embedded, cases=len(F.SHAPES_GEMM_NT), worst_error_over_bound=worst)


@EMBED
def test_gemm_decodes_every_byte(lib, embedded):
    """one nonzero product per dot product, EPI_F32, scales NULL: C holds the decoded value of every finite byte --
    subnormals, the top of the range and -0 (as +0) -- on the A and the B route of NT (a_fmt 0 and 1) and of TN"""
    for c in F.decode_cases():
        A, B = src(c.A, embedded), src(c.B, embedded)
        out = dst(c.M, c.N, f32, embedded)
        gemm8(lib, NT if c.layout == "NT" else TN, _lib.EPI_F32, c.M, c.N, c.K, A, B, out, a_fmt=c.a_fmt)
        out.exact(c.want, f"decode {c.name} {'embedded' if embedded else 'dense'}")


# ---- GEMM emit ---------------------------------------------------------------------------------------------------------
def colsum_check(cs, c0, stored, M, what):
    """colsum - c0 against the float64 column sums of the STORED bf16 result: the bound of the bf16 census,
    M 2^-24 sum_m |C| + ceil(M / 64) 2^-24 |c0| (at most one atomic per 256-row tile here)"""
    cs.contained(what + " colsum")
    got = cs.value()[0].double()
    assert torch.isfinite(got).all(), what + " colsum is not finite"
    c64 = stored.double()
    err = (got - c0 - c64.sum(0)).abs()
    bound = M * 2.0 ** -24 * c64.abs().sum(0) + -(-M // 64) * 2.0 ** -24 * c0.abs()
    bad = ~(err <= bound)
    assert not bad.any(), (what, "colsum", int(bad.sum()), err[bad][:4], bound[bad][:4])
    return float((err / bound).max())


@EMBED
@pytest.mark.parametrize("efmt", [0, 1], ids=["to_e4m3", "to_e5m2"])
@pytest.mark.parametrize("epi", ["BIAS_GELU", "DGELU"])
def test_gemm_emit(lib, epi, efmt, embedded, parity_log):
    """the emitting epilogues: q and qt == quant_ref, on the CPU, of the bf16 result THE SAME LAUNCH stored ("rounded to
    bf16 first"; that result is bounded against float64 by the two tests above) -- full sub-tiles only (fmed3f clamp,
    templated conversion), partial only (fminf(fmaxf()) clamp, run-time conversion), qt byte tails of 1, the three
    last-column cases; amax_in exact, half (saturates), 0, 2 and fmax / 256 (a dyadic scale: ties); amax_out from 0, below
    and above; column sums; the emit-only launches (no bf16 result) write the same bytes"""
    gelu = epi == "BIAS_GELU"
    worst = 0.0
    for shape in F.SHAPES_EMIT:
        M, N, K = shape
        if gelu:
            c = F.sparse_case(M, N, K)
            code = _lib.EPI_BIAS_GELU
        else:
            c = F.dgelu_case(M, N, K)
            code = _lib.EPI_DGELU
        A, B = src(c.A, embedded), src(c.B, embedded)
        bias = src(c.bias, embedded) if gelu else None
        aux = None if gelu else src(c.aux, embedded)

        def launch(res, emit, pre=None):
            if gelu:
                gemm8(lib, NT, code, M, N, K, A, B, pre, res, bias=bias, sa=c.sa, sb=c.sb, a_fmt=0, emit=emit)
            else:
                gemm8(lib, NT, code, M, N, K, A, B, res, aux=aux, sa=c.sa, sb=c.sb, a_fmt=1, emit=emit)
        plain = dst(M, N, bf16, embedded)
        launch(plain, None, dst(M, N, bf16, embedded) if gelu else None)
        top = float(plain.value().float().abs().max())
        assert top > 0
        c0 = G.ints((N,), 1, 3, 77 + N) * (G.ints((N,), 0, 1, 78 + N) * 2 - 1)
        for j, amax_in in enumerate((top, top / 2, 0.0, 2.0, F.FMAX[efmt] / 256)):
            start = (0.0, top / 4, top * 4)[j % 3]
            what = tag(f"{epi} emit fmt {efmt} amax_in {amax_in} start {start}", embedded, shape)
            res, pre = dst(M, N, bf16, embedded), (dst(M, N, bf16, embedded) if gelu else None)
            q, qt = dst(M, N, u8, embedded, align=8), dst(N, M, u8, embedded, align=4)
            am, rec, dq = Scalar(amax_in), Scalar(start), Scalar()
            cs = dst(1, N, f32, embedded, init=c0.to(f32).view(1, N))
            launch(res, dict(q=q, qt=qt, amax_in=am, amax_out=rec, dq_out=dq, fmt=efmt, colsum=cs), pre)
            res.exact(plain.value(), what + " the bf16 result against the launch without emit")
            if gelu:
                pre.exact(c.pre, what + " pre")
            stored = res.value()
            want, _ = F.quant_ref(stored, efmt, amax_in)
            q.exact(want, what + " q")
            qt.exact(want.t().contiguous(), what + " qt")
            check_dq(dq.get(), efmt, amax_in, what)
            assert f32bits(rec.get()) == f32bits(max(start, top)), (what, rec.get(), top)
            worst = max(worst, colsum_check(cs, c0, stored, M, what))
            # the emit-only forms (no bf16 result): the ONLY launches whose full sub-tiles take epilogue_full's quantiser
            # (BIAS_GELU -> e4m3 without column sums, DGELU -> e5m2 with and without); everything else above and below
            # runs epilogue_64x64's
            q1, qt1 = dst(M, N, u8, embedded, align=8), dst(N, M, u8, embedded, align=4)
            rec1, dq1 = Scalar(start), Scalar()
            launch(None, dict(q=q1, qt=qt1, amax_in=am, amax_out=rec1, dq_out=dq1, fmt=efmt), pre)
            q1.exact(want, what + " q of the emit-only launch")
            qt1.exact(want.t().contiguous(), what + " qt of the emit-only launch")
            check_dq(dq1.get(), efmt, amax_in, what + " emit-only")
            assert f32bits(rec1.get()) == f32bits(max(start, top)), (what, "emit-only", rec1.get(), top)
            q2, rec2 = dst(M, N, u8, embedded, align=8), Scalar(start)
            cs2 = dst(1, N, f32, embedded, init=c0.to(f32).view(1, N))
            launch(None, dict(q=q2, amax_in=am, amax_out=rec2, fmt=efmt, colsum=cs2), pre)
            q2.exact(want, what + " q alone, with column sums")
            assert f32bits(rec2.get()) == f32bits(max(start, top)), (what, "q alone", rec2.get(), top)
            worst = max(worst, colsum_check(cs2, c0, stored, M, what + " emit-only"))
            if gelu:
                pre.exact(c.pre, what + " pre after the emit-only launches")
    print(f"{epi} emit fmt {efmt}: colsum worst error / bound {worst:.4f}")
    parity_log("fp8_census.emit.colsum", epi=epi, fmt=efmt, embedded=embedded, cases=5 * len(F.SHAPES_EMIT),
               worst_error_over_bound=worst)


# ---- the fp8-emitting row kernels --------------------------------------------------------------------------------------
class Win:
    """a 2-D operand as a window of a wider parent: ld = columns + 8, four guard rows before and after"""

    def __init__(self, t, fill):
        if t.dtype == u8:
            self.before, self.where = F.embed_u8(t, R.GUARD_ROWS, R.GAP, 0)
        else:
            self.before, view = G.embed(t, pad_rows=R.GUARD_ROWS, pad_cols=R.GAP, col0=0, fill=fill)
            self.where = G.locate(self.before, view)
        self.dev = self.before.cuda()
        self.ld = self.before.stride(0)
        self.ptr = self.dev.data_ptr() + (self.where[0] * self.ld + self.where[1]) * t.element_size()

    def check(self, want, what):
        if want.dtype == u8:
            F.assert_window_u8(self.dev, self.before, self.where, want, what)
        else:
            G.assert_window(self.dev, self.before, self.where, want, what)

    def got(self):
        return G.window(self.dev.cpu(), self.where)


class Flat:
    def __init__(self, t, fill):
        self.initial, self.ptr = t, None
        if t is not None:
            self.before, _, guard = R.guarded(t, fill)
            self.dev = self.before.cuda()
            self.ptr = self.dev.data_ptr() + guard * t.element_size()

    def check(self, want, what, exact=True):
        return R.assert_guarded(self.dev, self.before, want, what, exact)


def blank_f32(*shape):
    return G.fill_value(f32, "sentinel").repeat(*shape)


def row_max(want):
    return want.to(f32).abs().max(1).values


def check_part(part, owned, what):
    """amax_part: `owned` maps entry -> expected value (fp32 bits); every other entry keeps the sentinel"""
    want = blank_f32(part.initial.numel())
    for w, v in owned.items():
        want[w] = v
    part.check(want, what + " amax_part")
    return float(max(owned.values()))


def amax_ins(top):
    return (0.75 * top, 0.0, 2.0)   # stale (saturates), 0 (scale 1), a power of two


ROW_BL = [(1, 17), (3, 21), (2, 16)]          # tails of 1 and 3 rows, none
ROW_D = [8, 144, 384, 520, 1152, 2048]        # row<1>, row<1>, q4<3>, row<2>, q4<9>, row<4>


@FMT
@pytest.mark.parametrize("D", ROW_D)
def test_rmsnorm_fwd_emits_exact_fp8(lib, fmt, D):
    """vds_rmsnorm_mod_fwd_fp8 on the row census cases whose bf16 result is exactly known: q == quant_ref(that result);
    amax_part[row] = max |row| (one-row-per-wave kernels) or amax_part[4 i] = max of rows 4 i .. 4 i + 3 (the q4
    kernels at D = 384 / 768 / 1152), every other entry untouched; rstd as the row census expects"""
    for B, L in ROW_BL:
        for with_w in (False, True):
            c = R.fwd_case(B, L, D, with_w)
            rows = B * L
            rm = row_max(c.want_y)
            if R.q4_rule(D):
                owned = {w: float(rm[w:w + 4].max()) for w in range(0, rows, 4)}
            else:
                owned = {w: float(rm[w]) for w in range(rows)}
            top = float(rm.max())
            for amax_in in amax_ins(top):
                what = f"rmsnorm fp8 fmt {fmt} {R.fwd_instance(D)} B {B} L {L} D {D} w {with_w} amax_in {amax_in}"
                x, mod, w = Win(c.x, "nan"), Win(c.mod, "nan"), Flat(c.w, "nan")
                q, rstd = Win(F.blank_u8(rows, D), "sentinel"), Flat(blank_f32(rows), "sentinel")
                part, am, dq = Flat(blank_f32(rows), "sentinel"), Scalar(amax_in), Scalar()
                rc = lib.vds_rmsnorm_mod_fwd_fp8(x.ptr, x.ld, w.ptr, mod.ptr, mod.ld, 0, 2 * D, q.ptr, q.ld, fmt, am.ptr, part.ptr,
                                                 dq.ptr, rstd.ptr, B, L, D, R.EPS, stream())
                assert rc == 0, (what, rc)
                q.check(F.quant_ref(c.want_y, fmt, amax_in)[0], what + " q")
                assert check_part(part, owned, what) == top
                check_dq(dq.get(), fmt, amax_in, what)
                u = R.ulps32(rstd.check(c.r64.to(f32), what + " rstd", exact=False), c.r64)
                assert u <= 4.0, f"{what}: rstd is {u:.2f} fp32 ulps from float64"


GATE_BL = [(1, 9), (3, 21), (2, 16), (2, 3)]  # 9 and 63 rows: tails of 1 and 3, ragged last workgroups; L = 3 < 4 waves


@FMT
@pytest.mark.parametrize("D", [8, 144, 520, 1152, 2048])
def test_gate_bwd_emits_exact_fp8(ops, lib, fmt, D):
    """vds_gate_bwd_fp8: q == quant_ref(dy), dy = dxn gate exactly; wave w of workgroup (blk, b) walks rows blk rpb + w,
    + 4, ... of sample b and owns the entry of its FIRST row, b L + blk rpb + w; a wave without rows owns none, so every
    entry written lies below B L (L = 3: numbering the grid's waves instead would need 8 entries for 6 rows; ew_min_rows
    = 1: four times the array); d(gate) and dbias exact"""
    assert ops.knob_get("ew_min_rows") == 8 and ops.knob_get("ew_wgs") in (0, 768)
    for B, L in GATE_BL:
        run_gate_fp8(lib, fmt, B, L, D, 8)
    # ew_min_rows = 1: one row per workgroup, wave 0 alone has a row -- the grid's waves number 4 B L, the array holds B L
    prev = ops.knob_set("ew_min_rows", 1)
    try:
        for B, L in ((3, 21), (2, 3)):
            run_gate_fp8(lib, fmt, B, L, D, 1)
    finally:
        ops.knob_set("ew_min_rows", prev)


def run_gate_fp8(lib, fmt, B, L, D, min_rows):
    """one (B, L) of test_gate_bwd_emits_exact_fp8 under ew_min_rows = min_rows"""
    c = R.gate_case(B, L, D)
    rows, rpb = B * L, R.rows_per_block(L, B, min_rows)
    gx = -(-L // rpb)
    rm = row_max(c.want_dy)
    owned = {}
    for b in range(B):
        for blk in range(gx):
            for w in range(4):
                ls = range(blk * rpb + w, min(L, (blk + 1) * rpb), 4)
                if len(ls):
                    owned[b * L + ls[0]] = max(float(rm[b * L + l]) for l in ls)
    assert max(owned) < rows and (min_rows != 1 or (rpb == 1 and len(owned) == rows))
    top = float(rm.max())
    for amax_in in amax_ins(top):
        what = f"gate fp8 fmt {fmt} B {B} L {L} D {D} ew_min_rows {min_rows} amax_in {amax_in}"
        dxn, y, mod = Win(c.dxn, "nan"), Win(c.y, "nan"), Win(c.mod, "nan")
        q, dmod, dbias = Win(F.blank_u8(rows, D), "sentinel"), Win(c.dmod0, "sentinel"), Flat(c.dbias0, "sentinel")
        part, am, dq = Flat(blank_f32(rows), "sentinel"), Scalar(amax_in), Scalar()
        rc = lib.vds_gate_bwd_fp8(dxn.ptr, dxn.ld, y.ptr, y.ld, mod.ptr, mod.ld, 2 * D, q.ptr, q.ld, fmt, am.ptr, part.ptr,
                                  dq.ptr, dmod.ptr, dbias.ptr, B, L, D, stream())
        assert rc == 0, (what, rc)
        q.check(F.quant_ref(c.want_dy, fmt, amax_in)[0], what + " q")
        assert check_part(part, owned, what) == top
        check_dq(dq.get(), fmt, amax_in, what)
        dmod.check(c.want_dmod, what + " dmod")
        dbias.check(c.want_dbias, what + " dbias")


@FMT
@pytest.mark.parametrize("hd,hdp,H", [(64, 64, 2), (64, 64, 12), (72, 96, 16), (64, 64, 32)], ids=["tok1", "tok2", "tok3", "tok4"])
def test_qkv_rope_bwd_emits_exact_fp8(lib, fmt, hd, hdp, H):
    """vds_qkv_rope_bwd_fp8: q == quant_ref(dqkv) with ldq = 3 D + 8, amax_part[token] = max |row|; dv0_acc and dlam as the
    row census expects"""
    D3 = 3 * H * hd
    for B, L in R.QKV_BWD_BL:
        for mix, add_dv0 in R.QKV_BWD_MODES:
            c = R.qkv_bwd_case(B, L, H, hd, hdp, mix, add_dv0)
            rows = B * L
            rm = row_max(c.want_dqkv)
            owned = {t: float(rm[t]) for t in range(rows)}
            top = float(rm.max())
            for amax_in in amax_ins(top)[:2 if mix == 2 else 3]:
                what = f"qkv bwd fp8 fmt {fmt} B {B} L {L} H {H} hd {hd} mix {mix} add_dv0 {add_dv0} amax_in {amax_in}"
                dq_, dk, dv = Flat(c.dq, "nan"), Flat(c.dk, "nan"), Flat(c.dv, "nan")
                cos, sin, raw = Flat(c.cos, "nan"), Flat(c.sin, "nan"), Flat(c.qkv_raw, "nan")
                v0, lam = Flat(c.v0, "nan"), Flat(c.lam, "nan")
                acc, dlam = Flat(c.acc0, "sentinel"), Flat(c.dlam0, "sentinel")
                q = Win(F.blank_u8(rows, D3), "sentinel")
                part, am, dq = Flat(blank_f32(rows), "sentinel"), Scalar(amax_in), Scalar()
                rc = lib.vds_qkv_rope_bwd_fp8(dq_.ptr, dk.ptr, dv.ptr, cos.ptr, sin.ptr, raw.ptr, v0.ptr, lam.ptr, acc.ptr, dlam.ptr,
                                              q.ptr, q.ld, fmt, am.ptr, part.ptr, dq.ptr, mix, add_dv0, B, L, H, hd, hdp, stream())
                assert rc == 0, (what, rc)
                q.check(F.quant_ref(c.want_dqkv, fmt, amax_in)[0], what + " q")
                assert check_part(part, owned, what) == top
                check_dq(dq.get(), fmt, amax_in, what)
                acc.check(c.want_acc, what + " dv0_acc")
                dlam.check(c.want_dlam, what + " dlam")


# ---- non-finite inputs: containment and record -------------------------------------------------------------------------
POISON = (float("nan"), INF, -INF)


def test_nonfinite_inputs_are_contained(lib, capsys):
    """one NaN, one +Inf and one -Inf in otherwise finite input, at each site that quantises: every output byte that does
    not derive from those three elements equals the run without them, and nothing outside the windows changes.  WHAT
    the three bytes and the recorded amax become is printed (DESIGN.md 25 holds the table) and deliberately not asserted:
    whether NaN should survive quantisation is a separate decision."""
    table = []

    def values(poison):
        return POISON if poison == 1 else (POISON[0],) * 3

    def record(site, bytes3, amax, amax_nan):
        table.append(f"nonfinite | {site:62s} | NaN -> {bytes3[0]:#04x} | +Inf -> {bytes3[1]:#04x} | -Inf -> {bytes3[2]:#04x} | "
                     f"amax {amax!r} | amax with NaN alone {amax_nan!r}")

    # vds_quant_fp8, both copies
    M, K = 130, 136
    spots = [(5, 17), (64, 70), (129, 135)]
    for fmt in (0, 1):
        outs = []
        for poison in (0, 1, 2):   # clean | NaN, +Inf, -Inf | NaN alone (for the recorded amax)
            xm = F.draw(M, K).clone()
            if poison:
                for (i, j), v in zip(spots, values(poison)):
                    xm[i, j] = v
            x, q, qt = src(xm, True), dst(M, K, u8, True, align=8), dst(K, M, u8, True, align=4)
            am, rec = Scalar(112.0), Scalar(0.0)
            quant(lib, x, M, K, fmt, am, q, qt, None, rec)
            q.contained("nonfinite quant q"), qt.contained("nonfinite quant qt")
            outs.append((q.value(), qt.value(), rec.get().item()))
        keep = torch.ones(M, K, dtype=torch.bool)
        for i, j in spots:
            keep[i, j] = False
        assert torch.equal(outs[0][0][keep], outs[1][0][keep]) and torch.equal(outs[0][1].t()[keep], outs[1][1].t()[keep])
        assert torch.equal(outs[1][0], outs[1][1].t()), "q and qt disagree on the non-finite elements"
        record(f"vds_quant_fp8 fmt {fmt}", [int(outs[1][0][i, j]) for i, j in spots], outs[1][2], outs[2][2])

    # the GEMM's emitting epilogues, on a shape with full sub-tiles only and one with partial ones only.  Which quantiser
    # runs is epilogue_full_dispatch's choice: a full sub-tile goes to epilogue_full (fmed3f clamp, templated conversion,
    # the caller's e_max) only in the emit-only forms the model launches -- BIAS_GELU -> e4m3 with C2 == NULL and no
    # column sums (fp8.fwd_gelu_emit), DGELU -> e5m2 with C == NULL (fp8.dgrad_gelu_emit) -- and every other launch, and
    # every partial sub-tile, to epilogue_64x64 (fminf(fmaxf()), run-time conversion).
    # BIAS_GELU: the three values in the bias, one output column each.  DGELU: its table look-up clamps the index, so a
    # non-finite aux never reaches the quantiser; the values enter as e5m2 bytes of A (0x7e NaN, 0x7c / 0xfc +-Inf),
    # one output row each.
    for shape, tiles in (((256, 256, 128), "full sub-tiles"), ((63, 64, 112), "partial sub-tiles")):
        M, N, K = shape
        full = tiles == "full sub-tiles"
        c = F.sparse_case(M, N, K)
        cols = [3, N // 2 + 1, N - 1]
        keep = torch.ones(M, N, dtype=torch.bool)
        keep[:, cols] = False
        for form, efmt in (("two outputs", 0), ("two outputs", 1), ("emit-only", 0)):
            path = "epilogue_full" if full and form == "emit-only" else "epilogue_64x64"
            outs = []
            for poison in (0, 1, 2):   # clean | NaN, +Inf, -Inf | NaN alone (for the recorded amax)
                bm = c.bias.clone()
                if poison:
                    for j, v in zip(cols, values(poison)):
                        bm[j] = v
                A, B, bias = src(c.A, True), src(c.B, True), src(bm, True)
                pre = dst(M, N, bf16, True)
                res = dst(M, N, bf16, True) if form == "two outputs" else None
                q, qt = dst(M, N, u8, True, align=8), dst(N, M, u8, True, align=4)
                am, rec = Scalar(2.0), Scalar(0.0)
                gemm8(lib, NT, _lib.EPI_BIAS_GELU, M, N, K, A, B, pre, res, bias=bias, sa=c.sa, sb=c.sb, a_fmt=0,
                      emit=dict(q=q, qt=qt, amax_in=am, amax_out=rec, fmt=efmt))
                for s in (pre, res, q, qt):
                    if s is not None:
                        s.contained(f"nonfinite BIAS_GELU {form} {tiles}")
                outs.append((q.value(), qt.value(), rec.get().item(), res.value() if res is not None else None, pre.value()))
            assert torch.equal(outs[0][0][keep], outs[1][0][keep]) and torch.equal(outs[0][1].t()[keep], outs[1][1].t()[keep])
            assert torch.equal(G.bits(outs[0][4])[keep], G.bits(outs[1][4])[keep])
            if form == "two outputs":
                assert torch.equal(G.bits(outs[0][3])[keep], G.bits(outs[1][3])[keep])
            assert torch.equal(outs[1][0], outs[1][1].t()), "q and qt disagree on the non-finite elements"
            record(f"gemm BIAS_GELU {form} fmt {efmt}, {tiles}: {path}", [int(outs[1][0][0, j]) for j in cols], outs[1][2],
                   outs[2][2])
            if form == "two outputs":
                table.append(f"nonfinite | {'  (its bf16 activations, row 0)':44s} | "
                             + " | ".join(repr(outs[1][3][0, j].item()) for j in cols))
        dg = F.dgelu_case(M, N, K)
        rws = [3, M // 2 + 1, M - 1]
        keep = torch.ones(M, N, dtype=torch.bool)
        keep[rws] = False
        outs = []
        for poison in (0, 1, 2):
            Am = dg.A.clone()
            if poison:
                for r, b in zip(rws, (0x7E, 0x7C, 0xFC) if poison == 1 else (0x7E,) * 3):
                    Am[r, 5] = b
            A, B, aux = src(Am, True), src(dg.B, True), src(dg.aux, True)
            q, qt = dst(M, N, u8, True, align=8), dst(N, M, u8, True, align=4)
            am, rec = Scalar(2.0), Scalar(0.0)
            gemm8(lib, NT, _lib.EPI_DGELU, M, N, K, A, B, None, aux=aux, sa=dg.sa, sb=dg.sb, a_fmt=1,
                  emit=dict(q=q, qt=qt, amax_in=am, amax_out=rec, fmt=1))
            q.contained(f"nonfinite DGELU emit-only {tiles} q"), qt.contained(f"nonfinite DGELU emit-only {tiles} qt")
            outs.append((q.value(), qt.value(), rec.get().item()))
        assert torch.equal(outs[0][0][keep], outs[1][0][keep]) and torch.equal(outs[0][1].t()[keep], outs[1][1].t()[keep])
        assert torch.equal(outs[1][0], outs[1][1].t()), "q and qt disagree on the non-finite elements"
        # (a column whose B[n, 5] is zero: NaN and Inf times 0 are both NaN, so take the first column with B[n, 5] != 0)
        n0 = int((F.decode(dg.B[:, 5], 0) != 0).nonzero()[0])
        record(f"gemm DGELU emit-only fmt 1, {tiles}: {'epilogue_full' if full else 'epilogue_64x64'}",
               [int(outs[1][0][r, n0]) for r in rws], outs[1][2], outs[2][2])

    # the row producers: gate backward (dxn), qkv / RoPE backward (dv, mix 0), RMSNorm forward (the shift: one element each)
    B, L, D = 3, 21, 144
    rows = B * L
    spots = [(2, 5), (30, 77), (62, 143)]
    keep = torch.ones(rows, D, dtype=torch.bool)
    for i, j in spots:
        keep[i, j] = False
    g = R.gate_case(B, L, D)
    for fmt in (1, 0):
        outs = []
        for poison in (0, 1, 2):   # clean | NaN, +Inf, -Inf | NaN alone (for the recorded amax)
            dxnm = g.dxn.clone()
            if poison:
                for (i, j), v in zip(spots, values(poison)):
                    dxnm[i, j] = v
            dxn, y, mod = Win(dxnm, "nan"), Win(g.y, "nan"), Win(g.mod, "nan")
            q, dmod = Win(F.blank_u8(rows, D), "sentinel"), Win(g.dmod0, "sentinel")
            part, am = Flat(torch.zeros(rows, dtype=f32), "sentinel"), Scalar(2.0)
            rc = lib.vds_gate_bwd_fp8(dxn.ptr, dxn.ld, y.ptr, y.ld, mod.ptr, mod.ld, 2 * D, q.ptr, q.ld, fmt, am.ptr, part.ptr, None,
                                      dmod.ptr, None, B, L, D, stream())
            assert rc == 0
            F.assert_outside_u8(q.dev, q.before, q.where, "nonfinite gate q")
            outs.append((q.got(), part.check(part.initial, "nonfinite gate amax_part", exact=False).max().item()))
        assert torch.equal(outs[0][0][keep], outs[1][0][keep])
        record(f"vds_gate_bwd_fp8 fmt {fmt}", [int(outs[1][0][i, j]) for i, j in spots], outs[1][1], outs[2][1])
    f = R.fwd_case(B, L, D, False)
    for fmt in (0, 1):
        outs = []
        for poison in (0, 1, 2):   # clean | NaN, +Inf, -Inf | NaN alone (for the recorded amax)
            modm = f.mod.clone()
            if poison:   # shift of sample b at column j: the elements (row, j) of that sample -- one sample per value
                for b, v in enumerate(values(poison)):
                    modm[b, 5 + b] = v
            x, mod = Win(f.x, "nan"), Win(modm, "nan")
            q, rstd = Win(F.blank_u8(rows, D), "sentinel"), Flat(blank_f32(rows), "sentinel")
            part, am = Flat(torch.zeros(rows, dtype=f32), "sentinel"), Scalar(2.0)
            rc = lib.vds_rmsnorm_mod_fwd_fp8(x.ptr, x.ld, None, mod.ptr, mod.ld, 0, 2 * D, q.ptr, q.ld, fmt, am.ptr, part.ptr, None,
                                             rstd.ptr, B, L, D, R.EPS, stream())
            assert rc == 0
            F.assert_outside_u8(q.dev, q.before, q.where, "nonfinite rmsnorm q")
            outs.append((q.got(), part.check(part.initial, "nonfinite rmsnorm amax_part", exact=False).max().item()))
        keep_f = torch.ones(rows, D, dtype=torch.bool)
        for b in range(3):
            keep_f[b * L:(b + 1) * L, 5 + b] = False
        assert torch.equal(outs[0][0][keep_f], outs[1][0][keep_f])
        record(f"vds_rmsnorm_mod_fwd_fp8 fmt {fmt}", [int(outs[1][0][b * L, 5 + b]) for b in range(3)], outs[1][1], outs[2][1])
    Bq, Lq, H, hd = 3, 25, 2, 64
    k = R.qkv_bwd_case(Bq, Lq, H, hd, hd, 0, 0)
    rows, Dh = Bq * Lq, H * hd
    spots = [(0, 3, 1, 7), (1, 10, 0, 33), (2, 24, 1, 63)]   # (b, l, h, d) of dv -> dqkv[b L + l, 2 D + h hd + d]
    for fmt in (1, 0):
        outs = []
        for poison in (0, 1, 2):   # clean | NaN, +Inf, -Inf | NaN alone (for the recorded amax)
            dvm = k.dv.clone()
            if poison:
                for (b, l, h, d), v in zip(spots, values(poison)):
                    dvm[b, h, l, d] = v
            dq_, dk, dv = Flat(k.dq, "nan"), Flat(k.dk, "nan"), Flat(dvm, "nan")
            cos, sin = Flat(k.cos, "nan"), Flat(k.sin, "nan")
            q = Win(F.blank_u8(rows, 3 * Dh), "sentinel")
            part, am = Flat(torch.zeros(rows, dtype=f32), "sentinel"), Scalar(2.0)
            rc = lib.vds_qkv_rope_bwd_fp8(dq_.ptr, dk.ptr, dv.ptr, cos.ptr, sin.ptr, None, None, None, None, None, q.ptr, q.ld, fmt,
                                          am.ptr, part.ptr, None, 0, 0, Bq, Lq, H, hd, hd, stream())
            assert rc == 0
            F.assert_outside_u8(q.dev, q.before, q.where, "nonfinite qkv q")
            outs.append((q.got(), part.check(part.initial, "nonfinite qkv amax_part", exact=False).max().item()))
        keep_q = torch.ones(rows, 3 * Dh, dtype=torch.bool)
        at = [(b * Lq + l, 2 * Dh + h * hd + d) for b, l, h, d in spots]
        for i, j in at:
            keep_q[i, j] = False
        assert torch.equal(outs[0][0][keep_q], outs[1][0][keep_q])
        record(f"vds_qkv_rope_bwd_fp8 fmt {fmt}", [int(outs[1][0][i, j]) for i, j in at], outs[1][1], outs[2][1])
    with capsys.disabled():
        print()
        for line in table:
            print(line)
