"""Exact census of the bf16 GEMM on the GPU (vds_gemm_bf16 / vds_gemm_bf16_grouped, csrc/gemm.hip).

Operands are small integers or small dyadic rationals (tests/helpers/gemm_census.py), so the fp32 accumulator is exact
in any summation order: every comparison below except the two GELU outputs and the fused column sums is bit for bit,
every element, at every listed shape, under every tiling, once with dense operands and once with every operand and
output embedded as a window of a larger parent (input parents NaN-filled, output parents sentinel-filled: a leak from a
gap shows as NaN, a stray store as a changed guard element).  tests/test_gemm_census_cpu.py checks, without a GPU,
that the exactness conditions hold for every case and that assert_window flags each kind of kernel fault.

The tilings agree bit for bit on every case here: each is compared with the same exact expectation, so no tiling-
against-tiling comparison is added.
"""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_census as G  # noqa: E402

from video_diffusion_speedrun_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
NT, NN, TN = _lib.VDS_NT, _lib.VDS_NN, _lib.VDS_TN
LAYOUT = {"NT": NT, "NN": NN, "TN": TN}
EMBED = pytest.mark.parametrize("embedded", [False, True], ids=["dense", "embedded"])


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import ops as _ops
    return _ops


@pytest.fixture(params=[0, 128, 256, 2], ids=["auto", "t128", "t256", "t256x128"])
def tile(request, ops):
    """every census test runs under the dispatcher's own choice and with each of the three tilings pinned"""
    ops.gemm_force_tile(request.param)
    yield request.param
    ops.gemm_force_tile(0)


@pytest.fixture
def deterministic(ops):
    """vds_set_deterministic(1) for the duration of one test (the tests size the workspace themselves)"""
    ops.set_deterministic(True, 64 << 20)
    yield
    ops.set_deterministic(False)


class Slot:
    """one operand or output on the GPU: the parent as it was (CPU), the parent on the device, the window passed to the
    kernel (its pointer and the parent's leading dimension)"""

    def __init__(self, t, embedded, fill):
        if t.dim() == 1:
            t = t.view(1, -1)
        self.before, self.where = G.place(t, embedded, fill)
        self.dev = self.before.cuda()
        self.view = G.window(self.dev, self.where)

    @property
    def ptr(self):
        return self.view.data_ptr()

    @property
    def ld(self):
        return self.dev.stride(0)

    def exact(self, want, what):
        G.assert_window(self.dev, self.before, self.where, want, what)

    def contained(self, what):
        G.assert_outside(self.dev, self.before, self.where, what)

    def value(self):
        return self.view.cpu()


def src(t, embedded):
    return Slot(t, embedded, "nan")


def dst(rows, cols, dtype, embedded, init=None):
    return Slot(G.blank(rows, cols, dtype) if init is None else init, embedded, "sentinel")


def gemm(ops, layout, epi, M, N, K, A, B, Cs=None, C2=None, bias=None, aux=None, gate=None, rpb=0, split_k=1, colsum=None,
         groups=None):
    """the raw C-ABI call with explicit leading dimensions and the windows' pointers"""
    def p(s):
        return s.ptr if s is not None else None

    def ld(s):
        return s.ld if s is not None else 0

    a = _lib.GemmArgs(layout, epi, M, N, K, p(A), ld(A), p(B), ld(B), p(Cs), ld(Cs), p(C2), ld(C2), p(bias), p(aux), ld(aux),
                      p(gate), ld(gate), rpb, split_k, p(colsum))
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    if groups is None:
        rc = lib.vds_gemm_bf16(C.byref(a), stream)
    else:
        rc = lib.vds_gemm_bf16_grouped(C.byref(a), C.byref(_lib.ModGroups(*groups)), stream)
    _lib.check(rc, f"gemm(layout={layout}, epi={epi}, {M}x{N}x{K}, split_k={split_k}, groups={groups})")


def tag(name, tile, embedded, shape, extra=""):
    return f"{name} tile={tile} {'embedded' if embedded else 'dense'} {shape[0]}x{shape[1]}x{shape[2]} {extra}"


# ---- STORE -------------------------------------------------------------------------------------------------------------
@EMBED
@pytest.mark.parametrize("layout", ["NT", "NN"])
def test_store_is_bit_exact(ops, tile, layout, embedded):
    """NT STORE with and without bias and NN STORE, dense set, whole shape list: C == bf16(exact), guard bands intact"""
    n = 0
    for shape in G.SHAPES[layout]:
        M, N, K = shape
        d = G.dense_case(layout, M, N, K)
        A, B = src(d.A, embedded), src(d.B, embedded)
        for with_bias in ((False, True) if layout == "NT" else (False,)):
            bias = src(d.bias, embedded) if with_bias else None
            out = dst(M, N, bf16, embedded)
            gemm(ops, LAYOUT[layout], _lib.EPI_STORE, M, N, K, A, B, out, bias=bias)
            out.exact(d.want_bias if with_bias else d.want, tag(f"{layout} STORE bias={with_bias}", tile, embedded, shape))
            n += 1
    assert n == len(G.SHAPES[layout]) * (2 if layout == "NT" else 1)


# ---- BIAS_GELU ---------------------------------------------------------------------------------------------------------
@EMBED
def test_bias_gelu_pre_exact_act_bounded(ops, tile, embedded, parity_log):
    """NT BIAS_GELU, sparse dyadic set: `pre` bit exact, `act` per element within
    2^-8 |want| + 1.5e-4 min(|x|, 1) where the table is read (256^2 tiling: both epilogue bodies look gelu up in
    g_gelu_lut) and within 2^-8 |want| + 1e-6 where gelu comes from the formula (128^2 and 256x128 tilings: their
    epilogue_64x64 instances have LUT = false).  Under the dispatcher's own choice (tile 0) these shapes go to the 128^2
    kernel today, but that is the cost model's decision, so the table bound is applied there.  The single-output form
    (C == NULL) must give the same `act` bits and leave the earlier `pre` buffer alone."""
    table = tile in (0, 256)
    worst = 0.0
    for shape in G.SHAPES_NT:
        M, N, K = shape
        s = G.sparse_case(M, N, K)
        A, B, bias = src(s.A, embedded), src(s.B, embedded), src(s.bias, embedded)
        pre, act = dst(M, N, bf16, embedded), dst(M, N, bf16, embedded)
        what = tag("BIAS_GELU", tile, embedded, shape)
        gemm(ops, NT, _lib.EPI_BIAS_GELU, M, N, K, A, B, pre, act, bias=bias)
        pre.exact(s.pre, what + "pre")
        act.contained(what + "act")
        got = act.value()
        err = (got.double() - s.act64).abs()
        bound = G.gelu_bound(s.act64, s.pre64, table)
        ratio = float((err / bound.clamp(min=1e-300)).max())
        print(f"{what}: act worst error / bound {ratio:.4f}")
        worst = max(worst, ratio)
        bad = ~(err <= bound)   # (also catches NaN)
        assert not bad.any(), (what, int(bad.sum()), s.pre64[bad][:4], got[bad][:4], s.act64[bad][:4])
        # single-output form
        pre_kept = pre.dev.clone()
        act1 = dst(M, N, bf16, embedded)
        gemm(ops, NT, _lib.EPI_BIAS_GELU, M, N, K, A, B, None, act1, bias=bias)
        act1.exact(got, what + "act of the single-output form against the two-output launch")
        assert torch.equal(G.bits(pre.dev), G.bits(pre_kept)), what + "the single-output launch touched pre"
    parity_log("gemm_census.bias_gelu.act", tile=tile, embedded=embedded, cases=len(G.SHAPES_NT), table_bound=table,
               worst_error_over_bound=worst)


# ---- GATE_RES ----------------------------------------------------------------------------------------------------------
@EMBED
def test_gate_res_is_bit_exact(ops, tile, embedded):
    """NT GATE_RES, dense set: y and x_new bit exact with rows_per_batch = 73 (64-row sub-tiles straddle samples: the
    predicated epilogue) and 128 (sub-tiles inside one sample: the lean one), bias and no bias; the single-output form
    gives the same x_new bits; aux, gate (ldgate > N, a column offset) and both outputs are windows when embedded"""
    n = 0
    for shape in G.SHAPES_NT:
        M, N, K = shape
        d = G.dense_case("NT", M, N, K)
        A, B = src(d.A, embedded), src(d.B, embedded)
        for rpb, with_bias in ((G.ROWS_PER_BATCH, True), (G.ROWS_PER_BATCH, False), (128, True)):
            nb = -(-M // rpb)
            gr = G.gate_res_case(d, G.gate_rows_plain(M, rpb), nb, with_bias)
            bias = src(d.bias, embedded) if with_bias else None
            aux, gate = src(gr.aux, embedded), src(gr.gate, embedded)
            y, xn = dst(M, N, bf16, embedded), dst(M, N, bf16, embedded)
            what = tag("GATE_RES", tile, embedded, shape, f"rows_per_batch={rpb} bias={with_bias} ")
            gemm(ops, NT, _lib.EPI_GATE_RES, M, N, K, A, B, y, xn, bias=bias, aux=aux, gate=gate, rpb=rpb)
            y.exact(gr.y, what + "y")
            xn.exact(gr.x_new, what + "x_new")
            xn1 = dst(M, N, bf16, embedded)
            gemm(ops, NT, _lib.EPI_GATE_RES, M, N, K, A, B, None, xn1, bias=bias, aux=aux, gate=gate, rpb=rpb)
            xn1.exact(gr.x_new, what + "x_new of the single-output form")
            y.exact(gr.y, what + "y after the single-output launch")
            n += 1
    assert n == 3 * len(G.SHAPES_NT)


@EMBED
def test_grouped_gate_res_is_bit_exact(ops, tile, embedded):
    """the grouped form (lead 16, period 3, S 19, B 4: 73 rows per sample, one gate row per modulation group): y and
    x_new bit exact, and bit-identical to a rows_per_batch = 1 launch with the expanded [M, N] gate table"""
    g = G.GROUPED
    L, ngroups = g["lead"] + g["period"] * g["S"], 1 + g["period"]
    for shape in G.SHAPES_GROUPED:
        M, N, K = shape
        assert M == g["B"] * L
        d = G.dense_case("NT", M, N, K)
        rows = G.gate_rows_grouped(M, L, g["lead"], g["period"])
        gr = G.gate_res_case(d, rows, g["B"] * ngroups)
        A, B, bias = src(d.A, embedded), src(d.B, embedded), src(d.bias, embedded)
        aux, gate = src(gr.aux, embedded), src(gr.gate, embedded)
        what = tag("GATE_RES grouped", tile, embedded, shape)
        for with_y in (True, False):
            y, xn = (dst(M, N, bf16, embedded) if with_y else None), dst(M, N, bf16, embedded)
            gemm(ops, NT, _lib.EPI_GATE_RES, M, N, K, A, B, y, xn, bias=bias, aux=aux, gate=gate, rpb=L,
                 groups=(g["lead"], g["period"]))
            if with_y:
                y.exact(gr.y, what + "y")
            xn.exact(gr.x_new, what + f"x_new (y stored: {with_y})")
        table = src(gr.gate[rows].contiguous(), embedded)   # one gate row per output row
        y1, xn1 = dst(M, N, bf16, embedded), dst(M, N, bf16, embedded)
        gemm(ops, NT, _lib.EPI_GATE_RES, M, N, K, A, B, y1, xn1, bias=bias, aux=aux, gate=table, rpb=1)
        y1.exact(gr.y, what + "y of the rows_per_batch = 1 launch")
        xn1.exact(xn.value(), what + "x_new of the rows_per_batch = 1 launch against the grouped launch")


# ---- DGELU -------------------------------------------------------------------------------------------------------------
@EMBED
def test_dgelu_bounded_and_column_sums(ops, tile, embedded, parity_log):
    """NN DGELU: dy and W small integers (acc exact), aux arbitrary bf16 in [-6, 6]; C = bf16(acc gelu'(aux)) per element
    within 2^-8 |want| + 1.5e-4 |acc| where gelu' is read from the table (256^2 tiling; also applied under the
    dispatcher's own choice, see test_bias_gelu_pre_exact_act_bounded) and 2^-8 |want| + 1e-6 |acc| where it comes from
    the formula (128^2, 256x128).
    Column sums, on EVERY shape of the list (M = 1, 8 and 33 included): the same call with `colsum` (starting from nonzero
    integers c0) must store the same C bits, colsum must be finite, its guard band intact, and colsum - c0 must equal
    the float64 column sums of the STORED bf16 C within
        M 2^-24 sum_m |C[m, n]|  +  ceil(M / 64) 2^-24 |c0[n]|.
    Derivation: a column is summed with M fp32 adds in all (M - t inside t partial sums, t atomic adds onto colsum).  A
    partial sum of C values never exceeds sum |C|, so each of those adds rounds by at most 2^-24 sum |C|: the first term,
    the fp32 summation bound.  The t adds onto colsum act on a value that also holds the start c0, which adds at most
    2^-24 |c0| each: the second term.  t is read from the code: one atomic per 256-row tile in the fused epilogue of
    the 256^2 tiling, one per block of 64 rows in vds_colsum_bf16 (the other tilings), so t <= ceil(M / 64).  Without
    the second term a correct kernel fails at M = 1, where colsum = fl(c0 + C) and |C| can be 1e-8.
    NOTE the NaN guard rows exist only in the EMBEDDED variant (aux, like every operand, is then a window of a NaN-filled
    parent, so a sum that read rows at or past M would be NaN); the dense variant cannot detect such a read and checks
    the arithmetic alone.  The embedded variant runs under every tiling."""
    table = tile in (0, 256)
    worst = worst_cs = 0.0
    n_cs = 0
    for shape in G.SHAPES_NN:
        M, N, K = shape
        dg = G.dgelu_case(M, N, K)
        A, B, aux = src(dg.A, embedded), src(dg.B, embedded), src(dg.aux, embedded)
        out = dst(M, N, bf16, embedded)
        what = tag("DGELU", tile, embedded, shape)
        gemm(ops, NN, _lib.EPI_DGELU, M, N, K, A, B, out, aux=aux)
        out.contained(what)
        got = out.value()
        err = (got.double() - dg.want64).abs()
        bound = G.dgelu_bound(dg.want64, dg.acc, table)
        ratio = float((err / bound.clamp(min=1e-300))[bound > 0].max()) if (bound > 0).any() else 0.0
        print(f"{what}: worst error / bound {ratio:.4f}")
        worst = max(worst, ratio)
        bad = ~(err <= bound)
        assert not bad.any(), (what, int(bad.sum()), dg.aux[bad][:4], dg.acc[bad][:4], got[bad][:4], dg.want64[bad][:4])
        c0 = G.ints((N,), 1, 3, 77 + N) * (G.ints((N,), 0, 1, 78 + N) * 2 - 1)
        cs = dst(1, N, f32, embedded, init=c0.to(f32).view(1, N))
        out2 = dst(M, N, bf16, embedded)
        gemm(ops, NN, _lib.EPI_DGELU, M, N, K, A, B, out2, aux=aux, colsum=cs)
        out2.exact(got, what + "C with colsum against C without")
        cs.contained(what + "colsum")
        got_cs = cs.value()[0].double()
        assert torch.isfinite(got_cs).all(), what + "colsum is not finite"
        c64 = got.double()
        cs_err = (got_cs - c0 - c64.sum(0)).abs()
        cs_bound = M * 2.0 ** -24 * c64.abs().sum(0) + -(-M // 64) * 2.0 ** -24 * c0.abs()
        r = float((cs_err / cs_bound).max())   # (c0 is nonzero: so is the bound)
        print(f"{what}: colsum worst error / bound {r:.4f}")
        worst_cs = max(worst_cs, r)
        bad = ~(cs_err <= cs_bound)
        assert not bad.any(), (what, "colsum", int(bad.sum()), cs_err[bad][:4], cs_bound[bad][:4])
        n_cs += 1
    assert n_cs == len(G.SHAPES_NN)
    parity_log("gemm_census.dgelu", tile=tile, embedded=embedded, cases=len(G.SHAPES_NN), colsum_cases=n_cs,
               table_bound=table, worst_error_over_bound=worst, colsum_worst_error_over_bound=worst_cs)


@pytest.mark.parametrize("mode", ["default", "deterministic"])
def test_dgelu_column_sums_in_every_tiling_and_mode(ops, tile, mode):
    """NN DGELU with `colsum` at 264 x 328 x 328 (ragged rows, a narrow ragged last column on the 256-wide tiling, 5.1 K
    tiles) under every tiling, in the default mode (fused into the 256^2 epilogue, a vds_colsum_bf16 pass after the other
    tilings) and in deterministic mode (the pass after every tiling): C within dgelu_bound of the float64 expectation,
    the same C bits with and without colsum, and colsum - c0 within the bound derived in
    test_dgelu_bounded_and_column_sums of the float64 column sums of the stored C.  Operands embedded: NaN past M."""
    M, N, K = shape = (264, 328, 328)
    assert shape in G.SHAPES_NN
    dg = G.dgelu_case(M, N, K)
    A, B, aux = src(dg.A, True), src(dg.B, True), src(dg.aux, True)
    c0 = G.ints((N,), 1, 3, 77 + N) * (G.ints((N,), 0, 1, 78 + N) * 2 - 1)
    what = tag(f"DGELU colsum {mode}", tile, True, shape)
    if mode == "deterministic":
        ops.set_deterministic(True, 64 << 20)
    try:
        out, out2 = dst(M, N, bf16, True), dst(M, N, bf16, True)
        cs = dst(1, N, f32, True, init=c0.to(f32).view(1, N))
        gemm(ops, NN, _lib.EPI_DGELU, M, N, K, A, B, out, aux=aux)
        gemm(ops, NN, _lib.EPI_DGELU, M, N, K, A, B, out2, aux=aux, colsum=cs)
        torch.cuda.synchronize()
    finally:
        if mode == "deterministic":
            ops.set_deterministic(False)
    out.contained(what)
    got = out.value()
    err = (got.double() - dg.want64).abs()
    bound = G.dgelu_bound(dg.want64, dg.acc, tile in (0, 256))
    print(f"{what}: worst error / bound {float((err / bound.clamp(min=1e-300))[bound > 0].max()):.4f}")
    assert not (~(err <= bound)).any(), what
    out2.exact(got, what + "C with colsum against C without")
    cs.contained(what + "colsum")
    got_cs = cs.value()[0].double()
    c64 = got.double()
    cs_err = (got_cs - c0 - c64.sum(0)).abs()
    cs_bound = M * 2.0 ** -24 * c64.abs().sum(0) + -(-M // 64) * 2.0 ** -24 * c0.abs()
    print(f"{what}: colsum worst error / bound {float((cs_err / cs_bound).max()):.4f}")
    assert torch.isfinite(got_cs).all() and not (~(cs_err <= cs_bound)).any(), (what, "colsum")


# ---- TN F32 ------------------------------------------------------------------------------------------------------------
SPLITS =(1, 3, 5, 0, -1, -2)   # none | 3 | 5 (more splits than K tiles on most shapes) | the auto forms | accumulate


def _tn_census(ops, tile, embedded, mode, two_slabs=False):
    """NOTE there is no 256^2 TN kernel: gemm_bf16_impl ignores a pinned 256 tiling for TN, so the t256 runs of the three
    TN tests take the same kernels as the auto runs (128^2 here) and add no coverage of their own; TN is exercised on
    the 128^2 kernel (auto, t128, t256) and the 256x128 kernel (t256x128)."""
    n = 0
    for shape in G.SHAPES_TN:
        M, N, K = shape
        if two_slabs:
            if 2 * M * N * 4 < 4096:
                continue   # vds_set_deterministic takes no workspace below 4096 bytes
            ops.set_deterministic(True, 2 * M * N * 4)   # room for two slabs: 3 and 5 splits are lowered to 2
        d = G.dense_case("TN", M, N, K)
        A, B = src(d.A, embedded), src(d.B, embedded)
        for split in SPLITS:
            accumulate = split < 0
            c0 = G.ints((M, N), -5, 5, 901 + M + N + K).to(f32) if accumulate else torch.zeros(M, N, dtype=f32)
            out = dst(M, N, f32, embedded, init=c0)
            gemm(ops, TN, _lib.EPI_F32, M, N, K, A, B, out, split_k=split)
            want = (c0.double() + d.acc).to(f32)
            assert torch.equal(want.double(), c0.double() + d.acc)
            out.exact(want, tag(f"TN F32 {mode} split_k={split}", tile, embedded, shape))
            n += 1
    return n


@EMBED
def test_tn_f32_is_exact(ops, tile, embedded):
    """TN F32, dense set, split_k in 1, 3, 5, 0, -1, -2: C == C0 + exact (C0 integers for the accumulating forms, zero
    otherwise), with ldc > N and an intact sentinel around the window when embedded.  On small integers fp32 atomics
    commit the same number in any order."""
    assert _tn_census(ops, tile, embedded, "atomic") == len(G.SHAPES_TN) * len(SPLITS)


@EMBED
def test_tn_f32_is_exact_in_deterministic_mode(ops, tile, embedded, deterministic):
    """the same in deterministic mode: slabs in the workspace and the fixed-order reduction"""
    assert _tn_census(ops, tile, embedded, "deterministic") == len(G.SHAPES_TN) * len(SPLITS)


@EMBED
def test_tn_f32_is_exact_with_a_two_slab_workspace(ops, tile, embedded, deterministic):
    """deterministic mode with a workspace that holds only two slabs [M, N]: the split count is lowered to fit, the
    result stays exact (shapes below 512 outputs are left out: the library takes no workspace under 4096 bytes)"""
    n = sum(1 for M, N, _ in G.SHAPES_TN if 2 * M * N * 4 >= 4096)
    assert n >= len(G.SHAPES_TN) - 2 and _tn_census(ops, tile, embedded, "two slabs", two_slabs=True) == n * len(SPLITS)
