"""The fp8 census without a GPU: the reference is right, the lists cover what they claim, every builder's exactness
assertion holds, each emulated kernel fault is flagged by the very comparison the GPU test makes, and the host entry
points refuse what the kernels cannot address (the refusals run when the library is built; nothing is launched)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import fp8_census as F  # noqa: E402
import gemm_census as G  # noqa: E402

from video_diffusion_speedrun_amd import _lib  # noqa: E402

bf16, f32, f64, u8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
FMT = pytest.mark.parametrize("fmt", [0, 1], ids=["e4m3", "e5m2"])


def same(x, fmt, amax):
    """quant_ref against quant_ref64: values and the sign of zero"""
    q, _ = F.quant_ref(x, fmt, amax)
    v, d = F.quant_ref64(x, fmt, amax), F.decode(q, fmt)
    return torch.equal(d, v) and torch.equal(torch.signbit(d), torch.signbit(v)) and torch.equal(F.encode64(v, fmt), q)


# ---- the reference -----------------------------------------------------------------------------------------------------
@FMT
def test_decode_table_is_torchs(fmt):
    t = torch.arange(256, dtype=u8).view(F.DTYPES[fmt]).to(f64)
    d = F.decode_table(fmt)
    assert bool(((t == d) | (t.isnan() & d.isnan())).all()) and torch.equal(torch.signbit(t), torch.signbit(d))
    assert float(d[~d.isnan() & ~d.isinf()].max()) == F.FMAX[fmt]
    assert F.SENTINEL_U8 in F.nonfinite_bytes(fmt)


@FMT
def test_quant_ref_is_the_float64_rounding_on_every_finite_pattern(fmt):
    x = F.pattern_matrix(True)
    allpat = F.pattern_matrix(False)
    fin = torch.isfinite(allpat.to(f32))
    assert int(fin.sum()) == 65280 and torch.equal(G.bits(x)[fin], G.bits(allpat)[fin])
    for amax in F.amax_values(fmt) + [F.SHAPE_AMAX[1], F.SHAPE_AMAX[0]]:
        assert same(x, fmt, amax), (fmt, amax)
        q, dq = F.quant_ref(x, fmt, amax)
        assert not (q == F.SENTINEL_U8).any() and torch.isfinite(F.decode(q, fmt)).all()
        # dq: the fp32 quotient amax / fmax (the float64 quotient of two fp32 numbers, rounded once, IS that), 1 for amax 0
        assert float(dq) == (float(torch.tensor(amax / F.FMAX[fmt], dtype=f64).to(f32)) if amax else 1.0), (fmt, amax)
    assert float(F.quant_ref(x, fmt, 0.0)[1]) == 1.0 and float(F.quant_ref(x, fmt, F.FMAX[fmt])[1]) == 1.0


@FMT
def test_quant_ref_on_every_shape_input(fmt):
    for M, K in F.SHAPES_QUANT:
        x = F.draw(M, K)
        assert x.numel() * 2 <= F.MAX_OPERAND_BYTES and torch.isfinite(x.to(f32)).all()
        for amax in F.SHAPE_AMAX:
            assert same(x, fmt, amax), (M, K, amax)


def test_pattern_matrix_holds_every_pattern_and_every_class():
    x = F.pattern_matrix(False)
    assert torch.equal(torch.sort(G.bits(x).flatten().to(torch.int32) & 0xFFFF).values, torch.arange(65536, dtype=torch.int32))
    nan, inf = F.nonfinite_positions()
    assert len(nan) == 254 and len(inf) == 2
    xf = F.pattern_matrix(True)
    for fmt, n_ties in ((0, 252), (1, 246)):   # the ties among the 65 280 finite patterns at scale 1
        fin = torch.isfinite(x.to(f32))
        assert int((F.ties(xf, fmt, F.FMAX[fmt]) & fin).sum()) == n_ties
        c = {k: int(m.sum()) for k, m in F.classes(xf, fmt, F.FMAX[fmt]).items()}
        assert c["saturating"] > 25000 and c["+0 result"] > 10000 and c["-0 result"] > 10000 and c["subnormal result"] > 500
    for fmt, few in ((0, 40), (1, 8)):         # a non-dyadic scale leaves almost none
        assert int(F.ties(xf, fmt, 3.0).sum()) <= few


@pytest.mark.parametrize("which", ["quant", "transpose", "gemm_nt", "gemm_tn", "emit"])
def test_coverage_is_complete(which):
    missing = [k for k, v in F.coverage(which).items() if not v]
    assert not missing, missing


def test_shape_lists_are_legal_and_small():
    assert len(set(F.SHAPES_QUANT)) == 16 and all(K % 8 == 0 for _, K in F.SHAPES_QUANT)
    assert all(K % 16 == 0 for _, K in F.SHAPES_TRANSPOSE)
    assert all(K % 16 == 0 and N % 8 == 0 for _, N, K in F.SHAPES_GEMM_NT)
    assert all(M % 16 == 0 and K % 16 == 0 and N % 8 == 0 for M, N, K in F.SHAPES_GEMM_TN)
    for M, N, K in F.SHAPES_GEMM_NT + F.SHAPES_GEMM_TN:
        assert max(M * K, N * K, M * N * 4) <= F.MAX_OPERAND_BYTES, (M, N, K)
    assert F.empty_split(400, 3) and not F.empty_split(656, 3)


# ---- builders ----------------------------------------------------------------------------------------------------------
def test_gemm_builders_hold_their_exactness_conditions():
    for a_fmt in (0, 1):
        for off in (0, 1, 2):
            for i, (M, N, K) in enumerate(F.SHAPES_GEMM_NT):
                d = F.dense_case("NT", M, N, K, a_fmt, i + off)
                assert d.A.dtype == u8 and d.A.shape == (M, K) and d.B.shape == (N, K) and d.sa != d.sb
                assert torch.equal(d.acc.to(f32).to(f64), d.acc)
    assert F.unbiased_rounding_cases() >= len(F.SHAPES_GEMM_NT) // 2
    for i, (M, N, K) in enumerate(F.SHAPES_GEMM_TN):
        d = F.dense_case("TN", M, N, K, 1, i)
        assert d.A.shape == (K, M) and d.B.shape == (K, N)
        c0 = G.ints((M, N), -5, 5, 901 + M + N + K)
        assert torch.equal((c0 + d.acc).to(f32).to(f64), c0 + d.acc)
    sa = {s for s, _ in F.SCALES}
    sb = {s for _, s in F.SCALES}
    assert None in sa and None in sb and all(a != b for a, b in F.SCALES) and len(sa - {None, 1.0}) and len(sb - {None, 1.0})
    for i, (M, N, K) in enumerate(F.SHAPES_GEMM_NT):
        d = F.dense_case("NT", M, N, K, 0, i + 2)
        for rpb, with_bias in ((F.ROWS_PER_BATCH, True), (F.ROWS_PER_BATCH, False), (128, True)):
            gr = G.gate_res_case(F.as_dense(d), G.gate_rows_plain(M, rpb), -(-M // rpb), with_bias)
            assert gr.x_new.shape == (M, N)
        s = F.sparse_case(M, N, K)
        assert torch.equal(s.pre.to(f64), s.pre64)
        dg = F.dgelu_case(M, N, K)
        assert dg.A.shape == (M, K) and dg.B.shape == (N, K) and torch.isfinite(dg.want64).all()
    cases = F.decode_cases()
    assert len(cases) == 6
    for fmt in (0, 1):   # every finite byte of the format appears on the A route, and e4m3's on the B route
        finite = sorted(set(range(256)) - set(F.nonfinite_bytes(fmt)) - {0})
        a_side = [c for c in cases if "A side" in c.name and c.a_fmt == fmt]
        assert a_side and all(sorted(set(c.A.flatten().tolist()) - {0}) == finite for c in a_side)
    assert F.nonfinite_bytes(0) == [0x7F, 0xFF] and F.nonfinite_bytes(1) == [0x7C, 0x7D, 0x7E, 0x7F, 0xFC, 0xFD, 0xFE, 0xFF]


# ---- sensitivity -------------------------------------------------------------------------------------------------------
def flagged(bad, want, what, embedded=False):
    """the comparison of the GPU test (assert_window_u8 on a dense or embedded parent) must raise"""
    before, where = F.place_u8(F.blank_u8(*want.shape), embedded)
    after = before.clone()
    G.window(after, where).copy_(bad)
    with pytest.raises(AssertionError):
        F.assert_window_u8(after, before, where, want, what)


def accepted(good, want, embedded=False):
    before, where = F.place_u8(F.blank_u8(*want.shape), embedded)
    after = before.clone()
    G.window(after, where).copy_(good)
    F.assert_window_u8(after, before, where, want, "the right answer")


def old_input(M, K):
    """the input of tests/test_fp8_gpu.py::test_quant_matches_torch_float8: Gaussian, amax = max |x|"""
    x = (torch.randn(M, K, generator=torch.Generator().manual_seed(M + K)) * 3.0).to(bf16)
    x[0, 0] = 0.0
    return x, float(x.float().abs().max())


@FMT
def test_rounding_faults_need_the_pattern_matrix(fmt):
    """faults 1 and 2.  Truncation shows on any input.  Round-half-away differs from round-half-even on exact ties alone:
    the pattern matrix at a dyadic scale flags it on hundreds of elements; of the four Gaussian inputs of the older test
    (amax = max |x|) three hold at most one tie and do not flag it, with the true or with the stale amax"""
    x = F.pattern_matrix(True)
    for amax in F.amax_values(fmt)[:3]:
        want, _ = F.quant_ref(x, fmt, amax)
        accepted(want, want)
        flagged(F.fault_quant(x, fmt, amax, "trunc"), want, "truncation")
        flagged(F.fault_quant(x, fmt, amax, "away"), want, "round half away")
        assert F.mismatch(F.fault_quant(x, fmt, amax, "away"), want) >= 100
    for M, K in ((128, 128), (516, 1152), (4, 8)):
        xo, amax = old_input(M, K)
        want, _ = F.quant_ref(xo, fmt, amax)
        if M > 4:
            flagged(F.fault_quant(xo, fmt, amax, "trunc"), want, "truncation, Gaussian input")
        assert int(F.ties(xo, fmt, amax).sum()) <= 1
        assert F.mismatch(F.fault_quant(xo, fmt, amax, "away"), want) == 0, "the Gaussian input caught the tie fault"
        assert F.mismatch(F.fault_quant(xo, fmt, 0.75 * amax, "away"), F.quant_ref(xo, fmt, 0.75 * amax)[0]) == 0
    # (the fourth shape of that test, 300 x 136, draws amax = 12.25 = 49 / 4: fmax / amax is 256 / 7 resp. 32768 / 7, every
    # bf16 value with 7 | mantissa lands on the grid or half way, and the fault shows there -- by the accident of one seed)
    xo, amax = old_input(300, 136)
    assert amax == 12.25
    assert int(F.ties(xo, fmt, amax).sum()) > 100
    assert F.mismatch(F.fault_quant(xo, fmt, amax, "away"), F.quant_ref(xo, fmt, amax)[0]) > 100


@FMT
def test_quantiser_faults_are_flagged_on_every_shape(fmt):
    """faults 1-10 and 16 on the shape list: each is flagged on every shape where it can act (the predicate is stated
    per fault), row-major and transposed, dense and embedded"""
    acted = {k: 0 for k in ("trunc", "away", "no saturation", "other format", "bytes", "dwords", "tail", "scale after",
                            "amax 0", "row", "column")}
    for M, K in F.SHAPES_QUANT:
        x = F.draw(M, K)
        for amax in F.SHAPE_AMAX:
            want, _ = F.quant_ref(x, fmt, amax)
            wt = want.t().contiguous()
            what = f"{M}x{K} amax {amax}"
            for kind, key in (("trunc", "trunc"), ("away", "away"), ("no saturation", "no saturation"),
                              ("scale after rounding", "scale after")):
                bad = F.fault_quant(x, fmt, amax, kind)
                # can act: truncation / half-away where some scaled value is off the grid resp. on a tie whose even
                # neighbour is the lower one; no saturation where a scaled value exceeds fmax; the late scale where
                # rounding twice differs from rounding once -- in each case exactly where the faulty bytes differ
                if F.mismatch(bad, want):
                    flagged(bad, want, f"{kind} {what}")
                    flagged(bad.t().contiguous(), wt, f"{kind} {what} transposed", embedded=True)
                    acted[key] += 1
            if amax == F.SHAPE_AMAX[1]:   # scale 4 / 512: the last element (300) saturates on every shape
                assert F.mismatch(F.fault_quant(x, fmt, amax, "no saturation"), want) >= 1, what
                assert M * K < 64 or F.mismatch(F.fault_quant(x, fmt, amax, "trunc"), want) >= 1, what
            flagged(F.fault_quant(x, fmt, amax, "other format"), want, f"other format {what}")
            acted["other format"] += 1
            if amax == 0:
                flagged(F.fault_quant(x, fmt, 0.0, "amax 0 as scale 0"), want, f"amax 0 {what}")
                acted["amax 0"] += 1
            for kind, key in (("bytes of a dword swapped", "bytes"), ("dwords of a group swapped", "dwords"),
                              ("neighbouring row", "row"), ("neighbouring column", "column")):
                bad = F.fault_bytes(want, kind)
                if F.mismatch(bad, want):   # (cannot act where the swapped bytes are equal, or M == 1 for the row)
                    flagged(bad, want, f"{kind} {what}", embedded=True)
                    acted[key] += 1
                else:
                    assert M * K <= 64 or (kind == "neighbouring row" and M == 1), (kind, what)
            if M % 4:
                bad = F.fault_tail(wt, M)
                assert F.mismatch(bad[:, :M - M % 4], wt[:, :M - M % 4]) == 0
                if F.mismatch(bad, wt):
                    flagged(bad, wt, f"tail {what}")
                    acted["tail"] += 1
            # 16: a guard-band byte written (embedded), a byte left unwritten (dense)
            for t in (want, wt):
                before, where = F.place_u8(F.blank_u8(*t.shape), True)
                after = before.clone()
                G.window(after, where).copy_(t)
                F.assert_window_u8(after, before, where, t)
                for r, c in ((where[0] - 1, where[1]), (where[0] + t.shape[0], where[1] + t.shape[1] - 1),
                             (where[0], where[1] + t.shape[1]), (where[0] + t.shape[0] - 1, where[1] - 1)):
                    stray = after.clone()
                    stray[r, c] = 0x38
                    with pytest.raises(AssertionError):
                        F.assert_window_u8(stray, before, where, t, "guard band")
                bad = t.clone()
                bad[-1, -1] = F.SENTINEL_U8
                flagged(bad, t, "one byte left unwritten")
    n, tails = len(F.SHAPES_QUANT) * len(F.SHAPE_AMAX), sum(1 for M, _ in F.SHAPES_QUANT if M % 4) * len(F.SHAPE_AMAX)
    assert acted["other format"] == n and acted["amax 0"] == len(F.SHAPES_QUANT)
    assert acted["trunc"] >= n - 6 and acted["no saturation"] >= len(F.SHAPES_QUANT) and acted["scale after"] >= n // 2
    assert acted["away"] >= 8, acted          # ties are 0.4 % of the patterns: the larger shapes hold some
    assert acted["bytes"] >= n - 6 and acted["dwords"] >= n - 6 and acted["column"] >= n - 8 and acted["row"] >= n - 12
    assert acted["tail"] >= tails - 3, acted


def test_gemm_faults_are_flagged():
    """faults 11-14 on the F32 / STORE expectations of the dense set"""
    def differs(bad64, d):
        assert F.mismatch(bad64.to(f32), d.acc.to(f32)) > 0
        if d.want is not None:
            assert F.mismatch(G.round_bf16(bad64.to(f32).to(f64)), d.want) > 0
    n = {"scale_b": 0, "format": 0, "tail": 0, "split": 0}
    for layout, shapes in (("NT", F.SHAPES_GEMM_NT), ("TN", F.SHAPES_GEMM_TN)):
        for i, (M, N, K) in enumerate(shapes):
            for a_fmt in ((0, 1) if layout == "NT" else (1,)):
                d = F.dense_case(layout, M, N, K, a_fmt, i)
                prod = (lambda a, b: a.t() @ b) if layout == "TN" else (lambda a, b: a @ b.t())
                ksl = (lambda t, lo, hi: t[lo:hi]) if layout == "TN" else (lambda t, lo, hi: t[:, lo:hi])
                s = F.factor(d.sa, d.sb)
                if d.sb is not None:   # 11: scale_b dropped (cannot act where the pointer is NULL)
                    differs(d.acc / d.sb, d)
                    n["scale_b"] += 1
                # 12: A decoded in the other format
                differs(prod(F.decode(d.A, 1 - a_fmt), d.B64) * s, d)
                n["format"] += 1
                if K % 128 == 16 and K > 16:   # 13: the K tail of 16 ignored
                    differs(prod(ksl(d.A64, 0, K - 16), ksl(d.B64, 0, K - 16)) * s, d)
                    n["tail"] += 1
                tiles = -(-K // 128)
                if tiles >= 2:   # 14: the last non-empty split of 3 dropped
                    per = -(-tiles // 3)
                    last = (-(-tiles // per) - 1) * per * 128
                    differs(prod(ksl(d.A64, 0, last), ksl(d.B64, 0, last)) * s, d)
                    n["split"] += 1
    assert n["scale_b"] >= 20 and n["format"] == 52 and n["tail"] >= 12 and n["split"] >= 12, n
    for c in F.decode_cases():   # 12 on the decode set: the same bytes read in the other format, element by element
        a_side = "A side" in c.name
        vals = torch.nan_to_num(F.decode(c.A if a_side else c.B, 1 - (c.a_fmt if a_side else 0)), nan=0.0, posinf=0.0, neginf=0.0)
        # (the other operand is an identity: C is the byte matrix's values, transposed on the NT B side and the TN A side)
        bad = vals.t() if (c.layout == "NT") != a_side else vals
        assert bad.shape == c.want.shape
        assert F.mismatch((bad + 0.0).to(f32).contiguous(), c.want) >= 200, c.name
        moved = c.want.roll(1, 0 if c.want.shape[0] == 256 else 1)   # a decode that permutes the values
        assert F.mismatch(moved.contiguous(), c.want) >= 200, c.name


@pytest.mark.parametrize("efmt", [0, 1])
def test_emit_from_the_fp32_result_is_flagged(efmt):
    """fault 15: quantising the fp32 value instead of its bf16 rounding differs wherever rounding twice is not rounding
    once -- at a dyadic scale on every emit shape"""
    for M, N, K in F.SHAPES_EMIT:
        act32 = F.dgelu_case(M, N, K).want64.to(f32)   # (continuous values: acc gelu'(aux) with aux drawn from [-6, 6])
        stored = act32.to(bf16)
        for amax in (F.FMAX[efmt] / 256, float(stored.float().abs().max())):
            want, _ = F.quant_ref(stored, efmt, amax)
            scale, _ = F.scale_of(efmt, amax)
            bad = (act32 * scale).clamp(-F.FMAX[efmt], F.FMAX[efmt]).to(F.DTYPES[efmt]).view(u8)
            assert F.mismatch(bad, want) > 0, (M, N, K, amax)
            flagged(bad, want, "emit from fp32", embedded=True)


# ---- host-side refusals ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


P = 0x10000   # a non-null, 16-byte aligned address: every call below is refused before anything is launched or read
ERR_ARG, ERR_UNSUPPORTED = -1, -2
NT, NN, TN = _lib.VDS_NT, _lib.VDS_NN, _lib.VDS_TN
STORE, GELU, GATE, DGELU, F32 = (_lib.EPI_STORE, _lib.EPI_BIAS_GELU, _lib.EPI_GATE_RES, _lib.EPI_DGELU, _lib.EPI_F32)


def _args(layout, epi, M=64, N=64, K=64, A=P, lda=64, ldb=64, C_=P, ldc=64, C2=None, ldc2=0, aux=None, ldaux=0, gate=None,
          ldgate=0, rpb=0, split_k=1):
    return _lib.GemmArgs(layout, epi, M, N, K, A, lda, P, ldb, C_, ldc, C2, ldc2, None, aux, ldaux, gate, ldgate, rpb, split_k, None)


def _emit(q=P, ldq=64, qt=None, ldqt=0, amax_in=P, fmt=0):
    return _lib.Fp8Out(q, ldq, qt, ldqt, amax_in, None, None, fmt, None)


def test_gemm_fp8_refusals(lib):
    gate_ok = dict(C2=P, ldc2=64, aux=P, ldaux=64, gate=P, ldgate=64)
    cases = {   # name -> (args, a_fmt, b_fmt, emit, expected)
        # new: the leading dimensions the epilogues cannot address, as vds_gemm_bf16 refuses them
        "ldc % 8 (STORE)": (_args(NT, STORE, ldc=68), 0, 0, None, ERR_ARG),
        "ldc % 8 (STORE, a_fmt 1)": (_args(NT, STORE, ldc=60), 1, 0, None, ERR_ARG),
        "ldc % 8 (BIAS_GELU)": (_args(NT, GELU, ldc=65, C2=P, ldc2=64), 0, 0, None, ERR_ARG),
        "ldc2 % 8 (BIAS_GELU)": (_args(NT, GELU, C2=P, ldc2=68), 0, 0, None, ERR_ARG),
        "ldc2 % 8 (BIAS_GELU, C == NULL)": (_args(NT, GELU, C_=None, C2=P, ldc2=66), 0, 0, None, ERR_ARG),
        "ldc % 8 (GATE_RES)": (_args(NT, GATE, **{**gate_ok, "ldc": 68}), 0, 0, None, ERR_ARG),
        "ldc2 % 8 (GATE_RES)": (_args(NT, GATE, **{**gate_ok, "ldc2": 68}), 0, 0, None, ERR_ARG),
        "ldaux % 8 (GATE_RES)": (_args(NT, GATE, **{**gate_ok, "ldaux": 68}), 0, 0, None, ERR_ARG),
        "ldgate % 4 (GATE_RES)": (_args(NT, GATE, **{**gate_ok, "ldgate": 66}), 0, 0, None, ERR_ARG),
        "ldgate % 4 (GATE_RES, odd)": (_args(NT, GATE, **{**gate_ok, "ldgate": 577}), 0, 0, None, ERR_ARG),
        "ldc % 8 (DGELU)": (_args(NT, DGELU, ldc=68, aux=P, ldaux=64), 1, 0, None, ERR_ARG),
        "ldaux % 8 (DGELU)": (_args(NT, DGELU, aux=P, ldaux=68), 1, 0, None, ERR_ARG),
        "ldaux % 8 (DGELU, emit-only)": (_args(NT, DGELU, C_=None, aux=P, ldaux=68), 1, 0, _emit(fmt=1), ERR_ARG),
        "ldc % 4 (F32)": (_args(NT, F32, ldc=66), 0, 0, None, ERR_ARG),
        "ldc % 4 (F32, split)": (_args(NT, F32, ldc=65, split_k=3), 1, 0, None, ERR_ARG),
        "ldc % 4 (TN F32)": (_args(TN, F32, ldc=70, split_k=0), 1, 0, None, ERR_ARG),
        "GATE_RES without C2": (_args(NT, GATE, aux=P, ldaux=64, gate=P, ldgate=64), 0, 0, None, ERR_ARG),
        # what was validated before stays refused
        "null A": (_args(NT, STORE, A=None), 0, 0, None, ERR_ARG),
        "M == 0": (_args(NT, STORE, M=0), 0, 0, None, ERR_ARG),
        "K % 16": (_args(NT, STORE, K=72), 0, 0, None, ERR_ARG),
        "lda % 16": (_args(NT, STORE, lda=72), 0, 0, None, ERR_ARG),
        "ldb % 16": (_args(NT, STORE, ldb=72), 0, 0, None, ERR_ARG),
        "N % 8": (_args(NT, STORE, N=60), 0, 0, None, ERR_ARG),
        "layout NN": (_args(NN, STORE), 0, 0, None, ERR_UNSUPPORTED),
        "b_fmt != 0": (_args(NT, STORE), 0, 1, None, ERR_UNSUPPORTED),
        "a_fmt 2": (_args(NT, STORE), 2, 0, None, ERR_UNSUPPORTED),
        "TN with a bf16 epilogue": (_args(TN, STORE), 1, 0, None, ERR_UNSUPPORTED),
        "TN with a_fmt 0": (_args(TN, F32), 0, 0, None, ERR_UNSUPPORTED),
        "TN with M % 16": (_args(TN, F32, M=72), 1, 0, None, ERR_UNSUPPORTED),
        "TN with emit": (_args(TN, F32), 1, 0, _emit(), ERR_UNSUPPORTED),
        "emit with STORE": (_args(NT, STORE), 0, 0, _emit(), ERR_ARG),
        "emit with GATE_RES": (_args(NT, GATE, **gate_ok), 0, 0, _emit(), ERR_ARG),
        "emit ldq % 8": (_args(NT, GELU, C2=P, ldc2=64), 0, 0, _emit(ldq=68), ERR_ARG),
        "emit ldqt % 4": (_args(NT, GELU, C2=P, ldc2=64), 0, 0, _emit(qt=P, ldqt=66), ERR_ARG),
        "emit fmt 2": (_args(NT, GELU, C2=P, ldc2=64), 0, 0, _emit(fmt=2), ERR_ARG),
        "emit without amax_in": (_args(NT, DGELU, aux=P, ldaux=64), 1, 0, _emit(amax_in=None, fmt=1), ERR_ARG),
        "split-K outside F32": (_args(NT, STORE, split_k=2), 0, 0, None, ERR_ARG),
        "C == NULL (STORE)": (_args(NT, STORE, C_=None), 0, 0, None, ERR_ARG),
        "C == NULL (DGELU without emit)": (_args(NT, DGELU, C_=None, aux=P, ldaux=64), 1, 0, None, ERR_ARG),
        "C == NULL and C2 == NULL (BIAS_GELU)": (_args(NT, GELU, C_=None), 0, 0, None, ERR_ARG),
        "C == NULL and C2 == NULL (BIAS_GELU, emit)": (_args(NT, GELU, C_=None), 0, 0, _emit(), ERR_ARG),
    }
    for what, (a, a_fmt, b_fmt, emit, want) in cases.items():
        rc = lib.vds_gemm_fp8(C.byref(a), None, None, a_fmt, b_fmt, C.byref(emit) if emit is not None else None, None)
        assert rc == want, (what, rc)


def test_quantiser_refusals(lib):
    q = lib.vds_quant_fp8
    ok = dict(x=P, ldx=64, M=4, K=64, fmt=0, amax=P, q=P, ldq=64, qt=P, ldt=4)

    def quant(**kw):
        a = {**ok, **kw}
        return q(a["x"], a["ldx"], a["M"], a["K"], a["fmt"], a["amax"], a["q"], a["ldq"], a["qt"], a["ldt"], None, None, None)
    for what, kw in {"null x": dict(x=None), "null amax": dict(amax=None), "no output": dict(q=None, qt=None), "M == 0": dict(M=0),
                     "K == 0": dict(K=0), "K % 8": dict(K=60), "ldx % 8": dict(ldx=68), "fmt 2": dict(fmt=2), "fmt -1": dict(fmt=-1),
                     "ldq % 8": dict(ldq=68), "ldt % 4": dict(ldt=6), "ldt % 4 (qt alone)": dict(q=None, ldt=5)}.items():
        assert quant(**kw) == ERR_ARG, what
    for what, a in {"null x": (None, 64, 4, 64, P), "null amax": (P, 64, 4, 64, None), "M == 0": (P, 64, 0, 64, P),
                    "K == 0": (P, 64, 4, 0, P), "K % 8": (P, 64, 4, 60, P), "ldx % 8": (P, 68, 4, 64, P)}.items():
        assert lib.vds_absmax(*a, None) == ERR_ARG, what
    for what, a in {"null q": (None, 64, 4, 64, P, 4), "null qt": (P, 64, 4, 64, None, 4), "M == 0": (P, 64, 0, 64, P, 4),
                    "K == 0": (P, 64, 4, 0, P, 4), "K % 16": (P, 64, 4, 56, P, 4), "ldq % 16": (P, 72, 4, 64, P, 4),
                    "ldt % 4": (P, 64, 4, 64, P, 6)}.items():
        assert lib.vds_transpose_fp8(*a, None) == ERR_ARG, what
