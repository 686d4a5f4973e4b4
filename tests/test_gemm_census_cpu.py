"""The exact GEMM census without a GPU (tests/helpers/gemm_census.py): the helper's expectations equal a plain float64
matmul formula, the exactness conditions that make a zero-tolerance comparison legitimate hold for every listed case,
the shape lists cover every tiling's edges, assert_window flags every emulated kernel fault, and vds_gemm_bf16 refuses
leading dimensions its 16-byte accesses cannot address (host-side checks: nothing is launched)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_census as G  # noqa: E402

from video_diffusion_speedrun_amd import _lib  # noqa: E402

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
ALL = [(layout, s) for layout in ("NT", "NN", "TN") for s in G.SHAPES[layout]]
IDS = [f"{layout}-{s[0]}x{s[1]}x{s[2]}" for layout, s in ALL]


# ---- coverage of the shape lists ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiling", G.TILINGS, ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
def test_shape_lists_cover_every_tiling(layout, tiling):
    missing = [name for name, ok in G.coverage(layout, tiling).items() if not ok]
    assert not missing, (layout, tiling, missing)


def test_shape_lists_are_small_and_legal():
    for layout, (M, N, K) in ALL:
        assert M <= 520 and N <= 392 and K <= 328 and N % 8 == 0
        assert (M % 8 == 0) if layout == "TN" else (K % 8 == 0)
    for layout in G.SHAPES:
        assert len(set(G.SHAPES[layout])) == len(G.SHAPES[layout]) <= 30
    g = G.GROUPED
    L = g["lead"] + g["period"] * g["S"]
    assert L == G.ROWS_PER_BATCH == 73 and L % 64 != 0
    assert all(M == g["B"] * L and N % 8 == 0 and K % 8 == 0 for M, N, K in G.SHAPES_GROUPED)
    assert any(M > G.ROWS_PER_BATCH for M, _, _ in G.SHAPES_NT)


# ---- expectations against a plain float64 formula, and the exactness conditions ---------------------------------------
@pytest.mark.parametrize("layout,shape", ALL, ids=IDS)
def test_dense_expectations_and_exactness(layout, shape):
    M, N, K = shape
    d = G.dense_case(layout, M, N, K)   # asserts |sum| < 2^24 and the share above 256 itself
    A, B = d.A.double(), d.B.double()
    ref = A @ B.t() if layout == "NT" else A @ B if layout == "NN" else A.t() @ B
    assert ref.shape == (M, N) and torch.equal(d.acc, ref)
    # integers below 2^24 in EVERY partial sum: |partial| <= sum_k |a| |b|
    l1 = G.matmul64(layout, A.abs(), B.abs())
    assert float(l1.max()) + 64 < 2 ** 24 and torch.equal(d.acc, d.acc.round())
    assert torch.equal(d.acc.float().double(), d.acc)   # the fp32 output of TN is this number
    if layout == "TN":
        return
    assert torch.equal(d.want, ref.float().to(bf16)) and torch.equal(d.want_bias, (ref + d.bias.double()).float().to(bf16))
    inexact = d.want_bias.double() != ref + d.bias.double()
    mag = (ref + d.bias.double()).abs()
    tie = (mag > 256) & (mag < 512) & (mag % 2 == 1)
    assert inexact.any()
    if M * N >= 1024:
        assert tie.any(), "no rounding tie among the results"   # odd integers in (256, 512) lie halfway
    # GATE_RES at the rows_per_batch values the GPU test uses
    for rpb, with_bias in ((G.ROWS_PER_BATCH, True), (G.ROWS_PER_BATCH, False), (128, True)):
        rows = G.gate_rows_plain(M, rpb)
        gr = G.gate_res_case(d, rows, -(-M // rpb), with_bias)
        y = ref + (d.bias.double() if with_bias else 0.0)
        x_new = gr.aux.double() + y * gr.gate.double().repeat_interleave(rpb, dim=0)[:M]
        assert torch.equal(x_new.float().double(), x_new) and torch.equal((y * 2).round(), y * 2)
        assert torch.equal(gr.y, y.float().to(bf16)) and torch.equal(gr.x_new, x_new.float().to(bf16))
        assert set(gr.gate.flatten().tolist()) <= set(G.GATES)


@pytest.mark.parametrize("shape", G.SHAPES_GROUPED, ids=lambda s: "x".join(map(str, s)))
def test_grouped_gate_rows_follow_mod_group_of(shape):
    from video_diffusion_speedrun_amd.ops import mod_group_of
    M, N, K = shape
    g = G.GROUPED
    L = g["lead"] + g["period"] * g["S"]
    rows = G.gate_rows_grouped(M, L, g["lead"], g["period"])
    for r in (0, 15, 16, 17, 18, 19, 72, 73, 89, 90, M - 1):
        assert rows[r] == (r // L) * (1 + g["period"]) + mod_group_of(r % L, g["lead"], g["period"])
    assert rows.max() == g["B"] * (1 + g["period"]) - 1 and len(set(rows.tolist())) == g["B"] * (1 + g["period"])
    d = G.dense_case("NT", M, N, K)
    gr = G.gate_res_case(d, rows, g["B"] * (1 + g["period"]))
    table = gr.gate.double()[rows]   # the expanded [M, N] gate table of a rows_per_batch = 1 launch
    x_new = gr.aux.double() + (d.acc + d.bias.double()) * table
    assert torch.equal(gr.x_new, x_new.float().to(bf16))


@pytest.mark.parametrize("shape", G.SHAPES_NT, ids=lambda s: "x".join(map(str, s)))
def test_sparse_expectations_and_exactness(shape):
    M, N, K = shape
    s = G.sparse_case(M, N, K)      # asserts |pre| < 6 and pre exactly bf16 itself
    pre = s.A.double() @ s.B.double().t() + s.bias.double()
    assert torch.equal(s.pre64, pre) and torch.equal(s.pre.double(), pre) and float(pre.abs().max()) < 6
    assert torch.equal((pre * 16).round(), pre * 16)   # multiples of 1/16 below 6: 7 significant bits at the most
    assert set(s.A.flatten().tolist()) <= {-1.0, 0.0, 1.0} and float((s.B.double() * 16).abs().max()) <= 2
    assert float(s.bias.double().abs().max()) <= 0.5
    assert torch.allclose(s.act64, torch.nn.functional.gelu(pre), rtol=0, atol=1e-12)
    dg = G.dgelu_case(M, N, K)
    acc = dg.A.double() @ dg.B.double()
    assert torch.equal(dg.acc, acc) and float(dg.aux.double().abs().max()) <= 6.0
    x = dg.aux.double().requires_grad_(True)
    torch.nn.functional.gelu(x).backward(acc)
    assert torch.allclose(dg.want64, x.grad, rtol=0, atol=1e-10 * max(1.0, float(acc.abs().max())))


def test_sparse_set_is_exact_up_to_k_328():
    """the property the sparse set is chosen for, at the largest contraction the lists use, whatever the shape"""
    s = G.sparse_case(520, 392, 328)
    assert float(s.pre64.abs().max()) < 6 and torch.equal(s.pre.double(), s.pre64)


# ---- windows -----------------------------------------------------------------------------------------------------------
def test_embed_and_assert_window():
    t = torch.arange(6 * 16, dtype=f32).reshape(6, 16).to(bf16)
    parent, view = G.embed(t, pad_rows=2, pad_cols=24, col0=16, fill="nan")
    assert parent.shape == (10, 40) and G.locate(parent, view) == (2, 16, 6, 16)
    assert view.stride(0) == 40 and view.data_ptr() % 16 == 0 and torch.equal(view, t)
    outside = torch.ones_like(parent, dtype=torch.bool)
    outside[2:8, 16:32] = False
    assert torch.isnan(parent[outside].float()).all()
    out, oview = G.embed(torch.zeros(6, 16, dtype=bf16), fill="sentinel")
    assert (out.view(torch.int16)[0] == G.SENTINEL_BF16).all() and not torch.isnan(out.float()).any()
    after = out.clone()
    G.window(after, G.locate(out, oview)).copy_(t)
    G.assert_window(after, out, oview, t)
    o32, v32 = G.embed(torch.zeros(8, 8, dtype=f32), fill="sentinel")
    assert (o32.view(torch.int32)[0] == G.SENTINEL_F32).all()
    # -0.0 against 0.0 and one NaN payload against another are different bits
    z = torch.zeros(6, 16, dtype=bf16)
    after = out.clone()
    with pytest.raises(AssertionError):
        G.assert_window(after, out, oview, -z)


# ---- sensitivity: every emulated fault must be flagged ----------------------------------------------------------------
def _flagged(after, before, where, want, what):
    try:
        G.assert_window(after, before, where, want, what)
    except AssertionError:
        return
    raise AssertionError(f"assert_window did not flag: {what}")


def _with_window(before, where, values):
    after = before.clone()
    G.window(after, where).copy_(values)
    return after


@pytest.mark.parametrize("layout,shape", ALL, ids=IDS)
def test_sensitivity_every_emulated_fault_is_flagged(layout, shape):
    M, N, K = shape
    d = G.dense_case(layout, M, N, K)
    A, B, bias = d.A.double(), d.B.double(), d.bias.double()
    tn = layout == "TN"
    exact = d.acc if tn else d.acc + bias                 # what the kernel holds before its store
    store = (lambda t: t.float()) if tn else (lambda t: t.float().to(bf16))
    want = store(exact)
    before, view = G.embed(torch.zeros_like(want), fill="sentinel")
    where = G.locate(before, view)
    r0, c0 = where[:2]
    G.assert_window(_with_window(before, where, want), before, where, want, "the correct result")
    tag = f"{layout} {M}x{N}x{K}: "
    row = M // 2

    # one 8-wide k chunk dropped for one row
    k0 = (K // 8 // 2) * 8
    A2 = A.clone()
    if tn:
        A2[k0:k0 + 8, row] = 0
    else:
        A2[row, k0:k0 + 8] = 0
    bad = G.matmul64(layout, A2, B) + (0 if tn else bias)
    _flagged(_with_window(before, where, store(bad)), before, where, want, tag + "k chunk dropped for one row")

    # a K tail taken from the NaN gap: the chunk after the last one of the contraction, read from A's parent
    if tn:   # k-major: the row after the last token is a guard row of the parent
        pa, va = G.embed(d.A, fill="nan")
        ra, ca = G.locate(pa, va)[:2]
        A_ext = pa[ra:ra + K + 1, ca:ca + M].double()
        B_ext = torch.cat([B, torch.ones(1, N, dtype=f64)])
    else:    # k-contiguous: the 8 elements after the row's K inside lda
        pa, va = G.embed(d.A, fill="nan")
        ra, ca = G.locate(pa, va)[:2]
        A_ext = pa[ra:ra + M, ca:ca + K + 8].double()
        ones = torch.ones(N, 8, dtype=f64) if layout == "NT" else torch.ones(8, N, dtype=f64)
        B_ext = torch.cat([B, ones], dim=1 if layout == "NT" else 0)
    bad = G.matmul64(layout, A_ext, B_ext) + (0 if tn else bias)
    assert torch.isnan(bad).all()
    _flagged(_with_window(before, where, store(bad)), before, where, want, tag + "K tail from the NaN gap")

    # one output row shifted by one
    if M >= 2:
        bad = want.clone()
        src = row + 1 if row + 1 < M else row - 1
        bad[row] = want[src]
        _flagged(_with_window(before, where, bad), before, where, want, tag + "one output row shifted by one")

    # bias omitted in one 8-column chunk of the last tile column
    if not tn:
        bad = want.clone()
        bad[:, N - 8:] = store(d.acc[:, N - 8:])
        _flagged(_with_window(before, where, bad), before, where, want, tag + "bias omitted in one 8-column chunk")

    # one element left unwritten / written one row past M / written one column chunk past N
    bad = want.clone()
    bad[M - 1, N - 1] = G.fill_value(want.dtype, "sentinel")
    _flagged(_with_window(before, where, bad), before, where, want, tag + "one element left unwritten")
    after = _with_window(before, where, want)
    after[r0 + M, c0 + N - 1] = want[M - 1, N - 1]
    _flagged(after, before, where, want, tag + "one element written one row past M")
    after = _with_window(before, where, want)
    after[r0, c0 + N] = want[0, N - 1]
    _flagged(after, before, where, want, tag + "one element written one column chunk past N")

    if tn:
        return
    # a truncating bf16 conversion instead of round-to-nearest-even
    _flagged(_with_window(before, where, G.trunc_bf16(exact)), before, where, want, tag + "truncating bf16 conversion")

    # the gate row of the neighbouring sample used for one row (GATE_RES, rows_per_batch = 73)
    nb = -(-M // G.ROWS_PER_BATCH)
    if nb >= 2:
        rows = G.gate_rows_plain(M, G.ROWS_PER_BATCH)
        gr = G.gate_res_case(d, rows, nb)
        other = int(rows[row]) + (1 if int(rows[row]) + 1 < nb else -1)
        bad = gr.x_new.clone()
        bad[row] = G.round_bf16(gr.aux[row].double() + exact[row] * gr.gate[other].double())
        _flagged(_with_window(before, where, bad), before, where, gr.x_new, tag + "gate row of the neighbouring sample")


@pytest.mark.parametrize("shape", G.SHAPES_GROUPED, ids=lambda s: "x".join(map(str, s)))
def test_sensitivity_gate_row_of_the_neighbouring_group(shape):
    M, N, K = shape
    g = G.GROUPED
    L = g["lead"] + g["period"] * g["S"]
    rows = G.gate_rows_grouped(M, L, g["lead"], g["period"])
    d = G.dense_case("NT", M, N, K)
    gr = G.gate_res_case(d, rows, g["B"] * (1 + g["period"]))
    before, view = G.embed(torch.zeros_like(gr.x_new), fill="sentinel")
    where = G.locate(before, view)
    for row in (0, 16, 17, M - 1):   # a lead row, the first rows of two frame groups, the last row
        other = int(rows[row]) + (1 if row != M - 1 else -1)
        bad = gr.x_new.clone()
        bad[row] = G.round_bf16(gr.aux[row].double() + (d.acc[row] + d.bias.double()) * gr.gate[other].double())
        _flagged(_with_window(before, where, bad), before, where, gr.x_new, f"grouped {shape}: neighbouring group, row {row}")


def test_sensitivity_bias_omitted_in_the_gelu_epilogue():
    """the sparse set: a bias chunk skipped in the last tile column changes `pre` bit for bit"""
    for M, N, K in G.SHAPES_NT:
        s = G.sparse_case(M, N, K)
        before, view = G.embed(torch.zeros_like(s.pre), fill="sentinel")
        where = G.locate(before, view)
        bad = s.pre.clone()
        bad[:, N - 8:] = (s.pre64 - s.bias.double())[:, N - 8:].float().to(bf16)
        if float(s.bias[N - 8:].double().abs().max()) == 0:
            continue   # not expressible: the chunk's bias is zero
        _flagged(_with_window(before, where, bad), before, where, s.pre, f"sparse {M}x{N}x{K}: bias chunk omitted")


# ---- host-side refusals -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


P = 0x10000   # a non-null, 16-byte aligned address: every call below is refused before anything is launched or read


def _args(layout, epi, M=64, N=64, K=64, lda=64, ldb=64, C_=P, ldc=64, C2=None, ldc2=0, aux=None, ldaux=0, gate=None,
          ldgate=0, rpb=0, split_k=1):
    return _lib.GemmArgs(layout, epi, M, N, K, P, lda, P, ldb, C_, ldc, C2, ldc2, None, aux, ldaux, gate, ldgate, rpb,
                         split_k, None)


def test_gemm_refuses_leading_dimensions_it_cannot_address(lib):
    NT, NN, TN = _lib.VDS_NT, _lib.VDS_NN, _lib.VDS_TN
    STORE, GELU, GATE, DGELU, F32 = (_lib.EPI_STORE, _lib.EPI_BIAS_GELU, _lib.EPI_GATE_RES, _lib.EPI_DGELU, _lib.EPI_F32)
    ERR_ARG = -1
    gate_ok = dict(C2=P, ldc2=64, aux=P, ldaux=64, gate=P, ldgate=64)
    bad = {
        "ldc % 8 (STORE)": _args(NT, STORE, ldc=68),
        "ldc % 8 (NN STORE)": _args(NN, STORE, ldc=60),
        "ldc % 8 (BIAS_GELU)": _args(NT, GELU, ldc=65, C2=P, ldc2=64),
        "ldc2 % 8 (BIAS_GELU)": _args(NT, GELU, C2=P, ldc2=68),
        "ldc2 % 8 (BIAS_GELU, C == NULL)": _args(NT, GELU, C_=None, C2=P, ldc2=66),
        "ldc % 8 (GATE_RES)": _args(NT, GATE, **{**gate_ok, "ldc": 68}),
        "ldc2 % 8 (GATE_RES)": _args(NT, GATE, **{**gate_ok, "ldc2": 68}),
        "ldaux % 8 (GATE_RES)": _args(NT, GATE, **{**gate_ok, "ldaux": 68}),
        "ldgate % 4 (GATE_RES)": _args(NT, GATE, **{**gate_ok, "ldgate": 66}),
        "ldgate % 4 (GATE_RES, odd)": _args(NT, GATE, **{**gate_ok, "ldgate": 577}),
        "ldc % 8 (DGELU)": _args(NN, DGELU, ldc=68, aux=P, ldaux=64),
        "ldaux % 8 (DGELU)": _args(NN, DGELU, aux=P, ldaux=68),
        "ldc % 4 (F32)": _args(TN, F32, ldc=66),
        "ldc % 4 (F32, split)": _args(TN, F32, ldc=65, split_k=3),
        "ldc % 4 (F32, auto)": _args(TN, F32, ldc=70, split_k=0),
        # what was validated before stays refused
        "null A": _lib.GemmArgs(NT, STORE, 64, 64, 64, None, 64, P, 64, P, 64),
        "M == 0": _args(NT, STORE, M=0),
        "N % 8": _args(NT, STORE, N=60),
        "lda % 8": _args(NT, STORE, lda=68),
        "ldb % 8": _args(NT, STORE, ldb=68),
        "K % 8 (NT)": _args(NT, STORE, K=60),
        "K % 8 (NN)": _args(NN, STORE, K=60),
        "M % 8 (TN)": _args(TN, F32, M=60),
        "layout": _args(3, STORE),
        "split-K outside TN + F32": _args(NT, STORE, split_k=2),
        "C == NULL (STORE)": _args(NT, STORE, C_=None),
        "C == NULL and C2 == NULL": _args(NT, GELU, C_=None),
    }
    for what, a in bad.items():
        assert lib.vds_gemm_bf16(C.byref(a), None) == ERR_ARG, what
    # the grouped entry point runs the same checks
    grp = _lib.ModGroups(16, 3)
    for what in ("ldc2 % 8 (GATE_RES)", "ldaux % 8 (GATE_RES)", "ldgate % 4 (GATE_RES)"):
        a = bad[what]
        a.M, a.rows_per_batch = 146, 73
        assert lib.vds_gemm_bf16_grouped(C.byref(a), C.byref(grp), None) == ERR_ARG, what
