"""The row census without a GPU: its conditions, its coverage and its sensitivity.

tests/helpers/row_census.py builds inputs whose right answer is one bit pattern per element.  Here:
  * every builder's assertions hold for every case the GPU test launches (all dyadic elements decided, sums within 24
    bits, the undecided share of the generic rows under the cap, the sentinel no value of any case);
  * the dispatch predicates restated in the helper are those of csrc/elementwise.hip, and the shape lists leave no branch
    without a case: reverting any one branch to a neighbouring instance leaves at least one case on the abandoned branch;
  * a plain torch fp32 restatement of each operation passes the census as it stands and fails it with each injected fault;
    the faults marked (norm passes) are accepted by close() of tests/test_kernels_gpu.py at that file's tolerance on that
    file's Gaussian inputs -- what the relative Frobenius norm cannot see."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_census as G  # noqa: E402
import row_census as R  # noqa: E402

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video_diffusion_speedrun_amd", "csrc",
                   "elementwise.hip")


# ---- the builders' assertions --------------------------------------------------------------------------------------------
def test_forward_cases_are_decided():
    for D in R.FWD_D:
        for B, L in R.FWD_BL:
            for with_w in (False, True):
                c = R.fwd_case(B, L, D, with_w)       # raises on an undecided element or a sentinel value
                assert not c.und.any() and c.want_y.shape == (B * L, D)
    c = R.fwd_case(3, 21, 384, True)
    # the recipe the issue warns of: shifts that can cancel x^ w (1 + scale) leave elements undecided
    small = c.shift.sign() * (c.shift.abs() / 16.0)
    _, und = R.decide(R.fwd_expect(c.x.to(f64), c.w.to(f64), c.s1, small, 21)[0])
    assert und.any(), "shifts of 0, +-1, +-2, +-3 must leave cancellations undecided"


@pytest.mark.parametrize("D", R.BWD_D)
def test_backward_cases_are_decided(D):
    shares = []
    for B, L, _, with_w, with_dres in R.bwd_plan(D):
        c = R.bwd_case(B, L, D, with_w, with_dres, "dyadic")
        assert not c.und.any() and c.share == 0.0
        if (B, L) in R.BWD_GENERIC_BL:
            assert not R.bwd_case(B, L, D, with_w, True, "const").und.any()
            g = R.bwd_case(B, L, D, with_w, with_dres, "generic")
            assert g.share <= R.UNDECIDED_CAP
            shares.append(g.share)
        R.gate_case(B, L, D)
    print(f"generic rows D {D}: undecided share {min(shares):.2%} .. {max(shares):.2%}")


def test_other_cases_build():
    B, L, D = R.BWD_FLOOR32
    for with_w in (False, True):
        R.bwd_case(B, L, D, with_w, True, "dyadic")
    R.gate_case(B, L, D)
    for M, N in [(M, N) for M in R.COLSUM_M for N in R.COLSUM_N] + [R.COLSUM_BIG]:
        for rps, roff in R.COLSUM_ROWS:
            R.colsum_case(M, N, rps, roff)
    for hd, hdp, H in R.QKV_FWD_TILE + R.QKV_FWD_ELEM:
        for B, L in R.QKV_BL:
            for v0 in (False, True):
                R.qkv_fwd_case(B, L, H, hd, hdp, v0)
    for hd, hdp, H, _ in R.QKV_BWD:
        for B, L in R.QKV_BWD_BL:
            for mix, add in R.QKV_BWD_MODES:
                R.qkv_bwd_case(B, L, H, hd, hdp, mix, add)
    for hd in R.ROPE_APPLY_HD:
        for inv in (0, 1):
            R.rope_apply_case(2, 3, R.ROPE_APPLY_L, hd, inv)


def test_builders_raise():
    """the assertions are live: a sum past 24 bits, a non-dyadic term and a sentinel value are refused"""
    with pytest.raises(AssertionError):
        R.exact_sum("x", torch.full((1 << 19, 1), 33.0, dtype=f64), 0, torch.zeros(1, dtype=f64))
    with pytest.raises(AssertionError):
        R.exact_sum("x", torch.full((4, 1), 1.0 / 3.0, dtype=f64), 0, torch.zeros(1, dtype=f64))
    with pytest.raises(AssertionError):
        R.assert_no_sentinel("x", G.fill_value(bf16, "sentinel").repeat(2))
    with pytest.raises(AssertionError):
        R.assert_decided("x", torch.tensor([False, True]))
    # 1 + 2^-8 is the tie between two bf16 numbers: moved either way it rounds differently
    _, und = R.decide([torch.tensor([1.0 + 2.0 ** -8], dtype=f64) * (1.0 + s * R.REL) for s in (0.0, -1.0, 1.0)])
    assert und.all()


# ---- coverage ----------------------------------------------------------------------------------------------------------
def test_coverage():
    missing = [k for k, v in R.coverage().items() if not v]
    assert not missing, missing


def test_predicates_are_the_source():
    """the literal conditions of elementwise.hip that the helper restates (a change there must be restated here)"""
    src = open(SRC).read()
    for text in ("const int nc_ = ((D) / 8 + 63) / 64;",
                 "if (D != 384 && D != 768 && D != 1152) return false;",
                 "const int floor_rows = (min_rows == 8 && total >= 8192) ? 32 : min_rows;",
                 "vdscfg::geti(vdscfg::EW_WGS) : 768;",
                 "if (tile > 0 && H * hd <= 2048 && H <= 256 && L >= 8",
                 "return on && (hdp & 7) == 0 && (hd & 7) == 0 && H * hd <= 2048;",
                 "if (((hdp - hd) >> 2) > (hd >> 3)) return VDS_ERR_UNSUPPORTED;",
                 "const int rpb = M > 8192 ? (M + 127) / 128 : 64;",
                 "if (D <= 512) ROPE_BWD(1);", "else if (D <= 1024) ROPE_BWD(2);", "else if (D <= 1536) ROPE_BWD(3);"):
        assert text in src, text
    for hd, hdp in R.TILE_INSTANCES:
        assert f"if (hd == {hd} && hdp == {hdp}) ROPE_TILE_T({hd}, {hdp});" in src
    assert src.count(") ROPE_TILE_T(") == len(R.TILE_INSTANCES)   # no instance the list does not know
    # the examples of the issue
    assert [R.rows_per_block(L, B) for L, B in ((75, 3), (4096, 2), (4100, 2), (20000, 2))] == [8, 32, 32, 53]
    assert R.rows_per_block(37, 3, wgs=2) == 56 and R.rows_per_block(37, 3, min_rows=1) == 1
    assert [R.nc_of(D) for D in (8, 512, 520, 1024, 1032, 1536, 1544, 2048, 2056)] == [1, 1, 2, 2, 3, 3, 4, 4, 5]
    assert [R.qkv_bwd_form(H, hd, hdp) for hd, hdp, H, _ in R.QKV_BWD[:4]] == ["tok<1>", "tok<2>", "tok<3>", "tok<4>"]


# ---- sensitivity: fp32 restatements with injected faults -----------------------------------------------------------------
def rel(a, b):
    """the norm check of tests/test_kernels_gpu.py"""
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def gauss(*shape, seed, scale=1.0, dtype=bf16):
    """gen() of tests/test_kernels_gpu.py"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def rms_fwd32(x, w, shift, scale, L, eps, fault=None, at=None):
    """vds_rmsnorm_mod_fwd in torch fp32 -> (y bf16, rstd f32); shift / scale [B, D] f32"""
    xf = x.float()
    rows, D = xf.shape
    b = torch.arange(rows) // L
    r = torch.rsqrt((xf * xf).sum(1) / D + (0.0 if fault == "eps dropped" else eps))
    first = torch.arange(L, rows, L)                     # the first row of every sample but the first
    if fault == "rstd of the previous row":
        r[first] = r[first - 1]
    if fault == "modulation row of sample b - 1":
        b[first] -= 1
    y = xf * r[:, None]
    if w is not None:
        y = y * w.float()
    y = (y * (1.0 + scale[b]) + shift[b]).to(bf16)
    if fault == "element of the neighbouring row":
        y[at[0], at[1]] = y[at[0] - 1, at[1]]
    return y, r


def census_fwd(c, fault=None, at=None):
    """does the restatement pass the census of case c?"""
    D = c.D
    y, r = rms_fwd32(c.x, c.w, c.mod[:, :D], c.mod[:, 2 * D:3 * D], c.L, R.EPS, fault, at)
    return torch.equal(G.bits(y), G.bits(c.want_y)) and R.ulps32(r, c.r64) <= 4.0


def test_forward_faults():
    c = R.fwd_case(3, 21, 384, True)
    assert census_fwd(c)
    diff = (G.bits(c.want_y[1]) != G.bits(c.want_y[0])).nonzero()
    at = (1, int(diff[0]))
    for fault in ("element of the neighbouring row", "eps dropped", "rstd of the previous row",
                  "modulation row of sample b - 1"):
        assert not census_fwd(c, fault, at), fault
    # (norm passes): the inputs, the reference and the tolerance of test_rmsnorm_mod_fwd_bwd
    B, L, D = 3, 75, 384
    x = gauss(B * L, D, seed=50)
    w = (1 + 0.1 * gauss(D, seed=51, dtype=f32)).to(bf16)
    mod = gauss(B, 9 * D, seed=52, dtype=f32) * 0.5
    shift, scale = mod[:, 3 * D:4 * D], mod[:, 4 * D:5 * D]
    b = torch.arange(B * L) // L
    xd = x.double()
    ref = xd / torch.sqrt((xd * xd).mean(1, keepdim=True) + 1e-6) * w.double() * (1 + scale[b].double()) + shift[b].double()
    good, _ = rms_fwd32(x, w, shift, scale, L, R.EPS)
    d = (good[1].float() - good[0].float()).abs()
    at = (1, int(((d > 0.5) & (d < 1.0)).nonzero()[0]))   # an error of the size of a typical element
    for fault in ("element of the neighbouring row", "eps dropped"):
        y, _ = rms_fwd32(x, w, shift, scale, L, R.EPS, fault, at)
        assert not torch.equal(G.bits(y), G.bits(good)) or fault == "eps dropped"
        e = rel(y, ref)
        print(f"{fault}: relative Frobenius error {e:.2e} (the norm check accepts < 4e-3)")
        assert e < 4e-3, (fault, e)


def rms_bwd32(c, fault=None):
    """vds_rmsnorm_mod_bwd in torch fp32 on a census case -> (dx window bf16, dmod f32 [B, 4 D], dw)"""
    B, L, D = c.B, c.L, c.D
    b = torch.arange(B * L) // L
    x, dy, rstd = c.x.float(), c.dy.float(), c.rstd
    s1 = 1.0 + c.mod[:, 2 * D:3 * D]
    xhat = x * rstd[:, None]
    t = dy * s1[b]
    g = t * c.w.float() if c.w is not None else t
    dot = (g * xhat).sum(1) / D
    dx = rstd[:, None] * (g - xhat * dot[:, None])
    if c.dres is not None:
        dx = c.dres.float() + dx
    out = G.fill_value(bf16, "sentinel").repeat(B * L, D)      # the output window as the census hands it over
    rows = B * L - 1 if fault == "last row of a ragged block unwritten" else B * L
    out[:rows] = dx.to(bf16)[:rows]
    dmod = c.dmod0.clone()
    d_shift = dy.view(B, L, D).sum(1)
    d_scale = (dy * xhat * (c.w.float() if c.w is not None else 1.0)).view(B, L, D).sum(1)
    if fault == "a column chunk of d(scale) into d(shift)":
        d_shift[:, 8:16] += d_scale[:, 8:16]
        d_scale[:, 8:16] = 0.0
    dmod[:, :D] += d_shift
    dmod[:, 2 * D:3 * D] += d_scale
    dw = c.dw0 + (t * xhat).sum(0) if c.w is not None else None
    return out, dmod, dw


def census_bwd(c, fault=None):
    dx, dmod, dw = rms_bwd32(c, fault)
    ok = torch.equal(G.bits(dx), G.bits(c.want_dx)) and torch.equal(G.bits(dmod), G.bits(c.want_dmod))
    return ok and (dw is None or torch.equal(G.bits(dw), G.bits(c.want_dw)))


def test_backward_faults():
    for kind in ("dyadic", "const"):
        for with_w in (False, True):
            c = R.bwd_case(3, 21, 144, with_w, True, kind)
            assert census_bwd(c), (kind, with_w)
            for fault in ("last row of a ragged block unwritten", "a column chunk of d(scale) into d(shift)"):
                assert not census_bwd(c, fault), (kind, with_w, fault)
    # the unwritten row shows through the sentinel alone: over a buffer that already holds the answer it is invisible
    c = R.bwd_case(3, 21, 144, False, True, "dyadic")
    dx, _, _ = rms_bwd32(c, "last row of a ragged block unwritten")
    assert (G.bits(dx[-1]) == G.SENTINEL_BF16).all() and torch.equal(G.bits(dx[:-1]), G.bits(c.want_dx[:-1]))
    # generic rows: the restatement stays within the census's tolerance, a wrong mean does not
    g = R.bwd_case(3, 21, 144, True, True, "generic")
    dx, _, _ = rms_bwd32(g)
    R.check_dx(dx, g)
    with pytest.raises(AssertionError):
        R.check_dx((dx.float() * (1.0 + 2.0 ** -6)).to(bf16), g)


def qkv_fwd32(c, fault=None):
    """vds_qkv_rope_fwd in torch fp32 -> (q, k, v) bf16 [B, H, L, hdp]"""
    B, L, H, hd, hdp = c.B, c.L, c.H, c.hd, c.hdp
    D = H * hd
    cos, sin = c.cos.clone(), c.sin.clone()
    if fault == "sin negated for one frequency":
        sin[:, 3] = -sin[:, 3]
    if fault == "table row of token l - 1":
        cos[1:], sin[1:] = c.cos[:-1], c.sin[:-1]
    lam = c.lam.float()
    outs = []
    kcols, vcols = R.pad_columns(hd, hdp)
    if fault == "ones column moved from hd + 4 to hd + 2":
        vcols = [hd, hd + 2]
    for which, ones in ((0, []), (1, kcols), (2, vcols)):
        x = R.head_major(c.qkv.float()[:, which * D:(which + 1) * D], B, L, H, hd)
        o = torch.zeros(B, H, L, hdp)
        if which < 2:
            o[..., :hd] = R.rotate(x, cos, sin)
        else:
            o[..., :hd] = lam * x + (1.0 - lam) * c.v0.float()[..., :hd] if c.v0 is not None else x
        for col in ones:
            o[..., col] = 1.0
        outs.append(o.to(bf16))
    return outs


def test_qkv_faults():
    c = R.qkv_fwd_case(3, 25, 3, 72, 96, True)

    def passes(fault=None):
        return all(torch.equal(G.bits(o), G.bits(w)) for o, w in zip(qkv_fwd32(c, fault), (c.want_q, c.want_k, c.want_v)))
    assert passes()
    for fault in ("sin negated for one frequency", "table row of token l - 1", "ones column moved from hd + 4 to hd + 2"):
        assert not passes(fault), fault
    # dlam = the sum of one partial per workgroup of four tokens (wave-per-token form): one partial lost
    b = R.qkv_bwd_case(3, 25, 12, 64, 64, 1, 0)
    D = b.H * b.hd
    vraw = R.head_major(b.qkv_raw.float()[:, 2 * D:], b.B, b.L, b.H, b.hd)
    terms = (b.dv.float()[..., :b.hd] * (vraw - b.v0.float()[..., :b.hd])).permute(0, 2, 1, 3).reshape(b.B * b.L, D).sum(1)
    parts = torch.stack([terms[i:i + 4].sum() for i in range(0, b.B * b.L, 4)])
    assert torch.equal(G.bits(b.dlam0 + parts.sum()), G.bits(b.want_dlam))
    lost = int(parts.abs().argmax())
    assert parts[lost] != 0
    assert not torch.equal(G.bits(b.dlam0 + parts.sum() - parts[lost]), G.bits(b.want_dlam))


def test_sentinel_is_no_value():
    """the output fill is no result of any case (each builder asserts it for its own outputs) and no input value"""
    for t in (R.S1, R.WSET, R.SHIFT, R.DY, R.TAB, R.LAM):
        assert not (G.bits(torch.tensor(t).to(bf16)) == G.SENTINEL_BF16).any()
    c = R.fwd_case(5, 7, 1544, True)     # the one draw that had to be repeated
    assert not (G.bits(c.want_y) == G.SENTINEL_BF16).any()
    assert torch.isnan(G.fill_value(bf16, "nan")) and G.fill_value(f32, "sentinel").item() < -6e18
