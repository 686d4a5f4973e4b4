"""Exact census of the row kernels on the GPU: bits against tests/helpers/row_census.py.

Every call goes through the C entry point with caller-owned buffers.  Row-major operands are windows of wider parents
(ld = D + 8, four guard rows before and after); the tensors of vds_qkv_rope_* (no stride in the ABI) lie between two
guard bands of four rows.  Input parents are NaN outside the window, output parents hold a sentinel no case produces: after
the call the window equals the expectation bit for bit and every byte outside it is still the sentinel.  dmod is
[B, 4 D] with shift at column 0 and scale / gate at 2 D; the columns between hold the sentinel and must survive.

Instance -> cases (the lists and their predicates are in the helper; test_row_census_cpu.py asserts the coverage):
  rmsnorm_mod_fwd_kernel<1..4>       D = 8 .. 512 | 520 .. 1024 | 1032 .. 1536 | 1544 .. 2048; <1> <2> <3> also at
                                     D = 384 / 768 / 1152 with rmsnorm_q4 = 0           test_rmsnorm_fwd
  rmsnorm_mod_fwd_q4_kernel<3|6|9>   D = 384 / 768 / 1152 (default knob)                test_rmsnorm_fwd
      rows (B, L) = (1, 1) (1, 17) (2, 16) (3, 21) (5, 7): one row, tails of 1 and 3 rows, waves that span samples
  rmsnorm_mod_bwd_kernel<1..4, w>    D = 8 144 512 | 520 1024 | 1152 1536 | 2048, L = 1 3 8 9 21 37, B = 1 3, knobs
                                     default / ew_min_rows 1 8 32 / ew_wgs 2, atomics and deterministic:
                                     dyadic rows everywhere, constant-m and generic rows at (3, 21) and (1, 9)
                                                                                        test_rmsnorm_bwd
                                     (2, 4100, 8): the default 32-row floor            test_floor32
  gate_bwd_kernel<1..4>              the same launches, with and without dbias          test_gate_bwd, test_floor32
  colsum_kernel                      M = 1 63 64 65 203 x N = 8 72 512 520 1152 x (rows_per_sample, row_offset) =
                                     (0, 0) (29, 16) (7, 0); (8193, 8)                  test_colsum
  qkv_rope_fwd_tile_kernel<hd,hdp,T> (72, 96) (64, 64) (128, 128) (96, 96) (32, 32) x T = 2 4 8, H = 1 3 (16 at 72)
  qkv_rope_fwd_kernel                the same at rope_tile 0 and L = 5; (24, 24) (48, 56) (64, 68); H hd = 2112
                                                                                        test_qkv_fwd
  qkv_rope_bwd_tok_kernel<1..4>      (hd, H) = (64, 2) (64, 12) (72, 16) (64, 32)
  qkv_rope_bwd_kernel                rope_tok 0, (64, 68), H hd = 2112; all with mix 0 / 0 + add_dv0 / 1 / 2,
                                     atomics and deterministic                          test_qkv_bwd
  rope_apply_kernel                  hd = 32 72 128, L = 25, forward and inverse, strided views   test_rope_apply
  the _grouped entries               (2, 21) x D = 384 520: groups NULL = the plain entry; one group per sample = the plain
                                     form, deterministic                                test_grouped_entries_*, test_one_group_*
  return codes                       D = 2056, D = 12, a pad the kernels cannot write, leading dimensions off 8
                                                                                        test_refusals
Each test prints the worst rstd error in fp32 ulps / the undecided share of its generic rows."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_census as G  # noqa: E402
import row_census as R  # noqa: E402

from video_diffusion_speedrun_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
VDS_ERR_ARG, VDS_ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib(ops):
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Knobs:
    def __init__(self, ops, knobs):
        self.ops, self.knobs, self.prev = ops, knobs, {}

    def __enter__(self):
        for k, v in self.knobs.items():
            self.prev[k] = self.ops.knob_set(k, v)

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            self.ops.knob_set(k, v)


class Deterministic:
    """vds_set_deterministic for the block (32 MB of partials: the largest launch here needs 3)"""
    def __init__(self, ops, on):
        self.ops, self.on = ops, on

    def __enter__(self):
        if self.on:
            self.ops.set_deterministic(True, workspace_bytes=32 << 20)

    def __exit__(self, *exc):
        if self.on:
            self.ops.set_deterministic(False)


class Win:
    """a 2-D operand as a window of a wider parent on the device: ld = columns + 8, four guard rows before and after"""
    def __init__(self, t, fill):
        self.before, view = G.embed(t, pad_rows=R.GUARD_ROWS, pad_cols=R.GAP, col0=0, fill=fill)
        self.where = G.locate(self.before, view)
        self.initial = t
        self.dev = self.before.cuda()
        self.ld = self.before.stride(0)
        self.ptr = self.dev.data_ptr() + (self.where[0] * self.ld + self.where[1]) * t.element_size()

    def check(self, want, what):
        G.assert_window(self.dev, self.before, self.where, want, what)

    def untouched(self, what):
        self.check(self.initial, what)

    def got(self):
        return G.window(self.dev.cpu(), self.where)


class Flat:
    """a contiguous tensor between two guard bands on the device (None stays a null pointer)"""
    def __init__(self, t, fill):
        self.initial, self.ptr = t, None
        if t is not None:
            self.before, _, guard = R.guarded(t, fill)
            self.dev = self.before.cuda()
            self.ptr = self.dev.data_ptr() + guard * t.element_size()

    def check(self, want, what, exact=True):
        return R.assert_guarded(self.dev, self.before, want, what, exact)

    def untouched(self, what):
        self.check(self.initial, what)


def out_bf16(rows, cols, fill="sentinel"):
    return Win(G.fill_value(bf16, fill).repeat(rows, cols), fill)


def blank_f32(*shape):
    return G.fill_value(f32, "sentinel").repeat(*shape)


# ---- RMSNorm + modulate, forward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,q4", [(D, 1) for D in R.FWD_D] + [(D, 0) for D in (384, 768, 1152)])
def test_rmsnorm_fwd(ops, lib, D, q4):
    worst = 0.0
    with Knobs(ops, {"rmsnorm_q4": q4}):
        for B, L in R.FWD_BL:
            for with_w in (False, True):
                c = R.fwd_case(B, L, D, with_w)
                what = f"{R.fwd_instance(D, q4)} B {B} L {L} D {D} w {with_w}"
                x, mod, w = Win(c.x, "nan"), Win(c.mod, "nan"), Flat(c.w, "nan")
                y, rstd = out_bf16(B * L, D), Flat(blank_f32(B * L), "sentinel")
                rc = lib.vds_rmsnorm_mod_fwd(x.ptr, x.ld, w.ptr, mod.ptr, mod.ld, 0, 2 * D, y.ptr, y.ld, rstd.ptr, B, L, D,
                                             R.EPS, stream())
                assert rc == 0, (what, rc)
                y.check(c.want_y, what + " y")
                u = R.ulps32(rstd.check(c.r64.to(f32), what + " rstd", exact=False), c.r64)
                assert u <= 4.0, f"{what}: rstd is {u:.2f} fp32 ulps from float64"
                worst = max(worst, u)
    print(f"rmsnorm fwd {R.fwd_instance(D, q4)} D {D}: worst rstd error {worst:.2f} fp32 ulps")


# ---- RMSNorm + modulate, backward --------------------------------------------------------------------------------------
def run_rmsnorm_bwd(lib, c, what):
    B, L, D = c.B, c.L, c.D
    dy, x, mod, w = Win(c.dy, "nan"), Win(c.x, "nan"), Win(c.mod, "nan"), Flat(c.w, "nan")
    dres = Win(c.dres, "nan") if c.dres is not None else None
    rstd = Flat(c.rstd, "nan")
    dx = out_bf16(B * L, D, "nan" if c.kind == "generic" else "sentinel")
    dmod, dw = Win(c.dmod0, "sentinel"), Flat(c.dw0, "sentinel")
    rc = lib.vds_rmsnorm_mod_bwd(dy.ptr, dy.ld, x.ptr, x.ld, w.ptr, mod.ptr, mod.ld, 0, 2 * D, rstd.ptr,
                                 dres.ptr if dres else None, dres.ld if dres else 0, dx.ptr, dx.ld, dmod.ptr, dw.ptr,
                                 B, L, D, stream())
    assert rc == 0, (what, rc)
    if c.kind == "generic":
        R.check_dx(dx.got(), c)
        G.assert_outside(dx.dev, dx.before, dx.where, what + " dx")
        got = dmod.got()
        for c0 in (D, 3 * D):   # the columns of no call
            assert torch.equal(G.bits(got[:, c0:c0 + D]), G.bits(c.dmod0[:, c0:c0 + D])), what + " dmod poison"
        G.assert_outside(dmod.dev, dmod.before, dmod.where, what + " dmod")
        return
    dx.check(c.want_dx, what + " dx")
    dmod.check(c.want_dmod, what + " dmod")
    if c.w is not None:
        dw.check(c.want_dw, what + " dw")


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("D", R.BWD_D)
def test_rmsnorm_bwd(ops, lib, D, det):
    shares = []
    with Deterministic(ops, det):
        for B, L, knobs, with_w, with_dres in R.bwd_plan(D):
            with Knobs(ops, knobs):
                what = f"NC {R.nc_of(D)} B {B} L {L} D {D} w {with_w} dres {with_dres} {knobs} det {det}"
                run_rmsnorm_bwd(lib, R.bwd_case(B, L, D, with_w, with_dres, "dyadic"), what)
                if (B, L) in R.BWD_GENERIC_BL:
                    run_rmsnorm_bwd(lib, R.bwd_case(B, L, D, with_w, True, "const"), what + " const")
                    c = R.bwd_case(B, L, D, with_w, with_dres, "generic")
                    run_rmsnorm_bwd(lib, c, what + " generic")
                    shares.append(c.share)
    print(f"rmsnorm bwd D {D} det {det}: undecided share of the generic rows {min(shares):.2%} .. {max(shares):.2%}")


# ---- gate backward -----------------------------------------------------------------------------------------------------
def run_gate_bwd(lib, c, with_dbias, what):
    B, L, D = c.B, c.L, c.D
    dxn, y, mod = Win(c.dxn, "nan"), Win(c.y, "nan"), Win(c.mod, "nan")
    dy, dmod = out_bf16(B * L, D), Win(c.dmod0, "sentinel")
    dbias = Flat(c.dbias0 if with_dbias else None, "sentinel")
    rc = lib.vds_gate_bwd(dxn.ptr, dxn.ld, y.ptr, y.ld, mod.ptr, mod.ld, 2 * D, dy.ptr, dy.ld, dmod.ptr, dbias.ptr, B, L, D,
                          stream())
    assert rc == 0, (what, rc)
    dy.check(c.want_dy, what + " dy")
    dmod.check(c.want_dmod, what + " dmod")
    if with_dbias:
        dbias.check(c.want_dbias, what + " dbias")


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("D", R.BWD_D)
def test_gate_bwd(ops, lib, D, det):
    with Deterministic(ops, det):
        for B, L, knobs, with_dbias, _ in R.bwd_plan(D):
            with Knobs(ops, knobs):
                run_gate_bwd(lib, R.gate_case(B, L, D), with_dbias,
                             f"gate NC {R.nc_of(D)} B {B} L {L} D {D} dbias {with_dbias} {knobs} det {det}")


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
def test_floor32(ops, lib, det):
    """8200 rows: the default knobs walk 32 rows per workgroup (129 workgroups per sample, the last of 4 rows)"""
    B, L, D = R.BWD_FLOOR32
    assert R.rows_per_block(L, B) == 32 and ops.knob_get("ew_min_rows") == 8 and ops.knob_get("ew_wgs") in (0, 768)
    with Deterministic(ops, det):
        for with_w in (False, True):
            run_rmsnorm_bwd(lib, R.bwd_case(B, L, D, with_w, True, "dyadic"), f"floor 32 w {with_w} det {det}")
        run_gate_bwd(lib, R.gate_case(B, L, D), True, f"floor 32 gate det {det}")


# ---- column sums -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
def test_colsum(ops, lib, det):
    with Deterministic(ops, det):
        for M, N in [(M, N) for M in R.COLSUM_M for N in R.COLSUM_N] + [R.COLSUM_BIG]:
            for rps, roff in R.COLSUM_ROWS:
                xc, out0, want = R.colsum_case(M, N, rps, roff)
                what = f"colsum M {M} N {N} rows_per_sample {rps} row_offset {roff} det {det}"
                x, out = Win(xc, "nan"), Flat(out0, "sentinel")
                if rps == 0:
                    rc = lib.vds_colsum_bf16(x.ptr, x.ld, out.ptr, M, N, stream())
                else:
                    rc = lib.vds_colsum_bf16_rows(x.ptr, x.ld, out.ptr, M, N, rps, roff, stream())
                assert rc == 0, (what, rc)
                out.check(want, what)


# ---- qkv split / RoPE / residual-V -------------------------------------------------------------------------------------
def run_qkv_fwd(lib, c, what):
    B, L, H, hd, hdp = c.B, c.L, c.H, c.hd, c.hdp
    qkv, cos, sin = Flat(c.qkv, "nan"), Flat(c.cos, "nan"), Flat(c.sin, "nan")
    v0, lam = Flat(c.v0, "nan"), Flat(c.lam, "nan")
    outs = [Flat(G.fill_value(bf16, "sentinel").repeat(B, H, L, hdp), "sentinel") for _ in range(3)]
    rc = lib.vds_qkv_rope_fwd(qkv.ptr, cos.ptr, sin.ptr, v0.ptr, lam.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr, B, L, H, hd,
                              hdp, stream())
    assert rc == 0, (what, rc)
    for o, want, name in zip(outs, (c.want_q, c.want_k, c.want_v), "qkv"):
        o.check(want, f"{what} {name}")


@pytest.mark.parametrize("hd,hdp,H", R.QKV_FWD_TILE + R.QKV_FWD_ELEM)
def test_qkv_fwd(ops, lib, hd, hdp, H):
    tiles = (2, 4, 8, 0) if (hd, hdp, H) in R.QKV_FWD_TILE else (None,)
    for tile in tiles:
        with Knobs(ops, {} if tile is None else {"rope_tile": tile}):
            for B, L in R.QKV_BL:
                for with_v0 in (False, True):
                    form = R.qkv_fwd_form(H, hd, hdp, L, 4 if tile is None else tile)
                    run_qkv_fwd(lib, R.qkv_fwd_case(B, L, H, hd, hdp, with_v0),
                                f"{form} B {B} L {L} H {H} hd {hd} hdp {hdp} v0 {with_v0}")


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("i", range(len(R.QKV_BWD)), ids=[R.qkv_bwd_form(H, hd, hdp, k.get("rope_tok", 1)).replace(" ", "_")
                                                          for hd, hdp, H, k in R.QKV_BWD])
def test_qkv_bwd(ops, lib, i, det):
    hd, hdp, H, knobs = R.QKV_BWD[i]
    form = R.qkv_bwd_form(H, hd, hdp, knobs.get("rope_tok", 1))
    with Deterministic(ops, det), Knobs(ops, knobs):
        for B, L in R.QKV_BWD_BL:
            for mix, add_dv0 in R.QKV_BWD_MODES:
                c = R.qkv_bwd_case(B, L, H, hd, hdp, mix, add_dv0)
                what = f"{form} B {B} L {L} H {H} hd {hd} hdp {hdp} mix {mix} add_dv0 {add_dv0} det {det}"
                dq, dk, dv = Flat(c.dq, "nan"), Flat(c.dk, "nan"), Flat(c.dv, "nan")
                cos, sin, raw = Flat(c.cos, "nan"), Flat(c.sin, "nan"), Flat(c.qkv_raw, "nan")
                v0, lam = Flat(c.v0, "nan"), Flat(c.lam, "nan")
                acc, dlam = Flat(c.acc0, "sentinel"), Flat(c.dlam0, "sentinel")
                dqkv = Flat(G.fill_value(bf16, "sentinel").repeat(B * L, 3 * H * hd), "sentinel")
                rc = lib.vds_qkv_rope_bwd(dq.ptr, dk.ptr, dv.ptr, cos.ptr, sin.ptr, raw.ptr, v0.ptr, lam.ptr, acc.ptr, dlam.ptr,
                                          dqkv.ptr, mix, add_dv0, B, L, H, hd, hdp, stream())
                assert rc == 0, (what, rc)
                dqkv.check(c.want_dqkv, what + " dqkv")
                acc.check(c.want_acc, what + " dv0_acc")
                dlam.check(c.want_dlam, what + " dlam")


@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("hd", R.ROPE_APPLY_HD)
def test_rope_apply(lib, ops, hd, inverse):
    B, H, L = 2, 3, R.ROPE_APPLY_L
    xc, cosc, sinc, want = R.rope_apply_case(B, H, L, hd, inverse)
    # strided head-major views: rows 1 .. L of [B, H, L + 2, hd + 8] parents
    xin = G.fill_value(bf16, "nan").repeat(B, H, L + 2, hd + 8)
    xin[:, :, 1:L + 1, :hd] = xc
    before = G.fill_value(bf16, "sentinel").repeat(B, H, L + 2, hd + 8)
    xd, yd = xin.cuda(), before.cuda()
    cos, sin = Flat(cosc, "nan"), Flat(sinc, "nan")
    sb, sh, sl = xin.stride()[:3]
    off = sl * 2
    rc = lib.vds_rope_apply(xd.data_ptr() + off, sb, sh, sl, cos.ptr, sin.ptr, yd.data_ptr() + off, sb, sh, sl, B, H, L, hd,
                            inverse, stream())
    assert rc == 0, rc
    expect = before.clone()
    expect[:, :, 1:L + 1, :hd] = want
    assert torch.equal(G.bits(yd.cpu()), G.bits(expect)), f"rope_apply hd {hd} inverse {inverse}"


# ---- the grouped entries against the plain ones ------------------------------------------------------------------------
GROUPED_BL = (2, 21)       # three 8-row blocks per sample, the last of 5 rows
GROUPED_D = (384, 520)     # the four-rows-per-wave forward; two chunks per row with one lane in the second


def row_calls(lib, D, form):
    """forward, backward and gate backward of the dyadic cases at GROUPED_BL x D -> every output as the caller sees it.
    form "plain": the plain entries; None: the grouped entries with a NULL description; (lead, period) that puts all L rows of
    a sample into ONE group: the grouped entries on tables of two rows per sample, the rows of the empty groups NaN (mod) and
    sentinel (dmod: returned apart, they must survive).  Guard bands and gaps are checked on every output."""
    B, L = GROUPED_BL
    grouped = form != "plain"
    gr = None if form in ("plain", None) else C.byref(_lib.ModGroups(*form))
    slot, per = (0, 1) if gr is None else ((1 if form[0] == 0 else 0), 2)  # the table row of sample b: per * b + slot
    tail = ((gr,) if grouped else ()) + (stream(),)
    entry = (lambda n: getattr(lib, n + "_grouped")) if grouped else (lambda n: getattr(lib, n))

    def table(t, fill):
        out = G.fill_value(t.dtype, fill).repeat(per * B, t.shape[1])
        out[slot::per] = t
        return Win(out, fill)

    def rows(win, what):
        G.assert_outside(win.dev, win.before, win.where, what)
        return win.got()

    def flat(f, what):
        return f.check(f.initial, what, exact=False)

    def split(dmod, what, res):
        got = rows(dmod, what)
        res[what], res[what + " of the empty groups"] = got[slot::per], got[1 - slot::per] if per == 2 else got[:0]

    res = {}
    c = R.fwd_case(B, L, D, True)
    x, mod, w = Win(c.x, "nan"), table(c.mod, "nan"), Flat(c.w, "nan")
    y, rstd = out_bf16(B * L, D), Flat(blank_f32(B * L), "sentinel")
    rc = entry("vds_rmsnorm_mod_fwd")(x.ptr, x.ld, w.ptr, mod.ptr, mod.ld, 0, 2 * D, y.ptr, y.ld, rstd.ptr, B, L, D, R.EPS,
                                      *tail)
    assert rc == 0, ("fwd", form, rc)
    res["y"], res["rstd"] = rows(y, "y"), flat(rstd, "rstd")

    c = R.bwd_case(B, L, D, True, True, "dyadic")
    dy, x, mod, w = Win(c.dy, "nan"), Win(c.x, "nan"), table(c.mod, "nan"), Flat(c.w, "nan")
    dres, rstd, dx = Win(c.dres, "nan"), Flat(c.rstd, "nan"), out_bf16(B * L, D)
    dmod, dw = table(c.dmod0, "sentinel"), Flat(c.dw0, "sentinel")
    rc = entry("vds_rmsnorm_mod_bwd")(dy.ptr, dy.ld, x.ptr, x.ld, w.ptr, mod.ptr, mod.ld, 0, 2 * D, rstd.ptr, dres.ptr, dres.ld,
                                      dx.ptr, dx.ld, dmod.ptr, dw.ptr, B, L, D, *tail)
    assert rc == 0, ("bwd", form, rc)
    res["dx"], res["dw"] = rows(dx, "dx"), flat(dw, "dw")
    split(dmod, "dmod", res)

    c = R.gate_case(B, L, D)
    dxn, yy, mod = Win(c.dxn, "nan"), Win(c.y, "nan"), table(c.mod, "nan")
    dyo, dmod, dbias = out_bf16(B * L, D), table(c.dmod0, "sentinel"), Flat(c.dbias0, "sentinel")
    rc = entry("vds_gate_bwd")(dxn.ptr, dxn.ld, yy.ptr, yy.ld, mod.ptr, mod.ld, 2 * D, dyo.ptr, dyo.ld, dmod.ptr, dbias.ptr, B, L,
                               D, *tail)
    assert rc == 0, ("gate", form, rc)
    res["gate dy"], res["dbias"] = rows(dyo, "gate dy"), flat(dbias, "dbias")
    split(dmod, "gate dmod", res)
    torch.cuda.synchronize()
    return res


def same_bits(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(G.bits(a[k]), G.bits(b[k])), f"{what}: {k} differs"


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("D", GROUPED_D)
def test_grouped_entries_without_a_description_are_the_plain_entries(ops, lib, D, det):
    """groups == NULL forwards: every output of the three grouped entries has the plain entry's bits (dyadic cases: the column
    sums are exact, so the atomics' order does not show)"""
    with Deterministic(ops, det):
        plain = row_calls(lib, D, "plain")
        same_bits(plain, row_calls(lib, D, None), f"groups NULL, D {D}, det {det}")
    c = R.bwd_case(*GROUPED_BL, D, True, True, "dyadic")   # and they are the census's bits
    assert torch.equal(G.bits(plain["dmod"]), G.bits(c.want_dmod)) and torch.equal(G.bits(plain["dx"]), G.bits(c.want_dx))


@pytest.mark.parametrize("form", [(0, 1), (GROUPED_BL[1], 1)], ids=["all_rows_in_group_1", "all_rows_in_group_0"])
@pytest.mark.parametrize("D", GROUPED_D)
def test_one_group_per_sample_is_the_plain_form_in_deterministic_mode(ops, lib, D, form):
    """deterministic mode: with one non-empty group per sample the grouped grid is the plain grid plus workgroups that leave
    zeros, and the fixed-order sums add them in place -- dmod, dw and dbias (and y, rstd, dx, dy) equal the plain form's bit
    for bit; the dmod rows of the empty groups are not written"""
    with Deterministic(ops, True):
        plain, one = row_calls(lib, D, "plain"), row_calls(lib, D, form)
    for k in ("dmod", "gate dmod"):
        empty = one.pop(k + " of the empty groups")
        assert empty.shape == plain[k].shape and torch.all(G.bits(empty) == G.SENTINEL_F32), f"{k}: an empty group's row changed"
        plain.pop(k + " of the empty groups")
    same_bits(plain, one, f"groups {form}, D {D}")


# ---- return codes ------------------------------------------------------------------------------------------------------
def test_refusals(ops, lib):
    B, L = 2, 3

    def rms(D, ldgap=8, lddres_off=0):
        """one forward, one backward and one gate launch on full-size buffers -> their return codes; outputs untouched"""
        z = torch.zeros(B * L, D + 8, dtype=bf16)
        x, mod = Win(z, "nan"), Win(torch.zeros(B, 4 * (D + 8), dtype=f32), "nan")
        y, rstd = out_bf16(B * L, D + 8), Flat(blank_f32(B * L), "sentinel")
        dmod = Win(blank_f32(B, 4 * (D + 8)), "sentinel")
        dbias = Flat(blank_f32(D + 8), "sentinel")
        ld = x.ld - 8 + ldgap
        rcs = [lib.vds_rmsnorm_mod_fwd(x.ptr, ld, None, mod.ptr, mod.ld, 0, 2 * D + 8, y.ptr, ld, rstd.ptr, B, L, D, R.EPS,
                                       stream()),
               lib.vds_rmsnorm_mod_bwd(x.ptr, x.ld, x.ptr, x.ld, None, mod.ptr, mod.ld, 0, 2 * D + 8, rstd.ptr,
                                       x.ptr, x.ld + lddres_off, y.ptr, y.ld, dmod.ptr, None, B, L, D,
                                       stream()),
               lib.vds_gate_bwd(x.ptr, ld, x.ptr, x.ld, mod.ptr, mod.ld, 2 * D + 8, y.ptr, y.ld, dmod.ptr, dbias.ptr, B, L, D,
                                stream()),
               lib.vds_gate_bwd(x.ptr, x.ld, x.ptr, ld, mod.ptr, mod.ld, 2 * D + 8, y.ptr, y.ld, dmod.ptr, dbias.ptr, B, L, D,
                                stream()),
               lib.vds_gate_bwd(x.ptr, x.ld, x.ptr, x.ld, mod.ptr, mod.ld, 2 * D + 8, y.ptr, ld, dmod.ptr, dbias.ptr, B, L, D,
                                stream())]
        torch.cuda.synchronize()
        for o, name in ((y, "y"), (rstd, "rstd"), (dmod, "dmod"), (dbias, "dbias")):
            o.untouched(f"refused D {D}: {name}")
        return rcs

    assert rms(2056) == [VDS_ERR_UNSUPPORTED] * 5          # five chunks per lane: no instance
    assert rms(12) == [VDS_ERR_ARG] * 5                     # D % 8
    # leading dimensions that break the 16-byte row segments (ldx / ldy of the forward, lddres of the backward, lddxn, ldy
    # and lddy of the gate backward, one per launch): four elements short of the parents' own
    rcs = rms(144, ldgap=4, lddres_off=-4)
    assert rcs == [VDS_ERR_ARG] * 5, rcs
    # the pad the kernels cannot write: (hdp - hd) / 4 chunks of pad for hd / 8 threads per head
    hd, hdp, H = 64, 104, 2
    assert R.pad_refused(hd, hdp)
    qkv = Flat(torch.zeros(B * L, 3 * H * hd, dtype=bf16), "nan")
    tab = Flat(torch.zeros(L, hd // 2, dtype=f32), "nan")
    outs = [Flat(G.fill_value(bf16, "sentinel").repeat(B, H, L, hdp), "sentinel") for _ in range(3)]
    rc = lib.vds_qkv_rope_fwd(qkv.ptr, tab.ptr, tab.ptr, None, None, outs[0].ptr, outs[1].ptr, outs[2].ptr, B, L, H, hd, hdp,
                              stream())
    assert rc == VDS_ERR_UNSUPPORTED, rc
    torch.cuda.synchronize()
    for o in outs:
        o.untouched("refused pad")
