"""Exact census of the step-edge kernels on the GPU: bits against tests/helpers/edge_census.py.

Every call goes through the C entry point with caller-owned buffers.  Each tensor lies between two guard bands; input
parents are NaN outside the payload (where the dtype has one), output parents hold a sentinel no case produces: after
the call the payload equals the expectation bit for bit (or lies inside the derived bound, for SiLU) and every byte
outside it still holds the sentinel -- the register rows in front of every sample of the *_rows patch entries, the gap
between R D and batch_stride of vds_fill_registers, the words of a loss workspace past vds_flow_loss*_workspace_floats,
the deterministic partials past the entry's own size rule.

Branch -> cases (the lists and their predicates are in the helper; test_edge_census_cpu.py asserts the coverage and
prints the same table shape by shape):
  small_linear_fwd_mfma_kernel     N = 1024 / 1040 (a last workgroup with one live wave) x K = 32 160 192 224 416 1696
                                   (K / 32 below, at, above the 6-step unroll, two trips + 1, the largest in LDS),
                                   M = 1 4 5 8 9 16 and 17 / 33 in chunks, with and without bias, adaln_mfma 1 and 0
                                                                                         test_linear_fwd
  small_linear_fwd_kernel<4|8|16>  K = 1728 (the MFMA fallback); N = 1 3 4 5 17 203 x K = 8 504 512 520 (63 / 64 / 65
                                   chunks over 64 lanes), M = 17 and 33 in chunks        test_linear_fwd
  small_linear_dw_kernel           N = 1 5 70 x K = 8 72 x M = 1 16 17, dbias NULL / given, W and dx NULL
                                                                                         test_linear_dw
  small_linear_dx_kernel<4|8|16>   N = 17 33 70 (ny 1 2 3, ragged last range) x K = 8 72 (dead column lanes), chunked
                                   M, dW NULL, atomics and deterministic; dW + dbias + dx in one call
                                                                                         test_linear_dx
                                   rows > 384 (two LDS slices): per-set (5, 1600, 8192), batched 16 pointers over two
                                   matrices (5, 800, 4096)                               test_linear_dx_slices
  small_linear_dw_tile_kernel      (N, K) = (4, 8) (64, 128) (68, 136) x nb = 1 3 x M = 3 4 5 8 9 16, dbias table NULL /
                                   given; batched forward (MFMA and row) and dx          test_linear_batched
  act_in = 1                       all five kernels inside the derived bound             test_linear_silu
  flow_loss_partial / _final       per = 8 4096 | 4097 | 262144 / 262145 | 1048576 / 1048576 + 4097, B = 1 3 (5 up to
                                   4097), dout NULL / given, two calls                   test_flow_loss
  flow_loss_frames_partial/_final  (C, T, HW, tps) = (5,6,21,2) (16,4,136,2) (16,2,16512,1) (5,6,21,1|3) (5,2,21,2),
                                   B = 1 3 5; _bwd at the first two                      test_flow_loss_frames
  flow_loss_bwd_kernel             n = 8, 8 x 255, 8 x 256 x 2048, 8 x (256 x 2048 + 3)  test_flow_loss_bwd
  patchify / unpatchify<fwd|bwd>   (pt, p) = (1,1) (1,2) (2,2) (4,2) (1,4) x C = 3 16 x (4,6,10) (4,8,8) x B = 1 3,
                                   dense and 16 register rows per sample                 test_patches
  fill_registers / registers_bwd   (R, D) = (16,72) (16,128) (3,8) x B = 1 3 x three strides   test_registers
  noise_kernel / noise_frames      (B, per) = (3,100) (1|3,4097) (1,8); (5,6,21,1|2|3)   test_noise
  cfg_euler_kernel                 n = 8, 8 x 255, 8 x 256, 8 x 257, cfg 1 3 7.5, uncond NULL / given   test_cfg_euler
  cast kernels                     n = 1 7 8 9 2047 2048 2049, special values, pointers off 16 bytes; all 65536 bf16
                                                                                         test_casts
  rope_rows_kernel                 tables (5,3) (16,24) x (t,h,w) (1,1,1) (3,5,7) (4,8,8) x n_reg 0 16 x three starts,
                                   host and device offsets, the device clamp             test_rope_rows
  timestep_embedding_kernel        D = 2 16 258 384 1152 x B = 1 5 61                    test_timestep_embedding
  return codes                                                                           test_refusals
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import edge_census as E  # noqa: E402
import gemm_census as G  # noqa: E402
import row_census as R  # noqa: E402

from video_diffusion_speedrun_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
VDS_ERR_ARG = -1


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


class Flat:
    """a contiguous tensor between two guard bands on the device (None stays a null pointer)"""
    def __init__(self, t, fill):
        self.initial, self.ptr = t, None
        if t is not None:
            self.before, _, self.guard = R.guarded(t, fill)
            self.dev = self.before.cuda()
            self.ptr = self.dev.data_ptr() + self.guard * t.element_size()

    def check(self, want, what, exact=True):
        return R.assert_guarded(self.dev, self.before, want, what, exact)

    def got(self):
        return self.check(self.initial, "", exact=False)

    def untouched(self, what):
        self.check(self.initial, what)


def nan_in(t):
    return Flat(t, "nan")


def blank(dtype, *shape):
    return Flat(G.fill_value(dtype, "sentinel").repeat(*shape), "sentinel")


class Deterministic:
    """vds_set_deterministic with a workspace of exactly `floats` floats (the entry's own rule; 4096 bytes at least)
    between sentinel guard bands that must survive"""
    def __init__(self, lib, floats):
        self.lib, self.floats = lib, floats

    def __enter__(self):
        if self.floats:
            self.ws = blank(f32, max(1024, self.floats))
            assert self.lib.vds_set_deterministic(1, self.ws.ptr, max(1024, self.floats) * 4) >= 0
        return self

    def __exit__(self, *exc):
        if self.floats:
            torch.cuda.synchronize()
            assert self.lib.vds_set_deterministic(0, None, 0) >= 0
            if exc[0] is None:
                self.ws.check(self.ws.initial, "deterministic workspace", exact=False)


def table(ptrs):
    """device array of device pointers"""
    return torch.tensor([p if p is not None else 0 for p in ptrs], dtype=torch.int64).cuda()


# ---- small linears, act_in = 0: bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mfma", [1, 0], ids=["adaln_mfma_1", "adaln_mfma_0"])
def test_linear_fwd(ops, lib, mfma):
    with Knobs(ops, {"adaln_mfma": mfma}):
        for M, N, K, with_bias in E.fwd_plan():
            c = E.linear_case(M, N, K, 1, with_bias)
            what = f"fwd {E.fwd_kernels(M, N, K, mfma)} M {M} N {N} K {K} bias {with_bias}"
            x, W, bias = nan_in(c.x), nan_in(c.W[0]), nan_in(c.bias[0] if with_bias else None)
            y = blank(f32, M, N)
            rc = lib.vds_small_linear_fwd(x.ptr, W.ptr, bias.ptr, y.ptr, M, N, K, 0, stream())
            assert rc == 0, (what, rc)
            y.check(c.y[0], what)


def test_linear_dw(ops, lib):
    for M, N, K, with_dbias in E.dw_plan():
        c = E.linear_case(M, N, K, 1, True)
        what = f"dw M {M} N {N} K {K} dbias {with_dbias}"
        dy, x = nan_in(c.dy[0]), nan_in(c.x)
        dW, dbias = blank(f32, N, K), blank(f32, N) if with_dbias else Flat(None, "")
        rc = lib.vds_small_linear_bwd(dy.ptr, x.ptr, None, dW.ptr, dbias.ptr, None, M, N, K, 0, stream())
        assert rc == 0, (what, rc)
        dW.check(c.dW[0], what + " dW")
        if with_dbias:
            dbias.check(c.dbias[0], what + " dbias")


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
def test_linear_dx(ops, lib, det):
    for i, (M, N, K) in enumerate(E.dx_plan()):
        c = E.linear_case(M, N, K)
        both = i % 3 == 0        # dW + dbias + dx in one call; else dx alone (dW NULL)
        what = f"dx {E.dx_split(N, K)} M {M} N {N} K {K} det {det} with dW {both}"
        dy, x, W = nan_in(c.dy[0]), nan_in(c.x), nan_in(c.W[0])
        dx = Flat(c.dx0, "sentinel")
        dW, dbias = (blank(f32, N, K), blank(f32, N)) if both else (Flat(None, ""), Flat(None, ""))
        with Deterministic(lib, E.dx_workspace_floats(M, N, K) if det else 0):
            rc = lib.vds_small_linear_bwd(dy.ptr, x.ptr, W.ptr, dW.ptr, dbias.ptr, dx.ptr, M, N, K, 0, stream())
            assert rc == 0, (what, rc)
            dx.check(c.dx, what + " dx")
        if both:
            dW.check(c.dW[0], what + " dW")
            dbias.check(c.dbias[0], what + " dbias")


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("batched", [False, True], ids=["per_set", "batched"])
def test_linear_dx_slices(ops, lib, batched, det):
    """rows_per_block = 416 > 384: the workgroup walks two LDS slices of dy"""
    if not batched:
        M, N, K = E.DX_BIG
        assert E.dx_split(N, K) == (K // 64, 4, 416, 2)
        c = E.linear_case(M, N, K, 1, True, None, False)
        dy, x, W, dx = nan_in(c.dy[0]), nan_in(c.x), nan_in(c.W[0]), Flat(c.dx0, "sentinel")
        with Deterministic(lib, E.dx_workspace_floats(M, N, K) if det else 0):
            rc = lib.vds_small_linear_bwd(dy.ptr, x.ptr, W.ptr, None, None, dx.ptr, M, N, K, 0, stream())
            assert rc == 0, rc
            dx.check(c.dx, f"dx slices per-set det {det}")
        return
    M, N, K, nb = E.DX_BIG_BATCHED
    assert E.dx_split(N, K, nb) == (K // 64, 2, 416, 2)
    c = E.linear_case(M, N, K, 2, True, nb, False)
    dy, x, dx = nan_in(c.dy), nan_in(c.x), Flat(c.dx0, "sentinel")
    Ws = [nan_in(c.W[w]) for w in range(2)]
    tab = table([Ws[i % 2].ptr for i in range(nb)])
    with Deterministic(lib, E.dx_workspace_floats(M, N, K, nb) if det else 0):
        rc = lib.vds_small_linear_bwd_batched(dy.ptr, M * N, x.ptr, tab.data_ptr(), None, None, dx.ptr, nb, M, N, K, 0, stream())
        assert rc == 0, rc
        dx.check(c.dx, f"dx slices batched det {det}")


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
def test_linear_batched(ops, lib, det):
    if not det:
        for mfma in (1, 0):
            with Knobs(ops, {"adaln_mfma": mfma}):
                for M, N, K, nb, with_bias in E.BATCHED_FWD:
                    c = E.linear_case(M, N, K, nb, with_bias, nb)
                    what = f"fwd batched mfma {E.mfma_rule(M, N, K, mfma)} M {M} N {N} K {K} nb {nb} bias {with_bias}"
                    x, y = nan_in(c.x), blank(f32, nb, M, N)
                    Ws = [nan_in(c.W[i]) for i in range(nb)]
                    bs = [nan_in(c.bias[i]) for i in range(nb)] if with_bias else None
                    wt = table([w.ptr for w in Ws])
                    bt = table([b.ptr for b in bs]) if with_bias else None
                    rc = lib.vds_small_linear_fwd_batched(x.ptr, wt.data_ptr(), bt.data_ptr() if with_bias else None, y.ptr, M * N,
                                                          nb, M, N, K, 0, stream())
                    assert rc == 0, (what, rc)
                    y.check(c.y, what)
        for M, N, K, nb, with_dbias in E.tile_plan():
            c = E.linear_case(M, N, K, nb, True, nb)
            what = f"dw_tile<{E.fwd_instance(M)}> grid {E.dw_tile_grid(N, K, nb)} M {M} dbias {with_dbias}"
            dy, x = nan_in(c.dy), nan_in(c.x)
            dWs = [blank(f32, N, K) for _ in range(nb)]
            dbs = [blank(f32, N) for _ in range(nb)]
            wt, bt = table([d.ptr for d in dWs]), table([d.ptr for d in dbs])
            rc = lib.vds_small_linear_bwd_batched(dy.ptr, M * N, x.ptr, None, wt.data_ptr(), bt.data_ptr() if with_dbias else None,
                                                  None, nb, M, N, K, 0, stream())
            assert rc == 0, (what, rc)
            for i in range(nb):
                dWs[i].check(c.dW[i], f"{what} dW[{i}]")
                if with_dbias:
                    dbs[i].check(c.dbias[i], f"{what} dbias[{i}]")
                else:
                    dbs[i].untouched(f"{what} dbias[{i}] (no table)")
    for M, N, K, nb in E.BATCHED_DX:
        nw = max(1, nb - 1)      # W tables may repeat a matrix
        c = E.linear_case(M, N, K, nw, True, nb)
        what = f"dx batched {E.dx_split(N, K, nb)} M {M} N {N} K {K} nb {nb} det {det}"
        dy, x, dx = nan_in(c.dy), nan_in(c.x), Flat(c.dx0, "sentinel")
        Ws = [nan_in(c.W[w]) for w in range(nw)]
        wt = table([Ws[i % nw].ptr for i in range(nb)])
        dWs = [blank(f32, N, K) for _ in range(nb)]
        dwt = table([d.ptr for d in dWs])
        with Deterministic(lib, E.dx_workspace_floats(M, N, K, nb) if det else 0):
            rc = lib.vds_small_linear_bwd_batched(dy.ptr, M * N, x.ptr, wt.data_ptr(), dwt.data_ptr(), None, dx.ptr, nb, M, N, K, 0,
                                                  stream())
            assert rc == 0, (what, rc)
            dx.check(c.dx, what + " dx")
        for i in range(nb):
            dWs[i].check(c.dW[i], f"{what} dW[{i}]")


# ---- small linears, act_in = 1: the derived bound ------------------------------------------------------------------------
def test_linear_silu(ops, lib, parity_log):
    worst = {"row": 0.0, "mfma": 0.0, "dw": 0.0, "dx": 0.0, "dw_tile": 0.0, "dx_batched": 0.0}
    for mfma in (1, 0):
        with Knobs(ops, {"adaln_mfma": mfma}):
            for M, N, K, with_bias in E.ACT_FWD:
                c = E.act_case(M, N, K, with_bias)
                kern = "mfma" if E.mfma_rule(min(M, 16), N, K, mfma) else "row"
                what = f"silu fwd {kern} M {M} N {N} K {K}"
                x, W, bias = nan_in(c.x), nan_in(c.W[0]), nan_in(c.bias[0] if with_bias else None)
                y = blank(f32, M, N)
                rc = lib.vds_small_linear_fwd(x.ptr, W.ptr, bias.ptr, y.ptr, M, N, K, 1, stream())
                assert rc == 0, (what, rc)
                worst[kern] = max(worst[kern], E.within(what, y.check(c.y[0].to(f32), what, exact=False), c.y[0], c.y_bound[0], c.y_sum[0]))
    for det in (False, True):
        for M, N, K in E.ACT_BWD:
            c = E.act_case(M, N, K, True)
            what = f"silu bwd M {M} N {N} K {K} det {det}"
            dy, x, W = nan_in(c.dy[0]), nan_in(c.x), nan_in(c.W[0])
            dW, dbias, dx = blank(f32, N, K), blank(f32, N), Flat(torch.zeros(M, K, dtype=f32), "sentinel")
            with Deterministic(lib, E.dx_workspace_floats(M, N, K) if det else 0):
                rc = lib.vds_small_linear_bwd(dy.ptr, x.ptr, W.ptr, dW.ptr, dbias.ptr, dx.ptr, M, N, K, 1, stream())
                assert rc == 0, (what, rc)
                got_dx = dx.check(c.dx.to(f32), what, exact=False)
            worst["dw"] = max(worst["dw"], E.within(what + " dW", dW.check(c.dW[0].to(f32), what, exact=False), c.dW[0], c.dW_bound[0], c.dW_sum[0]))
            dbias.check(c.dbias[0], what + " dbias")
            worst["dx"] = max(worst["dx"], E.within(what + " dx", got_dx, c.dx, c.dx_bound, c.dx_sum))
        for M, N, K, nb in E.ACT_BATCHED:
            c = E.act_case(M, N, K, True, nb)
            what = f"silu bwd batched M {M} N {N} K {K} nb {nb} det {det}"
            dy, x = nan_in(c.dy), nan_in(c.x)
            Ws = [nan_in(c.W[i]) for i in range(nb)]
            dWs, dbs = [blank(f32, N, K) for _ in range(nb)], [blank(f32, N) for _ in range(nb)]
            dx = Flat(torch.zeros(M, K, dtype=f32), "sentinel")
            wt, dwt, dbt = table([w.ptr for w in Ws]), table([d.ptr for d in dWs]), table([d.ptr for d in dbs])
            with Deterministic(lib, E.dx_workspace_floats(M, N, K, nb) if det else 0):
                rc = lib.vds_small_linear_bwd_batched(dy.ptr, M * N, x.ptr, wt.data_ptr(), dwt.data_ptr(), dbt.data_ptr(), dx.ptr,
                                                      nb, M, N, K, 1, stream())
                assert rc == 0, (what, rc)
                got_dx = dx.check(c.dx.to(f32), what, exact=False)
            for i in range(nb):
                got = dWs[i].check(c.dW[i].to(f32), what, exact=False)
                worst["dw_tile"] = max(worst["dw_tile"], E.within(f"{what} dW[{i}]", got, c.dW[i], c.dW_bound[i], c.dW_sum[i]))
                dbs[i].check(c.dbias[i], f"{what} dbias[{i}]")
            worst["dx_batched"] = max(worst["dx_batched"], E.within(what + " dx", got_dx, c.dx, c.dx_bound, c.dx_sum))
    print("act_in 1, worst error in fp32 ulps of the sum of the addends' magnitudes (REL_SILU = 2^-20 is 8 .. 16 ulps): "
          + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    parity_log("edge_census.silu_ulps", **worst)


# ---- flow loss -----------------------------------------------------------------------------------------------------------
def run_flow_loss(lib, c, gscale, with_dout):
    B, per = c.B, c.per
    n_ws = lib.vds_flow_loss_workspace_floats(B, per)
    assert n_ws == B * E.flow_loss_bps(per)
    v, out = nan_in(c.v), nan_in(c.out)
    loss, ps, ws = blank(f32, 1), blank(f32, B), blank(f32, n_ws)
    dout = blank(bf16, B, per) if with_dout else Flat(None, "")
    rc = lib.vds_flow_loss(v.ptr, out.ptr, loss.ptr, ps.ptr, dout.ptr, gscale, B, per, ws.ptr, stream())
    assert rc == 0, rc
    what = f"flow_loss B {B} per {per} gscale {gscale}"
    got_ps = ps.check(c.per_sample.to(f32), what + " per_sample", exact=False)
    got_loss = loss.check(torch.zeros(1, dtype=f32), what + " loss", exact=False)
    ws.check(ws.initial, what + " workspace", exact=False)
    E.check_per_sample(what, got_ps, c.per_sample, c.per_exact)
    E.check_loss(what, got_loss[0], got_ps)
    share = None
    if with_dout:
        share = E.check_dout(what, dout.check(c.dout, what + " dout", exact=False), c.dout, c.und)
    return got_loss.clone(), got_ps.clone(), (dout.got().clone() if with_dout else None), share


@pytest.mark.parametrize("B,per", E.loss_plan())
def test_flow_loss(lib, B, per):
    gscale = 0.75 if per % 2 else 1.0
    c = E.loss_case(B, per, gscale)
    first = run_flow_loss(lib, c, gscale, True)
    again = run_flow_loss(lib, c, gscale, True)
    for a, b in zip(first[:3], again[:3]):
        assert torch.equal(G.bits(a), G.bits(b)), "two calls differ"
    nodout = run_flow_loss(lib, c, gscale, False)
    assert torch.equal(G.bits(nodout[0]), G.bits(first[0])) and torch.equal(G.bits(nodout[1]), G.bits(first[1]))
    print(f"flow_loss B {B} per {per} {E.loss_branches(per)}: undecided share of dout {first[3]:.2%}")


def run_flow_loss_frames(lib, c, gscale):
    B, C, T, HW, tps = c.B, c.C, c.T, c.HW, c.tps
    n_ws = lib.vds_flow_loss_frames_workspace_floats(B, c.F, c.n_f)
    assert n_ws == B * c.F * E.flow_loss_bps(c.n_f)
    v, out, w = nan_in(c.v), nan_in(c.out), nan_in(c.w)
    loss, ps, ws, dout = blank(f32, 1), blank(f32, B), blank(f32, n_ws), blank(bf16, B, C, T, HW)
    rc = lib.vds_flow_loss_frames(v.ptr, out.ptr, w.ptr, loss.ptr, ps.ptr, dout.ptr, gscale, B, C, T, HW, tps, ws.ptr, stream())
    assert rc == 0, rc
    what = f"flow_loss_frames B {B} C {C} T {T} HW {HW} tps {tps}"
    got_ps = ps.check(c.per_sample.to(f32), what + " per_sample", exact=False)
    got_loss = loss.check(torch.zeros(1, dtype=f32), what + " loss", exact=False)
    ws.check(ws.initial, what + " workspace", exact=False)
    E.check_per_sample(what, got_ps, c.per_sample, c.per_exact)
    E.check_loss(what, got_loss[0], got_ps)
    got_dout = dout.check(c.dout, what + " dout", exact=False)
    share = E.check_dout(what, got_dout, c.dout, c.und)
    return got_loss.clone(), got_ps.clone(), got_dout.clone(), share, (v, out, w)


@pytest.mark.parametrize("B,C,T,HW,tps", E.frames_plan())
def test_flow_loss_frames(lib, B, C, T, HW, tps):
    gscale = 0.75
    c = E.frame_loss_case(B, C, T, HW, tps, gscale)
    first = run_flow_loss_frames(lib, c, gscale)
    again = run_flow_loss_frames(lib, c, gscale)
    for a, b in zip(first[:3], again[:3]):
        assert torch.equal(G.bits(a), G.bits(b)), "two calls differ"
    zero = (c.w == 0)[:, None, :, None].expand(B, C, c.F, tps * HW).reshape(B, C, T, HW) | (c.w.sum(1) == 0)[:, None, None, None]
    assert (G.bits(first[2])[zero] == 0).all(), "a frame or sample without weight must get exact +0 gradients"
    if (C, T, HW, tps) in E.FRAMES_BWD:
        # the gradient-only path: partials == NULL, gloss read from the device; the bits of the forward call's dout
        v, out, w = first[4]
        gloss = nan_in(torch.tensor([gscale], dtype=f32))
        dout = blank(bf16, B, C, T, HW)
        rc = lib.vds_flow_loss_frames_bwd(v.ptr, out.ptr, w.ptr, gloss.ptr, dout.ptr, B, C, T, HW, tps, stream())
        assert rc == 0, rc
        dout.check(first[2], "flow_loss_frames_bwd against the forward call's dout")
    print(f"flow_loss_frames B {B} C {C} T {T} HW {HW} tps {tps} bps {E.flow_loss_bps(c.n_f)}: undecided share of dout {first[3]:.2%}")


@pytest.mark.parametrize("n", E.LOSS_BWD_N)
def test_flow_loss_bwd(lib, n):
    c = E.loss_bwd_case(n)
    v, out, gloss = nan_in(c.v), nan_in(c.out), nan_in(torch.tensor([c.gloss], dtype=f32))
    dout = blank(bf16, n)
    rc = lib.vds_flow_loss_bwd(v.ptr, out.ptr, gloss.ptr, dout.ptr, c.B, c.per, stream())
    assert rc == 0, rc
    what = f"flow_loss_bwd n {n} (workgroups, trips) {E.loss_bwd_blocks(n)}"
    share = E.check_dout(what, dout.check(c.dout, what, exact=False), c.dout, c.und)
    if n & (n - 1) == 0:
        assert share == 0.0
    print(f"{what}: undecided share {share:.2%}")


# ---- the exact movers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pt,p", E.PATCH_P)
def test_patches(lib, pt, p):
    for B, C, T, H, W, pt_, p_ in E.patch_plan():
        if (pt_, p_) != (pt, p):
            continue
        fwd, inv = E.patch_case(B, C, T, H, W, pt, p)
        n, feat = fwd.n, fwd.feat
        for lead, roff in E.PATCH_ROWS:
            rps = lead + n if lead else 0
            what = f"B {B} C {C} THW {(T, H, W)} pt {pt} p {p} rows_per_sample {rps} row_offset {roff}"
            # patchify: image in, token rows out (register rows keep the sentinel)
            img = nan_in(fwd.latent)
            rows = Flat(G.fill_value(bf16, "sentinel").repeat(B, lead + n, feat), "sentinel")
            if lead:
                rc = lib.vds_patchify_rows(img.ptr, rows.ptr, B, C, T, H, W, pt, p, rps, roff, stream())
            else:
                rc = lib.vds_patchify(img.ptr, rows.ptr, B, C, T, H, W, pt, p, stream())
            assert rc == 0, (what, rc)
            rows.check(E.rows_parent(fwd.tokens, lead, "sentinel"), "patchify " + what)
            # unpatchify: token rows in (register rows NaN), image out
            y = nan_in(E.rows_parent(inv.tokens, lead, "nan"))
            out = blank(bf16, B, C, T, H, W)
            if lead:
                rc = lib.vds_unpatchify_rows(y.ptr, out.ptr, B, C, T, H, W, pt, p, rps, roff, 0, stream())
            else:
                rc = lib.vds_unpatchify(y.ptr, out.ptr, B, C, T, H, W, pt, p, stream())
            assert rc == 0, (what, rc)
            out.check(inv.latent, "unpatchify " + what)
            # its backward: image gradient in, token-row gradient out
            dimg = nan_in(inv.latent)
            drows = Flat(G.fill_value(bf16, "sentinel").repeat(B, lead + n, feat), "sentinel")
            if lead:
                rc = lib.vds_unpatchify_rows(dimg.ptr, drows.ptr, B, C, T, H, W, pt, p, rps, roff, 1, stream())
            else:
                rc = lib.vds_unpatchify_bwd(dimg.ptr, drows.ptr, B, C, T, H, W, pt, p, stream())
            assert rc == 0, (what, rc)
            drows.check(E.rows_parent(inv.tokens, lead, "sentinel"), "unpatchify_bwd " + what)


def test_registers(lib):
    for B in E.REG_B:
        for R_, D in E.REG_RD:
            for bs in E.reg_strides(R_, D):
                c = E.reg_case(B, R_, D, bs)
                what = f"registers B {B} R {R_} D {D} batch_stride {bs}"
                reg = nan_in(c.reg)
                x = Flat(G.fill_value(bf16, "sentinel").repeat(B, bs), "sentinel")
                rc = lib.vds_fill_registers(reg.ptr, x.ptr, bs, B, R_, D, stream())
                assert rc == 0, (what, rc)
                x.check(c.want_x, "fill " + what)
                dx, dreg = nan_in(c.dx), Flat(c.dreg0, "sentinel")
                rc = lib.vds_registers_bwd(dx.ptr, bs, dreg.ptr, B, R_, D, stream())
                assert rc == 0, (what, rc)
                dreg.check(c.want_dreg, "bwd " + what)


def test_noise(lib):
    for B, per in E.NOISE:
        x, n, t, zt, v = E.noise_case(B, per)
        xd, nd, td = nan_in(x), nan_in(n), nan_in(t)
        z, vv = blank(bf16, B, per), blank(bf16, B, per)
        rc = lib.vds_noise_latents(xd.ptr, nd.ptr, td.ptr, z.ptr, vv.ptr, B, per, stream())
        assert rc == 0, rc
        z.check(zt, f"noise B {B} per {per} z_t")
        vv.check(v, f"noise B {B} per {per} v")
    for B, C, T, HW, tps in E.NOISE_FRAMES:
        x, n, t, zt, v = E.noise_frames_case(B, C, T, HW, tps)
        xd, nd, td = nan_in(x), nan_in(n), nan_in(t)
        z, vv = blank(bf16, B, C, T, HW), blank(bf16, B, C, T, HW)
        rc = lib.vds_noise_latents_frames(xd.ptr, nd.ptr, td.ptr, z.ptr, vv.ptr, B, C, T, HW, tps, stream())
        assert rc == 0, rc
        z.check(zt, f"noise frames B {B} tps {tps} z_t")
        vv.check(v, f"noise frames B {B} tps {tps} v")


def test_cfg_euler(lib):
    for n in E.EULER_N:
        for i, cfg in enumerate(E.EULER_CFG):
            for guided in (0, 1):
                dt = E.EULER_DT[i]
                cond, unc, acc0, acc1, lat = E.euler_case(n, cfg, dt, guided)
                what = f"cfg_euler n {n} cfg {cfg} dt {dt} guided {guided}"
                c, u, acc = nan_in(cond), nan_in(unc), Flat(acc0, "sentinel")
                out = blank(bf16, n)
                rc = lib.vds_cfg_euler_step(c.ptr, u.ptr, acc.ptr, out.ptr, cfg, dt, n, stream())
                assert rc == 0, (what, rc)
                acc.check(acc1, what + " acc")
                out.check(lat, what + " latents")


def test_casts(lib):
    for n in E.CAST_N:
        for off in (0, 1, 4):   # elements: both pointers 16-byte aligned; src off by 4 bytes and dst by 2; both by 16 and 8
            src = E.cast_values(n, off)
            s = nan_in(torch.cat([torch.zeros(off, dtype=f32), src]))
            d = blank(bf16, off + n)
            rc = lib.vds_cast_f32_bf16(s.ptr + 4 * off, d.ptr + 2 * off, n, stream())
            assert rc == 0, rc
            got = d.check(d.initial, f"cast n {n} off {off}", exact=False)
            assert (G.bits(got[:off]) == G.SENTINEL_BF16).all(), "the elements in front of an offset destination changed"
            E.assert_cast(f"cast f32 -> bf16 n {n} off {off}", got[off:], src)
    for n in (1, 255, 257, 65536):
        src = E.all_bf16()[-n:] if n < 65536 else E.all_bf16()
        s, d = Flat(src, "sentinel"), blank(f32, n)
        rc = lib.vds_cast_bf16_f32(s.ptr, d.ptr, n, stream())
        assert rc == 0, rc
        got = d.check(d.initial, f"cast bf16 -> f32 n {n}", exact=False)
        want = src.to(f32)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan) and torch.equal(G.bits(got)[~nan], G.bits(want)[~nan]), f"cast bf16 -> f32 n {n}"
        assert (G.bits(got)[nan] == (G.bits(src)[nan].to(torch.int32) << 16)).all(), "a NaN payload changed"


def test_rope_rows(lib):
    for nt, ns in E.ROPE_TABS:
        tabs = E.rope_tables(nt, ns)
        dev = [nan_in(t) for t in tabs]
        half = nt + 2 * ns
        for thw in E.ROPE_THW:
            t, h, w = thw
            for n_reg in E.ROPE_NREG:
                rows = n_reg + t * h * w
                for start in E.rope_starts(thw) + [E.ROPE_BAD_START]:
                    what = f"rope_rows tables {(nt, ns)} thw {thw} n_reg {n_reg} start {start}"
                    legal = E.rope_clamp(start, thw) == tuple(start)
                    cosb, sinb = blank(f32, rows, half), blank(f32, rows, half)
                    rc = lib.vds_rope_rows(dev[0].ptr, dev[1].ptr, dev[2].ptr, dev[3].ptr, nt, ns, t, h, w, *start, n_reg,
                                           cosb.ptr, sinb.ptr, stream())
                    wc, wsn = E.rope_expect(tabs, thw, E.rope_clamp(start, thw), n_reg)
                    if legal:
                        assert rc == 0, (what, rc)
                        cosb.check(wc, what + " cos")
                        sinb.check(wsn, what + " sin")
                    else:   # the host form refuses what the device form clamps
                        assert rc == VDS_ERR_ARG, (what, rc)
                        torch.cuda.synchronize()
                        cosb.untouched(what + " cos (refused)")
                        sinb.untouched(what + " sin (refused)")
                    sd = torch.tensor(start, dtype=torch.int32).cuda()
                    cosd, sind = blank(f32, rows, half), blank(f32, rows, half)
                    rc = lib.vds_rope_rows_dev(dev[0].ptr, dev[1].ptr, dev[2].ptr, dev[3].ptr, nt, ns, t, h, w, sd.data_ptr(), n_reg,
                                               cosd.ptr, sind.ptr, stream())
                    assert rc == 0, (what, rc)
                    cosd.check(wc, what + " cos (device offsets)")
                    sind.check(wsn, what + " sin (device offsets)")


# ---- timestep embedding ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", E.TEMB_D)
def test_timestep_embedding(lib, D):
    shares = []
    for B in E.TEMB_B:
        t, want, und = E.temb_case(B, D)
        what = f"timestep_embedding B {B} D {D}"
        td, out = nan_in(t), blank(f32, B, D)
        rc = lib.vds_timestep_embedding(td.ptr, out.ptr, B, D, stream())
        assert rc == 0, (what, rc)
        got = out.check(want, what, exact=False)
        assert torch.equal(got.to(bf16).to(f32), got), what + ": an output is no bf16 number"
        share = float(und.float().mean())
        assert share <= E.UNDECIDED_CAP, f"{what}: {share:.2%} undecided"
        diff = (G.bits(got) != G.bits(want)) & ~und
        if diff.any():
            b, j = (int(v) for v in diff.nonzero()[0])
            raise AssertionError(f"{what}: {int(diff.sum())} of {diff.numel()} decided elements differ, first at ({b}, {j}): "
                                 f"t {t[b].item()!r} got {got[b, j].item()!r} want {want[b, j].item()!r}")
        zero = t == 0
        assert (got[zero][:, :D // 2] == 1).all() and (G.bits(got[zero][:, D // 2:]) == 0).all(), what + ": t = 0"
        shares.append(share)
    print(f"timestep_embedding D {D}: undecided share {min(shares):.3%} .. {max(shares):.3%}")


# ---- return codes ----------------------------------------------------------------------------------------------------------
def test_refusals(lib):
    """VDS_ERR_ARG before any launch, and every output parent still holds its sentinel"""
    M, N, K = 4, 16, 16
    z32 = lambda *s: nan_in(torch.zeros(*s, dtype=f32))      # noqa: E731
    z16 = lambda *s: nan_in(torch.zeros(*s, dtype=bf16))     # noqa: E731
    x, W, bias, dy = z32(M, K + 8), z16(N, K + 8), z16(N + 8), z32(M, N + 8)
    y, dW, dbias, dx = blank(f32, M, N + 8), blank(f32, N, K + 8), blank(f32, N + 8), blank(f32, M, K + 8)
    outs = [(y, "y"), (dW, "dW"), (dbias, "dbias"), (dx, "dx")]
    s = stream()
    fwd = lambda x_=x.ptr, W_=W.ptr, b_=bias.ptr, y_=y.ptr, M_=M, N_=N, K_=K: \
        lib.vds_small_linear_fwd(x_, W_, b_, y_, M_, N_, K_, 0, s)                                  # noqa: E731
    bwd = lambda dy_=dy.ptr, x_=x.ptr, W_=W.ptr, dW_=dW.ptr, db_=dbias.ptr, dx_=dx.ptr, M_=M, N_=N, K_=K: \
        lib.vds_small_linear_bwd(dy_, x_, W_, dW_, db_, dx_, M_, N_, K_, 0, s)                      # noqa: E731
    wt, bt, dwt, dbt = table([W.ptr]), table([bias.ptr]), table([dW.ptr]), table([dbias.ptr])
    fwdb = lambda x_=x.ptr, y_=y.ptr, ys=M * N, nb=1, M_=M, N_=N, K_=K: \
        lib.vds_small_linear_fwd_batched(x_, wt.data_ptr(), bt.data_ptr(), y_, ys, nb, M_, N_, K_, 0, s)   # noqa: E731
    bwdb = lambda dy_=dy.ptr, x_=x.ptr, wt_=wt.data_ptr(), dx_=dx.ptr, nb=1, M_=M, N_=N, K_=K: \
        lib.vds_small_linear_bwd_batched(dy_, M * N, x_, wt_, dwt.data_ptr(), dbt.data_ptr(), dx_, nb, M_, N_, K_, 0, s)   # noqa: E731
    refused = {
        "fwd M 0": fwd(M_=0), "fwd N 0": fwd(N_=0), "fwd K 0": fwd(K_=0), "fwd K 12": fwd(K_=12), "fwd N -1": fwd(N_=-1),
        "fwd x + 4 bytes": fwd(x_=x.ptr + 4), "fwd W + 2 bytes": fwd(W_=W.ptr + 2), "fwd W + 8 bytes": fwd(W_=W.ptr + 8),
        "fwd y + 4 bytes": fwd(y_=y.ptr + 4), "fwd bias + 2 bytes": fwd(b_=bias.ptr + 2), "fwd bias + 4 bytes": fwd(b_=bias.ptr + 4),
        "bwd M 0": bwd(M_=0), "bwd N 0": bwd(N_=0), "bwd K 0": bwd(K_=0), "bwd K 12": bwd(K_=12),
        "bwd dx without W": bwd(W_=None), "bwd x + 8 bytes": bwd(x_=x.ptr + 8), "bwd W + 2 bytes": bwd(W_=W.ptr + 2),
        "bwd dW + 4 bytes": bwd(dW_=dW.ptr + 4), "bwd dy + 2 bytes": bwd(dy_=dy.ptr + 2), "bwd dx + 2 bytes": bwd(dx_=dx.ptr + 2),
        "bwd dbias + 2 bytes": bwd(db_=dbias.ptr + 2),
        "fwd batched nb 0": fwdb(nb=0), "fwd batched M 17": fwdb(M_=17), "fwd batched N 0": fwdb(N_=0), "fwd batched K 0": fwdb(K_=0),
        "fwd batched x + 4 bytes": fwdb(x_=x.ptr + 4), "fwd batched y + 8 bytes": fwdb(y_=y.ptr + 8),
        "fwd batched y_stride 66": fwdb(ys=66),
        "bwd batched nb 0": bwdb(nb=0), "bwd batched M 0": bwdb(M_=0), "bwd batched N 0": bwdb(N_=0), "bwd batched K 4": bwdb(K_=4),
        "bwd batched dx without W": bwdb(wt_=None), "bwd batched x + 4 bytes": bwdb(x_=x.ptr + 4),
        "bwd batched dy + 2 bytes": bwdb(dy_=dy.ptr + 2), "bwd batched dx + 2 bytes": bwdb(dx_=dx.ptr + 2),
    }
    # timestep embedding, registers, noising
    t, emb = z32(8), blank(f32, 4, 16)
    outs.append((emb, "timestep embedding"))
    for B, D in ((0, 16), (-1, 16), (4, 0), (4, 15), (4, -2)):
        refused[f"timestep_embedding B {B} D {D}"] = lib.vds_timestep_embedding(t.ptr, emb.ptr, B, D, s)
    reg, xr, dreg = z16(3 * 8), blank(bf16, 2, 40), blank(f32, 3 * 8)
    outs += [(xr, "fill_registers x"), (dreg, "registers_bwd dreg")]
    for B, R_, D, bs in ((0, 3, 8, 40), (2, 0, 8, 40), (2, 3, 0, 40), (2, 3, -8, 40), (2, 3, 8, 23)):
        refused[f"fill_registers {(B, R_, D, bs)}"] = lib.vds_fill_registers(reg.ptr, xr.ptr, bs, B, R_, D, s)
        refused[f"registers_bwd {(B, R_, D, bs)}"] = lib.vds_registers_bwd(xr.ptr, bs, dreg.ptr, B, R_, D, s)
    lat, zt, vv = z16(2, 64), blank(bf16, 2, 64), blank(bf16, 2, 64)
    outs += [(zt, "noise z_t"), (vv, "noise v")]
    for B, per in ((0, 64), (2, 0), (-2, 64), (2, -64)):
        refused[f"noise_latents B {B} per {per}"] = lib.vds_noise_latents(lat.ptr, lat.ptr, t.ptr, zt.ptr, vv.ptr, B, per, s)
    # patchify_rows: sizes the patch does not divide, non-positive sizes
    img, rows = z16(1, 2, 4, 6, 6), blank(bf16, 64, 64)
    outs.append((rows, "patchify rows"))
    for T, H, Wd, pt, p in ((3, 6, 6, 2, 2), (4, 5, 6, 2, 2), (4, 6, 5, 2, 2), (4, 6, 6, 0, 2), (4, 6, 6, 2, 0), (0, 6, 6, 2, 2)):
        refused[f"patchify_rows THW {(T, H, Wd)} pt {pt} p {p}"] = lib.vds_patchify_rows(img.ptr, rows.ptr, 1, 2, T, H, Wd, pt, p, 0, 0, s)
    refused["patchify_rows B 0"] = lib.vds_patchify_rows(img.ptr, rows.ptr, 0, 2, 4, 6, 6, 2, 2, 0, 0, s)
    refused["patchify_rows C 0"] = lib.vds_patchify_rows(img.ptr, rows.ptr, 1, 0, 4, 6, 6, 2, 2, 0, 0, s)
    refused["unpatchify_rows pt 0"] = lib.vds_unpatchify_rows(img.ptr, rows.ptr, 1, 2, 4, 6, 6, 0, 2, 0, 0, 0, s)
    refused["unpatchify_rows B 0"] = lib.vds_unpatchify_rows(img.ptr, rows.ptr, 0, 2, 4, 6, 6, 2, 2, 0, 0, 1, s)
    # flow_loss_bwd and the Euler step: 16-byte operands
    v, gl, dout = z16(64 + 8), z32(1), blank(bf16, 64 + 8)
    outs.append((dout, "flow_loss_bwd dout"))
    lb = lambda v_=v.ptr, o_=v.ptr, d_=dout.ptr, B=2, per=32: lib.vds_flow_loss_bwd(v_, o_, gl.ptr, d_, B, per, s)   # noqa: E731
    refused.update({"flow_loss_bwd v + 2 bytes": lb(v_=v.ptr + 2), "flow_loss_bwd out + 8 bytes": lb(o_=v.ptr + 8),
                    "flow_loss_bwd dout + 4 bytes": lb(d_=dout.ptr + 4), "flow_loss_bwd B 0": lb(B=0), "flow_loss_bwd per 0": lb(per=0),
                    "flow_loss_bwd n % 8": lb(per=30), "flow_loss_bwd B -2 per -32": lb(B=-2, per=-32)})
    acc, latn = blank(f32, 64 + 8), blank(bf16, 64 + 8)
    outs += [(acc, "cfg_euler acc"), (latn, "cfg_euler latents")]
    eu = lambda c_=v.ptr, u_=v.ptr, a_=acc.ptr, l_=latn.ptr, n=64: lib.vds_cfg_euler_step(c_, u_, a_, l_, 3.0, 0.5, n, s)   # noqa: E731
    refused.update({"cfg_euler cond + 2 bytes": eu(c_=v.ptr + 2), "cfg_euler uncond + 8 bytes": eu(u_=v.ptr + 8),
                    "cfg_euler acc + 4 bytes": eu(a_=acc.ptr + 4), "cfg_euler latents + 2 bytes": eu(l_=latn.ptr + 2),
                    "cfg_euler n 0": eu(n=0), "cfg_euler n 60": eu(n=60)})
    cast_dst = blank(bf16, 16)
    outs.append((cast_dst, "cast dst"))
    refused["cast_f32_bf16 n -1"] = lib.vds_cast_f32_bf16(x.ptr, cast_dst.ptr, -1, s)
    refused["cast_f32_bf16 src + 2 bytes"] = lib.vds_cast_f32_bf16(x.ptr + 2, cast_dst.ptr, 8, s)
    refused["cast_f32_bf16 dst + 1 byte"] = lib.vds_cast_f32_bf16(x.ptr, cast_dst.ptr + 1, 8, s)
    torch.cuda.synchronize()
    wrong = {k: rc for k, rc in refused.items() if rc != VDS_ERR_ARG}
    assert not wrong, f"not refused with VDS_ERR_ARG: {wrong}"
    for o, name in outs:
        o.untouched("refused calls: " + name)
    assert lib.vds_cast_f32_bf16(x.ptr, cast_dst.ptr, 0, s) == 0      # n = 0 stays a no-op, not an error
    cast_dst.untouched("cast n 0")

