"""The low-rank adapter kernels (csrc/lowrank.hip) on the GPU: every entry point and layout bit for bit against the
restatement of tests/helpers/lora_ref.py on exact inputs (every output element has ONE right bit pattern there), on the
smallest shapes at which each kernel can go wrong -- rows below / at / past the 16-row MFMA tile, the 64-row wave pair and
the 128-row workgroup, widths below / past the 32-wide k step, the 64-column group and the 128-column slab, one width
past each kernel's LDS chunk, and for the weight gradient one full M chunk, one chunk + 1 row and several chunks with a
short last one -- with dense operands and with every operand and output a window of a NaN- / sentinel-filled parent whose
guard bands must come back intact; every call runs twice and must repeat its bits.  One Gaussian case per kernel is
compared with fp32 torch by relative norm at the bound tests/test_kernels_gpu.py uses for the bf16 GEMM (4e-3)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lora_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
SENT_BF16 = torch.tensor([0xBEEF - 0x10000], dtype=torch.int16).view(bf16).item()      # -0.4668: no case produces it
SENT_F32 = torch.tensor([0xDEADBEEF - 0x100000000], dtype=torch.int32).view(f32).item()
GEMM_BOUND = 4e-3  # tests/test_kernels_gpu.py: bf16 GEMM on Gaussian operands

MS = (1, 15, 17, 64, 65, 257)
WIDTHS = (32, 96, 160, 384)
RL = [(r, lay) for r in LR.RANKS for lay in (0, 1)]
_WORST = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def _report(parity_log):
    yield
    if _WORST:
        parity_log("test_lora_kernels_gpu.gaussian_rel", **_WORST)


def same_bits(a, b):
    it = torch.int16 if a.dtype == bf16 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def place(t, windowed, fill):
    """the tensor on the GPU, dense or as a window of a `fill`-filled parent: (parent on the GPU | None, view, window)"""
    if not windowed:
        d = t.cuda()
        return None, d, None
    parent, win = LR.windowed(t, fill)
    parent = parent.cuda()
    return parent, LR.window_of(parent, win), win


def check_bands(parent, win, fill, what):
    if parent is not None:
        assert LR.bands_intact(parent.cpu(), win, fill), f"{what}: a guard band was written"


def test_chunk_sizes_are_the_restated_ones(ops):
    for r in LR.RANKS:
        assert ops.lowrank_chunk("down", r) == LR.down_chunk(r) and ops.lowrank_chunk("up", r) == LR.up_chunk(r)
        assert ops.lowrank_chunk("wgrad", r) == LR.WGRAD_CHUNK


@pytest.mark.parametrize("windowed", [False, True], ids=["dense", "window"])
@pytest.mark.parametrize("r,layout", RL)
def test_down_exact(ops, r, layout, windowed):
    kc = LR.down_chunk(r)
    shapes = [(M, K) for M in MS for K in WIDTHS] + [(65, kc + 32), (17, kc + 8), (33, 2 * kc + 40), (130, 8)]
    for M, K in shapes:
        c = LR.exact_case("down", M, K, r, layout, scale=0.5)
        px, x, wx = place(c["x"], windowed, NAN)
        pw, w, ww = place(c["w"], windowed, NAN)
        outs = []
        for _ in range(2):
            pu, u, wu = place(torch.full((M, r), SENT_BF16, dtype=bf16), windowed, SENT_BF16)
            got = ops.lowrank_down(x, w, 0.5, layout, out=u)
            assert got is u
            check_bands(pu, wu, SENT_BF16, f"down u M={M} K={K}")
            outs.append(u.cpu())
        assert same_bits(outs[0], c["expect"]), (M, K, r, layout, (outs[0].float() - c["expect"].float()).abs().max())
        assert same_bits(outs[0], outs[1]), ("run to run", M, K)
        check_bands(px, wx, NAN, "down x"), check_bands(pw, ww, NAN, "down w")


@pytest.mark.parametrize("windowed", [False, True], ids=["dense", "window"])
@pytest.mark.parametrize("r,layout", RL)
def test_up_add_exact(ops, r, layout, windowed):
    nc = LR.up_chunk(r)
    shapes = [(M, N) for M in MS for N in WIDTHS] + [(65, nc + 8), (17, 2 * nc + 72), (130, 8)]
    for M, N in shapes:
        c = LR.exact_case("up_add", M, N, r, layout, scale=0.5)
        pu, u, wu = place(c["u"], windowed, NAN)
        pw, w, ww = place(c["w"], windowed, NAN)
        outs = []
        for _ in range(2):
            py, y, wy = place(c["y"], windowed, SENT_BF16)
            assert ops.lowrank_up_add(u, w, y, 0.5, layout) is y
            check_bands(py, wy, SENT_BF16, f"up_add y M={M} N={N}")
            outs.append(y.cpu())
        assert same_bits(outs[0], c["expect"]), (M, N, r, layout, (outs[0].float() - c["expect"].float()).abs().max())
        assert same_bits(outs[0], outs[1]), ("run to run", M, N)
        check_bands(pu, wu, NAN, "up_add u"), check_bands(pw, ww, NAN, "up_add w")


@pytest.mark.parametrize("windowed", [False, True], ids=["dense", "window"])
@pytest.mark.parametrize("r,layout", RL)
def test_wgrad_exact(ops, r, layout, windowed):
    """accumulates onto a non-zero g; M: the row list plus one full chunk, one chunk + 1 row, two chunks and a short one"""
    C = LR.WGRAD_CHUNK
    shapes = [(M, N) for M in MS for N in WIDTHS] + [(C, 32), (C + 1, 96), (2 * C + 100, 160), (130, 8)]
    for M, N in shapes:
        c = LR.exact_case("wgrad", M, N, r, layout, scale=0.5)
        pa, a, wa = place(c["a"], windowed, NAN)
        pu, u, wu = place(c["u"], windowed, NAN)
        outs = []
        for _ in range(2):
            pg, g, wg = place(c["g"], windowed, SENT_F32)
            ops.lowrank_wgrad(a, u, g, 0.5, layout)
            check_bands(pg, wg, SENT_F32, f"wgrad g M={M} N={N}")
            outs.append(g.cpu())
        assert same_bits(outs[0], c["expect"]), (M, N, r, layout, (outs[0] - c["expect"]).abs().max())
        assert same_bits(outs[0], outs[1]), ("run to run", M, N)
        check_bands(pa, wa, NAN, "wgrad a"), check_bands(pu, wu, NAN, "wgrad u")
    # a caller's workspace of exactly the stated size, poisoned: every partial the reduction reads was written
    M, N = C + 1, 96
    c = LR.exact_case("wgrad", M, N, r, layout, scale=0.5)
    from video_diffusion_speedrun_amd import _lib
    need = int(_lib.load().vds_lowrank_wgrad_workspace_floats(M, N, r))
    ws = torch.full((need + 64,), NAN, dtype=f32, device="cuda")
    g = c["g"].cuda()
    ops.lowrank_wgrad(c["a"].cuda(), c["u"].cuda(), g, 0.5, layout, ws=ws[:need])
    assert same_bits(g.cpu(), c["expect"]) and torch.isnan(ws[need:]).all()


def test_exact_results_do_not_depend_on_the_determinism_mode(ops, request):
    c = LR.exact_case("wgrad", 2 * LR.WGRAD_CHUNK + 100, 160, 32, 0, scale=0.5)
    d = LR.exact_case("down", 257, 384, 32, 1, scale=0.5)
    res = []
    for det in (False, True):
        if det:
            ops.set_deterministic(True, 1 << 24)
            request.addfinalizer(lambda: ops.set_deterministic(False))
        g = c["g"].cuda()
        ops.lowrank_wgrad(c["a"].cuda(), c["u"].cuda(), g, 0.5, 0)
        u = ops.lowrank_down(d["x"].cuda(), d["w"].cuda(), 0.5, 1)
        res.append((g.cpu(), u.cpu()))
    ops.set_deterministic(False)
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1])
    assert same_bits(res[0][0], c["expect"]) and same_bits(res[0][1], d["expect"])


def _rel(a, b):
    a, b = a.to(f64).cpu().flatten(), b.to(f64).cpu().flatten()
    return ((a - b).norm() / b.norm()).item()


def _randn(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(bf16)


def test_gaussian_operands_against_fp32_torch(ops):
    """one Gaussian case per kernel (ragged M, K past a chunk, both layouts between them) by relative norm"""
    M, K, N, r = 1000, 1152, 1160, 32
    x, A = _randn(M, K, seed=1), _randn(r, K, seed=2, scale=0.05)
    u = ops.lowrank_down(x.cuda(), A.cuda(), 0.5, 0)
    u_ref = 0.5 * (x.float() @ A.float().t())
    _WORST["down"] = _rel(u, u_ref)
    assert _WORST["down"] <= GEMM_BOUND, _WORST
    Bm, y = _randn(r, N, seed=3, scale=0.3), _randn(M, N, seed=4)
    uu = u.cpu()
    got = ops.lowrank_up_add(uu.cuda(), Bm.cuda(), y.clone().cuda(), 2.0, 1)
    y_ref = y.float() + 2.0 * (uu.float() @ Bm.float())
    _WORST["up_add"] = _rel(got, y_ref)
    assert _WORST["up_add"] <= GEMM_BOUND, _WORST
    a = _randn(2 * LR.WGRAD_CHUNK + 904, N, seed=5)
    v = _randn(a.shape[0], r, seed=6)
    g0 = torch.randn(N, r, generator=torch.Generator().manual_seed(7))
    g = g0.clone().cuda()
    ops.lowrank_wgrad(a.cuda(), v.cuda(), g, 0.25, 0)
    g_ref = g0.double() + 0.25 * (a.double().t() @ v.double())
    _WORST["wgrad"] = _rel(g, g_ref)
    assert _WORST["wgrad"] <= GEMM_BOUND, _WORST
