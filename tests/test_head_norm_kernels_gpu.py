"""vds_head_rmsnorm_fwd / _bwd on the GPU (csrc/headnorm.hip).

Bit for bit on the exact inputs of tests/helpers/head_norm_ref.py -- dense and as the left column window of a parent twice
as wide (the form of ckv[:, :D]) -- inside NaN-sentinel-filled parents whose other bytes, and a guard band around rstd, must
come back intact; every call twice with equal bits, in both determinism modes.  Gaussian inputs per element against the
float64 restatement:
  forward   |out - ref| <= 2^-8 |ref| (1 + 2^-10)   bf16's unit roundoff plus fp32 noise;  rstd to 2^-22 relative
  backward  |out - ref| <= 2^-8 |ref| + 1e-5 r (|g| + |y| |mean(g y)|)   (DESIGN.md 14's bound), from the stored y and r
  radial    |sum_d dx y| <= 2^-7 sum_d |dx y|
  zero row  output 0, r = rsqrt(eps), gradient r g
Shapes: M x H x hd below -- tails in the head rows per workgroup (64) and in its chunk trips."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import head_norm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
MS, HS, HDS = (1, 3, 4, 5, 63, 65, 257), (1, 2, 3, 16), (24, 32, 64, 72, 96, 128)
SENT16, SENT32 = 0x7FB1, 0x7FA00001  # NaN bit patterns no kernel produces
GUARD = 64                           # elements of sentinel in front of and behind every buffer


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import _lib, ops
    return dict(ops=ops, lib=_lib.load(), check=_lib.check)


def parent16(rows, ld):
    """a sentinel-filled bf16 buffer and its [rows, ld] interior"""
    flat = torch.full((GUARD + rows * ld + GUARD,), SENT16, dtype=torch.int16, device="cuda")
    return flat, flat[GUARD:GUARD + rows * ld].view(bf16).view(rows, ld)


def placed(t, wide):
    """t [M, N] bf16 (CPU) as a device window: dense (ld = N) or the left columns of a parent twice as wide.
    -> (flat int16 buffer, window)"""
    M, N = t.shape
    flat, par = parent16(M, 2 * N if wide else N)
    win = par[:, :N]
    win.copy_(t.cuda())
    return flat, win


def outside_intact(flat, M, N, wide):
    """every element of the buffer that is not in the window still holds the sentinel"""
    ld = 2 * N if wide else N
    body = flat[GUARD:GUARD + M * ld].view(M, ld)
    ok = bool((flat[:GUARD] == SENT16).all()) and bool((flat[GUARD + M * ld:] == SENT16).all())
    return ok and (not wide or bool((body[:, N:] == SENT16).all()))


def guarded_f32(n):
    flat = torch.full((GUARD + n + GUARD,), SENT32, dtype=torch.int32, device="cuda")
    return flat, flat[GUARD:GUARD + n].view(f32)


def f32_guards_intact(flat, n):
    return bool((flat[:GUARD] == SENT32).all()) and bool((flat[GUARD + n:] == SENT32).all())


def fwd(vds, win, rstd, H, hd, eps=R.EPS):
    M = win.shape[0]
    vds["check"](vds["lib"].vds_head_rmsnorm_fwd(win.data_ptr(), win.stride(0), rstd.data_ptr(), M, H, hd, eps,
                                                 torch.cuda.current_stream().cuda_stream), "vds_head_rmsnorm_fwd")


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


def modes(vds):
    """both determinism modes, restored to off"""
    for on in (False, True):
        if on:
            vds["ops"].set_deterministic(True, 1 << 20)
        try:
            yield on
        finally:
            if on:
                vds["ops"].set_deterministic(False)


@pytest.mark.parametrize("hd", HDS)
def test_exact_inputs_bit_for_bit(vds, hd):
    ops = vds["ops"]
    cases = [(M, H, wide) + R.exact_forward(M, H, hd) + R.exact_backward(M, H, hd, (M + H) % 7 - 3)
             for M in MS for H in HS for wide in (False, True)]
    worst_r = 0.0
    for on in modes(vds):
        for M, H, wide, x, want, r, dy, y, rs, dwant in cases:
            tag = (hd, M, H, wide, on)
            N = H * hd
            # forward
            got = []
            for _ in range(2):
                flat, win = placed(x, wide)
                rflat, rstd = guarded_f32(M * H)
                fwd(vds, win, rstd, H, hd)
                torch.cuda.synchronize()
                assert outside_intact(flat, M, N, wide) and f32_guards_intact(rflat, M * H), tag
                got.append((bits(win).cpu(), bits(rstd).cpu(), rstd.cpu()))
            assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), tag
            assert torch.equal(got[0][0], bits(want)), tag
            e = ((got[0][2].to(f64).view(M, H) - r).abs() / r).max().item()
            worst_r = max(worst_r, e)
            # backward (y in the same form as dy; rstd through the wrapper)
            outs = []
            for _ in range(2):
                flat, win = placed(dy, wide)
                yflat, ywin = placed(y, wide)
                assert ops.head_rmsnorm_bwd(win, ywin, rs.cuda(), H, hd) is win
                torch.cuda.synchronize()
                assert outside_intact(flat, M, N, wide), tag
                assert outside_intact(yflat, M, N, wide) and torch.equal(bits(ywin).cpu(), bits(y)), tag  # y is read only
                outs.append(bits(win).cpu())
            assert torch.equal(outs[0], outs[1]), tag
            assert torch.equal(outs[0], bits(dwant)), tag
    print(f"hd{hd}: rstd on the exact inputs, worst relative error {worst_r:.3e} (2^-22 = {2.0 ** -22:.3e})")
    assert worst_r <= 2.0 ** -22


_gauss = {}


def gauss_case(M, H, hd):
    """Gaussian rows at row scales over 2^-6 .. 2^6, with zero rows (rows m H + h = 1 mod 5), and a Gaussian gradient"""
    key = (M, H, hd)
    if key not in _gauss:
        g = torch.Generator().manual_seed(100000 * hd + 100 * M + H)
        scale = 2.0 ** (torch.rand(M, H, 1, generator=g) * 12 - 6)
        x = torch.randn(M, H, hd, generator=g) * scale
        zero = (torch.arange(M * H) % 5 == 1).reshape(M, H)
        x[zero] = 0
        dy = torch.randn(M, H * hd, generator=g).to(bf16)
        _gauss[key] = (x.reshape(M, H * hd).to(bf16), dy, zero)
    return _gauss[key]


@pytest.mark.parametrize("hd", HDS)
def test_gaussian_inputs_per_element_against_float64(vds, hd):
    ops = vds["ops"]
    worst = dict(fwd=0.0, rstd=0.0, bwd=0.0, radial=0.0)
    for M in MS:
        for H in HS:
            tag = (hd, M, H)
            x, dy, zero = gauss_case(M, H, hd)
            ref, r = R.forward_ref(x, H, hd)
            _, win = placed(x, True)  # the ckv form
            rstd = ops.head_rmsnorm_fwd(win, H, hd)
            assert rstd.dtype == f32 and tuple(rstd.shape) == (M, H)
            y, rs = win.cpu().contiguous(), rstd.cpu()
            err = (y.to(f64) - ref).abs()
            bound = 2.0 ** -8 * ref.abs() * (1 + 2.0 ** -10)
            worst["fwd"] = max(worst["fwd"], (err / bound.clamp(min=1e-300)).max().item())
            e_r = ((rs.to(f64) - r).abs() / r).max().item()
            worst["rstd"] = max(worst["rstd"], e_r)
            assert torch.all(err <= bound), (tag, (err - bound).max().item())
            assert e_r <= 2.0 ** -22, (tag, e_r)
            # backward from the stored rows and the stored r, both layouts of y
            dref, scale = R.backward_ref(dy, y, rs, H, hd)
            _, dwin = placed(dy, False)
            ops.head_rmsnorm_bwd(dwin, win, rstd, H, hd)
            dx = dwin.cpu().to(f64)
            derr = (dx - dref).abs()
            dbound = 2.0 ** -8 * dref.abs() + 1e-5 * scale
            worst["bwd"] = max(worst["bwd"], (derr / dbound.clamp(min=1e-300)).max().item())
            assert torch.all(derr <= dbound), (tag, (derr - dbound).max().item())
            prod = (dx * y.to(f64)).reshape(M, H, hd)
            radial, total = prod.sum(-1).abs(), prod.abs().sum(-1)
            worst["radial"] = max(worst["radial"], (radial / total.clamp(min=1e-300)).max().item())
            assert torch.all(radial <= 2.0 ** -7 * total), tag
            if zero.any():  # zero rows: output 0, r = rsqrt(eps), the finite gradient r g
                yz, gz = y.reshape(M, H, hd)[zero], dy.to(f64).reshape(M, H, hd)[zero]
                assert torch.equal(yz, torch.zeros_like(yz)), tag
                assert torch.all((rs[zero].to(f64) - 1000.0).abs() <= 1000.0 * 2.0 ** -22), tag
                dz = dx.reshape(M, H, hd)[zero]
                assert torch.isfinite(dz).all() and float(dz.abs().max()) > 0
                assert torch.all((dz - rs[zero].to(f64)[:, None] * gz).abs() <= 2.0 ** -8 * (rs[zero].to(f64)[:, None] * gz).abs()), tag
    print(f"hd{hd}: worst fraction of the bound: forward {worst['fwd']:.3f}, backward {worst['bwd']:.3f}; rstd relative "
          f"{worst['rstd']:.3e} (2^-22 = {2.0 ** -22:.3e}); radial / sum|terms| {worst['radial']:.3e} (2^-7 = {2.0 ** -7:.3e})")


def test_windows_of_the_model(vds):
    """the two calls of a block: a contiguous qc [B L, D] and the k columns of ckv [B Lc, 2 D]; v stays what it was"""
    ops = vds["ops"]
    H, hd = 2, 72
    D = H * hd
    g = torch.Generator().manual_seed(9)
    ckv = torch.randn(48, 2 * D, generator=g).to(bf16).cuda()
    v_before = ckv[:, D:].clone()
    k_ref, r = R.forward_ref(ckv[:, :D].cpu(), H, hd)
    rstd = ops.head_rmsnorm_fwd(ckv[:, :D], H, hd)
    assert torch.equal(ckv[:, D:], v_before)
    assert torch.all((ckv[:, :D].cpu().to(f64) - k_ref).abs() <= 2.0 ** -8 * k_ref.abs() * (1 + 2.0 ** -10))
    assert tuple(rstd.shape) == (48, H)
    dckv = torch.randn(48, 2 * D, generator=g).to(bf16).cuda()
    dv_before = dckv[:, D:].clone()
    ops.head_rmsnorm_bwd(dckv[:, :D], ckv[:, :D], rstd, H, hd)
    assert torch.equal(dckv[:, D:], dv_before)
