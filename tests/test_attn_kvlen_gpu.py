"""Per-sample key counts in the attention kernels (vds_attn_fwd_kvlen / vds_attn_bwd_kvlen) against fp32 torch on the
CPU: scores of keys >= n masked with -inf, o = softmax . v, lse = logsumexp, gradients by autograd; a sample with n == 0
is zeros by definition.  Tolerances are those of tests/test_kernels_gpu.py for the same quantities (relative Frobenius
error: o 6e-3, lse 1e-3, dq / dk / dv 8e-3).  Every output buffer starts as NaN: whatever the library is said to write,
it has to write."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16, f32 = torch.bfloat16, torch.float32
TOL_O, TOL_LSE, TOL_G = 6e-3, 1e-3, 8e-3


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import ops as _ops
    return _ops


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def close(name, got, ref, tol):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    e = rel(got, ref)
    print(f"{name}: rel {e:.3e} (bound {tol:.1e})")
    assert e < tol, f"{name}: rel {e:.3e} >= {tol:.1e}"


def gen(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(bf16)


def heads(t2d, B, L, H, hd, off=0):
    """[B*L, ld] token-major rows -> [B,H,L,hd] (CPU copy of what ops.heads_view addresses)"""
    return t2d[:, off:off + H * hd].reshape(B, L, H, hd).permute(0, 2, 1, 3)


_inputs = {}
_refs = {}


def inputs(hd, B, H, Lq, Lk):
    key = (hd, B, H, Lq, Lk)
    if key not in _inputs:
        D = H * hd
        _inputs[key] = (gen(B * Lq, D, seed=101), gen(B * Lk, 2 * D, seed=102), gen(B * Lq, D, seed=103))
    return _inputs[key]


def masked_ref(hd, B, H, Lq, Lk, lens):
    """fp32 reference (computed once per case, shared, never modified): o, lse, dq, dk, dv as [B,H,L,hd] / [B,H,Lq]"""
    key = (hd, B, H, Lq, Lk, tuple(lens))
    if key in _refs:
        return _refs[key]
    qb, kvb, dob = inputs(hd, B, H, Lq, Lk)
    D = H * hd
    q = heads(qb, B, Lq, H, hd).float().requires_grad_(True)
    k = heads(kvb, B, Lk, H, hd, 0).float().requires_grad_(True)
    v = heads(kvb, B, Lk, H, hd, D).float().requires_grad_(True)
    do = heads(dob, B, Lq, H, hd).float()
    s = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
    n = torch.tensor(lens).view(B, 1, 1, 1)
    s = s.masked_fill(torch.arange(Lk).view(1, 1, 1, Lk) >= n, float("-inf"))
    live = [b for b in range(B) if lens[b] > 0]
    o = torch.zeros(B, H, Lq, hd)
    lse = torch.zeros(B, H, Lq)
    if live:
        ol = torch.softmax(s[live], dim=-1) @ v[live]
        ol.backward(do[live])
        o[live] = ol.detach()
        lse[live] = torch.logsumexp(s[live].detach(), dim=-1)
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    _refs[key] = (o, lse, z(q), z(k), z(v))
    return _refs[key]


def run(ops, hd, B, H, Lq, Lk, lens, pad_ones=0, legacy_ws=False, bwd=True):
    """the library on token-major q / o / do and a [B*Lk, 2D] kv buffer; lens = None: the calls without lengths.
    Returns CPU tensors o, lse, dq, dk, dv laid out like the reference."""
    qb, kvb, dob = inputs(hd, B, H, Lq, Lk)
    D = H * hd
    qd, kvd, dod = qb.cuda(), kvb.cuda(), dob.cuda()
    nan = float("nan")
    o = torch.full((B * Lq, D), nan, dtype=bf16, device="cuda")
    lse = torch.full((B, H, Lq), nan, dtype=f32, device="cuda")
    kvl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    qv, ov = ops.heads_view(qd, B, Lq, H, hd), ops.heads_view(o, B, Lq, H, hd)
    if pad_ones:
        kp, vp = ops.kv_pad_ones(kvd, B, Lk, H, hd, 96, 0, D)
        kk, vv = kp[..., :hd], vp[..., :hd]
    else:
        kk, vv = ops.heads_view(kvd, B, Lk, H, hd, 0), ops.heads_view(kvd, B, Lk, H, hd, D)
    ops.attn_fwd(qv, kk, vv, ov, lse, kv_pad_ones=pad_ones, kv_lens=kvl)
    out = [heads(o.cpu(), B, Lq, H, hd), lse.cpu()]
    if bwd:
        dqb = torch.full_like(qd, nan)
        dkvb = torch.full_like(kvd, nan)
        delta = torch.full((2, B, H, Lq), nan, dtype=f32, device="cuda") if legacy_ws else None
        ops.attn_bwd(qv, kk, vv, ov, lse, ops.heads_view(dod, B, Lq, H, hd), ops.heads_view(dqb, B, Lq, H, hd),
                     ops.heads_view(dkvb, B, Lk, H, hd, 0), ops.heads_view(dkvb, B, Lk, H, hd, D), delta,
                     kv_pad_ones=pad_ones, kv_lens=kvl)
        dkv = dkvb.cpu()
        out += [heads(dqb.cpu(), B, Lq, H, hd), heads(dkv, B, Lk, H, hd, 0), heads(dkv, B, Lk, H, hd, D)]
    torch.cuda.synchronize()
    return out


def check(tag, got, ref, lens, bwd=True):
    names = ["o", "lse", "dq", "dk", "dv"][:len(got)]
    for name, g in zip(names, got):
        assert torch.isfinite(g.float()).all(), f"{tag}.{name}: an element was left unwritten or is not finite"
    live = [b for b, n in enumerate(lens) if n > 0]
    close(f"{tag}.o", got[0], ref[0], TOL_O)
    if live:
        close(f"{tag}.lse", got[1][live], ref[1][live], TOL_LSE)
    for b, n in enumerate(lens):
        if n == 0:
            assert got[0][b].float().abs().max().item() == 0, f"{tag}.o[{b}]: no context must give exact zeros"
            assert got[1][b].abs().max().item() == 0, f"{tag}.lse[{b}]: no context must give lse = 0"
    if not bwd:
        return
    close(f"{tag}.dq", got[2], ref[2], TOL_G)
    close(f"{tag}.dk", got[3], ref[3], TOL_G)
    close(f"{tag}.dv", got[4], ref[4], TOL_G)
    for b, n in enumerate(lens):
        if n < got[3].shape[2]:
            assert got[3][b, :, n:].float().abs().max().item() == 0, f"{tag}.dk[{b}]: rows >= {n} must be exact zeros"
            assert got[4][b, :, n:].float().abs().max().item() == 0, f"{tag}.dv[{b}]: rows >= {n} must be exact zeros"
        if n == 0:
            assert got[2][b].float().abs().max().item() == 0, f"{tag}.dq[{b}]: no context must give exact zeros"


HEAD_DIMS = [32, 64, 72, 96, 128]
SMALL = dict(B=5, H=2, Lq=130, Lk=200)  # B*H = 10 crosses the 8-head grouping of the workgroup order
SMALL_LENS = [200, 128, 65, 1, 0]


@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_plain_kernels_small_case(ops, hd, order):
    """plain forward, dQ and dK/dV kernels of every instance: a full sample, a tile boundary (128), a ragged tile (65), one
    key and none; reversed to catch a wrong sample index"""
    lens = SMALL_LENS if order == "forward" else SMALL_LENS[::-1]
    got = run(ops, hd, lens=lens, **SMALL)
    check(f"small.hd{hd}.{order}", got, masked_ref(hd, lens=lens, **SMALL), lens)


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_full_lengths_match_the_call_without_lengths(ops, hd):
    lens = [SMALL["Lk"]] * SMALL["B"]
    got = run(ops, hd, lens=lens, **SMALL)
    plain = run(ops, hd, lens=None, **SMALL)
    check(f"full.hd{hd}", got, masked_ref(hd, lens=lens, **SMALL), lens)
    for name, g, p, tol in zip(["o", "lse", "dq", "dk", "dv"], got, plain, [TOL_O, TOL_LSE, TOL_G, TOL_G, TOL_G]):
        close(f"full.hd{hd}.{name}_vs_plain", g, p, tol)


@pytest.mark.parametrize("dkv16", [None, 2], ids=["dkv_default", "dkv16_forced"])
def test_ones_column_cross_path(ops, dkv16):
    """kv_pad_ones = 2, head_dim 72.  Lq = 2112 >= 2048 is the `p.Lq >= 2048` rule of run_fwd in csrc/attention.hip: from
    there on the forward runs on a 64-queries-per-wave ones-column kernel.  With the library's defaults (attn_mfma16 = 7,
    attn_delta_fold = 1) that is attn_fwd16_kernel, and the dQ pass is attn_bwd_dq16_kernel with the folded preprocess;
    test_ones_column_kernel_variants runs the other ones-column instances.  dK/dV once as the library chooses and once
    on the 16x16x32 cross kernel, forced for this small grid the way test_attention_cross_on_the_ones_column_kernels
    forces it."""
    shape = dict(B=2, H=2, Lq=2112, Lk=300)
    lens = [300, 70]
    prev = None if dkv16 is None else ops.knob_set("cross_dkv16", dkv16)
    try:
        got = run(ops, 72, lens=lens, pad_ones=2, **shape)
    finally:
        if prev is not None:
            ops.knob_set("cross_dkv16", prev)
    check(f"xones.{dkv16}", got, masked_ref(72, lens=lens, **shape), lens)


@pytest.mark.parametrize("variant,fold", [(0, 1), (7, 0), (7, 1)], ids=["mfma32", "all16_separate_delta", "all16_folded_delta"])
def test_ones_column_kernel_variants(ops, variant, fold):
    """every ones-column instance a kv_pad_ones = 2 call can be switched to, with a sample without keys among the others:
    mask 0 -> attn_fwd_wide_kernel<96, 80, true> and attn_bwd_dq_kernel<96, 80, true> (32x32x16); mask 7 without the
    folded preprocess -> attn_fwd16_kernel, attn_delta_*_kernel and attn_bwd_dq16_kernel<96, false>; mask 7 with it (the
    default) -> attn_bwd_dq16_kernel<96, true>, whose statistics of the keyless sample stay unwritten"""
    shape = dict(B=3, H=2, Lq=2112, Lk=300)
    lens = [70, 0, 300]
    prev_v = ops.attn_set_variant(variant)
    prev_f = ops.knob_set("attn_delta_fold", fold)
    try:
        got = run(ops, 72, lens=lens, pad_ones=2, **shape)
    finally:
        ops.attn_set_variant(prev_v)
        ops.knob_set("attn_delta_fold", prev_f)
    check(f"xones.variant{variant}.fold{fold}", got, masked_ref(72, lens=lens, **shape), lens)


@pytest.mark.parametrize("legacy_ws", [False, True], ids=["split", "unsplit"])
@pytest.mark.parametrize("B,lens", [(1, [129]), (2, [300, 0])], ids=["B1_129", "B2_300_0"])
def test_query_split_dkv(ops, B, lens, legacy_ws):
    """hd72_Lk300 of test_attention_cross_dkv_with_split_query_range: with the workspace the library asks for the dK/dV
    launch splits the query range (fp32 partials + dkv_reduce_kernel); with the legacy [2,B,H,Lq] workspace it does not"""
    shape = dict(B=B, H=2, Lq=2100, Lk=300)
    assert ops.attn_bwd_workspace_floats(B, 2, 2100, 300, 72) > 2 * B * 2 * 2100  # the library wants room for partials here
    got = run(ops, 72, lens=lens, legacy_ws=legacy_ws, **shape)
    check(f"qsplit.B{B}.{'unsplit' if legacy_ws else 'split'}", got, masked_ref(72, lens=lens, **shape), lens)


def test_graph_replay_reads_the_lengths_on_the_device(ops):
    """capture attn_fwd with a device kv_lens, change the tensor's contents, replay: the output is that of the new lengths"""
    hd = 64
    B, H, Lq, Lk = SMALL["B"], SMALL["H"], SMALL["Lq"], SMALL["Lk"]
    qb, kvb, _ = inputs(hd, B, H, Lq, Lk)
    D = H * hd
    qd, kvd = qb.cuda(), kvb.cuda()
    o = torch.full((B * Lq, D), float("nan"), dtype=bf16, device="cuda")
    lse = torch.full((B, H, Lq), float("nan"), dtype=f32, device="cuda")
    kvl = torch.tensor(SMALL_LENS, dtype=torch.int32, device="cuda")
    args = (ops.heads_view(qd, B, Lq, H, hd), ops.heads_view(kvd, B, Lk, H, hd, 0), ops.heads_view(kvd, B, Lk, H, hd, D),
            ops.heads_view(o, B, Lq, H, hd), lse)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attn_fwd(*args, kv_lens=kvl)  # warm-up outside the capture (first-launch attribute calls)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ops.attn_fwd(*args, kv_lens=kvl)
    new = SMALL_LENS[::-1]
    kvl.copy_(torch.tensor(new, dtype=torch.int32))
    o.fill_(float("nan"))
    lse.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    check("graph", [heads(o.cpu(), B, Lq, H, hd), lse.cpu()], masked_ref(hd, B, H, Lq, Lk, lens=new), new, bwd=False)


def test_kv_lens_argument_checks(ops):
    hd, B, H, Lq, Lk = 64, 2, 2, 16, 16
    D = H * hd
    q = torch.zeros(B * Lq, D, dtype=bf16, device="cuda")
    kv = torch.zeros(B * Lk, 2 * D, dtype=bf16, device="cuda")
    o, lse = torch.zeros_like(q), torch.zeros(B, H, Lq, dtype=f32, device="cuda")
    args = (ops.heads_view(q, B, Lq, H, hd), ops.heads_view(kv, B, Lk, H, hd, 0), ops.heads_view(kv, B, Lk, H, hd, D),
            ops.heads_view(o, B, Lq, H, hd), lse)
    for bad in ([16, 16], torch.tensor([16, 16], dtype=torch.int32), torch.tensor([16, 16], device="cuda"),
                torch.zeros(3, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")[::2]):
        with pytest.raises(ValueError):
            ops.attn_fwd(*args, kv_lens=bad)
