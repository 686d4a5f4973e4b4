"""Per-frame timesteps on the GPU: the grouped modulation kernels (vds_*_grouped) against the per-sample kernels run on
the gathered rows of every (sample, group) -- bit for bit where the arithmetic per row is the same -- and against float64
sums of the same bf16 inputs for the column sums; noising and the frame-weighted loss against tests/helpers/
frame_timesteps_ref.py; the model with timesteps [B, t] against the per-sample path (constant rows) and against the helper
reference (rows that differ); recomputation, graph replay, a sharded model, the sampler's conditioning frames, the fp8
refusal.  A [B, t] call always computes its modulation with the per-block linears (never the batched adaLN launch), so the
model tests below run the path every real shape takes.

Bounds.  Column sums (dmod, dw, dbias), per element: |err| <= (n + 4) 2^-24 sum|terms|, n = rows summed -- the fp32 summation
bound plus the few roundings inside each term.  Loss: 1e-5 relative against float64 (reordered fp32 sums over <= 6144 terms).
Model against the helper reference: the bounds of smoke() (output 2.5e-2, loss 1e-2, worst gradient 3e-2), with the two
references (per-frame / every frame at the row maximum) shown to be >= 5 x each bound apart first."""
import os
import sys

import pytest
import torch

from oracle import dit_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_timesteps_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
CONST = ["patch_proj", "context_kv", "positional_embedding"]
EPS24 = 2.0 ** -24


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import model, ops, optim, sampling, train
    return dict(model=model, ops=ops, optim=optim, train=train, sampling=sampling)


@pytest.fixture
def deterministic(vds, request):
    vds["ops"].set_deterministic(True, 256 << 20)
    request.addfinalizer(lambda: vds["ops"].set_deterministic(False))


def rel(a, b):
    a, b = a.float().cpu().flatten(), b.float().cpu().flatten()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


# --------------------------------------------------------------------------------------- kernels ----
# (B, lead, period, rows per frame): L = lead + period * rows
CASES = {
    "b2_p3_r25": (2, 16, 3, 25),   # odd sizes, more than one wave round per group
    "b1_p1_r7": (1, 16, 1, 7),     # one frame group
    "b3_p8_r1": (3, 16, 8, 1),     # one row per frame group: fewer rows than waves
    "b2_lead0": (2, 0, 4, 16),     # empty group 0: its dmod row must stay as passed in
}
POISON = 12345.0


class Knobs:
    def __init__(self, ops, knobs):
        self.ops, self.knobs, self.prev = ops, knobs, {}

    def __enter__(self):
        for k, v in self.knobs.items():
            self.prev[k] = self.ops.knob_set(k, v)

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            self.ops.knob_set(k, v)


_inputs = {}


def inputs(case, D):
    """CPU tensors of a (case, D), made once and never modified.  The modulation table has 4 D columns: shift at 0, scale
    (and the gate) at 2 D, so that columns D .. 2D-1 and 3D .. 4D-1 belong to no call."""
    if (case, D) in _inputs:
        return _inputs[(case, D)]
    B, lead, period, rpf = CASES[case]
    L, G = lead + period * rpf, 1 + period
    g = torch.Generator().manual_seed(100 * D + 7 * L + B)
    d = dict(B=B, L=L, G=G, lead=lead, period=period, D=D,
             x=(torch.randn(B * L, D, generator=g) * 1.5).to(bf16), dy=torch.randn(B * L, D, generator=g).to(bf16),
             dres=torch.randn(B * L, D, generator=g).to(bf16), y=torch.randn(B * L, D, generator=g).to(bf16),
             w=(1 + 0.25 * torch.randn(D, generator=g)).to(bf16), mod=torch.randn(B * G, 4 * D, generator=g) * 0.5)
    gidx = R.group_index(L, lead, period)
    d["rows"] = {(b, gg): (b * L + torch.nonzero(gidx == gg).flatten()) for b in range(B) for gg in range(G)}
    d["mrow"] = torch.cat([b * G + gidx for b in range(B)])  # the modulation row of every token row
    _inputs[(case, D)] = d
    return d


def dmod_init(d):
    """zeros where a call accumulates, POISON where it must not write: the unused columns and the rows of empty groups"""
    D = d["D"]
    t = torch.full((d["B"] * d["G"], 4 * D), POISON)
    for (b, gg), rows in d["rows"].items():
        if len(rows):
            t[b * d["G"] + gg, 0:D] = 0
            t[b * d["G"] + gg, 2 * D:3 * D] = 0
    return t


@pytest.mark.parametrize("has_w", [False, True], ids=["no_w", "w"])
# every instance the forward dispatcher can pick: one row per wave with 1, 2, 3 chunks per lane (D = 144; 768 and 1152 with the
# four-rows-per-wave form switched off) and four rows per wave at its three widths (D = 384, 768, 1152)
@pytest.mark.parametrize("D,knobs", [(144, {}), (384, {}), (768, {}), (768, {"rmsnorm_q4": 0}), (1152, {}),
                                     (1152, {"rmsnorm_q4": 0})],
                         ids=["d144", "d384_q4", "d768_q4", "d768_rows", "d1152_q4", "d1152_rows"])
@pytest.mark.parametrize("case", list(CASES))
def test_forward_norm_is_the_per_sample_kernel_on_gathered_rows(vds, case, D, knobs, has_w):
    ops, d = vds["ops"], inputs(case, D)
    B, L, grp = d["B"], d["L"], (d["lead"], d["period"])
    x, mod = d["x"].cuda(), d["mod"].cuda()
    w = d["w"].cuda() if has_w else None
    with Knobs(ops, knobs):
        y, rstd = ops.rmsnorm_mod_fwd_grouped(x, w, mod, 0, 2 * D, B, L, grp)
        torch.cuda.synchronize()
        for (b, gg), rows in d["rows"].items():
            if not len(rows):
                continue
            r = rows.cuda()
            m1 = mod[b * d["G"] + gg:b * d["G"] + gg + 1]
            y1, rstd1 = ops.rmsnorm_mod_fwd(x[r].contiguous(), w, m1, 0, 2 * D, 1, len(rows))
            assert torch.equal(bits(y[r]), bits(y1)), (b, gg)
            assert torch.equal(bits(rstd[r]), bits(rstd1)), (b, gg)
    assert torch.isfinite(y.float()).all()


def _sum_bound(terms, n):
    """float64 [n, D] terms -> (sum, (n + 4) 2^-24 sum|terms|) per column"""
    return terms.sum(0), (n + 4) * EPS24 * terms.abs().sum(0)


def _check_sum(got, terms, n, what):
    ref, bound = _sum_bound(terms, n)
    err = (got.double().cpu() - ref).abs()
    assert torch.all(err <= bound + 1e-30), (what, float((err / (bound + 1e-30)).max()))
    return float((err / (bound + 1e-30)).max())


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("has_w,has_res", [(False, False), (True, True)], ids=["plain", "w_dres"])
@pytest.mark.parametrize("D", [144, 768, 1152])  # 1, 2, 3 chunks per lane
@pytest.mark.parametrize("case", list(CASES))
def test_backward_norm(vds, case, D, has_w, has_res, det, request):
    ops, d = vds["ops"], inputs(case, D)
    if det:
        ops.set_deterministic(True, 256 << 20)
        request.addfinalizer(lambda: ops.set_deterministic(False))
    B, L, G, grp = d["B"], d["L"], d["G"], (d["lead"], d["period"])
    x, dy, mod = d["x"].cuda(), d["dy"].cuda(), d["mod"].cuda()
    w = d["w"].cuda() if has_w else None
    dres = d["dres"].cuda() if has_res else None
    _, rstd = ops.rmsnorm_mod_fwd_grouped(x, w, mod, 0, 2 * D, B, L, grp)

    def run():
        dmod = dmod_init(d).cuda()
        dw = torch.zeros(D, dtype=f32, device="cuda") if has_w else None
        dx = ops.rmsnorm_mod_bwd_grouped(dy, x, w, mod, 0, 2 * D, rstd, dres, dmod, dw, B, L, grp)
        torch.cuda.synchronize()
        return dx, dmod, dw

    dx, dmod, dw = run()
    # dx: the per-sample kernel on the gathered rows of every (sample, group)
    for (b, gg), rows in d["rows"].items():
        if not len(rows):
            continue
        r = rows.cuda()
        m1 = mod[b * G + gg:b * G + gg + 1]
        dm1 = torch.zeros(1, 4 * D, dtype=f32, device="cuda")
        dw1 = torch.zeros(D, dtype=f32, device="cuda") if has_w else None
        dx1 = ops.rmsnorm_mod_bwd(dy[r].contiguous(), x[r].contiguous(), w, m1, 0, 2 * D, rstd[r].contiguous(),
                                  dres[r].contiguous() if has_res else None, dm1, dw1, 1, len(rows))
        assert torch.equal(bits(dx[r]), bits(dx1)), (b, gg)
    # column sums against float64 sums of the same inputs (xhat = x * rstd with the kernel's own rstd)
    xhat = d["x"].double() * rstd.double().cpu()[:, None]
    dyd = d["dy"].double()
    wd = d["w"].double() if has_w else torch.ones(D, dtype=f64)
    worst = 0.0
    for (b, gg), rows in d["rows"].items():
        row = dmod[b * G + gg].cpu()
        if not len(rows):
            assert torch.all(row == POISON), (b, gg)  # an empty group's row: as it was passed in
            continue
        worst = max(worst, _check_sum(row[0:D], dyd[rows], len(rows), ("dshift", b, gg)))
        worst = max(worst, _check_sum(row[2 * D:3 * D], (dyd * xhat * wd)[rows], len(rows), ("dscale", b, gg)))
        assert torch.all(row[D:2 * D] == POISON) and torch.all(row[3 * D:] == POISON), (b, gg)  # columns of no call
    if has_w:
        sc1 = 1.0 + d["mod"].double()[d["mrow"], 2 * D:3 * D]
        worst = max(worst, _check_sum(dw, dyd * sc1 * xhat, B * L, "dw"))
    print(f"{case} D={D} w={has_w} det={det}: worst |err| / bound = {worst:.3f}")
    if det:
        dx2, dmod2, dw2 = run()
        assert torch.equal(bits(dx), bits(dx2)) and torch.equal(bits(dmod), bits(dmod2))
        assert dw is None or torch.equal(bits(dw), bits(dw2))


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("has_bias", [False, True], ids=["no_dbias", "dbias"])
@pytest.mark.parametrize("D", [144, 768, 1152])
@pytest.mark.parametrize("case", list(CASES))
def test_gate_backward(vds, case, D, has_bias, det, request):
    ops, d = vds["ops"], inputs(case, D)
    if det:
        ops.set_deterministic(True, 256 << 20)
        request.addfinalizer(lambda: ops.set_deterministic(False))
    B, L, G, grp = d["B"], d["L"], d["G"], (d["lead"], d["period"])
    dxn, y, mod = d["dy"].cuda(), d["y"].cuda(), d["mod"].cuda()
    gate_col = 2 * D

    def run():
        dmod = dmod_init(d).cuda()
        dmod[:, 0:D] = POISON  # only the gate columns belong to this call
        dbias = torch.zeros(D, dtype=f32, device="cuda") if has_bias else None
        dyo = ops.gate_bwd_grouped(dxn, y, mod, gate_col, dmod, dbias, B, L, grp)
        torch.cuda.synchronize()
        return dyo, dmod, dbias

    dyo, dmod, dbias = run()
    for (b, gg), rows in d["rows"].items():
        if not len(rows):
            continue
        r = rows.cuda()
        dm1 = torch.zeros(1, 4 * D, dtype=f32, device="cuda")
        dy1 = ops.gate_bwd(dxn[r].contiguous(), y[r].contiguous(), mod[b * G + gg:b * G + gg + 1], gate_col, dm1, None, 1,
                           len(rows))
        assert torch.equal(bits(dyo[r]), bits(dy1)), (b, gg)
    dd, yd = d["dy"].double(), d["y"].double()
    worst = 0.0
    for (b, gg), rows in d["rows"].items():
        row = dmod[b * G + gg].cpu()
        if not len(rows):
            assert torch.all(row == POISON), (b, gg)
            continue
        worst = max(worst, _check_sum(row[2 * D:3 * D], (dd * yd)[rows], len(rows), ("dgate", b, gg)))
        assert torch.all(row[0:2 * D] == POISON) and torch.all(row[3 * D:] == POISON), (b, gg)
    if has_bias:
        gate = d["mod"].double()[d["mrow"], 2 * D:3 * D]
        worst = max(worst, _check_sum(dbias, dd * gate, B * L, "dbias"))
    print(f"{case} D={D} dbias={has_bias} det={det}: worst |err| / bound = {worst:.3f}")
    if det:
        dy2, dmod2, dbias2 = run()
        assert torch.equal(bits(dyo), bits(dy2)) and torch.equal(bits(dmod), bits(dmod2))
        assert dbias is None or torch.equal(bits(dbias), bits(dbias2))


@pytest.mark.parametrize("want_y", [True, False], ids=["two_outputs", "xnew_only"])
@pytest.mark.parametrize("tile", [128, 256, 2, 0])
@pytest.mark.parametrize("N", [144, 1152])
@pytest.mark.parametrize("case", list(CASES))
def test_grouped_gate_res_gemm_equals_the_expanded_gate_table(vds, case, N, tile, want_y, request):
    """against vds_gemm_bf16 with rows_per_batch = 1 and the gate expanded to one f32 row per output row"""
    ops, d = vds["ops"], inputs(case, N)
    from video_diffusion_speedrun_amd._lib import EPI_GATE_RES, VDS_NT
    B, L, grp = d["B"], d["L"], (d["lead"], d["period"])
    M, K = B * L, 256
    g = torch.Generator().manual_seed(31 * M + N)
    a = torch.randn(M, K, generator=g).to(bf16).cuda()
    W = (torch.randn(N, K, generator=g) / 16).to(bf16).cuda()
    bias = torch.randn(N, generator=g).to(bf16).cuda()
    res, mod = d["x"].cuda(), d["mod"].cuda()
    gate_col = 2 * N
    expanded = mod[d["mrow"].cuda(), gate_col:gate_col + N].contiguous()
    prev = ops.gemm_force_tile(tile)
    request.addfinalizer(lambda: ops.gemm_force_tile(prev))
    y, xn = ops.linear_fwd_gate_res_grouped(a, W, bias, mod, gate_col, res, L, grp, want_y=want_y)
    y_ref = torch.empty(M, N, dtype=bf16, device="cuda") if want_y else None
    xn_ref = torch.empty(M, N, dtype=bf16, device="cuda")
    ops.gemm(VDS_NT, EPI_GATE_RES, M, N, K, a, K, W, K, y_ref, N, xn_ref, N, bias=bias, aux=res, ldaux=res.stride(0),
             gate=expanded, ldgate=N, rows_per_batch=1)
    torch.cuda.synchronize()
    assert torch.equal(bits(xn), bits(xn_ref))
    assert (y is None) == (not want_y) and (y is None or torch.equal(bits(y), bits(y_ref)))
    assert torch.isfinite(xn.float()).all() and not torch.equal(bits(xn), bits(res))


def test_grouped_calls_without_a_description_are_the_per_sample_calls(vds):
    """groups == NULL forwards: same bits as vds_rmsnorm_mod_fwd / vds_gemm_bf16"""
    import ctypes as C
    from video_diffusion_speedrun_amd import _lib
    ops, d = vds["ops"], inputs("b2_p3_r25", 144)
    B, L, D = d["B"], d["L"], 144
    x, mod = d["x"].cuda(), d["mod"][:B].contiguous().cuda()
    y0, r0 = ops.rmsnorm_mod_fwd(x, None, mod, 0, 2 * D, B, L)
    y1, r1 = torch.empty_like(y0), torch.empty_like(r0)
    ops.check(_lib.load().vds_rmsnorm_mod_fwd_grouped(x.data_ptr(), D, None, mod.data_ptr(), mod.stride(0), 0, 2 * D,
                                                      y1.data_ptr(), D, r1.data_ptr(), B, L, D, 1e-6, None, None), "fwd")
    torch.cuda.synchronize()
    assert torch.equal(bits(y0), bits(y1)) and torch.equal(bits(r0), bits(r1))


# -------------------------------------------------------------------------------- noising / loss ----
def test_noising_per_frame_is_exact(vds):
    ops = vds["ops"]
    g = torch.Generator().manual_seed(9)
    x, n = (torch.randn(3, 5, 6, 7, 3, generator=g).to(bf16) for _ in range(2))  # odd C, H, W; T = 6, time patch 2
    t = torch.rand(3, 3, generator=g).to(bf16)
    t[0, 0], t[1, 2] = 0.0, 1.0
    zt_ref, v_ref = R.noise_frames(x, n, t, 2)
    zt, v = ops.noise_latents_frames(x.cuda(), n.cuda(), t.float().cuda(), 2)
    assert torch.equal(bits(zt.cpu()), bits(zt_ref)) and torch.equal(bits(v.cpu()), bits(v_ref))
    assert torch.equal(zt.cpu()[0, :, 0:2], x[0, :, 0:2]) and torch.equal(zt.cpu()[1, :, 4:6], n[1, :, 4:6])
    # constant rows: the per-sample kernel
    tb = torch.tensor([0.25, 0.5, 0.875])
    zt0, v0 = ops.noise_latents(x.cuda(), n.cuda(), tb.cuda())
    zt1, v1 = ops.noise_latents_frames(x.cuda(), n.cuda(), tb[:, None].expand(3, 3).contiguous().cuda(), 2)
    assert torch.equal(bits(zt0), bits(zt1)) and torch.equal(bits(v0), bits(v1))
    # time patch 1 and 3: the frame index follows the latent frame
    for pt in (1, 3):
        tt = torch.rand(3, 6 // pt, generator=g).to(bf16)
        ref = R.noise_frames(x, n, tt, pt)[0]
        assert torch.equal(bits(ops.noise_latents_frames(x.cuda(), n.cuda(), tt.float().cuda(), pt)[0].cpu()), bits(ref))


def test_weighted_loss_and_its_gradient(vds):
    ops, train = vds["ops"], vds["train"]
    g = torch.Generator().manual_seed(10)
    B, C, T, H, W, pt = 3, 16, 6, 8, 8, 2  # n_f = 2048 elements per token-frame, 6144 per sample
    v, out = (torch.randn(B, C, T, H, W, generator=g).to(bf16) for _ in range(2))
    w = torch.tensor([[0.0, 0.0, 0.0], [0.0, 2.0, 0.5], [1.0, 1.0, 1.0]])
    o = out.float().requires_grad_(True)
    loss_ref, per_ref, _ = R.frame_loss(v, o, w, pt)
    loss_ref.backward()
    vc, oc, wc = v.cuda(), out.cuda(), w.cuda()
    loss, per, dout = ops.flow_loss_frames(vc, oc, wc, pt, want_grad=True)
    torch.cuda.synchronize()
    print("weighted loss", loss.item(), "ref", loss_ref.item(), "per", per.tolist())
    assert abs(loss.item() - loss_ref.item()) <= 1e-5 * abs(loss_ref.item())
    assert torch.all((per.double().cpu() - per_ref.detach()).abs() <= 1e-5 * per_ref.detach().abs())
    assert per[0].item() == 0.0 and torch.all(bits(dout[0]) == 0)      # no weight: zero loss, exactly zero gradient
    assert torch.all(bits(dout[1, :, 0:2]) == 0)                      # a weightless frame of a weighted sample
    gref = o.grad
    assert torch.all((dout.float().cpu() - gref).abs() <= 2.0 ** -8 * gref.abs() + 1e-12)  # one bf16 rounding
    # run to run: the same bits
    loss2, per2, dout2 = ops.flow_loss_frames(vc, oc, wc, pt, want_grad=True)
    assert torch.equal(bits(loss.reshape(1)), bits(loss2.reshape(1))) and torch.equal(bits(per), bits(per2))
    assert torch.equal(bits(dout), bits(dout2))
    # w = 1: today's loss up to summation order
    l1, p1, _ = ops.flow_loss_frames(vc, oc, torch.ones(B, 3, device="cuda"), pt, want_grad=False)
    l0, p0, _ = ops.flow_loss(vc, oc, want_grad=False)
    assert abs(l1.item() - l0.item()) <= 1e-5 * l0.item() and torch.allclose(p1, p0, rtol=1e-5, atol=0)
    # the autograd node: the upstream scalar is honoured (read from device memory)
    og = oc.clone().requires_grad_(True)
    lt, _ = train.frame_flow_loss(og, vc, wc, pt)
    (lt * 3.0).backward()
    assert torch.all((og.grad.float().cpu() - 3.0 * gref).abs() <= 2.0 ** -8 * (3.0 * gref).abs() + 1e-12)
    assert torch.all(bits(og.grad[0]) == 0)


# ----------------------------------------------------------------------------------------- model ----
def build(vds, cfg, P, mode="none", **kw):
    m = vds["model"].DiT(in_channels=cfg.in_channels, patch_size=cfg.patch_size, time_patch_size=cfg.time_patch_size,
                         hidden_size=cfg.hidden_size, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
                         cross_attn_input_size=cfg.cross_attn_input_size, residual_v=cfg.residual_v,
                         train_bias_and_rms=cfg.train_bias_and_rms, **kw)
    m.load_state_dict(P, strict=True)
    return m.to("cuda").enable_recompute(mode)


TS = [[0.0, 0.5, 0.96875], [0.9375, 0.25, 0.0625]]
START = (2, 3, 4)
_cases = {}


def model_case(name):
    """cfg, parameters (both time_embed weights x 8: without that the model barely depends on t) and inputs: latent
    [2,16,6,8,8] with (pt, p) = (2, 2), so t = 3 and L = 64; context [2,24,64]"""
    if name in _cases:
        return _cases[name]
    if name == "hd72":
        cfg = O.DiTConfig(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=144, depth=2, num_heads=2,
                          cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False)
        seed = 3
    else:
        cfg = O.DiTConfig(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=128, depth=3, num_heads=2,
                          cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False)
        seed = 13
    P = O.init_params(cfg, seed=seed, randomize_zero_init=True, init_std_factor=1.0)
    P["time_embed.0.weight"] = P["time_embed.0.weight"] * 8
    P["time_embed.2.weight"] = P["time_embed.2.weight"] * 8
    g = torch.Generator().manual_seed(seed + 1)
    latent = torch.randn(2, 16, 6, 8, 8, generator=g).to(bf16)
    ctx = torch.randn(2, 24, 64, generator=g).to(bf16)
    noise = torch.randn(2, 16, 6, 8, 8, generator=g).to(bf16)
    _cases[name] = (cfg, P, latent, ctx, noise)
    return _cases[name]


_refs = {}


def reference_step(name, rowmax):
    """one fp32 step of the helper reference, once per (case, rowmax): rowmax = every frame at its sample's largest
    timestep (what a model that ignored the per-frame levels would compute), the same noised input and weights"""
    if (name, rowmax) in _refs:
        return _refs[(name, rowmax)]
    cfg, P, latent, ctx, noise = model_case(name)
    ts = torch.tensor(TS).to(bf16)
    w = (ts > 0).float()
    zt, v = R.noise_frames(latent, noise, ts, cfg.time_patch_size)
    tm = ts.max(dim=1, keepdim=True).values.expand(2, 3) if rowmax else ts
    Pg = {k: p.clone().requires_grad_(True) for k, p in P.items()}
    out = R.dit_forward(Pg, cfg, zt.float(), ctx.float(), tm.float(), START)
    loss, _, _ = R.frame_loss(v, out, w, cfg.time_patch_size)
    loss.backward()
    res = dict(out=out.detach(), loss=loss.item(), zt=zt, v=v, ts=ts, w=w,
               grads={k: p.grad for k, p in Pg.items() if p.grad is not None})
    _refs[(name, rowmax)] = res
    return res


def step(vds, m, zt, v, ctx, ts, w, pt, **kw):
    m.zero_grad()
    out = m(zt.cuda(), ctx.cuda(), ts.cuda(), rope_start=START, **kw)
    if w is None:
        loss, _ = vds["train"].flow_loss(out, v.cuda())
    else:
        loss, _ = vds["train"].frame_flow_loss(out, v.cuda(), w.cuda(), pt)
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().clone(), loss.item(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("kw", [{}, {"qk_norm": True, "context_lens": [24, 7]}], ids=["plain", "qk_norm_context_lens"])
def test_constant_rows_equal_the_per_sample_path(vds, kw):
    """timesteps[:, None].expand(B, t) against timesteps: the same output bits, gradients equal up to reordered sums"""
    cfg, P, latent, ctx, noise = model_case("hd72")
    kw = dict(kw)
    lens = kw.pop("context_lens", None)
    fkw = {} if lens is None else {"context_lens": lens}
    t = torch.tensor([0.75, 0.1875]).to(bf16)
    zt, v = O.noise_latents(latent, noise, t)
    m = build(vds, cfg, P, **kw)
    out0, loss0, g0 = step(vds, m, zt, v, ctx, t, None, 2, **fkw)
    out1, loss1, g1 = step(vds, m, zt, v, ctx, t[:, None].expand(2, 3).contiguous(), None, 2, **fkw)
    assert torch.equal(bits(out0), bits(out1))
    worst = max((rel(g1[k], g0[k]), k) for k in g0 if float(g0[k].abs().max()) > 0)
    print("constant rows: worst gradient rel", worst)
    assert worst[0] <= 2e-4, worst
    for k in g0:
        if float(g0[k].abs().max()) == 0:
            assert float(g1[k].abs().max()) == 0, k
    # and a [B, t] call with the no-grad forward gives the same bits again
    with torch.no_grad():
        out2 = m(zt.cuda(), ctx.cuda(), t[:, None].expand(2, 3).contiguous().cuda(), rope_start=START, **fkw)
    assert torch.equal(bits(out2), bits(out0))
    for bad in (torch.zeros(2, 2), torch.zeros(2, 6), torch.zeros(3)):
        with pytest.raises(ValueError, match=r"\[2, 3\]"):
            m(zt.cuda(), ctx.cuda(), bad.cuda(), rope_start=START)


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_model_step_against_the_helper_reference(vds, name, parity_log):
    cfg, P, latent, ctx, noise = model_case(name)
    ref, flat = reference_step(name, False), reference_step(name, True)
    B_OUT, B_LOSS, B_GRAD = 2.5e-2, 1e-2, 3e-2
    # discrimination, on the CPU references alone: a model that conditioned every frame on the row maximum is >= 5 x
    # each bound away, on the output and on the block gradients named below
    d_out = rel(flat["out"], ref["out"])
    keys = [k for k in ref["grads"] if k.startswith("blocks.") and
            k.endswith(("qkv.weight", "mlp.0.weight", "cross_proj.weight", "adaLN_modulation.1.weight"))]
    d_grad = min((rel(flat["grads"][k], ref["grads"][k]), k) for k in keys)
    print(f"{name}: per-frame vs row-maximum reference: out {d_out:.3f}, closest gradient {d_grad}")
    assert d_out >= 5 * B_OUT and d_grad[0] >= 5 * B_GRAD, (d_out, d_grad)
    m = build(vds, cfg, P)
    zt, v = vds["ops"].noise_latents_frames(latent.cuda(), noise.cuda(), ref["ts"].float().cuda(), cfg.time_patch_size)
    assert torch.equal(bits(zt.cpu()), bits(ref["zt"])) and torch.equal(bits(v.cpu()), bits(ref["v"]))
    out, loss, grads = step(vds, m, zt, v, ctx, ref["ts"], ref["w"], cfg.time_patch_size)
    e_out = rel(out, ref["out"])
    e_loss = abs(loss - ref["loss"]) / abs(ref["loss"])
    worst = max((rel(grads[k], ref["grads"][k]), k) for k in grads
                if k in ref["grads"] and not k.endswith("lambda_param") and float(ref["grads"][k].abs().max()) > 0)
    print(f"{name}: out rel err {e_out:.3e}, loss rel {e_loss:.2e}, worst grad rel err {worst[0]:.3e} ({worst[1]})")
    parity_log(f"frame_timesteps_model_{name}", out=e_out, loss=e_loss, worst_grad=worst[0], worst_grad_name=worst[1],
               ref_distance_out=d_out, ref_distance_grad=d_grad[0])
    assert e_out <= B_OUT and e_loss <= B_LOSS
    assert worst[0] <= B_GRAD, worst


def test_recompute_is_bit_identical(vds, deterministic):
    cfg, P, latent, ctx, noise = model_case("hd64")
    ref = reference_step("hd64", False)
    args = (ref["zt"], ref["v"], ctx, ref["ts"], ref["w"], cfg.time_patch_size)
    out0, _, g0 = step(vds, build(vds, cfg, P, "none"), *args)
    assert float(g0["blocks.0.adaLN_modulation.1.weight"].abs().max()) > 0
    for mode in ("selective", "full"):
        out1, _, g1 = step(vds, build(vds, cfg, P, mode), *args)
        assert torch.equal(bits(out0), bits(out1)), mode
        for k in g0:
            assert torch.equal(bits(g0[k]), bits(g1[k])), (mode, k)


def test_per_frame_calls_take_the_per_block_modulation_path(vds, monkeypatch):
    """B*G = 8 rows would fit the batched adaLN launch: a [B, t] call must not use it (the [B] call still does)"""
    cfg, P, latent, ctx, noise = model_case("hd64")
    ref = reference_step("hd64", False)
    ops, calls = vds["ops"], []
    orig = ops.small_linear_fwd_batched
    monkeypatch.setattr(ops, "small_linear_fwd_batched", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    m = build(vds, cfg, P)
    with torch.no_grad():
        m(ref["zt"].cuda(), ctx.cuda(), ref["ts"].cuda(), rope_start=START)
        assert not calls
        m(ref["zt"].cuda(), ctx.cuda(), ref["ts"][:, 0].contiguous().cuda(), rope_start=START)
        assert len(calls) == 1


@pytest.mark.parametrize("reshard", [False, True], ids=["resident", "reshard_after_forward"])
def test_sharded_model_matches_unsharded(vds, deterministic, reshard):
    """apply_fsdp with the sharding runtime forced on over a 1-rank group: a [B, t] step gives the bits of the unsharded
    model in deterministic mode (both run the per-block modulation path: the same kernel sequence)"""
    import torch.distributed as dist
    from video_diffusion_speedrun_amd.fsdp import apply_fsdp
    cfg, P, latent, ctx, noise = model_case("hd64")
    ref = reference_step("hd64", False)
    args = (ref["zt"], ref["v"], ctx, ref["ts"], ref["w"], cfg.time_patch_size)

    def two_steps(m):
        opt = vds["optim"].MuAdamW(m.get_mup_setup(3e-3, 0.1, CONST)[0], betas=(0.95, 0.99))
        losses = []
        for _ in range(2):
            opt.zero_grad()
            out, loss, _ = step(vds, m, *args)
            opt.step()
            losses.append(loss)
        torch.cuda.synchronize()
        return out, losses, {k: v.clone() for k, v in m.full_state_dict().items()}

    out0, l0, p0 = two_steps(build(vds, cfg, P))
    assert l0[0] != l0[1]
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        m = apply_fsdp(build(vds, cfg, P), torch.bfloat16, torch.float32, force_runtime=True, reshard_after_forward=reshard)
        assert m._fsdp is not None
        out1, l1, p1 = two_steps(m)
        assert m._fsdp.n_all_gather > 0 and m._fsdp.n_reduce_scatter > 0
        assert torch.equal(bits(out0), bits(out1)) and l0 == l1, (l0, l1)
        assert not torch.equal(p0["blocks.1.adaLN_modulation.1.weight"], P["blocks.1.adaLN_modulation.1.weight"].cuda())
        for k in p0:
            assert torch.equal(p1[k], p0[k]), k
    finally:
        from video_diffusion_speedrun_amd import comm
        comm.destroy()
        dist.destroy_process_group()


def test_graph_replay_matches_eager(vds):
    """GraphedTrainStep(frame_mode="first_frame"): two eager steps, capture, three replays against five eager steps with
    the same seeds, within the bounds the graph tests use (losses 1e-4, parameters 2e-4 relative)"""
    from video_diffusion_speedrun_amd.graph import GraphedTrainStep
    cfg = O.DiTConfig(in_channels=16, hidden_size=128, depth=3, num_heads=2, cross_attn_input_size=64,
                      residual_v=True, train_bias_and_rms=False)
    P = O.init_params(cfg, seed=41, randomize_zero_init=True, init_std_factor=1.0)
    g = torch.Generator().manual_seed(5)
    batches = [{"latent": torch.randn(2, 16, 4, 8, 8, generator=g).cuda(), "context": torch.randn(2, 16, 64, generator=g).cuda(),
                "prompt": ["", ""]} for _ in range(5)]
    results = []
    for graphed in (False, True):
        m = build(vds, cfg, P)
        groups, _ = m.get_mup_setup(3e-3, 0.1, CONST)
        opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99))
        sched = vds["train"].get_schedule(opt, "cosine", 3, 50)
        torch.manual_seed(77)
        torch.cuda.manual_seed(77)
        losses = []
        if graphed:
            gs = GraphedTrainStep(m, opt, sched, "cuda", eager_steps=2, frame_mode="first_frame")
            for b in batches:
                losses.append(gs.step(b).item())
            assert gs.n_replays == 3 and opt._step == 5
        else:
            for b in batches:
                losses.append(vds["train"].train_step(m, opt, sched, b, "cuda", frame_mode="first_frame").item())
        torch.cuda.synchronize()
        results.append((losses, {k: v.clone() for k, v in m.full_state_dict().items()}))
    (l0, p0), (l1, p1) = results
    assert len(set(l0)) == 5
    print("graph first_frame: worst loss rel", max(abs(a - b) / abs(a) for a, b in zip(l0, l1)),
          "worst param rel", max(rel(p1[k], p0[k]) for k in p0))
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    for k in p0:
        assert rel(p1[k], p0[k]) <= 2e-4, (k, rel(p1[k], p0[k]))


def test_train_forward_modes(vds):
    """train.forward: explicit per-frame levels / weights reproduce the kernels' loss; "independent" runs; a sample
    without weight contributes nothing"""
    train, ops = vds["train"], vds["ops"]
    cfg, P, latent, ctx, noise = model_case("hd72")
    m = build(vds, cfg, P)
    batch = {"latent": latent.cuda(), "context": ctx.cuda()}
    ts, w = torch.tensor(TS), (torch.tensor(TS) > 0).float()
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    loss, _ = train.forward(m, batch, None, None, "cuda", 0, False, rope_start=START, frame_timesteps=ts, frame_weights=w)
    loss.backward()
    assert torch.isfinite(loss) and float(m.blocks[0].qkv.weight.grad.abs().max()) > 0
    l2, _ = train.forward(m, batch, None, None, "cuda", 0, False, rope_start=START, frame_mode="independent")
    assert torch.isfinite(l2) and l2.item() > 0
    l3, _ = train.forward(m, batch, None, None, "cuda", 0, False, rope_start=START, frame_timesteps=ts,
                          frame_weights=torch.zeros(2, 3))
    assert l3.item() == 0.0
    with pytest.raises(ValueError):
        train.forward(m, batch, None, None, "cuda", 0, False, frame_timesteps=torch.zeros(2, 2))


def test_sampler_holds_the_conditioning_frames(vds):
    """3 steps on a [1,16,4,8,8] latent with one token-frame (two latent frames) of conditioning"""
    S = vds["sampling"]
    cfg, P, _, _, _ = model_case("hd72")
    m = build(vds, cfg, P)
    g = torch.Generator().manual_seed(8)
    prompt = torch.randn(1, 12, 64, generator=g).to(bf16)
    lat0 = torch.randn(1, 16, 4, 8, 8, generator=g).to(bf16)
    cond = torch.randn(1, 16, 2, 8, 8, generator=g).to(bf16)
    steps, scale = 3, 4.0
    starts = [(1, 2, 3), (1, 2, 3), (4, 5, 6), (4, 5, 6), (7, 8, 9), (7, 8, 9)]
    acc = S.generate_latents(m, prompt.cuda(), inference_steps=steps, cfg_scale=scale, latents=lat0.cuda(),
                             rope_starts=starts, cond_latents=cond.cuda())
    assert acc.dtype == f32 and tuple(acc.shape) == (1, 16, 4, 8, 8) and torch.isfinite(acc).all()
    assert torch.equal(bits(acc[:, :, :2].cpu()), bits(cond.float()))
    ref = R.sample_loop(P, cfg, lat0, prompt, torch.zeros_like(prompt), steps, scale, starts, cond, dtype=f32)
    e = rel(acc[:, :, 2:], ref[:, :, 2:])
    free = S.generate_latents(m, prompt.cuda(), inference_steps=steps, cfg_scale=scale, latents=lat0.cuda(), rope_starts=starts)
    print("sampler with conditioning frames: rel err", e, "distance to the unconditioned run", rel(free[:, :, 2:], ref[:, :, 2:]))
    assert e <= 1.5e-2, e
    # the two-call form (distinct offsets inside a step) and the unguided form hold the frames too
    starts2 = [(1, 2, 3), (3, 2, 1)] * steps
    for kw in ({"cfg_scale": scale, "rope_starts": starts2}, {"cfg_scale": 1.0, "rope_starts": starts[0::2]}):
        a = S.generate_latents(m, prompt.cuda(), inference_steps=steps, latents=lat0.cuda(), cond_latents=cond.cuda(), **kw)
        assert torch.equal(bits(a[:, :, :2].cpu()), bits(cond.float())) and torch.isfinite(a).all()


def test_fp8_refuses_per_frame_timesteps(vds):
    cfg, P, latent, ctx, noise = model_case("hd72")
    m = build(vds, cfg, P).enable_fp8()
    with pytest.raises(NotImplementedError, match="per-frame timesteps"):
        m(latent.cuda(), ctx.cuda(), torch.tensor(TS).cuda(), rope_start=START)
