"""QK-norm on the GPU: the normed qkv / RoPE kernels (vds_qkv_rope_norm_fwd / _bwd) element by element against the float64
reference of tests/helpers/qk_norm_ref.py, everything they must not touch bit for bit against the plain kernels, and a
model built with qk_norm=True against the fp32 oracle whose apply_rotary is wrapped with rms_norm.

Bounds.  Forward, per element of q and k: |out - ref| <= 2^-8 (|x1n| + |x2n|) + 2^-8 |ref| + 1e-6 -- the kernel (fp32) and the
reference (float64) can differ where their rsqrt flips the bf16 rounding of a normalised element by one ulp, plus one flip of
the final rounding.  Backward, q / k sections: |out - ref| <= 2^-8 |ref| + 1e-5 r (|g| + |y| |mean(g y)|) -- the final rounding
plus fp32 noise of the cancelling difference, at the scale of the reference's own terms.  Model: the bounds of smoke()."""
import os
import sys

import pytest
import torch

from oracle import dit_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import qk_norm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
CONST = ["patch_proj", "context_kv", "positional_embedding"]


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import model, ops, optim, train
    return dict(model=model, ops=ops, optim=optim, train=train)


@pytest.fixture
def deterministic(vds, request):
    vds["ops"].set_deterministic(True, 256 << 20)
    request.addfinalizer(lambda: vds["ops"].set_deterministic(False))


def rel(a, b):
    a, b = a.float().cpu().flatten(), b.float().cpu().flatten()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def cosine(a, b):
    a, b = a.float().cpu().flatten(), b.float().cpu().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


# --------------------------------------------------------------------------------------- kernels ----
# name: (B, L, H, hd, hdp, {knob: value}); L counts plain token rows.  B * L = 38 at head_dim 72: at the default tile of 4
# tokens one tile spans the sample boundary and the last one holds 2 tokens.
CASES = {
    "hd72": (2, 19, 2, 72, 96, {}),
    "hd72_tile2": (2, 19, 2, 72, 96, {"rope_tile": 2}),
    "hd72_tile8": (2, 19, 2, 72, 96, {"rope_tile": 8}),
    "hd72_tok0": (2, 19, 2, 72, 96, {"rope_tok": 0}),      # backward: the element-wise form at a shape the token form takes
    "hd64": (2, 17, 3, 64, 64, {}),
    "hd128": (2, 9, 1, 128, 128, {}),
    "ew_hd24": (2, 9, 2, 24, 24, {}),                      # element-wise forward: no tile instance for head_dim 24
    "ew_hd72_L5": (2, 5, 2, 72, 96, {}),                   # ... below the tile kernel's L >= 8
    "ew_hd72_pad76": (2, 9, 2, 72, 76, {}),                # ... no ones columns; backward: hdp % 8 != 0 -> element-wise
}
FWD_CASES = [c for c in CASES if c != "hd72_tok0"]
BWD_CASES = [c for c in CASES if "tile" not in c]


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


def inputs(case):
    """the case's CPU tensors and float64 references, made once and shared by the tests (never modified)"""
    key = CASES[case][:5]
    if key in _inputs:
        return _inputs[key]
    B, L, H, hd, hdp = key
    D = H * hd
    g = torch.Generator().manual_seed(1000 * hd + 10 * L + H)
    qkv = (torch.randn(B * L, 3 * D, generator=g) * 1.5).to(bf16)
    qkv[3, (H - 1) * hd:H * hd] = 0  # one head row of q (token 3, last head): all zeros
    ang = torch.rand(L, hd // 2, generator=g) * 6.2832
    cos, sin = torch.cos(ang).float(), torch.sin(ang).float()
    v0 = torch.randn(B, H, L, hdp, generator=g).to(bf16)
    lam = torch.tensor([0.625]).to(bf16)
    dq, dk, dv = (torch.randn(B, H, L, hdp, generator=g).to(bf16) for _ in range(3))  # random pad columns too
    acc = torch.randn(B, H, L, hdp, generator=g)
    d = dict(B=B, L=L, H=H, hd=hd, hdp=hdp, qkv=qkv, cos=cos, sin=sin, v0=v0, lam=lam, dq=dq, dk=dk, dv=dv, acc=acc,
             fwd=R.forward_ref(qkv, cos, sin, B, L, H, hd), bwd=R.backward_ref(dq, dk, qkv, cos, sin, B, L, H, hd))
    _inputs[key] = d
    return d


@pytest.mark.parametrize("mix", [False, True], ids=["plain_v", "mixed_v"])
@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_kernel(vds, case, mix):
    ops, d = vds["ops"], inputs(case)
    B, L, H, hd, hdp = (d[k] for k in ("B", "L", "H", "hd", "hdp"))
    dev = lambda t: t.cuda()
    args = (dev(d["qkv"]), dev(d["cos"]), dev(d["sin"]), dev(d["v0"]) if mix else None, dev(d["lam"]) if mix else None,
            B, L, H, hd, hdp)
    with Knobs(ops, CASES[case][5]):
        q, k, v = ops.qkv_rope_norm_fwd(*args)
        q2, k2, v2 = ops.qkv_rope_norm_fwd(*args)
        qp, kp, vp = ops.qkv_rope_fwd(*args)
    torch.cuda.synchronize()
    q, k, v, qp, kp, vp = (t.cpu() for t in (q, k, v, qp, kp, vp))
    assert torch.equal(q, q2.cpu()) and torch.equal(k, k2.cpu()) and torch.equal(v, v2.cpu())  # reproducible
    worst = 0.0
    for name, out, (ref, partners) in (("q", q, d["fwd"][0]), ("k", k, d["fwd"][1])):
        assert not torch.isnan(out.float()).any(), name
        err = (out[..., :hd].to(f64) - ref).abs()
        bound = 2.0 ** -8 * partners + 2.0 ** -8 * ref.abs() + 1e-6
        worst = max(worst, float((err / bound).max()))
        assert torch.all(err <= bound), (name, float((err / bound).max()))
        # the norm did something: the plain kernel's rows differ
        assert not torch.equal(out[..., :hd], (qp if name == "q" else kp)[..., :hd])
    print(f"{case} mix={mix}: worst |out - ref| / bound = {worst:.3f}")
    # v and every pad column (the ones columns among them) are the plain kernel's bits
    assert torch.equal(v.view(torch.int16), vp.view(torch.int16))
    assert torch.equal(q[..., hd:].view(torch.int16), qp[..., hd:].view(torch.int16))
    assert torch.equal(k[..., hd:].view(torch.int16), kp[..., hd:].view(torch.int16))
    if hdp - hd >= 8:
        assert float(k[..., hd].min()) == 1.0 and float(k[..., hd + 1].min()) == 1.0
        assert float(v[..., hd].min()) == 1.0 and float(v[..., hd + 4].min()) == 1.0
        assert float(q[..., hd:].abs().max()) == 0.0 and float(k[..., hd + 2:].abs().max()) == 0.0
    elif hdp > hd:
        assert float(q[..., hd:].abs().max()) == 0.0 and float(k[..., hd:].abs().max()) == 0.0 and float(v[..., hd:].abs().max()) == 0.0
    # the zero row: zeros out
    assert float(q[0, H - 1, 3, :hd].abs().max()) == 0.0


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("mix", [0, 1, 2])
@pytest.mark.parametrize("case", BWD_CASES)
def test_backward_kernel(vds, case, mix, det, request):
    ops, d = vds["ops"], inputs(case)
    if det:
        ops.set_deterministic(True, 64 << 20)
        request.addfinalizer(lambda: ops.set_deterministic(False))
    add_dv0 = case == "hd72" and mix == 0  # block 0's call: dv + the accumulated v_0 gradient
    run_backward(ops, d, CASES[case][5], mix, add_dv0, det, case)


def run_backward(ops, d, knobs, mix, add_dv0, det, label):
    B, L, H, hd, hdp = (d[k] for k in ("B", "L", "H", "hd", "hdp"))
    D = H * hd
    dev = lambda t: t.cuda()
    fixed = (dev(d["dq"]), dev(d["dk"]), dev(d["dv"]), dev(d["cos"]), dev(d["sin"]))

    def call(fn, with_raw):
        acc = dev(d["acc"]).clone() if (mix == 1 or add_dv0) else None
        dlam = torch.full((1,), 0.25, dtype=f32, device="cuda") if mix else None
        out = fn(*fixed, dev(d["qkv"]) if (with_raw or mix) else None, dev(d["v0"]) if mix else None,
                 dev(d["lam"]) if mix else None, acc, dlam, mix, add_dv0, B, L, H, hd, hdp)
        torch.cuda.synchronize()
        return out.cpu(), None if acc is None else acc.cpu(), None if dlam is None else dlam.cpu()

    with Knobs(ops, knobs):
        got, acc, dlam = call(ops.qkv_rope_norm_bwd, True)
        got2, acc2, dlam2 = call(ops.qkv_rope_norm_bwd, True)
        plain, accp, dlamp = call(ops.qkv_rope_bwd, False)
    assert got.shape == (B * L, 3 * D) and not torch.isnan(got.float()).any()
    # reproducible: q / k / v sections and the accumulator in both modes (no atomics touch them); dlam in deterministic mode
    assert torch.equal(got.view(torch.int16), got2.view(torch.int16))
    if acc is not None:
        assert torch.equal(acc, acc2)
    # the v side is the plain kernel's, bit for bit
    assert torch.equal(got[:, 2 * D:].view(torch.int16), plain[:, 2 * D:].view(torch.int16))
    if acc is not None:
        assert torch.equal(acc, accp)
    if mix and det:
        assert torch.equal(dlam, dlamp) and torch.equal(dlam, dlam2)
    elif mix:
        assert abs(dlam.item() - dlamp.item()) <= 1e-4 * max(1.0, abs(dlamp.item()))
    worst = worst_rad = 0.0
    for section, (ref, scale, x) in enumerate(d["bwd"]):
        out = R._heads(got, B, L, H, hd, section).to(f64)
        err = (out - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + 1e-5 * scale
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert torch.all(err <= bound), (label, section, float((err / bound.clamp_min(1e-300)).max()))
        # the norm's Jacobian removes the radial component: what is left of sum_d dq_raw q_raw is rounding
        radial, total = (out * x).sum(-1).abs(), (out * x).abs().sum(-1)
        worst_rad = max(worst_rad, float((radial / total.clamp_min(1e-30)).max()))
        assert torch.all(radial <= 2.0 ** -7 * total), (label, section)
        assert not torch.equal(R._heads(got, B, L, H, hd, section), R._heads(plain, B, L, H, hd, section))
    print(f"{label} mix={mix} det={det}: worst |out - ref| / bound = {worst:.3f}, worst radial / sum|terms| = {worst_rad:.2e}")
    # the zero row of q: r = 1000, a finite gradient r * g
    zr = R._heads(got, B, L, H, hd, 0)[0, H - 1, 3].float()
    assert torch.isfinite(zr).all() and float(zr.abs().max()) > 0


# ----------------------------------------------------------------------------------------- model ----
def build(vds, cfg, P, mode="none", **kw):
    m = vds["model"].DiT(in_channels=cfg.in_channels, patch_size=cfg.patch_size, time_patch_size=cfg.time_patch_size,
                         hidden_size=cfg.hidden_size, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
                         cross_attn_input_size=cfg.cross_attn_input_size, residual_v=cfg.residual_v,
                         train_bias_and_rms=cfg.train_bias_and_rms, **kw)
    m.load_state_dict(P, strict=True)
    return m.to("cuda").enable_recompute(mode)


def model_case(name):
    """cfg, parameters and inputs: "smoke" = the model and inputs of smoke(); "hd64" = depth 3, D 128, head_dim 64"""
    if name == "smoke":
        cfg = O.DiTConfig(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=144, depth=2, num_heads=2,
                          cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False)
        P = O.init_params(cfg, seed=3, randomize_zero_init=True, init_std_factor=1.0)
        g = torch.Generator().manual_seed(4)
    else:
        cfg = O.DiTConfig(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=128, depth=3, num_heads=2,
                          cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False)
        P = O.init_params(cfg, seed=13, randomize_zero_init=True, init_std_factor=1.0)
        g = torch.Generator().manual_seed(14)
    B = 2
    latent = torch.randn(B, 16, 4, 8, 8, generator=g).to(bf16)
    ctx = torch.randn(B, 24, 64, generator=g).to(bf16)
    z = torch.randn(B, generator=g).to(bf16)
    noise = torch.randn(B, 16, 4, 8, 8, generator=g).to(bf16)
    t = O.time_shift(z)
    zt, v = O.noise_latents(latent, noise, t)
    return cfg, P, zt, v, ctx, t, (2, 3, 4)


_oracle = {}


def oracle_step(name, normed):
    """one fp32 oracle step (loss, output, gradients, the lambda gradients' term sums), computed once per (case, normed)"""
    if (name, normed) in _oracle:
        return _oracle[(name, normed)]
    cfg, P, zt, v, ctx, t, start = model_case(name)
    Pg = {k: w.clone().requires_grad_(True) for k, w in P.items()}
    cap = {}

    def run():
        out = O.dit_forward(Pg, cfg, zt.float(), ctx.float(), t.float(), start, cap)
        for i in range(1, cfg.depth):
            cap[f"blocks.{i}.v"].retain_grad()
        loss, _ = O.flow_loss(v, out)
        loss.backward()
        return out, loss

    if normed:
        with R.qk_normed_oracle():
            out, loss = run()
    else:
        out, loss = run()
    v0 = cap["blocks.0.v"].detach()
    l1 = {f"blocks.{i}.lambda_param": (cap[f"blocks.{i}.v"].grad * (cap[f"blocks.{i}.v"].detach() - v0)
                                       / P[f"blocks.{i}.lambda_param"].item()).abs().sum().item()
          for i in range(1, cfg.depth)}
    res = dict(out=out.detach(), loss=loss.item(), grads={k: p.grad for k, p in Pg.items() if p.grad is not None}, l1=l1)
    _oracle[(name, normed)] = res
    return res


@pytest.mark.parametrize("name", ["smoke", "hd64"])
def test_model_step_against_the_wrapped_oracle(vds, name):
    cfg, P, zt, v, ctx, t, start = model_case(name)
    ref, unnormed = oracle_step(name, True), oracle_step(name, False)
    # discrimination: the qkv weight gradients of the normed and the un-normed oracle are at least 10 x the 3e-2 bound apart,
    # so the gradient comparison below cannot pass on a path that skipped the norm (the outputs are only ~3e-3 apart)
    for i in range(cfg.depth):
        k = f"blocks.{i}.qkv.weight"
        dist = rel(unnormed["grads"][k], ref["grads"][k])
        print(f"{name}: {k} normed vs un-normed oracle {dist:.3f}")
        assert dist >= 10 * 3e-2, (k, dist)
    m = build(vds, cfg, P, qk_norm=True)
    out = m(zt.cuda(), ctx.cuda(), t.cuda(), rope_start=start)
    loss, _ = vds["train"].flow_loss(out, v.cuda())
    loss.backward()
    e_out = rel(out, ref["out"])
    e_loss = abs(loss.item() - ref["loss"]) / abs(ref["loss"])
    named = dict(m.named_parameters())
    worst = max((rel(p.grad, ref["grads"][k]), k) for k, p in named.items()
                if k in ref["grads"] and not k.endswith("lambda_param"))
    e_lam = {k: abs(named[k].grad.item() - ref["grads"][k].item()) / s for k, s in ref["l1"].items()}
    print(f"{name}: out rel err {e_out:.3e}, loss rel {e_loss:.2e}, worst grad rel err {worst[0]:.3e} ({worst[1]}), "
          f"lambda grad err / sum|terms| {e_lam}")
    assert e_out <= 2.5e-2 and e_loss <= 1e-2
    assert worst[0] <= 3e-2, worst
    assert all(e <= 2e-4 for e in e_lam.values()), e_lam


def grads_of(vds, m, zt, v, ctx, t, start):
    m.zero_grad()
    out = m(zt.cuda(), ctx.cuda(), t.cuda(), rope_start=start)
    loss, _ = vds["train"].flow_loss(out, v.cuda())
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}


def test_recompute_is_bit_identical(vds, deterministic):
    cfg, P, zt, v, ctx, t, start = model_case("hd64")
    out0, g0 = grads_of(vds, build(vds, cfg, P, "none", qk_norm=True), zt, v, ctx, t, start)
    assert float(g0["blocks.0.qkv.weight"].abs().max()) > 0
    for mode in ("selective", "full"):
        out1, g1 = grads_of(vds, build(vds, cfg, P, mode, qk_norm=True), zt, v, ctx, t, start)
        assert torch.equal(out0, out1), mode
        for k in g0:
            assert torch.equal(g0[k], g1[k]), (mode, k)


def test_default_is_the_model_without_the_keyword(vds, deterministic):
    cfg, P, zt, v, ctx, t, start = model_case("smoke")
    plain, off, on = build(vds, cfg, P), build(vds, cfg, P, qk_norm=False), build(vds, cfg, P, qk_norm=True)
    assert list(plain.state_dict().keys()) == list(off.state_dict().keys()) == list(on.state_dict().keys())
    out0, g0 = grads_of(vds, plain, zt, v, ctx, t, start)
    out1, g1 = grads_of(vds, off, zt, v, ctx, t, start)
    assert torch.equal(out0, out1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    out2, g2 = grads_of(vds, on, zt, v, ctx, t, start)
    assert not torch.equal(out0, out2) and not torch.equal(g0["blocks.1.qkv.weight"], g2["blocks.1.qkv.weight"])
    out3, g3 = grads_of(vds, on, zt, v, ctx, t, start)  # and the normed step is reproducible itself
    assert torch.equal(out2, out3) and all(torch.equal(g2[k], g3[k]) for k in g2)


def test_graph_replay_matches_eager(vds):
    """GraphedTrainStep on a qk_norm model: two eager steps, capture, three replays against five eager steps, within the
    bounds the graph tests use (losses 1e-4, parameters 2e-4 relative)."""
    from video_diffusion_speedrun_amd.graph import GraphedTrainStep
    cfg = O.DiTConfig(in_channels=16, hidden_size=128, depth=3, num_heads=2, cross_attn_input_size=64,
                      residual_v=True, train_bias_and_rms=False)
    P = O.init_params(cfg, seed=41, randomize_zero_init=True, init_std_factor=1.0)
    g = torch.Generator().manual_seed(5)
    batches = [{"latent": torch.randn(2, 16, 4, 8, 8, generator=g).cuda(), "context": torch.randn(2, 16, 64, generator=g).cuda(),
                "prompt": ["", ""]} for _ in range(5)]
    results = []
    for graphed in (False, True):
        m = build(vds, cfg, P, qk_norm=True)
        groups, _ = m.get_mup_setup(3e-3, 0.1, CONST)
        opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99))
        sched = vds["train"].get_schedule(opt, "cosine", 3, 50)
        torch.manual_seed(77)
        torch.cuda.manual_seed(77)
        losses = []
        if graphed:
            gs = GraphedTrainStep(m, opt, sched, "cuda", eager_steps=2)
            for b in batches:
                losses.append(gs.step(b).item())
            assert gs.n_replays == 3 and opt._step == 5
        else:
            for b in batches:
                losses.append(vds["train"].train_step(m, opt, sched, b, "cuda").item())
        torch.cuda.synchronize()
        results.append((losses, {k: v.clone() for k, v in m.full_state_dict().items()}))
    (l0, p0), (l1, p1) = results
    assert len(set(l0)) == 5
    print("graph qk_norm: worst loss rel", max(abs(a - b) / abs(a) for a, b in zip(l0, l1)),
          "worst param rel", max(rel(p1[k], p0[k]) for k in p0))
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    for k in p0:
        assert rel(p1[k], p0[k]) <= 2e-4, (k, rel(p1[k], p0[k]))


def test_fp8_linears_with_bf16_normed_attention(vds):
    """enable_fp8(attention=False) on a qk_norm model against the wrapped oracle, within the bounds of
    tests/test_model_gpu.py::test_fp8_step_close_to_oracle (output 2.5e-2, loss 1e-2, every gradient cosine >= 0.99 and
    relative error <= 0.15), on two passes: the second runs with delayed scaling, where the plain model's RoPE backward
    would emit fp8 and the normed one hands its bf16 result to the quantisation pass.  enable_fp8() itself is refused."""
    cfg, P, zt, v, ctx, t, start = model_case("smoke")
    ref = oracle_step("smoke", True)
    with pytest.raises(NotImplementedError, match=r"enable_fp8\(attention=False\)"):
        build(vds, cfg, P, qk_norm=True).enable_fp8()
    m = build(vds, cfg, P, qk_norm=True).enable_fp8(attention=False)
    for step in range(2):
        m.zero_grad()
        out = m(zt.cuda(), ctx.cuda(), t.cuda(), rope_start=start)
        loss, _ = vds["train"].flow_loss(out, v.cuda())
        loss.backward()
        assert rel(out, ref["out"]) <= 2.5e-2, (step, rel(out, ref["out"]))
        assert abs(loss.item() - ref["loss"]) / ref["loss"] <= 1e-2
        bad = []
        for k, p in m.named_parameters():
            r = ref["grads"].get(k)
            if r is None or k.endswith("lambda_param") or float(r.abs().max()) == 0:
                continue
            c, e = cosine(p.grad, r), rel(p.grad, r)
            if not (c >= 0.99 and e <= 0.15):
                bad.append((k, c, e))
        assert not bad, (step, bad)
    assert m._fp8_hist.ready
