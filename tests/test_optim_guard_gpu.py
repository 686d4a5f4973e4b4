"""GPU tests of the guarded optimizer step: the fixed-order global gradient norm, the clip, the non-finite skip and the
weight EMA of `MuAdamW(max_grad_norm=, skip_nonfinite=, ema_decay=)`, eager, replayed from a captured graph, sharded over
two emulated ranks and across a checkpoint.  inf / NaN appear here as ordinary floating-point data: nothing faults.

Tolerances:
    norm      : NORM_RTOL relative to the fp64 norm -- about 2x the worst value measured on the MI355X (every run logs
                its figures through `parity_log`).  A two-stage fp32 tree over 65 536-element chunks.
    clip      : 2e-6 relative per tensor, the bound of test_muadamw_matches_reference (fp32 AdamW vs torch on CPU)
    EMA       : 2 k 2^-24 max(|ema|, |p|) per element after k steps: one rounding each for the product and the sum of
                ema = d ema + (1 - d) p per step, contracted into an fma or not
"""
import os

import pytest
import torch

from oracle import dit_oracle as O

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
CONSTS = ["patch_proj", "context_kv", "positional_embedding"]
# measured on the MI355X: worst 6.2e-8 (the mixed list of test_grad_norm_matches_fp64_and_is_bit_reproducible; single
# tensors 0 .. 4.7e-8, a model's backward 1.1e-8, two emulated ranks 1.9e-8) -- one rounding of the fp32 result is 6e-8
NORM_RTOL = 1.3e-7
_NORM_WORST = [0.0]


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import video_diffusion_speedrun_amd as pkg
    from video_diffusion_speedrun_amd import model, ops, optim, train
    return dict(pkg=pkg, model=model, ops=ops, optim=optim, train=train)


@pytest.fixture(scope="module", autouse=True)
def _norm_report(parity_log):
    yield
    parity_log("test_optim_guard_gpu.grad_norm", worst_rel=_NORM_WORST[0], asserted=NORM_RTOL)


def rel(a, b):
    a, b = a.float().cpu().flatten(), b.float().cpu().flatten()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def bits(t):
    """a host copy compared as raw bits (NaN-safe)"""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16) if t.dtype == bf16 else t.view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def build(vds, cfg, P):
    m = vds["model"].DiT(in_channels=cfg.in_channels, patch_size=cfg.patch_size, time_patch_size=cfg.time_patch_size,
                         hidden_size=cfg.hidden_size, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
                         cross_attn_input_size=cfg.cross_attn_input_size, residual_v=cfg.residual_v,
                         train_bias_and_rms=cfg.train_bias_and_rms)
    m.load_state_dict(P, strict=True)
    return m.to("cuda")


def small_cfg(depth=2):
    return O.DiTConfig(in_channels=16, hidden_size=128, depth=depth, num_heads=2, cross_attn_input_size=64,
                       residual_v=True, train_bias_and_rms=False)


def norm_err(got, grads):
    want = torch.linalg.vector_norm(torch.cat([g.detach().double().flatten().cpu() for g in grads])).item()
    e = abs(float(got) - want) / want
    _NORM_WORST[0] = max(_NORM_WORST[0], e)
    return e, want


def plain_params(sizes, seed, shadow=True, misalign=()):
    """free-standing fp32 parameters with gradients (and bf16 shadows), like the optimizer sees them; `misalign`: indices
    whose parameter AND gradient start 4 bytes past a 16-byte boundary"""
    g = torch.Generator().manual_seed(seed)
    ps = []
    for i, n in enumerate(sizes):
        off = 1 if i in misalign else 0
        base, gbase = torch.randn(n + off, generator=g).cuda(), (torch.randn(n + off, generator=g) * 0.3).cuda()
        p = torch.nn.Parameter(base[off:])
        p.grad = gbase[off:]
        if off:
            assert p.data_ptr() % 16 == 4 and p.grad.data_ptr() % 16 == 4
        if shadow:
            p._vds_shadow = torch.zeros(n, dtype=bf16, device="cuda")
        ps.append(p)
    return ps


# ------------------------------------------------------------------------------------------ 4. norm
SIZES = [1, 3, 1023, 65536 + 5, 3 * 65536 + 17, 4099, 2 * 65536]


def test_grad_norm_matches_fp64_and_is_bit_reproducible(vds, parity_log):
    """every path of the sum-of-squares kernel: tensors of 1, 3, 1023, 65 536 + 5 elements and several chunks, one whose
    data pointers are 4- but not 16-byte aligned, a parameter without a gradient and an empty one (both skipped like
    today) -- vs torch.linalg.vector_norm of the concatenated gradients in fp64; two runs on the same gradients are
    bit-equal (no floating-point atomics)"""
    ps = plain_params(SIZES, seed=11, misalign=(5,))
    nograd = torch.nn.Parameter(torch.randn(100).cuda())                # .grad is None
    empty = torch.nn.Parameter(torch.zeros(0).cuda())
    empty.grad = torch.zeros(0).cuda()
    grads = [p.grad.clone() for p in ps]
    seen = []
    for run in range(2):
        opt = vds["optim"].MuAdamW([{"params": ps + [nograd, empty], "lr": 1e-3, "weight_decay": 0.1}],
                                   max_grad_norm=float("inf"))
        opt.step()
        seen.append(opt.grad_norm.clone())
        assert opt.grad_norm.dim() == 0 and opt.grad_norm.is_cuda
        assert all(torch.equal(p.grad, g) for p, g in zip(ps, grads))   # the gradients are read, never written
    e, want = norm_err(seen[0].item(), grads)
    parity_log("test_optim_guard_gpu.norm_mixed", rel_err=e, norm=want)
    print(f"grad norm: got {seen[0].item():.9g} want {want:.12g} rel err {e:.3e}")
    assert same_bits(seen[0], seen[1])
    assert e <= NORM_RTOL, e
    # one tensor at a time: each size alone through both stages
    for n in SIZES:
        (p,) = plain_params([n], seed=100 + n)
        opt = vds["optim"].MuAdamW([p], max_grad_norm=float("inf"))
        opt.step()
        e, want = norm_err(opt.grad_norm.item(), [p.grad])
        parity_log("test_optim_guard_gpu.norm_single", n=n, rel_err=e)
        print(f"grad norm n={n}: rel err {e:.3e}")
        assert e <= NORM_RTOL, (n, e)


def test_grad_norm_of_a_model_backward(vds, parity_log):
    cfg = small_cfg()
    m = build(vds, cfg, O.init_params(cfg, seed=21, randomize_zero_init=True, init_std_factor=1.0))
    groups, _ = m.get_mup_setup(3e-3, 0.1, CONSTS)
    opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99), max_grad_norm=1e9)
    g = torch.Generator().manual_seed(3)
    batch = {"latent": torch.randn(2, 16, 4, 8, 8, generator=g), "context": torch.randn(2, 16, 64, generator=g)}
    vds["train"].train_step(m, opt, None, batch, "cuda", rope_start=(1, 2, 3))
    e, want = norm_err(opt.grad_norm.item(), [p.grad for p in m.parameters() if p.grad is not None])
    parity_log("test_optim_guard_gpu.norm_model", rel_err=e, norm=want)
    assert e <= NORM_RTOL, e


# ------------------------------------------------------------------------------------------ 5. clip
def _g4(golden_dir):
    fx = torch.load(os.path.join(golden_dir, "g4_optim.pt"), weights_only=False)["adamw"]
    cfg = O.DiTConfig(**fx["cfg"])
    return fx, O.mup_settings(O.param_shapes(cfg), fx["lr"], fx["wd"], CONSTS)


GSCALE = 4.0  # the recorded gradients (global norm 2.4-2.5) times 4: norm ~10 against max_grad_norm = 1


def _run_g4(vds, fx, table, **opts):
    ps = {k: torch.nn.Parameter(v.clone().cuda()) for k, v in fx["p0"].items()}
    groups = [{"params": [p], "lr": table[k]["lr"], "weight_decay": table[k]["wd"]} for k, p in ps.items()]
    opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99), **opts)
    norms = []
    for s in range(2):
        mult = O.lr_lambda(s, "cosine", 20, 1000)
        for gi, (k, p) in enumerate(ps.items()):
            p.grad = (fx["grads"][s][k] * GSCALE).clone().cuda()
            opt.param_groups[gi]["lr"] = table[k]["lr"] * mult
        opt.step()
        if opt.guarded:
            norms.append(opt.grad_norm.item())
    return ps, opt, norms


def test_clipped_step_matches_clip_grad_norm_and_adamw(vds, golden_dir, parity_log):
    """two clipped steps on the g4_optim.pt setup (gradients scaled so the norm exceeds max_grad_norm = 1) vs
    torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW on CPU fp32 with the same groups: 2e-6 relative per tensor"""
    fx, table = _g4(golden_dir)
    ps, opt, norms = _run_g4(vds, fx, table, max_grad_norm=1.0)
    ref = {k: torch.nn.Parameter(v.clone()) for k, v in fx["p0"].items()}
    ropt = torch.optim.AdamW([{"params": [p], "lr": table[k]["lr"], "weight_decay": table[k]["wd"]}
                              for k, p in ref.items()], betas=(0.95, 0.99), eps=1e-8)
    worst = 0.0
    for s in range(2):
        mult = O.lr_lambda(s, "cosine", 20, 1000)
        for gi, (k, p) in enumerate(ref.items()):
            p.grad = (fx["grads"][s][k] * GSCALE).clone()
            ropt.param_groups[gi]["lr"] = table[k]["lr"] * mult
        total = torch.nn.utils.clip_grad_norm_(list(ref.values()), 1.0)
        assert total.item() > 5.0  # clipping is active
        assert norm_err(norms[s], [fx["grads"][s][k] * GSCALE for k in fx["p0"]])[0] <= NORM_RTOL  # the pre-clip norm
        ropt.step()
    for k, p in ps.items():
        assert torch.equal(p.grad.cpu(), fx["grads"][1][k] * GSCALE), k  # p.grad is not modified by clipping
        worst = max(worst, rel(p.data, ref[k].data))
        assert rel(p.data, ref[k].data) < 2e-6, (k, rel(p.data, ref[k].data))
    parity_log("test_optim_guard_gpu.clip_vs_torch", worst_rel=worst)
    print(f"clipped AdamW vs torch: worst rel {worst:.3e}")


def test_clip_above_the_norm_is_bit_identical_to_the_plain_step(vds, golden_dir):
    fx, table = _g4(golden_dir)
    plain, popt, _ = _run_g4(vds, fx, table)
    for mg in (1e4, float("inf")):
        ps, opt, norms = _run_g4(vds, fx, table, max_grad_norm=mg)
        assert 5.0 < norms[0] < 100.0
        assert opt._guard[1].item() == 1.0  # the coefficient, exactly
        for k in plain:
            assert same_bits(ps[k].data, plain[k].data), (mg, k)
            for key in ("exp_avg", "exp_avg_sq"):
                assert same_bits(opt.state[ps[k]][key], popt.state[plain[k]][key]), (mg, k, key)


# ------------------------------------------------------------------------------------------ 6. skip
SKIP_SIZES = [3 * 65536 + 5, 1023, 65536 + 5]


def _skip_setup(vds, **opts):
    ps = plain_params(SKIP_SIZES, seed=31)
    groups = [{"params": [p], "lr": 1e-3 * (i + 1), "weight_decay": 0.1} for i, p in enumerate(ps)]
    return ps, vds["optim"].MuAdamW(groups, betas=(0.95, 0.99), **opts)


def _snapshot(ps, opt):
    out = []
    for p in ps:
        st = opt.state[p]
        out.append([p.data.clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), p._vds_shadow.clone()] +
                   ([st["ema"].clone()] if "ema" in st else []))
    return out


@pytest.mark.parametrize("where", ["vectorised", "tail"])
@pytest.mark.parametrize("poison", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_nonfinite_step_is_skipped_and_the_next_one_trains(vds, poison, where):
    """one inf / NaN in one gradient element -- in a 16-byte-vector region, or in the last element of a tensor's scalar
    tail: parameters, moments, bf16 shadows and EMA keep every bit and the count reads 1; the following clean step is
    AdamW step number 2 (a skipped step still counts for the bias corrections) from untouched state"""
    ps, opt = _skip_setup(vds, max_grad_norm=1e6, skip_nonfinite=True, ema_decay=0.9)
    clean = [p.grad.clone() for p in ps]
    p0 = [p.data.clone() for p in ps]
    # state before the poisoned step: p0, zero moments, zero shadows, EMA = p0 (initialised on first sight)
    ti, ei = (0, 70000) if where == "vectorised" else (2, SKIP_SIZES[2] - 1)
    ps[ti].grad[ei] = poison
    opt.step()
    torch.cuda.synchronize()
    assert opt.skipped_steps() == 1 and not torch.isfinite(opt.grad_norm).item()
    for p, q in zip(ps, p0):
        st = opt.state[p]
        assert same_bits(p.data, q) and same_bits(st["ema"], q)
        assert not st["exp_avg"].any().item() and not st["exp_avg_sq"].any().item()
        assert not p._vds_shadow.view(torch.int16).any().item()
    # clean step = step number 2 of the reference from the same (untouched) state
    for p, g in zip(ps, clean):
        p.grad.copy_(g)
    opt.step()
    torch.cuda.synchronize()
    assert opt.skipped_steps() == 1 and opt._step == 2
    for i, (p, q, g) in enumerate(zip(ps, p0, clean)):
        r = torch.nn.Parameter(q.cpu().clone())
        r.grad = g.cpu().clone()
        ropt = torch.optim.AdamW([r], lr=1e-3 * (i + 1), weight_decay=0.1, betas=(0.95, 0.99), eps=1e-8)
        ropt.state[r] = {"step": torch.tensor(1.0), "exp_avg": torch.zeros_like(r), "exp_avg_sq": torch.zeros_like(r)}
        ropt.step()
        assert rel(p.data, r.data) < 2e-6, (i, rel(p.data, r.data))
        assert torch.equal(p._vds_shadow.cpu(), p.data.to(bf16).cpu())
        pn, qd = p.data.double().cpu(), q.double().cpu()
        want_ema = 0.9 * qd + 0.1 * pn
        bound = 2 * 2.0 ** -24 * torch.maximum(torch.maximum(want_ema.abs(), pn.abs()), qd.abs())
        assert ((opt.state[p]["ema"].double().cpu() - want_ema).abs() <= bound).all().item()


def test_a_skipped_step_after_real_steps_keeps_every_bit(vds):
    ps, opt = _skip_setup(vds, max_grad_norm=0.5, skip_nonfinite=True, ema_decay=0.5)
    for _ in range(2):
        opt.step()
    before = _snapshot(ps, opt)
    ps[1].grad[1022] = float("inf")
    opt.step()
    torch.cuda.synchronize()
    assert opt.skipped_steps() == 1
    for a, b in zip(before, _snapshot(ps, opt)):
        assert len(a) == 5 and all(same_bits(x, y) for x, y in zip(a, b))


def test_without_skip_nonfinite_the_behaviour_is_todays(vds):
    """skip_nonfinite=False: a poisoned gradient goes through the guarded kernel exactly as through the plain one"""
    results = []
    for opts in ({}, {"ema_decay": 0.9}, {"max_grad_norm": float("inf")}):
        ps, opt = _skip_setup(vds, **opts)
        ps[0].grad[70000] = float("inf")
        ps[2].grad[SKIP_SIZES[2] - 1] = float("nan")
        opt.step()
        torch.cuda.synchronize()
        assert opt.skipped_steps() == 0
        results.append([t[:4] for t in _snapshot(ps, opt)])
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert all(same_bits(x, y) for x, y in zip(a, b))
    assert torch.isinf(results[0][0][1][70000]).item() and not torch.isfinite(results[0][0][0][70000]).item()
    assert torch.isfinite(results[0][0][0][:70000]).all().item()  # only the poisoned elements are hit


# ------------------------------------------------------------------------------------------ 7. EMA
def _batch(seed, B=2):
    g = torch.Generator().manual_seed(seed)
    return {"latent": torch.randn(B, 16, 4, 8, 8, generator=g), "context": torch.randn(B, 16, 64, generator=g),
            "prompt": [""] * B}


def test_ema_follows_the_fp64_recurrence_on_the_gpus_own_parameters(vds, tmp_path, parity_log):
    from video_diffusion_speedrun_amd import checkpoint as ck
    cfg, K, D = small_cfg(), 6, 0.9
    P = O.init_params(cfg, seed=41, randomize_zero_init=True, init_std_factor=1.0)
    m = build(vds, cfg, P)
    groups, _ = m.get_mup_setup(3e-3, 0.1, CONSTS)
    opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99), ema_decay=D)
    batch = _batch(3)
    names = [n for n, _ in m.named_parameters()]
    ema = scale = None
    for s in range(K):
        gen = torch.Generator(device="cuda").manual_seed(100 + s)
        torch.manual_seed(0)
        if s == 0:  # the EMA starts as a copy of the parameters BEFORE the first update
            ema = {n: p.detach().double().cpu() for n, p in m.named_parameters()}
            scale = {n: e.abs() for n, e in ema.items()}
        vds["train"].train_step(m, opt, None, batch, "cuda", generator=gen, rope_start=(1, 2, 3))
        for n, p in m.named_parameters():
            pc = p.detach().double().cpu()
            ema[n] = D * ema[n] + (1 - D) * pc
            scale[n] = torch.maximum(scale[n], torch.maximum(ema[n].abs(), pc.abs()))
    worst = 0.0
    got = opt.ema_named(m)
    assert sorted(got) == sorted(names)
    for n in names:
        assert got[n].shape == dict(m.named_parameters())[n].shape and got[n].dtype == f32
        err = (got[n].double().cpu() - ema[n]).abs()
        bound = 2 * K * 2.0 ** -24 * scale[n]
        worst = max(worst, (err / bound.clamp_min(1e-30)).max().item())
        assert (err <= bound).all().item(), (n, (err / bound.clamp_min(1e-30)).max().item())
    parity_log("test_optim_guard_gpu.ema_recurrence", worst_fraction_of_bound=worst, steps=K)
    print(f"EMA vs fp64 recurrence: worst error / bound = {worst:.3f}")
    # a forward under ema_weights() == a forward of a fresh model loaded from model_ema.pt, to the bit
    ck.save_checkpoint(str(tmp_path / "c"), m, opt, step=K)
    assert sorted(os.listdir(tmp_path / "c")) == ["model.pt", "model_ema.pt", "optim_rank0_of1.pt"]
    state = ck.read_model_state(str(tmp_path / "c"), ema=True)
    for n in names:
        assert torch.equal(state[n], got[n].cpu()), n
    assert not torch.equal(state["final_proj.weight"], ck.read_model_state(str(tmp_path / "c"))["final_proj.weight"])
    x, ctx = batch["latent"].cuda().to(bf16), batch["context"].cuda().to(bf16)
    t = torch.tensor([0.3, 0.6]).cuda()
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    with torch.no_grad():
        raw = m(x, ctx, t, rope_start=(1, 2, 3)).clone()
        with opt.ema_weights():
            y_ema = m(x, ctx, t, rope_start=(1, 2, 3)).clone()
        y_file = build(vds, cfg, state)(x, ctx, t, rope_start=(1, 2, 3))
        back = m(x, ctx, t, rope_start=(1, 2, 3))
    assert same_bits(y_ema, y_file) and not same_bits(y_ema, raw) and same_bits(back, raw)
    for n, p in m.named_parameters():
        assert same_bits(p.detach(), before[n]) and same_bits(opt.state[p]["ema"], got[n]), n
    # without an EMA the files are today's
    opt2 = vds["optim"].MuAdamW(m.get_mup_setup(3e-3, 0.1, CONSTS)[0], betas=(0.95, 0.99), max_grad_norm=1.0)
    ck.save_checkpoint(str(tmp_path / "d"), m, opt2, step=1)
    assert sorted(os.listdir(tmp_path / "d")) == ["model.pt", "optim_rank0_of1.pt"]


def test_training_continues_bit_identically_after_an_ema_swap(vds, request):
    """deterministic mode: steps, a forward under ema_weights(), more steps == the same steps without the swap"""
    vds["ops"].set_deterministic(True, 256 << 20)
    request.addfinalizer(lambda: vds["ops"].set_deterministic(False))
    cfg = small_cfg()
    P = O.init_params(cfg, seed=41, randomize_zero_init=True, init_std_factor=1.0)
    batch = _batch(3)
    x, ctx = batch["latent"].cuda().to(bf16), batch["context"].cuda().to(bf16)
    t = torch.tensor([0.3, 0.6]).cuda()
    finals = []
    for swap in (False, True):
        m = build(vds, cfg, P)
        opt = vds["optim"].MuAdamW(m.get_mup_setup(3e-3, 0.1, CONSTS)[0], betas=(0.95, 0.99), max_grad_norm=1.0,
                                   skip_nonfinite=True, ema_decay=0.9)
        losses = []
        for s in range(4):
            if swap and s == 2:
                with torch.no_grad(), opt.ema_weights():
                    m(x, ctx, t, rope_start=(1, 2, 3))
            gen = torch.Generator(device="cuda").manual_seed(100 + s)
            torch.manual_seed(0)
            losses.append(vds["train"].train_step(m, opt, None, batch, "cuda", generator=gen, rope_start=(1, 2, 3)).item())
        finals.append((losses, m.full_state_dict(), opt.ema_named(m), [g.shadow.clone() for g in m._groups]))
    (l0, p0, e0, s0), (l1, p1, e1, s1) = finals
    assert l0 == l1
    assert all(same_bits(p0[k], p1[k]) for k in p0) and all(same_bits(e0[k], e1[k]) for k in e0)
    assert all(same_bits(a, b) for a, b in zip(s0, s1))


# ------------------------------------------------------------------------------------------ 8. graph
def test_graph_replay_with_all_three_options(vds):
    """GraphedTrainStep with clip + skip + EMA: replays match eager steps (the criterion of
    test_graph_replay_matches_eager_steps: losses 1e-4, parameters 2e-4 relative); ema_decay changes between replays
    without a new capture; a replay fed an inf latent is skipped and the next one trains; an eager forward under
    ema_weights() between two replays sees the EMA and the following replay the raw weights again"""
    from video_diffusion_speedrun_amd.graph import GraphedTrainStep
    cfg = small_cfg(depth=3)
    P = O.init_params(cfg, seed=41, randomize_zero_init=True, init_std_factor=1.0)
    g = torch.Generator().manual_seed(5)
    batches = [{"latent": torch.randn(2, 16, 4, 8, 8, generator=g).cuda(), "context": torch.randn(2, 16, 64, generator=g).cuda(),
                "prompt": ["", ""]} for _ in range(6)]
    decays = [0.9, 0.9, 0.9, 0.9, 0.5, 0.5]  # changed after the capture (steps 0-1 eager, step 2 captures)
    results = []
    for graphed in (False, True):
        m = build(vds, cfg, P)
        groups, _ = m.get_mup_setup(3e-3, 0.1, CONSTS)
        opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99), max_grad_norm=0.05, skip_nonfinite=True, ema_decay=0.9)
        sched = vds["train"].get_schedule(opt, "cosine", 3, 50)
        torch.manual_seed(77)
        torch.cuda.manual_seed(77)
        losses, norms = [], []
        gs = GraphedTrainStep(m, opt, sched, "cuda", eager_steps=2) if graphed else None
        for b, d in zip(batches, decays):
            opt.ema_decay = d
            if graphed:
                losses.append(gs.step(b).item())
            else:
                losses.append(vds["train"].train_step(m, opt, sched, b, "cuda").item())
            norms.append(opt.grad_norm.item())
        torch.cuda.synchronize()
        if graphed:
            assert gs.n_replays == 4 and opt._step == 6
        assert opt.skipped_steps() == 0 and min(norms) > 0.05  # every step was clipped
        results.append((losses, {k: v.clone() for k, v in m.full_state_dict().items()},
                        {k: v.clone() for k, v in opt.ema_named(m).items()}, norms))
    (l0, p0, e0, n0), (l1, p1, e1, n1) = results
    assert len(set(l0)) == 6
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(n0, n1)), (n0, n1)
    for k in p0:
        assert rel(p1[k], p0[k]) <= 2e-4, (k, rel(p1[k], p0[k]))
        assert rel(e1[k], e0[k]) <= 2e-4, (k, rel(e1[k], e0[k]))
    # (the eager run changed the decay at the same steps: replays that ignored the change would miss e0 by far more)
    # --- a poisoned batch is skipped on the device, the next replay trains
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    ema_before = {n: e.clone() for n, e in opt.ema_named(m).items()}
    bad = {"latent": batches[0]["latent"].clone(), "context": batches[0]["context"]}
    bad["latent"][1, 3, 2, 4, 4] = float("inf")
    gs.step(bad)
    torch.cuda.synchronize()
    assert opt.skipped_steps() == 1 and not torch.isfinite(opt.grad_norm).item()
    for n, p in m.named_parameters():
        assert same_bits(p.detach(), before[n]) and same_bits(opt.ema_named(m)[n], ema_before[n]), n
    loss = gs.step(batches[1]).item()
    torch.cuda.synchronize()
    assert loss == loss and opt.skipped_steps() == 1 and torch.isfinite(opt.grad_norm).item()
    changed = [n for n, p in m.named_parameters() if not same_bits(p.detach(), before[n])]
    assert len(changed) >= len(before) - 1  # blocks.0.lambda_param has no gradient path
    assert all(torch.isfinite(p).all().item() for p in m.parameters())
    # --- eager EMA forward between two replays
    x, ctx = batches[2]["latent"].to(bf16), batches[2]["context"].to(bf16)
    t = torch.tensor([0.3, 0.6]).cuda()
    with torch.no_grad():
        raw = m(x, ctx, t, rope_start=(1, 2, 3)).clone()
        with opt.ema_weights():
            y_ema = m(x, ctx, t, rope_start=(1, 2, 3)).clone()
        ema_model = build(vds, cfg, {n: e.reshape(P[n].shape).cpu() for n, e in opt.ema_named(m).items()})
        assert same_bits(y_ema, ema_model(x, ctx, t, rope_start=(1, 2, 3))) and not same_bits(y_ema, raw)
    held = {n: p.detach().clone() for n, p in m.named_parameters()}
    l_next = gs.step(batches[3]).item()
    torch.cuda.synchronize()
    assert gs.n_replays == 7 and opt.skipped_steps() == 1
    # the replay saw the raw weights again: the bf16 copies it computed with were re-cast from the raw masters before it,
    # and after it they are the cast of the stepped raw masters
    for grp in m._groups:
        assert torch.equal(grp.shadow.cpu(), grp.master.to(bf16).cpu())
    moved = [n for n, p in m.named_parameters() if not same_bits(p.detach(), held[n])]
    assert len(moved) >= len(held) - 1 and l_next == l_next


def test_ema_decay_change_takes_effect_in_a_replay(vds):
    """after the capture with d = 0.9, one replay with d = 0: the EMA equals the new parameters to the bit"""
    from video_diffusion_speedrun_amd.graph import GraphedTrainStep
    cfg = small_cfg()
    m = build(vds, cfg, O.init_params(cfg, seed=43, randomize_zero_init=True, init_std_factor=1.0))
    opt = vds["optim"].MuAdamW(m.get_mup_setup(3e-3, 0.1, CONSTS)[0], betas=(0.95, 0.99), ema_decay=0.9)
    gs = GraphedTrainStep(m, opt, None, "cuda", eager_steps=1)
    for s in range(3):
        gs.step(_batch(50 + s))
    torch.cuda.synchronize()
    assert gs.n_replays == 2
    assert any(not same_bits(e, dict(m.named_parameters())[n].detach()) for n, e in opt.ema_named(m).items())
    opt.ema_decay = 0.0
    gs.step(_batch(60))
    torch.cuda.synchronize()
    assert gs.n_replays == 3
    for n, p in m.named_parameters():
        assert same_bits(opt.ema_named(m)[n], p.detach()), n


# ------------------------------------------------------------------------------------------ 9. sharded
def _emulate_ranks(vds, monkeypatch, cfg, P, W, opts_of):
    """W replicas of one model in this process with the real shard layout, stream / event choreography, HIP kernels and
    sharded optimizer; the collectives are replaced by an in-process exchange (RCCL refuses two ranks on one device).
    The substitute of the optimizer's all-reduce computes the global sum of squares from every rank's gradient shards
    with torch (`opts_of()`: the optimizers, whose parameters carry the reduced gradient shards)."""
    from video_diffusion_speedrun_amd import params as PM
    from video_diffusion_speedrun_amd.fsdp import apply_fsdp
    reps, tokens, pending, calls = [], [object() for _ in range(W)], {}, []

    def find(buf, attr):
        for r, m in enumerate(reps):
            for gi, grp in enumerate(m._groups):
                if getattr(grp, attr).data_ptr() == buf.data_ptr():
                    return r, gi
        raise AssertionError("collective on an unknown buffer")

    def fake_all_gather(out, inp, group=None):
        _, gi = find(inp, "shadow")
        parts = out.view(W, -1)
        for r2, m2 in enumerate(reps):
            parts[r2].copy_(m2._groups[gi].master.to(bf16))

    def fake_reduce_scatter(out, inp, group=None):
        r, gi = find(inp, "gfull")
        pending.setdefault(gi, {})[r] = inp.clone()
        if len(pending[gi]) == W:
            avg = sum(pending[gi].values()) / W
            for r2, m2 in enumerate(reps):
                m2._groups[gi].gshard.copy_(avg.view(W, -1)[r2])

    def fake_all_reduce_sum(buf, group=None):
        assert buf.numel() == 1 and buf.dtype == f32 and group in tokens
        local = buf.item()
        total = sum(float((p.grad.double() ** 2).sum()) for m2 in reps for p in m2.parameters() if p.grad is not None)
        calls.append((tokens.index(group), local, total))
        buf.fill_(total)

    monkeypatch.setattr(PM, "all_gather_flat", fake_all_gather)
    monkeypatch.setattr(PM, "reduce_scatter_avg", fake_reduce_scatter)
    monkeypatch.setattr(PM, "all_reduce_sum", fake_all_reduce_sum)
    for r in range(W):
        m = build(vds, cfg, P)
        reps.append(apply_fsdp(m, torch.bfloat16, torch.float32, process_group=tokens[r], world_rank=(W, r)))
        assert m._fsdp is not None and m._groups[1].world == W and m._groups[1].rank == r
    return reps, pending, calls


def test_guarded_step_on_two_emulated_ranks(vds, monkeypatch, parity_log):
    """world size 2 on one GPU: the global norm equals the unsharded model's (NORM_RTOL: another summation order), the
    clipped sharded step matches the clipped unsharded step within the bound of test_two_emulated_ranks_on_one_gpu
    (2e-4), the concatenated EMA shards equal the unsharded EMA within the EMA bound"""
    W, D, MAXN = 2, 0.9, 0.05
    cfg = small_cfg(depth=3)
    P = O.init_params(cfg, seed=61, randomize_zero_init=True, init_std_factor=1.0)
    g = torch.Generator().manual_seed(62)
    x = torch.randn(4, 16, 4, 8, 8, generator=g).to(bf16).cuda()
    ctx = torch.randn(4, 16, 64, generator=g).to(bf16).cuda()
    t = torch.tensor([0.2, 0.5, 0.7, 0.9]).to(bf16).cuda()
    v = torch.randn(4, 16, 4, 8, 8, generator=g).to(bf16).cuda()
    start = (1, 2, 3)

    def step(m, sl):
        groups, _ = m.get_mup_setup(3e-3, 0.1, CONSTS)
        opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99), max_grad_norm=MAXN, skip_nonfinite=True, ema_decay=D)
        out = m(x[sl], ctx[sl], t[sl], rope_start=start)
        loss, _ = vds["train"].flow_loss(out, v[sl])
        loss.backward()
        return opt

    ref = build(vds, cfg, P)
    opt = step(ref, slice(0, 4))
    full_grads = [p.grad.clone() for p in ref.parameters() if p.grad is not None]
    opt.step()
    torch.cuda.synchronize()
    e_ref, want_norm = norm_err(opt.grad_norm.item(), full_grads)
    assert want_norm > 2 * MAXN and e_ref <= NORM_RTOL
    want, want_ema = ref.full_state_dict(), {n: e.clone() for n, e in opt.ema_named(ref).items()}

    opts = []
    reps, pending, calls = _emulate_ranks(vds, monkeypatch, cfg, P, W, lambda: opts)
    for r in range(W):
        opts.append(step(reps[r], slice(2 * r, 2 * r + 2)))
    torch.cuda.synchronize()
    assert all(len(d) == W for d in pending.values())
    for o in opts:
        o.step()
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == [0, 1]
    # each rank contributed ITS sum of squares, and the ranks' sums add up to the global one
    assert abs(sum(c[1] for c in calls) - calls[0][2]) <= 4 * NORM_RTOL * calls[0][2]
    for o in opts:
        e = abs(o.grad_norm.item() - want_norm) / want_norm
        _NORM_WORST[0] = max(_NORM_WORST[0], e)
        parity_log("test_optim_guard_gpu.norm_sharded", rel_err=e)
        print(f"sharded norm vs unsharded fp64 norm: rel err {e:.3e}")
        assert e <= NORM_RTOL, e
        assert o.skipped_steps() == 0
    shard_grads = [p.grad for m2 in reps for p in m2.parameters() if p.grad is not None]
    e, _ = norm_err(opts[0].grad_norm.item(), shard_grads)  # against the fp64 norm of the SAME (sharded) gradients
    assert e <= NORM_RTOL, e
    assert same_bits(opts[0].grad_norm, opts[1].grad_norm)
    for gi, grp0 in enumerate(reps[0]._groups):
        flat = torch.cat([m2._groups[gi].master for m2 in reps])
        eflat = torch.zeros_like(flat)
        for r, m2 in enumerate(reps):
            for n, e in opts[r].ema_named(m2).items():
                if n in m2._groups[gi].offsets:
                    lo, hi = m2._groups[gi].local_range(n)
                    assert e.numel() == hi - lo  # shard-sized: the EMA is divided by the world size for free
                    eflat[r * grp0.shard + lo:r * grp0.shard + hi] = e
        for n in grp0.names:
            o0 = grp0.offsets[n]
            got = flat[o0:o0 + want[n].numel()].view(want[n].shape)
            assert rel(got, want[n]) <= 2e-4, (n, rel(got, want[n]))
            got_e = eflat[o0:o0 + want[n].numel()].view(want[n].shape).double()
            # EMA after one step = D p0 + (1 - D) p1: the sharded p1 differs from the unsharded p1 by the step's own
            # tolerance, so compare each side with ITS recurrence (bound 2 k 2^-24 max(|ema|, |p|), k = 1)
            p0_, p1_ = P[n].double().cuda(), got.double()
            rec = D * p0_ + (1 - D) * p1_
            bound = 2 * 2.0 ** -24 * torch.maximum(torch.maximum(rec.abs(), p1_.abs()), p0_.abs())
            assert ((got_e - rec).abs() <= bound).all().item(), n
            assert rel(got_e, want_ema[n]) <= 2e-4, n
        # the EMA file of a sharded run: the shards gathered to full tensors with one all-gather per group.  The
        # substitute hands out the concatenation built above and checks what rank 0 contributes
        from video_diffusion_speedrun_amd import params as PM
        mine = opts[0].ema_named(reps[0])

        def gather_ema(out, inp, group=None, grp0=grp0, eflat=eflat, mine=mine):
            for n, e in mine.items():
                if n in grp0.offsets and e.numel():
                    lo, hi = grp0.local_range(n)
                    assert torch.equal(inp[lo:hi], e.flatten())
            out.copy_(eflat)

        monkeypatch.setattr(PM, "all_gather_flat", gather_ema)
        full = grp0.full_tensors_of(mine)
        for n in grp0.names:
            o0 = grp0.offsets[n]
            assert torch.equal(full[n], eflat[o0:o0 + want[n].numel()].view(want[n].shape)), n


def test_real_two_gpu_guarded_step():
    """the same over a real 2-rank RCCL communicator (vds_all_reduce_f32_sum on the communication stream); needs two GPUs"""
    import socket
    import subprocess
    import sys
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs in one box")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(repo, "tests", "helpers", "two_rank_guard_step.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=800)
    assert out.returncode == 0 and "TWO_RANK_GUARD_STEP_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


# ------------------------------------------------------------------------------------------ 10. resume
def test_checkpoint_resume_with_the_guard_is_exact(vds, tmp_path, request):
    """deterministic mode, clip + skip + EMA, one skipped step before the save: save / load / continue is bit-equal to
    the uninterrupted run in parameters, moments, EMA and skipped count"""
    from video_diffusion_speedrun_amd import checkpoint as ck
    vds["ops"].set_deterministic(True, 256 << 20)
    request.addfinalizer(lambda: vds["ops"].set_deterministic(False))
    cfg = small_cfg()
    P = O.init_params(cfg, seed=41, randomize_zero_init=True, init_std_factor=1.0)
    batch = _batch(3)
    bad = dict(batch, latent=batch["latent"].clone())
    bad["latent"][0, 0, 0, 0, 0] = float("nan")

    def fresh(Pinit):
        m = build(vds, cfg, Pinit)
        groups, _ = m.get_mup_setup(3e-3, 0.1, CONSTS)
        return m, vds["optim"].MuAdamW(groups, betas=(0.95, 0.99), max_grad_norm=0.05, skip_nonfinite=True, ema_decay=0.9)

    def step(m, opt, s, b=batch):
        gen = torch.Generator(device="cuda").manual_seed(100 + s)
        torch.manual_seed(0)
        return vds["train"].train_step(m, opt, None, b, "cuda", generator=gen, rope_start=(1, 2, 3)).item()

    def moments(m, opt):
        return {n: (opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), opt.state[p]["ema"].clone())
                for n, p in m.named_parameters()}

    m, opt = fresh(P)
    step(m, opt, 0)
    step(m, opt, 1, bad)  # skipped
    assert opt.skipped_steps() == 1
    step(m, opt, 2)
    ck.save_checkpoint(str(tmp_path / "c"), m, opt, step=3)
    l4 = step(m, opt, 3)
    ref, ref_st = m.full_state_dict(), moments(m, opt)
    m2, opt2 = fresh(O.init_params(cfg, seed=42, randomize_zero_init=True, init_std_factor=1.0))
    step(m2, opt2, 0)  # materialise the flat groups and the optimizer state before loading into them
    assert ck.load_checkpoint(str(tmp_path / "c"), m2, opt2) == 3
    assert opt2.skipped_steps() == 1 and opt2._step == 3
    l4b = step(m2, opt2, 3)
    assert l4 == l4b, (l4, l4b)
    got, got_st = m2.full_state_dict(), moments(m2, opt2)
    for k in ref:
        assert same_bits(got[k], ref[k]), k
        assert all(same_bits(a, b) for a, b in zip(got_st[k], ref_st[k])), k
    assert opt2.skipped_steps() == opt.skipped_steps() == 1
