"""Per-sample context lengths through the model, the recompute replay, the harness, the captured step and the sampler.

Reference: the fp32 CPU oracle run ONE SAMPLE AT A TIME on the truncated context, O.dit_forward(P, cfg, x[b:b+1],
ctx[b:b+1, :n_b], t[b:b+1], start); the per-sample O.flow_loss results are averaged over B and the gradients come from
that mean.  Tolerances are those tests/test_model_gpu.py states for the same quantities: output within
max(2.5 * e_ref, 1.5e-2) with e_ref from the oracle's own bf16 run, loss within 1e-2, parameter gradients within
GRAD_COS / GRAD_REL, lambda_param excluded as in that file."""
import pytest
import torch

from oracle import dit_oracle as O

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
GRAD_COS, GRAD_REL = 0.999, 3e-2  # tests/test_model_gpu.py


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import model, ops, optim, sampling, train
    return dict(model=model, ops=ops, optim=optim, sampling=sampling, train=train)


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


def build(vds, cfg, P):
    m = vds["model"].DiT(in_channels=cfg.in_channels, patch_size=cfg.patch_size, time_patch_size=cfg.time_patch_size,
                         hidden_size=cfg.hidden_size, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
                         cross_attn_input_size=cfg.cross_attn_input_size, residual_v=cfg.residual_v,
                         train_bias_and_rms=cfg.train_bias_and_rms)
    m.load_state_dict(P, strict=True)
    return m.to("cuda")


LENS = [24, 9, 1]
START = (5, 9, 17)
_cases = {}


def case(hd, H=2):
    """base configuration, inputs and the oracle's masked results -- made once per head dim, shared, never modified"""
    if hd in _cases:
        return _cases[hd]
    cfg = O.DiTConfig(in_channels=16, patch_size=2, time_patch_size=1, hidden_size=hd * H, depth=2, num_heads=H,
                      cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False)
    P = O.init_params(cfg, seed=11, randomize_zero_init=True, init_std_factor=0.5)
    g = torch.Generator().manual_seed(12)
    B = 3
    x = torch.randn(B, 16, 2, 8, 8, generator=g).to(bf16)
    ctx = torch.randn(B, 24, 64, generator=g).to(bf16)
    t = O.time_shift(torch.randn(B, generator=g)).to(bf16)
    v = torch.randn(B, 16, 2, 8, 8, generator=g).to(bf16)
    Pg = {k: w.clone().requires_grad_(True) for k, w in P.items()}
    Pb = {k: w.to(bf16) for k, w in P.items()}
    outs, outs_bf, losses = [], [], []
    for b, n in enumerate(LENS):
        o = O.dit_forward(Pg, cfg, x[b:b + 1].float(), ctx[b:b + 1, :n].float(), t[b:b + 1].float(), START)
        outs.append(o)
        losses.append(O.flow_loss(v[b:b + 1], o)[0])
        with torch.no_grad():
            outs_bf.append(O.dit_forward(Pb, cfg, x[b:b + 1], ctx[b:b + 1, :n], t[b:b + 1], START))
    l_ref = torch.stack(losses).mean()
    l_ref.backward()
    o_ref = torch.cat(outs).detach()
    _cases[hd] = dict(cfg=cfg, P=P, x=x, ctx=ctx, t=t, v=v, o_ref=o_ref, e_ref=rel(torch.cat(outs_bf), o_ref),
                      l_ref=l_ref.item(), grads={k: w.grad for k, w in Pg.items() if w.grad is not None})
    return _cases[hd]


@pytest.mark.parametrize("hd", [64, 72])
def test_masked_model_matches_the_oracle_on_truncated_contexts(vds, hd):
    c = case(hd)
    m = build(vds, c["cfg"], c["P"])
    out = m(c["x"].cuda(), c["ctx"].cuda(), c["t"].cuda(), rope_start=START, context_lens=LENS)
    e = rel(out, c["o_ref"])
    print(f"hd{hd}: out rel {e:.3e} (e_ref {c['e_ref']:.3e})")
    assert e <= max(2.5 * c["e_ref"], 1.5e-2), (e, c["e_ref"])
    loss, _ = vds["train"].flow_loss(out, c["v"].cuda())
    assert abs(loss.item() - c["l_ref"]) / c["l_ref"] <= 1e-2, (loss.item(), c["l_ref"])
    loss.backward()
    bad = []
    for k, p in m.named_parameters():
        if k not in c["grads"] or k.endswith("lambda_param"):
            continue
        cs, er = cosine(p.grad, c["grads"][k]), rel(p.grad, c["grads"][k])
        if not (cs >= GRAD_COS and er <= GRAD_REL):
            bad.append((k, cs, er))
    assert not bad, bad


@pytest.mark.parametrize("hd", [64, 72])
def test_recompute_replays_with_the_same_lengths(vds, deterministic, hd):
    """enable_recompute("selective" | "full"): gradients bit-identical to the non-recomputing masked run"""
    c = case(hd)
    x, ctx, t, v = c["x"].cuda(), c["ctx"].cuda(), c["t"].cuda(), c["v"].cuda()

    def run(mode):
        m = build(vds, c["cfg"], c["P"]).enable_recompute(mode)
        out = m(x, ctx, t, rope_start=START, context_lens=LENS)
        loss, _ = vds["train"].flow_loss(out, v)
        loss.backward()
        torch.cuda.synchronize()
        return loss.item(), out.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}

    l0, o0, g0 = run("none")
    for mode in ("selective", "full"):
        l1, o1, g1 = run(mode)
        assert l1 == l0 and torch.equal(o1, o0), mode
        diff = [k for k in g0 if not torch.equal(g1[k], g0[k])]
        assert not diff, (mode, diff)


def test_input_forms(vds):
    c = case(72)
    m = build(vds, c["cfg"], c["P"])
    x, ctx, t = c["x"].cuda(), c["ctx"].cuda(), c["t"].cuda()
    with torch.no_grad():
        a = m(x, ctx, t, rope_start=START, context_lens=LENS)
        b = m(x, ctx, t, rope_start=START, context_lens=torch.tensor(LENS, dtype=torch.int32, device="cuda"))
        d = m(x, ctx, t, rope_start=START, context_lens=torch.tensor(LENS))  # CPU int64
        assert torch.equal(a, b) and torch.equal(a, d)
        # without lengths: the untouched path, whether the keyword is absent or None
        assert torch.equal(m(x, ctx, t, rope_start=START, context_lens=None), m(x, ctx, t, rope_start=START))
        assert not torch.equal(a, m(x, ctx, t, rope_start=START))


def test_block_forward_with_lengths_matches_the_oracle_block(vds):
    M = vds["model"]
    cfg = O.DiTConfig(in_channels=16, hidden_size=144, depth=1, num_heads=2, cross_attn_input_size=64,
                      residual_v=True, train_bias_and_rms=True)
    P = O.init_params(cfg, seed=5, randomize_zero_init=True, init_std_factor=1.0)
    g = torch.Generator().manual_seed(6)
    B, L, Lc, D, hd = 3, 16 + 64, 24, 144, 72
    x = torch.randn(B, L, D, generator=g).to(bf16)
    ctx = torch.randn(B, Lc, 64, generator=g).to(bf16)
    cv = torch.randn(B, D, generator=g).to(bf16)
    gx = torch.randn(B, L, D, generator=g).to(bf16)
    cos, sin = O.rope_cos_sin(hd, (4, 4, 4), (3, 5, 7), 16)
    leaf = {k: w.clone().requires_grad_(True) for k, w in P.items() if k.startswith("blocks.")}
    xo = x.float().requires_grad_(True)
    ys = [O.block_forward(leaf, "blocks.0.", cfg, xo[b:b + 1], ctx[b:b + 1, :n].float(), cv[b:b + 1].float(), None, cos, sin)[0]
          for b, n in enumerate(LENS)]
    y_ref = torch.cat(ys)
    (y_ref * gx.float()).sum().backward()
    blk = M.DiTBlock(hidden_size=D, cross_attn_input_size=64, num_heads=2, mlp_ratio=cfg.mlp_ratio, qkv_bias=True,
                     residual_v=True)
    blk.load_state_dict({k[len("blocks.0."):]: w for k, w in P.items() if k.startswith("blocks.0.")}, strict=True)
    blk = blk.cuda()
    xh = x.cuda().requires_grad_(True)
    y, _ = blk(xh, ctx.cuda(), cv.cuda(), v_0=None, rope=(cos[None, None].cuda(), sin[None, None].cuda()), context_lens=LENS)
    assert rel(y, y_ref.detach()) <= 1.5e-2, rel(y, y_ref.detach())
    (y.float() * gx.cuda().float()).sum().backward()
    assert rel(xh.grad, xo.grad) <= GRAD_REL, rel(xh.grad, xo.grad)
    bad = [(n, rel(p.grad, leaf["blocks.0." + n].grad)) for n, p in blk.named_parameters()
           if leaf["blocks.0." + n].grad is not None and n != "lambda_param"
           and rel(p.grad, leaf["blocks.0." + n].grad) > GRAD_REL]
    assert not bad, bad


def test_fp8_with_lengths(vds):
    cfg = O.DiTConfig(in_channels=16, hidden_size=144, depth=2, num_heads=2, cross_attn_input_size=64,
                      residual_v=True, train_bias_and_rms=False)
    P = O.init_params(cfg, seed=3, randomize_zero_init=True, init_std_factor=1.0)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3, 16, 4, 8, 8, generator=g).to(bf16).cuda()
    ctx = torch.randn(3, 24, 64, generator=g).to(bf16).cuda()
    t = torch.rand(3, generator=g).to(bf16).cuda()
    m = build(vds, cfg, P).enable_fp8()
    with pytest.raises(NotImplementedError, match=r"enable_fp8\(cross_attention=False\)"):
        m(x, ctx, t, rope_start=START, context_lens=LENS)
    m = build(vds, cfg, P).enable_fp8(cross_attention=False)
    for _ in range(2):  # the second step runs with delayed scaling armed
        out = m(x, ctx, t, rope_start=START, context_lens=LENS)
        out.float().pow(2).mean().backward()
        assert torch.isfinite(out.float()).all()
        assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
        m.zero_grad()


def _harness_model(vds, seed=41, depth=2):
    cfg = O.DiTConfig(in_channels=16, hidden_size=128, depth=depth, num_heads=2, cross_attn_input_size=64,
                      residual_v=True, train_bias_and_rms=False)
    return cfg, O.init_params(cfg, seed=seed, randomize_zero_init=True, init_std_factor=1.0)


def test_train_forward_drops_a_caption_to_length_zero(vds, monkeypatch):
    train = vds["train"]
    cfg, P = _harness_model(vds)
    m = build(vds, cfg, P)
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(3, 16, 4, 8, 8, generator=g).cuda()
    ctx = torch.randn(3, 16, 64, generator=g).cuda()

    def losses(drop, batch):
        # the caption-drop draw is the one torch.rand(B, device=...) call of train.forward (a sample drops below 0.01)
        monkeypatch.setattr(train.torch, "rand", lambda n, device=None: torch.tensor(drop, device=device))
        torch.manual_seed(9)
        torch.cuda.manual_seed(9)
        with torch.no_grad():
            return train.forward(m, batch, None, None, "cuda", 0, False, rope_start=START)[0].item()

    dropped = losses([1.0, 0.0, 1.0], {"latent": lat, "context": ctx, "context_lens": [16, 7, 3]})
    ctx0 = ctx.clone()
    ctx0[1] = 0
    by_hand = losses([1.0, 1.0, 1.0], {"latent": lat, "context": ctx0, "context_lens": [16, 0, 3]})
    kept = losses([1.0, 1.0, 1.0], {"latent": lat, "context": ctx, "context_lens": [16, 7, 3]})
    assert dropped == by_hand, (dropped, by_hand)
    assert dropped != kept


def test_graphed_train_step_with_lengths(vds):
    """two eager steps and two replays with different context_lens per batch == an eager model stepped on the same batches
    (the standard of test_graph_replay_matches_eager_steps); dropping the key afterwards is refused"""
    from video_diffusion_speedrun_amd.graph import GraphedTrainStep
    cfg, P = _harness_model(vds, depth=3)
    g = torch.Generator().manual_seed(5)
    lens = [[16, 5], [1, 12], [9, 0], [3, 16]]
    batches = [{"latent": torch.randn(2, 16, 4, 8, 8, generator=g).cuda(), "context": torch.randn(2, 16, 64, generator=g).cuda(),
                "context_lens": n} for n in lens]
    results = []
    for graphed in (False, True):
        m = build(vds, cfg, P)
        groups, _ = m.get_mup_setup(3e-3, 0.1, ["patch_proj", "context_kv", "positional_embedding"])
        opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99))
        sched = vds["train"].get_schedule(opt, "cosine", 3, 50)
        torch.manual_seed(77)
        torch.cuda.manual_seed(77)
        if graphed:
            gs = GraphedTrainStep(m, opt, sched, "cuda", eager_steps=2)
            losses = [gs.step(b).item() for b in batches]
            assert gs.n_replays == 2
            with pytest.raises(ValueError):
                gs.step({k: v for k, v in batches[0].items() if k != "context_lens"})
        else:
            losses = [vds["train"].train_step(m, opt, sched, b, "cuda").item() for b in batches]
        torch.cuda.synchronize()
        results.append((losses, {k: v.clone() for k, v in m.full_state_dict().items()}))
    (l0, p0), (l1, p1) = results
    assert len(set(l0)) == 4
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    for k in p0:
        assert rel(p1[k], p0[k]) <= 2e-4, (k, rel(p1[k], p0[k]))


def test_generate_latents_with_an_empty_negative_prompt(vds):
    """prompt_lens=[7], no negative prompt: the result is that of calling the model step by step with lengths [7, 0]"""
    S, ops = vds["sampling"], vds["ops"]
    cfg, P = _harness_model(vds)
    m = build(vds, cfg, P)
    g = torch.Generator().manual_seed(8)
    prompt = torch.randn(1, 12, 64, generator=g).to(bf16).cuda()
    lat0 = torch.randn(1, 16, 4, 8, 8, generator=g).to(bf16).cuda()
    steps, scale = 3, 4.0
    starts = [(1, 2, 3), (1, 2, 3), (4, 5, 6), (4, 5, 6), (7, 8, 9), (7, 8, 9)]  # equal within a step: the batched form
    acc = S.generate_latents(m, prompt, inference_steps=steps, cfg_scale=scale, latents=lat0, rope_starts=starts,
                             prompt_lens=[7])
    lat = lat0.clone()
    ref = lat.to(f32)
    lens = torch.tensor([7, 0], dtype=torch.int32, device="cuda")
    with torch.no_grad():
        for j, i in enumerate(range(steps, 0, -1)):
            tt, tn = S.shifted_times(i, steps)
            out = m(torch.cat([lat, lat]), torch.cat([prompt, torch.zeros_like(prompt)]),
                    torch.tensor([tt, tt], device="cuda").to(bf16), rope_start=starts[2 * j], context_lens=lens)
            ops.cfg_euler_step(out[0:1].contiguous(), out[1:2].contiguous(), ref, lat, scale, tt - tn)
    assert torch.isfinite(acc).all()
    assert torch.equal(acc, ref)
    # the two-call form (distinct RoPE offsets inside a step) passes the lengths too: [7] and [0]
    starts2 = [(1, 2, 3), (3, 2, 1)] * steps
    acc2 = S.generate_latents(m, prompt, inference_steps=steps, cfg_scale=scale, latents=lat0, rope_starts=starts2,
                              prompt_lens=[7])
    lat, ref2 = lat0.clone(), lat0.to(f32)
    with torch.no_grad():
        for j, i in enumerate(range(steps, 0, -1)):
            tt, tn = S.shifted_times(i, steps)
            t1 = torch.tensor([tt], device="cuda").to(bf16)
            cond = m(lat, prompt, t1, rope_start=starts2[2 * j], context_lens=[7])
            unc = m(lat, torch.zeros_like(prompt), t1, rope_start=starts2[2 * j + 1], context_lens=[0])
            ops.cfg_euler_step(cond, unc, ref2, lat, scale, tt - tn)
    assert torch.isfinite(acc2).all() and torch.equal(acc2, ref2)
