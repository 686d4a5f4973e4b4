"""LoRA on the GPU, model level: tiny DiTs (hidden 128 = 2 heads of 64 and hidden 144 = 2 heads of 72, depth 2, latents
[2,16,2,8,8] with (pt, p) = (1, 2): 48 rows per sample, context [2,8,64]).

  * fresh adapters (B = 0) leave output and loss equal to the model before add_lora;
  * random adapters against the fp32 oracle run on the merged weights W + s B A with A, B as autograd leaves (the fp32
    restatement of the adapted model): output, loss, every adapter gradient, and through the reference-signature block
    call the input-side gradients dx, dc, dv_0 -- at the bounds of tests/test_model_gpu.py::test_oracle_parity_random
    (output max(2.5 e_ref, 1.5e-2), loss 1e-2, gradients cosine >= 0.999 and rel <= 3e-2); merge_lora() within the same;
  * frozen parameters: no .grad, exactly one weight-gradient GEMM fewer per frozen matrix (profiler class counts), and
    freezing one parameter leaves every other gradient bit-equal in deterministic mode;
  * recomputation bit for bit; three guarded MuAdamW steps on the adapter groups; GraphedTrainStep replay against eager;
  * all the attention / conditioning variants in one model, and a cached rollout, against the merged model."""
import os
import sys

import pytest
import torch

from oracle import dit_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lora_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
GRAD_COS, GRAD_REL = 0.999, 3e-2          # tests/test_model_gpu.py
B_OUT, B_LOSS = 2.5e-2, 1e-2              # tests/test_frame_causal_gpu.py: the model bound of the masked-model tests
START = (2, 3, 4)
TARGETS = ("qkv", "q_cross", "context_kv")
RANK, ALPHA = 16, 8.0
S = ALPHA / RANK


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import graph, model, ops, optim, sampling, train
    return dict(model=model, ops=ops, optim=optim, train=train, sampling=sampling, graph=graph)


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


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


_cases = {}


def case(name):
    """cfg, parameters, inputs and random adapter values of one model shape, built once"""
    if name not in _cases:
        hidden = {"hd64": 128, "hd72": 144}[name]
        cfg = O.DiTConfig(in_channels=16, patch_size=2, time_patch_size=1, hidden_size=hidden, depth=2, num_heads=2,
                          cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False)
        P = O.init_params(cfg, seed=21 + hidden, randomize_zero_init=True, init_std_factor=1.0)
        # gates x 8 and adapters of the size of the weights they sit on: the attention branches then carry enough of the
        # output for the adapters to move it by ~0.2 (fp32 oracle, with against without), 8 x the output bound
        for k in P:
            if "adaLN_modulation.1" in k:
                P[k] = P[k] * 8
        g = torch.Generator().manual_seed(hidden)
        x = torch.randn(2, 16, 2, 8, 8, generator=g).to(bf16)
        ctx = torch.randn(2, 8, 64, generator=g).to(bf16)
        t = O.time_shift(torch.randn(2, generator=g)).to(bf16)
        v = torch.randn(2, 16, 2, 8, 8, generator=g).to(bf16)
        ad = {}
        for i in range(cfg.depth):
            for tg, (out, inn) in {"qkv": (3 * hidden, hidden), "q_cross": (hidden, hidden),
                                   "context_kv": (2 * hidden, 64)}.items():
                ad[f"blocks.{i}.{tg}.lora_A"] = torch.randn(RANK, inn, generator=g) * inn ** -0.5
                ad[f"blocks.{i}.{tg}.lora_B"] = torch.randn(out, RANK, generator=g) * 0.5
        _cases[name] = dict(cfg=cfg, P=P, x=x, ctx=ctx, t=t, v=v, ad=ad)
    return _cases[name]


def build(vds, cs, lora=True, adapters=True, freeze_base=True, **kw):
    cfg = cs["cfg"]
    m = vds["model"].DiT(in_channels=cfg.in_channels, patch_size=cfg.patch_size, time_patch_size=cfg.time_patch_size,
                         hidden_size=cfg.hidden_size, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
                         cross_attn_input_size=cfg.cross_attn_input_size, residual_v=cfg.residual_v,
                         train_bias_and_rms=cfg.train_bias_and_rms, **kw)
    m.load_state_dict(cs["P"], strict=True)
    m = m.to("cuda")
    if lora:
        m.add_lora(rank=RANK, alpha=ALPHA, targets=TARGETS, freeze_base=freeze_base,
                   generator=torch.Generator().manual_seed(1))
        if adapters:
            m.load_lora_state_dict(dict(cs["ad"], rank=RANK, alpha=ALPHA, targets=list(TARGETS)))
    return m


def step(vds, m, cs, timesteps=None):
    m.zero_grad()
    out = m(cs["x"].cuda(), cs["ctx"].cuda(), (cs["t"] if timesteps is None else timesteps).cuda(), rope_start=START)
    loss, _ = vds["train"].flow_loss(out, cs["v"].cuda())
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().clone(), loss.item(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def merged_params(P, ad, leaves=False):
    """(oracle parameters with W + s B A on the adapted linears, the adapter leaves, the merged weights)"""
    Pg = {k: w.clone().requires_grad_(leaves) for k, w in P.items()}
    Ad = {k: w.clone().requires_grad_(leaves) for k, w in ad.items()}
    eff = {}
    for k in Ad:
        if k.endswith(".lora_A"):
            lin = k[:-len(".lora_A")]
            eff[lin + ".weight"] = Pg[lin + ".weight"] + S * (Ad[lin + ".lora_B"] @ Ad[k])
            if leaves:
                eff[lin + ".weight"].retain_grad()
    return dict(Pg, **eff), Ad, eff


_refs = {}


def reference(name):
    """the fp32 restatement of the adapted model, one step, once per shape; e_ref = its own bf16-vs-fp32 distance"""
    if name not in _refs:
        cs = case(name)
        Pe, Ad, eff = merged_params(cs["P"], cs["ad"], leaves=True)
        out = O.dit_forward(Pe, cs["cfg"], cs["x"].float(), cs["ctx"].float(), cs["t"].float(), START)
        loss, _ = O.flow_loss(cs["v"], out)
        loss.backward()
        with torch.no_grad():
            Pb = {k: w.detach().to(bf16) for k, w in merged_params(cs["P"], cs["ad"])[0].items()}
            e_ref = rel(O.dit_forward(Pb, cs["cfg"], cs["x"], cs["ctx"], cs["t"], START), out)
        _refs[name] = dict(out=out.detach(), loss=loss.item(), grads={k: w.grad for k, w in Ad.items()},
                           wgrads={k: w.grad for k, w in eff.items()}, e_ref=e_ref)
    return _refs[name]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hd64", "hd72"])
def test_fresh_adapters_change_nothing(vds, name):
    cs = case(name)
    m = build(vds, cs, lora=False)
    with torch.no_grad():
        out0 = m(cs["x"].cuda(), cs["ctx"].cuda(), cs["t"].cuda(), rope_start=START)
        loss0, _ = vds["train"].flow_loss(out0, cs["v"].cuda())
    m.add_lora(rank=RANK, alpha=ALPHA)
    out1, loss1, grads = step(vds, m, cs)
    assert torch.equal(out1, out0) and loss1 == loss0.item()
    assert set(grads) == {n for n, _ in m.lora_parameters()}
    # B = 0: dA = 0 exactly, dB is the first thing to move
    assert all(float(g.abs().max()) == 0 for k, g in grads.items() if k.endswith("lora_A"))
    assert all(float(g.abs().max()) > 0 for k, g in grads.items() if k.endswith("lora_B"))


@pytest.mark.parametrize("name", ["hd64", "hd72"])
def test_random_adapters_against_the_fp32_restatement(vds, name, parity_log):
    cs, ref = case(name), reference(name)
    m = build(vds, cs)
    out, loss, grads = step(vds, m, cs)
    e_out, e_loss = rel(out, ref["out"]), abs(loss - ref["loss"]) / ref["loss"]
    # the adapters matter here: without them the output is far outside the bound
    plain = build(vds, cs, lora=False)
    with torch.no_grad():
        d_plain = rel(plain(cs["x"].cuda(), cs["ctx"].cuda(), cs["t"].cuda(), rope_start=START), ref["out"])
    rows = [(k, cosine(grads[k], ref["grads"][k]), rel(grads[k], ref["grads"][k])) for k in ref["grads"]]
    worst = max(rows, key=lambda r: r[2])
    print(f"{name}: out {e_out:.3e} (e_ref {ref['e_ref']:.3e}; without adapters {d_plain:.3f}), loss {e_loss:.2e}, "
          f"worst adapter grad {worst}")
    assert d_plain >= 4 * B_OUT, d_plain
    assert e_out <= max(2.5 * ref["e_ref"], 1.5e-2), (e_out, ref["e_ref"])
    assert e_loss <= 1e-2, e_loss
    assert set(grads) == set(ref["grads"])
    bad = [r for r in rows if not (r[1] >= GRAD_COS and r[2] <= GRAD_REL)]
    assert not bad, bad
    # merged: the same model without adapters, within the same bounds of the same restatement
    mm = build(vds, cs).merge_lora()
    assert mm.lora is None and set(mm.state_dict()) == set(cs["P"])
    out_m, loss_m, grads_m = step(vds, mm, cs)
    e_out_m, e_loss_m = rel(out_m, ref["out"]), abs(loss_m - ref["loss"]) / ref["loss"]
    rows_m = [(k, cosine(grads_m[k], g), rel(grads_m[k], g)) for k, g in ref["wgrads"].items()]
    assert e_out_m <= max(2.5 * ref["e_ref"], 1.5e-2) and e_loss_m <= 1e-2, (e_out_m, e_loss_m)
    bad = [r for r in rows_m if not (r[1] >= GRAD_COS and r[2] <= GRAD_REL)]
    assert not bad, bad
    parity_log("test_lora_gpu.random_adapters." + name, out=e_out, e_ref=ref["e_ref"], loss=e_loss,
               worst_adapter_grad=worst, merged_out=e_out_m, merged_loss=e_loss_m,
               merged_worst_wgrad=max(rows_m, key=lambda r: r[2]))


@pytest.mark.parametrize("name", ["hd64", "hd72"])
def test_input_side_gradients_of_an_adapted_block(vds, name, parity_log):
    """block 1 of the adapted model through the reference-signature call: dx, dc and dv_0 against the fp32 block"""
    cs = case(name)
    cfg = cs["cfg"]
    D, H, hd = cfg.hidden_size, cfg.num_heads, cfg.head_dim
    g = torch.Generator().manual_seed(77)
    B, L = 2, 16 + 32
    x = torch.randn(B, L, D, generator=g).to(bf16)
    c = torch.randn(B, D, generator=g).to(bf16)
    v0 = torch.randn(B, H, L, hd, generator=g).to(bf16)
    gx = torch.randn(B, L, D, generator=g).to(bf16)
    cos, sin = O.rope_cos_sin(hd, (2, 4, 4), START, 16)
    Pe, _, _ = merged_params(cs["P"], cs["ad"])
    xo, co, vo = (t.float().requires_grad_(True) for t in (x, c, v0))
    y_ref, _ = O.block_forward(Pe, "blocks.1.", cfg, xo, cs["ctx"].float(), co, vo, cos, sin)
    (y_ref * gx.float()).sum().backward()
    blk = build(vds, cs).blocks[1]
    xh, ch, vh = (t.cuda().requires_grad_(True) for t in (x, c, v0))
    y, _ = blk(xh, cs["ctx"].cuda(), ch, v_0=vh, rope=(cos[None, None].cuda(), sin[None, None].cuda()))
    (y.float() * gx.cuda().float()).sum().backward()
    rows = {"y": rel(y, y_ref.detach()), "dx": rel(xh.grad, xo.grad), "dc": rel(ch.grad, co.grad),
            "dv0": rel(vh.grad, vo.grad)}
    print(name, rows)
    parity_log("test_lora_gpu.block_inputs." + name, **rows)
    assert rows["y"] <= 1.5e-2 and max(rows["dx"], rows["dc"], rows["dv0"]) <= GRAD_REL, rows
    assert min(cosine(xh.grad, xo.grad), cosine(ch.grad, co.grad), cosine(vh.grad, vo.grad)) >= GRAD_COS
    assert all(p.grad is None for n, p in blk.named_parameters() if "lora_" not in n)
    assert all(p.grad is not None for n, p in blk.named_parameters() if "lora_" in n)


# ---------------------------------------------------------------------------------------------- frozen parameters ----
def test_frozen_parameters_get_no_grad_and_no_weight_gradient_gemm(vds):
    cs = case("hd72")
    ops = vds["ops"]
    counts = {}
    for frozen in (False, True):
        m = build(vds, cs, freeze_base=frozen)
        step(vds, m, cs)  # (first call: flat groups, allocator)
        ops.prof_enable()
        try:
            _, _, grads = step(vds, m, cs)
            counts[frozen] = ops.prof_collect()
        finally:
            ops.prof_enable(0)
        named = dict(m.named_parameters())
        if frozen:
            assert all((p.grad is None) == ("lora_" not in n) for n, p in named.items())
        else:
            assert all(p.grad is not None for p in named.values())
    depth = cs["cfg"].depth
    n_frozen_matrices = 7 * depth + 2  # the block linears, patch_proj, final_proj: the weight gradients that are GEMMs
    tn = {k: v.get("gemm_tn", {"launches": 0})["launches"] for k, v in counts.items()}
    assert tn[False] - tn[True] == n_frozen_matrices, tn
    assert tn[True] == 0  # nothing but adapters trains: no weight-gradient GEMM is left
    # the data-gradient GEMMs and the forward are what they were
    assert counts[False]["gemm_nn"]["launches"] == counts[True]["gemm_nn"]["launches"]
    assert counts[False]["gemm_nt"]["launches"] == counts[True]["gemm_nt"]["launches"]


@pytest.mark.parametrize("which", ["blocks.1.mlp.0.weight", "blocks.0.context_kv.weight", "patch_embed.patch_proj.weight",
                                   "final_proj.bias", "blocks.0.lambda_param"])
def test_one_frozen_parameter_leaves_the_other_gradients_bit_equal(vds, deterministic, which):
    cs = case("hd64")
    if "base" not in cs:
        cs["base"] = step(vds, build(vds, cs, lora=False), cs)
    out0, loss0, g0 = cs["base"]
    m = build(vds, cs, lora=False)
    dict(m.named_parameters())[which].requires_grad_(False)
    out1, loss1, g1 = step(vds, m, cs)
    assert torch.equal(out1, out0) and loss1 == loss0
    assert set(g1) == set(g0) - {which}
    for k in g1:
        assert torch.equal(bits(g1[k]), bits(g0[k])), k


@pytest.mark.parametrize("mode", ["full", "selective"])
def test_recompute_is_bit_equal(vds, deterministic, mode):
    cs = case("hd72")
    if "det" not in cs:
        cs["det"] = step(vds, build(vds, cs), cs)
    out0, loss0, g0 = cs["det"]
    out1, loss1, g1 = step(vds, build(vds, cs).enable_recompute(mode), cs)
    assert torch.equal(out1, out0) and loss1 == loss0 and set(g1) == set(g0)
    for k in g0:
        assert torch.equal(bits(g1[k]), bits(g0[k])), k


# ------------------------------------------------------------------------------------------- optimizer and graph ----
def test_guarded_muadamw_steps_on_the_adapter_groups(vds):
    cs = case("hd64")
    m = build(vds, cs, adapters=False)
    groups, table = m.get_lora_setup(2e-3, 0.01)
    assert set(table) == {n for n, _ in m.lora_parameters()}
    opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99), max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.9)
    losses = []
    base0 = None
    for i in range(4):
        opt.zero_grad()
        out = m(cs["x"].cuda(), cs["ctx"].cuda(), cs["t"].cuda(), rope_start=START)
        loss, _ = vds["train"].flow_loss(out, cs["v"].cuda())
        losses.append(loss.item())
        if i == 3:
            break
        loss.backward()
        if base0 is None:
            base0 = {k: v.clone() for k, v in m.full_state_dict().items() if "lora_" not in k}
        opt.step()
    assert losses[3] < losses[0] and all(l == l for l in losses), losses
    assert opt.skipped_steps() == 0 and float(opt.grad_norm) > 0
    after = m.full_state_dict()
    for k, w in base0.items():
        assert torch.equal(bits(after[k]), bits(w)), k
    assert any(float(after[k].abs().max()) > 0 for k in after if k.endswith("lora_B"))
    assert set(opt.ema_named(m)) == set(table)


def test_graph_replay_matches_eager_steps(vds):
    """tests/test_model_gpu.py::test_graph_replay_matches_eager_steps on the adapted model and its adapter groups"""
    cs = case("hd64")
    g = torch.Generator().manual_seed(5)
    batches = [{"latent": torch.randn(2, 16, 2, 8, 8, generator=g).cuda(), "context": torch.randn(2, 8, 64, generator=g).cuda(),
                "prompt": ["", ""]} for _ in range(5)]
    results = []
    for graphed in (False, True):
        m = build(vds, cs)
        groups, _ = m.get_lora_setup(3e-3, 0.0)
        opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99))
        sched = vds["train"].get_schedule(opt, "cosine", 3, 50)
        torch.manual_seed(77)
        torch.cuda.manual_seed(77)
        losses = []
        if graphed:
            gs = vds["graph"].GraphedTrainStep(m, opt, sched, "cuda", eager_steps=2)
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
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    for k in p0:
        assert rel(p1[k], p0[k]) <= 2e-4, (k, rel(p1[k], p0[k]))
    assert any(not torch.equal(p0[k].cpu(), cs["ad"][k]) for k in cs["ad"])  # the adapters did train


# ------------------------------------------------------------------------------------------------- composition ----
FLAGS = dict(frame_causal=True, frame_major=True, frame_chunk=2, frame_window=2, qk_norm=True)


def test_composes_with_the_attention_and_conditioning_variants(vds):
    """frame-causal + frame-major + chunk + window + QK-norm + per-frame timesteps + context_lens in one adapted model
    against that model merged"""
    cs = case("hd72")
    ts = torch.tensor([[0.25, 0.9375], [0.5, 0.0625]]).to(bf16)
    res = []
    for merged in (False, True):
        m = build(vds, cs, **FLAGS)
        if merged:
            m.merge_lora()
        m.zero_grad()
        out = m(cs["x"].cuda(), cs["ctx"].cuda(), ts.cuda(), rope_start=START, context_lens=[5, 8])
        loss, _ = vds["train"].flow_loss(out, cs["v"].cuda())
        loss.backward()
        res.append((out.detach(), loss.item(), m))
    (o_l, l_l, m_l), (o_m, l_m, _) = res
    e_out, e_loss = rel(o_l, o_m), abs(l_l - l_m) / abs(l_m)
    print(f"composition: adapted vs merged out {e_out:.3e} loss {e_loss:.2e}")
    assert torch.isfinite(o_l.float()).all() and e_out <= B_OUT and e_loss <= B_LOSS, (e_out, e_loss)
    grads = {n: p.grad for n, p in m_l.lora_parameters()}
    assert all(g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0 for g in grads.values())
    # and the adapters are not a no-op in this model either
    plain = build(vds, cs, lora=False, **FLAGS)
    with torch.no_grad():
        o_p = plain(cs["x"].cuda(), cs["ctx"].cuda(), ts.cuda(), rope_start=START, context_lens=[5, 8])
    assert rel(o_p, o_m) >= 2 * B_OUT, rel(o_p, o_m)


def test_cached_rollout_against_the_merged_model(vds):
    """generate_latents(kv_cache=True): two chunks of two token-frames on the adapted model and on the merged one"""
    Smp = vds["sampling"]
    cs = case("hd72")
    g = torch.Generator().manual_seed(8)
    prompt = torch.randn(1, 8, 64, generator=g).to(bf16)
    lat0 = torch.randn(1, 16, 4, 8, 8, generator=g).to(bf16)
    flags = dict(frame_causal=True, frame_major=True, frame_chunk=2)
    kw = dict(latents=lat0.cuda(), inference_steps=2, cfg_scale=3.0, rollout_frames=2, rope_starts=[(1, 2, 3)], kv_cache=True)
    a = Smp.generate_latents(build(vds, cs, **flags), prompt.cuda(), **kw)
    b = Smp.generate_latents(build(vds, cs, **flags).merge_lora(), prompt.cuda(), **kw)
    c = Smp.generate_latents(build(vds, cs, lora=False, **flags), prompt.cuda(), **kw)
    e = rel(a, b)
    print(f"cached rollout: adapted vs merged {e:.3e} (bound {B_OUT:.1e}); without adapters {rel(c, b):.3f}")
    assert tuple(a.shape) == (1, 16, 4, 8, 8) and torch.isfinite(a).all()
    assert e <= B_OUT, e
    assert rel(c, b) >= 2 * B_OUT, rel(c, b)
