"""Token routing on the GPU: DiT.enable_token_routing(1, 2, 0.5) on the depth-4 hd72 / hd64 cases of
tests/helpers/routing_ref.py (N = 256 tokens, L = 272, Ls = 144) against routed_forward at the project's bounds (output
2.5e-2, loss 1e-2, worst gradient 3e-2); both settings of the deferred-dv0 knob and a reduction inside the span; routes that
hold token 0 and token N - 1; bypassed and kept tokens perturbed; the switch off is the model itself, bit for bit and launch
for launch, and a routed step launches the three row movers a counted number of times; eval / no_grad run every token;
recomputation bit for bit; QK-norm, context_lens, LoRA, a second backward; determinism; GraphedTrainStep; train.forward.

Bounds.  B_OUT / B_LOSS / B_GRAD were set on depth-2 / 3 models; every comparison here first runs the UNROUTED model of this
depth-4 case -- the code path of before -- against the unrouted reference (`unrouted_errors`, printed).  Where that run
itself leaves a bound, the routed model gets 1.5 x the unrouted model's measured error for that quantity (the margin covers
the different summation lengths); the bound never comes from a routed run."""
import os
import sys
from contextlib import ExitStack

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import routing_ref as RR  # noqa: E402
from test_frame_causal_gpu import B_GRAD, B_LOSS, B_OUT, CONST, bits, build, rel, within_bounds  # noqa: E402,F401

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
START, SPAN, KEEP = RR.START, RR.SPAN, RR.KEEP
ENTRIES = ("vds_rows_gather", "vds_rows_merge", "vds_rows_scatter_add_f32")


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import _lib, graph, model, ops, optim, train
    return dict(model=model, ops=ops, optim=optim, train=train, lib=_lib, graph=graph)


@pytest.fixture
def deterministic(vds, request):
    vds["ops"].set_deterministic(True, 256 << 20)
    request.addfinalizer(lambda: vds["ops"].set_deterministic(False))


def routed_model(vds, cs, mode="none", P=None, **kw):
    return build(vds, cs["cfg"], cs["P"] if P is None else P, mode, frame_causal=False, **kw).enable_token_routing(*SPAN, KEEP)


def step(vds, m, cs, route, zero=True, **kw):
    """one step with [B] timesteps and the flow loss; route: the pinned subset, or False"""
    if zero:
        m.zero_grad()
    out = m(cs["zt"].cuda(), cs["ctx"].cuda(), cs["ts"].cuda(), rope_start=START, route=route, **kw)
    loss, _ = vds["train"].flow_loss(out, cs["v"].cuda())
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().clone(), loss.item(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def errors(out, loss, grads, ref):
    named = {k: rel(grads[k], ref["grads"][k]) for k in grads
             if k in ref["grads"] and not k.endswith("lambda_param") and float(ref["grads"][k].abs().max()) > 0}
    worst = max((v, k) for k, v in named.items())
    return rel(out, ref["out"]), abs(loss - ref["loss"]) / abs(ref["loss"]), worst, named


_unrouted = {}


def unrouted_errors(vds, name):
    """(e_out, e_loss, worst gradient error) of the UNROUTED model of this case against the unrouted reference, once"""
    if name not in _unrouted:
        cs = RR.case(name)
        m = build(vds, cs["cfg"], cs["P"], frame_causal=False)
        e_out, e_loss, worst, _ = errors(*step(vds, m, cs, None), RR.reference_step(name, route=None))
        print(f"{name} UNROUTED model vs unrouted reference: out {e_out:.3e}, loss {e_loss:.2e}, worst grad {worst[0]:.3e} "
              f"({worst[1]})")
        _unrouted[name] = (e_out, e_loss, worst[0])
    return _unrouted[name]


def bounds(vds, name):
    """the project's bounds, or 1.5 x the unrouted model's own error where that model leaves one (module docstring)"""
    return tuple(b if e <= b else 1.5 * e for b, e in zip((B_OUT, B_LOSS, B_GRAD), unrouted_errors(vds, name)))


def check(vds, name, tag, out, loss, grads, ref, also=()):
    b_out, b_loss, b_grad = bounds(vds, name)
    e_out, e_loss, worst, named = errors(out, loss, grads, ref)
    print(f"{name} {tag}: out {e_out:.3e} (<= {b_out:.3e}), loss {e_loss:.2e} (<= {b_loss:.2e}), worst grad {worst[0]:.3e} "
          f"({worst[1]}) (<= {b_grad:.3e})" + "".join(f", {k} {named[k]:.3e}" for k in also))
    assert torch.isfinite(out.float()).all()
    assert e_out <= b_out and e_loss <= b_loss, (tag, e_out, e_loss)
    assert worst[0] <= b_grad, (tag, worst)
    for k in also:
        assert named[k] <= b_grad, (tag, k, named[k])


DV0_PATH, BYPASS_PATH = "blocks.0.qkv.weight", "blocks.0.mlp.0.weight"


# ---------------------------------------------------------------------------------- against the reference ----
@pytest.mark.parametrize("defer", ["deferred", "per_block", "chunk_of_1"])
@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_routed_step_against_the_reference(vds, monkeypatch, name, defer):
    """defer: the deferred d v_0 reduction as shipped (the span's two terms are flushed behind it), the per-block
    read-modify-write, and a reduction after EVERY block -- inside the span too, with the routed view's own flag"""
    M = vds["model"]
    monkeypatch.setattr(M, "_DV0_DEFER", defer != "per_block")
    monkeypatch.setattr(M, "_DV0_CHUNK", 1 if defer == "chunk_of_1" else 9)
    cs = RR.case(name)
    ref = RR.reference_step(name)
    m = routed_model(vds, cs)
    check(vds, name, f"routed ({defer})", *step(vds, m, cs, cs["route"]), ref, also=(DV0_PATH, BYPASS_PATH))


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_a_route_that_holds_the_first_and_the_last_token(vds, name):
    cs = RR.case(name)
    inner = [int(r) for r in cs["route"] if 0 < int(r) < RR.N_TOK - 1][:126]
    route = [0] + inner + [RR.N_TOK - 1]
    assert len(route) == 128 and route[0] == 0 and route[-1] == RR.N_TOK - 1
    ref = RR.reference_step(name, route=route)
    for form in (route, torch.tensor(route), torch.tensor(route, dtype=torch.int32).cuda()):
        check(vds, name, f"route 0..N-1 as {type(form).__name__}", *step(vds, routed_model(vds, cs), cs, form), ref,
              also=(DV0_PATH, BYPASS_PATH))


def _patch_of(tok):
    """latent slices of token `tok`: tokens are ordered (h w t), t fastest, on a (4, 8, 8) grid of 2 x 2 x 2 patches"""
    tt, ww, hh = tok % 4, (tok // 4) % 8, tok // 32
    return (slice(None), slice(None), slice(2 * tt, 2 * tt + 2), slice(2 * hh, 2 * hh + 2), slice(2 * ww, 2 * ww + 2))


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_bypassed_and_kept_tokens_perturbed(vds, name):
    """A forward with the blocks behind the span removed is not available; instead the latent is changed (+3) at the patch
    of one bypassed and of one kept token, and the CHANGE of the device's output is held against the change of the routed
    reference's.  Through the reference: 95 % and more of the change sits in that token's own output patch, every other
    position moves a little (the blocks outside the span attend every row).
      on the patch        rel(device change, reference change) <= B_OUT -- the issue's bound, on the difference itself;
      everywhere else     |device change - reference change| <= B_OUT |reference output|: positions the reference leaves
                          (nearly) alone stay put on the device on the scale the outputs themselves are held to;
      discrimination      the UNROUTED reference changes the patch differently, by at least 2 B_OUT of the change, for the
                          bypassed token (which never ran blocks 1 and 2) and for the kept one: the patch bound tells a
                          routed device from an unrouted one in both halves."""
    cs = RR.case(name)
    kept = set(int(r) for r in cs["route"])
    picks = {"bypassed": [t for t in range(RR.N_TOK) if t not in kept][40], "kept": int(cs["route"][40])}
    m = routed_model(vds, cs)

    def ref_fwd(x, route):
        with torch.no_grad():
            return RR.routed_forward(cs["P"], cs["cfg"], x.float(), cs["ctx"].float(), cs["ts"].float(), START, SPAN, route)

    def dev_fwd(x):
        with torch.no_grad():
            return m(x.cuda(), cs["ctx"].cuda(), cs["ts"].cuda(), rope_start=START, route=cs["route"]).float().cpu()
    a_ref, a_un, a_dev = ref_fwd(cs["zt"], cs["route"]), ref_fwd(cs["zt"], None), dev_fwd(cs["zt"])
    assert rel(a_dev, a_ref) <= B_OUT
    for kind, tok in picks.items():
        sl = _patch_of(tok)
        x = cs["zt"].clone()
        x[sl] = (x[sl].float() + 3.0).to(bf16)
        b_ref, b_un, b_dev = ref_fwd(x, cs["route"]), ref_fwd(x, None), dev_fwd(x)
        assert rel(b_dev, b_ref) <= B_OUT
        d_ref, d_un, d_dev = b_ref - a_ref, b_un - a_un, b_dev - a_dev
        assert d_ref[sl].norm() >= 0.95 * d_ref.norm()
        e_patch, wrong = rel(d_dev[sl], d_ref[sl]), rel(d_un[sl], d_ref[sl])
        rest = torch.ones_like(d_ref, dtype=torch.bool)
        rest[sl] = False
        e_rest = ((d_dev - d_ref)[rest].norm() / a_ref.norm()).item()
        print(f"{name} {kind} token {tok}: on its patch the change |{d_ref[sl].norm():.3f}| is off by {e_patch:.3e} of itself "
              f"(<= {B_OUT:.1e}; the unrouted reference by {wrong:.3f}); elsewhere the reference moves by "
              f"{d_ref[rest].norm() / a_ref.norm():.3e} of the output, the device is off by {e_rest:.3e} of the output "
              f"(<= {B_OUT:.1e})")
        assert wrong >= 2 * B_OUT, f"the reference does not tell a {kind} token's routing from none here"
        assert e_patch <= B_OUT, (kind, e_patch)
        assert e_rest <= B_OUT, (kind, e_rest)


# ------------------------------------------------------------------------------ the switch off is the model ----
def test_the_switch_off_is_the_model_itself_bit_for_bit(vds, deterministic):
    cs = RR.case("hd72")
    m = build(vds, cs["cfg"], cs["P"], frame_causal=False)
    out0, loss0, g0 = step(vds, m, cs, None)
    m.enable_token_routing(*SPAN, KEEP)
    out1, _, _ = step(vds, m, cs, cs["route"])
    assert not torch.equal(bits(out0), bits(out1)), "routing changed nothing"
    runs = [step(vds, m, cs, False)]
    m.enable_token_routing(None)
    runs.append(step(vds, m, cs, None))
    for out2, loss2, g2 in runs:
        assert torch.equal(bits(out0), bits(out2)) and loss0 == loss2 and set(g0) == set(g2)
        for k in g0:
            assert torch.equal(bits(g0[k]), bits(g2[k])), k


def test_switched_off_launches_the_kernel_classes_and_entry_points_of_before(vds, monkeypatch):
    cs = RR.case("hd72")
    ops, lib = vds["ops"], vds["lib"].load()
    hits, lens = [], []
    for name in ENTRIES:
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _n=name: (hits.append(_n), _fn(*a))[1])
    fn = ops.attn_fwd
    monkeypatch.setattr(ops, "attn_fwd", lambda *a, _fn=fn, **k: (lens.append(a[0].shape[2]), _fn(*a, **k))[1])

    def classes(m, route):
        torch.cuda.synchronize()
        ops.prof_enable()
        try:
            step(vds, m, cs, route)
            return {k: v["launches"] for k, v in ops.prof_collect().items()}
        finally:
            ops.prof_enable(0)
    m = build(vds, cs["cfg"], cs["P"], frame_causal=False)
    before = classes(m, None)
    depth = cs["cfg"].depth
    assert not hits and lens == [272] * (2 * depth), (hits, lens)  # self- and cross-attention of every block at L rows
    del lens[:]
    m.enable_token_routing(*SPAN, KEEP)
    routed = classes(m, cs["route"])
    # forward: X, v_0, cos, sin gathered before block 1, one merge behind block 2; backward: dX gathered at block 2, one
    # scatter-add of the routed d v_0 and one merge of dX behind block 1
    assert sorted(hits) == ["vds_rows_gather"] * 5 + ["vds_rows_merge"] * 2 + ["vds_rows_scatter_add_f32"]
    assert lens == [272] * 2 + [144] * 4 + [272] * 2  # the routed blocks are the block code at Ls rows
    assert set(k for k, v in routed.items() if v) == set(k for k, v in before.items() if v)  # no other kernel class
    del hits[:], lens[:]
    assert classes(m, False) == before and not hits and lens == [272] * (2 * depth)
    del lens[:]
    m.enable_token_routing(None)
    assert classes(m, None) == before and not hits and lens == [272] * (2 * depth)


def test_eval_and_no_grad_run_every_token(vds, deterministic):
    cs = RR.case("hd64")
    args = (cs["zt"].cuda(), cs["ctx"].cuda(), cs["ts"].cuda())
    plain = build(vds, cs["cfg"], cs["P"], frame_causal=False)
    with torch.no_grad():
        want = plain(*args, rope_start=START)
    m = routed_model(vds, cs)
    assert m.training
    with torch.no_grad():
        assert torch.equal(bits(m(*args, rope_start=START)), bits(want))  # training mode, no grad
    m.eval()
    assert torch.equal(bits(m(*args, rope_start=START).detach()), bits(want))  # grad enabled, eval mode
    m.train()
    torch.manual_seed(3)
    routed = m(*args, rope_start=START).detach()  # training mode with grad: a drawn route
    assert not torch.equal(bits(routed), bits(want))
    torch.manual_seed(3)
    route = m.draw_route(RR.N_TOK)  # (rope_start is pinned: the route is the first draw)
    assert torch.equal(bits(m(*args, rope_start=START, route=route).detach()), bits(routed))


# --------------------------------------------------------------------------------------------- compositions ----
def test_recompute_is_bit_identical(vds, deterministic):
    cs = RR.case("hd72")
    out0, _, g0 = step(vds, routed_model(vds, cs, "none"), cs, cs["route"])
    assert float(g0[DV0_PATH].abs().max()) > 0 and rel(out0, RR.reference_step("hd72")["out"]) <= B_OUT
    for mode in ("selective", "full"):
        out1, _, g1 = step(vds, routed_model(vds, cs, mode), cs, cs["route"])
        assert torch.equal(bits(out0), bits(out1)), mode
        assert set(g0) == set(g1)
        for k in g0:
            assert torch.equal(bits(g0[k]), bits(g1[k])), (mode, k)


@pytest.mark.parametrize("qk_norm", [True, "all"], ids=["qk_norm", "qk_norm_all"])
def test_qk_norm_against_the_reference(vds, qk_norm):
    from head_norm_ref import cross_normed_oracle
    from qk_norm_ref import qk_normed_oracle
    cs = RR.case("hd72")
    wrap = [qk_normed_oracle()] + ([cross_normed_oracle()] if qk_norm == "all" else [])
    ref = RR.reference_step("hd72", wrap=wrap, key=f"qk_norm={qk_norm!r}")
    assert rel(RR.reference_step("hd72")["out"], ref["out"]) > 2 * B_OUT, "the norm is a no-op here"
    m = routed_model(vds, cs, qk_norm=qk_norm)
    check(vds, "hd72", f"routed + qk_norm={qk_norm!r}", *step(vds, m, cs, cs["route"]), ref, also=(DV0_PATH, BYPASS_PATH))


def test_context_lens_against_the_reference(vds):
    cs = RR.case("hd64")
    lens = [24, 7]
    ref = RR.reference_step("hd64", wrap=[RR.context_lens_oracle(lens)], key="context_lens")
    assert rel(RR.reference_step("hd64")["out"], ref["out"]) > 2 * B_OUT, "the lengths are a no-op here"
    m = routed_model(vds, cs)
    check(vds, "hd64", "routed + context_lens", *step(vds, m, cs, cs["route"], context_lens=lens), ref,
          also=(DV0_PATH, BYPASS_PATH))


def test_lora_against_the_reference_on_the_merged_weights(vds):
    """LoRA r = 16 on qkv / q_cross / context_kv with a nonzero lora_B: the adapted routed model against the fp32 reference
    whose weights are W + s B A, built from leaves so that the adapters' gradients come out of the same backward"""
    cs = RR.case("hd72")
    g = torch.Generator().manual_seed(61)
    m = routed_model(vds, cs)
    m.add_lora(rank=16, generator=g)
    s = m.lora["alpha"] / m.lora["rank"]
    ad = {}
    with torch.no_grad():
        for n, p in m.lora_parameters():
            if n.endswith("lora_B"):
                p.copy_((torch.randn(p.shape, generator=g) * 0.05).to(p.device))
            ad[n] = p.detach().float().cpu().to(bf16).float().requires_grad_(True)  # the bf16 values the kernels read
    m.invalidate_compute_copy()
    Pe = {k: v.clone() for k, v in cs["P"].items()}
    for n in [n[:-len(".lora_A")] for n in ad if n.endswith(".lora_A")]:
        Pe[n + ".weight"] = cs["P"][n + ".weight"] + s * ad[n + ".lora_B"] @ ad[n + ".lora_A"]
    ref = RR.reference_step("hd72", P=Pe)
    for n, p in ad.items():
        ref["grads"][n] = p.grad
    assert rel(RR.reference_step("hd72")["out"], ref["out"]) >= 2 * B_OUT, "the adapters are a no-op in this case"
    out, loss, grads = step(vds, m, cs, cs["route"])
    assert set(grads) == set(ad), "only the adapters train"
    check(vds, "hd72", "routed + LoRA", out, loss, grads, ref, also=("blocks.0.qkv.lora_A", "blocks.2.q_cross.lora_B"))


def test_a_second_backward_accumulates(vds, deterministic):
    cs = RR.case("hd64")
    m = routed_model(vds, cs)
    _, _, g1 = step(vds, m, cs, cs["route"])
    _, _, g2 = step(vds, m, cs, cs["route"], zero=False)
    for k in g1:
        if float(g1[k].abs().max()) > 0:
            assert rel(g2[k], 2 * g1[k]) <= 1e-6, k


def test_deterministic_runs_repeat_and_routes_differ(vds, deterministic):
    cs = RR.case("hd72")
    m = routed_model(vds, cs)
    out0, loss0, g0 = step(vds, m, cs, cs["route"])
    out1, loss1, g1 = step(vds, m, cs, cs["route"])
    assert torch.equal(bits(out0), bits(out1)) and loss0 == loss1
    for k in g0:
        assert torch.equal(bits(g0[k]), bits(g1[k])), k
    other = sorted(set(range(RR.N_TOK)) - set(int(r) for r in cs["route"]))
    out2, loss2, _ = step(vds, m, cs, other)
    assert loss2 != loss0 and rel(out2, out0) > 2 * B_OUT


# --------------------------------------------------------------------------------------- trainer and graph ----
def _tiny_training():
    from oracle import dit_oracle as O
    cfg = O.DiTConfig(in_channels=16, hidden_size=128, depth=3, num_heads=2, cross_attn_input_size=64,
                      residual_v=True, train_bias_and_rms=False)
    P = O.init_params(cfg, seed=41, randomize_zero_init=True, init_std_factor=1.0)
    g = torch.Generator().manual_seed(5)
    batches = [{"latent": torch.randn(2, 16, 8, 8, 8, generator=g).cuda(), "context": torch.randn(2, 16, 64, generator=g).cuda(),
                "prompt": ["", ""]} for _ in range(5)]
    return cfg, P, batches


def test_graph_replay_matches_eager(vds):
    """as test_graph_replay_matches_eager: five steps eager and five through GraphedTrainStep (two eager, a capture, three
    replays) from the same seeds agree in loss and parameters; every replay runs a newly drawn route from the static
    tables; a replay with the route pinned reproduces the eager step that ran that route"""
    cfg, P, batches = _tiny_training()
    N = 4 * 4 * 4
    results, tables = [], []
    for graphed, span in ((False, (1, 2)), (True, (1, 2)), (False, None)):
        m = build(vds, cfg, P, frame_causal=False)
        m.enable_token_routing(*span) if span else None
        groups, _ = m.get_mup_setup(3e-3, 0.1, CONST)
        opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99))
        sched = vds["train"].get_schedule(opt, "cosine", 3, 50)
        torch.manual_seed(77)
        torch.cuda.manual_seed(77)
        losses = []
        if graphed:
            gs = vds["graph"].GraphedTrainStep(m, opt, sched, "cuda", eager_steps=2)
            for b in batches:
                losses.append(gs.step(b).item())
                tables.append((gs.route.idx.clone(), gs.route.inv.clone()))
            assert gs.n_replays == 3 and opt._step == 5
            assert tuple(gs.route.idx.shape) == (16 + N // 2,) and tuple(gs.route.inv.shape) == (16 + N,)
        else:
            for b in batches:
                losses.append(vds["train"].train_step(m, opt, sched, b, "cuda").item())
        torch.cuda.synchronize()
        results.append((losses, {k: v.clone() for k, v in m.full_state_dict().items()}))
    (l0, p0), (l1, p1), (l2, _) = results
    assert len(set(l0)) == 5
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    for k in p0:
        assert rel(p1[k], p0[k]) <= 2e-4, (k, rel(p1[k], p0[k]))
    assert l2[0] != l0[0], "the model without routing gives the same first loss: routing is not in the step"
    assert not torch.equal(tables[3][0], tables[4][0]), "two replays ran the same route"
    for idx, inv in tables:
        assert torch.equal(inv[idx.long()].cpu(), torch.arange(16 + N // 2, dtype=torch.int32))


def test_a_replay_with_a_pinned_route_reproduces_the_eager_step(vds):
    cfg, P, batches = _tiny_training()
    route = sorted(torch.randperm(64, generator=torch.Generator().manual_seed(2))[:32].tolist())
    losses = []
    for graphed in (False, True):
        m = build(vds, cfg, P, frame_causal=False).enable_token_routing(1, 2)
        groups, _ = m.get_mup_setup(3e-3, 0.1, CONST)
        opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99))
        torch.manual_seed(78)
        torch.cuda.manual_seed(78)
        if graphed:
            gs = vds["graph"].GraphedTrainStep(m, opt, None, "cuda", eager_steps=1)
            losses.append([gs.step(b, route=route).item() for b in batches[:3]])
            assert gs.n_replays == 2 and gs.route.idx[16:].cpu().tolist() == [16 + r for r in route]
        else:
            losses.append([vds["train"].train_step(m, opt, None, b, "cuda", route=route).item() for b in batches[:3]])
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(*losses)), losses
    # a pinned route is honoured or refused by DiT.forward's rule, never dropped: without the switch it is refused
    off = build(vds, cfg, P, frame_causal=False)
    groups, _ = off.get_mup_setup(3e-3, 0.1, CONST)
    with pytest.raises(ValueError, match=r"enable_token_routing\(first_block, last_block, keep\) first"):
        vds["graph"].GraphedTrainStep(off, vds["optim"].MuAdamW(groups, betas=(0.95, 0.99)), None, "cuda").step(batches[0], route=route)


def test_train_forward_and_train_step_on_a_routed_model(vds):
    cfg, P, batches = _tiny_training()
    runs = []
    for _ in range(2):
        m = build(vds, cfg, P, frame_causal=False).enable_token_routing(1, 2, 0.75)
        groups, _ = m.get_mup_setup(3e-3, 0.1, CONST)
        opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99))
        torch.manual_seed(9)
        torch.cuda.manual_seed(9)
        loss, _ = vds["train"].forward(m, batches[0], None, None, "cuda", 0, False)
        m.zero_grad()
        loss.backward()
        missing = [k for k, p in m.named_parameters() if p.requires_grad and p.grad is None]
        assert torch.isfinite(loss) and not missing, missing
        assert all(torch.isfinite(p.grad).all() for p in m.parameters())
        l2 = vds["train"].train_step(m, opt, None, batches[1], "cuda")
        runs.append((loss.item(), l2.item()))
    # the same seeds draw the same RoPE offsets and the same routes (another route moves the loss by per cents; the second
    # loss follows an optimizer step on gradients summed with atomics, hence not bit for bit)
    assert runs[0][0] == runs[1][0] and abs(runs[0][1] - runs[1][1]) <= 1e-5 * abs(runs[0][1]), runs
