"""Frame-band models on the GPU: DiT(...).enable_frame_band(band, chunk) on the tiny hd72 / hd64 configurations of
tests/test_frame_causal_gpu.py with t = 4 token-frames, (chunk, band) = (1, 1) and (2, 0), against the helper model under the
band mask (tests/helpers/frame_band_ref.py) at the bounds of tests/test_frame_window_gpu.py (output 2.5e-2, loss 1e-2, worst
gradient 3e-2); frames outside a frame's reach leave its output bit-identical; the compositions -- residual_v (every
configuration here), QK-norm True and "all", context_lens, [B] and per-frame timesteps, LoRA, recomputation bit for bit,
GraphedTrainStep, train.forward's frame modes, generate_latents without kv_cache; the model before enable_frame_band and
after enable_frame_band(None) is itself, bit for bit, and launches the kernel classes and entry points it launched."""
import os
import sys
from contextlib import ExitStack

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_band_ref as FB  # noqa: E402
from test_frame_causal_gpu import B_GRAD, B_LOSS, B_OUT, CONST, START, bits, build, rel, step, within_bounds  # noqa: E402
from test_frame_window_gpu import TS4, args_of, case4  # noqa: E402

R = FB.R
pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
CB = [(1, 1), (2, 0)]
cb_ids = [f"c{c}_b{b}" for c, b in CB]


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import _lib, graph, model, ops, optim, sampling, train
    return dict(model=model, ops=ops, optim=optim, train=train, sampling=sampling, lib=_lib, graph=graph)


@pytest.fixture
def deterministic(vds, request):
    vds["ops"].set_deterministic(True, 256 << 20)
    request.addfinalizer(lambda: vds["ops"].set_deterministic(False))


def band_model(vds, cfg, P, c, band, mode="none", **kw):
    """the bidirectional model (no frame_causal) with the switch"""
    return build(vds, cfg, P, mode, frame_causal=False, **kw).enable_frame_band(band, chunk=c)


_refs = {}


def reference_step(name, c, band):
    """one fp32 step of the helper model, once per case; band = None: every pair (a band of all t - 1 frames)"""
    key = (name, c, band)
    if key not in _refs:
        cs = case4(name)
        Pg = {k: p.clone().requires_grad_(True) for k, p in cs["P"].items()}
        out = FB.dit_forward(Pg, cs["cfg"], cs["zt"].float(), cs["ctx"].float(), cs["ts"].float(), START,
                             1 if band is None else c, 3 if band is None else band)
        loss, _, _ = R.frame_loss(cs["v"], out, cs["w"], cs["cfg"].time_patch_size)
        loss.backward()
        _refs[key] = dict(out=out.detach(), loss=loss.item(), grads={k: p.grad for k, p in Pg.items() if p.grad is not None})
    return _refs[key]


@pytest.mark.parametrize("c,band", CB, ids=cb_ids)
@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_model_step_against_the_band_masked_reference(vds, name, c, band):
    cs = case4(name)
    ref, full = reference_step(name, c, band), reference_step(name, c, None)
    d_out = rel(full["out"], ref["out"])  # discrimination, on the CPU references alone
    print(f"{name} c={c} band={band}: band-masked vs unmasked reference: out {d_out:.3f}")
    assert d_out >= 2 * B_OUT, d_out
    m = band_model(vds, cs["cfg"], cs["P"], c, band)
    assert m.frame_band == (c, band // c) and all(b.frame_band == (c, band // c) for b in m.blocks)
    out, loss, grads = step(vds, m, *args_of(cs))
    within_bounds(f"{name} chunk={c} band={band}", out, loss, grads, ref)
    t1 = cs["ts"][:, 1].contiguous()  # [B] timesteps: frames = (N_REG, t) comes from the latent shape
    with torch.no_grad():
        o1 = m(cs["zt"].cuda(), cs["ctx"].cuda(), t1.cuda(), rope_start=START)
        r1 = FB.dit_forward(cs["P"], cs["cfg"], cs["zt"].float(), cs["ctx"].float(), t1.float(), START, c, band)
    assert rel(o1, r1) <= B_OUT, rel(o1, r1)


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_a_band_of_every_frame_is_the_unmasked_model(vds, name):
    """only the summation order and the row layout differ: within the model bounds of the plain model's own step, and the
    helper under a band of every pair IS the unmasked helper"""
    cs = case4(name)
    ref = reference_step(name, 1, None)
    out0, loss0, g0 = step(vds, build(vds, cs["cfg"], cs["P"], frame_causal=False), *args_of(cs))
    for c, band in ((1, 3), (2, 2), (1, 40)):
        out1, loss1, g1 = step(vds, band_model(vds, cs["cfg"], cs["P"], c, band), *args_of(cs))
        within_bounds(f"{name} band of every frame (c={c}, band={band})", out1, loss1, g1, ref)
        assert rel(out1, out0) <= B_OUT and abs(loss1 - loss0) <= B_LOSS * abs(loss0) and set(g0) == set(g1)
    within_bounds(f"{name} no band", out0, loss0, g0, ref)


def test_the_switch_off_is_the_model_itself_bit_for_bit(vds, deterministic):
    cs = case4("hd72")
    m = build(vds, cs["cfg"], cs["P"], frame_causal=False)
    out0, loss0, g0 = step(vds, m, *args_of(cs))
    m.enable_frame_band(1)
    out1, _, _ = step(vds, m, *args_of(cs))
    assert not torch.equal(bits(out0), bits(out1)), "the band changed nothing"
    m.enable_frame_band(None)
    out2, loss2, g2 = step(vds, m, *args_of(cs))
    assert torch.equal(bits(out0), bits(out2)) and loss0 == loss2 and set(g0) == set(g2)
    for k in g0:
        assert torch.equal(bits(g0[k]), bits(g2[k])), k


def test_switched_off_launches_the_kernel_classes_and_entry_points_of_before(vds, monkeypatch):
    cs = case4("hd72")
    ops, lib = vds["ops"], vds["lib"].load()
    hits, seen = [], []
    for name in ("vds_band_attn_fwd", "vds_band_attn_bwd"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _n=name: (hits.append(_n), _fn(*a))[1])
    for name in ("attn_fwd", "attn_bwd"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _fn=fn, _n=name, **k: (seen.append((_n, k.get("frames"))), _fn(*a, **k))[1])

    def classes(m):
        torch.cuda.synchronize()
        ops.prof_enable()
        try:
            step(vds, m, *args_of(cs))
            return {k: v["launches"] for k, v in ops.prof_collect().items()}
        finally:
            ops.prof_enable(0)
    m = build(vds, cs["cfg"], cs["P"], frame_causal=False)
    before = classes(m)
    assert not hits and seen and all(fr is None for _, fr in seen), (hits, seen)
    del seen[:]
    m.enable_frame_band(1)
    with_band = classes(m)
    depth = cs["cfg"].depth
    assert sorted(hits) == ["vds_band_attn_bwd"] * depth + ["vds_band_attn_fwd"] * depth
    assert len(seen) == 2 * depth and all(fr is None for _, fr in seen)  # the cross-attention's calls only
    assert with_band != before  # the plain attention classes took the self-attention's launches
    del hits[:], seen[:]
    m.enable_frame_band(None)
    after = classes(m)
    assert after == before and not hits and len(seen) == 4 * depth


@pytest.mark.parametrize("name,c,band,frames_far", [("hd72", 1, 1, (0, 1)), ("hd64", 2, 0, (0, 1))],
                         ids=["hd72_c1_b1", "hd64_c2_b0"])
def test_frames_outside_a_frames_band_leave_it_bit_identical_in_one_block(vds, name, c, band, frames_far):
    """a ONE-block model (block 0 of the case): the registers attend every token and every token attends them, so from the
    second block on every frame reaches every other through the register rows -- that is the design -- but inside one block
    a token reads the registers' K / V, which come from the register tokens and the noise levels alone.  The last frame then
    depends on the frames of its band only (hd72, chunk 1, band 1: frames 2, 3; hd64, chunk 2, band 0: its own chunk, frames
    2, 3): other latents in frames 0 and 1 move it by exactly 0.0, frame 2 moves it far beyond the model bound -- and, the
    mask being two-sided, other latents in the LAST frame leave frame 0 bit-identical too."""
    from oracle import dit_oracle as O
    cs = case4(name)
    cfg = cs["cfg"]
    pt = cfg.time_patch_size
    cfg1 = O.DiTConfig(in_channels=cfg.in_channels, patch_size=cfg.patch_size, time_patch_size=pt,
                       hidden_size=cfg.hidden_size, depth=1, num_heads=cfg.num_heads,
                       cross_attn_input_size=cfg.cross_attn_input_size, residual_v=cfg.residual_v,
                       train_bias_and_rms=cfg.train_bias_and_rms)
    P1 = {k: v for k, v in cs["P"].items() if not k.startswith("blocks.") or k.startswith("blocks.0.")}
    m = band_model(vds, cfg1, P1, c, band)
    ts = torch.tensor(TS4).to(bf16)

    def edited(frames):
        x = cs["latent"].clone()
        for f in frames:
            x[:, :, f * pt:(f + 1) * pt] = (cs["latent"][:, :, f * pt:(f + 1) * pt].float() + 3.0).to(bf16)
        return x
    first, last = slice(0, pt), slice(3 * pt, 4 * pt)
    with torch.no_grad():
        run = lambda x: m(x.cuda(), cs["ctx"].cuda(), ts.cuda(), rope_start=START)
        a, far, near, back = run(cs["latent"]), run(edited(frames_far)), run(edited((2,))), run(edited((3,)))
    assert rel(far[:, :, first], a[:, :, first]) > 4 * B_OUT  # the edited frame itself moved
    assert torch.equal(bits(far[:, :, last]), bits(a[:, :, last])), "a frame outside the band reached the last frame"
    assert rel(near[:, :, last], a[:, :, last]) > 2 * B_OUT
    assert torch.equal(bits(back[:, :, first]), bits(a[:, :, first])), "the last frame reached frame 0"
    # and the plain model has no such frame: every frame reads every other
    plain = build(vds, cfg1, P1, frame_causal=False)
    with torch.no_grad():
        pa = plain(cs["latent"].cuda(), cs["ctx"].cuda(), ts.cuda(), rope_start=START)
        pf = plain(edited(frames_far).cuda(), cs["ctx"].cuda(), ts.cuda(), rope_start=START)
    assert not torch.equal(bits(pf[:, :, last]), bits(pa[:, :, last]))


def test_recompute_is_bit_identical(vds, deterministic):
    cs = case4("hd64")
    ref = reference_step("hd64", 1, 1)
    out0, _, g0 = step(vds, band_model(vds, cs["cfg"], cs["P"], 1, 1, "none"), *args_of(cs))
    assert float(g0["blocks.0.qkv.weight"].abs().max()) > 0
    assert rel(out0, ref["out"]) <= B_OUT
    for mode in ("selective", "full"):
        out1, _, g1 = step(vds, band_model(vds, cs["cfg"], cs["P"], 1, 1, mode), *args_of(cs))
        assert torch.equal(bits(out0), bits(out1)), mode
        for k in g0:
            assert torch.equal(bits(g0[k]), bits(g1[k])), (mode, k)


@pytest.mark.parametrize("qk_norm", [True, "all"], ids=["qk_norm", "qk_norm_all"])
def test_qk_norm_and_context_lens_against_the_helper(vds, qk_norm):
    from head_norm_ref import cross_normed_oracle
    from qk_norm_ref import qk_normed_oracle
    cs = case4("hd72")
    lens = [9, 24]
    with ExitStack() as st:
        st.enter_context(qk_normed_oracle())
        if qk_norm == "all":
            st.enter_context(cross_normed_oracle())
        Pg = {k: p.clone().requires_grad_(True) for k, p in cs["P"].items()}
        out = FB.dit_forward(Pg, cs["cfg"], cs["zt"].float(), cs["ctx"].float(), cs["ts"].float(), START, 1, 1,
                             context_lens=lens)
        loss, _, _ = R.frame_loss(cs["v"], out, cs["w"], cs["cfg"].time_patch_size)
        loss.backward()
    ref = dict(out=out.detach(), loss=loss.item(), grads={k: p.grad for k, p in Pg.items() if p.grad is not None})
    assert rel(reference_step("hd72", 1, 1)["out"], ref["out"]) > 2 * B_OUT, "the norm and the lengths are a no-op here"
    m = band_model(vds, cs["cfg"], cs["P"], 1, 1, qk_norm=qk_norm)
    out, loss, grads = step(vds, m, *args_of(cs), context_lens=lens)
    within_bounds(f"band + qk_norm={qk_norm!r} + context_lens", out, loss, grads, ref)


def test_lora_composed_against_its_helper(vds):
    """LoRA r = 16 on qkv / q_cross / context_kv + QK-norm "all" + context_lens under the band: the adapted model against
    the fp32 helper on the merged weights (the composition of tests/test_teacher_gpu.py, with the band mask)"""
    import test_lora_gpu as TL
    from head_norm_ref import cross_normed_oracle
    from qk_norm_ref import qk_normed_oracle
    cs = TL.case("hd72")
    cfg = cs["cfg"]
    g = torch.Generator().manual_seed(199)
    latent = torch.randn(2, 16, 4, 8, 8, generator=g).to(bf16)  # pt = 1: 4 token-frames
    noise = torch.randn(2, 16, 4, 8, 8, generator=g).to(bf16)
    ctx = torch.randn(2, 8, 64, generator=g).to(bf16)
    ts = torch.tensor([[0.25, 0.5, 0.9375, 0.125], [0.5, 0.75, 0.0625, 0.875]]).to(bf16)
    zt, v = R.noise_frames(latent, noise, ts, 1)
    lens = [5, 8]
    Pe, Ad, eff = TL.merged_params(cs["P"], cs["ad"], leaves=True)
    with ExitStack() as st:
        st.enter_context(qk_normed_oracle())
        st.enter_context(cross_normed_oracle())
        ref = FB.dit_forward(Pe, cfg, zt.float(), ctx.float(), ts.float(), TL.START, 1, 1, context_lens=lens)
        loss_r, _, _ = R.frame_loss(v, ref, torch.ones(2, 4), 1)
        loss_r.backward()
        with torch.no_grad():
            plain = FB.dit_forward(cs["P"], cfg, zt.float(), ctx.float(), ts.float(), TL.START, 1, 1, context_lens=lens)
    assert rel(plain, ref) >= 2 * B_OUT, "the adapters are a no-op in this case"
    m = TL.build(vds, cs, qk_norm="all").enable_frame_band(1)
    m.zero_grad()
    out = m(zt.cuda(), ctx.cuda(), ts.cuda(), rope_start=TL.START, context_lens=lens)
    loss, _ = vds["train"].frame_flow_loss(out, v.cuda(), torch.ones(2, 4, device="cuda"), 1)
    loss.backward()
    torch.cuda.synchronize()
    e, e_loss = rel(out, ref), abs(loss.item() - loss_r.item()) / abs(loss_r.item())
    print(f"composed: out {e:.3e} loss {e_loss:.2e}")
    assert torch.isfinite(out.float()).all() and e <= B_OUT and e_loss <= B_LOSS, (e, e_loss)
    worst = max((rel(p.grad, Ad[n].grad), n) for n, p in m.lora_parameters())
    print(f"    worst adapter gradient {worst}")
    assert worst[0] <= B_GRAD, worst


def _tiny_training(vds):
    from oracle import dit_oracle as O
    cfg = O.DiTConfig(in_channels=16, hidden_size=128, depth=3, num_heads=2, cross_attn_input_size=64,
                      residual_v=True, train_bias_and_rms=False)
    P = O.init_params(cfg, seed=41, randomize_zero_init=True, init_std_factor=1.0)
    g = torch.Generator().manual_seed(5)
    batches = [{"latent": torch.randn(2, 16, 8, 8, 8, generator=g).cuda(), "context": torch.randn(2, 16, 64, generator=g).cuda(),
                "prompt": ["", ""]} for _ in range(5)]
    return cfg, P, batches


@pytest.mark.parametrize("frame_mode", [None, "independent", "first_frame"])
def test_graph_replay_matches_eager_in_every_frame_mode(vds, frame_mode):
    """GraphedTrainStep and train.train_step (train.forward) on a band model -- chunk and band travel by value -- with [B]
    timesteps (frame_mode None) and per-frame ones: eager and captured steps agree, and the band is in the numbers"""
    cfg, P, batches = _tiny_training(vds)
    kw = {} if frame_mode is None else {"frame_mode": frame_mode}
    results = []
    for graphed, band in ((False, 1), (True, 1), (False, None)):
        m = build(vds, cfg, P, frame_causal=False).enable_frame_band(band)
        groups, _ = m.get_mup_setup(3e-3, 0.1, CONST)
        opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99))
        sched = vds["train"].get_schedule(opt, "cosine", 3, 50)
        torch.manual_seed(77)
        torch.cuda.manual_seed(77)
        losses = []
        if graphed:
            gs = vds["graph"].GraphedTrainStep(m, opt, sched, "cuda", eager_steps=2, **kw)
            for b in batches:
                losses.append(gs.step(b).item())
            assert gs.n_replays == 3 and opt._step == 5
        else:
            for b in batches:
                losses.append(vds["train"].train_step(m, opt, sched, b, "cuda", **kw).item())
        torch.cuda.synchronize()
        results.append((losses, {k: v.clone() for k, v in m.full_state_dict().items()}))
    (l0, p0), (l1, p1), (l2, _) = results
    assert len(set(l0)) == 5
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    for k in p0:
        assert rel(p1[k], p0[k]) <= 2e-4, (k, rel(p1[k], p0[k]))
    assert l2[0] != l0[0], "the model without the band gives the same first loss: the band is not in the step"


def test_generate_latents_without_a_cache(vds):
    """the sampler on a band model, whole-video and as an uncached rollout; kv_cache=True is refused with the way out"""
    S = vds["sampling"]
    from test_frame_causal_gpu import model_case
    cfg, P, _, _, _ = model_case("hd72")
    g = torch.Generator().manual_seed(8)
    prompt = torch.randn(1, 12, 64, generator=g).to(bf16)
    lat0 = torch.randn(1, 16, 8, 8, 8, generator=g).to(bf16)
    m = band_model(vds, cfg, P, 1, 1)
    plain = build(vds, cfg, P, frame_causal=False)
    kw = dict(latents=lat0.cuda(), inference_steps=3, cfg_scale=4.0, rope_starts=[(1, 2, 3)] * 6)
    a, b = S.generate_latents(m, prompt.cuda(), **kw), S.generate_latents(plain, prompt.cuda(), **kw)
    assert tuple(a.shape) == (1, 16, 8, 8, 8) and torch.isfinite(a).all()
    assert rel(a, b) > 1e-3, "the band is not in the sampler's calls"
    assert torch.equal(a, S.generate_latents(m, prompt.cuda(), **kw)), "not reproducible"
    r = S.generate_latents(m, prompt.cuda(), rollout_frames=2, **dict(kw, rope_starts=[(1, 2, 3)] * 12))
    assert tuple(r.shape) == (1, 16, 8, 8, 8) and torch.isfinite(r).all()
    with pytest.raises(ValueError, match="use kv_cache=False on this model"):
        S.generate_latents(m, prompt.cuda(), rollout_frames=1, kv_cache=True, **dict(kw, rope_starts=[(1, 2, 3)]))
    with pytest.raises(ValueError, match="has no K / V cache"):
        m.new_frame_cache(1, 4, 4, 4)
