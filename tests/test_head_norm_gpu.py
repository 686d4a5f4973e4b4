"""QK-norm in cross-attention on the GPU, model level: DiT(qk_norm="all") against the fp32 oracle whose self-attention AND
cross-attention are wrapped with rms_norm (tests/helpers/qk_norm_ref.py, tests/helpers/head_norm_ref.py), under the bounds of
tests/test_qk_norm_gpu.py::test_model_step_against_the_wrapped_oracle (output 2.5e-2, loss 1e-2, every gradient 3e-2), and
every path that runs a block: recompute, graph replay, context_lens / per-frame timesteps / the chunk-causal frame-major
self-attention in one model, LoRA, the cached rollout, fp8 linears.

Models: hidden 128 (2 heads of 64) and 144 (2 of 72), depth 2, B = 2, Lc = 24 (L = 40 or 64: never Lc, which is how the
oracle wrapper tells the cross-attention from the self-attention)."""
import os
import sys
from contextlib import ExitStack

import pytest
import torch

from oracle import dit_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_chunk_ref as CH  # noqa: E402
import head_norm_ref as HN  # noqa: E402
from qk_norm_ref import qk_normed_oracle  # noqa: E402
import test_frame_causal_gpu as TF  # noqa: E402

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
CONST = ["patch_proj", "context_kv", "positional_embedding"]
B_OUT, B_LOSS, B_GRAD = 2.5e-2, 1e-2, 3e-2
START = (2, 3, 4)
W_SCALE = 1.0  # on q_cross.weight and the k rows of context_kv.weight: the discrimination below holds as initialised


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import _lib, model, ops, optim, sampling, train
    return dict(model=model, ops=ops, optim=optim, train=train, sampling=sampling, lib=_lib)


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


def both_wrappers():
    """the oracle of a qk_norm="all" model"""
    st = ExitStack()
    st.enter_context(qk_normed_oracle())
    st.enter_context(HN.cross_normed_oracle())
    return st


def build(vds, cfg, P, mode="none", **kw):
    m = vds["model"].DiT(in_channels=cfg.in_channels, patch_size=cfg.patch_size, time_patch_size=cfg.time_patch_size,
                         hidden_size=cfg.hidden_size, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
                         cross_attn_input_size=cfg.cross_attn_input_size, residual_v=cfg.residual_v,
                         train_bias_and_rms=cfg.train_bias_and_rms, **kw)
    m.load_state_dict(P, strict=True)
    return m.to("cuda").enable_recompute(mode)


_cases = {}


def model_case(name):
    """cfg, parameters and inputs, once per name: "hd72" = the model and inputs of smoke(); "hd64" = hidden 128"""
    if name not in _cases:
        hidden, seed = {"hd72": (144, 3), "hd64": (128, 13)}[name]
        cfg = O.DiTConfig(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=hidden, depth=2, num_heads=2,
                          cross_attn_input_size=64, residual_v=True, train_bias_and_rms=False)
        P = O.init_params(cfg, seed=seed, randomize_zero_init=True, init_std_factor=1.0)
        for i in range(cfg.depth):
            P[f"blocks.{i}.q_cross.weight"] = P[f"blocks.{i}.q_cross.weight"] * W_SCALE
            P[f"blocks.{i}.context_kv.weight"][:hidden] *= W_SCALE
        g = torch.Generator().manual_seed(seed + 1)
        latent = torch.randn(2, 16, 4, 8, 8, generator=g).to(bf16)
        ctx = torch.randn(2, 24, 64, generator=g).to(bf16)
        z = torch.randn(2, generator=g).to(bf16)
        noise = torch.randn(2, 16, 4, 8, 8, generator=g).to(bf16)
        t = O.time_shift(z)
        zt, v = O.noise_latents(latent, noise, t)
        _cases[name] = (cfg, P, zt, v, ctx, t)
    return _cases[name]


_oracle = {}


def oracle_step(name, cross):
    """one fp32 oracle step with the self-attention normed and, with `cross`, the cross-attention too; once per key"""
    if (name, cross) not in _oracle:
        cfg, P, zt, v, ctx, t = model_case(name)
        Pg = {k: w.clone().requires_grad_(True) for k, w in P.items()}
        cap = {}
        with (both_wrappers() if cross else qk_normed_oracle()):
            out = O.dit_forward(Pg, cfg, zt.float(), ctx.float(), t.float(), START, cap)
            cap["blocks.1.v"].retain_grad()
            loss, _ = O.flow_loss(v, out)
            loss.backward()
        vm, lam1 = cap["blocks.1.v"], P["blocks.1.lambda_param"].item()
        l1 = (vm.grad * (vm.detach() - cap["blocks.0.v"].detach()) / lam1).abs().sum().item()
        _oracle[(name, cross)] = dict(out=out.detach(), loss=loss.item(), l1=l1,
                                      grads={k: p.grad for k, p in Pg.items() if p.grad is not None})
    return _oracle[(name, cross)]


def grads_of(vds, m, zt, v, ctx, t, **kw):
    m.zero_grad()
    out = m(zt.cuda(), ctx.cuda(), t.cuda(), rope_start=START, **kw)
    loss, _ = vds["train"].flow_loss(out, v.cuda())
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().clone(), loss.item(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_model_step_against_the_oracle_under_both_wrappers(vds, name):
    cfg, P, zt, v, ctx, t = model_case(name)
    ref, self_only = oracle_step(name, True), oracle_step(name, False)
    # discrimination, on the CPU: the q_cross / context_kv weight gradients of the cross-normed and the only-self-normed
    # oracle are at least 10 x the 3e-2 bound apart -- a model that treats "all" as True cannot pass the comparison below
    for i in range(cfg.depth):
        for k in (f"blocks.{i}.q_cross.weight", f"blocks.{i}.context_kv.weight"):
            dist = rel(self_only["grads"][k], ref["grads"][k])
            print(f"{name}: {k} cross-normed vs only-self-normed oracle {dist:.3f}")
            assert dist >= 10 * B_GRAD, (k, dist)
    m = build(vds, cfg, P, qk_norm="all")
    assert m.qk_norm is True and m.qk_norm_cross is True
    out, loss, grads = grads_of(vds, m, zt, v, ctx, t)
    e_out, e_loss = rel(out, ref["out"]), abs(loss - ref["loss"]) / abs(ref["loss"])
    worst = max((rel(g, ref["grads"][k]), k) for k, g in grads.items()
                if k in ref["grads"] and not k.endswith("lambda_param"))
    # d loss / d lambda: a sum of signed products that largely cancel, judged against the sum of their magnitudes (smoke())
    e_lam = abs(grads["blocks.1.lambda_param"].item() - ref["grads"]["blocks.1.lambda_param"].item()) / ref["l1"]
    print(f"{name}: out rel err {e_out:.3e}, loss rel {e_loss:.2e}, worst grad rel err {worst[0]:.3e} ({worst[1]}), "
          f"lambda grad err / sum|terms| {e_lam:.2e}")
    assert torch.isfinite(out.float()).all()
    assert e_out <= B_OUT and e_loss <= B_LOSS, (e_out, e_loss)
    assert worst[0] <= B_GRAD, worst
    assert e_lam <= 2e-4, e_lam


def test_false_and_true_models_launch_no_head_norm_kernel(vds, monkeypatch):
    cfg, P, zt, v, ctx, t = model_case("hd72")
    lib = vds["lib"].load()
    hits = []
    for name in ("vds_head_rmsnorm_fwd", "vds_head_rmsnorm_bwd"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _n=name: (hits.append(_n), _fn(*a))[1])
    for kw in (dict(), dict(qk_norm=False), dict(qk_norm=True)):
        for mode in ("none", "full"):
            del hits[:]
            grads_of(vds, build(vds, cfg, P, mode, **kw), zt, v, ctx, t)
            assert not hits, (kw, mode, hits)
    del hits[:]
    grads_of(vds, build(vds, cfg, P, qk_norm="all"), zt, v, ctx, t)
    assert sorted(hits) == ["vds_head_rmsnorm_bwd"] * 2 * cfg.depth + ["vds_head_rmsnorm_fwd"] * 2 * cfg.depth  # q and k
    del hits[:]
    grads_of(vds, build(vds, cfg, P, "full", qk_norm="all"), zt, v, ctx, t)  # the replay norms again
    assert hits.count("vds_head_rmsnorm_fwd") == 4 * cfg.depth and hits.count("vds_head_rmsnorm_bwd") == 2 * cfg.depth


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_recompute_is_bit_identical(vds, deterministic, name):
    cfg, P, zt, v, ctx, t = model_case(name)
    out0, loss0, g0 = grads_of(vds, build(vds, cfg, P, "none", qk_norm="all"), zt, v, ctx, t)
    assert float(g0["blocks.0.q_cross.weight"].abs().max()) > 0
    for mode in ("selective", "full"):
        out1, loss1, g1 = grads_of(vds, build(vds, cfg, P, mode, qk_norm="all"), zt, v, ctx, t)
        assert torch.equal(out0, out1) and loss0 == loss1, mode
        for k in g0:
            assert torch.equal(g0[k], g1[k]), (mode, k)


def test_graph_replay_matches_eager(vds):
    """GraphedTrainStep on a qk_norm="all" model: two eager steps, capture, three replays against five eager steps, within
    the bounds of tests/test_qk_norm_gpu.py::test_graph_replay_matches_eager (losses 1e-4, parameters 2e-4 relative)"""
    from video_diffusion_speedrun_amd.graph import GraphedTrainStep
    cfg = model_case("hd64")[0]
    P = O.init_params(cfg, seed=41, randomize_zero_init=True, init_std_factor=1.0)
    g = torch.Generator().manual_seed(5)
    batches = [{"latent": torch.randn(2, 16, 4, 8, 8, generator=g).cuda(), "context": torch.randn(2, 24, 64, generator=g).cuda(),
                "prompt": ["", ""]} for _ in range(5)]
    results = []
    for graphed in (False, True):
        m = build(vds, cfg, P, qk_norm="all")
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
        results.append((losses, {k: w.clone() for k, w in m.full_state_dict().items()}))
    (l0, p0), (l1, p1) = results
    assert len(set(l0)) == 5
    print("graph qk_norm=all: worst loss rel", max(abs(a - b) / abs(a) for a, b in zip(l0, l1)),
          "worst param rel", max(rel(p1[k], p0[k]) for k in p0))
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    for k in p0:
        assert rel(p1[k], p0[k]) <= 2e-4, (k, rel(p1[k], p0[k]))


LENS = [0, 17]
CHUNK = 2


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_composes_with_context_lens_frame_timesteps_and_the_chunk_mask(vds, name):
    """one model: context_lens = [0, 17] (sample 0 attends no context row at all), per-frame timesteps, frame_causal +
    frame_major + frame_chunk = 2 -- against the chunk-masked helper model (tests/helpers/frame_chunk_ref.py) under both
    wrappers, within the model-level bounds, on the inputs of tests/test_frame_causal_gpu.py"""
    cfg, P, latent, ctx, noise = TF.model_case(name)
    if cfg.depth != 2:
        cfg = O.DiTConfig(**{**cfg.__dict__, "depth": 2})
        P = {k: w for k, w in P.items() if not k.startswith("blocks.2.")}
    ts = torch.tensor(TF.TS).to(bf16)
    w = (ts > 0).float()
    zt, v = TF.R.noise_frames(latent, noise, ts, cfg.time_patch_size)
    refs = {}
    for cross in (True, False):
        Pg = {k: p.clone().requires_grad_(True) for k, p in P.items()}
        with (both_wrappers() if cross else qk_normed_oracle()):
            out = CH.dit_forward(Pg, cfg, zt.float(), ctx.float(), ts.float(), TF.START, CHUNK, context_lens=LENS)
            loss, _, _ = TF.R.frame_loss(v, out, w, cfg.time_patch_size)
            loss.backward()
        refs[cross] = dict(out=out.detach(), loss=loss.item(), grads={k: p.grad for k, p in Pg.items() if p.grad is not None})
    ref = refs[True]
    d = min(rel(refs[False]["grads"][k], ref["grads"][k]) for k in ref["grads"] if k.endswith("q_cross.weight"))
    print(f"{name}: q_cross.weight gradients, cross-normed vs only-self-normed helper: closest {d:.3f}")
    assert d >= 4 * B_GRAD, d  # (CPU references alone) far enough that a model within 3e-2 of one is outside 3e-2 of the other
    m = build(vds, cfg, P, qk_norm="all", frame_causal=True, frame_major=True, frame_chunk=CHUNK)
    out, loss, grads = TF.step(vds, m, zt, v, ctx, ts, w, cfg.time_patch_size, context_lens=LENS)
    assert all(torch.isfinite(g).all() for g in grads.values())
    TF.within_bounds(f"{name} all + lens + frames + chunk", out, loss, grads, ref)


@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_lora_adapted_model_against_the_same_model_merged(vds, name):
    import test_lora_gpu as TL
    cs = TL.case(name)
    assert {"q_cross", "context_kv"} <= set(TL.TARGETS)
    out_a, loss_a, grads_a = TL.step(vds, TL.build(vds, cs, qk_norm="all"), cs)
    merged = TL.build(vds, cs, qk_norm="all").merge_lora()
    assert merged.lora is None and merged.qk_norm_cross is True
    out_m, loss_m, _ = TL.step(vds, merged, cs)
    plain, _, _ = TL.step(vds, TL.build(vds, cs, lora=False, qk_norm="all"), cs)
    e_out, e_loss = rel(out_a, out_m), abs(loss_a - loss_m) / abs(loss_m)
    print(f"{name}: adapted vs merged: out {e_out:.3e}, loss {e_loss:.2e}; the model without adapters is {rel(plain, out_m):.3f} away")
    assert e_out <= B_OUT and e_loss <= B_LOSS, (e_out, e_loss)
    assert rel(plain, out_m) >= 2 * B_OUT
    for i in range(cs["cfg"].depth):  # the adapters behind the norm get their gradient through its backward
        for tg in ("q_cross", "context_kv"):
            for leaf in ("lora_A", "lora_B"):
                g = grads_a[f"blocks.{i}.{tg}.{leaf}"]
                assert torch.isfinite(g).all() and float(g.abs().max()) > 0, (i, tg, leaf)


@pytest.mark.parametrize("f0,k", [(0, 2), (2, 1)], ids=["first_chunk", "short_last_chunk"])
@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_a_cached_chunk_call_agrees_with_the_models_own_full_sequence_call(vds, name, f0, k):
    from test_frame_cache_gpu import BASE, REG, chunk_call
    from test_frame_cache_gpu import build as cache_build
    KC = CH.KC
    m = cache_build(vds, name, frame_major=True, frame_chunk=CHUNK, qk_norm="all")
    assert m.qk_norm_cross
    _, _, latent, ctx = KC.model_case(name)
    cache = m.new_frame_cache(2, 3, 4, 4)
    for g0 in range(0, f0, CHUNK):
        chunk_call(m, cache, latent, ctx, g0, CHUNK, torch.zeros(2, CHUNK, dtype=bf16))
        cache.commit()
    levels = torch.tensor(KC.T_CHUNK)[:, :k]
    out = chunk_call(m, cache, latent, ctx, f0, k, levels.to(bf16))
    torch.cuda.synchronize()
    ts = torch.ones(2, 3)
    ts[:, :f0] = 0
    ts[:, f0:f0 + k] = levels
    with torch.no_grad():
        full = m(latent.cuda(), ctx.cuda(), ts.to(bf16).cuda(), rope_start=BASE, register_timesteps=torch.tensor(REG))
        other = cache_build(vds, name, frame_major=True, frame_chunk=CHUNK, qk_norm=True)(
            latent.cuda(), ctx.cuda(), ts.to(bf16).cuda(), rope_start=BASE, register_timesteps=torch.tensor(REG))
    e = rel(out, full[:, :, 2 * f0:2 * (f0 + k)])
    print(f"{name} frames {f0}..{f0 + k - 1}: cached vs full-sequence {e:.3e} (bound {B_OUT:.1e})")
    assert torch.isfinite(out.float()).all() and e <= B_OUT, e
    assert not torch.equal(full, other)  # (the cross-attention norm is in the cached call's model)


def test_sampler_runs_the_normed_model(vds):
    S = vds["sampling"]
    cfg, P, zt, v, ctx, t = model_case("hd72")
    g = torch.Generator().manual_seed(8)
    prompt = torch.randn(1, 12, 64, generator=g).to(bf16)
    lat0 = torch.randn(1, 16, 4, 8, 8, generator=g).to(bf16)
    kw = dict(latents=lat0.cuda(), inference_steps=2, cfg_scale=4.0, rope_starts=[START] * 4)
    a = S.generate_latents(build(vds, cfg, P, qk_norm="all"), prompt.cuda(), **kw)
    b = S.generate_latents(build(vds, cfg, P, qk_norm=True), prompt.cuda(), **kw)
    assert torch.isfinite(a).all() and tuple(a.shape) == tuple(lat0.shape) and not torch.equal(a, b)


def test_fp8_linears_with_bf16_normed_attention(vds):
    """enable_fp8(attention=False) on a qk_norm="all" model against the oracle under both wrappers, within the bounds of
    tests/test_qk_norm_gpu.py::test_fp8_linears_with_bf16_normed_attention (output 2.5e-2, loss 1e-2, every gradient cosine
    >= 0.99 and relative error <= 0.15), on two passes (the second with delayed scaling); enable_fp8() itself is refused"""
    cfg, P, zt, v, ctx, t = model_case("hd72")
    ref = oracle_step("hd72", True)
    with pytest.raises(NotImplementedError, match=r"enable_fp8\(attention=False\)"):
        build(vds, cfg, P, qk_norm="all").enable_fp8()
    m = build(vds, cfg, P, qk_norm="all").enable_fp8(attention=False)
    for step in range(2):
        out, loss, grads = grads_of(vds, m, zt, v, ctx, t)
        assert rel(out, ref["out"]) <= 2.5e-2, (step, rel(out, ref["out"]))
        assert abs(loss - ref["loss"]) / ref["loss"] <= 1e-2
        bad = []
        for k, g in grads.items():
            r = ref["grads"].get(k)
            if r is None or k.endswith("lambda_param") or float(r.abs().max()) == 0:
                continue
            c, e = cosine(g, r), rel(g, r)
            if not (c >= 0.99 and e <= 0.15):
                bad.append((k, c, e))
        assert not bad, (step, bad)
    assert m._fp8_hist.ready
