"""Teacher forcing on the GPU, model level: DiT(frame_causal=True, frame_major=True[, frame_chunk=2]) called with
teacher_latents on the tiny hd72 / hd64 cases of tests/test_frame_causal_gpu.py (hidden 144 / 128, t = 3 token-frames).
  * every noisy chunk of ONE teacher call against the device's own cached chunk call -- the cache committed from clean calls
    at t = 0, the same rope_start base, the same register level -- within the one-call bound of tests/test_frame_cache_gpu.py
    (2.5e-2), for every chunk;
  * output, loss and every parameter gradient against teacher_ref.dit_forward in fp32, with the bounds of
    tests/test_model_gpu.py::test_oracle_parity_random (output max(2.5 e_ref, 1.5e-2), loss 1e-2, gradients cosine 0.999 and
    3e-2; lambda_param by its term sum, as there);
  * recomputation bit for bit; GraphedTrainStep(frame_mode="teacher") within the bounds of test_graph_replay_matches_eager_steps;
  * one composed model (QK-norm "all", context_lens, LoRA r = 16, frame_chunk = 2) against its helper;
  * a model called without teacher_latents calls what it called before."""
import os
import sys
from contextlib import ExitStack

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import teacher_ref as TR  # noqa: E402
from test_frame_causal_gpu import B_LOSS, B_OUT, CONST, START, bits, build, model_case, rel  # noqa: E402
from test_model_gpu import GRAD_COS, GRAD_REL, cosine  # noqa: E402

KC, R = TR.KC, TR.R
pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
TS_CHUNK = {1: [[0.5, 0.25, 0.96875], [0.9375, 0.75, 0.0625]], 2: [[0.5, 0.5, 0.96875], [0.9375, 0.9375, 0.0625]]}
REG = [1.0, 1.0]  # the level the cached rollout pins


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import _lib, model, ops, optim, train
    return dict(model=model, ops=ops, optim=optim, train=train, lib=_lib)


@pytest.fixture
def deterministic(vds, request):
    vds["ops"].set_deterministic(True, 256 << 20)
    request.addfinalizer(lambda: vds["ops"].set_deterministic(False))


def flags(chunk):
    return dict(frame_major=True, frame_chunk=chunk)


def noised(name, chunk):
    """(zt, v, ts): the case's latents noised per frame at TS_CHUNK[chunk] (one level per chunk)"""
    cfg, P, latent, ctx, noise = model_case(name)
    ts = torch.tensor(TS_CHUNK[chunk]).to(bf16)
    zt, v = R.noise_frames(latent, noise, ts, cfg.time_patch_size)
    return zt, v, ts


_refs = {}


def teacher_reference(name, chunk):
    """one fp32 step of the helper model under the teacher mask, once per case; e_ref: its own bf16-vs-fp32 distance"""
    key = (name, chunk)
    if key not in _refs:
        cfg, P, latent, ctx, noise = model_case(name)
        zt, v, ts = noised(name, chunk)
        w = torch.ones(2, 3)
        Pg = {k: p.clone().requires_grad_(True) for k, p in P.items()}
        out = TR.dit_forward(Pg, cfg, latent.float(), zt.float(), ctx.float(), ts.float(), START, chunk)
        loss, _, _ = R.frame_loss(v, out, w, cfg.time_patch_size)
        loss.backward()
        with torch.no_grad():
            Pb = {k: p.to(bf16) for k, p in P.items()}
            e_ref = rel(TR.dit_forward(Pb, cfg, latent, zt, ctx, ts, START, chunk), out)
        _refs[key] = dict(out=out.detach(), loss=loss.item(), zt=zt, v=v, ts=ts, w=w, e_ref=e_ref,
                          grads={k: p.grad for k, p in Pg.items() if p.grad is not None})
    return _refs[key]


def teacher_step(vds, m, name, chunk, **kw):
    cfg, P, latent, ctx, noise = model_case(name)
    zt, v, ts = noised(name, chunk)
    m.zero_grad()
    out = m(zt.cuda(), ctx.cuda(), ts.cuda(), rope_start=START, teacher_latents=latent.cuda(), **kw)
    loss, _ = vds["train"].frame_flow_loss(out, v.cuda(), torch.ones(2, 3, device="cuda"), cfg.time_patch_size)
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().clone(), loss.item(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("chunk", [1, 2])
@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_every_noisy_chunk_is_the_devices_own_cached_chunk_call(vds, name, chunk):
    from test_frame_cache_gpu import BASE, chunk_call
    cfg, P, latent, ctx, noise = model_case(name)
    zt, v, ts = noised(name, chunk)
    m = build(vds, cfg, P, **flags(chunk))
    reg = torch.tensor(KC.REG)  # (the sibling's pinned levels: chunk_call passes them)
    with torch.no_grad():
        out = m(zt.cuda(), ctx.cuda(), ts.cuda(), rope_start=BASE, teacher_latents=latent.cuda(), register_timesteps=reg)
    assert out.dtype == bf16 and tuple(out.shape) == tuple(latent.shape) and torch.isfinite(out.float()).all()
    cache = m.new_frame_cache(2, 3, 4, 4)
    for f0 in range(0, 3, chunk):
        k = min(chunk, 3 - f0)
        want = chunk_call(m, cache, zt, ctx, f0, k, ts[:, f0:f0 + k].contiguous())
        e = rel(out[:, :, 2 * f0:2 * (f0 + k)], want)
        print(f"{name} chunk {chunk} frames {f0}..{f0 + k - 1}: teacher vs the cached call {e:.3e} (bound {B_OUT:.1e})")
        assert e <= B_OUT, (f0, e)
        chunk_call(m, cache, latent, ctx, f0, k, torch.zeros(2, k, dtype=bf16))
        cache.commit()


@pytest.mark.parametrize("chunk", [1, 2])
@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_model_step_against_the_teacher_reference(vds, name, chunk):
    cfg, P, latent, ctx, noise = model_case(name)
    ref = teacher_reference(name, chunk)
    m = build(vds, cfg, P, **flags(chunk))
    out, loss, grads = teacher_step(vds, m, name, chunk)
    e, e_loss = rel(out, ref["out"]), abs(loss - ref["loss"]) / abs(ref["loss"])
    print(f"{name} chunk {chunk}: out {e:.3e} (e_ref {ref['e_ref']:.3e}), loss {e_loss:.2e}")
    assert tuple(out.shape) == tuple(latent.shape) and torch.isfinite(out.float()).all()
    assert e <= max(2.5 * ref["e_ref"], 1.5e-2), (e, ref["e_ref"])
    assert e_loss <= 1e-2, e_loss
    bad, worst = [], (0.0, None)
    for k, g in grads.items():
        if k not in ref["grads"] or k.endswith("lambda_param") or float(ref["grads"][k].abs().max()) == 0:
            continue
        c, eg = cosine(g, ref["grads"][k]), rel(g, ref["grads"][k])
        worst = max(worst, (eg, k))
        if not (c >= GRAD_COS and eg <= GRAD_REL):
            bad.append((k, c, eg))
    print(f"    worst gradient {worst}")
    assert not bad, bad
    assert float(grads["patch_embed.patch_proj.weight"].abs().max()) > 0  # the clean rows' gradients arrive through K / V
    # the default register level is 1.0 per sample
    with torch.no_grad():
        a = m(ref["zt"].cuda(), ctx.cuda(), ref["ts"].cuda(), rope_start=START, teacher_latents=latent.cuda())
        b = m(ref["zt"].cuda(), ctx.cuda(), ref["ts"].cuda(), rope_start=START, teacher_latents=latent.cuda(),
              register_timesteps=torch.ones(2))
    assert torch.equal(bits(a), bits(b))


def test_recompute_is_bit_identical(vds, deterministic):
    cfg, P, latent, ctx, noise = model_case("hd64")
    out0, l0, g0 = teacher_step(vds, build(vds, cfg, P, "none", **flags(2)), "hd64", 2)
    assert float(g0["blocks.0.qkv.weight"].abs().max()) > 0
    for mode in ("selective", "full"):
        out1, l1, g1 = teacher_step(vds, build(vds, cfg, P, mode, **flags(2)), "hd64", 2)
        assert torch.equal(bits(out0), bits(out1)) and l0 == l1, mode
        assert set(g0) == set(g1)
        for k in g0:
            assert torch.equal(bits(g0[k]), bits(g1[k])), (mode, k)


def test_graph_replay_matches_eager(vds):
    """GraphedTrainStep(frame_mode="teacher") on a frame_chunk=2 model; 4 token-frames: two chunks, one level each"""
    from oracle import dit_oracle as O
    from video_diffusion_speedrun_amd.graph import GraphedTrainStep
    cfg = O.DiTConfig(in_channels=16, hidden_size=128, depth=3, num_heads=2, cross_attn_input_size=64,
                      residual_v=True, train_bias_and_rms=False)
    P = O.init_params(cfg, seed=41, randomize_zero_init=True, init_std_factor=1.0)
    g = torch.Generator().manual_seed(5)
    batches = [{"latent": torch.randn(2, 16, 8, 8, 8, generator=g).cuda(), "context": torch.randn(2, 16, 64, generator=g).cuda(),
                "prompt": ["", ""]} for _ in range(5)]
    results = []
    for graphed in (False, True):
        m = build(vds, cfg, P, **flags(2))
        groups, _ = m.get_mup_setup(3e-3, 0.1, CONST)
        opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99))
        sched = vds["train"].get_schedule(opt, "cosine", 3, 50)
        torch.manual_seed(77)
        torch.cuda.manual_seed(77)
        losses = []
        if graphed:
            gs = GraphedTrainStep(m, opt, sched, "cuda", eager_steps=2, frame_mode="teacher")
            for b in batches:
                losses.append(gs.step(b).item())
            assert gs.n_replays == 3 and opt._step == 5
        else:
            for b in batches:
                losses.append(vds["train"].train_step(m, opt, sched, b, "cuda", frame_mode="teacher").item())
        torch.cuda.synchronize()
        results.append((losses, {k: v.clone() for k, v in m.full_state_dict().items()}))
    (l0, p0), (l1, p1) = results
    assert len(set(l0)) == 5
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    for k in p0:
        assert rel(p1[k], p0[k]) <= 2e-4, (k, rel(p1[k], p0[k]))


def test_composed_model_against_its_helper(vds):
    """QK-norm "all" + context_lens + LoRA r = 16 + frame_chunk = 2 under teacher forcing: the adapted model against the fp32
    helper on the merged weights, with the normed oracles"""
    import test_lora_gpu as TL
    from head_norm_ref import cross_normed_oracle
    from qk_norm_ref import qk_normed_oracle
    cs = TL.case("hd72")
    cfg = cs["cfg"]
    g = torch.Generator().manual_seed(99)
    latent = torch.randn(2, 16, 4, 8, 8, generator=g).to(bf16)  # pt = 1: 4 token-frames, two chunks of 2
    noise = torch.randn(2, 16, 4, 8, 8, generator=g).to(bf16)
    ctx = torch.randn(2, 8, 64, generator=g).to(bf16)
    ts = torch.tensor([[0.25, 0.25, 0.9375, 0.9375], [0.5, 0.5, 0.0625, 0.0625]]).to(bf16)
    zt, v = R.noise_frames(latent, noise, ts, 1)
    lens = [5, 8]
    Pe, Ad, eff = TL.merged_params(cs["P"], cs["ad"], leaves=True)
    with ExitStack() as st:
        st.enter_context(qk_normed_oracle())
        st.enter_context(cross_normed_oracle())
        ref = TR.dit_forward(Pe, cfg, latent.float(), zt.float(), ctx.float(), ts.float(), TL.START, 2, context_lens=lens)
        loss_r, _, _ = R.frame_loss(v, ref, torch.ones(2, 4), 1)
        loss_r.backward()
        with torch.no_grad():
            plain = TR.dit_forward(cs["P"], cfg, latent.float(), zt.float(), ctx.float(), ts.float(), TL.START, 2,
                                   context_lens=lens)
    assert rel(plain, ref) >= 2 * B_OUT, "the adapters are a no-op in this case"
    m = TL.build(vds, cs, frame_causal=True, frame_major=True, frame_chunk=2, qk_norm="all")
    m.zero_grad()
    out = m(zt.cuda(), ctx.cuda(), ts.cuda(), rope_start=TL.START, context_lens=lens, teacher_latents=latent.cuda())
    loss, _ = vds["train"].frame_flow_loss(out, v.cuda(), torch.ones(2, 4, device="cuda"), 1)
    loss.backward()
    torch.cuda.synchronize()
    e, e_loss = rel(out, ref), abs(loss.item() - loss_r.item()) / abs(loss_r.item())
    print(f"composed: out {e:.3e} loss {e_loss:.2e}")
    assert torch.isfinite(out.float()).all() and e <= B_OUT and e_loss <= B_LOSS, (e, e_loss)
    worst = max((rel(p.grad, Ad[n].grad), n) for n, p in m.lora_parameters())
    print(f"    worst adapter gradient {worst}")
    assert worst[0] <= GRAD_REL, worst


def test_entry_points_with_and_without_the_keyword(vds, monkeypatch):
    """without teacher_latents a model calls none of the new entry points and passes no teacher keyword -- the calls of
    before; with it every full-sequence self-attention goes through them"""
    cfg, P, latent, ctx, noise = model_case("hd72")
    zt, v, ts = noised("hd72", 2)
    ops, lib = vds["ops"], vds["lib"].load()
    seen, hits, old = [], [], []
    for name in ("vds_teacher_attn_fwd", "vds_teacher_attn_bwd"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _n=name: (hits.append(_n), _fn(*a))[1])
    for name in ("vds_attn_fwd_causal_fm_chunk", "vds_attn_bwd_causal_fm_chunk", "vds_attn_fwd_causal_fm", "vds_attn_bwd_causal_fm"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _n=name: (old.append(_n), _fn(*a))[1])
    for name in ("attn_fwd", "attn_bwd"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _fn=fn, _n=name, **k: (seen.append((_n, k.get("teacher"), k.get("frames"))), _fn(*a, **k))[1])

    def plain_step(m):
        m.zero_grad()
        out = m(zt.cuda(), ctx.cuda(), ts.cuda(), rope_start=START)
        out.float().sum().backward()
        torch.cuda.synchronize()
    for kw, entry in ((dict(frame_major=True), "_fm"), (flags(2), "_fm_chunk")):
        del seen[:], hits[:], old[:]
        plain_step(build(vds, cfg, P, **kw))
        assert seen and all(t is None for _, t, _ in seen) and not hits, (kw, seen, hits)
        assert sorted(old) == [f"vds_attn_bwd_causal{entry}"] * cfg.depth + [f"vds_attn_fwd_causal{entry}"] * cfg.depth
    for chunk in (1, 2):
        del seen[:], hits[:], old[:]
        teacher_step(vds, build(vds, cfg, P, **flags(chunk)), "hd72", chunk)
        assert sorted(hits) == ["vds_teacher_attn_bwd"] * cfg.depth + ["vds_teacher_attn_fwd"] * cfg.depth and not old
        selfs = [s for s in seen if s[2] is not None]
        assert len(selfs) == 2 * cfg.depth and all(t is True and tuple(fr) == (16, 6) for _, t, fr in selfs), selfs
