"""Activation recomputation on the GPU (DiT.enable_recompute): parity with the reference fixtures, bit-equality with
mode "none" in deterministic mode (gradients, optimizer steps, micro-batch accumulation, the sharding runtime), graph
capture, the single-output GEMM epilogues of a forward that keeps nothing, and the memory the modes hold.

The parity bounds are those tests/test_model_gpu.py states for the same fixtures (test_g1_golden_forward_backward,
test_g2_dit_s_config1, GRAD_COS / GRAD_REL / LAMBDA_ERR there), restated here."""
import os

import pytest
import torch

from oracle import dit_oracle as O

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
GRAD_COS, GRAD_REL = 0.999, 3e-2   # tests/test_model_gpu.py
LAMBDA_ERR = 5e-4                  # tests/test_model_gpu.py
MODES = ("full", "selective")
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


def build(vds, cfg, P, mode="none"):
    m = vds["model"].DiT(in_channels=cfg.in_channels, patch_size=cfg.patch_size, time_patch_size=cfg.time_patch_size,
                         hidden_size=cfg.hidden_size, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
                         cross_attn_input_size=cfg.cross_attn_input_size, residual_v=cfg.residual_v,
                         train_bias_and_rms=cfg.train_bias_and_rms)
    m.load_state_dict(P, strict=True)
    return m.to("cuda").enable_recompute(mode)


def lambda_term_sums(cfg, P, x, ctx, t, start, upstream):
    """sum_j |dv_j (v_raw_j - v_0_j)| per mixed block from the fp32 oracle: the scale a lambda gradient's error is judged
    against (as in tests/test_model_gpu.py)"""
    Pg = {k: w.clone().requires_grad_(True) for k, w in P.items()}
    cap = {}
    out = O.dit_forward(Pg, cfg, x.float(), ctx.float(), t.float(), start, cap)
    mixed = {i: cap[f"blocks.{i}.v"] for i in range(1, cfg.depth)}
    for vm in mixed.values():
        vm.retain_grad()
    upstream(out).backward()
    v0 = cap["blocks.0.v"].detach()
    return {f"blocks.{i}.lambda_param": (vm.grad * (vm.detach() - v0) / P[f"blocks.{i}.lambda_param"].item()).abs().sum().item()
            for i, vm in mixed.items()}


def check_all_grads(named, ref_grads, l1):
    """every gradient the fixture carries: tensors by cosine / relative error, lambdas against their term sums"""
    bad, n_lambda = [], 0
    for k, ref in ref_grads.items():
        got = named[k].grad
        assert got is not None and got.dtype == f32, k
        if k.endswith("lambda_param"):
            if k not in l1:  # block 0's lambda: unused by the model, zero in the reference too
                assert float(got.abs().max()) == 0.0, k
                continue
            r = ref["sample"] if isinstance(ref, dict) else ref
            err = abs(got.float().cpu().reshape(()).item() - r.float().reshape(()).item()) / l1[k]
            print(f"  {k}: lambda err / sum|terms| {err:.3e}")
            n_lambda += 1
            if err > LAMBDA_ERR:
                bad.append((k, err))
            continue
        if isinstance(ref, dict):
            g, r = got.float().cpu().flatten()[:: ref["step"]], ref["sample"]
        else:
            g, r = got, ref
        c, e = cosine(g, r), rel(g, r)
        if not (c >= GRAD_COS and e <= GRAD_REL):
            bad.append((k, c, e))
    assert n_lambda > 0
    assert not bad, f"gradient mismatches: {bad}"


# ---------------------------------------------------------------------------- 3. reference fixtures ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["g1_tiny_hd64.pt", "g1_tiny_hd72.pt"])
def test_g1_golden_forward_backward(vds, golden_dir, name, mode):
    fx = torch.load(os.path.join(golden_dir, name), weights_only=False)
    cfg = O.DiTConfig(**fx["cfg"])
    P = O.init_params(cfg, **fx["param_init"])
    P.update({k: v.clone() for k, v in fx["param_tweaks"].items()})
    m = build(vds, cfg, P, mode)
    x, ctx, t = fx["x"].cuda().to(bf16), fx["context"].cuda().to(bf16), fx["t"].cuda().to(bf16)
    out = m(x, ctx, t, rope_start=tuple(fx["rope_start"]))
    ref32, ref16 = fx["fp32"]["out"], fx["bf16"]["out"]
    e_ref, e = rel(ref16, ref32), rel(out, ref32)
    print(f"{name} {mode}: out rel err {e:.3e} (reference bf16 vs fp32 {e_ref:.3e})")
    assert e <= max(2.5 * e_ref, 1.5e-2), (e, e_ref)
    (out.float() * fx["dout"].cuda()).sum().backward()
    l1 = lambda_term_sums(cfg, P, fx["x"].to(bf16), fx["context"].to(bf16), fx["t"].to(bf16), tuple(fx["rope_start"]),
                          lambda o: (o * fx["dout"]).sum())
    check_all_grads(dict(m.named_parameters()), fx["fp32"]["grads"], l1)


@pytest.mark.parametrize("mode", MODES)
def test_g2_dit_s_config1(vds, golden_dir, mode):
    fx = torch.load(os.path.join(golden_dir, "g2_dit_s_c1.pt"), weights_only=False)
    cfg = O.DiTConfig(**fx["cfg"])
    P = O.init_params(cfg, seed=fx["param_seed"], randomize_zero_init=True, init_std_factor=0.1)
    g = torch.Generator().manual_seed(fx["input_seed"])
    x = torch.randn(4, 16, 8, 16, 16, generator=g)
    ctx = torch.randn(4, 512, 4096, generator=g)
    t = O.time_shift(torch.randn(4, generator=g))
    v = torch.randn(4, 16, 8, 16, 16, generator=g)
    m = build(vds, cfg, P, mode)
    out = m(x.cuda().to(bf16), ctx.cuda().to(bf16), t.cuda().to(bf16), rope_start=tuple(fx["rope_start"]))
    e = rel(out, fx["out"])
    loss, _ = vds["train"].flow_loss(out, v.cuda().to(bf16))
    print(f"g2 {mode}: out rel err {e:.3e}, loss {loss.item():.6f} vs {fx['loss']:.6f}")
    assert e <= 2.5e-2
    assert abs(loss.item() - fx["loss"]) / fx["loss"] <= 1e-2
    loss.backward()
    l1 = lambda_term_sums(cfg, P, x.to(bf16), ctx.to(bf16), t.to(bf16), tuple(fx["rope_start"]),
                          lambda o: O.flow_loss(v.to(bf16), o)[0])
    check_all_grads(dict(m.named_parameters()), fx["grad_digest"], l1)


# ------------------------------------------------------------------- 4. bit-equality with mode "none" ----
def _det_case(shape):
    if shape == "hd72_biases_and_norm_weights":
        cfg = O.DiTConfig(in_channels=16, hidden_size=144, depth=6, num_heads=2, cross_attn_input_size=64,
                          residual_v=True, train_bias_and_rms=True)
    else:
        cfg = O.DiTConfig(in_channels=16, hidden_size=128, depth=6, num_heads=2, cross_attn_input_size=64,
                          residual_v=True, train_bias_and_rms=False)
    P = O.init_params(cfg, seed=11, randomize_zero_init=True, init_std_factor=1.0)
    for i in range(1, cfg.depth):  # distinct mixing weights, so that a replay with the wrong v_0 / lambda would show
        P[f"blocks.{i}.lambda_param"] = torch.tensor([0.3 + 0.1 * i])
    return cfg, P, (16, 8, 16, 16), 24, 3


@pytest.mark.parametrize("shape", ["hd72_biases_and_norm_weights", "hd64_plain"])
def test_gradients_are_bit_equal_to_mode_none(vds, deterministic, shape):
    cfg, P, lat, Lc, B = _det_case(shape)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, *lat, generator=g).to(bf16).cuda()
    c = torch.randn(B, Lc, cfg.cross_attn_input_size, generator=g).to(bf16).cuda()
    t = torch.rand(B, generator=g).to(bf16).cuda()
    v = torch.randn(B, *lat, generator=g).to(bf16).cuda()

    def run(mode):
        m = build(vds, cfg, P, mode)
        out = m(x, c, t, rope_start=(3, 4, 5))
        loss, _ = vds["train"].flow_loss(out, v)
        loss.backward()
        torch.cuda.synchronize()
        return loss.item(), out.clone(), {k: p.grad.clone() for k, p in m.named_parameters()}

    l0, o0, g0 = run("none")
    assert all(float(g0[f"blocks.{i}.lambda_param"].abs().max()) > 0 for i in range(1, cfg.depth))
    for mode in MODES:
        l1, o1, g1 = run(mode)
        assert l1 == l0, (mode, l0, l1)
        assert torch.equal(o1, o0), mode
        diff = [k for k in g0 if not torch.equal(g1[k], g0[k])]
        assert not diff, (mode, diff)


# ------------------------------------------------------------ 5. optimizer steps and accumulation ----
def _batches(n, B=2):
    g = torch.Generator().manual_seed(3)
    return [{"latent": torch.randn(B, 16, 4, 8, 8, generator=g), "context": torch.randn(B, 16, 64, generator=g),
             "prompt": [""] * B} for _ in range(n)]


def _small_cfg():
    cfg = O.DiTConfig(in_channels=16, hidden_size=144, depth=4, num_heads=2, cross_attn_input_size=64,
                      residual_v=True, train_bias_and_rms=True)
    return cfg, O.init_params(cfg, seed=31, randomize_zero_init=True, init_std_factor=1.0)


@pytest.mark.parametrize("accumulate", [False, True], ids=["one_backward", "two_backwards_per_step"])
def test_three_optimizer_steps_are_bit_equal(vds, deterministic, accumulate):
    cfg, P = _small_cfg()
    batches = _batches(6)
    train = vds["train"]

    def run(mode):
        m = build(vds, cfg, P, mode)
        groups, _ = m.get_mup_setup(3e-3, 0.1, CONST)
        opt = vds["optim"].MuAdamW(groups, betas=(0.95, 0.99))
        losses = []
        for s in range(3):
            gen = torch.Generator(device="cuda").manual_seed(100 + s)
            torch.manual_seed(0)
            if not accumulate:
                losses.append(train.train_step(m, opt, None, batches[s], "cuda", generator=gen, rope_start=(1, 2, 3)).item())
                continue
            opt.zero_grad()
            for b in (batches[2 * s], batches[2 * s + 1]):  # micro-batches: the second backward adds to .grad
                loss, _ = train.forward(m, b, None, None, "cuda", 0, False, generator=gen, rope_start=(1, 2, 3))
                loss.backward()
                losses.append(loss.item())
            opt.step()
        torch.cuda.synchronize()
        return losses, {k: v.clone() for k, v in m.full_state_dict().items()}

    l0, p0 = run("none")
    assert any(not torch.equal(p0[k].float().cpu(), P[k].float()) for k in p0)  # the steps moved the parameters
    for mode in MODES:
        l1, p1 = run(mode)
        assert l1 == l0, (mode, l0, l1)
        diff = [k for k in p0 if not torch.equal(p1[k], p0[k])]
        assert not diff, (mode, diff)


# ------------------------------------------------------------------------ 6. the sharding runtime ----
def test_shard_runtime_on_one_gpu_is_bit_equal(vds, deterministic, monkeypatch):
    """apply_fsdp forced on with a 1-rank communicator (as test_shard_runtime_on_one_gpu_matches_unsharded does), resident
    and reshard_after_forward: the replay sits between pre_backward_block and post_backward_block, where the block's
    weights are gathered.  Five blocks on the ring's three buffers, every mixing block with a lambda of its own: a buffer
    is refilled while the deferred dv0 reduction is pending, and a lambda read from it would show in block 0's gradients."""
    import torch.distributed as dist
    from video_diffusion_speedrun_amd.fsdp import apply_fsdp
    from video_diffusion_speedrun_amd import comm
    monkeypatch.setenv("VDS_ADALN_BATCH", "0")  # the unsharded run on the per-block adaLN form the sharded one uses
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29541")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        cfg = O.DiTConfig(in_channels=16, hidden_size=128, depth=5, num_heads=2, cross_attn_input_size=64,
                          residual_v=True, train_bias_and_rms=False)
        P = O.init_params(cfg, seed=31, randomize_zero_init=True, init_std_factor=1.0)
        for i in range(1, cfg.depth):
            P[f"blocks.{i}.lambda_param"] = torch.tensor([0.2 + 0.15 * i])
        g = torch.Generator().manual_seed(6)
        x = torch.randn(2, 16, 4, 8, 8, generator=g).to(bf16).cuda()
        c = torch.randn(2, 16, 64, generator=g).to(bf16).cuda()
        t = torch.rand(2, generator=g).to(bf16).cuda()
        v = torch.randn(2, 16, 4, 8, 8, generator=g).to(bf16).cuda()

        def run(mode, sharded):
            m = build(vds, cfg, P, mode)
            if sharded:
                m = apply_fsdp(m, torch.bfloat16, torch.float32, force_runtime=True,
                               reshard_after_forward=sharded == "reshard_after_forward")
                assert m._fsdp is not None and m.recompute == mode
            out = m(x, c, t, rope_start=(1, 2, 3))
            loss, _ = vds["train"].flow_loss(out, v)
            loss.backward()
            torch.cuda.synchronize()
            # (one rank: every parameter's gradient shard is the whole fp32 gradient)
            grads = {k: q.grad.detach().flatten().clone() for k, q in m.named_parameters()}
            return loss.item(), grads

        l0, g0 = run("none", False)
        assert all(q.numel() == P[k].numel() for k, q in g0.items()) and sum(float(q.abs().sum()) for q in g0.values()) > 0
        for sharded in (True, "reshard_after_forward"):
            for mode in MODES:
                l1, g1 = run(mode, sharded)
                assert l1 == l0, (sharded, mode, l0, l1)
                diff = [k for k in g0 if not torch.equal(g1[k], g0[k])]
                assert not diff, (sharded, mode, diff)
    finally:
        comm.destroy()
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------- 7. graph capture ----
def test_graph_replay_matches_eager_selective(vds):
    """GraphedTrainStep with "selective": two eager steps, capture, three replays against five eager "selective" steps,
    within the bounds test_graph_replay_matches_eager_steps states (losses 1e-4, parameters 2e-4 relative)."""
    from video_diffusion_speedrun_amd.graph import GraphedTrainStep
    cfg = O.DiTConfig(in_channels=16, hidden_size=128, depth=3, num_heads=2, cross_attn_input_size=64,
                      residual_v=True, train_bias_and_rms=False)
    P = O.init_params(cfg, seed=41, randomize_zero_init=True, init_std_factor=1.0)
    g = torch.Generator().manual_seed(5)
    batches = [{"latent": torch.randn(2, 16, 4, 8, 8, generator=g).cuda(), "context": torch.randn(2, 16, 64, generator=g).cuda(),
                "prompt": ["", ""]} for _ in range(5)]
    results = []
    for graphed in (False, True):
        m = build(vds, cfg, P, "selective")
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
    print("graph selective: worst loss rel", max(abs(a - b) / abs(a) for a, b in zip(l0, l1)),
          "worst param rel", max(rel(p1[k], p0[k]) for k in p0))
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    for k in p0:
        assert rel(p1[k], p0[k]) <= 2e-4, (k, rel(p1[k], p0[k]))


# ------------------------------------------------------------------------------- 8. lean epilogues ----
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("M_rows", [2 * 8208, 2 * 8208 - 104, 200], ids=["M16416", "M16312_edge", "M200_small_tiles"])
def test_single_output_epilogues_store_the_same_bits(vds, M_rows, bias):
    """DiT-XL's fc1 (N = 4608) and gated (N = 1152) shapes, K = 1152 and 4608: `act` with want_pre=False and `x_new` with
    want_y=False equal the two-output launches bit for bit, through every tiling (auto picks the 256^2 kernel at the
    large M; 128 and 256 x 128 are forced too), with rows that end inside a tile and samples that end inside a
    sub-tile (rows_per_batch = M / 2 is not a multiple of 64)."""
    ops = vds["ops"]
    D = 1152
    g = torch.Generator().manual_seed(M_rows + bias)
    rn = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(bf16).cuda()
    x, h = rn(M_rows, D), rn(M_rows, 4 * D)
    W1, W2, Wp = rn(4 * D, D) * 0.06, rn(D, 4 * D) * 0.03, rn(D, D) * 0.06
    b1, b2 = (rn(4 * D), rn(D)) if bias else (None, None)
    res = rn(M_rows, D)
    mod = torch.randn(2, 9 * D, generator=g).cuda()
    L = M_rows // 2
    for tile in (0, 128, 256, 2):
        prev = ops.gemm_force_tile(tile)
        try:
            pre, act = ops.linear_fwd_gelu(x, W1, b1)
            none, act1 = ops.linear_fwd_gelu(x, W1, b1, want_pre=False)
            assert none is None and torch.equal(act1, act), ("fc1", tile)
            assert float(act.float().abs().max()) > 0
            for a, W, b, col in ((h, W2, b2, 8 * D), (x, Wp, None, 2 * D)):
                y, xn = ops.linear_fwd_gate_res(a, W, b, mod, col, res, L)
                none, xn1 = ops.linear_fwd_gate_res(a, W, b, mod, col, res, L, want_y=False)
                assert none is None and torch.equal(xn1, xn), ("gate_res", tile, col)
                # the replay's fc2 / projections: the plain store epilogue gives the bits of the gated launch's `y`
                assert torch.equal(ops.linear_fwd(a, W, b), y), ("store", tile, col)
        finally:
            ops.gemm_force_tile(prev)


@pytest.mark.parametrize("name", ["g1_tiny_hd64.pt", "g1_tiny_hd72.pt"])
def test_no_grad_forward_is_bit_equal_to_the_saving_forward(vds, golden_dir, name):
    fx = torch.load(os.path.join(golden_dir, name), weights_only=False)
    cfg = O.DiTConfig(**fx["cfg"])
    P = O.init_params(cfg, **fx["param_init"])
    P.update({k: v.clone() for k, v in fx["param_tweaks"].items()})
    m = build(vds, cfg, P)
    x, ctx, t = fx["x"].cuda().to(bf16), fx["context"].cuda().to(bf16), fx["t"].cuda().to(bf16)
    out = m(x, ctx, t, rope_start=tuple(fx["rope_start"]))
    assert out.requires_grad
    with torch.no_grad():
        out_ng = m(x, ctx, t, rope_start=tuple(fx["rope_start"]))
    assert not out_ng.requires_grad and torch.equal(out_ng, out.detach())
    for mode in MODES:  # the first forward of a recomputing model is that lean pass too
        assert torch.equal(m.enable_recompute(mode)(x, ctx, t, rope_start=tuple(fx["rope_start"])).detach(), out.detach())


# ------------------------------------------------------------------------------------- 9. memory ----
# Slack of the forward-delta check, on top of activation_bytes(...)["kept"]:
#   * 2 %: torch's caching allocator hands out blocks in multiples of 512 bytes, and a block of this model keeps ~25
#     tensors (a few hundred over 12 blocks); at the C1 shape the smallest of them (rstd: 4 KB, mod: 55 KB) lose up to 12 %
#     each to that rounding, the large ones nothing -- well under 2 % of the sum;
#   * 4 MiB: what rides along outside the blocks and is the same in every mode -- the output [4,16,8,16,16] bf16 (64 KB),
#     the root-level saves (patches 0.5 MB, block 0's v as v_0 0.8 MB, x_last / xnf 2 x 0.8 MB, cos / sin, the text
#     context's bf16 copy when the caller's was not contiguous) -- about 3 MB at this shape.
MEM_REL, MEM_ABS = 0.02, 4 << 20


def test_memory_kept_matches_the_accounting(vds):
    M = vds["model"]
    cfg = O.DiTConfig(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=384, depth=12, num_heads=6,
                      cross_attn_input_size=4096, residual_v=True, train_bias_and_rms=False)  # C1: DiT-S/2
    P = O.init_params(cfg, seed=7, randomize_zero_init=True, init_std_factor=0.1)
    B, lat, Lc = 4, (16, 8, 16, 16), 512
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, *lat, generator=g).to(bf16).cuda()
    c = torch.randn(B, Lc, 4096, generator=g).to(bf16).cuda()
    t = torch.rand(B, generator=g).to(bf16).cuda()
    v = torch.randn(B, *lat, generator=g).to(bf16).cuda()
    peaks, acct = {}, {}
    for mode in ("none",) + MODES:
        m = build(vds, cfg, P, mode)
        for _ in range(2):  # (first pass: compute copies, gradient buffers and p.grad come into being)
            m.zero_grad()
            out = m(x, c, t, rope_start=(1, 2, 3))
            vds["train"].flow_loss(out, v)[0].backward()
            del out
        m.zero_grad()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = m(x, c, t, rope_start=(1, 2, 3))
        torch.cuda.synchronize()
        delta = torch.cuda.memory_allocated() - before
        a = M.activation_bytes(m, B, lat[1:], Lc, mode)
        acct[mode] = a
        print(f"{mode}: forward keeps {delta} bytes, accounting {a['kept']} (+{(delta - a['kept']) / a['kept']:.2%})")
        assert delta >= a["kept"], (mode, delta, a)
        assert delta <= a["kept"] * (1 + MEM_REL) + MEM_ABS, (mode, delta, a)
        vds["train"].flow_loss(out, v)[0].backward()
        torch.cuda.synchronize()
        peaks[mode] = torch.cuda.max_memory_allocated() - before
        del out, m
    print("peaks over forward + backward, above the resident state:", peaks)
    per_block_saving = acct["none"]["per_block"] - acct["full"]["per_block"]
    assert peaks["none"] - peaks["full"] >= (cfg.depth - 2) * per_block_saving, (peaks, per_block_saving)
    assert peaks["none"] - peaks["selective"] >= (cfg.depth - 2) * (acct["none"]["per_block"] - acct["selective"]["per_block"])
