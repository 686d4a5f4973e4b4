"""LoRA without a GPU: what DiT.add_lora registers and freezes, every refusal, the adapter state dict and merge_lora
against float64, the C ABI of the low-rank kernels (declared, bound, host-side argument checks: nothing is launched), the
exactness conditions of the exact-input builder, and injected faults in the restatement (tests/helpers/lora_ref.py)."""
import ctypes as C
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lora_ref as LR  # noqa: E402

from video_diffusion_speedrun_amd import _lib  # noqa: E402
from video_diffusion_speedrun_amd import model as M  # noqa: E402

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
CONST = ["patch_proj", "context_kv", "positional_embedding"]


def tiny(**kw):
    torch.manual_seed(0)
    return M.DiT(in_channels=16, hidden_size=128, depth=2, num_heads=2, cross_attn_input_size=64, residual_v=True,
                 train_bias_and_rms=False, **kw)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---- add_lora ---------------------------------------------------------------------------------------------------------
def test_add_lora_registers_adapters_and_freezes_the_base():
    m = tiny()
    base = {n: p.detach().clone() for n, p in m.named_parameters()}
    assert m.add_lora(rank=16, generator=torch.Generator().manual_seed(1)) is m
    named = dict(m.named_parameters())
    new = [n for n in named if n not in base]
    want = [f"blocks.{i}.{t}.lora_{ab}" for i in range(2) for t in ("qkv", "q_cross", "context_kv") for ab in "AB"]
    assert sorted(new) == sorted(want)
    shapes = {"qkv": (384, 128), "q_cross": (128, 128), "context_kv": (256, 64)}
    for i in range(2):
        for t, (out, inn) in shapes.items():
            A, B = named[f"blocks.{i}.{t}.lora_A"], named[f"blocks.{i}.{t}.lora_B"]
            assert tuple(A.shape) == (16, inn) and tuple(B.shape) == (out, 16)
            assert A.dtype == f32 and B.dtype == f32
            assert B.abs().max().item() == 0.0
            assert 0 < A.abs().max().item() <= inn ** -0.5 and A.std().item() > 0.3 * inn ** -0.5
    # flags: the base is frozen and bit-unchanged, the adapters train
    for n, p in named.items():
        assert p.requires_grad == (n in new), n
        if n in base:
            assert torch.equal(p, base[n])
    assert m.paramstatus.keys() == named.keys()
    for n, info in m.paramstatus.items():
        assert info["requires_grad"] == (n in new) and tuple(info["shape"]) == tuple(named[n].shape)
    assert m._groups is None and m.lora == {"rank": 16, "alpha": 16.0, "targets": ("qkv", "q_cross", "context_kv")}
    assert all(b.lora_scale == 1.0 for b in m.blocks)
    # same generator seed, same A; alpha sets the scale
    m2 = tiny().add_lora(rank=16, alpha=4, generator=torch.Generator().manual_seed(1))
    assert torch.equal(m2.blocks[1].qkv.lora_A, m.blocks[1].qkv.lora_A) and m2.blocks[0].lora_scale == 0.25


def test_constructor_signatures_are_unchanged():
    for cls in (M.DiT, M.DiTBlock):
        names = list(inspect.signature(cls.__init__).parameters)
        assert names[-3:] == ["frame_chunk", "frame_window", "qk_norm"]
        assert not any("lora" in n for n in names)
    assert list(inspect.signature(M.DiT.add_lora).parameters) == ["self", "rank", "alpha", "targets", "freeze_base",
                                                                  "generator"]
    d = inspect.signature(M.DiT.add_lora).parameters
    assert d["rank"].default == 16 and d["alpha"].default is None and d["freeze_base"].default is True
    assert d["targets"].default == ("qkv", "q_cross", "context_kv") and d["generator"].default is None


def test_optimizer_setups_of_a_lora_model():
    m = tiny().add_lora(rank=32, targets=("qkv", "context_kv"))
    groups, table = m.get_mup_setup(1e-3, 0.1, CONST)
    adapters = {n for n, _ in m.lora_parameters()}
    assert len(adapters) == 8 and set(table) == adapters  # nothing frozen comes back
    assert all(p.requires_grad for g in groups for p in g["params"])
    lg, lt = m.get_lora_setup(2e-3, 0.01)
    assert set(lt) == adapters and len(lg) == 1 and len(lg[0]["params"]) == 8
    assert lg[0]["lr"] == 2e-3 and lg[0]["weight_decay"] == 0.01
    named = dict(m.named_parameters())
    for n, row in lt.items():
        assert row == {"lr": 2e-3, "wd": 0.01, "shape": named[n].shape}
    assert {id(p) for p in lg[0]["params"]} == {id(named[n]) for n in adapters}
    assert m.get_lora_setup(1e-3)[0][0]["weight_decay"] == 0.0
    mg, mt = m.get_muon_setup(1e-3, 0.1, CONST)
    assert not any(g.get("use_muon") for g in mg) and not any(r.get("muon") for r in mt.values())
    # a model without LoRA keeps the g4 cascade: get_mup_setup is untouched by an unfrozen add_lora too
    plain = tiny()
    ref = plain.get_mup_setup(1e-3, 0.1, CONST)[1]
    unfrozen = tiny().add_lora(freeze_base=False)
    got = unfrozen.get_mup_setup(1e-3, 0.1, CONST)[1]
    assert {k: (v["lr"], v["wd"]) for k, v in got.items() if k in ref} == {k: (v["lr"], v["wd"]) for k, v in ref.items()}
    assert all(p.requires_grad for p in unfrozen.parameters())
    # freezing by hand: refresh_paramstatus() is the public way to bring the setups' table up to date
    for n, p in plain.named_parameters():
        p.requires_grad_(n == "register_tokens")
    plain.refresh_paramstatus()
    assert list(plain.get_mup_setup(1e-3, 0.1, CONST)[1]) == ["register_tokens"]


def test_activation_bytes_count_the_kept_u():
    """the forward keeps u = x A^T of every adapted linear: 2 r bytes per row of its input"""
    plain, m = tiny(), tiny().add_lora(rank=32, targets=("qkv", "context_kv"))
    B, lat, Lc = 2, (2, 8, 8), 8
    a0, a1 = M.activation_bytes(plain, B, lat, Lc), M.activation_bytes(m, B, lat, Lc)
    rows = a0["rows"]
    assert a1["per_block"] - a0["per_block"] == 2 * 32 * (rows + B * Lc)
    for mode in ("full", "selective"):  # the replay recomputes u: nothing more is kept
        assert M.activation_bytes(m, B, lat, Lc, mode)["per_block"] == M.activation_bytes(plain, B, lat, Lc, mode)["per_block"]


def test_every_refusal_names_its_remedy():
    m = tiny().add_lora()
    with pytest.raises(ValueError, match="merge_lora"):
        m.add_lora()
    with pytest.raises(ValueError, match="attn_proj"):
        tiny().add_lora(targets=("qkv", "attn_proj"))
    with pytest.raises(ValueError, match="distinct"):
        tiny().add_lora(targets=("qkv", "qkv"))
    for r in (0, 8, 24, 128, True):
        with pytest.raises(ValueError, match=r"\(16, 32, 64\)"):
            tiny().add_lora(rank=r)
    with pytest.raises(ValueError, match="alpha"):
        tiny().add_lora(alpha=0)
    with pytest.raises(NotImplementedError, match="merge_lora"):
        m.enable_fp8()
    with pytest.raises(NotImplementedError, match=r"enable_fp8\(False\)"):
        tiny().enable_fp8().add_lora()
    from video_diffusion_speedrun_amd import fsdp
    with pytest.raises(NotImplementedError, match="merge_lora"):
        fsdp.apply_fsdp(m)
    sharded = tiny()
    sharded._world = 2  # what apply_fsdp leaves on a sharded model
    with pytest.raises(NotImplementedError, match="unsharded"):
        sharded.add_lora()
    with pytest.raises(ValueError, match="add_lora"):
        tiny().get_lora_setup(1e-3)
    with pytest.raises(ValueError, match="add_lora"):
        tiny().lora_state_dict()
    with pytest.raises(ValueError, match="add_lora"):
        tiny().merge_lora()
    with pytest.raises(ValueError, match="qkv"):
        M.DiT(in_channels=16, hidden_size=128, depth=1, num_heads=2, cross_attn_input_size=None).add_lora(
            targets=("q_cross",))
    assert m.enable_fp8(False) is m  # switching fp8 OFF on a LoRA model is not refused


# ---- state and merge ---------------------------------------------------------------------------------------------------
def _randomize(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.lora_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.05)


def test_lora_state_dict_round_trip_and_mismatches():
    m = tiny().add_lora(rank=16, alpha=8)
    _randomize(m, 3)
    sd = m.lora_state_dict()
    assert sd["rank"] == 16 and sd["alpha"] == 8.0 and sd["targets"] == ["qkv", "q_cross", "context_kv"]
    assert {k for k in sd if k not in ("rank", "alpha", "targets")} == {n for n, _ in m.lora_parameters()}
    m2 = tiny().add_lora(rank=16, alpha=8)
    m2.load_lora_state_dict(sd)
    for (n, p), (_, q) in zip(m.lora_parameters(), m2.lora_parameters()):
        assert torch.equal(p, q), n
    # the full state dict carries the extra keys and round-trips through load_state_dict
    m3 = tiny().add_lora(rank=16, alpha=8)
    m3.load_state_dict(m.state_dict(), strict=True)
    assert torch.equal(m3.blocks[1].context_kv.lora_B, m.blocks[1].context_kv.lora_B)
    for bad in (dict(sd, rank=32), dict(sd, alpha=16.0), dict(sd, targets=["qkv"]),
                {k: v for k, v in sd.items() if k != "blocks.0.qkv.lora_A"},
                dict(sd, extra=torch.zeros(1)), dict(sd, **{"blocks.0.qkv.lora_A": torch.zeros(16, 64)})):
        with pytest.raises(ValueError):
            m2.load_lora_state_dict(bad)
    with pytest.raises(ValueError, match="add_lora"):
        tiny().load_lora_state_dict(sd)


def test_merge_lora_against_float64():
    plain = tiny()
    keys = list(plain.state_dict().keys())
    m = tiny().add_lora(rank=32, alpha=8, generator=torch.Generator().manual_seed(2))
    _randomize(m, 4)
    s = 8 / 32
    want = {}
    for i, blk in enumerate(m.blocks):
        for t in ("qkv", "q_cross", "context_kv"):
            lin = getattr(blk, t)
            want[f"blocks.{i}.{t}.weight"] = LR.merged_weight(lin.weight.detach(), lin.lora_A.detach(),
                                                              lin.lora_B.detach(), s)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert m.merge_lora() is m
    sd = m.state_dict()
    assert list(sd.keys()) == keys and m.lora is None and all(b.lora_scale is None for b in m.blocks)
    assert all(p.requires_grad for p in m.parameters())
    assert all(v["requires_grad"] for v in m.paramstatus.values()) and list(m.paramstatus) == keys
    for k in keys:
        if k in want:
            # fp32 result of a rank-32 product: a few ulp of the largest term
            err = (sd[k].to(f64) - want[k]).abs().max().item()
            assert err <= 8 * 2.0 ** -24 * want[k].abs().max().item(), (k, err)
            assert not torch.equal(sd[k], before[k])
        else:
            assert torch.equal(sd[k], before[k]), k
    m.add_lora()  # a merged model takes new adapters


# ---- C ABI ------------------------------------------------------------------------------------------------------------
NEW = ("vds_lowrank_down", "vds_lowrank_up_add", "vds_lowrank_wgrad", "vds_lowrank_wgrad_workspace_floats",
       "vds_lowrank_chunk")


def test_new_symbols_are_declared_bound_and_in_the_makefile(lib):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(repo, "include", "vds.h")).read()
    for name in NEW:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    mk = open(os.path.join(repo, "video_diffusion_speedrun_amd", "csrc", "Makefile")).read()
    assert "lowrank.hip" in mk
    assert lib.vds_prof_class_name(_lib.PROF_NCLASS - 1) == b"fp8_quant"  # no profiler class was appended
    for r in LR.RANKS:
        assert lib.vds_lowrank_chunk(0, r) == LR.down_chunk(r) and lib.vds_lowrank_chunk(1, r) == LR.up_chunk(r)
        assert lib.vds_lowrank_chunk(2, r) == LR.WGRAD_CHUNK
        # the staged piece fits the 32 KB stage in both images of the small matrix
        assert r * (2 * LR.down_chunk(r) + 16) <= LR.LDS_STAGE and LR.down_chunk(r) * (2 * r + 16) <= LR.LDS_STAGE
        assert LR.up_chunk(r) * (2 * r + 16) <= LR.LDS_STAGE
    assert lib.vds_lowrank_chunk(0, 8) == 0
    assert lib.vds_lowrank_wgrad_workspace_floats(1, 8, 16) == 8 * 16
    assert lib.vds_lowrank_wgrad_workspace_floats(2048, 32, 16) == 32 * 16
    assert lib.vds_lowrank_wgrad_workspace_floats(2049, 32, 64) == 2 * 32 * 64
    assert lib.vds_lowrank_wgrad_workspace_floats(2049, 32, 24) == 0


def test_host_side_refusals_launch_nothing(lib):
    """every NULL / bad-r / bad-layout / bad-ld / misaligned / short-ws call returns VDS_ERR_ARG and leaves its own
    message.  The calls carry made-up device addresses, so they run in a child process that sees no GPU
    (tests/helpers/lora_refusals.py): were a host-side check ever lost, the launch fails there instead of running."""
    import subprocess
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "lora_refusals.py")
    sys.path.insert(0, os.path.dirname(script))
    import lora_refusals
    env = dict(os.environ, **lora_refusals.HIDE)
    r = subprocess.run([sys.executable, script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout
    assert "56 refusals checked, 0 wrong" in r.stdout, r.stdout  # 20 + 17 + 19 defects


def test_wrappers_refuse_operands_the_kernel_would_misread():
    """ops.lowrank_*: a wrong shape, dtype or layout raises before anything is handed to the library (CPU tensors here:
    a well-formed call would go on to the GPU-only assertion, which is not reached)"""
    from video_diffusion_speedrun_amd import ops
    z = lambda *s, dt=bf16: torch.zeros(*s, dtype=dt)  # noqa: E731
    x, A, Bm, u, y = z(4, 32), z(16, 32), z(24, 16), z(4, 16), z(4, 24)
    for bad in (lambda: ops.lowrank_down(x, z(16, 40)), lambda: ops.lowrank_down(x, z(16, 32, dt=f32)),
                lambda: ops.lowrank_down(x.float(), A), lambda: ops.lowrank_down(x, A, out=z(5, 16)),
                lambda: ops.lowrank_down(x, A, out=z(4, 16, dt=f32)), lambda: ops.lowrank_down(x, A, layout=1),
                lambda: ops.lowrank_down(x, A, layout=2),
                lambda: ops.lowrank_up_add(u, z(24, 32), y), lambda: ops.lowrank_up_add(u, Bm, y, layout=1),
                lambda: ops.lowrank_up_add(z(5, 16), Bm, y), lambda: ops.lowrank_up_add(u, Bm, y.float()),
                lambda: ops.lowrank_up_add(u, Bm.float(), y),
                lambda: ops.lowrank_wgrad(y, u, z(24, 16)), lambda: ops.lowrank_wgrad(y, u, z(16, 24, dt=f32)),
                lambda: ops.lowrank_wgrad(y, z(5, 16), z(24, 16, dt=f32)),
                lambda: ops.lowrank_wgrad(y, u, z(24, 16, dt=f32), layout=1),
                lambda: ops.lowrank_wgrad(y.float(), u, z(24, 16, dt=f32)),
                lambda: ops.lowrank_wgrad(y, u, z(24, 16, dt=f32), ws=z(24 * 16))):
        with pytest.raises(ValueError, match="lowrank_"):
            bad()
    with pytest.raises(AssertionError, match="GPU"):  # well-formed, but on the CPU
        ops.lowrank_down(x, A)


# ---- the exact-input builder and injected faults ------------------------------------------------------------------------
CASES = [("down", 65, 96, 16, 0), ("down", 17, 704, 16, 1), ("down", 33, 256, 64, 0),
         ("up_add", 65, 96, 32, 0), ("up_add", 17, 384, 64, 1),
         ("wgrad", 257, 96, 16, 0), ("wgrad", 2 * LR.WGRAD_CHUNK + 100, 32, 32, 1)]


@pytest.mark.parametrize("kind,Mr,W,r,layout", CASES)
def test_exact_builder_conditions_hold(kind, Mr, W, r, layout):
    """the builder asserts exact partial sums and representable outputs itself; here: its expectation equals a plain
    float64 formula to the bit, and scale / layout / accumulate each matter"""
    c = LR.exact_case(kind, Mr, W, r, layout, scale=0.5)
    if kind == "down":
        w = c["w"].to(f64) if layout == 0 else c["w"].to(f64).t()
        want = 0.5 * (c["x"].to(f64) @ w.t())
        assert c["expect"].dtype == bf16 and torch.equal(c["expect"].to(f64), want) and want.abs().max() > 0
        assert tuple(c["w"].shape) == ((r, W) if layout == 0 else (W, r))
    elif kind == "up_add":
        w = c["w"].to(f64) if layout == 0 else c["w"].to(f64).t()
        want = c["y"].to(f64) + 0.5 * (c["u"].to(f64) @ w.t())
        assert c["expect"].dtype == bf16 and torch.equal(c["expect"].to(f64), want)
        assert not torch.equal(c["expect"], c["y"])
    else:
        acc = 0.5 * (c["a"].to(f64).t() @ c["u"].to(f64))
        want = c["g"].to(f64) + (acc if layout == 0 else acc.t())
        assert c["expect"].dtype == f32 and torch.equal(c["expect"].to(f64), want) and c["g"].abs().max() > 0
    # a second build gives the same bits (seeded)
    assert torch.equal(LR.exact_case(kind, Mr, W, r, layout, scale=0.5)["expect"], c["expect"])


def _rel(a, b):
    a, b = a.to(f64).flatten(), b.to(f64).flatten()
    return ((a - b).norm() / b.norm()).item()


MODEL_BOUND = 3e-2  # GRAD_REL of tests/test_model_gpu.py: the norm bound of the model-level comparisons


def test_injected_faults_are_flagged_bitwise():
    """One defect at a time in the restatement.  The bitwise comparison flags every one.  The relative-norm comparison
    at the model-level bound (3e-2) MISSES the dropped last M chunk of the weight gradient when that chunk is short --
    one row past a full chunk of 2048 changes the sum by about sqrt(1 / 2049) = 2.2e-2 of its norm -- and sees the
    other three: the wrong layout and the dropped scale change everything, and a dropped last K chunk of 32 of 704
    columns is sqrt(32 / 704) = 0.21 of the norm."""
    missed = {}
    # down: K = 704 crosses the r = 16 chunk of 672: the last chunk holds 32 of 704 columns
    c = LR.exact_case("down", 33, 704, 16, 0, scale=0.5)
    assert LR.down_chunk(16) == 672
    # (a denser x than the builder's, so that the last chunk surely contributes)
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-1, 2, (33, 704), generator=g).to(bf16)
    good = LR.down(x, c["w"], 0, 0.5)
    for fault in ("layout", "scale", "k_chunk"):
        bad = LR.down(x, c["w"], 0, 0.5, fault=fault)
        assert not torch.equal(bad, good), fault
        missed["down." + fault] = _rel(bad, good) <= MODEL_BOUND
    # up_add
    c = LR.exact_case("up_add", 33, 96, 32, 0, scale=0.5)
    for fault in ("layout", "scale"):
        bad = LR.up_add(c["u"], c["w"], 0, c["y"], 0.5, fault=fault)
        assert not torch.equal(bad, c["expect"]), fault
        missed["up_add." + fault] = _rel(bad, c["expect"]) <= MODEL_BOUND
    # wgrad: one full chunk and one row
    c = LR.exact_case("wgrad", LR.WGRAD_CHUNK + 1, 32, 16, 0, scale=0.5)
    for fault in ("layout", "scale", "m_chunk"):
        bad = LR.wgrad(c["a"], c["u"], c["g"], 0, 0.5, fault=fault)
        assert not torch.equal(bad, c["expect"]), fault
        missed["wgrad." + fault] = _rel(bad, c["expect"]) <= MODEL_BOUND
    assert {k for k, v in missed.items() if v} == {"wgrad.m_chunk"}, missed


def test_lora_linear_restatement_matches_the_merged_weight():
    """the restated LoRA'd linear (bf16 roundings as the kernels place them) agrees with x (W + s B A)^T + b to bf16
    accuracy: the identity the model-level tests lean on"""
    g = torch.Generator().manual_seed(6)
    x = torch.randn(40, 64, generator=g).to(bf16)
    W = (torch.randn(96, 64, generator=g) * 0.1).to(bf16)
    b = (torch.randn(96, generator=g) * 0.1).to(bf16)
    A = (torch.randn(16, 64, generator=g) * 0.1).to(bf16)
    Bm = (torch.randn(96, 16, generator=g) * 0.1).to(bf16)
    y, u = LR.lora_linear(x, W, b, A, Bm, 0.5)
    assert y.dtype == bf16 and tuple(u.shape) == (40, 16)
    want = x.to(f64) @ LR.merged_weight(W, A, Bm, 0.5).t() + b.to(f64)
    assert _rel(y, want) <= 3 * 2.0 ** -8  # three bf16 roundings (u, the base output, the sum)
    y0, _ = LR.lora_linear(x, W, b, A, torch.zeros_like(Bm), 0.5)
    assert torch.equal(y0, (x.to(f64) @ W.to(f64).t() + b.to(f64)).to(f32).to(bf16))  # B = 0: the base output, bit for bit
