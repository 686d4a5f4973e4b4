"""Muon without a GPU: which parameters `DiT.get_muon_setup` hands to Muon, the argument checks of `MuonAdamW` and of the
C ABI (host side: nothing is launched), the refusal of sharded models, and the sanity of the torch restatement that the
GPU tests measure against (tests/helpers/muon_ref.py)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import muon_ref as R  # noqa: E402

from video_diffusion_speedrun_amd import _lib, optim  # noqa: E402
from video_diffusion_speedrun_amd.model import DiT  # noqa: E402

CONSTS = ["patch_proj", "context_kv", "positional_embedding"]
SPLITS = {"qkv.weight": 3, "attn_proj.weight": 1, "q_cross.weight": 1, "context_kv.weight": 2, "cross_proj.weight": 1,
          "mlp.0.weight": 1, "mlp.2.weight": 1}
SHAPES = [(64, 64), (136, 136), (264, 264), (128, 512), (512, 128), (200, 328)]


def tiny(**over):
    kw = dict(in_channels=16, hidden_size=128, depth=3, num_heads=2, cross_attn_input_size=64, residual_v=True)
    kw.update(over)
    return DiT(**kw)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_get_muon_setup_partitions_the_parameters():
    m = tiny()
    groups, table = m.get_muon_setup(1e-3, 0.1, CONSTS, muon_lr=0.03, muon_weight_decay=0.01, momentum=0.9,
                                     nesterov=False, ns_steps=4)
    mup_groups, mup_table = m.get_mup_setup(1e-3, 0.1, CONSTS)
    names = {id(p): n for n, p in m.named_parameters()}
    seen = {}
    for g in groups:
        for p in g["params"]:
            assert id(p) not in seen, names[id(p)]          # none twice
            seen[id(p)] = g
    assert set(seen) == {id(p) for p in m.parameters() if p.requires_grad}  # none missing
    want = {f"blocks.{i}.{s}": k for i in range(3) for s, k in SPLITS.items()}
    got = {names[i]: g["muon_split"] for i, g in seen.items() if g.get("use_muon")}
    assert got == want
    for g in groups:
        if g.get("use_muon"):
            assert (g["lr"], g["weight_decay"], g["momentum"], g["nesterov"], g["ns_steps"]) == (0.03, 0.01, 0.9, False, 4)
            assert all(p.dim() == 2 for p in g["params"])
    # every other parameter keeps exactly the (lr, wd) of get_mup_setup
    for n, p in m.named_parameters():
        g = seen[id(p)]
        if n in want:
            assert table[n]["muon"] and table[n]["split"] == want[n] and table[n]["lr"] == 0.03
        else:
            assert "use_muon" not in g and (g["lr"], g["weight_decay"]) == (mup_table[n]["lr"], mup_table[n]["wd"]), n
            assert table[n] == mup_table[n]
    for tag in ("bias", "norm", "lambda_param", "adaLN_modulation", "patch_embed", "time_embed", "register_tokens",
                "final_modulation", "final_norm", "final_proj"):
        hit = [n for n in names.values() if tag in n]
        assert hit and not any(n in want for n in hit), tag


def test_setup_without_cross_attention_has_no_cross_matrices():
    m = tiny(cross_attn_input_size=None, depth=1)
    groups, _ = m.get_muon_setup(1e-3, 0.1, CONSTS)
    names = {id(p): n for n, p in m.named_parameters()}
    muon = sorted(names[id(p)] for g in groups if g.get("use_muon") for p in g["params"])
    assert muon == sorted(f"blocks.0.{s}" for s in ("qkv.weight", "attn_proj.weight", "mlp.0.weight", "mlp.2.weight"))


def test_argument_validation(lib):
    m = tiny(depth=1)
    for bad in (dict(muon_lr=0.0), dict(muon_weight_decay=-1.0), dict(momentum=1.0), dict(ns_steps=-1),
                dict(ns_steps=2.5)):
        with pytest.raises(ValueError):
            m.get_muon_setup(1e-3, 0.1, CONSTS, **bad)
    w = torch.nn.Parameter(torch.zeros(48, 16))
    for bad in (dict(muon_split=4), dict(momentum=1.5), dict(ns_steps=100), dict(muon_split=3, params=[
            torch.nn.Parameter(torch.zeros(32, 16))]), dict(params=[torch.nn.Parameter(torch.zeros(16))]),
            dict(params=[torch.nn.Parameter(torch.zeros(12, 16))])):
        g = dict({"params": [w], "lr": 0.02, "weight_decay": 0.0, "use_muon": True}, **bad)
        with pytest.raises(ValueError):
            optim.MuonAdamW([g])
    opt = optim.MuonAdamW([{"params": [w], "lr": 0.02, "weight_decay": 0.0, "use_muon": True, "muon_split": 3}])
    assert (opt.param_groups[0]["momentum"], opt.param_groups[0]["nesterov"], opt.param_groups[0]["ns_steps"]) == (0.95, True, 5)
    # C ABI: dimensions that are no multiple of 8, null pointers, bad counts -> VDS_ERR_ARG before any launch
    assert lib.vds_muon_workspace_bytes(1, 64, 64) > 0
    assert lib.vds_muon_workspace_bytes(1, 60, 64) == 0 and lib.vds_muon_workspace_bytes(0, 64, 64) == 0
    assert lib.vds_muon_workspace_bytes(3, 128, 512) == lib.vds_muon_workspace_bytes(3, 512, 128)
    off = (C.c_int64 * 6)()
    assert lib.vds_muon_workspace_layout(2, 64, 128, C.addressof(off)) == 0
    assert list(off)[:4] == [0, 2 * 64 * 128 * 2, 4 * 64 * 128 * 2, 4 * 64 * 128 * 2 + 2 * 64 * 64 * 2]
    assert off[5] + 256 == lib.vds_muon_workspace_bytes(2, 64, 128)
    assert lib.vds_muon_workspace_layout(2, 64, 100, C.addressof(off)) == -1
    assert lib.vds_muon_momentum(None, 1, 64, 64, 0.95, 1, None, None, None) == -1
    assert lib.vds_muon_momentum(16, 1, 64, 60, 0.95, 1, None, 16, None) == -1     # cols % 8
    assert lib.vds_muon_momentum(16, 1, 64, 64, 1.0, 1, None, 16, None) == -1      # mu
    assert lib.vds_muon_orthogonalize(None, 1, 64, 64, 5, None) == -1
    assert lib.vds_muon_orthogonalize(16, 1, 64, 64, -1, None) == -1
    assert lib.vds_muon_orthogonalize(16, 1, 4, 64, 5, None) == -1
    assert lib.vds_muon_update(None, 1, 64, 64, 0.02, 0.0, 1.0, 0.0, None, None, None, None) == -1
    assert lib.vds_muon_update(16, 1, 64, 64, 0.02, 0.0, 1.0, 1.0, None, None, 16, None) == -1  # ema_decay
    assert C.sizeof(_lib.MuonMat) == 40


def test_sharded_parameters_are_refused():
    from video_diffusion_speedrun_amd.fsdp import apply_fsdp
    m = apply_fsdp(tiny(depth=1), torch.bfloat16, torch.float32, device="cpu", world_rank=(2, 0))
    groups, _ = m.get_muon_setup(1e-3, 0.1, CONSTS)
    with pytest.raises(ValueError, match="whole matrices"):
        optim.MuonAdamW(groups)
    # the AdamW half alone still takes the shards
    optim.MuonAdamW([g for g in groups if not g.get("use_muon")])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_two_restatements_agree(shape):
    """sanity of the reference itself: the bf16-emulated form against float64 (measured 0.012-0.014 on Gaussian inputs
    of these shapes), and the float64 form does what Muon is for -- singular values pushed towards 1 (all but the
    near-zero ones of a square Gaussian matrix, which five steps cannot lift)"""
    u = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[0] * 7 + shape[1]))
    o64, oem = R.orthogonalize_f64(u), R.orthogonalize_emulated(u)
    err = R.rel_fro(oem, o64)
    print(f"emulated vs float64 {shape}: {err:.4f}")
    assert err < 0.03
    sv = torch.linalg.svdvals(o64)
    assert sv.max() < 1.3 and (sv > 0.5).double().mean() >= 0.9
    # transposing the input transposes the output: the tall path runs the same iteration
    assert R.rel_fro(R.orthogonalize_f64(u.t()).t(), o64) < 1e-12


def test_restated_step_splits_rows():
    g = torch.Generator().manual_seed(3)
    p, gr, buf = (torch.randn(48, 32, generator=g) for _ in range(3))
    pn, bn = R.step_f64(p, gr, buf, 0.02, 0.1, split=3)
    for k in range(3):
        sl = slice(16 * k, 16 * k + 16)
        p1, b1 = R.step_f64(p[sl], gr[sl], buf[sl], 0.02, 0.1)
        assert torch.equal(pn[sl], p1) and torch.equal(bn[sl], b1)
