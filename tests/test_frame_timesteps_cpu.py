"""Per-frame timesteps without a GPU: the group map, the shape / validation errors of DiT.forward and the sampler, the
draw helpers of train.forward, the helper reference against the oracle for constant rows, and the ABI table."""
import os
import re
import sys

import pytest
import torch

from oracle import dit_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import frame_timesteps_ref as R  # noqa: E402

from video_diffusion_speedrun_amd import _lib, ops, train  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bf16, f32 = torch.bfloat16, torch.float32


def test_group_map():
    # 16 register rows, 3 token-frames, token order (h w t): rows 16, 19, 22, .. are frame 0
    got = [ops.mod_group_of(l, 16, 3) for l in range(16 + 9)]
    assert got == [0] * 16 + [1, 2, 3] * 3
    assert [ops.mod_group_of(l, 0, 4) for l in range(8)] == [1, 2, 3, 4, 1, 2, 3, 4]       # empty group 0
    assert [ops.mod_group_of(l, 2, 1) for l in range(5)] == [0, 0, 1, 1, 1]                # one frame
    assert [train.frame_group_of(l, 3) for l in (0, 15, 16, 17, 18, 19)] == [0, 0, 1, 2, 3, 1]
    for lead, period, L in ((16, 3, 91), (0, 4, 64), (16, 8, 24)):
        assert [ops.mod_group_of(l, lead, period) for l in range(L)] == R.group_index(L, lead, period).tolist()
        assert ops.check_mod_groups((lead, period), L) == (lead, period)


@pytest.mark.parametrize("groups,L", [((-1, 3), 20), ((16, 0), 20), ((16, 3), 20), ((21, 1), 20)])
def test_bad_group_descriptions_are_refused(groups, L):
    with pytest.raises(ValueError, match="modulation groups"):
        ops.check_mod_groups(groups, L)


def test_model_refuses_other_timestep_shapes():
    from video_diffusion_speedrun_amd.model import check_timesteps
    assert check_timesteps(torch.zeros(2), 2, 3) is False and check_timesteps(torch.zeros(2, 3), 2, 3) is True
    for bad in (torch.zeros(2, 2), torch.zeros(2, 6), torch.zeros(3), torch.zeros(2, 3, 1), torch.zeros(3, 3), [0.5, 0.5]):
        with pytest.raises(ValueError, match=r"\[2, 3\]"):
            check_timesteps(bad, 2, 3)


def test_first_frame_draws():
    B, n = 64, 5
    g = torch.Generator().manual_seed(3)
    t = train.draw_frame_levels("first_frame", B, n, "cpu", g)
    g2 = torch.Generator().manual_seed(3)
    assert t.dtype == bf16 and tuple(t.shape) == (B,)
    assert torch.equal(t, train.time_shift_from_normal(torch.randn(B, dtype=bf16, generator=g2)))  # the per-sample draw
    tf0, w0 = train.frame_schedule("first_frame", t, n, cond_prob=0.0, generator=g)
    assert torch.equal(tf0, t[:, None].expand(B, n)) and torch.equal(w0, torch.ones(B, n))
    tf1, w1 = train.frame_schedule("first_frame", t, n, cond_prob=1.0, generator=g)
    assert float(tf1[:, 0].abs().max()) == 0 and torch.equal(tf1[:, 1:], t[:, None].expand(B, n - 1))
    assert float(w1[:, 0].abs().max()) == 0 and torch.equal(w1[:, 1:], torch.ones(B, n - 1))
    tf, w = train.frame_schedule("first_frame", t, n, cond_prob=0.5, generator=g)
    assert w.dtype == f32 and tf.dtype == bf16 and tuple(tf.shape) == tuple(w.shape) == (B, n)
    zeroed = tf != t[:, None]          # (t > 0 always: the shifted sigmoid of a finite z)
    assert torch.equal(w == 0, zeroed) and torch.equal(w[:, 1:], torch.ones(B, n - 1))
    assert 0 < int(zeroed[:, 0].sum()) < B     # 64 coin flips: both outcomes occur
    with pytest.raises(ValueError):
        train.frame_schedule("first_frame", tf, n)


def test_independent_draws():
    g = torch.Generator().manual_seed(4)
    t = train.draw_frame_levels("independent", 3, 7, "cpu", g)
    assert t.dtype == bf16 and tuple(t.shape) == (3, 7) and float(t.min()) > 0 and float(t.max()) <= 1
    assert len(set(t.flatten().tolist())) > 10
    tf, w = train.frame_schedule("independent", t, 7)
    assert torch.equal(tf, t) and torch.equal(w, torch.ones(3, 7)) and w.dtype == f32
    with pytest.raises(ValueError):
        train.frame_schedule("independent", t, 6)
    with pytest.raises(ValueError):
        train.draw_frame_levels("every_other", 3, 7, "cpu")


def test_graphed_step_refuses_unknown_modes():
    from video_diffusion_speedrun_amd.graph import GraphedTrainStep
    with pytest.raises(ValueError, match="frame_mode"):
        GraphedTrainStep(None, None, None, "cpu", frame_mode="every_other")


def _case():
    cfg = O.DiTConfig(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=64, depth=2, num_heads=2,
                      cross_attn_input_size=32, residual_v=True, train_bias_and_rms=False)
    P = O.init_params(cfg, seed=5, randomize_zero_init=True, init_std_factor=1.0)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 16, 6, 4, 4, generator=g)
    ctx = torch.randn(2, 5, 32, generator=g)
    return cfg, P, x, ctx


def test_helper_reference_equals_the_oracle_for_constant_rows():
    cfg, P, x, ctx = _case()
    t = torch.tensor([0.25, 0.875])
    ref = O.dit_forward(P, cfg, x, ctx, t, (2, 3, 4))
    out = R.dit_forward(P, cfg, x, ctx, t[:, None].expand(2, 3).contiguous(), (2, 3, 4))
    assert float((out - ref).abs().max()) <= 1e-6 * max(1.0, float(ref.abs().max()))
    # and rows that differ change the output
    out2 = R.dit_forward(P, cfg, x, ctx, torch.tensor([[0.25, 0.25, 0.5], [0.875, 0.875, 0.875]]), (2, 3, 4))
    assert float((out2 - ref).abs().max()) > 1e-4
    assert float((out2[1] - ref[1]).abs().max()) <= 1e-6 * max(1.0, float(ref.abs().max()))  # sample 1 kept constant rows


def test_helper_noise_and_loss():
    g = torch.Generator().manual_seed(7)
    x, n = (torch.randn(2, 4, 6, 3, 3, generator=g).to(bf16) for _ in range(2))
    t = torch.tensor([0.5, 0.25]).to(bf16)
    zt0, v0 = O.noise_latents(x, n, t)
    zt1, v1 = R.noise_frames(x, n, t[:, None].expand(2, 3), 2)
    assert torch.equal(zt0, zt1) and torch.equal(v0, v1)
    tf = torch.tensor([[0.0, 0.5, 1.0], [0.25, 0.25, 0.75]]).to(bf16)
    zt, _ = R.noise_frames(x, n, tf, 2)
    assert torch.equal(zt[0, :, 0:2], x[0, :, 0:2]) and torch.equal(zt[0, :, 4:6], n[0, :, 4:6])
    out = torch.randn(2, 4, 6, 3, 3, generator=g).to(bf16)
    loss0, per0 = O.flow_loss(v0, out)
    loss1, per1, _ = R.frame_loss(v0, out, torch.ones(2, 3), 2)
    assert abs(loss0.item() - loss1.item()) <= 1e-6 * loss0.item() and torch.allclose(per0.double(), per1, rtol=1e-6)
    w = torch.tensor([[0.0, 0.0, 0.0], [0.0, 2.0, 1.0]])
    o = out.float().requires_grad_(True)
    loss, per, sse = R.frame_loss(v0, o, w, 2)
    loss.backward()
    assert per[0].item() == 0 and float(o.grad[0].abs().max()) == 0 and float(o.grad[1, :, 0:2].abs().max()) == 0
    assert abs(per[1].item() - (2 * sse[1, 1] + sse[1, 2]).item() / (4 * 2 * 9 * 3)) < 1e-12
    assert torch.isfinite(o.grad).all()


def test_abi_table_still_agrees_with_the_header():
    src = open(os.path.join(REPO, "include", "vds.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(vds_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_lib.SIGNATURES)
    new = {"vds_rmsnorm_mod_fwd_grouped", "vds_rmsnorm_mod_bwd_grouped", "vds_gate_bwd_grouped", "vds_gemm_bf16_grouped",
           "vds_noise_latents_frames", "vds_flow_loss_frames", "vds_flow_loss_frames_bwd",
           "vds_flow_loss_frames_workspace_floats"}
    assert new <= declared
    # each grouped call is its per-sample call plus one pointer (the group description) before the stream
    for name in ("vds_rmsnorm_mod_fwd", "vds_rmsnorm_mod_bwd", "vds_gate_bwd", "vds_gemm_bf16"):
        base, grp = _lib.SIGNATURES[name], _lib.SIGNATURES[name + "_grouped"]
        assert grp[:len(base) - 1] == base[:-1] and len(grp) == len(base) + 1
    import ctypes as C
    assert C.sizeof(_lib.ModGroups) == 8 and "} vds_mod_groups;" in src
    assert C.sizeof(_lib.GemmArgs) == 144  # the argument structs keep their layout


def test_library_checks_group_descriptions_on_the_host():
    """VDS_ERR_ARG before any launch: bad descriptions, and a group description on a GEMM that is not NT + GATE_RES"""
    import ctypes as C
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    one = C.c_void_p(16)  # non-null, never dereferenced: the argument checks come first
    L = 20
    for lead, period in ((-1, 3), (16, 0), (16, 3), (21, 1)):
        grp = C.byref(_lib.ModGroups(lead, period))
        assert lib.vds_rmsnorm_mod_fwd_grouped(one, 8, None, one, 16, 0, 8, one, 8, one, 1, L, 8, 1e-6, grp, None) == -1
        assert lib.vds_rmsnorm_mod_bwd_grouped(one, 8, one, 8, None, one, 16, 0, 8, one, None, 0, one, 8, one, None, 1, L, 8,
                                               grp, None) == -1
        assert lib.vds_gate_bwd_grouped(one, 8, one, 8, one, 8, 0, one, 8, one, None, 1, L, 8, grp, None) == -1
        a = _lib.GemmArgs(_lib.VDS_NT, _lib.EPI_GATE_RES, 2 * L, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, None, 16, 16, 16, 16,
                          L, 1, None)
        assert lib.vds_gemm_bf16_grouped(C.byref(a), grp, None) == -1
    ok = C.byref(_lib.ModGroups(4, 2))
    # B * G modulation rows are the backward grids' y dimension: more than 65535 is refused, 65535 itself passes this check
    big = C.byref(_lib.ModGroups(0, 7))
    assert lib.vds_rmsnorm_mod_bwd_grouped(one, 8, one, 8, None, one, 16, 0, 8, one, None, 0, one, 8, one, None, 8192, 7, 8,
                                           big, None) == -1
    assert lib.vds_gate_bwd_grouped(one, 8, one, 8, one, 8, 0, one, 8, one, None, 8192, 7, 8, big, None) == -1
    a = _lib.GemmArgs(_lib.VDS_NT, _lib.EPI_STORE, 2 * L, 16, 16, 16, 16, 16, 16, 16, 16)
    assert lib.vds_gemm_bf16_grouped(C.byref(a), ok, None) == -1           # not GATE_RES
    a = _lib.GemmArgs(_lib.VDS_NT, _lib.EPI_GATE_RES, 2 * L + 1, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, None, 16, 16, 16, 16,
                      L, 1, None)
    assert lib.vds_gemm_bf16_grouped(C.byref(a), ok, None) == -1           # M is not a multiple of L
    assert lib.vds_noise_latents_frames(one, one, one, one, one, 1, 4, 5, 9, 2, None) == -1   # T % time_patch != 0
    assert lib.vds_flow_loss_frames_workspace_floats(2, 3, 6144) == 2 * 3 * 2 and lib.vds_flow_loss_frames_workspace_floats(0, 3, 8) == 0


def test_sampler_refuses_bad_conditioning_latents(monkeypatch):
    from video_diffusion_speedrun_amd import sampling

    class M:
        time_patch_size = 2
    lat = torch.zeros(1, 16, 4, 4, 4)
    emb = torch.zeros(1, 4, 8)
    for bad in (torch.zeros(1, 16, 3, 4, 4), torch.zeros(1, 16, 6, 4, 4), torch.zeros(1, 16, 2, 4, 2), torch.zeros(16, 2, 4, 4)):
        with pytest.raises(ValueError, match="cond_latents"):
            sampling.generate_latents(M(), emb, latents=lat, cond_latents=bad, device="cpu", cfg_scale=1.0)
