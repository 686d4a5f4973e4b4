"""Activation recomputation, host side (no GPU): the public switch `DiT.enable_recompute` and the byte accounting
`model.activation_bytes`, checked against sums written out here from the shapes of the tensors `DiTBlock._fwd` keeps."""
import pytest

from video_diffusion_speedrun_amd import model as M

N_REG = 16


def _xl():
    return M.DiT(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=1152, depth=28, num_heads=16,
                 cross_attn_input_size=4096, residual_v=True, train_bias_and_rms=False)


def _g1(hd):
    # the configuration of tests/golden/g1_tiny_hd64.pt / g1_tiny_hd72.pt (oracle/make_golden.py)
    return M.DiT(in_channels=16, patch_size=2, time_patch_size=2, hidden_size=2 * hd, depth=2, num_heads=2,
                 cross_attn_input_size=64, residual_v=True, train_bias_and_rms=(hd == 72))


def test_modes_and_fp8_exclusion():
    m = _g1(64)
    assert m.recompute == "none"
    for mode in ("full", "selective", "none"):
        assert m.enable_recompute(mode) is m
        assert m.recompute == mode
    assert m.enable_recompute().recompute == "selective"  # the default argument
    with pytest.raises(ValueError):
        m.enable_recompute("bogus")
    assert m.recompute == "selective"  # a refused call changes nothing
    # fp8 + recomputation: refused whichever call comes last
    with pytest.raises(ValueError, match="fp8"):
        m.enable_fp8()
    assert not m.fp8
    m2 = _g1(64).enable_fp8()
    for mode in ("full", "selective"):
        with pytest.raises(ValueError, match="fp8"):
            m2.enable_recompute(mode)
    assert m2.recompute == "none"
    assert m2.enable_recompute("none") is m2  # today's behaviour stays available with fp8
    assert m2.enable_fp8(False).enable_recompute("full").recompute == "full"  # fp8 off again: allowed
    with pytest.raises(ValueError):
        M.activation_bytes(m, 1, (4, 8, 8), 8, "bogus")


def _expected(D, H, hd, hdp, depth, B, L, Lc):
    """bytes per block of every mode, from the list of kept tensors (bf16 = 2 bytes, f32 = 4)"""
    R = B * L
    elems_bf16 = (3 * R * D            # X, X1, X2
                  + R * D              # xn1
                  + R * 3 * D          # qkv
                  + 3 * B * H * L * hdp  # q, k, v in head-major rows padded to hdp
                  + R * D              # attn
                  + R * D              # y_sa
                  + 4 * R * D          # xn2, qc, catt, y_ca
                  + R * D              # xn3
                  + 2 * R * 4 * D      # hpre, hact
                  + R * D              # y_mlp
                  + B * Lc * 2 * D)    # ckv
    elems_f32 = (3 * R                 # rstd1, rstd2, rstd3
                 + 2 * B * H * L       # lse1, lse2
                 + B * 9 * D)          # mod
    none = 2 * elems_bf16 + 4 * elems_f32
    full = 2 * R * D + 4 * B * 9 * D
    selective = full + 2 * R * D + 4 * B * H * L
    return none, full, selective


@pytest.mark.parametrize("case", ["g1_hd64", "g1_hd72", "c3b_b12"])
def test_activation_bytes_equals_the_shape_sum(case):
    if case == "c3b_b12":
        m, B, lat, Lc, hdp = _xl(), 12, (16, 64, 64), 512, 96
        L = 8 * 32 * 32 + N_REG
        assert B * L == 98_496
    else:
        hd = int(case[-2:])
        m, B, lat, Lc, hdp = _g1(hd), 2, (4, 8, 8), 8, {64: 64, 72: 96}[hd]
        L = 2 * 4 * 4 + N_REG
    D, H, hd = m.hidden_size, m.num_heads, m.head_dim
    none, full, selective = _expected(D, H, hd, hdp, m.depth, B, L, Lc)
    for mode, per_block in (("none", none), ("full", full), ("selective", selective)):
        a = M.activation_bytes(m, B, lat, Lc, mode)
        assert a["rows"] == B * L
        assert a["per_block"] == per_block, (mode, a)
        assert a["kept"] == m.depth * per_block, (mode, a)
        assert a["transient"] == (0 if mode == "none" else none), (mode, a)
    if case == "c3b_b12":
        # the 27 D bf16 elements per token row of the issue's table: 62 208 bytes at D = 1152 (head dim 72 padded to 96)
        per_row_bf16 = 2 * (none - 4 * (3 * B * L + 2 * B * H * L + B * 9 * D) - 2 * B * Lc * 2 * D) // (2 * B * L)
        assert per_row_bf16 == 27 * D * 2 == 62_208
        assert 171e9 < 28 * none < 174e9  # "about 172 GB"
