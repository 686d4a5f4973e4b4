"""Token routing without a GPU: the reference of tests/helpers/routing_ref.py tells the routed model from the unrouted one
and from three wrong implementations (floors computed from the references alone); DiT.draw_route and the idx / inv tables;
the argument errors of enable_token_routing and of forward(route=); every refusal, in both orders where there are two; the
host-side refusals of the three C entries; activation_bytes(routing=)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import routing_ref as RR  # noqa: E402

from video_diffusion_speedrun_amd import _lib  # noqa: E402
from video_diffusion_speedrun_amd import model as M  # noqa: E402

B_OUT, B_GRAD = 2.5e-2, 3e-2  # the constants of tests/test_frame_causal_gpu.py
rel = RR.rel


def tiny(depth=4, **kw):
    return M.DiT(in_channels=16, hidden_size=128, depth=depth, num_heads=2, cross_attn_input_size=64, residual_v=True,
                 train_bias_and_rms=False, **kw)


# ------------------------------------------------------------------------------ the reference discriminates ----
@pytest.mark.parametrize("name", ["hd72", "hd64"])
def test_the_reference_tells_routing_and_its_defects_apart(name):
    """floors computed from the references alone (the library enters only through the tables the reference is checked to
    share with it)"""
    cs = RR.case(name)
    idx, inv = M.route_tables(cs["route"].to(torch.int32), RR.N_TOK)  # the reference routes the rows the library routes
    r_idx, r_inv = RR.tables(cs["route"], RR.N_TOK)
    assert torch.equal(idx.long(), r_idx) and torch.equal(inv.long(), r_inv)
    ref, full = RR.reference_step(name), RR.reference_step(name, route=None)
    d_out = rel(full["out"], ref["out"])
    print(f"{name}: routed vs unrouted reference: out {d_out:.3f}")
    assert d_out >= 2 * B_OUT, d_out
    moved = {}
    for defect in ("dv0", "rope", "bypass"):
        bad = RR.reference_step(name, defect=defect)
        moved[defect] = {k: rel(bad["grads"][k], ref["grads"][k]) for k in ref["grads"]
                         if k.startswith("blocks.") and not k.endswith("lambda_param")}
        print(f"{name} defect {defect}: out moves {rel(bad['out'], ref['out']):.3f}, blocks.0.qkv.weight "
              f"{moved[defect]['blocks.0.qkv.weight']:.3f}, worst block gradient {max(moved[defect].values()):.3f}")
    assert moved["dv0"]["blocks.0.qkv.weight"] >= 2 * B_GRAD  # the d v_0 path ends in block 0's qkv
    assert max(moved["rope"].values()) >= 2 * B_GRAD
    b0 = {k: v for k, v in moved["bypass"].items() if k.startswith("blocks.0.")}
    print(f"{name} defect bypass: the block-0 gradients move by {min(b0.values()):.3f} .. {max(b0.values()):.3f}")
    assert len(b0) >= 8 and min(b0.values()) >= 2 * B_GRAD, b0
    # the defects are defects of the BACKWARD only where the issue says so: "dv0" and "bypass" leave the output alone
    assert rel(RR.reference_step(name, defect="dv0")["out"], ref["out"]) == 0.0
    assert rel(RR.reference_step(name, defect="bypass")["out"], ref["out"]) == 0.0


def test_the_unrouted_reference_is_the_oracle():
    """a check of the helper alone (it imports nothing of the library, so it also passes without the feature): with
    route=None routed_forward must be oracle.dit_forward, bit for bit, or every floor above compares the wrong thing"""
    from oracle import dit_oracle as O
    cs = RR.case("hd64")
    with torch.no_grad():
        a = RR.routed_forward(cs["P"], cs["cfg"], cs["zt"].float(), cs["ctx"].float(), cs["ts"].float(), RR.START, RR.SPAN, None)
        b = O.dit_forward(cs["P"], cs["cfg"], cs["zt"].float(), cs["ctx"].float(), cs["ts"].float(), RR.START)
    assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------- the draw, the tables ----
@pytest.mark.parametrize("N,keep", [(256, 0.5), (256, 0.75), (7, 0.5), (3, 0.1), (1000, 0.333)])
def test_draw_route(N, keep):
    m = tiny().enable_token_routing(1, 2, keep)
    k = max(1, int(keep * N + 0.5))
    assert M.route_keep_count(N, keep) == k == RR.keep_count(N, keep)
    torch.manual_seed(5)
    r = m.draw_route(N)
    assert r.dtype == torch.int32 and tuple(r.shape) == (k,) and not r.is_cuda
    assert int(r.min()) >= 0 and int(r.max()) < N and bool((r[1:] > r[:-1]).all())
    torch.manual_seed(5)
    assert torch.equal(r, m.draw_route(N))
    torch.manual_seed(5)
    assert torch.equal(r.long(), torch.randperm(N)[:k].sort().values)
    if N >= 256:
        assert not torch.equal(r, m.draw_route(N))


def test_the_route_is_drawn_after_the_rope_offsets():
    m = tiny().enable_token_routing(1, 2, 0.5)
    thw = (4, 8, 8)
    torch.manual_seed(11)
    start, route = m.rope.draw_start(thw), m.draw_route(256)
    torch.manual_seed(11)
    sh = torch.randint(0, 128 - 8 + 1, (1,)).item()
    sw = torch.randint(0, 128 - 8 + 1, (1,)).item()
    st = torch.randint(0, 128 - 4 + 1, (1,)).item()
    by_hand = torch.randperm(256)[:128].sort().values
    assert start == (st, sh, sw) and torch.equal(route.long(), by_hand)


def test_draw_route_needs_the_switch():
    with pytest.raises(ValueError, match="enable_token_routing"):
        tiny().draw_route(16)


@pytest.mark.parametrize("route", [[0], [255], [0, 255], list(range(0, 256, 2)), list(range(256))])
def test_idx_and_inv_are_inverse_and_the_registers_come_first(route):
    idx, inv = M.route_tables(torch.tensor(route, dtype=torch.int32), 256)
    assert idx.dtype == inv.dtype == torch.int32 and tuple(idx.shape) == (16 + len(route),) and tuple(inv.shape) == (272,)
    assert idx[:16].tolist() == list(range(16)) and idx[16:].tolist() == [16 + r for r in route]
    assert torch.equal(inv[idx.long()], torch.arange(16 + len(route), dtype=torch.int32))
    assert int((inv >= 0).sum()) == 16 + len(route) and int(inv.min()) >= -1
    r_idx, r_inv = RR.tables(route, 256)
    assert torch.equal(idx.long(), r_idx) and torch.equal(inv.long(), r_inv)


# ------------------------------------------------------------------------------------------- argument errors ----
def test_enable_token_routing_arguments():
    m = tiny()
    assert m.token_routing is None
    assert m.enable_token_routing(1, 3, 0.25) is m and m.token_routing == (1, 3, 0.25)
    assert m.enable_token_routing(2, 2).token_routing == (2, 2, 0.5)
    assert m.enable_token_routing(None) is m and m.token_routing is None
    assert not any("rout" in k for k in m.state_dict()) and len(list(m.parameters())) == len(list(tiny().parameters()))
    for first, last in ((0, 2), (1, 4), (3, 2), (-1, 2), (4, 4)):
        with pytest.raises(ValueError, match="1 <= first_block <= last_block <= depth - 1 = 3"):
            m.enable_token_routing(first, last)
    for keep in (0.0, 1.0, -0.5, 1.5, float("nan"), "0.5", None):
        with pytest.raises(ValueError, match="0 < keep < 1"):
            m.enable_token_routing(1, 2, keep)
    for args in ((True, 2, 0.5), (1, True, 0.5), (1.0, 2, 0.5)):
        with pytest.raises(ValueError, match="must be an int"):
            m.enable_token_routing(*args)
    with pytest.raises(ValueError, match="0 < keep < 1"):
        m.enable_token_routing(1, 2, True)
    assert m.token_routing is None


def _cpu_call(m, route, **kw):
    """a call that is refused before the device is touched (the inputs are CPU tensors: anything later raises RuntimeError)"""
    return m(torch.zeros(1, 16, 4, 8, 8), torch.zeros(1, 4, 64), kw.pop("timesteps", torch.zeros(1)), route=route, **kw)


def test_route_argument():
    m = tiny().enable_token_routing(1, 2, 0.5)  # N = 2 * 4 * 4 = 32
    for bad, what in (([3, 1], "sorted and distinct"), ([1, 1, 2], "sorted and distinct"), ([0, 32], r"in \[0, 32\)"),
                      ([-1, 3], r"in \[0, 32\)"), ([], "empty"), ([0.5, 1], "ints"), ([True, 2], "ints"),
                      (torch.tensor([5, 2]), "sorted and distinct"), (torch.tensor([0.5]), "integer tensor"),
                      (torch.tensor([[1, 2]]), "integer tensor"), (7, "sequence of ints"),
                      (True, "route=True is no route")):
        with pytest.raises(ValueError, match=what):
            _cpu_call(m, bad)
    for good in ([0, 31], torch.tensor([4, 9, 30]), False, None):
        with pytest.raises(RuntimeError, match="GPU only"):  # accepted: the call gets as far as the device check
            _cpu_call(m, good)
    off = tiny()
    for route in ([1, 2], torch.tensor([1]), True):
        with pytest.raises(ValueError, match=r"enable_token_routing\(first_block, last_block, keep\) first"):
            _cpu_call(off, route)
    for route in (None, False):
        with pytest.raises(RuntimeError, match="GPU only"):
            _cpu_call(off, route)


def test_when_a_call_is_routed():
    m = tiny().enable_token_routing(1, 2, 0.5)
    assert m.training and m._route_requested(None) and m._route_requested([1]) and not m._route_requested(False)
    with torch.no_grad():
        assert not m._route_requested(None) and m._route_requested([1])
    m.eval()
    assert not m._route_requested(None) and m._route_requested([1]) and not m._route_requested(False)
    m.enable_token_routing(None)
    assert not m.train()._route_requested(None)


# ------------------------------------------------------------------------------------------------- refusals ----
def test_refused_on_a_frame_causal_model():
    for kw in (dict(frame_causal=True), dict(frame_causal=True, frame_major=True),
               dict(frame_causal=True, frame_major=True, frame_chunk=2),
               dict(frame_causal=True, frame_major=True, frame_chunk=2, frame_window=4)):
        with pytest.raises(ValueError, match="build the model without frame_causal to route it"):
            tiny(**kw).enable_token_routing(1, 2)


def test_refused_with_the_frame_band_in_both_orders():
    with pytest.raises(ValueError, match=r"call enable_frame_band\(None\) to route the model"):
        tiny().enable_frame_band(1).enable_token_routing(1, 2)
    m = tiny().enable_token_routing(1, 2)
    with pytest.raises(ValueError, match=r"enable_token_routing\(None\) to run the band"):
        m.enable_frame_band(1)
    assert m.frame_band is None and all(b.frame_band is None for b in m.blocks)
    m.enable_frame_band(None)  # switching the band OFF is no conflict
    assert m.enable_token_routing(None).enable_frame_band(1).frame_band == (1, 1)


def test_refused_with_fp8_in_both_orders():
    with pytest.raises(NotImplementedError, match=r"call enable_fp8\(False\) to route the model"):
        tiny().enable_fp8().enable_token_routing(1, 2)
    m = tiny().enable_token_routing(1, 2)
    with pytest.raises(NotImplementedError, match=r"enable_token_routing\(None\) to run it in fp8"):
        m.enable_fp8()
    assert not m.fp8
    m.enable_fp8(False)
    assert m.enable_token_routing(None).enable_fp8().fp8


def test_refused_on_a_sharded_model_in_both_orders():
    from video_diffusion_speedrun_amd import fsdp
    m = tiny()
    m._fsdp = object()  # what apply_fsdp leaves on the model
    with pytest.raises(NotImplementedError, match="route an unsharded model"):
        m.enable_token_routing(1, 2)
    m = tiny().enable_token_routing(1, 2)
    with pytest.raises(NotImplementedError, match="route an unsharded model"):
        fsdp.apply_fsdp(m)
    assert m._fsdp is None
    m._fsdp = object()  # sharded behind the switch's back: the call refuses
    with pytest.raises(NotImplementedError, match="route an unsharded model"):
        _cpu_call(m, None)


def test_calls_a_routed_model_refuses():
    m = tiny().enable_token_routing(1, 2)
    with pytest.raises(ValueError, match=r"pass timesteps \[B\], or route=False for this call"):
        _cpu_call(m, None, timesteps=torch.zeros(1, 2))
    with pytest.raises(ValueError, match="drop teacher_latents, or pass route=False"):
        _cpu_call(m, None, teacher_latents=torch.zeros(1, 16, 4, 8, 8))
    with pytest.raises(ValueError, match="pass frame_cache=None, or route=False"):
        _cpu_call(m, None, frame_cache=object())
    # route=False, eval() and no_grad run every token: these calls get past the routing checks (and fail further on,
    # for their own reasons or at the device check)
    with pytest.raises(RuntimeError, match="GPU only"):
        _cpu_call(m, False, timesteps=torch.zeros(1, 2))
    with pytest.raises(ValueError, match="frame_causal=True, frame_major=True"):
        _cpu_call(m, False, teacher_latents=torch.zeros(1, 16, 4, 8, 8))
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU only"):
        _cpu_call(m, None, timesteps=torch.zeros(1, 2))
    with pytest.raises(RuntimeError, match="GPU only"):
        _cpu_call(m.eval(), None, timesteps=torch.zeros(1, 2))


# --------------------------------------------------------------------------------------------- the C entries ----
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_host_side_refusals_of_the_row_movers(lib):
    """nothing is launched: every call below returns before its launch (the pointers are never dereferenced)"""
    A, Bp, Cp, T = 0x10000, 0x20000, 0x30000, 0x40000  # 16-byte aligned "pointers"
    ARG, UNSUPPORTED = -1, -2
    g, mg, sa = lib.vds_rows_gather, lib.vds_rows_merge, lib.vds_rows_scatter_add_f32
    for args in ((None, Bp, T, 1, 9, 4, 144), (A, None, T, 1, 9, 4, 144), (A, Bp, None, 1, 9, 4, 144),  # NULL
                 (A + 8, Bp, T, 1, 9, 4, 144), (A, Bp + 4, T, 1, 9, 4, 144), (A, Bp, T + 2, 1, 9, 4, 144),  # misaligned
                 (A, Bp, T, 1, 9, 4, 8), (A, Bp, T, 1, 9, 4, 24), (A, Bp, T, 1, 9, 4, 0), (A, Bp, T, 1, 9, 4, -16),
                 (A, Bp, T, 0, 9, 4, 144), (A, Bp, T, -1, 9, 4, 144), (A, Bp, T, 1, 0, 4, 144), (A, Bp, T, 1, -9, 4, 144),
                 (A, Bp, T, 1, 9, -1, 144)):
        assert g(*args, None) == ARG, args
        assert lib.vds_last_error().startswith(b"vds_rows_gather: ")
    assert g(A, Bp, T, 1, 9, 0, 144, None) == 0
    assert g(A, Bp, T, 1, 1, 2 ** 31 - 1, 2 ** 31 - 16, None) == UNSUPPORTED  # 2^58 pieces: no grid holds them
    assert g(A, Bp, T, 1, 1, 1, 2 ** 31, None) == UNSUPPORTED
    for args in ((None, Bp, Cp, T, 1, 9, 4, 144), (A, None, Cp, T, 1, 9, 4, 144), (A, Bp, None, T, 1, 9, 4, 144),
                 (A, Bp, Cp, None, 1, 9, 4, 144), (A + 8, Bp, Cp, T, 1, 9, 4, 144), (A, Bp + 8, Cp, T, 1, 9, 4, 144),
                 (A, Bp, Cp + 8, T, 1, 9, 4, 144), (A, Bp, Cp, T + 1, 1, 9, 4, 144), (A, Bp, Cp, T, 1, 9, 4, 8),
                 (A, Bp, Cp, T, 0, 9, 4, 144), (A, Bp, Cp, T, 1, 0, 4, 144), (A, Bp, Cp, T, 1, -3, 4, 144),
                 (A, Bp, Cp, T, 1, 9, -4, 144)):
        assert mg(*args, None) == ARG, args
        assert lib.vds_last_error().startswith(b"vds_rows_merge: ")
    assert mg(A, Bp, A, T, 1, 9, 0, 144, None) == 0 and mg(A, Bp, Cp, T, 1, 9, 0, 144, None) == 0
    assert mg(A, Bp, Cp, T, 1, 2 ** 31 - 1, 4, 2 ** 31 - 16, None) == UNSUPPORTED
    for args in ((None, Bp, T, 1, 9, 4, 36), (A, None, T, 1, 9, 4, 36), (A, Bp, None, 1, 9, 4, 36),
                 (A + 4, Bp, T, 1, 9, 4, 36), (A, Bp + 8, T, 1, 9, 4, 36), (A, Bp, T + 2, 1, 9, 4, 36),
                 (A, Bp, T, 1, 9, 4, 2), (A, Bp, T, 1, 9, 4, 6), (A, Bp, T, 1, 9, 4, 0), (A, Bp, T, 1, 9, 4, -4),
                 (A, Bp, T, 0, 9, 4, 36), (A, Bp, T, 1, 0, 4, 36), (A, Bp, T, 1, 9, -4, 36)):
        assert sa(*args, None) == ARG, args
        assert lib.vds_last_error().startswith(b"vds_rows_scatter_add_f32: ")
    assert sa(A, Bp, T, 1, 9, 0, 36, None) == 0
    assert sa(A, Bp, T, 1, 9, 2 ** 31 - 1, 2 ** 29, None) == UNSUPPORTED


# ----------------------------------------------------------------------------------------- activation_bytes ----
@pytest.mark.parametrize("mode", ["none", "full", "selective"])
def test_activation_bytes_sums_the_blocks_at_their_lengths(mode):
    m = tiny(depth=6, qk_norm="all")
    B, shape, Lc = 3, (8, 16, 16), 24
    plain = M.activation_bytes(m, B, shape, Lc, mode)
    assert M.activation_bytes(m, B, shape, Lc, mode, routing=None) == plain
    N = 4 * 8 * 8
    for first, last, keep in ((1, 4, 0.5), (2, 2, 0.75), (1, 5, 0.25)):
        got = M.activation_bytes(m, B, shape, Lc, mode, routing=(first, last, keep))
        k = max(1, int(keep * N + 0.5))
        # the per-block figure at Ls rows is what a model whose whole video is k tokens keeps per block
        short = M.activation_bytes(m, B, (2, 2, 2 * k), Lc, mode)
        assert short["rows"] == B * (16 + k) == got["rows_routed"] and got["per_block_routed"] == short["per_block"]
        n = last - first + 1
        assert got["kept"] == (6 - n) * plain["per_block"] + n * short["per_block"] < plain["kept"]
        assert {k_: got[k_] for k_ in plain if k_ != "kept"} == {k_: plain[k_] for k_ in plain if k_ != "kept"}
    with pytest.raises(ValueError, match="1 <= first_block"):
        M.activation_bytes(m, B, shape, Lc, mode, routing=(0, 2, 0.5))
