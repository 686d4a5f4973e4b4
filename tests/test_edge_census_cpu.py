"""The step-edge census without a GPU: the shape lists reach every branch (by the dispatch predicates restated in
tests/helpers/edge_census.py), every builder's own exactness checks hold, and every cap holds for the reference alone.
Prints, per predicate, the branch -> shapes table of the docstring of test_edge_census_gpu.py (run with -s)."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import edge_census as E  # noqa: E402
import gemm_census as G  # noqa: E402
import row_census as R  # noqa: E402

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64


def show(title, cov):
    print(f"\n{title}")
    for name, shapes in cov.items():
        shown = ", ".join(str(s) for s in shapes[:6]) + (f", ... ({len(shapes)})" if len(shapes) > 6 else "")
        print(f"  {name:<62} {shown}")
    empty = [name for name, shapes in cov.items() if not shapes]
    assert not empty, f"no case reaches: {empty}"


# ---- small linears -------------------------------------------------------------------------------------------------------
def test_linear_predicates():
    """the figures the issue names, from the restated predicates"""
    assert E.mfma_rule(16, 1024, 1696) and not E.mfma_rule(16, 1024, 1728)          # the largest K that fits in LDS
    assert not E.mfma_rule(17, 1024, 192) and not E.mfma_rule(4, 1008, 192) and not E.mfma_rule(4, 1032, 192)
    assert not E.mfma_rule(4, 1024, 200) and not E.mfma_rule(4, 1024, 192, knob=0)
    assert E.mfma_shape(1024, 192) == (8, 8, 1, 0) and E.mfma_shape(1040, 192)[:2] == (9, 1)
    assert [E.mfma_shape(1024, K)[2:] for K in E.MFMA_K] == [(0, 1), (0, 5), (1, 0), (1, 1), (2, 1), (8, 5)]
    assert [E.fwd_instance(m) for m in E.MS] == [4, 4, 8, 8, 16, 16]
    assert E.chunks(17) == [16, 1] and E.chunks(33) == [16, 16, 1] and E.chunks(16) == [16]
    assert [E.row_trips(K) for K in E.ROW_K] == [(1, 0, 1), (63, 0, 63), (64, 1, 0), (65, 1, 1)]
    assert E.dx_split(1600, 8192) == (128, 4, 416, 2)                               # per-set slice loop
    assert E.dx_split(800, 4096, 16) == (64, 2, 416, 2)                             # batched, 16 pointers
    assert E.dx_split(9 * 1152, 1152, 28)[1] == 5                                   # the batched workload: ny 5 ...
    assert E.dx_split(9 * 1152, 1152, 28)[2] > E.SL_DX_ROWS                         # ... of more than one slice
    assert [E.dx_split(N, 72)[1] for N in E.DX_N] == [1, 2, 3]
    assert E.dw_tile_grid(68, 136, 3) == (2, 2, 3) and E.dw_tile_grid(64, 128, 1) == (1, 1, 1)
    assert E.dx_workspace_floats(5, 1600, 8192) == 4 * 16 * 8192 and E.dx_workspace_floats(5, 800, 4096, 16) == 16 * 2 * 5 * 4096


def test_linear_coverage():
    show("small linears: branch -> (M, N, K[, nb])", E.linear_coverage())


def test_linear_cases_are_exact():
    """every builder asserts its own 24-bit fits; the MFMA split of x has two nonzero terms everywhere and three where K
    leaves room for a granule of 2^-18"""
    terms = {}
    for M, N, K, with_bias in E.fwd_plan():
        c = E.linear_case(M, N, K, 1, with_bias)
        R.assert_no_sentinel("y", c.y)
        if E.mfma_rule(min(M, 16), N, K):
            terms[(M, N, K)] = c.terms3
    assert min(terms.values()) >= 2 and max(terms.values()) == 3, terms
    print("\nnonzero bf16 terms of x in the MFMA cases:", {k: v for k, v in terms.items() if v == 3}, "three; the others two")
    for M, N, K, _ in E.dw_plan():
        c = E.linear_case(M, N, K, 1, True)
        R.assert_no_sentinel("dW", c.dW)
    for M, N, K in E.dx_plan():
        c = E.linear_case(M, N, K)
        assert (c.dx0 != 0).all() and not torch.equal(c.dx, c.dx0)
    for M, N, K, nb, _ in E.tile_plan():
        E.linear_case(M, N, K, nb, True, nb)
    for M, N, K, nb, with_bias in E.BATCHED_FWD:
        E.linear_case(M, N, K, nb, with_bias, nb)
    for M, N, K, nb in E.BATCHED_DX:
        E.linear_case(M, N, K, max(1, nb - 1), True, nb)


def test_linear_slice_cases_are_exact():
    M, N, K = E.DX_BIG
    c = E.linear_case(M, N, K, 1, True, None, False)
    # consuming only the first LDS slice of every row range changes the answer (what mutant 3 of the issue does)
    rows = E.dx_split(N, K)[2]
    first = sum(c.dy[0][:, r0:r0 + E.SL_DX_ROWS].to(f64) @ c.W[0][r0:r0 + E.SL_DX_ROWS].to(f64) for r0 in range(0, N, rows))
    assert (c.dx0.to(f64) + first != c.dx.to(f64)).float().mean() > 0.9
    M, N, K, nb = E.DX_BIG_BATCHED
    c = E.linear_case(M, N, K, 2, True, nb, False)
    assert not torch.equal(c.W[0], c.W[1])


def test_silu_cases_hold_their_margin():
    """at most 8 nonzero x per row and column on the loop edges; smallest addend > 4 x bound for every element (asserted
    by the builder), bound / sum|terms| below 1e-5"""
    print()
    for M, N, K, with_bias in E.ACT_FWD:
        c = E.act_case(M, N, K, with_bias)
        print(f"  act_in 1 fwd {(M, N, K)}: smallest addend / (4 x bound) = {c.margin:.0f}, columns {sorted(set((c.x != 0).nonzero()[:, 1].tolist()))[:12]}")
        assert c.margin > 1
    for M, N, K in E.ACT_BWD:
        c = E.act_case(M, N, K, True)
        assert c.margin > 1 and E.dx_split(N, K)[1] >= 1
        assert float(c.dx_bound.max()) < 1e-3
    for M, N, K, nb in E.ACT_BATCHED:
        assert E.act_case(M, N, K, True, nb).margin > 1
    for M, N, K, _ in E.ACT_FWD:     # every case here has the slots for every edge: each one holds a nonzero x
        used = set((E.act_case(M, N, K, _).x != 0).any(0).nonzero().flatten().tolist())
        assert 8 * M < len(E.edge_columns(K)) or used == set(E.edge_columns(K)), (M, N, K)
        assert {0, K - 1} <= used
    big = E.act_case(16, 1024, 1696, False).x
    assert (big[:, 1152:] != 0).any() and (big[:, 1536:] != 0).any()      # the last unrolled trips and the 5-step tail
    cols = E.edge_columns(416)
    for c_ in (0, 415, 7, 8, 31, 32, 191, 192, 383, 384, 407, 408):
        assert c_ in cols, c_
    assert all(any(t <= c_ < t + 128 for c_ in cols) for t in range(0, 416, 128))
    # the reference against itself: float64 SiLU rounded to fp32 is far inside the bound
    c = E.act_case(*E.ACT_FWD[0][:3], E.ACT_FWD[0][3])
    assert E.within("reference", c.y[0].to(f32), c.y[0], c.y_bound[0], c.y_sum[0]) <= 1.0


# ---- flow loss -----------------------------------------------------------------------------------------------------------
def test_loss_coverage():
    show("flow loss: branch -> per | (B, per) | (B, C, T, HW, tps) | n", E.loss_coverage())
    assert [E.flow_loss_bps(p) for p in E.LOSS_PER] == [1, 1, 2, 64, 65, 256, 256]
    assert E.flow_loss_bps(210) == 1 and E.flow_loss_bps(4352) == 2 and E.flow_loss_bps(264192) == 65
    assert E.loss_bwd_blocks(8 * 256 * 2048) == (2048, 1) and E.loss_bwd_blocks(8 * (256 * 2048 + 3)) == (2048, 2)


def test_loss_cases():
    """the builders assert the 24-bit fit and the distinct sums; the reference's undecided share of dout is far inside
    the 1% cap (the six values d k of a sample are decided or not as a class: the share is 0 at every case here)"""
    for B, per in E.loss_plan():
        c = E.loss_case(B, per, 0.75 if per % 2 else 1.0)
        assert (c.v.float() != c.out.float()).all()
        share = float(c.und.float().mean())
        assert share <= E.UNDECIDED_CAP / 10, (B, per, share)
        E.check_dout("reference", c.dout, c.dout, c.und)
        E.check_per_sample("reference", c.per_sample.to(f32), c.per_sample, c.per_exact)
        assert all(c.per_exact) == (per & (per - 1) == 0)
    # stage 2 stepping 128 lanes instead of 64 drops the partials 64 .. 127 (and 192 .. 255): the sum changes wherever
    # a sample has more than 64 workgroups
    for per in E.LOSS_PER:
        c = E.loss_case(1, per, 0.75 if per % 2 else 1.0)
        d = c.out.to(f64) - c.v.to(f64)
        parts = E.loss_partials((d * d)[0], per)
        assert parts.numel() == E.flow_loss_bps(per) and parts.sum() == c.sse[0]
        kept = parts.reshape(-1)[[j for j in range(parts.numel()) if (j // 64) % 2 == 0]].sum()
        assert (kept != c.sse[0]) == (E.flow_loss_bps(per) > 64), per


def test_frame_loss_cases():
    seen_w = set()
    for B, C, T, HW, tps in E.frames_plan():
        c = E.frame_loss_case(B, C, T, HW, tps, 0.75)
        share = float(c.und.float().mean())
        assert share <= E.UNDECIDED_CAP / 10, (B, C, T, HW, tps, share)
        seen_w |= set(c.w.flatten().tolist())
        if B > 1:
            assert c.w[1].sum() == 0 and c.per_sample[1] == 0 and (G.bits(c.dout[1]) == 0).all()   # a weightless sample
        if c.F > 1:
            assert c.w[0, c.F - 1] == 0 and c.w[0].sum() > 0                                       # a weightless frame
    assert seen_w == set(E.WEIGHTS)


def test_loss_bwd_cases():
    for n in E.LOSS_BWD_N:
        c = E.loss_bwd_case(n)
        share = float(c.und.float().mean())
        assert share <= E.UNDECIDED_CAP / 10 and (share == 0 or n & (n - 1))
        assert c.B * c.per == n


# ---- the movers ----------------------------------------------------------------------------------------------------------
def test_patch_cases():
    show("patches: branch -> (B, C, T, H, W, pt, p)", E.patch_coverage())
    plan = E.patch_plan()
    assert {s[5:] for s in plan} == set(E.PATCH_P) and {s[1] for s in plan} == set(E.PATCH_C) and {s[0] for s in plan} == {1, 3}
    for s in plan:
        fwd, inv = E.patch_case(*s)
        for t in (fwd.latent, fwd.tokens, inv.latent, inv.tokens):
            assert len(set(G.bits(t).flatten().tolist())) == t.numel()       # the values tell every element apart
        # the two permutations invert each other only through their own oracle: check the oracle's round trip
        assert torch.equal(G.bits(E.O.patchify(fwd.latent, s[5], s[6])), G.bits(fwd.tokens))
        parent = E.rows_parent(fwd.tokens, 16, "sentinel")
        assert (G.bits(parent[:, :16]) == G.SENTINEL_BF16).all() and torch.equal(G.bits(parent[:, 16:]), G.bits(fwd.tokens))


def test_register_cases():
    for B in E.REG_B:
        for R_, D in E.REG_RD:
            strides = E.reg_strides(R_, D)
            assert strides[0] == R_ * D and all(s > R_ * D for s in strides[1:])
            for bs in strides:
                c = E.reg_case(B, R_, D, bs)
                assert (c.dreg0 != 0).all() and (G.bits(c.want_x[:, R_ * D:]) == G.SENTINEL_BF16).all()
                assert torch.isnan(c.dx[:, R_ * D:].float()).all()


def test_noise_euler_cast_rope_cases():
    assert 0.0 in E.NOISE_T and 1.0 in E.NOISE_T
    assert any(float(torch.tensor(t, dtype=f32).to(bf16)) != float(torch.tensor(t, dtype=f32)) for t in E.NOISE_T)
    used_t = set()
    for B, per in E.NOISE:
        x, n, t, zt, v = E.noise_case(B, per)
        zero, one = t == 0, t == 1
        assert torch.equal(zt[zero], x[zero]) and torch.equal(zt[one], n[one])       # t = 0 / 1 return x / the noise
        used_t |= set(t.tolist())
    # the t the plain entry is given: 0, 1 and fp32 numbers that are no bf16 numbers
    assert 0.0 in used_t and 1.0 in used_t
    assert any(float(torch.tensor(v_, dtype=f32).to(bf16)) != v_ for v_ in used_t)
    assert (3, 100) in E.NOISE and 100 % 256 and any(per == 4097 for _, per in E.NOISE)
    for s in E.NOISE_FRAMES:
        x, n, t, zt, v = E.noise_frames_case(*s)
        assert t.shape == (s[0], s[2] // s[4])
    for n in E.EULER_N:
        for i, cfg in enumerate(E.EULER_CFG):
            for guided in (0, 1):
                cond, unc, acc0, acc1, lat = E.euler_case(n, cfg, E.EULER_DT[i], guided)
                assert (unc is None) == (not guided) and not torch.equal(acc0, acc1)
    assert [n // 8 - 256 for n in E.EULER_N[1:]] == [-1, 0, 1]
    for n in E.CAST_N:
        for off in (0, 1, 4):
            src = E.cast_values(n, off)
            E.assert_cast("reference", src.to(bf16), src)
    big = E.cast_values(2049)
    b = G.bits(big).tolist()
    for pattern in (0x3F808000, 0x3F818000, 0x00000000, -0x80000000, 0x00000001, 0x7F800000, -0x00800000, 0x7F7FFFFF):
        assert pattern in b, hex(pattern)
    assert torch.isnan(big).any() and torch.isinf(big.to(bf16)).sum() > torch.isinf(big).sum()   # values that round to inf
    assert E.all_bf16().numel() == 65536 and len(set(G.bits(E.all_bf16()).tolist())) == 65536
    for nt, ns in E.ROPE_TABS:
        tabs = E.rope_tables(nt, ns)
        for thw in E.ROPE_THW:
            for start in E.rope_starts(thw):
                assert E.rope_clamp(start, thw) == start
                cos, sin = E.rope_expect(tabs, thw, start, 16)
                assert cos.shape == (16 + thw[0] * thw[1] * thw[2], nt + 2 * ns)
                assert (cos[:16] == 1).all() and (sin[:16] == 0).all()
                # what mutant 5 of the issue does (the h offset on the w axis) changes the rows wherever they differ
                if start[1] != start[2] and start[1] + thw[2] <= 128:
                    wrong = E.rope_expect(tabs, thw, (start[0], start[1], start[1]), 16)[0]
                    assert not torch.equal(wrong, cos)
            c = E.rope_clamp(E.ROPE_BAD_START, thw)
            assert c == (0, 128 - thw[1], min(127, 128 - thw[2])) and c != E.ROPE_BAD_START


# ---- timestep embedding --------------------------------------------------------------------------------------------------
def test_timestep_embedding_cases():
    print()
    for D in E.TEMB_D:
        shares = []
        for B in E.TEMB_B:
            t, want, und = E.temb_case(B, D)
            assert want.shape == (B, D) and torch.equal(want.to(bf16).to(f32), want)
            if B > 1:
                assert t[0] == 0 and t[1] == 1 and t[2] == 2.0 ** -10 and ((t[3:] > 0) & (t[3:] < 1)).all()
            if B == 61:
                assert t.numel() == 61 and len(set(t.tolist())) == 61
            share = float(und.float().mean())
            assert share <= E.UNDECIDED_CAP, (B, D, share)
            shares.append(share)
            # absolute moves would leave the tiny sines undecided; the relative ones decide them
            half = D // 2
            tiny = (want[:, half:].abs() < 1e-3) & (want[:, half:] != 0)
            assert not und[:, half:][tiny].all() or not tiny.any()
        print(f"  timestep embedding D {D}: undecided share of the reference {min(shares):.3%} .. {max(shares):.3%}")
