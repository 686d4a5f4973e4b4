"""The optimizer census without a GPU: every builder's own exactness checks hold, the case lists reach every edge (by the
loops and dispatch predicates restated in tests/helpers/optim_census.py) and every cap holds for the reference alone.
Prints the edge -> cases tables (run with -s)."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import optim_census as C  # noqa: E402

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64


def show(title, cov):
    print(f"\n{title}")
    for name, cases in cov.items():
        shown = ", ".join(str(s) for s in cases[:4]) + (f", ... ({len(cases)})" if len(cases) > 4 else "")
        print(f"  {name:<52} {shown}")
    empty = [name for name, cases in cov.items() if not cases]
    assert not empty, f"no case reaches: {empty}"


# ---- AdamW -------------------------------------------------------------------------------------------------------------
def test_adamw_loops_restated():
    """the restated loops touch every element once, and give the trips and tails the issue names"""
    for extent in C.EXTENTS[:-1] + (8191, 8192, 8193):
        for unroll in (2, 4):
            for ok in (True, False):
                assert set(C.walk(extent, ok, unroll)[0]) == {1}
    trips = lambda n, u=2: sorted(set(C.walk(n, True, u)[1]))   # noqa: E731
    assert trips(1025) == [0] and trips(2044) == [0, 1] and trips(2047) == [0, 1] and trips(2048) == [1]
    assert trips(3076) == [1, 2] and trips(4096) == [2] and trips(4097) == [2] and trips(65541) == [32]
    assert trips(4095, 4) == [0, 1] and trips(4096, 4) == [1] and trips(8192, 4) == [2]
    assert sorted(set(C.walk(2047, True, 2)[2])) == [3, 4] and sorted(set(C.walk(4097, True, 2)[2])) == [1]
    assert set(C.walk(1, True, 2)[2]) == {1} and set(C.walk(3, False, 2)[2]) == {3} and set(C.walk(5, True, 2)[2]) == {1, 4}
    # the rule of include/vds.h: every stream decides
    assert C.vec_rule([0, 0, 0, 0], 0, 0) and not C.vec_rule([0, 4, 0, 0], 0, 0) and not C.vec_rule([0, 0, 0, 0], 0, 2)
    assert not C.vec_rule([0, 0, 0, 0], 1030, 0) and C.vec_rule([0, 0, 0, 0], 2060, 0) and C.vec_rule([0, 0, 0, 0, 0], 4, None)


def test_adamw_exact_recipe():
    """every intermediate of the chain is an fp32 number for every tensor of every case (the builder asserts it step by
    step); the shadow's rounding is exercised and p' takes enough values for a misplaced element to show"""
    big = None
    for case in C.adamw_cases():
        assert set(C.CHUNK_ELEMS) >= {case.chunk_elems}
        pairs = {(t.lr, t.wd) for t in case.tensors}
        assert len(pairs) == len(case.tensors), f"{case.name}: descriptors share an (lr, wd)"
        for i, t in enumerate(case.tensors):
            e = C.adamw_expect(case, i)
            assert (e.g != 0).all() and float(e.p0.abs().max()) <= 4.0
            if t.numel == 65541:
                big = e
    assert {c.chunk_elems for c in C.adamw_cases()} == set(C.CHUNK_ELEMS)
    assert big.distinct > 60000 and big.inexact_bf16 > 0.96, (big.distinct, big.inexact_bf16)
    print(f"\n65541 elements: {big.distinct} distinct p', {big.inexact_bf16:.2%} of them inexact in bf16")


def test_adamw_coverage():
    show("adamw: edge -> cases", C.adamw_coverage())


def test_adamw_real_constants_margin():
    """the derived bound leaves room: the smallest update is more than 4 bounds (asserted by the builder)"""
    for step in C.REAL_STEPS:
        for i, n in enumerate(C.REAL_NUMELS):
            r = C.adamw_real(n, step, 1e-3 * (i + 1), 0.1 / (i + 1), 0.7, 1.0, 0.5, 0.99, i)
            assert r.margin > 1.0 and float((r.bp / r.sp).max()) < 1e-6
    assert C.host_scalars(0.5, 0.75, 1) == (0.5, 2.0)


# ---- sum of squares, finalize ----------------------------------------------------------------------------------------------
def test_sumsq_cases():
    for case in C.sumsq_cases():
        gs, ct, cs, parts, total = C.sumsq_expect(case.name)
        assert float(total) == sum(float((g.double() ** 2).sum()) for g in gs)
    assert C.sumsq_stage2_trips(256) == 1 and C.sumsq_stage2_trips(257) == 2
    show("sumsq: edge -> cases", C.sumsq_coverage())


def test_finalize_restated():
    tab = C.finalize_table()
    assert len(tab) == 8 * 3 * 8 * 2
    inf, nan = float("inf"), float("nan")
    assert C.finalize_expect(0.0, 1.0, 1.0, 1) == (0.0, 1.0, 0)
    assert C.finalize_expect(16.0, 1.0, 1.0, 0)[:2] == (4.0, C.f32v(C.f32v(1.0) / C.f32v(4.0 + 1e-6)))
    assert C.finalize_expect(inf, 1.0, inf, 0) == (inf, 1.0, 0) and C.finalize_expect(3e38, 2.0, 1.0, 1)[2] == 1
    n, c, s = C.finalize_expect(nan, 1.0, 1.0, 0)          # a NaN norm with skipping off leaves a NaN coefficient
    assert n != n and c != c and s == 0
    n, c, s = C.finalize_expect(nan, 1.0, 0.0, 1)          # clipping off: the coefficient is 1, the step is skipped
    assert n != n and c == 1.0 and s == 1
    assert C.finalize_expect(1.0, 1.0, nan, 1) == (1.0, 1.0, 0)
    assert sum(C.finalize_expect(*row)[2] for row in tab) > 0


# ---- Muon ----------------------------------------------------------------------------------------------------------------
def test_momentum_cases():
    seen = set()
    for plan in C.mom_plan():
        c = C.momentum_case(*plan)
        nmat, rows, cols = plan[:3]
        assert c.x0.shape == (nmat, min(rows, cols), max(rows, cols))
        seen.add((rows > cols, rows % 64 != 0, cols % 64 != 0, plan[5]))
    assert {(True, True, False, 1), (False, False, True, 0), (False, True, True, 1), (True, True, True, 0)} <= seen, seen


def test_normalize_cases():
    grids = [C.normalize_grid(r * c) for _, r, c in C.NORM_SHAPES]
    assert grids[0] == (1, 1) and grids[-1] == (1024, 2) and 1024 * 2056 > 2097152
    for shape in C.NORM_SHAPES[:-1]:
        C.normalize_case(*shape)
    assert float(C.inv_norm(torch.tensor(16.0, dtype=f32))) == 0.25


def test_newton_schulz_recipes():
    """both recipes at the shapes of the issue and of the GPU test: every A exact in bf16 (asserted by the chain), the
    excluded shares under the caps; dense: the third product does not fit and is not capped"""
    assert {C.tri_tiles(m) for m, _ in C.NS_SHAPES} == {1, 3, 6}
    assert {C.k_tail(n) for _, n in C.NS_SHAPES} >= {0, 8, 40} and {C.k_tail(m) for m, _ in C.NS_SHAPES} >= {0, 8, 40}
    assert any(m % 128 and C.tri_tiles(m) > 1 for m, _ in C.NS_SHAPES)           # mirrored tiles with a ragged edge
    assert any(m % 64 for m, _ in C.NS_SHAPES)                                    # k-major rows past K: the next matrix
    print()
    for recipe in ("dense", "sparse"):
        for m, n in sorted(set(C.NS_CPU_SHAPES + C.NS_SHAPES)):
            sa, sb, sx = C.ns_chain(recipe, 3, m, n)[4]
            print(f"  {recipe:<7} [{m}, {n}]: excluded A {sa:.3%} B {sb:.3%} X' {sx:.3%}")
            assert sa == 0.0 and sb <= (0.001 if recipe == "dense" else 0.0) and (recipe == "dense" or sx == 0.0), (recipe, m, n)
            assert max(sa, sb) <= C.UNDECIDED_CAP
    for m, n in ((136, 136), (128, 520), (200, 328)):
        X = (C.ns_u("signed_permutation", 3, m, n).to(f64) / 4.0).to(bf16)
        X2 = C.ns_forward(X, 3)
        assert not torch.equal(X2, X)


def test_update_cases():
    for scalars in C.UPD_SCALARS:
        for rows, cols in C.UPD_EXACT:
            e = C.update_case(3, rows, cols, scalars)
            assert torch.equal(e.p, e.p_alt) and e.scale in (1.0, 2.0)
        e = C.update_case(3, *C.UPD_INEXACT, scalars)
        assert e.scale not in (1.0, 2.0) and not torch.equal(e.p, e.p_alt)
    assert C.muon_scale(512, 128) == 2.0 and C.muon_scale(128, 520) == 1.0


def test_workspace_layout():
    off, total = C.muon_layout(3, 200, 328)
    assert total % 256 == 0 and all(o % 256 == 0 for o, _ in off.values())
    assert off["x1"][0] >= off["x0"][1] and off["partials"][0] >= off["sumsq"][0] + 12
    assert any(o % 256 == 0 and n % 256 for o, n in off.values())       # padding gaps exist to be poisoned
