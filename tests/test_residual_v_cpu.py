"""Detection power of the residual-V tests with distinct per-block lambdas, computed from the references alone (no GPU):
a pairing of the wrong lambda with a block's dv must land far outside what the GPU tests tolerate, or those tests could
pass on it (tests/test_kernels_gpu.py::test_dv0_reduce_matches_float64_reference_with_distinct_lambdas,
tests/test_workloads_gpu.py::test_deep_residual_v_*)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import residual_v_cases as RV  # noqa: E402

GRAD_REL = RV.GRAD_REL


@pytest.mark.parametrize("hd,hdp", RV.DV0_HEADS)
@pytest.mark.parametrize("n", [n for n in RV.DV0_N if n > 1])
def test_dv0_bound_rejects_a_rotated_pairing_and_admits_fp32_summation(n, hd, hdp):
    """the float64 reference with the lambdas rotated by one position violates the fp32 bound at more than half of the
    elements (measured: at every element for n = 10, hd = 72), while a plain fp32 evaluation of the right pairing, term
    by term in either order the model uses, stays inside it: the bound separates a wrong kernel from a right one"""
    dvs, lams = RV.dv0_inputs(n, hd, hdp)
    want, scale = RV.dv0_reference(dvs, lams, hd)
    bound = RV.dv0_bound(n, scale)
    assert torch.isfinite(want).all() and float(bound.min()) > 0
    wrong, _ = RV.dv0_reference(dvs, RV.dv0_rotated(lams), hd)
    frac = ((wrong - want).abs() > bound).double().mean().item()
    print(f"n={n} hd={hd}: rotated pairing violates the bound at {100 * frac:.1f} % of the elements")
    assert frac > 0.5
    for order in (list(range(n)), [i for c in RV.dv0_chunks(n) for i in c]):
        acc = torch.zeros_like(want, dtype=torch.float32)
        for i in order:
            acc = acc + (1.0 - lams[i].float()) * dvs[i][..., :hd].float()
        assert bool(((acc.double() - want).abs() <= bound).all())


def test_dv0_chunks_walk_the_list_from_its_end():
    assert RV.dv0_chunks(1) == [[0]]
    assert RV.dv0_chunks(9) == [list(range(8, -1, -1))]
    assert RV.dv0_chunks(10) == [list(range(9, 0, -1)), [0]]
    assert [len(c) for c in RV.dv0_chunks(40)] == [9, 9, 9, 9, 4] and RV.dv0_chunks(40)[0][0] == 39


@pytest.mark.parametrize("key", sorted(RV.DEEP_HIDDEN))
def test_deep_case_fan_in_moves_under_a_stale_pairing(key):
    """depth 12, lambdas 0.27 ... 0.97: the gradient that reaches v_0 with each block's term weighted by the lambda of the
    block 1, 3 or 4 positions on (3 and 4: the buffer counts of the reshard runtime's ring) differs from the right one by
    more than 5 x GRAD_REL in relative L2, in the fan-in and in block 0's total dv -- the oracle comparison of the GPU
    tests cannot pass on such a pairing inside its tolerance"""
    cfg, P, x, ctx, t, v = RV.deep_case(key)
    (_, loss, grads, _), dv = RV.oracle_step_with_dv(cfg, P, x, ctx, t, v, RV.DEEP_ROPE_START)
    right = RV.fan_in(P, dv)
    own = dv[0].double() - right  # what block 0's own attention sends to its v
    assert loss > 0 and all(float(grads[f"blocks.{i}.lambda_param"].abs()) > 0 for i in range(1, cfg.depth))
    for shift in (1, 3, 4):
        wrong = RV.fan_in(P, dv, shift)
        e_fan, e_tot = RV.rel_l2(wrong, right), RV.rel_l2(own + wrong, dv[0])
        print(f"{key}: pairing rotated by {shift}: fan-in moves by {e_fan:.3f}, block 0's dv by {e_tot:.3f}")
        assert e_fan > 5 * GRAD_REL and e_tot > 5 * GRAD_REL
