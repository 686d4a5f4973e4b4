"""The softmax census (tests/helpers/softmax_census.py) without a GPU: its conditions hold on every case the GPU module
runs (the underflow threshold per head dim, the |dP - delta| floor, bounds of the plain path within 2^-6 A), the closed
forms of the hard recipes agree with the float64 expectation, the torch emulation of the kernels (attn_census.emulate,
tiled by 32-key sub-blocks with the lazy threshold) stays inside every bound under every evaluation order a kernel can
take, the injected faults leave it, and the instance -> case table of tests/test_softmax_census_gpu.py is complete."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_census as AC  # noqa: E402
import frame_band_ref as FB  # noqa: E402
import frame_chunk_ref as FCH  # noqa: E402
import frame_major_ref as FM  # noqa: E402
import frame_window_ref as FW  # noqa: E402
import softmax_census as SC  # noqa: E402
import teacher_ref as TR  # noqa: E402
from test_attn_census_cpu import TOL_G, TOL_LSE, TOL_O, _random_causal, f64_reference, rel  # noqa: E402

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16
HEAD_DIMS = [32, 64, 72, 96, 128]
CROSS_SHAPES = [(130, 257), (200, 100), (130, 33), (200, 64), (130, 192)]  # (Lq, Lk)
SELF_LENGTHS = [130, 200]
B_H = (3, 2)  # B * H = 6: the five ladder patterns, one twice

# masked family -> (mask [B, Lq, Lk] in the rows the kernels use, the shape its runner takes).  window_lead0: no lead rows,
# so the first sub-blocks a late query's workgroup visits lie wholly before its window (m = -1e30, l = 0 until it opens)
KV_LENS = [33, 100, 300, 64, 1, 192]


def by_frame(L, lead, period, waves):
    """g(q) for token-major frame masks: the frame (lead rows with frame 0), split further by wave -- up to 16 groups"""
    q = torch.arange(L)
    return (((q - lead) % period) * (q >= lead)) * waves + (q // 32) % waves


MASKED = {
    "kvlen": (lambda: AC.kvlen_mask(130, 257, KV_LENS), KV_LENS),
    "causal": (lambda: AC.causal_mask(2, 200, 16, 8), (200, 16, 8), by_frame(200, 16, 8, 2)),
    "past": (lambda: AC.past_mask(2, 130, 16, 2, 48), (16, 2, 48), by_frame(130, 16, 2, 4)),
    "fm": (lambda: FM.census_mask(2, 200, 16, 8), (200, 16, 8)),
    "chunk": (lambda: FCH.census_mask(2, 200, 16, 8, 2), (200, 16, 8, 2)),
    "window": (lambda: FW.census_mask(2, 200, 16, 8, 1, 2), (200, 16, 8, 1, 2)),
    "window_lead0": (lambda: FW.census_mask(2, 200, 0, 8, 1, 2), (200, 0, 8, 1, 2)),
    "teacher": (lambda: TR.census_mask(2, *TR.SHAPES[0]), TR.SHAPES[0]),
    "band": (lambda: FB.census_mask(2, 200, 16, 8, 1, 1), (200, 16, 8, 1, 1)),
}
# the evaluation orders: forward (emulate_fwd_tiled keywords; None: the dense softmax), is it the ones path, backward route
ORDERS = {
    "dense": (None, False, False),
    "wave32": (dict(rows=32), False, False),  # attn_fwd_kernel
    "wave64": (dict(rows=64), False, False),  # the 64-queries-per-wave forwards
    "own": (dict(own=True), False, False),  # lazy_softmax<OWN>: the frame-major forwards
    "ones32": (dict(ones=True, rows=32), True, True),
    "ones64": (dict(ones=True, rows=64), True, False),  # ones forward, plain-route backward
    "wave32_ones_bwd": (dict(rows=32), False, True),
}
_cache = {}


def unmasked_cases(hd, B, H, Lq, Lk, bwd=True):
    """(tag, q, k, v, do, mask) of one shape: the hard recipe at every shift under both group assignments, the ladder"""
    key = (hd, B, H, Lq, Lk, bwd)
    if key not in _cache:
        mask = torch.ones(B, Lq, Lk, dtype=torch.bool)
        out = []
        for shift in SC.SHIFTS:
            for assign in ("mod", "wave"):
                q, k, v = SC.hard_inputs(hd, H, mask, assign, shift)
                out.append((f"hard{shift:+d}.{assign}", q, k, v, SC.probe_do(q, k, v, mask)[0] if bwd else None, mask))
        q, k, v = SC.ladder_inputs(hd, B, H, Lq, Lk)
        out.append(("ladder", q, k, v, SC.probe_do(q, k, v, mask)[0] if bwd else None, mask))
        _cache[key] = out
    return _cache[key]


def masked_case(family, hd, H=2, bwd=True):
    """the hard recipe under the family's mask, groups by wave (token-major rows: by frame): the set scores 0, the keys no
    row of the group attends are traps at +G"""
    key = (family, hd, H, bwd)
    if key not in _cache:
        mask = MASKED[family][0]().clone()
        q, k, v = SC.hard_inputs(hd, H, mask, MASKED[family][2] if len(MASKED[family]) > 2 else "wave")
        _cache[key] = (f"{family}.hard.wave", q, k, v, SC.probe_do(q, k, v, mask)[0] if bwd else None, mask)
    return _cache[key]


def emulation(order, mask, fault=None):
    tiled, _, bwd_ones = ORDERS[order]
    return lambda q, k, v, do: AC.emulate(q, k, v, do, mask, tiled=tiled, bwd_ones=bwd_ones, fault=fault)


def all_cpu_cases():
    B, H = B_H
    for hd, (Lq, Lk) in ((32, (130, 257)), (72, (200, 100)), (128, (130, 33)), (64, (200, 64)), (96, (130, 192))):
        yield from unmasked_cases(hd, B, H, Lq, Lk)
    yield from unmasked_cases(72, 1, 2, 200, 200)
    for family in MASKED:
        yield masked_case(family, 72 if family in ("teacher", "band") else 64)


def test_the_shapes_are_the_issues():
    assert {s[0] for s in CROSS_SHAPES} | set(SELF_LENGTHS) == {130, 200}
    assert {s[1] for s in CROSS_SHAPES} == {33, 64, 100, 192, 257}
    assert B_H[0] * B_H[1] <= 6


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_underflow_threshold(hd):
    """G scale log2e >= 200 at every head dim, and in every hard case each unmasked score is its row's maximum or at
    least 200 binades below it (a trap: 200 above the set): nothing lies where denormal handling could matter"""
    c = SC.LOG2E / math.sqrt(hd)
    assert SC.A_GRP ** 2 * c >= 200
    for t in (30, -30, 120, -120):
        a, b = SC.shift_factors(hd, t)
        assert abs(a * b * c - t) <= 0.02 * abs(t) and float(torch.tensor(float(a)).to(bf16)) == a
    B, H = B_H
    cases = unmasked_cases(hd, B, H, 130, 257, bwd=False)[:-1] + [masked_case(f, hd, bwd=False) for f in ("kvlen", "causal")]
    for tag, q, k, v, _, mask in cases:
        ref = SC.expect(q, k, v, None, mask)
        s2 = ref["s2"].masked_fill(~mask[:, None], float("-inf"))
        below = s2.amax(-1, keepdim=True) - s2
        assert ((below == 0) | (below >= 200)).all(), tag
        valid = mask.any(1)[:, None, None, :] & ~mask[:, None]  # masked, but inside the launch: traps or -G
        assert ((ref["s2"] - s2.amax(-1, keepdim=True)).abs()[valid.expand_as(s2)] >= 200).all(), tag


@pytest.mark.parametrize("hd", [32, 72])
def test_hard_recipes_have_closed_forms(hd):
    """lse = ln N + T scale and o N = the label counts of the set, in float64, with the set read off the SCORES"""
    B, H = B_H
    cases = unmasked_cases(hd, B, H, 130, 257, bwd=False)[:-1] + [masked_case(f, hd, bwd=False) for f in MASKED]
    for tag, q, k, v, _, mask in cases:
        ref = SC.expect(q, k, v, None, mask)
        s = ref["s2"].masked_fill(~mask[:, None], float("-inf"))
        top = s.amax(-1, keepdim=True)
        inset = (s == top) & mask[:, None]
        n = inset.sum(-1)
        assert (n >= 1).all(), tag
        T = (q[0, 0, 0, hd - 1].double() * k[0, 0, 0, hd - 1].double()).item() / math.sqrt(hd)
        assert torch.allclose(ref["lse"], n.double().log() + top.squeeze(-1) / SC.LOG2E, rtol=0, atol=1e-9), tag
        assert ((top == T * SC.LOG2E) | (top == (T - SC.A_GRP ** 2 / math.sqrt(hd)) * SC.LOG2E)).all(), tag
        assert (top == T * SC.LOG2E).float().mean() > 0.8, tag  # (-G on every key: rows whose wave's set is outside their window)
        assert torch.allclose(ref["o"] * n[..., None], inset.double() @ v.double(), rtol=0, atol=1e-9), tag
        traps = ref["s2"] > top  # a masked key above the set: every masked family has some
        if tag.split(".")[0] in MASKED and not tag.startswith("window_lead0"):
            assert (traps & ~mask[:, None]).any(), tag
        assert not (traps & mask[:, None]).any(), tag


def test_the_sets_are_the_issues():
    s = SC.key_sets(257)
    assert s["first"] == [0] and s["last_valid"] == [256] and s["straddle_sub"] == [31, 32] and s["straddle_tile"] == [63, 64]
    assert len(s["one_per_sub"]) == 9 and sorted({k // 32 for k in s["one_per_sub"]}) == list(range(9))
    assert s["last_sub"] == [256] and SC.key_sets(100)["last_sub"] == [96, 97, 98, 99] and len(s["all"]) == 257
    assert s["pipe_sub1"] == list(range(32, 64)) and s["pipe_sub0"] == list(range(64, 96))
    for hd in HEAD_DIMS:  # a group column in the last 16-column K-slice, the shift in the last real column
        assert SC.col(9, 10, hd) == hd - 2 and (hd - 2) // 16 == (hd - 1) // 16


def test_the_ladder_straddles_the_threshold():
    for hd in HEAD_DIMS:
        q, k, _ = SC.ladder_inputs(hd, 3, 2, 130, 257)
        rise = q[0, 0, :, hd - 1].double() * SC.LOG2E / math.sqrt(hd)
        for w in range(0, 128, 32):
            assert (rise[w:w + 32] < 8).any() and (rise[w:w + 32] > 8).any()
        assert (rise[:96] != rise[32:128]).all()  # rows q and q + 32 differ
        span = (rise.max() * k[..., hd - 1].double().max()).item()
        assert span <= 41, span


def test_probe_rows_keep_the_floor():
    """dO is nonzero on probe rows only, PROBES_PER_HEAD of them in every head, and |dP - delta| >= 0.25 max |dP| (or 0)
    holds on each wherever P > 0"""
    for tag, q, k, v, do, mask in all_cpu_cases():
        rows = (do != 0).any(-1).sum(-1)
        assert (rows >= 4).all() and (rows <= SC.PROBES_PER_HEAD).all(), (tag, rows)
        assert SC.probe_rows_ok(q, k, v, do, mask), tag


def test_plain_bounds_stay_within_2_to_the_minus_6_of_a():
    for tag, q, k, v, do, mask in all_cpu_cases():
        if tag.startswith("ladder"):
            continue
        ref = SC.expect(q, k, v, do, mask)
        e_o, e_lse = SC.forward_bounds(ref)
        assert (e_o <= 2.0 ** -6 * ref["o"].abs()).all() and e_lse.max() <= 2.0 ** -6, tag
        assert (e_o / ref["o"].abs().clamp(min=1e-300)).max() <= 2.0 ** -8 + 1e-3, tag  # in fact the store's half ulp and fp32 terms


@pytest.mark.parametrize("order", list(ORDERS))
def test_the_emulation_stays_inside_every_bound(order):
    _, fwd_ones, bwd_ones = ORDERS[order]
    worst = {}
    for tag, q, k, v, do, mask in all_cpu_cases():
        w = SC.census(f"{order}.{tag}", emulation(order, mask), q, k, v, do, mask, fwd_ones, bwd_ones)
        worst = {n: max(x, worst.get(n, 0.0)) for n, x in w.items()}
    print(f"emulation {order}: " + " ".join(f"{n} {x:.3f}" for n, x in worst.items()))


# fault -> (order it is injected in, head dim, case tag, output, the element it must move by >= 2 bounds)
FAULTS = {}


def find_case(hd, tag):
    B, H = B_H
    if tag.split(".")[0] in MASKED:
        return masked_case(tag.split(".")[0], hd)
    return next(c for c in unmasked_cases(hd, B, H, 130, 257) if c[0] == tag)


def excess(run, q, k, v, do, mask, fwd_ones=False, bwd_ones=False):
    """error / bound per element of every output of run (a non-finite element counts as inf)"""
    ref = SC.expect(q, k, v, do, mask)
    e_o, e_lse = SC.forward_bounds(ref, fwd_ones)
    bounds = dict(o=e_o, lse=e_lse)
    bounds.update(zip(("dq", "dk", "dv"), SC.backward_bounds(ref, q, k, do, fwd_ones, bwd_ones)))
    got = dict(zip(("o", "lse", "dq", "dk", "dv"), run(q, k, v, do)))
    out = {}
    for n, g in got.items():
        err = (g.to(f64) - ref[n]).abs()
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
        out[n] = torch.where(err == 0, torch.zeros_like(err), err / bounds[n].clamp(min=1e-300))
    return out


# fault -> (evaluation order it is injected in, head dim, case, output, an element it moves by at least 2 bounds)
FAULTS = {
    "l_not_rescaled": ("wave32", 64, "hard+0.mod", "lse", (0, 0, 1)),  # set = the last valid key: l keeps 256 dead keys
    "neighbour_alpha": ("wave32", 64, "hard+0.mod", "o", (0, 0, 3, 1)),  # rows 2 and 3 rescale at different sub-blocks
    "p0_after_rescale": ("wave32", 64, "hard+0.wave", "o", (0, 0, 96, 1)),  # set {63, 64}: sub-block 0 all -G, key 63 in sub-block 1
    "pad_column": ("wave32", 64, "hard+0.mod", "lse", (0, 0, 2)),
    "last_key_not_in_max": ("wave32", 64, "hard+0.mod", "o", (0, 0, 1, 0)),  # the set is the last key of the ragged tile
    "masked_raises_max": ("wave32", 64, "causal.hard.wave", "o", (0, 0, 0, 0)),  # a trap at +G above the set
    "lse_other_half": ("wave64", 64, "ladder", "lse", (2, 1, 96)),  # rows q and q + 32 climb with different t_q
    "lse_bf16": ("wave32_ones_bwd", 64, "ladder", "dv", (2, 1, 0, 0)),
}
# what a float64 reference cannot fail, because the arithmetic stays right:
#   stale_threshold   m only ever rises, so `mx > m_stale + 8` holds wherever `mx > m + 8` does: the stale compare rescales
#                     MORE often, and every m is a valid reference point -- the outputs stay inside every bound
#   delta_unrounded   delta from the unrounded o is CLOSER to the float64 delta than the one the kernels are bound by
BENIGN = ("stale_threshold", "delta_unrounded")


@pytest.mark.parametrize("fault", list(FAULTS))
def test_an_injected_fault_leaves_the_bound_by_a_factor_of_two(fault):
    order, hd, tag, name, at = FAULTS[fault]
    _, fwd_ones, bwd_ones = ORDERS[order]
    _, q, k, v, do, mask = find_case(hd, tag)
    clean = excess(emulation(order, mask), q, k, v, do, mask, fwd_ones, bwd_ones)
    assert all(x.max() <= 1 for x in clean.values())
    bad = excess(emulation(order, mask, fault), q, k, v, do, mask, fwd_ones, bwd_ones)
    print(f"{fault}: {name}{list(at)} at {bad[name][at].item():.3g} bounds; worst " +
          " ".join(f"{n} {x.max().item():.3g}" for n, x in bad.items()))
    assert bad[name][at] >= 2, (fault, bad[name][at])
    with pytest.raises(AssertionError, match=rf"{fault}\.\w+\[.*(bound|finite)"):  # and the census itself names an element
        SC.census(fault, emulation(order, mask, fault), q, k, v, do, mask, fwd_ones, bwd_ones)


@pytest.mark.parametrize("fault", BENIGN)
def test_two_of_the_listed_faults_change_nothing_a_reference_can_see(fault):
    """(see BENIGN) every case stays inside every bound; the stale threshold does rescale more often"""
    for order in ("wave32", "own"):
        for tag, q, k, v, do, mask in unmasked_cases(64, *B_H, 130, 257):
            SC.census(f"{fault}.{tag}", emulation(order, mask, fault), q, k, v, do, mask)
    if fault == "delta_unrounded":
        _, q, k, v, do, mask = find_case(64, "ladder")
        ref = SC.expect(q, k, v, do, mask)
        o, _, of = AC.emulate_fwd_tiled(q, k, v, mask)
        d = lambda x: ((do.to(f64) * x.to(f64)).sum(-1) - ref["delta"]).abs().max()
        assert d(of) < d(o)


def test_the_lse_pair_fault_fails_after_a_ones_forward_too():
    """after the ones FORWARD the bound of P carries U scale sum |q_i k_i| for Q' = bf16(Q scale log2e), and a bf16 lse
    without its lo part (2^-9 |lse log2e| at worst) is of that size: the ladder still fails, by less than the factor of
    two that FAULTS shows after a plain forward"""
    _, q, k, v, do, mask = find_case(64, "ladder")
    with pytest.raises(AssertionError, match=r"lse_bf16\.d[qkv]\[.*bound"):
        SC.census("lse_bf16", emulation("ones32", mask, "lse_bf16"), q, k, v, do, mask, True, True)


@pytest.mark.parametrize("fault", ["l_not_rescaled", "neighbour_alpha", "stale_threshold", "p0_after_rescale"])
def test_the_norm_checks_on_gaussian_inputs_accept_the_first_four_faults(fault):
    """the inputs of tests/test_attn_causal_gpu.py and an unmasked Gaussian case, by relative Frobenius norm at the
    existing bounds (o 6e-3, lse 1e-3, gradients 8e-3): after the first sub-block no Gaussian score is 2^8 above the
    running maximum, so the rescale these faults break never runs"""
    hd, B, H, L = 64, 2, 2, 280
    q, k, v, do = _random_causal(hd, B, H, L)
    for mask in (AC.causal_mask(B, L, 16, 8), torch.ones(B, L, L, dtype=torch.bool)):
        got = AC.emulate(q, k, v, do, mask, tiled=dict(rows=32), fault=fault)
        ref = f64_reference(q, k, v, do, mask)
        errs = [rel(g, r) for g, r in zip(got, ref)]
        print(f"{fault}: " + " ".join(f"{e:.2e}" for e in errs))
        assert all(e < t for e, t in zip(errs, [TOL_O, TOL_LSE, TOL_G, TOL_G, TOL_G]))


def test_a_bf16_rounding_costs_up_to_2_to_the_minus_8():
    """why the forward bound counts U = 2^-8 per bf16 rounding and not 2^-9: head dim 72, Lq x Lk = 200 x 100, ladder,
    o[0, 0, 0, 0] is one key's P = 2^-5.97 over l, rounded once as P and once by the store -- the dense emulation is off by
    2^-7.65 of the element, more than 2 x 2^-9 allows"""
    tag, q, k, v, do, mask = unmasked_cases(72, *B_H, 200, 100)[-1]
    ref = SC.expect(q, k, v, None, mask)
    o = AC.emulate(q, k, v, None, mask)[0]
    r = ((o[0, 0, 0, 0].double() - ref["o"][0, 0, 0, 0]).abs() / ref["o"][0, 0, 0, 0]).item()
    assert 2.0 ** -8 < r < 2.0 ** -7, r


def test_the_instance_table_of_the_gpu_module_is_complete():
    """every family the GPU module runs is named in its docstring's table, every name there is a family, and the table
    lists every kernel piece and entry-point family the census is about"""
    import fnmatch
    import re
    import test_softmax_census_gpu as G
    doc = G.__doc__
    names = {n.strip() for grp in re.findall(r"\[([^\]]+)\]", doc) for n in re.split(r"[,/]", grp)}
    ids = {f for f, _ in G.UNMASKED_CASES} | {f"{f}-{h}" for f, h in G.MASKED_CASES}
    for i in ids:
        assert any(fnmatch.fnmatch(i, n) for n in names), f"{i} is not in the table"
    for n in names:
        assert any(fnmatch.fnmatch(i, n) for i in ids), f"the table names {n}, which nothing runs"
    for piece in ("lazy_softmax", "lazy_softmax<OWN>", "ones_softmax", "PIPE", "attn_fwd_wide_kernel", "attn_fwd16_kernel",
                  "attn_bwd_dq_kernel", "attn_bwd_dkv_kernel", "attn_bwd_dq16_kernel", "attn_bwd_dkv16_kernel",
                  "attn_delta_kernel", "dkv_reduce_kernel", "attn_qsplit", "cross_dkv16 = 2", "(hi, lo)",
                  "KVLEN", "CAUSAL", "PAST", "FM", "WIN", "TF", "BAND", "vds_teacher_attn_fwd", "vds_band_attn_fwd",
                  "_causal_fm_chunk", "_causal_fm_window", "vds_attn_fwd_causal_past", "m = -1e30"):
        assert piece in doc, piece
    assert {UN[0] for f, UN in G.UNMASKED.items() if f.startswith("plain")} == set(HEAD_DIMS)
    assert {(v, f) for v in (0, 1, 3, 7) for f in (0, 1)} == {(s[3]["variant"], s[3]["fold"]) for n, s in G.UNMASKED.items()
                                                              if n.startswith("ones_v")}
    assert set(G.MASKED_HEADS) == set(MASKED)
    assert {s for f, s in G.UNMASKED_CASES if isinstance(s, tuple)} >= set(CROSS_SHAPES)


def test_every_backward_case_has_gradients_worth_checking():
    """in every hard case the probes reach at least three different set sizes, one of them no power of two (P is rounded),
    and in every case each of dq, dk, dv has elements with a nonzero bound and nonzero values -- a backward whose answers
    are all exact zeros or powers of two would pin nothing.  (dq lives on the score columns only; the ladder's dq sums dS
    over balanced sub-blocks and may cancel to zero: it is held to its bound all the same.)"""
    for tag, q, k, v, do, mask in all_cpu_cases():
        ref = SC.expect(q, k, v, do, mask)
        probe = (do != 0).any(-1)
        sizes = {int(n) for n in (ref["p"] > 0).sum(-1)[probe]}
        assert tag.startswith("ladder") or (len(sizes) >= 3 and any(n & (n - 1) for n in sizes)), (tag, sizes)
        for name, e in zip(("dq", "dk", "dv"), SC.backward_bounds(ref, q, k, do)):
            bounded, nonzero = int((e > 0).sum()), int((ref[name].abs() > 1e-12).sum())
            assert bounded >= 32 and (nonzero >= 8 or (tag, name) == ("ladder", "dq")), (tag, name, bounded, nonzero)
