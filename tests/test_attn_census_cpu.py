"""The mask census (tests/helpers/attn_census.py) without a GPU: its expectations agree with float64 attention + autograd on
its own inputs, its conditions (n_c <= 64, |w - mean_w| >= 0.25 or exactly 0) hold for every case
tests/test_attn_census_gpu.py runs, and it discriminates: a torch emulation of the kernels' arithmetic passes every checker
with the right mask and fails with the mask flipped at ONE pair, while the relative Frobenius checks of
tests/test_attn_causal_gpu.py / test_attn_past_gpu.py / test_attn_kvlen_gpu.py on their random inputs accept the same flip.

The sub-block shortcut of the PAST kernels (fc_past_open) is emulated block by block.  Its three conditions err on the safe
side: `k0 + 32 <= lead + past` turned into `<`, or into `<= lead + past + 1` (the one extra key is row `lead`, frame 0, which
every token query attends), and `q0 >= lead` turned into `q0 > lead` all give the dense mask again -- no output can tell them
apart, which test_past_shortcut_* states.  What the census guards there is the pair just outside: the last past key, the
first past key at the first token row."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_census as AC  # noqa: E402

FC, KC = AC.FC, AC.KC
f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16

# the cases of tests/test_attn_census_gpu.py (kept in step by test_the_gpu_module_runs_these_cases)
CAUSAL = [(280, 16, 8), (140, 5, 3), (203, 0, 7), (159, 16, 13), (230, 32, 33), (293, 33, 65), (193, 64, 1)]
PAST = [(16, 15), (16, 16), (16, 17), (16, 47), (16, 48), (16, 49), (16, 112), (16, 14), (16, 46), (32, 32), (32, 33),
        (5, 27), (0, 64)]
PAST_PERIODS = {2: 70, 7: 20}  # period -> frames' rows: Lq = lead + 140
KV_LQ, KV_LK = 130, 200
KV_LENS = [[0, 1, 15, 16, 17, 63], [64, 65, KV_LK - 1, KV_LK, KV_LK + 5, 128]]
HEAD_DIMS = [32, 64, 72, 96, 128]
TOL_O, TOL_LSE, TOL_G = 6e-3, 1e-3, 8e-3  # the bounds of the three existing attention-mask test files


def f64_reference(q, k, v, do, mask):
    """float64 attention under mask [B, Lq, Lk] + autograd -> o, lse, dq, dk, dv (samples that attend nothing: zeros)"""
    q, k, v = (t.to(f64).requires_grad_(True) for t in (q, k, v))
    live = mask.any(-1).all(-1)
    o = torch.zeros(q.shape, dtype=f64)
    lse = torch.zeros(q.shape[:3], dtype=f64)
    idx = live.nonzero().flatten().tolist()
    ol, ll = [], []
    for b in idx:  # (masked_attention takes one [Lq, Lk] mask)
        ob, lb = FC.masked_attention(q[b], k[b], v[b], mask[b])
        ol.append(ob)
        ll.append(lb)
    if idx:
        ol = torch.stack(ol)
        if do is not None:
            ol.backward(do[idx].to(f64))
        o[idx], lse[idx] = ol.detach(), torch.stack(ll).detach()
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return o, lse, z(q), z(k), z(v)


def census(tag, hd, B, H, mask, lead=None, period=None, run=AC.emulate, bwd=True):
    """the whole census of one case on `run` (the emulation here, the library in the GPU module)"""
    _, Lq, Lk = mask.shape
    q, k, v = AC.forward_inputs(hd, B, H, Lq, Lk)
    o, lse = run(q, k, v, None, mask)[:2]
    AC.check_count(tag, lse, mask)
    AC.check_labels(tag, o, mask)
    if not bwd:
        return
    w = AC.signs(B, H, Lk, lead, period)
    pq = AC.probe_rows(B, H, hd, Lq, lead, period)
    q, k, v, do = AC.dkv_probe_inputs(hd, B, H, Lq, Lk, pq, w)
    o, lse, dq, dk, dv = run(q, k, v, do, mask)
    edv, edk, gap = AC.expect_dkv(mask, pq, w, hd)
    assert gap >= AC.MIN_GAP
    AC.check_count(tag + ".dkv", lse, mask)
    AC.check_support_and_values(tag + ".dv", dv, edv, AC.REL_DV)
    AC.check_support_and_values(tag + ".dk", dk, edk, AC.REL_DK)
    AC.check_zero(tag + ".dkv.dq", dq)
    pk = AC.probe_rows(B, H, hd, Lk, lead, period)
    q, k, v, do = AC.dq_probe_inputs(hd, B, H, Lq, Lk, pk, w)
    o, lse, dq, dk, dv = run(q, k, v, do, mask)
    edq, gap = AC.expect_dq(mask, pk, w, hd)
    assert gap >= AC.MIN_GAP
    AC.check_support_and_values(tag + ".dq", dq, edq, AC.REL_DK)
    AC.check_zero(tag + ".dq.dk", dk)


def all_masks():
    """(tag, mask [B, Lq, Lk], lead, period, backward?) of every GPU case"""
    for L, lead, period in CAUSAL:
        yield f"causal.L{L}_{lead}_{period}", AC.causal_mask(2, L, lead, period), lead, period, True
    for lead, past in PAST:
        for period, n in PAST_PERIODS.items():
            yield f"past.lead{lead}_past{past}_p{period}", AC.past_mask(2, lead + n * period, lead, period, past), lead, \
                period, False
    for i, lens in enumerate(KV_LENS):
        yield f"kvlen.cross{i}", AC.kvlen_mask(KV_LQ, KV_LK, lens), None, None, True
        yield f"kvlen.self{i}", AC.kvlen_mask(KV_LK, KV_LK, lens), None, None, True


def test_the_cases_are_valid_library_calls():
    """(L - lead) % period == 0 -- the entry points refuse anything else -- and the past sums sit where the issue wants"""
    for L, lead, period in CAUSAL:
        assert L >= lead and (L - lead) % period == 0, (L, lead, period)
    assert {lead + past for lead, past in PAST} >= {31, 32, 33, 63, 64, 65, 128, 30, 62}
    assert sorted(set(sum(KV_LENS, []))) == sorted({0, 1, 15, 16, 17, 63, 64, 65, 128, KV_LK - 1, KV_LK, KV_LK + 5})
    assert AC.kvlen_mask(4, KV_LK, [KV_LK + 5])[0].all()  # Lk + 5 clamps to Lk


def test_the_gpu_module_runs_these_cases():
    import ast
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_attn_census_gpu.py")).read()
    assert "from test_attn_census_cpu import" in src
    names = {a.name for n in ast.walk(ast.parse(src)) if isinstance(n, ast.ImportFrom) and n.module == "test_attn_census_cpu"
             for a in n.names}
    assert names >= {"CAUSAL", "PAST", "PAST_PERIODS", "KV_LENS", "KV_LQ", "KV_LK", "HEAD_DIMS"}


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_conditions_hold_for_every_case(hd):
    """n_c <= 64 for the label census and |w - mean_w| >= 0.25 (or exactly 0) on every attended probe pair, at the head
    counts the GPU module uses (B * H = 10 plain, 4 in the ones layout, 12 with key lengths); all rows probed at L <= 640"""
    for tag, mask, lead, period, bwd in all_masks():
        assert AC.label_counts(mask, hd).max().item() <= AC.MAX_LABEL, tag
        if not bwd:
            continue
        B, Lq, Lk = mask.shape
        for BB, H in ((5, 2), (2, 2), (6, 2)):
            m = mask[:1].expand(BB, Lq, Lk) if lead is not None else mask.repeat(3, 1, 1)[:BB]
            w = AC.signs(BB, H, Lk, lead, period)
            pq, pk = AC.probe_rows(BB, H, hd, Lq, lead, period), AC.probe_rows(BB, H, hd, Lk, lead, period)
            assert AC.expect_dkv(m, pq, w, hd)[2] >= AC.MIN_GAP, tag
            assert AC.expect_dq(m, pk, w, hd)[1] >= AC.MIN_GAP, tag
            for p, L in ((pq, Lq), (pk, Lk)):
                assert all(len(set(r.tolist())) == hd for r in p.reshape(-1, hd)), tag  # distinct inside a head
                if BB * H * hd >= L:
                    assert len(set(p.flatten().tolist())) == L, tag
    # 2096 rows (nothing in the GPU module is longer) at the smallest head dim but 32, where n_c is largest
    assert AC.label_counts(AC.causal_mask(1, 2096, 16, 8), 64).max().item() <= AC.MAX_LABEL


def test_probe_order_starts_with_the_edges():
    order = AC.probe_order(280, 16, 8)
    assert sorted(order) == list(range(280))
    head = set(order[:64])
    assert {0, 127, 128, 255, 256, 279, 63, 64, 31, 32, 15, 16, 17} <= head
    assert set(range(16, 24)) <= set(order[:80])  # a row of every frame


@pytest.mark.parametrize("hd", [32, 72])
def test_expectations_agree_with_float64_autograd(hd):
    """on the census inputs, for every case: lse = ln N, o N = n_c, and the probe gradients, against
    frame_causal_ref.masked_attention in float64 + autograd"""
    H = 2
    for tag, mask, lead, period, bwd in all_masks():
        B, Lq, Lk = mask.shape
        q, k, v = AC.forward_inputs(hd, B, H, Lq, Lk)
        o, lse = f64_reference(q, k, v, None, mask)[:2]
        n = AC.counts(mask)[:, None, :].to(f64)
        live = (n > 0).expand(lse.shape)
        assert torch.allclose(lse.exp()[live], n.expand(lse.shape)[live], rtol=1e-12, atol=0), tag
        assert torch.allclose(o * n[..., None], AC.label_counts(mask, hd)[:, None].to(f64).expand(o.shape), rtol=0, atol=1e-9), tag
        if not bwd:
            continue
        w = AC.signs(B, H, Lk, lead, period)
        pq, pk = AC.probe_rows(B, H, hd, Lq, lead, period), AC.probe_rows(B, H, hd, Lk, lead, period)
        q, k, v, do = AC.dkv_probe_inputs(hd, B, H, Lq, Lk, pq, w)
        _, _, dq, dk, dv = f64_reference(q, k, v, do, mask)
        edv, edk, _ = AC.expect_dkv(mask, pq, w, hd)
        assert torch.allclose(dv, edv, rtol=0, atol=1e-12) and torch.allclose(dk, edk, rtol=0, atol=1e-12), tag
        assert ((edv != 0) == (dv.abs() > 1e-14)).all() and dq.abs().max() == 0, tag
        q, k, v, do = AC.dq_probe_inputs(hd, B, H, Lq, Lk, pk, w)
        _, _, dq, dk, dv = f64_reference(q, k, v, do, mask)
        edq, _ = AC.expect_dq(mask, pk, w, hd)
        assert torch.allclose(dq, edq, rtol=0, atol=1e-12) and dk.abs().max() == 0, tag


@pytest.mark.parametrize("hd", [64, 72])
def test_the_emulation_passes_every_checker(hd):
    for tag, mask, lead, period, bwd in all_masks():
        census(tag, hd, mask.shape[0], 2, mask, lead, period, bwd=bwd)


def test_past_shortcut_is_the_dense_mask_and_its_safe_variants_too():
    """fc_past_open block by block, 32 and 64 queries per wave: the dense mask at every case; so are `<` for `<=`, one key
    of slack, and `q0 > lead` for `q0 >= lead` -- the shortcut only ever skips work, these variants change no output"""
    for lead, past in PAST:
        for period, n in PAST_PERIODS.items():
            Lq = lead + n * period
            dense = AC.past_mask(1, Lq, lead, period, past)
            for rows in (32, 64):
                for k_slack, q_slack in ((0, 0), (-1, 0), (1, 0), (0, -1)):
                    got = AC.past_mask_by_blocks(1, Lq, lead, period, past, k_slack, q_slack, rows)
                    assert torch.equal(got, dense), (lead, past, period, rows, k_slack, q_slack)


def test_past_shortcut_two_keys_of_slack_or_a_lead_query_in_the_wave_is_caught():
    """the nearest variants that do change the mask: two keys of slack at lead + past = 62 (a frame-1 key opens to the
    frame-0 queries), a wave that starts one row before lead = 33 (its lead query sees the past)"""
    for (lead, past, k_slack, q_slack) in ((16, 46, 2, 0), (33, 63, 0, 1)):
        Lq = lead + 140
        wrong = AC.past_mask_by_blocks(2, Lq, lead, 2, past, k_slack, q_slack)
        right = AC.past_mask(2, Lq, lead, 2, past)
        assert not torch.equal(wrong, right)
        with pytest.raises(AssertionError, match=r"\[b=0, h=0, q="):
            census("mut", 64, 2, 2, right, lead, 2, run=lambda q, k, v, do, m: AC.emulate(q, k, v, do, wrong), bwd=False)


def _random_causal(hd, B, H, L):
    g = torch.Generator().manual_seed(201)
    qkv = torch.randn(B * L, 3 * H * hd, generator=g).to(bf16)
    do = torch.randn(B * L, H * hd, generator=torch.Generator().manual_seed(202)).to(bf16)
    hv = lambda t, off: t[:, off:off + H * hd].reshape(B, L, H, hd).permute(0, 2, 1, 3)
    return hv(qkv, 0), hv(qkv, H * hd), hv(qkv, 2 * H * hd), hv(do, 0)


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-20)).item()


def norm_checks_accept(q, k, v, do, wrong, right):
    """the emulation under the WRONG mask against the reference under the right one, by relative Frobenius norm at the
    existing bounds"""
    got = AC.emulate(q, k, v, do, wrong)
    ref = f64_reference(q, k, v, do, right)
    errs = [rel(g, r) for g, r in zip(got, ref)]
    print("norm checks:", " ".join(f"{e:.2e}" for e in errs))
    return all(e < t for e, t in zip(errs, [TOL_O, TOL_LSE, TOL_G, TOL_G, TOL_G]))


def flipped(mask, b, q, k):
    m = mask.clone()
    m[b, q, k] = ~m[b, q, k]
    return m


# one pair each.  causal (203, 0, 7): query 128, the first row of the second 128-row tile, is frame 2 and gains key 3
# (frame 3); (280, 16, 8): query 279, the last row, loses key 279.  past, lead + past = 64, period 2: token query 16 loses
# the last past key 63 (an off-by-one in `k0 + 32 <= lead + past`); lead = 32: query 32, the first token row and the first
# row of wave 1, loses the first past key 32 (an off-by-one around `q0 >= lead`).  kvlen: query 0 gains the first key past
# its sample's length.  (The norm checks are not blind to EVERY single pair at these small shapes: a query that attends few
# keys and gains one with a large random score -- query 128 of (280, 16, 8) with key 17, the last lead row with a past key
# -- moves its row of o enough to reach 6e-3.  That is luck, not coverage.)
SINGLE_PAIR = {
    "extra_key_at_a_tiles_first_row": ("causal", (203, 0, 7), (128, 3)),
    "missing_key_at_the_last_row": ("causal", (280, 16, 8), (279, 279)),
    "last_past_key_missing_at_sum_64": ("past", (16, 48, 2), (16, 63)),
    "first_past_key_missing_at_the_first_token_row_at_lead_32": ("past", (32, 32, 2), (32, 32)),
    "one_key_past_the_length": ("kvlen", [64, 65, 199, 200, 205, 128], (0, None)),
}


@pytest.mark.parametrize("name", list(SINGLE_PAIR))
def test_one_flipped_pair_fails_the_census_and_passes_the_norm_checks(name):
    kind, case, (qr, kr) = SINGLE_PAIR[name]
    hd, H = 64, 2
    if kind == "causal":
        L, lead, period = case
        B = 5
        right = AC.causal_mask(B, L, lead, period).clone()
        rand = _random_causal(hd, B, H, L)  # the inputs of tests/test_attn_causal_gpu.py
    elif kind == "past":
        lead, past, period = case
        B, Lq = 2, lead + 140
        right = AC.past_mask(B, Lq, lead, period, past).clone()
        g = torch.Generator().manual_seed(301)
        rand = [torch.randn(B, H, n, hd, generator=g).to(bf16) for n in (Lq, Lq + past, Lq + past)] + [None]
    else:
        lead = period = None
        B = 6
        right = AC.kvlen_mask(KV_LQ, KV_LK, case).clone()
        g = torch.Generator().manual_seed(101)
        rand = [torch.randn(B, H, n, hd, generator=g).to(bf16) for n in (KV_LQ, KV_LK, KV_LK, KV_LQ)]
    bwd = kind != "past"
    Lq, Lk = right.shape[1:]
    pq, pk = AC.probe_rows(B, H, hd, Lq, lead, period), AC.probe_rows(B, H, hd, Lk, lead, period)
    # the sample whose mask is flipped: one in which the pair's rows are probes (every row is a probe of SOME head; the flip
    # is in one sample only)
    b = 1
    if bwd:
        b = next(i for i in range(B) if (pq[i] == qr).any() and (pk[i] == (case[i] if kr is None else kr)).any())
        kr = case[b] if kr is None else kr  # kvlen: the first key past the sample's length
    wrong = flipped(right, b, qr, kr)
    assert (wrong != right).sum().item() == 1
    bwd = kind != "past"
    census(name, hd, B, H, right, lead, period, bwd=bwd)  # the right mask passes
    bad_run = lambda q, k, v, do, m: AC.emulate(q, k, v, do, wrong)
    with pytest.raises(AssertionError, match=rf"\[b={b}, h=0, q={qr}\]"):  # the count names the row
        census(name, hd, B, H, right, lead, period, run=bad_run, bwd=False)
    # ... and so does each of the other checkers on its own
    q, k, v = AC.forward_inputs(hd, B, H, right.shape[1], right.shape[2])
    with pytest.raises(AssertionError, match=rf"o\[b={b}, h=0, q={qr}, c={kr % hd}\]"):
        AC.check_labels(name, AC.emulate(q, k, v, None, wrong)[0], right)
    if bwd:
        w = AC.signs(B, H, Lk, lead, period)
        q, k, v, do = AC.dkv_probe_inputs(hd, B, H, Lq, Lk, pq, w)
        edv, edk, _ = AC.expect_dkv(right, pq, w, hd)
        _, _, _, dk, dv = AC.emulate(q, k, v, do, wrong)
        with pytest.raises(AssertionError, match=rf"\[b={b}, h=\d, row={kr}, c="):
            AC.check_support_and_values(name + ".dv", dv, edv, AC.REL_DV)
        with pytest.raises(AssertionError, match=rf"\[b={b}, h=\d, row={kr}, c="):
            AC.check_support_and_values(name + ".dk", dk, edk, AC.REL_DK)
        q, k, v, do = AC.dq_probe_inputs(hd, B, H, Lq, Lk, pk, w)
        edq, _ = AC.expect_dq(right, pk, w, hd)
        with pytest.raises(AssertionError, match=rf"\[b={b}, h=\d, row={qr}, c="):
            AC.check_support_and_values(name + ".dq", AC.emulate(q, k, v, do, wrong)[2], edq, AC.REL_DK)
    assert norm_checks_accept(*rand, wrong, right), "the existing norm checks see this flip"
