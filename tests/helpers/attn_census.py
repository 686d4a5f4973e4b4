"""Mask census for the attention kernels (tests/test_attn_census_cpu.py, tests/test_attn_census_gpu.py): inputs for which
the right answer of a masked attention call is a count, so that ONE wrong (query, key) pair anywhere fails a test.  CPU
only, no import of the library.

Every score is made equal (Q = 0 or K = 0), so P[q, k] = 1 / N(q) on the attended pairs, N(q) = the keys q attends.

  forward   Q = 0, K random (live loads that cannot matter), V[k, :] = one-hot of label(k) = k % hd:
              lse[q] = ln N(q)                      -> check_count:  |exp(lse) - N| < 0.25
              o[q, c] N(q) = n_c(q), the attended keys with label c -> check_labels: |o N - n_c| < 0.25
  dK / dV   K = 0, up to hd probe queries q_c per head (another set in every head): Q[q_c] = dO[q_c] = e_c, every other
            row of Q and dO zero, V[k, :] = w(k) in {+1, -1}:
              dV[k, c] = 1 / N(q_c),  dK[k, c] = scale (w(k) - mean_w(q_c)) / N(q_c)  if q_c attends k, else exactly 0
  dQ        Q = 0, probe keys K[k_c] = e_c, every other row of K zero, dO[q] = e_0, V[k, 0] = w(k):
              dQ[q, c] = scale (w(k_c) - mean_w(q)) / N(q)  if q attends k_c, else exactly 0
            -> check_support_and_values: got != 0 exactly where the float64 expectation is, then every element within a
               relative bound (REL_DV, REL_DK; dQ takes REL_DK)

The bounds come from the formats (bf16: 8 significant bits, round to nearest: 2^-8 relative at worst, 2^-9 absolute below 1):

  0.25     adjacent counts differ by 1.  lse is fp32: ln N <= 8 has an ulp of 5e-7 and the kernels' log2 / the test's exp
           keep |exp(lse) - N| below N * 1e-5.  exp2(0) = 1 is exact in bf16, V is 0 / 1 and the fp32 accumulators hold
           integers, so o is the bf16 rounding of n_c / N: |o N - n_c| <= n_c 2^-8, <= 0.25 while n_c <= 64 (MAX_LABEL; the
           cases stay at n_c <= 17, an error below 0.07)
  REL_DV   2^-7: P = 1 / N rounded to bf16 (2^-8); the single product P * 1 is exact in the fp32 accumulator and a bf16
           value already, so the store adds nothing; 2 x margin
  REL_DK   2^-6: delta = dO . o is read from the bf16 o, |error| <= 2^-9 because |mean_w| < 1, against |w - mean_w| >= 0.25
           (MIN_GAP): 2^-7; dS rounded to bf16: 2^-8; the product with the softmax scale rounded by the store: 2^-8.  Where
           w(k) = mean_w exactly (a query whose keys all carry one sign) o is +-1, delta is exact and the expectation and
           the kernel's value are both 0: the support check covers it.

The masks are bool [B, Lq, Lk] built from frame_causal_ref.allowed, frame_cache_ref.past_allowed and k < kv_lens[b]."""
import math

import torch

import frame_cache_ref as KC

FC = KC.FC
f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16
TOL_COUNT = 0.25
REL_DV, REL_DK = 2.0 ** -7, 2.0 ** -6
MAX_LABEL, MIN_GAP = 64, 0.25


# ------------------------------------------------------------------------------ masks ----
def causal_mask(B, L, lead, period):
    return FC.allowed(L, lead, period)[None].expand(B, L, L)


def past_mask(B, Lq, lead, period, past):
    return KC.past_allowed(Lq, lead, period, past)[None].expand(B, Lq, Lq + past)


def kvlen_mask(Lq, Lk, lens):
    """sample b attends its first min(max(lens[b], 0), Lk) keys"""
    n = torch.tensor(lens).clamp(0, Lk)
    return (torch.arange(Lk)[None, None, :] < n[:, None, None]).expand(len(lens), Lq, Lk)


# ----------------------------------------------------------------------------- probes ----
def probe_order(L, lead=None, period=None):
    """every row of range(L) once, the rows at which a kernel's row logic changes first: the first and last row of every
    16-, 32-, 64- and 128-row block, lead - 1, lead, lead + 1, the last row, one row of every frame; then the rest"""
    first = []
    for blk in (128, 64, 32, 16):
        for s in range(0, L, blk):
            first += [s, min(s + blk, L) - 1]
    if lead is not None:
        first += [lead - 1, lead, lead + 1]
        first += [lead + f for f in range(period)]
    first.append(L - 1)
    seen, order = set(), []
    for r in first + list(range(L)):
        if 0 <= r < L and r not in seen:
            seen.add(r)
            order.append(r)
    return order


def probe_rows(B, H, hd, L, lead=None, period=None):
    """int64 [B, H, hd]: head i takes rows i * hd .. of probe_order, round robin -- distinct inside a head, another set in
    every head, and every row is a probe of some head when B * H * hd >= L"""
    assert hd <= L
    order = probe_order(L, lead, period)
    idx = (torch.arange(B * H * hd) % L).view(B, H, hd)
    return torch.tensor(order)[idx]


def signs(B, H, Lk, lead=None, period=None):
    """w [B, H, Lk] in {+1, -1}, balanced inside every set of keys a query can attend: alternating over the lead rows and
    over the rows of each frame (or over all rows without frames), flipped from one head to the next"""
    k = torch.arange(Lk)
    if lead is None:
        w = 1 - 2 * (k % 2)
    else:
        w = torch.where(k < lead, 1 - 2 * (k % 2), 1 - 2 * (((k - lead) // period) % 2))
    flip = 1 - 2 * (torch.arange(B * H) % 2).view(B, H, 1)
    return (w[None, None, :] * flip).to(f64)


# ----------------------------------------------------------------------------- inputs ----
def forward_inputs(hd, B, H, Lq, Lk, seed=11):
    """bf16 q, k, v [B, H, L, hd]: Q = 0, K random, V the one-hot of k % hd"""
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros(B, H, Lq, hd, dtype=bf16)
    k = torch.randn(B, H, Lk, hd, generator=g).to(bf16)
    v = torch.zeros(B, H, Lk, hd, dtype=bf16)
    v[:, :, torch.arange(Lk), torch.arange(Lk) % hd] = 1
    return q, k, v


def dkv_probe_inputs(hd, B, H, Lq, Lk, probes, w):
    """bf16 q, k, v, do: K = 0, Q[q_c] = dO[q_c] = e_c on the probe queries [B, H, hd], V[k, :] = w(k)"""
    q = torch.zeros(B, H, Lq, hd, dtype=bf16)
    q.scatter_(2, probes[:, :, None, :], torch.ones(B, H, 1, hd, dtype=bf16))  # q[b, h, probes[b, h, c], c] = 1
    k = torch.zeros(B, H, Lk, hd, dtype=bf16)
    v = w.to(bf16)[..., None].expand(B, H, Lk, hd).contiguous()
    return q, k, v, q.clone()


def dq_probe_inputs(hd, B, H, Lq, Lk, probes, w):
    """bf16 q, k, v, do: Q = 0, K[k_c] = e_c on the probe keys [B, H, hd], dO[q] = e_0, V[k, 0] = w(k)"""
    q = torch.zeros(B, H, Lq, hd, dtype=bf16)
    k = torch.zeros(B, H, Lk, hd, dtype=bf16)
    k.scatter_(2, probes[:, :, None, :], torch.ones(B, H, 1, hd, dtype=bf16))
    v = torch.zeros(B, H, Lk, hd, dtype=bf16)
    v[..., 0] = w.to(bf16)
    do = torch.zeros(B, H, Lq, hd, dtype=bf16)
    do[..., 0] = 1
    return q, k, v, do


# ----------------------------------------------------------------------- expectations ----
def counts(mask):
    """N int64 [B, Lq]"""
    return mask.sum(-1)


def label_counts(mask, hd):
    """n_c int64 [B, Lq, hd]: the attended keys with k % hd == c"""
    Lk = mask.shape[-1]
    onehot = torch.zeros(Lk, hd, dtype=f64)
    onehot[torch.arange(Lk), torch.arange(Lk) % hd] = 1
    return (mask.to(f64) @ onehot).round().long()


def _mean_w(mask, w):
    """mean of w over the keys each query attends, f64 [B, H, Lq] (0 where it attends none)"""
    m = mask.to(f64)[:, None]  # [B, 1, Lq, Lk]
    n = m.sum(-1)
    return (m * w[:, :, None, :]).sum(-1) / n.clamp(min=1), n


def expect_dkv(mask, probes, w, hd):
    """(dV, dK) f64 [B, H, Lk, hd] of dkv_probe_inputs, and the smallest nonzero |w(k) - mean_w(q_c)| of an attended pair"""
    B, H, _ = probes.shape
    mean, n = _mean_w(mask, w)  # [B, H, Lq]
    bi = torch.arange(B)[:, None, None]
    att = mask[bi, probes].to(f64)  # [B, H, hd, Lk]: probe c attends key k
    n_c = torch.gather(n.expand(B, H, -1), 2, probes)[..., None].clamp(min=1)
    mean_c = torch.gather(mean, 2, probes)[..., None]
    gap = att * (w[:, :, None, :] - mean_c)
    dv = (att / n_c).transpose(2, 3)
    dk = (gap / n_c / math.sqrt(hd)).transpose(2, 3)
    return dv.contiguous(), dk.contiguous(), _min_gap(gap)


def expect_dq(mask, probes, w, hd):
    """dQ f64 [B, H, Lq, hd] of dq_probe_inputs, and the smallest nonzero |w(k_c) - mean_w(q)| of an attended pair"""
    B, H, _ = probes.shape
    mean, n = _mean_w(mask, w)
    Lq = mask.shape[1]
    att = torch.gather(mask[:, None].expand(B, H, Lq, -1), 3, probes[:, :, None, :].expand(B, H, Lq, hd)).to(f64)
    w_c = torch.gather(w, 2, probes)[:, :, None, :]  # [B, H, 1, hd]
    gap = att * (w_c - mean[..., None])
    return gap / n.clamp(min=1)[..., None] / math.sqrt(hd), _min_gap(gap)


def _min_gap(gap):
    nz = gap.abs()[gap != 0]
    return nz.min().item() if nz.numel() else float("inf")


# --------------------------------------------------------------------------- checkers ----
def _first(bad):
    return tuple(int(i) for i in bad.nonzero()[0])


def check_count(tag, lse, mask):
    """lse f32 [B, H, Lq]: |exp(lse) - N(q)| < 0.25 in float64 on every row; a row that attends nothing has lse = 0
    (what tests/test_attn_kvlen_gpu.py pins for it).  Returns the worst |exp(lse) - N|."""
    n = counts(mask)[:, None, :].expand(lse.shape)
    assert torch.isfinite(lse).all(), f"{tag}.lse: row (b, h, q) = {_first(~torch.isfinite(lse))} unwritten or not finite"
    err = torch.where(n > 0, (lse.to(f64).exp() - n).abs(), lse.to(f64).abs() * 1e30)
    bad = ~(err < TOL_COUNT)
    if bad.any():
        b, h, q = _first(bad)
        raise AssertionError(f"{tag}.lse[b={b}, h={h}, q={q}]: exp(lse) = {math.exp(lse[b, h, q].item()):.4f}, the row "
                             f"attends {int(n[b, h, q])} keys")
    return err[n > 0].max().item() if (n > 0).any() else 0.0


def check_labels(tag, o, mask):
    """o [B, H, Lq, hd]: |o N - n_c| < 0.25 for every label c; a row that attends nothing is exact zeros.  Returns the
    worst |o N - n_c|."""
    hd = o.shape[-1]
    n = counts(mask)[:, None, :, None].to(f64)
    n_c = label_counts(mask, hd)[:, None].expand(o.shape)
    assert n_c.max().item() <= MAX_LABEL, f"{tag}: n_c = {n_c.max().item()} > {MAX_LABEL}: the bf16 store is too coarse"
    od = o.to(f64)
    assert torch.isfinite(od).all(), f"{tag}.o: (b, h, q, c) = {_first(~torch.isfinite(od))} unwritten or not finite"
    err = torch.where(n > 0, (od * n - n_c).abs(), od.abs() * 1e30)
    bad = ~(err < TOL_COUNT)
    if bad.any():
        b, h, q, c = _first(bad)
        raise AssertionError(f"{tag}.o[b={b}, h={h}, q={q}, c={c}] * N = {od[b, h, q, c].item() * n[b, 0, q, 0].item():.4f}"
                             f": the row attends {int(n_c[b, h, q, c])} keys with k % {hd} == {c} of {int(n[b, 0, q, 0])}")
    return err.max().item()


def check_support_and_values(tag, got, ref, rel):
    """got [B, H, L, hd] against the float64 expectation: nonzero exactly where it is, then |got - ref| <= rel |ref| on
    every element.  Returns the worst relative error."""
    g = got.to(f64)
    assert g.shape == ref.shape, (tag, g.shape, ref.shape)
    assert torch.isfinite(g).all(), f"{tag}: (b, h, row, c) = {_first(~torch.isfinite(g))} unwritten or not finite"
    bad = (g != 0) != (ref != 0)
    if bad.any():
        b, h, r, c = _first(bad)
        raise AssertionError(f"{tag}[b={b}, h={h}, row={r}, c={c}] = {g[b, h, r, c].item():.6g}, expected "
                             f"{ref[b, h, r, c].item():.6g}: " + ("an excluded pair contributes" if ref[b, h, r, c] == 0
                                                                 else "an attended pair is missing"))
    err = (g - ref).abs() / ref.abs().clamp(min=1e-300)
    err = torch.where(ref != 0, err, torch.zeros_like(err))
    bad = ~(err <= rel)
    if bad.any():
        b, h, r, c = _first(bad)
        raise AssertionError(f"{tag}[b={b}, h={h}, row={r}, c={c}] = {g[b, h, r, c].item():.6g}, expected "
                             f"{ref[b, h, r, c].item():.6g}: relative error {err[b, h, r, c].item():.3e} > {rel:.3e}")
    return err.max().item()


def check_zero(tag, got):
    """an output the inputs make exactly zero (dQ with K = 0, dK with Q = 0): written, and zero"""
    g = got.to(f64)
    assert torch.isfinite(g).all(), f"{tag}: (b, h, row, c) = {_first(~torch.isfinite(g))} unwritten or not finite"
    assert (g == 0).all(), f"{tag}[(b, h, row, c) = {_first(g != 0)}] must be an exact zero"


# -------------------------------------------------- a torch emulation of the kernels ----
LOG2E, LAZY_THR = 1.4426950408889634, 8.0  # csrc/attention.hip


def _any_in_wave(x, rows):
    """bool [B, H, Lq] -> the ballot of each wave of `rows` queries, on every row of the wave"""
    B, H, L = x.shape
    xp = torch.nn.functional.pad(x, (0, (-L) % rows)).view(B, H, -1, rows)
    return xp.any(-1, keepdim=True).expand_as(xp).reshape(B, H, -1)[..., :L]


def emulate_fwd_tiled(q, k, v, mask, own=False, ones=False, rows=32, fault=None):
    """the forward kernels' evaluation order: 32-key sub-blocks, a running maximum m in the log2 domain that starts at
    -1e30 and is raised (O and l rescaled) only where the ballot of a wave of `rows` queries finds a sub-block maximum
    above m + LAZY_THR -- every row of the wave then (lazy_softmax), or only the rows that are over it themselves (own:
    lazy_softmax<OWN>).  ones (ones_softmax): Q' = bf16(Q scale log2e), m a bf16 value that starts at 0, a row's
    first sub-block with an attended key always sets it, and the denominator is summed from the bf16 P (it is a row of the O accumulator).
    fault: one of the defects tests/test_softmax_census_cpu.py injects.  Returns o (bf16), lse (fp32), o unrounded."""
    B, H, Lq, hd = q.shape
    Lk = k.shape[2]
    r = lambda t: t.to(bf16).to(f32)
    c = torch.tensor(1.0 / math.sqrt(hd), dtype=f32) * torch.tensor(LOG2E, dtype=f32)
    qf, kf, vf = q.to(f32), k.to(f32), v.to(f32)
    s_all = (r(qf * c) if ones else qf) @ kf.transpose(-1, -2)
    if fault == "pad_column":  # a column beyond head_dim meets a 1 in Q and the key's parity in K
        s_all = s_all + (torch.arange(Lk) % 2).to(f32) * (c if ones else 1.0)
    m4 = mask[:, None].expand(B, H, Lq, Lk)
    valid = mask.any(1)[:, None, None, :].expand(B, H, Lq, Lk)  # keys inside the launch's bounds
    last = (valid[:, 0, 0].long() * torch.arange(Lk)).amax(-1)  # the last valid key of each sample
    neg = torch.tensor(float("-inf"))
    m = torch.full((B, H, Lq), 0.0 if ones else -1e30, dtype=f32)
    m_prev, l, o = m.clone(), torch.zeros(B, H, Lq), torch.zeros(B, H, Lq, hd)
    pending, seen = None, torch.zeros(B, H, Lq, dtype=torch.bool)
    for i, k0 in enumerate(range(0, Lk, 32)):
        sl = slice(k0, min(k0 + 32, Lk))
        live = m4[..., sl]
        s = s_all[..., sl] if ones else s_all[..., sl] * c
        sm = torch.where(live, s, neg)
        src = sm
        if fault == "masked_raises_max":
            src = torch.where(valid[..., sl], s, neg)
        if fault == "last_key_not_in_max":
            src = torch.where((torch.arange(sl.start, sl.stop)[None, :] == last[:, None])[:, None, None, :], neg, sm)
        mx = src.amax(-1)
        if ones:
            rel = mx - m
            fresh = ~seen & torch.isfinite(rel)  # the row's first sub-block with a key it attends sets m, whatever it is
            seen = seen | fresh
            m_new = torch.where(_any_in_wave((rel > LAZY_THR) | fresh, rows), r(m + rel.clamp(min=0)), m)
            m_new = torch.where(fresh, r(m + rel), m_new)
        else:
            trig = mx > (m_prev if fault == "stale_threshold" else m) + LAZY_THR
            m_new = torch.where(trig if own else _any_in_wave(trig, rows), torch.maximum(m, mx), m)
        alpha = torch.exp2(m - m_new)
        if ones:
            alpha = torch.where(fresh, torch.ones(()), alpha)  # (ones_softmax: first -> alpha = 1; O and l are 0)
        if fault == "neighbour_alpha":
            alpha = alpha[..., (torch.arange(Lq) ^ 1).clamp(max=Lq - 1)]
        e = torch.where(live, torch.exp2(s - m_new[..., None]), torch.zeros(()))
        pv = r(e) @ vf[:, :, sl]
        l = (l if fault == "l_not_rescaled" else l * alpha) + (r(e) if ones else e).sum(-1)
        o = o * alpha[..., None]
        if fault == "p0_after_rescale" and i % 2 == 0:
            pending = pv  # sub-block 0's product lands after sub-block 1's rescale
        else:
            o = o + pv + (0 if pending is None else pending)
            pending = None
        m_prev, m = m, m_new
    if pending is not None:
        o = o + pending
    some = (l > 0)
    m_out = m[..., (torch.arange(Lq) ^ 32).clamp(max=Lq - 1)] if fault == "lse_other_half" else m
    lse = torch.where(some, (m_out + torch.log2(l.clamp(min=1e-37))) * math.log(2.0), torch.zeros(()))
    of = torch.where(some[..., None], o / l.clamp(min=1e-37)[..., None], torch.zeros(()))
    if fault in ("last_key_not_in_max", "masked_raises_max"):  # an overflowed or emptied row stays what the hardware gives
        lse = torch.where(mask.any(-1)[:, None], (m_out + torch.log2(l)) * math.log(2.0), torch.zeros(()))
        of = torch.where(mask.any(-1)[:, None, :, None], o / l[..., None], torch.zeros(()))
    return of.to(bf16), lse, of


def emulate_bwd(q, k, v, do, mask, o, lse, ones=False, fault=None, o_unrounded=None):
    """the backward kernels on a forward's o and lse: P = exp2(s c - lse log2e) recomputed in fp32 (ones: from Q' = bf16(Q c)
    and -lse log2e as a bf16 (hi, lo) pair), delta from the bf16 o, P and dS rounded to bf16 for their products, fp32
    sums, bf16 stores.  Returns dq, dk, dv."""
    hd = q.shape[-1]
    scale = 1.0 / math.sqrt(hd)
    r = lambda t: t.to(bf16).to(f32)
    c = torch.tensor(scale, dtype=f32) * torch.tensor(LOG2E, dtype=f32)
    qf, kf, vf, dof = q.to(f32), k.to(f32), v.to(f32), do.to(f32)
    m4 = mask[:, None]
    lse2 = lse * torch.tensor(LOG2E, dtype=f32)
    if fault == "lse_bf16":
        lse2 = r(lse2)
    elif ones:
        lse2 = r(lse2) + r(lse2 - r(lse2))
    s2 = (r(qf * c) @ kf.transpose(-1, -2)) if ones else (qf @ kf.transpose(-1, -2)) * c
    p = torch.where(m4, torch.exp2(s2 - lse2[..., None]), torch.zeros(()))
    delta = (dof * (o_unrounded if fault == "delta_unrounded" else o.to(f32))).sum(-1, keepdim=True)
    ds = r(p * (dof @ vf.transpose(-1, -2) - delta))
    dv = (r(p).transpose(-1, -2) @ dof).to(bf16)
    dk = ((ds.transpose(-1, -2) @ qf) * scale).to(bf16)
    dq = ((ds @ kf) * scale).to(bf16)
    return dq, dk, dv


def emulate(q, k, v, do, mask, tiled=None, bwd_ones=False, fault=None):
    """the kernels' arithmetic on bf16 inputs [B, H, L, hd] under a bool mask [B, Lq, Lk]: fp32 scores, mask, softmax, P and
    dS rounded to bf16 for their products, fp32 sums, bf16 outputs; delta from the bf16 o.  A sample that attends nothing
    gives zeros.  Returns o, lse and (do given) dq, dk, dv.
    tiled: keywords of emulate_fwd_tiled (own, ones, rows) -- the forward by 32-key sub-blocks with the lazy threshold,
    the backward by emulate_bwd (bwd_ones: its ones route); fault goes to whichever of the two knows it."""
    if tiled is not None or bwd_ones or fault is not None:
        o, lse, of = emulate_fwd_tiled(q, k, v, mask, fault=fault, **(tiled or {}))
        if do is None:
            return o, lse
        return (o, lse) + emulate_bwd(q, k, v, do, mask, o, lse, bwd_ones, fault, of)
    scale = 1.0 / math.sqrt(q.shape[-1])
    r = lambda t: t.to(bf16).to(f32)
    qf, kf, vf = q.to(f32), k.to(f32), v.to(f32)
    m4 = mask[:, None]
    live = m4.any(-1, keepdim=True)
    s = ((qf @ kf.transpose(-1, -2)) * scale).masked_fill(~m4, float("-inf"))
    mx = torch.where(live, s.amax(-1, keepdim=True), torch.zeros(()))
    e = torch.where(m4, (s - mx).exp(), torch.zeros(()))
    l = e.sum(-1, keepdim=True)
    o = torch.where(live, (r(e) @ vf) / l.clamp(min=1e-30), torch.zeros(())).to(bf16)
    lse = torch.where(live, mx + l.clamp(min=1e-30).log(), torch.zeros(())).squeeze(-1)
    if do is None:
        return o, lse
    dof = do.to(f32)
    p = torch.where(m4, (s - lse[..., None]).exp(), torch.zeros(()))
    delta = (dof * o.to(f32)).sum(-1, keepdim=True)
    ds = r(p * (dof @ vf.transpose(-1, -2) - delta))
    dv = (r(p).transpose(-1, -2) @ dof).to(bf16)
    dk = ((ds.transpose(-1, -2) @ qf) * scale).to(bf16)
    dq = ((ds @ kf) * scale).to(bf16)
    return o, lse, dq, dk, dv


def past_mask_by_blocks(B, Lq, lead, period, past, k_slack=0, q_slack=0, rows=32):
    """the mask the PAST forward kernels apply, the way they apply it: a wave of `rows` queries from q0 takes a 32-key
    sub-block from k0 unmasked when  k0 >= lead and k0 + 32 <= lead + past + k_slack and q0 + q_slack >= lead
    (fc_past_open in csrc/attention.hip; the slacks are 0 there) and element by element otherwise"""
    Lk = Lq + past
    dense = KC.past_allowed(Lq, lead, period, past)
    out = dense.clone()
    for q0 in range(0, Lq, rows):
        for k0 in range(0, Lk, 32):
            if k0 >= lead and k0 + 32 <= lead + past + k_slack and q0 + q_slack >= lead:
                out[q0:q0 + rows, k0:k0 + 32] = True
    return out[None].expand(B, Lq, Lk)
