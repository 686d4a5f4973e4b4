"""Softmax census of the attention value path (tests/test_softmax_census_cpu.py, tests/test_softmax_census_gpu.py): inputs
whose float64 answer is exact by construction or well conditioned, and a bound for EVERY element of o, lse, dq, dk, dv that
is computed in float64 from the kernels' arithmetic -- no norm, no global tolerance.  CPU only, no import of the library.

Inputs (bf16, [B, H, L, hd]).  Q and K hold small integers, so every score q . k is exact in fp32.  Group g of n <= 16 has
the score column col(g) = g, the last group hd - 2 (inside the last 16-column K-slice; hd - 1, the last real column, carries
the shift / ladder factor).  V[k, :] is the one-hot of k % hd: V >= 0, so A = sum p |v| / sum p equals o and the forward
bound is sharp; an element no attended key feeds is an exact zero.

  hard      Q[q, col(g(q))] = -64, K[k, col(g)] = 64 (1 - M[g, k]) with M in {0, 1, 2}: a key of the row's set scores 0,
            every other key -G = -4096, a TRAP key (M = 2: masked for every row of the group) +G.  G scale log2e >= 522:
            P of a -G key, and every accumulator that is rescaled across it, is an exact zero whatever the hardware does
            with denormals (test_underflow_threshold).  lse = ln N(q) + T scale, o = the mean of V over the set.
  shifted   the same with Q[:, hd - 1] = t, K[:, hd - 1] = t': every score moves by T = t t', T scale log2e ~ +-30, +-120.
  ladder    Q[q, hd - 1] = t_q, K[k, hd - 1] = rung(k) in 0 .. 4: s = t_q rung(k); t_q scale log2e cycles through
            6, 7.5, 8.5, 10 inside a wave, so a rise of one rung per sub-block lies on both sides of LAZY_THR = 8 and the
            rows of one wave disagree about rescaling.  At most 4 rungs x 10 = 40 binades.
  g(q)      "mod": q % n (the rows of a wave differ);  "wave": q // 32 (whole waves agree; some never rescale);  under a
            token-major frame mask: (frame, wave), because the traps are the keys NO row of the group attends.
  dO        alternating signs, magnitude 1 or 2 by row, on 16 probe rows per head, zeros elsewhere; on every element with
            P > 0 of a probe row
            |dP - delta| >= 0.25 max |dP| or exactly 0 (probe_rows_ok), which keeps the cancellation out of the bound.

Bounds.  U = 2^-8: the relative error of a bf16 rounding at its worst, a value just above a power of two (the figure
2^-9 holds just below one; test_a_bf16_rounding_costs_up_to_2_to_the_minus_8 names an element of the ladder where the
emulation is off by 2^-7.65 A).  hulp(x) = 2^(floor(log2 |x|) - 8), bf16's half ulp at x.  F = 2^-23 (fp32).  Per row:
eps_s, the error of one score in the natural-log domain --
  plain   ln2 F (4 max|s c| + 20): the fp32 product s c, the subtraction of m (|m| <= max|s c| + 8) and v_exp_f32
  ones    + U scale max_k sum_i |q_i k_i|: Q' = bf16(Q scale log2e) is rounded once per element of Q
forward   |o - o_ref| <= (r_P + 2 eps_s + 16 F) A + hulp(A (1 + r_P + 2 eps_s + 16 F)): the bf16 P, numerator and
          denominator each off by eps_s, the bf16 store.  r_P = U on the plain path, where l is summed in fp32 from the
          unrounded e -- and 0 on a row whose live scores are all equal, because m is then that score and P = 1 exactly
          (the hard recipes: their bound is the half ulp of the store and the fp32 terms); r_P = 2 U on the ones path,
          whose denominator is a row of the O accumulator, summed from the bf16 P.
          |lse - lse_ref| <= eps_s + (Lk / 32 + 40) F + 2 ln2 F |lse log2e|  (+ U on the ones path, for that denominator)
backward  P = exp2(s c - lse log2e) is off by rel_p = expm1(eps_p), eps_p = the backward's own eps_s + the forward's lse
          bound (+ 2^-16 ln2 |lse log2e| where -lse log2e travels as a bf16 (hi, lo) pair);
          dV   sum_q P |dO| (U + rel_p (1 + U)) + U |dV_ref|          (bf16 P, bf16 store)
          delta is read from the bf16 o:  E_delta = sum_c |dO_c| E_o[c] (+ 2^-16 |delta| for its (hi, lo) pair)
          dS   P (1 + rel_p) E_delta + P |dP - delta| (rel_p + U (1 + rel_p))       (bf16 dS)
          dK   scale sum_q E_dS |Q| + U |dK_ref| (+ U scale sum_q |dS Q| where the operand was pre-scaled and rounded)
          dQ   the same with K.
An element whose bound is 0 must be an exact zero (the support check of the mask census, here from the scores)."""
import math

import torch

import attn_census as AC

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16
LOG2E, LN2 = AC.LOG2E, math.log(2.0)
U, F = 2.0 ** -8, 2.0 ** -23
A_GRP = 64  # |Q| and |K| of a group column: G = 4096
DEAD = 190.0  # binades below the row maximum from which a score counts as an exact zero
SHIFTS = (0, 30, -30, 120, -120)  # T scale log2e, about
LADDER_RISE = (6.0, 7.5, 8.5, 10.0)  # t_q scale log2e
PATTERNS = ("ascending", "descending", "spike_last", "spike_sub1", "sawtooth")
PROBES_PER_HEAD = 16


def col(g, n, hd):
    return hd - 2 if g == n - 1 else g


# ------------------------------------------------------------------------------- sets ----
def key_sets(n_valid):
    """the sets of the hard recipe over keys 0 .. n_valid - 1, clipped to them (an emptied set falls back to the last
    key): name -> sorted keys"""
    n = n_valid
    last_sub = 32 * ((n - 1) // 32)
    sets = {
        "first": [0],
        "last_valid": [n - 1],
        "straddle_sub": [31, 32],
        "straddle_tile": [63, 64],
        "three": sorted({0, n // 2, n - 1}),  # a size that is no power of two at every Lk: P = 1/3 is rounded
        "one_per_sub": [min(32 * j + (5 * j + 3) % 32, n - 1) for j in range((n + 31) // 32)],
        "last_sub": list(range(last_sub, n)),
        "all": list(range(n)),
        "pipe_sub1": list(range(32, 64)),  # sub-block 0 of the tile is all -G
        "pipe_sub0": list(range(64, 96)) if n > 96 else list(range(0, 32)),  # and the reverse
    }
    return {name: ([k for k in ks if k < n] or [n - 1]) for name, ks in sets.items()}


def group_of(Lq, n, assign):
    q = torch.arange(Lq)
    return q % n if assign == "mod" else (q // 32) % n


def set_matrix(mask, assign):
    """M int64 [B, n, Lk] for a bool mask [B, Lq, Lk] and g(q): 1 on the keys of group g's set -- a set of key_sets over
    the keys EVERY row of the group attends (if there is none: the first row's) --, 2 on its traps -- the keys NO row of
    the group attends --, else 0; and g [Lq].  assign: "mod", "wave", or g itself (token-major frame masks: the frame, since
    a wave of token-major rows holds every frame and so has no key that all its rows are denied)"""
    B, Lq, Lk = mask.shape
    names = list(key_sets(Lk))
    if torch.is_tensor(assign):
        g, n = assign, int(assign.max()) + 1
    else:
        n = len(names) if assign == "mod" else min(len(names), (Lq + 31) // 32)
        g = group_of(Lq, n, assign)
    M = torch.zeros(B, n, Lk, dtype=torch.long)
    for b in range(B):
        for i in range(n):
            rows = mask[b, g == i]
            common = rows.all(0).nonzero().flatten()
            if common.numel() == 0:  # (a window that moves inside the wave: the rows past it see -G on all their keys)
                common = rows[0].nonzero().flatten()
            picks = key_sets(common.numel())[names[(i + b) % len(names)]]
            M[b, i, common[picks]] = 1
            M[b, i, ~rows.any(0)] = 2
    return M, g


# ----------------------------------------------------------------------------- inputs ----
def shift_factors(hd, target):
    """t, t' with t t' scale log2e ~ target, both integers bf16 holds"""
    if target == 0:
        return 0, 0
    c = LOG2E / math.sqrt(hd)
    tp = 1 if abs(target) / c <= 256 else 8
    t = round(abs(target) / c / tp)
    assert t <= 256
    return int(math.copysign(t, target)), tp


def values(B, H, Lk, hd):
    v = torch.zeros(B, H, Lk, hd, dtype=bf16)
    v[:, :, torch.arange(Lk), torch.arange(Lk) % hd] = 1
    return v


def hard_inputs(hd, H, mask, assign, shift=0):
    """q, k, v of the hard recipe under mask [B, Lq, Lk] (all True: unmasked), shifted by T scale log2e ~ shift"""
    B, Lq, Lk = mask.shape
    M, g = set_matrix(mask, assign)
    n = M.shape[1]
    assert n <= 16 and n - 1 <= hd - 3
    cols = torch.tensor([col(i, n, hd) for i in range(n)])
    q = torch.zeros(B, H, Lq, hd, dtype=bf16)
    k = torch.zeros(B, H, Lk, hd, dtype=bf16)
    q[:, :, torch.arange(Lq), cols[g]] = -A_GRP
    k[:, :, :, cols] = (A_GRP * (1 - M)).to(bf16).transpose(1, 2)[:, None]
    t, tp = shift_factors(hd, shift)
    q[..., hd - 1] = t
    k[..., hd - 1] = tp
    return q, k, values(B, H, Lk, hd)


def rungs(pattern, Lk, n_valid):
    k = torch.arange(Lk)
    if pattern == "ascending":
        return (k // 32).clamp(max=4)
    if pattern == "descending":
        return (4 - k // 32).clamp(min=0)
    if pattern == "spike_last":
        return (k == n_valid - 1).long()  # one rung: rows at 6 and 7.5 keep P up to 2^7.5, rows at 8.5 and 10 rescale
    if pattern == "spike_sub1":
        return (k == min(40, n_valid - 1)).long()
    return (k // 32) % 3  # sawtooth over sub-blocks: 0, 1, 2, 0, ..


def ladder_inputs(hd, B, H, Lq, Lk):
    """q, k, v of the ladder recipe: head i runs PATTERNS[i % 5]; t_q differs between the rows of a wave and between
    rows q and q + 32"""
    c = LOG2E / math.sqrt(hd)
    ts = torch.tensor([round(x / c) for x in LADDER_RISE])
    q = torch.zeros(B, H, Lq, hd, dtype=bf16)
    k = torch.zeros(B, H, Lk, hd, dtype=bf16)
    rows = torch.arange(Lq)
    q[..., hd - 1] = ts[(rows + rows // 32) % 4].to(bf16)
    for i in range(B * H):
        k[i // H, i % H, :, hd - 1] = rungs(PATTERNS[i % len(PATTERNS)], Lk, Lk).to(bf16)
    return q, k, values(B, H, Lk, hd)


def grad_pattern(hd, q):
    """dO[q, :]: alternating signs, magnitude 1 on even rows and 2 on odd ones"""
    return ((1 - 2 * (torch.arange(hd) % 2)) * (1 + q % 2)).to(f64)


def probe_do(q, k, v, mask):
    """dO [B, H, Lq, hd] bf16: grad_pattern on up to PROBES_PER_HEAD rows per head, taken in attn_census.probe_order (one per
    group and wave before a second of any) from the rows on which |dP - delta| >= 0.25 max |dP| (or exactly 0) holds
    wherever P > 0; and the number of probe rows"""
    B, H, Lq, hd = q.shape
    ref = expect(q, k, v, None, mask)
    order = AC.probe_order(Lq)
    full = torch.stack([grad_pattern(hd, r) for r in range(Lq)])  # [Lq, hd]
    dP = full[None, None] @ v.to(f64).transpose(-1, -2)  # [B, H, Lq, Lk]
    delta = (ref["p"] * dP).sum(-1, keepdim=True)
    gap = (dP - delta).abs()
    ok = ((gap >= 0.25 * dP.abs().amax(-1, keepdim=True)) | (gap < 1e-12) | (ref["p"] == 0)).all(-1)  # [B, H, Lq]
    do = torch.zeros(B, H, Lq, hd, dtype=bf16)
    count = 0
    kind = torch.unique(q[0, 0].float(), dim=0, return_inverse=True)[1] * 64 + torch.arange(Lq) // 32  # (row of Q, wave)
    for b in range(B):
        for h in range(H):
            start = (b * H + h) * PROBES_PER_HEAD  # another stretch of the edge list in every head
            rot = [r for r in order[start % Lq:] + order[:start % Lq] if ok[b, h, r]]
            rows, seen = [], set()
            for r in rot:  # rows of distinct (group or t_q, wave) first, so a head's probes spread over the sets
                if int(kind[r]) not in seen and len(rows) < PROBES_PER_HEAD:
                    seen.add(int(kind[r]))
                    rows.append(r)
            rows += [r for r in rot if r not in rows][:PROBES_PER_HEAD - len(rows)]
            do[b, h, rows] = full[rows].to(bf16)
            count += len(rows)
    return do, count


def probe_rows_ok(q, k, v, do, mask):
    """the floor of the backward bound on the inputs themselves: on every probe row, wherever P > 0"""
    ref = expect(q, k, v, do, mask)
    probe = (do != 0).any(-1)
    gap = (ref["dP"] - ref["delta"][..., None]).abs()
    floor = 0.25 * ref["dP"].abs().amax(-1, keepdim=True)
    return bool((((gap >= floor) | (gap < 1e-12) | (ref["p"] == 0)) | ~probe[..., None]).all())


# ----------------------------------------------------------------------- expectations ----
def expect(q, k, v, do, mask):
    """float64 attention on the bf16 inputs under mask [B, Lq, Lk]: dict of o, lse, p, s2 (scores in the log2 domain),
    absqk (sum_i |q_i k_i| scale) and, with do: dq, dk, dv, dP, delta, ds.  A score more than DEAD binades under its
    row's maximum has P = 0 exactly (the kernels' fp32 exp2 gives that; test_underflow_threshold keeps every score of
    the hard recipes out of the band between); a row that attends nothing gives zeros."""
    hd = q.shape[-1]
    scale = 1.0 / math.sqrt(hd)
    qd, kd, vd = q.to(f64), k.to(f64), v.to(f64)
    m4 = mask[:, None]
    s = (qd @ kd.transpose(-1, -2)) * scale
    sm = s.masked_fill(~m4, float("-inf"))
    mx = sm.amax(-1, keepdim=True)
    some = torch.isfinite(mx)
    mx = torch.where(some, mx, torch.zeros((), dtype=f64))
    e = torch.where(m4 & ((mx - s) * LOG2E <= DEAD), (s - mx).exp(), torch.zeros((), dtype=f64))
    l = e.sum(-1, keepdim=True)
    p = e / l.clamp(min=1e-300)
    out = {"p": p, "s2": s * LOG2E, "o": p @ vd, "absqk": (qd.abs() @ kd.abs().transpose(-1, -2)) * scale,
           "lse": torch.where(some, mx + l.clamp(min=1e-300).log(), torch.zeros((), dtype=f64)).squeeze(-1)}
    if do is not None:
        dod = do.to(f64)
        dP = dod @ vd.transpose(-1, -2)
        delta = (p * dP).sum(-1)
        ds = p * (dP - delta[..., None])
        out.update(dP=dP, delta=delta, ds=ds, dv=p.transpose(-1, -2) @ dod, dk=(ds.transpose(-1, -2) @ qd) * scale,
                   dq=(ds @ kd) * scale)
    return out


# ----------------------------------------------------------------------------- bounds ----
def _eps_s(ref, ones):
    """[B, H, Lq, 1]: the error of one score of the row in the natural-log domain, over the keys with P > 0"""
    alive = ref["p"] > 0
    smax = torch.where(alive, ref["s2"].abs(), torch.zeros((), dtype=f64)).amax(-1, keepdim=True)
    eps = LN2 * F * (4 * smax + 20)
    if ones:
        eps = eps + U * torch.where(alive, ref["absqk"], torch.zeros((), dtype=f64)).amax(-1, keepdim=True)
    return eps


def hulp(x):
    """bf16's half ulp at x (float64 tensor, x > 0 where it matters)"""
    return torch.where(x > 0, torch.exp2(torch.floor(torch.log2(x.clamp(min=1e-300))) - 8), torch.zeros((), dtype=f64))


def forward_bounds(ref, ones=False):
    """(E_o [B, H, Lq, hd], E_lse [B, H, Lq]) for a forward on the plain (lazy_softmax) or the ones path"""
    eps = _eps_s(ref, ones)
    Lk = ref["p"].shape[-1]
    alive = ref["p"] > 0
    inf = torch.tensor(float("inf"), dtype=f64)
    top, low = torch.where(alive, ref["s2"], -inf).amax(-1, keepdim=True), torch.where(alive, ref["s2"], inf).amin(-1, keepdim=True)
    flat = top == low  # every live score of the row is the same
    r_p = 2 * U if ones else torch.where(flat, torch.zeros((), dtype=f64), torch.tensor(U, dtype=f64))
    rel = r_p + 2 * eps + 16 * F
    a = ref["o"].abs()
    e_o = rel * a + hulp(a * (1 + rel))
    e_lse = eps.squeeze(-1) + (Lk / 32 + 40) * F + 2 * LN2 * F * (ref["lse"] * LOG2E).abs() + (U if ones else 0.0)
    return e_o, e_lse


def backward_bounds(ref, q, k, do, fwd_ones=False, bwd_ones=False):
    """(E_dq, E_dk, E_dv) for a backward on the plain or the ones route, after a forward on either path"""
    hd = q.shape[-1]
    scale = 1.0 / math.sqrt(hd)
    e_o, e_lse = forward_bounds(ref, fwd_ones)
    p, dod = ref["p"], do.to(f64).abs()
    alive = p > 0
    eps_p = LN2 * F * (2 * ref["s2"].abs() + 2 * (ref["lse"] * LOG2E).abs()[..., None] + 2) + e_lse[..., None]
    if bwd_ones:
        eps_p = eps_p + U * ref["absqk"] + 2.0 ** -16 * LN2 * (ref["lse"] * LOG2E).abs()[..., None]
    rel_p = torch.where(alive, torch.expm1(eps_p), torch.zeros((), dtype=f64))
    e_dv = (p * (U + rel_p * (1 + U))).transpose(-1, -2) @ dod + U * ref["dv"].abs()
    e_delta = (dod * e_o).sum(-1) + 8 * F * (dod * ref["o"].abs()).sum(-1)
    if bwd_ones:
        e_delta = e_delta + 2.0 ** -16 * ref["delta"].abs()
    gap = (ref["dP"] - ref["delta"][..., None]).abs()
    e_ds = p * (1 + rel_p) * e_delta[..., None] + p * gap * (rel_p + U * (1 + rel_p))
    pre = U if bwd_ones else 0.0
    qa, ka = q.to(f64).abs(), k.to(f64).abs()
    e_dk = scale * ((e_ds + pre * ref["ds"].abs()).transpose(-1, -2) @ qa) + U * ref["dk"].abs()
    e_dq = scale * ((e_ds + pre * ref["ds"].abs()) @ ka) + U * ref["dq"].abs()
    return e_dq, e_dk, e_dv


# --------------------------------------------------------------------------- checkers ----
def check(tag, got, ref, bound):
    """every element of got within bound of the float64 ref (a bound of 0: an exact zero).  Returns the worst
    error / bound over the elements with a bound."""
    g = got.to(f64)
    assert g.shape == ref.shape == bound.shape, (tag, g.shape, ref.shape, bound.shape)
    if not torch.isfinite(g).all():
        raise AssertionError(f"{tag}{list(AC._first(~torch.isfinite(g)))} unwritten or not finite")
    err = (g - ref).abs()
    bad = err > bound
    if bad.any():
        i = AC._first(bad)
        raise AssertionError(f"{tag}{list(i)} = {g[i].item():.6g}, expected {ref[i].item():.6g}: error "
                             f"{err[i].item():.3e} > bound {bound[i].item():.3e}"
                             + (" (must be an exact zero)" if bound[i] == 0 else ""))
    has = bound > 0
    return (err[has] / bound[has]).max().item() if has.any() else 0.0


def census(tag, run, q, k, v, do, mask, fwd_ones=False, bwd_ones=False):
    """one case on run(q, k, v, do) -> o, lse[, dq, dk, dv]: every element of every output.  Returns the worst
    error / bound per output."""
    ref = expect(q, k, v, do, mask)
    out = run(q, k, v, do)
    e_o, e_lse = forward_bounds(ref, fwd_ones)
    worst = {"lse": check(tag + ".lse", out[1], ref["lse"], e_lse), "o": check(tag + ".o", out[0], ref["o"], e_o)}
    if do is not None:
        bounds = backward_bounds(ref, q, k, do, fwd_ones, bwd_ones)
        for name, got, e in zip(("dq", "dk", "dv"), out[2:], bounds):
            worst[name] = check(f"{tag}.{name}", got, ref[name], e)
    return worst
