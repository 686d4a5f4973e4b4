"""Exact census of the optimizer kernels (csrc/optim.hip, csrc/muon.hip): inputs, float64 expectations, loop predicates.

AdamW, the sum of squares with its finalize, and Muon's momentum, normalise, Newton-Schulz tile GEMM and update, pinned
element by element as edge_census.py pins the step-edge kernels.  Everything here runs on the CPU with torch alone; the
GPU test compares bits.  A builder never skips a case: it ASSERTS the property that makes its comparison legitimate and
raises otherwise.

AdamW, exact recipe.  betas (1/2, 3/4), eps 2^-6, step 1: bc1 = 1/2 and 1 / sqrt(bc2) = 2 exactly.  Per element
s = (2^j - eps) / 2, j in {-1, 0, 1, 2}; the scaled gradient is +-q s and v0 = c s^2 with (q, c) one of RECIPE_QC, so
that 3/4 c + 1/4 q^2 = 1: v' = s^2, sqrt(v') = s, the denominator 2 s + eps = 2^j.  m0 is a multiple of 1/8, p0 of
2^-10 up to 4, the EMA of 1/16 up to 1, every scalar dyadic.  `adamw_expect` walks the kernel's chain in float64 and asserts
after EVERY operation that the value is an fp32 number: contraction into fmas then changes nothing and p, m, v, the
shadow bf16(p) and the EMA have ONE right answer each.

Sum of squares.  g in +-{1/2, 1, 2}: every square is a multiple of 1/4 and `exact_fit` asserts that the whole table
sums below 2^24 of them: every partial and the total are exact in any order.

guard_finalize is restated operation by operation in fp32 (sqrt, add, divide, compare: each correctly rounded, and no
product feeds a sum, so there is no fma to form).

Muon.  Momentum: g' in +-{1, 2}, buf in {-4, 0, 4}, mu in {1/2, 3/4}: buf, u and every partial of sum u^2 are exact
(asserted).  Normalise: inv = 1 / (sqrt(sumsq) + 1e-7) and bf16(fp32(u inv)) restated in fp32.  The Newton-Schulz
iteration: u in {0, +-1}, sumsq = 16 written by the test so that X = u / 4 exactly; each of the three products is
expected in float64 from the GPU's OWN stored operand of the product before it, every operand itself pinned.  An
element is compared when the magnitudes of its addends sum below 2^24 granules (the fp32 sum is then exact in any
order, whatever the MFMA's internal order is) and when the epilogue alpha acc + beta add rounds to the same bf16
whichever way the compiler contracts it (three forms: none, fma(beta, add, fl(alpha acc)), fma(alpha, acc,
fl(beta add))).  The share of the other elements is capped at UNDECIDED_CAP = 1 % per product and recipe.  Update: dyadic
scalars and a dyadic O make p', the shadow and the EMA exact; at [328, 200] the scale sqrt(328 / 200) is inexact and
p' must be one of the two fp32 results (contracted or not).
"""
import functools
import math
from collections import namedtuple

import torch

import edge_census as E
import gemm_census as G
import row_census as R

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
bits = G.bits
exact_fit, multiples = E.exact_fit, E.multiples
UNDECIDED_CAP = E.UNDECIDED_CAP
FLT_MAX = 3.4028234663852886e38


def gen(*key):
    return R._gen(*key)


def sqrt32(x32):
    """the correctly rounded fp32 square root / quotient, through float64 (53 >= 2 x 24 + 2 bits: the second rounding is
    innocuous).  torch's own fp32 sqrt is NOT correctly rounded on every CPU: one ulp off was seen"""
    return torch.sqrt(x32.to(f64)).to(f32)


def div32(a32, b32):
    return (a32.to(f64) / b32.to(f64)).to(f32)


def f32v(x):
    """the fp32 number nearest a Python float, as a Python float"""
    return float(torch.tensor(x, dtype=f32))


# ==== AdamW: the loops of adamw_kernel and grad_sumsq_partial_kernel, restated ==========================================
def walk(extent, vec_ok, unroll):
    """the two loops of a 256-thread workgroup over a chunk of `extent` elements -> (touch count per element, vector
    trips per thread [256], elements of every tail visit as a list of lengths).  unroll 2: adamw_kernel, 4: the sum"""
    touched = [0] * extent
    trips, tails = [0] * 256, []
    for tid in range(256):
        i = tid * 4
        if vec_ok:
            while i + (unroll - 1) * 1024 + 4 <= extent:
                for u in range(unroll):
                    for e in range(4):
                        touched[i + u * 1024 + e] += 1
                trips[tid] += 1
                i += unroll * 1024
        while i < extent:
            n = min(extent, i + 4) - i
            tails.append(n)
            for e in range(n):
                touched[i + e] += 1
            i += 1024
    return touched, trips, tails


def chunk_list(numel, chunk_elems):
    return list(range(0, numel, chunk_elems))


def vec_rule(byte_offsets, s0, shadow_off=None):
    """the 16-byte path of a chunk that starts at element s0: every fp32 stream on a 16-byte boundary there, the shadow
    (bf16) on an 8-byte one.  byte_offsets: displacement of every fp32 base from a 16-byte boundary (absent streams left
    out)"""
    ok = all((b + 4 * s0) % 16 == 0 for b in byte_offsets)
    return ok and (shadow_off is None or (shadow_off + 2 * s0) % 8 == 0)


# ---- the exact recipe ------------------------------------------------------------------------------------------------
BETA1, BETA2, EPS_X = 0.5, 0.75, 2.0 ** -6
RECIPE_QC = ((2.0, 0.0), (1.0, 1.0), (0.5, 1.25), (0.25, 21.0 / 16.0), (1.25, 13.0 / 16.0), (1.75, 5.0 / 16.0))
# (lr, wd) per descriptor, all different
LR_WD = tuple((2.0 ** -a, w) for a in (3, 4, 5, 6) for w in (0.25, 0.5, 0.0, 0.125, 0.0625))
# (lr_mult, grad_scale, ema decay)
SETTINGS = ((1.0, 1.0, 0.5), (0.5, 2.0, 0.75), (0.25, 0.5, 0.5))
EXTENTS = (1, 3, 4, 5, 1023, 1024, 1025, 2044, 2047, 2048, 2049, 3076, 4096, 4097, 65536 + 5)
CHUNK_ELEMS = (4, 1028, 1030, 2048, 65536)
STREAMS = ("p", "g", "m", "v", "pb", "ema")

Tensor = namedtuple("Tensor", "numel lr wd shadow ema off")      # off: {stream: displacement in ELEMENTS}
Case = namedtuple("Case", "name tensors chunk_elems order form setting coef skipped table_ema")


def tensor(numel, i, shadow=True, ema=True, off=None):
    lr, wd = LR_WD[i % len(LR_WD)]
    return Tensor(numel, lr, wd, shadow, ema, dict(off or {}))


def adamw_cases():
    """every launch of the exact census (issue section 1); form in multi | multi_dev | guarded | guarded_dev"""
    cases = []
    ext = [tensor(n, i, shadow=i % 4 != 3, ema=i % 3 != 2) for i, n in enumerate(EXTENTS)]
    for form in ("multi", "multi_dev", "guarded", "guarded_dev"):
        cases.append(Case(f"extents/{form}", ext, 65536, "forward", form, SETTINGS[len(cases) % 3], 0.5 if "guarded" in form else 1.0,
                          0, True))
    lens = {4: (1, 3, 4, 5, 23, 8), 1028: (1028, 2049, 4097 + 1028, 1, 2056), 1030: (5000, 1030, 2061, 7, 3090),
            2048: (4096 + 5, 2048, 2047, 6144, 3)}
    for j, (ce, ns) in enumerate(lens.items()):
        ts = [tensor(n, i + j, shadow=i != 1, ema=i != 2) for i, n in enumerate(ns)]
        cases.append(Case(f"chunk{ce}/multi", ts, ce, "shuffled", "multi", SETTINGS[j % 3], 1.0, 0, True))
        cases.append(Case(f"chunk{ce}/guarded", ts, ce, "reversed", "guarded", SETTINGS[(j + 1) % 3], 1.0 if j % 2 else 0.5, 0, True))
    for k, s in enumerate(STREAMS):     # one stream alone off its boundary: 4 bytes (fp32), 2 bytes (the shadow)
        ts = [tensor(4097, k, off={s: 1}), tensor(2048, k + 1), tensor(2049, k + 2, off={s: 3 if s != "pb" else 1})]
        cases.append(Case(f"misaligned_{s}/guarded", ts, 65536, "forward", "guarded", SETTINGS[k % 3], 1.0, 0, True))
        if s != "ema":
            cases.append(Case(f"misaligned_{s}/multi", ts, 65536, "forward", "multi", SETTINGS[(k + 1) % 3], 1.0, 0, True))
    five = [tensor(n, i) for i, n in enumerate((2049, 5, 4100, 1024, 3077, 4096))]
    cases.append(Case("no_ema_table/guarded", five, 2048, "shuffled", "guarded", SETTINGS[0], 1.0, 0, False))
    cases.append(Case("no_ema_table/guarded_dev", five, 2048, "shuffled", "guarded_dev", SETTINGS[1], 0.5, 0, False))
    cases.append(Case("no_shadow_at_all/multi_dev", [t._replace(shadow=False) for t in five], 65536, "reversed", "multi_dev", SETTINGS[2],
                      1.0, 0, True))
    cases.append(Case("skipped/guarded", five, 2048, "forward", "guarded", SETTINGS[0], 0.5, 1, True))
    cases.append(Case("skipped/guarded_dev", five, 65536, "forward", "guarded_dev", SETTINGS[1], 1.0, 1, True))
    cases.append(Case("no_chunks/multi", five, 2048, "none", "multi", SETTINGS[0], 1.0, 0, True))
    cases.append(Case("no_chunks/guarded", five, 2048, "none", "guarded", SETTINGS[0], 1.0, 0, True))
    return cases


def chunk_table(case):
    """(chunk_tensor, chunk_start) in the case's order"""
    pairs = [(i, s) for i, t in enumerate(case.tensors) for s in chunk_list(t.numel, case.chunk_elems)]
    if case.order == "none":
        return [], []
    if case.order == "reversed":
        pairs = pairs[::-1]
    elif case.order == "shuffled":
        perm = torch.randperm(len(pairs), generator=gen(len(pairs), 3)).tolist()
        pairs = [pairs[k] for k in perm]
        assert len(pairs) < 3 or pairs != sorted(pairs)
    return [p[0] for p in pairs], [p[1] for p in pairs]


def has_ema(case, t):
    return "guarded" in case.form and case.table_ema and t.ema


def chunk_vec_ok(case, t, s0):
    """vec_ok of adamw_kernel for the chunk of tensor t that starts at s0 (bases 16-byte aligned + the displacement)"""
    streams = ["p", "g", "m", "v"] + (["ema"] if has_ema(case, t) else [])
    return vec_rule([4 * t.off.get(s, 0) for s in streams], s0, 2 * t.off.get("pb", 0) if t.shadow else None)


Adam = namedtuple("Adam", "p0 g m0 v0 ema0 p m v pb ema distinct inexact_bf16")


@functools.lru_cache(maxsize=64)
def _adamw_data(numel, lr, wd, setting, coef, seed):
    lr_mult, grad_scale, decay_ema = setting
    g_ = gen(numel, seed, int(lr * 2 ** 12), 101)
    what = f"adamw n {numel} lr {lr} wd {wd} setting {setting} coef {coef}"
    j = torch.randint(-1, 3, (numel,), generator=g_).to(f64)
    s = (2.0 ** j - EPS_X) / 2.0
    k = torch.randint(0, len(RECIPE_QC), (numel,), generator=g_)
    q = torch.tensor([a for a, _ in RECIPE_QC], dtype=f64)[k]
    c = torch.tensor([b for _, b in RECIPE_QC], dtype=f64)[k]
    sg = E.signs((numel,), g_)
    gs = grad_scale * coef                                   # grad_scale *= guard->coef: dyadic, exact
    g = R.assert_f32(what + " g", sg * q * s / gs).to(f64)
    assert (g != 0).all()
    m0 = R.ints((numel,), -32, 32, g_) / 8.0
    v0 = R.assert_f32(what + " v0", c * s * s).to(f64)
    p0 = R.ints((numel,), -4096, 4096, g_) / 1024.0
    ema0 = R.ints((numel,), -16, 16, g_) / 16.0
    A = lambda name, t: R.assert_f32(f"{what} {name}", t).to(f64)   # noqa: E731
    # the chain of adamw_kernel, one fp32 check per operation
    lr_e = A("lr", torch.tensor(lr * lr_mult, dtype=f64))
    dec = A("decay", 1.0 - A("lr wd", lr_e * wd))
    bc1, rs = 1.0 - BETA1, 1.0 / math.sqrt(1.0 - BETA2)
    assert bc1 == 0.5 and rs == 2.0
    step = A("step_size", lr_e / bc1)
    gg = A("gg", g * gs)
    pd = A("p decay", p0 * dec)
    m = A("m", A("b1 m", BETA1 * m0) + A("(1 - b1) gg", (1.0 - BETA1) * gg))
    v = A("v", A("b2 v", BETA2 * v0) + A("(1 - b2) gg gg", A("(1 - b2) gg", (1.0 - BETA2) * gg) * gg))
    assert torch.equal(v, s * s)
    root = A("sqrt v", torch.sqrt(v))
    assert torch.equal(root, s)
    den = A("denom", A("sqrt rs", root * rs) + EPS_X)
    assert torch.equal(den, 2.0 ** j)
    p = A("p'", pd - A("step m / denom", step * A("m / denom", m / den)))
    ema = A("ema'", A("d ema", decay_ema * ema0) + A("(1 - d) p", (1.0 - decay_ema) * p))
    pb = p.to(f32).to(bf16)
    assert not torch.equal(p, p0) or numel < 4
    return Adam(p0.to(f32), g.to(f32), m0.to(f32), v0.to(f32), ema0.to(f32), p.to(f32), m.to(f32), v.to(f32), pb, ema.to(f32),
                len(set(p.tolist())), float((pb.to(f64) != p).double().mean()))


def adamw_expect(case, i):
    """inputs and the one right answer of tensor i of a case"""
    t = case.tensors[i]
    return _adamw_data(t.numel, t.lr, t.wd, case.setting, case.coef, i)


def adamw_coverage():
    """edge -> cases that reach it, from the restated loops"""
    cov = {k: [] for k in ("vector trips 0", "vector trips 1", "vector trips 2", "threads of one chunk leave at different trips",
                           "tail of 1", "tail of 2", "tail of 3", "tail of 4", "chunk off the 16-byte grid (scalar path)",
                           "several chunks, the last short", "shadow NULL", "ema entry NULL", "ema table NULL",
                           "chunks out of tensor order", "n_chunks 0", "skipped", "coef 1/2", "five tensors or more")}
    for s in STREAMS:
        cov[f"{s} alone displaced"] = []
    for case in adamw_cases():
        ct, cs = chunk_table(case)
        if not ct:
            cov["n_chunks 0"].append(case.name)
        if len(case.tensors) >= 5:
            cov["five tensors or more"].append(case.name)
        if ct and list(zip(ct, cs)) != sorted(zip(ct, cs)):
            cov["chunks out of tensor order"].append(case.name)
        if case.skipped:
            cov["skipped"].append(case.name)
        if case.coef == 0.5 and "guarded" in case.form:
            cov["coef 1/2"].append(case.name)
        if "guarded" in case.form and not case.table_ema:
            cov["ema table NULL"].append(case.name)
        for i, s0 in zip(ct, cs):
            t = case.tensors[i]
            extent = min(t.numel, s0 + case.chunk_elems) - s0
            ok = chunk_vec_ok(case, t, s0)
            touched, trips, tails = walk(extent, ok, 2)
            assert set(touched) == {1}, f"{case.name}: the restated loop does not touch every element once"
            if ok:
                for n in set(trips):
                    if n <= 2:
                        cov[f"vector trips {n}"].append((case.name, extent))
                if len(set(trips)) > 1:
                    cov["threads of one chunk leave at different trips"].append((case.name, extent))
            elif not t.off and s0:
                cov["chunk off the 16-byte grid (scalar path)"].append((case.name, s0))
            for n in set(tails):
                cov[f"tail of {n}"].append((case.name, extent))
            if s0 and extent < case.chunk_elems:
                cov["several chunks, the last short"].append((case.name, t.numel))
            if not t.shadow:
                cov["shadow NULL"].append(case.name)
            if "guarded" in case.form and case.table_ema and not t.ema:
                cov["ema entry NULL"].append(case.name)
            for s in STREAMS:
                if set(t.off) == {s} and not ok and (s != "ema" or has_ema(case, t)) and (s != "pb" or t.shadow):
                    cov[f"{s} alone displaced"].append(case.name)
    return {k: sorted(set(map(str, v))) for k, v in cov.items()}


# ---- the real constants: per-element bound -------------------------------------------------------------------------------
# |got - want| <= c 2^-24 sum|addends| per element, c counted from the chain of adamw_kernel.  One unit = 2^-24 relative,
# the rounding of one fp32 operation (half an ulp); sqrt and the division are given TWO units (a whole ulp) so that the
# bound does not rest on their being correctly rounded.  A contraction into an fma only removes a rounding.
#   gg = g gs                                 1 unit
#   m' = b1 m + (1 - b1) gg                   addend b1 m: its product and the sum, 2; addend (1 - b1) gg: gg, its product
#                                             and the sum, 3                                               C_M = 3
#   v' = b2 v + (1 - b2) gg gg                addend b2 v: 2; the other: gg twice, two products, the sum, 5   C_V = 5
#   denom = sqrt(v') rs + eps                 v' has 5 (its addends are positive: the bound is relative), the root halves
#                                             them, 2.5, + 2 for the root + 1 product + 1 sum: 6.5, relative to denom
#   q = m' / denom                            3 of S_m = |b1 m| + |(1 - b1) gg| from m', 6.5 + 2 of |m'| <= S_m: 11.5
#   upd = step_size q                         12.5
#   p' = p decay - upd                        addend p decay: its product and the sum, 2; addend upd: 12.5 + the sum,
#                                             13.5, of step_size S_m / denom                               C_P = 14
#   ema' = d ema + (1 - d) p'                 addend d ema: 2; (1 - d) p': C_P through p' + product + sum  C_EMA = 16
# with the addends of p' taken as |p decay| and step_size S_m / denom, those of ema' as |d ema|, (1 - d) |p decay| and
# (1 - d) step_size S_m / denom.  Second-order terms (products of two roundings, 2^-48) are covered by rounding 13.5 up.
C_M, C_V, C_P, C_EMA = 3.0, 5.0, 14.0, 16.0
REAL_BETAS, REAL_EPS = (0.95, 0.99), 1e-8
REAL_STEPS = (1, 7)
REAL_NUMELS = (4097, 1025, 65536 + 5)
Real = namedtuple("Real", "p0 g m0 v0 ema0 p m v ema bp bm bv bema sp sm sv sema margin")


def host_scalars(beta1, beta2, step):
    """(bc1, 1 / sqrt(bc2)) as vds_adamw_multi forms them: 1 - powf(beta, step) and 1.0f / sqrtf(bc2), the C library's powf"""
    import ctypes
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.powf.restype, libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    t = lambda x: torch.tensor(x, dtype=f32)   # noqa: E731
    bc1 = t(1.0) - t(libm.powf(beta1, float(step)))
    bc2 = t(1.0) - t(libm.powf(beta2, float(step)))
    return float(bc1), float(div32(t(1.0), sqrt32(bc2)))


@functools.lru_cache(maxsize=32)
def adamw_real(numel, step, lr, wd, lr_mult, grad_scale, coef, d, seed):
    """Gaussian inputs, float64 expectation from the scalars at the fp32 values the kernel holds, per-element bounds.
    m0 and g share their sign and stay away from zero, so that m' does not cancel: the smallest update must exceed four
    times the bound of its element (asserted), a dropped or doubled update cannot hide"""
    g_ = gen(numel, step, seed, 113)
    t = lambda x: torch.tensor(x, dtype=f32)   # noqa: E731
    sg = E.signs((numel,), g_)
    mag = lambda sc: (torch.randn(numel, generator=g_, dtype=f64).abs() * sc + 0.05 * sc)   # noqa: E731
    g = (sg * mag(0.3)).to(f32)
    m0 = (sg * mag(0.1)).to(f32)
    v0 = (mag(0.3) ** 2).to(f32)
    p0 = (torch.randn(numel, generator=g_, dtype=f64) * 0.05).to(f32)       # the scale of the model's weights
    ema0 = (torch.randn(numel, generator=g_, dtype=f64) * 0.05).to(f32)
    b1, b2, eps = t(REAL_BETAS[0]), t(REAL_BETAS[1]), t(REAL_EPS)
    bc1, rs = host_scalars(REAL_BETAS[0], REAL_BETAS[1], step)
    gs = t(grad_scale) * t(coef)
    lr_e = t(lr) * t(lr_mult)
    dec = t(1.0) - lr_e * t(wd)
    step_size = div32(lr_e, t(bc1))
    omb1, omb2, omd = t(1.0) - b1, t(1.0) - b2, t(1.0) - t(d)
    D = lambda x: x.to(f64)   # noqa: E731
    gg = D(g) * D(gs)
    a_m = (D(b1) * D(m0), D(omb1) * gg)
    m = a_m[0] + a_m[1]
    s_m = a_m[0].abs() + a_m[1].abs()
    a_v = (D(b2) * D(v0), D(omb2) * gg * gg)
    v = a_v[0] + a_v[1]
    den = torch.sqrt(v) * rs + D(eps)
    pd = D(p0) * D(dec)
    upd = D(step_size) * (m / den)
    p = pd - upd
    s_p = pd.abs() + D(step_size) * s_m / den
    ema = D(t(d)) * D(ema0) + D(omd) * p
    s_e = (D(t(d)) * D(ema0)).abs() + D(omd) * s_p
    bp, bm, bv, be = (c * E.U24 * s for c, s in ((C_P, s_p), (C_M, s_m), (C_V, v), (C_EMA, s_e)))
    margin = float((upd.abs() / (4.0 * bp)).min())
    assert margin > 1.0, f"adamw_real n {numel} step {step}: smallest update only {margin:.2f} x 4 x the bound"
    return Real(p0, g, m0, v0, ema0, p, m, v, ema, bp, bm, bv, be, s_p, s_m, v, s_e, margin)


# ==== sum of squares ==================================================================================================
SUMSQ_VALUES = (0.5, 1.0, 2.0)
SumsqCase = namedtuple("SumsqCase", "name numels offs chunk_elems")


def sumsq_cases():
    cases = [SumsqCase("extents", EXTENTS + (8191, 8192, 8193, 4099), (0,) * 19, 65536),
             SumsqCase("chunk4_275_chunks", (1100, 3, 5), (0, 0, 0), 4)]
    for ce in (1028, 1030, 2048, 4096):
        cases.append(SumsqCase(f"chunk{ce}", (ce * 3 + 5, ce, 4097, 1), (0, 0, 0, 0), ce))
    cases.append(SumsqCase("misaligned", (8193, 4096, 4100, 5), (1, 0, 3, 2), 65536))
    return cases


def sumsq_stage2_trips(n_chunks):
    return (n_chunks + 255) // 256


@functools.lru_cache(maxsize=None)
def sumsq_expect(name):
    """-> (gradients per tensor, chunk_tensor, chunk_start, fp32 partials, fp32 total): exact in any order"""
    case = {c.name: c for c in sumsq_cases()}[name]
    g_ = gen(len(case.numels), case.chunk_elems, 103)
    gs = [E.signs((n,), g_) * R.pick(SUMSQ_VALUES, (n,), g_) for n in case.numels]
    assert all((g != 0).all() for g in gs)
    ct = [i for i, n in enumerate(case.numels) for _ in chunk_list(n, case.chunk_elems)]
    cs = [s for n in case.numels for s in chunk_list(n, case.chunk_elems)]
    parts = torch.stack([(gs[i][s:s + case.chunk_elems] ** 2).sum() for i, s in zip(ct, cs)])
    multiples(name + " squares", torch.cat(gs) ** 2, 0.25)
    exact_fit(name + " sumsq", parts.sum().reshape(1), 0.25)
    assert len(set(parts.tolist())) > min(3, len(ct) - 1), "the partials must differ"
    return [g.to(f32) for g in gs], ct, cs, R.assert_f32(name + " partials", parts), R.assert_f32(name + " total", parts.sum().reshape(1))


def sumsq_coverage():
    cov = {k: [] for k in ("vector trips 0", "vector trips 1", "vector trips 2", "tail of 1", "tail of 2", "tail of 3", "tail of 4",
                           "g off its boundary", "chunk off the 16-byte grid", "stage 2: one trip", "stage 2: two trips")}
    for case in sumsq_cases():
        _, ct, cs, _, _ = sumsq_expect(case.name)
        cov["stage 2: one trip" if sumsq_stage2_trips(len(ct)) == 1 else "stage 2: two trips"].append(case.name)
        for i, s0 in zip(ct, cs):
            extent = min(case.numels[i], s0 + case.chunk_elems) - s0
            ok = vec_rule([4 * case.offs[i]], s0)
            touched, trips, tails = walk(extent, ok, 4)
            assert set(touched) == {1}
            if ok:
                for n in set(trips):
                    if n <= 2:
                        cov[f"vector trips {n}"].append((case.name, extent))
            elif case.offs[i]:
                cov["g off its boundary"].append(case.name)
            else:
                cov["chunk off the 16-byte grid"].append((case.name, s0))
            for n in set(tails):
                cov[f"tail of {n}"].append((case.name, extent))
    return {k: sorted(set(map(str, v))) for k, v in cov.items()}


# ==== guard_finalize, restated in fp32 ================================================================================
FIN_SUMSQ = (0.0, 2.0 ** -126, 1.0, 16.0, 1e10, 3e38, float("inf"), float("nan"))
FIN_SCALE = (1.0, 2.0, 8.0)
FIN_MAXNORM = (-1.0, 0.0, 0.5, 1.0, 1e4, FLT_MAX, float("inf"), float("nan"))
FIN_SKIP = (0, 1)


def finalize_table():
    return [(s, k, mn, sk) for s in FIN_SUMSQ for k in FIN_SCALE for mn in FIN_MAXNORM for sk in FIN_SKIP]


def finalize_expect(sumsq, scale, max_norm, skip_nonfinite):
    """(norm, coef, skipped) of guard_finalize(sumsq * scale, ...): every operation one correctly rounded fp32 operation"""
    t = lambda x: torch.tensor(x, dtype=f32)   # noqa: E731
    norm = sqrt32(t(sumsq) * t(scale))
    coef = t(1.0)
    mn = t(max_norm)
    if bool(mn > 0) and bool(mn <= t(FLT_MAX)):
        c = div32(mn, norm + t(1e-6))
        coef = t(1.0) if bool(c > 1.0) else c
    skipped = 1 if (skip_nonfinite and not bool(norm.abs() <= t(FLT_MAX))) else 0
    return float(norm), float(coef), skipped


def same_f32(a, b):
    """two Python floats as fp32: the same bits, or both NaN"""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return torch.equal(bits(torch.tensor([a], dtype=f32)), bits(torch.tensor([b], dtype=f32)))


# ==== Muon ============================================================================================================
ET = 64


def up256(v):
    return (v + 255) & ~255


def muon_layout(nmat, rows, cols):
    """byte offsets of the workspace sections (muon_layout of muon.hip) -> dict name: (offset, payload bytes), total"""
    m, n = min(rows, cols), max(rows, cols)
    tiles = -(-rows // ET) * -(-cols // ET)
    xb, gb = up256(nmat * m * n * 2), up256(nmat * m * m * 2)
    off = {"x0": (0, nmat * m * n * 2), "x1": (xb, nmat * m * n * 2), "a": (2 * xb, nmat * m * m * 2), "b": (2 * xb + gb, nmat * m * m * 2)}
    o = 2 * xb + 2 * gb
    off["sumsq"] = (o, nmat * 4)
    o += up256(nmat * 4)
    off["partials"] = (o, nmat * tiles * 4)
    return off, o + up256(nmat * tiles * 4)


MOM_SHAPES = ((8, 8), (64, 64), (72, 200), (200, 72), (128, 520), (520, 128))
MOM_MU = (0.5, 0.75)
MOM_COEF = (1.0, 0.5)
MOM_NMAT = (1, 3)
Momentum = namedtuple("Momentum", "g buf0 buf x0 sumsq partials")


def mom_plan():
    plan, i = [], 0
    for rows, cols in MOM_SHAPES:
        for nmat in MOM_NMAT:
            for nesterov in (0, 1):
                plan.append((nmat, rows, cols, MOM_MU[i % 2], MOM_COEF[(i // 2) % 2], nesterov))
                i += 1
    return plan


@functools.lru_cache(maxsize=None)
def momentum_case(nmat, rows, cols, mu, coef, nesterov):
    what = f"momentum {nmat} x [{rows}, {cols}] mu {mu} coef {coef} nesterov {nesterov}"
    g_ = gen(nmat, rows, cols, int(mu * 4), int(coef * 2), nesterov, 105)
    gp = E.signs((nmat, rows, cols), g_) * R.pick((1.0, 2.0), (nmat, rows, cols), g_)     # g' = coef g
    g = gp / coef
    buf0 = R.ints((nmat, rows, cols), -1, 1, g_) * 4.0
    A = lambda name, t: R.assert_f32(f"{what} {name}", t).to(f64)   # noqa: E731
    gg = A("coef g", g * coef)
    b = A("buf", A("mu buf", mu * buf0) + gg)
    u = A("u", gg + A("mu b", mu * b)) if nesterov else b
    x0 = u.to(f32).to(bf16)
    assert torch.equal(x0.to(f64), u), what + ": u is no bf16 number"
    multiples(what + " u", u, 0.25)
    sq = u * u
    exact_fit(what + " sumsq", sq.sum((1, 2)), 1.0 / 16.0)
    tr, tc = -(-rows // ET), -(-cols // ET)
    pad = torch.zeros(nmat, tr * ET, tc * ET, dtype=f64)
    pad[:, :rows, :cols] = sq
    parts = pad.reshape(nmat, tr, ET, tc, ET).sum((2, 4)).reshape(nmat, tr * tc)
    sums = A("sumsq", sq.sum((1, 2)))
    assert len(set(sums.tolist())) == nmat, what + ": the matrices must have different sums"
    if rows > cols:
        x0 = x0.transpose(1, 2).contiguous()
    return Momentum(g.to(f32), buf0.to(f32), b.to(f32), x0, sums.to(f32), A("partials", parts).to(f32))


NORM_SHAPES = ((1, 8, 8), (3, 72, 200), (3, 520, 128), (1, 1024, 2056))     # (nmat, rows, cols)
NORM_BLOCK_CAP = 1024


def normalize_grid(per_mat):
    """(workgroups, trips of the grid-stride loop of the busiest thread)"""
    blocks = min(NORM_BLOCK_CAP, (per_mat // 8 + 255) // 256)
    return blocks, -(-(per_mat // 8) // (blocks * 256))


def inv_norm(sumsq32):
    """1 / (sqrt(sumsq) + 1e-7), three correctly rounded fp32 operations"""
    return div32(torch.ones((), dtype=f32), sqrt32(sumsq32) + torch.tensor(1e-7, dtype=f32))


@functools.lru_cache(maxsize=2)
def normalize_case(nmat, rows, cols):
    g_ = gen(nmat, rows, cols, 107)
    m, n = min(rows, cols), max(rows, cols)
    u = (torch.randn(nmat, m, n, generator=g_, dtype=f32) * 1.5).to(bf16)
    sumsq = (u.to(f64) ** 2).sum((1, 2)).to(f32) * torch.tensor([1.0, 0.25, 3.0][:nmat], dtype=f32)
    inv = inv_norm(sumsq)
    want = (u.to(f32) * inv[:, None, None]).to(bf16)       # one fp32 product, one bf16 rounding
    assert not torch.equal(bits(want), bits(u))
    return u, sumsq, want


# ---- the Newton-Schulz iteration ---------------------------------------------------------------------------------------
NS_A, NS_B, NS_C = f32v(3.4445), f32v(-4.7750), f32v(2.0315)
BM = 128
# (m, n); the last one is here for its K tails of 40 (104 = 64 + 40, 168 = 128 + 40): every other tail is 8
NS_SHAPES = ((8, 8), (64, 64), (128, 128), (136, 136), (264, 264), (128, 520), (8, 520), (200, 328), (104, 168))
NS_CPU_SHAPES = ((64, 64), (136, 136), (264, 264), (128, 512), (200, 328), (264, 520), (8, 520))
NS_NMAT = (1, 3)
NS_RECIPES = ("dense", "sparse", "signed_permutation")


def tri_tiles(m):
    t = -(-m // BM)
    return t * (t + 1) // 2


def k_tail(K):
    return K % 64


def ns_u(recipe, nmat, m, n):
    """u [nmat, m, n] with entries in {0, +-1} (scaled permutation: +-{1/2, 1, 2}); distinct matrices; X = u / 4"""
    g_ = gen(nmat, m, n, NS_RECIPES.index(recipe), 109)
    if recipe == "dense":
        u = E.signs((nmat, m, n), g_)
    elif recipe == "sparse":
        u = torch.zeros(nmat, m, n, dtype=f64)
        per = min(32, n)
        for k in range(nmat):
            for r in range(m):
                cols = torch.randperm(n, generator=g_)[:per]
                u[k, r, cols] = E.signs((per,), g_)
        for k, c in (u == 0).all(1).nonzero().tolist():     # a column no row has drawn gets one entry
            u[k, (c * 7 + k) % m, c] = 1.0 if c % 2 else -1.0
        assert not (u == 0).all(1).any(), "an empty column of u"
    else:
        u = torch.zeros(nmat, m, n, dtype=f64)
        for k in range(nmat):
            cols = torch.randperm(n, generator=g_)[:m]
            u[k, torch.arange(m), cols] = E.signs((m,), g_) * R.pick((0.5, 1.0, 2.0), (m,), g_)
    if recipe != "signed_permutation":
        assert not (u == 0).all(1).any(), "an empty column of u"
    assert nmat == 1 or not any(torch.equal(u[0], u[k]) for k in range(1, nmat))
    return G.to_bf16_exact(u)


def lsb(t64):
    """the granule of every element: the value of the lowest set bit of a bf16 number held in float64 (inf for 0)"""
    m, e = torch.frexp(t64.abs())
    mi = (m * 256.0).round().to(torch.int64)
    assert torch.equal(mi.to(f64) / 256.0, m), "not bf16 numbers"
    low = (mi & -mi).to(f64)
    out = low * torch.pow(torch.tensor(2.0, dtype=f64), (e - 8).to(f64))
    return torch.where(t64 == 0, torch.full_like(t64, float("inf")), out)


def _fits(abs_sum, gran):
    """the fp32 sum of addends that are multiples of `gran` is exact in any order: magnitudes below 2^24 granules"""
    return (abs_sum / gran < 2.0 ** 24) | (abs_sum == 0)


def _row_gran(t64):
    g = lsb(t64).amin(-1)
    return torch.where(torch.isinf(g), torch.ones_like(g), g)


def _epilogue(acc, alpha, beta, add):
    """bf16(alpha acc + beta add) under the three contractions the compiler may choose -> (want, undecided)"""
    r32 = lambda t: t.to(f32).to(f64)   # noqa: E731
    va, vb = r32(alpha * acc), r32(beta * add)
    return R.decide([r32(va + vb), r32(va + beta * add), r32(alpha * acc + vb)])


def ns_expect_a(X):
    """A = bf16(X X^T) from a stored X [nmat, m, n] -> (want, excluded)"""
    x = X.to(f64)
    acc = x @ x.transpose(1, 2)
    g = _row_gran(x)
    fit = _fits(x.abs() @ x.abs().transpose(1, 2), g[:, :, None] * g[:, None, :])
    return acc.to(f32).to(bf16), ~fit


def ns_expect_b(A):
    """B = bf16(c A A + b A) from a stored A [nmat, m, m] (the kernel multiplies A by ITSELF as an NT product: A A^T)"""
    a = A.to(f64)
    acc = a @ a.transpose(1, 2)
    g = _row_gran(a)
    fit = _fits(a.abs() @ a.abs().transpose(1, 2), g[:, :, None] * g[:, None, :])
    want, und = _epilogue(acc, NS_C, NS_B, a)
    return want, und | ~fit


def ns_expect_x(B, X):
    """X' = bf16(B X + a X) from the stored B [nmat, m, m] and X [nmat, m, n]"""
    b, x = B.to(f64), X.to(f64)
    acc = b @ x
    gb = _row_gran(b)
    gx = _row_gran(x.transpose(1, 2))
    fit = _fits(b.abs() @ x.abs(), gb[:, :, None] * gx[:, None, :])
    want, und = _epilogue(acc, 1.0, NS_A, x)
    return want, und | ~fit


def check_product(what, got, want, excluded, cap=UNDECIDED_CAP):
    """compared elements bit-equal, the excluded share under the cap -> the share"""
    share = float(excluded.double().mean())
    assert share <= cap, f"{what}: {share:.2%} of the elements undecided or not fitting 24 bits"
    diff = (bits(got) != bits(want)) & ~excluded
    if diff.any():
        idx = tuple(int(v) for v in diff.nonzero()[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.numel()} compared elements differ, first at (matrix, row, col) "
                             f"{idx}: got {got[idx].item()!r} want {want[idx].item()!r}")
    return share


def ns_chain(recipe, nmat, m, n):
    """the helper's own chain from X = u / 4 (CPU test): the shares of excluded elements of the three products"""
    X = (ns_u(recipe, nmat, m, n).to(f64) / 4.0).to(bf16)
    A, ex_a = ns_expect_a(X)
    assert torch.equal(A.to(f64), X.to(f64) @ X.to(f64).transpose(1, 2)), "A is inexact in bf16"
    Bm, ex_b = ns_expect_b(A)
    X1, ex_x = ns_expect_x(Bm, X)
    return X, A, Bm, X1, tuple(float(e.double().mean()) for e in (ex_a, ex_b, ex_x))


def ns_forward(X, iters):
    """`iters` iterations of the helper's chain from a stored X; raises when any element is excluded on the way (the
    signed-permutation recipe: every sum has one addend)"""
    for it in range(iters):
        A, ea = ns_expect_a(X)
        Bm, eb = ns_expect_b(A)
        X, ex = ns_expect_x(Bm, X)
        assert not (ea.any() or eb.any() or ex.any()), f"iteration {it}: an element without one right answer"
    return X


# ---- update --------------------------------------------------------------------------------------------------------------
UPD_EXACT = ((64, 64), (128, 520), (512, 128))
UPD_INEXACT = (328, 200)
UPD_SCALARS = ((2.0 ** -4, 2.0 ** -2, 0.5, 0.75), (2.0 ** -3, 2.0 ** -3, 1.0, 0.5))     # (lr, wd, lr_mult, ema decay)
Update = namedtuple("Update", "p0 ema0 o p p_alt pb ema scale")


def muon_scale(rows, cols):
    """sqrtf(max(1, (float)rows / (float)cols)) in fp32"""
    ratio = div32(torch.tensor(float(rows), dtype=f32), torch.tensor(float(cols), dtype=f32))
    return float(sqrt32(torch.clamp(ratio, min=1.0)))


@functools.lru_cache(maxsize=None)
def update_case(nmat, rows, cols, scalars):
    """O in the orientation of the matrices.  Exact shapes: p == p_alt, the one right answer.  [328, 200]: p the
    uncontracted and p_alt the contracted fp32 result; the shadow and the EMA follow from the GPU's own p (ema_from)"""
    lr, wd, lr_mult, d = scalars
    what = f"update {nmat} x [{rows}, {cols}] {scalars}"
    g_ = gen(nmat, rows, cols, int(lr * 4096), 111)
    p0 = R.ints((nmat, rows, cols), -4096, 4096, g_) / 1024.0
    ema0 = R.ints((nmat, rows, cols), -64, 64, g_) / 16.0
    o = R.ints((nmat, rows, cols), -32, 32, g_) / 16.0
    o[o == 0] = 0.4375
    scale = muon_scale(rows, cols)
    A = lambda name, t: R.assert_f32(f"{what} {name}", t).to(f64)   # noqa: E731
    lr_e = A("lr", torch.tensor(lr * lr_mult, dtype=f64))
    dec = A("decay", 1.0 - A("lr wd", lr_e * wd))
    m, _ = math.frexp(lr * lr_mult)
    assert m == 0.5, "lr x lr_mult must be a power of two: step = lr scale is then exact"
    step = A("step", lr_e * scale)
    pd = A("p decay", p0 * dec)
    r32 = lambda t: t.to(f32).to(f64)   # noqa: E731
    p = r32(pd - r32(step * o))
    p_alt = r32(pd - step * o)
    if scale in (1.0, 2.0):
        assert torch.equal(p, p_alt) and torch.equal(p, pd - step * o), what + ": p' is not exact"
    else:
        assert 0.0 < float((p != p_alt).double().mean()), what + ": the two forms never differ"
    return Update(p0.to(f32), ema0.to(f32), G.to_bf16_exact(o), p.to(f32), p_alt.to(f32), p.to(f32).to(bf16),
                  ema_from(ema0.to(f32), p.to(f32), d, exact=scale in (1.0, 2.0)), scale)


def ema_from(ema0, p, d, exact):
    """d ema + (1 - d) p: both products are exact (d and 1 - d have two significant bits at most, checked), one rounding"""
    e, q = ema0.to(f64) * d, p.to(f64) * (1.0 - d)
    if exact:
        R.assert_f32("ema'", e + q)
    else:
        assert torch.equal(e.to(f32).to(f64), e)
        # (1 - d) p may need one bit more than fp32 holds when 1 - d = 3/4-like; d in {1/2, 3/4}: 1 - d is a power of two
        m, _ = math.frexp(1.0 - d)
        assert m == 0.5
    return (e + q).to(f32)
