"""Exact census of the row kernels (csrc/elementwise.hip): inputs, float64 expectations, dispatch predicates, shape lists.

The roots of every bit-equality chain of the element-wise family -- vds_rmsnorm_mod_fwd / _bwd, vds_gate_bwd,
vds_colsum_bf16[_rows], vds_qkv_rope_fwd / _bwd and vds_rope_apply -- are pinned element by element, as gemm_census.py
pins the GEMM.  Operands are signs times powers of two and small dyadic rationals: every product and every fp32 sum is
exact in any order (lanes, the 16- against the 64-lane reduction, the LDS pass, atomics, the deterministic partials).
What stays inexact is ONE intermediate per kernel -- the rsqrt of the forward, dot / D of the backward -- and the fp32
operations behind it.  The expectation is computed in float64 from the formula in the kernel's comment and again with
that intermediate moved by +- 2^-21 relative (~8 fp32 ulps: a hardware rsqrt, a reciprocal-multiply division) and the
result by the half ulp of its last fp32 rounding; an element is DECIDED when every variant rounds (RNE) to the same bf16.
Dyadic builders ASSERT that every element is decided (and that every sum fits 24 bits) and raise otherwise; they never
skip a case.  Everything here runs on the CPU with torch alone; the GPU test compares bits.
"""
import functools
from collections import namedtuple

import torch

from gemm_census import SENTINEL_BF16, SENTINEL_F32, bits, fill_value, round_bf16, to_bf16_exact  # noqa: F401

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64

EPS = float(torch.tensor(1e-6, dtype=f32))   # the fp32 number the kernels are given
REL = 2.0 ** -21                             # the move of an inexact intermediate
LAST = 2.0 ** -23                            # one fp32 rounding of the result (half an ulp <= 2^-24) with a margin of 2
UNDECIDED_CAP = 0.05                         # generic rows: the largest share of a tensor that may be undecided
JMIN, NJ = -12, 19                           # rows are +-2^j, j in [-12, 6]: mean squares from 6e-8 (eps decides) to 4096

S1 = (1.0, 2.0, -1.0, -2.0, 0.5, 4.0, 0.0, 1.5)              # 1 + scale
WSET = (1.0, -1.0, 2.0, 0.5)                                  # RMSNorm weight
SHIFT = (0.0, 16.0, -16.0, 32.0, -32.0, 48.0, -48.0)          # shift / dres: too large for x^ w (1 + scale) to cancel
DY = (0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0)
TAB = (0.0, 1.0, -1.0, 0.5, -0.5)                             # cos / sin table entries
LAM = (0.5, 0.25)


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 12345) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def pick(values, shape, g):
    return torch.tensor(values, dtype=f64)[torch.randint(0, len(values), tuple(shape), generator=g)]


def ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(f64)


def exps(R):
    """the exponent j of every row: all 19 values of [-12, 6] from 19 rows on, in an order with no run"""
    return torch.tensor([JMIN + (7 * r + 3) % NJ for r in range(R)], dtype=f64)


def decide(variants):
    """variants[0] is the float64 result, the others the moved ones -> (bf16 of variants[0], mask of undecided elements)"""
    r = [v.to(f32).to(bf16) for v in variants]
    und = torch.zeros(variants[0].shape, dtype=torch.bool)
    for t in r[1:]:
        und |= bits(t) != bits(r[0])
    return r[0], und


def assert_decided(what, und):
    assert not und.any(), f"{what}: {int(und.sum())} of {und.numel()} elements undecided (the recipe is not exact)"


def assert_f32(what, t64):
    """an exact result must be an fp32 number"""
    assert torch.equal(t64.to(f32).to(f64), t64), f"{what}: not an fp32 number"
    return t64.to(f32)


def exact_sum(what, terms, dim, init):
    """init + sum of `terms` over `dim` as fp32: exact in any order when every term is a multiple of 2^-6 and the sum of
    the magnitudes stays below 2^24 of them"""
    t = terms * 64.0
    assert torch.equal(t, t.round()), f"{what}: terms are no multiples of 2^-6"
    total = t.abs().sum(dim) + (init * 64.0).abs()
    assert float(total.max()) < 2 ** 24, f"{what}: the sum needs more than 24 bits"
    return assert_f32(what, init + terms.sum(dim))


def assert_no_sentinel(what, t):
    s = SENTINEL_BF16 if t.dtype == bf16 else SENTINEL_F32
    assert not (bits(t) == s).any(), f"{what}: the sentinel is a value of this case"


def ulps32(got, want64):
    """|got - want| in fp32 ulps of want"""
    w = want64.abs().to(f32)
    ulp = (torch.nextafter(w, torch.full_like(w, float("inf"))) - w).to(f64)
    return ((got.to(f64) - want64).abs() / ulp).max().item()


# ---- dispatch predicates (restated from elementwise.hip) ---------------------------------------------------------------
def nc_of(D):
    """NC_DISPATCH: 16-byte chunks per lane of a one-row-per-wave kernel; > 4 is VDS_ERR_UNSUPPORTED"""
    return (D // 8 + 63) // 64


def q4_rule(D, knob=1):
    return D in (384, 768, 1152) and knob != 0


def fwd_instance(D, q4=1):
    return f"q4<{D // 128}>" if q4_rule(D, q4) else f"row<{nc_of(D)}>"


def rows_per_block(L, B, min_rows=8, wgs=0):
    """rows_per_block_for: ceil(B L / 768), floored at ew_min_rows -- at 32 from 8192 rows while the knob is the default 8"""
    min_rows = max(1, min_rows)
    target = wgs if wgs > 0 else 768
    total = L * B
    rpb = (total + target - 1) // target
    floor_rows = 32 if (min_rows == 8 and total >= 8192) else min_rows
    return max(rpb, floor_rows)


def block_classes(L, B, min_rows=8, wgs=0):
    """the walks of one launch of a backward row kernel"""
    rpb = rows_per_block(L, B, min_rows, wgs)
    c = set()
    if min_rows == 8 and wgs == 0:
        c.add("floor 32 (default knobs)" if L * B >= 8192 else "floor 8 (default knobs)")
        if rpb > 32:
            c.add("ceil(rows / 768) rows")
    if rpb > L:
        c.add("block longer than L")
    if min(rpb, L) < 4:
        c.add("block shorter than 4 rows (idle waves)")
    if L % rpb:
        c.add("ragged last block")
    if L > rpb:
        c.add("several blocks per sample")
    if rpb >= 8 and L >= 8:
        c.add("a wave walks several rows")
    if min_rows == 1:
        c.add("ew_min_rows 1")
    if min_rows == 32:
        c.add("ew_min_rows 32")
    if wgs:
        c.add("ew_wgs")
    return c


TILE_INSTANCES = ((72, 96), (64, 64), (128, 128), (96, 96), (32, 32))


def qkv_fwd_form(H, hd, hdp, L, tile=4):
    """qkv_rope_fwd_impl: the token-tile instance or the reason for the element-wise kernel"""
    if tile <= 0:
        return "elem: rope_tile 0"
    if H * hd > 2048 or H > 256:
        return "elem: H hd > 2048"
    if L < 8:
        return "elem: L < 8"
    if (hd, hdp) not in TILE_INSTANCES:
        if hdp % 8:
            return "elem: hdp % 8"
        return "elem: no tile instance"
    return f"tile<{hd},{hdp},{tile if tile in (2, 8) else 4}>"


def qkv_bwd_form(H, hd, hdp, tok=1):
    """qkv_rope_bwd_impl: wave-per-token with NI items per lane, or the element-wise kernel"""
    if not tok:
        return "elem: rope_tok 0"
    if hdp % 8:
        return "elem: hdp % 8"
    if H * hd > 2048:
        return "elem: H hd > 2048"
    D = H * hd
    return f"tok<{1 if D <= 512 else 2 if D <= 1024 else 3 if D <= 1536 else 4}>"


def pad_refused(hd, hdp):
    return ((hdp - hd) >> 2) > (hd >> 3)


# ---- shape lists -------------------------------------------------------------------------------------------------------
FWD_D = [
    8,      # one chunk: one live lane
    72,     # 9 chunks
    144,    # the smoke model's width
    384,    # q4<3> (and row<1> with rmsnorm_q4 = 0)
    512,    # the last width of NC = 1
    520,    # one chunk past: NC = 2 with one live lane in the second pass
    768,    # q4<6> (row<2>)
    1024,   # the last width of NC = 2
    1032,   # one chunk past: NC = 3
    1152,   # q4<9> (row<3>): DiT-XL
    1536,   # the last width of NC = 3
    1544,   # one chunk past: NC = 4
    2048,   # the last supported width
]
FWD_BL = [
    (1, 1),     # one row: three idle waves, fifteen idle 16-lane groups
    (1, 17),    # a 1-row tail behind four full waves (q4: 1 row behind one full wave)
    (2, 16),    # no tail at all
    (3, 21),    # 63 rows: 3-row tail; L = 21: a wave's four rows span two samples
    (5, 7),     # 35 rows: 3-row tail of the 4-row workgroups; L = 7: a workgroup spans up to three samples
]
BWD_D = [
    8,      # NC = 1, one live lane
    144,
    512,    # the last width of NC = 1
    520,    # NC = 2, one live lane in the second pass
    1024,
    1152,   # NC = 3: DiT-XL
    1536,
    2048,   # NC = 4
]
BWD_L = [1, 3, 8, 9, 21, 37]   # below a workgroup's four waves, one block exactly, one row past, several ragged blocks
BWD_B = [1, 3]
BWD_KNOBS = [
    {},                     # the defaults: 8 rows per workgroup
    {"ew_min_rows": 1},     # one row per workgroup: three idle waves
    {"ew_min_rows": 8},     # the default, set explicitly
    {"ew_min_rows": 32},    # the floor the 8192-row rule picks
    {"ew_wgs": 2},          # ceil(B L / 2) rows per workgroup: blocks longer than L
]
BWD_GENERIC_BL = [(3, 21), (1, 9)]   # generic rows (dx only): ragged blocks of three samples; one row past a block
BWD_FLOOR32 = (2, 4100, 8)   # (B, L, D): 8200 rows reach the default 32-row floor without a knob (131 KB per tensor)
COLSUM_M = [1, 63, 64, 65, 203]      # below / at / past the 64 rows of a workgroup; 8193 (N = 8): 65-row workgroups
COLSUM_N = [8, 72, 512, 520, 1152]   # one workgroup column, its edge, one chunk past, three
COLSUM_BIG = (8193, 8)
COLSUM_ROWS = [(0, 0), (29, 16), (7, 0)]   # (rows_per_sample, row_offset)
# (hd, hdp, H, B, L) of the qkv / RoPE forward; every one runs with and without v0, tile cases at rope_tile 2, 4, 8, 0
QKV_BL = [
    (3, 25),    # 75 tokens: ragged tile of every T, tiles that span two samples
    (1, 8),     # the smallest L of the token-tile form
    (1, 9),     # one token past
    (2, 5),     # L < 8: element-wise
]
QKV_FWD_TILE = [(hd, hdp, H) for hd, hdp in TILE_INSTANCES for H in (1, 3)] + [(72, 96, 16)]   # H = 16: DiT-XL's row
QKV_FWD_ELEM = [
    (24, 24, 3),    # no tile instance, no pad
    (48, 56, 3),    # no tile instance, 8 pad columns: the ones columns of the element-wise kernel
    (64, 68, 3),    # hdp % 8 != 0: 4 pad columns, no ones
    (64, 64, 33),   # H hd = 2112 > 2048
]
# (hd, hdp, H, knobs) of the qkv / RoPE backward
QKV_BWD = [
    (64, 64, 2, {}),                 # tok<1>
    (64, 64, 12, {}),                # tok<2>
    (72, 96, 16, {}),                # tok<3>: DiT-XL, 9 chunks per head
    (64, 64, 32, {}),                # tok<4>
    (72, 96, 3, {"rope_tok": 0}),    # element-wise by the knob
    (64, 68, 3, {}),                 # element-wise: hdp % 8 != 0
    (64, 64, 33, {}),                # element-wise: H hd = 2112
]
QKV_BWD_BL = [(3, 25), (1, 9)]      # 75 tokens: 3-token tail of the 4-token workgroups; 9: one token past two
QKV_BWD_MODES = [(0, 0), (0, 1), (1, 0), (2, 0)]   # (mix, add_dv0)
ROPE_APPLY_HD = [32, 72, 128]
ROPE_APPLY_L = 25


def bwd_plan(D):
    """(B, L, knobs, with_w, with_dres) of every backward launch at width D: the two flags rotate through their four
    combinations, so every width meets each of them under every knob"""
    n = 0
    for B in BWD_B:
        for L in BWD_L:
            for k in BWD_KNOBS:
                n += 1
                yield B, L, k, bool(n & 1), bool(n & 2)


def bwd_launches():
    """(B, L, D, knobs) of every backward / gate launch of the census"""
    out = [(B, L, D, k) for D in BWD_D for B in BWD_B for L in BWD_L for k in BWD_KNOBS]
    return out + [BWD_FLOOR32 + ({},)]


def coverage():
    """name -> bool: every dispatch branch of the seven entry points holds at least one census case"""
    cov = {}
    inst = {fwd_instance(D, 1) for D in FWD_D} | {fwd_instance(D, 0) for D in (384, 768, 1152)}
    for name in ("row<1>", "row<2>", "row<3>", "row<4>", "q4<3>", "q4<6>", "q4<9>"):
        cov[f"fwd {name}"] = name in inst
    for nc, edge in ((1, 512), (2, 1024), (3, 1536), (4, 2048)):
        cov[f"fwd NC {nc} at its last width"] = edge in FWD_D and nc_of(edge) == nc
        if nc < 4:
            cov[f"fwd one chunk past NC {nc}"] = edge + 8 in FWD_D and nc_of(edge + 8) == nc + 1
    rows = {B * L for B, L in FWD_BL}
    cov["fwd one row"] = 1 in rows
    cov["fwd full workgroups only"] = any(r % 16 == 0 for r in rows)
    cov["fwd ragged last wave (q4) and workgroup"] = any(r % 4 == 3 for r in rows)
    cov["fwd a wave's four rows span two samples"] = any(L % 4 and B > 1 for B, L in FWD_BL)
    for q4 in (0, 1):
        cov[f"fwd rmsnorm_q4 = {q4} at 384 / 768 / 1152"] = all(D in FWD_D for D in (384, 768, 1152))
    launches = bwd_launches()
    for nc in (1, 2, 3, 4):
        cov[f"bwd NC {nc}"] = any(nc_of(D) == nc for _, _, D, _ in launches)
        classes = set()
        for B, L, D, k in launches:
            if nc_of(D) == nc:
                classes |= block_classes(L, B, k.get("ew_min_rows", 8), k.get("ew_wgs", 0))
        for c in ("floor 8 (default knobs)", "block longer than L", "block shorter than 4 rows (idle waves)",
                  "ragged last block", "several blocks per sample", "a wave walks several rows", "ew_min_rows 1",
                  "ew_min_rows 32", "ew_wgs"):
            cov[f"bwd NC {nc}: {c}"] = c in classes
    for D in BWD_D:
        flags = {(w, r) for _, _, _, w, r in bwd_plan(D)}
        cov[f"bwd D {D}: with and without w and dres"] = len(flags) == 4
        for k in BWD_KNOBS:
            cov[f"bwd D {D} {k}: with and without w"] = len({w for _, _, kk, w, _ in bwd_plan(D) if kk == k}) == 2
    B, L, D = BWD_FLOOR32
    cov["bwd floor 32 (default knobs)"] = "floor 32 (default knobs)" in block_classes(L, B) and rows_per_block(L, B) == 32
    cov["bwd one chunk past NC 1"] = 520 in BWD_D
    cs = set(COLSUM_M)
    cov["colsum below / at / past 64 rows"] = {63, 64, 65} <= cs and 1 in cs
    cov["colsum several row blocks"] = any(m > 128 for m in cs)
    cov["colsum 8192+ rows"] = COLSUM_BIG[0] > 8192
    cov["colsum one chunk past a workgroup column"] = {512, 520} <= set(COLSUM_N)
    cov["colsum skipped register rows"] = any(o > 0 for _, o in COLSUM_ROWS) and any(r > 0 and o == 0 for r, o in COLSUM_ROWS)
    forms = {qkv_fwd_form(H, hd, hdp, L, t) for hd, hdp, H in QKV_FWD_TILE for _, L in QKV_BL for t in (2, 4, 8, 0)}
    forms |= {qkv_fwd_form(H, hd, hdp, L, 4) for hd, hdp, H in QKV_FWD_ELEM for _, L in QKV_BL}
    for hd, hdp in TILE_INSTANCES:
        for t in (2, 4, 8):
            cov[f"qkv fwd tile<{hd},{hdp},{t}>"] = f"tile<{hd},{hdp},{t}>" in forms
    for why in ("rope_tile 0", "L < 8", "H hd > 2048", "hdp % 8", "no tile instance"):
        cov[f"qkv fwd elem: {why}"] = f"elem: {why}" in forms
    cov["qkv fwd elem with ones columns"] = any(hdp - hd >= 8 for hd, hdp, _ in QKV_FWD_ELEM)
    cov["qkv fwd elem with 4 pad columns"] = any(hdp - hd == 4 for hd, hdp, _ in QKV_FWD_ELEM)
    cov["qkv fwd ragged tile"] = any((B * L) % 8 and (B * L) % 4 and (B * L) % 2 for B, L in QKV_BL)
    bforms = {qkv_bwd_form(H, hd, hdp, k.get("rope_tok", 1)) for hd, hdp, H, k in QKV_BWD}
    for ni in (1, 2, 3, 4):
        cov[f"qkv bwd tok<{ni}>"] = f"tok<{ni}>" in bforms
    for why in ("rope_tok 0", "hdp % 8", "H hd > 2048"):
        cov[f"qkv bwd elem: {why}"] = f"elem: {why}" in bforms
    cov["qkv bwd ragged workgroup"] = any((B * L) % 4 for B, L in QKV_BWD_BL)
    cov["refusal D = 2056"] = nc_of(2056) > 4
    cov["refusal pad"] = pad_refused(64, 104) and not any(pad_refused(hd, hdp) for hd, hdp, _ in QKV_FWD_TILE + QKV_FWD_ELEM)
    return cov


# ---- RMSNorm + modulate, forward ---------------------------------------------------------------------------------------
Fwd = namedtuple("Fwd", "B L D x w mod s1 shift want_y r64 und")


def mod_table(B, D, first, third):
    """f32 [B, 4 D]: `first` at column 0, `third` at 2 D, NaN in the columns no call may read"""
    m = torch.full((B, 4 * D), float("nan"), dtype=f32)
    for c0, v in ((0, first), (2 * D, third)):
        v64 = v if isinstance(v, torch.Tensor) else torch.full((B, D), float(v), dtype=f64)
        m[:, c0:c0 + D] = assert_f32("modulation table", v64)
    return m


def fwd_expect(x, w, s1, shift, L, eps=EPS):
    """(float64 y of every variant, float64 rstd): y = x r [w] (1 + scale) + shift, r = (mean x^2 + eps)^-1/2"""
    R, D = x.shape
    b = torch.arange(R) // L
    r64 = 1.0 / torch.sqrt((x * x).sum(1) / D + eps)
    variants = []
    for dr in (0.0, -REL, REL):
        p = x * (r64 * (1.0 + dr))[:, None]
        if w is not None:
            p = p * w
        y = p * s1[b] + shift[b]
        variants += [y, y * (1.0 - LAST), y * (1.0 + LAST)]
    return variants, r64


# a draw whose y holds the sentinel's value (-0.4668, reachable as x^ w (1 + scale) of an eps-damped row) is drawn again
FWD_SALT = {(5, 7, 1544, True): 1}


@functools.lru_cache(maxsize=None)
def fwd_case(B, L, D, with_w):
    salt = FWD_SALT.get((B, L, D, bool(with_w)))
    g = _gen(1, B, L, D, with_w, *([salt] if salt else []))
    R = B * L
    j = exps(R)
    sign = pick((1.0, -1.0), (R, D), g)
    x = sign * (2.0 ** j)[:, None]
    if R >= 3:
        x[R // 2] = 0.0                                    # r = eps^-1/2, y = shift
        up = torch.randint(0, 2, (D,), generator=g).to(f64)
        up[0], up[1] = 0.0, 1.0
        x[R // 3] = sign[R // 3] * 2.0 ** (j[R // 3] + up)  # two magnitudes: an irrational r
    w = pick(WSET, (D,), g) if with_w else None
    s1, shift = pick(S1, (B, D), g), pick(SHIFT, (B, D), g)
    variants, r64 = fwd_expect(x, w, s1, shift, L)
    want, und = decide(variants)
    assert_decided(f"rmsnorm fwd B {B} L {L} D {D}", und)
    assert_no_sentinel(f"rmsnorm fwd y B {B} L {L} D {D} w {with_w}", want)
    ms = (x * x).sum(1) / D
    if R >= NJ:
        assert (ms < EPS / 8).any() and (ms > 1.0).any()   # rows that eps decides, rows that it does not touch
    return Fwd(B, L, D, to_bf16_exact(x), None if w is None else to_bf16_exact(w), mod_table(B, D, shift, s1 - 1.0),
               s1, shift, want, r64, und)


# ---- RMSNorm + modulate, backward --------------------------------------------------------------------------------------
Bwd = namedtuple("Bwd", "B L D kind x w dy dres mod rstd dmod0 dw0 want_dx und want_dmod want_dw share dx64")


def bwd_expect(x, w, dy, dres, s1, rstd, L, generic):
    """float64 dx of every variant + the terms of the three column sums.  The kernel's comment:
    g = dy (1 + scale) [w], dot = mean_d(g x^), dx = dres + r (g - x^ dot);  d(shift) = sum dy, d(scale) = sum dy x^ [w],
    dw = sum dy (1 + scale) x^"""
    R, D = x.shape
    b = torch.arange(R) // L
    xhat = x * rstd[:, None]
    t = dy * s1[b]
    g = t * w if w is not None else t
    terms = g * xhat
    dot = terms.sum(1) / D
    # the error of dot: the division (relative); on generic rows the fp32 sum of D rounded terms as well, bounded by
    # 2^-21 of the mean magnitude of the terms (any order: a lane adds at most 32 terms, the butterfly 6 more)
    e_dot = REL * dot.abs() + (REL * terms.abs().mean(1) if generic else 0.0)
    d0 = dres if dres is not None else torch.zeros_like(x)
    variants = []
    for sd in (0.0, -1.0, 1.0):
        dt = (dot + sd * e_dot)[:, None]
        v = d0 + rstd[:, None] * (g - xhat * dt)
        # the fp32 operations behind dot: one rounding of the result on dyadic rows, a few of the parts on generic ones
        # (nothing where dot is exactly zero: every fp32 operation is then exact, ties included)
        e_out = 2 * LAST * (d0.abs() + rstd[:, None] * (g.abs() + (xhat * dt).abs())) if generic else \
            LAST * v.abs() * (dot != 0)[:, None]
        variants += [v, v - e_out, v + e_out]
    return variants, dy, dy * xhat * (w if w is not None else 1.0), t * xhat, terms


@functools.lru_cache(maxsize=None)
def bwd_case(B, L, D, with_w, with_dres, kind="dyadic"):
    """kind "dyadic": every row has sum_d g x^ = 0 (columns 2k, 2k+1 carry opposite terms): dx = dres + r g, exact;
    "const": g x^ is one constant m per row (dot = m up to the division): dx = dres up to r m 2^-21, needs dres;
    "generic": Gaussian x, dy, dres (dx only: undecided elements may be one bf16 ulp off the float64 rounding)"""
    assert kind in ("dyadic", "const", "generic") and (kind != "const" or with_dres)
    g = _gen(2, B, L, D, with_w, with_dres, ("dyadic", "const", "generic").index(kind))
    R, P = B * L, D // 2
    b = torch.arange(R) // L
    # (generic rows leave 1 + scale = 0 out: where g = 0, dx is -r x^ dot alone and as uncertain as a cancelling dot)
    mag1 = torch.full((B, P), 2.0, dtype=f64) if kind == "const" else \
        pick((1.0, 2.0, 0.5, 4.0, 1.5) if kind == "generic" else (1.0, 2.0, 0.5, 4.0, 0.0, 1.5), (B, P), g)
    magw = torch.ones(P, dtype=f64) if kind == "const" else pick((1.0, 2.0, 0.5), (P,), g)
    s1 = mag1.repeat_interleave(2, 1) * pick((1.0, -1.0), (B, D), g)
    w = magw.repeat_interleave(2) * pick((1.0, -1.0), (D,), g) if with_w else None
    if kind == "generic":
        x = (torch.randn(R, D, generator=g, dtype=f64) * 1.5).to(bf16).to(f64)
        rstd = torch.rsqrt(((x * x).sum(1) / D + EPS).to(f32)).to(f64)   # an fp32 input: the backward takes it as given
        dy = torch.randn(R, D, generator=g, dtype=f64).to(bf16).to(f64)
        dres = torch.randn(R, D, generator=g, dtype=f64).to(bf16).to(f64) if with_dres else None
    else:
        j = exps(R)
        rstd = 2.0 ** -j
        mag = pick((0.5, 1.0, 2.0, 3.0), (R, 1) if kind == "const" else (R, P), g)
        mag = mag.expand(R, D) if kind == "const" else mag.repeat_interleave(2, 1)
        dy = mag * pick((1.0, -1.0), (R, D), g)
        sx = pick((1.0, -1.0), (R, D), g)
        c = dy * s1[b] * (w if w is not None else 1.0)
        if kind == "const":
            sx = torch.sign(c) * pick((1.0, -1.0), (R, 1), g)
        else:
            even, odd = c[:, 0::2] * sx[:, 0::2], c[:, 1::2]
            sx[:, 1::2] = torch.where(odd != 0, -torch.sign(even) * torch.sign(odd), sx[:, 1::2])
        x = sx * (2.0 ** j)[:, None]
        dres = pick(SHIFT[1:] if kind == "const" else SHIFT, (R, D), g) if with_dres else None
    variants, t_shift, t_scale, t_w, terms = bwd_expect(x, w, dy, dres, s1, rstd, L, kind == "generic")
    want, und = decide(variants)
    what = f"rmsnorm bwd {kind} B {B} L {L} D {D} w {with_w} dres {with_dres}"
    share = float(und.float().mean())
    dmod0 = torch.full((B, 4 * D), 0.0, dtype=f32)
    dmod0.view(torch.int32).fill_(SENTINEL_F32)          # the columns D .. 2D-1 and 3D .. 4D-1 must survive
    dw0 = ints((D,), -3, 3, g) if with_w else None
    want_dmod = want_dw = None
    if kind == "generic":
        assert share <= UNDECIDED_CAP, f"{what}: {share:.1%} of dx undecided"
        dmod0[:, :D], dmod0[:, 2 * D:3 * D] = 0.0, 0.0
    else:
        assert_decided(what, und)
        if kind == "dyadic":
            assert (terms.sum(1) == 0).all()
            assert_f32(what, variants[0])
        else:
            assert torch.equal(want.to(f64), dres), "a constant-m row: dx = dres"
        i_sh, i_sc = ints((B, D), -3, 3, g), ints((B, D), -3, 3, g)
        dmod0[:, :D], dmod0[:, 2 * D:3 * D] = i_sh.to(f32), i_sc.to(f32)
        want_dmod = dmod0.clone()
        want_dmod[:, :D] = exact_sum(what + " d(shift)", t_shift.view(B, L, D), 1, i_sh)
        want_dmod[:, 2 * D:3 * D] = exact_sum(what + " d(scale)", t_scale.view(B, L, D), 1, i_sc)
        assert_no_sentinel("dmod", want_dmod[:, :D]), assert_no_sentinel("dmod", want_dmod[:, 2 * D:3 * D])
        if with_w:
            want_dw = exact_sum(what + " dw", t_w, 0, dw0)
    if kind != "generic":   # (Gaussian rows can give any bf16: their output window starts as NaN, which no finite row gives)
        assert_no_sentinel("dx", want)
    assert torch.isfinite(want.to(f32)).all()
    cast = to_bf16_exact
    return Bwd(B, L, D, kind, cast(x), None if w is None else cast(w), cast(dy), None if dres is None else cast(dres),
               mod_table(B, D, 0.0, s1 - 1.0), assert_f32("rstd", rstd), dmod0, None if dw0 is None else dw0.to(f32), want, und,
               want_dmod, want_dw, share, variants[0])


def check_dx(got, case):
    """decided elements bit for bit; undecided ones (generic rows only) within one bf16 ulp of the float64 rounding"""
    gb, wb = bits(got.contiguous()).to(torch.int32), bits(case.want_dx).to(torch.int32)
    bad = (gb != wb) & ~case.und
    far = case.und & ((gb - wb).abs() > 1)     # neighbouring bf16 numbers of one sign: bit patterns one apart
    assert not bad.any() and not far.any(), \
        f"dx: {int(bad.sum())} decided elements differ, {int(far.sum())} undecided ones are further than one ulp"


# ---- gate backward -----------------------------------------------------------------------------------------------------
Gate = namedtuple("Gate", "B L D dxn y mod dmod0 dbias0 want_dy want_dmod want_dbias")
GATE = S1


@functools.lru_cache(maxsize=None)
def gate_case(B, L, D):
    """dy = dxn gate[b], d(gate)[b] = sum_l dxn y, dbias = sum_{b, l} dy: every output exact"""
    g = _gen(3, B, L, D)
    R = B * L
    dxn, y, gate = pick(DY, (R, D), g), ints((R, D), -3, 3, g), pick(GATE, (B, D), g)
    dy = dxn * gate[torch.arange(R) // L]
    dmod0 = torch.zeros(B, 4 * D, dtype=f32)
    dmod0.view(torch.int32).fill_(SENTINEL_F32)
    i_g, dbias0 = ints((B, D), -3, 3, g), ints((D,), -3, 3, g)
    dmod0[:, 2 * D:3 * D] = i_g.to(f32)
    want_dmod = dmod0.clone()
    want_dmod[:, 2 * D:3 * D] = exact_sum("d(gate)", (dxn * y).view(B, L, D), 1, i_g)
    want_dbias = exact_sum("dbias", dy, 0, dbias0)
    want_dy = round_bf16(dy)
    assert torch.equal(want_dy.to(f64), dy)
    assert_no_sentinel("gate dy", want_dy), assert_no_sentinel("d(gate)", want_dmod[:, 2 * D:3 * D])
    mod = torch.full((B, 4 * D), float("nan"), dtype=f32)
    mod[:, 2 * D:3 * D] = gate.to(f32)
    return Gate(B, L, D, to_bf16_exact(dxn), to_bf16_exact(y), mod, dmod0, dbias0.to(f32), want_dy, want_dmod, want_dbias)


# ---- column sums -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def colsum_case(M, N, rps, roff):
    """out[n] += sum over the rows r with rps == 0 or r % rps >= roff -> (x bf16, out0 f32, want f32)"""
    g = _gen(4, M, N, rps, roff)
    x, out0 = ints((M, N), -8, 8, g), ints((N,), -3, 3, g)
    keep = torch.ones(M, dtype=torch.bool) if rps == 0 else (torch.arange(M) % rps) >= roff
    want = exact_sum("colsum", x * keep[:, None].to(f64), 0, out0)
    assert_no_sentinel("colsum", want)
    return to_bf16_exact(x), out0.to(f32), want


# ---- qkv split / RoPE / residual-V -------------------------------------------------------------------------------------
def rope_tables(L, half, g):
    """cos / sin entries from {0, +-1, +-0.5} per (table row, frequency): the kernels are linear in the table, so it need
    not be a rotation; a wrong row, frequency, half or sign changes the answer"""
    return pick(TAB, (L, half), g), pick(TAB, (L, half), g)


def rotate(x, cos, sin, inverse=False):
    """x [..., L, hd] -> y1 = x1 c + x2 s, y2 = x2 c - x1 s on the halves (the transposed rotation when inverse)"""
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    s = -sin if inverse else sin
    return torch.cat([x1 * cos + x2 * s, x2 * cos - x1 * s], -1)


def pad_columns(hd, hdp):
    """(k ones columns, v ones columns) of a head row; the rest of the pad is zero"""
    ones = hdp - hd >= 8
    return ([hd, hd + 1] if ones else []), ([hd, hd + 4] if ones else [])


QkvFwd = namedtuple("QkvFwd", "B L H hd hdp qkv cos sin v0 lam want_q want_k want_v")


def head_major(t, B, L, H, hd):
    """[B L, H hd] token-major -> [B, H, L, hd]"""
    return t.view(B, L, H, hd).permute(0, 2, 1, 3)


@functools.lru_cache(maxsize=None)
def qkv_fwd_case(B, L, H, hd, hdp, with_v0):
    g = _gen(5, B, L, H, hd, hdp, with_v0)
    D = H * hd
    qkv = ints((B * L, 3 * D), -4, 4, g)
    cos, sin = rope_tables(L, hd // 2, g)
    lam = LAM[(B + L + H) % 2]
    v0 = torch.zeros(B, H, L, hdp, dtype=f64)
    v0[..., :hd] = ints((B, H, L, hd), -4, 4, g)
    outs = []
    kcols, vcols = pad_columns(hd, hdp)
    for which, ones in ((0, []), (1, kcols), (2, vcols)):
        x = head_major(qkv[:, which * D:(which + 1) * D], B, L, H, hd)
        o = torch.zeros(B, H, L, hdp, dtype=f64)
        if which < 2:
            o[..., :hd] = rotate(x, cos, sin)
        else:
            o[..., :hd] = lam * x + (1.0 - lam) * v0[..., :hd] if with_v0 else x
        for c in ones:
            o[..., c] = 1.0
        # (no "+ 0.0" here: a zero keeps the sign IEEE gives x1 c + x2 s -- minus when both products are -0 -- and the
        # kernels, fused or not, give the same)
        r = round_bf16(o)
        assert torch.equal(r.to(f64), o), "qkv forward: every output must be a bf16 number"
        assert_no_sentinel("qkv forward", r)
        outs.append(r)
    return QkvFwd(B, L, H, hd, hdp, to_bf16_exact(qkv), cos.to(f32), sin.to(f32), to_bf16_exact(v0) if with_v0 else None,
                  torch.tensor([lam], dtype=bf16), *outs)


QkvBwd = namedtuple("QkvBwd", "B L H hd hdp mix add_dv0 dq dk dv cos sin qkv_raw v0 lam acc0 dlam0 want_dqkv want_acc want_dlam")


@functools.lru_cache(maxsize=None)
def qkv_bwd_case(B, L, H, hd, hdp, mix, add_dv0):
    """dqkv = [inverse rotation of dq | of dk | lam dv (mix) or dv + dv0_acc (add_dv0) or dv];  mix == 1:
    dv0_acc += (1 - lam) dv;  mix != 0: dlam += sum dv (v_raw - v0).  The pad columns of dq / dk / dv / v0 are NaN (no
    kernel may read them) and those of dv0_acc hold the sentinel (no kernel may write them)."""
    g = _gen(6, B, L, H, hd, hdp, mix, add_dv0)
    D = H * hd
    cos, sin = rope_tables(L, hd // 2, g)
    lam = LAM[(B + L + H + mix) % 2]

    def heads(lo, hi):
        t = torch.full((B, H, L, hdp), float("nan"), dtype=f64)
        t[..., :hd] = ints((B, H, L, hd), lo, hi, g)
        return t
    dq, dk, dv, v0 = heads(-4, 4), heads(-4, 4), heads(-4, 4), heads(-4, 4)
    qkv_raw = ints((B * L, 3 * D), -4, 4, g)
    acc0 = heads(-8, 8)
    dlam0 = 5.0

    def token_major(t):
        return t.permute(0, 2, 1, 3).reshape(B * L, D)
    dvd = dv[..., :hd]
    want_acc, want_dlam = acc0[..., :hd].clone(), dlam0
    if mix:
        out_v = lam * dvd
        if mix == 1:
            want_acc = want_acc + (1.0 - lam) * dvd
        vraw = head_major(qkv_raw[:, 2 * D:], B, L, H, hd)
        terms = dvd * (vraw - v0[..., :hd])
        assert float(terms.abs().sum()) + dlam0 < 2 ** 24, "dlam needs more than 24 bits"
        want_dlam = dlam0 + float(terms.sum())
    else:
        out_v = dvd + acc0[..., :hd] if add_dv0 else dvd
    dqkv = torch.cat([token_major(rotate(dq[..., :hd], cos, sin, True)), token_major(rotate(dk[..., :hd], cos, sin, True)),
                      token_major(out_v)], 1)   # (zeros keep their IEEE sign, as in the forward)
    want = round_bf16(dqkv)
    assert torch.equal(want.to(f64), dqkv), "qkv backward: every output must be a bf16 number"
    assert_no_sentinel("dqkv", want)
    acc_f32 = torch.zeros(B, H, L, hdp, dtype=f32)
    acc_f32.view(torch.int32).fill_(SENTINEL_F32)
    want_acc_f32 = acc_f32.clone()
    acc_f32[..., :hd], want_acc_f32[..., :hd] = assert_f32("dv0_acc", acc0[..., :hd]), assert_f32("dv0_acc", want_acc)
    nanb = lambda t: t.to(bf16)   # noqa: E731  (NaN pad: not a to_bf16_exact round trip)
    for t in (dq, dk, dv, v0):
        assert torch.equal(nanb(t)[..., :hd].to(f64), t[..., :hd])
    return QkvBwd(B, L, H, hd, hdp, mix, add_dv0, nanb(dq), nanb(dk), nanb(dv), cos.to(f32), sin.to(f32),
                  to_bf16_exact(qkv_raw), nanb(v0), torch.tensor([lam], dtype=bf16), acc_f32,
                  torch.tensor([dlam0], dtype=f32), want, want_acc_f32, torch.tensor([want_dlam], dtype=f32))


@functools.lru_cache(maxsize=None)
def rope_apply_case(B, H, L, hd, inverse):
    """-> (x bf16 [B, H, L, hd], cos, sin f32, want bf16)"""
    g = _gen(7, B, H, L, hd, inverse)
    x = ints((B, H, L, hd), -4, 4, g)
    cos, sin = rope_tables(L, hd // 2, g)
    y = rotate(x, cos, sin, bool(inverse))
    want = round_bf16(y)
    assert torch.equal(want.to(f64), y)
    assert_no_sentinel("rope_apply", want)
    return to_bf16_exact(x), cos.to(f32), sin.to(f32), want


# ---- windows -----------------------------------------------------------------------------------------------------------
GUARD_ROWS, GAP = 4, 8


def guard_of(t):
    """guard band of a contiguous tensor: four of its rows, at least 64 elements, a multiple of 8 (16-byte alignment)"""
    return max(64, -(-GUARD_ROWS * t.shape[-1] // 8) * 8)


def guarded(t, fill):
    """a contiguous tensor between two guard bands (for the tensors whose ABI takes no stride):
    -> (flat parent, view shaped like t, guard)"""
    guard = guard_of(t)
    flat = fill_value(t.dtype, fill).repeat(t.numel() + 2 * guard)
    view = flat[guard:guard + t.numel()].view(t.shape)
    view.copy_(t)
    return flat, view, guard


def assert_guarded(parent_after, parent_before, want, what, exact=True):
    """the payload equals `want` bit for bit (exact) and the guard bands are what they were; returns the payload"""
    after, before = parent_after.cpu(), parent_before.cpu()
    n, guard = want.numel(), guard_of(want)
    assert after.numel() == n + 2 * guard
    got = after[guard:guard + n].view(want.shape)
    if exact:
        diff = bits(got) != bits(want.contiguous())
        if diff.any():
            idx = tuple(int(v) for v in diff.nonzero()[0])
            raise AssertionError(f"{what}: {int(diff.sum())} of {n} elements differ, first at {idx}: got "
                                 f"{got[idx].item()!r} want {want[idx].item()!r}")
    assert torch.equal(bits(after[:guard]), bits(before[:guard])) and \
        torch.equal(bits(after[guard + n:]), bits(before[guard + n:])), f"{what}: a guard band changed"
    return got
