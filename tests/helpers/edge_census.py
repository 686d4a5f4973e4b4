"""Exact census of the step-edge kernels (csrc/elementwise.hip): inputs, float64 expectations, dispatch predicates, lists.

What runs at the two ends of a training or sampling step -- the small-M linears (five kernels), the timestep embedding,
patchify / unpatchify, the register rows, noising, the flow loss and its backward entries, the sampler's Euler step, the
two casts and the RoPE row gather -- pinned element by element, as gemm_census.py pins the GEMM and row_census.py the
row kernels.  Everything here runs on the CPU with torch alone; the GPU test compares bits.  A builder never skips a
case: it ASSERTS the property that makes its comparison legitimate and raises otherwise.

Small linears, act_in = 0.  x and dy are fp32, W and bias bf16, all of them dyadic: x a multiple of 1/4 up to 1/2, W and
dy signs times {1/2, 1} (W) and {1/2, 1, 2} (dy), bias and the initial dx multiples of 1/8.  A few entries per row of x
are WIDE: 1 + 2^-8 + g with g the finest granule the sums still hold, so that the MFMA forward's (hi, mid, lo) bf16
split of x has three nonzero terms wherever K allows.  `exact_fit` asserts that every sum of magnitudes stays below
2^24 granules: every product and every fp32 partial sum is then exact in any order -- lanes, the butterfly, the three
MFMAs per K step, the LDS reduction of dx, atomics, the deterministic partials -- and y, dW, dbias and dx have ONE right
answer each.

Small linears, act_in = 1.  SiLU is x / (1 + __expf(-x)) and its derivative s (1 + x (1 - s)), s = 1 / (1 + __expf(-x))
(common.h:53-57); neither is exact.  x has at most 8 nonzero entries per row and per column (silu(0) = 0 and
silu'(0) = 1/2 are exact), placed on the edges of the kernels' loops, 0.5 <= |x| <= 4; |W|, |dy| in {1/2, 1, 2}.
Per-element bound against float64:
      |got - want| <= REL_SILU sum|terms| + (n_terms + 1) 2^-24 sum|terms|,        REL_SILU = 2^-20
with `terms` the addends that are summed inexactly: W silu(x) (and the bias) for y, dy silu(x) for dW, and for dx the
partial sums of its ny row ranges times silu'(x) -- |sum_n dy W| s (1 + |x| (1 - s)) when ny = 1.
Where REL_SILU comes from: on |x| <= 4 the product x log2(e) that __expf forms is rounded once (half an ulp of a number
up to 5.8: |x| 2^-24 relative to the exponential, 4 x 2^-24 at most), the hardware exponential is good to about one
ulp, the add and the divide cost one ulp each, the derivative adds a multiply, a subtract and a multiply-add: about
14 x 2^-24 in all, rounded up to 16 x 2^-24 = 2^-20.  The second term of the bound is the fp32 rounding of each addend
and of the running sum.  With at most 9 addends the bound stays below 1e-5 of the sum of their magnitudes (1.6e-6 of
it) while a dropped or doubled addend moves the result by at least 0.035, the smallest |W silu(x)|: `act_case` asserts
smallest |term| > 4 x bound for every element.

Flow loss.  d = out - v is one of +-1/8, +-1/4, +-1/2 (never zero: a skipped or doubled element changes the sum), v and
out are multiples of 1/8 below 16.5, so every d^2 is a multiple of 2^-6 and every partial sum exact in any order.

The movers (patchify, registers, noising, the Euler step, the casts, the RoPE gather) have one right answer by
construction; the timestep embedding goes through `decide` like the inexact intermediates of row_census.py.
"""
import functools
import math
from collections import namedtuple

import torch

import gemm_census as G
import row_census as R
from oracle import dit_oracle as O

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
bits = G.bits

REL_SILU = 2.0 ** -20        # relative error of silu_f / dsilu_f (derivation above)
U24 = 2.0 ** -24             # half an fp32 ulp, relative
UNDECIDED_CAP = 0.01         # flow-loss gradients and the timestep embedding: largest undecided share
SL_DX_ROWS = 384             # rows of W per LDS slice of small_linear_dx_kernel
LDS_BYTES = 160 * 1024


def gen(*key):
    return R._gen(*key)


def signs(shape, g):
    return torch.randint(0, 2, tuple(shape), generator=g).to(f64) * 2.0 - 1.0


# ---- dispatch predicates of the small linears (restated from elementwise.hip) ------------------------------------------
def mfma_rule(M, N, K, knob=1):
    """small_linear_fwd_mfma: the MFMA forward serves the launch (knob adaln_mfma)"""
    return bool(knob) and M <= 16 and K % 32 == 0 and N % 16 == 0 and N >= 1024 and 48 * (2 * K + 16) <= LDS_BYTES


def fwd_instance(m):
    """the template argument of small_linear_fwd_kernel / _dx_kernel / _dw_tile_kernel for m <= 16 rows"""
    assert 1 <= m <= 16
    return 4 if m <= 4 else 8 if m <= 8 else 16


def chunks(M):
    """vds_small_linear_fwd / _bwd (dx): rows per launch"""
    return [min(16, M - r0) for r0 in range(0, M, 16)]


def fwd_kernels(M, N, K, knob=1):
    """kernel of every launch of vds_small_linear_fwd"""
    return ["mfma" if mfma_rule(m, N, K, knob) else f"row<{fwd_instance(m)}>" for m in chunks(M)]


def mfma_shape(N, K):
    """(workgroups, live waves of the last one, unrolled trips of six K steps, tail steps)"""
    wgs = (N // 16 + 7) // 8
    return wgs, N // 16 - (wgs - 1) * 8, (K // 32) // 6, (K // 32) % 6


def row_trips(K):
    """16-byte chunks of a row of W over the 64 lanes of small_linear_fwd_kernel: (chunks, full trips, lanes of the last)"""
    c = K // 8
    return c, c // 64, c % 64


def dx_split(N, K, nb=None):
    """grid of small_linear_dx_kernel -> (gx, ny, rows per workgroup, LDS slices per workgroup); nb = None: per-set
    (budget 512 workgroups), else batched over nb sets (budget 2048)"""
    gx = (K // 8 + 7) // 8
    g, budget = (gx, 512) if nb is None else (gx * nb, 2048)
    ny = max(1, min((N + 31) // 32, (budget + g - 1) // g))
    rows = ((N + ny - 1) // ny + 31) // 32 * 32
    ny = (N + rows - 1) // rows
    return gx, ny, rows, (min(rows, N) + SL_DX_ROWS - 1) // SL_DX_ROWS


def dx_workspace_floats(M, N, K, nb=None):
    """the deterministic partials the entry asks vds_set_deterministic's workspace for"""
    ny = dx_split(N, K, nb)[1]
    return ny * 16 * K if nb is None else nb * ny * M * K


def dw_grid(N, K):
    """small_linear_dw_kernel: (threads with work, workgroups)"""
    n = (N + 3) // 4 * (K // 8)
    return n, (n + 255) // 256


def dw_tile_grid(N, K, nb):
    return (K + 127) // 128, (N + 63) // 64, nb


# ---- shape lists ---------------------------------------------------------------------------------------------------------
MFMA_N = (1024, 1040)                      # full workgroups; a last workgroup with ONE live wave behind the barrier
MFMA_K = (32, 160, 192, 224, 416, 1696)    # K / 32 = 1 5 6 7 13 53: below / at / above the 6-step unroll, 2 trips + 1
MFMA_K_FALLBACK = 1728                     # 48 (2 K + 16) > 160 KiB: the row kernel serves it
MS = (1, 4, 5, 8, 9, 16)
ROW_N = (1, 3, 4, 5, 17, 203)
ROW_K = (8, 504, 512, 520)                 # 1 chunk; 63, 64, 65 chunks over 64 lanes
ROW_M_CHUNKED = (17, 33)                   # 16 + 1, 16 + 16 + 1
DW_N, DW_K, DW_M = (1, 5, 70), (8, 72), (1, 16, 17)
TILE_NK = ((4, 8), (64, 128), (68, 136))
TILE_NB = (1, 3)
TILE_M = (3, 4, 5, 8, 9, 16)
DX_N, DX_K = (17, 33, 70), (8, 72)        # ny 1 (the split gives 33 rows two ranges already), 2 and 3 with a ragged last one
DX_BIG = (5, 1600, 8192)                   # per-set: ny 4, 416 rows per workgroup: two LDS slices
DX_BIG_BATCHED = (5, 800, 4096, 16)        # batched, 16 pointers over two matrices: ny 2, 416 rows


def _cyc(seq, i):
    return seq[i % len(seq)]


def fwd_plan():
    """(M, N, K, with_bias) of vds_small_linear_fwd: every K with both N, every M at the unroll edge, the fallback, the
    row kernel's N x K with M walking the instances and the chunked M"""
    plan = []
    for i, K in enumerate(MFMA_K + (MFMA_K_FALLBACK,)):
        for j, N in enumerate(MFMA_N):
            plan.append((_cyc(MS, 2 * i + j), N, K, (i + j) % 2 == 0))
    for i, M in enumerate(MS):
        plan += [(M, 1040, 192, i % 2 == 1), (M, 1024, 224, i % 2 == 0)]
    allm = MS + ROW_M_CHUNKED
    i = 0
    for N in ROW_N:
        for K in ROW_K:
            plan.append((_cyc(allm, i), N, K, i % 2 == 0))
            i += 1
    for i, M in enumerate(allm):
        plan.append((M, 17, 72, i % 2 == 1))
    plan += [(17, 1024, 192, True), (33, 1040, 32, False)]   # chunked rows through the MFMA kernel
    return plan


def dw_plan():
    """(M, N, K, with_dbias) of the dW-only call of vds_small_linear_bwd"""
    return [(M, N, K, db) for N in DW_N for K in DW_K for M in DW_M for db in (False, True)]


def dx_plan():
    """(M, N, K) of the dx calls of vds_small_linear_bwd (the big one apart)"""
    allm = MS + ROW_M_CHUNKED
    plan, i = [], 0
    for N in DX_N:
        for K in DX_K:
            for _ in range(2):
                plan.append((_cyc(allm, i), N, K))
                i += 1
    return plan


def tile_plan():
    """(M, N, K, nb, with_dbias) of the dW call of vds_small_linear_bwd_batched"""
    plan, i = [], 0
    for N, K in TILE_NK:
        for nb in TILE_NB:
            for _ in range(2):
                plan.append((_cyc(TILE_M, i), N, K, nb, i % 2 == 0))
                i += 1
    return plan


BATCHED_FWD = [(5, 1040, 192, 3, True), (9, 1024, 224, 2, False), (4, 17, 72, 3, True), (16, 203, 8, 2, False)]
BATCHED_DX = [(4, 70, 72, 3), (9, 33, 8, 1), (16, 70, 8, 2)]
ACT_FWD = [(5, 1040, 224, True), (16, 1024, 1696, False), (9, 17, 520, True), (33, 203, 72, False), (1, 5, 8, True)]
ACT_BWD = [(5, 70, 72), (16, 33, 8), (17, 70, 520), (1, 5, 8)]
ACT_BATCHED = [(5, 68, 136, 3), (16, 64, 128, 1), (4, 70, 72, 2)]


def linear_coverage():
    """branch -> shapes that reach it (the values are asserted non-empty by test_edge_census_cpu.py)"""
    fwd = fwd_plan()
    cov = {}

    def put(name, shapes):
        cov[name] = sorted(set(shapes))

    mf = [(M, N, K) for M, N, K, _ in fwd if all(k == "mfma" for k in fwd_kernels(M, N, K))]
    put("mfma: every workgroup full (N 1024)", [s for s in mf if mfma_shape(s[1], s[2])[:2] == (8, 8)])
    put("mfma: last workgroup with one live wave (N 1040)", [s for s in mf if mfma_shape(s[1], s[2])[1] == 1])
    for name, pred in (("below the unroll, tail only", lambda u, t: u == 0 and t > 0), ("one unrolled trip, no tail", lambda u, t: (u, t) == (1, 0)),
                       ("one trip + tail", lambda u, t: u == 1 and t > 0), ("two trips + tail of one", lambda u, t: (u, t) == (2, 1)),
                       ("largest K in LDS (1696)", lambda u, t: (u, t) == (8, 5))):
        put("mfma K/32: " + name, [s for s in mf if pred(*mfma_shape(s[1], s[2])[2:])])
    put("mfma: K 1728 falls back to the row kernel", [(M, N, K) for M, N, K, _ in fwd if K == MFMA_K_FALLBACK and N >= 1024
                                                     and not mfma_rule(M, N, K) and mfma_rule(M, N, 1696)])
    for m in MS:
        put(f"mfma: M {m}", [s for s in mf if s[0] == m])
    put("mfma: with bias", [(M, N, K) for M, N, K, b in fwd if b and mfma_rule(min(M, 16), N, K)])
    put("mfma: without bias", [(M, N, K) for M, N, K, b in fwd if not b and mfma_rule(min(M, 16), N, K)])
    put("mfma: chunked rows (M > 16)", [(M, N, K) for M, N, K, _ in fwd if M > 16 and mfma_rule(16, N, K)])
    row = [(M, N, K) for M, N, K, _ in fwd if not mfma_rule(min(M, 16), N, K)]
    for inst in (4, 8, 16):
        put(f"row<{inst}>", [s for s in row if f"row<{inst}>" in fwd_kernels(*s)])
    for n in ROW_N:
        put(f"row: N {n} (N % 4 = {n % 4}, {(n + 15) // 16} workgroups)", [s for s in row if s[1] == n])
    for k in ROW_K:
        put("row: K %d (%d chunks: %d full trips + %d lanes)" % ((k,) + row_trips(k)), [s for s in row if s[2] == k])
    for m in ROW_M_CHUNKED:
        put(f"row: M {m} in chunks {chunks(m)}", [s for s in row if s[0] == m])
    dw = dw_plan()
    for n in DW_N:
        put(f"dw: N {n}", [s[:3] for s in dw if s[1] == n])
    for k in DW_K:
        put(f"dw: K {k}", [s[:3] for s in dw if s[2] == k])
    for m in DW_M:
        put(f"dw: M {m} (one launch)", [s[:3] for s in dw if s[0] == m])
    put("dw: several workgroups", [s[:3] for s in dw if dw_grid(s[1], s[2])[1] > 1] + [s for s in ACT_BWD if dw_grid(s[1], s[2])[1] > 1])
    put("dw: dbias NULL", [s[:3] for s in dw if not s[3]])
    put("dw: dbias given", [s[:3] for s in dw if s[3]])
    tl = tile_plan()
    for nk in TILE_NK:
        put("dw_tile: (N, K) %s grid %s" % (nk, dw_tile_grid(nk[0], nk[1], 1)[:2]), [s[:4] for s in tl if s[1:3] == nk])
    for nb in TILE_NB:
        put(f"dw_tile: nb {nb}", [s[:4] for s in tl if s[3] == nb])
    for m in TILE_M:
        put(f"dw_tile<{fwd_instance(m)}>: M {m}", [s[:4] for s in tl if s[0] == m])
    put("dw_tile: dbias table NULL", [s[:4] for s in tl if not s[4]])
    put("dw_tile: dbias table given", [s[:4] for s in tl if s[4]])
    dx = dx_plan()
    put("dx: dead column lanes (K/8 % 8 != 0)", [s for s in dx if (s[2] // 8) % 8])
    put("dx: ny 1", [s for s in dx if dx_split(s[1], s[2])[1] == 1])
    put("dx: ny > 1, ragged last range", [s for s in dx if dx_split(s[1], s[2])[1] > 1 and s[1] % dx_split(s[1], s[2])[2]])
    put("dx: chunked rows (M > 16)", [s for s in dx if s[0] > 16])
    for inst in (4, 8, 16):
        put(f"dx<{inst}>", [s for s in dx if inst in [fwd_instance(m) for m in chunks(s[0])]])
    put("dx: slice loop, per-set (rows > 384)", [DX_BIG] if dx_split(*DX_BIG[1:])[2:] == (416, 2) and dx_split(*DX_BIG[1:])[1] == 4 else [])
    M, N, K, nb = DX_BIG_BATCHED
    put("dx: slice loop, batched (rows > 384)", [DX_BIG_BATCHED] if dx_split(N, K, nb)[1:] == (2, 416, 2) else [])
    put("dx batched: ny > 1", [s for s in BATCHED_DX if dx_split(s[1], s[2], s[3])[1] > 1])
    put("fwd batched: mfma", [s[:4] for s in BATCHED_FWD if mfma_rule(s[0], s[1], s[2])])
    put("fwd batched: row", [s[:4] for s in BATCHED_FWD if not mfma_rule(s[0], s[1], s[2])])
    put("act_in 1: mfma", [s[:3] for s in ACT_FWD if mfma_rule(min(s[0], 16), s[1], s[2])])
    put("act_in 1: row", [s[:3] for s in ACT_FWD if not mfma_rule(min(s[0], 16), s[1], s[2])])
    put("act_in 1: dw and dx, ny > 1", [s for s in ACT_BWD if dx_split(s[1], s[2])[1] > 1])
    put("act_in 1: dw_tile and batched dx", ACT_BATCHED)
    return cov


# ---- small linears: exact operands ---------------------------------------------------------------------------------------
def exact_fit(what, abs_sum, gran):
    """every partial sum of addends that are multiples of `gran` is an fp32 number when the magnitudes sum below 2^24 gran"""
    worst = float(abs_sum.max()) / gran
    assert worst < 2 ** 24, f"{what}: a sum needs {math.log2(worst):.1f} bits"


def multiples(what, t, gran):
    q = t / gran
    assert torch.equal(q, q.round()), f"{what}: not multiples of 2^{int(math.log2(gran))}"


def wide_granule(M, K):
    """finest granule g of a wide x entry: the row sums of |x W| (<= K / 2 + a few) and the column sums of |dy x| (<= 2.1 M)
    must stay below 2^24 of g / 2; 2^-18 at most (1 + 2^-8 + g then has three nonzero bf16 terms: 1 + 2^-7, -2^-8, g)"""
    bound = max(K // 2 + 16, 3 * M)
    return 2.0 ** -min(18, 23 - math.ceil(math.log2(bound)))


def split3(x64):
    """the MFMA forward's (hi, mid, lo) bf16 terms of an fp32 number"""
    rem, out = x64.to(f32), []
    for _ in range(3):
        p = rem.to(bf16).to(f32)
        out.append(p)
        rem = rem - p
    return out, rem


Linear = namedtuple("Linear", "M N K nb x W bias dy dx0 y dW dbias dx terms3")


@functools.lru_cache(maxsize=8)
def linear_case(M, N, K, nw=1, with_bias=True, nb=None, want_dw=True):
    """act_in = 0.  nw distinct weight matrices; set i of a batched call (nb sets) uses matrix i % nw.  y [sets, M, N],
    dW [sets, N, K] (None without want_dw: the large dx cases), dbias [sets, N]; dx [M, K] accumulates over all sets from
    dx0."""
    sets = 1 if nb is None else nb
    g = gen(M, N, K, nw, sets, 71)
    x = torch.randint(-2, 3, (M, K), generator=g).to(f64) / 4.0
    gw = wide_granule(M, K)
    wide = (1.0 + 2.0 ** -8 + gw)
    for b in range(M):   # three wide entries per row: first and last chunk and one inside
        for j, k in enumerate(sorted({0, K - 1, (37 * b + 11) % K})):
            x[b, k] = wide * (1.0 if (b + j) % 2 else -1.0)
    W = signs((nw, N, K), g) * R.pick((0.5, 1.0), (nw, N, K), g)
    bias = R.ints((nw, N), -16, 16, g) / 8.0 if with_bias else None
    dy = signs((sets, M, N), g) * R.pick((0.5, 1.0, 2.0), (sets, M, N), g)
    dx0 = R.ints((M, K), -16, 16, g) / 8.0
    dx0[dx0 == 0] = 0.375
    what = f"linear M {M} N {N} K {K} nw {nw} nb {nb}"
    multiples(what + " x", x, gw)
    assert torch.equal(x.to(f32).to(f64), x)
    # forward: products are multiples of gw / 2; the bias joins the same sum
    # (1.02: the magnitudes of the three bf16 terms of a wide entry add up to a little more than the entry)
    absy = 1.02 * (x.abs() @ W.abs().amax(0).t()) + (bias.abs().amax(0) if with_bias else 0.0)
    exact_fit(what + " y", absy, gw / 2)
    # dW: M addends dy x, multiples of gw / 2;  dbias: M addends of dy
    exact_fit(what + " dW", dy.abs().amax(0).t().amax(0, keepdim=True).t() * x.abs().sum(0, keepdim=True), gw / 2)
    # dx: dx0 + sum over sets and n of dy W, multiples of 1/8 (products: 1/4)
    idx = [i % nw for i in range(sets)]
    absdx = dx0.abs() + sum(sum(dy[s].abs() for s in range(sets) if s % nw == w) @ W[w].abs() for w in range(nw))
    exact_fit(what + " dx", absdx, 0.125)
    y = torch.stack([x @ W[w].t() + (bias[w] if with_bias else 0.0) for w in idx]) + 0.0
    dW = torch.stack([dy[s].t() @ x for s in range(sets)]) + 0.0 if want_dw else None
    dbias = dy.sum(1) + 0.0
    dx = dx0 + sum(sum(dy[s] for s in range(sets) if s % nw == w) @ W[w] for w in range(nw))
    terms, rem = split3(x)
    assert not rem.any(), what + ": x is not the sum of three bf16 terms"
    n3 = sum(int((t != 0).any()) for t in terms)
    return Linear(M, N, K, nb, x.to(f32), G.to_bf16_exact(W), G.to_bf16_exact(bias) if with_bias else None, dy.to(f32),
                  R.assert_f32(what + " dx0", dx0), R.assert_f32(what + " y", y),
                  R.assert_f32(what + " dW", dW) if want_dw else None,
                  R.assert_f32(what + " dbias", dbias), R.assert_f32(what + " dx", dx), n3)


# ---- small linears: SiLU operands ----------------------------------------------------------------------------------------
def silu64(x):
    return x / (1.0 + torch.exp(-x))


def dsilu64(x):
    s = 1.0 / (1.0 + torch.exp(-x))
    return s * (1.0 + x * (1.0 - s))


def edge_columns(K):
    """columns on the edges of the kernels' loops: 0, K - 1, both sides of every 8- (first and last), 32- and 192-
    element boundary (the chunk, the MFMA K step, the unrolled trip), and one per 128-column tile (dw_tile)"""
    cols = {0, K - 1}
    for step in (32, 192):
        for e in range(step, K, step):
            cols |= {e - 1, e}
    for e in (8, K - 8):
        if 0 < e < K:
            cols |= {e - 1, e}
    cols |= {t + 77 % max(1, min(128, K - t)) for t in range(0, K, 128)}
    return sorted(c for c in cols if 0 <= c < K)


def sparse_x(M, K, g):
    """<= 8 nonzero entries per row AND per column, on edge_columns(K), 0.5 <= |x| <= 4, generic fp32 values"""
    edges = edge_columns(K)
    cols = edges
    if 8 * M < len(cols):   # fewer slots than edges: an evenly spaced choice of them that keeps the first and the last
        cols = sorted({cols[round(i * (len(cols) - 1) / max(1, 8 * M - 1))] for i in range(8 * M)})
    x = torch.zeros(M, K, dtype=f64)
    per_col = {c: 0 for c in cols}
    for b in range(M):
        n = 0
        for j in range(len(cols)):
            c = cols[(b * len(cols) // M + j) % len(cols)]     # the rows' runs of 8 start len / M apart: they tile the list
            if n < 8 and per_col[c] < 8 and x[b, c] == 0:
                mag = 0.5 + 3.5 * float(torch.rand((), generator=g, dtype=f64))
                x[b, c] = mag if (b + j) % 3 else -mag
                per_col[c] += 1
                n += 1
    x = x.to(f32).to(f64)
    nz = x != 0
    assert int(nz.sum(1).max()) <= 8 and int(nz.sum(0).max()) <= 8
    assert nz[:min(M, len(cols))].any(1).all(), "a row without a nonzero entry"
    used = set(nz.any(0).nonzero().flatten().tolist())
    assert used == set(cols) and {0, K - 1} <= used, f"K {K} M {M}: edges without a nonzero x: {sorted(set(cols) - used)}"
    assert used == set(edges) or 8 * M < len(edges)
    assert float(x[nz].abs().min()) >= 0.5 and float(x[nz].abs().max()) <= 4.0
    return x


Act = namedtuple("Act", "M N K nb x W bias dy y y_sum y_bound dW dW_sum dW_bound dbias dx dx_sum dx_bound margin")


@functools.lru_cache(maxsize=32)
def act_case(M, N, K, with_bias=True, nb=None):
    """act_in = 1: float64 expectations and the per-element bounds of the module docstring; dx starts from zero (its
    bound has no room for the rounding of a large initial value).  Batched: nb sets, nb distinct W."""
    sets = 1 if nb is None else nb
    g = gen(M, N, K, sets, 73)
    x = sparse_x(M, K, g)
    W = signs((sets, N, K), g) * R.pick((0.5, 1.0, 2.0), (sets, N, K), g)
    bias = (signs((sets, N), g) * R.pick((0.5, 1.0, 2.0), (sets, N), g)) if with_bias else None
    dy = signs((sets, M, N), g) * R.pick((0.5, 1.0, 2.0), (sets, M, N), g)
    sx, ds = silu64(x), dsilu64(x)
    nz = (x != 0).to(f64)
    what = f"act M {M} N {N} K {K} nb {nb}"
    # y: addends W silu(x) over the nonzero columns of the row, and the bias
    y = torch.stack([sx @ W[s].t() + (bias[s] if with_bias else 0.0) for s in range(sets)])
    sum_y = torch.stack([sx.abs() @ W[s].abs().t() + (bias[s].abs() if with_bias else 0.0) for s in range(sets)])
    n_y = nz.sum(1)[None, :, None] + (1.0 if with_bias else 0.0)
    y_bound = (REL_SILU + (n_y + 1.0) * U24) * sum_y
    # dW: addends dy silu(x) over the rows whose x is nonzero in that column (none: an exact zero)
    dW = torch.stack([dy[s].t() @ sx for s in range(sets)])
    sum_w = torch.stack([dy[s].abs().t() @ sx.abs() for s in range(sets)])
    dW_bound = (REL_SILU + (nz.sum(0)[None, None, :] + 1.0) * U24) * sum_w
    dbias = R.assert_f32(what + " dbias", dy.sum(1) + 0.0)
    # dx: the exact partial sums of the ny row ranges, each times silu'(x), meet in atomics
    gx, ny, rows, _ = dx_split(N, K, nb)
    parts = torch.stack([dy[s][:, r0:r0 + rows] @ W[s][r0:r0 + rows] for s in range(sets) for r0 in range(0, N, rows)])
    assert parts.shape[0] == sets * ny
    exact_fit(what + " dx partials", parts.abs(), 0.25)
    mag = 1.0 / (1.0 + torch.exp(-x))
    mag = mag * (1.0 + x.abs() * (1.0 - mag))          # s (1 + |x| (1 - s)) >= |silu'(x)|
    dx = parts.sum(0) * ds
    sum_x = parts.abs().sum(0) * mag
    dx_bound = (REL_SILU + (parts.shape[0] + 1.0) * U24) * sum_x
    # a dropped or doubled addend must show: the smallest addend against four times the bound
    m_y = float((W.abs().min() * sx[x != 0].abs().min()) / (4.0 * y_bound.max()))
    live = sum_w > 0
    m_w = float((dy.abs().min() * sx[x != 0].abs().min()) / (4.0 * dW_bound[live].max()))
    m_x = float((0.25 * mag / (4.0 * dx_bound.clamp(min=1e-300)))[parts.abs().sum(0) > 0].min())   # one (dy W) of 1/4 times the factor
    assert min(m_y, m_w, m_x) > 1.0, f"{what}: smallest addend over 4 x bound: y {m_y:.1f} dW {m_w:.1f} dx {m_x:.1f}"
    assert float((y_bound / sum_y.clamp(min=1e-300)).max()) < 1e-5 and float((dW_bound[live] / sum_w[live]).max()) < 1e-5
    return Act(M, N, K, nb, x.to(f32), G.to_bf16_exact(W), G.to_bf16_exact(bias) if with_bias else None, dy.to(f32),
               y, sum_y, y_bound, dW, sum_w, dW_bound, dbias, dx, sum_x, dx_bound, min(m_y, m_w, m_x))


def within(what, got, want64, bound, scale):
    """|got - want| <= bound element by element -> the worst error in fp32 ulps of `scale`, the sum of the magnitudes of
    the element's addends (a sum that cancels has no ulp of its own to measure with); REL_SILU is 8 to 16 of them"""
    err = (got.to(f64) - want64).abs()
    bad = err > bound
    if bad.any():
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, first at {idx}: got "
                             f"{got[idx].item()!r} want {want64[idx].item()!r} bound {bound[idx].item():.3e}")
    live = scale > 0
    if not live.any():
        return 0.0
    s32 = scale[live].to(f32)
    ulp = (torch.nextafter(s32, torch.full_like(s32, float("inf"))) - s32).to(f64)
    return float((err[live] / ulp).max())


# ---- flow loss -----------------------------------------------------------------------------------------------------------
def flow_loss_bps(per):
    """workgroups per sample (or per token-frame) of stage 1"""
    return max(1, min(256, (per + 4095) // 4096))


def loss_branches(per):
    """stage 1 walks a sample in strides of bps * 256 elements: `strides` full ones and `rest` elements of a last, partly
    filled one; stage 2 sums the bps partials in `lane_trips` trips of 64 lanes"""
    bps, want = flow_loss_bps(per), (per + 4095) // 4096
    return dict(bps=bps, capped=want > 256, lane_trips=(bps + 63) // 64, strides=per // (bps * 256), rest=per % (bps * 256))


LOSS_PER = (8, 4096, 4097, 262144, 262145, 1048576, 1048576 + 4097)
LOSS_B = (1, 3)
LOSS_B5_PER = (8, 4096, 4097)              # B = 5: one wave of stage 2 serves samples 0 and 4
FRAMES = [(5, 6, 21, 2), (16, 4, 136, 2), (16, 2, 16512, 1), (5, 6, 21, 1), (5, 6, 21, 3), (5, 2, 21, 2)]   # (C, T, HW, tps)
FRAMES_BWD = FRAMES[:2]
LOSS_BWD_N = (8, 8 * 255, 8 * 256 * 2048, 8 * (256 * 2048 + 3))
WEIGHTS = (0.0, 0.5, 1.0, 2.0)


def loss_plan():
    return [(B, per) for per in LOSS_PER for B in LOSS_B] + [(5, per) for per in LOSS_B5_PER]


def frames_plan():
    return [(B, C, T, HW, tps) for C, T, HW, tps in FRAMES for B in LOSS_B] + [(5,) + FRAMES[0]]


def loss_partials(sq_row, per):
    """stage 1 of the flow loss restated: the partial of workgroup x is the sum over the elements i with
    (i // 256) % bps == x"""
    bps = flow_loss_bps(per)
    pad = (-per) % (bps * 256)
    return torch.cat([sq_row, torch.zeros(pad, dtype=sq_row.dtype)]).reshape(-1, bps, 256).sum((0, 2))


def loss_bwd_blocks(n):
    """(workgroups, trips of the grid-stride loop) of flow_loss_bwd_kernel"""
    blocks = min(2048, (n // 8 + 255) // 256)
    return blocks, (n // 8 + blocks * 256 - 1) // (blocks * 256)


def loss_coverage():
    cov = {}
    plan = loss_plan()
    for name, pred in (("bps 1, one partial wave", lambda d: d["bps"] == 1),
                       ("bps 2, one element past the full strides", lambda d: d["bps"] == 2 and d["rest"] == 1),
                       ("bps 64: one lane trip of stage 2", lambda d: d["bps"] == 64),
                       ("bps 65: two lane trips of stage 2", lambda d: d["bps"] == 65 and d["lane_trips"] == 2),
                       ("bps 256 exactly, full strides only", lambda d: d["bps"] == 256 and not d["capped"] and d["rest"] == 0),
                       ("bps capped at 256, a partly filled last stride", lambda d: d["capped"] and d["rest"] > 0)):
        cov["loss: " + name] = sorted({per for _, per in plan if pred(loss_branches(per))})
    cov["loss: B 5, a wave of stage 2 serves two samples"] = [s for s in plan if s[0] > 4]
    fr = frames_plan()
    nf = lambda s: s[1] * s[4] * s[3]   # noqa: E731
    cov["frames: channel runs straddle workgroups (n_f 210)"] = [s for s in fr if nf(s) == 210 and s[1] > 1]
    cov["frames: bps 2 (n_f 4352)"] = [s for s in fr if flow_loss_bps(nf(s)) == 2]
    cov["frames: bps 65 (n_f 264192), F 2"] = [s for s in fr if flow_loss_bps(nf(s)) == 65 and s[2] // s[4] == 2]
    for F in (1, 2, 3):
        cov[f"frames: F {F}"] = [s for s in fr if s[2] // s[4] == F]
    for tps in (1, 2, 3):
        cov[f"frames: tps {tps}"] = [s for s in fr if s[4] == tps]
    cov["frames: B 5"] = [s for s in fr if s[0] > 4]
    for name, pred in (("one workgroup, one thread", lambda n: n == 8), ("one workgroup, 255 threads", lambda n: n == 8 * 255),
                       ("2048 workgroups exactly", lambda n: loss_bwd_blocks(n) == (2048, 1) and n // 8 == 2048 * 256),
                       ("the grid-stride second trip", lambda n: loss_bwd_blocks(n) == (2048, 2))):
        cov["loss_bwd: " + name] = [n for n in LOSS_BWD_N if pred(n)]
    return cov


def _diffs(shape, g, bump):
    """d in {+-1/8, +-1/4, +-1/2}, never zero: 1/8 with a thin, case-dependent share of the larger two; the first
    bump + 1 elements are 1/2 (what tells the samples and frames of the smallest cases apart)"""
    r = torch.rand(tuple(shape), generator=g)
    mag = torch.full(tuple(shape), 0.125, dtype=f64)
    mag[r < 0.02 + 0.01 * bump] = 0.25
    mag[r < 0.004 + 0.002 * bump] = 0.5
    mag.view(-1)[:bump + 1] = 0.5
    return mag * signs(shape, g)


def _v_and_out(d, g):
    v = torch.randint(-120, 121, d.shape, generator=g).to(f64) / 8.0
    out = v + d
    return G.to_bf16_exact(v), G.to_bf16_exact(out)


def _ratio(num64, den64):
    """num / den as (float64 quotient, is it an fp32 number)"""
    q = num64 / den64
    return q, torch.equal(q.to(f32).to(f64), q) and torch.equal(q * den64, num64)


def _dout(d, k64, exact):
    """bf16(d k) -> (want, undecided mask): k exact, or moved by +- 2^-22 relative"""
    if exact:
        want = (d * k64).to(f32).to(bf16)
        return want, torch.zeros(d.shape, dtype=torch.bool)
    return R.decide([d * k64, d * k64 * (1.0 + 2.0 ** -22), d * k64 * (1.0 - 2.0 ** -22)])


def _dyadic(v):
    m, _ = math.frexp(v)
    return m * 256 == int(m * 256)


Loss = namedtuple("Loss", "B per v out sse per_sample per_exact dout und")


@functools.lru_cache(maxsize=4)
def loss_case(B, per, gscale=1.0):
    g = gen(B, per, 81)
    d = torch.cat([_diffs((1, per), g, b) for b in range(B)])
    v, out = _v_and_out(d, g)
    sq = d * d
    sse = R.exact_sum(f"loss B {B} per {per}", sq, 1, torch.zeros(B, dtype=f64)).to(f64)
    assert len(set(sse.tolist())) == B, "the samples must have different sums"
    ps, exact = zip(*[_ratio(sse[b], torch.tensor(float(per), dtype=f64)) for b in range(B)])
    k_exact = (B * per) & (B * per - 1) == 0 and _dyadic(gscale)
    den = float(torch.tensor(float(B), dtype=f32) * torch.tensor(float(per), dtype=f32))   # fl(B per), as the kernel forms it
    want, und = _dout(d, 2.0 * gscale / den, k_exact)
    return Loss(B, per, v, out, sse, torch.stack(ps), exact, want, und)


def check_per_sample(what, got, want64, exact):
    """bit-equal where the quotient is an fp32 number, else within one fp32 ulp of float64"""
    for b in range(want64.numel()):
        if exact[b]:
            assert got[b].item() == want64[b].item(), f"{what}: per_sample[{b}] {got[b].item()!r} != {want64[b].item()!r} (exact)"
        else:
            u = R.ulps32(got[b:b + 1], want64[b:b + 1])
            assert u <= 1.0, f"{what}: per_sample[{b}] is {u:.2f} fp32 ulps from float64"


def check_loss(what, got_loss, got_per_sample):
    """the batch mean from the GPU's OWN per_sample, summed in index order in fp32, divided once"""
    tot = torch.zeros((), dtype=f32)
    for b in range(got_per_sample.numel()):
        tot = tot + got_per_sample[b]
    q, exact = _ratio(tot.to(f64), torch.tensor(float(got_per_sample.numel()), dtype=f64))
    if exact:
        assert got_loss.item() == q.item(), f"{what}: loss {got_loss.item()!r} != {q.item()!r} (exact)"
    else:
        u = R.ulps32(got_loss.reshape(1), q.reshape(1))
        assert u <= 1.0, f"{what}: loss is {u:.2f} fp32 ulps from the mean of its own per_sample"


def check_dout(what, got, want, und):
    """decided elements bit-equal; the undecided share under the cap -> the share"""
    share = float(und.float().mean())
    assert share <= UNDECIDED_CAP, f"{what}: {share:.2%} of dout undecided"
    diff = (bits(got) != bits(want)) & ~und
    if diff.any():
        idx = tuple(int(v) for v in diff.nonzero()[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.numel()} decided elements of dout differ, first at {idx}: "
                             f"got {got[idx].item()!r} want {want[idx].item()!r}")
    return share


FrameLoss = namedtuple("FrameLoss", "B C T HW tps F n_f v out w acc per_sample per_exact dout und")


def frame_weights(B, F):
    """weights in {0, 1/2, 1, 2}: sample 1 (when there is one) has no weight at all, sample 0 a weightless frame when F > 1"""
    w = torch.tensor([[WEIGHTS[1 + (2 * b + f) % 3] for f in range(F)] for b in range(B)], dtype=f64)
    if F > 1:
        w[0, F - 1] = 0.0
    if B > 1:
        w[1] = 0.0
    return w


@functools.lru_cache(maxsize=4)
def frame_loss_case(B, C, T, HW, tps, gscale=1.0):
    F, n_f = T // tps, C * tps * HW
    what = f"frames B {B} C {C} T {T} HW {HW} tps {tps}"
    for salt in range(16):   # (a draw in which two frames or samples happen to have the same sum is drawn again)
        g = gen(B, C, T, HW, tps, 83, salt)
        d = torch.stack([torch.stack([_diffs((C, tps, HW), g, F * b + f) for f in range(F)], 1) for b in range(B)])  # [B,C,F,tps,HW]
        sse = R.exact_sum(what, (d * d).permute(0, 2, 1, 3, 4).reshape(B, F, n_f), 2, torch.zeros(B, F, dtype=f64)).to(f64)
        if all(len(set(sse[b].tolist())) == F for b in range(B)) and len(set(sse.sum(1).tolist())) == B:
            break
    else:
        raise AssertionError(what + ": frames / samples must have different sums")
    v, out = _v_and_out(d.reshape(B, C, T, HW), g)
    w = frame_weights(B, F)
    multiples(what + " weighted", w * sse, 2.0 ** -7)
    exact_fit(what + " weighted", (w * sse).sum(1), 2.0 ** -7)
    acc = R.assert_f32(what + " weighted", (w * sse).sum(1)).to(f64)
    wsum = w.sum(1)
    ps, exact = [], []
    for b in range(B):
        if wsum[b] > 0:
            q, e = _ratio(acc[b], torch.tensor(float(n_f), dtype=f64) * wsum[b])
        else:
            q, e = torch.zeros((), dtype=f64), True
        ps.append(q)
        exact.append(e)
    assert n_f < 2 ** 24
    want = torch.zeros(B, C, F, tps, HW, dtype=bf16)
    und = torch.zeros(B, C, F, tps, HW, dtype=torch.bool)
    for b in range(B):
        for f in range(F):
            if wsum[b] > 0 and w[b, f] > 0:
                den = float(B) * float(n_f) * float(wsum[b])
                num = 2.0 * gscale * float(w[b, f])
                k_exact = _dyadic(num) and _dyadic(den) and float(int(den)) == den and int(den) & (int(den) - 1) == 0
                want[b, :, f], und[b, :, f] = _dout(d[b, :, f], num / float(torch.tensor(den, dtype=f32)), k_exact)
    return FrameLoss(B, C, T, HW, tps, F, n_f, v, out, w.to(f32), acc, torch.stack(ps), exact,
                     want.reshape(B, C, T, HW), und.reshape(B, C, T, HW))


LossBwd = namedtuple("LossBwd", "B per n v out gloss dout und")


@functools.lru_cache(maxsize=2)
def loss_bwd_case(n, gloss=0.75):
    """vds_flow_loss_bwd over n elements: k = 2 gloss fl(1 / n)"""
    B = 3 if n % 3 == 0 else 1
    g = gen(n, 85)
    d = _diffs((n,), g, 1)
    v, out = _v_and_out(d, g)
    inv_n = float(torch.ones((), dtype=f32) / torch.tensor(float(n), dtype=f32))
    assert _dyadic(gloss) and float(torch.tensor(float(n), dtype=f32)) == n
    want, und = _dout(d, 2.0 * gloss * inv_n, n & (n - 1) == 0)
    return LossBwd(B, n // B, n, v, out, gloss, want, und)


# ---- the exact movers ----------------------------------------------------------------------------------------------------
PATCH_P = ((1, 1), (1, 2), (2, 2), (4, 2), (1, 4))    # (pt, p)
PATCH_C = (3, 16)
PATCH_THW = ((4, 6, 10), (4, 8, 8))
PATCH_B = (1, 3)
PATCH_ROWS = ((0, 0), (16, 16))                        # (register rows in front of every sample, row_offset); 0: dense


def patch_plan():
    return [(B, C, T, H, W, pt, p) for pt, p in PATCH_P for C in PATCH_C for T, H, W in PATCH_THW for B in PATCH_B
            if T % pt == 0 and H % p == 0 and W % p == 0]


def patch_coverage():
    plan = patch_plan()
    cov = {f"patch: (pt, p) {pp}": [s for s in plan if s[5:] == pp] for pp in PATCH_P}
    cov["patch: odd C"] = [s for s in plan if s[1] % 2]
    cov["patchify: grid ends inside a token"] = [s for s in plan if (s[0] * s[1] * s[2] * s[3] * s[4] // s[6]) % 256
                                                 and (256 % (s[1] * s[5] * s[6]))]
    cov["unpatchify: grid ends inside a workgroup"] = [s for s in plan if (s[0] * s[1] * s[2] * s[3] * s[4]) % 256]
    return cov


def index_values(n, salt=0):
    """n bf16 numbers whose bit patterns encode their index: finite, positive, no NaN pattern, never the sentinel"""
    assert n <= 0x7F00
    pat = (torch.arange(n, dtype=torch.int32) + 0x40 + salt) % 0x7F80
    assert len(set(pat.tolist())) == n
    t = pat.to(torch.int16).view(bf16)
    assert not torch.isnan(t.float()).any()
    R.assert_no_sentinel("index values", t)
    return t


Patch = namedtuple("Patch", "latent tokens n feat")


@functools.lru_cache(maxsize=None)
def patch_case(B, C, T, H, W, pt, p):
    """latent [B,C,T,H,W] with index values and the oracle's tokens of it [B, n, C pt p p] (patchify); the same numbers
    read as tokens [B, n, p p pt C] and their image (unpatchify)"""
    n, feat = (T // pt) * (H // p) * (W // p), C * pt * p * p
    latent = index_values(B * C * T * H * W).reshape(B, C, T, H, W)
    tokens = O.patchify(latent, pt, p).contiguous()
    assert tokens.shape == (B, n, feat)
    y = index_values(B * n * feat, salt=7).reshape(B, n, feat)
    image = O.unpatchify(y, C, T // pt, H // p, W // p, pt, p).contiguous()
    assert image.shape == (B, C, T, H, W)
    return Patch(latent, tokens, n, feat), Patch(image, y, n, feat)


def rows_parent(tokens, lead, fill):
    """[B, n, feat] tokens as rows lead .. lead + n of a [B, lead + n, feat] parent filled with `fill`"""
    B, n, feat = tokens.shape
    parent = G.fill_value(bf16, fill).repeat(B, lead + n, feat)
    parent[:, lead:] = tokens
    return parent


REG_RD = ((16, 72), (16, 128), (3, 8))
REG_B = (1, 3)


def reg_strides(R_, D):
    return (R_ * D, R_ * D + 40, (R_ + 5) * D)


Regs = namedtuple("Regs", "B R D bs reg want_x dx dreg0 want_dreg")


@functools.lru_cache(maxsize=None)
def reg_case(B, R_, D, bs):
    g = gen(B, R_, D, bs, 87)
    reg = index_values(R_ * D)
    want_x = G.fill_value(bf16, "sentinel").repeat(B, bs)
    want_x[:, :R_ * D] = reg
    dxv = R.ints((B, R_ * D), -64, 64, g) / 16.0
    dx = G.fill_value(bf16, "nan").repeat(B, bs)
    dx[:, :R_ * D] = G.to_bf16_exact(dxv)
    dreg0 = R.ints((R_ * D,), -16, 16, g) / 8.0
    dreg0[dreg0 == 0] = 0.625
    want = R.exact_sum(f"registers B {B} R {R_} D {D}", dxv, 0, dreg0)
    return Regs(B, R_, D, bs, reg, want_x, dx, R.assert_f32("dreg0", dreg0), want)


def generic_bf16(shape, g, scale=1.5):
    return (torch.randn(tuple(shape), generator=g, dtype=f32) * scale).to(bf16)


def rbf(t32):
    """one bf16 rounding of an fp32 tensor, back in fp32 (bf2f(f2bf(.)))"""
    return t32.to(bf16).to(f32)


def noise_expect(x, n, t_el):
    """noise_kernel's rounding points in fp32: (1 - t) rounds, each product rounds, the sum rounds"""
    xv, nv = x.to(f32), n.to(f32)
    omt = rbf(1.0 - t_el)
    a, c = rbf(xv * omt), rbf(nv * t_el)
    return (a + c).to(bf16), (xv - nv).to(bf16)


NOISE = [(3, 100), (1, 4097), (3, 4097), (1, 8)]
NOISE_T = (0.0, 1.0, 0.3, 1.0 / 3.0, 0.7431640625, 0.999)     # 0, 1, fp32 numbers that are no bf16 numbers
NOISE_FRAMES = [(B, 5, 6, 21, tps) for tps in (1, 2, 3) for B in (1, 3)]


def noise_t(count, salt):
    return torch.tensor([NOISE_T[(i + salt) % len(NOISE_T)] for i in range(count)], dtype=f32)


@functools.lru_cache(maxsize=None)
def noise_case(B, per):
    g = gen(B, per, 89)
    x, n = generic_bf16((B, per), g), generic_bf16((B, per), g)
    t = noise_t(B, per % 5)     # (3, 100): t = (0, 1, 0.3); the others start further down the list
    zt, v = noise_expect(x, n, t[:, None])
    return x, n, t, zt, v


@functools.lru_cache(maxsize=None)
def noise_frames_case(B, C, T, HW, tps):
    g = gen(B, C, T, HW, tps, 91)
    x, n = generic_bf16((B, C, T, HW), g), generic_bf16((B, C, T, HW), g)
    F = T // tps
    t = noise_t(B * F, tps).reshape(B, F)
    t_el = t.repeat_interleave(tps, dim=1)[:, None, :, None]
    zt, v = noise_expect(x, n, t_el)
    return x, n, t, zt, v


EULER_N = (8, 8 * 255, 8 * 256, 8 * 257)
EULER_CFG = (1.0, 3.0, 7.5)
EULER_DT = (-0.0625, 0.046875, -0.99609375)      # dyadic, at most 8 significant bits: dt out is exact in fp32


@functools.lru_cache(maxsize=None)
def euler_case(n, cfg, dt, guided):
    g = gen(n, int(cfg * 2), int(dt * 2 ** 20), guided, 93)
    cond, unc = generic_bf16((n,), g), generic_bf16((n,), g)
    acc = torch.randn(n, generator=g, dtype=f32) * 2.0
    m, _ = math.frexp(abs(dt))
    assert m * 256 == int(m * 256), "dt needs more than 8 significant bits"
    c, u = cond.to(f32), unc.to(f32)
    o = rbf(u + rbf(cfg * rbf(c - u))) if guided else c
    prod = o.to(f64) * dt
    assert torch.equal(prod.to(f32).to(f64), prod)      # exact: a fused multiply-add and mul + add agree
    new = (acc.to(f64) + prod).to(f32)
    return cond, (unc if guided else None), acc, new, new.to(bf16)


CAST_N = (1, 7, 8, 9, 2047, 2048, 2049)


def cast_values(n, salt=0):
    """fp32 data for the f32 -> bf16 cast: ties (to even, both ways), +-0, subnormals, +-inf, values that round to inf,
    NaN, and generic numbers"""
    special = torch.tensor([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x00000000, 0x80000000, 0x00000001, 0x80400000,
                            0x00008000, 0x00018000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7F8000, 0x7F7F7FFF, 0x7FC00000,
                            0xFFC00001, 0x7F800001, 0x3EAAAAAB, 0xC0490FDB], dtype=torch.int64)
    special = torch.where(special >= 2 ** 31, special - 2 ** 32, special).to(torch.int32).view(f32)
    body = torch.randn(n, generator=gen(n, salt, 95), dtype=f32) * 3.0
    k = min(n, special.numel())
    idx = (torch.arange(k) * 7 + salt) % special.numel()
    pos = (torch.arange(k) * max(1, n // k) + (n - 1)) % n if n > 1 else torch.zeros(1, dtype=torch.long)
    body[pos[:k]] = special[idx]
    return body


def assert_cast(what, got, src):
    want = src.to(bf16)
    nan = torch.isnan(src)
    assert torch.equal(torch.isnan(got.float()), nan), what + ": NaN positions"
    ok = (bits(got) == bits(want)) | nan
    assert ok.all(), f"{what}: {int((~ok).sum())} elements differ, first at {int((~ok).nonzero()[0])}"


def all_bf16():
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(bf16)


ROPE_TABS = ((5, 3), (16, 24))
ROPE_THW = ((1, 1, 1), (3, 5, 7), (4, 8, 8))
ROPE_NREG = (0, 16)
ROPE_BAD_START = (-5, 200, 127)


def rope_starts(thw):
    return [(0, 0, 0), (2, 3, 4), tuple(128 - d for d in thw)]


def rope_clamp(start, thw):
    return tuple(min(max(s, 0), 128 - d) for s, d in zip(start, thw))


@functools.lru_cache(maxsize=None)
def rope_tables(nt, ns):
    g = gen(nt, ns, 97)
    return tuple(torch.randn(128, n, generator=g, dtype=f32) for n in (nt, nt, ns, ns))   # t cos, t sin, s cos, s sin


def rope_expect(tabs, thw, start, n_reg):
    """torch gather: row n_reg + i is the table entry of unravel(i, (t, h, w)) + start"""
    tc, ts, sc, ss = tabs
    t, h, w = thw
    ti, hi, wi = torch.meshgrid(torch.arange(t), torch.arange(h), torch.arange(w), indexing="ij")
    ti, hi, wi = (ti.flatten() + start[0]), (hi.flatten() + start[1]), (wi.flatten() + start[2])
    cos = torch.cat([tc[ti], sc[hi], sc[wi]], 1)
    sin = torch.cat([ts[ti], ss[hi], ss[wi]], 1)
    half = cos.shape[1]
    return torch.cat([torch.ones(n_reg, half), cos]), torch.cat([torch.zeros(n_reg, half), sin])


# ---- timestep embedding --------------------------------------------------------------------------------------------------
TEMB_D = (2, 16, 258, 384, 1152)
TEMB_B = (1, 5, 61)
TEMB_C = float(torch.tensor(-9.210340371976184, dtype=f32))


def temb_t(B):
    """0, 1, 2^-10 and evenly spaced values in (0, 1): the range the trainer and the sampler pass"""
    if B == 1:
        return torch.tensor([0.4375], dtype=f32)
    head = [0.0, 1.0, 2.0 ** -10]
    rest = [(i + 1) / (B - 2) for i in range(B - 3)]
    return torch.tensor(head + rest, dtype=f32)


@functools.lru_cache(maxsize=None)
def temb_case(B, D):
    """the kernel's formula: f = exp(c i / half) with the exponent's two fp32 roundings restated, a = t f, [cos a | sin a]
    rounded to bf16.  The argument moves by +- 2^-21 RELATIVE, the result by +- 2^-23 RELATIVE (absolute moves would
    leave the tiny sines undecided) -> (t, want bf16-in-fp32 [B, D], undecided mask)"""
    half = D // 2
    t = temb_t(B)
    i = torch.arange(half, dtype=f32)
    z = (torch.tensor(TEMB_C, dtype=f32) * i) / torch.tensor(float(half), dtype=f32)     # fp32, in the kernel's order
    a = t.to(f64)[:, None] * torch.exp(z.to(f64))[None, :]
    variants = []
    for da in (0.0, 2.0 ** -21, -2.0 ** -21):
        for dr in (0.0, 2.0 ** -23, -2.0 ** -23):
            am = a * (1.0 + da)
            variants.append(torch.cat([torch.cos(am), torch.sin(am)], 1) * (1.0 + dr))
    want, und = R.decide(variants)
    zero = t == 0
    assert not und[zero].any() and (want[zero][:, :half] == 1).all() and (want[zero][:, half:] == 0).all()
    return t, want.to(f32), und
