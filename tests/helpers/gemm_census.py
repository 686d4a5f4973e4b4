"""Exact census of the bf16 GEMM (csrc/gemm.hip): operands, expectations, windows and the shape lists.

Operands are small integers or small dyadic rationals, so every product and every fp32 partial sum is exact: the
accumulator is the same number in any summation order, tiling, split-K or atomic order, and every output element has
ONE right answer -- the round-to-nearest-even bf16 of an exactly known number (or that number, for fp32 outputs).
Everything here runs on the CPU with torch alone; the GPU test compares bits.  Each builder ASSERTS the property that
makes the zero-tolerance comparison legitimate and raises if it does not hold (it never skips a case).
"""
import functools
import math
from collections import namedtuple

import torch

from video_diffusion_speedrun_amd.ops import mod_group_of

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64

# (bm, bn, bk) of the three tilings; the value vds_gemm_force_tile pins each with
TILINGS = ((128, 128, 64), (256, 256, 64), (256, 128, 32))
FORCE_TILE = {(128, 128, 64): 128, (256, 256, 64): 256, (256, 128, 32): 2}

# ---- shape lists (M, N, K): each entry is one of the smallest shapes that can break something -------------------------
# NT and NN share a list (M rows of A, N output columns, K the contraction, K % 8 == 0, N % 8 == 0).
SHAPES_NT = [
    (1, 8, 8),          # the smallest legal problem
    (33, 16, 8),
    (64, 256, 8),       # K below one K tile of every tiling: the prologues are deeper than the K loop
    (77, 72, 72),
    (127, 120, 40),     # below the 128 tile in M and N
    (128, 128, 72),     # equal
    (129, 136, 104),    # one legal step past
    (130, 8, 136),
    (145, 64, 264),
    (200, 392, 104),    # 256-wide tiling: last tile column of 136 (not narrow, ragged)
    (255, 248, 136),    # below the 256 tile
    (256, 256, 200),    # equal
    (257, 264, 64),     # one legal step past
    (256, 128, 128),    # full tiles only, K a multiple of every bk
    (264, 328, 328),    # 256-wide tiling: last tile column of 72 (narrow, ragged); 5.1 K tiles of 64
    (292, 136, 72),     # 4 samples of 73 rows (the grouped GATE_RES form)
    (300, 384, 128),    # 256-wide tiling: last tile column of exactly 128 (narrow, full)
    (384, 320, 192),
    (385, 200, 40),
    (513, 128, 104),
    (519, 264, 72),
    (520, 392, 8),      # a few tiles past in M and N
    (8, 384, 200),
    (1, 392, 40),
]
SHAPES_NN = list(SHAPES_NT)
# TN: C[M, N] (fp32) = A[K, M]^T B[K, N]; M % 8 == 0 and N % 8 == 0, K (the token count) is free
SHAPES_TN = [
    (8, 8, 1),          # the smallest legal output, one token
    (8, 8, 7),
    (120, 120, 77),
    (128, 128, 8),
    (136, 136, 40),
    (248, 248, 72),
    (256, 256, 104),
    (264, 264, 136),
    (520, 392, 200),
    (384, 328, 64),
    (296, 384, 128),
    (16, 392, 328),
    (72, 8, 300),
    (520, 8, 33),
    (8, 136, 129),
    (128, 256, 256),
    (272, 72, 7),
    (392, 128, 1),
]
SHAPES = {"NT": SHAPES_NT, "NN": SHAPES_NN, "TN": SHAPES_TN}
ROWS_PER_BATCH = 73               # GATE_RES: not a multiple of 64, so 64-row sub-tiles straddle samples
GROUPED = dict(lead=16, period=3, S=19, B=4)   # the grouped GATE_RES form: L = 16 + 3 * 19 = 73 rows per sample
SHAPES_GROUPED = [(292, 136, 72), (292, 392, 200), (292, 128, 8)]   # M = B * L

GATES = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 1.5)
SENTINEL_BF16 = 0xBEEF - 0x10000          # int16 bit pattern of the bf16 output fill (-0.4668: not a value any case produces)
SENTINEL_F32 = 0xDEADBEEF - 0x100000000   # int32 bit pattern of the fp32 output fill


def step_m(layout):
    """one legal step in M: 1 row for NT / NN, 8 for TN"""
    return 8 if layout == "TN" else 1


def coverage(layout, tiling):
    """name -> bool: the coverage predicates of the shape list of `layout` against one tiling"""
    bm, bn, bk = tiling
    shapes = SHAPES[layout]
    Ms, Ns, Ks = {s[0] for s in shapes}, {s[1] for s in shapes}, {s[2] for s in shapes}
    sm = step_m(layout)
    cov = {
        "M below bm": any(m < bm for m in Ms), "M equal bm": bm in Ms, "M one step past bm": bm + sm in Ms,
        "M a few tiles past bm": any(m > 2 * bm for m in Ms),
        "N below bn": any(n < bn for n in Ns), "N equal bn": bn in Ns, "N one step past bn": bn + 8 in Ns,
        # (N stops at 392: the 256-wide tiling gets a second, ragged tile column, the 128-wide ones four)
        "N tiles past bn": any(n > bn + 8 for n in Ns),
        "K a multiple of bk": any(k % bk == 0 for k in Ks),
    }
    for steps in (1, 2, 3, 4):
        cov[f"K {steps} steps with a tail of 8"] = (steps - 1) * bk + 8 in Ks
    if bn == 256:
        last = {n - (n - 1) // 256 * 256 for n in Ns if n > 256}
        cov["last tile column 128 (narrow, full)"] = 128 in last
        cov["last tile column 72 (narrow, ragged)"] = 72 in last
        cov["last tile column 136 (not narrow, ragged)"] = 136 in last
    if layout == "TN":
        cov["smallest legal output"] = any(m == 8 and n == 8 for m, n, _ in shapes)
        for k in (1, 7, 77):
            cov[f"{k} tokens"] = k in Ks
    else:
        cov["M == 1, N == 8, K == 8"] = (1, 8, 8) in shapes
    return cov


# ---- values ------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(layout, M, N, K, salt=0):
    return (("NT", "NN", "TN").index(layout) * 1000003 + M * 7919 + N * 104729 + K * 1299709 + salt) % (2 ** 31 - 1)


gen, seed_of = _gen, _seed   # the public names (fp8_census.py builds its cases on the same seeds)


def ints(shape, lo, hi, seed, dtype=f64):
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).to(dtype)


def dense_range(K):
    """|a|, |b| <= r with the sum of K products of spread ~ sqrt(K) r^2 / 3 ~ 256 and more: results on both sides of 256,
    where a bf16 store starts to round (r <= 128: bf16 holds the integers up to 256 exactly)"""
    return int(min(128, max(3, math.ceil(math.sqrt(1024.0 / math.sqrt(K))))))


def to_bf16_exact(t):
    """float64 -> bf16 for operand values: must be exact"""
    r = t.to(bf16)
    assert torch.equal(r.to(f64), t), "operand values must be bf16 numbers"
    return r


def round_bf16(t64):
    """the one rounding of an expectation: float64 -> (exactly) fp32 -> round-to-nearest-even bf16 (torch's cast)"""
    t32 = t64.to(f32)
    assert torch.equal(t32.to(f64), t64), "the exact result must be an fp32 number"
    return t32.to(bf16)


def trunc_bf16(t64):
    """the FAULTY conversion: fp32 -> bf16 by dropping the low 16 bits"""
    bits = t64.to(f32).view(torch.int32) & ~0xFFFF
    return bits.view(f32).to(bf16)


def opA(layout, A):
    return A.t() if layout == "TN" else A


def opB(layout, B):
    return B.t() if layout == "NT" else B


def matmul64(layout, A, B):
    """sum_k opA[m, k] opB[k, n] in float64 (exact for the operand sets here).  + 0.0: a sum that is zero is +0, as in an
    accumulator that starts from +0 (a BLAS may return the -0 of a lone product)"""
    return opA(layout, A.to(f64)) @ opB(layout, B.to(f64)) + 0.0


Dense = namedtuple("Dense", "layout M N K A B bias acc want want_bias")


@functools.lru_cache(maxsize=None)
def dense_case(layout, M, N, K):
    """dense set (STORE, GATE_RES, F32): integer A, B, bias.  acc / want are float64 (exact), want* the bf16 stores."""
    r = dense_range(K)
    a_shape = (K, M) if layout == "TN" else (M, K)
    b_shape = (N, K) if layout == "NT" else (K, N)
    A = ints(a_shape, -r, r, _seed(layout, M, N, K, 1))
    B = ints(b_shape, -r, r, _seed(layout, M, N, K, 2))
    bias = ints((N,), -64, 64, _seed(layout, M, N, K, 3))
    amax, bmax = float(A.abs().max()), float(B.abs().max())
    assert K * amax * bmax + 64 < 2 ** 24, "fp32 accumulation must be exact"
    acc = matmul64(layout, A, B)
    assert (acc.abs() > 256).any(), f"{layout} {M}x{N}x{K}: no result above 256 (the bf16 store would never round)"
    want = want_bias = None
    if layout != "TN":
        want, want_bias = round_bf16(acc), round_bf16(acc + bias)
        assert (want.to(f64) != acc).any() and (want_bias.to(f64) != acc + bias).any(), \
            f"{layout} {M}x{N}x{K}: every result is a bf16 number (rounding is not exercised)"
    return Dense(layout, M, N, K, to_bf16_exact(A), to_bf16_exact(B), to_bf16_exact(bias), acc, want, want_bias)


GateRes = namedtuple("GateRes", "aux gate rows y x_new")


def gate_rows_plain(M, rows_per_batch):
    return torch.arange(M) // rows_per_batch


def gate_rows_grouped(M, L, lead, period):
    """gate-table row of every output row: sample b = r // L, group mod_group_of(r % L)"""
    return torch.tensor([(r // L) * (1 + period) + mod_group_of(r % L, lead, period) for r in range(M)])


def gate_res_case(d, rows, n_gate_rows, with_bias=True):
    """GATE_RES on a dense case: y = acc (+ bias), x_new = aux + y * gate[rows[m]] -- exact in fp32, rounded once"""
    M, N = d.M, d.N
    g = _gen(_seed(d.layout, M, N, d.K, 4))
    gate = torch.tensor(GATES, dtype=f64)[torch.randint(0, len(GATES), (n_gate_rows, N), generator=g)]
    aux = ints((M, N), -32, 32, _seed(d.layout, M, N, d.K, 5))
    y = d.acc + (d.bias.to(f64) if with_bias else 0.0)
    x_new = aux + y * gate[rows]
    assert float(x_new.abs().max()) * 2 < 2 ** 24  # halves of integers below 2^23: fp32 numbers, fma or not
    return GateRes(to_bf16_exact(aux), gate.to(f32), rows, round_bf16(y), round_bf16(x_new))


def phi(x):
    return 0.5 * torch.erfc(-x / math.sqrt(2.0))


def gelu64(x):
    return x * phi(x)


def dgelu64(x):
    return phi(x) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


Sparse = namedtuple("Sparse", "M N K A B bias pre pre64 act64")


@functools.lru_cache(maxsize=None)
def sparse_case(M, N, K):
    """sparse dyadic set (NT BIAS_GELU): A in {-1, 0, 0, 1}, B in {-2..2}/16, bias multiples of 1/16 in [-0.5, 0.5].
    Every pre-activation is a multiple of 1/16 below 6 in magnitude, hence exactly a bf16 number: the table path
    (rounds pre to bf16 first) and the formula path (does not) see the same argument."""
    A = torch.tensor([-1.0, 0.0, 0.0, 1.0], dtype=f64)[torch.randint(0, 4, (M, K), generator=_gen(_seed("NT", M, N, K, 6)))]
    B = ints((N, K), -2, 2, _seed("NT", M, N, K, 7)) / 16.0
    bias = ints((N,), -8, 8, _seed("NT", M, N, K, 8)) / 16.0
    pre64 = (A @ B.t() + 0.0) + bias
    assert float(pre64.abs().max()) < 6.0, f"sparse {M}x{N}x{K}: |pre| reaches {float(pre64.abs().max())}"
    pre = pre64.to(f32).to(bf16)
    assert torch.equal(pre.to(f64), pre64), "every pre-activation must be exactly a bf16 number"
    return Sparse(M, N, K, to_bf16_exact(A), to_bf16_exact(B), to_bf16_exact(bias), pre, pre64, gelu64(pre64))


DGelu = namedtuple("DGelu", "M N K A B aux acc want64")


@functools.lru_cache(maxsize=None)
def dgelu_case(M, N, K):
    """NN DGELU: dy [M, K] and W [K, N] small integers (acc exact), aux arbitrary bf16 values in [-6, 6]"""
    A = ints((M, K), -2, 2, _seed("NN", M, N, K, 9))
    B = ints((K, N), -2, 2, _seed("NN", M, N, K, 10))
    assert K * 4 < 2 ** 24
    aux = ((torch.rand(M, N, generator=_gen(_seed("NN", M, N, K, 11)), dtype=f64) * 12.0 - 6.0).to(f32).to(bf16))
    aux[0, :4] = torch.tensor([0.0, -0.0, 6.0, -6.0]).to(bf16)
    acc = A @ B + 0.0
    return DGelu(M, N, K, to_bf16_exact(A), to_bf16_exact(B), aux, acc, acc * dgelu64(aux.to(f64)))


# the two GELU epilogues: per-element bounds from what the code states (never from a run).  One bf16 rounding of the
# result (half an ulp <= 2^-8 |want|) plus the stated error of the path:
#   table   (g_gelu_lut: 1e-4 of the 0.5 plateau where the index clamps):  1.5e-4 min(|x|, 1)  /  1.5e-4 |acc|
#   formula (gauss_cdf in common.h: 4e-7 absolute in gelu, 3e-7 in gelu'):   1e-6               /  1e-6 |acc|
def gelu_bound(want64, x64, table):
    return want64.abs() * 2.0 ** -8 + (1.5e-4 * x64.abs().clamp(max=1.0) if table else 1e-6)


def dgelu_bound(want64, acc64, table):
    return want64.abs() * 2.0 ** -8 + (1.5e-4 if table else 1e-6) * acc64.abs()


# ---- windows -----------------------------------------------------------------------------------------------------------
def bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def fill_value(dtype, fill):
    """`fill`: "nan" (input parents) or "sentinel" (output parents: a fixed bit pattern)"""
    if fill == "nan":
        return torch.tensor(float("nan"), dtype=dtype)
    assert fill == "sentinel"
    if dtype == bf16:
        return torch.tensor(SENTINEL_BF16, dtype=torch.int16).view(bf16)
    return torch.tensor(SENTINEL_F32, dtype=torch.int32).view(f32)


def embed(t, pad_rows=3, pad_cols=16, col0=8, fill="nan"):
    """place the logical matrix `t` as a window inside a larger parent: leading dimension = row length + pad_cols (a
    multiple of 8), window at column col0 (a multiple of 8) and row pad_rows (nonzero), pad_rows guard rows before and
    after.  Returns (parent, view); the view is t's values inside the parent."""
    assert t.dim() == 2 and pad_rows > 0 and pad_cols % 8 == 0 and col0 % 8 == 0 and 0 <= col0 <= pad_cols
    rows, cols = t.shape
    parent = fill_value(t.dtype, fill).repeat(rows + 2 * pad_rows, cols + pad_cols)
    view = parent[pad_rows:pad_rows + rows, col0:col0 + cols]
    view.copy_(t)
    return parent, view


def locate(parent, view):
    """(row0, col0, rows, cols) of a 2-D window `view` of `parent`"""
    ld = parent.stride(0)
    assert view.dim() == 2 and view.stride(0) == ld and view.stride(1) == 1
    off = view.storage_offset() - parent.storage_offset()
    return off // ld, off % ld, view.shape[0], view.shape[1]


def window(parent, where):
    r0, c0, rows, cols = where
    return parent[r0:r0 + rows, c0:c0 + cols]


def assert_window(parent_after, parent_before, where, want, what=""):
    """the window `where` (a view of parent_before, or (row0, col0, rows, cols)) of parent_after must equal `want` bit
    for bit, and every byte outside it must be what it was in parent_before"""
    if isinstance(where, torch.Tensor):
        where = locate(parent_before, where)
    after, before = parent_after.cpu(), parent_before.cpu()
    assert after.shape == before.shape and after.dtype == before.dtype == want.dtype, what
    got = window(after, where)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = bits(got.contiguous()) != bits(want.contiguous())
    if diff.any():
        i, j = (int(v) for v in diff.nonzero()[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.numel()} elements differ, first at ({i}, {j}): "
                             f"got {got[i, j].item()!r} want {want[i, j].item()!r}")
    assert_outside(after, before, where, what)


def assert_outside(parent_after, parent_before, where, what=""):
    """every byte of the parent outside the window must be what it was"""
    if isinstance(where, torch.Tensor):
        where = locate(parent_before, where)
    after, before = parent_after.cpu(), parent_before.cpu()
    outside = bits(after) != bits(before)
    window(outside, where).fill_(False)
    if outside.any():
        i, j = (int(v) for v in outside.nonzero()[0])
        raise AssertionError(f"{what}: {int(outside.sum())} elements outside the window {where} changed, first at "
                             f"parent ({i}, {j})")


def place(t, embedded, fill):
    """an operand or output of a GEMM call: (parent, where).  embedded: a window of a larger parent (embed); else the
    parent is the dense matrix itself.  Outputs pass the initial content of the window in `t`."""
    if embedded:
        parent, view = embed(t, fill=fill)
        return parent, locate(parent, view)
    return t.clone(), (0, 0, t.shape[0], t.shape[1])


def blank(rows, cols, dtype):
    """initial content of an output window: the sentinel (a dense output has no guard band, so an element the kernel
    leaves unwritten must still show)"""
    return fill_value(dtype, "sentinel").repeat(rows, cols)
