"""Exact census of the fp8 path (csrc/quant.hip, vds_gemm_fp8 and its emitting epilogues, the fp8-emitting row kernels):
the one right answer of a quantisation, the input that meets every value class, operands, shape lists, emulated faults.

quant_ref states the contract of vds.h once -- ONE fp32 multiply by fp32(fmax) / fp32(amax), a clamp to +-fmax, a
round-to-nearest-even cast (torch's float8 dtypes) -- and quant_ref64 restates it with float64 arithmetic and an explicit
rounding onto the fp8 grid; tests/test_fp8_census_cpu.py proves the two equal on every finite bf16 pattern.  Every fp8
byte a kernel writes therefore has one right value, and the GPU test compares bytes.  The GEMM operands are the small
dyadic values whose products and fp32 sums are exact (as gemm_census.py), so its outputs are compared bit for bit too.
Everything here runs on the CPU with torch alone.  Each builder ASSERTS what makes the zero tolerance legitimate.
"""
import functools
from collections import namedtuple

import torch

import gemm_census as G

bf16, f32, f64, u8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8

FMAX = (448.0, 57344.0)                       # e4m3fn, e5m2
DTYPES = (torch.float8_e4m3fn, torch.float8_e5m2)
MBITS = (3, 2)                                # mantissa bits
EMIN = (-6, -14)                              # exponent of the smallest normal number
SENTINEL_U8 = 0x7F                            # NaN in both formats: no finite input quantises to it
AMAX_OF = (lambda fmax: fmax, lambda fmax: fmax / 64, lambda fmax: fmax * 1024, lambda fmax: 0.0, lambda fmax: 3.0)
AMAX_NAMES = ("fmax", "fmax/64", "fmax*2^10", "0", "3.0")


def amax_values(fmt):
    """the five amax of the exhaustive quantiser test: scales 1, 64, 2^-10, 1 (amax 0) and the non-dyadic fmax / 3"""
    return [f(FMAX[fmt]) for f in AMAX_OF]


# ---- the reference -----------------------------------------------------------------------------------------------------
def scale_of(fmt, amax):
    """(fp32 scale, fp32 dequantisation factor) of one amax: fmax / amax and amax / fmax, each ONE fp32 division"""
    fmax, am = torch.tensor(FMAX[fmt], dtype=f32), torch.tensor(float(amax), dtype=f32)
    if float(am) > 0:
        return fmax / am, am / fmax
    return torch.tensor(1.0, dtype=f32), torch.tensor(1.0, dtype=f32)


def quant_ref(x, fmt, amax):
    """bf16 tensor -> (uint8 tensor of fp8 bytes, fp32 dq).  Finite inputs only."""
    assert x.dtype == bf16
    scale, dq = scale_of(fmt, amax)
    y = (x.to(f32) * scale).clamp(-FMAX[fmt], FMAX[fmt])
    return y.to(DTYPES[fmt]).view(u8), dq


@functools.lru_cache(maxsize=None)
def decode_table(fmt):
    """float64 [256]: the value of every byte, from the bit fields (independent of torch's float8 types); NaN / Inf as such"""
    mb, emin = MBITS[fmt], EMIN[fmt]
    out = torch.zeros(256, dtype=f64)
    for b in range(256):
        s, e, m = b >> 7, (b & 0x7F) >> mb, b & ((1 << mb) - 1)
        if e == 0:
            v = m * 2.0 ** (emin - mb)
        else:
            v = (1.0 + m * 2.0 ** -mb) * 2.0 ** (e - 1 + emin)
        if fmt == 0 and (b & 0x7F) == 0x7F:
            v = float("nan")
        if fmt == 1 and e == 31:
            v = float("inf") if m == 0 else float("nan")
        out[b] = -v if s else v
    return out


def decode(q, fmt):
    return decode_table(fmt)[q.long()]


def nonfinite_bytes(fmt):
    return [b for b in range(256) if not torch.isfinite(decode_table(fmt)[b])]


def grid(y64, fmt):
    """|y| in units of the fp8 quantum at y (float64; the quantum of the subnormal range below the smallest normal)"""
    a = y64.abs()
    _, e = torch.frexp(a)                                  # a = m 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    e = (e - 1).clamp(min=EMIN[fmt]).to(f64)
    quantum = 2.0 ** (e - MBITS[fmt])
    return a / quantum, quantum


def quant_ref64(x, fmt, amax, rounding="rne"):
    """the same contract in float64 -> float64 VALUES (sign of zero kept).  The fp32 multiply is the exact product rounded
    to fp32 once; the cast is an explicit rounding of |y| / quantum.  rounding: "rne" | "trunc" | "away" (the faults)"""
    scale, _ = scale_of(fmt, amax)
    y = (x.to(f64) * scale.to(f64)).to(f32).to(f64)
    y = y.clamp(-FMAX[fmt], FMAX[fmt])
    t, quantum = grid(y, fmt)
    if rounding == "rne":
        r = torch.round(t)                                 # (half to even)
    elif rounding == "trunc":
        r = torch.floor(t)
    else:
        r = torch.floor(t + 0.5)
    return torch.copysign(r * quantum, y)


def encode64(v64, fmt):
    """float64 values that ARE fp8 numbers -> bytes (by search in the decode table; -0 -> 0x80)"""
    tab = decode_table(fmt)
    finite = torch.tensor([b for b in range(128) if torch.isfinite(tab[b])])
    vals = tab[finite]                                     # ascending
    idx = torch.searchsorted(vals, v64.abs().contiguous())
    idx = idx.clamp(max=len(vals) - 1)
    assert torch.equal(vals[idx], v64.abs()), "not an fp8 number"
    return (finite[idx] + 128 * torch.signbit(v64).long()).to(u8)


def ties(x, fmt, amax):
    """mask: x * scale lies exactly half way between two fp8 numbers (inside the range)"""
    scale, _ = scale_of(fmt, amax)
    y = (x.to(f64) * scale.to(f64)).to(f32).to(f64)
    t, _ = grid(y, fmt)
    return (t - torch.floor(t) == 0.5) & (y.abs() < FMAX[fmt])


def classes(x, fmt, amax):
    """name -> mask of the value classes a quantiser can get wrong"""
    scale, _ = scale_of(fmt, amax)
    y = x.to(f64) * scale.to(f64)
    q, _ = quant_ref(x, fmt, amax)
    v = decode(q, fmt)
    return {"tie": ties(x, fmt, amax), "subnormal result": (v != 0) & (v.abs() < 2.0 ** EMIN[fmt]),
            "saturating": y.abs() > FMAX[fmt], "+0 result": q == 0, "-0 result": q == 0x80}


# ---- the pattern matrix ------------------------------------------------------------------------------------------------
def _permutation():
    """a fixed bijection of the 16-bit patterns (multiply by an odd number / xor-shift steps: each one invertible) that
    spreads the low pattern bits -- which decide ties -- over all residues of the position"""
    x = torch.arange(65536, dtype=torch.int64)
    x = (x * 40503) & 0xFFFF
    x = x ^ (x >> 7)
    x = (x * 0x2F65) & 0xFFFF
    x = x ^ (x >> 9)
    x = (x * 0x6A2B) & 0xFFFF
    x = x ^ (x >> 5)
    assert torch.equal(torch.sort(x).values, torch.arange(65536)), "not a permutation"
    return x


@functools.lru_cache(maxsize=None)
def pattern_matrix(finite_only=False):
    """bf16 [256, 256] holding all 65 536 bit patterns.  finite_only: the 256 patterns with exponent 0xFF (2 Inf, 254 NaN)
    have bit 14 cleared (large finite values, which saturate).  Asserts that every (m % 4, k % 8) class of positions
    holds ties, subnormal results, saturating values and zero results of both signs, in both formats at scale 1."""
    pat = _permutation().view(256, 256)
    nonfin = (pat & 0x7F80) == 0x7F80
    assert int(nonfin.sum()) == 256
    fin = torch.where(nonfin, pat & 0xBFFF, pat)
    x = (fin if finite_only else pat).to(torch.int32).to(torch.int16).view(256, 256)   # (wraps to the signed pattern)
    x = x.view(bf16)
    assert finite_only == bool(torch.isfinite(x.to(f32)).all())
    xf = fin.to(torch.int32).to(torch.int16).view(bf16)
    m4, k8 = (torch.arange(256) % 4)[:, None], (torch.arange(256) % 8)[None, :]
    for fmt in (0, 1):
        for name, mask in classes(xf, fmt, FMAX[fmt]).items():
            for a in range(4):
                for b in range(8):
                    n = int((mask & (m4 == a) & (k8 == b)).sum())
                    assert n >= 1, f"pattern matrix: no {name} at m % 4 == {a}, k % 8 == {b} (fmt {fmt})"
    return x


def nonfinite_positions():
    """((m, k) of the 254 NaN patterns, (m, k) of the 2 Inf patterns) in pattern_matrix()"""
    x = pattern_matrix().to(f32)
    return torch.isnan(x).nonzero(), torch.isinf(x).nonzero()


@functools.lru_cache(maxsize=None)
def pool():
    """the finite patterns below 256 in magnitude, in matrix order: the values the shape cases draw from"""
    x = pattern_matrix(True).flatten()
    return x[x.to(f32).abs() < 256.0]


PEAK, BEYOND = 300.0, 10000.0     # the largest value of a shape case (at its last element); the value put just outside
SHAPE_AMAX = (PEAK, 112.0, 0.0)   # the true maximum (a non-dyadic scale), 112 (scale 4 / 512: values above 112 saturate), 0


@functools.lru_cache(maxsize=None)
def draw(M, K, salt=0):
    """bf16 [M, K] from pool(), max |x| = PEAK at the LAST element and nowhere else"""
    p = pool()
    off = (M * 7919 + K * 104729 + salt * 1299709) % len(p)
    x = p[(off + torch.arange(M * K)) % len(p)].view(M, K).clone()
    x[M - 1, K - 1] = PEAK
    assert float(x.to(f32).abs().max()) == PEAK and int((x.to(f32).abs() == PEAK).sum()) == 1
    return x


# ---- shape lists -------------------------------------------------------------------------------------------------------
QT = 128   # tile edge of the quantiser, absmax and transpose kernels
SHAPES_QUANT = [   # (M, K), K % 8 == 0
    (1, 8), (3, 120), (4, 128), (127, 136), (128, 128), (129, 8), (130, 264), (257, 120),
    (1, 264), (3, 128), (127, 8), (128, 264), (129, 136), (130, 120), (257, 136), (4, 8),
]
_K16 = {8: 16, 120: 112, 128: 128, 136: 144, 264: 272}
SHAPES_TRANSPOSE = [(M, _K16[K]) for M, K in SHAPES_QUANT]   # K % 16 == 0
SHAPES_GEMM_NT = [   # (M, N, K): K % 16 == 0, N % 8 == 0, any M; 256 x 256 output tiles, K tiles of 128 bytes
    (1, 8, 16),         # the smallest legal problem
    (33, 16, 16),
    (63, 64, 112),      # partial sub-tiles only
    (64, 256, 16),      # K below one K tile
    (65, 72, 128),
    (127, 120, 144),
    (128, 128, 272),
    (129, 136, 112),
    (255, 248, 144),    # below the tile
    (256, 256, 128),    # equal: full sub-tiles only, one K tile exactly
    (257, 264, 400),    # one step past; 3 K tiles and a tail of 16; 3 splits of 400 leave one empty
    (256, 128, 656),    # 5 K tiles and a tail of 16
    (264, 328, 272),    # last tile column of 72 (narrow, ragged)
    (301, 384, 128),    # last tile column of exactly 128 (narrow, full)
    (200, 392, 112),    # last tile column of 136 (not narrow, ragged)
    (292, 136, 144),    # 4 samples of 73 rows
    (520, 392, 16),     # a few tiles past in M and N
    (520, 264, 400),
    (8, 384, 656),
    (1, 392, 144),
]
SHAPES_GEMM_TN = [   # C[M, N] = A[K, M]^T B[K, N]: M % 16 == 0, N % 8 == 0, K % 16 == 0 tokens
    (16, 8, 16),        # the smallest legal problem
    (112, 120, 16),
    (128, 128, 112),
    (144, 136, 128),
    (240, 248, 144),
    (256, 256, 128),
    (272, 264, 400),
    (384, 328, 144),    # last tile column of 72
    (304, 384, 112),    # of 128
    (528, 392, 128),    # of 136; a few tiles past
    (16, 392, 400),
    (272, 8, 112),
]
SHAPES_EMIT = [(256, 256, 128), (63, 64, 112), (257, 264, 400), (301, 384, 128), (264, 328, 272), (200, 392, 112)]
ROWS_PER_BATCH = G.ROWS_PER_BATCH
MAX_OPERAND_BYTES = 1 << 20


def _last_col(N):
    return N - (N - 1) // 256 * 256


def sub_tiles(M, N):
    """(some 64 x 64 sub-tile lies fully inside, some sticks out) -- restated from gemm_tile: full = row0 + 64 <= M and
    col0 + 64 <= N (the narrow last column steps by 32: a multiple of 64 inside is a multiple of 32 inside)"""
    full = M >= 64 and N >= 64
    partial = M % 64 != 0 or N % 64 != 0
    return full, partial


def empty_split(K, splits):
    """K tiles of 128 bytes dealt out ceil(tiles / splits) at a time: the last split gets none"""
    tiles = -(-K // 128)
    per = -(-tiles // splits)
    return tiles > 1 and per * (splits - 1) >= tiles


def coverage(which):
    """name -> bool for one list: "quant" | "transpose" | "gemm_nt" | "gemm_tn" | "emit" """
    cov = {}
    if which in ("quant", "transpose"):
        shapes = SHAPES_QUANT if which == "quant" else SHAPES_TRANSPOSE
        step = 8 if which == "quant" else 16
        Ms, Ks = {m for m, _ in shapes}, {k for _, k in shapes}
        cov = {"M == 1": 1 in Ms, "M below the tile": 127 in Ms, "M equal": QT in Ms, "M one past": QT + 1 in Ms,
               "M several tiles": any(m > 2 * QT for m in Ms), "smallest K": step in Ks, "K below the tile": any(step < k < QT for k in Ks),
               "K equal": QT in Ks, "K one step past": QT + step in Ks, "K several tiles": any(k > 2 * QT for k in Ks),
               "smallest problem": (1, step) in shapes}
        for r in (0, 1, 2, 3):
            cov[f"M % 4 == {r}"] = any(m % 4 == r for m in Ms)
        cov["byte tail in the last of several tiles"] = any(m % 4 and m > QT for m in Ms)
        cov["byte tail of 3 at the end of a tile"] = QT - 1 in Ms
        return cov
    if which == "emit":
        cov["full sub-tiles only"] = any(sub_tiles(M, N) == (True, False) for M, N, _ in SHAPES_EMIT)
        cov["partial sub-tiles only"] = any(sub_tiles(M, N) == (False, True) for M, N, _ in SHAPES_EMIT)
        cov["qt byte tail of 1"] = sum(1 for M, _, _ in SHAPES_EMIT if M % 4 == 1) >= 2
        cov["qt byte tail of 3"] = any(M % 4 == 3 for M, _, _ in SHAPES_EMIT)
        for last in (72, 128, 136):
            cov[f"last tile column {last}"] = any(N > 256 and _last_col(N) == last for _, N, _ in SHAPES_EMIT)
        cov["subset of the NT list"] = all(s in SHAPES_GEMM_NT for s in SHAPES_EMIT)
        return cov
    tn = which == "gemm_tn"
    shapes = SHAPES_GEMM_TN if tn else SHAPES_GEMM_NT
    Ms, Ns, Ks = {s[0] for s in shapes}, {s[1] for s in shapes}, {s[2] for s in shapes}
    sm = 16 if tn else 1
    cov = {"M below 256": any(m < 256 for m in Ms), "M equal": 256 in Ms, "M one step past": 256 + sm in Ms,
           "M a few tiles past": any(m > 512 for m in Ms), "N below 256": any(n < 256 for n in Ns), "N equal": 256 in Ns,
           "N one step past": 264 in Ns, "K below one tile": 16 in Ks and 112 in Ks, "K one tile": 128 in Ks,
           "K one step past": 144 in Ks, "K several tiles and a tail of 16": 400 in Ks,
           "smallest problem": ((16, 8, 16) if tn else (1, 8, 16)) in shapes,
           "3 splits leave one empty": any(empty_split(k, 3) for k in Ks)}
    for last in (72, 128, 136):
        cov[f"last tile column {last}"] = any(n > 256 and _last_col(n) == last for n in Ns)
    if not tn:
        cov["K in {16, 112, 128, 144, 272, 400, 656}"] = Ks == {16, 112, 128, 144, 272, 400, 656}
        cov["M in {1, 63, 64, 65, 255, 256, 257, 301, 520}"] = {1, 63, 64, 65, 255, 256, 257, 301, 520} <= Ms
        cov["full sub-tiles only"] = any(sub_tiles(M, N) == (True, False) for M, N, _ in shapes)
        cov["partial sub-tiles only"] = any(sub_tiles(M, N) == (False, True) for M, N, _ in shapes)
        cov["both kinds in one launch"] = any(sub_tiles(M, N) == (True, True) for M, N, _ in shapes)
        cov["whole samples of 73 rows"] = any(M % ROWS_PER_BATCH == 0 for M in Ms)
    return cov


# ---- GEMM operands -----------------------------------------------------------------------------------------------------
A_VALUES = (-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0, 3.0)
B_VALUES = (-1.5, -1.0, 0.0, 0.25, 1.0, 2.0)
UNIT = 0.125                                              # the smallest product
# (scale_a, scale_b); None = a NULL pointer.  Each is NULL somewhere and != 1 somewhere, and the two never agree.
SCALES = ((0.5, 4.0), (None, 0.5), (4.0, None), (2.0 ** -7, 0.5), (4.0, 2.0 ** -7))


def scales_of(i):
    return SCALES[i % len(SCALES)]


def factor(sa, sb):
    return (1.0 if sa is None else sa) * (1.0 if sb is None else sb)


def to_fp8_exact(t64, fmt):
    """float64 -> fp8 bytes (uint8): must be exact"""
    q = t64.to(f32).to(DTYPES[fmt])
    assert torch.equal(q.to(f32).to(f64), t64), f"operand values must be fp8 numbers (fmt {fmt})"
    assert torch.equal(decode(q.view(u8), fmt), t64)
    return q.view(u8)


def _pick(values, shape, seed):
    return torch.tensor(values, dtype=f64)[torch.randint(0, len(values), tuple(shape), generator=G.gen(seed))]


Dense8 = namedtuple("Dense8", "layout M N K a_fmt A B bias sa sb acc want want_bias A64 B64")


@functools.lru_cache(maxsize=None)
def dense_case(layout, M, N, K, a_fmt, si):
    """dense set: A from A_VALUES (fp8 format a_fmt), B from B_VALUES (e4m3), bias multiples of 1/64.  acc is the float64
    product TIMES the scales (exact: powers of two); want / want_bias are the bf16 stores (NT)."""
    tn = layout == "TN"
    A64 = _pick(A_VALUES, (K, M) if tn else (M, K), G.seed_of(layout, M, N, K, 21))
    B64 = _pick(B_VALUES, (K, N) if tn else (N, K), G.seed_of(layout, M, N, K, 22))
    bias = G.ints((N,), -64, 64, G.seed_of(layout, M, N, K, 23)) / 64.0
    sa, sb = scales_of(si)
    assert sa != sb
    assert K * A64.abs().max() * B64.abs().max() / UNIT < 2 ** 24, "fp32 accumulation must be exact"
    raw = (A64.t() @ B64 if tn else A64 @ B64.t()) + 0.0
    acc = raw * factor(sa, sb)
    want = want_bias = None
    if not tn:
        want, want_bias = G.round_bf16(acc), G.round_bf16(acc + bias)
        assert M * N < 64 or (want_bias.to(f64) != acc + bias).any(), \
            f"{layout} {M}x{N}x{K}: every biased result is a bf16 number (the store's rounding is not exercised)"
    return Dense8(layout, M, N, K, a_fmt, to_fp8_exact(A64, a_fmt), to_fp8_exact(B64, 0), G.to_bf16_exact(bias), sa, sb,
                  acc, want, want_bias, A64, B64)


def unbiased_rounding_cases(a_fmt=0):
    """how many NT dense cases round in the store WITHOUT a bias (sums of a few eighths seldom need a ninth bit at K = 16:
    the builder asserts the biased store per case and this count over the list)"""
    n = 0
    for i, (M, N, K) in enumerate(SHAPES_GEMM_NT):
        d = dense_case("NT", M, N, K, a_fmt, i)
        n += bool((d.want.to(f64) != d.acc).any())
    return n


def as_dense(d):
    """the fields gemm_census.gate_res_case reads"""
    return G.Dense(d.layout, d.M, d.N, d.K, None, None, d.bias, d.acc, d.want, d.want_bias)


Sparse8 = namedtuple("Sparse8", "M N K A B bias sa sb pre pre64 act64")


@functools.lru_cache(maxsize=None)
def sparse_case(M, N, K):
    """sparse dyadic set (BIAS_GELU, a_fmt 0): A in {-1, 0, 0, 1}, B in {-2 .. 2} 2^-5 (2^-6 from K = 400 on), scales
    0.5 x 4, bias multiples of 1/16: every pre-activation is exactly a bf16 number below 6 in magnitude"""
    A = _pick((-1.0, 0.0, 0.0, 1.0), (M, K), G.seed_of("NT", M, N, K, 26))
    B = G.ints((N, K), -2, 2, G.seed_of("NT", M, N, K, 27)) * (2.0 ** -6 if K >= 400 else 2.0 ** -5)
    bias = G.ints((N,), -8, 8, G.seed_of("NT", M, N, K, 28)) / 16.0
    sa, sb = 0.5, 4.0
    pre64 = (A @ B.t() + 0.0) * factor(sa, sb) + bias
    assert float(pre64.abs().max()) < 6.0, f"sparse {M}x{N}x{K}: |pre| reaches {float(pre64.abs().max())}"
    pre = pre64.to(f32).to(bf16)
    assert torch.equal(pre.to(f64), pre64), "every pre-activation must be exactly a bf16 number"
    return Sparse8(M, N, K, to_fp8_exact(A, 0), to_fp8_exact(B, 0), G.to_bf16_exact(bias), sa, sb, pre, pre64, G.gelu64(pre64))


DGelu8 = namedtuple("DGelu8", "M N K A B aux sa sb acc want64")


@functools.lru_cache(maxsize=None)
def dgelu_case(M, N, K):
    """DGELU (a_fmt 1): gemm_census.dgelu_case's integers (dy e5m2 [M, K], W^T e4m3 [N, K]), scales NULL x 0.5"""
    dg = G.dgelu_case(M, N, K)
    sa, sb = None, 0.5
    acc = dg.acc * factor(sa, sb)
    return DGelu8(M, N, K, to_fp8_exact(dg.A.to(f64), 1), to_fp8_exact(dg.B.to(f64).t().contiguous(), 0), dg.aux, sa, sb, acc,
                  acc * G.dgelu64(dg.aux.to(f64)))


Decode = namedtuple("Decode", "name layout M N K a_fmt A B want")


def _one(fmt):
    return int(to_fp8_exact(torch.ones(1, dtype=f64), fmt)[0])


@functools.lru_cache(maxsize=None)
def decode_cases():
    """one nonzero product per dot product: C holds the decoded value of every finite byte (+0 for the byte of -0: the
    product -0 joins an accumulator of +0) -- the whole code space, subnormals included, on each operand route"""
    r = torch.arange(256)
    out = []

    def bytes_of(fmt):
        b = r.to(u8).clone()
        for x in nonfinite_bytes(fmt):
            b[x] = 0
        return b

    def scatter(fmt):   # [256, 16]: byte r at column r % 16
        t = torch.zeros(256, 16, dtype=u8)
        t[r, r % 16] = bytes_of(fmt)
        return t

    def eye(fmt):
        return torch.eye(16, dtype=u8) * _one(fmt)

    def want(fmt):     # [256, 16]
        w = torch.zeros(256, 16, dtype=f64)
        w[r, r % 16] = decode(bytes_of(fmt), fmt)
        return (w + 0.0).to(f32)
    for a_fmt in (0, 1):
        out.append(Decode(f"NT A side a_fmt {a_fmt}", "NT", 256, 16, 16, a_fmt, scatter(a_fmt), eye(0), want(a_fmt)))
        out.append(Decode(f"NT B side a_fmt {a_fmt}", "NT", 16, 256, 16, a_fmt, eye(a_fmt), scatter(0), want(0).t().contiguous()))
    out.append(Decode("TN A side", "TN", 256, 16, 16, 1, scatter(1).t().contiguous(), eye(0), want(1)))
    out.append(Decode("TN B side", "TN", 16, 256, 16, 1, eye(1), scatter(0).t().contiguous(), want(0).t().contiguous()))
    for c in out:
        assert torch.isfinite(c.want).all() and not (G.bits(c.want) == G.SENTINEL_F32).any()
        assert int((c.want != 0).sum()) == 256 - len(nonfinite_bytes(c.a_fmt if "A side" in c.name else 0)) - 2
    return out


# ---- windows of bytes --------------------------------------------------------------------------------------------------
def bits(t):
    """gemm_census.bits extended to 1-byte types"""
    return t.view(u8) if t.element_size() == 1 else G.bits(t)


def embed_u8(t, pad_rows=3, pad_cols=32, col0=16):
    """a uint8 matrix as a window of a parent full of SENTINEL_U8 (pad_cols, col0: the caller keeps the call's alignment)"""
    assert t.dtype == u8 and t.dim() == 2 and 0 <= col0 <= pad_cols
    rows, cols = t.shape
    parent = torch.full((rows + 2 * pad_rows, cols + pad_cols), SENTINEL_U8, dtype=u8)
    parent[pad_rows:pad_rows + rows, col0:col0 + cols] = t
    return parent, (pad_rows, col0, rows, cols)


def place_u8(t, embedded):
    if embedded:
        return embed_u8(t)
    return t.clone(), (0, 0, t.shape[0], t.shape[1])


def blank_u8(rows, cols):
    return torch.full((rows, cols), SENTINEL_U8, dtype=u8)


def mismatch(got, want):
    """number of differing elements (bits) -- the comparison every census assertion makes"""
    return int((bits(got.contiguous()) != bits(want.contiguous())).sum())


def assert_window_u8(after, before, where, want, what=""):
    """the byte window must equal `want`, no expectation may hold the sentinel, every byte outside must be unchanged"""
    after, before = after.cpu(), before.cpu()
    assert want.dtype == u8 and not (want == SENTINEL_U8).any(), f"{what}: the sentinel is a value of this case"
    got = G.window(after, where)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = got != want
    if diff.any():
        i, j = (int(v) for v in diff.nonzero()[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.numel()} bytes differ, first at ({i}, {j}): got "
                             f"{int(got[i, j]):#04x} want {int(want[i, j]):#04x}")
    assert_outside_u8(after, before, where, what)


def assert_outside_u8(after, before, where, what=""):
    outside = after.cpu() != before.cpu()
    G.window(outside, where).fill_(False)
    if outside.any():
        i, j = (int(v) for v in outside.nonzero()[0])
        raise AssertionError(f"{what}: {int(outside.sum())} bytes outside the window {where} changed, first at parent ({i}, {j})")


# ---- emulated faults (tests/test_fp8_census_cpu.py: each must be flagged) ----------------------------------------------
def fault_quant(x, fmt, amax, kind):
    """the bytes a faulty quantiser would write for the row-major copy"""
    if kind in ("trunc", "away"):
        return encode64(quant_ref64(x, fmt, amax, kind), fmt)
    if kind == "no saturation":     # the unclamped cast: NaN where e4m3 overflows, Inf for e5m2
        scale, _ = scale_of(fmt, amax)
        y = x.to(f32) * scale
        q = y.clamp(-FMAX[fmt], FMAX[fmt]).to(DTYPES[fmt]).view(u8).clone()
        over = y.abs() > FMAX[fmt] * (1 + 2.0 ** -(MBITS[fmt] + 1))   # (rounds past fmax)
        q[over] = (0x7F if fmt == 0 else 0x7C) + 128 * (y[over] < 0).to(u8)
        return q
    if kind == "other format":
        return quant_ref(x, 1 - fmt, amax * FMAX[1 - fmt] / FMAX[fmt] if amax else 0.0)[0]
    if kind == "scale after rounding":   # bf16 -> fp8 first (saturating), then the scale, then fp8 again
        scale, _ = scale_of(fmt, amax)
        first = x.to(f32).clamp(-FMAX[fmt], FMAX[fmt]).to(DTYPES[fmt]).to(f32)
        return (first * scale).clamp(-FMAX[fmt], FMAX[fmt]).to(DTYPES[fmt]).view(u8)
    if kind == "amax 0 as scale 0":
        assert amax == 0
        return (x.to(f32) * 0.0).to(DTYPES[fmt]).view(u8)
    raise ValueError(kind)


def fault_bytes(q, kind):
    """layout faults on a correct [M, K] byte matrix"""
    q = q.clone()
    M, K = q.shape
    if kind == "bytes of a dword swapped":
        q[:, 1::4], q[:, 2::4] = q[:, 2::4].clone(), q[:, 1::4].clone()
    elif kind == "dwords of a group swapped":
        g = q.view(M, K // 8, 2, 4)
        q = g.flip(2).reshape(M, K).clone()
    elif kind == "neighbouring row":      # the last element whose upper neighbour differs takes that neighbour's byte
        at = (q[1:] != q[:-1]).nonzero()
        if len(at):
            m, k = (int(v) for v in at[-1])
            q[m + 1, k] = q[m, k]
    elif kind == "neighbouring column":
        at = (q[:, 1:] != q[:, :-1]).nonzero()
        if len(at):
            m, k = (int(v) for v in at[-1])
            q[m, k + 1] = q[m, k]
    else:
        raise ValueError(kind)
    return q


def fault_tail(qt, M):
    """transposed copy [K, M] with row m + 1 in place of m, in the byte tail (the last M % 4 columns) only; the row past
    the last one reads as zero (the staging tile's rows at and past M hold zeros)"""
    qt = qt.clone()
    t = M % 4
    if t:
        tail = qt[:, M - t:].clone()
        qt[:, M - t:M - 1] = tail[:, 1:]
        qt[:, M - 1] = 0
    return qt
