"""Restatement of the low-rank adapter kernels (csrc/lowrank.hip) and exact inputs for them.

    down      u[m, j]  = bf16(scale * sum_k x[m, k] w(j, k))                       w(j, k) = w[j, k] | w[k, j]
    up_add    y[m, n]  = bf16(fma(scale, sum_j u[m, j] w(n, j), float(y[m, n])))   w(n, j) = w[n, j] | w[j, n]
    wgrad     g(n, j)  = fma(scale, sum_m a[m, n] u[m, j], g(n, j))  in fp32       g(n, j) = g[n, j] | g[j, n]

The sums are taken in float64 and rounded once to fp32 (the kernels accumulate in fp32; on the exact inputs below the
two are the same number), the bf16 roundings sit where the kernels have them.  Everything runs on the CPU with torch.

Exact inputs (`exact_case`): operands are small integers and dyadic rationals and `scale` is a power of two, so every
product and every fp32 partial sum is exact in ANY summation order -- chunking, MFMA order, the split over workgroups --
and every bf16 output is the exactly representable value of an exactly known number: each output element has one right
bit pattern.  The builder asserts both properties (it never skips a case), following tests/helpers/gemm_census.py.

`fault=` injects one defect into a restatement, to show that the bitwise comparison sees it (tests/test_lora_cpu.py):
    "layout"   the small matrix is read with the other w_layout / the result written with the other g_layout
    "scale"    scale is dropped (taken as 1)
    "m_chunk"  the last chunk of rows of the M split is dropped (wgrad: rows, in chunks of WGRAD_CHUNK)
    "k_chunk"  the last K chunk of the LDS staging is dropped (down: k, in chunks of down_chunk(r))
"""
import torch

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64

RANKS = (16, 32, 64)
LDS_STAGE = 32 * 1024
WGRAD_CHUNK = 2048
ROWS_PER_WORKGROUP = 128


def down_chunk(r):
    """elements of K per LDS stage of vds_lowrank_down (rows of 2 r + 16 bytes in 32 KB, whole MFMA k steps of 32)"""
    return LDS_STAGE // (2 * r + 16) // 32 * 32


def up_chunk(r):
    """columns of y per workgroup of vds_lowrank_up_add (whole 64-column groups)"""
    return LDS_STAGE // (2 * r + 16) // 64 * 64


def _small(w, layout, r, fault):
    """w(j, k) as a [r, K] float64 matrix (down) / w(n, j) as [N, r] (up_add) from the stored matrix and its layout"""
    if fault == "layout":  # the same memory read with the other layout
        w = w.contiguous().reshape(w.shape[1], w.shape[0])
        layout = 1 - layout
    return w.to(f64), layout


def down(x, w, layout, scale, fault=None):
    """x [M, K] bf16; w [r, K] (layout 0) or [K, r] (layout 1) bf16 -> u [M, r] bf16"""
    r = w.shape[0] if layout == 0 else w.shape[1]
    K = x.shape[1]
    wm, lay = _small(w, layout, r, fault)
    wjk = wm if lay == 0 else wm.t()  # [r, K]
    xs = x.to(f64)
    if fault == "k_chunk":
        kc = down_chunk(r)
        keep = (K - 1) // kc * kc  # the chunks before the last one
        xs, wjk = xs[:, :keep], wjk[:, :keep]
    acc = (xs @ wjk.t()).to(f32)
    s = 1.0 if fault == "scale" else scale
    return (acc * torch.tensor(s, dtype=f32)).to(bf16)


def up_add(u, w, layout, y, scale, fault=None):
    """u [M, r]; w [N, r] (layout 0) or [r, N] (layout 1); y [M, N] bf16 -> the new y (bf16; y itself is not modified)"""
    r = u.shape[1]
    wm, lay = _small(w, layout, r, fault)
    wnj = wm if lay == 0 else wm.t()  # [N, r]
    acc = (u.to(f64) @ wnj.t()).to(f32)
    s = 1.0 if fault == "scale" else scale
    # fma: the product is not rounded on its own (exact anyway when scale is a power of two)
    return (y.to(f64) + acc.to(f64) * s).to(f32).to(bf16)


def wgrad(a, u, g, layout, scale, fault=None):
    """a [M, N], u [M, r] bf16; g fp32 [N, r] (layout 0) or [r, N] (layout 1) -> the new g (g itself is not modified)"""
    M = a.shape[0]
    if fault == "m_chunk":
        M = (M - 1) // WGRAD_CHUNK * WGRAD_CHUNK
    acc = (a[:M].to(f64).t() @ u[:M].to(f64)).to(f32)  # [N, r]
    s = 1.0 if fault == "scale" else scale
    lay = 1 - layout if fault == "layout" else layout
    if lay == 1:
        acc = acc.t()
    if fault == "layout":  # the [N, r] result written into the other layout's memory
        acc = acc.contiguous().reshape(g.shape)
    return (g.to(f64) + acc.to(f64) * s).to(f32)


def lora_linear(x, W, b, A, B, s):
    """a LoRA'd block linear as the model runs it: the base GEMM's bf16 output, then u = bf16(x A^T) and
    y = bf16(y + s u B^T) in place.  x [M, in], W [out, in], b [out] | None, A [r, in], B [out, r], all bf16."""
    y = x.to(f64) @ W.to(f64).t()
    if b is not None:
        y = y + b.to(f64)
    y = y.to(f32).to(bf16)
    u = down(x, A, 0, 1.0)
    return up_add(u, B, 0, y, s), u


def merged_weight(W, A, B, s):
    """W + s B A in float64: what merge_lora() must leave in the fp32 master (up to fp32 rounding)"""
    return W.to(f64) + s * (B.to(f64) @ A.to(f64))


# ---- exact inputs ---------------------------------------------------------------------------------------------------
def _ints(shape, lo, hi, gen, density=1.0):
    t = torch.randint(lo, hi + 1, shape, generator=gen).to(f64)
    if density < 1.0:
        t = t * (torch.rand(shape, generator=gen) < density)
    return t


def _dyadic(shape, gen, density=1.0):
    """values in {-1, -0.5, 0, 0.5, 1}"""
    return _ints(shape, -2, 2, gen, density) * 0.5


def _assert_exact_sums(p, q, unit, what):
    """every partial sum of sum_k p[., k] q[k, .] is a multiple of `unit` below 2^24 units in magnitude: exact in fp32 in
    any order"""
    bound = (p.abs() @ q.abs()).max().item() / unit
    assert bound < 2 ** 24, f"{what}: a partial sum may reach {bound} units of {unit}: not exact in fp32"
    prod_units = (p.abs().max() * q.abs().max()).item() / unit
    assert prod_units == round(prod_units), f"{what}: products are not multiples of {unit}"


def _assert_bf16(t, what):
    assert torch.equal(t.to(bf16).to(f64), t), f"{what}: a value is not representable in bf16"


def exact_case(kind, M, W, r, layout, scale=0.5, seed=0):
    """exact operands for one kernel call: kind "down" (W = K), "up_add" (W = N) or "wgrad" (W = N).  Returns a dict of
    CPU tensors (bf16 operands, fp32 g) plus "scale" and "expect" (the restatement's result)."""
    assert kind in ("down", "up_add", "wgrad") and r in RANKS and W % 8 == 0
    assert scale in (0.25, 0.5, 1.0, 2.0, 4.0), "scale must be a power of two"
    gen = torch.Generator().manual_seed(1000 * seed + 7 * M + 3 * W + r + layout)
    if kind == "down":
        K = W
        dens = min(1.0, 96.0 / K)  # keeps |sum| small enough for an exact bf16 result at every K
        x = _ints((M, K), -2, 2, gen, dens)
        w = _dyadic((r, K), gen)
        _assert_exact_sums(x, w.t(), 0.5, "down")
        _assert_bf16(x, "x"), _assert_bf16(w, "w")
        _assert_bf16((x @ w.t()) * scale, "down: u")
        ws = w if layout == 0 else w.t().contiguous()
        c = dict(x=x.to(bf16), w=ws.to(bf16), scale=scale)
        c["expect"] = down(c["x"], c["w"], layout, scale)
    elif kind == "up_add":
        N = W
        u = _ints((M, r), -1, 1, gen)
        w = _dyadic((N, r), gen)
        y = _ints((M, N), -8, 8, gen)
        _assert_exact_sums(u, w.t(), 0.5, "up_add")
        for t, n in ((u, "u"), (w, "w"), (y, "y"), (y + (u @ w.t()) * scale, "up_add: y")):
            _assert_bf16(t, n)
        ws = w if layout == 0 else w.t().contiguous()
        c = dict(u=u.to(bf16), w=ws.to(bf16), y=y.to(bf16), scale=scale)
        c["expect"] = up_add(c["u"], c["w"], layout, c["y"], scale)
    else:
        N = W
        a = _ints((M, N), -3, 3, gen)
        u = _dyadic((M, r), gen)
        g = _ints((N, r), -5, 5, gen)  # the gradient buffer already holds something
        _assert_exact_sums(a.t(), u, 0.5, "wgrad")
        res = g + (a.t() @ u) * scale
        assert res.abs().max().item() / (0.5 * scale) < 2 ** 24 and torch.equal(res.to(f32).to(f64), res), "wgrad: g"
        _assert_bf16(a, "a"), _assert_bf16(u, "u")
        gs = g if layout == 0 else g.t().contiguous()
        c = dict(a=a.to(bf16), u=u.to(bf16), g=gs.to(f32), scale=scale)
        c["expect"] = wgrad(c["a"], c["u"], c["g"], layout, scale)
    return c


def windowed(t, fill, pad_rows=3, pad_cols=8):
    """(parent, window): `t` as a window of a wider, taller parent filled with `fill` (NaN, or a sentinel): the parent's
    guard bands must come back untouched and nothing in them may reach a result.  pad_cols is a multiple of 8."""
    R, Cc = t.shape
    parent = torch.full((R + 2 * pad_rows, Cc + 2 * pad_cols), fill, dtype=t.dtype)
    parent[pad_rows:pad_rows + R, pad_cols:pad_cols + Cc] = t
    return parent, (pad_rows, pad_cols, R, Cc)


def window_of(parent, win):
    r0, c0, R, Cc = win
    return parent[r0:r0 + R, c0:c0 + Cc]


def bands_intact(parent, win, fill):
    """every element outside the window still holds `fill` (NaN compares by bit pattern)"""
    r0, c0, R, Cc = win
    mask = torch.ones(parent.shape, dtype=torch.bool)
    mask[r0:r0 + R, c0:c0 + Cc] = False
    ref = torch.full(parent.shape, fill, dtype=parent.dtype)
    itype = torch.int16 if parent.dtype == bf16 else torch.int32
    return torch.equal(parent.view(itype)[mask], ref.view(itype)[mask])
