"""Head RMS-norm references (tests/test_head_norm_cpu.py, tests/test_head_norm_kernels_gpu.py, tests/test_head_norm_gpu.py),
on CPU tensors, written from the definitions in include/vds.h.

  forward_ref / backward_ref   float64 restatements of vds_head_rmsnorm_fwd / _bwd: nothing rounded.  `fault` injects one of
                               FAULTS -- what the bitwise compare on the exact inputs has to flag.
  exact_forward / exact_backward   inputs on which the right bf16 output is ONE bit pattern whatever the order of the fp32
                               additions: every product and sum is exact, and the builder asserts that the one inexact
                               intermediate (r, resp. the mean) may move by a relative 2^-21 without a bit changing.
  cross_normed_oracle          the fp32 oracle of a model built with qk_norm="all": its cross-attention norms q and k."""
import contextlib

import torch

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16
EPS = 1e-6
FAULTS = ("no_eps", "mean_hd_plus_1", "last_head_skipped", "neighbour_r")
SLACK = 2.0 ** -21


def _heads(x, H, hd):
    M = x.shape[0]
    assert x.dim() == 2 and x.shape[1] == H * hd, (tuple(x.shape), H, hd)
    return x.to(f64).reshape(M, H, hd)


def forward_ref(x, H, hd, eps=EPS, fault=None):
    """x: [M, H * hd] (bf16 values) -> (y float64 [M, H * hd] = x * r, unrounded; r float64 [M, H])"""
    assert fault is None or fault in FAULTS
    xh = _heads(x, H, hd)
    n = hd + 1 if fault == "mean_hd_plus_1" else hd
    r = torch.rsqrt((xh * xh).sum(dim=-1) / n + (0.0 if fault == "no_eps" else eps))
    ra = r.roll(1, dims=1) if fault == "neighbour_r" else r
    y = xh * ra[..., None]
    if fault == "last_head_skipped":
        y[:, H - 1] = xh[:, H - 1]
    return y.reshape(x.shape[0], H * hd), r


def backward_ref(dy, y, rstd, H, hd, fault=None):
    """dy, y: [M, H * hd] (bf16 values; y = the stored normed rows), rstd [M, H] (the stored fp32 r) ->
    (dx float64 [M, H * hd] = r (g - y mean_d(g y)), unrounded; scale = r (|g| + |y| |mean_d(g y)|), the size of the two
    terms whose difference dx is)"""
    assert fault is None or fault in FAULTS
    g, yh = _heads(dy, H, hd), _heads(y, H, hd)
    r = rstd.to(f64).reshape(-1, H)
    if fault == "neighbour_r":
        r = r.roll(1, dims=1)
    n = hd + 1 if fault == "mean_hd_plus_1" else hd
    mu = (g * yh).sum(dim=-1, keepdim=True) / n
    dx = r[..., None] * (g - yh * mu)
    if fault == "last_head_skipped":
        dx[:, H - 1] = g[:, H - 1]
    scale = r[..., None] * (g.abs() + yh.abs() * mu.abs())
    M = dy.shape[0]
    return dx.reshape(M, H * hd), scale.reshape(M, H * hd)


# ----------------------------------------------------------------------------------------- exact inputs ----
def pattern_counts(hd):
    """(twos, ones, zeros) of a head row c_i in {0, +-1, +-2} with sum c_i^2 = hd"""
    assert hd % 8 == 0 and hd >= 8
    twos, ones = (6, 48) if hd == 72 else (hd // 8, hd // 2)
    assert 4 * twos + ones == hd and twos + ones <= hd
    return twos, ones, hd - twos - ones


def _patterns(M, H, hd, g):
    """integer rows c [M, H, hd] (float64): per row a random placement and random signs of pattern_counts(hd)"""
    twos, ones, zeros = pattern_counts(hd)
    base = torch.tensor([2.0] * twos + [1.0] * ones + [0.0] * zeros, dtype=f64)
    perm = torch.rand(M, H, hd, generator=g).argsort(dim=-1)
    sign = torch.randint(0, 2, (M, H, hd), generator=g).to(f64) * 2 - 1
    return base[perm] * sign


def _same_bits(a, b):
    return torch.equal(a.to(bf16).view(torch.int16), b.to(bf16).view(torch.int16))


def zero_row(i):
    """the head rows (numbered m * H + h) the exact forward input leaves at zero"""
    return i % 7 == 3


def exact_forward(M, H, hd, seed=0, eps=EPS):
    """-> (x bf16 [M, H * hd], want bf16 [M, H * hd], r float64 [M, H]).  Row (m, h) is c_i * 2^a with a in -5 .. 4 drawn
    per row: the mean square is 4^a exactly, r = rsqrt(4^a + eps) and x r rounds to c_i.  Rows with zero_row(m H + h) are
    zero: r = rsqrt(eps), output 0."""
    g = torch.Generator().manual_seed(1000 * hd + 10 * H + M + seed)
    c = _patterns(M, H, hd, g)
    a = torch.randint(-5, 5, (M, H), generator=g)
    zero = torch.tensor([zero_row(i) for i in range(M * H)]).reshape(M, H)
    x = torch.where(zero[..., None], torch.zeros_like(c), c * (2.0 ** a.to(f64))[..., None])
    want = torch.where(zero[..., None], torch.zeros_like(c), c)
    assert torch.equal(x.to(bf16).to(f64), x)  # the inputs are bf16 values
    ms = (x * x).sum(dim=-1) / hd
    assert torch.equal(ms, torch.where(zero, torch.zeros_like(ms), 4.0 ** a.to(f64)))
    r = torch.rsqrt(ms + eps)
    for d in (-SLACK, 0.0, SLACK):  # the one inexact intermediate may move: no output bit depends on it
        assert _same_bits(x * (r * (1 + d))[..., None], want), d
    return x.reshape(M, H * hd).to(bf16), want.reshape(M, H * hd).to(bf16), r


def exact_backward(M, H, hd, k, seed=0):
    """-> (dy bf16, y bf16, rstd f32 [M, H], want bf16).  rstd = 2^k (k an int or an int tensor [M, H]); y the integer
    pattern rows; g = mu y + n with an integer mu in -3 .. 3 per row and integer noise n, |n| <= 3, with sum n y = 0:
    sum g y = mu hd, the mean is mu and the right output is 2^k n."""
    g = torch.Generator().manual_seed(2000 * hd + 10 * H + M + seed)
    y = _patterns(M, H, hd, g)
    mu = torch.randint(-3, 4, (M, H, 1), generator=g).to(f64)
    twos, n_ones, _ = pattern_counts(hd)
    assert n_ones % 2 == 0 and 4 * twos <= n_ones
    # n = s sign(y) with integer s, NON-ZERO wherever y is (where y mu is subtracted the result must not be a difference
    # that is zero only for the exact mean) and sum_i s_i |y_i| = 0:
    #   on the twos    s in {+-1, +-2} at random: they contribute S2 = 2 sum s, even, |S2| <= 4 twos <= the number of ones;
    #   on the ones    +1 / -1 alternating in column order (sum 0), then -S2 spread in units over the ones whose sign it has
    #                  (half of them; at most 2 units each, so |s| <= 3 and none becomes 0);
    #   on the zeros   any integer in -3 .. 3.
    is2, is1 = (y.abs() == 2), (y.abs() == 1)
    s2 = (torch.randint(1, 3, (M, H, hd), generator=g) * (torch.randint(0, 2, (M, H, hd), generator=g) * 2 - 1)).to(f64) * is2
    adj = -2 * s2.sum(dim=-1, keepdim=True)                    # what the ones have to add up to
    rank = is1.to(f64).cumsum(dim=-1)                          # 1-based rank among the row's ones
    base = torch.where(rank % 2 == 1, 1.0, -1.0)
    j = ((rank - 1) // 2).clamp(min=0)                         # index among the ones of one sign
    half = n_ones // 2
    q = adj.abs()
    units = (q // half) + (j < q % half).to(f64)
    s1 = (base + torch.where(base == adj.sign(), units * adj.sign(), torch.zeros_like(units))) * is1
    n = (s2 + s1) * y.sign() + torch.randint(-3, 4, (M, H, hd), generator=g).to(f64) * (y == 0)
    assert torch.equal((n * y).sum(dim=-1), torch.zeros(M, H, dtype=f64))
    assert bool(((n != 0) | (y == 0)).all()) and float(n.abs().max()) <= 3
    gy = mu * y + n
    assert torch.equal((gy * y).sum(dim=-1, keepdim=True), mu * hd)
    r = 2.0 ** (k.to(f64) if isinstance(k, torch.Tensor) else torch.full((M, H), float(k), dtype=f64))
    want = r[..., None] * n
    for v in (gy, y, want):
        assert torch.equal(v.to(bf16).to(f64), v)
    for d in (-SLACK, 0.0, SLACK):
        assert _same_bits(r[..., None] * (gy - y * (mu * (1 + d))), want), d
    flat = lambda v: v.reshape(M, H * hd).to(bf16)
    return flat(gy), flat(y), r.to(f32), flat(want)


# ----------------------------------------------------------------------------------------------- oracle ----
@contextlib.contextmanager
def cross_normed_oracle():
    """For the duration of the block, a call of oracle.dit_oracle.attention whose key count differs from its query count --
    the cross-attention, in a test that chooses Lc != L -- norms q and k with oracle.rms_norm first: the oracle of a model
    built with qk_norm="all" once qk_norm_ref.qk_normed_oracle() wraps the self-attention as well (the two nest in either
    order).  The helper models' own masked cross-attention (frame_causal_ref.cross_attention with context_lens, which does
    not go through oracle.attention) is wrapped the same way when that helper is loaded.  Restored on exit."""
    import sys
    from oracle import dit_oracle as O
    orig = O.attention

    def attention(q, k, v):
        if k.shape[-2] != q.shape[-2]:
            q, k = O.rms_norm(q), O.rms_norm(k)
        return orig(q, k, v)

    FC = sys.modules.get("frame_causal_ref")
    orig_cross = FC.cross_attention if FC is not None else None

    def cross_attention(q, k, v, context_lens):
        if context_lens is None:  # goes through O.attention, which norms
            return orig_cross(q, k, v, context_lens)
        return orig_cross(O.rms_norm(q), O.rms_norm(k), v, context_lens)

    O.attention = attention
    if FC is not None:
        FC.cross_attention = cross_attention
    try:
        yield
    finally:
        O.attention = orig
        if FC is not None:
            FC.cross_attention = orig_cross
