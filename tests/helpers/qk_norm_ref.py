"""QK-norm references (tests/test_qk_norm_cpu.py, tests/test_qk_norm_gpu.py): float64 restatements of the normed qkv / RoPE
forward and backward on CPU tensors, and the wrapper that turns the fp32 oracle into the oracle of the normed model."""
import contextlib

import torch

f64, bf16 = torch.float64, torch.bfloat16
EPS = 1e-6


def _heads(x2d, B, L, H, hd, section):
    """section (0 q, 1 k, 2 v) of a token-major [B*L, 3*H*hd] tensor as [B, H, L, hd]"""
    D = H * hd
    return x2d[:, section * D:(section + 1) * D].reshape(B, L, H, hd).permute(0, 2, 1, 3)


def _rotate(x, cos, sin, inverse=False):
    """half-split rotation y1 = x1 c + x2 s, y2 = x2 c - x1 s (inverse: its transpose); cos / sin [L, hd/2]"""
    d = x.shape[-1] // 2
    x1, x2 = x[..., :d], x[..., d:]
    if inverse:
        sin = -sin
    return torch.cat([x1 * cos + x2 * sin, x2 * cos - x1 * sin], dim=-1)


def forward_ref(qkv, cos, sin, B, L, H, hd, eps=EPS):
    """qkv: bf16 [B*L, 3*H*hd]; cos / sin f32 [L, hd/2].  For q and k (section 0 / 1) returns (ref, partners), both float64
    [B, H, L, hd]: ref = rotation(bf16(x * rsqrt(mean_d(x^2) + eps))) without a final rounding -- the one rounding point
    between the norm and the rotation is the model's -- and partners = |x1n| + |x2n|, the magnitudes of the two normalised
    elements every output element is rotated from."""
    cos, sin = cos.to(f64), sin.to(f64)
    out = []
    for section in (0, 1):
        x = _heads(qkv, B, L, H, hd, section).to(f64)
        r = torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + eps)
        xn = (x * r).to(bf16).to(f64)
        d = hd // 2
        pair = xn[..., :d].abs() + xn[..., d:].abs()
        out.append((_rotate(xn, cos, sin), torch.cat([pair, pair], dim=-1)))
    return out


def backward_ref(dq, dk, qkv, cos, sin, B, L, H, hd, eps=EPS):
    """dq, dk: bf16 [B, H, L, hdp] (pad columns ignored); qkv: the forward's input.  For q and k returns (ref, scale, x),
    float64 [B, H, L, hd]: ref = r (g - y mean_d(g y)) with g = the inverse rotation of the gradient, y = x r, nothing
    rounded; scale = r (|g| + |y| |mean_d(g y)|), the size of the two terms whose difference ref is; x = the raw rows."""
    cos, sin = cos.to(f64), sin.to(f64)
    out = []
    for section, grad in ((0, dq), (1, dk)):
        x = _heads(qkv, B, L, H, hd, section).to(f64)
        g = _rotate(grad[..., :hd].to(f64), cos, sin, inverse=True)
        r = torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + eps)
        y = x * r
        m = (g * y).mean(dim=-1, keepdim=True)
        out.append((r * (g - y * m), r * (g.abs() + y.abs() * m.abs()), x))
    return out


@contextlib.contextmanager
def qk_normed_oracle():
    """For the duration of the block, oracle.dit_oracle.apply_rotary -- which block_forward calls on q and k only -- is
    rms_norm followed by the rotation: the oracle of a model built with qk_norm=True.  Restored on exit."""
    from oracle import dit_oracle as O
    orig = O.apply_rotary

    def wrapped(x, cos, sin):
        return orig(O.rms_norm(x), cos, sin)

    O.apply_rotary = wrapped
    try:
        yield
    finally:
        O.apply_rotary = orig
