"""Muon, restated in torch on the CPU from the algorithm -- the expected values of the Muon tests.

    g' = coef g;  buf = mu buf + g';  u = g' + mu buf (nesterov) | buf
    X = u / (||u||_F + 1e-7);  `steps` times:  A = X X^T,  B = b A + c A A,  X = a X + B X
    p = p (1 - lr wd) - lr sqrt(max(1, rows / cols)) O

Two forms of the orthogonalisation: float64, and "bf16-emulated" -- u, X, A and B rounded to bf16 where the kernels store
them, products of bf16-valued operands summed in fp32 (a different summation order than the MFMA's)."""
import math

import torch

NS_A, NS_B, NS_C = 3.4445, -4.7750, 2.0315
EPS = 1e-7


def momentum_f64(g, buf, mu, nesterov, coef=1.0):
    """-> (u, new buf), float64"""
    g = g.double() * coef
    buf = mu * buf.double() + g
    return (g + mu * buf if nesterov else buf), buf


def orthogonalize_f64(u, steps=5):
    """u [rows, cols] -> O [rows, cols], float64; the iteration runs on the orientation with the fewer rows"""
    X = u.double()
    tall = X.shape[0] > X.shape[1]
    if tall:
        X = X.t()
    X = X / (X.norm() + EPS)
    for _ in range(steps):
        A = X @ X.t()
        B = NS_B * A + NS_C * (A @ A)
        X = NS_A * X + B @ X
    return X.t() if tall else X


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def orthogonalize_emulated(u, steps=5):
    """the same with the kernels' roundings: u (fp32 in), X, A, B stored as bf16; fp32 products and sums"""
    u = u.float()
    tall = u.shape[0] > u.shape[1]
    if tall:
        u = u.t()
    norm = u.double().pow(2).sum().sqrt().float()   # the kernels sum the squares of the fp32 u
    X = _bf(_bf(u) * (1.0 / (norm + EPS)))
    for _ in range(steps):
        A = _bf(X @ X.t())
        B = _bf(NS_C * (A @ A) + NS_B * A)
        X = _bf(B @ X + NS_A * X)
    return (X.t() if tall else X).double()


def update_f64(p, O, lr, wd, ema=None, ema_decay=None):
    """-> (new p, new ema | None), float64"""
    rows, cols = p.shape
    p = p.double() * (1.0 - lr * wd) - lr * math.sqrt(max(1.0, rows / cols)) * O.double()
    if ema is not None:
        ema = ema_decay * ema.double() + (1.0 - ema_decay) * p
    return p, ema


def step_f64(p, g, buf, lr, wd, mu=0.95, nesterov=True, steps=5, split=1, coef=1.0, emulated=False):
    """one Muon step of a parameter made of `split` matrices stacked along its rows -> (new p, new buf), float64"""
    rows = p.shape[0] // split
    ps, bs = [], []
    orth = orthogonalize_emulated if emulated else orthogonalize_f64
    for k in range(split):
        sl = slice(k * rows, (k + 1) * rows)
        u, b = momentum_f64(g[sl], buf[sl], mu, nesterov, coef)
        pn, _ = update_f64(p[sl], orth(u, steps), lr, wd)
        ps.append(pn)
        bs.append(b)
    return torch.cat(ps), torch.cat(bs)


def rel_fro(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()
