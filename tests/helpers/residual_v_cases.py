"""Residual-V with per-block lambdas that differ: the inputs, the plain high-precision references and the bounds shared by
the kernel test of `ops.dv0_reduce` (tests/test_kernels_gpu.py), the deep model cases (tests/test_workloads_gpu.py) and
the CPU tests of their detection power (tests/test_residual_v_cpu.py).  Everything here runs on the CPU.

Every block i > 0 mixes v_i = lam_i v_raw_i + (1 - lam_i) v_0 (model.py:129-130), so d v_0 collects
sum_i (1 - lam_i) dv_i over all blocks.  With every lambda at its initial 0.5 that sum cannot tell which lambda went with
which dv; the cases here can."""
import os

import torch

from oracle import dit_oracle as O

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64

# ------------------------------------------------------------------------------------ dv0_reduce ----
DV0_N = (1, 9, 10, 27, 32, 33, 40)              # around the model's chunk of 9 and the kernel's 32 pointers per launch
DV0_HEADS = ((72, 96), (64, 64), (128, 128))    # (head_dim, padded head_dim)
DV0_DIMS = (2, 2, 37)                           # B, H, L: 148 rows -- 148 * hd / 8 work items, no multiple of the 256 per workgroup
DV0_CHUNK = 9                                   # model._DV0_CHUNK's default
DV0_SENTINEL = 5.0
U32 = 2.0 ** -24                                # unit roundoff of fp32


def dv0_inputs(n, hd, hdp, seed=900):
    """n (dv_i, lam_i): lam_i = bf16(-0.25 + 1.5 i / n) -- distinct in bf16, not symmetric about 0.5, below 0 at i = 0 and
    above 1 for i > 5 n / 6 (the reference model does not clamp) --, dv_i = bf16((1 + i) * randn) with NaN in the pad
    columns (attention leaves them unwritten: they must never be read)"""
    B, H, L = DV0_DIMS
    g = torch.Generator().manual_seed(seed + 1000 * hd + n)
    lams = [torch.tensor([-0.25 + 1.5 * i / n]).to(bf16) for i in range(n)]
    assert len({float(l) for l in lams}) == n
    dvs = []
    for i in range(n):
        dv = ((1 + i) * torch.randn(B, H, L, hdp, generator=g)).to(bf16)
        dv[..., hd:] = float("nan")
        dvs.append(dv)
    return dvs, lams


def dv0_reference(dvs, lams, hd):
    """(want, scale) in float64: want = sum_i (1 - lam_i) dv_i[..., :hd], scale = sum_i |(1 - lam_i) dv_i[..., :hd]|"""
    terms = [(1.0 - l.to(f64)) * dv[..., :hd].to(f64) for dv, l in zip(dvs, lams)]
    return sum(terms), sum(t.abs() for t in terms)


def dv0_bound(n, scale):
    """the kernel forms each term in fp32 and adds the n of them in fp32: one rounding for 1 - lam, one per product, one
    per addition -> |got - want| <= (n + 2) 2^-24 sum_i |(1 - lam_i) dv_i| to first order; twice that is asserted"""
    return 2.0 * (n + 2) * U32 * scale


def dv0_rotated(lams):
    """the pairing a kernel that takes each lambda from the neighbouring pointer would use"""
    return lams[1:] + lams[:1]


def dv0_chunks(n, chunk=DV0_CHUNK):
    """the index lists DiTBlock._bwd hands to ops.dv0_reduce, in its order: the backward walks the blocks from the last
    to the first, appends each to the pending list and reduces it whenever it holds `chunk` entries, and once more at
    block 0 for what is left.  The first reduction overwrites the accumulator, the later ones add to it."""
    order = list(range(n - 1, -1, -1))
    return [order[k:k + chunk] for k in range(0, n, chunk)]


# ------------------------------------------------------------------------------- deep model case ----
# bf16 path against the fp32 oracle, per parameter tensor (tests/test_workloads_gpu.py uses these for all its cases).
# Measured on the MI355X (parity_report.jsonl, round 2): worst rel-L2 8.6e-3 (blocks.5.qkv.weight at depth 6), worst
# cosine 0.99997 -> bounds at ~2x the measured error
GRAD_COS, GRAD_REL = 0.9995, 2e-2
DEEP_DEPTH = 12          # > the chunk of 9 and > the 3 or 4 gathered-weight buffers of the reshard runtime
DEEP_ROPE_START = (1, 2, 3)
DEEP_HIDDEN = {"hd72": 144, "hd64": 128}


def deep_lambda(i):
    """blocks 1..11: 0.27 ... 0.97 in steps of 0.07 -- distinct in bf16 (spacing 2^-9 at most there), none 0.5; rounded to
    bf16 so that the fp32 oracle and the bf16 model mix with the same numbers"""
    return torch.tensor([0.2 + 0.07 * i]).to(bf16).float()


def deep_case(key, uniform_lambda=False):
    """(cfg, P, x, ctx, t, v) of the deep residual-V case: two heads of 72 (the padded path, with biases and norm weights)
    or of 64, depth 12, latent [2, 16, 4, 8, 8], 24 context tokens.  uniform_lambda: every lambda left at 0.5, the
    configuration the suite's gradient bounds were measured on."""
    cfg = O.DiTConfig(in_channels=16, hidden_size=DEEP_HIDDEN[key], depth=DEEP_DEPTH, num_heads=2,
                      cross_attn_input_size=64, residual_v=True, train_bias_and_rms=(key == "hd72"))
    P = O.init_params(cfg, seed=31, randomize_zero_init=True, init_std_factor=1.0)
    if not uniform_lambda:
        for i in range(1, cfg.depth):
            P[f"blocks.{i}.lambda_param"] = deep_lambda(i)
        lams = [float(P[f"blocks.{i}.lambda_param"]) for i in range(1, cfg.depth)]
        assert len(set(lams)) == cfg.depth - 1 and 0.5 not in lams
    g = torch.Generator().manual_seed(32)
    x = torch.randn(2, 16, 4, 8, 8, generator=g).to(bf16)
    ctx = torch.randn(2, 24, 64, generator=g).to(bf16)
    t = torch.tensor([0.35, 0.8]).to(bf16)
    v = torch.randn(2, 16, 4, 8, 8, generator=g).to(bf16)
    return cfg, P, x, ctx, t, v


def oracle_step_with_dv(cfg, P, x, ctx, t, v, start, sublayers=()):
    """fp32 oracle forward + loss + backward on the bf16-rounded inputs.  Returns (ref, dv): ref = (out, loss, grads,
    last block's sub-layer outputs), the reference tests/test_workloads_gpu.py::check_step compares with (its oracle_step is
    this function).  d loss / d lambda_i = sum(dv_i * (v_raw_i - v_0)) is a scalar made of B*L*D signed products that
    largely cancel; its natural error scale is the sum of the |products|, not the cancelled sum, so grads carries it per
    mixed block as `<name>.l1` (v_raw - v_0 = (v_mixed - v_0) / lambda, model.py:129-130).  The sub-layer outputs are those
    of the LAST block (the model output is blind to in-block errors -- with N(0, 0.02) gates a block contributes ~2 % of the
    residual stream -- so they are compared directly).  dv = {i: d loss / d v_i} for every block, v_i being the V that
    block i's attention consumed (mixed for i > 0) -- dv[0] is block 0's TOTAL, its own attention's share plus the fan-in
    from the mixing blocks.  Without residual-V: no `.l1` entries, dv empty."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    Pg = {k: w.clone().requires_grad_(True) for k, w in P.items()}
    cap = {}
    o_ref = O.dit_forward(Pg, cfg, x.float(), ctx.float(), t.float(), start, cap)
    vs = {i: cap[f"blocks.{i}.v"] for i in range(cfg.depth)} if cfg.residual_v else {}
    for vm in vs.values():
        vm.retain_grad()
    l_ref, _ = O.flow_loss(v, o_ref)
    l_ref.backward()
    grads = {k: w.grad for k, w in Pg.items() if w.grad is not None}
    v0 = vs[0].detach() if vs else None
    for i in range(1, cfg.depth if vs else 0):
        lam = P[f"blocks.{i}.lambda_param"].item()
        grads[f"blocks.{i}.lambda_param.l1"] = (vs[i].grad * (vs[i].detach() - v0) / lam).abs().sum()
    pre = f"blocks.{cfg.depth - 1}."
    subs = {n: cap[pre + n].detach() for n in sublayers if pre + n in cap}
    return (o_ref.detach(), l_ref.item(), grads, subs), {i: vm.grad.detach() for i, vm in vs.items()}


def fan_in(P, dv, shift=0):
    """sum_i (1 - lam_j) dv_i over the mixing blocks i = 1 .. depth - 1 with j = i (shift 0: what d v_0 receives), or with
    j rotated by `shift` positions among the mixing blocks: the pairing a backward produces that reads block i's lambda
    from a buffer another block's weights have been gathered into since (one buffer of the ring every `shift` blocks)"""
    idx = sorted(i for i in dv if i > 0)
    n = len(idx)
    return sum((1.0 - P[f"blocks.{idx[(k + shift) % n]}.lambda_param"].double()) * dv[i].double()
               for k, i in enumerate(idx))


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()
