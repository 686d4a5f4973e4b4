"""GPU tests of Muon (csrc/muon.hip, optim.MuonAdamW): the three kernels against the torch restatement of
tests/helpers/muon_ref.py, a tiny DiT trained with MuonAdamW, a resume and a graph replay.

Bars:
    orthogonalisation : err_gpu = ||O_gpu - O_f64||_F / ||O_f64||_F <= 2 x err_emul, err_emul the same figure for the
                        bf16-emulated restatement (rounds u, X, A, B to bf16 where the kernels store them), computed
                        here.  The factor 2 covers a different fp32 summation order flipping bf16 roundings.
    momentum / update : fp32 arithmetic, 1e-6 of the largest magnitude per tensor (each element is two or three fp32
                        operations, 2^-24 = 6e-8 relative each, contracted into fmas or not); u is stored as bf16: one
                        bf16 rounding (2^-8 relative) of the float64 value.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import muon_ref as R  # noqa: E402

from oracle import dit_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
CONSTS = ["patch_proj", "context_kv", "positional_embedding"]
SHAPES = [(64, 64), (136, 136), (264, 264), (128, 512), (512, 128), (200, 328)]
NMATS = [1, 3, 7]


@pytest.fixture(scope="module")
def vds():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import model, ops, optim, train
    return dict(model=model, ops=ops, optim=optim, train=train)


def bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16) if t.dtype == bf16 else t.view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def guard_record(coef=1.0, skipped=0):
    rec = torch.zeros(4, dtype=torch.int32)
    rec.view(f32)[1] = coef
    rec[2] = skipped
    return rec.cuda()


class Group:
    """nmat matrices [rows, cols] given as offset slices of ONE parameter / gradient / momentum buffer, as split qkv is"""

    def __init__(self, vds, nmat, rows, cols, seed, shadow=True, ema=False):
        g = torch.Generator().manual_seed(seed)
        self.nmat, self.rows, self.cols = nmat, rows, cols
        self.p = (torch.randn(nmat * rows, cols, generator=g) * 0.05).cuda()
        self.g = torch.randn(nmat * rows, cols, generator=g).cuda()
        self.buf = (torch.randn(nmat * rows, cols, generator=g) * 0.5).cuda()
        self.pb = torch.zeros(nmat * rows, cols, dtype=bf16).cuda() if shadow else None
        self.ema = (torch.randn(nmat * rows, cols, generator=g) * 0.05).cuda() if ema else None
        ops = vds["ops"]
        n = rows * cols
        self.table = ops.muon_table([(self.p.data_ptr() + 4 * k * n, self.g.data_ptr() + 4 * k * n,
                                      self.buf.data_ptr() + 4 * k * n,
                                      None if self.pb is None else self.pb.data_ptr() + 2 * k * n,
                                      None if self.ema is None else self.ema.data_ptr() + 4 * k * n)
                                     for k in range(nmat)], "cuda")
        self.ws = torch.empty(ops.muon_workspace_bytes(nmat, rows, cols), dtype=torch.uint8, device="cuda")
        self.views = ops.muon_views(self.ws, nmat, rows, cols)

    def mats(self, t):
        return t.view(self.nmat, self.rows, self.cols)

    def x0(self):
        """workspace slot 0 in the orientation of the matrices"""
        x = self.views["x0"]
        return x.transpose(1, 2) if self.rows > self.cols else x


# ------------------------------------------------------------------------------------ kernel level
_REF = {}


def reference(nmat, rows, cols):
    """seeded Gaussian u and its two restated orthogonalisations, computed once per case"""
    key = (nmat, rows, cols)
    if key not in _REF:
        g = torch.Generator().manual_seed(1000 * nmat + rows + 3 * cols)
        u = torch.randn(nmat, rows, cols, generator=g)
        o64 = torch.stack([R.orthogonalize_f64(u[k]) for k in range(nmat)])
        oem = torch.stack([R.orthogonalize_emulated(u[k]) for k in range(nmat)])
        _REF[key] = (u, o64, oem)
    return _REF[key]


@pytest.mark.parametrize("nmat", NMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_orthogonalize_matches_restatement(vds, parity_log, shape, nmat):
    """momentum (mu = 0, zero buffer: u = g) -> orthogonalize on nmat offset slices of one buffer; every matrix within
    2 x the emulated restatement's own error against float64; a second run on the same input is bit-equal"""
    rows, cols = shape
    u, o64, oem = reference(nmat, rows, cols)
    G = Group(vds, nmat, rows, cols, seed=1)
    G.g.copy_(u.view(nmat * rows, cols))
    G.buf.zero_()
    ops = vds["ops"]
    outs = []
    for _ in range(2):
        G.buf.zero_()
        ops.muon_momentum(G.table.data_ptr(), nmat, rows, cols, 0.0, False, None, G.ws)
        ops.muon_orthogonalize(G.ws, nmat, rows, cols, 5)
        torch.cuda.synchronize()
        outs.append(G.x0().clone())
    assert same_bits(outs[0].contiguous(), outs[1].contiguous())
    got = outs[0].float().cpu()
    assert torch.isfinite(got).all()
    worst = 0.0
    for k in range(nmat):
        e_gpu, e_emul = R.rel_fro(got[k], o64[k]), R.rel_fro(oem[k], o64[k])
        worst = max(worst, e_gpu / e_emul)
        print(f"orthogonalize [{rows}, {cols}] matrix {k}/{nmat}: err_gpu {e_gpu:.5f} err_emul {e_emul:.5f} "
              f"ratio {e_gpu / e_emul:.3f}")
        assert e_gpu <= 2.0 * e_emul, (k, e_gpu, e_emul)
    parity_log("test_muon_gpu.orthogonalize", rows=rows, cols=cols, nmat=nmat, worst_ratio=worst)


def test_sumsq_matches_fp64_and_is_reproducible(vds):
    G = Group(vds, 3, 200, 328, seed=5)
    seen = []
    for _ in range(2):
        buf0 = G.buf.clone()
        vds["ops"].muon_momentum(G.table.data_ptr(), 3, 200, 328, 0.95, True, None, G.ws)
        torch.cuda.synchronize()
        seen.append(G.views["sumsq"].clone())
        u, _ = R.momentum_f64(G.mats(G.g).cpu(), G.mats(buf0).cpu(), 0.95, True)
        want = u.pow(2).sum(dim=(1, 2))
        assert ((seen[-1].double().cpu() - want).abs() <= 1e-6 * want).all()
        G.buf.copy_(buf0)
    assert same_bits(seen[0], seen[1])


@pytest.mark.parametrize("shape", [(128, 512), (512, 128), (200, 328)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("nesterov", [True, False], ids=["nesterov", "plain"])
def test_momentum_and_update_match_float64(vds, shape, nesterov):
    """wide, tall (the transposed path) and partial-tile shapes; weight decay; the bf16 shadow is exactly bf16(p); EMA"""
    rows, cols = shape
    nmat, mu, lr, wd, d = 3, 0.9, 0.02, 0.1, 0.99
    G = Group(vds, nmat, rows, cols, seed=7, ema=True)
    ops = vds["ops"]
    p0, buf0, ema0 = G.p.clone(), G.buf.clone(), G.ema.clone()
    ops.muon_momentum(G.table.data_ptr(), nmat, rows, cols, mu, nesterov, None, G.ws)
    torch.cuda.synchronize()
    u64, b64 = R.momentum_f64(G.mats(G.g).cpu(), G.mats(buf0).cpu(), mu, nesterov)
    assert (G.mats(G.buf).double().cpu() - b64).abs().max() <= 1e-6 * b64.abs().max()
    u_gpu = G.x0().float().cpu().double()
    assert ((u_gpu - u64).abs() <= 2.0 ** -8 * u64.abs() + 1e-6 * u64.abs().max()).all()
    # update from a known O: seeded bf16 values written into the workspace in its own orientation
    o = (torch.randn(nmat, rows, cols, generator=torch.Generator().manual_seed(9)) * 0.1).to(bf16)
    G.views["x0"].copy_((o.transpose(1, 2) if rows > cols else o).contiguous())
    ops.muon_update(G.table.data_ptr(), nmat, rows, cols, lr, wd, 0.5, d, None, None, G.ws)  # lr x multiplier 0.5
    torch.cuda.synchronize()
    for k in range(nmat):
        p64, e64 = R.update_f64(G.mats(p0)[k].cpu(), o[k].float(), lr * 0.5, wd, G.mats(ema0)[k].cpu(), d)
        assert (G.mats(G.p)[k].double().cpu() - p64).abs().max() <= 1e-6 * p64.abs().max()
        assert (G.mats(G.ema)[k].double().cpu() - e64).abs().max() <= 1e-6 * e64.abs().max()
    assert same_bits(G.pb, G.p.to(bf16))
    assert not torch.equal(G.p, p0)


def test_update_reads_the_device_scalars(vds):
    """with scalars_dev the LR multiplier and the EMA decay come from device memory, not from the arguments"""
    rows, cols, nmat = 64, 64, 1
    G = Group(vds, nmat, rows, cols, seed=8, ema=True)
    p0, ema0 = G.p.clone(), G.ema.clone()
    o = (torch.randn(nmat, rows, cols, generator=torch.Generator().manual_seed(2)) * 0.1).to(bf16)
    G.views["x0"].copy_(o)
    sc = torch.tensor([0.0, 0.0, 0.25, 0.9], dtype=f32).cuda()
    vds["ops"].muon_update(G.table.data_ptr(), nmat, rows, cols, 0.02, 0.0, 123.0, 0.5, sc.data_ptr(), None, G.ws)
    torch.cuda.synchronize()
    p64, e64 = R.update_f64(p0.cpu(), o[0].float(), 0.02 * 0.25, 0.0, ema0.cpu(), 0.9)
    assert (G.p.double().cpu() - p64).abs().max() <= 1e-6 * p64.abs().max()
    assert (G.ema.double().cpu() - e64).abs().max() <= 1e-6 * e64.abs().max()


@pytest.mark.parametrize("shape", [(64, 64), (512, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_skipped_step_keeps_every_bit_and_clip_scales_the_gradient(vds, shape):
    rows, cols = shape
    nmat = 3
    G = Group(vds, nmat, rows, cols, seed=11, ema=True)
    G.g[5, 3] = float("nan")
    G.pb.copy_(G.p.to(bf16))
    ops = vds["ops"]
    keep = [t.clone() for t in (G.p, G.buf, G.pb, G.ema)]
    rec = guard_record(coef=0.5, skipped=1)
    ops.muon_momentum(G.table.data_ptr(), nmat, rows, cols, 0.95, True, rec.data_ptr(), G.ws)
    ops.muon_orthogonalize(G.ws, nmat, rows, cols, 5)
    ops.muon_update(G.table.data_ptr(), nmat, rows, cols, 0.02, 0.1, 1.0, 0.9, None, rec.data_ptr(), G.ws)
    torch.cuda.synchronize()
    for a, b in zip((G.p, G.buf, G.pb, G.ema), keep):
        assert same_bits(a, b)
    # an applied step with a clip coefficient below 1: the momentum sees coef * g
    G.g[5, 3] = 0.25
    rec = guard_record(coef=0.5, skipped=0)
    buf0 = G.buf.clone()
    ops.muon_momentum(G.table.data_ptr(), nmat, rows, cols, 0.95, True, rec.data_ptr(), G.ws)
    torch.cuda.synchronize()
    u64, b64 = R.momentum_f64(G.mats(G.g).cpu(), G.mats(buf0).cpu(), 0.95, True, coef=0.5)
    assert (G.mats(G.buf).double().cpu() - b64).abs().max() <= 1e-6 * b64.abs().max()
    u_gpu = G.x0().float().cpu().double()
    assert ((u_gpu - u64).abs() <= 2.0 ** -8 * u64.abs() + 1e-6 * u64.abs().max()).all()


# ------------------------------------------------------------------------------------- model level
def tiny_cfg():
    return O.DiTConfig(in_channels=16, hidden_size=128, depth=3, num_heads=2, cross_attn_input_size=64,
                       residual_v=True, train_bias_and_rms=False)


def build(vds, cfg, P):
    m = vds["model"].DiT(in_channels=cfg.in_channels, patch_size=cfg.patch_size, time_patch_size=cfg.time_patch_size,
                         hidden_size=cfg.hidden_size, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio,
                         cross_attn_input_size=cfg.cross_attn_input_size, residual_v=cfg.residual_v,
                         train_bias_and_rms=cfg.train_bias_and_rms)
    m.load_state_dict(P, strict=True)
    return m.to("cuda")


def make_batches(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [{"latent": torch.randn(2, 16, 4, 8, 8, generator=g).cuda(), "context": torch.randn(2, 16, 64, generator=g).cuda(),
             "prompt": ["", ""]} for _ in range(n)]


@pytest.fixture(scope="module")
def tiny_params():
    return O.init_params(tiny_cfg(), seed=41, randomize_zero_init=True, init_std_factor=1.0)


def test_three_train_steps_match_the_restatement(vds, tiny_params, parity_log):
    """tiny DiT (hidden 128, 2 heads, depth 3, cross-attention), three train_steps with MuonAdamW: after each step every
    Muon-managed parameter's update matches the float64 restatement applied to the same p.grad within the kernel bar
    (2 x the emulated restatement's error), and the AdamW-managed parameters are bit-equal to a MuAdamW fed the same
    gradients"""
    MUON_LR = 0.02
    m = build(vds, tiny_cfg(), tiny_params)
    groups, table = m.get_muon_setup(3e-3, 0.1, CONSTS, muon_lr=MUON_LR)
    opt = vds["optim"].MuonAdamW(groups, betas=(0.95, 0.99))
    named = dict(m.named_parameters())
    muon = {n: table[n]["split"] for n in named if table.get(n, {}).get("muon")}
    assert len(muon) == 7 * 3
    # the AdamW twin: the same non-Muon groups over copies of the parameters
    twin = {n: torch.nn.Parameter(p.detach().clone()) for n, p in named.items() if n not in muon}
    twin_of = {id(named[n]): twin[n] for n in twin}
    opt2 = vds["optim"].MuAdamW([dict(g, params=[twin_of[id(p)] for p in g["params"]]) for g in groups
                                 if not g.get("use_muon")], betas=(0.95, 0.99))
    seen = []
    real_step = opt.step

    def recording_step(*a, **k):
        seen.append({n: (p.detach().clone(), p.grad.detach().clone()) for n, p in named.items() if p.grad is not None})
        return real_step(*a, **k)
    opt.step = recording_step
    torch.manual_seed(77)
    torch.cuda.manual_seed(77)
    bufs = {n: torch.zeros(named[n].shape, dtype=torch.float64) for n in muon}
    worst = 0.0
    for step, b in enumerate(make_batches(3)):
        vds["train"].train_step(m, opt, None, b, "cuda")
        torch.cuda.synchronize()
        before = seen[-1]
        for n, split in muon.items():
            p0, g = (t.cpu() for t in before[n])
            want, nb = R.step_f64(p0, g, bufs[n], MUON_LR, 0.0, split=split)
            emul, _ = R.step_f64(p0, g, bufs[n], MUON_LR, 0.0, split=split, emulated=True)
            bufs[n] = nb
            d_gpu, d_want, d_emul = named[n].detach().double().cpu() - p0.double(), want - p0.double(), emul - p0.double()
            e_gpu, e_emul = R.rel_fro(d_gpu, d_want), R.rel_fro(d_emul, d_want)
            worst = max(worst, e_gpu / e_emul)
            assert e_gpu <= 2.0 * e_emul, (step, n, e_gpu, e_emul)
            mb = opt.state[named[n]]["momentum_buffer"]
            assert mb.dtype == f32 and mb.shape == named[n].shape
            assert (mb.double().cpu() - nb).abs().max() <= 1e-6 * nb.abs().max() * (step + 1)
        for n, q in twin.items():
            q.grad = before[n][1].clone() if n in before else None
        opt2.step()
        torch.cuda.synchronize()
        for n, q in twin.items():
            assert same_bits(q, named[n]), (step, n)
    print(f"model level: worst err_gpu / err_emul over 3 steps x 21 parameters: {worst:.3f}")
    parity_log("test_muon_gpu.model", worst_ratio=worst)


def test_resume_is_bit_exact_in_deterministic_mode(vds, tiny_params):
    """state_dict -> fresh optimizer -> load_state_dict: the next step equals the uninterrupted run to the bit"""
    ops = vds["ops"]
    prev = ops.set_deterministic(True, workspace_bytes=64 << 20)
    try:
        finals = []
        for resume in (False, True):
            m = build(vds, tiny_cfg(), tiny_params)
            groups, _ = m.get_muon_setup(3e-3, 0.1, CONSTS)
            kw = dict(betas=(0.95, 0.99), max_grad_norm=1.0, ema_decay=0.99)
            opt = vds["optim"].MuonAdamW(groups, **kw)
            torch.manual_seed(78)
            torch.cuda.manual_seed(78)
            for i, b in enumerate(make_batches(3, seed=6)):
                if resume and i == 2:
                    sd = opt.state_dict()
                    groups, _ = m.get_muon_setup(3e-3, 0.1, CONSTS)
                    opt = vds["optim"].MuonAdamW(groups, **kw)
                    opt.load_state_dict(sd)
                vds["train"].train_step(m, opt, None, b, "cuda")
            torch.cuda.synchronize()
            st = {n: opt.state[p] for n, p in m.named_parameters()}
            finals.append(({n: p.detach().clone() for n, p in m.named_parameters()},
                           {n: s["momentum_buffer"].clone() for n, s in st.items() if "momentum_buffer" in s},
                           {n: s["ema"].clone() for n, s in st.items() if "ema" in s}))
        assert len(finals[0][1]) == 21 and set(finals[0][1]) <= set(finals[0][2])
        for a, b in zip(finals[0], finals[1]):
            assert a.keys() == b.keys()
            for n in a:
                assert same_bits(a[n], b[n]), n
    finally:
        ops.set_deterministic(prev)


def test_graph_replay_matches_eager_steps_with_muon(vds, tiny_params):
    """GraphedTrainStep with MuonAdamW: two eager steps, capture, three replays under a cosine schedule; the losses
    agree with five eager steps within the bound of test_graph_replay_matches_eager_steps (1e-4 relative)"""
    from video_diffusion_speedrun_amd.graph import GraphedTrainStep
    batches = make_batches(5)
    results = []
    for graphed in (False, True):
        m = build(vds, tiny_cfg(), tiny_params)
        groups, _ = m.get_muon_setup(3e-3, 0.1, CONSTS)
        opt = vds["optim"].MuonAdamW(groups, betas=(0.95, 0.99))
        sched = vds["train"].get_schedule(opt, "cosine", 3, 50)
        torch.manual_seed(77)
        torch.cuda.manual_seed(77)
        losses = []
        if graphed:
            gs = GraphedTrainStep(m, opt, sched, "cuda", eager_steps=2)
            for b in batches:
                losses.append(gs.step(b).item())
            assert gs.n_replays == 3 and opt._step == 5
        else:
            for b in batches:
                losses.append(vds["train"].train_step(m, opt, sched, b, "cuda").item())
        torch.cuda.synchronize()
        results.append(losses)
    l0, l1 = results
    print("eager ", l0, "\nreplay", l1)
    assert len(set(l0)) == 5
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
