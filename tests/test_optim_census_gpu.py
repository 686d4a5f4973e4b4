"""Exact census of the optimizer kernels on the GPU: bits against tests/helpers/optim_census.py.

Every call goes through the C entry point with tables built here (MuAdamW fixes chunk_elems, so it cannot serve).  Every
buffer -- p, g, m, v, the shadow, the EMA, buf, the sum-of-squares workspace, the Muon workspace -- lies between two
guard bands: inputs are NaN outside the payload, outputs hold a sentinel no case produces, the Muon workspace is all
ones bits (NaN in bf16 and fp32) wherever the test did not write.  After the call the payload equals the expectation bit
for bit, the gradients and every byte outside a payload are what they were: the gaps of the 256-byte padding between the
workspace sections too.

Kernel -> cases (lists and predicates in the helper; test_optim_census_cpu.py asserts the coverage):
  adamw_kernel<false|true>       extents 1 3 4 5 1023 1024 1025 2044 2047 2048 2049 3076 4096 4097 65541 x the four
                                 entries; chunk_elems 4 1028 1030 2048, chunks shuffled / reversed; each of p g m v
                                 shadow EMA alone displaced; NULL shadows, NULL EMA entries, a NULL table; coef 1 and
                                 1/2; skipped; n_chunks 0                              test_adamw_exact
                                 the real constants, steps 1 and 7, per-element bound  test_adamw_real_constants
  grad_sumsq_partial / _final    the same extents + 8191 8192 8193, chunk_elems 4 (275 chunks: two trips of stage 2)
                                 1028 1030 2048 4096, g displaced, n_chunks 0          test_sumsq
  guard_finalize                 8 x 3 x 8 x 2 table through vds_optim_guard_finalize, 8 x 8 x 2 through the fused
                                 second stage                                          test_finalize
  muon_momentum / _sumsq_final   six shapes x nmat 1 3 x Nesterov, mu 1/2 3/4, coef 1 1/2   test_muon_momentum
  muon_normalize_kernel          steps = 0, general bf16, [1024, 2056]: two trips      test_muon_normalize
  ns_gemm_kernel                 steps = 1: eight shapes x nmat 1 3 x dense / sparse; steps 2 and 3
                                                                                       test_newton_schulz_*
  muon_update_kernel             exact shapes, [328, 200], NULL shadow / EMA per matrix, device scalars with decoys,
                                 skipped                                               test_muon_update
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_census as G  # noqa: E402
import optim_census as C  # noqa: E402
import row_census as R  # noqa: E402

from video_diffusion_speedrun_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
bits = G.bits
GUARD = 64      # elements of a guard band: a multiple of 16 bytes for every dtype used here


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib(ops):
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """a flat tensor between two guard bands on the device, its payload `off` elements past a 16-byte boundary"""
    def __init__(self, t, fill, off=0):
        self.initial, self.n, self.off = t.contiguous(), t.numel(), off
        self.before = G.fill_value(t.dtype, fill).repeat(2 * GUARD + off + self.n + 8)
        self.before[GUARD + off:GUARD + off + self.n] = self.initial.flatten()
        self.dev = self.before.cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.ptr = self.dev.data_ptr() + (GUARD + off) * t.element_size()

    def at(self, elem):
        return self.ptr + elem * self.initial.element_size()

    def got(self):
        return self.dev.cpu()[GUARD + self.off:GUARD + self.off + self.n].view(self.initial.shape)

    def check(self, want, what, compare=True):
        after = self.dev.cpu()
        lo, hi = GUARD + self.off, GUARD + self.off + self.n
        assert torch.equal(bits(after[:lo]), bits(self.before[:lo])) and torch.equal(bits(after[hi:]), bits(self.before[hi:])), \
            f"{what}: a guard band changed"
        got = after[lo:hi].view(self.initial.shape)
        if compare:
            diff = bits(got) != bits(want.contiguous().view(self.initial.shape))
            if diff.any():
                idx = tuple(int(v) for v in diff.nonzero()[0])
                raise AssertionError(f"{what}: {int(diff.sum())} of {self.n} elements differ, first at {idx}: got "
                                     f"{got[idx].item()!r} want {want.view(self.initial.shape)[idx].item()!r}")
        return got

    def untouched(self, what):
        self.check(self.initial, what + " (must keep every bit)")


def blank(dtype, n, off=0):
    return Buf(G.fill_value(dtype, "sentinel").repeat(n), "sentinel", off)


def dev_bytes(cstruct_array):
    return torch.frombuffer(bytearray(bytes(cstruct_array)), dtype=torch.uint8).cuda()


def guard_record(coef=1.0, skipped=0):
    rec = torch.zeros(4, dtype=torch.int32)
    rec.view(f32)[1] = coef
    rec[2] = skipped
    return rec.cuda()


# ==== AdamW ===========================================================================================================
class AdamTensors:
    def __init__(self, case, expect):
        self.bufs = []
        for t, e in zip(case.tensors, expect):
            o = t.off
            self.bufs.append(dict(p=Buf(e.p0, "sentinel", o.get("p", 0)), g=Buf(e.g, "nan", o.get("g", 0)),
                                  m=Buf(e.m0, "sentinel", o.get("m", 0)), v=Buf(e.v0, "sentinel", o.get("v", 0)),
                                  pb=blank(bf16, t.numel, o.get("pb", 0)), ema=Buf(e.ema0, "sentinel", o.get("ema", 0))))
        descs = (_lib.AdamWTensor * len(case.tensors))()
        for d, t, b in zip(descs, case.tensors, self.bufs):
            d.p, d.g, d.m, d.v = b["p"].ptr, b["g"].ptr, b["m"].ptr, b["v"].ptr
            d.p_bf16 = b["pb"].ptr if t.shadow else None
            d.numel, d.lr, d.wd = t.numel, t.lr, t.wd
        self.desc = dev_bytes(descs)
        self.ema_tab = torch.tensor([b["ema"].ptr if t.ema else 0 for t, b in zip(case.tensors, self.bufs)], dtype=torch.int64).cuda()


def launch_adamw(lib, case, T, betas, eps, step, scalars, d):
    """scalars = (bc1, 1 / sqrt(bc2)) for the _dev forms"""
    ct, cs = C.chunk_table(case)
    ctd = torch.tensor(ct or [0], dtype=torch.int32).cuda()
    csd = torch.tensor(cs or [0], dtype=torch.int64).cuda()
    lr_mult, grad_scale, _ = case.setting
    rec = guard_record(case.coef, case.skipped)
    sc = torch.tensor([scalars[0], scalars[1], lr_mult, d], dtype=f32).cuda()
    tab = T.ema_tab.data_ptr() if case.table_ema else None
    head = (T.desc.data_ptr(), ctd.data_ptr(), csd.data_ptr(), len(ct), case.chunk_elems, betas[0], betas[1], eps)
    if case.form == "multi":
        rc = lib.vds_adamw_multi(*head, step, lr_mult, grad_scale, stream())
    elif case.form == "multi_dev":
        rc = lib.vds_adamw_multi_dev(*head, sc.data_ptr(), grad_scale, stream())
    elif case.form == "guarded":
        rc = lib.vds_adamw_guarded_multi(*head, step, lr_mult, grad_scale, rec.data_ptr(), tab, d, stream())
    else:
        rc = lib.vds_adamw_guarded_multi_dev(*head, sc.data_ptr(), grad_scale, rec.data_ptr(), tab, stream())
    torch.cuda.synchronize()
    assert rc == 0, (case.name, rc)
    return bool(ct) and not case.skipped


def test_adamw_exact(lib):
    """one right answer per element of p, m, v, the shadow and the EMA, for every launch of C.adamw_cases()"""
    for case in C.adamw_cases():
        expect = [C.adamw_expect(case, i) for i in range(len(case.tensors))]
        T = AdamTensors(case, expect)
        applied = launch_adamw(lib, case, T, (C.BETA1, C.BETA2), C.EPS_X, 1, (0.5, 2.0), case.setting[2])
        for i, (t, e, b) in enumerate(zip(case.tensors, expect, T.bufs)):
            what = f"adamw {case.name} tensor {i} ({t.numel} elements, chunk_elems {case.chunk_elems})"
            b["g"].untouched(what + " g")
            if not applied:
                for k in ("p", "m", "v", "pb", "ema"):
                    b[k].untouched(f"{what} {k}")
                continue
            b["p"].check(e.p, what + " p")
            b["m"].check(e.m, what + " m")
            b["v"].check(e.v, what + " v")
            if t.shadow:
                b["pb"].check(e.pb, what + " shadow")
            else:
                b["pb"].untouched(what + " shadow of a NULL p_bf16")
            if C.has_ema(case, t):
                b["ema"].check(e.ema, what + " ema")
            else:
                b["ema"].untouched(what + " ema that was not passed")


def ulps_of(got, want64, scale64):
    """worst |got - want| in fp32 ulps of `scale`, the sum of the magnitudes of the element's addends"""
    s32 = scale64.to(f32)
    ulp = (torch.nextafter(s32, torch.full_like(s32, float("inf"))) - s32).to(f64)
    return float(((got.to(f64) - want64).abs() / ulp).max())


@pytest.mark.parametrize("step", C.REAL_STEPS)
def test_adamw_real_constants(lib, parity_log, step):
    """betas (0.95, 0.99), eps 1e-8, Gaussian data: |got - want| <= c 2^-24 sum|addends| per element and output (c derived in
    the helper), the shadow is bf16 of the GPU's own p bit for bit"""
    worst = dict(p=0.0, m=0.0, v=0.0, ema=0.0)
    lr_mult, grad_scale, d = 0.7, 1.0, 0.99
    for form, ce, coef, offs in (("multi", 65536, 1.0, {}), ("guarded", 2048, 0.5, {}), ("guarded", 1030, 1.0, {"g": 1}),
                                 ("guarded_dev", 65536, 0.5, {}), ("multi_dev", 1028, 1.0, {})):
        ts = [C.Tensor(n, 1e-3 * (i + 1), 0.1 / (i + 1), True, True, dict(offs) if i == 0 else {}) for i, n in enumerate(C.REAL_NUMELS)]
        case = C.Case(f"real/{form}/{ce}", ts, ce, "forward", form, (lr_mult, grad_scale, d), coef, 0, True)
        real = [C.adamw_real(t.numel, step, t.lr, t.wd, lr_mult, grad_scale, coef if "guarded" in form else 1.0, d, i)
                for i, t in enumerate(ts)]
        T = AdamTensors(case, real)
        assert launch_adamw(lib, case, T, C.REAL_BETAS, C.REAL_EPS, step, C.host_scalars(*C.REAL_BETAS, step), d)
        for i, (t, r, b) in enumerate(zip(ts, real, T.bufs)):
            what = f"adamw {case.name} step {step} tensor {i}"
            b["g"].untouched(what + " g")
            outs = [("p", r.p, r.bp, r.sp), ("m", r.m, r.bm, r.sm), ("v", r.v, r.bv, r.sv)]
            if "guarded" in form:
                outs.append(("ema", r.ema, r.bema, r.sema))
            else:
                b["ema"].untouched(what + " ema")
            for k, want, bound, scale in outs:
                got = b[k].check(None, f"{what} {k}", compare=False)
                u = ulps_of(got, want, scale)
                print(f"{what} {k}: worst {u:.3f} fp32 ulps of the addends' magnitudes")
                worst[k] = max(worst[k], u)
                bad = (got.to(f64) - want).abs() > bound
                if bad.any():
                    j = int(bad.nonzero()[0])
                    raise AssertionError(f"{what} {k}: {int(bad.sum())} of {t.numel} elements outside the bound, first at {j}: got "
                                         f"{got[j].item()!r} want {want[j].item()!r} bound {bound[j].item():.3e}")
            b["pb"].check(b["p"].got().to(bf16), what + " shadow = bf16(p)")
    parity_log("test_optim_census_gpu.adamw_real", step=step, worst_ulps=worst,
               bound_ulps=dict(p=C.C_P / 2, m=C.C_M / 2, v=C.C_V / 2, ema=C.C_EMA / 2))


# ==== sum of squares and finalize =====================================================================================
def sumsq_tables(numels, gbufs):
    descs = (_lib.AdamWTensor * len(numels))()
    for d, n, b in zip(descs, numels, gbufs):
        d.g, d.numel = b.ptr, n
    return dev_bytes(descs)


def read_guard(rec):
    r = rec.cpu()
    return float(r.view(f32)[0]), float(r.view(f32)[1]), int(r[2]), int(r[3])


def test_sumsq(lib):
    """every partial and the total equal float64 bit for bit; the workspace past n_chunks floats and g keep every bit"""
    for case in C.sumsq_cases():
        gs, ct, cs, parts, total = C.sumsq_expect(case.name)
        gb = [Buf(g, "nan", o) for g, o in zip(gs, case.offs)]
        desc = sumsq_tables(case.numels, gb)
        ctd, csd = torch.tensor(ct, dtype=torch.int32).cuda(), torch.tensor(cs, dtype=torch.int64).cuda()
        assert lib.vds_grad_sumsq_workspace_floats(len(ct)) == len(ct)
        ws, out = blank(f32, len(ct)), blank(f32, 1)
        rec = guard_record(7.0, 1)
        rc = lib.vds_grad_sumsq_multi(desc.data_ptr(), ctd.data_ptr(), csd.data_ptr(), len(ct), case.chunk_elems, ws.ptr, out.ptr,
                                      1.0, 1, rec.data_ptr(), stream())
        torch.cuda.synchronize()
        what = f"sumsq {case.name} ({len(ct)} chunks of {case.chunk_elems})"
        assert rc == 0, (what, rc)
        ws.check(parts, what + " partial of chunk")
        out.check(total, what + " total")
        for i, b in enumerate(gb):
            b.untouched(f"{what} g of tensor {i}")
        norm, coef, skipped, n_skipped = read_guard(rec)
        want = C.finalize_expect(float(total), 1.0, 1.0, 1)
        assert C.same_f32(norm, want[0]) and C.same_f32(coef, want[1]) and (skipped, n_skipped) == (0, 0), (what, norm, coef, skipped)
    # n_chunks = 0: the sum is 0, the coefficient 1, nothing skipped
    g = Buf(torch.ones(8, dtype=f32), "nan")
    desc = sumsq_tables([8], [g])
    idx = torch.zeros(1, dtype=torch.int64).cuda()
    ws, out, rec = blank(f32, 1), blank(f32, 1), guard_record(7.0, 1)
    rc = lib.vds_grad_sumsq_multi(desc.data_ptr(), idx.data_ptr(), idx.data_ptr(), 0, 2048, ws.ptr, out.ptr, 1.0, 1, rec.data_ptr(),
                                  stream())
    torch.cuda.synchronize()
    assert rc == 0
    out.check(torch.zeros(1, dtype=f32), "sumsq of no chunks")
    ws.untouched("workspace of no chunks")
    assert read_guard(rec) == (0.0, 1.0, 0, 0)


def test_finalize(lib):
    """guard_finalize against its fp32 restatement through both entries; n_skipped accumulates over the calls"""
    rec = guard_record(0.0, 0)
    src = torch.zeros(1, dtype=f32).cuda()
    count = 0
    for sumsq, scale, max_norm, skip in C.finalize_table():
        src.fill_(sumsq)
        rc = lib.vds_optim_guard_finalize(src.data_ptr(), scale, max_norm, skip, rec.data_ptr(), stream())
        assert rc == 0
        got = read_guard(rec)
        want = C.finalize_expect(sumsq, scale, max_norm, skip)
        count += want[2]
        what = f"finalize sumsq {sumsq!r} scale {scale} max_norm {max_norm!r} skip_nonfinite {skip}"
        assert C.same_f32(got[0], want[0]), f"{what}: norm {got[0]!r} want {want[0]!r}"
        assert C.same_f32(got[1], want[1]), f"{what}: coef {got[1]!r} want {want[1]!r}"
        assert got[2:] == (want[2], count), f"{what}: (skipped, n_skipped) {got[2:]} want {(want[2], count)}"
    assert count > 0
    # the fused second stage: one gradient element g, sumsq = fl(g g)
    rec = guard_record(0.0, 0)
    count = 0
    g = Buf(torch.ones(1, dtype=f32), "nan")
    desc = sumsq_tables([1], [g])
    idx = torch.zeros(1, dtype=torch.int64).cuda()
    idx32 = torch.zeros(1, dtype=torch.int32).cuda()
    ws, out = blank(f32, 1), blank(f32, 1)
    for gv in (0.0, 2.0 ** -63, 1.0, 4.0, 1e5, 1.7e19, float("inf"), float("nan")):
        g.dev[GUARD] = gv
        sumsq = float(torch.tensor(gv, dtype=f32) * torch.tensor(gv, dtype=f32))
        for max_norm in C.FIN_MAXNORM:
            for skip in C.FIN_SKIP:
                rc = lib.vds_grad_sumsq_multi(desc.data_ptr(), idx32.data_ptr(), idx.data_ptr(), 1, 4, ws.ptr, out.ptr, max_norm, skip,
                                              rec.data_ptr(), stream())
                assert rc == 0
                got, got_sumsq = read_guard(rec), float(out.got()[0])
                want = C.finalize_expect(sumsq, 1.0, max_norm, skip)
                count += want[2]
                what = f"fused finalize g {gv!r} max_norm {max_norm!r} skip_nonfinite {skip}"
                assert C.same_f32(got_sumsq, sumsq), f"{what}: sumsq {got_sumsq!r} want {sumsq!r}"
                assert C.same_f32(got[0], want[0]) and C.same_f32(got[1], want[1]), f"{what}: (norm, coef) {got[:2]} want {want[:2]}"
                assert got[2:] == (want[2], count), f"{what}: (skipped, n_skipped) {got[2:]} want {(want[2], count)}"


# ==== Muon ============================================================================================================
WS_GUARD = 256     # bytes


class Workspace:
    """a Muon workspace between two guard bands, all ones bits wherever the test writes nothing"""
    def __init__(self, lib, nmat, rows, cols):
        self.layout, self.total = C.muon_layout(nmat, rows, cols)
        assert lib.vds_muon_workspace_bytes(nmat, rows, cols) == self.total
        off = (ctypes.c_int64 * 6)()
        assert lib.vds_muon_workspace_layout(nmat, rows, cols, ctypes.addressof(off)) == 0
        assert list(off) == [self.layout[k][0] for k in ("x0", "x1", "a", "b", "sumsq", "partials")], "the restated layout"
        self.m, self.n, self.nmat = min(rows, cols), max(rows, cols), nmat
        self.host = torch.full((self.total + 2 * WS_GUARD,), 0xFF, dtype=torch.uint8)
        self.dev = None

    def _slice(self, t, name):
        o, nbytes = self.layout[name]
        return t[WS_GUARD + o:WS_GUARD + o + nbytes]

    def write(self, name, t):
        raw = t.contiguous().view(torch.uint8).flatten()
        assert raw.numel() == self.layout[name][1]
        self._slice(self.host, name).copy_(raw)

    def upload(self):
        self.dev = self.host.cuda()
        assert self.dev.data_ptr() % 16 == 0
        return self.dev.data_ptr() + WS_GUARD

    def read(self, name):
        raw = self._slice(self.dev.cpu(), name)
        shape = {"x0": (self.nmat, self.m, self.n), "x1": (self.nmat, self.m, self.n), "a": (self.nmat, self.m, self.m),
                 "b": (self.nmat, self.m, self.m), "sumsq": (self.nmat,), "partials": (self.nmat, -1)}[name]
        return raw.view(f32 if name in ("sumsq", "partials") else bf16).view(shape)

    def rest_intact(self, written, what):
        """every byte outside the payloads of the sections in `written`: the guard bands, the padding, the other sections"""
        after, keep = self.dev.cpu(), torch.ones(self.host.numel(), dtype=torch.bool)
        for name in written:
            self._slice(keep, name).fill_(False)
        bad = (after != self.host) & keep
        assert not bad.any(), f"{what}: byte {int(bad.nonzero()[0]) - WS_GUARD} of the workspace changed outside {written}"


def same(what, got, want):
    diff = bits(got) != bits(want.contiguous())
    if diff.any():
        idx = tuple(int(v) for v in diff.nonzero()[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.numel()} elements differ, first at {idx}: got {got[idx].item()!r} "
                             f"want {want[idx].item()!r}")


def muon_table(ops, nmat, per, p, g, buf, pb=None, ema=None, no_pb=(), no_ema=()):
    return ops.muon_table([(p.at(k * per), g.at(k * per), buf.at(k * per),
                            None if pb is None or k in no_pb else pb.at(k * per),
                            None if ema is None or k in no_ema else ema.at(k * per)) for k in range(nmat)], "cuda")


def test_muon_momentum(ops, lib):
    """buf, x0 = bf16(u) (transposed for the tall shapes), the partials and the per-matrix sum of squares, bit for bit"""
    for nmat, rows, cols, mu, coef, nesterov in C.mom_plan():
        c = C.momentum_case(nmat, rows, cols, mu, coef, nesterov)
        what = f"momentum {nmat} x [{rows}, {cols}] mu {mu} coef {coef} nesterov {nesterov}"
        p, g, buf = blank(f32, nmat * rows * cols), Buf(c.g, "nan"), Buf(c.buf0, "sentinel")
        tab = muon_table(ops, nmat, rows * cols, p, g, buf)
        ws = Workspace(lib, nmat, rows, cols)
        rec = guard_record(coef, 0)
        rc = lib.vds_muon_momentum(tab.data_ptr(), nmat, rows, cols, mu, nesterov, rec.data_ptr() if coef != 1.0 else None, ws.upload(),
                                   stream())
        torch.cuda.synchronize()
        assert rc == 0, (what, rc)
        buf.check(c.buf, what + " buf")
        g.untouched(what + " g")
        p.untouched(what + " p")
        same(what + " x0 (matrix, workspace row, col)", ws.read("x0"), c.x0)
        same(what + " partial (matrix, tile)", ws.read("partials"), c.partials)
        same(what + " sumsq of matrix", ws.read("sumsq"), c.sumsq)
        ws.rest_intact(("x0", "partials", "sumsq"), what)
    # a skipped step keeps every bit of buf and of the workspace
    c = C.momentum_case(3, 200, 72, 0.5, 0.5, 1)
    p, g, buf = blank(f32, 3 * 200 * 72), Buf(c.g, "nan"), Buf(c.buf0, "sentinel")
    tab, ws, rec = muon_table(ops, 3, 200 * 72, p, g, buf), Workspace(lib, 3, 200, 72), guard_record(0.5, 1)
    assert lib.vds_muon_momentum(tab.data_ptr(), 3, 200, 72, 0.5, 1, rec.data_ptr(), ws.upload(), stream()) == 0
    torch.cuda.synchronize()
    buf.untouched("skipped momentum buf")
    ws.rest_intact((), "skipped momentum")


def test_muon_normalize(lib):
    """steps = 0: x0 = bf16(fp32(u inv)) in place, inv restated in fp32; nothing else of the workspace changes"""
    for nmat, rows, cols in C.NORM_SHAPES:
        u, sumsq, want = C.normalize_case(nmat, rows, cols)
        ws = Workspace(lib, nmat, rows, cols)
        ws.write("x0", u)
        ws.write("sumsq", sumsq)
        rc = lib.vds_muon_orthogonalize(ws.upload(), nmat, rows, cols, 0, stream())
        torch.cuda.synchronize()
        what = f"normalize {nmat} x [{rows}, {cols}] grid {C.normalize_grid(rows * cols)}"
        assert rc == 0, (what, rc)
        same(what + " x0 (matrix, row, col)", ws.read("x0"), want)
        ws.rest_intact(("x0",), what)


def run_ns(lib, u, steps):
    nmat, m, n = u.shape
    ws = Workspace(lib, nmat, m, n)
    ws.write("x0", u)
    ws.write("sumsq", torch.full((nmat,), 16.0, dtype=f32))
    rc = lib.vds_muon_orthogonalize(ws.upload(), nmat, m, n, steps, stream())
    torch.cuda.synchronize()
    assert rc == 0
    return ws


def check_last_iteration(what, ws, cap_x=C.UNDECIDED_CAP):
    """a, b and x0 against the helper's expectation from the GPU's own x1, a and b -> the three excluded shares"""
    X, A, B, X1 = ws.read("x1"), ws.read("a"), ws.read("b"), ws.read("x0")
    want, ex = C.ns_expect_a(X)
    sa = C.check_product(what + " A = X X^T", A, want, ex)
    want, ex = C.ns_expect_b(A)
    sb = C.check_product(what + " B = c A A + b A", B, want, ex)
    want, ex = C.ns_expect_x(B, X)
    sx = C.check_product(what + " X' = B X + a X", X1, want, ex, cap_x)
    ws.rest_intact(("x0", "x1", "a", "b"), what)
    return sa, sb, sx


@pytest.mark.parametrize("recipe", ["dense", "sparse"])
def test_newton_schulz_one_iteration(lib, parity_log, recipe):
    """steps = 1 from x0 = u and sumsq = 16 in a workspace of NaN: x1 = u / 4, then each product from the stored operand
    of the one before.  dense: the third product is compared where its sum fits 24 bits, without a cap (the issue: it
    does not fit under this recipe)"""
    for m, n in C.NS_SHAPES:
        for nmat in C.NS_NMAT:
            u = C.ns_u(recipe, nmat, m, n)
            what = f"newton-schulz {recipe} {nmat} x [{m}, {n}] ({C.tri_tiles(m)} triangular tiles, K tails {C.k_tail(n)} / {C.k_tail(m)})"
            ws = run_ns(lib, u, 1)
            same(what + " x1 = u / 4 (matrix, row, col)", ws.read("x1"), (u.to(f64) / 4.0).to(bf16))
            sa, sb, sx = check_last_iteration(what, ws, cap_x=1.0 if recipe == "dense" else C.UNDECIDED_CAP)
            print(f"{what}: excluded A {sa:.3%} B {sb:.3%} X' {sx:.3%}")
            parity_log("test_optim_census_gpu.newton_schulz", recipe=recipe, m=m, n=n, nmat=nmat, excluded_a=sa, excluded_b=sb,
                       excluded_x=sx)


@pytest.mark.parametrize("steps", [2, 3])
def test_newton_schulz_ping_pong(lib, steps):
    """both parities of the start slot: the iterate before the last iteration (x1) equals the helper's chain run forward
    from u / 4, and the last iteration is pinned product by product from it"""
    for m, n in ((136, 136), (128, 520), (200, 328)):
        u = C.ns_u("signed_permutation", 3, m, n)
        what = f"newton-schulz steps {steps} 3 x [{m}, {n}]"
        ws = run_ns(lib, u, steps)
        same(what + f" x1 after {steps - 1} iterations (matrix, row, col)", ws.read("x1"),
             C.ns_forward((u.to(f64) / 4.0).to(bf16), steps - 1))
        check_last_iteration(what, ws)


def test_muon_update(ops, lib):
    """p, the shadow and the EMA bit for bit at the exact shapes; NULL shadow / EMA for one matrix each; device scalars
    beside decoy arguments; [328, 200]: either fp32 form of p per element, shadow and EMA from the GPU's own p; skipped"""
    runs = [(nmat, r, c, C.UPD_SCALARS[i % 2], i % 2 == 1, 0) for i, (r, c) in enumerate(C.UPD_EXACT + (C.UPD_INEXACT,)) for nmat in (1, 3)]
    runs.append((3, 512, 128, C.UPD_SCALARS[0], True, 1))
    for nmat, rows, cols, scalars, from_device, skipped in runs:
        lr, wd, lr_mult, d = scalars
        e = C.update_case(nmat, rows, cols, scalars)
        what = f"update {nmat} x [{rows}, {cols}] scale {e.scale} device scalars {from_device} skipped {skipped}"
        per = rows * cols
        p, pb, ema = Buf(e.p0, "sentinel"), blank(bf16, nmat * per), Buf(e.ema0, "sentinel")
        g, buf = Buf(torch.ones(nmat * per, dtype=f32), "nan"), Buf(torch.ones(nmat * per, dtype=f32), "nan")
        no_pb, no_ema = ((1,), (2,)) if nmat == 3 else ((), ())
        tab = muon_table(ops, nmat, per, p, g, buf, pb, ema, no_pb, no_ema)
        ws = Workspace(lib, nmat, rows, cols)
        ws.write("x0", e.o.transpose(1, 2) if rows > cols else e.o)
        sc = torch.tensor([-3.0, -5.0, lr_mult, d], dtype=f32).cuda()
        rec = guard_record(0.25, skipped)
        args = (123.0, 0.3, sc.data_ptr()) if from_device else (lr_mult, d, None)     # decoys beside the device scalars
        rc = lib.vds_muon_update(tab.data_ptr(), nmat, rows, cols, lr, wd, args[0], args[1], args[2], rec.data_ptr(), ws.upload(),
                                 stream())
        torch.cuda.synchronize()
        assert rc == 0, (what, rc)
        ws.rest_intact((), what)
        g.untouched(what + " g")
        buf.untouched(what + " buf")
        if skipped:
            for b, k in ((p, "p"), (pb, "shadow"), (ema, "ema")):
                b.untouched(f"{what} {k}")
            continue
        if e.scale in (1.0, 2.0):
            got_p = p.check(e.p, what + " p (matrix, row, col)")
        else:
            got_p = p.check(None, what + " p", compare=False)
            ok = (bits(got_p) == bits(e.p)) | (bits(got_p) == bits(e.p_alt))
            assert ok.all(), (f"{what}: p at (matrix, row, col) {tuple(int(v) for v in (~ok).nonzero()[0])} is neither the contracted "
                              f"nor the uncontracted fp32 result")
        want_pb, want_ema = got_p.to(bf16), C.ema_from(e.ema0, got_p, d, exact=False)
        for k in no_pb:
            want_pb[k] = G.fill_value(bf16, "sentinel")
        for k in no_ema:
            want_ema[k] = e.ema0[k]
        pb.check(want_pb, what + " shadow (matrix, row, col)")
        ema.check(want_ema, what + " ema (matrix, row, col)")
