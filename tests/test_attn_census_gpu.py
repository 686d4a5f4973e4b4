"""Exact mask census of every masked attention kernel instance (tests/helpers/attn_census.py): inputs whose right answer is a
count -- lse = ln N(q), o N = the attended keys per label, probe gradients that are nonzero exactly on the attended pairs --
so one wrong (query, key) pair anywhere fails.  Bounds (0.25, 2^-7, 2^-6) are derived in the helper; every output starts as
NaN.  The cases and their conditions are checked without a GPU in tests/test_attn_census_cpu.py.

Shapes.  Frame-causal (L, lead, period): (280, 16, 8), (140, 5, 3), (203, 0, 7), (159, 16, 13), (230, 32, 33), (293, 33, 65),
(193, 64, 1) -- periods above 32 and 64 leave frames out of a sub-block, leads 32 / 64 sit on wave / tile starts, 33 one past
(159 and 293 are the lengths next to 157 and 290 that the entry points accept: (L - lead) % period == 0).  With a past: lead
16 with past 14 .. 17, 46 .. 49, 112 (lead + past = 30 .. 33, 62 .. 65, 128), lead 32 with 32 / 33, lead 5 with 27, lead 0
with 64; periods 2 and 7, Lq = lead + 140.  Key lengths {0, 1, 15, 16, 17, 63, 64, 65, 128, Lk - 1, Lk, Lk + 5} over two
launches of B = 6, Lk = 200, cross (Lq = 130) and self (Lq = 200) layout.

Instance -> case (run_fwd / run_bwd in csrc/attention.hip; every CAUSAL, PAST and KVLEN instance set_lds lists):

  attn_fwd_kernel<HDP, HDQ, 2, true, ..>  x 5 head dims
      CAUSAL  test_causal[plain_hd*]; <96, 80> on the ones layout: test_causal[ones_narrow]
      PAST    test_past[fwd_hd*], [fwd_hd72_ones]
      KVLEN   test_kvlen[plain_hd*]; <96, 80> on kv_pad_ones = 2: test_kvlen[xones_narrow]
  attn_fwd_wide_kernel<HDP, HDQ, false, ..>  HDP 64, 96 / 80, 96 / 96 (knob attn_fwd_wide = 1; the rule is Lq >= 2048)
      CAUSAL  test_causal[wide_hd64 / 72 / 96]     PAST  test_past[wide_hd64 / 72 / 96]     KVLEN  test_kvlen[wide_hd64 / 72 / 96]
      <32, 32, false, ..>: listed by set_lds, launched by nothing (use_wide exists for HDP 64 and 96 only)
  attn_fwd_wide_kernel<96, 80, true, ..>  (ones columns, knob, variant bit 4 off)
      CAUSAL  test_causal[ones_mfma32]     PAST  test_past[wide_ones_mask0 / 3]     KVLEN  test_kvlen[xones_mfma32]
  attn_fwd16_kernel<96, ..>  (ones columns, knob, variant bit 4 on)
      CAUSAL  test_causal[ones_default / all16_*]     PAST  test_past[fwd16_*]     KVLEN  test_kvlen[xones_default / ...]
  attn_bwd_dq_kernel<HDP, HDQ, false, ..>  x 5     CAUSAL  test_causal[plain_hd*]     KVLEN  test_kvlen[plain_hd*]
  attn_bwd_dq_kernel<96, 80, true, ..>             CAUSAL  test_causal[ones_mfma32]   KVLEN  test_kvlen[xones_mfma32]
  attn_bwd_dq16_kernel<96, false, ..>              CAUSAL  [ones_all16_separate_delta]  KVLEN  [xones_separate_delta]
  attn_bwd_dq16_kernel<96, true, ..>               CAUSAL  [ones_default / all16_folded_delta]  KVLEN  [xones_default]
  attn_bwd_dkv_kernel<HDP, HDQ, false, ..>  x 5    CAUSAL  test_causal[plain_hd*], query-split: [qsplit_hd64] (L = 1040)
                                                   KVLEN   test_kvlen[plain_hd*], [xones_*]; query-split + dkv_reduce_kernel
                                                           <true>: [qsplit_hd72] (knob attn_qsplit = 2)
  attn_bwd_dkv_kernel<96, 80, true, false, CAUSAL>     test_causal[ones_mfma32]
  attn_bwd_dkv16_kernel<96, true, false, CAUSAL>       test_causal[ones_default / all16_*]
  attn_bwd_dkv16_kernel<96, false, KVLEN>              test_kvlen[xones_dkv16] (knob cross_dkv16 = 2)

Nothing here needs L >= 2048: the knob reaches the same instances at L <= 293."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_census as AC  # noqa: E402
from test_attn_census_cpu import CAUSAL, HEAD_DIMS, KV_LENS, KV_LK, KV_LQ, PAST, PAST_PERIODS  # noqa: E402

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import ops as _ops
    return _ops


class knobs:
    """attn_fwd_wide / attn_delta_fold / cross_dkv16 / attn_qsplit and the variant mask for the length of a call"""

    def __init__(self, ops, variant=None, **kn):
        self.ops, self.variant, self.kn = ops, variant, {k: v for k, v in kn.items() if v is not None}

    def __enter__(self):
        self.prev_v = self.ops.attn_set_variant(self.variant) if self.variant is not None else None
        self.prev = {k: self.ops.knob_set(k, v) for k, v in self.kn.items()}

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            self.ops.knob_set(k, v)
        if self.prev_v is not None:
            self.ops.attn_set_variant(self.prev_v)


def tok(t):
    """[B, H, L, hd] -> token-major rows [B * L, H * hd]"""
    B, H, L, hd = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * L, H * hd)


def heads(t2d, B, L, H, hd, off=0):
    """[B*L, ld] token-major rows -> [B,H,L,hd] (CPU copy of what ops.heads_view addresses)"""
    return t2d[:, off:off + H * hd].reshape(B, L, H, hd).permute(0, 2, 1, 3)


_cache = {}


def cached(key, make):
    """census inputs and expectations, built once per case, shared and never modified"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ------------------------------------------------------------------ frame-causal ----
def run_causal(ops, q, k, v, do, frames, ones=False, legacy_ws=False, variant=None, wide=None, fold=None):
    """the launch plumbing of tests/test_attn_causal_gpu.py on census inputs [B, H, L, hd]: token-major qkv / dO / outputs
    through ops.heads_view, or (ones) the padded head-major rows ops.qkv_rope_fwd writes under an identity rotation"""
    B, H, L, hd = q.shape
    D = H * hd
    qkvd = torch.cat([tok(q), tok(k), tok(v)], dim=1).cuda()
    o = torch.full((B * L, D), NAN, dtype=bf16, device="cuda")
    lse = torch.full((B, H, L), NAN, dtype=f32, device="cuda")
    ov = ops.heads_view(o, B, L, H, hd)
    if ones:
        hdp = 96
        cos = torch.ones(L, hd // 2, dtype=f32, device="cuda")
        sin = torch.zeros(L, hd // 2, dtype=f32, device="cuda")
        qp, kp, vp = ops.qkv_rope_fwd(qkvd, cos, sin, None, None, B, L, H, hd, hdp)
        qv, kk, vv = qp[..., :hd], kp[..., :hd], vp[..., :hd]
        dqb, dkb, dvb = (torch.full((B, H, L, hdp), NAN, dtype=bf16, device="cuda") for _ in range(3))
        dqv, dkv, dvv = dqb[..., :hd], dkb[..., :hd], dvb[..., :hd]
    else:
        qv, kk, vv = (ops.heads_view(qkvd, B, L, H, hd, i * D) for i in range(3))
        dqkv = torch.full_like(qkvd, NAN)
        dqv, dkv, dvv = (ops.heads_view(dqkv, B, L, H, hd, i * D) for i in range(3))
    with knobs(ops, variant, attn_fwd_wide=wide, attn_delta_fold=fold):
        ops.attn_fwd(qv, kk, vv, ov, lse, kv_pad_ones=ones, frames=frames)
        if do is not None:
            n = 2 * B * H * L if legacy_ws else ops.attn_bwd_workspace_floats(B, H, L, L, hd, ones)
            delta = torch.full((n,), NAN, dtype=f32, device="cuda")
            dod = tok(do).cuda()
            ops.attn_bwd(qv, kk, vv, ov, lse, ops.heads_view(dod, B, L, H, hd), dqv, dkv, dvv, delta, kv_pad_ones=ones,
                         frames=frames)
    torch.cuda.synchronize()
    out = [heads(o.cpu(), B, L, H, hd), lse.cpu()]
    if do is not None:
        out += [t.cpu() for t in (dqv, dkv, dvv)]
    return out


def census(tag, run, hd, B, H, mask, lead=None, period=None, bwd=True):
    """forward count and labels, then the dK / dV and the dQ probes, on run(q, k, v, do) -> o, lse[, dq, dk, dv]"""
    _, Lq, Lk = mask.shape
    key = (hd, B, H, Lq, Lk, lead, period)
    q, k, v = cached(("fwd",) + key, lambda: AC.forward_inputs(hd, B, H, Lq, Lk))
    o, lse = run(q, k, v, None)[:2]
    worst = {"count": AC.check_count(tag, lse, mask), "labels": AC.check_labels(tag, o, mask)}
    if bwd:
        w = AC.signs(B, H, Lk, lead, period)
        pq, pk = AC.probe_rows(B, H, hd, Lq, lead, period), AC.probe_rows(B, H, hd, Lk, lead, period)
        q, k, v, do = cached(("dkv",) + key, lambda: AC.dkv_probe_inputs(hd, B, H, Lq, Lk, pq, w))
        o, lse, dq, dk, dv = run(q, k, v, do)
        edv, edk, gap = AC.expect_dkv(mask, pq, w, hd)
        assert gap >= AC.MIN_GAP
        worst["count"] = max(worst["count"], AC.check_count(tag + ".dkv", lse, mask))
        worst["dv"] = AC.check_support_and_values(tag + ".dv", dv, edv, AC.REL_DV)
        worst["dk"] = AC.check_support_and_values(tag + ".dk", dk, edk, AC.REL_DK)
        AC.check_zero(tag + ".dkv.dq", dq)
        q, k, v, do = cached(("dq",) + key, lambda: AC.dq_probe_inputs(hd, B, H, Lq, Lk, pk, w))
        o, lse, dq, dk, dv = run(q, k, v, do)
        edq, gap = AC.expect_dq(mask, pk, w, hd)
        assert gap >= AC.MIN_GAP
        worst["count"] = max(worst["count"], AC.check_count(tag + ".dq", lse, mask))
        worst["dq"] = AC.check_support_and_values(tag + ".dq", dq, edq, AC.REL_DK)
        AC.check_zero(tag + ".dq.dk", dk)
    print(f"census {tag}: " + " ".join(f"{n} {e:.3e}" for n, e in worst.items()))


# family -> (head dim, B, H, backward?, run_causal keywords).  B * H = 10 crosses the 8-head grouping of the workgroup order;
# the ones layout runs the variant masks and attn_delta_fold settings of test_ones_column_kernels at B = H = 2, under the
# attn_fwd_wide knob (the 64-queries-per-wave forward kernels at L < 2048); ones_narrow is attn_fwd_kernel<96, 80> on it
CAUSAL_FAMILIES = {f"plain_hd{hd}": (hd, 5, 2, True, {}) for hd in HEAD_DIMS}
CAUSAL_FAMILIES.update({f"wide_hd{hd}": (hd, 5, 2, False, dict(wide=1)) for hd in (64, 72, 96)})
CAUSAL_FAMILIES.update({
    "ones_default": (72, 2, 2, True, dict(ones=True, wide=1)),
    "ones_mfma32": (72, 2, 2, True, dict(ones=True, wide=1, variant=0)),
    "ones_all16_separate_delta": (72, 2, 2, True, dict(ones=True, wide=1, variant=7, fold=0)),
    "ones_all16_folded_delta": (72, 2, 2, True, dict(ones=True, wide=1, variant=7, fold=1)),
    "ones_narrow": (72, 2, 2, False, dict(ones=True, wide=0)),
})


@pytest.mark.parametrize("case", CAUSAL, ids=lambda c: "L%d_%d_%d" % c)
@pytest.mark.parametrize("family", list(CAUSAL_FAMILIES))
def test_causal(ops, family, case):
    hd, B, H, bwd, kw = CAUSAL_FAMILIES[family]
    L, lead, period = case
    run = lambda q, k, v, do: run_causal(ops, q, k, v, do, (lead, period), **kw)
    census(f"causal.{family}.L{L}_{lead}_{period}", run, hd, B, H, AC.causal_mask(B, L, lead, period), lead, period, bwd)


def test_causal_query_split_dkv(ops):
    """B = 1, H = 2, L = 1024 + 16 at head dim 64: the plain dK/dV launch splits the query range (fp32 partials +
    dkv_reduce_kernel); 128 of the 1040 rows are probes, the tile, wave and lead edges first"""
    hd, B, H, L, lead, period = 64, 1, 2, 1040, 16, 8
    assert ops.attn_bwd_workspace_floats(B, H, L, L, hd) > 2 * B * H * L
    run = lambda q, k, v, do: run_causal(ops, q, k, v, do, (lead, period))
    census("causal.qsplit_hd64.L1040_16_8", run, hd, B, H, AC.causal_mask(B, L, lead, period), lead, period)


# ------------------------------------------------------------- frame-causal, past ----
def padded(t, which):
    """[B,H,L,72] -> the padded rows [B,H,L,96] the qkv / RoPE kernel writes: zeros, K[72] = K[73] = 1, V[72] = V[76] = 1"""
    p = torch.zeros(*t.shape[:3], 96, dtype=bf16)
    p[..., :72] = t
    if which == "k":
        p[..., 72:74] = 1
    if which == "v":
        p[..., 72] = 1
        p[..., 76] = 1
    return p


def run_past(ops, q, k, v, lead, period, past, ones=False, wide=False, variant=None, entry=False):
    """the launch plumbing of tests/test_attn_past_gpu.py: contiguous head-major q / k / v (ones: the padded rows), o
    token-major; entry: through vds_attn_fwd_causal_past itself"""
    B, H, Lq, hd = q.shape
    if ones:
        qd, kd, vd = (padded(t, n).cuda()[..., :hd] for t, n in ((q, "q"), (k, "k"), (v, "v")))
    else:
        qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    o = torch.full((B * Lq, H * hd), NAN, dtype=bf16, device="cuda")
    lse = torch.full((B, H, Lq), NAN, dtype=f32, device="cuda")
    ov = ops.heads_view(o, B, Lq, H, hd)
    with knobs(ops, variant, attn_fwd_wide=1 if wide else None):
        if entry:
            from video_diffusion_speedrun_amd import _lib
            a = _lib.AttnArgs()
            a.B, a.H, a.Lq, a.Lk, a.head_dim = B, H, Lq, kd.shape[2], hd
            for name, t in (("q", qd), ("k", kd), ("v", vd), ("o", ov)):
                setattr(a, name, t.data_ptr())
                for s, val in zip(("sb", "sh", "sl"), t.stride()[:3]):
                    setattr(a, f"{name}_{s}", val)
            a.lse = lse.data_ptr()
            a.kv_pad_ones = int(ones)
            rc = _lib.load().vds_attn_fwd_causal_past(C.byref(a), C.byref(_lib.ModGroups(lead, period)), past,
                                                      torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc
        else:
            ops.attn_fwd(qd, kd, vd, ov, lse, kv_pad_ones=ones, frames=(lead, period), past=past)
    torch.cuda.synchronize()
    return heads(o.cpu(), B, Lq, H, hd), lse.cpu()


# the 14 families of tests/test_attn_past_gpu.py
PAST_FAMILIES = {
    "fwd_hd32": (32, {}), "fwd_hd64": (64, {}), "fwd_hd72": (72, {}), "fwd_hd96": (96, {}), "fwd_hd128": (128, {}),
    "fwd_hd72_ones": (72, dict(ones=True)),
    "wide_hd64": (64, dict(wide=True)), "wide_hd72": (72, dict(wide=True)), "wide_hd96": (96, dict(wide=True)),
    "wide_ones_mask0": (72, dict(ones=True, wide=True, variant=0)),
    "wide_ones_mask3": (72, dict(ones=True, wide=True, variant=3)),
    "fwd16_mask4": (72, dict(ones=True, wide=True, variant=4)),
    "fwd16_mask7": (72, dict(ones=True, wide=True, variant=7)),
    "fwd16_default": (72, dict(ones=True, wide=True)),
}


@pytest.mark.parametrize("case", PAST, ids=lambda c: "lead%d_past%d" % c)
@pytest.mark.parametrize("family", list(PAST_FAMILIES))
def test_past(ops, family, case):
    """the label census over the Lk = Lq + past keys, periods 2 and 7; for one family the C entry point gives the same bits"""
    hd, kw = PAST_FAMILIES[family]
    lead, past = case
    B = H = 2
    for period, n in PAST_PERIODS.items():
        Lq = lead + n * period
        run = lambda q, k, v, do, **e: run_past(ops, q, k, v, lead, period, past, **kw, **e)
        tag = f"past.{family}.lead{lead}_past{past}_p{period}"
        census(tag, run, hd, B, H, AC.past_mask(B, Lq, lead, period, past), lead, period, bwd=False)
        if family == "fwd_hd64":
            q, k, v = _cache[("fwd", hd, B, H, Lq, Lq + past, lead, period)]
            a, b = run(q, k, v, None), run(q, k, v, None, entry=True)
            assert torch.equal(a[0].contiguous().view(torch.int16), b[0].contiguous().view(torch.int16)), tag
            assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), tag


# --------------------------------------------------------------- per-sample key lengths ----
def run_kvlen(ops, q, k, v, do, lens, pad_ones=0, variant=None, wide=None, fold=None, dkv16=None, qsplit=None):
    """the launch plumbing of tests/test_attn_kvlen_gpu.py: token-major q / o / dO and a [B*Lk, 2D] kv buffer; pad_ones = 2:
    k / v through ops.kv_pad_ones (the cross-attention on the ones-column kernels); lens = None: no key lengths, the
    unmasked instances"""
    B, H, Lq, hd = q.shape
    Lk = k.shape[2]
    D = H * hd
    qd, kvd = tok(q).cuda(), torch.cat([tok(k), tok(v)], dim=1).cuda()
    o = torch.full((B * Lq, D), NAN, dtype=bf16, device="cuda")
    lse = torch.full((B, H, Lq), NAN, dtype=f32, device="cuda")
    kvl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    qv, ov = ops.heads_view(qd, B, Lq, H, hd), ops.heads_view(o, B, Lq, H, hd)
    if pad_ones:
        kp, vp = ops.kv_pad_ones(kvd, B, Lk, H, hd, 96, 0, D)
        kk, vv = kp[..., :hd], vp[..., :hd]
    else:
        kk, vv = ops.heads_view(kvd, B, Lk, H, hd, 0), ops.heads_view(kvd, B, Lk, H, hd, D)
    with knobs(ops, variant, attn_fwd_wide=wide, attn_delta_fold=fold, cross_dkv16=dkv16, attn_qsplit=qsplit):
        ops.attn_fwd(qv, kk, vv, ov, lse, kv_pad_ones=pad_ones, kv_lens=kvl)
        out = [heads(o.cpu(), B, Lq, H, hd), lse.cpu()]
        if do is not None:
            dod = tok(do).cuda()
            dqb, dkvb = torch.full_like(qd, NAN), torch.full_like(kvd, NAN)
            delta = None
            if qsplit:  # room for the partials of a forced split (the library would not ask for one at this size)
                delta = torch.full((2 * B * H * Lq + qsplit * B * H * Lk * 2 * hd,), NAN, dtype=f32, device="cuda")
            ops.attn_bwd(qv, kk, vv, ov, lse, ops.heads_view(dod, B, Lq, H, hd), ops.heads_view(dqb, B, Lq, H, hd),
                         ops.heads_view(dkvb, B, Lk, H, hd, 0), ops.heads_view(dkvb, B, Lk, H, hd, D), delta,
                         kv_pad_ones=pad_ones, kv_lens=kvl)
            dkv = dkvb.cpu()
            out += [heads(dqb.cpu(), B, Lq, H, hd), heads(dkv, B, Lk, H, hd, 0), heads(dkv, B, Lk, H, hd, D)]
    torch.cuda.synchronize()
    return out


# family -> (head dim, backward?, run_kvlen keywords).  xones_*: kv_pad_ones = 2 at head dim 72, as
# test_ones_column_cross_path / test_ones_column_kernel_variants run it, under the attn_fwd_wide knob instead of Lq >= 2048;
# qsplit_hd72: test_query_split_dkv's kernels under the attn_qsplit knob
KVLEN_FAMILIES = {f"plain_hd{hd}": (hd, True, {}) for hd in HEAD_DIMS}
KVLEN_FAMILIES.update({f"wide_hd{hd}": (hd, False, dict(wide=1)) for hd in (64, 72, 96)})
KVLEN_FAMILIES.update({
    "xones_default": (72, True, dict(pad_ones=2, wide=1)),
    "xones_dkv16": (72, True, dict(pad_ones=2, wide=1, dkv16=2)),
    "xones_mfma32": (72, True, dict(pad_ones=2, wide=1, variant=0, fold=1)),
    "xones_separate_delta": (72, True, dict(pad_ones=2, wide=1, variant=7, fold=0)),
    "xones_narrow": (72, False, dict(pad_ones=2, wide=0)),
    "qsplit_hd72": (72, True, dict(qsplit=2)),
})


@pytest.mark.parametrize("launch", [0, 1])
@pytest.mark.parametrize("layout", ["cross", "self"])
@pytest.mark.parametrize("family", list(KVLEN_FAMILIES))
def test_kvlen(ops, family, layout, launch):
    """B = 6, H = 2 (12 heads: every row of Lq = 130 / Lk = 200 is a probe of some head from head dim 32 on)"""
    hd, bwd, kw = KVLEN_FAMILIES[family]
    lens = KV_LENS[launch]
    Lq = KV_LQ if layout == "cross" else KV_LK
    run = lambda q, k, v, do: run_kvlen(ops, q, k, v, do, lens, **kw)
    census(f"kvlen.{family}.{layout}{launch}", run, hd, len(lens), 2, AC.kvlen_mask(Lq, KV_LK, lens), bwd=bwd)
