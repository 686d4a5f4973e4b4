"""Softmax census of the attention value path (tests/helpers/softmax_census.py) on the library: EVERY element of o, lse, dq,
dk and dv against float64 attention on the same bf16 inputs, within a bound computed per element from the kernels'
arithmetic.  The inputs put the running maximum, the lazy rescale and the order of masking and maximum in charge of the
answer: the hard recipes (a set at score 0, everything else 4096 below, unshifted and shifted by about +-30 and +-120
binades, groups by q % n and by wave), the ladder (rises on both sides of LAZY_THR inside one wave), and under every mask
the hard recipe with the keys no row of the group attends 4096 ABOVE the set.  Every output starts as NaN.  The cases and
their conditions are checked without a GPU in tests/test_softmax_census_cpu.py, which also keeps this table complete.

Shapes: Lq in {130, 200}, Lk in {33, 64, 100, 192, 257}, B * H = 6 (unmasked), through the plumbing of
tests/test_attn_census_gpu.py (run_causal, run_kvlen, run_past) and of the frame-major census modules (device_run).

Instance -> case (run_fwd / run_bwd in csrc/attention.hip)

  unmasked vds_attn_fwd / vds_attn_bwd
  attn_fwd_kernel<HDP, HDQ, 2, true> (PIPE, lazy_softmax) x 5 head dims      test_unmasked[plain_hd*], [self_hd*]
      <96, 80> on the ones layout                                             test_unmasked[ones_narrow]
  attn_fwd_wide_kernel<HDP, HDQ, false> (lazy_softmax, 64 queries per wave)   test_unmasked[wide_hd64, wide_hd72, wide_hd96]
  attn_fwd_wide_kernel<96, 80, true> (ones_softmax)                           test_unmasked[ones_v0_*, ones_v1_*, ones_v3_*],
                                                                              [xones_mfma32]
  attn_fwd16_kernel<96>                                                       test_unmasked[ones_default, ones_v7_*],
                                                                              [xones_default, xones_dkv16, xones_separate_delta]
  attn_bwd_dq_kernel / attn_bwd_dkv_kernel<HDP, HDQ, false> x 5               test_unmasked[plain_hd*], [self_hd*]
  attn_bwd_dq_kernel / attn_bwd_dkv_kernel<96, 80, true> (Q' = bf16(Q c))     test_unmasked[ones_v0_*]; dq: [ones_v1_*]
  attn_bwd_dkv16_kernel<96, true> (-lse log2e from the (hi, lo) pair)         test_unmasked[ones_v1_*, ones_v3_*, ones_v7_*]
  attn_bwd_dq16_kernel<96, FOLD> (attn_delta_fold = 0 / 1)                    test_unmasked[ones_v3_fold*, ones_v7_fold*]
  attn_delta_kernel / attn_delta_tokmajor_kernel                              every case with a backward and no fold
  attn_bwd_dkv16_kernel<96, false> (kv_pad_ones = 2, cross_dkv16 = 2)         test_unmasked[xones_dkv16]
  attn_bwd_dkv_kernel, query range split + dkv_reduce_kernel (attn_qsplit)    test_unmasked[qsplit_hd72]

  masked (the hard recipe with traps; forward and backward, PAST forward only)
  KVLEN   vds_attn_*_kvlen                    test_masked[kvlen-*]
  CAUSAL  vds_attn_*_causal                   test_masked[causal-*]
  PAST    vds_attn_fwd_causal_past            test_masked[past-*]
  FM      vds_attn_*_causal_fm                test_masked[fm-*]                          (lazy_softmax<OWN>; attn_fwd16_kernel)
          vds_attn_*_causal_fm_chunk          test_masked[chunk-*]
  WIN     vds_attn_*_causal_fm_window         test_masked[window-*], [window_lead0-*]: no lead rows, the first sub-blocks a
                                              late query's workgroup visits are all masked (m = -1e30, l = 0 until it opens)
  TF      vds_teacher_attn_fwd / _bwd         test_masked[teacher-*]
  BAND    vds_band_attn_fwd / _bwd            test_masked[band-*]

Nothing here needs L >= 2048: the knobs reach the wide and the split instances at these sizes."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import softmax_census as SC  # noqa: E402
from test_attn_census_gpu import run_causal, run_kvlen, run_past  # noqa: E402
from test_attn_frame_band_census_gpu import device_run as band_run  # noqa: E402
from test_attn_frame_chunk_census_gpu import device_run as chunk_run  # noqa: E402
from test_attn_frame_major_census_gpu import HEADS, Variant, device_run as fm_run  # noqa: E402
from test_attn_frame_window_census_gpu import device_run as window_run  # noqa: E402
from test_attn_teacher_census_gpu import device_run as teacher_run  # noqa: E402
from test_softmax_census_cpu import B_H, CROSS_SHAPES, HEAD_DIMS, MASKED, SELF_LENGTHS, masked_case, unmasked_cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import ops as _ops
    return _ops


def report(tag, worst):
    print(f"softmax census {tag}: " + " ".join(f"{n} {x:.3f}" for n, x in worst.items()))


# family -> (head dim, layout, backward?, runner keywords, forward on the ones path?, backward on the ones route?, shapes).
# cross: run_kvlen without key lengths, (Lq, Lk); self: run_causal without frames, L.  Every head dim runs two of the five
# cross shapes, together all of them.  The ones layout (head dim 72) runs under attn_fwd_wide = 1, as in the mask census:
# variant bit 0 dK/dV, 1 dQ, 2 forward on the 16x16x32 kernels.
UNMASKED = {f"plain_hd{hd}": (hd, "cross", True, {}, False, False, [CROSS_SHAPES[i], CROSS_SHAPES[(i + 1) % 5]])
            for i, hd in enumerate(HEAD_DIMS)}
UNMASKED.update({f"self_hd{hd}": (hd, "self", True, {}, False, False, SELF_LENGTHS) for hd in (64, 72)})
UNMASKED.update({f"wide_hd{hd}": (hd, "cross", False, dict(wide=1), False, False, [(130, 257), (200, 100)])
                 for hd in (64, 72, 96)})
UNMASKED.update({f"ones_v{v}_fold{f}": (72, "self", True, dict(ones=True, wide=1, variant=v, fold=f), True, True, [200])
                 for v in (0, 1, 3, 7) for f in (0, 1)})
UNMASKED.update({
    "ones_default": (72, "self", True, dict(ones=True, wide=1), True, True, [130]),
    "ones_narrow": (72, "self", False, dict(ones=True, wide=0), False, False, [130]),
    "xones_default": (72, "cross", True, dict(pad_ones=2, wide=1), True, True, [(130, 257)]),
    "xones_dkv16": (72, "cross", True, dict(pad_ones=2, wide=1, dkv16=2), True, True, [(130, 257)]),
    "xones_mfma32": (72, "cross", True, dict(pad_ones=2, wide=1, variant=0, fold=1), True, True, [(130, 257)]),
    "xones_separate_delta": (72, "cross", True, dict(pad_ones=2, wide=1, variant=7, fold=0), True, True, [(200, 100)]),
    "qsplit_hd72": (72, "cross", True, dict(qsplit=2), False, False, [(130, 257), (200, 64)]),
})
UNMASKED_CASES = [(f, s) for f, spec in UNMASKED.items() for s in spec[6]]


@pytest.mark.parametrize("family,shape", UNMASKED_CASES, ids=[f"{f}-{s}" for f, s in UNMASKED_CASES])
def test_unmasked(ops, family, shape):
    """the hard recipe at five shifts under both group assignments, and the ladder: 11 launches of B * H = 6 heads"""
    hd, layout, bwd, kw, fwd_ones, bwd_ones, _ = UNMASKED[family]
    Lq, Lk = shape if layout == "cross" else (shape, shape)
    if layout == "cross":
        run = lambda q, k, v, do: run_kvlen(ops, q, k, v, do, None, **kw)
    else:
        run = lambda q, k, v, do: run_causal(ops, q, k, v, do, None, **kw)
    worst = {}
    for tag, q, k, v, do, mask in unmasked_cases(hd, *B_H, Lq, Lk, bwd):
        w = SC.census(f"{family}.{Lq}x{Lk}.{tag}", run, q, k, v, do, mask, fwd_ones, bwd_ones)
        worst = {n: max(x, worst.get(n, 0.0)) for n, x in w.items()}
    report(f"{family}.{Lq}x{Lk}", worst)


FM_RUNNERS = {"fm": fm_run, "chunk": chunk_run, "window": window_run, "window_lead0": window_run, "teacher": teacher_run}
# family -> the entries of HEADS (tests/test_attn_frame_major_census_gpu.py) it runs; the token-major families: head dims
MASKED_HEADS = {"kvlen": ("hd64", "hd72"), "causal": ("hd64", "hd72"), "past": ("hd64", "hd72"),
                "fm": ("hd64", "ones_all16_fold"), "chunk": ("hd64", "ones_all16_fold"),
                "window": ("hd64", "ones_all16_fold"), "window_lead0": ("hd64", "ones_all16_fold"),
                "teacher": ("hd64", "hd72_ones"), "band": ("hd64", "hd72_ones")}
MASKED_CASES = [(f, h) for f, hs in MASKED_HEADS.items() for h in hs]


@pytest.mark.parametrize("family,head", MASKED_CASES, ids=[f"{f}-{h}" for f, h in MASKED_CASES])
def test_masked(ops, family, head):
    """the hard recipe under the family's mask: the attended set scores 0, a masked key carries the row's highest score.
    The ones layout takes the bounds of the ones route: which kernels a family runs there is its own table's matter, and
    the bound of the plain route is the smaller one."""
    hd, ones, kn = HEADS[head]
    shape = MASKED[family][1]
    bwd = family != "past"
    tag, q, k, v, do, mask = masked_case(family, hd, bwd=bwd)
    if family == "kvlen":
        run = lambda q, k, v, do: run_kvlen(ops, q, k, v, do, shape)
    elif family == "causal":
        run = lambda q, k, v, do: run_causal(ops, q, k, v, do, shape[1:])
    elif family == "past":
        run = lambda q, k, v, do: run_past(ops, q, k, v, *shape)
    elif family == "band":
        run = lambda q, k, v, do: band_run(ops, shape, ones)(q, k, v, do, mask)
    else:
        run = lambda q, k, v, do: FM_RUNNERS[family](ops, shape, ones, False)(q, k, v, do, mask)
    with Variant(ops, kn):
        report(f"{family}.{head}", SC.census(f"{family}.{head}.{tag}", run, q, k, v, do, mask, ones, ones))
