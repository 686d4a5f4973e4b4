"""The mask census (tests/helpers/attn_census.py) on the frame-major attention kernels under the chunk mask
(vds_attn_*_causal_fm_chunk): lse = ln N, the label counts, and the dV / dK / dQ supports and values, with attn_census's
checks and bounds (0.25, 0.25, 2^-7, 2^-6, 2^-6) under the dense chunk mask of tests/helpers/frame_chunk_ref.py -- one wrong
(query, key) pair anywhere fails.  B * H * hd >= L, so every row is a probe; n_c <= 64 (the condition of the 0.25 bound) is
asserted for every case.

Kernel instance -> case: the chunk calls run the frame-major instances, so the map is the one of
tests/test_attn_frame_major_census_gpu.py.  The ones layout (kv_pad_ones = 1, head dim 72) reaches the 16x16x32 family
through the variant mask (vds_attn_set_variant: bit 0 dK/dV, 1 dQ, 2 forward), the attn_delta_fold knob and
attn_fwd_wide = 1 (64 queries per wave; the rule takes it from 2048 queries).
  attn_fwd_kernel<HDP, HDQ, 2, true, .., FM>          hd32 (32, 32), hd64 (64, 64), hd72 / hd72_ones / ones_dq16 /
                                                      ones_mfma32 (96, 80), hd96 (96, 96), hd128 (128, 128)
  attn_bwd_dq_kernel<HDP, HDQ, false, .., FM>         the same plain cases; ones_fwd16_dkv16, ones_mfma32 (96, 80)
  attn_bwd_dkv_kernel<HDP, HDQ, false, .., FM>        the same plain cases; ones_dq16, ones_mfma32 (96, 80)
  attn_fwd16_kernel<96, .., FM>                       ones_all16_fold, ones_all16_delta, ones_fwd16_dkv16
  attn_bwd_dq16_kernel<96, FOLD = true, .., FM>       hd72_ones (defaults), ones_all16_fold
  attn_bwd_dq16_kernel<96, FOLD = false, .., FM>      ones_all16_delta, ones_dq16
  attn_bwd_dkv16_kernel<96, QPAD, .., FM>             hd72_ones, ones_all16_fold, ones_all16_delta, ones_fwd16_dkv16
  attn_delta_tokmajor_kernel<FM>                      every case without FOLD (o / dO token-major views of [B*L, H*hd])
  attn_delta_kernel<FM>                               hd72_headmajor_o: o / dO as head-major [B, H, L, hd] buffers
Shapes: frame_chunk_ref.SHAPES -- short last chunks, one token group (c >= period), no lead rows, S = 1, chunks of several
256-row tiles; (80, 16, 64, 16) runs at hd <= 72 (a head needs hd distinct probe rows), the two long shapes at hd 72 and
128 (the float64 expectations stay small)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_census as AC  # noqa: E402
import frame_chunk_ref as CH  # noqa: E402
import frame_major_ref as FM  # noqa: E402
from test_attn_frame_major_census_gpu import HEADS, Variant  # noqa: E402

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
ids = CH.ids
CASES = [(s, h) for s in CH.SHAPES for h in HEADS
         if HEADS[h][0] <= s[0] and (s[0] <= 300 or HEADS[h][0] in (72, 128))]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import ops as _ops
    return _ops


def device_run(ops, shape, ones, headmajor_o):
    """attn_census's `run` on the library: q, k, v, do in frame-major rows [B, H, L, hd] -> o, lse[, dq, dk, dv] in
    frame-major rows.  o and dO live in TOKEN rows on the device: dO row tok(r) = do[r], and o is read back through tok"""
    L, lead, period, c = shape
    tok, fm = FM.tok_index(L, lead, period), FM.fm_index(L, lead, period)

    def run(q, k, v, do, mask):
        B, H, _, hd = q.shape
        hdp = 96 if ones else hd
        nan = float("nan")

        def padded(t, which):
            buf = torch.zeros(B, H, L, hdp, dtype=bf16)
            buf[..., :hd] = t
            if ones and which == "k":
                buf[..., hd] = 1
                buf[..., hd + 1] = 1
            if ones and which == "v":
                buf[..., hd] = 1
                buf[..., hd + 4] = 1
            return buf.cuda()
        qp, kp, vp = padded(q, "q"), padded(k, "k"), padded(v, "v")
        lse = torch.full((B, H, L), nan, dtype=f32, device="cuda")
        if headmajor_o:
            o = torch.full((B, H, L, hd), nan, dtype=bf16, device="cuda")
            ov = o
        else:
            o = torch.full((B * L, H * hd), nan, dtype=bf16, device="cuda")
            ov = ops.heads_view(o, B, L, H, hd)
        kw = dict(kv_pad_ones=ones, frames=(lead, period), frame_major=True, chunk=c)
        ops.attn_fwd(qp[..., :hd], kp[..., :hd], vp[..., :hd], ov, lse, **kw)
        torch.cuda.synchronize()
        out = [ov.cpu()[:, :, tok], lse.cpu()]
        if do is not None:
            do_tok = do[:, :, fm]  # token row l holds the frame-major row fm(l)
            if headmajor_o:
                dov = do_tok.contiguous().cuda()
            else:
                dod = do_tok.permute(0, 2, 1, 3).reshape(B * L, H * hd).contiguous().cuda()
                dov = ops.heads_view(dod, B, L, H, hd)
            g = [torch.full((B, H, L, hdp), nan, dtype=bf16, device="cuda") for _ in range(3)]
            ops.attn_bwd(qp[..., :hd], kp[..., :hd], vp[..., :hd], ov, lse, dov, *(t[..., :hd] for t in g), None, **kw)
            torch.cuda.synchronize()
            out += [t[..., :hd].cpu() for t in g]
        return out
    return run


@pytest.mark.parametrize("shape,head", CASES, ids=[f"{ids(s)}-{h}" for s, h in CASES])
def test_census(ops, shape, head):
    L, lead, period, c = shape
    hd, ones, kn = HEADS[head]
    BH = -(-L // hd)
    B, H = (BH + 1) // 2, 2
    assert B * H * hd >= L
    assert AC.label_counts(CH.census_mask(1, L, lead, period, c), hd).max().item() <= AC.MAX_LABEL  # n_c <= 64
    with Variant(ops, kn):
        CH.census(f"{ids(shape)}.{head}", hd, B, H, L, lead, period, c, run=device_run(ops, shape, ones, head.endswith("_o")))
