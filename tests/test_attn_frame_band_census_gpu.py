"""The mask census (tests/helpers/attn_census.py) on the BAND instances of the frame-major attention kernels
(vds_band_attn_fwd / _bwd): lse = ln N, the label counts, and the dV / dK / dQ supports and values, with attn_census's checks
and bounds (0.25, 0.25, 2^-7, 2^-6, 2^-6) under the dense band mask of tests/helpers/frame_band_ref.py -- one wrong
(query, key) pair anywhere fails.  B * H * hd >= L, so every row is a probe, and every (query, key) pair is counted; n_c <=
64 (the condition of the 0.25 bound) is asserted for every case.

Head dims 64 and 72 in the ones layout (the plain 32x32x16 BAND forward, dQ and dK/dV kernels; the ones layout also under the
variant mask and knobs that select the 16x16x32 family elsewhere and must land on the same kernels here), over
frame_band_ref.SHAPES: a first workgroup that mixes lead and token rows, short last chunks, runs that start and end inside
a 64-row tile, a gap between the lead tiles and the run, no lead rows, two lead tiles, a band that covers every pair."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_census as AC  # noqa: E402
import frame_band_ref as FB  # noqa: E402
import frame_major_ref as FM  # noqa: E402
from test_attn_frame_major_census_gpu import HEADS, Variant  # noqa: E402

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
ids = FB.ids
CASES = [(s, h) for s in FB.SHAPES for h in ("hd64", "hd72_ones", "ones_all16_fold")
         if h != "ones_all16_fold" or s in ((280, 16, 8, 2, 2), (656, 80, 9, 1, 2), (1040, 16, 8, 1, 1))]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import ops as _ops
    return _ops


def device_run(ops, shape, ones):
    """attn_census's `run` on the library: q, k, v, do in frame-major rows [B, H, L, hd] -> o, lse[, dq, dk, dv] in
    frame-major rows.  o and dO live in TOKEN rows on the device: dO row tok(r) = do[r], and o is read back through tok"""
    L, lead, period, c, band = shape
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
        o = torch.full((B * L, H * hd), nan, dtype=bf16, device="cuda")
        ov = ops.heads_view(o, B, L, H, hd)
        kw = dict(kv_pad_ones=ones, frames=(lead, period), frame_major=True, chunk=c, band=band // c)
        ops.band_attn_fwd(qp[..., :hd], kp[..., :hd], vp[..., :hd], ov, lse, **kw)
        torch.cuda.synchronize()
        out = [ov.cpu()[:, :, tok], lse.cpu()]
        if do is not None:
            do_tok = do[:, :, fm]  # token row l holds the frame-major row fm(l)
            dod = do_tok.permute(0, 2, 1, 3).reshape(B * L, H * hd).contiguous().cuda()
            dov = ops.heads_view(dod, B, L, H, hd)
            g = [torch.full((B, H, L, hdp), nan, dtype=bf16, device="cuda") for _ in range(3)]
            ops.band_attn_bwd(qp[..., :hd], kp[..., :hd], vp[..., :hd], ov, lse, dov, *(t[..., :hd] for t in g), None, **kw)
            torch.cuda.synchronize()
            out += [t[..., :hd].cpu() for t in g]
        return out
    return run


@pytest.mark.parametrize("shape,head", CASES, ids=[f"{ids(s)}-{h}" for s, h in CASES])
def test_census(ops, shape, head):
    L, lead, period, c, band = shape
    hd, ones, kn = HEADS[head]
    BH = -(-L // hd)
    B, H = (BH + 1) // 2, 2
    assert B * H * hd >= L
    assert AC.label_counts(FB.census_mask(1, L, lead, period, c, band), hd).max().item() <= AC.MAX_LABEL  # n_c <= 64
    with Variant(ops, kn):
        FB.census(f"{ids(shape)}.{head}", hd, B, H, shape, run=device_run(ops, shape, ones))
