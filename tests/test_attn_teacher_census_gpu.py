"""The mask census (tests/helpers/attn_census.py) on the TF instances of the frame-major attention kernels
(vds_teacher_attn_fwd / vds_teacher_attn_bwd): lse = ln N, the label counts, and the dV / dK / dQ supports and values, with
attn_census's checks and bounds under the dense teacher mask of tests/helpers/teacher_ref.py -- one wrong (query, key) pair
anywhere fails.  B * H * hd >= L, so every row is a probe (H = 2, B as large as that needs); n_c <= 64 is asserted for
every case.

Every entry of tests/test_attn_frame_major_census_gpu.py's HEADS runs: the TF runners take the plain 32x32x16 TF kernels for
every head dim and for the ones layout at head dim 72 whatever the variant mask and knobs say, which the cases under those
settings show.  Shapes: teacher_ref.SHAPES; the shapes above 320 rows run at hd 72 and 128 (the float64 expectations stay
small)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_census as AC  # noqa: E402
import frame_major_ref as FM  # noqa: E402
import teacher_ref as TR  # noqa: E402
from test_attn_frame_major_census_gpu import HEADS, Variant  # noqa: E402

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
ids = TR.ids
CASES = [(s, h) for s in TR.SHAPES for h in HEADS
         if HEADS[h][0] <= s[0] and (s[0] <= 320 or HEADS[h][0] in (72, 128))]


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
        kw = dict(kv_pad_ones=ones, frames=(lead, period), frame_major=True, chunk=c, teacher=True)
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
    assert AC.label_counts(TR.census_mask(1, *shape), hd).max().item() <= AC.MAX_LABEL  # n_c <= 64
    with Variant(ops, kn):
        TR.census(f"{ids(shape)}.{head}", hd, B, H, shape, run=device_run(ops, shape, ones, head.endswith("_o")))
