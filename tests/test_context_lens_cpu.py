"""Per-sample context lengths, the parts that need no GPU: the two C symbols and their host-side argument checks, the
mask -> lengths helper, the T5 glue's `return_lengths`, and the validation of a host sequence in DiT.forward."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from video_diffusion_speedrun_amd import _lib, train
from video_diffusion_speedrun_amd.model import DiT, DiTBlock, check_context_lens

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vds_attn_fwd_kvlen", "vds_attn_bwd_kvlen")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vds.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"\bint\s+{name}\s*\(\s*const\s+vds_attn_args\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,"
                         rf"\s*vds_stream_t\s+\w+\s*\)\s*;", src), f"{name} is not declared in include/vds.h"
        assert len(_lib.SIGNATURES[name]) == 3
        assert hasattr(raw, name), name


def test_host_side_argument_checks(lib):
    lens = (C.c_int32 * 4)(1, 1, 1, 1)  # never dereferenced: every call below is refused before a launch
    for fn in (lib.vds_attn_fwd_kvlen, lib.vds_attn_bwd_kvlen):
        assert fn(None, None, None) == -1                      # null args
        assert fn(None, C.cast(lens, C.c_void_p), None) == -1
        a = _lib.AttnArgs()
        a.B, a.H, a.Lq, a.Lk, a.head_dim = 4, 2, 16, 16, 72
        a.kv_pad_ones = 1                                      # self-attention on annotated q rows: no lengths
        assert fn(C.byref(a), C.cast(lens, C.c_void_p), None) == -1
        a.kv_pad_ones = 0
        assert fn(C.byref(a), C.cast(lens, C.c_void_p), None) == -1  # null operands, as in the calls without lengths
        assert fn(C.byref(a), None, None) == -1                      # forwarded to vds_attn_fwd / vds_attn_bwd


def test_lens_from_mask():
    m = torch.tensor([[1, 1, 1, 0, 0], [1, 0, 0, 0, 0], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0]])
    lens = train.lens_from_mask(m)
    assert lens.dtype == torch.int32 and lens.device.type == "cpu" and lens.tolist() == [3, 1, 5, 0]
    assert train.lens_from_mask(m.bool()).tolist() == [3, 1, 5, 0]
    assert train.lens_from_mask(torch.ones(2, 7, dtype=torch.int64)).tolist() == [7, 7]
    assert train.lens_from_mask(torch.zeros(3, 4)).tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        train.lens_from_mask(torch.tensor([[1, 1, 0, 1], [1, 1, 0, 0]]))  # a one after a zero
    with pytest.raises(ValueError):
        train.lens_from_mask(torch.tensor([[0, 1, 1, 1]]))                # left padding
    with pytest.raises(ValueError):
        train.lens_from_mask(torch.ones(4))


class _Tokens:
    def __init__(self, ids, mask):
        self.input_ids, self.attention_mask = ids, mask


def _fake_t5(max_len=6, width=8):
    """a tokenizer that makes one token per word plus an end token, and an encoder whose states are the ids"""
    def tokenizer(prompts, padding, max_length, truncation, return_length, return_overflowing_tokens, return_tensors):
        assert padding == "max_length" and truncation and return_tensors == "pt"
        ids = torch.zeros(len(prompts), max_length, dtype=torch.int64)
        mask = torch.zeros(len(prompts), max_length, dtype=torch.int64)
        for b, p in enumerate(prompts):
            n = min(len(p.split()) + 1, max_length)
            ids[b, :n] = torch.arange(1, n + 1)
            mask[b, :n] = 1
        return _Tokens(ids, mask)

    def encoder(input_ids, return_dict, output_hidden_states):
        h = input_ids.float().unsqueeze(-1).expand(-1, -1, width)
        return types.SimpleNamespace(hidden_states=(h * 0.5, h))
    encoder.dtype = torch.float32
    return encoder, tokenizer


def test_encode_prompt_with_t5_return_lengths():
    enc, tok = _fake_t5()
    prompts = ["a red fox", "", "one two three four five six seven"]
    plain = train.encode_prompt_with_t5(enc, tok, max_sequence_length=6, prompt=prompts, device="cpu")
    assert isinstance(plain, torch.Tensor) and tuple(plain.shape) == (3, 6, 8)   # the default return is unchanged
    states, lens = train.encode_prompt_with_t5(enc, tok, max_sequence_length=6, prompt=prompts, device="cpu",
                                               return_lengths=True)
    assert torch.equal(states, plain)
    assert lens.dtype == torch.int32 and lens.tolist() == [4, 1, 6]


def test_check_context_lens():
    assert check_context_lens([3, 0, 5], 3, 5).tolist() == [3, 0, 5]
    assert check_context_lens((1, 2), 2, 2).dtype == torch.int32
    assert check_context_lens(torch.tensor([4, 4], dtype=torch.int64), 2, 4).tolist() == [4, 4]
    for bad in ([3, 0], [3, 0, 5, 1]):               # wrong length
        with pytest.raises(ValueError):
            check_context_lens(bad, 3, 5)
    with pytest.raises(ValueError):
        check_context_lens([3, 6, 0], 3, 5)          # above Lc
    with pytest.raises(ValueError):
        check_context_lens([3, -1, 0], 3, 5)         # negative
    with pytest.raises(ValueError):
        check_context_lens([3.0, 1, 0], 3, 5)        # not ints
    with pytest.raises(ValueError):
        check_context_lens(torch.tensor([1.0, 2.0, 3.0]), 3, 5)
    with pytest.raises(ValueError):
        check_context_lens(torch.tensor([[1, 2, 3]]), 3, 5)
    with pytest.raises(ValueError):
        check_context_lens(torch.tensor([1, 9, 3]), 3, 5)   # a CPU tensor is validated like a sequence


def _tiny(**kw):
    return DiT(in_channels=16, patch_size=2, hidden_size=128, depth=1, num_heads=2, train_bias_and_rms=False, **kw)


def test_dit_forward_validates_a_host_sequence_before_anything_runs():
    """a bad host sequence is a ValueError even on CPU tensors, i.e. before the "GPU only" error of DiT.forward"""
    m = _tiny(cross_attn_input_size=32)
    x, ctx, t = torch.zeros(2, 16, 4, 8, 8), torch.zeros(2, 5, 32), torch.zeros(2)
    for bad in ([5], [5, 5, 5], [5, 6], [-1, 5]):
        with pytest.raises(ValueError):
            m(x, ctx, t, context_lens=bad)
    with pytest.raises(RuntimeError):   # a valid one goes on to the GPU-only error
        m(x, ctx, t, context_lens=[5, 0])
    with pytest.raises(ValueError):     # a model without cross-attention takes no lengths
        _tiny(cross_attn_input_size=None)(x, ctx, t, context_lens=[5, 0])
    m.enable_fp8()                      # fp8 cross-attention has no masked kernels: loud, and names the way out
    with pytest.raises(NotImplementedError, match=r"enable_fp8\(cross_attention=False\)"):
        m(x, ctx, t, context_lens=[5, 0])
    blk = DiTBlock(128, 32, 2)
    with pytest.raises(ValueError):
        blk(torch.zeros(2, 20, 128), torch.zeros(2, 5, 32), torch.zeros(2, 128), context_lens=[5, 9])
    with pytest.raises(ValueError):
        DiTBlock(128, None, 2)(torch.zeros(2, 20, 128), None, torch.zeros(2, 128), context_lens=[5, 5])
