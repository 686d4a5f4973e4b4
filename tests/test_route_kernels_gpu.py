"""The row movers of token routing (csrc/route.hip) through their C entries, bit for bit: vds_rows_gather against
torch.index_select, vds_rows_merge against torch.where on inv, vds_rows_scatter_add_f32 against index_add_ (one fp32 add per
element, so the bits must match).  Every operand is a window inside a sentinel-filled parent allocation: the guard bands must
come back intact, and an index out of range -- which must read nothing / write nothing -- would reach sentinel bytes INSIDE
the allocation and fail the comparison; no index in this file points outside an allocated buffer.

Shapes: row_bytes 16 (one piece), 144 (a cos row of head_dim 72), 160 (a v_0 row of hdp 80), 288 and 2304 (D = 144 and 1152
in bf16); outer 1 and 3; (n_in, n_out) = (1, 1), (17, 5), (272, 144), (272, 272) -- one row, a tile that holds several short
rows and ends inside one, more than one 1024-piece tile per slice, and the identity size."""
import pytest
import torch

pytestmark = pytest.mark.gpu
SENT = 0xA5
ROW_BYTES = [16, 144, 160, 288, 2304]
OUTER = [1, 3]
SHAPES = [(1, 1), (17, 5), (272, 144), (272, 272)]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from video_diffusion_speedrun_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Window:
    """[outer, n, row_bytes] bytes inside a parent filled with SENT; the bands are two rows (at least 256 bytes) wide"""

    def __init__(self, outer, n, row_bytes, fill=None, gen=None):
        self.pad = max(256, 2 * row_bytes)
        self.shape = (outer, n, row_bytes)
        self.total = outer * n * row_bytes
        self.parent = torch.full((2 * self.pad + self.total,), SENT, dtype=torch.uint8, device="cuda")
        assert self.parent.data_ptr() % 16 == 0 and self.pad % 16 == 0
        if fill == "random":
            self.view.copy_(torch.randint(0, 256, self.shape, dtype=torch.uint8, generator=gen).cuda())
        elif fill == "f32":  # small integers and halves: every sum of two is exact, but the bits are compared anyway
            vals = torch.randint(-64, 64, (outer, n, row_bytes // 4), generator=gen).float() * 0.5
            self.view.copy_(vals.view(torch.uint8).view(self.shape).cuda())

    @property
    def view(self):
        return self.parent[self.pad:self.pad + self.total].view(self.shape)

    @property
    def ptr(self):
        return self.parent.data_ptr() + self.pad

    def f32(self):
        return self.view.view(torch.float32)

    def bands_intact(self):
        return bool((self.parent[:self.pad] == SENT).all()) and bool((self.parent[self.pad + self.total:] == SENT).all())


def index_kinds(n_in, n_out, gen, duplicates):
    """idx tables [n_out] with entries in [0, n_in): identity, reversed, a seeded random subset (distinct; needs n_out <=
    n_in) and, for the gather, one with duplicates"""
    kinds = {"identity": torch.arange(n_out) % n_in, "reversed": (n_in - 1 - torch.arange(n_out)) % n_in,
             "random": torch.randperm(n_in, generator=gen)[:n_out]}
    if duplicates:
        kinds["duplicates"] = torch.randint(0, n_in, (n_out,), generator=gen)
        if n_out >= 2:
            kinds["duplicates"][1] = kinds["duplicates"][0]
    return {k: v.to(torch.int32) for k, v in kinds.items()}


def dev(t):
    return t.to(torch.int32).cuda().contiguous()


@pytest.mark.parametrize("n_in,n_out", SHAPES)
@pytest.mark.parametrize("outer", OUTER)
@pytest.mark.parametrize("row_bytes", ROW_BYTES)
def test_gather_is_index_select(lib, row_bytes, outer, n_in, n_out):
    gen = torch.Generator().manual_seed(row_bytes + 7 * outer + n_in)
    src = Window(outer, n_in, row_bytes, "random", gen)
    for kind, idx in index_kinds(n_in, n_out, gen, True).items():
        dst = Window(outer, n_out, row_bytes)
        d_idx = dev(idx)
        assert lib.vds_rows_gather(src.ptr, dst.ptr, d_idx.data_ptr(), outer, n_in, n_out, row_bytes, stream()) == 0
        torch.cuda.synchronize()
        want = src.view.index_select(1, d_idx.long())
        assert torch.equal(dst.view, want), kind
        assert dst.bands_intact() and src.bands_intact(), kind


@pytest.mark.parametrize("n_in,n_out", [(17, 5), (272, 144)])
@pytest.mark.parametrize("outer", OUTER)
@pytest.mark.parametrize("row_bytes", ROW_BYTES)
def test_gather_writes_zeros_for_an_index_out_of_range(lib, row_bytes, outer, n_in, n_out):
    """n_in, n_in + 1 and -1 would read the next slice, the row behind it, the slice before -- or the sentinel bands"""
    gen = torch.Generator().manual_seed(row_bytes + outer)
    src = Window(outer, n_in, row_bytes, "random", gen)
    idx = torch.randperm(n_in, generator=gen)[:n_out].to(torch.int32)
    idx[0], idx[2], idx[n_out - 1] = n_in, n_in + 1, -1
    dst = Window(outer, n_out, row_bytes)
    d_idx = dev(idx)
    assert lib.vds_rows_gather(src.ptr, dst.ptr, d_idx.data_ptr(), outer, n_in, n_out, row_bytes, stream()) == 0
    torch.cuda.synchronize()
    valid = (idx >= 0) & (idx < n_in)
    want = src.view.index_select(1, d_idx.long().clamp(0, n_in - 1))
    want[:, ~valid.cuda()] = 0
    assert int((~valid).sum()) == 3
    assert torch.equal(dst.view, want)
    assert dst.bands_intact() and src.bands_intact()


def inverse_of(idx, n_full):
    inv = torch.full((n_full,), -1, dtype=torch.int32)
    inv[idx.long()] = torch.arange(idx.shape[0], dtype=torch.int32)
    return inv


def merge_want(full, part, inv, n_part):
    routed = ((inv >= 0) & (inv < n_part)).cuda()
    picked = part.view.index_select(1, dev(inv).long().clamp(0, n_part - 1))
    return torch.where(routed[None, :, None], picked, full.view)


@pytest.mark.parametrize("n_full,n_part", SHAPES)
@pytest.mark.parametrize("outer", OUTER)
@pytest.mark.parametrize("row_bytes", ROW_BYTES)
def test_merge_is_where_on_inv(lib, row_bytes, outer, n_full, n_part):
    """into a third buffer and in place (dst == full); inv values n_part and -2 take the full row"""
    gen = torch.Generator().manual_seed(3 * row_bytes + outer + n_full)
    part = Window(outer, n_part, row_bytes, "random", gen)
    for kind, idx in index_kinds(n_full, n_part, gen, False).items():
        inv = inverse_of(idx, n_full)
        if n_full >= 17:  # two rows that take no part row carry the two out-of-range values; one routed row loses its part row
            free = (inv < 0).nonzero().flatten()
            if len(free) >= 2:
                inv[free[0]], inv[free[1]] = n_part, -2
            inv[int(idx[0])] = n_part
        full = Window(outer, n_full, row_bytes, "random", gen)
        want = merge_want(full, part, inv, n_part)
        d_inv = dev(inv)
        dst = Window(outer, n_full, row_bytes)
        assert lib.vds_rows_merge(full.ptr, part.ptr, dst.ptr, d_inv.data_ptr(), outer, n_full, n_part, row_bytes,
                                  stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(dst.view, want), kind
        assert dst.bands_intact() and part.bands_intact() and full.bands_intact(), kind
        assert lib.vds_rows_merge(full.ptr, part.ptr, full.ptr, d_inv.data_ptr(), outer, n_full, n_part, row_bytes,
                                  stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(full.view, want), kind + " in place"
        assert full.bands_intact() and part.bands_intact(), kind


@pytest.mark.parametrize("n_full,n_part", SHAPES)
@pytest.mark.parametrize("outer", OUTER)
@pytest.mark.parametrize("row_bytes", ROW_BYTES)
def test_scatter_add_is_index_add(lib, row_bytes, outer, n_full, n_part):
    gen = torch.Generator().manual_seed(5 * row_bytes + outer + n_full)
    part = Window(outer, n_part, row_bytes, "f32", gen)
    for kind, idx in index_kinds(n_full, n_part, gen, False).items():
        acc = Window(outer, n_full, row_bytes, "f32", gen)
        d_idx = dev(idx)
        want = acc.f32().clone().index_add_(1, d_idx.long(), part.f32())
        assert lib.vds_rows_scatter_add_f32(part.ptr, acc.ptr, d_idx.data_ptr(), outer, n_full, n_part, row_bytes // 4,
                                            stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(acc.f32().view(torch.int32), want.view(torch.int32)), kind
        assert acc.bands_intact() and part.bands_intact(), kind


@pytest.mark.parametrize("n_full,n_part", [(17, 5), (272, 144)])
@pytest.mark.parametrize("outer", OUTER)
@pytest.mark.parametrize("row_bytes", ROW_BYTES)
def test_scatter_add_skips_an_index_out_of_range(lib, row_bytes, outer, n_full, n_part):
    """n_full, n_full + 1 and -1 would add into the next slice, the row behind it, the slice before -- or the bands"""
    gen = torch.Generator().manual_seed(row_bytes + 11 * outer)
    part = Window(outer, n_part, row_bytes, "f32", gen)
    acc = Window(outer, n_full, row_bytes, "f32", gen)
    idx = torch.randperm(n_full, generator=gen)[:n_part].to(torch.int32)
    idx[0], idx[2], idx[n_part - 1] = n_full, n_full + 1, -1
    valid = (idx >= 0) & (idx < n_full)
    keep = valid.nonzero().flatten().cuda()
    want = acc.f32().clone().index_add_(1, dev(idx).long()[keep], part.f32().index_select(1, keep))
    d_idx = dev(idx)
    assert lib.vds_rows_scatter_add_f32(part.ptr, acc.ptr, d_idx.data_ptr(), outer, n_full, n_part, row_bytes // 4,
                                        stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(acc.f32().view(torch.int32), want.view(torch.int32))
    assert acc.bands_intact() and part.bands_intact()


def test_no_rows_is_ok_and_touches_nothing(lib):
    src = Window(2, 9, 144, "random", torch.Generator().manual_seed(1))
    dst = Window(2, 4, 144)
    idx = dev(torch.arange(4))
    assert lib.vds_rows_gather(src.ptr, dst.ptr, idx.data_ptr(), 2, 9, 0, 144, stream()) == 0
    acc = Window(2, 9, 144, "f32", torch.Generator().manual_seed(2))
    before = acc.parent.clone()
    assert lib.vds_rows_scatter_add_f32(dst.ptr, acc.ptr, idx.data_ptr(), 2, 9, 0, 36, stream()) == 0
    assert lib.vds_rows_merge(acc.ptr, dst.ptr, acc.ptr, dev(torch.full((9,), -1)).data_ptr(), 2, 9, 0, 144, stream()) == 0
    torch.cuda.synchronize()
    assert bool((dst.parent == SENT).all()) and torch.equal(acc.parent, before)


def test_ops_wrappers(lib):
    """ops.rows_gather / rows_merge / rows_scatter_add on the model's three tensors, and what they refuse"""
    from video_diffusion_speedrun_amd import ops
    g = torch.Generator().manual_seed(9)
    X = torch.randn(2, 40, 144, generator=g).to(torch.bfloat16).cuda()
    v0 = torch.randn(2, 2, 40, 96, generator=g).to(torch.bfloat16).cuda()
    cos = torch.randn(40, 36, generator=g).cuda()
    idx = dev(torch.tensor([0, 1, 5, 17, 39]))
    for t, dim in ((X, 1), (v0, 2), (cos, 0)):
        assert torch.equal(ops.rows_gather(t, idx), t.index_select(dim, idx.long()))
    inv = dev(inverse_of(idx.cpu(), 40))
    part = ops.rows_gather(X, idx) + 1
    want = X.clone()
    want[:, idx.long()] = part
    out = torch.empty_like(X)
    assert ops.rows_merge(X, part, inv, out=out) is out and torch.equal(out, want)
    assert ops.rows_merge(X, part, inv) is X and torch.equal(X, want)
    acc = torch.randn(2, 2, 40, 96, generator=g).cuda()
    p = torch.randn(2, 2, 5, 96, generator=g).cuda()
    want = acc.clone().index_add_(2, idx.long(), p)
    assert ops.rows_scatter_add(p, acc, idx) is acc and torch.equal(acc, want)
    with pytest.raises(ValueError, match="contiguous"):
        ops.rows_gather(X[:, :, :72], idx)
    with pytest.raises(ValueError, match="16-byte pieces"):
        ops.rows_gather(torch.zeros(4, 12, dtype=torch.bfloat16, device="cuda"), idx[:2])
    with pytest.raises(ValueError, match="int32"):
        ops.rows_gather(X, idx.long())
    with pytest.raises(ValueError, match=r"\.cuda\(\)"):
        ops.rows_gather(X.cpu(), idx)
    with pytest.raises(ValueError, match="int32"):
        ops.rows_gather(X, idx.cpu())
    with pytest.raises(ValueError, match="must agree"):
        ops.rows_merge(X, part.float(), inv)
    with pytest.raises(ValueError, match="shape \\[40\\]"):
        ops.rows_merge(X, part, inv[:39])
    with pytest.raises(ValueError, match="float32"):
        ops.rows_scatter_add(part, X, idx)
