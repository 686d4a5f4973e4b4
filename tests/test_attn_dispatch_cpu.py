"""The host dispatch of the 13 bf16 attention entry points without a GPU: ONE table of defects -- NULL pointers, strides off
their alignment, head dims without an instance, each mask's own refusals, each forwarding rule -- run through every entry
point, and the return code each documents in include/vds.h (-1 VDS_ERR_ARG, -2 VDS_ERR_UNSUPPORTED; ARG wins where both
apply).  Every call carries a defect, so every call is refused on the host: the tensor pointers are the value 16 and are never
dereferenced, nothing is launched."""
import ctypes as C
import os

import pytest

from video_diffusion_speedrun_amd import _lib

ARG, UNSUPPORTED = -1, -2
FWD_PTRS = ("q", "k", "v", "o", "lse")
BWD_PTRS = ("d_o", "dq", "dk", "dv", "delta")
FWD_STRIDES = {"q": 4, "k": 4, "v": 4, "o": 2}        # q / k / v strides: multiples of 8 elements; o: of 4
BWD_STRIDES = {"do": 4, "dq": 2, "dk": 2, "dv": 2}    # d_o: multiples of 8; dq / dk / dv: of 4
BIG = (1 << 21) + 8                                   # rows: more than the frame maps' fp32 quotients take

# entry point -> (backward, mask); the mask decides the extra arguments and which rows of the table apply
ENTRIES = {
    "vds_attn_fwd": (False, "none"), "vds_attn_bwd": (True, "none"),
    "vds_attn_fwd_kvlen": (False, "kvlen"), "vds_attn_bwd_kvlen": (True, "kvlen"),
    "vds_attn_fwd_causal": (False, "causal"), "vds_attn_bwd_causal": (True, "causal"),
    "vds_attn_fwd_causal_past": (False, "past"),
    "vds_attn_fwd_causal_fm": (False, "fm"), "vds_attn_bwd_causal_fm": (True, "fm"),
    "vds_attn_fwd_causal_fm_chunk": (False, "chunk"), "vds_attn_bwd_causal_fm_chunk": (True, "chunk"),
    "vds_attn_fwd_causal_fm_window": (False, "window"), "vds_attn_bwd_causal_fm_window": (True, "window"),
}
FRAMED = ("causal", "past", "fm", "chunk", "window")
FRAME_MAJOR = ("fm", "chunk", "window")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def call(lib, name, **defect):
    """the entry point on a call that WOULD run -- B 1, H 2, L 48, head dim 64, frames (16, 8); past 8 (Lk 56), chunk 2,
    window 2 of the 4 chunks where the entry point takes them -- with `defect` laid over it: fields of vds_attn_args by
    name, `L` (Lq and Lk), the extra arguments `kv_lens`, `frames`, `past`, `chunk`, `window`, or `args=None`"""
    bwd, mask = ENTRIES[name]
    d = dict(defect)
    extra = {"kv_lens": 16, "frames": (16, 8), "past": 8, "chunk": 2, "window": 2}
    extra.update({k: d.pop(k) for k in list(d) if k in extra})
    a = _lib.AttnArgs()
    L = d.pop("L", 48)
    a.B, a.H, a.Lq, a.Lk, a.head_dim = 1, 2, L, L + (extra["past"] if mask == "past" else 0), 64
    for f in FWD_PTRS + BWD_PTRS:
        setattr(a, f, 16)  # never dereferenced: every call is refused on the host
    for t in list(FWD_STRIDES) + list(BWD_STRIDES):
        setattr(a, t + "_sb", 2 * L * 64), setattr(a, t + "_sh", L * 64), setattr(a, t + "_sl", 64)
    ref = None if d.pop("args", a) is None else C.byref(a)
    for f, val in d.items():
        assert hasattr(a, f), f
        setattr(a, f, val)
    fr = None if extra["frames"] is None else C.byref(_lib.ModGroups(*extra["frames"]))
    more = {"none": (), "kvlen": (extra["kv_lens"],), "causal": (fr,), "fm": (fr,), "past": (fr, extra["past"]),
            "chunk": (fr, extra["chunk"]), "window": (fr, extra["chunk"], extra["window"])}[mask]
    return getattr(lib, name)(ref, *more, None)


def table(name):
    """(label, defect, documented return code) for one entry point"""
    bwd, mask = ENTRIES[name]
    rows = []

    def add(label, code, **defect):
        rows.append((label, defect, code))

    # ---- NULL pointers and non-positive lengths (vds_attn_bwd's lengths: test_bwd_refuses_non_positive_lengths)
    add("args NULL", ARG, args=None)
    for f in FWD_PTRS:
        add(f"{f} NULL", ARG, **{f: None})
    for f in BWD_PTRS:  # the forward calls do not look at the gradient pointers: the head dim is what they refuse
        add(f"{f} NULL", ARG if bwd else UNSUPPORTED, head_dim=136, **{f: None})
    if name != "vds_attn_bwd":
        for f in ("Lq", "Lk"):
            for val in (0, -8):
                add(f"{f} = {val}", ARG, **{f: val})
        add("L = 0", ARG, L=0)
    # ---- strides off their alignment
    for t, s in FWD_STRIDES.items():
        for ax in ("_sb", "_sh", "_sl"):
            add(f"{t}{ax} = {s}", ARG, **{t + ax: s})
    for t, s in BWD_STRIDES.items():
        for ax in ("_sb", "_sh", "_sl"):
            add(f"{t}{ax} = {s}", ARG if bwd else UNSUPPORTED, head_dim=136, **{t + ax: s})
    # ---- head dims without an instance; an earlier defect wins
    for hd in (0, 12, 136):
        add(f"head dim {hd}", UNSUPPORTED, head_dim=hd)
        add(f"head dim {hd}, q NULL", ARG, head_dim=hd, q=None)
    add("head dim 72, q_sl = 4", ARG, head_dim=72, q_sl=4)
    add("head dim 72, v NULL", ARG, head_dim=72, v=None)
    # ---- the masks' own refusals
    if mask == "kvlen":
        add("lengths on annotated q rows", ARG, kv_pad_ones=1)
        add("lengths on annotated q rows, head dim 136", ARG, kv_pad_ones=1, head_dim=136)
    if mask in FRAMED:
        add("Lq != Lk" + (" + past" if mask == "past" else ""), ARG, Lk=64)
        add("Lq != Lk, head dim 136", ARG, Lk=64, head_dim=136)
        add("the cross-attention layout", ARG, kv_pad_ones=2)
        for fr in ((16, 5), (-1, 8), (16, 0), (16, -8), (56, 8)):
            add(f"frames {fr} do not fit", ARG, frames=fr)
        add("frames do not fit, head dim 136", ARG, frames=(16, 5), head_dim=136)
        add("more than 2^21 rows", UNSUPPORTED, L=BIG, frames=(0, 8))
        add("more than 2^21 rows, the cross-attention layout", ARG, L=BIG, frames=(0, 8), kv_pad_ones=2)
        add("more than 2^21 rows, frames do not fit", ARG, L=BIG, frames=(0, 7))
        add("more than 2^21 rows, k_sh = 4", ARG, L=BIG, frames=(0, 8), k_sh=4)
    if mask == "past":
        add("more than 2^21 key rows", UNSUPPORTED, L=1 << 21, frames=(0, 8))  # Lq = 2^21 alone is accepted: Lk counts
        add("past < 0", ARG, past=-8)
        add("past < 0, frames NULL", ARG, past=-8, frames=None)
        add("frames NULL with a past", ARG, frames=None)
        add("frames NULL with a past, head dim 136", ARG, frames=None, head_dim=136)
    if mask in FRAME_MAJOR:
        add("frames NULL", ARG, frames=None)
        add("frames NULL, head dim 136", ARG, frames=None, head_dim=136)
        add("args NULL, frames NULL", ARG, args=None, frames=None)
        add("o slice of 4 GiB", UNSUPPORTED, o_sl=1 << 26)
        add("o slice of 4 GiB, Lq != Lk", ARG, o_sl=1 << 26, Lk=64)
        add("o slice of 4 GiB, v_sb = 4", ARG, o_sl=1 << 26, v_sb=4)
        if bwd:
            add("d_o slice of 4 GiB", UNSUPPORTED, do_sl=1 << 26)
            add("d_o slice of 4 GiB, frames do not fit", ARG, do_sl=1 << 26, frames=(16, 5))
    if mask in ("chunk", "window"):
        for c in (0, -1, -(1 << 31)):
            add(f"chunk = {c}", ARG, chunk=c)
            add(f"chunk = {c}, head dim 136", ARG, chunk=c, head_dim=136)
            add(f"chunk = {c}, args NULL", ARG, chunk=c, args=None)
    if mask == "window":
        for w in (0, -1, -(1 << 31)):
            add(f"window = {w}", ARG, window=w)
            add(f"window = {w}, head dim 136", ARG, window=w, head_dim=136)
            add(f"window = {w}, chunk = 1", ARG, window=w, chunk=1)
    # ---- the forwarding rules: the forwarded call's refusals, and none of the forwarding call's own
    if mask == "kvlen":
        add("kv_lens NULL -> plain: q NULL", ARG, kv_lens=None, q=None)
        add("kv_lens NULL -> plain: o_sl = 2", ARG, kv_lens=None, o_sl=2)
        add("kv_lens NULL -> plain: head dim 136", UNSUPPORTED, kv_lens=None, head_dim=136)
        add("kv_lens NULL -> plain: annotated q rows are its own layout", UNSUPPORTED, kv_lens=None, kv_pad_ones=1, head_dim=136)
        add("kv_lens NULL, args NULL", ARG, kv_lens=None, args=None)
    if mask == "causal":
        add("frames NULL -> plain: k NULL", ARG, frames=None, k=None)
        add("frames NULL -> plain: head dim 12", UNSUPPORTED, frames=None, head_dim=12)
        add("frames NULL -> plain: Lq != Lk is cross-attention", UNSUPPORTED, frames=None, Lk=64, head_dim=136)
        add("frames NULL -> plain: so is kv_pad_ones = 2", UNSUPPORTED, frames=None, kv_pad_ones=2, head_dim=136)
        add("frames NULL, args NULL", ARG, frames=None, args=None)
    if mask == "past":
        add("past 0 -> causal: Lq != Lk", ARG, past=0, Lk=56)
        add("past 0 -> causal: frames do not fit", ARG, past=0, frames=(16, 5))
        add("past 0 -> causal: more than 2^21 rows", UNSUPPORTED, past=0, L=BIG, frames=(0, 8))
        add("past 0 -> causal: head dim 136", UNSUPPORTED, past=0, head_dim=136)
        add("past 0 -> causal -> plain: frames NULL, head dim 136", UNSUPPORTED, past=0, frames=None, head_dim=136)
        add("past 0 -> causal -> plain: frames NULL, lse NULL", ARG, past=0, frames=None, lse=None)
        add("past 0, args NULL", ARG, past=0, args=None)
    if mask in ("chunk", "window"):
        forwards = [("chunk 1 -> fm", dict(chunk=1))]
        if mask == "window":
            forwards = [("window over every chunk -> chunk", dict(window=4)),
                        ("window past every chunk -> chunk", dict(chunk=3, window=40)),
                        ("window over the one chunk -> chunk", dict(chunk=11, window=1)),
                        ("window over every chunk -> chunk -> fm", dict(chunk=1, window=8)),
                        ("chunk 1 under a window stays windowed", dict(chunk=1))]
        for label, more in forwards:
            add(f"{label}: args NULL", ARG, args=None, **more)
            add(f"{label}: v NULL", ARG, v=None, **more)
            add(f"{label}: q_sb = 4", ARG, q_sb=4, **more)
            add(f"{label}: Lq != Lk", ARG, Lk=64, **more)
            add(f"{label}: the cross-attention layout", ARG, kv_pad_ones=2, **more)
            add(f"{label}: frames do not fit", ARG, frames=(16, 5), **more)
            add(f"{label}: frames NULL", ARG, frames=None, **more)
            add(f"{label}: more than 2^21 rows", UNSUPPORTED, L=BIG, frames=(0, 8), **more)
            add(f"{label}: o slice of 4 GiB", UNSUPPORTED, o_sl=1 << 26, **more)
            add(f"{label}: head dim 136", UNSUPPORTED, head_dim=136, **more)
            add(f"{label}: dk NULL, head dim 136", ARG if bwd else UNSUPPORTED, head_dim=136, dk=None, **more)
    if mask == "window":
        add("period < 1 -> chunk: its frames do not fit", ARG, frames=(16, 0))
        add("period < 1 -> chunk -> fm", ARG, frames=(16, -3), chunk=1)
    return rows


@pytest.mark.parametrize("name", list(ENTRIES))
def test_every_defect_gets_its_documented_code(lib, name):
    rows = table(name)
    assert len({label for label, _, _ in rows}) == len(rows) >= 40, "labels name the rows"
    got = [(label, call(lib, name, **defect), code) for label, defect, code in rows]
    wrong = [g for g in got if g[1] != g[2]]
    assert not wrong, f"{name}: (defect, returned, documented) {wrong}"


def test_the_table_reaches_every_entry_point():
    decl = [n for n in _lib.SIGNATURES if n.startswith("vds_attn_") and "fp8" not in n
            and n not in ("vds_attn_set_variant", "vds_attn_bwd_workspace_bytes")]
    assert sorted(decl) == sorted(ENTRIES) and len(ENTRIES) == 13


# vds_attn_bwd, called directly or reached through a NULL kv_lens / frames: non-positive lengths are VDS_ERR_ARG like in
# its twelve siblings, before anything is launched
BWD_LENGTHS = [dict(Lq=0), dict(Lq=-8), dict(Lk=0), dict(Lk=-8), dict(L=0), dict(Lq=0, head_dim=136), dict(Lk=-8, head_dim=12)]


@pytest.mark.parametrize("defect", BWD_LENGTHS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_bwd_refuses_non_positive_lengths(lib, defect):
    assert call(lib, "vds_attn_bwd", **defect) == ARG
    assert call(lib, "vds_attn_bwd_kvlen", kv_lens=None, **defect) == ARG
    assert call(lib, "vds_attn_bwd_causal", frames=None, **defect) == ARG
