"""The defect table of vds_teacher_attn_fwd / vds_teacher_attn_bwd, in the style of tests/test_attn_dispatch_cpu.py: every row
carries a defect, so every call is refused on the host -- the tensor pointers are the value 16 and are never dereferenced,
nothing is launched.  Run as a program it prints the rows whose return code is not the documented one, as JSON (the test
starts it in a child process that is shown no GPU)."""
import ctypes as C
import json
import os
import sys

ARG, UNSUPPORTED = -1, -2
FWD_PTRS = ("q", "k", "v", "o", "lse")
BWD_PTRS = ("d_o", "dq", "dk", "dv", "delta")
FWD_STRIDES = {"q": 4, "k": 4, "v": 4, "o": 2}
BWD_STRIDES = {"do": 4, "dq": 2, "dk": 2, "dv": 2}
BIG = (1 << 21) + 8
ENTRIES = {"vds_teacher_attn_fwd": False, "vds_teacher_attn_bwd": True}


def call(_lib, lib, name, **defect):
    """the entry point on a call that WOULD run -- B 1, H 2, L 48, head dim 64, frames (16, 8): 4 clean + 4 noisy frames of 4
    rows, chunk 2 -- with `defect` laid over it: fields of vds_attn_args by name, `L` (Lq and Lk), `frames`, `chunk`, or
    `args=None`"""
    d = dict(defect)
    extra = {"frames": (16, 8), "chunk": 2}
    extra.update({k: d.pop(k) for k in list(d) if k in extra})
    a = _lib.AttnArgs()
    L = d.pop("L", 48)
    a.B, a.H, a.Lq, a.Lk, a.head_dim = 1, 2, L, L, 64
    for f in FWD_PTRS + BWD_PTRS:
        setattr(a, f, 16)
    for t in list(FWD_STRIDES) + list(BWD_STRIDES):
        setattr(a, t + "_sb", 2 * L * 64), setattr(a, t + "_sh", L * 64), setattr(a, t + "_sl", 64)
    ref = None if d.pop("args", a) is None else C.byref(a)
    for f, val in d.items():
        assert hasattr(a, f), f
        setattr(a, f, val)
    fr = None if extra["frames"] is None else C.byref(_lib.ModGroups(*extra["frames"]))
    return getattr(lib, name)(ref, fr, extra["chunk"], None)


def table(name):
    """(label, defect, documented return code)"""
    bwd = ENTRIES[name]
    rows = []

    def add(label, code, **defect):
        rows.append((label, defect, code))

    add("args NULL", ARG, args=None)
    for f in FWD_PTRS:
        add(f"{f} NULL", ARG, **{f: None})
    for f in BWD_PTRS:  # the forward call does not look at the gradient pointers: the head dim is what it refuses
        add(f"{f} NULL", ARG if bwd else UNSUPPORTED, head_dim=136, **{f: None})
    for f in ("Lq", "Lk"):
        for val in (0, -8):
            add(f"{f} = {val}", ARG, **{f: val})
    add("L = 0", ARG, L=0)
    for t, s in FWD_STRIDES.items():
        for ax in ("_sb", "_sh", "_sl"):
            add(f"{t}{ax} = {s}", ARG, **{t + ax: s})
    for t, s in BWD_STRIDES.items():
        for ax in ("_sb", "_sh", "_sl"):
            add(f"{t}{ax} = {s}", ARG if bwd else UNSUPPORTED, head_dim=136, **{t + ax: s})
    for hd in (0, 12, 136):
        add(f"head dim {hd}", UNSUPPORTED, head_dim=hd)
        add(f"head dim {hd}, q NULL", ARG, head_dim=hd, q=None)
    add("head dim 72, q_sl = 4", ARG, head_dim=72, q_sl=4)
    # ---- the mask's own refusals
    add("Lq != Lk", ARG, Lk=64)
    add("Lq != Lk, head dim 136", ARG, Lk=64, head_dim=136)
    add("the cross-attention layout", ARG, kv_pad_ones=2)
    for fr in ((16, 5), (-1, 8), (16, 0), (16, -8), (56, 8)):
        add(f"frames {fr} do not fit", ARG, frames=fr)
    for fr in ((16, 1), (0, 3), (13, 7), (16, 32 + 1)):
        add(f"an odd period {fr}", ARG, frames=fr, L=fr[0] + fr[1] * 8)
    add("an odd period, head dim 136", ARG, frames=(0, 3), head_dim=136)
    add("an odd period, more than 2^21 rows", ARG, L=3 * (1 << 20), frames=(0, 3))
    add("frames do not fit, head dim 136", ARG, frames=(16, 5), head_dim=136)
    add("more than 2^21 rows", UNSUPPORTED, L=BIG, frames=(0, 8))
    add("more than 2^21 rows, the cross-attention layout", ARG, L=BIG, frames=(0, 8), kv_pad_ones=2)
    add("more than 2^21 rows, frames do not fit", ARG, L=BIG, frames=(0, 14))
    add("more than 2^21 rows, k_sh = 4", ARG, L=BIG, frames=(0, 8), k_sh=4)
    add("frames NULL", ARG, frames=None)
    add("frames NULL, head dim 136", ARG, frames=None, head_dim=136)
    add("args NULL, frames NULL", ARG, args=None, frames=None)
    add("o slice of 4 GiB", UNSUPPORTED, o_sl=1 << 26)
    add("o slice of 4 GiB, Lq != Lk", ARG, o_sl=1 << 26, Lk=64)
    if bwd:
        add("d_o slice of 4 GiB", UNSUPPORTED, do_sl=1 << 26)
        add("d_o slice of 4 GiB, an odd period", ARG, do_sl=1 << 26, frames=(8, 5), L=48)
    for c in (0, -1, -(1 << 31)):
        add(f"chunk = {c}", ARG, chunk=c)
        add(f"chunk = {c}, head dim 136", ARG, chunk=c, head_dim=136)
        add(f"chunk = {c}, args NULL", ARG, chunk=c, args=None)
    # ---- nothing is forwarded: chunk 1 and a chunk past the half stay teacher calls, with the teacher's refusals
    for label, more in (("chunk 1", dict(chunk=1)), ("chunk past the half", dict(chunk=9))):
        add(f"{label}: an odd period", ARG, frames=(0, 3), **more)
        add(f"{label}: v NULL", ARG, v=None, **more)
        add(f"{label}: head dim 136", UNSUPPORTED, head_dim=136, **more)
        add(f"{label}: more than 2^21 rows", UNSUPPORTED, L=BIG, frames=(0, 8), **more)
    return rows


def wrong_rows(_lib, lib):
    out = []
    for name in ENTRIES:
        rows = table(name)
        assert len({label for label, _, _ in rows}) == len(rows) >= 40, "labels name the rows"
        for label, defect, code in rows:
            got = call(_lib, lib, name, **defect)
            if got != code:
                out.append([name, label, got, code])
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from video_diffusion_speedrun_amd import _lib as L_
    print(json.dumps({"rows": sum(len(table(n)) for n in ENTRIES), "wrong": wrong_rows(L_, L_.load())}))
