"""The host dispatch of the 21 row-kernel entry points without a GPU -- RMSNorm forward and backward, gate backward, the
column sums, qkv / RoPE forward, cache forms and backward: ONE table of defects -- NULL pointers, widths, strides and column
offsets off their alignment, group descriptions that do not fit, each form's own refusals, each forwarding rule -- run
through every entry point, and the return code each documents in include/vds.h (-1 VDS_ERR_ARG, -2 VDS_ERR_UNSUPPORTED; ARG
wins where both apply).  Every call carries a defect, so every call is refused on the host: the tensor pointers are the
value 16 and are never dereferenced, nothing is launched."""
import ctypes as C
import os

import pytest

from video_diffusion_speedrun_amd import _lib

ARG, UNSUPPORTED = -1, -2
P = 16  # a tensor pointer: never dereferenced

# ---- the arguments of each family, in the order of include/vds.h ------------------------------------------------------------
# `[...]` = taken by some forms only: groups (_grouped), eps (_norm_), frames (_fm)
RMS_FWD = "x ldx w mod ldmod shift_col scale_col y ldy rstd B L D eps [groups] stream"
RMS_FWD8 = "x ldx w mod ldmod shift_col scale_col q ldq fmt amax_in amax_part dq_out rstd B L D eps stream"
RMS_BWD = "dy lddy x ldx w mod ldmod shift_col scale_col rstd dres lddres dx lddx dmod dw B L D [groups] stream"
GATE = "dxn lddxn y ldy mod ldmod gate_col dy lddy dmod dbias B L D [groups] stream"
GATE8 = "dxn lddxn y ldy mod ldmod gate_col q ldq fmt amax_in amax_part dq_out dmod dbias B L D stream"
COLSUM = "x ldx out M N [rows_per_sample] [row_offset] stream"
QKV_FWD = "qkv cosb sinb v0 lam q k v B L H hd hdp [eps] [frames] stream"
QKV_CACHE = "qkv cosb sinb v0 lam q k v kv_sb kv_sh kv_sl lead past B L H hd hdp [eps] stream"
QKV_BWD = "dq dk dv cosb sinb qkv_raw v0 lam dv0_acc dlam dqkv mix add_dv0 B L H hd hdp [eps] [frames] stream"
QKV_BWD8 = "dq dk dv cosb sinb qkv_raw v0 lam dv0_acc dlam q ldq fmt amax_in amax_part dq_out mix add_dv0 B L H hd hdp stream"

# entry point -> (argument list, the optional arguments it takes, the traits that pick its rows of the table)
ENTRIES = {
    "vds_rmsnorm_mod_fwd": (RMS_FWD, (), {"rms_fwd"}),
    "vds_rmsnorm_mod_fwd_grouped": (RMS_FWD, ("groups",), {"rms_fwd", "grouped"}),
    "vds_rmsnorm_mod_fwd_fp8": (RMS_FWD8, (), {"rms_fwd", "fp8"}),
    "vds_rmsnorm_mod_bwd": (RMS_BWD, (), {"rms_bwd"}),
    "vds_rmsnorm_mod_bwd_grouped": (RMS_BWD, ("groups",), {"rms_bwd", "grouped"}),
    "vds_gate_bwd": (GATE, (), {"gate"}),
    "vds_gate_bwd_grouped": (GATE, ("groups",), {"gate", "grouped"}),
    "vds_gate_bwd_fp8": (GATE8, (), {"gate", "fp8"}),
    "vds_colsum_bf16": (COLSUM, (), {"colsum"}),
    "vds_colsum_bf16_rows": (COLSUM, ("rows_per_sample", "row_offset"), {"colsum", "rows"}),
    "vds_qkv_rope_fwd": (QKV_FWD, (), {"qkv_fwd"}),
    "vds_qkv_rope_norm_fwd": (QKV_FWD, ("eps",), {"qkv_fwd", "norm"}),
    "vds_qkv_rope_fwd_fm": (QKV_FWD, ("frames",), {"qkv_fwd", "fm"}),
    "vds_qkv_rope_norm_fwd_fm": (QKV_FWD, ("eps", "frames"), {"qkv_fwd", "norm", "fm"}),
    "vds_qkv_rope_fwd_cache": (QKV_CACHE, (), {"qkv_fwd", "cache"}),
    "vds_qkv_rope_norm_fwd_cache": (QKV_CACHE, ("eps",), {"qkv_fwd", "norm", "cache"}),
    "vds_qkv_rope_bwd": (QKV_BWD, (), {"qkv_bwd"}),
    "vds_qkv_rope_norm_bwd": (QKV_BWD, ("eps",), {"qkv_bwd", "norm"}),
    "vds_qkv_rope_bwd_fm": (QKV_BWD, ("frames",), {"qkv_bwd", "fm"}),
    "vds_qkv_rope_norm_bwd_fm": (QKV_BWD, ("eps", "frames"), {"qkv_bwd", "norm", "fm"}),
    "vds_qkv_rope_bwd_fp8": (QKV_BWD8, (), {"qkv_bwd", "fp8"}),
}

# A call that WOULD run: B 2, L 24, D 384 with a [B, 9 D] modulation table and groups (8, 4); H 2 heads of 72 columns in rows
# of 96, frames (8, 4); a cache of 40 rows with 8 rows of past.  Every optional tensor is given.
GOOD = dict(
    x=P, w=P, mod=P, y=P, rstd=P, dy=P, dres=P, dx=P, dmod=P, dw=P, dxn=P, dbias=P, out=P, q=P, amax_in=P, amax_part=P,
    dq_out=P, qkv=P, cosb=P, sinb=P, v0=P, lam=P, k=P, v=P, dq=P, dk=P, dv=P, qkv_raw=P, dv0_acc=P, dlam=P, dqkv=P,
    ldx=384, ldy=384, lddy=384, lddx=384, lddres=384, lddxn=384, ldq=384, ldmod=9 * 384, shift_col=0, scale_col=768,
    gate_col=1536, fmt=0, B=2, L=24, D=384, M=48, N=384, rows_per_sample=24, row_offset=8, eps=1e-6, groups=(8, 4),
    frames=(8, 4), H=2, hd=72, hdp=96, kv_sb=2 * 40 * 96, kv_sh=40 * 96, kv_sl=96, lead=8, past=8, mix=0, add_dv0=0,
    stream=None)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def names_of(name):
    spec, optional, _ = ENTRIES[name]
    return [a.strip("[]") for a in spec.split() if not a.startswith("[") or a.strip("[]") in optional]


def call(lib, name, **defect):
    """the entry point on the call GOOD describes with `defect` laid over it; groups / frames: (lead, period) or None"""
    names = names_of(name)
    assert set(defect) <= set(names), (name, sorted(set(defect) - set(names)))
    vals = dict(GOOD, **defect)
    if name == "vds_qkv_rope_bwd_fp8" and "ldq" not in defect:
        vals["ldq"] = 3 * vals["H"] * vals["hd"]  # the [B*L, 3D] result
    args = []
    for n in names:
        val = vals[n]
        if n in ("groups", "frames") and val is not None:
            val = C.byref(_lib.ModGroups(*val))
        args.append(val)
    assert len(args) == len(_lib.SIGNATURES[name]), name
    return getattr(lib, name)(*args)


MISFITS = ((8, 5), (-1, 4), (8, 0), (8, -4), (32, 4))  # (L - lead) % period, lead < 0, period < 1 (twice), lead > L
NON_POSITIVE = (0, -1)


def table(name):
    """(label, defect, documented return code) for one entry point"""
    names, traits = names_of(name), ENTRIES[name][2]
    fp8, grouped = "fp8" in traits, "grouped" in traits
    rows = []

    def add(label, code, **defect):
        rows.append((label, defect, code))

    def nulls(*ptrs):
        for p in ptrs:
            add(f"{p} NULL", ARG, **{p: None})

    def off(*pairs):
        for n, val in pairs:
            add(f"{n} = {val}", ARG, **{n: val})

    def sizes(*dims):  # non-positive sizes where the entry documents the refusal
        for n in dims:
            for val in NON_POSITIVE:
                add(f"{n} = {val}", ARG, **{n: val})

    def qout():  # the fp8 output: include/vds.h, "fp8-emitting forms"
        nulls("q", "amax_in")
        off(("ldq", 380), ("fmt", 2), ("fmt", -1))

    def groups_rows(bg_limit):
        for g in MISFITS:
            add(f"groups {g} do not fit", ARG, groups=g)
        add("groups do not fit, D = 2056", ARG, groups=(8, 5), D=2056)
        if bg_limit:  # the modulation rows are the backward kernels' grid y dimension
            add("B * G = 65536", ARG, B=8192, groups=(0, 7), L=28)
            add("B * G = 81920", ARG, B=16384)
        # groups == NULL forwards to the plain entry: its refusals
        add("groups NULL -> plain: mod NULL", ARG, groups=None, mod=None)
        add("groups NULL -> plain: D = 380", ARG, groups=None, D=380)
        add("groups NULL -> plain: D = 2056", UNSUPPORTED, groups=None, D=2056)
        add("groups NULL -> plain: B = 0", ARG, groups=None, B=0)
        add("groups NULL -> plain: L = -1", ARG, groups=None, L=-1)

    if "rms_fwd" in traits:
        nulls("x", "mod", "rstd")
        off(("D", 380), ("ldx", 380), ("ldmod", 9 * 384 + 2), ("shift_col", 2), ("scale_col", 770))
        if fp8:
            qout()
        else:
            nulls("y")
            off(("ldy", 380))
        sizes("B", "L")
        add("D = 2056: no instance", UNSUPPORTED, D=2056)
        add("D = 2056, x NULL", ARG, D=2056, x=None)
        add("D = 2056, shift_col = 2", ARG, D=2056, shift_col=2)
        if grouped:
            groups_rows(bg_limit=False)
    if "rms_bwd" in traits:
        nulls("dy", "x", "mod", "rstd", "dx", "dmod")
        off(("D", 380), ("lddy", 380), ("ldx", 380), ("lddx", 380))
        add("w without dw", ARG, dw=None)
        add("dres with lddres = 380", ARG, lddres=380)
        add("dres with lddres = 4", ARG, lddres=4)
        sizes("B", "L")
        add("D = 2056: no instance", UNSUPPORTED, D=2056)
        add("D = 2056, w without dw", ARG, D=2056, dw=None)
        add("D = 2056, dres with lddres = 380", ARG, D=2056, lddres=380)
        if grouped:
            groups_rows(bg_limit=True)
    if "gate" in traits:
        nulls("dxn", "y", "mod", "dmod")
        off(("D", 380), ("lddxn", 380), ("ldy", 380))
        if fp8:
            qout()
        else:
            nulls("dy")
            off(("lddy", 380))
        sizes("B", "L")
        add("D = 2056: no instance", UNSUPPORTED, D=2056)
        add("D = 2056, mod NULL", ARG, D=2056, mod=None)
        if grouped:
            groups_rows(bg_limit=True)
    if "colsum" in traits:
        nulls("x", "out")
        off(("N", 380), ("ldx", 380), ("N", 4))
        if "rows" in traits:
            off(("rows_per_sample", -1), ("row_offset", -1))
    if "qkv_fwd" in traits:
        nulls("qkv", "cosb", "sinb", "q", "k", "v")
        off(("hd", 70), ("hd", 4))
        add("hdp < hd", ARG, hdp=64)
        add("hdp = 98", ARG, hdp=98)
        add("v0 without lam", ARG, lam=None)
        add("pad wider than half the head", UNSUPPORTED, hd=8, hdp=16)
        add("pad wider than half the head, q NULL", ARG, hd=8, hdp=16, q=None)
        add("pad wider than half the head, v0 without lam", ARG, hd=8, hdp=16, lam=None)
    if "qkv_bwd" in traits:
        nulls("dq", "dk", "dv", "cosb", "sinb")
        off(("hd", 70), ("hd", 4))
        if fp8:
            qout()
            add("hdp = 76", UNSUPPORTED, hdp=76)
            add("H * hd = 2304", UNSUPPORTED, H=32, ldq=3 * 2304)
            add("ldq = 424 < 3 * H * hd", UNSUPPORTED, ldq=424)
            add("hdp = 76, dk NULL", ARG, hdp=76, dk=None)
            add("H * hd = 2304, mix = 3", ARG, H=32, ldq=3 * 2304, mix=3)
            add("ldq = 424, add_dv0 without dv0_acc", ARG, ldq=424, add_dv0=1, dv0_acc=None)
            add("ldq = 420", ARG, ldq=420)
        else:
            nulls("dqkv")
        for mix in (1, 2):
            for p in ("qkv_raw", "v0", "lam", "dlam"):
                add(f"mix = {mix}, {p} NULL", ARG, mix=mix, **{p: None})
        add("mix = 1, dv0_acc NULL", ARG, mix=1, dv0_acc=None)
        off(("mix", 3), ("mix", -1))
        add("add_dv0 without dv0_acc", ARG, add_dv0=1, dv0_acc=None)
        add("add_dv0 without dv0_acc, mix = 2", ARG, add_dv0=1, dv0_acc=None, mix=2)
    if "norm" in traits:
        for eps in (0.0, -1e-6, float("nan")):
            add(f"eps = {eps}", ARG, eps=eps)
        add("eps = 0, pad wider than half the head", ARG, eps=0.0, hd=8, hdp=16)
        if "qkv_bwd" in traits:
            add("qkv_raw NULL, mix = 0", ARG, qkv_raw=None)
    if "fm" in traits:
        add("frames NULL", ARG, frames=None)
        for g in MISFITS:
            add(f"frames {g} do not fit", ARG, frames=g)
        sizes("B", "L", "H")
        add("frames NULL, pad wider than half the head", ARG, frames=None, hd=8, hdp=16)
        add("frames do not fit, pad wider than half the head", ARG, frames=(8, 5), hd=8, hdp=16)
    if "cache" in traits:
        off(("kv_sb", 2 * 40 * 96 + 2), ("kv_sh", 40 * 96 + 1), ("kv_sl", 98))
        add("kv_sl = 92 < hdp", ARG, kv_sl=92)
        add("lead > L", ARG, lead=25)
        off(("lead", -1), ("past", -1), ("past", -(1 << 31)))
        sizes("B", "L", "H")
        add("past < 0, pad wider than half the head", ARG, past=-8, hd=8, hdp=16)
        add("kv_sl = 12 < hdp, pad wider than half the head", ARG, kv_sl=12, hd=8, hdp=16)
    for _, defect, _ in rows:
        assert set(defect) <= set(names), (name, defect)
    return rows


@pytest.mark.parametrize("name", list(ENTRIES))
def test_every_defect_gets_its_documented_code(lib, name):
    rows = table(name)
    assert len({label for label, _, _ in rows}) == len(rows) >= 5, "labels name the rows"
    got = [(label, call(lib, name, **defect), code) for label, defect, code in rows]
    wrong = [g for g in got if g[1] != g[2]]
    assert not wrong, f"{name}: (defect, returned, documented) {wrong}"


def test_the_table_reaches_every_entry_point():
    decl = [n for n in _lib.SIGNATURES
            if n.startswith(("vds_rmsnorm_mod_", "vds_gate_bwd", "vds_colsum_bf16", "vds_qkv_rope_")) and n != "vds_qkv_rope_fwd_fp8"]
    assert sorted(decl) == sorted(ENTRIES) and len(ENTRIES) == 21
    assert sum(len(table(n)) for n in ENTRIES) >= 400
