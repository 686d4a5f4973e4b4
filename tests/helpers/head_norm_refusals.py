"""Host-side refusals of vds_head_rmsnorm_fwd / _bwd, run as a program of its own in a process that sees NO GPU.

The calls pass made-up (well-aligned) device addresses, each with exactly one defect that the host-side checks must refuse
with VDS_ERR_ARG before any launch.  Should a check ever be lost, the call would go on to launch a kernel on those
addresses -- so this never runs in a process with a visible device: tests/test_head_norm_cpu.py starts it with the
device-visibility variables set to hide every GPU, and it stops before its first call when torch still sees one.  Then a
lost check ends as a launch error (VDS_ERR_LAUNCH) in this process, not as a kernel on wild pointers.

Prints one line per wrong result and exits 1 if there was any; exit 3: a device was visible, nothing was called."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

HIDE = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1"}


def main():
    import torch
    if torch.cuda.is_available():
        print("a GPU is visible to this process: refusing to call the entry points with made-up addresses")
        return 3
    from video_diffusion_speedrun_amd import _lib
    lib = _lib.load()
    p, q, o = 0x10000, 0x20000, 0x30000
    ok_fwd = dict(x=p, ldx=144, rstd=o, M=4, H=2, hd=72, eps=1e-6)
    ok_bwd = dict(dy=p, lddy=144, y=q, ldy=288, rstd=o, M=4, H=2, hd=72)

    def call_fwd(**kw):
        a = dict(ok_fwd, **kw)
        return lib.vds_head_rmsnorm_fwd(a["x"], a["ldx"], a["rstd"], a["M"], a["H"], a["hd"], a["eps"], None)

    def call_bwd(**kw):
        a = dict(ok_bwd, **kw)
        return lib.vds_head_rmsnorm_bwd(a["dy"], a["lddy"], a["y"], a["ldy"], a["rstd"], a["M"], a["H"], a["hd"], None)

    inf, nan = float("inf"), float("nan")
    bad_fwd = [dict(x=None), dict(rstd=None), dict(M=0), dict(M=-4), dict(H=0), dict(H=-1), dict(hd=0), dict(hd=-8),
               dict(hd=36, ldx=72), dict(hd=68, ldx=136), dict(hd=136, ldx=272), dict(ldx=148), dict(ldx=136), dict(ldx=0),
               dict(x=p + 8), dict(x=p + 2), dict(rstd=o + 2), dict(rstd=o + 1), dict(eps=0.0), dict(eps=-1e-6),
               dict(eps=inf), dict(eps=nan)]
    bad_bwd = [dict(dy=None), dict(y=None), dict(rstd=None), dict(M=0), dict(H=0), dict(hd=0), dict(hd=-72),
               dict(hd=36, lddy=72), dict(hd=136, lddy=272, ldy=272), dict(lddy=148), dict(lddy=136), dict(ldy=292),
               dict(ldy=136), dict(dy=p + 8), dict(y=q + 4), dict(rstd=o + 2)]
    wrong = []
    n = 0
    for name, call, cases in (("vds_head_rmsnorm_fwd", call_fwd, bad_fwd), ("vds_head_rmsnorm_bwd", call_bwd, bad_bwd)):
        for kw in cases:
            rc = call(**kw)
            msg = lib.vds_last_error() or b""
            n += 1
            if rc != -1:
                wrong.append(f"{name}{kw}: returned {rc}, VDS_ERR_ARG (-1) expected")
            elif not msg.startswith(name.encode()):  # every refusal leaves its own message: none is a stale one
                wrong.append(f"{name}{kw}: vds_last_error() = {msg!r} does not name the entry point")
    for call, kw, word in ((call_fwd, dict(hd=36, ldx=72), b"hd = 36"), (call_fwd, dict(ldx=136), b"row stride of x"),
                           (call_fwd, dict(eps=0.0), b"eps"), (call_fwd, dict(rstd=o + 2), b"rstd"),
                           (call_fwd, dict(x=p + 8), b"16-byte"), (call_fwd, dict(x=None), b"NULL"),
                           (call_bwd, dict(ldy=136), b"row stride of y"), (call_bwd, dict(M=0), b"M = 0"),
                           (call_bwd, dict(dy=p + 8), b"dy must be 16-byte")):
        if call(**kw) != -1 or word not in (lib.vds_last_error() or b""):
            wrong.append(f"{kw}: the message {lib.vds_last_error()!r} does not say {word!r}")
    for line in wrong:
        print(line)
    print(f"{n} refusals checked, {len(wrong)} wrong")
    return 1 if wrong else 0


if __name__ == "__main__":
    sys.exit(main())
