"""Host-side refusals of the low-rank entry points, run as a program of its own in a process that sees NO GPU.

The calls pass made-up (well-aligned) device addresses, each with exactly one defect that the host-side checks must
refuse with VDS_ERR_ARG before any launch.  Should a check ever be lost, the call would go on to launch a kernel on
those addresses -- so this never runs in a process with a visible device: tests/test_lora_cpu.py starts it with the
device-visibility variables set to hide every GPU, and it stops before its first call when torch still sees one.  Then
a lost check ends as a launch error (VDS_ERR_LAUNCH) in this process, not as a kernel on wild pointers.

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
    down, up, wg = lib.vds_lowrank_down, lib.vds_lowrank_up_add, lib.vds_lowrank_wgrad
    ok_down = dict(x=p, ldx=32, w=q, ldw=32, lay=0, u=o, ldu=16, M=4, K=32, r=16)
    ok_up = dict(u=p, ldu=16, w=q, ldw=16, lay=0, y=o, ldy=32, M=4, N=32, r=16)
    ok_wg = dict(a=p, lda=32, u=q, ldu=16, g=o, ldg=16, lay=0, M=4, N=32, r=16, ws=0x40000, wsn=32 * 16)

    def call_down(**kw):
        a = dict(ok_down, **kw)
        return down(a["x"], a["ldx"], a["w"], a["ldw"], a["lay"], a["u"], a["ldu"], a["M"], a["K"], a["r"], 1.0, None)

    def call_up(**kw):
        a = dict(ok_up, **kw)
        return up(a["u"], a["ldu"], a["w"], a["ldw"], a["lay"], a["y"], a["ldy"], a["M"], a["N"], a["r"], 1.0, None)

    def call_wg(**kw):
        a = dict(ok_wg, **kw)
        return wg(a["a"], a["lda"], a["u"], a["ldu"], a["g"], a["ldg"], a["lay"], a["M"], a["N"], a["r"], 1.0, a["ws"],
                  a["wsn"], None)

    bad_down = [dict(x=None), dict(w=None), dict(u=None), dict(M=0), dict(K=0), dict(K=-8), dict(r=8), dict(r=24),
                dict(r=128), dict(lay=2), dict(K=36, ldx=40, ldw=40), dict(ldx=36), dict(ldw=36), dict(ldu=20),
                dict(ldx=24), dict(ldw=24), dict(ldu=8), dict(lay=1, ldw=8), dict(x=p + 2), dict(u=o + 8)]
    bad_up = [dict(u=None), dict(w=None), dict(y=None), dict(M=-1), dict(N=0), dict(r=0), dict(r=48), dict(lay=-1),
              dict(N=36, ldy=40), dict(ldu=20), dict(ldw=20), dict(ldy=36), dict(ldu=8), dict(ldw=8), dict(ldy=24),
              dict(lay=1, ldw=16), dict(y=o + 4)]
    bad_wg = [dict(a=None), dict(u=None), dict(g=None), dict(ws=None), dict(M=0), dict(N=0), dict(r=17), dict(lay=2),
              dict(N=36, lda=40), dict(lda=36), dict(ldu=12), dict(lda=24), dict(ldu=8), dict(ldg=8),
              dict(lay=1, ldg=16), dict(wsn=32 * 16 - 1), dict(M=2049, wsn=32 * 16), dict(ws=0x40004), dict(a=p + 8)]
    wrong = []
    n = 0
    for name, call, cases in (("vds_lowrank_down", call_down, bad_down), ("vds_lowrank_up_add", call_up, bad_up),
                              ("vds_lowrank_wgrad", call_wg, bad_wg)):
        for kw in cases:
            rc = call(**kw)
            msg = lib.vds_last_error() or b""
            n += 1
            if rc != -1:
                wrong.append(f"{name}{kw}: returned {rc}, VDS_ERR_ARG (-1) expected")
            elif not msg.startswith(name.encode()):  # every refusal leaves its own message: none is a stale one
                wrong.append(f"{name}{kw}: vds_last_error() = {msg!r} does not name the entry point")
    if call_wg(wsn=1) != -1 or b"workspace" not in lib.vds_last_error():
        wrong.append("vds_lowrank_wgrad(short workspace): no workspace message")
    if call_down(r=24) != -1 or b"r = 24" not in lib.vds_last_error():
        wrong.append("vds_lowrank_down(r=24): the message does not name the rank")
    for line in wrong:
        print(line)
    print(f"{n} refusals checked, {len(wrong)} wrong")
    return 1 if wrong else 0


if __name__ == "__main__":
    sys.exit(main())
