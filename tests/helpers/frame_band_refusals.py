"""Host-side refusals of vds_band_attn_fwd / _bwd, run as a program of its own in a process that sees NO GPU.

The calls pass made-up (well-aligned) device addresses, each with one defect that validate must refuse before any launch
-- VDS_ERR_ARG, or VDS_ERR_UNSUPPORTED, and VDS_ERR_ARG when a call has a defect of either kind.  Should a check ever be
lost, the call would go on to launch a kernel on those addresses -- so this never runs in a process with a visible device
(tests/helpers/lora_refusals.py states the arrangement): tests/test_frame_band_cpu.py starts it with every GPU hidden, and
it stops before its first call when torch still sees one.  A well-formed call then ends as VDS_ERR_LAUNCH, which the last
case pins: the refusals above it were refusals, not a library that rejects everything.

Prints one line per wrong result and exits 1 if there was any; exit 3: a device was visible, nothing was called."""
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

HIDE = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1"}
ARG, UNSUPPORTED, LAUNCH = -1, -2, -3


def main():
    import torch
    if torch.cuda.is_available():
        print("a GPU is visible to this process: refusing to call the entry points with made-up addresses")
        return 3
    from video_diffusion_speedrun_amd import _lib
    lib = _lib.load()

    def args(L=280, hd=64, Lk=None, pad=0, **kw):
        a = _lib.AttnArgs()
        a.B, a.H, a.Lq, a.Lk, a.head_dim = 2, 2, L, L if Lk is None else Lk, hd
        for i, n in enumerate(("q", "k", "v", "o", "d_o", "dq", "dk", "dv")):
            setattr(a, n, 0x100000 * (i + 1))
            s = "do" if n == "d_o" else n
            setattr(a, s + "_sl", hd)
            setattr(a, s + "_sh", L * hd)
            setattr(a, s + "_sb", 2 * L * hd)
        a.lse, a.delta = 0x900000, 0xa00000
        a.kv_pad_ones = pad
        a.ws_floats = 2 * 2 * 2 * L
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    big = 16 + 8 * (1 << 19)  # fits frames = (16, 8), and is past 2^21 rows
    # (what is wrong, expected code, AttnArgs keywords, frames or None, chunk, band_chunks)
    cases = [
        ("band_chunks < 0", ARG, {}, (16, 8), 1, -1),
        ("chunk < 1", ARG, {}, (16, 8), 0, 1),
        ("chunk < 0", ARG, {}, (16, 8), -3, 1),
        ("frames == NULL", ARG, {}, None, 1, 1),
        ("Lq != Lk", ARG, dict(Lk=281), (16, 8), 1, 1),
        ("kv_pad_ones == 2", ARG, dict(pad=2), (16, 8), 1, 1),
        ("frames do not fit: (L - lead) % period", ARG, {}, (16, 7), 1, 1),
        ("frames do not fit: lead > L", ARG, {}, (281, 1), 1, 1),
        ("frames do not fit: lead < 0", ARG, {}, (-8, 8), 1, 1),
        ("frames do not fit: period < 1", ARG, {}, (16, 0), 1, 1),
        ("q == NULL", ARG, dict(q=None), (16, 8), 1, 1),
        ("an odd stride", ARG, dict(k_sl=65), (16, 8), 1, 1),
        ("L > 2^21", UNSUPPORTED, dict(L=big), (16, 8), 1, 1),
        ("a head dim without an instance", UNSUPPORTED, dict(hd=256), (16, 8), 1, 1),
        ("L > 2^21 and band_chunks < 0: ARG first", ARG, dict(L=big), (16, 8), 1, -1),
        ("L > 2^21 and chunk < 1: ARG first", ARG, dict(L=big), (16, 8), 0, 0),
        ("no instance and band_chunks < 0: ARG first", ARG, dict(hd=256), (16, 8), 1, -2),
        ("no instance and frames == NULL: ARG first", ARG, dict(hd=256), None, 1, 0),
        ("no instance and Lq != Lk: ARG first", ARG, dict(hd=256, Lk=300), (16, 8), 1, 0),
        ("a well-formed call, no device", LAUNCH, {}, (16, 8), 1, 1),
        ("a well-formed call, lead = 0, short last chunk, a band of every pair", LAUNCH, dict(L=203), (0, 7), 3, 9),
    ]
    wrong, n = [], 0
    for what, want, kw, frames, chunk, band in cases:
        for name in ("vds_band_attn_fwd", "vds_band_attn_bwd"):
            fr = C.byref(_lib.ModGroups(*frames)) if frames is not None else None
            rc = getattr(lib, name)(C.byref(args(**kw)), fr, chunk, band, None)
            n += 1
            if rc != want:
                wrong.append(f"{name}({what}): returned {rc}, {want} expected")
    for line in wrong:
        print(line)
    print(f"{n} calls checked, {len(wrong)} wrong")
    return 1 if wrong else 0


if __name__ == "__main__":
    sys.exit(main())
