#!/usr/bin/env python3
"""Per-kernel listing of a gfx950 code object, and the comparison of two listings' sources.

    code_object_kernels.py OBJECT                 one line per kernel: name, code size, sha256 of its code bytes (symbol
                                                  address .. address + size), sha256 of its kernel descriptor (the entry
                                                  offset zeroed: it moves with the layout), and from the metadata note
                                                  VGPRs, AGPRs, SGPRs, static LDS, scratch, spills; waves/SIMD as the
                                                  unified register file allows (512 / VGPRs rounded up to 8, at most 8)
    code_object_kernels.py PARENT_OBJECT OBJECT   the verdict: kernels only in one of the two, kernels whose line differs

OBJECT is a code object (ELF) or the output of `hipcc --cuda-device-only -c` (an offload bundle: the gfx950 entry is
taken).  To prove a host-only change of a .hip file: build both commits' file with the Makefile's flags for it plus
--cuda-device-only, and compare.  Reads symbols and the metadata note through llvm-readelf, nothing else."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
          "vgpr_spill_count", "sgpr_spill_count")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(path, tmp):
    with open(path, "rb") as f:
        if f.read(24) != b"__CLANG_OFFLOAD_BUNDLE__":
            return path
    out = os.path.join(tmp, os.path.basename(path) + ".co")
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={path}",
        "--targets=hip-amdgcn-amd-amdhsa--gfx950", f"--output={out}")
    return out


def kernels(path):
    readelf = os.path.join(LLVM, "llvm-readelf")
    blob = open(path, "rb").read()
    sect = {}  # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S+\s+(?:PROGBITS)\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", run(readelf, "-SW", path), re.M):
        sect[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    sym = {}  # name -> bytes
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)$", run(readelf, "-sW", "--symbols", path), re.M):
        addr, size, ndx, name = int(m.group(1), 16), int(m.group(2)), int(m.group(4)), m.group(5)
        if ndx in sect:
            off = addr - sect[ndx][0] + sect[ndx][1]
            sym[name] = blob[off:off + size]
    meta, cur = {}, None
    for line in run(readelf, "--notes", path).splitlines():
        m = re.match(r"^  (- | {2})\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        cur[m.group(2)] = m.group(3).strip().strip("'")
        if m.group(2) == "name":
            meta[cur["name"]] = cur
    out = {}
    for name, md in meta.items():
        code, kd = sym[name], bytearray(sym[name + ".kd"])
        assert len(kd) == 64, name
        kd[16:24] = bytes(8)  # kernel_code_entry_byte_offset
        regs = int(md["vgpr_count"])
        waves = min(8, 512 // max(8, -(-regs // 8) * 8))
        res = " ".join(f"{k}={md.get(k, '0')}" for k in FIELDS)
        out[name] = f"{name} size={len(code)} code={hashlib.sha256(code).hexdigest()[:32]} " \
                    f"kd={hashlib.sha256(bytes(kd)).hexdigest()[:32]} {res} waves_per_simd={waves}"
    return out


def main(argv):
    if len(argv) not in (2, 3):
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        ks = [kernels(code_object(p, tmp)) for p in argv[1:]]
    if len(ks) == 1:
        print("\n".join(ks[0][n] for n in sorted(ks[0])))
        return 0
    a, b = ks
    gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    diff = sorted(n for n in set(a) & set(b) if a[n] != b[n])
    print(f"kernels: {len(a)} -> {len(b)}; in both: {len(set(a) & set(b))}, identical (code bytes, descriptor, resources): "
          f"{len(set(a) & set(b)) - len(diff)}")
    for title, names in (("only in the first", gone), ("only in the second", new), ("DIFFERENT", diff)):
        print(f"{title}: {len(names)}")
        for n in names:
            print("  " + n)
            if title == "DIFFERENT":
                print("    " + a[n] + "\n    " + b[n])
    return 1 if new or diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
