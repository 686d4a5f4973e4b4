#!/usr/bin/env python3
"""Records the decisions of the GEMM dispatcher of the commit BEFORE the check / plan / run split, for
tests/golden/gemm_plans.json.  That commit has no query entry, so its gemm.hip gets parent_plan_dump.patch (a dump of
__PRETTY_FUNCTION__ and the planning members of GemmP at the top of the three launch templates and of launch_split_det,
to stderr) on a scratch copy, is built, and this script runs the case list of tests/test_gemm_dispatch_cpu.py through
vds_gemm_bf16 / vds_gemm_bf16_grouped of that build on a machine WITHOUT a GPU: every call proceeds to its launch, dumps,
and returns VDS_ERR_LAUNCH.

    VDS_LIB_PATH=<the patched parent's libvds_hip.so> python profiles/gemm_dispatch/record_parent_plans.py OUT.json

Per call: the first dump line is the plan.  In deterministic mode a split-K call dumps launch_split_det first (the split
count asked for, before it is lowered to the workspace) and the launch after it, which names the tiling.  colsum is read
off the parent's code: fused (1) iff the launch has e_colsum, else a vds_colsum_bf16 pass (2) follows every call that
passes colsum."""
import ctypes as C
import json
import os
import re
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import test_gemm_dispatch_cpu as T  # noqa: E402
from video_diffusion_speedrun_amd import _lib  # noqa: E402

lib = C.CDLL(_lib.LIB_PATH)
lib.vds_knob_get.restype = C.c_double
lib.vds_knob_get.argtypes = [C.c_char_p]
lib.vds_knob_set.argtypes = [C.c_char_p, C.c_double]
lib.vds_set_deterministic.argtypes = [C.c_int32, C.c_void_p, C.c_size_t]
buf = C.create_string_buffer(4096 + 16)
ws = (C.addressof(buf) + 15) & ~15


def captured(fn):
    """fn() with file descriptor 2 redirected: (result, what it wrote)"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            r = fn()
            lib.fflush(None)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return r, tmp.read().decode()


plans = {}
for c in T.plan_cases():
    prev = {k: lib.vds_knob_get(k.encode()) for k in c["knobs"]}
    for k, v in c["knobs"].items():
        assert lib.vds_knob_set(k.encode(), float(v)) == 0
    lib.vds_gemm_force_tile(c["tile"])
    if c["det"]:
        assert lib.vds_set_deterministic(1, ws, 4096) >= 0
    g = c["groups"]
    a = T.args(c["layout"], c["epi"], c["M"], c["N"], c["K"], c["split_k"], c["colsum"], rpb=g[2] if g else 0)
    grp = C.byref(_lib.ModGroups(g[0], g[1])) if g else None
    rc, err = captured(lambda: lib.vds_gemm_bf16_grouped(C.byref(a), grp, None))
    lib.vds_set_deterministic(0, None, 0)
    lib.vds_gemm_force_tile(0)
    for k, v in prev.items():
        lib.vds_knob_set(k.encode(), v)
    lines = [ln for ln in err.splitlines() if ln.startswith("GEMMPLAN ")]
    assert rc == -3 and lines, (c["id"], rc, err)
    tiles_m, tiles_n, split_k, atomic, group_m, joint_xcd, narrow, fused = map(int, lines[0].split("|")[1].split())
    launch = next(ln for ln in lines if "launch_split_det" not in ln)
    tiling = 2 if "mid::launch" in launch else 256 if "big::launch" in launch else 128
    m = re.search(r"LAYOUT = (\d+), EPI = (\d+)", launch)
    assert (int(m.group(1)), int(m.group(2))) == (T.LAYOUTS[c["layout"]], 64 if g else T.EPILOGUES[c["epi"]]), (c["id"], launch)
    colsum = 0 if not c["colsum"] else 1 if fused else 2
    plans[c["id"]] = [tiling, tiles_m, tiles_n, split_k, atomic, group_m, joint_xcd, narrow, colsum]

with open(sys.argv[1], "w") as f:
    f.write('{"fields": %s,\n "plans": {\n' % json.dumps(T.FIELDS))
    f.write(",\n".join('  %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in plans.items()))
    f.write("\n }}\n")
print(len(plans), "plans")
