#!/usr/bin/env python3
"""tests/test_gemm_dispatch_cpu.py against a build of the commit before vds_gemm_plan existed:
    VDS_LIB_PATH=<the parent's libvds_hip.so> python profiles/gemm_dispatch/run_cpu_test_on_parent.py
The ctypes table must not ask that build for the new entry; the test file then skips its plan rows by itself."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from video_diffusion_speedrun_amd import _lib  # noqa: E402

_lib.SIGNATURES.pop("vds_gemm_plan")
TEST = os.path.join(REPO, "tests", "test_gemm_dispatch_cpu.py")
sys.exit(pytest.main([TEST, "-q", "-rfs", "--tb=line", "-p", "no:cacheprovider"]))
