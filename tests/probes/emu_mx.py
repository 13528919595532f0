#!/usr/bin/env python3
"""CPU emulation of the fp16+fp6 arithmetic (mlp_mx.h) on the synthetic NeRF: what error does the scheme itself leave?
The model lives in tests/nerf_kernel_cases.py (the plain per-sample sweep holds the fp16mx kernels against it); this script
prints its four modes on M = 1 000 points."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from nerf_kernel_cases import MODES, blocks, e2m3, mx_linear, probe_errors, run, split_act, split_w  # noqa: F401 (re-exported)

if __name__ == "__main__":
    errs = probe_errors()
    for name, _ in MODES:
        print("%-24s sigma %.2e  remap %.2e  rgb %.2e" % ((name,) + errs[name]))
