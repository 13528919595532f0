"""No GPU: what the stashed two-phase fine pass (csrc/mlp_nerf_mx2_stash.hip) promises on paper -- the stash size
arithmetic, that the generators still write the committed instruction streams byte for byte (and the build's own
mx2_stash_asm_nerf.inc, which csrc/Makefile generates and git does not hold), and the heads stream's size."""
import contextlib
import io
import math
import os
import runpy
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
CSRC = os.path.join(ROOT, "tgtc-style_amd", "csrc")
REGIONS, SLOT = 1024, 932


def generated(tool, *argv):
    """what `python tools/<tool> <argv>` prints, run in this process"""
    old_argv, old_path = sys.argv, list(sys.path)
    sys.argv = [os.path.join(TOOLS, tool)] + list(argv)
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            runpy.run_path(sys.argv[0], run_name="__main__")
    finally:
        sys.argv, sys.path[:] = old_argv, old_path
    return out.getvalue()


@pytest.mark.parametrize("tool,argv,inc", [("gen_mx2_asm.py", (), "mx2_asm_nerf.inc"), ("gen_mx2_asm.py", ("stash",), "mx2_stash_asm_nerf.inc"),
                                           ("gen_x3_asm.py", (), "x3_asm_nerf.inc"), ("gen_mx_asm.py", ("nerf",), "mx_asm_nerf.inc")])
def test_generators_reproduce_the_committed_streams(tool, argv, inc):
    with open(os.path.join(CSRC, inc)) as fh:
        assert generated(tool, *argv) == fh.read()


def asm_body(text, name):
    i = text.index("mx2_asm_%s(" % name)
    j = text.index("asm volatile(", i)
    return text[j:text.index("        : ", j)]


def test_the_producers_stream_is_the_sigma_pass():
    """instruction for instruction: only the operand lists differ (layer 7's output leaves as outputs, not as clobbers)"""
    with open(os.path.join(CSRC, "mx2_asm_nerf.inc")) as fh:
        committed = fh.read()
    stash = generated("gen_mx2_asm.py", "stash")
    assert asm_body(stash, "nerf_sigma_stash_pass") == asm_body(committed, "nerf_sigma_pass")
    heads = asm_body(stash, "nerf_heads_pass")
    assert heads.count("v_mfma") == asm_body(committed, "nerf_full_pass").count("v_mfma") - asm_body(committed, "nerf_sigma_pass").count("v_mfma")


def test_heads_stream_units():
    sys.path.insert(0, TOOLS)
    try:
        from gen_mx_asm import NERF_SHAPES, Table
    finally:
        sys.path.remove(TOOLS)
    t, h = Table(NERF_SHAPES), Table(NERF_SHAPES[9:])
    full, sigma, heads = t.bytes_upto(t.first[12]) // 1024, t.bytes_upto(t.first[9]) // 1024, h.bytes_upto(h.n) // 1024
    assert heads == full - sigma == 368
    # and group by group, without the padding: REMAP 16 x 2 K groups, C0 8 x (2 K groups + 1 direction k-step pair), C1 one K group
    raw = lambda tab, n: sum(tab.size(q) for q in range(n))     # noqa: E731
    assert raw(h, h.n) == raw(t, t.n) - raw(t, t.first[9]) == (32 + 16 + 1) * 7168 + 8 * 2048
    assert h.n == t.first[12] - t.first[9] == 57
    assert "kMx2HeadsPadChunks = 24, kMx2HeadsUnits = 368;" in generated("gen_mx2_asm.py", "stash")


def want_bytes(R, nt, share, grid):
    n_pass = (R * nt + 127) // 128
    grid = min(n_pass, grid)
    per_wave = (n_pass + grid - 1) // grid * 32
    cap = max(1, math.ceil(min(share, 1.0) * per_wave))
    return REGIONS * ((SLOT * cap + 15) // 16 * 16)


def test_stash_bytes_arithmetic():
    from tgtc_style_amd import hip
    lib = hip.load()
    f = lib.tgtc_net_stash_bytes
    assert f(0, 192, 0.5) == 0 and f(-1, 192, 0.5) == 0 and f(10, 0, 0.5) == 0 and f(10, 192, -0.1) == 0
    assert f(1, 1, 0.0) == REGIONS * 944                      # one slot per region: the least set_stash takes
    # exactly representable shares (the entry takes a float); without a device the grid is the largest one, 256
    import torch
    grid = min(256, torch.cuda.get_device_properties(0).multi_processor_count) if torch.cuda.is_available() else 256
    for R, nt, share in [(1, 1, 1.0), (7, 16, 1.0), (200, 192, 1.0), (200, 192, 0.5), (200, 192, 0.125), (160000, 192, 0.125),
                         (160000, 192, 2.0), (37, 32, 0.25)]:
        assert f(R, nt, share) == want_bytes(R, nt, share, grid), (R, nt, share)
    # the headline frame at the share above which AUTO stops culling: about 4 GB
    got = f(160000, 192, 0.14)
    assert got == want_bytes(160000, 192, float.fromhex("0x1.1eb852p-3"), grid) and 3.9e9 < got < 4.1e9
