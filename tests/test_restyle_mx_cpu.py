"""CPU: the host side of the fp16mx restyle from a trunk plane (tgtc_style_enable_mx / tgtc_style_has_mx /
tgtc_restyle_rays_trunk_folded_mx, RayRenderer.restyle(style_precision=)): exported symbols, the argument errors that are returned
before a device is touched -- on null handles and on FAKE handles (zeroed memory whose first two words are the handle's kind
and precision: what the checks in front of the first device call read) -- and the ValueErrors of restyle.

The packer's round trip (K groups back to the equalised weights within the e2m3 grid's half step, P groups exactly) is in
tests/test_restyle_mx_gpu.py: a style handle is made by tgtc_style_create, which needs a device, and the packed streams live in
device memory (tgtc_style_mx_read copies them back)."""
import ctypes
import os

import pytest
import torch

from test_restyle_cpu import _cpu_cache
from test_restyle_trunk_cpu import _Pair, _plane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tgtc_style_enable_mx", "tgtc_style_has_mx", "tgtc_restyle_rays_trunk_folded_mx")
SEAM = "tgtc_style_mx_read"                  # declared and exported; a test seam, not part of the integration guide
ERR_ARG, ERR_UNSUPPORTED = -1, -2
KIND_NERF, KIND_STYLE = 0, 1
PREC_FP16X3, PREC_FP16 = 0, 1


def fake_handle(kind, precision):
    """Zeroed memory behind (kind, precision): no device allocation, no mx streams."""
    buf = (ctypes.c_int32 * 1024)()
    buf[0], buf[1] = kind, precision
    return buf


def test_mx_symbols_exported_declared_and_registered():
    from tgtc_style_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tgtc_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in hip.header_symbols(), name
        assert name + "(" in header, name
        assert name in integration, name
    assert hasattr(lib, SEAM) and SEAM in hip.header_symbols() and SEAM + "(" in header
    bound = hip.load()
    assert len(bound.tgtc_style_enable_mx.argtypes) == 2 and len(bound.tgtc_style_has_mx.argtypes) == 1
    # the sibling's arguments, one for one
    assert bound.tgtc_restyle_rays_trunk_folded_mx.argtypes == bound.tgtc_restyle_rays_trunk_folded.argtypes
    assert hip.missing_symbols() == []


def test_enable_and_has_mx_on_null_and_fake_handles():
    from tgtc_style_amd import hip
    lib = hip.load()
    err = lambda: lib.tgtc_last_error()
    assert lib.tgtc_style_has_mx(None) == 0
    assert lib.tgtc_style_enable_mx(None, None) == ERR_ARG and b"style_enable_mx: style must be a style handle" in err()
    nerf = fake_handle(KIND_NERF, PREC_FP16X3)
    assert lib.tgtc_style_enable_mx(ctypes.addressof(nerf), None) == ERR_ARG and b"style handle" in err()
    assert lib.tgtc_style_has_mx(ctypes.addressof(nerf)) == 0
    fast = fake_handle(KIND_STYLE, PREC_FP16)
    assert lib.tgtc_style_enable_mx(ctypes.addressof(fast), None) == ERR_UNSUPPORTED and b"TGTC_PREC_FP16X3" in err()
    assert lib.tgtc_style_has_mx(ctypes.addressof(fast)) == 0
    exact = fake_handle(KIND_STYLE, PREC_FP16X3)
    assert lib.tgtc_style_has_mx(ctypes.addressof(exact)) == 0
    # the read-back seam: nothing to read without the streams
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    assert lib.tgtc_style_mx_read(None, p, 64, p, 64, p, 16) == ERR_ARG and b"style_mx_read" in err()
    assert lib.tgtc_style_mx_read(ctypes.addressof(nerf), p, 64, p, 64, p, 16) == ERR_ARG
    assert lib.tgtc_style_mx_read(ctypes.addressof(exact), p, 64, p, 64, p, 16) == ERR_UNSUPPORTED and b"no fp16mx streams" in err()


def test_restyle_mx_rejects_bad_arguments_before_touching_a_device():
    from tgtc_style_amd import hip
    lib = hip.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)        # stands for any non-null pointer: the calls must return before they read through it
    err = lambda: lib.tgtc_last_error()
    big = 1 << 40
    who = b"restyle_rays_trunk_folded_mx"

    def restyle(style=None, K=2, R=4, nc=64, nf=64, count=10):
        return lib.tgtc_restyle_rays_trunk_folded_mx(style, p, p, p, K, R, nc, nf, p, big, count, p, big, p, big, p, p, None)
    assert restyle() == ERR_ARG and who + b": null handle" in err()
    for K in (0, -3):
        assert restyle(K=K) == ERR_ARG and b"K >= 1" in err()
    assert restyle(R=-1) == ERR_ARG and restyle(count=-1) == ERR_ARG and b"bad argument" in err()
    assert restyle(nc=2) == ERR_ARG and restyle(nf=0) == ERR_ARG and b"n_fine >= 1" in err()
    assert restyle(count=4 * 128 + 1) == ERR_ARG and b"exceeds" in err()
    assert restyle(R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()
    assert restyle(K=1 << 20, R=1 << 10, count=1 << 11) == ERR_UNSUPPORTED and b"K x count" in err()
    # the range checks come before the handle is looked at
    nerf, style = fake_handle(KIND_NERF, PREC_FP16X3), fake_handle(KIND_STYLE, PREC_FP16X3)
    assert restyle(style=ctypes.addressof(style), R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()
    assert restyle(style=ctypes.addressof(nerf)) == ERR_ARG and b"style must be a style handle" in err()
    # a style handle without mx streams: unsupported, also for R == 0 and count == 0 (the mode was never enabled)
    for kw in ({}, {"R": 0, "count": 0}, {"count": 0}):
        assert restyle(style=ctypes.addressof(style), **kw) == ERR_UNSUPPORTED, kw
        assert who + b": the style handle has no fp16mx streams" in err()
    # the sibling on the same fake handle gets past that point (R == 0 is OK behind a handle): the rule is the new entry's
    assert lib.tgtc_restyle_rays_trunk_folded(ctypes.addressof(style), p, p, p, 2, 0, 64, 64, p, big, 0, p, big, p, big, p, p, None) == 0


def test_restyle_refuses_the_mx_mode_without_its_preconditions():
    from tgtc_style_amd.rendering import RayRenderer
    c = _cpu_cache()
    ro = rd = torch.zeros(c.R, 3, dtype=torch.float64)
    z2, z3 = torch.zeros(2, 32), torch.zeros(2, c.R, 32)
    r = RayRenderer(None, None, _Pair("fp16x3"))
    with pytest.raises(ValueError, match="style_precision is None or 'fp16mx'"):
        r.restyle(c, ro, rd, z2, style_precision="fp16")
    with pytest.raises(ValueError, match="restyles from a trunk plane"):
        r.restyle(c, ro, rd, z2, style_precision="fp16mx")                       # no plane
    c.attach_trunk(_plane(c, "fp16x3"), "fp16x3")
    with pytest.raises(ValueError, match=r"zs \[K,32\]"):
        r.restyle(c, ro, rd, z3, style_precision="fp16mx")                       # per-ray latents
    with pytest.raises(ValueError, match="restyles from a trunk plane"):
        r.restyle(c, ro, rd, z2, use_trunk=False, style_precision="fp16mx")
    with pytest.raises(ValueError, match="fp16x3 style pair"):
        RayRenderer(None, None, _Pair("fp16")).restyle(c, ro, rd, z2, style_precision="fp16mx")
    c.attach_trunk(_plane(c, "fp16"), "fp16")
    with pytest.raises(ValueError, match="fp16x3 trunk plane"):
        r.restyle(c, ro, rd, z2, style_precision="fp16mx")                       # an fp16 plane
