"""CPU: the host side of the trunk plane from an fp16mx fine network (tgtc_geometry_trunk_mx, tgtc_geometry_trunk_read,
GeometryCache.trunk_source, RayRenderer.build_trunk(trunk_precision=)): exported symbols, the argument errors that are returned
before a device is touched -- on null handles and on fake handles (zeroed memory behind the handle's kind and precision, what
the checks in front of the first device call read) --, the `source` rules of attach_trunk, trunk_source through save / load,
the ValueErrors of build_trunk, and the exactness of the ray grid the GPU bit test relies on."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from test_restyle_cpu import _cpu_cache
from test_restyle_mx_cpu import fake_handle
from test_restyle_trunk_cpu import _Pair, _plane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tgtc_geometry_trunk_mx", "tgtc_geometry_trunk_read")
ERR_ARG, ERR_UNSUPPORTED = -1, -2
KIND_NERF, KIND_STYLE = 0, 1
PREC_FP16X3, PREC_FP16, PREC_FP16_FP6 = 0, 1, 2
TILE = 131072


def test_trunk_mx_symbols_exported_declared_and_registered():
    from tgtc_style_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tgtc_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in hip.header_symbols(), name
        assert name + "(" in header, name
    assert "tgtc_geometry_trunk_mx" in integration
    bound = hip.load()
    assert bound.tgtc_geometry_trunk_mx.argtypes == bound.tgtc_geometry_trunk.argtypes      # the sibling's arguments, one for one
    assert len(bound.tgtc_geometry_trunk_read.argtypes) == 7
    assert hip.missing_symbols() == []


def test_trunk_mx_rejects_bad_arguments_before_touching_a_device():
    from tgtc_style_amd import hip
    lib = hip.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)        # stands for any non-null pointer: the calls must return before they read through it
    err = lambda: lib.tgtc_last_error()
    big = 1 << 40

    def trunk(fine=None, R=4, nc=64, nf=64, count=10, cache=p, cache_bytes=big, plane=p, plane_bytes=big):
        return lib.tgtc_geometry_trunk_mx(fine, p, p, R, nc, nf, cache, cache_bytes, count, plane, plane_bytes, None)
    assert trunk() == ERR_ARG and b"geometry_trunk_mx: null handle" in err()
    assert trunk(R=-1) == ERR_ARG and trunk(count=-1) == ERR_ARG and b"bad argument" in err()
    assert trunk(nc=2) == ERR_ARG and trunk(nf=0) == ERR_ARG and b"n_fine >= 1" in err()
    assert trunk(count=4 * 128 + 1) == ERR_ARG and b"exceeds" in err()                 # count > R x N
    assert trunk(R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()                    # R x N >= 2^31
    assert trunk(R=0, count=0) == ERR_ARG and b"null handle" in err()                  # R == 0 is OK only behind a handle
    # the range checks come before the handle is looked at; then its kind, then its precision
    mx, x3 = fake_handle(KIND_NERF, PREC_FP16_FP6), fake_handle(KIND_NERF, PREC_FP16X3)
    fast, style = fake_handle(KIND_NERF, PREC_FP16), fake_handle(KIND_STYLE, PREC_FP16X3)
    a = ctypes.addressof
    assert trunk(fine=a(x3), R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()
    assert trunk(fine=a(style)) == ERR_ARG and b"fine must be a NeRF handle" in err()
    for h in (x3, fast):
        assert trunk(fine=a(h)) == ERR_UNSUPPORTED and b"tgtc_geometry_trunk takes" in err()
        assert trunk(fine=a(h), R=0, count=0) == ERR_UNSUPPORTED                       # the handle is never this entry's
    # an fp16mx handle: R == 0 and count == 0 return without a launch; sizes are the fp16x3 plane's
    assert trunk(fine=a(mx), R=0, count=0) == 0 and trunk(fine=a(mx), count=0) == 0
    assert trunk(fine=a(mx), count=0, plane=None, plane_bytes=0) == 0
    assert trunk(fine=a(mx), plane=None) == ERR_ARG and trunk(fine=a(mx), cache=None) == ERR_ARG and b"null pointer" in err()
    assert trunk(fine=a(mx), cache_bytes=100) == ERR_ARG and b"cache of 100 bytes" in err()
    assert trunk(fine=a(mx), plane_bytes=TILE - 1) == ERR_ARG and b"plane of 131071 bytes, need 131072" in err()
    assert trunk(fine=a(mx), R=64, count=129, plane_bytes=2 * TILE - 1) == ERR_ARG and b"need 262144" in err()
    # today's entry keeps refusing that handle, and no plane size exists for its precision
    assert lib.tgtc_geometry_trunk(a(mx), p, p, 4, 64, 64, p, big, 10, p, big, None) == ERR_UNSUPPORTED
    assert b"fp16x3 and fp16 handles only" in err() and lib.tgtc_geometry_trunk_bytes(PREC_FP16_FP6, 1000) == 0


def test_trunk_read_rejects_bad_arguments_before_touching_a_device():
    from tgtc_style_amd import hip
    lib = hip.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    err = lambda: lib.tgtc_last_error()

    def read(precision=PREC_FP16X3, plane=p, nbytes=1 << 40, count=10, hi=p, lo=p):
        return lib.tgtc_geometry_trunk_read(precision, plane, nbytes, count, hi, lo, None)
    assert read(count=-1) == ERR_ARG and b"geometry_trunk_read: bad argument" in err()
    for precision in (-1, PREC_FP16_FP6, 3):
        assert read(precision=precision) == ERR_ARG and b"fp16x3 and fp16 only" in err()
    assert read(count=1 << 31) == ERR_UNSUPPORTED and b"2^31" in err()
    assert read(count=0) == 0 and read(count=0, plane=None, hi=None, lo=None, nbytes=0) == 0
    assert read(plane=None) == ERR_ARG and read(hi=None) == ERR_ARG and b"null pointer" in err()
    assert read(nbytes=TILE - 1) == ERR_ARG and b"need 131072" in err()
    assert read(count=129, nbytes=2 * TILE - 1) == ERR_ARG and b"need 262144" in err()
    assert read(precision=PREC_FP16, count=257, nbytes=2 * TILE - 1) == ERR_ARG and b"need 262144" in err()


def test_attach_trunk_source_rules():
    c = _cpu_cache()
    assert c.trunk is None and c.trunk_precision is None and c.trunk_source is None
    for precision in ("fp16x3", "fp16"):
        c.attach_trunk(_plane(c, precision), precision)
        assert c.trunk_precision == precision and c.trunk_source == precision            # the default: the plane's own precision
        c.attach_trunk(_plane(c, precision), precision, source=precision)
        assert c.trunk_source == precision
    c.attach_trunk(_plane(c, "fp16x3"), "fp16x3", source="fp16mx")
    assert c.trunk_precision == "fp16x3" and c.trunk_source == "fp16mx"
    kept = c.trunk
    for precision, source in (("fp16", "fp16mx"), ("fp16", "fp16x3"), ("fp16x3", "fp16"), ("fp16x3", "fp32"), ("fp16x3", 2)):
        with pytest.raises(ValueError):
            c.attach_trunk(_plane(c, precision), precision, source=source)
    with pytest.raises(ValueError):
        c.attach_trunk(_plane(c, "fp16x3"), "fp16mx")                                    # still no plane in that layout
    with pytest.raises(ValueError):
        c.attach_trunk(_plane(c, "fp16x3"), "fp16mx", source="fp16mx")
    assert c.trunk is kept and c.trunk_source == "fp16mx"                                # a refused plane changes nothing
    c.drop_trunk()
    assert c.trunk is None and c.trunk_precision is None and c.trunk_source is None


def test_trunk_source_through_save_and_load(tmp_path):
    from tgtc_style_amd.rendering import GeometryCache
    path = str(tmp_path / "cache.pt")
    c = _cpu_cache()
    c.attach_trunk(_plane(c, "fp16x3"), "fp16x3", source="fp16mx")
    c.save(path, with_trunk=True)
    raw = torch.load(path, map_location="cpu")
    assert raw["trunk_source"] == "fp16mx" and raw["trunk_precision"] == "fp16x3"
    d = GeometryCache.load(path, "cpu")
    assert d.trunk_source == "fp16mx" and d.trunk_precision == "fp16x3" and torch.equal(d.trunk, c.trunk)
    # a file without the key: the plane came from a handle of its own precision
    del raw["trunk_source"]
    torch.save(raw, path)
    d = GeometryCache.load(path, "cpu")
    assert d.trunk_source == "fp16x3" and d.trunk_precision == "fp16x3"
    d.save(path, with_trunk=True)
    assert GeometryCache.load(path, "cpu").trunk_source == "fp16x3"
    # a source that contradicts the layout does not load
    raw["trunk_source"] = "fp16"
    torch.save(raw, path)
    with pytest.raises(ValueError):
        GeometryCache.load(path, "cpu")
    # saved without the plane: no trace of it
    c.save(path)
    d = GeometryCache.load(path, "cpu")
    assert "trunk_source" not in torch.load(path, map_location="cpu") and d.trunk is None and d.trunk_source is None


def test_build_trunk_refuses_what_does_not_exist_before_any_launch():
    from tgtc_style_amd.rendering import RayRenderer
    c = _cpu_cache()
    ro = rd = torch.zeros(c.R, 3, dtype=torch.float64)
    for fine, asked in (("fp16mx", "fp16"), ("fp16mx", "fp16mx"), ("fp16x3", "fp16"), ("fp16x3", "fp16mx"), ("fp16", "fp16"),
                        ("fp16", "fp16x3"), ("fp16", "fp16mx"), ("fp16mx", 0)):
        with pytest.raises(ValueError, match="trunk_precision is None"):
            RayRenderer(None, _Pair(fine), _Pair("fp16x3")).build_trunk(c, ro, rd, trunk_precision=asked)
        assert c.trunk is None and c.trunk_source is None
    # what exists gets past that check: the next refusal is the device's (CPU tensors here)
    for fine in ("fp16mx", "fp16x3"):
        with pytest.raises(RuntimeError):
            RayRenderer(None, _Pair(fine), _Pair("fp16x3")).build_trunk(c, ro, rd, trunk_precision="fp16x3")
    with pytest.raises(RuntimeError):
        RayRenderer(None, _Pair("fp16mx"), _Pair("fp16x3")).build_trunk(c, ro, rd)
    assert c.trunk is None


# ------------------------------------------------------------------------------------------------------- the exact grid
def exact_rays(R, N, seed=97):
    """Rays whose o + t d is the same float64 however it is fused: origins multiples of 2^-10 in [-1, 1] (z = -1), directions
    multiples of 2^-8 in [-0.3, 0.3] (z = 2), depths multiples of 2^-16 in (0, 1), float32, sorted per ray.  A product is a
    multiple of 2^-24 below 2, a sum one below 4: at most 26 significant bits.  -> (ro [R,3], rd [R,3] float64, ts [R,N] float32)"""
    rng = np.random.default_rng(seed)
    ro = np.concatenate([rng.integers(-1024, 1025, (R, 2)) / 1024.0, -np.ones((R, 1))], 1)
    rd = np.concatenate([rng.integers(-76, 77, (R, 2)) / 256.0, 2 * np.ones((R, 1))], 1)
    ts = np.sort(rng.integers(1, 65536, (R, N)) / 65536.0, -1).astype(np.float32)
    return torch.from_numpy(ro), torch.from_numpy(rd), torch.from_numpy(ts)


def test_exact_grid_is_exact():
    R, N = 40, 129
    ro, rd, ts = exact_rays(R, N)
    assert ro.dtype == rd.dtype == torch.float64 and ts.dtype == torch.float32
    assert bool((ts[:, 1:] >= ts[:, :-1]).all()) and 0 < float(ts.min()) and float(ts.max()) < 1
    assert torch.equal(ro * 1024, (ro * 1024).round()) and torch.equal(rd * 256, (rd * 256).round())
    assert torch.equal(ts.double() * 65536, (ts.double() * 65536).round())
    got = ro[:, None, :] + ts[..., None].double() * rd[:, None, :]                      # float64, rounded twice if at all
    fused = torch.addcmul(ro[:, None, :].expand(R, N, 3), ts[..., None].double().expand(R, N, 3), rd[:, None, :].expand(R, N, 3))
    assert torch.equal(got, fused)
    o, d, t, g = ro.tolist(), rd.tolist(), ts.double().tolist(), got.tolist()
    for r in range(R):
        fo, fd = [Fraction(x) for x in o[r]], [Fraction(x) for x in d[r]]
        for s in range(N):
            ft = Fraction(t[r][s])
            assert all(Fraction(g[r][s][k]) == fo[k] + ft * fd[k] for k in range(3)), (r, s)
    assert float(got.abs().max()) < 4
