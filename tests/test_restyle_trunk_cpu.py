"""CPU: the host side of restyling from a cached trunk plane (tgtc_geometry_trunk_bytes / tgtc_geometry_trunk /
tgtc_restyle_rays_trunk / tgtc_restyle_rays_trunk_folded, GeometryCache.trunk, RayRenderer.build_trunk / restyle(use_trunk=)):
exported symbols, the size function against its formula, the argument errors that are returned before a handle or a device is
touched, the GeometryCache file round trip with and without the plane, the precision check of restyle."""
import ctypes
import itertools
import os

import pytest
import torch

from test_restyle_cpu import _cpu_cache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tgtc_geometry_trunk_bytes", "tgtc_geometry_trunk", "tgtc_restyle_rays_trunk", "tgtc_restyle_rays_trunk_folded")
ERR_ARG, ERR_UNSUPPORTED = -1, -2
COUNTS = (-1, 0, 1, 127, 128, 129, 255, 256, 257, 3042525, (1 << 31) - 1)
TILE = 131072


def want_bytes(precision, count):
    """ceil(count / S) x 131072 with S = 128 for TGTC_PREC_FP16X3 (0) and 256 for TGTC_PREC_FP16 (1); 0 otherwise."""
    per_tile = {0: 128, 1: 256}.get(precision)
    if per_tile is None or count <= 0:
        return 0
    return -(-count // per_tile) * TILE


def test_trunk_symbols_exported_declared_and_registered():
    from tgtc_style_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tgtc_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in hip.header_symbols(), name           # registered in the binding table
        assert name + "(" in header, name
        assert len(getattr(hip.load(), name).argtypes) == {"tgtc_geometry_trunk_bytes": 2, "tgtc_geometry_trunk": 12}.get(name, 18)
    assert hip.load().tgtc_geometry_trunk_bytes.restype is ctypes.c_size_t
    assert hip.missing_symbols() == []


def test_trunk_bytes_is_the_documented_formula():
    from tgtc_style_amd import hip, rendering
    lib = hip.load()
    assert want_bytes(0, 129) == 2 * TILE and want_bytes(1, 257) == 2 * TILE and want_bytes(0, 3042525) == 23770 * TILE
    for precision, count in itertools.product((-1, 0, 1, 2, 3, 7), COUNTS):
        want = want_bytes(precision, count)
        assert lib.tgtc_geometry_trunk_bytes(precision, count) == want, (precision, count)
        assert rendering.GeometryCache.trunk_nbytes(precision, count) == want, (precision, count)
    for name, enum in hip.PRECISIONS.items():
        for count in COUNTS:
            assert rendering.GeometryCache.trunk_nbytes(name, count) == want_bytes(enum, count), (name, count)
    assert want_bytes(hip.PRECISIONS["fp16mx"], 1000) == 0


def test_calls_reject_bad_arguments_before_touching_a_device():
    """Null handles stand for handles here (no device): every rule that does not need a real handle is checked; the rest
    (handle kinds, the plane's size by the handle's precision, null buffers) is checked in tests/test_restyle_trunk_gpu.py."""
    from tgtc_style_amd import hip
    lib = hip.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)        # stands for any non-null pointer: the calls must return before they read through it
    err = lambda: lib.tgtc_last_error()
    big = 1 << 40

    def trunk(R=4, nc=64, nf=64, count=10):
        return lib.tgtc_geometry_trunk(None, p, p, R, nc, nf, p, big, count, p, big, None)
    assert trunk() == ERR_ARG and b"geometry_trunk: null handle" in err()
    assert trunk(R=-1) == ERR_ARG and trunk(count=-1) == ERR_ARG and b"bad argument" in err()
    assert trunk(nc=2) == ERR_ARG and trunk(nf=0) == ERR_ARG and b"n_fine >= 1" in err()
    assert trunk(count=4 * 128 + 1) == ERR_ARG and b"exceeds" in err()                 # count > R x N
    assert trunk(R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()                    # R x N >= 2^31
    assert trunk(R=0, count=0) == ERR_ARG and b"null handle" in err()                  # R == 0 is OK only behind a handle

    for call, who in ((lib.tgtc_restyle_rays_trunk, b"restyle_rays_trunk"),
                      (lib.tgtc_restyle_rays_trunk_folded, b"restyle_rays_trunk_folded")):
        def restyle(K=2, R=4, nc=64, nf=64, count=10):
            return call(None, p, p, p, K, R, nc, nf, p, big, count, p, big, p, big, p, p, None)
        assert restyle() == ERR_ARG and who + b": null handle" in err()
        for K in (0, -3):
            assert restyle(K=K) == ERR_ARG and b"K >= 1" in err()
        assert restyle(R=-1) == ERR_ARG and restyle(count=-1) == ERR_ARG and b"bad argument" in err()
        assert restyle(nc=2) == ERR_ARG and restyle(nf=0) == ERR_ARG and b"n_fine >= 1" in err()
        assert restyle(count=4 * 128 + 1) == ERR_ARG and b"exceeds" in err()
        assert restyle(R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()
        assert restyle(K=1 << 20, R=1 << 10, count=1 << 11) == ERR_UNSUPPORTED and b"K x count" in err()


def _plane(c, precision, short=0):
    from tgtc_style_amd.rendering import GeometryCache
    n = GeometryCache.trunk_nbytes(precision, c.count) - short
    return (torch.arange(n, dtype=torch.int64) * 37 % 251).to(torch.uint8)


@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
def test_geometry_cache_file_round_trip_with_and_without_the_plane(tmp_path, precision):
    from tgtc_style_amd.rendering import GeometryCache
    path = str(tmp_path / "cache.pt")
    plain = _cpu_cache()
    assert plain.trunk is None and plain.trunk_precision is None
    plain.save(path)
    keys_today = set(torch.load(path, map_location="cpu"))
    assert keys_today == {"buffer", "R", "N", "count", "min_weight", "key", "n_coarse", "n_fine"}

    c = _cpu_cache()
    c.attach_trunk(_plane(c, precision), precision)
    assert c.trunk.numel() == TILE and c.trunk_precision == precision       # 9 list entries: one tile
    # without the plane (the default): the dict a cache without one saves, and a cache without one comes back
    c.save(path)
    assert set(torch.load(path, map_location="cpu")) == keys_today
    d = GeometryCache.load(path, "cpu")
    assert d.trunk is None and d.trunk_precision is None and torch.equal(d.buffer, c.buffer)
    # with it
    c.save(path, with_trunk=True)
    assert set(torch.load(path, map_location="cpu")) == keys_today | {"trunk", "trunk_precision"}
    d = GeometryCache.load(path, "cpu")
    assert d.trunk_precision == precision and d.trunk.dtype == torch.uint8 and torch.equal(d.trunk, c.trunk)
    assert d.trunk.data_ptr() != c.trunk.data_ptr() and torch.equal(d.buffer, c.buffer)
    d.drop_trunk()
    assert d.trunk is None and d.trunk_precision is None
    with pytest.raises(ValueError):
        d.save(path, with_trunk=True)                                        # nothing to save
    # a plane whose size contradicts trunk_nbytes does not load, nor attach
    for short in (1, -1):
        raw = torch.load(path, map_location="cpu")
        raw["trunk"] = _plane(c, precision, short)
        torch.save(raw, path)
        with pytest.raises(ValueError):
            GeometryCache.load(path, "cpu")
        with pytest.raises(ValueError):
            c.attach_trunk(raw["trunk"], precision)
    raw["trunk"], raw["trunk_precision"] = _plane(c, precision), "fp16mx"     # no plane exists in that precision
    torch.save(raw, path)
    with pytest.raises(ValueError):
        GeometryCache.load(path, "cpu")


class _Packed:
    def __init__(self, precision):
        self.precision, self.handle = precision, None


class _Pair:
    """Stands for a style pair: restyle must refuse the plane before it asks for a device or a handle."""
    def __init__(self, precision):
        self._p = _Packed(precision)

    def packed(self):
        return self._p


def test_restyle_refuses_a_plane_of_another_precision_and_a_missing_plane():
    from tgtc_style_amd.rendering import RayRenderer
    c = _cpu_cache()
    ro = rd = torch.zeros(c.R, 3, dtype=torch.float64)
    zs = torch.zeros(1, c.R, 32)
    r = RayRenderer(None, None, _Pair("fp16x3"))
    with pytest.raises(ValueError, match="no trunk plane"):
        r.restyle(c, ro, rd, zs, use_trunk=True)
    c.attach_trunk(_plane(c, "fp16"), "fp16")
    for use in (None, True):
        with pytest.raises(ValueError, match="built in fp16, the style pair is packed in fp16x3"):
            r.restyle(c, ro, rd, zs, use_trunk=use)
    with pytest.raises(ValueError, match="built in fp16, the style pair is packed in fp16x3"):
        r.restyle(c, ro, rd, zs[0, :1].expand(1, 32))                        # the folded form as well
