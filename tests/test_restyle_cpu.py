"""CPU: the host side of restyling rays from a cached geometry (tgtc_geometry_build / tgtc_geometry_pack / tgtc_restyle_rays):
exported symbols, the two size functions against the documented layouts, argument errors that are returned before a device
is touched, the GeometryCache file round trip, the --geometry_cache option."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from tgtc_style_amd import config as cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tgtc_geometry_build", "tgtc_geometry_cache_bytes", "tgtc_geometry_pack", "tgtc_restyle_workspace_bytes",
         "tgtc_restyle_rays")
ERR_ARG, ERR_UNSUPPORTED = -1, -2


def up(nbytes):
    return (nbytes + 255) // 256 * 256


def test_restyle_symbols_exported_and_declared():
    from tgtc_style_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tgtc_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in hip.header_symbols(), name
        assert name + "(" in header, name
    assert hip.load().tgtc_geometry_cache_bytes.restype is ctypes.c_size_t
    assert hip.load().tgtc_restyle_workspace_bytes.restype is ctypes.c_size_t
    assert hip.missing_symbols() == []


def test_size_functions_are_the_documented_layouts():
    """Cache: a 256-byte header, t float [R], ray_start uint32 [R+1], live / ts_live / w_live [count], each plane rounded up to
    256 bytes.  Restyle workspace: rgb_live float [K,count,3] rounded up to 256.  0 for negative arguments (K < 1)."""
    from tgtc_style_amd import hip, rendering
    lib = hip.load()
    for R, count in itertools.product((-1, 0, 1, 63, 64, 300, 160000, 1 << 24), (-1, 0, 1, 64, 65, 5703, 3041280, (1 << 31) - 1)):
        want = 0 if R < 0 or count < 0 else 256 + up(4 * R) + up(4 * (R + 1)) + 3 * up(4 * count)
        assert lib.tgtc_geometry_cache_bytes(R, count) == want, (R, count)
        if want:
            assert rendering.GeometryCache.nbytes(R, count) == want, (R, count)
    for count, K in itertools.product((-1, 0, 1, 21, 22, 5703, 3041280, (1 << 29)), (-1, 0, 1, 2, 3, 4)):
        want = 0 if count < 0 or K < 1 else up(12 * K * count)
        assert lib.tgtc_restyle_workspace_bytes(count, K) == want, (count, K)


def test_calls_reject_bad_arguments_before_touching_a_device():
    """Null handles stand for handles here (no device): every rule that does not need a real handle is checked; the rest
    (handle kinds, precisions, buffer sizes) is checked on the device in tests/test_restyle_gpu.py."""
    from tgtc_style_amd import hip
    lib = hip.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)        # stands for any non-null pointer: the calls must return before they read through it
    err = lambda: lib.tgtc_last_error()

    def build(min_weight=0., R=4):
        return lib.tgtc_geometry_build(None, None, p, p, R, 64, 64, 0., 1., None, min_weight, p, 4096, p, p, None)
    assert build() == ERR_ARG and b"geometry_build" in err()                        # null handles
    assert build(R=-1) == ERR_ARG
    assert build(min_weight=-1.) == ERR_ARG and b"min_weight" in err()
    assert build(min_weight=float("nan")) == ERR_ARG and b"min_weight" in err()

    def pack(ws=p, R=4, nc=64, nf=64, min_weight=0., count=10, cache=p, cache_bytes=1 << 40):
        return lib.tgtc_geometry_pack(ws, R, nc, nf, min_weight, count, cache, cache_bytes, None)
    assert pack(ws=None) == ERR_ARG and pack(cache=None) == ERR_ARG and b"null pointer" in err()
    assert pack(R=-1) == ERR_ARG and pack(count=-1) == ERR_ARG
    assert pack(nc=2) == ERR_ARG and pack(nf=0) == ERR_ARG and b"n_fine >= 1" in err()
    assert pack(min_weight=-1e-6) == ERR_ARG and pack(min_weight=float("nan")) == ERR_ARG and b"min_weight" in err()
    assert pack(count=4 * 128 + 1) == ERR_ARG and b"exceeds" in err()                # count > R x N
    assert pack(cache_bytes=lib.tgtc_geometry_cache_bytes(4, 10) - 1) == ERR_ARG and b"need" in err()
    assert pack(R=1 << 24) == ERR_UNSUPPORTED and b"2^31" in err()                   # R x N >= 2^31

    def restyle(K=2, R=4, count=10):
        return lib.tgtc_restyle_rays(None, None, p, p, p, K, R, 64, 64, p, 1 << 40, count, p, 1 << 40, p, p, None)
    assert restyle() == ERR_ARG and b"restyle_rays" in err()                         # null handles
    for K in (0, -3):
        assert restyle(K=K) == ERR_ARG and b"K >= 1" in err()
    assert restyle(R=-1) == ERR_ARG and restyle(count=-1) == ERR_ARG


def _cpu_cache(R=5, N=7, count=9, key="k1"):
    from tgtc_style_amd.rendering import GeometryCache
    rng = np.random.default_rng(3)
    buf = torch.zeros(GeometryCache.nbytes(R, count), dtype=torch.uint8)
    c = GeometryCache(buf, R, N, count, 1e-3, key, 3, 4)
    live = np.sort(rng.choice(R * N, count, replace=False)).astype(np.int32)
    c.header[:7] = torch.tensor([GeometryCache.MAGIC, GeometryCache.VERSION, R, 0, N, count,
                                 int(np.float32(1e-3).view(np.int32))], dtype=torch.int32)
    c.t[:] = torch.from_numpy(rng.uniform(0, 1, R).astype(np.float32))
    c.live[:] = torch.from_numpy(live)
    c.ray_start[:] = torch.from_numpy(np.searchsorted(live, np.arange(R + 1) * N).astype(np.int32))
    c.ts_live[:] = torch.from_numpy(rng.uniform(0, 1, count).astype(np.float32))
    c.w_live[:] = torch.from_numpy(rng.uniform(0, 1, count).astype(np.float32))
    return c


def test_geometry_cache_views_and_file_round_trip(tmp_path):
    from tgtc_style_amd.rendering import GeometryCache
    c = _cpu_cache()
    # the typed views are the documented planes of the one buffer
    off = 256
    for name, words in (("t", 5), ("ray_start", 6), ("live", 9), ("ts_live", 9), ("w_live", 9)):
        v = getattr(c, name)
        assert v.shape == (words,) and v.data_ptr() == c.buffer.data_ptr() + off, name
        off += up(4 * words)
    assert off == c.buffer.numel()
    path = str(tmp_path / "cache.pt")
    c.save(path)
    d = GeometryCache.load(path, "cpu")
    assert torch.equal(d.buffer, c.buffer) and d.buffer.data_ptr() != c.buffer.data_ptr()
    assert (d.R, d.N, d.count, d.key, d.n_coarse, d.n_fine) == (5, 7, 9, "k1", 3, 4)
    assert d.min_weight == float(np.float32(1e-3)) or d.min_weight == 1e-3
    assert torch.equal(d.live, c.live) and torch.equal(d.w_live, c.w_live) and int(d.ray_start[-1]) == 9
    # a buffer that contradicts its metadata, or a list that leaves the sample range, does not load
    bad = _cpu_cache()
    bad.header[4] = 8
    bad.save(path)
    with pytest.raises(ValueError):
        GeometryCache.load(path, "cpu")
    bad = _cpu_cache()
    bad.live[-1] = 5 * 7
    bad.save(path)
    with pytest.raises(ValueError):
        GeometryCache.load(path, "cpu")
    with pytest.raises(ValueError):
        GeometryCache(torch.zeros(GeometryCache.nbytes(5, 9) - 1, dtype=torch.uint8), 5, 7, 9, 0.)


def test_cli_geometry_cache_needs_share_geometry(tmp_path):
    from tgtc_style_amd import train_tgtcs
    base = ["--config", os.path.join(ROOT, "configs", "fern.txt")]
    assert cfg.parse_args(base).geometry_cache == ""
    a = cfg.parse_args(base + ["--share_geometry", "--geometry_cache", "/x/y"])
    assert a.geometry_cache == "/x/y" and a.cull_weight == -1
    with pytest.raises(SystemExit) as e:
        train_tgtcs.main(base + ["--synthetic", "--render_valid_style", "--basedir", str(tmp_path), "--geometry_cache",
                                 str(tmp_path / "g")])
    assert "--geometry_cache needs --share_geometry" in str(e.value)
    assert not os.path.exists(str(tmp_path / "g"))
    text = " ".join(cfg.config_parser().format_help().lower().split())
    assert "without any nerf density pass" in text and "an unset --cull_weight means 0" in text
