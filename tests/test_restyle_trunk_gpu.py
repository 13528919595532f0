"""GPU: restyling from a cached trunk plane (tgtc_geometry_trunk / tgtc_restyle_rays_trunk[_folded], RayRenderer.build_trunk /
restyle(use_trunk=), GeometryCache.trunk).

The statement is BIT IDENTITY with restyle(use_trunk=False) on the same cache -- tgtc_restyle_rays / tgtc_restyle_rays_folded,
which run the fine NeRF trunk themselves -- and needs no tolerance: a live sample is the same column of the same MFMA sequence
on the same operands, and base_remap's half8 values make a round trip through memory either way (the style handle's slab
there, the plane here)."""
import functools

import numpy as np
import pytest
import torch

from test_sparse_style_gpu import make, render_inputs, renderers  # noqa: F401

pytestmark = pytest.mark.gpu
PRECISIONS = ["fp16x3", "fp16"]
PER_TILE = {"fp16x3": 128, "fp16": 256}
TILE = 131072


@functools.lru_cache(maxsize=None)
def _nets(precision, **kw):
    """(renderer, nets, pair) of the sibling tests, packed once per precision and variant."""
    r, _, nets, pair = renderers(precision, **kw)
    return r, nets, pair


def _flat(zs):
    """K latents that are the same for every ray: zs [K,R,32] -> [K,32] (the folded entry points)."""
    return zs[:, 0].contiguous()


def _same_bits(r, cache, ro, rd, zs, renderer=None):
    """restyle from the plane (by `renderer`, default r) against restyle(use_trunk=False) by r; returns the plane's result."""
    assert cache.trunk is not None
    ref = r.restyle(cache, ro, rd, zs, use_trunk=False)
    out = (renderer or r).restyle(cache, ro, rd, zs)                     # use_trunk=None: the cache carries a plane
    forced = (renderer or r).restyle(cache, ro, rd, zs, use_trunk=True)
    assert out["rgb"].shape == ref["rgb"].shape == (zs.shape[0], cache.R, 3) and out["t"].shape == ref["t"].shape
    assert torch.equal(out["rgb"], ref["rgb"]), float((out["rgb"] - ref["rgb"]).abs().max())
    assert torch.equal(out["t"], ref["t"]) and out["live"] == ref["live"] == cache.count
    assert torch.equal(forced["rgb"], ref["rgb"]) and torch.equal(forced["t"], ref["t"])
    return out


# ------------------------------------------------------------------------------------------------ 1: bits of the restyle
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nc,nf", [(128, 64), (64, 64), (100, 28)])
@pytest.mark.parametrize("tau", [0., 1e-3])
def test_trunk_restyle_bits_of_the_restyle(precision, nc, nf, tau):
    r, _, _ = _nets(precision)
    R = 300
    ro, rd, zs3, jit = render_inputs(R, nc, 3, seed=11)
    cache = r.build_geometry(ro, rd, nc, nf, jitter=jit, min_weight=tau)
    assert cache.trunk is None and 0 < cache.count < R * (nc + nf)
    assert r.build_trunk(cache, ro, rd) is cache
    assert cache.trunk.dtype == torch.uint8 and cache.trunk.is_cuda and cache.trunk_precision == precision
    assert cache.trunk.numel() == -(-cache.count // PER_TILE[precision]) * TILE == cache.trunk_nbytes(precision, cache.count)
    for K in (1, 3):
        for zs in (zs3[:K].contiguous(), _flat(zs3[:K])):               # [K,R,32]: unfolded; [K,32]: folded
            out = _same_bits(r, cache, ro, rd, zs)
            assert bool(out["rgb"].any())


# ------------------------------------------------------------------------------------------------ 2: edges
@pytest.mark.parametrize("precision", PRECISIONS)
def test_edges_nothing_live_and_everything_live(precision):
    nc, nf, K = 64, 64, 2
    ro, rd, zs, jit = render_inputs(40, nc, K)
    r, _, _ = _nets(precision, fine_sigma_bias=-1e4)
    cache = r.build_geometry(ro, rd, nc, nf, jitter=jit, keep_trunk=True)
    assert cache.count == 0 and cache.trunk is not None and cache.trunk.numel() == 0
    for z in (zs, _flat(zs)):
        out = _same_bits(r, cache, ro, rd, z)
        assert not bool(out["rgb"].any()) and not bool(torch.signbit(out["rgb"]).any())     # +0
    r, _, _ = _nets(precision, fine_sigma_const=8.0)
    # 768 samples: a whole number of tiles in both precisions (128 / 256 samples per workgroup); 576: ragged in both
    for R, whole in ((4, True), (3, False)):
        ro, rd, zs, jit = render_inputs(R, 128, K)
        cache = r.build_geometry(ro, rd, 128, 64, jitter=jit, keep_trunk=True)
        assert cache.count == R * 192 and (cache.count % 256 == 0) == whole and (cache.count % 128 == 0) == whole
        for z in (zs, _flat(zs)):
            _same_bits(r, cache, ro, rd, z)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_edges_one_ray_and_more_than_one_tile_per_cu(precision):
    r, _, _ = _nets(precision)
    ro, rd, zs, jit = render_inputs(1, 128, 1)
    cache = r.build_geometry(ro, rd, 128, 64, jitter=jit, keep_trunk=True)
    assert cache.count > 0
    for z in (zs, _flat(zs)):
        _same_bits(r, cache, ro, rd, z)
    # more than one tile per CU: the persistent workgroups of producer and consumer loop over the list
    ro, rd, zs, jit = render_inputs(6000, 128, 2)
    cache = r.build_geometry(ro, rd, 128, 64, jitter=jit, keep_trunk=True)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(precision, "R=6000 live", cache.count, "tiles per CU >=", cache.count / 256 / cus)
    assert cache.count > 256 * cus
    for z in (zs, _flat(zs)):
        _same_bits(r, cache, ro, rd, z)


# ------------------------------------------------------------------------------------------------ 3: 64-bit plane offsets
def test_plane_offsets_past_2_to_the_32():
    """Everything live at R = 22 100, 128 + 64 samples: some 4.24 M list entries, 33 150 tiles of 128 KiB in fp16x3 -- tile
    x 131072 passes 2^31 at tile 16 384 and 2^32 at 32 768.  The compared image includes the last rays, whose tiles lie behind
    both."""
    r, _, _ = _nets("fp16x3", fine_sigma_const=8.0)
    R = 22100
    ro, rd, zs, jit = render_inputs(R, 128, 1)
    cache = r.build_geometry(ro, rd, 128, 64, jitter=jit, keep_trunk=True)
    print("live", cache.count, "of", R * 192, "plane bytes", cache.trunk.numel())
    assert cache.trunk.numel() > 1 << 32 and cache.trunk.numel() == -(-cache.count // 128) * TILE
    first_past = (1 << 32) // TILE * 128                                  # first list entry of the first tile behind 2^32 bytes
    ray_past = int(cache.live[first_past]) // 192 + 1                     # a ray that lies behind it entirely
    assert ray_past < R - 1
    out = _same_bits(r, cache, ro, rd, zs)
    assert bool(out["rgb"][0, ray_past:].any()) and bool(out["rgb"][0, -1].any())
    cache.drop_trunk()
    assert cache.trunk is None


# ------------------------------------------------------------------------------------------------ 4: the producer
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_plane_is_reproducible_and_the_build_reads_the_cache_only(tmp_path, precision):
    from tgtc_style_amd.rendering import GeometryCache
    r, _, _ = _nets(precision)
    R, nc, nf = 300, 100, 28
    ro, rd, zs, jit = render_inputs(R, nc, 2, seed=11)
    cache = r.build_geometry(ro, rd, nc, nf, jitter=jit, min_weight=1e-3, keep_trunk=True)
    first, before = cache.trunk, cache.buffer.clone()
    r.build_trunk(cache, ro, rd)
    assert cache.trunk.data_ptr() != first.data_ptr() and torch.equal(cache.trunk, first)      # two builds: the same bytes
    assert torch.equal(cache.buffer, before)
    # over a plane that held other bytes: every byte of every tile is written (no zero-fill is needed)
    from tgtc_style_amd import hip
    dirty = torch.full_like(first, 0xa5)
    hip.check(hip.load().tgtc_geometry_trunk(r.fine.packed().handle, hip.ptr(ro), hip.ptr(rd), R, nc, nf, hip.ptr(cache.buffer),
                                             cache.buffer.numel(), cache.count, hip.ptr(dirty), dirty.numel(), hip.stream()))
    assert torch.equal(dirty, first)
    # a cache that went through a file (without the plane) builds the same plane; with the plane it comes back with it
    path = str(tmp_path / "g.pt")
    cache.save(path)
    loaded = GeometryCache.load(path, torch.device("cuda"))
    assert loaded.trunk is None
    r.build_trunk(loaded, ro, rd)
    assert torch.equal(loaded.trunk, first) and loaded.trunk_precision == precision
    cache.save(path, with_trunk=True)
    loaded = GeometryCache.load(path, torch.device("cuda"))
    assert loaded.trunk.is_cuda and torch.equal(loaded.trunk, first) and loaded.trunk_precision == precision
    _same_bits(r, loaded, ro, rd, zs)


# ------------------------------------------------------------------------------------------------ 5: no NeRF handle
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_renderer_without_nerf_networks_restyles_from_the_plane(precision):
    from tgtc_style_amd import rendering
    r, _, pair = _nets(precision)
    R, nc, nf = 300, 128, 64
    ro, rd, zs, jit = render_inputs(R, nc, 2, seed=11)
    cache = r.build_geometry(ro, rd, nc, nf, jitter=jit, keep_trunk=True)
    bare = rendering.RayRenderer(None, None, pair)
    for z in (zs, _flat(zs)):
        _same_bits(r, cache, ro, rd, z, renderer=bare)


# ------------------------------------------------------------------------------------------------ 6: read-only, stateless
@pytest.mark.parametrize("precision", PRECISIONS)
def test_restyle_reads_the_plane_only_and_keeps_no_state(precision):
    r, _, _ = _nets(precision)
    R, nc, nf, K = 300, 128, 64, 2
    ro, rd, _, jit = render_inputs(R, nc, K, seed=11)
    cache = r.build_geometry(ro, rd, nc, nf, jitter=jit, keep_trunk=True)
    plane, buffer = cache.trunk.clone(), cache.buffer.clone()
    outs = []
    for seed in (21, 22, 23):
        zs = torch.from_numpy(np.random.default_rng(seed).standard_normal((K, R, 32)).astype(np.float32)).cuda()
        outs.append(_same_bits(r, cache, ro, rd, zs)["rgb"].clone())
        r.render_latents(ro, rd, nc, nf, jitter=jit, zs=zs, min_weight=0.)      # reuses both slab regions of the style handle
        again = r.restyle(cache, ro, rd, zs)
        assert torch.equal(again["rgb"], outs[-1])
    assert torch.equal(cache.trunk, plane) and torch.equal(cache.buffer, buffer)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])


# ------------------------------------------------------------------------------------------------ 7: argument rules
def test_trunk_argument_rules():
    from tgtc_style_amd import hip
    lib = hip.load()
    r, nets, pair = _nets("fp16x3")
    R, nc, nf, K = 16, 64, 64, 2
    ro, rd, zs, _ = render_inputs(R, nc, K)
    cache = r.build_geometry(ro, rd, nc, nf)
    n = cache.count
    assert n > 0
    with pytest.raises(ValueError):
        r.restyle(cache, ro, rd, zs, use_trunk=True)                   # no plane
    f, s = nets[1].packed().handle, pair.packed().handle
    cb, pb = cache.buffer.numel(), lib.tgtc_geometry_trunk_bytes(hip.PREC_FP16X3, n)
    plane = torch.empty(pb, dtype=torch.uint8, device="cuda")

    def trunk(fine=f, R=R, cache_bytes=cb, count=n, out=plane, plane_bytes=pb):
        return lib.tgtc_geometry_trunk(fine, hip.ptr(ro), hip.ptr(rd), R, nc, nf, hip.ptr(cache.buffer), cache_bytes, count,
                                       hip.ptr(out), plane_bytes, hip.stream())
    assert trunk() == 0
    assert trunk(plane_bytes=pb - 1) == -1 and trunk(cache_bytes=cb - 1) == -1 and trunk(out=None) == -1
    assert trunk(fine=s) == -1                                          # a style handle as the fine handle
    assert trunk(R=0) == 0
    from tgtc_style_amd import rendering
    mx = _nets("fp16mx+fp16x3")[1][0]                                   # that pair's coarse net is packed in fp16mx
    assert mx.packed().precision == "fp16mx" and trunk(fine=mx.packed().handle) == -2
    with pytest.raises(RuntimeError):
        rendering.RayRenderer(None, mx, pair).build_trunk(cache, ro, rd)
    assert cache.trunk is None

    rgb, t = torch.empty(K, R, 3, device="cuda"), torch.empty(R, device="cuda")
    for call, ws_bytes, z in ((lib.tgtc_restyle_rays_trunk, lib.tgtc_restyle_workspace_bytes, zs),
                              (lib.tgtc_restyle_rays_trunk_folded, lib.tgtc_restyle_folded_workspace_bytes, _flat(zs))):
        need = ws_bytes(n, K)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")

        def restyle(style=s, K=K, R=R, cache_bytes=cb, count=n, trunk=plane, plane_bytes=pb, ws_bytes=need, z=z, t_out=t):
            return call(style, hip.ptr(ro), hip.ptr(rd), hip.ptr(z), K, R, nc, nf, hip.ptr(cache.buffer), cache_bytes, count,
                        hip.ptr(trunk), plane_bytes, hip.ptr(ws), ws_bytes, hip.ptr(rgb), hip.ptr(t_out), hip.stream())
        assert restyle() == 0 and restyle(t_out=None) == 0
        assert restyle(plane_bytes=pb - 1) == -1                        # a plane one byte short
        assert restyle(style=f) == -1                                   # the fine handle as the style handle
        assert restyle(cache_bytes=cb - 1) == -1 and restyle(ws_bytes=need - 1) == -1
        assert restyle(trunk=None) == -1 and restyle(z=None) == -1 and restyle(K=0) == -1
        assert restyle(R=0) == 0
    # the plane's size goes by the STYLE handle's precision: an fp16 pair needs half of it for the same list
    pair16 = _nets("fp16")[2].packed().handle
    half = lib.tgtc_geometry_trunk_bytes(hip.PREC_FP16, n)
    assert half < pb
    ws = torch.empty(lib.tgtc_restyle_workspace_bytes(n, K), dtype=torch.uint8, device="cuda")
    assert lib.tgtc_restyle_rays_trunk(pair16, hip.ptr(ro), hip.ptr(rd), hip.ptr(zs), K, R, nc, nf, hip.ptr(cache.buffer), cb, n,
                                       hip.ptr(plane), half - 1, hip.ptr(ws), ws.numel(), hip.ptr(rgb), hip.ptr(t),
                                       hip.stream()) == -1
    torch.cuda.synchronize()
