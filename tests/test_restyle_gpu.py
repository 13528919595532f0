"""GPU: restyling rays from a cached geometry (tgtc_geometry_build / tgtc_geometry_pack / tgtc_restyle_rays,
RayRenderer.build_geometry / restyle, --geometry_cache).

The statement is BIT IDENTITY with the culled render (tgtc_render_rays_styled_sparse) at the build's min_weight and needs no
tolerance: a live sample is the same column of the same MFMA sequence on the same operands wherever it sits in a tile, and
the compositing over the list skips only terms that leave the dense kernel's accumulators unchanged (acc + w * 0, acc + 0 * c)."""
import os

import numpy as np
import pytest
import torch

from test_sparse_style_gpu import make, render_inputs, renderers, workspace_planes  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = ["fp16x3", "fp16"]


def _restyle_equals_sparse(r, ro, rd, nc, nf, zs, jit, tau=0., cache=None):
    """restyle from `cache` (built here if None) against render_latents(min_weight=tau); returns (cache, restyle's result)."""
    if cache is None:
        cache = r.build_geometry(ro, rd, nc, nf, jitter=jit, min_weight=tau)
    out = r.restyle(cache, ro, rd, zs)
    ref = r.render_latents(ro, rd, nc, nf, jitter=jit, zs=zs, min_weight=tau)
    assert out["rgb"].shape == ref["rgb"].shape and out["t"].shape == ref["t"].shape
    assert torch.equal(out["rgb"], ref["rgb"]), float((out["rgb"] - ref["rgb"]).abs().max())
    assert torch.equal(out["t"], ref["t"])
    assert out["live"] == cache.count == int(ref["live"])
    return cache, out


# ------------------------------------------------------------------------------------------------ 1: bits of the sparse render
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nc,nf", [(128, 64), (64, 64), (100, 28)])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("tau", [0., 1e-3])
def test_restyle_bits_of_the_sparse_render(precision, nc, nf, K, tau):
    r, _, _, _ = renderers(precision)
    R = 300
    ro, rd, zs, jit = render_inputs(R, nc, K, seed=11)
    cache, out = _restyle_equals_sparse(r, ro, rd, nc, nf, zs, jit, tau)
    print(precision, nc, nf, K, tau, "live", cache.count, "of", R * (nc + nf))
    assert 0 < cache.count < R * (nc + nf) and (cache.R, cache.N, cache.min_weight) == (R, nc + nf, tau)
    assert bool(out["rgb"].any())
    # without jitter as well (the build's other input path)
    _restyle_equals_sparse(r, ro, rd, nc, nf, zs, None, tau)


# ------------------------------------------------------------------------------------------------ 2: the cache's planes
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tau", [0., 1e-3])
def test_the_cache_is_what_the_header_says(precision, tau):
    r, _, _, _ = renderers(precision)
    R, nc, nf, K = 300, 128, 64, 2
    N = nc + nf
    ro, rd, zs, jit = render_inputs(R, nc, K, seed=11)
    cache = r.build_geometry(ro, rd, nc, nf, jitter=jit, min_weight=tau, key="abc")
    ref = r.render_latents(ro, rd, nc, nf, jitter=jit, zs=zs, min_weight=tau)
    p = workspace_planes(r, R, nc, nf, K)
    n = int(ref["live"])
    assert cache.count == n and cache.key == "abc" and (cache.n_coarse, cache.n_fine) == (nc, nf)
    assert cache.buffer.numel() == cache.nbytes(R, n)
    live = p["live"][:n]
    assert torch.equal(cache.live, live)
    assert torch.equal(cache.ts_live, p["ts_f"].flatten()[live.long()])
    assert torch.equal(cache.w_live, p["w_f"].flatten()[live.long()])
    assert torch.equal(cache.t, ref["t"])
    want = torch.searchsorted(live.long(), torch.arange(R + 1, device="cuda") * N).to(torch.int32)
    assert torch.equal(cache.ray_start, want)
    tau_bits = int(np.float32(tau).view(np.int32))
    assert cache.header[:8].tolist() == [cache.MAGIC, cache.VERSION, R, 0, N, n, tau_bits, 0] and not bool(cache.header[8:].any())
    # a ray with no live sample between two that have some: its empty range must composite to +0 like the dense kernel's
    per_ray = (cache.ray_start[1:] - cache.ray_start[:-1]).cpu().numpy()
    empty = np.nonzero(per_ray == 0)[0]
    assert any(per_ray[:e].any() and per_ray[e + 1:].any() for e in empty), per_ray


# ------------------------------------------------------------------------------------------------ 3: read-only, stateless
@pytest.mark.parametrize("precision", PRECISIONS)
def test_restyle_reads_the_cache_only_and_keeps_no_state(precision):
    r, _, _, _ = renderers(precision)
    R, nc, nf, K = 300, 128, 64, 2
    ro, rd, _, jit = render_inputs(R, nc, K, seed=11)
    cache = r.build_geometry(ro, rd, nc, nf, jitter=jit)
    before = cache.buffer.clone()
    outs = []
    for seed in (21, 22, 23):
        zs = torch.from_numpy(np.random.default_rng(seed).standard_normal((K, R, 32)).astype(np.float32)).cuda()
        _, out = _restyle_equals_sparse(r, ro, rd, nc, nf, zs, jit, cache=cache)     # the render in between reuses the workspace
        outs.append(out["rgb"].clone())
    assert torch.equal(cache.buffer, before)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])


# ------------------------------------------------------------------------------------------------ 4: edges
@pytest.mark.parametrize("precision", PRECISIONS)
def test_edges_nothing_live_and_everything_live(precision):
    nc, nf, K = 64, 64, 2
    ro, rd, zs, jit = render_inputs(40, nc, K)
    r, _, _, _ = renderers(precision, fine_sigma_bias=-1e4)
    cache, out = _restyle_equals_sparse(r, ro, rd, nc, nf, zs, jit)
    assert cache.count == 0 and not bool(out["rgb"].any()) and not bool(cache.ray_start.any())
    r, _, _, _ = renderers(precision, fine_sigma_const=8.0)
    # 768 samples: a whole number of tiles in both precisions (128 / 256 samples per workgroup); 576: ragged in both
    for R, whole in ((4, True), (3, False)):
        ro, rd, zs, jit = render_inputs(R, 128, K)
        cache, out = _restyle_equals_sparse(r, ro, rd, 128, 64, zs, jit)
        assert cache.count == R * 192 and (cache.count % 256 == 0) == whole and (cache.count % 128 == 0) == whole
        assert torch.equal(cache.live, torch.arange(R * 192, device="cuda", dtype=torch.int32))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_edges_one_ray_ragged_tile_and_many_tiles(precision):
    r, _, _, _ = renderers(precision)
    ro, rd, zs, jit = render_inputs(1, 128, 1)
    cache, _ = _restyle_equals_sparse(r, ro, rd, 128, 64, zs, jit)
    print(precision, "R=1 live", cache.count)
    assert cache.count > 0
    ro, rd, zs, jit = render_inputs(300, 128, 1)
    cache, _ = _restyle_equals_sparse(r, ro, rd, 128, 64, zs, jit)
    assert cache.count % 128 != 0 and cache.count % 256 != 0, cache.count
    # more than one tile per CU: the persistent workgroups loop over the list
    ro, rd, zs, jit = render_inputs(6000, 128, 2)
    cache, _ = _restyle_equals_sparse(r, ro, rd, 128, 64, zs, jit)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(precision, "R=6000 live", cache.count, "tiles per CU >=", cache.count / 256 / cus)
    assert cache.count > 256 * cus


# ------------------------------------------------------------------------------------------------ 5: file round trip
@pytest.mark.parametrize("precision", PRECISIONS)
def test_file_round_trip_and_mismatches(tmp_path, precision):
    from tgtc_style_amd.rendering import GeometryCache
    r, _, _, _ = renderers(precision)
    R, nc, nf, K = 300, 100, 28, 2
    ro, rd, zs, jit = render_inputs(R, nc, K, seed=11)
    cache = r.build_geometry(ro, rd, nc, nf, jitter=jit, min_weight=1e-3, key="frame 7")
    path = str(tmp_path / "g.pt")
    cache.save(path)
    loaded = GeometryCache.load(path, torch.device("cuda"))
    assert loaded.buffer.is_cuda and loaded.buffer.data_ptr() != cache.buffer.data_ptr() and torch.equal(loaded.buffer, cache.buffer)
    assert (loaded.R, loaded.N, loaded.count, loaded.min_weight, loaded.key) == (R, nc + nf, cache.count, 1e-3, "frame 7")
    del cache
    _, out = _restyle_equals_sparse(r, ro, rd, nc, nf, zs, jit, tau=1e-3, cache=loaded)
    again = r.restyle(loaded, ro, rd, zs, key="frame 7", n_coarse=nc, n_fine=nf)
    assert torch.equal(again["rgb"], out["rgb"]) and torch.equal(again["t"], out["t"])
    with pytest.raises(ValueError):
        r.restyle(loaded, ro, rd, zs, key="frame 8")
    with pytest.raises(ValueError):
        r.restyle(loaded, ro[:-1], rd[:-1], zs[:, :-1])                       # another R
    with pytest.raises(ValueError):
        r.restyle(loaded, ro, rd, zs, n_coarse=nc, n_fine=nf + 1)            # another N
    with pytest.raises(ValueError):
        r.restyle(loaded, ro, rd, zs[:, :, :16])


# ------------------------------------------------------------------------------------------------ 6: argument rules
def test_restyle_argument_rules():
    from tgtc_style_amd import hip
    lib = hip.load()
    r, _, nets, pair = renderers("fp16x3")
    R, nc, nf, K = 16, 64, 64, 2
    ro, rd, zs, _ = render_inputs(R, nc, K)
    cache = r.build_geometry(ro, rd, nc, nf)
    n = cache.count
    assert n > 0
    need = lib.tgtc_restyle_workspace_bytes(n, K)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rgb, t = torch.empty(K, R, 3, device="cuda"), torch.empty(R, device="cuda")
    c, f, s = nets[0].packed().handle, nets[1].packed().handle, pair.packed().handle
    cb = cache.buffer.numel()

    def call(fine=f, style=s, K=K, R=R, nc=nc, nf=nf, cache_bytes=cb, count=n, ws_bytes=need, z=zs, t_out=t):
        return lib.tgtc_restyle_rays(fine, style, hip.ptr(ro), hip.ptr(rd), hip.ptr(z), K, R, nc, nf, hip.ptr(cache.buffer),
                                     cache_bytes, count, hip.ptr(ws), ws_bytes, hip.ptr(rgb), hip.ptr(t_out), hip.stream())
    assert call() == 0 and call(t_out=None) == 0
    assert call(cache_bytes=cb - 1) == -1 and call(ws_bytes=need - 1) == -1
    assert call(K=0) == -1 and call(R=-1) == -1 and call(nc=2) == -1 and call(nf=0) == -1 and call(z=None) == -1
    assert call(style=f) == -1 and call(fine=s) == -1
    assert call(count=R * (nc + nf) + 1, cache_bytes=1 << 40, ws_bytes=1 << 40) == -1
    assert call(R=0) == 0
    _, _, nets16, _ = renderers("fp16")
    assert call(fine=nets16[1].packed().handle) == -1          # fine NeRF and style nets of different precisions
    assert call(R=1 << 24, cache_bytes=1 << 40) == -2           # R x N >= 2^31
    assert call(K=1 << 20, count=1 << 11, cache_bytes=1 << 40, ws_bytes=1 << 40) == -2     # K x count >= 2^31

    # the build and the pack
    need_b = lib.tgtc_render_styled_sparse_workspace_bytes(R, nc, nf, 1)
    wsb = torch.empty(need_b, dtype=torch.uint8, device="cuda")
    live = torch.zeros((), dtype=torch.int32, device="cuda")

    def build(coarse=c, fine=f, R=R, ws_bytes=need_b, tau=0., count=live):
        return lib.tgtc_geometry_build(coarse, fine, hip.ptr(ro), hip.ptr(rd), R, nc, nf, 0., 1., None, tau, hip.ptr(wsb), ws_bytes,
                                       hip.ptr(t), hip.ptr(count), hip.stream())
    assert build() == 0 and int(live) == n
    assert build(ws_bytes=need_b - 1) == -1 and build(fine=s) == -1 and build(coarse=s) == -1 and build(count=None) == -1
    assert build(tau=-1.) == -1 and build(R=0) == 0
    buf = torch.zeros(cb, dtype=torch.uint8, device="cuda")
    assert lib.tgtc_geometry_pack(hip.ptr(wsb), R, nc, nf, 0., n, hip.ptr(buf), cb - 1, hip.stream()) == -1
    assert lib.tgtc_geometry_pack(hip.ptr(wsb), R, nc, nf, 0., n, hip.ptr(buf), cb, hip.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf, cache.buffer)


# ------------------------------------------------------------------------------------------------ 7: CLI
def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


class _CountBuilds:
    def __enter__(self):
        from tgtc_style_amd import rendering
        self.cls, self.orig, self.calls = rendering.RayRenderer, rendering.RayRenderer.build_geometry, 0

        def counted(renderer, *a, **kw):
            self.calls += 1
            return self.orig(renderer, *a, **kw)
        self.cls.build_geometry = counted
        return self

    def __exit__(self, *exc):
        self.cls.build_geometry = self.orig


def test_cli_geometry_cache(tmp_path):
    """--share_geometry --geometry_cache D: the first run writes the cache files and the PNGs of --share_geometry --cull_weight 0;
    a second run reads them -- build_geometry is not called -- and writes the same PNGs."""
    from tgtc_style_amd import train_tgtcs
    base = ["--config", os.path.join(ROOT, "configs", "fern.txt"), "--synthetic", "--synthetic_hw", "40", "--synthetic_frames", "2",
            "--synthetic_styles", "2", "--chunk", "1024", "--batch_size", "512", "--render_valid_style", "--share_geometry"]
    D = str(tmp_path / "geometry")
    plain = _files(train_tgtcs.main(base + ["--basedir", str(tmp_path / "plain"), "--cull_weight", "0"]))
    with _CountBuilds() as n:
        first = _files(train_tgtcs.main(base + ["--basedir", str(tmp_path / "first"), "--geometry_cache", D]))
    assert n.calls == 2 and len(os.listdir(D)) == 2 and all(f.endswith(".pt") for f in os.listdir(D))
    with _CountBuilds() as n:
        second = _files(train_tgtcs.main(base + ["--basedir", str(tmp_path / "second"), "--geometry_cache", D]))
    assert n.calls == 0
    assert len(plain) == 8 and sorted(first) == sorted(plain) and sorted(second) == sorted(plain)
    for name in plain:
        assert first[name] == plain[name] and second[name] == plain[name], name
    # another threshold is another key: the files are rebuilt, not reused
    with _CountBuilds() as n:
        train_tgtcs.main(base + ["--basedir", str(tmp_path / "third"), "--geometry_cache", D, "--cull_weight", "1e-3"])
    assert n.calls == 2


def _cli_rank(rank, world, port, argv):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), TGTC_DIST_BACKEND="gloo")
    from tgtc_style_amd import train_tgtcs
    train_tgtcs.main(argv)


def test_cli_geometry_cache_two_ranks(tmp_path):
    """Two ranks, --shard rays: every rank keeps the cache of its own pixel range; the files of the one-rank run."""
    import socket
    import torch.multiprocessing as mp
    from tgtc_style_amd import train_tgtcs
    common = ["--config", os.path.join(ROOT, "configs", "fern.txt"), "--synthetic", "--synthetic_hw", "40", "--synthetic_frames", "2",
              "--synthetic_styles", "2", "--chunk", "1024", "--batch_size", "512", "--render_valid_style", "--share_geometry"]
    one = train_tgtcs.main(common + ["--basedir", str(tmp_path / "one"), "--cull_weight", "0"])
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: os.environ.get(k) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TGTC_DIST_BACKEND")}
    D = str(tmp_path / "geometry")
    try:
        mp.spawn(_cli_rank, args=(2, port, common + ["--basedir", str(tmp_path / "two"), "--shard", "rays", "--geometry_cache", D]),
                 nprocs=2, join=True)
    finally:
        for k, v in env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    two = os.path.join(str(tmp_path / "two"), os.path.relpath(one, str(tmp_path / "one")))
    a, b = _files(one), _files(two)
    assert len(a) == 8 and sorted(b) == sorted(a) and len(os.listdir(D)) == 4      # 2 frames x 2 pixel ranges
    for n in a:
        assert a[n] == b[n], n
