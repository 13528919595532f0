"""GPU: stylised frames of the fp16x3+fp16mx pair in one call, without a trunk plane (csrc/mlp_list_mx.hip:
styled_list_mx_kernel; tgtc_styled_forward_list_folded_mx, tgtc_render_rays_styled_sparse_folded_mx, tgtc_restyle_rays_folded_mx;
RayRenderer.render_latents / restyle(style_precision="fp16mx"); --style_precision).

The kernel is the trunk of trunk_plane_mx_kernel followed by the latent loop of restyle_trunk_mx_kernel per tile, with base_remap
parked in the style handle's slab instead of a plane, so its results are the BITS of the two-kernel path
(tgtc_geometry_trunk_mx -> tgtc_restyle_rays_trunk_folded_mx), and that is what tests 1, 2, 4, 5 and 6 ask for.

1. Bits, compact form: the seeded lists of the (40, 129) grid that end inside, one short of, on and one behind a 128-sample tile,
   behind two tiles, and the whole grid (a ragged last tile of many); K = 1 and K = 3 with the zero latent beside non-zero ones.
   rgb_live, rgb and t against the two-kernel path; the workspace is canary-filled.
2. Bits, scattered form: the listed rows of canary-filled dense planes equal the compact rows, every other row keeps the canary;
   a device count of 0 writes nothing.
3. Per sample against the float64 oracle (tests/test_fold_latents_gpu.py: oracle_planes), error max|a - ref| / max|ref|, hard bar
   1e-3 = TOL["fp16mx"] of tests/test_hip_nerf.py, over the list lengths x "abf" x base / rows / dead.
4. Revisits: about 2.2 x n_cu tiles, K = 2 -- every workgroup loads the NeRF table over latent K-1's bias table a second time.
5. One call on the headline renderer against build_geometry(keep_trunk=True, trunk_precision="fp16x3") + restyle.
6. The restyle without a plane: the bits of 5, cache.trunk stays None, no hidden plane is allocated.
7. Rules on real handles; the calls without the new argument keep their bits.
8. The command line."""
import math
import os

import numpy as np
import pytest
import torch

import test_fold_latents_gpu as F
import test_hip_style_shapes as S
from test_restyle_mx_gpu import list_cache, mx_pair, raw_restyle
from test_sparse_style_gpu import render_inputs, renderers
from test_trunk_mx_gpu import mx_nerf, produce

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-3                                  # TOL["fp16mx"] of tests/test_hip_nerf.py
CANARY, SPARE, CANARY_ROWS = -7.0, 4096, 64
GRID = F.BIG                                # (40, 129): 5 160 samples = 40.3 tiles of 128
NC, NF = 100, 29                            # n_coarse + n_fine = N of the grid
LIST_LENGTHS = [1, 17, 127, 128, 129, 257, None]     # None: every sample
BIT_LATENTS = ["a", "eda"]                  # K = 1 and 3; e is the zero latent, d a constant, a a seeded normal
WEIGHTS = ["base", "rows", "dead"]


def test_case_lists_are_the_ones_the_kernel_can_get_wrong():
    M = GRID[0] * GRID[1]
    assert {1, 17, 127, 128, 129, 257, None} == set(LIST_LENGTHS) and M == 5160 and M % 128 and M > 2 * 128
    assert {len(f) for f in BIT_LATENTS} == {1, 3} and "e" in BIT_LATENTS[1] and NC + NF == GRID[1]


# ------------------------------------------------------------------------------------------------------- launches
def raw_list_mx(nerf, pair, cache, ro, rd, z):
    """tgtc_restyle_rays_folded_mx into a canary-filled workspace with SPARE bytes behind it.  Returns (rgb_live [K,count,3],
    rgb [K,R,3], t [R]); asserts that every listed row was written, that the padding behind the rows and the spare bytes were not."""
    from tgtc_style_amd import hip
    lib = hip.load()
    K, n = z.shape[0], cache.count
    need = lib.tgtc_restyle_folded_workspace_bytes(n, K)
    ws = torch.full(((need + SPARE) // 4,), CANARY, device="cuda")
    rgb, t = torch.full((K, cache.R, 3), CANARY, device="cuda"), torch.full((cache.R,), CANARY, device="cuda")
    hip.check(lib.tgtc_restyle_rays_folded_mx(nerf.packed().handle, pair.packed().handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(z), K,
                                              cache.R, cache.n_coarse, cache.n_fine, hip.ptr(cache.buffer), cache.buffer.numel(), n,
                                              hip.ptr(ws), need, hip.ptr(rgb), hip.ptr(t), hip.stream()))
    torch.cuda.synchronize()
    plane_end = lib.tgtc_restyle_workspace_bytes(n, K) // 4             # the tables lie behind it
    live = ws[:K * n * 3].view(K, n, 3)
    assert bool((live != CANARY).all()), "a listed sample was left unwritten"
    assert bool((ws[K * n * 3:plane_end] == CANARY).all()) and bool((ws[need // 4:] == CANARY).all()), "wrote outside its planes"
    assert bool((rgb != CANARY).all()) and bool((t != CANARY).all())
    return live.clone(), rgb, t


def two_kernels(nerf, pair, cache, ro, rd, z):
    """The path on record: tgtc_geometry_trunk_mx into a plane of the cache's list, tgtc_restyle_rays_trunk_folded_mx from it.
    Returns (rgb_live, rgb).  The cache is left without a plane."""
    from tgtc_style_amd import hip
    cache.attach_trunk(produce(nerf, cache, ro, rd), "fp16x3", "fp16mx")
    try:
        return raw_restyle(hip.load().tgtc_restyle_rays_trunk_folded_mx, pair, cache, ro, rd, z)
    finally:
        cache.drop_trunk()


_GRID, _COMPACT = {}, {}


def grid(n):
    """(cache of the seeded list of length n on GRID, ro, rd, ts on the device, live on the device)"""
    if n not in _GRID:
        R, N = GRID
        ro, rd, ts, _ = S.ray_inputs(R, N, "a")
        live = F.sample_list(R * N, n)
        ro, rd = S.on_gpu(ro, rd)
        _GRID[n] = (list_cache(ro, ts, live, NC, NF), ro, rd, ts.cuda().contiguous(), live.cuda().contiguous())
    return _GRID[n]


def compact(n, families, wf):
    """(rgb_live, rgb, t) of tgtc_restyle_rays_folded_mx on grid(n): computed once, shared by tests 1, 2 and 3."""
    if (n, families, wf) not in _COMPACT:
        cache, ro, rd, _, _ = grid(n)
        _COMPACT[n, families, wf] = raw_list_mx(mx_nerf(), mx_pair(wf), cache, ro, rd, F.latent_rows(families).cuda())
    return _COMPACT[n, families, wf]


# ------------------------------------------------------------------------------------------------------- 1: bits, compact
@pytest.mark.parametrize("families", BIT_LATENTS)
@pytest.mark.parametrize("n", LIST_LENGTHS)
def test_compact_form_is_the_two_kernel_path_bit_for_bit(n, families):
    cache, ro, rd, _, _ = grid(n)
    live, rgb, t = compact(n, families, "base")
    ref_live, ref_rgb = two_kernels(mx_nerf(), mx_pair("base"), cache, ro, rd, F.latent_rows(families).cuda())
    assert live.shape == (len(families), cache.count, 3) and bool(torch.isfinite(live).all())
    assert float(live.min()) >= 0. and float(live.max()) <= 1. and bool(ref_rgb.any())
    assert torch.equal(live, ref_live), (n, families, float((live - ref_live).abs().max()))
    assert torch.equal(rgb, ref_rgb) and torch.equal(t, cache.t)
    if len(families) == 3:
        assert not torch.equal(live[0], live[1]) and not torch.equal(live[1], live[2])


# ------------------------------------------------------------------------------------------------------- 2: bits, scattered
def scattered(wf, n, z, count=None):
    """tgtc_styled_forward_list_folded_mx on grid(n) into canary-filled dense planes with CANARY_ROWS spare rows behind the last
    one; `count` replaces the list's length in the device word.  Returns the planes [K,M,3] and the spare rows."""
    from tgtc_style_amd import hip
    _, ro, rd, ts, live = grid(n)
    pair = mx_pair(wf)
    (R, N), K, M = ts.shape, z.shape[0], ts.numel()
    rgb = torch.full((K * M + CANARY_ROWS, 3), CANARY, device="cuda")
    n_live = torch.tensor(live.numel() if count is None else count, dtype=torch.int32, device="cuda")
    tables = F.fold(pair, z)
    hip.check(hip.load().tgtc_styled_forward_list_folded_mx(mx_nerf().packed().handle, pair.packed().handle, hip.ptr(ro), hip.ptr(rd),
                                                            hip.ptr(ts), hip.ptr(tables), K, R, N, hip.ptr(live), hip.ptr(n_live),
                                                            hip.ptr(rgb), hip.stream()))
    torch.cuda.synchronize()
    return rgb[:K * M].view(K, M, 3), rgb[K * M:]


@pytest.mark.parametrize("families", BIT_LATENTS)
@pytest.mark.parametrize("n", LIST_LENGTHS)
def test_scattered_form_writes_the_compact_rows_at_the_listed_samples(n, families):
    _, _, _, ts, live = grid(n)
    planes, spare = scattered("base", n, F.latent_rows(families).cuda())
    listed = torch.zeros(ts.numel(), dtype=torch.bool, device="cuda")
    listed[live.long()] = True
    assert torch.equal(planes[:, live.long()], compact(n, families, "base")[0]), (n, families)
    assert bool((planes[:, ~listed] == CANARY).all()) and bool((spare == CANARY).all()), "wrote outside the list"


def test_scattered_form_with_a_device_count_of_zero_writes_nothing():
    planes, spare = scattered("base", 257, F.latent_rows("ab").cuda(), count=0)
    assert bool((planes == CANARY).all()) and bool((spare == CANARY).all())


# ------------------------------------------------------------------------------------------------------- 3: float64
@pytest.mark.parametrize("wf", WEIGHTS)
@pytest.mark.parametrize("n", LIST_LENGTHS)
def test_per_sample_vs_float64(n, wf):
    """Hard bar 1e-3.  The errors (printed) are the plane path's, since the bits are."""
    R, N = GRID
    families = "abf"
    idx = F.sample_list(R * N, n).long()
    ref = torch.stack([F.oracle_planes(wf, R, N, f)[0][idx] for f in families])
    got = compact(n, families, wf)[0]
    e = S.rel(got, ref)
    print("fp16mx list kernel, no plane: list %-4s z(%s) %-5s err %.3e  bar %.1e" % (n if n else "all", families, wf, e, BAR))
    assert e <= BAR, (n, families, wf, e)


# ------------------------------------------------------------------------------------------------------- 4: revisits
def test_second_and_third_visit():
    """About 2.2 x n_cu tiles of 128 listed samples, K = 2: every persistent workgroup takes a second tile and some a third, and
    loads the NeRF table over latent 1's bias table at each.  One launch against launches over chunks of n_cu whole tiles (tile
    boundaries coincide, no workgroup revisits), against the two-kernel path, and against itself."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    N = NC + NF
    R = math.ceil(2.2 * n_cu * 128 / N) + 1
    M = R * N
    M -= M % 128 == 0                                                   # a ragged last tile
    assert (M + 127) // 128 > 2 * n_cu
    ro, rd, ts, _ = S.ray_inputs(R, N, "a", seed=62000 + n_cu)
    ro, rd = S.on_gpu(ro, rd)
    z = F.latent_rows("ab").cuda()
    nerf, pair = mx_nerf(), mx_pair("base")
    live = torch.arange(M, dtype=torch.int32)
    cache = list_cache(ro, ts, live, NC, NF)
    whole, rgb, _ = raw_list_mx(nerf, pair, cache, ro, rd, z)
    assert bool(torch.isfinite(whole).all()) and not torch.equal(whole[0], whole[1])
    again, rgb2, _ = raw_list_mx(nerf, pair, cache, ro, rd, z)
    assert torch.equal(again, whole) and torch.equal(rgb2, rgb)
    ref_live, ref_rgb = two_kernels(nerf, pair, cache, ro, rd, z)
    assert torch.equal(whole, ref_live) and torch.equal(rgb, ref_rgb)
    chunk = n_cu * 128
    for i0 in range(0, M, chunk):
        part = list_cache(ro, ts, live[i0:i0 + chunk].contiguous(), NC, NF)
        got, _, _ = raw_list_mx(nerf, pair, part, ro, rd, z)
        assert torch.equal(got, whole[:, i0:i0 + chunk]), "list entries %d.." % i0


# ------------------------------------------------------------------------------------------------------- 5, 6: the renderer
R_FRAME = 300
_HEAD = []


def headline():
    """The renderer of --precision fp16x3+fp16mx: coarse fp16x3, fine fp16mx, the style pair in fp16x3."""
    if not _HEAD:
        _HEAD.append(renderers("fp16x3+fp16mx")[0])
    r = _HEAD[0]
    assert (r.coarse.packed().precision, r.fine.packed().precision, r.style.packed().precision) == ("fp16x3", "fp16mx", "fp16x3")
    return r


def frame_inputs(nc, K):
    ro, rd, zs, jit = render_inputs(R_FRAME, nc, K)
    return ro, rd, zs[:, 0, :].contiguous(), jit


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("nc,nf", [(64, 64), (100, 28)])
def test_one_call_is_build_geometry_plus_the_restyle_from_the_plane(nc, nf, K):
    r = headline()
    ro, rd, z, jit = frame_inputs(nc, K)
    counts = []
    for tau in (0., 1e-3):
        out = r.render_latents(ro, rd, nc, nf, jitter=jit, zs=z, min_weight=tau, style_precision="fp16mx")
        rgb, t, n = out["rgb"].clone(), out["t"].clone(), int(out["live"])
        cache = r.build_geometry(ro, rd, nc, nf, jitter=jit, min_weight=tau, keep_trunk=True, trunk_precision="fp16x3")
        assert cache.trunk is not None and cache.trunk_source == "fp16mx"
        ref = r.restyle(cache, ro, rd, z, style_precision="fp16mx")
        assert n == cache.count == ref["live"] and 0 < n < R_FRAME * (nc + nf), (n, cache.count)
        assert rgb.shape == (K, R_FRAME, 3) and bool(torch.isfinite(rgb).all()) and bool(rgb.any())
        assert torch.equal(rgb, ref["rgb"]) and torch.equal(t, ref["t"]), (tau, float((rgb - ref["rgb"]).abs().max()))
        counts.append(n)
    assert counts[1] < counts[0]
    # nothing live (a weight is at most 1): colour +0, the depth image as ever
    out = r.render_latents(ro, rd, nc, nf, jitter=jit, zs=z, min_weight=2., style_precision="fp16mx")
    empty = r.build_geometry(ro, rd, nc, nf, jitter=jit, min_weight=2.)
    assert int(out["live"]) == 0 == empty.count
    assert not bool(out["rgb"].any()) and not bool(torch.signbit(out["rgb"]).any()) and torch.equal(out["t"], empty.t)
    assert torch.equal(out["t"], t)


@pytest.mark.parametrize("K", [1, 3])
def test_restyle_without_a_plane(K):
    r = headline()
    nc, nf = 64, 64
    ro, rd, z, jit = frame_inputs(nc, K)
    for tau in (0., 1e-3):
        one = r.render_latents(ro, rd, nc, nf, jitter=jit, zs=z, min_weight=tau, style_precision="fp16mx")
        one = {k: v.clone() for k, v in one.items()}
        bare = r.build_geometry(ro, rd, nc, nf, jitter=jit, min_weight=tau)
        assert bare.trunk is None
        out = r.restyle(bare, ro, rd, z, style_precision="fp16mx")          # (also the warm-up: mx streams, workspace)
        assert bare.trunk is None and bare.trunk_precision is None
        assert torch.equal(out["rgb"], one["rgb"]) and torch.equal(out["t"], one["t"]) and out["live"] == int(one["live"])
    # memory: with the workspace in place the call allocates its two results and nothing of a plane's size; the form with a
    # plane allocates the plane
    plane_bytes = bare.trunk_nbytes("fp16x3", bare.count)
    ws_bytes = r._ws_restyle.numel()
    assert plane_bytes >= 8 * 131072
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = r.restyle(bare, ro, rd, z, style_precision="fp16mx")
    torch.cuda.synchronize()
    without = torch.cuda.max_memory_allocated() - base
    del out
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r.build_trunk(bare, ro, rd, trunk_precision="fp16x3")
    out = r.restyle(bare, ro, rd, z, style_precision="fp16mx")
    torch.cuda.synchronize()
    with_plane = torch.cuda.max_memory_allocated() - base
    bare.drop_trunk()
    print("restyle K = %d, %d live: peak %d B without a plane, %d B with one (plane %d B, workspace %d B)"
          % (K, bare.count, without, with_plane, plane_bytes, ws_bytes))
    assert without < plane_bytes and without < plane_bytes + ws_bytes and with_plane >= plane_bytes
    # with a plane the call is the plane consumer's; use_trunk=False takes the new kernel again: the same bits either way
    r.build_trunk(bare, ro, rd, trunk_precision="fp16x3")
    assert torch.equal(r.restyle(bare, ro, rd, z, style_precision="fp16mx", use_trunk=False)["rgb"], one["rgb"])
    assert bare.trunk is not None
    assert torch.equal(r.restyle(bare, ro, rd, z, style_precision="fp16mx")["rgb"], one["rgb"])


# ------------------------------------------------------------------------------------------------------- 7: real handles
def test_rules_on_real_handles():
    from tgtc_style_amd import hip, models, rendering
    from test_sparse_style_gpu import make
    lib = hip.load()
    cm, sm, nets_x3 = make("fp16x3")
    _, _, nets_mx = make("fp16x3+fp16mx")
    pair = models.StylePair(cm, sm)                                      # a handle of its own: nothing enabled yet
    rx = rendering.RayRenderer(nets_x3[0], nets_x3[1], pair)
    rh = rendering.RayRenderer(nets_mx[0], nets_mx[1], pair)
    r16, _, nets16, pair16 = renderers("fp16")
    R, nc, nf, K = R_FRAME, 64, 64, 2
    ro, rd, z, jit = frame_inputs(nc, K)
    # what the calls without the new argument return before the new kernel has run on the style handle
    cache_x3 = rx.build_geometry(ro, rd, nc, nf, jitter=jit)
    before_frame = {k: v.clone() for k, v in rx.render_latents(ro, rd, nc, nf, jitter=jit, zs=z, min_weight=0.).items()}
    before_restyle = rx.restyle(cache_x3, ro, rd, z)["rgb"].clone()
    cache = rh.build_geometry(ro, rd, nc, nf, jitter=jit)
    assert 0 < cache.count < R * (nc + nf) and not pair.packed().has_mx()

    need = lib.tgtc_restyle_folded_workspace_bytes(cache.count, K)
    ws = torch.full((need // 4,), CANARY, device="cuda")
    rgb, t = torch.full((K, R, 3), CANARY, device="cuda"), torch.full((R,), CANARY, device="cuda")
    fine, s = nets_mx[1].packed().handle, pair.packed().handle

    def call(fine=fine, style=s, zz=z, ws_bytes=need, cache_bytes=cache.buffer.numel(), R=R):
        return lib.tgtc_restyle_rays_folded_mx(fine, style, hip.ptr(ro), hip.ptr(rd), hip.ptr(zz), K, R, nc, nf,
                                               hip.ptr(cache.buffer), cache_bytes, cache.count, hip.ptr(ws), ws_bytes,
                                               hip.ptr(rgb), hip.ptr(t), hip.stream())
    assert call() == -2 and b"no fp16mx streams" in lib.tgtc_last_error()                       # a pair without mx streams
    pair.packed().enable_mx()
    assert call(fine=nets_x3[1].packed().handle) == -2 and b"must be in fp16mx" in lib.tgtc_last_error()
    assert call(fine=nets16[1].packed().handle) == -2
    assert call(style=pair16.packed().handle) == -2 and b"no lo halves" in lib.tgtc_last_error()
    assert call(fine=s) == -1 and call(style=fine) == -1                                        # wrong handle kinds
    assert call(zz=None) == -1 and b"null pointer" in lib.tgtc_last_error()
    assert call(ws_bytes=need - 1) == -1 and b"workspace" in lib.tgtc_last_error()
    assert call(cache_bytes=cache.buffer.numel() - 1) == -1 and b"cache of" in lib.tgtc_last_error()
    torch.cuda.synchronize()
    assert bool((ws == CANARY).all()) and bool((rgb == CANARY).all()) and bool((t == CANARY).all()), "a refused call wrote"
    assert call(R=0) == 0
    torch.cuda.synchronize()
    assert bool((ws == CANARY).all()) and bool((rgb == CANARY).all())
    # the other two entry points refuse the same handles
    big = lib.tgtc_render_styled_sparse_folded_workspace_bytes(R, nc, nf, K)
    ws2 = torch.full((big // 4,), CANARY, device="cuda")
    live = torch.zeros((), dtype=torch.int32, device="cuda")

    def frame(coarse=nets_mx[0].packed().handle, fine=fine, style=s, ws_bytes=big):
        return lib.tgtc_render_rays_styled_sparse_folded_mx(coarse, fine, style, hip.ptr(ro), hip.ptr(rd), hip.ptr(z), K, R, nc, nf,
                                                            0., 1., hip.ptr(jit), 0., hip.ptr(ws2), ws_bytes, hip.ptr(rgb), hip.ptr(t),
                                                            hip.ptr(live), hip.stream())
    assert frame(fine=nets_x3[1].packed().handle) == -2 and frame(fine=nets16[1].packed().handle) == -2
    assert frame(style=pair16.packed().handle) == -2 and frame(style=fine) == -1 and frame(ws_bytes=big - 1) == -1
    tables = F.fold(pair, z)
    n_live = torch.tensor(cache.count, dtype=torch.int32, device="cuda")
    ts = torch.rand(R, nc + nf, device="cuda")

    def fwd(nerf=fine, style=s, tab=tables):
        return lib.tgtc_styled_forward_list_folded_mx(nerf, style, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), hip.ptr(tab), K, R, nc + nf,
                                                      hip.ptr(cache.live), hip.ptr(n_live), hip.ptr(ws2), hip.stream())
    assert fwd(nerf=nets_x3[1].packed().handle) == -2 and fwd(style=pair16.packed().handle) == -2
    assert fwd(nerf=s) == -1 and fwd(tab=None) == -1
    torch.cuda.synchronize()
    assert bool((ws2 == CANARY).all()) and bool((rgb == CANARY).all()) and int(live) == 0, "a refused call wrote"
    # the existing entry points still refuse the mixed pair
    assert lib.tgtc_restyle_rays_folded(fine, s, hip.ptr(ro), hip.ptr(rd), hip.ptr(z), K, R, nc, nf, hip.ptr(cache.buffer),
                                        cache.buffer.numel(), cache.count, hip.ptr(ws), need, hip.ptr(rgb), hip.ptr(t),
                                        hip.stream()) == -1
    assert b"different precisions" in lib.tgtc_last_error()
    with pytest.raises(RuntimeError):
        rh.render_latents(ro, rd, nc, nf, jitter=jit, zs=z, min_weight=0.)
    with pytest.raises(RuntimeError):
        rh.restyle(cache, ro, rd, z)
    # the wrappers' refusals, before any launch
    z3 = z[:, None, :].expand(-1, R, -1).contiguous()
    mode = dict(jitter=jit, style_precision="fp16mx")
    with pytest.raises(ValueError):
        rh.render_latents(ro, rd, nc, nf, zs=z3, min_weight=0., **mode)                          # a 3-D zs
    with pytest.raises(ValueError):
        rh.render_latents(ro, rd, nc, nf, zs=z, **mode)                                          # no min_weight
    with pytest.raises(ValueError):
        rx.render_latents(ro, rd, nc, nf, zs=z, min_weight=0., **mode)                           # an fp16x3 fine handle
    with pytest.raises(ValueError):
        rendering.RayRenderer(nets_mx[0], nets_mx[1], pair16).render_latents(ro, rd, nc, nf, zs=z, min_weight=0., **mode)   # an fp16 pair
    with pytest.raises(ValueError):
        rh.render_latents(ro, rd, nc, nf, zs=z, min_weight=0., jitter=jit, style_precision="fp16x3")
    with pytest.raises(ValueError):
        rx.restyle(cache_x3, ro, rd, z, style_precision="fp16mx")                                # no plane, an fp16x3 fine handle
    with pytest.raises(ValueError):
        rh.restyle(cache, ro, rd, z3, style_precision="fp16mx")
    with pytest.raises(ValueError):
        rh.restyle(cache, ro, rd, z, style_precision="fp16mx", use_trunk=True)                   # insists on a plane that is not there
    # the new kernel runs on the style handle (both slab regions) ...
    a = rh.render_latents(ro, rd, nc, nf, zs=z, min_weight=0., **mode)
    b = rh.restyle(cache, ro, rd, z, style_precision="fp16mx")
    assert torch.equal(a["rgb"], b["rgb"]) and bool(a["rgb"].any()) and not torch.equal(a["rgb"], before_frame["rgb"])
    # ... and the calls without the new argument return the bits they returned before
    after = rx.render_latents(ro, rd, nc, nf, jitter=jit, zs=z, min_weight=0.)
    assert torch.equal(after["rgb"], before_frame["rgb"]) and torch.equal(after["t"], before_frame["t"])
    assert torch.equal(rx.restyle(cache_x3, ro, rd, z)["rgb"], before_restyle)


# ------------------------------------------------------------------------------------------------------- 8: the command line
def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_cli_style_precision(tmp_path):
    """--precision fp16x3+fp16mx --render_valid_style --share_geometry --fold_latents --cull_weight 0 --style_precision fp16mx
    writes its PNGs; with --geometry_cache the same bytes, and again from the filled directory without a geometry build; without
    --style_precision the command fails as it did."""
    from test_restyle_gpu import _CountBuilds
    from tgtc_style_amd import train_tgtcs
    base = ["--config", os.path.join(ROOT, "configs", "fern.txt"), "--synthetic", "--synthetic_hw", "40", "--synthetic_frames", "2",
            "--synthetic_styles", "2", "--chunk", "1024", "--batch_size", "512", "--precision", "fp16x3+fp16mx",
            "--render_valid_style", "--share_geometry", "--fold_latents"]
    mx = ["--style_precision", "fp16mx"]
    with pytest.raises(RuntimeError):
        train_tgtcs.main(base + ["--basedir", str(tmp_path / "refused"), "--cull_weight", "0"])
    one = _files(train_tgtcs.main(base + mx + ["--basedir", str(tmp_path / "one"), "--cull_weight", "0"]))
    assert len(one) == 8 and all(n.endswith(".png") and len(b) > 100 for n, b in one.items())
    import io
    from PIL import Image
    for name, blob in one.items():
        assert np.asarray(Image.open(io.BytesIO(blob))).any(), name
    assert one["style_00000_fine_00000.png"] != one["style_00001_fine_00000.png"]
    D = str(tmp_path / "geometry")
    with _CountBuilds() as n:
        first = _files(train_tgtcs.main(base + mx + ["--basedir", str(tmp_path / "first"), "--cull_weight", "0", "--geometry_cache", D]))
    assert n.calls == 2 and len(os.listdir(D)) == 2
    with _CountBuilds() as n:
        second = _files(train_tgtcs.main(base + mx + ["--basedir", str(tmp_path / "second"), "--geometry_cache", D]))
    assert n.calls == 0
    for got in (first, second):
        assert sorted(got) == sorted(one)
        for name in one:
            assert got[name] == one[name], name
