"""GPU: frame-constant latents folded into per-latent biases (tgtc_style_fold_latents, the FOLD instances of
csrc/mlp_style_sparse.hip, tgtc_styled_forward_list_folded / tgtc_render_rays_styled_sparse_folded / tgtc_restyle_rays_folded,
RayRenderer.render_latents / restyle with zs [K,32], --fold_latents).

1. Per sample against the oracle in float64 (oracle.fields._styled_pass with z_k broadcast to the rays), through the scattered
   seam, over lists that end inside, on and behind a tile, K = 1 and 3, five latent families, and weights with heavy-tailed row
   scales and dead units (a fold taken from unequalised rows fails those two).  Error: max|a - ref| / max|ref| per tensor.
   Hard bar: TIGHT of tests/test_hip_style.py.  fp16x3 also carries that suite's reference-tied guard err <= K_GUARD * y,
   y = max(rel(float32 oracle, float64 oracle), 1.2e-7), with the K = 16 of the `fused rgb` family of
   tests/test_hip_style_shapes.py (DESIGN.md section 4 has the measured err / y).
2. z = 0: the folded restyle is the unfolded restyle with zs = 0, bit for bit (the tables are the handle's own, and the k-step
   that was left out added exact zeros).
3. Bits of the mode itself: K latents = K calls, no table survives a latent, a tile or a call, restyle = render, t and the
   count are the unfolded ones, an empty list gives +0.
4. Every persistent workgroup revisits: one launch = launches over chunks small enough that no workgroup loops.
5. Against the unfolded render under non-zero latents: 2 x TIGHT on the composited image (each side is within TIGHT of
   float64 per sample by 1 and tests/test_hip_style_shapes.py, weights sum to at most 1, colours lie in [0,1]).
6. The CLI with and without --fold_latents."""
import math
import os

import numpy as np
import pytest
import torch

import test_hip_style_shapes as S
from test_sparse_style_gpu import render_inputs, renderers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = ["fp16x3", "fp16"]
TIGHT = {"fp16x3": 5e-5, "fp16": 1e-2}      # tests/test_hip_style.py
Y_FLOOR = 1.2e-7
K_GUARD = 16                                 # the `fused rgb` family of tests/test_hip_style_shapes.py
TILE = {"fp16x3": 128, "fp16": 256}
CANARY, CANARY_ROWS = -7.0, 64
BIG = (40, 129)                              # 5 160 samples = 40.3 / 20.2 tiles, N = 8 * 16 + 1
LIST_LENGTHS = [1, 17, 127, 128, 129, 257, None]     # None: every sample
SMALL = [(1, 1), (3, 17), (7, 192)]
WEIGHTED = (9, 100)

# (R, N, list length, latent families of the K rows, weight family)
ORACLE_CASES = ([(BIG[0], BIG[1], n, fam, "base") for n in LIST_LENGTHS for fam in ("a", "abf")] +
                [(R, N, None, fam, "base") for (R, N), one in zip(SMALL, "fde") for fam in (one, "eda")] +
                [(WEIGHTED[0], WEIGHTED[1], None, fam, wf) for wf in ("rows", "dead") for fam in ("a", "abf")])


def test_case_lists_cover_what_the_kernels_can_get_wrong():
    assert {len(fam) for *_, fam, _ in ORACLE_CASES} == {1, 3}
    assert {f for *_, fam, _ in ORACLE_CASES for f in fam} == set("abdef")      # normal, mean + 5, constant, zero, one hot
    # lists that end one short of, on and one behind a 128-sample tile, and one behind two of them (= one 256-sample tile)
    assert {1, 17, 127, 128, 129, 257} <= {n for _, _, n, _, _ in ORACLE_CASES if n}
    assert BIG[1] % 16 and (BIG[0] * BIG[1]) % 256 and BIG[0] * BIG[1] > 2 * 256
    assert {wf for *_, wf in ORACLE_CASES} == {"base", "rows", "dead"}


# ------------------------------------------------------------------------------------------------------- inputs
def latent_row(family):
    """One 32-vector per family: a seeded normal, b normal with mean + 5, d a non-zero constant, e zero, f one hot channel."""
    rng = np.random.default_rng(7100 + "abdef".index(family))
    if family == "a":
        z = rng.standard_normal(32)
    elif family == "b":
        z = 5.0 + rng.standard_normal(32)
    elif family == "d":
        z = np.full(32, -1.375)
    elif family == "e":
        z = np.zeros(32)
    else:
        z = np.zeros(32)
        z[19] = 2.5
    return torch.from_numpy(z.astype(np.float32))


def latent_rows(families):
    return torch.stack([latent_row(f) for f in families])


def sample_list(M, n):
    """n seeded sample indices out of M, ascending (None: all of them)."""
    if n is None:
        return torch.arange(M, dtype=torch.int32)
    return torch.from_numpy(np.sort(np.random.default_rng(8200 + n).choice(M, n, replace=False)).astype(np.int32))


_PLANES = {}


def oracle_planes(wf, R, N, family):
    """(float64, float32) oracle colours [R*N,3] of every sample of the grid under the family's latent broadcast to the rays:
    computed once per (weights, grid, latent), shared by the list lengths, K and the two precisions."""
    key = (wf, R, N, family)
    if key not in _PLANES:
        from oracle import fields
        nerf, c, s = S.states(wf)
        ro, rd, ts, _ = S.ray_inputs(R, N, "a")
        pts = ro[:, None, :] + ts[..., None].double() * rd[:, None, :]
        dirs = rd[:, None, :].expand(-1, N, -1)
        z = latent_row(family)[None, :].expand(R, -1)
        with torch.no_grad():
            out = [fields._styled_pass(S.T(nerf, dt), S.T(c, dt), S.T(s, dt), pts, dirs, z.to(dt), dtype=dt)[0].reshape(R * N, 3)
                   for dt in (torch.float64, torch.float32)]
        assert out[0].dtype == torch.float64 and out[1].dtype == torch.float32
        _PLANES[key] = out
    return _PLANES[key]


# ------------------------------------------------------------------------------------------------------- launches
def fold(pair, z):
    """tgtc_style_fold_latents: z [K,32] on the device -> the K tables (bytes)."""
    from tgtc_style_amd import hip
    lib = hip.load()
    K = z.shape[0]
    tables = torch.empty(lib.tgtc_style_folded_bytes(K), dtype=torch.uint8, device="cuda")
    hip.check(lib.tgtc_style_fold_latents(pair.packed().handle, hip.ptr(z), K, hip.ptr(tables), tables.numel(), hip.stream()))
    return tables


def list_folded(p, wf, ro, rd, ts, z, live):
    """tgtc_styled_forward_list_folded into canary-filled planes with CANARY_ROWS spare rows behind the last one.  Returns
    rgb [K,M,3]; asserts that every listed row was written and no other."""
    from tgtc_style_amd import hip
    _, _, nerf, pair = S.networks(p, wf)
    (R, N), K, M = ts.shape, z.shape[0], ts.numel()
    rgb = torch.full((K * M + CANARY_ROWS, 3), CANARY, device="cuda")
    n_live = torch.tensor(live.numel(), dtype=torch.int32, device="cuda")
    tables = fold(pair, z)
    hip.check(hip.load().tgtc_styled_forward_list_folded(nerf.packed().handle, pair.packed().handle, hip.ptr(ro), hip.ptr(rd),
                                                         hip.ptr(ts), hip.ptr(tables), K, R, N, hip.ptr(live), hip.ptr(n_live),
                                                         hip.ptr(rgb), hip.stream()))
    torch.cuda.synchronize()
    planes = rgb[:K * M].view(K, M, 3)
    listed = torch.zeros(M, dtype=torch.bool, device="cuda")
    listed[live.long()] = True
    assert bool((planes[:, listed] != CANARY).all()), "a listed sample was left unwritten"
    assert bool((planes[:, ~listed] == CANARY).all()) and bool((rgb[K * M:] == CANARY).all()), "wrote outside the list"
    return planes


# ------------------------------------------------------------------------------------------------------- 1: float64
@pytest.mark.parametrize("p", PRECISIONS)
@pytest.mark.parametrize("R,N,n,families,wf", ORACLE_CASES)
def test_folded_list_kernel_vs_float64(p, R, N, n, families, wf):
    M, K = R * N, len(families)
    ro, rd, ts, _ = S.ray_inputs(R, N, "a")
    live = sample_list(M, n)
    planes = [oracle_planes(wf, R, N, f) for f in families]
    idx = live.long()
    ref = torch.stack([p64[idx] for p64, _ in planes])
    y = max(S.rel(torch.stack([p32[idx] for _, p32 in planes]), ref), Y_FLOOR)
    got = list_folded(p, wf, *S.on_gpu(ro, rd, ts, latent_rows(families), live))[:, idx.cuda()]
    e = S.rel(got, ref)
    bar = min(TIGHT[p], K_GUARD * y) if p == "fp16x3" else TIGHT[p]
    print("%-6s folded rgb (%d,%d) list %s z(%s) %-5s err %.3e  y %.3e  err/y %8.2f  bar %.3e"
          % (p, R, N, n if n else "all", families, wf, e, y, e / y, bar))
    assert e <= bar, (p, R, N, n, families, wf, e, y, bar)


# ------------------------------------------------------------------------------------------------------- the small render
RENDER = (97, 32, 16)       # rays, coarse, fine samples


def small_render(p, K, seed=11):
    r, _, nets, pair = renderers(p)
    R, nc, nf = RENDER
    ro, rd, zs, jit = render_inputs(R, nc, K, seed=seed)
    return r, ro, rd, zs[:, 0, :].contiguous(), jit, nc, nf       # z [K,32]: the first ray's rows


# ------------------------------------------------------------------------------------------------------- 2: zero latent
@pytest.mark.parametrize("p", PRECISIONS)
def test_zero_latent_is_the_unfolded_restyle_bit_for_bit(p):
    r, ro, rd, _, jit, nc, nf = small_render(p, 2)
    R = RENDER[0]
    cache = r.build_geometry(ro, rd, nc, nf, jitter=jit)
    assert 0 < cache.count < R * (nc + nf)
    unfolded = r.restyle(cache, ro, rd, torch.zeros(2, R, 32, device="cuda"))
    folded = r.restyle(cache, ro, rd, torch.zeros(2, 32, device="cuda"))
    assert bool(unfolded["rgb"].any())
    assert torch.equal(folded["rgb"], unfolded["rgb"]), float((folded["rgb"] - unfolded["rgb"]).abs().max())
    assert torch.equal(folded["t"], unfolded["t"]) and folded["live"] == unfolded["live"]


# ------------------------------------------------------------------------------------------------------- 3: bits of the mode
@pytest.mark.parametrize("p", PRECISIONS)
def test_bits_of_the_folded_mode(p):
    r, ro, rd, z, jit, nc, nf = small_render(p, 3)
    R = RENDER[0]
    cache = r.build_geometry(ro, rd, nc, nf, jitter=jit)
    out = r.restyle(cache, ro, rd, z)
    rgb, t = out["rgb"].clone(), out["t"].clone()
    assert rgb.shape == (3, R, 3) and bool(torch.isfinite(rgb).all()) and not torch.equal(rgb[0], rgb[1])
    # K = 3 is three K = 1 calls
    for k in range(3):
        one = r.restyle(cache, ro, rd, z[k:k + 1].contiguous())
        assert torch.equal(one["rgb"][0], rgb[k]), k
    # no table survives a latent or a tile
    aba = r.restyle(cache, ro, rd, z[[0, 1, 0]].contiguous())["rgb"]
    assert torch.equal(aba[0], aba[2]) and torch.equal(aba[0], rgb[0]) and torch.equal(aba[1], rgb[1])
    # t and the count are the unfolded ones
    zs_full = z[:, None, :].expand(-1, R, -1).contiguous()
    unfolded = r.restyle(cache, ro, rd, zs_full)
    assert torch.equal(t, unfolded["t"]) and out["live"] == unfolded["live"] == cache.count
    # restyle = render at both thresholds; the render's t and count are the unfolded render's
    for tau in (0., 1e-3):
        c = cache if tau == 0. else r.build_geometry(ro, rd, nc, nf, jitter=jit, min_weight=tau)
        a = r.restyle(c, ro, rd, z)
        b = r.render_latents(ro, rd, nc, nf, jitter=jit, zs=z, min_weight=tau)
        u = r.render_latents(ro, rd, nc, nf, jitter=jit, zs=zs_full, min_weight=tau)
        assert torch.equal(a["rgb"], b["rgb"]) and torch.equal(a["t"], b["t"]), tau
        assert torch.equal(b["t"], u["t"]) and int(b["live"]) == int(u["live"]) == c.count
    # a second call after a call with other latents reproduces the first
    r.restyle(cache, ro, rd, (2 * z + 1).contiguous())
    assert torch.equal(r.restyle(cache, ro, rd, z)["rgb"], rgb)
    # nothing live: colour +0 (not -0), from the render and from an empty cache
    e = r.render_latents(ro, rd, nc, nf, jitter=jit, zs=z, min_weight=2.)
    assert int(e["live"]) == 0 and not bool(e["rgb"].any()) and not bool(torch.signbit(e["rgb"]).any())
    empty = r.build_geometry(ro, rd, nc, nf, jitter=jit, min_weight=2.)
    e = r.restyle(empty, ro, rd, z)
    assert empty.count == 0 and not bool(e["rgb"].any()) and not bool(torch.signbit(e["rgb"]).any()) and torch.equal(e["t"], t)
    # the shapes the wrappers refuse
    with pytest.raises(ValueError):
        r.restyle(cache, ro, rd, z[:, :16].contiguous())
    with pytest.raises(ValueError):
        r.render_latents(ro, rd, nc, nf, jitter=jit, zs=z)              # 2-D zs without a min_weight


# ------------------------------------------------------------------------------------------------------- 4: revisits
@pytest.mark.parametrize("p", PRECISIONS)
def test_folded_list_kernel_second_and_third_visit(p):
    """About 1.5 x n_cu x 256 listed samples, K = 2: every persistent workgroup takes a second tile (and a third in fp16x3),
    reloading table 0 at each.  One launch against launches over chunks of the list that hold at most n_cu tiles."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    N = S.REVISIT_N
    R = math.ceil(1.5 * n_cu * 256 / N) + 7
    R += (R * N) % 128 == 0
    M = R * N
    tiles = (M + TILE[p] - 1) // TILE[p]
    assert tiles > n_cu, (tiles, n_cu)                     # otherwise nothing here loops and the case proves nothing
    ro, rd, ts, _ = S.ray_inputs(R, N, "a", seed=61000 + n_cu)
    z = latent_rows("ab")
    d = S.on_gpu(ro, rd, ts, z)
    live = torch.arange(M, dtype=torch.int32, device="cuda")
    whole = list_folded(p, "base", *d, live)
    assert bool(torch.isfinite(whole).all()) and not torch.equal(whole[0], whole[1])
    chunk = n_cu * 128 - 37                                # at most n_cu tiles of either size, ragged
    for i0 in range(0, M, chunk):
        part = live[i0:i0 + chunk].contiguous()
        got = list_folded(p, "base", *d, part)
        assert torch.equal(got[:, i0:i0 + chunk], whole[:, i0:i0 + chunk]), "samples %d.." % i0


# ------------------------------------------------------------------------------------------------------- 5: the unfolded path
@pytest.mark.parametrize("p", PRECISIONS)
def test_folded_render_against_the_unfolded_render(p):
    r, ro, rd, z, jit, nc, nf = small_render(p, 3, seed=12)
    R = RENDER[0]
    assert bool((z.abs().max(-1).values > 1).all())
    zs_full = z[:, None, :].expand(-1, R, -1).contiguous()
    for tau in (0., 1e-3):
        a = r.render_latents(ro, rd, nc, nf, jitter=jit, zs=z, min_weight=tau)
        b = r.render_latents(ro, rd, nc, nf, jitter=jit, zs=zs_full, min_weight=tau)
        d = float((a["rgb"] - b["rgb"]).abs().max())
        print("%-6s folded vs unfolded image, min_weight %g: max |diff| %.3e (bar %.1e)" % (p, tau, d, 2 * TIGHT[p]))
        assert bool(b["rgb"].any()) and d <= 2 * TIGHT[p], (p, tau, d)
        assert torch.equal(a["t"], b["t"])


# ------------------------------------------------------------------------------------------------------- argument rules
def test_folded_argument_rules_on_real_handles():
    from tgtc_style_amd import hip
    lib = hip.load()
    r, _, nets, pair = renderers("fp16x3")
    R, nc, nf, K = 16, 64, 64, 2
    ro, rd, zs, _ = render_inputs(R, nc, K)
    z = zs[:, 0, :].contiguous()
    cache = r.build_geometry(ro, rd, nc, nf)
    n, cb = cache.count, cache.buffer.numel()
    assert n > 0
    need = lib.tgtc_restyle_folded_workspace_bytes(n, K)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rgb, t = torch.empty(K, R, 3, device="cuda"), torch.empty(R, device="cuda")
    c, f, s = nets[0].packed().handle, nets[1].packed().handle, pair.packed().handle

    def call(fine=f, style=s, K=K, R=R, cache_bytes=cb, count=n, ws_bytes=need, z=z, t_out=t):
        return lib.tgtc_restyle_rays_folded(fine, style, hip.ptr(ro), hip.ptr(rd), hip.ptr(z), K, R, nc, nf, hip.ptr(cache.buffer),
                                            cache_bytes, count, hip.ptr(ws), ws_bytes, hip.ptr(rgb), hip.ptr(t_out), hip.stream())
    assert call() == 0 and call(t_out=None) == 0 and call(R=0) == 0
    assert call(cache_bytes=cb - 1) == -1 and call(ws_bytes=need - 1) == -1 and call(z=None) == -1
    assert call(style=f) == -1 and call(fine=s) == -1
    _, _, nets16, _ = renderers("fp16")
    assert call(fine=nets16[1].packed().handle) == -1          # fine NeRF and style nets of different precisions
    tables = torch.empty(lib.tgtc_style_folded_bytes(K), dtype=torch.uint8, device="cuda")
    assert lib.tgtc_style_fold_latents(s, hip.ptr(z), K, hip.ptr(tables), tables.numel() - 1, hip.stream()) == -1
    assert lib.tgtc_style_fold_latents(f, hip.ptr(z), K, hip.ptr(tables), tables.numel(), hip.stream()) == -1      # a NeRF handle
    assert lib.tgtc_style_fold_latents(s, hip.ptr(z), K, hip.ptr(tables), tables.numel(), hip.stream()) == 0
    need_r = lib.tgtc_render_styled_sparse_folded_workspace_bytes(R, nc, nf, K)
    wsr = torch.empty(need_r, dtype=torch.uint8, device="cuda")

    def render(ws_bytes=need_r, style=s, coarse=c):
        return lib.tgtc_render_rays_styled_sparse_folded(coarse, f, style, hip.ptr(ro), hip.ptr(rd), hip.ptr(z), K, R, nc, nf, 0.,
                                                         1., None, 0., hip.ptr(wsr), ws_bytes, hip.ptr(rgb), hip.ptr(t), None,
                                                         hip.stream())
    assert render() == 0 and render(ws_bytes=need_r - 1) == -1 and render(style=f) == -1 and render(coarse=s) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------- 6: CLI
def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _pixels(blob):
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(blob))).astype(np.int32)


def test_cli_fold_latents(tmp_path):
    """--share_geometry --cull_weight 0 with and without --fold_latents: the same file names, depth PNGs byte for byte, colour
    PNGs within one 8-bit level (a change of <= 1e-4 can only move a value across one quantisation edge).  A third run with
    --geometry_cache --fold_latents reuses the cache files an unfolded run wrote."""
    from test_restyle_gpu import _CountBuilds
    from tgtc_style_amd import train_tgtcs
    base = ["--config", os.path.join(ROOT, "configs", "fern.txt"), "--synthetic", "--synthetic_hw", "40", "--synthetic_frames", "2",
            "--synthetic_styles", "2", "--chunk", "1024", "--batch_size", "512", "--render_valid_style", "--share_geometry"]
    plain = _files(train_tgtcs.main(base + ["--basedir", str(tmp_path / "plain"), "--cull_weight", "0"]))
    folded = _files(train_tgtcs.main(base + ["--basedir", str(tmp_path / "folded"), "--cull_weight", "0", "--fold_latents"]))
    assert len(plain) == 8 and sorted(folded) == sorted(plain)

    def same_images(got):
        worst = 0
        for name in plain:
            if "depth" in name:
                assert got[name] == plain[name], name
            else:
                a, b = _pixels(got[name]), _pixels(plain[name])
                assert a.shape == b.shape and a.any(), name
                worst = max(worst, int(np.abs(a - b).max()))
        assert worst <= 1, worst
        return worst
    print("colour PNGs, folded vs unfolded: worst 8-bit difference", same_images(folded))
    D = str(tmp_path / "geometry")
    with _CountBuilds() as n:
        train_tgtcs.main(base + ["--basedir", str(tmp_path / "first"), "--geometry_cache", D])
    assert n.calls == 2 and len(os.listdir(D)) == 2
    with _CountBuilds() as n:
        cached = _files(train_tgtcs.main(base + ["--basedir", str(tmp_path / "cached"), "--geometry_cache", D, "--fold_latents"]))
    assert n.calls == 0 and sorted(cached) == sorted(plain)
    same_images(cached)
    for name in plain:                          # the folded restyle is the folded render, bit for bit
        assert cached[name] == folded[name], name
