"""GPU: the folded restyle from a trunk plane with the style networks in fp16mx (tgtc_style_enable_mx,
tgtc_restyle_rays_trunk_folded_mx, csrc/mlp_style_mx.hip, RayRenderer.restyle(style_precision="fp16mx")).

1. Per sample against the oracle in float64 (oracle.fields._styled_pass with z_k broadcast to the rays, the planes of
   tests/test_fold_latents_gpu.py), through the entry point on a cache whose list is a seeded sample list of the (40, 129) grid
   and that list's fp16x3 plane; the colours before compositing are the workspace's rgb_live plane.  Lists that end inside, one
   short of, on and one behind a 128-sample tile and one behind two tiles; K = 1 and 3; weights `base`, `rows`, `dead`.
   Error: max|a - ref| / max|ref|.  Hard bar 1e-3, the TOL["fp16mx"] of tests/test_hip_nerf.py.  On every case the error is
   also below that of an fp16 style handle (fp16 plane, tgtc_restyle_rays_trunk_folded) on the same case.
   Every launch is a canary check too: every listed row is written, nothing else of the workspace's colour plane is.
2. Against the fp16x3 sibling on a composited image: t and the count bit for bit, rgb within TIGHT["fp16x3"] + 1e-3.
3. Bits of the mode: K latents = K calls, two calls, no table survives a latent, a tile or a call, one launch = launches over
   tile-aligned chunks small enough that no workgroup revisits, an empty list gives +0.
4. Rules on real handles; restyle() without the argument keeps its bits when the streams arrive.
5. The packing (tgtc_style_mx_read): every K group decodes (Wh exactly; Wl6 x 2^EL and Wh6 x 2^EH within the e2m3 grid's half
   step of the residual / of Wh) to the equalised weights, every P group exactly, the row exponents put the row's largest
   magnitude in [2, 8), padding is zero; over the `base`, `rows` and `dead` weights."""
import math

import numpy as np
import pytest
import torch

import test_fold_latents_gpu as F
import test_hip_style_shapes as S
from test_sparse_style_gpu import renderers

pytestmark = pytest.mark.gpu
BAR = 1e-3                                  # TOL["fp16mx"] of tests/test_hip_nerf.py
TIGHT_X3 = 5e-5                             # TIGHT["fp16x3"] of tests/test_hip_style.py
CANARY, SPARE = -7.0, 4096
GRID = F.BIG                                # (40, 129): 5 160 samples = 40.3 tiles of 128
NC, NF = 100, 29                            # n_coarse + n_fine = N of the grid
LIST_LENGTHS = [1, 17, 127, 128, 129, 257, None]     # None: every sample
LATENTS = ["a", "abf", "eda"]               # K = 1 and 3; e is the zero latent
WEIGHTS = ["base", "rows", "dead"]
CASES = [(n, fam, wf) for wf in WEIGHTS for n in LIST_LENGTHS for fam in LATENTS]


# ------------------------------------------------------------------------------------------------------- a cache from a list
def list_cache(ro, ts, live, nc, nf):
    """A geometry cache (the layout include/tgtc_hip.h documents) whose list is `live` (ascending sample indices of the grid
    ts [R,N]), on the device: ts_live = ts[live], seeded weights below 1 / N, depths t = 0."""
    from tgtc_style_amd.rendering import GeometryCache
    (R, N), count = ts.shape, live.numel()
    assert nc + nf == N
    c = GeometryCache(torch.zeros(GeometryCache.nbytes(R, count), dtype=torch.uint8), R, N, count, 0., None, nc, nf)
    c.header[:7] = torch.tensor([GeometryCache.MAGIC, GeometryCache.VERSION, R, 0, N, count, 0], dtype=torch.int32)
    lv = live.cpu().numpy()
    c.live[:] = live.cpu()
    c.ray_start[:] = torch.from_numpy(np.searchsorted(lv, np.arange(R + 1) * N).astype(np.int32))
    c.ts_live[:] = ts.reshape(-1)[live.long().cpu()]
    c.w_live[:] = torch.from_numpy(np.random.default_rng(5).uniform(0, 1. / N, count).astype(np.float32))
    c.buffer = c.buffer.cuda()
    return c


def build_plane(nerf, cache, ro, rd):
    """tgtc_geometry_trunk on `nerf` (a packed fine net); attaches the plane in that net's precision."""
    from tgtc_style_amd import hip
    lib = hip.load()
    p = nerf.packed()
    plane = torch.empty(cache.trunk_nbytes(p.precision, cache.count), dtype=torch.uint8, device="cuda")
    hip.check(lib.tgtc_geometry_trunk(p.handle, hip.ptr(ro), hip.ptr(rd), cache.R, cache.n_coarse, cache.n_fine,
                                      hip.ptr(cache.buffer), cache.buffer.numel(), cache.count, hip.ptr(plane), plane.numel(),
                                      hip.stream()))
    cache.attach_trunk(plane, p.precision)
    return cache


def raw_restyle(call, pair, cache, ro, rd, z):
    """One of tgtc_restyle_rays_trunk_folded[_mx] into a canary-filled workspace with SPARE bytes behind it.  Returns
    (rgb_live [K,count,3], rgb [K,R,3]); asserts that every row of rgb_live was written, that the padding behind it and the
    spare bytes were not."""
    from tgtc_style_amd import hip
    lib = hip.load()
    K, n = z.shape[0], cache.count
    need = lib.tgtc_restyle_folded_workspace_bytes(n, K)
    ws = torch.full(((need + SPARE) // 4,), CANARY, device="cuda")
    rgb, t = torch.empty(K, cache.R, 3, device="cuda"), torch.empty(cache.R, device="cuda")
    hip.check(call(pair.packed().handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(z), K, cache.R, cache.n_coarse, cache.n_fine,
                   hip.ptr(cache.buffer), cache.buffer.numel(), n, hip.ptr(cache.trunk), cache.trunk.numel(), hip.ptr(ws), need,
                   hip.ptr(rgb), hip.ptr(t), hip.stream()))
    torch.cuda.synchronize()
    plane_end = lib.tgtc_restyle_workspace_bytes(n, K) // 4             # the tables lie behind it
    live = ws[:K * n * 3].view(K, n, 3)
    assert bool((live != CANARY).all()), "a listed sample was left unwritten"
    assert bool((ws[K * n * 3:plane_end] == CANARY).all()) and bool((ws[need // 4:] == CANARY).all()), "wrote outside its planes"
    return live.clone(), rgb


_CACHES = {}


def grid_cache(p, n):
    """(cache with its plane in precision p, ro, rd) for the list of length n on GRID: built once per precision and length
    (the fine NeRF net is the same in every weight family)."""
    if (p, n) not in _CACHES:
        R, N = GRID
        ro, rd, ts, _ = S.ray_inputs(R, N, "a")
        ro, rd = S.on_gpu(ro, rd)
        cache = list_cache(ro, ts, F.sample_list(R * N, n), NC, NF)
        _CACHES[p, n] = (build_plane(S.networks(p, "base")[2], cache, ro, rd), ro, rd)
    return _CACHES[p, n]


def mx_pair(wf):
    pair = S.networks("fp16x3", wf)[3]
    pair.packed().enable_mx()
    return pair


def test_case_list_is_the_cross_product_the_kernel_can_get_wrong():
    assert len(CASES) == 63 and {len(f) for _, f, _ in CASES} == {1, 3} and "e" in "".join(LATENTS)
    assert {1, 17, 127, 128, 129, 257, None} == set(LIST_LENGTHS) and GRID[0] * GRID[1] > 2 * 128 and (GRID[0] * GRID[1]) % 128


# ------------------------------------------------------------------------------------------------------- 1: float64
@pytest.mark.parametrize("n,families,wf", CASES)
def test_mx_restyle_per_sample_vs_float64_and_vs_fp16(n, families, wf):
    from tgtc_style_amd import hip
    lib = hip.load()
    R, N = GRID
    idx = F.sample_list(R * N, n).long()
    ref = torch.stack([F.oracle_planes(wf, R, N, f)[0][idx] for f in families])
    z = F.latent_rows(families).cuda()
    cache, ro, rd = grid_cache("fp16x3", n)
    got, _ = raw_restyle(lib.tgtc_restyle_rays_trunk_folded_mx, mx_pair(wf), cache, ro, rd, z)
    cache16, _, _ = grid_cache("fp16", n)
    fast, _ = raw_restyle(lib.tgtc_restyle_rays_trunk_folded, S.networks("fp16", wf)[3], cache16, ro, rd, z)
    e, e16 = S.rel(got, ref), S.rel(fast, ref)
    print("fp16mx restyle list %-4s z(%-3s) %-5s err %.3e  fp16 err %.3e  ratio %8.1f  bar %.1e"
          % (n if n else "all", families, wf, e, e16, e16 / e if e else float("inf"), BAR))
    assert e <= BAR, (n, families, wf, e)
    assert e < e16, (n, families, wf, e, e16)


# ------------------------------------------------------------------------------------------------------- 2: the fp16x3 sibling
def test_mx_image_against_the_fp16x3_sibling():
    r, ro, rd, z, jit, nc, nf = F.small_render("fp16x3", 3, seed=12)
    cache = r.build_geometry(ro, rd, nc, nf, jitter=jit, keep_trunk=True)
    assert 0 < cache.count < F.RENDER[0] * (nc + nf) and bool((z.abs().max(-1).values > 1).all())
    a = r.restyle(cache, ro, rd, z)
    b = r.restyle(cache, ro, rd, z, style_precision="fp16mx")
    assert r.style.packed().has_mx()
    d = float((a["rgb"] - b["rgb"]).abs().max())
    print("fp16mx vs fp16x3 image: max |diff| %.3e (bar %.2e)" % (d, TIGHT_X3 + BAR))
    assert torch.equal(a["t"], b["t"]) and a["live"] == b["live"] == cache.count
    assert bool(a["rgb"].any()) and d <= TIGHT_X3 + BAR, d
    assert bool(torch.isfinite(b["rgb"]).all()) and float(b["rgb"].min()) >= 0. and float(b["rgb"].max()) <= 1.


# ------------------------------------------------------------------------------------------------------- 3: bits of the mode
def test_bits_of_the_mx_mode():
    r, ro, rd, z, jit, nc, nf = F.small_render("fp16x3", 3)
    cache = r.build_geometry(ro, rd, nc, nf, jitter=jit, keep_trunk=True)
    mx = lambda c, zz: r.restyle(c, ro, rd, zz.contiguous(), style_precision="fp16mx")
    out = mx(cache, z)
    rgb, t = out["rgb"].clone(), out["t"].clone()
    assert rgb.shape == (3, F.RENDER[0], 3) and bool(torch.isfinite(rgb).all()) and not torch.equal(rgb[0], rgb[1])
    # K = 3 is three K = 1 calls; two calls give equal bits
    for k in range(3):
        assert torch.equal(mx(cache, z[k:k + 1])["rgb"][0], rgb[k]), k
    assert torch.equal(mx(cache, z)["rgb"], rgb)
    # no table survives a latent, a tile or a call: the zero row in front of and behind a non-zero row
    zero = torch.zeros(1, 32, device="cuda")
    alone = mx(cache, zero)["rgb"][0].clone()
    eae = mx(cache, torch.cat([zero, z[:1], zero]))["rgb"]
    assert torch.equal(eae[0], alone) and torch.equal(eae[2], alone) and torch.equal(eae[1], rgb[0])
    assert not torch.equal(alone, rgb[0])
    mx(cache, 2 * z + 1)
    assert torch.equal(mx(cache, zero)["rgb"][0], alone)
    # the fp16x3 restyle of the same handle in between changes nothing either
    r.restyle(cache, ro, rd, z)
    assert torch.equal(mx(cache, z)["rgb"], rgb)
    # nothing live: colour +0 (not -0)
    empty = r.build_geometry(ro, rd, nc, nf, jitter=jit, min_weight=2., keep_trunk=True)
    e = mx(empty, z)
    assert empty.count == 0 and not bool(e["rgb"].any()) and not bool(torch.signbit(e["rgb"]).any()) and torch.equal(e["t"], t)


def test_mx_kernel_second_and_third_visit():
    """About 2.2 x n_cu tiles of 128 listed samples, K = 2: every persistent workgroup takes a second tile and some a third,
    reloading table 0 at each.  One launch against launches over chunks of n_cu whole tiles (tile boundaries coincide)."""
    from tgtc_style_amd import hip
    lib = hip.load()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    N = NC + NF
    R = math.ceil(2.2 * n_cu * 128 / N) + 1
    M = R * N
    M -= M % 128 == 0                                                   # a ragged last tile
    assert (M + 127) // 128 > 2 * n_cu
    ro, rd, ts, _ = S.ray_inputs(R, N, "a", seed=62000 + n_cu)
    ro, rd = S.on_gpu(ro, rd)
    z = F.latent_rows("ab").cuda()
    nerf, pair = S.networks("fp16x3", "base")[2], mx_pair("base")
    live = torch.arange(M, dtype=torch.int32)
    whole, _ = raw_restyle(lib.tgtc_restyle_rays_trunk_folded_mx, pair, build_plane(nerf, list_cache(ro, ts, live, NC, NF), ro, rd),
                           ro, rd, z)
    assert bool(torch.isfinite(whole).all()) and not torch.equal(whole[0], whole[1])
    chunk = n_cu * 128
    for i0 in range(0, M, chunk):
        part = build_plane(nerf, list_cache(ro, ts, live[i0:i0 + chunk].contiguous(), NC, NF), ro, rd)
        got, _ = raw_restyle(lib.tgtc_restyle_rays_trunk_folded_mx, pair, part, ro, rd, z)
        assert torch.equal(got, whole[:, i0:i0 + chunk]), "list entries %d.." % i0


# ------------------------------------------------------------------------------------------------------- 4: real handles
def test_mx_rules_on_real_handles():
    from tgtc_style_amd import hip, models, rendering
    lib = hip.load()
    r, _, nets, _ = renderers("fp16x3")
    pair = models.StylePair(r.style.concat_model, r.style.style_model)       # a handle of its own: nothing enabled yet
    r = rendering.RayRenderer(nets[0], nets[1], pair)
    R, nc, nf = F.RENDER
    _, ro, rd, z, jit, _, _ = F.small_render("fp16x3", 2)
    cache = r.build_geometry(ro, rd, nc, nf, jitter=jit, keep_trunk=True)
    s = pair.packed().handle
    assert not pair.packed().has_mx() and lib.tgtc_style_has_mx(nets[1].packed().handle) == 0
    before = r.restyle(cache, ro, rd, z)["rgb"].clone()
    before3 = r.restyle(cache, ro, rd, z[:, None, :].expand(-1, R, -1).contiguous())["rgb"].clone()
    # not enabled: the entry point refuses, the sibling runs
    ws = torch.empty(lib.tgtc_restyle_folded_workspace_bytes(cache.count, 2), dtype=torch.uint8, device="cuda")
    rgb, t = torch.empty(2, R, 3, device="cuda"), torch.empty(R, device="cuda")

    def call(style=s, K=2, R=R, ws_bytes=ws.numel(), plane_bytes=cache.trunk.numel(), zz=z):
        return lib.tgtc_restyle_rays_trunk_folded_mx(style, hip.ptr(ro), hip.ptr(rd), hip.ptr(zz), K, R, nc, nf,
                                                     hip.ptr(cache.buffer), cache.buffer.numel(), cache.count, hip.ptr(cache.trunk),
                                                     plane_bytes, hip.ptr(ws), ws_bytes, hip.ptr(rgb), hip.ptr(t), hip.stream())
    assert call() == -2 and b"no fp16mx streams" in lib.tgtc_last_error()
    # enabling: refused for an fp16 pair and for a NeRF handle, idempotent for an fp16x3 pair
    pair16 = renderers("fp16")[3]
    assert lib.tgtc_style_enable_mx(pair16.packed().handle, hip.stream()) == -2 and not pair16.packed().has_mx()
    with pytest.raises(RuntimeError):
        pair16.packed().enable_mx()
    assert lib.tgtc_style_enable_mx(nets[1].packed().handle, hip.stream()) == -1
    assert lib.tgtc_style_enable_mx(s, hip.stream()) == 0 and pair.packed().has_mx()
    assert lib.tgtc_style_enable_mx(s, hip.stream()) == 0 and pair.packed().has_mx()
    assert call() == 0 and call(R=0) == 0
    assert call(ws_bytes=ws.numel() - 1) == -1 and call(plane_bytes=cache.trunk.numel() - 1) == -1
    assert call(zz=None) == -1 and call(K=0) == -1 and call(style=nets[1].packed().handle) == -1
    assert call(style=pair16.packed().handle) == -2
    torch.cuda.synchronize()
    # the wrapper's refusals, before any launch
    with pytest.raises(ValueError):
        r.restyle(cache, ro, rd, z[:, None, :].expand(-1, R, -1).contiguous(), style_precision="fp16mx")      # 3-D zs
    bare = r.build_geometry(ro, rd, nc, nf, jitter=jit)
    with pytest.raises(ValueError):
        r.restyle(bare, ro, rd, z, style_precision="fp16mx")                                                  # no plane
    r16 = renderers("fp16")[0]
    plane16 = r16.build_geometry(ro, rd, nc, nf, jitter=jit, keep_trunk=True)
    with pytest.raises(ValueError):
        r.restyle(plane16, ro, rd, z, style_precision="fp16mx")                                               # an fp16 plane
    with pytest.raises(ValueError):
        r16.restyle(plane16, ro, rd, z, style_precision="fp16mx")                                             # an fp16 pair
    # the new streams touch nothing: restyle() without the argument returns the bits it returned before
    mx = r.restyle(cache, ro, rd, z, style_precision="fp16mx")["rgb"]
    assert torch.equal(r.restyle(cache, ro, rd, z)["rgb"], before) and not torch.equal(mx, before)
    assert torch.equal(r.restyle(cache, ro, rd, z[:, None, :].expand(-1, R, -1).contiguous())["rgb"], before3)
    assert torch.equal(r.restyle(cache, ro, rd, z, use_trunk=False)["rgb"], before)


# ------------------------------------------------------------------------------------------------------- 5: the packing
# (here and not in tests/test_restyle_mx_cpu.py: a style handle is made by tgtc_style_create, which needs a device)
RING, CHUNK, K_GROUP = 131072, 16384, 7168
# (row tiles, 128-deep blocks, encoding k-steps) and [out, in] of the 13 folded layers: concat 0..4, style 0..7
SHAPES = [(16, 0, 2)] + [(16, 2, 0)] * 3 + [(16, 2, 2), (16, 4, 2)] + [(16, 2, 0)] * 3 + [(16, 2, 2)] + [(16, 2, 0)] * 2 + [(1, 2, 0)]
DIMS = [(256, 95)] + [(256, 288)] * 3 + [(256, 351), (256, 607)] + [(256, 288)] * 3 + [(256, 351)] + [(256, 288)] * 2 + [(3, 288)]
PE_COL0 = {0: 0, 4: 288, 5: 512, 9: 288}            # first column of the encoding in the layer's input; activations start at 0
BIAS0 = [256 * l for l in range(5)] + [1280 + 256 * l for l in range(8)]


def group_table():
    """[(layer, row tile, group in the row tile, encoding k-steps or 0, byte offset)] and the streams' length: K groups of 7 KiB,
    P groups of 2 KiB per k-step, none across the end of the 128 KiB ring, the style MLP's first group on a chunk."""
    off, groups = 0, []
    for l, (rt, nkb, npe) in enumerate(SHAPES):
        if l == 5:
            off = -(-off // CHUNK) * CHUNK
        for r in range(rt):
            for q in range(nkb + (npe > 0)):
                n = 0 if q < nkb else npe
                size = 2048 * n if n else K_GROUP
                if off // RING != (off + size - 1) // RING:
                    off = (off // RING + 1) * RING
                groups.append((l, r, q, n, off))
                off += size
    return groups, -(-off // CHUNK) * CHUNK


def pe63_col(ks, g, j):
    """Column of the 63-wide encoding in k-step ks, lane group g, element j (csrc/mlp_core.h); -1: padding."""
    q, fn = 8 * g + 4 * ks + (j >> 1), j & 1
    if q < 30:
        return 3 + 6 * (q // 3) + 3 * fn + q % 3
    return fn if q == 30 else (2 if fn == 0 else -1)


def act_col(ks, g, j):
    return 32 * ks + (4 * g + j if j < 4 else 16 + 4 * g + (j - 4))


def e2m3(codes):
    e, m = (codes >> 3) & 3, (codes & 7).astype(np.float64)
    v = np.where(e == 0, m / 8, (1 + m / 8) * 2.0 ** (e - 1))
    return np.where(codes & 32, -v, v)


def half_step(a):
    """Half the e2m3 grid's step at scaled magnitude a; past the top code (7.5) the distance to it."""
    return np.where(a < 2, 0.0625, np.where(a < 4, 0.125, np.where(a <= 7.5, 0.25, a - 7.5)))


@pytest.mark.parametrize("wf", WEIGHTS)
def test_packed_groups_decode_to_the_equalised_weights(wf):
    from tgtc_style_amd import hip
    lib = hip.load()
    pair = mx_pair(wf)
    groups, total = group_table()
    assert len(groups) == 450
    raw, rowexp = np.zeros(total, np.uint8), np.zeros(4096, np.uint16)
    flat = np.zeros(sum(o * i for o, i in DIMS), np.float32)
    hip.check(lib.tgtc_style_mx_read(pair.packed().handle, raw.ctypes.data, raw.nbytes, rowexp.ctypes.data, rowexp.nbytes,
                                     flat.ctypes.data, flat.size))
    assert lib.tgtc_style_mx_read(pair.packed().handle, raw.ctypes.data, raw.nbytes - 1, rowexp.ctypes.data, rowexp.nbytes,
                                  flat.ctypes.data, flat.size) == -1
    W, at = [], 0
    for o, i in DIMS:
        w = np.zeros((256, i + 1), np.float32)              # rows past `out` and the padding column (-1) read as zero
        w[:o, :i] = flat[at:at + o * i].reshape(o, i)
        W.append(w)
        at += o * i
    lane = np.arange(64)
    m, g, j8 = lane % 16, lane // 16, np.arange(8)
    used = np.zeros(total, bool)
    worst = {"Wl6": 0., "Wh6": 0.}
    for l, r, q, npe, off in groups:
        rows = (16 * r + m)[:, None]
        if npe:
            used[off:off + 2048 * npe] = True
            for k in range(npe):
                cols = np.array([[pe63_col(k, gg, j) for j in j8] for gg in g])
                w = W[l][rows, np.where(cols < 0, -1, PE_COL0[l] + cols)]
                hi = w.astype(np.float16)
                lo = (w - hi.astype(np.float32)).astype(np.float16)
                got = raw[off + 2048 * k:off + 2048 * (k + 1)].view(np.uint16).reshape(2, 64, 8)
                assert np.array_equal(got[0], hi.view(np.uint16)) and np.array_equal(got[1], lo.view(np.uint16)), (l, r, k)
            continue
        used[off:off + K_GROUP] = True
        cols = np.array([[[act_col(4 * q + s, gg, j) for j in j8] for s in range(4)] for gg in g])      # [lane, s, j]
        w = W[l][rows[:, :, None], cols]
        hi = w.astype(np.float16)
        got = raw[off:off + 4096].view(np.uint16).reshape(4, 64, 8).transpose(1, 0, 2)
        assert np.array_equal(got, hi.view(np.uint16)), (l, r, q)
        lo = w - hi.astype(np.float32)                                                                      # exact in float32
        pieces = [raw[off + 4096 + 1024 * i:off + 4096 + 1024 * (i + 1)].reshape(64, 16) for i in range(3)]
        ex = rowexp[BIAS0[l] + 16 * r + m].astype(np.int32)
        for name, blob, want, E in (("Wl6", np.concatenate([pieces[0], pieces[1][:, :8]], 1), lo, (ex >> 8) - 127),
                                    ("Wh6", np.concatenate([pieces[1][:, 8:], pieces[2]], 1), hi.astype(np.float32), (ex & 255) - 127)):
            bits = np.unpackbits(np.ascontiguousarray(blob), axis=1, bitorder="little").reshape(64, 32, 6)
            codes = (bits.astype(np.int32) << np.arange(6)).sum(-1).reshape(64, 4, 8)                    # code 8 s + j
            scale = 2.0 ** E.astype(np.float64)[:, None, None]
            a = np.abs(want.astype(np.float64)) / scale
            err = np.abs(e2m3(codes) * scale - want) / scale
            assert bool((err <= half_step(a) * (1 + 1e-9)).all()), (name, l, r, q, float((err - half_step(a)).max()))
            worst[name] = max(worst[name], float((err / half_step(a).clip(0.0625)).max()))
    # the row exponents: the operand's top binade or one below, over all the row's activation columns
    for l, (rt, nkb, _) in enumerate(SHAPES):
        if not nkb:
            continue
        w = W[l][:16 * rt, :128 * nkb]
        hi = w.astype(np.float16).astype(np.float32)
        ex = rowexp[BIAS0[l]:BIAS0[l] + 16 * rt].astype(np.int32)
        for part, E in ((hi, (ex & 255) - 127), (w - hi, (ex >> 8) - 127)):
            top = np.abs(part).max(1).astype(np.float64)
            live = top > 0
            a = top[live] / 2.0 ** E[live]
            assert bool(((a >= 2) & (a < 8)).all()), (l, float(a.min()), float(a.max()))
    assert not raw[~used].any(), "padding between the groups is not zero"
    print("%-5s 450 groups decoded: fp16 parts exact; worst error / half step: Wl6 %.3f, Wh6 %.3f" % (wf, worst["Wl6"], worst["Wh6"]))
