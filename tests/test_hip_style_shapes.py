"""Shape and edge sweep of the stylised per-sample kernels (csrc/mlp_style.hip: concat_kernel, style_kernel,
styled_rays_kernel) against the oracle evaluated in float64.

`test_hip_style.py` meets the oracle at M = 1, 33, 128, 300 for the granular operators and at (R, N) = (7, 192) for the
fused kernel; everything above it (multi-latent, culled, restyle) is pinned to these kernels bit for bit.  This file sweeps
what that leaves out: M = tile - 1, tile, tile + 1 for the 64 / 128 / 256-sample tiles; fused shapes whose 16-sample column
tiles straddle rays (N no multiple of 16) and end inside a tile; a launch in which every persistent workgroup takes a second
and a third tile (the barrier before the ring refill, the prologue on a warm ring, re-use of the slab and of the bias tables);
latents whose mean is far from zero, constant, zero, or confined to one channel per lane group; weights with heavy-tailed
per-feature scales and with dead units (the r1 == 0 / r2 == 0 branches of EqualisedNet::run); the rows behind every output
(canaries); and the bit properties the kernel header promises (a sample does not depend on its tile mates, sigma is
optional, no state survives a call).

Reference: oracle/fields.py (concat_mlp, style_mlp, _styled_pass) with state dicts and inputs cast to float64.
Error: max|a - ref| / max|ref| per tensor.  Bars: the hard one is TIGHT of test_hip_style.py, unchanged and without the
x 2 that file grants ragged sizes.  On top, each fp16x3 case carries a regression guard tied to the reference, not to the
kernel: y = max(rel(float32 oracle, float64 oracle), 1.2e-7) is computed per case and tensor, and
err <= min(TIGHT, K[family] * y) is asserted.  K is one power of two per output family: the next one at or above 4 x the
worst err / y measured in that family on the MI355X ("The stylised per-sample sweep", has the table);
4 x because the same kernel at another tile shape legitimately sums in another order.  fp16 is held to its hard bar only.
Every error is printed."""
import math

import numpy as np
import pytest
import torch

from tgtc_style_amd import synth

pytestmark = pytest.mark.gpu
PRECISIONS = ["fp16x3", "fp16"]
TIGHT = {"fp16x3": 5e-5, "fp16": 1e-2}      # tests/test_hip_style.py
Y_FLOOR = 1.2e-7        # float32 epsilon: the yardstick of a case where the float32 and float64 oracles agree exactly
# err <= min(TIGHT, K * y) for fp16x3.  Worst err / y measured per family on the MI355X: concat_features
# 2.15, style rgb 2.26, fused rgb 3.29, fused sigma 2.72; K = the next power of two at or above 4 x that.  K * y stays below
# TIGHT in every case of this file (at most 2.4e-5), so the guard is the bar that binds.
K = {"concat": 16, "style": 16, "fused rgb": 16, "fused sigma": 16}

# Tiles (MlpCfg in csrc/mlp_style.hip): concat MLP and fused kernel 128 (fp16x3) / 256 (fp16) samples, style MLP 64 / 128.
TILE = {"concat": {"fp16x3": 128, "fp16": 256}, "style": {"fp16x3": 64, "fp16": 128}, "fused": {"fp16x3": 128, "fp16": 256}}
GRANULAR_M = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]
FUSED_SHAPES = [(1, 1), (1, 15), (3, 17), (5, 37), (2, 64), (9, 100), (40, 129), (7, 192), (3, 200)]
LATENT_FAMILIES = "abcdef"
WEIGHT_FAMILIES = ["base", "rows", "outliers", "dead"]
GRANULAR_CASES = ([(M, "a", "base") for M in GRANULAR_M] + [(257, f, "base") for f in LATENT_FAMILIES[1:]] +
                  [(257, "a", w) for w in WEIGHT_FAMILIES[1:]])
FUSED_CASES = ([(R, N, "a", "base") for R, N in FUSED_SHAPES] +
               [(R, N, f, "base") for R, N in ((5, 37), (7, 192)) for f in LATENT_FAMILIES[1:]] +
               [(9, 100, "a", w) for w in WEIGHT_FAMILIES[1:]])
BITS_SHAPE = (40, 129)  # ragged in every sense: N = 8 * 16 + 1, 5 160 samples = 40.3 / 20.2 tiles
REVISIT_N = 100
CANARY_ROWS, CANARY = 64, -7.0


def test_case_lists_cover_the_tile_edges():
    """Needs no arithmetic, but it guards the sweeps below: if MlpCfg in csrc/mlp_style.hip changes (waves, column tiles
    per wave: CfgExact / CfgFast, CfgExactNarrow / CfgFastNarrow), update TILE and the case lists with it."""
    assert {t for d in TILE.values() for t in d.values()} == {64, 128, 256}
    for tile in (64, 128, 256):
        assert {tile - 1, tile, tile + 1} <= set(GRANULAR_M), tile
    assert any(N % 16 and R * N > max(TILE["fused"].values()) for R, N in FUSED_SHAPES)
    assert BITS_SHAPE in FUSED_SHAPES and BITS_SHAPE[1] % 16 and (BITS_SHAPE[0] * BITS_SHAPE[1]) % 256
    assert {f for *_, f, w in FUSED_CASES} == set(LATENT_FAMILIES) == {f for _, f, w in GRANULAR_CASES}
    assert {w for *_, w in FUSED_CASES} == set(WEIGHT_FAMILIES) == {w for *_, w in GRANULAR_CASES}


# ------------------------------------------------------------------------------------------------------- helpers
def T(sd, dtype=torch.float32):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in sd.items()}


def rel(a, ref):
    a, ref = torch.as_tensor(a).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    assert bool(torch.isfinite(a).all()), "non-finite output"
    return float((a - ref).abs().max() / ref.abs().max())


def check(p, family, name, got, ref, y):
    """Hard bar TIGHT[p]; for fp16x3 the reference-tied guard K[family] * y as well.  Prints the figures of the table."""
    e = rel(got, ref)
    bar = min(TIGHT[p], K[family] * y) if p == "fp16x3" else TIGHT[p]
    print("%-6s %-11s %-34s err %.3e  y %.3e  err/y %8.2f  bar %.3e" % (p, family, name, e, y, e / y, bar))
    assert e <= bar, (p, family, name, e, y, bar)
    return e


class Args:
    use_viewdir, act_type = True, "relu"
    embed_freq_coor, embed_freq_dir = 10, 4
    netdepth = netdepth_fine = 8
    netwidth = netwidth_fine = 256
    style_D, vae_latent = 8, 32
    precision = "fp16x3"


# ------------------------------------------------------------------------------------------------------- weights
DEAD_ROWS = [0, 7, 100, 129, 255]       # rows (and bias) zeroed in hidden layers 1 and 2: r1 == 0 in EqualisedNet::run
DEAD_COLS = [3, 64, 130, 200, 254]      # features nobody reads, zeroed in the consumer of every other layer: r2 == 0


def dead_units(concat_sd, style_sd):
    """Both MLPs with dead units.  Hidden layers 1 and 2: DEAD_ROWS and their bias are zero (the unit outputs 0).  Every
    other equalised layer (concat 0 and 3, style 0 and 3..6): columns DEAD_COLS of its consumer are zero (the unit is
    ignored).  A different function from the base nets: the oracle runs on these dicts."""
    c = {k: v.copy() for k, v in concat_sd.items()}
    s = {k: v.copy() for k, v in style_sd.items()}
    for sd, last in ((c, 3), (s, 6)):
        for l in range(last + 1):
            if l in (1, 2):
                sd["layers.%d.weight" % l][DEAD_ROWS, :] = 0
                sd["layers.%d.bias" % l][DEAD_ROWS] = 0
            else:
                sd["layers.%d.weight" % (l + 1)][:, DEAD_COLS] = 0      # cat(h, latent[, x]): h in columns 0..255
    return c, s


_STATES = {}


def states(wf):
    """(nerf, concat, style) numpy state dicts of a weight family (cached).  'rows' / 'outliers' compute the base nets'
    function: that is asserted in float64 here, before any sweep trusts it."""
    if wf in _STATES:
        return _STATES[wf]
    from oracle import fields
    nerf, c0, s0 = synth.nerf_state(1), synth.concat_state(2), synth.style_state(3)
    if wf == "base":
        c, s = c0, s0
    elif wf == "dead":
        c, s = dead_units(c0, s0)
        for l in (1, 2):
            assert not c["layers.%d.weight" % l][DEAD_ROWS].any() and not s["layers.%d.weight" % l][DEAD_ROWS].any()
        assert not c["layers.4.weight"][:, DEAD_COLS].any() and not s["layers.7.weight"][:, DEAD_COLS].any()
    else:
        c, s = synth.heavy_tailed_style(c0, s0, 11, wf)
        x = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (64, 63)))
        z = torch.from_numpy(np.random.default_rng(2).standard_normal((64, 32)))
        cf0 = fields.concat_mlp(T(c0, torch.float64), x, z)["concat_features"]
        cf1 = fields.concat_mlp(T(c, torch.float64), x, z)["concat_features"]
        both = torch.cat([torch.from_numpy(np.random.default_rng(3).uniform(0, 1, (64, 256))), cf0], -1)
        r0 = fields.style_mlp(T(s0, torch.float64), x, both, z)["rgb"]
        r1 = fields.style_mlp(T(s, torch.float64), x, torch.cat([both[:, :256], cf1], -1), z)["rgb"]
        assert float((r0 - r1).abs().max()) <= 1e-9
        assert max(float(np.abs(s["layers.%d.weight" % l]).max() / np.abs(s0["layers.%d.weight" % l]).max()) for l in range(7)) >= 16
    _STATES[wf] = (nerf, c, s)
    return _STATES[wf]


_NETS = {}


def networks(p, wf):
    """(concat module, style module, fine NeRF, StylePair) on the GPU, constructed once per precision and weight family."""
    if (p, wf) not in _NETS:
        from tgtc_style_amd import models
        a = type("A", (Args,), {"precision": p})
        nerf, c, s = states(wf)
        if (p, "nerf") not in _NETS:
            m = models.StyleNerf(a, mode="fine")
            m.load_state_dict(T(nerf))
            _NETS[p, "nerf"] = m.cuda()
        cm, sm = models.StyleMLP_before_concat(a), models.StyleMLP_Wild_multilayers(a)
        cm.load_state_dict(T(c)), sm.load_state_dict(T(s))
        cm, sm = cm.cuda(), sm.cuda()
        _NETS[p, wf] = (cm, sm, _NETS[p, "nerf"], models.StylePair(cm, sm))
    return _NETS[p, wf]


# ------------------------------------------------------------------------------------------------------- inputs
def latents(family, rng, n):
    """[n, 32] float32, one latent per ray (fused) or per row (granular)."""
    if family == "a":
        z = rng.standard_normal((n, 32))
    elif family == "b":
        z = 1.5 + rng.standard_normal((n, 32))
    elif family == "c":
        z = 4.0 * rng.standard_normal((n, 32))
    elif family == "d":         # one constant per ray in all 32 channels, spread over [-2, 2]: mean(z) = z
        z = np.repeat(rng.permutation(np.linspace(-2.0, 2.0, n))[:, None], 32, 1)
    elif family == "e":
        z = np.zeros((n, 32))
    elif family == "f":         # one channel per lane group: channel 8 g + j_g, another j_g and value per ray
        z = np.zeros((n, 32))
        for g in range(4):
            z[np.arange(n), 8 * g + rng.integers(0, 8, n)] = rng.uniform(0.5, 3.0, n) * rng.choice([-1.0, 1.0], n)
    else:
        raise ValueError(family)
    return torch.from_numpy(z.astype(np.float32))


def granular_inputs(M, family):
    rng = np.random.default_rng(40000 + 16 * M + LATENT_FAMILIES.index(family))
    x = torch.from_numpy(rng.uniform(-1, 1, (M, 63)).astype(np.float32))
    conc = torch.from_numpy(np.maximum(rng.standard_normal((M, 512)), 0).astype(np.float32))
    return x, conc, latents(family, rng, M)


def ray_inputs(R, N, family, seed=None):
    """The rays of test_styled_forward_rays_vs_oracle: origin xy ~ U(-1, 1), z = -1; direction xy ~ U(-0.3, 0.3), z = 2;
    ts sorted U(0, 1) in float32."""
    rng = np.random.default_rng(50000 + 1000 * R + 8 * N + LATENT_FAMILIES.index(family) if seed is None else seed)
    ro = torch.from_numpy(np.concatenate([rng.uniform(-1, 1, (R, 2)), -np.ones((R, 1))], 1))
    rd = torch.from_numpy(np.concatenate([rng.uniform(-.3, .3, (R, 2)), 2 * np.ones((R, 1))], 1))
    ts = torch.from_numpy(np.sort(rng.uniform(0, 1, (R, N)).astype(np.float32), -1))
    return ro, rd, ts, latents(family, rng, R)


# ------------------------------------------------------------------------------------------------------- oracle
_ORACLE = {}     # case key -> ([float64 reference tensors], [yardstick per tensor]); shared by the two precisions


def oracle(key, fn):
    """fn(dtype) -> list of tensors of the oracle evaluated in `dtype`.  Returns the float64 results and, per tensor, the
    yardstick y = max(rel(float32 oracle, float64 oracle), Y_FLOOR)."""
    if key not in _ORACLE:
        with torch.no_grad():
            r64, r32 = fn(torch.float64), fn(torch.float32)
        assert all(t.dtype == torch.float64 for t in r64) and all(t.dtype == torch.float32 for t in r32)
        _ORACLE[key] = (list(r64), [max(rel(a, b), Y_FLOOR) for a, b in zip(r32, r64)])
    return _ORACLE[key]


def granular_oracle(M, family, wf):
    from oracle import fields
    x, conc, z = granular_inputs(M, family)
    _, c, s = states(wf)
    return oracle(("granular", M, family, wf),
                  lambda dt: [fields.concat_mlp(T(c, dt), x.to(dt), z.to(dt))["concat_features"],
                              fields.style_mlp(T(s, dt), x.to(dt), conc.to(dt), z.to(dt))["rgb"]])


def styled_oracle(key, wf, ro, rd, ts, z, ray_of=None, sample_of=None):
    """Per-sample (rgb, sigma) of the stylised chain.  With ray_of / sample_of (flat index lists): only those samples, each
    as a ray of one sample -- the oracle is per sample, so a subset is exact."""
    from oracle import fields
    nerf, c, s = states(wf)
    if ray_of is None:
        pts = ro[:, None, :] + ts[..., None].double() * rd[:, None, :]
        dirs, zz = rd[:, None, :].expand(-1, ts.shape[1], -1), z
    else:
        pts = (ro[ray_of] + ts[ray_of, sample_of][:, None].double() * rd[ray_of])[:, None, :]
        dirs, zz = rd[ray_of][:, None, :], z[ray_of]
    return oracle(key, lambda dt: list(fields._styled_pass(T(nerf, dt), T(c, dt), T(s, dt), pts, dirs, zz.to(dt), dtype=dt)))


# ------------------------------------------------------------------------------------------------------- launches
def canary_out(rows, *tail):
    return torch.full((rows + CANARY_ROWS,) + tail, CANARY, device="cuda")


def assert_canary(out, rows, what):
    assert torch.equal(out[rows:], torch.full_like(out[rows:], CANARY)), what + ": wrote behind its output"
    assert bool((out[:rows] != CANARY).all()), what + ": left part of its output unwritten"


def fused(p, wf, ro, rd, ts, z, want_sigma=True):
    """tgtc_styled_forward_rays through the C ABI on device tensors.  Every call is a canary check too: both outputs
    carry CANARY_ROWS more rows than the kernel may write."""
    from tgtc_style_amd import hip
    _, _, nerf, pair = networks(p, wf)
    R, N = ts.shape
    rgb = canary_out(R * N, 3)
    sigma = canary_out(R * N) if want_sigma else None
    hip.check(hip.load().tgtc_styled_forward_rays(nerf.packed().handle, pair.packed().handle, hip.ptr(ro), hip.ptr(rd),
                                                  hip.ptr(ts), hip.ptr(z), R, N, hip.ptr(rgb), hip.ptr(sigma), hip.stream()))
    torch.cuda.synchronize()
    assert_canary(rgb, R * N, "fused rgb (%d,%d)" % (R, N))
    if want_sigma:
        assert_canary(sigma, R * N, "fused sigma (%d,%d)" % (R, N))
    return rgb[:R * N].view(R, N, 3), sigma[:R * N].view(R, N) if want_sigma else None


def on_gpu(*tensors):
    return tuple(t.cuda().contiguous() for t in tensors)


# ------------------------------------------------------------------------------------------------------- 1: granular
@pytest.mark.parametrize("p", PRECISIONS)
@pytest.mark.parametrize("M,family,wf", GRANULAR_CASES)
def test_granular_operators(p, M, family, wf):
    """tgtc_concat_mlp_forward and tgtc_style_mlp_forward through the module wrappers: M around every tile size (64, 128,
    256), a different latent in every row, every latent and weight family at M = 257 (one sample in the last tile)."""
    cm, sm, _, _ = networks(p, wf)
    x, conc, z = on_gpu(*granular_inputs(M, family))
    (ref_c, ref_s), (y_c, y_s) = granular_oracle(M, family, wf)
    cf = cm(x=x, latent=z)["concat_features"]
    rgb = sm(x=x, concated=conc, latent=z)["rgb"]
    name = "M=%d z(%s) %s" % (M, family, wf)
    check(p, "concat", name, cf, ref_c, y_c)
    check(p, "style", name, rgb, ref_s, y_s)


# ------------------------------------------------------------------------------------------------------- 2: fused, small
@pytest.mark.parametrize("p", PRECISIONS)
@pytest.mark.parametrize("R,N,family,wf", FUSED_CASES)
def test_fused_kernel_small_shapes(p, R, N, family, wf):
    """tgtc_styled_forward_rays per sample: one sample, one partial column tile, column tiles that straddle two and three
    rays (N = 17, 37), N a multiple of 16 and of 64, launches that end inside a tile, every latent family at a straddling
    and at an aligned shape, every weight family."""
    ro, rd, ts, z = ray_inputs(R, N, family)
    (ref_rgb, ref_sig), (y_rgb, y_sig) = styled_oracle(("fused", R, N, family, wf), wf, ro, rd, ts, z)
    rgb, sigma = fused(p, wf, *on_gpu(ro, rd, ts, z))
    name = "(%d,%d) z(%s) %s" % (R, N, family, wf)
    check(p, "fused rgb", name, rgb, ref_rgb, y_rgb)
    check(p, "fused sigma", name, sigma, ref_sig, y_sig)


# ------------------------------------------------------------------------------------------------------- 3: revisits
def revisit_subset(M, n_cu):
    """Flat sample indices the oracle is evaluated on: for both tile sizes the whole of tile 0, tile n_cu - 1, tile n_cu (a
    workgroup's first revisit), the last full tile and the ragged last tile; an even stride over the rest."""
    parts = [torch.arange(0, 256)]
    for tile in (128, 256):
        parts.append(torch.arange((n_cu - 1) * tile, (n_cu + 1) * tile))
    parts.append(torch.arange((M // 256 - 1) * 256, M))
    fixed = torch.unique(torch.cat(parts))
    stride = torch.linspace(0, M - 1, 4200 - fixed.numel()).long()
    return torch.unique(torch.cat([fixed, stride]))


@pytest.mark.parametrize("p", PRECISIONS)
def test_fused_kernel_second_and_third_visit(p):
    """About 1.5 x n_cu x 256 samples: every persistent workgroup takes a second tile in fp16 (256-sample tiles) and a
    second and a third in fp16x3 (128).  Against float64 on a subset (>= 4 096 samples incl. the tiles around the first
    revisit and the ragged end), and bit for bit against the same rays rendered in chunks small enough that no workgroup
    loops."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    N = REVISIT_N
    R = math.ceil(1.5 * n_cu * 256 / N) + 7
    R += (R * N) % 128 == 0                         # the last tile is ragged at either tile size
    M = R * N
    tiles = (M + TILE["fused"][p] - 1) // TILE["fused"][p]
    assert tiles > n_cu, (tiles, n_cu)                     # otherwise nothing here loops and the case proves nothing
    ro, rd, ts, z = ray_inputs(R, N, "a", seed=60000 + n_cu)
    idx = revisit_subset(M, n_cu)
    assert idx.numel() >= 4096 and int(idx[-1]) == M - 1
    ray_of, sample_of = idx // N, idx % N
    (ref_rgb, ref_sig), (y_rgb, y_sig) = styled_oracle(("revisit", n_cu), "base", ro, rd, ts, z, ray_of, sample_of)
    d = on_gpu(ro, rd, ts, z)
    rgb, sigma = fused(p, "base", *d)
    name = "(%d,%d) %d tiles on %d CUs" % (R, N, tiles, n_cu)
    check(p, "fused rgb", name, rgb.reshape(M, 3)[idx.cuda()][:, None, :], ref_rgb, y_rgb)
    check(p, "fused sigma", name, sigma.reshape(M)[idx.cuda()][:, None], ref_sig, y_sig)
    # all samples: chunks of at most n_cu * 128 / N - 1 rays hold at most n_cu tiles of either size
    chunk = n_cu * 128 // N - 1
    assert chunk >= 1 and (chunk * N + 127) // 128 <= n_cu
    for r0 in range(0, R, chunk):
        rgb_c, sigma_c = fused(p, "base", *(t[r0:r0 + chunk].contiguous() for t in d))
        assert torch.equal(rgb_c, rgb[r0:r0 + chunk]), ("rgb of rays %d.." % r0, float((rgb_c - rgb[r0:r0 + chunk]).abs().max()))
        assert torch.equal(sigma_c, sigma[r0:r0 + chunk]), ("sigma of rays %d.." % r0, float((sigma_c - sigma[r0:r0 + chunk]).abs().max()))


# ------------------------------------------------------------------------------------------------------- 4: bit properties
@pytest.mark.parametrize("p", PRECISIONS)
def test_fused_kernel_bit_properties(p):
    """(i) rays permuted at random give the same bits, permuted (a sample does not depend on its tile mates, its lane or
    its wave); (ii) sigma = NULL gives the rgb bits of the call with sigma; (iii) the same call after a call on other rays
    and latents gives the same bits (no state in the slab, the ring or the handle)."""
    R, N = BITS_SHAPE
    d = on_gpu(*ray_inputs(R, N, "a"))
    rgb, sigma = fused(p, "base", *d)
    rgb, sigma = rgb.clone(), sigma.clone()
    perm = torch.from_numpy(np.random.default_rng(7).permutation(R)).cuda()
    assert not torch.equal(perm, torch.arange(R, device="cuda"))
    rgb_p, sigma_p = fused(p, "base", *(t[perm].contiguous() for t in d))
    assert torch.equal(rgb_p, rgb[perm]) and torch.equal(sigma_p, sigma[perm])
    rgb_n, none = fused(p, "base", *d, want_sigma=False)
    assert none is None and torch.equal(rgb_n, rgb)
    other = on_gpu(*ray_inputs(33, 77, "c"))
    fused(p, "base", *other)
    rgb_2, sigma_2 = fused(p, "base", *d)
    assert torch.equal(rgb_2, rgb) and torch.equal(sigma_2, sigma)


@pytest.mark.parametrize("p", PRECISIONS)
@pytest.mark.parametrize("M", [1, 257])
def test_granular_operators_leave_the_rows_behind_their_outputs(p, M):
    """The C ABI called directly with CANARY_ROWS more rows than it may write, filled with CANARY: those rows keep their
    bits, every element below M has changed and equals the wrapper's result.  (The fused kernel's outputs carry the same
    canary rows in every call of this file: fused().)"""
    from tgtc_style_amd import hip
    cm, sm, _, _ = networks(p, "base")
    lib = hip.load()
    x, conc, z = on_gpu(*granular_inputs(M, "a"))
    want_c = cm(x=x, latent=z)["concat_features"].clone()
    want_s = sm(x=x, concated=conc, latent=z)["rgb"].clone()
    out_c, out_s = canary_out(M, 256), canary_out(M, 3)
    hip.check(lib.tgtc_concat_mlp_forward(cm._packed().handle, hip.ptr(x), hip.ptr(z), M, hip.ptr(out_c), hip.stream()))
    hip.check(lib.tgtc_style_mlp_forward(sm._packed().handle, hip.ptr(x), hip.ptr(conc), hip.ptr(z), M, hip.ptr(out_s), hip.stream()))
    torch.cuda.synchronize()
    assert_canary(out_c, M, "concat M=%d" % M)
    assert_canary(out_s, M, "style M=%d" % M)
    assert torch.equal(out_c[:M], want_c) and torch.equal(out_s[:M], want_s)


@pytest.mark.parametrize("p", PRECISIONS)
def test_fused_kernel_leaves_the_rows_behind_its_outputs(p):
    """rgb [M + 64, 3] and sigma [M + 64] filled with CANARY at the ragged shape: the rows from M on keep their bits, every
    element below M has changed; with sigma = NULL as well."""
    R, N = BITS_SHAPE
    d = on_gpu(*ray_inputs(R, N, "a"))
    fused(p, "base", *d)                        # asserts both canaries
    fused(p, "base", *d, want_sigma=False)
