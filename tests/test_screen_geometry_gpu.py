"""GPU: the chain geometry of the culled stylised render and of the geometry cache (include/tgtc_hip.h, last
section): the ray-only half from the plain chain's passes, each screened where its handle's policy says so -- the coarse pass
as in the plain chain, the sigma-only fine pass through nerf_x3s_kernel<IN_LIST> (fp16x3) or the new
nerf_mx2_kernel<IN_LIST, false> (fp16mx).

Every comparison is BIT IDENTITY (torch.equal) unless said otherwise: a listed sample is the same column of the same MFMA
sequence on the same operands as in the dense launch, and a sample the list leaves out has sigma_exact < 0 while
|sigma_screen - sigma_exact| < margin, so relu() of what its plane entry holds is the +0 the dense pass gets.

1. The list kernel against the dense sigma-only launch, sentinels around it, two launches into one plane, argument rules.
2. Screened equals unscreened: caches and renders under the four screen settings.
3. The anchor: t is the plain chain's; restyle from a chain cache is the chain render.
4. Not vacuous: the counters rise, the shares are far from 1, a dense call raises nothing.
5. Edges: everything / nothing a candidate, a coarse list that does not fit, rays that leave the screen's box.
6. AUTO follows the landed shares through tgtc_screen_auto_decision(0, ...) and (2, ...).
7. The command line, every run a fresh child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tgtc_style_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAIRS = {"mx": ("fp16x3", "fp16mx"), "x3": ("fp16x3", "fp16x3")}
LIST_KINDS = ["empty", "one", "127", "128", "129", "all", "third"]
LIST_R, LIST_N = 37, [128, 192]
RENDER_R = [1, 130, 4097]
RENDER_COUNTS = [(128, 64), (64, 32)]
TAUS = [0.0, 1e-3]
SETTINGS = [False, (True, False), (False, True), True]          # the first is the reference of the other three
SENTINEL = -7.25
POSE = 5


def T(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


class Args:
    use_viewdir, act_type = True, "relu"
    embed_freq_coor, embed_freq_dir = 10, 4
    netdepth = netdepth_fine = 8
    netwidth = netwidth_fine = 256
    style_D, vae_latent = 8, 32
    precision = "fp16x3"


def make(pair, shift=(0.0, 0.0)):
    """The synthetic pair as tests/test_density_screen_gpu.py builds it, in the precisions of PAIRS[pair]; shift: added to the
    sigma head's bias of (coarse, fine)."""
    from tgtc_style_amd import models
    nets = []
    for (seed, mode), prec, b in zip(((0, "coarse"), (1, "fine")), PAIRS[pair], shift):
        m = models.StyleNerf(type("A", (Args,), {"precision": prec}), mode=mode)
        sd = T(synth.nerf_state(seed))
        sd["net.sigma_layer.bias"] = sd["net.sigma_layer.bias"] + float(b)
        m.load_state_dict(sd)
        nets.append(m.cuda())
    return nets


_nets, _style = {}, []


def nets_of(pair, shift=(0.0, 0.0)):
    if (pair, shift) not in _nets:
        _nets[pair, shift] = make(pair, shift)
    return _nets[pair, shift]


def style_pair():
    """The fp16x3 style pair: the partner of an fp16x3 fine handle, and of an fp16mx one under style_precision="fp16mx"."""
    if not _style:
        from tgtc_style_amd import models
        cm = models.StyleMLP_before_concat(Args)
        cm.load_state_dict(T(synth.concat_state(2)))
        sm = models.StyleMLP_Wild_multilayers(Args)
        sm.load_state_dict(T(synth.style_state(3)))
        _style.append(models.StylePair(cm.cuda(), sm.cuda()))
    return _style[0]


def renderer(pair, screen, shift=(0.0, 0.0), nets=None):
    from tgtc_style_amd import rendering
    nets = nets or nets_of(pair, shift)
    return rendering.RayRenderer(nets[0], nets[1], style_pair(), screen=screen)


_frame = []


def frame_rays(R):
    """R rays spread evenly over the 400 x 400 frame of spiral_pose(POSE)."""
    from tgtc_style_amd import utils
    if not _frame:
        _frame.append(utils.gen_rays(400, 400, synth.fern_intrinsics(400, 400), synth.spiral_pose(POSE)))
    o, d = _frame[0]
    step = 160000 // R
    return o[::step][:R].contiguous(), d[::step][:R].contiguous()


def inputs(R, nc, K=2, seed=17):
    """(ro, rd, zs [K,32], zs [K,R,32], jitter [R,nc])"""
    ro, rd = frame_rays(R)
    rng = np.random.default_rng(seed)
    z = torch.from_numpy(rng.standard_normal((K, 32)).astype(np.float32)).cuda()
    zr = torch.from_numpy(rng.standard_normal((K, R, 32)).astype(np.float32)).cuda()
    jit = torch.from_numpy(rng.uniform(0, 1, (R, nc)).astype(np.float32)).cuda()
    return ro, rd, z, zr, jit


def forms(pair):
    """name -> (which latents, keyword arguments) of the render forms the pair has"""
    if pair == "mx":
        return {"fp16mx": ("folded", {"style_precision": "fp16mx"})}
    return {"folded": ("folded", {}), "per-ray": ("rays", {})}


def same(a, b, what=""):
    """the same bits where not NaN, NaN in the same places"""
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.is_floating_point():
        assert torch.equal(torch.isnan(a), torch.isnan(b)), what
        a, b = torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)
    assert torch.equal(a, b), what


CACHE_PLANES = ("header", "t", "ray_start", "live", "ts_live", "w_live")


def same_cache(a, b, what=""):
    assert (a.R, a.N, a.count) == (b.R, b.N, b.count), (what, a.count, b.count)
    for name in CACHE_PLANES:
        same(getattr(a, name), getattr(b, name), (what, name))
    assert torch.equal(a.buffer, b.buffer), what


def run_all(pair, R, nc, nf, tau, screen, shift=(0.0, 0.0), near=0., far=1., nets=None):
    """(cache, {form: outputs}) of build_geometry and render_latents under geometry="chain" with this screen setting"""
    ro, rd, z, zr, jit = inputs(R, nc)
    r = renderer(pair, screen, shift, nets)
    cache = r.build_geometry(ro, rd, nc, nf, near=near, far=far, jitter=jit, min_weight=tau, geometry="chain")
    outs = {}
    for name, (lat, kw) in forms(pair).items():
        out = r.render_latents(ro, rd, nc, nf, near=near, far=far, jitter=jit, zs=z if lat == "folded" else zr, min_weight=tau,
                               geometry="chain", **kw)
        torch.cuda.synchronize()
        outs[name] = {k: v.clone() for k, v in out.items()}
    return cache, outs


def same_runs(a, b, what=""):
    same_cache(a[0], b[0], what)
    assert sorted(a[1]) == sorted(b[1])
    for name in a[1]:
        assert sorted(a[1][name]) == ["live", "rgb", "t"]
        for k in ("rgb", "t", "live"):
            same(a[1][name][k], b[1][name][k], (what, name, k))


def counters(nets):
    return tuple(m.packed().screened_renders() for m in nets)


# ------------------------------------------------------------------------------------------------ 1: the list kernel
def make_list(kind, M, seed=3):
    if kind == "empty":
        idx = np.zeros(0, np.int64)
    elif kind == "one":
        idx = np.array([M // 2])
    elif kind in ("127", "128", "129"):
        idx = np.sort(np.random.default_rng(int(kind) + seed).choice(M, int(kind), replace=False))
    elif kind == "all":
        idx = np.arange(M)
    else:
        idx = np.sort(np.random.default_rng(seed).choice(M, M // 3, replace=False))     # an ascending random third
    return torch.from_numpy(idx.astype(np.int32)).cuda()


_dense = {}


def dense_sigma(n):
    """(fine fp16mx handle, (ro, rd, ts), sigma) of the dense sigma-only launch over LIST_R rays x n depths: computed once"""
    if n not in _dense:
        from tgtc_style_amd import hip
        net = nets_of("mx")[1].packed()
        ro, rd = frame_rays(LIST_R)
        ts = torch.from_numpy(np.sort(np.random.default_rng(n).uniform(0, 1, (LIST_R, n)).astype(np.float32), -1)).cuda()
        sigma = torch.full((LIST_R * n,), float("nan"), device="cuda")
        hip.check(hip.load().tgtc_nerf_forward_rays(net.handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), LIST_R, n, None,
                                                    hip.ptr(sigma), hip.stream()))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(sigma).all()) and float(sigma.std()) > 0
        _dense[n] = (net, (ro, rd, ts), sigma)
    return _dense[n]


def launch_list(net, rays, n, live, out):
    from tgtc_style_amd import hip
    ro, rd, ts = rays
    count = live.numel()
    buf = live if count else torch.zeros(1, dtype=torch.int32, device="cuda")
    n_live = torch.tensor([count], dtype=torch.int32, device="cuda")
    hip.check(hip.load().tgtc_nerf_sigma_list_mx(net.handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), LIST_R, n, hip.ptr(buf),
                                                 hip.ptr(n_live), hip.ptr(out), hip.stream()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", LIST_N)
@pytest.mark.parametrize("kind", LIST_KINDS)
def test_sigma_list_mx_kernel_bits_of_the_rays_kernel(kind, n):
    net, rays, sigma_dense = dense_sigma(n)
    M = LIST_R * n
    live = make_list(kind, M)
    out = torch.full((M + 64,), SENTINEL, device="cuda")
    launch_list(net, rays, n, live, out)
    listed = torch.zeros(M + 64, dtype=torch.bool, device="cuda")
    listed[live.long()] = True
    assert int(listed.sum()) == live.numel()
    assert torch.equal(out[:M][listed[:M]], sigma_dense[listed[:M]])
    assert bool((out[~listed] == SENTINEL).all())            # unlisted entries and the 64 words behind the plane
    # a second launch over another list into the same plane: the first list's entries stay, the second's are written
    other = make_list("third", M, seed=11)
    launch_list(net, rays, n, other, out)
    listed[other.long()] = True
    assert torch.equal(out[:M][listed[:M]], sigma_dense[listed[:M]])
    assert bool((out[~listed] == SENTINEL).all())


def test_sigma_list_mx_is_the_full_kernels_sigma():
    """the two-phase fine pass relies on it: sigma of the FULL launch (colour and density) = sigma of the sigma-only launches"""
    from tgtc_style_amd import hip
    n = 192
    net, (ro, rd, ts), sigma_dense = dense_sigma(n)
    rgb = torch.empty(LIST_R * n, 3, device="cuda")
    sigma = torch.empty(LIST_R * n, device="cuda")
    hip.check(hip.load().tgtc_nerf_forward_rays(net.handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), LIST_R, n, hip.ptr(rgb),
                                                hip.ptr(sigma), hip.stream()))
    torch.cuda.synchronize()
    assert torch.equal(sigma, sigma_dense)


def test_sigma_list_mx_argument_rules():
    from tgtc_style_amd import hip
    lib = hip.load()
    mx = nets_of("mx")[1].packed()
    x3 = nets_of("mx")[0].packed()
    fp16 = make_fp16().packed()
    n = 16
    ro, rd = frame_rays(7)
    ts = torch.linspace(0, 1, n, device="cuda").repeat(7, 1).contiguous()
    live = make_list("one", 7 * n)
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    sig = torch.zeros(7 * n, device="cuda")
    args = (hip.ptr(ro), hip.ptr(rd), hip.ptr(ts))
    call = lib.tgtc_nerf_sigma_list_mx
    assert call(mx.handle, *args, 7, n, hip.ptr(live), hip.ptr(one), hip.ptr(sig), hip.stream()) == 0
    assert call(mx.handle, *args, 0, n, None, None, None, hip.stream()) == 0
    assert call(mx.handle, *args, 7, n, hip.ptr(live), None, hip.ptr(sig), hip.stream()) == -1
    assert call(x3.handle, *args, 7, n, hip.ptr(live), hip.ptr(one), hip.ptr(sig), hip.stream()) == -2
    assert call(fp16.handle, *args, 7, n, hip.ptr(live), hip.ptr(one), hip.ptr(sig), hip.stream()) == -2
    assert call(mx.handle, *args, 1 << 40, n, hip.ptr(live), hip.ptr(one), hip.ptr(sig), hip.stream()) == -2
    assert call(mx.handle, *args, 1 << 27, n, hip.ptr(live), hip.ptr(one), hip.ptr(sig), hip.stream()) == -2      # R x N = 2^31
    # tgtc_nerf_sigma_list keeps refusing fp16mx
    assert lib.tgtc_nerf_sigma_list(mx.handle, *args, 7, n, hip.ptr(live), hip.ptr(one), hip.ptr(sig), hip.stream()) == -2
    torch.cuda.synchronize()


def make_fp16():
    from tgtc_style_amd import models
    m = models.StyleNerf(type("A", (Args,), {"precision": "fp16"}), mode="fine")
    m.load_state_dict(T(synth.nerf_state(1)))
    return m.cuda()


# ------------------------------------------------------------------------------------------------ 2: screened = unscreened
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("nc,nf", RENDER_COUNTS)
@pytest.mark.parametrize("R", RENDER_R)
def test_screened_geometry_bits_of_the_unscreened_one(R, nc, nf, pair, tau):
    off = run_all(pair, R, nc, nf, tau, SETTINGS[0])
    assert off[0].R == R and off[0].N == nc + nf and off[0].count < R * (nc + nf)
    for out in off[1].values():
        assert out["rgb"].shape == (2, R, 3) and bool(torch.isfinite(out["rgb"]).all())
        assert int(out["live"]) == off[0].count
        if R > 1:                                                 # (the one ray of R = 1 is a corner pixel: it may see nothing)
            assert off[0].count > 0 and bool(out["rgb"].any())
    for screen in SETTINGS[1:]:
        same_runs(run_all(pair, R, nc, nf, tau, screen), off, (R, nc, nf, pair, tau, screen))


# ------------------------------------------------------------------------------------------------ 3: the anchor
@pytest.mark.parametrize("pair", list(PAIRS))
def test_depths_are_the_plain_chains_and_restyle_is_the_render(pair):
    from tgtc_style_amd import rendering
    R, nc, nf = 4097, 128, 64
    ro, rd, z, zr, jit = inputs(R, nc)
    nets = nets_of(pair)
    plain = rendering.RayRenderer(nets[0], nets[1], fused=False, screen=False, cull=False).render(ro, rd, nc, nf, jitter=jit)
    torch.cuda.synchronize()
    t_plain = plain["t"].clone()
    r = renderer(pair, True)
    name, (lat, kw) = sorted(forms(pair).items())[0]
    zs = z if lat == "folded" else zr
    out = r.render_latents(ro, rd, nc, nf, jitter=jit, zs=zs, min_weight=0, geometry="chain", **kw)
    assert torch.equal(out["t"], t_plain), float((out["t"] - t_plain).abs().max())
    cache = r.build_geometry(ro, rd, nc, nf, jitter=jit, min_weight=0, geometry="chain")
    assert torch.equal(cache.t, t_plain)
    again = r.restyle(cache, ro, rd, zs, **kw)
    assert torch.equal(again["rgb"], out["rgb"]) and torch.equal(again["t"], out["t"]) and again["live"] == int(out["live"])
    # the geometry the call has without the argument is another one: its depths come from the ray kernel's first half
    other = r.render_latents(ro, rd, nc, nf, jitter=jit, zs=zs, min_weight=0, **kw)
    print("t: chain geometry vs ray-kernel geometry, max |difference| %.3e on %d rays" % (float((other["t"] - out["t"]).abs().max()), R))


# ------------------------------------------------------------------------------------------------ 4: not vacuous
@pytest.mark.parametrize("pair", list(PAIRS))
def test_the_screens_run_and_leave_most_samples_out(pair):
    R, nc, nf = 4097, 128, 64
    ro, rd, z, zr, jit = inputs(R, nc)
    nets = nets_of(pair)
    name, (lat, kw) = sorted(forms(pair).items())[0]
    zs = z if lat == "folded" else zr
    r = renderer(pair, True)
    before = counters(nets)
    r.build_geometry(ro, rd, nc, nf, jitter=jit, geometry="chain")
    torch.cuda.synchronize()
    assert counters(nets) == (before[0] + 1, before[1] + 1)
    r.render_latents(ro, rd, nc, nf, jitter=jit, zs=zs, min_weight=0, geometry="chain", **kw)
    torch.cuda.synchronize()
    assert counters(nets) == (before[0] + 2, before[1] + 2)
    shares = [m.packed().screen_fraction() for m in nets]
    print(pair, "candidate shares (coarse, fine)", shares)
    assert 0 < shares[0] < 0.6 and 0 < shares[1] < 0.6
    off = renderer(pair, False)
    off.build_geometry(ro, rd, nc, nf, jitter=jit, geometry="chain")
    off.render_latents(ro, rd, nc, nf, jitter=jit, zs=zs, min_weight=0, geometry="chain", **kw)
    torch.cuda.synchronize()
    assert counters(nets) == (before[0] + 2, before[1] + 2)


# ------------------------------------------------------------------------------------------------ 5: edges
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("shift,share", [(-1000.0, 0.0), (1000.0, 1.0)])
def test_nothing_and_everything_a_candidate(shift, share, pair):
    R, nc, nf = 130, 128, 64
    nets = nets_of(pair, (shift, shift))
    off = run_all(pair, R, nc, nf, 0.0, False, (shift, shift))
    before = counters(nets)
    on = run_all(pair, R, nc, nf, 0.0, True, (shift, shift))
    assert counters(nets) == (before[0] + 1 + len(forms(pair)), before[1] + 1 + len(forms(pair)))
    assert all(m.packed().screen_margin() > 0 for m in nets)
    assert [m.packed().screen_fraction() for m in nets] == [share, share]
    same_runs(on, off, (shift, pair))
    if share == 0.0:
        assert on[0].count == 0 and all(int(o["live"]) == 0 for o in on[1].values())      # empty lists, zero weights, live = 0
    else:
        assert on[0].count > 0


@pytest.mark.parametrize("pair", list(PAIRS))
def test_a_coarse_list_that_does_not_fit_runs_dense(pair):
    from tgtc_style_amd import hip
    R, nc, nf = 5, 16, 8
    assert hip.load().tgtc_screen_list_fits(R * (nc + nf) * 12, R * nc) == 0
    nets = nets_of(pair)
    off = run_all(pair, R, nc, nf, 0.0, False)
    before = counters(nets)
    on = run_all(pair, R, nc, nf, 0.0, True)
    runs = 1 + len(forms(pair))
    assert counters(nets) == (before[0], before[1] + runs)        # the fine list always fits its own plane
    same_runs(on, off, pair)


@pytest.mark.parametrize("pair", list(PAIRS))
def test_rays_that_leave_the_screens_box(pair):
    R, nc, nf = 130, 128, 64
    nets = nets_of(pair)
    off = run_all(pair, R, nc, nf, 0.0, False, near=0., far=3.)
    before = counters(nets)
    on = run_all(pair, R, nc, nf, 0.0, True, near=0., far=3.)
    runs = 1 + len(forms(pair))
    assert counters(nets) == (before[0] + runs, before[1] + runs)
    same_runs(on, off, pair)
    ro, rd, _, _, _ = inputs(R, nc)
    assert float((ro + 3.0 * rd).abs().max()) > 2.0               # the far end is outside |p| <= 2


# ------------------------------------------------------------------------------------------------ 6: AUTO
@pytest.mark.parametrize("pair", list(PAIRS))
def test_auto_follows_the_landed_shares(pair):
    from tgtc_style_amd import hip
    lib = hip.load()
    R, nc, nf = 4097, 128, 64
    nt = nc + nf
    off = run_all(pair, R, nc, nf, 0.0, False)
    nets = make(pair)                                             # fresh handles: nothing has landed
    ro, rd, z, zr, jit = inputs(R, nc)
    r = renderer(pair, None, nets=nets)
    first = r.build_geometry(ro, rd, nc, nf, jitter=jit, geometry="chain")
    torch.cuda.synchronize()
    assert counters(nets) == (0, 0)                               # shares unknown: dense
    assert all(m.packed().screen_margin() > 0 for m in nets)      # enabled by the call
    cs, fs = (m.packed().screen_fraction() for m in nets)
    print(pair, "landed candidate shares: coarse %.4f fine %.4f" % (cs, fs))
    assert 0 < cs < 1 and 0 < fs < 1
    want = (lib.tgtc_screen_auto_decision(0, round(cs * R * nc), R * nc), lib.tgtc_screen_auto_decision(2, round(fs * R * nt), R * nt))
    second = run_all(pair, R, nc, nf, 0.0, None, nets=nets)
    runs = 1 + len(forms(pair))
    assert counters(nets) == (want[0] * runs, want[1] * runs), (counters(nets), want)
    same_cache(first, off[0], pair)
    same_runs(second, off, pair)


# ------------------------------------------------------------------------------------------------ 7: the command line
CLI = ["--config", os.path.join(ROOT, "configs", "fern.txt"), "--synthetic", "--synthetic_hw", "40", "--synthetic_frames", "1",
       "--synthetic_styles", "2", "--chunk", "1024", "--batch_size", "1600", "--render_valid_style", "--share_geometry",
       "--fold_latents", "--cull_weight", "0"]


def cli(argv):
    """train_tgtcs.main(argv) in a fresh child process under a time limit; the output directory it printed"""
    code = "import sys; sys.path.insert(0, %r); from tgtc_style_amd import train_tgtcs; print('OUT=' + train_tgtcs.main(sys.argv[1:]))" % ROOT
    r = subprocess.run([sys.executable, "-c", code] + argv, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("OUT=")][-1]


def pngs(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def cache_files(d):
    return {n: (os.stat(os.path.join(d, n)).st_mtime_ns, torch.load(os.path.join(d, n), map_location="cpu")["key"])
            for n in sorted(os.listdir(d))}


def test_cli_chain_geometry_with_and_without_the_cache(tmp_path):
    gdir = str(tmp_path / "geometry")
    a = pngs(cli(CLI + ["--chain_geometry", "--basedir", str(tmp_path / "a")]))
    b = pngs(cli(CLI + ["--chain_geometry", "--basedir", str(tmp_path / "b"), "--geometry_cache", gdir]))
    assert sorted(a) == ["style_%05d_fine_%s00000.png" % (s, d) for s in (0, 1) for d in ("", "depth_")]
    assert a == b
    built = cache_files(gdir)
    assert len(built) == 1
    c = pngs(cli(CLI + ["--chain_geometry", "--basedir", str(tmp_path / "c"), "--geometry_cache", gdir]))
    assert c == a and cache_files(gdir) == built                  # the second run reuses the file
    cli(CLI + ["--basedir", str(tmp_path / "d"), "--geometry_cache", gdir])
    other = cache_files(gdir)
    assert sorted(other) == sorted(built)                         # the same file name, another key: rebuilt, not loaded
    for n in built:
        assert other[n][1] != built[n][1] and other[n][0] != built[n][0]


def test_case_lists_reach_the_shapes_named():
    assert LIST_KINDS == ["empty", "one", "127", "128", "129", "all", "third"] and LIST_R == 37 and LIST_N == [128, 192]
    for kind, count in (("empty", 0), ("one", 1), ("127", 127), ("128", 128), ("129", 129), ("all", 37 * 128), ("third", 37 * 128 // 3)):
        live = make_list(kind, 37 * 128).cpu().numpy()
        assert len(live) == count and (np.diff(live) > 0).all() and (len(live) == 0 or (0 <= live[0] and live[-1] < 37 * 128))
    assert RENDER_R == [1, 130, 4097] and RENDER_COUNTS == [(128, 64), (64, 32)] and TAUS == [0.0, 1e-3]
    assert SETTINGS == [False, (True, False), (False, True), True] and sorted(PAIRS) == ["mx", "x3"]
