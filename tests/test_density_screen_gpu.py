"""GPU: the density screen of the plain chain render ("The screen"): fp16 densities of every sample first, the
compaction of the candidates (screen density not <= -margin), the exact kernels on that list alone -- nerf_x3s_kernel<IN_LIST>
for the coarse pass, nerf_mx2_kernel<IN_LIST, true> with its density store for the fine pass.

Every comparison is BIT IDENTITY (torch.equal) unless said otherwise: a listed sample is the same column of the same MFMA
sequence on the same operands as in the dense launch, and a sample the list leaves out has sigma_exact < 0 while
|sigma_screen - sigma_exact| < margin, so relu() of what its plane entry holds is the +0 the dense pass gets.

Figures of the margin test on the MI355X (max |screen - exact| against the calibrated margin, 3 x 2048 rays x 128 depths):
see profiles/density_screen_timing.json, "margin_test"."""
import numpy as np
import pytest
import torch

from tgtc_style_amd import synth

pytestmark = pytest.mark.gpu

LIST_KINDS = ["empty", "one", "127", "128", "129", "all", "third"]
LIST_R = 37
RENDER_R = [1, 130, 4097]
RENDER_COUNTS = [(128, 64), (64, 32)]
SCREENS = {"coarse": (True, False), "fine": (False, True), "both": True}
SENTINEL = -7.25


def T(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


class Args:
    use_viewdir, act_type = True, "relu"
    embed_freq_coor, embed_freq_dir = 10, 4
    netdepth = netdepth_fine = 8
    netwidth = netwidth_fine = 256
    precision = "fp16x3"


def make(shift=(0.0, 0.0), precisions=("fp16x3", "fp16mx")):
    """The synthetic pair, coarse fp16x3 + fine fp16mx; shift: added to the sigma head's bias of (coarse, fine)."""
    from tgtc_style_amd import models
    nets = []
    for (seed, mode), prec, b in zip(((0, "coarse"), (1, "fine")), precisions, shift):
        m = models.StyleNerf(type("A", (Args,), {"precision": prec}), mode=mode)
        sd = T(synth.nerf_state(seed))
        sd["net.sigma_layer.bias"] = sd["net.sigma_layer.bias"] + float(b)
        m.load_state_dict(sd)
        nets.append(m.cuda())
    return nets


@pytest.fixture(scope="module")
def pair():
    nets = make()
    for m in nets:
        m.packed().enable_screen()
    return nets


def sample_inputs(R, n, seed=5):
    rng = np.random.default_rng(seed)
    ro = torch.from_numpy(np.concatenate([rng.uniform(-1, 1, (R, 2)), -np.ones((R, 1))], 1)).cuda()
    rd = torch.from_numpy(np.concatenate([rng.uniform(-.3, .3, (R, 2)), 2 * np.ones((R, 1))], 1)).cuda()
    ts = torch.from_numpy(np.sort(rng.uniform(0, 1, (R, n)).astype(np.float32), -1)).cuda()
    return ro, rd, ts


_frames = {}


def frame_rays(pose, R):
    """R rays spread evenly over the 400 x 400 frame of spiral_pose(pose)."""
    from tgtc_style_amd import utils
    if pose not in _frames:
        _frames[pose] = utils.gen_rays(400, 400, synth.fern_intrinsics(400, 400), synth.spiral_pose(pose))
    o, d = _frames[pose]
    step = 160000 // R
    return o[::step][:R].contiguous(), d[::step][:R].contiguous()


def make_list(kind, M):
    if kind == "empty":
        idx = np.zeros(0, np.int64)
    elif kind == "one":
        idx = np.array([M // 2])
    elif kind in ("127", "128", "129"):
        idx = np.sort(np.random.default_rng(int(kind)).choice(M, int(kind), replace=False))
    elif kind == "all":
        idx = np.arange(M)
    else:
        idx = np.sort(np.random.default_rng(3).choice(M, M // 3, replace=False))     # an ascending random third
    return torch.from_numpy(idx.astype(np.int32)).cuda()


_dense = {}


def dense_forward(pair, which, n):
    """(handle, inputs, rgb or None, sigma) of the dense launch over LIST_R rays x n depths: once per net, never written again."""
    if (which, n) not in _dense:
        from tgtc_style_amd import hip
        net = pair[which].packed()
        ro, rd, ts = sample_inputs(LIST_R, n)
        M = LIST_R * n
        rgb = torch.full((M, 3), float("nan"), device="cuda") if which == 1 else None
        sigma = torch.full((M,), float("nan"), device="cuda")
        hip.check(hip.load().tgtc_nerf_forward_rays(net.handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), LIST_R, n, hip.ptr(rgb),
                                                    hip.ptr(sigma), hip.stream()))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(sigma).all())
        _dense[(which, n)] = (net, (ro, rd, ts), rgb, sigma)
    return _dense[(which, n)]


# ------------------------------------------------------------------------------------------------ 1: the list kernels
@pytest.mark.parametrize("kind", LIST_KINDS)
def test_sigma_list_kernel_bits_of_the_rays_kernel(pair, kind):
    from tgtc_style_amd import hip
    lib = hip.load()
    n = 128
    net, (ro, rd, ts), _, sigma_dense = dense_forward(pair, 0, n)
    M = LIST_R * n
    live = make_list(kind, M)
    count = live.numel()
    buf = live if count else torch.zeros(1, dtype=torch.int32, device="cuda")
    n_live = torch.tensor([count], dtype=torch.int32, device="cuda")
    out = torch.full((M + 64,), SENTINEL, device="cuda")
    hip.check(lib.tgtc_nerf_sigma_list(net.handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), LIST_R, n, hip.ptr(buf), hip.ptr(n_live),
                                       hip.ptr(out), hip.stream()))
    torch.cuda.synchronize()
    listed = torch.zeros(M + 64, dtype=torch.bool, device="cuda")
    listed[live.long()] = True
    assert int(listed.sum()) == count
    assert torch.equal(out[:M][listed[:M]], sigma_dense[listed[:M]])
    assert bool((out[~listed] == SENTINEL).all())            # unlisted entries and the 64 behind the plane; "empty": everything


@pytest.mark.parametrize("kind", LIST_KINDS)
def test_full_list_kernel_with_sigma_bits_of_the_dense_kernel(pair, kind):
    from tgtc_style_amd import hip
    lib = hip.load()
    n = 192
    net, (ro, rd, ts), rgb_dense, sigma_dense = dense_forward(pair, 1, n)
    M = LIST_R * n
    live = make_list(kind, M)
    count = live.numel()
    buf = live if count else torch.zeros(1, dtype=torch.int32, device="cuda")
    n_live = torch.tensor([count], dtype=torch.int32, device="cuda")
    rgb = torch.full((M + 64, 3), SENTINEL, device="cuda")
    sigma = torch.full((M + 64,), SENTINEL, device="cuda")
    hip.check(lib.tgtc_nerf_forward_list_sigma(net.handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), LIST_R, n, hip.ptr(buf),
                                               hip.ptr(n_live), hip.ptr(rgb), hip.ptr(sigma), hip.stream()))
    torch.cuda.synchronize()
    listed = torch.zeros(M + 64, dtype=torch.bool, device="cuda")
    listed[live.long()] = True
    assert torch.equal(rgb[:M][listed[:M]], rgb_dense[listed[:M]]) and torch.equal(sigma[:M][listed[:M]], sigma_dense[listed[:M]])
    assert bool((rgb[~listed] == SENTINEL).all()) and bool((sigma[~listed] == SENTINEL).all())


def test_list_entries_argument_rules(pair):
    from tgtc_style_amd import hip
    lib = hip.load()
    coarse, fine = (m.packed() for m in pair)
    ro, rd, ts = sample_inputs(7, 16)
    live = make_list("one", 7 * 16)
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    sig = torch.zeros(7 * 16, device="cuda")
    rgb = torch.zeros(7 * 16, 3, device="cuda")
    args = (hip.ptr(ro), hip.ptr(rd), hip.ptr(ts))
    assert lib.tgtc_nerf_sigma_list(coarse.handle, *args, 7, 16, hip.ptr(live), hip.ptr(one), hip.ptr(sig), hip.stream()) == 0
    assert lib.tgtc_nerf_sigma_list(coarse.handle, *args, 0, 16, None, None, None, hip.stream()) == 0
    assert lib.tgtc_nerf_sigma_list(coarse.handle, *args, 7, 16, hip.ptr(live), None, hip.ptr(sig), hip.stream()) == -1
    assert lib.tgtc_nerf_sigma_list(fine.handle, *args, 7, 16, hip.ptr(live), hip.ptr(one), hip.ptr(sig), hip.stream()) == -2
    assert lib.tgtc_nerf_sigma_list(coarse.handle, *args, 1 << 40, 16, hip.ptr(live), hip.ptr(one), hip.ptr(sig), hip.stream()) == -2
    assert lib.tgtc_nerf_forward_list_sigma(fine.handle, *args, 7, 16, hip.ptr(live), hip.ptr(one), hip.ptr(rgb), None, hip.stream()) == -1
    assert lib.tgtc_nerf_forward_list_sigma(coarse.handle, *args, 7, 16, hip.ptr(live), hip.ptr(one), hip.ptr(rgb), hip.ptr(sig),
                                            hip.stream()) == -2
    assert lib.tgtc_nerf_screen_rays(coarse.handle, *args, 7, 16, hip.ptr(sig), hip.stream()) == 0
    assert lib.tgtc_nerf_screen_rays(coarse.handle, *args, 7, 16, None, hip.stream()) == -1
    assert lib.tgtc_nerf_screen_rays(make()[0].packed().handle, *args, 7, 16, hip.ptr(sig), hip.stream()) == -2     # no screen
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2: renders
def render(nets, ro, rd, nc, nf, screen, want_coarse=False, cull=None, **kw):
    """(outputs, screened coarse passes, screened fine passes) of one chain render"""
    from tgtc_style_amd import rendering
    hc, hf = (m.packed() for m in nets)
    before = (hc.screened_renders(), hf.screened_renders())
    r = rendering.RayRenderer(nets[0], nets[1], fused=False, screen=screen, cull=cull)
    out = r.render(ro, rd, nc, nf, want_coarse=want_coarse, **kw)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}, hc.screened_renders() - before[0], hf.screened_renders() - before[1]


def same(a, b):
    """the same bits where finite, NaN in the same places"""
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(torch.isnan(a[k]), torch.isnan(b[k])), k
        assert torch.equal(torch.nan_to_num(a[k], nan=0.0), torch.nan_to_num(b[k], nan=0.0)), (k, float((a[k] - b[k]).abs().nan_to_num().max()))


_off = {}


def render_off(pair, R, nc, nf):
    if (R, nc, nf) not in _off:
        ro, rd = frame_rays(3, R)
        out, sc, sf = render(pair, ro, rd, nc, nf, False)
        assert (sc, sf) == (0, 0) and all(bool(torch.isfinite(v).all()) for v in out.values())
        _off[(R, nc, nf)] = (ro, rd, out)
    return _off[(R, nc, nf)]


def fits(R, nc, nf):
    """(coarse, fine): do the list and the 8 KiB of scratch fit the fine colour plane / the dead coarse planes?"""
    up = lambda b: (b + 255) // 256 * 256
    return (R * (nc + nf) * 12 >= R * nc * 4 + 8192,
            2 * up(R * nc * 4) + up(R * nc * 12) + up(R * nc * 4) >= R * (nc + nf) * 4 + 8192)


@pytest.mark.parametrize("which", list(SCREENS))
@pytest.mark.parametrize("nc,nf", RENDER_COUNTS)
@pytest.mark.parametrize("R", RENDER_R)
def test_screened_render_bits_of_the_dense_render(pair, R, nc, nf, which):
    ro, rd, off = render_off(pair, R, nc, nf)
    on, sc, sf = render(pair, ro, rd, nc, nf, SCREENS[which])
    fc, ff = fits(R, nc, nf)
    assert sc == int(which != "fine" and fc) and sf == int(which != "coarse" and ff), (sc, sf)
    assert torch.equal(on["rgb"], off["rgb"]) and torch.equal(on["t"], off["t"])
    assert bool(off["rgb"].any())
    if R == 1:
        assert (sc, sf) == (0, 0)               # neither list fits: both passes dense


def test_screened_render_with_the_coarse_image(pair):
    R, nc, nf = 130, 128, 64
    ro, rd = frame_rays(3, R)
    off, _, _ = render(pair, ro, rd, nc, nf, False, want_coarse=True)
    on, sc, sf = render(pair, ro, rd, nc, nf, True, want_coarse=True)
    assert (sc, sf) == (0, 1)                   # the coarse colours are asked: that pass is dense
    assert sorted(on) == ["rgb", "rgb_coarse", "t", "t_coarse"]
    for k in off:
        assert torch.equal(on[k], off[k]), k


# ------------------------------------------------------------------------------------------------ 3: edges
@pytest.mark.parametrize("shift,share", [(-1000.0, 0.0), (1000.0, 1.0)])
def test_nothing_and_everything_listed(shift, share):
    R, nc, nf = 130, 128, 64
    nets = make(shift=(shift, shift))
    ro, rd = frame_rays(3, R)
    off, _, _ = render(nets, ro, rd, nc, nf, False)
    on, sc, sf = render(nets, ro, rd, nc, nf, True)
    assert (sc, sf) == (1, 1)
    assert nets[0].packed().screen_margin() > 0 and nets[1].packed().screen_margin() > 0
    assert nets[0].packed().screen_fraction() == share and nets[1].packed().screen_fraction() == share
    assert nets[1].packed().live_fraction() == share
    same(on, off)
    assert bool(torch.isfinite(on["rgb"]).all())


def test_densities_inside_the_margin(pair):
    """Both sigma heads shifted so that the median density is about -margin / 2 on rays whose samples crowd into a short
    stretch of depth: at least a fifth of the densities then lie in (-margin, 0], where the screen cannot decide.  The
    stretch is the longest of a fixed list at which that holds."""
    from tgtc_style_amd import hip
    lib = hip.load()
    R, nc, nf = 130, 128, 64
    ro, rd = frame_rays(3, 2)
    ro, rd = ro.repeat(R // 2, 1).contiguous(), rd.repeat(R // 2, 1).contiguous()
    margins = [m.packed().screen_margin() for m in pair]
    for width in (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 0.0):
        ts = torch.linspace(0.5, 0.5 + width, nc, device="cuda").repeat(R, 1).contiguous()
        shifts, inside = [], []
        for net, m in zip(pair, margins):
            sigma = torch.empty(R * nc, device="cuda")
            hip.check(lib.tgtc_nerf_forward_rays(net.packed().handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, nc, None,
                                                 hip.ptr(sigma), hip.stream()))
            torch.cuda.synchronize()
            shifts.append(-0.5 * m - float(sigma.median()))
            s = sigma + shifts[-1]
            inside.append(float(((s > -m) & (s <= 0)).float().mean()))
        if min(inside) >= 0.2:
            break
    print("depth stretch", width, "shifts", shifts, "share inside (-margin, 0]", inside)
    assert min(inside) >= 0.2
    nets = make(shift=shifts)
    off, _, _ = render(nets, ro, rd, nc, nf, False, near=0.5, far=0.5 + width)
    on, sc, sf = render(nets, ro, rd, nc, nf, True, near=0.5, far=0.5 + width)
    assert (sc, sf) == (1, 1)
    print("candidate shares", nets[0].packed().screen_fraction(), nets[1].packed().screen_fraction(), "live", nets[1].packed().live_fraction())
    assert nets[0].packed().screen_fraction() >= 0.2
    same(on, off)


def test_a_ray_with_a_nan_origin(pair):
    R, nc, nf = 130, 128, 64
    ro, rd = frame_rays(3, R)
    ro = ro.clone()
    ro[7, 1] = float("nan")
    off, _, _ = render(pair, ro, rd, nc, nf, False)
    on, sc, sf = render(pair, ro, rd, nc, nf, True)
    assert (sc, sf) == (1, 1)
    same(on, off)
    ok = torch.ones(R, dtype=torch.bool, device="cuda")
    ok[7] = False
    assert bool(torch.isfinite(on["rgb"][ok]).all()) and bool(torch.isfinite(on["t"][ok]).all())


# ------------------------------------------------------------------------------------------------ 4: the margin
def test_margin_holds_on_real_frames(pair):
    from tgtc_style_amd import hip
    lib = hip.load()
    R, n = 2048, 128
    ts = torch.linspace(0, 1, n, device="cuda").repeat(R, 1).contiguous()
    for which, net in enumerate(pair):
        h = net.packed()
        m = h.screen_margin()
        worst = 0.0
        for pose in (0, 60, 119):
            ro, rd = frame_rays(pose, R)
            exact, screen = torch.empty(R * n, device="cuda"), torch.empty(R * n, device="cuda")
            hip.check(lib.tgtc_nerf_forward_rays(h.handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, n, None, hip.ptr(exact), hip.stream()))
            hip.check(lib.tgtc_nerf_screen_rays(h.handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, n, hip.ptr(screen), hip.stream()))
            torch.cuda.synchronize()
            err = float((screen - exact).abs().max())
            worst = max(worst, err)
            print("net %d pose %3d: max |screen - exact| = %.4f, margin %.4f, margin / error = %.2f, candidates %.4f, live %.4f" % (
                which, pose, err, m, m / err, float((~(screen <= -m)).float().mean()), float((exact > 0).float().mean())))
            assert int(((exact > 0) & (screen <= -m)).sum()) == 0
        assert worst <= 0.5 * m, (worst, m)


# ------------------------------------------------------------------------------------------------ 5: policy
def test_auto_follows_the_landed_candidate_shares():
    from tgtc_style_amd import hip, rendering
    lib = hip.load()
    R, nc, nf = 300, 128, 64
    ro, rd = frame_rays(0, R)
    nets = make()
    hc, hf = (m.packed() for m in nets)
    r = rendering.RayRenderer(nets[0], nets[1], fused=False)                # screen=None: AUTO, the default
    first = {k: v.clone() for k, v in r.render(ro, rd, nc, nf).items()}
    torch.cuda.synchronize()
    assert hc.screen_margin() > 0 and hf.screen_margin() > 0                # enabled by the render
    assert (hc.screened_renders(), hf.screened_renders()) == (0, 0)         # shares unknown: dense
    cs, fs, live = hc.screen_fraction(), hf.screen_fraction(), hf.live_fraction()
    print("candidate shares: coarse %.4f fine %.4f; live share fine %.4f" % (cs, fs, live))
    assert 0.15 < cs < 0.45 and 0.05 < fs < 0.2 and 0 < live < fs           # the statistics are sane
    want = (lib.tgtc_screen_auto_decision(0, round(cs * R * nc), R * nc), lib.tgtc_screen_auto_decision(1, round(fs * R * (nc + nf)), R * (nc + nf)))
    second = r.render(ro, rd, nc, nf)
    torch.cuda.synchronize()
    assert (hc.screened_renders(), hf.screened_renders()) == want
    assert want == AUTO_SCREENS_THE_SYNTHETIC_PAIR
    assert hf.live_fraction() == live                                       # kept current by a screened render as well
    assert abs(hc.screen_fraction() - cs) < 0.01 and abs(hf.screen_fraction() - fs) < 0.01     # screen count vs exact count
    assert torch.equal(second["rgb"], first["rgb"]) and torch.equal(second["t"], first["t"])

    # cull=False keeps the fine screen off, whatever `screen` says
    before = hf.screened_renders()
    out, _, sf = render(nets, ro, rd, nc, nf, True, cull=False)
    assert sf == 0 and hf.screened_renders() == before and torch.equal(out["rgb"], first["rgb"])

    # every sample a candidate: AUTO stays dense
    nets = make(shift=(1000.0, 1000.0))
    hc, hf = (m.packed() for m in nets)
    r = rendering.RayRenderer(nets[0], nets[1], fused=False)
    for _ in range(3):
        r.render(ro, rd, nc, nf)
        torch.cuda.synchronize()
    assert hc.screen_fraction() == 1.0 and hf.screen_fraction() == 1.0
    assert (hc.screened_renders(), hf.screened_renders()) == (0, 0)

    assert lib.tgtc_net_set_screen(hf.handle, 3) == -1 and lib.tgtc_net_set_screen(None, hip.SCREEN_ON) == -1
    for mode in (hip.SCREEN_ON, hip.SCREEN_OFF, hip.SCREEN_AUTO):
        assert lib.tgtc_net_set_screen(hf.handle, mode) == 0


# what AUTO decides for (coarse, fine) on the synthetic pair's shares: the thresholds of csrc/render.hip (0.55, 0.42) against
# about 0.25 and 0.08 on these 300 rays
AUTO_SCREENS_THE_SYNTHETIC_PAIR = (1, 1)


# ------------------------------------------------------------------------------------------------ 6: enable
def test_enable_is_idempotent_and_refused_where_it_has_no_meaning():
    from tgtc_style_amd import hip
    lib = hip.load()
    nets = make()
    for m in nets:
        h = m.packed()
        assert h.screen_margin() == -1.0 and h.screen_fraction() == -1.0 and h.screened_renders() == 0
        h.enable_screen()
        margin = h.screen_margin()
        assert 0.5 < margin < 16.0
        h.enable_screen()
        assert h.screen_margin() == margin
    again = make()[0].packed()                                             # the margin is a function of the weights alone
    again.enable_screen()
    assert again.screen_margin() == nets[0].packed().screen_margin()
    fp16 = make(precisions=("fp16", "fp16"))[0].packed()
    assert lib.tgtc_net_enable_screen(fp16.handle, hip.stream()) == -2 and fp16.screen_margin() == -1.0
    assert lib.tgtc_net_set_screen(fp16.handle, hip.SCREEN_ON) == -2 and fp16.screened_renders() == -1
    style = hip.style_create(T(synth.concat_state()), T(synth.style_state()))
    assert lib.tgtc_net_enable_screen(style.handle, hip.stream()) == -2
    assert lib.tgtc_net_enable_screen(None, hip.stream()) == -1


def test_a_handle_without_a_screen_renders_as_before(pair):
    R, nc, nf = 130, 128, 64
    ro, rd, off = render_off(pair, R, nc, nf)
    nets = make()
    out, sc, sf = render(nets, ro, rd, nc, nf, False)
    assert (sc, sf) == (0, 0) and nets[0].packed().screen_margin() == -1.0 and nets[1].packed().screen_margin() == -1.0
    assert torch.equal(out["rgb"], off["rgb"]) and torch.equal(out["t"], off["t"])


def test_case_lists_reach_the_shapes_named():
    assert LIST_KINDS == ["empty", "one", "127", "128", "129", "all", "third"] and LIST_R == 37
    for kind, count in (("empty", 0), ("one", 1), ("127", 127), ("128", 128), ("129", 129), ("all", 37 * 128), ("third", 37 * 128 // 3)):
        live = make_list(kind, 37 * 128).cpu().numpy()
        assert len(live) == count and (np.diff(live) > 0).all() and (len(live) == 0 or (0 <= live[0] and live[-1] < 37 * 128))
    assert RENDER_R == [1, 130, 4097] and RENDER_COUNTS == [(128, 64), (64, 32)] and sorted(SCREENS) == ["both", "coarse", "fine"]
    assert [fits(R, 128, 64) for R in RENDER_R] == [(False, False), (True, True), (True, True)]
    assert [fits(R, 64, 32) for R in RENDER_R] == [(False, False), (True, True), (True, True)]
