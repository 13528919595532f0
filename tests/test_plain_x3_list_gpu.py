"""GPU: the two-phase fine pass for a fine handle in fp16x3 -- the full fp16x3 network over a device-side list
(tgtc_nerf_forward_list_x3, csrc/mlp_nerf_x3_list.hip), its wiring through fine_pass under TGTC_CULL_ON, RayRenderer and the
command line.

A listed sample is the same MFMA column on the same operands in the same order as in nerf_mlp_kernel<CfgExact, IN_RAYS, true>, so
1, 2, 3, 6, 7 and 8 ask for BIT IDENTITY (torch.equal / equal bytes).

1. The list kernel against the dense kernel: grids nerf_kernel_cases.LIST_SHAPES x weights base / rows / dead x list lengths at
   every boundary of a 16-sample tile and a 128-slot pass and the whole grid; unlisted entries keep a sentinel.
2. A device count of 0, a listed index >= M, sigma = NULL.
3. The persistent walk: second and third passes of every workgroup; a third call reproduces the first after another's inputs.
4. Per sample against float64 (nerf_kernel_cases.ray_case_oracle), bar TIGHT["fp16x3"] = 5e-5 max-norm relative per tensor.
5. Argument rules.
6. Render, cull=True against cull=False, screened and not; an empty and a full list.
7. AUTO (cull=None) leaves an fp16x3 fine pass dense whatever has landed and whatever screen the handle carries.
8. --two_phase writes the dense chain's bytes.

The live and candidate shares of 6: the fine net is synth.nerf_state(1) on rays of the benchmark's first frame, whose density is
positive on about a tenth of the fine samples (tests/test_plain_cull_gpu.py render_inputs; the float64 oracle's share, which does
not depend on the handle's precision); the test asserts both shares strictly inside (0, 1) itself."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nerf_kernel_cases as nk
from tgtc_style_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SENTINEL = -7.25
SPARE = 64
WEIGHTS = ["base", "rows", "dead"]
LENGTHS = [1, 15, 16, 17, 127, 128, 129, 257, None]          # None: every sample
ORACLE_GRID = {"base": (5, 37), "rows": (3, 200), "dead": (40, 129)}


def T(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


class Args:
    use_viewdir, act_type = True, "relu"
    embed_freq_coor, embed_freq_dir = 10, 4
    netdepth = netdepth_fine = 8
    netwidth = netwidth_fine = 256
    precision = "fp16x3"


def test_case_lists_reach_the_boundaries_named():
    assert nk.LIST_SHAPES == [(5, 37), (3, 200), (40, 129)] and sorted(ORACLE_GRID.values()) == sorted(nk.LIST_SHAPES)
    assert {1, 15, 16, 17, 127, 128, 129, 257, None} == set(LENGTHS)
    assert min(R * N for R, N in nk.LIST_SHAPES) == 185 and max(R * N for R, N in nk.LIST_SHAPES) == 5160


_NETS = {}


def fine_net(wf="base", precision="fp16x3"):
    """The fine NeRF of a weight family of nerf_kernel_cases as a module on the GPU (cached)."""
    if (wf, precision) not in _NETS:
        from tgtc_style_amd import models
        m = models.StyleNerf(type("A", (Args,), {"precision": precision}), mode="fine")
        m.load_state_dict(T(nk.states(wf)))
        _NETS[wf, precision] = m.cuda()
    return _NETS[wf, precision]


def spread(M, n):
    """n ascending sample indices spread over [0, M) (all of them for n None or n >= M), int32 on the device"""
    if n is None or n >= M:
        idx = np.arange(M)
    else:
        idx = np.unique(np.round(np.linspace(0, M - 1, n)).astype(np.int64))
        assert len(idx) == n
    return torch.from_numpy(idx.astype(np.int32)).cuda()


_DENSE = {}


def dense(wf, R, N, seed=None):
    """(inputs on the device, rgb [M,3] of the full dense launch, sigma [M] of the sigma-only launch): once, never written again"""
    key = (wf, R, N, seed)
    if key not in _DENSE:
        from tgtc_style_amd import hip
        lib, net = hip.load(), fine_net(wf).packed()
        ro, rd, ts = (x.cuda() for x in nk.ray_inputs(R, N, seed=seed))
        M = R * N
        rgb = torch.full((M, 3), float("nan"), device="cuda")
        sig_full = torch.full((M,), float("nan"), device="cuda")
        sigma = torch.full((M,), float("nan"), device="cuda")
        hip.check(lib.tgtc_nerf_forward_rays(net.handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, N, hip.ptr(rgb), hip.ptr(sig_full),
                                             hip.stream()))
        hip.check(lib.tgtc_nerf_forward_rays(net.handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, N, None, hip.ptr(sigma),
                                             hip.stream()))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(sigma).all()) and torch.equal(sigma, sig_full)
        _DENSE[key] = ((ro, rd, ts), rgb, sigma)
    return _DENSE[key]


def run_list(wf, inputs, live, count=None, with_sigma=True):
    """tgtc_nerf_forward_list_x3 into sentinel-filled planes with SPARE rows behind them -> (rgb [M + SPARE, 3], sigma [M + SPARE])"""
    from tgtc_style_amd import hip
    ro, rd, ts = inputs
    M = ts.numel()
    rgb = torch.full((M + SPARE, 3), SENTINEL, device="cuda")
    sigma = torch.full((M + SPARE,), SENTINEL, device="cuda")
    n_live = torch.tensor([live.numel() if count is None else count], dtype=torch.int32, device="cuda")
    hip.nerf_forward_list_x3(fine_net(wf).packed(), ro, rd, ts, live, n_live, rgb, sigma if with_sigma else None)
    torch.cuda.synchronize()
    return rgb, sigma


def check_list(wf, R, N, live, rgb, sigma, with_sigma=True, seed=None):
    _, rgb_dense, sigma_dense = dense(wf, R, N, seed)
    M = R * N
    listed = torch.zeros(M + SPARE, dtype=torch.bool, device="cuda")
    listed[live.long()] = True
    assert int(listed.sum()) == live.numel()
    assert torch.equal(rgb[:M][listed[:M]], rgb_dense[listed[:M]])
    assert bool((rgb[~listed] == SENTINEL).all()), "rgb written outside the list"
    if with_sigma:
        assert torch.equal(sigma[:M][listed[:M]], sigma_dense[listed[:M]])
        assert bool((sigma[~listed] == SENTINEL).all()), "sigma written outside the list"
    else:
        assert bool((sigma == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 1: bits of the dense kernel
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("wf", WEIGHTS)
@pytest.mark.parametrize("R,N", nk.LIST_SHAPES)
def test_list_kernel_gives_the_bits_of_the_dense_kernel(R, N, wf, n):
    inputs, _, _ = dense(wf, R, N)
    live = spread(R * N, n)
    rgb, sigma = run_list(wf, inputs, live)
    check_list(wf, R, N, live, rgb, sigma)


# ------------------------------------------------------------------------------------------------ 2: count and index edges
def test_a_device_count_of_zero_writes_nothing():
    R, N = 40, 129
    inputs, _, _ = dense("base", R, N)
    rgb, sigma = run_list("base", inputs, spread(R * N, 257), count=0)
    assert bool((rgb == SENTINEL).all()) and bool((sigma == SENTINEL).all())


def test_a_listed_index_past_the_grid_is_not_written():
    R, N = 5, 37
    M = R * N
    inputs, _, _ = dense("base", R, N)
    live = spread(M, 17)
    bad = torch.cat([live, torch.tensor([M + 3], dtype=torch.int32, device="cuda")])     # ascending; M + 3 is a SPARE row
    rgb, sigma = run_list("base", inputs, bad)
    check_list("base", R, N, live, rgb, sigma)                                          # the others written, M + 3 keeps the sentinel


def test_without_a_sigma_plane_only_rgb_is_written():
    R, N = 3, 200
    inputs, _, _ = dense("base", R, N)
    live = spread(R * N, 129)
    rgb, sigma = run_list("base", inputs, live, with_sigma=False)
    check_list("base", R, N, live, rgb, sigma, with_sigma=False)


# ------------------------------------------------------------------------------------------------ 3: the persistent walk
def test_second_and_third_visit():
    """About 2.2 passes of 128 list slots per CU and a ragged tail: every workgroup takes a second pass, some a third, each on a
    ring it primes again.  The full list gives the dense bits; after a call on other inputs a third call gives the first's."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    R, N = nk.revisit_rays(n_cu), nk.REVISIT_N
    M = R * N
    assert (M + 127) // 128 > 2 * n_cu and M % 128
    live = spread(M, None)
    first_in, _, _ = dense("base", R, N)
    other_in, _, _ = dense("base", R, N, seed=4242)
    first = run_list("base", first_in, live)
    check_list("base", R, N, live, *first)
    second = run_list("base", other_in, live)
    check_list("base", R, N, live, *second, seed=4242)
    assert not torch.equal(second[0], first[0])
    third = run_list("base", first_in, live)
    assert torch.equal(third[0], first[0]) and torch.equal(third[1], first[1])


# ------------------------------------------------------------------------------------------------ 4: float64
@pytest.mark.parametrize("wf", WEIGHTS)
def test_listed_samples_against_float64(wf):
    R, N = ORACLE_GRID[wf]
    M = R * N
    (ref_sigma, ref_rgb, _), _ = nk.ray_case_oracle((R, N, "each", wf))
    inputs, _, _ = dense(wf, R, N)
    for n in (129 if M > 129 else 17, None):
        live = spread(M, n)
        rgb, sigma = run_list(wf, inputs, live)
        idx = live.long().cpu()
        e_rgb, e_sigma = nk.S.rel(rgb[:M].cpu()[idx], ref_rgb[idx]), nk.S.rel(sigma[:M].cpu()[idx], ref_sigma[idx])
        print("fp16x3 list kernel %dx%d %-5s list %-4s: rgb %.3e  sigma %.3e  bar %.1e" % (R, N, wf, n or "all", e_rgb, e_sigma,
                                                                                          nk.TIGHT["fp16x3"]))
        assert e_rgb <= nk.TIGHT["fp16x3"] and e_sigma <= nk.TIGHT["fp16x3"], (wf, n, e_rgb, e_sigma)


# ------------------------------------------------------------------------------------------------ 5: argument rules
def test_argument_rules():
    from tgtc_style_amd import hip
    lib = hip.load()
    R, N = 7, 16
    ro, rd, ts = (x.cuda() for x in nk.ray_inputs(R, N))
    live = spread(R * N, 15)
    n_live = torch.tensor([15], dtype=torch.int32, device="cuda")
    rgb = torch.full((R * N, 3), SENTINEL, device="cuda")
    sigma = torch.full((R * N,), SENTINEL, device="cuda")
    x3 = fine_net("base").packed().handle

    def call(net=x3, R=R, N=N, ro=ro, rd=rd, ts=ts, live=live, n_live=n_live, rgb=rgb, sigma=sigma, entry=lib.tgtc_nerf_forward_list_x3):
        return entry(net, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, N, hip.ptr(live), hip.ptr(n_live), hip.ptr(rgb), hip.ptr(sigma),
                     hip.stream())
    assert call(net=None) == -1 and call(R=-1) == -1 and call(N=0) == -1
    for name in ("ro", "rd", "ts", "live", "n_live", "rgb"):
        assert call(**{name: None}) == -1, name
    assert call(R=1 << 40) == -2 and call(R=1 << 27, N=16) == -2                      # R x N >= 2^31
    for prec in ("fp16mx", "fp16"):
        assert call(net=fine_net("base", prec).packed().handle) == -2, prec
    torch.cuda.synchronize()
    assert bool((rgb == SENTINEL).all()) and bool((sigma == SENTINEL).all()), "a refused call wrote"
    assert call(R=0) == 0
    torch.cuda.synchronize()
    assert bool((rgb == SENTINEL).all())
    # the siblings keep refusing an fp16x3 handle
    assert lib.tgtc_nerf_forward_list(x3, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, N, hip.ptr(live), hip.ptr(n_live), hip.ptr(rgb),
                                      hip.stream()) == -2
    assert call(entry=lib.tgtc_nerf_forward_list_sigma) == -2
    assert call() == 0 and call(sigma=None) == 0
    torch.cuda.synchronize()
    assert int((rgb[:, 0] != SENTINEL).sum()) == 15 and int((sigma != SENTINEL).sum()) == 15
    with pytest.raises(RuntimeError):
        hip.nerf_forward_list_x3(fine_net("base", "fp16mx").packed(), ro, rd, ts, live, n_live, rgb)


def test_a_style_handle_is_refused():
    from tgtc_style_amd import hip
    lib = hip.load()
    style = hip.style_create(T(synth.concat_state(2)), T(synth.style_state(3)), "fp16x3")
    one = torch.zeros(16, dtype=torch.int32, device="cuda")
    buf = torch.zeros(64, device="cuda", dtype=torch.float64)
    f = torch.zeros(64, device="cuda")
    assert lib.tgtc_nerf_forward_list_x3(style.handle, hip.ptr(buf), hip.ptr(buf), hip.ptr(f), 1, 1, hip.ptr(one), hip.ptr(one),
                                         hip.ptr(f), None, hip.stream()) == -1


# ------------------------------------------------------------------------------------------------ 6: render, ON against OFF
R_RENDER = 300
_frame = {}


def render_inputs(R, nc, seed=11):
    """R rays spread evenly over the benchmark's first frame (400 x 400, spiral_pose(0)) and a jitter plane"""
    from tgtc_style_amd import utils
    if not _frame:
        _frame["o"], _frame["d"] = utils.gen_rays(400, 400, synth.fern_intrinsics(400, 400), synth.spiral_pose(0))
    step = 160000 // R
    ro, rd = _frame["o"][::step][:R].contiguous(), _frame["d"][::step][:R].contiguous()
    jit = torch.from_numpy(np.random.default_rng(seed).uniform(0, 1, (R, nc)).astype(np.float32)).cuda()
    return ro, rd, jit


def make_pair(fine_sigma_const=None, fine_precision="fp16x3"):
    """The synthetic pair, coarse fp16x3 + fine; fine_sigma_const: the fine density is that constant ('none' / 'all' of
    tests/test_fine_stash_gpu.py)"""
    from tgtc_style_amd import models
    nets = []
    for (seed, mode), prec in zip(((0, "coarse"), (1, "fine")), ("fp16x3", fine_precision)):
        m = models.StyleNerf(type("A", (Args,), {"precision": prec}), mode=mode)
        sd = T(synth.nerf_state(seed))
        if mode == "fine" and fine_sigma_const is not None:
            sd["net.sigma_layer.weight"] = torch.zeros_like(sd["net.sigma_layer.weight"])
            sd["net.sigma_layer.bias"] = torch.full_like(sd["net.sigma_layer.bias"], fine_sigma_const)
        m.load_state_dict(sd)
        nets.append(m.cuda())
    return nets


@pytest.fixture(scope="module")
def pair():
    return make_pair()


def render(nets, nc, nf, jitter, want_coarse, **kw):
    """-> (outputs, rise of culled_renders, rise of screened_renders on the fine handle)"""
    from tgtc_style_amd import rendering
    ro, rd, jit = render_inputs(R_RENDER, nc)
    fine = nets[1].packed()
    before = fine.culled_renders(), max(fine.screened_renders(), 0)
    out = rendering.RayRenderer(nets[0], nets[1], fused=False, **kw).render(ro, rd, nc, nf, jitter=jit if jitter else None,
                                                                           want_coarse=want_coarse)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}, fine.culled_renders() - before[0], max(fine.screened_renders(), 0) - before[1]


def same(a, b):
    assert sorted(a) == sorted(b)
    for k in b:
        assert bool(torch.isfinite(a[k]).all()) and bool(torch.isfinite(b[k]).all()), k
        assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))


@pytest.mark.parametrize("want_coarse", [False, True])
@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("nc,nf", [(64, 64), (100, 28)])
def test_two_phase_render_is_the_dense_render_bit_for_bit(pair, nc, nf, jitter, want_coarse):
    off, n_off, _ = render(pair, nc, nf, jitter, want_coarse, cull=False, screen=False)
    assert n_off == 0 and sorted(off) == (["rgb", "rgb_coarse", "t", "t_coarse"] if want_coarse else ["rgb", "t"])
    fine = pair[1].packed()
    for s in (False, (None, False), True):
        on, n_on, n_screened = render(pair, nc, nf, jitter, want_coarse, cull=True, screen=s)
        same(on, off)
        assert n_on == 1, s
        live = fine.live_fraction()
        assert 0 < live < 1, live
        if s is True:
            assert n_screened == 1
            share = fine.screen_fraction()
            assert 0 < share < 1 and share >= live, (share, live)
        else:
            assert n_screened == 0


@pytest.mark.parametrize("const,share", [(-3.0, 0.0), (8.0, 1.0)])
def test_an_empty_and_a_full_list(const, share):
    nets = make_pair(fine_sigma_const=const)
    off, n_off, _ = render(nets, 64, 64, True, False, cull=False, screen=False)
    for s in (False, True):          # (a constant density calibrates no margin: screen=True then renders unscreened)
        on, n_on, _ = render(nets, 64, 64, True, False, cull=True, screen=s)
        same(on, off)
        assert (n_off, n_on) == (0, 1) and nets[1].packed().live_fraction() == share


# ------------------------------------------------------------------------------------------------ 7: nothing changes unasked
def test_auto_leaves_an_fp16x3_fine_pass_dense():
    nets = make_pair()
    fine = nets[1].packed()
    nc, nf = 64, 64
    off, _, _ = render(nets, nc, nf, True, False, cull=False, screen=False)
    auto, n, _ = render(nets, nc, nf, True, False, cull=None)
    same(auto, off)
    assert n == 0 and fine.live_fraction() == -1.0                     # dense, and no statistic: the pass it always was
    on, n, n_screened = render(nets, nc, nf, True, False, cull=True, screen=True)
    same(on, off)
    assert (n, n_screened) == (1, 1) and 0 < fine.live_fraction() < 0.14 and fine.screen_margin() > 0
    for _ in range(2):                                               # a low share has landed, the handle carries a screen
        auto, n, n_screened = render(nets, nc, nf, True, False, cull=None, screen=True)
        same(auto, off)
        assert (n, n_screened) == (0, 0)


# ------------------------------------------------------------------------------------------------ 8: the command line
CLI = ["--config", os.path.join(ROOT, "configs", "fern.txt"), "--synthetic", "--synthetic_hw", "40", "--render_valid",
       "--precision", "fp16x3"]
CHILD = ("import sys; sys.path.insert(0, %r); from tgtc_style_amd import rendering, train_tgtcs\n"
         "if sys.argv[1] == 'dense':\n"
         "    R = rendering.RayRenderer\n"
         "    rendering.RayRenderer = lambda *a, **k: R(*a, **dict(k, fused=False, cull=False))\n"
         "print('OUT=' + train_tgtcs.main(sys.argv[2:]))") % ROOT


def cli(form, argv):
    """train_tgtcs.main(argv) in a fresh child process under a time limit ('dense': every renderer forced onto the dense chain);
    the files of the directory it printed"""
    r = subprocess.run([sys.executable, "-c", CHILD, form] + argv, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("OUT=")][-1]
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.endswith(".png")}


def test_cli_two_phase_writes_the_dense_chain_bytes(tmp_path):
    two = cli("asis", CLI + ["--two_phase", "--basedir", str(tmp_path / "two")])
    dense_ = cli("dense", CLI + ["--basedir", str(tmp_path / "dense")])
    assert len(two) >= 2 and any(n.startswith("rgb_") for n in two) and any(n.startswith("depth_") for n in two)
    assert sorted(two) == sorted(dense_)
    for n in two:
        assert len(two[n]) > 100 and two[n] == dense_[n], n
