"""GPU: the density screen's own kernel (csrc/mlp_nerf_fp16s.hip: four column tiles per wave, one wave per SIMD, persistent, one
generated instruction stream per pass of 256 samples; DESIGN 3.1 "The screen") against the launch it replaces, the sigma-only
CfgFast kernel of an fp16 handle, which the library still runs with TGTC_SCREEN_CFGFAST=1 in the environment (read at every
call).  Both accumulate every density in dense_layer's k order on one chain, so every comparison is BIT IDENTITY.

The grid of a launch over rays is min(passes, CUs) workgroups: every shape below 256 x CUs samples is a launch of fewer
workgroups than the device has CUs, 1 x 1 being one workgroup of which one lane stores; a workgroup never exists without a pass."""
import os

import numpy as np
import pytest
import torch

from tgtc_style_amd import synth

pytestmark = pytest.mark.gpu

SWITCH = "TGTC_SCREEN_CFGFAST"
# rays x depths: around the 64-sample wave tile and the 256-sample pass, many passes with a ragged tail
SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (2, 128), (3, 85), (1, 257), (5, 192), (1025, 3)]
SENTINEL = -7.25


def T(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


class Args:
    use_viewdir, act_type = True, "relu"
    embed_freq_coor, embed_freq_dir = 10, 4
    netdepth = netdepth_fine = 8
    netwidth = netwidth_fine = 256
    precision = "fp16x3"


def make():
    """The synthetic pair, coarse fp16x3 + fine fp16mx."""
    from tgtc_style_amd import models
    nets = []
    for (seed, mode), prec in zip(((0, "coarse"), (1, "fine")), ("fp16x3", "fp16mx")):
        m = models.StyleNerf(type("A", (Args,), {"precision": prec}), mode=mode)
        m.load_state_dict(T(synth.nerf_state(seed)))
        nets.append(m.cuda())
    return nets


@pytest.fixture(scope="module")
def pair():
    assert SWITCH not in os.environ
    nets = make()
    for m in nets:
        m.packed().enable_screen()
    return nets


def inputs(R, n, seed=11):
    rng = np.random.default_rng(seed)
    ro = torch.from_numpy(np.concatenate([rng.uniform(-1, 1, (R, 2)), -np.ones((R, 1))], 1)).cuda()
    rd = torch.from_numpy(np.concatenate([rng.uniform(-.3, .3, (R, 2)), 2 * np.ones((R, 1))], 1)).cuda()
    ts = torch.from_numpy(np.sort(rng.uniform(0, 1, (R, n)).astype(np.float32), -1)).cuda()
    return ro, rd, ts


def screen(net, ro, rd, ts, monkeypatch, cfgfast):
    """densities of the screen launch over [R, n] samples into a plane with 64 sentinels behind it"""
    from tgtc_style_amd import hip
    R, n = ts.shape
    if cfgfast:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    out = torch.full((R * n + 64,), SENTINEL, device="cuda")
    hip.check(hip.load().tgtc_nerf_screen_rays(net.packed().handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, n, hip.ptr(out), hip.stream()))
    torch.cuda.synchronize()
    monkeypatch.delenv(SWITCH, raising=False)
    assert bool((out[R * n:] == SENTINEL).all())
    return out[:R * n]


@pytest.mark.parametrize("R,n", SHAPES)
def test_stream_densities_are_the_bits_of_the_cfgfast_launch(pair, R, n, monkeypatch):
    ro, rd, ts = inputs(R, n)
    for net in pair:
        new = screen(net, ro, rd, ts, monkeypatch, False)
        old = screen(net, ro, rd, ts, monkeypatch, True)
        assert bool(torch.isfinite(old).all()) and bool((old != SENTINEL).all())
        assert np.array_equal(new.cpu().numpy(), old.cpu().numpy())


def test_no_rays_is_no_launch(pair):
    from tgtc_style_amd import hip
    for net in pair:
        assert hip.load().tgtc_nerf_screen_rays(net.packed().handle, None, None, None, 0, 16, None, hip.stream()) == 0
    torch.cuda.synchronize()


def test_non_finite_inputs_reach_their_own_samples_only(pair, monkeypatch):
    """NaN and +-inf in an origin, a direction and a depth: sigma is non-finite at exactly the samples they belong to, and the
    other samples keep the bits of the clean launch.  (The kernel tests the positions it loads: the fp16 ReLU, v_pk_max_f16 with
    zero, returns zero for a NaN, and the CfgFast launch gives all 257 injected samples of either net a finite density.)"""
    R, n = 7, 85                                     # 595 samples: three passes, tiles that mix rays
    ro, rd, ts = inputs(R, n)
    ro_b, rd_b, ts_b = ro.clone(), rd.clone(), ts.clone()
    ro_b[1, 0] = float("nan")
    rd_b[3, 1] = float("inf")
    rd_b[4, 2] = float("-inf")
    ts_b[5, 17] = float("nan")
    ts_b[6, 84] = float("inf")
    bad = torch.zeros(R, n, dtype=torch.bool, device="cuda")
    bad[1] = bad[3] = bad[4] = True
    bad[5, 17] = bad[6, 84] = True
    bad = bad.flatten()
    for net in pair:
        clean = screen(net, ro, rd, ts, monkeypatch, False)
        new = screen(net, ro_b, rd_b, ts_b, monkeypatch, False)
        old = screen(net, ro_b, rd_b, ts_b, monkeypatch, True)
        print("non-finite densities: stream %d, CfgFast %d, injected samples %d" % (
            int((~torch.isfinite(new)).sum()), int((~torch.isfinite(old)).sum()), int(bad.sum())))
        assert torch.equal(torch.isfinite(new), ~bad)
        assert torch.equal(new[~bad], clean[~bad])
        assert torch.equal(new[~bad], old[~bad])          # (the CfgFast launch's ReLU turns a NaN into zero: its densities there are finite)


@pytest.mark.parametrize("R", [64, 257])
def test_screened_render_bits_of_the_dense_render(pair, R):
    from tgtc_style_amd import rendering, utils
    o, d = utils.gen_rays(400, 400, synth.fern_intrinsics(400, 400), synth.spiral_pose(3))
    step = 160000 // R
    ro, rd = o[::step][:R].contiguous(), d[::step][:R].contiguous()
    hc, hf = (m.packed() for m in pair)
    outs = {}
    for name, on in (("off", False), ("on", True)):
        before = (hc.screened_renders(), hf.screened_renders())
        out = rendering.RayRenderer(pair[0], pair[1], fused=False, screen=on).render(ro, rd, 128, 64)
        torch.cuda.synchronize()
        outs[name] = {k: v.clone() for k, v in out.items()}
        assert (hc.screened_renders() - before[0], hf.screened_renders() - before[1]) == ((1, 1) if on else (0, 0))
    for k in ("rgb", "t"):
        assert np.array_equal(outs["on"][k].cpu().numpy(), outs["off"][k].cpu().numpy()), k
    assert bool(outs["off"]["rgb"].any()) and bool(torch.isfinite(outs["off"]["rgb"]).all())


def test_margin_is_the_cfgfast_calibration(pair, monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    old = make()
    for m in old:
        m.packed().enable_screen()
    torch.cuda.synchronize()
    monkeypatch.delenv(SWITCH)
    for a, b in zip(pair, old):
        assert a.packed().screen_margin() == b.packed().screen_margin() > 0
