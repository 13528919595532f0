"""GPU: the density screen's stream with the front end under it (csrc/mlp_nerf_fp16s.hip, tools/gen_fp16s_asm.py front=1; DESIGN
3.1 "The front end under the stream"): while a workgroup's waves run the MFMAs of pass p they load and encode the samples of
pass p + gridDim.x, in the same IEEE operations as the HIP front end.  The library still runs the serial-front stream with
TGTC_SCREEN_SERIAL_FRONT=1 and the CfgFast launch with TGTC_SCREEN_CFGFAST=1 (both read at every call): every comparison is
BIT IDENTITY, NaN against NaN.

A pass is 256 samples and the grid is min(passes, CUs) workgroups: the first pass of a workgroup is encoded by the HIP front
end, every later one by the stream of the pass before it."""
import math
import os

import numpy as np
import pytest
import torch

import test_screen_stream_gpu as S

pytestmark = pytest.mark.gpu

SERIAL = "TGTC_SCREEN_SERIAL_FRONT"
CFGFAST = S.SWITCH
PASS = 256


@pytest.fixture(scope="module")
def pair():
    assert SERIAL not in os.environ and CFGFAST not in os.environ
    nets = S.make()
    for m in nets:
        m.packed().enable_screen()
    return nets


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def screen(net, ro, rd, ts, monkeypatch, switch=None):
    """densities of the screen launch over [R, n] samples into a plane with 64 canaries behind it, which must be intact"""
    from tgtc_style_amd import hip
    R, n = ts.shape
    for k in (SERIAL, CFGFAST):
        monkeypatch.delenv(k, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    out = torch.full((R * n + 64,), S.SENTINEL, device="cuda")
    hip.check(hip.load().tgtc_nerf_screen_rays(net.packed().handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, n, hip.ptr(out), hip.stream()))
    torch.cuda.synchronize()
    if switch:
        monkeypatch.delenv(switch)
    assert bool((out[R * n:] == S.SENTINEL).all())
    return out[:R * n].cpu().numpy()


def same_three_ways(pair, R, n, monkeypatch):
    ro, rd, ts = S.inputs(R, n)
    for net in pair:
        new = screen(net, ro, rd, ts, monkeypatch)
        serial = screen(net, ro, rd, ts, monkeypatch, SERIAL)
        old = screen(net, ro, rd, ts, monkeypatch, CFGFAST)
        assert np.isfinite(old).all() and (old != S.SENTINEL).all()
        assert np.array_equal(new, serial)
        assert np.array_equal(new, old)


@pytest.mark.parametrize("passes", ["cus", "cus+1", "2cus", "2cus+1"])
def test_pass_counts_around_the_first_prefetch(pair, passes, monkeypatch):
    """CUs passes: no stream's encodings are ever used; CUs + 1: one workgroup's are; 2 CUs: every workgroup's, once; 2 CUs + 1:
    one workgroup takes a third pass from its second's stream"""
    n_pass = {"cus": cus(), "cus+1": cus() + 1, "2cus": 2 * cus(), "2cus+1": 2 * cus() + 1}[passes]
    same_three_ways(pair, n_pass * PASS // 128, 128, monkeypatch)


def test_revisits_with_a_ragged_tail(pair, monkeypatch):
    """the recipe of nerf_kernel_cases.revisit_rays for passes of 256 samples: 2.2 passes per CU and a last pass cut short"""
    n = 100
    R = math.ceil(2.2 * cus() * PASS / n) + 7
    while (R * n) % 16 == 0:
        R += 1
    same_three_ways(pair, R, n, monkeypatch)


@pytest.mark.parametrize("n", [37, 100, 128, 129, 192])
def test_depth_counts(pair, n, monkeypatch):
    """tiles that straddle rays (the stream divides every sample index by N on its own); but for 128 and 192 the sample count
    is no multiple of 16, 64 or 256"""
    R = math.ceil(2.2 * cus() * PASS / n)
    if n % 2 and R % 2 == 0:
        R += 1                                  # odd x odd: M is odd
    same_three_ways(pair, R, n, monkeypatch)


@pytest.mark.parametrize("nan_tile,inf_tile", [(0, 3), (3, 0)])
def test_non_finite_positions_of_a_prefetched_pass(pair, nan_tile, inf_tile, monkeypatch):
    """Rays of 16 samples are tiles: ray r is tile r % 4 of wave (r % 16) / 4 of pass r / 16.  A NaN origin and an infinite
    direction in passes that the stream of an earlier pass encodes: NaN on exactly their samples, in the in-stream and in the
    serial-front launch, and the bits of the clean launch everywhere else."""
    n = 16
    R = math.ceil(2.2 * cus() * PASS / n) + 3
    r_nan = 16 * (cus() + 1) + 4 * 1 + nan_tile          # second pass of workgroup 1, wave 1
    r_inf = 16 * (2 * cus() + 2) + 4 * 2 + inf_tile      # third pass of workgroup 2, wave 2
    assert r_inf < R
    ro, rd, ts = S.inputs(R, n)
    ro_b, rd_b = ro.clone(), rd.clone()
    ro_b[r_nan, 1] = float("nan")
    rd_b[r_inf, 2] = float("inf")
    bad = np.zeros((R, n), bool)
    bad[r_nan] = bad[r_inf] = True
    bad = bad.reshape(-1)
    for net in pair:
        clean = screen(net, ro, rd, ts, monkeypatch)
        new = screen(net, ro_b, rd_b, ts, monkeypatch)
        serial = screen(net, ro_b, rd_b, ts, monkeypatch, SERIAL)
        old = screen(net, ro_b, rd_b, ts, monkeypatch, CFGFAST)
        assert np.isfinite(clean).all()
        assert np.array_equal(np.isnan(new), bad)
        assert np.array_equal(new, serial, equal_nan=True)
        assert np.array_equal(new[~bad], clean[~bad])
        assert np.array_equal(new[~bad], old[~bad])


def test_screened_render_three_ways(pair, monkeypatch):
    """64 x 64 rays at 128 + 64: 2048 passes of the coarse screen and 3072 of the fine one, screens on, with the serial-front
    stream, and off"""
    from tgtc_style_amd import rendering, utils
    from tgtc_style_amd import synth
    o, d = utils.gen_rays(64, 64, synth.fern_intrinsics(64, 64), synth.spiral_pose(3))
    ro, rd = o.contiguous(), d.contiguous()
    outs = {}
    for name, on, switch in (("on", True, None), ("serial", True, SERIAL), ("off", False, None)):
        monkeypatch.delenv(SERIAL, raising=False)
        if switch:
            monkeypatch.setenv(switch, "1")
        out = rendering.RayRenderer(pair[0], pair[1], fused=False, screen=on).render(ro, rd, 128, 64)
        torch.cuda.synchronize()
        outs[name] = {k: out[k].cpu().numpy().copy() for k in ("rgb", "t")}
    monkeypatch.delenv(SERIAL, raising=False)
    for k in ("rgb", "t"):
        assert np.array_equal(outs["on"][k], outs["serial"][k]), k
        assert np.array_equal(outs["on"][k], outs["off"][k]), k
    assert outs["off"]["rgb"].any() and np.isfinite(outs["off"]["rgb"]).all()
