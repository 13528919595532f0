"""GPU: tgtc_composite_live_colours (composite_wave's LIVE_COLOURS instance, csrc/raypath.hip) -- what the two-phase fine
pass composites with instead of zero-filling its colour plane.  On a plane whose dead entries (sigma not > 0) hold NaN bit
patterns it gives the bits of tgtc_composite on the plane with +0 there: pixel, depth and weights, torch.equal.

R = 5: one workgroup of four rays and a tail.  N = 1; 63, 64, 65 around one sample per lane; 192, the frame's count (three
per lane)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

R = 5
NAN_BITS = np.array([0x7FC00000, 0xFFFFFFFF, 0x7F800001], dtype=np.uint32)   # quiet, all ones, signalling


@pytest.mark.parametrize("N", [1, 63, 64, 65, 192])
def test_nan_at_dead_entries_equals_zero_filled_plane(N):
    from tgtc_style_amd import hip
    lib = hip.load()
    rng = np.random.default_rng(N)
    sigma = (rng.standard_normal((R, N)) * 3.0).astype(np.float32)            # about half dead
    sigma[:, ::7] = 0.0                                                       # sigma = 0 and -0 are dead too
    sigma[:, 3::11] = -0.0
    sigma[0, :] = -1.0                                                        # a ray without a live sample
    if N > 1:
        sigma[1, :] = np.abs(sigma[1, :]) + 0.5                               # a ray without a dead one
    else:
        sigma[1:, 0] = (2.0, -0.0, 0.5, 1.5)
    dead = ~(sigma > 0.0)
    ts = np.sort(rng.uniform(0.0, 1.0, (R, N)).astype(np.float32), axis=1)
    rgb = rng.uniform(0.0, 1.0, (R, N, 3)).astype(np.float32)
    zeroed = rgb.copy()
    zeroed[dead] = 0.0
    poisoned = rgb.copy().view(np.uint32)
    poisoned[dead] = NAN_BITS[rng.integers(0, 3, (int(dead.sum()), 3))]
    poisoned = poisoned.view(np.float32)
    assert np.isnan(poisoned[dead]).all() and not np.isnan(poisoned[~dead]).any()

    sigma_d, ts_d = torch.from_numpy(sigma).cuda(), torch.from_numpy(ts).cuda()
    outs = []
    for fn, plane in ((lib.tgtc_composite, zeroed), (lib.tgtc_composite_live_colours, poisoned)):
        plane_d = torch.from_numpy(plane).cuda()
        rgb_exp = torch.full((R + 1, 3), -7.25, device="cuda")
        t_exp = torch.full((R + 1,), -7.25, device="cuda")
        w = torch.full((R + 1, N), -7.25, device="cuda")
        hip.check(fn(hip.ptr(plane_d), hip.ptr(sigma_d), hip.ptr(ts_d), R, N, hip.ptr(rgb_exp), hip.ptr(t_exp), hip.ptr(w),
                     hip.stream()))
        torch.cuda.synchronize()
        outs.append((rgb_exp, t_exp, w))
    for a, b in zip(*outs):
        assert bool(torch.isfinite(a).all())
        assert torch.equal(a, b)
    assert bool((outs[1][0][0] == 0.0).all())                                 # the ray without a live sample is black
    assert float(outs[1][0][1:R].abs().max()) > 0.0
