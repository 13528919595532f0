"""CPU: the cases of the density screen's domain sweep (tests/screen_cases.py; DESIGN 3.1 "The screen's domain") reach what
they name -- which samples of every ray family lie inside the declared box |x|, |y|, |z| <= B, the samples planted on its
faces and one float64 ulp on either side of them, the zero-crossing sets' conditions on the float64 reference -- and the box
holds every position the benchmark's frames and the tests' fern orbit reach."""
import numpy as np
import pytest
import torch

import nerf_kernel_cases as nk
import screen_cases as C


def test_case_lists_reach_what_they_name():
    assert C.B == 2.0 and (C.R, C.N) == (37, 128) and C.BOX_SHAPE == (592, 8) and C.R * C.N <= 5000 and C.ZERO_R * C.N <= 5000
    assert C.NETS == {"coarse": (0, "fp16x3"), "fine": (1, "fp16mx")}
    assert C.WEIGHT_FAMILIES == nk.WEIGHT_FAMILIES == ["base", "rows", "outliers", "dead"]
    assert C.RAY_FAMILIES == ["cal", "box", "ndc-wide", "mid", "wide", "far-llff", "straddle"]
    assert C.ZERO_SETS == {"zero-box": None, "zero-8": 8.0, "zero-30": 30.0, "zero-100": 100.0} and C.ZERO_R == 32
    assert len(C.CASES) == 2 * 4 * 11 and len(set(C.CASES)) == 88 and len(C.DOMAIN_CASES) == 16
    assert C.IN_DOMAIN == ["cal", "box", "zero-box"] and C.OUT_OF_DOMAIN == ["zero-8", "zero-30", "zero-100"]
    assert C.CHAIN_SHAPES == [(1, 1), (3, 85), (5, 192)] and C.CHAIN_WEIGHTS == ["base", "outliers"]
    for fam in C.IN_DOMAIN + C.OUT_OF_DOMAIN:
        inside = C.in_box(C.positions(*C.rays(fam, "fine", "dead")))
        assert inside.all() if fam in C.IN_DOMAIN else not inside.any()
    assert (C.R * C.N) % 256 and (C.R * C.N) // 256 >= 2          # several passes of the stream and a ragged one
    for fam in C.RAY_FAMILIES:
        ro, rd, ts = C.rays(fam)
        shape = C.BOX_SHAPE if fam == "box" else (C.R, C.N)
        assert ro.shape == rd.shape == (shape[0], 3) and ts.shape == shape and shape[0] * shape[1] == C.R * C.N
        assert ro.dtype == rd.dtype == torch.float64 and ts.dtype == torch.float32
        assert bool(torch.isfinite(ro).all() and torch.isfinite(rd).all() and torch.isfinite(ts).all())
        assert C.rays(fam)[0] is ro                                 # built once


@pytest.mark.parametrize("fam", C.RAY_FAMILIES)
def test_box_membership_of_the_ray_families(fam):
    p = C.positions(*C.rays(fam))
    inside = C.in_box(p)
    top = np.abs(p).max()
    share = inside.mean()
    print("%-9s largest |coordinate| %8.3f, inside the box %.3f" % (fam, top, share))
    # no sample but the planted ones is within FACE_EPS of a face: one rounding of o + t d or two, the same side
    assert (np.abs(np.abs(p) - C.B).min(-1)[~C.planted(fam)] > C.FACE_EPS).all()
    if fam == "cal":
        assert inside.all() and 0.9 * C.B < top < C.B
    elif fam == "ndc-wide":
        assert 2.0 < top <= 2.5 and np.abs(p[:, 2]).max() == 1.0 and 0.5 < share < 1.0
    elif fam == "box":
        assert inside.all() and top == C.B
        for k in range(3):                                          # every face is reached, and the box is filled
            assert p[:, k].max() == C.B and p[:, k].min() == -C.B
            assert np.histogram(p[:, k], 8, (-C.B, C.B))[0].min() >= 0.8 * len(p) / 8
        assert (np.abs(p[6 * C.BOX_SHAPE[1]]) == C.B).all()                    # ray 6's first sample: a corner
        assert C.planted(fam).sum() == C.BOX_FACE_RAYS and inside[C.planted(fam)].all()
    elif fam == "mid":
        assert 7.5 < top <= 8.0 and 0.01 < share < 0.5
    elif fam == "wide":
        assert 95.0 < top <= 100.0 and share < 0.05
    elif fam == "far-llff":
        ro, rd, ts = C.rays(fam)
        ref = nk.ray_inputs(C.R, C.N)
        assert torch.equal(ro, ref[0]) and torch.equal(rd, ref[1]) and 2.0 <= float(ts.min()) and float(ts.max()) <= 6.0
        assert p[:, 2].min() >= 3.0 and share == 0.0                # z = -1 + 2 t >= 3: behind the box
    else:
        by_ray = inside.reshape(C.R, C.N)
        n_plain = C.R - len(C.STRADDLE_PINS)
        for r in range(n_plain):                                    # outside, inside, outside again along the ray
            flips = np.flatnonzero(np.diff(by_ray[r].astype(int)))
            assert len(flips) == 2 and not by_ray[r, 0] and not by_ray[r, -1] and by_ray[r, flips[0] + 1], r
        assert sorted({a for _, a, _ in C.STRADDLE_PINS} | {r % 3 for r in range(n_plain)}) == [0, 1, 2]


def test_planted_samples_of_the_straddle_family():
    ro, rd, ts = (x.numpy() for x in C.rays("straddle"))
    p = C.positions(*C.rays("straddle")).reshape(C.R, C.N, 3)
    inside = C.in_box(p)
    # a coordinate exactly on a face is inside: ray 0 at t = 0.25 (-B), ray 1 at t = 0.75 (+B), 4 B t being exact
    for r, t, want in ((0, 0.25, -C.B), (1, 0.75, C.B)):
        j = int(np.flatnonzero(ts[r] == np.float32(t))[0])
        assert p[r, j, r % 3] == want and inside[r, j]
        assert not inside[r, j - 1 if t == 0.25 else j + 1]
    n_plain = C.R - len(C.STRADDLE_PINS)
    assert len(C.STRADDLE_PINS) == 18 and n_plain == 19
    ulp = np.spacing(C.B)
    seen = set()
    for i, (k, a, v) in enumerate(C.STRADDLE_PINS):
        r = n_plain + i
        assert rd[r, k] == 0.0 and (p[r, :, k] == v).all()          # o + t 0: the pinned coordinate of every sample, exactly
        travel = np.abs(p[r, :, a]) <= C.B
        assert travel.any() and not travel.all()
        if abs(v) > C.B:                                            # one ulp outside: no sample of the ray is inside
            assert abs(v) - C.B == ulp and not inside[r].any()
        else:                                                       # on the face or one ulp inside: the travel axis decides
            assert C.B - abs(v) in (0.0, ulp / 2) and np.array_equal(inside[r], travel)
        seen.add((k, np.sign(v), float(np.sign(abs(v) - C.B)) if abs(v) != C.B else 0.0))
    assert len(seen) == 18                                          # three axes x two faces x (outside, on, inside)
    assert np.nextafter(C.B, 0.0) == C.B - ulp / 2                  # (B is a power of two: the spacing halves below it)


@pytest.mark.parametrize("net", list(C.NETS))
@pytest.mark.parametrize("fam", list(C.ZERO_SETS))
def test_zero_crossing_sets_meet_their_conditions(net, fam):
    X = C.ZERO_SETS[fam]
    for wf in C.WEIGHT_FAMILIES:
        case = (net, wf, fam)
        ro, rd, ts = C.case_rays(case)
        assert ro.shape == (C.ZERO_R, 3) and ts.shape == (C.ZERO_R, C.N)
        assert len(np.unique(np.concatenate([ro.numpy(), rd.numpy()], 1), axis=0)) == C.ZERO_R      # distinct rays
        assert bool((ts[:, 1:] > ts[:, :-1]).all()) and 0.0 < float(ts.min()) and float(ts.max()) < 1.0
        p = C.positions(ro, rd, ts)
        inside = C.in_box(p)
        top = np.abs(p).max(-1)
        if X is None:
            assert inside.all()
        else:
            assert not inside.any() and 0.8 * X <= top.min() and top.max() <= 1.2 * X
        ref = C.case_ref(case).reshape(C.ZERO_R, C.N)
        pos, near = (ref > 0).mean(), (np.abs(ref) <= 8).mean()
        print("%-6s %-8s %-9s sigma64 > 0: %.3f, |sigma64| <= 8: %.3f, range %.2f .. %.2f, tau %.4f, rays scanned / bisected / usable %s" % (
            net, wf, fam, pos, near, ref.min(), ref.max(), C.tau(case), C.ZERO_STATS[(net, C.function_of(wf), X)]))
        assert 0.3 <= pos <= 0.7 and near >= 0.9
        assert ((ref > 0).any(1) & (ref < 0).any(1)).all()          # every ray contributes both signs
        assert ref.max() >= 2.0 and ref.min() <= -2.0               # ... out to the scale of the margins
    assert C.rays(fam, net, "rows")[0] is C.rays(fam, net, "base")[0] is C.rays(fam, net, "outliers")[0]
    assert C.rays(fam, net, "dead")[0] is not C.rays(fam, net, "base")[0]


def test_every_case_has_samples_the_exact_kernel_keeps_live():
    """2b of the sweep needs them: float64 densities above the exact kernel's own allowance tau, in every case; and the
    references are finite, of both signs, built once"""
    for case in C.CASES:
        ref = C.case_ref(case)
        assert np.isfinite(ref).all() and (ref > C.tau(case)).sum() >= 100 and (ref < 0).sum() >= 100, case
        assert C.case_ref(case) is ref and not ref.flags.writeable
        net, wf, fam = case
        scale = nk.K_X3 * nk.TIGHT["fp16x3"] if net == "coarse" else nk.TOL_MX
        assert C.tau(case) == scale * np.abs(ref).max()


def test_sigma64_is_the_oracle():
    from oracle import fields
    for net in C.NETS:
        for wf in ("base", "dead"):
            p = torch.from_numpy(C.positions(*C.rays("mid")))[:500]
            with torch.no_grad():
                want = fields.style_nerf(C.S.T(C.state(net, wf), torch.float64), p, torch.zeros_like(p), dtype=torch.float64)["sigma"]
            assert np.array_equal(C.sigma64(net, wf, p), want.numpy())


def test_weight_families_of_the_coarse_net():
    base = C.state("coarse", "base")
    assert C.state("coarse", "base") is base
    p = C.positions(*C.rays("box"))[::8]
    ref = C.sigma64("coarse", "base", p)
    for wf in ("rows", "outliers"):
        sd = C.state("coarse", wf)
        assert any(not np.array_equal(sd[k], base[k]) for k in sd)
        assert np.abs(C.sigma64("coarse", wf, p) - ref).max() <= 1e-9 * np.abs(ref).max()
    assert np.abs(C.sigma64("coarse", "dead", p) - ref).max() > 1e-2 * np.abs(ref).max()
    assert C.state("fine", "rows") is nk.states("rows")


def test_the_box_holds_the_frames():
    """Every position of the benchmark's 400 x 400 NDC frames and of the tests' fern orbit (the same 120 poses, all of them)
    at t in [0, 1], and of the ray generators the tests use, is inside the box -- with room: a frame never meets the domain
    rule.  The rays are the oracle's (oracle.rays.frame_rays_ndc); those of utils.gen_rays, which the renders use, are held to
    the same bound on the device in test_screen_domain_gpu.test_case_lists_reach_the_shapes_named."""
    top = C.frame_extent()
    small = C.frame_extent(8, 8, poses=(2,))
    print("largest |coordinate|: 400 x 400 frames %.4f, the 8 x 8 frame of smoke() %.4f; box %.1f" % (top, small, C.B))
    assert max(top, small) <= C.B - 0.5
    for ro, rd, ts in (nk.ray_inputs(130, 128), C.chain_rays((5, 192))):
        assert C.in_box(C.positions(ro, rd, ts)).all()


def test_model_of_the_screen_for_the_record():
    """error / margin of a plain fp16 model, margin = 8 x its largest error on `cal`: printed, nothing asserted on it"""
    for net in C.NETS:
        m = 8 * C.model_error(net, "base", C.positions(*C.rays("cal"))).max()
        print(net, "model margin %.3f;" % m, "  ".join("%s %.2f" % (
            fam, C.model_error(net, "base", C.positions(*C.rays(fam, net, "base"))).max() / m) for fam in C.FAMILIES))
