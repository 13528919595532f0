"""GPU: the density screen against float64, inside and far outside its declared box (tests/screen_cases.py; DESIGN 3.1 "The
screen's domain").  A screened render has the bits of a dense one as long as no sample the screen drops (sigma_screen <=
-margin) is live in the exact kernel; the margin is calibrated on the box |x|, |y|, |z| <= B = 2, and a sample outside it
is a candidate by construction (its screen density is NaN).  Swept here for the two nets x four weight families x eleven ray
families (seven by position, four around zeros of the float64 density at |x| up to 100):

  a  no sample the exact kernel has live is dropped;                       b  none that float64 has live beyond the exact
  c  inside the box the error is at most half the margin and the              kernel's own allowance tau is dropped;
     screen is within the fp16 bar of float64;                              d  the screen's packed form gives the bits of an
  e  screened renders equal dense renders in bits at near up to 50;            fp16 handle, which the per-sample sweep holds
  f  exactly the samples outside the box (or not finite) come out NaN.         to float64.

Figures on the MI355X: profiles/screen_domain.json.  Before the box (the margin calibrated on |x|, |y| <= 2.5, |z| <= 1 and
every finite position screened) a and b failed in the same 11 of the 88 cases each -- zero-100 for both nets in every weight
family (98 .. 108 of about 2 060 live samples dropped by the coarse net's screen, 179 .. 309 by the fine net's; errors up to
3.6 and 5.3 margins) and zero-30 for the fine net in base, rows and outliers (5 .. 7 dropped, errors up to 1.7 margins) --
and e failed at near 50 with the median at +margin / 2.  `wide` had errors of 2.3 .. 3.9 margins on hundreds of dropped
samples and lost no live one only because densities out there are in the thousands: the zero-crossing sets are what bites."""
import json
import math
import os

import numpy as np
import pytest
import torch

import nerf_kernel_cases as nk
import screen_cases as C
import test_density_screen_gpu as D

pytestmark = pytest.mark.gpu

SERIAL, CFGFAST = "TGTC_SCREEN_SERIAL_FRONT", "TGTC_SCREEN_CFGFAST"
SENTINEL = -7.25
RENDER_R, RENDER_COUNTS = 130, (128, 64)
NEARS = [0.5, 4.0, 16.0, 50.0]
PLAIN_RANGES = [(2.0, 6.0), (0.0, 50.0)]
RULE_FAMILIES = ["straddle", "wide", "mid", "far-llff", "ndc-wide"]

_handles = {}


def handle(net, wf, precision=None):
    """the packed handle of a net in a weight family with its screen enabled (once a module); precision 'fp16': the plain
    fp16 handle of the same state dict"""
    from tgtc_style_amd import hip
    assert SERIAL not in os.environ and CFGFAST not in os.environ
    key = (net, wf, precision)
    if key not in _handles:
        h = hip.nerf_create(C.state(net, wf), precision or C.NETS[net][1])
        if precision is None:
            h.enable_screen()
            assert h.screen_margin() > 0
        _handles[key] = h
    return _handles[key]


def launch(which, h, ro, rd, ts):
    """densities [R * N] (numpy) of tgtc_nerf_screen_rays / tgtc_nerf_forward_rays (sigma only) with 64 canaries behind them"""
    from tgtc_style_amd import hip
    lib = hip.load()
    R, n = ts.shape
    ro, rd, ts = ro.cuda().contiguous(), rd.cuda().contiguous(), ts.cuda().contiguous()
    out = torch.full((R * n + 64,), SENTINEL, device="cuda")
    if which == "screen":
        hip.check(lib.tgtc_nerf_screen_rays(h.handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, n, hip.ptr(out), hip.stream()))
    else:
        hip.check(lib.tgtc_nerf_forward_rays(h.handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, n, None, hip.ptr(out), hip.stream()))
    torch.cuda.synchronize()
    assert bool((out[R * n:] == SENTINEL).all())
    return out[:R * n].cpu().numpy()


_out = {}


def outputs(case):
    """(margin, screen, exact) of a case: launched once, never written again"""
    if case not in _out:
        net, wf, _ = case
        h = handle(net, wf)
        screen, exact = launch("screen", h, *C.case_rays(case)), launch("exact", h, *C.case_rays(case))
        assert np.isfinite(exact).all()
        screen.setflags(write=False), exact.setflags(write=False)
        _out[case] = (h.screen_margin(), screen, exact)
    return _out[case]


# ------------------------------------------------------------------------------------------------ a, b: nothing live is dropped
@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_no_sample_the_exact_kernel_has_live_is_dropped(case):
    m, screen, exact = outputs(case)
    dropped = screen <= -m                              # (a NaN, the density of a sample outside the box, is a candidate)
    err = np.abs(screen - exact)[dropped]
    lost = int(((exact > 0) & dropped).sum())
    inside = C.in_box(C.positions(*C.case_rays(case)))
    fin = np.isfinite(screen)
    print("SCREEN_DOMAIN " + json.dumps({
        "net": case[0], "weights": case[1], "rays": case[2], "margin": round(m, 4), "inside_box": round(float(inside.mean()), 4),
        "candidate_share": round(float(1 - dropped.mean()), 4), "live_exact": int((exact > 0).sum()), "live_dropped": lost,
        "dropped_max_err_over_margin": round(float(err.max() / m), 4) if err.size else None,
        "dropped_with_err_ge_margin": int((err >= m).sum()),
        "finite_max_err_over_margin": round(float(np.abs(screen - exact)[fin].max() / m), 4) if fin.any() else None}))
    assert lost == 0


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_no_sample_float64_has_live_is_dropped(case):
    m, screen, _ = outputs(case)
    ref, tau = C.case_ref(case), C.tau(case)
    live = ref > tau
    lost = int((live & (screen <= -m)).sum())
    print("%-28s tau %.4f: float64 densities above it %d, dropped %d" % (C.case_id(case), tau, int(live.sum()), lost))
    assert live.sum() > 0
    assert lost == 0


# ------------------------------------------------------------------------------------------------ c: headroom inside the box
@pytest.mark.parametrize("case", C.DOMAIN_CASES, ids=C.case_id)
def test_headroom_inside_the_domain(case):
    m, screen, exact = outputs(case)
    ref = C.case_ref(case)
    assert np.isfinite(screen).all()
    err = float(np.abs(screen - exact).max())
    rel = float(np.abs(screen - ref).max() / np.abs(ref).max())
    print("%-22s max |screen - exact| = %.4f = %.3f margins (margin %.4f); screen against float64 %.3e of max |sigma64| (bar %.0e)" % (
        C.case_id(case), err, err / m, m, rel, nk.TIGHT["fp16"]))
    assert err <= 0.5 * m
    assert rel <= nk.TIGHT["fp16"]


# ------------------------------------------------------------------------------------------------ d: the chain to float64
@pytest.mark.parametrize("wf", C.CHAIN_WEIGHTS)
@pytest.mark.parametrize("shape", C.CHAIN_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("net", list(C.NETS))
def test_screen_form_has_the_bits_of_an_fp16_handle(net, shape, wf):
    """kernel C of the per-sample sweep (an fp16 handle's sigma-only launch over rays) is what that sweep holds to float64; the
    screen packs its own fp16 form from the fp16x3 / fp16mx handle's layers and runs it through another kernel"""
    ro, rd, ts = C.chain_rays(shape)
    assert C.in_box(C.positions(ro, rd, ts)).all()
    screen = launch("screen", handle(net, wf), ro, rd, ts)
    fp16 = launch("exact", handle(net, wf, "fp16"), ro, rd, ts)
    assert np.isfinite(fp16).all() and (fp16 != SENTINEL).all()
    assert np.array_equal(screen, fp16)


# ------------------------------------------------------------------------------------------------ e: renders far from the box
def crowded(pair, near, sign):
    """the recipe of test_density_screen_gpu.test_densities_inside_the_margin at depth `near`: two rays repeated, depths
    crowded into [near, near + width], sigma heads shifted so that the median density is sign * margin / 2; the stretch is
    the longest of a fixed list at which a fifth of the shifted densities of either net lies within margin / 2 of that"""
    from tgtc_style_amd import hip
    lib = hip.load()
    R, (nc, nf) = RENDER_R, RENDER_COUNTS
    ro, rd = D.frame_rays(3, 2)
    ro, rd = ro.repeat(R // 2, 1).contiguous(), rd.repeat(R // 2, 1).contiguous()
    margins = [m.packed().screen_margin() for m in pair]
    for width in (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 0.0):
        ts = torch.linspace(near, near + width, nc, device="cuda").repeat(R, 1).contiguous()
        shifts, inside = [], []
        for net, m in zip(pair, margins):
            sigma = torch.empty(R * nc, device="cuda")
            hip.check(lib.tgtc_nerf_forward_rays(net.packed().handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, nc, None,
                                                 hip.ptr(sigma), hip.stream()))
            torch.cuda.synchronize()
            shifts.append(sign * 0.5 * m - float(sigma.median()))
            inside.append(float(((sigma + shifts[-1] - sign * 0.5 * m).abs() < 0.5 * m).float().mean()))
        if min(inside) >= 0.2:
            break
    return ro, rd, width, shifts, inside


@pytest.mark.parametrize("sign", [-1, 1], ids=["below", "above"])
@pytest.mark.parametrize("near", NEARS)
def test_screened_render_of_crowded_depths_far_out(near, sign):
    R, (nc, nf) = RENDER_R, RENDER_COUNTS
    pair = D.make()
    for m in pair:
        m.packed().enable_screen()
    ro, rd, width, shifts, inside = crowded(pair, near, sign)
    print("near %g: depth stretch %g, shifts %s, share within margin / 2 of %+d margin / 2: %s" % (near, width, shifts, sign, inside))
    assert min(inside) >= 0.2
    nets = D.make(shift=shifts)
    off, _, _ = D.render(nets, ro, rd, nc, nf, False, near=near, far=near + width)
    on, sc, sf = D.render(nets, ro, rd, nc, nf, True, near=near, far=near + width)
    print("candidate shares", nets[0].packed().screen_fraction(), nets[1].packed().screen_fraction(), "live", nets[1].packed().live_fraction())
    assert (sc, sf) == (1, 1)
    if near == 0.5:                                 # inside the box: the screen really is undecided on a fifth of the samples
        assert nets[0].packed().screen_fraction() >= 0.2
    else:                                           # outside it every sample is a candidate
        assert nets[0].packed().screen_fraction() == nets[1].packed().screen_fraction() == 1.0
    assert bool(off["rgb"].any()) and bool(torch.isfinite(off["rgb"]).all())
    D.same(on, off)


@pytest.mark.parametrize("near,far", PLAIN_RANGES)
def test_screened_render_of_depth_ranges_outside_ndc(near, far):
    R, (nc, nf) = RENDER_R, RENDER_COUNTS
    ro, rd, _ = nk.ray_inputs(R, nc)
    ro, rd = ro.cuda().contiguous(), rd.cuda().contiguous()
    pair = D.make()
    off, _, _ = D.render(pair, ro, rd, nc, nf, False, near=near, far=far)
    on, sc, sf = D.render(pair, ro, rd, nc, nf, True, near=near, far=far)
    print("near %g far %g: candidate shares %.4f %.4f, live %.4f" % (
        near, far, pair[0].packed().screen_fraction(), pair[1].packed().screen_fraction(), pair[1].packed().live_fraction()))
    assert (sc, sf) == (1, 1)
    assert bool(off["rgb"].any()) and bool(torch.isfinite(off["rgb"]).all())
    D.same(on, off)


# ------------------------------------------------------------------------------------------------ f: the rule outside the box
def in_box_stand_in(ro, rd, ts, inside):
    """the launch with every sample outside the box replaced by one inside it: a depth of the same ray that is inside, or,
    where a ray has none, a ray of the `cal` family"""
    ro, rd, ts = ro.clone(), rd.clone(), ts.clone()
    cal = C.rays("cal")
    for r in range(ts.shape[0]):
        if inside[r].any():
            ts[r, ~torch.from_numpy(inside[r])] = ts[r, int(np.flatnonzero(inside[r])[0])]
        else:
            ro[r], rd[r], ts[r] = cal[0][r % C.R], cal[1][r % C.R], cal[2][r % C.R, :ts.shape[1]]
    assert C.in_box(C.positions(ro, rd, ts)).all()
    return ro, rd, ts


def three_ways(h, ro, rd, ts, monkeypatch):
    outs = []
    for switch in (None, SERIAL, CFGFAST):
        for k in (SERIAL, CFGFAST):
            monkeypatch.delenv(k, raising=False)
        if switch:
            monkeypatch.setenv(switch, "1")
        outs.append(launch("screen", h, ro, rd, ts))
        if switch:
            monkeypatch.delenv(switch)
    return outs


@pytest.mark.parametrize("fam", RULE_FAMILIES)
@pytest.mark.parametrize("net", list(C.NETS))
def test_samples_outside_the_box_are_nan_and_nothing_else_is(net, fam, monkeypatch):
    ro, rd, ts = (x.clone() for x in C.rays(fam))
    if fam == "straddle":                           # ... "or a non-finite one": a NaN origin, an infinite depth
        ro[3, 1] = float("nan")
        ts[5, 40] = float("inf")
    with np.errstate(invalid="ignore"):
        inside = C.in_box(C.positions(ro, rd, ts)).reshape(ts.shape)
    if fam == "straddle":
        assert not inside[3].any() and not inside[5, 40] and inside[5].any()
    h = handle(net, "base")
    new, serial, old = three_ways(h, ro, rd, ts, monkeypatch)
    clean = launch("screen", h, *in_box_stand_in(ro, rd, ts, inside))
    inside = inside.reshape(-1)
    print("%s %s: %d of %d samples inside the box, %d finite densities" % (net, fam, inside.sum(), inside.size, np.isfinite(new).sum()))
    assert np.isfinite(clean).all()
    assert np.array_equal(np.isfinite(new), inside) and np.isnan(new[~inside]).all()
    assert np.array_equal(new, serial, equal_nan=True)
    assert np.array_equal(new[inside], clean[inside])               # no leak across the tiles that mix rays
    assert np.array_equal(new[inside], old[inside])                 # (the CfgFast launch knows no box: in-box samples only)


@pytest.mark.parametrize("out_tile,face_tile", [(0, 3), (3, 0)])
def test_box_rule_in_a_prefetched_pass(out_tile, face_tile, monkeypatch):
    """The placement of test_screen_front_gpu: rays of 16 samples are tiles, and the stream of an earlier pass encodes the
    second pass of workgroup 1 and the third of workgroup 2.  A ray outside the box in one, a ray exactly on a face (inside)
    and one an ulp beyond it in the other."""
    import test_screen_stream_gpu as S
    n = 16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    R = math.ceil(2.2 * cus * 256 / n) + 3
    r_out = 16 * (cus + 1) + 4 * 1 + out_tile
    r_face = 16 * (2 * cus + 2) + 4 * 2 + face_tile
    r_ulp = r_face + (1 if face_tile == 0 else -1)
    assert max(r_face, r_ulp) < R
    ro, rd, ts = (x.cpu() for x in S.inputs(R, n))
    clean_in = (ro.clone(), rd.clone(), ts)
    ro[r_out, 0] = C.B + 0.5                                        # x = B + 0.5 + t dx, |dx| <= 0.3: outside
    ro[r_face, 1], rd[r_face, 1] = -C.B, 0.0                        # y = -B exactly: inside
    ro[r_ulp, 1], rd[r_ulp, 1] = np.nextafter(-C.B, -np.inf), 0.0
    face_in = (ro.clone(), rd.clone(), ts)
    for r in (r_out, r_ulp):
        face_in[0][r], face_in[1][r] = clean_in[0][r], clean_in[1][r]
    inside = C.in_box(C.positions(ro, rd, ts))
    want = np.ones((R, n), bool)
    want[r_out] = want[r_ulp] = False
    assert np.array_equal(inside, want.reshape(-1))
    for net in C.NETS:
        h = handle(net, "base")
        new, serial, old = three_ways(h, ro, rd, ts, monkeypatch)
        clean = launch("screen", h, *face_in)
        assert np.isfinite(clean).all()
        assert np.array_equal(np.isnan(new), ~inside) and np.array_equal(np.isfinite(new), inside)
        assert np.array_equal(new, serial, equal_nan=True)
        assert np.array_equal(new[inside], clean[inside])
        assert np.array_equal(new[inside], old[inside])


def test_case_lists_reach_the_shapes_named():
    assert NEARS == [0.5, 4.0, 16.0, 50.0] and PLAIN_RANGES == [(2.0, 6.0), (0.0, 50.0)]
    assert RENDER_R == 130 and RENDER_COUNTS == (128, 64) and D.fits(130, 128, 64) == (True, True)
    assert RULE_FAMILIES == ["straddle", "wide", "mid", "far-llff", "ndc-wide"]
    shares = {fam: C.in_box(C.positions(*C.rays(fam))).mean() for fam in RULE_FAMILIES}
    for pose in (0, 3, 60, 119):                    # the frames the screen's tests and the benchmark render: utils.gen_rays
        o, d = D.frame_rays(pose, 2048)
        top = float(torch.maximum(o.abs().max(), (o + d).abs().max()))
        assert top <= C.B - 0.5, (pose, top)
    assert shares["wide"] == shares["far-llff"] == 0 and all(0.01 < shares[f] < 0.99 for f in ("straddle", "mid", "ndc-wide"))
