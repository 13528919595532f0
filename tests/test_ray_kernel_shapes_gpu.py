"""GPU: the two ray kernels (csrc/render_fused.hip in its three precision pairs, csrc/render_styled_fused.hip) swept over the
sample-count grid tgtc_render_path declares them built for, every ray held to a reference, no ray exempt.

tests/test_fused_gpu.py meets them at 128+64 and 64+64 (16+16 against the chain) with the 1e-3 end-to-end bar, which cannot be
tighter because the inverse-CDF sampler amplifies rounding (tests/conditioning.py).  Here the comparison is CONDITIONAL on
the kernel's own merged depths ts_k, which tgtc_render_depths / RayRenderer.ray_kernel_depths make observable (the
depths-only instance of the plain ray kernel on the kernel's coarse handle):

  depths   ts_k ascending; every coarse depth (tgtc_sample_coarse) in it bit for bit, as a multiset; on 16 rays
           conditioning.sampler_bound(ts_c, w_c, ts_k) == 0 with w_c from the per-stage operators at the coarse precision,
           and for a coarse fp16x3 |w_c - float32 oracle's| <= 2e-5 (certificate 2a of tests/conditioning.py).
  R1       network + compositing: |pixel - float64 oracle at ts_k| <= LIMIT of tests/test_fused_gpu.py (absolute, rgb and t);
           where the fine precision is fp16x3 also <= K[family] x y, y = max(|float32 - float64 conditional oracle| of that
           case, 1.2e-7): the rule of tests/test_hip_style_shapes.py.
  R2       compositing + tile indexing alone: the per-sample kernel of the same precision on the same rays and ts_k
           (tgtc_nerf_forward_rays / tgtc_styled_forward_rays), composited by oracle.raymarch.composite in float64;
           |pixel - that| <= K2[kernel] x y2, y2 = max(|float32 composite - float64 composite| of those inputs, 1.2e-7).

K and K2 are powers of two: the next one at or above 4 x the worst err / y measured on the MI355X over this file's cases
(4 x: another shape legitimately sums in another order).  DESIGN.md section 4, "The ray-kernel shape sweep", has the table.
tests/test_ray_kernel_shapes_cpu.py holds what this rests on: the case lists, y <= 1e-5 and the sampler bound's exactness on
the oracle's own depths.  Every error, y and bar is printed."""
import numpy as np
import pytest
import torch

import conditioning
import ray_kernel_cases as rk

pytestmark = pytest.mark.gpu

LIMIT = {"fp16x3": 1e-3, "fp16mx": 1e-3, "fp16": 2e-2}      # tests/test_fused_gpu.py, by fine precision
W_COARSE = 2e-5                                            # tests/conditioning.py, certificate 2a
Y_FLOOR = 1.2e-7                                           # float32 epsilon (tests/test_hip_style_shapes.py)
# kernel -> (coarse precision, fine precision, stylised, step of the case list)
KERNELS = {"fp16x3+fp16x3": ("fp16x3", "fp16x3", False, 16), "fp16x3+fp16mx": ("fp16x3", "fp16mx", False, 16),
           "fp16+fp16": ("fp16", "fp16", False, 32), "styled": ("fp16x3", "fp16x3", True, 16)}
# DESIGN.md section 4, "The ray-kernel shape sweep".  Worst err / y measured on the MI355X over this file's cases: plain rgb
# 3.19, plain t 2.99, styled rgb 3.31, styled t 2.99; K = the next power of two at or above 4 x that.  K x y stays below 4e-5.
K = {"plain rgb": 16, "plain t": 16, "styled rgb": 16, "styled t": 16}
# worst err / y2 (rgb or t): fp16x3+fp16x3 2.34, fp16x3+fp16mx 2.92, fp16+fp16 3.36, styled 2.34.  K2 x y2 stays below 5e-6:
# the per-sample network arithmetic of all four ray kernels IS the per-sample kernel's, fp16mx and fp16 included.
K2 = {"fp16x3+fp16x3": 16, "fp16x3+fp16mx": 16, "fp16+fp16": 16, "styled": 16}
CANARY_ROWS, CANARY = 64, -7.0
SWEEP = [(k, case) for k, v in KERNELS.items() for case in rk.CASES[v[3]]]
SWEEP_IDS = ["%s-%s" % (k, rk.case_id(case)) for k, case in SWEEP]


class Args:
    use_viewdir, act_type = True, "relu"
    embed_freq_coor, embed_freq_dir = 10, 4
    netdepth = netdepth_fine = 8
    netwidth = netwidth_fine = 256
    style_D, vae_latent = 8, 32
    precision = "fp16x3"


_R = {}


def renderer(kernel, sigma_const=None):
    """RayRenderer(fused="single") of a kernel over the synth nets (seeds 0 / 1 / 2 / 3), built once."""
    if (kernel, sigma_const) not in _R:
        from tgtc_style_amd import models, rendering
        pc, pf, styled, _ = KERNELS[kernel]
        c, f, cs, ss = rk.states(sigma_const=sigma_const)
        nets = []
        for sd, mode, prec in ((c, "coarse", pc), (f, "fine", pf)):
            m = models.StyleNerf(type("A", (Args,), {"precision": prec}), mode=mode)
            m.load_state_dict(sd)
            nets.append(m.cuda())
        pair = None
        if styled:
            cm, sm = models.StyleMLP_before_concat(Args), models.StyleMLP_Wild_multilayers(Args)
            cm.load_state_dict(cs), sm.load_state_dict(ss)
            pair = models.StylePair(cm.cuda(), sm.cuda())
        _R[kernel, sigma_const] = rendering.RayRenderer(nets[0], nets[1], style=pair, fused="single")
    return _R[kernel, sigma_const]


def inputs(kernel, case, n=rk.R):
    """(ro, rd, z or None, jitter or None) of a case on the CPU."""
    ro, rd = rk.rays(n)
    z = rk.latents(n) if KERNELS[kernel][2] else None
    return ro, rd, z, (rk.jitter(n, case[0]) if case[2] else None)


def gpu(t):
    return None if t is None else t.cuda().contiguous()


def launch(r, case, ro, rd, z, jit):
    """One launch of the ray kernel and one of its depths-only instance through the C ABI, every output with CANARY_ROWS
    rows more than the kernel may write: -> rgb [R,3], t [R], ts_k [R, nc + nf] (device; the canaries are asserted)."""
    from tgtc_style_amd import hip
    lib = hip.load()
    nc, nf, _, near, far = case
    R = ro.shape[0]
    rgb = torch.full((R + CANARY_ROWS, 3), CANARY, device="cuda")
    t = torch.full((R + CANARY_ROWS,), CANARY, device="cuda")
    ts = torch.full((R + CANARY_ROWS, nc + nf), CANARY, device="cuda")
    tail = (hip.PATH_RAY_KERNEL, None, 0, hip.ptr(rgb), hip.ptr(t), None, None, hip.stream())
    if z is None:
        hip.check(lib.tgtc_render_rays_plain(r.coarse.packed().handle, r.fine.packed().handle, hip.ptr(ro), hip.ptr(rd), R, nc, nf,
                                             near, far, hip.ptr(jit), *tail))
    else:
        hip.check(lib.tgtc_render_rays_styled(r.coarse.packed().handle, r.fine.packed().handle, r.style.packed().handle,
                                              hip.ptr(ro), hip.ptr(rd), hip.ptr(z), R, nc, nf, near, far, hip.ptr(jit), *tail))
    hip.check(lib.tgtc_render_depths(r.coarse.packed().handle, hip.ptr(ro), hip.ptr(rd), R, nc, nf, near, far, hip.ptr(jit),
                                     hip.ptr(ts), hip.stream()))
    torch.cuda.synchronize()
    for name, out in (("rgb", rgb), ("t", t), ("ts_out", ts)):
        assert torch.equal(out[R:], torch.full_like(out[R:], CANARY)), name + ": wrote behind its output"
        assert bool((out[:R] != CANARY).all()), name + ": left part of its output unwritten"
        assert bool(torch.isfinite(out[:R]).all()), name + ": not finite"
    return rgb[:R], t[:R], ts[:R]


def per_sample(r, ro, rd, ts, z):
    """The per-sample kernel of the fine precision on (rays, ts): rgb [R,N,3], sigma [R,N] on the CPU."""
    from tgtc_style_amd import hip
    lib = hip.load()
    R, N = ts.shape
    rgb = torch.full((R * N, 3), float("nan"), device="cuda")
    sigma = torch.full((R * N,), float("nan"), device="cuda")
    ts = ts.contiguous()
    if z is None:
        hip.check(lib.tgtc_nerf_forward_rays(r.fine.packed().handle, hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, N, hip.ptr(rgb),
                                             hip.ptr(sigma), hip.stream()))
    else:
        hip.check(lib.tgtc_styled_forward_rays(r.fine.packed().handle, r.style.packed().handle, hip.ptr(ro), hip.ptr(rd),
                                               hip.ptr(ts), hip.ptr(z), R, N, hip.ptr(rgb), hip.ptr(sigma), hip.stream()))
    torch.cuda.synchronize()
    return rgb.view(R, N, 3).cpu(), sigma.view(R, N).cpu()


# ------------------------------------------------------------------------------------------------------- checks
def check_depths(kernel, case, r, ro, rd, jit, ts_k, sub, sigma_const=None):
    """The stage checks on ts_k [R, nc + nf] (device): ascending, the coarse depths as a multiset, and on the rays `sub` the
    sampler bound on the per-stage operators' coarse weights (+ certificate 2a for a coarse fp16x3)."""
    from tgtc_style_amd import utils
    nc, nf, _, near, far = case
    assert bool((ts_k[:, 1:] >= ts_k[:, :-1]).all()), "merged depths not ascending"
    ts_c = utils.sampling_pts_uniform(ro, rd, nc, near=near, far=far, jitter=jit)[1]
    tk, tc = ts_k.cpu().numpy().view(np.int32), ts_c.cpu().numpy().view(np.int32)
    assert (tk >= 0).all() and (tc >= 0).all()        # non-negative floats: the bit patterns sort like the values
    for i in range(tk.shape[0]):
        uc, cc = np.unique(tc[i], return_counts=True)
        uk, ck = np.unique(tk[i], return_counts=True)
        pos = np.minimum(np.searchsorted(uk, uc), uk.size - 1)
        assert (uk[pos] == uc).all() and (ck[pos] >= cc).all(), "ray %d: a coarse depth is missing from the merged depths" % i
    st = conditioning.hip_stages(r.coarse, ro[sub], rd[sub], nc, nf, near=near, far=far, jitter=None if jit is None else jit[sub])
    assert torch.equal(st["ts_c"], ts_c[sub].cpu())
    excess = conditioning.sampler_bound(st["ts_c"], st["w_c"], ts_k[sub].cpu(), nf)
    note = ""
    if KERNELS[kernel][0] == "fp16x3":
        w_or = rk.oracle_render("plain", case, ro[sub].cpu(), rd[sub].cpu(), jit=None if jit is None else jit[sub].cpu(),
                                 sigma_const=sigma_const)["w_coarse"]
        e_w = float((st["w_c"] - w_or).abs().max())
        note = "  coarse weights vs float32 oracle %.2e (bar %.0e)" % (e_w, W_COARSE)
        assert e_w <= W_COARSE, (kernel, case, e_w)
    print("%-14s %-22s depths: %d rays ascending with their coarse depths; sampler excess max %.1e on %d rays%s" % (
        kernel, rk.case_id(case), tk.shape[0], float(excess.max()), len(sub), note))
    assert float(excess.max()) == 0.0, (kernel, case, excess.tolist())


def check_pixels(kernel, label, case, r, ro, rd, z, rgb, t, ts_k, sigma_const=None):
    """R1 and R2 for the rays given (device tensors; every ray counts).  Returns the err / y figures of the table."""
    from oracle import raymarch
    pf, styled = KERNELS[kernel][1], KERNELS[kernel][2]
    kind = "styled" if styled else "plain"
    got = (rgb.cpu().double(), t.cpu().double())
    ts_cpu = ts_k.cpu()
    # R1
    ref, ys = rk.conditional(kind, case, ro.cpu(), rd.cpu(), ts_cpu, None if z is None else z.cpu(), sigma_const)
    figures = {}
    for name, g, want, y in zip(("rgb", "t"), got, ref, ys):
        e, y = float((g - want).abs().max()), max(y, Y_FLOOR)
        fam = "%s %s" % (kind, name)
        bar = min(LIMIT[pf], K[fam] * y) if pf == "fp16x3" else LIMIT[pf]
        print("%-14s %-22s R1 %-10s err %.3e  y %.3e  err/y %9.2f  bar %.3e" % (kernel, label, fam, e, y, e / y, bar))
        assert e <= bar, ("R1", kernel, label, fam, e, y, bar)
        figures["R1 " + fam] = e / y
    # R2
    rgb_s, sig_s = per_sample(r, ro, rd, ts_k, z)
    c64 = raymarch.composite(rgb_s.double(), sig_s.double(), ts_cpu.double())[:2]
    c32 = raymarch.composite(rgb_s, sig_s, ts_cpu)[:2]
    for name, g, want, lo in zip(("rgb", "t"), got, c64, c32):
        e, y2 = float((g - want).abs().max()), max(float((lo.double() - want).abs().max()), Y_FLOOR)
        bar = K2[kernel] * y2
        print("%-14s %-22s R2 %-10s err %.3e  y2 %.3e  err/y2 %8.2f  bar %.3e" % (kernel, label, name, e, y2, e / y2, bar))
        assert e <= bar, ("R2", kernel, label, name, e, y2, bar)
        figures["R2 " + name] = e / y2
    return figures


# ------------------------------------------------------------------------------------------------------- 1: the sweep
@pytest.mark.parametrize("kernel,case", SWEEP, ids=SWEEP_IDS)
def test_shape(kernel, case):
    """Every case of the kernel's list: the depth stage checks, then R1 and R2 on all 41 rays.  Through RayRenderer, as a
    caller reaches the kernels; the results are the bits of the C ABI launch with canaries behind every output."""
    r = renderer(kernel)
    nc, nf, _, near, far = case
    ro, rd, z, jit = (gpu(x) for x in inputs(kernel, case))
    assert (r._fused_styled_shape if z is not None else r._fused_shape)(nc, nf)
    out = r.render(ro, rd, nc, nf, near=near, far=far, jitter=jit, z=z)
    ts_k = r.ray_kernel_depths(ro, rd, nc, nf, near=near, far=far, jitter=jit)
    rgb, t, ts_c = launch(r, case, ro, rd, z, jit)
    assert torch.equal(out["rgb"], rgb) and torch.equal(out["t"], t) and torch.equal(ts_k, ts_c)
    check_depths(kernel, case, r, ro, rd, jit, ts_k, rk.SUB16.cuda())
    check_pixels(kernel, rk.case_id(case), case, r, ro, rd, z, rgb, t, ts_k)


# ------------------------------------------------------------------------------------------------------- 2: bit properties
def edge_cases(kernel):
    """The smallest and the full-strip shape of the kernel's list, each without and with jitter."""
    step = KERNELS[kernel][3]
    return [c for c in rk.CASES[step] if (c[0], c[1]) in (rk.SMALL[step], rk.FULL)]


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_ray_counts_and_the_rows_behind_the_outputs(kernel):
    """1, 7, 8, 9 rays from the front, the middle and the end of the 41: every sub-range reproduces the bits of the 41-ray
    launch (pixels and depths), and the 64 rows behind rgb, t and ts_out keep their canaries in every launch -- the masked
    store of the duplicated tail ray."""
    r = renderer(kernel)
    for case in edge_cases(kernel):
        ro, rd, z, jit = (gpu(x) for x in inputs(kernel, case))
        whole = launch(r, case, ro, rd, z, jit)
        for n in (1, 7, 8, 9):
            for lo in (0, 13, rk.R - n):
                part = launch(r, case, *(None if x is None else x[lo:lo + n].contiguous() for x in (ro, rd, z, jit)))
                for name, a, b in zip(("rgb", "t", "ts"), part, whole):
                    assert torch.equal(a, b[lo:lo + n]), (kernel, case, n, lo, name)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_second_and_third_visit(kernel):
    """R = 2 x 8 x CUs + 3 rays at the smallest shape: 2 x CUs + 1 groups of eight, so every persistent workgroup takes a
    second group and the one that takes the three-ray tail group a third (more where the stylised kernel runs on fewer
    workgroups than CUs).  Rays 0..40 are the 41 of the sweep and reproduce its bits; R1 and R2 on 64 rays: the first two
    groups, two groups of the second visits, two from the middle and the last 16 rays with the tail group."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    R = 2 * 8 * n_cu + 3
    step = KERNELS[kernel][3]
    case = next(c for c in rk.CASES[step] if (c[0], c[1]) == rk.SMALL[step] and c[2])       # jittered: a row per ray
    r = renderer(kernel)
    o41, d41 = rk.rays()
    o2, d2 = rk.rays(R - rk.R)
    ro, rd = torch.cat([o41, o2]), torch.cat([d41, d2])
    z = torch.cat([rk.latents(), rk.latents(R - rk.R)]) if KERNELS[kernel][2] else None
    jit = torch.cat([rk.jitter(rk.R, case[0]), rk.jitter(R - rk.R, case[0])])
    ro, rd, z, jit = (gpu(x) for x in (ro, rd, z, jit))
    rgb, t, ts = launch(r, case, ro, rd, z, jit)
    small = launch(r, case, *(None if x is None else x[:rk.R].contiguous() for x in (ro, rd, z, jit)))
    for name, a, b in zip(("rgb", "t", "ts"), small, (rgb, t, ts)):
        assert torch.equal(a, b[:rk.R]), (kernel, name)
    sel = torch.cat([torch.arange(0, 16), torch.arange(8 * n_cu, 8 * n_cu + 16), torch.arange(12 * n_cu, 12 * n_cu + 16),
                     torch.arange(R - 16, R)]).cuda()
    assert sel.numel() == 64 and int(sel.max()) == R - 1
    pick = lambda x: None if x is None else x[sel].contiguous()
    check_depths(kernel, case, r, pick(ro), pick(rd), pick(jit), pick(ts), torch.arange(0, 64, 4).cuda())
    check_pixels(kernel, "%d rays on %d CUs" % (R, n_cu), case, r, pick(ro), pick(rd), pick(z), pick(rgb), pick(t), pick(ts))


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_no_state_between_launches(kernel):
    """Shape A, then shape B, then A again gives A's bits; the same with a jittered launch of A in between (the jitter plane
    waits in the weight strip, the strips and the ring are not cleared between launches)."""
    r = renderer(kernel)
    a, b, a_jit, b_jit = edge_cases(kernel)
    assert not a[2] and a_jit[2] and (a[0], a[1]) == (a_jit[0], a_jit[1]) and (b[0], b[1]) == rk.FULL and b_jit[2]
    args = {c: tuple(gpu(x) for x in inputs(kernel, c)) for c in (a, a_jit, b_jit)}
    first = launch(r, a, *args[a])
    for between in (b_jit, a_jit):
        launch(r, between, *args[between])
        again = launch(r, a, *args[a])
        for name, x, y in zip(("rgb", "t", "ts"), again, first):
            assert torch.equal(x, y), (kernel, between, name)
    jit_first = launch(r, a_jit, *args[a_jit])
    launch(r, a, *args[a])
    for name, x, y in zip(("rgb", "t", "ts"), launch(r, a_jit, *args[a_jit]), jit_first):
        assert torch.equal(x, y), (kernel, "jittered", name)


# ------------------------------------------------------------------------------------------------------- 3: constant density
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_nothing_live(kernel):
    """Both NeRF nets with sigma = -3 everywhere: every weight is +0, so rgb == 0 and t == 0 exactly, the pdf is uniform and
    the merged depths are the oracle's uniform inverse CDF to 1e-6 (a float32 ulp of a depth below 1 is 6e-8; the cdf of
    equal weights carries no cancellation)."""
    r = renderer(kernel, sigma_const=-3.0)
    for case in edge_cases(kernel):
        ro, rd, z, jit = inputs(kernel, case)
        rgb, t, ts = launch(r, case, *(gpu(x) for x in (ro, rd, z, jit)))
        assert not bool(rgb.any()) and not bool(t.any()), (kernel, case)
        want = rk.oracle_render("plain", case, ro, rd, jit=jit, sigma_const=-3.0)["ts_fine"]
        e = float((ts.cpu() - want).abs().max())
        print("%-14s %-22s sigma = -3: depths vs the oracle's uniform inverse CDF %.2e" % (kernel, rk.case_id(case), e))
        assert e <= 1e-6, (kernel, case, e)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_everything_dense(kernel):
    """Both NeRF nets with sigma = 8 everywhere (every sample live, the transmittance falls through all tiles): the depth
    stage checks, R1 and R2."""
    r = renderer(kernel, sigma_const=8.0)
    for case in edge_cases(kernel):
        ro, rd, z, jit = (gpu(x) for x in inputs(kernel, case))
        rgb, t, ts = launch(r, case, ro, rd, z, jit)
        check_depths(kernel, case, r, ro, rd, jit, ts, rk.SUB16.cuda(), sigma_const=8.0)
        check_pixels(kernel, rk.case_id(case) + " sigma=8", case, r, ro, rd, z, rgb, t, ts, sigma_const=8.0)


# ------------------------------------------------------------------------------------------------------- 4: argument rules
def test_render_depths_argument_rules():
    from tgtc_style_amd import hip
    lib = hip.load()
    ERR_ARG, ERR_UNSUPPORTED = -1, -2
    x3, f16, mx = renderer("fp16x3+fp16x3"), renderer("fp16+fp16"), renderer("fp16x3+fp16mx")
    ro, rd = (gpu(x) for x in rk.rays(8))
    ts = torch.full((8 + CANARY_ROWS, 256), CANARY, device="cuda")

    def call(handle, nc, nf, R=8, o=ro, d=rd, out=ts):
        return lib.tgtc_render_depths(handle, hip.ptr(o), hip.ptr(d), R, nc, nf, 0.0, 1.0, None, hip.ptr(out), hip.stream())

    h3, h16 = x3.coarse.packed().handle, f16.coarse.packed().handle
    for nc, nf in ((208, 48), (100, 28), (16, 0), (0, 16), (192, 80)):
        assert call(h3, nc, nf) == ERR_UNSUPPORTED and call(h16, nc, nf) == ERR_UNSUPPORTED, (nc, nf)
    assert call(h16, 16, 8) == ERR_UNSUPPORTED and call(h16, 16, 16) == ERR_UNSUPPORTED and call(h16, 48, 16) == ERR_UNSUPPORTED
    assert call(mx.fine.packed().handle, 64, 64) == ERR_UNSUPPORTED           # an fp16mx handle: no depths-only kernel
    assert call(x3.style.packed().handle if x3.style else renderer("styled").style.packed().handle, 64, 64) == ERR_ARG
    assert call(None, 64, 64) == ERR_ARG and call(h3, 64, 64, R=-1) == ERR_ARG
    assert call(h3, 64, 64, o=None) == ERR_ARG and call(h3, 64, 64, d=None) == ERR_ARG and call(h3, 64, 64, out=None) == ERR_ARG
    assert call(h3, 64, 64, R=0) == 0 and call(h3, 64, 64, R=0, o=None, d=None, out=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(ts, torch.full_like(ts, CANARY))                      # none of the calls above launched anything
    with pytest.raises(ValueError):
        x3.ray_kernel_depths(ro, rd, 100, 28)
    assert call(h3, 16, 16) == 0 and call(h16, 32, 32) == 0
    torch.cuda.synchronize()
