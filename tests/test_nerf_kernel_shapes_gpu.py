"""Shape and edge sweep of the plain NeRF per-sample kernels against the oracle evaluated in float64: nerf_mlp_kernel<CfgExact>
(A, fp16x3), nerf_x3s_kernel (B, fp16x3 densities over rays), nerf_mlp_kernel<CfgFast> (C, fp16), nerf_mx_kernel (D, fp16mx
with base_remap) and nerf_mx2_kernel (E, fp16mx without; rays; the list) -- the kernels of the benchmark's default render.

`test_hip_nerf.py` holds them to one max-norm figure per tensor on uniform weights, points in the unit box and a fresh
direction per sample.  This file sweeps what that leaves out (tests/nerf_kernel_cases.py has the lists): M around the 16- and
32-sample waves and the 128- and 256-sample workgroups; rays whose N is no multiple of 16; a launch in which every persistent
workgroup of B and E takes a second pass and some a third; directions chosen for the two-tile front end's shortcut
(csrc/mlp_nerf_front.h nerf_encode: tile 1 reuses tile 0's direction encoding when all 16 lanes agree); heavy-tailed and dead
weights per sample (the r1 == 0 / r2 == 0 branches of EqualisedNet::run on the NeRF layout, an all-zero weight row and an
all-zero fp6 activation block); points far outside the unit box, zeros and tiny values; encodings that are no encodings; the
rows behind every output; the encodings the kernels write; bit properties; non-finite samples; the argument rules.

Reference: oracle.fields.style_nerf / nerf_mlp with weights and inputs in float64.  Error: max|a - ref| / max|ref| per tensor.
Bars (nerf_kernel_cases.py, "bars"): fp16x3 err <= min(5e-5, 16 y), y = max(rel(float32 oracle, float64 oracle), 1.2e-7) per
case and tensor; fp16mx err <= 1e-3 (except point family `wide`) and, on base and dead weights, err <= 4 y_mx wherever
4 y_mx <= 1e-3, y_mx the error of the arithmetic model of the mode on the CPU; fp16 err <= 1e-2 at `unit`, `special` and the
encoded families.  Every figure is printed.  DESIGN.md section 4, "The plain per-sample sweep", has the measured table."""
import numpy as np
import pytest
import torch

import nerf_kernel_cases as nk
import test_hip_style_shapes as S
from test_plain_cull_gpu import make_list
from test_trunk_mx_cpu import exact_rays

pytestmark = pytest.mark.gpu
ARG, UNSUPPORTED = -1, -2       # TGTC_ERR_ARG, TGTC_ERR_UNSUPPORTED (include/tgtc_hip.h)


# ------------------------------------------------------------------------------------------------------- launches
_NETS = {}


def net(p, wf="base"):
    """The fine NeRF of a weight family in one precision on the GPU, constructed once."""
    if (p, wf) not in _NETS:
        from tgtc_style_amd import models
        m = models.StyleNerf(type("A", (S.Args,), {"precision": p}), mode="fine")
        m.load_state_dict(S.T(nk.states(wf)))
        _NETS[p, wf] = m.cuda()
    return _NETS[p, wf]


def handle(p, wf="base"):
    return net(p, wf).packed().handle


def gpu(*tensors):
    return tuple(t.cuda().contiguous() for t in tensors)


def _outputs(M, want, widths):
    return {k: (S.canary_out(M, *w) if k in want else None) for k, w in widths.items()}


def _finish(out, M, what):
    torch.cuda.synchronize()
    for k, v in out.items():
        if v is not None:
            S.assert_canary(v, M, "%s %s" % (what, k))
    return {k: (None if v is None else v[:M]) for k, v in out.items()}


def forward_pts(p, wf, pts, dirs, want=("rgb", "sigma", "base_remap")):
    """tgtc_nerf_forward on device tensors; `want` names the outputs that are not NULL (also "pts_enc", "dirs_enc").  Every
    call is a canary check: each output carries 64 more rows than the kernel may write."""
    from tgtc_style_amd import hip
    M = pts.shape[0]
    o = _outputs(M, want, {"rgb": (3,), "sigma": (), "base_remap": (256,), "pts_enc": (63,), "dirs_enc": (27,)})
    hip.check(hip.load().tgtc_nerf_forward(handle(p, wf), hip.ptr(pts), hip.ptr(dirs), M, hip.ptr(o["rgb"]), hip.ptr(o["sigma"]),
                                           hip.ptr(o["base_remap"]), hip.ptr(o["pts_enc"]), hip.ptr(o["dirs_enc"]), hip.stream()))
    return _finish(o, M, "nerf_forward %s M=%d" % (p, M))


def forward_enc(p, wf, pe, de, want=("rgb", "sigma", "base_remap")):
    from tgtc_style_amd import hip
    M = pe.shape[0]
    o = _outputs(M, want, {"rgb": (3,), "sigma": (), "base_remap": (256,)})
    hip.check(hip.load().tgtc_nerf_mlp_forward(handle(p, wf), hip.ptr(pe), hip.ptr(de), M, hip.ptr(o["rgb"]), hip.ptr(o["sigma"]),
                                               hip.ptr(o["base_remap"]), hip.stream()))
    return _finish(o, M, "nerf_mlp_forward %s M=%d" % (p, M))


def forward_rays(p, wf, ro, rd, ts, want=("rgb", "sigma")):
    from tgtc_style_amd import hip
    R, N = ts.shape
    o = _outputs(R * N, want, {"rgb": (3,), "sigma": ()})
    hip.check(hip.load().tgtc_nerf_forward_rays(handle(p, wf), hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, N, hip.ptr(o["rgb"]),
                                                hip.ptr(o["sigma"]), hip.stream()))
    return _finish(o, R * N, "nerf_forward_rays %s (%d,%d)" % (p, R, N))


def kernel_of(p, entry, remap=True, rgb=True):
    if p == "fp16":
        return "C"
    if p == "fp16x3":
        return "B" if entry == "rays" and not rgb else "A"
    return "D" if entry != "rays" and remap else "E"


# ------------------------------------------------------------------------------------------------------- bars
def check(p, kernel, name, tensor, got, ref, y, ymx, wf="base", pf="unit"):
    """One figure against its bars (module docstring); prints the line of the table.  -> err"""
    e = S.rel(got, ref)
    if p == "fp16x3":
        yard, bar = y, min(nk.TIGHT[p], nk.K_X3 * y)
    elif p == "fp16mx":
        yard = ymx
        bars = ([] if pf == "wide" else [nk.TOL_MX]) + ([] if nk.mx_guard(wf, ymx) is None else [nk.mx_guard(wf, ymx)])
        bar = min(bars) if bars else None
    else:
        yard, bar = y, (nk.TIGHT[p] if pf in ("unit", "special") else None)
    print("%-6s %s %-10s %-30s err %.3e  y %.3e  err/y %8.2f  bar %s" % (p, kernel, tensor, name, e, yard, e / yard,
                                                                         "%.3e" % bar if bar is not None else "(printed)"))
    if bar is not None:
        assert e <= bar, (p, kernel, tensor, name, e, yard, bar)
    return e


def check_all(p, kernel, name, out, refs, ys, ymxs, wf="base", pf="unit", tensors=nk.TENSORS):
    return {t: check(p, kernel, name, t, out[t], refs[nk.TENSORS.index(t)], ys[nk.TENSORS.index(t)], ymxs[nk.TENSORS.index(t)], wf, pf)
            for t in tensors if out.get(t) is not None}


def assert_mx_beats_fp16(n_samples, errs, name):
    """err(fp16mx) < err(fp16) on the same case for 128 samples and more, as tests/test_restyle_mx_gpu.py asserts."""
    if n_samples >= 128:
        for t, e in errs["fp16mx"].items():
            assert e < errs["fp16"][t], (name, t, e, errs["fp16"][t])


def check_encodings(p, kernel, name, x, enc, n_freqs, asserted):
    """Raw columns: float32(x) exactly.  sin / cos columns: within 3e-7 absolute of the float64 encoding."""
    ref = nk.encodings64(x.cpu(), n_freqs)
    e = float((enc.double().cpu()[:, 3:] - ref[:, 3:]).abs().max())
    print("%-6s %s %-10s %-30s abs err %.3e  bar %s" % (p, kernel, "enc%d" % enc.shape[1], name, e, "%.1e" % nk.ENC_ABS if asserted else "(printed)"))
    assert torch.equal(enc[:, :3].cpu(), x.cpu().float()), (p, kernel, name, "raw columns")
    assert bool(torch.isfinite(enc).all())
    if asserted:
        assert e <= nk.ENC_ABS, (p, kernel, name, e)


# ------------------------------------------------------------------------------------------------------- 1: sample counts
@pytest.mark.parametrize("M", nk.M_LIST)
def test_sample_counts(M):
    """Every M x three precisions through StyleNerf.forward (the module path of test_hip_nerf.py) and through
    tgtc_nerf_mlp_forward: sigma, rgb and base_remap against float64."""
    case, ecase = (M, "unit", "each", "base"), (M, "true", "each", "base")
    pts, dirs = nk.pts_inputs(case)
    pe, de = nk.enc_inputs(ecase)
    (refs, ys), ymx = nk.pts_case_oracle(case), nk.pts_case_y_mx(case)
    (erefs, eys), eymx = nk.enc_case_oracle(ecase), nk.enc_case_y_mx(ecase)
    errs, eerrs = {}, {}
    for p in nk.PRECISIONS:
        out = net(p)(pts=pts.cuda(), dirs=dirs.cuda())
        assert out["sigma"].shape == (M,) and out["rgb"].shape == (M, 3) and out["base_remap"].shape == (M, 256)
        errs[p] = check_all(p, kernel_of(p, "pts"), "module M=%d" % M, out, refs, ys, ymx)
        eerrs[p] = check_all(p, kernel_of(p, "enc"), "mlp_forward M=%d" % M, forward_enc(p, "base", *gpu(pe, de)), erefs, eys, eymx)
    assert_mx_beats_fp16(M, errs, "module M=%d" % M)
    assert_mx_beats_fp16(M, eerrs, "mlp_forward M=%d" % M)


def test_one_sample_as_drawn():
    """The M = 1 case above is the candidate of 16 with the largest float64 |sigma| (nk._dense_sample: a lone sample near
    sigma = 0 has no max|ref| to be read against).  The draw as it comes is launched here through the module, D, E and
    tgtc_nerf_mlp_forward in every precision: its figures are printed, its outputs are finite, the 64 rows behind stay."""
    from oracle import fields
    pts, dirs = nk.points("unit", 1, raw=True), nk.directions("each", 1)
    assert not torch.equal(pts, nk.points("unit", 1))
    refs, _ = nk.pts_oracle(("pts", "one sample as drawn"), "base", pts, dirs)
    pe, de = fields.posenc(pts, 10).float().contiguous(), fields.posenc(dirs, 4).float().contiguous()
    print("one sample as drawn: float64 sigma %.3f" % float(refs[0]))
    for p in nk.PRECISIONS:
        runs = {"module": net(p)(pts=pts.cuda(), dirs=dirs.cuda()), "nerf_forward": forward_pts(p, "base", *gpu(pts, dirs)),
                "nerf_forward, no remap": forward_pts(p, "base", *gpu(pts, dirs), ("rgb", "sigma")),
                "mlp_forward": forward_enc(p, "base", *gpu(pe, de)),
                "mlp_forward, no remap": forward_enc(p, "base", *gpu(pe, de), ("rgb", "sigma"))}
        for how, out in runs.items():
            for t, ref in zip(nk.TENSORS, refs):
                if out.get(t) is not None:
                    assert out[t].shape == ref.shape and bool(torch.isfinite(out[t]).all()), (p, how, t)
                    print("%-6s %-10s %-24s err %.3e  (printed)" % (p, t, how, S.rel(out[t], ref)))


# ------------------------------------------------------------------------------------------------------- 2: families
@pytest.mark.parametrize("case", nk.FAMILY_PTS_CASES, ids=nk.pts_id)
def test_point_families(case):
    """tgtc_nerf_forward at M = 257 in every point, direction and weight family: with base_remap and the encodings requested (A,
    C, D) and without base_remap (A, C, E: the two-tile front end, whose direction shortcut is live when dirs_enc is NULL)."""
    M, pf, dp, wf = case
    pts, dirs = gpu(*nk.pts_inputs(case))
    (refs, ys), ymx = nk.pts_case_oracle(case), nk.pts_case_y_mx(case)
    name, errs = nk.pts_id(case), {}
    for p in nk.PRECISIONS:
        full = forward_pts(p, wf, pts, dirs, ("rgb", "sigma", "base_remap", "pts_enc", "dirs_enc"))
        errs[p] = check_all(p, kernel_of(p, "pts"), name, full, refs, ys, ymx, wf, pf)
        lean = forward_pts(p, wf, pts, dirs, ("rgb", "sigma"))
        check_all(p, kernel_of(p, "pts", remap=False), name, lean, refs, ys, ymx, wf, pf)
        enc_asserted = p != "fp16" or pf == "unit"
        check_encodings(p, kernel_of(p, "pts"), name, pts, full["pts_enc"], 10, enc_asserted)
        check_encodings(p, kernel_of(p, "pts"), name, dirs, full["dirs_enc"], 4, enc_asserted)
    assert_mx_beats_fp16(M, errs, name)


@pytest.mark.parametrize("case", nk.FAMILY_ENC_CASES, ids=nk.pts_id)
def test_encoded_families(case):
    """tgtc_nerf_mlp_forward at M = 257: true encodings in every direction and weight family, and 90 free columns."""
    M, ef, dp, wf = case
    pe, de = gpu(*nk.enc_inputs(case))
    (refs, ys), ymx = nk.enc_case_oracle(case), nk.enc_case_y_mx(case)
    name, errs = nk.pts_id(case), {}
    for p in nk.PRECISIONS:
        errs[p] = check_all(p, kernel_of(p, "enc"), name, forward_enc(p, wf, pe, de), refs, ys, ymx, wf)
        check_all(p, kernel_of(p, "enc", remap=False), name, forward_enc(p, wf, pe, de, ("rgb", "sigma")), refs, ys, ymx, wf)
    assert_mx_beats_fp16(M, errs, name)


@pytest.mark.parametrize("pf", nk.POINT_FAMILIES)
@pytest.mark.parametrize("M", nk.ENC_M)
def test_encodings_written_by_the_kernels(M, pf):
    """pts_enc / dirs_enc of tgtc_nerf_forward from A, C, D and E (E: no base_remap).  The range reduction is float64, so the
    accuracy of fp16x3 and fp16mx does not depend on |x|; fp16 (v_sin / v_cos on a float32 fraction) is held at `unit`."""
    case = (M, pf, "each", "base")
    pts, dirs = gpu(*nk.pts_inputs(case))
    for p in nk.PRECISIONS:
        for remap in ((True, False) if p == "fp16mx" else (True,)):
            want = ("rgb", "sigma", "pts_enc", "dirs_enc") + (("base_remap",) if remap else ())
            out = forward_pts(p, "base", pts, dirs, want)
            k = kernel_of(p, "pts", remap=remap)
            check_encodings(p, k, nk.pts_id(case), pts, out["pts_enc"], 10, p != "fp16" or pf == "unit")
            check_encodings(p, k, nk.pts_id(case), dirs, out["dirs_enc"], 4, p != "fp16" or pf == "unit")


# ------------------------------------------------------------------------------------------------------- 3: ray shapes
@pytest.mark.parametrize("case", nk.RAY_CASES, ids=nk.ray_id)
def test_ray_shapes(case):
    """tgtc_nerf_forward_rays full (A, C, E) and sigma-only (B, C, E) against float64; the sigma-only densities are the full
    launch's bit for bit (the culled renders rely on it)."""
    R, N, rdk, wf = case
    ro, rd, ts = gpu(*nk.ray_inputs(R, N, rdk))
    (refs, ys), ymx = nk.ray_case_oracle(case), nk.ray_case_y_mx(case)
    name, errs = nk.ray_id(case), {}
    for p in nk.PRECISIONS:
        full = forward_rays(p, wf, ro, rd, ts)
        errs[p] = check_all(p, kernel_of(p, "rays"), name, full, refs, ys, ymx, wf)
        lean = forward_rays(p, wf, ro, rd, ts, ("sigma",))
        check_all(p, kernel_of(p, "rays", rgb=False), name + " sigma-only", lean, refs, ys, ymx, wf)
        assert torch.equal(lean["sigma"], full["sigma"]), (p, name, float((lean["sigma"] - full["sigma"]).abs().max()))
    assert_mx_beats_fp16(R * N, errs, name)


# ------------------------------------------------------------------------------------------------------- 4: one tile = two tiles
@pytest.mark.parametrize("case", nk.PTS_CASES, ids=nk.pts_id)
def test_fp16mx_one_tile_kernel_equals_the_two_tile_kernel_on_points(case):
    """rgb and sigma of tgtc_nerf_forward with base_remap (D) and without (E): the same bits."""
    pts, dirs = gpu(*nk.pts_inputs(case))
    d, e = forward_pts("fp16mx", case[3], pts, dirs), forward_pts("fp16mx", case[3], pts, dirs, ("rgb", "sigma"))
    assert torch.equal(d["rgb"], e["rgb"]), float((d["rgb"] - e["rgb"]).abs().max())
    assert torch.equal(d["sigma"], e["sigma"]), float((d["sigma"] - e["sigma"]).abs().max())


@pytest.mark.parametrize("case", nk.ENC_CASES, ids=nk.pts_id)
def test_fp16mx_one_tile_kernel_equals_the_two_tile_kernel_on_encodings(case):
    pe, de = gpu(*nk.enc_inputs(case))
    d, e = forward_enc("fp16mx", case[3], pe, de), forward_enc("fp16mx", case[3], pe, de, ("rgb", "sigma"))
    assert torch.equal(d["rgb"], e["rgb"]), float((d["rgb"] - e["rgb"]).abs().max())
    assert torch.equal(d["sigma"], e["sigma"]), float((d["sigma"] - e["sigma"]).abs().max())


@pytest.mark.parametrize("R,N", nk.RAY_SHAPES)
def test_fp16mx_rays_equal_the_one_tile_kernel_on_their_points(R, N):
    """On rays whose o + t d is exact in float64 (exact_rays), the rays instance of E gives the bits of D on the same points:
    the 2e-4 of test_hip_nerf.py's comparison at N = 192 is the rounding of o + t d, not of the network."""
    ro, rd, ts = exact_rays(R, N)
    pts, dirs = nk.ray_points(ro, rd, ts)
    e = forward_rays("fp16mx", "base", *gpu(ro, rd, ts))
    d = forward_pts("fp16mx", "base", *gpu(pts, dirs))
    assert torch.equal(e["rgb"], d["rgb"]), float((e["rgb"] - d["rgb"]).abs().max())
    assert torch.equal(e["sigma"], d["sigma"]), float((e["sigma"] - d["sigma"]).abs().max())


# ------------------------------------------------------------------------------------------------------- 5: the list instance
@pytest.mark.parametrize("kind", nk.LIST_KINDS)
@pytest.mark.parametrize("R,N", nk.LIST_SHAPES)
def test_list_instance_at_other_ray_lengths(R, N, kind):
    """tgtc_nerf_forward_list at N != 192: listed rows carry the dense rays launch's bits, every other row and the 64 rows
    behind keep the canary."""
    from tgtc_style_amd import hip
    ro, rd, ts = gpu(*nk.ray_inputs(R, N))
    dense = forward_rays("fp16mx", "base", ro, rd, ts)["rgb"]
    M = R * N
    live = make_list(kind, M)
    count = live.numel()
    assert 0 < count <= M
    n_live = torch.tensor([count], dtype=torch.int32, device="cuda")
    out = S.canary_out(M, 3)
    hip.check(hip.load().tgtc_nerf_forward_list(handle("fp16mx"), hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), R, N, hip.ptr(live),
                                                hip.ptr(n_live), hip.ptr(out), hip.stream()))
    torch.cuda.synchronize()
    listed = torch.zeros(M + S.CANARY_ROWS, dtype=torch.bool, device="cuda")
    listed[live.long()] = True
    assert torch.equal(out[:M][listed[:M]], dense[listed[:M]])
    assert bool((out[~listed] == S.CANARY).all()), "wrote a row that is not listed"


# ------------------------------------------------------------------------------------------------------- 6: revisits
def test_persistent_kernels_second_and_third_pass():
    """2.2 passes of 128 samples per CU over rays of 100 samples: every workgroup of B and E takes a second pass, some a third,
    the tail is ragged.  Against float64 on all samples, and bit for bit against the same rays in chunks of 32 (25 passes: no
    workgroup loops)."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    R, N = nk.revisit_rays(n_cu), nk.REVISIT_N
    passes = (R * N + 127) // 128
    assert 2 * n_cu < passes < 3 * n_cu and (R * N) % 128 and (32 * N + 127) // 128 <= n_cu
    ro, rd, ts = nk.ray_inputs(R, N, seed=74000 + n_cu)
    pts, dirs = nk.ray_points(ro, rd, ts)
    refs, ys = nk.pts_oracle(("revisit", n_cu), "base", pts, dirs)
    ymx = nk.y_mx(("revisit", n_cu), "base", nk.encodings64(pts[:nk.MX_SAMPLES], 10), nk.encodings64(dirs[:nk.MX_SAMPLES], 4))
    d = gpu(ro, rd, ts)
    name = "(%d,%d) %d passes on %d CUs" % (R, N, passes, n_cu)
    for p, want in (("fp16x3", ("sigma",)), ("fp16mx", ("rgb", "sigma")), ("fp16mx", ("sigma",))):
        out = forward_rays(p, "base", *d, want)
        check_all(p, kernel_of(p, "rays", rgb="rgb" in want), name, out, refs, ys, ymx)
        for r0 in range(0, R, 32):
            part = forward_rays(p, "base", *(t[r0:r0 + 32].contiguous() for t in d), want)
            for k in want:
                a, b = part[k], out[k][r0 * N:(r0 + 32) * N]
                assert torch.equal(a, b), (p, k, "rays %d.." % r0, float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------------- 7: bit properties
def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))


def _clone(out):
    return {k: (None if v is None else v.clone()) for k, v in out.items()}


# (kernel, precision, entry, outputs that select it)
BIT_KERNELS = [("A", "fp16x3", "pts", ("rgb", "sigma", "base_remap")), ("C", "fp16", "pts", ("rgb", "sigma", "base_remap")),
               ("D", "fp16mx", "pts", ("rgb", "sigma", "base_remap")), ("E", "fp16mx", "pts", ("rgb", "sigma")),
               ("A", "fp16x3", "rays", ("rgb", "sigma")), ("B", "fp16x3", "rays", ("sigma",)), ("C", "fp16", "rays", ("rgb", "sigma")),
               ("C", "fp16", "rays", ("sigma",)), ("E", "fp16mx", "rays", ("rgb", "sigma")), ("E", "fp16mx", "rays", ("sigma",))]


@pytest.mark.parametrize("kernel,p,entry,want", BIT_KERNELS, ids=lambda v: v if isinstance(v, str) else "+".join(v))
def test_bit_properties(kernel, p, entry, want):
    """On M = 257 points / (40, 129) rays: a permutation of the samples or rays permutes the outputs; the same call twice, and
    after a call on other inputs, and alternating with a handle of another precision, gives the same bits; an output's bits
    do not depend on which other outputs are NULL (within one kernel: D / E and A / B are pinned to each other in 3 and 4)."""
    other_p = {"fp16x3": "fp16mx", "fp16mx": "fp16", "fp16": "fp16x3"}[p]
    if entry == "pts":
        d = gpu(*nk.pts_inputs((nk.FAMILY_M, "unit", "each", "base")))
        other = gpu(*nk.pts_inputs((129, "mid", "one", "base")))
        n, run = nk.FAMILY_M, forward_pts
    else:
        d = gpu(*nk.ray_inputs(*nk.BITS_SHAPE))
        other = gpu(*nk.ray_inputs(33, 77))
        n, run = nk.BITS_SHAPE[0], forward_rays
    first = _clone(run(p, "base", *d, want))
    perm = torch.from_numpy(np.random.default_rng(7).permutation(n)).cuda()
    assert not torch.equal(perm, torch.arange(n, device="cuda"))
    got = run(p, "base", *(t[perm].contiguous() for t in d), want)
    rows = d[-1].shape[1] if entry == "rays" else 1
    for k in want:
        a = got[k].reshape(n, rows, -1)
        assert torch.equal(a, first[k].reshape(n, rows, -1)[perm]), (kernel, k, "permutation")
    _same(run(p, "base", *d, want), first, "the same call twice")
    run(p, "base", *other, want)
    _same(run(p, "base", *d, want), first, "after a call on other inputs")
    second = _clone(run(other_p, "base", *d, want))
    _same(run(p, "base", *d, want), first, "after a handle of another precision")
    _same(run(other_p, "base", *d, want), second, "the other handle, after this one")
    # NULL outputs that do not switch the kernel: D needs base_remap, E must not have it, B is sigma alone
    for sub in {"A": (("rgb",), ("sigma",), ("rgb", "sigma")), "C": (("rgb",), ("sigma",), ("rgb", "sigma")),
                "D": (("base_remap",), ("rgb", "base_remap"), ("sigma", "base_remap")), "E": (("rgb",), ("sigma",), ("rgb", "sigma")),
                "B": ()}[kernel]:
        if set(sub) <= set(want) and set(sub) != set(want) and (entry == "pts" or "rgb" in sub or "rgb" not in want):
            got = run(p, "base", *d, sub)
            _same(got, {k: first[k] for k in got}, "outputs %s only" % "+".join(sub))


ENC_WANTS = (("pts_enc",), ("dirs_enc",), ("pts_enc", "dirs_enc"))


@pytest.mark.parametrize("dp", nk.DIR_PATTERNS)
@pytest.mark.parametrize("kernel,p,want", [(k, p, w) for k, p, e, w in BIT_KERNELS if e == "pts"], ids=lambda v: v if isinstance(v, str) else "+".join(v))
def test_requested_encodings_change_no_other_output(kernel, p, want, dp):
    """rgb, sigma and base_remap of tgtc_nerf_forward with pts_enc / dirs_enc requested are those of the call without, bit for
    bit, in every direction pattern.  Asking for dirs_enc is what switches the two-tile front end's direction shortcut off
    (nerf_encode, NCT = 2: kernels C and E), so on `one` and `blocks32`, where the call without takes it in every wave, and on
    `lane` and a ragged last wave, this is the shortcut against the encoder inside one kernel.  The encodings written do not
    depend on which outputs go with them either."""
    d = gpu(*nk.pts_inputs((nk.FAMILY_M, "unit", dp, "base")))
    first = _clone(forward_pts(p, "base", *d, want))
    got = {more: _clone(forward_pts(p, "base", *d, want + more)) for more in ENC_WANTS}
    for more, out in got.items():
        _same({k: out[k] for k in want}, {k: first[k] for k in want}, "%s with %s" % (kernel, "+".join(more)))
        _same({k: out[k] for k in more}, {k: got[ENC_WANTS[2]][k] for k in more}, "%s: %s alone" % (kernel, "+".join(more)))


# ------------------------------------------------------------------------------------------------------- 8: non-finite samples
def _poison_slots(M):
    nan = torch.arange(5, M, 128)
    inf = torch.arange(70, M, 128)
    return nan, inf


@pytest.mark.parametrize("entry", ["pts", "enc", "rays"])
def test_non_finite_samples_stay_in_their_column(entry):
    """One sample per 128 NaN and one +inf (the NDC warp produces them for d_z = 0): every other sample's outputs are bit
    identical to the launch with finite values in those slots.  Nothing is asserted about the poisoned samples.  (No index is
    derived from a sample's value: nerf_load_samples indexes by the sample number only, the encoders by lane and band.)"""
    for p in nk.PRECISIONS:
        if entry == "rays":
            R, N = 3, 200
            ro, rd, ts = gpu(*nk.ray_inputs(R, N))
            M = R * N
            nan, inf = _poison_slots(M)
            bad = ts.clone()
            bad.view(-1)[nan.cuda()] = float("nan")
            bad.view(-1)[inf.cuda()] = float("inf")
            variants = [(forward_rays, (ro, rd, ts), (ro, rd, bad), w) for w in (("rgb", "sigma"), ("sigma",))]
        else:
            M = nk.FAMILY_M
            nan, inf = _poison_slots(M)
            if entry == "pts":
                a, b = gpu(*nk.pts_inputs((M, "unit", "each", "base")))
                run = forward_pts
            else:
                a, b = gpu(*nk.enc_inputs((M, "true", "each", "base")))
                run = forward_enc
            bad_a, bad_b = a.clone(), b.clone()
            bad_a[nan.cuda(), 1] = float("nan")
            bad_b[nan.cuda()[::2], 0] = float("nan")
            bad_a[inf.cuda(), 2] = float("inf")
            variants = [(run, (a, b), (bad_a, bad_b), w) for w in (("rgb", "sigma", "base_remap"), ("rgb", "sigma"))]
        keep = torch.ones(M, dtype=torch.bool, device="cuda")
        keep[nan.cuda()] = False
        keep[inf.cuda()] = False
        assert int((~keep).sum()) == nan.numel() + inf.numel() >= 4
        for run, good, bad, want in variants:
            clean = _clone(run(p, "base", *good, want))
            assert all(bool(torch.isfinite(v).all()) for v in clean.values() if v is not None)
            got = run(p, "base", *bad, want)            # (canaries checked inside; a NaN is not the canary)
            for k, v in got.items():
                if v is not None:
                    assert torch.equal(v[keep], clean[k][keep]), (p, entry, k, want, "a finite sample changed")


# ------------------------------------------------------------------------------------------------------- 9: argument rules
def test_argument_rules_on_real_handles():
    """What the host code checks before any launch (csrc/mlp_nerf.hip, the extern "C" entry points)."""
    from tgtc_style_amd import hip
    lib, st = hip.load(), hip.stream()
    pair = S.networks("fp16x3", "base")[3].packed().handle           # a style handle: kind != 0
    pts, dirs = gpu(*nk.pts_inputs((16, "unit", "each", "base")))
    pe, de = gpu(*nk.enc_inputs((16, "true", "each", "base")))
    ro, rd, ts = gpu(*nk.ray_inputs(2, 8))
    rgb, sigma = S.canary_out(16, 3), S.canary_out(16)
    live, n_live = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda")
    P = hip.ptr
    for p in nk.PRECISIONS:
        h = handle(p)
        assert lib.tgtc_nerf_forward(h, None, None, 0, None, None, None, None, None, st) == 0
        assert lib.tgtc_nerf_mlp_forward(h, None, None, 0, None, None, None, st) == 0
        assert lib.tgtc_nerf_forward_rays(h, None, None, None, 0, 8, None, None, st) == 0
        assert lib.tgtc_nerf_forward(h, None, P(dirs), 16, P(rgb), P(sigma), None, None, None, st) == ARG
        assert lib.tgtc_nerf_forward(h, P(pts), None, 16, P(rgb), P(sigma), None, None, None, st) == ARG
        assert lib.tgtc_nerf_forward(h, P(pts), P(dirs), -1, P(rgb), P(sigma), None, None, None, st) == ARG
        assert lib.tgtc_nerf_mlp_forward(h, None, P(de), 16, P(rgb), P(sigma), None, st) == ARG
        assert lib.tgtc_nerf_mlp_forward(h, P(pe), None, 16, P(rgb), P(sigma), None, st) == ARG
        assert lib.tgtc_nerf_mlp_forward(h, P(pe), P(de), -1, P(rgb), P(sigma), None, st) == ARG
        assert lib.tgtc_nerf_forward_rays(h, None, P(rd), P(ts), 2, 8, P(rgb), P(sigma), st) == ARG
        assert lib.tgtc_nerf_forward_rays(h, P(ro), P(rd), None, 2, 8, P(rgb), P(sigma), st) == ARG
        assert lib.tgtc_nerf_forward_rays(h, P(ro), P(rd), P(ts), -1, 8, P(rgb), P(sigma), st) == ARG
        assert lib.tgtc_nerf_forward_rays(h, P(ro), P(rd), P(ts), 2, 0, P(rgb), P(sigma), st) == ARG
        assert lib.tgtc_nerf_forward_rays(h, P(ro), P(rd), P(ts), 2, 8, None, None, st) == ARG       # both outputs NULL
        assert lib.tgtc_nerf_forward_list(h, P(ro), P(rd), P(ts), 0, 8, None, None, None, st) == 0
        assert lib.tgtc_nerf_forward_list(h, P(ro), P(rd), P(ts), 2, 0, P(live), P(n_live), P(rgb), st) == ARG
        assert lib.tgtc_nerf_forward_list(h, P(ro), P(rd), P(ts), 2, 8, None, P(n_live), P(rgb), st) == ARG
        assert lib.tgtc_nerf_forward_list(h, P(ro), P(rd), P(ts), 2, 8, P(live), P(n_live), P(rgb), st) == (0 if p == "fp16mx" else UNSUPPORTED)
    assert lib.tgtc_nerf_forward(pair, P(pts), P(dirs), 16, P(rgb), P(sigma), None, None, None, st) == ARG
    assert lib.tgtc_nerf_mlp_forward(pair, P(pe), P(de), 16, P(rgb), P(sigma), None, st) == ARG
    assert lib.tgtc_nerf_forward_rays(pair, P(ro), P(rd), P(ts), 2, 8, P(rgb), P(sigma), st) == ARG
    assert lib.tgtc_nerf_forward_list(pair, P(ro), P(rd), P(ts), 2, 8, P(live), P(n_live), P(rgb), st) == ARG
    assert lib.tgtc_nerf_forward(None, P(pts), P(dirs), 16, P(rgb), P(sigma), None, None, None, st) == ARG
    torch.cuda.synchronize()
    # nothing but the one valid list launch (sample 0 of 16) wrote anything
    assert bool((sigma == S.CANARY).all()) and bool((rgb[1:] == S.CANARY).all()) and bool((rgb[0] != S.CANARY).all())
