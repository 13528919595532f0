"""CPU: what the ray-kernel shape sweep (tests/test_ray_kernel_shapes_gpu.py) rests on, from the library's host code and the
oracle alone.

  * The case lists of tests/ray_kernel_cases.py resolve to the ray kernels and reach every edge of their per-ray code.
  * The GPU tests compare a ray kernel's pixel with the float64 oracle evaluated AT THE KERNEL'S OWN merged depths, within
    K x y, y = the float32-vs-float64 distance of that conditional oracle.  That is a sound yardstick only where (a) the
    conditional oracle is well conditioned -- y stays at float32 rounding, 1e-5, on every ray of every case -- and (b) the
    sampler-bound check they apply to the kernel's depths (conditioning.sampler_bound) accepts the float32 oracle's own
    depths on its own weights, i.e. is exact on correct input.  Both are asserted here for every case, plain and stylised.
    If a ray breaks one, choose other rays in ray_kernel_cases.rays, not a wider bar."""
import pytest
import torch

import conditioning
import ray_kernel_cases as rk

ALL = [(step, case) for step in (16, 32) for case in rk.CASES[step]]
IDS = ["step%d-%s" % (step, rk.case_id(case)) for step, case in ALL]
Y_MAX = 1e-5        # float32 rounding of a 256-sample compositing sum of O(1) terms; (a) above


def test_case_lists_cover_the_ray_kernel_edges():
    """If kFusedMaxCoarse / kFusedMaxTotal (csrc/render_args.h) or the step of ray_kernel_built (csrc/render.hip) change,
    update MAX_COARSE / MAX_TOTAL / STEP and the shape lists of tests/ray_kernel_cases.py with them."""
    from tgtc_style_amd import hip
    lib = hip.load()
    RAY, X3, F16, MX = hip.PATH_RAY_KERNEL, hip.PREC_FP16X3, hip.PREC_FP16, hip.PREC_FP16_FP6
    kernels = {16: [(X3, X3, -1), (X3, MX, -1), (X3, X3, X3)], 32: [(F16, F16, -1)]}
    for step, shapes in ((16, rk.SHAPES_16), (32, rk.SHAPES_32)):
        assert {(nc, nf) for nc, nf, *_ in rk.CASES[step]} == set(shapes)
        for nc, nf in shapes:
            for pc, pf, ps in kernels[step]:
                assert lib.tgtc_render_path(RAY, pc, pf, ps, nc, nf, 0) == RAY, (pc, pf, ps, nc, nf)
        # the limits the lists were written for are the library's: one step beyond either is refused
        pc, pf, ps = kernels[step][0]
        assert rk.MAX_COARSE % step == 0 and rk.MAX_TOTAL % step == 0
        assert lib.tgtc_render_path(RAY, pc, pf, ps, rk.MAX_COARSE, rk.MAX_TOTAL - rk.MAX_COARSE, 0) == RAY
        assert lib.tgtc_render_path(RAY, pc, pf, ps, rk.MAX_COARSE + step, step, 0) == -2
        assert lib.tgtc_render_path(RAY, pc, pf, ps, rk.MAX_COARSE, rk.MAX_TOTAL - rk.MAX_COARSE + step, 0) == -2
        assert lib.tgtc_render_path(RAY, pc, pf, ps, step, step, 0) == RAY
        assert lib.tgtc_render_path(RAY, pc, pf, ps, step + step // 2, step + step // 2, 0) == -2        # the step itself
        assert rk.STEP["fp16x3" if step == 16 else "fp16"] == step
        assert {rk.pdf_per_lane(nc) for nc, _ in shapes} == {1, 2, 3}                   # the blocked cdf scan
        assert any(nc - 2 < 64 for nc, _ in shapes)                                     # most lanes own no pdf entry
        assert any(nf > 192 for _, nf in shapes) and any(64 < nf <= 192 for _, nf in shapes)   # the 64-lane stride over n_fine
        totals = {nc + nf for nc, nf in shapes}
        assert {64, rk.MAX_TOTAL} <= totals and totals & {208, 224}                     # rank slots: one, a part of the fourth, all
        assert (rk.MAX_COARSE, rk.MAX_TOTAL - rk.MAX_COARSE) in shapes                  # both strips full
        assert rk.SMALL[step] == min(shapes) and rk.FULL in shapes
        assert set(rk.JITTERED[step]) <= set(shapes) and any(rk.pdf_per_lane(nc) == 2 for nc, _ in rk.JITTERED[step])
        assert rk.SMALL[step] in rk.JITTERED[step] and rk.FULL in rk.JITTERED[step]
        assert any((near, far) != (0.0, 1.0) for *_, near, far in rk.CASES[step])
    assert rk.R == 41 and rk.R % 8 == 1 and len(set(rk.SUB16.tolist())) == 16


_own = {}


def own_render(kind, step, case):
    """The float32 oracle's own render of a case (cached; never modified): its dict plus the coarse depths."""
    key = (kind, case)
    if key not in _own:
        from oracle import raymarch
        nc, nf, jit, near, far = case
        ro, rd = rk.rays()
        j = rk.jitter(rk.R, nc) if jit else None
        out = rk.oracle_render(kind, case, ro, rd, rk.latents(), torch.float32, jit=j)
        out["ts_coarse"] = raymarch.sample_coarse(ro, rd, nc, near, far, j)[1]
        _own[key] = out
    return _own[key]


@pytest.mark.parametrize("step,case", ALL, ids=IDS)
@pytest.mark.parametrize("kind", ["plain", "styled"])
def test_conditional_oracle_is_well_conditioned(kind, step, case):
    """(a): at the float32 oracle's own merged depths the float32 and float64 oracles' fine pass + compositing agree within
    1e-5 on every ray."""
    ro, rd = rk.rays()
    ts = own_render(kind, step, case)["ts_fine"]
    assert ts.dtype == torch.float32 and ts.shape == (rk.R, case[0] + case[1])
    _, (y_rgb, y_t) = rk.conditional(kind, case, ro, rd, ts, rk.latents())
    print("%s %s: y rgb %.3e  y t %.3e" % (kind, rk.case_id(case), y_rgb, y_t))
    assert y_rgb <= Y_MAX and y_t <= Y_MAX, (kind, case, y_rgb, y_t)


@pytest.mark.parametrize("step,case", ALL, ids=IDS)
def test_sampler_bound_accepts_the_oracles_own_depths(step, case):
    """(b): conditioning.sampler_bound of the float32 oracle's depths on its own coarse weights is 0 on the 16 rays the GPU
    tests apply it to.  The stylised oracle's coarse weights depend on sigma alone: its depths are the plain oracle's bits,
    so one check serves both."""
    plain, styled = own_render("plain", step, case), own_render("styled", step, case)
    assert torch.equal(plain["ts_fine"], styled["ts_fine"]) and torch.equal(plain["w_coarse"], styled["w_coarse"])
    s = rk.SUB16
    excess = conditioning.sampler_bound(plain["ts_coarse"][s], plain["w_coarse"][s], plain["ts_fine"][s], case[1])
    assert float(excess.max()) == 0.0, (case, excess.tolist())
