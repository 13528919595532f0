"""GPU: tgtc_coarse_to_fine (csrc/raypath.hip, coarse_to_fine_kernel) against the pair it replaces between the passes of a
render: tgtc_composite (zero colours, weights out) followed by tgtc_sample_fine.  Every comparison is of BITS.

R = 9: the kernel takes four rays per workgroup, so two full workgroups and a tail of one ray.
Shapes (N, n_fine): (3, 1) the smallest, one new sample at u = 0; (3, 2); (16, 16); (64, 64) and (66, 64), the last N with one
pdf entry per lane of the cdf scan; (67, 5), the first with two; (128, 64) the frame's; (130, 3) the last with two; (195, 7)
the first with four; (256, 1); (256, 256) both limits (N = 256, N + n_fine = 512).

Every output plane is pre-filled with CANARY, a NaN bit pattern, and compared by bits: a slot that no lane wrote fails the
`isfinite` assertions on the pair's outputs.

Which path a ray takes is reported by tgtc_coarse_to_fine_traced and asserted for every case: MERGE_DEPTHS are the depth
rows whose rays must all take the merge; in "descending" ray DESC_ROW -- its coarse depths descend -- must take the counting
sort and the eight others the merge.  That row keeps the random densities under every density plane: its deltas are
negative, a saturated density there gives infinite weights and NaN depths, whose order neither kernel defines."""
import numpy as np
import pytest
import torch

from sampler_cases import DESC_ROW, R, depth_rows      # R = 9, DESC_ROW = 4

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1), (3, 2), (16, 16), (64, 64), (66, 64), (67, 5), (128, 64), (130, 3), (195, 7), (256, 1), (256, 256)]
SIGMAS = ["random", "dead", "saturated", "constant"]
MERGE_DEPTHS = ["linspace", "jittered", "ties"]
DEPTHS = MERGE_DEPTHS + ["descending"]
CANARY = 0x7FC0BEEF          # a quiet NaN, as int32


def sigma_plane(kind, N, rng):
    rand = (rng.standard_normal((R, N)) * 3.0).astype(np.float32)     # about half negative
    if kind == "random":
        s = rand.copy()
    elif kind == "dead":                                              # all <= 0: uniform pdf, den below 1e-5 -> 1
        s = -np.abs(rand)
        s[:, ::3] = 0.0
        s[:, 1::5] = -0.0
    elif kind == "saturated":                                         # alpha = 1 at one sample per ray, on top of random
        s = rand.copy()
        s[np.arange(R), rng.integers(0, N - 1, R)] = 1e9
    else:
        s = np.full((R, N), 2.0, np.float32)
    return s, rand


def canary_plane(rows, cols):
    return torch.full((rows, cols), CANARY, dtype=torch.int32, device="cuda").view(torch.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


_cases = {}


def case(N, NF, skind, dkind):
    """inputs and the pair's outputs, computed once"""
    key = (N, NF, skind, dkind)
    if key not in _cases:
        from tgtc_style_amd import hip
        lib = hip.load()
        rng = np.random.default_rng(1000 * N + NF + 17 * SIGMAS.index(skind) + 101 * DEPTHS.index(dkind))
        s, rand = sigma_plane(skind, N, rng)
        ts = depth_rows(dkind, N, rng)
        if dkind == "descending":
            s[DESC_ROW] = rand[DESC_ROW]
        sigma, ts = torch.from_numpy(s).cuda(), torch.from_numpy(np.ascontiguousarray(ts)).cuda()
        ro = torch.zeros(R, 3, dtype=torch.float64, device="cuda")
        rd = torch.ones(R, 3, dtype=torch.float64, device="cuda")
        rgb = torch.zeros(R, N, 3, device="cuda")
        rgb_exp, t_exp = torch.empty(R, 3, device="cuda"), torch.empty(R, device="cuda")
        w = canary_plane(R + 1, N)
        out = canary_plane(R + 1, N + NF)
        hip.check(lib.tgtc_composite(hip.ptr(rgb), hip.ptr(sigma), hip.ptr(ts), R, N, hip.ptr(rgb_exp), hip.ptr(t_exp), hip.ptr(w),
                                     hip.stream()))
        hip.check(lib.tgtc_sample_fine(hip.ptr(ro), hip.ptr(rd), hip.ptr(ts), hip.ptr(w), R, N, NF, None, hip.ptr(out),
                                       hip.stream()))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out[:R]).all()) and bool(torch.isfinite(w[:R]).all())
        _cases[key] = (sigma, ts, w, out)
    return _cases[key]


@pytest.mark.parametrize("dkind", DEPTHS)
@pytest.mark.parametrize("skind", SIGMAS)
@pytest.mark.parametrize("N,NF", SHAPES)
def test_bits_of_composite_then_sample_fine(N, NF, skind, dkind):
    from tgtc_style_amd import hip
    lib = hip.load()
    sigma, ts, w_ref, out_ref = case(N, NF, skind, dkind)
    for with_weights in (True, False):
        w = canary_plane(R + 1, N)
        out = canary_plane(R + 1, N + NF)
        took = torch.full((R + 1,), 77, dtype=torch.int32, device="cuda")
        hip.check(lib.tgtc_coarse_to_fine_traced(hip.ptr(sigma), hip.ptr(ts), R, N, NF, hip.ptr(out),
                                                 hip.ptr(w) if with_weights else None, hip.ptr(took), hip.stream()))
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(out_ref))                       # depths, and the canary row behind them
        if with_weights:
            assert torch.equal(bits(w), bits(w_ref))
        else:
            assert bool((bits(w) == CANARY).all())                         # no plane given: nothing written
        want = [0] * R + [77]
        if dkind == "descending":
            want[DESC_ROW] = 1
        assert took.tolist() == want, (N, NF, skind, dkind, took.tolist())
    # the entry point without the trace is the same launch
    out = canary_plane(R + 1, N + NF)
    hip.check(lib.tgtc_coarse_to_fine(hip.ptr(sigma), hip.ptr(ts), R, N, NF, hip.ptr(out), None, hip.stream()))
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(out_ref))


def test_ties_across_the_runs_occur():
    """The "ties" rows put three equal coarse depths in a row: both bins between them are that depth, and under the uniform
    pdf of the "dead" plane a new sample falls between them and equals the coarse depth exactly -- the merged order of such a
    tie (coarse first) is part of the comparison above."""
    _, ts, _, out = case(64, 64, "dead", "ties")
    t = ts[:, 32]
    assert bool(((out[:R] == t[:, None]).sum(1) >= 4).all())              # the triple and at least one new sample


def test_shape_limits_are_refused():
    from tgtc_style_amd import hip
    lib = hip.load()
    x = torch.zeros(R, 600, device="cuda")
    for N, NF in ((2, 4), (257, 1), (256, 257), (16, 0)):
        assert lib.tgtc_coarse_to_fine(hip.ptr(x), hip.ptr(x), R, N, NF, hip.ptr(x), None, hip.stream()) == -2
    assert lib.tgtc_coarse_to_fine(None, hip.ptr(x), R, 16, 16, hip.ptr(x), None, hip.stream()) == -1
    assert lib.tgtc_coarse_to_fine(None, None, 0, 16, 16, None, None, hip.stream()) == 0


# ------------------------------------------------------------------------------------------------ through RayRenderer
def T(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


class Args:
    use_viewdir, act_type = True, "relu"
    embed_freq_coor, embed_freq_dir = 10, 4
    netdepth = netdepth_fine = 8
    netwidth = netwidth_fine = 256
    precision = "fp16x3"


_nets = []


def nets():
    if not _nets:
        from tgtc_style_amd import models, synth
        for (seed, mode), prec in zip(((0, "coarse"), (1, "fine")), ("fp16x3", "fp16mx")):
            m = models.StyleNerf(type("A", (Args,), {"precision": prec}), mode=mode)
            m.load_state_dict(T(synth.nerf_state(seed)))
            _nets.append(m.cuda())
    return _nets


def align256(x):
    return (x + 255) & ~255


@pytest.mark.parametrize("nc,nf", [(16, 16), (128, 64)])
def test_render_equals_the_render_with_the_pair(nc, nf, monkeypatch):
    """41 rays on the chain (the frame's precision pair): rgb and t with the one kernel are the bits of the render that
    keeps compositor + sampler (TGTC_PER_RAY_PAIR=1).  That the switch switches is read off the workspace: on the dense fine
    pass nothing but the compositor writes the coarse weights plane, which therefore keeps its canary with the one kernel.
    The canary is 0xFF: every float the workspace holds before a render is a NaN, also where the culled fine pass leaves its
    colour plane unwritten."""
    from tgtc_style_amd import rendering, synth, utils
    coarse, fine = nets()
    o, d = utils.gen_rays(8, 8, synth.fern_intrinsics(8, 8), synth.spiral_pose(3), first_pixel=5, n=41)
    n = o.shape[0]
    w_c = slice(2 * align256(n * nc * 4) + align256(n * nc * 12), 2 * align256(n * nc * 4) + align256(n * nc * 12) + n * nc * 4)
    outs, touched = {}, {}
    for cull in (False, True):
        for pair in ("0", "1"):
            monkeypatch.setenv("TGTC_PER_RAY_PAIR", pair)
            r = rendering.RayRenderer(coarse, fine, fused=False, cull=cull)
            r._workspace(n, nc, nf, o.device).fill_(0xFF)
            out = r.render(o, d, nc, nf)
            torch.cuda.synchronize()
            outs[cull, pair] = out
            touched[cull, pair] = bool((r._ws[w_c] != 0xFF).any())
    assert touched[False, "1"] and not touched[False, "0"]
    for cull in (False, True):
        assert torch.equal(bits(outs[cull, "0"]["rgb"]), bits(outs[cull, "1"]["rgb"]))
        assert torch.equal(bits(outs[cull, "0"]["t"]), bits(outs[cull, "1"]["t"]))
    assert torch.equal(bits(outs[True, "0"]["rgb"]), bits(outs[False, "1"]["rgb"]))
    assert bool(torch.isfinite(outs[True, "0"]["rgb"]).all())
