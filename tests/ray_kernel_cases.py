"""Test helper: the sample-count cases of the ray-kernel shape sweep (tests/test_ray_kernel_shapes_cpu.py, _gpu.py), the rays,
jitter planes and latents they render, and the oracle evaluated CONDITIONALLY on given merged depths.

The ray kernels (csrc/render_fused.hip, csrc/render_styled_fused.hip) are built for: n_coarse and n_coarse + n_fine multiples
of STEP (16; 32 when the coarse precision is fp16), 16 <= n_coarse <= MAX_COARSE, n_coarse + n_fine <= MAX_TOTAL
(tgtc_render_path).  The per-ray code that depends on the shape is sample_fine_wave / composite_tile (csrc/raymarch_wave.h):
C = ceil((n_coarse - 2) / 64) pdf entries per lane in the blocked cdf scan, a 64-lane stride over n_fine, T = n_coarse + n_fine
depths in four rank slots per lane, and an LDS strip depths[256] | weights[192] | compositing state.  Each case below is the
smallest shape of something in that list ("The ray-kernel shape sweep").

No fixtures and no GPU here: numpy / torch CPU only."""
import numpy as np
import torch

from tgtc_style_amd import synth

MAX_COARSE, MAX_TOTAL = 192, 256          # kFusedMaxCoarse, kFusedMaxTotal (csrc/render_args.h)
STEP = {"fp16x3": 16, "fp16": 32}         # tiles per pass x 16 samples, by coarse precision

# (n_coarse, n_fine): coarse fp16x3 -- plain fp16x3 + fp16x3, plain fp16x3 + fp16mx, stylised
SHAPES_16 = [
    (16, 16),     # one coarse tile; 14 pdf entries on 64 lanes; T = 32
    (16, 240),    # four fine samples per lane; T = 256: all four rank slots, depth strip full
    (48, 16),     # T = 64: exactly one rank slot
    (64, 64),     # C = 1 upper edge (62 entries); the golden shape
    (80, 48),     # C = 2 lower edge (78); T = 128
    (128, 64),    # the baseline
    (144, 112),   # C = 3 lower edge (142); T = 256
    (192, 16),    # n_coarse maximum; T = 208: the fourth rank slot on 16 lanes only
    (192, 64),    # both maxima: depth and weight strips full
]
# coarse fp16 (two tiles per pass): plain fp16 + fp16
SHAPES_32 = [(32, 32), (32, 224), (64, 64), (96, 32), (128, 64), (160, 96), (192, 32), (192, 64)]
# jitter on the smallest, the C = 2 and the full-strip shape of each list; near, far = 0.05, 0.9 on the C = 2 lower edge
JITTERED = {16: [(16, 16), (80, 48), (192, 64)], 32: [(32, 32), (96, 32), (192, 64)]}
NEAR_FAR = {(80, 48): (0.05, 0.9), (96, 32): (0.05, 0.9)}


def _cases(shapes, step):
    out = [(nc, nf, False) + NEAR_FAR.get((nc, nf), (0.0, 1.0)) for nc, nf in shapes]
    return out + [(nc, nf, True) + NEAR_FAR.get((nc, nf), (0.0, 1.0)) for nc, nf in JITTERED[step]]


# a case: (n_coarse, n_fine, jittered, near, far)
CASES = {16: _cases(SHAPES_16, 16), 32: _cases(SHAPES_32, 32)}
SMALL, FULL = {16: (16, 16), 32: (32, 32)}, (192, 64)      # the shapes of the bit-property and edge tests


def case_id(case):
    nc, nf, jit, near, far = case
    return "%d+%d%s%s" % (nc, nf, "-jit" if jit else "", "" if (near, far) == (0.0, 1.0) else "-near%g-far%g" % (near, far))


def pdf_per_lane(nc):
    """C of sample_fine_wave: pdf entries per lane of the blocked cdf scan."""
    return (nc - 2 + 63) // 64


# ------------------------------------------------------------------------------------------------------- inputs
R = 41                  # 5 groups of the 8 rays a workgroup renders per step, and a tail of one
SUB16 = torch.linspace(0, R - 1, 16).round().long()       # the rays of the sampler-bound checks (a Python loop per ray)
FRAME = 400
_cache = {}


def frame_rays():
    """All rays of the 400 x 400 fern-shaped frame at spiral_pose(3), float64 [160000, 3] x 2 (oracle.rays, CPU)."""
    if "frame" not in _cache:
        from oracle import rays
        o, d = rays.frame_rays_ndc(FRAME, FRAME, synth.fern_intrinsics(FRAME, FRAME), synth.spiral_pose(3))
        _cache["frame"] = (torch.from_numpy(np.ascontiguousarray(o)), torch.from_numpy(np.ascontiguousarray(d)))
    return _cache["frame"]


def rays(n=R):
    """n rays spread with linspace over the frame."""
    o, d = frame_rays()
    idx = torch.linspace(0, FRAME * FRAME - 1, n).round().long()
    return o[idx].contiguous(), d[idx].contiguous()


def jitter(n, nc):
    """[n, nc] float32 in [0, 1), one plane per (n, nc)."""
    return torch.from_numpy(np.random.default_rng(7000 + 300 * nc + n).uniform(0, 1, (n, nc)).astype(np.float32))


def latents(n=R):
    """Per-ray latents randn [n, 32] float32."""
    return torch.randn(n, 32, generator=torch.Generator().manual_seed(5))


def T(sd, dtype=torch.float32):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in sd.items()}


def states(dtype=torch.float32, sigma_const=None):
    """(coarse NeRF, fine NeRF, concat MLP, style MLP) state dicts, synth seeds 0 / 1 / 2 / 3.  sigma_const: both NeRF nets
    with a constant density (sigma_layer.weight = 0, bias = the constant), as tests/test_plain_cull_gpu.py builds them."""
    sds = [T(synth.nerf_state(0), dtype), T(synth.nerf_state(1), dtype), T(synth.concat_state(2), dtype),
           T(synth.style_state(3), dtype)]
    if sigma_const is not None:
        for sd in sds[:2]:
            sd["net.sigma_layer.weight"] = torch.zeros_like(sd["net.sigma_layer.weight"])
            sd["net.sigma_layer.bias"] = torch.full_like(sd["net.sigma_layer.bias"], sigma_const)
    return sds


# ------------------------------------------------------------------------------------------------------- oracle
def oracle_render(kind, case, ro, rd, z=None, dtype=torch.float32, ts_fine=None, jit=None, sigma_const=None):
    """oracle.fields.render_plain (kind "plain") / render_styled ("styled") of a case in `dtype` (state dicts in dtype, rays
    float64 as everywhere); ts_fine: the fine network and its compositing at THESE merged depths.  -> the oracle's dict."""
    from oracle import fields
    nc, nf, _, near, far = case
    c, f, cm, sm = states(dtype, sigma_const)
    with torch.no_grad():
        if kind == "plain":
            return fields.render_plain(c, f, ro, rd, nc, nf, near, far, dtype=dtype, ts_fine=ts_fine, jitter=jit)
        return fields.render_styled(c, f, cm, sm, ro, rd, z.to(dtype), nc, nf, near, far, jitter=jit, dtype=dtype, ts_fine=ts_fine)


def pixels(out):
    """oracle dict -> (rgb [R,3], t [R]) float64"""
    return out["rgb_fine"].double(), out["t_fine"].double()


def conditional(kind, case, ro, rd, ts, z=None, sigma_const=None):
    """The float64 oracle's pixels (rgb, t) at the merged depths `ts`, and the yardsticks (y_rgb, y_t) =
    max |float32 oracle - float64 oracle| at those same depths (absolute, not floored)."""
    r64 = pixels(oracle_render(kind, case, ro, rd, z, torch.float64, ts_fine=ts, sigma_const=sigma_const))
    r32 = pixels(oracle_render(kind, case, ro, rd, z, torch.float32, ts_fine=ts, sigma_const=sigma_const))
    return r64, tuple(float((a - b).abs().max()) for a, b in zip(r32, r64))
