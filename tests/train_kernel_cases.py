"""Test helper: the cases of the training-kernel sweep (tests/test_train_kernel_shapes_cpu.py, _gpu.py), their inputs and their
float64 references.  Four kernel families ("The training-kernel sweep"):

A  compositing forward / backward  (csrc/raypath.hip: composite_kernel<C>, composite_backward_kernel<C>, one wavefront per
   ray, C = ceil(N / 64) samples per lane, instances C = 1, 2, 3, 4, 8)
B  the dense layer and its backward  (csrc/style2d.hip: tgtc_s2d_linear[_pre], tgtc_s2d_linear_backward, tgtc_s2d_activation)
C  the latent gather and its backward  (csrc/raypath.hip: latents_kernel, latents_backward_kernel)
D  the fused trainer  (csrc/mlp_train.hip) at the edges of its 128-sample tile and with uneven upstream gradients

No fixtures and no GPU here: numpy / torch CPU only."""
import math

import numpy as np
import torch

from oracle import fields, raymarch


def T(sd, dtype=None):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) if dtype else torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def rows_error(got, ref):
    """[R] float64: max_i |got - ref| of row r divided by max_i |ref| of row r (everything behind the first dimension is the
    row).  A row whose reference is all zero must be exactly zero: its entry is 0 if it is and inf if it is not."""
    R = ref.shape[0]
    g, r = got.double().reshape(R, -1), ref.double().reshape(R, -1)
    num, den = (g - r).abs().amax(1), r.abs().amax(1)
    num = torch.where(torch.isnan(g).any(1), torch.full_like(num, float("inf")), num)
    dead = den == 0
    return torch.where(dead, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float("inf"))), num / den.clamp_min(1e-300))


# =============================================================================================== A. compositing
# both sides of every C boundary, the first N of C = 4 (193) and of C = 8 (257), a C = 8 shape with idle lanes (320: lanes
# 40..63 own no sample), 449 (the first N at which every lane of the C = 8 instance owns one) and the maximum
COMPOSITE_N = [2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 449, 511, 512]
COMPOSITE_R = 5                      # one workgroup of four rays and a tail of one
COMPOSITE_R_EDGES = (193, [0, 1, 4])  # at N = 193: no ray, one ray, exactly one workgroup
COMPOSITE_MAX_N = 512
FAMILIES = ["base", "opaque", "ties", "gate", "dead", "thin"]
FAMILY_N = [65, 193, 512]
NOISELESS = ("dead", "thin")         # families that are defined without the density noise
POINTER_N = [65, 257]
# the bounds of tests/test_hip_train_gpu.py, applied per ray: max(these, 3 x the float32 yardstick of that ray)
COMPOSITE_BOUNDS = {"rgb_exp": 2e-6, "t_exp": 2e-6, "weights": 2e-6, "d_rgb": 1e-5, "d_sigma": 1e-4}


def composite_instance(N):
    """The template instance launch_composite_ex / launch_composite_backward pick for N samples per ray."""
    C = (N + 63) // 64
    return C if C <= 4 else (8 if C <= 8 else None)


def composite_cases():
    """(family, N, white_bkgd, with_noise) of the per-ray comparison."""
    out = []
    for fam in FAMILIES:
        for N in (COMPOSITE_N if fam == "base" else FAMILY_N):
            for white in (0, 1):
                for nz in ((False,) if fam in NOISELESS else (True, False)):
                    out.append((fam, N, white, nz))
    return out


def base_inputs(R, N, seed):
    """rgb [R,N,3], sigma [R,N], sorted depths [R,N], noise [R,N] (float32): the generic inputs of tests/test_hip_train_gpu.py"""
    rng = np.random.default_rng(seed)
    rgb = torch.from_numpy(rng.random((R, N, 3)).astype(np.float32))
    sigma = torch.from_numpy((rng.standard_normal((R, N)) * 8).astype(np.float32))
    ts = torch.from_numpy(np.sort(rng.random((R, N)).astype(np.float32), -1))
    noise = torch.from_numpy(rng.standard_normal((R, N)).astype(np.float32))
    return rgb, sigma, ts, noise


def opaque_index(N):
    return N // 3


def composite_inputs(family, R, N, with_noise=True):
    """-> rgb, sigma, ts, noise (None without noise), float32 on the CPU.

    base    generic
    opaque  sample N // 3 has sigma = 3e4, noise = 0 and the next depth >= 0.01 behind: alpha == 1 exactly in float32,
            keep = 1e-10, every sample behind it sees T ~ 1e-10
    ties    every odd depth equals the even depth before it: delta = 0, alpha = 0 and d sigma = 0 there
    gate    sigma and noise are multiples of 2^-10 and sigma + noise is a chosen target -- a third positive, a third negative,
            a third exactly 0 -- so the float32 sum is exact and the float64 reference sees the same density
    dead    sigma <= 0 everywhere (some exactly 0), no noise: every output and gradient exactly 0, rgb_exp exactly 1 on white
    thin    |sigma| * 1e-4, no noise, the last sample (delta = 1e10) at 0: alpha below 1e-4 on more than 99 % of the samples
            and below 1e-3 on all, the whole ray transparent (sum of alpha < 3e-3)"""
    seed = 1000 * FAMILIES.index(family) + N + 7 * R
    rgb, sigma, ts, noise = base_inputs(R, N, seed)
    rng = np.random.default_rng(seed + 500000)
    if family == "opaque":
        k = opaque_index(N)
        sigma[:, k], noise[:, k] = 3e4, 0.0
        ts[:, k + 1:] += 0.01
    elif family == "ties":
        m = N // 2
        ts[:, 1:2 * m:2] = ts[:, 0:2 * m:2]
    elif family == "gate":
        q = 2.0 ** -10
        sigma = torch.round(sigma / q) * q
        kind = torch.from_numpy(rng.integers(0, 3, (R, N)))
        mag = torch.from_numpy(np.maximum(np.round(np.abs(rng.standard_normal((R, N)) * 4) / q), 1.0) * q).float()   # >= 2^-10
        target = torch.where(kind == 0, mag, torch.where(kind == 1, -mag, torch.zeros_like(mag)))
        if with_noise:
            noise = target - sigma          # exact: multiples of 2^-10 below 2^7
        else:
            sigma = target                  # without the noise the density itself carries the three kinds
    elif family == "dead":
        sigma = -sigma.abs()
        sigma[:, ::5] = 0.0
    elif family == "thin":
        sigma = sigma.abs() * 1e-4
        sigma[:, -1] = 0.0
    if family in NOISELESS:
        assert not with_noise
    return rgb, sigma, ts, (noise if with_noise else None)


def composite_upstream(R, N, seed=7):
    """dL/d rgb_exp [R,3], dL/d t_exp [R], dL/d weights [R,N]"""
    g = np.random.default_rng(seed + N)
    return (torch.from_numpy(g.standard_normal((R, 3)).astype(np.float32)), torch.from_numpy(g.standard_normal(R).astype(np.float32)),
            torch.from_numpy(g.standard_normal((R, N)).astype(np.float32)))


def composite_reference(rgb, sigma, ts, noise, white, g_rgb=None, g_t=None, g_w=None, dtype=torch.float64):
    """Autograd through oracle.raymarch.composite on the float32 inputs converted to `dtype`, as
    test_composite_backward_matches_autograd_on_the_oracle builds it; a missing upstream gradient is zero.
    -> dict of float64 tensors rgb_exp, t_exp, weights, d_rgb, d_sigma"""
    r, s = rgb.to(dtype).requires_grad_(True), sigma.to(dtype).requires_grad_(True)
    o_rgb, o_t, o_w = raymarch.composite(r, s if noise is None else s + noise.to(dtype), ts.to(dtype))
    if white:
        o_rgb = o_rgb + (1. - o_w.sum(-1, keepdim=True))          # utils.py:381-384
    loss = (r * 0).sum() + (s * 0).sum()
    for o, g in ((o_rgb, g_rgb), (o_t, g_t), (o_w, g_w)):
        if g is not None:
            loss = loss + (o * g.to(dtype)).sum()
    d_r, d_s = torch.autograd.grad(loss, (r, s))
    return {"rgb_exp": o_rgb.detach().double(), "t_exp": o_t.detach().double(), "weights": o_w.detach().double(),
            "d_rgb": d_r.double(), "d_sigma": d_s.double()}


_composite_refs = {}


def composite_references(family, N, white, with_noise, R=COMPOSITE_R):
    """(inputs, upstream, float64 reference, float32 yardstick reference) of a case, computed once."""
    key = (family, N, white, with_noise, R)
    if key not in _composite_refs:
        inp = composite_inputs(family, R, N, with_noise)
        up = composite_upstream(R, N)
        _composite_refs[key] = (inp, up, composite_reference(*inp, white, *up), composite_reference(*inp, white, *up, dtype=torch.float32))
    return _composite_refs[key]


# =============================================================================================== B. dense layers
# (in_features, out_features) of every nn.Linear of the four trainable modules of models.py: MLP_style (the NeRF network),
# StyleMLP_before_concat, StyleMLP_Wild_multilayers -- StyleLatents_variational has none
LAYER_SHAPES = {
    "nerf": [(63, 256), (256, 256), (319, 256), (256, 1), (283, 128), (128, 3)],
    "concat": [(95, 256), (288, 256), (351, 256)],
    "style": [(607, 256), (288, 256), (351, 256), (288, 3)],
}
# (M, K, N), fp16x3; nsplit / mpad: backward_split below
LINEAR_CASES = [
    (1, 63, 256),        # nsplit 1, mpad 32 > M; K % 4 != 0 (no pre-split weight in the forward)
    (33, 319, 256),      # nsplit 1, mpad 64 > M: a second, partial 32-row transpose tile
    (1024, 256, 256),    # nsplit 1, mpad == M: no memset
    (1025, 256, 256),    # nsplit 2, mpad 1088 > M
    (2048, 283, 128),    # nsplit 2, mpad == M
    (1025, 256, 1),      # N % 4 != 0: scale_copy + float loads in the dx GEMM; nsplit 2
    (1025, 128, 3),      # the same at N = 3; nsplit 2
    (6401, 256, 256),    # 101 x 4 = 404 tiles of 64 x 64 in the dx GEMM: the 64 x 64 workgroup tile (mid >= 400)
    (65537, 63, 256),    # nsplit 64: the cap
]
SUBSET_CASES = [(1025, 256, 256), (33, 319, 256)]              # every non-empty subset of {dx, dW, db}
SCALE_CASE = (1025, 256, 256)                                  # upstream gradient x 2^-100, 1, 2^100 and zero
SCALES = [-100, 0, 100]
UNEVEN_CASE = (1025, 256, 256)                                 # rows of dy that differ by 2^30
FP16_CASES = [(33, 319, 256), (1025, 256, 256), (1025, 256, 3)]
ACTIVATION_N = [1, 255, 256, 257]
LINEAR_BOUNDS = {"y": 2e-6, "dx": 5e-6, "dW": 5e-6, "db": 5e-6}      # tests/test_hip_backward_gpu.py, of the tensor maximum
FP16_BOUND = 2e-6
SUBSETS = [("dx",), ("dW",), ("db",), ("dx", "dW"), ("dx", "db"), ("dW", "db"), ("dx", "dW", "db")]


def backward_split(M, K, N):
    """csrc/style2d.hip backward_split: -> (nsplit, mc), mpad = nsplit * mc"""
    tiles = ((N + 63) // 64) * ((K + 63) // 64)
    nsplit = max(1, min(min(64, (512 + tiles - 1) // tiles), (M + 1023) // 1024))
    mc = ((M + nsplit - 1) // nsplit + 31) // 32 * 32
    return nsplit, mc


def gemm_mid(M, N, batch=1):
    """launch_gemm's tile count of an [M, N] product: below 400 the 32 x 32 workgroup tile, from 400 on 64 x 64"""
    return ((M + 63) // 64) * ((N + 63) // 64) * batch


def linear_inputs(M, K, N, seed=None):
    """x [M,K], W [N,K] ~ 1/sqrt(K), b [N], dy [M,N] float32"""
    rng = np.random.default_rng(M + K + 7 * N if seed is None else seed)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    return f(M, K), f(N, K) / math.sqrt(K), f(N) * 0.1, f(M, N)


def scale_case_dy(dy):
    """dy rescaled so that max |dy| = 1536 lies in [2^10, 2^11): grad_scale_kernel's exponent 10 - e is then 0 at scale 1
    and exactly +-100 -- the ends of the range it clamps to -- at 2^-+100, so the rescaling is a power of two the
    kernel undoes exactly at all three scales (the per-row exponents of dx, row_scale_kernel, clamp at +-126 and stay
    inside too: tests/test_train_kernel_shapes_cpu.py)."""
    return dy * (1536.0 / float(dy.abs().max()))


def uneven_rows(dy):
    """every third row of dy at 2^-30 of the others"""
    out = dy.clone()
    out[1::3] *= 2.0 ** -30
    return out


def grad_scale_exponent(dy):
    """grad_scale_kernel: k with s = 2^k, from the bits of max |dy| (0 for a zero / non-finite maximum)"""
    m = float(dy.abs().max())
    if m == 0 or not math.isfinite(m):
        return 0
    e = math.frexp(m)[1] - 1            # max |dy| in [2^e, 2^(e+1))
    return max(-100, min(100, 10 - e))


def row_scale_exponents(dy):
    """row_scale_kernel: [M] int k_m with s_m = 2^k_m from the largest magnitude of row m (ungated); |k_m| <= 126, 0 for a zero row"""
    m = dy.abs().amax(1)
    e = torch.frexp(m)[1] - 1
    k = torch.clamp(10 - e, -126, 126)
    return torch.where((m == 0) | ~torch.isfinite(m), torch.zeros_like(k), k)


def linear_reference(x, W, b, dy, gate, dtype=torch.float64):
    """y = x W^T + b and the gradients of sum(y * gate * dy): -> dict y (ungated), dx, dW, db in float64.  gate [M,N] bool or None"""
    x_, W_, dy_ = x.to(dtype), W.to(dtype), dy.to(dtype)
    y = x_ @ W_.T + b.to(dtype)
    g = dy_ if gate is None else dy_ * gate.to(dtype)
    return {"y": y.double(), "dx": (g @ W_).double(), "dW": (g.T @ x_).double(), "db": g.sum(0).double()}


def split16(v):
    """float32 -> (hi, lo) as float32 values of the fp16 halves: hi = fp16(v), lo = fp16(v - hi) (split_kernel)"""
    hi = v.half().float()
    return hi, (v - hi).half().float()


def fp16_model(x, W, b, dy, gate, dtype=torch.float64):
    """What precision = fp16 computes, as read from gemm_kernel<.., SPLIT = false, ..> and tgtc_s2d_linear_backward:

    forward   y = fp16(x) . fp16(W)^T + b: put4<false> (or the pre-split hi halves) rounds BOTH operands once to fp16
              (round to nearest even), the MFMA accumulates in float32, the bias is added in float32
    backward  s = 2^k from max |dy| (ungated, grad_scale_kernel), s_m = 2^k_m from the maximum of row m (row_scale_kernel);
              g = gate ? s * dy : 0 and g' = gate ? s_m * dy : 0 in float32 (exact: powers of two)
              dx = (1/s_m) fp16(g') . fp16(W)   -- N % 4 == 0: scale_split_kernel's hi halves x split_kernel's hi halves of
                                                   W^T; otherwise scale_copy_kernel's floats and W^T rounded by put4<false>
              dW = (1/s) fp16(g)^T . fp16(x)    -- transpose_ld_half_kernel's hi halves of both, SPLIT = false reads no lo
              db = (1/s) sum_m (hi + lo)(g)     -- rowsum_kernel adds BOTH halves whatever the precision
    -> the products of those rounded operands in `dtype` (float64: the reference; float32: the yardstick)"""
    s = 2.0 ** grad_scale_exponent(dy)
    sm = torch.ldexp(torch.ones(dy.shape[0]), row_scale_exponents(dy))[:, None]
    gated = dy if gate is None else dy * gate.float()
    gh, gl = split16(gated * s)
    xh, Wh = x.half().to(dtype), W.half().to(dtype)
    y = xh @ Wh.T + b.to(dtype)
    gh_ = gh.to(dtype)
    return {"y": y.double(), "dx": (((gated * sm).half().to(dtype) @ Wh) / sm.to(dtype)).double(), "dW": ((gh_.T @ xh) / s).double(),
            "db": ((gh.to(dtype) + gl.to(dtype)).sum(0) / s).double()}


def activation_inputs(mode, n):
    """(dy, y) of tgtc_s2d_activation.  mode 0 (ReLU backward): y has exact zeros, negatives and positives; mode 1 (sigmoid
    backward): y in (0, 1); mode 2 (sigmoid forward, y unused): inputs over +-100, both ends included"""
    rng = np.random.default_rng(10 * n + mode)
    dy = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
    if mode == 0:
        y = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
        y[::3] = 0.0
        return dy, y
    if mode == 1:
        return dy, torch.from_numpy(rng.uniform(0, 1, n).astype(np.float32))
    x = torch.from_numpy(rng.uniform(-100, 100, n).astype(np.float32))
    x[0] = 100.0
    x[-1] = -100.0 if n > 1 else x[-1]
    return x, None


def activation_reference(mode, dy, y):
    d = dy.double()
    if mode == 0:
        return d * (y > 0).double()
    if mode == 1:
        return d * y.double() * (1 - y.double())
    return torch.sigmoid(d)


# =============================================================================================== C. latent gather
LATENT_S, LATENT_F, LATENT_D = 3, 5, 32
LATENT_R = [0, 1, 7, 8, 9, 257]          # R * D on both sides of the 256-thread block (8 * 32 = 256)
LATENT_SCALES = [0.0, 0.35, 1.0]
LATENT_CROWD = (1, 2, 200)               # at R = 257: 200 rays on row (sid 1, fid 2)
def bad_latent_ids(S=LATENT_S, F=LATENT_F):
    """(sid, fid, type) that StyleLatents_variational.forward refuses with S styles of F frames.  The fourth is the first
    flat index behind the x7 table, 7 S F, reached from the last style; with ONE style that is the pair (S - 1, 7 F), and with
    more styles (S - 1, 7 F) itself is a valid wrapped id (flat = (S - 1) F + 7 F < 7 S F) here and in the reference."""
    return [(S, 0, "llff"), (-1, F, "llff"), (0, -1, "llff"), (S - 1, 7 * S * F - (S - 1) * F, "llff"), (0, S * F, "blender")]


def latent_tables(S=LATENT_S, F=LATENT_F, D=LATENT_D):
    """latents [S,F,D], mu [S,D] float32: randn / 4.  The forward bound of the sweep is the 1e-7 ABSOLUTE of
    test_latents_golden against float64; mu + s (z - mu) in float32 rounds the difference and the sum once each, half an ulp
    of each, which stays below 1e-7 while |z - mu| < 1 and |out| < 1 (3e-8 + 3e-8) -- randn / 4 keeps 4-sigma values there,
    so that the bound measures the kernel and not the number format."""
    rng = np.random.default_rng(4)
    return (torch.from_numpy((rng.standard_normal((S, F, D)) / 4).astype(np.float32)),
            torch.from_numpy((rng.standard_normal((S, D)) / 4).astype(np.float32)))


def latent_ids(R, llff, S=LATENT_S, F=LATENT_F):
    """style_ids, frame_ids [R] int64, all valid: sid in [0, S), fid >= 0, sid * F + fid < rows (7 * rows for llff); the
    largest flat index is taken whenever R > 0, and at R = 257 200 rays share one row (and few other rows are hit at all)."""
    rng = np.random.default_rng(R + (1000 if llff else 0))
    rows = S * F
    limit = 7 * rows if llff else rows
    sid = torch.from_numpy(rng.integers(0, S, R))
    fid = torch.from_numpy(rng.integers(0, F, R))
    if llff and R:
        wrap = torch.from_numpy(rng.integers(0, 7, R))
        fid = torch.minimum(fid + wrap * rows, limit - 1 - sid * F)
    if R >= 257:
        s0, f0, n = LATENT_CROWD
        sid[:n], fid[:n] = s0, f0
        sid[n:], fid[n:] = torch.tensor([0, 2, 2])[torch.arange(R - n) % 3], torch.tensor([4, 0, 3])[torch.arange(R - n) % 3]
    if R:
        sid[-1], fid[-1] = S - 1, limit - 1 - (S - 1) * F
    return sid.long(), fid.long()


def latent_reference(lat, mu, sid, fid, scale, llff, g, dtype=torch.float64):
    """oracle.fields.latents_forward with autograd -> out, d_latents, d_mu (float64)"""
    w = {"latents": lat.to(dtype).requires_grad_(True), "style_latents_mu": mu.to(dtype).requires_grad_(True)}
    out = fields.latents_forward(w, sid, fid, sigma_scale=scale, llff=llff)
    loss = (out * g.to(dtype)).sum() + (w["latents"] * 0).sum() + (w["style_latents_mu"] * 0).sum()
    d_lat, d_mu = torch.autograd.grad(loss, (w["latents"], w["style_latents_mu"]))
    return out.detach().double(), d_lat.double(), d_mu.double()


# =============================================================================================== D. fused trainer
TRAIN_DRAWS, TRAIN_SEED = 1024, 20
TRAIN_M = [1, 127, 128, 129, 385]        # one sample; one short of, exactly, one past the 128-sample tile; three tiles and one
TRAIN_MARGIN = 1e-4
G_RGB, G_SIGMA = 1e-3, 1e-5              # the upstream scales of test_fused_training_path_matches_the_unfused_one


def float64_preactivations(sd, pts, dirs):
    """every ReLU layer's pre-activations of the oracle's network in float64: [M, units] (models.py:95-111)"""
    w = {k: v.double() for k, v in T(sd).items()}
    pe, de = fields.posenc(pts, 10).double(), fields.posenc(dirs, 4).double()
    lin = lambda name, x: x @ w["net.%s.weight" % name].T + w["net.%s.bias" % name]
    zs, h = [], None
    for i in range(8):
        x = pe if i == 0 else (torch.cat([pe, h], -1) if i == 5 else h)
        z = lin("base_layers.%d" % i, x)
        zs.append(z)
        h = torch.relu(z)
    z = lin("base_remap_layer", h)
    zs.append(z)
    z = lin("rgb_layers.0", torch.cat([torch.relu(z), de], -1))
    zs.append(z)
    return torch.cat(zs, -1)


_train = {}


def train_samples():
    """(pts, dirs) float64 [n, 3]: the draws whose float64 pre-activations are all at least TRAIN_MARGIN from zero -- the
    samples on whose ReLU gates a float32 forward and the float64 oracle cannot disagree."""
    if "samples" not in _train:
        from tgtc_style_amd import synth
        rng = np.random.default_rng(TRAIN_SEED)
        pts = torch.from_numpy(rng.uniform(-1.2, 1.2, (TRAIN_DRAWS, 3)))
        dirs = torch.from_numpy(rng.uniform(-1, 1, (TRAIN_DRAWS, 3)))
        keep = (float64_preactivations(synth.nerf_state(1), pts, dirs).abs() >= TRAIN_MARGIN).all(-1)
        _train["samples"] = (pts[keep].contiguous(), dirs[keep].contiguous())
    return _train["samples"]


def train_upstream(M, scales=None):
    """w_rgb [M,3], w_sigma [M] float32: randn at G_RGB / G_SIGMA, times a per-sample scale (exact powers of two)"""
    rng = np.random.default_rng(300 + M)
    w_rgb = torch.from_numpy(rng.standard_normal((M, 3)).astype(np.float32) * np.float32(G_RGB))
    w_sig = torch.from_numpy(rng.standard_normal(M).astype(np.float32) * np.float32(G_SIGMA))
    if scales is not None:
        w_rgb, w_sig = w_rgb * scales[:, None], w_sig * scales
    return w_rgb, w_sig


def uneven_scales(case):
    """[385] float32 per-sample factors: four workgroup tiles, the last holding one sample.
    1: tile 0 at 1, tile 1 exactly zero, tile 2 at 2^-80, the lone sample at 2^10
    2: only tile 2 non-zero, at 2^-80 -- above the 2^-92 that scale_exp clamps at, so the rescaling is exact
    3: only tile 2, at 2^-110 -- below the clamp: precision is lost by design, the gradients must stay finite"""
    s = torch.zeros(385)
    if case == 1:
        s[:128], s[256:384], s[384] = 1.0, 2.0 ** -80, 2.0 ** 10
    else:
        s[256:384] = 2.0 ** (-80 if case == 2 else -110)
    return s


def train_reference(pts, dirs, w_rgb, w_sig, dtype):
    """d/d every weight of sum(w_rgb * rgb) + sum(w_sigma * sigma) of the oracle's fine network (synth seed 1) in `dtype`"""
    from tgtc_style_amd import synth
    M = pts.shape[0]
    w = {k: v.clone().to(dtype).requires_grad_() for k, v in T(synth.nerf_state(1)).items()}
    ret = fields.nerf_mlp(w, fields.posenc(pts, 10).to(dtype), fields.posenc(dirs, 4).to(dtype))
    ((ret["rgb"] * w_rgb.to(dtype)).sum() + (ret["sigma"].reshape(M) * w_sig.to(dtype)).sum()).backward()
    return {k: v.grad.double() for k, v in w.items()}, ret["rgb"].detach().double(), ret["sigma"].detach().reshape(M).double()


def train_references(M, case=None):
    """(pts, dirs, w_rgb, w_sig, float64 gradients, float32 gradients, float64 rgb, float64 sigma), computed once"""
    key = (M, case)
    if key not in _train:
        pts, dirs = (t[:M] for t in train_samples())
        w_rgb, w_sig = train_upstream(M, None if case is None else uneven_scales(case))
        g64, rgb, sig = train_reference(pts, dirs, w_rgb, w_sig, torch.float64)
        g32, _, _ = train_reference(pts, dirs, w_rgb, w_sig, torch.float32)
        _train[key] = (pts, dirs, w_rgb, w_sig, g64, g32, rgb, sig)
    return _train[key]
