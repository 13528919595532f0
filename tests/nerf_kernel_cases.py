"""Test helper: the cases of the plain per-sample sweep (tests/test_nerf_kernel_shapes_cpu.py, _gpu.py) -- sample counts, ray
shapes, point / encoded-input / direction / weight families of the five plain NeRF kernels -- with their inputs, the float64
oracle, and the arithmetic model of the fp16mx mode (moved here from tests/probes/emu_mx.py, which now imports it).

Kernels (csrc/mlp_nerf.hip, mlp_nerf_x3s.hip, mlp_nerf_mx.hip, mlp_nerf_mx2.hip), all per sample, a sample one MFMA column:
  A  nerf_mlp_kernel<CfgExact>  fp16x3   8 waves x 1 tile  = 128 samples per workgroup
  B  nerf_x3s_kernel            fp16x3   persistent, 4 waves x 2 tiles = 128 per pass (rays, sigma only)
  C  nerf_mlp_kernel<CfgFast>   fp16     8 waves x 2 tiles = 256 per workgroup
  D  nerf_mx_kernel             fp16mx   128 per workgroup (whenever base_remap is asked)
  E  nerf_mx2_kernel            fp16mx   persistent, 4 waves x 2 tiles = 128 per pass (no base_remap; rays; the list)

No fixtures and no GPU here: numpy / torch CPU only."""
import numpy as np
import torch

from tgtc_style_amd import synth

import test_hip_style_shapes as S       # rel, oracle, T, Y_FLOOR: the stylised sweep's helpers, shared

# ------------------------------------------------------------------------------------------------------- cases
TILES = (16, 32, 128, 256)      # one-tile wave, two-tile wave, workgroup / pass of A, B, D, E, workgroup of C
M_LIST = [1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1000]
RAY_SHAPES = [(1, 1), (1, 15), (4, 8), (6, 16), (3, 17), (5, 24), (4, 32), (5, 37), (2, 64), (9, 100), (40, 129), (7, 192),
              (3, 200)]
FAMILY_M = 257                  # one sample in the third (A, B, D, E) / second (C) workgroup, in tile 0 of a two-tile wave
BITS_SHAPE = (40, 129)
LIST_SHAPES = [(5, 37), (3, 200), (40, 129)]
LIST_KINDS = ["all", "third", "one", "127", "128", "129"]
ENC_M = [33, 257]               # the encodings as outputs
REVISIT_N = 100
POINT_FAMILIES = ["unit", "mid", "wide", "special"]
ENC_FAMILIES = ["true", "free"]
DIR_PATTERNS = ["each", "one", "lane", "blocks16", "blocks32"]
RAY_DIRS = ["each", "parallel"]     # per-ray directions; the per-sample patterns of a ray launch are its N
WEIGHT_FAMILIES = ["base", "rows", "outliers", "dead"]
PRECISIONS = ["fp16x3", "fp16mx", "fp16"]
KERNELS = {"A": "fp16x3", "B": "fp16x3", "C": "fp16", "D": "fp16mx", "E": "fp16mx"}

# (M, point family, direction pattern, weight family): tgtc_nerf_forward
PTS_CASES = ([(M, "unit", "each", "base") for M in M_LIST] +
             [(FAMILY_M, pf, "each", "base") for pf in POINT_FAMILIES[1:]] +
             [(FAMILY_M, "unit", dp, "base") for dp in DIR_PATTERNS[1:]] +
             [(FAMILY_M, "unit", "each", wf) for wf in WEIGHT_FAMILIES[1:]])
# (M, encoded family, direction pattern, weight family): tgtc_nerf_mlp_forward
ENC_CASES = ([(M, "true", "each", "base") for M in M_LIST] + [(FAMILY_M, "free", "each", "base")] +
             [(FAMILY_M, "true", dp, "base") for dp in DIR_PATTERNS[1:]] +
             [(FAMILY_M, "true", "each", wf) for wf in WEIGHT_FAMILIES[1:]])
FAMILY_PTS_CASES = [c for c in PTS_CASES if c[0] == FAMILY_M]
FAMILY_ENC_CASES = [c for c in ENC_CASES if c[0] == FAMILY_M]
# (R, N, ray directions, weight family): tgtc_nerf_forward_rays
RAY_CASES = ([(R, N, rdk, "base") for R, N in RAY_SHAPES for rdk in RAY_DIRS] +
             [(R, N, "each", wf) for R, N in ((5, 37), (9, 100)) for wf in WEIGHT_FAMILIES[1:]])
# which kernels a case list reaches, by entry point (csrc/mlp_nerf.hip dispatch_nerf, mlp_nerf_mx.hip nerf_mx_launch)
REACHES = {"pts": "ACDE", "enc": "ACDE", "rays": "ABCE"}


def pts_id(case):
    return "M%d-%s-%s-%s" % case


def ray_id(case):
    return "%dx%d-%s-%s" % case


# ------------------------------------------------------------------------------------------------------- inputs
SPECIAL = np.array([0.0, 2.0 ** -30, -2.0 ** -30, 0.5, -0.5, 1.0, -1.0])


def points(family, M, seed=0, raw=False):
    """[M, 3] float64 sample positions.  raw: the one-sample `unit` case as drawn (see _dense_sample)."""
    rng = np.random.default_rng(70000 + 8 * M + POINT_FAMILIES.index(family) + 1000003 * seed)
    if family == "special":
        p = SPECIAL[rng.integers(0, len(SPECIAL), (M, 3))]
        p[0] = 0.0                      # the all-zero point (directions() gives it the all-zero direction)
        return torch.from_numpy(p)
    half = {"unit": 1.5, "mid": 8.0, "wide": 100.0}[family]
    if M == 1 and family == "unit":
        candidates = torch.from_numpy(rng.uniform(-half, half, (16, 3)))
        return candidates[:1].contiguous() if raw else _dense_sample(candidates)    # candidate 0 is what a draw of one gives
    return torch.from_numpy(rng.uniform(-half, half, (M, 3)))


def _dense_sample(candidates):
    """The one-sample case.  Errors are read against max|ref| of the tensor, and a single sample whose density happens to sit
    near zero (sigma crosses zero; |sigma| < 10 in five of eight draws, against 100 .. 240 for the tensors of every larger
    case) has no scale to be read against: the arithmetic model itself is at 2e-3 .. 1e-2 there.  So the sample is the one of
    16 candidates with the largest |sigma| in the float64 oracle on the base weights -- chosen on the CPU from the reference
    alone, and test_mx_guard_is_in_force_on_points holds the case to 4 y_mx <= 1e-3 like every other.  The draw as it comes
    (candidate 0, points(.., raw=True)) is launched as well, through every kernel: figures printed, outputs finite, canaries."""
    from oracle import fields
    d = directions("each", 1).expand(candidates.shape[0], 3)
    with torch.no_grad():
        sigma = fields.style_nerf(S.T(synth.nerf_state(1), torch.float64), candidates, d, dtype=torch.float64)["sigma"]
    return candidates[int(sigma.abs().argmax())][None].contiguous()


def directions(pattern, M, special=False):
    """[M, 3] float64 view directions, one per sample, in one of DIR_PATTERNS.  special: rows drawn from SPECIAL instead
    ('each' only), row 0 all zero."""
    rng = np.random.default_rng(71000 + 8 * M + DIR_PATTERNS.index(pattern))
    if special:
        assert pattern == "each"
        d = SPECIAL[rng.integers(0, len(SPECIAL), (M, 3))]
        d[0] = 0.0
        return torch.from_numpy(d)
    a, b = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
    assert np.abs(a - b).max() > 0.25           # "clearly different": far beyond every bar of the colour head
    i = np.arange(M)
    if pattern == "each":
        d = rng.uniform(-1, 1, (M, 3))
    elif pattern == "one":
        d = np.repeat(a[None], M, 0)
    elif pattern == "lane":                     # lane 5 of tile 1 of every two-tile wave
        d = np.where((i % 32 == 21)[:, None], b[None], a[None])
    elif pattern == "blocks16":
        d = np.where(((i // 16) % 2 == 1)[:, None], b[None], a[None])
    elif pattern == "blocks32":
        d = np.where(((i // 32) % 2 == 1)[:, None], b[None], a[None])
    else:
        raise ValueError(pattern)
    return torch.from_numpy(np.ascontiguousarray(d))


def pts_inputs(case):
    M, pf, dp, _ = case
    return points(pf, M), directions(dp, M, special=pf == "special")


def enc_inputs(case):
    """(pts_enc [M,63], dirs_enc [M,27]) float32.  'true': the float32 encodings of `unit` points and the pattern's directions;
    'free': U(-1, 1) in all 90 columns (no encoding of anything)."""
    from oracle import fields
    M, ef, dp, _ = case
    if ef == "free":
        rng = np.random.default_rng(72000 + M)
        return (torch.from_numpy(rng.uniform(-1, 1, (M, 63)).astype(np.float32)),
                torch.from_numpy(rng.uniform(-1, 1, (M, 27)).astype(np.float32)))
    return fields.posenc(points("unit", M), 10).float().contiguous(), fields.posenc(directions(dp, M), 4).float().contiguous()


def ray_inputs(R, N, rdk="each", seed=None):
    """The rays of the stylised sweep: origin xy ~ U(-1, 1), z = -1; direction xy ~ U(-0.3, 0.3), z = 2; ts sorted U(0, 1)
    float32.  'parallel': every ray carries ray 0's direction (different origins)."""
    rng = np.random.default_rng(73000 + 1000 * R + 8 * N if seed is None else seed)
    ro = np.concatenate([rng.uniform(-1, 1, (R, 2)), -np.ones((R, 1))], 1)
    rd = np.concatenate([rng.uniform(-.3, .3, (R, 2)), 2 * np.ones((R, 1))], 1)
    if rdk == "parallel":
        rd = np.repeat(rd[:1], R, 0)
    ts = np.sort(rng.uniform(0, 1, (R, N)).astype(np.float32), -1)
    return torch.from_numpy(ro), torch.from_numpy(np.ascontiguousarray(rd)), torch.from_numpy(ts)


def ray_points(ro, rd, ts):
    """pts = o + t d in float64 from the float32 depths, and the per-sample directions: [R*N, 3] each."""
    R, N = ts.shape
    pts = ro[:, None, :] + ts[..., None].double() * rd[:, None, :]
    return pts.reshape(R * N, 3), rd[:, None, :].expand(R, N, 3).reshape(R * N, 3)


def revisit_rays(n_cu):
    """R of the revisit launch of the persistent kernels B and E: 2.2 passes of 128 samples per CU and a ragged tail."""
    import math
    return math.ceil(2.2 * n_cu * 128 / REVISIT_N) + 7


# ------------------------------------------------------------------------------------------------------- weights
DEAD_LAYERS = (1, 2, 6, 7)              # trunk layers whose dead rows are zeroed: r1 == 0 in EqualisedNet::run
DEAD_ROWS = [0, 7, 100, 129, 255]
DEAD_COLS = [3, 64, 130, 200, 254]      # features nobody reads: r2 == 0
DEAD_RGB1_COLS = [5, 77]


def blocks():
    """Feature index lists of the 8 (kb, g) blocks of a 256-wide activation vector: the 32 values one lane converts to fp6
    together.  Checked against csrc/mlp_mx.h: a lane holds the 32 consecutive k = 32 (l >> 4) + i of a 128-deep block kb, i = 8 s
    + j over the four fp16 k-steps s; the values arrive from the accumulators of row tiles rt = 8 kb + 2 s + h, whose lane group
    g = l >> 4 holds rows 16 rt + 4 g + r (the base_remap store of mlp_nerf.hip writes exactly 16 rt + 4 g + 2 hf + {0, 1}):
    feature 128 kb + 32 s + 16 h + 4 g + r."""
    out = []
    for kb in range(2):
        for g in range(4):
            out.append([128 * kb + 32 * s + 16 * h + 4 * g + r for s in range(4) for h in range(2) for r in range(4)])
    return out


DEAD_BLOCK = blocks()[1]                # kb = 0, g = 1: 32 s + 16 h + 4 * 1 + r


def dead_units(sd):
    """The fine NeRF with dead units: a different function, the oracle runs on it.  Trunk layers 1, 2, 6, 7: rows DEAD_ROWS and
    the 32 rows of one fp6 activation block (DEAD_BLOCK) and their biases are zero.  Layers 3 and 4: their features DEAD_COLS
    are read by nobody (columns of base_layers.4, and of base_layers.5 at offset 63: it reads cat(pe, h)).  base_remap's
    features DEAD_COLS are not read by rgb_layers.0, and two features of rgb_layers.0 not by rgb_layers.1.  Layer 7's dead
    rows leave nonzero columns in both of its consumers (sigma_layer, base_remap_layer) unread."""
    sd = {k: v.copy() for k, v in sd.items()}
    rows = sorted(set(DEAD_ROWS) | set(DEAD_BLOCK))
    for l in DEAD_LAYERS:
        sd["net.base_layers.%d.weight" % l][rows, :] = 0
        sd["net.base_layers.%d.bias" % l][rows] = 0
    sd["net.base_layers.4.weight"][:, DEAD_COLS] = 0
    sd["net.base_layers.5.weight"][:, [63 + c for c in DEAD_COLS]] = 0
    sd["net.rgb_layers.0.weight"][:, DEAD_COLS] = 0
    sd["net.rgb_layers.1.weight"][:, DEAD_RGB1_COLS] = 0
    return sd


_STATES = {}
_DEAD_SCENE = []


def dead_scene():
    """(max|sigma|, share of samples with sigma > 0, min rgb, max rgb) of the 'dead' weights on 1 000 `unit` points in float64:
    what states("dead") asserted to be a scene."""
    states("dead")
    return _DEAD_SCENE[0]


def states(wf):
    """The fine NeRF synth.nerf_state(1) in a weight family, numpy state dict (cached).  'rows' / 'outliers' compute the base
    function and 'dead' stays a scene: both asserted in float64 here, before any sweep trusts them."""
    if wf in _STATES:
        return _STATES[wf]
    from oracle import fields
    base = synth.nerf_state(1)
    if wf == "base":
        _STATES[wf] = base
        return base
    p, d = points("unit", 1000, seed=1), directions("each", 1000)
    with torch.no_grad():
        ref = fields.style_nerf(S.T(base, torch.float64), p, d, dtype=torch.float64)
    if wf == "dead":
        sd = dead_units(base)
        with torch.no_grad():
            out = fields.style_nerf(S.T(sd, torch.float64), p, d, dtype=torch.float64)
        sig, rgb = out["sigma"], out["rgb"]
        _DEAD_SCENE.append((float(sig.abs().max()), float((sig > 0).double().mean()), float(rgb.min()), float(rgb.max())))
        # still a scene: densities of both signs at the base net's scale, colours that vary, and not the base function
        assert 10 <= float(sig.abs().max()) <= 1000 and 0.05 <= float((sig > 0).double().mean()) <= 0.5
        assert float(rgb.max() - rgb.min()) >= 0.3
        assert S.rel(out["rgb"], ref["rgb"]) > 1e-2 and S.rel(out["sigma"], ref["sigma"]) > 1e-2
        # the dead units are dead: the remap features nobody reads still vary, the dead block of layer 7 zeroes no output
        assert float(out["base_remap"][:, DEAD_COLS].abs().max()) > 0
    else:
        sd = synth.heavy_tailed(base, 11, wf)
        with torch.no_grad():
            out = fields.style_nerf(S.T(sd, torch.float64), p, d, dtype=torch.float64)
        for k in ("sigma", "rgb", "base_remap"):
            assert float((out[k] - ref[k]).abs().max()) <= 1e-9 * float(ref[k].abs().max()), (wf, k)
        assert max(float(np.abs(sd["net.base_layers.%d.weight" % l]).max() / np.abs(base["net.base_layers.%d.weight" % l]).max())
                   for l in range(8)) >= 16
    _STATES[wf] = sd
    return sd


# ------------------------------------------------------------------------------------------------------- oracle
TENSORS = ("sigma", "rgb", "base_remap")


def _three(out):
    return [out["sigma"], out["rgb"], out["base_remap"]]


def pts_oracle(key, wf, pts, dirs):
    """([sigma, rgb, base_remap] in float64, [y per tensor]) of oracle.fields.style_nerf; y = max(rel(float32 oracle, float64
    oracle), Y_FLOOR).  Cached under `key` and never written again."""
    from oracle import fields
    sd = states(wf)
    return S.oracle(("nerf",) + tuple(key), lambda dt: _three(fields.style_nerf(S.T(sd, dt), pts, dirs, dtype=dt)))


def enc_oracle(key, wf, pe, de):
    """The same of oracle.fields.nerf_mlp on the float32 encodings cast to the oracle's dtype."""
    from oracle import fields
    sd = states(wf)
    return S.oracle(("nerf",) + tuple(key), lambda dt: _three(fields.nerf_mlp(S.T(sd, dt), pe.to(dt), de.to(dt))))


def pts_case_oracle(case):
    pts, dirs = pts_inputs(case)
    return pts_oracle(("pts",) + tuple(case), case[3], pts, dirs)


def enc_case_oracle(case):
    pe, de = enc_inputs(case)
    return enc_oracle(("enc",) + tuple(case), case[3], pe, de)


def ray_case_oracle(case):
    R, N, rdk, wf = case
    return pts_oracle(("rays",) + tuple(case), wf, *ray_points(*ray_inputs(R, N, rdk)))


def encodings64(x, n_freqs):
    """float64 encoding of float64 x: the reference of the encodings the kernels write."""
    from oracle import fields
    return fields.posenc(x.double(), n_freqs)


# ------------------------------------------------------------------------------------------------------- fp16mx model
# The arithmetic of csrc/mlp_mx.h in numpy: y = Wh.Ah (fp16 x fp16) + Wl6.Ah6 + Wh6.Al6 (block-scaled e2m3 fp6), one exponent
# per weight row and one per 32 activations of a lane.  Left out: layer 0 (exact here), the packer's choice of the weight
# exponents where it differs from floor(log2(max)), EqualisedNet, and the finer scale of the kernel's lo block: with a block
# maximum in [2^E, 2^(E+1)), mx_store_act converts the unscaled lo values at 2^(E-13) (codes reach 4 of e2m3's 7.5), while
# split_act converts lo x 2048 at 2^(E-1), which is 2^(E-12) on lo (codes reach 2).  The model's Wh.Al6 term is one bit coarser
# than the kernel's: it makes y_mx larger, so the 4 y_mx guard is looser by that much, never tighter than the kernel can meet.
VALS = np.array([(c & 7) * 0.125 if (c >> 3) == 0 else (1 + (c & 7) / 8) * 2.0 ** ((c >> 3) - 1) for c in range(32)])


def e2m3(x):
    a = np.minimum(np.abs(x), 7.5)
    q = np.where(a < 1, a * 8, np.where(a < 2, 8 + (a - 1) * 8, np.where(a < 4, 16 + (a - 2) * 4, 24 + (a - 4) * 2)))
    c = np.clip(np.rint(q), 0, 31).astype(np.int64)
    return np.sign(x) * VALS[c]


def split_act(a, variant=None):
    """a: [M, K] float32 non-negative -> (Ah, Ah6, Al6) as float64 values"""
    ah = a.astype(np.float16).astype(np.float64)
    lo = ((a.astype(np.float32) - ah.astype(np.float32)) * np.float32(2048)).astype(np.float16).astype(np.float64)
    ah6 = np.zeros_like(ah)
    al6 = np.zeros_like(ah)
    K = a.shape[1]
    for idx in blocks():
        idx = [i for i in idx if i < K]
        if not idx:
            continue
        m = ah[:, idx].max(1)
        e = np.floor(np.log2(np.maximum(m, 2.0 ** -14)))
        s = 2.0 ** (e - 1)
        ah6[:, idx] = e2m3(ah[:, idx] / s[:, None]) * s[:, None]
        al6[:, idx] = e2m3(lo[:, idx] / s[:, None]) * s[:, None] / 2048
    return ah, ah6, al6


def split_w(W):
    wh = W.astype(np.float16).astype(np.float64)
    wl = (W.astype(np.float32) - wh.astype(np.float32)).astype(np.float64)
    m = np.abs(wh).max(1)
    e = np.floor(np.log2(np.maximum(m, 2.0 ** -14)))
    sh = 2.0 ** (e - 1)
    sl = sh / 2048
    wh6 = e2m3(wh / sh[:, None]) * sh[:, None]
    wl6 = e2m3(wl / sl[:, None]) * sl[:, None]
    return wh, wl6, wh6


def mx_linear(a, W, b, terms=(1, 1, 1)):
    ah, ah6, al6 = split_act(a, None)
    wh, wl6, wh6 = split_w(W)
    y = ah @ wh.T
    if terms[1]:
        y = y + ah6 @ wl6.T
    if terms[2]:
        y = y + al6 @ wh6.T
    return y + b


def exact_linear(a, W, b):
    return a.astype(np.float64) @ W.astype(np.float64).T + b


MODES = (("fp16+fp6 (all terms)", mx_linear), ("no corr1 (Wl.Ah)", lambda a, W, b: mx_linear(a, W, b, (1, 0, 1))),
         ("no corr2 (Wh.Al)", lambda a, W, b: mx_linear(a, W, b, (1, 1, 0))), ("fp16 only", lambda a, W, b: mx_linear(a, W, b, (1, 0, 0))))


def run(sd, pe, de, lin):
    """The fine NeRF on float64 arrays pe [M,63], de [M,27] with `lin(a, W, b)` as every dense layer but the first.
    -> (sigma [M], base_remap [M,256], rgb [M,3])"""
    relu = lambda x: np.maximum(x, 0)
    W = lambda n: sd["net." + n + ".weight"].astype(np.float64)
    B = lambda n: sd["net." + n + ".bias"].astype(np.float64)
    h = relu(pe @ W("base_layers.0").T + B("base_layers.0")).astype(np.float32)
    for i in range(7):
        n = "base_layers.%d" % (i + 1)
        if i == 4:
            w = W(n)
            y = lin(h, w[:, 63:].astype(np.float32), B(n)) + pe @ w[:, :63].T
        else:
            y = lin(h, W(n).astype(np.float32), B(n))
        h = relu(y).astype(np.float32)
    sigma = lin(h, W("sigma_layer").astype(np.float32), B("sigma_layer"))[:, 0]
    remap = relu(lin(h, W("base_remap_layer").astype(np.float32), B("base_remap_layer"))).astype(np.float32)
    w = W("rgb_layers.0")
    f = relu(lin(remap, w[:, :256].astype(np.float32), B("rgb_layers.0")) + de @ w[:, 256:].T).astype(np.float32)
    rgb = 1 / (1 + np.exp(-lin(f, W("rgb_layers.1").astype(np.float32), B("rgb_layers.1"))))
    return sigma, remap, rgb


def np_rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def probe_case():
    """The probe's own case: M = 1 000, nerf_state(1), points and directions U(-1, 1).  -> (sd, pe, de) float64 arrays holding
    the float32 encodings."""
    from oracle import fields
    rng = np.random.default_rng(0)
    pts, dirs = rng.uniform(-1, 1, (1000, 3)), rng.uniform(-1, 1, (1000, 3))
    pe = fields.posenc(torch.from_numpy(pts), 10).numpy().astype(np.float32).astype(np.float64)
    de = fields.posenc(torch.from_numpy(dirs), 4).numpy().astype(np.float32).astype(np.float64)
    return synth.nerf_state(1), pe, de


def probe_errors():
    """{mode name: (err sigma, err remap, err rgb)} of the four MODES on the probe's case, against `exact_linear`."""
    sd, pe, de = probe_case()
    ref = run(sd, pe, de, exact_linear)
    return {name: tuple(np_rel(o, r) for o, r in zip(run(sd, pe, de, lin), ref)) for name, lin in MODES}


MX_SAMPLES = 512
_YMX = {}


def y_mx(key, wf, pe, de):
    """Per tensor (sigma, rgb, base_remap): rel(model, float64) on at most MX_SAMPLES samples of a case; pe / de are the float32
    encodings the kernel is given or forms.  Cached."""
    key = tuple(key)
    if key not in _YMX:
        sd = states(wf)
        pe = pe[:MX_SAMPLES].float().double().numpy()
        de = de[:MX_SAMPLES].float().double().numpy()
        ref, got = run(sd, pe, de, exact_linear), run(sd, pe, de, mx_linear)
        _YMX[key] = [np_rel(got[i], ref[i]) for i in (0, 2, 1)]          # run's order is sigma, remap, rgb
    return _YMX[key]


def pts_case_y_mx(case):
    pts, dirs = pts_inputs(case)
    return y_mx(("pts",) + tuple(case), case[3], encodings64(pts, 10), encodings64(dirs, 4))


def enc_case_y_mx(case):
    return y_mx(("enc",) + tuple(case), case[3], *enc_inputs(case))


def ray_case_y_mx(case):
    R, N, rdk, wf = case
    pts, dirs = ray_points(*ray_inputs(R, N, rdk))
    return y_mx(("rays",) + tuple(case), wf, encodings64(pts, 10), encodings64(dirs, 4))


# ------------------------------------------------------------------------------------------------------- bars
TIGHT = {"fp16x3": 5e-5, "fp16": 1e-2}      # tests/test_hip_nerf.py TIGHT, without that file's x 2
TOL_MX = 1e-3                               # tests/test_hip_nerf.py TOL["fp16mx"]
K_X3 = 16                                   # the K of every family of the stylised sweep (tests/test_hip_style_shapes.py)
K_MX = 4                                    # the project's allowance for another summation order
ENC_ABS = 3e-7                              # sin / cos columns: the 2e-7 max-norm-relative bar of the golden test at max|ref| 1.5
MX_GUARDED_WEIGHTS = ("base", "dead")
MX_GUARDED_POINTS = ("unit", "mid")


def mx_guard(wf, y):
    """The fp16mx regression guard of one tensor: K_MX * y_mx where the weights are modelled (no equalisation in the model:
    'rows' / 'outliers' are not) and the guard is below the hard bar; else None (the ratio is printed only)."""
    return K_MX * y if wf in MX_GUARDED_WEIGHTS and K_MX * y <= TOL_MX else None
