"""Test helper: the cases of the density screen's domain sweep (tests/test_screen_domain_cpu.py, _gpu.py; DESIGN 3.1 "The
screen's domain") -- the two nets of the plain chain in the four weight families of nerf_kernel_cases, ray families inside,
across and far outside the screen's declared box |x|, |y|, |z| <= B, and rays whose samples crowd around a zero of the
float64 density, where a screen that errs drops live samples without luck being needed.

Every family is R x N samples generated as rays (origins, directions float64, depths float32): tgtc_nerf_screen_rays and
tgtc_nerf_forward_rays take them unchanged.  No fixtures and no GPU here: numpy / torch CPU only."""
import numpy as np
import torch

from tgtc_style_amd import synth

import nerf_kernel_cases as nk
import test_hip_style_shapes as S       # T, rel

# ------------------------------------------------------------------------------------------------------- cases
B = 2.0                                 # the declared box of the screen: kScreenBox of csrc/mlp_nerf_mx.h
R, N = 37, 128                          # 4 736 samples a family: 18.5 passes of the screen's stream, tiles that mix rays
NETS = {"coarse": (0, "fp16x3"), "fine": (1, "fp16mx")}         # synth.nerf_state seed, precision of the handle
WEIGHT_FAMILIES = ["base", "rows", "outliers", "dead"]
RAY_FAMILIES = ["cal", "box", "ndc-wide", "mid", "wide", "far-llff", "straddle"]
ZERO_SETS = {"zero-box": None, "zero-8": 8.0, "zero-30": 30.0, "zero-100": 100.0}      # |x| of the set; None: inside the box
ZERO_R = 32
FAMILIES = RAY_FAMILIES + list(ZERO_SETS)
IN_DOMAIN = ["cal", "box", "zero-box"]              # every sample inside the box
OUT_OF_DOMAIN = ["zero-8", "zero-30", "zero-100"]   # every sample outside it
CHAIN_SHAPES = [(1, 1), (3, 85), (5, 192)]          # the fp16 handle against the screen's packed form
CHAIN_WEIGHTS = ["base", "outliers"]
HALF = {"mid": 8.0, "wide": 100.0}
FACE_EPS = 1e-9     # no sample but the planted ones is this close to a face: o + t d rounded once (the kernels' FMA) or twice
#                     (numpy) is then on the same side of it
CASES = [(net, wf, fam) for net in NETS for wf in WEIGHT_FAMILIES for fam in FAMILIES]
DOMAIN_CASES = [(net, wf, fam) for net in NETS for wf in WEIGHT_FAMILIES for fam in ("cal", "box")]


def case_id(case):
    return "-".join(case)


# ------------------------------------------------------------------------------------------------------- weights
_STATES = {}
COARSE_HEAVY_SEED = 10                  # (the fine net's families are drawn with 11: nerf_kernel_cases.states)


def state(net, wf):
    """numpy state dict of a net in a weight family.  Fine: nerf_kernel_cases.states.  Coarse: the same construction on
    synth.nerf_state(0), asserted in float64 the same way -- 'rows' / 'outliers' compute the base function, 'dead' stays a
    scene."""
    if net == "fine":
        return nk.states(wf)
    if wf in _STATES:
        return _STATES[wf]
    from oracle import fields
    base = synth.nerf_state(0)
    if wf == "base":
        _STATES[wf] = base
        return base
    p, d = nk.points("unit", 1000, seed=2), nk.directions("each", 1000)
    with torch.no_grad():
        ref = fields.style_nerf(S.T(base, torch.float64), p, d, dtype=torch.float64)
        sd = nk.dead_units(base) if wf == "dead" else synth.heavy_tailed(base, COARSE_HEAVY_SEED, wf)
        out = fields.style_nerf(S.T(sd, torch.float64), p, d, dtype=torch.float64)
    if wf == "dead":
        sig, rgb = out["sigma"], out["rgb"]
        # (densities of both signs at the base net's scale: the dead rows lift this net's positive share from 0.18 to 0.78,
        # where the fine net's stays near 0.2 -- a scene all the same, one sample in five of it empty space)
        assert 10 <= float(sig.abs().max()) <= 1000 and 0.05 <= float((sig > 0).double().mean()) <= 0.85
        assert float(rgb.max() - rgb.min()) >= 0.3
        assert S.rel(out["rgb"], ref["rgb"]) > 1e-2 and S.rel(out["sigma"], ref["sigma"]) > 1e-2
        assert float(out["base_remap"][:, nk.DEAD_COLS].abs().max()) > 0
    else:
        for k in ("sigma", "rgb", "base_remap"):
            assert float((out[k] - ref[k]).abs().max()) <= 1e-9 * float(ref[k].abs().max()), (wf, k)
        assert max(float(np.abs(sd["net.base_layers.%d.weight" % l]).max() / np.abs(base["net.base_layers.%d.weight" % l]).max())
                   for l in range(8)) >= 16
    _STATES[wf] = sd
    return sd


def function_of(wf):
    """'rows' and 'outliers' compute the base function: the zero-crossing rays of a net are built once per function"""
    return "dead" if wf == "dead" else "base"


# ------------------------------------------------------------------------------------------------------- oracle
_W64 = {}


def sigma64(net, wf, pts):
    """float64 density of [M, 3] float64 positions (numpy or torch): the trunk and the sigma head of oracle.fields.nerf_mlp
    on the float64 encodings (test_sigma64_is_the_oracle ties the two)."""
    from oracle import fields
    if (net, wf) not in _W64:
        _W64[(net, wf)] = S.T(state(net, wf), torch.float64)
    sd = _W64[(net, wf)]
    pe = fields.posenc(torch.as_tensor(pts, dtype=torch.float64), 10)
    with torch.no_grad():
        h = torch.relu(fields._lin(sd, "net.base_layers.0", pe))
        for i in range(7):
            if i == 4:
                h = torch.cat([pe, h], -1)
            h = torch.relu(fields._lin(sd, "net.base_layers.%d" % (i + 1), h))
        return fields._lin(sd, "net.sigma_layer", h).squeeze(-1).numpy()


def positions(ro, rd, ts):
    """[R * N, 3] float64 numpy: o + t d from the float32 depths"""
    return nk.ray_points(ro, rd, ts)[0].numpy()


def in_box(pts):
    """the domain rule in float64: every coordinate |p| <= B (a NaN or an infinity is outside)"""
    return (np.abs(pts) <= B).all(-1)


# ------------------------------------------------------------------------------------------------------- ray families
def _t(ro, rd, ts):
    return (torch.from_numpy(np.ascontiguousarray(ro, dtype=np.float64)), torch.from_numpy(np.ascontiguousarray(rd, dtype=np.float64)),
            torch.from_numpy(np.ascontiguousarray(ts, dtype=np.float32)))


def _segments(rng, half, shrink=1.0):
    """rays from p0 to p1, both uniform in the cube of half-width `half` (p1 in that cube times `shrink`), depths sorted
    U(0, 1): the samples fill the cube"""
    p0 = rng.uniform(-half, half, (R, 3))
    p1 = rng.uniform(-half, half, (R, 3)) * shrink
    ts = np.sort(rng.uniform(0, 1, (R, N)).astype(np.float32), -1)
    return p0, p1 - p0, ts


BOX_SHAPE = (592, 8)    # R x N of `box`, the same 4 736 samples
BOX_FACE_RAYS = 7       # rays 0..5 of `box` start on the six faces, ray 6 in a corner: their first depth is 0, the origin itself
PIN_VALUES = [B, np.nextafter(B, np.inf), np.nextafter(B, 0.0), -B, np.nextafter(-B, -np.inf), np.nextafter(-B, 0.0)]
STRADDLE_PINS = [(k, a, v) for k, a in ((0, 2), (1, 2), (2, 0)) for v in PIN_VALUES]    # (pinned axis, travel axis, value)
STRADDLE_EXACT = {0: 0.25, 1: 0.75}     # ray -> a depth at which its travel coordinate is exactly -B / +B

_RAYS = {}


def rays(family, net="coarse", wf="base"):
    """(ro [R, 3], rd [R, 3] float64, ts [R, N] float32) CPU tensors of a family (cached; `box` is BOX_SHAPE, a zero-crossing
    set ZERO_R x N).  Only the zero-crossing sets depend
    on the net and on the function its weights compute."""
    key = (family, net, function_of(wf)) if family in ZERO_SETS else family
    if key not in _RAYS:
        _RAYS[key] = _zero_rays(net, function_of(wf), ZERO_SETS[family]) if family in ZERO_SETS else _t(*_family(family))
    return _RAYS[key]


def _family(family):
    rng = np.random.default_rng(81000 + FAMILIES.index(family))
    if family == "cal":                 # the calibration's distribution: rays between two uniform points of the box, equal steps
        ro, rd, _ = _segments(rng, B, 1 - 2.0 ** -20)
        return ro, rd, np.repeat(np.linspace(0, 1, N, dtype=np.float32)[None], R, 0)
    if family == "ndc-wide":            # the calibration's rays before the box: an NDC frame widened to |x|, |y| <= 2.5, |z| <= 1
        ro = np.concatenate([rng.uniform(-1.5, 1.5, (R, 2)), -np.ones((R, 1))], 1)
        rd = np.concatenate([rng.uniform(-1, 1, (R, 2)), 2 * np.ones((R, 1))], 1)
        return ro, rd, np.repeat(np.linspace(0, 1, N, dtype=np.float32)[None], R, 0)
    if family == "box":
        # the whole box, uniformly: many short rays from a uniform point to one within 0.5 a coordinate of it (kept 2^-20
        # relative inside the faces); the faces themselves: a ray's first sample is its origin where its depth is 0
        Rb, Nb = BOX_SHAPE
        ro = rng.uniform(-B, B, (Rb, 3))
        p1 = np.clip(ro + rng.uniform(-0.5, 0.5, (Rb, 3)), -B * (1 - 2.0 ** -20), B * (1 - 2.0 ** -20))
        ts = np.sort(rng.uniform(0, 1, (Rb, Nb)).astype(np.float32), -1)
        for r in range(6):
            ro[r, r % 3] = B if r < 3 else -B
        ro[6] = (B, -B, B)
        ts[:BOX_FACE_RAYS, 0] = 0.0
        return ro, p1 - ro, ts
    if family in HALF:
        return _segments(rng, HALF[family])
    if family == "far-llff":            # the rays of the per-sample sweep at a forward-facing scene's depths outside NDC
        ro, rd, ts = nk.ray_inputs(R, N)
        return ro.numpy(), rd.numpy(), (2 + 4 * ts.numpy()).astype(np.float32)
    assert family == "straddle"
    # every ray travels one axis from -2 B to +2 B (inside for t in [0.25, 0.75]: 4 B t is exact, so t = 0.25 / 0.75 sit
    # exactly on the face), the other coordinates inside; the pinned rays hold one of those (direction 0: o + t 0 = o exactly)
    # on a face, or one float64 ulp on either side of it
    ro = rng.uniform(-B / 2, B / 2, (R, 3))
    rd = rng.uniform(-B / 4, B / 4, (R, 3))
    ts = np.sort(rng.uniform(0, 1, (R, N)).astype(np.float32), -1)
    n_plain = R - len(STRADDLE_PINS)
    for r in range(R):
        k, a, v = STRADDLE_PINS[r - n_plain] if r >= n_plain else (None, r % 3, None)
        ro[r, a], rd[r, a] = -2 * B, 4 * B
        if k is not None:
            ro[r, k], rd[r, k] = v, 0.0
    for r, t in STRADDLE_EXACT.items():
        ts[r, np.abs(ts[r] - t).argmin()] = t
        ts[r] = np.sort(ts[r])
    return ro, rd, ts


def planted(family):
    """bool [R * N]: the samples put on a face or within an ulp of one on purpose (t d is exact for them: their position is
    the same float64 in numpy and in the kernels)"""
    m = np.zeros(BOX_SHAPE if family == "box" else (R, N), bool)
    if family == "box":
        m[:BOX_FACE_RAYS, 0] = True
    if family == "straddle":
        m[R - len(STRADDLE_PINS):] = True
        ts = rays(family)[2].numpy()
        for r, t in STRADDLE_EXACT.items():
            m[r] |= ts[r] == np.float32(t)
    return m.reshape(-1)


# ------------------------------------------------------------------------------------------------------- zero crossings
ZERO_CANDIDATES, ZERO_GRID, ZERO_BISECTED = 768, 64, 64
ZERO_SPAN = 4.0                         # the float64 densities of a ray's stretch span about +-ZERO_SPAN: the margins are 3..5
ZERO_STATS = {}


def _zero_rays(net, fn, X):
    """ZERO_R rays x N depths around a zero of the float64 density.  Candidate rays start inside the box (X None; direction
    coordinates within +-0.5 around a start within +-(B - 1), so they stay inside) or with one coordinate at +-X (0.97 .. 1.03) and the others in [-X, X]
    (directions within +-max(0.5, X / 8): far out the density changes sign less often per unit of length).  sigma64 is scanned on
    ZERO_GRID depths, the first sign change in [0.1, 0.9] of the first ZERO_BISECTED rays that have one is bisected, the
    stretch t0 +- w sized by the slope there (w = ZERO_SPAN / |dsigma/dt|), and a ray is kept when the float64 densities of
    its N float32 depths (all different) have both signs, a positive share in [0.3, 0.7] and nine in ten within +-8 -- all
    of it chosen from the reference."""
    wf = fn
    rng = np.random.default_rng(82000 + 100 * list(NETS).index(net) + 10 * (fn == "dead") + list(ZERO_SETS.values()).index(X))
    C, G = ZERO_CANDIDATES, ZERO_GRID
    if X is None:
        ro = rng.uniform(-(B - 1), B - 1, (C, 3))
    else:
        ro = rng.uniform(-X, X, (C, 3))
        ax = rng.integers(0, 3, C)
        ro[np.arange(C), ax] = rng.choice([-1.0, 1.0], C) * X * rng.uniform(0.97, 1.03, C)
    rd = rng.uniform(-0.5, 0.5, (C, 3)) * max(1.0, (X or 0.0) / 4)
    s = sigma64(net, wf, (ro[:, None] + np.linspace(0.1, 0.9, G)[None, :, None] * rd[:, None]).reshape(-1, 3)).reshape(C, G)
    scanned = ((s[:, :-1] > 0) != (s[:, 1:] > 0)).any(1)
    first = np.flatnonzero(scanned)[:ZERO_BISECTED]
    ro, rd, s, C = ro[first], rd[first], s[first], len(first)

    def f(t):                           # sigma64 at depth t[c] (or t[c, j]) of candidate c
        t = np.asarray(t, np.float64)
        p = ro[:, None] + t.reshape(C, -1)[..., None] * rd[:, None]
        return sigma64(net, wf, p.reshape(-1, 3)).reshape(t.shape)

    grid = np.linspace(0.1, 0.9, G)
    change = (s[:, :-1] > 0) != (s[:, 1:] > 0)
    has = change.any(1)
    i = change.argmax(1)
    lo, hi = grid[i], grid[i + 1]
    flo = s[np.arange(C), i]
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        fm = f(mid)
        left = (fm > 0) == (flo > 0)
        lo, hi = np.where(left, mid, lo), np.where(left, hi, mid)
    t0 = 0.5 * (lo + hi)
    h = 1e-6
    slope = (f(t0 + h) - f(t0 - h)) / (2 * h)
    with np.errstate(divide="ignore"):
        w = ZERO_SPAN / np.abs(slope)
    ok = has & np.isfinite(w) & (w <= 0.09) & (w >= 2e-5)
    ts = (t0[:, None] + w[:, None] * np.linspace(-1, 1, N)[None]).astype(np.float32)
    ts[~ok] = 0.5
    sig = f(ts.astype(np.float64))
    pos = (sig > 0).mean(1)
    ok &= (pos >= 0.3) & (pos <= 0.7) & ((np.abs(sig) <= 8).mean(1) >= 0.9) & (np.diff(ts, axis=1) > 0).all(1)
    keep = np.flatnonzero(ok)[:ZERO_R]
    assert len(keep) == ZERO_R, "only %d of %d candidate rays of %s / %s / %s have a usable crossing" % (ok.sum(), C, net, fn, X)
    ZERO_STATS[(net, fn, X)] = (int(scanned.sum()), C, int(ok.sum()))
    return _t(ro[keep], rd[keep], ts[keep])


# ------------------------------------------------------------------------------------------------------- case oracle
_REF = {}


def case_rays(case):
    net, wf, fam = case
    return rays(fam, net, wf)


def case_ref(case):
    """float64 densities [R * N] of a case (cached, never written again)"""
    if case not in _REF:
        net, wf, _ = case
        ref = sigma64(net, wf, positions(*case_rays(case)))
        ref.setflags(write=False)
        _REF[case] = ref
    return _REF[case]


def tau(case):
    """The exact kernel's own allowance against float64 on a case, from the project's bars: a sample whose float64 density
    exceeds it is live for the exact kernel too."""
    net, _, _ = case
    top = float(np.abs(case_ref(case)).max())
    return nk.K_X3 * nk.TIGHT["fp16x3"] * top if NETS[net][1] == "fp16x3" else nk.TOL_MX * top


def chain_rays(shape):
    """in-domain rays of the fp16-handle comparison: the per-sample sweep's (|x|, |y| <= 1.3, |z| <= 1)"""
    return nk.ray_inputs(*shape)


# ------------------------------------------------------------------------------------------------------- frames
def frame_extent(H=400, W=400, poses=range(120)):
    """largest |coordinate| of the NDC frame rays of the benchmark and of the tests' fern orbit at t in [0, 1] (o + t d is
    linear in t: the extremes are at the ends), from the oracle's ray generator"""
    from oracle import rays as orays
    top = 0.0
    for i in poses:
        o, d = orays.frame_rays_ndc(H, W, synth.fern_intrinsics(H, W), synth.spiral_pose(i))
        top = max(top, float(np.abs(o).max()), float(np.abs(o + d).max()))
    return top


# ------------------------------------------------------------------------------------------------------- fp16 model
def model_error(net, wf, pts):
    """|sigma_model - sigma64| of a plain model of the screen (fp16 operands, products summed in float64, no equalisation) on
    [M, 3] positions: for the record only, nothing is asserted on it"""
    from oracle import fields
    sd = state(net, wf)
    h16 = lambda x: x.astype(np.float16).astype(np.float64)
    W = lambda n: sd["net." + n + ".weight"].astype(np.float64)
    b = lambda n: sd["net." + n + ".bias"].astype(np.float64)
    lin = lambda a, n: h16(a) @ h16(W(n)).T + b(n)
    pe = fields.posenc(torch.as_tensor(pts, dtype=torch.float64), 10).numpy()
    with np.errstate(over="ignore", invalid="ignore"):
        h = np.maximum(lin(pe, "base_layers.0"), 0)
        for i in range(7):
            h = np.maximum(lin(np.concatenate([pe, h], 1) if i == 4 else h, "base_layers.%d" % (i + 1)), 0)
        return np.abs(lin(h, "sigma_layer")[:, 0] - sigma64(net, wf, pts))
