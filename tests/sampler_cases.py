"""Test helper: the cases of the sampler shape sweep (tests/test_sampler_shapes_cpu.py, _gpu.py) -- shapes, depth rows, weight
families, the density planes that make a compositor produce them -- and thin wrappers around the oracle's sampler
(oracle.raymarch.sample_fine) and the acceptance test (conditioning.sampler_bound).

The stand-alone samplers tgtc_sample_fine / tgtc_coarse_to_fine (csrc/raypath.hip) accept 3 <= N <= 256, 1 <= n_fine and
N + n_fine <= 512.  What depends on the shape in them: C = ceil((N - 2) / 64) pdf entries per lane in the blocked float64 cdf
scan, the 64-lane strides over N, N - 1, N - 2 and n_fine, the rank sort over T = N + n_fine, and the two merge binary
searches of coarse_to_fine_kernel.  Each shape below is the smallest of something in that list ("The
sampler shape sweep").

No fixtures and no GPU here: numpy / torch CPU only."""
import numpy as np
import torch

import conditioning
from oracle import raymarch

R = 9                       # coarse_to_fine_kernel takes four rays per workgroup: two full workgroups and a tail of one
MAX_N, MAX_TOTAL = 256, 512   # kFineMaxN, kFineMaxTotal (csrc/raypath.hip)

# (N, n_fine)
SHAPES = [
    (3, 1),        # one pdf entry, one new sample: u = linspace(0, 1, 1) = [0]
    (3, 2),        # one pdf entry, u = [0, 1]
    (4, 1),        # two pdf entries, one new sample
    (16, 16),      # 14 pdf entries on 64 lanes
    (65, 64),      # 63 pdf entries: one lane of the scan owns none; 64 bins on 64 lanes
    (66, 64),      # 64 pdf entries: the last N with C = 1
    (67, 5),       # 65: the first with C = 2
    (100, 28),     # a shape the renders use (tests/test_restyle_gpu.py)
    (130, 3),      # 128: the last with C = 2
    (131, 64),     # 129: the first with C = 3
    (194, 62),     # 192: the last with C = 3; T = 256
    (195, 7),      # 193: the first with C = 4
    (256, 1),      # N maximum, one new sample
    (256, 256),    # both limits: N = 256, T = 512
]

FAMILIES = [
    "pow6",        # uniform ** 6: a few samples carry the ray
    "zero",        # all zero: uniform pdf
    "onehot",      # 1 at a random interior sample
    "ends",        # weight only at sample 0 and N - 1, which the pdf drops: uniform pdf again
    "spikes",      # samples 1 and N - 2: the first and the last pdf entry
    "tiny",        # uniform * 1e-7: below the 1e-5 floor
    "const",       # a constant
]
UNIFORM_PDF = ["zero", "const"]     # the families whose pdf is uniform by construction (the 1e-6 comparison)

ASCENDING = ["linspace", "jittered", "ties"]
DEPTHS = ASCENDING + ["descending"]
DESC_ROW = 4                # the one row of "descending" whose coarse depths descend


def pdf_per_lane(N):
    """C of sample_fine_kernel / coarse_to_fine_kernel: pdf entries per lane of the blocked cdf scan."""
    return (N - 2 + 63) // 64


def case_id(N, NF, fam, dkind):
    return "%d+%d-%s-%s" % (N, NF, fam, dkind)


# ------------------------------------------------------------------------------------------------------- inputs
def depth_rows(kind, N, rng):
    """[R, N] float32 coarse depths: "linspace" the same row for all rays, "jittered" ascending with a random offset per
    sample, "ties" with repeated coarse depths (pairs and, from N = 16 on, one triple per ray), "descending" = jittered with
    row DESC_ROW reversed."""
    lin = np.linspace(0.0, 1.0, N, dtype=np.float32)
    if kind == "linspace":
        return np.tile(lin, (R, 1))
    jit = np.sort(lin[None, :] + rng.uniform(-0.4, 0.4, (R, N)).astype(np.float32) / N, axis=1).astype(np.float32)
    if kind == "jittered":
        return jit
    if kind == "ties":
        ts = jit.copy()
        ts[:, 1] = ts[:, 0] if N > 3 else ts[:, 2]
        for k in range(5, N - 2, 7):
            ts[:, k] = ts[:, k - 1]
        if N >= 16:
            ts[:, N // 2] = ts[:, N // 2 + 1] = ts[:, N // 2 - 1]
        return ts
    ts = jit.copy()
    ts[DESC_ROW] = ts[DESC_ROW, ::-1]
    return ts


def weights(fam, N, rng):
    """[R, N] float32 in [0, 1]."""
    u = rng.uniform(0.0, 1.0, (R, N))
    w = np.zeros((R, N))
    if fam == "pow6":
        w = u ** 6
    elif fam == "onehot":
        w[np.arange(R), rng.integers(1, N - 1, R)] = 1.0
    elif fam == "ends":
        w[:, 0], w[:, N - 1] = 0.3, 0.7
    elif fam == "spikes":
        w[:, 1] = 0.5
        w[:, N - 2] = w[:, N - 2] + 0.4        # N = 3: one sample carries both
    elif fam == "tiny":
        w = u * 1e-7
    elif fam == "const":
        w[:] = 0.25
    return w.astype(np.float32)


def sigma_for(w, ts, rng):
    """[R, N] float32 densities under which a compositor (utils.py:354-386) gives weights proportional to `w` on the depths
    `ts`: rows are scaled to a sum of at most 0.95, then alpha_i = w_i / T_i and sigma_i = -log(1 - alpha_i) / delta_i,
    computed in float64.  Where the target is 0 the density is negative or a signed zero; where delta_i <= 0 (a tie, the
    descending row) no density gives a weight and it is 0.  The weights a test feeds are those a compositor then returns,
    never `w` itself."""
    w = w.astype(np.float64)
    w = w * np.minimum(1.0, 0.95 / np.maximum(w.sum(1, keepdims=True), 1e-30))
    delta = np.concatenate([ts[:, 1:].astype(np.float64) - ts[:, :-1], np.full((R, 1), 1e10)], 1)
    dead = -np.abs(rng.standard_normal(w.shape) * 3.0)
    dead[:, ::3] = 0.0
    dead[:, 1::5] = -0.0
    sigma, trans = dead.copy(), np.ones(R)
    for i in range(w.shape[1]):
        alpha = np.minimum(w[:, i] / trans, 1.0 - 1e-9)
        live = (w[:, i] > 0) & (delta[:, i] > 0)
        sigma[live, i] = (-np.log1p(-alpha[live]) / delta[live, i])
        trans = np.where(live, trans * (1.0 - alpha), trans)
    return sigma.astype(np.float32)


_inputs = {}


def inputs(N, NF, fam, dkind):
    """The inputs of a case as CPU tensors, computed once and never modified: ts [R, N] coarse depths, w [R, N] the family's
    weights (what tgtc_sample_fine is fed), sigma [R, N] the densities of sigma_for (what tgtc_composite and
    tgtc_coarse_to_fine are fed), w_comp [R, N] the float32 oracle compositor's weights on (sigma, ts), and rays o, d
    [R, 3] float64 -- an origin of magnitude 1e3, directions with negative and zero components."""
    key = (N, NF, fam, dkind)
    if key not in _inputs:
        rng = np.random.default_rng(100000 * N + 100 * NF + 10 * FAMILIES.index(fam) + DEPTHS.index(dkind))
        ts = depth_rows(dkind, N, rng)
        w = weights(fam, N, rng)
        sigma = sigma_for(w, ts, rng)
        o = rng.uniform(-1.0, 1.0, (R, 3)) * 1e3
        d = rng.uniform(-1.0, 1.0, (R, 3))
        d[::3, 0], d[1::3, 1], d[2::3, 2] = 0.0, -0.0, -np.abs(d[2::3, 2])
        t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in dict(ts=ts, w=w, sigma=sigma, o=o, d=d).items()}
        t["w_comp"] = raymarch.composite(torch.zeros(R, N, 3), t["sigma"], t["ts"])[2]
        _inputs[key] = t
    return _inputs[key]


# ------------------------------------------------------------------------------------------------------- oracle
def oracle_depths(ts, w, NF, dtype=torch.float64):
    """oracle.raymarch.sample_fine's merged depths [r, N + NF] of (ts, w) evaluated in `dtype`."""
    z = torch.zeros(ts.shape[0], 3, dtype=torch.float64)
    return raymarch.sample_fine(z, z, ts.to(dtype), w.to(dtype), NF)[1]


def oracle_new(ts, w, NF, dtype=torch.float64):
    """The oracle's NF new depths alone, in the order of u (also on a row that is not ascending)."""
    ts, w = ts.to(dtype), w.to(dtype)
    return raymarch.inverse_cdf(0.5 * (ts[..., 1:] + ts[..., :-1]), w[..., 1:-1], NF)


def bound(ts, w, ts_out, NF):
    """conditioning.sampler_bound at its default delta (4e-6, the project's number): the excess per ray, 0 = admissible."""
    return conditioning.sampler_bound(ts, w, ts_out, NF)


def whole_bin(w, NF):
    """[r, NF] bool: the samples whose admissible interval under sampler_bound is a whole bin -- the float64 cdf step of the
    bin that u_j falls into is below 2e-5."""
    p = w.double().numpy()[:, 1:-1] + 1e-5
    cdf = np.concatenate([np.zeros((p.shape[0], 1)), np.cumsum(p / p.sum(1, keepdims=True), 1)], 1)
    u = np.linspace(0.0, 1.0, NF)
    out = np.empty((p.shape[0], NF), bool)
    for r in range(p.shape[0]):
        k = np.clip(np.searchsorted(cdf[r], u, side="right") - 1, 0, p.shape[1] - 1)
        out[r] = (cdf[r, k + 1] - cdf[r, k]) < 2e-5
    return torch.from_numpy(out)


def descending_rows_with_one_answer():
    """[(N, n_fine, family)]: the "descending" cases on whose row DESC_ROW the float32 and the float64 oracle's new depths
    agree to 1e-6, i.e. where one oracle output can be the yardstick of that row."""
    rows = []
    for N, NF in SHAPES:
        for fam in FAMILIES:
            x = inputs(N, NF, fam, "descending")
            r = slice(DESC_ROW, DESC_ROW + 1)
            d = oracle_new(x["ts"][r], x["w"][r], NF, torch.float32).double() - oracle_new(x["ts"][r], x["w"][r], NF)
            if float(d.abs().max()) <= 1e-6:
                rows.append((N, NF, fam))
    return rows


def new_depth_intervals(ts, w, NF, delta=4e-6):
    """For ONE ray (ts [N], w [N]) whose depths need not ascend: (lo [NF], hi [NF]) float64, sorted each, between which the
    ray's sorted new depths must lie.  The statement of conditioning.sampler_bound with its delta, reduced to what an
    unsorted row allows: a sample whose u is within delta of a bin with a cdf step below 2e-5 may lie anywhere in the bins u
    can fall into; every other sample is the float64 oracle's, to 1e-6."""
    t, p = ts.double().numpy(), w.double().numpy()[1:-1] + 1e-5
    mid = 0.5 * (t[1:] + t[:-1])
    cdf = np.concatenate([[0.0], np.cumsum(p / p.sum())])
    new = oracle_new(ts[None], w[None], NF)[0].numpy()
    lo, hi = new - 1e-6, new + 1e-6
    for j, u in enumerate(np.linspace(0.0, 1.0, NF)):
        k = np.nonzero((cdf[:-1] - delta <= u) & (u <= cdf[1:] + delta))[0]
        if k.size and float((cdf[k + 1] - cdf[k]).min()) < 2e-5:
            edges = np.concatenate([mid[k], mid[k + 1], new[j:j + 1]])
            lo[j], hi[j] = edges.min() - 1e-6, edges.max() + 1e-6
    return np.sort(lo), np.sort(hi)


def without(merged, coarse):
    """The sorted list `merged` [T] minus the multiset `coarse` [N], each coarse depth taken out once, bit for bit; None if one
    is missing."""
    rest = merged.tolist()
    for v in coarse.tolist():
        if v not in rest:
            return None
        rest.remove(v)
    return np.asarray(rest, np.float64)
