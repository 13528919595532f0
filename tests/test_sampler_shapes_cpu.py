"""CPU: what the sampler shape sweep (tests/test_sampler_shapes_gpu.py) rests on, from the oracle alone.

The GPU tests accept a kernel's merged depths where conditioning.sampler_bound has excess 0 on them: a point tolerance against
one oracle output cannot do that job, the float32 and the float64 oracle differ by up to a bin on the one-hot and uniform ** 6
weights (the reference is discontinuous there, tests/conditioning.py).  That is a sound acceptance test only if

  a. it is exact on correct input: on every case, with the very weights the GPU tests feed, the float32 and the float64
     oracle both have excess 0 at the default delta; and
  b. it is sharp: a sampler that is wrong in one place -- CPU variants of the oracle's sampler with one change each -- gets
     excess > 0 on at least one case of the list.  One listed change, searchsorted(right=False), is inside the bound on every
     input there can be; test_searchsorted_left_is_inside_the_bound_by_construction asserts the reason.

Both are asserted here, and (c) that the case list holds the shapes it was written for."""
import numpy as np
import pytest
import torch

import sampler_cases as sc

CASES = [(N, NF, fam, dkind) for N, NF in sc.SHAPES for fam in sc.FAMILIES for dkind in sc.ASCENDING]
# A bin with a cdf step below 2e-5 is one of at most N - 2 <= 254: together they cover 0.5 % of the range of u, and beyond that
# only the two end samples of a ray, u = 0 and u = 1, sit on the edge of one: 2 x 5292 rays of the 216972 pairs, 4.9 %.
WHOLE_BIN_MAX = 0.06


# ------------------------------------------------------------------------------------------------------- c
def test_case_list_covers_the_shape_edges():
    """If kFineMaxN / kFineMaxTotal (csrc/raypath.hip) or the lane count of the blocked scan change, update MAX_N /
    MAX_TOTAL / pdf_per_lane and SHAPES of tests/sampler_cases.py with them."""
    shapes = set(sc.SHAPES)
    assert len(shapes) == len(sc.SHAPES)
    for N, NF in shapes:
        assert 3 <= N <= sc.MAX_N and 1 <= NF and N + NF <= sc.MAX_TOTAL
    # every C, and both sides of every boundary: the last N with C - 1 entries per lane and the first with C
    assert {sc.pdf_per_lane(N) for N, _ in shapes} == {1, 2, 3, 4}
    for C in (2, 3, 4):
        first = 64 * (C - 1) + 3
        assert sc.pdf_per_lane(first) == C and sc.pdf_per_lane(first - 1) == C - 1
        assert any(N == first for N, _ in shapes) and any(N == first - 1 for N, _ in shapes), C
    assert any(N - 2 == 63 for N, _ in shapes)                        # one lane of the scan without an entry
    assert min(shapes) == (3, 1) and (sc.MAX_N, sc.MAX_TOTAL - sc.MAX_N) in shapes and (sc.MAX_N, 1) in shapes
    assert {N for N, NF in shapes if NF == 1} >= {3, 4, sc.MAX_N}     # n_fine = 1: u = [0]
    totals = {N + NF for N, NF in shapes}
    assert {256, 512} <= totals                                       # the rank sort: four and eight full strides
    assert any(NF > 192 for _, NF in shapes) and any(NF % 64 for _, NF in shapes)      # the 64-lane stride over n_fine
    assert (100, 28) in shapes
    assert sc.R % 4 == 1 and sc.R > 8                                 # two workgroups of coarse_to_fine_kernel and a tail
    assert 0 <= sc.DESC_ROW < sc.R


def test_inputs_are_what_the_families_say():
    for N, NF in sc.SHAPES:
        for fam in sc.FAMILIES:
            for dkind in sc.DEPTHS:
                x = sc.inputs(N, NF, fam, dkind)
                ts, w, wc = x["ts"], x["w"], x["w_comp"]
                assert ts.dtype == w.dtype == wc.dtype == x["sigma"].dtype == torch.float32
                assert float(w.min()) >= 0.0 and float(w.max()) <= 1.0
                assert bool(torch.isfinite(wc).all()) and float(wc.min()) >= 0.0 and float(wc.max()) <= 1.0
                asc = [r for r in range(sc.R) if not (dkind == "descending" and r == sc.DESC_ROW)]
                assert bool((ts[asc, 1:] >= ts[asc, :-1]).all())
                if dkind == "descending":
                    assert bool((ts[sc.DESC_ROW, 1:] <= ts[sc.DESC_ROW, :-1]).all())
                if fam in ("zero", "ends"):
                    assert float(w[:, 1:-1].abs().max()) == 0.0 and float(wc[:, 1:-1].abs().max()) == 0.0
                if fam == "onehot":
                    assert bool(((w == 1.0).sum(1) == 1).all()) and float(w[:, 0].max()) == 0.0 == float(w[:, -1].max())
                if fam == "tiny":
                    assert 0.0 < float(w.max()) < 1e-5
                if fam in ("pow6", "onehot", "spikes", "const") and dkind in ("linspace", "jittered"):
                    # the densities of sigma_for give the family back, scaled: the compositor's weights are w * s per ray
                    s = (wc.double() * w.double()).sum(1) / (w.double() ** 2).sum(1)
                    assert float((wc.double()[:, :-1] - s[:, None] * w.double()[:, :-1]).abs().max()) <= 1e-6
        o, d = x["o"], x["d"]
        assert float(o.abs().max()) > 500.0 and bool((d == 0).any()) and bool((d < 0).any())


# ------------------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("N,NF", sc.SHAPES, ids=["%d+%d" % s for s in sc.SHAPES])
def test_the_bound_accepts_both_oracles(N, NF):
    """sampler_bound == 0 for the float32 and the float64 oracle on every family x ascending depth kind of the shape, on the
    family's own weights (the input of tgtc_sample_fine) and on the compositor's (the input of tgtc_coarse_to_fine)."""
    apart = 0.0
    for fam in sc.FAMILIES:
        for dkind in sc.ASCENDING:
            x = sc.inputs(N, NF, fam, dkind)
            for wkey in ("w", "w_comp"):
                outs = [sc.oracle_depths(x["ts"], x[wkey], NF, dtype) for dtype in (torch.float32, torch.float64)]
                apart = max(apart, float((outs[0].double() - outs[1]).abs().max()))
                for out in outs:
                    e = sc.bound(x["ts"], x[wkey], out, NF)
                    assert float(e.max()) == 0.0, (sc.case_id(N, NF, fam, dkind), wkey, out.dtype, e.tolist())
    print("%d+%d: excess 0 on %d cases x 2 weight planes x 2 oracles, which are up to %.1e apart" % (
        N, NF, len(sc.FAMILIES) * len(sc.ASCENDING), apart))


def test_the_bound_is_not_met_by_being_empty():
    """The share of (case, sample) pairs whose admissible interval is a whole bin (den < 2e-5), over both weight planes.
    Whole bins are the nature of the one-hot, the spikes and the uniform ** 6 rows -- most of their bins carry 1e-5 of a pdf
    whose sum is O(1) -- and absent from the families with a uniform pdf."""
    whole = {fam: 0 for fam in sc.FAMILIES}
    total = dict(whole)
    for N, NF, fam, dkind in CASES:
        x = sc.inputs(N, NF, fam, dkind)
        for wkey in ("w", "w_comp"):
            wb = sc.whole_bin(x[wkey], NF)
            whole[fam], total[fam] = whole[fam] + int(wb.sum()), total[fam] + wb.numel()
    share = sum(whole.values()) / sum(total.values())
    print("whole-bin share %.1f %% of %d (case, sample) pairs; by family: %s" % (
        100.0 * share, sum(total.values()), ", ".join("%s %.1f %%" % (f, 100.0 * whole[f] / total[f]) for f in sc.FAMILIES)))
    for fam in ("zero", "ends", "tiny"):
        assert whole[fam] == 0, fam
    assert share <= WHOLE_BIN_MAX, share


# ------------------------------------------------------------------------------------------------------- b
def variant_depths(ts, w, NF, variant):
    """oracle.raymarch.sample_fine in float32 with ONE change."""
    mid = 0.5 * (ts[..., 1:] + ts[..., :-1])
    wi = w[..., :-2] if variant == "weights_shifted" else w[..., 1:-1]
    wi = wi + 1e-5
    pdf = wi / wi.sum(-1, keepdim=True)
    if variant == "scan_drops_entry_64" and pdf.shape[-1] > 64:        # the first entry of a lane of the blocked scan
        pdf = pdf.clone()
        pdf[..., 64] = 0.0
    cdf = torch.cumsum(pdf, -1)
    if variant == "cdf_without_leading_zero":
        cdf = torch.cat([cdf, cdf[..., -1:]], -1)                      # same length, shifted by one entry
    else:
        cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    u = torch.linspace(0., 1., NF + 1)[:-1] if variant == "u_open_interval" else torch.linspace(0., 1., NF)
    u = u.expand(list(cdf.shape[:-1]) + [NF]).contiguous()
    idx = torch.searchsorted(cdf, u, right=variant != "searchsorted_left")
    lo, hi = (idx - 1).clamp(min=0), idx.clamp(max=cdf.shape[-1] - 1)
    c_lo, c_hi = torch.gather(cdf, -1, lo), torch.gather(cdf, -1, hi)
    b_lo, b_hi = torch.gather(mid, -1, lo), torch.gather(mid, -1, hi)
    den = c_hi - c_lo
    if variant != "no_small_den_rule":
        den = torch.where(den < 1e-5, torch.ones_like(den), den)
    new = b_lo + (u - c_lo) / den * (b_hi - b_lo)
    return torch.sort(torch.cat([ts, new], -1), -1)[0], new


def test_the_unchanged_variant_is_the_oracle():
    for N, NF, fam, dkind in CASES[::5]:
        x = sc.inputs(N, NF, fam, dkind)
        assert torch.equal(variant_depths(x["ts"], x["w"], NF, None)[0], sc.oracle_depths(x["ts"], x["w"], NF, torch.float32))


def excess(x, out, NF):
    """What the GPU tests assert of a kernel's depths: finite, and sampler_bound == 0.  (A NaN compares false with either
    end of its interval, so the bound alone lets it pass: the finiteness assertion beside it is part of the check.)"""
    if not bool(torch.isfinite(out).all()):
        return float("inf")
    return float(sc.bound(x["ts"], x["w"], out, NF).max())


# variant -> the cases tried first, so that the test ends at the first catch: the one written next to the variant in DESIGN.md
WRONG = {
    "weights_shifted": (16, 16, "onehot"),
    "no_small_den_rule": (3, 2, "zero"),
    "cdf_without_leading_zero": (16, 16, "zero"),
    "u_open_interval": (3, 2, "zero"),
    "scan_drops_entry_64": (67, 5, "spikes"),       # entry 64 of 65 is the first of lane 32 at C = 2, and the last pdf entry
}


@pytest.mark.parametrize("variant", list(WRONG))
def test_the_check_rejects_a_subtly_wrong_sampler(variant):
    first = [c for c in CASES if c[:3] == WRONG[variant]]
    assert first
    for N, NF, fam, dkind in first + [c for c in CASES if c[:3] != WRONG[variant]]:
        x = sc.inputs(N, NF, fam, dkind)
        e = excess(x, variant_depths(x["ts"], x["w"], NF, variant)[0], NF)
        if e > 0.0:
            print("%s: caught on %s, excess %.2e" % (variant, sc.case_id(N, NF, fam, dkind), e))
            assert (N, NF, fam) == WRONG[variant], "caught, but not where DESIGN.md section 4 says: update its table"
            return
    raise AssertionError("%s escapes every case" % variant)


def test_searchsorted_left_is_inside_the_bound_by_construction():
    """searchsorted(right=False) is the one listed change that NO input can make the bound reject, and the reason is the
    statement of tests/conditioning.py itself.  The two searches differ only where u equals a cdf entry, cdf[k], bit for bit.
    There right=True interpolates in bin k at position 0 and returns its lower edge mid[k]; right=False interpolates in bin
    k - 1 at position (cdf[k] - cdf[k-1]) / den = 1 and returns the same mid[k] -- unless den < 1e-5, where den := 1 pins the
    sample near mid[k-1], one bin lower.  But u is then on the edge of a bin whose cdf step is below 1e-5, and the bound
    admits the whole of such a bin (den < 2e-5), as it must: a cdf one ulp higher moves the reference's own sample there.
    Asserted: the variant does differ from the oracle, by whole bins; every sample that moves by more than 1e-6 has u on a
    float32 cdf entry and a step below 1e-5 beneath it; the excess is 0 everywhere."""
    moved = 0
    for N, NF, fam, dkind in CASES:
        x = sc.inputs(N, NF, fam, dkind)
        out, new = variant_depths(x["ts"], x["w"], NF, "searchsorted_left")
        ref_out, ref_new = variant_depths(x["ts"], x["w"], NF, None)
        far = (new - ref_new).abs() > 1e-6
        if bool(far.any()):
            p = x["w"][:, 1:-1] + 1e-5
            cdf = torch.cat([torch.zeros(sc.R, 1), torch.cumsum(p / p.sum(-1, keepdim=True), -1)], -1)
            u = torch.linspace(0., 1., NF).expand(sc.R, NF).contiguous()
            k = torch.searchsorted(cdf, u, right=False).clamp(min=1, max=cdf.shape[-1] - 1)
            on_entry = torch.gather(cdf, -1, k) == u
            step = torch.gather(cdf, -1, k) - torch.gather(cdf, -1, k - 1)
            assert bool((on_entry & (step < 1e-5))[far].all()), sc.case_id(N, NF, fam, dkind)
            moved += int(far.sum())
        if not torch.equal(out, ref_out):
            assert excess(x, out, NF) == 0.0, sc.case_id(N, NF, fam, dkind)
    print("searchsorted(right=False): %d samples move by more than 1e-6, all on a cdf entry above a step < 1e-5; excess 0" % moved)
    assert moved > 0


# ------------------------------------------------------------------------------------------------------- descending rows
def test_the_oracle_agrees_with_itself_on_descending_rows():
    """The GPU test of the descending row compares with the float64 oracle where the float32 oracle is within 1e-6 of it:
    that must leave rows, of every shape."""
    rows = sc.descending_rows_with_one_answer()
    print("descending rows on which the float32 and the float64 oracle agree to 1e-6: %d of %d" % (
        len(rows), len(sc.SHAPES) * len(sc.FAMILIES)))
    assert {(N, NF) for N, NF, _ in rows} == set(sc.SHAPES)
    assert {fam for _, _, fam in rows} >= {"zero", "ends", "tiny", "const"}
    # and on those rows both oracles pass what the GPU test asks of the kernel
    bins = 0
    for N, NF, fam in rows:
        x, r = sc.inputs(N, NF, fam, "descending"), sc.DESC_ROW
        lo, hi = sc.new_depth_intervals(x["ts"][r], x["w"][r], NF)
        bins += int((hi - lo > 1e-5).sum())
        for dtype in (torch.float32, torch.float64):
            new = sc.without(sc.oracle_depths(x["ts"][r:r + 1], x["w"][r:r + 1], NF, dtype)[0], x["ts"][r].to(dtype))
            assert new is not None and len(new) == NF
            assert float(np.maximum(lo - new, new - hi).max()) <= 0.0, (N, NF, fam, dtype)
    print("of their %d new samples %d may lie anywhere in a bin" % (sum(NF for _, NF, _ in rows), bins))
