#!/usr/bin/env python3
"""Timing of the folded restyle from a trunk plane with the style networks in fp16mx: the frame, pose, shapes and schedule of
tools/time_restyle_trunk.py (400x400 fern-shaped, pose 5, R = 160 000, 128c + 64f, fp16x3 nets), one geometry cache with its
fp16x3 plane, K in {1, 2, 4} frame-constant latents (zs [K,32]).

    A = RayRenderer.restyle(cache, ...)                             (tgtc_restyle_rays_trunk_folded: three fp16 MFMA products per
                                                                     algorithmic product)
    B = RayRenderer.restyle(cache, ..., style_precision="fp16mx")   (tgtc_restyle_rays_trunk_folded_mx: per 128-deep block four
                                                                     fp16 and two block-scaled fp6 MFMAs instead of twelve)

Same process, A and B alternating, both warmed up (B's streams are packed in the warm-up), device events around RENDERS
restyles each, ROUNDS A/B rounds so that the spread of A against itself is known.  A is the path this mode leaves alone: it
is compared with the folded fp16x3 rows of profiles/restyle_trunk_timing.json.  B's image is checked against A's at
TIGHT["fp16x3"] + 1e-3 (tests/test_restyle_mx_gpu.py).  The claim, at each K: every B below every A, by more than A's spread.

Prints and writes profiles/restyle_trunk_mx_timing.json.  Needs a GPU: there is no fallback."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tgtc_style_amd import rendering, synth, utils  # noqa: E402

H = W = 400
NC, NF = 128, 64
KS = (1, 2, 4)
ROUNDS, RENDERS = 3, 5
IMAGE_BAR = 5e-5 + 1e-3
# MFMA issue slots per row tile of a layer: K blocks at 12 (fp16x3) / 6 (fp16mx), encoding k-steps at 3 in both
SLOTS_X3 = sum(rt * (12 * nkb + 3 * npe) for rt, nkb, npe in
               [(16, 0, 2), (16, 2, 0), (16, 2, 0), (16, 2, 0), (16, 2, 2), (16, 4, 2)] + [(16, 2, 0)] * 3 + [(16, 2, 2)] +
               [(16, 2, 0)] * 2 + [(1, 2, 0)])
SLOTS_MX = sum(rt * (6 * nkb + 3 * npe) for rt, nkb, npe in
               [(16, 0, 2), (16, 2, 0), (16, 2, 0), (16, 2, 0), (16, 2, 2), (16, 4, 2)] + [(16, 2, 0)] * 3 + [(16, 2, 2)] +
               [(16, 2, 0)] * 2 + [(1, 2, 0)])


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(RENDERS):
        out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / RENDERS, out


def measure(r, cache, o, d, z, parent_row):
    K = z.shape[0]
    run_a = lambda: r.restyle(cache, o, d, z)
    run_b = lambda: r.restyle(cache, o, d, z, style_precision="fp16mx")
    for _ in range(2):      # warm-up of both (workspace, code objects, B's streams)
        a_out, b_out = run_a(), run_b()
    torch.cuda.synchronize()
    diff = float((a_out["rgb"] - b_out["rgb"]).abs().max())
    assert torch.equal(b_out["t"], a_out["t"]) and diff <= IMAGE_BAR, "B is not A's image within the bar: %g" % diff
    a_ms, b_ms = [], []
    for _ in range(ROUNDS):
        a_ms.append(timed(run_a)[0])
        b_ms.append(timed(run_b)[0])
    a, b = sum(a_ms) / ROUNDS, sum(b_ms) / ROUNDS
    rec = {"A_ms": a_ms, "B_ms": b_ms, "A_ms_mean": a, "B_ms_mean": b, "B_over_A": b / a,
           "A_spread_rel": (max(a_ms) - min(a_ms)) / a, "B_spread_rel": (max(b_ms) - min(b_ms)) / b,
           "every_B_below_every_A_by_more_than_A_spread": min(a_ms) - max(b_ms) > max(a_ms) - min(a_ms),
           "predicted_B_over_A_by_mfma_slots": SLOTS_MX / SLOTS_X3, "image_max_abs_diff": diff,
           "B_rays_x_latents_per_s": cache.R * K / b * 1e3}
    if parent_row is not None:
        rec["A_ms_mean_in_restyle_trunk_timing_json"] = parent_row["B_ms_mean"]
        rec["A_over_that"] = a / parent_row["B_ms_mean"]
    print("  K=%d  A (fp16x3) %7.2f ms [%s]   B (fp16mx) %7.2f ms [%s]   B/A %.3f (MFMA slots: %.3f)   spread of A %.2f %%   "
          "image diff %.2e%s" % (K, a, " ".join("%.2f" % x for x in a_ms), b, " ".join("%.2f" % x for x in b_ms), b / a,
                                 SLOTS_MX / SLOTS_X3, 100 * rec["A_spread_rel"], diff,
                                 "   A / recorded A %.3f" % rec["A_over_that"] if parent_row is not None else ""), flush=True)
    return rec


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_restyle_trunk_mx: no GPU visible; there is nothing to time without one")
    o, d = utils.gen_rays(H, W, synth.fern_intrinsics(H, W), synth.spiral_pose(5))
    r = bench.make_renderer("fp16x3", True)
    r = rendering.RayRenderer(r.coarse, r.fine, style=r.style)
    R = o.shape[0]
    gen = torch.Generator(device="cuda").manual_seed(1)
    zs_all = torch.randn(max(KS), R, 32, device="cuda", generator=gen)      # the latents of tools/time_restyle_trunk.py
    cache = r.build_geometry(o, d, NC, NF, min_weight=0., keep_trunk=True)
    parent = None
    try:
        with open(os.path.join(ROOT, "profiles", "restyle_trunk_timing.json")) as f:
            parent = json.load(f)["per_precision"]["fp16x3"]["folded"]
    except (OSError, KeyError, ValueError):
        pass
    result = {"frame": [H, W], "pose": 5, "rays": R, "n_coarse": NC, "n_fine": NF, "rounds": ROUNDS,
              "renders_per_measurement": RENDERS, "device": torch.cuda.get_device_name(0), "live_samples": cache.count,
              "A": "restyle(zs [K,32]) from the plane, fp16x3", "B": "restyle(zs [K,32], style_precision='fp16mx') from the plane",
              "mfma_slots_per_latent": {"fp16x3": SLOTS_X3, "fp16mx": SLOTS_MX}, "K": {}}
    print("live %d of %d; plane %d bytes" % (cache.count, R * (NC + NF), cache.trunk.numel()), flush=True)
    for K in KS:
        result["K"][str(K)] = measure(r, cache, o, d, zs_all[:K, 0].contiguous(), parent[str(K)] if parent else None)
    result["claim_holds_at_every_K"] = all(v["every_B_below_every_A_by_more_than_A_spread"] for v in result["K"].values())
    print("every B below every A by more than A's spread, at every K:", result["claim_holds_at_every_K"])

    out_path = os.path.join(ROOT, "profiles", "restyle_trunk_mx_timing.json")
    if len(sys.argv) > 1:
        out_path = sys.argv[1]
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
