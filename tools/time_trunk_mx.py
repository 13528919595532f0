#!/usr/bin/env python3
"""Timing of the trunk plane from an fp16mx fine network: the frame, pose, shapes and schedule of tools/time_restyle_trunk.py
(400x400 fern-shaped, pose 5, R = 160 000, 128c + 64f), ONE geometry cache, built by the headline pair fp16x3+fp16mx, so that both
producers walk the same list.

    A = RayRenderer.build_trunk(cache, ...)                            from the fine weights packed in fp16x3
                                                                       (tgtc_geometry_trunk: the path this mode leaves alone)
    B = RayRenderer.build_trunk(cache, ..., trunk_precision="fp16x3")  from the same weights packed in fp16mx
                                                                       (tgtc_geometry_trunk_mx, csrc/mlp_trunk_mx.hip)

Same process, A and B alternating on the same cache (each build attaches its plane in place of the other's), after a warm-up
that leaves the allocator holding a plane, device events around RENDERS builds each, ROUNDS A/B rounds so that the spread of A
against itself is known.  B counts as faster only if every B round is below every A round by more than A's spread.  The
prediction is by MFMA issue slots per row tile: a 128-deep block costs 12 in fp16x3 and 6.15 in fp16mx (csrc/mlp_mx.h), an
encoding k-step 3 in both.

Then, per K in {1, 2, 4} frame-constant latents, the restyle with style_precision="fp16mx" from plane B and from plane A (the
consumer reads bytes: no difference is expected), and the image difference max |A - B| of the two planes under the fp16x3 and
the fp16mx style networks.

Prints and writes profiles/trunk_mx_timing.json.  Needs a GPU: there is no fallback."""
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
# (row tiles, 128-deep blocks, encoding k-steps) of the trunk: layers 0-7, the sigma layer, base_remap_layer
TRUNK = [(16, 0, 2)] + [(16, 2, 0)] * 4 + [(16, 2, 2)] + [(16, 2, 0)] * 2 + [(1, 2, 0), (16, 2, 0)]
SLOTS_X3 = sum(rt * (12 * nkb + 3 * npe) for rt, nkb, npe in TRUNK)
SLOTS_MX = sum(rt * (6.15 * nkb + 3 * npe) for rt, nkb, npe in TRUNK)


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(RENDERS):
        out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / RENDERS, out


def interleaved(run_a, run_b):
    a_ms, b_ms = [], []
    for _ in range(ROUNDS):
        a_ms.append(timed(run_a)[0])
        b_ms.append(timed(run_b)[0])
    a, b = sum(a_ms) / ROUNDS, sum(b_ms) / ROUNDS
    return {"A_ms": a_ms, "B_ms": b_ms, "A_ms_mean": a, "B_ms_mean": b, "B_over_A": b / a,
            "A_spread_rel": (max(a_ms) - min(a_ms)) / a, "B_spread_rel": (max(b_ms) - min(b_ms)) / b,
            "every_B_below_every_A_by_more_than_A_spread": min(a_ms) - max(b_ms) > max(a_ms) - min(a_ms)}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_trunk_mx: no GPU visible; there is nothing to time without one")
    o, d = utils.gen_rays(H, W, synth.fern_intrinsics(H, W), synth.spiral_pose(5))
    head = bench.make_renderer("fp16x3+fp16mx", True)
    head = rendering.RayRenderer(head.coarse, head.fine, style=head.style)
    x3 = rendering.RayRenderer(None, bench.make_renderer("fp16x3", False).fine, style=head.style)   # the same fine weights
    assert head.fine.packed().precision == "fp16mx" and x3.fine.packed().precision == "fp16x3"
    R = o.shape[0]
    cache = head.build_geometry(o, d, NC, NF, min_weight=0.)
    run_a = lambda: x3.build_trunk(cache, o, d)
    run_b = lambda: head.build_trunk(cache, o, d, trunk_precision="fp16x3")
    for _ in range(2):                  # warm-up: code objects, and a second plane for the allocator to hand back and forth
        run_a(), run_b()
    plane_b = cache.trunk
    plane_a = run_a().trunk
    assert cache.trunk_source == "fp16x3" and torch.equal(run_b().trunk, plane_b) and cache.trunk_source == "fp16mx"
    result = {"frame": [H, W], "pose": 5, "rays": R, "n_coarse": NC, "n_fine": NF, "rounds": ROUNDS,
              "renders_per_measurement": RENDERS, "device": torch.cuda.get_device_name(0), "live_samples": cache.count,
              "trunk_bytes": plane_b.numel(),
              "A": "build_trunk from the fine weights in fp16x3 (tgtc_geometry_trunk)",
              "B": "build_trunk(trunk_precision='fp16x3') from the same weights in fp16mx (tgtc_geometry_trunk_mx)",
              "mfma_slots_per_sample_column": {"fp16x3": SLOTS_X3, "fp16mx": SLOTS_MX}}
    print("live %d of %d; plane %d bytes" % (cache.count, R * (NC + NF), plane_b.numel()), flush=True)
    rec = interleaved(run_a, run_b)
    rec["predicted_B_over_A_by_mfma_slots"] = SLOTS_MX / SLOTS_X3
    rec["measured_over_predicted"] = rec["B_over_A"] / rec["predicted_B_over_A_by_mfma_slots"]
    result["build_trunk"] = rec
    print("build_trunk  A (fp16x3) %6.2f ms [%s]   B (fp16mx) %6.2f ms [%s]   B/A %.3f (MFMA slots: %.3f)   spread of A %.2f %%   "
          "every B below every A by more than that: %s"
          % (rec["A_ms_mean"], " ".join("%.2f" % x for x in rec["A_ms"]), rec["B_ms_mean"], " ".join("%.2f" % x for x in rec["B_ms"]),
             rec["B_over_A"], rec["predicted_B_over_A_by_mfma_slots"], 100 * rec["A_spread_rel"],
             rec["every_B_below_every_A_by_more_than_A_spread"]), flush=True)

    # the consumer on either plane
    gen = torch.Generator(device="cuda").manual_seed(1)
    zs_all = torch.randn(max(KS), R, 32, device="cuda", generator=gen)      # the latents of tools/time_restyle_trunk.py
    result["restyle_fp16mx"] = {}
    for K in KS:
        z = zs_all[:K, 0].contiguous()

        def from_plane(plane, source, **kw):
            cache.attach_trunk(plane, "fp16x3", source)
            return head.restyle(cache, o, d, z, **kw)
        run_pa = lambda: from_plane(plane_a, "fp16x3", style_precision="fp16mx")
        run_pb = lambda: from_plane(plane_b, "fp16mx", style_precision="fp16mx")
        for _ in range(2):
            img_a, img_b = run_pa(), run_pb()
        torch.cuda.synchronize()
        rec = interleaved(run_pa, run_pb)
        rec["image_max_abs_diff_style_fp16mx"] = float((img_a["rgb"] - img_b["rgb"]).abs().max())
        rec["image_max_abs_diff_style_fp16x3"] = float((from_plane(plane_a, "fp16x3")["rgb"] - from_plane(plane_b, "fp16mx")["rgb"]).abs().max())
        assert torch.equal(img_a["t"], img_b["t"])
        result["restyle_fp16mx"][str(K)] = rec
        print("  K=%d restyle(style_precision='fp16mx')  from plane A %6.2f ms [%s]   from plane B %6.2f ms [%s]   B/A %.3f   "
              "max |A - B| %.2e (fp16mx style nets), %.2e (fp16x3 style nets)"
              % (K, rec["A_ms_mean"], " ".join("%.2f" % x for x in rec["A_ms"]), rec["B_ms_mean"],
                 " ".join("%.2f" % x for x in rec["B_ms"]), rec["B_over_A"], rec["image_max_abs_diff_style_fp16mx"],
                 rec["image_max_abs_diff_style_fp16x3"]), flush=True)

    out_path = os.path.join(ROOT, "profiles", "trunk_mx_timing.json")
    if len(sys.argv) > 1:
        out_path = sys.argv[1]
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
