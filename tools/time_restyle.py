#!/usr/bin/env python3
"""Timing of the restyle from a cached geometry: a whole 400x400 fern-shaped frame (R = 160 000), 128c + 64f, fp16x3, under
K in {1, 2, 4} latent sets.

    A = RayRenderer.render_latents(min_weight=0)    (the culled render: geometry half, sigma pass, weights, compaction, then
                                                     the style networks on the live samples and K dense compositing launches)
    B = RayRenderer.restyle(cache, ...)             (the cache built BEFORE the timed region: the compact style kernel over the
                                                     cached list and one compositing launch over (latent, ray))

Same process, A and B alternating, every shape warmed up, device events around RENDERS renders each, ROUNDS A/B rounds so
that the spread of A against itself is known.  B's image is checked torch.equal to A's.  One build_geometry (build, the
count read, pack) is timed against A as well, with a host clock around a call that ends in the count read and a final
synchronise.  The prediction is by op count: per fine sample B costs f x (556 800 + K x 950 112)
multiply-accumulates, A costs 128/192 x 491 264 + 491 264 + f x (556 800 + K x 950 112), with f the live fraction read from
the cache.

Prints and writes profiles/restyle_timing.json.  Needs a GPU: there is no fallback."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tgtc_style_amd import rendering, synth, utils  # noqa: E402

H = W = 400
NC, NF = 128, 64
NT = NC + NF
KS = (1, 2, 4)
ROUNDS, RENDERS = 3, 5
MAC_SIGMA, MAC_TRUNK, MAC_PER_LATENT = 491264, 556800, 950112     # per sample


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(RENDERS):
        out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / RENDERS, out


def predicted_ratio(K, f):
    style = f * (MAC_TRUNK + K * MAC_PER_LATENT)
    return style / (NC * MAC_SIGMA / NT + MAC_SIGMA + style)


def measure(r, cache, o, d, zs):
    K = zs.shape[0]
    run_a = lambda: r.render_latents(o, d, NC, NF, zs=zs, min_weight=0.)
    run_b = lambda: r.restyle(cache, o, d, zs)
    for _ in range(2):      # warm-up of both shapes (workspaces, code objects)
        a_out, b_out = run_a(), run_b()
    torch.cuda.synchronize()
    assert torch.equal(b_out["rgb"], a_out["rgb"]) and torch.equal(b_out["t"], a_out["t"]), "B is not A's image"
    assert int(a_out["live"]) == cache.count
    a_ms, b_ms = [], []
    for _ in range(ROUNDS):
        a_ms.append(timed(run_a)[0])
        b_ms.append(timed(run_b)[0])
    f = cache.count / (cache.R * NT)
    a, b = sum(a_ms) / ROUNDS, sum(b_ms) / ROUNDS
    rec = {"A_ms": a_ms, "B_ms": b_ms, "A_ms_mean": a, "B_ms_mean": b, "B_over_A": b / a,
           "A_spread_rel": (max(a_ms) - min(a_ms)) / a, "B_spread_rel": (max(b_ms) - min(b_ms)) / b,
           "B_below_A_by_more_than_A_spread": max(b_ms) < min(a_ms) and (a - b) > (max(a_ms) - min(a_ms)),
           "predicted_B_over_A_by_op_count": predicted_ratio(K, f),
           "B_rays_x_latents_per_s": zs.shape[1] * K / b * 1e3}
    rec["measured_over_predicted"] = rec["B_over_A"] / rec["predicted_B_over_A_by_op_count"]
    print("K=%d  A (culled render) %8.2f ms [%s]   B (restyle) %8.2f ms [%s]   B/A %.3f (op count: %.3f, x%.2f)   "
          "spread of A %.2f %%" % (K, a, " ".join("%.2f" % x for x in a_ms), b, " ".join("%.2f" % x for x in b_ms), b / a,
                                    rec["predicted_B_over_A_by_op_count"], rec["measured_over_predicted"],
                                    100 * rec["A_spread_rel"]), flush=True)
    return rec


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_restyle: no GPU visible; there is nothing to time without one")
    precision = "fp16x3"
    r = bench.make_renderer(precision, True)
    r = rendering.RayRenderer(r.coarse, r.fine, style=r.style)
    o, d = utils.gen_rays(H, W, synth.fern_intrinsics(H, W), synth.spiral_pose(5))
    R = H * W
    zs_all = torch.randn(max(KS), R, 32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    build = lambda: r.build_geometry(o, d, NC, NF, min_weight=0.)
    cache = build()                     # warm-up, and the cache of every B below
    build_ms = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        build()
        torch.cuda.synchronize()
        build_ms.append((time.perf_counter() - t0) * 1e3)
    result = {"frame": [H, W], "pose": 5, "rays": R, "n_coarse": NC, "n_fine": NF, "precision": precision, "rounds": ROUNDS,
              "renders_per_measurement": RENDERS, "device": torch.cuda.get_device_name(0), "live_samples": cache.count,
              "live_fraction": cache.count / (R * NT), "cache_bytes": cache.buffer.numel(),
              "build_geometry_ms": build_ms, "build_geometry_ms_mean": sum(build_ms) / ROUNDS, "per_K": {}}
    print("build_geometry (build + count read + pack) %.2f ms [%s]; live %.4f; cache %d bytes" % (
        result["build_geometry_ms_mean"], " ".join("%.2f" % x for x in build_ms), result["live_fraction"], result["cache_bytes"]),
        flush=True)
    for K in KS:
        result["per_K"][str(K)] = measure(r, cache, o, d, zs_all[:K].contiguous())
    result["build_geometry_over_A_K1"] = result["build_geometry_ms_mean"] / result["per_K"]["1"]["A_ms_mean"]

    out_path = os.path.join(ROOT, "profiles", "restyle_timing.json")
    if len(sys.argv) > 1:
        out_path = sys.argv[1]
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
