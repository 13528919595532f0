#!/usr/bin/env python3
"""Timing of the restyle from a cached trunk plane: the frame of tools/time_restyle.py (400x400 fern-shaped, pose 5, R = 160 000,
128c + 64f), one geometry cache per precision, fp16x3 and fp16, K in {1, 2, 4} latents, unfolded (zs [K,R,32]) and folded
(zs [K,32]).

    A = RayRenderer.restyle(cache, ..., use_trunk=False)   (tgtc_restyle_rays[_folded]: the fine NeRF trunk, then the style
                                                            networks, per tile of the cached list)
    B = RayRenderer.restyle(cache, ...)                    (tgtc_restyle_rays_trunk[_folded]: the style networks alone,
                                                            base_remap read from the plane built BEFORE the timed region)

Same process, A and B alternating, every shape warmed up, device events around RENDERS renders each, ROUNDS A/B rounds so
that the spread of A against itself is known.  B's image is checked torch.equal to A's.  build_trunk (one launch of the trunk
producer) is timed with device events as well.  The prediction is by fragment count per live sample: the
trunk walks 1 096 fragments, a latent 656 + 1 209 = 1 865 (576 + 1 096 = 1 672 folded), so B/A = K x 1865 / (1096 + K x 1865).

Prints and writes profiles/restyle_trunk_timing.json.  Needs a GPU: there is no fallback."""
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
NT = NC + NF
KS = (1, 2, 4)
ROUNDS, RENDERS = 3, 5
FRAGS_TRUNK, FRAGS_LATENT, FRAGS_LATENT_FOLDED = 1096, 656 + 1209, 576 + 1096


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(RENDERS):
        out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / RENDERS, out


def predicted_ratio(K, folded):
    per_latent = FRAGS_LATENT_FOLDED if folded else FRAGS_LATENT
    return K * per_latent / (FRAGS_TRUNK + K * per_latent)


def measure(r, cache, o, d, zs):
    K, folded = zs.shape[0], zs.dim() == 2
    run_a = lambda: r.restyle(cache, o, d, zs, use_trunk=False)
    run_b = lambda: r.restyle(cache, o, d, zs, use_trunk=True)
    for _ in range(2):      # warm-up of both shapes (workspaces, code objects)
        a_out, b_out = run_a(), run_b()
    torch.cuda.synchronize()
    assert torch.equal(b_out["rgb"], a_out["rgb"]) and torch.equal(b_out["t"], a_out["t"]), "B is not A's image"
    a_ms, b_ms = [], []
    for _ in range(ROUNDS):
        a_ms.append(timed(run_a)[0])
        b_ms.append(timed(run_b)[0])
    a, b = sum(a_ms) / ROUNDS, sum(b_ms) / ROUNDS
    rec = {"A_ms": a_ms, "B_ms": b_ms, "A_ms_mean": a, "B_ms_mean": b, "B_over_A": b / a,
           "A_spread_rel": (max(a_ms) - min(a_ms)) / a, "B_spread_rel": (max(b_ms) - min(b_ms)) / b,
           "B_below_A_by_more_than_A_spread": max(b_ms) < min(a_ms) and (a - b) > (max(a_ms) - min(a_ms)),
           "predicted_B_over_A_by_fragment_count": predicted_ratio(K, folded),
           "B_rays_x_latents_per_s": cache.R * K / b * 1e3}
    rec["measured_over_predicted"] = rec["B_over_A"] / rec["predicted_B_over_A_by_fragment_count"]
    print("  %-8s K=%d  A (restyle) %7.2f ms [%s]   B (from the plane) %7.2f ms [%s]   B/A %.3f (fragments: %.3f, x%.2f)   "
          "spread of A %.2f %%" % ("folded" if folded else "unfolded", K, a, " ".join("%.2f" % x for x in a_ms), b,
                                    " ".join("%.2f" % x for x in b_ms), b / a, rec["predicted_B_over_A_by_fragment_count"],
                                    rec["measured_over_predicted"], 100 * rec["A_spread_rel"]), flush=True)
    return rec


def one_precision(precision, o, d):
    r = bench.make_renderer(precision, True)
    r = rendering.RayRenderer(r.coarse, r.fine, style=r.style)
    R = o.shape[0]
    gen = torch.Generator(device="cuda").manual_seed(1)
    zs_all = torch.randn(max(KS), R, 32, device="cuda", generator=gen)
    cache = r.build_geometry(o, d, NC, NF, min_weight=0.)
    r.build_trunk(cache, o, d)          # warm-up, and the plane of every B below
    plane = cache.trunk
    build_ms = []
    for _ in range(ROUNDS):
        build_ms.append(timed(lambda: r.build_trunk(cache, o, d))[0])
    assert torch.equal(cache.trunk, plane), "two builds of the plane differ"
    del plane
    rec = {"live_samples": cache.count, "live_fraction": cache.count / (R * NT), "cache_bytes": cache.buffer.numel(),
           "trunk_bytes": cache.trunk.numel(), "trunk_bytes_per_live_sample": cache.trunk.numel() / max(cache.count, 1),
           "build_trunk_ms": build_ms, "build_trunk_ms_mean": sum(build_ms) / ROUNDS, "unfolded": {}, "folded": {}}
    print("%s: live %d (%.4f); cache %d bytes; plane %d bytes; build_trunk %.2f ms [%s]" % (
        precision, cache.count, rec["live_fraction"], rec["cache_bytes"], rec["trunk_bytes"], rec["build_trunk_ms_mean"],
        " ".join("%.2f" % x for x in build_ms)), flush=True)
    for K in KS:
        rec["unfolded"][str(K)] = measure(r, cache, o, d, zs_all[:K].contiguous())
        rec["folded"][str(K)] = measure(r, cache, o, d, zs_all[:K, 0].contiguous())
    rec["claim_K1_B_below_A_by_more_than_A_spread"] = all(rec[form]["1"]["B_below_A_by_more_than_A_spread"]
                                                          for form in ("unfolded", "folded"))
    return rec


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_restyle_trunk: no GPU visible; there is nothing to time without one")
    o, d = utils.gen_rays(H, W, synth.fern_intrinsics(H, W), synth.spiral_pose(5))
    result = {"frame": [H, W], "pose": 5, "rays": H * W, "n_coarse": NC, "n_fine": NF, "rounds": ROUNDS,
              "renders_per_measurement": RENDERS, "device": torch.cuda.get_device_name(0),
              "A": "restyle(use_trunk=False)", "B": "restyle(use_trunk=True)", "per_precision": {}}
    for precision in ("fp16x3", "fp16"):
        result["per_precision"][precision] = one_precision(precision, o, d)
        torch.cuda.empty_cache()
    result["claim_K1_holds_in_both_precisions"] = all(p["claim_K1_B_below_A_by_more_than_A_spread"]
                                                      for p in result["per_precision"].values())
    print("K = 1: B below A by more than A's spread in both precisions:", result["claim_K1_holds_in_both_precisions"])

    out_path = os.path.join(ROOT, "profiles", "restyle_trunk_timing.json")
    if len(sys.argv) > 1:
        out_path = sys.argv[1]
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
