#!/usr/bin/env python3
"""Timing of the folded restyle (frame-constant latents as per-latent bias tables) against the unfolded one: the frame, pose,
sample counts, rounds and JSON shape of tools/time_restyle.py -- a whole 400x400 fern-shaped frame (R = 160 000), 128c + 64f,
fp16x3, K in {1, 2, 4} -- on ONE geometry cache built before the timed region.

    A = RayRenderer.restyle(cache, ..., zs [K,R,32])   (this build's unfolded restyle, the K latents copied to every ray; it is
                                                        the B of tools/time_restyle.py / profiles/restyle_timing.json)
    B = RayRenderer.restyle(cache, ..., zs [K,32])     (tgtc_restyle_rays_folded: the fold kernel, the folded compact style
                                                        kernel, the same compositing launch)

Same process, A and B alternating, every shape warmed up, device events around RENDERS renders each, ROUNDS A/B rounds so
that the spread of A against itself is known.  B's image is checked against A's at 2 x 5e-5 (the folded and the unfolded
kernels round the latent differently), its depth image bit for bit.  The prediction is by op count in fragments (16x16x32
MFMA operands): per live sample the trunk costs 1096, a latent 1865 unfolded and 1672 folded, so
B / A = (1096 + 1672 K) / (1096 + 1865 K); the compositing launch and the fold kernel are not in it.

`parent_A_ms` (optional, argv[2]: a profiles/restyle_timing.json written by tools/time_restyle.py at the parent commit on the
same device in the same session) is recorded beside A with the relative difference of the means, so that A can be seen to be
the restyle it claims to be.

Prints and writes profiles/fold_latents_timing.json.  Needs a GPU: there is no fallback."""
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
FRAG_TRUNK, FRAG_LATENT, FRAG_LATENT_FOLDED = 1096, 656 + 1209, 576 + 1096     # csrc/mlp_layouts.h


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(RENDERS):
        out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / RENDERS, out


def predicted_ratio(K):
    return (FRAG_TRUNK + FRAG_LATENT_FOLDED * K) / (FRAG_TRUNK + FRAG_LATENT * K)


def measure(r, cache, o, d, z, parent):
    K, R = z.shape[0], o.shape[0]
    zs = z[:, None, :].expand(-1, R, -1).contiguous()
    run_a = lambda: r.restyle(cache, o, d, zs)
    run_b = lambda: r.restyle(cache, o, d, z)
    for _ in range(2):      # warm-up of both shapes (workspaces, code objects)
        a_out, b_out = run_a(), run_b()
    torch.cuda.synchronize()
    diff = float((a_out["rgb"] - b_out["rgb"]).abs().max())
    assert diff <= 1e-4 and torch.equal(b_out["t"], a_out["t"]), "B is not A's image: max |diff| %g" % diff
    a_ms, b_ms = [], []
    for _ in range(ROUNDS):
        a_ms.append(timed(run_a)[0])
        b_ms.append(timed(run_b)[0])
    a, b = sum(a_ms) / ROUNDS, sum(b_ms) / ROUNDS
    rec = {"A_ms": a_ms, "B_ms": b_ms, "A_ms_mean": a, "B_ms_mean": b, "B_over_A": b / a,
           "A_spread_rel": (max(a_ms) - min(a_ms)) / a, "B_spread_rel": (max(b_ms) - min(b_ms)) / b,
           "B_below_A_by_more_than_A_spread": max(b_ms) < min(a_ms) and (a - b) > (max(a_ms) - min(a_ms)),
           "predicted_B_over_A_by_op_count": predicted_ratio(K),
           "saved_ms_per_latent": (a - b) / K, "max_abs_image_diff_B_vs_A": diff,
           "latent_plane_bytes_A": zs.numel() * 4, "latent_bytes_B": z.numel() * 4,
           "B_rays_x_latents_per_s": R * K / b * 1e3}
    rec["measured_over_predicted"] = rec["B_over_A"] / rec["predicted_B_over_A_by_op_count"]
    if parent is not None:
        p = parent["per_K"][str(K)]
        rec["parent_A_ms"] = p["B_ms"]
        rec["A_over_parent_A"] = a / p["B_ms_mean"]
    print("K=%d  A (unfolded restyle) %8.2f ms [%s]   B (folded) %8.2f ms [%s]   B/A %.3f (op count: %.3f, x%.2f)   "
          "spread of A %.2f %%   image diff %.1e%s" % (
              K, a, " ".join("%.2f" % x for x in a_ms), b, " ".join("%.2f" % x for x in b_ms), b / a,
              rec["predicted_B_over_A_by_op_count"], rec["measured_over_predicted"], 100 * rec["A_spread_rel"], diff,
              "   A / parent's restyle %.4f" % rec["A_over_parent_A"] if parent is not None else ""), flush=True)
    return rec


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_fold_latents: no GPU visible; there is nothing to time without one")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fold_latents_timing.json")
    parent = json.load(open(sys.argv[2])) if len(sys.argv) > 2 else None
    precision = "fp16x3"
    r = bench.make_renderer(precision, True)
    r = rendering.RayRenderer(r.coarse, r.fine, style=r.style)
    o, d = utils.gen_rays(H, W, synth.fern_intrinsics(H, W), synth.spiral_pose(5))
    R = H * W
    z_all = torch.randn(max(KS), 32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    cache = r.build_geometry(o, d, NC, NF, min_weight=0.)
    result = {"frame": [H, W], "pose": 5, "rays": R, "n_coarse": NC, "n_fine": NF, "precision": precision, "rounds": ROUNDS,
              "renders_per_measurement": RENDERS, "device": torch.cuda.get_device_name(0), "live_samples": cache.count,
              "live_fraction": cache.count / (R * NT), "A": "RayRenderer.restyle(cache, zs [K,R,32]) of this build",
              "B": "RayRenderer.restyle(cache, zs [K,32]): tgtc_restyle_rays_folded", "per_K": {}}
    if parent is not None:
        assert (parent["rays"], parent["n_coarse"], parent["n_fine"], parent["precision"], parent["live_samples"]) == (
            R, NC, NF, precision, cache.count), "the parent's record is of another frame"
        result["parent_A"] = ("B_ms of tools/time_restyle.py run at the parent commit on this device in the same session "
                              "(its B is this tool's A; latents drawn per ray there, copied per ray here)")
    print("live %.4f (%d samples)" % (result["live_fraction"], cache.count), flush=True)
    for K in KS:
        result["per_K"][str(K)] = measure(r, cache, o, d, z_all[:K].contiguous(), parent)
    if parent is not None:
        worst = max(abs(v["A_over_parent_A"] - 1) for v in result["per_K"].values())
        result["A_matches_parent_within"] = worst
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
