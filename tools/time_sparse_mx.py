#!/usr/bin/env python3
"""Timing of the stylised frame of the fp16x3+fp16mx pair in one call and of its restyle without a plane
(csrc/mlp_list_mx.hip): the frame, pose, shapes and schedule of tools/time_restyle_trunk.py and tools/time_trunk_mx.py
(400x400 fern-shaped, pose 5, R = 160 000, 128c + 64f), K in {1, 2, 4} frame-constant latents.

(i) the whole frame, min_weight = 0
    A = render_latents(zs [K,32], min_weight=0) of the all-fp16x3 renderer   (tgtc_render_rays_styled_sparse_folded: the only
                                                                             one-call culled stylised frame there was)
    B = the same call of the fp16x3+fp16mx renderer with style_precision="fp16mx"   (tgtc_render_rays_styled_sparse_folded_mx)
(ii) the restyle of the fp16x3+fp16mx renderer from ONE geometry cache
    A  = restyle(style_precision="fp16mx") from a resident fp16x3 plane      (tgtc_restyle_rays_trunk_folded_mx)
    A' = build_trunk(trunk_precision="fp16x3") + A                           (tgtc_geometry_trunk_mx in front of it)
    B  = restyle(style_precision="fp16mx") without a plane                   (tgtc_restyle_rays_folded_mx)

Same process, A and B (A, A' and B) alternating, after a warm-up, device events around RENDERS calls each, ROUNDS rounds so that
the spread of A against itself is known.  B counts as faster only if every B round is below every A round by more than A's
spread.  Beside the times: the live share, the peak device memory of one call of each (torch.cuda.max_memory_allocated, and
its rise over what was allocated before the call), and that B of (ii) carries the bits of A.

Prints and writes profiles/sparse_mx_timing.json.  Needs a GPU: there is no fallback."""
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


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(RENDERS):
        out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / RENDERS, out


def interleaved(runs):
    """runs: name -> callable; ROUNDS rounds of one measurement of each, in the order given."""
    ms = {name: [] for name in runs}
    for _ in range(ROUNDS):
        for name, fn in runs.items():
            ms[name].append(timed(fn)[0])
    rec = {}
    for name, v in ms.items():
        mean = sum(v) / len(v)
        rec[name] = {"ms": v, "ms_mean": mean, "spread_rel": (max(v) - min(v)) / mean}
    return rec


def below(rec, b, a):
    """Is every round of b below every round of a by more than a's spread?"""
    va, vb = rec[a]["ms"], rec[b]["ms"]
    return min(va) - max(vb) > max(va) - min(va)


def peak(fn):
    """(peak bytes allocated during one call, its rise over the bytes allocated before the call)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    top = torch.cuda.max_memory_allocated()
    del out
    return {"peak_bytes": top, "rise_bytes": top - base}


def line(title, rec):
    return title + "   ".join("%s %7.2f ms [%s]" % (n, r["ms_mean"], " ".join("%.2f" % x for x in r["ms"])) for n, r in rec.items()
                              if isinstance(r, dict) and "ms" in r)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_sparse_mx: no GPU visible; there is nothing to time without one")
    o, d = utils.gen_rays(H, W, synth.fern_intrinsics(H, W), synth.spiral_pose(5))
    head = bench.make_renderer("fp16x3+fp16mx", True)
    head = rendering.RayRenderer(head.coarse, head.fine, style=head.style)
    x3 = bench.make_renderer("fp16x3", True)
    x3 = rendering.RayRenderer(x3.coarse, x3.fine, style=x3.style)
    assert head.fine.packed().precision == "fp16mx" and head.style.packed().precision == "fp16x3"
    assert x3.fine.packed().precision == "fp16x3" and x3.style.packed().precision == "fp16x3"
    R = o.shape[0]
    gen = torch.Generator(device="cuda").manual_seed(1)
    zs_all = torch.randn(max(KS), R, 32, device="cuda", generator=gen)      # the latents of tools/time_restyle_trunk.py
    result = {"frame_hw": [H, W], "pose": 5, "rays": R, "n_coarse": NC, "n_fine": NF, "rounds": ROUNDS,
              "renders_per_measurement": RENDERS, "device": torch.cuda.get_device_name(0), "min_weight": 0.0,
              "frame_A": "all-fp16x3 render_latents(zs [K,32], min_weight=0) (tgtc_render_rays_styled_sparse_folded)",
              "frame_B": "fp16x3+fp16mx render_latents(..., style_precision='fp16mx') (tgtc_render_rays_styled_sparse_folded_mx)",
              "restyle_A": "restyle(style_precision='fp16mx') from a resident fp16x3 plane (tgtc_restyle_rays_trunk_folded_mx)",
              "restyle_A1": "build_trunk(trunk_precision='fp16x3') + A (tgtc_geometry_trunk_mx in front of it)",
              "restyle_B": "restyle(style_precision='fp16mx') without a plane (tgtc_restyle_rays_folded_mx)",
              "frame": {}, "restyle": {}}

    # ---- (i) the whole frame
    for K in KS:
        z = zs_all[:K, 0].contiguous()
        run_a = lambda: x3.render_latents(o, d, NC, NF, zs=z, min_weight=0.)
        run_b = lambda: head.render_latents(o, d, NC, NF, zs=z, min_weight=0., style_precision="fp16mx")
        for _ in range(2):
            img_a, img_b = run_a(), run_b()
        torch.cuda.synchronize()
        rec = interleaved({"A": run_a, "B": run_b})
        rec["B_over_A"] = rec["B"]["ms_mean"] / rec["A"]["ms_mean"]
        rec["every_B_below_every_A_by_more_than_A_spread"] = below(rec, "B", "A")
        rec["live_A"], rec["live_B"] = int(img_a["live"]), int(img_b["live"])
        rec["live_share_A"], rec["live_share_B"] = rec["live_A"] / (R * (NC + NF)), rec["live_B"] / (R * (NC + NF))
        # (two frames from two fine networks: the sampler's ill-conditioned rays of DESIGN section 4 carry the maximum)
        diff = (img_a["rgb"] - img_b["rgb"]).abs().amax(dim=(0, 2))
        rec["image_max_abs_diff"] = float(diff.max())
        rec["image_median_abs_diff"] = float(diff.median())
        rec["rays_above_1e-3"] = float((diff > 1e-3).float().mean())
        del img_a, img_b
        rec["memory_A"], rec["memory_B"] = peak(run_a), peak(run_b)
        result["frame"][str(K)] = rec
        print(line("frame   K=%d  " % K, rec) + "   B/A %.3f   every B below every A by more than A's spread: %s   live %.4f / %.4f   "
              "|A - B| per ray: median %.2e, above 1e-3 on %.2f %%, max %.2e   peak %.0f / %.0f MB"
              % (rec["B_over_A"], rec["every_B_below_every_A_by_more_than_A_spread"], rec["live_share_A"], rec["live_share_B"],
                 rec["image_median_abs_diff"], 100 * rec["rays_above_1e-3"], rec["image_max_abs_diff"], rec["memory_A"]["peak_bytes"] / 1e6, rec["memory_B"]["peak_bytes"] / 1e6), flush=True)
    # the workspaces of (i) are not part of (ii)
    x3._ws_multi = None
    del x3

    # ---- (ii) the restyle
    cache = head.build_geometry(o, d, NC, NF, min_weight=0.)
    head._ws_multi = None
    torch.cuda.empty_cache()
    result["live_samples"], result["live_share"] = cache.count, cache.count / (R * (NC + NF))
    result["trunk_bytes"] = cache.trunk_nbytes("fp16x3", cache.count)
    print("live %d of %d; a plane would hold %d bytes" % (cache.count, R * (NC + NF), result["trunk_bytes"]), flush=True)
    for K in KS:
        z = zs_all[:K, 0].contiguous()
        cache.drop_trunk()
        run_b = lambda: head.restyle(cache, o, d, z, style_precision="fp16mx", use_trunk=False)
        run_a = lambda: head.restyle(cache, o, d, z, style_precision="fp16mx")
        run_a1 = lambda: head.restyle(head.build_trunk(cache, o, d, trunk_precision="fp16x3"), o, d, z, style_precision="fp16mx")
        img_b = run_b()
        mem_b = peak(run_b)                                      # before any plane exists
        for _ in range(2):
            img_a1, img_a, img_b = run_a1(), run_a(), run_b()
        torch.cuda.synchronize()
        same = torch.equal(img_a["rgb"], img_b["rgb"]) and torch.equal(img_a1["rgb"], img_b["rgb"]) and torch.equal(img_a["t"], img_b["t"])
        del img_a, img_a1, img_b
        rec = interleaved({"A": run_a, "A1": run_a1, "B": run_b})
        rec["B_over_A1"] = rec["B"]["ms_mean"] / rec["A1"]["ms_mean"]
        rec["B_over_A"] = rec["B"]["ms_mean"] / rec["A"]["ms_mean"]
        rec["every_B_below_every_A1_by_more_than_A1_spread"] = below(rec, "B", "A1")
        rec["every_A1_below_every_B_by_more_than_B_spread"] = below(rec, "A1", "B")
        rec["B_is_the_bits_of_A"] = same
        rec["memory_A"] = peak(run_a)                            # the plane is resident: part of the peak, not of the rise
        cache.drop_trunk()
        torch.cuda.empty_cache()
        rec["memory_A1"] = peak(run_a1)
        rec["memory_B"] = mem_b
        result["restyle"][str(K)] = rec
        print(line("restyle K=%d  " % K, rec) + "   B/A' %.3f   B/A %.3f   every B below every A' by more than its spread: %s   bits of A: %s   "
              "peak A %.0f  A' %.0f  B %.0f MB"
              % (rec["B_over_A1"], rec["B_over_A"], rec["every_B_below_every_A1_by_more_than_A1_spread"], same,
                 rec["memory_A"]["peak_bytes"] / 1e6, rec["memory_A1"]["peak_bytes"] / 1e6, rec["memory_B"]["peak_bytes"] / 1e6), flush=True)

    out_path = os.path.join(ROOT, "profiles", "sparse_mx_timing.json")
    if len(sys.argv) > 1:
        out_path = sys.argv[1]
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
