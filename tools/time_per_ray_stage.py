#!/usr/bin/env python3
"""Development timing of the per-ray stage of the plain chain, one 400x400 frame at 128 + 64 samples, coarse
fp16x3 + fine fp16mx, HIP events on the launch stream, the variants interleaved, on the planes of a real render.

    python tools/time_per_ray_stage.py [--rounds N] [--out FILE]
        between the passes:   tgtc_composite (weights out) + tgtc_sample_fine      against  tgtc_coarse_to_fine
        after the fine pass:  zero-fill of the colour plane + tgtc_composite        against  tgtc_composite_live_colours
        and whether the two sides of each pair give the same bits on these planes
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from time_plain_cull import H, NC, NF, NT, W, stats, timed
from tgtc_style_amd import hip, rendering, synth, utils


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()

    lib = hip.load()
    coarse, fine = bench.build_nets("fp16x3+fp16mx")
    R = H * W
    # the planes of a real frame: a dense render leaves all of them in the workspace (csrc/render.hip, RenderWorkspace)
    r = rendering.RayRenderer(coarse, fine, fused=False, cull=False, screen=False)
    o, d = (x.contiguous() for x in utils.gen_rays(H, W, synth.fern_intrinsics(H, W), synth.spiral_pose(0)))
    r.render(o, d, NC, NF, near=0., far=1.)
    torch.cuda.synchronize()
    wsf = r._ws.view(torch.float32)
    ts_c = wsf[:R * NC].clone()
    sigma_c = wsf[R * NC:2 * R * NC].clone()
    base = 6 * R * NC
    ts_f = wsf[base:base + R * NT].clone()
    sigma_f = wsf[base + R * NT:base + 2 * R * NT].clone()
    rgb_f = wsf[base + 2 * R * NT:base + 5 * R * NT].clone()
    live = sigma_f > 0
    rgb_zeroed = rgb_f.view(-1, 3) * live[:, None]
    rgb_poisoned = torch.where(live[:, None], rgb_f.view(-1, 3), torch.full_like(rgb_f.view(-1, 3), float("nan"))).contiguous()
    scratch_plane = torch.empty_like(rgb_zeroed)

    w_pair, out_pair = torch.empty(R * NC, device="cuda"), torch.empty(R * NT, device="cuda")
    out_one = torch.empty(R * NT, device="cuda")
    px = [torch.empty(R, 3, device="cuda") for _ in range(2)]
    pt = [torch.empty(R, device="cuda") for _ in range(2)]
    st = hip.stream

    def pair():
        hip.check(lib.tgtc_composite(hip.ptr(rgb_zeroed), hip.ptr(sigma_c), hip.ptr(ts_c), R, NC, hip.ptr(px[0]), hip.ptr(pt[0]),
                                     hip.ptr(w_pair), st()))
        hip.check(lib.tgtc_sample_fine(hip.ptr(o), hip.ptr(d), hip.ptr(ts_c), hip.ptr(w_pair), R, NC, NF, None, hip.ptr(out_pair), st()))

    def one():
        hip.check(lib.tgtc_coarse_to_fine(hip.ptr(sigma_c), hip.ptr(ts_c), R, NC, NF, hip.ptr(out_one), None, st()))

    def fill_and_composite():
        scratch_plane.zero_()
        hip.check(lib.tgtc_composite(hip.ptr(rgb_zeroed), hip.ptr(sigma_f), hip.ptr(ts_f), R, NT, hip.ptr(px[0]), hip.ptr(pt[0]), None, st()))

    def live_colours():
        hip.check(lib.tgtc_composite_live_colours(hip.ptr(rgb_poisoned), hip.ptr(sigma_f), hip.ptr(ts_f), R, NT, hip.ptr(px[1]),
                                                  hip.ptr(pt[1]), None, st()))

    # (tgtc_composite needs a colour plane: the coarse pair reads the first R * NC rows of the fine one, as a sigma-only
    # coarse pass would not -- its kernel time is the trace's, this is the upper bound)
    t = timed({"composite_weights_then_sample_fine": pair, "coarse_to_fine": one,
               "zero_fill_then_composite": fill_and_composite, "composite_live_colours": live_colours}, args.rounds)
    torch.cuda.synchronize()
    took = torch.empty(R, dtype=torch.int32, device="cuda")
    hip.check(lib.tgtc_coarse_to_fine_traced(hip.ptr(sigma_c), hip.ptr(ts_c), R, NC, NF, hip.ptr(out_one), None, hip.ptr(took), st()))
    torch.cuda.synchronize()
    result = {"shape": "%d rays, %d coarse + %d fine samples, planes of spiral pose 0" % (R, NC, NF), "rounds": args.rounds,
              "kernels": {k: stats(v) for k, v in t.items()},
              "live_share_fine": float(live.float().mean()),
              "rays_on_the_counting_sort": int(took.sum()),
              "fine_depths_same_bits": bool(torch.equal(out_pair.view(torch.int32), out_one.view(torch.int32))),
              "fine_image_same_bits": bool(torch.equal(px[0], px[1]) and torch.equal(pt[0], pt[1]))}
    for k, v in t.items():
        print("%-36s %8.3f ms (min %.3f, max %.3f)" % (k, np.mean(v), np.min(v), np.max(v)), flush=True)
    print({k: v for k, v in result.items() if k != "kernels"}, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
