#!/usr/bin/env python3
"""Development timing of the stashed two-phase fine pass (csrc/mlp_nerf_mx2_stash.hip), one 400x400 frame at
128 + 64 samples, coarse fp16x3 + fine fp16mx, HIP events on the launch stream, the variants interleaved.

    python tools/time_fine_stash.py [--all-live] [--out FILE]
        launches on the fine depths of a real render: the density-only launch against the producer (tgtc_nerf_stash_fill, its
        scratch memset included), the list launch on the frame's own list against the heads-only launch;
        the whole frame under cull OFF, ON without a stash, ON with the stash, AUTO with the stash
        (--all-live: a fine network whose density is positive everywhere -- AUTO must stay dense and cost what OFF costs)
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
    ap.add_argument("--all-live", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()

    lib = hip.load()
    focal = synth.fern_intrinsics(H, W)
    if args.all_live:
        from tgtc_style_amd import models
        state = {k: np.array(v) for k, v in synth.nerf_state(1).items()}
        state["net.sigma_layer.weight"][:] = 0.
        state["net.sigma_layer.bias"][:] = 1.
        coarse, _ = bench.build_nets("fp16x3+fp16mx")
        fine = models.StyleNerf(type("A", (bench.NetArgs,), {"precision": "fp16mx"}), mode="fine")
        fine.load_state_dict(bench.t_state(state))
        fine = fine.cuda()
    else:
        coarse, fine = bench.build_nets("fp16x3+fp16mx")
    R = H * W
    net = fine.packed()
    result = {"shape": "%d rays x %d depths (128 coarse + 64 fine), coarse fp16x3 + fine fp16mx" % (R, NT), "rounds": args.rounds}
    stash = torch.empty(lib.tgtc_net_stash_bytes(R, NT, rendering.RayRenderer.STASH_SHARE), dtype=torch.uint8, device="cuda")
    result["stash_bytes"] = stash.numel()

    if not args.all_live:
        # the fine depths and the list of a real frame
        r = rendering.RayRenderer(coarse, fine, fused=False, cull=False, screen=False)
        o, d = (x.contiguous() for x in utils.gen_rays(H, W, focal, synth.spiral_pose(0)))
        r.render(o, d, NC, NF, near=0., far=1.)
        torch.cuda.synchronize()
        wsf = r._ws.view(torch.float32)
        ts = wsf[6 * R * NC:6 * R * NC + R * NT].clone().view(R, NT)
        live_mask = wsf[6 * R * NC + R * NT:6 * R * NC + 2 * R * NT].clone() > 0
        result["live_share_pose0"] = float(live_mask.float().mean())
        live = torch.nonzero(live_mask).flatten().to(torch.int32).contiguous()
        n_live = torch.tensor([live.numel()], dtype=torch.int32, device="cuda")
        rgb = torch.empty(R * NT, 3, device="cuda")
        sigma = torch.empty(R * NT, device="cuda")
        scratch = torch.empty(2048, dtype=torch.int32, device="cuda")
        ovf = torch.empty(R * NT, dtype=torch.int32, device="cuda")
        net.set_stash(stash)
        h = net.handle
        a = (hip.ptr(o), hip.ptr(d), hip.ptr(ts), R, NT)
        calls = {
            "density_only_launch": lambda: hip.check(lib.tgtc_nerf_forward_rays(h, *a, None, hip.ptr(sigma), hip.stream())),
            "producer_launch": lambda: hip.check(lib.tgtc_nerf_stash_fill(h, *a, hip.ptr(sigma), hip.ptr(scratch), hip.ptr(ovf), hip.stream())),
            "list_launch_on_the_frames_list": lambda: hip.check(lib.tgtc_nerf_forward_list(h, *a, hip.ptr(live), hip.ptr(n_live), hip.ptr(rgb), hip.stream())),
            "heads_launch": lambda: hip.check(lib.tgtc_nerf_stash_heads(h, hip.ptr(o), hip.ptr(d), R, NT, hip.ptr(scratch), hip.ptr(rgb), hip.stream())),
        }
        t = timed(calls, args.rounds)
        torch.cuda.synchronize()
        result["kernels"] = {k: stats(v) for k, v in t.items()}
        result["list_entries"], result["overflow_entries"] = int(live.numel()), int(scratch[0])
        for k, v in t.items():
            print("%-32s %8.3f ms (min %.3f, max %.3f)" % (k, np.mean(v), np.min(v), np.max(v)), flush=True)
        print("list %d entries, overflow %d" % (result["list_entries"], result["overflow_entries"]), flush=True)
        net.set_stash(None)

    rays = [utils.gen_rays(H, W, focal, synth.spiral_pose(i)) for i in range(2)]
    renderers = {"OFF": rendering.RayRenderer(coarse, fine, fused=False, cull=False, screen=False),
                 "ON_no_stash": rendering.RayRenderer(coarse, fine, fused=False, cull=True, stash=False, screen=False),
                 "ON_stash": rendering.RayRenderer(coarse, fine, fused=False, cull=True, stash=stash, screen=False),
                 "AUTO_stash": rendering.RayRenderer(coarse, fine, fused=False, cull=None, stash=stash, screen=False)}
    if args.all_live:      # culling can only lose here: time what the default does against OFF, and OFF against itself
        renderers = {"OFF": renderers["OFF"], "OFF_again": rendering.RayRenderer(coarse, fine, fused=False, cull=False, screen=False),
                     "AUTO_stash": renderers["AUTO_stash"]}

    def call(mode, i=[0]):
        i[0] += 1
        return renderers[mode].render(*rays[i[0] % 2], NC, NF, near=0., far=1.)
    for mode in renderers:     # a landed statistic for AUTO
        call(mode)
        torch.cuda.synchronize()
    before = net.culled_renders()
    t = timed({m: (lambda m=m: call(m)) for m in renderers}, args.rounds)
    result["frame"] = {m: stats(v) for m, v in t.items()}
    result["culled_renders_during_timing"] = net.culled_renders() - before
    result["live_fraction"] = net.live_fraction()
    for m, v in t.items():
        print("frame, cull %-12s %8.3f ms (min %.3f, max %.3f)" % (m, np.mean(v), np.min(v), np.max(v)), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
