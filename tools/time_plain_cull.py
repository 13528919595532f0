#!/usr/bin/env python3
"""Development timing of the two-phase fine pass of the plain render ("densities first"), one 400x400 frame at
128 + 64 samples, coarse fp16x3 + fine fp16mx, HIP events on the launch stream, the variants interleaved.

    python tools/time_plain_cull.py --step0 [--out FILE]     THE STEP-0 GATE: f = the full fine launch (tgtc_nerf_forward_rays
                                                             with rgb), s = the same launch with rgb = NULL, on the fine depths
                                                             of a real render; L* = 1 - s/f; the live share of poses 0..119
    python tools/time_plain_cull.py [--all-live] [--out FILE]  f, s, the list launch on the frame's own list, and the whole
                                                             frame under cull OFF / ON / AUTO (--all-live: a fine network whose
                                                             density is positive everywhere, where culling can only lose)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from tgtc_style_amd import hip, rendering, synth, utils

H = W = 400
NC, NF = 128, 64
NT = NC + NF


def timed(calls, rounds):
    """{name: fn} -> {name: [ms per round]}, the calls interleaved inside every round."""
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(rounds)] for k in calls}
    for i in range(rounds):
        for k, fn in calls.items():
            ev[k][i][0].record()
            fn()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in ev[k]] for k in calls}


def stats(ms):
    return {"mean_ms": float(np.mean(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "runs": [round(m, 4) for m in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step0", action="store_true")
    ap.add_argument("--all-live", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--poses", type=int, default=120, help="--step0: live share over spiral poses 0 .. poses-1")
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
    ws = torch.empty(lib.tgtc_render_workspace_bytes(R, NC, NF), dtype=torch.uint8, device="cuda")
    wsf = ws.view(torch.float32)
    assert (R * NC * 4) % 256 == 0 and (R * NT * 4) % 256 == 0      # the planes are then contiguous
    ts_f = wsf[6 * R * NC:6 * R * NC + R * NT]
    sigma_f = wsf[6 * R * NC + R * NT:6 * R * NC + 2 * R * NT]
    rgb_img, t_img = torch.empty(R, 3, device="cuda"), torch.empty(R, device="cuda")

    def frame(pose):
        o, d = utils.gen_rays(H, W, focal, synth.spiral_pose(pose))
        o, d = o.contiguous(), d.contiguous()
        hip.check(lib.tgtc_render_rays_plain(coarse.packed().handle, fine.packed().handle, hip.ptr(o), hip.ptr(d), R, NC, NF, 0., 1.,
                                             None, hip.PATH_CHAIN, hip.ptr(ws), ws.numel(), hip.ptr(rgb_img), hip.ptr(t_img), None,
                                             None, hip.stream()))
        return o, d

    result = {"shape": "%d rays x %d depths (128 coarse + 64 fine), coarse fp16x3 + fine fp16mx" % (R, NT), "rounds": args.rounds}
    o, d = frame(0)
    torch.cuda.synchronize()
    ts = ts_f.clone().view(R, NT)
    live_mask = sigma_f.clone() > 0
    result["live_share_pose0"] = float(live_mask.float().mean())
    rgb = torch.empty(R * NT, 3, device="cuda")
    sigma = torch.empty(R * NT, device="cuda")
    h = fine.packed().handle
    calls = {
        "f_full_fine_launch": lambda: hip.check(lib.tgtc_nerf_forward_rays(h, hip.ptr(o), hip.ptr(d), hip.ptr(ts), R, NT, hip.ptr(rgb), hip.ptr(sigma), hip.stream())),
        "s_density_only_launch": lambda: hip.check(lib.tgtc_nerf_forward_rays(h, hip.ptr(o), hip.ptr(d), hip.ptr(ts), R, NT, None, hip.ptr(sigma), hip.stream())),
    }
    if not args.step0:
        live = torch.nonzero(live_mask).flatten().to(torch.int32).contiguous()
        n_live = torch.tensor([live.numel()], dtype=torch.int32, device="cuda")
        calls["list_launch_on_the_frames_list"] = lambda: hip.check(lib.tgtc_nerf_forward_list(
            h, hip.ptr(o), hip.ptr(d), hip.ptr(ts), R, NT, hip.ptr(live), hip.ptr(n_live), hip.ptr(rgb), hip.stream()))
        result["list_entries"] = int(live.numel())
    t = timed(calls, args.rounds)
    result["kernels"] = {k: stats(v) for k, v in t.items()}
    f, s = np.mean(t["f_full_fine_launch"]), np.mean(t["s_density_only_launch"])
    result["f_ms"], result["s_ms"], result["L_star"] = float(f), float(s), float(1.0 - s / f)
    print("f = %.3f ms   s = %.3f ms   L* = 1 - s/f = %.4f   live share (pose 0) = %.4f" % (f, s, 1 - s / f, result["live_share_pose0"]), flush=True)

    if args.step0:
        shares = []
        for pose in range(args.poses):
            frame(pose)
            shares.append((sigma_f > 0).float().mean())
        shares = torch.stack(shares).cpu().numpy()
        result["live_share_poses"] = {"poses": args.poses, "min": float(shares.min()), "max": float(shares.max()),
                                      "mean": float(shares.mean()),
                                      "max_step_between_consecutive_poses": float(np.abs(np.diff(shares)).max()) if len(shares) > 1 else 0.0}
        print("live share over %d poses: min %.4f  mean %.4f  max %.4f  largest step %.4f" % (
            args.poses, shares.min(), shares.mean(), shares.max(), result["live_share_poses"]["max_step_between_consecutive_poses"]), flush=True)
    else:
        rays = [utils.gen_rays(H, W, focal, synth.spiral_pose(i)) for i in range(2)]
        renderers = {mode: rendering.RayRenderer(coarse, fine, fused=False, cull=cull, screen=False)
                     for mode, cull in (("OFF", False), ("ON", True), ("AUTO", None))}
        # one handle carries the mode: set it before every call
        def call(mode, i=[0]):
            renderers[mode].apply_cull()
            i[0] += 1
            return renderers[mode].render(*rays[i[0] % 2], NC, NF, near=0., far=1.)
        for mode in renderers:     # a landed statistic for AUTO
            call(mode)
            torch.cuda.synchronize()
        before = fine.packed().culled_renders()
        t = timed({m: (lambda m=m: call(m)) for m in renderers}, args.rounds)
        result["frame"] = {m: stats(v) for m, v in t.items()}
        result["culled_renders_during_timing"] = fine.packed().culled_renders() - before
        result["live_fraction"] = fine.packed().live_fraction()
        for m, v in t.items():
            print("frame, cull %-4s %8.3f ms (min %.3f, max %.3f)" % (m, np.mean(v), np.min(v), np.max(v)), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
