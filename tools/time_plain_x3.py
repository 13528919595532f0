#!/usr/bin/env python3
"""Development timing of the two-phase fine pass for a fine handle in fp16x3: 400 x 400 synthetic fern frames at
128 + 64 samples, the benchmark's orbit poses, both handles in fp16x3, four forms of the plain render in ONE process:

    a  RayRenderer(fused=True)                                    today's default: the ray kernel
    b  RayRenderer(fused=False, cull=False)                       the dense chain
    c  RayRenderer(fused=False, cull=True, screen=(None, False))  two-phase, fine pass unscreened
    d  RayRenderer(fused=False, cull=True, screen=True)           two-phase behind the density screen

alternated over --rounds rounds after a warm-up, every frame a host clock around a render that ends in a device
synchronise.  (c) and (d) must give the bits of (b) on every frame timed: asserted.  The yardsticks are (a) and (b) of the same
process, never a number from another run.

    python tools/time_plain_x3.py [--rounds N] [--step0] [--out profiles/plain_x3_two_phase_timing.json]

--step0 adds the isolated launches on the fine depths of a real render (pose 0), HIP events on the launch stream, interleaved:
p the screen launch, c the dense full launch, s the dense sigma-only launch, l the full list launch (rgb + sigma) on the
frame's candidates and (rgb only) on its live samples -- what the pass-3 threshold of tgtc_screen_auto_decision is derived from
(csrc/render.hip, the comment above kScreenFineX3Threshold) -- and the live / candidate shares of poses 0 .. --poses - 1."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from tgtc_style_amd import hip, rendering, synth, utils

H = W = 400
NC, NF = 128, 64
NT = NC + NF
FORMS = (("a_ray_kernel", dict(fused=True)),
         ("b_dense_chain", dict(fused=False, cull=False)),
         ("c_two_phase", dict(fused=False, cull=True, screen=(None, False))),
         ("d_two_phase_screened", dict(fused=False, cull=True, screen=True)))


def stats(ms):
    return {"mean_ms": float(np.mean(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "runs": [round(m, 4) for m in ms]}


def timed_events(calls, rounds):
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


def frames(coarse, fine, rounds, n_poses, result):
    focal = synth.fern_intrinsics(H, W)
    rays = [tuple(x.contiguous() for x in utils.gen_rays(H, W, focal, synth.spiral_pose(i))) for i in range(n_poses)]
    renderers = {name: rendering.RayRenderer(coarse, fine, **kw) for name, kw in FORMS}
    hf = fine.packed()

    def render(name, pose):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = renderers[name].render(*rays[pose], NC, NF, near=0., far=1.)      # (every render puts its modes on the handles)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for name in renderers:                      # warm-up: code objects, workspaces, the screens' calibration, landed shares
        for pose in range(n_poses):
            render(name, pose)
    ms = {name: [] for name in renderers}
    counters = {"culled": 0, "screened": 0}
    shares = {"live": [], "candidates": []}
    for rnd in range(rounds):
        for pose in range(n_poses):
            outs = {}
            for name in renderers:
                before = hf.culled_renders(), hf.screened_renders()
                t, out = render(name, pose)
                ms[name].append(t)
                outs[name] = {k: v.clone() for k, v in out.items()}
                took = hf.culled_renders() - before[0], hf.screened_renders() - before[1]
                assert took == {"a_ray_kernel": (0, 0), "b_dense_chain": (0, 0), "c_two_phase": (1, 0),
                                "d_two_phase_screened": (1, 1)}[name], (name, took)
                if name == "d_two_phase_screened":
                    shares["live"].append(hf.live_fraction())
                    shares["candidates"].append(hf.screen_fraction())
            for name in ("c_two_phase", "d_two_phase_screened"):
                for k in ("rgb", "t"):
                    assert torch.equal(outs[name][k], outs["b_dense_chain"][k]), (name, k, rnd, pose)
            counters["culled"] += 2
            counters["screened"] += 1
    result["frame"] = {name: stats(v) for name, v in ms.items()}
    result["frames_timed_per_form"] = rounds * n_poses
    result["bits"] = "c and d equal b (rgb, t) on every frame timed"
    result["two_phase_renders_during_timing"] = counters
    result["live_fraction_fine"] = {"min": min(shares["live"]), "max": max(shares["live"])}
    result["screen_fraction_fine"] = {"min": min(shares["candidates"]), "max": max(shares["candidates"])}
    for name, v in ms.items():
        print("frame %-22s %8.3f ms (min %.3f, max %.3f)" % (name, np.mean(v), np.min(v), np.max(v)), flush=True)
    print("shares: live", result["live_fraction_fine"], "candidates", result["screen_fraction_fine"], flush=True)
    d, a, b = (float(np.mean(ms[k])) for k in ("d_two_phase_screened", "a_ray_kernel", "b_dense_chain"))
    result["d_beats_a_and_b"] = bool(d < a and d < b)


def step0(coarse, fine, rounds, n_poses, result):
    lib = hip.load()
    hc, hf = coarse.packed(), fine.packed()
    R = H * W
    focal = synth.fern_intrinsics(H, W)
    ws = torch.empty(lib.tgtc_render_workspace_bytes(R, NC, NF), dtype=torch.uint8, device="cuda")
    wsf = ws.view(torch.float32)
    assert (R * NC * 4) % 256 == 0 and (R * NT * 4) % 256 == 0      # the planes are then contiguous
    ts_f = wsf[6 * R * NC:6 * R * NC + R * NT]
    sigma_f = wsf[6 * R * NC + R * NT:6 * R * NC + 2 * R * NT]
    rgb_img, t_img = torch.empty(R, 3, device="cuda"), torch.empty(R, device="cuda")
    if not hf.screen_tried:
        hf.enable_screen()
    m_f = hf.screen_margin()
    hc.set_screen(hip.SCREEN_OFF)
    hf.set_cull(hip.CULL_OFF)              # the dense fine pass leaves the exact density of every sample in sigma_f

    def frame(pose):
        o, d = (x.contiguous() for x in utils.gen_rays(H, W, focal, synth.spiral_pose(pose)))
        hip.check(lib.tgtc_render_rays_plain(hc.handle, hf.handle, hip.ptr(o), hip.ptr(d), R, NC, NF, 0., 1., None,
                                             hip.PATH_CHAIN, hip.ptr(ws), ws.numel(), hip.ptr(rgb_img), hip.ptr(t_img), None,
                                             None, hip.stream()))
        return o, d

    o, d = frame(0)
    torch.cuda.synchronize()
    tf = ts_f.clone()
    sig = torch.empty(R * NT, device="cuda")
    hip.check(lib.tgtc_nerf_screen_rays(hf.handle, hip.ptr(o), hip.ptr(d), hip.ptr(tf), R, NT, hip.ptr(sig), hip.stream()))
    torch.cuda.synchronize()
    cand = torch.nonzero(~(sig <= -m_f)).flatten().to(torch.int32).contiguous()
    live = torch.nonzero(sigma_f > 0).flatten().to(torch.int32).contiguous()
    n_cand = torch.tensor([cand.numel()], dtype=torch.int32, device="cuda")
    n_live = torch.tensor([live.numel()], dtype=torch.int32, device="cuda")
    out_sigma, rgb = torch.empty(R * NT, device="cuda"), torch.empty(R * NT, 3, device="cuda")
    st = hip.stream()
    rays_args = (hip.ptr(o), hip.ptr(d), hip.ptr(tf), R, NT)
    calls = {
        "p_screen": lambda: hip.check(lib.tgtc_nerf_screen_rays(hf.handle, *rays_args, hip.ptr(out_sigma), st)),
        "c_dense_full": lambda: hip.check(lib.tgtc_nerf_forward_rays(hf.handle, *rays_args, hip.ptr(rgb), hip.ptr(out_sigma), st)),
        "s_dense_sigma": lambda: hip.check(lib.tgtc_nerf_forward_rays(hf.handle, *rays_args, None, hip.ptr(out_sigma), st)),
        "l_list_candidates": lambda: hip.check(lib.tgtc_nerf_forward_list_x3(
            hf.handle, *rays_args, hip.ptr(cand), hip.ptr(n_cand), hip.ptr(rgb), hip.ptr(out_sigma), st)),
        "l_list_live": lambda: hip.check(lib.tgtc_nerf_forward_list_x3(
            hf.handle, *rays_args, hip.ptr(live), hip.ptr(n_live), hip.ptr(rgb), None, st)),
    }
    t = timed_events(calls, rounds)
    mean = {k: float(np.mean(v)) for k, v in t.items()}
    p, c, s = mean["p_screen"], mean["c_dense_full"], mean["s_dense_sigma"]
    rate = mean["l_list_candidates"] / max(cand.numel(), 1)
    rate_live = mean["l_list_live"] / max(live.numel(), 1)
    l = rate * R * NT
    out = {"margin_fine": m_f, "kernels": {k: stats(v) for k, v in t.items()},
           "candidates_pose0": cand.numel() / (R * NT), "live_pose0": live.numel() / (R * NT),
           "p_ms": p, "c_ms": c, "s_ms": s, "list_ns_per_listed_sample": rate * 1e6, "list_live_ns_per_listed_sample": rate_live * 1e6,
           "l_ms": l, "C_star": (c - p) / l, "L_star_unscreened": (c - s) / (rate_live * R * NT)}
    print("step0: p = %.3f ms  c = %.3f ms  s = %.3f ms  list %.3f ns per listed sample (l = %.3f ms)  C* = %.4f  L* = %.4f"
          % (p, c, s, rate * 1e6, l, out["C_star"], out["L_star_unscreened"]), flush=True)
    shares = []
    for pose in range(n_poses):
        o, d = frame(pose)
        hip.check(lib.tgtc_nerf_screen_rays(hf.handle, hip.ptr(o), hip.ptr(d), hip.ptr(ts_f), R, NT, hip.ptr(sig), hip.stream()))
        shares.append(torch.stack([(~(sig <= -m_f)).float().mean(), (sigma_f > 0).float().mean()]))
    shares = torch.stack(shares).cpu().numpy()
    for j, name in enumerate(("candidate_share_fine", "live_share_fine")):
        col = shares[:, j]
        out[name + "_poses"] = {"poses": n_poses, "min": float(col.min()), "max": float(col.max()), "mean": float(col.mean())}
        print("%s over %d poses: min %.4f  mean %.4f  max %.4f" % (name, n_poses, col.min(), col.mean(), col.max()), flush=True)
    spread = out["candidate_share_fine_poses"]["max"] - out["candidate_share_fine_poses"]["min"]
    out["launch_margin"] = 0.005
    out["derived_threshold"] = out["C_star"] - spread - out["launch_margin"]
    print("derived pass-3 threshold: %.4f - %.4f - 0.005 = %.4f" % (out["C_star"], spread, out["derived_threshold"]), flush=True)
    result["step0"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step0", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frame-poses", type=int, default=2, help="orbit poses 0 .. n-1 rendered by every form in every round")
    ap.add_argument("--poses", type=int, default=120, help="--step0: shares over spiral poses 0 .. poses-1")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("at least three rounds")
    coarse, fine = bench.build_nets("fp16x3")
    result = {"shape": "%d rays x %d depths (128 coarse + 64 fine), coarse fp16x3 + fine fp16x3" % (H * W, NT), "rounds": args.rounds,
              "timer": "host clock around render + device synchronise (frames); HIP events, interleaved (step0)"}
    with torch.no_grad():
        frames(coarse, fine, args.rounds, args.frame_poses, result)
        if args.step0:
            step0(coarse, fine, args.rounds, args.poses, result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
