#!/usr/bin/env python3
"""Development timing of the density screen of the plain render ("The screen"), one 400x400 frame at 128 + 64
samples, coarse fp16x3 + fine fp16mx, HIP events on the launch stream, the variants interleaved.

    python tools/time_density_screen.py --step0 [--out FILE]   THE STEP-0 GATE, on the depths of a real render: p_c / p_f = the
                                                               screen launches of the two passes, c = the dense coarse launch,
                                                               today's fine pass (the frame without screens less its coarse
                                                               half, timed piece by piece), the two list launches on the frame's
                                                               own candidates; C*_coarse = 1 - p_c / c, C*_fine from
                                                               p_f + C f_list = today's fine pass; the candidate shares of
                                                               poses 0..119
    python tools/time_density_screen.py [--all-live] [--out FILE]   the whole frame with the screens OFF, the coarse one ON, the
                                                               fine one ON, both ON, and AUTO (--all-live: sigma-head biases
                                                               + 1000 on both networks -- every sample a candidate, where a
                                                               screen can only lose and AUTO has to stay dense)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from tgtc_style_amd import hip, models, rendering, synth, utils

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


def build_nets(all_live):
    if not all_live:
        return bench.build_nets("fp16x3+fp16mx")
    nets = []
    for (seed, mode), prec in zip(((0, "coarse"), (1, "fine")), ("fp16x3", "fp16mx")):
        state = {k: np.array(v) for k, v in synth.nerf_state(seed).items()}
        state["net.sigma_layer.bias"] = state["net.sigma_layer.bias"] + 1000.
        m = models.StyleNerf(type("A", (bench.NetArgs,), {"precision": prec}), mode=mode)
        m.load_state_dict(bench.t_state(state))
        nets.append(m.cuda())
    return nets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step0", action="store_true")
    ap.add_argument("--all-live", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--poses", type=int, default=120, help="--step0: candidate shares over spiral poses 0 .. poses-1")
    ap.add_argument("--out")
    args = ap.parse_args()

    lib = hip.load()
    focal = synth.fern_intrinsics(H, W)
    coarse, fine = build_nets(args.all_live)
    hc, hf = coarse.packed(), fine.packed()
    hc.enable_screen()
    hf.enable_screen()
    m_c, m_f = hc.screen_margin(), hf.screen_margin()
    R = H * W
    result = {"shape": "%d rays x %d depths (128 coarse + 64 fine), coarse fp16x3 + fine fp16mx" % (R, NT), "rounds": args.rounds,
              "margin_coarse": m_c, "margin_fine": m_f}
    print("margins: coarse %.4f  fine %.4f" % (m_c, m_f), flush=True)

    if args.step0:
        ws = torch.empty(lib.tgtc_render_workspace_bytes(R, NC, NF), dtype=torch.uint8, device="cuda")
        wsf = ws.view(torch.float32)
        assert (R * NC * 4) % 256 == 0 and (R * NT * 4) % 256 == 0      # the planes are then contiguous
        ts_c, sigma_c = wsf[:R * NC], wsf[R * NC:2 * R * NC]
        ts_f = wsf[6 * R * NC:6 * R * NC + R * NT]
        sigma_f = wsf[6 * R * NC + R * NT:6 * R * NC + 2 * R * NT]
        rgb_img, t_img = torch.empty(R, 3, device="cuda"), torch.empty(R, device="cuda")
        hc.set_screen(hip.SCREEN_OFF)
        hf.set_screen(hip.SCREEN_OFF)
        hf.set_cull(hip.CULL_OFF)          # the dense fine pass leaves the exact density of every sample in sigma_f

        def frame(pose):
            o, d = utils.gen_rays(H, W, focal, synth.spiral_pose(pose))
            o, d = o.contiguous(), d.contiguous()
            hip.check(lib.tgtc_render_rays_plain(hc.handle, hf.handle, hip.ptr(o), hip.ptr(d), R, NC, NF, 0., 1., None,
                                                 hip.PATH_CHAIN, hip.ptr(ws), ws.numel(), hip.ptr(rgb_img), hip.ptr(t_img), None,
                                                 None, hip.stream()))
            return o, d

        o, d = frame(0)
        torch.cuda.synchronize()
        tc, tf = ts_c.clone(), ts_f.clone()
        sig_c, sig_f = torch.empty(R * NC, device="cuda"), torch.empty(R * NT, device="cuda")
        hip.check(lib.tgtc_nerf_screen_rays(hc.handle, hip.ptr(o), hip.ptr(d), hip.ptr(tc), R, NC, hip.ptr(sig_c), hip.stream()))
        hip.check(lib.tgtc_nerf_screen_rays(hf.handle, hip.ptr(o), hip.ptr(d), hip.ptr(tf), R, NT, hip.ptr(sig_f), hip.stream()))
        torch.cuda.synchronize()
        result["screen_error_pose0"] = {"coarse_max": float((sig_c - sigma_c).abs().max()), "fine_max": float((sig_f - sigma_f).abs().max())}
        cand_c = torch.nonzero(~(sig_c <= -m_c)).flatten().to(torch.int32).contiguous()
        cand_f = torch.nonzero(~(sig_f <= -m_f)).flatten().to(torch.int32).contiguous()
        n_c = torch.tensor([cand_c.numel()], dtype=torch.int32, device="cuda")
        n_f = torch.tensor([cand_f.numel()], dtype=torch.int32, device="cuda")
        result["candidates_pose0"] = {"coarse": cand_c.numel() / (R * NC), "fine": cand_f.numel() / (R * NT)}
        out_c, out_f, rgb = torch.empty(R * NC, device="cuda"), torch.empty(R * NT, device="cuda"), torch.empty(R * NT, 3, device="cuda")
        w_c = torch.empty(R * NC, device="cuda")
        # today's fine pass: AUTO's choice on a landed share, with the stash RayRenderer attaches
        today = rendering.RayRenderer(coarse, fine, fused=False, screen=False)
        today.render(o, d, NC, NF)
        torch.cuda.synchronize()
        st = hip.stream()
        calls = {
            "p_c_screen_coarse": lambda: hip.check(lib.tgtc_nerf_screen_rays(hc.handle, hip.ptr(o), hip.ptr(d), hip.ptr(tc), R, NC, hip.ptr(out_c), st)),
            "c_dense_coarse": lambda: hip.check(lib.tgtc_nerf_forward_rays(hc.handle, hip.ptr(o), hip.ptr(d), hip.ptr(tc), R, NC, None, hip.ptr(out_c), st)),
            "sigma_list_coarse_candidates": lambda: hip.check(lib.tgtc_nerf_sigma_list(
                hc.handle, hip.ptr(o), hip.ptr(d), hip.ptr(tc), R, NC, hip.ptr(cand_c), hip.ptr(n_c), hip.ptr(out_c), st)),
            "p_f_screen_fine": lambda: hip.check(lib.tgtc_nerf_screen_rays(hf.handle, hip.ptr(o), hip.ptr(d), hip.ptr(tf), R, NT, hip.ptr(out_f), st)),
            "full_list_fine_candidates": lambda: hip.check(lib.tgtc_nerf_forward_list_sigma(
                hf.handle, hip.ptr(o), hip.ptr(d), hip.ptr(tf), R, NT, hip.ptr(cand_f), hip.ptr(n_f), hip.ptr(rgb), hip.ptr(out_f), st)),
            "frame_today": lambda: today.render(o, d, NC, NF),
            "sample_coarse": lambda: hip.check(lib.tgtc_sample_coarse(hip.ptr(o), hip.ptr(d), R, NC, 0., 1., None, None, hip.ptr(w_c), st)),
            "coarse_to_fine": lambda: hip.check(lib.tgtc_coarse_to_fine(hip.ptr(sigma_c), hip.ptr(tc), R, NC, NF, hip.ptr(out_f), None, st)),
        }
        t = timed(calls, args.rounds)
        result["kernels"] = {k: stats(v) for k, v in t.items()}
        mean = {k: float(np.mean(v)) for k, v in t.items()}
        p_c, c, p_f = mean["p_c_screen_coarse"], mean["c_dense_coarse"], mean["p_f_screen_fine"]
        fine_today = mean["frame_today"] - mean["sample_coarse"] - c - mean["coarse_to_fine"]
        rate_c = mean["sigma_list_coarse_candidates"] / max(cand_c.numel(), 1)
        rate_f = mean["full_list_fine_candidates"] / max(cand_f.numel(), 1)
        result.update({"p_c_ms": p_c, "c_ms": c, "p_f_ms": p_f, "fine_pass_today_ms": fine_today,
                       "coarse_list_ns_per_sample": rate_c * 1e6, "fine_list_ns_per_sample": rate_f * 1e6,
                       "C_star_coarse": 1.0 - p_c / c, "C_star_coarse_by_list_rate": (c - p_c) / (rate_c * R * NC),
                       "C_star_fine": (fine_today - p_f) / (rate_f * R * NT)})
        print("p_c = %.3f ms  c = %.3f ms  C*_coarse = %.4f (by the list's rate %.4f)" % (p_c, c, 1 - p_c / c, result["C_star_coarse_by_list_rate"]))
        print("p_f = %.3f ms  fine pass today = %.3f ms  full list %.2f ns/sample  C*_fine = %.4f" % (p_f, fine_today, rate_f * 1e6, result["C_star_fine"]), flush=True)
        hf.set_cull(hip.CULL_OFF)          # (the renderer above put AUTO back)
        hf.set_stash(None)
        shares = []
        for pose in range(args.poses):
            frame(pose)
            shares.append(torch.stack([(~(sigma_c <= -m_c)).float().mean(), (~(sigma_f <= -m_f)).float().mean(),
                                       (sigma_c > 0).float().mean(), (sigma_f > 0).float().mean()]))
        shares = torch.stack(shares).cpu().numpy()
        for j, name in enumerate(("candidate_share_coarse", "candidate_share_fine", "live_share_coarse", "live_share_fine")):
            col = shares[:, j]
            result[name + "_poses"] = {"poses": args.poses, "min": float(col.min()), "max": float(col.max()), "mean": float(col.mean()),
                                       "max_step_between_consecutive_poses": float(np.abs(np.diff(col)).max()) if len(col) > 1 else 0.0}
            print("%s over %d poses: min %.4f  mean %.4f  max %.4f" % (name, args.poses, col.min(), col.mean(), col.max()), flush=True)
    else:
        rays = [utils.gen_rays(H, W, focal, synth.spiral_pose(i)) for i in range(2)]
        modes = (("OFF", False), ("COARSE_ON", (True, False)), ("FINE_ON", (False, True)), ("ON", True), ("AUTO", None))
        renderers = {mode: rendering.RayRenderer(coarse, fine, fused=False, screen=screen) for mode, screen in modes}

        def call(mode, i=[0]):
            i[0] += 1
            return renderers[mode].render(*rays[i[0] % 2], NC, NF, near=0., far=1.)   # (every render puts its modes on the handles)
        for mode in renderers:     # landed statistics for AUTO
            call(mode)
            torch.cuda.synchronize()
        before = (hc.screened_renders(), hf.screened_renders())
        t = timed({m: (lambda m=m: call(m)) for m in renderers}, args.rounds)
        result["frame"] = {m: stats(v) for m, v in t.items()}
        result["screened_renders_during_timing"] = {"coarse": hc.screened_renders() - before[0], "fine": hf.screened_renders() - before[1]}
        result["screen_fraction"] = {"coarse": hc.screen_fraction(), "fine": hf.screen_fraction()}
        result["live_fraction_fine"] = hf.live_fraction()
        for m, v in t.items():
            print("frame, screen %-9s %8.3f ms (min %.3f, max %.3f)" % (m, np.mean(v), np.min(v), np.max(v)), flush=True)
        print("screened during timing:", result["screened_renders_during_timing"], "shares:", result["screen_fraction"], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
