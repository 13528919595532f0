#!/usr/bin/env python3
"""Timing of the chain geometry of the culled stylised frame and of the geometry build (csrc/render.hip:
ray_geometry, fine_sigma_pass): the frame, pose, shapes and schedule of tools/time_sparse_mx.py (400x400 fern-shaped, pose 5,
R = 160 000, 128c + 64f), K in {1, 2, 4} frame-constant latents, one process, the variants interleaved.

    python tools/time_screen_geometry.py --step0 [--poses N]
        THE FIGURES OF THE THRESHOLD of pass 2 (kScreenFineSigmaThreshold), for a fine handle in fp16mx and in fp16x3, on the fine
        depths of a real render of the frame: p = the screen launch, s = the dense sigma-only launch, l = the sigma list launch
        on the frame's own candidates scaled to all samples; C* = (s - p) / l.  The candidate share of the fine pass over
        spiral poses 0 .. N-1 (its spread is the margin the threshold gives away).
    python tools/time_screen_geometry.py
        (i)  the frame of the headline pair: A = render_latents(zs [K,32], min_weight=0, style_precision="fp16mx"),
             B = the same with geometry="chain", screens OFF / ON / AUTO, after one warm-up render has landed the shares;
             the same for the all-fp16x3 pair (A = render_latents(zs [K,32], min_weight=0));
        (ii) build_geometry in both geometries (each build has its one synchronisation inside);
        (iii) every sample a candidate (sigma-head biases + 1000): B under AUTO against B with the screens OFF.
        B counts as faster only if every B round is below every A round by more than A's spread.  For information: the share
        of rays whose A and B pixels differ by more than 1e-3 (two coarse kernels: the sampler's ill-conditioned rays of
        DESIGN section 4).

Both write into profiles/screen_geometry_timing.json ("step0" and "frames"), keeping the other part.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tgtc_style_amd import hip, models, rendering, synth, utils  # noqa: E402

H = W = 400
NC, NF = 128, 64
NT = NC + NF
KS = (1, 2, 4)
ROUNDS, RENDERS = 3, 5
PAIRS = {"fp16x3+fp16mx": {"style_precision": "fp16mx"}, "fp16x3": {}}
SCREENS = {"B_off": False, "B_on": True, "B_auto": None}


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
    return {name: {"ms": v, "ms_mean": sum(v) / len(v), "spread_rel": (max(v) - min(v)) / (sum(v) / len(v))} for name, v in ms.items()}


def below(rec, b, a):
    """Is every round of b below every round of a by more than a's spread?"""
    va, vb = rec[a]["ms"], rec[b]["ms"]
    return min(va) - max(vb) > max(va) - min(va)


def line(title, rec):
    return title + "   ".join("%s %7.2f ms [%s]" % (n, r["ms_mean"], " ".join("%.2f" % x for x in r["ms"])) for n, r in rec.items()
                              if isinstance(r, dict) and "ms" in r)


def make(precision, shift=0.0):
    """(coarse, fine, style pair) of bench.make_renderer, the sigma heads' biases shifted"""
    r = bench.make_renderer(precision, True)
    if shift:
        precs = (precision.split("+") * 2)[:2]
        nets = []
        for (seed, mode), prec in zip(((0, "coarse"), (1, "fine")), precs):
            state = {k: np.array(v) for k, v in synth.nerf_state(seed).items()}
            state["net.sigma_layer.bias"] = state["net.sigma_layer.bias"] + shift
            m = models.StyleNerf(type("A", (bench.NetArgs,), {"precision": prec}), mode=mode)
            m.load_state_dict(bench.t_state(state))
            nets.append(m.cuda())
        return nets[0], nets[1], r.style
    return r.coarse, r.fine, r.style


def step0(poses, rounds):
    lib = hip.load()
    focal = synth.fern_intrinsics(H, W)
    R = H * W
    assert (R * NC * 4) % 256 == 0 and (R * NT * 4) % 256 == 0      # the workspace's planes are then contiguous
    out = {"shape": "%d rays x %d fine depths (128 coarse + 64 fine) of pose 5" % (R, NT), "rounds": rounds}
    for precision in PAIRS:
        coarse, fine = bench.build_nets(precision)
        hc, hf = coarse.packed(), fine.packed()
        hf.enable_screen()
        m_f = hf.screen_margin()
        hf.set_screen(hip.SCREEN_OFF)
        hf.set_cull(hip.CULL_OFF)          # the dense fine pass leaves the exact density of every sample in sigma_f
        ws = torch.empty(lib.tgtc_render_workspace_bytes(R, NC, NF), dtype=torch.uint8, device="cuda")
        wsf = ws.view(torch.float32)
        ts_f = wsf[6 * R * NC:6 * R * NC + R * NT]
        sigma_f = wsf[6 * R * NC + R * NT:6 * R * NC + 2 * R * NT]
        rgb_img, t_img = torch.empty(R, 3, device="cuda"), torch.empty(R, device="cuda")

        def frame(pose):
            o, d = utils.gen_rays(H, W, focal, synth.spiral_pose(pose))
            o, d = o.contiguous(), d.contiguous()
            hip.check(lib.tgtc_render_rays_plain(hc.handle, hf.handle, hip.ptr(o), hip.ptr(d), R, NC, NF, 0., 1., None,
                                                 hip.PATH_CHAIN, hip.ptr(ws), ws.numel(), hip.ptr(rgb_img), hip.ptr(t_img), None,
                                                 None, hip.stream()))
            return o, d

        o, d = frame(5)
        torch.cuda.synchronize()
        tf, exact = ts_f.clone(), sigma_f.clone()
        sig = torch.empty(R * NT, device="cuda")
        hip.check(lib.tgtc_nerf_screen_rays(hf.handle, hip.ptr(o), hip.ptr(d), hip.ptr(tf), R, NT, hip.ptr(sig), hip.stream()))
        torch.cuda.synchronize()
        cand = torch.nonzero(~(sig <= -m_f)).flatten().to(torch.int32).contiguous()
        n = torch.tensor([cand.numel()], dtype=torch.int32, device="cuda")
        buf = torch.empty(R * NT, device="cuda")
        list_call = lib.tgtc_nerf_sigma_list_mx if hf.precision == "fp16mx" else lib.tgtc_nerf_sigma_list
        st = hip.stream()
        calls = {
            "p_screen": lambda: hip.check(lib.tgtc_nerf_screen_rays(hf.handle, hip.ptr(o), hip.ptr(d), hip.ptr(tf), R, NT, hip.ptr(buf), st)),
            "s_dense_sigma": lambda: hip.check(lib.tgtc_nerf_forward_rays(hf.handle, hip.ptr(o), hip.ptr(d), hip.ptr(tf), R, NT, None, hip.ptr(buf), st)),
            "sigma_list_candidates": lambda: hip.check(list_call(hf.handle, hip.ptr(o), hip.ptr(d), hip.ptr(tf), R, NT, hip.ptr(cand),
                                                                 hip.ptr(n), hip.ptr(buf), st)),
        }
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
        ms = {k: [a.elapsed_time(b) for a, b in ev[k]] for k in calls}
        mean = {k: float(np.mean(v)) for k, v in ms.items()}
        rate = mean["sigma_list_candidates"] / max(cand.numel(), 1)
        rec = {"fine_precision": hf.precision, "margin": m_f, "screen_error_max": float((sig - exact).abs().max()),
               "candidate_share": cand.numel() / (R * NT), "kernels_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
               "p_ms": mean["p_screen"], "s_ms": mean["s_dense_sigma"], "list_ns_per_sample": rate * 1e6,
               "l_ms": rate * R * NT, "C_star": (mean["s_dense_sigma"] - mean["p_screen"]) / (rate * R * NT)}
        shares = []
        for pose in range(poses):
            frame(pose)
            shares.append((~(sigma_f <= -m_f)).float().mean())
        if shares:
            col = torch.stack(shares).cpu().numpy()
            rec["candidate_share_poses"] = {"poses": poses, "min": float(col.min()), "max": float(col.max()), "mean": float(col.mean()),
                                            "spread": float(col.max() - col.min())}
        out[precision] = rec
        print("%-14s p = %.3f ms  s = %.3f ms  list %.3f ns/sample (l = %.3f ms)  C* = %.4f  share pose 5 %.4f  orbit %s" % (
            precision, rec["p_ms"], rec["s_ms"], rec["list_ns_per_sample"], rec["l_ms"], rec["C_star"], rec["candidate_share"],
            rec.get("candidate_share_poses")), flush=True)
        del ws, wsf, coarse, fine
        torch.cuda.empty_cache()
    return out


def frames():
    o, d = utils.gen_rays(H, W, synth.fern_intrinsics(H, W), synth.spiral_pose(5))
    R = o.shape[0]
    gen = torch.Generator(device="cuda").manual_seed(1)
    zs_all = torch.randn(max(KS), 32, device="cuda", generator=gen)
    result = {"frame_hw": [H, W], "pose": 5, "rays": R, "n_coarse": NC, "n_fine": NF, "rounds": ROUNDS,
              "renders_per_measurement": RENDERS, "device": torch.cuda.get_device_name(0), "min_weight": 0.0,
              "A": "render_latents(zs [K,32], min_weight=0[, style_precision='fp16mx'])",
              "B": "the same with geometry='chain'; B_off / B_on / B_auto: screen=False / True / None", "pairs": {}}
    for precision, kw in PAIRS.items():
        coarse, fine, style = make(precision)
        a = rendering.RayRenderer(coarse, fine, style)
        bs = {name: rendering.RayRenderer(coarse, fine, style, screen=s) for name, s in SCREENS.items()}
        rec_pair = {"frame": {}, "build_geometry": {}}
        for K in KS:
            z = zs_all[:K].contiguous()
            run = {"A": lambda: a.render_latents(o, d, NC, NF, zs=z, min_weight=0., **kw)}
            for name, r in bs.items():
                run[name] = (lambda r: lambda: r.render_latents(o, d, NC, NF, zs=z, min_weight=0., geometry="chain", **kw))(r)
            imgs = {}
            for _ in range(2):                             # the warm-up: it lands the shares AUTO reads
                for name, fn in run.items():
                    imgs[name] = fn()
                    torch.cuda.synchronize()
            rec = interleaved(run)
            for name in SCREENS:
                rec[name + "_over_A"] = rec[name]["ms_mean"] / rec["A"]["ms_mean"]
                rec["every_%s_below_every_A_by_more_than_A_spread" % name] = below(rec, name, "A")
            rec["B_bits_equal_across_screens"] = all(torch.equal(imgs["B_off"][k], imgs[n][k]) for n in ("B_on", "B_auto") for k in ("rgb", "t"))
            diff = (imgs["A"]["rgb"] - imgs["B_on"]["rgb"]).abs().amax(dim=(0, 2))
            rec["rays_A_vs_B_above_1e-3"] = float((diff > 1e-3).float().mean())
            rec["candidate_shares"] = [coarse.packed().screen_fraction(), fine.packed().screen_fraction()]
            rec_pair["frame"][str(K)] = rec
            print(line("%-14s frame K=%d  " % (precision, K), rec) + "   on/A %.3f auto/A %.3f  wins (off, on, auto): %s %s %s  bits %s  rays > 1e-3: %.2f %%"
                  % (rec["B_on_over_A"], rec["B_auto_over_A"], rec["every_B_off_below_every_A_by_more_than_A_spread"],
                     rec["every_B_on_below_every_A_by_more_than_A_spread"], rec["every_B_auto_below_every_A_by_more_than_A_spread"],
                     rec["B_bits_equal_across_screens"], 100 * rec["rays_A_vs_B_above_1e-3"]), flush=True)
            del imgs
        run = {"A": lambda: a.build_geometry(o, d, NC, NF, min_weight=0.)}
        for name, r in bs.items():
            run[name] = (lambda r: lambda: r.build_geometry(o, d, NC, NF, min_weight=0., geometry="chain"))(r)
        for fn in run.values():
            fn()
        rec = interleaved(run)
        for name in SCREENS:
            rec["every_%s_below_every_A_by_more_than_A_spread" % name] = below(rec, name, "A")
        rec_pair["build_geometry"] = rec
        print(line("%-14s build_geometry  " % precision, rec), flush=True)
        # every sample a candidate: a screen can only lose, AUTO has to stay dense
        a._ws_multi = None
        for r in bs.values():
            r._ws_multi = None
        del a, bs, coarse, fine
        torch.cuda.empty_cache()
        coarse, fine, style = make(precision, shift=1000.0)
        off = rendering.RayRenderer(coarse, fine, style, screen=False)
        auto = rendering.RayRenderer(coarse, fine, style, screen=None)
        z = zs_all[:1].contiguous()
        run = {"B_off": lambda: off.render_latents(o, d, NC, NF, zs=z, min_weight=0., geometry="chain", **kw),
               "B_auto": lambda: auto.render_latents(o, d, NC, NF, zs=z, min_weight=0., geometry="chain", **kw)}
        for _ in range(2):
            for fn in run.values():
                fn()
                torch.cuda.synchronize()
        before = (coarse.packed().screened_renders(), fine.packed().screened_renders())
        rec = interleaved(run)
        rec["screened_passes_under_auto"] = [coarse.packed().screened_renders() - before[0], fine.packed().screened_renders() - before[1]]
        rec["auto_within_off_span"] = min(rec["B_off"]["ms"]) <= rec["B_auto"]["ms_mean"] <= max(rec["B_off"]["ms"])
        rec_pair["all_candidates_K1"] = rec
        print(line("%-14s all candidates K=1  " % precision, rec) + "   screened passes under AUTO %s" % rec["screened_passes_under_auto"], flush=True)
        result["pairs"][precision] = rec_pair
        off._ws_multi = auto._ws_multi = None
        del off, auto, coarse, fine
        torch.cuda.empty_cache()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step0", action="store_true")
    ap.add_argument("--poses", type=int, default=120, help="--step0: candidate shares over spiral poses 0 .. poses-1")
    ap.add_argument("--rounds", type=int, default=5, help="--step0: timed rounds of every launch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "screen_geometry_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_screen_geometry: no GPU visible; there is nothing to time without one")
    record = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            record = json.load(f)
    if args.step0:
        record["step0"] = step0(args.poses, args.rounds)
    else:
        record["frames"] = frames()
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
