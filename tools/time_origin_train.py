#!/usr/bin/env python3
"""Timing of the Origin_train loop (`train_tgtcs --origin_train`, train_loop.origin_train) against the bare iteration it
wraps, on the synthetic teacher scene (20 frames of 100 x 100, 200 000 rays), 64 + 64 samples, batches of 1 024 and 2 048.

    A = training.origin_train_step on ONE resident batch, draws from the global generator, losses left on the device:
        the iteration as it was timed before the loop existed (3.1 ms at 1 024 rays)
    B = the loop in steady state: a shuffled batch through tgtc_train_batch, draws from the per-step seeded generator,
        the iteration, the running loss sum, the learning-rate decay; the host waits only at the `i_print` lines
        (every 100 steps), whose own steps/s are what is reported

A and B alternate, ROUNDS times, so the spread of A against itself is known.  The pieces B adds are timed on their own
(the batch: permutation slice + tgtc_train_batch; the seeded draws), and tgtc_train_batch alone against the same batch
assembled the reference's way on the device -- float64 ray tables of every frame from utils.gen_rays, built once, and three
row gathers per batch.

Prints and writes profiles/origin_train_loop_timing.json (or the path given).  Needs a GPU: there is no fallback."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tgtc_style_amd import config as cfg, models, synth, train_data, train_loop, training, utils  # noqa: E402

HW = 100
BATCHES = (1024, 2048)
ROUNDS = 3
STEPS_A, WARM_A = 200, 20
I_PRINT, LOOP_STEPS = 100, 400          # lines at 0, 100, ..., 400: the first window is warm-up


def t_state(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def students(args, fused=True):
    m, mf = models.StyleNerf(args, mode="coarse"), models.StyleNerf(args, mode="fine")
    m.load_state_dict(t_state(synth.nerf_state(10))), mf.load_state_dict(t_state(synth.nerf_state(11)))
    return m.cuda().trainable(fused=fused), mf.cuda().trainable(fused=fused)


def wall_ms(fn, steps, warm):
    for i in range(warm + steps):
        if i == warm:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def device_us(fn, steps=500, warm=20):
    for _ in range(warm):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(steps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps * 1e3


def bare_step(args, data, batch):
    m, mf = students(args)
    opt = train_loop.make_optimizer(args, m, mf)
    o, d, gt = data.batch(train_data.EpochSampler(data.rays_num, batch, 0).batch_indices(0))
    return wall_ms(lambda: training.origin_train_step(m, mf, opt, o, d, gt, args.N_samples, args.N_samples_fine, data.near,
                                                      data.far, sigma_noise_std=args.sigma_noise_std, as_float=False),
                   STEPS_A, WARM_A)


def loop(args, data, batch):
    a = cfg.parse_args(["--config", os.path.join(ROOT, "configs", "fern.txt"), "--batch_size", str(batch), "--origin_step",
                        str(LOOP_STEPS), "--i_print", str(I_PRINT), "--train_seed", "0"])
    m, mf = students(a)
    log = []
    with tempfile.TemporaryDirectory() as sv:
        train_loop.origin_train(a, m, mf, data, sv, 0, log=log)
    steady = [e for e in log if e["window"] == I_PRINT][1:]
    assert len(steady) == LOOP_STEPS // I_PRINT - 1 and all(e["overflows"] == 0 for e in log)
    return [1e3 / e["steps_per_s"] for e in steady], log[-1]["mean_loss"]


def pieces(args, data, batch):
    sampler = train_data.EpochSampler(data.rays_num, batch, 0)
    step = [0]

    def gather():
        data.batch(sampler.batch_indices(step[0]))
        step[0] += 1

    gen = torch.Generator(device="cuda")
    n, nf = args.N_samples, args.N_samples + args.N_samples_fine

    def draws(seeded):
        g = None
        if seeded:
            gen.manual_seed(train_loop.step_seed(0, step[0]))
            g = gen
        step[0] += 1
        torch.rand(batch, n, device="cuda", generator=g)
        torch.randn(batch, n, device="cuda", generator=g) * args.sigma_noise_std
        torch.randn(batch, nf, device="cuda", generator=g) * args.sigma_noise_std

    index = sampler.batch_indices(1)
    kernel_us = device_us(lambda: data.batch(index))
    # the reference's tables on the device: rays of every pixel of every frame, built once, gathered per batch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rays = [utils.gen_rays(data.h, data.w, data.f, data.cps[f], pixel_alignment=data.pixel_alignment) for f in range(data.frame_num)]
    tab_o, tab_d = torch.cat([o for o, _ in rays]), torch.cat([d for _, d in rays])
    tab_c = data.images.reshape(-1, 3)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    o, d, c = data.batch(index)
    assert torch.equal(tab_o[index], o) and torch.equal(tab_d[index], d) and torch.equal(tab_c[index], c)
    tables_us = device_us(lambda: (tab_o[index], tab_d[index], tab_c[index]))
    return {"batch_ms_wall": wall_ms(gather, 500, 20), "seeded_draws_ms_wall": wall_ms(lambda: draws(True), 500, 20),
            "global_draws_ms_wall": wall_ms(lambda: draws(False), 500, 20),
            "tgtc_train_batch_us": kernel_us, "ray_tables_three_gathers_us": tables_us, "ray_tables_build_ms": build_ms,
            "ray_tables_bytes": int(tab_o.numel() * 8 * 2), "train_batch_tables_bytes": int(data.c2w.numel() * 4)}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_origin_train: no GPU visible; there is nothing to time without one")
    args = cfg.parse_args(["--config", os.path.join(ROOT, "configs", "fern.txt"), "--synthetic", "--synthetic_hw", str(HW)])
    data = train_data.TrainRays.from_synthetic(args, torch.device("cuda", 0))
    result = {"device": torch.cuda.get_device_name(0), "scene": "synthetic teacher, %d frames of %d x %d" % (data.frame_num, HW, HW),
              "rays": data.rays_num, "n_coarse": args.N_samples, "n_fine": args.N_samples_fine,
              "sigma_noise_std": args.sigma_noise_std, "rounds": ROUNDS, "steps_per_A": STEPS_A, "i_print": I_PRINT, "per_batch": {}}
    for batch in BATCHES:
        a_ms, b_ms = [], []
        for _ in range(ROUNDS):
            a_ms.append(bare_step(args, data, batch))
            windows, final = loop(args, data, batch)
            b_ms.append(sum(windows) / len(windows))
        a, b = sum(a_ms) / ROUNDS, sum(b_ms) / ROUNDS
        rec = {"A_bare_step_ms": a_ms, "B_loop_ms_per_step": b_ms, "A_ms_mean": a, "B_ms_mean": b, "overhead_ms": b - a,
               "overhead_over_step": (b - a) / a, "A_spread_rel": (max(a_ms) - min(a_ms)) / a,
               "B_spread_rel": (max(b_ms) - min(b_ms)) / b, "steps_per_s": 1e3 / b, "mean_loss_of_the_last_window": final}
        rec.update(pieces(args, data, batch))
        result["per_batch"][str(batch)] = rec
        print("batch %d: A (bare step) %.3f ms [%s]   B (loop) %.3f ms [%s]   overhead %.3f ms = %.1f %% of the step   batch %.3f ms, "
              "seeded draws %.3f ms (global %.3f) wall; tgtc_train_batch %.1f us vs three gathers of the ray tables %.1f us"
              % (batch, a, " ".join("%.3f" % x for x in a_ms), b, " ".join("%.3f" % x for x in b_ms), b - a, 100 * (b - a) / a,
                 rec["batch_ms_wall"], rec["seeded_draws_ms_wall"], rec["global_draws_ms_wall"], rec["tgtc_train_batch_us"],
                 rec["ray_tables_three_gathers_us"]), flush=True)
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "origin_train_loop_timing.json")
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
