#!/usr/bin/env python3
"""Timing of the Style_train loop (`train_tgtcs --style_train`, train_loop.style_train) against the iteration as it ran
before the loop existed, on the synthetic scene (20 frames of 100 x 100, one style, 200 000 rows), 64 + 64 samples,
batch_size_style 256 (fern's) and 1 024.

    A = training.style_train_step on ONE resident shuffled batch plus ONE resident frame-ordered batch: two passes over
        the operators, one Adam over the style MLPs and the latent table, draws from the global generator, losses left
        on the device
    B = the loop in steady state: both batches from one launch of tgtc_style_train_batch, ONE pass over R + B rows
        (training.style_train_iteration), two optimisers from one backward, draws from the per-step seeded generator, the
        running sums; the host waits only at the `i_print` lines, whose own steps/s are what is reported (the first
        window is warm-up and is dropped; no checkpoint is written inside a measured window)

A and B alternate in one process, ROUNDS times, and the spread of each is reported.  The batch call is timed on its own,
issued back to back (host enqueue included), next to tgtc_train_batch on the same rows.

Prints and writes profiles/style_train_loop_timing.json (or the path given).  Needs a GPU: there is no fallback.

    time_style_train_loop.py chain [path]

times a third variant against B instead, ROUNDS_CHAIN rounds each, alternated in one process:

    C = B with `--style_chain`: the two style MLPs of a pass through the library's style trainer
        (tgtc_style_trainer_forward / _backward, style_chain.StyleTrainer) instead of the per-layer path

and writes profiles/style_chain_timing.json (or the path given): milliseconds per step of both with min .. max over the
rounds, and whether the two ranges overlap."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tgtc_style_amd import config as cfg, models, synth, train_data, train_loop, training  # noqa: E402

HW = 100
BATCHES = (256, 1024)
ROUNDS = 3
ROUNDS_CHAIN = 5
STEPS_A, WARM_A = 40, 8
I_PRINT, LOOP_STEPS = 25, 75            # lines at 0, 25, 50, 75: the first window is warm-up
FERN = os.path.join(ROOT, "configs", "fern.txt")


def t_state(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def networks(args, data):
    m, mf = models.StyleNerf(args, mode="coarse"), models.StyleNerf(args, mode="fine")
    m.load_state_dict(t_state(synth.nerf_state(0))), mf.load_state_dict(t_state(synth.nerf_state(1)))
    cm, sm = models.StyleMLP_before_concat(args), models.StyleMLP_Wild_multilayers(args)
    cm.load_state_dict(t_state(synth.concat_state(2))), sm.load_state_dict(t_state(synth.style_state(3)))
    lat = models.StyleLatents_variational(style_num=data.style_num, frame_num=data.frame_num, latent_dim=args.vae_latent)
    lat.load_state_dict(t_state(synth.latents_state(4, style_num=data.style_num, frame_num=data.frame_num)))
    return m.cuda(), mf.cuda(), cm.cuda(), sm.cuda(), lat.cuda()


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


def two_pass_step(args, data, batch):
    m, mf, cm, sm, lat = networks(args, data)
    m.set_enable_style(True), mf.set_enable_style(True)
    cm.trainable(), sm.trainable(), lat.trainable()
    opt = torch.optim.Adam(list(sm.parameters()) + list(cm.parameters()) + [lat.latents], lr=args.lrate)
    b = data.batch(train_data.EpochSampler(data.data_num, batch, 0, full_batches=True).batch_indices(0), coh=(0, 1, 0, batch))
    R = batch
    coh_batch = {k: b[k][R:] for k in ("rays_o", "rays_d", "rgb_origin", "style_id", "frame_id")}
    coherence = training.CoherenceState(data.frame_num)
    return wall_ms(lambda: training.style_train_step(
        m, mf, cm, sm, lat, opt, b["rays_o"][:R], b["rays_d"][:R], b["rgb_gt"][:R], b["style_id"][:R], b["frame_id"][:R],
        args.N_samples, args.N_samples_fine, data.near, data.far, sigma_noise_std=args.sigma_noise_std,
        rgb_loss_lambda=args.rgb_loss_lambda, logp_loss_lambda=args.logp_loss_lambda, data_type=args.dataset_type,
        coherence=coherence, coh_batch=coh_batch, loss_coh_lambda=args.loss_coh_lambda, as_float=False), STEPS_A, WARM_A)


def loop(data, batch, chain=False):
    a = cfg.parse_args(["--config", FERN, "--batch_size_style", str(batch), "--total_step", str(LOOP_STEPS), "--i_print",
                        str(I_PRINT), "--i_weights", "1000000", "--train_seed", "0"] + (["--style_chain"] if chain else []))
    m, mf, cm, sm, lat = networks(a, data)
    log = []
    with tempfile.TemporaryDirectory() as sv:
        train_loop.style_train(a, m, mf, cm, sm, lat, data, sv, 0, log=log)
    steady = [e for e in log if e["window"] == I_PRINT][1:]
    assert len(steady) == LOOP_STEPS // I_PRINT - 1
    return [1e3 / e["steps_per_s"] for e in steady], log[-1]["mean_loss"]


def batch_call(data, batch):
    index = train_data.EpochSampler(data.data_num, batch, 0, full_batches=True).batch_indices(1)
    both = device_us(lambda: data.batch(index, coh=(0, 3, 128, batch)))
    shuffled_only = device_us(lambda: data.batch(index))
    origin = device_us(lambda: train_data.TrainRays.batch(data, index % data.rays_num))
    return {"tgtc_style_train_batch_us": both, "tgtc_style_train_batch_shuffled_rows_only_us": shuffled_only,
            "tgtc_train_batch_us": origin}


def chain_main(data, args, out_path):
    """B against C, ROUNDS_CHAIN rounds each, alternated; says whether the two ranges of round means overlap."""
    result = {"device": torch.cuda.get_device_name(0),
              "scene": "synthetic, %d style(s), %d frames of %d x %d" % (data.style_num, data.frame_num, HW, HW),
              "rows": data.data_num, "n_coarse": args.N_samples, "n_fine": args.N_samples_fine, "rounds": ROUNDS_CHAIN,
              "i_print": I_PRINT, "steady_windows_per_round": LOOP_STEPS // I_PRINT - 1,
              "B": "train_loop.style_train in steady state, the two style MLPs on the per-layer path (autograd_ops.py)",
              "C": "the same loop with --style_chain: both style MLPs through tgtc_style_trainer_forward / _backward",
              "per_batch": {}}
    for batch in BATCHES:
        b_ms, c_ms, finals = [], [], {}
        for _ in range(ROUNDS_CHAIN):
            for ms, chain in ((b_ms, False), (c_ms, True)):
                windows, finals["C" if chain else "B"] = loop(data, batch, chain)
                ms.append(sum(windows) / len(windows))
        b, c = sum(b_ms) / len(b_ms), sum(c_ms) / len(c_ms)
        apart = max(c_ms) < min(b_ms) or min(c_ms) > max(b_ms)
        rec = {"B_per_layer_ms_per_step": b_ms, "C_chain_ms_per_step": c_ms, "B_ms_mean": b, "C_ms_mean": c,
               "B_ms_min_max": [min(b_ms), max(b_ms)], "C_ms_min_max": [min(c_ms), max(c_ms)], "C_over_B": c / b,
               "difference_exceeds_the_rounds_spread": apart,
               "mean_loss_of_the_last_window": finals}
        result["per_batch"][str(batch)] = rec
        print("batch_size_style %d: B (per-layer) %.3f ms [%.3f .. %.3f]   C (chain) %.3f ms [%.3f .. %.3f]   C / B %.3f   "
              "the ranges %s" % (batch, b, min(b_ms), max(b_ms), c, min(c_ms), max(c_ms), c / b,
                                 "do not overlap" if apart else "OVERLAP: no difference beyond the rounds' spread"), flush=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_style_train_loop: no GPU visible; there is nothing to time without one")
    args = cfg.parse_args(["--config", FERN, "--synthetic", "--synthetic_hw", str(HW), "--synthetic_styles", "1"])
    data = train_data.StyleTrainRays.from_synthetic(args, torch.device("cuda", 0))
    if len(sys.argv) > 1 and sys.argv[1] == "chain":
        return chain_main(data, args, sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "style_chain_timing.json"))
    result = {"device": torch.cuda.get_device_name(0),
              "scene": "synthetic, %d style(s), %d frames of %d x %d" % (data.style_num, data.frame_num, HW, HW),
              "rows": data.data_num, "n_coarse": args.N_samples, "n_fine": args.N_samples_fine,
              "sigma_noise_std": args.sigma_noise_std, "rounds": ROUNDS, "steps_per_A": STEPS_A, "i_print": I_PRINT,
              "A": "training.style_train_step: resident shuffled batch + resident frame-ordered batch, two passes, one Adam",
              "B": "train_loop.style_train in steady state: one batch launch, one pass, two optimisers from one backward",
              "per_batch": {}}
    for batch in BATCHES:
        a_ms, b_ms = [], []
        for _ in range(ROUNDS):
            a_ms.append(two_pass_step(args, data, batch))
            windows, final = loop(data, batch)
            b_ms.append(sum(windows) / len(windows))
        a, b = sum(a_ms) / ROUNDS, sum(b_ms) / ROUNDS
        rec = {"A_two_pass_step_ms": a_ms, "B_loop_ms_per_step": b_ms, "A_ms_mean": a, "B_ms_mean": b, "B_over_A": b / a,
               "A_spread_rel": (max(a_ms) - min(a_ms)) / a, "B_spread_rel": (max(b_ms) - min(b_ms)) / b,
               "steps_per_s": 1e3 / b, "mean_loss_of_the_last_window": final}
        rec.update(batch_call(data, batch))
        result["per_batch"][str(batch)] = rec
        print("batch_size_style %d: A (two passes) %.3f ms [%s]   B (loop, one pass) %.3f ms [%s]   B / A %.3f   batch call %.1f us "
              "(shuffled rows only %.1f us; tgtc_train_batch %.1f us)"
              % (batch, a, " ".join("%.3f" % x for x in a_ms), b, " ".join("%.3f" % x for x in b_ms), b / a,
                 rec["tgtc_style_train_batch_us"], rec["tgtc_style_train_batch_shuffled_rows_only_us"], rec["tgtc_train_batch_us"]),
              flush=True)
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "style_train_loop_timing.json")
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
