#!/usr/bin/env python3
"""Timing of the sparse backward of the fused trainer (include/tgtc_train.h "Sparse backward") against the dense
one -- the same process, the two modes alternated ROUNDS times, mean and min..max of the rounds.

    (a) tgtc_trainer_backward alone at M = 131 072 (1 024 rays x 128 samples of the fine network): the upstream gradients
        of a random share L of the samples kept, the rest zeroed, L in SHARES; dense on the same inputs.  The break-even
        share is where the two lines cross (linear between the measured shares).
    (b) training.origin_train_step on ONE resident batch of the synthetic teacher scene, 1 024 and 2 048 rays, 64 + 64
        samples, sigma_noise_std 1, in two states: freshly initialised students (torch's default nn.Linear initialisation)
        and students that carry the teacher's weights (synth.nerf_state(0) / (1)).

Every sparse figure comes with the live share its counters saw (tgtc_trainer_live_counts).  Prints and writes
profiles/sparse_backward_timing.json (or the path given).  Needs a GPU: there is no fallback."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tgtc_style_amd import config as cfg, fused_train, models, synth, train_data, train_loop, training  # noqa: E402

M = 131072
SHARES = (1.0, 0.5, 0.25, 0.1, 0.03)
ROUNDS = 3
BACKWARDS, WARM_BACKWARDS = 20, 3
BATCHES = (1024, 2048)
STEPS, WARM_STEPS = 100, 10
HW = 100


def t_state(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def stats(xs):
    return {"mean": sum(xs) / len(xs), "min": min(xs), "max": max(xs), "rounds": xs}


def device_ms(fn, n, warm):
    for _ in range(warm):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(n):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / n


def wall_ms(fn, steps, warm):
    for i in range(warm + steps):
        if i == warm:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def backward_alone(args):
    rng = np.random.default_rng(0)
    pts = torch.from_numpy(rng.uniform(-1.2, 1.2, (M, 3))).cuda()
    dirs = torch.from_numpy(rng.uniform(-1, 1, (M, 3))).cuda()
    g_rgb = torch.from_numpy(rng.standard_normal((M, 3)).astype(np.float32) * 1e-3).cuda()
    g_sig = torch.from_numpy(rng.standard_normal(M).astype(np.float32) * 1e-5).cuda()
    keep_order = torch.from_numpy(rng.permutation(M)).cuda()
    net = models.StyleNerf(args, mode="fine")
    net.load_state_dict(t_state(synth.nerf_state(1)))
    params = [p.detach().float().contiguous() for p in fused_train.mlp_parameters(net.cuda().net)]
    trainers = {False: fused_train.NerfTrainer(sparse=False), True: fused_train.NerfTrainer(sparse=True)}
    ws, rgb = {}, {}
    for sp, tr in trainers.items():
        ws[sp] = tr.lease(M, pts.device)
        rgb[sp], _ = tr.forward(params, pts, dirs, ws[sp])
    out = {}
    for share in SHARES:
        mask = torch.zeros(M, device="cuda")
        mask[keep_order[:int(round(share * M))]] = 1.0
        d_rgb, d_sig = (g_rgb * mask[:, None]).contiguous(), (g_sig * mask).contiguous()
        ms = {False: [], True: []}
        before = trainers[True].live_counts()
        for _ in range(ROUNDS):
            for sp in (False, True):
                ms[sp].append(device_ms(lambda: trainers[sp].backward(params, rgb[sp], d_rgb, d_sig, ws[sp]), BACKWARDS, WARM_BACKWARDS))
        after = trainers[True].live_counts()
        rec = {"dense_ms": stats(ms[False]), "sparse_ms": stats(ms[True]),
               "live_share_from_the_counters": (after[0] - before[0]) / (after[1] - before[1])}
        out["%g" % share] = rec
        print("backward alone, M %d, L %.2f (counters: %.4f): dense %.3f ms [%.3f..%.3f]   sparse %.3f ms [%.3f..%.3f]"
              % (M, share, rec["live_share_from_the_counters"], rec["dense_ms"]["mean"], rec["dense_ms"]["min"], rec["dense_ms"]["max"],
                 rec["sparse_ms"]["mean"], rec["sparse_ms"]["min"], rec["sparse_ms"]["max"]), flush=True)
    for tr in trainers.values():
        assert tr.overflows() == 0
    # break-even: linear between neighbouring shares, on the means
    pts_ = sorted((float(k), v["sparse_ms"]["mean"] - v["dense_ms"]["mean"]) for k, v in out.items())
    even = None
    for (l0, d0), (l1, d1) in zip(pts_, pts_[1:]):
        if d0 <= 0 < d1:
            even = l0 + (l1 - l0) * (0 - d0) / (d1 - d0)
    return out, even


def students(args, state, sparse):
    m, mf = models.StyleNerf(args, mode="coarse"), models.StyleNerf(args, mode="fine")
    if state == "teacher_weights":
        m.load_state_dict(t_state(synth.nerf_state(0))), mf.load_state_dict(t_state(synth.nerf_state(1)))
    return m.cuda().trainable(sparse=sparse), mf.cuda().trainable(sparse=sparse)


def iteration(args, data):
    out = {}
    for batch in BATCHES:
        o, d, gt = data.batch(train_data.EpochSampler(data.rays_num, batch, 0).batch_indices(0))
        for state in ("fresh", "teacher_weights"):
            ms, live = {False: [], True: []}, {"coarse": [], "fine": []}
            for _ in range(ROUNDS):
                for sp in (False, True):
                    torch.manual_seed(0)                       # the same fresh weights and the same draws in both modes
                    m, mf = students(args, state, sp)
                    opt = train_loop.make_optimizer(args, m, mf)
                    step = lambda: training.origin_train_step(m, mf, opt, o, d, gt, args.N_samples, args.N_samples_fine, data.near,
                                                              data.far, sigma_noise_std=args.sigma_noise_std, as_float=False)
                    ms[sp].append(wall_ms(step, STEPS, WARM_STEPS))
                    assert m.training_overflows() + mf.training_overflows() == 0
                    if sp:
                        for name, net in (("coarse", m), ("fine", mf)):
                            n = net.training_live_counts()
                            live[name].append(n[0] / n[1])
                    m.trainable(False), mf.trainable(False)
                    del m, mf, opt
                    torch.cuda.empty_cache()
            rec = {"dense_ms": stats(ms[False]), "sparse_ms": stats(ms[True]), "live_coarse": stats(live["coarse"]),
                   "live_fine": stats(live["fine"])}
            spread = max(rec["dense_ms"]["max"] - rec["dense_ms"]["min"], rec["sparse_ms"]["max"] - rec["sparse_ms"]["min"])
            rec["dense_minus_sparse_ms"] = rec["dense_ms"]["mean"] - rec["sparse_ms"]["mean"]
            rec["largest_spread_of_the_rounds_ms"] = spread
            rec["faster_by_more_than_the_spread"] = bool(rec["dense_minus_sparse_ms"] > spread)
            out["%d rays, %s" % (batch, state)] = rec
            print("origin_train_step, %d rays, %s: dense %.3f ms [%.3f..%.3f]   sparse %.3f ms [%.3f..%.3f]   live %.3f coarse %.3f fine"
                  % (batch, state, rec["dense_ms"]["mean"], rec["dense_ms"]["min"], rec["dense_ms"]["max"], rec["sparse_ms"]["mean"],
                     rec["sparse_ms"]["min"], rec["sparse_ms"]["max"], rec["live_coarse"]["mean"], rec["live_fine"]["mean"]), flush=True)
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_sparse_backward: no GPU visible; there is nothing to time without one")
    args = cfg.parse_args(["--config", os.path.join(ROOT, "configs", "fern.txt"), "--synthetic", "--synthetic_hw", str(HW)])
    result = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS,
              "backward_alone": {"M": M, "backwards_per_round": BACKWARDS, "clock": "device events"}}
    result["backward_alone"]["per_share"], result["backward_alone"]["break_even_share"] = backward_alone(args)
    print("break-even share: %s" % result["backward_alone"]["break_even_share"], flush=True)
    torch.cuda.empty_cache()
    data = train_data.TrainRays.from_synthetic(args, torch.device("cuda", 0))
    result["origin_train_step"] = {"scene": "synthetic teacher, %d frames of %d x %d" % (data.frame_num, HW, HW),
                                   "n_coarse": args.N_samples, "n_fine": args.N_samples_fine, "sigma_noise_std": args.sigma_noise_std,
                                   "steps_per_round": STEPS, "clock": "wall, one synchronisation at the end",
                                   "live shares": "sums over all steps of a round, warm-up included", "per_case": iteration(args, data)}
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_backward_timing.json")
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
