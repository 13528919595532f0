#!/usr/bin/env python3
"""What the float64 sum of d sigma_layer.bias (sigma_bias_kernel, csrc/mlp_train.hip) costs the fused trainer: the product
library against a development build that leaves the launch out, on ONE box, alternated ROUNDS times.  A library is per
process, so every measurement is a child process of this one (TGTC_LIB selects the build); the parent opens no GPU.

    (a) tgtc_trainer_backward alone, dense, M = 131 072 (1 024 rays x 128 samples of the fine network), device events
    (b) training.origin_train_step on one resident batch of the synthetic teacher scene, 1 024 rays, 64 + 64 samples,
        students with the teacher's weights, dense backward, wall clock with one synchronisation at the end

The development build is the product's objects with mlp_train.hip compiled under -DTGTC_ABL_NOSIGMABIAS, in csrc/:

    hipcc <the Makefile's CXXFLAGS> -DTGTC_ABL_NOSIGMABIAS -c mlp_train.hip -o /tmp/mlp_train_nosb.o
    hipcc -shared -fPIC --offload-arch=gfx950 -o libtgtc_dev_nosb.so <every product object but mlp_train.o> /tmp/mlp_train_nosb.o

Prints and writes profiles/sigma_bias_timing.json (or the path given).  Needs a GPU: there is no fallback."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tgtc-style_amd", "csrc")
BUILDS = {"without": os.path.join(CSRC, "libtgtc_dev_nosb.so"), "with": os.path.join(CSRC, "libtgtc_hip.so")}
ROUNDS = 3
M = 131072
BACKWARDS, WARM_BACKWARDS = 200, 20
RAYS, STEPS, WARM_STEPS = 1024, 200, 20
HW = 100


def child():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from tgtc_style_amd import config as cfg, fused_train, models, synth, train_data, train_loop, training
    from time_sparse_backward import device_ms, t_state, wall_ms
    if not torch.cuda.is_available():
        raise SystemExit("time_sigma_bias: no GPU visible; there is nothing to time without one")
    args = cfg.parse_args(["--config", os.path.join(ROOT, "configs", "fern.txt"), "--synthetic", "--synthetic_hw", str(HW)])
    rng = np.random.default_rng(0)
    pts = torch.from_numpy(rng.uniform(-1.2, 1.2, (M, 3))).cuda()
    dirs = torch.from_numpy(rng.uniform(-1, 1, (M, 3))).cuda()
    d_rgb = torch.from_numpy(rng.standard_normal((M, 3)).astype(np.float32) * 1e-3).cuda()
    d_sig = torch.from_numpy(rng.standard_normal(M).astype(np.float32) * 1e-5).cuda()
    net = models.StyleNerf(args, mode="fine")
    net.load_state_dict(t_state(synth.nerf_state(1)))
    params = [p.detach().float().contiguous() for p in fused_train.mlp_parameters(net.cuda().net)]
    tr = fused_train.NerfTrainer()
    ws = tr.lease(M, pts.device)
    rgb, _ = tr.forward(params, pts, dirs, ws)
    backward = device_ms(lambda: tr.backward(params, rgb, d_rgb, d_sig, ws), BACKWARDS, WARM_BACKWARDS)
    assert tr.overflows() == 0
    data = train_data.TrainRays.from_synthetic(args, torch.device("cuda", 0))
    o, d, gt = data.batch(train_data.EpochSampler(data.rays_num, RAYS, 0).batch_indices(0))
    torch.manual_seed(0)
    m, mf = models.StyleNerf(args, mode="coarse"), models.StyleNerf(args, mode="fine")
    m.load_state_dict(t_state(synth.nerf_state(0))), mf.load_state_dict(t_state(synth.nerf_state(1)))
    m, mf = m.cuda().trainable(), mf.cuda().trainable()
    opt = train_loop.make_optimizer(args, m, mf)
    step = wall_ms(lambda: training.origin_train_step(m, mf, opt, o, d, gt, args.N_samples, args.N_samples_fine, data.near, data.far,
                                                      sigma_noise_std=args.sigma_noise_std, as_float=False), STEPS, WARM_STEPS)
    assert m.training_overflows() + mf.training_overflows() == 0
    print("RESULT " + json.dumps({"backward_ms": backward, "origin_train_step_ms": step}), flush=True)


def main():
    for name, path in BUILDS.items():
        if not os.path.exists(path):
            raise SystemExit("time_sigma_bias: %s (the build %s the launch) is not built; see the top of this file" % (path, name))
    runs = {name: [] for name in BUILDS}
    for _ in range(ROUNDS):
        for name, path in BUILDS.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, TGTC_LIB=path),
                                 check=True, capture_output=True, text=True, timeout=280).stdout
            rec = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
            runs[name].append(rec)
            print("%-7s backward alone %.4f ms   origin_train_step %.4f ms" % (name, rec["backward_ms"], rec["origin_train_step_ms"]), flush=True)
    result = {"rounds": ROUNDS, "backward_alone": {"M": M, "backwards_per_round": BACKWARDS, "clock": "device events", "mode": "dense"},
              "origin_train_step": {"rays": RAYS, "steps_per_round": STEPS, "clock": "wall, one synchronisation at the end",
                                    "scene": "synthetic teacher, %d x %d, students with the teacher's weights" % (HW, HW)}}
    for key, field in (("backward_alone", "backward_ms"), ("origin_train_step", "origin_train_step_ms")):
        for name in BUILDS:
            xs = [r[field] for r in runs[name]]
            result[key][name + "_ms"] = {"mean": sum(xs) / len(xs), "min": min(xs), "max": max(xs), "rounds": xs}
        a, b = result[key]["without_ms"], result[key]["with_ms"]
        result[key]["with_minus_without_ms"] = b["mean"] - a["mean"]
        result[key]["ranges_overlap"] = not (b["min"] > a["max"] or b["max"] < a["min"])
        print("%s: without %.4f ms [%.4f..%.4f]   with %.4f ms [%.4f..%.4f]   difference %+.4f ms, the ranges %s"
              % (key, a["mean"], a["min"], a["max"], b["mean"], b["min"], b["max"], result[key]["with_minus_without_ms"],
                 "overlap" if result[key]["ranges_overlap"] else "do not overlap"), flush=True)
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sigma_bias_timing.json")
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
