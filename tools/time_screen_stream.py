#!/usr/bin/env python3
"""Development timing of the density screen's kernel alone ("The screen"): the four-tile persistent stream
(csrc/mlp_nerf_fp16s.hip) beside the CfgFast sigma-only launch it replaces (TGTC_SCREEN_CFGFAST=1, read by the library at every
call) and beside the same stream with the HIP front end in front of every pass (TGTC_SCREEN_SERIAL_FRONT=1, read likewise:
the yardstick of the front end under the stream), on the rays of one 400x400 frame at 128 depths (coarse net) and at 192 depths (fine net), HIP events on the launch stream,
the three launches interleaved inside every round.

    python tools/time_screen_stream.py [--rounds 5] [--out FILE]

THE GATE of the stream: it is the screen's default only if it beats the CfgFast launch at both depth counts by more than the
rounds' own spread.  THE GATE of the in-stream front end: every round of the default launch below every round of the serial-front
launch at both depth counts.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from tgtc_style_amd import hip, synth, utils

H = W = 400
SWITCH = "TGTC_SCREEN_CFGFAST"
SERIAL = "TGTC_SCREEN_SERIAL_FRONT"
ARMS = {"stream": None, "serial": SERIAL, "cfgfast": SWITCH}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()

    lib = hip.load()
    nets = bench.build_nets("fp16x3+fp16mx")
    handles = [m.packed() for m in nets]
    for h in handles:
        h.enable_screen()
    R = H * W
    o, d = utils.gen_rays(H, W, synth.fern_intrinsics(H, W), synth.spiral_pose(0))
    o, d = o.contiguous(), d.contiguous()
    st = hip.stream()
    result = {"shape": "%d rays, coarse net at 128 depths and fine net at 192 depths" % R, "rounds": args.rounds, "launches": {}}
    for h, n in zip(handles, (128, 192)):
        ts = torch.linspace(0, 1, n, device="cuda").repeat(R, 1).contiguous()
        out = {k: torch.empty(R * n, device="cuda") for k in ARMS}

        def launch(kind):
            for sw in (SWITCH, SERIAL):
                os.environ.pop(sw, None)
            if ARMS[kind]:
                os.environ[ARMS[kind]] = "1"
            hip.check(lib.tgtc_nerf_screen_rays(h.handle, hip.ptr(o), hip.ptr(d), hip.ptr(ts), R, n, hip.ptr(out[kind]), st))

        for _ in range(3):                 # untimed: the first launches after a pause run at ramping clocks
            for kind in out:
                launch(kind)
        torch.cuda.synchronize()
        same = bool(torch.equal(out["stream"], out["cfgfast"]) and torch.equal(out["stream"], out["serial"]))
        # one leading round more than asked, timed like the rest and dropped: the first pair of events of a process takes
        # up to 2 ms of set-up into whichever launch comes first
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.rounds + 1)] for k in out}
        for i in range(args.rounds + 1):
            for k in out:
                ev[k][i][0].record()
                launch(k)
                ev[k][i][1].record()
        torch.cuda.synchronize()
        for sw in (SWITCH, SERIAL):
            os.environ.pop(sw, None)
        ms = {k: [a.elapsed_time(b) for a, b in ev[k][1:]] for k in out}
        spread = max(max(v) - min(v) for v in ms.values())
        gain = float(np.mean(ms["cfgfast"]) - np.mean(ms["stream"]))
        result["launches"]["%d_depths" % n] = {
            "samples": R * n, "bits_equal": same, "stream_ms": [round(v, 4) for v in ms["stream"]], "serial_front_ms": [round(v, 4) for v in ms["serial"]],
            "cfgfast_ms": [round(v, 4) for v in ms["cfgfast"]],
            "stream_mean_ms": float(np.mean(ms["stream"])), "serial_front_mean_ms": float(np.mean(ms["serial"])),
            "cfgfast_mean_ms": float(np.mean(ms["cfgfast"])), "gain_ms": gain,
            "front_gain_ms": float(np.mean(ms["serial"]) - np.mean(ms["stream"])),
            "largest_spread_ms": float(spread), "passes_gate": bool(max(ms["stream"]) < min(ms["cfgfast"]) and gain > spread),
            "front_passes_gate": bool(max(ms["stream"]) < min(ms["serial"]))}
        print("%3d depths: stream %.3f ms (min %.3f max %.3f)  serial front %.3f ms (min %.3f max %.3f)  CfgFast %.3f ms (min %.3f max %.3f)  "
              "gain %.3f ms, of the front end %.3f ms  spread %.3f ms  bits equal: %s" % (
                  n, np.mean(ms["stream"]), min(ms["stream"]), max(ms["stream"]), np.mean(ms["serial"]), min(ms["serial"]), max(ms["serial"]),
                  np.mean(ms["cfgfast"]), min(ms["cfgfast"]), max(ms["cfgfast"]), gain, np.mean(ms["serial"]) - np.mean(ms["stream"]), spread, same), flush=True)
    result["gate"] = all(v["passes_gate"] for v in result["launches"].values())
    result["front_gate"] = all(v["front_passes_gate"] for v in result["launches"].values())
    print("gate:", "PASS" if result["gate"] else "FAIL", " front-end gate:", "PASS" if result["front_gate"] else "FAIL")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
