#!/usr/bin/env python3
"""Development timing of the HIP code in front of every pass of the persistent NeRF kernels ("front end"): the
three density launches of the headline frame, 400x400 rays at 128 + 64 samples, under several builds of the library in ONE
process, interleaved, HIP events on the launch stream.

    python tools/time_front_end.py --lib abl1=PATH [--lib abl4=PATH ...] [--rounds N] [--out FILE]
        x3s_coarse_density      tgtc_nerf_forward_rays, coarse fp16x3 handle, 128 depths, density only   (nerf_x3s_kernel)
        mx2_fine_density        tgtc_nerf_forward_rays, fine fp16mx handle, 192 depths, density only     (nerf_mx2_kernel)
        mx2_stash_producer      tgtc_nerf_stash_fill, the same pass + parking                           (nerf_mx2_stash_kernel)

"base" is the product library.  The others are development builds of mlp_nerf_x3s.hip, mlp_nerf_mx2.hip and
mlp_nerf_mx2_stash.hip with -DTGTC_FRONT_ABL=k -DTGTC_MX2_ABL=k linked against the product's other objects: k = 1 drops the
sample loads and the encoders, k = 4 keeps the loads and drops the encoders' arithmetic.  Their densities are WRONG by
construction; base - abl1 is what the front end costs a launch, the ceiling of anything that makes it cheaper.  (With wrong
densities the producer parks another share of its samples: its figure under an ablation is not comparable, the density-only
launch of the same stream is.)  A handle packed by the product library is passed to the other builds: same struct, same
device memory."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from time_plain_cull import H, NC, NF, NT, W, stats, timed
from tgtc_style_amd import hip, rendering, synth, utils


def bind(path):
    lib = ctypes.CDLL(path)
    for name in ("tgtc_nerf_forward_rays", "tgtc_nerf_stash_fill"):
        fn = getattr(lib, name)
        fn.argtypes = hip._SIGNATURES[name]
        fn.restype = ctypes.c_int
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], metavar="TAG=PATH")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()

    libs = {"base": hip.load()}
    for spec in args.lib:
        tag, path = spec.split("=", 1)
        libs[tag] = bind(path)
    coarse, fine = bench.build_nets("fp16x3+fp16mx")
    R = H * W
    r = rendering.RayRenderer(coarse, fine, fused=False, cull=False, screen=False)
    o, d = (x.contiguous() for x in utils.gen_rays(H, W, synth.fern_intrinsics(H, W), synth.spiral_pose(0)))
    r.render(o, d, NC, NF, near=0., far=1.)
    torch.cuda.synchronize()
    wsf = r._ws.view(torch.float32)
    ts_c = wsf[:R * NC].clone()
    ts_f = wsf[6 * R * NC:6 * R * NC + R * NT].clone()
    sigma = torch.empty(R * NT, device="cuda")
    scratch = torch.empty(2048, dtype=torch.int32, device="cuda")
    ovf = torch.empty(R * NT, dtype=torch.int32, device="cuda")
    stash = torch.empty(libs["base"].tgtc_net_stash_bytes(R, NT, rendering.RayRenderer.STASH_SHARE), dtype=torch.uint8, device="cuda")
    fine.packed().set_stash(stash)
    hc, hf = coarse.packed().handle, fine.packed().handle

    def check(rc):
        assert rc == 0, rc

    calls = {}
    for tag, lib in libs.items():
        calls["x3s_coarse_density/" + tag] = lambda lib=lib: check(lib.tgtc_nerf_forward_rays(
            hc, hip.ptr(o), hip.ptr(d), hip.ptr(ts_c), R, NC, None, hip.ptr(sigma), hip.stream()))
        calls["mx2_fine_density/" + tag] = lambda lib=lib: check(lib.tgtc_nerf_forward_rays(
            hf, hip.ptr(o), hip.ptr(d), hip.ptr(ts_f), R, NT, None, hip.ptr(sigma), hip.stream()))
        calls["mx2_stash_producer/" + tag] = lambda lib=lib: check(lib.tgtc_nerf_stash_fill(
            hf, hip.ptr(o), hip.ptr(d), hip.ptr(ts_f), R, NT, hip.ptr(sigma), hip.ptr(scratch), hip.ptr(ovf), hip.stream()))
    t = timed(calls, args.rounds)
    torch.cuda.synchronize()
    # a build that is not an ablation must give the product's densities, bit for bit
    same = {}
    for name in ("x3s_coarse_density", "mx2_fine_density", "mx2_stash_producer"):
        sigma.fill_(float("nan"))
        calls[name + "/base"]()
        ref = sigma.clone()
        for tag in libs:
            if tag != "base" and not tag.startswith("abl"):
                sigma.fill_(float("nan"))
                calls[name + "/" + tag]()
                same[name + "/" + tag] = bool(torch.equal(sigma.view(torch.int32), ref.view(torch.int32)))
    torch.cuda.synchronize()
    fine.packed().set_stash(None)
    result = {"shape": "%d rays, %d coarse / %d fine depths, planes of spiral pose 0" % (R, NC, NT), "rounds": args.rounds,
              "launches": {k: stats(v) for k, v in t.items()}, "same_bits_as_base": same}
    print("same bits as base:", same, flush=True)
    for k, v in t.items():
        print("%-34s %8.3f ms (min %.3f, max %.3f)" % (k, np.mean(v), np.min(v), np.max(v)), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
