"""Batched lens undistortion (pislam_warp_batch) on VGA frames; prints one JSON line.

Setup: `frames` synthetic 640 x 480 frames (synth.make_level0, eight distinct ones repeated) through the warp of a
EuRoC-like camera: EuRoC cam0's focal lengths and distortion (k1 -0.2834, k2 0.0740, p1 1.9e-4, p2 1.8e-5) with the
principal point moved to where it lies in the central 640 columns of that 752 x 480 sensor.  Timed, each as the median
device-event time of single calls after a warm-up: the warp at log_cell 0 (a dense mesh) and 3, each with the tile
plan deciding (auto) and with option "warp_direct" (every tap from global memory), and, in the same run,
pislam_pyramid_build_batch with one level on the same frames, without the blur (a plain copy of the same bytes) and
with it (gaussian5x5) — the library's nearest kernels.  bytes = source + destination + mesh (both axes) per call; gb_s is what they imply.  The two
modes' outputs are compared.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats`."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EUROC_VGA_K = [[458.654, 0.0, 367.215 - 56.0], [0.0, 457.296, 248.375], [0.0, 0.0, 1.0]]
EUROC_DIST = [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05]


def timed(fn, stream, torch, warmup, iters):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record(stream)
        fn()
        b.record(stream)
    stream.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200, help="timed calls per configuration")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_warp needs a GPU (there is no CPU fallback)")
    from pislam_amd import synth
    from pislam_amd.capi import Context
    from pislam_amd.frontend import PyramidBuilder, Warp
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx = Context(device=0, stream=stream.cuda_stream)
    W, H, B = 640, 480, args.frames
    res = {}
    with torch.cuda.stream(stream):
        distinct = np.stack([synth.make_level0(args.seed + i, W, H) for i in range(min(8, B))])
        frames = torch.from_numpy(distinct).to(dev).repeat((B + len(distinct) - 1) // len(distinct), 1, 1)[:B].contiguous()
        out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        for lc in (0, 3):
            warp = Warp.from_calibration(EUROC_VGA_K, EUROC_DIST, (W, H), log_cell=lc, ctx=ctx)
            info = warp.info()
            mesh_bytes = 2 * 4 * (((W - 1) >> lc) + 2) * (((H - 1) >> lc) + 2)
            nbytes = 2 * B * W * H + mesh_bytes
            got = {}
            for mode, direct in (("auto", 0), ("direct", 1)):
                ctx.set_option("warp_direct", direct)
                ms = timed(lambda: warp(frames, out), stream, torch, args.warmup, args.iters)
                got[mode] = out.clone()
                res[f"log_cell{lc}_{mode}"] = {"ms": round(ms, 4), "bytes": nbytes, "gb_s": round(nbytes / ms / 1e6, 1)}
            ctx.set_option("warp_direct", 0)
            res[f"log_cell{lc}_tiles"] = info
            res[f"log_cell{lc}_modes_equal"] = bool(torch.equal(got["auto"], got["direct"]))
            warp.close()
        for key, blur in (("build_one_level", False), ("build_one_level_blur", True)):
            pb = PyramidBuilder(W, H, (), blur=blur, ctx=ctx)
            pyr = torch.zeros((B, pb.rows, pb.vstep), dtype=torch.uint8, device=dev)
            pb(frames, pyr)
            ms = timed(lambda: pb(frames, pyr, margins_clean=True), stream, torch, args.warmup, args.iters)
            res[key] = {"ms": round(ms, 4), "bytes": 2 * B * W * H, "gb_s": round(2 * B * W * H / ms / 1e6, 1)}
    res.update({"frames": B, "width": W, "height": H})
    print(json.dumps({"tool": "bench_warp", "iters": args.iters, "results": res}))


if __name__ == "__main__":
    main()
