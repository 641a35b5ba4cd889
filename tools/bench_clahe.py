"""Batched CLAHE (pislam_clahe_batch) in front of the pyramid build; prints one JSON line.

Workloads: `frames` synthetic 640 x 480 frames (synth.make_level0, eight distinct ones repeated) at 8 x 8 tiles and
clip_q8 768 (ORB-SLAM3's setting); the same with constant frames (every lane of the table kernel hits one histogram
bin: the worst case for its LDS atomics); and a quarter as many 1280 x 960 frames.  Timed per workload, each as the
median device-event time of single calls after a warm-up: the table kernel (pislam_clahe_luts_batch), the apply kernel
(pislam_clahe_apply_batch) and the whole call, each with the kernels' alternatives ("clahe_combine" 0: one LDS atomic
per pixel; "clahe_lut_global" 1: tables read from global memory per pixel), and, in the same run as yardsticks, a
device-to-device copy of the same frames and pislam_pyramid_build_batch with one blurred level on them.  bytes = the
frames read twice and written once plus the tables written once and read once; gb_s is what they imply for the whole
call.  x_copy is the whole call's time over the copy's."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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
    ap.add_argument("--frames", type=int, default=256, help="VGA frames per batch (1280 x 960: a quarter as many)")
    ap.add_argument("--iters", type=int, default=200, help="timed calls per configuration")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_clahe needs a GPU (there is no CPU fallback)")
    from pislam_amd import synth
    from pislam_amd.capi import Context
    from pislam_amd.frontend import Clahe, PyramidBuilder
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx = Context(device=0, stream=stream.cuda_stream)
    res = {}
    workloads = (("vga", 640, 480, args.frames, False), ("vga_constant", 640, 480, args.frames, True),
                 ("1280x960", 1280, 960, max(1, args.frames // 4), False))
    with torch.cuda.stream(stream):
        for name, W, H, B, constant in workloads:
            if constant:
                frames = torch.full((B, H, W), 117, dtype=torch.uint8, device=dev)
            else:
                distinct = np.stack([synth.make_level0(args.seed + i, W, H) for i in range(min(8, B))])
                frames = torch.from_numpy(distinct).to(dev).repeat((B + len(distinct) - 1) // len(distinct), 1, 1)[:B].contiguous()
            clahe = Clahe(W, H, tiles=(8, 8), clip_q8=768, ctx=ctx)
            out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
            luts = torch.empty((B, 8, 8, 256), dtype=torch.uint8, device=dev)
            nbytes = 3 * B * W * H + 2 * B * clahe.lut_size
            r = {"frames": B, "width": W, "height": H, "bytes": nbytes}
            got = {}
            for tag, combine, lut_global in (("", 1, 0), ("_alt", 0, 1)):
                ctx.set_option("clahe_combine", combine)
                ctx.set_option("clahe_lut_global", lut_global)
                r["luts_ms" + tag] = round(timed(lambda: clahe.luts(frames, luts), stream, torch, args.warmup, args.iters), 4)
                r["apply_ms" + tag] = round(timed(lambda: clahe.apply(frames, luts, out), stream, torch, args.warmup, args.iters), 4)
                r["call_ms" + tag] = round(timed(lambda: clahe(frames, out, luts), stream, torch, args.warmup, args.iters), 4)
                got[tag] = (out.clone(), luts.clone())
            ctx.set_option("clahe_combine", 1)
            ctx.set_option("clahe_lut_global", 0)
            r["variants_equal"] = bool(torch.equal(got[""][0], got["_alt"][0]) and torch.equal(got[""][1], got["_alt"][1]))
            r["copy_ms"] = round(timed(lambda: out.copy_(frames), stream, torch, args.warmup, args.iters), 4)
            pb = PyramidBuilder(W, H, (), blur=True, ctx=ctx)
            pyr = torch.zeros((B, pb.rows, pb.vstep), dtype=torch.uint8, device=dev)
            pb(frames, pyr)
            r["build_one_level_blur_ms"] = round(timed(lambda: pb(frames, pyr, margins_clean=True), stream, torch, args.warmup, args.iters), 4)
            r["gb_s"] = round(nbytes / r["call_ms"] / 1e6, 1)
            r["copy_gb_s"] = round(2 * B * W * H / r["copy_ms"] / 1e6, 1)
            r["x_copy"] = round(r["call_ms"] / r["copy_ms"], 2)
            res[name] = r
    print(json.dumps({"tool": "bench_clahe", "iters": args.iters, "results": res}))


if __name__ == "__main__":
    main()
