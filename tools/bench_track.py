"""Pyramidal Lucas-Kanade tracker (pislam_track_lk_batch) on 256 VGA pairs, every keypoint a point; prints one JSON line.

Setup: each pair is a synthetic level-0 frame (synth.make_level0) and the same scene moved by --shift px
(next(x, y) = prev(x - dx, y - dy)); both pyramids are built on the GPU by PyramidBuilder and go through one
OrbFrontend call as 2P pyramids.  The points are all keypoints of the previous frame (keypointsToQ8), no guess.
Timed: trackLKBatch at max_coarse 0 and 2 (level_step 3) and win_radius 3 and 7, the other parameters at their
defaults, and as the yardstick matchStereoBatch on the same pairs (next as left, prev as right, max_disp 64, the
settings of tools/bench_stereo.py), re-measured in the same run.  Timing: after a warm-up, the median device-event time
of single calls.  The tracked share and the mean iteration count of the own level come from the status words.  Kernel
times come from a separate run under `rocprofv3 --kernel-trace --stats` (tracing slows the host; keep it out of
these numbers)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SETTINGS = [(w, mc) for mc in (0, 2) for w in (3, 7)]


def run(args, torch, ctx, stream):
    from pislam_amd import synth
    from pislam_amd.frontend import (OrbFrontend, PyramidBuilder, keypointsToQ8, level_scales_q16, matchStereoBatch,
                                     reserveMatchStereo, trackLKBatch)
    w0, h0, P, max_kp = 640, 480, args.pairs, 2048
    dx, dy = args.shift
    dev = torch.device("cuda:0")
    l0 = synth.make_many(range(args.seed, args.seed + P), workers=min(16, os.cpu_count() or 1), kind="level0", w0=w0, h0=h0)
    frames = np.concatenate([l0, np.roll(l0, (dy, dx), axis=(1, 2))])
    with torch.cuda.stream(stream):
        pb = PyramidBuilder(w0, h0, ctx=ctx)
        levels, vstep, rows = pb.levels, pb.vstep, pb.rows
        pyr = torch.zeros((2 * P, rows, vstep), dtype=torch.uint8, device=dev)
        pb(torch.from_numpy(frames).to(dev), pyr)
        fe = OrbFrontend(levels, vstep=vstep, rows=rows, max_keypoints=max_kp, ctx=ctx)
        kp, desc, counts = fe.alloc_outputs(2 * P, dev)
        fe(pyr, kp, desc, counts)
        pk, pd, pc = kp[:P].contiguous(), desc[:P].contiguous(), counts[:P].contiguous()
        nk, nd, nc = kp[P:].contiguous(), desc[P:].contiguous(), counts[P:].contiguous()
        prev, nxt = pyr[:P], pyr[P:]
        scale = level_scales_q16(levels)
        pts = keypointsToQ8(pk).contiguous()
        outs = [torch.empty(s, dtype=torch.int32, device=dev) for s in ((P, max_kp, 2), (P, max_kp), (P, max_kp), (P,))]
        calls = {}
        for w, mc in SETTINGS:
            calls[f"track_w{w}_coarse{mc}"] = (lambda w=w, mc=mc: trackLKBatch(
                prev, nxt, pts, pc, levels, scale, win_radius=w, max_coarse=mc, level_step=3, next_q8=outs[0],
                status=outs[1], err=outs[2], ntracked=outs[3], ctx=ctx))
        rr = [int(np.floor(2 * s / 65536 + 0.5)) for s in scale]
        base = dict(level_span=1, max_hamming=74, sad_radius=5, search_radius=5, min_disp=0, max_disp=64)
        reserveMatchStereo(levels, scale, rr, max_kp, P, words=desc.shape[2], ctx=ctx, **base)
        so = [torch.empty((P, max_kp), dtype=torch.int32, device=dev) for _ in range(4)]
        ns = torch.empty((P,), dtype=torch.int32, device=dev)
        calls["stereo_max64"] = lambda: matchStereoBatch(nk, nd, nc, pk, pd, pc, nxt, prev, levels, scale, rr, idx=so[0],
                                                         dist=so[1], disp_q8=so[2], sad=so[3], nstereo=ns, ctx=ctx, **base)
        ms = {}
        for key, fn in calls.items():
            for _ in range(args.warmup):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
            for a, b in ev:
                a.record(stream)
                fn()
                b.record(stream)
            stream.synchronize()
            ms[key] = float(np.median([a.elapsed_time(b) for a, b in ev]))
        n = np.minimum(pc.cpu().numpy().view(np.uint32), max_kp).astype(np.int64)
        live = np.arange(max_kp)[None, :] < n[:, None]
        stats = {}
        for w, mc in SETTINGS:
            key = f"track_w{w}_coarse{mc}"
            calls[key]()
            stream.synchronize()
            st = outs[1].cpu().numpy().view(np.uint32)[live]
            nq = outs[0].cpu().numpy()[live].astype(np.int64) - pts.cpu().numpy()[live]
            ok = (st & 255) == 0
            lvl = np.zeros(len(st), np.int64)
            y = (pk.cpu().numpy().view(np.uint32)[live] & 0xFFF).astype(np.int64)
            for l, t in enumerate(levels):
                lvl[(y >= t[2]) & (y < t[2] + t[1])] = l
            s = np.asarray(scale, np.float64)[lvl] / 65536
            e = np.maximum(np.abs(nq[:, 0] / 256 * s - dx), np.abs(nq[:, 1] / 256 * s - dy))      # level-0 pixels
            assert int(ok.sum()) == int(outs[3].cpu().numpy().sum())
            stats[key] = {
                "tracked_share": round(float(ok.mean()), 4),
                "codes_1_to_4": [int(((st & 255) == c).sum()) for c in (1, 2, 3, 4)],
                "mean_iterations_of_tracked": round(float((st[ok] >> 8).mean()), 2),
                "tracked_within_half_level0_px_of_the_shift": round(float((e[ok] <= 0.5).mean()), 4),
            }
    return {"ms": {k: round(v, 4) for k, v in ms.items()}, "stats": stats, "mean_points_per_pair": round(float(n.mean()), 1),
            "points": int(n.sum()), "pairs": P, "max_keypoints": max_kp, "shift": [dx, dy], "scale_q16": scale,
            "levels": [list(map(int, t)) for t in levels]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--shift", type=int, nargs=2, default=(3, 1), metavar=("DX", "DY"), help="motion of the next frame (px)")
    ap.add_argument("--iters", type=int, default=200, help="timed calls per setting")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_track needs a GPU (there is no CPU fallback)")
    from pislam_amd.capi import Context
    stream = torch.cuda.Stream(torch.device("cuda:0"))
    ctx = Context(device=0, stream=stream.cuda_stream)
    print(json.dumps({"tool": "bench_track", "iters": args.iters, "results": run(args, torch, ctx, stream)}))


if __name__ == "__main__":
    main()
