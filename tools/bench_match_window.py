"""Windowed matcher against the brute-force matcher on the same front-end pairs; prints one JSON line.

Setup per layout: 257 synthetic pyramids (synth.make_batch) through OrbFrontend; pyramid k's keypoints and
descriptors are matched against pyramid k + 1's as 256 pairs, with radius round(15 / 1.2^l) on level l.
Timing: after a warm-up, the median device-event time of single calls (windowed: index + match; brute force:
matchHammingBatch on the same descriptors and counts).  mean_candidates_per_query comes from this tool's own host
count of the window on a sample of pairs (queries outside every level count as 0).  Kernel times come from a
separate run under `rocprofv3 --kernel-trace --stats` (tracing slows the host; keep it out of these numbers)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LAYOUTS = {
    # name: (w0, h0, vstep, packed levels, shapes per frame (None = synth default), max_keypoints)
    "vga": (640, 480, 640, False, None, 2048),
    "1280x960": (1280, 960, 1280, True, 148, 4096),
}


def candidates_per_query(qkp, tkp, levels, radius):
    """Mean window candidates per query of one pair (host count, the semantics of include/pislam_hip.h)."""
    def lid(pos):
        pos = pos.astype(np.int64)
        x, y = (pos >> 12) & 0xFFF, pos & 0xFFF
        l = np.full(len(pos), -1, np.int64)
        for k, t in enumerate(levels):
            c0 = t[3] if len(t) > 3 else 0
            l[(x >= c0) & (x < c0 + t[0]) & (y >= t[2]) & (y < t[2] + t[1])] = k
        return l, x, y
    lq, xq, yq = lid(qkp)
    lt, xt, yt = lid(tkp)
    r = np.asarray(radius, np.int64)[np.maximum(lq, 0)][:, None]
    m = ((lq[:, None] >= 0) & (lq[:, None] == lt[None, :]) & (np.abs(xq[:, None] - xt[None, :]) <= r)
         & (np.abs(yq[:, None] - yt[None, :]) <= r))
    return float(m.sum(1).mean()) if len(qkp) else 0.0


def run_layout(name, args, torch, ctx, stream):
    from pislam_amd import synth
    from pislam_amd.frontend import OrbFrontend, matchHammingBatch, matchHammingWindowBatch, reserveMatchWindow
    w0, h0, vstep, packed, nshapes, max_kp = LAYOUTS[name]
    levels = synth.packed_level_table(w0, h0) if packed else synth.level_table(w0, h0)
    rows = synth.pyramid_rows(levels)
    P = args.pairs
    pyr = synth.make_batch(args.seed, P + 1, w0=w0, h0=h0, vstep=vstep, levels=levels, nshapes=nshapes)
    dev = torch.device("cuda:0")
    radius = [int(round(args.radius / 1.2 ** l)) for l in range(len(levels))]
    with torch.cuda.stream(stream):
        fe = OrbFrontend(levels, vstep=vstep, rows=rows, max_keypoints=max_kp, ctx=ctx)
        kp, desc, counts = fe.alloc_outputs(P + 1, dev)
        fe(torch.from_numpy(pyr).to(dev), kp, desc, counts)
        qk, qd, qc = kp[:P].contiguous(), desc[:P].contiguous(), counts[:P].contiguous()
        tk, td, tc = kp[1:].contiguous(), desc[1:].contiguous(), counts[1:].contiguous()
        reserveMatchWindow(levels, radius, max_kp, P, words=desc.shape[2], ctx=ctx)
        win_out = [torch.empty((P, max_kp), dtype=torch.int32, device=dev) for _ in range(3)]
        bf_out = [torch.empty((P, max_kp), dtype=torch.int32, device=dev) for _ in range(3)]
        calls = {
            "window": lambda: matchHammingWindowBatch(qk, qd, qc, tk, td, tc, levels, radius, *win_out, ctx=ctx),
            "brute_force": lambda: matchHammingBatch(qd, qc, td, tc, *bf_out, ctx=ctx),
        }
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
    hk, hc = kp.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32)
    n = np.minimum(hc, max_kp).astype(np.int64)
    sample = range(0, P, max(1, P // args.sample))
    cand = [candidates_per_query(hk[k, :n[k]], hk[k + 1, :n[k + 1]], levels, radius) for k in sample]
    return {
        "window_ms": round(ms["window"], 4), "brute_force_ms": round(ms["brute_force"], 4),
        "speedup": round(ms["brute_force"] / ms["window"], 3),
        "mean_candidates_per_query": round(float(np.mean(cand)), 2),
        "mean_train_per_pair": round(float(n[1:].mean()), 1), "mean_queries_per_pair": round(float(n[:P].mean()), 1),
        "radius": radius, "levels": [list(map(int, t)) for t in levels], "pairs": P, "max_keypoints": max_kp,
        "candidate_sample_pairs": len(cand),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--layouts", default="vga,1280x960", help="comma-separated: " + ", ".join(LAYOUTS))
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--radius", type=int, default=15, help="level-0 window radius; level l uses round(r / 1.2^l)")
    ap.add_argument("--iters", type=int, default=200, help="timed calls per matcher")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sample", type=int, default=16, help="pairs of the host candidate count")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_match_window needs a GPU (there is no CPU fallback)")
    from pislam_amd.capi import Context
    stream = torch.cuda.Stream(torch.device("cuda:0"))
    ctx = Context(device=0, stream=stream.cuda_stream)
    res = {name: run_layout(name, args, torch, ctx, stream) for name in args.layouts.split(",")}
    print(json.dumps({"tool": "bench_match_window", "iters": args.iters, "radius0": args.radius, "results": res}))


if __name__ == "__main__":
    main()
