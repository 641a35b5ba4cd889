"""Scale-aware guided window matcher against the windowed and brute-force matchers on the same front-end pairs;
prints one JSON line.

Setup per layout: 257 synthetic pyramids (synth.make_batch) through OrbFrontend; pyramid k's keypoints and
descriptors are matched against pyramid k + 1's as 256 pairs.  The scaled matcher uses scale_q16 =
frontend.level_scales_q16(levels) and radius0[l] = round(15 * s_l / 65536) (15 level pixels, in level-0 pixels) at
level span 0, 1 and 2, with no prediction; the windowed matcher uses radius round(15 / 1.2^l) as
tools/bench_match_window.py does.  Timing: after a warm-up, the median device-event time of single calls (index +
match for both window matchers; brute force: matchHammingBatch on the same descriptors and counts).
mean_candidates_per_query comes from this tool's own host count on a sample of pairs (queries outside every level count
as 0).  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (tracing slows the host; keep
it out of these numbers)."""
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
SPANS = (0, 1, 2)


def _positions(pos, levels, scale_q16):
    """(level id or -1, x, y, X, Y): stacked and mapped level-0 coordinates (include/pislam_hip.h)."""
    pos = pos.astype(np.int64)
    x, y = (pos >> 12) & 0xFFF, pos & 0xFFF
    lid = np.full(len(pos), -1, np.int64)
    X, Y = np.zeros_like(x), np.zeros_like(y)
    for k, t in enumerate(levels):
        c0 = t[3] if len(t) > 3 else 0
        m = (x >= c0) & (x < c0 + t[0]) & (y >= t[2]) & (y < t[2] + t[1])
        lid[m] = k
        X[m] = ((x[m] - c0) * scale_q16[k] + 32768) >> 16
        Y[m] = ((y[m] - t[2]) * scale_q16[k] + 32768) >> 16
    return lid, x, y, X, Y


def candidates_per_query(qkp, tkp, levels, scale_q16, radius0, spans, radius):
    """Mean candidates per query of one pair: {span: scaled matcher, "window": windowed matcher}."""
    if len(qkp) == 0:
        return {**{s: 0.0 for s in spans}, "window": 0.0}
    lq, xq, yq, Xq, Yq = _positions(qkp, levels, scale_q16)
    lt, xt, yt, Xt, Yt = _positions(tkp, levels, scale_q16)
    both = (lq[:, None] >= 0) & (lt[None, :] >= 0)
    r0 = np.asarray(radius0, np.int64)[np.maximum(lq, 0)][:, None]
    near = both & (np.abs(Xq[:, None] - Xt[None, :]) <= r0) & (np.abs(Yq[:, None] - Yt[None, :]) <= r0)
    dl = np.abs(lq[:, None] - lt[None, :])
    out = {s: float((near & (dl <= s)).sum(1).mean()) for s in spans}
    r = np.asarray(radius, np.int64)[np.maximum(lq, 0)][:, None]
    win = both & (dl == 0) & (np.abs(xq[:, None] - xt[None, :]) <= r) & (np.abs(yq[:, None] - yt[None, :]) <= r)
    out["window"] = float(win.sum(1).mean())
    return out


def run_layout(name, args, torch, ctx, stream):
    from pislam_amd import synth
    from pislam_amd.frontend import (OrbFrontend, level_scales_q16, matchHammingBatch, matchHammingScaledWindowBatch,
                                     matchHammingWindowBatch, reserveMatchScaledWindow, reserveMatchWindow)
    w0, h0, vstep, packed, nshapes, max_kp = LAYOUTS[name]
    levels = synth.packed_level_table(w0, h0) if packed else synth.level_table(w0, h0)
    rows = synth.pyramid_rows(levels)
    P = args.pairs
    pyr = synth.make_batch(args.seed, P + 1, w0=w0, h0=h0, vstep=vstep, levels=levels, nshapes=nshapes)
    dev = torch.device("cuda:0")
    scale = level_scales_q16(levels)
    radius0 = [int(np.floor(args.radius * s / 65536 + 0.5)) for s in scale]
    radius = [int(round(args.radius / 1.2 ** l)) for l in range(len(levels))]
    with torch.cuda.stream(stream):
        fe = OrbFrontend(levels, vstep=vstep, rows=rows, max_keypoints=max_kp, ctx=ctx)
        kp, desc, counts = fe.alloc_outputs(P + 1, dev)
        fe(torch.from_numpy(pyr).to(dev), kp, desc, counts)
        qk, qd, qc = kp[:P].contiguous(), desc[:P].contiguous(), counts[:P].contiguous()
        tk, td, tc = kp[1:].contiguous(), desc[1:].contiguous(), counts[1:].contiguous()
        words = desc.shape[2]
        for span in SPANS:
            reserveMatchScaledWindow(levels, scale, radius0, span, max_kp, P, words=words, ctx=ctx)
        reserveMatchWindow(levels, radius, max_kp, P, words=words, ctx=ctx)
        out = [torch.empty((P, max_kp), dtype=torch.int32, device=dev) for _ in range(3)]
        calls = {f"scaled_span{s}": (lambda s=s: matchHammingScaledWindowBatch(qk, qd, qc, tk, td, tc, levels, scale,
                                                                               radius0, s, None, *out, ctx=ctx))
                 for s in SPANS}
        calls["window"] = lambda: matchHammingWindowBatch(qk, qd, qc, tk, td, tc, levels, radius, *out, ctx=ctx)
        calls["brute_force"] = lambda: matchHammingBatch(qd, qc, td, tc, *out, ctx=ctx)
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
    cand = [candidates_per_query(hk[k, :n[k]], hk[k + 1, :n[k + 1]], levels, scale, radius0, SPANS, radius) for k in sample]
    mean_cand = {f"scaled_span{s}": round(float(np.mean([c[s] for c in cand])), 2) for s in SPANS}
    mean_cand["window"] = round(float(np.mean([c["window"] for c in cand])), 2)
    return {
        "ms": {k: round(v, 4) for k, v in ms.items()},
        "mean_candidates_per_query": mean_cand,
        "mean_train_per_pair": round(float(n[1:].mean()), 1), "mean_queries_per_pair": round(float(n[:P].mean()), 1),
        "scale_q16": scale, "radius0": radius0, "window_radius": radius, "levels": [list(map(int, t)) for t in levels],
        "pairs": P, "max_keypoints": max_kp, "candidate_sample_pairs": len(cand),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--layouts", default="vga,1280x960", help="comma-separated: " + ", ".join(LAYOUTS))
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--radius", type=int, default=15,
                    help="window radius in level pixels: radius0[l] = round(r * s_l / 65536); windowed: round(r / 1.2^l)")
    ap.add_argument("--iters", type=int, default=200, help="timed calls per matcher")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sample", type=int, default=16, help="pairs of the host candidate count")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_match_scaled needs a GPU (there is no CPU fallback)")
    from pislam_amd.capi import Context
    stream = torch.cuda.Stream(torch.device("cuda:0"))
    ctx = Context(device=0, stream=stream.cuda_stream)
    res = {name: run_layout(name, args, torch, ctx, stream) for name in args.layouts.split(",")}
    print(json.dumps({"tool": "bench_match_scaled", "iters": args.iters, "radius": args.radius, "results": res}))


if __name__ == "__main__":
    main()
