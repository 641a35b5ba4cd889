"""Rectified stereo matcher (pislam_match_stereo_batch) against brute force on the same pairs; prints one JSON line.

Setup per layout: each pair is a synthetic level-0 frame (synth.make_level0) and its copy shifted left by --disp px
(right(x) = left(x + d)).  VGA pyramids are built on the GPU by PyramidBuilder; the packed 1280x960 layout is built on
the host from the two level-0 frames with the synth helpers (synth.packed_level_table, bilinear resample).  Left and
right pyramids go through one OrbFrontend call as 2P pyramids.  scale_q16 = frontend.level_scales_q16(levels),
row_radius0[l] = round(2 s_l / 65536), level span 1, SAD radius 5, search radius 5, max_hamming 74, min_disp 0 and
max_disp 64 or 448.  Timing: after a warm-up, the median device-event time of single calls; brute force is
matchHammingBatch on the same descriptors and counts.  mean_candidates_per_query and the accept rates come from the
library's outputs and this tool's own host count on a sample of pairs.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats` (tracing slows the host; keep it out of these numbers)."""
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
    # name: (w0, h0, pairs, shapes per frame (None = synth default), max_keypoints)
    "vga": (640, 480, 256, None, 2048),
    "1280x960": (1280, 960, 128, 148, 4096),
}
BANDS = (64, 448)


def _mapped(pos, levels, scale_q16):
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
    return lid, X, Y


def candidates_per_query(lkp, rkp, levels, scale_q16, rr, span, max_disp):
    if len(lkp) == 0:
        return 0.0
    ll, Xl, Yl = _mapped(lkp, levels, scale_q16)
    lr, Xr, Yr = _mapped(rkp, levels, scale_q16)
    dx = Xl[:, None] - Xr[None, :]
    m = ((ll[:, None] >= 0) & (lr[None, :] >= 0) & (np.abs(ll[:, None] - lr[None, :]) <= span)
         & (np.abs(Yl[:, None] - Yr[None, :]) <= np.asarray(rr, np.int64)[np.maximum(lr, 0)][None, :])
         & (dx >= 0) & (dx <= max_disp))
    return float(m.sum(1).mean())


def run_layout(name, args, torch, ctx, stream):
    from pislam_amd import synth
    from pislam_amd.frontend import (OrbFrontend, PyramidBuilder, level_scales_q16, matchHammingBatch,
                                     matchStereoBatch, reserveMatchStereo)
    w0, h0, P, nshapes, max_kp = LAYOUTS[name]
    P = args.pairs or P
    d = args.disp
    dev = torch.device("cuda:0")
    l0 = synth.make_many(range(args.seed, args.seed + P), workers=min(16, os.cpu_count() or 1), kind="level0",
                         w0=w0, h0=h0, nshapes=nshapes)
    frames = np.concatenate([l0, np.roll(l0, -d, axis=2)])
    with torch.cuda.stream(stream):
        if name == "vga":
            pb = PyramidBuilder(w0, h0, ctx=ctx)
            levels, vstep, rows = pb.levels, pb.vstep, pb.rows
            pyr = torch.zeros((2 * P, rows, vstep), dtype=torch.uint8, device=dev)
            pb(torch.from_numpy(frames).to(dev), pyr)
        else:
            levels = synth.packed_level_table(w0, h0)
            vstep, rows = w0, synth.pyramid_rows(levels)
            host = np.zeros((2 * P, rows, vstep), np.uint8)
            for k in range(2 * P):
                for (w, h, r0, c0) in levels:
                    host[k, r0:r0 + h, c0:c0 + w] = frames[k] if (w, h) == (w0, h0) else synth._resize_bilinear(frames[k], w, h)
            pyr = torch.from_numpy(host).to(dev)
        fe = OrbFrontend(levels, vstep=vstep, rows=rows, max_keypoints=max_kp, ctx=ctx)
        kp, desc, counts = fe.alloc_outputs(2 * P, dev)
        fe(pyr, kp, desc, counts)
        lk, ld, lc = kp[:P].contiguous(), desc[:P].contiguous(), counts[:P].contiguous()
        rk, rd, rc = kp[P:].contiguous(), desc[P:].contiguous(), counts[P:].contiguous()
        lp, rp = pyr[:P], pyr[P:]
        scale = level_scales_q16(levels)
        rr = [int(np.floor(2 * s / 65536 + 0.5)) for s in scale]
        words = desc.shape[2]
        base = dict(level_span=1, max_hamming=74, sad_radius=5, search_radius=5, min_disp=0)
        out = [torch.empty((P, max_kp), dtype=torch.int32, device=dev) for _ in range(4)]
        ns = torch.empty((P,), dtype=torch.int32, device=dev)
        calls, stats = {}, {}
        for mx in BANDS:
            reserveMatchStereo(levels, scale, rr, max_kp, P, words=words, max_disp=mx, ctx=ctx, **base)
            calls[f"stereo_max{mx}"] = (lambda mx=mx: matchStereoBatch(
                lk, ld, lc, rk, rd, rc, lp, rp, levels, scale, rr, max_disp=mx, idx=out[0], dist=out[1],
                disp_q8=out[2], sad=out[3], nstereo=ns, ctx=ctx, **base))
        bf = [torch.empty((P, max_kp), dtype=torch.int32, device=dev) for _ in range(3)]
        calls["brute_force"] = lambda: matchHammingBatch(ld, lc, rd, rc, *bf, ctx=ctx)
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
        n = np.minimum(lc.cpu().numpy().view(np.uint32), max_kp).astype(np.int64)
        hl, hr = lk.cpu().numpy().view(np.uint32), rk.cpu().numpy().view(np.uint32)
        nr = np.minimum(rc.cpu().numpy().view(np.uint32), max_kp).astype(np.int64)
        sample = range(0, P, max(1, P // args.sample))
        for mx in BANDS:
            res = {}
            for mf in (False, True):
                matchStereoBatch(lk, ld, lc, rk, rd, rc, lp, rp, levels, scale, rr, max_disp=mx, median_filter=mf,
                                 idx=out[0], dist=out[1], disp_q8=out[2], sad=out[3], nstereo=ns, ctx=ctx, **base)
                stream.synchronize()
                res[mf] = int(ns.cpu().numpy().sum())
            stats[f"stereo_max{mx}"] = {
                "mean_candidates_per_query": round(float(np.mean(
                    [candidates_per_query(hl[k, :n[k]], hr[k, :nr[k]], levels, scale, rr, 1, mx) for k in sample])), 2),
                "accept_rate_before_filter": round(res[False] / max(1, int(n.sum())), 4),
                "accept_rate_after_filter": round(res[True] / max(1, int(n.sum())), 4),
            }
    return {
        "ms": {k: round(v, 4) for k, v in ms.items()}, "stats": stats,
        "mean_left_per_pair": round(float(n.mean()), 1), "scale_q16": scale, "row_radius0": rr,
        "levels": [list(map(int, t)) for t in levels], "pairs": P, "max_keypoints": max_kp, "disp": d,
        "candidate_sample_pairs": len(sample),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--layouts", default="vga,1280x960", help="comma-separated: " + ", ".join(LAYOUTS))
    ap.add_argument("--pairs", type=int, default=0, help="pairs per layout (0: 256 VGA, 128 at 1280x960)")
    ap.add_argument("--disp", type=int, default=16, help="shift of the right copy (px)")
    ap.add_argument("--iters", type=int, default=200, help="timed calls per matcher")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sample", type=int, default=8, help="pairs of the host candidate count")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_stereo needs a GPU (there is no CPU fallback)")
    from pislam_amd.capi import Context
    stream = torch.cuda.Stream(torch.device("cuda:0"))
    ctx = Context(device=0, stream=stream.cuda_stream)
    res = {name: run_layout(name, args, torch, ctx, stream) for name in args.layouts.split(",")}
    print(json.dumps({"tool": "bench_stereo", "iters": args.iters, "results": res}))


if __name__ == "__main__":
    main()
