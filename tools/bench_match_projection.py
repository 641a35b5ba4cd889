"""Map-point search by projection against the scaled window matcher on the same counts, and against a device copy of
its inputs; prints one JSON line.

Setup: 256 synthetic VGA pyramids (synth.make_batch) through OrbFrontend give the train side (about 1000 keypoints a
frame).  Each frame gets `--points` map points (default 2048, the query stride): one per keypoint in turn, placed at a
random depth on the ray through the keypoint's level-0 position plus a jitter of a few pixels, with the keypoint's
descriptor and a distance range that predicts its level or the next, a normal along the viewing ray plus noise; the pose
is a small motion away from the one the points were made with.  th = 3 and the local-map defaults of
frontend.matchProjectionBatch (levels pl - 1 .. pl, cos_min 0.5, cos_near 0.998, the same-level rule).
Reported next to it:
  scaled        matchHammingScaledWindowBatch on the same counts, with qpred = this call's pred, level span 1 and
                radius0 = radius_far; the query keypoint is the corner of level pl (a dead query lies in no level).
  copy          torch copies of every input array into buffers of the same size (what touching the inputs once costs).
Timing: after a warm-up the three are timed in turn, `--iters` rounds, one device-event pair per call; the median and the
10th / 90th percentile of each are printed.  Kernel times come from a separate run under `rocprofv3 --kernel-trace
--stats` (tracing slows the host; keep it out of these numbers)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FX, FY, CX, CY = 500.0, 500.0, 320.0, 240.0


def make_points(rng, kp, counts, levels, scale_q16, level_scale, npts):
    """Map points of every frame from its own keypoints (host arrays): xw, drange, normal float32 and the index of the
    keypoint each point was made from."""
    B = kp.shape[0]
    xw = np.zeros((B, npts, 3), np.float32)
    drange = np.zeros((B, npts, 2), np.float32)
    normal = np.zeros((B, npts, 3), np.float32)
    src = np.zeros((B, npts), np.int64)
    ls = np.asarray(level_scale, np.float64)
    nl = len(levels)
    for b in range(B):
        n = max(1, min(int(counts[b]), kp.shape[1]))
        j = np.arange(npts) % n
        k = kp[b, j].astype(np.int64)
        x, y = (k >> 12) & 0xFFF, k & 0xFFF
        lid = np.zeros(npts, np.int64)
        X, Y = np.zeros(npts), np.zeros(npts)
        for l, t in enumerate(levels):
            c0 = t[3] if len(t) > 3 else 0
            m = (x >= c0) & (x < c0 + t[0]) & (y >= t[2]) & (y < t[2] + t[1])
            lid[m] = l
            X[m] = ((x[m] - c0) * scale_q16[l] + 32768) >> 16
            Y[m] = ((y[m] - t[2]) * scale_q16[l] + 32768) >> 16
        u, v = X + rng.integers(-4, 5, npts), Y + rng.integers(-4, 5, npts)
        z = rng.uniform(2, 20, npts)
        Xc = np.stack([(u - CX) / FX * z, (v - CY) / FY * z, z], 1)
        d = np.linalg.norm(Xc, axis=1)
        pl = np.clip(lid + rng.integers(0, 2, npts), 1, nl - 1)   # (level 0 is predicted only at d == dmax)
        dmax = d * np.where(pl == nl - 1, 1.1 * ls[nl - 1], np.sqrt(ls[pl - 1] * ls[pl]))
        nrm = Xc / d[:, None] + rng.normal(0, 0.05, (npts, 3))
        xw[b], drange[b] = Xc, np.stack([0.2 * dmax, dmax], 1)
        normal[b] = nrm / np.linalg.norm(nrm, axis=1)[:, None]
        src[b] = j
    return xw, drange, normal, src


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--points", type=int, default=2048, help="map points per frame (the query stride)")
    ap.add_argument("--th", type=float, default=3.0)
    ap.add_argument("--iters", type=int, default=200, help="timed rounds (every call once per round)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_match_projection needs a GPU (there is no CPU fallback)")
    from pislam_amd import synth
    from pislam_amd.capi import Context
    from pislam_amd.frontend import (OrbFrontend, level_scales_q16, matchHammingScaledWindowBatch, matchProjectionBatch,
                                     projectionRadii, reserveMatchProjection, reserveMatchScaledWindow)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx = Context(device=0, stream=stream.cuda_stream)
    rng = np.random.default_rng(args.seed)
    levels = synth.level_table(640, 480)
    rows = synth.pyramid_rows(levels)
    B, Q, max_kp = args.frames, args.points, 2048
    scale = level_scales_q16(levels)
    level_scale = (np.asarray(scale, np.float32) / np.float32(65536.0)).astype(np.float32)
    far, near = projectionRadii(scale, args.th)
    pyr = synth.make_batch(args.seed, B, w0=640, h0=480, vstep=640, levels=levels)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with torch.cuda.stream(stream):
        fe = OrbFrontend(levels, vstep=640, rows=rows, max_keypoints=max_kp, ctx=ctx)
        tk, td, tc = fe.alloc_outputs(B, dev)
        fe(torch.from_numpy(pyr).to(dev), tk, td, tc)
        stream.synchronize()
        words = int(td.shape[2])
        hk, hc = tk.cpu().numpy().view(np.uint32), tc.cpu().numpy().view(np.uint32)
        hd = td.cpu().numpy()
        xw_h, dr_h, nr_h, src = make_points(rng, hk, np.where(hc == 0xFFFFFFFF, 0, hc), levels, scale, level_scale, Q)
        qd = T(np.stack([hd[b][src[b]] for b in range(B)]))
        xw, drange, normal = T(xw_h), T(dr_h), T(nr_h)
        qc = torch.full((B,), Q, dtype=torch.int32, device=dev)
        # a small motion away from the identity the points were made with: 0.3 degrees about y, 0.02 along x
        a = np.deg2rad(0.3)
        pose = np.array([np.cos(a), 0, np.sin(a), 0, 1, 0, -np.sin(a), 0, np.cos(a), 0.02, 0, 0], np.float32)
        pose = T(np.tile(pose, (B, 1)))
        cam = T(np.tile(np.array([FX, FY, CX, CY, 40.0], np.float32), (B, 1)))
        reserveMatchProjection(levels, max_kp, B, scale_q16=scale, radius_far=far.tolist(), radius_near=near.tolist(),
                               words=words, ctx=ctx)
        reserveMatchScaledWindow(levels, scale, far.tolist(), 1, max_kp, B, words=words, ctx=ctx)
        out = [torch.empty((B, Q), dtype=torch.int32, device=dev) for _ in range(3)]
        pred = torch.empty((B, Q, 2), dtype=torch.int32, device=dev)
        plevel = torch.empty((B, Q), dtype=torch.uint8, device=dev)

        def projection():
            matchProjectionBatch(pose, cam, xw, qd, qc, tk, td, tc, levels, drange=drange, normal=normal, scale_q16=scale,
                                 level_scale=level_scale, radius_far=far.tolist(), radius_near=near.tolist(), idx=out[0],
                                 dist=out[1], dist2=out[2], pred=pred, plevel=plevel, ctx=ctx)

        projection()
        stream.synchronize()
        pl = plevel.cpu().numpy().astype(np.int64)
        live = pl != 0xFF
        matched = out[0].cpu().numpy() >= 0
        # the scaled call's query keypoints: the corner of level pl, or a position in no level for a dead query
        corner = np.array([((t[3] if len(t) > 3 else 0) << 12) | t[2] for t in levels], np.int64)
        qk = T(np.where(live, corner[np.minimum(pl, len(levels) - 1)], (4095 << 12) | 4095).astype(np.int32))
        out2 = [torch.empty((B, Q), dtype=torch.int32, device=dev) for _ in range(3)]

        def scaled():
            matchHammingScaledWindowBatch(qk, qd, qc, tk, td, tc, levels, scale, far.tolist(), 1, pred, *out2, ctx=ctx)

        ins = [pose, cam, xw, qd, qc, drange, normal, tk, td, tc]
        dup = [torch.empty_like(t) for t in ins]

        def copy():
            for s, d in zip(ins, dup):
                d.copy_(s, non_blocking=True)

        calls = {"projection": projection, "scaled": scaled, "copy": copy}
        for _ in range(args.warmup):
            for fn in calls.values():
                fn()
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
              for k in calls}
        for i in range(args.iters):
            for k, fn in calls.items():
                a, b = ev[k][i]
                a.record(stream)
                fn()
                b.record(stream)
        stream.synchronize()
    ms = {}
    for k in calls:
        t = np.array([a.elapsed_time(b) for a, b in ev[k]])
        ms[k] = {"median": round(float(np.median(t)), 4), "p10": round(float(np.percentile(t, 10)), 4),
                 "p90": round(float(np.percentile(t, 90)), 4)}
    n = np.minimum(np.where(hc == 0xFFFFFFFF, 0, hc), max_kp).astype(np.int64)
    print(json.dumps({
        "tool": "bench_match_projection", "frames": B, "points_per_frame": Q, "th": args.th, "iters": args.iters,
        "words": words, "mean_train_per_frame": round(float(n.mean()), 1), "live_share": round(float(live.mean()), 4),
        "matched_share": round(float(matched.mean()), 4), "ms": ms,
        "projection_over_scaled": round(ms["projection"]["median"] / ms["scaled"]["median"], 3),
        "input_bytes": int(sum(t.numel() * t.element_size() for t in ins)),
        "radius_far": far.tolist(), "radius_near": near.tolist(), "scale_q16": scale}))


if __name__ == "__main__":
    main()
