"""Map-point fusion search (matchFuseBatch) against the projection matcher on the same inputs, and against a device
copy of its inputs; prints one JSON line.

Setup: bench_match_projection's (256 synthetic VGA pyramids through OrbFrontend, about 1000 keypoints a frame, `--points`
map points a frame made from the frame's own keypoints a few pixels off, a small motion away from the pose they were
made with).  The keypoints' observations are poseObservationsQ8's; half of them are stereo, with the disparity bf / z of
the first point made from the keypoint plus noise of a quarter pixel.  Timed in turn, in one run:
  fuse          matchFuseBatch with Fuse's defaults (th 3, radius th * scale, levels pl - 1 .. pl, chi2 5.99 / 7.8)
  projection    matchProjectionBatch on the same inputs with its local-map defaults (radii 4 th / 2.5 th * scale)
  copy          torch copies of every input array into buffers of the same size (what touching the inputs once costs).
Also reported: the share of queries fuse matches, and, counted on the host over the first `--stat-frames` frames with the
call's own pred / plevel, the share of fuse's window candidates that the reprojection test removes.
Timing: after a warm-up the three are timed in turn, `--iters` rounds, one device-event pair per call; the median and the
10th / 90th percentile of each are printed."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_match_projection import CX, CY, FX, FY, make_points  # noqa: E402

BF = 40.0


def removed_share(frames, pose, cam, xw, pred, plevel, kp, counts, obs, levels, scale_q16, radius, inv_sigma2, below, above,
                  chi2_mono, chi2_stereo):
    """(window candidates, those the reprojection test removes) over the given frames, in numpy float32 by the
    contract's formulas, from the call's own pred and plevel."""
    F = np.float32
    window = removed = 0
    for b in frames:
        n = int(counts[b])
        k = kp[b, :n].astype(np.int64)
        x, y = (k >> 12) & 0xFFF, k & 0xFFF
        lt = np.full(n, -1, np.int64)
        X, Y = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for l, t in enumerate(levels):
            c0 = t[3] if len(t) > 3 else 0
            m = (x >= c0) & (x < c0 + t[0]) & (y >= t[2]) & (y < t[2] + t[1])
            lt[m] = l
            X[m] = ((x[m] - c0) * scale_q16[l] + 32768) >> 16
            Y[m] = ((y[m] - t[2]) * scale_q16[l] + 32768) >> 16
        T, C, P = pose[b].astype(F), cam[b].astype(F), xw[b].astype(F)
        xc_ = ((T[0] * P[:, 0] + T[1] * P[:, 1]) + T[2] * P[:, 2]) + T[9]
        yc_ = ((T[3] * P[:, 0] + T[4] * P[:, 1]) + T[5] * P[:, 2]) + T[10]
        zc_ = ((T[6] * P[:, 0] + T[7] * P[:, 1]) + T[8] * P[:, 2]) + T[11]
        with np.errstate(all="ignore"):
            iz = F(1.0) / zc_
            pu, pv = C[0] * (xc_ * iz) + C[2], C[1] * (yc_ * iz) + C[3]
            pur = pu - C[4] * iz
            pl = plevel[b].astype(np.int64)
            live = pl != 0xFF
            r = np.asarray(radius, np.int64)[np.minimum(pl, len(levels) - 1)]
            win = (live[:, None] & (lt[None, :] >= 0) & (lt[None, :] >= pl[:, None] - below) & (lt[None, :] <= pl[:, None] + above)
                   & (np.abs(pred[b, :, 0].astype(np.int64)[:, None] - X[None, :]) <= r[:, None])
                   & (np.abs(pred[b, :, 1].astype(np.int64)[:, None] - Y[None, :]) <= r[:, None]))
            o = np.clip(obs[b, :n].astype(np.int64), -(1 << 22), 1 << 22).astype(F) * F(1.0 / 256.0)
            mono = obs[b, :n, 2] == -(1 << 31)
            w = np.asarray(inv_sigma2, F)[np.maximum(lt, 0)][None, :]
            ex, ey, er = pu[:, None] - o[None, :, 0], pv[:, None] - o[None, :, 1], pur[:, None] - o[None, :, 2]
            e2 = ex * ex + ey * ey
            ok = np.where(mono[None, :], e2 * w <= F(chi2_mono), (e2 + er * er) * w <= F(chi2_stereo))
        window += int(win.sum())
        removed += int((win & ~ok).sum())
    return window, removed


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--points", type=int, default=2048, help="map points per frame (the query stride)")
    ap.add_argument("--th", type=float, default=3.0)
    ap.add_argument("--iters", type=int, default=200, help="timed rounds (every call once per round)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--stat-frames", type=int, default=8, help="frames whose candidates are counted on the host")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_fuse needs a GPU (there is no CPU fallback)")
    from pislam_amd import synth
    from pislam_amd.capi import Context
    from pislam_amd.frontend import (OrbFrontend, level_scales_q16, matchFuseBatch, matchProjectionBatch, poseLevelWeights,
                                     poseObservationsQ8, projectionRadii, reserveMatchFuse, reserveMatchProjection)
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
    fuse_r = projectionRadii(scale, args.th, near=1, far=1)[0]
    inv_sigma2 = poseLevelWeights(len(levels))
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
        n = np.minimum(np.where(hc == 0xFFFFFFFF, 0, hc), max_kp).astype(np.int64)
        xw_h, dr_h, nr_h, src = make_points(rng, hk, n, levels, scale, level_scale, Q)
        qd = T(np.stack([hd[b][src[b]] for b in range(B)]))
        xw, drange, normal = T(xw_h), T(dr_h), T(nr_h)
        qc = torch.full((B,), Q, dtype=torch.int32, device=dev)
        # the observations: half the keypoints stereo, disparity bf / z of the first point made from the keypoint
        disp = np.full(hk.shape, -1, np.int64)
        m = min(Q, hk.shape[1])
        disp[:, :m] = np.floor(256.0 * BF / xw_h[:, :m, 2] + rng.normal(0, 64, (B, m)) + 0.5).astype(np.int64)
        disp[rng.random(hk.shape) < 0.5] = -1
        tobs, _ = poseObservationsQ8(tk, levels, scale, disp_q8=T(np.maximum(disp, -1)))
        a = np.deg2rad(0.3)
        pose_h = np.tile(np.array([np.cos(a), 0, np.sin(a), 0, 1, 0, -np.sin(a), 0, np.cos(a), 0.02, 0, 0], np.float32), (B, 1))
        cam_h = np.tile(np.array([FX, FY, CX, CY, BF], np.float32), (B, 1))
        pose, cam = T(pose_h), T(cam_h)
        reserveMatchFuse(levels, max_kp, B, scale_q16=scale, radius_far=fuse_r.tolist(), words=words, ctx=ctx)
        reserveMatchProjection(levels, max_kp, B, scale_q16=scale, radius_far=far.tolist(), radius_near=near.tolist(),
                               words=words, ctx=ctx)
        out = [torch.empty((B, Q), dtype=torch.int32, device=dev) for _ in range(3)]
        pred = torch.empty((B, Q, 2), dtype=torch.int32, device=dev)
        plevel = torch.empty((B, Q), dtype=torch.uint8, device=dev)
        out2 = [torch.empty((B, Q), dtype=torch.int32, device=dev) for _ in range(3)]
        pred2 = torch.empty((B, Q, 2), dtype=torch.int32, device=dev)
        plevel2 = torch.empty((B, Q), dtype=torch.uint8, device=dev)

        def fuse():
            matchFuseBatch(pose, cam, xw, qd, qc, tk, td, tobs, tc, levels, drange=drange, normal=normal, scale_q16=scale,
                           level_scale=level_scale, radius_far=fuse_r.tolist(), inv_sigma2=inv_sigma2, idx=out[0],
                           dist=out[1], dist2=out[2], pred=pred, plevel=plevel, ctx=ctx)

        def projection():
            matchProjectionBatch(pose, cam, xw, qd, qc, tk, td, tc, levels, drange=drange, normal=normal, scale_q16=scale,
                                 level_scale=level_scale, radius_far=far.tolist(), radius_near=near.tolist(), idx=out2[0],
                                 dist=out2[1], dist2=out2[2], pred=pred2, plevel=plevel2, ctx=ctx)

        ins = [pose, cam, xw, qd, qc, drange, normal, tk, td, tobs, tc]
        dup = [torch.empty_like(t) for t in ins]

        def copy():
            for s, d in zip(ins, dup):
                d.copy_(s, non_blocking=True)

        calls = {"fuse": fuse, "projection": projection, "copy": copy}
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
        live = plevel.cpu().numpy() != 0xFF
        matched = out[0].cpu().numpy() >= 0
        matched_proj = out2[0].cpu().numpy() >= 0
        frames = range(min(B, args.stat_frames))
        window, removed = removed_share(frames, pose_h, cam_h, xw_h, pred.cpu().numpy(), plevel.cpu().numpy(), hk, n,
                                        tobs.cpu().numpy(), levels, scale, fuse_r, inv_sigma2, 1, 0, 5.99, 7.8)
    ms = {}
    for k in calls:
        t = np.array([a.elapsed_time(b) for a, b in ev[k]])
        ms[k] = {"median": round(float(np.median(t)), 4), "p10": round(float(np.percentile(t, 10)), 4),
                 "p90": round(float(np.percentile(t, 90)), 4)}
    print(json.dumps({
        "tool": "bench_fuse", "frames": B, "points_per_frame": Q, "th": args.th, "iters": args.iters, "words": words,
        "mean_train_per_frame": round(float(n.mean()), 1), "stereo_share": round(float((disp >= 0).mean()), 4),
        "live_share": round(float(live.mean()), 4), "matched_share": round(float(matched.mean()), 4),
        "projection_matched_share": round(float(matched_proj.mean()), 4), "ms": ms,
        "fuse_over_projection": round(ms["fuse"]["median"] / ms["projection"]["median"], 3),
        "window_candidates": window, "removed_by_test": removed,
        "removed_share": round(removed / max(window, 1), 4), "stat_frames": len(frames),
        "input_bytes": int(sum(t.numel() * t.element_size() for t in ins)),
        "radius_fuse": fuse_r.tolist(), "radius_far": far.tolist(), "radius_near": near.tolist(), "scale_q16": scale}))


if __name__ == "__main__":
    main()
