"""Batched absolute-pose RANSAC (pislam_pnp_ransac_batch) on synthetic frames, next to a device copy of the same input
bytes, to the pose call on the same batch and to the two-view call on a batch of the same size; prints one JSON line.

Setup: `frames` frames (fx = fy = 500, cx = 320, cy = 240), each with about `obs` map points whose pixels are uniform
over a VGA image at depths 2..20, a true pose of a rotation of up to 1 rad and a translation of up to 2 per axis, pixel
noise uniform in +-0.75 px, 40 % of the observations displaced by 30..200 px, no level table; `hypotheses` hypotheses.
Timed, each as the median device-event time of single calls after a warm-up: the absolute-pose call, a device-to-device
copy of the input bytes (cameras, points, observations, counts), pislam_pose_refine_batch (default parameters) started
from the call's own pose_out, and pislam_two_view_ransac_batch (F, as many hypotheses) on as many pairs of as many
matches."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MONO = -(1 << 31)


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


def rodrigues(r):
    th = np.linalg.norm(r)
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]) / th
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def scene(rng, n, outliers=0.4, noise=0.75):
    px = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1)
    z = rng.uniform(2, 20, n)
    xc = np.stack([(px[:, 0] - 320) / 500 * z, (px[:, 1] - 240) / 500 * z, z], 1)
    axis = rng.normal(0, 1, 3)
    R, t = rodrigues(axis / np.linalg.norm(axis) * rng.uniform(0.01, 1)), rng.uniform(-2, 2, 3)
    xw = ((xc - t) @ R).astype(np.float32)
    xc = xw.astype(np.float64) @ R.T + t
    uv = np.stack([500 * xc[:, 0] / xc[:, 2] + 320, 500 * xc[:, 1] / xc[:, 2] + 240], 1) + rng.uniform(-noise, noise, (n, 2))
    bad = rng.permutation(n)[:int(round(outliers * n))]
    ang, mag = rng.uniform(0, 2 * np.pi, len(bad)), rng.uniform(30, 200, len(bad))
    uv[bad] += np.stack([np.cos(ang), np.sin(ang)], 1) * mag[:, None]
    obs = np.concatenate([np.rint(uv * 256), np.full((n, 1), MONO)], 1).astype(np.int32)
    good = np.ones(n, bool)
    good[bad] = False
    return xw, obs, R, t, good


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--obs", type=int, default=1000, help="mean observations per frame (uniform within +- 100)")
    ap.add_argument("--hypotheses", type=int, default=200)
    ap.add_argument("--iters", type=int, default=100, help="timed calls per entry point")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pnp needs a GPU (there is no CPU fallback)")
    from pislam_amd.capi import Context
    from pislam_amd.frontend import pnpRansacBatch, poseRefineBatch, twoViewRansacBatch
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx = Context(device=0, stream=stream.cuda_stream)
    B, S, H = args.frames, args.obs + 100, args.hypotheses
    rng = np.random.default_rng(args.seed)
    xw, obs = np.zeros((B, S, 3), np.float32), np.zeros((B, S, 3), np.int32)
    counts, truth = np.zeros(B, np.int32), []
    for b in range(B):
        n = int(rng.integers(args.obs - 100, args.obs + 101))
        xw[b, :n], obs[b, :n], R, t, good = scene(rng, n)
        counts[b] = n
        truth.append((R, t, good))
    cam = np.tile(np.array([500, 500, 320, 240, 50], np.float32), (B, 1))
    res = {}
    with torch.cuda.stream(stream):
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        ins = [T(a) for a in (cam, xw, obs, counts)]
        o = pnpRansacBatch(*ins, hypotheses=H, seed=args.seed, ctx=ctx)
        keep = dict(zip(("best", "score", "ninliers", "inlier", "pose_out", "status"), o))
        run = lambda: pnpRansacBatch(*ins, hypotheses=H, seed=args.seed, ctx=ctx, **keep)
        res["pnp_ransac_ms"] = round(timed(run, stream, torch, args.warmup, args.iters), 4)
        dst = [torch.empty_like(a) for a in ins]

        def copy():
            for d, s in zip(dst, ins):
                d.copy_(s)
        res["copy_inputs_ms"] = round(timed(copy, stream, torch, args.warmup, args.iters), 4)
        res["input_bytes"] = int(sum(a.numel() * a.element_size() for a in ins))
        po = poseRefineBatch(keep["pose_out"], *ins, ctx=ctx)
        pok = dict(zip(("pose_out", "inlier", "ninliers", "cost", "status"), po))
        res["pose_refine_ms"] = round(timed(lambda: poseRefineBatch(keep["pose_out"], *ins, ctx=ctx, **pok), stream, torch,
                                            args.warmup, args.iters), 4)
        p1 = torch.from_numpy(rng.integers(0, 640 * 256, (B, S, 2)).astype(np.int32)).to(dev)
        p2 = p1 + torch.from_numpy(rng.integers(-512, 512, (B, S, 2)).astype(np.int32)).to(dev)
        tv = twoViewRansacBatch(p1, p2, ins[3], model="F", hypotheses=H, seed=args.seed, ctx=ctx)
        tvk = dict(zip(("best", "score", "ninliers", "inlier", "model_n", "stats"), tv))
        res["two_view_F_ms"] = round(timed(lambda: twoViewRansacBatch(p1, p2, ins[3], model="F", hypotheses=H, seed=args.seed,
                                                                      ctx=ctx, **tvk), stream, torch, args.warmup,
                                           args.iters), 4)
        out = {k: v.cpu().numpy() for k, v in keep.items()}
        ref = {k: v.cpu().numpy() for k, v in pok.items()}
    rot, tr, kept, acc, kept2, acc2 = [], [], [], [], [], []
    for b, (R, t, good) in enumerate(truth):
        Re, te = out["pose_out"][b, :9].astype(np.float64).reshape(3, 3), out["pose_out"][b, 9:].astype(np.float64)
        E = Re @ R.T
        s = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]]) / 2
        rot.append(np.degrees(np.arctan2(np.linalg.norm(s), (np.trace(E) - 1) / 2)))
        tr.append(np.linalg.norm(te - t))
        inl, inl2 = out["inlier"][b, :counts[b]].astype(bool), ref["inlier"][b, :counts[b]].astype(bool)
        kept.append(inl[good].mean()), acc.append(inl[~good].mean())
        kept2.append(inl2[good].mean()), acc2.append(inl2[~good].mean())
    res.update({"frames": B, "stride": S, "hypotheses": H, "mean_obs": round(float(counts.mean()), 1),
                "codes_ok": int((out["status"] & 255 == 0).sum()),
                "mean_valid_hypotheses": round(float((out["status"] >> 8).mean()), 1),
                "worst_rotation_deg": round(float(max(rot)), 4), "worst_translation": round(float(max(tr)), 5),
                "true_inliers_kept": round(float(np.mean(kept)), 4), "worst_frame_kept": round(float(np.min(kept)), 4),
                "outliers_accepted": round(float(np.mean(acc)), 4),
                "refined_codes_ok": int((ref["status"] & 255 == 0).sum()),
                "refined_true_inliers_kept": round(float(np.mean(kept2)), 4),
                "refined_outliers_accepted": round(float(np.mean(acc2)), 4)})
    print(json.dumps({"tool": "bench_pnp", "iters": args.iters, "results": res}))


if __name__ == "__main__":
    main()
