"""Batched motion-only pose optimisation (pislam_pose_refine_batch) on synthetic frames, next to a device copy of the
same input bytes and to the two-view call on a batch of the same size; prints one JSON line.

Setup: `frames` frames (fx = fy = 500, cx = 320, cy = 240, bf = 50), each with about `obs` map points in front of the
camera, a true pose a small rotation (0.05 rad per axis) and translation (0.2) away from the identity start, pixel noise
0.5 * 1.2^level over levels 0..7, 20 % of the observations displaced by up to 40 px, half of them stereo; default
parameters (4 rounds of up to 10 iterations, 3 of them robust).  Timed, each as the median device-event time of single
calls after a warm-up: the pose call (from which ms per pass = ms / the mean number of evaluations of a frame; the
frames run side by side, so the figure over the longest frame's evaluations is given too), a device-to-device copy of
the input bytes (poses, cameras, points, observations, levels, counts), and pislam_two_view_ransac_batch (F, 200
hypotheses) on as many pairs of as many matches."""
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


def scene(rng, n, stereo=0.5, outliers=0.2):
    xw = np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(3, 15, n)], 1).astype(np.float32)
    R, t = rodrigues(rng.normal(0, 0.05, 3)), rng.normal(0, 0.2, 3)
    xc = xw.astype(np.float64) @ R.T + t
    level = rng.integers(0, 8, n)
    sig = 0.5 * 1.2 ** level
    u = 500 * xc[:, 0] / xc[:, 2] + 320 + rng.normal(0, 1, n) * sig
    v = 500 * xc[:, 1] / xc[:, 2] + 240 + rng.normal(0, 1, n) * sig
    ur = u - 50 / xc[:, 2] + rng.normal(0, 1, n) * sig
    bad = rng.permutation(n)[:int(round(outliers * n))]
    for a in (u, v, ur):
        a[bad] += rng.uniform(-40, 40, len(bad))
    is_stereo = rng.uniform(0, 1, n) < stereo
    obs = np.stack([np.rint(u * 256), np.rint(v * 256), np.where(is_stereo, np.rint(ur * 256), MONO)], 1).astype(np.int64)
    good = np.ones(n, bool)
    good[bad] = False
    return xw, obs.astype(np.int32), level.astype(np.uint8), R, t, good


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--obs", type=int, default=1000, help="mean observations per frame (uniform within +- 100)")
    ap.add_argument("--iters", type=int, default=100, help="timed calls per entry point")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose needs a GPU (there is no CPU fallback)")
    from pislam_amd.capi import Context
    from pislam_amd.frontend import poseLevelWeights, poseRefineBatch, twoViewRansacBatch
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx = Context(device=0, stream=stream.cuda_stream)
    B, S = args.frames, args.obs + 100
    rng = np.random.default_rng(args.seed)
    xw, obs, level = np.zeros((B, S, 3), np.float32), np.zeros((B, S, 3), np.int32), np.zeros((B, S), np.uint8)
    counts, truth = np.zeros(B, np.int32), []
    for b in range(B):
        n = int(rng.integers(args.obs - 100, args.obs + 101))
        xw[b, :n], obs[b, :n], level[b, :n], R, t, good = scene(rng, n)
        counts[b] = n
        truth.append((R, t, good))
    pose = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (B, 1))
    cam = np.tile(np.array([500, 500, 320, 240, 50], np.float32), (B, 1))
    tab = poseLevelWeights(8)
    res = {}
    with torch.cuda.stream(stream):
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        ins = [T(a) for a in (pose, cam, xw, obs, counts)]
        lv = T(level)
        o = poseRefineBatch(*ins, level=lv, inv_sigma2=tab, ctx=ctx)
        keep = dict(zip(("pose_out", "inlier", "ninliers", "cost", "status"), o))
        run = lambda: poseRefineBatch(*ins, level=lv, inv_sigma2=tab, ctx=ctx, **keep)
        res["pose_refine_ms"] = round(timed(run, stream, torch, args.warmup, args.iters), 4)
        src = ins + [lv]
        dst = [torch.empty_like(a) for a in src]

        def copy():
            for d, s in zip(dst, src):
                d.copy_(s)
        res["copy_inputs_ms"] = round(timed(copy, stream, torch, args.warmup, args.iters), 4)
        res["input_bytes"] = int(sum(a.numel() * a.element_size() for a in src))
        p1 = torch.from_numpy(rng.integers(0, 640 * 256, (B, S, 2)).astype(np.int32)).to(dev)
        p2 = p1 + torch.from_numpy(rng.integers(-512, 512, (B, S, 2)).astype(np.int32)).to(dev)
        tv = twoViewRansacBatch(p1, p2, ins[4], model="F", hypotheses=200, seed=args.seed, ctx=ctx)
        tvk = dict(zip(("best", "score", "ninliers", "inlier", "model_n", "stats"), tv))
        res["two_view_F_200_ms"] = round(timed(lambda: twoViewRansacBatch(p1, p2, ins[4], model="F", hypotheses=200,
                                                                          seed=args.seed, ctx=ctx, **tvk), stream, torch,
                                               args.warmup, args.iters), 4)
        out = {k: v.cpu().numpy() for k, v in keep.items()}
    ev = out["status"] >> 8
    rot, tr, kept, acc = [], [], [], []
    for b, (R, t, good) in enumerate(truth):
        Re, te = out["pose_out"][b, :9].astype(np.float64).reshape(3, 3), out["pose_out"][b, 9:].astype(np.float64)
        E = Re @ R.T
        s = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]]) / 2
        rot.append(np.degrees(np.arctan2(np.linalg.norm(s), (np.trace(E) - 1) / 2)))
        tr.append(np.linalg.norm(te - t))
        inl = out["inlier"][b, :counts[b]].astype(bool)
        kept.append(inl[good].mean())
        acc.append(inl[~good].mean())
    res.update({"frames": B, "stride": S, "mean_obs": round(float(counts.mean()), 1), "codes_ok": int((out["status"] & 255 == 0).sum()),
                "mean_evaluations": round(float(ev.mean()), 2), "max_evaluations": int(ev.max()),
                "ms_per_pass": round(res["pose_refine_ms"] / max(float(ev.mean()), 1.0), 5),
                "ms_per_pass_of_the_longest_frame": round(res["pose_refine_ms"] / max(int(ev.max()), 1), 5),
                "worst_rotation_deg": round(float(max(rot)), 4), "worst_translation": round(float(max(tr)), 5),
                "true_inliers_kept": round(float(np.mean(kept)), 4), "outliers_accepted": round(float(np.mean(acc)), 4)})
    print(json.dumps({"tool": "bench_pose", "iters": args.iters, "results": res}))


if __name__ == "__main__":
    main()
