"""Batched local bundle adjustment (pislam_local_ba_batch) on synthetic windows, next to a device copy of its input
bytes and to the pose call on as many frames of as many observations; prints one JSON line.

Setup: `windows` windows of `free` free and `fixed` fixed key frames on an arc in front of `points` map points; a point
is seen by a key frame with the probability that gives about `observations` observations per window; 0.5 px of noise,
half of the observations stereo, 5 % of them moved by 20 px; the free poses and the points start off the truth by about
0.002 rad, 0.01 and 0.02 units.  Timed, each as the median device-event time of single calls after a warm-up (the
workspace is reserved first): the call with ORB-SLAM's schedule (2 rounds of up to 5 and 10 iterations, the first
robust), a device-to-device copy of its input bytes, and pislam_pose_refine_batch (its default schedule) on `windows`
frames of `observations` observations (the window's points seen from its first key frame: a pose problem of the same
size, not the same problem).  `passes` is the mean number of passes over a window's observations (status >> 8)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_sim3 import timed  # noqa: E402

MONO = -(1 << 31)
CAM = np.array([500, 500, 320, 240, 40], np.float64)


def rotations(v):
    """Rodrigues for rows of rotation vectors."""
    th = np.linalg.norm(v, axis=1)[:, None, None]
    k = v / np.maximum(th[:, :, 0], 1e-12)
    K = np.zeros((len(v), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def window(rng, nkf, nfree, npt, nobs):
    xw = np.stack([rng.uniform(-2, 2, npt), rng.uniform(-1.5, 1.5, npt), rng.uniform(4, 8, npt)], 1)
    k = np.arange(nkf) - nkf / 2
    R = rotations(np.stack([np.zeros(nkf), 0.02 * k, np.zeros(nkf)], 1) + rng.normal(0, 0.01, (nkf, 3)))
    c = np.stack([0.12 * k, rng.normal(0, 0.05, nkf), rng.normal(0, 0.05, nkf)], 1)
    t = -np.einsum("kij,kj->ki", R, c)
    pt, kf = np.nonzero(rng.random((npt, nkf)) < nobs / (npt * nkf))          # sorted by point, then key frame
    xc = np.einsum("nij,nj->ni", R[kf], xw[pt]) + t[kf]
    u = CAM[0] * xc[:, 0] / xc[:, 2] + CAM[2] + rng.normal(0, 0.5, len(pt))
    v = CAM[1] * xc[:, 1] / xc[:, 2] + CAM[3] + rng.normal(0, 0.5, len(pt))
    ur = u - CAM[4] / xc[:, 2] + rng.normal(0, 0.5, len(pt))
    gross = rng.random(len(pt)) < 0.05
    a = rng.uniform(0, 2 * np.pi, len(pt))
    u, v = u + 20 * gross * np.cos(a), v + 20 * gross * np.sin(a)
    obs = np.stack([np.rint(256 * u), np.rint(256 * v), np.where(rng.random(len(pt)) < 0.5, np.rint(256 * ur), MONO)], 1)
    R0 = R.copy()
    R0[:nfree] = rotations(rng.normal(0, 0.002 / np.sqrt(3), (nfree, 3))) @ R[:nfree]
    t0 = t.copy()
    t0[:nfree] += rng.normal(0, 0.01 / np.sqrt(3), (nfree, 3))
    poses = np.concatenate([R0.reshape(nkf, 9), t0], 1)
    truth = np.concatenate([R.reshape(nkf, 9), t], 1)
    return poses, truth, xw + rng.normal(0, 0.02 / np.sqrt(3), xw.shape), xw, kf, pt, obs.astype(np.int64)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--free", type=int, default=8)
    ap.add_argument("--fixed", type=int, default=8)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--observations", type=int, default=5000, help="mean observations per window")
    ap.add_argument("--iters", type=int, default=30, help="timed calls per entry point")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_local_ba needs a GPU (there is no CPU fallback)")
    from pislam_amd.capi import Context
    from pislam_amd.frontend import localBundleAdjustBatch, poseRefineBatch, reserveLocalBundleAdjust
    B, nkf, nfree, npt = args.windows, args.free + args.fixed, args.free, args.points
    rng = np.random.default_rng(args.seed)
    wins = [window(rng, nkf, nfree, npt, args.observations) for _ in range(B)]
    S = max(len(w[4]) for w in wins)
    poses = np.stack([w[0] for w in wins]).astype(np.float32)
    xw = np.stack([w[2] for w in wins]).astype(np.float32)
    cams = np.tile(CAM.astype(np.float32), (B, nkf, 1))
    kf, pt = np.zeros((B, S), np.uint8), np.zeros((B, S), np.int16)
    obs, counts = np.zeros((B, S, 3), np.int32), np.zeros(B, np.int32)
    for b, w in enumerate(wins):
        n = len(w[4])
        kf[b, :n], pt[b, :n], obs[b, :n], counts[b] = w[4], w[5], w[6], n
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx = Context(device=0, stream=stream.cuda_stream)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    full = lambda v: T(np.full(B, v, np.int32))
    res = {}
    with torch.cuda.stream(stream):
        ins = [T(poses), T(cams), full(nkf), full(nfree), T(xw), full(npt), T(obs), T(kf), T(pt), T(counts)]
        reserveLocalBundleAdjust(nkf, npt, S, B, ctx=ctx)
        names = ("poses_out", "xw_out", "inlier", "ninliers", "cost", "status")
        keep = dict(zip(names, localBundleAdjustBatch(*ins, ctx=ctx)))
        res["local_ba_ms"] = round(timed(lambda: localBundleAdjustBatch(*ins, ctx=ctx, **keep), stream, torch, args.warmup,
                                         args.iters), 4)
        dst = [torch.empty_like(a) for a in ins]

        def copy():
            for d, s in zip(dst, ins):
                d.copy_(s)
        res["copy_inputs_ms"] = round(timed(copy, stream, torch, args.warmup, args.iters), 4)
        res["input_bytes"] = int(sum(a.numel() * a.element_size() for a in ins))
        # the pose call on as many frames of as many observations: every observation's point against key frame 0's camera
        pxw = np.zeros((B, S, 3), np.float32)
        pobs = np.zeros((B, S, 3), np.int32)
        for b, w in enumerate(wins):
            n = len(w[4])
            X = w[3][w[5]]
            xc = X @ w[1][0, :9].reshape(3, 3).T + w[1][0, 9:]
            pxw[b, :n] = X
            pobs[b, :n] = np.stack([np.rint(256 * (CAM[0] * xc[:, 0] / xc[:, 2] + CAM[2] + rng.normal(0, 0.5, n))),
                                    np.rint(256 * (CAM[1] * xc[:, 1] / xc[:, 2] + CAM[3] + rng.normal(0, 0.5, n))),
                                    np.full(n, MONO)], 1)
        po_in = (T(poses[:, 0]), T(cams[:, 0]), T(pxw), T(pobs), T(counts))
        pk = dict(zip(("pose_out", "inlier", "ninliers", "cost", "status"), poseRefineBatch(*po_in, ctx=ctx)))
        res["pose_refine_ms"] = round(timed(lambda: poseRefineBatch(*po_in, ctx=ctx, **pk), stream, torch, args.warmup,
                                            args.iters), 4)
        stream.synchronize()
    out = {k: v.cpu().numpy() for k, v in keep.items()}
    passes, pose_passes = out["status"] >> 8, pk["status"].cpu().numpy() >> 8
    res.update({"windows": B, "free": nfree, "fixed": nkf - nfree, "points": npt, "stride": S,
                "mean_observations": round(float(counts.mean()), 1), "codes_ok": int((out["status"] & 255 == 0).sum()),
                "passes": round(float(passes.mean()), 2), "pose_passes": round(float(pose_passes.mean()), 2),
                "local_ba_us_per_pass": round(1e3 * res["local_ba_ms"] / float(passes.mean()), 2),
                "pose_us_per_pass": round(1e3 * res["pose_refine_ms"] / float(pose_passes.mean()), 2),
                "mean_inliers": round(float(out["ninliers"].mean()), 1),
                "mean_cost_per_inlier": round(float((out["cost"] / np.maximum(out["ninliers"], 1)).mean()), 4)})
    print(json.dumps({"tool": "bench_local_ba", "iters": args.iters, "results": res}))


if __name__ == "__main__":
    main()
