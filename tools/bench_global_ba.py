"""Global bundle adjustment of whole maps (pislam_global_ba_batch) on synthetic maps, next to a device copy of its input
bytes and, for one window, to the local call; prints one JSON line.

Setup: key frames 0.1 apart on a line, looking along z at points 4 to 8 in front of them; a point is seen by the
`observations / points` key frames nearest to it; 0.5 px of noise, half of the observations stereo, 5 % of them moved by
20 px; the free poses and the points start off the truth by about 0.002 rad, 0.01 and 0.02 units.  Key frame 0 is held
(ORB-SLAM's gauge).  Three shapes: `big`, one map of --big-kfs key frames, --big-points points and --big-obs
observations; `local`, --maps maps of --kfs key frames (the covisibility bench's two shapes); `window`, one window at the
local call's limits (32 key frames of which 16 free, 4096 points, 16384 observations), run through both calls.  Timed,
each as the median device-event time of single calls after a warm-up (the workspace is reserved first): the call with
ORB-SLAM's schedule (one robust round of 10 iterations) and --cg-iters / --cg-tol, and a device-to-device copy of its
input bytes.  launches_issued is the fixed sequence of the call; launches_with_work counts, from the call's own `work` and
`status` words, the launches in which the busiest map of the batch still had work: 7 + per solve begun 4 (factors, set-up,
PCG start, decision) + 3 per PCG iteration + 2 per trial state (step, pass) + 2 per round."""
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

from bench_local_ba import CAM, MONO, rotations  # noqa: E402
from bench_sim3 import timed  # noqa: E402


def make_map(rng, nk, npt, nobs, fixed):
    """(poses, xw, kf, pt, obs, fixed) of one map; the list is sorted by point and by key frame within a point."""
    per = int(max(2, min(nk, round(nobs / npt))))
    R = rotations(rng.normal(0, 0.01, (nk, 3)))
    c = np.stack([0.1 * np.arange(nk), rng.normal(0, 0.05, nk), rng.normal(0, 0.05, nk)], 1)
    t = -np.einsum("kij,kj->ki", R, c)
    xw = np.stack([rng.uniform(0, 0.1 * (nk - 1), npt) if nk > 1 else np.zeros(npt), rng.uniform(-1.5, 1.5, npt),
                   rng.uniform(4, 8, npt)], 1)
    first = np.clip(np.rint(xw[:, 0] / 0.1).astype(np.int64) - per // 2, 0, nk - per)
    pt = np.repeat(np.arange(npt), per)
    kf = (first[:, None] + np.arange(per)[None, :]).reshape(-1)
    n = len(pt)
    xc = np.einsum("nij,nj->ni", R[kf], xw[pt]) + t[kf]
    u = CAM[0] * xc[:, 0] / xc[:, 2] + CAM[2] + rng.normal(0, 0.5, n)
    v = CAM[1] * xc[:, 1] / xc[:, 2] + CAM[3] + rng.normal(0, 0.5, n)
    ur = u - CAM[4] / xc[:, 2] + rng.normal(0, 0.5, n)
    gross = rng.random(n) < 0.05
    a = rng.uniform(0, 2 * np.pi, n)
    u, v = u + 20 * gross * np.cos(a), v + 20 * gross * np.sin(a)
    obs = np.stack([np.rint(256 * u), np.rint(256 * v), np.where(rng.random(n) < 0.5, np.rint(256 * ur), MONO)], 1)
    free = ~fixed
    R0, t0 = R.copy(), t.copy()
    R0[free] = rotations(rng.normal(0, 0.002 / np.sqrt(3), (int(free.sum()), 3))) @ R[free]
    t0[free] += rng.normal(0, 0.01 / np.sqrt(3), (int(free.sum()), 3))
    poses = np.concatenate([R0.reshape(nk, 9), t0], 1)
    return poses, xw + rng.normal(0, 0.02 / np.sqrt(3), xw.shape), kf, pt, obs.astype(np.int64)


def launches(rounds, iters, cg_iters):
    return 7 + sum(it * (6 + 3 * cg_iters) + 2 for it in iters[:rounds])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--maps", type=int, default=256)
    ap.add_argument("--kfs", type=int, default=32)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--obs", type=int, default=5000)
    ap.add_argument("--big-kfs", type=int, default=2048)
    ap.add_argument("--big-points", type=int, default=100000)
    ap.add_argument("--big-obs", type=int, default=1000000)
    ap.add_argument("--cg-iters", type=int, default=50)
    ap.add_argument("--cg-tol", type=float, default=1e-4)
    ap.add_argument("--iters", type=int, default=5, help="timed calls per entry")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--shapes", default="big,local,window")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_global_ba needs a GPU (there is no CPU fallback)")
    from pislam_amd.capi import Context
    from pislam_amd.frontend import (globalBundleAdjustBatch, keyFrameObservationIndex, localBundleAdjustBatch,
                                     reserveGlobalBundleAdjust, reserveLocalBundleAdjust)
    rng = np.random.default_rng(args.seed)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx = Context(device=0, stream=stream.cuda_stream)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sched = dict(rounds=1, iters=(10,), huber_rounds=1, min_obs=10, eps=1e-6, cg_iters=args.cg_iters, cg_tol=args.cg_tol)
    results = {}

    def run(name, B, nk, npt, nobs, nfixed_last=0):
        fixed = np.zeros(nk, bool)
        if nfixed_last:
            fixed[nk - nfixed_last:] = True
        else:
            fixed[0] = True
        maps = [make_map(rng, nk, npt, nobs, fixed) for _ in range(B)]
        S = max(len(m[2]) for m in maps)
        poses = np.stack([m[0] for m in maps]).astype(np.float32)
        xw = np.stack([m[1] for m in maps]).astype(np.float32)
        cams = np.tile(CAM.astype(np.float32), (B, nk, 1))
        kf, pt = np.zeros((B, S), np.int16), np.zeros((B, S), np.int32)
        obs, counts = np.zeros((B, S, 3), np.int32), np.zeros(B, np.int32)
        for b, m in enumerate(maps):
            n = len(m[2])
            kf[b, :n], pt[b, :n], obs[b, :n], counts[b] = m[2], m[3], m[4], n
        full = lambda v: T(np.full(B, v, np.int32))
        res = {"maps": B, "key_frames": nk, "points": npt, "stride": S, "mean_observations": round(float(counts.mean()), 1)}
        with torch.cuda.stream(stream):
            dkf, dcounts = T(kf), T(counts)
            kf_ptr, kf_obs = keyFrameObservationIndex(dkf, dcounts, nk)
            ins = [T(poses), T(cams), T(np.tile(fixed.astype(np.uint8), (B, 1))), full(nk), T(xw), full(npt), T(obs), dkf, T(pt),
                   dcounts, kf_ptr, kf_obs]
            torch.cuda.current_stream().synchronize()
            reserveGlobalBundleAdjust(nk, npt, S, B, ctx=ctx)
            names = ("poses_out", "xw_out", "inlier", "ninliers", "cost", "status", "work")
            keep = dict(zip(names, globalBundleAdjustBatch(*ins, ctx=ctx, **sched)))
            res["global_ba_ms"] = round(timed(lambda: globalBundleAdjustBatch(*ins, ctx=ctx, **sched, **keep), stream, torch,
                                              args.warmup, args.iters), 3)
            dst = [torch.empty_like(a) for a in ins]

            def copy():
                for d, s in zip(dst, ins):
                    d.copy_(s)
            res["copy_inputs_ms"] = round(timed(copy, stream, torch, args.warmup, args.iters), 4)
            res["input_bytes"] = int(sum(a.numel() * a.element_size() for a in ins))
            stream.synchronize()
            out = {k: v.cpu().numpy() for k, v in keep.items()}
            solves, cg = out["work"][:, 0].astype(np.int64), out["work"][:, 1].astype(np.int64)
            trials = (out["status"] >> 8).astype(np.int64) - 2
            res.update({"codes_ok": int((out["status"] & 255 == 0).sum()), "solves": int(solves.max()),
                        "pcg_iterations": int(cg.max()), "mean_pcg_iterations": round(float(cg.mean()), 1),
                        "ms_per_pcg_iteration": round(res["global_ba_ms"] / max(int(cg.max()), 1), 4),
                        "launches_issued": launches(1, (10,), args.cg_iters),
                        "launches_with_work": int((7 + 4 * solves + 3 * cg + 2 * np.maximum(trials, 0) + 2).max()),
                        "mean_inliers": round(float(out["ninliers"].mean()), 1),
                        "mean_cost_per_inlier": round(float((out["cost"] / np.maximum(out["ninliers"], 1)).mean()), 4)})
            if nfixed_last:                                  # the same window through the local call, its own schedule's shape
                nfree = nk - nfixed_last
                lins = [ins[0], ins[1], full(nk), full(nfree), ins[4], full(npt), ins[6], T(kf.astype(np.uint8)), T(pt.astype(np.int16)),
                        dcounts]
                lsched = {k: sched[k] for k in ("rounds", "iters", "huber_rounds", "min_obs", "eps")}
                reserveLocalBundleAdjust(nk, npt, S, B, ctx=ctx)
                lk = dict(zip(names[:6], localBundleAdjustBatch(*lins, ctx=ctx, **lsched)))
                res["local_ba_ms"] = round(timed(lambda: localBundleAdjustBatch(*lins, ctx=ctx, **lsched, **lk), stream, torch,
                                                 args.warmup, args.iters), 3)
                stream.synchronize()
                lc = lk["cost"].cpu().numpy()
                res["local_cost"], res["global_cost"] = round(float(lc[0]), 4), round(float(out["cost"][0]), 4)
                res["masks_equal"] = bool((lk["inlier"].cpu().numpy() == out["inlier"]).all())
        results[name] = res

    shapes = args.shapes.split(",")
    if "big" in shapes:
        run("big", 1, args.big_kfs, args.big_points, args.big_obs)
    if "local" in shapes:
        run("local", args.maps, args.kfs, args.points, args.obs)
    if "window" in shapes:
        run("window", 1, 32, 4096, 16384, nfixed_last=16)
    print(json.dumps({"tool": "bench_global_ba", "iters": args.iters, "cg_iters": args.cg_iters, "cg_tol": args.cg_tol,
                      "results": results}))


if __name__ == "__main__":
    main()
