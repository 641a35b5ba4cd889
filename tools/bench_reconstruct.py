"""Batched two-view reconstruction (pislam_two_view_reconstruct_batch) on synthetic matched pairs, next to a device
copy of the same input bytes and to the two-view RANSAC call on the same batch; prints one JSON line.

Setup: `pairs` camera pairs (fx = fy = 500, cx = 320, cy = 240; a rotation of a few degrees and a baseline of 0.5 with
points 4 to 12 units away), each with about `matches` matches in Q8 with 0.5 px of noise, 20 % of them with a random
partner.  pislam_two_view_ransac_batch (F, `hypotheses` hypotheses) gives the inlier mask.  The reconstruction runs on
the masked matches with 4 candidates (the four motions of the true essential matrix) and with 8 (four wrong motions
added), default parameters.  Timed, each as the median device-event time of single calls after a warm-up: the
reconstruction at 4 and at 8 candidates, a device-to-device copy of its input bytes (points, counts, mask, cameras,
candidates), and the RANSAC call.  Also run once, untimed: the whole host chain twoViewDenormalise -> twoViewCandidates
on the RANSAC's own F (not refitted from the inliers), and the reconstruction from those candidates."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CAM = np.array([500, 500, 320, 240], np.float32)


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


def motion(R, t):
    return np.concatenate([R.reshape(9), t]).astype(np.float32)


def scene(rng, n, outliers=0.2, noise=0.5):
    R = rodrigues(rng.normal(0, 0.04, 3))
    t = np.array([-0.5, 0, 0]) + rng.normal(0, 0.05, 3)
    z = rng.uniform(4, 12, n)
    X1 = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], 1)
    X2 = X1 @ R.T + t
    px = lambda X: np.stack([500 * X[:, 0] / X[:, 2] + 320, 500 * X[:, 1] / X[:, 2] + 240], 1) + rng.normal(0, noise, (n, 2))
    u, v = px(X1), px(X2)
    bad = rng.permutation(n)[:int(round(outliers * n))]
    v[bad] = np.stack([rng.uniform(0, 640, len(bad)), rng.uniform(0, 480, len(bad))], 1)
    good = np.ones(n, bool)
    good[bad] = False
    tu = t / np.linalg.norm(t)
    R2 = (2 * np.outer(tu, tu) - np.eye(3)) @ R
    four = [motion(R, tu), motion(R2, tu), motion(R, -tu), motion(R2, -tu)]
    wrong = [motion(rodrigues(rng.normal(0, 0.1, 3)) @ R, tu), motion(np.eye(3), tu), motion(R, np.array([0, 0, 1.0])),
             motion(R.T, -tu)]
    return np.rint(u * 256).astype(np.int32), np.rint(v * 256).astype(np.int32), good, np.stack(four + wrong), X1[:, 2] / np.linalg.norm(t)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--matches", type=int, default=800, help="mean matches per pair (uniform within +- 100)")
    ap.add_argument("--hypotheses", type=int, default=200)
    ap.add_argument("--iters", type=int, default=100, help="timed calls per entry point")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_reconstruct needs a GPU (there is no CPU fallback)")
    from pislam_amd.capi import Context
    from pislam_amd.frontend import twoViewCandidates, twoViewDenormalise, twoViewRansacBatch, twoViewReconstructBatch
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx = Context(device=0, stream=stream.cuda_stream)
    B, S = args.pairs, args.matches + 100
    rng = np.random.default_rng(args.seed)
    p1, p2 = np.zeros((B, S, 2), np.int32), np.zeros((B, S, 2), np.int32)
    counts, cand, truth, depth = np.zeros(B, np.int32), np.zeros((B, 8, 12), np.float32), [], []
    for b in range(B):
        n = int(rng.integers(args.matches - 100, args.matches + 101))
        p1[b, :n], p2[b, :n], good, cand[b], z = scene(rng, n)
        counts[b] = n
        truth.append(good)
        depth.append(z)
    res = {}
    names = ("best", "status", "ngood", "npar", "pose_out", "xw", "point")
    with torch.cuda.stream(stream):
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        p1_d, p2_d, n_d, cam_d = T(p1), T(p2), T(counts), T(np.tile(CAM, (B, 1)))
        tv = twoViewRansacBatch(p1_d, p2_d, n_d, model="F", hypotheses=args.hypotheses, seed=args.seed, ctx=ctx)
        tvk = dict(zip(("best", "score", "ninliers", "inlier", "model_n", "stats"), tv))
        mask = tvk["inlier"]
        out = {}
        for k in (4, 8):
            c_d = T(cand[:, :k])
            o = twoViewReconstructBatch(p1_d, p2_d, n_d, cam_d, c_d, mask=mask, ctx=ctx)
            keep = dict(zip(names, o))
            run = lambda: twoViewReconstructBatch(p1_d, p2_d, n_d, cam_d, c_d, mask=mask, ctx=ctx, **keep)
            res["reconstruct_%d_candidates_ms" % k] = round(timed(run, stream, torch, args.warmup, args.iters), 4)
            out[k] = {kk: v.cpu().numpy() for kk, v in keep.items()}
        src = [p1_d, p2_d, n_d, mask, cam_d, c_d]
        dst = [torch.empty_like(a) for a in src]

        def copy():
            for d, s in zip(dst, src):
                d.copy_(s)
        res["copy_inputs_ms"] = round(timed(copy, stream, torch, args.warmup, args.iters), 4)
        res["input_bytes"] = int(sum(a.numel() * a.element_size() for a in src))
        res["two_view_F_%d_ms" % args.hypotheses] = round(timed(
            lambda: twoViewRansacBatch(p1_d, p2_d, n_d, model="F", hypotheses=args.hypotheses, seed=args.seed, ctx=ctx, **tvk),
            stream, torch, args.warmup, args.iters), 4)
        # the host chain on the RANSAC's own model
        F = twoViewDenormalise("F", tvk["model_n"], tvk["stats"])
        own = twoViewCandidates("F", F, CAM)                      # NaN rows where the RANSAC found no model
        chain = dict(zip(names, twoViewReconstructBatch(p1_d, p2_d, n_d, cam_d, T(own), mask=mask, ctx=ctx)))
        chain = {k: v.cpu().numpy() for k, v in chain.items()}
        inl = mask.cpu().numpy()
    for k in (4, 8):
        st = out[k]["status"]
        res["codes_%d" % k] = [int((st & 255 == c).sum()) for c in range(5)]
        res["true_motion_chosen_%d" % k] = int(((st & 255 == 0) & (out[k]["best"] == 0)).sum())
    err, pts = [], []
    for b in range(B):
        n = counts[b]
        pt = out[4]["point"][b, :n].astype(bool) & truth[b]
        if pt.any():
            err.append(np.median(np.abs(out[4]["xw"][b, :n][pt, 2] - depth[b][pt]) / depth[b][pt]))
        pts.append(out[4]["point"][b, :n].sum() / max(int(inl[b, :n].sum()), 1))
    rot = []
    for b in range(B):
        if chain["status"][b] & 255 == 0:
            Re, Rt = chain["pose_out"][b, :9].astype(np.float64).reshape(3, 3), cand[b, 0, :9].astype(np.float64).reshape(3, 3)
            rot.append(np.degrees(np.arccos(np.clip((np.trace(Re @ Rt.T) - 1) / 2, -1, 1))))
    res.update({"pairs": B, "stride": S, "mean_matches": round(float(counts.mean()), 1),
                "mean_inliers": round(float(np.mean([inl[b, :counts[b]].sum() for b in range(B)])), 1),
                "points_per_inlier_4": round(float(np.mean(pts)), 4),
                "median_relative_depth_error_4": round(float(np.median(err)), 5) if err else None,
                "chain_codes": [int((chain["status"] & 255 == c).sum()) for c in range(5)],
                "chain_median_rotation_error_deg": round(float(np.median(rot)), 4) if rot else None})
    print(json.dumps({"tool": "bench_reconstruct", "iters": args.iters, "results": res}))


if __name__ == "__main__":
    main()
