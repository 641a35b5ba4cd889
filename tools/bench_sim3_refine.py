"""Batched Sim(3) refinement (pislam_sim3_refine_batch) on synthetic loop candidates, at two shapes, started from the
Sim(3) RANSAC call's result; each next to a device copy of the same input bytes, to the RANSAC call itself and to the
pose call on a batch of the same size; prints one JSON line.

Setup: tools/bench_sim3.py's scenes (`pairs` pairs, about `matches` matches each, pixel noise +-0.75 px, 1 % depth
noise, 40 % of the matches with their camera-2 side replaced, no levels).  The RANSAC call (`hypotheses` hypotheses) runs
once; its sim_out and inlier mask are the refinement's sim_in and mask.  Timed, each as the median device-event time of
single calls after a warm-up: the refinement (ORB-SLAM's schedule: 2 rounds of up to 5 iterations, Huber on, th2 = 10),
a device-to-device copy of its input bytes, the RANSAC call, and pislam_pose_refine_batch (its default schedule) on as
many frames of as many observations (camera 1's pixels against camera 2's points, started from the first twelve words of
the RANSAC result: a pose problem of the same size, not the same problem).  `passes` is the mean number of passes over
a pair's matches (status >> 8), for both optimisers: ms per call / passes compares their cost per pass."""
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

from bench_sim3 import scene, timed  # noqa: E402


def shape(args, torch, ctx, stream, dev, matches, spread):
    from pislam_amd.frontend import poseRefineBatch, sim3RansacBatch, sim3RefineBatch
    B, S, H = args.pairs, matches + spread, args.hypotheses
    rng = np.random.default_rng(args.seed)
    x1, x2 = np.zeros((B, S, 3), np.float32), np.zeros((B, S, 3), np.float32)
    o1, o2 = np.zeros((B, S, 3), np.int32), np.zeros((B, S, 3), np.int32)
    counts, truth = np.zeros(B, np.int32), []
    for b in range(B):
        n = int(rng.integers(matches - spread, matches + spread + 1))
        x1[b, :n], x2[b, :n], o1[b, :n], o2[b, :n], sim, good = scene(rng, n)
        counts[b] = n
        truth.append((sim, good))
    cam = np.tile(np.array([500, 500, 320, 240, 50], np.float32), (B, 1))
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ins = [T(a) for a in (cam, cam, x1, x2, o1, o2, counts)]
    res = {}
    rk = dict(zip(("best", "score", "ninliers", "inlier", "sim_out", "status"),
                  sim3RansacBatch(*ins, hypotheses=H, seed=args.seed, ctx=ctx)))
    res["sim3_ransac_ms"] = round(timed(lambda: sim3RansacBatch(*ins, hypotheses=H, seed=args.seed, ctx=ctx, **rk), stream, torch,
                                        args.warmup, args.iters), 4)
    sim_in, mask = rk["sim_out"], rk["inlier"]
    keep = dict(zip(("sim_out", "inlier", "ninliers", "cost", "status"), sim3RefineBatch(sim_in, *ins, mask=mask, ctx=ctx)))
    run = lambda: sim3RefineBatch(sim_in, *ins, mask=mask, ctx=ctx, **keep)
    res["sim3_refine_ms"] = round(timed(run, stream, torch, args.warmup, args.iters), 4)
    nomask = dict(zip(("sim_out", "inlier", "ninliers", "cost", "status"), sim3RefineBatch(sim_in, *ins, ctx=ctx)))
    res["sim3_refine_no_mask_ms"] = round(timed(lambda: sim3RefineBatch(sim_in, *ins, ctx=ctx, **nomask), stream, torch,
                                                args.warmup, args.iters), 4)
    src = [sim_in, mask] + ins
    dst = [torch.empty_like(a) for a in src]

    def copy():
        for d, s in zip(dst, src):
            d.copy_(s)
    res["copy_inputs_ms"] = round(timed(copy, stream, torch, args.warmup, args.iters), 4)
    res["input_bytes"] = int(sum(a.numel() * a.element_size() for a in src))
    pose = sim_in[:, :12].contiguous()
    po_in = (pose, ins[0], ins[3], ins[4], ins[6])
    pk = dict(zip(("pose_out", "inlier", "ninliers", "cost", "status"), poseRefineBatch(*po_in, ctx=ctx)))
    res["pose_refine_ms"] = round(timed(lambda: poseRefineBatch(*po_in, ctx=ctx, **pk), stream, torch, args.warmup, args.iters), 4)
    stream.synchronize()
    out = {k: v.cpu().numpy() for k, v in keep.items()}
    before = {k: v.cpu().numpy() for k, v in rk.items()}
    passes, pose_passes = out["status"] >> 8, pk["status"].cpu().numpy() >> 8
    rot, scl, rot0, scl0, kept, acc = [], [], [], [], [], []

    def errors(sim, R, s):
        E = sim[:9].astype(np.float64).reshape(3, 3) @ R.T
        v = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]]) / 2
        return np.degrees(np.arctan2(np.linalg.norm(v), (np.trace(E) - 1) / 2)), abs(float(sim[12]) / s - 1)
    for b, ((R, t, s), good) in enumerate(truth):
        if before["status"][b] & 255 or out["status"][b] & 255:
            continue
        r0, s0 = errors(before["sim_out"][b], R, s)
        r1, s1 = errors(out["sim_out"][b], R, s)
        rot0.append(r0), scl0.append(s0), rot.append(r1), scl.append(s1)
        inl = out["inlier"][b, :counts[b]].astype(bool)
        kept.append(inl[good].mean()), acc.append(inl[~good].mean())
    res.update({"pairs": B, "stride": S, "hypotheses": H, "mean_matches": round(float(counts.mean()), 1),
                "codes_ok": int((out["status"] & 255 == 0).sum()),
                "passes": round(float(passes.mean()), 2), "pose_passes": round(float(pose_passes.mean()), 2),
                "refine_us_per_pass": round(1e3 * res["sim3_refine_ms"] / float(passes.mean()), 2),
                "pose_us_per_pass": round(1e3 * res["pose_refine_ms"] / float(pose_passes.mean()), 2),
                "mean_rotation_deg_before": round(float(np.mean(rot0)), 4), "mean_rotation_deg": round(float(np.mean(rot)), 4),
                "mean_scale_error_before": round(float(np.mean(scl0)), 5), "mean_scale_error": round(float(np.mean(scl)), 5),
                "mean_inliers_before": round(float(before["ninliers"].mean()), 1),
                "mean_inliers": round(float(out["ninliers"].mean()), 1),
                "true_inliers_kept": round(float(np.mean(kept)), 4), "outliers_accepted": round(float(np.mean(acc)), 4)})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--matches", type=int, default=1000, help="mean matches per pair of the large shape (uniform within +- 100)")
    ap.add_argument("--loop-matches", type=int, default=100, help="mean matches per pair of the loop-closing shape (+- 20)")
    ap.add_argument("--hypotheses", type=int, default=200)
    ap.add_argument("--iters", type=int, default=100, help="timed calls per entry point")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sim3_refine needs a GPU (there is no CPU fallback)")
    from pislam_amd.capi import Context
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx = Context(device=0, stream=stream.cuda_stream)
    with torch.cuda.stream(stream):
        res = {"large_shape": shape(args, torch, ctx, stream, dev, args.matches, 100),
               "loop_shape": shape(args, torch, ctx, stream, dev, args.loop_matches, 20)}
    print(json.dumps({"tool": "bench_sim3_refine", "iters": args.iters, "results": res}))


if __name__ == "__main__":
    main()
