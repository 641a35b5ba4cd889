"""Batched Sim(3) RANSAC (pislam_sim3_ransac_batch) on synthetic loop candidates, at two shapes, each next to a device
copy of the same input bytes and to the absolute-pose call on a batch of the same size; prints one JSON line.

Setup: `pairs` (key frame, candidate) pairs (fx = fy = 500, cx = 320, cy = 240), each with about `matches` matched map
points of camera 1's frustum (pixels uniform over a VGA image, depths 2..20); a similarity of a rotation of up to 0.3
rad, a translation of up to 1 per axis and a scale drift of e^-0.7 .. e^0.7 takes camera 2's frame into camera 1's;
pixel noise uniform in +-0.75 px, 1 % depth noise on the points, 40 % of the matches with their camera-2 side replaced
by a random point; no levels; `hypotheses` hypotheses.  Shapes: the absolute-pose call's (about 1000 matches) and loop
closing's (about 100).  Timed, each as the median device-event time of single calls after a warm-up: the similarity
call, a device-to-device copy of its input bytes, and pislam_pnp_ransac_batch (as many hypotheses) on as many frames of
as many observations (camera 1's pixels against camera 2's points: the fixed-scale part of the same problem)."""
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


def project(X):
    return np.stack([500 * X[:, 0] / X[:, 2] + 320, 500 * X[:, 1] / X[:, 2] + 240], 1)


def frustum(rng, n):
    px = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1)
    z = rng.uniform(2, 20, n)
    return np.stack([(px[:, 0] - 320) / 500 * z, (px[:, 1] - 240) / 500 * z, z], 1)


def scene(rng, n, outliers=0.4, noise=0.75, depth_noise=0.01):
    X1 = frustum(rng, n)
    axis = rng.normal(0, 1, 3)
    R, t = rodrigues(axis / np.linalg.norm(axis) * rng.uniform(0.01, 0.3)), rng.uniform(-1, 1, 3)
    s = float(np.exp(rng.uniform(-0.7, 0.7)))
    X2 = (X1 - t) @ R / s
    uv1 = project(X1) + rng.uniform(-noise, noise, (n, 2))
    uv2 = project(X2) + rng.uniform(-noise, noise, (n, 2))
    X1 = X1 * (1 + depth_noise * rng.normal(0, 1, (n, 1)))
    X2 = X2 * (1 + depth_noise * rng.normal(0, 1, (n, 1)))
    bad = rng.permutation(n)[:int(round(outliers * n))]
    Y = frustum(rng, len(bad)) / s
    X2[bad], uv2[bad] = Y, project(Y)
    q = lambda uv: np.concatenate([np.rint(uv * 256), np.full((n, 1), MONO)], 1).astype(np.int32)
    good = np.ones(n, bool)
    good[bad] = False
    return X1.astype(np.float32), X2.astype(np.float32), q(uv1), q(uv2), (R, t, s), good


def shape(args, torch, ctx, stream, dev, matches, spread):
    from pislam_amd.frontend import pnpRansacBatch, sim3RansacBatch
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
    res = {}
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ins = [T(a) for a in (cam, cam, x1, x2, o1, o2, counts)]
    o = sim3RansacBatch(*ins, hypotheses=H, seed=args.seed, ctx=ctx)
    keep = dict(zip(("best", "score", "ninliers", "inlier", "sim_out", "status"), o))
    run = lambda: sim3RansacBatch(*ins, hypotheses=H, seed=args.seed, ctx=ctx, **keep)
    res["sim3_ransac_ms"] = round(timed(run, stream, torch, args.warmup, args.iters), 4)
    dst = [torch.empty_like(a) for a in ins]

    def copy():
        for d, s in zip(dst, ins):
            d.copy_(s)
    res["copy_inputs_ms"] = round(timed(copy, stream, torch, args.warmup, args.iters), 4)
    res["input_bytes"] = int(sum(a.numel() * a.element_size() for a in ins))
    pn_in = (ins[0], ins[3], ins[4], ins[6])
    pn = pnpRansacBatch(*pn_in, hypotheses=H, seed=args.seed, ctx=ctx)
    pnk = dict(zip(("best", "score", "ninliers", "inlier", "pose_out", "status"), pn))
    res["pnp_ransac_ms"] = round(timed(lambda: pnpRansacBatch(*pn_in, hypotheses=H, seed=args.seed, ctx=ctx, **pnk), stream,
                                       torch, args.warmup, args.iters), 4)
    out = {k: v.cpu().numpy() for k, v in keep.items()}
    rot, scl, kept, acc = [], [], [], []
    for b, ((R, t, s), good) in enumerate(truth):
        Re = out["sim_out"][b, :9].astype(np.float64).reshape(3, 3)
        E = Re @ R.T
        v = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]]) / 2
        rot.append(np.degrees(np.arctan2(np.linalg.norm(v), (np.trace(E) - 1) / 2)))
        scl.append(abs(float(out["sim_out"][b, 12]) / s - 1))
        inl = out["inlier"][b, :counts[b]].astype(bool)
        kept.append(inl[good].mean()), acc.append(inl[~good].mean())
    res.update({"pairs": B, "stride": S, "hypotheses": H, "mean_matches": round(float(counts.mean()), 1),
                "codes_ok": int((out["status"] & 255 == 0).sum()),
                "mean_valid_hypotheses": round(float((out["status"] >> 8).mean()), 1),
                "worst_rotation_deg": round(float(max(rot)), 4), "worst_scale_error": round(float(max(scl)), 5),
                "true_inliers_kept": round(float(np.mean(kept)), 4), "worst_pair_kept": round(float(np.min(kept)), 4),
                "outliers_accepted": round(float(np.mean(acc)), 4)})
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
        raise SystemExit("bench_sim3 needs a GPU (there is no CPU fallback)")
    from pislam_amd.capi import Context
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx = Context(device=0, stream=stream.cuda_stream)
    with torch.cuda.stream(stream):
        res = {"pnp_shape": shape(args, torch, ctx, stream, dev, args.matches, 100),
               "loop_shape": shape(args, torch, ctx, stream, dev, args.loop_matches, 20)}
    print(json.dumps({"tool": "bench_sim3", "iters": args.iters, "results": res}))


if __name__ == "__main__":
    main()
