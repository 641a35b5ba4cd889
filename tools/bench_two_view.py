"""Batched two-view RANSAC (F and H) on synthetic matched pairs, next to the match selection on the same pairs; prints
one JSON line.

Setup: `pairs` camera pairs (640 x 480, focal length 500, a small rotation plus a translation, half of the pairs looking
at a plane), each with about `matches` true matches at integer level-0 pixels, 20 % of them with a random partner, plus
100 proposals the selection has to reject (distance above the threshold).  The matcher's outputs (idx, dist, dist2,
angles) are synthesised so that pislam_match_select_batch with ORB-SLAM's settings selects exactly the matches;
matchedPointsQ8 turns its lists into the point lists, and pislam_two_view_ransac_batch runs on those with `hypotheses`
hypotheses per pair, once per model.  Timed, each as the median device-event time of single calls after a warm-up:
the selection, the torch plumbing of matchedPointsQ8, and the two-view call for F and for H."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H, FOCAL = 640, 480, 500.0


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


def scene(rng, n, plane, outliers=0.2):
    """n matches as integer pixels of both images ([n][2] each, inside the frame) and the mask of the true ones."""
    K = np.array([[FOCAL, 0, W / 2], [0, FOCAL, H / 2], [0, 0, 1]])
    u = np.stack([rng.uniform(40, W - 40, n), rng.uniform(40, H - 40, n)], 1)
    rays = np.linalg.inv(K) @ np.vstack([u.T, np.ones(n)])
    z = 8.0 / (np.array([0.15, -0.1, 1.0]) @ rays) if plane else rng.uniform(4, 12, n)
    a = rng.normal(0, 0.02, 3)
    Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
    Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
    Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
    Q = K @ ((Rz @ Ry @ Rx) @ (rays * z) + rng.normal(0, 0.3, (3, 1)))
    v = (Q[:2] / Q[2]).T + rng.normal(0, 0.5, (n, 2))
    bad = rng.permutation(n)[:int(round(outliers * n))]
    v[bad] = np.stack([rng.uniform(0, W, len(bad)), rng.uniform(0, H, len(bad))], 1)
    good = np.ones(n, bool)
    good[bad] = False
    clip = lambda p: np.stack([np.clip(np.rint(p[:, 0]), 0, W - 1), np.clip(np.rint(p[:, 1]), 0, H - 1)], 1).astype(np.int64)
    return clip(u), clip(v), good


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
        raise SystemExit("bench_two_view needs a GPU (there is no CPU fallback)")
    from pislam_amd.capi import Context
    from pislam_amd.frontend import matchedPointsQ8, selectMatchesBatch, twoViewModelRatio, twoViewRansacBatch
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx = Context(device=0, stream=stream.cuda_stream)
    P, EXTRA = args.pairs, 100
    S = args.matches + 100 + EXTRA
    rng = np.random.default_rng(args.seed)
    levels = [(W, H, 0, 0)]
    qkp, tkp = np.zeros((P, S), np.int64), np.zeros((P, S), np.int64)
    idx, dist, dist2 = np.full((P, S), -1, np.int32), np.full((P, S), 256, np.int32), np.full((P, S), 256, np.int32)
    qang, tang = rng.integers(0, 30, (P, S)).astype(np.uint8), np.zeros((P, S), np.uint8)
    counts, truth = np.zeros(P, np.int32), []
    for b in range(P):
        n = int(rng.integers(args.matches - 100, args.matches + 101))
        u, v, good = scene(rng, n + EXTRA, b % 2 == 1)
        perm = rng.permutation(S)[:n + EXTRA]
        qkp[b, :n + EXTRA] = (u[:, 0] << 12) | u[:, 1]
        tkp[b, perm] = (v[:, 0] << 12) | v[:, 1]
        idx[b, :n + EXTRA], dist[b, :n], dist[b, n:n + EXTRA], dist2[b, :n + EXTRA] = perm, 20, 90, 60
        tang[b, perm] = qang[b, :n + EXTRA]
        counts[b] = n + EXTRA
        truth.append(good[:n])
    res = {}
    with torch.cuda.stream(stream):
        T = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if dt is None else torch.from_numpy(
            np.ascontiguousarray(a)).to(dev).to(dt)
        qkp_d, tkp_d = T(qkp, torch.int32), T(tkp, torch.int32)
        mo = (T(idx), T(dist), T(dist2))
        qc, tc = T(counts), torch.full((P,), S, dtype=torch.int32, device=dev)
        qa, ta = T(qang), T(tang)
        sel = dict(sel_q=torch.empty((P, S), dtype=torch.int32, device=dev), sel_t=torch.empty((P, S), dtype=torch.int32, device=dev),
                   nsel=torch.empty((P,), dtype=torch.int32, device=dev))
        run_sel = lambda: selectMatchesBatch(*mo, qc, tc, qangle=qa, tangle=ta, ctx=ctx, **sel)
        res["select_orbslam_ms"] = round(timed(run_sel, stream, torch, args.warmup, args.iters), 4)
        s3 = (sel["sel_q"], sel["sel_t"], sel["nsel"])
        res["matched_points_torch_ms"] = round(timed(lambda: matchedPointsQ8(qkp_d, tkp_d, s3, levels), stream, torch, 3, 10), 4)
        p1, p2, n = matchedPointsQ8(qkp_d, tkp_d, s3, levels)
        out = {}
        for name in ("F", "H"):
            o = twoViewRansacBatch(p1, p2, n, model=name, hypotheses=args.hypotheses, seed=args.seed, ctx=ctx)
            keep = dict(zip(("best", "score", "ninliers", "inlier", "model_n", "stats"), o))
            res["two_view_%s_ms" % name] = round(timed(lambda: twoViewRansacBatch(p1, p2, n, model=name, hypotheses=args.hypotheses,
                                                                                 seed=args.seed, ctx=ctx, **keep), stream, torch,
                                                       args.warmup, args.iters), 4)
            out[name] = {k: v.cpu().numpy() for k, v in keep.items()}
        nn = n.cpu().numpy()
    want = np.array([len(t) for t in truth])
    if not (nn == want).all():
        raise SystemExit("the selection did not select exactly the synthesised matches")
    tp = {m: np.mean([out[m]["inlier"][b, :nn[b]][truth[b]].mean() for b in range(P) if (m == "F") or b % 2 == 1]) for m in "FH"}
    fp = {m: np.mean([out[m]["inlier"][b, :nn[b]][~truth[b]].mean() for b in range(P) if (m == "F") or b % 2 == 1]) for m in "FH"}
    ratio = twoViewModelRatio(out["H"]["score"].view(np.uint32), out["F"]["score"].view(np.uint32))
    res.update({"pairs": P, "stride": S, "mean_matches": round(float(nn.mean()), 1), "hypotheses": args.hypotheses,
                "models_found_F": int((out["F"]["best"] >= 0).sum()), "models_found_H": int((out["H"]["best"] >= 0).sum()),
                "true_inliers_marked_F": round(float(tp["F"]), 4), "outliers_marked_F": round(float(fp["F"]), 4),
                "true_inliers_marked_H_planes": round(float(tp["H"]), 4), "outliers_marked_H_planes": round(float(fp["H"]), 4),
                "mean_ratio_planes": round(float(ratio[1::2].mean()), 3), "mean_ratio_general": round(float(ratio[0::2].mean()), 3)})
    print(json.dumps({"tool": "bench_two_view", "iters": args.iters, "results": res}))


if __name__ == "__main__":
    main()
