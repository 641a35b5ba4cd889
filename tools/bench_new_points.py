"""New map points between two key frames: the epipolar matcher next to the word-guided matcher on the same inputs, and
the triangulation next to a device copy of its inputs; prints one JSON line.

Setup: `--pairs` (256) synthetic key-frame pairs with a VGA camera (fx = fy = 500, bf = 40), key frame 2 a random motion
of 0.05 .. 1 units away from key frame 1.  Each side has `--keypoints` (1000) keypoints in a stride of 1024: 70 % are the
two views of a common point at 1.5 .. 25 units (a pixel of noise in image 2, the level from the depth, a third of them
with a stereo observation, the train descriptor a copy of the query's with 12 flipped bits), the rest unrelated.  A
keypoint's group is its point's id modulo `--groups` (100: a vocabulary cut at depth 2), the same on both sides, so the
word-guided matcher sees about keypoints / groups candidates per query and the epipolar test thins them.  ORB-SLAM's
bounds: chi2 3.84, epipole_r2 100, eight levels of 1.2.  The triangulation runs on `--matches` (300) slots per pair: true
matches, gathered on the host once.
Reported:
  epipolar        matchEpipolarBatch
  bow             matchHammingBowBatch on the same descriptors, groups and counts
  triangulate     triangulateBatch with normal and drange
  copy            torch copies of every input array of triangulateBatch into buffers of the same size
Timing: after a warm-up the calls are timed in turn, `--iters` rounds, one device-event pair per call; the median and the
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

CAM = np.array([500.0, 500.0, 320.0, 240.0, 40.0], np.float32)
MONO = -(1 << 31)


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def project(pose, X):
    Xc = X @ pose[:9].reshape(3, 3).T + pose[9:]
    z = Xc[:, 2]
    u = CAM[0] * Xc[:, 0] / z + CAM[2]
    return np.stack([u, CAM[1] * Xc[:, 1] / z + CAM[3], u - CAM[4] / z], 1), z


def make_pair(rng, n, stride, ngroups, words):
    """Host arrays of one pair: poses, and per side descriptors, groups, observations, levels; `own` = the train index
    of each query's true match or -1."""
    R1 = rodrigues(rng.normal(size=3), rng.uniform(0, 0.2))
    t1 = rng.normal(0, 1, 3)
    R2 = rodrigues(rng.normal(size=3), rng.uniform(0, 0.08)) @ R1
    base = rng.normal(size=3)
    O2 = -R1.T @ t1 + base / np.linalg.norm(base) * rng.choice([0.05, 0.3, 1.0])
    pose1 = np.concatenate([R1.reshape(-1), t1])
    pose2 = np.concatenate([R2.reshape(-1), -R2 @ O2])
    z = rng.uniform(1.5, 25, n)
    Xc = np.stack([rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-0.45, 0.45, n) * z, z], 1)
    X = (Xc - t1) @ R1
    (o1, z1), (o2, z2) = project(pose1, X), project(pose2, X)
    o2[:, :2] += rng.normal(0, 1, (n, 2))
    common = rng.random(n) < 0.7
    stray = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n), np.zeros(n)], 1)
    o2 = np.where(common[:, None], o2, stray)
    level = lambda zz: np.clip(np.round(np.log(np.maximum(zz, 1e-3) / 2) / np.log(1.2)), 0, 7).astype(np.uint8)
    q8 = lambda o: np.clip(np.round(o * 256), -(1 << 30), 1 << 30).astype(np.int64)
    qobs, tobs = q8(o1), q8(o2)
    qobs[rng.random(n) < 0.67, 2] = MONO
    tobs[(rng.random(n) < 0.67) | ~common, 2] = MONO
    qd = rng.integers(0, 2 ** 32, (n, words), dtype=np.uint64).astype(np.uint32)
    td = qd.copy()
    for k in range(12):
        bit = rng.integers(0, 32 * words, n)
        td[np.arange(n), bit // 32] ^= (np.uint32(1) << (bit % 32).astype(np.uint32))
    td = np.where(common[:, None], td, rng.integers(0, 2 ** 32, (n, words), dtype=np.uint64).astype(np.uint32))
    qg = rng.integers(0, ngroups, n)
    tg = np.where(common, qg, rng.integers(0, ngroups, n))
    order = rng.permutation(n)
    pad = lambda a, dt: np.concatenate([a, np.zeros((stride - n,) + a.shape[1:], a.dtype)]).astype(dt)
    own = np.where(common, np.argsort(order), -1)
    return dict(pose1=pose1.astype(np.float32), pose2=pose2.astype(np.float32), qd=pad(qd, np.uint32), qg=pad(qg, np.uint32),
                qobs=pad(qobs, np.int32), ql=pad(level(z1), np.uint8), td=pad(td[order], np.uint32),
                tg=pad(tg[order], np.uint32), tobs=pad(tobs[order], np.int32), tl=pad(level(z2)[order], np.uint8), own=own)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--groups", type=int, default=100)
    ap.add_argument("--words", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200, help="timed rounds (every call once per round)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_new_points needs a GPU (there is no CPU fallback)")
    from pislam_amd.capi import Context
    from pislam_amd.frontend import (epipolarGeometry, mapPointLevelTables, matchEpipolarBatch, matchHammingBowBatch,
                                     reserveMatchBow, reserveMatchEpipolar, triangulateBatch)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx = Context(device=0, stream=stream.cuda_stream)
    rng = np.random.default_rng(args.seed)
    B, n, stride, M = args.pairs, args.keypoints, 1024, args.matches
    if not 1 <= n <= stride or not 1 <= M <= stride:
        raise SystemExit("--keypoints and --matches must be 1..1024")
    pairs = [make_pair(rng, n, stride, args.groups, args.words) for _ in range(B)]
    stack = lambda k: np.stack([p[k] for p in pairs])
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to(dev)
    ls, sg = mapPointLevelTables(8, 1.2)
    cam = np.tile(CAM, (B, 1))
    f12, ep = epipolarGeometry(stack("pose1"), stack("pose2"), cam, cam)
    # the triangulation's slots: the first M true matches of each pair
    o1, o2 = np.zeros((B, stride, 3), np.int32), np.zeros((B, stride, 3), np.int32)
    l1, l2 = np.full((B, stride), 255, np.uint8), np.full((B, stride), 255, np.uint8)
    nslot = np.zeros(B, np.int32)
    for b, p in enumerate(pairs):
        q = np.flatnonzero(p["own"] >= 0)[:M]
        t = p["own"][q]
        o1[b, :len(q)], o2[b, :len(q)], l1[b, :len(q)], l2[b, :len(q)] = p["qobs"][q], p["tobs"][t], p["ql"][q], p["tl"][t]
        nslot[b] = len(q)
    with torch.cuda.stream(stream):
        d = {k: T(stack(k)) for k in ("qd", "qg", "qobs", "ql", "td", "tg", "tobs", "tl", "pose1", "pose2")}
        d.update(F=T(f12), ep=T(ep), cam=T(cam), o1=T(o1), o2=T(o2), l1=T(l1), l2=T(l2), nslot=T(nslot))
        counts = torch.full((B,), n, dtype=torch.int32, device=dev)
        reserveMatchEpipolar(args.groups, stride, B, words=args.words, ctx=ctx)
        reserveMatchBow(args.groups, stride, B, words=args.words, ctx=ctx)
        out = [torch.empty((B, stride), dtype=torch.int32, device=dev) for _ in range(3)]
        out2 = [torch.empty((B, stride), dtype=torch.int32, device=dev) for _ in range(3)]
        tri = dict(xw=torch.empty((B, stride, 3), dtype=torch.float32, device=dev),
                   status=torch.empty((B, stride), dtype=torch.uint8, device=dev),
                   normal=torch.empty((B, stride, 3), dtype=torch.float32, device=dev),
                   drange=torch.empty((B, stride, 2), dtype=torch.float32, device=dev),
                   npoints=torch.empty((B,), dtype=torch.int32, device=dev))

        def epipolar():
            matchEpipolarBatch(d["qd"], d["qg"], d["qobs"], d["ql"], counts, d["td"], d["tg"], d["tobs"], d["tl"], counts,
                               args.groups, d["F"], d["ep"], level_sigma2=sg, level_scale=ls, idx=out[0], dist=out[1],
                               dist2=out[2], ctx=ctx)

        def bow():
            matchHammingBowBatch(d["qd"], d["qg"], counts, d["td"], d["tg"], counts, args.groups, *out2, ctx=ctx)

        def triangulate():
            triangulateBatch(d["pose1"], d["pose2"], d["cam"], d["cam"], d["o1"], d["o2"], d["l1"], d["l2"], d["nslot"],
                             level_scale=ls, level_sigma2=sg, ctx=ctx, **tri)

        ins = [d[k] for k in ("pose1", "pose2", "cam", "cam", "o1", "o2", "l1", "l2", "nslot")]
        dup = [torch.empty_like(t) for t in ins]

        def copy():
            for s, t in zip(ins, dup):
                t.copy_(s, non_blocking=True)

        calls = {"epipolar": epipolar, "bow": bow, "triangulate": triangulate, "copy": copy}
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
        epipolar()
        stream.synchronize()
    ms = {}
    for k in calls:
        t = np.array([a.elapsed_time(b) for a, b in ev[k]])
        ms[k] = {"median": round(float(np.median(t)), 4), "p10": round(float(np.percentile(t, 10)), 4),
                 "p90": round(float(np.percentile(t, 90)), 4)}
    idx, bidx = out[0].cpu().numpy()[:, :n], out2[0].cpu().numpy()[:, :n]
    own = np.stack([p["own"] for p in pairs])
    status = tri["status"].cpu().numpy()
    live = np.arange(stride)[None, :] < nslot[:, None]
    print(json.dumps({
        "tool": "bench_new_points", "pairs": B, "keypoints": n, "groups": args.groups, "words": args.words, "iters": args.iters,
        "slots_per_pair": round(float(nslot.mean()), 1), "ms": ms,
        "epipolar_over_bow": round(ms["epipolar"]["median"] / ms["bow"]["median"], 3),
        "triangulate_over_copy": round(ms["triangulate"]["median"] / ms["copy"]["median"], 3),
        "epipolar_matched_share": round(float((idx >= 0).mean()), 4), "bow_matched_share": round(float((bidx >= 0).mean()), 4),
        "epipolar_true_share": round(float(((idx == own) & (own >= 0)).sum() / max(1, (own >= 0).sum())), 4),
        "bow_true_share": round(float(((bidx == own) & (own >= 0)).sum() / max(1, (own >= 0).sum())), 4),
        "points_share": round(float((status[live] == 0).mean()), 4),
        "triangulate_input_bytes": int(sum(t.numel() * t.element_size() for t in ins))}))


if __name__ == "__main__":
    main()
