"""Batched covisibility graph (pislam_covisibility_batch) on synthetic maps, next to a device copy of its input bytes and
to the host round trip it replaces; prints one JSON line.

Two shapes.  `local`: `maps` local maps of `kfs` key frames, `points` points and `obs` observations (each point seen by
obs / points random key frames of the map): the window of tools/bench_local_ba.py, so the time stands next to
pislam_local_ba_batch's.  `whole`: ONE map of `big_kfs` key frames and about `big_obs` observations, each point seen by a
random subset of a run of consecutive key frames: the large graph of tools/bench_pose_graph.py.  Observations carry random
pyramid levels; ORB-SLAM's parameters (15, 3, 1); `nb_stride` neighbours kept per key frame.

Timed, each as the median device-event time of single calls after a warm-up (the workspace is reserved first): the call,
and a device-to-device copy of its input bytes.  `round_trip_ms` is what a caller without the call does between two
launches, as a median wall time: copy the observations to the host, compute the same seven outputs with numpy
(`host_numpy` below, checked against the call's outputs word for word before anything is timed), copy them back."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_sim3 import timed  # noqa: E402

NAMES = ("nb_idx", "nb_weight", "nb_count", "parent", "kf_points", "kf_redundant", "status")


def local_maps(rng, maps, kfs, points, obs):
    per = max(obs // points, 1)
    kf = np.sort(np.argsort(rng.random((maps, points, kfs)), axis=2)[:, :, :per], axis=2)       # `per` distinct key frames a point
    pt = np.broadcast_to(np.arange(points)[None, :, None], kf.shape)
    n = points * per
    return kf.reshape(maps, n).astype(np.int16), pt.reshape(maps, n).astype(np.int32), np.full(maps, n, np.int32)


def whole_map(rng, kfs, obs, window=30, per=10):
    points = obs // per
    first = rng.integers(0, kfs - window, points)
    kf = first[:, None] + np.sort(np.argsort(rng.random((points, window)), axis=1)[:, :per], axis=1)
    pt = np.broadcast_to(np.arange(points)[:, None], kf.shape)
    n = points * per
    return kf.reshape(1, n).astype(np.int16), pt.reshape(1, n).astype(np.int32), np.full(1, n, np.int32)


def host_numpy(kf, pt, level, n, nk, prm, nbs):
    """The call's outputs for one valid map of n sorted observations, with numpy: the contract of include/pislam_hip.h."""
    min_weight, min_observers, slack = prm
    kf, pt, level = kf[:n].astype(np.int64), pt[:n].astype(np.int64), level[:n].astype(np.int64)
    W = np.zeros(nk * nk, np.int64)
    others = np.zeros(n, np.int64)
    d = 1
    while True:                                              # the observation d places on belongs to the same point
        same = pt[d:] == pt[:-d] if d < n else np.zeros(0, bool)
        if not same.any():
            break
        a, b = kf[:-d][same], kf[d:][same]
        W += np.bincount(a * nk + b, minlength=nk * nk) + np.bincount(b * nk + a, minlength=nk * nk)
        la, lb = level[:-d][same], level[d:][same]
        np.add.at(others, np.nonzero(same)[0], (lb <= la + slack).astype(np.int64))
        np.add.at(others, np.nonzero(same)[0] + d, (la <= lb + slack).astype(np.int64))
        d += 1
    W = W.reshape(nk, nk)
    j = np.arange(nk)
    order = np.argsort(-W * 65536 + j[None, :], axis=1, kind="stable")
    sw = np.take_along_axis(W, order, 1)
    count = (sw >= min_weight).sum(1)
    fallback = (count == 0) & (sw[:, 0] > 0)
    count = count + fallback
    m = min(nbs, nk)
    live = j[None, :m] < count[:, None]
    nb_idx, nb_weight = np.where(live, order[:, :m], -1), np.where(live, sw[:, :m], -1)
    early = np.where(j[None, :] < j[:, None], W, 0)
    parent = np.where(early.max(1) > 0, early.argmax(1), 0xFFFF)
    return dict(nb_idx=nb_idx, nb_weight=nb_weight, nb_count=count, parent=parent, kf_points=np.bincount(kf, minlength=nk),
                kf_redundant=np.bincount(kf[others >= min_observers], minlength=nk), status=0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--maps", type=int, default=256)
    ap.add_argument("--kfs", type=int, default=32)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--obs", type=int, default=5000)
    ap.add_argument("--big-kfs", type=int, default=2048)
    ap.add_argument("--big-obs", type=int, default=1000000)
    ap.add_argument("--nb-stride", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20, help="timed calls per entry")
    ap.add_argument("--host-iters", type=int, default=3, help="timed host round trips per shape")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_covisibility needs a GPU (there is no CPU fallback)")
    from pislam_amd.capi import Context
    from pislam_amd.frontend import covisibilityBatch, reserveCovisibility
    rng = np.random.default_rng(args.seed)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx = Context(device=0, stream=stream.cuda_stream)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    prm = (15, 3, 1)
    res = {}
    with torch.cuda.stream(stream):
        for tag, nk, (kf, pt, counts) in (("local", args.kfs, local_maps(rng, args.maps, args.kfs, args.points, args.obs)),
                                          ("whole", args.big_kfs, whole_map(rng, args.big_kfs, args.big_obs))):
            B, S = kf.shape
            nbs = min(args.nb_stride, nk)
            level = rng.integers(0, 8, (B, S)).astype(np.uint8)
            ins = [T(kf), T(pt), T(counts), T(np.full(B, nk, np.int32))]
            d_level = T(level)
            kw = dict(obs_level=d_level, kf_stride=nk, nb_stride=nbs, min_weight=prm[0], cull_min_observers=prm[1],
                      cull_level_slack=prm[2], ctx=ctx)
            reserveCovisibility(nk, S, B, ctx=ctx)
            keep = dict(zip(NAMES, covisibilityBatch(*ins, **kw)))
            for k in ("nb_idx", "nb_weight"):
                keep[k].fill_(-1)                            # (what host_numpy puts behind a row's count)
            ms = timed(lambda: covisibilityBatch(*ins, **kw, **keep), stream, torch, args.warmup, args.iters)
            src = ins + [d_level]
            dst = [torch.empty_like(a) for a in src]

            def copy():
                for d, s in zip(dst, src):
                    d.copy_(s)
            copy_ms = timed(copy, stream, torch, args.warmup, args.iters)
            stream.synchronize()
            got = {k: v.cpu().numpy().astype(np.int64) for k, v in keep.items()}

            def round_trip(check=False):
                h_kf, h_pt, h_n, h_level = (a.cpu().numpy() for a in (ins[0], ins[1], ins[2], d_level))
                maps = [host_numpy(h_kf[b], h_pt[b], h_level[b], int(h_n[b]), nk, prm, nbs) for b in range(B)]
                host = {k: np.stack([np.asarray(m[k]) for m in maps]) for k in NAMES}
                back = [T(host[k].astype(np.int16 if k in ("nb_idx", "parent") else np.int32)) for k in NAMES]
                stream.synchronize()
                if check:
                    for k in NAMES:
                        want = host[k] & 0xFFFF if k == "parent" else host[k]
                        have = got[k] & 0xFFFF if k == "parent" else got[k]
                        assert (have == want).all(), f"{tag}: {k} differs from the numpy restatement"
                return back
            round_trip(check=True)
            trips = []
            for _ in range(args.host_iters):
                t0 = time.perf_counter()
                round_trip()
                trips.append(1e3 * (time.perf_counter() - t0))
            res[tag] = {"maps": B, "key_frames": nk, "observations": int(counts.sum()), "nb_stride": nbs,
                        "covisibility_ms": round(ms, 4), "copy_inputs_ms": round(copy_ms, 4),
                        "input_bytes": int(sum(a.numel() * a.element_size() for a in src)),
                        "workspace_bytes": 4 * B * (nk * nk + 2 * nk + 1), "round_trip_ms": round(float(np.median(trips)), 2),
                        "mean_neighbours": round(float(got["nb_count"].mean()), 2), "max_weight": int(got["nb_weight"].max()),
                        "redundant_key_frames": int((got["kf_redundant"] > 0.9 * got["kf_points"]).sum())}
        stream.synchronize()
    print(json.dumps({"tool": "bench_covisibility", "iters": args.iters, "params": dict(zip(("min_weight", "cull_min_observers",
                                                                                             "cull_level_slack"), prm)), "results": res}))


if __name__ == "__main__":
    main()
