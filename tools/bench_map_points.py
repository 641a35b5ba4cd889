"""Batched map-point update (pislam_map_points_update_batch) on synthetic maps, next to a device copy of its input bytes,
to the host round trip it replaces and, for the local maps, to pislam_covisibility_batch on the same lists; prints one
JSON line.

Two shapes, those of tools/bench_covisibility.py.  `local`: `maps` local maps of `kfs` key frames, `points` points and
`obs` observations (each point seen by obs / points random key frames of the map).  `whole`: ONE map of `big_kfs` key
frames and about `big_obs` observations, each point seen by 10 of a run of 30 consecutive key frames.  Observations carry
random pyramid levels and descriptors (a centre per point, up to 40 bits flipped per observer); the poses look at the
points from a few units away; every point has a reference key frame among its observers.

Timed, each as the median device-event time of single calls after a warm-up: the call with every output, the call
without descriptors (geometry and counts only), a device-to-device copy of the input bytes and, for `local`, the
covisibility call (workspace reserved first).  `round_trip_ms` is what a caller without the call does between two
launches, as a median wall time: copy the observations, descriptors, poses and points to the host, compute the same
outputs with numpy (`host_numpy` below: the contract of include/pislam_hip.h for tracks of one length, binary32 one
operation at a time, checked against the call's outputs word for word before anything is timed), copy them back."""
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

from bench_covisibility import local_maps, whole_map  # noqa: E402
from bench_sim3 import timed  # noqa: E402

NAMES = ("normal", "drange", "desc", "nobs", "first", "pt_status", "status")
POP8 = np.array([bin(v).count("1") for v in range(256)], np.uint16)
F32 = np.float32


def scene(rng, kf, pt, nk, points):
    """Levels, descriptors, poses, points and reference key frames for the lists of local_maps / whole_map."""
    B, S = kf.shape
    level = rng.integers(0, 8, (B, S)).astype(np.uint8)
    centre = rng.integers(0, 1 << 32, (B, points, 8), dtype=np.uint64).astype(np.uint32)
    word = lambda: rng.integers(0, 1 << 32, (B, S, 8), dtype=np.uint64).astype(np.uint32)
    noise = np.where(rng.random((B, S, 1)) < 0.3, np.uint32(0), word() & word() & word())   # about 32 bits, or none
    desc = np.take_along_axis(centre, pt.astype(np.int64)[:, :, None], 1) ^ noise
    poses = np.zeros((B, nk, 12), F32)
    poses[:, :, [0, 4, 8]] = 1.0
    poses[:, :, 9:] = rng.normal(0, 1, (B, nk, 3))
    xw = (rng.normal(0, 1, (B, points, 3)) + [0, 0, 6]).astype(F32)
    per = S // points
    ref = kf.reshape(B, points, per)[:, :, per // 2].astype(np.int16)
    return level, desc, poses, xw, np.ascontiguousarray(ref)


def host_numpy(kf, level, desc, poses, xw, ref, ls, per, chunk=4096):
    """The call's outputs for one valid map whose every point has `per` observers, in list order, with numpy."""
    points = len(xw)
    k = kf.astype(np.int64).reshape(points, per)
    with np.errstate(all="ignore"):
        P = poses[k]                                                           # [points][per][12]
        O = np.stack([-((P[..., j] * P[..., 9] + P[..., 3 + j] * P[..., 10]) + P[..., 6 + j] * P[..., 11]) for j in range(3)], 2)
        e = xw[:, None, :] - O
        d = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
        u = e / d[..., None]
        w = u[:, 0].copy()
        for i in range(1, per):
            w = w + u[:, i]
        wn = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        normal = w / wn[:, None]
        hit = k == (ref.astype(np.int64) & 0xFFFF)[:, None]
        r = np.where(hit.any(1), hit.argmax(1), 0)
        lr = np.take_along_axis(level.reshape(points, per).astype(np.int64), r[:, None], 1)[:, 0]
        rr = np.take_along_axis(d, r[:, None], 1)[:, 0] * ls[np.minimum(lr, len(ls) - 1)]
        drange = np.stack([rr / ls[-1], rr], 1)
    status = np.where(hit.any(1), 0, 2)
    assert normal.dtype == drange.dtype == F32 and np.isfinite(normal).all() and np.isfinite(drange).all() and (lr < len(ls)).all()
    by = desc.view(np.uint8).reshape(points, per, 32)
    pick = np.empty(points, np.int64)
    for p0 in range(0, points, chunk):
        c = by[p0:p0 + chunk]
        D = POP8[c[:, :, None, :] ^ c[:, None, :, :]].sum(3, dtype=np.uint16)
        pick[p0:p0 + chunk] = np.sort(D, axis=2)[:, :, (per - 1) // 2].argmin(1)
    chosen = desc.reshape(points, per, 8)[np.arange(points), pick]
    return dict(normal=normal, drange=drange, desc=chosen, nobs=np.full(points, per, np.int32),
                first=np.arange(points, dtype=np.int32) * per, pt_status=status.astype(np.uint8), status=0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--maps", type=int, default=256)
    ap.add_argument("--kfs", type=int, default=32)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--obs", type=int, default=5000)
    ap.add_argument("--big-kfs", type=int, default=2048)
    ap.add_argument("--big-obs", type=int, default=1000000)
    ap.add_argument("--iters", type=int, default=20, help="timed calls per entry")
    ap.add_argument("--host-iters", type=int, default=3, help="timed host round trips per shape")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_map_points needs a GPU (there is no CPU fallback)")
    from pislam_amd.capi import Context
    from pislam_amd.frontend import covisibilityBatch, mapPointLevelTables, mapPointsUpdateBatch, reserveCovisibility
    rng = np.random.default_rng(args.seed)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx = Context(device=0, stream=stream.cuda_stream)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ls = mapPointLevelTables(8, 1.2)[0]
    res = {}
    with torch.cuda.stream(stream):
        for tag, nk, (kf, pt, counts) in (("local", args.kfs, local_maps(rng, args.maps, args.kfs, args.points, args.obs)),
                                          ("whole", args.big_kfs, whole_map(rng, args.big_kfs, args.big_obs))):
            B, S = kf.shape
            points = int(pt.max()) + 1
            per = S // points
            level, desc, poses, xw, ref = scene(rng, kf, pt, nk, points)
            ins = [T(kf), T(pt), T(counts), T(np.full(B, nk, np.int32)), T(level), T(poses), T(xw), T(np.full(B, points, np.int32))]
            d_desc, d_ref = T(desc.view(np.int32)), T(ref)
            kw = dict(ref=d_ref, level_scale=ls, ctx=ctx)
            keep = dict(zip(NAMES, mapPointsUpdateBatch(*ins, obs_desc=d_desc, **kw)))
            ms = timed(lambda: mapPointsUpdateBatch(*ins, obs_desc=d_desc, **kw, **keep), stream, torch, args.warmup, args.iters)
            plain = {k: v for k, v in keep.items() if k != "desc"}
            geo_ms = timed(lambda: mapPointsUpdateBatch(*ins, **kw, **plain), stream, torch, args.warmup, args.iters)
            src = ins + [d_desc, d_ref]
            dst = [torch.empty_like(a) for a in src]

            def copy():
                for d, s in zip(dst, src):
                    d.copy_(s)
            copy_ms = timed(copy, stream, torch, args.warmup, args.iters)
            entry = {}
            if tag == "local":
                reserveCovisibility(nk, S, B, ctx=ctx)
                ckw = dict(obs_level=ins[4], kf_stride=nk, nb_stride=nk, ctx=ctx)
                cv = covisibilityBatch(*ins[:4], **ckw)
                names = ("nb_idx", "nb_weight", "nb_count", "parent", "kf_points", "kf_redundant", "status")
                entry["covisibility_ms"] = round(timed(lambda: covisibilityBatch(*ins[:4], **ckw, **dict(zip(names, cv))), stream,
                                                       torch, args.warmup, args.iters), 4)
            stream.synchronize()
            got = {k: v.cpu().numpy() for k, v in keep.items()}

            def round_trip(check=False):
                h_kf, h_level, h_desc, h_poses, h_xw, h_ref = (a.cpu().numpy() for a in (ins[0], ins[4], d_desc, ins[5], ins[6], d_ref))
                maps = [host_numpy(h_kf[b], h_level[b], h_desc[b], h_poses[b], h_xw[b], h_ref[b], ls, per) for b in range(B)]
                host = {k: np.stack([np.asarray(m[k]) for m in maps]) for k in NAMES}
                back = [T(host[k]) for k in NAMES]
                stream.synchronize()
                if check:
                    for k in NAMES:
                        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(host[k].astype(got[k].dtype))
                        assert a.tobytes() == b.tobytes(), f"{tag}: {k} differs from the numpy restatement"
                return back
            round_trip(check=True)
            trips = []
            for _ in range(args.host_iters):
                t0 = time.perf_counter()
                round_trip()
                trips.append(1e3 * (time.perf_counter() - t0))
            entry.update({"maps": B, "key_frames": nk, "points": B * points, "observations": int(counts.sum()), "track": per,
                          "update_ms": round(ms, 4), "update_without_descriptors_ms": round(geo_ms, 4),
                          "copy_inputs_ms": round(copy_ms, 4),
                          "input_bytes": int(sum(a.numel() * a.element_size() for a in src)),
                          "round_trip_ms": round(float(np.median(trips)), 2),
                          "hamming_pairs": int(B * points * per * per),
                          "first_observer_chosen": round(float((got["desc"].view(np.uint32) == desc.reshape(B, points, per, 8)[:, :, 0])
                                                               .all(2).mean()), 3)})
            res[tag] = entry
        stream.synchronize()
    print(json.dumps({"tool": "bench_map_points", "iters": args.iters, "results": res}))


if __name__ == "__main__":
    main()
