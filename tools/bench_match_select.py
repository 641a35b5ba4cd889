"""Batched angle bins and on-device match selection on front-end pairs; prints one JSON line.

Setup: pairs + 1 synthetic VGA pyramids (synth.make_batch, the other tools' workload) through OrbFrontend; pyramid k's
descriptors are matched against pyramid k + 1's by the brute-force matcher.  Timed, each as the median device-event
time of single calls after a warm-up: pislam_orb_angles_batch over all pairs + 1 pyramids, and
pislam_match_select_batch over the pairs with ORB-SLAM's settings {50, 8 / 10, unique, 3 bins, 10 %} — with and without
the rotation check, and with everything off (compaction only).  brute_force_ms is the match the selection follows.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (tracing slows the host; keep it out of
these numbers)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--max-keypoints", type=int, default=4096, help="stride of every per-keypoint array")
    ap.add_argument("--iters", type=int, default=200, help="timed calls per entry point")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_match_select needs a GPU (there is no CPU fallback)")
    from pislam_amd import synth
    from pislam_amd.capi import Context
    from pislam_amd.frontend import OrbFrontend, matchHammingBatch, orbAnglesBatch, selectMatchesBatch
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx = Context(device=0, stream=stream.cuda_stream)
    P, S = args.pairs, args.max_keypoints
    levels = synth.level_table()
    res = {}
    with torch.cuda.stream(stream):
        fe = OrbFrontend(levels, vstep=640, rows=synth.pyramid_rows(levels), max_keypoints=S, ctx=ctx)
        pyr = torch.from_numpy(synth.make_batch(args.seed, P + 1)).to(dev)
        kp, desc, counts = fe.alloc_outputs(P + 1, dev)
        fe(pyr, kp, desc, counts)
        ang = torch.empty((P + 1, S), dtype=torch.uint8, device=dev)
        res["angles_ms"] = round(timed(lambda: orbAnglesBatch(pyr, kp, counts, ang, ctx=ctx), stream, torch, args.warmup,
                                       args.iters), 4)
        qd, qc, td, tc = desc[:P].contiguous(), counts[:P].contiguous(), desc[1:].contiguous(), counts[1:].contiguous()
        qa, ta = ang[:P].contiguous(), ang[1:].contiguous()
        mo = [torch.empty((P, S), dtype=torch.int32, device=dev) for _ in range(3)]
        res["brute_force_ms"] = round(timed(lambda: matchHammingBatch(qd, qc, td, tc, *mo, ctx=ctx), stream, torch,
                                            args.warmup, args.iters), 4)
        outs = dict(sel_q=torch.empty((P, S), dtype=torch.int32, device=dev), sel_t=torch.empty((P, S), dtype=torch.int32, device=dev),
                    nsel=torch.empty((P,), dtype=torch.int32, device=dev))
        for key, kw in (("select_orbslam_ms", dict(qangle=qa, tangle=ta)),
                        ("select_no_rotation_ms", dict()),
                        ("select_all_off_ms", dict(max_dist=256, ratio=None, unique=False))):
            res[key] = round(timed(lambda: selectMatchesBatch(*mo, qc, tc, t_stride=S, ctx=ctx, **kw, **outs), stream, torch,
                                   args.warmup, args.iters), 4)
            if key == "select_orbslam_ms":
                res["mean_selected"] = round(float(outs["nsel"].cpu().numpy().mean()), 1)
        n = np.minimum(counts.cpu().numpy().view(np.uint32), S)
    res.update({"pairs": P, "max_keypoints": S, "mean_keypoints": round(float(n.mean()), 1)})
    print(json.dumps({"tool": "bench_match_select", "iters": args.iters, "results": res}))


if __name__ == "__main__":
    main()
