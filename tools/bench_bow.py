"""Bag-of-words transform, vector and word-guided matcher on front-end pairs; prints one JSON line.

Setup per layout: pairs + 1 synthetic pyramids (synth.make_batch) through OrbFrontend; pyramid k's descriptors are
matched against pyramid k + 1's.  Two vocabularies: "fit", a complete 10-ary tree of depth 3 grown here by hierarchical
k-majority over the run's own descriptors (1 111 nodes: stays in L2), and "large", 10-ary depth 6 with random
descriptors (1 111 111 nodes, 36 MB: beyond L2, inside the Infinity Cache).  Timing: after a warm-up, the median
device-event time of single calls.  descents_per_s counts descriptors; implied_gather_tbs of the large vocabulary is
descents x 6 levels x 10 children x 32 B / time.  The matcher runs on the "fit" groups at group_depth 2 (100 groups)
and 3 (1000 groups), beside matchHammingBatch on the same pairs; mean_candidates_per_query is a host count on a sample
of pairs.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (tracing slows the host; keep
it out of these numbers)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LAYOUTS = {
    # name: (w0, h0, vstep, packed levels, shapes per frame (None = synth default), max_keypoints, default pairs)
    "vga": (640, 480, 640, False, None, 2048, 256),
    "1280x960": (1280, 960, 1280, True, 148, 4096, 128),
}
K, FIT_DEPTH, LARGE_DEPTH = 10, 3, 6


def hamming(a, b):
    ab = np.unpackbits(np.ascontiguousarray(a).view(np.uint8), axis=1).astype(np.float32)
    bb = np.unpackbits(np.ascontiguousarray(b).view(np.uint8), axis=1).astype(np.float32)
    return ab.sum(1)[:, None] + bb.sum(1)[None, :] - 2 * (ab @ bb.T)


def kmajority_nodes(rng, desc, k, depth):
    """Node descriptors of a complete k-ary tree (breadth-first order) by hierarchical k-majority over desc [n][words]."""
    nn = sum(k ** d for d in range(depth + 1))
    inner = sum(k ** d for d in range(depth))
    nodes = rng.integers(0, 2**32, (nn, desc.shape[1]), dtype=np.uint64).astype(np.uint32)
    bits = np.unpackbits(np.ascontiguousarray(desc).view(np.uint8), axis=1)
    members = {0: np.arange(len(desc))}
    for n in range(inner):
        S = members.pop(n, np.zeros(0, np.int64))
        if len(S) == 0:
            continue
        centres = desc[rng.choice(S, k, replace=len(S) < k)].copy()
        for it in range(4):
            a = hamming(desc[S], centres).argmin(1)
            if it == 3:
                break
            for c in range(k):
                m = S[a == c]
                if len(m):
                    centres[c] = np.packbits((bits[m].sum(0) * 2 > len(m)).astype(np.uint8)).view(np.uint32)
        nodes[n * k + 1:n * k + 1 + k] = centres
        for c in range(k):
            members[n * k + 1 + c] = S[a == c]
    return nodes


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


def run_layout(name, args, torch, ctx, stream):
    from pislam_amd import synth
    from pislam_amd.frontend import (OrbFrontend, Vocabulary, bowTransformBatch, bowVectorBatch, matchHammingBatch,
                                     matchHammingBowBatch, reserveMatchBow)
    w0, h0, vstep, packed, nshapes, max_kp, pairs = LAYOUTS[name]
    P = args.pairs or pairs
    levels = synth.packed_level_table(w0, h0) if packed else synth.level_table(w0, h0)
    rows = synth.pyramid_rows(levels)
    pyr = synth.make_batch(args.seed, P + 1, w0=w0, h0=h0, vstep=vstep, levels=levels, nshapes=nshapes)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(args.seed)
    res = {}
    with torch.cuda.stream(stream):
        fe = OrbFrontend(levels, vstep=vstep, rows=rows, max_keypoints=max_kp, ctx=ctx)
        kp, desc, counts = fe.alloc_outputs(P + 1, dev)
        fe(torch.from_numpy(pyr).to(dev), kp, desc, counts)
        stream.synchronize()
        hd, hc = desc.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32)
        n = np.minimum(hc, max_kp).astype(np.int64)
        words = hd.shape[2]
        sample = np.concatenate([hd[b, :n[b]] for b in range(0, P + 1, max(1, (P + 1) // 16))])
        fit_nodes = kmajority_nodes(rng, sample, K, FIT_DEPTH)
        large_nodes = rng.integers(0, 2**32, (sum(K ** d for d in range(LARGE_DEPTH + 1)), words), dtype=np.uint64).astype(np.uint32)
        descents = int(n.sum())
        outs = [torch.empty((P + 1, max_kp), dtype=torch.int32, device=dev) for _ in range(3)]
        groups = {}
        for key, nodes, depth, gds in (("fit", fit_nodes, FIT_DEPTH, (2, 3)), ("large", large_nodes, LARGE_DEPTH, (2,))):
            for gd in gds:
                v = Vocabulary.from_kary(nodes, K, depth, gd, ctx=ctx)
                ms = timed(lambda: bowTransformBatch(v, desc, counts, *outs, ctx=ctx), stream, torch, args.warmup, args.iters)
                if key == "fit":
                    groups[gd] = (outs[1].clone(), v.ngroups)
                if gd == 2:
                    r = {"ms": round(ms, 4), "descents": descents, "descents_per_s": round(descents / (ms * 1e-3), 0),
                         "nodes": int(len(nodes)), "table_mb": round(nodes.nbytes / 1e6, 1)}
                    if key == "large":
                        r["implied_gather_tbs"] = round(descents * depth * K * words * 4 / (ms * 1e-3) / 1e12, 3)
                    res["transform_" + key] = r
                if key == "fit" and gd == 2:
                    bow = [torch.empty((P + 1, max_kp), dtype=torch.int32, device=dev) for _ in range(2)]
                    bn = torch.empty((P + 1,), dtype=torch.int32, device=dev)
                    word = outs[0].clone()
                    res["vector_ms"] = round(timed(lambda: bowVectorBatch(word, counts, *bow, bn, ctx=ctx), stream, torch,
                                                   args.warmup, args.iters), 4)
                    res["mean_distinct_words"] = round(float(bn.cpu().numpy().mean()), 1)
                stream.synchronize()
                v.close()
        qd, qc, td, tc = desc[:P].contiguous(), counts[:P].contiguous(), desc[1:].contiguous(), counts[1:].contiguous()
        mo = [torch.empty((P, max_kp), dtype=torch.int32, device=dev) for _ in range(3)]
        res["brute_force_ms"] = round(timed(lambda: matchHammingBatch(qd, qc, td, tc, *mo, ctx=ctx), stream, torch,
                                            args.warmup, args.iters), 4)
        for gd, (g, ngroups) in groups.items():
            qg, tg = g[:P].contiguous(), g[1:].contiguous()
            reserveMatchBow(ngroups, max_kp, P, words=words, ctx=ctx)
            ms = timed(lambda: matchHammingBowBatch(qd, qg, qc, td, tg, tc, ngroups, *mo, ctx=ctx), stream, torch,
                       args.warmup, args.iters)
            hg = g.cpu().numpy()
            cand = [float((hg[k, :n[k], None] == hg[k + 1, None, :n[k + 1]]).sum(1).mean()) for k in
                    range(0, P, max(1, P // args.sample)) if n[k]]
            res[f"match_bow_group_depth_{gd}"] = {"ms": round(ms, 4), "ngroups": ngroups,
                                                  "speedup_over_brute_force": round(res["brute_force_ms"] / ms, 3),
                                                  "mean_candidates_per_query": round(float(np.mean(cand)), 2)}
    res.update({"pairs": P, "max_keypoints": max_kp, "words": int(words), "mean_keypoints": round(float(n.mean()), 1)})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--layouts", default="vga,1280x960", help="comma-separated: " + ", ".join(LAYOUTS))
    ap.add_argument("--pairs", type=int, default=0, help="pairs per layout (0: 256 VGA, 128 at 1280x960)")
    ap.add_argument("--iters", type=int, default=200, help="timed calls per entry point")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sample", type=int, default=16, help="pairs of the host candidate count")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bow needs a GPU (there is no CPU fallback)")
    from pislam_amd.capi import Context
    stream = torch.cuda.Stream(torch.device("cuda:0"))
    ctx = Context(device=0, stream=stream.cuda_stream)
    res = {name: run_layout(name, args, torch, ctx, stream) for name in args.layouts.split(",")}
    print(json.dumps({"tool": "bench_bow", "iters": args.iters, "results": res}))


if __name__ == "__main__":
    main()
