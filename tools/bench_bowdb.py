"""Key-frame database: integer weights, add (with the index rebuild) and query on front-end outputs; prints one JSON line.

Setup: queries + 1 synthetic VGA pyramids (synth.make_batch) through OrbFrontend, then transform -> vector -> weight on
two vocabularies: "fit", a complete 10-ary tree of depth 3 grown by hierarchical k-majority over the run's own
descriptors (1000 words), and "large", 10-ary depth 6 with random descriptors (1 000 000 words).  The database is filled
with the vectors of these frames, cycled until it holds 1 000, 10 000 and 100 000 key frames, in adds of `queries`
frames; add_ms is the last such add (the index rebuild over the whole database included).  Timing: after a warm-up, the
median device-event time of single calls.  postings_per_query is the mean length sum of the posting lists a query
walks, postings_per_s = queries x that / query time.  Baseline: what a user with torch alone would write on the device:
the database's sparse CSR weight matrix [key frames][words] times the dense query matrix [words][queries]
(torch.sparse.mm; an index_add_ over the gathered postings if this torch build refuses that).  It computes products,
not minima, and selects nothing: a cost baseline only.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats` (tracing only, the program after `--`)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_bow import K, FIT_DEPTH, LARGE_DEPTH, kmajority_nodes, timed  # noqa: E402


def torch_baseline(torch, kw, kv, kn, qw, qv, qn, nwords, stream, warmup, iters):
    """Median ms of the sparse-times-dense product on the same data, which form ran, or why none did."""
    N, S = kw.shape
    Q = qw.shape[0]
    dev = kw.device
    try:
        valid = torch.arange(S, device=dev)[None, :] < kn[:, None]
        crow = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        crow[1:] = torch.cumsum(kn.long(), 0)
        col, val = kw[valid].long(), kv[valid].float()
        qvalid = torch.arange(qw.shape[1], device=dev)[None, :] < qn[:, None]
        dense = torch.zeros((nwords, Q), dtype=torch.float32, device=dev)
        qi = torch.arange(Q, device=dev)[:, None].expand_as(qw)[qvalid]
        dense[qw[qvalid].long(), qi] = qv[qvalid].float()
    except Exception as e:                                           # (out of memory at a size that does not fit)
        return None, f"setup: {type(e).__name__}"
    try:
        A = torch.sparse_csr_tensor(crow, col, val, size=(N, nwords))
        fn = lambda: torch.sparse.mm(A, dense)
        fn()
        stream.synchronize()
        return timed(fn, stream, torch, warmup, iters), "torch.sparse.mm (CSR x dense)"
    except Exception:
        pass
    try:
        rows = torch.repeat_interleave(torch.arange(N, device=dev), kn.long())
        out = torch.zeros((N, Q), dtype=torch.float32, device=dev)

        def fn():
            out.zero_()
            out.index_add_(0, rows, dense[col] * val[:, None])
        fn()
        stream.synchronize()
        return timed(fn, stream, torch, warmup, max(5, iters // 10)), "index_add_ over the gathered postings"
    except Exception as e:
        return None, f"{type(e).__name__}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--sizes", default="1000,10000,100000", help="key frames in the database, comma-separated")
    ap.add_argument("--vocabs", default="fit,large")
    ap.add_argument("--topk", type=int, default=16)
    ap.add_argument("--iters", type=int, default=200, help="timed calls per entry point")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--baseline", type=int, default=1, help="0: skip the torch baseline")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bowdb needs a GPU (there is no CPU fallback)")
    from pislam_amd import synth
    from pislam_amd.capi import Context
    from pislam_amd.frontend import (BowDatabase, OrbFrontend, Vocabulary, bowTransformBatch, bowVectorBatch,
                                     bowWeightBatch)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx = Context(device=0, stream=stream.cuda_stream)
    Q, max_kp = args.queries, 2048
    levels = synth.level_table()
    rng = np.random.default_rng(args.seed)
    res = {}
    with torch.cuda.stream(stream):
        fe = OrbFrontend(levels, vstep=640, rows=synth.pyramid_rows(levels), max_keypoints=max_kp, ctx=ctx)
        kp, desc, counts = fe.alloc_outputs(Q + 1, dev)
        fe(torch.from_numpy(synth.make_batch(args.seed, Q + 1)).to(dev), kp, desc, counts)
        stream.synchronize()
        hd, hc = desc.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32)
        n = np.minimum(hc, max_kp).astype(np.int64)
        words = hd.shape[2]
        sample = np.concatenate([hd[b, :n[b]] for b in range(0, Q + 1, max(1, (Q + 1) // 16))])
        nodes = {"fit": (kmajority_nodes(rng, sample, K, FIT_DEPTH), FIT_DEPTH),
                 "large": (rng.integers(0, 2**32, (sum(K ** d for d in range(LARGE_DEPTH + 1)), words),
                                        dtype=np.uint64).astype(np.uint32), LARGE_DEPTH)}
        new = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
        for key in args.vocabs.split(","):
            v = Vocabulary.from_kary(*nodes[key][:1], K, nodes[key][1], 2, ctx=ctx)
            nwords = v.nwords
            idf = torch.from_numpy(rng.integers(1, 60000, nwords).astype(np.int32)).to(dev)
            word = bowTransformBatch(v, desc, counts, want_group=False, want_wdist=False, ctx=ctx)[0]
            bw, tf, bn = bowVectorBatch(word, counts, ctx=ctx)
            wt = new(Q + 1, max_kp)
            r = {"nwords": nwords,
                 "weight_ms": round(timed(lambda: bowWeightBatch(bw, tf, bn, idf, nwords, wt, ctx=ctx), stream, torch,
                                          args.warmup, args.iters), 4)}
            stream.synchronize()
            r["mean_distinct_words"] = round(float(bn.cpu().numpy().mean()), 1)
            stride = int(bn.max().item())
            stride = max(1, -(-stride // 64) * 64)
            kw, kv = bw[:, :stride].contiguous(), wt[:, :stride].contiguous()
            qw, qv, qn = kw[:Q].contiguous(), kv[:Q].contiguous(), bn[:Q].contiguous()
            outs = [new(Q, args.topk), new(Q, args.topk), new(Q, args.topk), new(Q)]
            for size in [int(s) for s in args.sizes.split(",")]:
                db = BowDatabase(nwords, stride, size, ctx=ctx)
                ev = []
                while db.size < size:
                    k = min(Q, size - db.size)
                    o = db.size % (Q + 1)
                    k = min(k, Q + 1 - o)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    db.add(kw[o:o + k], kv[o:o + k], bn[o:o + k])
                    b.record(stream)
                    ev.append((a, b, k))
                stream.synchronize()
                full = [a.elapsed_time(b) for a, b, k in ev if k == ev[0][2]]
                db.reserve_query(Q, args.topk)
                fn = lambda: db.query(qw, qv, qn, topk=args.topk, min_common_pct=80, top_id=outs[0], top_score=outs[1],
                                      top_common=outs[2], max_common=outs[3])
                ms = timed(fn, stream, torch, args.warmup, args.iters)
                # postings a query walks: the database's entries per word, summed over the query's words
                reps = torch.tensor([(size - o + Q) // (Q + 1) for o in range(Q + 1)], device=dev)   # times frame o is stored
                valid = torch.arange(stride, device=dev)[None, :] < bn[:, None]
                per_word = torch.zeros(nwords, dtype=torch.int64, device=dev)
                per_word.index_add_(0, kw[valid].long(), reps[:, None].expand(Q + 1, stride)[valid])
                touched = float(per_word[qw[valid[:Q]].long()].sum().item()) / Q
                e = {"add_ms_last_batch": round(full[-1], 4), "add_batch": ev[0][2], "fill_ms": round(sum(a.elapsed_time(b) for a, b, _ in ev), 2),
                     "query_ms": round(ms, 4), "postings_per_query": round(touched, 1),
                     "postings_per_s": round(Q * touched / (ms * 1e-3), 0),
                     "self_first": int((outs[0][:, 0].cpu().numpy() % (Q + 1) == np.arange(Q)).sum())}
                if args.baseline:
                    idx = torch.arange(size, device=dev) % (Q + 1)
                    try:
                        bms, how = torch_baseline(torch, kw[idx], kv[idx], bn[idx], qw, qv, qn, nwords, stream, 3, 20)
                    except Exception as ex:
                        bms, how = None, type(ex).__name__
                    e["torch_baseline_ms"] = None if bms is None else round(bms, 4)
                    e["torch_baseline"] = how
                    e["baseline_over_query"] = None if bms is None else round(bms / ms, 2)
                    torch.cuda.empty_cache()
                r[f"keyframes_{size}"] = e
                stream.synchronize()
                db.close()
            res[key] = r
            v.close()
    print(json.dumps({"tool": "bench_bowdb", "queries": Q, "topk": args.topk, "iters": args.iters, "results": res}))


if __name__ == "__main__":
    main()
