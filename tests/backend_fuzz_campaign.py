"""Long-running seeded fuzz campaign of the back-end kernels against their host probes (test infrastructure; run on the GPU
box).  The counterpart of tests/fuzz_campaign.py for the kernels of tests/test_backend_fuzz.py, with that module's
generator and comparison:
    python tests/backend_fuzz_campaign.py --kernel NAME|all --seeds 4000 [--start 100000] [--chunk 256]
    python tests/backend_fuzz_campaign.py --kernel NAME --seed S --dump [--start 100000] [--chunk 256]
The seeds are taken CHUNK at a time; the cases of a chunk that share a parameter set make one call, as in the tests.
Prints every mismatch with its seed and exits non-zero on any.  Every launch is followed by a synchronise and an error
check; on a HIP error, or a call the library refuses, the campaign stops at once and starts nothing further.

--dump needs no GPU: it prints the case's probe line (at its place in its call, which the RANSAC samplers depend on), the
probe's result and the restatement's."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def show(r):
    if isinstance(r, dict):
        return "\n".join("  %-12s %s" % (k, show(v).replace("\n", " ")) for k, v in r.items())
    a = np.asarray(r)
    if a.dtype == np.float32:
        return " ".join("%08x" % v for v in np.ascontiguousarray(a).reshape(-1).view(np.uint32)[:64]) + (" ..." if a.size > 64 else "")
    if a.dtype == np.float64:
        return " ".join("%016x" % v for v in np.ascontiguousarray(a).reshape(-1).view(np.uint64)[:64])
    return " ".join(str(v) for v in a.reshape(-1)[:256].tolist()) + (" ..." if a.size > 256 else "")


def dump(fz, args):
    kernel, row = args.kernel, fz.ROWS[args.kernel]
    first = args.start + (args.seed - args.start) // args.chunk * args.chunk
    for s, cases in fz.batches(kernel, range(first, first + args.chunk)):
        for b, c in enumerate(cases):
            if c["seed"] != args.seed:
                continue
            items = [x["item"] for x in cases]
            print("case", fz.tag(c), "at place %d of %d in its call" % (b, len(cases)))
            lines = row.lines(row.sets[s], items)
            print("probe line%s:" % ("s (one per slot)" if len(lines) != len(items) else ""))
            if len(lines) == len(items):
                print(lines[b])
            else:                                            # one line per slot: this case's
                at = sum(len(x["obs1"]) for x in items[:b])
                print("\n".join(lines[at:at + len(items[b]["obs1"])]))
            want = fz.expect(kernel, s, cases)[b]
            print("the probe's result:\n" + show(want))
            ref = row.restate(row.sets[s], items, b)
            print("the restatement's result:\n" + show({k: ref[k] for k in want if k in ref}))
            try:
                row.same(want, ref, fz.tag(c))
                print("the two agree")
            except AssertionError as e:
                print("THE TWO DIFFER:", str(e)[:300])
                return 1
            return 0
    print("seed %d is not in the chunk from %d" % (args.seed, first))
    return 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", default="all")
    ap.add_argument("--seeds", type=int, default=1024)
    ap.add_argument("--start", type=int, default=100000)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--seed", type=int)
    ap.add_argument("--dump", action="store_true")
    args = ap.parse_args()
    import test_backend_fuzz as fz
    if args.dump:
        return dump(fz, args)
    import torch
    from pislam_amd.capi import Context
    ctx = Context(device=0)
    bad, t0 = 0, time.time()
    for kernel in (fz.KERNELS if args.kernel == "all" else [args.kernel]):
        row, kbad, calls, tk = fz.ROWS[kernel], 0, 0, time.time()
        for first in range(args.start, args.start + args.seeds, args.chunk):
            seeds = range(first, min(first + args.chunk, args.start + args.seeds))
            for s, cases in fz.batches(kernel, seeds):
                want = fz.expect(kernel, s, cases)
                try:
                    got = row.launch(ctx, row.sets[s], [c["item"] for c in cases])
                    torch.cuda.synchronize()
                except Exception as e:                       # a refused call or a HIP error: nothing further is started
                    print("STOPPED: %s, seeds %d..%d, parameter set %d: %s: %s" % (kernel, seeds[0], seeds[-1], s, type(e).__name__, str(e)[:500]),
                          flush=True)
                    return 2
                calls += 1
                for c, msg in fz.mismatches(kernel, s, cases, want, got):
                    kbad += 1
                    print("MISMATCH", fz.tag(c), msg, flush=True)
        bad += kbad
        print("%s: %d cases from seed %d in %d calls: %d mismatches, %.0f s" % (kernel, args.seeds, args.start, calls, kbad, time.time() - tk),
              flush=True)
    print("%d mismatches in all, %.0f s" % (bad, time.time() - t0))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
