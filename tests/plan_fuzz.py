"""Helper of tests/test_sanitizers.py (not a test module): runs N random front-end configurations through the library's
host-only plan builder (pislam_debug_build_plan: strip plan, launch order, bucket selection plan + their invariants).  Run
with the sanitizer build of the library (tools/asan_round.sh: PISLAM_HIP_LIB + the ASan runtime preloaded), every
out-of-bounds access, signed overflow or invalid shift of the host code on that path aborts the process.

usage: python tests/plan_fuzz.py <cases> [<first seed>]      prints "<ok> plans, <refused> refused, 0 violations"
       python tests/plan_fuzz.py lines [<cases> <first seed>]  prints cases as lines for tools/probes/frontend_host_check.cpp """
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pislam_amd import capi  # noqa: E402


def case(seed):
    rng = np.random.default_rng(seed)
    kind = int(rng.integers(0, 4))
    if kind == 0:                                     # a x1.2 pyramid of a random frame size, stacked
        w0, h0 = int(rng.integers(40, 2000)), int(rng.integers(40, 1200))
        nl = int(rng.integers(1, 17))
        sizes = [(max(1, int(w0 / 1.2 ** k + 0.5)), max(1, int(h0 / 1.2 ** k + 0.5))) for k in range(nl)]
        vstep = (w0 + int(rng.choice([0, 0, 1, 15, 16]))) if rng.integers(0, 2) else (w0 + 15) // 16 * 16
        levels, row = [], 0
        for w, h in sizes:
            levels.append((w, h, row, 0))
            row += h
        rows = row + int(rng.integers(0, 3))
    else:                                             # random rectangles, some side by side
        vstep = int(rng.choice([64, 192, 208, 256, 320, 640, 1280, 1920, 4096]))
        nl = int(rng.integers(1, 17))
        levels, row, col, band = [], 0, 0, 0
        for _ in range(nl):
            w, h = int(rng.integers(1, vstep + 1)), int(rng.integers(1, 400))
            if col and col + 16 + w <= vstep and rng.integers(0, 2):
                c0 = (col + 2 + 15) // 16 * 16
                levels.append((w, h, row, c0))
                col, band = c0 + w, max(band, h)
            else:
                row += band
                levels.append((w, h, row, 0))
                col, band = w, h
        rows = row + band + int(rng.integers(0, 3))
    par = dict(vstep=vstep, rows=rows, nlevels=len(levels), border=int(rng.choice([16, 16, 17, 20, 24, 40])),
               fast_threshold=int(rng.integers(0, 256)), harris_threshold=int(rng.choice([-(1 << 31), 0, 1 << 15, (1 << 31) - 1])),
               log_bucket_size=int(rng.choice([0, 0, 1, 2, 3, 4, 5, 6, 7, 8])), bucket_limit=int(rng.integers(1, 65)),
               words=int(rng.choice([1, 2, 4, 8])), max_keypoints=int(rng.choice([1, 16, 4096, 65536])))
    opts = dict(alias=int(rng.integers(0, 2)), run_len=int(rng.choice([0, 0, 1, 2, 7, 64])),
                strip_rows=int(rng.choice([0, 0, 2, 10, 16, 22, 32, 64])), tile_cols=int(rng.choice([0, 0, -1, 64, 96, 320, 448, 4096])),
                strip_rows_max=int(rng.choice([0, 0, 16, 36, 64])), bucket_select=int(rng.integers(0, 2)),
                wgs_per_cu=int(rng.choice([0, 0, 1, 3, 5, 8])), strip_px=int(rng.choice([16384, 4096, 65536])),
                run_order=int(rng.integers(0, 2)), orb_in_strip=int(rng.integers(0, 2)), sub_batches=int(rng.choice([1, 1, 0, 3, 16])),
                lds_pad=int(rng.choice([0, 0, 4096])), bucket_round_up=int(rng.integers(0, 2)))
    batch = int(rng.choice([1, 2, 3, 8, 64, 256, 4096, 70000]))
    cus = int(rng.choice([256, 256, 1, 64, 304]))
    lanes = int(rng.choice([1, 1, 3, 8]))
    return levels, par, opts, batch, cus, lanes


PARAM_FIELDS = ("vstep", "rows", "nlevels", "border", "fast_threshold", "harris_threshold", "log_bucket_size", "bucket_limit",
                "words", "max_keypoints")


def build_plan(lib, levels, par, batch, cus, lanes, options):
    """One call of pislam_debug_build_plan: (return code, summary[0..7], error string)."""
    P = capi.FrontendParams(*[par[k] for k in PARAM_FIELDS])
    L = (capi.Level * len(levels))(*[capi.Level(*t) for t in levels])
    summary = (ctypes.c_uint32 * 8)()
    err = ctypes.create_string_buffer(256)
    rc = lib.pislam_debug_build_plan(ctypes.byref(P), L, batch, cus, lanes, options.encode(), ctypes.byref(summary), err, 256)
    return rc, list(summary), err.value.decode()


def options_string(opts):
    return ",".join(f"{k}={v}" for k, v in opts.items())


def run_case(lib, seed):
    levels, par, opts, batch, cus, lanes = case(seed)
    return build_plan(lib, levels, par, batch, cus, lanes, options_string(opts))


def case_line(name, levels, par, batch, cus, lanes, options):
    """A case as one line of the text tools/probes/frontend_host_check.cpp reads (tests/golden/frontend_plan_cases.txt): name,
    the ten parameter fields, batch, CUs, lanes, the options string (- for none), then width height row0 col0 of every level."""
    words = [name] + [par[k] for k in PARAM_FIELDS] + [batch, cus, lanes, options or "-"] + [v for t in levels for v in t]
    return " ".join(str(w) for w in words)


def seed_line(seed):
    levels, par, opts, batch, cus, lanes = case(seed)
    return case_line(f"seed{seed}", levels, par, batch, cus, lanes, options_string(opts))


# Every key of pislam_ctx_set_option, and the values that straddle its range checks (tests/test_plan_golden.py passes each
# pair alone in the options string, on the VGA level table of tests/test_abi.py at batch 256).
OPTION_KEYS = ("pipeline", "own_stream", "dump_score", "repeat_strips", "alias", "run_len", "lds_pad", "wgs_per_cu", "match_mfma",
               "run_order", "strip_px", "strip_rows_max", "tile_cols", "frame", "frame_test", "frame_rearm", "build_chain",
               "orb_in_strip", "bucket_select", "dist_rccl_single", "bucket_round_up", "orb_chunks", "sub_batches", "sub_mb",
               "ablate", "strip_rows", "no_such_option")
OPTION_VALUES = (-1, 0, 1, 5, 64, 65, 100000)


def vga_case(log_bucket_size=4):
    """The VGA level table and parameters of tests/test_abi.py (there without buckets; the option cases use 16-pixel ones)."""
    from pislam_amd import synth
    levels = [(w, h, r0, 0) for w, h, r0 in synth.level_table()]
    par = dict(vstep=640, rows=2210, nlevels=8, border=16, fast_threshold=20, harris_threshold=1 << 15,
               log_bucket_size=log_bucket_size, bucket_limit=3, words=8, max_keypoints=4096)
    return levels, par


def run_option(lib, key, value):
    levels, par = vga_case()
    return build_plan(lib, levels, par, 256, 256, 1, f"{key}={value}")


def option_line(key, value):
    levels, par = vga_case()
    return case_line(f"{key}={value}", levels, par, 256, 256, 1, f"{key}={value}")


# The generated cases of tests/test_frontend_plan_golden.py, behind the fixed ones of tests/golden/frontend_plan_cases.txt:
# these seeds, then every option of fp::Options (own_stream and frame_rearm belong to the context) with every value.
CASE_SEEDS = range(0, 400)


def generated_lines():
    return [seed_line(s) for s in CASE_SEEDS] + [option_line(k, v) for k in OPTION_KEYS if k not in ("own_stream", "frame_rearm")
                                                 for v in OPTION_VALUES]


def main():
    if sys.argv[1:2] == ["lines"]:                    # lines [<seeds> <first seed>]: cases for tools/probes/frontend_host_check.cpp
        lines = [seed_line(s) for s in range(int(sys.argv[3]), int(sys.argv[3]) + int(sys.argv[2]))] if len(sys.argv) > 3 else generated_lines()
        print("\n".join(lines))
        return 0
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    lib = capi.load(rebuild_if_stale=False)
    ok = refused = 0
    for seed in range(first, first + n):
        rc, _, err = run_case(lib, seed)
        if rc == 0:
            ok += 1
        elif rc == -1:                                # PISLAM_ERR_INVALID: refused parameters, or the staged pipeline takes the call
            refused += 1
        else:
            levels, par, opts, batch, cus, lanes = case(seed)
            print(f"seed {seed}: rc {rc}: {err}\n  levels {levels}\n  params {par}\n  options {opts} batch {batch} "
                  f"cus {cus} lanes {lanes}")
            return 1
    print(f"{ok} plans, {refused} refused, 0 violations ({n} cases from seed {first}; library {capi.library_path()})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
