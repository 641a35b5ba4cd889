#!/usr/bin/env python3
"""tests/golden/make_golden.py — regenerates the committed fixtures (dev container only).

  demo_pyramid.npz   : the reference's own demo input (demo/input.png, a 640x2210 grey stacked
                       pyramid = DATA, decoded to raw pixels) plus the outputs of every stage of
                       the hot path on it.  The outputs are produced by the oracle and are only
                       written if their SHA-256 prefixes equal the ones SURVEY.md §8c recorded from
                       the reference's headers, so the fixture is pinned to the reference's results.
  synth_small.npz    : a 3-level 160x120 synthetic pyramid + oracle outputs (regression fixture
                       for the generator and the oracle; small enough for pure-Python checks).
  brief_table_ref.npy: written by oracle/gen_brief_pattern.py (probe of the compiled Brief.h).
  plan_summaries.json: what pislam_debug_build_plan answers for the seeded cases of tests/plan_fuzz.py and for every option
                       at the edges of its range (`make_golden.py plans`: recorded from the library that is loaded, which
                       must be the one whose planner is the reference for tests/test_plan_golden.py).
  build_plans.json   : what pislam_pyramid_build_batch answered, before its planner moved into pislam_prep_plan.h, for the
                       fixed cases of tools/probes/prep_host_check.cpp: one [name, answer] pair per line of that program's
                       --dump.  Not made by this script: the function's text at that commit was compiled on the host with
                       is_device_ptr, the HIP calls and the launches replaced by stubs that record them, and the line was
                       printed from inside it (docs/experiments.md section V).  A planner that is meant to change plans
                       re-records it as `prep_host_check --dump`.
  frontend_plan_cases.txt : the fixed named cases tools/probes/frontend_host_check.cpp and tests/test_frontend_plan_golden.py
                       run, one per line (`make_golden.py plan-cases`); the test appends tests/plan_fuzz.py's generated_lines().
  frontend_plans.json: per case (fixed by name, seeds in order, options by key in the order of their values) the first 16 hex digits of the SHA-256 of its fp::plan_digest line, as
                       the planner answered before it moved into pislam_frontend_plan.h.  Not made by this script: in a
                       scratch copy of that commit plan_digest was pasted behind FrontendPlan and one extra exported function
                       made the digest the way frontend_host_check does (options through pislam_ctx_set_option on a stack
                       context, check_params, plan_frontend; the refusal is the context's error text); that library was built
                       with `python -m pislam_amd.build` and called through ctypes for every case line (docs/experiments.md
                       section X).  A planner that is meant to change plans re-records it from `frontend_host_check --dump`.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import orc            # noqa: E402
from pislam_amd import synth      # noqa: E402

# SHA-256 prefixes recorded in SURVEY.md §8c ("Results obtained")
SURVEY_PINS = {
    "img": "0f7c28c31d3466be", "det": "205ff4f820fd568c", "score": "7f0f15bfc5110f4c",
    "kp": "03f731507fe64358", "kp_bucket43": "feb6071b7035e57d", "centroids": "6e06b93c6186852c",
    "angles": "5c511df056e40160", "desc": "86199421e6b3a298",
}


def H(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def stages(img, levels):
    det = np.zeros_like(img)
    for w, h, r0 in levels:
        orc.fast_detect(img[r0:r0 + h], det[r0:r0 + h], w, h, 20)
    score = det.copy()
    for w, h, r0 in levels:
        orc.fast_score_harris(img[r0:r0 + h], score[r0:r0 + h], w, h)
    kp = np.concatenate([orc.fast_extract(score[r0:r0 + h], w, h) + np.uint32(r0) for w, h, r0 in levels])
    kpb = np.concatenate([orc.fast_extract(score[r0:r0 + h], w, h, log_bucket=4, bucket_limit=3) + np.uint32(r0)
                          for w, h, r0 in levels])
    cen = orc.orb_centroids(img, kp)
    ang = orc.atan2_bins(cen)
    desc = orc.orb_compute(img, kp)
    return dict(det=det, score=score, kp=kp.astype(np.uint32), kp_bucket43=kpb.astype(np.uint32),
                centroids=cen, angles=ang, desc=desc)


PLAN_SEEDS = (0, 1000)


def plan_summaries():
    import json
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import plan_fuzz
    from pislam_amd import capi
    lib = capi.load(rebuild_if_stale=False)
    seeds = range(PLAN_SEEDS[0], PLAN_SEEDS[0] + PLAN_SEEDS[1])
    cases = [plan_fuzz.run_case(lib, s) for s in seeds]
    # the conditions tests/test_plan_golden.py states about its inputs
    assert 4 * sum(rc == 0 for rc, _, _ in cases) >= len(cases)
    assert sum(s[7] > 0 for _, s, _ in cases) >= 20
    assert sum(s[0] > len(plan_fuzz.case(sd)[0]) for sd, (_, s, _) in zip(seeds, cases)) >= 20
    options = {k: [plan_fuzz.run_option(lib, k, v) for v in plan_fuzz.OPTION_VALUES] for k in plan_fuzz.OPTION_KEYS}
    with open(os.path.join(HERE, "plan_summaries.json"), "w") as f:
        json.dump(dict(seeds=list(PLAN_SEEDS), cases=cases, option_values=list(plan_fuzz.OPTION_VALUES),
                       options=options), f, separators=(",", ":"))
        f.write("\n")
    print("plan_summaries.json ok:", len(cases), "cases,", len(options), "options")


def plan_cases():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import plan_fuzz
    vga, par = plan_fuzz.vga_case(log_bucket_size=0)
    lines = [plan_fuzz.case_line(f"vga-b{b}", vga, par, b, 256, 1, "") for b in (1, 2, 3, 64, 256)]
    lines.append(plan_fuzz.case_line("vga-b256-lanes3", vga, par, 256, 256, 3, ""))
    lines.append(plan_fuzz.case_line("vga-b256-sub3", vga, par, 256, 256, 1, "sub_batches=3"))
    lines.append(plan_fuzz.case_line("vga-b256-buckets", *plan_fuzz.vga_case(), 256, 256, 1, ""))
    wide = synth.packed_level_table()                          # 1280 x 960: the two largest levels are cut into x-tiles
    lines.append(plan_fuzz.case_line("1280x960-b256", wide, dict(par, vstep=1280, rows=synth.pyramid_rows(wide)), 256, 256, 1, ""))
    narrow = [(31, 40, 0, 0), (26, 33, 40, 0)]                 # every level narrower than 2 x border: strips_per_pyr == 0
    lines.append(plan_fuzz.case_line("narrower-than-the-border", narrow, dict(par, vstep=32, rows=73, nlevels=2), 4, 256, 1, ""))
    tiled = [(832, 40, 40 * i, 0) for i in range(12)] + [(100, 40, 480, 0)]   # 12 levels of two x-tiles + one: 25 plan entries
    lines.append(plan_fuzz.case_line("25-plan-entries", tiled, dict(par, vstep=832, rows=520, nlevels=13), 64, 256, 1, ""))
    with open(os.path.join(HERE, "frontend_plan_cases.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("frontend_plan_cases.txt ok:", len(lines), "fixed cases")


def main():
    if sys.argv[1:] == ["plans"]:
        return plan_summaries()
    if sys.argv[1:] == ["plan-cases"]:
        return plan_cases()
    from PIL import Image
    img = np.ascontiguousarray(np.array(Image.open("/root/reference/demo/input.png")))
    levels = synth.level_table()
    out = stages(img, levels)
    out["img"] = img
    for k, v in SURVEY_PINS.items():
        assert H(out[k]) == v, f"{k}: oracle output {H(out[k])} != SURVEY pin {v}"
    # det/score maps are recomputable; keep the fixture small: image + list outputs + map hashes
    np.savez_compressed(os.path.join(HERE, "demo_pyramid.npz"), img=img, kp=out["kp"],
                        kp_bucket43=out["kp_bucket43"], centroids=out["centroids"], angles=out["angles"],
                        desc=out["desc"], det_nonzero=np.flatnonzero(out["det"]).astype(np.uint32),
                        score_idx=np.flatnonzero(out["score"]).astype(np.uint32),
                        score_val=out["score"].reshape(-1)[np.flatnonzero(out["score"])])
    print("demo_pyramid.npz ok:", {k: H(out[k]) for k in SURVEY_PINS})

    lv = synth.level_table(160, 120, 3)
    p = synth.make_pyramid(7, w0=160, h0=120, nlevels=3, levels=lv, nshapes=12)
    s = stages(p, lv)
    np.savez_compressed(os.path.join(HERE, "synth_small.npz"), img=p, levels=np.array(lv, np.int32), **s)
    print("synth_small.npz ok:", len(s["kp"]), "kp", H(p))


if __name__ == "__main__":
    main()
