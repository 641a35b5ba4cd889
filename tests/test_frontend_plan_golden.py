"""CPU suite: the front end's host planner (pislam_amd/csrc/pislam_frontend_plan.h), compiled with g++ alone, answers every
recorded case as the library the golden file was recorded from.

The cases: the fixed named ones of tests/golden/frontend_plan_cases.txt (tests/golden/make_golden.py plan-cases), then
tests/plan_fuzz.py's generated_lines(): seeds 0..399 of case() and every option of fp::Options alone at the edges of its range.
tools/probes/frontend_host_check.cpp --dump prints fp::plan_digest of each from the header: the refusal text or "ok", every
scalar of fp::FrontendPlan, FNV-1a-64 hashes of the bytes of the strip plan, the selection plan and the unit plan, and length
and hash of the unit table.  tests/golden/frontend_plans.json holds 16 hex digits of the SHA-256 of that line per case, as the
planner answered before it moved into the header (make_golden.py says how it was recorded).  A change of the planner that is
meant to keep every plan keeps this test; one that means to change plans re-records the file."""
import hashlib
import json
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

import plan_fuzz

SCALARS = ("fused nsub submax lds lds_alias klds sel sel_lds glds alias ovf_stride sdesc_per_pyr generic_orb frame nch fch per_max "
           "olds fper flds").split()


def scalars(digest):
    """(refusal text or "ok", {scalar: value}) of a digest: the text, the scalars, then F= Q= U= utab=."""
    words = digest.split(" ")
    text, values = words[:-len(SCALARS) - 4], words[-len(SCALARS) - 4:-4]
    return " ".join(text), dict(zip(SCALARS, map(int, values)))


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """[(name, digest)] of every case, from the header alone."""
    tmp = tmp_path_factory.mktemp("frontend_plan")
    exe, cases = tmp / "frontend_host_check", tmp / "cases.txt"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "pislam_amd", "csrc"),
                        os.path.join(ROOT, "tools", "probes", "frontend_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(GOLDEN, "frontend_plan_cases.txt")) as f:
        cases.write_text(f.read() + "\n".join(plan_fuzz.generated_lines()) + "\n")
    r = subprocess.run([str(exe), "--dump", str(cases)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])        # (non-zero: a plan violates an invariant)
    return [tuple(line.split(": ", 1)) for line in r.stdout.splitlines()]


def test_planner_header_alone_answers_every_case_as_recorded(dump):
    with open(os.path.join(GOLDEN, "frontend_plans.json")) as f:
        g = json.load(f)
    keys = [k for k in plan_fuzz.OPTION_KEYS if k not in ("own_stream", "frame_rearm")]
    assert list(g["options"]) == keys
    want = list(g["fixed"].items())
    want += zip((f"seed{s}" for s in plan_fuzz.CASE_SEEDS), " ".join(g["seeds"]).split())
    want += [(f"{k}={v}", h) for k in keys for v, h in zip(plan_fuzz.OPTION_VALUES, g["options"][k].split())]
    assert [n for n, _ in dump] == [n for n, _ in want]
    for (name, digest), (_, h) in zip(dump, want):
        assert hashlib.sha256(digest.encode()).hexdigest()[:16] == h, (name, digest)


def test_cases_cover_what_they_are_there_for(dump):
    """Caps on the inputs, not measurements: the recorded library has 238, 118, 86, 53 and 22 (the test above holds the digests
    these figures are read from to the recorded ones)."""
    answers = {name: scalars(d) for name, d in dump}
    seeds = plan_fuzz.CASE_SEEDS
    accepted = [s for s in seeds if answers[f"seed{s}"][0] == "ok" and answers[f"seed{s}"][1]["fused"]]
    assert len(accepted) >= 100
    assert sum(answers[f"seed{s}"][1]["sel"] for s in accepted) >= 20
    assert sum(plan_fuzz.case(s)[3] <= 2 for s in accepted) >= 20
    assert sum(plan_fuzz.case(s)[1]["vstep"] % 16 != 0 and answers[f"seed{s}"][1]["generic_orb"] for s in accepted) >= 10
    # plan entries are inside the hashed strip plan: plan_summaries.json has them for the same seeds, from the same library
    with open(os.path.join(GOLDEN, "plan_summaries.json")) as f:
        summaries = json.load(f)
    assert summaries["seeds"][0] == seeds[0] and summaries["seeds"][1] >= len(seeds)
    assert [s for s in seeds if summaries["cases"][s][0] == 0] == accepted
    assert sum(summaries["cases"][s][1][0] > len(plan_fuzz.case(s)[0]) for s in seeds) >= 20
    fixed = [a for name, a in answers.items() if not name.startswith("seed") and "=" not in name]
    assert len(fixed) >= 10 and all(text == "ok" for text, _ in fixed)
    assert any(a["frame"] == 1 for _, a in fixed) and any(a["nsub"] > 1 for _, a in fixed)
    assert answers["narrower-than-the-border"][1]["fused"] == 1 and answers["narrower-than-the-border"][1]["glds"] == 0
    assert answers["25-plan-entries"][1]["fused"] == 0
