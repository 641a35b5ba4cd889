"""CPU suite: the pyramid build's host planner (pislam_amd/csrc/pislam_prep_plan.h) answers every recorded case as the
library the golden file was recorded from.

tests/golden/build_plans.json holds, per fixed case of tools/probes/prep_host_check.cpp, what pislam_pyramid_build_batch
made of it before the planner moved into the header: the refusal text, or whether the reductions run as one launch, that
launch's grid and counter words, which reductions take the 4-block kernel, and FNV-1a-64 hashes of the bytes of
pp::ZeroPlan and pp::ChainPlan (tests/golden/make_golden.py says how it was recorded).  A change of the planner that is
meant to keep every plan keeps this test; one that means to change plans re-records the file."""
import json
import os
import subprocess

from conftest import GOLDEN, ROOT


def golden():
    with open(os.path.join(GOLDEN, "build_plans.json")) as f:
        return json.load(f)["cases"]


def test_fixed_build_plans_equal_the_recorded_ones(tmp_path):
    exe = tmp_path / "prep_host_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "pislam_amd", "csrc"),
                        os.path.join(ROOT, "tools", "probes", "prep_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), "--dump"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = [line.split(": ", 1) for line in r.stdout.splitlines()]
    want = golden()
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, g), (_, w) in zip(got, want):
        assert g == w, name
    # what the file is there to cover: every refusal, both kernels, the one-launch build and its fall-backs
    answers = dict(want)
    assert sum(not a.startswith("ok ") for a in answers.values()) == 6 and len(set(answers.values())) >= 20
    assert "chain=1" in answers["64x40-9"] and "chain=0" in answers["48x40-9"]
    assert "chain=0" in answers["40x40-quad-loads-do-not-fit"] and "quads=4 " in answers["40x40-quad-loads-do-not-fit"]
    assert "chain=0" in answers["pyramids-misaligned"] and "quads=0 " in answers["vstep-misaligned"]
