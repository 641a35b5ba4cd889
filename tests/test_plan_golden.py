"""CPU suite: the host planner answers every recorded case as the library the golden file was recorded from.

tests/golden/plan_summaries.json (tests/golden/make_golden.py plans) holds, for the seeded cases of tests/plan_fuzz.py and for
every option key with the values -1, 0, 1, 5, 64, 65 and 100000 alone in the options string (VGA level table, 16-pixel buckets,
batch 256), what pislam_debug_build_plan returned: return code, summary[0..7] and the error string.  A change of the planner
that is meant to keep every plan keeps this test; one that means to change plans re-records the file.

The seeded cases (seeds 0..999) were checked when the file was written: 615 return 0 (at least a quarter asked), 315 have
summary[7] > 0 (the bucket selection pass; at least 20 asked) and 195 have more plan entries than levels (x-tiles; at least
20 asked)."""
import json
import os

from conftest import GOLDEN

import plan_fuzz


def golden():
    with open(os.path.join(GOLDEN, "plan_summaries.json")) as f:
        return json.load(f)


def lib():
    from pislam_amd import capi
    return capi.load(rebuild_if_stale=False)


def test_seeded_plans_equal_the_recorded_ones():
    g, L = golden(), lib()
    first, n = g["seeds"]
    assert n == len(g["cases"]) >= 1000
    assert 4 * sum(rc == 0 for rc, _, _ in g["cases"]) >= n
    assert sum(s[7] > 0 for _, s, _ in g["cases"]) >= 20
    assert sum(s[0] > len(plan_fuzz.case(first + i)[0]) for i, (_, s, _) in enumerate(g["cases"])) >= 20
    for i, want in enumerate(g["cases"]):
        got = plan_fuzz.run_case(L, first + i)
        assert list(got) == want, f"seed {first + i}: {plan_fuzz.case(first + i)}"


def test_every_option_answers_its_range_edges_as_recorded():
    g, L = golden(), lib()
    assert tuple(g["option_values"]) == plan_fuzz.OPTION_VALUES and set(g["options"]) == set(plan_fuzz.OPTION_KEYS)
    for key in plan_fuzz.OPTION_KEYS:
        for value, want in zip(plan_fuzz.OPTION_VALUES, g["options"][key]):
            assert list(plan_fuzz.run_option(L, key, value)) == want, f"{key}={value}"
