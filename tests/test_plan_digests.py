"""The slice and lane planners' tables, byte for byte, on the CPU
(csrc/plan_slices.hip, csrc/plan_lanes.hip through mc_debug_plan_digest): every
case of tests/_plan_cases.py plans to the status, the message and the table
digests of tests/golden/plan_digests.json, recorded by
scripts/gen_plan_digests.py from the build before the planners were split into
stages.  A mismatch names the table."""
import json
import os

import pytest

from _plan_cases import CASES, PLANNER_ENV, PLANS, observe

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "plan_digests.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_file_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_plan_tables_are_unchanged(name, golden, monkeypatch):
    for var in PLANNER_ENV:
        monkeypatch.delenv(var, raising=False)
    for var, value in CASES[name][2].items():
        monkeypatch.setenv(var, value)
    want, got = golden[name], observe(name)
    if name in PLANS:       # (a plan was meant: never a recorded decline)
        assert want["status"] == 0 and int(want["digests"]["lane.ok"], 16) != 0
    else:
        assert want["status"] != 0 and want["error"]
    assert (got["status"], got["error"]) == (want["status"], want["error"])
    differ = [t for t in want["digests"] if got["digests"][t] != want["digests"][t]]
    assert not differ, f"{name}: tables that changed: {differ}"
    assert got == want
