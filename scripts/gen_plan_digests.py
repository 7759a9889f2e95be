#!/usr/bin/env python3
"""Record tests/golden/plan_digests.json: the status, error text and table
digests (mc_debug_plan_digest) of every case of tests/_plan_cases.py, from the
library as built.  Run on the CPU; a planner change that is meant to keep the
plans rewrites the file with no diff."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from _plan_cases import CASES, PLANNER_ENV, PLANS, observe  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "plan_digests.json")


def main():
    out = {}
    for name, (_, _, env) in CASES.items():
        for var in PLANNER_ENV:
            os.environ.pop(var, None)
        os.environ.update(env)
        out[name] = observe(name)
        planned = out[name]["status"] == 0 and int(out[name]["digests"]["lane.ok"], 16) != 0
        print(f"{name}: status {out[name]['status']} {out[name]['error']}")
        if (name in PLANS) != planned:
            raise SystemExit(f"{name}: expected {'a plan' if name in PLANS else 'a decline'}")
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
