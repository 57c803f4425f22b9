"""Writes tests/golden/optsim3_spread.json: per case of tests/optsim3_cases.py and per float output, the largest scaled difference
between any two of the reference's arithmetic forms (tests/optsim3_reference.FORMS).  tests/test_optimize_sim3.py derives its
tolerances from this file (optsim3_cases.bounds) and checks that it is up to date.  Run: python tests/golden/make_optsim3_spread.py"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import optsim3_cases as OC  # noqa: E402
import optsim3_reference as OR  # noqa: E402

if __name__ == "__main__":
    out = {"forms": list(OR.FORMS), "rule": "bound = max(2 float ulps at the output's scale, 16 x spread)",
           "spread": {c.name: OC.spread(c) for c in OC.all_cases()}}
    with open(OC.SPREAD_FILE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OC.SPREAD_FILE)
