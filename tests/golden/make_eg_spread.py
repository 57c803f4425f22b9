"""Writes tests/golden/eg_spread.json: per case of tests/eg_cases.py and per output, the largest difference in ulps of the output's
format between the device form of tests/eg_reference.py and each of its other arithmetic forms (eg_reference.FORMS: contraction,
the summation orders, LLT and LDLT, libm one ulp up).  tests/test_optimize_essential_graph.py derives its bounds from this file
(eg_cases.bounds) and checks that it is up to date.  It is measured on the reference alone, never from the device.
Run: python tests/golden/make_eg_spread.py"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import eg_cases as EC  # noqa: E402

if __name__ == "__main__":
    out = {n: EC.measure_spread(n) for n in EC.NAMES}
    with open(EC.SPREAD_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", EC.SPREAD_PATH)
