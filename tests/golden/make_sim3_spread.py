"""Writes tests/golden/sim3_spread.json: per case of tests/sim3_cases.py and per float output (R, t, s, and err relative to its
threshold) the largest scaled difference between the results of tests/sim3_reference.py under its arithmetic forms (float against
double accumulation for the centroid, M and the scale sums; numpy.linalg.eigh against the Jacobi).  tests/test_sim3_solver.py
derives its float tolerances and the window of its case condition from this file (sim3_cases.bounds, sim3_cases.window) and
checks that it is up to date.  Run from the repository root:
    python tests/golden/make_sim3_spread.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sim3_cases as SC  # noqa: E402


def measure():
    return {c.name: SC.spread(c) for c in SC.all_cases()}


if __name__ == "__main__":
    with open(os.path.join(HERE, "sim3_spread.json"), "w") as f:
        json.dump(measure(), f, indent=1, sort_keys=True)
        f.write("\n")
