"""Writes tests/golden/pose_opt_spread.json: per case of tests/pose_cases.py and per float output (R, t, Ow, chi2) the largest scaled
difference between the results of tests/pose_reference.py under its three summation orders.  tests/test_pose_optimization.py
derives its float tolerances from this file (pose_cases.bounds) and checks that it is up to date.  Run from the repository root:
    python tests/golden/make_pose_opt_spread.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pose_cases as PC  # noqa: E402


def measure():
    return {c.name: PC.spread(c) for c in PC.all_cases()}


if __name__ == "__main__":
    with open(os.path.join(HERE, "pose_opt_spread.json"), "w") as f:
        json.dump(measure(), f, indent=1, sort_keys=True)
        f.write("\n")
