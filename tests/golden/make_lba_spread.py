"""Writes tests/golden/lba_spread.json: per case of tests/lba_cases.py and per float output, the largest scaled difference between
any two of the reference's arithmetic forms (tests/lba_reference.FORMS: contraction on and off, three summation orders, LLT and
LDLT).  tests/test_local_bundle_adjustment.py derives its tolerances and the case condition's window from this file
(lba_cases.bounds, lba_cases.window_of) and checks that it is up to date.  Run: python tests/golden/make_lba_spread.py"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import lba_cases as LC  # noqa: E402
import lba_reference as LR  # noqa: E402

if __name__ == "__main__":
    out = {"forms": ["fma=%d order=%s chol=%s" % (f.fma, f.order, f.chol) for f in LR.FORMS],
           "rule": "bound = max(2 float ulps at the output's scale, 16 x spread); window = max(1e-9, 16 x the case's largest spread)",
           "spread": {n: LC.spread(n) for n in LC.CASE_NAMES}}
    with open(LC.SPREAD_FILE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", LC.SPREAD_FILE)
