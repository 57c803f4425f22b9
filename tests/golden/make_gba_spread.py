"""Writes tests/golden/gba_spread.json: per case of tests/gba_cases.py and per float output the largest scaled difference between any
two of the twelve arithmetic forms of the reference (tests/gba_reference.py, gba_cases.spread), and for the anchored cases the relative
difference between the reference's final chi2 and scipy.optimize.least_squares' with the bound 16 x that value.  The cases of
gba_cases.ONE_FORM run under all forms here and under one form in the suite.  tests/test_global_bundle_adjustment.py derives its bounds
from this file and checks that it is up to date.  It is measured on the reference alone, never from the device.
Run: python tests/golden/make_gba_spread.py"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gba_cases as GC  # noqa: E402
import gba_reference as GR  # noqa: E402

if __name__ == "__main__":
    out = {"forms": ["fma=%d order=%s chol=%s" % (f.fma, f.order, f.chol) for f in GR.FORMS],
           "rule": "bound = max(2 float ulps at the output's scale, 16 x spread); window = max(1e-9, 16 x the case's largest spread); "
                   "anchor bound = 16 x the measured relative difference",
           "spread": {n: GC.spread(n) for n in GC.CASE_NAMES}, "anchor": {}}
    for n in GC.ANCHORED:
        chi_ref, chi_sp, rel = GC.anchor(n)
        out["anchor"][n] = {"chi2_reference": chi_ref, "chi2_scipy": chi_sp, "relative_difference": rel, "bound": 16.0 * rel}
    with open(GC.SPREAD_FILE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GC.SPREAD_FILE)
