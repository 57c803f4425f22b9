"""Writes tests/golden/pnp_spread.json: per case of tests/pnp_cases.py, the spread between the reference's forms of Refine's long sums
(sequential from 0, the device's shape too; pairwise halves) in the returned pose and in error2 (pnp_cases.spread).  Measured on the
reference only, never on the library; raises if the forms disagree in an integer output.

    python tests/golden/make_pnp_spread.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pnp_cases as PC  # noqa: E402

if __name__ == "__main__":
    out = {c.name: PC.spread(c) for c in PC.all_cases()}
    with open(PC.SPREAD_FILE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d cases)" % (PC.SPREAD_FILE, len(out)))
