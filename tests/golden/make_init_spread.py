"""Writes tests/golden/init_spread.json: per case of tests/init_cases.py, the spread among the reference's three forms of
acos(c)*180/pi (the double acos of the float, float32 arccos, atan2 of the sine and cosine) at the order statistic CheckRT picks
(init_cases.spread).  Measured on the reference only, never on the library.

    python tests/golden/make_init_spread.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import init_cases as IC  # noqa: E402

if __name__ == "__main__":
    out = {c.name: IC.spread(c, IC.run(c)) for c in IC.build()}
    with open(IC.SPREAD_FILE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d cases)" % (IC.SPREAD_FILE, len(out)))
