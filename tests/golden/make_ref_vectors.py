#!/usr/bin/env python3
"""Generate tests/golden/ref_dbow2.npz and tests/golden/ref_kahan.npz.

WHAT THESE VECTORS ARE: the outputs of the REFERENCE's own code -- DBoW2's BowVector.cpp /
FeatureVector.cpp and include/math/math.hpp's KahanSum, compiled into oracle/_ref/ by
oracle/Makefile.ref -- for exactly the inputs tests/test_bow.py and tests/test_calibration.py
draw.  The tests compare the product and the oracle with these stored outputs, so they run
where the reference sources are absent; where oracle/_ref/ is built they also recompute the
reference's outputs and require them to equal the stored ones.

Each case stores the SHA-256 of its inputs ("<key>.inputs"): a test whose inputs drift from
the ones recorded here fails instead of comparing against the wrong vector.

Run from the repository root on a machine with the reference sources:
    python tests/golden/make_ref_vectors.py
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import orb_oracle  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return np.array(h.hexdigest())


def bow_case(out, key, word, weight, node, scoring=None, weighting=None):
    (bid, bval), (fnode, fstart, ffeat) = orb_oracle.ref_bow_vectors(word, weight, node, scoring, weighting)
    out[key + ".inputs"] = digest(word, weight, node)
    out[key + ".bid"], out[key + ".bval"] = bid, bval
    out[key + ".fnode"], out[key + ".fstart"], out[key + ".ffeat"] = fnode, fstart, ffeat


def main():
    if orb_oracle.ref_dbow2() is None or orb_oracle.ref_kahan_sum(np.zeros((1, 3))) is None:
        raise SystemExit("oracle/_ref/ is not built and cannot be (the reference sources are absent)")
    out = {}
    # test_bow.py::test_bow_vectors_match_real_reference_code
    rng = np.random.RandomState(3)
    for n in (0, 1, 7, 500, 2000):
        word = rng.randint(0, 300, n).astype(np.uint32)
        wtab = np.round(rng.uniform(0.0, 9.0, 300), 5)
        wtab[rng.randint(0, 300, 20)] = 0.0
        weight = wtab[word]
        node = (word // 7).astype(np.uint32)
        bow_case(out, "tfidf_l1_n%d" % n, word, weight, node)
    # test_bow.py::test_bow_vectors_every_scoring_and_weighting_type
    for scoring in range(6):
        for weighting in range(4):
            rng = np.random.RandomState(40 + scoring * 4 + weighting)
            word = rng.randint(0, 120, 700).astype(np.uint32)
            wtab = np.round(rng.uniform(0.0, 9.0, 120), 5)
            wtab[rng.randint(0, 120, 9)] = 0.0
            weight, node = wtab[word], (word // 5).astype(np.uint32)
            bow_case(out, "s%d_w%d" % (scoring, weighting), word, weight, node, scoring, weighting)
    np.savez_compressed(os.path.join(OUT, "ref_dbow2.npz"), **out)

    # test_calibration.py::test_kahan_sum_equals_the_reference_header
    r = np.random.default_rng(6)
    v = r.normal(0, 1, (5000, 3)) * 10.0 ** r.integers(-8, 9, (5000, 1))
    np.savez_compressed(os.path.join(OUT, "ref_kahan.npz"), **{"kahan.inputs": digest(v), "kahan.sum": orb_oracle.ref_kahan_sum(v)})


if __name__ == "__main__":
    main()
