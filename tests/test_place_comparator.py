"""The C++ comparator of tools/next_tier_bench.py's place-recognition row (tools/place_comparator.py: std::map BowVectors, std::list
inverted lists) equals the sequential reference of tests/place_reference.py on the constructed and random cases, so the time the
tool prints beside the GPU's is the time of a correct restatement."""
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import place_cases as PC  # noqa: E402
import place_comparator as CMP  # noqa: E402


def test_comparator_equals_the_reference():
    assert shutil.which("g++"), "the comparator is compiled with g++"
    cases = PC.edge_cases() + [PC.random_case(s) for s in range(12)] + [PC.long_vectors_case("reloc"), PC.many_key_frames_case("loop")]
    failed = []
    for c in cases:
        want = PC.run_reference(c)
        t = PC.table(PC.build(c))
        loop = c.form == "loop"
        cand, ncand, common, score, stats, sec = CMP.run(loop, t["bow_start"], t["bow_id"], t["bow_val"], t["in_db"], t["neigh_start"], t["neigh"],
                                                         [t["query"]], None if loop else t["state"], [t["min_score"]], [0, len(t["conn"])],
                                                         t["conn"], ccap=1200)
        got = dict(cand=cand[0, :ncand[0]].tolist(), common=common[0], score=score[0], stats=tuple(int(x) for x in stats[0]))
        if not PC.same(got, want) or sec < 0:
            failed.append((c.name, got["cand"], want["cand"], got["stats"], want["stats"]))
    assert not failed, failed
