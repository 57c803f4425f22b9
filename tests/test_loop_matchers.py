"""Loop closing's four matchers on the GPU -- ORBmatcher::SearchByBoW(pKF1, pKF2, ...), SearchBySim3, SearchByProjection(pKF, Scw,
...) and Fuse(pKF, Scw, ...) (pilotguru_amd/csrc/loop.hip; include/pgorb.h) -- against the plain sequential reference (tests/loop_reference.py) on constructed
cases (tests/loop_cases.py).  The contract is equality, not a tolerance."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_cases as LC  # noqa: E402
import loop_reference as LR  # noqa: E402

EDGES = ["bad", "already_found", "behind", "outside_image", "on_max_bound", "on_depth_min", "on_depth_max", "depth_low", "depth_high",
         "angle", "octave_above", "tie", "dist_50", "dist_51", "no_match", "no_candidate", "matched", "taken_skipped", "added",
         "replace_requested", "replace_self", "kf_point_bad"]
RUN = {3: LC.run_ref3, 4: LC.run_ref4}


@pytest.fixture(scope="module")
def cases():
    return LC.edge_cases()


def test_loop_symbols_and_null_context():
    """Fails without the feature: the eight entry points exist and refuse a NULL context."""
    from pilotguru_amd import _lib
    L = _lib.lib()
    names = ("pgorb_search_by_projection_sim3", "pgorb_search_by_projection_sim3_batch_device", "pgorb_fuse_sim3",
             "pgorb_fuse_sim3_batch_device", "pgorb_search_by_sim3", "pgorb_search_by_sim3_batch_device", "pgorb_search_by_bow_keyframes",
             "pgorb_search_by_bow_keyframes_batch_device")
    for name in names:
        assert name in _lib.SYMBOLS and hasattr(L, name)
    b = (0.0, 640.0, 0.0, 480.0)
    assert L.pgorb_search_by_projection_sim3(None, None, None, 0, None, *b, None, 0, None, None, None, 0, None, 10, None, None) == -1
    assert L.pgorb_fuse_sim3(None, None, None, 0, None, *b, None, 0, None, None, None, 0, None, 4.0, *([None] * 5)) == -1
    assert L.pgorb_search_by_projection_sim3_batch_device(None, None, None, None, 1, None, None, None, 1, None, *b, None, 0, None, None,
                                                          None, 1, None, None, 10, None, None, None, None) == -1
    assert L.pgorb_fuse_sim3_batch_device(None, None, None, None, 1, None, None, None, 1, None, *b, None, 0, None, None, None, 1, None,
                                          None, 4.0, *([None] * 7)) == -1


    assert L.pgorb_search_by_sim3(None, *([None, None, 0, None, None, None] * 2), *b, 0, None, None, None, None, 7.5, None) == -1
    assert L.pgorb_search_by_sim3_batch_device(None, None, None, None, 1, None, None, None, None, 1, None, *b, None, 0, None, None, None,
                                               None, None, None, 7.5, None, None, None) == -1
    assert L.pgorb_search_by_bow_keyframes(None, *([None, None, None, 0, None, None, None, 0] * 2), 0.75, 1, None) == -1
    assert L.pgorb_search_by_bow_keyframes_batch_device(None, None, None, None, 1, None, None, None, None, None, None, 1, None, None, 0.75,
                                                        1, None, None, None) == -1


EDGES1 = ["common_node", "big_node", "invalid1", "invalid2", "matched2_skipped", "dist_50", "ratio_failed", "rotation_dropped"]


@pytest.fixture(scope="module")
def bows():
    return LC.bow_cases()


def test_bow_keyframe_cases_reach_every_edge_and_catch_every_mutant(bows):
    hits = collections.Counter()
    want = [LC.run_ref1(c, hits=hits) for c in bows]
    missing = [e for e in EDGES1 if not hits[e]]
    assert not missing, (missing, dict(hits))
    by_name = {c.name: w for c, w in zip(bows, want)}
    assert by_name["no_common_node"][0] == 0 and by_name["one_big_node"][0] > 0
    for name, rules in LR.MUTANTS1.items():
        assert any(not LC.same(w, LC.run_ref1(c, rules)) for w, c in zip(want, bows)), name


def test_mirror_rejects_malformed_feature_vectors(bows):
    import pilotguru_amd as pg
    c = bows[0]
    m = pg.ORBmatcher(LC.NNRATIO, True)
    d, a, v, fv = c.k1
    ok = [None, d, a, v, fv, c.k2[0], c.k2[1], c.k2[2], c.k2[3]]
    bad_fvs = [(fv[0], fv[1][:-1], fv[2]), (fv[0], fv[1], np.full_like(fv[2], len(a))), (fv[0][::-1].copy(), fv[1], fv[2]),
               (fv[0], fv[1][::-1].copy(), fv[2])]
    for i, b in enumerate(bad_fvs):
        with pytest.raises(ValueError):
            m.SearchByBoWKeyFrames(*(ok[:4] + [b] + ok[5:]))
            pytest.fail("FeatureVector %d was accepted" % i)
    for args in (ok[:1] + [d[:-1]] + ok[2:], ok[:3] + [v[:-1]] + ok[4:], ok[:7] + [c.k2[2][:-1]] + ok[8:]):
        with pytest.raises(ValueError):
            m.SearchByBoWKeyFrames(*args)


EDGES2 = ["already1", "already2", "bad", "behind", "outside_image", "depth", "no_candidate", "tie", "between_thresholds", "disagree"]


@pytest.fixture(scope="module")
def pairs():
    return LC.pair_cases()


def test_sim3_cases_reach_every_edge_and_catch_every_mutant(pairs):
    hits = collections.Counter()
    want = [LC.run_ref2(c, hits=hits) for c in pairs]
    missing = [e for e in EDGES2 if not hits[e]]
    assert not missing, (missing, dict(hits))
    assert all(w[0] >= 1 for w, c in zip(want, pairs) if len(c.slots2) > 20), [w[0] for w in want]      # the scenes do produce agreed pairs
    for name, rules in LR.MUTANTS2.items():
        assert any(not LC.same(w, LC.run_ref2(c, rules)) for w, c in zip(want, pairs)), name


def test_cases_reach_every_edge(cases):
    hits = collections.Counter()
    for c in cases:
        LC.run_ref3(c, hits=hits)
        LC.run_ref4(c, hits=hits)
    missing = [e for e in EDGES if not hits[e]]
    assert not missing, (missing, dict(hits))


def test_every_rule_mutant_is_caught(cases):
    """Every mutant changes the result of at least one case, in each routine it belongs to.  None is exempt: every rule of
    loop_reference.Rules is separated by some input here."""
    for which, skip in ((3, LR.ONLY_4), (4, LR.ONLY_3)):
        want = [RUN[which](c) for c in cases]
        for name, rules in LR.MUTANTS.items():
            if name in skip:
                continue
            assert any(not LC.same(w, RUN[which](c, rules)) for w, c in zip(want, cases)), (which, name)


@pytest.mark.parametrize("seed", range(40))
def test_two_pass_decompositions_equal_the_sequential_routines(seed):
    """The kernels' specification: lists without the candidates above TH_LOW, decided in query order (3), and matching from the
    entry state with the first matched query per slot as the one that adds (4), equal the reference run query after query."""
    c = LC.collision_case(seed)
    assert LC.same(LC.run_ref3(c), LC.run_two_pass3(c))
    assert LC.same(LC.run_ref4(c), LC.run_two_pass4(c))


@pytest.mark.parametrize("seed", range(40))
def test_rounds_of_independent_queries_equal_the_sequence(seed):
    """k_ps3_decide's readiness rule on random lists with heavy overlap, without a GPU: the same assignments as the walk in query
    order, in fewer rounds than queries."""
    rng = np.random.RandomState(seed)
    nk, nq = 12 + seed % 7, 60
    lists = []
    for q in range(nq):
        ks = rng.choice(nk, int(rng.randint(0, 5)), replace=False)
        lists.append([(int(rng.randint(0, 51)), pos, int(k)) for pos, k in enumerate(ks)])
    taken0 = [bool(rng.rand() < 0.15) for _ in range(nk)]
    taken, want = list(taken0), {}
    for q, lst in enumerate(lists):
        free = [e for e in lst if not taken[e[2]]]
        if free:
            taken[min(free)[2]] = True
            want[min(free)[2]] = q
    got, rounds = LR.decide_in_rounds(lists, taken0)
    assert got == want and rounds <= nq


def test_collision_cases_hold_contests_chains_and_repeats():
    contested, chain, rep3, rep4 = 0, 0, False, False
    for seed in range(40):
        c = LC.collision_case(seed)
        kf, _, matched, q = c.build()
        # 3: for every keypoint, the queries that list it within TH_LOW on entry
        n3, asg, _ = LC.run_ref3(c)
        want = collections.Counter()
        for mp in q:
            if mp.bad or any(m is mp for m in matched):
                continue
            fr = LR.front(kf, mp, c.th)
            if fr is None:
                continue
            dmp = int.from_bytes(mp.desc.tobytes(), "little")
            for idx in fr[3]:
                if LR._dist(dmp, kf.dint[idx]) <= LR.TH_LOW:
                    want[idx] += 1
        contested = max([contested] + [want[i] for i in range(len(asg)) if asg[i] >= 0])
        taken_by = [c.queries[a] for a in asg if a >= 0]
        rep3 |= len(set(taken_by)) < len(taken_by)                            # one point written into two keypoints
        n4, act, rep, bi = LC.run_ref4(c)[:4]
        per = collections.Counter(int(b) for a, b in zip(act, bi) if a in (LR.ADDED, LR.REPLACE_REQUESTED, LR.KF_POINT_BAD))
        chain = max([chain] + list(per.values()))
        rep4 |= any(a == LR.REPLACE_REQUESTED and r == c.queries[i] for i, (a, r) in enumerate(zip(act, rep)))
    assert contested >= 4 and chain >= 3 and rep3 and rep4, (contested, chain, rep3, rep4)


def test_python_mirror_rejects_bad_inputs():
    import pilotguru_amd as pg
    c = LC.collision_case(0)
    kid, k, d, P, b = c.kf
    K = LC.FC.MC.KeyFrameArrays(None, k, d)
    T = LC.table(c.points)
    q = np.array(c.queries, np.int32)
    m = pg.ORBmatcher()
    for f in (m.SearchByProjectionSim3, m.FuseSim3):
        bad_inputs = [
            lambda: f(K, P, c.slots[:-1], T, q, bounds=b),                      # slots length
            lambda: f(K, P, c.slots, T, np.append(q, T.n), bounds=b),           # query out of range
            lambda: f(K, P, c.slots, T, np.append(q, -1), bounds=b),            # a NULL query
            lambda: f(K, P, np.where(c.slots >= 0, 10 ** 6, -1), T, q, bounds=b),
            lambda: f(K, P, c.slots, T, q, th=0, bounds=b),
            lambda: f(K, P, c.slots, T, q, bounds=b[:3]),
            lambda: f(LC.FC.MC.KeyFrameArrays(None, k, d[:-1]), P, c.slots, T, q, bounds=b),
        ]
        for i, g in enumerate(bad_inputs):
            with pytest.raises(ValueError):
                g()
                pytest.fail("input %d was accepted" % i)
    with pytest.raises(ValueError, match="FuseSim3"):
        m.FuseSim3(K, P, c.slots, T, np.append(q, T.n), bounds=b)             # the message names the routine
    with pytest.raises(ValueError):
        m.SearchByProjectionSim3(K, P, c.slots, T, q, th=2.5, bounds=b)        # th is an int there
    pc = LC.pair_case(4, npts=5)
    K1, K2 = (LC.FC.MC.KeyFrameArrays(None, k, d) for k, d, _ in (pc.kf1, pc.kf2))
    T2 = LC.table(pc.points)
    ok = dict(KF1=K1, KF2=K2, pose1=pc.kf1[2], pose2=pc.kf2[2], kf_point1=pc.slots1, kf_point2=pc.slots2, table=T2, sim3=pc.sim3,
              already1=pc.already1, already2=pc.already2, bounds=LC.BOUNDS)
    for bad in (dict(kf_point1=pc.slots1[:-1]), dict(kf_point2=np.full(len(pc.slots2), T2.n, np.int32)), dict(already1=pc.already1[:-1]),
                dict(th=0.0), dict(bounds=(0.0, 1.0)), dict(sim3=np.zeros(2, pg.SIM3_DTYPE))):
        with pytest.raises(ValueError):
            m.SearchBySim3(**dict(ok, **bad))
    for S in (np.eye(3), np.zeros((4, 4))):
        with pytest.raises(ValueError):
            pg.sim3_pose(S, 500.0, 500.0, 320.0, 240.0)


def test_sim3_pose_decomposes_a_scaled_pose():
    import pilotguru_amd as pg
    R = LC.FC.MC.rot(0.1, -0.2, 0.3)
    t = np.array([0.3, -0.1, 0.7])
    S = np.eye(4)
    S[:3, :3], S[:3, 3] = 1.7 * R, 1.7 * t
    P = pg.sim3_pose(S.astype(np.float32), 500.0, 510.0, 320.0, 240.0)
    T = np.asarray(P["Tcw"], np.float64).reshape(3, 4)
    assert np.allclose(T[:, :3], R, atol=1e-6) and np.allclose(T[:, 3], t, atol=1e-6)
    assert np.allclose(P["Ow"], -R.T @ t, atol=1e-6) and float(P["fy"]) == 510.0


# ---------------------------------------------------------------- GPU
def _extractor(w=640, h=480):
    import pilotguru_amd as pg
    return pg.ORBextractor(2000, LC.FC.MC.SCALE, LC.FC.NLEVELS, 20, 7, max_width=w, max_height=h)


def _big_cases():
    rng = np.random.RandomState(77)
    return [LC.dense_window_case(rng), LC.chain_case(rng)]


@pytest.mark.gpu
@pytest.mark.parametrize("which", [3, 4])
def test_gpu_single_calls_equal_reference(cases, which):
    ext = _extractor()
    run = LC.run_gpu3 if which == 3 else LC.run_gpu4
    for c in cases + [LC.collision_case(s) for s in range(12)] + _big_cases():
        want, got = RUN[which](c), run(c, ext)
        assert LC.same(want, got), (c.name, want, got)


def test_big_cases_are_what_they_claim():
    dense, chain = _big_cases()
    kf, _, matched, q = dense.build()
    fr = LR.front(kf, q[0], dense.th)
    dmp = int.from_bytes(q[0].desc.tobytes(), "little")
    assert sum(LR._dist(dmp, kf.dint[i]) <= LR.TH_LOW for i in fr[3]) > 64
    n, asg, _ = LC.run_ref3(chain)
    assert n >= 6 and [int(a) for a in asg[:n]] == list(range(n))              # query k takes keypoint k: its better ones are taken


@pytest.mark.gpu
@pytest.mark.parametrize("which", [3, 4])
def test_gpu_batched_forms_equal_reference(cases, which):
    ext = _extractor()
    th3 = [c for c in cases if c.th == 3]
    batch = [LC.wide_case(3, 257)] + th3 + [LC.collision_case(s) for s in range(6)] + [LC.wide_case(4, 40), LC.chain_case(np.random.RandomState(5))]
    assert {"no_queries", "no_keypoints"} <= {c.name for c in batch}
    out = LC.run_gpu_batched(batch, ext, which, qcap=320)
    for c, got in zip(batch, out):
        assert LC.same(RUN[which](c), got[:-1]), c.name
        assert np.all(got[-1] == LC.SENTINEL), (c.name, "wrote past the entries in use")
    dense = [LC.dense_window_case(np.random.RandomState(s)) for s in (1, 2, 3)]
    for c, got in zip(dense, LC.run_gpu_batched(dense, ext, which)):
        assert LC.same(RUN[which](c), got[:-1]), c.name


@pytest.mark.gpu
def test_gpu_search_by_sim3_equals_reference(pairs):
    ext = _extractor()
    for c in pairs:
        want, got = LC.run_ref2(c), LC.run_gpu2(c, ext)
        assert LC.same(want, got), (c.name, want, got)
    for c, got in zip(pairs, LC.run_gpu2_batched(pairs, ext)):
        assert LC.same(LC.run_ref2(c), got[:2]), c.name
        assert np.all(got[2] == LC.SENTINEL), (c.name, "wrote past n1")


@pytest.mark.gpu
def test_gpu_search_by_bow_keyframes_equals_reference(bows):
    """Single calls and one batched call, with a node above 64 features on each side and a pair without a common node."""
    ext = _extractor()
    for c in bows:
        want, got = LC.run_ref1(c), LC.run_gpu1(c, ext)
        assert LC.same(want, got), (c.name, want, got)
    for c, got in zip(bows, LC.run_gpu1_batched(bows, ext)):
        assert LC.same(LC.run_ref1(c), got), c.name


@pytest.mark.gpu
def test_gpu_compute_sim3_chain_equals_reference():
    """ComputeSim3's matcher chain on one pair of constructed key frames: 1 -> masks -> 2 -> 3, each step fed by the one before."""
    ext = _extractor()
    c, b, Pscw = LC.chain_inputs()
    want = LC.run_chain(c, b, Pscw, LC.run_ref1, LC.run_ref2, LC.run_ref3)
    got = LC.run_chain(c, b, Pscw, lambda x: LC.run_gpu1(x, ext), lambda x: LC.run_gpu2(x, ext), lambda x: LC.run_gpu3(x, ext))
    assert all(np.array_equal(np.asarray(w), np.asarray(g)) for w, g in zip(want, got)), (want, got)
    assert (want[0] >= 0).sum() > 0 and want[2] >= 0


@pytest.mark.gpu
def test_gpu_routines_interleaved_on_one_context_repeat_their_results(cases, pairs, bows):
    """Shared arenas: each of the four routines twice on one context with the others in between."""
    ext = _extractor()
    cs = [LC.wide_case(9, 300), LC.collision_case(3)]
    runs = [[(LC.run_gpu1(bows[i], ext), LC.run_gpu2(pairs[i], ext), LC.run_gpu3(c, ext), LC.run_gpu4(c, ext)) for i, c in enumerate(cs)]
            for _ in range(2)]
    for i, c in enumerate(cs):
        want = (LC.run_ref1(bows[i]), LC.run_ref2(pairs[i]), LC.run_ref3(c), LC.run_ref4(c))
        for a, b_, w in zip(runs[0][i], runs[1][i], want):
            assert LC.same(a, b_) and LC.same(a, w), c.name
