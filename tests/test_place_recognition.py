"""Place recognition (pilotguru_amd/csrc/place.hip: k_bow_vectors, k_bow_score_pairs, k_place_overlap, k_place_decide; include/
pgorb.h) against the plain sequential KeyFrameDatabase of tests/place_reference.py on the cases of tests/place_cases.py.  Every
comparison is exact: integers as integers, floats and doubles as bit patterns."""
import collections
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import place_cases as PC  # noqa: E402
import place_reference as PR  # noqa: E402
import vocab_cases as VC  # noqa: E402

NEW_SYMBOLS = ("pgorb_bow_vectors_batch_device", "pgorb_bow_score_l1_batch_device", "pgorb_detect_relocalization_candidates",
               "pgorb_detect_relocalization_candidates_batch_device", "pgorb_detect_loop_candidates",
               "pgorb_detect_loop_candidates_batch_device")
EDGES = ["count_equals_min", "no_sharing", "empty_query", "neighbour_not_in_db", "stale_changes_candidates", "stale_changes_best",
         "neighbour_tie", "acc_equals_retain", "duplicate_best", "connected_excluded", "si_equals_min_score", "below_min_contributes",
         "best_stays_min_score", "erase_changes_order"]


@pytest.fixture(scope="module")
def cases():
    return PC.edge_cases()


@pytest.fixture(scope="module")
def wants(cases):
    return [PC.run_reference(c) for c in cases]


# ---- CPU: the boundary, the cases and the reference themselves ------------------------------------------------------------------

def test_place_symbols_and_null_context():
    from pilotguru_amd import _lib
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    N = None
    assert L.pgorb_bow_vectors_batch_device(N, N, N, N, 1, 1, N, N, N, N) == -1
    assert L.pgorb_bow_score_l1_batch_device(N, N, N, N, 1, 1, N, N, 0, N, N) == -1
    assert L.pgorb_detect_relocalization_candidates_batch_device(N, N, N, N, 1, 1, N, N, N, 0, N, N, 0, N, N, N, N, N) == -1
    assert L.pgorb_detect_loop_candidates_batch_device(N, N, N, N, 1, 1, N, N, N, 0, N, N, N, 0, N, 0, N, N, N, N, N) == -1
    assert L.pgorb_detect_relocalization_candidates(N, 1, N, N, N, N, N, N, 0, N, N, 0, N, N) == -1
    assert L.pgorb_detect_loop_candidates(N, 1, N, N, N, N, N, N, 0, 0.0, N, 0, N, 0, N, N, N) == -1


def test_cases_reach_every_edge(cases):
    hits = collections.Counter()
    for c in cases:
        PC.run_reference(c, hits=hits)
        PC.extra_edges(c, hits)
    missing = [e for e in EDGES if not hits[e]]
    assert not missing, (missing, dict(hits))
    loop_hits = collections.Counter()
    for c in cases:
        if c.form == "loop":
            PC.run_reference(c, hits=loop_hits)
    assert all(loop_hits[e] for e in ("connected_excluded", "si_equals_min_score", "below_min_contributes", "best_stays_min_score",
                                      "count_equals_min", "duplicate_best")), dict(loop_hits)


def test_every_rule_mutant_is_caught(cases, wants):
    """Every reading of the issue's list changes what at least one case returns -- except `0.8 in double`, which cannot at any size
    a test can hold: int(n*0.8f) == int(n*0.8) for every count n below 5 242 881 (checked here exhaustively), five times the words
    of the largest ORB vocabulary and far past the 65 536-frame and 8192-feature limits of the calls."""
    survivors = [name for name, rules in PR.MUTANTS.items()
                 if name not in PR.EQUIVALENT and all(PC.same(w, PC.run_reference(c, rules)) for w, c in zip(wants, cases))]
    assert not survivors, survivors
    assert PR.EQUIVALENT == ("factor=double",)
    m = np.arange(0, 1 << 23, dtype=np.int64)
    as_float = (m.astype(np.float32) * np.float32(0.8)).astype(np.int64)
    as_double = (m.astype(np.float64) * 0.8).astype(np.int64)
    assert int(np.nonzero(as_float != as_double)[0][0]) == 5242881


@pytest.mark.parametrize("seed", range(40))
def test_closed_form_sharing_order(seed):
    """The kernels' specification: lKFsSharingWords is the members sharing a word, sorted by (smallest common word, add position),
    with the number of common words -- equal to the inverted-file walk, erasures and re-adds included, in both forms."""
    c = PC.random_case(seed)
    b = PC.build(c)
    members = [b.objs[i] for i, member in b.rows if member]
    if c.form == "reloc":
        res = PR.detect_relocalization_candidates(b.db, b.qobj.id, b.qobj.bow)
        got = [(kf, kf.mnRelocWords) for kf in res.sharing]
        want = PR.sharing_closed_form(members, b.qobj.bow)
    else:
        res = PR.detect_loop_candidates(b.db, b.qobj, c.min_score)
        got = [(kf, kf.mnLoopWords) for kf in res.sharing]
        want = PR.sharing_closed_form(members, b.qobj.bow, b.qobj.connected)
    assert [(kf.id, n) for kf, n in got] == [(kf.id, n) for kf, n in want]
    assert len(got) >= 3


def test_random_cases_erase_and_reorder():
    moved = 0
    for seed in range(40):
        hits = collections.Counter()
        PC.extra_edges(PC.random_case(seed), hits)
        moved += hits["erase_changes_order"]
    assert moved >= 10, moved


def test_python_mirror_rejects_bad_inputs():
    import pilotguru_amd as pg
    db = pg.KeyFrameDatabase(None)
    good = (np.array([1, 4, 9], np.uint32), np.array([0.5, 0.25, 0.25]))
    db.add("a", good, neighbours=["b"])
    db.add("b", good)
    bad_inputs = [
        lambda: db.add("c", (np.array([4, 1], np.uint32), np.array([0.5, 0.5]))),            # unsorted word ids
        lambda: db.add("c", (np.array([4, 4], np.uint32), np.array([0.5, 0.5]))),            # a repeated word id
        lambda: db.add("c", (np.array([1, 4], np.uint32), np.array([0.5]))),                 # lengths differ
        lambda: db.add("c", 5),                                                              # not a BowVector
        lambda: db.add("a", good),                                                           # already a member
        lambda: db.add("c", good, neighbours=list("abcdefghijk")),                           # eleven neighbours
        lambda: db.set_neighbours("a", range(11)),
        lambda: db.erase("zz"),                                                              # never added
        lambda: db.DetectRelocalizationCandidates((np.array([3, 2], np.uint32), np.array([0.5, 0.5]))),
        lambda: db.DetectLoopCandidates((np.array([3, 3], np.uint32), np.array([0.5, 0.5])), 0.1),
        lambda: db.DetectLoopCandidates(good, 0.1, connected=["nobody"]),
        lambda: db.score(good, (np.array([2, 1], np.uint32), np.array([0.5, 0.5]))),
    ]
    for i, f in enumerate(bad_inputs):
        with pytest.raises(ValueError):
            f()
            pytest.fail("input %d was accepted" % i)
    db.erase("a")
    with pytest.raises(ValueError):
        db.erase("a")                                                                        # erased twice
    db.add("a", good)                                                                        # ... and may come back
    assert len(db) == 2 and db.score(good, good) == 1.0


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    e = pg.ORBextractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240, max_batch=2)
    yield e
    e.close()


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _p(a):
    return C.c_void_p(a.ctypes.data)


def gpu_single(ext, t, form, ccap=64):
    """One case through the single host call: the outputs in the shape of PC.expected."""
    n = t["nrows"]
    cand, common, stats = np.full(max(ccap, 1), -7, np.int32), np.full(n, -7, np.int32), np.full(3, -7, np.int32)
    L = ext._L
    if form == "reloc":
        score = t["state"].copy()
        rc = L.pgorb_detect_relocalization_candidates(ext._h, n, _p(t["bow_start"]), _p(t["bow_id"]), _p(t["bow_val"]), _p(t["in_db"]),
                                                      _p(t["neigh_start"]), _p(t["neigh"]), t["query"], _p(score), _p(cand), ccap,
                                                      _p(common), _p(stats))
    else:
        score = np.full(n, -7, np.float32)
        rc = L.pgorb_detect_loop_candidates(ext._h, n, _p(t["bow_start"]), _p(t["bow_id"]), _p(t["bow_val"]), _p(t["in_db"]),
                                            _p(t["neigh_start"]), _p(t["neigh"]), t["query"], float(t["min_score"]), _p(t["conn"]),
                                            len(t["conn"]), _p(cand), ccap, _p(common), _p(score), _p(stats))
    ext._check(rc)
    assert (cand[min(rc, ccap):] == -7).all()
    return dict(cand=cand[:min(rc, ccap)].tolist(), ncand=rc, common=common, score=score, stats=tuple(int(x) for x in stats))


def merged(tables, cap):
    """Several cases as ONE table: rows one after another, every case's words moved into a range of its own."""
    N = sum(t["nrows"] for t in tables)
    M = dict(N=N, cap=cap, id=np.full((N, cap), 0xDEADBEEF, np.uint32), val=np.full((N, cap), np.nan), nbow=np.zeros(N, np.int32),
             in_db=np.zeros(N, np.uint8), neigh=np.full((N, PC.NEIGH), -1, np.int32), state=np.zeros(N, np.float32), query=[], min_score=[],
             conn_start=[0], conn=[], base=[])
    base = 0
    for k, t in enumerate(tables):
        M["base"].append(base)
        for r in range(t["nrows"]):
            a, e = t["bow_start"][r], t["bow_start"][r + 1]
            M["id"][base + r, :e - a] = t["bow_id"][a:e] + np.uint32(100000 * k)
            M["val"][base + r, :e - a] = t["bow_val"][a:e]
            M["nbow"][base + r] = e - a
            a, e = t["neigh_start"][r], t["neigh_start"][r + 1]
            M["neigh"][base + r, :e - a] = t["neigh"][a:e] + base
            if e - a < PC.NEIGH:
                M["neigh"][base + r, PC.NEIGH - 1] = N + 5 + r                     # out of range: skipped like -1
        M["in_db"][base:base + t["nrows"]] = t["in_db"]
        M["state"][base:base + t["nrows"]] = t["state"]
        M["query"].append(base + t["query"])
        M["min_score"].append(t["min_score"])
        M["conn"].extend((t["conn"] + base).tolist())
        M["conn_start"].append(len(M["conn"]))
        base += t["nrows"]
    return M


def gpu_batch(ext, M, form, ccap, state=None):
    """All queries of a merged table in one batched call; rows of guard values around every output."""
    import torch
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()
    N, cap, nq = M["N"], M["cap"], len(M["query"])
    ids, val, nbow = dev(M["id"].view(np.int32), np.int32), dev(M["val"], np.float64), dev(M["nbow"], np.int32)
    in_db, neigh, query = dev(M["in_db"], np.uint8), dev(M["neigh"], np.int32), dev(M["query"], np.int32)
    g = 0x5EC0DE55
    cand = torch.full((nq + 2, max(ccap, 1)), g, dtype=torch.int32, device="cuda")
    ncand = torch.full((nq + 2,), g, dtype=torch.int32, device="cuda")
    common = torch.full((nq + 2, N), g, dtype=torch.int32, device="cuda")
    score = torch.full((nq + 2, N), 123.0, dtype=torch.float32, device="cuda")
    stats = torch.full((nq + 2, 3), g, dtype=torch.int32, device="cuda")
    L = ext._L
    if form == "reloc":
        st = dev(M["state"] if state is None else state, np.float32)
        rc = L.pgorb_detect_relocalization_candidates_batch_device(ext._h, _tp(ids), _tp(val), _tp(nbow), N, cap, _tp(in_db), _tp(neigh),
                                                                   _tp(query), nq, _tp(st), _tp(cand[1]), ccap, _tp(ncand[1:]),
                                                                   _tp(common[1]), _tp(score[1]), _tp(stats[1]), _stream())
    else:
        ms, cs = dev(M["min_score"], np.float32), dev(M["conn_start"], np.int32)
        cn = dev(M["conn"] if len(M["conn"]) else [0], np.int32)
        rc = L.pgorb_detect_loop_candidates_batch_device(ext._h, _tp(ids), _tp(val), _tp(nbow), N, cap, _tp(in_db), _tp(neigh), _tp(query),
                                                         nq, _tp(ms), _tp(cs), _tp(cn), len(M["conn"]), _tp(cand[1]), ccap, _tp(ncand[1:]),
                                                         _tp(common[1]), _tp(score[1]), _tp(stats[1]), _stream())
    ext._check(rc)
    torch.cuda.synchronize()
    cand, ncand, common, score, stats = [x.cpu().numpy() for x in (cand, ncand, common, score, stats)]
    for a in (cand, common, stats):
        assert (a[0] == g).all() and (a[-1] == g).all()
    assert ncand[0] == g and ncand[-1] == g and (score[0] == 123.0).all() and (score[-1] == 123.0).all()
    out = []
    for q in range(nq):
        k = int(ncand[1 + q])
        assert (cand[1 + q, min(k, ccap):] == g).all()
        out.append(dict(cand=cand[1 + q, :min(k, ccap)].tolist(), ncand=k, common=common[1 + q], score=score[1 + q],
                        stats=tuple(int(x) for x in stats[1 + q])))
    return out


def widen(want, M, k, form):
    """Case k's expectation over the merged table's rows."""
    base, n = M["base"][k], len(want["common"])
    common = np.zeros(M["N"], np.int32)
    common[base:base + n] = want["common"]
    score = M["state"].copy() if form == "reloc" else np.zeros(M["N"], np.float32)
    score[base:base + n] = want["score"]
    return dict(cand=[r + base for r in want["cand"]], common=common, score=score, stats=want["stats"])


def differs(got, want):
    return [f for f in ("cand", "stats") if list(got[f]) != list(want[f])] + \
        [f for f in ("common", "score") if got[f].tobytes() != want[f].tobytes()]


def check_cases(ext, cases, wants, cap, ccap=64, single=True):
    failed = {}
    for form in ("reloc", "loop"):
        sel = [(c, w) for c, w in zip(cases, wants) if c.form == form]
        if not sel:
            continue
        tabs = [PC.table(PC.build(c)) for c, _ in sel]
        if single:
            for (c, w), t in zip(sel, tabs):
                got = gpu_single(ext, t, form, ccap)
                bad = differs(got, w)
                if bad or got["ncand"] != len(w["cand"]):
                    failed[c.name + "/single"] = (bad, got["cand"], w["cand"], got["stats"], w["stats"])
        M = merged(tabs, cap)
        for k, ((c, w), got) in enumerate(zip(sel, gpu_batch(ext, M, form, ccap))):
            ww = widen(w, M, k, form)
            bad = differs(got, ww)
            if bad or got["ncand"] != len(w["cand"]):
                failed[c.name + "/batch"] = (bad, got["cand"], ww["cand"], got["stats"], ww["stats"])
    return failed


@pytest.mark.gpu
def test_gpu_edge_cases_both_forms_single_and_batch(ext, cases, wants):
    """Every constructed edge plus random databases with erasures (12-40 key frames of 3-40 words, cap 64), each through the single
    host call and all together as one batch per form: candidates, counts, common words, stored scores and stats."""
    extra = [PC.random_case(s) for s in range(6)]
    all_cases = list(cases) + extra
    all_wants = list(wants) + [PC.run_reference(c) for c in extra]
    assert sum(len(w["cand"]) for w in all_wants) > 20
    failed = check_cases(ext, all_cases, all_wants, cap=64)
    assert not failed, failed


@pytest.mark.gpu
def test_gpu_candidate_capacity_is_respected(ext, cases, wants):
    """ccap below the number of candidates: the full count comes back, only the first ccap are written."""
    k = [c.name for c in cases].index("duplicate_best")
    t = PC.table(PC.build(cases[k]))
    got = gpu_single(ext, t, "reloc", ccap=1)
    assert got["ncand"] == 2 and got["cand"] == wants[k]["cand"][:1]
    got = gpu_batch(ext, merged([t], 64), "reloc", 0)[0]
    assert got["ncand"] == 2 and got["cand"] == []


@pytest.mark.gpu
def test_gpu_long_vectors(ext):
    """A 300-word query against 300-word key frames: slices across lanes, several ballot trips, running sums of ~225 terms."""
    cs = [PC.long_vectors_case("reloc"), PC.long_vectors_case("loop")]
    ws = [PC.run_reference(c) for c in cs]
    assert all(w["stats"][1] > 192 and w["stats"][2] >= 2 for w in ws), [w["stats"] for w in ws]
    failed = check_cases(ext, cs, ws, cap=320)
    assert not failed, failed


@pytest.mark.gpu
def test_gpu_many_key_frames(ext):
    """1100 key frames of 2-4 words: the sharing list, the scored set and the candidates are longer than one workgroup."""
    cs = [PC.many_key_frames_case("reloc"), PC.many_key_frames_case("loop")]
    ws = [PC.run_reference(c) for c in cs]
    assert ws[0]["stats"][0] > 1024 and len(ws[0]["cand"]) > 64, (ws[0]["stats"], len(ws[0]["cand"]))
    failed = check_cases(ext, cs, ws, cap=64, ccap=1200)
    assert not failed, failed


@pytest.mark.gpu
def test_gpu_chain_of_six_queries(ext):
    """Six relocalisation queries in sequence: every query's d_score row is the next call's state, as the reference's key frames
    carry mRelocScore from one query to the next."""
    base, queries = PC.chain_case()
    b = PC.build(base)
    t = PC.table(b)
    state = t["state"].copy()
    stale = collections.Counter()
    for k, q in enumerate(queries):
        qbow = PC._bow(q)
        res = PR.detect_relocalization_candidates(b.db, 2000 + k, qbow, hits=stale)
        b.qobj.id, b.qobj.bow = 2000 + k, [(w, np.float64(v)) for w, v in qbow]
        want = PC.expected(b, res, state)
        tk = PC.table(b)
        M = merged([tk], 64)
        got = gpu_batch(ext, M, "reloc", 64, state=state)[0]
        assert not differs(got, want), (k, differs(got, want), got["cand"], want["cand"])
        state = got["score"].copy()
    assert stale["stale_read"] > 10


def _host_bow(word, weight, weighting):
    from pilotguru_amd import vocab as V
    (bid, bval), _ = V.bow_vectors(word, weight, np.zeros(len(word), np.uint32), 0, weighting)
    return bid, bval


def _gpu_bow_vectors(ext, word, weight, n, cap):
    import torch
    F = len(n)
    g = 0x5EC0DE55
    bid = torch.full((F + 2, cap), g, dtype=torch.int32, device="cuda")
    bval = torch.full((F + 2, cap), -5.0, dtype=torch.float64, device="cuda")
    nb = torch.full((F + 2,), g, dtype=torch.int32, device="cuda")
    ext._check(ext._L.pgorb_bow_vectors_batch_device(ext._h, _tp(word), _tp(weight), _tp(n), F, cap, _tp(bid[1]), _tp(bval[1]), _tp(nb[1:]),
                                                     _stream()))
    torch.cuda.synchronize()
    bid, bval, nb = bid.cpu().numpy(), bval.cpu().numpy(), nb.cpu().numpy()
    assert (bid[0] == g).all() and (bid[-1] == g).all() and (bval[0] == -5.0).all() and (bval[-1] == -5.0).all() and nb[0] == g and nb[-1] == g
    return bid[1:-1].view(np.uint32), bval[1:-1], nb[1:-1]


@pytest.mark.gpu
def test_gpu_bow_vectors_equal_the_host(ext, tmp_path):
    """pgorb_bow_vectors_batch_device == pgorb_bow_vectors byte for byte on irregular trees (TF_IDF and TF): frames with repeated
    words, stopped words, an empty frame, a full-cap frame; then a 3000-feature frame (several ranks per thread)."""
    import torch
    from pilotguru_amd import vocab as V
    trees = [VC.random_tree(1, 10, 6), VC.random_tree(3, 7, 5), VC.random_tree(4, 20, 3)._replace(weighting=1)]
    cap = 257
    seen_stop = seen_repeat = 0
    for ti, tree in enumerate(trees):
        path = VC.write_text(tree, os.path.join(str(tmp_path), "t%d.txt" % ti))
        V.ORBVocabulary(text_file=path).upload(ext)
        rng = np.random.RandomState(20 + ti)
        pool = VC.node_queries(tree, rng, 30, 60)
        nh = np.array([cap, 0, 100, 63, 129], np.int32)
        desc = rng.randint(0, 256, (len(nh), cap, 32)).astype(np.uint8)
        for f, n in enumerate(nh):
            src = pool if f != 2 else pool[rng.choice(len(pool), 7, replace=False)]
            desc[f, :n] = src[rng.randint(0, len(src), n)]
        d_desc, d_n = torch.from_numpy(desc).cuda(), torch.from_numpy(nh).cuda()
        word = torch.empty((len(nh), cap), dtype=torch.int32, device="cuda")
        wt = torch.empty((len(nh), cap), dtype=torch.float64, device="cuda")
        node = torch.empty((len(nh), cap), dtype=torch.int32, device="cuda")
        ext._check(ext._L.pgorb_bow_transform_device(ext._h, _tp(d_desc), len(nh) * cap, 2, _tp(word), _tp(wt), _tp(node), _stream()))
        bid, bval, nb = _gpu_bow_vectors(ext, word, wt, d_n, cap)
        hw, hwt = word.cpu().numpy().view(np.uint32), wt.cpu().numpy()
        for f, n in enumerate(nh):
            wid, wval = _host_bow(hw[f, :n], hwt[f, :n], tree.weighting)
            assert nb[f] == len(wid) and np.array_equal(bid[f, :nb[f]], wid) and bval[f, :nb[f]].tobytes() == wval.tobytes(), (tree.name, f)
            seen_stop += int((hwt[f, :n] <= 0).sum())
            seen_repeat += n - int((hwt[f, :n] <= 0).sum()) - len(wid)
        assert nb[1] == 0
    assert seen_stop > 0 and seen_repeat > 50, (seen_stop, seen_repeat)
    # constructed per-feature results: 3000 features over 500 words, zero and negative weights in between; n above cap is clamped
    rng = np.random.RandomState(3)
    cap = 3001
    nh = np.array([3000, 3500, 1025], np.int32)
    hw = rng.randint(0, 500, (3, cap)).astype(np.uint32)
    hw[2] = rng.randint(0, 2 ** 31, cap)
    hwt = np.round(rng.uniform(0.5, 12.0, (3, cap)), 6)
    hwt[rng.uniform(size=hwt.shape) < 0.1] = 0.0
    hwt[0, 5] = -1.0
    bid, bval, nb = _gpu_bow_vectors(ext, torch.from_numpy(hw.view(np.int32)).cuda(), torch.from_numpy(hwt).cuda(), torch.from_numpy(nh).cuda(), cap)
    for f, n in enumerate(np.minimum(nh, cap)):
        wid, wval = _host_bow(hw[f, :n], hwt[f, :n], 1)
        assert nb[f] == len(wid) and np.array_equal(bid[f, :nb[f]], wid) and bval[f, :nb[f]].tobytes() == wval.tobytes(), f
    t = torch.zeros(8200, dtype=torch.int32, device="cuda")
    assert ext._L.pgorb_bow_vectors_batch_device(ext._h, _tp(t), _tp(t), _tp(t), 1, 8193, _tp(t), _tp(t), _tp(t), _stream()) == -6
    # a vocabulary that does not score with L1 is refused by every call of the family
    l2 = trees[1]._replace(scoring=1, name="l2")
    V.ORBVocabulary(text_file=VC.write_text(l2, os.path.join(str(tmp_path), "l2.txt"))).upload(ext)
    assert ext._L.pgorb_bow_vectors_batch_device(ext._h, _tp(t), _tp(t), _tp(t), 1, 64, _tp(t), _tp(t), _tp(t), _stream()) == -1
    assert ext._L.pgorb_bow_score_l1_batch_device(ext._h, _tp(t), _tp(t), _tp(t), 1, 64, _tp(t), _tp(t), 1, _tp(t), _stream()) == -1
    tb = PC.table(PC.build(PC.edge_cases()[0]))
    with pytest.raises(Exception):
        gpu_single(ext, tb, "reloc")
    idf = trees[1]._replace(weighting=2, name="idf")
    V.ORBVocabulary(text_file=VC.write_text(idf, os.path.join(str(tmp_path), "idf.txt"))).upload(ext)
    assert ext._L.pgorb_bow_vectors_batch_device(ext._h, _tp(t), _tp(t), _tp(t), 1, 64, _tp(t), _tp(t), _tp(t), _stream()) == -1


@pytest.mark.gpu
def test_gpu_scores_equal_the_host():
    """pgorb_bow_score_l1_batch_device == pgorb_bow_score_l1 as bits: disjoint, identical, empty and 300-word vectors, an
    out-of-range pair."""
    import torch
    import pilotguru_amd as pg
    from pilotguru_amd import vocab as V
    e = pg.ORBextractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240, max_batch=2)
    try:
        rng = np.random.RandomState(11)
        vecs = [PC._bow(PC._rand_bow(rng, 300, 400)) for _ in range(4)] + [PC._bow(PC._rand_bow(rng, n, 90)) for n in (1, 3, 40, 64, 65)]
        vecs += [[(w + 1000, v) for w, v in vecs[4]], [], PC._bow({1: 1.0 + 2.0 ** -24, 2: 1.5 * 2.0 ** -54, 3: 1.5 * 2.0 ** -54})]
        F, cap = len(vecs), 320
        ids, val, nb = np.full((F, cap), 0xDEADBEEF, np.uint32), np.full((F, cap), np.nan), np.array([len(v) for v in vecs], np.int32)
        for f, v in enumerate(vecs):
            ids[f, :len(v)] = [w for w, _ in v]
            val[f, :len(v)] = [x for _, x in v]
        pairs = np.array([(a, b) for a in range(F) for b in range(F)] + [(0, F), (-1, 2)], np.int32)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        out = torch.full((len(pairs) + 2,), 77.0, dtype=torch.float64, device="cuda")
        pa, pb, d_ids, d_val, d_nb = d(pairs[:, 0]), d(pairs[:, 1]), d(ids.view(np.int32)), d(val), d(nb)
        e._check(e._L.pgorb_bow_score_l1_batch_device(e._h, _tp(d_ids), _tp(d_val), _tp(d_nb), F, cap, _tp(pa), _tp(pb),
                                                      len(pairs), _tp(out[1:]), _stream()))
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert out[0] == 77.0 and out[-1] == 77.0
        arr = lambda v: (np.array([w for w, _ in v], np.uint32), np.array([x for _, x in v], np.float64))
        want = np.array([V.bow_score_l1(arr(vecs[a]) if 0 <= a < F else arr([]), arr(vecs[b]) if 0 <= b < F else arr([])) for a, b in pairs])
        assert out[1:-1].tobytes() == want.tobytes(), np.nonzero(out[1:-1].view(np.uint64) != want.view(np.uint64))[0][:10]
        assert want[0 * F + 0] > 0.99 and want[4 * F + 9] == 0 and want[0 * F + 1] > 0.1
    finally:
        e.close()


def _mirror_of(case, ext):
    """The case's add / erase operations replayed on pilotguru_amd.KeyFrameDatabase (keys = logical ids)."""
    import pilotguru_amd as pg
    db = pg.KeyFrameDatabase(ext, max_candidates=1200)
    arr = lambda d: (np.array(sorted(d), np.uint32), np.array([d[w] for w in sorted(d)], np.float64))
    ops = case.ops if case.ops is not None else [("add", i) for i, k in enumerate(case.kfs) if k.member]
    seen = set()
    for op, i in ops:
        if op == "erase":
            db.erase(i)
        elif i in seen:
            db.add(i, arr(case.kfs[i].bow))                                  # added again: the mirror carries its score over
        else:
            db.add(i, arr(case.kfs[i].bow), neighbours=case.kfs[i].neigh[:PC.NEIGH], initial_score=case.kfs[i].state)
            seen.add(i)
    return db, arr, sum(1 for op, _ in ops if op == "add")


@pytest.mark.gpu
def test_gpu_python_mirror_runs_the_cases(ext, cases, wants):
    """pilotguru_amd.KeyFrameDatabase on every edge case and on random databases with erasures: the returned keys, last_common,
    last_scores and last_stats equal the reference (the mirror's rows are the table's rows of the add() calls)."""
    extra = [PC.random_case(s) for s in range(6)]
    failed = []
    for c, w in zip(list(cases) + extra, list(wants) + [PC.run_reference(c) for c in extra]):
        b = PC.build(c)
        db, arr, nadd = _mirror_of(c, ext)
        if c.form == "reloc":
            keys = db.DetectRelocalizationCandidates(arr(c.query))
        else:
            keys = db.DetectLoopCandidates(arr(c.query), c.min_score, connected=[j for j in c.connected if b.objs[j].row < nadd])
        want_keys = [b.rows[r][0] for r in w["cand"]]
        ok = (keys == want_keys and np.array_equal(db.last_common, w["common"][:nadd]) and
              db.last_scores.tobytes() == w["score"][:nadd].tobytes() and db.last_stats == tuple(w["stats"]))
        if not ok:
            failed.append((c.name, keys, want_keys, db.last_stats, w["stats"]))
    assert not failed, failed


@pytest.mark.gpu
def test_gpu_python_mirror_sequence_with_erase_and_readd(ext):
    """Two relocalisation queries through the mirror: the first scores S, S is erased and added again, the second reads S's stale
    score as A's neighbour -- the reference's objects carry mRelocScore the same way."""
    import pilotguru_amd as pg
    bows = {"A": PC._w(range(1, 6), 0.1), "B": PC._w(range(1, 6), 0.1), "S": {1: 0.75}}
    q1, q2 = {1: 0.75}, PC._w(range(1, 6), 0.1)
    objs = {k: PR.KeyFrame(k, PC._bow(v)) for k, v in bows.items()}
    objs["A"].ordered = [objs["S"]]
    ref = PR.Database()
    db = pg.KeyFrameDatabase(ext)
    arr = lambda d: (np.array(sorted(d), np.uint32), np.array([d[w] for w in sorted(d)], np.float64))
    for k in "ABS":
        ref.add(objs[k])
        db.add(k, arr(bows[k]), neighbours=["S"] if k == "A" else None)
    hits = collections.Counter()
    r1 = PR.detect_relocalization_candidates(ref, 1, PC._bow(q1), hits=hits)
    assert db.DetectRelocalizationCandidates(arr(q1)) == [kf.id for kf in r1.cand]
    assert db.last_stats == (3, 1, 3) and [float(x) for x in db.last_scores] == [float(objs[k].mRelocScore) for k in "ABS"]
    ref.erase(objs["S"]); ref.add(objs["S"])
    db.erase("S"); db.add("S", arr(bows["S"]))
    r2 = PR.detect_relocalization_candidates(ref, 2, PC._bow(q2), hits=hits)
    got = db.DetectRelocalizationCandidates(arr(q2))
    assert hits["stale_read"] == 1 and [kf.id for kf in r2.cand] == ["S"] and got == ["S"], (got, dict(hits))
    assert db.last_stats == (len(r2.sharing), r2.max_common, r2.nscores)
    assert [float(x) for x in db.last_scores] == [float(objs[k].mRelocScore) for k in "ABS"] + [float(objs["S"].mRelocScore)]
    assert [int(x) for x in db.last_common] == [5, 5, 0, 1]
    small = pg.KeyFrameDatabase(ext, max_candidates=0)
    small.add("A", arr(bows["A"]))
    with pytest.raises(ValueError):
        small.DetectRelocalizationCandidates(arr(q2))                          # one candidate, room for none
    assert float(small.last_scores[0]) == 0.5                                    # ... and the score was still stored


@pytest.mark.gpu
def test_gpu_single_calls_check_their_inputs(ext, cases):
    """Every malformed input of the single host calls is PGORB_E_ARG before anything is launched."""
    t0 = PC.table(PC.build([c for c in cases if c.name == "connected"][0]))
    n = t0["nrows"]

    def call(form="loop", **kw):
        t = dict(t0)
        t.update(kw)
        try:
            return gpu_single(ext, t, form)["ncand"]
        except Exception as e:
            return e.code

    def swapped(key, i, j):
        a = t0[key].copy()
        a[i], a[j] = a[j], a[i]
        return a

    def with_value(key, i, v):
        a = t0[key].copy()
        a[i] = v
        return a
    assert call() == 1 and call("reloc") >= 0
    eleven = np.zeros(n + 1, np.int32)
    eleven[1:] = 11
    bad = {
        "unsorted word ids": dict(bow_id=swapped("bow_id", 0, 1)),
        "a repeated word id": dict(bow_id=with_value("bow_id", 1, t0["bow_id"][0])),
        "neighbour out of range": dict(neigh=with_value("neigh", 0, n)),
        "negative neighbour": dict(neigh=with_value("neigh", 0, -1)),
        "connected out of range": dict(conn=np.array([n], np.int32)),
        "query out of range": dict(query=n),
        "eleven neighbours": dict(neigh_start=eleven, neigh=np.zeros(11 * n, np.int32)),
        "bow_start not from 0": dict(bow_start=with_value("bow_start", 0, 1)),
        "bow_start decreases": dict(bow_start=with_value("bow_start", 1, t0["bow_start"][2] + 1)),
        "neigh_start decreases": dict(neigh_start=with_value("neigh_start", 1, t0["neigh_start"][-1] + 1)),
    }
    got = {name: (call("loop", **kw), call("reloc", **kw)) for name, kw in bad.items()}
    got["connected out of range"] = (got["connected out of range"][0], -1)      # (the relocalisation form takes no connected set)
    assert all(v == (-1, -1) for v in got.values()), got
