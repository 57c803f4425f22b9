"""Cases for the place-recognition queries (tests/test_place_recognition.py): constructed edges of KeyFrameDatabase::
DetectRelocalizationCandidates / DetectLoopCandidates, random databases with erasures, and the two large shapes.

A case lists LOGICAL key frames and the add / erase operations on them.  build() replays the operations on real objects
(tests/place_reference.py) and lays out the table the library takes: one row per add() in add order (an erased key frame's row
stays, with membership cleared; adding it again appends a new row), then the frames that never entered the database, then the
query's own row.  Edge values are dyadic, so every score (a sum of min(query value, key frame value) over the common words) is exact.
"""
import os
import sys
from dataclasses import dataclass, field

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import place_reference as PR  # noqa: E402

f32 = np.float32
NEIGH = 10


@dataclass
class KF:
    bow: dict                                  # word -> value
    neigh: list = field(default_factory=list)  # logical ids, ordered (may exceed 10: only the first 10 reach the table)
    state: float = 0.0                         # stored mRelocScore on entry
    member: bool = True                        # False: never added to the database


@dataclass
class Case:
    name: str
    form: str                                  # "reloc" | "loop"
    kfs: list
    query: dict
    ops: list = None                           # [("add" | "erase", logical id)]; None: every member once, in order
    min_score: float = 0.0
    connected: tuple = ()                      # logical ids (loop form)
    query_id: int = 1000


@dataclass
class Built:
    case: Case
    db: object
    objs: list                                 # reference KeyFrame of every logical key frame (obj.row = its current table row)
    rows: list                                 # table rows: (logical id, in_db)
    qobj: object


def _bow(d):
    return sorted((int(w), float(v)) for w, v in d.items())


def build(case):
    objs = [PR.KeyFrame(i, _bow(k.bow), k.state) for i, k in enumerate(case.kfs)]
    db = PR.Database()
    rows = []
    ops = case.ops if case.ops is not None else [("add", i) for i, k in enumerate(case.kfs) if k.member]
    for o in objs:
        o.in_db, o.row = False, -1
    for op, i in ops:
        o = objs[i]
        if op == "add":
            db.add(o)
            o.in_db, o.row = True, len(rows)
            rows.append([i, True])
        else:
            db.erase(o)
            o.in_db = False
            rows[o.row][1] = False
    for i, o in enumerate(objs):
        if o.row < 0:
            o.row = len(rows)
            rows.append([i, False])
    for o, k in zip(objs, case.kfs):
        o.ordered = [objs[j] for j in k.neigh]
    q = PR.KeyFrame(case.query_id, _bow(case.query))
    q.connected = set(objs[j] for j in case.connected)
    q.row = len(rows)
    return Built(case, db, objs, [tuple(r) for r in rows], q)


def table(b):
    """The library's inputs for one built case: CSR BowVectors, membership, neighbour CSR (first 10), state, the query row and the
    connected rows."""
    case = b.case
    nrows = len(b.rows) + 1
    bows, in_db, neigh, state = [], np.zeros(nrows, np.uint8), [], np.zeros(nrows, np.float32)
    for r, (i, member) in enumerate(b.rows):
        o = b.objs[i]
        bows.append(o.bow)
        in_db[r] = member
        live = o.row == r
        neigh.append([x.row for x in o.ordered[:NEIGH]] if live else [])
        state[r] = f32(case.kfs[i].state)
    bows.append(b.qobj.bow)
    neigh.append([])
    start = np.zeros(nrows + 1, np.int32)
    start[1:] = np.cumsum([len(x) for x in bows])
    ids = np.array([w for x in bows for w, _ in x], np.uint32)
    vals = np.array([v for x in bows for _, v in x], np.float64)
    nstart = np.zeros(nrows + 1, np.int32)
    nstart[1:] = np.cumsum([len(x) for x in neigh])
    nidx = np.array([j for x in neigh for j in x], np.int32)
    conn = np.array(sorted(b.objs[j].row for j in case.connected), np.int32)[::-1].copy()      # "in any order"
    return dict(nrows=nrows, bow_start=start, bow_id=ids, bow_val=vals, in_db=in_db, neigh_start=nstart, neigh=nidx, state=state,
                query=nrows - 1, conn=conn, min_score=f32(case.min_score))


def expected(b, res, state_rows):
    """A reference Result as the library's outputs: candidates as rows, common words and stored scores per row, stats."""
    nrows = len(b.rows) + 1
    common = np.zeros(nrows, np.int32)
    score = np.array(state_rows, np.float32).copy() if b.case.form == "reloc" else np.zeros(nrows, np.float32)
    loop = b.case.form == "loop"
    for kf in res.sharing:
        common[kf.row] = kf.mnLoopWords if loop else kf.mnRelocWords
    for kf in res.sharing:
        if getattr(kf, "scored_by", None) == b.qobj.id:                 # (the reference's bookkeeping of who was scored now)
            score[kf.row] = f32(kf.mLoopScore if loop else kf.mRelocScore)
    return dict(cand=[kf.row for kf in res.cand], common=common, score=score,
                stats=(len(res.sharing), res.max_common, res.nscores), best=[kf.row for kf in res.best_kf])


def run_reference(case, rules=PR.REFERENCE, hits=None):
    b = build(case)
    t = table(b)
    index_of = lambda kf: kf.row
    if case.form == "reloc":
        res = PR.detect_relocalization_candidates(b.db, b.qobj.id, b.qobj.bow, index_of, rules, hits)
    else:
        res = PR.detect_loop_candidates(b.db, b.qobj, case.min_score, index_of, rules, hits)
    return expected(b, res, t["state"])


def same(a, b):
    return (a["cand"] == b["cand"] and np.array_equal(a["common"], b["common"]) and a["score"].tobytes() == b["score"].tobytes() and
            tuple(a["stats"]) == tuple(b["stats"]))


def extra_edges(case, hits):
    """Edges that only a comparison shows: what the stale read changes, and an erase that changes the sharing order."""
    want = run_reference(case)
    if case.form == "reloc":
        zero = run_reference(case, PR.Rules(stale="zero"))
        if want["cand"] != zero["cand"] and want["best"] == zero["best"]:
            hits["stale_changes_candidates"] += 1
        if want["best"] != zero["best"]:
            hits["stale_changes_best"] += 1
    if case.ops is not None and any(op == "erase" for op, _ in case.ops):
        b = build(case)
        res = PR.detect_relocalization_candidates(b.db, b.qobj.id, b.qobj.bow) if case.form == "reloc" else \
            PR.detect_loop_candidates(b.db, b.qobj, case.min_score)
        logical = [kf.id for kf in res.sharing]
        plain = build(Case(case.name, case.form, case.kfs, case.query, None, case.min_score, case.connected))
        res2 = PR.detect_relocalization_candidates(plain.db, plain.qobj.id, plain.qobj.bow) if case.form == "reloc" else \
            PR.detect_loop_candidates(plain.db, plain.qobj, case.min_score)
        kept = [kf.id for kf in res2.sharing if kf.id in logical]
        if kept != logical:
            hits["erase_changes_order"] += 1


def _w(words, v):
    return {w: v for w in words}


def edge_cases():
    E = 2.0 ** -40
    c = []
    # count == minCommonWords is not scored: max 5 -> min 4
    c.append(Case("threshold", "reloc", [KF(_w(range(1, 6), 0.125)), KF(_w(range(1, 5), 0.125)), KF(_w(range(1, 6), 0.0625)),
                                          KF({9: 0.5}, member=False)], _w(range(1, 6), 0.25)))
    # nobody shares a word; a frame outside the database has the query's words
    c.append(Case("no_sharing", "reloc", [KF(_w(range(1, 6), 0.125)), KF({7: 0.5, 8: 0.5}), KF({100: 0.5, 101: 0.5}, member=False),
                                           KF({3: 1.0}, neigh=[0, 1])], {100: 0.5, 101: 0.5}))
    c.append(Case("empty_query", "reloc", [KF(_w(range(1, 6), 0.125), neigh=[1]), KF({1: 0.5}), KF({2: 1.0})], {}))
    # neighbours outside the database: one never added, one erased; their states would change everything if read
    c.append(Case("neighbour_not_in_db", "reloc",
                  [KF(_w(range(1, 6), 0.125), neigh=[1, 2, 3]), KF(_w(range(1, 6), 0.25), state=5.0, member=False),
                   KF(_w(range(1, 4), 0.25), state=7.0), KF(_w(range(1, 6), 0.0625))], _w(range(1, 6), 0.25),
                  ops=[("add", 0), ("add", 2), ("add", 3), ("erase", 2)]))
    # the stale score of a sharing, unscored neighbour (one common word of five): 0.25 keeps pBestKF and drops the other entry
    c.append(Case("stale_candidates", "reloc", [KF(_w(range(1, 6), 0.1), neigh=[2]), KF(_w(range(1, 6), 0.1)), KF({1: 0.5}, state=0.25)],
                  _w(range(1, 6), 0.1)))
    # ... 0.75 also moves pBestKF to the unscored neighbour
    c.append(Case("stale_best", "reloc", [KF(_w(range(1, 6), 0.1), neigh=[2]), KF(_w(range(1, 6), 0.1)), KF({1: 0.5}, state=0.75)],
                  _w(range(1, 6), 0.1)))
    # two neighbours whose double scores differ below float resolution: a tie in float, the first keeps
    c.append(Case("neighbour_tie", "reloc", [KF({1: 0.125, 2: 0.125}, neigh=[1, 2]), KF({1: 0.25, 2: 0.25}), KF({1: 0.25, 2: 0.25 + E})],
                  {1: 1.0, 2: 1.0}))
    # acc == 0.75f * best: 2 + 1 + 2^-24 is 3 in float; best 4
    c.append(Case("retain_equal", "reloc", [KF(_w(range(1, 5), 1.0)), KF(_w(range(1, 5), 0.5), neigh=[2, 3]), KF({1: 1.0}, state=1.0),
                                             KF({2: 1.0}, state=2.0 ** -24)], _w(range(1, 5), 2.0)))
    # entries in list order: 1 -> P, 2 -> Q, 0 -> P: P is emitted once, at entry 1's place
    c.append(Case("duplicate_best", "reloc", [KF({3: 0.25}, neigh=[3]), KF({1: 0.25}, neigh=[3]), KF({2: 0.3125}, neigh=[4]), KF({3: 0.5}),
                                               KF({3: 0.5})], {1: 1.0, 2: 1.0, 3: 1.0}))
    # list order is (first common word, add index), not the index
    c.append(Case("word_order", "reloc", [KF({9: 0.5}), KF({2: 0.5}), KF({4: 0.5})], {2: 1.0, 4: 1.0, 9: 1.0}))
    # the eleventh covisible key frame is never read
    c.append(Case("eleven_neighbours", "reloc",
                  [KF(_w(range(1, 6), 0.125), neigh=list(range(1, 12)))] + [KF({1 + i % 5: 0.5}, state=0.0) for i in range(10)] +
                  [KF({2: 0.5}, state=8.0)], _w(range(1, 6), 0.25)))
    # a running double sum lands on a float tie (1 + 2^-24 -> 1.0f); a tree sum lands above it
    m1, m2 = 1.0 + 2.0 ** -24, 1.5 * 2.0 ** -54
    c.append(Case("running_sum", "reloc", [KF({1: m1, 2: m2, 3: m2}), KF({1: 0.5, 2: 0.25, 3: 0.125})], {1: m1, 2: m2, 3: m2}))
    # erase and add again: the key frame moves to the end of every inverted list
    c.append(Case("erase_order", "reloc", [KF({5: 0.5, 6: 0.5}, neigh=[1]), KF({5: 0.25, 6: 0.5}), KF({5: 0.125, 6: 0.125})], {5: 1.0, 6: 1.0},
                  ops=[("add", 0), ("add", 1), ("add", 2), ("erase", 0), ("add", 0)]))
    # ---- loop form
    # a connected key frame never enters the list and gives nothing as a neighbour; count 2 == min 2 is not scored
    c.append(Case("connected", "loop", [KF(_w((1, 2, 3), 0.5)), KF(_w((1, 2, 3), 0.25), neigh=[0, 2]), KF(_w((1, 2), 0.5)), KF({3: 0.5}, neigh=[1])],
                  _w((1, 2, 3), 1.0), min_score=0.125, connected=(0,)))
    # si == minScore is kept; si < minScore is not an entry but still contributes as a neighbour
    c.append(Case("min_score", "loop", [KF(_w((1, 2), 0.25), neigh=[1]), KF(_w((1, 2), 0.125), neigh=[0]), KF(_w((1, 2), 0.5))],
                  _w((1, 2), 1.0), min_score=0.5))
    # bestAccScore stays at minScore
    c.append(Case("best_stays", "loop", [KF(_w((1, 2), 0.25)), KF(_w((1, 2), 0.125))], _w((1, 2), 1.0), min_score=0.5))
    c.append(Case("loop_no_sharing", "loop", [KF(_w((1, 2), 0.25)), KF({4: 1.0})], {1: 1.0, 4: 1.0}, min_score=0.0, connected=(0, 1)))
    c.append(Case("loop_empty_query", "loop", [KF(_w((1, 2), 0.25), neigh=[1]), KF({4: 1.0})], {}, min_score=0.0))
    c.append(Case("loop_duplicate", "loop", [KF({3: 0.25}, neigh=[3]), KF({1: 0.25}, neigh=[3]), KF({2: 0.3125}, neigh=[4]), KF({3: 0.5}),
                                              KF({3: 0.5}), KF({1: 0.5, 7: 0.5}, neigh=[0])], {1: 1.0, 2: 1.0, 3: 1.0}, min_score=0.0625,
                  ops=[("add", 5), ("add", 0), ("add", 1), ("add", 2), ("add", 3), ("add", 4), ("erase", 5)]))
    return c


def _rand_bow(rng, nwords, vocab):
    w = np.sort(rng.choice(vocab, size=nwords, replace=False))
    v = rng.uniform(0.05, 1.0, nwords)
    v = v / v.sum()
    return {int(a): float(b) for a, b in zip(w, v)}


def random_case(seed, form=None, nkf=None, words=(3, 40), vocab=90, erasures=True, name=None):
    """A random database with erasures and re-adds, dense sharing, random covisibility and stale states."""
    rng = np.random.RandomState(1000 + seed)
    form = form or ("reloc", "loop")[seed % 2]
    nkf = nkf or int(rng.randint(12, 40))
    kfs = []
    for i in range(nkf):
        nw = int(rng.randint(words[0], words[1] + 1))
        nn = int(rng.randint(0, 13))
        neigh = [int(x) for x in rng.choice(nkf, size=min(nn, nkf - 1), replace=False) if x != i]
        kfs.append(KF(_rand_bow(rng, nw, vocab), neigh, float(f32(rng.uniform(0, 0.3))), member=rng.uniform() > 0.1))
    ops = [("add", i) for i, k in enumerate(kfs) if k.member]
    if erasures:
        members = [i for _, i in ops]
        for i in rng.choice(members, size=max(1, len(members) // 4), replace=False):
            ops.append(("erase", int(i)))
            if rng.uniform() < 0.6:
                ops.append(("add", int(i)))
    q = _rand_bow(rng, int(rng.randint(words[0], words[1] + 1)), vocab)
    conn = tuple(int(x) for x in rng.choice(nkf, size=int(rng.randint(0, 5)), replace=False))
    return Case(name or "random%d" % seed, form, kfs, q, ops, float(f32(rng.uniform(0.0, 0.08))), conn if form == "loop" else ())


def long_vectors_case(form):
    """A 300-word query against 300-word key frames: five 64-word slices per list, many ballot trips, long running sums."""
    c = random_case(7, form, nkf=12, words=(300, 300), vocab=400, erasures=False, name="long_" + form)
    return c


def many_key_frames_case(form):
    """1100 key frames of 2-4 words against a query that holds every word: a sharing list longer than one workgroup; the ~360
    four-word key frames are scored, each has one scored neighbour (so every entry stays above the retention threshold and many
    entries name the same pBestKF) and a few unscored ones with small stale scores."""
    rng = np.random.RandomState(77)
    nkf = 1100
    nw = rng.randint(2, 5, nkf)
    four, fewer = np.nonzero(nw == 4)[0], np.nonzero(nw < 4)[0]
    kfs = []
    for i in range(nkf):
        w = np.sort(rng.choice(12, size=nw[i], replace=False))
        if nw[i] == 4 and rng.uniform() < 0.5:
            vals = [0.05, 0.05, 0.45, 0.45]
        else:
            vals = [1.0 / nw[i]] * nw[i]
        neigh = []
        if nw[i] == 4:
            neigh = [int(x) for x in rng.choice(fewer, size=int(rng.randint(0, 6)), replace=False)]
            neigh.insert(int(rng.randint(0, len(neigh) + 1)), int(rng.choice(four[four != i])))
        kfs.append(KF({int(a): float(b) for a, b in zip(w, vals)}, neigh, float(f32(rng.uniform(0, 0.004)))))
    q = {int(x): 1.0 / 12 for x in range(12)}
    conn = tuple(int(x) for x in rng.choice(nkf, size=40, replace=False))
    return Case("many_" + form, form, kfs, q, None, 0.01, conn if form == "loop" else ())


def chain_case():
    """One database and six relocalisation queries run in sequence: every query's stored scores are the next one's stale state."""
    base = random_case(3, "reloc", nkf=30, words=(5, 30), vocab=60, erasures=True, name="chain")
    rng = np.random.RandomState(5)
    return base, [_rand_bow(rng, int(rng.randint(5, 30)), 60) for _ in range(6)]
