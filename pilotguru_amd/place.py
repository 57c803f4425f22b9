"""Mirror of ORB_SLAM2::KeyFrameDatabase (thirdparty/orb-slam2/src/KeyFrameDatabase.cc) over libpgorb's place-recognition calls
(csrc/place.hip): add / erase keep the table the library takes, the two Detect* queries run on the GPU.

The table holds one row per add(), in add order -- the order of every inverted list of the reference (:53-59).  erase() clears a
row's membership (:61-80); adding the key frame again appends a new row, as the reference appends it to the end of its lists.
The stored relocalisation scores (mRelocScore) live here between queries, so a sequence of queries sees what the reference's
sequence sees; a key frame that is erased and added again keeps its score, as the reference's object does.  The reference never
initialises mRelocScore (KeyFrame.cc:138); a key frame's first row starts at `initial_score` (0.0 when not given).
"""
import ctypes as C

import numpy as np

MAX_NEIGHBOURS = 10


def _bow(bow, name):
    try:
        ids, vals = bow
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        vals = np.ascontiguousarray(vals, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("%s: a BowVector is (word ids, values)" % name)
    if len(ids) != len(vals):
        raise ValueError("%s: %d word ids, %d values" % (name, len(ids), len(vals)))
    if len(ids) > 1 and not (ids[1:] > ids[:-1]).all():
        raise ValueError("%s: word ids are unsorted or repeat" % name)
    return ids, vals


class KeyFrameDatabase:
    def __init__(self, extractor, max_candidates=256):
        from . import _lib
        self._e = extractor                   # the context the queries run on (add / erase and the input checks need none)
        self._L = _lib.lib()
        self.max_candidates = int(max_candidates)
        self._keys, self._bows, self._member = [], [], []
        self._neigh = {}                      # key -> ordered covisible keys
        self._row = {}                        # key -> its current row
        self._score = []                      # mRelocScore per row
        self.last_common = self.last_stats = self.last_scores = None

    def __len__(self):
        return sum(self._member)

    def add(self, key, bow, neighbours=None, initial_score=None):
        """KeyFrameDatabase::add(pKF).  `neighbours` (optional) = the keys of GetBestCovisibilityKeyFrames(10), in order.
        `initial_score` (optional) sets mRelocScore; without it a key frame added again keeps the score of its erased row."""
        if key in self._row and self._member[self._row[key]]:
            raise ValueError("KeyFrameDatabase.add: key frame %r is already in the database" % (key,))
        ids, vals = _bow(bow, "KeyFrameDatabase.add")
        if neighbours is not None:
            self.set_neighbours(key, neighbours)
        if initial_score is None:
            initial_score = self._score[self._row[key]] if key in self._row else 0.0
        self._row[key] = len(self._keys)
        self._keys.append(key); self._bows.append((ids, vals)); self._member.append(True)
        self._score.append(np.float32(initial_score))

    def set_neighbours(self, key, neighbours):
        neighbours = list(neighbours)
        if len(neighbours) > MAX_NEIGHBOURS:
            raise ValueError("KeyFrameDatabase: %d neighbours, at most %d (GetBestCovisibilityKeyFrames(10))" % (len(neighbours), MAX_NEIGHBOURS))
        self._neigh[key] = neighbours

    def erase(self, key):
        """KeyFrameDatabase::erase(pKF)."""
        r = self._row.get(key)
        if r is None or not self._member[r]:
            raise ValueError("KeyFrameDatabase.erase: key frame %r is not in the database" % (key,))
        self._member[r] = False

    def score(self, a, b):
        """mpVoc->score(a, b) for L1_NORM (L1Scoring::score): the double the reference returns."""
        from .vocab import bow_score_l1
        return bow_score_l1(_bow(a, "KeyFrameDatabase.score"), _bow(b, "KeyFrameDatabase.score"))

    def _tables(self, query_bow):
        bows = self._bows + [query_bow]
        n = len(bows)
        start = np.zeros(n + 1, np.int32)
        start[1:] = np.cumsum([len(i) for i, _ in bows])
        ids = np.concatenate([i for i, _ in bows]) if n else np.zeros(0, np.uint32)
        vals = np.concatenate([v for _, v in bows]) if n else np.zeros(0, np.float64)
        in_db = np.array(self._member + [False], np.uint8)
        lists = []
        for r, k in enumerate(self._keys):
            live = self._row[k] == r
            lists.append([self._row[x] for x in self._neigh.get(k, []) if x in self._row] if live else [])
        lists.append([])
        nstart = np.zeros(n + 1, np.int32)
        nstart[1:] = np.cumsum([len(x) for x in lists])
        neigh = np.array([j for x in lists for j in x], np.int32)
        return n, start, np.ascontiguousarray(ids, np.uint32), np.ascontiguousarray(vals, np.float64), in_db, nstart, neigh

    def _finish(self, rc, cand, common, stats, scores):
        self._e._check(rc)
        self.last_common, self.last_stats, self.last_scores = common[:-1], tuple(int(x) for x in stats), scores[:-1]
        if rc > self.max_candidates:
            raise ValueError("KeyFrameDatabase: %d candidates, max_candidates is %d" % (rc, self.max_candidates))
        return [self._keys[r] for r in cand[:rc]]

    def DetectRelocalizationCandidates(self, bow):
        """KeyFrameDatabase::DetectRelocalizationCandidates(F) with F->mBowVec = bow: the candidate keys in the reference's order."""
        q = _bow(bow, "DetectRelocalizationCandidates")
        n, start, ids, vals, in_db, nstart, neigh = self._tables(q)
        p = lambda a: C.c_void_p(a.ctypes.data)
        state = np.array(self._score + [np.float32(0)], np.float32)
        cand, common, stats = np.zeros(max(self.max_candidates, 1), np.int32), np.zeros(n, np.int32), np.zeros(3, np.int32)
        rc = self._L.pgorb_detect_relocalization_candidates(self._e._h, n, p(start), p(ids), p(vals), p(in_db), p(nstart), p(neigh), n - 1,
                                                            p(state), p(cand), self.max_candidates, p(common), p(stats))
        if rc >= 0:
            self._score = list(state[:-1])                # the scores are written whether or not the candidates fit
        return self._finish(rc, cand, common, stats, state)

    def DetectLoopCandidates(self, bow, min_score, connected=()):
        """KeyFrameDatabase::DetectLoopCandidates(pKF, minScore) with pKF->mBowVec = bow and pKF->GetConnectedKeyFrames() =
        `connected` (keys; the choice of that set stays with the caller)."""
        q = _bow(bow, "DetectLoopCandidates")
        for k in connected:
            if k not in self._row:
                raise ValueError("DetectLoopCandidates: connected key frame %r was never added" % (k,))
        n, start, ids, vals, in_db, nstart, neigh = self._tables(q)
        p = lambda a: C.c_void_p(a.ctypes.data)
        conn = np.array([self._row[k] for k in connected], np.int32)
        cand, common, stats = np.zeros(max(self.max_candidates, 1), np.int32), np.zeros(n, np.int32), np.zeros(3, np.int32)
        scores = np.zeros(n, np.float32)
        rc = self._L.pgorb_detect_loop_candidates(self._e._h, n, p(start), p(ids), p(vals), p(in_db), p(nstart), p(neigh), n - 1,
                                                  float(min_score), p(conn), len(conn), p(cand), self.max_candidates, p(common), p(scores),
                                                  p(stats))
        return self._finish(rc, cand, common, stats, scores)
