"""A plain, sequential restatement of KeyFrameDatabase (thirdparty/orb-slam2/src/KeyFrameDatabase.cc): add (:53-59), erase (:61-80),
DetectLoopCandidates (:89-210) and DetectRelocalizationCandidates (:212-310), with L1Scoring::score (Thirdparty/DBoW2/DBoW2/
ScoringObject.cpp:23-60).  It is written from that upstream text; it does not use oracle/ and was not derived from the HIP kernels
(pilotguru_amd/csrc/place.hip).

Objects are real: a KeyFrame carries mnRelocQuery / mnRelocWords / mRelocScore and the loop twins, its ordered covisible key frames
and its connected set; the database's inverted file is a dict of Python lists in add() order.  Float steps go through np.float32.
`rules` (a Rules) switches one reading at a time; `hits` (a collections.Counter or None) counts the edges reached.

mRelocScore is not initialised by the reference's constructor (KeyFrame.cc:138), so its value for a never-scored key frame is
indeterminate there; here a KeyFrame is built with the value the case gives it (the product takes it as `score_state`).
"""
from dataclasses import dataclass

import numpy as np

f32, f64 = np.float32, np.float64


@dataclass(frozen=True)
class Rules:
    threshold: str = "gt"        # mnWords > minCommonWords is scored | "ge"
    factor: str = "float"        # int minCommonWords = maxCommonWords*0.8f | "double": maxCommonWords*0.8
    score_sum: str = "running"   # one running double sum over the common words in word order | "pairwise": a tree
    score_type: str = "float"    # float si = score(...) | "double": si and the stored score stay double
    acc: str = "float"           # float accScore += stored score | "double"
    stale: str = "stale"         # relocalisation: a sharing, unscored neighbour gives its stale mRelocScore | "zero"
    order: str = "list"          # lKFsSharingWords in inverted-file order | "index": by add index only
    dedup: str = "first"         # a pBestKF is emitted at its first retained entry | "last"
    retain: str = "gt"           # accScore > 0.75f*bestAccScore | "ge"
    neighbours: int = 10         # GetBestCovisibilityKeyFrames(10) | 11


REFERENCE = Rules()
MUTANTS = {
    "threshold=ge": Rules(threshold="ge"),
    "factor=double": Rules(factor="double"),
    "score_sum=pairwise": Rules(score_sum="pairwise"),
    "score_type=double": Rules(score_type="double"),
    "acc=double": Rules(acc="double"),
    "stale=zero": Rules(stale="zero"),
    "order=index": Rules(order="index"),
    "dedup=last": Rules(dedup="last"),
    "retain=ge": Rules(retain="ge"),
    "neighbours=11": Rules(neighbours=11),
}
# int(maxCommonWords*0.8f) == int(maxCommonWords*0.8) for every count below 5 242 881: 0.8f and 0.8 both lie above 4/5 by less
# than 2e-8 relative, so up to there the product is on an integer's near side only at multiples of 5, where both round to that
# integer, and stays a fifth away from one everywhere else.  No BowVector holds that many words (the largest ORB vocabulary has a
# million), so no case can tell the two apart; tests/test_place_recognition.py checks the bound exhaustively instead.
EQUIVALENT = ("factor=double",)


class KeyFrame:
    def __init__(self, kid, bow, reloc_score=0.0):
        self.id = kid
        self.bow = [(int(w), f64(v)) for w, v in bow]                      # ascending word ids (a std::map)
        self.ordered = []                                                  # mvpOrderedConnectedKeyFrames
        self.connected = set()                                             # GetConnectedKeyFrames()
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = -1, 0, f32(reloc_score)
        self.mnLoopQuery, self.mnLoopWords, self.mLoopScore = -1, 0, f32(0)

    def best_covisibles(self, n):
        return self.ordered[:n]


def _pairwise(t):
    if len(t) == 1:
        return t[0]
    mid = len(t) // 2
    return f64(_pairwise(t[:mid]) + _pairwise(t[mid:]))


def score_l1(a, b, rules=REFERENCE):
    """L1Scoring::score (ScoringObject.cpp:23-60): a merge walk over two ascending vectors."""
    terms = []
    i = j = 0
    while i < len(a) and j < len(b):
        if a[i][0] == b[j][0]:
            vi, wi = a[i][1], b[j][1]
            terms.append(f64(f64(abs(f64(vi - wi)) - abs(vi)) - abs(wi)))
            i += 1
            j += 1
        elif a[i][0] < b[j][0]:
            i += 1
        else:
            j += 1
    if rules.score_sum == "pairwise" and terms:
        s = _pairwise(terms)
    else:
        s = f64(0)
        for t in terms:
            s = f64(s + t)
    return f64(-s / f64(2.0))


class Database:
    def __init__(self):
        self.inverted = {}                                                 # word -> [KeyFrame] in add order

    def add(self, kf):
        for w, _ in kf.bow:
            self.inverted.setdefault(w, []).append(kf)

    def erase(self, kf):
        for w, _ in kf.bow:
            lst = self.inverted.get(w, [])
            for k, other in enumerate(lst):
                if other is kf:
                    del lst[k]
                    break


@dataclass
class Result:
    cand: list               # the returned key frames
    sharing: list            # lKFsSharingWords
    max_common: int
    nscores: int
    best_kf: list            # pBestKF of every entry of lScoreAndMatch, in list order (None when the walk ended early)


def _min_common(max_common, rules):
    if rules.factor == "double":
        return int(max_common * 0.8)
    return int(f32(f32(max_common) * f32(0.8)))


def _as_score(s, rules):
    return f64(s) if rules.score_type == "double" else f32(s)


def _add(acc, v, rules):
    if rules.acc == "double":
        return f64(f64(acc) + f64(v))
    return f32(f32(acc) + f32(v))


def _emit(acc_and_best, best_acc, rules, hits):
    keep = f32(f32(0.75) * f32(best_acc))                                  # float minScoreToRetain = 0.75f*bestAccScore
    order = acc_and_best if rules.dedup == "first" else acc_and_best[::-1]
    out, seen = [], set()
    for acc, kf in order:
        if hits is not None and acc == keep:
            hits["acc_equals_retain"] += 1
        if acc > keep or (rules.retain == "ge" and acc == keep):
            if id(kf) in seen:
                if hits is not None:
                    hits["duplicate_best"] += 1
                continue
            seen.add(id(kf))
            out.append(kf)
    if rules.dedup == "last":                                              # (the mutant keeps a key frame's LAST place in list order)
        out = out[::-1]
    return out


def _sharing_order(lst, index_of, rules):
    return sorted(lst, key=index_of) if rules.order == "index" else lst


def detect_relocalization_candidates(db, frame_id, bow, index_of=None, rules=REFERENCE, hits=None):
    """KeyFrameDatabase.cc:212-310.  `bow` = F->mBowVec; `index_of(kf)` = the add index (only the order=index mutant reads it)."""
    bow = [(int(w), f64(v)) for w, v in bow]
    sharing = []
    for w, _ in bow:                                                       # :220-236
        for kf in db.inverted.get(w, []):
            if kf.mnRelocQuery != frame_id:
                kf.mnRelocWords = 0
                kf.mnRelocQuery = frame_id
                sharing.append(kf)
            kf.mnRelocWords += 1
    if hits is not None and not bow:
        hits["empty_query"] += 1
    if not sharing:
        if hits is not None:
            hits["no_sharing"] += 1
        return Result([], [], 0, 0, [])
    sharing = _sharing_order(sharing, index_of, rules)
    max_common = max(kf.mnRelocWords for kf in sharing)                    # :241-246
    min_common = _min_common(max_common, rules)
    entries, nscores = [], 0
    for kf in sharing:                                                     # :253-263
        if hits is not None and kf.mnRelocWords == min_common:
            hits["count_equals_min"] += 1
        if kf.mnRelocWords > min_common or (rules.threshold == "ge" and kf.mnRelocWords == min_common):
            nscores += 1
            si = _as_score(score_l1(bow, kf.bow, rules), rules)
            kf.mRelocScore = si
            kf.scored_by = frame_id
            entries.append((si, kf))
    if not entries:
        return Result([], sharing, max_common, nscores, [])
    best_acc = f32(0)                                                      # :270
    acc_and_best = []
    for si, kf in entries:                                                 # :273-298
        best_score, acc, best_kf = si, si, kf
        for kf2 in kf.best_covisibles(rules.neighbours):
            if kf2.mnRelocQuery != frame_id:
                if hits is not None and not getattr(kf2, "in_db", True):
                    hits["neighbour_not_in_db"] += 1
                continue
            v = kf2.mRelocScore
            if getattr(kf2, "scored_by", None) != frame_id:                # shares words, was not scored now: a stale value
                if hits is not None:
                    hits["stale_read"] += 1
                if rules.stale == "zero":
                    v = f32(0)
            acc = _add(acc, v, rules)
            if hits is not None and v == best_score and best_kf is not kf:
                hits["neighbour_tie"] += 1
            if v > best_score:
                best_kf, best_score = kf2, v
        acc_and_best.append((acc, best_kf))
        if acc > best_acc:
            best_acc = acc
    return Result(_emit(acc_and_best, best_acc, rules, hits), sharing, max_common, nscores, [b for _, b in acc_and_best])


def detect_loop_candidates(db, kf_q, min_score, index_of=None, rules=REFERENCE, hits=None):
    """KeyFrameDatabase.cc:89-210.  kf_q = pKF (its bow, id and connected set are read)."""
    min_score = f32(min_score)
    connected = kf_q.connected
    sharing = []
    for w, _ in kf_q.bow:                                                  # :99-117
        for kf in db.inverted.get(w, []):
            if kf.mnLoopQuery != kf_q.id:
                kf.mnLoopWords = 0
                if kf not in connected:
                    kf.mnLoopQuery = kf_q.id
                    sharing.append(kf)
                elif hits is not None:
                    hits["connected_excluded"] += 1
            kf.mnLoopWords += 1
    if hits is not None and not kf_q.bow:
        hits["empty_query"] += 1
    if not sharing:
        if hits is not None:
            hits["no_sharing"] += 1
        return Result([], [], 0, 0, [])
    sharing = _sharing_order(sharing, index_of, rules)
    max_common = max(kf.mnLoopWords for kf in sharing)                     # :124-129
    min_common = _min_common(max_common, rules)
    entries, nscores = [], 0
    for kf in sharing:                                                     # :136-150
        if hits is not None and kf.mnLoopWords == min_common:
            hits["count_equals_min"] += 1
        if kf.mnLoopWords > min_common or (rules.threshold == "ge" and kf.mnLoopWords == min_common):
            nscores += 1
            si = _as_score(score_l1(kf_q.bow, kf.bow, rules), rules)
            kf.mLoopScore = si
            kf.scored_by = kf_q.id
            if hits is not None and si == min_score:
                hits["si_equals_min_score"] += 1
            if si >= min_score:
                entries.append((si, kf))
            else:
                kf.below_min_for = kf_q.id
    if not entries:
        return Result([], sharing, max_common, nscores, [])
    best_acc = min_score                                                   # :159
    acc_and_best = []
    for si, kf in entries:                                                 # :162-186
        best_score, acc, best_kf = si, si, kf
        for kf2 in kf.best_covisibles(rules.neighbours):
            ok = kf2.mnLoopQuery == kf_q.id and (kf2.mnLoopWords > min_common or
                                                 (rules.threshold == "ge" and kf2.mnLoopWords == min_common))
            if not ok:
                if hits is not None and not getattr(kf2, "in_db", True):
                    hits["neighbour_not_in_db"] += 1
                continue
            v = kf2.mLoopScore
            if hits is not None and getattr(kf2, "below_min_for", None) == kf_q.id:
                hits["below_min_contributes"] += 1
            acc = _add(acc, v, rules)
            if hits is not None and v == best_score and best_kf is not kf:
                hits["neighbour_tie"] += 1
            if v > best_score:
                best_kf, best_score = kf2, v
        acc_and_best.append((acc, best_kf))
        if acc > best_acc:
            best_acc = acc
    if hits is not None and best_acc == min_score:
        hits["best_stays_min_score"] += 1
    return Result(_emit(acc_and_best, best_acc, rules, hits), sharing, max_common, nscores, [b for _, b in acc_and_best])


def sharing_closed_form(members, query_bow, excluded=()):
    """The kernels' specification of lKFsSharingWords: `members` = the database's key frames in add order; the list is those with at
    least one common word (and not in `excluded`), sorted by (smallest common word, add position), each with its number of common
    words.  Returns [(kf, count)]."""
    qw = set(int(w) for w, _ in query_bow)
    rows = []
    for pos, kf in enumerate(members):
        common = [w for w, _ in kf.bow if w in qw]
        if common and kf not in excluded:
            rows.append((min(common), pos, kf, len(common)))
    rows.sort(key=lambda r: (r[0], r[1]))
    return [(r[2], r[3]) for r in rows]
