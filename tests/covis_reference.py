"""A literal, object-level restatement of the covisibility graph of thirdparty/orb-slam2, in plain Python:
  KeyFrame::UpdateConnections, AddConnection, UpdateBestCovisibles           src/KeyFrame.cc:392-482, :226-260
  GetBestCovisibilityKeyFrames, GetCovisiblesByWeight                        src/KeyFrame.cc:277-302
  LoopConnections of LoopClosing::CorrectLoop                                src/LoopClosing.cc:548-566
  Tracking::UpdateLocalKeyFrames, UpdateLocalPoints                          src/Tracking.cc:1196-1321
Key frames and map points are objects; std::map<KeyFrame*, ..> and std::set<KeyFrame*> are dicts and sets ITERATED BY ADDRESS
RANK (KeyFrame.addr), AddConnection is called where the reference calls it and the breaks stand where its breaks stand.  Nothing
here knows how csrc/covisibility.hip is organised; `decomposed_update_connections` restates the closed form that file relies on
 and the tests hold it against the literal sequence.

Rules names every reading; MUTANTS flips one each, and tests/test_covisibility.py / test_update_local_map.py assert that every
mutant changes a compared output on a named case of tests/covis_cases.py."""
import collections
import copy
import dataclasses

UPDATED, RESORTED, EMPTY, FALLBACK, PARENT_SET, LIMIT = 1, 2, 4, 8, 16, 32
NO_VOTES, LM_LIMIT = 1, 2
MAX_KF, MAX_CONN, INFO = 4096, 2048, 4


@dataclasses.dataclass(frozen=True)
class Rules:
    th_strict: bool = False              # counter > th instead of >= th (:444)
    ties_ascending: bool = False         # equal weights in ascending address order
    kfmax_last: bool = False             # pKFmax the LAST maximum (>= at :439)
    map_only_sends: bool = False         # mConnectedKeyFrameWeights = the connections at or above th, not KFcounter (:470)
    resort_from_sends: bool = False      # UpdateBestCovisibles over the entries at or above th only
    unchanged_resorts: bool = False      # AddConnection with an equal weight still calls UpdateBestCovisibles (:234-235)
    sends_any_position: bool = False     # the AddConnection calls of EARLIER list members survive a later own update
    bad_points_counted: bool = False     # no isBad() test at :412
    parent_for_id0: bool = False         # mnId != 0 not tested at :474
    # views and the local map
    cap_ge: bool = False                 # size() >= 80 at Tracking.cc:1267
    parent_break_inner: bool = False     # the break at :1310 leaves no loop
    parent_bad_test: bool = False        # the parent tested for isBad()
    expand_appended: bool = False        # the expansion runs over the entries it appends too
    bad_after_max: bool = False          # a bad key frame can still be the maximum (:1249 after :1252)
    eleventh_neighbour: bool = False     # GetBestCovisibilityKeyFrames(11)
    children_index_order: bool = False   # the children in index order, not address order
    by_weight_strict: bool = False       # GetCovisiblesByWeight: an equal weight left out of the prefix


REFERENCE = Rules()
GRAPH_MUTANTS = {n: Rules(**{n: True}) for n in ("th_strict", "ties_ascending", "kfmax_last", "map_only_sends", "resort_from_sends",
                                                  "unchanged_resorts", "sends_any_position", "bad_points_counted", "parent_for_id0")}
LOCAL_MUTANTS = {n: Rules(**{n: True}) for n in ("cap_ge", "parent_break_inner", "parent_bad_test", "expand_appended", "bad_after_max",
                                                  "eleventh_neighbour", "children_index_order", "by_weight_strict")}


class MapPoint:
    def __init__(self, idx, bad=False):
        self.idx, self.bad, self.observations = idx, bad, []          # observations: key frames, iterated in the order given

    def isBad(self):
        return self.bad


class KeyFrame:
    def __init__(self, idx, addr, id0=False, bad=False):
        self.idx, self.addr, self.id0, self.bad = idx, addr, id0, bad
        self.mvpMapPoints = []                                         # MapPoint or None per slot
        self.weights = {}                                              # mConnectedKeyFrameWeights
        self.ordered, self.ordered_w = [], []                          # mvpOrderedConnectedKeyFrames, mvOrderedWeights
        self.parent, self.first = None, True
        self.status = 0

    def isBad(self):
        return self.bad

    def _sorted(self, pairs, rules):
        # sort(vPairs) ascending by (weight, address), then push_front: descending (weight, address)
        if rules.ties_ascending:
            return sorted(pairs, key=lambda wk: (-wk[0], wk[1].addr))
        return sorted(pairs, key=lambda wk: (wk[0], wk[1].addr), reverse=True)

    def UpdateBestCovisibles(self, rules, th):
        pairs = [(w, k) for k, w in sorted(self.weights.items(), key=lambda kw: kw[0].addr)]
        if rules.resort_from_sends:
            pairs = [(w, k) for w, k in pairs if w >= th]
        pairs = self._sorted(pairs, rules)
        self.ordered, self.ordered_w = [k for _, k in pairs], [w for w, _ in pairs]

    def AddConnection(self, pKF, weight, rules, th):
        if pKF not in self.weights:
            self.weights[pKF] = weight
        elif self.weights[pKF] != weight:
            self.weights[pKF] = weight
        else:
            if rules.unchanged_resorts:
                self.UpdateBestCovisibles(rules, th)
                self.status |= RESORTED
            return
        self.UpdateBestCovisibles(rules, th)
        self.status |= RESORTED

    def UpdateConnections(self, th, rules, log=None):
        KFcounter = collections.OrderedDict()
        for pMP in self.mvpMapPoints:
            if pMP is None:
                continue
            if pMP.isBad() and not rules.bad_points_counted:
                continue
            for pKF in pMP.observations:
                if pKF is self:
                    continue
                KFcounter[pKF] = KFcounter.get(pKF, 0) + 1
        if not KFcounter:
            self.status |= EMPTY
            return
        nmax, pKFmax, vPairs = 0, None, []
        for pKF in sorted(KFcounter, key=lambda k: k.addr):
            c = KFcounter[pKF]
            if c > nmax or (rules.kfmax_last and c >= nmax):
                nmax, pKFmax = c, pKF
            if (c > th) if rules.th_strict else (c >= th):
                vPairs.append((c, pKF))
                pKF.AddConnection(self, c, rules, th)
                if log is not None:
                    log.append((self, pKF, c))
        self.status = UPDATED
        if not vPairs:
            vPairs.append((nmax, pKFmax))
            pKFmax.AddConnection(self, nmax, rules, th)
            if log is not None:
                log.append((self, pKFmax, nmax))
            self.status |= FALLBACK
        vPairs = self._sorted(vPairs, rules)
        self.weights = {k: w for w, k in vPairs} if rules.map_only_sends else dict(KFcounter)
        self.ordered, self.ordered_w = [k for _, k in vPairs], [w for w, _ in vPairs]
        if self.first and (not self.id0 or rules.parent_for_id0):
            self.parent = self.ordered[0]
            self.first = False
            self.status |= PARENT_SET

    def GetBestCovisibilityKeyFrames(self, N):
        return list(self.ordered) if len(self.ordered) < N else self.ordered[:N]

    def GetCovisiblesByWeight(self, w, rules=REFERENCE):
        if not self.ordered:
            return []
        # upper_bound(first, last, w, weightComp) with weightComp(a, b) = a > b: the first element e with w > e
        it = next((t for t, e in enumerate(self.ordered_w) if (w >= e if rules.by_weight_strict else w > e)), None)
        if it is None:
            return []
        return self.ordered[:it]


def correct_loop_connections(kfs, lst, th, rules=REFERENCE):
    """LoopClosing.cc:548-566 over mvpCurrentConnectedKFs = lst: UpdateConnections one after another and the LoopConnections map.
    Returns [(pKFi, pKFj, weight)] in map-then-set address order, the weight what Optimizer.cc:866 reads afterwards."""
    for k in kfs:
        k.status = 0
    loop, log = {}, []
    for pKFi in lst:
        prev = list(pKFi.ordered)
        pKFi.UpdateConnections(th, rules, log)
        s = set(pKFi.weights)
        for k in prev:
            s.discard(k)
        for k in lst:
            s.discard(k)
        loop[pKFi] = s
    if rules.sends_any_position:
        for src, dst, c in log:
            dst.AddConnection(src, c, rules, th)
    out = []
    for pKFi in sorted(loop, key=lambda k: k.addr):
        for pKFj in sorted(loop[pKFi], key=lambda k: k.addr):
            out.append((pKFi, pKFj, pKFi.weights.get(pKFj, 0)))
    return out


def decomposed_update_connections(kfs, lst, th):
    """The closed form, on the same objects, without running one update after another: the counters depend on
    the map alone; key frame j SENDS (i, c_j[i]) to every i with c_j[i] >= th, or to its single pKFmax; row i ends as its base --
    its own result when it is a list member with a non-empty counter, else its input with, for an EMPTY member, the sends of the
    members before it -- overwritten by the sends of the members after its position (all members when it is not in the list), and
    re-sorted from the whole final map exactly when one of those sends differed from the entry it met."""
    pos = {k: n for n, k in enumerate(lst)}
    counter, send = {}, {}
    for i in lst:
        c = {}
        for pMP in i.mvpMapPoints:
            if pMP is None or pMP.isBad():
                continue
            for k in pMP.observations:
                if k is not i:
                    c[k] = c.get(k, 0) + 1
        counter[i] = c
        s = {k: w for k, w in c.items() if w >= th}
        if c and not s:
            m = max(c.values())
            kmax = min((k for k in c if c[k] == m), key=lambda k: k.addr)
            s = {kmax: m}
        send[i] = s

    def order(m):
        return sorted(((w, k) for k, w in m.items()), key=lambda wk: (wk[0], wk[1].addr), reverse=True)

    result, loop = {}, {}
    for i in kfs:
        status = 0
        base, ordered, parent, first = dict(i.weights), list(zip(i.ordered_w, i.ordered)), i.parent, i.first
        later = lst
        if i in pos:
            changed = False
            for j in lst[:pos[i]]:
                if i in send[j]:
                    changed |= base.get(j) != send[j][i]
                    base[j] = send[j][i]
            prev = set(base) if changed else set(i.ordered)
            if counter[i]:
                base, ordered, status = dict(counter[i]), order(send[i]), UPDATED
                if not any(w >= th for w in counter[i].values()):
                    status |= FALLBACK
                if first and not i.id0:
                    parent, first, status = ordered[0][1], False, status | PARENT_SET
            else:
                status = EMPTY
                if changed:
                    ordered, status = order(base), status | RESORTED
            loop[i] = set(base) - prev - set(lst)
            later = lst[pos[i] + 1:]
        changed = False
        for j in later:
            if i in send[j]:
                changed |= base.get(j) != send[j][i]
                base[j] = send[j][i]
        if changed:
            ordered, status = order(base), status | RESORTED
        result[i] = (base, ordered, parent, first, status)
    for i, (base, ordered, parent, first, status) in result.items():
        i.weights, i.ordered, i.ordered_w, i.parent, i.first, i.status = base, [k for _, k in ordered], [w for w, _ in ordered], parent, first, status
    out = []
    for i in sorted(loop, key=lambda k: k.addr):
        for j in sorted(loop[i], key=lambda k: k.addr):
            out.append((i, j, i.weights.get(j, 0)))
    return out


def covisibility_views(kfs, nbest, w, rules=REFERENCE):
    """(best [nkf] lists, covisibles [nkf] lists of (kf, weight), by_weight [nkf] lengths)"""
    return ([k.GetBestCovisibilityKeyFrames(nbest) for k in kfs], [list(zip(k.ordered, k.ordered_w)) for k in kfs],
            [len(k.GetCovisiblesByWeight(w, rules)) for k in kfs])


def update_local_map(kfs, frame_points, prev_local=None, nbest=10, max_local=80, rules=REFERENCE):
    """Tracking::UpdateLocalMap for a frame whose mvpMapPoints is frame_points (MapPoint or None).  Returns (slots after the first
    loop, mvpLocalKeyFrames, mpReferenceKF or None = kept, mvpLocalMapPoints, no_votes)."""
    slots = list(frame_points)
    keyframeCounter = {}
    for i, pMP in enumerate(slots):
        if pMP is not None:
            if not pMP.isBad():
                for k in pMP.observations:
                    keyframeCounter[k] = keyframeCounter.get(k, 0) + 1
            else:
                slots[i] = None
    no_votes = not keyframeCounter
    pKFmax = None
    if no_votes:
        local = list(prev_local) if prev_local is not None else []
    else:
        mx, local, marked = 0, [], set()
        for pKF in sorted(keyframeCounter, key=lambda k: k.addr):
            c = keyframeCounter[pKF]
            if rules.bad_after_max and c > mx:
                mx, pKFmax = c, pKF
            if pKF.isBad():
                continue
            if c > mx:
                mx, pKFmax = c, pKF
            local.append(pKF)
            marked.add(pKF)
        children = collections.defaultdict(list)
        for k in kfs:
            if k.parent is not None:
                children[k.parent].append(k)
        e, end = 0, len(local)
        while e < (len(local) if rules.expand_appended else end):
            if len(local) >= max_local if rules.cap_ge else len(local) > max_local:
                break
            pKF = local[e]
            e += 1
            for n in pKF.GetBestCovisibilityKeyFrames(nbest + (1 if rules.eleventh_neighbour else 0)):
                if not n.isBad() and n not in marked:
                    local.append(n)
                    marked.add(n)
                    break
            for ch in sorted(children[pKF], key=(lambda k: k.idx) if rules.children_index_order else (lambda k: k.addr)):
                if not ch.isBad() and ch not in marked:
                    local.append(ch)
                    marked.add(ch)
                    break
            pParent = pKF.parent
            if pParent is not None and not (rules.parent_bad_test and pParent.isBad()):
                if pParent not in marked:
                    local.append(pParent)
                    marked.add(pParent)
                    if not rules.parent_break_inner:
                        break
    points, taken = [], set()
    for pKF in local:
        for pMP in pKF.mvpMapPoints:
            if pMP is not None and pMP not in taken and not pMP.isBad():
                points.append(pMP)
                taken.add(pMP)
    return slots, local, pKFmax, points, no_votes


def clone(kfs):
    return copy.deepcopy(kfs)
