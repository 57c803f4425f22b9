"""The map edits as the reference's objects carry them out, written from the text of thirdparty/orb-slam2 (src/MapPoint.cc:119-232,
src/KeyFrame.cc:313-336) and of the six call sites that produce them: LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:142-161),
the tail of CreateNewMapPoints (:436-449), ORBmatcher::Fuse's tail (src/ORBmatcher.cc:961-979), SearchAndFuse (src/LoopClosing.cc:
601-615), LocalBundleAdjustment's erasures (src/Optimizer.cc:748-757) and CorrectLoop's matched points (src/LoopClosing.cc:520-537).

MapPoint and KeyFrame are objects; mObservations is a std::map<KeyFrame*, size_t>, which iterates by the key frames' ADDRESSES --
here by `rank`.  `apply_edits` drives them from an edit list one edit after another and reports what pgorb_apply_map_edits reports.

Rules holds the named mutants: every field False is the reference."""
import dataclasses

import numpy as np

NOP, ADD, REPLACE, ERASE, SET_REF = 0, 1, 2, 3, 4
APPLIED, ALREADY, SELF, NOT_OBSERVED, WENT_BAD, BAD_INDEX, LIMIT = 1, 2, 4, 8, 16, 32, 64
TOUCH_CHANGED, TOUCH_SURVIVOR, TOUCH_STALE = 1, 2, 4
INFO, MAX_BAG, MAX_EDITS, MAX_LIST = 8, 2048, 4096, 4194304
EDIT_DTYPE = np.dtype([("op", "<i4"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4")])


@dataclasses.dataclass
class Rules:
    add_skips_slot_when_observed: bool = False      # ADD leaves the slot alone when the list already holds the key frame
    replace_tests_slot: bool = False                # REPLACE asks the key frame's slots, not the survivor's list, whether it is in the key frame
    replace_skips_bad_loser_counters: bool = False  # a loser that is already bad does not hand its counters over
    replace_keeps_loser_good: bool = False          # the loser does not go bad
    replace_self_clears: bool = False               # a->Replace(a) clears a
    erase_bad_at_three: bool = False                # SetBadFlag at <= 3 observations left
    erase_bad_below_two: bool = False               # ... at < 2
    erase_ref_to_last: bool = False                 # mpRefKF moves to the last entry of what is left
    erase_keeps_slot: bool = False                  # the erased key frame keeps its slot
    set_bad_clears_own_slots_only: bool = False     # SetBadFlag clears only slots that still hold the point
    set_bad_drops_ref: bool = False                 # SetBadFlag forgets mpRefKF
    first_writer_wins: bool = False                 # a slot keeps the value of the first edit of the list that wrote it
    list_order_by_index: bool = False               # mObservations iterates by key-frame index, not by address rank
    dead_entries_counted: bool = False              # masked entries of the input lists exist


MUTANTS = {f.name: Rules(**{f.name: True}) for f in dataclasses.fields(Rules)}


class Map:
    """what the objects share: the rules, the count of slot assignments, and -- for the first-writer mutant -- who wrote a slot"""

    def __init__(self, rules):
        self.rules, self.slot_writes, self.edit, self.writer = rules, 0, -1, {}
        self.history, self.shared = {}, 0                    # for the coverage tests: the edits that wrote each slot, Replace's "already there" branch


class KeyFrame:
    def __init__(self, world, index, rank, mnId, nslots):
        self.world, self.index, self.rank, self.mnId = world, index, rank, mnId
        self.mvpMapPoints = [None] * nslots

    def _set(self, idx, value):
        m = self.world
        m.slot_writes += 1
        m.history.setdefault((self.index, idx), []).append(m.edit)
        if m.rules.first_writer_wins and m.writer.setdefault((self.index, idx), m.edit) != m.edit:
            return
        self.mvpMapPoints[idx] = value

    def AddMapPoint(self, pMP, idx):                          # KeyFrame.cc:313-317
        self._set(idx, pMP)

    def EraseMapPointMatchIdx(self, idx):                     # :319-323
        self._set(idx, None)

    def EraseMapPointMatch(self, pMP):                        # :325-330: the index comes from the point's list
        idx = pMP.GetIndexInKeyFrame(self)
        if idx >= 0:
            self._set(idx, None)

    def ReplaceMapPointMatch(self, idx, pMP):                 # :333-336
        self._set(idx, pMP)

    def GetMapPoint(self, idx):
        return self.mvpMapPoints[idx]


class MapPoint:
    def __init__(self, world, index, pRefKF=None):
        self.world, self.index = world, index
        self.mObservations = {}
        self.mbBad, self.mnVisible, self.mnFound, self.mpReplaced, self.mpRefKF = False, 1, 1, None, pRefKF    # MapPoint.cc:62-64
        self.mnFirstKFid = pRefKF.mnId if pRefKF is not None else -1
        self.touched = 0

    def observations(self):
        """(key frame, index) as the std::map iterates"""
        key = (lambda kv: kv[0].index) if self.world.rules.list_order_by_index else (lambda kv: (kv[0].rank, kv[0].index))
        return sorted(self.mObservations.items(), key=key)

    def Observations(self):
        return len(self.mObservations)

    def isBad(self):
        return self.mbBad

    def IsInKeyFrame(self, pKF):
        return pKF in self.mObservations

    def GetIndexInKeyFrame(self, pKF):
        return self.mObservations.get(pKF, -1)

    def _changed(self):
        self.touched |= TOUCH_CHANGED | (TOUCH_STALE if self.touched & TOUCH_SURVIVOR else 0)

    def AddObservation(self, pKF, idx):                       # :119-130
        if pKF in self.mObservations:
            return False
        self.mObservations[pKF] = idx
        self._changed()
        return True

    def EraseObservation(self, pKF):                          # :132-158; returns (was listed, went bad)
        r = self.world.rules
        bBad = False
        listed = pKF in self.mObservations
        if listed:
            del self.mObservations[pKF]
            self._changed()
            if self.mpRefKF is pKF:
                left = self.observations()
                self.mpRefKF = (left[-1 if r.erase_ref_to_last else 0][0]) if left else None      # begin() of an empty map: none
            n = len(self.mObservations)
            bBad = n <= 3 if r.erase_bad_at_three else (n < 2 if r.erase_bad_below_two else n <= 2)
        if bBad:
            self.SetBadFlag()
        return listed, bBad

    def SetBadFlag(self):                                     # :172-187
        obs = self.observations()
        self.mbBad = True
        self.mObservations = {}
        if self.world.rules.set_bad_drops_ref:
            self.mpRefKF = None
        for pKF, idx in obs:
            if self.world.rules.set_bad_clears_own_slots_only and pKF.mvpMapPoints[idx] is not self:
                continue
            pKF.EraseMapPointMatchIdx(idx)

    def Replace(self, pMP):                                   # :196-232, without ComputeDistinctiveDescriptors and Map::EraseMapPoint
        r = self.world.rules
        if pMP is self and not r.replace_self_clears:
            return False
        obs = self.observations()
        was_bad = self.mbBad
        self.mObservations = {}
        if obs:
            self.touched |= TOUCH_CHANGED
        if not r.replace_keeps_loser_good:
            self.mbBad = True
        nvisible, nfound = self.mnVisible, self.mnFound
        self.mpReplaced = pMP
        for pKF, idx in obs:
            inkf = (pMP in pKF.mvpMapPoints) if r.replace_tests_slot else pMP.IsInKeyFrame(pKF)
            if not inkf:
                pKF.ReplaceMapPointMatch(idx, pMP)
                pMP.AddObservation(pKF, idx)
            else:
                self.world.shared += 1
                pKF.EraseMapPointMatchIdx(idx)
        if not (was_bad and r.replace_skips_bad_loser_counters):
            pMP.mnFound = _i32(pMP.mnFound + nfound)
            pMP.mnVisible = _i32(pMP.mnVisible + nvisible)
        pMP.touched = (pMP.touched | TOUCH_SURVIVOR) & ~TOUCH_STALE       # the descriptor is computed here
        return True


def _i32(x):
    return int(np.int64(x).astype(np.int32))


class World:
    """the objects of one table: key_frames[f], points[p]"""

    def __init__(self, a, rules=None):
        """a: the arrays of map_edit_cases.arrays()"""
        rules = rules or Rules()
        self.map = Map(rules)
        nkf, n = len(a["n"]), a["n"]
        order = a["order"] if a["order"] is not None else np.arange(nkf)
        ids = a.get("kf_id", np.arange(nkf))
        self.key_frames = [KeyFrame(self.map, f, int(order[f]), int(ids[f]), int(n[f])) for f in range(nkf)]
        self.points = []
        st, live = a["obs_start"], a["obs_live"]
        for p in range(len(st) - 1):
            mp = MapPoint(self.map, p)
            mp.mbBad, mp.mnVisible, mp.mnFound = bool(a["point_bad"][p]), int(a["visible"][p]), int(a["found"][p])
            mp.mpReplaced = int(a["replaced"][p])                          # an index or -1 on entry; a MapPoint once Replace ran
            mp.mnFirstKFid = int(a["first_kf_id"][p]) if "first_kf_id" in a else -1
            for o in range(st[p], st[p + 1]):
                if live[o] or rules.dead_entries_counted:
                    mp.mObservations[self.key_frames[a["obs_frame"][o]]] = int(a["obs_idx"][o])
            ro = int(a["ref_obs"][p])
            o = st[p] + ro
            mp.mpRefKF = self.key_frames[a["obs_frame"][o]] if 0 <= ro < st[p + 1] - st[p] and (live[o] or rules.dead_entries_counted) else None
            self.points.append(mp)
        for f in range(nkf):
            for i in range(n[f]):
                v = int(a["kf_point"][f, i])
                self.key_frames[f].mvpMapPoints[i] = self.points[v] if v >= 0 else None
        self.recent = []

    def new_point(self, pRefKF):
        mp = MapPoint(self.map, len(self.points), pRefKF)
        self.points.append(mp)
        return mp


def components(a, edits):
    """the component (its smallest point) of every point, by the REPLACE edits whose indices are in range"""
    npoints = len(a["obs_start"]) - 1
    root = list(range(npoints))

    def find(x):
        while root[x] != x:
            x = root[x]
        return x
    for e in edits:
        if e["op"] == REPLACE and 0 <= e["a"] < npoints and 0 <= e["b"] < npoints and e["a"] != e["b"]:
            x, y = find(int(e["a"])), find(int(e["b"]))
            root[max(x, y)] = min(x, y)
    return [find(p) for p in range(npoints)]


def edit_valid(a, e):
    npoints, nkf = len(a["obs_start"]) - 1, len(a["n"])
    op, x, y, z = int(e["op"]), int(e["a"]), int(e["b"]), int(e["c"])
    if op == ADD:
        return 0 <= x < npoints and 0 <= y < nkf and 0 <= z < a["n"][y]
    if op == REPLACE:
        return 0 <= x < npoints and 0 <= y < npoints
    if op in (ERASE, SET_REF):
        return 0 <= x < npoints and 0 <= y < nkf
    return False


def bag_limit(a, edits, rules=None):
    """does a component's live input entries plus its ADD edits exceed MAX_BAG?  (the lists that count are those of the points an
    ADD, an ERASE or a REPLACE with two different points names)"""
    comp = components(a, edits)
    lv = a["obs_live"] if not (rules and rules.dead_entries_counted) else np.ones_like(a["obs_live"])
    load, named = {}, set()
    for e in edits:
        if e["op"] in (NOP, SET_REF) or not edit_valid(a, e) or (e["op"] == REPLACE and e["a"] == e["b"]):
            continue
        named.add(int(e["a"]))
        if e["op"] == REPLACE:
            named.add(int(e["b"]))
        if e["op"] == ADD:
            load[comp[e["a"]]] = load.get(comp[e["a"]], 0) + 1
    for p in named:
        load[comp[p]] = load.get(comp[p], 0) + int(lv[a["obs_start"][p]:a["obs_start"][p + 1]].sum())
    return any(v > MAX_BAG for v in load.values())


def apply_edits(a, edits, obs_cap_out, select_bits=0, sel_cap=0, rules=None, sentinel=None):
    """the edits one after another on the objects; returns the arrays pgorb_apply_map_edits leaves.  sentinel: what the outputs
    held before (a dict of arrays); None = zeros / -1."""
    rules = rules or Rules()
    W = World(a, rules)
    npoints, nkf, ne = len(W.points), len(W.key_frames), len(edits)
    status = np.zeros(ne, np.int32)
    bad_in = [p.mbBad for p in W.points]
    for k, e in enumerate(edits):
        W.map.edit = k
        op, x, y, z = int(e["op"]), int(e["a"]), int(e["b"]), int(e["c"])
        if op == NOP:
            continue
        if not edit_valid(a, e):
            status[k] = BAD_INDEX
            continue
        P = W.points[x]
        if op == ADD:
            kf = W.key_frames[y]
            added = P.AddObservation(kf, z)
            status[k] = APPLIED | (0 if added else ALREADY)
            if added or not rules.add_skips_slot_when_observed:
                kf.AddMapPoint(P, z)
        elif op == REPLACE:
            status[k] = APPLIED if P.Replace(W.points[y]) else SELF
        elif op == ERASE:
            kf = W.key_frames[y]
            if not rules.erase_keeps_slot:
                kf.EraseMapPointMatch(P)
            listed, went = P.EraseObservation(kf)
            status[k] = (APPLIED | (WENT_BAD if went else 0)) if listed else NOT_OBSERVED
        else:
            P.mpRefKF = W.key_frames[y]
            status[k] = APPLIED
    return report(W, a, edits, status, bad_in, obs_cap_out, select_bits, sel_cap, sentinel)


def table(W, cap):
    """the objects as arrays: slots, flags, counters, the CSR in iteration order, ref_obs"""
    nkf, npoints = len(W.key_frames), len(W.points)
    kf_point = np.full((nkf, cap), -1, np.int32)
    for f, K in enumerate(W.key_frames):
        for i, v in enumerate(K.mvpMapPoints):
            kf_point[f, i] = v.index if v is not None else -1
    st, of, oi, ref = [0], [], [], []
    for P in W.points:
        obs = P.observations()
        of += [K.index for K, _ in obs]
        oi += [i for _, i in obs]
        ref.append(next((k for k, (K, _) in enumerate(obs) if K is P.mpRefKF), -1))
        st.append(len(of))
    rep = [(P.mpReplaced.index if isinstance(P.mpReplaced, MapPoint) else int(P.mpReplaced if P.mpReplaced is not None else -1)) for P in W.points]
    i32 = lambda x: np.array(x, np.int32).reshape(-1)
    return dict(kf_point=kf_point, point_bad=np.array([P.mbBad for P in W.points], np.uint8).reshape(-1), visible=i32([P.mnVisible for P in W.points]),
                found=i32([P.mnFound for P in W.points]), replaced=i32(rep), obs_start=i32(st), obs_frame=i32(of), obs_idx=i32(oi), ref_obs=i32(ref),
                touched=i32([P.touched for P in W.points]), first_kf_id=i32([P.mnFirstKFid for P in W.points]))


def report(W, a, edits, status, bad_in, obs_cap_out, select_bits, sel_cap, sentinel):
    npoints, ne = len(W.points), len(edits)
    cap = a["kf_point"].shape[1]
    t = table(W, cap)
    total = int(t["obs_start"][-1])
    selected = [p for p in range(npoints) if sel_cap and t["touched"][p] & select_bits]
    s = sentinel or {}
    blank = lambda k, shape, fill: (np.array(s[k]) if k in s else np.full(shape, fill, np.int32))
    out = dict(obs_start_out=blank("obs_start_out", npoints + 1, 0), obs_frame_out=blank("obs_frame_out", obs_cap_out, 0),
               obs_idx_out=blank("obs_idx_out", obs_cap_out, 0), ref_obs_out=blank("ref_obs_out", npoints, -1), edit_status=blank("edit_status", ne, 0),
               touched=blank("touched", npoints, 0), select_out=blank("select_out", sel_cap, -1), info=blank("info", INFO, 0))
    out["stats"] = dict(shared=W.map.shared, history=W.map.history, status=status)
    carried = sum(1 for e in edits if e["op"] != NOP and edit_valid(a, e))       # more than MAX_EDITS edits carried out: the fourth capacity
    if total > obs_cap_out or len(selected) > sel_cap or bag_limit(a, edits, W.map.rules) or carried > MAX_EDITS:
        out["info"][0] = LIMIT
        out.update({k: a[k].copy() for k in ("kf_point", "point_bad", "visible", "found", "replaced")})
        return out
    comp = components(a, edits)
    ncomp = len({comp[int(e["a"])] for e in edits if e["op"] != NOP and edit_valid(a, e)})
    out["obs_start_out"][:npoints + 1] = t["obs_start"]
    out["obs_frame_out"][:total] = t["obs_frame"]
    out["obs_idx_out"][:total] = t["obs_idx"]
    out["ref_obs_out"][:npoints] = t["ref_obs"]
    out["edit_status"][:ne] = status
    out["touched"][:npoints] = t["touched"]
    out["select_out"][:sel_cap] = -1
    out["select_out"][:len(selected)] = selected
    out["info"][:INFO] = [0, total, int(np.sum((status & APPLIED) != 0)), sum(1 for P, b in zip(W.points, bad_in) if P.mbBad and not b), ncomp,
                      W.map.slot_writes, int(np.sum((t["touched"] & TOUCH_STALE) != 0)), len(selected)]
    out.update({k: t[k] for k in ("kf_point", "point_bad", "visible", "found", "replaced")})
    return out


# ---------------------------------------------------------------- the six call-site loops, on the objects
def process_new_key_frame(W, kf):
    """LocalMapping.cc:142-161; returns the class of every slot (0, 1 = observation added, 2 = the else branch)"""
    K = W.key_frames[kf]
    cls = [0] * len(K.mvpMapPoints)
    for i, pMP in enumerate(K.mvpMapPoints):
        if pMP is not None and not pMP.isBad():
            if not pMP.IsInKeyFrame(K):
                pMP.AddObservation(K, i)
                cls[i] = 1
            else:
                W.recent.append(pMP)
                cls[i] = 2
    return cls


def create_new_map_points_tail(W, kf1, records):
    """:436-449 for records (kf2, idx1, idx2) in creation order; returns the new points' indices"""
    K1 = W.key_frames[kf1]
    made = []
    for kf2, idx1, idx2 in records:
        K2 = W.key_frames[kf2]
        pMP = W.new_point(K1)
        pMP.AddObservation(K1, idx1)
        pMP.AddObservation(K2, idx2)
        K1.AddMapPoint(pMP, idx1)
        K2.AddMapPoint(pMP, idx2)
        W.recent.append(pMP)
        made.append(pMP.index)
    return made


FUSE_SKIPPED, FUSE_NO_MATCH, FUSE_ADDED, FUSE_MERGED, FUSE_REPLACED, FUSE_KF_POINT_BAD, FUSE_REPLACE_REQUESTED = 0, 1, 2, 3, 4, 5, 6


def fuse_tail(W, kf, queries, best_idx):
    """ORBmatcher.cc:961-979 for the queries whose bestDist passed (best_idx >= 0), in query order; returns the actions taken"""
    K = W.key_frames[kf]
    action = []
    for q, s in zip(queries, best_idx):
        if s < 0:
            action.append(FUSE_NO_MATCH)
            continue
        pMP, pMPinKF = W.points[q], K.GetMapPoint(s)
        if pMPinKF is not None:
            if not pMPinKF.isBad():
                if pMPinKF.Observations() > pMP.Observations():
                    pMP.Replace(pMPinKF)
                    action.append(FUSE_MERGED)
                else:
                    pMPinKF.Replace(pMP)
                    action.append(FUSE_REPLACED)
            else:
                action.append(FUSE_KF_POINT_BAD)
        else:
            pMP.AddObservation(K, s)
            K.AddMapPoint(pMP, s)
            action.append(FUSE_ADDED)
    return action


def fuse_sim3_and_replace(W, kf, queries, best_idx):
    """ORBmatcher.cc:1085-1099 then LoopClosing.cc:607-615; returns (action, replace_point)"""
    K = W.key_frames[kf]
    action, rep = [], []
    for q, s in zip(queries, best_idx):
        rep.append(None)
        if s < 0:
            action.append(FUSE_NO_MATCH)
            continue
        pMP, pMPinKF = W.points[q], K.GetMapPoint(s)
        if pMPinKF is not None:
            if not pMPinKF.isBad():
                rep[-1] = pMPinKF
                action.append(FUSE_REPLACE_REQUESTED)
            else:
                action.append(FUSE_KF_POINT_BAD)
        else:
            pMP.AddObservation(K, s)
            K.AddMapPoint(pMP, s)
            action.append(FUSE_ADDED)
    for q, pRep in zip(queries, rep):
        if pRep is not None:
            pRep.Replace(W.points[q])
    return action, [(-1 if r is None else r.index) for r in rep]


def lba_erase(W, pairs):
    """Optimizer.cc:748-757 for vToErase = (key frame, point) in the order of the edges"""
    for kf, p in pairs:
        K, P = W.key_frames[kf], W.points[p]
        K.EraseMapPointMatch(P)
        P.EraseObservation(K)


def loop_matches(W, cur_kf, matched):
    """LoopClosing.cc:520-537"""
    K = W.key_frames[cur_kf]
    for i, m in enumerate(matched):
        if m >= 0:
            pLoopMP, pCurMP = W.points[m], K.GetMapPoint(i)
            if pCurMP is not None:
                pCurMP.Replace(pLoopMP)
            else:
                K.AddMapPoint(pLoopMP, i)
                pLoopMP.AddObservation(K, i)
