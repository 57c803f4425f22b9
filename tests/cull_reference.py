"""A literal, object-level restatement of local mapping's two cullings of thirdparty/orb-slam2, in plain Python:
  LocalMapping::MapPointCulling                                   src/LocalMapping.cc:170-207
  LocalMapping::KeyFrameCulling                                   src/LocalMapping.cc:634-698
  KeyFrame::SetBadFlag, EraseConnection, ChangeParent, EraseMapPointMatch   src/KeyFrame.cc:556-648, :262-275, :509-514, :331-335
  MapPoint::EraseObservation, SetBadFlag                          src/MapPoint.cc:132-158, :172-187
Key frames and map points are objects; std::map<KeyFrame*, ..> and std::set<KeyFrame*> are dicts and sets ITERATED BY ADDRESS RANK
(KeyFrame.addr), on top of the key frame of tests/covis_reference.py (its map, its ordered list, UpdateBestCovisibles).  Nothing
here knows how csrc/culling.hip is organised.  `dirty_set_keyframe_culling` restates the walk as a pre-count of every member from
the input state plus a re-count of the members a cull touched; the tests hold it against the literal sequence.

Rules names every reading; MUTANTS flips one each, and tests/test_culling.py asserts that every mutant changes a compared output
on a case of tests/cull_cases.py named for it."""
import dataclasses

import numpy as np

import covis_reference as CR

MP_KEEP, MP_WAS_BAD, MP_FOUND_RATIO, MP_FEW_OBS, MP_AGED, MP_NONE = 0, 1, 2, 3, 4, 5
KF_KEEP, KF_CULLED, KF_TO_BE_ERASED, KF_ID0, KF_WAS_BAD, KF_NONE = 0, 1, 2, 3, 4, 5
ROW_ERASED, ROW_CLEARED, ROW_REPARENTED = 1, 2, 4
LIMIT, INFO = 32, 4


@dataclasses.dataclass(frozen=True)
class Rules:
    # KeyFrameCulling
    redundant_ge: bool = False           # nRedundantObservations >= 0.9*nMPs (:694)
    obs_ge: bool = False                 # Observations() >= thObs (:664)
    level_no_plus1: bool = False         # scaleLeveli <= scaleLevel (:677)
    self_counted: bool = False           # no pKFi == pKF skip (:673)
    th_two: bool = False                 # two observers at that scale are enough (:680, :685)
    bad_points_counted: bool = False     # no isBad() test at :654
    no_sequence: bool = False            # every member evaluated from the input state
    # MapPoint::EraseObservation / SetBadFlag
    bad_at_three: bool = False           # nObs <= 3 (MapPoint.cc:151)
    ref_kept: bool = False               # mpRefKF not moved (:147)
    slots_kept: bool = False             # no EraseMapPointMatch (:182-186)
    # KeyFrame::SetBadFlag
    own_slots_cleared: bool = False      # the culled key frame's mvpMapPoints cleared
    not_erase_ignored: bool = False      # mbNotErase not looked at (KeyFrame.cc:562)
    id0_culled: bool = False             # mnId == 0 neither skipped (:645) nor returned from (:560)
    no_resort: bool = False              # EraseConnection without UpdateBestCovisibles (:273)
    children_index_order: bool = False   # mspChildrens in index order
    candidates_not_grown: bool = False   # sParentCandidates.insert(pC) left out (:625)
    max_ge: bool = False                 # w >= max (:611): the last maximum wins
    leftover_keep_parent: bool = False   # no ChangeParent(mpParent) for the children that are left (:635-639)
    # MapPointCulling
    ratio_le: bool = False               # GetFoundRatio() <= 0.25f (:190)
    ratio_integer: bool = False          # 4*found < visible in integers
    few_obs_lt: bool = False             # Observations() < cnThObs (:196)
    age_gt: bool = False                 # > 2 and > 3 (:196, :202)
    tests_reordered: bool = False        # the age-out test before the two culling tests


REFERENCE = Rules()
KF_MUTANTS = {n: Rules(**{n: True}) for n in ("redundant_ge", "obs_ge", "level_no_plus1", "self_counted", "th_two", "bad_points_counted", "no_sequence",
                                               "bad_at_three", "ref_kept", "slots_kept", "own_slots_cleared", "not_erase_ignored", "id0_culled",
                                               "no_resort", "children_index_order", "candidates_not_grown", "max_ge", "leftover_keep_parent")}
MP_MUTANTS = {n: Rules(**{n: True}) for n in ("ratio_le", "ratio_integer", "few_obs_lt", "age_gt", "tests_reordered")}


class MapPoint:
    def __init__(self, idx, bad=False, first_kf_id=0, visible=1, found=1):
        self.idx, self.bad = idx, bad
        self.mObservations = {}                                        # KeyFrame -> keypoint index
        self.mpRefKF = None
        self.mnFirstKFid, self.mnVisible, self.mnFound = first_kf_id, visible, found

    def isBad(self):
        return self.bad

    def Observations(self):                                            # nObs, monocular: one per observation
        return len(self.mObservations)

    def GetObservations(self):
        return sorted(self.mObservations.items(), key=lambda kv: kv[0].addr)

    def GetFoundRatio(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.float32(self.mnFound) / np.float32(self.mnVisible)

    def EraseObservation(self, pKF, rules=REFERENCE):
        bBad = False
        if pKF in self.mObservations:
            del self.mObservations[pKF]
            if self.mpRefKF is pKF and not rules.ref_kept:
                obs = self.GetObservations()
                self.mpRefKF = obs[0][0] if obs else None              # the reference dereferences end(); None is this project's reading
            if self.Observations() <= (3 if rules.bad_at_three else 2):
                bBad = True
        if bBad:
            self.SetBadFlag(rules)

    def SetBadFlag(self, rules=REFERENCE):
        self.bad = True
        obs = self.GetObservations()
        self.mObservations = {}
        if rules.slots_kept:
            return
        for pKF, idx in obs:
            pKF.EraseMapPointMatch(idx)


class KeyFrame(CR.KeyFrame):
    def __init__(self, idx, addr, id0=False, bad=False, not_erase=False):
        super().__init__(idx, addr, id0, bad)
        self.octave = []                                               # mvKeysUn[i].octave
        self.mbNotErase, self.mbToBeErased = not_erase, False
        self.row_status = 0
        self.high_conn = self.high_ord = 0                             # the longest each row has been: what a rewrite pads up to

    def note_lengths(self):
        self.high_conn, self.high_ord = max(self.high_conn, len(self.weights)), max(self.high_ord, len(self.ordered))

    def EraseMapPointMatch(self, idx):
        self.mvpMapPoints[idx] = None

    def GetWeight(self, pKF):
        return self.weights.get(pKF, 0)

    def ChangeParent(self, pKF):
        self.parent = pKF
        self.row_status |= ROW_REPARENTED

    def EraseConnection(self, pKF, rules=REFERENCE):
        if pKF in self.weights:
            self.note_lengths()
            del self.weights[pKF]
            if not rules.no_resort:
                self.UpdateBestCovisibles(CR.REFERENCE, 0)
            self.note_lengths()
            self.row_status |= ROW_ERASED

    def SetBadFlag(self, kfs, rules=REFERENCE):
        """True when it ran to its end"""
        if self.id0 and not rules.id0_culled:
            return False
        if self.mbNotErase and not rules.not_erase_ignored:
            self.mbToBeErased = True
            return False
        for k in sorted(self.weights, key=lambda k: k.addr):
            k.EraseConnection(self, rules)
        for pMP in list(self.mvpMapPoints):
            if pMP is not None:
                pMP.EraseObservation(self, rules)
        if rules.own_slots_cleared:
            self.mvpMapPoints = [None] * len(self.mvpMapPoints)
        self.note_lengths()
        self.weights, self.ordered, self.ordered_w = {}, [], []
        self.row_status |= ROW_CLEARED
        # mspChildrens: the key frames whose parent this is.  The reference drops a culled child from the set (:640), the parent
        # pointer still names it: hence the isBad() test here and none at :599
        children = [c for c in kfs if c.parent is self and not c.isBad()]
        children.sort(key=(lambda c: c.idx) if rules.children_index_order else (lambda c: c.addr))
        sParentCandidates = [self.parent]
        while children:
            bContinue, mx, pC, pP = False, -1, None, None
            for pKF in children:
                for x in pKF.ordered:
                    for cand in sParentCandidates:
                        if cand is not None and x is cand:
                            w = pKF.GetWeight(x)
                            if w > mx or (rules.max_ge and w >= mx):
                                pC, pP, mx, bContinue = pKF, x, w, True
            if not bContinue:
                break
            pC.ChangeParent(pP)
            if not rules.candidates_not_grown:
                sParentCandidates.append(pC)
            children.remove(pC)
        if not rules.leftover_keep_parent:
            for c in children:
                c.ChangeParent(self.parent)
        self.bad = True
        return True


def evaluate(pKF, rules=REFERENCE):
    """(nMPs, nRedundantObservations) of LocalMapping.cc:646-691"""
    thObs = 3
    enough = 2 if rules.th_two else thObs
    nRedundantObservations = nMPs = 0
    for i, pMP in enumerate(pKF.mvpMapPoints):
        if pMP is None:
            continue
        if pMP.isBad() and not rules.bad_points_counted:
            continue
        nMPs += 1
        if (pMP.Observations() >= thObs) if rules.obs_ge else (pMP.Observations() > thObs):
            scaleLevel = pKF.octave[i]
            nObs = 0
            for pKFi, idx in pMP.GetObservations():
                if pKFi is pKF and not rules.self_counted:
                    continue
                if pKFi.octave[idx] <= scaleLevel + (0 if rules.level_no_plus1 else 1):
                    nObs += 1
                    if nObs >= enough:
                        break
            if nObs >= enough:
                nRedundantObservations += 1
    return nMPs, nRedundantObservations


def _decide(counts, rules):
    nMPs, nRed = counts
    return nRed >= 0.9 * nMPs if rules.redundant_ge else nRed > 0.9 * nMPs


def _finish(pKF, counts, kfs, rules, on_cull=None):
    if pKF.isBad():                                                    # a second SetBadFlag finds its maps and children empty
        return (pKF.idx, counts[0], counts[1], KF_WAS_BAD)
    if not _decide(counts, rules):
        return (pKF.idx, counts[0], counts[1], KF_KEEP)
    if on_cull is not None and not (pKF.mbNotErase and not rules.not_erase_ignored):
        on_cull(pKF)
    done = pKF.SetBadFlag(kfs, rules)
    return (pKF.idx, counts[0], counts[1], KF_CULLED if done else KF_TO_BE_ERASED)


def keyframe_culling(cur, kfs, rules=REFERENCE):
    """LocalMapping::KeyFrameCulling with mpCurrentKeyFrame = cur.  Returns the records (key frame, nMPs, nRedundant, action)."""
    for k in kfs:
        k.row_status = 0
        k.high_conn, k.high_ord = len(k.weights), len(k.ordered)
    vpLocalKeyFrames = list(cur.ordered)
    before = {k: evaluate(k, rules) for k in vpLocalKeyFrames} if rules.no_sequence else None
    records = []
    for pKF in vpLocalKeyFrames:
        if pKF.id0 and not rules.id0_culled:
            records.append((pKF.idx, -1, -1, KF_ID0))
            continue
        counts = before[pKF] if before is not None else evaluate(pKF, rules)
        records.append(_finish(pKF, counts, kfs, rules))
    return records


def dirty_set_keyframe_culling(cur, kfs):
    """The same walk with every member counted up front from the input state, and counted again only when a cull touched it: a
    member's counts can change only through a point that a culled key frame also held, so SetBadFlag marks every observer of the
    culled key frame's points (and, for maps whose slots and lists disagree, every holder) dirty."""
    for k in kfs:
        k.row_status = 0
        k.high_conn, k.high_ord = len(k.weights), len(k.ordered)
    lst = list(cur.ordered)
    before = {k: evaluate(k) for k in lst}
    dirty = set()

    def on_cull(pKF):
        touched = {p for p in pKF.mvpMapPoints if p is not None}
        for p in touched:
            dirty.update(p.mObservations)
        for k in kfs:
            if any(p in touched for p in k.mvpMapPoints):
                dirty.add(k)
    records = []
    for pKF in lst:
        if pKF.id0:
            records.append((pKF.idx, -1, -1, KF_ID0))
            continue
        counts = evaluate(pKF) if pKF in dirty else before[pKF]
        records.append(_finish(pKF, counts, kfs, REFERENCE, on_cull))
    return records


def map_point_culling(recent, cur_kf_id, th_obs=2, rules=REFERENCE):
    """LocalMapping::MapPointCulling over mlpRecentAddedMapPoints = recent.  Returns (actions, the surviving list)."""
    actions, kept = [], []
    for pMP in recent:
        age = int(cur_kf_id) - int(pMP.mnFirstKFid)
        ratio = pMP.GetFoundRatio()
        if rules.ratio_integer:
            low = 4 * pMP.mnFound < pMP.mnVisible
        else:
            low = bool(ratio <= np.float32(0.25)) if rules.ratio_le else bool(ratio < np.float32(0.25))
        few = pMP.Observations() < th_obs if rules.few_obs_lt else pMP.Observations() <= th_obs
        old2, old3 = (age > 2, age > 3) if rules.age_gt else (age >= 2, age >= 3)
        if pMP.isBad():
            act = MP_WAS_BAD
        elif rules.tests_reordered and old3:
            act = MP_AGED
        elif low:
            act = MP_FOUND_RATIO
        elif old2 and few:
            act = MP_FEW_OBS
        elif old3:
            act = MP_AGED
        else:
            act = MP_KEEP
        if act in (MP_FOUND_RATIO, MP_FEW_OBS):
            pMP.SetBadFlag(rules)
        if act == MP_KEEP:
            kept.append(pMP)
        actions.append(act)
    return actions, kept


def compact_observations(obs_start, obs_frame, obs_idx, obs_live, ref_obs):
    """the plain loop pgorb_compact_observations_device is held against"""
    start, frame, idx, ref = [0], [], [], []
    for p in range(len(obs_start) - 1):
        r = -1
        for o in range(obs_start[p], obs_start[p + 1]):
            if obs_live[o]:
                if o - obs_start[p] == ref_obs[p]:
                    r = len(frame) - start[p]
                frame.append(int(obs_frame[o]))
                idx.append(int(obs_idx[o]))
        start.append(len(frame))
        ref.append(r)
    return np.array(start, np.int32), np.array(frame, np.int32), np.array(idx, np.int32), np.array(ref, np.int32)
