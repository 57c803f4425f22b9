"""Worlds for the cullings (tests/test_culling.py): a map in plain lists on top of the World of tests/covis_cases.py (octaves, the
keypoint index and the live flag of every observation, the reference key frame, mbNotErase), the conversion to the objects of
tests/cull_reference.py and to the arrays of include/pgorb.h, constructed cases by name, seeded random worlds, and the runners
(reference, host form, device form)."""
import copy
import ctypes as C
import random

import numpy as np

import covis_cases as CC
import cull_reference as CU

FILL, SENT = CC.FILL, -9                    # unused row entries on entry; output arrays before the call
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


class World(CC.World):
    def __init__(self, nkf, order=None, id0=None):
        super().__init__(nkf, order, id0)
        self.octv = [[] for _ in range(nkf)]
        self.obs_idx, self.live, self.ref = [], [], []
        self.first_kf_id, self.visible, self.found = [], [], []
        self.not_erase, self.to_be_erased = [False] * nkf, [False] * nkf

    def point(self, observers, octave=0, bad=False, ref_kf=None, dead=(), first=0, visible=1, found=1):
        """a point observed by `observers`, listed in ADDRESS order, in a fresh slot of each; octave: one value or {key frame:
        octave}; ref_kf: mpRefKF (default: the first of the list); dead: the observers whose observation is already erased"""
        obs = sorted(observers, key=self.rank)
        p = len(self.obs)
        self.obs.append(obs)
        self.point_bad.append(bad)
        self.obs_idx.append([len(self.slots[f]) for f in obs])
        for f in obs:
            self.slots[f].append(p)
            self.octv[f].append(octave[f] if isinstance(octave, dict) else octave)
        self.live.append([f not in dead for f in obs])
        self.ref.append(-1 if not obs else 0 if ref_kf is None else obs.index(ref_kf))
        self.first_kf_id.append(first)
        self.visible.append(visible)
        self.found.append(found)
        return p

    def hole(self, f, count=1):
        self.slots[f] += [-1] * count
        self.octv[f] += [0] * count

    def link(self, i, j, wij, wji=None, ordered=True):
        """a connection in both rows"""
        self.connect(i, j, wij, ordered)
        self.connect(j, i, wij if wji is None else wji, ordered)

    def sort_lists(self):
        """every ordered list as UpdateBestCovisibles leaves it: descending (weight, address)"""
        for f in range(self.nkf):
            self.ordl[f].sort(key=lambda jw: (jw[1], self.rank(jw[0])), reverse=True)


def objects(w):
    kfs = [CU.KeyFrame(f, w.rank(f), w.id0[f], w.kf_bad[f], w.not_erase[f]) for f in range(w.nkf)]
    pts = [CU.MapPoint(p, w.point_bad[p], w.first_kf_id[p], w.visible[p], w.found[p]) for p in range(len(w.obs))]
    for p, pt in enumerate(pts):
        for f, i, alive in zip(w.obs[p], w.obs_idx[p], w.live[p]):
            if alive:
                pt.mObservations[kfs[f]] = i
        pt.mpRefKF = kfs[w.obs[p][w.ref[p]]] if w.ref[p] >= 0 else None
    for f, k in enumerate(kfs):
        k.mvpMapPoints = [pts[p] if p >= 0 else None for p in w.slots[f]]
        k.octave = list(w.octv[f])
        k.weights = {kfs[j]: x for j, x in w.conn[f].items()}
        k.ordered, k.ordered_w = [kfs[j] for j, _ in w.ordl[f]], [x for _, x in w.ordl[f]]
        k.parent = kfs[w.parent[f]] if w.parent[f] >= 0 else None
        k.mbToBeErased = w.to_be_erased[f]
    return kfs, pts


def arrays(w, conn_cap):
    """every input of the two cullings as the arrays of include/pgorb.h"""
    a = CC.table_arrays(w)
    cap, nkf, m = a["cap"], max(w.nkf, 1), a["nobs"]
    kps = np.zeros((nkf, cap), KEYPOINT_DTYPE)
    kps["octave"] = 99                                                  # past n[f]: never read
    for f, o in enumerate(w.octv):
        kps["octave"][f, :len(o)] = o
    flat = lambda rows, dt: np.array([x for r in rows for x in r] + [0], dt)
    a.update(kps=kps, point_bad=np.array(w.point_bad + [0], np.uint8), obs_idx=flat(w.obs_idx, np.int32), obs_live=flat(w.live, np.uint8),
             ref_obs=np.array(w.ref + [0], np.int32), not_erase=np.array(w.not_erase + [0], np.uint8),
             to_be_erased=np.array(w.to_be_erased + [0], np.uint8), first_kf_id=np.array(w.first_kf_id + [0], np.int32),
             visible=np.array(w.visible + [0], np.int32), found=np.array(w.found + [0], np.int32))
    a["obs_frame"] = a["obs_frame"][:m + 1]
    a.update(CC.state_arrays(w, conn_cap))
    return a


def _table_after(w, a, kfs, pts):
    """the slots, the bad flags, the mask and ref_obs as the objects stand"""
    e = {k: a[k].copy() for k in ("kf_point", "point_bad", "obs_live", "ref_obs")}
    for f, k in enumerate(kfs):
        e["kf_point"][f, :len(k.mvpMapPoints)] = [p.idx if p is not None else -1 for p in k.mvpMapPoints]
    o = 0
    for p, pt in enumerate(pts):
        e["point_bad"][p] = pt.bad
        for f in w.obs[p]:
            e["obs_live"][o] = kfs[f] in pt.mObservations
            o += 1
        e["ref_obs"][p] = w.obs[p].index(pt.mpRefKF.idx) if pt.mpRefKF is not None and pt.mpRefKF.idx in w.obs[p] else -1
    return e


class KfCase:
    def __init__(self, name, world, cur, list_cap=None, conn_cap=None):
        self.name, self.w, self.cur, self.list_cap, self.conn_cap = name, world, cur, list_cap, conn_cap


KF_KEYS = ("kf_point", "point_bad", "obs_live", "ref_obs", "kf_bad", "to_be_erased", "conn_kf", "conn_w", "nconn", "ord_kf", "ord_w", "nord",
           "parent", "row_status", "record", "info")


def expected_kf(c, rules=CU.REFERENCE, dirty=False):
    """What pgorb_keyframe_culling leaves: every in/out and output array after the literal sequence (or its dirty-set form)."""
    w = c.w
    conn_cap = c.conn_cap if c.conn_cap is not None else max([len(m) for m in w.conn] + [1])
    nl = len(w.ordl[c.cur])
    list_cap = c.list_cap if c.list_cap is not None else nl + 1
    a = arrays(w, conn_cap)
    e = {k: a[k].copy() for k in ("kf_point", "point_bad", "obs_live", "ref_obs", "kf_bad", "to_be_erased", "conn_kf", "conn_w", "nconn", "ord_kf",
                                  "ord_w", "nord", "parent")}
    e.update(row_status=np.full(max(w.nkf, 1), SENT, np.int32), record=np.full((list_cap, 4), SENT, np.int32), conn_cap=conn_cap, list_cap=list_cap,
             inputs=a)
    if nl > list_cap:
        e["info"] = np.array([CU.LIMIT, nl, 0, 0], np.int32)
        return e
    kfs, pts = objects(w)
    rec = CU.dirty_set_keyframe_culling(kfs[c.cur], kfs) if dirty else CU.keyframe_culling(kfs[c.cur], kfs, rules)
    e.update(_table_after(w, a, kfs, pts))
    for f, k in enumerate(kfs):
        e["kf_bad"][f], e["to_be_erased"][f], e["row_status"][f] = k.bad, k.mbToBeErased, k.row_status
        e["parent"][f] = k.parent.idx if k.parent is not None else -1
        if k.row_status & (CU.ROW_ERASED | CU.ROW_CLEARED):
            row = sorted(k.weights.items(), key=lambda kw: kw[0].addr)
            e["conn_kf"][f, :k.high_conn], e["conn_w"][f, :k.high_conn] = -1, 0
            e["ord_kf"][f, :k.high_ord], e["ord_w"][f, :k.high_ord] = -1, 0
            e["nconn"][f], e["nord"][f] = len(row), len(k.ordered)
            e["conn_kf"][f, :len(row)], e["conn_w"][f, :len(row)] = [j.idx for j, _ in row], [x for _, x in row]
            e["ord_kf"][f, :len(k.ordered)], e["ord_w"][f, :len(k.ordered)] = [j.idx for j in k.ordered], k.ordered_w
    e["record"][:len(rec)] = rec
    went = sum(1 for p, pt in enumerate(pts) if pt.bad and not w.point_bad[p])
    e["info"] = np.array([0, len(rec), sum(r[3] == CU.KF_CULLED for r in rec), went], np.int32)
    e["kfs"] = kfs
    return e


def same(x, y, keys, nkf=None):
    return all(np.array_equal(np.asarray(x[k]), np.asarray(y[k])) for k in keys)


def diff(x, y, keys):
    return [k for k in keys if not np.array_equal(np.asarray(x[k]), np.asarray(y[k]))]


class MpCase:
    def __init__(self, name, world, recent, cur_kf_id, th_obs=2):
        self.name, self.w, self.recent, self.cur_kf_id, self.th_obs = name, world, list(recent), cur_kf_id, th_obs


MP_KEYS = ("kf_point", "point_bad", "obs_live", "action", "recent_out", "nrecent_out", "info")


def expected_mp(c, rules=CU.REFERENCE):
    w = c.w
    a = arrays(w, max([len(m) for m in w.conn] + [1]))
    kfs, pts = objects(w)
    actions, kept = CU.map_point_culling([pts[p] for p in c.recent], c.cur_kf_id, c.th_obs, rules)
    e = _table_after(w, a, kfs, pts)
    del e["ref_obs"]
    out = np.full(max(len(c.recent), 1), SENT, np.int32)
    out[:len(kept)] = [p.idx for p in kept]
    e.update(action=np.array(actions + ([SENT] if not actions else []), np.int32), recent_out=out, nrecent_out=np.array([len(kept)], np.int32),
             info=np.array([0, len(kept), sum(x in (CU.MP_FOUND_RATIO, CU.MP_FEW_OBS) for x in actions), 0], np.int32), inputs=a)
    return e


# ---------------------------------------------------------------- constructed cases
def _member_world(nkf=6, order=None):
    """cur = nkf - 1 lists member 1; key frames 2, 3, 4 support; key frame 0 is the mnId == 0 root of the tree 0 <- 1 <- .. """
    w = World(nkf, order, [f == 0 for f in range(nkf)])
    w.parent = [-1] + list(range(nkf - 1))
    w.first = [False] * nkf
    w.link(nkf - 1, 1, 20)
    return w


def _decision(nred, ntotal, empty=0):
    w = _member_world()
    w.share([1, 2, 3, 4], nred)
    w.share([1, 2], ntotal - nred)
    w.hole(1, empty)
    return w


def kf_cases():
    out = []
    add = lambda name, w, cur=None, **kw: out.append(KfCase(name, w, w.nkf - 1 if cur is None else cur, **kw))
    # the decision nRedundant > 0.9 * nMPs in double
    add("nine_of_ten", _decision(9, 10))
    add("ten_of_eleven", _decision(10, 11, empty=2))
    add("no_points", _decision(0, 0, empty=3))
    # Observations() > 3: three live observers that are all other key frames (the member's own observation is already erased)
    w = _member_world()
    w.share([1, 2, 3, 4], 4, dead=(1,))
    add("three_foreign_observers", w)
    # the octave test: <= level + 1
    w = _member_world()
    w.share([1, 2, 3, 4], 4, octave={1: 1, 2: 2, 3: 2, 4: 0})
    add("octave_plus_one", w)
    # two fine observers and a coarse one: the member itself is not counted, and two are not enough
    w = _member_world()
    w.share([1, 2, 3, 4], 4, octave={1: 0, 2: 1, 3: 0, 4: 2})
    add("two_fine_observers", w)
    # bad points in the member's slots do not count into nMPs
    w = _member_world()
    w.share([1, 2, 3, 4], 10)
    for _ in range(3):
        p = w.point([1, 2], bad=True, dead=(1, 2))
        assert w.slots[1][-1] == p
    add("bad_points_in_slots", w)
    # two members, each redundant only while the other lives
    w = _member_world(7)
    w.link(6, 2, 10)
    w.share([1, 2, 3, 4], 5)
    w.sort_lists()
    add("mutually_redundant", w)
    # a cull takes points to two observers (and, for the mutant, to three): a later member loses slots, its nMPs changes
    w = _member_world(7)
    w.link(6, 2, 10)
    w.share([1, 2, 3, 4, 5], 20)
    w.share([1, 2, 3], 1)
    w.share([1, 2, 3, 4], 1, octave={1: 0, 2: 0, 3: 0, 4: 5})
    w.share([2, 3], 2)
    w.sort_lists()
    add("third_loses_slot", w)
    # the reference key frame culled: first in its list, in the middle of it, and with nothing live left besides two
    w = _member_world(7, order=[3, 2, 6, 0, 5, 1, 4])
    w.share([1, 2, 3, 4], 8, ref_kf=1)
    w.share([1, 2, 3, 4, 5], 3, ref_kf=1)
    w.share([1, 2, 3, 4], 2, ref_kf=3)
    w.share([1, 2, 3], 1, ref_kf=1)
    add("reference_culled", w)
    # mbNotErase, mnId == 0
    w = _decision(10, 10)
    w.not_erase[1] = True
    add("not_erase_member", w)
    w = _decision(10, 10)
    w.id0, w.parent = [False, True] + [False] * 4, [-1, -1, 1, 2, 3, 4]
    add("id0_member", w)
    # a member that is already bad: counted, recorded, nothing written
    w = _decision(10, 10)
    w.kf_bad[1] = True
    add("bad_member", w)
    # the spanning tree: a child linked to the parent, one linked only to the first child, one linked to nobody
    w = _member_world(9)
    w.share([1, 2, 3, 4], 6)
    w.parent = [-1, 0, 0, 0, 0, 1, 1, 1, 4]
    w.link(5, 0, 7); w.link(6, 5, 9); w.link(6, 2, 30); w.link(7, 3, 4)
    w.sort_lists()
    add("three_children", w)
    # tied weights among the children, under an address order that is not the index order
    w = _member_world(8, order=[0, 1, 2, 3, 4, 6, 5, 7])
    w.share([1, 2, 3, 4], 6)
    w.parent = [-1, 0, 0, 0, 0, 1, 1, 4]
    w.link(5, 0, 5); w.link(6, 0, 5); w.link(5, 6, 9)
    w.sort_lists()
    add("tied_children", w)
    # a thresholded ordered row (fewer entries than its map) that grows on the re-sort; an asymmetric connection on either side
    w = _member_world(8)
    w.share([1, 2, 3, 4], 6)
    w.link(2, 1, 20); w.link(2, 3, 16); w.link(2, 4, 3, ordered=False); w.link(2, 5, 2, ordered=False)
    w.connect(1, 6, 4)                                                  # 1's map holds 6, 6's row does not hold 1
    w.connect(5, 1, 3); w.connect(5, 6, 8)                              # 5's row holds 1, 1's map does not hold 5
    w.sort_lists()
    add("thresholded_row_grows", w)
    # list_cap exact and one short
    w = _member_world(7)
    w.link(6, 2, 10); w.link(6, 3, 5)
    w.share([1, 2, 3, 4], 5)
    w.sort_lists()
    add("list_cap_exact", w, list_cap=3)
    add("list_cap_one_short", copy.deepcopy(w), list_cap=2)
    return out


def stride_world():
    """shapes that cross the kernel's strides: a member with 300 slots, a point with 70 observers, a culled key frame with 70
    connections and children on both sides of the tree repair"""
    nkf = 80
    w = World(nkf, order=[(7 * f + 3) % nkf for f in range(nkf)], id0=[f == 0 for f in range(nkf)])
    w.parent = [-1, 0] + [1] * 6 + [0] * (nkf - 8)
    w.first = [False] * nkf
    r = random.Random(5)
    for _ in range(290):
        w.point([1] + r.sample(range(2, nkf - 1), 3), octave=r.randint(0, 1))
    w.share([1, 2, 3], 4)
    w.hole(1, 5)
    w.point(list(range(1, 71)))
    assert len(w.slots[1]) == 300
    for j in range(2, 72):
        w.link(1, j, 1 + (j * 5) % 9, ordered=j % 3 != 0)
    w.link(nkf - 1, 1, 30); w.link(nkf - 1, 2, 12); w.link(nkf - 1, 3, 8)
    w.link(2, 0, 6); w.link(3, 2, 4); w.link(4, 3, 4); w.link(5, 0, 6, ordered=False)
    w.sort_lists()
    return KfCase("strides", w, nkf - 1)


def _mp_world():
    w = World(5)
    mk = lambda nobs, **kw: w.point(list(range(nobs)), **kw)
    return w, mk


def mp_cases():
    out = []

    def one(name, cur, th=2, **kw):
        w, mk = _mp_world()
        nobs = kw.pop("nobs", 4)
        p = mk(nobs, **kw)
        mk(3, first=cur, visible=4, found=4)                            # a neighbour that stays
        out.append(MpCase(name, w, [p, p + 1], cur, th))
    one("ratio_quarter_exact", 10, first=10, visible=4, found=1)
    one("ratio_float_rounding", 10, first=10, visible=(1 << 26) + 1, found=1 << 24)
    one("ratio_below", 10, first=10, visible=9, found=2)
    one("visible_zero_found_zero", 10, first=10, visible=0, found=0)
    one("visible_zero_found_one", 10, first=10, visible=0, found=1)
    one("few_obs_edge", 12, first=10, visible=4, found=4, nobs=2)
    one("few_obs_three", 12, first=10, visible=4, found=4, nobs=3)
    one("age_one_few_obs", 11, first=10, visible=4, found=4, nobs=1)
    one("aged_out", 13, first=10, visible=4, found=4, nobs=4)
    one("aged_low_ratio", 13, first=10, visible=40, found=4, nobs=4)
    one("was_bad", 10, first=10, visible=40, found=4, bad=True, dead=(0, 1, 2, 3))
    one("dead_observations", 12, first=10, visible=4, found=4, nobs=4, dead=(0, 3))
    # one list with every action, and a point with 70 observers (more than a wave)
    w = World(72)
    acts = [w.point([0, 1, 2, 3], first=10, visible=4, found=4), w.point([0, 1], first=9, visible=4, found=4), w.point([2, 3, 4], first=10, visible=40, found=1),
            w.point([1, 2, 3], first=7, visible=4, found=4), w.point([0, 4], bad=True, dead=(0, 4), first=10),
            w.point(list(range(1, 71)), first=11, visible=400, found=3), w.point([5, 6, 7], first=11, visible=4, found=2)]
    out.append(MpCase("every_action", w, acts, 11))
    return out


# ---------------------------------------------------------------- seeded random worlds
def grow_tree(w):
    """the parents an incremental map has: the best covisible among the EARLIER key frames, else the one before"""
    for f in range(w.nkf):
        earlier = [j for j, _ in w.ordl[f] if j < f]
        w.parent[f] = -1 if f == 0 else earlier[0] if earlier else f - 1
        w.first[f] = False


def random_world(seed):
    r = random.Random(seed)
    nkf, npts, cap = r.randint(4, 12), r.randint(12, 48), 16
    order = None if r.random() < 0.3 else r.sample(range(nkf), nkf)
    w = World(nkf, order, [f == 0 for f in range(nkf)])
    dense = r.random() < 0.7
    for _ in range(npts):
        k = min((3 if r.random() < 0.08 else r.randint(4, 8)) if dense else r.randint(2, 6), nkf)
        fs = [f for f in r.sample(range(nkf), k) if len(w.slots[f]) < cap - 1]
        if fs:
            w.point(fs, octave={f: r.randint(0, 2) for f in fs}, ref_kf=r.choice(fs))
    for f in range(nkf):
        if r.random() < 0.3 and len(w.slots[f]) < cap:
            w.hole(f)
    CC._settle(w, r.choice([1, 2, 3]))
    grow_tree(w)
    for p in range(len(w.obs)):                                        # a few observations already erased, a few bad points left in slots
        if r.random() < 0.08:
            k = r.randrange(len(w.obs[p]))
            w.live[p][k] = False
        if r.random() < 0.04:
            w.point_bad[p], w.live[p] = True, [False] * len(w.obs[p])
    for f in range(1, nkf):
        w.not_erase[f] = r.random() < 0.06
        w.kf_bad[f] = r.random() < 0.03
    return KfCase("random%d" % seed, w, nkf - 1)


def random_mp(seed):
    c = random_world(seed)
    r = random.Random(seed + 10 ** 6)
    w = c.w
    n = len(w.obs)
    cur = r.randint(3, 9)
    for p in range(n):
        w.first_kf_id[p] = cur - r.choice([0, 0, 1, 2, 2, 3, 4])
        w.visible[p] = r.choice([0, 1, 4, 8, 8, 40])
        w.found[p] = r.choice([0, 1, 2, 2, 8, 10])
    return MpCase("random%d" % seed, w, r.sample(range(n), r.randint(0, n)), cur, r.choice([2, 2, 3]))


# ---------------------------------------------------------------- runners
dev, ptr = CC.dev, CC.ptr
TABLE_IN = ("kps", "kf_point", "n", "point_bad", "obs_start", "obs_frame", "obs_idx", "obs_live", "ref_obs", "order", "id0", "not_erase", "kf_bad",
            "to_be_erased", "first_kf_id", "visible", "found", "conn_kf", "conn_w", "nconn", "ord_kf", "ord_w", "nord", "parent")


def upload(a):
    import torch
    d = {}
    for k in TABLE_IN:
        v = a[k]
        d[k] = None if v is None else torch.from_numpy(np.frombuffer(v.tobytes(), np.uint8).copy()).cuda() if v.dtype == KEYPOINT_DTYPE else dev(v)
    return d


def run_device_kf(c, ext, e, d=None, stream=None):
    """pgorb_keyframe_culling_device on torch tensors; returns the tensors (for a chain)"""
    import torch
    w, a = c.w, e["inputs"]
    d = upload(a) if d is None else d
    full = lambda *shape: torch.full(shape, SENT, dtype=torch.int32, device="cuda")
    d.update(row_status=full(max(w.nkf, 1) + 2), record=full(e["list_cap"] + 2, 4), info=full(CU.INFO))
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = ext._L.pgorb_keyframe_culling_device(
        ext._h, ptr(d["kps"]), ptr(d["kf_point"]), ptr(d["n"]), w.nkf, a["cap"], len(w.obs), ptr(d["point_bad"]), ptr(d["obs_start"]), ptr(d["obs_frame"]),
        ptr(d["obs_idx"]), a["nobs"], ptr(d["obs_live"]), ptr(d["ref_obs"]), ptr(d["order"]), ptr(d["id0"]), ptr(d["not_erase"]), ptr(d["kf_bad"]),
        ptr(d["to_be_erased"]), c.cur, e["conn_cap"], ptr(d["conn_kf"]), ptr(d["conn_w"]), ptr(d["nconn"]), ptr(d["ord_kf"]), ptr(d["ord_w"]),
        ptr(d["nord"]), ptr(d["parent"]), e["list_cap"], ptr(d["record"]), ptr(d["row_status"]), ptr(d["info"]), C.c_void_p(s.cuda_stream))
    assert rc == 0, (rc, ext._L.pgorb_last_error(ext._h))
    return d


def download_kf(d, e):
    import torch
    torch.cuda.synchronize()
    out = {k: d[k].cpu().numpy() for k in KF_KEYS}
    assert np.all(out["row_status"][-2:] == SENT) and np.all(out["record"][-2:] == SENT), "wrote past an output array"
    out["row_status"], out["record"] = out["row_status"][:-2], out["record"][:-2]
    return out


def run_host_kf(c, ext, e):
    """pgorb_keyframe_culling itself (not the Python mirror, which hides the untouched bytes) on copies of the inputs"""
    w, a = c.w, e["inputs"]
    h = {k: (None if a[k] is None else a[k].copy()) for k in TABLE_IN}
    nkf = w.nkf
    kp, sl = (C.c_void_p * max(nkf, 1))(), (C.c_void_p * max(nkf, 1))()
    for f in range(nkf):
        kp[f], sl[f] = h["kps"][f].ctypes.data, h["kf_point"][f].ctypes.data
    h.update(row_status=np.full(max(nkf, 1), SENT, np.int32), record=np.full((e["list_cap"], 4), SENT, np.int32), info=np.full(CU.INFO, SENT, np.int32))
    p = lambda k: None if h[k] is None else C.c_void_p(h[k].ctypes.data)
    rc = ext._L.pgorb_keyframe_culling(
        ext._h, nkf, kp, sl, p("n"), len(w.obs), p("point_bad"), p("obs_start"), p("obs_frame"), p("obs_idx"), p("obs_live"), p("ref_obs"), p("order"),
        p("id0"), p("not_erase"), p("kf_bad"), p("to_be_erased"), c.cur, e["conn_cap"], p("conn_kf"), p("conn_w"), p("nconn"), p("ord_kf"), p("ord_w"),
        p("nord"), p("parent"), e["list_cap"], p("record"), p("row_status"), p("info"))
    assert rc >= 0 and rc == (0 if h["info"][0] else h["info"][2]), (rc, ext._L.pgorb_last_error(ext._h))
    return h


def run_device_mp(c, ext, e, stream=None):
    import torch
    w, a = c.w, e["inputs"]
    d = upload(a)
    nr = len(c.recent)
    full = lambda *shape: torch.full(shape, SENT, dtype=torch.int32, device="cuda")
    d.update(recent=dev(np.array(c.recent + [0], np.int32)), action=full(max(nr, 1) + 2), recent_out=full(max(nr, 1) + 2), nrecent_out=full(3), info=full(CU.INFO))
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = ext._L.pgorb_map_point_culling_device(
        ext._h, ptr(d["kf_point"]), ptr(d["n"]), w.nkf, a["cap"], len(w.obs), ptr(d["point_bad"]), ptr(d["obs_start"]), ptr(d["obs_frame"]),
        ptr(d["obs_idx"]), a["nobs"], ptr(d["obs_live"]), ptr(d["first_kf_id"]), ptr(d["visible"]), ptr(d["found"]), nr, ptr(d["recent"]), c.cur_kf_id,
        c.th_obs, ptr(d["action"]), ptr(d["recent_out"]), ptr(d["nrecent_out"]), ptr(d["info"]), C.c_void_p(s.cuda_stream))
    assert rc == 0, (rc, ext._L.pgorb_last_error(ext._h))
    return d


def download_mp(d, c):
    import torch
    torch.cuda.synchronize()
    out = {k: d[k].cpu().numpy() for k in MP_KEYS}
    nr = max(len(c.recent), 1)
    assert np.all(out["action"][nr:] == SENT) and np.all(out["recent_out"][nr:] == SENT) and np.all(out["nrecent_out"][1:] == SENT), "wrote past an output array"
    out["action"], out["recent_out"], out["nrecent_out"] = out["action"][:nr], out["recent_out"][:nr], out["nrecent_out"][:1]
    return out


def run_host_mp(c, ext, e):
    w, a = c.w, e["inputs"]
    h = {k: (None if a[k] is None else a[k].copy()) for k in TABLE_IN}
    nkf, nr = w.nkf, len(c.recent)
    sl = (C.c_void_p * max(nkf, 1))()
    for f in range(nkf):
        sl[f] = h["kf_point"][f].ctypes.data
    h.update(recent=np.array(c.recent + [0], np.int32), action=np.full(max(nr, 1), SENT, np.int32), recent_out=np.full(max(nr, 1), SENT, np.int32),
             nrecent_out=np.full(1, SENT, np.int32), info=np.full(CU.INFO, SENT, np.int32))
    p = lambda k: C.c_void_p(h[k].ctypes.data)
    rc = ext._L.pgorb_map_point_culling(
        ext._h, nkf, sl, p("n"), len(w.obs), p("point_bad"), p("obs_start"), p("obs_frame"), p("obs_idx"), p("obs_live"), p("first_kf_id"), p("visible"),
        p("found"), nr, p("recent"), c.cur_kf_id, c.th_obs, p("action"), p("recent_out"), p("nrecent_out"), p("info"))
    assert rc == h["info"][2], (rc, ext._L.pgorb_last_error(ext._h))
    return h
