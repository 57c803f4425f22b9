"""Worlds for the covisibility graph (tests/test_covisibility.py, tests/test_update_local_map.py): a map in plain lists, the
conversion to the objects of tests/covis_reference.py and to the arrays of include/pgorb.h, constructed cases by name, seeded
random worlds, and the runners (reference, single call, device form)."""
import copy
import ctypes as C
import random

import numpy as np

import covis_reference as CR

FILL = -7                                   # what unused row entries hold on entry: a write past a count shows


class World:
    def __init__(self, nkf, order=None, id0=None):
        self.nkf, self.order = nkf, order
        self.id0 = list(id0) if id0 is not None else [False] * nkf
        self.kf_bad = [False] * nkf
        self.slots = [[] for _ in range(nkf)]
        self.obs, self.point_bad = [], []
        self.conn = [dict() for _ in range(nkf)]
        self.ordl = [[] for _ in range(nkf)]
        self.parent, self.first = [-1] * nkf, [True] * nkf

    def point(self, observers, holders=None, bad=False):
        """a point observed by `observers` (in that list order) and held in one slot of each of `holders` (default: the observers)"""
        p = len(self.obs)
        self.obs.append(list(observers))
        self.point_bad.append(bad)
        for f in (observers if holders is None else holders):
            self.slots[f].append(p)
        return p

    def share(self, kfs, count, **kw):
        return [self.point(kfs, **kw) for _ in range(count)]

    def rank(self, f):
        return f if self.order is None else self.order[f]

    def connect(self, i, j, w, ordered=True):
        self.conn[i][j] = w
        if ordered:
            self.ordl[i].append((j, w))


def objects(w):
    kfs = [CR.KeyFrame(f, w.rank(f), w.id0[f], w.kf_bad[f]) for f in range(w.nkf)]
    pts = [CR.MapPoint(p, w.point_bad[p]) for p in range(len(w.obs))]
    for p, o in enumerate(w.obs):
        pts[p].observations = [kfs[f] for f in o]
    for f, k in enumerate(kfs):
        k.mvpMapPoints = [pts[p] if p >= 0 else None for p in w.slots[f]]
        k.weights = {kfs[j]: x for j, x in w.conn[f].items()}
        k.ordered, k.ordered_w = [kfs[j] for j, _ in w.ordl[f]], [x for _, x in w.ordl[f]]
        k.parent = kfs[w.parent[f]] if w.parent[f] >= 0 else None
        k.first = w.first[f]
    return kfs, pts


def table_arrays(w, cap=None):
    cap = max([len(s) for s in w.slots] + [1]) if cap is None else cap
    kf_point = np.full((max(w.nkf, 1), cap), -1, np.int32)
    for f, s in enumerate(w.slots):
        kf_point[f, :len(s)] = s
    n = np.array([len(s) for s in w.slots] + ([0] if not w.nkf else []), np.int32)
    st = np.zeros(len(w.obs) + 1, np.int32)
    st[1:] = np.cumsum([len(o) for o in w.obs])
    of = np.array([f for o in w.obs for f in o] + [0], np.int32)
    return dict(kf_point=kf_point, n=n, cap=cap, obs_start=st, obs_frame=of, nobs=int(st[-1]), point_bad=np.array(w.point_bad + [0], np.uint8),
                kf_bad=np.array(w.kf_bad + [0], np.uint8), order=None if w.order is None else np.array(w.order, np.int32),
                id0=np.array(w.id0 + [0], np.uint8))


def state_arrays(w, conn_cap):
    k1 = max(w.nkf, 1)
    a = dict(conn_kf=np.full((k1, conn_cap), FILL, np.int32), conn_w=np.full((k1, conn_cap), FILL, np.int32), nconn=np.zeros(k1, np.int32),
             ord_kf=np.full((k1, conn_cap), FILL, np.int32), ord_w=np.full((k1, conn_cap), FILL, np.int32), nord=np.zeros(k1, np.int32),
             parent=np.array(w.parent + ([-1] if not w.nkf else []), np.int32), first=np.array(w.first + ([1] if not w.nkf else []), np.uint8))
    for f in range(w.nkf):
        row = sorted(w.conn[f].items(), key=lambda jw: w.rank(jw[0]))
        a["nconn"][f], a["nord"][f] = len(row), len(w.ordl[f])
        a["conn_kf"][f, :len(row)], a["conn_w"][f, :len(row)] = [j for j, _ in row], [x for _, x in row]
        a["ord_kf"][f, :len(w.ordl[f])], a["ord_w"][f, :len(w.ordl[f])] = [j for j, _ in w.ordl[f]], [x for _, x in w.ordl[f]]
    return a


class GraphCase:
    def __init__(self, name, world, lst, th=15, conn_cap=None, loop_cap=None):
        self.name, self.w, self.lst, self.th = name, world, list(lst), th
        self.conn_cap, self.loop_cap = conn_cap, loop_cap


def expected_update(c, rules=CR.REFERENCE, decomposed=False):
    """What pgorb_update_connections leaves: the arrays after the literal sequence (or the closed form), under the capacities."""
    w = c.w
    kfs, _ = objects(w)
    lst = [kfs[i] for i in c.lst]
    loop = CR.decomposed_update_connections(kfs, lst, c.th) if decomposed else CR.correct_loop_connections(kfs, lst, c.th, rules)
    conn_cap = c.conn_cap if c.conn_cap is not None else max([len(k.weights) for k in kfs] + [len(m) for m in w.conn] + [1])
    a = state_arrays(w, conn_cap)
    status = np.zeros(max(w.nkf, 1), np.int32)
    limited = set()
    for f, k in enumerate(kfs):
        if len(k.weights) > conn_cap:
            status[f] = CR.LIMIT
            limited.add(k)
            continue
        status[f] = k.status
        if k.status & (CR.UPDATED | CR.RESORTED):
            row = sorted(k.weights.items(), key=lambda kw: kw[0].addr)
            a["nconn"][f], a["nord"][f] = len(row), len(k.ordered)
            a["conn_kf"][f, :len(row)], a["conn_w"][f, :len(row)] = [j.idx for j, _ in row], [x for _, x in row]
            a["ord_kf"][f, :len(k.ordered)], a["ord_w"][f, :len(k.ordered)] = [j.idx for j in k.ordered], k.ordered_w
            a["parent"][f], a["first"][f] = (k.parent.idx if k.parent is not None else -1), k.first
    loop = [(i.idx, j.idx, x) for i, j, x in loop if i not in limited]
    loop_cap = c.loop_cap if c.loop_cap is not None else len(loop) + 2
    lc = np.zeros((max(loop_cap, 1), 3), np.int32)
    lc[:, :2] = -1
    info = np.array([CR.LIMIT if len(loop) > loop_cap else 0, len(loop), len(limited), 0], np.int32)
    if len(loop) <= loop_cap and loop:
        lc[:len(loop)] = loop
    a.update(status=status, loop_conn=lc[:loop_cap], info=info, conn_cap=conn_cap, loop_cap=loop_cap, kfs=kfs)
    return a


STATE_KEYS = ("conn_kf", "conn_w", "nconn", "ord_kf", "ord_w", "nord", "parent", "first", "status", "loop_conn", "info")


def same_update(x, y, nkf):
    return all(np.array_equal(np.asarray(x[k])[:nkf] if k not in ("loop_conn", "info") else x[k],
                              np.asarray(y[k])[:nkf] if k not in ("loop_conn", "info") else y[k]) for k in STATE_KEYS)


def diff_update(x, y, nkf):
    return [k for k in STATE_KEYS if not same_update({**y, k: x[k]}, y, nkf)]


# ---------------------------------------------------------------- constructed graph cases
def _settle(w, th):
    """the state a whole-map UpdateConnections leaves, as the input of a later partial update"""
    kfs, _ = objects(w)
    for k in kfs:
        k.UpdateConnections(th, CR.REFERENCE)
    for f, k in enumerate(kfs):
        w.conn[f] = {j.idx: x for j, x in k.weights.items()}
        w.ordl[f] = [(j.idx, x) for j, x in zip(k.ordered, k.ordered_w)]
        w.parent[f], w.first[f] = (k.parent.idx if k.parent is not None else -1), k.first
    return w


def graph_cases():
    out = []
    # counts of th - 1 and th; a target outside the list; nlist = 1
    w = World(4)
    w.share([0, 1], 2); w.share([0, 2], 3); w.share([0, 3], 4)
    out.append(GraphCase("th_edge", w, [0], th=3))
    # the fallback with tied maxima under a non-identity order: pKFmax is the first in ADDRESS order
    w = World(4, order=[1, 3, 0, 2])
    w.share([0, 1], 2); w.share([0, 2], 2); w.share([0, 3], 1)
    out.append(GraphCase("fallback_tied", w, [0, 2], th=15))
    # weight ties under a non-identity order, every key frame in the list
    w = World(5, order=[4, 1, 3, 0, 2], id0=[True, False, False, False, False])
    for i in range(5):
        for j in range(i + 1, 5):
            w.share([i, j], 3 if (i + j) % 2 else 4)
    out.append(GraphCase("ties_whole_map", w, [3, 0, 4, 1, 2], th=3))
    # a sender before and after its target: stale input rows that differ from the counters
    w = World(4, order=[2, 0, 3, 1])
    w.share([0, 1], 3); w.share([1, 2], 4); w.share([0, 2], 1); w.share([2, 3], 3); w.share([1, 3], 1)
    for i in range(4):
        for j in range(4):
            if i != j and (i + 2 * j) % 3:
                w.connect(i, j, 1 + (i * j) % 4, ordered=(i + j) % 2 == 0)
        w.first[i] = i % 2 == 0
    out.append(GraphCase("sender_before_and_after", w, [1, 2, 0], th=3))
    # an unchanged send leaves the ordered list alone (its sub-threshold entries stay out); a changed one brings them in
    w = World(4)
    w.share([0, 1], 5); w.share([1, 2], 1); w.share([1, 3], 2); w.share([0, 2], 6)
    _settle(w, 3)
    w2 = copy.deepcopy(w)
    out.append(GraphCase("unchanged_send", w, [0], th=3))
    w2.share([0, 1], 1)
    out.append(GraphCase("changed_send", w2, [0], th=3))
    # inconsistent slots (c_ij != c_ji), duplicate slots, bad points, a point only its own key frame observes
    w = World(5, order=[3, 4, 0, 2, 1])
    w.share([0, 1], 3, holders=[0]); w.share([0, 1, 2], 2, holders=[1, 2]); w.share([2, 3], 4, bad=True); w.share([2, 3], 1)
    p = w.point([1, 3]); w.slots[1].append(p); w.slots[1].append(p)
    w.point([4]); w.point([0, 4], holders=[0])
    out.append(GraphCase("inconsistent_duplicate_bad", w, [4, 1, 0, 3, 2], th=3))
    # an empty counter keeps first_connection; an EMPTY member still receives sends from both sides; id0 gets no parent
    w = World(4, id0=[True, False, False, False])
    w.share([0, 1], 3, holders=[0]); w.share([2, 1], 3, holders=[2]); w.share([0, 3], 3)
    w.connect(1, 3, 2, ordered=False)
    out.append(GraphCase("empty_member", w, [0, 1, 2], th=3))
    # cap_per_frame no multiple of 64, an observation list longer than 64
    w = World(70)
    w.share(list(range(70)), 3)
    for f in range(70):
        w.slots[f] += [-1] * (f % 5)
    w.share([0, 69], 64)
    out.append(GraphCase("long_list", w, list(range(0, 70, 3)), th=3))
    # more than 1024 key frames with few slots each
    w = World(1100, order=[(7 * f + 3) % 1100 for f in range(1100)])
    for f in range(1100):
        w.share([f, (f + 1) % 1100], 2); w.share([f, (f + 37) % 1100], 1)
    out.append(GraphCase("many_key_frames", w, list(range(1099, -1, -1)), th=2))
    # conn_cap and loop_conn_cap reached exactly and one past
    w = World(6)
    for j in range(1, 6):
        w.share([0, j], 1 + j % 2)
    w.share([1, 2], 3)
    for name, cc in (("conn_cap_exact", 5), ("conn_cap_one_past", 4)):
        out.append(GraphCase(name, copy.deepcopy(w), [0, 1], th=2, conn_cap=cc))
    n = len(expected_update(GraphCase("", copy.deepcopy(w), [0, 1], th=2))["loop_conn"]) - 2
    assert n >= 2
    for name, lc in (("loop_cap_exact", n), ("loop_cap_one_past", n - 1)):
        out.append(GraphCase(name, copy.deepcopy(w), [0, 1], th=2, loop_cap=lc))
    return out


def random_world(seed):
    r = random.Random(seed)
    nkf, npts, th = r.randint(2, 9), r.randint(1, 40), r.choice([2, 3, 15])
    order = None if r.random() < 0.3 else r.sample(range(nkf), nkf)
    w = World(nkf, order, [f == 0 and r.random() < 0.7 for f in range(nkf)])
    w.obs = [r.sample(range(nkf), r.randint(0, nkf)) for _ in range(npts)]
    w.point_bad = [r.random() < 0.1 for _ in range(npts)]
    if r.random() < 0.6:
        w.slots = [[p for p in range(npts) if f in w.obs[p]] + [-1] for f in range(nkf)]
    else:
        w.slots = [[r.choice([-1] + list(range(npts))) for _ in range(r.randint(0, 30))] for _ in range(nkf)]
    for f in range(nkf):
        others = [x for x in range(nkf) if x != f]
        w.conn[f] = {j: r.randint(1, 5) for j in r.sample(others, r.randint(0, nkf - 1))}
        o = [(j, x) for j, x in w.conn[f].items() if r.random() < 0.7]
        r.shuffle(o)
        w.ordl[f], w.first[f] = o, r.random() < 0.5
        w.parent[f] = r.choice([-1] + others)
        w.kf_bad[f] = r.random() < 0.15
    lst = r.sample(range(nkf), r.randint(1, nkf))
    return GraphCase("random%d" % seed, w, lst, th)


# ---------------------------------------------------------------- the local map
class LocalCase:
    def __init__(self, name, world, frame, prev=None, nbest=10, max_local=80, lkf_cap=None, qcap=None):
        self.name, self.w, self.frame, self.prev = name, world, list(frame), prev
        self.nbest, self.max_local, self.lkf_cap, self.qcap = nbest, max_local, lkf_cap, qcap


def expected_local(c, rules=CR.REFERENCE):
    kfs, pts = objects(c.w)
    slots, local, ref, points, no_votes = CR.update_local_map(kfs, [pts[p] if p >= 0 else None for p in c.frame],
                                                              None if c.prev is None else [kfs[f] for f in c.prev], c.nbest, c.max_local, rules)
    lkf_cap = c.lkf_cap if c.lkf_cap is not None else max(len(local), len(c.prev or []), 1) + 1
    qcap = c.qcap if c.qcap is not None else max(len(points), 1) + 1
    status = CR.NO_VOTES if no_votes else 0
    local, points = [k.idx for k in local], [p.idx for p in points]
    if len(local) > lkf_cap or len(points) > qcap:
        status, local, points = status | CR.LM_LIMIT, [], []
    return dict(kp_point=np.array([p.idx if p is not None else -1 for p in slots], np.int32), local_kf=np.array(local, np.int32),
                ref_kf=ref.idx if ref is not None else -1, queries=np.array(points, np.int32), status=status, lkf_cap=lkf_cap, qcap=qcap)


LOCAL_KEYS = ("kp_point", "local_kf", "ref_kf", "queries", "status")


def same_local(x, y):
    return all(np.array_equal(x[k], y[k]) for k in LOCAL_KEYS)


def _chain_world(nkf, order=None, pts_per_kf=3):
    """a ride: key frame f shares points with f + 1, the parent of f is f - 1, the graph settled at th 1"""
    w = World(nkf, order, [f == 0 for f in range(nkf)])
    for f in range(nkf - 1):
        w.share([f, f + 1], pts_per_kf)
    return _settle(w, 1)


def local_cases():
    out = []
    w = _chain_world(8, order=[5, 2, 7, 0, 3, 6, 1, 4])
    votes = lambda w, kfs: [p for p in range(len(w.obs)) if set(w.obs[p]) & set(kfs)]
    # tied votes: the first strict maximum in address order
    out.append(LocalCase("tied_votes", w, [w.slots[3][0], -1, w.slots[3][1], w.slots[5][0], w.slots[5][1]]))
    # a bad voted key frame (it votes, it is skipped, it can not be the reference); a cleared slot
    w2 = copy.deepcopy(w)
    w2.kf_bad[3] = True
    w2.point_bad[w2.slots[5][0]] = True
    out.append(LocalCase("bad_voted_and_cleared_slot", w2, list(w2.slots[3]) + [w2.slots[5][0], w2.slots[6][0]]))
    w3 = copy.deepcopy(w)
    for f in (2, 3):
        w3.kf_bad[f] = True
    out.append(LocalCase("all_voted_bad", w3, [w3.slots[2][-1]]))
    out.append(LocalCase("no_votes", w, [-1, -1]))
    out.append(LocalCase("no_votes_previous_list", w, [-1], prev=[4, 1, 6]))
    wb = copy.deepcopy(w)
    wb.point_bad[0] = True
    out.append(LocalCase("no_votes_only_bad_points", wb, [0, 0], prev=[2]))
    # the 11th neighbour: ten marked neighbours, the eleventh free
    w = World(14)
    for j in range(1, 12):
        w.share([0, j], 20 - j)
    _settle(w, 1)
    w.parent = [-1] * 14
    fr = [w.slots[j][0] for j in range(1, 11)]
    out.append(LocalCase("eleventh_neighbour", w, fr))
    # children against ranks; a bad child; a bad parent (pushed: no bad test); the parent ending the walk on the first entry
    w = World(7, order=[3, 6, 0, 5, 1, 4, 2])
    w.share([0, 1], 2); w.share([5, 6], 2)
    w.parent = [-1, 0, 0, 0, -1, 4, 0]
    w.kf_bad[2] = True
    out.append(LocalCase("children_by_rank", w, [w.slots[0][0], w.slots[1][0]]))
    w = World(6)
    w.share([1, 2], 2); w.share([3, 4], 2)
    w.parent = [-1, 0, 1, -1, 3, 3]
    w.kf_bad[0] = True
    out.append(LocalCase("bad_parent_ends_the_walk", w, [w.slots[1][0], w.slots[3][0]]))
    # first stages of 80, 81 and 82 key frames: the cap test is size() > 80
    for n1 in (79, 80, 81, 82):
        w = World(n1 + 3, order=[(11 * f + 2) % (n1 + 3) for f in range(n1 + 3)])
        p = w.point(list(range(n1)))
        w.connect(0, n1, 9); w.connect(1, n1 + 1, 9); w.connect(2, n1 + 2, 9)
        q = w.point([n1, n1 + 1, n1 + 2])
        out.append(LocalCase("first_stage_%d" % n1, w, [p]))
        assert q
    # capacities
    w = _chain_world(8)
    base = LocalCase("", w, list(w.slots[3]))
    e = expected_local(base)
    nl, nq = len(e["local_kf"]), len(e["queries"])
    assert nl > 2 and nq > 2
    out.append(LocalCase("lkf_cap_exact", w, base.frame, lkf_cap=nl, qcap=nq))
    out.append(LocalCase("lkf_cap_one_past", w, base.frame, lkf_cap=nl - 1))
    out.append(LocalCase("qcap_one_past", w, base.frame, qcap=nq - 1))
    return out


def random_local(seed):
    g = random_world(seed)
    r = random.Random(seed + 10 ** 6)
    w = g.w
    npts = len(w.obs)
    frame = [r.choice([-1] + list(range(npts))) for _ in range(r.randint(0, 12))]
    prev = None if r.random() < 0.5 else r.sample(range(w.nkf), r.randint(0, w.nkf))
    return LocalCase("random%d" % seed, w, frame, prev, nbest=r.choice([1, 2, 10]), max_local=r.choice([1, 3, 80]))


def view_world():
    """rows of 0, 3 and 12 entries with equal weights at the query weight"""
    w = World(14)
    for j in range(1, 13):
        w.share([0, j], 5 + j // 3)
    w.share([13, 1], 7); w.share([13, 2], 7); w.share([13, 3], 9)
    return _settle(w, 1)


# ---------------------------------------------------------------- runners
def run_single_update(c, ext, e):
    """the Python mirror over the single call; e = expected_update(c) for the capacities"""
    import pilotguru_amd as pg
    w, t = c.w, table_arrays(c.w)
    g = pg.CovisibilityGraph(ext, w.nkf, e["conn_cap"], w.order, w.id0)
    a = state_arrays(w, e["conn_cap"])
    g.conn_kf, g.conn_w, g.nconn, g.ord_kf, g.ord_w, g.nord, g.parent, g.first_connection = (a[k] for k in STATE_KEYS[:8])
    status, loop, info = g.UpdateConnections(w.slots, len(w.obs), t["obs_start"], t["obs_frame"][:t["nobs"]], c.lst, w.point_bad, c.th, e["loop_cap"])
    lc = np.zeros((max(e["loop_cap"], 1), 3), np.int32)
    lc[:, :2] = -1
    lc[:len(loop)] = loop
    return dict(conn_kf=g.conn_kf, conn_w=g.conn_w, nconn=g.nconn, ord_kf=g.ord_kf, ord_w=g.ord_w, nord=g.nord, parent=g.parent,
                first=g.first_connection, status=status, loop_conn=lc[:e["loop_cap"]], info=info)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def upload_world(w, conn_cap, extra_frames=0):
    t = table_arrays(w)
    d = {k: (None if t[k] is None else dev(t[k])) for k in ("kf_point", "n", "obs_start", "obs_frame", "point_bad", "kf_bad", "order", "id0")}
    d.update(cap=t["cap"], nobs=t["nobs"], npoints=len(w.obs))
    d.update({k: dev(v) for k, v in state_arrays(w, conn_cap).items()})
    return d


def run_device_update(c, ext, e, d=None, stream=None):
    """pgorb_update_connections_batch_device on torch tensors; returns the arrays and the tensors (for a chain)"""
    import torch
    w = c.w
    d = upload_world(w, e["conn_cap"]) if d is None else d
    lst = dev(np.array(c.lst + [0], np.int32))
    status = torch.full((max(w.nkf, 1) + 2,), -9, dtype=torch.int32, device="cuda")
    loop = torch.full((max(e["loop_cap"], 1) + 2, 3), -9, dtype=torch.int32, device="cuda")
    info = torch.full((CR.INFO,), -9, dtype=torch.int32, device="cuda")
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = ext._L.pgorb_update_connections_batch_device(
        ext._h, ptr(d["kf_point"]), ptr(d["n"]), w.nkf, d["cap"], d["npoints"], ptr(d["point_bad"]), ptr(d["obs_start"]), ptr(d["obs_frame"]),
        d["nobs"], ptr(d["order"]), ptr(d["id0"]), len(c.lst), ptr(lst), c.th, e["conn_cap"], ptr(d["conn_kf"]), ptr(d["conn_w"]), ptr(d["nconn"]),
        ptr(d["ord_kf"]), ptr(d["ord_w"]), ptr(d["nord"]), ptr(d["parent"]), ptr(d["first"]), ptr(status), e["loop_cap"],
        ptr(loop) if e["loop_cap"] else None, ptr(info), C.c_void_p(s.cuda_stream))
    assert rc == 0, (rc, ext._L.pgorb_last_error(ext._h))
    d.update(status=status, loop_conn=loop, info=info, lst=lst)
    return d


def download_update(d, e):
    import torch
    torch.cuda.synchronize()
    out = {k: d[k].cpu().numpy() for k in STATE_KEYS}
    assert np.all(out["status"][-2:] == -9) and np.all(out["loop_conn"][max(e["loop_cap"], 1):] == -9), "wrote past an output array"
    out["status"], out["loop_conn"] = out["status"][:-2], out["loop_conn"][:e["loop_cap"]]
    return out


def run_device_local(cases, ext, world, stream=None, conn_cap=None, lkf_cap=8, qcap=8, nbest=10, max_local=80, prev=True):
    """pgorb_update_local_map_batch_device: the frames of `cases` (all over `world`) as one batch; the frame of pair p is batch frame
    nkf + p.  Returns the outputs as arrays and the tensors."""
    import torch
    w = copy.deepcopy(world)
    npairs = len(cases)
    nkf = w.nkf
    conn_cap = conn_cap or max([len(o) for o in w.ordl] + [len(m) for m in w.conn] + [1])
    for c in cases:                                                        # the frames join the batch; nothing names them
        w.slots.append([-1] * len(c.frame))
    w.nkf, w.kf_bad, w.id0 = nkf + npairs, w.kf_bad + [False] * npairs, w.id0 + [False] * npairs
    t = table_arrays(w)
    cap, nfr = t["cap"], nkf + npairs
    st = state_arrays(world, conn_cap)
    pad = lambda x, fill: np.concatenate([x[:nkf], np.full((npairs,) + x.shape[1:], fill, x.dtype)])
    kp = np.full((npairs, cap), -1, np.int32)
    pv, npv = np.zeros((npairs, lkf_cap), np.int32), np.zeros(npairs, np.int32)
    for p, c in enumerate(cases):
        kp[p, :len(c.frame)] = c.frame
        if c.prev is not None:
            pv[p, :len(c.prev)], npv[p] = c.prev, len(c.prev)
    order = np.array([world.rank(f) for f in range(nkf)] + list(range(nkf, nfr)), np.int32)
    d = dict(kf_point=dev(t["kf_point"]), n=dev(t["n"]), kf_bad=dev(t["kf_bad"]),
             pair_frame=dev(np.arange(nkf, nfr, dtype=np.int32)), kp_point=dev(kp), point_bad=dev(t["point_bad"]), obs_start=dev(t["obs_start"]),
             obs_frame=dev(t["obs_frame"]), ord_kf=dev(pad(st["ord_kf"], FILL)), nord=dev(pad(st["nord"], 0)), parent=dev(pad(st["parent"], -1)),
             order=dev(order), prev=dev(pv), nprev=dev(npv))
    full = lambda *shape: torch.full(shape, -9, dtype=torch.int32, device="cuda")
    d.update(kp_out=full(npairs + 1, cap), local_kf=full(npairs + 1, lkf_cap), nlocal=full(npairs + 1), ref=full(npairs + 1),
             queries=full(npairs + 1, qcap), nq=full(npairs + 1), lm_status=full(npairs + 1))
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = ext._L.pgorb_update_local_map_batch_device(
        ext._h, ptr(d["kf_point"]), ptr(d["n"]), nfr, cap, ptr(d["kf_bad"]), ptr(d["pair_frame"]), npairs, ptr(d["kp_point"]), len(w.obs),
        ptr(d["point_bad"]), ptr(d["obs_start"]), ptr(d["obs_frame"]), t["nobs"], conn_cap, ptr(d["ord_kf"]), ptr(d["nord"]), ptr(d["parent"]),
        ptr(d["order"]), nbest, max_local, lkf_cap, ptr(d["prev"]) if prev else None, ptr(d["nprev"]) if prev else None, ptr(d["kp_out"]),
        ptr(d["local_kf"]), ptr(d["nlocal"]), ptr(d["ref"]), qcap, ptr(d["queries"]), ptr(d["nq"]), ptr(d["lm_status"]), C.c_void_p(s.cuda_stream))
    assert rc == 0, (rc, ext._L.pgorb_last_error(ext._h))
    d.update(cap=cap, npairs=npairs)
    return d


def download_local(d, cases):
    import torch
    torch.cuda.synchronize()
    h = {k: d[k].cpu().numpy() for k in ("kp_out", "local_kf", "nlocal", "ref", "queries", "nq", "lm_status")}
    assert all(np.all(h[k][-1] == -9) for k in h), "wrote past the last pair"
    out = []
    for p, c in enumerate(cases):
        nl, nq = int(h["nlocal"][p]), int(h["nq"][p])
        out.append(dict(kp_point=h["kp_out"][p, :len(c.frame)], local_kf=h["local_kf"][p, :nl], ref_kf=int(h["ref"][p]), queries=h["queries"][p, :nq],
                        status=int(h["lm_status"][p])))
    return out, h
