"""Every entry point at its stated capacity: the largest size its gate accepts, filled almost wholly with inert entries so that
the sequential references stay cheap, and a handful of live entries at the top of every index range.  A helper module (no
tests): tests/test_capacity.py runs the cases.

The sizes come from the gates in pilotguru_amd/csrc (read there, not measured):
  LDS            160 KB of dynamic LDS per workgroup (match_common.h: pg_raise_lds)
  KP_MAX         16 000 keypoints per frame: every guided matcher, Fuse, loop closing, CreateNewMapPoints
  SbP line       keypoints * 13 + queries * 10 + 256 <= LDS (window_match.hip: the three SearchByProjection forms)
  CNM_NEIGH      PGORB_CNM_MAX_NEIGHBOURS = 64 (mapping.hip)
  PLACE_*        65 536 frames in a place table, 65 535 queries per batch, 8 192 features for k_bow_vectors (place.hip)
  K7_MAX         2^20 - 1 train descriptors / descriptors per frame (api.hip; match.hip: key = distance << 20 | index)
  LEVEL_PX       4 095 px per level side (K2's record x | y << 12 | score << 24; api.hip, plan.hip)
  LEVEL_KP       65 533 keypoints on one pyramid level (plan.hip: selCap = quota + 2 <= 65 535, K3's 16-bit arrival index)

A capacity case is a dict: name, the case of the family's own module (`case`), and `fields`: for every index field the case
fills, (limit, used, ties).  `limit` is the number of values the gate lets into the field, so limit - 1 is the last valid
index and (limit - 1).bit_length() the bits the field needs; `used(want)` names the indices of that field which the wanted
result holds; `ties` lists (low, high) rivals with low == high mod half the field: the wanted result holds `high`, a field one
bit too narrow would produce `low`."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matcher_cases as MC  # noqa: E402
from matcher_cases import BOUNDS, at_distance, rand_desc  # noqa: E402

LDS = 160 * 1024
KP_MAX = 16000
CNM_NEIGH = 64
PLACE_FRAMES, PLACE_QUERIES, PLACE_FEATURES = 65536, 65535, 8192
K7_MAX = (1 << 20) - 1
LEVEL_PX = 4095
LEVEL_KP = 65533


def sbp_lds(cap, qcap):
    """window_match.hip: the dynamic LDS of k_search_by_projection for `cap` keypoints and `qcap` queries."""
    return cap * 13 + qcap * 10 + 256


def sbp_largest_qcap(cap):
    return (LDS - 256 - cap * 13) // 10


# three points on the LDS line: a single query, as many queries as keypoints, a small frame
SBP_POINTS = [(12582, 1), (7112, 7112), (1000, sbp_largest_qcap(1000))]


def half(limit):
    """The top bit of a field that holds the indices 0 .. limit - 1."""
    return 1 << ((limit - 1).bit_length() - 1)


def field(limit, used, ties=()):
    return dict(limit=limit, used=used, ties=list(ties))


def truncated(indices, limit):
    """What a field one bit too narrow would hold."""
    return sorted(set(int(i) % half(limit) for i in indices))


# ---------------------------------------------------------------- filler
def _filler_keys(n, rng, octave):
    """n keypoints spread over the right two thirds of the 640 x 480 grid (x >= 200), in no particular order: every cell
    there holds several, cell order is not index order, and no window of a live site (x <= 110) reaches one."""
    k = MC.keys(rng.uniform(200.0, 630.0, n).astype(np.float32), rng.uniform(8.0, 470.0, n).astype(np.float32), octave=octave)
    return k


SITES = [(60.0, 60.0), (60.0, 180.0), (60.0, 300.0), (60.0, 420.0)]       # isolated: 120 px apart, windows below 50 px


def _place(k, i, x, y, octave=0):
    k["x"][i], k["y"][i], k["octave"][i], k["angle"][i] = x, y, octave, 0.0


# ---------------------------------------------------------------- Frame grid + SearchForInitialization
def sfi_capacity_case(seed=1, cap=KP_MAX):
    """Both frames full.  F1's filler sits above level 0 (skipped, ORBmatcher.cc:424), F2's filler on level 3 and outside every
    window.  Live: the last keypoint of F1 matched to the last of F2; F1 8200 choosing F2 8200 (distance 20) over F2 8 (30);
    F1 15998 stealing F2 15990 from F1 15990; F1 5 matched to F2 15997."""
    rng = np.random.RandomState(seed)
    h = half(cap)
    k1, k2 = _filler_keys(cap, rng, 1), _filler_keys(cap, rng, 3)
    d1, d2 = rand_desc(rng, cap), rand_desc(rng, cap)
    last = cap - 1
    (ax, ay), (bx, by), (cx, cy), (dx, dy) = SITES
    _place(k1, last, ax, ay); _place(k2, last, ax + 1, ay); d2[last] = at_distance(d1[last], 10, rng)
    _place(k1, h + 8, bx, by); _place(k2, h + 8, bx + 1, by); _place(k2, 8, bx - 1, by)
    d2[h + 8], d2[8] = at_distance(d1[h + 8], 20, rng), at_distance(d1[h + 8], 30, rng)
    _place(k1, last - 9, cx, cy); _place(k1, last - 1, cx, cy); _place(k2, last - 9, cx + 1, cy)
    d1[last - 9], d1[last - 1] = at_distance(d2[last - 9], 25, rng), at_distance(d2[last - 9], 15, rng)
    _place(k1, 5, dx, dy); _place(k2, last - 2, dx + 1, dy); d2[last - 2] = at_distance(d1[5], 12, rng)
    case = MC.sfi_case("cap", "sfi_cap_%d" % cap, k1, d1, k2, d2, win=20, ratio=0.9)
    m12 = lambda want: want[1]
    return dict(name=case["name"], case=case, size="2 frames x %d keypoints" % cap,
                fills="vnMatches12 / vnMatches21 / vMatchedDistance [cap] in LDS (cap * 10 + 192 B), 16-bit i2 of a list entry",
                fields={"F1 keypoint": field(cap, lambda w: np.flatnonzero(m12(w) >= 0)),
                        "F2 keypoint": field(cap, lambda w: m12(w)[m12(w) >= 0], [(8, h + 8)])})


def grid_capacity_case(seed=2, cap=KP_MAX):
    """A full frame through AssignFeaturesToGrid: keypoints everywhere, some outside the grid, the last index in the first cell."""
    rng = np.random.RandomState(seed)
    k = MC.keys(rng.uniform(-5.0, 645.0, cap).astype(np.float32), rng.uniform(-5.0, 485.0, cap).astype(np.float32))
    _place(k, cap - 1, 1.0, 1.0)
    _place(k, half(cap) + 3, 1.5, 2.0)
    _place(k, 3, 2.0, 1.5)
    case = MC._case("cap", "grid_cap_%d" % cap, "grid", keys=k, bounds=BOUNDS)
    return dict(name=case["name"], case=case, size="%d keypoints" % cap, fills="mGrid as CSR: 32-bit indices, no limit of its own",
                fields={"keypoint": field(cap, lambda w: w[1][:w[0][1]])})


# ---------------------------------------------------------------- the three SearchByProjection forms on the LDS line
def sbp_capacity_case(kind, cap, qcap, seed=3):
    """`cap` keypoints and `qcap` queries with sbp_lds(cap, qcap) at the budget.  Filler keypoints: level 7, outside every
    window.  Filler queries: invalid (odd) or projected far outside the grid (even).  Live, with hk / hq the top bits of the
    two fields: site 1 the last query takes the last keypoint; site 2 query hq + 3 meets a distance tie between keypoint hk + 5
    (lower column: scanned first, wins) and keypoint 5; site 3 query 4 (no observations) takes keypoint hk + 6 and query hq + 4
    overwrites it (points / last frame), or is blocked by it (key frame: any point blocks).  With one query only site 2 exists,
    between the last keypoint and the last keypoint - hk."""
    rng = np.random.RandomState(seed + cap)
    hk = half(cap)
    k = _filler_keys(cap, rng, 7)
    d = rand_desc(rng, cap)
    qd = rand_desc(rng, qcap)
    valid = (np.arange(qcap) % 2 == 0).astype(np.uint8)
    x = np.full(qcap, -500.0, np.float32); y = np.full(qcap, -500.0, np.float32)
    obs = np.ones(qcap, np.uint8)
    tie_levels = (1, 0) if kind == "points" else (0, 0)

    def tie(site, q, hi, lo):
        sx, sy = SITES[site]
        _place(k, hi, sx - 7.0, sy, tie_levels[0]); _place(k, lo, sx + 7.0, sy, tie_levels[1])
        d[hi], d[lo] = at_distance(qd[q], 20, rng), at_distance(qd[q], 20, rng)
        valid[q], x[q], y[q] = 1, sx, sy

    if qcap == 1:
        kB, kb = cap - 1, cap - 1 - hk
        tie(1, 0, kB, kb)
        q_field = None                     # a one-entry field has no top
    else:
        hq = half(qcap)
        kA, kB, kb, kC = cap - 1, hk + 5, 5, hk + 6
        qLast, qH, ql, qH2 = qcap - 1, hq + 3, 4, hq + 4
        sx, sy = SITES[0]
        _place(k, kA, sx + 1.0, sy); d[kA] = at_distance(qd[qLast], 10, rng); valid[qLast], x[qLast], y[qLast] = 1, sx, sy
        tie(1, qH, kB, kb)
        sx, sy = SITES[2]
        _place(k, kC, sx + 1.0, sy)
        qd[ql], qd[qH2] = at_distance(d[kC], 10, rng), at_distance(d[kC], 12, rng)
        obs[ql] = 0
        for q in (ql, qH2):
            valid[q], x[q], y[q] = 1, sx, sy
        q_field = field(qcap, lambda w: w[1][w[1] >= 0], [] if kind == "keyframe" else [(ql, qH2)])
    name = "%s_cap_%d_q_%d" % (kind, cap, qcap)
    zi, zf = np.zeros(qcap, np.int32), np.zeros(qcap, np.float32)
    common = dict(keys=k, desc=d, bounds=BOUNDS, has=np.zeros(cap, np.uint8), valid=valid, pd=qd)
    if kind == "points":           # r = 4 * th * sf[1] = 14.4 px on levels 0 and 1
        case = MC._case("cap", name, kind, px=x, py=y, lvl=zi + 1, vc=zf + np.float32(0.9), obs=obs, th=3.0, ratio=0.9, **common)
    elif kind == "frame":          # r = th * sf[0] = 15 px on levels 0 and 1
        case = MC._case("cap", name, kind, u=x, v=y, oct=zi, ang=zf, obs=obs, th=15.0, ori=True, **common)
    else:                          # PredictScale(4, 4) = level 0: r = 15 px
        case = MC._case("cap", name, kind, found=np.zeros(qcap, np.uint8), u=x, v=y, d3=zf + 4.0, mind=zf + 1.0, maxd=zf + 4.0, ang=zf,
                        th=15.0, orbdist=100, ori=True, **common)
    fields = {"keypoint": field(cap, lambda w: np.flatnonzero(w[1] >= 0), [(kb, kB)])}
    if q_field:
        fields["query"] = q_field
    return dict(name=name, case=case, size="%d keypoints, %d queries" % (cap, qcap),
                fills="k_search_by_projection's LDS: %d of %d B; 14-bit keypoint index of a candidate, 16-bit query lists" % (sbp_lds(cap, qcap), LDS),
                fields=fields)


def sbp_capacity_cases():
    return [sbp_capacity_case(kind, cap, qcap) for cap, qcap in SBP_POINTS for kind in ("points", "frame", "keyframe")]


def sbp_one_past(kind, cap, qcap):
    """The same shapes with one more query: nothing live, the gate answers before anything runs."""
    c = sbp_capacity_case(kind, cap, qcap)["case"]
    a = dict(c["a"])
    for key in ("valid", "px", "py", "lvl", "vc", "obs", "u", "v", "oct", "ang", "found", "d3", "mind", "maxd"):
        if key in a:
            a[key] = np.concatenate([a[key], a[key][-1:]])
    a["pd"] = np.concatenate([a["pd"], a["pd"][-1:]])
    return dict(c, a=a)


# ---------------------------------------------------------------- the BoW-node matchers
def fv_of(node_of):
    """matcher_cases._fv for long frames (one stable sort, not one pass per node)."""
    node_of = np.asarray(node_of, np.int64)
    order = np.argsort(node_of, kind="stable")
    nodes, first = np.unique(node_of[order], return_index=True)
    return nodes.astype(np.uint32), np.concatenate([first, [len(node_of)]]).astype(np.int32), order.astype(np.uint32)


def bow_members(cap):
    """The shared node's 260 members in each frame: 248 low indices, two just above the top bit, the last ten."""
    h = half(cap)
    return np.concatenate([np.arange(248), [h + 8, h + 9], np.arange(cap - 10, cap)])


BOW_NODE, BOW_LONG_NODE = 7, 9


def bow_long_members(cap):
    """The frame side of a second shared node: 8 300 features, so list positions reach past bit 13 (a rank is
    dist << 16 | position).  The key frame has three features in it."""
    h = half(cap)
    return np.concatenate([np.arange(300, h - 2), np.arange(h + 18, h + 18 + 8300 - (h - 302))])


def bow_nodes(cap, rng, own, long_side):
    """Node of every feature: the members share BOW_NODE (> 256 features: the kernels' long-node path), the filler is spread
    over 40 nodes no other frame has (`own` keeps the two frames' filler nodes apart)."""
    node = 100 + own + 2 * rng.randint(0, 40, cap)
    node[bow_long_members(cap) if long_side else np.arange(300, 303)] = BOW_LONG_NODE
    node[bow_members(cap)] = BOW_NODE
    return node


def bow_descriptors(cap, rng):
    """Live pairs (the first frame's feature -> the second's): last <-> last (distance 10); last - 9 choosing h + 8 (20) over
    8 (30); h + 9 (whose alias 9 matches nothing) taking last - 4 (15); in the long node 300 choosing the feature at list position
    8 299 (10) over the one at position 8 299 - 8 192 (18).  Every other pair of a shared node is a random pair."""
    h, last = half(cap), cap - 1
    d1, d2 = rand_desc(rng, cap), rand_desc(rng, cap)
    d2[last] = at_distance(d1[last], 10, rng)
    d2[h + 8], d2[8] = at_distance(d1[last - 9], 20, rng), at_distance(d1[last - 9], 30, rng)
    d2[last - 4] = at_distance(d1[h + 9], 15, rng)
    lm = bow_long_members(cap)
    assert len(lm) == 8300
    d2[lm[-1]], d2[lm[8299 - 8192]] = at_distance(d1[300], 10, rng), at_distance(d1[300], 18, rng)
    return d1, d2


def bow_capacity_case(seed=4, cap=KP_MAX):
    """SearchByBoW(KeyFrame, Frame) on two full frames: see bow_descriptors."""
    rng = np.random.RandomState(seed)
    h = half(cap)
    kd, fd = bow_descriptors(cap, rng)
    kk = MC.keys(np.zeros(cap), np.zeros(cap)); fk = MC.keys(np.zeros(cap), np.zeros(cap))
    kn, fn = bow_nodes(cap, rng, 0, False), bow_nodes(cap, rng, 1, True)
    case = MC._case("cap", "bow_cap_%d" % cap, "bow", kk=kk, kd=kd, kv=np.ones(cap, np.uint8), kfv=fv_of(kn), knode=kn.astype(np.int32),
                    fk=fk, fd=fd, ffv=fv_of(fn), fnode=fn.astype(np.int32), ratio=0.7, ori=True)
    return dict(name=case["name"], case=case, size="2 frames x %d features, shared nodes of %d and 3 x 8300" % (cap, len(bow_members(cap))),
                fills="dist << 16 | list position ranks, feature indices up to 15 999, nodes past the 256 features held in registers",
                fields={"frame feature": field(cap, lambda w: np.flatnonzero(w[1] >= 0), [(8, h + 8)]),
                        "key-frame feature": field(cap, lambda w: w[1][w[1] >= 0], [(9, h + 9)])})


# ---------------------------------------------------------------- K7: the popcount matcher
def k7_capacity_case(seed=5, nb=K7_MAX, na=70):
    """nb random train descriptors, na queries.  Queries 0, 7, .. 35 have an exact and a one-bit-off copy at two of the indices
    nb - 1 - t (nb - 1 = 2^20 - 2), 2^19 + t and 5 + t, in all six orders (t = 0 .. 5), so best and second best both come from
    the top of the index field.  Query 1: exact copies at 15 and 2^19 + 15 (equal keys but for the index: the lower one wins);
    query 2: at 2^19 + 20 and nb - 21; query 3: exact at 2^19 + 30, one bit off at its alias 30."""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (na, 32)).astype(np.uint8)
    b = rng.randint(0, 256, (nb, 32)).astype(np.uint8)
    h = half(nb)

    def near(q):
        d = a[q].copy()
        d[q % 32] ^= 1 << (q % 8)
        return d
    orders = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    for t, (e, n) in enumerate(orders):
        spots = (nb - 1 - t, h + t, 5 + t)
        b[spots[e]], b[spots[n]] = a[7 * t], near(7 * t)
    b[15], b[h + 15] = a[1], a[1]
    b[h + 20], b[nb - 21] = a[2], a[2]
    b[h + 30], b[30] = a[3], near(3)
    return dict(name="k7_nb_%d" % nb, a=a, b=b, size="%d queries x %d train descriptors" % (na, nb),
                fills="key = distance << 20 | train index (20 bits)",
                fields={"train": field(nb, lambda w: w[0][w[0] >= 0], [(30, h + 30)])})


# ---------------------------------------------------------------- key frames of 16 000 keypoints: Fuse and loop closing's projection matchers
def lift_plan(n, total, winners, loser):
    """Where the n keypoints of a small case go in a key frame of `total`: the first winner to the last slot, the second to
    half + 5, `loser` (a keypoint that wins nothing) to its alias 5, the others to the slots just below the last."""
    h = half(total)
    new = np.full(n, -1, np.int64)
    new[winners[0]], new[winners[1]], new[loser] = total - 1, h + 5, 5
    rest = [i for i in range(n) if new[i] < 0]
    new[rest] = total - 2 - np.arange(len(rest))
    assert len(set(new.tolist())) == n and new.min() >= 0
    return new


def lift_frame(k, d, new, total, rng, per_keypoint=(), spread=(8.0, 200.0)):
    """The frame with its keypoints moved to the slots `new` and inert keypoints (level 7, x inside `spread`) in all the others;
    per_keypoint: (array, filler value) pairs that move with the keypoints."""
    K = MC.keys(rng.uniform(spread[0], spread[1], total).astype(np.float32), rng.uniform(8.0, 470.0, total).astype(np.float32), octave=7)
    D = rand_desc(rng, total)
    K[new], D[new] = k, d
    out = []
    for arr, fill in per_keypoint:
        a = np.full(total, fill, np.asarray(arr).dtype)
        a[new] = arr
        out.append(a)
    return K, D, out


def _two_winners_and_a_loser(best, n):
    """From the keypoints a small case's reference chose (in query order): two distinct winners and a keypoint never chosen."""
    seen = []
    for b in best:
        if b >= 0 and int(b) not in seen:
            seen.append(int(b))
    losers = [i for i in range(n) if i not in seen]
    assert len(seen) >= 2 and losers, "the base case needs two winning keypoints and one that wins nothing"
    return seen[:2], losers[0]


def fuse_capacity_case(seed=3, total=KP_MAX):
    """fuse_cases.collision_case (20 points onto 6 keypoints, live and bad occupants, chains) inside a key frame of 16 000."""
    import fuse_cases as FC
    c = FC.collision_case(seed)
    ref = FC.run_reference(c)
    kid, k, d, P, b = c.kf
    new = lift_plan(len(k), total, *_two_winners_and_a_loser(ref[2], len(k)))
    K, D, _ = lift_frame(k, d, new, total, np.random.RandomState(seed))
    pts = []
    for p in c.points:
        q = dict(p, obs=[(o, int(new[i]) if o == kid else i) for o, i in p["obs"]])
        if "bad_slots" in p:
            q["bad_slots"] = [(o, int(new[i])) for o, i in p["bad_slots"]]
        pts.append(q)
    case = FC.Case("fuse_cap_%d" % total, (kid, K, D, P, b), pts, c.queries, others=c.others, th=c.th)
    return dict(name=case.name, case=case, size="key frame of %d keypoints, %d queries" % (total, len(c.queries)),
                fills="slot chains and best_idx at keypoints >= 15 990; the window scan's grid of 16 000",
                fields={"keypoint": field(total, lambda w: w[2][w[2] >= 0], [(5, half(total) + 5)])})


def _loop_lift(c, ref_best, total, seed):
    import loop_cases as LC
    kid, k, d, P, b = c.kf
    new = lift_plan(len(k), total, *_two_winners_and_a_loser(ref_best, len(k)))
    K, D, (slots,) = lift_frame(k, d, new, total, np.random.RandomState(seed), [(c.slots, -1)])
    return LC.Case(c.name + "_cap_%d" % total, (kid, K, D, P, b), c.points, slots, c.queries, th=c.th)


def ps3_capacity_cases(total=KP_MAX):
    """SearchByProjection(pKF, Scw): loop_cases.collision_case, and dense_window_case, whose first query lists more than 64
    keypoints (evaluated in place by k_ps3_decide) and takes the one lifted to slot 15 999."""
    import loop_cases as LC
    out = []
    for c in (LC.collision_case(1), LC.dense_window_case(np.random.RandomState(2))):
        asg = LC.run_ref3(c)[1]
        by_query = sorted((int(q), i) for i, q in enumerate(asg) if q >= 0)
        case = _loop_lift(c, [i for _, i in by_query], total, 11)
        out.append(dict(name="ps3_" + case.name, case=case, size="key frame of %d keypoints, %d queries" % (total, len(c.queries)),
                        fills="distance << 24 | position << 16 | keypoint lists; minq / taken [cap] in LDS (cap * 5 B)",
                        fields={"keypoint": field(total, lambda w: np.flatnonzero(w[1] >= 0), [(5, half(total) + 5)])}))
    return out


def fs3_capacity_case(total=KP_MAX):
    """Fuse(pKF, Scw): loop_cases.collision_case inside a key frame of 16 000."""
    import loop_cases as LC
    c = LC.collision_case(2)
    case = _loop_lift(c, LC.run_ref4(c)[3], total, 12)
    return dict(name="fs3_" + case.name, case=case, size="key frame of %d keypoints, %d queries" % (total, len(c.queries)),
                fills="head[cap] (atomicMin of the query index) and best_idx at keypoints >= 15 990",
                fields={"keypoint": field(total, lambda w: w[3][w[3] >= 0], [(5, half(total) + 5)])})


def sim3_capacity_case(total=KP_MAX):
    """SearchBySim3: loop_cases.pair_case with both key frames lifted to 16 000 keypoints (the filler lies all over the image
    here, inert by its level alone)."""
    import loop_cases as LC
    c = LC.pair_case(0)
    m12 = LC.run_ref2(c)[1]
    n1, n2 = len(c.kf1[0]), len(c.kf2[0])
    new1 = lift_plan(n1, total, *_two_winners_and_a_loser(np.flatnonzero(m12 >= 0), n1))
    new2 = lift_plan(n2, total, *_two_winners_and_a_loser(m12[m12 >= 0], n2))
    rng = np.random.RandomState(13)
    K1, D1, (s1, a1) = lift_frame(c.kf1[0], c.kf1[1], new1, total, rng, [(c.slots1, -1), (c.already1, 0)], spread=(8.0, 632.0))
    K2, D2, (s2, a2) = lift_frame(c.kf2[0], c.kf2[1], new2, total, rng, [(c.slots2, -1), (c.already2, 0)], spread=(8.0, 632.0))
    case = LC.PairCase("sim3_cap_%d" % total, (K1, D1, c.kf1[2]), (K2, D2, c.kf2[2]), c.points, s1, s2, c.sim3, a1, a2, c.th)
    h = half(total)
    return dict(name=case.name, case=case, size="2 key frames x %d keypoints" % total,
                fills="both directions' best keypoints at slots >= 15 990; two grids of 16 000",
                fields={"KF1 keypoint": field(total, lambda w: np.flatnonzero(w[1] >= 0), [(5, h + 5)]),
                        "KF2 keypoint": field(total, lambda w: w[1][w[1] >= 0], [(5, h + 5)])})


# ---------------------------------------------------------------- SearchByBoW(KF, KF) and SearchForTriangulation at 16 000 features
def _node_pair_fields(cap):
    h = half(cap)
    return {"first keypoint": field(cap, lambda w: np.flatnonzero(w[1] >= 0), [(9, h + 9)]),
            "second keypoint": field(cap, lambda w: w[1][w[1] >= 0], [(8, h + 8)])}


def kfbow_capacity_case(seed=6, cap=KP_MAX):
    """SearchByBoW(pKF1, pKF2): the frames of bow_capacity_case (bow_descriptors, bow_nodes) as two key frames, every point valid."""
    import loop_cases as LC
    rng = np.random.RandomState(seed)
    d1, d2 = bow_descriptors(cap, rng)
    z, one = np.zeros(cap, np.float32), np.ones(cap, np.uint8)
    case = LC.BowCase("kfbow_cap_%d" % cap, d1, z, one, bow_nodes(cap, rng, 0, False), d2, z, one, bow_nodes(cap, rng, 1, True))
    return dict(name=case.name, case=case, size="2 key frames x %d features, shared nodes of 260 and 3 x 8300" % cap,
                fills="dist << 16 | list position ranks, vbMatched2 [cap], feature indices up to 15 999", fields=_node_pair_fields(cap))


def tri_capacity_case(seed=7, cap=KP_MAX):
    """SearchForTriangulation on the same node layout.  Every keypoint lies on the line y = 100 under a fundamental matrix whose
    epipolar lines are horizontal and an epipole far away, so within a shared node only the descriptors decide."""
    import triangulation_cases as TC
    rng = np.random.RandomState(seed)
    d1, d2 = bow_descriptors(cap, rng)
    k = MC.keys(10.0 + (np.arange(cap) % 600), np.full(cap, 100.0))
    z = np.zeros(cap, np.uint8)
    case = dict(name="tri_cap_%d" % cap, k1=k, d1=d1, fv1=fv_of(bow_nodes(cap, rng, 0, False)), h1=z, k2=k.copy(), d2=d2,
                fv2=fv_of(bow_nodes(cap, rng, 1, True)), h2=z, F=TC.F_H.copy(), ep=(np.float32(TC.EP_FAR[0]), np.float32(TC.EP_FAR[1])), ori=True)
    return dict(name=case["name"], case=case, size="2 key frames x %d keypoints, shared nodes of 260 and 3 x 8300" % cap,
                fills="dist << 16 | list position ranks, keypoint indices up to 15 999", fields=_node_pair_fields(cap))


# ---------------------------------------------------------------- CreateNewMapPoints: 64 neighbours, KF1 of 16 000 keypoints
def _node_of(fv, n):
    node = np.zeros(n, np.int64)
    for a, nd in enumerate(fv[0]):
        node[fv[2][fv[1][a]:fv[1][a + 1]]] = int(nd)
    return node


def cnm_capacity_case(seed=5, total=KP_MAX, nneigh=CNM_NEIGH):
    """mapping_cases.scene (KF1 and three neighbours over 60 points) with KF1 lifted to 16 000 keypoints and 64 neighbour
    slots: the sideways neighbours sit in slots 40 and 63 (the last), the yawed one in slot 7 seeing a third of its keypoints;
    the other slots hold neighbours the reference gets nothing from: a baseline too small (skipped), no keypoints, or keypoints
    in vocabulary nodes KF1 lacks."""
    import mapping_cases as MP
    KF1, neigh = MP.scene(seed, nneigh=6, npts=60, nodes=6, far=False)
    rng = np.random.RandomState(seed)
    small = MP.run_reference(KF1, [neigh[5], neigh[0]])[0]
    won = [int(p[1]) for p in small]
    n1 = len(KF1["k"])
    new = lift_plan(n1, total, *_two_winners_and_a_loser(won, n1))
    K, D, (h1,) = lift_frame(KF1["k"], KF1["d"], new, total, rng, [(KF1["h"], 0)], spread=(8.0, 632.0))
    node = 1000 + rng.randint(0, 40, total)
    node[new] = _node_of(KF1["fv"], n1)
    big = dict(k=K, d=D, fv=fv_of(node), h=h1, pose=KF1["pose"])
    third = dict(neigh[1])
    keep = np.arange(len(third["k"])) % 3 == 0
    third.update(k=third["k"][keep], d=third["d"][keep], h=third["h"][keep], fv=fv_of(_node_of(third["fv"], len(keep))[keep]))
    empty = dict(k=MC.keys([], []), d=np.zeros((0, 32), np.uint8), fv=fv_of(np.zeros(0, np.int64)), h=np.zeros(0, np.uint8),
                 pose=neigh[0]["pose"], median=np.float32(4.0))
    foreign = dict(neigh[0], fv=fv_of(_node_of(neigh[0]["fv"], len(neigh[0]["k"])) + 500))
    dead = [neigh[4], empty, foreign]
    slots = [dead[s % 3] for s in range(nneigh)]
    slots[7], slots[40], slots[nneigh - 1] = third, neigh[5], neigh[0]
    h = half(total)
    return dict(name="cnm_cap_%d_x_%d" % (total, nneigh), case=(big, slots), size="KF1 of %d keypoints, %d neighbours" % (total, nneigh),
                fills="win[16000] (int8 neighbour slot), cnt / off [64], idx1 up to 15 999",
                fields={"KF1 keypoint": field(total, lambda w: [p[1] for p in w[0]], [(5, h + 5)]),
                        "neighbour": field(nneigh, lambda w: [p[0] for p in w[0]])})


# ---------------------------------------------------------------- place recognition: 65 536 frames, 65 535 queries, 8 192 features
class PlaceTable:
    """One table of `nrows` frames for both Detect* queries, laid out by hand (place_cases puts the query last; here the query
    rows come first so that a database member can sit in the last row): rows 0 and 1 are query frames outside the database, the
    others are members in add order.  frames: {row: (bow dict, neighbour rows, stored score)}; every other member row is filler
    of 2-4 words that no query holds (words >= 1000)."""

    def __init__(self, nrows, frames, queries, form, min_score=0.0, connected=(), seed=9):
        import place_reference as PR
        rng = np.random.RandomState(seed)
        self.nrows, self.form, self.min_score, self.connected = nrows, form, float(min_score), tuple(connected)
        nw = rng.randint(2, 5, nrows)
        first = rng.randint(1000, 30000, nrows)
        self.bows = [[(int(first[r]) + 7 * k, 1.0 / nw[r]) for k in range(nw[r])] for r in range(nrows)]
        self.neigh = [[] for _ in range(nrows)]
        self.state = np.zeros(nrows, np.float32)
        self.in_db = np.ones(nrows, np.uint8)
        for r, bow in queries.items():
            self.bows[r], self.in_db[r] = sorted(bow.items()), 0
        for r, (bow, neigh, st) in frames.items():
            self.bows[r], self.neigh[r], self.state[r] = sorted(bow.items()), list(neigh), np.float32(st)
        self.objs = [PR.KeyFrame(r, self.bows[r], self.state[r]) for r in range(nrows)]
        self.db = PR.Database()
        for r, o in enumerate(self.objs):
            o.row = r
            if self.in_db[r]:
                self.db.add(o)
        for r in frames:
            self.objs[r].ordered = [self.objs[j] for j in self.neigh[r]]

    def view(self, form):
        """The same table read by the other query form (the relocalisation form has no minimum score and no connected set)."""
        import copy
        v = copy.copy(self)
        v.form = form
        if form == "reloc":
            v.min_score, v.connected = 0.0, ()
        return v

    def reference(self, query_row):
        """The sequential reference's result for one query row, in the shape of place_cases.expected."""
        import place_reference as PR
        for o in self.objs:                                                  # a fresh query: the reference's bookkeeping cleared
            o.mnRelocQuery, o.mnRelocWords, o.mRelocScore = -1, 0, np.float32(self.state[o.row])
            o.mnLoopQuery, o.mnLoopWords, o.mLoopScore = -1, 0, np.float32(0)
            o.scored_by = None
        q = PR.KeyFrame(10 ** 6 + query_row, self.bows[query_row])
        q.row = query_row
        q.connected = set(self.objs[j] for j in self.connected)
        if self.form == "reloc":
            res = PR.detect_relocalization_candidates(self.db, q.id, q.bow, lambda kf: kf.row)
        else:
            res = PR.detect_loop_candidates(self.db, q, self.min_score, lambda kf: kf.row)
        loop = self.form == "loop"
        common = np.zeros(self.nrows, np.int32)
        score = np.zeros(self.nrows, np.float32) if loop else self.state.copy()
        for kf in res.sharing:
            common[kf.row] = kf.mnLoopWords if loop else kf.mnRelocWords
            if getattr(kf, "scored_by", None) == q.id:
                score[kf.row] = np.float32(kf.mLoopScore if loop else kf.mRelocScore)
        return dict(cand=[kf.row for kf in res.cand], common=common, score=score, stats=(len(res.sharing), res.max_common, res.nscores))

    def csr(self, query_row):
        """The single host call's inputs (place_cases.table's dict)."""
        start = np.zeros(self.nrows + 1, np.int32)
        start[1:] = np.cumsum([len(b) for b in self.bows])
        nstart = np.zeros(self.nrows + 1, np.int32)
        nstart[1:] = np.cumsum([len(x) for x in self.neigh])
        return dict(nrows=self.nrows, bow_start=start, bow_id=np.array([w for b in self.bows for w, _ in b], np.uint32),
                    bow_val=np.array([v for b in self.bows for _, v in b], np.float64), in_db=self.in_db, neigh_start=nstart,
                    neigh=np.array([j for x in self.neigh for j in x], np.int32), state=self.state.copy(), query=query_row,
                    conn=np.array(self.connected, np.int32), min_score=np.float32(self.min_score))

    def padded(self, query_rows, cap=4):
        """The batched form's inputs (test_place_recognition.merged's dict) for the given query rows."""
        N = self.nrows
        ids, val = np.full((N, cap), 0xDEADBEEF, np.uint32), np.full((N, cap), np.nan)
        neigh = np.full((N, 10), -1, np.int32)
        for r, b in enumerate(self.bows):
            ids[r, :len(b)], val[r, :len(b)] = [w for w, _ in b], [v for _, v in b]
            neigh[r, :len(self.neigh[r])] = self.neigh[r]
        nq = len(query_rows)
        return dict(N=N, cap=cap, id=ids, val=val, nbow=np.array([len(b) for b in self.bows], np.int32), in_db=self.in_db, neigh=neigh,
                    state=self.state.copy(), query=list(query_rows), min_score=[np.float32(self.min_score)] * nq,
                    conn_start=[len(self.connected) * k for k in range(nq + 1)], conn=list(self.connected) * nq, base=[0] * nq)


def _place_frames(last, h):
    """Live frames around the two query rows 0 and 1 (query 0 = words 1-4 at 0.25).  A (the last row) equals the query (score 1),
    B (row h, the top bit alone) scores 0.875, C (row last - h, A's alias) 0.625 and is A's and B's only neighbour: A and B
    accumulate 1.625 and 1.5, C stays below 0.75 of the best, so the candidates are B then A in list order.  D (row 5) shares one
    word only and is never scored; E (row last - 1) equals the query too: the loop form lists it as connected."""
    A = {1: 0.25, 2: 0.25, 3: 0.25, 4: 0.25}
    B = {1: 0.25, 2: 0.25, 3: 0.125, 4: 0.375}
    C = {1: 0.625, 2: 0.125, 3: 0.125, 4: 0.125}
    frames = {last: (A, [last - h], 0.0), h: (B, [last - h], 0.0), last - h: (C, [], 0.0), 5: ({1: 0.5, 900: 0.5}, [], 0.125)}
    queries = {0: dict(A), 1: {1: 0.5, 2: 0.25, 4: 0.25}}
    return frames, queries


_PLACE_TABLE = {}


def place_capacity_case(form, nrows=PLACE_FRAMES):
    """Both forms read one table (built once): E is connected in the loop form; in the relocalisation form it is scored 1 and,
    alone, stays below 0.75 of the best accumulated score."""
    last, h = nrows - 1, half(nrows)
    if nrows not in _PLACE_TABLE:
        frames, queries = _place_frames(last, h)
        frames[last - 1] = (dict(queries[0]), [], 0.0)
        _PLACE_TABLE[nrows] = PlaceTable(nrows, frames, queries, None, min_score=0.5, connected=(last - 1, 7))
    t = _PLACE_TABLE[nrows].view(form)
    return dict(name="place_%s_%d" % (form, nrows), case=t, size="table of %d frames of 2-4 words" % nrows,
                fills="ordering keys first word << 16 | frame (16 bits); 40 B per (query, frame) of scratch",
                fields={"frame": field(nrows, lambda w: w["cand"], [(last - h, last)])})


def place_many_queries_case(form, nq=PLACE_QUERIES, nrows=12):
    """A small table (the same live frames, rows 11 / 8 / 3) and nq queries that alternate between the two query rows: the launch
    has nq workgroup rows, the slab nq * nrows entries; the reference runs once per distinct query."""
    last, h = nrows - 1, half(nrows)
    frames, queries = _place_frames(last, h)
    t = PlaceTable(nrows, frames, queries, form, min_score=0.25, connected=(4,)).view(form)
    rows = [k % 2 for k in range(nq)]
    rows[-1] = 0
    return dict(name="place_%s_%d_queries" % (form, nq), case=t, query_rows=rows, size="%d queries over %d frames" % (nq, nrows),
                fills="one workgroup row per query (gridDim.y = 65 535)",
                fields={"query": field(nq, lambda w: np.flatnonzero(np.asarray(w["ncand"]) > 0))})


def bow_vectors_reference(word, weight):
    """TemplatedVocabulary::transform's BowVector of one frame's per-feature (word, weight) results, by the book: features with
    weight > 0 in feature order add to their word's value from 0.0; L1 norm as the running sum of fabs over ascending words."""
    vals = {}
    for w, x in zip(word.tolist(), weight.tolist()):
        if x > 0:
            vals[w] = np.float64(vals.get(w, np.float64(0.0)) + np.float64(x))
    ids = sorted(vals)
    norm = np.float64(0.0)
    for w in ids:
        norm = np.float64(norm + abs(vals[w]))
    out = np.array([vals[w] for w in ids], np.float64)
    return np.array(ids, np.uint32), out / norm if norm > 0 else out


def bow_vectors_capacity_case(seed=8, cap=PLACE_FEATURES):
    """One frame of `cap` per-feature results over 700 words with stopped (zero-weight) features in between.  Word 3's features
    are 5 (weight 1), cap / 2 + 5 (1) and cap - 1 (2^53): added in feature order they give 2^53 + 2, with the last one first 2^53."""
    rng = np.random.RandomState(seed)
    word = rng.randint(10, 710, cap).astype(np.uint32)
    weight = np.round(rng.uniform(0.5, 12.0, cap), 6)
    weight[rng.uniform(size=cap) < 0.1] = 0.0
    for i, x in ((5, 1.0), (cap // 2 + 5, 1.0), (cap - 1, 2.0 ** 53)):
        word[i], weight[i] = 3, x
    return dict(name="bow_vectors_%d" % cap, word=word, weight=weight, size="%d features" % cap,
                fills="k_bow_vectors: 8 ranks per thread, cap * 13 + 4116 B of LDS")


# ---------------------------------------------------------------- the extractor: 4 095 px level sides, 65 533 keypoints on a level
EDGE = 16                       # minBorderX = EDGE_THRESHOLD - 3 (ORBextractor.cc:773)


def noise_frame(seed, h, w):
    """Uniform noise: FAST corners everywhere, the last cell column and row included."""
    return np.random.RandomState(seed).randint(0, 256, (h, w)).astype(np.uint8)


def banded_frame(seed, h, w, top=150, bottom=200):
    """Noise in the first `top` and the last `bottom` rows, flat grey between (no corner there: the oracle passes over it fast)."""
    img = np.full((h, w), 128, np.uint8)
    img[:top], img[h - bottom:] = noise_frame(seed, top, w), noise_frame(seed + 1, bottom, w)
    return img


def tallest_width(h=LEVEL_PX):
    """The narrowest frame of height h whose level 0 still has a quadtree root: nIni = round((w - 32) / (h - 32)) >= 1
    (ORBextractor.cc:543).  A narrower one with corners is PGORB_E_TOOSMALL: the reference divides by nIni there."""
    w = EDGE * 2 + 1
    while int(np.round(np.float32(w - 2 * EDGE) / np.float32(h - 2 * EDGE))) < 1:
        w += 1
    return w


def extractor_capacity_cases():
    """(name, image, nfeatures, nlevels, what it fills).  The wide strip runs with one level and with seven, the most a side of
    200 px allows (an eighth level of 56 px has no 30 px cell: PGORB_E_TOOSMALL).  A strip 200 px wide and 4 095 px tall has no
    quadtree root (nIni = 0) and is PGORB_E_TOOSMALL as soon as it has a corner, so the height limit runs at the narrowest width
    that has one, tallest_width() = 2 064."""
    wt = tallest_width()
    return [dict(name="wide_4095x200_1_level", img=noise_frame(1, 200, LEVEL_PX), nfeatures=2000, nlevels=1, axis="x",
                 size="4095 x 200 px, 1 level", fills="K2's record x | y << 12 | score << 24: x up to 4 075"),
            dict(name="wide_4095x200_7_levels", img=noise_frame(1, 200, LEVEL_PX), nfeatures=2000, nlevels=7, axis="x",
                 size="4095 x 200 px, 7 levels", fills="the same through a pyramid of seven levels"),
            dict(name="tall_%dx4095_1_level" % wt, img=banded_frame(3, LEVEL_PX, wt), nfeatures=2000, nlevels=1, axis="y",
                 size="%d x 4095 px, 1 level" % wt, fills="K2's record: y up to 4 075"),
            dict(name="quota_65533", img=noise_frame(2, 960, 1280), nfeatures=LEVEL_KP, nlevels=1, axis=None,
                 size="1280 x 960 px of noise, 1 level, nfeatures 65533", fills="K3's 16-bit arrival index; selCap = 65 535")]


def last_cell_start(side):
    """Where the last cell of a level side begins: cells of ceil(span / n) px from the border on, while iniX < maxBorderX - 6
    (ORBextractor.cc:784-810)."""
    span = side - 2 * EDGE
    n = int(np.float32(span) / np.float32(30.0))
    cell = int(np.ceil(np.float32(span) / n))
    j = 0
    while EDGE + (j + 1) * cell < side - EDGE - 6:
        j += 1
    return EDGE + j * cell
