"""Constructed problems for Tracking's decisions (tests/test_track_decide.py), the expected results through the restatement
(tests/track_decide_reference.py), and the runners of both forms of every entry point.

A problem is a dict of numpy arrays named as in SPECS.  Arrays that a call writes start as the sentinel byte SENT wherever the
call has no entry value of its own, and the restatement starts from the same bytes, so every comparison covers the untouched
bytes too.  Entries of a row at or past the frame's count hold in-range table indices: reading them would change a result."""
import ctypes as C

import numpy as np

import track_decide_reference as TR

f32, f64, i32, u8, u64 = np.float32, np.float64, np.int32, np.uint8, np.uint64
SENT = 0xA5
IMAX = 2 ** 31 - 1
CAM = (500.0, 510.0, 320.0, 240.0)

# the arguments of every entry point in order: int:key, in:key (an array that is read, None allowed) or io:key (in and out)
SPECS = {
    "check_replaced": "int:ntrack in:n int:nframes int:cap in:frame io:last_point int:npoints in:replaced",
    "increase_visible": "int:ntrack in:n int:nframes int:cap in:frame in:run in:kp_point int:qcap in:nq in:queries in:in_view int:npoints "
                        "io:visible",
    "query_seen_from_outliers": "int:ntrack in:n int:nframes int:cap in:frame in:kp_before in:outlier in:kp_after int:qcap in:nq in:queries int:npoints "
                                "io:query_seen",
    "track_decide": "int:ntrack int:mode in:modes int:after_retry in:n int:nframes int:cap in:frame in:run in:nmatches in:nmatches_map "
                    "in:pose_before in:kp_before in:pose_opt in:kp_opt in:outlier int:npoints in:has_obs io:found in:counters io:ok io:inliers "
                    "io:retry io:pose_final io:kp_final",
    "track_finish": "int:ntrack in:n int:nframes int:cap in:frame in:ok in:inliers io:counters in:pose_final in:kp_point io:outlier int:npoints "
                    "in:point_bad in:has_obs in:obs_start in:obs_frame int:nobs in:obs_live io:kf_point io:kf_pose io:kf_id io:kp_out io:ref_kf_out "
                    "io:new_kf io:interrupt_ba",
    "scene_median_depth": "int:nlist in:kf_list int:q in:kf_point in:n int:nframes int:cap in:poses int:npoints in:points io:median io:status",
    "scale_initial_map": "int:kf_ini int:kf_cur in:kf_point in:n int:nframes int:cap io:poses int:npoints io:points in:point_bad in:obs_start "
                         "in:obs_frame int:nobs in:obs_live io:info",
}
NAMES = tuple("pgorb_" + k for k in SPECS) + tuple("pgorb_%s_batch_device" % k for k in SPECS if k != "scale_initial_map") + \
    ("pgorb_scale_initial_map_device",)


def spec(name):
    return [s.split(":") for s in SPECS[name].split()]


def io_keys(name):
    return [k for kind, k in spec(name) if kind == "io"]


def sent(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(u8).reshape(-1)[:] = SENT
    return a


def same(a, b):
    return set(a) == set(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def diff(a, b):
    return [k for k in a if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _one(a):
    """the array, or one zero element of its type when it is empty (an empty array has no address)"""
    a = np.ascontiguousarray(a)
    return a if a.size else np.zeros(1, a.dtype)


def call_host(ext, name, P):
    """the host form on copies -> (return code, the in/out arrays afterwards)"""
    held, args = {}, [ext._h]
    for kind, k in spec(name):
        if kind == "int":
            args.append(int(P[k]))
        elif P.get(k) is None:
            args.append(None)
        else:
            held[k] = np.array(_one(P[k]))
            args.append(_p(held[k]))
    rc = getattr(ext._L, "pgorb_" + name)(*args)
    return rc, {k: held[k].reshape(-1)[:np.asarray(P[k]).size].reshape(np.asarray(P[k]).shape) for k in io_keys(name) if k in held}


def call_device(ext, name, P, stream=None):
    """the resident form on uploaded copies -> (return code, the in/out arrays afterwards)"""
    import torch
    held, args = {}, [ext._h]
    for kind, k in spec(name):
        if kind == "int":
            args.append(int(P[k]))
        elif P.get(k) is None:
            args.append(None)
        else:
            held[k] = torch.from_numpy(np.frombuffer(_one(P[k]).tobytes(), u8).copy()).cuda()
            args.append(C.c_void_p(held[k].data_ptr()))
    s = stream if stream is not None else torch.cuda.current_stream()
    fn = "pgorb_scale_initial_map_device" if name == "scale_initial_map" else "pgorb_%s_batch_device" % name
    with torch.cuda.stream(s):
        rc = getattr(ext._L, fn)(*args, C.c_void_p(s.cuda_stream))
    s.synchronize()
    out = {}
    for k in io_keys(name):
        a = np.asarray(P[k])
        out[k] = np.frombuffer(held[k].cpu().numpy().tobytes(), a.dtype)[:a.size].reshape(a.shape)
    return rc, out


def expect(name, P, rules=TR.NONE):
    """what the restatement leaves in the in/out arrays"""
    g = P.get
    if name == "check_replaced":
        return dict(last_point=TR.check_replaced(P["last_point"], P["n"], g("frame"), P["npoints"], P["replaced"], rules))
    if name == "increase_visible":
        return dict(visible=TR.increase_visible(P["kp_point"], P["n"], g("frame"), g("run"), P["nq"], P["queries"], P["in_view"], P["visible"],
                                                g("point_bad"), g("kp_before"), rules))
    if name == "query_seen_from_outliers":
        return dict(query_seen=TR.query_seen_from_outliers(P["kp_before"], P["outlier"], P["n"], g("frame"), P["nq"], P["queries"], P["npoints"],
                                                           P["query_seen"], g("kp_after")))
    if name == "track_decide":
        o = TR.decide(P["mode"], g("modes"), P["after_retry"], P["n"], g("frame"), g("run"), P["nmatches"], P["nmatches_map"], P["pose_before"],
                      P["kp_before"], P["pose_opt"], P["kp_opt"], P["outlier"], P["npoints"], g("has_obs"), P["found"], P["counters"],
                      {k: P[k] for k in ("ok", "inliers", "retry", "pose_final", "kp_final")}, rules)
        return {k: o[k] for k in io_keys(name)}
    if name == "track_finish":
        o = TR.finish(P["n"], g("frame"), P["ok"], P["inliers"], P["counters"], P["pose_final"], P["kp_point"], P["outlier"], P["npoints"],
                      g("point_bad"), g("has_obs"), P["obs_start"], P["obs_frame"], g("obs_live"), P["kf_point"], P["kf_pose"], P["kf_id"],
                      {k: P[k] for k in ("kp_out", "ref_kf_out", "new_kf", "interrupt_ba")}, rules)
        return {k: o[k] for k in io_keys(name)}
    if name == "scene_median_depth":
        if rules:
            med, st = np.array(P["median"]), np.array(P["status"])
            for e, kf in enumerate(P["kf_list"]):
                if 0 <= kf < P["nframes"]:
                    med[e], st[e] = TR.scene_median_depth(P["kf_point"][kf], int(P["n"][kf]), P["poses"][kf]["Tcw"], P["points"], P["q"],
                                                          g("point_bad"), rules)
            return dict(median=med, status=st)
        med, st = TR.median_list(P["kf_list"], P["q"], P["kf_point"], P["n"], P["poses"], P["points"], P["median"], P["status"])
        return dict(median=med, status=st)
    if name == "scale_initial_map":
        poses, points, info = TR.scale_initial_map(P["kf_ini"], P["kf_cur"], P["kf_point"], P["n"], P["poses"], P["points"], g("point_bad"),
                                                   P["obs_start"], P["obs_frame"], g("obs_live"), rules)
        return dict(poses=poses, points=points, info=info)
    raise KeyError(name)


# ---------------------------------------------------------------- builders
def rot(axis, deg):
    a = np.asarray(axis, f64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], f64)
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def make_pose(R, t):
    p = np.zeros((), TR.KF_POSE_DTYPE)
    p["Tcw"] = np.concatenate([np.asarray(R, f32).reshape(3, 3), np.asarray(t, f32).reshape(3, 1)], 1).reshape(12)
    TR.set_ow(p)
    p["fx"], p["fy"], p["cx"], p["cy"] = CAM
    p["invfx"], p["invfy"] = f32(1) / f32(CAM[0]), f32(1) / f32(CAM[1])
    return p


def poses_of(r, k):
    return np.array([make_pose(rot(r.uniform(-1, 1, 3) + [0, 0, 1.5], r.uniform(-20, 20)), r.uniform(-1, 1, 3)) for _ in range(k)], TR.KF_POSE_DTYPE)


SLOT_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)


def frames_of(r, ntrack, cap, counts, spare=2):
    """ntrack + spare frames; tracker t sits in frame perm[t] with counts[t % len(counts)] slots (cut to cap)"""
    nframes = ntrack + spare
    frame = r.permutation(nframes)[:ntrack].astype(i32)
    n = r.randint(0, cap + 1, nframes).astype(i32)
    for t in range(ntrack):
        n[frame[t]] = min(counts[t % len(counts)], cap)
    return nframes, frame, n


def slots_of(r, shape, npoints, none=0.3):
    """table indices with -1, npoints and INT32_MAX among them; a small table makes one point sit in several slots and rows"""
    s = r.randint(0, npoints, shape).astype(i32)
    u = r.uniform(size=shape)
    s[u < none] = -1
    s[(u >= none) & (u < none + 0.02)] = npoints
    s[(u >= none + 0.02) & (u < none + 0.04)] = IMAX
    return s


def stats_problem(seed, ntrack, cap, counts=SLOT_COUNTS, npoints=97, qcap=41):
    """check_replaced, increase_visible and query_seen_from_outliers on one world: replacement chains of length 1 to 3, bad points
    in the slots on entry, a gated tracker between two live ones (every third), one point held by two slots of tracker 0 and by
    four trackers"""
    r = np.random.RandomState(seed)
    nframes, frame, n = frames_of(r, ntrack, cap, counts)
    before = slots_of(r, (ntrack, cap), npoints)
    for t in range(min(ntrack, 4)):                                 # point 5: in four trackers; twice in tracker 0
        if n[frame[t]] >= 2:
            before[t, 0] = 5
    if n[frame[0]] >= 2:
        before[0, 1] = 5
    bad = (r.uniform(size=npoints) < 0.2).astype(u8)
    bad[5] = 0
    kp = before.copy()
    kp[(kp >= 0) & (kp < npoints) & (bad[np.clip(kp, 0, npoints - 1)] != 0)] = -1
    replaced = np.full(npoints, -1, i32)
    for p in range(0, npoints - 3, 4):                              # p -> p + 1 -> p + 2 for every eighth, p -> p + 1 for the others
        replaced[p] = p + 1
        if p % 8 == 0:
            replaced[p + 1] = p + 2
    run = np.ones(ntrack, u8)
    run[1::3] = 0
    nq = r.randint(0, qcap + 1, ntrack).astype(i32)
    nq[0] = qcap
    queries = (np.stack([r.permutation(npoints)[:qcap] for _ in range(ntrack)]) if qcap <= npoints else r.randint(0, npoints, (ntrack, qcap))).astype(i32)
    if qcap > 3:
        queries[:, 1], queries[:, 2] = npoints, IMAX                # out of range: no point, never in view or seen
        queries[:, 3] = -1
    return dict(ntrack=ntrack, nframes=nframes, cap=cap, n=n, frame=frame, npoints=npoints, last_point=before.copy(), replaced=replaced,
                kp_before=before, kp_point=kp, point_bad=bad, outlier=(r.uniform(size=(ntrack, cap)) < 0.3).astype(u8), run=run, qcap=qcap, nq=nq,
                kp_after=None, queries=queries, in_view=(r.uniform(size=(ntrack, qcap)) < 0.5).astype(u8), visible=r.randint(0, 1000, npoints).astype(i32),
                query_seen=sent((ntrack, qcap), u8))


def counters_of(k):
    c = np.zeros(k, TR.COUNTERS_DTYPE)
    c["pad"] = 0x5A                                                 # carried through untouched
    return c


def decide_outputs(ntrack, cap):
    return dict(ok=sent(ntrack, u8), inliers=sent(ntrack, i32), retry=sent(ntrack, u8), pose_final=sent(ntrack, TR.KF_POSE_DTYPE),
                kp_final=sent((ntrack, cap), i32))


def decide_problem(seed, ntrack, cap, counts=SLOT_COUNTS, npoints=97, mode=None, after_retry=0):
    """random stages, counts around every threshold, a gated tracker among live ones"""
    r = np.random.RandomState(seed)
    nframes, frame, n = frames_of(r, ntrack, cap, counts)
    ct = counters_of(ntrack)
    ct["frame_id"] = r.randint(100, 200, ntrack)
    ct["last_reloc_frame_id"] = ct["frame_id"] - r.randint(0, 60, ntrack)
    ct["max_frames"] = 30
    run = np.ones(ntrack, u8)
    run[1::3] = 0
    P = dict(ntrack=ntrack, mode=0 if mode is None else mode, modes=r.randint(0, 3, ntrack).astype(i32) if mode is None else None,
             after_retry=after_retry, n=n, nframes=nframes, cap=cap, frame=frame, run=run, nmatches=r.randint(12, 24, ntrack).astype(i32),
             nmatches_map=r.randint(8, 13, ntrack).astype(i32), pose_before=poses_of(r, ntrack), kp_before=slots_of(r, (ntrack, cap), npoints),
             pose_opt=poses_of(r, ntrack), kp_opt=slots_of(r, (ntrack, cap), npoints, none=0.1),
             outlier=(r.uniform(size=(ntrack, cap)) < 0.2).astype(u8), npoints=npoints, has_obs=(r.uniform(size=npoints) < 0.8).astype(u8),
             found=r.randint(0, 1000, npoints).astype(i32), counters=ct)
    P.update(decide_outputs(ntrack, cap))
    return P


LOCAL_ROW = 64


def local_row(k, npoints):
    """a TrackLocalMap row with exactly k inliers: points 0 .. k - 1 (observed), two points without observations (found, no inlier),
    an outlier, and three slots without a point, one of them flagged"""
    s = list(range(k)) + [60, 61, 70, -1, IMAX, npoints]
    o = [0] * (k + 2) + [1, 0, 1, 0]
    return s, o


def decide_sweep(after_retry=0):
    """every threshold at value - 1, value, value + 1: nmatches at 15 (reference key frame) and 20 (motion model) with nmatches_map at
    10; inliers at 30 and 50, away from and soon after a relocalisation; the wrap case; a gated tracker between live ones"""
    T = []
    for nm in (14, 15, 16):
        for mp in (9, 10, 11):
            T.append(dict(mode=TR.REFERENCE_KF, nm=nm, mp=mp))
    T.append(dict(mode=TR.LOCAL_MAP, k=40, run=0))
    for nm in (19, 20, 21):
        for mp in (9, 10, 11):
            T.append(dict(mode=TR.MOTION_MODEL, nm=nm, mp=mp))
    for k in (29, 30, 31, 49, 50, 51):
        for recent in (0, 1):
            T.append(dict(mode=TR.LOCAL_MAP, k=k, frame_id=1000, reloc=990 if recent else 970, maxf=30))
    # mnLastRelocFrameId + mMaxFrames wraps: (2^32 - 10) + 30 = 20 in 32 bits, so frame 25 is NOT soon after the relocalisation and 40
    # inliers are enough; frame 15 is, and they are not.  In 64 bits the sum is 2^32 + 20 and both frames would be
    T.append(dict(mode=TR.LOCAL_MAP, k=40, frame_id=25, reloc=2 ** 32 - 10, maxf=30))
    T.append(dict(mode=TR.LOCAL_MAP, k=40, frame_id=15, reloc=2 ** 32 - 10, maxf=30))
    T.append(dict(mode=TR.LOCAL_MAP, k=40, frame_id=2 ** 32 + 15, reloc=2 ** 32 - 10, maxf=30))      # mnId itself is 64 bits wide
    ntrack, cap, npoints = len(T), LOCAL_ROW + 3, 81
    r = np.random.RandomState(7)
    P = decide_problem(11, ntrack, cap, npoints=npoints, mode=0, after_retry=after_retry)
    P["modes"], P["frame"], P["nframes"] = np.array([t["mode"] for t in T], i32), None, ntrack
    P["n"] = np.full(ntrack, LOCAL_ROW, i32)
    P["has_obs"] = np.ones(npoints, u8)
    P["has_obs"][60:70] = 0
    P["run"] = np.array([t.get("run", 1) for t in T], u8)
    for t, d in enumerate(T):
        P["nmatches"][t], P["nmatches_map"][t] = d.get("nm", 0), d.get("mp", 0)
        if d["mode"] == TR.LOCAL_MAP:
            s, o = local_row(d["k"], npoints)
            P["kp_opt"][t, :], P["outlier"][t, :] = -1, 0
            P["kp_opt"][t, :len(s)], P["outlier"][t, :len(o)] = s, o
            P["kp_opt"][t, LOCAL_ROW:] = r.randint(0, 60, cap - LOCAL_ROW)       # past the count: would be inliers
            c = P["counters"][t]
            c["frame_id"], c["last_reloc_frame_id"], c["max_frames"] = d.get("frame_id", 500), d.get("reloc", 0) & 0xFFFFFFFF, d.get("maxf", 30)
    return P, T


def table_for_finish(nframes):
    """100 points: 0-63 three live observations; 64-71 two; 72-79 three entries, one of them dead; 80-87 bad with three live ones;
    88-95 none (visual-odometry points: has_obs 0); 96-99 three live entries, one naming a frame outside the batch"""
    start, fr, live = [0], [], []
    for p in range(100):
        k = 3 if p < 64 or 72 <= p < 88 or p >= 96 else 2 if p < 72 else 0
        for j in range(k):
            fr.append(nframes + 5 if p >= 96 and j == 1 else (p + j) % nframes)
            live.append(0 if 72 <= p < 80 and j == 0 else 1)
        start.append(len(fr))
    bad = np.zeros(100, u8)
    bad[80:88] = 1
    has = np.ones(100, u8)
    has[88:96] = 0
    return dict(npoints=100, obs_start=np.array(start, i32), obs_frame=np.array(fr, i32), obs_live=np.array(live, u8), nobs=len(fr), point_bad=bad,
                has_obs=has)


def ref_row(good):
    """a reference key frame's row: `good` points with three live observations, then one or two of every other kind"""
    return list(range(good)) + [64, 65, 72, 80, 96, -1, IMAX, 100, 88]


FINISH_DEFAULT = dict(ok=1, inl=17, good=20, nkfs=5, frame_id=1000, last_kf=900, reloc=0, maxf=30, minf=0, stopped=0, stop_req=0, accept=1, notstop=1)


def finish_sweep():
    """one tracker per rule of NeedNewKeyFrame / CreateNewKeyFrame, thresholds at value - 1, value, value + 1"""
    T = [dict(name="plain")]
    T += [dict(name="c2_%d" % inl, inl=inl) for inl in (17, 18, 19)]                         # 20 * 0.9f = 18: 17 < 18, 18 and 19 are not
    T += [dict(name="gt15_%d" % inl, inl=inl, good=40) for inl in (15, 16, 17)]
    T += [dict(name="c1a_%d" % d, frame_id=930 + d, accept=0) for d in (-1, 0, 1)]            # mapper busy: c1b is out, InterruptBA reported
    T += [dict(name="c1b_%d" % d, frame_id=910 + d, minf=10, maxf=500) for d in (-1, 0, 1)]
    T += [dict(name="c1b_busy", frame_id=915, minf=10, maxf=500, accept=0)]
    T += [dict(name="stopped", stopped=1), dict(name="stop_requested", stop_req=1)]
    T += [dict(name="reloc_recent", reloc=990, nkfs=31), dict(name="reloc_recent_few_kfs", reloc=990, nkfs=30)]
    T += [dict(name="set_not_stop_fails", notstop=0), dict(name="lost", ok=0)]
    T += [dict(name="two_kfs", nkfs=2, good=14, inl=16)]                                      # nMinObs 2: 14 + 4 = 18 -> 16.2f; with 3: 14 -> 12.6f
    T += [dict(name="wrap_kf", frame_id=25, last_kf=2 ** 32 - 10, reloc=2 ** 32 - 100)]        # 32 bits: 20 <= 25: c1a; 64 bits: no
    T += [dict(name="wrap_reloc", frame_id=2 ** 32 + 5, last_kf=100, reloc=2 ** 32 - 10, nkfs=31)]
    return [dict(FINISH_DEFAULT, **t) for t in T]


def finish_problem(T, seed=3, cap=70, live_n=64):
    """tracker t sits in frame t and its reference key frame is frame ntrack + t"""
    r = np.random.RandomState(seed)
    ntrack = len(T)
    nframes = 2 * ntrack
    tab = table_for_finish(nframes)
    n = np.full(nframes, live_n, i32)
    kf_point = r.randint(0, 64, (nframes, cap)).astype(i32)
    kp = np.full((ntrack, cap), -1, i32)
    outl = np.zeros((ntrack, cap), u8)
    ct = counters_of(ntrack)
    for t, d in enumerate(T):
        row = ref_row(d["good"])
        n[ntrack + t] = len(row)
        kf_point[ntrack + t, :len(row)] = row
        # the frame's own slots: observed points, some flagged; visual-odometry points, one flagged; no point with and without a flag
        s = list(range(30, 50)) + [88, 89, 90, -1, -1, IMAX, 100, 33]
        o = [0] * 15 + [1] * 5 + [0, 1, 0, 0, 1, 1, 0, 1]
        kp[t, :len(s)], outl[t, :len(o)] = s, o
        kp[t, live_n:], outl[t, live_n:] = r.randint(0, 64, cap - live_n), 1
        c = ct[t]
        c["frame_id"], c["last_reloc_frame_id"], c["last_kf_frame_id"] = d["frame_id"], d["reloc"] & 0xFFFFFFFF, d["last_kf"] & 0xFFFFFFFF
        c["max_frames"], c["min_frames"], c["nkfs"], c["ref_kf"], c["next_kf_id"] = d["maxf"], d["minf"], d["nkfs"], ntrack + t, 2 ** 33 + 7 * t
        c["stopped"], c["stop_requested"], c["accept_keyframes"], c["set_not_stop_ok"] = d["stopped"], d["stop_req"], d["accept"], d["notstop"]
    P = dict(ntrack=ntrack, n=n, nframes=nframes, cap=cap, frame=None, ok=np.array([d["ok"] for d in T], u8), inliers=np.array([d["inl"] for d in T], i32),
             counters=ct, pose_final=poses_of(r, ntrack), kp_point=kp, outlier=outl, kf_point=kf_point, kf_pose=poses_of(r, nframes),
             kf_id=(np.arange(nframes) + 1000).astype(u64), kp_out=sent((ntrack, cap), i32), ref_kf_out=sent(ntrack, i32), new_kf=sent(ntrack, i32),
             interrupt_ba=sent(ntrack, u8))
    P.update(tab)
    return P


def finish_random(seed, ntrack):
    r = np.random.RandomState(seed)
    T = []
    for t in range(ntrack):
        T.append(dict(FINISH_DEFAULT, name="r%d" % t, ok=int(r.uniform() < 0.8), inl=int(r.randint(10, 30)), good=int(r.randint(10, 40)),
                      nkfs=int(r.randint(1, 40)), frame_id=int(r.randint(900, 1000)), last_kf=int(r.randint(850, 990)), reloc=int(r.randint(850, 990)),
                      minf=int(r.randint(0, 20)), stopped=int(r.uniform() < 0.1), stop_req=int(r.uniform() < 0.1), accept=int(r.uniform() < 0.7),
                      notstop=int(r.uniform() < 0.8)))
    return finish_problem(T, seed)


def depth_pose():
    """row 2 = (1e-30, 0, 1 | 0): z is the point's z (the x term vanishes against any z used here), except that x = -1e-30 with z = 0
    gives -1e-60 in double, which rounds to the float -0.0: the only way to a negative zero, since a sum from +0 never is one"""
    p = make_pose(np.eye(3), [0.0, 0.0, 0.0])
    p["Tcw"][8] = f32(1e-30)
    return p


MEDIAN_ROWS = (
    ("empty", []), ("one", [3.0]), ("two", [2.0, 1.0]), ("three", [3.0, 1.0, 2.0]), ("four", [4.0, 1.0, 3.0, 2.0]),
    ("equal", [2.5] * 9), ("straddle_low", [7.0, 1.0, 1.0, 7.0, 1.0, 7.0]), ("straddle_high", [7.0, 1.0, 7.0, 7.0, 1.0, 1.0, 7.0]),
    ("negative", [-1.0, -3.0, -2.0, -5.0, 0.5]), ("all_negative", [-1.0, -3.0, -2.0]), ("zeros", ["-0", 0.0, "-0", 5.0, -5.0]),
    ("neg_zero_only", ["-0"]), ("nan", [1.0, float("nan"), 2.0]), ("infs", [float("inf"), 1.0, float("-inf"), 2.0, float("inf")]),
    ("only_inf", [float("inf")] * 3), ("bad_points", [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]), ("denormal", [1e-45, -1e-45, 0.0, 1e-40]),
)


def median_problem(q, cap=300, big=0, seed=5):
    """one frame per row of MEDIAN_ROWS with the depths as listed (the slots interleaved with -1, npoints and INT32_MAX), frames of
    the counts of SLOT_COUNTS with seeded random depths under a general pose, and with `big` a frame of 16000; the list names every
    frame, some twice, with -1 holes, and is longer than 128"""
    r = np.random.RandomState(seed)
    rows, pts, poses, names = [], [], [], []

    def point(x, y, z):
        m = np.zeros((), TR.MAP_POINT_DTYPE)
        m["pos"] = (x, y, z)
        pts.append(m)
        return len(pts) - 1
    bad_at = []
    for name, depths in MEDIAN_ROWS:
        s = []
        for z in depths:
            s += [point(-1e-30, 0.0, 0.0) if z == "-0" else point(0.0, r.uniform(-5, 5), z), -1]
        if name == "bad_points":
            bad_at += s[0:6:2]                                      # the three smallest are bad: a bad test moves the median
        rows.append(s + [IMAX, "np"])
        poses.append(depth_pose())
        names.append(name)
    general = poses_of(r, 1)[0]
    cloud = [point(*r.uniform(-3, 3, 3)) for _ in range(300)]
    for cnt in SLOT_COUNTS:
        rows.append([cloud[i] for i in r.randint(0, len(cloud), cnt)])
        poses.append(general)
        names.append("n%d" % cnt)
    if big:
        first = len(pts)
        for _ in range(big):
            point(*r.uniform(-3, 3, 3))
        rows.append(list(range(first, first + big)))
        poses.append(general)
        names.append("n%d" % big)
        cap = big
    npoints = len(pts)
    nframes = len(rows)
    kf_point = r.randint(0, npoints, (nframes, cap)).astype(i32)
    n = np.zeros(nframes, i32)
    for f, s in enumerate(rows):
        s = [npoints if v == "np" else v for v in s]
        n[f] = len(s)
        kf_point[f, :len(s)] = s
    lst = list(range(nframes)) + [-1, 0, -1, 3] + list(r.randint(-1, nframes, 130 - nframes - 4 if not big else 3))
    bad = np.zeros(npoints, u8)
    bad[bad_at] = 1
    return dict(nlist=len(lst), kf_list=np.array(lst, i32), q=q, kf_point=kf_point, n=n, nframes=nframes, cap=cap, poses=np.array(poses, TR.KF_POSE_DTYPE),
                npoints=npoints, points=np.array(pts, TR.MAP_POINT_DTYPE), median=sent(len(lst), f32), status=sent(len(lst), i32), point_bad=bad,
                names=names)


def scale_problem(kind, seed=9, cap=130):
    """the initial map: key frame 0 (pKFini) and 1 (pKFcur) share 104 points with two live observations each; `kind`:
    accepted -- point 3 sits in two slots of key frame 0 and is scaled twice; negative_median -- the scene lies behind pKFini;
    few_tracked -- five of pKFcur's points are bad: 99 tracked; empty -- pKFini holds no point"""
    r = np.random.RandomState(seed)
    npts = 104
    pts = np.zeros(npts + 2, TR.MAP_POINT_DTYPE)
    pts["pos"] = r.uniform(-1, 1, (npts + 2, 3)).astype(f32) + np.array([0, 0, 4 if kind != "negative_median" else -4], f32)
    poses = np.array([make_pose(np.eye(3), [0, 0, 0]), make_pose(rot([0, 1, 0.1], 5.0), [-0.7, 0.02, 0.1]), make_pose(rot([1, 0, 0], 2.0), [1, 1, 1])],
                     TR.KF_POSE_DTYPE)
    kf_point = r.randint(0, npts, (3, cap)).astype(i32)
    ini = list(range(npts)) + [3, -1, IMAX, npts + 2, npts]          # npts: a point that only key frame 0 holds, without observations
    cur = list(r.permutation(npts)) + [-1, npts + 1]
    if kind == "empty":
        ini = [-1, IMAX, npts + 2]
    n = np.array([len(ini), len(cur), cap], i32)
    kf_point[0, :len(ini)], kf_point[1, :len(cur)] = ini, cur
    start, fr = [0], []
    for p in range(npts + 2):
        if p < npts:
            fr += [0, 1]
        start.append(len(fr))
    bad = np.zeros(npts + 2, u8)
    if kind == "few_tracked":
        bad[10:15] = 1
    live = np.ones(len(fr), u8)
    return dict(kf_ini=0, kf_cur=1, kf_point=kf_point, n=n, nframes=3, cap=cap, poses=poses, npoints=npts + 2, points=pts, point_bad=bad,
                obs_start=np.array(start, i32), obs_frame=np.array(fr, i32), nobs=len(fr), obs_live=live, info=sent(TR.DECIDE_INFO, i32))


INDEX_KEYS = ("last_point", "kp_before", "kp_point", "kp_opt", "kf_point", "kp_after")


def clean(P):
    """the problem as the checked host forms accept it: every slot outside [-1, npoints) becomes -1, every such query 0, and an
    observation that names a frame outside the batch is marked dead (it does not exist either way)"""
    Q = dict(P)
    np_ = P["npoints"]
    for k in INDEX_KEYS:
        if Q.get(k) is not None:
            a = np.array(Q[k])
            a[(a < -1) | (a >= np_)] = -1
            Q[k] = a
    if Q.get("queries") is not None:
        a = np.array(Q["queries"])
        a[(a < 0) | (a >= np_)] = 0
        Q["queries"] = a
    if Q.get("obs_frame") is not None:
        live = np.ones(len(Q["obs_frame"]), u8) if Q.get("obs_live") is None else np.array(Q["obs_live"])
        live[(Q["obs_frame"] < 0) | (Q["obs_frame"] >= Q["nframes"])] = 0
        Q["obs_live"] = live
    return Q


def find_c2_pair(limit=1 << 24):
    """the smallest nRefMatches below `limit`, and the inlier count with it, for which the float and the double reading of
    mnMatchesInliers < nRefMatches * 0.9f disagree; None when there is none"""
    nref = np.arange(1, limit, dtype=np.int64)
    p32 = nref.astype(f32) * f32(0.9)
    p64 = nref.astype(f64) * f64(f32(0.9))
    for d in (0, 1):
        inl = np.floor(p64).astype(np.int64) + d
        w = np.nonzero((inl.astype(f32) < p32) != (inl.astype(f64) < p64))[0]
        if len(w):
            return int(inl[w[0]]), int(nref[w[0]])
    return None


# ---------------------------------------------------------------- the median list in front of CreateNewMapPoints
def cnm_problems(MC):
    """Two small problems of tests/mapping_cases.py and a table that gives every neighbour five points at camera depths around the
    median its scene states (4, and 0.2 for the tiny-baseline neighbour that the baseline test then skips).  Frames are laid out as
    MC.run_gpu_batched lays them out: problem by problem, the current key frame first.  Returns (problems, tables): kf_point, n,
    points, M, and medians = per problem (frame indices, the restatement's medians)."""
    problems = [MC.scene(s, nneigh=5 - 2 * s, npts=120) for s in range(2)]
    frames, neigh_idx = [], []
    for KF1, neigh in problems:
        frames.append(KF1)
        neigh_idx.append(list(range(len(frames), len(frames) + len(neigh))))
        frames += neigh
    cap = max(len(f["k"]) for f in frames) + 3
    kf_point = np.full((len(frames), cap), -1, i32)
    pts = []
    for (KF1, neigh), idx in zip(problems, neigh_idx):
        for N, f in zip(neigh, idx):
            T = np.asarray(N["pose"]["Tcw"], f64).reshape(3, 4)
            d = float(N["median"])
            for j, z in enumerate((0.5 * d, 0.75 * d, d, 1.5 * d, 2.0 * d)):
                m = np.zeros((), TR.MAP_POINT_DTYPE)
                m["pos"] = T[:, :3].T @ (np.array([0.1 * j, -0.05 * j, z]) - T[:, 3])
                kf_point[f, 2 * j] = len(pts)
                pts.append(m)
    points = np.array(pts, TR.MAP_POINT_DTYPE)
    n = np.array([len(f["k"]) for f in frames], i32)
    medians = [(idx, [TR.scene_median_depth(kf_point[f], int(n[f]), frames[f]["pose"]["Tcw"], points, 2)[0] for f in idx]) for idx in neigh_idx]
    return problems, dict(kf_point=kf_point, n=n, points=points, M=6, medians=medians, cap=cap)


def run_cnm_with_device_medians(MC, problems, tables, ext):
    """pgorb_scene_median_depth_batch_device over the flat neighbour table, then pgorb_create_new_map_points_batch_device reading
    that output in place; frames, padding and outputs as in MC.run_gpu_batched.  Returns per problem (points, count)."""
    import torch
    import pilotguru_amd as pg
    L, hd = ext._L, ext._h
    frames = []
    for KF1, neigh in problems:
        frames += [KF1] + list(neigh)
    B, nkf, M, cap = len(frames), len(problems), tables["M"], tables["cap"]
    kp = np.zeros((B, cap), pg.KEYPOINT_DTYPE)
    kp["x"], kp["y"], kp["angle"] = np.nan, np.nan, np.nan
    ds = np.full((B, cap, 32), 0xFF, u8)
    hp = np.ones((B, cap), u8)
    fvn, fvs, fvf = np.full((B, cap), 0xFFFFFFFF, np.uint32), np.zeros((B, cap + 1), i32), np.full((B, cap), 0xFFFFFFFF, np.uint32)
    nfv, poses = np.zeros(B, i32), np.zeros(B, TR.KF_POSE_DTYPE)
    for f, F in enumerate(frames):
        k, fv = F["k"], F["fv"]
        kp[f, :len(k)], ds[f, :len(k)], hp[f, :len(k)] = k, F["d"], F["h"]
        nfv[f] = len(fv[0])
        fvn[f, :len(fv[0])], fvs[f, :len(fv[1])], fvf[f, :len(fv[2])] = fv[0], fv[1], fv[2]
        poses[f] = F["pose"]
    nb, nn, kf1 = np.full((nkf, M), -1, i32), np.zeros(nkf, i32), np.zeros(nkf, i32)
    for k, (idx, _) in enumerate(tables["medians"]):
        nn[k], kf1[k] = len(idx), idx[0] - 1
        nb[k, :len(idx)] = idx
    keep = []

    def p(t):
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    Tt = lambda x: torch.from_numpy(np.frombuffer(np.ascontiguousarray(x).tobytes(), u8).copy()).cuda()
    md = torch.zeros(nkf * M, dtype=torch.float32, device="cuda")
    st = torch.zeros(nkf * M, dtype=torch.int32, device="cuda")
    d_nb, d_n, d_pose = Tt(nb), Tt(tables["n"]), Tt(poses)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ext._check(L.pgorb_scene_median_depth_batch_device(hd, nkf * M, p(d_nb), 2, p(Tt(tables["kf_point"])), p(d_n), B, cap, p(d_pose), len(tables["points"]),
                                                       p(Tt(tables["points"])), p(md), p(st), s))
    pts = torch.full((nkf, cap * 44), 0x7F, dtype=torch.uint8, device="cuda")
    npt = torch.full((nkf,), -9, dtype=torch.int32, device="cuda")
    cnt = torch.full((nkf, M), -9, dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_create_new_map_points_batch_device(hd, p(Tt(kp)), p(Tt(ds)), p(d_n), cap, p(Tt(fvn)), p(Tt(fvs)), p(Tt(fvf)), p(Tt(nfv)), p(d_pose),
                                                          p(Tt(hp)), p(Tt(kf1)), nkf, p(d_nb), p(Tt(nn)), M, p(md), p(pts), p(npt), p(cnt), None, None, None, s))
    torch.cuda.synchronize()
    ph = pts.cpu().numpy().view(pg.NEW_MAP_POINT_DTYPE).reshape(nkf, cap)
    return [(MC.gpu_points(ph[k, :int(npt[k])]), list(cnt[k, :len(neigh)].cpu().numpy())) for k, (KF1, neigh) in enumerate(problems)]
