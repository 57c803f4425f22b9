"""A numpy restatement of the decisions of the tracking thread, written from the reference source (thirdparty/orb-slam2), one
function per cited block.  Every conversion is restated with numpy's fixed-width types: an `unsigned int + int` sum is np.uint32
arithmetic (it wraps), the c2 product is np.float32, Mat::dot is a float64 sum from 0.  The layout is the library's: slots are
table indices (-1 = NULL, anything outside [0, npoints) counts as NULL and is copied through), "tracker t" is row t of the
[ntrack][cap] arrays, its frame is frame[t] and its slot count n[frame[t]].

`rules` names deliberate misreadings (MUTANTS); tests/test_track_decide.py kills each on the case constructed for it."""
import numpy as np

f32, f64, u32, u64, i32 = np.float32, np.float64, np.uint32, np.uint64, np.int32
MOTION_MODEL, REFERENCE_KF, LOCAL_MAP, WRONG_INIT, DECIDE_INFO = 0, 1, 2, 4, 4
DEPTH_EMPTY, DEPTH_NAN, DEPTH_MAX_LIST = 1, 2, 262144

KF_POSE_DTYPE = np.dtype([("Tcw", "<f4", (12,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
                          ("invfx", "<f4"), ("invfy", "<f4")])
MAP_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4")])
COUNTERS_DTYPE = np.dtype([("frame_id", "<u8"), ("last_reloc_frame_id", "<u4"), ("last_kf_frame_id", "<u4"), ("max_frames", "<i4"),
                           ("min_frames", "<i4"), ("nkfs", "<i4"), ("ref_kf", "<i4"), ("next_kf_id", "<u8"), ("stopped", "u1"),
                           ("stop_requested", "u1"), ("accept_keyframes", "u1"), ("set_not_stop_ok", "u1"), ("pad", "u1", (4,))])

MUTANTS = {name: frozenset([name]) for name in (
    "follow_chains", "double_held_once", "bad_slots_visible", "found_for_outliers", "inliers_without_has_obs",
    "le_15", "le_20", "le_10", "le_30", "le_50", "sum_64bit", "c2_double", "tracked_without_bad", "tracked_dead_obs",
    "median_count_over_q", "median_bad_test", "ow_not_refreshed", "outliers_removed_before_kf")}
NONE = frozenset()


def _rows(n, frame, ntrack, nframes, cap):
    """(frame, slot count) of every tracker"""
    out = []
    for t in range(ntrack):
        f = int(frame[t]) if frame is not None else t
        out.append((f, min(max(int(n[f]), 0), cap) if 0 <= f < nframes else 0))
    return out


def _inr(p, npoints):
    return 0 <= p < npoints


def _lt(a, b, swapped):
    """a < b, or the mutant a <= b"""
    return a <= b if swapped else a < b


def check_replaced(last_point, n, frame, npoints, replaced, rules=NONE):
    """Tracking::CheckReplacedInLastFrame, Tracking.cc:735-745: pMP = pMP->GetReplaced() when that is not NULL -- one step."""
    out = np.array(last_point, i32)
    ntrack, cap = out.shape
    for t, (f, cnt) in enumerate(_rows(n, frame, ntrack, len(n), cap)):
        for i in range(cnt):
            p = int(out[t, i])
            if _inr(p, npoints) and replaced[p] >= 0:
                p = int(replaced[p])
                while "follow_chains" in rules and _inr(p, npoints) and replaced[p] >= 0:
                    p = int(replaced[p])
                out[t, i] = p
    return out


def increase_visible(kp_point, n, frame, run, nq, queries, in_view, visible, point_bad=None, kp_point_before=None, rules=NONE):
    """The two IncreaseVisible of SearchLocalPoints, Tracking.cc:1148 (every slot that still holds a point after the bad ones were
    cleared) and :1168 (every query in view).  kp_point is pgorb_search_local_points' kp_point_out.  The mutant that counts bad
    slots reads kp_point_before, the slots on entry."""
    vis = np.array(visible, i32)
    npoints = len(vis)
    ntrack, cap = np.asarray(kp_point).shape
    for t, (f, cnt) in enumerate(_rows(n, frame, ntrack, len(n), cap)):
        if run is not None and not run[t]:
            continue
        slots = kp_point_before if "bad_slots_visible" in rules else kp_point
        seen = set()
        for i in range(cnt):
            p = int(slots[t][i])
            if _inr(p, npoints) and not ("double_held_once" in rules and p in seen):
                vis[p] += 1
                seen.add(p)
        for q in range(min(max(int(nq[t]), 0), np.asarray(queries).shape[1])):
            p = int(queries[t][q])
            if in_view[t][q] and _inr(p, npoints):
                vis[p] += 1
    return vis


def query_seen_from_outliers(kp_point, outlier, n, frame, nq, queries, npoints, seen_in, kp_after=None):
    """mnLastFrameSeen = mCurrentFrame.mnId of the discard loops, Tracking.cc:781 and :904: set for the point of every slot that the
    loop empties.  Such a slot shows as an outlier flag (outlier, None = no flags) or, after a PoseOptimization that discards and so
    clears its flags, as a slot of kp_after that no longer holds what kp_point held."""
    out = np.array(seen_in, np.uint8)
    ntrack, cap = np.asarray(kp_point).shape
    for t, (f, cnt) in enumerate(_rows(n, frame, ntrack, len(n), cap)):
        marked = {int(kp_point[t][i]) for i in range(cnt) if _inr(int(kp_point[t][i]), npoints) and
                  ((outlier is not None and outlier[t][i]) or (kp_after is not None and kp_after[t][i] != kp_point[t][i]))}
        for q in range(min(max(int(nq[t]), 0), out.shape[1])):
            out[t, q] = 1 if int(queries[t][q]) in marked else 0
    return out


def wrapped_sum(a, b, rules=NONE):
    """`unsigned int + int` (Tracking.h:213-214, :230-231): the int converts to unsigned, the sum wraps modulo 2^32, and the result
    widens to mnId's long unsigned int for the comparison"""
    if "sum_64bit" in rules:
        return int(a) + int(b)
    with np.errstate(over="ignore"):
        return int(u64(u32(a) + i32(b).astype(u32)))


def decide(mode, modes, after_retry, n, frame, run, nmatches, nmatches_map, pose_before, kp_before, pose_opt, kp_opt, outlier, npoints,
           has_obs, found, counters, out, rules=NONE):
    """bOK of one stage.  TrackReferenceKeyFrame Tracking.cc:760, :789; TrackWithMotionModel :879-886, :918; TrackLocalMap :932-964.
    `out` = dict(ok, inliers, retry, pose_final, kp_final) holding the arrays' entry bytes; a copy is updated and returned with found."""
    o = {k: np.array(v) for k, v in out.items()}
    fnd = np.array(found, i32)
    ntrack, cap = np.asarray(kp_opt).shape
    for t, (f, cnt) in enumerate(_rows(n, frame, ntrack, len(n), cap)):
        if run is not None and not run[t]:
            o["ok"][t] = 0
            continue
        m = int(modes[t]) if modes is not None else mode
        if m == LOCAL_MAP:
            inl = 0
            for i in range(cnt):                                    # :935-954
                p = int(kp_opt[t][i])
                if not _inr(p, npoints):
                    continue
                if not outlier[t][i] or "found_for_outliers" in rules:
                    fnd[p] += 1                                     # IncreaseFound()
                if not outlier[t][i] and (has_obs is None or has_obs[p] or "inliers_without_has_obs" in rules):
                    inl += 1                                        # Observations() > 0
            c = counters[t]
            recent = int(c["frame_id"]) < wrapped_sum(c["last_reloc_frame_id"], c["max_frames"], rules)
            ok = not (recent and _lt(inl, 50, "le_50" in rules)) and not _lt(inl, 30, "le_30" in rules)
            o["inliers"][t] = inl
            opt = True
        elif m == REFERENCE_KF:
            opt = not _lt(int(nmatches[t]), 15, "le_15" in rules)   # :760
            ok = opt and not _lt(int(nmatches_map[t]), 10, "le_10" in rules)
        else:
            opt = not _lt(int(nmatches[t]), 20, "le_20" in rules)   # :879, :885
            ok = opt and not _lt(int(nmatches_map[t]), 10, "le_10" in rules)
            o["retry"][t] = 1 if (not after_retry and not opt) else 0
        o["ok"][t] = 1 if ok else 0
        o["pose_final"][t] = pose_opt[t] if opt else pose_before[t]
        o["kp_final"][t, :cnt] = (kp_opt if opt else kp_before)[t][:cnt]
    o["found"] = fnd
    return o


def observations(p, obs_start, obs_frame, obs_live, nframes, rules=NONE):
    """Observations() of point p: the live entries of its list that name a frame of the batch"""
    c = 0
    for j in range(int(obs_start[p]), int(obs_start[p + 1])):
        if (obs_live is None or obs_live[j] or "tracked_dead_obs" in rules) and 0 <= obs_frame[j] < nframes:
            c += 1
    return c


def tracked_map_points(row, cnt, min_obs, npoints, point_bad, obs_start, obs_frame, obs_live, nframes, rules=NONE):
    """KeyFrame::TrackedMapPoints(minObs), KeyFrame.cc:353-378 (minObs > 0 in both callers)"""
    c = 0
    for i in range(cnt):
        p = int(row[i])
        if _inr(p, npoints) and (point_bad is None or not point_bad[p] or "tracked_without_bad" in rules) and \
                observations(p, obs_start, obs_frame, obs_live, nframes, rules) >= min_obs:
            c += 1
    return c


def c2_of(inliers, nref, rules=NONE):
    """mnMatchesInliers < nRefMatches * thRefRatio (Tracking.cc:1026): int * float is a float product, the int on the left converts
    to float"""
    if "c2_double" in rules:
        return f64(inliers) < f64(nref) * f64(f32(0.9))
    return f32(inliers) < f32(nref) * f32(0.9)


def finish(n, frame, ok, inliers, counters, pose_final, kp_point, outlier, npoints, point_bad, has_obs, obs_start, obs_frame, obs_live,
           kf_point, kf_pose, kf_id, out, rules=NONE):
    """The tail of Track() for the trackers with bOK, Tracking.cc:445-476, with NeedNewKeyFrame :968-1052 and CreateNewKeyFrame
    :1054-1132.  `out` = dict(kp_out, ref_kf_out, new_kf, interrupt_ba) holding entry bytes.  Returns the arrays afterwards."""
    o = {k: np.array(v) for k, v in out.items()}
    C, outl, kfp, kfq, kid = np.array(counters), np.array(outlier, np.uint8), np.array(kf_point, i32), np.array(kf_pose), np.array(kf_id, u64)
    ntrack, cap = np.asarray(kp_point).shape
    nframes = len(n)
    for t, (f, cnt) in enumerate(_rows(n, frame, ntrack, nframes, cap)):
        c = C[t]
        slots = np.array(kp_point[t], i32)
        if not ok[t]:
            o["kp_out"][t, :cnt] = slots[:cnt]
            o["ref_kf_out"][t], o["new_kf"][t], o["interrupt_ba"][t] = c["ref_kf"], -1, 0
            continue
        for i in range(cnt):                                        # :445-454
            p = int(slots[i])
            if _inr(p, npoints) and has_obs is not None and not has_obs[p]:
                slots[i] = -1
                outl[t, i] = 0
        need = False
        idle = bool(c["accept_keyframes"])
        early = c["stopped"] or c["stop_requested"] or \
            (int(c["frame_id"]) < wrapped_sum(c["last_reloc_frame_id"], c["max_frames"], rules) and c["nkfs"] > c["max_frames"])
        if not early:
            r = int(c["ref_kf"])
            nr = min(max(int(n[r]), 0), cap) if 0 <= r < nframes else 0
            nref = tracked_map_points(kfp[r] if nr else [], nr, 2 if c["nkfs"] <= 2 else 3, npoints, point_bad, obs_start, obs_frame, obs_live,
                                      nframes, rules)
            c1a = int(c["frame_id"]) >= wrapped_sum(c["last_kf_frame_id"], c["max_frames"], rules)
            c1b = int(c["frame_id"]) >= wrapped_sum(c["last_kf_frame_id"], c["min_frames"], rules) and idle
            inl = int(inliers[t])
            c2 = bool(c2_of(inl, nref, rules)) and inl > 15
            need = (c1a or c1b) and c2
        create = need and idle and bool(c["set_not_stop_ok"]) and 0 <= f < nframes
        if create:                                                  # :1059-1062, :1130
            row = slots.copy()
            if "outliers_removed_before_kf" in rules:
                row[:cnt][(outl[t, :cnt] != 0) & (row[:cnt] >= 0) & (row[:cnt] < npoints)] = -1
            kfp[f, :cnt] = row[:cnt]
            kfq[f] = pose_final[t]
            kid[f] = c["next_kf_id"]
            C[t]["next_kf_id"] = u64(int(c["next_kf_id"]) + 1)
            C[t]["ref_kf"], C[t]["last_kf_frame_id"], C[t]["nkfs"] = f, u32(int(c["frame_id"]) & 0xFFFFFFFF), c["nkfs"] + 1
        for i in range(cnt):                                        # :472-476
            if _inr(int(slots[i]), npoints) and outl[t, i]:
                slots[i] = -1
        o["kp_out"][t, :cnt] = slots[:cnt]
        o["ref_kf_out"][t], o["new_kf"][t], o["interrupt_ba"][t] = C[t]["ref_kf"], f if create else -1, 1 if need and not idle else 0
    o.update(counters=C, outlier=outl, kf_point=kfp, kf_pose=kfq, kf_id=kid)
    return o


def depth_of(Tcw, pos):
    """z = Rcw2.dot(x3Dw) + zcw (KeyFrame.cc:758): Mat::dot on CV_32F sums the widened products in double from 0, zcw widens, the
    sum rounds to float once"""
    s = f64(0.0)
    for k in range(3):
        s = s + f64(Tcw[8 + k]) * f64(pos[k])
    return f32(s + f64(Tcw[11]))


def scene_median_depth(row, cnt, Tcw, points, q, point_bad=None, rules=NONE):
    """KeyFrame::ComputeSceneMedianDepth(q), KeyFrame.cc:736-766 -> (depth, status).  No isBad() test.  Empty: the reference reads out
    of bounds; NaN: std::sort is undefined; both give -1 and a status.  A zero of either sign is returned as +0."""
    npoints = len(points)
    d = []
    for i in range(cnt):
        p = int(row[i])
        if _inr(p, npoints) and not ("median_bad_test" in rules and point_bad is not None and point_bad[p]):
            d.append(depth_of(Tcw, points[p]["pos"]))
    if any(np.isnan(z) for z in d):
        return f32(-1.0), DEPTH_NAN
    if not d:
        return f32(-1.0), DEPTH_EMPTY
    d.sort()
    k = len(d) // q if "median_count_over_q" in rules else (len(d) - 1) // q
    z = d[min(k, len(d) - 1)]
    return (f32(0.0) if z == 0 else z), 0


def median_list(kf_list, q, kf_point, n, poses, points, median_in, status_in):
    med, st = np.array(median_in, f32), np.array(status_in, i32)
    nframes, cap = np.asarray(kf_point).shape
    for e, kf in enumerate(kf_list):
        if 0 <= kf < nframes:
            med[e], st[e] = scene_median_depth(kf_point[kf], min(max(int(n[kf]), 0), cap), poses[kf]["Tcw"], points, q)
    return med, st


def set_ow(P):
    """SetPose's Ow = -Rcw.t()*tcw: gemm's small-matrix path, three float terms in index order, alpha = -1 applied in double"""
    T = P["Tcw"]
    for r in range(3):
        s = f32(f32(f32(T[r] * T[3]) + f32(T[4 + r] * T[7])) + f32(T[8 + r] * T[11]))
        P["Ow"][r] = f32(f64(s) * f64(-1.0))


def scale_initial_map(kf_ini, kf_cur, kf_point, n, poses, points, point_bad, obs_start, obs_frame, obs_live, rules=NONE):
    """CreateInitialMapMonocular, Tracking.cc:684-709 -> (poses, points, info)"""
    P, X = np.array(poses), np.array(points)
    nframes, cap = np.asarray(kf_point).shape
    cnt = lambda f: min(max(int(n[f]), 0), cap)
    med, st = scene_median_depth(kf_point[kf_ini], cnt(kf_ini), P[kf_ini]["Tcw"], X, 2)      # :685
    tracked = tracked_map_points(kf_point[kf_cur], cnt(kf_cur), 1, len(X), point_bad, obs_start, obs_frame, obs_live, nframes)
    wrong = bool(med < 0) or tracked < 100                         # :688
    info = np.array([st | (WRONG_INIT if wrong else 0), int(np.array(med, f32).view(i32)), tracked, 0], i32)
    if wrong:
        return P, X, info
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        inv = f32(1.0) / f32(med)                                   # :686
        for k in (3, 7, 11):                                        # :697
            P[kf_cur]["Tcw"][k] = f32(P[kf_cur]["Tcw"][k] * inv)
        if "ow_not_refreshed" not in rules:
            set_ow(P[kf_cur])                                       # :698
        scaled = set()
        for i in range(cnt(kf_ini)):                                # :702-709: once per slot
            p = int(kf_point[kf_ini][i])
            if _inr(p, len(X)):
                X[p]["pos"] = (X[p]["pos"] * inv).astype(f32)
                scaled.add(p)
    info[3] = len(scaled)
    return P, X, info
