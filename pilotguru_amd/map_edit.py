"""The map edits (include/pgorb.h, csrc/map_edit.hip): the edit record and its constants, pgorb_apply_map_edits from numpy arrays,
and numpy restatements of the producers that turn each step's output into an edit list at fixed positions."""
import ctypes as C

import numpy as np

MAP_EDIT_DTYPE = np.dtype([("op", "<i4"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4")])
EDIT_NOP, EDIT_ADD, EDIT_REPLACE, EDIT_ERASE, EDIT_SET_REF = 0, 1, 2, 3, 4
EDIT_APPLIED, EDIT_ALREADY, EDIT_SELF, EDIT_NOT_OBSERVED, EDIT_WENT_BAD, EDIT_BAD_INDEX, EDIT_LIMIT = 1, 2, 4, 8, 16, 32, 64
EDIT_TOUCH_CHANGED, EDIT_TOUCH_SURVIVOR, EDIT_TOUCH_STALE = 1, 2, 4
EDIT_INFO, EDIT_MAX_BAG, EDIT_MAX_EDITS, EDIT_MAX_LIST = 8, 2048, 4096, 4194304
_FUSE_ADDED, _FUSE_MERGED, _FUSE_REPLACED, _FUSE_REPLACE_REQUESTED = 2, 3, 4, 6


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def map_edits(rows):
    """an edit list from (op, a, b, c) tuples (b and c may be left out)"""
    out = np.zeros(len(rows), MAP_EDIT_DTYPE)
    for k, r in enumerate(rows):
        out[k] = tuple(r) + (0,) * (4 - len(r))
    return out


def apply_map_edits(ext, edits, kf_point, npoints, point_bad, visible, found, replaced, obs_start, obs_frame, obs_idx, obs_live, ref_obs,
                    kf_order=None, obs_cap_out=None, select_bits=0, sel_cap=None):
    """pgorb_apply_map_edits: the edits (MAP_EDIT_DTYPE) applied with the result of applying them one after another.  kf_point[f] =
    key frame f's slots; the table's flags and counters; its lists as CSR with the mask obs_live (None = all live) and ref_obs.
    obs_cap_out (default: live entries + ADD edits) and sel_cap (default: npoints) size the outputs.  Nothing passed in is changed.
    Returns a dict: kf_point (a list of arrays), point_bad, visible, found, replaced afterwards, the fresh obs_start / obs_frame /
    obs_idx / ref_obs, edit_status, touched, select (the points with touched & select_bits), info and applied; info[0] == EDIT_LIMIT:
    a capacity was exceeded and nothing was done (the state comes back as it went in, the new lists as None).  Raises ValueError for
    everything pgorb_apply_map_edits refuses."""
    fn = "apply_map_edits"
    ed = np.ascontiguousarray(edits, MAP_EDIT_DTYPE).reshape(-1)
    n, nkf, ne = int(npoints), len(kf_point), len(ed)
    if n < 0:
        raise ValueError(fn + ": npoints < 0")
    if ne > EDIT_MAX_LIST or int(np.sum(ed["op"] != EDIT_NOP)) > EDIT_MAX_EDITS:
        raise ValueError(fn + ": more than EDIT_MAX_EDITS edits that are not NOP, or a list longer than EDIT_MAX_LIST")
    if ne and (ed["op"].min() < EDIT_NOP or ed["op"].max() > EDIT_SET_REF):
        raise ValueError(fn + ": an unknown op")
    slots = [np.array(np.ascontiguousarray(s, np.int32).reshape(-1)) for s in kf_point]
    if any(len(s) > 16000 for s in slots):
        raise ValueError(fn + ": more than 16000 keypoints")
    nk = np.array([len(s) for s in slots] + ([0] if not nkf else []), np.int32)
    ko = None
    if kf_order is not None:
        ko = np.ascontiguousarray(kf_order, np.int32).reshape(-1)
        if len(ko) != nkf or not np.array_equal(np.sort(ko), np.arange(nkf)):
            raise ValueError(fn + ": kf_order is not a permutation")

    def per_point(x, dtype, name):
        x = np.array(np.ascontiguousarray(x, dtype).reshape(-1))
        if len(x) != n:
            raise ValueError("%s: %s needs one entry per point" % (fn, name))
        return x if n else np.zeros(1, dtype)
    pb, vi, fo, rp, ro = (per_point(x, dt, nm) for x, dt, nm in ((point_bad, np.uint8, "point_bad"), (visible, np.int32, "visible"), (found, np.int32, "found"),
                                                                   (replaced, np.int32, "replaced"), (ref_obs, np.int32, "ref_obs")))
    st = np.ascontiguousarray(obs_start, np.int32).reshape(-1)
    if len(st) != n + 1 or st[0] != 0 or np.any(np.diff(st) < 0):
        raise ValueError(fn + ": obs_start must rise from 0")
    m = int(st[-1])
    of, oi = (np.ascontiguousarray(x, np.int32).reshape(-1) for x in (obs_frame, obs_idx))
    lv = np.ones(m, np.uint8) if obs_live is None else np.ascontiguousarray(obs_live, np.uint8).reshape(-1)
    if min(len(of), len(oi), len(lv)) < m:
        raise ValueError(fn + ": obs_frame, obs_idx and obs_live need one entry per observation")
    of, oi, lv = of[:m], oi[:m], lv[:m]
    ln = np.diff(st)
    if np.any((ln > 0) & ((ro[:n] < -1) | (ro[:n] >= ln))):
        raise ValueError(fn + ": ref_obs lies outside the point's list")
    on = lv != 0
    if np.any(on) and (of[on].min() < 0 or of[on].max() >= nkf or oi[on].min() < 0 or np.any(oi[on] >= nk[np.clip(of[on], 0, max(nkf - 1, 0))])):
        raise ValueError(fn + ": an observation names a key frame or keypoint out of range")
    owner = np.repeat(np.arange(n, dtype=np.int64), ln)
    if len(np.unique(owner[on] * max(nkf, 1) + of[on])) != int(on.sum()):
        raise ValueError(fn + ": a list names a key frame twice")
    if obs_cap_out is None:
        obs_cap_out = int(on.sum()) + int(np.sum(ed["op"] == EDIT_ADD))
    sel_cap = n if sel_cap is None else int(sel_cap)
    if obs_cap_out < 0 or sel_cap < 0:
        raise ValueError(fn + ": a negative capacity")
    ptrs = (C.c_void_p * max(nkf, 1))()
    for f, s in enumerate(slots):
        ptrs[f] = s.ctypes.data if len(s) else None
    pad = lambda x, dt: x if len(x) else np.zeros(1, dt)
    so, fo_, io = np.zeros(n + 1, np.int32), np.zeros(max(obs_cap_out, 1), np.int32), np.zeros(max(obs_cap_out, 1), np.int32)
    ro_out, status, touched = np.full(max(n, 1), -1, np.int32), np.zeros(max(ne, 1), np.int32), np.zeros(max(n, 1), np.int32)
    select, info = np.full(max(sel_cap, 1), -1, np.int32), np.zeros(EDIT_INFO, np.int32)
    applied = ext._check(ext._L.pgorb_apply_map_edits(
        ext._h, _p(pad(ed, MAP_EDIT_DTYPE)), ne, nkf, ptrs, _p(nk), _p(ko), n, _p(pb), _p(vi), _p(fo), _p(rp), _p(st), _p(pad(of, np.int32)),
        _p(pad(oi, np.int32)), _p(pad(lv, np.uint8)), _p(ro), int(obs_cap_out), _p(so), _p(fo_), _p(io), _p(ro_out), _p(status), _p(touched),
        int(select_bits), sel_cap, _p(select), _p(info)))
    res = dict(kf_point=slots, point_bad=pb[:n], visible=vi[:n], found=fo[:n], replaced=rp[:n], edit_status=status[:ne], touched=touched[:n],
               info=info, applied=int(applied), obs_start=None, obs_frame=None, obs_idx=None, ref_obs=None, select=None)
    if info[0] != EDIT_LIMIT:
        total = int(so[-1])
        res.update(obs_start=so, obs_frame=fo_[:total].copy(), obs_idx=io[:total].copy(), ref_obs=ro_out[:n], select=select[:int(info[7])].copy())
    return res


# ---------------------------------------------------------------- the producers, restated in numpy
def _lists_hold(obs_start, obs_frame, obs_live, p, kf):
    a, b = int(obs_start[p]), int(obs_start[p + 1])
    lv = np.ones(b - a, bool) if obs_live is None else np.asarray(obs_live[a:b]) != 0
    return bool(np.any((np.asarray(obs_frame[a:b]) == kf) & lv))


def map_edits_from_keyframe(kf_point_row, npoints, point_bad, obs_start, obs_frame, obs_live, kf, cap=None):
    """pgorb_map_edits_from_keyframe_device: (edits [cap], slot_class [cap]) for the slots kf_point_row of key frame kf"""
    row = np.asarray(kf_point_row, np.int32).reshape(-1)
    cap = len(row) if cap is None else cap
    edits, cls = np.zeros(cap, MAP_EDIT_DTYPE), np.zeros(cap, np.int32)
    seen = set()
    for i, P in enumerate(row):
        P = int(P)
        if 0 <= P < npoints and not point_bad[P]:
            if P in seen or _lists_hold(obs_start, obs_frame, obs_live, P, kf):
                cls[i] = 2
            else:
                cls[i] = 1
                edits[i] = (EDIT_ADD, P, kf, i)
        if P >= 0:
            seen.add(P)
    return edits, cls


def map_edits_from_fuse(kf_point_row, kf, queries, action, best_idx, replace_point=None, qcap=None):
    """pgorb_map_edits_from_fuse_device for one problem: [qcap] edits, or [2 * qcap] with replace_point (the Sim3 form)"""
    nq = len(queries)
    qcap = nq if qcap is None else qcap
    edits = np.zeros(qcap * (2 if replace_point is not None else 1), MAP_EDIT_DTYPE)
    occupant = {}
    for q in range(nq):
        P, act, s = int(queries[q]), int(action[q]), int(best_idx[q])
        if P < 0 or not 0 <= s < len(kf_point_row):
            continue
        occ = occupant.get(s, int(kf_point_row[s]))
        if act == _FUSE_ADDED:
            edits[q] = (EDIT_ADD, P, kf, s)
            occupant[s] = P
        elif replace_point is not None:
            if act == _FUSE_REPLACE_REQUESTED:
                edits[qcap + q] = (EDIT_REPLACE, int(replace_point[q]), P, 0)
        elif act == _FUSE_MERGED:
            edits[q] = (EDIT_REPLACE, P, occ, 0)
        elif act == _FUSE_REPLACED:
            edits[q] = (EDIT_REPLACE, occ, P, 0)
            occupant[s] = P
    return edits


def map_edits_from_lba_erase(obs_start, obs_frame, erase):
    """pgorb_map_edits_from_lba_erase_device: ERASE(point of j, obs_frame[j]) at edit j where erase[j] is set"""
    st = np.asarray(obs_start, np.int64).reshape(-1)
    m = int(st[-1])
    owner = np.repeat(np.arange(len(st) - 1), np.diff(st))
    edits = np.zeros(m, MAP_EDIT_DTYPE)
    on = np.asarray(erase[:m]) != 0
    edits["op"][on], edits["a"][on], edits["b"][on] = EDIT_ERASE, owner[on], np.asarray(obs_frame[:m])[on]
    return edits


def map_edits_from_loop_matches(kf_point_row, cur_kf, matched, npoints):
    """pgorb_map_edits_from_loop_matches_device: REPLACE(occupant, matched) or ADD(matched, cur_kf, i) at edit i"""
    row = np.asarray(kf_point_row, np.int32).reshape(-1)
    edits = np.zeros(len(row), MAP_EDIT_DTYPE)
    for i, m in enumerate(np.asarray(matched).reshape(-1)[:len(row)]):
        m = int(m)
        if 0 <= m < npoints:
            edits[i] = (EDIT_REPLACE, int(row[i]), m, 0) if 0 <= row[i] < npoints else (EDIT_ADD, m, cur_kf, i)
    return edits


def observation_ids(obs_start, obs_frame, kf_id):
    """pgorb_observation_ids_device: the KeyFrame::mnId of every observation, each list ascending (uint64)"""
    st = np.asarray(obs_start, np.int64).reshape(-1)
    ids = np.asarray(kf_id, np.uint64)[np.asarray(obs_frame[:int(st[-1])], np.int64)]
    for p in range(len(st) - 1):
        ids[st[p]:st[p + 1]] = np.sort(ids[st[p]:st[p + 1]])
    return ids


def process_new_key_frame(ext, kf, kf_point, npoints, point_bad, visible, found, replaced, obs_start, obs_frame, obs_idx, obs_live, ref_obs,
                          kf_order=None):
    """LocalMapping::ProcessNewKeyFrame's loop (src/LocalMapping.cc:142-161) for key frame kf: the edits of
    map_edits_from_keyframe applied by apply_map_edits.  Returns its dict with slot_class added (1 = the observation was added:
    refresh that point; 2 = mlpRecentAddedMapPoints.push_back)."""
    if not 0 <= int(kf) < len(kf_point):
        raise ValueError("ProcessNewKeyFrame: kf is out of range")
    edits, cls = map_edits_from_keyframe(kf_point[kf], int(npoints), np.asarray(point_bad), obs_start, obs_frame, obs_live, int(kf))
    res = apply_map_edits(ext, edits, kf_point, npoints, point_bad, visible, found, replaced, obs_start, obs_frame, obs_idx, obs_live, ref_obs,
                          kf_order=kf_order, select_bits=EDIT_TOUCH_CHANGED)
    res["slot_class"] = cls
    return res
