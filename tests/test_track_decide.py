"""Tracking's decisions on the GPU (pilotguru_amd/csrc/track_decide.hip; include/pgorb.h: CheckReplacedInLastFrame, Tracking.cc:735-745;
the IncreaseVisible of SearchLocalPoints, :1148, :1168; the discard loops' mnLastFrameSeen, :781, :904; bOK of the three stages, :760,
:789, :879-886, :918, :932-964; the tail of Track(), :445-476 with NeedNewKeyFrame :968-1052 and CreateNewKeyFrame :1054-1132;
KeyFrame::TrackedMapPoints and ComputeSceneMedianDepth, KeyFrame.cc:353-378, :736-766; CreateInitialMapMonocular's scale, :684-709)
against the numpy restatement of those lines (tests/track_decide_reference.py) on the problems of tests/track_decide_cases.py.

Every output is an integer or a float obtained by a stated sequence of correctly rounded operations, so every comparison is byte for
byte, untouched bytes included (outputs start as a sentinel); no tolerance appears anywhere.

The CPU tests check presence and the record layout (they fail without the feature), expectations written out by hand, every named
mutant of the restatement on the case constructed for it, the c2 pair found by search, the wrap case, and the refusals of the Python
mirrors without a device.

Slot counts: 0, 1, 63, 64, 65, 255, 256, 257 under cap_per_frame = 300 and 70 (no multiple of 64; a count above the cap is cut to it)
and one frame at 16000, where cap_per_frame is the limit itself, 16000 = 250 * 64.

The chained frame runs the whole sequence of a monocular Track() three times on one stream without a host read and then holds every
stage against its restatement fed with what the stage before it left."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_decide_cases as K  # noqa: E402
import track_decide_reference as TR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64, i32, u8 = np.float32, np.float64, np.int32, np.uint8


@pytest.fixture(scope="module")
def sweeps():
    """the constructed problems and what the restatement leaves, computed once"""
    out = {}
    for name, P in (("stats", K.stats_problem(1, 5, 70)), ("decide0", K.decide_sweep(0)[0]), ("decide1", K.decide_sweep(1)[0]),
                    ("finish", K.finish_problem(K.finish_sweep())), ("median1", K.median_problem(1)), ("median2", K.median_problem(2)),
                    ("scale_accepted", K.scale_problem("accepted")), ("scale_negative_median", K.scale_problem("negative_median")),
                    ("scale_few_tracked", K.scale_problem("few_tracked")), ("scale_empty", K.scale_problem("empty"))):
        out[name] = P
    return out


ENTRY = {"stats": ("check_replaced", "increase_visible", "query_seen_from_outliers"), "decide0": ("track_decide",), "decide1": ("track_decide",),
         "finish": ("track_finish",), "median1": ("scene_median_depth",), "median2": ("scene_median_depth",),
         "scale_accepted": ("scale_initial_map",), "scale_negative_median": ("scale_initial_map",), "scale_few_tracked": ("scale_initial_map",),
         "scale_empty": ("scale_initial_map",)}


@pytest.fixture(scope="module")
def expected(sweeps):
    return {(name, e): K.expect(e, P) for name, P in sweeps.items() for e in ENTRY[name]}


# ---------------------------------------------------------------- CPU
C_LAYOUT = r"""
#include "include/pgorb.h"
#include <stddef.h>
#include <stdio.h>
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
int main(void)
{
    printf("pgorb_track_counters %zu\n", sizeof(pgorb_track_counters));
    F(pgorb_track_counters, frame_id); F(pgorb_track_counters, last_reloc_frame_id); F(pgorb_track_counters, last_kf_frame_id);
    F(pgorb_track_counters, max_frames); F(pgorb_track_counters, min_frames); F(pgorb_track_counters, nkfs); F(pgorb_track_counters, ref_kf);
    F(pgorb_track_counters, next_kf_id); F(pgorb_track_counters, stopped); F(pgorb_track_counters, stop_requested);
    F(pgorb_track_counters, accept_keyframes); F(pgorb_track_counters, set_not_stop_ok); F(pgorb_track_counters, pad);
    return 0;
}
"""


def test_symbols_constants_mirrors_and_null_context():
    from pilotguru_amd import _lib
    import pilotguru_amd as pg
    L = _lib.lib()
    assert len(K.NAMES) == 14
    for name in K.NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    for name in K.SPECS:
        args = [0 if kind == "int" else None for kind, _ in K.spec(name)]
        assert getattr(L, "pgorb_" + name)(None, *args) == -1, name
        dev = "pgorb_scale_initial_map_device" if name == "scale_initial_map" else "pgorb_%s_batch_device" % name
        assert getattr(L, dev)(None, *args, None) == -1, name
    hdr = open(os.path.join(ROOT, "include", "pgorb.h")).read()
    defs = dict(re.findall(r"#define\s+PGORB_((?:DECIDE|DEPTH)_\w+)\s+(\d+)", hdr))
    assert len(defs) == 8
    for k, v in defs.items():
        assert getattr(pg, k) == int(v) and getattr(_lib, "PGORB_" + k) == int(v), k
    assert (pg.DECIDE_MOTION_MODEL, pg.DECIDE_REFERENCE_KF, pg.DECIDE_LOCAL_MAP, pg.DECIDE_WRONG_INIT, pg.DECIDE_INFO) == \
        (TR.MOTION_MODEL, TR.REFERENCE_KF, TR.LOCAL_MAP, TR.WRONG_INIT, TR.DECIDE_INFO)
    assert (pg.DEPTH_EMPTY, pg.DEPTH_NAN, pg.DEPTH_MAX_LIST) == (TR.DEPTH_EMPTY, TR.DEPTH_NAN, TR.DEPTH_MAX_LIST)
    assert (pg.DECIDE_MOTION_MODEL, pg.DECIDE_REFERENCE_KF) == (pg.TRACK_MOTION_MODEL, pg.TRACK_REFERENCE_KF)      # predict's d_mode serves
    assert pg.TRACK_COUNTERS_DTYPE == TR.COUNTERS_DTYPE and pg.KF_POSE_DTYPE == TR.KF_POSE_DTYPE and pg.MAP_POINT_DTYPE == TR.MAP_POINT_DTYPE
    for cls, fn in ((pg.Tracking, "CheckReplacedInLastFrame"), (pg.Tracking, "IncreaseVisible"), (pg.Tracking, "QuerySeenFromOutliers"),
                    (pg.Tracking, "Decide"), (pg.Tracking, "FinishFrame"), (pg.Tracking, "ScaleInitialMap"), (pg.LocalMapping, "SceneMedianDepth")):
        assert callable(getattr(cls, fn))
    mk = open(os.path.join(ROOT, "pilotguru_amd", "csrc", "Makefile")).read()
    assert "track_decide.hip" in mk and "-ffp-contract=off" in mk
    # what is still left to the caller is named once, and the old sentences are gone
    assert "Still left to the caller: the relocalisation bookkeeping" in hdr
    for gone in ("the caller does IncreaseVisible", "so the caller computes it", "bOK itself and the nmatches retries"):
        assert gone not in hdr, gone


def test_counters_layout_agrees_with_the_header(tmp_path):
    from pilotguru_amd import _lib
    src, exe = os.path.join(str(tmp_path), "layout.c"), os.path.join(str(tmp_path), "layout")
    open(src, "w").write(C_LAYOUT)
    subprocess.run(["cc", "-std=c99", "-I", ROOT, src, "-o", exe], check=True)
    got = dict(line.split() for line in subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines())
    dt, seen = _lib.TRACK_COUNTERS_DTYPE, 0
    for k, v in got.items():
        if "." in k:
            assert dt.fields[k.split(".")[1]][1] == int(v), k
            seen += 1
        else:
            assert dt.itemsize == int(v) == 48
    assert seen == len(dt.names) == 13


def _one_tracker(slots, **kw):
    """a one-tracker, one-frame problem around a hand-written row"""
    s = np.array([slots], i32)
    return dict(dict(ntrack=1, nframes=1, cap=s.shape[1], n=np.array([s.shape[1]], i32), frame=None), **kw), s


def test_hand_written_expectations(sweeps, expected):
    # CheckReplacedInLastFrame: 0 -> 1 -> 2 is ONE step from 0; -1, npoints and INT32_MAX are no point; 3 has no replacement
    rep = np.array([1, 2, -1, -1, -1, 0], i32)
    base, s = _one_tracker([0, 1, 2, 3, -1, 6, K.IMAX, 5])
    assert TR.check_replaced(s, base["n"], None, 6, rep).tolist() == [[1, 2, 2, 3, -1, 6, K.IMAX, 0]]
    assert TR.check_replaced(s, np.array([3], i32), None, 6, rep).tolist() == [[1, 2, 2, 3, -1, 6, K.IMAX, 5]]      # the count bounds the row
    # IncreaseVisible: point 2 in two slots counts twice; the query in view adds one; a gated tracker adds nothing
    base, s = _one_tracker([2, -1, 2, 0, 7, 4])
    q, iv = np.array([[4, 1, 0, 7]], i32), np.array([[1, 0, 1, 1]], u8)
    vis = TR.increase_visible(s, base["n"], None, None, np.array([3], i32), q, iv, np.array([10, 20, 30, 40, 50], i32))
    assert vis.tolist() == [12, 20, 32, 40, 52]                     # 0: slot + query; 2: two slots; 4: slot + query; query 3 is past nq
    assert TR.increase_visible(s, base["n"], None, np.array([0], u8), np.array([3], i32), q, iv, np.zeros(5, i32)).tolist() == [0] * 5
    # query_seen: the points of the outlier slots 1 and 3 (4 and 2), not the inlier 0 and not beyond nq
    base, s = _one_tracker([0, 4, 1, 2, -1])
    seen = TR.query_seen_from_outliers(s, np.array([[0, 1, 0, 1, 1]], u8), base["n"], None, np.array([4], i32), np.array([[2, 0, 4, 3, 4]], i32), 5,
                                       K.sent((1, 5), u8))
    assert seen.tolist() == [[1, 0, 1, 0, K.SENT]]
    # the same from the slots after a discarding PoseOptimization, whose flags are all clear: slots 1 and 3 were emptied
    seen = TR.query_seen_from_outliers(s, None, base["n"], None, np.array([4], i32), np.array([[2, 0, 4, 3, 4]], i32), 5, K.sent((1, 5), u8),
                                       np.array([[0, -1, 1, -1, -1]], i32))
    assert seen.tolist() == [[1, 0, 1, 0, K.SENT]]
    # the stages: (stage, nmatches, nmatches_map) -> (ok, final = opt?, retry)
    P, T = sweeps["decide0"], K.decide_sweep(0)[1]
    e, e1 = expected[("decide0", "track_decide")], expected[("decide1", "track_decide")]
    for t, d in enumerate(T):
        opt = e["pose_final"][t].tobytes() == P["pose_opt"][t].tobytes()
        before = e["pose_final"][t].tobytes() == P["pose_before"][t].tobytes()
        if d.get("run", 1) == 0:
            assert e["ok"][t] == 0 and e["pose_final"][t].tobytes() == K.sent(1, TR.KF_POSE_DTYPE).tobytes() and e["inliers"][t] == K.sent(1, i32)[0]
        elif d["mode"] == TR.REFERENCE_KF:
            assert (e["ok"][t], opt, before) == (int(d["nm"] >= 15 and d["mp"] >= 10), d["nm"] >= 15, d["nm"] < 15) and e["retry"][t] == K.SENT
            assert e["kp_final"][t, :64].tolist() == (P["kp_opt"] if d["nm"] >= 15 else P["kp_before"])[t, :64].tolist()
        elif d["mode"] == TR.MOTION_MODEL:
            assert (e["ok"][t], opt, before) == (int(d["nm"] >= 20 and d["mp"] >= 10), d["nm"] >= 20, d["nm"] < 20)
            assert e["retry"][t] == int(d["nm"] < 20) and e1["retry"][t] == 0 and e1["ok"][t] == e["ok"][t]
        else:
            recent = d["frame_id"] < ((d["reloc"] + d["maxf"]) % 2 ** 32)
            assert e["inliers"][t] == d["k"] and e["ok"][t] == int(d["k"] >= (50 if recent else 30)) and opt
    assert e["kp_final"][:, 64:].tobytes() == K.sent((len(T), 3), i32).tobytes()                 # past the count: untouched
    wrap = [t for t, d in enumerate(T) if d.get("reloc", 0) > 2 ** 31]
    assert e["ok"][wrap].tolist() == [1, 0, 1] and len(wrap) == 3
    # found: every slot with a point and no flag, observed or not; tracker 19 is the first local-map row, 29 inliers + 2 unobserved
    first = next(t for t, d in enumerate(T) if d["mode"] == TR.LOCAL_MAP and d.get("run", 1))
    solo = {k: (v[first:first + 1] if isinstance(v, np.ndarray) and len(v) == len(T) and k != "n" else v) for k, v in P.items()}
    solo.update(ntrack=1, nframes=len(T), frame=np.array([first], i32), modes=None, mode=TR.LOCAL_MAP, run=None)
    d = K.expect("track_decide", solo)["found"] - P["found"]
    assert d[:29].tolist() == [1] * 29 and d[29:60].sum() == 0 and d[60:62].tolist() == [1, 1] and d[70] == 0 and d.sum() == 31
    # the tail of Track()
    P, T = sweeps["finish"], K.finish_sweep()
    e = expected[("finish", "track_finish")]
    made = {d["name"]: int(e["new_kf"][t]) >= 0 for t, d in enumerate(T)}
    assert made == {"plain": True, "c2_17": True, "c2_18": False, "c2_19": False, "gt15_15": False, "gt15_16": True, "gt15_17": True,
                    "c1a_-1": False, "c1a_0": False, "c1a_1": False, "c1b_-1": False, "c1b_0": True, "c1b_1": True, "c1b_busy": False,
                    "stopped": False, "stop_requested": False, "reloc_recent": False, "reloc_recent_few_kfs": True, "set_not_stop_fails": False,
                    "lost": False, "two_kfs": True, "wrap_kf": True, "wrap_reloc": True}
    ib = {d["name"]: int(e["interrupt_ba"][t]) for t, d in enumerate(T)}
    assert [k for k, v in ib.items() if v] == ["c1a_0", "c1a_1"]     # the condition held and the mapper was busy
    t = 0                                                           # "plain": the frame's row, in the reference's order
    assert e["kp_out"][t, :28].tolist() == list(range(30, 45)) + [-1] * 5 + [-1, -1, -1, -1, -1, K.IMAX, 100, -1]
    assert e["kf_point"][t, :28].tolist() == list(range(30, 50)) + [-1, -1, -1, -1, -1, K.IMAX, 100, 33]      # outliers still present
    assert e["outlier"][t, :28].tolist() == [0] * 15 + [1] * 5 + [0, 0, 0, 0, 1, 1, 0, 1]                    # the VO slot's flag is cleared
    c0, c1 = P["counters"][t], e["counters"][t]
    assert (c1["ref_kf"], c1["nkfs"], c1["last_kf_frame_id"], c1["next_kf_id"]) == (0, c0["nkfs"] + 1, 1000, c0["next_kf_id"] + 1)
    assert e["kf_id"][t] == c0["next_kf_id"] and e["kf_pose"][t].tobytes() == P["pose_final"][t].tobytes() and e["ref_kf_out"][t] == 0
    t = next(i for i, d in enumerate(T) if d["name"] == "wrap_reloc")
    assert e["counters"][t]["last_kf_frame_id"] == 5                # (uint32)(2^32 + 5)
    t = next(i for i, d in enumerate(T) if d["name"] == "lost")
    assert e["kp_out"][t, :64].tolist() == P["kp_point"][t, :64].tolist() and e["outlier"][t].tolist() == P["outlier"][t].tolist()
    assert e["counters"][t].tobytes() == P["counters"][t].tobytes() and e["kf_point"][t].tolist() == P["kf_point"][t].tolist()
    t = next(i for i, d in enumerate(T) if d["name"] == "set_not_stop_fails")      # (a) and (d) ran, (c) did not
    assert e["kp_out"][t, :28].tolist() == e["kp_out"][0, :28].tolist() and e["kf_point"][t].tolist() == P["kf_point"][t].tolist()
    # TrackedMapPoints by hand: 20 good + (64, 65: two observations) + 72 (one of three dead) + 80 (bad) + 96 (one outside the batch)
    tab = K.table_for_finish(8)
    tm = lambda m, **kw: TR.tracked_map_points(K.ref_row(20), len(K.ref_row(20)), m, 100, tab["point_bad"], tab["obs_start"], tab["obs_frame"],
                                               tab["obs_live"], 8, **kw)
    assert (tm(3), tm(2), tm(1)) == (20, 24, 24)
    # the median
    for q, want in ((1, dict(empty=-1, one=3, two=2, three=3, four=4, equal=2.5, straddle_low=7, straddle_high=7, negative=0.5, all_negative=-1,
                             zeros=5, neg_zero_only=0, nan=-1, infs=np.inf, only_inf=np.inf, bad_points=6, denormal=1e-40)),
                    (2, dict(empty=-1, one=3, two=1, three=2, four=2, equal=2.5, straddle_low=1, straddle_high=7, negative=-2, all_negative=-2,
                             zeros=0, neg_zero_only=0, nan=-1, infs=2, only_inf=np.inf, bad_points=3, denormal=0))):
        P, e = sweeps["median%d" % q], expected[("median%d" % q, "scene_median_depth")]
        for f, name in enumerate(P["names"][:len(K.MEDIAN_ROWS)]):
            assert e["median"][f] == f32(want[name]) and (want[name] < 0 or not np.signbit(e["median"][f])), (q, name)
            assert e["status"][f] == (TR.DEPTH_EMPTY if name == "empty" else TR.DEPTH_NAN if name == "nan" else 0), (q, name)
        holes = [i for i, kf in enumerate(P["kf_list"]) if kf < 0]
        assert len(holes) >= 2 and e["median"][holes].tobytes() == K.sent(len(holes), f32).tobytes()
    assert TR.depth_of(K.depth_pose()["Tcw"], np.array([-1e-30, 0, 0], f32)).tobytes() == f32(-0.0).tobytes()      # the negative zero is real
    # the initial map
    P, e = sweeps["scale_accepted"], expected[("scale_accepted", "scale_initial_map")]
    med = e["info"][1:2].view(f32)[0]
    inv = f32(1.0) / med
    assert e["info"][0] == 0 and e["info"][2] == 104 and e["info"][3] == 105 and 3.5 < med < 4.5
    assert e["points"]["pos"][0].tolist() == (P["points"]["pos"][0] * inv).tolist()
    assert e["points"]["pos"][3].tolist() == ((P["points"]["pos"][3] * inv).astype(f32) * inv).tolist()           # two slots: scaled twice
    assert e["points"][105].tobytes() == P["points"][105].tobytes() and e["poses"][[0, 2]].tobytes() == P["poses"][[0, 2]].tobytes()
    assert e["poses"][1]["Tcw"][[3, 7, 11]].tolist() == (P["poses"][1]["Tcw"][[3, 7, 11]] * inv).tolist()
    assert e["poses"][1]["Tcw"][[0, 5, 10]].tolist() == P["poses"][1]["Tcw"][[0, 5, 10]].tolist() and e["poses"][1]["Ow"].tolist() != P["poses"][1]["Ow"].tolist()
    for kind, status, tracked in (("negative_median", TR.WRONG_INIT, 104), ("few_tracked", TR.WRONG_INIT, 99), ("empty", TR.WRONG_INIT | TR.DEPTH_EMPTY, 104)):
        P, e = sweeps["scale_" + kind], expected[("scale_" + kind, "scale_initial_map")]
        assert e["info"][0] == status and e["info"][2] == tracked and e["info"][3] == 0
        assert e["poses"].tobytes() == P["poses"].tobytes() and e["points"].tobytes() == P["points"].tobytes()       # nothing written


NAMED = (("follow_chains", "stats", "check_replaced"), ("double_held_once", "stats", "increase_visible"), ("bad_slots_visible", "stats", "increase_visible"),
         ("found_for_outliers", "decide0", "track_decide"), ("inliers_without_has_obs", "decide0", "track_decide"), ("le_15", "decide0", "track_decide"),
         ("le_20", "decide0", "track_decide"), ("le_10", "decide0", "track_decide"), ("le_30", "decide0", "track_decide"), ("le_50", "decide0", "track_decide"),
         ("sum_64bit", "decide0", "track_decide"), ("sum_64bit", "finish", "track_finish"), ("tracked_without_bad", "finish", "track_finish"),
         ("tracked_dead_obs", "finish", "track_finish"), ("outliers_removed_before_kf", "finish", "track_finish"),
         ("median_count_over_q", "median2", "scene_median_depth"), ("median_bad_test", "median2", "scene_median_depth"),
         ("ow_not_refreshed", "scale_accepted", "scale_initial_map"))


def test_every_mutant_is_caught_by_name(sweeps, expected):
    """each misreading changes the result of the problem constructed for it; c2_double has no problem: see the c2 test"""
    assert {m for m, _, _ in NAMED} | {"c2_double"} == set(TR.MUTANTS)
    for mutant, prob, entry in NAMED:
        assert not K.same(K.expect(entry, sweeps[prob], TR.MUTANTS[mutant]), expected[(prob, entry)]), mutant
    # and where: the threshold mutants move exactly the tracker that sits on the threshold
    T = K.decide_sweep(0)[1]
    e = expected[("decide0", "track_decide")]
    for mutant, at in (("le_15", dict(mode=TR.REFERENCE_KF, nm=15)), ("le_20", dict(mode=TR.MOTION_MODEL, nm=20)), ("le_30", dict(mode=TR.LOCAL_MAP, k=30)),
                       ("le_50", dict(mode=TR.LOCAL_MAP, k=50))):
        m = K.expect("track_decide", sweeps["decide0"], TR.MUTANTS[mutant])
        moved = [t for t in range(len(T)) if m["ok"][t] != e["ok"][t]]
        assert moved and all(all(T[t].get(k) == v for k, v in at.items()) for t in moved), (mutant, moved)
    m = K.expect("track_decide", sweeps["decide0"], TR.MUTANTS["le_10"])
    assert {T[t]["mp"] for t in range(len(T)) if m["ok"][t] != e["ok"][t]} == {10}
    m = K.expect("track_decide", sweeps["decide0"], TR.MUTANTS["sum_64bit"])
    assert [T[t]["frame_id"] for t in range(len(T)) if m["ok"][t] != e["ok"][t]] == [25, 2 ** 32 + 15]
    F = K.finish_sweep()
    e = expected[("finish", "track_finish")]
    m = K.expect("track_finish", sweeps["finish"], TR.MUTANTS["sum_64bit"])
    assert [F[t]["name"] for t in range(len(F)) if m["new_kf"][t] != e["new_kf"][t]] == ["wrap_kf", "wrap_reloc"]
    for mutant in ("tracked_without_bad", "tracked_dead_obs"):      # 21 * 0.9f = 18.9: 18 inliers now pass c2
        m = K.expect("track_finish", sweeps["finish"], TR.MUTANTS[mutant])
        assert "c2_18" in [F[t]["name"] for t in range(len(F)) if m["new_kf"][t] != e["new_kf"][t]], mutant


def test_c2_float_and_double_disagree_only_above_the_capacity():
    """mnMatchesInliers < nRefMatches * thRefRatio: the float and the double reading first disagree at nRefMatches = 1572869 with
    1415582 inliers -- 1572869 * 0.9f = 1415582.07 in double, which is above 2^20 where a float's spacing is 0.125, and rounds to
    1415582.0f, so 1415582 < product holds in double and not in float.  A product below 2^17 keeps three fractional bits more than the
    0.1 steps need, so NO PAIR EXISTS with nRefMatches <= 16000, the most a key frame's row can hold: no problem on the device can
    tell the two readings apart, and the c2_double mutant is pinned here, on the restatement's own expression."""
    assert K.find_c2_pair() == (1415582, 1572869)
    assert K.find_c2_pair(16001) is None
    assert not TR.c2_of(1415582, 1572869) and TR.c2_of(1415582, 1572869, TR.MUTANTS["c2_double"])
    assert TR.c2_of(1415581, 1572869) and TR.c2_of(1415581, 1572869, TR.MUTANTS["c2_double"])
    assert not TR.c2_of(18, 20) and TR.c2_of(17, 20) and f32(20) * f32(0.9) == f32(18)


def test_wrapped_sum_is_32_bit_unsigned():
    assert TR.wrapped_sum(2 ** 32 - 10, 30) == 20 and TR.wrapped_sum(2 ** 32 - 10, 30, TR.MUTANTS["sum_64bit"]) == 2 ** 32 + 20
    assert TR.wrapped_sum(5, -10) == 2 ** 32 - 5                    # a negative mMaxFrames converts to unsigned first
    assert TR.wrapped_sum(2 ** 32 - 30, 30) == 0 and TR.wrapped_sum(2 ** 32 - 31, 30) == 2 ** 32 - 1


class _NoLibrary:
    """an extractor whose library must not be reached"""
    class _L:
        def __getattr__(self, name):
            raise AssertionError("the library was called")
    _L = _L()
    _h = None

    @staticmethod
    def _check(rc):
        return rc


def _mirror_calls(pg, ext):
    """name -> a function of a problem that calls the Python mirror"""
    return {
        "check_replaced": lambda P: pg.Tracking.CheckReplacedInLastFrame(ext, P["last_point"], P["n"], P["npoints"], P["replaced"], P["frame"]),
        "increase_visible": lambda P: pg.Tracking.IncreaseVisible(ext, P["kp_point"], P["n"], P["nq"], P["queries"], P["in_view"], P["visible"], P["frame"], P["run"]),
        "query_seen_from_outliers": lambda P: pg.Tracking.QuerySeenFromOutliers(ext, P["kp_before"], P["outlier"], P["n"], P["nq"], P["queries"], P["npoints"],
                                                                               P["frame"], P["kp_after"]),
        "track_decide": lambda P: pg.Tracking.Decide(ext, P["mode"] if P["modes"] is None else P["modes"], P["n"], P["nmatches"], P["nmatches_map"],
                                                     P["pose_before"], P["kp_before"], P["pose_opt"], P["kp_opt"], P["outlier"], P["npoints"], P["found"],
                                                     P["counters"], P["has_obs"], P["after_retry"], P["frame"], P["run"]),
        "track_finish": lambda P: pg.Tracking.FinishFrame(ext, P["n"], P["ok"], P["inliers"], P["counters"], P["pose_final"], P["kp_point"], P["outlier"],
                                                          P["npoints"], P["obs_start"], P["obs_frame"], P["kf_point"], P["kf_pose"], P["kf_id"], P["point_bad"],
                                                          P["has_obs"], P["obs_live"], P["frame"]),
        "scene_median_depth": lambda P: pg.LocalMapping.SceneMedianDepth(ext, P["kf_list"], P["q"], P["kf_point"], P["n"], P["poses"], P["points"]),
        "scale_initial_map": lambda P: pg.Tracking.ScaleInitialMap(ext, P["kf_ini"], P["kf_cur"], P["kf_point"], P["n"], P["poses"], P["points"],
                                                                   P["obs_start"], P["obs_frame"], P["point_bad"], P["obs_live"]),
    }


def _malformed(name, P):
    """(what is wrong, the problem with it) for what the checked form of `name` refuses"""
    def v(**kw):
        Q = dict(P)
        for k, (at, x) in kw.items():
            a = np.array(Q[k])
            a[at] = x
            Q[k] = a
        return Q
    if name in ("check_replaced", "increase_visible", "query_seen_from_outliers", "track_decide", "track_finish"):
        yield "a negative count of a frame", v(n=(int(P["frame"][0]) if P["frame"] is not None else 0, -1))
        yield "a count above the capacity", v(n=(int(P["frame"][0]) if P["frame"] is not None else 0, P["cap"] + 1))
        key = {"check_replaced": "last_point", "increase_visible": "kp_point", "query_seen_from_outliers": "kp_before", "track_decide": "kp_opt",
               "track_finish": "kp_point"}[name]
        t = next(t for t in range(P["ntrack"]) if P["n"][P["frame"][t] if P["frame"] is not None else t] > 0)      # a slot inside its row's count
        yield "a slot of npoints", v(**{key: ((t, 0), P["npoints"])})
        yield "a slot of -2", v(**{key: ((t, 0), -2)})
        if P["frame"] is not None:
            yield "a frame out of range", v(frame=(0, P["nframes"]))
    if name == "check_replaced":
        yield "a replacement out of range", v(replaced=(0, P["npoints"]))
    if name in ("increase_visible", "query_seen_from_outliers"):
        yield "a query count above qcap", v(nq=(0, P["qcap"] + 1))
        yield "a query out of range", v(queries=((0, 0), -1))
    if name == "track_decide":
        yield "an unknown mode", v(modes=(0, 3))
    if name == "track_finish":
        yield "two trackers on one frame row", dict(P, frame=np.array([0, 0] + list(range(2, P["ntrack"])), i32))
        c = np.array(P["counters"])
        c[0]["ref_kf"] = 1
        yield "a reference key frame that is a tracker's frame row", dict(P, counters=c)
        c = np.array(P["counters"])
        c[0]["ref_kf"] = P["nframes"]
        yield "a reference key frame out of range", dict(P, counters=c)
        yield "obs_start not rising", v(obs_start=(1, 7))
        yield "a live observation outside the batch", v(obs_frame=(0, P["nframes"]))
    if name == "scene_median_depth":
        yield "q of 0", dict(P, q=0)
        yield "a key frame out of range", v(kf_list=(0, P["nframes"]))
        yield "a slot out of range", v(kf_point=((1, 0), P["npoints"]))
        yield "a count above the capacity", v(n=(0, P["cap"] + 1))
    if name == "scale_initial_map":
        yield "kf_ini == kf_cur", dict(P, kf_cur=0)
        yield "kf_cur out of range", dict(P, kf_cur=3)
        yield "a slot out of range", v(kf_point=((1, 0), -2))
        yield "obs_start not ending at nobs", v(obs_start=(-1, 5))
        yield "a negative count", v(n=(2, -1))


PROBLEM_OF = {"check_replaced": "stats", "increase_visible": "stats", "query_seen_from_outliers": "stats", "track_decide": "decide0",
              "track_finish": "finish", "scene_median_depth": "median2", "scale_initial_map": "scale_accepted"}


def test_python_mirrors_refuse_malformed_input_without_a_device(sweeps):
    """the checks of the host forms, restated in the mirrors: a negative count, indices out of range, two trackers on one frame row,
    cap_per_frame > 16000 and a missing array are refused before the library is reached; a well-formed problem reaches it"""
    import pilotguru_amd as pg
    calls = _mirror_calls(pg, _NoLibrary())
    for name, prob in PROBLEM_OF.items():
        P = K.clean(sweeps[prob])
        with pytest.raises(AssertionError, match="the library was called"):
            calls[name](P)
        n = 0
        for what, Q in _malformed(name, P):
            with pytest.raises(ValueError):
                calls[name](Q)
                pytest.fail("%s accepted %s" % (name, what))
            n += 1
        assert n >= 4, name
    wide = np.full((1, 16001), -1, i32)
    n1 = np.array([0], i32)
    with pytest.raises(ValueError):
        pg.Tracking.CheckReplacedInLastFrame(_NoLibrary(), wide, n1, 4, np.full(4, -1, i32))
    with pytest.raises(ValueError):
        pg.LocalMapping.SceneMedianDepth(_NoLibrary(), [0], 2, wide, n1, np.zeros(1, pg.KF_POSE_DTYPE), np.zeros(1, pg.MAP_POINT_DTYPE))
    with pytest.raises(ValueError):
        pg.Tracking.IncreaseVisible(_NoLibrary(), np.full((1, 4), -1, i32), n1, [0], np.zeros((1, 16001), i32), np.zeros((1, 16001), u8), np.zeros(4, i32))
    P = K.clean(sweeps["stats"])
    with pytest.raises((ValueError, TypeError)):
        pg.Tracking.CheckReplacedInLastFrame(_NoLibrary(), P["last_point"], P["n"], P["npoints"], None, P["frame"])
    with pytest.raises(ValueError):
        pg.Tracking.CheckReplacedInLastFrame(_NoLibrary(), P["last_point"], P["n"], -1, P["replaced"], P["frame"])


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    return pg.ORBextractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240)


def _check(ext, name, P, host=True, want=None, stream=None):
    """the resident form on P as it stands (indices out of range included), and both forms on the problem the checked form accepts"""
    want = K.expect(name, P) if want is None else want
    rc, got = K.call_device(ext, name, P, stream)
    assert rc == 0 and K.same(got, want), (name, rc, K.diff(got, want))
    if host:
        Q = K.clean(P)
        wq = K.expect(name, Q)
        rc, got = K.call_device(ext, name, Q)
        assert rc == 0 and K.same(got, wq), (name, "clean", rc, K.diff(got, wq))
        rc, got = K.call_host(ext, name, Q)
        assert rc >= 0 and K.same(got, wq), (name, "host", rc, K.diff(got, wq))
        return rc
    return got


STATS = ("check_replaced", "increase_visible", "query_seen_from_outliers")


@pytest.mark.gpu
@pytest.mark.parametrize("ntrack,cap", [(1, 70), (3, 300), (130, 70), (130, 300)])
def test_gpu_statistics_equal_the_reference_in_both_forms(ext, ntrack, cap):
    """every slot count under both capacities, 1, 3 and 130 trackers, a gated tracker between live ones, a point in two slots of one
    frame and in four trackers, -1, npoints and INT32_MAX in the slots and queries"""
    P = K.stats_problem(ntrack * 1000 + cap, ntrack, cap)
    assert P["n"][P["frame"]].tolist() == [min(K.SLOT_COUNTS[t % 8], cap) for t in range(ntrack)]
    for name in STATS:
        _check(ext, name, P)
    # query_seen from the slots a discarding PoseOptimization leaves (flags cleared): the same marks, with no flags and with zeros
    after = np.where(P["outlier"] != 0, -1, P["kp_before"]).astype(i32)
    want = K.expect("query_seen_from_outliers", P)
    _check(ext, "query_seen_from_outliers", dict(P, outlier=None, kp_after=after), host=False, want=want)
    _check(ext, "query_seen_from_outliers", dict(P, outlier=np.zeros_like(P["outlier"]), kp_after=after), want=want)


@pytest.mark.gpu
def test_gpu_statistics_at_16000_slots(ext):
    P = K.stats_problem(4, 3, 16000, counts=(16000, 257, 15999), npoints=5000, qcap=16000)
    for name in STATS:
        _check(ext, name, P)


@pytest.mark.gpu
def test_gpu_counters_accumulate_over_two_calls(ext):
    """visible after two successive IncreaseVisible calls and found after two successive decisions, compared exactly"""
    P = K.stats_problem(8, 130, 70)
    one = _check(ext, "increase_visible", P, host=False)
    two = _check(ext, "increase_visible", dict(P, visible=one["visible"]), host=False)
    assert (two["visible"] - P["visible"]).tolist() == (2 * (one["visible"] - P["visible"])).tolist() and (one["visible"] != P["visible"]).any()
    assert (one["visible"] - P["visible"])[5] >= 5                  # point 5: twice in tracker 0, once in trackers 2 and 3; tracker 1 is gated
    D = K.decide_problem(9, 130, 70, mode=TR.LOCAL_MAP)
    one = _check(ext, "track_decide", D, host=False)
    two = _check(ext, "track_decide", dict(D, found=one["found"]), host=False)
    assert (two["found"] - D["found"]).tolist() == (2 * (one["found"] - D["found"])).tolist() and (one["found"] != D["found"]).any()


@pytest.mark.gpu
def test_gpu_decisions_on_every_threshold(ext, sweeps, expected):
    for name in ("decide0", "decide1"):
        _check(ext, "track_decide", sweeps[name], want=expected[(name, "track_decide")])
    made = _check(ext, "track_finish", sweeps["finish"], want=expected[("finish", "track_finish")])
    assert made == int((expected[("finish", "track_finish")]["new_kf"] >= 0).sum()) == 10


@pytest.mark.gpu
@pytest.mark.parametrize("ntrack,cap", [(1, 70), (3, 300), (130, 70)])
def test_gpu_random_decisions_equal_the_reference_in_both_forms(ext, ntrack, cap):
    for mode in (None, TR.MOTION_MODEL, TR.REFERENCE_KF, TR.LOCAL_MAP):
        _check(ext, "track_decide", K.decide_problem(ntrack + cap, ntrack, cap, mode=mode, after_retry=ntrack % 2))
    _check(ext, "track_finish", K.finish_random(ntrack, ntrack))


@pytest.mark.gpu
def test_gpu_decisions_at_16000_slots(ext):
    D = K.decide_problem(12, 3, 16000, counts=(16000, 257, 15999), npoints=5000)
    D["modes"][:] = [TR.LOCAL_MAP, TR.MOTION_MODEL, TR.LOCAL_MAP]
    D["run"][:] = 1
    _check(ext, "track_decide", D)
    F = K.finish_problem([dict(K.FINISH_DEFAULT, name="big", good=40, inl=30), dict(K.FINISH_DEFAULT, name="big_lost", ok=0)], cap=16000, live_n=16000)
    _check(ext, "track_finish", F)


def _tracker(P, t, keys, shared=()):
    """tracker t of a problem as a one-tracker problem over the same frames and table"""
    Q = dict(P)
    for k in keys:
        if P.get(k) is not None:
            Q[k] = np.array(P[k][t:t + 1])
    Q["ntrack"] = 1
    Q["frame"] = np.array([P["frame"][t] if P.get("frame") is not None else t], i32)
    return Q


@pytest.mark.gpu
def test_gpu_results_do_not_depend_on_batch_position_stream_or_repeat(ext, sweeps, expected):
    import torch
    P, e = sweeps["decide0"], expected[("decide0", "track_decide")]
    per = ("modes", "run", "nmatches", "nmatches_map", "pose_before", "kp_before", "pose_opt", "kp_opt", "outlier", "counters", "ok", "inliers", "retry",
           "pose_final", "kp_final")
    for t in (0, 9, 19, 33):
        rc, got = K.call_device(ext, "track_decide", _tracker(P, t, per))
        assert rc == 0 and all(got[k][0].tobytes() == e[k][t].tobytes() for k in ("ok", "inliers", "retry", "pose_final", "kp_final")), t
    F, e = sweeps["finish"], expected[("finish", "track_finish")]
    per = ("ok", "inliers", "counters", "pose_final", "kp_point", "outlier", "kp_out", "ref_kf_out", "new_kf", "interrupt_ba")
    for t in (0, 2, 8, 22):
        rc, got = K.call_device(ext, "track_finish", _tracker(F, t, per))
        assert rc == 0 and all(got[k][0].tobytes() == e[k][t].tobytes() for k in ("counters", "outlier", "kp_out", "ref_kf_out", "new_kf", "interrupt_ba")), t
        assert got["kf_point"][t].tobytes() == e["kf_point"][t].tobytes() and got["kf_id"][t] == e["kf_id"][t]
    side = torch.cuda.Stream()
    for prob, name in (("stats", "increase_visible"), ("stats", "query_seen_from_outliers"), ("decide0", "track_decide"), ("finish", "track_finish"),
                       ("median2", "scene_median_depth"), ("scale_accepted", "scale_initial_map")):
        want = expected[(prob, name)]
        for s in (side, None, side):
            rc, got = K.call_device(ext, name, sweeps[prob], s)
            assert rc == 0 and K.same(got, want), (name, K.diff(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("q", [1, 2])
def test_gpu_median_depth_equals_the_reference_in_both_forms(ext, sweeps, expected, q):
    """count 0 to 4, equal depths, two values straddling the chosen index, negative depths, -0.0 next to +0.0, a NaN, +-inf,
    denormals, every slot count, a list of 130 entries with -1 holes and repeats"""
    _check(ext, "scene_median_depth", sweeps["median%d" % q], want=expected[("median%d" % q, "scene_median_depth")])
    assert sweeps["median%d" % q]["nlist"] == 130


@pytest.mark.gpu
def test_gpu_median_of_16000_random_depths(ext):
    P = K.median_problem(2, big=16000)
    assert P["cap"] == 16000 and P["n"][-1] == 16000
    want = K.expect("scene_median_depth", P)
    d = np.sort(np.array([TR.depth_of(P["poses"][-1]["Tcw"], P["points"][p]["pos"]) for p in P["kf_point"][-1]], f32))
    at = list(P["kf_list"]).index(P["nframes"] - 1)
    assert want["median"][at] == d[(16000 - 1) // 2] and d[7999] != d[8000]
    _check(ext, "scene_median_depth", P, want=want)
    _check(ext, "scene_median_depth", dict(P, q=1), host=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["accepted", "negative_median", "few_tracked", "empty"])
def test_gpu_initial_map_scale_equals_the_reference_in_both_forms(ext, sweeps, expected, kind):
    want = expected[("scale_" + kind, "scale_initial_map")]
    rc = _check(ext, "scale_initial_map", sweeps["scale_" + kind], want=want)
    assert rc == (105 if kind == "accepted" else 0)


@pytest.mark.gpu
def test_gpu_python_mirrors_return_what_the_reference_leaves(ext, sweeps):
    import pilotguru_amd as pg
    calls = _mirror_calls(pg, ext)
    P = K.clean(sweeps["stats"])
    assert calls["check_replaced"](P).tobytes() == K.expect("check_replaced", P)["last_point"].tobytes()
    assert calls["increase_visible"](P).tobytes() == K.expect("increase_visible", P)["visible"].tobytes()
    seen = K.expect("query_seen_from_outliers", dict(P, query_seen=np.zeros_like(P["query_seen"])))["query_seen"]
    assert calls["query_seen_from_outliers"](P).tobytes() == seen.tobytes()
    P = K.clean(sweeps["decide0"])
    r, e = calls["track_decide"](P), K.expect("track_decide", P)
    assert r["ok"].tolist() == e["ok"].tolist() and r["found"].tolist() == e["found"].tolist()
    live = P["run"] != 0
    assert r["pose_final"][live].tobytes() == e["pose_final"][live].tobytes() and r["kp_point_final"][live, :64].tolist() == e["kp_final"][live, :64].tolist()
    P = K.clean(sweeps["finish"])
    r, e = calls["track_finish"](P), K.expect("track_finish", P)
    for a, b in (("counters", "counters"), ("outlier", "outlier"), ("kf_point", "kf_point"), ("kf_pose", "kf_pose"), ("kf_id", "kf_id"), ("ref_kf", "ref_kf_out"),
                 ("new_kf", "new_kf"), ("interrupt_ba", "interrupt_ba")):
        assert r[a].tobytes() == e[b].tobytes(), a
    assert r["kp_point_out"][:, :64].tolist() == e["kp_out"][:, :64].tolist() and r["made"] == 10
    P = K.clean(sweeps["median2"])
    med, st = calls["scene_median_depth"](P)
    e = K.expect("scene_median_depth", dict(P, median=np.zeros(P["nlist"], f32), status=np.zeros(P["nlist"], i32)))
    assert med.tobytes() == e["median"].tobytes() and st.tolist() == e["status"].tolist()
    P = K.clean(sweeps["scale_accepted"])
    r, e = calls["scale_initial_map"](P), K.expect("scale_initial_map", P)
    assert r["poses"].tobytes() == e["poses"].tobytes() and r["points"].tobytes() == e["points"].tobytes() and r["info"].tolist() == e["info"].tolist()
    assert not r["wrong"] and f32(r["median"]) == e["info"][1:2].view(f32)[0]


@pytest.mark.gpu
def test_gpu_checked_forms_refuse_malformed_input_and_limits(ext, sweeps):
    from pilotguru_amd import _lib
    import torch
    for name, prob in PROBLEM_OF.items():
        P = K.clean(sweeps[prob])
        for what, Q in _malformed(name, P):
            assert K.call_host(ext, name, Q)[0] == _lib.PGORB_E_ARG, (name, what)
        for k in [k for kind, k in K.spec(name) if kind == "int" and k not in ("mode", "after_retry", "kf_ini", "kf_cur", "q")]:
            assert K.call_host(ext, name, dict(P, **{k: -1}))[0] == _lib.PGORB_E_ARG, (name, k)
        first = next(k for kind, k in K.spec(name) if kind == "io")
        assert K.call_host(ext, name, dict(P, **{first: None}))[0] == _lib.PGORB_E_ARG, (name, first)
    # the limits: nothing is launched, so one small buffer stands for every array
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    hb = np.zeros(4096, u8)
    for name in K.SPECS:
        for what, over in (("cap", 16001), ("nframes", 4097), ("ntrack", 4097), ("nlist", TR.DEPTH_MAX_LIST + 1), ("qcap", 16001)):
            if what not in [k for _, k in K.spec(name)]:
                continue
            args = [(over if k == what else 1) if kind == "int" else C.c_void_p(d.data_ptr()) for kind, k in K.spec(name)]
            dev = "pgorb_scale_initial_map_device" if name == "scale_initial_map" else "pgorb_%s_batch_device" % name
            assert getattr(ext._L, dev)(ext._h, *args, None) == _lib.PGORB_E_LIMIT, (name, what)
            args = [(over if k == what else 1) if kind == "int" else K._p(hb) for kind, k in K.spec(name)]
            assert getattr(ext._L, "pgorb_" + name)(ext._h, *args) == _lib.PGORB_E_LIMIT, (name, what)


@pytest.mark.gpu
def test_gpu_median_list_feeds_create_new_map_points(ext):
    """the flat d_neigh of pgorb_create_new_map_points_batch_device (-1 past each problem's neighbours) as the list, q = 2, and the
    output array passed on as d_median_depth without leaving the device: the points equal those of the same call fed the medians
    that the restatement computes on the host"""
    import mapping_cases as MC
    problems, tables = K.cnm_problems(MC)
    host = MC.run_gpu_batched([(KF1, [dict(N, median=m) for N, m in zip(neigh, med)]) for (KF1, neigh), (_, med) in zip(problems, tables["medians"])],
                              ext, M=tables["M"])
    dev = K.run_cnm_with_device_medians(MC, problems, tables, ext)
    assert sum(len(h[0]) for h in host) > 50
    for h, g in zip(host, dev):
        assert MC.same_point_lists(h[0], g[0]) and list(h[1]) == list(g[1])
    assert sum(c == -1 for h in host for c in h[1]) > 0             # a small median skips a neighbour on both paths (the baseline test)


def _local_map_of_a_flat_graph(kp_point, kf_point, n, bad, obs_start, obs_frame):
    """Tracking::UpdateLocalMap (Tracking.cc:1186-1321) where no key frame has a neighbour, a child or a parent: the slots with the bad
    points cleared, the voted key frames in index order, the first strict maximum as reference, and UpdateLocalPoints over them"""
    slots = np.array(kp_point, i32)
    votes = {}
    for i, p in enumerate(slots):
        if p >= 0:
            if bad[p]:
                slots[i] = -1
            else:
                for k in obs_frame[obs_start[p]:obs_start[p + 1]]:
                    votes[int(k)] = votes.get(int(k), 0) + 1
    local = sorted(votes)
    ref = max(local, key=lambda k: (votes[k], -k)) if local else -1
    q = []
    for k in local:
        for p in kf_point[k][:n[k]]:
            if p >= 0 and not bad[p] and int(p) not in q:
                q.append(int(p))
    return slots, local, ref, q


@pytest.mark.gpu
def test_gpu_one_chained_frame_three_times_on_a_resident_batch(ext):
    """check_replaced -> predict -> SearchByProjection(last frame) -> slots -> PoseOptimization (discarding) -> decide -> UpdateLocalMap
    -> query_seen (from the slots the discard emptied) -> SearchLocalPoints -> increase_visible -> slots -> PoseOptimization -> decide
    (local map) -> finish -> commit, for three consecutive frames (frames 0, 3 and 4 of one resident batch; reference-KF mode, then the
    motion model twice) on one stream with NO host read in between: every call reads what the call before it wrote, where it lies; the
    only host writes are the frame's id, time and mode.  Afterwards every stage is held against its restatement fed with what the stage
    before it produced: the two pose optimisations within the bounds of tests/pose_cases.py, everything else byte for byte -- visible,
    found, the slots, d_ok, the key-frame row and the trajectory records among them.  The map is the scene of tests/test_track_pose.py's
    chain: the last frame is key frame 1, an empty key frame 2 observes every point too (so that TrackedMapPoints(2) counts them)."""
    import torch
    import pose_cases as PC
    import tracking_cases as TKC
    import tracking_reference as TKR
    import track_pose_cases as TPK
    import track_pose_reference as TPR
    import test_track_pose as TP
    from pilotguru_amd.orb import KEYPOINT_DTYPE
    c, state, _ = TP._chain_scene()
    b = TKC.as_batch(c)
    (fcur, fother, _), = b.pairs
    cur, oth = b.frames[fcur], b.frames[fother]
    CUR, OTH, KF2, nf, cap = (0, 3, 4), 1, 2, 5, b.qcap
    n_arr = np.array([len(cur[0]), len(oth[0]), 0, len(cur[0]), len(cur[0])], i32)
    ncur = len(cur[0])
    kp, ds = np.zeros((nf, cap), KEYPOINT_DTYPE), np.zeros((nf, cap, 32), u8)
    for f in CUR:
        kp[f, :ncur], ds[f, :ncur] = cur[0], cur[1]
    kp[OTH, :len(oth[0])], ds[OTH, :len(oth[0])] = oth[0], oth[1]
    pts, pd, bad, obs = TKC.table_arrays(b.points)
    npts, qcap = len(pts), len(pts)
    state = np.array(state)
    state[0]["last_ref_kf"] = OTH
    kf0 = np.zeros(nf, TR.KF_POSE_DTYPE)
    kf0[:] = c.pose
    kfp0 = np.full((nf, cap), -1, i32)
    kfp0[OTH, :len(c.other_point)] = c.other_point
    start, of = [0], []
    for pnt in range(npts):
        of += ([OTH] if pnt in set(c.other_point.tolist()) else []) + [KF2]
        start.append(len(of))
    start, of = np.array(start, i32), np.array(of, i32)
    rep0 = np.full(npts, -1, i32)
    first = int(c.other_point[c.other_point >= 0][0])
    rep0[first] = first                                              # a replacement that names the point itself: wired, and harmless
    ct0 = K.counters_of(1)
    ct0[0]["max_frames"], ct0[0]["nkfs"], ct0[0]["ref_kf"], ct0[0]["next_kf_id"], ct0[0]["accept_keyframes"], ct0[0]["set_not_stop_ok"] = 30, 2, OTH, 2, 1, 1
    vis0, fnd0 = np.arange(npts).astype(i32) * 3, np.arange(npts).astype(i32) * 5
    L, h = ext._L, ext._h
    keep = []

    def p(t):
        if t is None:
            return None
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    dev = lambda a: torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), u8).copy()).cuda()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dk, dd, dn = dev(kp), dev(ds), dev(n_arr)
    gs = torch.empty((nf, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    gi = torch.empty((nf, cap), dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_frame_grid_batch_device(h, p(dk), p(dn), nf, cap, *TKC.BOUNDS, p(gs), p(gi), s))
    dpts, dpd, dbad, dobs, dst, dof, drep = dev(pts), dev(pd), dev(bad), dev(obs), dev(start), dev(of), dev(rep0)

    def row(a, dtype, fill=0):
        x = np.full((1, cap), fill, dtype)
        x[0, :len(a)] = a
        return dev(x)
    op, flag, has = row(c.other_point, i32, -1), row(c.flag, u8), row(c.has, u8)
    po = dev(np.array([OTH], i32))
    dord, dnord, dpar = dev(np.full((nf, 4), -1, i32)), dev(np.zeros(nf, i32)), dev(np.full(nf, -1, i32))
    dkfp, dkf, dkid = dev(kfp0), dev(kf0), dev(np.arange(nf).astype(np.uint64))
    S, T, N = TPK._up(state), TPK._sent(4 * 72), TPK._up(np.zeros(1, i32))
    cnt = torch.from_numpy(np.frombuffer(ct0.tobytes(), np.int64).copy()).cuda()
    vis, fnd = dev(vis0).view(torch.int32), dev(fnd0).view(torch.int32)
    SB = lambda nbytes: TPK._sent(nbytes)
    frames = []
    for f, mode in enumerate(TP.CHAIN_MODES):
        cnt[0] = 100 + f                                             # mCurrentFrame.mnId: a host write, no read
        pf = dev(np.array([CUR[f]], i32))
        F = dict(pf=pf, pred=SB(84), ps=SB(4), asg=SB(cap * 4), nm=SB(4), kpp=dev(np.full((1, cap), -1, i32)), pose1=SB(84), outl1=SB(cap), kpo1=SB(cap * 4),
                 nmap1=SB(4), info1=SB(32), ninl1=SB(4), chi1=SB(cap * 4), ok1=SB(1), inl1=SB(4), retry=SB(1), posef1=SB(84), kpf1=SB(cap * 4),
                 ulm=SB(cap * 4), lkf=SB(8 * 4), nlkf=SB(4), refkf=SB(4), q=SB(qcap * 4), nq=SB(4), ustat=SB(4), seen=SB(qcap), inview=SB(qcap),
                 px=SB(qcap * 4), py=SB(qcap * 4), lv=SB(qcap * 4), vc=SB(qcap * 4), slp=SB(cap * 4), ntm=SB(4), asg2=SB(cap * 4), nm2=SB(4),
                 pose2=SB(84), outl2=SB(cap), kpo2=SB(cap * 4), nmap2=SB(4), info2=SB(32), ninl2=SB(4), chi2=SB(cap * 4), ok2=SB(1), inl2=SB(4),
                 retry2=SB(1), posef2=SB(84), kpf2=SB(cap * 4), kpout=SB(cap * 4), refout=SB(4), newkf=SB(4), intba=SB(1), cs=SB(4),
                 tm=TPK._up(np.array([10.0 + f / 30.0], f64)), ids=TPK._up(np.array([f], np.int64)))
        ck = ext._check
        ck(L.pgorb_check_replaced_batch_device(h, 1, p(dn), nf, cap, p(po), p(op), npts, p(drep), s))
        F["op"] = op.clone()
        ck(L.pgorb_track_predict_batch_device(h, 1, mode, None, p(S), p(T), 4, p(N), nf, p(dkf), p(F["pred"]), p(F["ps"]), s))
        ck(L.pgorb_search_by_projection_last_frame_batch_device(
            h, p(dk), p(dd), p(dn), cap, p(gs), p(gi), p(pf), p(po), 1, *TKC.BOUNDS, p(F["pred"]), p(has), p(op), p(flag), npts, p(dpts), p(dpd), p(dobs),
            c.th, int(c.ori), None, None, None, p(F["asg"]), p(F["nm"]), s))
        ck(L.pgorb_slots_from_assignment_batch_device(h, p(F["asg"]), p(op), cap, p(F["kpp"]), cap, 1, s))
        # one wrong match, made on the device: the first matched slot takes the point of the last one, so that the optimisation has an
        # outlier to discard (the scene itself is clean)
        kv = F["kpp"].view(torch.int32)
        held = (kv >= 0).int()
        j, j2 = torch.argmax(held), cap - 1 - torch.argmax(torch.flip(held, [0]))
        kv.index_copy_(0, j.view(1), kv[j2].view(1).clone())
        ck(L.pgorb_pose_optimization_batch_device(h, p(dk), p(dn), cap, p(pf), 1, p(F["pred"]), p(F["kpp"]), npts, p(dpts), p(dobs), 1, p(F["pose1"]),
                                                  p(F["outl1"]), p(F["kpo1"]), p(F["nmap1"]), p(F["chi1"]), p(F["info1"]), p(F["ninl1"]), s))
        F["fnd_a"], F["cnt_a"] = fnd.clone(), cnt.clone()
        ck(L.pgorb_track_decide_batch_device(h, 1, mode, None, 0, p(dn), nf, cap, p(pf), None, p(F["nm"]), p(F["nmap1"]), p(F["pred"]), p(F["kpp"]),
                                             p(F["pose1"]), p(F["kpo1"]), p(F["outl1"]), npts, p(dobs), p(fnd), p(cnt), p(F["ok1"]), p(F["inl1"]),
                                             p(F["retry"]), p(F["posef1"]), p(F["kpf1"]), s))
        F["kfp_a"] = dkfp.clone()
        ck(L.pgorb_update_local_map_batch_device(h, p(dkfp), p(dn), nf, cap, None, p(pf), 1, p(F["kpf1"]), npts, p(dbad), p(dst), p(dof), len(of), 4, p(dord),
                                                 p(dnord), p(dpar), None, 10, 80, 8, None, None, p(F["ulm"]), p(F["lkf"]), p(F["nlkf"]), p(F["refkf"]),
                                                 qcap, p(F["q"]), p(F["nq"]), p(F["ustat"]), s))
        ck(L.pgorb_query_seen_from_outliers_batch_device(h, 1, p(dn), nf, cap, p(pf), p(F["kpp"]), p(F["outl1"]), p(F["kpo1"]), qcap, p(F["nq"]), p(F["q"]),
                                                         npts, p(F["seen"]), s))
        ck(L.pgorb_search_local_points_batch_device(
            h, p(dk), p(dd), p(dn), cap, p(gs), p(gi), p(pf), 1, *TKC.BOUNDS, p(F["posef1"]), p(F["ulm"]), npts, p(dpts), p(dpd), p(dbad), p(dobs), qcap,
            p(F["nq"]), p(F["q"]), p(F["seen"]), 0.5, 1.0, 0.8, p(F["inview"]), p(F["px"]), p(F["py"]), p(F["lv"]), p(F["vc"]), p(F["slp"]), p(F["ntm"]),
            p(F["asg2"]), p(F["nm2"]), s))
        F["vis_a"] = vis.clone()
        ck(L.pgorb_increase_visible_batch_device(h, 1, p(dn), nf, cap, p(pf), p(F["ok1"]), p(F["slp"]), qcap, p(F["nq"]), p(F["q"]), p(F["inview"]), npts,
                                                 p(vis), s))
        F["vis_b"] = vis.clone()
        F["kpp2"] = F["slp"].clone()
        ck(L.pgorb_slots_from_assignment_batch_device(h, p(F["asg2"]), p(F["q"]), qcap, p(F["kpp2"]), cap, 1, s))
        ck(L.pgorb_pose_optimization_batch_device(h, p(dk), p(dn), cap, p(pf), 1, p(F["posef1"]), p(F["kpp2"]), npts, p(dpts), p(dobs), 0, p(F["pose2"]),
                                                  p(F["outl2"]), p(F["kpo2"]), p(F["nmap2"]), p(F["chi2"]), p(F["info2"]), p(F["ninl2"]), s))
        F["outl2_a"] = F["outl2"].clone()
        ck(L.pgorb_track_decide_batch_device(h, 1, TR.LOCAL_MAP, None, 0, p(dn), nf, cap, p(pf), p(F["ok1"]), p(F["nm2"]), p(F["nmap2"]), p(F["posef1"]),
                                             p(F["kpp2"]), p(F["pose2"]), p(F["kpo2"]), p(F["outl2"]), npts, p(dobs), p(fnd), p(cnt), p(F["ok2"]), p(F["inl2"]),
                                             p(F["retry2"]), p(F["posef2"]), p(F["kpf2"]), s))
        F["fnd_b"], F["kf_a"], F["kid_a"] = fnd.clone(), dkf.clone(), dkid.clone()
        ck(L.pgorb_track_finish_batch_device(h, 1, p(dn), nf, cap, p(pf), p(F["ok2"]), p(F["inl2"]), p(cnt), p(F["posef2"]), p(F["kpf2"]), p(F["outl2"]), npts,
                                             p(dbad), p(dobs), p(dst), p(dof), len(of), None, p(dkfp), p(dkf), p(dkid), p(F["kpout"]), p(F["refout"]),
                                             p(F["newkf"]), p(F["intba"]), s))
        F["cnt_b"], F["kfp_b"], F["kf_b"], F["kid_b"], F["state_mid"] = cnt.clone(), dkfp.clone(), dkf.clone(), dkid.clone(), S.clone()
        ck(L.pgorb_track_commit_batch_device(h, 1, p(S), p(F["posef2"]), p(F["ok2"]), p(F["refout"]), p(F["tm"]), p(F["ids"]), nf, p(dkf), p(T), 4, p(N),
                                             p(F["cs"]), s))
        F["state"], F["traj"], F["count"] = S.clone(), T.clone(), N.clone()
        frames.append(F)
    torch.cuda.synchronize()                                             # the first download
    A = lambda t, dt, *shape: np.frombuffer(t.cpu().numpy().tobytes(), dt).reshape(*shape) if shape else np.frombuffer(t.cpu().numpy().tobytes(), dt)
    _, mps = c.build()
    trk = TPR.Tracker(state[0], cap=4)
    fill = np.frombuffer(bytes([TPK.SENT]) * (4 * 72), TPK.TRAJECTORY_RECORD_DTYPE)
    I = lambda t: A(t, i32)
    one = dict(ntrack=1, nframes=nf, cap=cap, n=n_arr, npoints=npts)
    kf_made = 0
    for f, (mode, F) in enumerate(zip(TP.CHAIN_MODES, frames)):
        w = "frame %d: " % f
        fr1 = np.array([CUR[f]], i32)
        kf_tab = A(F["kf_a"] if f == 0 else frames[f - 1]["kf_b"], TR.KF_POSE_DTYPE)
        assert I(F["op"]).tolist() == TR.check_replaced(row_h(c.other_point, cap), n_arr, np.array([OTH], i32), npts, rep0).reshape(-1).tolist(), w + "check_replaced"
        pred, status = TPR.predict(trk, mode, kf_tab)
        assert [status] == I(F["ps"]).tolist() == [0] and A(F["pred"], u8).tobytes() == pred.tobytes(), w + "the prediction"
        fr = TKR.Frame(1, c.keys, c.desc, TKC.BOUNDS, pred, TKC.SF, TKC.log_sf(), TKC.NLEVELS)
        r1 = TKR.search_by_projection_last_frame(fr, c.other_keys, [None if x < 0 else mps[x] for x in c.other_point], c.flag, c.has, c.th, c.ori)
        assert int(I(F["nm"])[0]) == r1["nmatches"] and np.array_equal(I(F["asg"])[:ncur], r1["assigned"]), w + "the search"
        kpp = np.where(r1["assigned"] >= 0, c.other_point[np.maximum(r1["assigned"], 0)], -1).astype(i32)
        at = np.flatnonzero(kpp >= 0)
        assert len(at) >= 20 and kpp[at[0]] != kpp[at[-1]]
        kpp[at[0]] = kpp[at[-1]]                                       # the wrong match made on the device
        assert np.array_equal(I(F["kpp"])[:ncur], kpp) and (I(F["kpp"])[ncur:] == -1).all(), w + "the slots"
        xy, P3 = np.stack([c.keys["x"], c.keys["y"]], 1), np.array([q["pos"] for q in c.points], f32)
        pc = PC.Case("chain1_%d" % f, xy, c.keys["octave"], pred, kpp, P3, obs)
        pose1 = A(F["pose1"], TR.KF_POSE_DTYPE)[0]
        got = PC.result_of(pose1, A(F["outl1"], u8)[:ncur], I(F["kpo1"])[:ncur], I(F["nmap1"])[0], A(F["chi1"], f32)[:ncur], I(F["info1"]), I(F["ninl1"])[0])
        d = PC.differences(pc, PC.run_reference(pc, discard=True), got, PC.spread(pc))
        assert not d, w + "the first pose optimisation differs from the reference: %s" % d
        assert not A(F["outl1"], u8)[:ncur].any() and (I(F["kpo1"])[:ncur] != kpp).any(), w + "the discard emptied slots and cleared their flags"
        # the first decision, from what the device's stages left
        D = dict(one, mode=mode, modes=None, after_retry=0, frame=fr1, run=None, nmatches=I(F["nm"]), nmatches_map=I(F["nmap1"]),
                 pose_before=A(F["pred"], TR.KF_POSE_DTYPE), kp_before=I(F["kpp"]).reshape(1, cap), pose_opt=A(F["pose1"], TR.KF_POSE_DTYPE),
                 kp_opt=I(F["kpo1"]).reshape(1, cap), outlier=A(F["outl1"], u8).reshape(1, cap), has_obs=obs, found=I(F["fnd_a"]),
                 counters=A(F["cnt_a"], TR.COUNTERS_DTYPE), **K.decide_outputs(1, cap))
        e = K.expect("track_decide", D)
        g1 = dict(found=I(F["fnd_a"]), ok=A(F["ok1"], u8), inliers=I(F["inl1"]), retry=A(F["retry"], u8), pose_final=A(F["posef1"], TR.KF_POSE_DTYPE),
                  kp_final=I(F["kpf1"]).reshape(1, cap))
        assert K.same(g1, e) and g1["ok"][0] == 1, w + "the first decision: %s" % K.diff(g1, e)
        # UpdateLocalMap over the flat graph, then query_seen from the slots the discard emptied
        slots, local, ref, q = _local_map_of_a_flat_graph(g1["kp_final"][0, :ncur], A(F["kfp_a"], i32, nf, cap), n_arr, bad, start, of)
        nq = I(F["nq"])[0]
        assert I(F["ulm"])[:ncur].tolist() == slots.tolist() and I(F["lkf"])[:I(F["nlkf"])[0]].tolist() == local and I(F["refkf"])[0] == ref, w + "UpdateLocalMap"
        assert I(F["q"])[:nq].tolist() == q and nq > 20 and I(F["ustat"])[0] == 0, w + "the local points"
        Q = dict(one, frame=fr1, kp_before=D["kp_before"], outlier=D["outlier"], kp_after=D["kp_opt"], qcap=qcap, nq=I(F["nq"]), queries=I(F["q"]).reshape(1, qcap),
                 query_seen=K.sent((1, qcap), u8))
        e = K.expect("query_seen_from_outliers", Q)["query_seen"]
        seen = A(F["seen"], u8).reshape(1, qcap)
        assert seen.tobytes() == e.tobytes() and seen[0, :nq].sum() == (D["kp_opt"][0, :ncur] != kpp).sum() > 0, w + "query_seen"
        # SearchLocalPoints
        fr = TKR.Frame(1, c.keys, c.desc, TKC.BOUNDS, g1["pose_final"][0], TKC.SF, TKC.log_sf(), TKC.NLEVELS)
        fr.slots = [None if x < 0 else mps[x] for x in g1["kp_final"][0, :ncur]]
        r2 = TKR.search_local_points(fr, [mps[x] for x in q], seen[0, :nq], 1.0, 0.8, 0.5)
        g2 = dict(nmatches=I(F["nm2"])[0], assigned=I(F["asg2"])[:ncur], in_view=A(F["inview"], u8)[:nq], level=I(F["lv"])[:nq], kp_point_out=I(F["slp"])[:ncur],
                  n_to_match=I(F["ntm"])[0], proj_x=A(F["px"], f32)[:nq], proj_y=A(F["py"], f32)[:nq], view_cos=A(F["vc"], f32)[:nq])
        assert not TKC.differences("local", r2, g2), w + "SearchLocalPoints: %s" % TKC.differences("local", r2, g2)
        assert not g2["in_view"][seen[0, :nq] != 0].any(), w + "a discarded point is not projected again"
        V = dict(one, frame=fr1, run=g1["ok"], kp_point=I(F["slp"]).reshape(1, cap), qcap=qcap, nq=I(F["nq"]), queries=Q["queries"],
                 in_view=A(F["inview"], u8).reshape(1, qcap), visible=I(F["vis_a"]))
        assert I(F["vis_b"]).tolist() == K.expect("increase_visible", V)["visible"].tolist() and (I(F["vis_b"]) != I(F["vis_a"])).any(), w + "visible"
        kpp2 = np.where(r2["assigned"] >= 0, np.array(q, i32)[np.maximum(r2["assigned"], 0)], r2["kp_point_out"]).astype(i32)
        assert np.array_equal(I(F["kpp2"])[:ncur], kpp2), w + "the slots of the local map"
        pc = PC.Case("chain2_%d" % f, xy, c.keys["octave"], g1["pose_final"][0], kpp2, P3, obs)
        pose2 = A(F["pose2"], TR.KF_POSE_DTYPE)[0]
        got = PC.result_of(pose2, A(F["outl2_a"], u8)[:ncur], I(F["kpo2"])[:ncur], I(F["nmap2"])[0], A(F["chi2"], f32)[:ncur], I(F["info2"]), I(F["ninl2"])[0])
        d = PC.differences(pc, PC.run_reference(pc, discard=False), got, PC.spread(pc))
        assert not d, w + "the second pose optimisation differs from the reference: %s" % d
        D = dict(one, mode=TR.LOCAL_MAP, modes=None, after_retry=0, frame=fr1, run=g1["ok"], nmatches=I(F["nm2"]), nmatches_map=I(F["nmap2"]),
                 pose_before=g1["pose_final"], kp_before=I(F["kpp2"]).reshape(1, cap), pose_opt=A(F["pose2"], TR.KF_POSE_DTYPE),
                 kp_opt=I(F["kpo2"]).reshape(1, cap), outlier=A(F["outl2_a"], u8).reshape(1, cap), has_obs=obs, found=I(F["fnd_a"]),
                 counters=A(F["cnt_a"], TR.COUNTERS_DTYPE), **K.decide_outputs(1, cap))
        e = K.expect("track_decide", D)
        g3 = dict(found=I(F["fnd_b"]), ok=A(F["ok2"], u8), inliers=I(F["inl2"]), retry=A(F["retry2"], u8), pose_final=A(F["posef2"], TR.KF_POSE_DTYPE),
                  kp_final=I(F["kpf2"]).reshape(1, cap))
        assert K.same(g3, e) and (g3["found"] != D["found"]).any(), w + "the local-map decision: %s" % K.diff(g3, e)
        X = dict(one, frame=fr1, ok=g3["ok"], inliers=g3["inliers"], counters=D["counters"], pose_final=g3["pose_final"], kp_point=g3["kp_final"],
                 outlier=D["outlier"], point_bad=bad, has_obs=obs, obs_start=start, obs_frame=of, nobs=len(of), obs_live=None, kf_point=A(F["kfp_a"], i32, nf, cap),
                 kf_pose=A(F["kf_a"], TR.KF_POSE_DTYPE), kf_id=A(F["kid_a"], np.uint64), kp_out=K.sent((1, cap), i32), ref_kf_out=K.sent(1, i32),
                 new_kf=K.sent(1, i32), interrupt_ba=K.sent(1, u8))
        e = K.expect("track_finish", X)
        g4 = dict(counters=A(F["cnt_b"], TR.COUNTERS_DTYPE), outlier=A(F["outl2"], u8).reshape(1, cap), kf_point=A(F["kfp_b"], i32, nf, cap),
                  kf_pose=A(F["kf_b"], TR.KF_POSE_DTYPE), kf_id=A(F["kid_b"], np.uint64), kp_out=I(F["kpout"]).reshape(1, cap), ref_kf_out=I(F["refout"]),
                  new_kf=I(F["newkf"]), interrupt_ba=A(F["intba"], u8))
        assert K.same(g4, e), w + "the tail of Track(): %s" % K.diff(g4, e)
        kf_made += int(g4["new_kf"][0] >= 0)
        print(w + "nmatches %d, map %d; local map: %d queries, %d seen, %d matches, inliers %d, ok %d; new key frame %d" % (
            r1["nmatches"], I(F["nmap1"])[0], nq, seen[0, :nq].sum(), r2["nmatches"], g3["inliers"][0], g3["ok"][0], g4["new_kf"][0]))
        assert A(F["state_mid"], u8).tobytes() == trk.state().tobytes(), w + "the state before the commit"
        assert TPR.commit(trk, g3["pose_final"][0], int(g3["ok"][0]), int(g4["ref_kf_out"][0]), 10.0 + f / 30.0, f, g4["kf_pose"], 4) == 0 and I(F["cs"]).tolist() == [0]
        assert A(F["state"], u8).tobytes() == trk.state().tobytes() and A(F["traj"], u8).tobytes() == trk.records(4, fill).tobytes(), w + "the commit"
        assert I(F["count"]).tolist() == [f + 1]
    assert trk.has_velocity and kf_made == 1                         # frame 0 becomes a key frame; against it c2 fails for the next two


def row_h(a, cap):
    x = np.full((1, cap), -1, i32)
    x[0, :len(a)] = a
    return x
