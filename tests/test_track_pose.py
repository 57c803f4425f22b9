"""The trajectory read-out on the GPU (pilotguru_amd/csrc/track_pose.hip; include/pgorb.h: Tracking's pose record, Tracking.cc:792-798,
:866, :764, :432-440, :493, :497-506; KeyFrame::SetBadFlag's mTcp, KeyFrame.cc:641; System::GetTrajectory, System.cc:371-412) against
the numpy restatement of those lines (tests/track_pose_reference.py) on the constructed cases, the predict / commit sequences, the
mTcp list, seeded random worlds and one large case (tests/track_pose_cases.py).  The library is built with -ffp-contract=off and
these paths use + - x / and correctly rounded square roots only, so every GPU comparison is byte for byte, untouched bytes included
(the outputs start as a sentinel).

The CPU tests check presence and record layouts (they fail without the feature), every named mutant of the restatement on the case
constructed for it, expectations written out by hand, the restatement's two forms (and its batched form) against each other, an
independent float64 anchor with a bound computed from each case, what the random worlds cover, the refusals of the Python and C++
mirrors without a device, and System.write_poses through the built optical_trajectories --poses_in."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_pose_cases as K  # noqa: E402
import track_pose_reference as TR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pilotguru_amd", "host", "optical_trajectories")
NAMES = ("pgorb_track_predict", "pgorb_track_predict_batch_device", "pgorb_track_commit", "pgorb_track_commit_batch_device",
         "pgorb_keyframe_tcp", "pgorb_keyframe_tcp_device", "pgorb_get_trajectory", "pgorb_get_trajectory_device")
f32, f64 = np.float32, np.float64


def by_name(cases, name):
    return next(c for c in cases if c["name"] == name)


@pytest.fixture(scope="module")
def trajs():
    """(case, what the reference leaves), computed once"""
    return [(c, TR.get_trajectory(c)) for c in K.trajectory_cases()]


@pytest.fixture(scope="module")
def worlds():
    out = []
    for n in K.WORLD_RECORDS:
        for nkf in K.WORLD_KFS:
            c = K.random_world(0, n, nkf)
            hits = {}
            out.append((c, TR.get_trajectory(c, hits=hits), hits))
    return out


@pytest.fixture(scope="module")
def large():
    c = K.large_world()
    return c, TR.get_trajectory_batched(c)


@pytest.fixture(scope="module")
def sequences():
    return K.run_sequences_reference()


# ---------------------------------------------------------------- CPU
C_LAYOUT = r"""
#include "include/pgorb.h"
#include <stddef.h>
#include <stdio.h>
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
int main(void)
{
    printf("pgorb_kf_pose %zu\npgorb_track_state %zu\npgorb_trajectory_record %zu\n", sizeof(pgorb_kf_pose), sizeof(pgorb_track_state),
           sizeof(pgorb_trajectory_record));
    F(pgorb_track_state, last); F(pgorb_track_state, velocity); F(pgorb_track_state, last_ref_kf); F(pgorb_track_state, has_last);
    F(pgorb_track_state, has_velocity); F(pgorb_track_state, pad);
    F(pgorb_trajectory_record, pose); F(pgorb_trajectory_record, ref_kf); F(pgorb_trajectory_record, has_pose); F(pgorb_trajectory_record, lost);
    F(pgorb_trajectory_record, pad); F(pgorb_trajectory_record, frame_time); F(pgorb_trajectory_record, frame_id);
    return 0;
}
"""


def test_symbols_constants_mirrors_and_null_context():
    from pilotguru_amd import _lib
    import pilotguru_amd as pg
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name)
    p = None
    assert L.pgorb_track_predict(p, 0, p, p, 0, p, p) == -1
    assert L.pgorb_track_predict_batch_device(p, 0, 0, p, p, p, 0, p, 0, p, p, p, p) == -1
    assert L.pgorb_track_commit(p, p, p, 0, 0, 0.0, 0, 0, p, p, 0, p) == -1
    assert L.pgorb_track_commit_batch_device(p, 0, *([p] * 6), 0, p, p, 0, p, p, p) == -1
    assert L.pgorb_keyframe_tcp(p, 0, p, p, 0, p, p, p) == -1
    assert L.pgorb_keyframe_tcp_device(p, 0, p, p, 0, p, p, p, p, p) == -1
    assert L.pgorb_get_trajectory(p, 0, *([p] * 5), 0, *([p] * 8)) == -1
    assert L.pgorb_get_trajectory_device(p, 0, *([p] * 5), 0, *([p] * 10)) == -1
    hdr = open(os.path.join(ROOT, "include", "pgorb.h")).read()
    defs = dict(re.findall(r"#define\s+PGORB_((?:TRACK|TRAJ|TCP)_\w+)\s+(\(1 << 22\)|\d+)", hdr))
    assert len(defs) == 13
    for k, v in defs.items():
        v = 1 << 22 if "<<" in v else int(v)
        assert getattr(pg, k) == v and getattr(_lib, "PGORB_" + k) == v, k
    assert (pg.TRACK_MOTION_MODEL, pg.TRACK_REFERENCE_KF, pg.TRACK_NO_LAST, pg.TRACK_NO_VELOCITY, pg.TRACK_BAD_INDEX, pg.TRACK_FULL) == \
        (TR.MOTION_MODEL, TR.REFERENCE_KF, TR.NO_LAST, TR.NO_VELOCITY, TR.BAD_INDEX, TR.FULL)
    assert (pg.TRAJ_BROKEN, pg.TRAJ_BAD_TIME, pg.TRAJ_NO_ORIGIN, pg.TRAJ_INFO, pg.TCP_INFO) == (TR.BROKEN, TR.BAD_TIME, TR.NO_ORIGIN, TR.TRAJ_INFO, TR.TCP_INFO)
    assert (pg.CULL_KF_CULLED, pg.CULL_LIMIT) == (TR.CULLED, TR.CULL_LIMIT)
    for cls, fn in ((pg.Tracking, "PredictPose"), (pg.Tracking, "CommitFrame"), (pg.LocalMapping, "KeyFrameTcp"), (pg.System, "GetTrajectory"),
                    (pg.System, "write_poses")):
        assert callable(getattr(cls, fn))
    hpp = open(os.path.join(ROOT, "pilotguru_amd", "host", "orb_extractor.hpp")).read()
    assert "PredictPose" in hpp and "CommitFrame" in hpp and "class System" in hpp and "pgorb_get_trajectory(" in hpp
    mk = open(os.path.join(ROOT, "pilotguru_amd", "csrc", "Makefile")).read()
    assert "track_pose.hip" in mk and "-ffp-contract=off" in mk


def test_record_layouts_agree_with_the_header(tmp_path):
    from pilotguru_amd import _lib
    src, exe = os.path.join(str(tmp_path), "layout.c"), os.path.join(str(tmp_path), "layout")
    open(src, "w").write(C_LAYOUT)
    subprocess.run(["cc", "-std=c99", "-I", ROOT, src, "-o", exe], check=True)
    got = dict(line.split() for line in subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines())
    dts = {"pgorb_kf_pose": _lib.KF_POSE_DTYPE, "pgorb_track_state": _lib.TRACK_STATE_DTYPE, "pgorb_trajectory_record": _lib.TRAJECTORY_RECORD_DTYPE}
    seen = 0
    for k, v in got.items():
        if "." in k:
            s, m = k.split(".")
            assert dts[s].fields[m][1] == int(v), k
            seen += 1
        else:
            assert dts[k].itemsize == int(v), k
    assert seen == len(_lib.TRACK_STATE_DTYPE.names) + len(_lib.TRAJECTORY_RECORD_DTYPE.names)


NAMED = (("right_to_left", "chain"), ("identity_skipped", "signed_zeros"), ("fourth_term_dropped", "signed_zeros_fourth_term"),
         ("origin_index0", "origin"), ("alpha_in_float", "signed_zeros"), ("quat_untransposed", "half_turns"), ("quat_untransposed", "chain"),
         ("time_rounded", "times"))


def test_every_mutant_is_caught_by_name(trajs, sequences):
    assert {n for n, _ in NAMED} | {"velocity_cleared_when_lost"} == set(TR.MUTANTS)
    caught = {name: [c["name"] for c, e in trajs if not K.same(TR.get_trajectory(c, rules), e)] for name, rules in TR.MUTANTS.items()}
    for name, where in NAMED:
        assert where in caught[name], (name, caught[name])
    # the identity case has nothing any reading could change, and the velocity rule is no part of GetTrajectory
    assert all("identity" not in v for v in caught.values()) and caught["velocity_cleared_when_lost"] == []
    m = K.run_sequences_reference(TR.MUTANTS["velocity_cleared_when_lost"])
    differs = [f for f, (a, b) in enumerate(zip(sequences, m)) if not K.same(a, b, K.SEQ_KEYS)]
    assert differs and differs[0] == 2                              # tracker 1 is lost in frame 2: its velocity must survive
    for name, rules in TR.MUTANTS.items():                          # no other reading touches the sequences' velocity rule
        if name in ("time_rounded", "origin_index0", "quat_untransposed", "identity_skipped", "right_to_left"):
            assert all(K.same(a, b, K.SEQ_KEYS) for a, b in zip(sequences, K.run_sequences_reference(rules))), name


def _signs(a):
    return [bool(x) for x in np.signbit(np.asarray(a, f64)).reshape(-1)]


def test_hand_written_expectations(trajs, sequences):
    c, e = by_name([x[0] for x in trajs], "identity"), by_name_e(trajs, "identity")
    assert e["quat_wxyz"].tolist() == [[1.0, 0.0, 0.0, 0.0]] and e["time_usec"].tolist() == [1500000] and e["frame_id"].tolist() == [7]
    # Ow of the identity pose is -0 (alpha = -1 times a +0 sum), so Two carries -0 and the camera centre is -(+0) = -0
    assert _signs(c["pose"][0]["Ow"]) == [True] * 3 and e["translation"].tolist() == [[0.0] * 3] and _signs(e["translation"]) == [True] * 3
    e = by_name_e(trajs, "half_turns")                              # (w, x, y, z): the half turns about x, y, z; PERM' = 120 degrees about -(1, 1, 1)
    assert e["quat_wxyz"][:3].tolist() == [[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]
    assert e["quat_wxyz"][3].tolist() == [-0.5, 0.5, 0.5, 0.5]      # the x branch: trace 0 is not > 0; (w, x, y, z) ~ -(0.5, -0.5, -0.5, -0.5)
    assert e["translation"][:3].tolist() == [[-0.5, -0.25, 2.0], [0.5, 0.25, 2.0], [0.5, -0.25, -2.0]] and e["translation"][3].tolist() == [-2.0, -3.0, -1.0]
    e = by_name_e(trajs, "origin")
    assert e["info"].tolist() == [0, 2, 0, 4]                       # key frame 2: the smallest LIVE id; 3 is bad, 2^33 + 5 is larger than 2^32 + 7
    e = by_name_e(trajs, "signed_zeros")
    # record 0: half_z * (eye * [half_z | (-1, -2, 0)]) = [I | (1, 2, 0)]; 1: [half_z | (-1, -2, 0)]; 2: half_z alone; 3: 45 degrees about z with
    # t = (1, -1, 0): R't = (c - s, -s - c, 0) and c == s in float
    assert e["quat_wxyz"][:3].tolist() == [[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 1.0]]
    assert _signs(e["quat_wxyz"][:3]) == [False, True, False, False] + [False] * 8      # qx of record 0 is (m21 - m12) t = (-0 - +0) t = -0
    assert e["translation"].tolist() == [[-1.0, -2.0, 0.0], [-1.0, -2.0, 0.0], [0.0, 0.0, 0.0], [0.0, float(f32(np.sqrt(f32(2)))), 0.0]]
    assert _signs(e["translation"]) == [True, True, True] * 3 + [True, False, True]      # every zero is alpha = -1 times a +0 sum
    assert np.allclose(e["quat_wxyz"][3], [np.cos(np.pi / 8), 0, 0, -np.sin(np.pi / 8)], atol=1e-7) and _signs(e["quat_wxyz"][3]) == [False, False, False, True]
    e = by_name_e(trajs, "signed_zeros_fourth_term")
    assert e["quat_wxyz"].tolist() == [[0.0, 1.0, 0.0, 0.0]] and _signs(e["quat_wxyz"]) == [False] * 4
    assert e["translation"].tolist() == [[-2.0, 0.0, 0.0]] and _signs(e["translation"]) == [True, True, True]
    e = by_name_e(trajs, "lost")
    assert e["is_lost"].tolist() == [1, 0, 1, 0, 1, 0, 1] and e["status"].tolist() == [0] * 7 and e["frame_id"].tolist() == [0, 10, 20, 30, 40, 50, 60]
    for i in (0, 2, 4, 6):
        assert e["quat_wxyz"][i].tobytes() == bytes(32) and e["translation"][i].tobytes() == bytes(24) and e["time_usec"][i] == (3 + i) * 1000000
    e = by_name_e(trajs, "times")                                   # 0.29 * 1e6 and (1e9 + 0.999999) * 1e6 are integers in double; the next three are not
    assert e["time_usec"].tolist() == [290000, 100000, 1000000000999999, -290000, 299999, 2000000, -299999, 0, 0]
    e = by_name_e(trajs, "broken")
    assert e["status"].tolist() == K.BROKEN_EXPECTED and e["info"].tolist() == [0, 0, 5, 8]
    for i, s in enumerate(K.BROKEN_EXPECTED):
        assert (e["quat_wxyz"][i].tobytes() == bytes(32)) == bool(s)
    # the sequences: statuses, counts, and what a lost frame leaves
    M, V, B, FULL = TR.NO_LAST, TR.NO_VELOCITY, TR.BAD_INDEX, TR.FULL
    assert [f["pred_status"].tolist() for f in sequences] == [[M, M | V | B], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0]]
    assert [f["commit_status"].tolist() for f in sequences] == [[0, 0]] * 5 + [[FULL, FULL]]
    assert [f["count"].tolist() for f in sequences] == [[1, 1], [2, 2], [3, 3], [4, 4], [5, 5], [5, 5]]
    assert sequences[0]["state"]["has_velocity"].tolist() == [0, 0] and sequences[1]["state"]["has_velocity"].tolist() == [1, 1]
    assert sequences[3]["state"]["velocity"][0].tobytes() == sequences[2]["state"]["velocity"][0].tobytes()      # tracker 0 lost in frame 3
    assert sequences[2]["state"]["velocity"][1].tobytes() == sequences[1]["state"]["velocity"][1].tobytes()      # tracker 1 lost in frame 2
    assert sequences[3]["traj"]["lost"].tolist() == [[0, 0, 0, 1, K.SENT], [0, 0, 1, 0, K.SENT]]
    assert sequences[4]["traj"]["ref_kf"][:, 4].tolist() == [2, 1] and sequences[4]["state"]["last_ref_kf"].tolist() == [2, 1]
    assert sequences[5]["state"].tobytes() == sequences[5]["state_mid"].tobytes() and sequences[5]["traj"].tobytes() == sequences[4]["traj"].tobytes()
    # UpdateLastFrame moves the last pose when the key frames moved (frame 3 on), and only in motion-model mode
    assert sequences[3]["state_mid"]["last"]["Tcw"].tobytes() != sequences[2]["state"]["last"]["Tcw"].tobytes()
    assert sequences[1]["state_mid"].tobytes() == sequences[0]["state"].tobytes()
    # the mTcp list
    t = K.tcp_case()
    tcp, info = TR.keyframe_tcp(t["pose"], t["parent"], t["record"], t["nlist"], t["tcp"])
    assert info.tolist() == [0, 2, 2, 0]
    assert [k for k in range(6) if tcp[k].tobytes() != t["tcp"][k].tobytes()] == [2, 4]


def by_name_e(trajs, name):
    return next(e for c, e in trajs if c["name"] == name)


def test_quaternion_branches_of_the_constructed_cases(trajs):
    def branches(name):
        c, hits = by_name([x[0] for x in trajs], name), {}
        TR.get_trajectory(c, hits=hits)
        return {k: v for k, v in hits.items() if k.startswith("quat_")}
    assert branches("identity") == {"quat_trace": 1}
    assert branches("half_turns") == {"quat_x": 2, "quat_y": 1, "quat_z": 1}      # the second x is the boundary: trace exactly 0
    c = by_name([x[0] for x in trajs], "half_turns")
    R = TR.mat44(c["traj"][3]["pose"])[:3, :3].astype(f64)
    assert (R[0, 0] + R[1, 1]) + R[2, 2] == 0.0
    hits = {}
    TR.get_trajectory(by_name([x[0] for x in trajs], "chain"), hits=hits)
    assert [hits.get("depth_%d" % d) for d in range(4)] == [2, 2, 1, 1]


def test_the_forms_of_the_reference_agree(trajs, worlds, sequences):
    for c, e in trajs:
        assert K.same(TR.get_trajectory(c, literal=True), e) and K.same(TR.get_trajectory_batched(c), e), c["name"]
    for c, e, _ in worlds:
        assert K.same(TR.get_trajectory_batched(c), e), c["name"]
        if len(c["traj"]) <= 257:
            assert K.same(TR.get_trajectory(c, literal=True), e), c["name"]
    assert all(K.same(a, b, K.SEQ_KEYS) for a, b in zip(sequences, K.run_sequences_reference(literal=True)))
    t = K.tcp_case()
    a, b = TR.keyframe_tcp(t["pose"], t["parent"], t["record"], t["nlist"], t["tcp"]), \
        TR.keyframe_tcp(t["pose"], t["parent"], t["record"], t["nlist"], t["tcp"], literal=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    no = dict(by_name([x[0] for x in trajs], "chain"))
    no["kf_bad"] = np.ones(6, np.uint8)
    assert TR.get_trajectory(no)["info"].tolist() == TR.get_trajectory_batched(no)["info"].tolist() == [TR.NO_ORIGIN, -1, 0, 6]


def test_float64_anchor_agrees_within_the_bound_of_each_case(trajs, worlds):
    """plain float64 matrix algebra (np.linalg.inv, the quaternion as an eigenvector) against the restatement, up to the quaternion's
    sign, within the bound tests/track_pose_cases.py: anchor derives from each record's own chain"""
    checked = 0
    for c, e in trajs + [(c, e) for c, e, _ in worlds]:
        n = len(c["traj"])
        for i in range(0, n, max(1, n // 64)):
            a = K.anchor(c, i)
            if a is None:
                assert e["is_lost"][i] or e["status"][i] & TR.BROKEN
                continue
            q, t, bq, bt = a
            dq = min(np.abs(q - e["quat_wxyz"][i]).max(), np.abs(q + e["quat_wxyz"][i]).max())
            dt = np.abs(t - e["translation"][i])
            assert bq < 1e-3 and bt.max() < 1e-2, "a bound this loose anchors nothing"
            assert dq <= bq and np.all(dt <= bt), (c["name"], i, dq, bq, dt, bt)
            checked += 1
    assert checked > 500


def test_random_worlds_cover_what_they_are_for(worlds):
    tot = {}
    for c, e, hits in worlds:
        for k, v in hits.items():
            tot[k] = tot.get(k, 0) + v
    assert tot["depth_3"] >= 20 and tot["depth_1"] >= 20 and tot["depth_2"] >= 20, tot
    assert all(tot.get("quat_" + b, 0) >= 20 for b in ("trace", "x", "y", "z")), tot
    assert tot["lost"] >= 100
    assert {len(c["traj"]) for c, _, _ in worlds} == set(K.WORLD_RECORDS) and {len(c["pose"]) for c, _, _ in worlds} == set(K.WORLD_KFS)
    assert any(TR.origin_of(c["kf_bad"], c["kf_id"]) != 0 for c, _, _ in worlds) and any(int(c["kf_id"].max()) > 1 << 32 for c, _, _ in worlds)
    assert max(c["kf_bad"].mean() for c, _, _ in worlds) <= 0.4 and all(not e["status"].any() for _, e, _ in worlds)


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


def _bad_tables(c):
    """(what is wrong, the case) for everything pgorb_get_trajectory refuses"""
    def v(**kw):
        d = {k: np.array(x) for k, x in c.items() if k != "name"}
        for k, (i, f, x) in kw.items():
            if f is None:
                d[k][i] = x
            else:
                d[k][f][i] = x
        return d
    yield "a bad key frame without a parent", v(parent=(2, None, -1))
    yield "a bad key frame with a parent out of range", v(parent=(2, None, 6))
    yield "a reference of nkf", v(traj=(1, "ref_kf", 6))
    yield "a negative reference", v(traj=(1, "ref_kf", -1))
    yield "a NaN time", v(traj=(0, "frame_time", np.nan))
    yield "an infinite time", v(traj=(0, "frame_time", np.inf))
    yield "a time outside int64 microseconds", v(traj=(0, "frame_time", 1e13))
    yield "a time below int64 microseconds", v(traj=(0, "frame_time", -1e13))
    d = v()
    d["kf_bad"][:] = 1
    d["parent"][0] = 1
    yield "no live key frame", d


def test_python_mirrors_refuse_malformed_input_without_a_device(trajs):
    import pilotguru_amd as pg
    c = by_name([x[0] for x in trajs], "chain")
    ext = _NoLibrary()
    get = lambda d: pg.System.GetTrajectory(ext, d["pose"], d["kf_bad"], d["parent"], d["kf_id"], d["tcp"], d["traj"])
    for what, d in _bad_tables(c):
        with pytest.raises(ValueError):
            get(d)
    with pytest.raises(ValueError):
        pg.System.GetTrajectory(ext, c["pose"][:3], c["kf_bad"], c["parent"], c["kf_id"], c["tcp"], c["traj"])
    with pytest.raises(ValueError):
        pg.System.GetTrajectory(ext, np.zeros(5000, pg.KF_POSE_DTYPE), np.zeros(5000, np.uint8), np.zeros(5000, np.int32), np.zeros(5000, np.uint64), None, c["traj"])
    with pytest.raises(AssertionError, match="the library was called"):
        get(c)
    state, frames = K.track_sequences()
    with pytest.raises(ValueError):
        pg.Tracking.PredictPose(ext, state[0], 2, frames[0]["kf"])
    with pytest.raises(ValueError):
        pg.Tracking.PredictPose(ext, state[0], pg.TRACK_REFERENCE_KF, np.zeros(5000, pg.KF_POSE_DTYPE))
    with pytest.raises(AssertionError, match="the library was called"):
        pg.Tracking.PredictPose(ext, state[0], pg.TRACK_REFERENCE_KF, frames[0]["kf"])
    x = frames[0]["trackers"][0]
    with pytest.raises(ValueError):
        pg.Tracking.CommitFrame(ext, state[0], x["pose"], 1, 0, 0.0, 0, np.zeros(5000, pg.KF_POSE_DTYPE), np.zeros(4, pg.TRAJECTORY_RECORD_DTYPE), 0)
    with pytest.raises(AssertionError, match="the library was called"):
        pg.Tracking.CommitFrame(ext, state[0], x["pose"], 1, 0, 0.0, 0, frames[0]["kf"], np.zeros(4, pg.TRAJECTORY_RECORD_DTYPE), 0)
    t = K.tcp_case()
    with pytest.raises(ValueError):
        pg.LocalMapping.KeyFrameTcp(ext, t["pose"][:3], t["parent"], t["record"])
    with pytest.raises(ValueError):
        pg.LocalMapping.KeyFrameTcp(ext, t["pose"], t["parent"], t["record"], tcp=np.zeros((5, 12), f32))
    with pytest.raises(AssertionError, match="the library was called"):
        pg.LocalMapping.KeyFrameTcp(ext, t["pose"], t["parent"], t["record"])


CPP_DRIVER = r"""
#include "pilotguru_amd/host/orb_extractor.hpp"
#include <cstdio>
#include <limits>
template <class F> static void run(const char* name, F&& f)
{
    try { f(); std::printf("%s ok\n", name); }
    catch (const std::invalid_argument&) { std::printf("%s invalid_argument\n", name); }
    catch (const std::runtime_error&) { std::printf("%s runtime_error\n", name); }
}
static pgorb_kf_pose ident()
{
    pgorb_kf_pose P{};
    P.Tcw[0] = P.Tcw[5] = P.Tcw[10] = 1.0f;
    P.fx = P.fy = 500.0f;
    return P;
}
int main()
{
    using namespace pgorb;
    // three key frames: 0 live, 1 culled under 0, 2 live; two records
    const std::vector<pgorb_kf_pose> poses(3, ident());
    const std::vector<uint8_t> bad = {0, 1, 0};
    const std::vector<int32_t> parent = {-1, 0, 0};
    const std::vector<uint64_t> ids = {0, 1, 2};
    const std::vector<float> tcp(36, 0.0f);
    pgorb_trajectory_record r{};
    r.pose[0] = r.pose[5] = r.pose[10] = 1.0f; r.has_pose = 1; r.ref_kf = 1; r.frame_time = 1.0;
    const std::vector<pgorb_trajectory_record> traj(2, r);
    System sys(nullptr);
    Tracking trk(nullptr);
    run("well_formed", [&] { sys.GetTrajectory(poses, bad, parent, ids, tcp, traj); });
    { auto p = parent; p[1] = -1; run("bad_without_parent", [&] { sys.GetTrajectory(poses, bad, p, ids, tcp, traj); }); }
    { auto p = parent; p[1] = 3; run("bad_parent_range", [&] { sys.GetTrajectory(poses, bad, p, ids, tcp, traj); }); }
    { auto t = traj; t[1].ref_kf = 3; run("ref_range", [&] { sys.GetTrajectory(poses, bad, parent, ids, tcp, t); }); }
    { auto t = traj; t[1].ref_kf = 3; t[1].lost = 1; run("ref_range_lost", [&] { sys.GetTrajectory(poses, bad, parent, ids, tcp, t); }); }
    { auto t = traj; t[0].frame_time = std::numeric_limits<double>::quiet_NaN(); run("time_nan", [&] { sys.GetTrajectory(poses, bad, parent, ids, tcp, t); }); }
    { auto t = traj; t[0].frame_time = 1e13; run("time_range", [&] { sys.GetTrajectory(poses, bad, parent, ids, tcp, t); }); }
    { std::vector<uint8_t> b = {1, 1, 1}; auto p = parent; p[0] = 1; run("no_live", [&] { sys.GetTrajectory(poses, b, p, ids, tcp, traj); }); }
    { auto b = bad; b.pop_back(); run("sizes", [&] { sys.GetTrajectory(poses, b, parent, ids, tcp, traj); }); }
    pgorb_track_state st{};
    pgorb_kf_pose out{};
    run("predict_well_formed", [&] { trk.PredictPose(st, PGORB_TRACK_REFERENCE_KF, poses, nullptr, out); });
    run("predict_mode", [&] { trk.PredictPose(st, 2, poses, nullptr, out); });
    std::vector<pgorb_trajectory_record> mine(4);
    int32_t count = 0;
    run("commit_well_formed", [&] { trk.CommitFrame(st, poses[0], true, 0, 1.0, 7, poses, mine, count); });
    count = -1;
    run("commit_count", [&] { trk.CommitFrame(st, poses[0], true, 0, 1.0, 7, poses, mine, count); });
    return 0;
}
"""


def test_cpp_mirror_rejects_bad_inputs_before_calling_the_library(tmp_path):
    """pgorb::System and pgorb::Tracking throw std::invalid_argument for what the single calls would refuse, before any pointer
    reaches the library; well-formed input reaches it (a NULL context here, so PGORB_E_ARG comes back as std::runtime_error)."""
    src, exe = os.path.join(str(tmp_path), "traj_driver.cc"), os.path.join(str(tmp_path), "traj_driver")
    open(src, "w").write(CPP_DRIVER)
    subprocess.run(["g++", "-std=c++17", "-I", ROOT, "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", os.path.join(ROOT, "pilotguru_amd"), "-lpgorb",
                    "-Wl,-rpath," + os.path.join(ROOT, "pilotguru_amd"), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = dict(line.split() for line in subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines())
    reached = {"well_formed", "ref_range_lost", "predict_well_formed", "commit_well_formed"}
    assert len(out) == 13
    for k, v in out.items():
        assert v == ("runtime_error" if k in reached else "invalid_argument"), (k, v)


def test_write_poses_round_trips_through_the_cli(tmp_path, trajs, worlds):
    """System.write_poses -> the built optical_trajectories --poses_in -> trajectory-0.json: the ids, the lost flags and, to 15
    significant digits, the translations (the reference's writer prints 15).  No GPU is involved."""
    import pilotguru_amd as pg
    if not os.path.exists(CLI):
        pytest.fail("pilotguru_amd/host/optical_trajectories is not built")
    # a planar ride (the CLI drops a trajectory whose third principal component is not small), some records lost
    n = 60
    h = np.linspace(0.0, 1.2, n)
    traj = dict(translation=np.stack([np.cumsum(np.sin(h)) * 0.1, np.zeros(n) + 1e-4 * np.sin(7 * h), np.cumsum(np.cos(h)) * 0.1], 1) * (1 + 1 / 3.0),
                quat_wxyz=np.stack([np.cos(h / 2), np.zeros(n), np.sin(h / 2), np.zeros(n)], 1) / 3.0 * 3.0,
                time_usec=(1000000 + 33333 * np.arange(n)).astype(np.int64), frame_id=(5 + np.arange(n)).astype(np.int64), is_lost=np.zeros(n, np.uint8))
    traj["is_lost"][[0, 17, 18, n - 1]] = 1
    for k in ("translation", "quat_wxyz"):
        traj[k][traj["is_lost"] != 0] = 0.0
    poses = os.path.join(str(tmp_path), "poses.txt")
    pg.System.write_poses(poses, traj)
    lines = open(poses).read().splitlines()
    assert len(lines) == n
    for i, ln in enumerate(lines):                                  # %.17g: every double comes back bit for bit
        w = ln.split()
        assert [int(w[0]), int(w[1]), int(w[2])] == [int(traj["time_usec"][i]), int(traj["is_lost"][i]), int(traj["frame_id"][i])]
        assert np.array([float(x) for x in w[3:]], f64).tobytes() == np.concatenate([traj["translation"][i], traj["quat_wxyz"][i]]).tobytes()
    r = subprocess.run([CLI, "--poses_in=" + poses, "--out_dir=" + str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr
    d = json.load(open(os.path.join(str(tmp_path), "trajectory-0.json")))
    assert len(d["trajectory"]) == n
    r15 = lambda x: float("%.15g" % x)
    for i, p in enumerate(d["trajectory"]):
        assert p["frame_id"] == int(traj["frame_id"][i]) and p["time_usec"] == int(traj["time_usec"][i]) and p["is_lost"] is bool(traj["is_lost"][i])
        assert p["pose"]["translation"] == [r15(v) for v in traj["translation"][i]]
    # and a GetTrajectory result as the reference returns it: same keys, same layout
    c, e = next(x for x in trajs if x[0]["name"] == "chain")
    pg.System.write_poses(poses, e)
    assert len(open(poses).read().splitlines()) == len(c["traj"])


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    return pg.ORBextractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240)


def _check_traj(c, e, ext, host=True, **kw):
    n = len(c["traj"])
    got = K.run_get_trajectory_device(c, ext, **kw)
    assert K.same(got, K.padded(e, n)), c["name"]
    if host:
        rc, out = K.run_get_trajectory_host(c, ext)
        assert rc == int(((e["is_lost"] == 0) & ((e["status"] & TR.BROKEN) == 0)).sum()) and K.same(out, e), c["name"]


@pytest.mark.gpu
def test_gpu_constructed_cases_equal_the_reference_in_both_forms(ext, trajs):
    from pilotguru_amd import _lib
    for c, e in trajs:
        _check_traj(c, e, ext, host=c["name"] != "broken")
    # the single call refuses the broken table; a table whose only faults are the cycle and the record without a pose runs and marks them
    c, e = next(x for x in trajs if x[0]["name"] == "broken")
    assert K.run_get_trajectory_host(c, ext)[0] == _lib.PGORB_E_ARG
    d = {k: np.array(v) for k, v in c.items() if k != "name"}
    d["name"] = "cycle_and_no_pose"
    d["parent"][1] = 0
    d["traj"] = d["traj"][[0, 1, 2, 3, 5, 6]]
    e2 = TR.get_trajectory(d)
    assert e2["status"].tolist() == [0, 0, 0, TR.BROKEN, TR.BROKEN, 0]
    _check_traj(d, e2, ext)


@pytest.mark.gpu
def test_gpu_random_worlds_equal_the_reference(ext, worlds):
    for i, (c, e, _) in enumerate(worlds):
        _check_traj(c, e, ext, host=i % 5 == 2)


@pytest.mark.gpu
def test_gpu_large_case_equals_the_reference(ext, large):
    """108 000 records over 2 000 key frames, 30 % of them culled"""
    c, e = large
    assert len(c["traj"]) == 108000 and int(c["kf_bad"].sum()) == 600
    _check_traj(c, e, ext, host=True)


@pytest.mark.gpu
def test_gpu_count_on_the_device_cuts_the_records(ext, trajs):
    """d_count = a tracker's d_ntrajectory entry: records at or past it are not read and their outputs keep their bytes; no live key
    frame: PGORB_TRAJ_NO_ORIGIN and nothing else written"""
    c, e = next(x for x in trajs if x[0]["name"] == "chain")
    for count in (0, 3, 6, 9, -2):
        m = max(0, min(count, 6))
        got = K.run_get_trajectory_device(c, ext, count=count)
        assert K.same(got, K.padded(TR.get_trajectory(c, n=m), 6)), count
    d = dict(c)
    d["kf_bad"] = np.ones(6, np.uint8)
    got = K.run_get_trajectory_device(d, ext)
    assert K.same(got, K.padded(TR.get_trajectory(d), 6)) and got["info"].tolist() == [TR.NO_ORIGIN, -1, 0, 6]


@pytest.mark.gpu
def test_gpu_single_calls_refuse_malformed_input(ext, trajs):
    from pilotguru_amd import _lib
    c = by_name([x[0] for x in trajs], "chain")
    assert K.run_get_trajectory_host(c, ext)[0] == 6
    for what, d in _bad_tables(c):
        assert K.run_get_trajectory_host(d, ext)[0] == _lib.PGORB_E_ARG, what
    hbuf = np.zeros(4096, np.uint8)
    L, h, p = ext._L, ext._h, K._p(hbuf)
    assert L.pgorb_get_trajectory(h, -1, *([p] * 5), 0, *([p] * 8)) == _lib.PGORB_E_ARG
    assert L.pgorb_get_trajectory(h, 1, p, None, p, p, p, 0, *([p] * 8)) == _lib.PGORB_E_ARG
    assert L.pgorb_track_predict(h, 2, p, p, 1, p, p) == _lib.PGORB_E_ARG
    assert L.pgorb_track_predict(h, 0, None, p, 1, p, p) == _lib.PGORB_E_ARG
    assert L.pgorb_track_commit(h, p, p, 1, 0, 0.0, 0, -1, p, p, 1, p) == _lib.PGORB_E_ARG
    assert L.pgorb_track_commit(h, p, p, 1, 0, 0.0, 0, 1, p, None, 1, p) == _lib.PGORB_E_ARG
    assert L.pgorb_keyframe_tcp(h, 1, p, p, -1, p, p, p) == _lib.PGORB_E_ARG
    assert L.pgorb_keyframe_tcp(h, 1, p, p, 1, None, p, p) == _lib.PGORB_E_ARG


@pytest.mark.gpu
def test_gpu_limits_at_capacity_and_one_past_it(ext, worlds):
    """PGORB_E_LIMIT one past every capacity (nothing is launched, so nothing large is allocated), and each call at its capacity:
    4 096 key frames in one culled chain, 1 << 22 records (a world's records repeated on the device), 4 096 trackers, and a record
    array of 1 << 22 entries whose last one is written and then found full"""
    import torch
    from pilotguru_amd import _lib
    L, h = ext._L, ext._h
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p, MAXN, MAXKF, MAXT = C.c_void_p(d.data_ptr()), 1 << 22, 4096, 4096
    assert L.pgorb_get_trajectory_device(h, MAXKF + 1, *([p] * 5), 1, *([p] * 10)) == _lib.PGORB_E_LIMIT
    assert L.pgorb_get_trajectory_device(h, 1, *([p] * 5), MAXN + 1, *([p] * 10)) == _lib.PGORB_E_LIMIT
    assert L.pgorb_track_predict_batch_device(h, MAXT + 1, 0, p, p, p, 1, p, 1, p, p, p, None) == _lib.PGORB_E_LIMIT
    assert L.pgorb_track_predict_batch_device(h, 1, 0, p, p, p, MAXN + 1, p, 1, p, p, p, None) == _lib.PGORB_E_LIMIT
    assert L.pgorb_track_predict_batch_device(h, 1, 0, p, p, p, 1, p, MAXKF + 1, p, p, p, None) == _lib.PGORB_E_LIMIT
    assert L.pgorb_track_commit_batch_device(h, MAXT + 1, *([p] * 6), 1, p, p, 1, p, p, None) == _lib.PGORB_E_LIMIT
    assert L.pgorb_track_commit_batch_device(h, 1, *([p] * 6), MAXKF + 1, p, p, 1, p, p, None) == _lib.PGORB_E_LIMIT
    assert L.pgorb_track_commit_batch_device(h, 1, *([p] * 6), 1, p, p, MAXN + 1, p, p, None) == _lib.PGORB_E_LIMIT
    assert L.pgorb_keyframe_tcp_device(h, MAXKF + 1, p, p, 1, p, p, p, p, None) == _lib.PGORB_E_LIMIT
    assert L.pgorb_keyframe_tcp_device(h, 1, p, p, MAXKF + 1, p, p, p, p, None) == _lib.PGORB_E_LIMIT
    hbuf = np.zeros(4096, np.uint8)
    hp = K._p(hbuf)
    assert L.pgorb_get_trajectory(h, MAXKF + 1, *([hp] * 5), 0, *([hp] * 8)) == _lib.PGORB_E_LIMIT
    assert L.pgorb_get_trajectory(h, 1, *([hp] * 5), MAXN + 1, *([hp] * 8)) == _lib.PGORB_E_LIMIT
    assert L.pgorb_track_predict(h, 0, hp, hp, MAXKF + 1, hp, hp) == _lib.PGORB_E_LIMIT
    assert L.pgorb_track_commit(h, hp, hp, 1, 0, 0.0, 0, 1, hp, hp, MAXN + 1, hp) == _lib.PGORB_E_LIMIT
    assert L.pgorb_keyframe_tcp(h, 1, hp, hp, MAXKF + 1, hp, hp, hp) == _lib.PGORB_E_LIMIT
    # nkf at capacity: key frame 0 live, every other one culled under its predecessor; records at depth 0, 1, 4 094 and 4 095
    pose = K.stack([K.make_pose(K.rot([0.1, 1, 0.2], 0.05 * (k % 7)), [0.001 * (k % 11), 0.0, 0.002]) for k in range(16)], K.KF_POSE_DTYPE)
    pose = np.tile(pose, MAXKF // 16)
    bad, parent = np.ones(MAXKF, np.uint8), np.arange(-1, MAXKF - 1).astype(np.int32)
    bad[0] = 0
    c = K.case("chain4096", pose, bad, parent, np.arange(MAXKF), [K.record(K.rows(np.eye(3), [0.1, 0, 0]), k, 1.0, k) for k in (0, 1, MAXKF - 2, MAXKF - 1)])
    _check_traj(c, TR.get_trajectory_batched(c), ext)
    # n at capacity: 4 096 records of a world 1 024 times over, compared on the device
    w, e, _ = next(x for x in worlds if len(x[0]["traj"]) == 4099 and len(x[0]["pose"]) == 300)
    w = dict(w)
    w["traj"] = w["traj"][:4096]
    e = TR.get_trajectory(w, n=4096)
    D = K.table_device_arrays(w)
    traj = K._up(w["traj"]).repeat(1024)
    O = {k: torch.full((MAXN * nb,), K.SENT, dtype=torch.uint8, device="cuda") for k, nb in (("quat_wxyz", 32), ("translation", 24), ("time_usec", 8),
                                                                                           ("frame_id", 8), ("is_lost", 1), ("status", 4))}
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    q = K._q
    assert L.pgorb_get_trajectory_device(h, 300, q(D["pose"]), q(D["bad"]), q(D["par"]), q(D["ids"]), q(D["tcp"]), MAXN, q(traj), None, q(O["quat_wxyz"]),
                                         q(O["translation"]), q(O["time_usec"]), q(O["frame_id"]), q(O["is_lost"]), q(O["status"]), q(info), None) == 0
    torch.cuda.synchronize()
    for k in O:
        assert torch.equal(O[k], K._up(e[k]).repeat(1024)), k
    assert info.cpu().tolist() == [0, int(e["info"][1]), 1024 * int(e["info"][2]), MAXN]
    del O, traj
    # ntrack at capacity: the two trackers of the sequences after frame 2, 2 048 times over, through predict and commit
    _tracker_capacity(ext, MAXT)
    # traj_cap at capacity: one tracker whose count is one below it
    state, frames = K.track_sequences()
    S, N = K._up(state[:1]), K._up(np.array([MAXN - 1], np.int32))
    T = torch.full((MAXN * 72,), K.SENT, dtype=torch.uint8, device="cuda")
    x, kf = frames[0]["trackers"][0], K._up(frames[0]["kf"])
    held = [K._up(x["pose"]), K._up(np.array([1], np.uint8)), K._up(np.array([0], np.int32)), K._up(np.array([x["time"]], f64)),
            K._up(np.array([x["id"]], np.int64))]
    args = [q(t) for t in held]
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    trk = TR.Tracker(state[0])
    assert TR.commit(trk, x["pose"], 1, 0, x["time"], x["id"], frames[0]["kf"], MAXN) == 0
    for want_status, want_count in ((0, MAXN), (TR.FULL, MAXN)):
        assert L.pgorb_track_commit_batch_device(h, 1, q(S), *args, 4, q(kf), q(T), MAXN, q(N), q(st), None) == 0
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [want_status] and np.frombuffer(N.cpu().numpy().tobytes(), np.int32).tolist() == [want_count]
        assert T[(MAXN - 1) * 72:].cpu().numpy().tobytes() == trk.trajectory[0].tobytes() and int(T[(MAXN - 1) * 72 - 1]) == K.SENT
        assert S.cpu().numpy().tobytes() == trk.state().tobytes()


def _tracker_capacity(ext, ntrack):
    import torch
    ref = K.run_sequences_reference()
    state, frames = K.track_sequences()
    fr, cap, q, s = frames[3], K.CAP, K._q, torch.cuda.current_stream()
    rep = ntrack // 2
    S = K._up(ref[2]["state"]).repeat(rep)
    T = K._up(ref[2]["traj"]).repeat(rep)
    N = K._up(ref[2]["count"]).repeat(rep)
    x = fr["trackers"]
    kf, modes = K._up(fr["kf"]), K._up(np.array([v["mode"] for v in x], np.int32)).repeat(rep)
    pred, ps, cs = K._sent(ntrack * 84), K._sent(ntrack * 4), K._sent(ntrack * 4)
    assert ext._L.pgorb_track_predict_batch_device(ext._h, ntrack, 0, q(modes), q(S), q(T), cap, q(N), 4, q(kf), q(pred), q(ps), C.c_void_p(s.cuda_stream)) == 0
    pose, ok, rk = K._up(K.stack([v["pose"] for v in x], K.KF_POSE_DTYPE)).repeat(rep), K._up(np.array([v["ok"] for v in x], np.uint8)).repeat(rep), \
        K._up(np.array([v["ref_kf"] for v in x], np.int32)).repeat(rep)
    tm, ids = K._up(np.array([v["time"] for v in x], f64)).repeat(rep), K._up(np.array([v["id"] for v in x], np.int64)).repeat(rep)
    assert ext._L.pgorb_track_commit_batch_device(ext._h, ntrack, q(S), q(pose), q(ok), q(rk), q(tm), q(ids), 4, q(kf), q(T), cap, q(N), q(cs),
                                                  C.c_void_p(s.cuda_stream)) == 0
    s.synchronize()
    for got, want in ((pred, ref[3]["pred"]), (ps, ref[3]["pred_status"]), (cs, ref[3]["commit_status"]), (S, ref[3]["state"]), (T, ref[3]["traj"]),
                      (N, ref[3]["count"])):
        assert torch.equal(got, K._up(want).repeat(rep))


@pytest.mark.gpu
def test_gpu_predict_commit_sequences_equal_the_reference_in_both_forms(ext, sequences):
    """six frames on two trackers: both modes, a lost frame in the middle, a reference change, the capacity reached"""
    dev, host = K.run_sequences_device(ext), K.run_sequences_host(ext)
    for f, (e, a, b) in enumerate(zip(sequences, dev, host)):
        assert K.same(a, e, K.SEQ_KEYS), f
        # the single calls see one tracker: the record array behind the count and the statuses are the same, the sentinel included
        assert K.same(b, e, K.SEQ_KEYS), f


@pytest.mark.gpu
def test_gpu_python_mirrors_return_what_the_reference_leaves(ext, trajs, sequences):
    import pilotguru_amd as pg
    c, e = next(x for x in trajs if x[0]["name"] == "chain")
    got = pg.System.GetTrajectory(ext, c["pose"], c["kf_bad"], c["parent"], c["kf_id"], c["tcp"], c["traj"])
    assert K.same({k: got[k] for k in K.TRAJ_KEYS}, e) and got["origin"] == 0
    state, frames = K.track_sequences()
    st, traj, cnt = state[0], np.zeros(K.CAP, pg.TRAJECTORY_RECORD_DTYPE), 0
    for f, fr in enumerate(frames):
        x = fr["trackers"][0]
        r = pg.Tracking.PredictPose(ext, st, x["mode"], fr["kf"], traj[cnt - 1] if cnt else None)
        assert r["status"] == sequences[f]["pred_status"][0] and r["pose"].tobytes() == sequences[f]["pred"][0].tobytes()
        assert r["state"].tobytes() == sequences[f]["state_mid"][0].tobytes()
        r = pg.Tracking.CommitFrame(ext, r["state"], x["pose"], x["ok"], x["ref_kf"], x["time"], x["id"], fr["kf"], traj, cnt)
        st, traj, cnt = r["state"], r["trajectory"], r["ntrajectory"]
        assert r["status"] == sequences[f]["commit_status"][0] and st.tobytes() == sequences[f]["state"][0].tobytes() and cnt == sequences[f]["count"][0]
        assert traj[:cnt].tobytes() == sequences[f]["traj"][0][:cnt].tobytes()
    t = K.tcp_case()
    r = pg.LocalMapping.KeyFrameTcp(ext, t["pose"], t["parent"], t["record"][:t["nlist"]], t["tcp"])
    tcp, info = TR.keyframe_tcp(t["pose"], t["parent"], t["record"], t["nlist"], t["tcp"])
    assert r["tcp"].tobytes() == tcp.tobytes() and r["info"].tolist() == info.tolist() and r["written"] == 2


@pytest.mark.gpu
def test_gpu_keyframe_tcp_writes_the_culled_rows_only(ext):
    t = K.tcp_case()
    tcp, info = TR.keyframe_tcp(t["pose"], t["parent"], t["record"], t["nlist"], t["tcp"])
    got, ginfo = K.run_tcp_device(t, ext)
    assert got.tobytes() == tcp.tobytes() and ginfo.tolist() == info.tolist() == [0, 2, 2, 0]
    assert [k for k in range(6) if got[k].tobytes() != t["tcp"][k].tobytes()] == [2, 4]      # the others keep the poison pattern
    rc, htcp, hinfo = K.run_tcp_host(t, ext)
    assert rc == 2 and htcp.tobytes() == tcp.tobytes() and hinfo.tolist() == info.tolist()
    got, ginfo = K.run_tcp_device(t, ext, limit=True)                # a culling that reported PGORB_CULL_LIMIT did nothing
    assert got.tobytes() == t["tcp"].tobytes() and ginfo.tolist() == [0, 0, 0, 0]


@pytest.mark.gpu
def test_gpu_repeat_second_stream_and_a_used_context_give_the_same_bytes(ext, trajs, worlds, sequences):
    import torch
    t = K.tcp_case()
    want_tcp = TR.keyframe_tcp(t["pose"], t["parent"], t["record"], t["nlist"], t["tcp"])[0].tobytes()
    picks = [x for x in trajs if x[0]["name"] in ("chain", "signed_zeros")] + [(c, e) for c, e, _ in worlds if len(c["traj"]) == 257 and len(c["pose"]) == 17]
    for c, e in picks:
        first = K.run_get_trajectory_device(c, ext)
        K.run_sequences_device(ext)                                  # the context runs other calls in between
        again = K.run_get_trajectory_device(c, ext)
        other = K.run_get_trajectory_device(c, ext, stream=torch.cuda.Stream())
        want = K.padded(e, len(c["traj"]))
        assert K.same(first, again) and K.same(first, other) and K.same(first, want), c["name"]
    s2 = torch.cuda.Stream()
    for a, b, e in zip(K.run_sequences_device(ext), K.run_sequences_device(ext, stream=s2), sequences):
        assert K.same(a, e, K.SEQ_KEYS) and K.same(b, e, K.SEQ_KEYS)
    assert K.run_tcp_device(t, ext)[0].tobytes() == K.run_tcp_device(t, ext, stream=s2)[0].tobytes() == want_tcp


CHAIN_MODES = (TR.REFERENCE_KF, TR.MOTION_MODEL, TR.MOTION_MODEL)


def _frame_references(c, mps, obs, pose):
    """one frame of the tracking chain from the predicted pose: the last-frame search of tests/tracking_reference.py, the slots it gives
    and the pose problem of tests/pose_cases.py they make, under the condition every compared pose case meets"""
    import pose_cases as PC
    import pose_reference as PR
    import tracking_cases as TKC
    import tracking_reference as TKR
    fr = TKR.Frame(1, c.keys, c.desc, TKC.BOUNDS, pose, TKC.SF, TKC.log_sf(), TKC.NLEVELS)
    r1 = TKR.search_by_projection_last_frame(fr, c.other_keys, [None if s < 0 else mps[s] for s in c.other_point], c.flag, c.has, c.th, c.ori)
    a = r1["assigned"]
    kp_point = np.where(a >= 0, c.other_point[np.maximum(a, 0)], -1).astype(np.int32)
    pc = PC.Case("chain_" + c.name, np.stack([c.keys["x"], c.keys["y"]], 1), c.keys["octave"], pose, kp_point, np.array([p["pos"] for p in c.points], f32), obs)
    traces = []
    for order in PR.ORDERS:
        tr = []
        PC.run_reference(pc, order, discard=True, trace=tr)
        traces.append(tr)
    for tr in traces:
        for (fl, c2), (fl0, _) in zip(tr, traces[0]):
            assert np.array_equal(fl, fl0) and (np.abs(c2 / 5.991 - 1.0) > 1e-4).all(), "%s: rebuild the scene" % pc.name
    return r1, kp_point, pc, PC.run_reference(pc, discard=True), PC.spread(pc)


def _chain_scene():
    import tracking_cases as TKC
    c = [x for x in TKC.single_cases() if x.name == "last_scene"][0]
    state = np.zeros(1, K.TRACK_STATE_DTYPE)
    state[0]["last"], state[0]["has_last"], state[0]["last_ref_kf"] = c.pose, 1, 0
    return c, state, K.stack([c.pose], K.KF_POSE_DTYPE)


def test_tracking_chain_scene_meets_the_case_condition():
    """the three frames of the resident chain with the reference's own pose standing in for the device's: the second and third
    frame start from the motion model's prediction, find matches and leave edges to optimise"""
    import tracking_cases as TKC
    c, state, kf = _chain_scene()
    _, mps = c.build()
    obs = TKC.table_arrays(c.points)[3]
    trk = TR.Tracker(state[0], cap=4)
    for f, mode in enumerate(CHAIN_MODES):
        pred, status = TR.predict(trk, mode, kf)
        assert status == 0
        r1, kp_point, pc, r3, _ = _frame_references(c, mps, obs, pred)
        assert r1["nmatches"] >= 20 and pc.edges >= 30 and r3["nmatches_map"] >= 10
        out = np.array(pred)
        out["Tcw"], out["Ow"] = np.asarray(r3["Tcw"], f32).reshape(12), np.asarray(r3["Ow"], f32).reshape(3)
        assert TR.commit(trk, out, 1, 0, 10.0 + f / 30.0, f, kf, 4) == 0
    assert trk.has_velocity and len(trk.trajectory) == 3


@pytest.mark.gpu
def test_gpu_chain_predict_search_slots_pose_commit_on_a_resident_batch(ext):
    """pgorb_track_predict_batch_device -> pgorb_search_by_projection_last_frame_batch_device ->
    pgorb_slots_from_assignment_batch_device -> pgorb_pose_optimization_batch_device -> pgorb_track_commit_batch_device for three
    consecutive frames (reference-KF mode, then the motion model twice) with nothing downloaded in between: every stage reads the
    previous stage's arrays where they lie.  Afterwards every stage is held against its reference fed with what the stage before it
    produced; the pose optimisation within the bounds of tests/pose_cases.py, everything else byte for byte."""
    import torch
    import pose_cases as PC
    import tracking_cases as TKC
    from pilotguru_amd.orb import KEYPOINT_DTYPE
    c, state, kf = _chain_scene()
    b = TKC.as_batch(c)
    L, h = ext._L, ext._h
    nf, cap = len(b.frames), b.qcap
    kp, ds = np.zeros((nf, cap), KEYPOINT_DTYPE), np.zeros((nf, cap, 32), np.uint8)
    for f, (k, d) in enumerate(b.frames):
        kp[f, :len(k)] = k
        ds[f, :len(k)] = d
    pts, pd, bad, obs = TKC.table_arrays(b.points)
    npts = len(pts)
    keep = []

    def p(t):
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def row(a, dtype, fill=0):
        x = np.full((1, cap), fill, dtype)
        x[0, :len(a)] = a
        return dev(x)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dk, dd, dn = dev(kp.view(np.uint8).reshape(nf, cap, 28)), dev(ds), dev(np.array([len(k) for k, _ in b.frames], np.int32))
    gs = torch.empty((nf, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    gi = torch.empty((nf, cap), dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_frame_grid_batch_device(h, p(dk), p(dn), nf, cap, *TKC.BOUNDS, p(gs), p(gi), s))
    dpts, dpd, dobs = dev(pts.view(np.uint8).reshape(npts, 32)), dev(pd), dev(obs)
    (fcur, fother, _), = b.pairs
    pf, po = dev(np.array([fcur], np.int32)), dev(np.array([fother], np.int32))
    op, flag, has = row(c.other_point, np.int32, -1), row(c.flag, np.uint8), row(c.has, np.uint8)
    I32 = lambda *sh: torch.full(sh, -9, dtype=torch.int32, device="cuda")
    S, T, N, dkf = K._up(state), K._sent(4 * 72), K._up(np.zeros(1, np.int32)), K._up(kf)
    ok, rk = K._up(np.array([1], np.uint8)), K._up(np.array([0], np.int32))
    frames = []
    for f, mode in enumerate(CHAIN_MODES):
        F = dict(pred=K._sent(84), ps=I32(1), asg=I32(1, cap), nm=I32(1), kpp=torch.full((1, cap), -1, dtype=torch.int32, device="cuda"),
                 pose_out=torch.zeros(84, dtype=torch.uint8, device="cuda"), outl=torch.full((1, cap), 9, dtype=torch.uint8, device="cuda"), kpo=I32(1, cap),
                 nmap=I32(1), info=I32(1, 8), ninl=I32(1), chi=torch.zeros((1, cap), dtype=torch.float32, device="cuda"), cs=I32(1),
                 tm=K._up(np.array([10.0 + f / 30.0], f64)), ids=K._up(np.array([f], np.int64)))
        ext._check(L.pgorb_track_predict_batch_device(h, 1, mode, None, p(S), p(T), 4, p(N), 1, p(dkf), p(F["pred"]), p(F["ps"]), s))
        ext._check(L.pgorb_search_by_projection_last_frame_batch_device(
            h, p(dk), p(dd), p(dn), cap, p(gs), p(gi), p(pf), p(po), 1, *TKC.BOUNDS, p(F["pred"]), p(has), p(op), p(flag), npts, p(dpts), p(dpd), p(dobs),
            c.th, int(c.ori), None, None, None, p(F["asg"]), p(F["nm"]), s))
        ext._check(L.pgorb_slots_from_assignment_batch_device(h, p(F["asg"]), p(op), cap, p(F["kpp"]), cap, 1, s))
        ext._check(L.pgorb_pose_optimization_batch_device(h, p(dk), p(dn), cap, p(pf), 1, p(F["pred"]), p(F["kpp"]), npts, p(dpts), p(dobs), 1, p(F["pose_out"]),
                                                          p(F["outl"]), p(F["kpo"]), p(F["nmap"]), p(F["chi"]), p(F["info"]), p(F["ninl"]), s))
        F["state_mid"] = S.clone()
        ext._check(L.pgorb_track_commit_batch_device(h, 1, p(S), p(F["pose_out"]), p(ok), p(rk), p(F["tm"]), p(F["ids"]), 1, p(dkf), p(T), 4, p(N), p(F["cs"]), s))
        F["state"], F["traj"], F["count"] = S.clone(), T.clone(), N.clone()
        frames.append(F)
    torch.cuda.synchronize()                                             # the first download
    H = lambda t: t.cpu().numpy()
    _, mps = c.build()
    n = len(c.keys)
    trk = TR.Tracker(state[0], cap=4)
    fill = np.frombuffer(bytes([K.SENT]) * (4 * 72), K.TRAJECTORY_RECORD_DTYPE)
    for f, (mode, F) in enumerate(zip(CHAIN_MODES, frames)):
        pred, status = TR.predict(trk, mode, kf)
        assert [status] == H(F["ps"]).tolist() == [0] and H(F["pred"]).tobytes() == pred.tobytes(), "frame %d: the prediction" % f
        assert H(F["state_mid"]).tobytes() == trk.state().tobytes(), "frame %d: UpdateLastFrame" % f
        r1, kp_point, pc, r3, spread = _frame_references(c, mps, obs, pred)
        assert int(F["nm"][0]) == r1["nmatches"] and np.array_equal(H(F["asg"][0, :n]), r1["assigned"]), "frame %d: the search" % f
        assert np.array_equal(H(F["kpp"][0, :n]), kp_point) and (H(F["kpp"][0, n:]) == -1).all(), "frame %d: the slots" % f
        pose_out = np.frombuffer(H(F["pose_out"]).tobytes(), K.KF_POSE_DTYPE)[0]
        got = PC.result_of(pose_out, H(F["outl"][0, :n]), H(F["kpo"][0, :n]), F["nmap"][0], H(F["chi"][0, :n]), H(F["info"][0]), F["ninl"][0])
        d = PC.differences(pc, r3, got, spread)
        assert not d, "frame %d: the pose optimisation differs from the reference: %s" % (f, d)
        assert TR.commit(trk, pose_out, 1, 0, 10.0 + f / 30.0, f, kf, 4) == 0 and H(F["cs"]).tolist() == [0]
        assert H(F["state"]).tobytes() == trk.state().tobytes() and H(F["traj"]).tobytes() == trk.records(4, fill).tobytes(), "frame %d: the commit" % f
        assert np.frombuffer(H(F["count"]).tobytes(), np.int32).tolist() == [f + 1]
    assert trk.has_velocity and r1["nmatches"] >= 20


CULL_SEEDS = (5, 7, 13, 25)          # worlds of tests/cull_cases.py whose culling takes 1, 2, 3 and 2 key frames; 5 starts with a bad one


def _cull_world_with_poses(seed):
    """a seeded world of tests/cull_cases.py, what its key-frame culling leaves, poses for its key frames and 40 records over them"""
    import cull_cases as CK
    c = CK.random_world(seed)
    e = CK.expected_kf(c)
    nkf = c.w.nkf
    rng = np.random.default_rng(seed)
    pose = K.stack([K.make_pose(K.rot(rng.normal(size=3), rng.uniform(-40, 40)), rng.normal(0, 1, 3)) for _ in range(nkf)], K.KF_POSE_DTYPE)
    traj = K.stack([K.record(K.rows(K.rot(rng.normal(size=3), rng.uniform(-20, 20)), rng.normal(0, 0.1, 3)), int(rng.integers(0, nkf)), 5.0 + i / 30.0, i,
                             lost=int(i % 9 == 4)) for i in range(40)], K.TRAJECTORY_RECORD_DTYPE)
    tcp0 = K.frozen_tcp(pose, e["inputs"]["parent"], e["inputs"]["kf_bad"])            # the key frames that were bad before this culling
    return c, e, pose, traj, tcp0


def test_cull_worlds_of_the_chain_cull_key_frames():
    culled = []
    for seed in CULL_SEEDS:
        c, e, pose, traj, tcp0 = _cull_world_with_poses(seed)
        rec = e["record"][:e["info"][1]]
        culled.append([int(r[0]) for r in rec if r[3] == TR.CULLED])
        tcp, info = TR.keyframe_tcp(pose, e["parent"], e["record"], e["info"][1], tcp0)
        assert info[1] == len(culled[-1]) and info[2] == 0
        w = dict(name="cull", pose=pose, kf_bad=e["kf_bad"][:c.w.nkf], parent=e["parent"][:c.w.nkf], kf_id=np.arange(c.w.nkf).astype(np.uint64), tcp=tcp, traj=traj)
        assert any(TR.chain_depth(w, i) >= 1 for i in range(40) if not traj[i]["lost"]), seed
        assert TR.get_trajectory(w)["info"][3] == 40
    assert [len(x) for x in culled] == [1, 2, 3, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", CULL_SEEDS)
def test_gpu_chain_culling_tcp_and_trajectory_on_resident_arrays(ext, seed):
    """pgorb_keyframe_culling_device -> pgorb_keyframe_tcp_device -> pgorb_get_trajectory_device on a world of tests/cull_cases.py with
    poses attached: the record, the info, the parents and the bad flags are read where the culling left them, nothing downloaded in
    between, against the same chain of references"""
    import torch
    import cull_cases as CK
    c, e, pose, traj, tcp0 = _cull_world_with_poses(seed)
    nkf, q, s = c.w.nkf, K._q, torch.cuda.current_stream()
    d = CK.run_device_kf(c, ext, e)
    dpose, dtcp, dinfo = K._up(pose), K._up(tcp0), K._sent(16)
    assert ext._L.pgorb_keyframe_tcp_device(ext._h, nkf, q(dpose), q(d["parent"]), e["list_cap"], q(d["record"]), q(d["info"]), q(dtcp), q(dinfo),
                                            C.c_void_p(s.cuda_stream)) == 0
    ids = np.arange(nkf).astype(np.uint64)
    O = dict(quat_wxyz=K._sent(40 * 32), translation=K._sent(40 * 24), time_usec=K._sent(40 * 8), frame_id=K._sent(40 * 8), is_lost=K._sent(40),
             status=K._sent(40 * 4), info=K._sent(16))
    dids, dtraj = K._up(ids), K._up(traj)
    assert ext._L.pgorb_get_trajectory_device(ext._h, nkf, q(dpose), q(d["kf_bad"]), q(d["parent"]), q(dids), q(dtcp), 40, q(dtraj), None, q(O["quat_wxyz"]),
                                              q(O["translation"]), q(O["time_usec"]), q(O["frame_id"]), q(O["is_lost"]), q(O["status"]), q(O["info"]),
                                              C.c_void_p(s.cuda_stream)) == 0
    s.synchronize()
    got_cull = CK.download_kf(d, e)
    assert CK.same(got_cull, e, ("record", "info", "parent", "kf_bad")), CK.diff(got_cull, e, ("record", "info", "parent", "kf_bad"))
    tcp, info = TR.keyframe_tcp(pose, e["parent"], e["record"], e["info"][1], tcp0)
    assert dtcp.cpu().numpy().tobytes() == tcp.tobytes() and np.frombuffer(dinfo.cpu().numpy().tobytes(), np.int32).tolist() == info.tolist()
    w = dict(name="cull", pose=pose, kf_bad=e["kf_bad"][:nkf], parent=e["parent"][:nkf], kf_id=ids, tcp=tcp, traj=traj)      # the arrays of tests/cull_cases.py are padded
    assert K.same(K.download_trajectory(O, 40), TR.get_trajectory(w))


@pytest.mark.gpu
def test_gpu_chain_commit_tcp_and_trajectory_on_resident_arrays(ext):
    """commit -> (a culling's record) -> pgorb_keyframe_tcp_device -> pgorb_get_trajectory_device with d_count = the tracker's
    d_ntrajectory entry, nothing downloaded in between: the records the commits wrote and the mTcp rows the tcp call froze are read
    where they lie, against the same chain of references"""
    import torch
    q, s = K._q, torch.cuda.current_stream()
    state, frames = K.track_sequences()
    kf = frames[0]["kf"]
    S, T, N = K._up(state), K._sent(2 * K.CAP * 72), K._up(np.zeros(2, np.int32))
    trk = [TR.Tracker(state[t], cap=K.CAP) for t in range(2)]
    dkf, cs = K._up(kf), K._sent(8)
    refs = ((0, 1), (2, 3), (3, 3), (1, 2))
    for f, fr in enumerate(frames[:4]):
        x = fr["trackers"]
        pose, ok, rk = K._up(K.stack([v["pose"] for v in x], K.KF_POSE_DTYPE)), K._up(np.array([v["ok"] for v in x], np.uint8)), K._up(np.array(refs[f], np.int32))
        tm, ids = K._up(np.array([v["time"] for v in x], f64)), K._up(np.array([v["id"] for v in x], np.int64))
        assert ext._L.pgorb_track_commit_batch_device(ext._h, 2, q(S), q(pose), q(ok), q(rk), q(tm), q(ids), 4, q(dkf), q(T), K.CAP, q(N), q(cs),
                                                      C.c_void_p(s.cuda_stream)) == 0
        for t in range(2):
            assert TR.commit(trk[t], x[t]["pose"], x[t]["ok"], refs[f][t], x[t]["time"], x[t]["id"], kf, K.CAP) == 0
    # key frames 3 and 2 are culled (3 under 2, 2 under 1), as a key-frame culling would have recorded them
    parent, bad = np.array([-1, 0, 1, 2], np.int32), np.array([0, 0, 1, 1], np.uint8)
    rec = np.array([[3, 30, 29, TR.CULLED], [1, 30, 2, 0], [2, 25, 25, TR.CULLED]], np.int32)
    dtcp, dinfo = K._sent(4 * 48), K._sent(16)
    assert ext._L.pgorb_keyframe_tcp_device(ext._h, 4, q(dkf), q(K._up(parent)), 3, q(K._up(rec)), q(K._up(np.array([0, 3, 2, 0], np.int32))), q(dtcp), q(dinfo),
                                            C.c_void_p(s.cuda_stream)) == 0
    fill = np.frombuffer(bytes([K.SENT]) * (4 * 48), f32).reshape(4, 12)
    tcp, _ = TR.keyframe_tcp(kf, parent, rec, 3, fill)
    D = dict(pose=dkf, bad=K._up(bad), par=K._up(parent), ids=K._up(np.array([10, 11, 12, 13], np.uint64)), tcp=dtcp)
    for t in range(2):
        O = dict(quat_wxyz=K._sent(K.CAP * 32), translation=K._sent(K.CAP * 24), time_usec=K._sent(K.CAP * 8), frame_id=K._sent(K.CAP * 8),
                 is_lost=K._sent(K.CAP), status=K._sent(K.CAP * 4), info=K._sent(16))
        assert ext._L.pgorb_get_trajectory_device(
            ext._h, 4, q(D["pose"]), q(D["bad"]), q(D["par"]), q(D["ids"]), q(D["tcp"]), K.CAP, C.c_void_p(T.data_ptr() + t * K.CAP * 72),
            C.c_void_p(N.data_ptr() + 4 * t), q(O["quat_wxyz"]), q(O["translation"]), q(O["time_usec"]), q(O["frame_id"]), q(O["is_lost"]), q(O["status"]),
            q(O["info"]), C.c_void_p(s.cuda_stream)) == 0
        s.synchronize()
        c = dict(name="resident", pose=kf, kf_bad=bad, parent=parent, kf_id=np.array([10, 11, 12, 13], np.uint64), tcp=tcp, traj=trk[t].records())
        e = TR.get_trajectory(c)
        assert len(c["traj"]) == 4 and (e["status"] == 0).all()
        assert K.same(K.download_trajectory(O, K.CAP), K.padded(e, K.CAP)), t
