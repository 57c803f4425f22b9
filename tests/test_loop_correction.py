"""Loop correction on the GPU (pilotguru_amd/csrc/loop_correct.hip; include/pgorb.h: CorrectLoop's propagation, LoopClosing.cc:438-516,
and the map update after global bundle adjustment, :679-742) against the literal object-level reference
(tests/loop_correct_reference.py) on constructed cases, 300 seeded random worlds and two large cases (tests/loop_correct_cases.py).
The library is built with -ffp-contract=off and these paths use + - x / and correctly rounded square roots only, so every comparison
is exact, untouched bytes included (the outputs start as a sentinel).

The CPU tests check presence (they fail without the four symbols), what every rule mutant changes on the case named for it, the
branches of Quaterniond(R) the constructed cases take, the reference's coverage of the random worlds, the restatement the kernels
use against the literal sequences, and the refusals of the Python and C++ mirrors.  The GPU tests compare the device forms and
the single calls with the reference and with each other byte for byte, chain into and out of the existing entry points, and
repeat."""
import ctypes as C
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_correct_cases as K  # noqa: E402
import loop_correct_reference as LR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pgorb_correct_loop_poses", "pgorb_correct_loop_poses_device", "pgorb_global_ba_map_update", "pgorb_global_ba_map_update_device")
NRANDOM = 300
f32 = np.float32


def by_name(cases, name):
    return next(c for c in cases if c["name"] == name)


@pytest.fixture(scope="module")
def loops():
    """(case, what the reference leaves), computed once"""
    return [(c, LR.correct_loop(c)) for c in K.loop_cases()]


@pytest.fixture(scope="module")
def maps():
    return [(c, LR.update_map(c)) for c in K.map_cases()]


@pytest.fixture(scope="module")
def randoms():
    out = []
    for s in range(NRANDOM):
        lc, mc = K.random_world(s)
        out.append((lc, LR.correct_loop(lc), mc, LR.update_map(mc)))
    return out


@pytest.fixture(scope="module")
def large():
    a, b = K.claim64x256(), K.chain300()
    return a, LR.correct_loop(a), b, LR.update_map(b)


# ---------------------------------------------------------------- CPU
def test_symbols_constants_mirrors_and_null_context():
    from pilotguru_amd import _lib
    import pilotguru_amd as pg
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name)
    p = None
    assert L.pgorb_correct_loop_poses(p, 0, p, p, p, 0, p, 0, p, p, p, 0, *([p] * 15)) == -1
    assert L.pgorb_correct_loop_poses_device(p, p, p, 0, 1, p, 0, p, 0, p, p, p, p, 0, *([p] * 5), 0, *([p] * 11)) == -1
    assert L.pgorb_global_ba_map_update(p, 0, *([p] * 6), 0, *([p] * 9)) == -1
    assert L.pgorb_global_ba_map_update_device(p, 0, *([p] * 6), 0, *([p] * 10)) == -1
    hdr = open(os.path.join(ROOT, "include", "pgorb.h")).read()
    defs = dict(re.findall(r"#define\s+PGORB_((?:LC|MU)_\w+)\s+(\d+)", hdr))
    assert len(defs) == 4
    for k, v in defs.items():
        assert getattr(pg, k) == int(v), k
    assert (int(defs["LC_OVER_OBS"]), int(defs["LC_BAD_INDEX"]), int(defs["LC_INFO"]), int(defs["MU_INFO"])) == \
        (LR.OVER_OBS, LR.BAD_INDEX, LR.LC_INFO, LR.MU_INFO)
    assert int(re.search(r"#define\s+PGORB_MP_MAX_OBS\s+(\d+)", hdr).group(1)) == LR.MAX_OBS
    for fn in ("CorrectLoopPoses", "CorrectLoopPoses_device", "UpdateMapAfterGBA", "UpdateMapAfterGBA_device"):
        assert callable(getattr(pg.LoopClosing, fn))
    hpp = open(os.path.join(ROOT, "pilotguru_amd", "host", "orb_extractor.hpp")).read()
    assert "class LoopClosing" in hpp and "pgorb_correct_loop_poses(" in hpp and "pgorb_global_ba_map_update(" in hpp


LOOP_NAMED = (("claim_index_order", "address_vs_index"), ("corrected_twice", "address_vs_index"), ("t_not_divided_by_s", "scale_half"),
              ("t_not_divided_by_s", "scale_two"), ("cur_composed", "unnormalised_scw"), ("all_centres_corrected", "address_vs_index"),
              ("own_centre_corrected", "address_vs_index"), ("all_centres_as_passed", "inconsistent_slots"))
MAP_NAMED = (("done_child_recomputed", "chain"), ("regrouped", "chain"), ("parent_pose_after", "chain"), ("ref_not_visited_moved", "bad_in_chain"),
             ("done_point_transformed", "chain"))


def test_every_mutant_is_caught_by_name(loops, maps):
    caught = {}
    loop_names, map_names = {n for n, _ in LOOP_NAMED}, {n for n, _ in MAP_NAMED}
    assert loop_names | map_names == set(LR.MUTANTS) and not loop_names & map_names
    for name, rules in LR.MUTANTS.items():
        if name in loop_names:
            caught[name] = [c["name"] for c, e in loops if not K.same(LR.correct_loop(c, rules), e, K.LOOP_KEYS)]
        else:
            caught[name] = [c["name"] for c, e in maps if not K.same(LR.update_map(c, rules), e, K.MAP_KEYS)]
    for name, where in LOOP_NAMED + MAP_NAMED:
        assert where in caught[name], (name, caught[name])
    # every mutant stands for one field of Rules
    changed = {tuple(f.name for f in dataclasses.fields(LR.Rules) if getattr(r, f.name) != getattr(LR.REFERENCE, f.name)) for r in LR.MUTANTS.values()}
    assert all(len(c) == 1 for c in changed) and {c[0] for c in changed} == {f.name for f in dataclasses.fields(LR.Rules)}
    # the index-order case has nothing the address order could change, and a consistent map needs no corrected centre
    assert "index_order" not in caught["claim_index_order"] and caught["all_centres_as_passed"] == ["inconsistent_slots"]


def test_hand_written_expectations(loops, maps):
    c, e = next(x for x in loops if x[0]["name"] == "address_vs_index")
    # rank(3) = 0 < rank(4) = 1 < rank(1) = 3 < rank(2) = 5: point 0 {1, 3} -> 3, point 1 {1, 2, 3} -> 3, point 3 {2} -> 2, point 4 {4, 1} -> 4;
    # point 2 is held by no member and keeps GetReferenceKeyFrame(); point 5 is bad
    assert list(e["corrected_by"]) == [3, 3, -1, 2, 4, -1] and list(e["point_ref_kf"]) == [3, 3, 0, 2, 4, 3]
    assert list(e["has_corrected"]) == [0, 1, 1, 1, 1, 0] and list(e["info"]) == [0, 4, 4, 0]
    assert e["corrected"][2].tobytes() == c["scw"].tobytes()                      # byte for byte
    assert e["pose_out"][0].tobytes() == c["pose"][0].tobytes() and e["points"][2].tobytes() == c["points"][2].tobytes()
    assert e["points"][5].tobytes() == c["points"][5].tobytes()
    for k in ("fx", "fy", "cx", "cy", "invfx", "invfy"):
        assert e["pose_out"][k].tobytes() == c["pose"][k].tobytes()
    c, e = next(x for x in loops if x[0]["name"] == "padded_row")
    assert list(e["has_corrected"]) == [0, 1, 1, 1, 0, 0] and e["info"][1] == 3
    c, e = next(x for x in loops if x[0]["name"] == "over_max_obs")
    assert list(e["info"]) == [LR.OVER_OBS, 4, 2, 1] and e["points"][0]["pos"].tobytes() != c["points"][0]["pos"].tobytes()
    assert e["points"][0]["normal"].tobytes() == c["points"][0]["normal"].tobytes() and e["points"][0]["max_distance"] == c["points"][0]["max_distance"]
    c, e = next(x for x in loops if x[0]["name"] == "inconsistent_slots")
    assert list(e["corrected_by"]) == [5, 5, 0, 3] and e["points"][1]["normal"].tobytes() == c["points"][1]["normal"].tobytes()
    c, e = next(x for x in maps if x[0]["name"] == "chain")
    assert list(e["kf_updated"]) == [1, 1, 1, 1, 1, 0, 0] and list(e["info"][:3]) == [0, 5, 3]
    assert e["pose_out"][3].tobytes() == c["pose_gba"][3].tobytes() and e["pose_out"][5].tobytes() == c["pose"][5].tobytes()
    c, e = next(x for x in maps if x[0]["name"] == "origin_not_done")
    assert list(e["kf_updated"]) == [0, 0, 1, 1, 0]
    c, e = next(x for x in maps if x[0]["name"] == "bad_in_chain")
    assert list(e["kf_updated"]) == [1, 1, 0, 0, 0, 1, 1]
    c, e = next(x for x in maps if x[0]["name"] == "cycle")
    assert list(e["kf_updated"]) == [1, 1, 0, 0, 0, 0]


def test_constructed_cases_take_every_branch_of_the_quaternion(loops):
    hits = {}
    for c, _ in loops:
        LR.correct_loop(c, hits=hits)
    for k in ("quat_trace", "quat_x", "quat_y", "quat_z", "already_corrected"):
        assert hits.get(k, 0) > 0, (k, hits)
    # ... and the relative rotations Tic of the half-turn case take the three non-trace branches too
    c = by_name([c for c, _ in loops], "half_turns")
    Twc = LR.pose_inverse(c["pose"][0]["Tcw"], c["pose"][0]["Ow"])
    assert [LR.quat_branch(LR.mul44(LR.mat44(c["pose"][f]["Tcw"]), Twc)[:3, :3].astype(np.float64)) for f in (1, 2, 3)] == ["x", "y", "z"]


def test_random_worlds_cover_what_they_are_for(randoms):
    n = len(randoms)
    assert n == NRANDOM
    assert all(4 <= lc["nkf"] <= 12 and max(len(s) for s in lc["kf_point"]) <= 16 and lc["npoints"] <= 48 for lc, _, _, _ in randoms)
    facts = [K.world_facts(lc, mc, el, em) for lc, el, mc, em in randoms]
    assert sum(f["first_not_index"] for f in facts) >= 0.25 * n
    assert sum(f["chain2"] for f in facts) >= 0.10 * n
    assert sum(f["not_visited"] for f in facts) >= 0.10 * n
    assert sum(f["ref_both"] for f in facts) >= 0.10 * n


def test_restatement_equals_the_literal_sequences(loops, maps, randoms):
    for c, e in loops + [(lc, el) for lc, el, _, _ in randoms]:
        got = LR.correct_loop_claims(c)
        assert K.same(got, e, K.LOOP_KEYS), (c["name"], K.diff(got, e, K.LOOP_KEYS))
    for c, e in maps + [(mc, em) for _, _, mc, em in randoms]:
        got = LR.update_map_chains(c)
        assert K.same(got, e, K.MAP_KEYS), (c["name"], K.diff(got, e, K.MAP_KEYS))


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


def _py_loop(pg, c, ext, **kw):
    v = dict(octaves=c["octaves"], pose=c["pose"], cur=c["cur_kf"], scw=c["scw"], lst=c["list"], slots=c["kf_point"], pts=c["points"],
             st=c["obs_start"], of=c["obs_frame"], oi=c["obs_idx"], ro=c["ref_obs"], rk=c["ref_kf"], pb=c["point_bad"], order=c["kf_order"])
    v.update(kw)
    return pg.LoopClosing.CorrectLoopPoses(ext, v["octaves"], v["pose"], v["cur"], v["scw"], v["lst"], v["slots"], v["pts"], v["st"], v["of"], v["oi"],
                                           v["ro"], v["rk"], v["pb"], v["order"])


def _py_map(pg, c, ext, **kw):
    v = dict(pose=c["pose"], gba=c["pose_gba"], kd=c["kf_done"], par=c["parent"], org=c["kf_origin"], pts=c["points"], pgba=c["pos_gba"],
             pd=c["point_done"], rk=c["ref_kf"], kb=c["kf_bad"], pb=c["point_bad"])
    v.update(kw)
    return pg.LoopClosing.UpdateMapAfterGBA(ext, v["pose"], v["gba"], v["kd"], v["par"], v["org"], v["pts"], v["pgba"], v["pd"], v["rk"], v["kb"], v["pb"])


def _bad_loop_inputs(c):
    nan_pose, inf_ow, nan_pt = c["pose"].copy(), c["pose"].copy(), c["points"].copy()
    nan_pose["Tcw"][1, 5] = np.nan
    inf_ow["Ow"][0, 2] = np.inf
    nan_pt["pos"][0, 1] = np.nan
    s_nan, s_zero, s_neg = c["scw"].copy(), c["scw"].copy(), c["scw"].copy()
    s_nan["t"][1], s_zero["s"], s_neg["s"] = np.nan, 0.0, -1.0
    start0, down, twice, far, nokf = c["obs_start"].copy(), c["obs_start"].copy(), c["obs_frame"].copy(), c["obs_idx"].copy(), c["obs_frame"].copy()
    start0[0], down[2], twice[1], far[0], nokf[0] = 1, down[1] - 1, twice[0], 99, c["nkf"]
    ro, rk = c["ref_obs"].copy(), c["ref_kf"].copy()
    ro[0], rk[1] = 7, c["nkf"]
    slot = [s.copy() for s in c["kf_point"]]
    slot[1][0] = c["npoints"]
    return (dict(cur=-1), dict(cur=c["nkf"]), dict(pose=nan_pose), dict(pose=inf_ow), dict(pts=nan_pt), dict(scw=s_nan), dict(scw=s_zero),
            dict(scw=s_neg), dict(st=start0), dict(st=down), dict(of=twice), dict(oi=far), dict(of=nokf), dict(ro=ro), dict(rk=rk),
            dict(slots=slot), dict(order=[0] * c["nkf"]), dict(octaves=c["octaves"][1:] + c["octaves"][:1]))


def _bad_map_inputs(c):
    nan_pose, nan_gba, nan_pt, nan_pg = c["pose"].copy(), c["pose_gba"].copy(), c["points"].copy(), c["pos_gba"].copy()
    nan_pose["Ow"][2, 0] = np.nan
    nan_gba["Tcw"][0, 3] = np.inf                                    # key frame 0 is done: its result is read
    nan_pt["pos"][1, 2] = np.nan
    nan_pg[0, 0] = np.nan                                            # point 0 is done
    par_hi, par_lo, cyc, rk = c["parent"].copy(), c["parent"].copy(), c["parent"].copy(), c["ref_kf"].copy()
    par_hi[1], par_lo[1], rk[0] = c["nkf"], -2, c["nkf"]
    cyc[1], cyc[2] = 2, 1
    return (dict(pose=nan_pose), dict(gba=nan_gba), dict(pts=nan_pt), dict(pgba=nan_pg), dict(par=par_hi), dict(par=par_lo), dict(par=cyc), dict(rk=rk),
            dict(kd=c["kf_done"][1:]), dict(pd=c["point_done"][1:]))


def test_python_mirrors_refuse_malformed_input_without_a_device(loops, maps):
    import pilotguru_amd as pg
    c = by_name([c for c, _ in loops], "address_vs_index")
    for kw in _bad_loop_inputs(c):
        with pytest.raises(ValueError):
            _py_loop(pg, c, _NoLibrary(), **kw)
    with pytest.raises(AssertionError, match="the library was called"):
        _py_loop(pg, c, _NoLibrary())
    c = by_name([c for c, _ in maps], "chain")
    for kw in _bad_map_inputs(c):
        with pytest.raises(ValueError):
            _py_map(pg, c, _NoLibrary(), **kw)
    with pytest.raises(AssertionError, match="the library was called"):
        _py_map(pg, c, _NoLibrary())


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
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // three key frames, two points: point 0 seen by 0 and 1, point 1 by 1 and 2
    std::vector<std::vector<int32_t>> slots = {{0, -1}, {0, 1}, {1}}, octaves = {{0, 0}, {0, 1}, {2}};
    MapPointObservations obs;
    obs.obsStart = {0, 2, 4};
    obs.obsFrame = {0, 1, 1, 2};
    obs.obsIdx = {0, 0, 1, 0};
    obs.refObs = {0, 1};
    pgorb_sim3d scw{};
    scw.r[3] = 1.0; scw.s = 1.5;
    LoopClosing lc(nullptr);
    auto loop = [&](std::vector<std::vector<int32_t>> s, std::vector<std::vector<int32_t>> o, MapPointObservations ob, int cur, pgorb_sim3d S,
                    std::vector<pgorb_kf_pose> poses, float x, std::vector<int32_t> refKf, std::vector<int32_t> order) {
        std::vector<pgorb_map_point> pts(2);
        pts[0].pos[0] = x;
        LoopCorrection out;
        lc.CorrectLoopPoses(o, poses, cur, S, {0, 1, -1}, s, pts, {}, ob, refKf, order, out);
    };
    const std::vector<pgorb_kf_pose> P(3, ident());
    std::vector<pgorb_kf_pose> Pnan = P;
    Pnan[1].Ow[2] = nan;
    pgorb_sim3d s0 = scw, snan = scw;
    s0.s = 0.0; snan.t[0] = nan;
    MapPointObservations twice = obs; twice.obsFrame = {0, 0, 1, 2};
    MapPointObservations idx = obs; idx.obsIdx = {0, 0, 2, 0};
    MapPointObservations ref = obs; ref.refObs = {0, 2};
    run("lc_well_formed", [&] { loop(slots, octaves, obs, 2, scw, P, 0.5f, {0, 2}, {}); });
    run("lc_cur", [&] { loop(slots, octaves, obs, 3, scw, P, 0.5f, {0, 2}, {}); });
    run("lc_slot", [&] { loop({{2}, {0, 1}, {1}}, octaves, obs, 2, scw, P, 0.5f, {0, 2}, {}); });
    run("lc_octaves", [&] { loop(slots, {{0}, {0, 1}, {2}}, obs, 2, scw, P, 0.5f, {0, 2}, {}); });
    run("lc_scale", [&] { loop(slots, octaves, obs, 2, s0, P, 0.5f, {0, 2}, {}); });
    run("lc_scw", [&] { loop(slots, octaves, obs, 2, snan, P, 0.5f, {0, 2}, {}); });
    run("lc_pose", [&] { loop(slots, octaves, obs, 2, scw, Pnan, 0.5f, {0, 2}, {}); });
    run("lc_point", [&] { loop(slots, octaves, obs, 2, scw, P, nan, {0, 2}, {}); });
    run("lc_obs_twice", [&] { loop(slots, octaves, twice, 2, scw, P, 0.5f, {0, 2}, {}); });
    run("lc_obs_idx", [&] { loop(slots, octaves, idx, 2, scw, P, 0.5f, {0, 2}, {}); });
    run("lc_ref_obs", [&] { loop(slots, octaves, ref, 2, scw, P, 0.5f, {0, 2}, {}); });
    run("lc_ref_kf", [&] { loop(slots, octaves, obs, 2, scw, P, 0.5f, {0, 3}, {}); });
    run("lc_order", [&] { loop(slots, octaves, obs, 2, scw, P, 0.5f, {0, 2}, {0, 0, 1}); });
    auto upd = [&](std::vector<int32_t> parent, std::vector<pgorb_kf_pose> gba, std::vector<uint8_t> done, std::vector<float> posGba,
                   std::vector<int32_t> refKf) {
        std::vector<pgorb_map_point> pts(2);
        MapUpdate out;
        lc.UpdateMapAfterGBA(P, gba, done, parent, {1, 0, 0}, {}, pts, posGba, {1, 0}, {}, refKf, out);
    };
    const std::vector<float> pg(6, 0.25f);
    std::vector<float> pgnan = pg;
    pgnan[1] = nan;
    run("mu_well_formed", [&] { upd({-1, 0, 1}, P, {1, 0, 0}, pg, {0, 2}); });
    run("mu_parent", [&] { upd({-1, 3, 1}, P, {1, 0, 0}, pg, {0, 2}); });
    run("mu_cycle", [&] { upd({-1, 2, 1}, P, {1, 0, 0}, pg, {0, 2}); });
    run("mu_self", [&] { upd({-1, 0, 2}, P, {1, 0, 0}, pg, {0, 2}); });
    run("mu_gba", [&] { upd({-1, 0, 1}, Pnan, {1, 1, 0}, pg, {0, 2}); });
    run("mu_done", [&] { upd({-1, 0, 1}, P, {1, 0}, pg, {0, 2}); });
    run("mu_pos_gba", [&] { upd({-1, 0, 1}, P, {1, 0, 0}, pgnan, {0, 2}); });
    run("mu_ref_kf", [&] { upd({-1, 0, 1}, P, {1, 0, 0}, pg, {0, -2}); });
    return 0;
}
"""


def test_cpp_mirror_rejects_bad_inputs_before_calling_the_library(tmp_path):
    """pgorb::LoopClosing throws std::invalid_argument for what the single calls would refuse, before any pointer reaches the
    library; well-formed input reaches it (a NULL context here, so PGORB_E_ARG comes back as std::runtime_error)."""
    import subprocess
    src, exe = os.path.join(str(tmp_path), "loop_driver.cc"), os.path.join(str(tmp_path), "loop_driver")
    open(src, "w").write(CPP_DRIVER)
    lib = os.path.join(ROOT, "pilotguru_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", ROOT, src, "-o", exe, "-L", lib, "-lpgorb", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    got = dict(l.split() for l in subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines())
    assert got.pop("lc_well_formed") == "runtime_error" and got.pop("mu_well_formed") == "runtime_error", got
    assert len(got) == 19 and set(got.values()) == {"invalid_argument"}, got


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    return pg.ORBextractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240)


def _check_loop(c, e, ext, host=True):
    got, _ = K.run_device_loop(c, ext)
    assert K.same(got, e, K.LOOP_KEYS), (c["name"], "device", K.diff(got, e, K.LOOP_KEYS))
    if host:
        h = K.run_host_loop(c, ext)
        assert h["ret"] == e["info"][2], (c["name"], h["ret"])
        assert K.same(h, e, K.LOOP_KEYS), (c["name"], "host", K.diff(h, e, K.LOOP_KEYS))
        assert K.same(h, got, K.LOOP_KEYS), (c["name"], "host != device")


def _check_map(c, e, ext, host=True):
    got, _ = K.run_device_map(c, ext)
    assert K.same(got, e, K.MAP_KEYS), (c["name"], "device", K.diff(got, e, K.MAP_KEYS))
    if host and not c.get("device_only"):
        h = K.run_host_map(c, ext)
        assert h["ret"] == e["info"][1], (c["name"], h["ret"])
        assert K.same(h, e, K.MAP_KEYS), (c["name"], "host", K.diff(h, e, K.MAP_KEYS))
        assert K.same(h, got, K.MAP_KEYS), (c["name"], "host != device")


@pytest.mark.gpu
def test_gpu_constructed_cases_equal_the_reference_in_both_forms(ext, loops, maps):
    """the padded-row list, the inconsistent slots, the point over PGORB_MP_MAX_OBS and the scales 0.5 and 2 among them"""
    assert np.array_equal(np.asarray(ext.GetScaleFactors(), f32)[:8], np.asarray(LR.SF, f32)[:8])
    for c, e in loops:
        _check_loop(c, e, ext)
    for c, e in maps:
        _check_map(c, e, ext)


@pytest.mark.gpu
def test_gpu_random_worlds_equal_the_reference(ext, randoms):
    for i, (lc, el, mc, em) in enumerate(randoms):
        _check_loop(lc, el, ext, host=i % 10 == 7)
        _check_map(mc, em, ext, host=i % 10 == 7)


@pytest.mark.gpu
def test_gpu_large_cases_equal_the_reference(ext, large):
    """64 members x 256 slots with every point shared, for the claim; a chain of 300 key frames under one adjusted origin"""
    a, ea, b, eb = large
    assert ea["info"][1] == 64 and ea["info"][2] == a["npoints"] == 2048 and list(eb["info"]) == [0, 301, 300, 4000]
    _check_loop(a, ea, ext)
    _check_map(b, eb, ext)


@pytest.mark.gpu
def test_gpu_list_count_cuts_a_row_with_stale_entries(ext, loops):
    """a row of ord_kf passed with its capacity: what lies behind the row's count is not read as a member"""
    import torch
    c, e = next(x for x in loops if x[0]["name"] == "address_vs_index")
    stale = dict(c, list=np.array(list(c["list"]) + [0, 5], np.int32))
    cnt = torch.tensor([len(c["list"])], dtype=torch.int32, device="cuda")
    got, _ = K.run_device_loop(stale, ext, list_count=cnt)
    assert K.same(got, e, K.LOOP_KEYS), K.diff(got, e, K.LOOP_KEYS)
    got, _ = K.run_device_loop(stale, ext)
    assert got["info"][1] == e["info"][1] + 2


@pytest.mark.gpu
def test_gpu_device_form_out_of_range_entries_are_nothing(ext, loops):
    """an observation outside the batch and a ref_obs outside its list leave the point's normal and distances alone
    (PGORB_LC_BAD_INDEX); a slot out of range is no slot; a rank named twice makes the smaller index no key frame"""
    c, e = next(x for x in loops if x[0]["name"] == "address_vs_index")
    broken = dict(c, obs_frame=c["obs_frame"].copy(), ref_obs=c["ref_obs"].copy(), kf_point=[s.copy() for s in c["kf_point"]])
    broken["obs_frame"][0] = c["nkf"] + 3                            # point 0
    broken["ref_obs"][1] = 9                                         # point 1
    broken["kf_point"][2][list(c["kf_point"][2]).index(3)] = c["npoints"] + 5      # the only slot that holds point 3
    got, _ = K.run_device_loop(broken, ext)
    assert got["info"][0] == LR.BAD_INDEX and list(got["corrected_by"]) == [3, 3, -1, -1, 4, -1]
    for p in (0, 1):
        assert got["points"][p]["pos"].tobytes() == e["points"][p]["pos"].tobytes()
        assert got["points"][p]["normal"].tobytes() == c["points"][p]["normal"].tobytes()
        assert got["points"][p]["min_distance"] == c["points"][p]["min_distance"]
    assert got["points"][4].tobytes() == e["points"][4].tobytes() and got["points"][3].tobytes() == c["points"][3].tobytes()
    order = c["kf_order"].copy()
    order[1] = order[3]                                              # key frames 1 and 3 claim one rank: 3 keeps it
    got, _ = K.run_device_loop(dict(c, kf_order=order), ext)
    assert list(got["has_corrected"]) == [0, 0, 1, 1, 1, 0] and got["info"][1] == 3


@pytest.mark.gpu
def test_gpu_single_calls_refuse_malformed_input(ext, loops, maps):
    from pilotguru_amd import _lib
    c = by_name([c for c, _ in loops], "address_vs_index")
    key = dict(octaves="octaves", pose="pose", cur="cur_kf", scw="scw", slots="kf_point", pts="points", st="obs_start", of="obs_frame", oi="obs_idx",
               ro="ref_obs", rk="ref_kf", order="kf_order")
    for kw in _bad_loop_inputs(c)[:-1]:
        bad = dict(c, **{key[k]: (np.array(v, np.int32) if k == "order" else v) for k, v in kw.items()})
        assert K.run_host_loop(bad, ext)["ret"] == _lib.PGORB_E_ARG, list(kw)
    assert K.run_host_loop(c, ext)["ret"] == 4
    m = by_name([c for c, _ in maps], "chain")
    key = dict(pose="pose", gba="pose_gba", pts="points", pgba="pos_gba", par="parent", rk="ref_kf")
    for kw in _bad_map_inputs(m)[:-2]:
        bad = dict(m, **{key[k]: v for k, v in kw.items()})
        assert K.run_host_map(bad, ext)["ret"] == _lib.PGORB_E_ARG, list(kw)
    assert K.run_host_map(by_name([c for c, _ in maps], "cycle"), ext)["ret"] == _lib.PGORB_E_ARG
    L, h, p = ext._L, ext._h, None
    assert L.pgorb_correct_loop_poses(h, -1, p, p, p, 0, p, 0, p, p, p, 0, *([p] * 15)) == _lib.PGORB_E_ARG
    assert L.pgorb_global_ba_map_update(h, -1, *([p] * 6), 0, *([p] * 9)) == _lib.PGORB_E_ARG
    assert L.pgorb_global_ba_map_update(h, 5000, *([p] * 6), 0, *([p] * 9)) in (_lib.PGORB_E_ARG, _lib.PGORB_E_LIMIT)


@pytest.mark.gpu
def test_gpu_python_mirrors_return_what_the_reference_leaves(ext, loops, maps):
    import pilotguru_amd as pg
    for name in ("address_vs_index", "inconsistent_slots", "padded_row"):
        c, e = next(x for x in loops if x[0]["name"] == name)
        r = _py_loop(pg, c, ext)
        got = dict(r, pose_out=r["poses"])
        assert K.same(got, e, K.LOOP_KEYS), (name, K.diff(got, e, K.LOOP_KEYS))
        assert r["corrected_points"] == e["info"][2] and r["members"] == e["info"][1]
    for name in ("chain", "bad_in_chain"):
        c, e = next(x for x in maps if x[0]["name"] == name)
        r = _py_map(pg, c, ext)
        got = dict(r, pose_out=r["poses"])
        assert K.same(got, e, K.MAP_KEYS), (name, K.diff(got, e, K.MAP_KEYS))


@pytest.mark.gpu
def test_gpu_repeat_second_stream_and_a_used_context_give_the_same_bytes(ext, loops, maps, large):
    import torch
    a, ea, b, eb = large
    for c, e in [x for x in loops if x[0]["name"] in ("address_vs_index", "half_turns")] + [(a, ea)]:
        first, _ = K.run_device_loop(c, ext)
        K.run_device_map(b, ext)                                     # another entry point and another size in the same context
        again, _ = K.run_device_loop(c, ext)
        other, _ = K.run_device_loop(c, ext, stream=torch.cuda.Stream())
        assert K.same(first, again, K.LOOP_KEYS) and K.same(first, other, K.LOOP_KEYS) and K.same(first, e, K.LOOP_KEYS), c["name"]
    for c, e in [x for x in maps if x[0]["name"] in ("chain", "bad_in_chain")] + [(b, eb)]:
        first, _ = K.run_device_map(c, ext)
        K.run_device_loop(loops[0][0], ext)
        again, _ = K.run_device_map(c, ext)
        other, _ = K.run_device_map(c, ext, stream=torch.cuda.Stream())
        assert K.same(first, again, K.MAP_KEYS) and K.same(first, other, K.MAP_KEYS) and K.same(first, e, K.MAP_KEYS), c["name"]


@pytest.mark.gpu
def test_gpu_chain_correction_into_the_essential_graph_on_resident_arrays(ext, loops):
    """correction -> pgorb_optimize_essential_graph_device with the produced Sim3 arrays, d_pose_out and d_point_ref_kf, nothing
    downloaded in between, against the same call fed from arrays the host prepared from the reference"""
    import torch
    import pilotguru_amd as pg
    from pilotguru_amd.orb import KF_POSE_DTYPE, MAP_POINT_DTYPE, SIM3D_DTYPE
    c, e = next(x for x in loops if x[0]["name"] == "address_vs_index")
    nkf, n = c["nkf"], c["npoints"]
    got, D = K.run_device_loop(c, ext)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32).reshape(-1).copy()).cuda()
    up = lambda a: torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).cuda()
    kf_id = torch.arange(nkf, dtype=torch.int64, device="cuda")
    parent = i32([-1, 0, 1, 2, 3, 4])
    loop_conn = i32([[2, 0, 150], [1, 5, 120]])
    les, le = i32([0, 0, 0, 0, 0, 0, 0]), i32([0])[:0]
    cs, cv, cw = i32([0, 1, 2, 3, 3, 3, 3]), i32([1, 2, 0]), i32([130, 140, 110])
    common = dict(loop_kf=0, cur_kf=c["cur_kf"], d_parent=parent, d_loop_conn=loop_conn, d_loop_edge_start=les, d_loop_edge=le, d_covis_start=cs,
                  d_covis=cv, d_covis_weight=cw, npoints=n, iterations=5)
    chained = pg.Optimizer.OptimizeEssentialGraph_device(
        ext, kf_id, D["pose_out"], d_points=D["pts"], d_point_ref_kf=D["point_ref_kf"].view(torch.int32), d_point_bad=D["pb"],
        d_has_corrected=D["has_corrected"], d_corrected=D["corrected"], d_has_non_corrected=D["has_non_corrected"], d_non_corrected=D["non_corrected"],
        **common)
    pts_h = up(e["points"])
    hosted = pg.Optimizer.OptimizeEssentialGraph_device(
        ext, kf_id, up(e["pose_out"]), d_points=pts_h, d_point_ref_kf=i32(e["point_ref_kf"]), d_point_bad=up(c["point_bad"]),
        d_has_corrected=up(e["has_corrected"]), d_corrected=up(e["corrected"]), d_has_non_corrected=up(e["has_non_corrected"]),
        d_non_corrected=up(e["non_corrected"]), **common)
    torch.cuda.synchronize()
    for k in ("pose_out", "sim3_out", "edge_out", "info"):
        assert chained[k].cpu().numpy().tobytes() == hosted[k].cpu().numpy().tobytes(), k
    assert D["pts"].cpu().numpy().tobytes()[:n * MAP_POINT_DTYPE.itemsize] == pts_h.cpu().numpy().tobytes()
    info = chained["info"].cpu().numpy()
    assert info[0] == 0 and info[2] > 0 and info[7] > 0                # the graph was optimised
    assert np.frombuffer(pts_h.cpu().numpy().tobytes(), MAP_POINT_DTYPE)["pos"].tobytes() != e["points"]["pos"].tobytes()
    assert SIM3D_DTYPE.itemsize == 64 and KF_POSE_DTYPE.itemsize == 84


@pytest.mark.gpu
def test_gpu_chain_global_bundle_adjustment_map_update_refresh_on_resident_arrays(ext):
    """pgorb_global_bundle_adjustment_device -> map update -> pgorb_refresh_map_points_batch_device (normal and depth) with nothing
    downloaded in between, against the reference's update of the downloaded adjustment followed by update_normal_and_depth"""
    import torch
    import gba_cases as GC
    import lba_cases as LC
    import map_point_reference as MR
    from pilotguru_amd.orb import KF_POSE_DTYPE, MAP_POINT_DTYPE, MP_NORMAL_DEPTH
    name = "init2"
    P = GC.case(name)[0]
    D = GC.device_arrays(P)
    T, cap = D[0], D[1]
    nf, npts, nobs = P.nframes, len(P.pos), len(P.obs_frame)
    pose_in = np.frombuffer(T["pose"].cpu().numpy().tobytes(), KF_POSE_DTYPE)[:nf].copy()
    r, D, out = GC.run_gpu_device(name, ext, D=D)
    pts_in = np.frombuffer(T["pts"].cpu().numpy().tobytes(), MAP_POINT_DTYPE)[:npts].copy()      # the table as the adjustment left it
    gba = np.frombuffer(out["pose_out"].cpu().numpy().tobytes(), KF_POSE_DTYPE)[:nf].copy()
    kd, pd = out["kf_done"].cpu().numpy()[:nf].copy(), out["point_done"].cpu().numpy()[:npts].copy()
    pos_gba = out["pos_out"].cpu().numpy().reshape(-1, 3)[:npts].copy()
    parent, origin = np.array([-1] + list(range(nf - 1)), np.int32), np.array([1] + [0] * (nf - 1), np.uint8)
    ref_kf = np.array([P.obs_frame[P.obs_start[p]] if P.obs_start[p + 1] > P.obs_start[p] else -1 for p in range(npts)], np.int32)
    q = lambda t: C.c_void_p(t.data_ptr())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_par, d_org, d_rk = dev(parent), dev(origin), dev(ref_kf)
    d_po = torch.full((nf * KF_POSE_DTYPE.itemsize,), K.SENT, dtype=torch.uint8, device="cuda")
    d_ku, d_pu = torch.full((nf,), K.SENT, dtype=torch.uint8, device="cuda"), torch.full((npts,), K.SENT, dtype=torch.uint8, device="cuda")
    d_info = torch.zeros(4, dtype=torch.int32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert ext._L.pgorb_global_ba_map_update_device(ext._h, nf, q(T["pose"]), q(out["pose_out"]), q(out["kf_done"]), q(d_par), q(d_org), q(T["kb"]),
                                                    npts, q(T["pts"]), q(out["pos_out"]), q(out["point_done"]), q(T["pb"]), q(d_rk), q(d_po), q(d_ku),
                                                    q(d_pu), q(d_info), s) == 0
    status = torch.zeros(max(npts, 1), dtype=torch.int32, device="cuda")
    d_desc = torch.zeros((nf, cap, 32), dtype=torch.uint8, device="cuda")
    d_pd = torch.zeros((npts, 32), dtype=torch.uint8, device="cuda")
    d_ref = torch.zeros(npts, dtype=torch.int32, device="cuda")
    ext._check(ext._L.pgorb_refresh_map_points_batch_device(
        ext._h, q(T["kps"]), q(d_desc), q(T["n"]), nf, cap, q(d_po), q(T["kb"]), npts, q(T["pts"]), q(d_pd), q(T["pb"]), q(T["os"]), q(T["of"]),
        q(T["oi"]), nobs, q(d_ref), npts, None, MP_NORMAL_DEPTH, None, q(status), s))
    torch.cuda.synchronize()
    rows = np.frombuffer(T["pts"].cpu().numpy().tobytes(), MAP_POINT_DTYPE)[:npts]
    case = K.map_case("after_gba", pose_in, gba, kd, parent, origin, None, pts_in["pos"], pos_gba, pd, None, ref_kf)
    case["points"] = pts_in
    e = LR.update_map(case)
    assert e["info"][1] == nf and e["point_updated"].any()
    assert np.frombuffer(d_po.cpu().numpy().tobytes(), KF_POSE_DTYPE).tobytes() == e["pose_out"].tobytes()
    assert d_ku.cpu().numpy().tobytes() == e["kf_updated"].tobytes() and d_pu.cpu().numpy().tobytes() == e["point_updated"].tobytes()
    assert rows["pos"].tobytes() == e["points"]["pos"].tobytes()
    sf = np.asarray(ext.GetScaleFactors(), f32)
    kfs = [MR.KeyFrame(LC.keypoints(P.keys_xy[f], P.octaves[f]), np.zeros((len(P.octaves[f]), 32), np.uint8), e["pose_out"][f]["Ow"]) for f in range(nf)]
    checked = 0
    for p in range(npts):
        if P.obs_start[p + 1] == P.obs_start[p]:
            continue
        mp = MR.MapPoint(e["points"][p]["pos"], np.zeros(32, np.uint8))
        mp.obs = [(kfs[P.obs_frame[k]], int(P.obs_idx[k])) for k in range(P.obs_start[p], P.obs_start[p + 1])]
        mp.ref = mp.obs[0][0]
        assert MR.update_normal_and_depth(mp, sf, LC.NLEVELS)
        assert rows["normal"][p].tobytes() == mp.normal.tobytes() and f32(rows["min_distance"][p]) == mp.min_d and \
            f32(rows["max_distance"][p]) == mp.max_d, p
        checked += 1
    assert checked
