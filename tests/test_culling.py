"""Local mapping's two cullings on the GPU (pilotguru_amd/csrc/culling.hip; include/pgorb.h: LocalMapping::MapPointCulling,
LocalMapping::KeyFrameCulling with KeyFrame::SetBadFlag and MapPoint::EraseObservation, and the compaction of the observation lists)
against the literal object-level reference (tests/cull_reference.py) on constructed cases and seeded random worlds
(tests/cull_cases.py).  Integers only: every comparison is exact, untouched bytes included (the outputs start as a sentinel).

The CPU tests check presence (they fail without the five symbols), the reference's coverage of the random worlds, the dirty-set
restatement against the literal sequence, what every rule mutant changes on the case named for it, a few expectations spelled out
as numbers, the numpy compaction against a plain loop, and the refusals of the Python and C++ mirrors.  The GPU tests compare the
device forms and the host forms with the reference and with each other byte for byte."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import covis_cases as CC  # noqa: E402
import cull_cases as K  # noqa: E402
import cull_reference as CU  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pgorb_compact_observations_device", "pgorb_map_point_culling", "pgorb_map_point_culling_device", "pgorb_keyframe_culling",
         "pgorb_keyframe_culling_device")
NRANDOM = 300


@pytest.fixture(scope="module")
def kf_cases():
    return K.kf_cases() + [K.stride_world()]


@pytest.fixture(scope="module")
def mp_cases():
    return K.mp_cases()


@pytest.fixture(scope="module")
def randoms():
    """(case, what the reference leaves), computed once"""
    out = []
    for s in range(NRANDOM):
        c = K.random_world(s)
        out.append((c, K.expected_kf(c)))
    return out


def test_symbols_constants_mirrors_and_null_context():
    from pilotguru_amd import _lib
    import pilotguru_amd as pg
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name)
    p = None
    assert L.pgorb_compact_observations_device(p, 0, p, p, p, 0, *([p] * 8)) == -1
    assert L.pgorb_map_point_culling(p, 0, p, p, 0, *([p] * 8), 0, p, 0, 2, p, p, p, p) == -1
    assert L.pgorb_map_point_culling_device(p, p, p, 0, 1, 0, p, p, p, p, 0, p, p, p, p, 0, p, 0, 2, p, p, p, p, p) == -1
    assert L.pgorb_keyframe_culling(p, 0, p, p, p, 0, *([p] * 11), 0, 1, *([p] * 7), 1, p, p, p) == -1
    assert L.pgorb_keyframe_culling_device(p, p, p, p, 0, 1, 0, p, p, p, p, 0, *([p] * 7), 0, 1, *([p] * 7), 1, p, p, p, p) == -1
    hdr = open(os.path.join(ROOT, "include", "pgorb.h")).read()
    defs = dict(re.findall(r"#define\s+PGORB_(CULL_\w+)\s+(\d+)", hdr))
    assert len(defs) == 17
    for k, v in defs.items():
        assert getattr(pg, k) == int(v), k
    for k, v in (("MP_KEEP", CU.MP_KEEP), ("MP_WAS_BAD", CU.MP_WAS_BAD), ("MP_FOUND_RATIO", CU.MP_FOUND_RATIO), ("MP_FEW_OBS", CU.MP_FEW_OBS),
                 ("MP_AGED", CU.MP_AGED), ("MP_NONE", CU.MP_NONE), ("KF_KEEP", CU.KF_KEEP), ("KF_CULLED", CU.KF_CULLED),
                 ("KF_TO_BE_ERASED", CU.KF_TO_BE_ERASED), ("KF_ID0", CU.KF_ID0), ("KF_WAS_BAD", CU.KF_WAS_BAD), ("KF_NONE", CU.KF_NONE),
                 ("ROW_ERASED", CU.ROW_ERASED), ("ROW_CLEARED", CU.ROW_CLEARED), ("ROW_REPARENTED", CU.ROW_REPARENTED), ("LIMIT", CU.LIMIT),
                 ("INFO", CU.INFO)):
        assert int(defs["CULL_" + k]) == v, k
    assert (int(defs["CULL_MP_KEEP"]), int(defs["CULL_MP_WAS_BAD"]), int(defs["CULL_MP_FOUND_RATIO"]), int(defs["CULL_MP_FEW_OBS"]),
            int(defs["CULL_MP_AGED"]), int(defs["CULL_MP_NONE"])) == (0, 1, 2, 3, 4, 5)
    assert callable(pg.LocalMapping.MapPointCulling) and callable(pg.LocalMapping.KeyFrameCulling) and callable(pg.compact_observations)
    hpp = open(os.path.join(ROOT, "pilotguru_amd", "host", "orb_extractor.hpp")).read()
    assert "MapPointCulling" in hpp and "KeyFrameCulling" in hpp and "pgorb_map_point_culling(" in hpp and "pgorb_keyframe_culling(" in hpp


def test_random_worlds_cover_what_they_are_for(randoms):
    """by the reference alone: the shares of the 300 worlds that cull a key frame, cull two or more, have a point go bad, and
    re-parent two or more children"""
    n = len(randoms)
    assert all(4 <= c.w.nkf <= 12 and max(len(s) for s in c.w.slots) <= 16 and len(c.w.obs) <= 48 for c, _ in randoms)
    assert sum(e["info"][2] >= 1 for _, e in randoms) >= 0.25 * n
    assert sum(e["info"][2] >= 2 for _, e in randoms) >= 0.05 * n
    assert sum(e["info"][3] >= 1 for _, e in randoms) >= 0.10 * n
    assert sum(int(np.sum((e["row_status"] & CU.ROW_REPARENTED) != 0)) >= 2 for _, e in randoms) >= 0.05 * n


def test_dirty_set_restatement_equals_the_literal_sequence(kf_cases, randoms):
    for c, want in [(c, K.expected_kf(c)) for c in kf_cases] + randoms:
        got = K.expected_kf(c, dirty=True)
        assert K.same(got, want, K.KF_KEYS), (c.name, K.diff(got, want, K.KF_KEYS))


KF_NAMED = (("redundant_ge", "nine_of_ten"), ("redundant_ge", "no_points"), ("obs_ge", "three_foreign_observers"), ("level_no_plus1", "octave_plus_one"),
            ("self_counted", "two_fine_observers"), ("th_two", "two_fine_observers"), ("bad_points_counted", "bad_points_in_slots"),
            ("no_sequence", "mutually_redundant"), ("bad_at_three", "third_loses_slot"), ("ref_kept", "reference_culled"),
            ("slots_kept", "third_loses_slot"), ("own_slots_cleared", "ten_of_eleven"), ("not_erase_ignored", "not_erase_member"),
            ("id0_culled", "id0_member"), ("no_resort", "thresholded_row_grows"), ("children_index_order", "tied_children"),
            ("candidates_not_grown", "three_children"), ("max_ge", "tied_children"), ("leftover_keep_parent", "three_children"))
MP_NAMED = (("ratio_le", "ratio_quarter_exact"), ("ratio_integer", "ratio_float_rounding"), ("few_obs_lt", "few_obs_edge"), ("age_gt", "few_obs_edge"),
            ("age_gt", "aged_out"), ("tests_reordered", "aged_low_ratio"))


def test_every_mutant_is_caught_by_name(kf_cases, mp_cases, randoms):
    pool = kf_cases + [c for c, _ in randoms[:60]]
    want = [K.expected_kf(c) for c in kf_cases] + [e for _, e in randoms[:60]]
    caught = {}
    for name, rules in CU.KF_MUTANTS.items():
        caught[name] = [c.name for c, e in zip(pool, want) if not K.same(e, K.expected_kf(c, rules), K.KF_KEYS)]
        assert caught[name], name
    want = [K.expected_mp(c) for c in mp_cases]
    for name, rules in CU.MP_MUTANTS.items():
        caught[name] = [c.name for c, e in zip(mp_cases, want) if not K.same(e, K.expected_mp(c, rules), K.MP_KEYS)]
        assert caught[name], name
    assert {n for n, _ in KF_NAMED} == set(CU.KF_MUTANTS) and {n for n, _ in MP_NAMED} == set(CU.MP_MUTANTS)
    assert set(CU.KF_MUTANTS) | set(CU.MP_MUTANTS) == {f.name for f in CU.dataclasses.fields(CU.Rules)}
    for name, where in KF_NAMED + MP_NAMED:
        assert where in caught[name], (name, caught[name][:8])


def test_hand_written_expectations(kf_cases, mp_cases):
    by = {c.name: c for c in kf_cases}
    rec = lambda e: [tuple(int(x) for x in r) for r in e["record"][:e["info"][1]]]
    e = K.expected_kf(by["nine_of_ten"])                      # 9 > 0.9 * 10 is false in double
    assert rec(e) == [(1, 10, 9, CU.KF_KEEP)] and list(e["info"]) == [0, 1, 0, 0] and not e["row_status"].any() and not e["kf_bad"].any()
    e = K.expected_kf(by["ten_of_eleven"])                    # 10 > 9.9; the point of {1, 2} goes bad and key frame 2 loses its slot
    assert rec(e) == [(1, 11, 10, CU.KF_CULLED)] and list(e["info"]) == [0, 1, 1, 1] and e["kf_bad"][1] == 1
    assert list(e["row_status"][:6]) == [0, CU.ROW_CLEARED, CU.ROW_REPARENTED, 0, 0, CU.ROW_ERASED]
    assert e["parent"][2] == 0 and e["parent"][1] == 0 and e["nconn"][1] == 0 and e["nconn"][5] == 0 and e["conn_kf"][5, 0] == -1
    assert e["kf_point"][2, 10] == -1 and e["point_bad"][10] == 1 and list(e["kf_point"][1, :11]) == list(range(11))   # the member's own slots stay
    assert not e["obs_live"][40:42].any() and e["obs_live"][:40].reshape(10, 4).sum(0).tolist() == [0, 10, 10, 10]
    e = K.expected_kf(by["no_points"])
    assert rec(e) == [(1, 0, 0, CU.KF_KEEP)]
    e = K.expected_kf(by["mutually_redundant"])               # the first is culled, the second then sees Observations() == 3
    assert rec(e) == [(1, 5, 5, CU.KF_CULLED), (2, 5, 0, CU.KF_KEEP)]
    e = K.expected_kf(by["third_loses_slot"])
    assert rec(e) == [(1, 22, 20, CU.KF_CULLED), (2, 23, 20, CU.KF_KEEP)] and e["info"][3] == 1
    e = K.expected_kf(by["reference_culled"])                 # address order 3, 5, 1, 4, 2: the reference moves to the first live entry, key frame 3
    assert rec(e) == [(1, 14, 13, CU.KF_CULLED)]
    assert e["ref_obs"][:14].tolist() == [0] * 14 and e["inputs"]["ref_obs"][:14].tolist() == [1] * 8 + [2] * 3 + [0, 0] + [1]
    e = K.expected_kf(by["not_erase_member"])
    assert rec(e) == [(1, 10, 10, CU.KF_TO_BE_ERASED)] and e["to_be_erased"][1] == 1 and not e["kf_bad"].any() and not e["row_status"].any()
    assert rec(K.expected_kf(by["id0_member"])) == [(1, -1, -1, CU.KF_ID0)]
    e = K.expected_kf(by["bad_member"])
    assert rec(e) == [(1, 10, 10, CU.KF_WAS_BAD)] and not e["row_status"].any() and e["obs_live"][:40].all()
    e = K.expected_kf(by["three_children"])                   # 5 is linked to the parent, 6 only to 5, 7 to nobody
    assert list(e["parent"][:9]) == [-1, 0, 0, 0, 0, 0, 5, 0, 4] and [int(x) for x in e["row_status"][5:8]] == [CU.ROW_REPARENTED] * 3
    e = K.expected_kf(by["tied_children"])                    # 6 comes first in address order and takes the tie; 5 then prefers 6 (9) over 0 (5)
    assert e["parent"][6] == 0 and e["parent"][5] == 6
    e = K.expected_kf(by["thresholded_row_grows"])
    assert e["inputs"]["nord"][2] == 2 and e["nord"][2] == 3 and list(e["ord_kf"][2, :3]) == [3, 4, 5] and list(e["ord_w"][2, :3]) == [16, 3, 2]
    assert e["row_status"][6] == 0 and e["row_status"][5] == 0 and 1 in e["conn_kf"][5, :e["nconn"][5]]      # the asymmetric connections
    e = K.expected_kf(by["list_cap_one_short"])
    assert list(e["info"]) == [CU.LIMIT, 3, 0, 0] and np.all(e["record"] == K.SENT) and np.all(e["row_status"] == K.SENT)
    mp = {c.name: K.expected_mp(c) for c in mp_cases}
    assert mp["ratio_quarter_exact"]["action"][0] == CU.MP_KEEP and mp["ratio_float_rounding"]["action"][0] == CU.MP_KEEP
    assert np.float32(1 << 24) / np.float32((1 << 26) + 1) == np.float32(0.25) and 4 * (1 << 24) < (1 << 26) + 1
    assert mp["visible_zero_found_zero"]["action"][0] == CU.MP_KEEP and mp["visible_zero_found_one"]["action"][0] == CU.MP_KEEP
    assert mp["few_obs_edge"]["action"][0] == CU.MP_FEW_OBS and mp["few_obs_three"]["action"][0] == CU.MP_KEEP
    assert mp["age_one_few_obs"]["action"][0] == CU.MP_KEEP and mp["aged_out"]["action"][0] == CU.MP_AGED
    assert mp["aged_low_ratio"]["action"][0] == CU.MP_FOUND_RATIO and mp["was_bad"]["action"][0] == CU.MP_WAS_BAD
    e = mp["every_action"]
    assert list(e["action"]) == [0, 3, 2, 4, 1, 2, 0] and list(e["recent_out"][:2]) == [0, 6] and list(e["info"]) == [0, 2, 3, 0]
    assert e["point_bad"][5] == 1 and not e["obs_live"][e["inputs"]["obs_start"][5]:e["inputs"]["obs_start"][6]].any()
    assert all(e["kf_point"][f, len(mp_cases[-1].w.slots[f]) - 1] == -1 for f in (1, 70))         # the 70 observers lose their (last) slot


def by_name(cases, name):
    return next(c for c in cases if c.name == name)


def _compaction_input(seed, npoints):
    r = np.random.RandomState(seed)
    ln = r.randint(0, 9, npoints)
    st = np.zeros(npoints + 1, np.int32)
    st[1:] = np.cumsum(ln)
    m = int(st[-1])
    live = (r.rand(m) < 0.6).astype(np.uint8)
    live[st[5]:st[6]] = 0
    live[st[7]:st[8]] = 1
    ref = np.array([r.randint(-1, max(x, 1)) for x in ln], np.int32)
    return st, r.randint(0, 50, m).astype(np.int32), r.randint(0, 900, m).astype(np.int32), live, ref


def test_compact_observations_against_a_plain_loop():
    import pilotguru_amd as pg
    for seed, n in ((0, 0), (1, 1), (2, 40), (3, 700)):
        a = _compaction_input(seed, max(n, 8))
        if n == 0:
            a = (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.int32))
        want, got = CU.compact_observations(*a), pg.compact_observations(*a)
        assert all(np.array_equal(x, y) and y.dtype == np.int32 for x, y in zip(want, got)), seed
    st, of, oi, live, ref = _compaction_input(4, 30)
    assert int(pg.compact_observations(st, of, oi, live, ref)[0][-1]) == int(live.sum())
    out = (np.zeros_like(st), np.zeros_like(of), np.zeros_like(oi), np.zeros_like(ref))
    got = pg.compact_observations(st, of, oi, live, ref, out=out)
    assert got[0] is out[0] and np.array_equal(out[1][:out[0][-1]], CU.compact_observations(st, of, oi, live, ref)[1])
    for alias in ((st, out[1], out[2], out[3]), (out[0], of, out[2], out[3]), (out[0], out[1], oi[:], out[3]), (out[0], out[1], out[2], ref)):
        with pytest.raises(ValueError):
            pg.compact_observations(st, of, oi, live, ref, out=alias)
    with pytest.raises(ValueError):
        pg.compact_observations(st[::-1].copy(), of, oi, live, ref)


class _NoLibrary:
    class _L:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)
    _L = _L()
    _h = None

    @staticmethod
    def _check(rc):
        return rc


def test_python_mirrors_refuse_malformed_input_without_a_device(kf_cases, mp_cases):
    import pilotguru_amd as pg
    c = by_name(kf_cases, "three_children")
    w = c.w
    e = K.expected_kf(c)
    a = e["inputs"]
    m = a["nobs"]

    def kf(state=None, **kw):
        v = dict(cur=c.cur, octv=w.octv, slots=w.slots, st=a["obs_start"], of=a["obs_frame"][:m], oi=a["obs_idx"][:m], live=a["obs_live"][:m],
                 ref=a["ref_obs"][:len(w.obs)], order=w.order, list_cap=None)
        v.update(kw)
        g = pg.CovisibilityGraph(_NoLibrary(), w.nkf, e["conn_cap"], v["order"], w.id0)
        for k in ("conn_kf", "conn_w", "nconn", "ord_kf", "ord_w", "nord", "parent"):
            getattr(g, k)[...] = a[k]
        for k, x in (state or {}).items():
            getattr(g, k)[...] = x
        return pg.LocalMapping.KeyFrameCulling(g, v["cur"], v["octv"], v["slots"], len(w.obs), w.point_bad, v["st"], v["of"], v["oi"], v["live"], v["ref"],
                                               list_cap=v["list_cap"])
    bad_start = a["obs_start"].copy()
    bad_start[2] = bad_start[1] - 1
    twice = a["obs_frame"][:m].copy()
    twice[1] = twice[0]
    for kw in (dict(cur=-1), dict(cur=w.nkf), dict(list_cap=0), dict(octv=w.octv[1:]), dict(slots=[[len(w.obs)]] + w.slots[1:]), dict(st=bad_start),
               dict(of=np.full(m, w.nkf, np.int32)), dict(of=twice), dict(oi=np.full(m, 99, np.int32)), dict(oi=a["obs_idx"][:m - 1]),
               dict(live=a["obs_live"][:m - 1]), dict(ref=np.full(len(w.obs), 4, np.int32)), dict(ref=np.full(len(w.obs), -2, np.int32)),
               dict(order=[0] * w.nkf), dict(state=dict(nconn=e["conn_cap"] + 1)), dict(state=dict(conn_kf=0)), dict(state=dict(ord_kf=w.nkf - 1, nord=1)),
               dict(state=dict(parent=w.nkf))):
        with pytest.raises(ValueError):
            kf(**kw)
    with pytest.raises(AssertionError, match="the library was called"):
        kf()
    c = by_name(mp_cases, "every_action")
    w = c.w
    a = K.expected_mp(c)["inputs"]
    m, n = a["nobs"], len(w.obs)

    def mp(**kw):
        v = dict(slots=w.slots, oi=a["obs_idx"][:m], live=a["obs_live"][:m], first=w.first_kf_id, recent=c.recent)
        v.update(kw)
        return pg.LocalMapping.MapPointCulling(_NoLibrary(), v["slots"], n, w.point_bad, a["obs_start"], a["obs_frame"][:m], v["oi"], v["live"], v["first"],
                                               w.visible, w.found, v["recent"], c.cur_kf_id)
    for kw in (dict(recent=[0, 0]), dict(recent=[n]), dict(recent=[-1]), dict(first=w.first_kf_id[1:]), dict(oi=np.full(m, 99, np.int32)),
               dict(live=a["obs_live"][:m - 1]), dict(slots=w.slots[1:])):
        with pytest.raises(ValueError):
            mp(**kw)
    with pytest.raises(AssertionError, match="the library was called"):
        mp()


CPP_DRIVER = r"""
#include "pilotguru_amd/host/orb_extractor.hpp"
#include <cstdio>
template <class F> static void run(const char* name, F&& f)
{
    try { f(); std::printf("%s ok\n", name); }
    catch (const std::invalid_argument&) { std::printf("%s invalid_argument\n", name); }
    catch (const std::runtime_error&) { std::printf("%s runtime_error\n", name); }
}
int main()
{
    using namespace pgorb;
    // three key frames, two points: point 0 seen by 0 and 1, point 1 by 1 and 2
    std::vector<std::vector<int32_t>> slots = {{0, -1}, {0, 1}, {1}};
    std::vector<std::vector<int32_t>> octaves = {{0, 0}, {0, 1}, {2}};
    MapPointObservations obs;
    obs.obsStart = {0, 2, 4};
    obs.obsFrame = {0, 1, 1, 2};
    obs.obsIdx = {0, 0, 1, 0};
    LocalMapping lm(nullptr);
    auto kf = [&](std::vector<std::vector<int32_t>> s, std::vector<std::vector<int32_t>> o, MapPointObservations ob, std::vector<uint8_t> live,
                  std::vector<int32_t> ref, int cur, int listCap, int parent0) {
        CovisibilityGraph g(nullptr, 3, 4);
        g.parent[0] = parent0;
        std::vector<uint8_t> pointBad(2, 0), kfBad(3, 0), toBeErased(3, 0);
        std::vector<int32_t> record, status;
        lm.KeyFrameCulling(g, cur, o, s, pointBad, ob, live, ref, {}, kfBad, toBeErased, listCap, record, status);
    };
    MapPointObservations twice = obs; twice.obsFrame = {0, 0, 1, 2};
    MapPointObservations range = obs; range.obsFrame = {0, 3, 1, 2};
    MapPointObservations idx = obs; idx.obsIdx = {0, 0, 2, 0};
    run("kf_well_formed", [&] { kf(slots, octaves, obs, {1, 1, 1, 1}, {0, 0}, 2, 4, -1); });
    run("kf_cur", [&] { kf(slots, octaves, obs, {1, 1, 1, 1}, {0, 0}, 3, 4, -1); });
    run("kf_list_cap", [&] { kf(slots, octaves, obs, {1, 1, 1, 1}, {0, 0}, 2, 0, -1); });
    run("kf_slot", [&] { kf({{2}, {0, 1}, {1}}, octaves, obs, {1, 1, 1, 1}, {0, 0}, 2, 4, -1); });
    run("kf_octaves", [&] { kf(slots, {{0}, {0, 1}, {2}}, obs, {1, 1, 1, 1}, {0, 0}, 2, 4, -1); });
    run("kf_obs_twice", [&] { kf(slots, octaves, twice, {1, 1, 1, 1}, {0, 0}, 2, 4, -1); });
    run("kf_obs_range", [&] { kf(slots, octaves, range, {1, 1, 1, 1}, {0, 0}, 2, 4, -1); });
    run("kf_obs_idx", [&] { kf(slots, octaves, idx, {1, 1, 1, 1}, {0, 0}, 2, 4, -1); });
    run("kf_live", [&] { kf(slots, octaves, obs, {1, 1, 1}, {0, 0}, 2, 4, -1); });
    run("kf_ref", [&] { kf(slots, octaves, obs, {1, 1, 1, 1}, {0, 2}, 2, 4, -1); });
    run("kf_parent", [&] { kf(slots, octaves, obs, {1, 1, 1, 1}, {0, 0}, 2, 4, 3); });
    auto mp = [&](MapPointObservations ob, std::vector<uint8_t> live, std::vector<int32_t> first, std::vector<int32_t> recent) {
        std::vector<std::vector<int32_t>> s = slots;
        std::vector<uint8_t> pointBad(2, 0);
        std::vector<int32_t> action, survivors;
        lm.MapPointCulling(s, pointBad, ob, live, first, {4, 4}, {4, 4}, recent, 5, 2, action, survivors);
    };
    run("mp_well_formed", [&] { mp(obs, {1, 1, 1, 1}, {3, 3}, {1, 0}); });
    run("mp_recent_twice", [&] { mp(obs, {1, 1, 1, 1}, {3, 3}, {1, 1}); });
    run("mp_recent_range", [&] { mp(obs, {1, 1, 1, 1}, {3, 3}, {2}); });
    run("mp_first", [&] { mp(obs, {1, 1, 1, 1}, {3}, {0}); });
    run("mp_live", [&] { mp(obs, {1, 1}, {3, 3}, {0}); });
    run("mp_obs_idx", [&] { mp(idx, {1, 1, 1, 1}, {3, 3}, {0}); });
    return 0;
}
"""


def test_cpp_mirror_rejects_bad_inputs_before_calling_the_library(tmp_path):
    """pgorb::LocalMapping::MapPointCulling / KeyFrameCulling throw std::invalid_argument for what the single calls would refuse,
    before any pointer reaches the library; well-formed input reaches it (a NULL context here, so PGORB_E_ARG comes back as
    std::runtime_error)."""
    import subprocess
    src, exe = os.path.join(str(tmp_path), "cull_driver.cc"), os.path.join(str(tmp_path), "cull_driver")
    open(src, "w").write(CPP_DRIVER)
    lib = os.path.join(ROOT, "pilotguru_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", ROOT, src, "-o", exe, "-L", lib, "-lpgorb", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    got = dict(l.split() for l in subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines())
    assert got.pop("kf_well_formed") == "runtime_error" and got.pop("mp_well_formed") == "runtime_error", got
    assert len(got) == 15 and set(got.values()) == {"invalid_argument"}, got


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    return pg.ORBextractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240)


def _host_equals_device(host, got, keys, name):
    for k in keys:
        assert np.asarray(host[k]).tobytes() == np.asarray(got[k]).tobytes(), (name, k)


@pytest.mark.gpu
def test_gpu_constructed_key_frame_cases_equal_the_reference_in_both_forms(ext, kf_cases):
    """every constructed case, the capacities exact and one short and the shapes that cross the kernel's strides (300 slots, 70
    observers, 70 connections) among them"""
    for c in kf_cases:
        e = K.expected_kf(c)
        got = K.download_kf(K.run_device_kf(c, ext, e), e)
        assert K.same(got, e, K.KF_KEYS), (c.name, "device", K.diff(got, e, K.KF_KEYS))
        host = K.run_host_kf(c, ext, e)
        assert K.same(host, e, K.KF_KEYS), (c.name, "host", K.diff(host, e, K.KF_KEYS))
        _host_equals_device(host, got, K.KF_KEYS, c.name)


@pytest.mark.gpu
def test_gpu_random_key_frame_worlds_equal_the_reference(ext, randoms):
    for c, e in randoms:
        got = K.download_kf(K.run_device_kf(c, ext, e), e)
        assert K.same(got, e, K.KF_KEYS), (c.name, K.diff(got, e, K.KF_KEYS))


@pytest.mark.gpu
def test_gpu_map_point_culling_equals_the_reference_in_both_forms(ext, mp_cases):
    for c in mp_cases + [K.random_mp(s) for s in range(NRANDOM)]:
        e = K.expected_mp(c)
        got = K.download_mp(K.run_device_mp(c, ext, e), c)
        assert K.same(got, e, K.MP_KEYS), (c.name, "device", K.diff(got, e, K.MP_KEYS))
        if not c.name.startswith("random") or c.name.endswith("7"):
            host = K.run_host_mp(c, ext, e)
            assert K.same(host, e, K.MP_KEYS), (c.name, "host", K.diff(host, e, K.MP_KEYS))
            _host_equals_device(host, got, K.MP_KEYS, c.name)


@pytest.mark.gpu
def test_gpu_recent_entry_out_of_range_is_dropped_by_the_device_form(ext, mp_cases):
    c = by_name(mp_cases, "every_action")
    e = K.expected_mp(c)
    n = len(c.w.obs)
    c2 = K.MpCase("out_of_range", c.w, [n, c.recent[0], -1] + c.recent[1:], c.cur_kf_id)
    got = K.download_mp(K.run_device_mp(c2, ext, e), c2)
    assert list(got["action"]) == [CU.MP_NONE, 0, CU.MP_NONE] + list(e["action"][1:]) and list(got["recent_out"][:2]) == [0, 6]
    assert got["nrecent_out"][0] == 2 and all(np.array_equal(got[k], e[k]) for k in ("kf_point", "point_bad", "obs_live"))


@pytest.mark.gpu
def test_gpu_host_forms_refuse_malformed_input(ext, kf_cases, mp_cases):
    from pilotguru_amd import _lib
    c = by_name(kf_cases, "three_children")
    e = K.expected_kf(c)
    a, w = e["inputs"], c.w
    m = a["nobs"]

    def kf(change):
        a2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
        c2, e2 = K.KfCase(c.name, w, c.cur), dict(e, inputs=a2)
        change(a2, c2, e2)
        try:
            K.run_host_kf(c2, ext, e2)
        except AssertionError as x:
            return x.args[0][0]
        return 0

    def setv(k, i, v):
        return lambda a2, c2, e2: a2[k].__setitem__(i, v)
    changes = [setv("kf_point", (1, 0), len(w.obs)), setv("kf_point", (1, 0), -2), setv("n", 0, -1), setv("obs_start", 0, 1), setv("obs_start", 2, 0),
               setv("obs_frame", 0, w.nkf), setv("obs_frame", 1, int(a["obs_frame"][0])), setv("obs_idx", 0, 99), setv("obs_idx", 0, -1),
               setv("ref_obs", 0, 4), setv("ref_obs", 0, -2), setv("nconn", 0, e["conn_cap"] + 1), setv("nord", 0, -1), setv("conn_kf", (1, 0), 1),
               setv("conn_kf", (1, 0), w.nkf), setv("ord_kf", (1, 0), 3), setv("parent", 2, w.nkf), setv("parent", 2, -2),
               lambda a2, c2, e2: a2["conn_kf"].__setitem__((5, slice(0, 2)), a2["conn_kf"][5, 1::-1].copy()),
               lambda a2, c2, e2: a2.__setitem__("order", np.zeros(w.nkf, np.int32)),
               lambda a2, c2, e2: setattr(c2, "cur", w.nkf), lambda a2, c2, e2: setattr(c2, "cur", -1), lambda a2, c2, e2: e2.__setitem__("list_cap", 0)]
    for i, ch in enumerate(changes):
        assert kf(ch) == _lib.PGORB_E_ARG, i
    assert kf(lambda a2, c2, e2: None) == 0
    c = by_name(mp_cases, "every_action")
    e = K.expected_mp(c)
    a, w = e["inputs"], c.w

    def mp(change, recent=None):
        a2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
        change(a2)
        try:
            K.run_host_mp(K.MpCase(c.name, w, c.recent if recent is None else recent, c.cur_kf_id), ext, dict(e, inputs=a2))
        except AssertionError as x:
            return x.args[0][0]
        return 0
    for i, ch in enumerate([lambda a2: a2["kf_point"].__setitem__((0, 0), len(w.obs)), lambda a2: a2["obs_start"].__setitem__(0, 1),
                            lambda a2: a2["obs_frame"].__setitem__(0, w.nkf), lambda a2: a2["obs_frame"].__setitem__(1, int(a["obs_frame"][0])),
                            lambda a2: a2["obs_idx"].__setitem__(0, 99), lambda a2: a2["n"].__setitem__(0, -1)]):
        assert mp(ch) == _lib.PGORB_E_ARG, i
    assert mp(lambda a2: None, [0, 0]) == _lib.PGORB_E_ARG and mp(lambda a2: None, [len(w.obs)]) == _lib.PGORB_E_ARG and mp(lambda a2: None) == 0


@pytest.mark.gpu
def test_gpu_python_mirrors_return_what_the_host_forms_leave(ext, kf_cases, mp_cases):
    import pilotguru_amd as pg
    c = by_name(kf_cases, "third_loses_slot")
    e = K.expected_kf(c)
    a, w = e["inputs"], c.w
    m, n = a["nobs"], len(w.obs)
    g = pg.CovisibilityGraph(ext, w.nkf, e["conn_cap"], w.order, w.id0)
    for k in ("conn_kf", "conn_w", "nconn", "ord_kf", "ord_w", "nord", "parent"):
        getattr(g, k)[...] = a[k]
    r = pg.LocalMapping.KeyFrameCulling(g, c.cur, w.octv, w.slots, n, w.point_bad, a["obs_start"], a["obs_frame"][:m], a["obs_idx"][:m], a["obs_live"][:m],
                                        a["ref_obs"][:n], w.kf_bad, w.not_erase, w.to_be_erased)
    nl = int(e["info"][1])
    assert np.array_equal(r["record"], e["record"][:nl]) and np.array_equal(r["row_status"], e["row_status"]) and np.array_equal(r["info"], e["info"])
    for f in range(w.nkf):
        assert list(r["kf_point"][f]) == list(e["kf_point"][f, :len(w.slots[f])]), f
    for k, cnt in (("point_bad", n), ("obs_live", m), ("ref_obs", n), ("kf_bad", w.nkf)):
        assert np.array_equal(r[k], e[k][:cnt]), k
    for k in ("conn_kf", "conn_w", "nconn", "ord_kf", "ord_w", "nord", "parent"):
        assert np.array_equal(getattr(g, k), e[k]), k
    c = by_name(mp_cases, "every_action")
    e = K.expected_mp(c)
    a, w = e["inputs"], c.w
    m, n = a["nobs"], len(w.obs)
    r = pg.LocalMapping.MapPointCulling(ext, w.slots, n, w.point_bad, a["obs_start"], a["obs_frame"][:m], a["obs_idx"][:m], a["obs_live"][:m], w.first_kf_id,
                                        w.visible, w.found, c.recent, c.cur_kf_id)
    assert list(r["action"]) == list(e["action"]) and list(r["recent"]) == [0, 6] and np.array_equal(r["point_bad"], e["point_bad"][:n])
    assert np.array_equal(r["obs_live"], e["obs_live"][:m]) and all(list(r["kf_point"][f]) == list(e["kf_point"][f, :len(w.slots[f])]) for f in range(w.nkf))


def _compact_device(ext, st, of, oi, live, ref, stream=None):
    import torch
    n, m = len(st) - 1, len(of)
    d = [CC.dev(x) if len(x) else CC.dev(np.zeros(1, x.dtype)) for x in (st, of, oi, live, ref)]
    full = lambda k: torch.full((k,), K.SENT, dtype=torch.int32, device="cuda")
    out = [full(n + 3), full(m + 2), full(m + 2), full(n + 2), full(3)]
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = ext._L.pgorb_compact_observations_device(ext._h, n, *[CC.ptr(x) for x in d[:3]], m, CC.ptr(d[3]), CC.ptr(d[4]), *[CC.ptr(x) for x in out],
                                                  C.c_void_p(s.cuda_stream))
    assert rc == 0, (rc, ext._L.pgorb_last_error(ext._h))
    return d, out


@pytest.mark.gpu
def test_gpu_compaction_equals_the_plain_loop(ext):
    """3000 points: more than one tile of the scan; an empty table; untouched bytes"""
    import torch
    for seed, n in ((1, 3000), (2, 257), (3, 8)):
        a = _compaction_input(seed, n)
        want = CU.compact_observations(*a)
        _, out = _compact_device(ext, *a)
        torch.cuda.synchronize()
        h = [t.cpu().numpy() for t in out]
        new = int(want[0][-1])
        assert np.array_equal(h[0][:n + 1], want[0]) and np.all(h[0][n + 1:] == K.SENT), seed
        assert np.array_equal(h[1][:new], want[1]) and np.array_equal(h[2][:new], want[2]) and np.all(h[1][new:] == K.SENT) and np.all(h[2][new:] == K.SENT)
        assert np.array_equal(h[3][:n], want[3]) and np.all(h[3][n:] == K.SENT) and h[4][0] == new and np.all(h[4][1:] == K.SENT)
    empty = (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.int32))
    _, out = _compact_device(ext, *empty)
    torch.cuda.synchronize()
    assert out[0].cpu().numpy()[0] == 0 and out[4].cpu().numpy()[0] == 0


@pytest.mark.gpu
def test_gpu_repeat_and_second_stream_give_the_same_bytes(ext, kf_cases, mp_cases):
    import torch
    for c in [by_name(kf_cases, n) for n in ("strides", "three_children", "third_loses_slot")]:
        e = K.expected_kf(c)
        first = K.download_kf(K.run_device_kf(c, ext, e), e)
        again = K.download_kf(K.run_device_kf(c, ext, e), e)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            d = K.run_device_kf(c, ext, e, stream=st)
        st.synchronize()
        other = K.download_kf(d, e)
        for k in K.KF_KEYS:
            assert first[k].tobytes() == again[k].tobytes() == other[k].tobytes(), (c.name, k)
    c = by_name(mp_cases, "every_action")
    e = K.expected_mp(c)
    first = K.download_mp(K.run_device_mp(c, ext, e), c)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d = K.run_device_mp(c, ext, e, stream=st)
    st.synchronize()
    other = K.download_mp(d, c)
    for k in K.MP_KEYS:
        assert first[k].tobytes() == other[k].tobytes(), k


@pytest.mark.gpu
def test_gpu_chain_into_update_connections_and_the_refresh_on_resident_arrays(ext, kf_cases):
    """KeyFrameCulling -> compaction -> pgorb_update_connections_batch_device of a new key frame -> pgorb_refresh_map_points_batch_device
    on one stream with nothing downloaded in between: the bytes of the same two calls fed what the reference's culling and the plain
    compaction leave."""
    import torch
    from pilotguru_amd.orb import KF_POSE_DTYPE, MAP_POINT_DTYPE, MP_BOTH
    c = by_name(kf_cases, "third_loses_slot")
    c = K.KfCase(c.name, c.w, c.cur, conn_cap=8)                         # room for the row UpdateConnections writes afterwards
    e = K.expected_kf(c)
    a, w = e["inputs"], c.w
    nkf, n, m, cap = w.nkf, len(w.obs), a["nobs"], a["cap"]
    assert e["info"][2] == 1 and e["info"][3] == 1
    r = np.random.RandomState(3)
    bytes_of = lambda x: torch.from_numpy(np.frombuffer(np.ascontiguousarray(x).tobytes(), np.uint8).copy()).cuda()
    pose = np.zeros(nkf, KF_POSE_DTYPE)
    pose["Ow"] = r.uniform(-1, 1, (nkf, 3))
    pts = np.zeros(n, MAP_POINT_DTYPE)
    pts["pos"] = r.uniform(-1, 1, (n, 3)) + [0, 0, 6]
    desc, pdesc = r.randint(0, 256, (nkf, cap, 32)).astype(np.uint8), np.zeros((n, 32), np.uint8)
    new_kf = 2                                                           # the key frame whose connections are updated next: it lost two slots

    def tail(kf_point, point_bad, st, of, oi, ref, graph, stream):
        """the two calls after the compaction; returns every array they write"""
        full = lambda *shape: torch.full(shape, K.SENT, dtype=torch.int32, device="cuda")
        lst, status, info = CC.dev(np.array([new_kf], np.int32)), full(nkf), full(CU.INFO)
        first = CC.dev(np.zeros(nkf, np.uint8))
        q = CC.ptr
        s = C.c_void_p(stream.cuda_stream)
        rc = ext._L.pgorb_update_connections_batch_device(
            ext._h, q(kf_point), q(d0["n"]), nkf, cap, n, q(point_bad), q(st), q(of), m, q(d0["order"]), q(d0["id0"]), 1, q(lst), 2, e["conn_cap"],
            *[q(graph[k]) for k in ("conn_kf", "conn_w", "nconn", "ord_kf", "ord_w", "nord", "parent")], q(first), q(status), 0, None, q(info), s)
        assert rc == 0, (rc, ext._L.pgorb_last_error(ext._h))
        d_pts, d_pd, best, mstat = bytes_of(pts), bytes_of(pdesc), full(n), full(n)
        rc = ext._L.pgorb_refresh_map_points_batch_device(
            ext._h, q(d0["kps"]), q(d_desc), q(d0["n"]), nkf, cap, q(d_pose), q(d0["kf_bad_after"]), n, q(d_pts), q(d_pd), q(point_bad), q(st), q(of), q(oi),
            m, q(ref), n, None, MP_BOTH, q(best), q(mstat), s)
        assert rc == 0, (rc, ext._L.pgorb_last_error(ext._h))
        return [graph[k] for k in ("conn_kf", "conn_w", "nconn", "ord_kf", "ord_w", "nord", "parent")] + [status, info, d_pts, d_pd, best, mstat]

    stream = torch.cuda.current_stream()
    d_desc, d_pose = bytes_of(desc), bytes_of(pose)
    d0 = K.upload(a)
    d0["kf_bad_after"] = d0["kf_bad"]
    d = K.run_device_kf(c, ext, e, d=d0, stream=stream)
    full = lambda k: torch.full((k,), K.SENT, dtype=torch.int32, device="cuda")
    cst, cof, coi, cref, cinfo = full(n + 1), full(m + 1), full(m + 1), full(n + 1), full(1)
    rc = ext._L.pgorb_compact_observations_device(ext._h, n, CC.ptr(d["obs_start"]), CC.ptr(d["obs_frame"]), CC.ptr(d["obs_idx"]), m, CC.ptr(d["obs_live"]),
                                                  CC.ptr(d["ref_obs"]), CC.ptr(cst), CC.ptr(cof), CC.ptr(coi), CC.ptr(cref), CC.ptr(cinfo),
                                                  C.c_void_p(stream.cuda_stream))
    assert rc == 0
    chained = tail(d["kf_point"], d["point_bad"], cst, cof, coi, cref, d, stream)
    torch.cuda.synchronize()
    chained = [t.cpu().numpy().tobytes() for t in chained]
    # fed: the reference's state after the cull and the plain compaction
    want = CU.compact_observations(a["obs_start"], a["obs_frame"], a["obs_idx"], e["obs_live"], e["ref_obs"])
    assert int(cinfo.cpu().numpy()[0]) == int(want[0][-1]) < m
    pad = lambda x, k: np.concatenate([x, np.full(k - len(x), K.SENT, np.int32)])
    graph = {k: CC.dev(e[k]) for k in ("conn_kf", "conn_w", "nconn", "ord_kf", "ord_w", "nord", "parent")}
    d0["kf_bad_after"] = CC.dev(e["kf_bad"])
    fed = tail(CC.dev(e["kf_point"]), CC.dev(e["point_bad"]), CC.dev(pad(want[0], n + 1)), CC.dev(pad(want[1], m + 1)), CC.dev(pad(want[2], m + 1)),
               CC.dev(pad(want[3], n + 1)), graph, stream)
    torch.cuda.synchronize()
    fed = [t.cpu().numpy().tobytes() for t in fed]
    assert chained == fed
    row = np.frombuffer(fed[0], np.int32).reshape(nkf, -1)[new_kf, :np.frombuffer(fed[2], np.int32)[new_kf]]
    assert np.frombuffer(fed[7], np.int32)[new_kf] & 1 and 1 not in row and 3 in row      # the row was rewritten from the counters, without the culled key frame
    assert (np.frombuffer(fed[12], np.int32) > 0).sum() >= n - 4                           # the points that are left were refreshed
