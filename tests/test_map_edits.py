"""The map edits on the GPU (pilotguru_amd/csrc/map_edit.hip; include/pgorb.h: MapPoint::AddObservation, Replace, EraseObservation with
their KeyFrame slot writes, applied from an ordered edit list, and the producers of that list) against the literal object-level
reference (tests/map_edit_reference.py) on constructed cases and seeded random worlds (tests/map_edit_cases.py).  Integers only:
every comparison is exact, untouched bytes included (the outputs start as a sentinel).

The CPU tests check presence (they fail without the symbols), that the restatement of the kernel's decomposition equals the literal
sequence, what every rule mutant changes on the case named for it, the reference's coverage of the random worlds, the numpy
producers against the reference's call-site loops, and the refusals of the Python mirror.  The GPU tests compare the device form,
the host form and the reference byte for byte, the device producers with their numpy forms, and check determinism and capacities."""
import ctypes as C
import dataclasses
import os
import re
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_edit_cases as K  # noqa: E402
import map_edit_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pgorb_apply_map_edits", "pgorb_apply_map_edits_device", "pgorb_map_edits_from_keyframe_device",  "pgorb_map_edits_from_fuse_device", "pgorb_map_edits_from_lba_erase_device", "pgorb_map_edits_from_loop_matches_device",
         "pgorb_observation_ids_device")
NRANDOM = 300


@pytest.fixture(scope="module")
def cases():
    return K.cases()


@pytest.fixture(scope="module")
def randoms():
    """(case, what the reference leaves), computed once"""
    out = []
    for s in range(NRANDOM):
        c = K.random_world(s)
        out.append((c, K.expected(c)))
    return out


def by_name(cases, name):
    return next(c for c in cases if c.name == name)


def test_symbols_constants_and_null_context():
    from pilotguru_amd import _lib
    import pilotguru_amd as pg
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name)
    p = None
    assert L.pgorb_apply_map_edits(p, p, 0, 0, p, p, p, 0, *([p] * 9), 0, *([p] * 6), 0, 0, p, p) == -1
    assert L.pgorb_apply_map_edits_device(p, p, 0, p, p, p, 0, 1, p, 0, *([p] * 7), 0, p, p, 0, *([p] * 6), 0, 0, p, p, p) == -1
    assert L.pgorb_map_edits_from_keyframe_device(p, p, p, 1, 1, 0, p, p, p, 0, p, 0, p, p, p) == -1
    assert L.pgorb_map_edits_from_fuse_device(p, p, p, 1, 1, 0, 0, 1, *([p] * 7)) == -1
    assert L.pgorb_map_edits_from_lba_erase_device(p, 0, p, p, 0, p, p, p) == -1
    assert L.pgorb_map_edits_from_loop_matches_device(p, p, p, 1, 1, 0, 0, p, p, p) == -1
    assert L.pgorb_observation_ids_device(p, 0, p, p, 0, p, 0, p, p) == -1
    hdr = open(os.path.join(ROOT, "include", "pgorb.h")).read()
    defs = dict(re.findall(r"#define\s+PGORB_(EDIT_\w+)\s+(\d+)", hdr))
    assert len(defs) == 19
    for k, v in defs.items():
        assert getattr(pg, k) == int(v), k
        assert getattr(R, k[5:]) == int(v), k
    assert "typedef struct pgorb_map_edit { int32_t op, a, b, c; } pgorb_map_edit;" in hdr
    assert pg.MAP_EDIT_DTYPE.itemsize == 16 and pg.MAP_EDIT_DTYPE == R.EDIT_DTYPE
    assert callable(pg.apply_map_edits) and callable(pg.LocalMapping.ProcessNewKeyFrame)


def test_decomposition_equals_the_literal_sequence(cases, randoms):
    """components, the bag, the last write per slot, plan then commit: the kernel's algorithm, before a GPU sees it"""
    for c, want in [(c, K.expected(c)) for c in cases] + randoms:
        got = K.apply_decomposed(c, want)
        assert K.same(got, want), (c.name, K.diff(got, want))
    for c in cases + [c for c, _ in randoms[:40]]:                  # NOP padding changes nothing but the positions of the status words
        cp, at = K.padded(c, len(c.edits))
        want, plain = K.expected(cp), K.expected(c)
        got = K.apply_decomposed(cp, want)
        assert K.same(got, want), (cp.name, K.diff(got, want))
        assert all(np.array_equal(got[k], plain[k]) for k in K.KEYS if k != "edit_status"), cp.name
        assert np.array_equal(got["edit_status"][at], plain["edit_status"][:len(c.edits)][c.edits["op"] != R.NOP]), cp.name
    c = by_name(cases, "fuse_chain_on_one_slot")                    # ... and under each of the limits
    e = K.expected(c)
    for short in (dataclasses.replace(c, obs_cap_out=int(e["info"][1]) - 1), dataclasses.replace(c, sel_cap=int(e["info"][7]) - 1)):
        want = K.expected(short)
        assert want["info"][0] == R.LIMIT and K.same(K.apply_decomposed(short, want), want)
    for c in (_bag_case(0), _bag_case(1)):
        want = K.expected(c)
        assert (want["info"][0] == R.LIMIT) == c.name.endswith("past") and K.same(K.apply_decomposed(c, want), want), c.name


NAMED = (("add_skips_slot_when_observed", "add_already_observed"), ("replace_tests_slot", "replace_shared_key_frame"),
         ("replace_skips_bad_loser_counters", "loser_already_bad"), ("replace_keeps_loser_good", "replace_disjoint"), ("replace_self_clears", "self_replace"),
         ("erase_bad_at_three", "erase_moves_reference"), ("erase_bad_below_two", "erase_three_to_two_then_again"), ("erase_ref_to_last", "erase_moves_reference"),
         ("erase_keeps_slot", "erase_moves_reference"), ("set_bad_clears_own_slots_only", "set_bad_clears_a_foreign_slot"),
         ("set_bad_drops_ref", "bad_point_added_again_keeps_reference"), ("first_writer_wins", "dangling_slot_collision"), ("list_order_by_index", "add_front"),
         ("list_order_by_index", "add_middle"), ("dead_entries_counted", "dead_masked_input"))


def test_every_mutant_is_caught_by_name(cases):
    want = {c.name: K.expected(c, exact=False) for c in cases}
    caught = {name: [c.name for c in cases if not K.same(K.expected(c, rules, exact=False), want[c.name])] for name, rules in R.MUTANTS.items()}
    assert {n for n, _ in NAMED} == set(R.MUTANTS)
    for name, where in NAMED:
        assert where in caught[name], (name, caught[name])


def test_hand_written_expectations(cases):
    e = {c.name: K.expected(c) for c in cases}
    lists = lambda x: [list(zip(x["obs_frame_out"][a:b].tolist(), x["obs_idx_out"][a:b].tolist())) for a, b in zip(x["obs_start_out"][:-3], x["obs_start_out"][1:-2])]
    assert lists(e["add_front"])[0] == [(1, 3), (0, 0), (4, 0)] and lists(e["add_middle"])[0] == [(1, 0), (0, 3), (2, 0)]      # by rank: 1, 3, 0, 4, 2
    assert lists(e["add_end"])[0] == [(0, 0), (4, 0), (2, 3)]
    x = e["add_already_observed"]
    assert x["edit_status"][0] == R.APPLIED | R.ALREADY and x["kf_point"][0, 5] == 0 and x["kf_point"][0, 2] == 0 and x["touched"][0] == 0
    x = e["replace_shared_key_frame"]                              # key frame 1 is the survivor's already: its slot is cleared, not handed over
    assert lists(x)[:2] == [[], [(1, 2), (0, 1), (2, 0)]] and x["kf_point"][1, 1] == -1 and x["kf_point"][0, 1] == 1 and x["kf_point"][1, 2] == 2
    assert list(x["point_bad"][:2]) == [1, 0] and x["replaced"][0] == 1 and x["found"][1] == 5 + 6 and x["visible"][1] == 10 + 11
    assert x["touched"][1] == R.TOUCH_CHANGED | R.TOUCH_SURVIVOR and list(x["select_out"][:3]) == [0, 1, -1]
    assert e["self_replace"]["edit_status"][0] == R.SELF and not e["self_replace"]["point_bad"].any()
    x = e["chain"]
    assert lists(x) == [[], [], [(1, 1), (0, 4), (2, 2)]] and x["kf_point"][0, 0] == -1 and x["kf_point"][0, 4] == 2 and x["found"][2] == 5 + 6 + 7 and list(x["replaced"]) == [1, 2, -1]
    x = e["loser_already_bad"]
    assert x["found"][1] == 9 and x["visible"][1] == 15 and x["info"][3] == 0 and x["edit_status"][0] == R.APPLIED
    x = e["dangling_slot_collision"]                               # the later edit's value, though another component wrote the slot first
    assert x["kf_point"][2, 3] == 1 and x["info"][4] == 2 and x["edit_status"][1] == R.APPLIED | R.ALREADY
    x = e["erase_moves_reference"]
    assert lists(x)[0] == [(3, 0), (0, 0), (4, 0)] and x["ref_obs_out"][0] == 0 and not x["point_bad"][0] and x["kf_point"][1, 0] == -1
    x = e["erase_three_to_two_then_again"]
    assert list(x["edit_status"][:2]) == [R.APPLIED | R.WENT_BAD, R.NOT_OBSERVED] and x["point_bad"][0] and not (x["kf_point"][:3, 0] >= 0).any()
    assert x["ref_obs_out"][0] == -1 and x["info"][5] == 3
    x = e["bad_point_added_again_keeps_reference"]
    assert lists(x)[0] == [(1, 6)] and x["ref_obs_out"][0] == 0 and x["point_bad"][0] == 1
    assert e["set_bad_clears_a_foreign_slot"]["kf_point"][2, 2] == -1
    x = e["erase_last_observation"]
    assert x["ref_obs_out"][0] == -1 and x["point_bad"][0] and x["obs_start_out"][1] == 0
    x = e["erase_unlisted_key_frame"]
    assert x["edit_status"][0] == R.NOT_OBSERVED and x["info"][2] == 0 and x["touched"][0] == 0
    x = e["fuse_chain_on_one_slot"]
    assert x["kf_point"][3, 4] == 2 and lists(x) == [[], [], [(1, 2), (3, 4), (0, 2), (2, 2)]] and list(x["point_bad"]) == [1, 1, 0] and x["info"][6] == 0
    x = e["two_new_points_on_one_idx2"]
    assert x["kf_point"][2, 6] == 2 and lists(x)[1:] == [[(4, 1), (2, 6)], [(4, 2), (2, 6)]] and list(x["ref_obs_out"][1:3]) == [0, 0]
    x = e["point_in_two_slots_of_a_new_key_frame"]
    assert [int(v) for v in by_name(cases, "point_in_two_slots_of_a_new_key_frame").edits["op"]] == [0, R.ADD, R.ADD, 0, 0, 0, 0, 0]
    x = e["dead_masked_input"]
    assert lists(x) == [[(1, 4), (0, 0), (2, 0)], [(4, 1)], [(1, 2)]] and list(x["ref_obs_out"][:3]) == [-1, 0, 0] and x["edit_status"][0] == R.APPLIED
    x = e["bad_indices"]
    assert list(x["edit_status"][:9]) == [R.BAD_INDEX] * 8 + [R.APPLIED] and x["kf_point"][1, 7] == 0
    assert list(e["selection_of_survivors_only"]["select_out"][:3]) == [1, -1, -1]
    x = e["stale_descriptor"]
    assert x["touched"][1] == R.TOUCH_CHANGED | R.TOUCH_SURVIVOR | R.TOUCH_STALE and x["info"][6] == 1
    x = e["empty_edit_list_compacts"]
    assert lists(x) == [[(0, 0), (2, 0)], []] and list(x["ref_obs_out"][:2]) == [1, -1] and list(x["info"][:8]) == [0, 2, 0, 0, 0, 0, 0, 0]


def test_random_worlds_cover_what_they_are_for(randoms):
    """by the reference alone"""
    n = len(randoms)
    shared = went_bad = comp3 = collide = 0
    for c, e in randoms:
        a = c.a
        assert 4 <= len(a["n"]) <= 12 and a["cap"] <= 16 and len(a["obs_start"]) - 1 <= 48 and len(c.edits) <= 64
        s = e["stats"]
        comp = R.components(a, c.edits)
        per = Counter(comp[int(x["a"])] for x in c.edits if x["op"] != R.NOP and R.edit_valid(a, x))
        shared += s["shared"] > 0
        went_bad += bool(np.any(s["status"] & R.WENT_BAD))
        comp3 += any(v >= 3 for v in per.values())
        collide += any(len({comp[int(c.edits[k]["a"])] for k in h}) > 1 for h in s["history"].values())
    assert shared >= 0.25 * n and went_bad >= 0.10 * n and comp3 >= 0.10 * n and collide >= 0.05 * n, (shared, went_bad, comp3, collide)


def _bag_case(past):
    """two points of 1024 observations each, merged: a component of exactly MAX_BAG entries; one ADD more is one past it"""
    half = R.MAX_BAG // 2
    lists = [[(f, 0) for f in range(half)], [(f, 0) for f in range(half, 2 * half)], [(0, 1)]]
    a = K.world(2 * half, 2, lists, list(np.random.RandomState(5).permutation(2 * half)))
    return K.Case("bag_past" if past else "bag_full", a, K.E((R.REPLACE, 0, 1), (R.ADD, 1, 0, 1)) if past else K.E((R.REPLACE, 0, 1), (R.ADD, 2, 3, 1)))


def _wide_cases():
    r = np.random.RandomState(9)
    nkf, cap, old, fresh = 6, 2000, 1500, 400
    free = [list(r.permutation(cap)) for _ in range(nkf)]
    lists = [[(int(f), int(free[f].pop())) for f in r.permutation(nkf)[:r.randint(2, 5)]] for _ in range(old)] + [[] for _ in range(fresh)]
    a = K.world(nkf, cap, lists, list(r.permutation(nkf)), bad=range(old, old + fresh))
    a["point_bad"][old:] = 0                                       # the rows a producer has just filled: good, no list yet
    ed = np.zeros(3 * cap, R.EDIT_DTYPE)                           # (SET_REF, ADD, ADD) at 3j .. 3j + 2, NOP past the count
    for j in range(fresh):
        kf2, i1, i2 = int(r.randint(1, nkf)), int(free[0].pop()), int(r.randint(cap))
        ed[3 * j], ed[3 * j + 1], ed[3 * j + 2] = (R.SET_REF, old + j, 0, 0), (R.ADD, old + j, 0, i1), (R.ADD, old + j, kf2, i2)
    import pilotguru_amd as pg
    erase = pg.map_edits_from_lba_erase(a["obs_start"], a["obs_frame"], r.rand(a["nobs"]) < 0.1).astype(R.EDIT_DTYPE)
    return [K.Case("wide_new_points", a, ed), K.Case("wide_erase", a, erase)]


def _full_list_case():
    """MAX_EDITS edits, every one carried out"""
    a = K.world(8, 16, [[(p % 8, p // 8)] for p in range(64)], list(np.random.RandomState(6).permutation(8)))
    k = np.arange(R.MAX_EDITS)
    ed = np.zeros(R.MAX_EDITS, R.EDIT_DTYPE)
    ed["op"], ed["a"], ed["b"], ed["c"] = R.ADD, k % 64, (k // 64) % 8, (k * 7) % 16
    ed["op"][k % 97 == 0] = R.ERASE
    return K.Case("full_list", a, ed)


# ---------------------------------------------------------------- the producers against the call-site loops (CPU)
def _state(W, cap):
    t = R.table(W, cap)
    return {k: t[k] for k in ("kf_point", "point_bad", "visible", "found", "replaced", "obs_start", "obs_frame", "obs_idx", "ref_obs")}


def _after_edits(a, edits, npoints_after=None):
    """the reference's objects after the edit list, as _state gives them"""
    e = R.apply_edits(a, edits.astype(R.EDIT_DTYPE), 1 << 16, 0, 0)
    assert e["info"][0] == 0
    total = int(e["info"][1])
    return dict(kf_point=e["kf_point"], point_bad=e["point_bad"], visible=e["visible"], found=e["found"], replaced=e["replaced"],
                obs_start=e["obs_start_out"], obs_frame=e["obs_frame_out"][:total], obs_idx=e["obs_idx_out"][:total], ref_obs=e["ref_obs_out"])


def _same_state(x, y):
    return [k for k in x if not np.array_equal(x[k], y[k])]


def _clean(c):
    """a random world without dangling slots: every slot holds the point that lists it (what the producers' call sites require)"""
    a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.a.items()}
    a["kf_point"][:] = -1
    st = a["obs_start"]
    for p in range(len(st) - 1):
        for o in range(st[p], st[p + 1]):
            if a["obs_live"][o] and not a["point_bad"][p]:
                a["kf_point"][a["obs_frame"][o], a["obs_idx"][o]] = p
    return a


def test_numpy_producers_equal_the_call_site_loops(randoms):
    import pilotguru_amd as pg
    for c, _ in randoms[:120]:
        a = _clean(c)
        r = np.random.RandomState(len(c.edits))
        nkf, npoints, cap = len(a["n"]), len(a["obs_start"]) - 1, a["cap"]
        kf = int(r.randint(nkf))
        # ProcessNewKeyFrame: the new key frame's slots hold points that do not list it yet, one of them twice
        b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
        for i in r.choice(cap, 4, replace=False):
            b["kf_point"][kf, i] = r.randint(-1, npoints)
        b["kf_point"][kf, r.randint(cap)] = b["kf_point"][kf, 0]
        W = R.World(b)
        cls = R.process_new_key_frame(W, kf)
        edits, got_cls = pg.map_edits_from_keyframe(b["kf_point"][kf], npoints, b["point_bad"], b["obs_start"], b["obs_frame"], b["obs_live"], kf)
        assert list(got_cls) == cls and not _same_state(_state(W, cap), _after_edits(b, edits)), (c.name, "keyframe")
        # the LBA erasures, in the order of the lists
        erase = (r.rand(a["nobs"]) < 0.3) & (a["obs_live"] != 0)
        owner = np.repeat(np.arange(npoints), np.diff(a["obs_start"]))
        W = R.World(a)
        R.lba_erase(W, [(int(a["obs_frame"][o]), int(owner[o])) for o in np.nonzero(erase)[0]])
        edits = pg.map_edits_from_lba_erase(a["obs_start"], a["obs_frame"], erase)
        assert not _same_state(_state(W, cap), _after_edits(a, edits)), (c.name, "lba")
        # CorrectLoop's matched points
        matched = np.where(r.rand(cap) < 0.4, r.randint(0, npoints, cap), -1)
        W = R.World(a)
        R.loop_matches(W, kf, matched)
        edits = pg.map_edits_from_loop_matches(a["kf_point"][kf], kf, matched, npoints)
        assert not _same_state(_state(W, cap), _after_edits(a, edits)), (c.name, "loop")
        # Fuse's tail: distinct good queries that are not in the key frame, a few of them on one slot
        good = [p for p in range(npoints) if not a["point_bad"][p] and not np.any(a["obs_frame"][a["obs_start"][p]:a["obs_start"][p + 1]][
            a["obs_live"][a["obs_start"][p]:a["obs_start"][p + 1]] != 0] == kf)]
        queries = [int(q) for q in r.permutation(good)[:8]]
        best = [int(r.choice([-1, 0, 0, 1, 2, 3])) for _ in queries]
        W = R.World(a)
        action = R.fuse_tail(W, kf, queries, best)
        edits = pg.map_edits_from_fuse(a["kf_point"][kf], kf, queries, action, best)
        assert not _same_state(_state(W, cap), _after_edits(a, edits)), (c.name, "fuse")
        W = R.World(a)
        action, rep = R.fuse_sim3_and_replace(W, kf, queries, best)
        edits = pg.map_edits_from_fuse(a["kf_point"][kf], kf, queries, action, best, replace_point=rep)
        assert not _same_state(_state(W, cap), _after_edits(a, edits)), (c.name, "fuse_sim3")


def test_observation_ids_restatement():
    import pilotguru_amd as pg
    ids = pg.observation_ids([0, 3, 3, 5], [2, 0, 1, 1, 2], np.array([50, 7, 9], np.uint64))
    assert ids.dtype == np.uint64 and list(ids) == [7, 9, 50, 7, 9]


class _NoLibrary:
    class _L:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)
    _L = _L()
    _h = None

    @staticmethod
    def _check(rc):
        return rc


def test_python_mirror_refuses_malformed_input_without_a_device(cases):
    import pilotguru_amd as pg
    c = by_name(cases, "fuse_chain_on_one_slot")
    a = c.a
    n = len(a["obs_start"]) - 1

    def call(**kw):
        v = dict(edits=c.edits, slots=[a["kf_point"][f] for f in range(5)], npoints=n, bad=a["point_bad"], st=a["obs_start"], of=a["obs_frame"], oi=a["obs_idx"],
                 live=a["obs_live"], ref=a["ref_obs"], order=a["order"], cap_out=None, sel_cap=None)
        v.update(kw)
        return pg.apply_map_edits(_NoLibrary(), v["edits"], v["slots"], v["npoints"], v["bad"], a["visible"], a["found"], a["replaced"], v["st"], v["of"], v["oi"],
                                  v["live"], v["ref"], kf_order=v["order"], obs_cap_out=v["cap_out"], sel_cap=v["sel_cap"])
    unknown = c.edits.copy()
    unknown["op"][1] = 5
    start = a["obs_start"].copy()
    start[1] = 3
    twice = a["obs_frame"].copy()
    twice[1] = twice[0]
    for kw in (dict(edits=unknown), dict(edits=np.full(R.MAX_EDITS + 1, 1, np.int32).astype(R.EDIT_DTYPE)), dict(npoints=-1), dict(npoints=n + 1), dict(bad=a["point_bad"][:2]),
               dict(st=start), dict(st=a["obs_start"] + 1), dict(of=twice), dict(of=np.full(a["nobs"], 5, np.int32)), dict(oi=np.full(a["nobs"], 8, np.int32)),
               dict(oi=a["obs_idx"][:-1]), dict(live=a["obs_live"][:-1]), dict(ref=np.full(n, 3, np.int32)), dict(ref=np.full(n, -2, np.int32)),
               dict(order=[0, 1, 2, 3, 3]), dict(order=[0, 1, 2]), dict(cap_out=-1), dict(sel_cap=-1)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(AssertionError, match="the library was called"):
        call()
    with pytest.raises(ValueError):
        pg.LocalMapping.ProcessNewKeyFrame(_NoLibrary(), 5, [a["kf_point"][f] for f in range(5)], n, a["point_bad"], a["visible"], a["found"], a["replaced"],
                                           a["obs_start"], a["obs_frame"], a["obs_idx"], a["obs_live"], a["ref_obs"])


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
    MapPointObservations obs;
    obs.obsStart = {0, 2, 4};
    obs.obsFrame = {0, 1, 1, 2};
    obs.obsIdx = {0, 0, 1, 0};
    obs.refObs = {0, 0};
    LocalMapping lm(nullptr);
    std::vector<pgorb_map_edit> edits = {{PGORB_EDIT_REPLACE, 0, 1, 0}, {PGORB_EDIT_ADD, 1, 0, 1}};
    auto go = [&](std::vector<pgorb_map_edit> e, MapPointObservations ob, std::vector<uint8_t> live, std::vector<int32_t> order, size_t npoints, bool alias) {
        std::vector<std::vector<int32_t>> s = slots;
        std::vector<uint8_t> bad(npoints, 0);
        std::vector<int32_t> visible(2, 1), found(2, 1), replaced(2, -1), status, touched, selected;
        MapPointObservations out;
        lm.ApplyMapEdits(e, s, order, bad, visible, found, replaced, ob, live, alias ? ob : out, status, touched, PGORB_EDIT_TOUCH_CHANGED, selected);
    };
    MapPointObservations twice = obs; twice.obsFrame = {0, 0, 1, 2};
    MapPointObservations range = obs; range.obsFrame = {0, 3, 1, 2};
    MapPointObservations idx = obs; idx.obsIdx = {0, 0, 2, 0};
    MapPointObservations start = obs; start.obsStart = {0, 3, 2};
    MapPointObservations ref = obs; ref.refObs = {0, 2};
    std::vector<pgorb_map_edit> unknown = edits; unknown[0].op = 5;
    run("well_formed", [&] { go(edits, obs, {}, {}, 2, false); });
    run("masked_duplicate_is_no_duplicate", [&] { go(edits, twice, {1, 0, 1, 1}, {2, 0, 1}, 2, false); });
    run("unknown_op", [&] { go(unknown, obs, {}, {}, 2, false); });
    run("too_many_edits", [&] { go(std::vector<pgorb_map_edit>(PGORB_EDIT_MAX_EDITS + 1, pgorb_map_edit{PGORB_EDIT_ADD, 0, 0, 0}), obs, {}, {}, 2, false); });
    run("obs_twice", [&] { go(edits, twice, {}, {}, 2, false); });
    run("obs_range", [&] { go(edits, range, {}, {}, 2, false); });
    run("obs_idx", [&] { go(edits, idx, {}, {}, 2, false); });
    run("obs_start", [&] { go(edits, start, {}, {}, 2, false); });
    run("ref_obs", [&] { go(edits, ref, {}, {}, 2, false); });
    run("live_short", [&] { go(edits, obs, {1, 1}, {}, 2, false); });
    run("order_twice", [&] { go(edits, obs, {}, {0, 0, 1}, 2, false); });
    run("order_short", [&] { go(edits, obs, {}, {0, 1}, 2, false); });
    run("point_count", [&] { go(edits, obs, {}, {}, 3, false); });
    run("aliased_output", [&] { go(edits, obs, {}, {}, 2, true); });
    return 0;
}
"""


def test_cpp_mirror_rejects_bad_inputs_before_calling_the_library(tmp_path):
    """pgorb::LocalMapping::ApplyMapEdits throws std::invalid_argument for what pgorb_apply_map_edits would refuse, before any pointer
    reaches the library; well-formed input reaches it (a NULL context here, so PGORB_E_ARG comes back as std::runtime_error)."""
    import subprocess
    src, exe = os.path.join(str(tmp_path), "edit_driver.cc"), os.path.join(str(tmp_path), "edit_driver")
    open(src, "w").write(CPP_DRIVER)
    lib = os.path.join(ROOT, "pilotguru_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", ROOT, src, "-o", exe, "-L", lib, "-lpgorb", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    got = dict(l.split() for l in subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines())
    assert got.pop("well_formed") == "runtime_error" and got.pop("masked_duplicate_is_no_duplicate") == "runtime_error", got
    assert len(got) == 12 and set(got.values()) == {"invalid_argument"}, got


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    return pg.ORBextractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240)


def _check_both_forms(c, ext, e, host=True):
    got = K.download(K.run_device(c, ext, e))
    assert K.same(got, e), (c.name, "device", K.diff(got, e))
    if host:
        h = K.run_host(c, ext, e)
        assert K.same(h, e), (c.name, "host", K.diff(h, e))
        assert h["returned"] == (0 if e["info"][0] == R.LIMIT else e["info"][2])
        for k in K.KEYS:
            assert np.asarray(h[k]).tobytes() == np.asarray(got[k]).tobytes(), (c.name, k)


@pytest.mark.gpu
def test_gpu_constructed_cases_equal_the_reference_in_both_forms(ext, cases):
    for c in cases:
        _check_both_forms(c, ext, K.expected(c))


@pytest.mark.gpu
def test_gpu_random_worlds_equal_the_reference_in_both_forms(ext, randoms):
    for c, e in randoms:
        _check_both_forms(c, ext, e)


@pytest.mark.gpu
def test_gpu_same_bytes_on_a_second_stream_on_a_repeat_and_with_nops_in_between(ext, cases, randoms):
    import torch
    for c, e in [(by_name(cases, n), None) for n in ("fuse_chain_on_one_slot", "dangling_slot_collision", "two_new_points_on_one_idx2")] + randoms[:12]:
        e = e or K.expected(c)
        first = K.download(K.run_device(c, ext, e))
        again = K.download(K.run_device(c, ext, e))
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            d = K.run_device(c, ext, e, stream=st)
        st.synchronize()
        other = K.download(d)
        for k in K.KEYS:
            assert first[k].tobytes() == again[k].tobytes() == other[k].tobytes(), (c.name, k)
        cp, at = K.padded(c, len(c.edits))
        ep = K.expected(cp)
        pad = K.download(K.run_device(cp, ext, ep))
        assert K.same(pad, ep), (cp.name, K.diff(pad, ep))
        for k in K.KEYS:
            if k not in ("edit_status",):
                assert pad[k].tobytes() == first[k].tobytes(), (cp.name, k)
        assert np.array_equal(pad["edit_status"][at], first["edit_status"][:len(c.edits)][c.edits["op"] != R.NOP]) and not pad["edit_status"][:len(cp.edits)][
            np.setdiff1d(np.arange(len(cp.edits)), at)].any()


@pytest.mark.gpu
def test_gpu_edit_count_on_the_device_and_no_mask(ext, randoms):
    """d_nedits bounds the list from the device; d_obs_live NULL means every entry lives"""
    for c, _ in randoms[:20]:
        k = len(c.edits) // 2
        short = dataclasses.replace(c, edits=c.edits[:k])
        e = K.expected(short)
        d = K.upload(c, dict(e))
        _, _, s = K.sentinel(dataclasses.replace(c, obs_cap_out=e["obs_cap_out"], sel_cap=e["sel_cap"]))
        d["edit_status"] = K.dev(s["edit_status"])
        got = K.download(K.run_device(c, ext, e, d=d, nedits_dev=K.dev(np.array([k], np.int32))))
        assert np.array_equal(got["edit_status"][:k], e["edit_status"][:k]) and not got["edit_status"][k:len(c.edits)].any()
        got["edit_status"] = e["edit_status"]
        assert K.same(got, e), (c.name, K.diff(got, e))
        a = dict(c.a, obs_live=np.ones_like(c.a["obs_live"]))
        full = dataclasses.replace(c, a=a)
        e = K.expected(full)
        got = K.download(K.run_device(full, ext, e, live=False))
        assert K.same(got, e), (c.name, "no mask", K.diff(got, e))


@pytest.mark.gpu
def test_gpu_capacities_exact_and_one_past(ext, cases):
    from pilotguru_amd import _lib
    c = by_name(cases, "fuse_chain_on_one_slot")
    e = K.expected(c)                                               # obs_cap_out exact: the default of every case
    assert e["obs_cap_out"] == e["info"][1] and e["info"][0] == 0
    for short in (dataclasses.replace(c, obs_cap_out=int(e["info"][1]) - 1), dataclasses.replace(c, sel_cap=int(e["info"][7]) - 1)):
        want = K.expected(short)
        assert want["info"][0] == R.LIMIT and np.all(want["info"][1:] == K.SENT)
        _check_both_forms(short, ext, want)                         # every in/out byte unchanged, every output byte the sentinel
    exact = dataclasses.replace(c, sel_cap=int(e["info"][7]))
    _check_both_forms(exact, ext, K.expected(exact))
    full, past = _bag_case(0), _bag_case(1)
    e = K.expected(full)
    assert e["info"][0] == 0 and e["info"][1] == R.MAX_BAG + 2
    _check_both_forms(full, ext, e)
    e = K.expected(past)
    assert e["info"][0] == R.LIMIT
    _check_both_forms(past, ext, e)
    c = _full_list_case()
    e = K.expected(c)
    assert e["info"][0] == 0 and e["info"][2] > R.MAX_EDITS - 64
    _check_both_forms(c, ext, e)
    more = dataclasses.replace(c, edits=np.concatenate([c.edits[:100], K.E((R.NOP,)), c.edits[100:]]))      # a NOP more is no edit more
    _check_both_forms(more, ext, K.expected(more))
    over = dataclasses.replace(c, edits=np.concatenate([c.edits, K.E((R.ADD, 0, 0, 0))]))
    e = K.expected(over)
    assert e["info"][0] == R.LIMIT
    got = K.download(K.run_device(over, ext, e))                    # the device form learns the count on the device: LIMIT, nothing written
    assert K.same(got, e), K.diff(got, e)
    with pytest.raises(AssertionError) as x:
        K.run_host(over, ext, e)
    assert x.value.args[0][0] == _lib.PGORB_E_LIMIT
    with pytest.raises(AssertionError) as x:
        K.run_device(dataclasses.replace(c, edits=np.zeros(R.MAX_LIST + 1, R.EDIT_DTYPE)), ext, e)
    assert x.value.args[0][0] == _lib.PGORB_E_LIMIT


@pytest.mark.gpu
def test_gpu_lists_as_long_as_the_producers_write_them_at_2000_keypoints(ext):
    """the list length is the producer's array, not the number of edits: 3 * cap entries after CreateNewMapPoints and nobs entries
    after the local bundle adjustment, at cap_per_frame = 2000, both longer than MAX_EDITS and mostly NOP"""
    for c in _wide_cases():
        assert len(c.edits) > R.MAX_EDITS
        e = K.expected(c)
        assert e["info"][0] == 0 and e["info"][2] >= 300
        _check_both_forms(c, ext, e)


@pytest.mark.gpu
def test_gpu_host_form_refuses_malformed_input(ext, cases):
    from pilotguru_amd import _lib
    c = by_name(cases, "fuse_chain_on_one_slot")
    e = K.expected(c)

    def host(change=None, edits=None, **kw):
        a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.a.items()}
        if change:
            change(a)
        try:
            K.run_host(dataclasses.replace(c, a=a, edits=c.edits if edits is None else edits), ext, dict(e, **kw))
        except AssertionError as x:
            return x.args[0][0]
        return 0

    def setv(k, i, v):
        return lambda a: a[k].__setitem__(i, v)
    unknown = c.edits.copy()
    unknown["op"][0] = 5
    negative = c.edits.copy()
    negative["op"][0] = -1
    assert host() == 0
    for i, ch in enumerate([setv("n", 0, -1), setv("obs_start", 0, 1), setv("obs_start", 2, 0), setv("obs_frame", 0, 5), setv("obs_frame", 1, int(c.a["obs_frame"][0])),
                            setv("obs_idx", 0, 8), setv("obs_idx", 0, -1), setv("ref_obs", 0, 2), setv("ref_obs", 0, -2), setv("order", 0, 0), setv("order", 0, 5)]):
        assert host(ch) == _lib.PGORB_E_ARG, i
    assert host(edits=unknown) == _lib.PGORB_E_ARG and host(edits=negative) == _lib.PGORB_E_ARG
    assert host(obs_cap_out=-1) == _lib.PGORB_E_ARG and host(sel_cap=-1) == _lib.PGORB_E_ARG
    # outputs over inputs
    a = c.a
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    n, m = len(a["obs_start"]) - 1, a["nobs"]
    slots = [a["kf_point"][f].copy() for f in range(5)]
    ptrs = (C.c_void_p * 5)(*[s.ctypes.data for s in slots])
    buf = {k: np.zeros(16, np.int32) for k in ("so", "fo", "io", "ro", "st", "t", "sel", "info")}

    def alias(**kw):
        v = dict(so=buf["so"], fo=buf["fo"], io=buf["io"], ro=buf["ro"])
        v.update(kw)
        return ext._L.pgorb_apply_map_edits(ext._h, p(c.edits), len(c.edits), 5, ptrs, p(a["n"]), p(a["order"]), n, p(a["point_bad"].copy()), p(a["visible"].copy()),
                                            p(a["found"].copy()), p(a["replaced"].copy()), p(a["obs_start"]), p(a["obs_frame"]), p(a["obs_idx"]), p(a["obs_live"]),
                                            p(a["ref_obs"]), m + 1, p(v["so"]), p(v["fo"]), p(v["io"]), p(v["ro"]), p(buf["st"]), p(buf["t"]), 3, n, p(buf["sel"]),
                                            p(buf["info"]))
    assert alias() >= 0
    big = lambda x: np.concatenate([x, np.zeros(8, np.int32)])
    st2, of2, oi2, ro2 = big(a["obs_start"]), big(a["obs_frame"]), big(a["obs_idx"]), big(a["ref_obs"])
    a2 = dict(a, obs_start=st2, obs_frame=of2, obs_idx=oi2, ref_obs=ro2)
    a, keep = a2, a
    assert alias(so=st2) == _lib.PGORB_E_ARG and alias(fo=of2) == _lib.PGORB_E_ARG and alias(io=oi2[1:]) == _lib.PGORB_E_ARG and alias(ro=ro2) == _lib.PGORB_E_ARG
    assert alias(fo=oi2) == _lib.PGORB_E_ARG


@pytest.mark.gpu
def test_gpu_python_mirror_returns_what_the_host_form_leaves(ext, cases):
    import pilotguru_amd as pg
    c = by_name(cases, "fuse_chain_on_one_slot")
    a, e = c.a, K.expected(c)
    n = len(a["obs_start"]) - 1
    r = pg.apply_map_edits(ext, c.edits, [a["kf_point"][f] for f in range(5)], n, a["point_bad"], a["visible"], a["found"], a["replaced"], a["obs_start"],
                           a["obs_frame"], a["obs_idx"], a["obs_live"], a["ref_obs"], kf_order=a["order"], select_bits=c.select_bits)
    total = int(e["info"][1])
    assert r["applied"] == 3 and np.array_equal(r["info"], e["info"][:R.INFO]) and np.array_equal(r["obs_start"], e["obs_start_out"][:n + 1])
    assert np.array_equal(r["obs_frame"], e["obs_frame_out"][:total]) and np.array_equal(r["obs_idx"], e["obs_idx_out"][:total])
    assert np.array_equal(r["ref_obs"], e["ref_obs_out"][:n]) and list(r["select"]) == [0, 1, 2] and np.array_equal(r["touched"], e["touched"][:n])
    assert all(np.array_equal(r["kf_point"][f], e["kf_point"][f]) for f in range(5)) and np.array_equal(r["point_bad"], e["point_bad"])
    assert np.array_equal(r["found"], e["found"]) and np.array_equal(r["replaced"], e["replaced"]) and not a["point_bad"].any()
    c = by_name(cases, "point_in_two_slots_of_a_new_key_frame")
    a, e = c.a, K.expected(c)
    r = pg.LocalMapping.ProcessNewKeyFrame(ext, 4, [a["kf_point"][f] for f in range(5)], 2, a["point_bad"], a["visible"], a["found"], a["replaced"],
                                           a["obs_start"], a["obs_frame"], a["obs_idx"], a["obs_live"], a["ref_obs"], kf_order=a["order"])
    assert list(r["slot_class"]) == [0, 1, 1, 0, 0, 2, 0, 0] and np.array_equal(r["obs_start"], e["obs_start_out"][:3]) and list(r["select"]) == [0, 1]
    r = pg.apply_map_edits(ext, c.edits, [a["kf_point"][f] for f in range(5)], 2, a["point_bad"], a["visible"], a["found"], a["replaced"], a["obs_start"],
                           a["obs_frame"], a["obs_idx"], a["obs_live"], a["ref_obs"], kf_order=a["order"], obs_cap_out=4)
    assert r["info"][0] == R.LIMIT and r["obs_start"] is None and r["applied"] == 0


# ---------------------------------------------------------------- the device producers against their numpy forms
def _edits_of(t, k):
    return np.frombuffer(t.cpu().numpy().tobytes(), R.EDIT_DTYPE)[:k]


def _sent_edits(k):
    import torch
    return torch.full((4 * (k + 2),), K.SENT, dtype=torch.int32, device="cuda")


@pytest.mark.gpu
def test_gpu_producers_equal_their_numpy_forms(ext, randoms):
    import torch
    import pilotguru_amd as pg
    L, h, q = ext._L, ext._h, K.ptr
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    full = lambda k: torch.full((k,), K.SENT, dtype=torch.int32, device="cuda")
    tail_ok = lambda t, k: bool(np.all(t.cpu().numpy()[k:] == K.SENT))
    for c, _ in randoms[:60]:
        a = _clean(c)
        r = np.random.RandomState(7 + len(c.edits))
        nkf, npoints, cap, m = len(a["n"]), len(a["obs_start"]) - 1, a["cap"], a["nobs"]
        kf = int(r.randint(nkf))
        for i in r.choice(cap, 4, replace=False):
            a["kf_point"][kf, i] = r.randint(-1, npoints + 1)
        a["kf_point"][kf, r.randint(cap)] = a["kf_point"][kf, 0]
        a["n"][kf] = cap - 1                                       # the last slot is past the key frame's count
        d = {k: K.dev(a[k]) for k in ("kf_point", "n", "point_bad", "obs_start", "obs_frame", "obs_live")}
        # ProcessNewKeyFrame
        ed, cls = _sent_edits(cap), full(cap + 2)
        assert L.pgorb_map_edits_from_keyframe_device(h, q(d["kf_point"]), q(d["n"]), nkf, cap, npoints, q(d["point_bad"]), q(d["obs_start"]), q(d["obs_frame"]), m,
                                                      q(d["obs_live"]), kf, q(ed), q(cls), s) == 0
        want, wcls = pg.map_edits_from_keyframe(a["kf_point"][kf, :cap - 1], npoints, a["point_bad"], a["obs_start"], a["obs_frame"], a["obs_live"], kf, cap=cap)
        assert np.array_equal(_edits_of(ed, cap), want) and np.array_equal(cls.cpu().numpy()[:cap], wcls) and tail_ok(ed, 4 * cap) and tail_ok(cls, cap), c.name
        # the LBA erasures
        erase = (r.rand(max(m, 1)) < 0.3).astype(np.uint8)
        ed = _sent_edits(m)
        assert L.pgorb_map_edits_from_lba_erase_device(h, npoints, q(d["obs_start"]), q(d["obs_frame"]), m, q(K.dev(erase)), q(ed), s) == 0
        assert np.array_equal(_edits_of(ed, m), pg.map_edits_from_lba_erase(a["obs_start"], a["obs_frame"], erase)) and tail_ok(ed, 4 * m), c.name
        # CorrectLoop's matched points
        matched = np.where(r.rand(cap) < 0.5, r.randint(-1, npoints + 2, cap), -1).astype(np.int32)
        ed = _sent_edits(cap)
        assert L.pgorb_map_edits_from_loop_matches_device(h, q(d["kf_point"]), q(d["n"]), nkf, cap, npoints, kf, q(K.dev(matched)), q(ed), s) == 0
        assert np.array_equal(_edits_of(ed, cap), np.concatenate([pg.map_edits_from_loop_matches(a["kf_point"][kf, :cap - 1], kf, matched, npoints),
                                                                  np.zeros(1, R.EDIT_DTYPE)])) and tail_ok(ed, 4 * cap), c.name
        # Fuse, both forms: qcap 12, 9 queries
        qcap, nq = 12, 9
        queries = r.randint(-1, npoints, qcap).astype(np.int32)
        action = r.choice([0, 1, 2, 3, 4, 5], qcap).astype(np.int32)
        best = r.choice([-1, 0, 0, 1, 1, 2, cap - 1, cap], qcap).astype(np.int32)
        dq, da, db, dn = K.dev(queries), K.dev(action), K.dev(best), K.dev(np.array([nq], np.int32))
        ed = _sent_edits(qcap)
        assert L.pgorb_map_edits_from_fuse_device(h, q(d["kf_point"]), q(d["n"]), nkf, cap, npoints, kf, qcap, q(dn), q(dq), q(da), q(db), None, q(ed), s) == 0
        want = pg.map_edits_from_fuse(a["kf_point"][kf, :cap - 1], kf, queries[:nq], action[:nq], best[:nq], qcap=qcap)
        assert np.array_equal(_edits_of(ed, qcap), want) and tail_ok(ed, 4 * qcap), c.name
        action3 = np.where(action >= 3, 6, action).astype(np.int32)
        rep = np.where(action3 == 6, r.randint(0, npoints, qcap), -1).astype(np.int32)
        ed = _sent_edits(2 * qcap)
        assert L.pgorb_map_edits_from_fuse_device(h, q(d["kf_point"]), q(d["n"]), nkf, cap, npoints, kf, qcap, q(dn), q(dq), q(K.dev(action3)), q(db), q(K.dev(rep)),
                                                  q(ed), s) == 0
        want = pg.map_edits_from_fuse(a["kf_point"][kf, :cap - 1], kf, queries[:nq], action3[:nq], best[:nq], replace_point=rep, qcap=qcap)
        assert np.array_equal(_edits_of(ed, 2 * qcap), want) and tail_ok(ed, 8 * qcap), c.name
        # the ids of the lists
        ids = torch.full((m + 2,), K.SENT, dtype=torch.int64, device="cuda")
        assert L.pgorb_observation_ids_device(h, npoints, q(d["obs_start"]), q(d["obs_frame"]), m, q(K.dev(a["kf_id"].view(np.int64))), nkf, q(ids), s) == 0
        got = ids.cpu().numpy()
        assert np.array_equal(got[:m].astype(np.uint64), pg.observation_ids(a["obs_start"], a["obs_frame"], a["kf_id"])) and np.all(got[m:] == K.SENT), c.name


# ---------------------------------------------------------------- chains on resident arrays
@pytest.mark.gpu
def test_gpu_chain_fuse_edit_refresh_ids_for_three_targets(ext):
    """SearchInNeighbors' first loop on the device: pgorb_fuse_batch_device -> pgorb_map_edits_from_fuse_device ->
    pgorb_apply_map_edits_device -> pgorb_refresh_map_points_batch_device(d_select_out) -> pgorb_observation_ids_device -> the
    next target's Fuse, three targets, nothing read back before the end.  The final slots, table, lists and descriptors are those
    of the sequential reference objects (tests/fuse_reference.py: Fuse with Replace and ComputeDistinctiveDescriptors), and each
    target's row equals Fuse's own d_kf_point_out."""
    import torch
    import fuse_cases as FC
    import fuse_reference as FR
    from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE, MP_DESCRIPTOR
    current, targets, points = FC.neighbourhood(3, ntargets=3, npts=70)
    kfs = [current] + targets
    nframes, npoints = len(kfs), len(points)
    nk = np.array([len(k.keys) for k in kfs], np.int32)
    cap = int(nk.max()) + 2
    assert cap <= 64 + 2 and [k.id for k in kfs] == [1000 + f for f in range(nframes)]      # ids rise with the index: address rank = index
    kp = np.zeros((nframes, cap), KEYPOINT_DTYPE)
    kp["x"], kp["y"] = np.nan, np.nan
    ds = np.full((nframes, cap, 32), 0xFF, np.uint8)
    slots = np.full((nframes, cap), -1, np.int32)
    poses = np.zeros(nframes, KF_POSE_DTYPE)
    for f, k in enumerate(kfs):
        kp[f, :nk[f]], ds[f, :nk[f]], poses[f] = k.keys, k.desc, k.pose
        slots[f, :nk[f]] = [-1 if s is None else s.id for s in k.slots]
    pts, pd, pb, st, ob = FC.table_arrays(points)
    of = np.array([k.id - 1000 for p in points for k in sorted(p.obs)], np.int32)
    oi = np.array([p.obs[k] for p in points for k in sorted(p.obs)], np.int32)
    queries = np.array([-1 if s is None else s.id for s in current.slots], np.int32)
    qcap, nobs0 = len(queries) + 3, len(of)
    ocap = nobs0 + 3 * qcap
    Q = np.full(qcap, 0x7FFF0000, np.int32)
    Q[:len(queries)] = queries
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    full = lambda *shape: torch.full(shape, K.SENT, dtype=torch.int32, device="cuda")
    q = K.ptr
    L, h = ext._L, ext._h
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pad = lambda x, k, dt: np.concatenate([x, np.zeros(k - len(x), dt)])
    dk, dd, dn, dslots, dpose = T(kp.view(np.uint8).reshape(nframes, cap, 28)), T(ds), T(nk), T(slots), T(poses.view(np.uint8))
    dids, dkfbad = T(np.array([k.id for k in kfs], np.uint64).view(np.int64)), T(np.zeros(nframes, np.uint8))
    dpts, dpd, dpb = T(pts.view(np.uint8)), T(pd), T(pb)
    dvis, dfound, drepl = T(np.ones(npoints, np.int32)), T(np.ones(npoints, np.int32)), T(np.full(npoints, -1, np.int32))
    csr = [dict(start=T(st), frame=T(pad(of, ocap, np.int32)), idx=T(pad(oi, ocap, np.int32)), ref=T(np.zeros(npoints, np.int32)),
                kf=T(pad(ob.view(np.int64), ocap, np.int64))),
           dict(start=full(npoints + 1), frame=full(ocap), idx=full(ocap), ref=full(npoints), kf=torch.zeros(ocap, dtype=torch.int64, device="cuda"))]
    gs, gi = torch.zeros((nframes, 3073), dtype=torch.int32, device="cuda"), torch.zeros((nframes, cap), dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_frame_grid_batch_device(h, q(dk), q(dn), nframes, cap, *FC.BOUNDS, q(gs), q(gi), s))
    dQ, dnq = T(Q), T(np.array([len(queries)], np.int32))
    rows, outs, infos, keep = [], [], [], []
    for t in range(1, nframes):
        a, b = csr[(t - 1) % 2], csr[t % 2]
        act, bi, bd, so, nf = full(qcap), full(qcap), full(qcap), full(cap), full(1)
        edits, status, touched, select, info = full(4 * qcap), full(qcap), full(npoints), full(npoints), full(R.INFO)
        best, mstat, dkf = full(npoints), full(npoints), T(np.array([t], np.int32))
        keep += [act, bi, bd, nf, edits, status, touched, select, best, mstat, dkf]
        ext._check(L.pgorb_fuse_batch_device(h, q(dk), q(dd), q(dn), cap, q(gs), q(gi), q(dkf), 1, q(dids), q(dpose), *FC.BOUNDS, q(dslots), npoints, q(dpts),
                                             q(dpd), q(dpb), q(a["start"]), q(a["kf"]), qcap, q(dnq), q(dQ), 3.0, q(act), q(bi), q(bd), q(so), q(nf), s))
        ext._check(L.pgorb_map_edits_from_fuse_device(h, q(dslots), q(dn), nframes, cap, npoints, t, qcap, q(dnq), q(dQ), q(act), q(bi), None, q(edits), s))
        ext._check(L.pgorb_apply_map_edits_device(h, q(edits), qcap, None, q(dslots), q(dn), nframes, cap, None, npoints, q(dpb), q(dvis), q(dfound), q(drepl),
                                                  q(a["start"]), q(a["frame"]), q(a["idx"]), ocap, None, q(a["ref"]), ocap, q(b["start"]), q(b["frame"]),
                                                  q(b["idx"]), q(b["ref"]), q(status), q(touched), R.TOUCH_SURVIVOR, npoints, q(select), q(info), s))
        ext._check(L.pgorb_refresh_map_points_batch_device(h, q(dk), q(dd), q(dn), nframes, cap, q(dpose), q(dkfbad), npoints, q(dpts), q(dpd), q(dpb),
                                                           q(b["start"]), q(b["frame"]), q(b["idx"]), ocap, q(b["ref"]), npoints, q(select), MP_DESCRIPTOR,
                                                           q(best), q(mstat), s))
        ext._check(L.pgorb_observation_ids_device(h, npoints, q(b["start"]), q(b["frame"]), ocap, q(dids), nframes, q(b["kf"]), s))
        rows.append(dslots[t].clone())
        outs.append(so)
        infos.append(info)
    torch.cuda.synchronize()
    # the sequential reference on the objects
    vp = list(current.slots)
    for kf in targets:
        FR.fuse(kf, vp, 3.0)
    final = csr[(nframes - 1) % 2]
    got_slots, got_st = dslots.cpu().numpy(), final["start"].cpu().numpy()
    got_of, got_oi, got_kf = final["frame"].cpu().numpy(), final["idx"].cpu().numpy(), final["kf"].cpu().numpy()
    got_pd, got_pb, got_found, got_vis = dpd.cpu().numpy(), dpb.cpu().numpy(), dfound.cpu().numpy(), dvis.cpu().numpy()
    merged = 0
    for t in range(1, nframes):
        assert infos[t - 1].cpu().numpy()[0] == 0
        merged += int(infos[t - 1].cpu().numpy()[2])
        assert np.array_equal(rows[t - 1].cpu().numpy()[:nk[t]], outs[t - 1].cpu().numpy()[:nk[t]]), t       # the target's row is Fuse's own kf_point_out
    assert merged >= 6                                                     # the chain did something
    for f, k in enumerate(kfs):
        assert list(got_slots[f, :nk[f]]) == [-1 if x is None else x.id for x in k.slots], f
    for i, p in enumerate(points):
        lst = sorted((k.id, x) for k, x in p.obs.items())
        a, b = got_st[i], got_st[i + 1]
        assert [(int(f) + 1000, int(x)) for f, x in zip(got_of[a:b], got_oi[a:b])] == lst and list(got_kf[a:b]) == [k for k, _ in lst], i
        assert bool(got_pb[i]) == p.bad and got_pd[i].tobytes() == p.desc.tobytes() and got_found[i] == p.found and got_vis[i] == p.visible, i


@pytest.mark.gpu
def test_gpu_chain_local_bundle_adjustment_erase_edit_update_connections(ext):
    """pgorb_local_bundle_adjustment_batch_device -> pgorb_map_edits_from_lba_erase_device -> pgorb_apply_map_edits_device ->
    pgorb_update_connections_batch_device on one stream, nothing read back before the end: the slots, flags and lists are those of
    the reference objects after Optimizer.cc:748-757 with the same erasures, and the graph rows are the bytes of the same call fed
    that state."""
    import torch
    import lba_cases as LC
    from pilotguru_amd.orb import COVIS_INFO, KEYPOINT_DTYPE, Optimizer
    P, rounds = LC.case("outliers")
    nf, npts, nobs = P.nframes, len(P.pos), len(P.obs_frame)
    n = np.array([len(o) for o in P.octaves], np.int32)
    cap = int(n.max()) + 3
    assert cap <= 64 + 3
    kp = np.zeros((nf, cap), KEYPOINT_DTYPE)
    kp["x"], kp["y"], kp["octave"] = np.nan, np.nan, 99
    slots = np.full((nf, cap), -1, np.int32)
    for f in range(nf):
        kp[f, :n[f]], slots[f, :n[f]] = LC.keypoints(P.keys_xy[f], P.octaves[f]), P.kf_point[f]
    poses, pts = LC.pose_records(P), LC.table(P)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    full = lambda *shape: torch.full(shape, K.SENT, dtype=torch.int32, device="cuda")
    q = K.ptr
    L, h = ext._L, ext._h
    st = torch.cuda.current_stream()
    s = C.c_void_p(st.cuda_stream)
    d_kps, d_n, d_pose = T(kp.view(np.uint8).reshape(nf, cap, KEYPOINT_DTYPE.itemsize)), T(n), T(poses.view(np.uint8).reshape(nf, -1))
    d_slots, d_pts, d_os, d_of, d_oi = T(slots), T(pts.view(np.uint8).reshape(npts, -1)), T(P.obs_start), T(P.obs_frame), T(P.obs_idx)
    d_pb, d_kb, d_id = T(np.asarray(P.point_bad, np.uint8)), T(np.asarray(P.kf_bad, np.uint8)), T(np.asarray(P.fixed_id0, np.uint8))
    d_ws, d_wk = T(np.array([0, len(P.local_kf)], np.int32)), T(np.asarray(P.local_kf, np.int32))
    vis, found = np.arange(3, 3 + npts, dtype=np.int32), np.arange(1, 1 + npts, dtype=np.int32)
    ref = np.where(np.diff(P.obs_start) > 0, 0, -1).astype(np.int32)
    d_vis, d_found, d_repl, d_ref = T(vis), T(found), T(np.full(npts, -1, np.int32)), T(ref)
    conn_cap, th = 8, 2

    def graph():
        g = dict(conn_kf=T(np.full((nf, conn_cap), -1, np.int32)), conn_w=T(np.zeros((nf, conn_cap), np.int32)), nconn=T(np.zeros(nf, np.int32)),
                 ord_kf=T(np.full((nf, conn_cap), -1, np.int32)), ord_w=T(np.zeros((nf, conn_cap), np.int32)), nord=T(np.zeros(nf, np.int32)),
                 parent=T(np.full(nf, -1, np.int32)), first=T(np.ones(nf, np.uint8)), status=full(nf), info=full(COVIS_INFO))
        return g

    def connections(g, kf_point, point_bad, start, frame):
        rc = L.pgorb_update_connections_batch_device(h, q(kf_point), q(d_n), nf, cap, npts, q(point_bad), q(start), q(frame), nobs, None, q(d_id), len(P.local_kf),
                                                     q(d_wk), th, conn_cap, *[q(g[k]) for k in ("conn_kf", "conn_w", "nconn", "ord_kf", "ord_w", "nord", "parent", "first",
                                                                                               "status")], 0, None, q(g["info"]), s)
        assert rc == 0, (rc, L.pgorb_last_error(h))
    out = Optimizer.LocalBundleAdjustment_batch_device(ext, d_kps, d_n, cap, d_pose, d_slots, d_ws, d_wk, npts, d_pts, d_os, d_of, d_oi, d_pb, d_kb, d_id, rounds,
                                                       stream=st.cuda_stream)
    edits, status, touched, select, info = full(4 * nobs), full(nobs), full(npts), full(npts), full(R.INFO)
    n_st, n_of, n_oi, n_ref = full(npts + 1), full(nobs), full(nobs), full(npts)
    ext._check(L.pgorb_map_edits_from_lba_erase_device(h, npts, q(d_os), q(d_of), nobs, q(out["erase"]), q(edits), s))
    ext._check(L.pgorb_apply_map_edits_device(h, q(edits), nobs, None, q(d_slots), q(d_n), nf, cap, None, npts, q(d_pb), q(d_vis), q(d_found), q(d_repl), q(d_os),
                                              q(d_of), q(d_oi), nobs, None, q(d_ref), nobs, q(n_st), q(n_of), q(n_oi), q(n_ref), q(status), q(touched),
                                              R.TOUCH_CHANGED, npts, q(select), q(info), s))
    g = graph()
    connections(g, d_slots, d_pb, n_st, n_of)
    torch.cuda.synchronize()
    erase = out["erase"].cpu().numpy()[0]
    assert int(erase.sum()) >= 10
    a = dict(n=n, order=None, cap=cap, kf_point=slots, point_bad=np.asarray(P.point_bad, np.uint8), visible=vis, found=found, replaced=np.full(npts, -1, np.int32),
             obs_start=np.asarray(P.obs_start, np.int32), obs_frame=np.asarray(P.obs_frame, np.int32), obs_idx=np.asarray(P.obs_idx, np.int32),
             obs_live=np.ones(nobs, np.uint8), ref_obs=ref, nobs=nobs)
    W = R.World(a)
    owner = np.repeat(np.arange(npts), np.diff(P.obs_start))
    R.lba_erase(W, [(int(P.obs_frame[o]), int(owner[o])) for o in np.nonzero(erase)[0]])
    t = R.table(W, cap)
    total = int(t["obs_start"][-1])
    inf = info.cpu().numpy()
    assert inf[0] == 0 and inf[1] == total and inf[5] == nobs - total and inf[2] <= int(erase.sum()) and inf[3] >= 1     # every entry that left cleared a slot; a point went bad
    assert np.array_equal(d_slots.cpu().numpy(), t["kf_point"]) and np.array_equal(d_pb.cpu().numpy(), t["point_bad"])
    assert np.array_equal(n_st.cpu().numpy(), t["obs_start"]) and np.array_equal(n_of.cpu().numpy()[:total], t["obs_frame"])
    assert np.array_equal(n_oi.cpu().numpy()[:total], t["obs_idx"]) and np.array_equal(n_ref.cpu().numpy(), t["ref_obs"])
    assert np.all(n_of.cpu().numpy()[total:] == K.SENT) and np.array_equal(d_vis.cpu().numpy(), vis) and np.array_equal(d_found.cpu().numpy(), found)
    fed = graph()
    pad = lambda x: np.concatenate([x, np.full(nobs - len(x), K.SENT, np.int32)])
    connections(fed, T(t["kf_point"]), T(t["point_bad"]), T(t["obs_start"]), T(pad(t["obs_frame"])))
    torch.cuda.synchronize()
    for k in g:
        assert g[k].cpu().numpy().tobytes() == fed[k].cpu().numpy().tobytes(), k
    assert int(g["nconn"].cpu().numpy().sum()) > 0
