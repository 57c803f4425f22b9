"""The covisibility graph on the GPU (pilotguru_amd/csrc/covisibility.hip; include/pgorb.h: KeyFrame::UpdateConnections of a list of
key frames with LoopConnections, and the views the other entry points read) against the literal object-level reference
(tests/covis_reference.py) on constructed cases and seeded random maps (tests/covis_cases.py).  Integers only: every comparison is
exact, unused row entries included."""
import copy
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import covis_cases as CC  # noqa: E402
import covis_reference as CR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pgorb_update_connections", "pgorb_update_connections_batch_device", "pgorb_covisibility_views_device",
         "pgorb_update_local_map", "pgorb_update_local_map_batch_device")
NRANDOM = 300


@pytest.fixture(scope="module")
def cases():
    return CC.graph_cases()


@pytest.fixture(scope="module")
def randoms():
    return [CC.random_world(s) for s in range(NRANDOM)]


def test_symbols_constants_and_null_context():
    from pilotguru_amd import _lib
    import pilotguru_amd as pg
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name)
    p = None
    assert L.pgorb_update_connections(p, 0, p, p, 0, p, p, p, p, p, 0, p, 15, 1, *([p] * 9), 0, p, p) == -1
    assert L.pgorb_update_connections_batch_device(p, p, p, 0, 1, 0, p, p, p, 0, p, p, 0, p, 15, 1, *([p] * 9), 0, p, p, p) == -1
    assert L.pgorb_covisibility_views_device(p, 0, 1, p, p, p, 10, p, 0, p, p, p, 0, p, p, p) == -1
    hdr = open(os.path.join(ROOT, "include", "pgorb.h")).read()
    defs = dict(re.findall(r"#define\s+PGORB_(COVIS_\w+|LOCALMAP_\w+)\s+(\d+)", hdr))
    assert len(defs) == 11
    for k, v in defs.items():
        assert getattr(pg, k) == int(v), k
    assert (CR.UPDATED, CR.RESORTED, CR.EMPTY, CR.FALLBACK, CR.PARENT_SET, CR.LIMIT, CR.MAX_KF, CR.MAX_CONN, CR.INFO, CR.NO_VOTES, CR.LM_LIMIT) == \
        tuple(int(defs[k]) for k in ("COVIS_UPDATED", "COVIS_RESORTED", "COVIS_EMPTY", "COVIS_FALLBACK", "COVIS_PARENT_SET", "COVIS_LIMIT",
                                     "COVIS_MAX_KF", "COVIS_MAX_CONN", "COVIS_INFO", "LOCALMAP_NO_VOTES", "LOCALMAP_LIMIT"))
    assert callable(pg.CovisibilityGraph.UpdateConnections) and callable(pg.Tracking.UpdateLocalMap)
    hpp = open(os.path.join(ROOT, "pilotguru_amd", "host", "orb_extractor.hpp")).read()
    assert "class CovisibilityGraph" in hpp and "UpdateLocalMap" in hpp and "pgorb_update_connections(" in hpp and "pgorb_update_local_map(" in hpp


def test_decomposition_equals_the_literal_sequence(cases, randoms):
    """the closed form csrc/covisibility.hip relies on, against one UpdateConnections after another."""
    for c in list(cases) + randoms:
        want, got = CC.expected_update(c), CC.expected_update(c, decomposed=True)
        assert CC.same_update(want, got, c.w.nkf), (c.name, CC.diff_update(got, want, c.w.nkf))


def test_every_graph_mutant_is_caught(cases, randoms):
    pool = [c for c in cases if c.w.nkf <= 100] + randoms[:80]
    want = [CC.expected_update(c) for c in pool]
    caught = {}
    for name, rules in CR.GRAPH_MUTANTS.items():
        caught[name] = [c.name for c, w in zip(pool, want) if not CC.same_update(w, CC.expected_update(c, rules), c.w.nkf)]
        assert caught[name], name
    # ... each on a constructed case, by name (with consistent slots c_ij == c_ji an earlier member's send meets its own value again:
    # sends_any_position can only show where the slots are inconsistent)
    for name, where in (("th_strict", "th_edge"), ("kfmax_last", "fallback_tied"), ("ties_ascending", "ties_whole_map"),
                        ("sends_any_position", "inconsistent_duplicate_bad"), ("unchanged_resorts", "unchanged_send"),
                        ("resort_from_sends", "changed_send"), ("map_only_sends", "th_edge"),
                        ("bad_points_counted", "inconsistent_duplicate_bad"), ("parent_for_id0", "ties_whole_map")):
        assert where in caught[name], (name, caught[name][:8])


def test_hand_written_expectations(cases):
    by = {c.name: c for c in cases}
    e = CC.expected_update(by["th_edge"])                     # th 3: counts 2, 3, 4 -> the map holds all three, the list the two at or above th
    assert e["nconn"][0] == 3 and list(e["conn_w"][0, :3]) == [2, 3, 4] and list(e["ord_kf"][0, :2]) == [3, 2] and e["nord"][0] == 2
    assert e["parent"][0] == 3 and e["first"][0] == 0 and e["status"][0] == CR.UPDATED | CR.PARENT_SET
    assert e["status"][1] == 0 and e["nconn"][1] == 0                                  # below th: no AddConnection
    assert e["status"][2] == CR.RESORTED and list(e["conn_kf"][2, :1]) == [0] and e["first"][2] == 1
    assert [tuple(r) for r in e["loop_conn"][:e["info"][1]]] == [(0, 1, 2), (0, 2, 3), (0, 3, 4)]
    e = CC.expected_update(by["fallback_tied"])               # ranks: kf 2 first, then 0, 3, 1; counters of kf 0: {1: 2, 2: 2, 3: 1}
    assert e["status"][0] == CR.UPDATED | CR.FALLBACK | CR.PARENT_SET and list(e["ord_kf"][0, :e["nord"][0]]) == [2]   # kf 2 sends 2 back: unchanged
    assert list(e["conn_kf"][0, :3]) == [2, 3, 1] and e["parent"][0] == 2              # pKFmax = kf 2, the first maximum in address order
    e = CC.expected_update(by["unchanged_send"])
    assert e["status"][1] == 0 and e["status"][2] == 0 and e["status"][0] == CR.UPDATED
    e = CC.expected_update(by["changed_send"])                # kf 1's list gains its sub-threshold entries (1-2: 1, 1-3: 2)
    assert e["status"][1] == CR.RESORTED and list(e["ord_kf"][1, :3]) == [0, 3, 2] and list(e["ord_w"][1, :3]) == [6, 2, 1]
    e = CC.expected_update(by["empty_member"])
    assert e["status"][1] == CR.EMPTY | CR.RESORTED and e["first"][1] == 1 and e["parent"][1] == -1 and e["nconn"][1] == 3
    assert e["parent"][0] == -1 and e["first"][0] == 1                                 # mnId == 0
    e = CC.expected_update(by["conn_cap_one_past"])
    assert e["status"][0] == CR.LIMIT and e["nconn"][0] == 0 and e["info"][2] == 1 and e["status"][1] & CR.UPDATED
    e = CC.expected_update(by["loop_cap_one_past"])
    assert e["info"][0] == CR.LIMIT and np.all(e["loop_conn"][:, 0] == -1) and e["info"][1] == e["loop_cap"] + 1


def test_views_reference_reads_upper_bound_as_written():
    kfs, _ = CC.objects(CC.view_world())
    k = kfs[0]
    assert k.ordered_w == sorted(k.ordered_w, reverse=True) and k.ordered_w.count(6) == 3
    assert len(k.GetCovisiblesByWeight(6)) == sum(x >= 6 for x in k.ordered_w)                 # the equal weights are inside the prefix
    assert len(k.GetCovisiblesByWeight(min(k.ordered_w))) == 0 and len(k.GetCovisiblesByWeight(10 ** 6)) == 0
    assert len(k.GetCovisiblesByWeight(6, CR.LOCAL_MUTANTS["by_weight_strict"])) != len(k.GetCovisiblesByWeight(6))
    assert len(k.GetBestCovisibilityKeyFrames(10)) == 10 and len(kfs[13].GetBestCovisibilityKeyFrames(10)) == 3


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
    c = next(c for c in cases if c.name == "sender_before_and_after")
    w, t = c.w, CC.table_arrays(c.w)

    def call(**kw):
        a = dict(slots=w.slots, npoints=len(w.obs), st=t["obs_start"], of=t["obs_frame"][:t["nobs"]], lst=c.lst, th=3, order=w.order, state={})
        a.update(kw)
        g = pg.CovisibilityGraph(_NoLibrary(), w.nkf, 4, a["order"])
        for k, v in a["state"].items():
            getattr(g, k)[...] = v
        return g.UpdateConnections(a["slots"], a["npoints"], a["st"], a["of"], a["lst"], None, a["th"], 0)
    bad_start = t["obs_start"].copy()
    bad_start[2] = bad_start[1] - 1
    for kw in (dict(th=0), dict(lst=[0, 0]), dict(lst=[4]), dict(slots=[[len(w.obs)]] + w.slots[1:]), dict(slots=w.slots[1:]), dict(st=bad_start),
               dict(of=np.full(t["nobs"], 9, np.int32)), dict(of=np.zeros(t["nobs"], np.int32)), dict(order=[0, 1, 1, 2]),
               dict(state=dict(nconn=5)), dict(state=dict(nconn=2, conn_kf=np.array([3, 1, 0, 0]))), dict(state=dict(nord=1, ord_kf=2)),
               dict(state=dict(parent=7))):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(AssertionError, match="the library was called"):
        call()
    for args in ((0,), (CR.MAX_CONN + 1,)):
        with pytest.raises(ValueError):
            pg.CovisibilityGraph(_NoLibrary(), 3, *args)
    with pytest.raises(ValueError):
        pg.CovisibilityGraph(_NoLibrary(), CR.MAX_KF + 1, 4)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    return pg.ORBextractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240)


@pytest.mark.gpu
def test_gpu_constructed_cases_equal_the_reference_in_both_forms(ext, cases):
    for c in cases:
        e = CC.expected_update(c)
        got = CC.download_update(CC.run_device_update(c, ext, e), e)
        assert CC.same_update(got, e, c.w.nkf), (c.name, "device", CC.diff_update(got, e, c.w.nkf))
        single = CC.run_single_update(c, ext, e)
        assert CC.same_update(single, e, c.w.nkf), (c.name, "single", CC.diff_update(single, e, c.w.nkf))
        assert all(np.asarray(single[k])[:c.w.nkf].tobytes() == np.asarray(got[k])[:c.w.nkf].tobytes() for k in CC.STATE_KEYS[:9]), c.name


@pytest.mark.gpu
def test_gpu_random_maps_equal_the_reference(ext, randoms):
    for c in randoms[:120]:
        e = CC.expected_update(c)
        got = CC.download_update(CC.run_device_update(c, ext, e), e)
        assert CC.same_update(got, e, c.w.nkf), (c.name, CC.diff_update(got, e, c.w.nkf))


@pytest.mark.gpu
def test_gpu_repeat_and_second_stream_give_the_same_bytes(ext, cases):
    import torch
    for c in [c for c in cases if c.name in ("ties_whole_map", "long_list", "sender_before_and_after")]:
        e = CC.expected_update(c)
        first = CC.download_update(CC.run_device_update(c, ext, e), e)
        again = CC.download_update(CC.run_device_update(c, ext, e), e)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            d = CC.run_device_update(c, ext, e, stream=st)
        st.synchronize()
        other = CC.download_update(d, e)
        for k in CC.STATE_KEYS:
            assert first[k].tobytes() == again[k].tobytes() == other[k].tobytes(), (c.name, k)


def _views(ext, d, nkf, conn_cap, nbest, ncovis_cap, w, stream=None):
    import torch
    full = lambda *shape: torch.full(shape, -9, dtype=torch.int32, device="cuda")
    v = dict(best=full(nkf + 1, nbest), covis_start=full(nkf + 2), covis=full(ncovis_cap + 1), covis_weight=full(ncovis_cap + 1), by_weight=full(nkf + 1),
             vinfo=full(2))
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = ext._L.pgorb_covisibility_views_device(ext._h, nkf, conn_cap, CC.ptr(d["ord_kf"]), CC.ptr(d["ord_w"]), CC.ptr(d["nord"]), nbest, CC.ptr(v["best"]),
                                                ncovis_cap, CC.ptr(v["covis_start"]), CC.ptr(v["covis"]), CC.ptr(v["covis_weight"]), w,
                                                CC.ptr(v["by_weight"]), CC.ptr(v["vinfo"]), C.c_void_p(s.cuda_stream))
    assert rc == 0, rc
    return v


@pytest.mark.gpu
def test_gpu_views_equal_the_reference_at_the_capacity_and_one_past(ext):
    import torch
    w = CC.view_world()
    kfs, _ = CC.objects(w)
    nkf, conn_cap = w.nkf, 13
    best, covis, by_weight = CR.covisibility_views(kfs, 10, 6)
    total = sum(len(r) for r in covis)
    assert max(len(r) for r in covis) > 10 and min(len(r) for r in covis) >= 1
    d = {k: CC.dev(v) for k, v in CC.state_arrays(w, conn_cap).items()}
    for cap in (total, total - 1):
        v = _views(ext, d, nkf, conn_cap, 10, cap, 6)
        torch.cuda.synchronize()
        h = {k: t.cpu().numpy() for k, t in v.items()}
        assert np.all(h["best"][nkf] == -9) and h["covis_start"][nkf + 1] == -9 and h["covis"][cap] == -9 and h["by_weight"][nkf] == -9
        for f in range(nkf):
            assert list(h["best"][f]) == [k.idx for k in best[f]] + [-1] * (10 - len(best[f])), f
            assert h["by_weight"][f] == by_weight[f], f
        if cap == total:
            assert list(h["vinfo"]) == [0, total]
            for f in range(nkf):
                a, b = h["covis_start"][f], h["covis_start"][f + 1]
                assert list(zip(h["covis"][a:b], h["covis_weight"][a:b])) == [(k.idx, x) for k, x in covis[f]], f
        else:
            assert list(h["vinfo"]) == [CR.LIMIT, total] and np.all(h["covis_start"][:nkf + 1] == 0) and np.all(h["covis"] == -9)


def _loop_world():
    """12 key frames of a ride, settled; then SearchAndFuse's effect: points of the loop side (0, 1) seen by the current side (10, 11)"""
    w = CC.World(12, order=[(5 * f + 4) % 12 for f in range(12)], id0=[f == 0 for f in range(12)])
    for f in range(11):
        w.share([f, f + 1], 6)
    for f in range(10):
        w.share([f, f + 2], 3 + f % 2)
    CC._settle(w, 4)
    w.share([0, 11], 5); w.share([1, 11], 4); w.share([0, 10], 4); w.share([1, 10], 2)
    return w


@pytest.mark.gpu
def test_gpu_chain_into_the_essential_graph_on_resident_arrays(ext):
    """update_connections -> views -> pgorb_optimize_essential_graph_device on one stream with nothing downloaded in between: the
    device-written CSR, parent and padded loop_conn give the bytes of the same call fed the reference's lists."""
    import torch
    import eg_cases as EC
    import pilotguru_amd as pg
    w = _loop_world()
    c = CC.GraphCase("loop", w, [11, 10, 9], th=4, loop_cap=16)
    e = CC.expected_update(c)
    nloop = int(e["info"][1])
    assert nloop >= 3 and e["conn_cap"] >= 4
    best, covis, _ = CR.covisibility_views(e["kfs"], 10, 0)
    ncovis = sum(len(r) for r in covis)
    g = EC.build(12, 5, min_feat=4)
    bytes_of = lambda a: torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).cuda()

    def essential_graph(parent, loop_conn, covis_start, cv, cw, stream):
        d_pts = bytes_of(g["points"])
        hold = [torch.from_numpy(g["kf_id"].astype(np.int64)).cuda(), bytes_of(g["pose"]), CC.dev(g["loop_edge_start"]), CC.dev(np.zeros(1, np.int32))[:0],
                CC.dev(g["point_ref_kf"]), bytes_of(g["kf_bad"]), bytes_of(g["point_bad"]), bytes_of(g["has_corrected"]), bytes_of(g["corrected"]),
                bytes_of(g["has_non_corrected"]), bytes_of(g["non_corrected"])]
        out = pg.Optimizer.OptimizeEssentialGraph_device(
            ext, hold[0], hold[1], g["loop_kf"], g["cur_kf"], parent, loop_conn, hold[2], hold[3], covis_start, cv, cw, len(g["points"]), d_pts, hold[4],
            d_kf_bad=hold[5], d_point_bad=hold[6], d_has_corrected=hold[7], d_corrected=hold[8], d_has_non_corrected=hold[9], d_non_corrected=hold[10],
            bFixScale=g["fix_scale"], min_feat=4, iterations=g["iterations"], stream=stream.cuda_stream)
        return out, d_pts, hold

    st = torch.cuda.current_stream()
    d = CC.run_device_update(c, ext, e, stream=st)
    v = _views(ext, d, 12, e["conn_cap"], 10, ncovis, 0, stream=st)
    chained = essential_graph(d["parent"], d["loop_conn"][:16].reshape(-1), v["covis_start"][:13], v["covis"][:ncovis], v["covis_weight"][:ncovis], st)
    torch.cuda.synchronize()
    start = np.zeros(13, np.int32)
    start[1:] = np.cumsum([len(r) for r in covis])
    fed = essential_graph(CC.dev(e["parent"]), CC.dev(e["loop_conn"][:nloop].reshape(-1)), CC.dev(start),
                          CC.dev(np.array([k.idx for r in covis for k, _ in r], np.int32)), CC.dev(np.array([x for r in covis for _, x in r], np.int32)), st)
    torch.cuda.synchronize()
    info = fed[0]["info"].cpu().numpy()
    assert info[0] == 0 and info[3] >= 1 and info[3:7].sum() > 12 and info[7] > 0, info
    for k in ("pose_out", "sim3_out", "info"):
        assert chained[0][k].cpu().numpy().tobytes() == fed[0][k].cpu().numpy().tobytes(), k
    assert chained[1].cpu().numpy().tobytes() == fed[1].cpu().numpy().tobytes()
    ne = int(info[3:7].sum())
    rec = pg.EG_EDGE_DTYPE.itemsize
    assert chained[0]["edge_out"].cpu().numpy().reshape(-1)[:ne * rec].tobytes() == fed[0]["edge_out"].cpu().numpy().reshape(-1)[:ne * rec].tobytes()


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
    std::vector<int32_t> status;
    auto update = [&](std::vector<std::vector<int32_t>> s, MapPointObservations o, std::vector<int32_t> list, int th, std::vector<int32_t> order, int nconn0) {
        CovisibilityGraph g(nullptr, 3, 4, order);
        g.nconn[0] = nconn0;
        g.UpdateConnections(s, 2, {}, o, list, th, status);
    };
    MapPointObservations twice = obs; twice.obsFrame = {0, 0, 1, 2};
    MapPointObservations range = obs; range.obsFrame = {0, 3, 1, 2};
    run("well_formed", [&] { update(slots, obs, {1, 0}, 15, {}, 0); });
    run("th", [&] { update(slots, obs, {1, 0}, 0, {}, 0); });
    run("list_twice", [&] { update(slots, obs, {1, 1}, 15, {}, 0); });
    run("list_range", [&] { update(slots, obs, {3}, 15, {}, 0); });
    run("slot_range", [&] { update({{2}, {0}, {1}}, obs, {0}, 15, {}, 0); });
    run("obs_twice", [&] { update(slots, twice, {0}, 15, {}, 0); });
    run("obs_range", [&] { update(slots, range, {0}, 15, {}, 0); });
    run("order", [&] { update(slots, obs, {0}, 15, {0, 0, 1}, 0); });
    run("row_count", [&] { update(slots, obs, {0}, 15, {}, 5); });
    run("row_entry", [&] { update(slots, obs, {0}, 15, {}, 1); });          // connKf[0][0] is -1
    run("conn_cap", [&] { CovisibilityGraph g(nullptr, 3, PGORB_COVIS_MAX_CONN + 1); });
    Tracking tr(nullptr);
    auto local = [&](std::vector<int32_t> frame, std::vector<int32_t>* prev, int lkfCap, int qcap, int parent0) {
        CovisibilityGraph g(nullptr, 3, 4);
        g.parent[0] = parent0;
        tr.UpdateLocalMap(g, frame, slots, 2, {}, obs, {}, prev, 10, 80, lkfCap, qcap);
    };
    std::vector<int32_t> prevBad = {3};
    run("local_well_formed", [&] { local({0, 1, -1}, nullptr, 8, 8, -1); });
    run("local_slot", [&] { local({2}, nullptr, 8, 8, -1); });
    run("local_prev", [&] { local({0}, &prevBad, 8, 8, -1); });
    run("local_lkf_cap", [&] { local({0}, nullptr, 0, 8, -1); });
    run("local_qcap", [&] { local({0}, nullptr, 8, 16001, -1); });
    run("local_parent", [&] { local({0}, nullptr, 8, 8, 3); });
    return 0;
}
"""


def test_cpp_mirror_rejects_bad_inputs_before_calling_the_library(tmp_path):
    """pgorb::CovisibilityGraph::UpdateConnections and pgorb::Tracking::UpdateLocalMap throw std::invalid_argument for what the single
    calls would refuse, before any pointer reaches the library; well-formed input reaches it (a NULL context here, so PGORB_E_ARG comes
    back as std::runtime_error)."""
    import subprocess
    src, exe = os.path.join(str(tmp_path), "covis_driver.cc"), os.path.join(str(tmp_path), "covis_driver")
    open(src, "w").write(CPP_DRIVER)
    lib = os.path.join(ROOT, "pilotguru_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", ROOT, src, "-o", exe, "-L", lib, "-lpgorb", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    got = dict(l.split() for l in subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines())
    assert got.pop("well_formed") == "runtime_error" and got.pop("local_well_formed") == "runtime_error", got
    assert len(got) == 15 and set(got.values()) == {"invalid_argument"}, got
