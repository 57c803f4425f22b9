"""Tracking::UpdateLocalMap on the GPU (pilotguru_amd/csrc/covisibility.hip, k_cov_local; include/pgorb.h) against the literal
reference (tests/covis_reference.py: UpdateLocalKeyFrames + UpdateLocalPoints, Tracking.cc:1196-1321) on constructed cases and
seeded random maps (tests/covis_cases.py), and chained into pgorb_search_local_points_batch_device.  Every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import covis_cases as CC  # noqa: E402
import covis_reference as CR  # noqa: E402

NRANDOM = 300


@pytest.fixture(scope="module")
def cases():
    return CC.local_cases()


@pytest.fixture(scope="module")
def randoms():
    return [CC.random_local(s) for s in range(NRANDOM)]


def test_hand_written_expectations(cases):
    by = {c.name: c for c in cases}
    e = CC.expected_local(by["tied_votes"])                    # kfs 2, 3, 4, 5 with 2 votes each; addresses: 3 < 4 < 5 < 2
    assert e["ref_kf"] == 3 and list(e["local_kf"][:4]) == [3, 4, 5, 2] and list(e["kp_point"]) == by["tied_votes"].frame
    # entry 3: its best neighbour that is not marked, no unmarked child (4 is in), no parent left (2 is in) ...
    e = CC.expected_local(by["bad_voted_and_cleared_slot"])
    assert e["ref_kf"] != 3 and 3 not in e["local_kf"][:3] and e["kp_point"][-2] == -1 and e["status"] == 0
    e = CC.expected_local(by["all_voted_bad"])
    assert e["ref_kf"] == -1 and len(e["local_kf"]) == 0 and len(e["queries"]) == 0 and e["status"] == 0
    e = CC.expected_local(by["no_votes"])
    assert e["status"] == CR.NO_VOTES and len(e["local_kf"]) == 0 and e["ref_kf"] == -1
    e = CC.expected_local(by["no_votes_previous_list"])
    assert e["status"] == CR.NO_VOTES and list(e["local_kf"]) == [4, 1, 6] and len(e["queries"]) > 0
    e = CC.expected_local(by["no_votes_only_bad_points"])
    assert e["status"] == CR.NO_VOTES and list(e["kp_point"]) == [-1, -1] and list(e["local_kf"]) == [2]
    e = CC.expected_local(by["eleventh_neighbour"])
    assert sorted(e["local_kf"]) == list(range(11)) and e["ref_kf"] == 0
    e = CC.expected_local(by["children_by_rank"])              # children of 0 by address: 2 (bad), 6, 3, 1
    assert list(e["local_kf"]) == [0, 1, 6]
    e = CC.expected_local(by["bad_parent_ends_the_walk"])      # entry 1 pushes its bad parent 0 and the walk ends: 5, the child of 3, stays out
    assert list(e["local_kf"]) == [1, 2, 3, 4, 0]
    for n1, extra in ((79, 2), (80, 1), (81, 0), (82, 0)):
        e = CC.expected_local(by["first_stage_%d" % n1])
        assert len(e["local_kf"]) == n1 + extra, n1
    assert CC.expected_local(by["lkf_cap_exact"])["status"] == 0
    for name in ("lkf_cap_one_past", "qcap_one_past"):
        e = CC.expected_local(by[name])
        assert e["status"] == CR.LM_LIMIT and len(e["local_kf"]) == 0 and len(e["queries"]) == 0 and e["ref_kf"] >= 0


def test_every_local_map_mutant_is_caught(cases, randoms):
    pool = list(cases) + randoms
    want = [CC.expected_local(c) for c in pool]
    caught = {}
    for name, rules in CR.LOCAL_MUTANTS.items():
        if name == "by_weight_strict":                        # (a view: tests/test_covisibility.py)
            continue
        caught[name] = [c.name for c, w in zip(pool, want) if not CC.same_local(w, CC.expected_local(c, rules))]
        assert caught[name], name
    for name, where in (("cap_ge", "first_stage_80"), ("parent_bad_test", "bad_parent_ends_the_walk"),
                        ("parent_break_inner", "bad_parent_ends_the_walk"), ("eleventh_neighbour", "eleventh_neighbour"),
                        ("children_index_order", "children_by_rank"), ("bad_after_max", "bad_voted_and_cleared_slot")):
        assert where in caught[name], (name, caught[name][:8])
    assert any(n.startswith("random") for n in caught["expand_appended"])


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
    c = next(c for c in cases if c.name == "tied_votes")
    w, t = c.w, CC.table_arrays(c.w)
    st = CC.state_arrays(w, 4)

    def call(**kw):
        a = dict(frame=c.frame, slots=w.slots, of=t["obs_frame"][:t["nobs"]], prev=None, lkf_cap=16, qcap=64, nord=st["nord"], parent=st["parent"])
        a.update(kw)
        g = pg.CovisibilityGraph(_NoLibrary(), w.nkf, 4, w.order)
        g.ord_kf[...], g.nord[...], g.parent[...] = st["ord_kf"], a["nord"], a["parent"]
        return pg.Tracking.UpdateLocalMap(g, a["frame"], a["slots"], len(w.obs), t["obs_start"], a["of"], prev_local_kf=a["prev"],
                                          lkf_cap=a["lkf_cap"], qcap=a["qcap"])
    for kw in (dict(frame=[len(w.obs)]), dict(frame=[-2]), dict(slots=w.slots[:-1]), dict(of=np.full(t["nobs"], 8, np.int32)), dict(prev=[8]),
               dict(prev=list(range(8)) * 3), dict(lkf_cap=0), dict(lkf_cap=CR.MAX_KF + 1), dict(qcap=16001), dict(nord=5), dict(parent=8)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(AssertionError, match="the library was called"):
        call()


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    return pg.ORBextractor(500, 1.2, 8, 20, 7, max_width=640, max_height=480)


def _single(ext, c, e):
    import pilotguru_amd as pg
    w, t = c.w, CC.table_arrays(c.w)
    conn_cap = max([len(o) for o in w.ordl] + [len(m) for m in w.conn] + [1])
    st = CC.state_arrays(w, conn_cap)
    g = pg.CovisibilityGraph(ext, w.nkf, conn_cap, w.order)
    g.ord_kf[...], g.nord[...], g.parent[...] = st["ord_kf"], st["nord"], st["parent"]
    g.ord_kf[g.ord_kf == CC.FILL] = -1
    return pg.Tracking.UpdateLocalMap(g, c.frame, w.slots, len(w.obs), t["obs_start"], t["obs_frame"][:t["nobs"]], w.point_bad, w.kf_bad, c.prev,
                                      c.nbest, c.max_local, e["lkf_cap"], e["qcap"])


def _device(ext, c, e, stream=None):
    d = CC.run_device_local([c], ext, c.w, stream=stream, lkf_cap=e["lkf_cap"], qcap=e["qcap"], nbest=c.nbest, max_local=c.max_local,
                            prev=c.prev is not None)
    return d


@pytest.mark.gpu
def test_gpu_constructed_cases_equal_the_reference_in_both_forms(ext, cases):
    for c in cases:
        e = CC.expected_local(c)
        (got,), h = CC.download_local(_device(ext, c, e), [c])
        assert CC.same_local(got, e), (c.name, "device", got, e)
        single = _single(ext, c, e)
        assert CC.same_local(single, e), (c.name, "single", single, e)


@pytest.mark.gpu
def test_gpu_random_maps_in_one_batch_equal_the_reference(ext, randoms):
    """every pair of a batch over one world, with different frames: the result does not depend on the batch position"""
    for s in range(0, 40):
        base = randoms[s]
        group = [CC.LocalCase("p%d" % k, base.w, randoms[(s + 7 * k) % NRANDOM].frame[:6], base.prev, base.nbest, base.max_local) for k in range(5)]
        group = [g for g in group if all(p < len(base.w.obs) for p in g.frame)]
        es = [CC.expected_local(g) for g in group]
        lkf_cap, qcap = max(e["lkf_cap"] for e in es), max(e["qcap"] for e in es)
        group.append(group[0])
        es.append(es[0])
        d = CC.run_device_local(group, ext, base.w, lkf_cap=lkf_cap, qcap=qcap, nbest=base.nbest, max_local=base.max_local, prev=base.prev is not None)
        got, _ = CC.download_local(d, group)
        for g, e, r in zip(group, es, got):
            assert CC.same_local(r, e), (base.name, g.name, r, e)


@pytest.mark.gpu
def test_gpu_repeat_and_second_stream_give_the_same_bytes(ext, cases):
    import torch
    for c in [c for c in cases if c.name in ("tied_votes", "first_stage_80", "children_by_rank")]:
        e = CC.expected_local(c)
        _, first = CC.download_local(_device(ext, c, e), [c])
        _, again = CC.download_local(_device(ext, c, e), [c])
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            d = _device(ext, c, e, stream=st)
        st.synchronize()
        _, other = CC.download_local(d, [c])
        for k in first:
            assert first[k].tobytes() == again[k].tobytes() == other[k].tobytes(), (c.name, k)


@pytest.mark.gpu
def test_gpu_chain_into_search_local_points_on_resident_arrays(ext):
    """update_local_map -> pgorb_search_local_points_batch_device on one stream with nothing downloaded in between: d_queries / d_nq
    and the cleared slots as written give the bytes of the same call fed the reference's lists."""
    import torch
    import tracking_cases as TC
    from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE
    t = TC.local_scene("chain", 23, TC.generic_pose(1), 120, 20, 3.0)
    t.points[int(t.slots[t.slots >= 0][0])]["bad"] = True             # one tracked point has gone bad: its slot is cleared
    npts, nkf = len(t.points), 6
    w = CC.World(nkf, order=[2, 5, 0, 3, 1, 4], id0=[f == 0 for f in range(nkf)])
    for j in range(npts):
        w.point([f for f in range(nkf) if j % nkf in (f, (f + 1) % nkf) or (j % 11 == 0 and f == 3)], bad=bool(t.points[j]["bad"]))
    CC._settle(w, 1)
    c = CC.LocalCase("chain", w, [int(s) for s in t.slots])
    e = CC.expected_local(c)
    e["qcap"] = max(e["qcap"], 8)
    assert len(e["queries"]) > 40 and (np.asarray(c.frame) != e["kp_point"]).any() and e["status"] == 0
    st = torch.cuda.current_stream()
    s = C.c_void_p(st.cuda_stream)
    d = _device(ext, c, e, stream=st)
    cap, nfr, n = d["cap"], nkf + 1, len(t.keys)
    kp = np.zeros((nfr, cap), KEYPOINT_DTYPE)                          # (the key frames' keypoints are not read: zeros)
    ds = np.full((nfr, cap, 32), 0xFF, np.uint8)
    kp[nkf, :n], ds[nkf, :n] = t.keys, t.desc
    pts, pd, bad, obs = TC.table_arrays(t.points)
    hold = dict(dk=CC.dev(kp.view(np.uint8).reshape(nfr, cap, 28)), dd=CC.dev(ds), gs=torch.empty((nfr, 64 * 48 + 1), dtype=torch.int32, device="cuda"),
                gi=torch.full((nfr, cap), -7, dtype=torch.int32, device="cuda"), pts=CC.dev(pts.view(np.uint8).reshape(len(pts), 32)), pd=CC.dev(pd),
                bad=CC.dev(bad), obs=CC.dev(obs), pose=CC.dev(np.array([t.pose], KF_POSE_DTYPE).view(np.uint8).reshape(1, -1)))
    p = CC.ptr
    L, h = ext._L, ext._h
    ext._check(L.pgorb_frame_grid_batch_device(h, p(hold["dk"]), p(d["n"]), nfr, cap, *TC.BOUNDS, p(hold["gs"]), p(hold["gi"]), s))
    qcap = e["qcap"]

    def search(slots, queries, nq):
        out = lambda dtype, *shape: torch.full(shape, 77, dtype=dtype, device="cuda")
        o = dict(in_view=out(torch.uint8, 1, qcap), kp_point_out=out(torch.int32, 1, cap), n_to_match=out(torch.int32, 1), assigned=out(torch.int32, 1, cap),
                 nmatches=out(torch.int32, 1))
        ext._check(L.pgorb_search_local_points_batch_device(
            h, p(hold["dk"]), p(hold["dd"]), p(d["n"]), cap, p(hold["gs"]), p(hold["gi"]), p(d["pair_frame"]), 1, *TC.BOUNDS, p(hold["pose"]), p(slots),
            len(pts), p(hold["pts"]), p(hold["pd"]), p(hold["bad"]), p(hold["obs"]), qcap, p(nq), p(queries), None, 0.5, 3.0, 0.8, p(o["in_view"]),
            None, None, None, None, p(o["kp_point_out"]), p(o["n_to_match"]), p(o["assigned"]), p(o["nmatches"]), s))
        return o
    chained = search(d["kp_out"], d["queries"], d["nq"])               # as written, no synchronisation in between
    torch.cuda.synchronize()
    nq = len(e["queries"])
    slots, q = np.full((1, cap), -1, np.int32), np.zeros((1, qcap), np.int32)
    slots[0, :n], q[0, :nq] = e["kp_point"], e["queries"]
    fed = search(CC.dev(slots), CC.dev(q), CC.dev(np.array([nq], np.int32)))
    torch.cuda.synchronize()
    a, b = ({k: v.cpu().numpy() for k, v in o.items()} for o in (chained, fed))
    assert int(b["nmatches"][0]) > 0 and int(b["n_to_match"][0]) > 0
    assert a["nmatches"].tobytes() == b["nmatches"].tobytes() and a["n_to_match"].tobytes() == b["n_to_match"].tobytes()
    assert a["assigned"][0, :n].tobytes() == b["assigned"][0, :n].tobytes() and a["kp_point_out"][0, :n].tobytes() == b["kp_point_out"][0, :n].tobytes()
    assert a["in_view"][0, :nq].tobytes() == b["in_view"][0, :nq].tobytes()
