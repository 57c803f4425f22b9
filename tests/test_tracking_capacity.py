"""The tracking thread's matchers with the projection on the device at their stated capacity and one past it (the pattern of
tests/test_capacity.py): the deciding kernel's LDS line  keypoints * 13 + queries * 10 + 256 <= 163840  at its two ends, and for
pgorb_search_local_points the 1 048 576 table points its seen marks allow.  Small synthetic contents under the identity pose: a
handful of live points, among them the last keypoint, the last query and the last table point, everything else behind the camera
or NULL.  On the CPU the shapes are shown to lie on the limits; on the GPU the single call and the batched form give the
reference's result at capacity and PGORB_E_LIMIT one past it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracking_cases as TC  # noqa: E402
from matcher_cases import keys, rand_desc  # noqa: E402

LDS = 163840
SHAPES = [(12582, 1), (7112, 7112)]              # (keypoints, queries) on the LDS line
TABLE_MAX = 1 << 20
KINDS = ["local", "last", "kf"]
_CACHE = {}


def lds(cap, q):
    return cap * 13 + q * 10 + 256


def test_shapes_lie_on_the_limits():
    for cap, q in SHAPES:
        assert lds(cap, q) <= LDS < lds(cap, q + 1) and cap <= 16000 and q <= 16000
    assert lds(7112, 7112) <= LDS < lds(7113, 7113)          # the batched frame-to-frame forms: a pair's queries are a frame
    assert (TABLE_MAX + 31) // 32 * 4 == 128 * 1024           # the seen marks of one pair at the table limit


def capacity_case(kind, cap, nq):
    """cap keypoints and nq queries; the live points are the first, (when there are several) the second and the last query, their
    keypoints the last ones of the frame."""
    key = (kind, cap, nq)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.RandomState(cap + nq)
    live = sorted({0, min(1, nq - 1), nq - 1})
    P = [TC.pt((0, 0, -4.0)) for _ in range(nq)]
    for j, q in enumerate(live):
        P[q] = TC.pt((1.0 + j, 0.5 * j, 4.0), min_d=2, max_d=8, has_obs=j != 1)
    TC._finish_points(P, rng)
    kl, dl, _ = TC.keypoints_for(rng, TC.EDGE_POSE, P, live, 0)
    nf = cap - len(kl)
    kf_ = keys(rng.uniform(-300, 300, nf), rng.uniform(100, 230, nf), octave=rng.randint(0, 8, nf).astype(np.int32))   # away from the live ones
    k, d = np.concatenate([kf_, kl]), np.concatenate([rand_desc(rng, nf), dl])
    if kind == "local":
        slots = np.full(cap, -1, np.int32)
        c = TC.Case(kind, "cap_%s_%d_%d" % key, k, d, TC.EDGE_POSE, P, 3.0, slots=slots, queries=np.arange(nq))
    else:
        octs = np.zeros(nq, np.int32)
        for q in live:
            octs[q] = TC._front(TC.EDGE_POSE, P[q])[3]
        ok = keys(np.zeros(nq), np.zeros(nq), octave=octs, angle=rng.uniform(0, 360, nq).astype(np.float32))
        c = TC.Case(kind, "cap_%s_%d_%d" % key, k, d, TC.EDGE_POSE, P, 6.0, other_keys=ok, other_point=np.arange(nq), ori=False)
    w = TC.run_reference(c)
    _CACHE[key] = (c, w)
    return c, w


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cap,nq", SHAPES)
def test_cases_use_the_last_keypoint_and_the_last_query(kind, cap, nq):
    c, w = capacity_case(kind, cap, nq)
    assert len(c.keys) == cap and (len(c.queries) if kind == "local" else len(c.other_keys)) == nq
    a = w["assigned"]
    assert a.max() == nq - 1 and a[cap - 3:].max() >= 0 and w["nmatches"] == len({0, min(1, nq - 1), nq - 1})
    assert np.flatnonzero(a >= 0).max() >= cap - 3


def big_table_case():
    """1 048 576 table points, almost all of them zeros nobody names: the last one sits in a slot (its seen mark is the last bit) and is
    queried too, the one before it is in view.  The reference runs on the named points alone."""
    if "table" in _CACHE:
        return _CACHE["table"]
    rng = np.random.RandomState(3)
    named = [0, 5, TABLE_MAX - 2, TABLE_MAX - 1]
    small = TC._finish_points([TC.pt((1.0 + j, 0.5 * j, 4.0), min_d=2, max_d=8) for j in range(4)], rng)
    k, d, owner = TC.keypoints_for(rng, TC.EDGE_POSE, small, range(4), 8)
    slots = np.full(len(k), -1, np.int32)
    slots[np.flatnonzero(owner == 3)[0]] = 3
    cs = TC.Case("local", "cap_table", k, d, TC.EDGE_POSE, small, 3.0, slots=slots, queries=[3, 2, 0, 1])
    w = TC.run_reference(cs)
    pts, pd, bad, obs = TC.table_arrays(small)
    big = (np.zeros(TABLE_MAX, pts.dtype), np.zeros((TABLE_MAX, 32), np.uint8), np.zeros(TABLE_MAX, np.uint8), np.ones(TABLE_MAX, np.uint8))
    for a, b in zip(big, (pts, pd, bad, obs)):
        a[named] = b
    remap = np.array(named + [-1], np.int32)                  # (index -1 stays -1)
    _CACHE["table"] = (cs, w, big, remap)
    return _CACHE["table"]


def test_big_table_case_marks_the_last_point_seen():
    cs, w, big, remap = big_table_case()
    assert remap[w["kp_point_out"]].max() == TABLE_MAX - 1 and list(w["in_view"]) == [0, 1, 1, 1] and w["nmatches"] == 3


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    e = pg.ORBextractor(1000, 1.2, TC.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=4)
    yield e
    e.close()


def _one_past(c, kind):
    """The same case with one more query: nothing of it is read, the gate answers first."""
    if kind == "local":
        P = c.points + [TC.pt((0, 0, -4.0), desc=np.zeros(32, np.uint8))]
        return TC.Case(kind, c.name + "+1", c.keys, c.desc, c.pose, P, c.th, slots=c.slots, queries=np.arange(len(P)))
    ok = np.concatenate([c.other_keys, c.other_keys[-1:]])
    return TC.Case(kind, c.name + "+1", c.keys, c.desc, c.pose, c.points, c.th, other_keys=ok,
                   other_point=np.concatenate([c.other_point, [-1]]), ori=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cap,nq", SHAPES)
def test_gpu_at_the_lds_line_and_one_past_it(ext, kind, cap, nq):
    from pilotguru_amd._lib import PGORB_E_LIMIT, PgorbError
    c, w = capacity_case(kind, cap, nq)
    assert not TC.differences(kind, w, TC.run_gpu(c, ext)), "single call at capacity"
    over = _one_past(c, kind)
    with pytest.raises(PgorbError) as e:
        TC.run_gpu(over, ext)
    assert e.value.code == PGORB_E_LIMIT
    if kind == "local" or cap == nq:              # batched frame-to-frame: the queries are a frame of the batch, so cap == qcap
        assert not TC.differences(kind, w, TC.run_gpu_batch(TC.as_batch(c), ext)[0]), "batched form at capacity"
        with pytest.raises(PgorbError) as e:
            TC.run_gpu_batch(TC.as_batch(over), ext)
        assert e.value.code == PGORB_E_LIMIT


@pytest.mark.gpu
def test_gpu_local_points_at_the_table_limit_and_one_past_it(ext):
    import pilotguru_amd as pg
    import torch
    from pilotguru_amd._lib import PGORB_E_LIMIT, PgorbError
    cs, w, big, remap = big_table_case()
    inv = {int(v): i for i, v in enumerate(remap[:-1])}
    F = TC.ArrayFrame(ext, cs.keys, cs.desc, TC.BOUNDS)
    m = pg.ORBmatcher(cs.nnratio, True)

    def call(npoints_extra):
        pts, pd, bad, obs = (np.concatenate([a, a[:npoints_extra]]) for a in big)
        T = pg.MapPointTable(pts, pd, bad, np.zeros(len(pts) + 1, np.int32), np.zeros(0, np.uint64))
        return m.SearchLocalPoints(F, cs.pose, remap[cs.slots], T, remap[cs.queries], None, cs.th, 0.5, point_has_obs=obs)
    got = call(0)
    got["kp_point_out"] = np.array([inv.get(int(v), -1) for v in got["kp_point_out"]], np.int32)
    assert not TC.differences("local", w, got), "single call at the table limit"
    with pytest.raises(PgorbError) as e:
        call(1)
    assert e.value.code == PGORB_E_LIMIT
    # the batched form: the table on the device, one pair
    L, h = ext._L, ext._h
    p = lambda t: C.c_void_p(t.data_ptr())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n, nq = len(cs.keys), len(cs.queries)
    dk, dd, dn = dev(cs.keys.view(np.uint8).reshape(n, 28)), dev(cs.desc), dev(np.array([n], np.int32))
    gs, gi = torch.empty(64 * 48 + 1, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ext._check(L.pgorb_frame_grid_batch_device(h, p(dk), p(dn), 1, n, *TC.BOUNDS, p(gs), p(gi), s))
    tab = [dev(np.concatenate([a, a[:1]]).view(np.uint8)) for a in big]
    pose = dev(np.ascontiguousarray(cs.pose, TC.KF_POSE_DTYPE).reshape(1).view(np.uint8))
    sl, q, dnq = dev(remap[cs.slots]), dev(remap[cs.queries]), dev(np.array([nq], np.int32))
    iv = torch.zeros(nq, dtype=torch.uint8, device="cuda")
    kpo, asg = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    ntm, nm = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")

    def batched(npoints):
        return L.pgorb_search_local_points_batch_device(h, p(dk), p(dd), p(dn), n, p(gs), p(gi), None, 1, *TC.BOUNDS, p(pose), p(sl), npoints,
                                                        p(tab[0]), p(tab[1]), p(tab[2]), p(tab[3]), nq, p(dnq), p(q), None, 0.5, cs.th, cs.nnratio,
                                                        p(iv), None, None, None, None, p(kpo), p(ntm), p(asg), p(nm), s)
    ext._check(batched(TABLE_MAX))
    torch.cuda.synchronize()
    assert int(nm[0]) == w["nmatches"] and int(ntm[0]) == w["n_to_match"]
    assert np.array_equal(asg.cpu().numpy(), w["assigned"]) and np.array_equal(iv.cpu().numpy(), w["in_view"])
    assert np.array_equal(np.array([inv.get(int(v), -1) for v in kpo.cpu().numpy()], np.int32), w["kp_point_out"])
    assert batched(TABLE_MAX + 1) == PGORB_E_LIMIT
