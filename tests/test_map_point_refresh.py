"""The map-point refresh on the GPU (pilotguru_amd/csrc/map_point.hip, k_mp_bin / k_mp_seg / k_mp_big; include/pgorb.h:
MapPoint::ComputeDistinctiveDescriptors + MapPoint::UpdateNormalAndDepth of many points in one call) against the plain sequential
reference (tests/map_point_reference.py) on constructed cases and random scenes (tests/map_point_cases.py).  Every comparison is
exact: integer decisions, and floats as bit patterns."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_cases as FC  # noqa: E402
import fuse_reference as FR  # noqa: E402
import map_point_cases as PC  # noqa: E402
import map_point_reference as MPR  # noqa: E402
import mapping_cases as MC  # noqa: E402
from matcher_cases import SF  # noqa: E402
from pilotguru_amd.orb import KF_POSE_DTYPE, MAP_POINT_DTYPE  # noqa: E402

EDGES = ["empty", "bad_point", "n1", "n2", "n3", "n4", "equal_medians", "best_last", "identical", "dist_256", "one_bad_kf", "all_kf_bad",
         "ref_not_first", "octave_top", "octave_0", "n63", "n64", "n65", "n%d" % MPR.MAX_OBS, "n_over", "selection_skips", "what_1",
         "what_2", "what_3", "shared_kfs"]


@pytest.fixture(scope="module")
def cases():
    return PC.edge_cases()


def test_refresh_symbols_and_null_context():
    from pilotguru_amd import _lib
    L = _lib.lib()
    for name in ("pgorb_refresh_map_points", "pgorb_refresh_map_points_batch_device"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.pgorb_refresh_map_points(None, 0, *([None] * 5), 0, *([None] * 7), 0, None, 3, None, None) == -1
    assert L.pgorb_refresh_map_points_batch_device(None, None, None, None, 0, 1, None, None, 0, *([None] * 6), 0, None, 0, None, 3,
                                                   None, None, None) == -1


def test_cases_reach_every_edge(cases):
    hits = collections.Counter()
    for c in cases:
        PC.run_reference(c, hits=hits)
    missing = [e for e in EDGES if not hits[e]]
    assert not missing, (missing, dict(hits))


def test_every_rule_mutant_is_caught(cases):
    small = [c for c in cases if max(len(p["obs"]) for p in c.points) <= 70]
    want = [PC.run_reference(c) for c in small]
    for name, rules in MPR.MUTANTS.items():
        assert any(not PC.same(w, PC.run_reference(c, rules)) for w, c in zip(want, small)), name


def test_limit_leaves_the_point_untouched(cases):
    c = next(c for c in cases if c.name == "n_max_plus_1")
    pts, desc, best, status = PC.run_reference(c)
    t = PC.table_arrays(c.points)
    assert status[0] == MPR.LIMIT and best[0] == -1 and pts.tobytes() == t[0].tobytes() and desc.tobytes() == t[1].tobytes()
    c = next(c for c in cases if c.name == "n_max_plus_1_bad_point")
    assert PC.run_reference(c)[3][0] == 0                                       # a bad point is a no-op before it is a limit


def test_random_scene_has_the_stated_distribution():
    c = PC.random_scene(3, nkf=260, nkeys=40, npts=4000)
    n = np.array([len(p["obs"]) for p in c.points])
    assert 0.55 < np.mean(n <= 4) < 0.65 and n.max() >= 200 and np.mean(n > 40) > 0.03 and len(c.kfs) >= 20


def test_descriptor_choice_equals_the_fuse_reference(cases):
    """Two independent restatements of ComputeDistinctiveDescriptors agree: tests/fuse_reference.py's (observations in key-frame id
    order) on key frames whose ids rise in list order."""
    checked = 0
    for c in cases + [PC.random_scene(1, nkf=30, nkeys=60, npts=300)]:
        if max(len(p["obs"]) for p in c.points) > 70:
            continue
        want = PC.run_reference(c, what=MPR.DESCRIPTOR)[1]
        kfs = [FC.make_kf(100 + f, k, d, P, FC.BOUNDS) for f, (k, d, P, _) in enumerate(c.kfs)]
        for kf, (_, _, _, bad) in zip(kfs, c.kfs):
            kf.bad = bad
        for i in c.selection():
            p = c.points[i]
            mp = FR.MapPoint(i, p["pos"], p["normal"], p["min_d"], p["max_d"], p["desc"])
            for f, idx in p["obs"]:
                mp.add_observation(kfs[f], idx)
            mp.bad = p["bad"]
            mp.compute_distinctive_descriptors()
            assert mp.desc.tobytes() == want[i].tobytes(), (c.name, i)
            checked += 1
    assert checked > 300


def _cnm_as_refresh(KF1, neigh, points):
    """The points of a CreateNewMapPoints result as a refresh case: lists (KF1, neighbour), the reference key frame KF1."""
    kfs = [(K["k"], K["d"], K["pose"], False) for K in [KF1] + list(neigh)]
    rng = np.random.RandomState(0)
    pts = []
    for s, i1, i2, pos, _, _, _ in points:
        pts.append(PC.make_point(rng, [(0, i1), (1 + s, i2)], ref=0, pos=pos))
    return PC.Case("cnm", kfs, pts)


def test_two_observations_equal_the_mapping_reference():
    """For (KF1, neighbour) with KF1 the reference key frame, UpdateNormalAndDepth here equals, bit for bit, what
    tests/mapping_reference.py's triangulate() stores for the same point."""
    KF1, neigh = MC.scene(2, nneigh=3, npts=120)
    points = MC.run_reference(KF1, neigh)[0]
    assert len(points) > 20
    got = PC.run_reference(_cnm_as_refresh(KF1, neigh, points), what=MPR.NORMAL_DEPTH)[0]
    for g, (_, _, _, pos, normal, mn, mx) in zip(got, points):
        assert g["normal"].tobytes() == np.asarray(normal, np.float32).tobytes()
        assert f32b(g["min_distance"]) == f32b(mn) and f32b(g["max_distance"]) == f32b(mx)


def f32b(x):
    return np.float32(x).tobytes()


def _malformed(c):
    """name -> keyword changes of _call() that pgorb_refresh_map_points refuses"""
    pts, desc, bad, st, of, oi, ref = PC.table_arrays(c.points)
    two = next(i for i in range(len(c.points)) if len(c.points[i]["obs"]) >= 2 and not c.points[i]["bad"])
    twice = of.copy(); twice[st[two] + 1] = twice[st[two]]
    far = of.copy(); far[0] = len(c.kfs)
    neg = oi.copy(); neg[0] = -1
    big = oi.copy(); big[0] = len(c.kfs[of[0]][0])
    down = st.copy(); down[3] = down[2] - 1
    rbad = ref.copy(); rbad[two] = len(c.points[two]["obs"])
    return dict(frame_out_of_range=dict(of=far), keypoint_negative=dict(oi=neg), keypoint_out_of_range=dict(oi=big), obs_start_decreases=dict(st=down),
                obs_start_not_from_0=dict(st=st + 1), key_frame_twice=dict(of=twice), ref_obs_outside=dict(ref=rbad),
                select_out_of_range=dict(select=[0, len(pts)]), select_negative=dict(select=[-1]), select_repeated=dict(select=[1, 2, 1]),
                what_0=dict(what=0), what_4=dict(what=4), descriptor_rows=dict(desc=desc[:-1]))


def test_python_mirror_rejects_bad_inputs(cases):
    import pilotguru_amd as pg
    c = next(c for c in cases if c.name == "shared_key_frames")
    K = [MC.KeyFrameArrays(None, k, d) for k, d, _, _ in c.kfs]
    base = dict(zip(("pts", "desc", "bad", "st", "of", "oi", "ref"), PC.table_arrays(c.points)), select=None, what=3)

    class Reached(Exception):
        pass

    class NoLibrary:                                                      # the checks come before the library is called
        def __getattr__(self, name):
            raise Reached(name)

    def call(**kw):
        a = dict(base, **kw)
        return pg.LocalMapping.RefreshMapPoints(K, [P for _, _, P, _ in c.kfs], a["pts"], a["desc"], a["st"], a["of"], a["oi"], a["ref"],
                                                a["bad"], [b for _, _, _, b in c.kfs], a["select"], a["what"], ext=NoLibrary())
    with pytest.raises(Reached):
        call()
    for name, kw in _malformed(c).items():
        with pytest.raises(ValueError):
            call(**kw)
            pytest.fail("input %s was accepted" % name)


# ---------------------------------------------------------------- the C++ mirror (pilotguru_amd/host/orb_extractor.hpp)
CPP_DRIVER = r"""
// reads cases written by tests/test_map_point_refresh.py and prints what pgorb::LocalMapping::RefreshMapPoints returns: the count,
// the status and best_obs lists, the points and the descriptors as hex, one line each, or the exception
#include <cstdio>
#include <cstring>
#include <fstream>
#include "pilotguru_amd/host/orb_extractor.hpp"
using namespace pgorb;
template <class T> static void rd(std::ifstream& f, std::vector<T>& v) { int32_t n; f.read((char*)&n, 4); v.resize(n); if (n) f.read((char*)v.data(), (size_t)n * sizeof(T)); }
static void line(const std::vector<int32_t>& v) { for (size_t i = 0; i < v.size(); i++) std::printf(i ? " %d" : "%d", v[i]); std::printf("\n"); }
static void hex(const void* p, size_t n) { for (size_t i = 0; i < n; i++) std::printf("%02x", ((const uint8_t*)p)[i]); std::printf("\n"); }
int main(int argc, char** argv)
{
    const bool run = argc > 1 && std::strcmp(argv[1], "run") == 0;        // "check": no context, the wrapper's checks only
    ORBextractor* ext = run ? new ORBextractor(1000, 1.2f, 8, 20, 7, 640, 480) : nullptr;
    LocalMapping lm(ext ? ext->context() : nullptr);
    for (int a = 2; a < argc; a++) {
        std::ifstream f(argv[a], std::ios::binary);
        int32_t nkf, what, hasSelect;
        f.read((char*)&nkf, 4);
        std::vector<KeyFrame> kfs(nkf);
        std::vector<const KeyFrame*> kp;
        for (auto& K : kfs) { rd(f, K.frame.mvKeysUndistorted); rd(f, K.frame.mDescriptors); f.read((char*)&K.pose, sizeof K.pose); kp.push_back(&K); }
        std::vector<uint8_t> kfBad, desc, bad;
        std::vector<pgorb_map_point> pts;
        MapPointObservations O;
        std::vector<int32_t> select, status, best;
        rd(f, kfBad); rd(f, pts); rd(f, desc); rd(f, bad); rd(f, O.obsStart); rd(f, O.obsFrame); rd(f, O.obsIdx); rd(f, O.refObs);
        f.read((char*)&hasSelect, 4); rd(f, select); f.read((char*)&what, 4);
        try {
            std::printf("%d\n", lm.RefreshMapPoints(kp, kfBad, pts, desc, bad, O, hasSelect ? &select : nullptr, what, status, &best));
            line(status); line(best); hex(pts.data(), pts.size() * sizeof(pgorb_map_point)); hex(desc.data(), desc.size());
        } catch (const std::invalid_argument&) { std::printf("invalid_argument\n");
        } catch (const std::runtime_error&) { std::printf("runtime_error\n"); }
    }
    delete ext;
    return 0;
}
"""


def _cpp_driver(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = os.path.join(str(tmp_path), "refresh_driver.cc"), os.path.join(str(tmp_path), "refresh_driver")
    open(src, "w").write(CPP_DRIVER)
    lib = os.path.join(root, "pilotguru_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", root, src, "-o", exe, "-L", lib, "-lpgorb", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _write_case(path, c, **kw):
    a = dict(zip(("pts", "desc", "bad", "st", "of", "oi", "ref"), PC.table_arrays(c.points)), select=c.select, what=c.what)
    a.update(kw)

    def arr(x, dt):
        x = np.ascontiguousarray(x, dt).reshape(-1)
        return np.int32(len(x)).tobytes() + x.tobytes()
    with open(path, "wb") as f:
        f.write(np.int32(len(c.kfs)).tobytes())
        for k, d, P, _ in c.kfs:
            f.write(arr(k, k.dtype) + arr(d, np.uint8) + np.asarray(P, KF_POSE_DTYPE).tobytes())
        f.write(arr([b for _, _, _, b in c.kfs], np.uint8) + arr(a["pts"], MAP_POINT_DTYPE) + arr(a["desc"], np.uint8) + arr(a["bad"], np.uint8) +
                arr(a["st"], np.int32) + arr(a["of"], np.int32) + arr(a["oi"], np.int32) + arr(a["ref"], np.int32) +
                np.int32(a["select"] is not None).tobytes() + arr([] if a["select"] is None else a["select"], np.int32) + np.int32(a["what"]).tobytes())


def _run_driver(exe, mode, paths):
    return subprocess.run([exe, mode] + paths, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines()


def test_cpp_mirror_rejects_bad_inputs_before_calling_the_library(tmp_path, cases):
    """pgorb::LocalMapping::RefreshMapPoints throws std::invalid_argument for every input pgorb_refresh_map_points would refuse,
    before any pointer reaches the library; well-formed input reaches it (a NULL context here, so PGORB_E_ARG comes back as
    std::runtime_error)."""
    exe = _cpp_driver(tmp_path)
    c = next(c for c in cases if c.name == "shared_key_frames")
    variants = [dict()] + list(_malformed(c).values())
    paths = []
    for n, kw in enumerate(variants):
        paths.append(os.path.join(str(tmp_path), "case%d.bin" % n))
        _write_case(paths[-1], c, **kw)
    got = _run_driver(exe, "check", paths)
    assert got == ["runtime_error"] + ["invalid_argument"] * (len(variants) - 1), list(zip(["ok"] + list(_malformed(c)), got))


# ---------------------------------------------------------------- GPU
def _extractor(w=640, h=480):
    import pilotguru_amd as pg
    return pg.ORBextractor(2000, MC.SCALE, NLEVELS, 20, 7, max_width=w, max_height=h)


NLEVELS = MC.NLEVELS


@pytest.mark.gpu
def test_gpu_single_call_equals_reference(cases):
    ext = _extractor()
    for c in cases:
        want, got = PC.run_reference(c), PC.run_gpu(c, ext)
        assert PC.same(want, got), (c.name, want[2:], got[2:])
    assert ext.GetScaleFactors()[:NLEVELS].tobytes() == np.asarray(SF[:NLEVELS], np.float32).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("what", [MPR.BOTH, MPR.DESCRIPTOR, MPR.NORMAL_DEPTH])
def test_gpu_batched_form_equals_reference(cases, what):
    ext = _extractor()
    out, untouched = PC.run_gpu_batched(cases, ext, what)
    for c, got in zip(cases, out):
        assert PC.same(PC.run_reference(c, what=what), got), c.name
    assert untouched, "wrote past nsel or outside the selected points"


@pytest.mark.gpu
def test_gpu_batched_form_refuses_bad_indices_per_point(cases):
    """The unchecked form turns an index out of range into a no-op with a negative status for THAT point."""
    c = next(c for c in cases if c.name == "shared_key_frames")
    broken = PC.Case("broken", c.kfs, [dict(p) for p in c.points])
    broken.points[4] = dict(broken.points[4], obs=[(10 ** 6, 0)] + broken.points[4]["obs"][1:])        # a frame outside the batch
    broken.points[11] = dict(broken.points[11], obs=[(broken.points[11]["obs"][0][0], 10 ** 6)] + broken.points[11]["obs"][1:])
    broken.points[20] = dict(broken.points[20], ref=99)
    ext = _extractor()
    (got,), untouched = PC.run_gpu_batched([broken], ext, MPR.BOTH)
    want = PC.run_reference(c)
    t = PC.table_arrays(c.points)
    for i in range(len(c.points)):
        if i in (4, 11, 20):
            assert got[3][i] == -1 and got[2][i] == -1 and got[0][i].tobytes() == t[0][i].tobytes() and got[1][i].tobytes() == t[1][i].tobytes()
        else:
            assert all(g[i].tobytes() == w[i].tobytes() for g, w in zip(got, want)), i
    assert untouched


@pytest.mark.gpu
def test_gpu_random_scene_1080p_equals_reference():
    """22 key frames x 2000 keypoints, 5000 points of the skewed length distribution: every point, no tolerance."""
    ext = _extractor(1920, 1080)
    c = PC.random_scene(7)
    want, got = PC.run_reference(c), PC.run_gpu(c, ext)
    assert len(c.points) >= 5000 and len(c.kfs) == 22 and len(c.kfs[0][0]) == 2000
    assert np.array_equal(want[3], got[3]) and np.array_equal(want[2], got[2])
    assert PC.same(want, got)
    assert (want[3] == 3).sum() > 4000


@pytest.mark.gpu
def test_gpu_random_scene_with_a_long_tail_equals_reference():
    """260 small key frames, so that the lists reach 200-260 observations (k_mp_big) beside the short ones, in one batched call."""
    ext = _extractor()
    c = PC.random_scene(11, nkf=260, nkeys=120, npts=2500)
    assert max(len(p["obs"]) for p in c.points) >= 200
    (got,), untouched = PC.run_gpu_batched([c], ext, MPR.BOTH)
    assert PC.same(PC.run_reference(c), got) and untouched


def _refresh_objects(kfs, points):
    """fuse_reference objects -> a refresh case over `points` (live ones listed in key-frame id order, as fuse_reference iterates
    them; mpRefKF, which fuse_reference does not track, is taken to be the observer with the lowest id)."""
    where = {kf.id: f for f, kf in enumerate(kfs)}
    frames = [(kf.keys, kf.desc, kf.pose, kf.bad) for kf in kfs]
    pts = []
    for mp in points:
        obs = [(where[kf.id], int(mp.obs[kf])) for kf in sorted(mp.obs)]
        pts.append(dict(pos=mp.pos, desc=mp.desc, normal=mp.normal, min_d=mp.min_d, max_d=mp.max_d, bad=mp.bad, obs=obs, ref=0))
    return PC.Case("search_in_neighbors", frames, pts)


@pytest.mark.gpu
def test_gpu_tail_of_search_in_neighbors_equals_reference():
    """SearchInNeighbors to its end: the two Fuse rounds on the GPU, then the update of every live point of the current key frame
    (LocalMapping.cc:519-532) in one refresh call, against fuse_reference's rounds followed by the reference's loop."""
    ext = _extractor()

    def finish(cur, targets, refresh):
        live = [mp for mp in cur.slots if mp is not None and not mp.bad]
        live = list({mp.id: mp for mp in live}.values())
        out = refresh(_refresh_objects([cur] + targets, live))
        for mp, p, d in zip(live, out[0], out[1]):
            mp.desc, mp.normal, mp.min_d, mp.max_d = d.copy(), p["normal"].copy(), p["min_distance"], p["max_distance"]
        return len(live), out

    cur, targets, points = FC.neighbourhood(5, 640, 480, 20, 1000, 500.0)
    want_n = FR.search_in_neighbors(cur, targets)
    nlive, want_out = finish(cur, targets, PC.run_reference)
    want = FC.map_state([cur] + targets, points), [(f32b(p.min_d), f32b(p.max_d), p.normal.tobytes()) for p in points]
    cur, targets, points = FC.neighbourhood(5, 640, 480, 20, 1000, 500.0)
    got_n = FC.search_in_neighbors_gpu(ext, cur, targets, points)
    _, got_out = finish(cur, targets, lambda c: PC.run_gpu(c, ext))
    got = FC.map_state([cur] + targets, points), [(f32b(p.min_d), f32b(p.max_d), p.normal.tobytes()) for p in points]
    assert got_n == want_n and nlive > 300
    assert PC.same(want_out, got_out)
    assert got == want
    assert (want_out[3] == 3).all() and len(set(want_out[2])) > 1


@pytest.mark.gpu
def test_gpu_refresh_reproduces_create_new_map_points():
    """Every point pgorb_create_new_map_points returns, refreshed with the list (KF1, neighbour) and ref_obs = 0, reproduces that
    call's normal, min_distance and max_distance bit for bit (k_cnm_triangulate's two-observation form)."""
    ext = _extractor()
    total = 0
    for seed in (1, 2):
        KF1, neigh = MC.scene(seed)
        points = MC.run_gpu(KF1, neigh, ext)[0]
        got = PC.run_gpu(_cnm_as_refresh(KF1, neigh, points), ext)
        assert (got[3] == 3).all()
        for g, (_, _, _, pos, normal, mn, mx) in zip(got[0], points):
            assert g["pos"].tobytes() == pos.tobytes() and g["normal"].tobytes() == normal.tobytes()
            assert f32b(g["min_distance"]) == f32b(mn) and f32b(g["max_distance"]) == f32b(mx)
        total += len(points)
    assert total > 100


@pytest.mark.gpu
def test_gpu_cpp_mirror_equals_reference(tmp_path, cases):
    exe = _cpp_driver(tmp_path)
    chosen = [c for c in cases if len(c.kfs) <= 70]
    paths = []
    for n, c in enumerate(chosen):
        paths.append(os.path.join(str(tmp_path), "case%d.bin" % n))
        _write_case(paths[-1], c)
    got = _run_driver(exe, "run", paths)
    want = []
    for c in chosen:
        pts, desc, best, status = PC.run_reference(c)
        want += ["%d" % int((status > 0).sum())] + [" ".join("%d" % x for x in v) for v in (status, best)] + [pts.tobytes().hex(), desc.tobytes().hex()]
    assert got == want
