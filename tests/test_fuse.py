"""ORBmatcher::Fuse on the GPU (pilotguru_amd/csrc/fuse.hip, k_fuse_match / k_fuse_resolve; include/pgorb.h) against the plain
sequential reference (tests/fuse_reference.py) on constructed cases and SearchInNeighbors scenes (tests/fuse_cases.py)."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_cases as FC  # noqa: E402
import fuse_reference as FR  # noqa: E402
from pilotguru_amd.orb import KF_POSE_DTYPE  # noqa: E402

EDGES = ["null", "bad", "in_kf", "behind", "outside_image", "on_max_bound", "on_depth_min", "on_depth_max", "depth_low",
         "depth_high", "angle", "octave_above", "chi2", "chi2_near", "tie", "dist_50", "dist_51", "no_match", "no_candidate",
         "added", "merged", "replaced", "kf_point_bad", "obs_tie", "overlap"]


@pytest.fixture(scope="module")
def cases():
    return FC.edge_cases()


def test_fuse_symbols_and_null_context():
    from pilotguru_amd import _lib
    L = _lib.lib()
    for name in ("pgorb_fuse", "pgorb_fuse_batch_device"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.pgorb_fuse(None, None, None, 0, None, 0, 0.0, 640.0, 0.0, 480.0, None, 0, *([None] * 5), 0, None, 3.0, *([None] * 4)) == -1
    assert L.pgorb_fuse_batch_device(None, None, None, None, 1, None, None, None, 1, None, None, 0.0, 640.0, 0.0, 480.0, None, 0,
                                     *([None] * 5), 1, None, None, 3.0, *([None] * 5), None) == -1


def test_cases_reach_every_edge(cases):
    hits = collections.Counter()
    for c in cases:
        FC.run_reference(c, hits=hits)
    missing = [e for e in EDGES if not hits[e]]
    assert not missing, (missing, dict(hits))


def test_every_rule_mutant_is_caught(cases):
    want = [FC.run_reference(c) for c in cases]
    for name, rules in FR.MUTANTS.items():
        assert any(not FC.same(w, FC.run_reference(c, rules)) for w, c in zip(want, cases)), name


@pytest.mark.parametrize("seed", range(40))
def test_two_pass_decomposition_equals_the_sequential_fuse(seed):
    """The kernels' specification: every query matched on the entry state, then each slot's chain in query order with observation
    sets as unions, equals ORBmatcher::Fuse run query after query on real objects (heavy slot collisions)."""
    c = FC.collision_case(seed)
    kf, _, _, q = c.build()
    nf2, acts, slots2 = FR.fuse_two_pass(kf, q, c.th)
    nf, a, bi, bd, slots = FC.run_reference(c)
    assert nf2 == nf
    assert [x[0] for x in acts] == list(a) and [x[1] for x in acts] == list(bi) and [x[2] for x in acts] == list(bd)
    assert [-1 if s is None else s.id for s in slots2] == list(slots)


def test_collision_cases_hold_long_chains():
    longest, kinds = 0, set()
    for seed in range(40):
        a, bi = FC.run_reference(FC.collision_case(seed))[1:3]
        per = collections.Counter(int(b) for x, b in zip(a, bi) if x >= FR.ADDED)
        longest = max([longest] + list(per.values()))
        kinds |= {int(x) for x in a}
    assert longest >= 4 and kinds == set(range(6)), (longest, kinds)


def test_python_mirror_rejects_bad_inputs():
    import pilotguru_amd as pg
    c = FC.collision_case(0)
    kid, k, d, P, b = c.kf
    K = FC.MC.KeyFrameArrays(None, k, d)
    pts, pd, pb, st, ob = FC.table_arrays(c.points)
    T = pg.MapPointTable(pts, pd, pb, st, ob)
    slots, q = c.slots(), np.array(c.queries, np.int32)
    fuse = pg.ORBmatcher().Fuse
    bad_inputs = [
        lambda: pg.MapPointTable(pts, pd[:-1], pb, st, ob),                      # descriptor rows
        lambda: pg.MapPointTable(pts, pd, pb[:-1], st, ob),                      # bad flags
        lambda: pg.MapPointTable(pts, pd, pb, st[:-1], ob),                      # obs_start length
        lambda: pg.MapPointTable(pts, pd, pb, st, ob[:-1]),                      # fewer ids than obs_start says
        lambda: pg.MapPointTable(pts, pd, pb, st, _unsorted(st, ob)),            # an unsorted list
        lambda: fuse(K, P, kid, slots[:-1], T, q, bounds=b),                     # slots length
        lambda: fuse(K, P, kid, slots, T, np.append(q, len(pts)), bounds=b),     # query out of range
        lambda: fuse(K, P, kid, slots, T, np.append(q, q[q >= 0][0]), bounds=b), # a repeated query
        lambda: fuse(K, P, kid + 1, slots, T, q, bounds=b),                      # occupants do not list the key frame
        lambda: fuse(K, P, kid, np.where(slots >= 0, 10 ** 6, -1), T, q, bounds=b),
        lambda: fuse(K, P, kid, slots, T, q, th=0.0, bounds=b),
        lambda: fuse(FC.MC.KeyFrameArrays(None, k, d[:-1]), P, kid, slots, T, q, bounds=b),
    ]
    for i, f in enumerate(bad_inputs):
        with pytest.raises(ValueError):
            f()
            pytest.fail("input %d was accepted" % i)


def _unsorted(st, ob):
    ob = ob.copy()
    for i in range(len(st) - 1):
        if st[i + 1] - st[i] >= 2:
            ob[st[i]], ob[st[i] + 1] = ob[st[i] + 1], ob[st[i]]
            return ob
    raise AssertionError("no list of two")


# ---------------------------------------------------------------- GPU
def _extractor(w=640, h=480):
    import pilotguru_amd as pg
    return pg.ORBextractor(2000, FC.MC.SCALE, FC.NLEVELS, 20, 7, max_width=w, max_height=h)


@pytest.mark.gpu
def test_gpu_single_call_equals_reference(cases):
    ext = _extractor()
    for c in cases + [FC.collision_case(s) for s in range(12)]:
        want = FC.run_reference(c)
        got = FC.run_gpu(c, ext)
        assert FC.same(want, got), (c.name, want, got)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,npts,focal", [(640, 480, 1000, 500.0), (1920, 1080, 2000, 1000.0)])
def test_gpu_search_in_neighbors_equals_reference(w, h, npts, focal):
    ext = _extractor(w, h)
    cur, targets, points = FC.neighbourhood(5, w, h, 20, npts, focal)
    want_n = FR.search_in_neighbors(cur, targets)
    want = FC.map_state([cur] + targets, points)
    cur, targets, points = FC.neighbourhood(5, w, h, 20, npts, focal)
    seen = set()
    got_n = FC.search_in_neighbors_gpu(ext, cur, targets, points, seen_actions=seen)
    assert got_n == want_n
    got = FC.map_state([cur] + targets, points)
    assert got[0] == want[0], "slots differ"
    assert got[1] == want[1], "points differ"
    assert seen == set(range(6)), seen
    assert sum(want_n) > 100


@pytest.mark.gpu
def test_gpu_batched_form_equals_reference(cases):
    ext = _extractor()
    empty = FC.Case("empty", cases[0].kf, cases[0].points, [])
    batch = cases + [empty] + [FC.collision_case(s) for s in range(8)]
    out = FC.run_gpu_batched(batch, ext)
    for c, got in zip(batch, out):
        assert FC.same(FC.run_reference(c), got[:5]), c.name
        assert np.all(got[5] == -9), (c.name, "wrote past nq")


# ---------------------------------------------------------------- the C++ mirror (pilotguru_amd/host/orb_extractor.hpp)
CPP_DRIVER = r"""
// reads cases written by tests/test_fuse.py and prints what pgorb::ORBmatcher::Fuse returns: "nfused", then the actions, best
// indices, best distances and slots afterwards, one line each, or the exception
#include <cstdio>
#include <cstring>
#include <fstream>
#include "pilotguru_amd/host/orb_extractor.hpp"
using namespace pgorb;
template <class T> static void rd(std::ifstream& f, std::vector<T>& v) { int32_t n; f.read((char*)&n, 4); v.resize(n); if (n) f.read((char*)v.data(), (size_t)n * sizeof(T)); }
static void line(const std::vector<int32_t>& v) { for (size_t i = 0; i < v.size(); i++) std::printf(i ? " %d" : "%d", v[i]); std::printf("\n"); }
int main(int argc, char** argv)
{
    const bool run = argc > 1 && std::strcmp(argv[1], "run") == 0;        // "check": no context, the wrapper's checks only
    ORBextractor* ext = run ? new ORBextractor(1000, 1.2f, 8, 20, 7, 640, 480) : nullptr;
    ORBmatcher m(ext ? ext->context() : nullptr);
    for (int a = 2; a < argc; a++) {
        std::ifstream f(argv[a], std::ios::binary);
        Frame F; MapPointTable T; pgorb_kf_pose pose; uint64_t kfId; float th;
        std::vector<int32_t> slots, queries, action, bi, bd, out;
        rd(f, F.mvKeysUndistorted); rd(f, F.mDescriptors);
        f.read((char*)&pose, sizeof pose); f.read((char*)&kfId, 8);
        f.read((char*)&F.mnMinX, 4); f.read((char*)&F.mnMaxX, 4); f.read((char*)&F.mnMinY, 4); f.read((char*)&F.mnMaxY, 4);
        rd(f, slots); rd(f, T.points); rd(f, T.descriptors); rd(f, T.bad); rd(f, T.obsStart); rd(f, T.obsKf); rd(f, queries);
        f.read((char*)&th, 4);
        try {
            std::printf("%d\n", m.Fuse(F, pose, kfId, slots, T, queries, action, th, &bi, &bd, &out));
            line(action); line(bi); line(bd); line(out);
        } catch (const std::invalid_argument&) { std::printf("invalid_argument\n");
        } catch (const std::runtime_error&) { std::printf("runtime_error\n"); }
    }
    delete ext;
    return 0;
}
"""


def _cpp_driver(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = os.path.join(str(tmp_path), "fuse_driver.cc"), os.path.join(str(tmp_path), "fuse_driver")
    open(src, "w").write(CPP_DRIVER)
    lib = os.path.join(root, "pilotguru_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", root, src, "-o", exe, "-L", lib, "-lpgorb", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _write_case(path, c, slots=None, queries=None, kf_id=None, desc=None, th=None, unsorted=False):
    kid, k, d, P, b = c.kf
    pts, pd, pb, st, ob = FC.table_arrays(c.points)
    ob = _unsorted(st, ob) if unsorted else ob

    def arr(a, dt):
        a = np.ascontiguousarray(a, dt)
        return np.int32(a.shape[0] if a.ndim else 1).tobytes() + a.tobytes()
    d = d if desc is None else desc
    with open(path, "wb") as f:
        f.write(arr(k, k.dtype) + np.int32(np.asarray(d).size).tobytes() + np.ascontiguousarray(d, np.uint8).tobytes() +
                np.asarray(P, KF_POSE_DTYPE).tobytes() + np.uint64(kid if kf_id is None else kf_id).tobytes() +
                np.array(b, np.float32).tobytes() + arr(c.slots() if slots is None else slots, np.int32) + arr(pts, pts.dtype) +
                np.int32(pd.size).tobytes() + pd.tobytes() + arr(pb, np.uint8) + arr(st, np.int32) + arr(ob, np.uint64) +
                arr(np.array(c.queries if queries is None else queries, np.int32), np.int32) +
                np.float32(c.th if th is None else th).tobytes())


def _run_driver(exe, mode, paths):
    return subprocess.run([exe, mode] + paths, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines()


def test_cpp_mirror_rejects_bad_inputs_before_calling_the_library(tmp_path):
    """pgorb::ORBmatcher::Fuse throws std::invalid_argument for every input pgorb_fuse would refuse, before any pointer reaches
    the library; well-formed input reaches it (a NULL context here, so PGORB_E_ARG comes back as std::runtime_error)."""
    exe = _cpp_driver(tmp_path)
    c = FC.collision_case(0)
    slots, q = c.slots(), np.array(c.queries, np.int32)
    variants = [dict(), dict(queries=np.append(q, len(c.points))), dict(queries=np.append(q, q[q >= 0][0])),
                dict(slots=slots[:-1]), dict(slots=np.where(slots >= 0, 10 ** 6, -1)), dict(kf_id=8),
                dict(desc=c.kf[2][:-1]), dict(th=0.0), dict(unsorted=True)]
    paths = []
    for n, kw in enumerate(variants):
        paths.append(os.path.join(str(tmp_path), "case%d.bin" % n))
        _write_case(paths[-1], c, **kw)
    got = _run_driver(exe, "check", paths)
    assert got == ["runtime_error"] + ["invalid_argument"] * (len(variants) - 1), got


@pytest.mark.gpu
def test_gpu_cpp_mirror_equals_reference(tmp_path, cases):
    exe = _cpp_driver(tmp_path)
    chosen = cases + [FC.collision_case(s) for s in range(4)]
    paths = []
    for n, c in enumerate(chosen):
        paths.append(os.path.join(str(tmp_path), "case%d.bin" % n))
        _write_case(paths[-1], c)
    got = _run_driver(exe, "run", paths)
    want = []
    for c in chosen:
        nf, a, bi, bd, sl = FC.run_reference(c)
        want += ["%d" % nf] + [" ".join("%d" % x for x in v) for v in (a, bi, bd, sl)]
    assert got == want
