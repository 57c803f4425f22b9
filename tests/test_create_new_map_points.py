"""LocalMapping::CreateNewMapPoints on the GPU (pilotguru_amd/csrc/mapping.hip, k_cnm_*; include/pgorb.h) against the plain
sequential reference (tests/mapping_reference.py) on constructed scenes (tests/mapping_cases.py)."""
import collections
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mapping_cases as MC  # noqa: E402
import mapping_reference as MR  # noqa: E402
from pilotguru_amd.orb import KF_POSE_DTYPE  # noqa: E402

SEEDS = (0, 1, 2)
# the rejections every seeded scene reaches (the reference's hit counters)
EDGES = ["parallax_low", "parallax_negative", "z1_behind", "z2_behind", "chi2_1_rejected", "scale_low", "scale_high",
         "baseline_skipped", "triangulated", "svd_5_sweeps"]


def _same(want, got):
    pts, cnt, F, ep, h = want
    gp, gc, gF, gep, gh = got[:5]
    return (MC.same_point_lists(pts, gp) and [int(x) for x in cnt] == [int(x) for x in gc] and
            np.asarray(F, np.float32).tobytes() == np.asarray(gF, np.float32).tobytes() and
            np.asarray(ep, np.float32).tobytes() == np.asarray(gep, np.float32).tobytes() and np.array_equal(np.asarray(h), np.asarray(gh)))


def test_scenes_reach_every_edge():
    hits = collections.Counter()
    for seed in SEEDS:
        MC.run_reference(*MC.scene(seed), hits=hits)
    missing = [e for e in EDGES if not hits[e]]
    assert not missing, (missing, dict(hits))


def test_every_rule_mutant_is_caught():
    want = {seed: MC.run_reference(*MC.scene(seed)) for seed in SEEDS}
    for name, rules in MR.MUTANTS.items():
        assert any(not _same(want[s], MC.run_reference(*MC.scene(s), rules=rules)) for s in SEEDS), name


@pytest.mark.parametrize("seed", range(6))
def test_parallel_first_success_equals_the_sequential_loop(seed):
    KF1, neigh = MC.scene(100 + seed, nneigh=5 + seed)
    pts = MC.run_reference(KF1, neigh)[0]
    assert pts, "the scene makes no point"
    assert MC.same_point_lists(pts, MC.parallel_first_success(KF1, neigh))


def test_first_success_wins_and_a_failure_passes_on():
    """An idx1 that triangulates with several neighbours gets the first one's point; one that fails with an earlier neighbour and
    succeeds with a later one gets the later one's."""
    KF1, neigh = MC.scene(0)
    tried = collections.defaultdict(list)
    for s, (m12, res) in sorted(MC.per_pair_results(KF1, neigh).items()):
        for i, r in res.items():
            tried[i].append((s, r is not None))
    owner = {q[1]: q[0] for q in MC.run_reference(KF1, neigh)[0]}
    first_of_many = [i for i, t in tried.items() if sum(ok for _, ok in t) >= 2]
    failed_then_ok = [i for i, t in tried.items() if not t[0][1] and any(ok for _, ok in t[1:])]
    assert first_of_many and failed_then_ok, (len(first_of_many), len(failed_then_ok))
    for i in first_of_many + failed_then_ok:
        assert owner[i] == next(s for s, ok in tried[i] if ok)


def test_create_new_map_points_symbols_and_null_context():
    from pilotguru_amd import _lib
    L = _lib.lib()
    for name in ("pgorb_create_new_map_points", "pgorb_create_new_map_points_batch_device"):
        assert hasattr(L, name)
    assert L.pgorb_create_new_map_points(None, *([None] * 3), 0, *([None] * 3), 0, None, 0, *([None] * 15)) == -1
    assert L.pgorb_create_new_map_points_batch_device(None, None, None, None, 1, *([None] * 7), 0, None, None, 1, *([None] * 8)) == -1


class _Ctx:
    """Enough of an extractor for the wrapper's argument checks, which run before the library is called."""
    ext = None


def test_python_wrapper_rejects_bad_sizes():
    import pilotguru_amd as pg
    KF1, neigh = MC.scene(0, nneigh=2)
    K1 = MC.KeyFrameArrays(None, KF1["k"], KF1["d"])
    Ks = [MC.KeyFrameArrays(None, K["k"], K["d"]) for K in neigh]
    fvs, poses, med = [K["fv"] for K in neigh], [K["pose"] for K in neigh], [K["median"] for K in neigh]
    call = pg.LocalMapping.CreateNewMapPoints
    with pytest.raises(ValueError):
        call(K1, Ks, KF1["fv"], fvs[:1], KF1["pose"], poses, med)
    with pytest.raises(ValueError):
        call(K1, Ks, KF1["fv"], fvs, KF1["pose"], poses, med[:1])
    with pytest.raises(ValueError):
        call(K1, Ks, KF1["fv"], fvs, KF1["pose"], poses, med, has_point1=np.zeros(K1.N - 1, np.uint8))
    with pytest.raises(ValueError):
        call(K1, Ks, KF1["fv"], fvs, KF1["pose"], poses, med, has_points=[K["h"][:-1] for K in neigh])
    bad = MC.KeyFrameArrays(None, neigh[0]["k"], neigh[0]["d"][:-1])
    with pytest.raises(ValueError):
        call(K1, [bad, Ks[1]], KF1["fv"], fvs, KF1["pose"], poses, med)
    with pytest.raises(ValueError):
        call(K1, Ks, (KF1["fv"][0], KF1["fv"][1][:-1], KF1["fv"][2]), fvs, KF1["pose"], poses, med)
    with pytest.raises(ValueError):
        call(K1, Ks * 33, KF1["fv"], fvs * 33, KF1["pose"], poses * 33, med * 33)


# ---------------------------------------------------------------- GPU
def _extractor(w=640, h=480, batch=1):
    import pilotguru_amd as pg
    return pg.ORBextractor(1000, MC.SCALE, MC.NLEVELS, 20, 7, max_width=w, max_height=h, max_batch=batch)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_gpu_single_call_equals_reference(seed):
    ext = _extractor()
    KF1, neigh = MC.scene(seed)
    want = MC.run_reference(KF1, neigh)
    got = MC.run_gpu(KF1, neigh, ext)
    assert len(want[0]) > 50
    assert _same(want, got), (len(want[0]), len(got[0]), want[1], got[1])


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,focal", [(640, 480, 500.0), (1920, 1080, 1000.0)])
def test_gpu_twenty_neighbours_equal_reference(w, h, focal):
    """20 neighbours (the monocular nn of :212) over 600 points: every rejection is reached and the points agree bit for bit."""
    ext = _extractor()
    KF1, neigh = MC.scene(7, w=w, h=h, nneigh=20, npts=600, nodes=90, focal=focal)
    hits = collections.Counter()
    want = MC.run_reference(KF1, neigh, hits=hits)
    assert len(want[0]) > 150
    for e in ("parallax_low", "chi2_1_rejected", "scale_low", "scale_high", "z1_behind", "z2_behind"):
        assert hits[e], e
    got = MC.run_gpu(KF1, neigh, ext)
    assert _same(want, got), (len(want[0]), len(got[0]), want[1], got[1])


RIDE_NEIGHBOURS = [1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 24, 28, 32, 36, 40, 44, 48, 52]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,nf", [(640, 480, 1000), (1920, 1080, 2000)])
def test_gpu_synthetic_ride_equals_reference(tmp_path, w, h, nf):
    """Key frame 0 of a synth_ride and 20 neighbours 1-52 frames on (a sideways camera over a fronto-parallel plane, as
    sideways_geometry in tools/next_tier_bench.py): extraction, FeatureVectors and CreateNewMapPoints on the GPU, the points equal
    the reference's bit for bit.  The nearest neighbour is skipped by the baseline test, near ones fail the parallax limit and
    mismatched octaves the scale test.  (With equal octaves the matcher's line test, 3.84 sigma^2, leaves no room for the
    5.991 sigma^2 reprojection test to fail on a ride; the constructed scenes reach it.)"""
    import pilotguru_amd as pg
    from pilotguru_amd import vocab as V
    from pilotguru_amd.synth import synth_ride
    dx, dy = 3, 1
    ride = synth_ride(5, w, h, max(RIDE_NEIGHBOURS) + 1, dx=dx, dy=dy)
    ext = pg.ORBextractor(nf, MC.SCALE, MC.NLEVELS, 20, 7, max_width=w, max_height=h)
    desc, weight, parent = V.synth_vocabulary(6, 4, seed=4)
    path = os.path.join(str(tmp_path), "voc.txt")
    V.write_vocabulary_text(path, 6, 4, desc, weight, parent)
    voc = V.ORBVocabulary(text_file=path)
    voc.upload(ext)
    frames = [0] + RIDE_NEIGHBOURS
    kps, descs, fvs = {}, {}, {}
    for f in frames:
        F = pg.Frame(ext, ride[f])
        kps[f], descs[f] = F.mvKeysUndistorted, F.mDescriptors
        fvs[f] = voc.transform(F.mDescriptors, 2)[1]
    KF1, neigh = MC.ride_scene(kps, descs, fvs, frames, w, h, dx, dy)
    hits = collections.Counter()
    want = MC.run_reference(KF1, neigh, hits=hits)
    assert len(want[0]) > 300 and want[1][0] == -1, (len(want[0]), want[1])
    assert hits["parallax_low"] and (hits["scale_low"] + hits["scale_high"]), dict(hits)
    got = MC.run_gpu(KF1, neigh, ext)
    assert _same(want, got), (len(want[0]), len(got[0]), want[1], got[1])


@pytest.mark.gpu
def test_gpu_batched_form_equals_reference():
    """Four key frames in one call, with NaN / 0xFF padding, an empty neighbour list and a slot table wider than needed."""
    ext = _extractor()
    problems = [MC.scene(s, nneigh=5 + s) for s in range(3)]
    KF1, neigh = MC.scene(3)
    problems.append((KF1, []))
    out = MC.run_gpu_batched(problems, ext, M=12)
    for (KF1, neigh), got in zip(problems, out):
        want = MC.run_reference(KF1, neigh)
        assert _same(want, got), (len(want[0]), len(got[0]), want[1], got[1])
        assert (got[5][len(neigh):] == 0).all()


@pytest.mark.gpu
def test_gpu_batched_form_with_device_feature_vectors():
    """The batch with FeatureVectors built on the device by pgorb_feature_vectors_batch_device from the scenes' node ids."""
    import torch
    ext = _extractor()
    problems = [MC.scene(20 + s) for s in range(3)]

    def device_fv(frames, cap):
        B = len(frames)
        node = np.zeros((B, cap), np.uint32)
        n = np.zeros(B, np.int32)
        for f, F in enumerate(frames):
            nodes, starts, feats = F["fv"]
            for a in range(len(nodes)):
                node[f, feats[starts[a]:starts[a + 1]]] = nodes[a]
            n[f] = len(F["k"])
        dn, dcnt = torch.from_numpy(node).cuda(), torch.from_numpy(n).cuda()
        fvn = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
        fvs = torch.zeros((B, cap + 1), dtype=torch.int32, device="cuda")
        fvf = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
        nfv = torch.zeros(B, dtype=torch.int32, device="cuda")
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        vp = lambda t: C.c_void_p(t.data_ptr())
        ext._check(ext._L.pgorb_feature_vectors_batch_device(ext._h, vp(dn), vp(dcnt), B, cap, vp(fvn), vp(fvs), vp(fvf), vp(nfv), s))
        device_fv.keep = (dn, dcnt)
        return fvn, fvs, fvf, nfv
    out = MC.run_gpu_batched(problems, ext, device_fv=device_fv)
    for (KF1, neigh), got in zip(problems, out):
        assert _same(MC.run_reference(KF1, neigh), got)


# ---------------------------------------------------------------- the C++ mirror (pilotguru_amd/host/orb_extractor.hpp)
CPP_DRIVER = r"""
// reads key frames written by tests/test_create_new_map_points.py and prints what pgorb::LocalMapping::CreateNewMapPoints returns:
// "npoints count..." then one line per point (slot idx1 idx2 and the float bits of pos, normal, min, max), or the exception
#include <cstdio>
#include <cstring>
#include <fstream>
#include "pilotguru_amd/host/orb_extractor.hpp"
using namespace pgorb;
template <class T> static void rd(std::ifstream& f, std::vector<T>& v, int32_t n) { v.resize(n); if (n) f.read((char*)v.data(), (size_t)n * sizeof(T)); }
static int32_t i32(std::ifstream& f) { int32_t v; f.read((char*)&v, 4); return v; }
static void readKF(std::ifstream& f, KeyFrame& K)
{
    const int32_t n = i32(f), nfv = i32(f), nstart = i32(f), nfeat = i32(f), nhas = i32(f), ndesc = i32(f);
    rd(f, K.frame.mvKeysUndistorted, n); rd(f, K.frame.mDescriptors, ndesc); rd(f, K.hasPoint, nhas);
    rd(f, K.featVec.mNode, nfv); rd(f, K.featVec.mStart, nstart); rd(f, K.featVec.mFeat, nfeat);
    f.read((char*)&K.pose, sizeof K.pose); f.read((char*)&K.medianDepth, 4);
}
static unsigned bits(float x) { unsigned u; std::memcpy(&u, &x, 4); return u; }
int main(int argc, char** argv)
{
    const bool run = argc > 1 && std::strcmp(argv[1], "run") == 0;        // "check": no context, the wrapper's checks only
    ORBextractor* ext = run ? new ORBextractor(1000, 1.2f, 8, 20, 7, 640, 480) : nullptr;
    LocalMapping lm(ext ? ext->context() : nullptr);
    for (int a = 2; a < argc; a++) {
        std::ifstream f(argv[a], std::ios::binary);
        const int32_t nn = i32(f);
        KeyFrame K1;
        std::vector<KeyFrame> K(nn);
        readKF(f, K1);
        std::vector<const KeyFrame*> neigh;
        for (int s = 0; s < nn; s++) { readKF(f, K[s]); neigh.push_back(&K[s]); }
        std::vector<pgorb_new_map_point> pts;
        std::vector<int32_t> count;
        try {
            const int np = lm.CreateNewMapPoints(K1, neigh, pts, count);
            std::printf("%d", np);
            for (size_t s = 0; s < count.size(); s++) std::printf(" %d", count[s]);
            std::printf("\n");
            for (const pgorb_new_map_point& p : pts)
                std::printf("%d %d %d %08x %08x %08x %08x %08x %08x %08x %08x\n", p.neighbour, p.idx1, p.idx2, bits(p.pos[0]), bits(p.pos[1]),
                            bits(p.pos[2]), bits(p.normal[0]), bits(p.normal[1]), bits(p.normal[2]), bits(p.min_distance), bits(p.max_distance));
        } catch (const std::invalid_argument&) { std::printf("invalid_argument\n");
        } catch (const std::runtime_error&) { std::printf("runtime_error\n"); }
    }
    delete ext;
    return 0;
}
"""


def _cpp_driver(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = os.path.join(str(tmp_path), "cnm_driver.cc"), os.path.join(str(tmp_path), "cnm_driver")
    open(src, "w").write(CPP_DRIVER)
    lib = os.path.join(root, "pilotguru_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", root, src, "-o", exe, "-L", lib, "-lpgorb", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _write_scene(path, KF1, neigh):
    def kf(K):
        fv = [np.asarray(x) for x in K["fv"]]
        d = np.ascontiguousarray(K["d"], np.uint8)
        head = np.array([len(K["k"]), len(fv[0]), len(fv[1]), len(fv[2]), len(K["h"]), d.size], np.int32)
        return (head.tobytes() + np.ascontiguousarray(K["k"]).tobytes() + d.tobytes() + np.asarray(K["h"], np.uint8).tobytes() +
                fv[0].astype(np.uint32).tobytes() + fv[1].astype(np.int32).tobytes() + fv[2].astype(np.uint32).tobytes() +
                np.asarray(K["pose"], KF_POSE_DTYPE).tobytes() + np.float32(K.get("median", 0)).tobytes())
    with open(path, "wb") as f:
        f.write(np.int32(len(neigh)).tobytes() + kf(KF1) + b"".join(kf(K) for K in neigh))


def _run_driver(exe, mode, paths):
    import subprocess
    return subprocess.run([exe, mode] + paths, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines()


def test_cpp_mirror_checks_sizes_before_calling_the_library(tmp_path):
    """pgorb::LocalMapping::CreateNewMapPoints refuses descriptors, masks and FeatureVectors of the wrong size, in KF1 or in a
    neighbour, with std::invalid_argument before any pointer reaches the library; well-formed input reaches it (a NULL context
    here, so the library's PGORB_E_ARG comes back as std::runtime_error)."""
    exe = _cpp_driver(tmp_path)
    KF1, neigh = MC.scene(0, nneigh=2)

    def edit(K, **kw):
        K = dict(K)
        K.update(kw)
        return K
    variants = [("well formed", KF1, neigh), ("empty masks", edit(KF1, h=np.zeros(0, np.uint8)), [edit(K, h=np.zeros(0, np.uint8)) for K in neigh]),
                ("short KF1 mask", edit(KF1, h=KF1["h"][:-1]), neigh),
                ("long neighbour mask", KF1, [neigh[0], edit(neigh[1], h=np.zeros(len(neigh[1]["k"]) + 1, np.uint8))]),
                ("short neighbour descriptors", KF1, [edit(neigh[0], d=neigh[0]["d"][:-1]), neigh[1]]),
                ("KF1 starts of wrong length", edit(KF1, fv=(KF1["fv"][0], KF1["fv"][1][:-1], KF1["fv"][2])), neigh),
                ("neighbour features shorter than start[n]", KF1, [neigh[0], edit(neigh[1], fv=(neigh[1]["fv"][0], neigh[1]["fv"][1], neigh[1]["fv"][2][:3]))]),
                ("65 neighbours", KF1, neigh * 32 + neigh[:1])]
    paths = []
    for k, (_, K1, nb) in enumerate(variants):
        paths.append(os.path.join(str(tmp_path), "scene%d.bin" % k))
        _write_scene(paths[-1], K1, nb)
    got = _run_driver(exe, "check", paths)
    assert got == ["runtime_error", "runtime_error"] + ["invalid_argument"] * 6, list(zip([v[0] for v in variants], got))


@pytest.mark.gpu
def test_gpu_cpp_mirror_equals_reference(tmp_path):
    exe = _cpp_driver(tmp_path)
    scenes = [MC.scene(s) for s in (30, 31)]
    paths = []
    for k, (KF1, neigh) in enumerate(scenes):
        paths.append(os.path.join(str(tmp_path), "scene%d.bin" % k))
        _write_scene(paths[-1], KF1, neigh)
    got = _run_driver(exe, "run", paths)
    want = []
    for KF1, neigh in scenes:
        pts, cnt = MC.run_reference(KF1, neigh)[:2]
        want.append(" ".join(["%d" % len(pts)] + ["%d" % c for c in cnt]))
        for p in pts:
            fl = list(p[3]) + list(p[4]) + [p[5], p[6]]
            want.append(" ".join(["%d" % p[0], "%d" % p[1], "%d" % p[2]] + ["%08x" % int(np.float32(x).view(np.uint32)) for x in fl]))
    assert got == want
