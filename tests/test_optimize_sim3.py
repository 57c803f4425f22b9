"""pgorb_optimize_sim3 (pilotguru_amd/csrc/optimize_sim3.hip): Optimizer::OptimizeSim3 on the GPU against the plain reference of
tests/optsim3_reference.py on the constructed loop candidates of tests/optsim3_cases.py.

The CPU tests anchor the reference (noise-free scenes, the numeric Jacobian against an analytic one, the 7 x 7 solve), hold every
case to the case condition, show what each rule mutant changes, and keep tests/golden/optsim3_spread.json up to date.  The GPU
tests compare the single call with the reference (integers exactly, floats by optsim3_cases.bounds), the batch with its singles
byte for byte, the two mirrors with the single call, the refusals, and the resident chain of LoopClosing::ComputeSim3's five steps.

On the MI355X the largest scaled differences from the reference over the cases and the chain were R 3.7e-9 (bound 2.4e-7),
t 1.5e-8 (4.8e-7), s 1.8e-7 (4.3e-6), scw_R 1.2e-7 (1.9e-6), scw_t 1.3e-7 (2.0e-6), scw_Ow 2.4e-7 (3.8e-6) and chi2 1.6e-6 (7.3e-5);
most float outputs equalled the reference's bit for bit, and every integer did."""
import ctypes as C
import json
import os
import sys
from dataclasses import replace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import optsim3_cases as OC  # noqa: E402
import optsim3_reference as OR  # noqa: E402

f32, f64 = np.float32, np.float64
NAMES = ("pgorb_optimize_sim3", "pgorb_optimize_sim3_batch_device")


def cases():
    return {c.name: c for c in OC.all_cases()}


# ---------------------------------------------------------------- presence
def test_symbols_and_mirrors_are_present():
    """The two entry points are exported and refuse a NULL context; both mirrors and the constants exist."""
    import pilotguru_amd as pg
    from pilotguru_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name)
    z = np.zeros(64, f32)
    p = C.c_void_p(z.ctypes.data)
    assert L.pgorb_optimize_sim3(None, p, 0, p, p, p, 0, p, p, p, None, 0, p, None, p, 10.0, 0, p, p, None, None, None, None) == _lib.PGORB_E_ARG
    assert L.pgorb_optimize_sim3_batch_device(None, p, p, 1, p, p, 0, p, p, p, None, 0, p, None, p, 10.0, 0, p, p, None, None, None, None, None,
                                              None) == _lib.PGORB_E_ARG
    assert (pg.OS3_FEW, pg.OS3_NONFINITE, pg.OS3_INFO) == (OR.OS3_FEW, OR.OS3_NONFINITE, 8)
    assert callable(pg.Optimizer.OptimizeSim3) and callable(pg.Optimizer.OptimizeSim3_batch_device)
    hpp = open(os.path.join(os.path.dirname(HERE), "pilotguru_amd", "host", "orb_extractor.hpp")).read()
    assert "OptimizeSim3Result OptimizeSim3(" in hpp and "pgorb_optimize_sim3(ctx_" in hpp
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "pgorb.h")).read()
    assert all(("int  %s(" % n) in hdr for n in NAMES) and "#define PGORB_OS3_INFO       8" in hdr


# ---------------------------------------------------------------- anchors
def test_noise_free_scenes_return_to_the_generating_sim3():
    """Started off the truth without noise, the result is the generating Sim3 up to the float rounding of the points and keypoints
    (a 1e-7 relative change of a point at 8 m moves its image by 1e-4 pixels)."""
    for seed, kw in ((401, {}), (402, dict(s=1.7, rot=0.6)), (403, dict(s=0.6, cam2=OC.K2_OTHER, octaves="mixed")), (404, dict(fix_scale=1))):
        c = OC.scene("anchor", seed, 60, start=(0.05, 0.1, 0.05), **kw)
        r = OC.run_reference(c)
        Rs, ts, s = c.true
        assert r["status"] == 0 and r["ret"] == 60 and r["nbad"] == 0
        assert np.abs(r["R"].reshape(3, 3) - Rs).max() < 2e-6 and np.abs(r["t"] - ts).max() < 2e-5 and abs(float(r["s"]) - s) < 2e-5, (seed, r["t"] - ts)
        assert float(r["chi2_12"].max()) < 1e-4 and float(r["chi2_21"].max()) < 1e-4


def test_numeric_jacobian_agrees_with_the_analytic_one_as_far_as_its_step_allows():
    """A central difference with delta = 1e-9 of an error of magnitude P (pixels) carries the rounding of the two evaluations,
    each a few ulps of P, divided by 2e-9; the truncation term is O(delta^2) and invisible.  The bound is measured from the scene:
    16 ulps at the largest projected coordinate over 2*delta.  The two differ (the step is that coarse) but stay inside it."""
    worst = 0.0
    for c in (OC.case("noisy_65"), OC.case("outliers_300"), OC.case("far_start_fixed")):
        E = OR.gather(c.keys1, c.octaves1, c.pose1, c.kf_point1, c.keys2, c.octaves2, c.pose2, c.kf_point2,
                      OR.merged_matches(c.matches12, c.new_matches12), c.points, c.bad, OC.INV_SIGMA2)
        est = OR.from_estimate(*c.estimate)
        act = np.ones(len(E), bool)
        Jn = OR.numeric_jacobian(est, E, act, bool(c.fix_scale), OR.LibM())
        Ja = OR.analytic_jacobian(est, E, act, bool(c.fix_scale))
        a0, a1, b0, b1 = OR.pair_errors(est, E)
        scale = max(float(np.abs(E.obs1 - np.stack([a0, a1], 1)).max()), float(np.abs(E.obs2 - np.stack([b0, b1], 1)).max()))      # the projections
        bound = 16.0 * float(np.spacing(scale)) / (2 * OR.DELTA_NUM)
        d = max(float(np.abs(np.array(Jn[k]) - np.array(Ja[k])).max()) for k in range(4))
        size = max(float(np.abs(np.array(Ja[k])).max()) for k in range(4))
        assert 0.0 < d <= bound and bound < 1e-5 * size, (c.name, d, bound, size)
        if c.fix_scale:
            assert all(not np.array(Jn[k])[6].any() for k in range(4))  # column 6 is exactly 0
        worst = max(worst, d / bound)
    assert worst > 0.01                                                 # the bound is not idle either


def test_the_7x7_solve_agrees_with_numpy():
    rng = np.random.RandomState(5)
    for _ in range(20):
        A = rng.normal(0, 1, (30, 7)) * rng.uniform(0.1, 100, 7)
        H, b = A.T @ A + 1e-3 * np.eye(7), rng.normal(0, 1, 7)
        x, ok = OR.ldlt_solve(H, b)
        want = np.linalg.solve(H, b)
        assert ok and np.abs(x - want).max() <= 1e-9 * np.abs(want).max() * np.linalg.cond(H) * 1e-4 + 1e-12
    assert not OR.ldlt_solve(-np.eye(7), np.ones(7))[1]


# ---------------------------------------------------------------- the cases
CASE_HITS = {"nine_left": "few", "few_0": "few", "few_9": "few", "start_at_truth": "ended_on_rejected", "start_at_truth_fixed": "ended_on_rejected",
             "far_start": "exp_large_sigma_large_theta", "far_start_fixed": "exp_small_sigma_large_theta", "clean_10": "exp_large_sigma_small_theta",
             "noisy_64": "exp_small_sigma_small_theta", "noisy_65": "lm_rejected"}


@pytest.mark.parametrize("name", OC.CASE_NAMES)
def test_case_meets_the_case_condition(name):
    """Across the reference's five forms the Levenberg trace and every classification are identical and no chi2 lies within 1e-4
    of th2; the case also does what it was built for."""
    c = OC.case(name)
    assert OC.condition(c) == []
    r, _, hits = OC.reference(c)["edges"]
    if name in CASE_HITS:
        assert hits.get(CASE_HITS[name]), (name, hits)


def test_cases_cover_the_counts_and_the_paths():
    ref = {n: OC.reference(c)["edges"][0] for n, c in cases().items()}
    assert {ref[n]["ncorr"] for n in ref} >= {10, 11, 63, 64, 65, 256, 257, 300}
    assert ref["ten_left"]["ncorr"] - ref["ten_left"]["nbad"] == 10 and ref["ten_left"]["status"] == 0
    assert ref["nine_left"]["ncorr"] - ref["nine_left"]["nbad"] == 9 and ref["nine_left"]["status"] == OR.OS3_FEW
    assert ref["nine_left"]["nbad"] == int((ref["nine_left"]["matches12_out"] < 0).sum() - (OC.case("nine_left").matches12 < 0).sum())
    assert any(r["nbad"] == 0 and r["more"] == 5 and r["status"] == 0 for r in ref.values())
    assert any(r["nbad"] > 0 and r["more"] == 10 and r["status"] == 0 for r in ref.values())
    assert {c.fix_scale for c in cases().values()} == {0, 1}
    c = OC.case("dropped_40")                                           # each reason a correspondence is dropped for
    m = c.matches12
    assert ((m >= 0) & (c.kf_point1 < 0)).any() and (c.kf_point2[m[m >= 0]] < 0).any() and c.bad[c.kf_point1[(m >= 0) & (c.kf_point1 >= 0)]].any()
    assert ref["dropped_40"]["ncorr"] == 40
    c = OC.case("outliers_300")
    assert (c.octaves1[c.matches12 >= 0] > 0).any() and (c.octaves2 > 0).any() and abs(c.true[2] - 1) < 1e-9 and OC.case("noisy_256").true[2] == 1.7
    assert (c.new_matches12 >= 0).sum() == 20 and ((c.new_matches12 >= 0) & (c.matches12 >= 0) & (c.new_matches12 != c.matches12)).any()
    assert ref["start_at_truth"]["trials"] == [1, 1]                    # rho == 0 on the first trial of both calls


def test_spread_file_is_up_to_date():
    """tests/golden/optsim3_spread.json (tests/golden/make_optsim3_spread.py writes it) holds what the reference shows now."""
    rec = OC.recorded_spread()
    assert sorted(rec) == sorted(OC.CASE_NAMES)
    for c in OC.all_cases():
        now = OC.spread(c)
        for k in OC.FLOAT_OUTPUTS:
            assert abs(now[k] - rec[c.name][k]) <= 1e-3 * max(now[k], rec[c.name][k]), (c.name, k, now[k], rec[c.name][k])


# ---------------------------------------------------------------- mutants
def _changed(mut, names=None):
    """The cases on which the mutant differs from the reference in a compared output."""
    rec = OC.recorded_spread()
    out = []
    for c in OC.all_cases():
        if names is None or c.name in names:
            d = OC.differences(c, OC.reference(c)["edges"][0], OC.run_reference(c, rules=OR.MUTANTS[mut]), rec[c.name])
            if d:
                out.append((c.name, d))
    return out


DETECTED = {"analytic_jacobian": None, "lambda_carried_across_calls": None, "more_iterations_swapped": None, "few_at_ten": ("ten_left",),
            "estimate_written_on_few": ("nine_left", "few_9"), "huber_off_in_second_call": ("huber_second_call",), "new_matches_ignored": ("outliers_300", "new_matches_50")}


@pytest.mark.parametrize("mut", sorted(DETECTED))
def test_mutant_changes_a_compared_output(mut):
    assert _changed(mut, DETECTED[mut]), mut


def test_mutant_remove_at_equal_shows_on_a_probe():
    """`>=` for `> th2` differs only when a chi2 EQUALS th2, which the case condition forbids on every compared case (there the two
    are equivalent, asserted below).  The probe: identity poses and S12, an exact start, and one correspondence entered twice
    with its KF1 observation moved by (+3, +1) and by (-3, -1) pixels at octave 0.  Every subtraction involved is exact, so the two
    gradients cancel bit for bit, b == 0, the step is 0 and rho == 0: nothing moves, and both edges hold chi2 = 9 + 1 = 10 exactly
    at the classification.  The reference keeps both pairs, the mutant removes them.  Not a GPU case."""
    c = OC.scene("probe", 14, 30, start=None, identity=True)
    used = np.flatnonzero(c.matches12 >= 0)
    i, j = int(used[3]), int(used[4])
    c.matches12[j], c.kf_point1[j] = c.matches12[i], c.kf_point1[i]
    c.keys1[j] = c.keys1[i] - np.array([3.0, 1.0], f32)
    c.keys1[i] = c.keys1[i] + np.array([3.0, 1.0], f32)
    tr = {}
    r = OC.run_reference(c, trace=tr)
    assert [float(tr["cls"][0][1][list(used).index(k)]) for k in (i, j)] == [10.0, 10.0] and r["trials"] == [1, 1]
    m = OC.run_reference(c, rules=OR.MUTANTS["remove_at_equal"])
    assert r["nbad"] == 0 and m["nbad"] == 2 and (r["matches12_out"][[i, j]] >= 0).all() and (m["matches12_out"][[i, j]] == -1).all()
    assert OC.condition(c) != []
    rec = OC.recorded_spread()
    for c in OC.all_cases():
        assert OC.differences(c, OC.reference(c)["edges"][0], OC.run_reference(c, rules=OR.MUTANTS["remove_at_equal"]), rec[c.name]) == [], c.name


def test_equivalent_mutants_are_equivalent():
    """Three rules cannot show in a compared output; each is asserted to be exactly that.
    x[6] not zeroed: under fix_scale column 6 of every Jacobian is exactly 0, so row 6 of H and b[6] are 0, the LDLT gives
    L[6][k] = 0 and x[6] = 0 / lambda = 0 by itself: identical in every bit.
    Errors recomputed before the classification: a call ends on a rejected trial only with rho == 0 (the trial's chi2 equals the
    estimate's) or after 10 rejections (lambda has grown by 2^45 by then: the trial is the estimate to the last bits), so the
    stale errors equal the recomputed ones within the bounds; on every other ending the last trial IS the estimate.  The cases
    start_at_truth* end both calls on a rejected trial.
    Edge order e12... then e21...: only the order of the sums changes, which is one more arithmetic form: every float within the
    bounds and every integer equal, except that the number of trials may differ where a fixed-scale case spends its last
    iteration on the rounding floor (the case condition holds for the forms it names, not for every order of the sums)."""
    rec = OC.recorded_spread()
    hit = 0
    for c in OC.all_cases():
        want, _, hits = OC.reference(c)["edges"]
        hit += hits.get("ended_on_rejected", 0)
        if c.fix_scale:
            got = OC.run_reference(c, rules=OR.MUTANTS["x6_not_zeroed"])
            assert all(np.array_equal(np.asarray(want[k]), np.asarray(got[k])) for k in want if k not in ("final", "scw_Tcw", "scw_Ow")), c.name
        assert OC.differences(c, want, OC.run_reference(c, rules=OR.MUTANTS["errors_recomputed_before_classification"]), rec[c.name]) == [], c.name
        d = OC.differences(c, want, OC.run_reference(c, rules=OR.MUTANTS["edge_order_blocked"]), rec[c.name])
        assert d == [] or (d == ["trials"] and c.fix_scale), (c.name, d)
    assert hit >= 4


def test_every_mutant_is_covered():
    assert set(OR.MUTANTS) == set(DETECTED) | {"remove_at_equal", "x6_not_zeroed", "errors_recomputed_before_classification", "edge_order_blocked"}


# ---------------------------------------------------------------- the Python mirror, without a device
class _KF:
    def __init__(self, ext, xy, octaves):
        self.ext, self.N, self.mvKeysUndistorted = ext, len(octaves), OC.keypoints(xy, octaves)


def _table(c):
    import pilotguru_amd as pg
    n = len(c.points)
    return pg.MapPointTable(OC.table(c.points)[:n], np.zeros((n, 32), np.uint8), c.bad, np.arange(n + 1, dtype=np.int32), np.zeros(max(n, 1), np.uint64))


def _mirror(c, ext=None):
    import pilotguru_amd as pg
    return pg.Optimizer.OptimizeSim3(_KF(ext, c.keys1, c.octaves1), _KF(ext, c.keys2, c.octaves2), OC.pose_record(c.pose1), OC.pose_record(c.pose2),
                                     c.kf_point1, c.kf_point2, c.matches12, _table(c), OC.estimate_record(c.estimate)[0], c.th2, bool(c.fix_scale),
                                     c.new_matches12)


def _variant(c, **over):
    v = OC.Case(c.name, c.keys1, c.octaves1, c.pose1, c.kf_point1, c.keys2, c.octaves2, c.pose2, c.kf_point2, c.matches12, c.new_matches12,
                c.points, c.bad, c.estimate, c.fix_scale, c.th2, c.true)
    for k, val in over.items():
        setattr(v, k, val)
    return v


def _bad_inputs(c):
    """(what, the case with it) for every input the checked call must refuse: see include/pgorb.h."""
    used = np.flatnonzero(OR.merged_matches(c.matches12, c.new_matches12) >= 0)
    used = used[c.kf_point1[used] >= 0]
    out = []

    def put(what, field, idx, value):
        a = np.array(getattr(c, field), copy=True)
        a[idx] = value
        out.append((what, _variant(c, **{field: a})))
    put("kf_point1 == npoints", "kf_point1", 0, len(c.points))
    put("kf_point1 < -1", "kf_point1", 1, -2)
    put("kf_point2 == npoints", "kf_point2", 2, len(c.points))
    put("matches12 == n2", "matches12", 3, c.n2)
    put("matches12 < -1", "matches12", 4, -2)
    put("new_matches12 == n2", "new_matches12", 5, c.n2)
    put("new_matches12 < -1", "new_matches12", 6, -2)
    put("octave == levels", "octaves1", used[0], OC.NLEVELS)
    put("octave < 0", "octaves2", OR.merged_matches(c.matches12, c.new_matches12)[used[1]], -1)
    put("a referenced point is NaN", "points", c.kf_point1[used[2]], np.nan)
    for k, v in (("Tcw", np.nan), ("fx", np.inf)):
        for which in ("pose1", "pose2"):
            P = dict(getattr(c, which))
            P[k] = P[k].copy() if k == "Tcw" else f32(v)
            if k == "Tcw":
                P["Tcw"][7] = v
            out.append(("%s.%s = %r" % (which, k, v), _variant(c, **{which: P})))
    R, t, s = c.estimate
    Rn = R.copy()
    Rn[4] = np.nan
    out += [("R NaN", _variant(c, estimate=(Rn, t, s))), ("t inf", _variant(c, estimate=(R, np.array([0, np.inf, 0], f32), s))),
            ("s == 0", _variant(c, estimate=(R, t, f32(0)))), ("s < 0", _variant(c, estimate=(R, t, f32(-1)))), ("s NaN", _variant(c, estimate=(R, t, f32(np.nan)))),
            ("th2 == 0", _variant(c, th2=0.0)), ("th2 < 0", _variant(c, th2=-1.0)), ("th2 NaN", _variant(c, th2=float("nan")))]
    return out


def test_mirror_refuses_malformed_input_without_a_device():
    """Pure host checks: every malformed input is a ValueError before any library call; well-formed input gets past them (to the
    missing extractor).  An unreferenced point may be anything."""
    c = OC.case("outliers_300")
    with pytest.raises(AttributeError):
        _mirror(c)
    pts = np.concatenate([c.points, np.full((1, 3), np.nan, f32)])
    with pytest.raises(AttributeError):
        _mirror(_variant(c, points=pts, bad=np.append(c.bad, 0).astype(np.uint8)))
    for what, v in _bad_inputs(c):
        if not what.startswith("octave"):                               # (the levels are the extractor's: checked with one, on the GPU)
            with pytest.raises(ValueError):
                _mirror(v)
                pytest.fail(what)
    with pytest.raises(ValueError):
        _mirror(_variant(c, matches12=c.matches12[:-1]))


def test_batched_wrapper_refuses_mistyped_or_short_tensors_without_a_device():
    import torch
    import pilotguru_amd as pg
    from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE, SIM3_ESTIMATE_DTYPE
    B, cap, nf = 2, 8, 4
    I = lambda *sh: torch.zeros(sh, dtype=torch.int32)  # noqa: E731
    U = lambda *sh: torch.zeros(sh, dtype=torch.uint8)  # noqa: E731
    good = dict(d_kps=U(nf, cap, KEYPOINT_DTYPE.itemsize), d_n=I(nf), d_pair_kf1=I(B), d_pair_kf2=I(B), d_pose=U(nf, KF_POSE_DTYPE.itemsize),
                d_kf_point=I(nf, cap), d_matches12=I(B, cap), d_points=U(5, 32), d_point_bad=U(5), d_estimate=U(B, SIM3_ESTIMATE_DTYPE.itemsize),
                d_new=I(B, cap), th2=10.0)

    def call(**over):
        a = dict(good, **over)
        return pg.Optimizer.OptimizeSim3_batch_device(None, a["d_kps"], a["d_n"], cap, a["d_pair_kf1"], a["d_pair_kf2"], a["d_pose"], a["d_kf_point"],
                                                      a["d_matches12"], 5, a["d_points"], a["d_point_bad"], a["d_estimate"], a["th2"], False, a["d_new"])
    with pytest.raises((AttributeError, RuntimeError)) as e:            # well-formed: past the checks, to the missing device or extractor
        call()
    assert not isinstance(e.value, ValueError)
    for over in (dict(d_pair_kf1=U(B * 4)), dict(d_pair_kf2=I(B + 1)), dict(d_matches12=U(B, cap * 4)), dict(d_matches12=I(B, cap + 1)),
                 dict(d_new=I(B, cap - 1)), dict(d_new=U(B, cap * 4)), dict(d_estimate=U(B, 51)), dict(d_kf_point=I(nf, cap - 1)),
                 dict(d_kps=U(nf, cap, 27)), dict(d_pose=U(nf - 1, KF_POSE_DTYPE.itemsize)), dict(d_points=U(4, 32)), dict(d_point_bad=U(4)),
                 dict(d_n=U(nf * 4)), dict(th2=0.0), dict(th2=float("nan"))):
        with pytest.raises(ValueError):
            call(**over)
            pytest.fail(repr(over.keys()))


# ---------------------------------------------------------------- the C++ mirror (pilotguru_amd/host/orb_extractor.hpp)
CPP_DRIVER = r"""
// reads problems written by tests/test_optimize_sim3.py and prints what pgorb::Optimizer::OptimizeSim3 returns: "nIn", then
// estimate | scwPose | matches12 | chi2_12 | chi2_21 | info as hex bytes, or the exception
#include <cstdio>
#include <cstring>
#include <fstream>
#include "pilotguru_amd/host/orb_extractor.hpp"
using namespace pgorb;
template <class T> static void rd(std::ifstream& f, std::vector<T>& v) { int32_t n; f.read((char*)&n, 4); v.resize(n); if (n) f.read((char*)v.data(), (size_t)n * sizeof(T)); }
static void hex(const void* p, size_t n) { for (size_t i = 0; i < n; i++) std::printf("%02x", ((const unsigned char*)p)[i]); }
int main(int argc, char** argv)
{
    const bool run = argc > 1 && std::strcmp(argv[1], "run") == 0;        // "check": no context, the mirror's checks only
    ORBextractor* ext = run ? new ORBextractor(1000, 1.2f, 8, 20, 7, 640, 480) : nullptr;
    for (int a = 2; a < argc; a++) {
        std::ifstream f(argv[a], std::ios::binary);
        Frame F1, F2; pgorb_kf_pose pose1, pose2; std::vector<int32_t> s1, s2, m12, nm12; std::vector<pgorb_map_point> points; std::vector<uint8_t> bad;
        pgorb_sim3_estimate est; float th2; int32_t fix;
        rd(f, F1.mvKeysUndistorted); rd(f, F2.mvKeysUndistorted); f.read((char*)&pose1, sizeof pose1); f.read((char*)&pose2, sizeof pose2);
        rd(f, s1); rd(f, s2); rd(f, m12); rd(f, nm12); rd(f, points); rd(f, bad); f.read((char*)&est, sizeof est); f.read((char*)&th2, 4); f.read((char*)&fix, 4);
        try {
            Optimizer O(ext ? ext->context() : nullptr);
            const OptimizeSim3Result r = O.OptimizeSim3(F1, F2, pose1, pose2, s1, s2, m12, nm12, points, bad, est, th2, fix != 0);
            std::printf("%d\n", r.inliers);
            hex(&r.estimate, sizeof r.estimate); hex(&r.scwPose, sizeof r.scwPose); hex(r.matches12.data(), r.matches12.size() * 4);
            hex(r.chi2_12.data(), r.chi2_12.size() * 4); hex(r.chi2_21.data(), r.chi2_21.size() * 4); hex(r.info, sizeof r.info);
            std::printf("\n");
        } catch (const std::invalid_argument&) { std::printf("invalid_argument\n");
        } catch (const std::runtime_error&) { std::printf("runtime_error\n"); }
    }
    delete ext;
    return 0;
}
"""


def _cpp_driver(tmp_path):
    import subprocess
    root = os.path.dirname(HERE)
    src, exe = os.path.join(str(tmp_path), "optsim3_driver.cc"), os.path.join(str(tmp_path), "optsim3_driver")
    open(src, "w").write(CPP_DRIVER)
    lib = os.path.join(root, "pilotguru_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", root, src, "-o", exe, "-L", lib, "-lpgorb", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _write_problem(path, c):
    def arr(a, dt):
        a = np.ascontiguousarray(a, dt)
        return np.int32(a.shape[0]).tobytes() + a.tobytes()
    k1, k2, pts = OC.keypoints(c.keys1, c.octaves1), OC.keypoints(c.keys2, c.octaves2), OC.table(c.points)[:len(c.points)]
    with open(path, "wb") as f:
        f.write(arr(k1, k1.dtype) + arr(k2, k2.dtype) + np.asarray(OC.pose_record(c.pose1)).tobytes() + np.asarray(OC.pose_record(c.pose2)).tobytes() +
                arr(c.kf_point1, np.int32) + arr(c.kf_point2, np.int32) + arr(c.matches12, np.int32) +
                arr(np.zeros(0, np.int32) if c.new_matches12 is None else c.new_matches12, np.int32) + arr(pts, pts.dtype) +
                arr(np.zeros(0, np.uint8) if c.bad is None else c.bad, np.uint8) + OC.estimate_record(c.estimate).tobytes() +
                f32(c.th2).tobytes() + np.int32(c.fix_scale).tobytes())


def _run_driver(exe, mode, paths):
    import subprocess
    return subprocess.run([exe, mode] + paths, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines()


def test_cpp_mirror_rejects_bad_inputs_before_calling_the_library(tmp_path):
    """pgorb::Optimizer::OptimizeSim3 throws std::invalid_argument for every input pgorb_optimize_sim3 would refuse, before any
    pointer reaches the library; well-formed input reaches it (a NULL context here, so PGORB_E_ARG comes back as std::runtime_error).
    (Without a context the mirror cannot know the levels: the octave rows are the library's, checked on the GPU.)"""
    exe = _cpp_driver(tmp_path)
    c = OC.case("outliers_300")
    bad = [(w, v) for w, v in _bad_inputs(c) if not w.startswith("octave")] + [("matches12 too short", _variant(c, matches12=c.matches12[:-1]))]
    paths = [os.path.join(str(tmp_path), "p%d.bin" % i) for i in range(len(bad) + 1)]
    _write_problem(paths[0], c)
    for path, (_, v) in zip(paths[1:], bad):
        _write_problem(path, v)
    out = _run_driver(exe, "check", paths)
    assert out[0] == "runtime_error"
    assert out[1:] == ["invalid_argument"] * len(bad), [w for (w, _), o in zip(bad, out[1:]) if o != "invalid_argument"]


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    e = pg.ORBextractor(1000, 1.2, OC.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=4)
    assert np.array_equal(np.asarray(e.GetInverseScaleSigmaSquares(), f32)[:OC.NLEVELS], OC.INV_SIGMA2)
    yield e
    e.close()


def _check(c, want, got, what):
    assert not isinstance(got, int), "%s (%s): error %r" % (c.name, what, got)
    rec = OC.recorded_spread()[c.name] if c.name in OC.CASE_NAMES else OC.spread(c)
    d = OC.scaled_differences(want, got)
    print("%s (%s): " % (c.name, what) + ", ".join("%s %.2g / %.2g" % (k, d[k], OC.bounds(rec)[k]) for k in OC.FLOAT_OUTPUTS))
    assert OC.differences(c, want, got, rec) == [], "%s (%s)" % (c.name, what)
    if want["status"]:
        assert not got["scw"].tobytes().strip(b"\0"), "%s: scw_pose is zeroed with a status" % c.name


@pytest.mark.gpu
@pytest.mark.parametrize("name", OC.CASE_NAMES)
def test_gpu_single_call_equals_the_reference(ext, name):
    c = OC.case(name)
    got = OC.run_gpu(c, ext)
    _check(c, OC.reference(c)["edges"][0], got, "single")
    if not got["status"]:
        P1 = OC.pose_record(c.pose1)
        assert all(got["scw"][k] == P1[k] for k in ("fx", "fy", "cx", "cy", "invfx", "invfy"))      # KF1's camera


@pytest.fixture(scope="module")
def singles(ext):
    return [OC.run_gpu(c, ext) for c in OC.all_cases()]


def _same(a, b):
    return a["bytes"] == b["bytes"] and a["ret"] == b["ret"] and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in
                                                                       ("matches12_out", "chi2_12", "chi2_21", "iterations", "trials", "status", "ncorr", "nbad", "more"))


@pytest.mark.gpu
def test_gpu_batch_equals_its_singles_byte_for_byte(ext, singles):
    got = OC.run_gpu_batch(OC.all_cases(), ext)
    for c, s, b in zip(OC.all_cases(), singles, got):
        assert _same(s, b) and b["tail_ok"], c.name


@pytest.mark.gpu
def test_gpu_batch_is_unchanged_by_pair_order_and_by_a_repeat(ext, singles):
    import torch
    cs = OC.all_cases()
    order = list(np.random.RandomState(3).permutation(len(cs)))
    a = OC.run_gpu_batch(cs, ext, order)
    b = OC.run_gpu_batch(cs, ext, order, stream=torch.cuda.Stream())
    for j, ra, rb in zip(order, a, b):
        assert _same(singles[j], ra) and _same(ra, rb), cs[j].name


@pytest.mark.gpu
def test_gpu_python_mirror_equals_the_single_call(ext, singles):
    for name in ("outliers_300", "nine_left", "few_0", "far_start_fixed", "dropped_40"):
        c = OC.case(name)
        s, m = singles[OC.CASE_NAMES.index(name)], _mirror(c, ext)
        assert m["ret"] == s["ret"] and np.asarray(m["estimate"]).tobytes() + np.asarray(m["scw_pose"]).tobytes() == s["bytes"], name
        assert np.array_equal(m["matches12_out"], s["matches12_out"]) and m["chi2_12"].tobytes() == s["chi2_12"].tobytes() and \
            m["chi2_21"].tobytes() == s["chi2_21"].tobytes(), name
        assert (m["status"], m["correspondences"], m["nbad"], m["iterations"], m["trials"], m["more_iterations"]) == \
            (s["status"], s["ncorr"], s["nbad"], s["iterations"], s["trials"], s["more"]), name


@pytest.mark.gpu
def test_gpu_cpp_mirror_equals_the_single_call(ext, singles, tmp_path):
    exe = _cpp_driver(tmp_path)
    names = ["outliers_300", "nine_left", "few_0", "far_start_fixed"]
    c = OC.case("outliers_300")
    o1 = c.octaves1.copy()
    o1[np.flatnonzero((OR.merged_matches(c.matches12, c.new_matches12) >= 0) & (c.kf_point1 >= 0))[0]] = OC.NLEVELS
    paths = [os.path.join(str(tmp_path), "%s.bin" % n) for n in names + ["octave"]]
    for n, path in zip(names, paths):
        _write_problem(path, OC.case(n))
    _write_problem(paths[-1], _variant(c, octaves1=o1))
    out = _run_driver(exe, "run", paths)
    assert out[-1] == "invalid_argument"
    for i, n in enumerate(names):
        s = singles[OC.CASE_NAMES.index(n)]
        info = np.array([s["status"], s["ncorr"], s["nbad"], s["iterations"][0], s["trials"][0], s["iterations"][1], s["trials"][1], s["more"]], np.int32)
        assert int(out[2 * i]) == s["ret"], n
        assert bytes.fromhex(out[2 * i + 1]) == s["bytes"] + s["matches12_out"].tobytes() + s["chi2_12"].tobytes() + s["chi2_21"].tobytes() + info.tobytes(), n


@pytest.mark.gpu
def test_gpu_library_refuses_malformed_input_and_limits(ext):
    """PGORB_E_ARG for every malformed input of the single call (and the Python mirror refuses the same before the library);
    16000 keypoints a key frame run, 16001 are PGORB_E_LIMIT in both forms; the batched form refuses th2 <= 0."""
    from pilotguru_amd import _lib
    c = OC.case("outliers_300")
    for what, v in _bad_inputs(c):
        assert OC.run_gpu(v, ext) == _lib.PGORB_E_ARG, what
        with pytest.raises(ValueError):
            _mirror(v, ext)
            pytest.fail(what)
    small = OC.case("noisy_11")
    pad = lambda a, n, fill: np.concatenate([a, np.full((n - len(a),) + a.shape[1:], fill, a.dtype)])  # noqa: E731
    def grown(n):
        return _variant(small, keys1=pad(small.keys1, n, 0), octaves1=pad(small.octaves1, n, 0), kf_point1=pad(small.kf_point1, n, -1),
                        matches12=pad(small.matches12, n, -1))
    at = OC.run_gpu(grown(OC.MAX_N), ext)
    s = OC.run_gpu(small, ext)
    assert not isinstance(at, int) and at["ret"] == s["ret"] and at["bytes"] == s["bytes"]
    assert OC.run_gpu(grown(OC.MAX_N + 1), ext) == _lib.PGORB_E_LIMIT
    z = np.zeros(64, f32)
    p = C.c_void_p(z.ctypes.data)
    L, h = ext._L, ext._h
    assert L.pgorb_optimize_sim3_batch_device(h, p, p, OC.MAX_N + 1, p, p, 1, p, p, p, None, 0, p, None, p, 10.0, 0, p, p, None, None, None, None, None,
                                              None) == _lib.PGORB_E_LIMIT
    assert L.pgorb_optimize_sim3_batch_device(h, p, p, 8, p, p, 1, p, p, p, None, 0, p, None, p, 0.0, 0, p, p, None, None, None, None, None,
                                              None) == _lib.PGORB_E_ARG


# ---------------------------------------------------------------- the chain of ComputeSim3 on a resident batch, steps 1-5
def test_chain_cases_meet_the_case_condition():
    for seed in OC.CHAIN_SEEDS:
        assert OC.condition(OC.chain_reference(seed)[-1]) == [], seed


@pytest.mark.gpu
def test_gpu_chain_of_compute_sim3_on_a_resident_batch(ext):
    """pgorb_search_by_bow_keyframes_batch_device -> pgorb_sim3_solver_batch_device -> pgorb_search_by_sim3_batch_device ->
    pgorb_optimize_sim3_batch_device -> pgorb_slots_from_assignment_batch_device -> pgorb_search_by_projection_sim3_batch_device on
    three key-frame pairs: d_matches12_out and d_found go from the solver to the optimiser, SearchBySim3's d_match12 is its
    d_new_matches12, its d_matches12_out (turned into table indices on the device) and d_scw_pose go to step 5, with no download
    in between; every stage is then compared with its reference.  The frames lie as KF1 of every pair, then KF2 of every pair, so
    step 5's key-frame index is the pair index and d_scw_pose needs no reordering."""
    import torch
    import loop_cases as LC
    import loop_reference as LR
    import sim3_cases as SC
    import pilotguru_amd as pg
    from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE, SIM3_DTYPE, SIM3_ESTIMATE_DTYPE
    ch = [OC.chain_reference(seed) for seed in OC.CHAIN_SEEDS]
    L, h = ext._L, ext._h
    B = len(ch)
    nf = 2 * B
    cap = max(max(len(x[0].slots1), len(x[0].slots2)) for x in ch) + 5
    kp = np.zeros((nf, cap), KEYPOINT_DTYPE)
    ds = np.full((nf, cap, 32), 0xFF, np.uint8)
    n, nfv = np.zeros(nf, np.int32), np.zeros(nf, np.int32)
    fn, ff, fs = np.zeros((nf, cap), np.uint32), np.zeros((nf, cap), np.uint32), np.zeros((nf, cap + 1), np.int32)
    v1, v2 = np.zeros((B, cap), np.uint8), np.zeros((B, cap), np.uint8)
    slots = np.full((nf, cap), -1, np.int32)
    poses = np.zeros(nf, KF_POSE_DTYPE)
    draws = np.zeros((B, 300, 3), np.uint32)
    allpts, off = [], []
    for x in ch:
        off.append(len(allpts))
        allpts += x[0].points
    qcap = max(int((x[0].slots2 >= 0).sum()) for x in ch) + 3
    Q, nq = np.full((B, qcap), 0x7FFF0000, np.int32), np.zeros(B, np.int32)
    for j, x in enumerate(ch):
        c, b, dr = x[0], x[1], x[2]
        for f, (k, d, P), sl, (_, _, v, fv), vm in ((j, c.kf1, c.slots1, b.k1, v1), (B + j, c.kf2, c.slots2, b.k2, v2)):
            m = len(k)
            n[f] = m; kp[f, :m] = k; ds[f, :m] = d; poses[f] = P; vm[j, :m] = v
            slots[f, :m] = np.where(sl >= 0, sl + off[j], -1)
            nfv[f] = len(fv[0]); fn[f, :len(fv[0])] = fv[0]; fs[f, :len(fv[1])] = fv[1]; ff[f, :m] = fv[2]
        draws[j] = dr
        q = c.slots2[c.slots2 >= 0] + off[j]                            # mvpLoopMapPoints: the loop key frame's points
        nq[j] = len(q); Q[j, :len(q)] = q
    pts, pd, pb, _, _ = LC.FC.table_arrays(allpts)
    keep = []

    def p(t):
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    Tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dk, dd, dn = Tt(kp.view(np.uint8).reshape(nf, cap, 28)), Tt(ds), Tt(n)
    f1, f2 = Tt(np.arange(0, B, dtype=np.int32)), Tt(np.arange(B, nf, dtype=np.int32))
    dpose, dslots = Tt(poses.view(np.uint8)), Tt(slots)
    dpts, dpd, dpb = Tt(pts.view(np.uint8)), Tt(pd), Tt(pb)
    gs = torch.zeros((nf, 3073), dtype=torch.int32, device="cuda")
    gi = torch.zeros((nf, cap), dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_frame_grid_batch_device(h, p(dk), p(dn), nf, cap, *LC.BOUNDS, p(gs), p(gi), s))
    I32 = lambda *sh: torch.full(sh, -9, dtype=torch.int32, device="cuda")  # noqa: E731
    m12, nm = I32(B, cap), I32(B)
    ext._check(L.pgorb_search_by_bow_keyframes_batch_device(h, p(dk), p(dd), p(dn), cap, p(Tt(fn.view(np.int32))), p(Tt(fs)), p(Tt(ff.view(np.int32))),
                                                            p(Tt(nfv)), p(f1), p(f2), B, p(Tt(v1)), p(Tt(v2)), LC.NNRATIO, 1, p(m12), p(nm), s))
    sol = pg.Sim3Solver.iterate_batch_device(ext, dk, dn, cap, f1, f2, dpose, dslots, m12, len(allpts), dpts, dpb, Tt(draws.view(np.int32)),
                                             0.99, 20, 300, 300)
    s12, nfound = I32(B, cap), I32(B)
    ext._check(L.pgorb_search_by_sim3_batch_device(h, p(dk), p(dd), p(dn), cap, p(gs), p(gi), p(f1), p(f2), B, p(dpose), *LC.BOUNDS, p(dslots),
                                                   len(allpts), p(dpts), p(dpd), p(dpb), p(sol["found_sim3"]), p(sol["already1"]), p(sol["already2"]),
                                                   SC.CHAIN_TH, p(s12), p(nfound), s))
    opt = pg.Optimizer.OptimizeSim3_batch_device(ext, dk, dn, cap, f1, f2, dpose, dslots, sol["matches12_out"], len(allpts), dpts, dpb, sol["found"],
                                                 10.0, False, s12)
    matched = torch.full((B, cap), -1, dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_slots_from_assignment_batch_device(h, p(opt["matches12_out"]), p(dslots[B:]), cap, p(matched), cap, B, s))
    asg, mout, n5 = I32(B, cap), I32(B, cap), I32(B)
    ext._check(L.pgorb_search_by_projection_sim3_batch_device(h, p(dk), p(dd), p(dn), cap, p(gs), p(gi), p(f1), B, p(opt["scw_pose"]), *LC.BOUNDS,
                                                              p(matched), len(allpts), p(dpts), p(dpd), p(dpb), qcap, p(Tt(nq)), p(Tt(Q)), OC.CHAIN_TH,
                                                              p(asg), p(mout), p(n5), s))
    torch.cuda.synchronize()                                             # the first download
    H = lambda t: t.cpu().numpy()  # noqa: E731
    found = np.frombuffer(H(sol["found"]).tobytes(), SIM3_ESTIMATE_DTYPE)
    best = np.frombuffer(H(sol["best"]).tobytes(), SIM3_ESTIMATE_DTYPE)
    sim3 = np.frombuffer(H(sol["found_sim3"]).tobytes(), SIM3_DTYPE)
    eo = np.frombuffer(H(opt["estimate"]).tobytes(), SIM3_ESTIMATE_DTYPE)
    sp = np.frombuffer(H(opt["scw_pose"]).tobytes(), KF_POSE_DTYPE)
    for j, (c, b, dr, rm12, sc, r, (n3, rs12), oc) in enumerate(ch):
        a, b2 = len(c.slots1), len(c.slots2)
        assert int(nm[j]) == int((rm12 >= 0).sum()) and np.array_equal(H(m12[j, :a]), rm12), "%s: SearchByBoW" % c.name
        got = SC.result_of(H(sol["ninliers"])[j], found[j], sim3[j], best[j], H(sol["inlier"][j, :a]), H(sol["matches12_out"][j, :a]),
                           H(sol["already1"][j, :a]), H(sol["already2"][j, :b2]), H(sol["info"][j]))
        assert SC.differences(sc, r, got, SC.spread(sc))[0] == [], "%s: Sim3Solver" % c.name
        kf1, kf2 = c.build()
        w3 = LR.search_by_sim3(kf1, kf2, sim3[j], list(got["already1"]), list(got["already2"]), c.th)
        assert int(nfound[j]) == w3[0] and np.array_equal(H(s12[j, :a]), np.array(w3[1], np.int32)), "%s: SearchBySim3" % c.name
        # step 4's reference reads what the device's steps 2 and 3 produced, which have just been compared
        oc4 = OC.chain_case(c, got["matches12_out"], H(s12[j, :a]), (found[j]["R12"], found[j]["t12"], found[j]["s12"]), "dev_" + oc.name)
        assert OC.condition(oc4) == [], oc4.name
        g4 = OC.result_of(H(opt["nin"])[j], eo[j], H(opt["matches12_out"][j, :a]), H(opt["chi2_12"][j, :a]), H(opt["chi2_21"][j, :a]), sp[j], H(opt["info"][j]))
        _check(oc4, OC.reference(oc4)["edges"][0], g4, "chained")
        assert g4["ret"] >= 20                                          # nInliers >= 20: ComputeSim3 goes on to step 5
        # step 5's reference reads the device's Scw and matches
        mi = np.where(g4["matches12_out"] >= 0, c.slots2[np.maximum(g4["matches12_out"], 0)], -1)
        assert np.array_equal(H(matched[j, :a]), np.where(mi >= 0, mi + off[j], -1)), "%s: matched_in" % c.name
        kf = LC.FC.make_kf(1, c.kf1[0], c.kf1[1], sp[j], LC.BOUNDS)
        mps = kf2.slots and {id(m): m for m in kf1.slots + kf2.slots if m is not None}
        by_id = {m.id: m for m in mps.values()}
        mlist = [by_id[int(i)] if i >= 0 else None for i in mi]
        n5r, a5 = LR.search_by_projection_sim3(kf, [by_id[int(q) - off[j]] for q in Q[j, :nq[j]]], mlist, OC.CHAIN_TH)
        assert int(n5[j]) == n5r and np.array_equal(H(asg[j, :a]), np.array(a5, np.int32)), "%s: SearchByProjection(Scw)" % c.name
