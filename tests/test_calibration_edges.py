"""fit_motion's velocity calibration pinned to an independent reference on constructed edge cases.

tests/test_calibration.py compares pilotguru_amd/csrc/calib.hip with oracle/calib_oracle.c, two restatements from one reading of the
reference.  Here both are compared with a third, tests/calibration_reference.py -- sequential Python floats, written from the
reference's sources, importing neither -- on the recordings of tests/calibration_cases.py, whose integer timestamps meet the merge,
interval, chunk, numeric and solver edges by construction.  Every comparison but the scipy anchor is exact: integers as integers,
doubles as bit patterns with all NaNs folded to one."""
import collections
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calibration_cases as CC  # noqa: E402
import calibration_reference as CR  # noqa: E402
from test_calibration import imu_ride, irregular_series  # noqa: E402

bits = CC.bits


@pytest.fixture(scope="module")
def cases():
    return CC.edge_cases()


@pytest.fixture(scope="module")
def wanted(cases):
    """the reference's result of every case, computed once"""
    return {c.name: CC.run_reference(c) for c in cases}


# ---------------------------------------------------------------- CPU: the cases and the reference

def test_reference_stands_alone():
    """The reference imports neither side it is compared with, and computes in plain Python floats."""
    import ast
    tree = ast.parse(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "calibration_reference.py")).read())
    mods = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    mods |= {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert mods == {"math", "dataclasses"}, mods


def test_cases_reach_every_edge(cases):
    reached = collections.Counter()
    for c in cases:
        hits = collections.Counter()
        CC.run_reference(c, hits=hits)
        missing = [e for e in c.edges if not hits[e]]
        assert not missing, (c.name, missing, dict(hits))              # a case reaches what it was built for ...
        reached.update(e for e in c.edges)
        assert set(c.edges) <= set(CC.EDGES), c.name
    missing = [e for e in CC.EDGES if not reached[e]]
    assert not missing, missing                                        # ... and every edge has a case built for it
    assert "exit_-3" not in CC.EDGES                                   # shown unreachable in tests/calibration_cases.py


def test_every_rule_mutant_is_caught(cases, wanted):
    small = [c for c in cases if not c.big]
    for name, rules in CR.MUTANTS.items():
        assert any(not CC.same(wanted[c.name], CC.run_reference(c, rules)) for c in small), name


def test_sample_on_fix_comparison_is_equivalent():
    """The one rule variant of the issue's list that is not in MUTANTS: `<=` -> `<` for a sample exactly on a fix gives the same
    intervals on every input (the argument is in tests/calibration_reference.py).  Enumerated here: every pair of increasing series
    over a grid of 7 instants with up to 4 fixes and up to 4 samples."""
    grid = range(7)
    n = 0
    for nf, ns in itertools.product(range(1, 5), range(1, 5)):
        for fixes in itertools.combinations(grid, nf):
            for samples in itertools.combinations(grid, ns):
                a = CR.make_interpolation_intervals(list(fixes), list(samples))
                b = CR.make_interpolation_intervals(list(fixes), list(samples), le_as_lt=True)
                assert a == b, (fixes, samples)
                n += set(fixes) & set(samples) != set()
    assert n > 5000                                                    # most of them have a sample on a fix


def test_merge_example_of_the_header():
    """include/interpolation/align_time_series.hpp:17-26, worked by hand.  Start = max(1, 2) = 2: the first series has no sample at
    2, so it begins one before its first sample >= 2, at index 0; the second at index 0.  Next times (3, 3): both advance.  (4, 4):
    both.  (6, 5): the second only.  (6, 6): both.  Then the second series has no next sample: the end."""
    assert CR.merge_time_series([[1, 3, 4, 6, 7], [2, 3, 4, 5, 6]]) == [(0, 0), (1, 1), (2, 2), (2, 3), (3, 4)]
    m = CR.Merged([1, 3, 4, 6, 7], [2, 3, 4, 5, 6])
    assert m.times == [2, 3, 4, 5, 6]
    # and the intervals of fixes at 3 (on a sample) and 5.5 (inside the event that ends at 6) against those times, by hand:
    # (2, 3] belongs to fix 0 and is dropped (reference_idx > 0); (3, 4], (4, 5] whole; (5, 5.5] is the first part of event 4
    assert CR.make_interpolation_intervals([30, 55], [20, 30, 40, 50, 60]) == [[], [(1, 2, 30, 40), (1, 3, 40, 50), (1, 4, 50, 55)]]


def _oracle_result(oracle, c):
    """the oracle on a case, in run_reference's form"""
    try:
        out = dict(eval=[oracle.calibrator_eval(*c.gps, *c.rot, *c.acc, x) for x in c.points])
        x, res, it = oracle.fit_windows(*c.gps, *c.rot, *c.acc, c.batch, c.shift, c.iters)
    except ValueError:
        return "refused"
    out["fit"] = (x, res, it)
    out["tail"] = None
    if c.tail is not None:
        t = c.tail
        try:
            out["tail"] = oracle.fit_motion_velocities(*c.gps, *c.rot, *c.acc, t["axis"], c.batch, c.shift, c.iters, t["sigma"],
                                                       t["min_velocity"], t["min_rotation"])
        except ValueError as e:
            assert "-2" in str(e), e                                   # porc_fit_motion_velocities: a window's line search threw
            out["tail"] = CR.E_LIMIT
    return out


def _assert_equal(name, want, got):
    """want: run_reference's dict; got: dict(eval=[(fx, grad)], fit=(x[nw][9], res[nw], it[nw]), tail)"""
    assert not isinstance(want, str) and not isinstance(got, str), (name, want if isinstance(want, str) else "", got if isinstance(got, str) else "")
    for i, ((fx, g), (gfx, gg)) in enumerate(zip(want["eval"], got["eval"])):
        assert np.array_equal(bits([fx] + list(g)), bits([gfx] + list(gg))), (name, "eval", i, fx, gfx, g, list(gg))
    if "fit" in got and "fit" in want:
        x, res, it = got["fit"]
        assert [w[2] for w in want["fit"]] == [int(v) for v in it], (name, "iterations", [w[2] for w in want["fit"]], list(it))
        assert np.array_equal(bits([w[0] for w in want["fit"]]), bits(x)), (name, "x")
        assert np.array_equal(bits([w[1] for w in want["fit"]]), bits(res)), (name, "residual")
    if "tail" in got and want.get("tail") is not None:
        wt, gt = want["tail"], got["tail"]
        if isinstance(wt, str) or isinstance(gt, str):
            assert wt == gt, (name, "tail", wt if isinstance(wt, str) else "values", gt if isinstance(gt, str) else "values")
        else:
            assert list(wt[0]) == [int(t) for t in gt[0]], (name, "tail times")
            assert np.array_equal(bits(wt[1]), bits(gt[1])) and np.array_equal(bits(wt[2]), bits(gt[2])), (name, "tail values")


def test_reference_equals_oracle_on_constructed_cases(oracle, cases, wanted):
    for c in cases:
        _assert_equal(c.name, wanted[c.name], _oracle_result(oracle, c))
    exits = collections.Counter(it for c in cases for _, _, it in wanted[c.name]["fit"])
    assert exits[-2] and exits[1] and not exits[-3]                   # the codes compared above include the throw and the early return
    for name, (gps, rot, acc) in CC.refusals().items():               # what the reference CHECK-fails, both reject
        c = CC.Case(name, gps, rot, acc, 3, 3, 2)
        assert CC.run_reference(c) == "refused", name
        assert _oracle_result(oracle, c) == "refused", name
    for bad in ((3, 4, 2), (0, 0, 2), (3, 0, 2), (3, 3, 0)):          # fit_motion.cc:307-310 on the fit's arguments
        with pytest.raises(CR.Refused):
            CR.check_flags(*bad)
    with pytest.raises(CR.Refused):                                   # :311
        CR.check_flags(3, 3, 2, 0.0)


def _random_cases():
    """A few of test_calibration.py's random inputs, small enough for the Python solver."""
    out = []
    for seed in (21, 22):
        gps, rot, acc = imu_ride(seed, n_gps=9, imu_hz=25.0)
        out.append(CC.Case("imu_ride_%d" % seed, gps, rot, acc, 5, 2, 7, tail=dict(axis=CC.AXIS, sigma=0.01, min_velocity=5.0, min_rotation=0.05)))
    for seed in (1, 7, 14):                                            # the three smallest of the first twenty
        gps, rot, acc = irregular_series(np.random.default_rng(100 + seed))
        out.append(CC.Case("irregular_%d" % seed, gps, rot, acc, 6, 3, 5, tail=dict(axis=CC.AXIS, sigma=0.01, min_velocity=3.0, min_rotation=0.1)))
    return out


def test_reference_equals_oracle_on_random_series(oracle):
    for c in _random_cases():
        _assert_equal(c.name, CC.run_reference(c), _oracle_result(oracle, c))


def test_rotation_composition_against_scipy():
    """The anchor that leans on neither restatement: RotationMotionToQuaternion composed over 48 steps (rates ~0.8 rad/s, 5-400 ms)
    against scipy's Rotation.from_rotvec products.  Two double evaluations of the same rotation, compared up to sign."""
    from scipy.spatial.transform import Rotation
    r = np.random.RandomState(0)
    rates, dts = r.normal(0, 0.8, (48, 3)), r.uniform(0.005, 0.4, 48)
    q, want, worst = (1.0, 0.0, 0.0, 0.0), Rotation.identity(), 0.0
    for w, dt in zip(rates, dts):
        q = CR.quat_mul(q, CR.rotation_motion_to_quaternion(float(w[0]), float(w[1]), float(w[2]), float(dt)))
        want = want * Rotation.from_rotvec(w * dt)
        x, y, z, s = want.as_quat()
        d = min(max(abs(a - b) for a, b in zip(q, (s, x, y, z))), max(abs(a + b) for a, b in zip(q, (s, x, y, z))))
        worst = max(worst, d)
    print("largest quaternion difference: %.3g" % worst)
    assert worst <= 16 * 7.78e-16                                      # measured 7.77e-16 on the CPU; 16x for libm and ordering


# ---------------------------------------------------------------- GPU: calib.hip == the reference

@pytest.fixture(scope="module")
def ctx():
    import pilotguru_amd as pg
    return pg.ORBextractor(500, 1.2, 4, 20, 7, max_width=320, max_height=240, max_batch=1)


def _gpu_eval(ctx, c, points):
    from pilotguru_amd.calibration import AccelerometerCalibrator
    fx, g = AccelerometerCalibrator(ctx, c.gps, c.rot, c.acc)(points)
    return list(zip(np.atleast_1d(fx), np.atleast_2d(g)))


@pytest.mark.gpu
def test_gpu_calibrator_eval_equals_reference(ctx, cases, wanted):
    for c in cases:
        _assert_equal(c.name, wanted[c.name], dict(eval=_gpu_eval(ctx, c, c.points)))
    c = next(c for c in cases if c.name == "steps_256")              # more points than one wave has lanes, in one call
    xs = np.concatenate([c.points, np.random.RandomState(3).normal(0, 1, (67, 9))])
    cal = CR.Calibrator(*c.series())
    _assert_equal(c.name, dict(eval=[cal.eval(list(map(float, x))) for x in xs]), dict(eval=_gpu_eval(ctx, c, xs)))


@pytest.mark.gpu
def test_gpu_window_fits_equal_reference(ctx, cases, wanted):
    from pilotguru_amd.calibration import FitVelocityWindows
    exits = collections.Counter()
    for c in cases:
        x, res, it = FitVelocityWindows(ctx, c.gps, c.rot, c.acc, c.batch, c.shift, c.iters)
        _assert_equal(c.name, wanted[c.name], dict(eval=[], fit=(x, res, it)))
        exits.update(int(v) for v in it)
        if c.name in ("no_steps", "nan_sample"):
            assert np.isnan(res).any(), c.name                         # the NaN windows are among what was compared
    assert exits[-2] and exits[1]


@pytest.mark.gpu
def test_gpu_fit_motion_velocities_equal_reference(ctx, cases, wanted):
    from pilotguru_amd import _lib
    from pilotguru_amd.calibration import ComputeForwardVelocitiesFromImu
    seen = set()
    for c in list(cases) + _random_cases():
        if c.tail is None:
            continue
        want = wanted[c.name] if c.name in wanted else CC.run_reference(c)
        t = c.tail
        try:
            got = ComputeForwardVelocitiesFromImu(ctx, c.gps, c.rot, c.acc, t["axis"], c.batch, c.shift, c.iters, t["sigma"], t["min_velocity"],
                                                  t["min_rotation"])
        except _lib.PgorbError as e:
            assert e.code == _lib.PGORB_E_LIMIT and "line search" in str(e), e
            got = CR.E_LIMIT
        seen.add(got if isinstance(got, str) else "values")
        _assert_equal(c.name, want, dict(eval=[], tail=got))
    assert seen == {"values", CR.E_LIMIT}


@pytest.mark.gpu
def test_gpu_refuses_what_the_reference_checks(ctx):
    from pilotguru_amd import _lib
    from pilotguru_amd.calibration import AccelerometerCalibrator, FitVelocityWindows
    for name, (gps, rot, acc) in CC.refusals().items():
        with pytest.raises(_lib.PgorbError) as e:
            FitVelocityWindows(ctx, gps, rot, acc, 3, 3, 2)
        assert e.value.code == _lib.PGORB_E_ARG, name
        with pytest.raises(_lib.PgorbError):
            AccelerometerCalibrator(ctx, gps, rot, acc)(np.zeros(9))
    gps, rot, acc = CC.ride("r", 19, 4, 4, 4, 3).series()
    for batch, shift, iters in ((3, 4, 2), (0, 0, 2), (3, 0, 2), (3, 3, 0)):
        with pytest.raises(_lib.PgorbError) as e:
            FitVelocityWindows(ctx, gps, rot, acc, batch, shift, iters)
        assert e.value.code == _lib.PGORB_E_ARG, (batch, shift, iters)


def _many_fix_case(n_fix):
    """n_fix fixes against six samples: steps in the first eight intervals, then fixes without steps after the end of the recording"""
    imu = CC._grid(6, 10_000)
    gps_t = [imu[1] + 5_000 * i for i in range(n_fix)]
    return CC._make("fixes_%d" % n_fix, 30, gps_t, imu, imu, iters=2)


@pytest.mark.gpu
def test_gpu_window_size_limit(ctx):
    """The workgroup keeps two 3-vectors per fix of its window in LDS, so run_windows refuses a locations_batch_size that does not
    fit -- before the launch.  The border is found from the library's return codes: the largest size it accepts gives the reference's
    eval and fit, the next one PGORB_E_LIMIT with a message."""
    from pilotguru_amd import _lib
    from pilotguru_amd.calibration import FitVelocityWindows

    def accepted(n):
        c = _many_fix_case(n)
        try:
            return _gpu_eval(ctx, c, c.points[:1])
        except _lib.PgorbError as e:
            assert e.code == _lib.PGORB_E_LIMIT and "locations_batch_size" in str(e), e
            return None

    lo, hi = 64, 1 << 16
    assert accepted(lo) is not None and accepted(hi) is None
    while hi - lo > 1:                                                 # the LDS need grows with the number of fixes: one border
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if accepted(mid) is not None else (lo, mid)
    print("largest accepted locations_batch_size: %d" % lo)
    assert lo >= 400                                                   # fit_motion's default is 40; the many_fixes case uses 400
    c = _many_fix_case(lo)
    want = CC.run_reference(c)
    _assert_equal(c.name, want, dict(eval=_gpu_eval(ctx, c, c.points)))
    _assert_equal(c.name, want, dict(eval=[], fit=FitVelocityWindows(ctx, c.gps, c.rot, c.acc, lo, lo, c.iters)))
    c = _many_fix_case(hi)
    with pytest.raises(_lib.PgorbError) as e:
        FitVelocityWindows(ctx, c.gps, c.rot, c.acc, hi, hi, c.iters)
    assert e.value.code == _lib.PGORB_E_LIMIT and str(e.value)
