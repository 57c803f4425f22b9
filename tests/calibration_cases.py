"""Constructed recordings for fit_motion's velocity calibration: every timestamp is an integer placed so that the case meets its
edge by construction (tests/calibration_reference.py counts the edges in `hits`).  A Case is what the three library entry points
take: the GPS, gyroscope and accelerometer series, the window arguments, the points at which eval is compared, and -- for the tail
cases -- the arguments of fit_motion_velocities.

Exit codes of the solver.  1 (converged at the first evaluation), the iteration count and -2 are reached below.  -3 ("the step rose
above max_step", LineSearch.h:106-107) is unreachable from fit_motion: the test sits after a failed Armijo trial, and the step it
sees is either the first one, 1 / |grad f(0)|, or 1.0 (LBFGS.h:177), halved zero or more times (the backtracking search under
LBFGS_LINESEARCH_BACKTRACKING_ARMIJO never takes width = inc).  A first step above 1e20 needs |grad f(0)| < 1e-20, and then the
convergence test of LBFGS.h:93, gnorm <= 1e-5 * max(|0|, 1), has already returned 1.  A NaN gradient gives a NaN step, and
`step > max_step` is false for it.  So -3 is in no case and not in EDGES."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calibration_reference as CR  # noqa: E402

B = 1_000_000_000                  # a recording's clock origin, usec

EDGES = [
    # merge and intervals
    "merge_equal_ts", "merge_late_start", "merge_early_end", "sample_on_fix", "split_event", "two_fixes_between_samples",
    "fix_before_first_event", "fix_after_last_event", "window_one_fix", "window_no_steps", "last_window_short", "shift_eq_batch", "shift_1",
    # chunking (the kernel's concern; the cases carry it)
    "interval_steps_1", "interval_steps_63", "interval_steps_64", "interval_steps_65", "interval_steps_127", "interval_steps_128",
    "interval_steps_129", "interval_steps_256", "interval_steps_257", "window_steps_multiple_of_128", "window_all_one_step_intervals",
    "long_interval_20_chunks", "window_many_fixes",
    # numeric
    "travel_zero", "rate_zero", "nan_loss", "nan_search_succeeds",
    # solver exits and paths
    "exit_first_eval", "converged_k_gt_1", "max_iter_1", "max_iter_wraps", "search_0_halvings", "search_many_halvings", "search_20_fail",
    "exit_-2",
    # the tail of fit_motion_velocities
    "event_in_several_windows", "event_in_no_window", "split_event_in_trajectory", "window_below_rotation_gate", "velocity_above_gate",
    "velocity_below_gate", "velocity_on_gate", "negative_exit_refused",
]


class Case:
    def __init__(self, name, gps, rot, acc, batch, shift, iters, edges=(), points=None, tail=None, big=False):
        self.name = name
        self.edges = tuple(edges)      # the edges the case is built to reach
        self.gps = (np.asarray(gps[0], np.float64), np.asarray(gps[1], np.int64))
        self.rot = (np.asarray(rot[0], np.float64).reshape(-1, 3), np.asarray(rot[1], np.int64))
        self.acc = (np.asarray(acc[0], np.float64).reshape(-1, 3), np.asarray(acc[1], np.int64))
        self.batch, self.shift, self.iters = batch, shift, iters
        r = np.random.RandomState(len(name))
        self.points = np.asarray(points if points is not None else
                                 [np.zeros(9), r.normal(0, 1, 9), np.concatenate([[0.1, -0.2, -9.8], r.normal(0, 0.05, 6)])], np.float64)
        self.tail = tail               # None | dict(axis, sigma, min_velocity, min_rotation)
        self.big = big                 # thousands of steps: left out of the mutant sweep

    def series(self):
        return self.gps, self.rot, self.acc


def _values(seed, n_gps, n_rot, n_acc, rot_sigma=0.3):
    r = np.random.RandomState(seed)
    return np.abs(r.normal(10, 3, n_gps)), r.normal(0, rot_sigma, (n_rot, 3)), r.normal(0, 1.0, (n_acc, 3)) + [0.3, -0.2, 9.8]


def _make(name, seed, gps_t, rot_t, acc_t, batch=None, shift=None, iters=4, **kw):
    v, rot, acc = _values(seed, len(gps_t), len(rot_t), len(acc_t))
    batch = batch if batch is not None else len(gps_t)
    return Case(name, (v, gps_t), (rot, rot_t), (acc, acc_t), batch, shift if shift is not None else batch, iters, **kw)


def _grid(n, dt=1000, t0=B):
    return [t0 + dt * i for i in range(n)]


def _fixes_for_counts(imu_t, counts, first=1):
    """fixes on samples so that interval r holds exactly counts[r-1] steps: fix 0 on sample `first` (> 0: the step that ends at
    sample 0 does not exist), fix r on sample first + counts[0] + ... + counts[r-1]"""
    idx, out = first, [imu_t[first]]
    for c in counts:
        idx += c
        out.append(imu_t[idx])
    return out


def merge_header():
    """The two series of align_time_series.hpp:17-26 (x 100 ms): rotations at 1 3 4 6 7, accelerations at 2 3 4 5 6 -> merged events at
    2 3 4 5 6.  Equal timestamps at 3, 4 and 6; the rotations start earlier (their first() is idx - 1); the accelerations end earlier.
    Fixes: 1.5 and 1.8 before the first event, 3.0 on a sample, 4.5 / 4.6 / 4.7 between the samples at 4 and 5 (the event at 5 is
    split over four intervals, two of them from fix to fix), 6.5 and 7.0 after the last event."""
    u = 100_000
    rot_t = [B + k * u for k in (1, 3, 4, 6, 7)]
    acc_t = [B + k * u for k in (2, 3, 4, 5, 6)]
    gps_t = [B + int(k * u) for k in (1.5, 1.8, 3.0, 4.5, 4.6, 4.7, 6.5, 7.0)]
    return _make("merge_header", 1, gps_t, rot_t, acc_t, iters=5,
                 edges=("merge_equal_ts", "merge_late_start", "merge_early_end", "sample_on_fix", "split_event", "two_fixes_between_samples",
                        "fix_before_first_event", "fix_after_last_event"))


def ride(name, seed, n_gps, batch, shift, iters, hz=20, fix_every=0.5, quiet_until=0, **kw):
    """Two IMU clocks of their own (the gyroscope 3 ms late, one sample in seven of the accelerometer dropped), fixes every
    `fix_every` s starting 0.26 s into the recording (off the IMU grid).  The device yaws at 0.8 rad/s, or not at all before
    sample `quiet_until`."""
    n = int((n_gps * fix_every + 1.0) * hz)
    dt = 1_000_000 // hz
    rot_t = [B + 3000 + dt * i for i in range(n)]
    acc_t = [B + dt * i for i in range(n) if i % 7 != 3]
    gps_t = [B + 260_000 + int(fix_every * 1_000_000) * i for i in range(n_gps)]
    c = _make(name, seed, gps_t, rot_t, acc_t, batch, shift, iters, **kw)
    c.rot[0][:] *= 0.05
    c.rot[0][:, 2] += 0.8
    c.rot[0][:quiet_until] = 0.0
    return c


def no_steps():
    """Six fixes, the first three before the recording starts: the window of fixes 0-2 has fixes and no step (0/0)."""
    imu = _grid(40, 10_000)
    gps_t = [B - 300_000, B - 200_000, B - 100_000, B + 55_000, B + 155_000, B + 255_000]
    return _make("no_steps", 3, gps_t, imu, imu, batch=3, shift=3, iters=3, edges=("window_no_steps", "fix_before_first_event"))


def chunk_lengths():
    """One window whose intervals hold exactly 1, 63, 64, 65, 127, 128, 129, 256 and 257 steps (fixes on samples)."""
    imu = _grid(1100)
    return _make("chunk_lengths", 4, _fixes_for_counts(imu, CR.STEP_COUNTS), imu, imu, iters=2, big=True,
                 edges=tuple("interval_steps_%d" % n for n in CR.STEP_COUNTS))


def steps_256():
    """100 + 28 + 128 steps: the window's step count is a multiple of 128, its interval boundaries are not."""
    imu = _grid(260)
    return _make("steps_256", 5, _fixes_for_counts(imu, (100, 28, 128)), imu, imu, iters=3, edges=("window_steps_multiple_of_128",))


def one_step_intervals(n_fix, name, **kw):
    """Every fix on a sample, one sample apart: every interval has one step, every chunk is the last of its interval."""
    imu = _grid(n_fix + 3, 20_000)
    return _make(name, 6, _fixes_for_counts(imu, (1,) * (n_fix - 1)), imu, imu, **kw)


def long_interval():
    """One interval of 2600 steps (21 chunks) between one-step intervals: the pipeline's lag is large against the chunk count."""
    imu = _grid(2610)
    return _make("long_interval", 7, _fixes_for_counts(imu, (1, 1, 2600, 1, 1)), imu, imu, iters=2, big=True, edges=("long_interval_20_chunks",))


def still():
    """Zero accelerations, zero rotation rates, x = 0: integrated_travel is exactly zero (the 1e-5 carries the division), the rate is
    zero (1e-30 carries that one), the gradient is exactly zero and the solver returns 1 at the first evaluation."""
    imu = _grid(30, 10_000)
    c = _make("still", 8, [imu[2], imu[9], imu[20]], imu, imu, iters=5, edges=("travel_zero", "rate_zero", "exit_first_eval"))
    c.rot[0][:] = 0.0
    c.acc[0][:] = 0.0
    return c


def tiny_gradient():
    """A gradient of about 1e-7 at x = 0: not zero, and below epsilon * max(|x|, 1) = 1e-5 -- converged at the first evaluation
    only because of the max."""
    imu = _grid(30, 10_000)
    c = _make("tiny_gradient", 9, [imu[2], imu[9], imu[20]], imu, imu, iters=5, edges=("exit_first_eval",))
    c.acc[0][:] *= 1e-9
    c.gps[0][:] = 1e-3
    return c


def nan_sample():
    """One accelerometer sample is NaN: the loss is NaN from the first evaluation on, `fx > ...` is false, every search "succeeds" at
    its first trial and the solver runs to max_iterations."""
    c = ride("nan_sample", 10, 4, 4, 4, 3, edges=("nan_loss", "nan_search_succeeds"))
    c.acc[0][11, 1] = np.nan
    return c


def converging():
    """Two fixes 80 ms apart around four samples, speeds of ~1 m/s: the fit reaches gnorm <= 1e-5 * max(|x|, 1) after a few iterations."""
    imu = _grid(12, 20_000)
    c = _make("converging", 11, [imu[2] + 5_000, imu[6] + 5_000], imu, imu, iters=60, edges=("converged_k_gt_1", "search_0_halvings"))
    c.gps[0][:] = [1.0, 1.2]
    return c


def overshoot():
    """Steps of 10^5 s: a unit change of a bias moves the travel by ~10^10 m, so the first step (unit length by construction,
    1 / |grad|) overshoots the valley and the search halves it several times before Armijo holds."""
    imu = _grid(8, 100_000_000_000)
    c = _make("overshoot", 12, [imu[1], imu[3], imu[6]], imu, imu, iters=2, edges=("search_many_halvings",))
    c.acc[0][:] *= 1e-6
    c.rot[0][:] *= 1e-12
    return c


def narrow_valley():
    """GPS speeds of zero, accelerations of ~1e-8 m/s^2, steps of 100 s: the loss is |travel0 + A x|^2 / T, a quadratic whose minimum
    along -grad lies at a step of about 2 |travel0| / |A| ~ 1e-8 of the first, unit-length one.  2^-19 of that step still overshoots,
    so all 20 trials fail.  The reference's `throw` for that sits inside the loop behind `iter >= max_linesearch` and cannot fire:
    the solver goes on from the twentieth trial point."""
    imu = _grid(8, 100_000_000)
    c = _make("narrow_valley", 12, [imu[1], imu[3], imu[6]], imu, imu, iters=2, edges=("search_20_fail",))
    c.acc[0][:] *= 1e-9
    c.rot[0][:] *= 1e-12
    c.gps[0][:] = 0.0
    return c


def huge_gradient(tail=None, name="huge_gradient"):
    """One step of 10^12 s against a GPS speed of 1 m/s.  |grad f(0)| ~ 10^24, so the first step is ~10^-24 < min_step; the trial
    point has unit length, its travel is ~10^23 m against a reference distance of 10^12 m, the Armijo test fails and the reference
    throws "the line search step became smaller than the minimum value allowed": exit -2."""
    imu = _grid(4, 10 ** 18)
    c = _make(name, 13, [imu[1], imu[2]], imu, imu, iters=5, tail=tail, edges=("exit_-2",) + (("negative_exit_refused",) if tail else ()))
    c.gps[0][:] = 1.0
    c.acc[0][:] = [1e-13, 0.0, 0.0]
    c.rot[0][:] = 0.0
    return c


def flat_plateau():
    """GPS speeds of 1e17 m/s: |travel| - reference_distance == -reference_distance for every x the solver visits, so the loss is
    the same double at every trial point and step * dg_test is below half an ulp of it: fx == fx_init + step * dg_test exactly.
    Armijo's `>` accepts the first trial."""
    imu = _grid(12, 100_000)
    c = _make("flat_plateau", 14, [imu[1], imu[5], imu[9]], imu, imu, iters=1, edges=("search_0_halvings",))
    c.gps[0][:] = 1e17
    return c


AXIS = np.array([0.1, -0.2, 1.0]) / np.linalg.norm([0.1, -0.2, 1.0])


def tail_ride():
    """Four windows of 5 fixes, shift 3, over 11 fixes.  No rotation during the first two seconds, so the first window stays below the
    rotation gate; events before the first fix are reached by no window, events under two windows by several.  The velocity gate is
    the reference's own speed at one event of the last window, so one sample sits exactly on it, others on both sides."""
    c = ride("tail_ride", 15, 11, 5, 3, 6, quiet_until=48, tail=dict(axis=AXIS, sigma=0.01, min_velocity=0.0, min_rotation=0.3),
             edges=("event_in_several_windows", "event_in_no_window", "split_event_in_trajectory", "window_below_rotation_gate",
                    "velocity_above_gate", "velocity_below_gate", "velocity_on_gate"))
    fits = CR.fit_windows(*c.series(), c.batch, c.shift, c.iters, with_calibrators=True)
    x, _, _, cal = fits[-2]
    traj = cal.integrate_trajectory(x[0:3], x[3:6], x[6:9])
    speeds = sorted(CR.norm3(traj[e][1]) for e in traj)
    c.tail["min_velocity"] = speeds[len(speeds) // 2]
    return c


def edge_cases():
    return [
        merge_header(), ride("windows", 2, 11, 4, 2, 9, edges=("window_one_fix", "last_window_short", "max_iter_wraps")),
        ride("shift_1", 16, 5, 3, 1, 4, edges=("shift_1",)), ride("shift_eq_batch", 17, 7, 3, 3, 4, edges=("shift_eq_batch",)), no_steps(),
        chunk_lengths(), steps_256(),
        one_step_intervals(9, "one_step_intervals", iters=4, edges=("window_all_one_step_intervals", "interval_steps_1")),
        one_step_intervals(400, "many_fixes", iters=2, big=True, edges=("window_many_fixes", "window_all_one_step_intervals")), long_interval(),
        still(), tiny_gradient(), nan_sample(), converging(), ride("one_iteration", 18, 4, 4, 4, 1, edges=("max_iter_1",)), overshoot(),
        narrow_valley(), huge_gradient(), flat_plateau(),
        tail_ride(), huge_gradient(dict(axis=AXIS, sigma=0.01, min_velocity=1.0, min_rotation=0.1), "tail_negative_exit"),
    ]


def refusals():
    """name -> (gps, rot, acc) that the reference CHECK-fails (or where it reads front() of an empty vector)"""
    c = ride("r", 19, 4, 4, 4, 3)
    g, r, a = c.series()
    swap = lambda s: (s[0], np.concatenate([s[1][:1], s[1][2:3], s[1][1:2], s[1][3:]]))
    twice = lambda s: (s[0], np.concatenate([s[1][:2], s[1][1:-1]]))
    return {
        "gps_unordered": (swap(g), r, a), "gps_repeated": (twice(g), r, a), "rot_unordered": (g, swap(r), a), "acc_repeated": (g, r, twice(a)),
        "disjoint": (g, (r[0], r[1] + 10 ** 9), a), "rot_empty": (g, (r[0][:0], r[1][:0]), a),
    }


def run_reference(case, rules=None, hits=None, fit=True):
    """Everything the library reports for a case, from the reference: dict(events, times, eval=[(loss, grad)], fit=[(x, residual,
    iterations)], tail=(time_usec, speed, forward_axis) | CR.E_LIMIT | None), or the string "refused"."""
    rules = rules if rules is not None else CR.REFERENCE
    gps, rot, acc = case.series()
    try:
        cal = CR.Calibrator(gps, rot, acc, rules, hits)
        out = dict(events=cal.imu.events, times=cal.imu.times, intervals=cal.intervals, eval=[cal.eval(list(map(float, x))) for x in case.points])
        if fit:
            out["fit"] = CR.fit_windows(gps, rot, acc, case.batch, case.shift, case.iters, rules, hits)
            out["tail"] = None
            if case.tail is not None:
                t = case.tail
                out["tail"] = CR.fit_motion_velocities(gps, rot, acc, t["axis"], case.batch, case.shift, case.iters, t["sigma"],
                                                       t["min_velocity"], t["min_rotation"], rules, hits)
        return out
    except CR.Refused:
        return "refused"


def bits(a):
    """bit patterns, all NaNs folded to one"""
    a = np.ascontiguousarray(a, np.float64).copy()
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def same(a, b):
    """two run_reference results agree: integers as integers, doubles as bit patterns"""
    if isinstance(a, str) or isinstance(b, str):
        return a == b
    if a["events"] != b["events"] or a["intervals"] != b["intervals"]:
        return False
    flat = lambda r: (np.concatenate([[fx] + list(g) for fx, g in r["eval"]]),
                      np.concatenate([list(x) + [fx] for x, fx, _ in r.get("fit", [])] or [[]]), [it for _, _, it in r.get("fit", [])])
    (ea, fa, ia), (eb, fb, ib) = flat(a), flat(b)
    if ia != ib or not np.array_equal(bits(ea), bits(eb)) or not np.array_equal(bits(fa), bits(fb)):
        return False
    ta, tb = a.get("tail"), b.get("tail")
    if ta is None or tb is None or isinstance(ta, str) or isinstance(tb, str):
        return ta == tb
    return ta[0] == tb[0] and np.array_equal(bits(ta[1]), bits(tb[1])) and np.array_equal(bits(ta[2]), bits(tb[2]))


def edge_report(cases=None):
    """edge -> the cases that reach it (for the pull request's table)"""
    out = collections.OrderedDict((e, []) for e in EDGES)
    for c in cases or edge_cases():
        h = collections.Counter()
        run_reference(c, hits=h)
        for e in EDGES:
            if h[e]:
                out[e].append(c.name)
    return out
