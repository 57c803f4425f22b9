"""A plain, sequential restatement in Python floats of what fit_motion does for velocities: the merge of the two IMU clocks, the
interpolation intervals of a window of GPS fixes, AccelerometerCalibrator::eval, LBFGSpp's minimize with the backtracking/Armijo
search, IntegrateTrajectory and the tail of ComputeAndSaveForwardVelocitiesFromImu.  It is written from the reference's own text
(file:line at each rule, paths relative to the reference project); it imports neither oracle/ nor pilotguru_amd and was not
derived from oracle/calib_oracle.c or pilotguru_amd/csrc/calib.hip.

Python floats are IEEE doubles, one rounding per operation, no contraction; math.sin / cos / erf / acos are the host libm.  Where
Eigen fixes an evaluation order the helper says which (Eigen 3.3~beta1, the libeigen3-dev the reference's Dockerfile installs,
built for SSE2; an -march=native build widens the packets and may contract, so the reference's own doubles depend on its build
machine -- the order below is the baseline x86-64 one):
  dot3 / norm3      Eigen/src/Core/Redux.h, redux_novec_unroller<Func, Derived, 0, 3>: the range is split in halves, length/2 first:
                    t0 + (t1 + t2).  A fixed 3-vector is not vectorised.  Rows of a 3x3 * 3x1 product are the same redux
                    (Eigen/src/Core/ProductEvaluators.h, the lazy coefficient-based product: lhs.row(i).cwiseProduct(rhs).sum()).
  dot9 / norm9      Redux.h, redux_impl<Func, Derived, LinearVectorizedTraversal, NoUnrolling> with 2-double packets on a 9-vector:
                    p0 = (t0,t1), p1 = (t2,t3); p0 += (t4,t5), p1 += (t6,t7); p0 += p1; predux = lane0 + lane1; then the scalar
                    tail + t8.
  transform_vector  Eigen/src/Geometry/Quaternion.h, QuaternionBase::_transformVector: uv = vec x v; uv += uv;
                    (v + w * uv) + vec x uv.
  rotation_matrix   Quaternion.h, QuaternionBase::toRotationMatrix: tx = 2x, ty, tz; twx = tx*w ...; the nine coefficients from them.
  quat_mul          Quaternion.h, the generic quat_product: four terms per coefficient, left to right.

`rules` (a Rules) switches one rule at a time; `hits` (a collections.Counter or None) counts the edges reached.  Series are
(values, time_usec) pairs: GPS speed [n], gyroscope rates [n][3], accelerations [n][3]; times are Python ints."""
import math
from dataclasses import dataclass

NAN = float("nan")
LB_M, LB_FTOL, LB_TRIALS, LB_MIN_STEP, LB_MAX_STEP = 6, 1e-4, 20, 1e-20, 1e+20     # LBFGS/Param.h:164-173
EPSILON = 1e-5                                                                    # fit_motion.cc:168
E_LIMIT = "PGORB_E_LIMIT"
STEP_COUNTS = (1, 63, 64, 65, 127, 128, 129, 256, 257)


class Refused(Exception):
    """What the reference CHECK-fails (or cannot survive: front() of an empty vector)."""


@dataclass(frozen=True)
class Rules:
    split: str = "keep"            # the part of an event before a fix is its own interval (align_time_series.cc:185-190) | "drop"
    idx_guard: str = "keep"        # interpolation_idx > 0 (:173, :185) | "drop"
    equal_ts: str = "all"          # every series whose next time is the earliest advances (:100-105) | "first": one only
    first: str = "idx-1"           # a series that has no sample at start_time begins one earlier (:69-71) | "idx"
    total_time: str = "running"    # total_time_usec runs over the whole window (velocity.cc:65, :134) | "per_interval"
    twr: str = "running"           # total_time_weighted_rotation too (:64, :152) | "per_interval"
    travel: str = "after"          # travel += dt * the velocity AFTER the step (:111-112) | "before"
    travel_eps: str = "keep"       # / (norm + 1e-5) (:126-128) | "drop"
    armijo: str = "gt"             # fx > fx_init + step * dg_test fails the trial (LineSearch.h:73) | "ge"
    step_reset: str = "one"        # step = 1 after an iteration (LBFGS.h:177) | "keep"
    bound: str = "min"             # bound = min(m, k) (LBFGS.h:153) | "m"
    scale: str = "ys/yy"           # m_drt *= ys / yy (LBFGS.h:165) | "ys/ys"
    conv: str = "max"              # gnorm <= epsilon * max(xnorm, 1) (LBFGS.h:93, :119) | "plain": epsilon * xnorm
    split_winner: str = "later"    # the later part of a split event overwrites the earlier (velocity.cc:244-250) | "earlier"
    vel_gate: str = "ge"           # velocity.norm() >= min velocity (fit_motion.cc:234-235) | "gt"
    rot_gate: str = "window"       # the rotation gate is one decision per window (fit_motion.cc:225-232) | "sample"
    average: str = "hits"          # sum / the number of windows that reached the event (fit_motion.cc:265-268) | "windows"


REFERENCE = Rules()
MUTANTS = {
    "split=drop": Rules(split="drop"),
    "idx_guard=drop": Rules(idx_guard="drop"),
    "equal_ts=first": Rules(equal_ts="first"),
    "first=idx": Rules(first="idx"),
    "total_time=per_interval": Rules(total_time="per_interval"),
    "twr=per_interval": Rules(twr="per_interval"),
    "travel=before": Rules(travel="before"),
    "travel_eps=drop": Rules(travel_eps="drop"),
    "armijo=ge": Rules(armijo="ge"),
    "step_reset=keep": Rules(step_reset="keep"),
    "bound=m": Rules(bound="m"),
    "scale=ys/ys": Rules(scale="ys/ys"),
    "conv=plain": Rules(conv="plain"),
    "split_winner=earlier": Rules(split_winner="earlier"),
    "vel_gate=gt": Rules(vel_gate="gt"),
    "rot_gate=sample": Rules(rot_gate="sample"),
    "average=windows": Rules(average="windows"),
}
# Not in the table: "`<=` becomes `<` for an IMU sample exactly on a fix" (align_time_series.cc:170).  It is equivalent on every
# input.  With `<` the sample at index i stays unconsumed at fix r; the split rule (:185-190) then pushes {r, i, latest, fix}, which
# is the interval {r, i, latest, sample time} the loop would have pushed, under the same guards (i > 0, r > 0, and i < size holds
# because sample i exists; fix > latest holds because the samples increase).  At fix r+1 the loop meets sample i with
# interpolation_ts == latest_ts, pushes nothing and moves on: the same state as after `<=`.
# tests/test_calibration_edges.py::test_sample_on_fix_comparison_is_equivalent checks that by enumeration; `le_as_lt` below is
# only for that test.


def _hit(hits, name):
    if hits is not None:
        hits[name] += 1


def _div(a, b):
    """IEEE a / b (Python raises on a zero divisor)."""
    if b == 0.0:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _sqrt(a):
    return math.sqrt(a) if not a < 0.0 else NAN


def _sin(a):
    return math.sin(a) if math.isfinite(a) else NAN


def _cos(a):
    return math.cos(a) if math.isfinite(a) else NAN


# ---------------------------------------------------------------- Eigen's orders (see the module text)

def dot3(a, b):
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])


def norm3(a):
    return _sqrt(dot3(a, a))


def dot9(a, b):
    p0 = [a[0] * b[0], a[1] * b[1]]
    p1 = [a[2] * b[2], a[3] * b[3]]
    p0 = [p0[0] + a[4] * b[4], p0[1] + a[5] * b[5]]
    p1 = [p1[0] + a[6] * b[6], p1[1] + a[7] * b[7]]
    p0 = [p0[0] + p1[0], p0[1] + p1[1]]
    return (p0[0] + p0[1]) + a[8] * b[8]


def norm9(a):
    return _sqrt(dot9(a, a))


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def quat_mul(a, b):
    """(w, x, y, z) * (w, x, y, z)"""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx)


def transform_vector(q, v):
    vec = q[1:]
    uv = _cross(vec, v)
    uv = [u + u for u in uv]
    c = _cross(vec, uv)
    return [(v[k] + q[0] * uv[k]) + c[k] for k in range(3)]


def rotation_matrix(q):
    """row-major 3x3"""
    w, x, y, z = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1.0 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1.0 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1.0 - (txx + tyy)]


# ---------------------------------------------------------------- geometry.cc

def rotation_motion_to_quaternion(rx, ry, rz, duration_sec, hits=None):
    """geometry.cc:6-22"""
    rate = _sqrt(rx * rx + ry * ry + rz * rz)                                   # :10-12
    if rate == 0.0:
        _hit(hits, "rate_zero")
    half_theta = rate * duration_sec * 0.5                                      # :13
    s = _div(_sin(half_theta), rate + 1e-30)                                    # :14-15
    return (_cos(half_theta), rx * s, ry * s, rz * s)                           # :17-21


def integrate_motion(q, v, raw_rotation, raw_acc, global_bias, local_bias, duration_usec):
    """geometry.cc:24-53 -> (orientation, velocity, duration_usec)"""
    if duration_usec < 0:                                                       # :32
        raise Refused("CHECK_GE(duration_usec, 0)")
    duration_sec = float(duration_usec) * 1e-6                                  # :33
    local = [raw_acc[k] + local_bias[k] for k in range(3)]                      # :36-37
    rotated = transform_vector(q, local)                                        # :39-40
    glob = [rotated[k] + global_bias[k] for k in range(3)]                      # :42-43
    vel = [v[k] + glob[k] * duration_sec for k in range(3)]                     # :45-46
    return quat_mul(q, raw_rotation), vel, duration_usec                        # :49-52


# ---------------------------------------------------------------- align_time_series.cc

def _check_increasing(times):
    """CheckTimestampsIncreasing (:22-26)"""
    for i in range(len(times) - 1):
        if not times[i] < times[i + 1]:
            raise Refused("CHECK_LT(times[i], times[i + 1])")


def _lower_bound(a, v):
    lo, hi = 0, len(a)
    while lo < hi:
        mid = (lo + hi) // 2
        if a[mid] < v:
            lo = mid + 1
        else:
            hi = mid
    return lo


def merge_time_series(series, rules=REFERENCE, hits=None):
    """MergeTimeSeries (:29-113): a list of index tuples, one index per component series."""
    for t in series:
        if len(t) == 0:                                                         # :35
            raise Refused("CHECK(!component->empty())")
        _check_increasing(t)                                                    # :36
    start_time = max(t[0] for t in series)                                      # :49-50
    end_time = min(t[-1] for t in series)                                       # :54
    if end_time < start_time:                                                   # :58-60
        return []
    cur = []
    for t in series:
        idx = _lower_bound(t, start_time)                                       # :65-67
        if not idx < len(t):                                                    # :68
            raise Refused("CHECK_LT(component_time_idx, size)")
        if t[idx] > start_time:                                                 # :69-71
            _hit(hits, "merge_late_start")
            if rules.first == "idx":
                cur.append(idx)
                continue
            if not idx > 0:
                raise Refused("CHECK_GT(component_time_idx, 0)")
            cur.append(idx - 1)
        else:                                                                   # :72-75
            cur.append(idx)
    result = []
    while True:
        result.append(tuple(cur))                                               # :80
        nxt = []
        for i, t in enumerate(series):                                          # :84-91
            if cur[i] + 1 >= len(t):
                if any(cur[j] + 1 < len(series[j]) for j in range(len(series))):
                    _hit(hits, "merge_early_end")
                return result
            nxt.append(t[cur[i] + 1])
        next_time = min(nxt)                                                    # :94-95
        if nxt.count(next_time) > 1:
            _hit(hits, "merge_equal_ts")
        for i in range(len(series)):                                            # :100-109
            if nxt[i] == next_time:
                cur[i] += 1
                if rules.equal_ts == "first":
                    break


def effective_time(series, event):
    """GetEffectiveTimeStamp (:115-128): the latest of the component times"""
    return max(t[i] for t, i in zip(series, event))


class Merged:
    """MergedTimeSeries (:130-143) over {rotation times, acceleration times}"""

    def __init__(self, rot_t, acc_t, rules=REFERENCE, hits=None):
        self.series = [list(map(int, rot_t)), list(map(int, acc_t))]
        self.events = merge_time_series(self.series, rules, hits)
        self.times = [effective_time(self.series, e) for e in self.events]


def make_interpolation_intervals(reference_ts, interp_ts, rules=REFERENCE, hits=None, le_as_lt=False):
    """MakeInterpolationIntervals (:155-196): per reference timestamp a list of
    (reference_end_time_index, interpolation_end_time_index, start_usec, end_usec)."""
    _check_increasing(reference_ts)                                             # :158
    _check_increasing(interp_ts)                                                # :159
    if not reference_ts or not interp_ts:                                       # front() of an empty vector (:163)
        raise Refused("front() of an empty vector")
    guard = rules.idx_guard == "keep"
    result = []
    latest_ts = min(interp_ts[0], reference_ts[0])                              # :162-163
    idx, n = 0, len(interp_ts)
    last_split = None
    for r, reference_ts_r in enumerate(reference_ts):                           # :164-165
        intervals = []
        while idx < n and (interp_ts[idx] < reference_ts_r if le_as_lt else interp_ts[idx] <= reference_ts_r):   # :169-170
            ts = interp_ts[idx]
            if ts > latest_ts and (idx > 0 or not guard) and r > 0:             # :173-177
                intervals.append((r, idx, latest_ts, ts))
                if ts == reference_ts_r:
                    _hit(hits, "sample_on_fix")
            latest_ts = ts                                                      # :178
            idx += 1                                                            # :179
        if r > 0 and idx == 0:
            _hit(hits, "fix_before_first_event")
        if r > 0 and idx == n and reference_ts_r > latest_ts:
            _hit(hits, "fix_after_last_event")
        if (idx > 0 or not guard) and r > 0 and idx < n and reference_ts_r > latest_ts and rules.split == "keep":   # :185-190
            intervals.append((r, idx, latest_ts, reference_ts_r))
            _hit(hits, "split_event")
            if last_split == (r - 1, idx) and len(intervals) == 1:
                _hit(hits, "two_fixes_between_samples")
            last_split = (r, idx)
        latest_ts = reference_ts_r                                              # :191
        if len(intervals) in STEP_COUNTS:
            _hit(hits, "interval_steps_%d" % len(intervals))
        result.append(intervals)                                                # :192
    return result


# ---------------------------------------------------------------- velocity.cc

class Calibrator:
    """AccelerometerCalibrator (velocity.cc:29-39): one window of GPS fixes against the whole IMU recording."""

    def __init__(self, gps, rot, acc, rules=REFERENCE, hits=None, merged=None):
        self.rules, self.hits = rules, hits
        self.ref_v = [float(v) for v in gps[0]]
        self.ref_t = [int(t) for t in gps[1]]
        self.rot = [tuple(float(c) for c in r) for r in rot[0]]
        self.acc = [tuple(float(c) for c in a) for a in acc[0]]
        self.imu = merged if merged is not None else Merged(rot[1], acc[1], rules, hits)     # :35-37
        self.intervals = make_interpolation_intervals(self.ref_t, self.imu.times, rules, hits)   # :14-26, :38-39
        counts = [len(iv) for iv in self.intervals]
        total = sum(counts)
        if len(counts) == 1:
            _hit(hits, "window_one_fix")
        elif total == 0:
            _hit(hits, "window_no_steps")
        if total and total % 128 == 0:
            _hit(hits, "window_steps_multiple_of_128")
        if len(counts) >= 4 and all(c == 1 for c in counts[1:]):
            _hit(hits, "window_all_one_step_intervals")
        if counts and max(counts) > 19 * 128 and 1 in counts:
            _hit(hits, "long_interval_20_chunks")
        if len(counts) >= 300:
            _hit(hits, "window_many_fixes")

    def steps(self):
        """the window's intervals in order, flattened"""
        return [iv for ivs in self.intervals for iv in ivs]

    def eval(self, x):
        """AccelerometerCalibrator::eval (velocity.cc:41-180) -> (loss, gradient[9])"""
        rules, hits = self.rules, self.hits
        if len(x) != 9:                                                         # :47
            raise Refused("CHECK_EQ(in.size(), 9)")
        gradient = [0.0] * 9                                                    # :50-52
        global_bias, local_bias = list(x[0:3]), list(x[3:6])                    # :55-56
        result = 0.0                                                            # :59
        q = (1.0, 0.0, 0.0, 0.0)                                                # :62
        v = list(x[6:9])                                                        # :57, :63
        twr = [0.0] * 9                                                         # :64
        total_time_usec = 0                                                     # :65
        grand_total_usec = 0
        for intervals in self.intervals:                                        # :67-68
            travel = [0.0, 0.0, 0.0]                                            # :71
            reference_distance = 0.0                                            # :74
            outcomes = []                                                       # :78
            if rules.total_time == "per_interval":
                total_time_usec = 0
            if rules.twr == "per_interval":
                twr = [0.0] * 9
            for r_idx, i_idx, start_usec, end_usec in intervals:                # :79
                ri, ai = self.imu.events[i_idx]                                 # :80-85
                if not start_usec <= end_usec:                                  # DurationSec (align_time_series.cc:145-148)
                    raise Refused("CHECK_LE(start_usec, end_usec)")
                duration_sec = float(end_usec - start_usec) * 1e-6
                raw_rotation = rotation_motion_to_quaternion(*self.rot[ri], duration_sec, hits)     # :87-90
                before = v
                q, v, dur = integrate_motion(q, v, raw_rotation, self.acc[ai], global_bias, local_bias, end_usec - start_usec)   # :95-102
                outcomes.append((q, dur))                                       # :99
                tv = before if rules.travel == "before" else v
                travel = [travel[k] + duration_sec * tv[k] for k in range(3)]   # :111-112
                reference_distance = reference_distance + duration_sec * self.ref_v[r_idx]         # :116-118
            if intervals and travel == [0.0, 0.0, 0.0]:
                _hit(hits, "travel_zero")
            distance_diff = norm3(travel) - reference_distance                  # :122
            result = result + distance_diff * distance_diff                     # :123
            den = norm3(travel) + 1e-5 if rules.travel_eps == "keep" else norm3(travel)
            d = [_div((2.0 * distance_diff) * travel[k], den) for k in range(3)]     # :126-128
            for oq, dur in outcomes:                                            # :130-131
                interval_sec = float(dur) * 1e-6                                # :132-133
                total_time_usec += dur                                          # :134
                grand_total_usec += dur
                total_time_sec = float(total_time_usec) * 1e-6                  # :135
                for k in range(3):                                              # :141-143
                    gradient[k] = gradient[k] + total_time_sec * interval_sec * d[k]
                R = rotation_matrix(oq)                                         # :149-150
                twr = [twr[k] + R[k] * interval_sec for k in range(9)]          # :152
                # interval_sec * twr^T * d (:154-156): the scaled transpose, then rows dot d
                scaled = [[interval_sec * twr[3 * c + row] for c in range(3)] for row in range(3)]
                for k in range(3):                                              # :157-159
                    gradient[3 + k] = gradient[3 + k] + dot3(scaled[k], d)
                for k in range(3):                                              # :162-164
                    gradient[6 + k] = gradient[6 + k] + interval_sec * d[k]
        total_time_sec = float(grand_total_usec) * 1e-6                         # :169
        result = _div(result, total_time_sec)                                   # :170
        gradient = [_div(g, total_time_sec) for g in gradient]                  # :171-173
        if result != result and grand_total_usec > 0:
            _hit(hits, "nan_loss")
        return result, gradient

    def integrate_trajectory(self, global_bias, local_bias, initial_velocity):
        """IntegrateTrajectory (velocity.cc:199-256) -> {event index: [orientation, velocity, duration_usec]}"""
        result = {}                                                             # :204
        q, v = (1.0, 0.0, 0.0, 0.0), list(initial_velocity)                     # :206-207
        for intervals in self.intervals:                                        # :209-211
            for r_idx, i_idx, start_usec, end_usec in intervals:
                ri, ai = self.imu.events[i_idx]                                 # :212-218
                raw_rotation = rotation_motion_to_quaternion(*self.rot[ri], float(end_usec - start_usec) * 1e-6)   # :220-223
                q, v, dur = integrate_motion(q, v, raw_rotation, self.acc[ai], global_bias, local_bias, end_usec - start_usec)   # :228-234
                if i_idx not in result:                                         # :239-243
                    result[i_idx] = [q, v, dur]
                else:                                                           # :244-251
                    _hit(self.hits, "split_event_in_trajectory")
                    if self.rules.split_winner == "later":
                        result[i_idx][0], result[i_idx][1] = q, v
                    result[i_idx][2] += dur
        return result


# ---------------------------------------------------------------- LBFGS.h, LBFGS/LineSearch.h

def minimize(f, x, epsilon=EPSILON, max_iterations=0, rules=REFERENCE, hits=None):
    """LBFGSSolver::minimize (LBFGS.h:78-182) with LineSearch::Backtracking under the default LBFGS_LINESEARCH_BACKTRACKING_ARMIJO
    (LineSearch.h:40-111), past = 0.  -> (x, fx, iterations); iterations < 0 where the reference throws: -2 the step fell below
    min_step (LineSearch.h:103-104), -3 it rose above max_step (:106-107)."""
    m = LB_M
    x = list(x)

    def converged(xnorm, gnorm):                                                # LBFGS.h:93, :119
        if rules.conv == "plain":
            return gnorm <= epsilon * xnorm
        return gnorm <= epsilon * (1.0 if xnorm < 1.0 else xnorm)              # std::max(xnorm, 1.0)

    fx, grad = f(x)                                                             # :86
    xnorm, gnorm = norm9(x), norm9(grad)                                        # :87-88
    if converged(xnorm, gnorm):                                                 # :93-96
        _hit(hits, "exit_first_eval")
        return x, fx, 1
    drt = [-g for g in grad]                                                    # :99
    step = _div(1.0, norm9(drt))                                                # :101
    k, end = 1, 0                                                               # :103-104
    s = [[0.0] * 9 for _ in range(m)]          # m_s, m_y: resized, never read before written under bound = min(m, k)
    y = [[0.0] * 9 for _ in range(m)]
    ys_hist, alpha = [0.0] * m, [0.0] * m
    while True:
        xp, gradp = list(x), list(grad)                                         # :108-109
        # ---- Backtracking (LineSearch.h:40-111)
        fx_init = fx                                                            # :55
        dg_init = dot9(grad, drt)                                               # :57
        dg_test = LB_FTOL * dg_init                                             # :62
        it = 0
        while it < LB_TRIALS:                                                   # :66
            x = [xp[i] + step * drt[i] for i in range(9)]                       # :69
            fx, grad = f(x)                                                     # :71
            rhs = fx_init + step * dg_test
            if fx > rhs or (rules.armijo == "ge" and fx == rhs):                # :73-75: width = dec
                pass
            else:                                                               # :76-79
                if fx != fx:
                    _hit(hits, "nan_search_succeeds")
                _hit(hits, "search_0_halvings" if it == 0 else "search_many_halvings" if it >= 3 else "search_few_halvings")
                break
            # :100-101 cannot fire: iter < max_linesearch inside the loop
            if step < LB_MIN_STEP:                                              # :103-104
                _hit(hits, "exit_-2")
                return x, fx, -2
            if step > LB_MAX_STEP:                                              # :106-107
                _hit(hits, "exit_-3")
                return x, fx, -3
            step = step * 0.5                                                   # :109
            it += 1
        else:
            _hit(hits, "search_20_fail")       # the loop ends, nothing throws: the solver goes on from the twentieth trial point
        # ---- back in minimize
        xnorm, gnorm = norm9(x), norm9(grad)                                    # :115-116
        if converged(xnorm, gnorm):                                             # :119-122
            _hit(hits, "converged_k_gt_1" if k > 1 else "converged_k_1")
            return x, fx, k
        if max_iterations != 0 and k >= max_iterations:                         # :132-135
            _hit(hits, "max_iter_1" if k == 1 else "max_iter_wraps" if k > m else "max_iter_few")
            return x, fx, k
        s[end] = [x[i] - xp[i] for i in range(9)]                               # :140-142
        y[end] = [grad[i] - gradp[i] for i in range(9)]                         # :143
        ys = dot9(y[end], s[end])                                               # :147
        yy = dot9(y[end], y[end])                                               # :148
        ys_hist[end] = ys                                                       # :149
        drt = [-g for g in grad]                                                # :152
        bound = m if rules.bound == "m" else min(m, k)                          # :153
        end = (end + 1) % m                                                     # :154
        j = end                                                                 # :155
        for _ in range(bound):                                                  # :156-163
            j = (j + m - 1) % m
            alpha[j] = _div(dot9(s[j], drt), ys_hist[j])
            drt = [drt[i] - alpha[j] * y[j][i] for i in range(9)]
        sc = _div(ys, ys) if rules.scale == "ys/ys" else _div(ys, yy)           # :165
        drt = [d * sc for d in drt]
        for _ in range(bound):                                                  # :167-174
            beta = _div(dot9(y[j], drt), ys_hist[j])
            ab = alpha[j] - beta
            drt = [drt[i] + ab * s[j][i] for i in range(9)]
            j = (j + 1) % m
        if rules.step_reset == "one":
            step = 1.0                                                          # :177
        k += 1                                                                  # :178


# ---------------------------------------------------------------- fit_motion.cc

def check_flags(batch, shift, iters, sigma=None):
    """main()'s CHECKs on the fit's arguments (fit_motion.cc:307-311)"""
    if not iters > 0:
        raise Refused("CHECK_GT(FLAGS_optimization_iters, 0)")
    if not batch > 0:
        raise Refused("CHECK_GT(FLAGS_locations_batch_size, 0)")
    if not shift > 0:
        raise Refused("CHECK_GT(FLAGS_locations_shift_step, 0)")
    if not batch >= shift:
        raise Refused("CHECK_GE(FLAGS_locations_batch_size, FLAGS_locations_shift_step)")
    if sigma is not None and not sigma > 0:
        raise Refused("CHECK_GT(FLAGS_post_smoothing_sigma_sec, 0)")


def windows(n_gps, batch, shift):
    """the window loop (fit_motion.cc:179-183): [(start, end)]"""
    return [(start, min(start + batch, n_gps)) for start in range(0, n_gps, shift)]


def fit_windows(gps, rot, acc, batch, shift, iters, rules=REFERENCE, hits=None, with_calibrators=False):
    """fit_motion.cc:179-197 -> per window (x[9], residual, iterations or negative exit)"""
    check_flags(batch, shift, iters)
    if len(gps[0]) == 0:                                                        # CHECK(!locations_json.empty()) (:127)
        raise Refused("no GPS fixes")
    merged = Merged(rot[1], acc[1], rules, hits)
    if shift == batch:
        _hit(hits, "shift_eq_batch")
    if shift == 1:
        _hit(hits, "shift_1")
    out = []
    for start, end in windows(len(gps[0]), batch, shift):
        if end - start < batch and start > 0:
            _hit(hits, "last_window_short")
        cal = Calibrator((gps[0][start:end], gps[1][start:end]), rot, acc, rules, hits, merged)       # :184-190
        x, fx, it = minimize(cal.eval, [0.0] * 9, EPSILON, iters, rules, hits)                        # :192-197
        out.append((x, fx, it, cal) if with_calibrators else (x, fx, it))
    return out


def kahan_add(total, rem, v):
    """KahanSum<Vector3d>::add (include/math/math.hpp:13-19), componentwise"""
    for k in range(3):
        proposed = v[k] + rem[k]
        updated = total[k] + proposed
        actual = updated - total[k]
        rem[k] = proposed - actual
        total[k] = updated


def normal_cdf(x, mean, sigma):
    """smoothing.cc:49-53"""
    return 0.5 * (1.0 + math.erf(_div(x - mean, _sqrt(2.0) * sigma)))


def smooth_time_series(values, times, targets, sigma):
    """SmoothTimeSeries (src/slam/smoothing.cc:56-98)"""
    if not sigma > 0 or len(values) != len(times):                              # :60-61
        raise Refused("CHECK_GT(sigma, 0)")
    result = [0.0] * len(targets)
    left, right, n = 0, 0, len(values)
    for ti, target in enumerate(targets):
        while left + 1 < n and (target - times[left + 1]) > 3 * sigma:          # :71-74
            left += 1
        while right + 1 < n and (times[right] - target) < 3 * sigma:            # :75-78
            right += 1
        prev = 0.0                                                              # :80
        for i in range(left, right):                                            # :81-92
            mid = (times[i] + times[i + 1]) / 2.0
            cdf = normal_cdf(mid, target, sigma)
            result[ti] = result[ti] + values[i] * (cdf - prev)
            prev = cdf
        result[ti] = result[ti] + values[right] * (1.0 - prev)                  # :93-94
    return result


def fit_motion_velocities(gps, rot, acc, vertical_axis, batch, shift, iters, sigma, min_velocity, min_rotation, rules=REFERENCE, hits=None):
    """ComputeAndSaveForwardVelocitiesFromImu (fit_motion.cc:156-293) up to the JSON writers ->
    (time_usec[n], speed_m_s[n], forward_axis[3]), or E_LIMIT where a window's line search throws."""
    check_flags(batch, shift, iters, sigma)
    fits = fit_windows(gps, rot, acc, batch, shift, iters, rules, hits, with_calibrators=True)
    if any(it < 0 for _, _, it, _ in fits):
        _hit(hits, "negative_exit_refused")
        return E_LIMIT
    total, rem = [0.0] * 3, [0.0] * 3                                           # :171-172
    velocities = {}                                                             # :178
    for x, _, _, cal in fits:
        traj = cal.integrate_trajectory(x[0:3], x[3:6], x[6:9])                 # :204-214
        keys = sorted(traj)                                                     # a std::map iterates in key order
        for e in keys:                                                          # :218-221
            velocities.setdefault(e, []).append(norm3(traj[e][1]))
        min_rotation_cos = 1.0                                                  # :225-229
        for e in keys:
            aw = abs(traj[e][0][0])
            min_rotation_cos = aw if aw < min_rotation_cos else min_rotation_cos     # std::min(a, b): b < a ? b : a
        window_ok = _acos(min_rotation_cos) >= min_rotation                     # :231-232
        if keys and not window_ok:
            _hit(hits, "window_below_rotation_gate")
        for e in keys:                                                          # :233-244
            if rules.rot_gate == "sample":
                if not _acos(abs(traj[e][0][0])) >= min_rotation:
                    continue
            elif not window_ok:
                continue
            speed = norm3(traj[e][1])
            _hit(hits, "velocity_on_gate" if speed == min_velocity else "velocity_above_gate" if speed > min_velocity else "velocity_below_gate")
            if speed > min_velocity or (speed == min_velocity and rules.vel_gate == "ge"):            # :234-235
                qo = traj[e][0]
                inv = (qo[0], -qo[1], -qo[2], -qo[3])                           # conjugate (:238-239)
                kahan_add(total, rem, transform_vector(inv, traj[e][1]))        # :240-242
    whole = Calibrator(gps, rot, acc, rules, None)                              # :251-252
    if any(len(v) > 1 for v in velocities.values()):
        _hit(hits, "event_in_several_windows")
    if len(velocities) < len(whole.imu.events):
        _hit(hits, "event_in_no_window")
    averaged, t_sec, t_usec = [], [], []
    for e in sorted(velocities):                                                # :259-269
        t_usec.append(whole.imu.times[e])
        t_sec.append(float(t_usec[-1] - t_usec[0]) * 1e-6)
        acc_sum = 0.0                                                           # std::accumulate(begin, end, 0.0)
        for v in velocities[e]:
            acc_sum = acc_sum + v
        averaged.append(_div(acc_sum, float(len(fits) if rules.average == "windows" else len(velocities[e]))))
    smoothed = smooth_time_series(averaged, t_sec, t_sec, sigma)                # :271-273
    axis = [float(a) for a in vertical_axis]
    dp = dot3(axis, total)                                                      # :281-282
    forward = [total[k] - axis[k] * dp for k in range(3)]
    nn = norm3(forward) + 1e-5                                                  # :283 (operator/= divides: Eigen 3.3's div_assign_op)
    return t_usec, smoothed, [_div(f, nn) for f in forward]


def _acos(a):
    return math.acos(a) if -1.0 <= a <= 1.0 else NAN
