"""The sensor stage restated from the reference's text (test infrastructure only).

Plain Python / numpy, written from the reference's sources and from nothing else: not from
oracle/oracle.c and not from the kernels.  np.float32 stands where the reference has a
`float` (luke::gfloat is float, customtypes.h:22), a Python float where it has a `double`;
every expression keeps the reference's operand types and evaluation order.

What is restated, by reference file:line:

- minstd_rand0 and uniform_real_distribution<float>{0, 1} as libstdc++ evaluates them
  (MjType::generator is a std::default_random_engine, mjclass.cpp:4; bits/random.tcc,
  generate_canonical<float, 24>: the engine's range 2147483646 is below 2^24 bits only
  once, so k = 1 engine call per float; the sum and the range are floats; a quotient that
  rounds to 1 is replaced by nextafter(1, 0))
- Sensor::randomise_mu, apply_normalisation, apply_noise, ready_to_read, update_n_readings
                                      mjclass.h:137-142, 155-276
- Settings::apply_noise_params        mjclass.cpp:5293-5346
- Settings::update_sensor_settings    mjclass.cpp:5236-5265, called with the double
                                      time_per_step of mjclass.cpp:311-313
- luke::SlidingWindow                 slidingwindow.h:36-67 (on a window of GM_RING readings)
- MjClass::monitor_sensors            mjclass.cpp:741-898
- sense_gripper_state's noise calls   mjclass.cpp:920-936
- the seven samplers                  mjclass.h:278-453; configure_settings' choice of them
                                      mjclass.cpp:144-211; get_observation's stream order
                                      mjclass.cpp:1707-1959 (wrist_sensor_Z is sampled with
                                      wrist_sensor_XY's counts, 1806)
- luke::read_armadillo_gauge          myfunctions.cpp:2699-2795

Transcendentals: std::log and std::cos of a float argument are evaluated in float64 and
rounded to float32 (the correctly rounded float result but for double rounding, which no
library promises either); the rest of `mag` keeps the reference's types: -2.0 * logf in
double, sqrt in double, times the float noise_std, rounded to float (mjclass.h:211).

The bending gauge: the joint points come from cumulative angles with math.sin / math.cos,
and the cubic is the exact least-squares solution on the raw abscissa (the 4 x 4 normal
equations solved in fractions.Fraction), where the reference calls arma::polyfit.  Its value
at gauge.xpos is rounded once to float and multiplied by 1000 (gauge()).  The reference's
own evaluation loop accumulates `gfloat y` term by term (myfunctions.cpp:2742-2745: four
roundings to float of partial sums that are larger than the result); gauge_text() restates
that on the exact coefficients, and DESIGN.md section 4 records how far the two are apart.

Every function that branches records the branch it took in `trace` (a set of strings); the
case table asserts its coverage with it.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

F = np.float32
RING = 64
MINSTD_A, MINSTD_M = 16807, 2147483647
EPS = F(np.finfo(np.float32).eps)                       # numeric_limits<float>::epsilon()
TWO_PI = F(2.0 * math.pi)                               # constexpr float two_pi = 2.0 * M_PI
ONE_BELOW = np.nextafter(F(1), F(0))

# sensor slots (the order of simsettings.h's sensor macro, LUKE_MJSETTINGS_SENSOR)
SENSOR_ORDER = ("motor_state_sensor", "base_state_sensor_Z", "base_state_sensor_XY", "base_state_sensor_yaw",
                "bending_gauge", "axial_gauge", "palm_sensor", "wrist_sensor_XY", "wrist_sensor_Z",
                "cartesian_contacts_XYZ")
SLOT = {n: k for k, n in enumerate(SENSOR_ORDER)}
STATE_SENSORS = ("motor_state_sensor", "base_state_sensor_XY", "base_state_sensor_Z", "base_state_sensor_yaw",
                 "cartesian_contacts_XYZ")              # the order of mjclass.cpp:5341-5345
# window ids of the state record (gm_state.h's stream enum)
ST_GAUGE, ST_AXIAL, ST_PALM, ST_WX, ST_WY, ST_WZ, ST_MOTOR, ST_BASE, ST_YAW, ST_CART = 0, 3, 6, 7, 8, 9, 10, 13, 16, 17
ST_SI_GAUGE, ST_SI_AXIAL, ST_SI_PALM, ST_SI_WZ = 29, 32, 35, 36
RAW, CHANGE, AVERAGE, MEDIAN, SIGN, SCALED, SCALED_SQ = range(7)       # MjType::Sample


def _t(trace, name):
    if trace is not None:
        trace.add(name)


# ---------------------------------------------------------------- the generator
def minstd_next(state):
    return (int(state) * MINSTD_A) % MINSTD_M


def state_before_output(k):
    """The engine state whose next output is k."""
    return (int(k) * pow(MINSTD_A, -1, MINSTD_M)) % MINSTD_M


class Rng:
    """MjType::generator and uniform_dist {0, 1}.  `draws` counts engine calls."""

    def __init__(self, state, trace=None):
        self.state, self.draws, self.trace = int(state), 0, trace

    def engine(self):
        self.state = minstd_next(self.state)
        self.draws += 1
        return self.state

    def canonical(self):
        rng_range = F(2147483646.0)                     # _RealType(__urng.max() - __urng.min() + 1), here 2^31
        total = F(F(self.engine() - 1) * F(1))          # __sum += _RealType(__urng() - __urng.min()) * __tmp
        tmp = F(F(1) * rng_range)
        ret = F(total / tmp)
        if ret >= F(1):
            _t(self.trace, "unif:guard")
            ret = ONE_BELOW
        else:
            _t(self.trace, "unif:plain")
        return ret

    def uniform(self):
        """uniform_real_distribution<float>{0, 1}::operator(): (b - a) * canonical + a."""
        return F(F(F(1) - F(0)) * self.canonical() + F(0))


# ---------------------------------------------------------------- Sensor
class Sensor:
    """One MjType::Sensor after configure_settings (its noise parameters resolved)."""

    def __init__(self, name, in_use, normalise, read_rate, use_normalisation, use_noise, raw_value_offset,
                 noise_mag, noise_mu, noise_std, noise_overriden):
        self.name = name
        self.in_use, self.use_normalisation, self.use_noise = bool(in_use), bool(use_normalisation), bool(use_noise)
        self.normalise, self.read_rate, self.raw_value_offset = F(normalise), F(read_rate), F(raw_value_offset)
        self.noise_mag, self.noise_mu, self.noise_std = F(noise_mag), F(noise_mu), F(noise_std)
        self.noise_overriden = bool(noise_overriden)
        self.prev_steps = self.readings_per_step = self.total_readings = 1

    def randomise_mu(self, rng):
        """mjclass.h:137-142."""
        return [F(self.noise_mu * F(F(F(2) * rng.uniform()) - F(1))) for _ in range(3)]

    def apply_normalisation(self, value, trace=None):
        """mjclass.h:155-174."""
        value = F(value)
        if not self.use_normalisation:
            _t(trace, "normalise:off")
            return value
        if self.normalise <= 0:
            _t(trace, "normalise:bumper_negative" if value < 0 else "normalise:bumper_not_negative")
            return F(-1) if value < 0 else F(1)
        elif value > self.normalise:
            _t(trace, "normalise:above")
            return F(1.0)
        if value < -self.normalise:
            _t(trace, "normalise:below")
            return F(-1.0)
        _t(trace, "normalise:inside")
        return F(value / self.normalise)

    def apply_noise(self, value, rng, rand_mu, i=1, trace=None, draws=None):
        """mjclass.h:176-223.  rand_mu: this sensor's three means.  draws (a list) receives
        (kind, value before, value after the addition and before the clamp)."""
        value = F(value)
        if not self.use_noise:
            _t(trace, "noise:off")
            return value
        mu = F(rand_mu[i - 1])
        before = value
        if self.noise_std < EPS:
            _t(trace, "noise:uniform_mag" if self.noise_mag > 0 else "noise:uniform_zero_mag")
            noise = F(mu + F(self.noise_mag * F(F(F(2) * rng.uniform()) - F(1))))
            value = F(value + noise)
            kind = "uniform"
        else:
            while True:
                u1 = rng.uniform()
                if not u1 <= EPS:
                    break
                _t(trace, "noise:gauss_rejected")
            u2 = rng.uniform()
            log_u1 = F(math.log(float(u1)))
            mag = F(float(self.noise_std) * math.sqrt(-2.0 * float(log_u1)))
            z0 = F(F(mag * F(math.cos(float(F(TWO_PI * u2))))) + mu)
            value = F(value + z0)
            _t(trace, "noise:gauss")
            kind = "gauss"
        if draws is not None:
            draws.append((kind, before, value))
        if value > 1:
            _t(trace, "noise:clamp_high")
            value = F(1)
        elif value < -1:
            _t(trace, "noise:clamp_low")
            value = F(-1)
        else:
            _t(trace, "noise:inside")
        return value

    def ready_to_read(self, time, last_read, trace=None):
        """mjclass.h:225-241.  Returns (ready, new last_read_time)."""
        time_between_reads = float(F(F(1) / self.read_rate))
        due = last_read + time_between_reads
        if time > due:
            _t(trace, "ready:yes")
            return True, time
        _t(trace, "ready:at_equality" if time == due else "ready:no")
        return False, last_read

    def update_n_readings_state(self, prev_steps):
        self.prev_steps, self.readings_per_step = int(prev_steps), 1
        self.total_readings = 1 + self.readings_per_step * self.prev_steps

    def update_n_readings_time(self, time_since_last_sample):
        """mjclass.h:266-276: the parameter is a float."""
        readings_since_step = float(F(F(time_since_last_sample) * self.read_rate))
        self.readings_per_step = int(math.floor(readings_since_step))
        self.total_readings = 1 + self.readings_per_step * self.prev_steps


def make_sensors(s, time_per_step):
    """The ten sensors of a settings struct after apply_noise_params' parameter half
    (mjclass.cpp:5300-5338) and update_sensor_settings (5236-5265)."""
    out = {}
    for n in SENSOR_ORDER:
        x = getattr(s, n)
        sen = Sensor(n, x.in_use, x.normalise, x.read_rate, x.use_normalisation, x.use_noise, x.raw_value_offset,
                     x.noise_mag, x.noise_mu, x.noise_std, x.noise_overriden)
        if not sen.noise_overriden:
            sen.noise_mag, sen.noise_std, sen.noise_mu = F(s.sensor_noise_mag), F(s.sensor_noise_std), F(s.sensor_noise_mu)
        out[n] = sen
    for n in STATE_SENSORS:
        if not out[n].noise_overriden:
            out[n].noise_mag, out[n].noise_mu, out[n].noise_std = F(s.state_noise_mag), F(s.state_noise_mu), F(s.state_noise_std)
    for n in SENSOR_ORDER:
        out[n].prev_steps = int(s.sensor_n_prev_steps)
    for n in STATE_SENSORS:
        out[n].update_n_readings_state(s.state_n_prev_steps)
    for n in SENSOR_ORDER:
        if n not in STATE_SENSORS:
            out[n].update_n_readings_time(time_per_step)
    return out


def apply_noise_params(sensors, rng):
    """The draws of mjclass.cpp:5300-5311 and 5341-5345: rand_mu [10][3] by slot."""
    mu = [[F(0)] * 3 for _ in SENSOR_ORDER]
    for n in SENSOR_ORDER:
        mu[SLOT[n]] = sensors[n].randomise_mu(rng)
    for n in STATE_SENSORS:
        mu[SLOT[n]] = sensors[n].randomise_mu(rng)
    return mu


# ---------------------------------------------------------------- luke::SlidingWindow
class Window:
    def __init__(self, v, i, trace=None):
        self.v = [F(x) for x in v]
        self.i = int(i)
        self.trace = trace
        self.adds = 0

    def add(self, element):
        self.i += 1
        if self.i > len(self.v) - 1:
            _t(self.trace, "window:write_wraps")
            self.i = 0
        self.v[self.i] = F(element)
        self.adds += 1

    def latest(self):
        return self.v[0] if self.i == -1 else self.v[self.i]

    def read_element(self, n):
        assert n >= 0
        idx = self.i - n
        if idx < 0:
            _t(self.trace, "window:read_wraps")
        while idx < 0:
            idx += len(self.v)
        return self.v[idx]

    def read(self, n):
        return [self.read_element(j) for j in range(n - 1, -1, -1)]


# ---------------------------------------------------------------- the samplers
MAX_CHANGE = F(0.07)                                         # mjclass.h:107
MAX_CHANGE_2 = F(0.10)                                       # mjclass.h:110
SQ_FACTOR = F(1.0 / float(F(MAX_CHANGE_2 * MAX_CHANGE_2)))   # mjclass.h:111
SIGN_TOL = F(1e-6)                                           # mjclass.h:384


def sample(mode, sen, w, trace=None):
    """Sensor::*_sample (mjclass.h:278-453) of window w with sensor sen's counts."""
    total, rps, prev = sen.total_readings, sen.readings_per_step, sen.prev_steps
    if mode == RAW:
        _t(trace, f"sample:raw:{total - 1}")
        return w.read(total - 1)
    res = [F(0)] * (2 * prev + 1)
    res[0] = w.read_element(total - 1)
    for i in range(prev):
        first = total - 1 - i * rps
        res[2 * i + 2] = w.read_element(first - rps)
        a, b = res[2 * i], res[2 * i + 2]
        if mode == CHANGE:
            _t(trace, "sample:change")
            r = F(b - a)
        elif mode == AVERAGE:
            _t(trace, "sample:average")
            acc = F(0)
            for j in range(rps + 1):
                acc = F(acc + w.read_element(first - j))
            r = F(acc / F(rps + 1))
        elif mode == MEDIAN:
            values = sorted(w.read_element(first - j) for j in range(rps + 1))
            n = len(values) // 2
            med = values[n]
            if not len(values) & 1:
                _t(trace, "sample:median_even")
                med = F(float(F(values[n - 1] + med)) / 2.0)
            else:
                _t(trace, "sample:median_odd")
            r = med
        elif mode == SIGN:
            change = F(b - a)
            if change > SIGN_TOL:
                _t(trace, "sample:sign_up"); r = F(1.0)
            elif change < -SIGN_TOL:
                _t(trace, "sample:sign_down"); r = F(-1.0)
            else:
                _t(trace, "sample:sign_none"); r = F(0.0)
        elif mode == SCALED:
            r = F(F(b - a) / MAX_CHANGE)
            if r > 1.0:
                _t(trace, "sample:scaled_high"); r = F(1.0)
            elif r < -1.0:
                _t(trace, "sample:scaled_low"); r = F(-1.0)
            else:
                _t(trace, "sample:scaled_inside")
        else:
            change = F(abs(F(b - a)))
            r = F(F(F(b - a) * change) * SQ_FACTOR)
            if r > 1.0:
                _t(trace, "sample:scaled_sq_high"); r = F(1.0)
            elif r < -1.0:
                _t(trace, "sample:scaled_sq_low"); r = F(-1.0)
            else:
                _t(trace, "sample:scaled_sq_inside")
        res[2 * i + 1] = r
    return res


def sample_functions(s, trace=None):
    """configure_settings' sampleFcnPtr and stateFcnPtr (mjclass.cpp:144-211).  A
    state_sample_mode of scaled_change_sq assigns sampleFcnPtr (205): the state streams keep
    the pointer's earlier value, MjClass's sign_sample (DESIGN.md's quirk list)."""
    sensor_fcn, state_fcn = int(s.sensor_sample_mode), int(s.state_sample_mode)
    if state_fcn == SCALED_SQ:
        _t(trace, "sample:state_mode_6_quirk")
        sensor_fcn, state_fcn = SCALED_SQ, SIGN
    return sensor_fcn, state_fcn


def observation(s, sensors, windows, trace=None):
    """get_observation (mjclass.cpp:1707-1959).  windows: {stream id: Window}."""
    sf, tf = sample_functions(s, trace)
    out = []

    def put(name, fcn, streams, counts=None):
        if sensors[name].in_use:
            for st in streams:
                out.extend(sample(fcn, sensors[counts or name], windows[st], trace))
    put("bending_gauge", sf, (ST_GAUGE, ST_GAUGE + 1, ST_GAUGE + 2))
    put("axial_gauge", sf, (ST_AXIAL, ST_AXIAL + 1, ST_AXIAL + 2))
    put("palm_sensor", sf, (ST_PALM,))
    put("wrist_sensor_XY", sf, (ST_WX, ST_WY))
    put("wrist_sensor_Z", sf, (ST_WZ,), counts="wrist_sensor_XY")
    put("motor_state_sensor", tf, (ST_MOTOR, ST_MOTOR + 1, ST_MOTOR + 2))
    put("base_state_sensor_XY", tf, (ST_BASE, ST_BASE + 1))
    put("base_state_sensor_Z", tf, (ST_BASE + 2,))
    put("base_state_sensor_yaw", tf, (ST_YAW,))
    put("cartesian_contacts_XYZ", CHANGE, tuple(range(ST_CART, ST_CART + 12)))
    return out


# ---------------------------------------------------------------- the bending gauge
def gauge_points(joint_values, segment_length, fixed_first_segment):
    """myfunctions.cpp:2711-2736."""
    X = [segment_length if fixed_first_segment else 0.0]
    Y = [0.0]
    cumulative = 0.0
    for i, q in enumerate(joint_values):
        cumulative = float(q) if i == 0 else cumulative + float(q)
        X.append(X[i] + segment_length * math.cos(cumulative))
        Y.append(Y[i] + segment_length * math.sin(cumulative))
    return X, Y


def exact_polyfit(X, Y, order=3):
    """The least-squares polynomial through (X, Y), highest power first, exactly."""
    n = order + 1
    xs, ys = [Fraction(x) for x in X], [Fraction(y) for y in Y]
    A = [[sum(x ** (2 * order - r - c) for x in xs) for c in range(n)] for r in range(n)]
    b = [sum(x ** (order - r) * y for x, y in zip(xs, ys)) for r in range(n)]
    for k in range(n):
        p = next(r for r in range(k, n) if A[r][k] != 0)
        A[k], A[p], b[k], b[p] = A[p], A[k], b[p], b[k]
        for r in range(k + 1, n):
            f = A[r][k] / A[k][k]
            A[r] = [x - f * y for x, y in zip(A[r], A[k])]
            b[r] -= f * b[k]
    c = [Fraction(0)] * n
    for k in range(n - 1, -1, -1):
        c[k] = (b[k] - sum(A[k][j] * c[j] for j in range(k + 1, n))) / A[k][k]
    return c


def gauge_exact(joint_values, segment_length, fixed_first_segment, xpos, order=3):
    """(the fitted y at xpos as a Fraction, the tip deflection |Y| in mm)."""
    X, Y = gauge_points(joint_values, segment_length, fixed_first_segment)
    c = exact_polyfit(X, Y, order)
    xp = Fraction(xpos)
    return sum(ci * xp ** (order - i) for i, ci in enumerate(c)), abs(Y[-1]) * 1000.0


def gauge(joint_values, segment_length, fixed_first_segment, xpos, order=3):
    """read_armadillo_gauge with the fitted value rounded to float once: (float)y * 1000."""
    y, _ = gauge_exact(joint_values, segment_length, fixed_first_segment, xpos, order)
    return F(F(float(y)) * F(1000))


def gauge_text(joint_values, segment_length, fixed_first_segment, xpos, order=3):
    """The evaluation loop as written (myfunctions.cpp:2742-2745, 2794): `gfloat y`
    accumulates coeff(i) * pow(xpos, order - i) with a rounding to float per term."""
    X, Y = gauge_points(joint_values, segment_length, fixed_first_segment)
    c = exact_polyfit(X, Y, order)
    y = F(0.0)
    for i, ci in enumerate(c):
        y = F(float(y) + float(ci) * math.pow(xpos, order - i))
    return F(y * F(1000))


# ---------------------------------------------------------------- the record and the stage
class Record:
    """What the stage carries between calls: time, last_read [10], the generator's state,
    rand_mu [10][3], and the windows with their indices."""

    def __init__(self, time, last_read, rng, rand_mu, ring, ring_i, trace=None):
        self.time = float(time)
        self.last_read = [float(x) for x in last_read]
        self.rng = Rng(rng, trace)
        self.rand_mu = [[F(x) for x in row] for row in rand_mu]
        self.w = {st: Window(ring[st], ring_i[st], trace) for st in range(len(ring_i))}
        self.trace = trace
        self.draws = []                 # every noise draw: (kind, value before, value after, before the clamp)
        self.reads = []                 # (substep index, sensor name) of every reading taken
        self.gauss_slots = set()        # (stream, window slot) of every value that came from a Gaussian draw
        self.gauge_slots = {}           # (stream, window slot) -> (finger, d value / d gauge reading)

    def add(self, st, value, gauss=False, gauge=None):
        w = self.w[st]
        w.add(value)
        self.gauss_slots.discard((st, w.i))
        self.gauge_slots.pop((st, w.i), None)
        if gauss:
            self.gauss_slots.add((st, w.i))
        if gauge is not None:
            self.gauge_slots[(st, w.i)] = gauge


def monitor_sensors(rec, s, sensors, time, meas, factor, k=0):
    """mjclass.cpp:741-898 at sim time `time`.  meas() is asked for what the model cannot
    derive: meas("gauges") -> three raw gauge readings (floats), meas("axial") -> three SI
    values, meas("palm") -> the palm's SI value after the scale factor (or
    meas("palm_raw") -> before it, when given)."""
    tr = rec.trace

    def ready(name):
        ok, rec.last_read[SLOT[name]] = sensors[name].ready_to_read(time, rec.last_read[SLOT[name]], tr)
        if ok:
            rec.reads.append((k, name))
        return ok

    def noisy(name, value, i):
        sen = sensors[name]
        return sen.apply_noise(value, rec.rng, rec.rand_mu[SLOT[name]], i, tr, rec.draws)

    def gaussian(name):
        return sensors[name].use_noise and not sensors[name].noise_std < EPS

    if ready("bending_gauge"):
        sen = sensors["bending_gauge"]
        g = [F(x) for x in meas("gauges")]
        for f in range(3):
            rec.add(ST_SI_GAUGE + f, F(float(g[f]) * factor), gauge=(f, factor))
        g = [sen.apply_normalisation(x, tr) for x in g]
        g = [noisy("bending_gauge", g[f], f + 1) for f in range(3)]
        scale = 1.0 / float(sen.normalise) if sen.use_normalisation and sen.normalise > 0 else 1.0
        for f in range(3):
            rec.add(ST_GAUGE + f, g[f], gaussian("bending_gauge"), gauge=(f, scale))
    if ready("axial_gauge"):
        sen = sensors["axial_gauge"]
        a = [F(x) for x in meas("axial")]
        for f in range(3):
            rec.add(ST_SI_AXIAL + f, a[f])
        a = [sen.apply_normalisation(x, tr) for x in a]
        a = [noisy("axial_gauge", a[f], f + 1) for f in range(3)]
        for f in range(3):
            rec.add(ST_AXIAL + f, a[f], gaussian("axial_gauge"))
    if ready("palm_sensor"):
        sen = sensors["palm_sensor"]
        raw = meas("palm_raw")
        if raw is not None:
            p = F(float(F(raw)) * float(s.palm_scale_factor))       # gfloat *= double
        else:
            p = F(meas("palm"))
        rec.add(ST_SI_PALM, p)
        p = sen.apply_normalisation(p, tr)
        p = noisy("palm_sensor", p, 1)
        rec.add(ST_PALM, p, gaussian("palm_sensor"))
    if ready("wrist_sensor_Z"):
        sen = sensors["wrist_sensor_Z"]
        z = F(0.0)                                                  # data->userdata[2], written nowhere
        z = F(z - sen.raw_value_offset)
        rec.add(ST_SI_WZ, z)
        z = sen.apply_normalisation(z, tr)
        z = noisy("wrist_sensor_Z", z, 1)
        rec.add(ST_WZ, z, gaussian("wrist_sensor_Z"))


def sense_gripper_state_noise(rec, sensors, readings):
    """mjclass.cpp:920-936 on the seven normalised readings (gripper x, y, z, base x, y, z,
    yaw): the noise calls in their order, then the appends."""
    tr = rec.trace
    calls = (("motor_state_sensor", 1), ("motor_state_sensor", 2), ("motor_state_sensor", 3),
             ("base_state_sensor_XY", 1), ("base_state_sensor_XY", 2), ("base_state_sensor_Z", 1),
             ("base_state_sensor_yaw", 1))
    vals = []
    for (name, i), v in zip(calls, readings):
        vals.append(sensors[name].apply_noise(v, rec.rng, rec.rand_mu[SLOT[name]], i, tr, rec.draws))
    for st, v, (name, _) in zip((ST_MOTOR, ST_MOTOR + 1, ST_MOTOR + 2, ST_BASE, ST_BASE + 1, ST_BASE + 2, ST_YAW), vals, calls):
        rec.add(st, v, sensors[name].use_noise and not sensors[name].noise_std < EPS)
    return vals


def substep_times(time, dt, n):
    """mjData's time after each of n substeps: time += timestep."""
    out = []
    for _ in range(n):
        time = time + dt
        out.append(time)
    return out
