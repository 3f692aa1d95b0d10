"""The env-step readout restated from the reference's text (test infrastructure only).

Plain Python / numpy, written from the reference's sources and from nothing else: not
from oracle/oracle.c and not from the kernel.  np.float32 stands where the reference has a
`float`, a Python float where it has a `double`; every expression keeps the reference's
operand types and evaluation order, and the event loops run in the macro order of
simsettings.h (gmx.BINARY_EVENTS / LINEAR_EVENTS are that order).

What is restated, by reference file:line:

- update_env's event rules            mjclass.cpp:1138-1293 (values of 1011-1068 as far as
                                      they can be formed from the state record)
- the successful_grasp macro          mjclass.cpp:1305-1320
- update_events                       mjclass.cpp:5437-5469
- calc_rewards, reward() and its caps mjclass.cpp:5471-5528, 3000-3049
- is_done                             mjclass.cpp:1632-1698; MjEnv.step (MjEnv.py:2188-2205)
                                      calls it before reward(), so a done caused by the cap
                                      shows one step late
- linear_reward, normalise_between    mjclass.cpp:4866-4904
- set_continous_action / set_action   mjclass.cpp:1517-1630 with ActionSetting's function
                                      choice (mjclass.h:488-571), configure_settings' action
                                      list (mjclass.cpp:109-141), luke::move_* and
                                      lift_base_to_height (myfunctions.cpp:2422-2536), the
                                      Gripper limits (gripper.h:29-58, 84-165;
                                      gripper.cpp:6-131), the base limits
                                      (myfunctions.cpp:245-261) and get_fingertip_z_height
                                      (myfunctions.cpp:3608-3620)
- sense_gripper_state's seven state readings, noise off   mjclass.cpp:900-936
- the observation's length            mjclass.cpp:1707-1959 by stream, Sensor::update_n_readings
                                      (mjclass.h:243-276), update_sensor_settings
                                      (mjclass.cpp:5236-5265)

Two points the reference's text settles:

- Obj::peak_finger_axial_force (mjclass.h:824) is value-initialised and assigned nowhere:
  mjclass.cpp:1099 writes env_.grp.peak_finger_axial_force, another field.  The second
  operand of the `lifted` rule (mjclass.cpp:1156) is therefore 0 < ftol, always true.
- `abs(continous_fraction)` (mjclass.cpp:1571) is unqualified, but gripper.h includes
  <math.h>, whose C++ wrapper brings std::abs's float overload into the global namespace:
  the penalty is |fraction| as a float, not truncated to int.

Every function that branches records the branch it took in `trace` (a set of strings); the
case table asserts its coverage with it.
"""
from __future__ import annotations

import math

import numpy as np

F = np.float32
FTOL = 1e-5                     # MjClass::ftol, a double (mjclass.h:1570)


def _t(trace, name):
    if trace is not None:
        trace.add(name)


class Undecided(Exception):
    """A comparison on the palm force magnitude that its known bounds do not decide."""


class Interval:
    """The palm force magnitude is not in the state record: it is known only as
    lo <= value <= hi (0, 0 without palm contact; the axial component from below)."""

    def __init__(self, lo, hi):
        self.lo, self.hi = float(lo), float(hi)

    def gt(self, x):
        if self.lo > x:
            return True
        if self.hi <= x:
            return False
        raise Undecided(f"palm magnitude in [{self.lo}, {self.hi}] > {x}")

    def lt(self, x):
        if self.hi < x:
            return True
        if self.lo >= x:
            return False
        raise Undecided(f"palm magnitude in [{self.lo}, {self.hi}] < {x}")


# ---------------------------------------------------------------- utility functions
def linear_reward(val, mn, mx, overshoot, trace=None):
    """mjclass.cpp:4866-4894, all float."""
    val, mn, mx, overshoot = F(val), F(mn), F(mx), F(overshoot)
    if val < mn:
        _t(trace, "linear:below_min")
        return F(0.0)
    if val > mx:
        if overshoot < mx:
            _t(trace, "linear:saturated")
            return F(1.0)
        if val > overshoot:
            _t(trace, "linear:past_overshoot")
            return F(0.0)
        _t(trace, "linear:falling")
        mn = F(0)
        mx = F(overshoot - mx)
        val = F(overshoot - val)
    else:
        _t(trace, "linear:rising")
    return F(F(val - mn) / F(mx - mn))


def normalise_between(val, mn, mx, trace=None):
    """mjclass.cpp:4896-4904, all float (the arguments are converted at the call)."""
    val, mn, mx = F(val), F(mn), F(mx)
    if val > mx:
        _t(trace, "normalise:above")
        return F(1.0)
    if val < mn:
        _t(trace, "normalise:below")
        return F(-1.0)
    _t(trace, "normalise:at_max" if val == mx else "normalise:at_min" if val == mn else "normalise:inside")
    return F(F(F(F(2) * F(val - mn)) / F(mx - mn)) - F(1))


def c_round(x):
    """C's round(): halves away from zero."""
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


# ---------------------------------------------------------------- luke::Gripper
class Gripper:
    """gripper.h:29-58 (constants), 84-165 (setters), gripper.cpp:6-131 (limits)."""
    to_rad = math.pi / 180.0
    limit_tol = 1e-4
    leadscrew_dist = 35e-3
    finger_length = 235e-3
    hook_length = 35.0e-3
    xy_min, xy_max, z_min, z_max = 49e-3, 134e-3, 0e-3, 165e-3
    th_min, th_max = -40 * to_rad, 40 * to_rad
    fingertip_radius_min = -1
    hypotenuse = math.sqrt(math.pow(finger_length, 2) + math.pow(hook_length, 2))
    resting_angle = math.atan(hook_length / finger_length)
    xy_step_m = 4 / (1.0 * 400 * 1e3)
    z_step_m = 4.8768 / (1 * 400 * 1e3)

    def __init__(self, x, y, z, th, trace=None):
        self.x, self.y, self.z, self.th = float(x), float(y), float(z), float(th)
        self.sx = self.sy = self.sz = None
        self.trace = trace

    def calc_y(self, th):
        return self.x + 1 * self.leadscrew_dist * math.sin(th)

    def calc_th(self, x, y):
        return math.asin((y - x) / self.leadscrew_dist) * 1

    def get_th_rad(self):
        return self.calc_th(self.x, self.y)

    def calc_max_fingertip_angle(self):
        a = (self.fingertip_radius_min - self.x) / self.hypotenuse
        if not -1.0 <= a <= 1.0:
            return math.nan                         # asin outside its domain: the check below is false
        return (math.asin(a) + self.resting_angle) * 1

    def update_xy(self):
        wl = True
        if self.x > self.xy_max + self.limit_tol:
            _t(self.trace, "limit:x_max"); self.x = self.xy_max; wl = False
        if self.x < self.xy_min - self.limit_tol:
            _t(self.trace, "limit:x_min"); self.x = self.xy_min; wl = False
        if self.y > self.xy_max + self.limit_tol:
            _t(self.trace, "limit:y_max"); self.y = self.xy_max; wl = False
        if self.y < self.xy_min - self.limit_tol:
            _t(self.trace, "limit:y_min"); self.y = self.xy_min; wl = False
        new_th = self.calc_th(self.x, self.y)
        if new_th > self.th_max:
            _t(self.trace, "limit:th_max"); new_th = self.th_max; self.y = self.calc_y(self.th_max); wl = False
        if new_th < self.th_min:
            _t(self.trace, "limit:th_min"); new_th = self.th_min; self.y = self.calc_y(self.th_min); wl = False
        self.th = new_th
        th_lim = self.calc_max_fingertip_angle()
        if self.th < th_lim:
            _t(self.trace, "limit:fingertip_radius"); self.y = self.calc_y(th_lim); self.th = th_lim; wl = False
        self.sx = c_round((self.xy_max - self.x) / self.xy_step_m)
        self.sy = c_round((self.xy_max - self.y) / self.xy_step_m)
        return wl

    def update_z(self):
        wl = True
        if self.z > self.z_max + self.limit_tol:
            _t(self.trace, "limit:z_max"); self.z = self.z_max; wl = False
        if self.z < self.z_min - self.limit_tol:
            _t(self.trace, "limit:z_min"); self.z = self.z_min; wl = False
        self.sz = c_round(self.z / self.z_step_m)
        return wl

    def set_xyz_m(self, x, y, z):
        self.x, self.y, self.z = x, y, z
        wl = True
        wl = bool(wl * self.update_xy())
        wl = bool(wl * self.update_z())
        return wl

    def set_xyz_m_rad(self, x, th, z):
        self.x = x
        self.y = self.calc_y(th)
        in_lim = self.update_xy()
        self.z = z
        return in_lim if self.update_z() else False


# ---------------------------------------------------------------- configuration
ACTION_NAMES = ("gripper_X", "gripper_prismatic_X", "gripper_Y", "gripper_revolute_Y", "gripper_Z",
                "base_X", "base_Y", "base_Z", "base_roll", "base_pitch", "base_yaw")     # simsettings.h:119-129
POSITIVE, NEGATIVE, CONTINOUS = 0, 1, 2                     # MjType::Action, three codes per action
TERMINATION = 3 * len(ACTION_NAMES)
BASE_MIN = (-500e-3, -500e-3, -30e-3, -0.5, -0.5, -math.pi / 2)       # myfunctions.cpp:247-259
BASE_MAX = (500e-3, 500e-3, 30e-3, 0.5, 0.5, math.pi / 2)


def action_options(s):
    """configure_settings, mjclass.cpp:109-141."""
    out = []
    for k, name in enumerate(ACTION_NAMES):
        if getattr(s, name).in_use:
            out += [3 * k + CONTINOUS] if s.continous_actions else [3 * k + POSITIVE, 3 * k + NEGATIVE]
    if s.use_termination_action:
        out.append(TERMINATION)
    return out


def n_obs(s):
    """get_observation's length: per stream the sampler's size, 2 * prev_steps + 1 (raw:
    total_readings - 1), over the streams of mjclass.cpp:1707-1959.  wrist_sensor_Z is
    sampled through wrist_sensor_XY's counts."""
    tfa = F(s.time_for_action)

    def size(sensor_name, state):
        sen = getattr(s, sensor_name)
        mode = s.state_sample_mode if state else s.sensor_sample_mode
        prev = s.state_n_prev_steps if state else s.sensor_n_prev_steps
        if sensor_name == "cartesian_contacts_XYZ":
            return 2 * prev + 1                                  # always the change sampler
        if mode == 0:                                            # MjType::Sample::raw
            rps = 1 if state else int(math.floor(float(tfa) * float(sen.read_rate)))
            return rps * prev
        return 2 * prev + 1
    n = 0
    if s.bending_gauge.in_use: n += 3 * size("bending_gauge", False)
    if s.axial_gauge.in_use: n += 3 * size("axial_gauge", False)
    if s.palm_sensor.in_use: n += size("palm_sensor", False)
    if s.wrist_sensor_XY.in_use: n += 2 * size("wrist_sensor_XY", False)
    if s.wrist_sensor_Z.in_use: n += size("wrist_sensor_XY", False)
    if s.motor_state_sensor.in_use: n += 3 * size("motor_state_sensor", True)
    if s.base_state_sensor_XY.in_use: n += 2 * size("base_state_sensor_XY", True)
    if s.base_state_sensor_Z.in_use: n += size("base_state_sensor_Z", True)
    if s.base_state_sensor_yaw.in_use: n += size("base_state_sensor_yaw", True)
    if s.cartesian_contacts_XYZ.in_use: n += 12 * size("cartesian_contacts_XYZ", True)
    return n


def n_streams(s):
    return (3 * bool(s.bending_gauge.in_use) + 3 * bool(s.axial_gauge.in_use) + bool(s.palm_sensor.in_use)
            + 2 * bool(s.wrist_sensor_XY.in_use) + bool(s.wrist_sensor_Z.in_use) + 3 * bool(s.motor_state_sensor.in_use)
            + 2 * bool(s.base_state_sensor_XY.in_use) + bool(s.base_state_sensor_Z.in_use)
            + bool(s.base_state_sensor_yaw.in_use) + 12 * bool(s.cartesian_contacts_XYZ.in_use))


# ---------------------------------------------------------------- actions
class Target:
    """target_ (the gripper and base targets) and what set_action carries to update_env."""

    def __init__(self, end, base, exceed_limits_value, penalty_lin, penalty_sq):
        self.end = end
        self.base = [float(b) for b in base]
        self.exceed_limits_value = bool(exceed_limits_value)
        self.penalty_lin, self.penalty_sq = F(penalty_lin), F(penalty_sq)
        self.termination_signal_sent = False
        self.lift_substeps = 0


def _clamp_base(tg, k, trace, name):
    wl = True
    if tg.base[k] > BASE_MAX[k]:
        _t(trace, f"limit:{name}_max"); tg.base[k] = BASE_MAX[k]; wl = False
    if tg.base[k] < BASE_MIN[k]:
        _t(trace, f"limit:{name}_min"); tg.base[k] = BASE_MIN[k]; wl = False
    return wl


def move_base_target_m(tg, x, y, z, trace):
    tg.base[0] += x; tg.base[1] += y; tg.base[2] += z
    wl = True
    for k, name in enumerate(("base_x", "base_y", "base_z")):
        wl = _clamp_base(tg, k, trace, name) and wl
    return wl


def move_base_target_rad(tg, roll, pitch, yaw, trace):
    tg.base[5] += yaw                                    # roll and pitch do nothing (myfunctions.cpp:2495-2497)
    return _clamp_base(tg, 5, trace, "base_yaw")


def call_action_function(tg, name, sign, call_value, trace):
    """mjclass.h:488-571."""
    call_value *= sign
    arg = 0 if name.endswith(("X", "roll")) else 1 if name.endswith(("Y", "pitch")) else 2
    a = [0.0, 0.0, 0.0]
    a[arg] = call_value
    if name.startswith("gripper"):
        e = tg.end
        if name.endswith(("prismatic_X", "revolute_Y")):
            return e.set_xyz_m_rad(e.x + a[0], e.th + a[1], e.z + a[2])
        return e.set_xyz_m(e.x + a[0], e.y + a[1], e.z + a[2])
    if name.endswith(("X", "Y", "Z")):
        return move_base_target_m(tg, a[0], a[1], a[2], trace)
    return move_base_target_rad(tg, a[0], a[1], a[2], trace)


def fingertip_z_height(tg, finger_length):
    """myfunctions.cpp:3608-3620."""
    straight = F(-BASE_MIN[2] - tg.base[2])
    tip_lift = F(finger_length * (1 - math.cos(tg.end.get_th_rad())))
    height_above_min = F(straight + tip_lift)
    return F(float(height_above_min) + BASE_MIN[2])


def set_action(tg, s, finger_length, sim_steps_per_action, action, continous_fraction, trace=None):
    """MjClass::set_action, mjclass.cpp:1528-1630."""
    wl = True
    tg.termination_signal_sent = False
    options = action_options(s)
    if action < 0 or action >= len(options):
        _t(trace, "action:out_of_range")
        return
    code = options[action]
    frac = F(continous_fraction)
    if code == TERMINATION:
        value = frac if s.continous_actions else F(1.0)
        triggered = bool(value > F(s.termination_threshold))
        _t(trace, "termination:triggered" if triggered else "termination:below_threshold")
        if triggered:
            tg.termination_signal_sent = True
            if s.lift_on_termination:
                _t(trace, "termination:lift")
                tg.base[2] = -BASE_MAX[2]                       # lift_base_to_height(base_max_[2])
                _clamp_base(tg, 2, trace, "base_z")
                tg.lift_substeps += sim_steps_per_action * 2
            else:
                _t(trace, "termination:no_lift")
        wl = True
    else:
        name, sub = ACTION_NAMES[code // 3], code % 3
        a = getattr(s, name)
        _t(trace, f"code:{name}:{('positive', 'negative', 'continous')[sub]}")
        if sub == POSITIVE:
            wl = call_action_function(tg, name, a.sign, a.value, trace)
        elif sub == NEGATIVE:
            wl = call_action_function(tg, name, a.sign, -1 * a.value, trace)
        else:
            wl = call_action_function(tg, name, a.sign, a.value * float(frac), trace)
            tg.penalty_lin = F(tg.penalty_lin + F(abs(frac)))
            tg.penalty_sq = F(tg.penalty_sq + F(frac * frac))
    if float(fingertip_z_height(tg, finger_length)) < s.fingertip_min_mm * 1e-3:
        _t(trace, "limit:fingertip_min")
        wl = False
    if not wl:
        _t(trace, "exceed_limits:set")
    elif tg.exceed_limits_value:
        _t(trace, "exceed_limits:latched")
    tg.exceed_limits_value = bool(tg.exceed_limits_value + (not wl))


def set_actions(tg, s, finger_length, sim_steps_per_action, continuous=None, discrete=None, trace=None):
    """MjEnv._take_action: set_continous_action for every index in order (the fraction
    clipped to [-1, 1], mjclass.cpp:1521-1523), or one set_discrete_action."""
    if continuous is not None:
        for i, f in enumerate(continuous):
            f = F(f)
            if f < F(-1.0):
                _t(trace, "fraction:clipped_low"); f = F(-1.0)
            elif f > F(1.0):
                _t(trace, "fraction:clipped_high"); f = F(1.0)
            set_action(tg, s, finger_length, sim_steps_per_action, i, f, trace)
    else:
        set_action(tg, s, finger_length, sim_steps_per_action, int(discrete), 0, trace)


def state_readings(tg, trace=None):
    """sense_gripper_state's normalised readings, noise off (mjclass.cpp:909-918):
    gripper x, y, z, base x, y, z, yaw."""
    e, b = tg.end, tg.base
    return [normalise_between(e.x, Gripper.xy_min, Gripper.xy_max, trace),
            normalise_between(e.y, Gripper.xy_min, Gripper.xy_max, trace),
            normalise_between(e.z, Gripper.z_min, Gripper.z_max, trace),
            normalise_between(b[0], BASE_MIN[0], BASE_MAX[0], trace),
            normalise_between(b[1], BASE_MIN[1], BASE_MAX[1], trace),
            normalise_between(b[2], BASE_MIN[2], BASE_MAX[2], trace),
            normalise_between(b[5], BASE_MIN[5], BASE_MAX[5], trace)]


# ---------------------------------------------------------------- update_env
def update_env(prior, s, n_actions, meas, binary_events, linear_events, trace=None):
    """mjclass.cpp:1011-1068 (values), 1138-1293 (rules), 1305-1320 (successful_grasp),
    5437-5469 (update_events).

    prior: bev_row, bev_abs, lev_row, lev_abs (dicts by event name), grp_peak_lateral,
           termination_signal_sent, exceed_limits_value, penalty_lin, penalty_sq.
    meas:  f1, f2, f3, ground (force magnitudes, float), palm_mag (Interval), palm_axial_pos
           (max(0, axial), float), peak_lateral_now (float or None when it did not exceed the
           running peak), peak_axial, sensors (dict of the direct sensor events' values),
           obj (x, y, z doubles), start_z, base (x, y, z doubles).
    Returns bev_row, bev_abs, bev_last, lev_row, lev_abs, lev_last, grp_peak_lateral."""
    f1, f2, f3, gnd = F(meas["f1"]), F(meas["f2"]), F(meas["f3"]), F(meas["ground"])
    pm = meas["palm_mag"]
    ox, oy, oz = meas["obj"]
    bx, by, bz = meas["base"]
    dist = F(math.sqrt(math.pow(bx - ox, 2) + math.pow(by - oy, 2)))               # 1011
    lift_height = F(oz - meas["start_z"])                                         # 1024
    avg_finger = F(0.33333 * float(F(F(f1 + f2) + f3)))                           # 1026-1029
    ov_avg = avg_finger if avg_finger > F(0) else F(0)                            # 1052 (obj_values wiped, 1005)
    ov_palm = F(meas["palm_axial_pos"])                                           # 1055
    peak = F(prior["grp_peak_lateral"])
    if meas["peak_lateral_now"] is not None and F(meas["peak_lateral_now"]) > peak:   # 1058
        _t(trace, "peak_lateral:raised")
        peak = F(meas["peak_lateral_now"])
    else:
        _t(trace, "peak_lateral:kept")
    highest_lift = lift_height if lift_height > F(0) else F(0)                    # 1061
    gripper_z_height = F(-1 * bz)                                                 # 1068

    V = {n: False for n in binary_events}
    V["exceed_limits"] = bool(prior["exceed_limits_value"])
    V["step_num"] = True
    closest = float(dist)
    lifted = oob = l2h = th = stable = False
    if float(gnd) < FTOL and 0.0 < FTOL:                                          # 1155-1156
        V["lifted"] = lifted = True
    _t(trace, "lifted:yes" if lifted else "lifted:no")
    for nm, c in (("x_high", ox > s.oob_distance), ("x_low", ox < -s.oob_distance),
                  ("y_high", oy > s.oob_distance), ("y_low", oy < -s.oob_distance)):
        _t(trace, f"oob:{nm}:{'out' if c else 'in'}")
        if c:
            V["oob"] = oob = True
    if float(highest_lift) > s.lift_height - FTOL and lifted and not oob:         # 1169
        V["lifted_to_height"] = l2h = True
    _t(trace, "lifted_to_height:yes" if l2h else "lifted_to_height:no")
    if l2h:
        if float(gripper_z_height) > s.gripper_target_height - FTOL:              # 1176
            V["target_height"] = th = True
        _t(trace, "target_height:yes" if th else "target_height:no")
    if float(f1) > FTOL or float(f2) > FTOL or float(f3) > FTOL or pm.gt(FTOL):   # 1183
        V["object_contact"] = True
    sf, sfl = s.stable_finger_force, s.stable_finger_force_lim
    if (float(f1) > sf and float(f2) > sf and float(f3) > sf and float(f1) < sfl and float(f2) < sfl and float(f3) < sfl
            and pm.gt(s.stable_palm_force) and pm.lt(s.stable_palm_force_lim) and V["lifted"]):   # 1192
        V["object_stable"] = stable = True
    _t(trace, "object_stable:yes" if stable else "object_stable:no")
    if stable and th:
        V["stable_height"] = True
        _t(trace, "stable_height:yes")
    if prior["termination_signal_sent"]:                                          # 1212
        if s.lifted_termination.done:
            V["lifted_termination" if l2h else "failed_termination"] = True
            _t(trace, "terminated:lifted" if l2h else "terminated:failed_not_lifted")
        else:
            V["stable_termination" if V["stable_height"] else "failed_termination"] = True
            _t(trace, "terminated:stable" if V["stable_height"] else "terminated:failed_not_stable")
    within = float(dist) < s.XY_distance_threshold                               # 1237
    _t(trace, "within_XY:yes" if within else "within_XY:no")
    if within:
        V["within_XY_distance"] = True
    R = prior["bev_row"]
    if (not R["dropped"]) * (not V["lifted"]) * R["lifted"]:                      # 1249-1255
        d = 1; _t(trace, "dropped:first")
    elif V["lifted"]:
        d = 0; _t(trace, "dropped:lifted_again")
    elif R["dropped"]:
        d = R["dropped"] + 1; _t(trace, "dropped:continues")
    else:
        d = 0; _t(trace, "dropped:never_lifted")
    V["dropped"] = bool(d)                                                        # the event's value is a bool

    L = dict(meas["sensors"])                                                     # 1279-1286
    L["exceed_axial"] = F(meas["peak_axial"])
    L["exceed_lateral"] = peak
    L["palm_force"] = F(ov_palm * F(V["lifted"]))                                 # 1268
    L["exceed_palm"] = ov_palm
    if ov_palm > F(0):
        _t(trace, "palm:pressed_lifted" if V["lifted"] else "palm:pressed_not_lifted")
    L["finger_force"] = ov_avg
    L["finger1_force"], L["finger2_force"], L["finger3_force"], L["ground_force"] = f1, f2, f3, gnd
    div = F(n_actions - s.use_termination_action)                                 # 1289-1290
    L["action_penalty_lin"] = F(F(prior["penalty_lin"]) / div)
    L["action_penalty_sq"] = F(F(prior["penalty_sq"]) / div)
    L["object_XY_distance"] = F(-closest)
    L.setdefault("grasp_metric", F(0))                                            # never assigned

    for n in binary_events:                                                       # 1305-1320
        b = getattr(s, n)
        if V[n] and b.reward >= (1.0 - 1e-5) and b.done:
            hit = R[n] + 1 >= b.trigger
            _t(trace, f"success_macro:{'triggered' if hit else 'row_short'}")
            if hit:
                V["successful_grasp"] = True

    out = dict(bev_row={}, bev_abs={}, bev_last={}, lev_row={}, lev_abs={}, lev_last={}, grp_peak_lateral=peak)
    for n in binary_events:                                                       # 5443-5449
        v = int(V[n])
        out["bev_row"][n] = R[n] * v + v
        out["bev_abs"][n] = prior["bev_abs"][n] + v
        out["bev_last"][n] = v
        if R[n] and not v:
            _t(trace, "row:binary_reset")
    for n in linear_events:                                                       # 5451-5461
        l = getattr(s, n)
        val = F(L[n])
        active = bool(val > F(l.min) and (val < F(l.overshoot) or F(l.overshoot) < 0))
        if not val > F(l.min):
            _t(trace, "active:not_above_min")
        elif F(l.overshoot) < 0:
            _t(trace, "active:no_overshoot")
        else:
            _t(trace, "active:under_overshoot" if active else "active:past_overshoot")
        if prior["lev_row"][n] and not active:
            _t(trace, "row:linear_reset")
        out["lev_row"][n] = prior["lev_row"][n] * active + active
        out["lev_abs"][n] = prior["lev_abs"][n] + active
        out["lev_last"][n] = val
    return out


# ---------------------------------------------------------------- is_done, reward
def is_done(s, bev_row, lev_row, cumulative_reward, binary_events, linear_events, trace=None):
    """mjclass.cpp:1632-1698."""
    for n in binary_events:
        e = getattr(s, n)
        if e.done and bev_row[n] >= e.done:
            _t(trace, f"done:binary:{'first' if e.done == 1 else 'count'}")
            return True
        if e.done > 1 and bev_row[n]:
            _t(trace, "done:binary:count_short")
    for n in linear_events:
        e = getattr(s, n)
        if e.done and lev_row[n] >= e.done:
            _t(trace, f"done:linear:{'first' if e.done == 1 else 'count'}")
            return True
        if e.done > 1 and lev_row[n]:
            _t(trace, "done:linear:count_short")
    if s.cap_reward and s.quit_if_cap_exceeded:
        c = float(F(cumulative_reward))
        if c - FTOL < float(F(s.reward_cap_lower_bound)):
            _t(trace, "done:lower_cap")
            return True
        if c + FTOL > float(F(s.reward_cap_upper_bound)):
            _t(trace, "done:upper_cap")
            return True
        _t(trace, "done:inside_caps")
    elif s.quit_if_cap_exceeded:
        _t(trace, "done:quit_without_cap")
    return False


def reward(s, bev_row, lev_row, lev_last, cumulative_reward, binary_events, linear_events, trace=None, wide=False):
    """calc_rewards (mjclass.cpp:5471-5528) then reward()'s caps (3025-3043).  Returns
    (transition reward, new cumulative reward).  wide=True evaluates the same expressions in
    Python floats (the f32 / f64 difference bounds a result that cannot be bit-equal)."""
    T = float if wide else F
    r = T(0)
    for n in binary_events:
        e = getattr(s, n)
        if bev_row[n] >= e.trigger:
            _t(trace, "reward:binary")
            r = T(r + T(e.reward))
        elif bev_row[n]:
            _t(trace, "reward:binary_trigger_short")
    for n in linear_events:
        e = getattr(s, n)
        if lev_row[n] >= e.trigger:
            fraction = linear_reward(lev_last[n], e.min, e.max, e.overshoot, trace)
            if wide:
                fraction = _linear_wide(lev_last[n], e.min, e.max, e.overshoot)
            r = T(r + T(T(e.reward) * T(fraction)))
        elif lev_row[n]:
            _t(trace, "reward:linear_trigger_short")
    c = T(T(cumulative_reward) + r)
    lo, hi = T(F(s.reward_cap_lower_bound)), T(F(s.reward_cap_upper_bound))
    if c < lo:
        if s.cap_reward:
            _t(trace, "cap:lower_clipped")
            r = T(r + T(lo - c))
            c = lo
        else:
            _t(trace, "cap:lower_off")
    if c > hi:
        if s.cap_reward:
            _t(trace, "cap:upper_clipped")
            r = T(r + T(hi - c))
            c = hi
        else:
            _t(trace, "cap:upper_off")
    return r, c


def _linear_wide(val, mn, mx, overshoot):
    val, mn, mx, overshoot = float(F(val)), float(F(mn)), float(F(mx)), float(F(overshoot))
    if val < mn:
        return 0.0
    if val > mx:
        if overshoot < mx:
            return 1.0
        if val > overshoot:
            return 0.0
        mn, mx, val = 0.0, overshoot - mx, overshoot - val
    return (val - mn) / (mx - mn)
