"""Crafted states for the env-step readout (test infrastructure only).

The physics half of the env-step is pinned elsewhere; this table reaches the branches of the
lane-0 half -- set_action, sense_gripper_state, update_env, is_done, reward -- that the grasp
rollouts never reach.  Every case is one env: the oracle's reset record for a sphere, edited
through env_state_view (object pose, targets, prior event rows, prior cumulative reward), and
an action.  Cases are grouped in batches, one per settings variant, N = 8 fingers, at most 64
envs each.  Every case names the branches of tests/readout_model.py's trace it is there for.

Object poses: "float" puts the sphere 3 m up over the gripper's axis (it touches nothing for
the 3 S substeps of a termination lift and more: ground force exactly 0, so `lifted`, and
through start_qpos `lifted_to_height`); "ground" leaves it resting where it was spawned.

The batches:

  chain        canonical, stable_finger_force = stable_palm_force = -1 (a floating object is
               `stable`), stable_height trigger 5, oob done 3, lifted trigger 3, ground_force
               done 2: the event chain, oob's four comparisons, within_XY, the dropped
               ternary, counts
  blocked      chain with stable_palm_force_lim < 0: the chain stops at object_stable
  term_stable  chain + the termination action, continuous, lifted_termination.done 0,
               lift_on_termination 0: the threshold at 0.9f, stable / failed termination,
               fractions outside [-1, 1]
  term_lifted  lifted_termination.done 1, lift_on_termination 1
  discrete     discrete actions, every action kind in use and the termination action: every
               code once, every target limit pushed outward and inward, the fingertip minimum
  caps         cap_reward with bounds +-0.05, step_num -0.01, lifted +0.03
  caps_quit    caps with quit_if_cap_exceeded (two env-steps)
  quit_nocap   cap_reward 0 with quit_if_cap_exceeded
  linear       linear_reward's five branches on ground_force (objects of four masses, trigger
               0 so the inactive branches are evaluated) and object_XY_distance, the active
               rule, exceed_lateral's running peak
  grasp        five states of one grasp-lift-hold episode of the oracle (a 3 cm sphere: first
               touch on the ground, carried, squeezed, held, the palm pressed on): the five
               branches again on finger1/2/3_force, ground_force and palm_force with their own
               min / max / overshoot, constants chosen from the oracle's forces in those states
  sensors_all  every sensor in use (29 streams); sensors_one: base_state_sensor_Z alone
"""
from __future__ import annotations

import ctypes as C
import math
import sys

import numpy as np

import contact_cases as cc
import oracle_lib as ol
import readout_model as rm

F = np.float32
FLOAT_Z = 3.0
SPH = cc.SPH


def config_view(gm, cfg):
    """A ConfigBlob read as gm_config (include/gripper_mi355x.h)."""
    n_codes = 3 * len(gm.ACTION_KINDS) + 1

    class Config(C.Structure):
        _fields_ = [("s", gm.Settings), ("n_actions", C.c_int32), ("action_options", C.c_int32 * n_codes),
                    ("sensor_fcn", C.c_int32), ("state_fcn", C.c_int32), ("sensor_fcn_state_override", C.c_int32),
                    ("sim_steps_per_action", C.c_int32), ("n_obs", C.c_int32), ("timestep", C.c_double),
                    ("sim_gauge_raw_to_N_factor", C.c_double), ("base_min", C.c_double * 6), ("base_max", C.c_double * 6)]
    assert C.sizeof(Config) == len(cfg.buf), (C.sizeof(Config), len(cfg.buf))
    return Config.from_buffer(cfg.buf)


class Case:
    def __init__(self, name, branches, pose="ground", xy=(0.0, 0.0), mass=0.1, radius=0.02, cont=None, disc=None,
                 base=None, end=None, rows=None, lrows=None, cum=None, peak=None, pending_exceed=None, palm=(0.0, 0.0), record=None):
        self.name, self.branches = name, tuple(branches)
        self.pose, self.xy, self.mass, self.radius, self.record = pose, xy, mass, radius, record
        self.cont, self.disc = cont, disc
        self.base, self.end, self.palm = base or {}, end, palm      # palm: bounds of its force magnitude, None: from its axial part
        self.rows, self.lrows, self.cum, self.peak, self.pending_exceed = rows or {}, lrows or {}, cum, peak, pending_exceed


class Batch:
    def __init__(self, name, settings, cases, steps=1):
        self.name, self.settings, self.cases, self.steps = name, settings, cases, steps
        self.discrete = not settings.continous_actions
        assert len(cases) <= 64


# ---------------------------------------------------------------- settings variants
def canon(gm):
    """The canonical settings with the two sensor events whose ramp starts at 0 N moved to
    -0.5 N: an untouched gauge reads 0 but for rounding, and no case may hang on that."""
    s = gm.canonical_settings(noise=False, seed=3)
    s.good_bend_sensor.min = -0.5
    s.good_palm_sensor.min = -0.5
    return s


def s_chain(gm):
    s = canon(gm)
    s.stable_finger_force = -1.0
    s.stable_palm_force = -1.0
    s.stable_height.trigger = 5
    s.oob.done = 3
    s.lifted.trigger = 3
    s.ground_force.done = 2
    s.ground_force.min = 0.5           # a resting 0.1 kg sphere presses with 0.98 N, a floating one with exactly 0
    return s


def s_blocked(gm):
    s = s_chain(gm)
    s.stable_palm_force_lim = -0.5
    return s


def s_term_stable(gm):
    s = s_chain(gm)
    s.stable_height.trigger = 1
    s.stable_height.done = 0
    s.use_termination_action = 1
    s.lift_on_termination = 0
    for n, r in (("stable_termination", 1.0), ("lifted_termination", 1.0), ("failed_termination", -1.0)):
        e = getattr(s, n)
        e.reward, e.done, e.trigger = r, 1, 1
    s.lifted_termination.done = 0
    return s


def s_term_lifted(gm):
    s = s_term_stable(gm)
    s.lifted_termination.done = 1
    s.lift_on_termination = 1
    return s


def s_discrete(gm):
    s = s_term_stable(gm)
    s.continous_actions = 0
    for n in gm.ACTION_KINDS:
        a = getattr(s, n)
        a.in_use = 1
        if a.value == 0.0:
            a.value = 0.01 if n in ("base_roll", "base_pitch") else 0.002
    return s


def s_caps(gm, cap=1, quit_=0):
    s = canon(gm)
    for n in gm.BINARY_EVENTS + gm.LINEAR_EVENTS:
        getattr(s, n).reward = 0.0
    s.step_num.reward = -0.01
    s.lifted.reward = 0.03
    s.cap_reward, s.quit_if_cap_exceeded = cap, quit_
    s.reward_cap_lower_bound, s.reward_cap_upper_bound = -0.05, 0.05
    return s


LIN_GROUND = (1.0, 2.0, 4.0)            # ground_force min, max, overshoot: the resting spheres weigh 0.49 .. 4.9 N
LIN_MASSES = (0.05, 0.15, 0.3, 0.5)


def s_linear(gm):
    s = canon(gm)
    for n in gm.BINARY_EVENTS + gm.LINEAR_EVENTS:
        getattr(s, n).reward = 0.0
    g = s.ground_force
    g.reward, g.done, g.trigger, (g.min, g.max, g.overshoot) = 0.1, 0, 0, LIN_GROUND
    p = s.palm_force
    p.reward, p.done, p.trigger, p.min, p.max, p.overshoot = 0.05, 0, 0, 1.0, 3.0, 6.0     # the reference's defaults
    d = s.object_XY_distance
    d.reward, d.done, d.trigger, d.min, d.max = 0.05, 0, 1, -0.2, -5e-3        # overshoot stays -1
    e = s.exceed_lateral
    e.reward, e.done, e.trigger, e.min, e.max = -0.05, 0, 1, -2.0, 1.0
    return s


GRASP_RADIUS, GRASP_SEED = 0.03, 5
# the oracle's finger forces in the five states: 0.0227 (on the ground, 0.948 N left on it),
# 0.571, 0.836 / 0.856 / 0.856, 1.563 / 1.565 / 1.565, 1.767 with 2.57 N on the palm
GRASP_STEPS = (36, 39, 42, 51, 88)
GRASP_LINEAR = {"finger1_force": (0.1, 0, 0.1, 0.7, 1.2), "finger2_force": (0.1, 1, 0.1, 0.5, -1.0),
                "finger3_force": (-0.1, 1, 0.5, 1.0, 1.7), "ground_force": (0.05, 1, 0.5, 0.9, -1.0),
                "palm_force": (0.05, 1, 1.0, 3.0, 6.0)}       # reward, trigger, min, max, overshoot


def s_grasp(gm):
    s = canon(gm)
    for n, (r, trig, mn, mx, ov) in GRASP_LINEAR.items():
        e = getattr(s, n)
        e.reward, e.done, e.trigger, e.min, e.max, e.overshoot = r, 0, trig, mn, mx, ov
    # the palm's magnitude is known from below only: limits that any magnitude is inside
    s.stable_palm_force, s.stable_palm_force_lim = -1.0, math.inf
    return s


def grasp_cases(gm, sc, s):
    """The records before env-steps GRASP_STEPS of the grasp program on the oracle (one centred
    sphere), each with the program's action for that step."""
    cfg = gm.ConfigBlob(s, sc.model)
    objs = (gm._lib.Object * 1)()
    objs[0].type, objs[0].mass, objs[0].friction = SPH, 0.1, 1.0
    objs[0].size[0] = objs[0].size[1] = objs[0].size[2] = GRASP_RADIUS
    env = ol.OracleEnv(sc.model, cfg, objs, 0)
    sp = gm.Spawn()
    sp.object_index, sp.x, sp.y, sp.zrot = 0, 0.0, 0.0, 0.0
    env.reset(sp)
    want = {36: ("first touch, still on the ground", ("linear:below_min", "linear:saturated", "lifted:no")),
            39: ("carried", ("linear:rising", "lifted:yes")), 42: ("squeezed", ("linear:falling",)),
            51: ("held", ("linear:past_overshoot",)),
            88: ("the palm pressed on", ("palm:pressed_lifted", "active:past_overshoot", "row:linear_reset"))}
    cs = []
    for k in range(max(GRASP_STEPS) + 1):
        a = env.driver_actions(mode=3, seed=GRASP_SEED)
        if k in want:
            cs.append(Case(f"grasp program, step {k}: {want[k][0]}", want[k][1], radius=GRASP_RADIUS, cont=a.copy(),
                           record=env.export_state(), palm=None))
        env.set_action(a)
        env.action_step()
        env.is_done()
        env.reward()
    return cs


def s_sensors(gm, only=None):
    s = canon(gm)
    for n in gm.SENSORS:
        getattr(s, n).in_use = 1 if only is None else int(n == only)
    return s


# ---------------------------------------------------------------- the table
def chain_cases(s):
    gth = s.gripper_target_height - rm.FTOL
    up, dn = {2: -(gth + 1e-5)}, {2: -(gth - 1e-5)}
    cs = [Case("floating, gripper low", ("lifted:yes", "lifted_to_height:yes", "target_height:no", "object_stable:yes"), "float"),
          Case("floating, gripper 1e-5 under the target height", ("target_height:no",), "float", base=dn),
          Case("floating, gripper 1e-5 over the target height, stable_height row trigger - 2",
               ("target_height:yes", "stable_height:yes", "success_macro:row_short"), "float", base=up, rows={"stable_height": 3}),
          Case("stable_height row trigger - 1", ("success_macro:triggered", "reward:binary"), "float", base=up,
               rows={"stable_height": 4}),
          Case("stable_height row at trigger", ("success_macro:triggered",), "float", base=up, rows={"stable_height": 5}),
          Case("on the ground", ("lifted:no", "lifted_to_height:no", "object_stable:no", "dropped:never_lifted"))]
    d = s.oob_distance
    for nm, ax, sg in (("x_high", 0, 1), ("x_low", 0, -1), ("y_high", 1, 1), ("y_low", 1, -1)):
        for side, off in (("out", 1e-3), ("in", -1e-3)):
            xy = [0.0, 0.0]
            xy[ax] = sg * (d + off)
            cs.append(Case(f"floating 1 mm {side}side oob, {nm}", (f"oob:{nm}:{side}",), "float", xy=tuple(xy)))
    for prior in (1, 2):
        cs.append(Case(f"oob with its row at {prior} (done = 3)", ("done:binary:count" if prior == 2 else "done:binary:count_short",),
                       "float", xy=(d + 1e-3, 0.0), rows={"oob": prior}))
        cs.append(Case(f"lifted with its row at {prior} (trigger = 3)", ("reward:binary" if prior == 2 else "reward:binary_trigger_short",),
                       "float", rows={"lifted": prior}))
    t = s.XY_distance_threshold
    cs.append(Case("floating 1 mm inside the XY distance", ("within_XY:yes",), "float", xy=(t - 1e-3, 0.0)))
    cs.append(Case("floating 1 mm outside the XY distance", ("within_XY:no",), "float", xy=(0.0, t + 1e-3)))
    want = {(0, 3, "ground"): "dropped:first", (0, 0, "ground"): "dropped:never_lifted", (1, 0, "ground"): "dropped:continues",
            (1, 3, "ground"): "dropped:continues", (5, 0, "ground"): "dropped:continues", (5, 3, "ground"): "dropped:continues"}
    for pd in (0, 1, 5):
        for pl in (0, 3):
            for pose in ("ground", "float"):
                cs.append(Case(f"dropped row {pd}, lifted row {pl}, now {pose}", (want.get((pd, pl, pose), "dropped:lifted_again"),),
                               pose, rows={"dropped": pd, "lifted": pl}))
    cs.append(Case("ground_force row 0 (done = 2)", ("done:linear:count_short",), lrows={"ground_force": 0}))
    cs.append(Case("ground_force row 1 (done = 2)", ("done:linear:count",), lrows={"ground_force": 1}))
    cs.append(Case("ground_force row 4, now floating", ("row:linear_reset",), "float", lrows={"ground_force": 4}))
    cs.append(Case("lifted row 3, now on the ground", ("row:binary_reset",), rows={"lifted": 3}))
    cs.append(Case("exceed_limits and action penalties pending from an earlier call", ("exceed_limits:latched",),
                   pending_exceed=1, cont=[0.5, 0.0, -0.25, 0.0]))
    return cs


def blocked_cases(s):
    up = {2: -(s.gripper_target_height - rm.FTOL + 1e-5)}
    return [Case("floating at the target height, palm limit below 0", ("object_stable:no", "target_height:yes"), "float", base=up)]


T09 = F(0.9)
T09_NEXT = np.nextafter(T09, F(1))


def term_cases(s, lifted):
    up = {2: -(s.gripper_target_height - rm.FTOL + 1e-5)}
    lift = ("termination:lift",) if s.lift_on_termination else ("termination:no_lift",)
    good = "terminated:lifted" if lifted else "terminated:stable"
    bad = "terminated:failed_not_lifted" if lifted else "terminated:failed_not_stable"
    cs = [Case("termination fraction 0.9f", ("termination:below_threshold",), "float", base=up, cont=[0, 0, 0, 0, T09]),
          Case("termination fraction next above 0.9f", ("termination:triggered", good) + lift, "float", base=up,
               cont=[0, 0, 0, 0, T09_NEXT]),
          Case("termination fraction 1", ("termination:triggered", good), "float", base=up, cont=[0.5, -0.25, 0.125, 0, 1.0]),
          Case("termination on the ground", (bad,), cont=[0, 0, 0, 0, 1.0]),
          Case("fractions outside [-1, 1]", ("fraction:clipped_low", "fraction:clipped_high"), cont=[1.5, -2.0, 3.0, -1.25, 7.0])]
    return cs


def home():
    g = rm.Gripper(134e-3 - 4e-3, 134e-3 - 4e-3, 4.8768e-3, 0.0)       # xy_home, z_home (gripper.h:51-52)
    g.update_xy(); g.update_z()
    return g


def discrete_cases(s):
    opts = rm.action_options(s)
    cs = []
    for i, code in enumerate(opts):
        nm = "termination" if code == rm.TERMINATION else f"{rm.ACTION_NAMES[code // 3]} {'+-'[code % 3]}"
        br = ("termination:triggered",) if code == rm.TERMINATION else \
            (f"code:{rm.ACTION_NAMES[code // 3]}:{('positive', 'negative')[code % 3]}",)
        cs.append(Case(f"discrete code {nm} from home", br, "float", disc=i))

    def code(name, sub):
        return opts.index(3 * rm.ACTION_NAMES.index(name) + sub)

    def outward(name, sub, is_max):
        a = getattr(s, name)
        return (a.sign * a.value * (1 if sub == rm.POSITIVE else -1) > 0) == is_max
    G = rm.Gripper
    th40 = 40 * G.to_rad * (1 - 1e-9)              # a hair inside: asin(sin(th)) must not round past the limit
    h = home()
    ends = [("x_max", "gripper_prismatic_X", (G.xy_max, 0.0, h.z)), ("x_min", "gripper_prismatic_X", (G.xy_min, 0.0, h.z)),
            ("th_max", "gripper_revolute_Y", (0.09, th40, h.z)), ("th_min", "gripper_revolute_Y", (0.09, -th40, h.z)),
            ("y_max", "gripper_Y", (G.xy_max - 0.01, None, h.z)), ("y_min", "gripper_Y", (G.xy_min + 0.01, None, h.z)),
            ("z_max", "gripper_Z", (h.x, 0.0, G.z_max)), ("z_min", "gripper_Z", (h.x, 0.0, G.z_min))]
    for lim, act, (x, th, z) in ends:
        g = rm.Gripper(x, x, z, 0.0)
        if th is None:                                   # y at its own leadscrew limit, x 1 cm inside
            g.y = G.xy_max if lim == "y_max" else G.xy_min
        else:
            g.y = g.calc_y(th)
        assert g.update_xy() and g.update_z(), lim
        for sub in (rm.POSITIVE, rm.NEGATIVE):
            out = outward(act, sub, lim.endswith("max"))
            cs.append(Case(f"gripper at {lim}, {act} {'+-'[sub]} ({'outward' if out else 'inward'})",
                           (f"limit:{lim}", "exceed_limits:set") if out else (), "float", disc=code(act, sub), end=g))
    # within limit_tol past a leadscrew limit nothing is clamped: the reading is outside [-1, 1]
    for lim, x in (("max", G.xy_max - 1.95e-3), ("min", G.xy_min + 1.95e-3)):
        g = rm.Gripper(x, x, h.z, 0.0)
        assert g.update_xy() and g.update_z()
        for sub in (rm.POSITIVE, rm.NEGATIVE):
            cs.append(Case(f"gripper x 1.95 mm from its {lim}, gripper_prismatic_X {'+-'[sub]}", (), "float",
                           disc=code("gripper_prismatic_X", sub), end=g))
    for k, (nm, act) in enumerate((("base_x", "base_X"), ("base_y", "base_Y"), ("base_z", "base_Z"), (None, None), (None, None),
                                   ("base_yaw", "base_yaw"))):
        if nm is None:
            continue
        for side, v in (("max", rm.BASE_MAX[k]), ("min", rm.BASE_MIN[k])):
            for sub in (rm.POSITIVE, rm.NEGATIVE):
                out = outward(act, sub, side == "max")
                br = (f"limit:{nm}_{side}", "exceed_limits:set") if out else ()
                if nm == "base_z" and side == "max":         # 3 cm down, 2.8 cm down: the fingertips below their minimum
                    br += ("limit:fingertip_min", "exceed_limits:set")
                cs.append(Case(f"{nm} at its {side}, {act} {'+-'[sub]} ({'outward' if out else 'inward'})", br, "float",
                               disc=code(act, sub), base={k: v}))
    return cs


def caps_cases(s):
    lo, hi = F(s.reward_cap_lower_bound), F(s.reward_cap_upper_bound)
    cs = []
    for nm, c, pose in (("inside the lower bound", -0.03, "ground"), ("crossing the lower bound", -0.045, "ground"),
                        ("at the lower bound", lo, "ground"), ("just inside the lower bound", np.nextafter(lo, F(0)), "ground"),
                        ("inside the upper bound", 0.02, "float"), ("crossing the upper bound", 0.045, "float"),
                        ("at the upper bound", hi, "float"), ("just inside the upper bound", np.nextafter(hi, F(0)), "float")):
        cs.append(Case(nm, (), pose, cum=F(c)))
    return cs


PALM_PEN = 2e-3


def palm_press_radius(sc):
    """Radius of the sphere that rests on the ground under the palm with its top PALM_PEN
    inside the palm's face (the reset pose of the gripper)."""
    (cp, Rp), hp = sc.fk_geoms(sc.q0)[sc.g_palm], sc.gsize[sc.g_palm]
    assert abs(abs(Rp[2, 0]) - 1.0) < 1e-6 and abs(cp[0]) < 1e-6 and abs(cp[1]) < 1e-6      # the face looks straight down
    return 0.5 * (cp[2] - hp[0] + PALM_PEN)


def linear_cases(s, sc):
    cs = []
    for m, br in zip(LIN_MASSES, ("linear:below_min", "linear:rising", "linear:falling", "linear:past_overshoot")):
        cs.append(Case(f"resting sphere of {m} kg", (br,), mass=m, xy=(0.05, 0.0)))
    cs.append(Case("sphere on the axis: XY distance saturated", ("linear:saturated", "active:no_overshoot")))
    # the palm presses a sphere that the ground holds: exceed_palm reads the force, palm_force (* lifted) reads 0
    cs.append(Case("palm pressing a sphere on the ground", ("lifted:no", "palm:pressed_not_lifted"), mass=0.5,
                   radius=palm_press_radius(sc), palm=None))
    cs.append(Case("running lateral peak above this step's", ("peak_lateral:kept",), peak=0.5, xy=(0.05, 0.0)))
    cs.append(Case("running lateral peak below this step's", ("peak_lateral:raised",), peak=-1.0, xy=(0.05, 0.0)))
    return cs


def sensor_cases(s):
    return [Case("on the ground", ()), Case("floating", (), "float", cont=[0.5, -0.5, 0.25, -1.0])]


def make_batches(gm, sc):
    B = []
    s = s_chain(gm); B.append(Batch("chain", s, chain_cases(s)))
    s = s_blocked(gm); B.append(Batch("blocked", s, blocked_cases(s)))
    s = s_term_stable(gm); B.append(Batch("term_stable", s, term_cases(s, False), steps=2))
    s = s_term_lifted(gm); B.append(Batch("term_lifted", s, term_cases(s, True), steps=2))
    s = s_discrete(gm); B.append(Batch("discrete", s, discrete_cases(s)))
    s = s_caps(gm); B.append(Batch("caps", s, caps_cases(s), steps=2))
    s = s_caps(gm, quit_=1); B.append(Batch("caps_quit", s, caps_cases(s), steps=2))
    s = s_caps(gm, cap=0, quit_=1); B.append(Batch("quit_nocap", s, caps_cases(s)[1::4] + [Case("far below", (), cum=F(-1.0))]))
    s = s_linear(gm); B.append(Batch("linear", s, linear_cases(s, sc)))
    s = s_grasp(gm); B.append(Batch("grasp", s, grasp_cases(gm, sc, s)))
    s = s_sensors(gm); B.append(Batch("sensors_all", s, sensor_cases(s)))
    s = s_sensors(gm, "base_state_sensor_Z"); B.append(Batch("sensors_one", s, sensor_cases(s)))
    return B


# ---------------------------------------------------------------- records
def build(gm, sc, batch):
    """cfg, objects, records [n, size] and actions of a batch.  sc: contact_cases.Scene (the
    N = 8 model and the object's qpos address)."""
    cfg = gm.ConfigBlob(batch.settings, sc.model)
    masses = sorted({(c.mass, c.radius) for c in batch.cases})
    objs = (gm._lib.Object * len(masses))()
    for i, (m, r) in enumerate(masses):
        objs[i].type, objs[i].mass, objs[i].friction = SPH, m, 1.0
        objs[i].size[0] = objs[i].size[1] = objs[i].size[2] = r
    recs = []
    be, le = gm.BINARY_EVENTS, gm.LINEAR_EVENTS
    for i, c in enumerate(batch.cases):
        if c.record is not None:                     # a state of a rollout, taken as it is
            assert len(masses) == 1
            recs.append(np.array(c.record, dtype=np.uint8))
            continue
        o = ol.OracleEnv(sc.model, cfg, objs, env_id=i)
        sp = gm.Spawn()
        sp.object_index, sp.x, sp.y, sp.zrot = masses.index((c.mass, c.radius)), float(c.xy[0]), float(c.xy[1]), 0.0
        o.reset(sp)
        rec = o.export_state()[None].copy()
        v = gm.env_state_view(rec)
        if c.pose == "float":
            v["qpos"][0][sc.qadr_obj + 2] = FLOAT_Z
            v["qvel"][0][:] = 0.0
            v["qacc_warm"][0][:] = 0.0
        for k, val in c.base.items():
            v["base"][0][k] = val
        if c.end is not None:
            g = c.end
            for f, val in (("x", g.x), ("y", g.y), ("z", g.z), ("th", g.th), ("sx", g.sx), ("sy", g.sy), ("sz", g.sz)):
                v["end"][f][0] = val
        for n, r in c.rows.items():
            v["bev_row"][0][be.index(n)] = r
            v["bev_abs"][0][be.index(n)] = r
        for n, r in c.lrows.items():
            v["lev_row"][0][le.index(n)] = r
            v["lev_abs"][0][le.index(n)] = r
        if c.cum is not None:
            v["cumulative_reward"][0] = c.cum
        if c.peak is not None:
            v["grp_peak_lateral"][0] = c.peak
        if c.pending_exceed is not None:             # what an earlier set_action call of the same env-step left
            v["bev_value"][0][be.index("exceed_limits")] = c.pending_exceed
            v["lev_value"][0][le.index("action_penalty_lin")] = 0.75
            v["lev_value"][0][le.index("action_penalty_sq")] = 0.5625
        recs.append(rec[0])
    recs = np.ascontiguousarray(np.stack(recs))
    na = cfg.n_actions
    if batch.discrete:
        acts = np.array([c.disc for c in batch.cases], dtype=np.int32)
    else:
        acts = np.zeros((len(batch.cases), na), dtype=np.float32)
        for i, c in enumerate(batch.cases):
            if c.cont is not None:
                acts[i] = np.asarray(c.cont, dtype=np.float32)
    return cfg, objs, recs, acts


# ---------------------------------------------------------------- the model on a record
def model_step(gm, sc, batch, cfg, before, after, action, trace=None, palm=(0.0, 0.0)):
    # palm None: the magnitude is at least its axial component, and nothing more is known
    """The model's answer for one env: the prior tracker state and targets from the record
    before the step, the action, and the measured quantities from the record after it.
    before / after: one-element env_state_view rows."""
    s = batch.settings
    be, le = gm.BINARY_EVENTS, gm.LINEAR_EVENTS
    e = before["end"]
    tg = rm.Target(rm.Gripper(e["x"], e["y"], e["z"], e["th"], trace), before["base"],
                   before["bev_value"][be.index("exceed_limits")],
                   before["lev_value"][le.index("action_penalty_lin")], before["lev_value"][le.index("action_penalty_sq")])
    tg.end.sx, tg.end.sy, tg.end.sz = int(e["sx"]), int(e["sy"]), int(e["sz"])
    fl = float(sc.model.params.finger_length)
    if batch.discrete:
        rm.set_actions(tg, s, fl, cfg.sim_steps_per_action, discrete=int(action), trace=trace)
    else:
        rm.set_actions(tg, s, fl, cfg.sim_steps_per_action, continuous=action, trace=trace)
    ll = {n: F(after["lev_last"][k]) for k, n in enumerate(le)}
    prior_peak = F(before["grp_peak_lateral"])
    now = ll["exceed_lateral"]
    sensors = {n: ll[n] for n in le if n.endswith("_sensor")}
    qa = sc.qadr_obj
    meas = dict(f1=ll["finger1_force"], f2=ll["finger2_force"], f3=ll["finger3_force"], ground=ll["ground_force"],
                palm_mag=rm.Interval(*palm) if palm is not None else rm.Interval(ll["exceed_palm"], sys.float_info.max), palm_axial_pos=ll["exceed_palm"],
                peak_lateral_now=None if now.tobytes() == prior_peak.tobytes() else now, peak_axial=ll["exceed_axial"],
                sensors=sensors, obj=tuple(float(x) for x in after["qpos"][qa:qa + 3]), start_z=float(before["start_qpos"][2]),
                base=tuple(tg.base[:3]))
    prior = dict(bev_row={n: int(before["bev_row"][k]) for k, n in enumerate(be)},
                 bev_abs={n: int(before["bev_abs"][k]) for k, n in enumerate(be)},
                 lev_row={n: int(before["lev_row"][k]) for k, n in enumerate(le)},
                 lev_abs={n: int(before["lev_abs"][k]) for k, n in enumerate(le)},
                 grp_peak_lateral=prior_peak, termination_signal_sent=tg.termination_signal_sent,
                 exceed_limits_value=tg.exceed_limits_value, penalty_lin=tg.penalty_lin, penalty_sq=tg.penalty_sq)
    n_actions = len(rm.action_options(s))
    out = rm.update_env(prior, s, n_actions, meas, be, le, trace)
    out["done"] = rm.is_done(s, out["bev_row"], out["lev_row"], before["cumulative_reward"], be, le, trace)
    out["reward"], out["cumulative_reward"] = rm.reward(s, out["bev_row"], out["lev_row"], out["lev_last"],
                                                        before["cumulative_reward"], be, le, trace)
    out["reward_wide"], _ = rm.reward(s, out["bev_row"], out["lev_row"], out["lev_last"], before["cumulative_reward"], be, le,
                                      None, wide=True)
    out["target"] = tg
    out["state_readings"] = rm.state_readings(tg, trace)
    return out


TH_ULPS = 2


def same_angle(a, b, ulps):
    """The cached finger angle is asin((y - x) / leadscrew) of the same bits on every side, by
    each side's own math library (glibc for the reference, the oracle and the model; the HIP
    device library on the device), each within 1 ulp of the exact value: device values may
    differ from the others by TH_ULPS = 2 ulps, host values by none."""
    return abs(a - b) <= ulps * np.spacing(max(abs(a), abs(b)))


def compare_with_model(gm, out, after, who, th_ulps=0):
    """Bit for bit: rows, abs counts, last values, done, reward, cumulative reward, the
    targets and their step counts, termination_signal_sent, the seven state readings; the
    cached finger angle within th_ulps (same_angle)."""
    be, le = gm.BINARY_EVENTS, gm.LINEAR_EVENTS
    for f in ("bev_row", "bev_abs", "bev_last"):
        got = {n: int(after[f][k]) for k, n in enumerate(be)}
        assert got == out[f], f"{who}: {f} {[(n, got[n], out[f][n]) for n in be if got[n] != out[f][n]]}"
    for f in ("lev_row", "lev_abs"):
        got = {n: int(after[f][k]) for k, n in enumerate(le)}
        assert got == out[f], f"{who}: {f} {[(n, got[n], out[f][n]) for n in le if got[n] != out[f][n]]}"
    for k, n in enumerate(le):
        a, b = F(after["lev_last"][k]), F(out["lev_last"][n])
        assert a.tobytes() == b.tobytes(), f"{who}: lev_last[{n}] {a!r} vs model {b!r}"
    assert int(after["done"]) == int(out["done"]), f"{who}: done {int(after['done'])} vs model {out['done']}"
    r, c = F(after["reward"]), F(after["cumulative_reward"])
    assert r.tobytes() == F(out["reward"]).tobytes(), f"{who}: reward {r!r} vs model {out['reward']!r}"
    assert c.tobytes() == F(out["cumulative_reward"]).tobytes(), f"{who}: cumulative {c!r} vs model {out['cumulative_reward']!r}"
    assert F(after["grp_peak_lateral"]).tobytes() == F(out["grp_peak_lateral"]).tobytes(), f"{who}: grp_peak_lateral"
    tg = out["target"]
    e = after["end"]
    for f, val in (("x", tg.end.x), ("y", tg.end.y), ("z", tg.end.z)):
        assert float(e[f]) == val, f"{who}: end.{f} {float(e[f])!r} vs model {val!r}"
    assert same_angle(float(e["th"]), tg.end.th, th_ulps), f"{who}: end.th {float(e['th'])!r} vs model {tg.end.th!r}"
    for f, val in (("sx", tg.end.sx), ("sy", tg.end.sy), ("sz", tg.end.sz)):
        assert int(e[f]) == val, f"{who}: end.{f} {int(e[f])} vs model {val}"
    assert [float(x) for x in after["base"]] == tg.base, f"{who}: base {after['base']} vs model {tg.base}"
    assert int(after["termination_signal_sent"]) == int(tg.termination_signal_sent), f"{who}: termination_signal_sent"
    ri = after["ring_i"]
    for j, st in enumerate((10, 11, 12, 13, 14, 15, 16)):           # ST_MOTOR x y z, ST_BASE x y z, ST_YAW (gm_state.h)
        got = F(after["ring"][st][ri[st]])
        assert got.tobytes() == F(out["state_readings"][j]).tobytes(), \
            f"{who}: state reading {j} {got!r} vs model {out['state_readings'][j]!r}"


def margin_ok(value, threshold):
    """|value - threshold| clear of a relative 1e-4, floored at 1e-6 absolute."""
    return abs(float(value) - float(threshold)) > max(1e-4 * abs(float(threshold)), 1e-6)
