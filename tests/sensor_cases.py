"""Crafted states for the sensor stage (test infrastructure only).

The sensor stage is the third part of the env-step's lane-0 logic: the per-env generator,
the readiness test and its cached minimum (next_sensor_read), normalisation, noise, the
bending gauge, monitor_sensors, the noise half of sense_gripper_state, the mean draws of a
reset and the seven window samplers.  tests/sensor_model.py restates it from the reference's
text; this table reaches what the grasp rollouts and the canonical settings never do.

Every case is one env: the oracle's reset record of a sphere, edited through env_state_view
(time, last_read, rng, rand_mu, the windows and their indices, the finger joints, the
targets).  Cases are grouped in batches, one per settings variant, N = 8 fingers, at most 64
envs and at most 3 env-steps each.  Every crafted number comes from the model.

The batches (`kind`: "step" = env-steps through action_step, "substep" = one substep,
"reset" = a reset from a crafted generator state):

  rates, rates_bend, rates_axial, rates_palm
               bending / axial / palm / wrist Z at 10 / 25 / 7 / 50 Hz, and with each of the
               other three in turn at 50 Hz; 3 env-steps: every sensor's append count and
               last_read against a readiness test made after every substep
  ready_edge   10 Hz; per sensor, last_read + (double)(1 / rate) equal to the new time, one
               ulp under it, one ulp over it: not read, read, not read.  The equal case comes
               twice: alone (monitor_sensors is not called at all) and with another sensor
               overdue (it is called, and the strict > decides)
  uniform_small, uniform_big
               uniform noise of magnitude 0.05 / 0.5 on the bending gauge and the motor state
               sensor, crafted means; with 0.5 and readings at +-1 the clamp on each side
  gauss_edges  Gaussian noise (std 0.025), the generator crafted so that the first u1 is
               rejected (outputs 2 and 257), is the first accepted (258), takes the
               distribution's >= 1 guard (2147483585) or is the last that does not
               (2147483584), so that u2 is 0, 1/4, 1/2, 3/4 of the range, and a reading of 1
               with a positive mean and u2 = 0 (the clamp)
  switches_a, switches_b
               use_noise 0, use_normalisation 0, normalise 0 and -1 (the bumper rule, on
               wrist Z with raw_value_offset +3 and -3), palm_scale_factor 2.5, an overridden
               sensor next to shared parameters that differ
  means        sensor_noise_mu 0.05, state_noise_mu 0.025, base_state_sensor_Z and the
               bending gauge overridden: rand_mu [10][3] and the stream after a reset
  ring64_m0 .. ring64_m6, ring64_median64, ring64_median_odd
               bending gauge and palm sensor at 105 Hz (21 readings per env-step, a window of
               exactly 64), every sampler; 315 Hz with one previous step (the median of 64
               values); 100 Hz (the median of 21); ring_i -1, 0, 1, 62, 63 on a ramp
  thresholds_m0 .. thresholds_m6
               sensor and state sample mode m (m = 6: the state streams keep sign_sample),
               windows written directly: changes of 0 and of the floats just under, at and
               just over 1e-6f, 0.07f, 0.10f, both signs
  gauge        joint angles written into qpos, the object 3 m up: straight, uniform
               curvature of both signs, an S, one joint bent alone (first, middle, last),
               0.25 rad per joint
"""
from __future__ import annotations

import numpy as np

import contact_cases as cc
import oracle_lib as ol
import readout_cases as rc
import readout_model as rm
import sensor_model as sm
from gmx.settings import set_gaussian_noise

F = np.float32
SPH = cc.SPH
FLOAT_Z = rc.FLOAT_Z
MONITORED = ("bending_gauge", "axial_gauge", "palm_sensor", "wrist_sensor_Z")
ALL_STREAMS = tuple(range(0, 37))


class Case:
    def __init__(self, name, branches=(), pose="ground", mass=0.1, radius=0.02, edit=None, cont=None, palm_press=False):
        self.name, self.branches, self.pose, self.mass, self.radius = name, tuple(branches), pose, mass, radius
        self.edit, self.cont, self.palm_press = edit, cont, palm_press


class Batch:
    def __init__(self, name, settings, cases, kind="step", steps=1, gauss=False, angles=False):
        self.name, self.settings, self.cases, self.kind, self.steps = name, settings, cases, kind, steps
        self.gauss = gauss               # Gaussian draws: those window values are held to the noise bound
        self.angles = angles             # the model derives the gauge readings from the joint angles
        assert len(cases) <= 64 and steps <= 4


# ---------------------------------------------------------------- settings variants
def canon(gm, noise=False):
    s = gm.canonical_settings(noise=noise, seed=3)
    s.good_bend_sensor.min = -0.5
    s.good_palm_sensor.min = -0.5
    return s


def uncalibrated(s):
    """auto_calibrate_gauges off: the gauge's SI window holds the raw reading (factor 1), which
    the model then takes from the record like the axial and palm values; normalise 0.25 mm."""
    s.auto_calibrate_gauges = 0
    s.bending_gauge.normalise = 0.25
    return s


RATES = {"rates": (10.0, 25.0, 7.0, 50.0), "rates_bend": (50.0, 25.0, 7.0, 10.0),
         "rates_axial": (10.0, 50.0, 7.0, 25.0), "rates_palm": (10.0, 25.0, 50.0, 7.0)}


def s_rates(gm, name):
    s = uncalibrated(canon(gm))
    for n, r in zip(MONITORED, RATES[name]):
        getattr(s, n).read_rate = r
    s.axial_gauge.in_use = 1
    return s


def set_uniform_noise(sensor, mag):
    """Sensor::set_uniform_noise (mjclass.h:130-135)."""
    sensor.noise_mag, sensor.noise_mu, sensor.noise_std, sensor.noise_overriden = mag, 0.0, -1.0, 1


def s_uniform(gm, mag):
    s = uncalibrated(canon(gm, noise=True))
    set_uniform_noise(s.bending_gauge, mag)
    set_uniform_noise(s.motor_state_sensor, mag)
    return s


def s_gauss(gm):
    return uncalibrated(canon(gm, noise=True))


def s_switches(gm, variant):
    s = uncalibrated(canon(gm, noise=True))
    s.axial_gauge.in_use = 1
    s.palm_scale_factor = 2.5
    s.base_position_noise = 0.0                                # the palm-press case needs the base where the reset pose has it
    set_gaussian_noise(s.bending_gauge, 0.1, 0.01)          # its own mean and std; the shared ones are 0.05 / 0.025
    if variant == "a":
        s.axial_gauge.use_noise = 0
        s.palm_sensor.use_normalisation = 0
        s.wrist_sensor_Z.normalise = 0.0
        s.wrist_sensor_Z.raw_value_offset = 3.0
    else:
        s.palm_sensor.use_noise = 0
        s.axial_gauge.use_normalisation = 0
        s.wrist_sensor_Z.normalise = -1.0
        s.wrist_sensor_Z.raw_value_offset = -3.0
    return s


def s_means(gm):
    s = canon(gm, noise=True)
    set_gaussian_noise(s.bending_gauge, 0.1, 0.01)
    return s


def s_ring64(gm, mode, rate=105.0, prev=3):
    s = uncalibrated(canon(gm))
    s.sensor_sample_mode = mode
    s.state_sample_mode = mode
    s.sensor_n_prev_steps = prev
    s.bending_gauge.read_rate = rate
    s.palm_sensor.read_rate = rate
    return s


def s_thresholds(gm, mode):
    s = uncalibrated(canon(gm))
    s.sensor_sample_mode = mode
    s.state_sample_mode = mode
    return s


def s_gauge(gm):
    s = canon(gm)
    s.bending_gauge.use_normalisation = 0
    return s


# ---------------------------------------------------------------- edits
def finger_q(sc, f):
    d = sc.model.dof_seg[f]
    return slice(d, d + sc.n_seg)


def still(v):
    v["qvel"][0][:] = 0.0
    v["qacc_warm"][0][:] = 0.0


def overdue(v, slots=MONITORED, by=1.0):
    for n in slots:
        v["last_read"][0][sm.SLOT[n]] = v["time"][0] - by


def pose_fingers(sc, v, shape, scales=(1.0, 0.5, -1.0)):
    for f in range(3):
        v["qpos"][0][finger_q(sc, f)] = np.asarray(shape, dtype=np.float64) * scales[f]
    still(v)


def set_end(v, x, y, z):
    g = rm.Gripper(x, y, z, 0.0)
    assert g.update_xy() and g.update_z()
    for f, val in (("x", g.x), ("y", g.y), ("z", g.z), ("th", g.th), ("sx", g.sx), ("sy", g.sy), ("sz", g.sz)):
        v["end"][f][0] = val


def fill_ramp(v, streams=ALL_STREAMS):
    """Window k of stream st holds (k - 32) / 64 + st / 4096: every value exact in float,
    distinct within a stream and between neighbouring streams."""
    for st in streams:
        v["ring"][0][st][:] = [F((k - 32) / 64.0 + st / 4096.0) for k in range(sm.RING)]


def place(v, st, back, value):
    """Write `value` as the reading `back` appends before the latest of stream st."""
    i = int(v["ring_i"][0][st])
    v["ring"][0][st][(i - back) % sm.RING] = value


# ---------------------------------------------------------------- the cases
def rates_cases():
    return [Case("resting sphere, closing", ("ready:yes", "ready:no"), cont=[0.5, 0.0, 0.0, 0.0]),
            Case("floating sphere, lifting", ("ready:yes",), "float", cont=[0.0, 0.0, 0.0, -1.0]),
            Case("resting sphere, read 30 ms ago", ("ready:no",),
                 edit=lambda sc, v: [v["last_read"][0].__setitem__(sm.SLOT[n], -0.03) for n in MONITORED])]


EDGE_TIME0 = 0.15


def edge_last_read(time1, tbr, which):
    """last_read with last_read + tbr equal to time1 ("equal"), to the double under it
    ("under") or over it ("over"), found by walking doubles from time1 - tbr."""
    want = {"equal": time1, "under": np.nextafter(time1, -np.inf), "over": np.nextafter(time1, np.inf)}[which]
    lr = float(want) - tbr
    for _ in range(64):
        got = lr + tbr
        if got == want:
            return lr
        lr = float(np.nextafter(lr, np.inf if got < want else -np.inf))
    raise AssertionError(f"no last_read with last_read + {tbr!r} == {want!r}")


def ready_edge_cases(dt):
    time1 = EDGE_TIME0 + dt                                     # the oracle's time += dt
    tbr = float(F(F(1) / F(10.0)))
    cs = []
    for n in MONITORED:
        other = MONITORED[(MONITORED.index(n) + 1) % 4]
        for which, alone in (("equal", True), ("equal", False), ("under", True), ("over", True)):
            lr = edge_last_read(time1, tbr, which)
            assert {"equal": lr + tbr == time1, "under": lr + tbr < time1, "over": lr + tbr > time1}[which]
            assert abs((lr + tbr) - time1) <= np.spacing(time1)

            def edit(sc, v, n=n, lr=lr, alone=alone, other=other):
                v["time"][0] = EDGE_TIME0
                v["last_read"][0][:] = EDGE_TIME0
                v["last_read"][0][sm.SLOT[n]] = lr
                if not alone:
                    overdue(v, (other,))
            br = {"equal": ("ready:at_equality",), "under": ("ready:yes",), "over": ("ready:no",)}[which]
            cs.append(Case(f"{n}: due time {which} to the new time{'' if alone else f', {other} overdue'}",
                           br + (() if alone else ("ready:yes",)), edit=edit))
    return cs


BENT = [0.05] * 8               # still over 0.25 mm at the gauge after a substep of springing back: normalised to 1
MU_CRAFTED = 0.02


def uniform_cases():
    G = rm.Gripper
    cs = []
    for pose, shape in (("straight", [0.0] * 8), ("bent out", BENT), ("bent in", [-x for x in BENT])):
        for tgt, x in (("at its maximum", G.xy_max), ("at its minimum", G.xy_min), ("in the middle", 0.09)):
            def edit(sc, v, shape=shape, x=x):
                v["qpos"][0][sc.qadr_obj + 2] = FLOAT_Z
                pose_fingers(sc, v, shape)
                set_end(v, x, x, 0.08 if x == 0.09 else (G.z_max if x == G.xy_max else G.z_min))
                v["next"][0] = v["end"][0]
                overdue(v)
                v["rand_mu"][0][sm.SLOT["bending_gauge"]] = (MU_CRAFTED, -MU_CRAFTED, 0.0)
                v["rand_mu"][0][sm.SLOT["motor_state_sensor"]] = (-MU_CRAFTED, 0.0, MU_CRAFTED)
            cs.append(Case(f"fingers {pose}, motor targets {tgt}", ("noise:uniform_mag",), "float", edit=edit))
    return cs


def gauss_cases():
    M, inv = sm.MINSTD_M, pow(sm.MINSTD_A, -1, sm.MINSTD_M)
    cs = []

    def first(k, name, br, shape=None, mu=None):
        def edit(sc, v):
            v["qpos"][0][sc.qadr_obj + 2] = FLOAT_Z
            pose_fingers(sc, v, shape or [0.0] * 8)
            overdue(v)
            v["rng"][0] = sm.state_before_output(k)
            if mu is not None:
                v["rand_mu"][0][sm.SLOT["bending_gauge"]] = mu
        cs.append(Case(name, br, "float", edit=edit))
    first(2, "first u1 from output 2: rejected", ("noise:gauss_rejected",))
    first(257, "first u1 from output 257: the last rejected", ("noise:gauss_rejected",))
    first(258, "first u1 from output 258: the first accepted", ("noise:gauss",))
    first(2147483585, "first u1 from output 2147483585: rounds to 1, the guard", ("unif:guard",))
    first(2147483584, "first u1 from output 2147483584: the last below the guard", ("noise:gauss",))
    for q, k2 in (("0", 1), ("1/4", (M - 1) // 4 + 1), ("1/2", (M - 1) // 2 + 1), ("3/4", 3 * ((M - 1) // 4) + 1)):
        k1 = (k2 * inv) % M
        assert k1 > 258 and sm.minstd_next(k1) == k2
        first(k1, f"first u2 at {q} of the range", ("noise:gauss",))
    k1 = (1 * inv) % M                                          # u2 = 0: cos = 1, z0 = mag + mu > 0
    first(k1, "reading 1, positive mean, u2 = 0: the clamp", ("noise:clamp_high", "normalise:above"), shape=BENT,
          mu=(0.05, 0.05, 0.05))
    return cs


def switches_cases(sc):
    def floating(sc_, v):
        v["qpos"][0][sc_.qadr_obj + 2] = FLOAT_Z
        still(v)
        overdue(v)
    return [Case("resting sphere", ("noise:off", "normalise:off"), edit=lambda sc_, v: overdue(v)),
            Case("floating sphere", ("noise:off",), "float", edit=floating),
            Case("palm pressing a sphere on the ground", ("normalise:off",), mass=0.5, radius=rc.palm_press_radius(sc),
                 edit=lambda sc_, v: overdue(v), palm_press=True)]


def means_cases():
    def with_rng(state):
        return lambda sc, v: v["rng"].__setitem__(0, state)
    return [Case("generator as the reset left it"),
            Case("generator at 1", edit=with_rng(1)),
            Case("first mean from output 2147483585: the guard", ("unif:guard",), edit=with_rng(sm.state_before_output(2147483585))),
            Case("first mean from output 1: u = 0", edit=with_rng(sm.state_before_output(1))),
            Case("generator at its largest state", edit=with_rng(sm.MINSTD_M - 1))]


RING_I = (-1, 0, 1, 62, 63)


def ring64_cases():
    cs = []
    for ri in RING_I:
        def edit(sc, v, ri=ri):
            fill_ramp(v)
            v["ring_i"][0][:] = ri
            overdue(v)
        cs.append(Case(f"every window index at {ri}", ("window:write_wraps", "window:read_wraps") if ri >= 62 else (), edit=edit))
    return cs


def threshold_values():
    out = [F(0.0)]
    for t in (F(1e-6), F(0.07), F(0.10)):
        for sg in (1, -1):
            out += [F(sg) * np.nextafter(t, F(0)), F(sg) * t, F(sg) * np.nextafter(t, F(1))]
    return out


THRESHOLD_I = 10
SENSOR_STREAMS = (sm.ST_GAUGE, sm.ST_GAUGE + 1, sm.ST_GAUGE + 2, sm.ST_PALM, sm.ST_WZ)      # 10 Hz: two appends per env-step
STATE_STREAMS = (sm.ST_MOTOR, sm.ST_MOTOR + 1, sm.ST_MOTOR + 2, sm.ST_BASE + 2)             # one append per env-step


def thresholds_cases():
    """Three envs.  A sensor stream (readings_per_step 2, 3 previous steps) is sampled at 6, 4,
    2, 0 appends back, two of them new: the readings now 4, 2, 0 back are old and crafted as
    -d1, 0, d2.  A state stream (readings_per_step 1) is sampled at 3, 2, 1, 0 back, one
    new: the readings now 2, 1, 0 back."""
    vals = threshold_values()
    cs = []
    for e in range(3):
        def edit(sc, v, e=e):
            fill_ramp(v)
            v["ring_i"][0][:] = THRESHOLD_I
            v["last_read"][0][:] = v["time"][0] - 0.03          # two readings at 10 Hz in the 0.2 s of the env-step
            for streams, backs in ((SENSOR_STREAMS, (4, 2, 0)), (STATE_STREAMS, (2, 1, 0))):
                for j, st in enumerate(streams):
                    d1 = vals[(2 * (len(streams) * e + j)) % len(vals)]
                    d2 = vals[(2 * (len(streams) * e + j) + 1) % len(vals)]
                    a, b, c = F(-d1), F(0.0), d2                # b - a and c - b are d1 and d2 exactly
                    assert F(b - a).tobytes() == F(d1 + F(0)).tobytes() and F(c - b) == d2
                    for back, x in zip(backs, (a, b, c)):
                        place(v, st, back, x)
        cs.append(Case(f"threshold changes, set {e}", (), edit=edit))
    return cs


GAUGE_SHAPES = (("straight", [0.0] * 8, ()),
                ("uniform curvature, outward", [0.03] * 8, ()),
                ("uniform curvature, inward", [-0.03] * 8, ()),
                ("an S", [0.06, 0.04, 0.02, 0.0, -0.02, -0.04, -0.06, -0.04], ()),
                ("first joint alone", [0.1] + [0.0] * 7, ()),
                ("middle joint alone", [0.0] * 4 + [0.1] + [0.0] * 3, ()),
                ("last joint alone", [0.0] * 7 + [0.1], ()),
                ("0.25 rad per joint", [0.25] * 8, ()))


def gauge_cases():
    cs = []
    for name, shape, br in GAUGE_SHAPES:
        def edit(sc, v, shape=shape):
            v["qpos"][0][sc.qadr_obj + 2] = FLOAT_Z
            pose_fingers(sc, v, shape)
            overdue(v, ("bending_gauge",))
        cs.append(Case(name, br + ("ready:yes", "normalise:off"), "float", edit=edit))
    return cs


def make_batches(gm, sc):
    dt = rc.config_view(gm, sc.cfg).timestep
    B = [Batch(n, s_rates(gm, n), rates_cases(), steps=3, angles=True) for n in RATES]
    B.append(Batch("ready_edge", canon(gm), ready_edge_cases(dt), kind="substep", angles=True))
    B.append(Batch("uniform_small", s_uniform(gm, 0.05), uniform_cases(), gauss=True))
    B.append(Batch("uniform_big", s_uniform(gm, 0.5), uniform_cases(), gauss=True))
    B.append(Batch("gauss_edges", s_gauss(gm), gauss_cases(), steps=2, gauss=True))
    B.append(Batch("switches_a", s_switches(gm, "a"), switches_cases(sc), gauss=True))
    B.append(Batch("switches_b", s_switches(gm, "b"), switches_cases(sc), gauss=True))
    B.append(Batch("means", s_means(gm), means_cases(), kind="reset"))
    B += [Batch(f"ring64_m{m}", s_ring64(gm, m), ring64_cases()) for m in range(7)]
    B.append(Batch("ring64_median64", s_ring64(gm, sm.MEDIAN, 315.0, 1), ring64_cases()))
    B.append(Batch("ring64_median_odd", s_ring64(gm, sm.MEDIAN, 100.0, 3), ring64_cases()))
    B += [Batch(f"thresholds_m{m}", s_thresholds(gm, m), thresholds_cases()) for m in range(7)]
    B.append(Batch("gauge", s_gauge(gm), gauge_cases(), kind="substep", angles=True))
    return B


# ---------------------------------------------------------------- records
def build(gm, sc, batch):
    """cfg, objects, records [n, size], actions and spawn table of a batch."""
    cfg = gm.ConfigBlob(batch.settings, sc.model)
    kinds = sorted({(c.mass, c.radius) for c in batch.cases})
    objs = (gm._lib.Object * len(kinds))()
    for i, (m, r) in enumerate(kinds):
        objs[i].type, objs[i].mass, objs[i].friction = SPH, m, 1.0
        objs[i].size[0] = objs[i].size[1] = objs[i].size[2] = r
    recs = []
    spawn = (gm.Spawn * len(batch.cases))()
    for i, c in enumerate(batch.cases):
        o = ol.OracleEnv(sc.model, cfg, objs, env_id=i)
        sp = spawn[i]
        sp.object_index, sp.x, sp.y, sp.zrot = kinds.index((c.mass, c.radius)), 0.0, 0.0, 0.0
        o.reset(sp)
        rec = o.export_state()[None].copy()
        v = gm.env_state_view(rec)
        if c.pose == "float":
            v["qpos"][0][sc.qadr_obj + 2] = FLOAT_Z
            still(v)
        if c.edit is not None:
            c.edit(sc, v)
        recs.append(rec[0])
    recs = np.ascontiguousarray(np.stack(recs))
    acts = np.zeros((len(batch.cases), cfg.n_actions), dtype=np.float32)
    for i, c in enumerate(batch.cases):
        if c.cont is not None:
            acts[i] = np.asarray(c.cont, dtype=np.float32)
    return cfg, objs, recs, acts, spawn


# ---------------------------------------------------------------- the model on a record
class Setup:
    """What the model needs of a batch beside the records: the sensors as the reference
    configures them, the substep count, the gauge's constants."""

    def __init__(self, gm, sc, batch, cfg):
        c = rc.config_view(gm, cfg)
        s = batch.settings
        self.s, self.dt = s, float(c.timestep)
        self.n_sub = int(np.ceil(s.time_for_action / self.dt))                  # mjclass.cpp:306
        self.time_per_step = self.dt * self.n_sub                               # mjclass.cpp:311
        self.sensors = sm.make_sensors(s, self.time_per_step)
        if s.auto_calibrate_gauges:     # calibration is out of scope: its two results are taken as configured
            self.sensors["bending_gauge"].normalise = F(c.s.bending_gauge.normalise)
            self.sensors["wrist_sensor_Z"].raw_value_offset = F(c.s.wrist_sensor_Z.raw_value_offset)
        self.factor = float(c.sim_gauge_raw_to_N_factor)
        m = sc.m
        self.gauge_args = (float(m.segment_length), bool(m.fixed_first_segment), float(m.gauge_xpos), int(m.gauge_order))
        self.config = c


def windows_of(row, trace=None):
    return {st: sm.Window(row["ring"][st], row["ring_i"][st], trace) for st in ALL_STREAMS}


def samplers_on(setup, row, trace=None):
    """The model's observation of a record's own windows."""
    return np.array(sm.observation(setup.s, setup.sensors, windows_of(row, trace), trace), dtype=np.float32)


def model_run(sc, setup, before, after, kind, angles=None, trace=None, palm_raw=None):
    """The stage from record `before` over one env-step ("step") or one substep ("substep").
    `after` is the record under test: the SI axial and palm values of every reading, and the
    raw gauge reading where the gauge factor is 1, are taken from its SI windows at the slot
    the model is about to write; angles(k) -> the three fingers' joint angles after substep
    k, where the model derives the gauge itself.  Returns the sm.Record."""
    rec = sm.Record(before["time"], before["last_read"], before["rng"], before["rand_mu"], before["ring"], before["ring_i"], trace)
    n = 1 if kind == "substep" else setup.n_sub + int(before["extra_substeps"])
    times = sm.substep_times(float(before["time"]), float(before["dt"]), n)
    cur = [0]

    def slot_value(st):
        return F(after["ring"][st][(rec.w[st].i + 1) % sm.RING])

    def meas(what):
        if what == "gauges":
            if angles is not None:
                q = angles(cur[0])
                return [sm.gauge(q[f], *setup.gauge_args) for f in range(3)]
            assert setup.factor == 1.0
            return [slot_value(sm.ST_SI_GAUGE + f) for f in range(3)]
        if what == "axial":
            return [slot_value(sm.ST_SI_AXIAL + f) for f in range(3)]
        if what == "palm_raw":
            return None if palm_raw is None else palm_raw(rec.w[sm.ST_SI_PALM].i + 1)
        return slot_value(sm.ST_SI_PALM)

    for k, t in enumerate(times):
        cur[0] = k
        sm.monitor_sensors(rec, setup.s, setup.sensors, t, meas, setup.factor, k)
    rec.time = times[-1]
    if kind == "step":
        e, b = after["end"], after["base"]
        G = rm.Gripper
        readings = [rm.normalise_between(e["x"], G.xy_min, G.xy_max), rm.normalise_between(e["y"], G.xy_min, G.xy_max),
                    rm.normalise_between(e["z"], G.z_min, G.z_max)] + \
                   [rm.normalise_between(b[k], rm.BASE_MIN[k], rm.BASE_MAX[k]) for k in (0, 1, 2, 5)]
        sm.sense_gripper_state_noise(rec, setup.sensors, readings)
        for st in range(sm.ST_CART, sm.ST_CART + 12):           # the cartesian stream's geometry is not restated
            rec.add(st, slot_value(st))
    return rec


def finger_angles(sc, row):
    return [np.array(row["qpos"][finger_q(sc, f)], dtype=np.float64) for f in range(3)]


def compare(setup, rec, after, who, noise_units=0.0, gauge_rel=None, tips=None, late=None):
    """Model record against a record under test.  Bit for bit: time, last_read, the generator,
    every window index, every window value off the transcendental paths.  Values from a
    Gaussian draw: within noise_units * 2^-24.  Gauge-derived values where the model derived
    the gauge (gauge_rel): within gauge_rel * the finger's tip deflection (tips, mm), in the
    window's own unit.  Returns (worst noise error in 2^-24, worst gauge error relative to
    the tip deflection).  late (a list): the noise bound's misses are collected there instead
    of raised, so that a caller can print every figure before it asserts."""
    assert float(after["time"]) == rec.time, f"{who}: time {float(after['time'])!r} vs model {rec.time!r}"
    assert int(after["rng"]) == rec.rng.state, f"{who}: generator {int(after['rng'])} vs model {rec.rng.state} ({rec.rng.draws} draws)"
    for n, k in sm.SLOT.items():
        assert float(after["last_read"][k]) == rec.last_read[k], \
            f"{who}: last_read[{n}] {float(after['last_read'][k])!r} vs model {rec.last_read[k]!r}"
    worst_noise = worst_gauge = 0.0
    for st in ALL_STREAMS:
        w = rec.w[st]
        assert int(after["ring_i"][st]) == w.i, f"{who}: ring_i[{st}] {int(after['ring_i'][st])} vs model {w.i} ({w.adds} appends)"
        got = np.asarray(after["ring"][st], dtype=np.float32)
        for k in range(sm.RING):
            a, b = F(got[k]), F(w.v[k])
            if a.tobytes() == b.tobytes():
                continue
            if (st, k) in rec.gauss_slots:
                err = abs(float(a) - float(b)) / 2.0 ** -24
                worst_noise = max(worst_noise, err)
                msg = f"{who}: window {st}[{k}] {a!r} vs model {b!r}: {err:.3f} x 2^-24 > {noise_units}"
                if late is not None and err > noise_units:
                    late.append((err, abs(float(a) - float(b)) / float(np.spacing(abs(b))), msg))
                    continue
                assert err <= noise_units, msg
            elif gauge_rel is not None and (st, k) in rec.gauge_slots:
                f, scale = rec.gauge_slots[(st, k)]
                err = abs(float(a) - float(b)) / (scale * tips[f]) if tips[f] > 0 else np.inf
                worst_gauge = max(worst_gauge, err)
                assert err <= gauge_rel, f"{who}: window {st}[{k}] {a!r} vs model {b!r}: {err:.3e} of the tip deflection > {gauge_rel:.3e}"
            else:
                raise AssertionError(f"{who}: window {st}[{k}] {a!r} vs model {b!r}")
    return worst_noise, worst_gauge
