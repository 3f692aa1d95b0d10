"""Crafted states for the constraint stage (test infrastructure only).

One env per case.  A case is a GmEnvState record, its object, the model it runs on (N
finger segments and a model-constant variant) and what family it belongs to:

a  reused records: the collider table of tests/contact_cases.py (44 for N = 8, 6 for
   N = 10, nefc == 132 among them) and grasp states of the scripted mix (6 phases x box,
   cylinder, sphere) with random joint velocities added;
b  the object on the ground only (the decoupled first Newton point): sphere, box, cylinder
   on its rim and on its side, each at rest, sliding along t1, sliding askew, spinning about
   the normal, moving upward (no edge active, every force exactly 0) and lifting while
   sliding (one edge active); the resting box also for N = 5 and N = 10; the sphere and the
   box at rest and sliding askew with object friction 1.7 (every geom of the model has
   friction 1, where mu^2 is invisible);
c  warm starts: twelve (b) states (every shape at rest, sliding askew, lifting while
   sliding) and four grasp states with qacc_warm = 0, the converged qacc, its negative, and
   a random vector of 1e3 times its norm;
d  motor locks: 1 to 4 active, lock_q offsets of 0, 0.3, 0.7 and 2 solimp widths in both
   signs, moving slides, finger prismatics (two world components) and the palm slide (one),
   with and without finger-object contacts;
e  six solimp / solref variants of the model on six states each;
f  capped solves: newton_maxit = 1 and 2 on those non-converged warm starts of (c) that
   need more iterations than the cap.

Model-constant variants write the blob through ip.GmModel.from_buffer(model.buf); every
(N, variant) pair is its own env batch of at most 64 records.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import contact_cases as cc
import indep_physics as ip
import oracle_lib as ol

MAX_BATCH = 64
SOLIMP = (0.9, 0.95, 0.001, 0.5, 2.0)
WIDTH = SOLIMP[2]
VARIANTS = {
    "default": {},
    "power 1": dict(solimp=(0.9, 0.95, 0.001, 0.5, 1.0)),
    "power 3": dict(solimp=(0.9, 0.95, 0.001, 0.5, 3.0)),
    "midpoint 0.3": dict(solimp=(0.9, 0.95, 0.001, 0.3, 2.0)),
    "dmin == dmax": dict(solimp=(0.9, 0.9, 0.001, 0.5, 2.0)),
    "width 0": dict(solimp=(0.9, 0.95, 0.0, 0.5, 2.0)),
    "solref (0.004, 0.7)": dict(solref=(0.004, 0.7)),
    "newton_maxit 1": dict(newton_maxit=1),
    "newton_maxit 2": dict(newton_maxit=2),
}
E_VARIANTS = list(VARIANTS)[1:7]
WARM = ("zero", "converged", "negated", "random x 1e3")


class Item:
    def __init__(self, name, family, n_seg, rec, obj, variant="default", base=None, warm=None, may_overflow=False):
        self.name, self.family, self.n_seg, self.variant = name, family, n_seg, variant
        self.rec = np.array(rec, dtype=np.uint8, copy=True)
        self.obj = type(obj).from_buffer_copy(obj)
        self.base = base            # the Item whose problem this one shares (another warm start of it)
        self.warm = warm
        self.may_overflow = may_overflow

    def derive(self, gm, name, family, **kw):
        it = Item(name, family, self.n_seg, self.rec, self.obj, kw.pop("variant", self.variant),
                  kw.pop("base", None), kw.pop("warm", None), self.may_overflow)
        return it, gm.env_state_view(it.rec)


_scenes = {}


def scene(gm, n_seg, variant="default"):
    """cc.Scene for N segments with the variant's constants written into its blob."""
    key = (n_seg, variant)
    if key not in _scenes:
        sc = cc.Scene(gm, n_seg)
        raw = ip.GmModel.from_buffer(sc.model.buf)
        assert tuple(raw.solimp[:]) == SOLIMP and tuple(raw.solref[:]) == (0.02, 1.0) and raw.mujoco_actuators == 1
        for f, val in VARIANTS[variant].items():
            if f == "newton_maxit":
                raw.newton_maxit = val
            else:
                for k, x in enumerate(val):
                    getattr(raw, f)[k] = x
        sc.M = ip.Model(sc.model)
        sc.m = sc.M.raw
        _scenes[key] = sc
    return _scenes[key]


class Batch:
    """Items of one (N, variant): the objects array, the records (obj_index rewritten to
    the item's slot) and, after run_oracle, the oracle's substep from them."""

    def __init__(self, gm, items):
        assert 0 < len(items) <= MAX_BATCH and len({(i.n_seg, i.variant) for i in items}) == 1
        self.items = items
        self.n_seg, self.variant = items[0].n_seg, items[0].variant
        self.sc = scene(gm, self.n_seg, self.variant)
        self.objs = (gm._lib.Object * len(items))()
        self.recs = np.ascontiguousarray(np.stack([i.rec for i in items]))
        v = gm.env_state_view(self.recs)
        for k, it in enumerate(items):
            C.memmove(C.byref(self.objs[k]), C.byref(it.obj), C.sizeof(it.obj))
            v["obj_index"][k] = k

    def run_oracle(self, gm):
        """One substep per record on one oracle env: contacts, forces, qacc, the state
        after, and the Newton iterations / line-search evaluations / cap of that solve."""
        sc, n = self.sc, len(self.items)
        o = ol.OracleEnv(sc.model, sc.cfg, self.objs, env_id=0)
        self.ncon = np.zeros(n, dtype=np.int32)
        self.con = np.zeros((n, 32, 16))
        self.efc = np.zeros((n, 132))
        self.qacc = np.zeros((n, sc.nv))
        self.after = np.zeros_like(self.recs)
        self.iters, self.ls_evals = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        v0 = gm.env_state_view(self.recs)
        for k in range(n):
            s0 = ol.solver_stats(o)
            o.import_state(self.recs[k])
            self.ncon[k], self.con[k], self.efc[k], self.qacc[k] = o.debug_substep()
            s1 = ol.solver_stats(o)
            assert s1["solves"] == s0["solves"] + 1
            self.iters[k] = s1["iterations"] - s0["iterations"]
            self.ls_evals[k] = s1["line_search_evals"] - s0["line_search_evals"]
            self.after[k] = o.export_state()
        va = gm.env_state_view(self.after)
        self.nl = v0["lock_active"][:, :sc.m.nlock].astype(bool).sum(axis=1)
        self.nefc = (self.nl + 4 * self.ncon).astype(np.int32)
        self.capped = va["newton_caps"] > v0["newton_caps"]
        self.overflow = va["overflow"] > v0["overflow"]
        for a in (self.recs, self.ncon, self.con, self.efc, self.qacc, self.after):
            a.setflags(write=False)
        return self

    def contacts(self, k, ncon=None, con=None):
        n = int(self.ncon[k] if ncon is None else ncon[k])
        c = (self.con if con is None else con)[k, :n]
        return dict(dist=c[:, 0], pos=c[:, 1:4], frame=c[:, 4:13].reshape(n, 3, 3), g1=c[:, 13], g2=c[:, 14], mu=c[:, 15])


def batches_of(gm, items):
    groups = {}
    for it in items:
        groups.setdefault((it.n_seg, it.variant), []).append(it)
    out = []
    for g in groups.values():
        # the warm starts of one state stay in one batch
        units = []
        for it in g:
            if units and it.base is not None and units[-1][-1].base is it.base and units[-1][-1].family == it.family:
                units[-1].append(it)
            else:
                units.append([it])
        chunk = []
        for u in units:
            if len(chunk) + len(u) > MAX_BATCH:
                out.append(Batch(gm, chunk))
                chunk = []
            chunk = chunk + u
        out.append(Batch(gm, chunk))
    return out


# ---------------------------------------------------------------- (a) reused records
def contact_items(gm, n_seg):
    sc = scene(gm, n_seg)
    cases = cc.make_cases(sc)
    objs, recs = cc.build_records(sc, cases)
    return [Item("contact table: " + c.name, "a", n_seg, recs[i], objs[i], may_overflow="engulfing" in c.name or
                 "2 dropped" in c.name) for i, c in enumerate(cases)]


GRASP_PHASES = (8, 16, 24, 32, 40, 47)


def grasp_items(gm, seed=11):
    """Six phases of the scripted grasp mix for a box, a cylinder and a sphere (set6 objects
    0, 1, 2), joint velocities kicked by N(0, 0.1)."""
    sc = scene(gm, 8)
    objs = gm.make_object_set("set6_synthetic", 3)
    assert [int(objs[i].type) for i in range(3)] == [cc.BOX, cc.CYL, cc.SPH]
    rng = np.random.default_rng(seed)
    script = gm.GraspScript(sc.settings, 1, seed=5)
    out = []
    for oi in range(3):
        o = ol.OracleEnv(sc.model, sc.cfg, objs, env_id=2 + oi)
        sp = gm.Spawn()
        sp.object_index, sp.x, sp.y, sp.zrot = oi, 0.004, -0.003, 0.3
        o.reset(sp)
        for k in range(max(GRASP_PHASES) + 1):
            if k in GRASP_PHASES:
                rec = o.export_state()
                v = gm.env_state_view(rec)
                assert int(v["extra_substeps"]) == 0
                v["qvel"][:sc.nv] += rng.normal(0.0, 0.1, size=sc.nv)
                out.append(Item(f"grasp: object {oi}, env-step {k}", "a", 8, rec, objs[oi]))
            o.step(script.actions(k)[0])
    return out


# ---------------------------------------------------------------- (b) object on the ground
def ground_shapes(sc, pen=1e-3):
    at = lambda z: np.array([cc.FAR[0], cc.FAR[1], z])
    hs = np.array([0.02, 0.015, 0.01])
    rc, hh = 0.02, 0.03
    R20 = ip.quat2mat(cc.mat2quat(ip.rotx(np.radians(20))))
    Rside = ip.quat2mat(cc.mat2quat(ip.roty(np.pi / 2)))

    def cyl_low(R):
        a = R[:, 2]
        return hh * abs(a[2]) + rc * np.sqrt(max(0.0, 1.0 - a[2] * a[2])) - pen
    return [("sphere", cc.Case("sphere", "b", cc.SPH, [0.025], at(0.025 - pen), np.eye(3)), 1),
            ("box", cc.Case("box", "b", cc.BOX, hs, at(hs[2] - pen), ip.rotz(0.3)), 4),
            ("cylinder on its rim", cc.Case("rim", "b", cc.CYL, [rc, hh], at(cyl_low(R20)), R20), 1),
            ("cylinder on its side", cc.Case("side", "b", cc.CYL, [rc, hh], at(cyl_low(Rside)), Rside), 2)]


MOTIONS = ("at rest", "sliding along t1", "sliding askew", "spinning about the normal", "moving upward",
           "lifting while sliding")


def ground_items(gm, n_seg, motions=MOTIONS, shapes=None, pen=1e-3, family="b", friction=None):
    sc = scene(gm, n_seg)
    sh = [s for s in ground_shapes(sc, pen) if shapes is None or s[0] in shapes]
    objs, recs = cc.build_records(sc, [c for _, c, _ in sh])
    # the contact frame of the resting state (contacts are inputs: the collider has its own tests)
    ncon, _, con, _, _, _, _ = ol.batch_substep(sc.model, sc.cfg, objs, recs)
    out = []
    d0 = sc.m.dof_obj
    for i, (name, case, n_expected) in enumerate(sh):
        assert ncon[i] == n_expected, (name, ncon[i])
        n, t1, t2 = con[i, 0, 4:7], con[i, 0, 7:10], con[i, 0, 10:13]
        assert np.abs(n - cc.Z).max() < 1e-12
        for mo in motions:
            it = Item(f"{name} on the ground, {mo}, N = {n_seg}" + ("" if pen == 1e-3 else f", {pen * 1e3:g} mm deep") +
                      ("" if friction is None else f", friction {friction:g}"), family, n_seg, recs[i], objs[i])
            v = gm.env_state_view(it.rec)
            if friction is not None:        # every other geom has friction 1: the contact's mu is the larger one
                it.obj.friction = friction
                v["obj_friction"] = friction
            lin, ang = np.zeros(3), np.zeros(3)
            if mo == "sliding along t1":
                lin = 0.2 * t1
            elif mo == "sliding askew":
                lin = 0.2 * t1 + 0.12 * t2
            elif mo == "spinning about the normal":
                ang = case.R.T @ (5.0 * n)              # the free joint's angular velocity is in the body frame
            elif mo == "moving upward":
                lin = 0.5 * n
            elif mo == "lifting while sliding":
                lin = 0.2 * n + 0.5 * t1
            v["qvel"][d0:d0 + 3] = lin
            v["qvel"][d0 + 3:d0 + 6] = ang
            out.append(it)
    return out


# ---------------------------------------------------------------- (c) warm starts
def warm_items(gm, bases, family="c", seed=23):
    """Four warm starts of each base item; the converged qacc comes from the oracle's solve
    of the base state."""
    rng = np.random.default_rng(seed)
    out = []
    for b in batches_of(gm, bases):
        b.run_oracle(gm)
        nv = b.sc.nv
        for k, base in enumerate(b.items):
            qa = b.qacc[k]
            r = rng.normal(size=nv)
            starts = dict(zip(WARM, (np.zeros(nv), qa, -qa, r * (1e3 * np.linalg.norm(qa) / np.linalg.norm(r)))))
            for w, vec in starts.items():
                it, v = base.derive(gm, f"{base.name}; warm start {w}", family, base=base, warm=w)
                v["qacc_warm"][:nv] = vec
                out.append(it)
    return out


# ---------------------------------------------------------------- (d) motor locks
def sphere_on_finger(sc, pen, r=0.01):
    """A sphere pen deep in the inner face of finger 1's fifth box (contact_cases.sphere_cases)."""
    geoms = sc.fk_geoms(sc.q0)
    g = sc.finger_geom(0, 4)
    (c, R), hs = geoms[g], sc.gsize[g]
    ax, sg = sc.inner_face(geoms, g)
    n = sg * R[:, ax]
    on_face = c + R @ np.array([0.002, 0.0, -0.003]) + n * hs[ax]
    return cc.Case(f"sphere {pen * 1e3:g} mm into a finger face", "d", cc.SPH, [r], on_face + n * (r - pen), np.eye(3))


def sphere_on_palm(sc, pen, r=0.01):
    geoms = sc.fk_geoms(sc.q0)
    (cp, Rp), hp = geoms[sc.g_palm], sc.gsize[sc.g_palm]
    down = -Rp[:, 0] if Rp[2, 0] > 0 else Rp[:, 0]
    return cc.Case(f"sphere {pen * 1e3:g} mm into the palm", "d", cc.SPH, [r],
                   cp + Rp @ np.array([0.0, 0.005, -0.004]) + down * (hp[0] + r - pen), np.eye(3))


# (which of the four locks are active, their lock_q offsets in solimp widths, the slides' velocities)
LOCKS = [
    ("1 lock", (1, 0, 0, 0), (0.3, 0, 0, 0), (0.01, 0, 0, 0)),
    ("2 locks", (1, 1, 0, 0), (-0.3, 0.7, 0, 0), (-0.02, 0.01, 0, 0)),
    ("3 locks", (1, 1, 1, 0), (-0.7, 2.0, 0.0, 0), (0.01, -0.01, 0.02, 0)),
    ("4 locks", (1, 1, 1, 1), (-2.0, 0.3, 0.7, -0.3), (0.01, 0.02, -0.01, 0.005)),
    ("palm lock alone", (0, 0, 0, 1), (0, 0, 0, 0.7), (0, 0, 0, -0.01)),
    ("palm lock saturated", (0, 0, 0, 1), (0, 0, 0, -2.0), (0, 0, 0, 0.01)),
    ("3 locks, palm among them", (1, 0, 1, 1), (0.7, 0, -0.3, 2.0), (0.0, 0, 0.01, 0.01)),
]


def lock_items(gm, family="d", pens=(1e-3, 1e-3, 1e-3)):
    sc = scene(gm, 8)
    far = ground_shapes(sc)[0][1]                      # the sphere on the ground, away from the gripper
    touching = [sphere_on_finger(sc, pens[0]), sphere_on_palm(sc, pens[1]),
                [c for c in cc.box_cases(sc) if c.name == "box flush on a finger face"][0]]
    cases = [far] + touching
    objs, recs = cc.build_records(sc, cases)
    plan = [(0, k) for k in range(len(LOCKS))] + [(1, 2), (1, 3), (2, 5), (2, 3), (3, 1), (3, 6)]
    out = []
    for ci, li in plan:
        lname, active, offs, vels = LOCKS[li]
        it = Item(f"{lname}, {cases[ci].name}", family, 8, recs[ci], objs[ci])
        v = gm.env_state_view(it.rec)
        for k in range(sc.m.nlock):
            d = int(sc.m.lock_dof[k])
            v["lock_active"][k] = active[k]
            v["lock_q"][k] = v["qpos"][d] - offs[k] * WIDTH
            v["qvel"][d] = vels[k]
        out.append(it)
    return out


# ---------------------------------------------------------------- (e) solimp / solref variants
def variant_items(gm, grasp):
    """Six states per variant: two on the ground (0.2 and 0.7 widths deep: either side of
    mid x width at mid = 0.5 and at 0.3 < 0.7), two grasp states, two lock states (a contact
    two widths deep beyond the saturation, lock offsets on both sigmoid halves)."""
    sc = scene(gm, 8)
    g1 = ground_items(gm, 8, motions=("sliding askew",), shapes=("sphere",), pen=0.2 * WIDTH, family="e")
    g2 = ground_items(gm, 8, motions=("at rest",), shapes=("box",), pen=0.7 * WIDTH, family="e")
    lk = lock_items(gm, family="e", pens=(2 * WIDTH, 0.2 * WIDTH, 1e-3))
    pick = g1 + g2 + grasp + [lk[3], lk[7]]
    assert len(pick) == 6 and "4 locks" in lk[3].name and "finger face" in lk[7].name
    out = []
    for var in E_VARIANTS:
        for p in pick:
            it, _ = p.derive(gm, f"{p.name} [{var}]", "e", variant=var)
            out.append(it)
    return out


# ---------------------------------------------------------------- the table
def build_table(gm):
    """Every batch of the table, the oracle run on each."""
    a = contact_items(gm, 8) + contact_items(gm, 10)
    grasp = grasp_items(gm)
    b8 = ground_items(gm, 8)
    b_other = ground_items(gm, 5, motions=("at rest",), shapes=("box",)) + \
        ground_items(gm, 10, motions=("at rest",), shapes=("box",))
    # mu != 1 (every geom of the model has friction 1, so mu^2 would otherwise be invisible)
    b_mu = ground_items(gm, 8, motions=("at rest", "sliding askew"), shapes=("sphere", "box"), friction=1.7)
    # four grasp states for the warm starts: ones with contacts, from the later phases
    gb = batches_of(gm, grasp)[0].run_oracle(gm)
    with_contacts = [k for k in range(len(grasp)) if gb.ncon[k] >= 2]
    assert len(with_contacts) >= 6
    warm_grasp = [grasp[k] for k in with_contacts[-4:]]
    # warm starts (and, from them, the capped solves) on every shape at rest, sliding askew and
    # lifting while sliding, and on the four grasp states: the other motions of (b) take the
    # same paths, and four warm starts of all of them double the table for nothing new
    b_warm = [it for it in b8 if any(m in it.name for m in (", at rest,", ", sliding askew,", ", lifting while sliding,"))]
    assert len(b_warm) == 12
    c = warm_items(gm, b_warm + warm_grasp)
    d = lock_items(gm)
    e = variant_items(gm, [grasp[with_contacts[0]], grasp[with_contacts[-1]]])
    # (f): the non-converged warm starts that take more iterations than the cap
    f = []
    for bt in batches_of(gm, c):
        bt.run_oracle(gm)
        for k, it in enumerate(bt.items):
            if it.n_seg != 8 or it.warm not in WARM[2:]:
                continue
            for cap in (1, 2):
                if bt.iters[k] > cap:
                    nit, _ = it.derive(gm, f"{it.name} [newton_maxit {cap}]", "f", variant=f"newton_maxit {cap}",
                                       base=it.base, warm=it.warm)
                    f.append(nit)
    items = a + grasp + b8 + b_other + b_mu + c + d + e + f
    batches = [bt.run_oracle(gm) for bt in batches_of(gm, items)]
    return batches
