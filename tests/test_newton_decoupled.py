"""The Newton point on the contact patterns that decouple the object from the gripper
(gm_newton_point.h newton_point).

The object's ground contacts are composed across the contact lanes of the object-ground
pair and summed in slot order; when no gripper body touches the object (any_o false) the
gripper rows' composites are zero and the object block of the Hessian stands alone, and a
gripper body on the ground (any_g) takes the ground pass.  Which of these a substep runs
is decided by its contacts, so the states here are crafted (tests/contact_cases.py: the
oracle's reset record with qpos / qvel overwritten) to hold each pattern on purpose, and
every comparison is test_grasp_parity.compare_substep's, with its quantities and
tolerances: contacts to 1e-9, efc and qacc to 1e-7 of scale, the object's cfrc_ext to
1e-7, qpos to 1e-9 after the substep.

- ground-contact counts 0 (a sphere in the air), 1 (a sphere on the ground), 2 (a cylinder
  lying on its side) and 4 (a box flat, a cylinder upright), the gripper far away;
- in the same batch the other patterns: a slab on the ground with one finger link (finger
  1's hook) in it, and the three hooks in the ground with a box on the ground (the ground
  pass, which re-reads the per-contact Q / F after the ground composite was staged);
- a pattern that switches inside one env-step: a slab on the ground just clear of finger
  1's hook, the fingers closing (+1 gripper_prismatic_X) until the hook is in it, beside a
  slab that stays clear -- the decoupled and the coupled assembly in one launch, against
  the oracle's env-step (test_grasp_parity.compare_step's contract, and qpos to 1e-6: 63
  substeps at the substep bound of 1e-9 with a factor of ten for the contact onset);
- the object's quaternion step on both sides of its |w| > 1e-15 branch: at rest (|w| = 0
  exactly: a sphere in free fall from rest takes no angular acceleration) and spinning,
  in the air and on the ground; one substep against the oracle, and one env-step on DUO
  workgroups against the one-wave kernel bit for bit (the diagnostic substep always runs
  the one-wave kernel).

The object-ground pair is the first candidate pair, so its contacts take slots 0 .. 3 and
the cut at GM_MAX_CON cannot fall inside them: the capacity states of
tests/test_contact_cases.py (ncon = 32 with four ground contacts) cover the full width.
"""
import os

import numpy as np
import pytest

import contact_cases as cc
import indep_physics as ip
from conftest import gpu_available
from test_grasp_parity import compare_step, compare_substep

pytestmark = pytest.mark.gpu

N_SEG = 8
CLEAR = 0.04          # slab this far inwards of finger 1's face: clear of the hook for the whole env-step
ONSET = (0.033, 0.034)  # clear of the hook at first, in it after one closing env-step


def slab(sc, name, top, gap=0.0, pen=2e-4):
    """contact_cases.full_width_cases' slab: standing on the ground (pen deep), its face
    parallel (but for TILT) to finger 1's lowest segment, pen into that face or gap clear of
    it; top: the height of its upper face."""
    geoms = sc.fk_geoms(sc.q0)
    g = sc.finger_geom(0, sc.n_seg)
    (c, R), hs = geoms[g], sc.gsize[g]
    ax, sg = sc.inner_face(geoms, g)
    n = sg * R[:, ax]
    hz = 0.5 * (top + pen)
    hx, hy = 0.01, 0.02
    Rs = np.column_stack([R[:, 2] if np.linalg.det(np.column_stack([R[:, 2], n, -R[:, 0]])) > 0 else -R[:, 2], n, -R[:, 0]])
    Rs = Rs @ ip.rotz(cc.TILT)
    ctr = c + n * (hs[ax] + hy - pen + gap)
    ctr = ctr + Rs[:, 2] * ((hz - pen - ctr @ cc.Z) / Rs[2, 2])
    return cc.Case(name, "newton", cc.BOX, [hx, hy, hz], ctr, Rs, kind=cc.ORACLE, mass=0.5)


def pattern(sc, ncon, con):
    """(object-ground contacts, gripper-object contacts, gripper-ground contacts) of one env."""
    ids = [(int(con[k, 13]), int(con[k, 14])) for k in range(int(ncon))]
    n_go = sum(p == (sc.g_ground, sc.g_obj) for p in ids)
    n_o = sum(sc.g_obj in p and sc.g_ground not in p for p in ids)
    n_g = sum(sc.g_ground in p and sc.g_obj not in p for p in ids)
    return n_go, n_o, n_g


class Batch:
    """Crafted cases as one device batch: records, objects and the oracle's substep."""

    def __init__(self, gm, sc, cases, qvel_obj=None):
        import oracle_lib as ol
        self.sc, self.cases = sc, cases
        self.objs, recs = cc.build_records(sc, cases)
        if qvel_obj is not None:
            v = gm.env_state_view(recs)
            v["qvel"][:, sc.m.dof_obj:sc.m.dof_obj + 6] = qvel_obj
        self.recs = recs
        self.ncon, self.nefc, self.con, *_ = ol.batch_substep(sc.model, sc.cfg, self.objs, recs)
        self.patterns = [pattern(sc, self.ncon[i], self.con[i]) for i in range(len(cases))]
        self.recs.setflags(write=False)

    def env(self, gm, duo=None):
        old = os.environ.get("GM_DUO")
        if duo is not None:
            os.environ["GM_DUO"] = duo
        try:
            return gm.BatchedGripperEnv(len(self.cases), settings=self.sc.settings, seed=3, model_blob=self.sc.model,
                                        objects=self.objs)
        finally:
            if old is None:
                os.environ.pop("GM_DUO", None)
            else:
                os.environ["GM_DUO"] = old


@pytest.fixture(scope="module")
def sc(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    return cc.Scene(gm, N_SEG)


def at(z):
    return np.array([cc.FAR[0], cc.FAR[1], z])


def test_ground_counts_and_mixed_patterns_substep(gm, sc):
    import oracle_lib as ol
    ground = {c.name: c for c in cc.ground_cases(sc)}
    cases = [cc.Case("sphere in the air", "newton", cc.SPH, [0.025], at(0.1), np.eye(3)),
             ground["sphere 2 mm deep"], ground["cylinder on its side"], ground["box flat"], ground["cylinder upright"],
             ground["box yawed"], slab(sc, "slab with finger 1's hook in it", 0.012), cc.hook_case(sc),
             slab(sc, "slab clear of the hook", 0.03, gap=CLEAR), ground["box tilted about x"]]
    b = Batch(gm, sc, cases)
    # what each state was crafted to hold (the oracle's contacts)
    want = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (4, 0, 0), (4, 0, 0), (4, 0, 0), (4, 2, 0), (4, 0, 6), (4, 0, 0), (2, 0, 0)]
    assert b.patterns == want, b.patterns
    env = b.env(gm)
    try:
        rep = compare_substep(gm, ol, env, dict(rec=b.recs, k=0))
    finally:
        env.close()
    print(f"\nground counts and mixed patterns, one substep: {rep}")


def test_pattern_switch_inside_one_env_step(gm, sc):
    import oracle_lib as ol
    cases = [slab(sc, f"slab {g * 1e3:.0f} mm inwards of finger 1", 0.03, gap=g) for g in ONSET] + \
            [slab(sc, "slab clear of the hook", 0.03, gap=CLEAR), slab(sc, "slab with finger 1's hook in it", 0.012)] * 2 + \
            [slab(sc, f"slab {g * 1e3:.0f} mm inwards of finger 1", 0.03, gap=g) for g in ONSET]
    b = Batch(gm, sc, cases)
    onset = [i for i, c in enumerate(cases) if "inwards" in c.name]
    clear = [i for i, c in enumerate(cases) if "clear" in c.name]
    assert all(b.patterns[i] == (4, 0, 0) for i in onset + clear), b.patterns
    assert all(b.patterns[i][1] > 0 for i in range(len(cases)) if i not in onset + clear), b.patterns
    act = np.zeros((len(cases), 4), dtype=np.float32)
    assert gm.scripted.in_use_actions(sc.settings)[0] == "gripper_prismatic_X"
    act[:, 0] = 1.0                                        # the fingers close
    env = b.env(gm)
    try:
        env.set_env_states(b.recs)
        obs, rew, _, _ = env.step(act)
        _, done = env.reward_done()
        snap = dict(k=0, rec=b.recs, a=act, obs=obs, rew=rew, done=done, after=env.env_states())
        rep = compare_step(gm, ol, env, snap)
        print(f"\nclosing env-step: {rep}")
        # the switch happened (oracle): a finger is in the slab after the env-step, none in the clear one
        ncon, _, con, *_ = ol.batch_substep(sc.model, sc.cfg, b.objs, snap["after"])
        after = [pattern(sc, ncon[i], con[i]) for i in range(len(cases))]
        assert all(after[i][1] > 0 and after[i][2] == 0 for i in onset), after
        assert all(after[i][1:] == (0, 0) for i in clear), after
        assert rep["qpos_max"] <= 1e-6, rep
    finally:
        env.close()


def spin_batch(gm, sc):
    ground = {c.name: c for c in cc.ground_cases(sc)}
    air = cc.Case("sphere in the air", "newton", cc.SPH, [0.025], at(0.1), np.eye(3))
    cases = [air, air, ground["sphere 2 mm deep"], ground["sphere 2 mm deep"], ground["box flat"], ground["box flat"],
             air, ground["cylinder on its side"]]
    qvel = np.zeros((len(cases), 6))
    qvel[1, 3:] = (3.0, -2.0, 5.0)                         # spinning in free fall
    qvel[3, 3:] = (0.0, 4.0, 1.0)                          # rolling and spinning on the ground
    qvel[5, 3:] = (0.0, 0.0, 2.0)                          # a box turning on its face
    qvel[6] = (0.1, -0.2, 0.0, 1e-9, 0.0, 0.0)             # |w| h far below the sine's first term, above the branch
    qvel[7, 3:] = (0.5, 0.0, 0.0)
    return Batch(gm, sc, cases, qvel_obj=qvel)


def test_quaternion_step_at_rest_and_spinning(gm, sc):
    import oracle_lib as ol
    b = spin_batch(gm, sc)
    env = b.env(gm)
    try:
        rep = compare_substep(gm, ol, env, dict(rec=b.recs, k=0))
        env.set_env_states(b.recs)
        env.debug_substep(full=True)
        dv, v0 = gm.env_state_view(env.env_states()), gm.env_state_view(b.recs)
    finally:
        env.close()
    print(f"\nquaternion step, one substep: {rep}")
    qa = sc.qadr_obj + 3
    # at rest in free fall the orientation is untouched (the |w| <= 1e-15 branch: normalise only)
    np.testing.assert_array_equal(dv["qpos"][0][qa:qa + 4], v0["qpos"][0][qa:qa + 4])
    for i in (1, 3, 5, 7):
        assert np.abs(dv["qpos"][i][qa:qa + 4] - v0["qpos"][i][qa:qa + 4]).max() > 1e-4, b.cases[i].name
    assert np.abs(np.linalg.norm(dv["qpos"][:, qa:qa + 4], axis=1) - 1.0).max() <= 1e-15


def test_quaternion_step_duo_equals_one_wave(gm, sc):
    b = spin_batch(gm, sc)
    a, o = b.env(gm, "1"), b.env(gm, "0")
    try:
        assert a.dispatch_info()["waves_per_env"] == 2 and o.dispatch_info()["waves_per_env"] == 1
        act = np.zeros((len(b.cases), a.n_actions), dtype=np.float32)
        outs = []
        for e in (a, o):
            e.set_env_states(b.recs)
            obs, rew, done, _ = e.step(act)
            outs.append((obs.copy(), np.asarray(rew).copy(), np.asarray(done).copy(), e.env_states()))
        (oa, ra, da, sa), (ob, rb, db, sb) = outs
        np.testing.assert_array_equal(oa, ob, err_msg="observations")
        np.testing.assert_array_equal(ra, rb, err_msg="rewards")
        np.testing.assert_array_equal(da, db, err_msg="done flags")
        va, vb = gm.env_state_view(sa), gm.env_state_view(sb)
        for f in va.dtype.names:
            np.testing.assert_array_equal(va[f], vb[f], err_msg=f)
        assert (va["time"] > gm.env_state_view(b.recs)["time"]).all() and np.isfinite(va["qpos"]).all()
    finally:
        a.close()
        o.close()
