"""The free object's work spread over lanes (gm_rows.h body_vel, gm_dynamics.h crb_rne) against
the same sources built without it (-DGM_NO_OBJECT_LANES, gmx.build.build_no_object_lanes), byte
for byte.

Every value is produced by the same operations on the same operands in the same order, on six
lanes instead of one, so the comparison is equality of the fp64 records (env_states), of every
output and of the diagnostic substep's contacts, row forces, qacc and wrench: no tolerance, and
the reference is the second library, never the code under test alone.

One batch of eight crafted states (tests/contact_cases.py; N = 8, CL = 10):

- an object at rest on the ground, the gripper clear (obj_only and the decoupled point): a box, a
  sphere and a cylinder;
- an object spinning and translating fast, all six qvel components non-zero with mixed signs: a
  sphere in the air, a cylinder on its side and a box on the ground (the kicked box's first Newton
  point is not accepted, so rows_jar runs more than once: the Newton-point count of the profiled
  env-step says so);
- a finger pressing the object (the slab with finger 1's hook in it: the general body_vel path
  and the general Newton point), at rest and moving;
- the lock rows all active, none active and exactly one active (each lock in turn), every active
  lock 1 mm off its anchor so that its row has a position error.

The same comparison runs on a 1-env and a 2-env context on DUO workgroups (the helper wave forms
the contact rows), and the default library's DUO env-step equals its one-wave env-step.
"""
import numpy as np
import pytest

import contact_cases as cc
import indep_physics as ip
from conftest import gpu_available
from test_decoupled_point import assert_same, make_env, run
from test_newton_decoupled import at, pattern, slab

pytestmark = pytest.mark.gpu

N_SEG = 8


@pytest.fixture(scope="module")
def sc(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    return cc.Scene(gm, N_SEG)


@pytest.fixture(scope="module")
def libs(gm):
    """(default library, the one built with -DGM_NO_OBJECT_LANES)."""
    if not gpu_available():
        pytest.skip("no GPU")
    from gmx.build import build_no_object_lanes
    return gm.load_library(), gm.load_library(build_no_object_lanes())


class Crafted:
    """Crafted cases as one device batch: the records with the object's qvel and the lock
    flags written in, and each env's contact pattern at that state (the oracle's collider)."""

    def __init__(self, gm, sc, cases, qvel_obj, locks):
        import oracle_lib as ol
        self.cases = cases
        self.objs, recs = cc.build_records(sc, cases)
        v = gm.env_state_view(recs)
        d0 = sc.m.dof_obj
        v["qvel"][:, d0:d0 + 6] = qvel_obj
        self.nlock = int(sc.m.nlock)
        ld = ip.arr(sc.m.lock_dof)[:self.nlock]
        for i, active in enumerate(locks):
            v["lock_active"][i][:] = 0
            v["lock_active"][i][:self.nlock] = active[:self.nlock]
            v["lock_q"][i][:self.nlock] = v["qpos"][i][ld] + 1e-3
        self.recs = recs
        ncon, _, con, *_ = ol.batch_substep(sc.model, sc.cfg, self.objs, recs)
        self.patterns = [pattern(sc, ncon[i], con[i]) for i in range(len(cases))]
        self.recs.setflags(write=False)


FAST = np.array([[0.7, -0.4, 0.3, -3.0, 2.0, 5.0],
                 [-0.5, 0.6, -0.2, 4.0, -1.5, -2.5],
                 [0.3, 0.2, -0.1, 1.0, -2.0, 0.5],
                 [-0.05, 0.04, -0.02, 0.3, -0.2, 0.1]])
ALL, NONE = (1, 1, 1, 1), (0, 0, 0, 0)
ONE = [tuple(int(j == k) for j in range(4)) for k in range(4)]
REST, KICKED, PRESSED = (0, 1, 2), 5, (6, 7)


def cases_qvel_locks(sc):
    ground = {c.name: c for c in cc.ground_cases(sc)}
    cases = [ground["box flat"], ground["sphere 2 mm deep"], ground["cylinder upright"],
             cc.Case("sphere in the air", "newton", cc.SPH, [0.025], at(0.1), np.eye(3)),
             ground["cylinder on its side"], ground["box flat"],
             slab(sc, "slab with finger 1's hook in it", 0.012), slab(sc, "slab with finger 1's hook in it", 0.012)]
    qvel = np.zeros((8, 6))
    qvel[3], qvel[4], qvel[5], qvel[7] = FAST
    locks = [ALL, NONE, ONE[0], ONE[1], ONE[2], ALL, NONE, ALL]
    return cases, qvel, locks


@pytest.fixture(scope="module")
def batch(gm, sc):
    cases, qvel, locks = cases_qvel_locks(sc)
    b = Crafted(gm, sc, cases, qvel, locks)
    assert b.nlock >= 3, b.nlock
    assert {c.otype for c in cases} == {cc.SPH, cc.BOX, cc.CYL}
    # what each state was crafted to hold: (object-ground, gripper-object, gripper-ground) contacts
    want = [(4, 0, 0), (1, 0, 0), (4, 0, 0), (0, 0, 0), (2, 0, 0), (4, 0, 0), (4, 2, 0), (4, 2, 0)]
    assert b.patterns == want, b.patterns
    la = gm.env_state_view(b.recs)["lock_active"][:, :b.nlock].sum(axis=1)
    assert (la == b.nlock).any() and (la == 0).any() and (la == 1).any(), la
    return b


def test_substep_and_env_step_equal_the_switch_off_build(gm, sc, libs, batch):
    act = np.zeros((len(batch.cases), 4), dtype=np.float32)
    outs, points = [], []
    for lib in libs:
        env = make_env(gm, sc, batch, lib)
        try:
            assert env.dispatch_info()["waves_per_env"] == 1
            outs.append(run(gm, env, batch.recs, act))
            env.set_env_states(batch.recs)
            env.set_action(act)
            ph = env.step_profiled()
            points.append((ph[:, env.PH_NEWTON].copy(), env.decoupled_points.copy()))
            outs[-1]["states_after_profiled_step"] = env.env_states()
            nsub = env.cfg.sim_steps_per_action + gm.env_state_view(batch.recs)["extra_substeps"]
        finally:
            env.close()
    assert_same(outs[0], outs[1], "crafted batch")
    v0, v1 = gm.env_state_view(batch.recs), gm.env_state_view(outs[0]["states"])
    assert (v1["time"] > v0["time"]).all() and np.isfinite(v1["qpos"]).all()
    (newton, dec), (newton_off, dec_off) = points
    print(f"\nsubsteps {nsub.tolist()}, Newton points {newton.tolist()}, decoupled first points {dec.tolist()}")
    assert np.array_equal(newton, newton_off) and np.array_equal(dec, dec_off)
    for i in REST:                      # obj_only and the decoupled point on every substep
        assert dec[i] == nsub[i], (batch.cases[i].name, int(dec[i]))
    for i in PRESSED:                   # the general body_vel path and the general point
        assert dec[i] < nsub[i], (batch.cases[i].name, int(dec[i]))
    assert newton[KICKED] > nsub[KICKED], int(newton[KICKED])   # a multi-point solve: rows_jar again


@pytest.mark.parametrize("envs", [(6,), (0, 4)])
def test_duo_contexts_equal_the_switch_off_build(gm, sc, libs, envs):
    """A 1-env and a 2-env context on DUO workgroups: the pressed slab; the box at rest and the
    spinning cylinder."""
    cases, qvel, locks = cases_qvel_locks(sc)
    b = Crafted(gm, sc, [cases[i] for i in envs], qvel[list(envs)], [locks[i] for i in envs])
    act = np.zeros((len(envs), 4), dtype=np.float32)
    outs = []
    for lib in libs:
        env = make_env(gm, sc, b, lib, duo="1")
        try:
            assert env.dispatch_info()["waves_per_env"] == 2
            outs.append(run(gm, env, b.recs, act))
        finally:
            env.close()
    assert_same(outs[0], outs[1], f"DUO, {len(envs)} env(s)")


def test_duo_env_step_equals_one_wave(gm, sc, libs, batch):
    act = np.zeros((len(batch.cases), 4), dtype=np.float32)
    outs = []
    for duo, waves in (("1", 2), ("0", 1)):
        env = make_env(gm, sc, batch, libs[0], duo=duo)
        try:
            assert env.dispatch_info()["waves_per_env"] == waves
            env.set_env_states(batch.recs)
            obs, rew, _, _ = env.step(act)
            _, done = env.reward_done()
            outs.append(dict(obs=np.array(obs, copy=True), rew=np.array(rew, copy=True), done=np.array(done, copy=True),
                             states=env.env_states()))
        finally:
            env.close()
    assert_same(outs[0], outs[1], "DUO against one wave")
