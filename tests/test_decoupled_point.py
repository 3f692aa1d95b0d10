"""The decoupled Newton point (gm_newton_point.h newton_point_decoupled) against the same
sources built without it (-DGM_NO_DECOUPLED_POINT), byte for byte.

When every contact of a substep is the object's with the ground, the first Newton point of
the solve factors the gripper's arrow matrix and the object's 6x6 block side by side instead
of as one chain.  It leaves out only operations on exact zeros, so its results are the general
point's bit for bit; the comparison here is therefore equality of the fp64 records
(env_states) and of every output, never a tolerance, and the reference is the second library,
never the code under test alone.

One batch of crafted states (tests/contact_cases.py, as tests/test_newton_decoupled.py builds
them; N = 8): object-ground contact counts 0, 1, 2 and 4 with the gripper clear, a slab with a
finger link in it (coupled), the hooks in the ground (the ground pass), a slab that stays
clear and one the closing fingers reach during the env-step.

- one diagnostic substep and one env-step (63 substeps), both libraries: equal records;
- the per-env count of solves that took the decoupled point (step_profiled, the upper half of
  the "cu" column): every solve on the clear envs, not the first one on the coupled envs, some
  but not all on the slab the fingers reach, none at all in the library built without it;
- a capped solve (gm_model.newton_maxit = 1) and a multi-point solve on decoupled envs whose
  object was kicked, so that the first point is not accepted: equal records again, and the cap
  was really hit;
- the same env-step on DUO workgroups equals the one-wave kernel's;
- the shortest and the longest compiled finger chain (N = 5 and N = 10) from a reset under
  random actions: equal outputs and records, and the decoupled point was taken.
"""
import ctypes as C
import os

import numpy as np
import pytest

import contact_cases as cc
from conftest import gpu_available
from test_newton_decoupled import Batch, CLEAR, ONSET, at, slab

pytestmark = pytest.mark.gpu

N_SEG = 8


@pytest.fixture(scope="module")
def sc(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    return cc.Scene(gm, N_SEG)


@pytest.fixture(scope="module")
def libs(gm):
    """(default library, the one built with -DGM_NO_DECOUPLED_POINT)."""
    if not gpu_available():
        pytest.skip("no GPU")
    from gmx.build import build_no_decoupled
    return gm.load_library(), gm.load_library(build_no_decoupled())


def make_env(gm, sc, b, lib, duo="0", model=None):
    old = os.environ.get("GM_DUO")
    os.environ["GM_DUO"] = duo
    try:
        return gm.BatchedGripperEnv(len(b.cases), settings=sc.settings, seed=3, model_blob=model or sc.model,
                                    objects=b.objs, lib=lib)
    finally:
        if old is None:
            os.environ.pop("GM_DUO", None)
        else:
            os.environ["GM_DUO"] = old


@pytest.fixture(scope="module")
def batch(gm, sc):
    ground = {c.name: c for c in cc.ground_cases(sc)}
    cases = [cc.Case("sphere in the air", "newton", cc.SPH, [0.025], at(0.1), np.eye(3)),
             ground["sphere 2 mm deep"], ground["cylinder on its side"], ground["box flat"],
             slab(sc, "slab with finger 1's hook in it", 0.012), cc.hook_case(sc),
             slab(sc, "slab clear of the hook", 0.03, gap=CLEAR),
             slab(sc, "slab the closing fingers reach", 0.03, gap=ONSET[1])]
    b = Batch(gm, sc, cases)
    want = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (4, 0, 0), (4, 2, 0), (4, 0, 6), (4, 0, 0), (4, 0, 0)]
    assert b.patterns == want, b.patterns
    return b


CLEAR_ENVS, COUPLED_ENVS, ONSET_ENV = (0, 1, 2, 3, 6), (4, 5), 7


def closing(gm, sc, n):
    act = np.zeros((n, 4), dtype=np.float32)
    assert gm.scripted.in_use_actions(sc.settings)[0] == "gripper_prismatic_X"
    act[:, 0] = 1.0
    return act


def run(gm, env, recs, act):
    """One diagnostic substep, then one env-step, each from recs: everything they return."""
    out = {}
    env.set_env_states(recs)
    ncon, con, efc, qacc, nefc, w = env.debug_substep(full=True)
    out.update(sub_ncon=ncon, sub_con=con, sub_efc=efc, sub_qacc=qacc, sub_nefc=nefc, sub_wrench=w,
               sub_states=env.env_states())
    env.set_env_states(recs)
    obs, rew, _, _ = env.step(act)
    _, done = env.reward_done()
    out.update(obs=np.array(obs, copy=True), rew=np.array(rew, copy=True), done=np.array(done, copy=True),
               states=env.env_states())
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        assert x.tobytes() == y.tobytes(), f"{what}: {k} differs between the libraries"


def test_substep_and_env_step_equal_the_switch_off_build(gm, sc, libs, batch):
    act = closing(gm, sc, len(batch.cases))
    outs = []
    for lib in libs:
        env = make_env(gm, sc, batch, lib)
        try:
            assert env.dispatch_info()["waves_per_env"] == 1
            outs.append(run(gm, env, batch.recs, act))
        finally:
            env.close()
    assert_same(outs[0], outs[1], "crafted batch")
    v0, v1 = gm.env_state_view(batch.recs), gm.env_state_view(outs[0]["states"])
    assert (v1["time"] > v0["time"]).all() and np.isfinite(v1["qpos"]).all()


def test_each_case_takes_its_path(gm, sc, libs, batch):
    act = closing(gm, sc, len(batch.cases))
    counts = []
    for lib in libs:
        env = make_env(gm, sc, batch, lib)
        try:
            env.set_env_states(batch.recs)
            env.set_action(act)
            ph = env.step_profiled()
            assert (ph[:, 27] < 2 ** 16).all()           # the CU id proper
            counts.append(env.decoupled_points.copy())
            nsub = env.cfg.sim_steps_per_action + gm.env_state_view(batch.recs)["extra_substeps"]
            solves = ph[:, env.PH_NEWTON]
        finally:
            env.close()
    on, off = counts
    print(f"\nsubsteps {nsub.tolist()}, decoupled first points {on.tolist()}, Newton points {solves.tolist()}")
    assert not off.any(), off
    for i in CLEAR_ENVS:
        assert on[i] == nsub[i], (batch.cases[i].name, int(on[i]))
    for i in COUPLED_ENVS:      # (its first substep at the least holds a gripper contact)
        assert on[i] < nsub[i], (batch.cases[i].name, int(on[i]))
    assert 0 < on[ONSET_ENV] < nsub[ONSET_ENV], int(on[ONSET_ENV])


def test_capped_and_multi_point_solves_equal_the_switch_off_build(gm, sc, libs):
    import indep_physics as ip
    ground = {c.name: c for c in cc.ground_cases(sc)}
    cases = [ground["box flat"], ground["cylinder on its side"], ground["sphere 2 mm deep"], ground["box yawed"],
             ground["box tilted about x"], ground["cylinder upright"], ground["box flat"], ground["box flat"]]
    rng = np.random.default_rng(11)
    # the object kicked: the warm start's active edges are then not the optimum's, so the first
    # (decoupled) point is not accepted
    b = Batch(gm, sc, cases, qvel_obj=rng.normal(0.0, 0.5, size=(len(cases), 6)))
    assert all(p[1:] == (0, 0) for p in b.patterns), b.patterns
    capped = gm.ModelBlob(sc.model.params)
    ip.GmModel.from_buffer(capped.buf).newton_maxit = 1
    act = np.zeros((len(cases), 4), dtype=np.float32)
    for name, model in (("capped", capped), ("multi-point", None)):
        outs = []
        for lib in libs:
            env = make_env(gm, sc, b, lib, model=model)
            try:
                outs.append(run(gm, env, b.recs, act))
            finally:
                env.close()
        assert_same(outs[0], outs[1], name)
        caps = gm.env_state_view(outs[0]["sub_states"])["newton_caps"] - gm.env_state_view(b.recs)["newton_caps"]
        print(f"\n{name}: capped solves in the first substep per env {caps.tolist()}")
        if model is not None:
            assert (caps > 0).any(), caps


@pytest.mark.parametrize("n_seg,timestep", [(5, 6.76e-3), (10, 2.1e-3)])
def test_other_chain_lengths_equal_the_switch_off_build(gm, libs, n_seg, timestep):
    """The shortest and the longest compiled chain (CL = n_seg + 2 = 7: the chains' own pivots
    CL .. 7 are a single iteration; CL = 12): 32 envs of the mixed object set from a reset,
    six env-steps of random actions (the object rests on the ground under the open gripper, so
    most solves are decoupled), every output and the records equal."""
    p = gm.ModelParams()
    gm.load_library().gm_default_model_params(C.byref(p))
    p.n_seg, p.timestep = n_seg, timestep
    model = gm.ModelBlob(p)
    n, outs, taken = 32, [], []
    acts = np.random.default_rng(n_seg).uniform(-1, 1, size=(6, n, 4)).astype(np.float32)
    for lib in libs:
        old = os.environ.get("GM_DUO")
        os.environ["GM_DUO"] = "0"
        try:
            env = gm.BatchedGripperEnv(n, object_set="set6_synthetic", settings=gm.canonical_settings(noise=False, seed=7),
                                       seed=7, model_blob=model, lib=lib)
        finally:
            if old is None:
                os.environ.pop("GM_DUO", None)
            else:
                os.environ["GM_DUO"] = old
        try:
            assert env.model.nv == 3 * (n_seg + 2) + 8 and env.dispatch_info()["waves_per_env"] == 1
            env.reset()
            o = {}
            for t in range(5):
                obs, rew, term, _ = env.step(acts[t])
                o[f"obs{t}"], o[f"rew{t}"], o[f"done{t}"] = np.array(obs, copy=True), np.array(rew, copy=True), np.array(term, copy=True)
            o["states"] = env.env_states()
            env.set_action(acts[5])
            env.step_profiled()
            taken.append(int(env.decoupled_points.sum()))
            o["states_after_profiled_step"] = env.env_states()
            outs.append(o)
        finally:
            env.close()
    assert_same(outs[0], outs[1], f"N = {n_seg}")
    print(f"\nN = {n_seg}: decoupled first points in one env-step of {n} envs: {taken}")
    assert taken[0] > 0 and taken[1] == 0, taken


def test_duo_env_step_equals_one_wave(gm, sc, libs, batch):
    act = closing(gm, sc, len(batch.cases))
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
