"""The env-step readout on crafted states (tests/readout_cases.py) against an independent
restatement of the reference (tests/readout_model.py).

CPU: the oracle steps every case from its record and is compared with the model bit for bit
(rows, abs counts, last values, done, reward and cumulative reward as float32, the targets,
their step counts, the state readings); the model's branch trace is asserted to cover every
branch the table is there for; every physics value a case depends on is asserted clear of its
threshold by a relative 1e-4 (floor 1e-6); linear_reward and the caps have hand-computed
known answers.

GPU: each batch through set_env_states -> set_action / set_discrete_action -> action_step
against the oracle's batch_step (integers bit for bit, observations and reward under
test_grasp_parity's bounds) and against the model fed the device's own measured values (bit
for bit: the readout is compiled without contraction); the cap and termination batches once
more through gm_rollout's in-launch episode end against the per-step calls.

No case needed the f32 / f64 reward bound: every reward is bit-equal.  The one field held to
a tolerance is the cached finger angle end.th on the device (readout_cases.same_angle, 2 ulps;
measured on an MI355X: 1 ulp on one batch, 0 on the others).
"""
import numpy as np
import pytest

import contact_cases as cc
import readout_cases as rc
import readout_model as rm
from conftest import gpu_available

F = np.float32

REQUIRED = {
    "lifted:yes", "lifted:no", "lifted_to_height:yes", "lifted_to_height:no", "target_height:yes", "target_height:no",
    "object_stable:yes", "object_stable:no", "stable_height:yes", "within_XY:yes", "within_XY:no",
    "success_macro:triggered", "success_macro:row_short",
    "dropped:first", "dropped:lifted_again", "dropped:continues", "dropped:never_lifted",
    "termination:triggered", "termination:below_threshold", "termination:lift", "termination:no_lift",
    "terminated:lifted", "terminated:stable", "terminated:failed_not_lifted", "terminated:failed_not_stable",
    "fraction:clipped_low", "fraction:clipped_high",
    "cap:lower_clipped", "cap:upper_clipped", "cap:lower_off", "cap:upper_off",
    "done:lower_cap", "done:upper_cap", "done:inside_caps", "done:quit_without_cap",
    "done:binary:first", "done:binary:count", "done:binary:count_short", "done:linear:count", "done:linear:count_short",
    "reward:binary", "reward:binary_trigger_short", "row:binary_reset", "row:linear_reset",
    "active:not_above_min", "active:no_overshoot", "active:under_overshoot", "active:past_overshoot",
    "linear:below_min", "linear:rising", "linear:saturated", "linear:falling", "linear:past_overshoot",
    "peak_lateral:kept", "peak_lateral:raised", "palm:pressed_not_lifted", "palm:pressed_lifted",
    "limit:x_max", "limit:x_min", "limit:y_max", "limit:y_min", "limit:th_max", "limit:th_min", "limit:z_max", "limit:z_min",
    "limit:base_x_max", "limit:base_x_min", "limit:base_y_max", "limit:base_y_min", "limit:base_z_max", "limit:base_z_min",
    "limit:base_yaw_max", "limit:base_yaw_min", "limit:fingertip_min", "exceed_limits:set", "exceed_limits:latched",
    "normalise:inside", "normalise:above", "normalise:below", "normalise:at_max", "normalise:at_min",
} | {f"oob:{a}:{b}" for a in ("x_high", "x_low", "y_high", "y_low") for b in ("out", "in")} \
  | {f"code:{n}:{sub}" for n in rm.ACTION_NAMES for sub in ("positive", "negative", "continous")
     if sub != "continous" or n in ("gripper_prismatic_X", "gripper_revolute_Y", "gripper_Z", "base_Z")}


class Built:
    """One batch: records, actions, and the oracle's steps from them (shared, read-only)."""

    def __init__(self, gm, sc, batch):
        import oracle_lib as ol
        self.batch = batch
        self.cfg, self.objs, self.recs, self.acts = rc.build(gm, sc, batch)
        self.steps = []                      # (before, action, obs, rew, done, after) per env-step
        before = self.recs
        for k in range(batch.steps):
            act = self.action(k)
            kw = dict(discrete=act) if batch.discrete else dict(actions=act)
            obs, rew, done, after = ol.batch_step(sc.model, self.cfg, self.objs, before, **kw)
            for a in (obs, rew, done, after):
                a.setflags(write=False)
            self.steps.append((before, act, obs, rew, done, after))
            before = after
        self.recs.setflags(write=False)

    def action(self, k):
        if k == 0:
            return self.acts
        return np.zeros_like(self.acts)     # a second env-step repeats code 0 / sends zero fractions


_built = {}


@pytest.fixture(scope="module")
def table(gm):
    if "sc" not in _built:
        _built["sc"] = cc.Scene(gm, 8)
        _built["batches"] = {b.name: b for b in rc.make_batches(gm, _built["sc"])}

    def get(name):
        if name not in _built:
            _built[name] = Built(gm, _built["sc"], _built["batches"][name])
        return _built[name]
    get.sc = _built["sc"]
    get.names = list(_built["batches"])
    return get


BATCHES = ["chain", "blocked", "term_stable", "term_lifted", "discrete", "caps", "caps_quit", "quit_nocap", "linear",
           "grasp", "sensors_all", "sensors_one"]


def model_on(gm, sc, t, k, after_records, traces=None):
    """The model for env-step k of a batch, fed the measured values of after_records."""
    before, act = t.steps[k][0], t.steps[k][1]
    bv, av = gm.env_state_view(before), gm.env_state_view(after_records)
    outs = []
    for i, c in enumerate(t.batch.cases):
        tr = set()
        outs.append(rc.model_step(gm, sc, t.batch, t.cfg, bv[i], av[i], act[i], tr, palm=c.palm))
        if traces is not None:
            traces.append(tr)
    return outs


def test_known_answers():
    """linear_reward and the caps with the reference's default numbers, worked by hand."""
    lr = rm.linear_reward
    assert lr(4.5, 1, 3, 6) == F(0.5)          # palm_force 1 / 3 / 6: halfway down the falling ramp
    assert lr(2.0, 1, 3, 6) == F(0.5)          # halfway up the rising ramp
    assert lr(0.5, 1, 3, 6) == 0 and lr(6.5, 1, 3, 6) == 0 and lr(3.0, 1, 3, 6) == 1 and lr(6.0, 1, 3, 6) == 0
    assert lr(7.0, 2, 6, -1) == 1 and lr(3.0, 2, 6, -1) == F(0.25)       # exceed_axial 2 / 6 / -1
    assert lr(-0.1025, -0.2, -5e-3, -1) == F(F(F(-0.1025) - F(-0.2)) / F(F(-5e-3) - F(-0.2)))
    assert rm.normalise_between(91.5e-3, 49e-3, 134e-3) == F(F(F(2) * F(F(91.5e-3) - F(49e-3))) / F(F(134e-3) - F(49e-3))) - F(1)
    assert abs(float(rm.normalise_between(91.5e-3, 49e-3, 134e-3))) < 1e-6

    class S:                                    # the defaults of simsettings.h:74-77
        cap_reward, quit_if_cap_exceeded, reward_cap_lower_bound, reward_cap_upper_bound = 1, 1, -1.0, 1.0

        class step_num:
            reward, done, trigger = -0.01, 0, 1

        class oob:
            reward, done, trigger = -1.0, 1, 1
    s = S()
    # oob fires at cumulative -0.5: -0.01 - 1 = -1.01 would leave -1.51, the cap returns -0.5
    r, c = rm.reward(s, {"step_num": 1, "oob": 1}, {}, {}, F(-0.5), ["step_num", "oob"], [])
    assert c == F(-1.0) and r == F(F(F(-0.01) + F(-1.0)) + F(F(-1.0) - F(F(-0.5) + F(F(-0.01) + F(-1.0)))))
    assert abs(float(r) + 0.5) < 1e-6
    r, c = rm.reward(s, {"step_num": 1, "oob": 0}, {}, {}, F(-0.5), ["step_num", "oob"], [])
    assert r == F(-0.01) and c == F(F(-0.5) + F(-0.01))
    # is_done looks at the cumulative reward of before this step's reward(): -1 is done, -0.99 is not
    assert rm.is_done(s, {"step_num": 1, "oob": 0}, {}, F(-1.0), ["step_num", "oob"], [])
    assert not rm.is_done(s, {"step_num": 1, "oob": 0}, {}, F(-0.99), ["step_num", "oob"], [])
    assert rm.is_done(s, {"step_num": 1, "oob": 0}, {}, F(-0.999995), ["step_num", "oob"], [])     # within ftol of the bound
    assert rm.is_done(s, {"step_num": 1, "oob": 0}, {}, F(1.0), ["step_num", "oob"], [])
    assert rm.is_done(s, {"step_num": 0, "oob": 1}, {}, F(0.0), ["step_num", "oob"], [])


def test_model_configuration_matches(gm, table):
    """The model's action list, base limits and observation length against gm_configure's."""
    sc = table.sc
    for name in table.names:
        b = _built["batches"][name]
        cfg = gm.ConfigBlob(b.settings, sc.model)
        c = rc.config_view(gm, cfg)
        opts = rm.action_options(b.settings)
        assert c.n_actions == len(opts) and list(c.action_options[:len(opts)]) == opts, name
        assert tuple(c.base_min) == rm.BASE_MIN and tuple(c.base_max) == rm.BASE_MAX, name
        assert cfg.n_obs == rm.n_obs(b.settings), (name, cfg.n_obs, rm.n_obs(b.settings))
    assert rm.n_streams(_built["batches"]["sensors_all"].settings) == 29
    assert rm.n_streams(_built["batches"]["sensors_one"].settings) == 1
    # raw sampling, wrist Z at another read rate than wrist XY: Z is still sampled with XY's counts
    s = rc.s_sensors(gm)
    s.sensor_sample_mode = 0
    s.wrist_sensor_Z.read_rate = 25.0
    assert gm.ConfigBlob(s, sc.model).n_obs == rm.n_obs(s)
    s.wrist_sensor_XY.read_rate = 20.0
    assert gm.ConfigBlob(s, sc.model).n_obs == rm.n_obs(s)


def physics_margins(gm, sc, t, k):
    """(case, what, value, threshold) for every physics value of env-step k that a rule of
    the model compares with a threshold."""
    s = t.batch.settings
    before, after = gm.env_state_view(t.steps[k][0]), gm.env_state_view(t.steps[k][5])
    le = gm.LINEAR_EVENTS
    out = []
    for i, c in enumerate(t.batch.cases):
        ll = {n: float(after["lev_last"][i][j]) for j, n in enumerate(le)}
        q = after["qpos"][i][sc.qadr_obj:sc.qadr_obj + 3]
        lift = max(0.0, float(F(q[2] - before["start_qpos"][i][2])))
        dist = float(F(np.hypot(after["base"][i][0] - q[0], after["base"][i][1] - q[1])))
        pairs = [("ground force / ftol", ll["ground_force"], rm.FTOL), ("lift / lift_height", lift, s.lift_height - rm.FTOL),
                 ("XY distance", dist, s.XY_distance_threshold)]
        if any(b.startswith("palm:pressed") for b in c.branches):
            pairs += [("palm axial force / 0", ll["exceed_palm"], 0.0), ("palm axial force / ftol", ll["exceed_palm"], rm.FTOL)]
        pairs += [(f"finger {j} force / ftol", ll[f"finger{j}_force"], rm.FTOL) for j in (1, 2, 3)]
        pairs += [(f"finger {j} force / stable", ll[f"finger{j}_force"], s.stable_finger_force) for j in (1, 2, 3)]
        pairs += [(f"oob {ax}{sg:+d}", float(q[a]), sg * s.oob_distance) for a, ax in ((0, "x"), (1, "y")) for sg in (1, -1)]
        for n in le:
            e = getattr(s, n)
            if n.startswith("action_penalty") or not (e.reward or e.done):
                continue
            pairs += [(f"{n} / min", ll[n], e.min)]
            if e.reward:
                pairs += [(f"{n} / max", ll[n], e.max)]
            if e.overshoot >= 0:
                pairs += [(f"{n} / overshoot", ll[n], e.overshoot)]
        out += [(c.name, w, v, th) for w, v, th in pairs]
    return out


@pytest.mark.parametrize("name", BATCHES)
def test_oracle_matches_model(gm, table, name):
    t, sc = table(name), table.sc
    for k in range(t.batch.steps):
        before, act, obs, rew, done, after = t.steps[k]
        traces = []
        outs = model_on(gm, sc, t, k, after, traces)
        av = gm.env_state_view(after)
        for i, c in enumerate(t.batch.cases):
            who = f"{name} / {c.name} / step {k}"
            rc.compare_with_model(gm, outs[i], av[i], "oracle, " + who)
            assert F(rew[i]).tobytes() == F(outs[i]["reward"]).tobytes() and int(done[i]) == int(outs[i]["done"]), who
            if k == 0:
                missing = [b for b in c.branches if b not in traces[i]]
                assert not missing, f"{who}: the case does not take its own branch {missing}; took {sorted(traces[i])}"
        bad = [(n, w, v, th) for n, w, v, th in physics_margins(gm, sc, t, k) if not rc.margin_ok(v, th)]
        assert not bad, f"{name}, step {k}: physics values too close to a threshold {bad}"
        _built.setdefault("traces", {})[(name, k)] = set().union(*traces)
    assert obs.shape[1] == rm.n_obs(t.batch.settings)


def test_table_covers_every_branch(gm, table):
    """Every branch of REQUIRED is taken by at least one case (the model's trace)."""
    seen = set()
    for name in BATCHES:
        t = table(name)
        for k in range(t.batch.steps):
            traces = []
            model_on(gm, table.sc, t, k, t.steps[k][5], traces)
            seen |= set().union(*traces)
    missing = sorted(REQUIRED - seen)
    assert not missing, f"branches no case takes: {missing}"
    # the cap cases by construction: the step's reward crosses each bound, starts at it, stays inside
    t = table("caps")
    cum0 = gm.env_state_view(t.recs)["cumulative_reward"]
    cum1 = gm.env_state_view(t.steps[0][5])["cumulative_reward"]
    lo, hi = F(t.batch.settings.reward_cap_lower_bound), F(t.batch.settings.reward_cap_upper_bound)
    rew = t.steps[0][3]
    by = {c.name: i for i, c in enumerate(t.batch.cases)}
    for nm, bound, step_reward in (("lower", lo, -0.01), ("upper", hi, 0.02)):
        i = by[f"crossing the {nm} bound"]
        assert cum0[i] != bound and cum1[i] == bound and 0 < abs(rew[i]) < abs(step_reward) - 1e-3
        i = by[f"at the {nm} bound"]
        assert cum0[i] == bound and cum1[i] == bound and abs(rew[i]) < 1e-6
        i = by[f"inside the {nm} bound"]
        assert lo < cum1[i] < hi and abs(rew[i] - step_reward) < 1e-6
    # quit_if_cap_exceeded: at the bound done at once; crossing: not this step, the next
    t = table("caps_quit")
    d0, d1 = t.steps[0][4], t.steps[1][4]
    for nm in ("lower", "upper"):
        assert d0[by[f"at the {nm} bound"]] == 1
        assert d0[by[f"crossing the {nm} bound"]] == 0 and d1[by[f"crossing the {nm} bound"]] == 1
        assert d0[by[f"inside the {nm} bound"]] == 0
    assert not table("quit_nocap").steps[0][4].any()
    assert not table("caps").steps[0][4].any() and not table("caps").steps[1][4].any()


# ---------------------------------------------------------------- GPU
INT_FIELDS = ("bev_row", "bev_abs", "bev_last", "lev_row", "lev_abs", "num_action_steps", "old_x", "old_y", "old_z",
              "lock_active", "rng", "ring_i", "termination_signal_sent", "done", "extra_substeps")


def make_env(gm, sc, t):
    return gm.BatchedGripperEnv(len(t.batch.cases), settings=t.batch.settings, seed=3, model_blob=sc.model, objects=t.objs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", BATCHES)
def test_device_matches_oracle_and_model(gm, table, name):
    if not gpu_available():
        pytest.skip("no GPU")
    from test_grasp_parity import OBS_ATOL, OBS_RTOL, obs_err
    t, sc = table(name), table.sc
    env = make_env(gm, sc, t)
    dev = []
    try:
        env.set_env_states(t.recs)
        for k in range(t.batch.steps):
            act = t.steps[k][1]
            if t.batch.discrete:
                env.set_discrete_action(act)
            else:
                env.set_action(act)
            env.action_step()
            obs, rew, done = env.outputs()
            dev.append((obs, rew, done.astype(np.uint8), env.env_states()))
    finally:
        env.close()
    assert env.n_obs == rm.n_obs(t.batch.settings)
    for k, (obs, rew, done, after) in enumerate(dev):
        _, _, obs_o, rew_o, done_o, after_o = t.steps[k]
        dv, ov = gm.env_state_view(after), gm.env_state_view(after_o)
        rel, ab = obs_err(obs, obs_o)
        dth = np.abs(dv["end"]["th"] - ov["end"]["th"]) / np.spacing(np.maximum(np.abs(ov["end"]["th"]), 1e-300))
        print(f"\n{name}, step {k}: obs worst rel {rel.max():.3e} abs {ab.max():.3e}, "
              f"reward worst |d| {np.abs(rew - rew_o).max():.3e}, finger angle worst {dth.max():.1f} ulp")
        # ---- the oracle, from the same records
        for i, c in enumerate(t.batch.cases):
            who = f"{name} / {c.name} / step {k}"
            assert rel[i] <= OBS_RTOL and ab[i] <= OBS_ATOL, f"{who}: observation rel {rel[i]:.3e} abs {ab[i]:.3e}"
            assert done[i] == done_o[i], f"{who}: done {done[i]} vs oracle {done_o[i]}"
            for f in INT_FIELDS:
                assert np.array_equal(dv[f][i], ov[f][i]), f"{who}: {f} {dv[f][i]} vs oracle {ov[f][i]}"
            for g in ("end", "next"):
                for f in ("sx", "sy", "sz"):
                    assert dv[g][f][i] == ov[g][f][i], f"{who}: {g}.{f}"
            for f in ("x", "y", "z"):
                assert dv["end"][f][i] == ov["end"][f][i], f"{who}: end.{f}"
            assert rc.same_angle(float(dv["end"]["th"][i]), float(ov["end"]["th"][i]), rc.TH_ULPS), \
                f"{who}: end.th {dv['end']['th'][i]!r} vs oracle {ov['end']['th'][i]!r}"
            assert np.array_equal(dv["base"][i], ov["base"][i]), f"{who}: base target"
        np.testing.assert_allclose(rew, rew_o, rtol=1e-5, atol=1e-6, err_msg=f"{name}, step {k}: reward")
        # ---- the model, fed the device's own measured values (step k's prior state is the
        # device's own record where k > 0)
        before = t.steps[k][0] if k == 0 else dev[k - 1][3]
        bv = gm.env_state_view(before)
        for i, c in enumerate(t.batch.cases):
            who = f"device, {name} / {c.name} / step {k}"
            out = rc.model_step(gm, sc, t.batch, t.cfg, bv[i], dv[i], t.steps[k][1][i], set(), palm=c.palm)
            rc.compare_with_model(gm, out, dv[i], who, th_ulps=rc.TH_ULPS)
            assert F(rew[i]).tobytes() == F(out["reward"]).tobytes(), f"{who}: returned reward {rew[i]!r} vs {out['reward']!r}"
            assert int(done[i]) == int(out["done"]), f"{who}: returned done"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["caps_quit", "term_stable", "term_lifted"])
def test_fused_rollout_from_crafted_records_equals_per_step(gm, table, name):
    """gm_rollout's in-launch episode end sees the same done: two env-steps of the random
    driver from the crafted records equal the per-step calls (gmx.random_fractions ->
    set_action -> action_step -> the device auto-reset) bit for bit."""
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    t, sc = table(name), table.sc
    n = len(t.batch.cases)
    seed, max_ep, K = 16, 250, 2       # seed 16: the random driver's termination fraction is above 0.9 for two envs at step 0
    a, b = make_env(gm, sc, t), make_env(gm, sc, t)
    try:
        ra = torch.zeros((K, n, 3), dtype=torch.int32, device="cuda")
        rb = torch.zeros((K, n, 3), dtype=torch.int32, device="cuda")
        a.set_env_states(t.recs)
        a.rollout(K, action_mode=1, seed=seed, max_episode_steps=max_ep, records_dev_ptr=ra.data_ptr())
        b.set_env_states(t.recs)
        dones = []
        for k in range(K):
            v = gm.env_state_view(b.env_states())
            fr = gm.random_fractions(seed, np.arange(n), v["episode"], v["num_action_steps"], b.n_actions)
            b.set_action(fr)
            b.action_step()
            dones.append(b.reward_done()[1].copy())
            b.autoreset_device(0, None, max_episode_steps=max_ep, episodes_dev_ptr=rb[k].data_ptr())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(ra.cpu().numpy(), rb.cpu().numpy(), err_msg="episode-end records")
        va, vb = gm.env_state_view(a.env_states()), gm.env_state_view(b.env_states())
        for f in va.dtype.names:
            np.testing.assert_array_equal(va[f], vb[f], err_msg=f)
        oa, ob = a.outputs(), b.outputs()
        for x, y, w in zip(oa, ob, ("observations", "rewards", "done flags")):
            np.testing.assert_array_equal(x, y, err_msg=w)
        ep0 = gm.env_state_view(t.recs)["episode"]
        if name != "caps_quit":
            v0 = gm.env_state_view(t.recs)
            fr0 = gm.random_fractions(seed, np.arange(n), v0["episode"], v0["num_action_steps"], b.n_actions)
            sent = fr0[:, -1] > F(t.batch.settings.termination_threshold)
            assert sent.sum() >= 2 and not sent.all()
            # a termination ends the episode (stable / lifted / failed termination all have done = 1)
            assert np.array_equal(dones[0], sent) and np.array_equal(va["episode"] > ep0, sent | dones[1])
        if name == "caps_quit":
            # the envs that start at a bound end their episode inside the launch
            by = {c.name: i for i, c in enumerate(t.batch.cases)}
            for nm in ("at the lower bound", "at the upper bound"):
                assert dones[0][by[nm]] and va["episode"][by[nm]] > ep0[by[nm]], nm
    finally:
        a.close()
        b.close()
