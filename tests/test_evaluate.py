"""The evaluation launch (include/gripper_mi355x.h gm_evaluate and the like; gmx/eval.py): every
active env runs one episode and retires from the work queue.  Its reports must equal, bit for
bit, (1) values latched by a per-step loop that uses none of the new calls, and (2) the per-step
sequence act -> gm_step -> gm_eval_record -> gm_autoreset_episodes for every driver; the envs
must be left parked at their terminal states with nothing recorded anywhere; the queue must be
left fit for a training rollout; the grasp program's reports must agree with the fp64 oracle;
gmx.Evaluator must be the waves done by hand; and bad arguments must be refused.

The episodes are staggered by construction: env e starts with num_action_steps = e % 4 and every
fifth env's object is spawned out of bounds (done at its first env-step), so with max_ep = 7 the
lengths are 1..4 and 7 and both end codes occur.  Every third env is inactive."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

N, MAX_EP, SEED, PSEED, DEC0 = 96, 7, 41, 9, 1000
SENTINEL = -7
HANDOFF = {"GM_CHUNK_SUBSTEPS": "1", "GM_CHUNK_MARGIN": "0", "GM_CHUNK_YIELDS": "60", "GM_CHUNK_CMARGIN": "0",
           "GM_CHUNK_GRID": "24"}
# (96 envs get DUO workgroups by default; "one-wave" runs the kernels a 4096-env batch runs)
DISPATCH = {"default": None, "handoff-heavy": HANDOFF, "one-wave": {"GM_DUO": "0"},
            "one-wave-handoff": dict(HANDOFF, GM_DUO="0"), "one-shot": {"GM_CHUNK_SUBSTEPS": "0"}}
FIELDS = ("ret", "length", "end", "rows", "abs", "last")
ACTIVE = (np.arange(N) % 3 != 2)                                 # every third env is inactive


def make_env(gm, env_vars=None, n=N, discrete=False):
    # (no scene spawn search: the out-of-bounds spawns below must stay where the table puts them)
    s = gm.canonical_settings(noise=True, seed=SEED)
    if discrete:
        s.continous_actions = 0
    old = {k: os.environ.get(k) for k in (env_vars or {})}
    os.environ.update(env_vars or {})
    try:
        env = gm.BatchedGripperEnv(n, object_set="set6_synthetic", settings=s, seed=SEED)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    env.reset()
    return env


# ---------------------------------------------------------------- the drivers, per step and fused
class Driver:
    """One agent on one env: act(k), the per-step half, and evaluate(**kw), the launch."""

    def __init__(self, gm, kind, env):
        from gmx.policy import DevicePolicy
        from gmx.ppo import DeviceActorCritic, DeviceCategoricalActorCritic, TrajectoryBuffer
        from gmx.sac import DeviceSAC
        self.kind, self.env, self.agent, self.traj = kind, env, None, None
        if kind == "dqn":
            self.agent = DevicePolicy(env, seed=3)
        elif kind in ("ppo-sample", "ppo-mean"):
            self.agent = DeviceActorCritic(env, hidden=(64, 64), seed=3)
            self.traj = TrajectoryBuffer(env, 1)
        elif kind == "cat":
            self.agent = DeviceCategoricalActorCritic(env, hidden=(64, 64), seed=3)
            self.traj = TrajectoryBuffer(env, 1, act_dim=1)
        elif kind == "sac-mean":
            self.agent = DeviceSAC(env, hidden=(64, 64), seed=3)

    @staticmethod
    def discrete(kind):
        return kind in ("dqn", "cat")

    def act(self, k):
        env, lib = self.env, self.env.lib
        if self.kind == "dqn":
            self.agent.act(0.0, seed=PSEED, decision=DEC0 + k)
        elif self.kind in ("ppo-sample", "ppo-mean", "cat"):
            self.agent.act(self.traj, 0, sample=self.kind != "ppo-mean", noise=0.0, seed=PSEED, decision=DEC0 + k)
        elif self.kind == "sac-mean":
            self.agent.act("mean", seed=PSEED, decision=DEC0 + k)
        else:
            d_act = C.c_void_p(lib.gm_device_actions(env.ctx))
            if self.kind == "script-1":
                env._check(lib.gm_random_actions(env.ctx, PSEED, d_act, 1))
            else:
                env._check(lib.gm_program_actions(env.ctx, PSEED, C.c_float(0.2), 3, d_act, 1))
            env._check(lib.gm_set_action(env.ctx, d_act, 1))

    def evaluate(self, **kw):
        if self.kind == "dqn":
            return self.agent.evaluate(seed=PSEED, decision0=DEC0, **kw)
        if self.kind in ("ppo-sample", "ppo-mean", "cat"):
            return self.agent.evaluate(sample=self.kind != "ppo-mean", seed=PSEED, decision0=DEC0, **kw)
        if self.kind == "sac-mean":
            return self.agent.evaluate("mean", seed=PSEED, decision0=DEC0, **kw)
        return self.env.evaluate(action_mode=1 if self.kind == "script-1" else 3, seed=PSEED, jitter=0.2, **kw)

    def close(self):
        if self.agent is not None:
            self.agent.close()
        self.env.close()


def stagger(gm, drv):
    """One warm env-step (the hand-off dispatch needs the costs a context records from its first
    env-step on), then the staggered start: every fifth env's object out of bounds, env e at
    num_action_steps = e % 4.  Returns the state records the evaluation starts from."""
    env = drv.env
    drv.act(0)
    env.lib.gm_step(env.ctx)
    env.reset(spawn=env.make_spawn(x=np.where(np.arange(env.n_envs) % 5 == 0, 0.09, 0.0), y=0.0, rot=0.0))
    st = env.env_states()
    gm.env_state_view(st)["num_action_steps"][:] = np.arange(env.n_envs) % 4
    env.set_env_states(st)
    return env.env_states()


def sentinel_report(gm, env):
    import torch
    rep = gm.new_report(env)
    for t in rep.values():
        t.fill_(SENTINEL if t.dtype != torch.uint8 else 200)
    torch.cuda.synchronize()
    return rep


def host(rep):
    return {k: v.cpu().numpy() for k, v in rep.items()}


def expected_inactive(rep_host):
    """What the sentinel report holds for the inactive envs after a launch: end = 0, the rest untouched."""
    for f in FIELDS:
        want = 0 if f == "end" else SENTINEL
        np.testing.assert_array_equal(rep_host[f][~ACTIVE], np.full_like(rep_host[f][~ACTIVE], want), err_msg=f)


def latched_reference(gm, drv):
    """The per-step loop with calls the evaluation adds nothing to: act -> gm_step -> read the
    event rows, the state records and the done flags -> auto-reset; each active env's values are
    latched at its first end.  Returns (report arrays, the state record of each env at its end)."""
    env = drv.env
    W = len(gm.EVENT_NAMES)
    rep = dict(ret=np.full(N, SENTINEL, np.float32), length=np.full(N, SENTINEL, np.int32), end=np.full(N, 200, np.uint8),
               rows=np.full((N, W), SENTINEL, np.int32), abs=np.full((N, W), SENTINEL, np.int32),
               last=np.full((N, W), SENTINEL, np.float32))
    rep["end"][~ACTIVE] = 0
    end_states = env.env_states()
    open_ = ACTIVE.copy()
    for k in range(MAX_EP):
        drv.act(k)
        env.lib.gm_step(env.ctx)
        rows, absc, last = env.event_rows()
        raw = env.env_states()
        st = gm.env_state_view(raw)
        _, done = env.reward_done()
        end = np.where(done, 1, np.where(st["num_action_steps"] >= MAX_EP, 2, 0)).astype(np.uint8)
        now = open_ & (end != 0)
        rep["ret"][now], rep["length"][now], rep["end"][now] = st["cumulative_reward"][now], st["num_action_steps"][now], end[now]
        rep["rows"][now], rep["abs"][now], rep["last"][now] = rows[now], absc[now], last[now]
        end_states[now] = raw[now]
        open_ &= ~now
        env.autoreset_device(0, None, max_episode_steps=MAX_EP)
    assert not open_.any(), "every active env ends within max_ep env-steps"
    return rep, end_states


@pytest.fixture(scope="module")
def dqn_reference(gm):
    """The DQN reference, computed once: (reports, end-state records, start-state records)."""
    if not gpu_available():
        pytest.skip("no GPU")
    drv = Driver(gm, "dqn", make_env(gm, discrete=True))
    try:
        start = stagger(gm, drv)
        rep, end_states = latched_reference(gm, drv)
    finally:
        drv.close()
    # the staggering worked, judged on the reference alone
    assert len(np.unique(rep["length"][ACTIVE])) >= 4, np.unique(rep["length"][ACTIVE])
    assert set(np.unique(rep["end"][ACTIVE])) == {1, 2}
    return rep, end_states, start


# ---------------------------------------------------------------- 1. independent reference
@pytest.mark.parametrize("dispatch", list(DISPATCH))
def test_policy_evaluate_equals_latched_per_step_values(gm, dqn_reference, dispatch):
    ref, _, start = dqn_reference
    drv = Driver(gm, "dqn", make_env(gm, DISPATCH[dispatch], discrete=True))
    try:
        np.testing.assert_array_equal(stagger(gm, drv), start)      # identically prepared
        out = sentinel_report(gm, drv.env)
        got = host(drv.evaluate(max_episode_steps=MAX_EP, active=ACTIVE, out=out))
        for f in FIELDS:
            np.testing.assert_array_equal(got[f], ref[f], err_msg=f)
        expected_inactive(got)
        info = drv.env.dispatch_info()
        assert (info["chunk"] == 0) == (dispatch == "one-shot")
        if dispatch in ("default", "one-wave", "one-wave-handoff"):
            assert info["waves_per_env"] == (2 if dispatch == "default" else 1)
        if "handoff" in dispatch:
            assert drv.env.chunk_stats()["yields"] > 0
    finally:
        drv.close()


# ---------------------------------------------------------------- 2. fused equals per-step with gm_eval_record
def per_step_evaluation(gm, drv):
    """act -> gm_step -> gm_eval_record -> gm_autoreset_episodes, max_ep times."""
    import torch
    env = drv.env
    out = sentinel_report(gm, env)
    out["end"][torch.from_numpy(~ACTIVE).to(out["end"].device)] = 0
    act = torch.from_numpy(ACTIVE.astype(np.uint8)).to(out["end"].device)
    torch.cuda.synchronize()
    for k in range(MAX_EP):
        drv.act(k)
        env.lib.gm_step(env.ctx)
        env.eval_record(act, out, max_episode_steps=MAX_EP)
        env.autoreset_device(0, None, max_episode_steps=MAX_EP)
    torch.cuda.synchronize()
    assert int(act.sum()) == 0, "every active env reported"
    return host(out)


@pytest.mark.parametrize("dispatch", ["default", "handoff-heavy", "one-wave"])
@pytest.mark.parametrize("kind", ["dqn", "ppo-sample", "ppo-mean", "cat", "sac-mean", "script-1", "script-3"])
def test_fused_evaluation_equals_per_step_sequence(gm, kind, dispatch):
    if not gpu_available():
        pytest.skip("no GPU")
    a = Driver(gm, kind, make_env(gm, discrete=Driver.discrete(kind)))
    b = Driver(gm, kind, make_env(gm, DISPATCH[dispatch], discrete=Driver.discrete(kind)))
    try:
        np.testing.assert_array_equal(stagger(gm, a), stagger(gm, b))
        ref = per_step_evaluation(gm, a)
        got = host(b.evaluate(max_episode_steps=MAX_EP, active=ACTIVE, out=sentinel_report(gm, b.env)))
        for f in FIELDS:
            np.testing.assert_array_equal(got[f], ref[f], err_msg=f)
        expected_inactive(got)
        assert set(np.unique(got["end"][ACTIVE])) == {1, 2}
        assert len(np.unique(got["length"][ACTIVE])) >= 4
        assert b.env.dispatch_info()["chunk"] > 0
        if dispatch != "handoff-heavy":
            assert b.env.dispatch_info()["waves_per_env"] == (1 if dispatch == "one-wave" else 2)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 3. envs really retire
def test_envs_retire_at_their_terminal_state_and_nothing_is_recorded(gm, dqn_reference):
    import torch
    from gmx.policy import ReplayBuffer
    ref, end_states, start = dqn_reference
    drv = Driver(gm, "dqn", make_env(gm, discrete=True))
    try:
        env = drv.env
        buf = ReplayBuffer(env, 2 * N)
        np.testing.assert_array_equal(stagger(gm, drv), start)
        for f in ("state", "action", "next_state", "reward", "end"):
            getattr(buf, f).fill_(3)                    # a memory with recognisable rows ...
        drv.agent.push_begin(buf)                       # ... that the agent has pushed into
        torch.cuda.synchronize()
        before_buf = {f: getattr(buf, f).clone() for f in ("state", "action", "next_state", "reward", "end")}
        got = host(drv.evaluate(max_episode_steps=MAX_EP, active=ACTIVE))
        np.testing.assert_array_equal(got["length"][ACTIVE], ref["length"][ACTIVE])
        assert env.chunk_stats()["finished"] == N
        assert env.dispatch_info()["last_launch_env_steps"] == MAX_EP
        # the diagnostics: an inactive env's job has no clocks and ended when it was picked
        clk, yields = env.job_stats()
        assert (clk[ACTIVE] > 0).all() and (clk[~ACTIVE] == 0).all() and (yields[~ACTIVE] == 0).all()
        _, _, ev = env.chunk_timeline()
        np.testing.assert_array_equal(ev[~ACTIVE, 0], ev[~ACTIVE, 1])
        assert (ev[ACTIVE, 1] > ev[ACTIVE, 0]).all()
        raw = env.env_states()
        st, want, st0 = gm.env_state_view(raw), gm.env_state_view(end_states), gm.env_state_view(start)
        # every active env is parked at its end step, before any reset; the others were not touched
        for f in st.dtype.names:
            np.testing.assert_array_equal(st[f][ACTIVE], want[f][ACTIVE], err_msg=f)
        np.testing.assert_array_equal(raw[~ACTIVE], start[~ACTIVE])
        np.testing.assert_array_equal(st["num_action_steps"][ACTIVE], got["length"][ACTIVE])
        np.testing.assert_array_equal(st["episode"], st0["episode"])
        for f, t in before_buf.items():
            assert torch.equal(getattr(buf, f), t), f
        assert buf.pushed == 0
    finally:
        drv.close()


def test_actor_critic_evaluation_leaves_a_trajectory_buffer_alone(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    drv = Driver(gm, "ppo-sample", make_env(gm))
    try:
        traj = drv.traj                                  # the one-row buffer the agent has acted into
        stagger(gm, drv)
        names = ("obs", "act", "logp", "val", "rew", "end", "boot", "last_val", "mu")
        before = {f: getattr(traj, f).clone() for f in names}
        assert float(before["logp"].abs().sum()) > 0     # (the warm env-step's act wrote the row)
        got = host(drv.evaluate(max_episode_steps=MAX_EP, active=ACTIVE))
        assert set(np.unique(got["end"][ACTIVE])) == {1, 2}
        for f in names:
            assert torch.equal(getattr(traj, f), before[f]), f
    finally:
        drv.close()


# ---------------------------------------------------------------- 4. the dispatch cost table
def test_rollout_after_an_evaluation_equals_one_after_the_per_step_sequence(gm):
    """A fused evaluation leaves the queue and its cost table fit for a training rollout: from the
    same state records the next rollout gives the results it gives on a context whose evaluation
    ran as the per-step sequence."""
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    K, mx = 4, 3
    a, b = Driver(gm, "script-3", make_env(gm)), Driver(gm, "script-3", make_env(gm))
    try:
        np.testing.assert_array_equal(stagger(gm, a), stagger(gm, b))
        ref = per_step_evaluation(gm, a)
        got = host(b.evaluate(max_episode_steps=MAX_EP, active=ACTIVE, out=sentinel_report(gm, b.env)))
        for f in FIELDS:
            np.testing.assert_array_equal(got[f], ref[f], err_msg=f)
        snaps = []
        ra, rb = (torch.zeros((K, N, 3), dtype=torch.int32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        for drv, rec in ((a, ra), (b, rb)):
            env = drv.env
            env.reset(spawn=env.make_spawn(idx=np.arange(N) % len(env.objects), x=0.0, y=0.0, rot=0.0))
            if drv is b:
                env.set_env_states(snaps[0][0])          # the same records (episode counters, RNG streams)
            start = env.env_states()
            env.rollout(K, action_mode=0, seed=PSEED, max_episode_steps=mx, records_dev_ptr=rec.data_ptr())
            torch.cuda.synchronize()
            rew, done = env.reward_done()
            snaps.append((start, env.env_states(), env.observation(), rew, done, rec.cpu().numpy(), env.chunk_stats(),
                          env.dispatch_info(), env.job_stats()))
        sa, sb = snaps
        for i in range(6):
            np.testing.assert_array_equal(sa[i], sb[i], err_msg=str(i))
        for s in snaps:
            assert s[6]["finished"] == N and s[6]["started"] == N, s[6]
            assert s[7]["last_launch_env_steps"] == K
            assert (s[8][0] > 0).all()                   # every env's job ran and recorded its clocks
        assert int(gm.env_state_view(sb[1])["episode"].min()) > int(gm.env_state_view(sb[0])["episode"].min())
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 5. against the oracle
def test_program_evaluation_agrees_with_the_oracle(gm):
    """env.evaluate(action_mode=3) on the centred set6 objects of test_distributed.program_records
    (spheres on even ids: carried to successful_grasp; a box on odd ids: squeezed, not carried)."""
    if not gpu_available():
        pytest.skip("no GPU")
    import oracle_lib
    n, mx = 4, 110
    s = gm.canonical_settings(noise=False, seed=5)
    env = gm.BatchedGripperEnv(n, object_set="set6_synthetic", settings=s, seed=1234)
    try:
        objs = env.objects
        spheres = [i for i in range(len(objs)) if objs[i].type == 2 and objs[i].size[0] > 0.02]
        boxes = [i for i in range(len(objs)) if objs[i].type == 6]
        idx = [spheres[g // 2 % len(spheres)] if g % 2 == 0 else boxes[0] for g in range(n)]
        sp = env.make_spawn(idx=idx, x=0.0, y=0.0, rot=0.0)
        env.reset(spawn=sp)
        got = host(env.evaluate(action_mode=3, seed=5, max_episode_steps=mx))
        nb = len(gm.BINARY_EVENTS)
        i_succ = list(gm.BINARY_EVENTS).index("successful_grasp")
        ret, length, absb = [], [], []
        for g in range(n):
            o = oracle_lib.OracleEnv(env.model, env.cfg, objs, g)
            o.reset(sp[g])
            tot = np.float32(0.0)
            for k in range(mx):
                o.set_action(o.driver_actions(mode=3, seed=5, gid=g))
                o.action_step()
                d, r = o.is_done(), o.reward()
                tot = np.float32(tot + np.float32(r))
                if d:
                    break
            ret.append(tot)
            length.append(k + 1)
            absb.append(o.event_rows()[1][:nb])
        np.testing.assert_array_equal(got["length"], length)
        np.testing.assert_array_equal((got["abs"][:, i_succ] > 0).astype(int), [1, 0, 1, 0])
        np.testing.assert_array_equal(got["abs"][:, :nb], np.array(absb))
        np.testing.assert_allclose(got["ret"], np.array(ret, dtype=np.float32), rtol=1e-6)
        np.testing.assert_array_equal(got["end"], np.where(np.array(length) < mx, 1, got["end"]))
    finally:
        env.close()


# ---------------------------------------------------------------- 6. Evaluator
def test_evaluator_is_the_waves_done_by_hand(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    from gmx.policy import DevicePolicy
    n, mx, objects = 8, 5, [3, 0, 7, 12, 5]

    def fresh():
        s = gm.canonical_settings(noise=True, seed=SEED)
        s.continous_actions = 0
        env = gm.BatchedGripperEnv(n, object_set="set6_synthetic", settings=s, seed=SEED)
        env.reset()
        return env, DevicePolicy(env, seed=3)

    a, pa = fresh()
    b, pb = fresh()
    try:
        ev = gm.Evaluator(a, test_objects=objects, trials_per_object=3, max_episode_steps=mx)
        data = ev.run(pa, seed=PSEED, decision0=DEC0)
        plan = gm.test_plan(5, 3, n)
        assert len(plan) == 2 and data.shape == (15,)
        for wave in plan:
            act = wave["active"]
            idx = np.array(objects)[np.where(act, wave["obj_idx"], 0)]
            b.reset(spawn=b.make_spawn(idx=idx))
            rep = host(pb.evaluate(seed=PSEED, decision0=DEC0, max_episode_steps=mx, active=act))
            rows = data[wave["trial"][act]]
            np.testing.assert_array_equal(rows["obj_idx"], wave["obj_idx"][act])
            np.testing.assert_array_equal(rows["obj_trial"], wave["obj_trial"][act])
            np.testing.assert_array_equal(rows["reward"], rep["ret"][act])
            np.testing.assert_array_equal(rows["length"], rep["length"][act])
            np.testing.assert_array_equal(rows["end"], rep["end"][act])
            for f in ("rows", "abs", "last"):
                np.testing.assert_array_equal(rows[f], rep[f][act], err_msg=f)
        np.testing.assert_array_equal(data["obj_idx"], np.arange(15) // 3)
        np.testing.assert_array_equal(data["obj_trial"], np.arange(15) % 3)
        np.testing.assert_array_equal(data["object_type"], [a.objects[objects[t // 3]].type for t in range(15)])
        assert (data["end"] > 0).all() and (data["length"] >= 1).all() and (data["length"] <= mx).all()
        perf = gm.test_performance(data)
        assert perf["trials"] == 15 and list(perf["per_object"]) == [0, 1, 2, 3, 4]
        # the env is left reset: a training rollout follows
        assert (gm.env_state_view(a.env_states())["num_action_steps"] == 0).all()
        pa.rollout(np.zeros(3, np.float32), seed=PSEED, decision0=0, max_episode_steps=mx)
        assert np.isfinite(a.observation()).all()
        assert a.chunk_stats()["finished"] == n
    finally:
        pa.close()
        pb.close()
        a.close()
        b.close()


# ---------------------------------------------------------------- 7. arguments
def test_bad_arguments_are_refused_without_a_launch(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.eval import report_struct
    from gmx.policy import DevicePolicy
    from gmx._lib import RolloutParams
    GM_E_ARG = -1
    drv = Driver(gm, "dqn", make_env(gm, n=8, discrete=True))
    cont = make_env(gm, n=8)
    try:
        env, lib, pol = drv.env, drv.env.lib, drv.agent
        rep = gm.new_report(env)
        o = report_struct(rep)
        torch.cuda.synchronize()
        env.lib.gm_step(env.ctx)
        before = env.env_states()

        def refused(rc, word):
            assert rc == GM_E_ARG, rc
            msg = lib.gm_last_error(env.ctx).decode()
            assert word in msg, msg

        p = RolloutParams()
        p.action_mode, p.max_episode_steps, p.seed, p.jitter = 3, 0, 1, 0.2
        refused(lib.gm_evaluate(env.ctx, C.byref(p), None, C.byref(o)), "max_episode_steps")
        refused(lib.gm_policy_evaluate(pol._p, 0, 0, 0, None, C.byref(o)), "max_episode_steps")
        refused(lib.gm_policy_evaluate(pol._p, 0, 0, -3, None, C.byref(o)), "max_episode_steps")
        refused(lib.gm_policy_evaluate(pol._p, 0, 0, MAX_EP, None, None), "report arrays")
        for f in FIELDS:
            missing = report_struct(dict(rep, **{f: None}))
            refused(lib.gm_policy_evaluate(pol._p, 0, 0, MAX_EP, None, C.byref(missing)), "missing")
        p.max_episode_steps = MAX_EP
        refused(lib.gm_evaluate(env.ctx, C.byref(p), None, None), "report arrays")
        p.action_mode = 2
        refused(lib.gm_evaluate(env.ctx, C.byref(p), None, C.byref(o)), "action_mode")
        act = torch.ones(8, dtype=torch.uint8, device="cuda")
        refused(lib.gm_eval_record(env.ctx, 0, C.c_void_p(act.data_ptr()), C.byref(o)), "max_episode_steps")
        refused(lib.gm_eval_record(env.ctx, MAX_EP, None, C.byref(o)), "active")
        with pytest.raises(RuntimeError, match="max_episode_steps"):
            pol.evaluate(max_episode_steps=0)
        # no launch: the env-step counter of the last launch and every state record are as they were
        assert env.dispatch_info()["last_launch_env_steps"] == 1
        np.testing.assert_array_equal(env.env_states(), before)
        # the project's rule for a policy of the other action kind: it cannot be created, and
        # without a handle there is nothing to evaluate
        with pytest.raises(RuntimeError, match="discrete actions"):
            DevicePolicy(cont, seed=3)
        assert lib.gm_policy_evaluate(None, 0, 0, MAX_EP, None, C.byref(o)) == GM_E_ARG
        assert lib.gm_ac_evaluate(None, 1, 0, 0, MAX_EP, None, C.byref(o)) == GM_E_ARG
        assert lib.gm_sac_evaluate(None, 0, 0, 0, MAX_EP, None, C.byref(o)) == GM_E_ARG
    finally:
        drv.close()
        cont.close()


def switch_action_kind(gm, env, continuous):
    """gm_update_config with the env's settings and the other action kind (as a facade's mj.set
    write does it on a live context).  Returns the config blob, which the caller keeps alive."""
    s = gm.canonical_settings(noise=True, seed=SEED)
    s.continous_actions = 1 if continuous else 0
    cfg = gm.ConfigBlob(s, env.model)
    assert cfg.n_obs == env.n_obs
    env._check(env.lib.gm_update_config(env.ctx, cfg.ptr))
    return cfg


def test_an_agent_refuses_an_env_switched_to_the_other_action_kind(gm):
    """An evaluation on a continuous-action env through gm_policy_evaluate, and its counterparts:
    the creators refuse a handle for the other action kind, so the case arises where
    gm_update_config changes continous_actions under a live handle.  Each agent call returns
    GM_E_ARG with a message and starts no launch."""
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.eval import report_struct
    from gmx.ppo import DeviceActorCritic, DeviceCategoricalActorCritic
    from gmx.sac import DeviceSAC
    GM_E_ARG = -1
    disc, cont = Driver(gm, "dqn", make_env(gm, n=8, discrete=True)), Driver(gm, "sac-mean", make_env(gm, n=8))
    cat = DeviceCategoricalActorCritic(disc.env, hidden=(64, 64), seed=3)
    ac = DeviceActorCritic(cont.env, hidden=(64, 64), seed=3)
    try:
        keep, before = [], {}
        for drv in (disc, cont):
            drv.env.lib.gm_step(drv.env.ctx)
            before[drv] = drv.env.env_states()
        keep.append(switch_action_kind(gm, disc.env, continuous=True))
        keep.append(switch_action_kind(gm, cont.env, continuous=False))
        lib = disc.env.lib
        calls = [(disc, lambda o: lib.gm_policy_evaluate(disc.agent._p, 0, 0, MAX_EP, None, o), "gm_policy_evaluate",
                  "discrete actions"),
                 (disc, lambda o: lib.gm_ac_evaluate(cat._p, 1, 0, 0, MAX_EP, None, o), "gm_ac_evaluate", "discrete actions"),
                 (cont, lambda o: lib.gm_ac_evaluate(ac._p, 1, 0, 0, MAX_EP, None, o), "gm_ac_evaluate", "continuous actions"),
                 (cont, lambda o: lib.gm_sac_evaluate(cont.agent._p, 0, 0, 0, MAX_EP, None, o), "gm_sac_evaluate",
                  "continuous actions")]
        for drv, call, who, word in calls:
            o = report_struct(gm.new_report(drv.env))
            torch.cuda.synchronize()
            assert call(C.byref(o)) == GM_E_ARG, who
            msg = lib.gm_last_error(drv.env.ctx).decode()
            assert who in msg and word in msg, msg
            assert drv.env.dispatch_info()["last_launch_env_steps"] == 1
            np.testing.assert_array_equal(drv.env.env_states(), before[drv])
        with pytest.raises(RuntimeError, match="discrete actions"):
            disc.agent.evaluate(max_episode_steps=MAX_EP)
    finally:
        cat.close()
        ac.close()
        disc.close()
        cont.close()
