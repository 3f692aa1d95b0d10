"""gm_ac_act on a categorical handle against a torch forward of the same f32 parameters and
observations, and the sampler against the float64 inverse CDF of the device's own logits.

The tolerance is tests/test_actor_critic_forward.py's: every expected value is computed on the CPU
in float32 and in float64, and the device must agree with the float64 one within
8 x max|f32 - f64| + one f32 ulp of the largest magnitude.  The draw has a kink wherever u s meets
a running sum of e_j = exp(x_j - max x): those sums and t = u s are evaluated from the device's
logits in f32 and f64, the same bound is formed on them, and an env whose t is within it of a
running sum is left out of the index comparison -- at most 1 % of the envs (asserted)."""
import ctypes as C

import numpy as np
import pytest

from conftest import gpu_available
from test_actor_critic_forward import bound, torch_forward

pytestmark = pytest.mark.gpu

N, SEED, PSEED, DEC = 300, 17, 23, 5000
NETS = {"20-20": dict(hidden=(20, 20)), "256-3": dict(hidden=(256, 3), hidden_v=(3, 256))}


def make_env(gm, n=N, continuous=False, termination=False):
    s = gm.canonical_settings(noise=True, seed=SEED)           # the canonical settings, discrete actions
    s.continous_actions = int(continuous)
    s.use_termination_action = int(termination)
    env = gm.BatchedGripperEnv(n, object_set="set6_synthetic", settings=s, seed=SEED)
    env.reset()
    if not continuous:
        rng = np.random.default_rng(0)
        for _ in range(3):                                      # observations that are not all alike
            env.step(rng.integers(0, env.n_actions, size=n), discrete=True)
    return env


def run_act(ac, traj, **kw):
    import torch
    ac.act(traj, 0, seed=PSEED, decision=DEC, **kw)
    torch.cuda.synchronize()
    return {k: getattr(traj, k)[0].cpu().numpy().copy() for k in ("obs", "act", "logp", "val", "mu")}


def running_sums(x, u, dtype):
    """(running sums of e_j = exp(x_j - max x) [n, A], t = u s [n]) in `dtype`, in index order."""
    x = x.astype(dtype)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    run = np.zeros_like(e)
    acc = np.zeros(len(x), dtype)
    for j in range(x.shape[1]):
        acc = acc + e[:, j]
        run[:, j] = acc
    return run, u.astype(dtype) * run[:, -1], e


@pytest.mark.parametrize("net", sorted(NETS))
def test_forward_and_draw(gm, net):
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.ppo import DeviceCategoricalActorCritic, TrajectoryBuffer, categorical_uniforms
    env = make_env(gm)
    ac = DeviceCategoricalActorCritic(env, seed=1, **NETS[net])
    try:
        assert (env.n_obs, env.n_actions) == (63, 8) and ac.params.size == sum(
            s[i + 1] * s[i] + s[i + 1] for s in (ac.actor_sizes, ac.critic_sizes) for i in range(len(s) - 1))
        obs = env.observation()
        assert len(np.unique(obs, axis=0)) > N // 2
        traj = TrajectoryBuffer(env, 1, act_dim=1)
        assert traj.act.shape == (1, N, 1) and traj.mu.shape == (1, N, 8)
        d = run_act(ac, traj, sample=True)
        np.testing.assert_array_equal(d["obs"], obs)
        a_dev = d["act"][:, 0]
        np.testing.assert_array_equal(a_dev, np.round(a_dev))
        assert a_dev.min() >= 0 and a_dev.max() < env.n_actions
        idx = torch.from_numpy(a_dev.astype(np.int64))

        class Nets:                         # torch_forward reads params (with a tail it ignores here)
            params, actor_sizes, critic_sizes = ac.params, ac.actor_sizes, ac.critic_sizes
        ref, ratios = {}, {}
        for dt in (torch.float32, torch.float64):
            logits, val, tail = torch_forward(Nets, obs, dt)
            assert tail.numel() == 0
            logp = torch.log_softmax(logits, dim=-1).gather(1, idx[:, None])[:, 0]
            ref[dt] = dict(mu=logits, val=val, logp=logp)
        for q in ("mu", "val", "logp"):
            b = bound(ref[torch.float32][q], ref[torch.float64][q])
            err = float(np.abs(d[q].astype(np.float64) - ref[torch.float64][q].numpy()).max())
            ratios[q] = err / b
            print(f"{net} {q}: max |device - f64| {err:.3e}, bound {b:.3e}, ratio {err / b:.3f}")
        assert max(ratios.values()) <= 1.0, f"worst |device - f64| / bound per quantity: {ratios}"

        # the chosen index: the float64 inverse CDF of the device's own logits at the mirror's u
        u = categorical_uniforms(PSEED, env.env_offset + np.arange(N), DEC)
        r32, t32, _ = running_sums(d["mu"], u, np.float32)
        r64, t64, e64 = running_sums(d["mu"], u, np.float64)
        b = bound(torch.from_numpy(np.concatenate([r32.ravel(), t32])), torch.from_numpy(np.concatenate([r64.ravel(), t64])))
        near = (np.abs(r64 - t64[:, None]) <= b).any(axis=1)
        hit = r64 > t64[:, None]
        want = np.where(hit.any(axis=1), hit.argmax(axis=1), 7 - (e64[:, ::-1] > 0).argmax(axis=1))
        share = float(near.mean())
        print(f"{net} draw: bound on the running sums {b:.3e}, envs left out {int(near.sum())} / {N} ({share:.2%})")
        assert share <= 0.01, f"{share:.2%} of the envs lie within the bound of a running sum"
        np.testing.assert_array_equal(a_dev[~near], want[~near])
        counts = np.bincount(a_dev.astype(np.int64), minlength=8)
        assert (counts > 0).sum() >= 6, counts                    # sampled, not the argmax
        # logp is the taken class's, from the device's own logits, to f32 rounding of x - lse
        x64 = d["mu"].astype(np.float64)
        lse = x64.max(axis=1) + np.log(np.exp(x64 - x64.max(axis=1, keepdims=True)).sum(axis=1))
        np.testing.assert_allclose(d["logp"], x64[np.arange(N), a_dev.astype(int)] - lse, rtol=0, atol=4e-6)

        # the same call again: the same bytes (counter-based draws)
        again = run_act(ac, traj, sample=True)
        for k in d:
            assert d[k].tobytes() == again[k].tobytes(), k

        # sample = 0: the argmax of the device's own logits, lowest index on a tie; and the float64
        # forward's argmax wherever its top two logits differ by more than the bound
        e = run_act(ac, traj, sample=False)
        np.testing.assert_array_equal(e["mu"], d["mu"])
        np.testing.assert_array_equal(e["val"], d["val"])
        np.testing.assert_array_equal(e["act"][:, 0], np.argmax(e["mu"], axis=1))
        l64 = ref[torch.float64]["mu"].numpy()
        top2 = np.sort(l64, axis=1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > bound(ref[torch.float32]["mu"], ref[torch.float64]["mu"])
        assert clear.mean() > 0.9
        np.testing.assert_array_equal(e["act"][clear, 0], np.argmax(l64, axis=1)[clear])
        assert (e["logp"] >= d["logp"]).all() and (e["logp"] < 0).all()    # the mode's log-probability
    finally:
        ac.close()
        env.close()


def test_act_applies_the_index_as_the_discrete_path(gm):
    """The env a categorical act drives ends in the state of a second env given the same indices
    through set_discrete_action, with the termination action in use (9 actions)."""
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.ppo import DeviceCategoricalActorCritic, TrajectoryBuffer
    n = 48
    a, b = make_env(gm, n, termination=True), make_env(gm, n, termination=True)
    ac = DeviceCategoricalActorCritic(a, hidden=(20, 20), seed=1)
    try:
        assert a.n_actions == 9
        np.testing.assert_array_equal(a.env_states(), b.env_states())
        traj = TrajectoryBuffer(a, 1, act_dim=1)
        ac.act(traj, 0, sample=True, seed=PSEED, decision=DEC)
        a.action_step()
        torch.cuda.synchronize()
        idx = traj.act[0, :, 0].cpu().numpy().astype(np.int32)
        assert len(np.unique(idx)) >= 5 and (idx == 8).any()      # the termination action among them
        b.set_discrete_action(idx)
        b.action_step()
        va, vb = gm.env_state_view(a.env_states()), gm.env_state_view(b.env_states())
        for name in va.dtype.names:
            np.testing.assert_array_equal(va[name], vb[name], err_msg=name)
        np.testing.assert_array_equal(a.observation(), b.observation())
    finally:
        ac.close()
        a.close()
        b.close()


def test_create_checks(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    from gmx.ppo import DeviceActorCritic, DeviceCategoricalActorCritic, TrajectoryBuffer
    env = make_env(gm, 4, continuous=True)
    try:
        with pytest.raises(RuntimeError, match="gm_ac_create_categorical: .*discrete actions"):
            DeviceCategoricalActorCritic(env, hidden=(16,))
        # the Gaussian actor and its learner refuse a buffer of the categorical width (they would read past it)
        from gmx.ppo import DevicePPOLearner
        gac = DeviceActorCritic(env, hidden=(16,))
        gl = DevicePPOLearner(gac)
        try:
            narrow = TrajectoryBuffer(env, 2, act_dim=1)
            for call in (lambda: gac.act(narrow, 0), lambda: gac.rollout(narrow), lambda: gl.update(narrow)):
                with pytest.raises(ValueError, match="act_dim"):
                    call()
        finally:
            gl.close()
            gac.close()
        a = np.asarray([env.n_obs, 16, env.n_actions], np.int32)
        c = np.asarray([env.n_obs, 16, 1], np.int32)
        prm = np.zeros(100000, np.float32)
        i32p = C.POINTER(C.c_int32)
        h = C.c_void_p()
        rc = env.lib.gm_ac_create_categorical(env.ctx, a.ctypes.data_as(i32p), 3, c.ctypes.data_as(i32p), 3,
                                              prm.ctypes.data_as(C.POINTER(C.c_float)), C.byref(h))
        assert rc == -1 and not h.value
        assert b"continous_actions" in env.lib.gm_last_error(env.ctx)
    finally:
        env.close()
    env = make_env(gm, 4)
    try:
        no, na = env.n_obs, env.n_actions
        with pytest.raises(RuntimeError, match="continuous actions"):       # the Gaussian actor still refuses
            DeviceActorCritic(env, actor_sizes=[no, 16, na], critic_sizes=[no, 16, 1])
        for asz, csz, word in (([no + 1, 16, na], [no, 16, 1], "actor"), ([no, 16, na + 1], [no, 16, 1], "actor"),
                               ([no, 16, na], [no, 16, 2], "critic"), ([no, 16, na], [no - 1, 16, 1], "critic")):
            with pytest.raises(RuntimeError, match="gm_ac_create_categorical: the " + word):
                DeviceCategoricalActorCritic(env, actor_sizes=asz, critic_sizes=csz)
        with pytest.raises(ValueError, match="parameters expected"):        # a Gaussian's count, with log_std
            DeviceCategoricalActorCritic(env, hidden=(16,), params=np.zeros((no + 1) * 16 + 17 * na + (no + 1) * 16 + 17 + na,
                                                                            np.float32))
        ac = DeviceCategoricalActorCritic(env, hidden=(16,))
        try:
            traj = TrajectoryBuffer(env, 2, act_dim=1)
            with pytest.raises(ValueError, match="noise"):
                ac.act(traj, 0, noise=0.1)
            with pytest.raises(ValueError, match="noise"):
                ac.rollout(traj, noise=0.1)
            with pytest.raises(ValueError, match="act_dim"):
                ac.act(TrajectoryBuffer(env, 2), 0)
            # the library's own check, under the Python one
            t = traj.struct()
            for rc in (env.lib.gm_ac_act(ac._p, C.byref(t), 0, 1, C.c_float(0.1), C.c_uint64(0), C.c_uint64(0)),
                       env.lib.gm_ac_rollout(ac._p, C.byref(t), 1, 1, C.c_float(0.1), C.c_uint64(0), C.c_uint64(0), 0,
                                             C.c_void_p(0))):
                assert rc == -1 and b"noise" in env.lib.gm_last_error(env.ctx)
            ac.act(traj, 0)                                                  # and noise 0 runs
        finally:
            ac.close()
    finally:
        env.close()
