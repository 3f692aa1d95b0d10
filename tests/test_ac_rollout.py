"""gm_ac_rollout: the PPO actor-critic's rollout fused into one persistent launch (each env's own
wave runs actor and critic between its env-steps and fills the trajectory buffer) must equal,
bit for bit, the per-step sequence gm_ac_act (the batched MFMA kernels) -> gm_step ->
gm_ac_record -> gm_autoreset_episodes, then gm_ac_finish (include/gripper_mi355x.h).  Checked
on the whole fp64 state record, observations, rewards, done flags, every episode-end record
and every array of the trajectory buffer, with episodes short enough to be truncated and reset
inside the launch, and under the hand-off heavy dispatch (envs change waves and XCDs mid
env-step).  Also: sharding leaves the buffers unchanged, and the loop closes -- a torch Adam
step on the collected batch, handed back with set_params, changes the device's mu to the
updated torch nets'."""
import hashlib
import os

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

N, K, MAX_EP, SEED, PSEED, DEC0 = 96, 12, 5, 41, 9, 1000
NOISE = 0.05
FIELDS = ("obs", "act", "logp", "val", "rew", "end", "boot", "last_val", "mu")

HANDOFF = {"GM_CHUNK_SUBSTEPS": "1", "GM_CHUNK_MARGIN": "0", "GM_CHUNK_YIELDS": "60", "GM_CHUNK_CMARGIN": "0",
           "GM_CHUNK_GRID": "24"}


def make_env(gm, env_vars=None, n=N, env_offset=0):
    import bench
    s = gm.canonical_settings(noise=True, seed=SEED)           # the canonical continuous actions
    old = {k: os.environ.get(k) for k in (env_vars or {})}
    os.environ.update(env_vars or {})
    try:
        env = gm.BatchedGripperEnv(n, object_set="set6_synthetic", settings=s, seed=SEED, env_offset=env_offset)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    env.set_scene_spawn(bench.mjenv_spawn_params(gm), max_tries=3)
    env.reset()
    return env


def per_step(env, ac, traj, records, k0, k1, max_ep=MAX_EP, post=None, after=None):
    """Rows k0 .. k1 - 1 through the per-step API (no gm_ac_finish).  post / after: lists that
    receive each env-step's observation before / after the auto-reset."""
    import torch
    for k in range(k0, k1):
        ac.act(traj, k, sample=True, noise=NOISE, seed=PSEED, decision=DEC0 + k)
        env.lib.gm_step(env.ctx)
        if post is not None:
            post.append(env.observation())                     # the post-step observation
        ac.record(traj, k, max_episode_steps=max_ep)
        env.autoreset_device(0, None, max_episode_steps=max_ep, episodes_dev_ptr=records[k].data_ptr())
        if after is not None:
            after.append(env.observation())                    # the reset observation where the env was reset
    torch.cuda.synchronize()


def snapshot(env, traj, records):
    import torch
    torch.cuda.synchronize()
    st = env.env_states()
    rew, done = env.reward_done()
    out = dict(hash=hashlib.sha1(np.ascontiguousarray(st).tobytes()).hexdigest(), state=st, observation=env.observation(),
               reward=rew, done=done, records=records.cpu().numpy())
    for f in FIELDS:
        out[f] = getattr(traj, f).cpu().numpy()
    return out


def assert_same(gm, sa, sb):
    va, vb = gm.env_state_view(sa["state"]), gm.env_state_view(sb["state"])
    for f in va.dtype.names:
        np.testing.assert_array_equal(va[f], vb[f], err_msg=f)
    assert sa["hash"] == sb["hash"]
    for f in ("observation", "reward", "done", "records") + FIELDS:
        np.testing.assert_array_equal(sa[f], sb[f], err_msg=f)


@pytest.mark.parametrize("dispatch", ["default", "handoff-heavy", "one-shot"])
def test_ac_rollout_equals_per_step(gm, dispatch):
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.ppo import DeviceActorCritic, TrajectoryBuffer
    from gmx.shard import unpack_episodes
    ra = torch.zeros((K, N, 3), dtype=torch.int32, device="cuda")
    rb = torch.zeros((K, N, 3), dtype=torch.int32, device="cuda")
    a = make_env(gm)
    b = make_env(gm, {"handoff-heavy": HANDOFF, "one-shot": {"GM_CHUNK_SUBSTEPS": "0"}}.get(dispatch))
    pa, pb = DeviceActorCritic(a, seed=3), DeviceActorCritic(b, seed=3)
    ta, tb = TrajectoryBuffer(a, K), TrajectoryBuffer(b, K)
    try:
        post, after = [], []
        reset_obs0 = a.observation()
        per_step(a, pa, ta, ra, 0, K, post=post, after=after)
        pa.finish(ta)
        # the hand-off dispatch needs the dispatch costs a context records from its first
        # env-step on: b takes that one through the per-step API too
        k0 = 1 if dispatch == "handoff-heavy" else 0
        per_step(b, pb, tb, rb, 0, k0)
        pb.rollout(tb, sample=True, noise=NOISE, seed=PSEED, decision0=DEC0 + k0, max_episode_steps=MAX_EP,
                   records_dev_ptr=rb[k0:].data_ptr(), k0=k0)
        sa, sb = snapshot(a, ta, ra), snapshot(b, tb, rb)
        assert_same(gm, sa, sb)
        # -- what keeps the identity from holding vacuously (on the per-step side's data)
        end, boot, obs = sa["end"], sa["boot"], sa["obs"]
        _, length, _ = unpack_episodes(torch.from_numpy(sa["records"].reshape(-1, 3)))
        assert int((length > 0).sum()) >= N, int((length > 0).sum())
        n_term, n_trunc = int((end == 1).sum()), int((end == 2).sum())
        assert n_trunc > 0 and set(np.unique(end)) <= {0, 1, 2}, \
            f"end == 2 occurs {n_trunc} times, end == 1 {n_term} times (terminal ends are not required here)"
        assert ((boot != 0) == (end == 2)).all()
        np.testing.assert_array_equal((sa["records"][..., 1] > 0), end != 0)     # record length > 0 <=> an end
        np.testing.assert_array_equal(obs[0], reset_obs0)
        for k in range(K - 1):
            cont = end[k] == 0
            np.testing.assert_array_equal(obs[k + 1][cont], post[k][cont])       # the post-step observation
            np.testing.assert_array_equal(obs[k + 1][~cont], after[k][~cont])    # the reset observation
            np.testing.assert_array_equal(after[k][cont], post[k][cont])         # (no reset where none was due)
            # and a reset observation is not the post-step one, env by env
            assert (obs[k + 1][~cont] != post[k][~cont]).any(axis=1).all()
        assert len(np.unique(sa["act"])) > N
        assert np.abs(sa["act"] - sa["mu"]).max() > 0.1 and np.isfinite(sa["logp"]).all()
        assert (sa["last_val"] != 0).all() and (sa["val"] != 0).all()
        assert int(gm.env_state_view(sa["state"])["episode"].min()) >= 2
        if dispatch == "handoff-heavy":
            st = b.chunk_stats()
            assert st["yields"] > N and st["steals"] > 0, st
        assert (b.dispatch_info()["chunk"] == 0) == (dispatch == "one-shot")
        assert (sa["end"] == sb["end"]).all(), f"{dispatch}: end == 1 occurs {n_term} times, end == 2 {n_trunc} times"
    finally:
        pa.close()
        pb.close()
        a.close()
        b.close()


def test_ac_rollout_equals_per_step_widest_and_narrowest_layers(gm):
    """The same identity where the shared forward's indexing is at its limits: actor hidden
    (256, 3) and critic hidden (3, 256) put width 256 (GP_MAX_WIDTH: 16 output tiles, then 64
    k-steps up to the row stride) and width 3 (one partial tile, then k padded to 4) in both
    positions.  33 envs: two full 16-env tiles and a one-env tail in the batched kernel;
    2-step episodes, so truncation, the bootstrap value and the in-launch reset occur."""
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.ppo import DeviceActorCritic, TrajectoryBuffer
    n, k, mx = 33, 3, 2
    ra = torch.zeros((k, n, 3), dtype=torch.int32, device="cuda")
    rb = torch.zeros((k, n, 3), dtype=torch.int32, device="cuda")
    a, b = make_env(gm, n=n), make_env(gm, n=n)
    pa, pb = (DeviceActorCritic(e, hidden=(256, 3), hidden_v=(3, 256), seed=3) for e in (a, b))
    ta, tb = TrajectoryBuffer(a, k), TrajectoryBuffer(b, k)
    try:
        per_step(a, pa, ta, ra, 0, k, max_ep=mx)
        pa.finish(ta)
        pb.rollout(tb, sample=True, noise=NOISE, seed=PSEED, decision0=DEC0, max_episode_steps=mx,
                   records_dev_ptr=rb.data_ptr())
        sa, sb = snapshot(a, ta, ra), snapshot(b, tb, rb)
        assert_same(gm, sa, sb)
        assert b.dispatch_info()["chunk"] > 0                                   # the fused launch, not its fallback
        assert (sa["end"] == 2).any() and ((sa["boot"] != 0) == (sa["end"] == 2)).all()
        assert len(np.unique(sa["mu"])) > n and (sa["val"] != 0).all() and (sa["last_val"] != 0).all()
    finally:
        pa.close()
        pb.close()
        a.close()
        b.close()


def test_ac_rollout_equals_per_step_full_size(gm):
    """The same identity at the headline batch (4096 envs, every XCD's queue busy), with
    3-step episodes so every env is truncated and reset inside the launch."""
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.ppo import DeviceActorCritic, TrajectoryBuffer
    n, k, mx = 4096, 4, 3
    ra = torch.zeros((k, n, 3), dtype=torch.int32, device="cuda")
    rb = torch.zeros((k, n, 3), dtype=torch.int32, device="cuda")
    a, b = make_env(gm, n=n), make_env(gm, n=n)
    pa, pb = DeviceActorCritic(a, seed=5), DeviceActorCritic(b, seed=5)
    ta, tb = TrajectoryBuffer(a, k), TrajectoryBuffer(b, k)
    try:
        per_step(a, pa, ta, ra, 0, k, max_ep=mx)
        pa.finish(ta)
        per_step(b, pb, tb, rb, 0, 1, max_ep=mx)         # (b's dispatch costs from one env-step)
        pb.rollout(tb, sample=True, noise=NOISE, seed=PSEED, decision0=DEC0 + 1, max_episode_steps=mx,
                   records_dev_ptr=rb[1:].data_ptr(), k0=1)
        sa, sb = snapshot(a, ta, ra), snapshot(b, tb, rb)
        assert sa["hash"] == sb["hash"]
        for f in ("observation", "reward", "done", "records") + FIELDS:
            assert hashlib.sha1(sa[f].tobytes()).hexdigest() == hashlib.sha1(sb[f].tobytes()).hexdigest(), f
        assert int((sa["records"][..., 1] > 0).sum()) >= n      # every env's episode ended inside
        assert (sa["end"][2] != 0).all() and ((sa["boot"] != 0) == (sa["end"] == 2)).all()
    finally:
        pa.close()
        pb.close()
        a.close()
        b.close()


def test_ac_rollout_is_shard_independent(gm):
    """Two 48-env contexts at env_offset 0 and 48 collect what one 96-env context collects:
    the draws (actions, spawns) are keyed by the global env id."""
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.ppo import DeviceActorCritic, TrajectoryBuffer
    k = 7
    whole = make_env(gm)
    halves = [make_env(gm, n=N // 2, env_offset=0), make_env(gm, n=N // 2, env_offset=N // 2)]
    acs, out = [], []
    try:
        for env in [whole] + halves:
            ac = DeviceActorCritic(env, seed=3)
            acs.append(ac)
            t = TrajectoryBuffer(env, k)
            ac.rollout(t, sample=True, noise=NOISE, seed=PSEED, decision0=DEC0, max_episode_steps=MAX_EP)
            torch.cuda.synchronize()
            out.append({f: getattr(t, f).cpu().numpy() for f in FIELDS})
        for f in FIELDS:
            ax = 0 if f == "last_val" else 1
            np.testing.assert_array_equal(out[0][f], np.concatenate([out[1][f], out[2][f]], axis=ax), err_msg=f)
        assert (out[0]["end"] == 2).any()
        assert not np.array_equal(out[1]["act"], out[2]["act"])
    finally:
        for ac in acs:
            ac.close()
        whole.close()
        for e in halves:
            e.close()


def test_loop_closes(gm):
    """One rollout -> TrajectoryBuffer.get -> one Adam step of the clipped PPO loss on torch
    copies of the two nets -> set_params: a second act's mu on the same observations equals the
    updated torch nets' within the measured forward tolerance (tests/test_actor_critic_forward.py)
    and differs from the first."""
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from torch import nn
    from gmx.ppo import DeviceActorCritic, TrajectoryBuffer, params_from_state_dict
    env = make_env(gm)
    ac = DeviceActorCritic(env, seed=3)
    try:
        traj = TrajectoryBuffer(env, K)
        ac.rollout(traj, sample=True, noise=0.0, seed=PSEED, decision0=DEC0, max_episode_steps=MAX_EP)
        batch = {k: v.detach().cpu() for k, v in traj.get(0.99, 0.97).items()}
        assert batch["obs"].shape == (K * N, env.n_obs) and batch["adv"].shape == (K * N,)

        def mlp(sizes):
            layers = []
            for i in range(len(sizes) - 1):
                layers += [nn.Linear(sizes[i], sizes[i + 1]), nn.Tanh() if i < len(sizes) - 2 else nn.Identity()]
            return nn.Sequential(*layers)
        mu_net, v_net = mlp(ac.actor_sizes), mlp(ac.critic_sizes)
        log_std = nn.Parameter(torch.zeros(env.n_actions))
        flat = torch.from_numpy(ac.params)
        pos = 0
        with torch.no_grad():
            for prm in list(mu_net.parameters()) + list(v_net.parameters()) + [log_std]:
                prm.copy_(flat[pos:pos + prm.numel()].reshape(prm.shape))
                pos += prm.numel()
        assert pos == flat.numel()

        def logp(obs, act):
            return torch.distributions.Normal(mu_net(obs), torch.exp(log_std)).log_prob(act).sum(-1)
        # (Adam's first step moves every parameter by about lr, the actor's output bias included,
        # so mu moves by more than the 1e-3 asked below)
        opt = torch.optim.Adam(list(mu_net.parameters()) + list(v_net.parameters()) + [log_std], lr=3e-3)
        ratio = torch.exp(logp(batch["obs"], batch["act"]) - batch["logp"])
        loss_pi = -torch.min(ratio * batch["adv"], torch.clamp(ratio, 0.8, 1.2) * batch["adv"]).mean()
        loss_v = ((v_net(batch["obs"])[:, 0] - batch["ret"]) ** 2).mean()
        opt.zero_grad()
        (loss_pi + loss_v).backward()
        opt.step()

        sd = {"pi.log_std": log_std.detach()}
        sd.update({"pi.mu_net." + k: v for k, v in mu_net.state_dict().items()})
        sd.update({"vf.v_net." + k: v for k, v in v_net.state_dict().items()})
        obs = env.observation()
        one = TrajectoryBuffer(env, 1)
        ac.act(one, 0, sample=False)
        torch.cuda.synchronize()
        mu_before = one.mu[0].cpu().numpy().copy()
        ac.set_params(sd)
        np.testing.assert_array_equal(ac.params, params_from_state_dict(sd)[2])
        ac.act(one, 0, sample=False)
        torch.cuda.synchronize()
        mu_after, val_after = one.mu[0].cpu().numpy(), one.val[0].cpu().numpy()
        x = torch.from_numpy(obs)
        with torch.no_grad():
            m32, v32 = mu_net(x), v_net(x)[:, 0]
            m64, v64 = mu_net.double()(x.double()), v_net.double()(x.double())[:, 0]
        for dev, r32, r64, name in ((mu_after, m32, m64, "mu"), (val_after, v32, v64, "val")):
            r64 = r64.numpy()
            b = 8.0 * float(np.abs(r32.numpy().astype(np.float64) - r64).max()) + \
                float(np.spacing(np.float32(np.abs(r64).max())))
            err = float(np.abs(dev.astype(np.float64) - r64).max())
            assert err <= b, f"{name}: |device - f64| {err:.3e} > bound {b:.3e}"
        assert np.abs(mu_after - mu_before).max() > 1e-3
    finally:
        ac.close()
        env.close()
