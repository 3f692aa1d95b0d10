"""gm_ac_act on the GPU against a torch forward of the same f32 parameters and observations.

The tolerance is measured, not chosen: every expected value is computed on the CPU twice, in
float32 and in float64, and the device must agree with the float64 one within
8 x max|f32 - f64| of that quantity plus one f32 ulp of its largest magnitude (8 for the
different summation order -- the MFMA's k-ordered chain against torch's GEMM -- and few-ulp
tanhf / logf / cospif).  Measured worst |device - f64| / bound over both nets: see DESIGN.md."""
import math

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

N, SEED, PSEED, DEC = 300, 17, 23, 5000
NOISE = 0.05


def make_env(gm, n=N):
    env = gm.BatchedGripperEnv(n, object_set="set6_synthetic", settings=gm.canonical_settings(noise=True, seed=SEED),
                               seed=SEED)
    env.reset()
    env.rollout(3, action_mode=1, seed=5, max_episode_steps=0)     # observations that are not all alike
    return env


def torch_forward(ac, obs, dtype):
    """(mu, val, log_std) of the flat parameters with torch on the CPU in `dtype`."""
    import torch
    p = torch.from_numpy(ac.params).to(dtype)
    x0 = torch.from_numpy(obs).to(dtype)
    pos = 0
    outs = []
    for sizes in (ac.actor_sizes, ac.critic_sizes):
        x = x0
        for l in range(len(sizes) - 1):
            fin, fout = sizes[l], sizes[l + 1]
            W = p[pos:pos + fout * fin].reshape(fout, fin)
            pos += fout * fin
            b = p[pos:pos + fout]
            pos += fout
            x = torch.nn.functional.linear(x, W, b)
            if l < len(sizes) - 2:
                x = torch.tanh(x)
        outs.append(x)
    return outs[0], outs[1][:, 0], p[pos:]


def logp_of(a, mu, log_std):
    import torch
    std = torch.exp(log_std)
    return (-((a - mu) ** 2) / (2 * std ** 2) - log_std - 0.5 * math.log(2 * math.pi)).sum(-1)


def bound(x32, x64):
    """8 x max|f32 - f64| + one f32 ulp of the largest magnitude."""
    x64 = x64.numpy()
    return 8.0 * float(np.abs(x32.numpy().astype(np.float64) - x64).max()) + \
        float(np.spacing(np.float32(np.abs(x64).max())))


def run_act(gm, ac, traj, **kw):
    import torch
    ac.act(traj, 0, seed=PSEED, decision=DEC, **kw)
    torch.cuda.synchronize()
    return {k: getattr(traj, k)[0].cpu().numpy().copy() for k in ("obs", "act", "logp", "val", "mu")}


@pytest.mark.parametrize("hidden", [(64, 64), (20, 20)])
def test_forward_matches_torch(gm, hidden):
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.ppo import DeviceActorCritic, TrajectoryBuffer, normal_draws, noise_draws
    env = make_env(gm)
    ac = DeviceActorCritic(env, hidden=hidden, seed=1)
    try:
        obs = env.observation()
        assert len(np.unique(obs, axis=0)) > N // 2
        traj = TrajectoryBuffer(env, 1)
        d = run_act(gm, ac, traj, sample=True, noise=0.0)
        np.testing.assert_array_equal(d["obs"], obs)
        gids = env.env_offset + np.arange(N)
        z = normal_draws(PSEED, gids, DEC, env.n_actions)
        ref, ratios = {}, {}
        for dt in (torch.float32, torch.float64):
            mu, val, ls = torch_forward(ac, obs, dt)
            a_dev = torch.from_numpy(d["act"]).to(dt)
            ref[dt] = dict(mu=mu, val=val, logp=logp_of(a_dev, mu, ls),
                           act=mu + torch.exp(ls) * torch.from_numpy(z).to(dt))
        for q in ("mu", "val", "logp", "act"):
            b = bound(ref[torch.float32][q], ref[torch.float64][q])
            err = float(np.abs(d[q].astype(np.float64) - ref[torch.float64][q].numpy()).max())
            ratios[q] = err / b
            print(f"hidden {hidden} {q}: max |device - f64| {err:.3e}, bound {b:.3e}, ratio {err / b:.3f}")
        assert max(ratios.values()) <= 1.0, f"worst |device - f64| / bound per quantity: {ratios}"
        assert np.abs(d["act"] - d["mu"]).max() > 0.1                 # sampled

        # sample = 0: the mean action, bit for bit, and its log-probability
        e = run_act(gm, ac, traj, sample=False, noise=0.0)
        np.testing.assert_array_equal(e["act"], e["mu"])
        np.testing.assert_array_equal(e["mu"], d["mu"])
        np.testing.assert_array_equal(e["val"], d["val"])
        ls32 = ac.params[-env.n_actions:].astype(np.float64)
        np.testing.assert_allclose(e["logp"], np.full(N, (-ls32 - 0.5 * math.log(2 * math.pi)).sum()), rtol=1e-6)

        # exploration noise: added after logp, uniform in [-NOISE, NOISE), the mirror's draws
        f = run_act(gm, ac, traj, sample=True, noise=NOISE)
        np.testing.assert_array_equal(f["logp"], d["logp"])
        np.testing.assert_array_equal(f["mu"], d["mu"])
        tol = bound(ref[torch.float32]["act"], ref[torch.float64]["act"])
        dn = f["act"].astype(np.float64) - ref[torch.float64]["act"].numpy()
        assert dn.min() >= -NOISE - tol and dn.max() < NOISE + tol, (dn.min(), dn.max())
        u = noise_draws(PSEED, gids, DEC, env.n_actions, NOISE)
        assert np.abs(dn - u).max() <= tol, (np.abs(dn - u).max(), tol)
        assert np.abs(f["act"] - d["act"]).max() > NOISE / 2
    finally:
        ac.close()
        env.close()


def test_buffer_keeps_unclipped_actions(gm):
    """log_std = +1: some |a| > 1 reach the buffer unclipped, and the env they drive ends in
    the state of a second env given set_action(clip(a))."""
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.ppo import DeviceActorCritic, TrajectoryBuffer, init_params
    n = 48
    a, b = make_env(gm, n), make_env(gm, n)
    sizes = ([a.n_obs, 64, 64, a.n_actions], [a.n_obs, 64, 64, 1])
    prm = init_params(*sizes, seed=1)
    prm[-a.n_actions:] = 1.0
    ac = DeviceActorCritic(a, params=prm)
    try:
        np.testing.assert_array_equal(a.env_states(), b.env_states())
        traj = TrajectoryBuffer(a, 1)
        ac.act(traj, 0, sample=True, noise=NOISE, seed=PSEED, decision=DEC)
        a.action_step()
        torch.cuda.synchronize()
        act = traj.act[0].cpu().numpy()
        assert (np.abs(act) > 1.0).sum() > n // 4, "no action left [-1, 1]: the test shows nothing"
        b.set_action(np.clip(act, -1.0, 1.0))
        b.action_step()
        sa, sb = a.env_states(), b.env_states()
        va, vb = gm.env_state_view(sa), gm.env_state_view(sb)
        for name in va.dtype.names:
            np.testing.assert_array_equal(va[name], vb[name], err_msg=name)
        np.testing.assert_array_equal(a.observation(), b.observation())
    finally:
        ac.close()
        a.close()
        b.close()
