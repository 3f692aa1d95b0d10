"""gm_ac_gae (GAE-lambda advantages and rewards-to-go, PPOBuffer.finish_trajectory per env and
trajectory segment) on synthetic buffers against a float64 evaluation of the recurrences
written here, and TrajectoryBuffer.get's advantage normalisation."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

N, K = 70, 12


def reference(rew, val, end, boot, last_val, gamma, lam):
    rew, val, boot, last_val = (x.astype(np.float64) for x in (rew, val, boot, last_val))
    adv, ret = np.zeros((K + 1, N)), np.zeros((K + 1, N))
    for k in range(K - 1, -1, -1):
        for e in range(N):
            c = end[k, e]
            nxt_v = 0.0 if c == 1 else boot[k, e] if c == 2 else (last_val[e] if k == K - 1 else val[k + 1, e])
            delta = rew[k, e] + gamma * nxt_v - val[k, e]
            adv[k, e] = delta + (0.0 if c else gamma * lam * adv[k + 1, e])
            nxt_r = 0.0 if c == 1 else boot[k, e] if c == 2 else (last_val[e] if k == K - 1 else ret[k + 1, e])
            ret[k, e] = rew[k, e] + gamma * nxt_r
    return adv[:K], ret[:K]


def synthetic():
    rng = np.random.default_rng(11)
    rew = rng.uniform(-1, 1, (K, N)).astype(np.float32)
    val = rng.uniform(-2, 2, (K, N)).astype(np.float32)
    last_val = rng.uniform(-2, 2, N).astype(np.float32)
    end = np.zeros((K, N), np.uint8)
    # env 0: no end at all; then one env per branch; the rest random
    end[0, 1] = 1                      # terminal at k = 0
    end[K - 1, 2] = 1                  # terminal at K - 1
    end[K - 1, 3] = 2                  # truncated at K - 1
    end[K // 2, 4] = 2                 # truncated mid-way
    end[5, 5], end[6, 5] = 1, 2        # two ends in a row
    end[7, 6], end[8, 6] = 2, 1
    end[0, 7] = 2                      # truncated at k = 0
    end[:, 8:] = rng.choice([0, 0, 0, 1, 2], size=(K, N - 8)).astype(np.uint8)
    # boot: the bootstrap value where truncated; elsewhere gm_ac_record writes 0 -- a value
    # there must not be read, so some of those hold garbage
    boot = np.where(end == 2, rng.uniform(-2, 2, (K, N)), 0.0).astype(np.float32)
    boot[:, ::2] = np.where(end[:, ::2] == 2, boot[:, ::2], 9.0)
    return rew, val, end, boot, last_val


@pytest.fixture(scope="module")
def ctx(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    from gmx.ppo import TrajectoryBuffer
    env = gm.BatchedGripperEnv(N, object_set="set1_synthetic", settings=gm.canonical_settings(noise=False, seed=2), seed=2)
    traj = TrajectoryBuffer(env, K)
    data = synthetic()
    for name, x in zip(("rew", "val", "end", "boot", "last_val"), data):
        getattr(traj, name).copy_(torch.from_numpy(x))
    torch.cuda.synchronize()
    yield env, traj, data
    env.close()


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.97), (1.0, 1.0)])
def test_gae_matches_float64(ctx, gamma, lam):
    env, traj, (rew, val, end, boot, last_val) = ctx
    assert (end[:, 0] == 0).all() and end[0, 1] == 1 and end[K - 1, 2] == 1 and end[K - 1, 3] == 2
    adv, ret = traj.gae(gamma, lam)
    adv, ret = adv.cpu().numpy(), ret.cpu().numpy()
    want_adv, want_ret = reference(rew, val, end, boot, last_val, gamma, lam)
    big = max(np.abs(rew).max(), np.abs(val).max(), np.abs(boot[end == 2]).max())
    # 12 steps x 3 roundings x 6e-8 with margin, over the geometric sum of the recurrence
    # (K in its place when gamma lam = 1)
    atol = 1e-5 * big * (K if gamma * lam == 1.0 else 1.0 / (1.0 - gamma * lam))
    ea, er = np.abs(adv - want_adv).max(), np.abs(ret - want_ret).max()
    print(f"gamma {gamma} lam {lam}: max |adv - f64| {ea:.3e}, |ret - f64| {er:.3e}, atol {atol:.3e}")
    np.testing.assert_allclose(adv, want_adv, rtol=0, atol=atol)
    np.testing.assert_allclose(ret, want_ret, rtol=0, atol=atol)
    # a shorter scan reads only its own rows: row n_steps - 1 continues into last_val
    adv5, ret5 = traj.gae(gamma, lam, n_steps=5)
    cont = end[4] == 0
    np.testing.assert_allclose(ret5.cpu().numpy()[4][cont], (rew[4] + np.float32(gamma) * last_val)[cont], rtol=0, atol=atol)


def test_get_normalises_advantages(ctx):
    import torch
    env, traj, data = ctx
    out = traj.get(0.99, 0.97)
    assert out["obs"].shape == (K * N, env.n_obs) and out["act"].shape == (K * N, env.n_actions)
    for k in ("ret", "adv", "logp"):
        assert out[k].shape == (K * N,)
    adv = out["adv"].double().cpu()
    assert abs(float(adv.mean())) < 1e-5
    assert abs(float(adv.std(unbiased=True)) - 1.0) < 1e-5
    raw, ret = traj.gae(0.99, 0.97)
    np.testing.assert_array_equal(out["ret"].cpu().numpy(), ret.reshape(-1).cpu().numpy())
    std, mean = torch.std_mean(raw)
    np.testing.assert_array_equal(out["adv"].cpu().numpy(), ((raw - mean) / std).reshape(-1).cpu().numpy())
