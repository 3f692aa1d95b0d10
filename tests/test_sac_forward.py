"""gm_sac_act on the GPU against a torch evaluation of the same f32 parameters and observations.

The tolerance is tests/test_actor_critic_forward.py's measured rule, not a chosen constant: every
expected value is computed on the CPU twice, in float32 and in float64, and the device must agree
with the float64 one within 8 x max|f32 - f64| of that quantity plus one f32 ulp of its largest
magnitude.  u is checked against mu + std z with the mirror's z, act against limit tanh(u) of the
DEVICE's u, and logp from the device's u too (inverting tanh is ill-conditioned).  33 envs: two
full 16-env tiles and a one-env tail.  Measured worst |device - f64| / bound: see DESIGN.md."""
import numpy as np
import pytest

from conftest import gpu_available
from sac_model import module_from_flat, in_dtype, actor_head, logp_of, check

pytestmark = pytest.mark.gpu

N, SEED, PSEED, DEC = 33, 17, 23, 5000


def make_env(gm, n=N):
    env = gm.BatchedGripperEnv(n, object_set="set6_synthetic", settings=gm.canonical_settings(noise=True, seed=SEED),
                               seed=SEED)
    env.reset()
    env.rollout(3, action_mode=1, seed=5, max_episode_steps=0)     # observations that are not all alike
    return env


def reference(gm, env, sac, obs, dev, limit):
    """{dtype: dict of expected mu, log_std, u, act, logp} for the device's read-back `dev`."""
    import torch
    from gmx.sac import normal_draws
    z = normal_draws(PSEED, env.env_offset + np.arange(env.n_envs), DEC, env.n_actions)
    mod = module_from_flat(env.n_obs, env.n_actions, sac.pi_sizes[1:-1], sac.activation, sac.params)
    ref = {}
    for dt in (torch.float32, torch.float64):
        mu, ls = actor_head(in_dtype(mod, dt), torch.from_numpy(obs).to(dt))
        u_dev = torch.from_numpy(dev["u"]).to(dt)
        ref[dt] = dict(mu=mu, log_std=ls, u=mu + torch.exp(ls) * torch.from_numpy(z).to(dt),
                       act=limit * torch.tanh(u_dev), logp=logp_of(u_dev, mu, ls))
    return ref


def assert_within(dev, ref, names, label):
    import torch
    ratios = {}
    for q in names:
        check(q, dev[q], ref[torch.float32][q], ref[torch.float64][q], ratios, label)
    assert max(ratios.values()) <= 1.0, f"{label}: worst |device - f64| / bound per quantity: {ratios}"


@pytest.mark.parametrize("hidden,activation,limit", [((256, 256), "relu", 1.0), ((20, 20), "tanh", 0.5),
                                                     ((256, 3), "relu", 1.0), ((3, 256), "relu", 1.0)])
def test_act_matches_torch(gm, hidden, activation, limit):
    if not gpu_available():
        pytest.skip("no GPU")
    from gmx.sac import DeviceSAC, uniform_action_draws, init_params
    env = make_env(gm)
    sac = DeviceSAC(env, hidden=hidden, seed=1, activation=activation, action_limit=limit)
    try:
        obs = env.observation()
        assert len(np.unique(obs, axis=0)) > N // 2
        sac.act("sample", seed=PSEED, decision=DEC)
        d = sac.read()
        ref = reference(gm, env, sac, obs, d, limit)
        assert_within(d, ref, ("mu", "log_std", "u", "act", "logp"), f"hidden {hidden} {activation}")
        assert np.abs(d["u"] - d["mu"]).max() > 0.1 and np.isfinite(d["logp"]).all()         # sampled
        assert np.abs(d["act"]).max() <= limit and len(np.unique(d["act"])) > N

        # GM_SAC_MEAN: u == mu bit for bit, the same head
        e = sac.act("mean", seed=PSEED, decision=DEC) or sac.read()
        np.testing.assert_array_equal(e["u"], e["mu"])
        np.testing.assert_array_equal(e["mu"], d["mu"])
        np.testing.assert_array_equal(e["log_std"], d["log_std"])

        # GM_SAC_RANDOM: the mirror's uniform actions bit for bit, whatever the weights
        gids = env.env_offset + np.arange(N)
        want = uniform_action_draws(PSEED, gids, DEC, env.n_actions).astype(np.float32)
        r1 = sac.act("random", seed=PSEED, decision=DEC) or sac.read()
        np.testing.assert_array_equal(r1["act"], want)
        assert not r1["u"].any() and not r1["logp"].any()
        sac.set_params(init_params(sac.pi_sizes, sac.q_sizes, seed=99))
        r2 = sac.act("random", seed=PSEED, decision=DEC) or sac.read()
        np.testing.assert_array_equal(r2["act"], want)
        m2 = sac.act("mean", seed=PSEED, decision=DEC) or sac.read()
        assert np.abs(m2["mu"] - d["mu"]).max() > 1e-3            # (the other weights are really there)
    finally:
        sac.close()
        env.close()


def crafted(gm, env, edit, hidden=(20, 20)):
    """A DeviceSAC whose state dict `edit` changed, and its read-back after one sampled act."""
    from gmx.sac import DeviceSAC, flat_to_state_dict, init_params, sizes
    psz, qsz = sizes(env.n_obs, env.n_actions, hidden)
    sd = flat_to_state_dict(psz, qsz, init_params(psz, qsz, seed=2))
    edit(sd)
    sac = DeviceSAC(env, hidden=hidden)
    sac.set_params(sd)
    sac.act("sample", seed=PSEED, decision=DEC)
    return sac, sac.read()


def test_log_std_clamps_engage(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    env = make_env(gm)

    def edit(sd):
        sd["pi.log_std_layer.weight"][:2] *= 0.25      # (the biases decide, whatever the hidden row)
        sd["pi.log_std_layer.bias"][0] = 5.0
        sd["pi.log_std_layer.bias"][1] = -30.0
    sac, d = crafted(gm, env, edit)
    try:
        np.testing.assert_array_equal(d["log_std"][:, 0], np.full(N, 2.0, np.float32))
        np.testing.assert_array_equal(d["log_std"][:, 1], np.full(N, -20.0, np.float32))
        assert (np.abs(d["log_std"][:, 2:]) < 2.0).all()          # the others are not clamped
        assert np.isfinite(d["logp"]).all() and np.isfinite(d["u"]).all()
        ref = reference(gm, env, sac, env.observation(), d, 1.0)
        assert_within(d, ref, ("mu", "log_std", "u", "act"), "clamped log_std")
        # std = exp(2) on action 0: the sample really spreads; std = exp(-20) on action 1: u is mu
        assert np.abs(d["u"][:, 0] - d["mu"][:, 0]).max() > 3.0
        assert np.abs(d["u"][:, 1] - d["mu"][:, 1]).max() < 1e-6
    finally:
        sac.close()
        env.close()


def test_logp_is_finite_where_tanh_saturates(gm):
    if not gpu_available():
        pytest.skip("no GPU")
    env = make_env(gm)

    def edit(sd):
        sd["pi.mu_layer.bias"][0] = 12.0
        sd["pi.mu_layer.bias"][1] = -12.0
    sac, d = crafted(gm, env, edit)
    try:
        # tanh rounded to +-1 (f32 tanh is +-1 from |u| of about 9; std is about 1, so most envs are there)
        assert (d["act"][:, 0] == 1.0).sum() > N // 2 and (d["act"][:, 1] == -1.0).sum() > N // 2
        assert np.abs(d["act"]).max() <= 1.0
        assert np.isfinite(d["logp"]).all()
        ref = reference(gm, env, sac, env.observation(), d, 1.0)
        assert_within(d, ref, ("mu", "log_std", "u", "act", "logp"), "saturated tanh")
    finally:
        sac.close()
        env.close()


def test_params_round_trip(gm):
    """set_params (flat or state dict) -> get_params / state_dict / get_packed: the device holds
    pack()'s blob and hands the flat order back bit for bit (the stacked head unstacked)."""
    if not gpu_available():
        pytest.skip("no GPU")
    from gmx.sac import DeviceSAC, flat_to_state_dict, init_params, pack
    env = make_env(gm)
    sac = DeviceSAC(env, hidden=(20, 7), seed=1)
    try:
        flat = init_params(sac.pi_sizes, sac.q_sizes, seed=8)
        assert len(np.unique(flat)) > flat.size // 2
        sac.set_params(flat_to_state_dict(sac.pi_sizes, sac.q_sizes, flat))
        np.testing.assert_array_equal(sac.params, flat)
        np.testing.assert_array_equal(sac.get_params(), flat)
        np.testing.assert_array_equal(sac.get_packed(), pack(sac.pi_sizes, sac.q_sizes, flat)[0])
        sd = sac.state_dict()
        want = flat_to_state_dict(sac.pi_sizes, sac.q_sizes, flat)
        assert list(sd) == list(want)
        for k in want:
            np.testing.assert_array_equal(sd[k], want[k], err_msg=k)
    finally:
        sac.close()
        env.close()
